// enhance.hip — Enhance-A-Video (Luo et al. 2025; "FETA" in the Wan / HunyuanVideo / CogVideoX wrappers) for the visual blocks' self-attention:
// the cross-frame attention score of one forward and block, and the in-place scale of the attention output by it.  The rule is written once in
// include/k5.h (k5_enhance_scores_bf16).
//   enhance_scores_kernel   q | k after norm_qk + RoPE -> part[p][h] = sum over the T queries of one spatial column of their off-diagonal softmax mass
//   enhance_finish_kernel   part -> score = max(1, mean * (T + weight)), float64, fixed order, one workgroup
//   scale_by_dev_kernel     x = bf16(float(x) * score), 16 bytes per lane, grid-stride; a workgroup that reads score == 1 returns at once
#include "k5_common.h"
#include "k5_kernels.h"

namespace {

inline int done() { return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP; }

K5_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One workgroup per spatial position p, its four waves walk the heads h = wave, wave + 4, ..: together they read the column's T token rows in
// full.  One wave holds the column's T x T logits of one head as K·Qᵀ in NT x NT accumulator tiles of v_mfma_f32_32x32x16_bf16 (NT = 1: T <= 32,
// NT = 2: T <= 64): the query t is the accumulator's column (the lane), the key u its row (the registers and the lane half), so the softmax of
// a query is a reduction over a lane's registers and one exchange with lane ^ 32, as in attn_fwd.hip.
// Operands straight from memory, no LDS: lane (r = lane & 31, hf = lane >> 5) of row tile i owns token row 32 i + r and loads its 64 bytes
// d = 32 hf .. 32 hf + 31 of the head as four 16-byte fragments; fragment s is k-step s of both operands.  That is a permutation of the head
// dimension inside the dot product (logical k = 16 s + 8 hf + j is d = 32 hf + 8 s + j), the same one for q and k, so the product is unchanged
// and a lane reads one contiguous 64-byte piece of its row.
// Padding: a lane whose frame 32 i + r is >= T loads nothing (its fragments are zero and frame_rows is not read for it).  A padded key row gets
// the logit -inf, so it adds exactly 0 to every sum; a padded query column is all-finite (zero logits) and is left out of the column's sum.
// Order of the sums (the same on every launch): the row maximum and the two sums of a query walk the key tiles and registers in ascending
// order, then add the other lane half's; the column's T ratios are added in float64 by the xor butterfly.
template <int NT>
__global__ __launch_bounds__(256) void enhance_scores_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, int ldq, int ldk, int Hh,
                                                             int T, int S, const int32_t* __restrict__ frame_rows, float qk_scale,
                                                             double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int p = blockIdx.x;
  bool have[NT];
  int64_t row[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int t = 32 * i + r;
    have[i] = t < T;
    row[i] = 0;
    if (have[i]) row[i] = frame_rows ? (int64_t)frame_rows[(int64_t)p * T + t] : (int64_t)t * S + p;
  }
  // per lane and accumulator register, as numbers (so that they live in vector registers, not as 32 lane masks in scalar ones): the last key
  // tile's pad term (0, or -inf from frame T on; the tiles before it have no padding) and the diagonal tile's weights (key == query: 1 | 0)
  float padb[16], dgw[16], ofw[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    padb[g] = 32 * (NT - 1) + mfma32_row(g, lane) < T ? 0.0f : -INFINITY;
    dgw[g] = mfma32_row(g, lane) == r ? 1.0f : 0.0f;
    ofw[g] = 1.0f - dgw[g];
  }
  for (int h = wave; h < Hh; h += 4) {
    bf16x8 qf[NT][4], kf[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
        if (have[i]) {
          a = *reinterpret_cast<const u32x4*>(Q + row[i] * ldq + h * 64 + 32 * hf + 8 * s);
          b = *reinterpret_cast<const u32x4*>(K + row[i] * ldk + h * 64 + 32 * hf + 8 * s);
        }
        qf[i][s] = __builtin_bit_cast(bf16x8, a);
        kf[i][s] = __builtin_bit_cast(bf16x8, b);
      }
    }
    double col = 0.0;   // the off-diagonal mass of this lane's queries (lane half 0 only: both halves hold the same)
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      f32x16 z[NT];
#pragma unroll
      for (int ui = 0; ui < NT; ++ui) {
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma32(kf[ui][s], qf[ti][s], acc);
        z[ui] = acc;
      }
      float m = -INFINITY;
#pragma unroll
      for (int ui = 0; ui < NT; ++ui) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          z[ui][g] = ui == NT - 1 ? fmaf(z[ui][g], qk_scale, padb[g]) : z[ui][g] * qk_scale;   // one rounding either way (the pad term is 0 or -inf)
          m = fmaxf(m, z[ui][g]);
        }
      }
      m = fmaxf(m, __shfl_xor(m, 32, 64));   // finite: key 0 is never padded
      float off = 0.f, diag = 0.f;
#pragma unroll
      for (int ui = 0; ui < NT; ++ui) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const float e = __builtin_amdgcn_exp2f(z[ui][g] - m);
          if (ui == ti) { diag = fmaf(e, dgw[g], diag); off = fmaf(e, ofw[g], off); }   // exact: the weights are 0 and 1
          else off += e;
        }
      }
      off += __shfl_xor(off, 32, 64);
      diag += __shfl_xor(diag, 32, 64);
      const float ratio = off / (off + diag);
      if (hf == 0 && have[ti]) col += (double)ratio;
    }
    col = wave_sum_f64(col);
    if (lane == 0) part[(int64_t)p * Hh + h] = col;
  }
}

// score = max(1, mean * (T + weight)) with mean = sum(part) / (T (T - 1) n), everything float64: thread g adds part[g], part[g + 256], .. in
// ascending order, thread 0 the 256 group sums in group order (the arrangement of guidance_finish_kernel).  A NaN mean is handed through.
__global__ __launch_bounds__(256) void enhance_finish_kernel(const double* __restrict__ part, int64_t n, int T, float weight,
                                                             float* __restrict__ score_out) {
  __shared__ double red[256];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) a += part[i];
  red[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += red[i];
    const double mean = t / ((double)T * (double)(T - 1)) / (double)n;
    const double s = mean * ((double)T + (double)weight);
    score_out[0] = (float)(s < 1.0 ? 1.0 : s);
  }
}

// x[row][0 .. D) *= *score in place: bf16(float(x) * s), nearest-even, one rounded product.  s == 1 is x itself for every finite x, so such a
// workgroup leaves memory alone (NaN payloads and -0 stay what they were).
__global__ __launch_bounds__(256) void scale_by_dev_kernel(bf16_t* __restrict__ x, int64_t total, int nch, int ld, const float* __restrict__ score) {
  const float s = *score;
  if (s == 1.0f) return;
  const bool flat = ld == 8 * nch;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    int64_t off = g * 8;
    if (!flat) { const int64_t row = g / nch; off = row * ld + (g - row * nch) * 8; }
    u32x4 v = *reinterpret_cast<const u32x4*>(x + off);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float lo = __fmul_rn(__uint_as_float(v[j] << 16), s), hi = __fmul_rn(__uint_as_float(v[j] & 0xffff0000u), s);
      v[j] = pack_bf16x2(lo, hi);
    }
    *reinterpret_cast<u32x4*>(x + off) = v;
  }
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

long long k5_enhance_parts(int Hh, int S) { return (Hh < 1 || S < 1) ? 0 : (long long)Hh * S; }

int k5_launch_enhance_scores(const void* Q, const void* K, int ldq, int ldk, int Hh, int T, int S, const int32_t* frame_rows, float qk_scale,
                             float weight, double* part, float* score_out, hipStream_t stream) {
  if (!Q || !K || !part || !score_out || misaligned16(Q) || misaligned16(K) || (reinterpret_cast<uintptr_t>(part) & 7) ||
      (reinterpret_cast<uintptr_t>(score_out) & 3) || (reinterpret_cast<uintptr_t>(frame_rows) & 3))
    return K5_ERR_ARG;
  if (Hh < 1 || S < 1 || T < 2 || (int64_t)ldq < 64 * (int64_t)Hh || (int64_t)ldk < 64 * (int64_t)Hh || (ldq & 7) || (ldk & 7)) return K5_ERR_ARG;
  if (!(weight >= 0.0f) || !__builtin_isfinite(weight) || !(qk_scale > 0.0f) || !__builtin_isfinite(qk_scale)) return K5_ERR_ARG;
  if (T > 64) return K5_ERR_UNSUPPORTED;   // four 32 x 32 accumulators per wave
  if (T <= 32)
    hipLaunchKernelGGL(enhance_scores_kernel<1>, dim3(S), dim3(256), 0, stream, (const bf16_t*)Q, (const bf16_t*)K, ldq, ldk, Hh, T, S, frame_rows,
                       qk_scale, part);
  else
    hipLaunchKernelGGL(enhance_scores_kernel<2>, dim3(S), dim3(256), 0, stream, (const bf16_t*)Q, (const bf16_t*)K, ldq, ldk, Hh, T, S, frame_rows,
                       qk_scale, part);
  hipLaunchKernelGGL(enhance_finish_kernel, dim3(1), dim3(256), 0, stream, part, (int64_t)k5_enhance_parts(Hh, S), T, weight, score_out);
  return done();
}

int k5_launch_scale_by_dev(void* x, int rows, int D, int ld, const float* score_dev, hipStream_t stream) {
  if (!x || !score_dev || rows <= 0 || D <= 0 || ld < D) return K5_ERR_ARG;
  if ((D & 7) || (ld & 7) || misaligned16(x) || (reinterpret_cast<uintptr_t>(score_dev) & 3)) return K5_ERR_ARG;
  const int64_t total = (int64_t)rows * (D >> 3);
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(scale_by_dev_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, stream, (bf16_t*)x, total, D >> 3, ld,
                     score_dev);
  return done();
}
