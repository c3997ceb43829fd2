// small_ops.hip — HBM-bound elementwise / normalisation kernels and the fp32 "island" ops of the
// Kandinsky-5 DiT for gfx950.  All bf16 traffic is 16 B per lane (8 x bf16), coalesced over the
// feature axis; row statistics are wave-level (64-lane) shuffles.  Reference call sites:
//   apply_scale_shift_norm  kandinsky/models/nn.py:25-28      -> ln_modulate_kernel     (K1)
//   apply_gate_sum          nn.py:30-33                        -> gate_sum_kernel        (K2)
//   MagCache calibration    residual + norm ratio / cosine distance against the slot's previous residual -> magcache_stats_kernel
//   norm_qk + apply_rotary  nn.py:193-197, 35-40               -> rmsnorm_rope_kernel    (K5+K3)
//   Modulation / TimeEmbeddings linears (fp32 islands) nn.py:56-61,161-164 -> gemv_f32_kernel
//   TimeEmbeddings sinusoid nn.py:57-58                        -> time_features_kernel
//   TextEmbeddings.norm     nn.py:67,72                        -> ln_affine_kernel       (K13)
//   VisualEmbeddings patchify nn.py:81-95 (+ fractal_flatten models/utils.py:31-41) -> patchify_kernel
//   OutLayer un-patchify    nn.py:384-399 (+ fractal_unflatten :44-51)             -> unpatchify_kernel
//   CFG combine + Euler     generation_utils.py:74-76,128      -> euler_step_kernel      (K18)
//   RoPE1D/RoPE3D tables    nn.py:99-150                        -> rope_table_kernel      (K15)
//   stochastic step noise   (none: the reference's loop is the ODE step)   -> philox_normal4 inside euler_step_kernel, noise_normal_kernel
#include <stdlib.h>

#include "k5_common.h"
#include "k5_kernels.h"

namespace {

constexpr int MAXC = 4;  // 16-B chunks per lane per row: D <= 64*8*4 = 2048

// ---------------------------------------------------------------------------------------------
// K1: one wave per row.  Round 6: the per-column vectors (scale + 1 | shift, or weight | bias) are staged ONCE per workgroup in LDS — until
// round 5 every row re-read both vectors from L1 (14 KB of fp32 per 3.5-KB row at D = 1792: two thirds of the bytes the texture path moved).
// 76 -> 64 us per call at 47 616 x 1792 (4.5 -> 5.4 TB/s, profiles/r06_ln_rows_ab.log).  A wave may walk several rows (`4 gridDim` apart;
// K5_LN_WG caps the grid) but one row per wave measured best: 5.36 TB/s against 4.7-5.2 with 512-4096 workgroups.  Same operations in the same
// order per row: the bits do not change.  (All four 16-B loads of a row are issued in one burst ahead of the arithmetic: the same kernel with the
// loads inside the chunk loop ran at 4.1 TB/s, profiles/r06_ln_rows_ab.log second table.)
template <bool AFFINE>
__global__ __launch_bounds__(256) void ln_kernel(const bf16_t* __restrict__ x, const float* __restrict__ a,
                                                 const float* __restrict__ b, bf16_t* __restrict__ out,
                                                 float* __restrict__ out_f32, int rows, int D, int ldx, int ldo,
                                                 uint8_t* __restrict__ out8 = nullptr) {   // e4m3(bf16(.)), static scale 1, row stride D (fp8 modes of the engine)
  // [a | b][half 0 | half 1][chunk][4]: a lane's two 16-B halves of a chunk sit in two planes, so that consecutive lanes read consecutive
  // 16 B (conflict-free ds_read_b128)
  __shared__ __attribute__((aligned(16))) float vec[2][2][64 * MAXC][4];
  const int lane = threadIdx.x & 63;
  const int nch = D >> 3;
  for (int c = threadIdx.x; c < 2 * nch; c += 256) {       // c = 2 chunk + half
    const f32x4 av = *reinterpret_cast<const f32x4*>(a + 4 * c), bv = *reinterpret_cast<const f32x4*>(b + 4 * c);
    *reinterpret_cast<f32x4*>(vec[0][c & 1][c >> 1]) = AFFINE ? av : f32x4{av[0] + 1.0f, av[1] + 1.0f, av[2] + 1.0f, av[3] + 1.0f};   // K1: scale + 1
    *reinterpret_cast<f32x4*>(vec[1][c & 1][c >> 1]) = bv;
  }
  __syncthreads();
  const int stride = 4 * gridDim.x;
  int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  u32x4 raw[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i)
    if (lane + 64 * i < nch) raw[i] = *reinterpret_cast<const u32x4*>(x + (size_t)row * ldx + 8 * (lane + 64 * i));
  for (; row < rows; row += stride) {
    float v[MAXC][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      if (lane + 64 * i < nch) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[i][2 * j] = __uint_as_float(raw[i][j] << 16);
          v[i][2 * j + 1] = __uint_as_float(raw[i][j] & 0xffff0000u);
          sum += v[i][2 * j] + v[i][2 * j + 1];
        }
      }
    }
    const int nrow = row + stride;
    if (nrow < rows) {   // (a capped grid) the next row of this wave: in flight under this row's arithmetic and stores
#pragma unroll
      for (int i = 0; i < MAXC; ++i)
        if (lane + 64 * i < nch) raw[i] = *reinterpret_cast<const u32x4*>(x + (size_t)nrow * ldx + 8 * (lane + 64 * i));
    }
    const float mean = wave_sum(sum) / (float)D;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      if (lane + 64 * i < nch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; sq += d * d; }
      }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)D + 1e-5f);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int ch = lane + 64 * i;
      if (ch < nch) {
        float o[8];
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(vec[0][0][ch]), a1 = *reinterpret_cast<const f32x4*>(vec[0][1][ch]);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(vec[1][0][ch]), b1 = *reinterpret_cast<const f32x4*>(vec[1][1][ch]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float n = (v[i][j] - mean) * rstd;
          const float aj = j < 4 ? a0[j] : a1[j - 4], bj = j < 4 ? b0[j] : b1[j - 4];
          // K1: n * (scale + 1) + shift ; K13: n * weight + bias
          o[j] = __fadd_rn(__fmul_rn(n, aj), bj);
        }
        if (out) {
          u32x4 pk = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
          *reinterpret_cast<u32x4*>(out + (size_t)row * ldo + 8 * ch) = pk;
        }
        if (out_f32) {
#pragma unroll
          for (int j = 0; j < 8; ++j) out_f32[(size_t)row * D + 8 * ch + j] = bf_round(o[j]);
        }
        if (out8) {   // what k5_launch_quant_rows_fp8 (static scale) makes of the bf16 row: the bf16 rounding first, then the saturating e4m3 one
          uint2 q8;
          q8.x = pack_fp8x4(bf_round(o[0]), bf_round(o[1]), bf_round(o[2]), bf_round(o[3]));
          q8.y = pack_fp8x4(bf_round(o[4]), bf_round(o[5]), bf_round(o[6]), bf_round(o[7]));
          *reinterpret_cast<uint2*>(out8 + (size_t)row * D + 8 * ch) = q8;
        }
      }
    }
  }
}

// workgroups of a launch: one wave per row unless K5_LN_WG caps the grid (A/B: a wave then walks several rows)
inline int ln_grid(int rows) {
  static const int cap = getenv("K5_LN_WG") ? atoi(getenv("K5_LN_WG")) : 0x7fffffff;
  const int wg = (rows + 3) / 4;
  return wg < cap ? wg : cap;
}

// ---------------------------------------------------------------------------------------------
// K5 + K3: one thread per 16-B chunk (8 of the 64 head elements); 8-lane groups own one head.  Grid-stride over rows with a
// stride that is a multiple of H*8 threads, so a thread keeps its (head, chunk) and can carry the head's running
// max |x|^2 in a register: one atomic per 8-lane group per launch instead of one per head vector.
// MEANS (round 4, NABLA): the pass also leaves the 64-token BLOCK MEANS of the heads' unscaled, normalised + rotated values — what
// block_mean_kernel (nabla.hip) computed by reading q | k once more: fp32 sum of the bf16-rounded values in row order, x 1/64, one bf16 rounding
// (the reference's bf16 `.mean(-2)`, utils.py:140-143).  A thread then walks whole blocks of 64 CONSECUTIVE rows (block bb = slot, slot + S, ...)
// instead of rows `stride` apart, so the sums stay in its registers; heads < scale_from_head go to mean_q [head][mq_stride blocks][64], the others
// to mean_k [head - scale_from_head][mk_stride][64].  With the means taken here the unscaled keys need not be stored: scaled in place.
template <bool MEANS>
__global__ __launch_bounds__(256) void rmsnorm_rope_kernel(bf16_t* __restrict__ x, const float* __restrict__ weight,
                                                           const float* __restrict__ cosT, const float* __restrict__ sinT,
                                                           int rows, int H, int heads_per_weight, int ld, int rope_heads,
                                                           float out_scale, int scale_from_head, bf16_t* __restrict__ scaled_out,
                                                           int ld_scaled, float* __restrict__ stats, const float* __restrict__ centre,
                                                           bf16_t* __restrict__ mean_q, int mq_stride, bf16_t* __restrict__ mean_k, int mk_stride) {
  // stats: per-head maxima of this block: |x_h|^2 for the H heads of a row, then (centre given) |k'_h - c_h|^2 for the scaled heads —
  // the radius of a head's keys around the centre key_centre_kernel estimated; H + (H - scale_from_head) <= 256 entries
  __shared__ unsigned int smax[256];
  if (stats) { smax[threadIdx.x] = 0u; __syncthreads(); }
  const int64_t total = (int64_t)rows * H * 8;
  const int64_t stride = (int64_t)gridDim.x * 256;        // multiple of H * 8 (launcher)
  const int64_t g0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(g0 & 7);
  const int head = (int)((g0 >> 3) % H);
  const float* w = weight + (head / heads_per_weight) * 64 + 8 * c;
  float wv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) wv[j] = w[j];
  const bool rope = cosT && head < rope_heads;
  const bool scaled = head >= scale_from_head;
  float n2max = 0.f, r2max = 0.f;
  float msum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float cv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool centred = stats && centre && scaled;
  if (centred) {
#pragma unroll
    for (int j = 0; j < 8; ++j) cv[j] = centre[(head - scale_from_head) * 64 + 8 * c + j];
  }
  // every lane of a wave runs the same number of iterations except in the last one (shuffles need the whole 8-lane group:
  // groups never straddle the end because total is a multiple of 8)
  const int slot0 = (int)(g0 / (H * 8)), nslot = (int)(stride / (H * 8)), nblk = rows >> 6;
  // MEANS: iteration i = (block, t): block = slot0 + (i / 64) * nslot, row = 64 block + t; otherwise row i of this thread's stride
  // MEANS: the NEXT row's 16 bytes are requested before this row is worked on and stored (the compiler cannot move a load of x above a store
  // to x by itself): two loads in flight per thread — with whole 64-row blocks per thread the launch is a little over one round of resident
  // workgroups, and one load per thread did not keep HBM busy through its second round
  // (Round 6: the same prefetch in the dense form — rows `stride` apart, ~20 per thread at 47 616 tokens — measured SLOWER: 154 us against 142-144,
  // profiles/r06_elem_ab.log; seven waves per SIMD with one load each already cover the latency, the second load only adds to the queue.)
  u32x4 raw_pf = {0u, 0u, 0u, 0u};
  if (MEANS && slot0 < nblk) raw_pf = *reinterpret_cast<const u32x4*>(x + (size_t)(64 * slot0) * ld + head * 64 + 8 * c);
  for (int64_t g = g0, it = 0; MEANS ? (slot0 + (int)(it >> 6) * nslot < nblk) : (g < total); g += stride, ++it) {
    const int mblk = MEANS ? slot0 + (int)(it >> 6) * nslot : 0, mt = (int)(it & 63);
    const int row = MEANS ? 64 * mblk + mt : (int)((g >> 3) / H);
    bf16_t* px = x + (size_t)row * ld + head * 64 + 8 * c;
    u32x4 raw;
    if (MEANS) {
      raw = raw_pf;
      const int nblk_next = slot0 + (int)((it + 1) >> 6) * nslot;
      if (nblk_next < nblk) raw_pf = *reinterpret_cast<const u32x4*>(x + (size_t)(64 * nblk_next + (int)((it + 1) & 63)) * ld + head * 64 + 8 * c);
    } else {
      raw = *reinterpret_cast<const u32x4*>(px);
    }
    float v[8];
    float sq = 0.f;
    // The sum of squares with its operations SPELLED OUT (round 6) — what the compiler made of `sq += lo * lo + hi * hi` in both instantiations of this
    // kernel (a pair is fma(hi, hi, lo * lo); the pairs added in order; the eight chunks of a head as a tree; fma(sq, 1/64, eps)) — because the
    // attention kernel's fused query norm (attn_fwd.hip, K5QueryNorm) restates it and contraction had picked fma(lo, lo, hi * hi) there: 1 (row, head) in
    // 10^4 then got another last bit of 1 / rms and, now and then, another bf16 rounding of a query element.  Same bits as before here.
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = __uint_as_float(raw[j] << 16);
      v[2 * j + 1] = __uint_as_float(raw[j] & 0xffff0000u);
      sq = __fadd_rn(sq, fmaf(v[2 * j + 1], v[2 * j + 1], __fmul_rn(v[2 * j], v[2 * j])));
    }
    sq = __fadd_rn(sq, __shfl_xor(sq, 1, 64));
    sq = __fadd_rn(sq, __shfl_xor(sq, 2, 64));
    sq = __fadd_rn(sq, __shfl_xor(sq, 4, 64));
    const float rs = rsqrtf(fmaf(sq, 1.0f / 64.0f, 1.1920928955078125e-07f));  // eps = finfo(fp32).eps
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = bf_round(__fmul_rn(__fmul_rn(v[j], rs), wv[j]));  // .type_as(q)
    if (rope) {
      const f32x4 cs = *reinterpret_cast<const f32x4*>(cosT + (size_t)row * 32 + 4 * c);
      const f32x4 sn = *reinterpret_cast<const f32x4*>(sinT + (size_t)row * 32 + 4 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // __fmul_rn / __fadd_rn are plain * and + to this compiler (no OCML_BASIC_ROUNDED_OPERATIONS): under -ffp-contract=fast ONE of the two products
        // of a rotation is fused into the add, and which one is the compiler's choice per kernel.  Spelled out (round 6) as what both instantiations of
        // this kernel had: the product with the ODD element rounded, the one with the even element fused — the form the attention kernel's fused query
        // norm restates (it had the other one: 7 (row, head) pairs in 10^4 got another bf16 rounding of one query element).  Same bits as before here.
        const float x0 = y[2 * j], x1 = y[2 * j + 1];
        y[2 * j] = fmaf(cs[j], x0, -__fmul_rn(sn[j], x1));
        y[2 * j + 1] = fmaf(sn[j], x0, __fmul_rn(cs[j], x1));
      }
    }
    if (MEANS) {
      if (mt == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) msum[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) msum[j] += bf_round(y[j]);       // the bf16 values the unscaled tensor holds (held), in row order
      if (mt == 63) {
        const u32x4 mk = {pack_bf16x2(msum[0] * (1.f / 64), msum[1] * (1.f / 64)), pack_bf16x2(msum[2] * (1.f / 64), msum[3] * (1.f / 64)),
                          pack_bf16x2(msum[4] * (1.f / 64), msum[5] * (1.f / 64)), pack_bf16x2(msum[6] * (1.f / 64), msum[7] * (1.f / 64))};
        bf16_t* mo = head < scale_from_head ? (mean_q ? mean_q + ((size_t)head * mq_stride + mblk) * 64 + 8 * c : nullptr)
                                            : (mean_k ? mean_k + ((size_t)(head - scale_from_head) * mk_stride + mblk) * 64 + 8 * c : nullptr);
        if (mo) *reinterpret_cast<u32x4*>(mo) = mk;
      }
    }
    u32x4 pks = {0u, 0u, 0u, 0u};
    if (scaled) {   // keys handed to the pre-scaled softmax: k' = bf16(log2(e)/8 * k), one rounding
      if (scaled_out) {   // NABLA: the unscaled keys stay in place (block map), the scaled copy goes to its own buffer
        pks = u32x4{pack_bf16x2(__fmul_rn(y[0], out_scale), __fmul_rn(y[1], out_scale)), pack_bf16x2(__fmul_rn(y[2], out_scale), __fmul_rn(y[3], out_scale)),
                    pack_bf16x2(__fmul_rn(y[4], out_scale), __fmul_rn(y[5], out_scale)), pack_bf16x2(__fmul_rn(y[6], out_scale), __fmul_rn(y[7], out_scale))};
        *reinterpret_cast<u32x4*>(scaled_out + (size_t)row * ld_scaled + (head - scale_from_head) * 64 + 8 * c) = pks;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = __fmul_rn(y[j], out_scale);
      }
    }
    const u32x4 pk = {pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]), pack_bf16x2(y[4], y[5]), pack_bf16x2(y[6], y[7])};
    *reinterpret_cast<u32x4*>(px) = pk;
    if (stats) {   // |x|^2 of the bf16 values the softmax will consume (the scaled copy where there is one)
      const u32x4 src = (scaled && scaled_out) ? pks : pk;
      float n2 = 0.f, r2 = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float lo = __uint_as_float(src[j] << 16), hi = __uint_as_float(src[j] & 0xffff0000u);
        n2 += lo * lo + hi * hi;
        if (centred) { const float dl = lo - cv[2 * j], dh = hi - cv[2 * j + 1]; r2 += dl * dl + dh * dh; }
      }
      n2 += __shfl_xor(n2, 1, 64);   // the head vector's 8 lanes
      n2 += __shfl_xor(n2, 2, 64);
      n2 += __shfl_xor(n2, 4, 64);
      n2max = n2 == n2 ? fmaxf(n2max, n2) : __uint_as_float(0x7f800000u);   // NaN -> +inf: forces the online-max path
      if (centred) {
        r2 += __shfl_xor(r2, 1, 64);
        r2 += __shfl_xor(r2, 2, 64);
        r2 += __shfl_xor(r2, 4, 64);
        r2max = r2 == r2 ? fmaxf(r2max, r2) : __uint_as_float(0x7f800000u);
      }
    }
  }
  // per-head max over the rows of this call: |q.k'| <= |q| |k'| then bounds every exp2 argument of the head
  // (attn_flags_kernel).  Non-negative floats order like their bit patterns.  No global atomics (a hundred thousand of them on
  // 28 addresses cost more than the kernel): LDS max per block, one partial row per block, reduced by stats_reduce_kernel.
  if (stats) {
    const int Hs = centre ? H + (H - scale_from_head) : H;
    if (c == 0 && (MEANS ? slot0 < nblk : g0 < total)) {
      atomicMax(&smax[head], __float_as_uint(n2max));
      if (centred) atomicMax(&smax[H + head - scale_from_head], __float_as_uint(r2max));
    }
    __syncthreads();
    if ((int)threadIdx.x < Hs) stats[(size_t)blockIdx.x * Hs + threadIdx.x] = __uint_as_float(smax[threadIdx.x]);
  }
}

// Centre of a head's keys for the centred Cauchy-Schwarz bound of the attention's per-row softmax offsets (attn_fwd.hip, AttnP::kcentre):
// c_h = mean of k'_j over a strided SAMPLE of the rows — any vector is a valid centre for the upper bound q.k' <= q.c + |q| max|k' - c|, and
// a convex combination of actual keys also gives the lower bound max_j q.k'_j >= q.c that rules the row-sum underflow out.  Runs BEFORE
// rmsnorm_rope_kernel on the raw projection, with that kernel's arithmetic (RMSNorm, weight, bf16, RoPE, scale, bf16), so that the main
// kernel can take max|k' - c|^2 in its one pass.  One block per key head: thread = (sample lane t >> 3, 16-B chunk t & 7); fixed-order sums.
// Sample size: ANY convex combination of keys is a valid centre; what the sample has to catch is a component the head's keys share, and
// 256 rows spread over the sequence do.  The kernel is one workgroup per head with a serial chain of row loads per thread — 1024 rows
// measured 56 us per block (+1.8 ms per step, same-box A/B against attn_row_offsets = 0: 544.3 vs 542.0 ms), 8 iterations instead of 32.
constexpr int K5_CENTRE_SAMPLE = 256;
__global__ __launch_bounds__(256) void key_centre_kernel(const bf16_t* __restrict__ x, const float* __restrict__ weight,
                                                         const float* __restrict__ cosT, const float* __restrict__ sinT, int rows, int ld,
                                                         int head0, int heads_per_weight, int rope_heads, float out_scale, int nsample,
                                                         float* __restrict__ centre) {
  __shared__ float part[32][64];
  const int hk = blockIdx.x, head = head0 + hk, c = threadIdx.x & 7, sl = threadIdx.x >> 3;
  const float* w = weight + (head / heads_per_weight) * 64 + 8 * c;
  float wv[8], acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { wv[j] = w[j]; acc[j] = 0.f; }
  const bool rope = cosT && head < rope_heads;
  // every row this thread samples is requested BEFORE any of them is worked on (round 5: the serial chain of 8 dependent row loads was 10.9 us per
  // block at 3328 tokens — a launch that costs one memory round trip instead of eight); same values summed in the same order
  constexpr int NIT = K5_CENTRE_SAMPLE / 32;
  u32x4 raws[NIT]; f32x4 csv[NIT], snv[NIT]; int rowv[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = it * 32 + sl;
    const bool live = i < nsample;
    rowv[it] = (int)(((long long)(live ? i : 0) * rows) / nsample);
    raws[it] = *reinterpret_cast<const u32x4*>(x + (size_t)rowv[it] * ld + head * 64 + 8 * c);
    if (rope) {
      csv[it] = *reinterpret_cast<const f32x4*>(cosT + (size_t)rowv[it] * 32 + 4 * c);
      snv[it] = *reinterpret_cast<const f32x4*>(sinT + (size_t)rowv[it] * 32 + 4 * c);
    }
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = it * 32 + sl;
    const bool live = i < nsample;
    const u32x4 raw = raws[it];
    float v[8], sq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = __uint_as_float(raw[j] << 16);
      v[2 * j + 1] = __uint_as_float(raw[j] & 0xffff0000u);
      sq += v[2 * j] * v[2 * j] + v[2 * j + 1] * v[2 * j + 1];
    }
    sq += __shfl_xor(sq, 1, 64);
    sq += __shfl_xor(sq, 2, 64);
    sq += __shfl_xor(sq, 4, 64);
    const float rs = rsqrtf(sq * (1.0f / 64.0f) + 1.1920928955078125e-07f);
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = bf_round(__fmul_rn(__fmul_rn(v[j], rs), wv[j]));
    if (rope) {
      const f32x4 cs = csv[it], sn = snv[it];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x0 = y[2 * j], x1 = y[2 * j + 1];
        y[2 * j] = __fadd_rn(__fmul_rn(cs[j], x0), __fmul_rn(-sn[j], x1));
        y[2 * j + 1] = __fadd_rn(__fmul_rn(sn[j], x0), __fmul_rn(cs[j], x1));
      }
    }
    if (live)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += bf_round(__fmul_rn(y[j], out_scale));
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[sl][8 * c + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < 64) {
    float s = 0.f;
    for (int l = 0; l < 32; ++l) s += part[l][threadIdx.x];
    centre[hk * 64 + threadIdx.x] = s / (float)nsample;
  }
}

// out[h] = max(out[h], max over the nblk partial rows): a few blocks, each over a slice of the rows (thread t: head t % H, row
// lane t / H), then one atomic per head and block — a handful, not one per head vector
__global__ __launch_bounds__(256) void stats_reduce_kernel(const float* __restrict__ part, int nblk, int H, float* __restrict__ out) {
  __shared__ float red[256];
  const int per = 256 / H;                  // row lanes per head
  const int h = threadIdx.x % H, lane = threadIdx.x / H;
  const int b0 = (int)((long long)nblk * blockIdx.x / gridDim.x), b1 = (int)((long long)nblk * (blockIdx.x + 1) / gridDim.x);
  float m = 0.f;
  if (lane < per)
    for (int b = b0 + lane; b < b1; b += per) { const float v = part[(size_t)b * H + h]; m = v == v ? fmaxf(m, v) : __uint_as_float(0x7f800000u); }
  red[threadIdx.x] = lane < per ? m : 0.f;
  __syncthreads();
  if ((int)threadIdx.x < H) {
    float r = 0.f;
    for (int l = 0; l < per; ++l) r = fmaxf(r, red[l * H + threadIdx.x]);   // NaNs were mapped to +inf above
    atomicMax(reinterpret_cast<unsigned int*>(out) + threadIdx.x, __float_as_uint(r));
  }
}

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_sum_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ y,
                                                       const float* __restrict__ gate, bf16_t* __restrict__ out,
                                                       int64_t nchunks, int chunks_per_row) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < nchunks; g += (int64_t)gridDim.x * 256) {
    const int ch = (int)(g % chunks_per_row);
    const u32x4 rx = *reinterpret_cast<const u32x4*>(x + g * 8);
    const u32x4 ry = *reinterpret_cast<const u32x4*>(y + g * 8);
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gate + 8 * ch), g1 = *reinterpret_cast<const f32x4*>(gate + 8 * ch + 4);
    float o[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gl = j < 2 ? g0[2 * j] : g1[2 * j - 4], gh = j < 2 ? g0[2 * j + 1] : g1[2 * j - 3];
      o[2 * j] = __fadd_rn(__uint_as_float(rx[j] << 16), __fmul_rn(gl, __uint_as_float(ry[j] << 16)));
      o[2 * j + 1] = __fadd_rn(__uint_as_float(rx[j] & 0xffff0000u), __fmul_rn(gh, __uint_as_float(ry[j] & 0xffff0000u)));
    }
    u32x4 pk = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
    *reinterpret_cast<u32x4*>(out + g * 8) = pk;
  }
}

// ---------------------------------------------------------------------------------------------
// MagCache calibration (k5_launch_magcache_stats): res = bf16(vis - ori) — the operations of gate_sum_kernel with the -1 gate, so the bits of
// the residual MagCache caches — and, against the slot's previous residual, the per-row norm ratio rho = |res_i| / |prev_i| and cosine distance
// of the calibration script of the MagCache paper.  One wave per row (the ln_kernel shape); a lane's loads of up to MAXC chunks of vis | ori |
// prev are issued in one burst ahead of the arithmetic and the stores, which also makes res == ori safe (a lane reads a chunk of ori before it
// writes that chunk of res, and no other lane touches it).  Row sums of squares and the dot product are fp32 over the bf16 values of res AS
// STORED; everything across rows is float64 in a fixed order: a wave adds its rows in row order, thread 0 the workgroup's four waves in wave
// order into part[block][4], magcache_finish_kernel the blocks in index order.  No atomics: two launches give the same bits.
// Rows with |prev_i| = 0 or |res_i| = 0 have no ratio: left out of the three sums and of the count.
template <bool HAS_PREV>
__global__ __launch_bounds__(256) void magcache_stats_kernel(const bf16_t* vis, const bf16_t* ori, const bf16_t* __restrict__ prev,
                                                             bf16_t* res, double* __restrict__ part, int rows, int nch) {
  __shared__ double red[4][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};   // sum rho | sum rho^2 | sum (1 - cos) | rows counted (wave-uniform)
  for (int row = blockIdx.x * 4 + wave; row < rows; row += 4 * gridDim.x) {
    const size_t base = (size_t)row * nch * 8;
    float sr = 0.f, sp = 0.f, dp = 0.f;
    for (int c0 = 0; c0 < nch; c0 += 64 * MAXC) {
      u32x4 rv[MAXC], ro[MAXC], rp[MAXC];
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        const int ch = c0 + lane + 64 * i;
        if (ch < nch) {
          rv[i] = *reinterpret_cast<const u32x4*>(vis + base + 8 * ch);
          ro[i] = *reinterpret_cast<const u32x4*>(ori + base + 8 * ch);
          if (HAS_PREV) rp[i] = *reinterpret_cast<const u32x4*>(prev + base + 8 * ch);
        }
      }
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        const int ch = c0 + lane + 64 * i;
        if (ch < nch) {
          u32x4 pk;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            // x + (-1 * y), as gate_sum_kernel forms it
            const float lo = __fadd_rn(__uint_as_float(rv[i][j] << 16), __fmul_rn(-1.0f, __uint_as_float(ro[i][j] << 16)));
            const float hi = __fadd_rn(__uint_as_float(rv[i][j] & 0xffff0000u), __fmul_rn(-1.0f, __uint_as_float(ro[i][j] & 0xffff0000u)));
            pk[j] = pack_bf16x2(lo, hi);
            if (HAS_PREV) {
              const float rl = __uint_as_float(pk[j] << 16), rh = __uint_as_float(pk[j] & 0xffff0000u);
              const float pl = __uint_as_float(rp[i][j] << 16), ph = __uint_as_float(rp[i][j] & 0xffff0000u);
              sr = fmaf(rl, rl, sr); sr = fmaf(rh, rh, sr);
              sp = fmaf(pl, pl, sp); sp = fmaf(ph, ph, sp);
              dp = fmaf(rl, pl, dp); dp = fmaf(rh, ph, dp);
            }
          }
          *reinterpret_cast<u32x4*>(res + base + 8 * ch) = pk;
        }
      }
    }
    if (HAS_PREV) {
      sr = wave_sum(sr); sp = wave_sum(sp); dp = wave_sum(dp);   // xor butterfly: every lane holds the same bits
      if (sr > 0.f && sp > 0.f) {
        const double r2 = (double)sr / (double)sp;
        acc[0] += sqrt(r2);
        acc[1] += r2;
        acc[2] += 1.0 - (double)dp / sqrt((double)sr * (double)sp);
        acc[3] += 1.0;
      }
    }
  }
  if (HAS_PREV) {
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) part[(size_t)blockIdx.x * 4 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  }
}

// out[k] (+)= sum over the nblk partials of component k, in index order: thread (g, k) adds blocks g, g + 256, ... in that order, then thread k
// the 256 group sums in group order.  One workgroup.
__global__ __launch_bounds__(1024) void magcache_finish_kernel(const double* __restrict__ part, int nblk, double* __restrict__ out, int accumulate) {
  __shared__ double red[256][4];
  const int k = threadIdx.x & 3, g = threadIdx.x >> 2;
  double a = 0.0;
  for (int b = g; b < nblk; b += 256) a += part[(size_t)b * 4 + k];
  red[g][k] = a;
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += red[i][threadIdx.x];
    out[threadIdx.x] = accumulate ? out[threadIdx.x] + t : t;
  }
}

// ---------------------------------------------------------------------------------------------
// fp32 GEMV, one wave per output row (weights streamed once, 16 B per lane)
__global__ __launch_bounds__(256) void gemv_f32_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                       const float* __restrict__ b, float* __restrict__ y, int N, int K,
                                                       int silu_in, const float* __restrict__ add) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* w = W + (size_t)n * K;
  float acc = 0.f;
  for (int k = 4 * lane; k < K; k += 256) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + k);
    f32x4 xv = *reinterpret_cast<const f32x4*>(x + k);
    if (silu_in) {
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[j] = xv[j] / (1.0f + expf(-xv[j]));
    }
    acc += wv[0] * xv[0] + wv[1] * xv[1] + wv[2] * xv[2] + wv[3] * xv[3];
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    float r = acc + (b ? b[n] : 0.f);
    if (add) r += add[n];
    y[n] = r;
  }
}

// tvec / step: hipGraph-replayable form — the time is read from a device table at the device-side step counter
__global__ void time_features_kernel(float t, const float* __restrict__ tvec, const int* __restrict__ step, float* __restrict__ out, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = D / 2;
  if (i >= half) return;
  if (tvec) t = tvec[*step];
  // get_freqs(models/utils.py:21-28): exp(-ln(1e4) * i / half) in fp32
  const float f = expf(__fdiv_rn(__fmul_rn(-9.210340371976184f, (float)i), (float)half));
  const float a = __fmul_rn(t, f);
  out[i] = cosf(a);
  out[half + i] = sinf(a);
}

// cos/sin tables [ntok][32]: column j in [0,n0) uses axis 0 ... ; angle = pos * freq / scale
__global__ void rope_table_kernel(float* __restrict__ cosT, float* __restrict__ sinT, const int32_t* __restrict__ p0,
                                  const int32_t* __restrict__ p1, const int32_t* __restrict__ p2, int T, int H, int W,
                                  int n0, int n1, int n2, float s0, float s1, float s2, const int32_t* __restrict__ tok_perm) {
  const int np = n0 + n1 + n2;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)T * H * W * np;
  if (gid >= total) return;
  const int j = (int)(gid % np);
  const int64_t row = gid / np;
  const int64_t tok = tok_perm ? tok_perm[row] : row;
  const int w = (int)(tok % W), h = (int)((tok / W) % H), t = (int)(tok / ((int64_t)W * H));
  int pos, i, n;
  float sc;
  if (j < n0) { pos = p0[t]; i = j; n = n0; sc = s0; }
  else if (j < n0 + n1) { pos = p1[h]; i = j - n0; n = n1; sc = s1; }
  else { pos = p2[w]; i = j - n0 - n1; n = n2; sc = s2; }
  const float f = expf(__fdiv_rn(__fmul_rn(-9.210340371976184f, (float)i), (float)n));
  const float a = __fdiv_rn(__fmul_rn((float)pos, f), sc);
  cosT[gid] = cosf(a);
  sinT[gid] = sinf(a);
}

__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, int T, int H,
                                                       int W, int Cx, int Cin, int Kpad, const int32_t* __restrict__ tok_perm) {
  // one thread per output element of [Ntok][Kpad]; feature = (ph*2+pw)*Cin + c  (pt = 1)
  const int Hp = H / 2, Wp = W / 2;
  const int64_t total = (int64_t)T * Hp * Wp * Kpad;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int f = (int)(g % Kpad);
    const int64_t row = g / Kpad;
    float v = 0.f;
    if (f < 4 * Cin) {
      const int64_t tok = tok_perm ? tok_perm[row] : row;
      const int wp = (int)(tok % Wp), hp = (int)((tok / Wp) % Hp), t = (int)(tok / ((int64_t)Wp * Hp));
      const int c = f % Cin, pp = f / Cin, ph = pp >> 1, pw = pp & 1;
      if (c < Cx) v = x[(((int64_t)t * H + 2 * hp + ph) * W + 2 * wp + pw) * Cx + c];
    }
    out[g] = f2bf(v);
  }
}

__global__ __launch_bounds__(256) void patchify_cond_kernel(const float* __restrict__ x, const float* __restrict__ vc,
                                                            bf16_t* __restrict__ out, int T, int H, int W, int Cx, int Cin,
                                                            int Kpad, const int32_t* __restrict__ tok_perm) {
  // patchify_kernel on torch.cat([x, vc], -1) without the concatenation: channels [0, Cx) from the latent x (T,H,W,Cx), channels
  // [Cx, Cin) from the conditioning vc (T,H,W,Cin-Cx); same feature order, permutation, zero pad and RNE cast
  const int Hp = H / 2, Wp = W / 2, Cv = Cin - Cx;
  const int64_t total = (int64_t)T * Hp * Wp * Kpad;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int f = (int)(g % Kpad);
    const int64_t row = g / Kpad;
    float v = 0.f;
    if (f < 4 * Cin) {
      const int64_t tok = tok_perm ? tok_perm[row] : row;
      const int wp = (int)(tok % Wp), hp = (int)((tok / Wp) % Hp), t = (int)(tok / ((int64_t)Wp * Hp));
      const int c = f % Cin, pp = f / Cin, ph = pp >> 1, pw = pp & 1;
      const int64_t pix = ((int64_t)t * H + 2 * hp + ph) * W + 2 * wp + pw;
      v = c < Cx ? x[pix * Cx + c] : vc[pix * Cv + (c - Cx)];
    }
    out[g] = f2bf(v);
  }
}

__global__ __launch_bounds__(256) void patchify_view_kernel(const float* __restrict__ x, int64_t xf, int64_t xr,
                                                            const float* __restrict__ vc, int64_t vf, int64_t vr,
                                                            bf16_t* __restrict__ out, int T, int H, int W, int Cx, int Cin, int Kpad,
                                                            const int32_t* __restrict__ tok_perm) {
  // patchify_kernel / patchify_cond_kernel on a (T,H,W) box inside a larger tensor: x has frame stride xf and row stride xr (elements; a row's
  // cells are Cx apart), vc (nullable; then the channels [Cx, Cin) are zero) has vf, vr and cells Cin - Cx apart.  Reads only cells of the box.
  const int Hp = H / 2, Wp = W / 2, Cv = Cin - Cx;
  const int64_t total = (int64_t)T * Hp * Wp * Kpad;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int f = (int)(g % Kpad);
    const int64_t row = g / Kpad;
    float v = 0.f;
    if (f < 4 * Cin) {
      const int64_t tok = tok_perm ? tok_perm[row] : row;
      const int wp = (int)(tok % Wp), hp = (int)((tok / Wp) % Hp), t = (int)(tok / ((int64_t)Wp * Hp));
      const int c = f % Cin, pp = f / Cin, ph = pp >> 1, pw = pp & 1;
      const int r = 2 * hp + ph, col = 2 * wp + pw;
      if (c < Cx) v = x[(int64_t)t * xf + (int64_t)r * xr + (int64_t)col * Cx + c];
      else if (vc) v = vc[(int64_t)t * vf + (int64_t)r * vr + (int64_t)col * Cv + (c - Cx)];
    }
    out[g] = f2bf(v);
  }
}

__global__ __launch_bounds__(256) void unpatchify_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, int T,
                                                         int Hp, int Wp, int C, int ldx, const int32_t* __restrict__ tok_perm) {
  // x [Ntok][C*4] feature (c, ph, pw) -> out (T, 2Hp, 2Wp, C)
  const int F = 4 * C;
  const int64_t total = (int64_t)T * Hp * Wp * F;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int f = (int)(g % F);
    const int64_t row = g / F;
    const int64_t tok = tok_perm ? tok_perm[row] : row;
    const int wp = (int)(tok % Wp), hp = (int)((tok / Wp) % Hp), t = (int)(tok / ((int64_t)Wp * Hp));
    const int c = f >> 2, ph = (f >> 1) & 1, pw = f & 1;
    out[(((int64_t)t * 2 * Hp + 2 * hp + ph) * (2 * Wp) + 2 * wp + pw) * C + c] = x[row * ldx + f];
  }
}

// Element k of a vector of packed bf16 pairs (u32x2 / u32x4) as float: the low half of a word is the element of the lower index.
template <typename V>
__device__ __forceinline__ float bf16_at(V r, int k) {
  const uint32_t p = r[k >> 1];
  return __uint_as_float((k & 1) ? (p & 0xffff0000u) : (p << 16));
}

// The CFG combine, uncond + w * (cond - uncond), with each eager bf16 op rounded (generation_utils.py:74-76): bf16 after the difference, after
// the product and after the sum.  Every product feeds a bf16 rounding before it meets an add, so nothing here can contract and no pragma is
// needed; keep it that way.  The step, the windows and the preview all combine through this one function: their bits agree by construction.
__device__ __forceinline__ float cfg_velocity(float w, float c, float u) {
  return bf_round(__fadd_rn(u, bf_round(__fmul_rn(w, bf_round(__fsub_rn(c, u))))));
}

// Editing (video-to-video, keep mask): x_sigma = (1 - sigma) * x0 + sigma * eps with each of the three operations rounded to fp32 on its own, so
// that the torch expression `a * x0 + sigma * eps` as separate ops is the oracle bit for bit.  __fmul_rn / __fadd_rn are plain * and + to this
// compiler (see the rotation above) and hipcc contracts by default, hence the pragma: nothing in these two functions may fuse.  The pragma holds only
// under hipcc's DEFAULT contraction mode (fast-honor-pragmas), which is what build.py compiles with: an explicit -ffp-contract=fast on the command
// line makes the compiler ignore it and fuse one product of each sum (seen in the ISA), which breaks the bit-exact tests.  Do not add that flag.
__device__ __forceinline__ float renoise_at(float a, float sigma, float x0, float eps) {
#pragma clang fp contract(off)
  const float p = a * x0;
  const float q = sigma * eps;
  return p + q;
}
// x with the kept part put back: m == 1 -> known, m == 0 -> x, otherwise x + m * (known - x)
__device__ __forceinline__ float keep_blend(float x, float known, float m) {
#pragma clang fp contract(off)
  if (m == 1.0f) return known;
  if (m == 0.0f) return x;
  const float d = known - x;
  const float md = m * d;
  return x + md;
}
// v = bf16(alpha * c + beta * u) with the two products and the sum rounded to fp32 each on its own (the pragma: see renoise_at)
__device__ __forceinline__ float guided_velocity(float alpha, float beta, float c, float u) {
#pragma clang fp contract(off)
  const float p = alpha * c;
  const float q = beta * u;
  return bf_round(p + q);
}
// Skip-layer guidance on top of a step's velocity: v = bf16(base + bf16(g * bf16(c - s))), the eager bf16 expression `base + g * (c - s)` with
// every op rounded; each product and difference meets a bf16 rounding before the next op, the pragma only says so
__device__ __forceinline__ float skip_velocity(float base, float g, float c, float s) {
#pragma clang fp contract(off)
  const float d = bf_round(c - s);
  const float e = bf_round(g * d);
  return bf_round(base + e);
}

// ---------------------------------------------------------------------------------------------
// Counter-based noise (stochastic sampling): Philox4x32-10 (Salmon et al. 2011) — multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
// constants 0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped between rounds.  Nothing is read from memory and no state lives anywhere: the
// words of a block are a pure function of (counter, key).  A round is two 32 x 32 -> 64 products, each a v_mul_hi_u32 and a v_mul_lo_u32, both
// quarter-rate: 40 of them per block are the generator's cost, far above the four transcendentals that follow, so one thread evaluates a
// whole block and keeps all four words — a thread per ELEMENT would pay the forty multiplies four times for the same bits.
K5_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// u = ((r >> 9) + 0.5) * 2^-23: 23 bits and the half fit fp32's 24, the scaling is a power of two — exact, and inside (0, 1)
K5_DEV float philox_unit(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 0x1p-23f; }

// The four standard normals of block `blk` of stream `stream_id` under `seed`: key = (low, high word of the seed), counter = (low, high word
// of blk, stream_id, 0); (z0, z1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1) and (z2, z3) from (u2, u3) likewise (Box-Muller).  fp32 throughout with
// the library's logf / sqrtf / sincospif, no fast-math intrinsic; sincospif takes 2 u1 (exact) and so spares the rounding of 2 pi u1.
K5_DEV void philox_normal4(uint64_t blk, uint64_t seed, uint32_t stream_id, float (&z)[4]) {
  uint32_t r[4];
  philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), stream_id, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
  for (int j = 0; j < 4; j += 2) {
    const float rad = sqrtf(-2.0f * logf(philox_unit(r[j])));
    float sn, cs;
    sincospif(2.0f * philox_unit(r[j + 1]), &sn, &cs);
    z[j] = rad * cs;
    z[j + 1] = rad * sn;
  }
}

__global__ __launch_bounds__(256) void philox_words_kernel(uint32_t* __restrict__ out, uint64_t blk0, int64_t nblk, uint64_t seed, uint32_t c2,
                                                           uint32_t c3) {
  for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < nblk; b += (int64_t)gridDim.x * 256) {
    const uint64_t blk = blk0 + (uint64_t)b;   // wraps mod 2^64
    uint32_t r[4];
    philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[b * 4 + k] = r[k];
  }
}

// out[g] = z[g & 3] of block g >> 2: a thread per block; the thread of a last, partial block evaluates it whole and stores what exists
__global__ __launch_bounds__(256) void noise_normal_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint32_t stream_id) {
  const int64_t nblk = (n + 3) >> 2;
  for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < nblk; b += (int64_t)gridDim.x * 256) {
    float z[4];
    philox_normal4((uint64_t)b, seed, stream_id, z);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (b * 4 + k < n) out[b * 4 + k] = z[k];
  }
}

// The sampler's update of one step, one pass over the latent (K18): the velocity is v = guided_velocity(ab[0], ab[1], c, u) with coefficients
// from device memory (guidance_finish_kernel wrote them), else cfg_velocity(w, c, u), else (vu NULL) c itself; img += bf16(dt * v)
// (generation_utils.py:128, (0-dim fp32) * (bf16) -> bf16); then, under a keep mask, the keep rule at sigma_next: element g of cell g / C reads
// mask[g / C].  v_out (nullable, may be vc, hence no __restrict__ on either: element g is read before it is written, by the same thread)
// receives v, for the watch's preview.  In the captured step dt and sigma_next come from the device tables at the device step counter;
// signext is given only when something reads sigma_next.  Two instantiations, coefficients from the device (AB: ab and v_out are read) or not:
// with that choice made at run time the plain update measured 1.1 - 1.6 us slower per launch at the 5 s clip's 3.0 M elements.
// A third instantiation (SK) is the skip-layer-guidance step: a third stream vs, the conditional velocity with some blocks skipped, and a scale
// sg by value; the velocity above is the base and v = skip_velocity(base, sg, c, s).  There ab is looked at at run time (the step runs a third
// forward, a branch on a uniform is nothing next to it) and v_out receives v with or without coefficients.
// A fourth instantiation (ST) is the stochastic step (k5_stochastic_euler): after x1 = x + bf16(dt v), with dt the step's dt_down, comes
// x2 = renoise_at(scale, noise_coef, x1, z) when noise_coef != 0 (x1 itself when it is 0: the launch is the same, a branch on a uniform), z from
// `znoise` or, without one, from philox_normal4 — then the keep rule.  There a thread owns the four elements of one Philox block (g >> 2), so
// the forty quarter-rate multiplies of a block are paid once for four elements; ab and vs are looked at at run time as in SK.  The one thread
// whose block reaches past n (n % 4 != 0) still evaluates the whole block — one block's arithmetic per launch, for one to three elements.
// In the captured step scale and noise_coef come from device tables at the step counter, next to dtvec, and the stream id is stream_id + *step.
// ST is a template parameter, not a branch: the three instantiations above keep one element per thread and their instruction stream
// (the per-element body below is theirs, PER = 1 folds the inner loop away; 24 / 25 / 26 VGPRs as before).  Measured at the 5 s clip's 3.0 M
// elements, legs alternated in one process (tools/stochastic_bench.py, profiles/stochastic_bench.jsonl): the plain update 5.98 us against 6.04 us
// from the build without ST; ST with in-kernel noise 10.64 us, with znoise 9.23 us (+ 7.41 us for the launch that would write it), with
// noise_coef == 0 7.93 us.
template <bool AB, bool SK, bool ST>
__global__ __launch_bounds__(256) void euler_step_kernel(float* __restrict__ img, const bf16_t* vc, const bf16_t* __restrict__ vu, float w,
                                                         const float* __restrict__ ab, float dt, const float* __restrict__ x0,
                                                         const float* __restrict__ eps, const float* __restrict__ mask, float sigma_next,
                                                         int C, bf16_t* v_out, const float* __restrict__ dtvec,
                                                         const float* __restrict__ signext, const int* __restrict__ step, int64_t n,
                                                         const bf16_t* __restrict__ vs, float sg, float scale, float noise_coef,
                                                         const float* __restrict__ znoise, uint64_t seed, uint32_t stream_id,
                                                         const float* __restrict__ scalevec, const float* __restrict__ coefvec) {
  if (dtvec) dt = dtvec[*step];
  if (signext) sigma_next = signext[*step];
  if (ST && scalevec) { scale = scalevec[*step]; noise_coef = coefvec[*step]; stream_id += (uint32_t)*step; }
  const bool skip = ST ? vs != nullptr : SK;
  const bool coeffs = (SK || ST) ? ab != nullptr : AB;
  const bool noisy = ST && noise_coef != 0.0f;
  const float alpha = coeffs ? ab[0] : 0.0f, beta = coeffs ? ab[1] : 0.0f;
  const float a = 1.0f - sigma_next;
  const bf16_t* up = vu ? vu : vc;   // without guidance u is unused: the same address again costs no traffic, a branch around the load would cost a wait
  constexpr int PER = ST ? 4 : 1;    // elements per thread
  const int64_t items = ST ? (n + 3) >> 2 : n;
  // ST: a thread's four elements are 16 B of the latent and 8 B of each velocity, so where n % 4 == 0 and the bases allow it they move as one
  // access each; otherwise element by element (64 lanes x 4 B at a 16-B stride: the same lines, four instructions each)
  const auto at = [](const void* q, uintptr_t m) { return (reinterpret_cast<uintptr_t>(q) & (m - 1)) == 0; };
  const bool vec = ST && (n & 3) == 0 && at(img, 16) && at(vc, 8) && at(up, 8) && at(vs, 8) && at(znoise, 16) && at(v_out, 8);
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 xv = {0.0f, 0.0f, 0.0f, 0.0f}, zv = xv;
    u32x2 cv = {0u, 0u}, uv = cv, sv = cv, ov = cv;
    if (ST && vec) {   // every load ahead of the generator's arithmetic
      xv = *reinterpret_cast<const f32x4*>(img + it * 4);
      cv = *reinterpret_cast<const u32x2*>(vc + it * 4);
      uv = *reinterpret_cast<const u32x2*>(up + it * 4);
      sv = skip ? *reinterpret_cast<const u32x2*>(vs + it * 4) : cv;
      if (noisy && znoise) zv = *reinterpret_cast<const f32x4*>(znoise + it * 4);
    }
    if (ST && noisy && !znoise) philox_normal4((uint64_t)it, seed, stream_id, z);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int64_t g = ST ? it * 4 + k : it;
      if (ST && g >= n) break;
      float x, c, u, s3;
      if (ST && vec) {
        x = xv[k]; c = bf16_at(cv, k); u = bf16_at(uv, k); s3 = bf16_at(sv, k);
      } else {
        // every load that does not hang on a value first, so that they are in flight together: a thread has one or two elements, latency is the cost
        const bf16_t cb = vc[g];
        const bf16_t ub = up[g];
        const bf16_t sb = (SK || ST) && skip ? vs[g] : cb;
        x = img[g];
        c = bf2f(cb); u = bf2f(ub); s3 = bf2f(sb);
      }
      const float m = mask ? mask[g / C] : 0.0f;
      float v = coeffs ? guided_velocity(alpha, beta, c, u) : (vu ? cfg_velocity(w, c, u) : c);
      if ((SK || ST) && skip) v = skip_velocity(v, sg, c, s3);
      x = __fadd_rn(x, bf_round(__fmul_rn(dt, v)));
      if (ST && noisy) x = renoise_at(scale, noise_coef, x, znoise ? (vec ? zv[k] : znoise[g]) : z[k]);
      if (m != 0.0f) x = keep_blend(x, renoise_at(a, sigma_next, x0[g], eps[g]), m);
      if (ST && vec) {
        xv[k] = x;
        ov[k >> 1] |= (__float_as_uint(bf_round(v)) >> 16) << (16 * (k & 1));   // bf_round(v) == v: its low half is zero
      } else {
        img[g] = x;
        if ((AB || SK || ST) && v_out) v_out[g] = f2bf(v);
      }
    }
    if (ST && vec) {
      *reinterpret_cast<f32x4*>(img + it * 4) = xv;
      if (v_out) *reinterpret_cast<u32x2*>(v_out + it * 4) = ov;
    }
  }
}

// e added to z under the keep mask: m == 1 -> z, m == 0 -> z + e, otherwise z + (1 - m) * e, the difference, the product and the sum rounded
// to fp32 each on its own (the pragma: see renoise_at)
__device__ __forceinline__ float flowedit_add(float z, float e, float m) {
#pragma clang fp contract(off)
  if (m == 1.0f) return z;
  if (m == 0.0f) return z + e;
  const float k = 1.0f - m;
  const float ke = k * e;
  return z + ke;
}
// zt = zs + (z_fe - x_src): the difference first, so that z_fe == x_src gives zs bit for bit
__device__ __forceinline__ float flowedit_target(float zs, float zfe, float x0) {
#pragma clang fp contract(off)
  const float d = zfe - x0;
  return zs + d;
}

// FlowEdit (k5_flowedit_step, the rule is written at k5_flowedit_step_args): one pass finishes step i and prepares step i + 1.  UPDATE: z_fe +=
// bf16(dt * bf16(v_t - v_s)) under the keep mask, v_s / v_t the CFG velocities of the source and target side (cfg_velocity; an `us` / `ut` of
// NULL is weight 1: the conditional velocity itself).  PREPARE: zs = renoise_at(1 - sigma, sigma, x_src, z) and zt = zs + (z_fe - x_src) for the
// next step, z from `znoise` or philox_normal4.  A thread owns the four elements of one Philox block, as euler_step_kernel<ST> does: 16 B of each
// fp32 stream and 8 B of each bf16 stream per access where n % 4 == 0 and the bases allow it (a wave then covers 1 KiB / 512 B of consecutive
// addresses per instruction), otherwise element by element with the same bits.  The update runs before the generator, so the four velocity
// streams are dead and z_fe is stored before the Philox rounds need registers.  As compiled by build.py (resources.json): <true, true> 55 VGPRs,
// 106 SGPRs with 9 of them spilled to lanes, 7 waves per SIMD — the ten pointers and the wide scalars, not the vector registers, cost the eighth
// wave; <true, false> 38 VGPRs and <false, true> 48, both at 8 waves.  z_fe is read and written by the same thread only.
template <bool UPDATE, bool PREPARE>
__global__ __launch_bounds__(256) void flowedit_step_kernel(float* __restrict__ zfe, const float* __restrict__ x0, const bf16_t* __restrict__ cs,
                                                            const bf16_t* __restrict__ us, const bf16_t* __restrict__ ct,
                                                            const bf16_t* __restrict__ ut, float w_src, float w_tar, float dt,
                                                            const float* __restrict__ mask, int C, float sigma, float* __restrict__ zs_out,
                                                            float* __restrict__ zt_out, const float* __restrict__ znoise, uint64_t seed,
                                                            uint32_t stream_id, int64_t n) {
  const float a = 1.0f - sigma;
  const bf16_t* usp = us ? us : cs;   // weight 1: u is unused, the same address again costs no traffic (see euler_step_kernel)
  const bf16_t* utp = ut ? ut : ct;
  const int64_t items = (n + 3) >> 2;
  const auto at = [](const void* q, uintptr_t m) { return (reinterpret_cast<uintptr_t>(q) & (m - 1)) == 0; };
  const bool vec = (n & 3) == 0 && at(zfe, 16) && at(x0, 16) && at(cs, 8) && at(us, 8) && at(ct, 8) && at(ut, 8) && at(zs_out, 16) &&
                   at(zt_out, 16) && at(znoise, 16);
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 fv = {0.0f, 0.0f, 0.0f, 0.0f}, xv = fv, zv = fv, sv = fv, tv = fv;
    u32x2 csv = {0u, 0u}, usv = csv, ctv = csv, utv = csv;
    if (vec) {   // every load ahead of the arithmetic
      fv = *reinterpret_cast<const f32x4*>(zfe + it * 4);
      if (UPDATE) {
        csv = *reinterpret_cast<const u32x2*>(cs + it * 4);
        usv = *reinterpret_cast<const u32x2*>(usp + it * 4);
        ctv = *reinterpret_cast<const u32x2*>(ct + it * 4);
        utv = *reinterpret_cast<const u32x2*>(utp + it * 4);
      }
      if (PREPARE) xv = *reinterpret_cast<const f32x4*>(x0 + it * 4);
      if (PREPARE && znoise) zv = *reinterpret_cast<const f32x4*>(znoise + it * 4);
    }
    // the update first: its four velocity streams are done with, and z_fe is on its way out, before the generator's arithmetic needs registers
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t g = it * 4 + k;
      if (g >= n) break;
      if (!vec) fv[k] = zfe[g];
      if (UPDATE) {
        float c1, u1, c2, u2;
        if (vec) {
          c1 = bf16_at(csv, k); u1 = bf16_at(usv, k); c2 = bf16_at(ctv, k); u2 = bf16_at(utv, k);
        } else {
          const bf16_t b1 = cs[g], b2 = usp[g], b3 = ct[g], b4 = utp[g];
          c1 = bf2f(b1); u1 = bf2f(b2); c2 = bf2f(b3); u2 = bf2f(b4);
        }
        const float m = mask ? mask[g / C] : 0.0f;
        const float v_s = us ? cfg_velocity(w_src, c1, u1) : c1;
        const float v_t = ut ? cfg_velocity(w_tar, c2, u2) : c2;
        const float d = bf_round(__fsub_rn(v_t, v_s));
        const float e = bf_round(__fmul_rn(dt, d));
        fv[k] = flowedit_add(fv[k], e, m);
        if (!vec) zfe[g] = fv[k];
      }
    }
    if (UPDATE && vec) *reinterpret_cast<f32x4*>(zfe + it * 4) = fv;
    if (PREPARE) {
      if (!znoise) philox_normal4((uint64_t)it, seed, stream_id, z);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t g = it * 4 + k;
        if (g >= n) break;
        const float x = vec ? xv[k] : x0[g];
        const float zz = znoise ? (vec ? zv[k] : znoise[g]) : z[k];
        const float s1 = renoise_at(a, sigma, x, zz);
        const float t1 = flowedit_target(s1, fv[k], x);
        if (vec) { sv[k] = s1; tv[k] = t1; } else { zs_out[g] = s1; zt_out[g] = t1; }
      }
      if (vec) {
        *reinterpret_cast<f32x4*>(zs_out + it * 4) = sv;
        *reinterpret_cast<f32x4*>(zt_out + it * 4) = tv;
      }
    }
  }
}

__global__ __launch_bounds__(256) void edit_renoise_kernel(float* __restrict__ out, const float* __restrict__ x0,
                                                           const float* __restrict__ eps, float sigma, int64_t n) {
  const float a = 1.0f - sigma;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256)
    out[g] = renoise_at(a, sigma, x0[g], eps[g]);
}

// ---------------------------------------------------------------------------------------------
// Guidance coefficients (k5_launch_guidance_coeffs): the guided velocity of a step is v = alpha * c + beta * u with alpha, beta
// per SAMPLE, from five sums over the two velocities — Sc = sum c, Su = sum u, Scc = sum c^2, Suu = sum u^2, Scu = sum c u.  Everything is
// float64: a product of two bf16 values is exact there, and the order is fixed as in magcache_stats_kernel — a lane adds its 16-byte chunks
// in index order (the eight elements of a chunk in order), an xor butterfly adds the wave, thread 0 the four waves in wave order into
// part[block][5], guidance_finish_kernel the blocks in index order.  No atomics: two launches, two ranks, the two handles of a pair give the
// same bits.
K5_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void guidance_stats_kernel(const bf16_t* __restrict__ vc, const bf16_t* __restrict__ vu,
                                                             double* __restrict__ part, int64_t nch) {
  __shared__ double red[4][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // Sc | Su | Scc | Suu | Scu
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < nch; g += (int64_t)gridDim.x * 256) {
    const u32x4 rc = *reinterpret_cast<const u32x4*>(vc + g * 8);
    const u32x4 ru = *reinterpret_cast<const u32x4*>(vu + g * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // element index order: the low half of a word first
      const double c = (double)bf16_at(rc, k), u = (double)bf16_at(ru, k);
      acc[0] += c; acc[1] += u;
      acc[2] += c * c; acc[3] += u * u; acc[4] += c * u;   // the products are exact, fused or not
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) acc[k] = wave_sum_f64(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) red[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 5) part[(size_t)blockIdx.x * 5 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// sums[k] = the nblk partials of component k in index order (thread (g, k) adds blocks g, g + 64, ..., then thread k the 64 group sums in group
// order), then thread 0 forms the coefficients in float64:
//   s = zero_star ? Scu / (Suu + 1e-8) : 1                    (CFG-Zero*: the projection of c on u)
//   alpha = w, beta = s (1 - w)                               (v = s u + w (c - s u))
//   rescale > 0: k = rescale * sqrt(var c / var v) + (1 - rescale) with the variances from the sums (CFG rescale, std over the sample);
//                var v <= 0 or var c < 0 (rounding of a constant tensor) leaves k = 1
// and writes ab = {(float)alpha, (float)beta}.  One workgroup.  In the captured step w = wvec[*step].
__global__ __launch_bounds__(320) void guidance_finish_kernel(const double* __restrict__ part, int nblk, double n, float w, int zero_star,
                                                              float rescale, const float* __restrict__ wvec, const int* __restrict__ step,
                                                              double* __restrict__ sums, float* __restrict__ ab) {
  __shared__ double red[64][5];
  __shared__ double tot[5];
  const int k = threadIdx.x % 5, g = threadIdx.x / 5;
  double a = 0.0;
  for (int b = g; b < nblk; b += 64) a += part[(size_t)b * 5 + k];
  red[g][k] = a;
  __syncthreads();
  if (threadIdx.x < 5) {
    double t = 0.0;
    for (int i = 0; i < 64; ++i) t += red[i][threadIdx.x];
    tot[threadIdx.x] = t;
    sums[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double Sc = tot[0], Su = tot[1], Scc = tot[2], Suu = tot[3], Scu = tot[4];
    const double wd = (double)(wvec ? wvec[*step] : w);
    const double s = zero_star ? Scu / (Suu + 1e-8) : 1.0;
    double alpha = wd, beta = s * (1.0 - wd);
    if (rescale > 0.0f) {
      const double phi = (double)rescale;
      const double var_c = Scc - Sc * Sc / n;
      const double var_v = alpha * alpha * var_c + 2.0 * alpha * beta * (Scu - Sc * Su / n) + beta * beta * (Suu - Su * Su / n);
      const double kf = (var_v > 0.0 && var_c >= 0.0) ? phi * sqrt(var_c / var_v) + (1.0 - phi) : 1.0;
      alpha *= kf; beta *= kf;
    }
    ab[0] = (float)alpha;
    ab[1] = (float)beta;
  }
}

// Context windows: one term of the cross-fade, acc = wt_0 * v_0 for the first window that covers the cell and acc + wt_i * v_i for
// every later one.  The product and the sum round to fp32 each on its own (the pragma: see renoise_at), so the torch expression with separate
// ops is the oracle bit for bit, and one window of weight 1 leaves v itself.
__device__ __forceinline__ float window_term(float acc, float wt, float v, bool first) {
#pragma clang fp contract(off)
  const float p = wt * v;
  if (first) return p;
  return acc + p;
}

// Spatial context windows (tiles): the share of window (it, iy, ix) at a cell is the product of its three per-axis weights, left to right, each
// product rounded to fp32 on its own (the pragma: see renoise_at)
__device__ __forceinline__ float tile_share(float wt, float wy, float wx) {
#pragma clang fp contract(off)
  const float ty = wt * wy;
  return ty * wx;
}

// The windows of one axis that cover coordinate p: starts ascend, window i spans starts[i] .. starts[i] + F - 1, so the covering windows are
// the contiguous range [lo, hi).  n <= 64; with a workgroup-uniform p (a row's frame and row index) the loop is scalar loads and compares.
__device__ __forceinline__ void covering(const int32_t* __restrict__ starts, int n, int F, int p, int& lo, int& hi) {
  lo = n; hi = 0;
  for (int i = 0; i < n; ++i) {
    const int j = p - starts[i];
    if (j >= 0 && j < F) { lo = i < lo ? i : lo; hi = i + 1; }
  }
}

// euler_step_kernel's CFG update over a clip whose velocities come from the windows of a 3-D plan (a temporal plan: ny = nx = 1 with weights
// 1.0, where tile_share leaves wt itself): img fp32 (T,H,W,C), vc / vu bf16 [nwin][Ft][Fh][Fw][C], window k = (it * ny + iy) * nx + ix at
// (st[it], sy[iy], sx[ix]).  A workgroup takes whole rows (t, y) of the latent, grid-stride: the frame and row ranges of covering windows,
// their weights and local indices are the workgroup's (scalar), no lane divides a 64-bit index.  Inside a row a lane owns VEC consecutive
// channels of one cell (VEC divides C), walks the windows that cover the cell in ascending k — a product of three contiguous index ranges —
// forms v_k with cfg_velocity, blends with window_term under the share tile_share(wt, wy, wx) and applies img += bf16(dt * acc).  Only slots
// inside a window's box are read, whatever the tables hold; a cell no window covers is left as it is.
template <int VEC>
__global__ __launch_bounds__(256) void cfg_euler_tiles_kernel(float* __restrict__ img, const bf16_t* __restrict__ vc,
                                                              const bf16_t* __restrict__ vu, float w, float dt, k5_tile_plan p, int T, int H,
                                                              int W, int C) {
  const int per_cell = C / VEC, units = W * per_cell, rows = T * H;   // a row's lane-sized pieces; the launcher keeps both products in an int
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int t = row / H, y = row - t * H;
    int t_lo, t_hi, y_lo, y_hi;
    covering(p.starts_t, p.nt, p.Ft, t, t_lo, t_hi);
    covering(p.starts_y, p.ny, p.Fh, y, y_lo, y_hi);
    for (int u = threadIdx.x; u < units; u += 256) {
      const int x = u / per_cell, c = (u - x * per_cell) * VEC;
      int x_lo, x_hi;
      covering(p.starts_x, p.nx, p.Fw, x, x_lo, x_hi);
      float acc[VEC];
      bool first = true;
      for (int it = t_lo; it < t_hi; ++it) {
        const int jt = t - p.starts_t[it];
        const float wt = p.wt[it * p.Ft + jt];
        for (int iy = y_lo; iy < y_hi; ++iy) {
          const int jy = y - p.starts_y[iy];
          const float wy = p.wy[iy * p.Fh + jy];
          const int64_t slot_row = (((int64_t)it * p.ny + iy) * p.nx * p.Ft + jt) * p.Fh + jy;   // of window (it, iy, 0); one window further: Ft * Fh rows
          for (int ix = x_lo; ix < x_hi; ++ix) {
            const int jx = x - p.starts_x[ix];
            const float share = tile_share(wt, wy, p.wx[ix * p.Fw + jx]);
            const int64_t off = ((slot_row + (int64_t)ix * p.Ft * p.Fh) * p.Fw + jx) * C + c;
            float v[VEC];
            if constexpr (VEC == 4) {
              const u32x2 cr = *reinterpret_cast<const u32x2*>(vc + off);
              u32x2 ur = {0u, 0u};
              if (vu) ur = *reinterpret_cast<const u32x2*>(vu + off);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                v[e] = bf16_at(cr, e);
                if (vu) v[e] = cfg_velocity(w, v[e], bf16_at(ur, e));
              }
            } else {
              v[0] = bf2f(vc[off]);
              if (vu) v[0] = cfg_velocity(w, v[0], bf2f(vu[off]));
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = window_term(first ? 0.0f : acc[e], share, v[e], first);
            first = false;
          }
        }
      }
      if (first) continue;
      float* q = img + ((int64_t)row * W + x) * C + c;
      if constexpr (VEC == 4) {
        f32x4 r = *reinterpret_cast<const f32x4*>(q);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = __fadd_rn(r[e], bf_round(__fmul_rn(dt, acc[e])));
        *reinterpret_cast<f32x4*>(q) = r;
      } else {
        q[0] = __fadd_rn(q[0], bf_round(__fmul_rn(dt, acc[0])));
      }
    }
  }
}

__global__ void step_inc_kernel(int* step) { *step += 1; }

__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, int64_t n) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) out[g] = f2bf(x[g]);
}

inline int grid_for(int64_t n, int per_block = 256, int cap = 8192) {
  int64_t b = (n + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
inline int done() { return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP; }

}  // namespace

int k5_launch_ln_modulate(const void* x, const float* scale, const float* shift, void* out, int rows, int D,
                          int ldx, int ldo, hipStream_t s, void* out_e4m3) {
  if (rows <= 0 || D <= 0 || (!out && !out_e4m3) || !x || !scale || !shift) return K5_ERR_ARG;
  if (ldx < D || (out && ldo < D)) return K5_ERR_ARG;   // a row stride shorter than a row: rows would overlap
  if ((D & 7) || (ldx & 7) || (ldo & 7)) return K5_ERR_ALIGN;
  if (D > 64 * 8 * MAXC) return K5_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(ln_kernel<false>, dim3(ln_grid(rows)), dim3(256), 0, s, (const bf16_t*)x, scale, shift,
                     (bf16_t*)out, (float*)nullptr, rows, D, ldx, ldo, (uint8_t*)out_e4m3);
  return done();
}

int k5_launch_ln_affine(const void* x, const float* w, const float* b, void* out_bf16, float* out_f32, int rows,
                        int D, hipStream_t s) {
  if (rows <= 0 || D <= 0) return K5_ERR_ARG;
  if (D & 7) return K5_ERR_ALIGN;
  if (D > 64 * 8 * MAXC) return K5_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(ln_kernel<true>, dim3(ln_grid(rows)), dim3(256), 0, s, (const bf16_t*)x, w, b,
                     (bf16_t*)out_bf16, out_f32, rows, D, D, D);
  return done();
}

// Ulysses sequence parallelism (engine.hip run_self_attention_heads): head-group repacking around the two all-to-alls.
// pack: x [rows][2 D] = (q heads | k heads) of the rank's token rows -> out [P][slot_rows][2 Dp], block g = (q | k) of the heads rank g attends
__global__ __launch_bounds__(256) void ulysses_pack_qk_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, int rows, int slot_rows, int D, int Dp) {
  const int cpr = 2 * D / 8;                                   // 16-B chunks per row
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)rows * cpr; i += (int64_t)gridDim.x * 256) {
    const int row = (int)(i / cpr), col = (int)(i % cpr) * 8;
    const int part = col >= D ? 1 : 0, cc = col - part * D, g = cc / Dp, within = cc - g * Dp;
    *reinterpret_cast<u32x4*>(out + ((size_t)g * slot_rows + row) * (2 * Dp) + part * Dp + within) = *reinterpret_cast<const u32x4*>(x + (size_t)row * 2 * D + col);
  }
}
// unpack: in [P][slot_rows][Dp] (block g = the outputs of rank g's heads for this rank's rows) -> out [rows][D]
__global__ __launch_bounds__(256) void ulysses_unpack_o_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, int rows, int slot_rows, int D, int Dp) {
  const int cpr = D / 8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)rows * cpr; i += (int64_t)gridDim.x * 256) {
    const int row = (int)(i / cpr), col = (int)(i % cpr) * 8;
    const int g = col / Dp, within = col - g * Dp;
    *reinterpret_cast<u32x4*>(out + (size_t)row * D + col) = *reinterpret_cast<const u32x4*>(in + ((size_t)g * slot_rows + row) * Dp + within);
  }
}

// two-level schedule (engine.hip run_self_attention_heads, two_level): x [rows][2 D] = (q heads | k' heads) of the rank's rows -> q_out / k_out, each
// [G][slot_rows][Dp] (block g = head group g): the per-destination send planes of the two exchanges, contiguous per destination
__global__ __launch_bounds__(256) void sp2d_pack_qk_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ q_out, bf16_t* __restrict__ k_out, int rows,
                                                           int slot_rows, int D, int Dp) {
  const int cpr = 2 * D / 8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)rows * cpr; i += (int64_t)gridDim.x * 256) {
    const int row = (int)(i / cpr), col = (int)(i % cpr) * 8;
    const int part = col >= D ? 1 : 0, cc = col - part * D, g = cc / Dp, within = cc - g * Dp;
    *reinterpret_cast<u32x4*>((part ? k_out : q_out) + ((size_t)g * slot_rows + row) * Dp + within) = *reinterpret_cast<const u32x4*>(x + (size_t)row * 2 * D + col);
  }
}

size_t k5_rmsnorm_stats_workspace_bytes(int H) { return (size_t)4096 * 2 * H * sizeof(float); }   // partial rows of up to 2 H entries (norms + radii)

int k5_launch_rmsnorm_rope(void* x, const float* weight, const float* cosT, const float* sinT, int rows, int H,
                           int ld, const int32_t* heads_cfg, hipStream_t s, float out_scale, int scale_from_head, void* scaled_out,
                           int ld_scaled, float* stats, float* stats_ws, float* key_centre, void* mean_q, int mq_stride, void* mean_k, int mk_stride) {
  // heads_cfg (host pointer, optional): {heads_per_weight, rope_heads}; default: one weight, rope on all heads
  if (rows <= 0 || H <= 0 || !x || !weight) return K5_ERR_ARG;
  if ((cosT != nullptr) != (sinT != nullptr)) return K5_ERR_ARG;   // the rotation needs both tables
  // heads_per_weight divides the head index on the device and picks the weight row; rope_heads is an upper bound on the rotated heads
  if (heads_cfg && (heads_cfg[0] <= 0 || heads_cfg[1] < 0)) return K5_ERR_ARG;
  if (ld < 64 * (int64_t)H) return K5_ERR_ARG;   // H heads of 64 do not fit a row
  const bool means = mean_q || mean_k;
  if (means && ((rows & 63) || (mean_q && mq_stride < rows / 64) || (mean_k && mk_stride < rows / 64))) return K5_ERR_ARG;
  if (ld & 7) return K5_ERR_ALIGN;
  const int hpw = heads_cfg ? heads_cfg[0] : H;
  const int rope_heads = heads_cfg ? heads_cfg[1] : H;
  const int64_t total = (int64_t)rows * H * 8;
  // grid: a multiple of `unit` blocks so that the grid stride (grid * 256 threads) is a multiple of H * 8 threads per row
  int gcd = 256, b8 = H * 8;
  for (int a = gcd, b = b8; b;) { const int t = a % b; a = b; b = t; gcd = a; }
  const int unit = b8 / gcd;
  if (stats && (!stats_ws || H > 256)) return K5_ERR_ARG;
  int64_t cap = 4096 / unit * unit;   // with statistics: one partial row per block (k5_rmsnorm_stats_workspace_bytes)
  if (cap < unit) { if (stats) return K5_ERR_UNSUPPORTED; cap = unit; }
  int64_t blocks = (total + 255) / 256;
  if (blocks > cap) blocks = cap;
  blocks = (blocks + unit - 1) / unit * unit;           // <= cap: cap is a multiple of unit
  if (means) {   // slots (threads per head chunk) = blocks * 256 / (H * 8): every slot the same number k of 64-row blocks where the cap allows
    const int64_t nblk = rows / 64, smax_ = cap * 256 / b8;
    const int64_t k = (nblk + smax_ - 1) / smax_, want = (nblk + k - 1) / k;
    blocks = (want * b8 + 255) / 256;
    blocks = (blocks + unit - 1) / unit * unit;
    if (blocks > cap) blocks = cap;
  }
  // key_centre (nullable, with stats and scaled heads only): [H - scale_from_head][64] floats OUT = the centres of the scaled (key) heads;
  // stats then has H + (H - scale_from_head) entries: the squared norms, then the squared radii around the centres
  const bool centred = key_centre && stats && scale_from_head < H;
  if (centred)
    hipLaunchKernelGGL(key_centre_kernel, dim3(H - scale_from_head), dim3(256), 0, s, (const bf16_t*)x, weight, cosT, sinT, rows, ld, scale_from_head, hpw,
                       rope_heads, out_scale, rows < K5_CENTRE_SAMPLE ? rows : K5_CENTRE_SAMPLE, key_centre);
  const int Hs = centred ? H + (H - scale_from_head) : H;
  if (stats && Hs > 256) return K5_ERR_UNSUPPORTED;   // the statistics live in a 256-entry LDS table; without them any head count goes (cross-attention keys of all blocks: 896)
  if (means)
    hipLaunchKernelGGL(rmsnorm_rope_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, (bf16_t*)x, weight,
                       cosT, sinT, rows, H, hpw, ld, rope_heads, out_scale, scale_from_head, (bf16_t*)scaled_out, ld_scaled, stats ? stats_ws : nullptr,
                       centred ? key_centre : nullptr, (bf16_t*)mean_q, mq_stride, (bf16_t*)mean_k, mk_stride);
  else
    hipLaunchKernelGGL(rmsnorm_rope_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, (bf16_t*)x, weight,
                       cosT, sinT, rows, H, hpw, ld, rope_heads, out_scale, scale_from_head, (bf16_t*)scaled_out, ld_scaled, stats ? stats_ws : nullptr,
                       centred ? key_centre : nullptr, (bf16_t*)nullptr, 0, (bf16_t*)nullptr, 0);
  if (stats) hipLaunchKernelGGL(stats_reduce_kernel, dim3(blocks >= 2048 ? 64 : (blocks >= 512 ? 16 : 1)), dim3(256), 0, s, stats_ws, (int)blocks, Hs, stats);
  return done();
}

int k5_launch_ulysses_pack_qk(const void* x, void* out, int rows, int slot_rows, int D, int P, hipStream_t s) {
  if (rows <= 0 || slot_rows < rows || P <= 0 || D % P || (D / P) % 8) return K5_ERR_ARG;
  hipLaunchKernelGGL(ulysses_pack_qk_kernel, dim3(grid_for((int64_t)rows * (2 * D / 8))), dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)out, rows, slot_rows, D, D / P);
  return done();
}
int k5_launch_ulysses_unpack_o(const void* in, void* out, int rows, int slot_rows, int D, int P, hipStream_t s) {
  if (rows <= 0 || slot_rows < rows || P <= 0 || D % P || (D / P) % 8) return K5_ERR_ARG;
  hipLaunchKernelGGL(ulysses_unpack_o_kernel, dim3(grid_for((int64_t)rows * (D / 8))), dim3(256), 0, s, (const bf16_t*)in, (bf16_t*)out, rows, slot_rows, D, D / P);
  return done();
}

int k5_launch_sp2d_pack_qk(const void* x, void* q_out, void* k_out, int rows, int slot_rows, int D, int G, hipStream_t s) {
  if (rows <= 0 || slot_rows < rows || G <= 0 || D % G || (D / G) % 8) return K5_ERR_ARG;
  hipLaunchKernelGGL(sp2d_pack_qk_kernel, dim3(grid_for((int64_t)rows * (2 * D / 8))), dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)q_out, (bf16_t*)k_out, rows,
                     slot_rows, D, D / G);
  return done();
}

int k5_launch_gate_sum(const void* x, const void* y, const float* gate, void* out, int rows, int D, hipStream_t s) {
  if (rows <= 0 || D <= 0) return K5_ERR_ARG;
  if (D & 7) return K5_ERR_ALIGN;
  const int64_t nch = (int64_t)rows * (D / 8);
  hipLaunchKernelGGL(gate_sum_kernel, dim3(grid_for(nch)), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)y, gate,
                     (bf16_t*)out, nch, D / 8);
  return done();
}

int k5_magcache_stats_blocks(int rows) {
  const int wg = (rows + 3) / 4;
  return wg < 16384 ? wg : 16384;
}

int k5_launch_magcache_stats(const void* vis, const void* ori, const void* prev, void* res, double* sums, double* part, int accumulate,
                             int rows, int D, hipStream_t s) {
  if (rows <= 0 || D <= 0 || !vis || !ori || !res || !sums) return K5_ERR_ARG;
  if (D & 7) return K5_ERR_ALIGN;
  const int grid = k5_magcache_stats_blocks(rows);
  if (!prev) {   // a slot's first call: nothing to compare with
    hipLaunchKernelGGL(magcache_stats_kernel<false>, dim3(grid), dim3(256), 0, s, (const bf16_t*)vis, (const bf16_t*)ori, (const bf16_t*)nullptr,
                       (bf16_t*)res, (double*)nullptr, rows, D / 8);
    if (!accumulate && hipMemsetAsync(sums, 0, 4 * sizeof(double), s) != hipSuccess) return K5_ERR_HIP;
    return done();
  }
  if (!part) return K5_ERR_ARG;
  hipLaunchKernelGGL(magcache_stats_kernel<true>, dim3(grid), dim3(256), 0, s, (const bf16_t*)vis, (const bf16_t*)ori, (const bf16_t*)prev,
                     (bf16_t*)res, part, rows, D / 8);
  hipLaunchKernelGGL(magcache_finish_kernel, dim3(1), dim3(1024), 0, s, (const double*)part, grid, sums, accumulate);
  return done();
}

int k5_launch_gemv_f32(const float* x, const float* W, const float* b, float* y, int N, int K, int silu_in,
                       const float* add, hipStream_t s) {
  if (N <= 0 || K <= 0 || !x || !W || !y) return K5_ERR_ARG;
  if (K & 3) return K5_ERR_ALIGN;
  hipLaunchKernelGGL(gemv_f32_kernel, dim3((N + 3) / 4), dim3(256), 0, s, x, W, b, y, N, K, silu_in, add);
  return done();
}

int k5_launch_time_features(float t, float* out, int D, hipStream_t s, const float* tvec, const int* step) {
  if (D <= 0 || (D & 1) || ((tvec != nullptr) != (step != nullptr))) return K5_ERR_ARG;
  hipLaunchKernelGGL(time_features_kernel, dim3((D / 2 + 255) / 256), dim3(256), 0, s, t, tvec, step, out, D);
  return done();
}

int k5_launch_step_inc(int* step, hipStream_t s) {
  hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, step);
  return done();
}

int k5_launch_rope_table(float* cosT, float* sinT, const int32_t* p0, const int32_t* p1, const int32_t* p2, int T,
                         int H, int W, int n0, int n1, int n2, float s0, float s1, float s2, const int32_t* tok_perm,
                         hipStream_t s) {
  // every extent on its own: a product of two negative extents is positive.  A table row is the 32 rotation pairs of a 64-wide head
  // (rmsnorm_rope_kernel and the attention's fused query norm read rows of 32 floats), so the three axis widths add up to 32; an axis of
  // width 0 has no positions (the 1-D text table is 32 | 0 | 0)
  if (T <= 0 || H <= 0 || W <= 0 || n0 < 0 || n1 < 0 || n2 < 0 || n0 + n1 + n2 != 32) return K5_ERR_ARG;
  if (!cosT || !sinT || (n0 && !p0) || (n1 && !p1) || (n2 && !p2)) return K5_ERR_ARG;
  const int64_t total = (int64_t)T * H * W * 32;
  hipLaunchKernelGGL(rope_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cosT, sinT, p0, p1, p2,
                     T, H, W, n0, n1, n2, s0, s1, s2, tok_perm);
  return done();
}

int k5_launch_patchify(const float* x, void* out, int T, int H, int W, int C, int Cin_total, int Kpad,
                       const int32_t* tok_perm, hipStream_t s) {
  if (!x || !out || T <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || Kpad < 4 * Cin_total || C <= 0 || C > Cin_total) return K5_ERR_ARG;
  const int64_t total = (int64_t)T * (H / 2) * (W / 2) * Kpad;
  hipLaunchKernelGGL(patchify_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, (bf16_t*)out, T, H, W, C, Cin_total, Kpad,
                     tok_perm);
  return done();
}

int k5_launch_patchify_cond(const float* x, const float* vcond, void* out, int T, int H, int W, int C, int Cin_total, int Kpad,
                            const int32_t* tok_perm, hipStream_t s) {
  if (!x || !vcond || !out || T <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || Kpad < 4 * Cin_total || C <= 0 || C >= Cin_total)
    return K5_ERR_ARG;
  const int64_t total = (int64_t)T * (H / 2) * (W / 2) * Kpad;
  hipLaunchKernelGGL(patchify_cond_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, vcond, (bf16_t*)out, T, H, W, C, Cin_total,
                     Kpad, tok_perm);
  return done();
}

int k5_launch_patchify_view(const float* x, int64_t x_frame, int64_t x_row, const float* vcond, int64_t vc_frame, int64_t vc_row, void* out,
                            int T, int H, int W, int C, int Cin_total, int Kpad, const int32_t* tok_perm, hipStream_t s) {
  if (!x || !out || T <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || Kpad < 4 * Cin_total || C <= 0 || C > Cin_total) return K5_ERR_ARG;
  if (vcond && C >= Cin_total) return K5_ERR_ARG;
  // a stride spans the extent below it: a row holds W cells, a frame H rows
  if (x_row < (int64_t)W * C || x_frame < (int64_t)H * x_row) return K5_ERR_ARG;
  if (vcond && (vc_row < (int64_t)W * (Cin_total - C) || vc_frame < (int64_t)H * vc_row)) return K5_ERR_ARG;
  const int64_t total = (int64_t)T * (H / 2) * (W / 2) * Kpad;
  hipLaunchKernelGGL(patchify_view_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, x_frame, x_row, vcond, vc_frame, vc_row, (bf16_t*)out, T,
                     H, W, C, Cin_total, Kpad, tok_perm);
  return done();
}

int k5_launch_unpatchify(const void* x, void* out, int T, int Hp, int Wp, int C, int ldx, const int32_t* tok_perm,
                         hipStream_t s) {
  if (!x || !out || T <= 0 || Hp <= 0 || Wp <= 0 || C <= 0 || ldx < 4 * (int64_t)C) return K5_ERR_ARG;   // every extent on its own, not their product
  const int64_t total = (int64_t)T * Hp * Wp * 4 * C;
  hipLaunchKernelGGL(unpatchify_kernel, dim3(grid_for(total)), dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)out, T, Hp, Wp,
                     C, ldx, tok_perm);
  return done();
}

int k5_launch_euler_step(const K5EulerStepArgs& a) {
  if (!a.img || !a.v_cond || a.cells <= 0 || a.C <= 0) return K5_ERR_ARG;
  if ((a.ab && !a.v_uncond) || (a.v_out && !a.ab && !a.v_skip) || (a.keep_mask && (!a.source || !a.noise))) return K5_ERR_ARG;
  if (((a.dtvec != nullptr) != (a.step != nullptr)) || (a.signext && !a.dtvec)) return K5_ERR_ARG;
  if (a.v_skip ? !(a.skip_scale > 0.0f && __builtin_isfinite(a.skip_scale)) : a.skip_scale != 0.0f) return K5_ERR_ARG;   // also a NaN or negative scale
  if (a.stochastic) {
    if (!__builtin_isfinite(a.scale) || !(a.noise_coef >= 0.0f && __builtin_isfinite(a.noise_coef))) return K5_ERR_ARG;   // also a NaN
    if (((a.scalevec != nullptr) != (a.coefvec != nullptr)) || (a.scalevec && !a.step)) return K5_ERR_ARG;
  } else if (a.znoise || a.scalevec || a.coefvec) return K5_ERR_ARG;
  const int64_t n = a.cells * a.C;
  const auto kernel = a.stochastic ? euler_step_kernel<false, false, true>
                      : a.v_skip   ? euler_step_kernel<false, true, false>
                      : a.ab       ? euler_step_kernel<true, false, false>
                                   : euler_step_kernel<false, false, false>;
  hipLaunchKernelGGL(kernel, dim3(grid_for(a.stochastic ? (n + 3) / 4 : n)), dim3(256), 0, a.stream, a.img, (const bf16_t*)a.v_cond,
                     (const bf16_t*)a.v_uncond, a.w, a.ab, a.dt, a.source, a.noise, a.keep_mask, a.sigma_next, a.C, (bf16_t*)a.v_out, a.dtvec,
                     a.signext, a.step, n, (const bf16_t*)a.v_skip, a.skip_scale, a.scale, a.noise_coef, a.znoise, a.seed, a.stream_id,
                     a.scalevec, a.coefvec);
  return done();
}

const char* k5_flowedit_step_refusal(const k5_flowedit_step_args& a) {
  const auto off4 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; };
  if (!a.z_fe) return "z_fe is NULL";
  if (!a.x_src) return "x_src is NULL";
  if (a.cells < 1 || a.C < 1) return "cells and C must be >= 1";
  if ((a.c_src != nullptr) != (a.c_tar != nullptr)) return "c_src and c_tar go together";
  if (!a.c_src && !a.prepare) return "neither velocities nor a next sigma: nothing to do";
  if (a.c_src && a.w_src != 1.0f && !a.u_src) return "w_src != 1 needs u_src";
  if (a.c_src && a.w_tar != 1.0f && !a.u_tar) return "w_tar != 1 needs u_tar";
  if (a.prepare && (!a.zs || !a.zt)) return "a next sigma needs zs and zt";
  if (off4(a.z_fe) || off4(a.x_src) || off4(a.c_src) || off4(a.u_src) || off4(a.c_tar) || off4(a.u_tar) || off4(a.keep_mask) || off4(a.zs) ||
      off4(a.zt) || off4(a.znoise))
    return "a pointer is not 4-byte aligned";
  return nullptr;
}

int k5_launch_flowedit_step(const k5_flowedit_step_args& a, hipStream_t s) {
  if (k5_flowedit_step_refusal(a)) return K5_ERR_ARG;
  const int64_t n = a.cells * a.C;
  const bool update = a.c_src != nullptr;
  const auto kernel = update ? (a.prepare ? flowedit_step_kernel<true, true> : flowedit_step_kernel<true, false>)
                             : flowedit_step_kernel<false, true>;
  // a weight of 1 is the conditional velocity itself: its u is not handed on and so is never read
  hipLaunchKernelGGL(kernel, dim3(grid_for((n + 3) / 4, 256, 2048)), dim3(256), 0, s, a.z_fe, a.x_src, (const bf16_t*)a.c_src,
                     (const bf16_t*)(a.w_src != 1.0f ? a.u_src : nullptr), (const bf16_t*)a.c_tar,
                     (const bf16_t*)(a.w_tar != 1.0f ? a.u_tar : nullptr), a.w_src, a.w_tar, a.dt, update ? a.keep_mask : nullptr, a.C,
                     a.sigma_next, a.zs, a.zt, a.prepare ? a.znoise : nullptr, a.seed, a.stream_id, n);
  return done();
}

int k5_launch_philox_words(uint32_t* out, uint64_t blk0, int64_t nblk, uint64_t seed, uint32_t c2, uint32_t c3, hipStream_t s) {
  if (!out || nblk < 1 || (reinterpret_cast<uintptr_t>(out) & 3)) return K5_ERR_ARG;
  hipLaunchKernelGGL(philox_words_kernel, dim3(grid_for(nblk)), dim3(256), 0, s, out, blk0, nblk, seed, c2, c3);
  return done();
}

int k5_launch_noise_normal(float* out, int64_t n, uint64_t seed, uint32_t stream_id, hipStream_t s) {
  if (!out || n < 1 || (reinterpret_cast<uintptr_t>(out) & 3)) return K5_ERR_ARG;
  hipLaunchKernelGGL(noise_normal_kernel, dim3(grid_for((n + 3) / 4, 256, 1024)), dim3(256), 0, s, out, n, seed, stream_id);
  return done();
}

int k5_launch_edit_renoise(float* out, const float* source, const float* noise, float sigma, int64_t n, hipStream_t s) {
  if (!out || !source || !noise || n <= 0) return K5_ERR_ARG;
  hipLaunchKernelGGL(edit_renoise_kernel, dim3(grid_for(n)), dim3(256), 0, s, out, source, noise, sigma, n);
  return done();
}

int k5_guidance_blocks(int64_t n) {
  const int64_t wg = (n / 8 + 255) / 256;
  return wg < 1 ? 1 : wg < 1024 ? (int)wg : 1024;
}

int k5_launch_guidance_coeffs(const void* vc, const void* vu, int64_t n, float w, int zero_star, float rescale, double* part, double* sums,
                              float* ab, hipStream_t s, const float* wvec, const int* step) {
  const auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  if (!vc || !vu || !part || !sums || !ab || n < 1 || !(rescale >= 0.0f && rescale <= 1.0f) || ((wvec != nullptr) != (step != nullptr)))
    return K5_ERR_ARG;
  if (misaligned(vc) || misaligned(vu) || misaligned(part) || misaligned(sums) || misaligned(ab)) return K5_ERR_ARG;
  if (n & 7) return K5_ERR_ALIGN;
  const int grid = k5_guidance_blocks(n);
  hipLaunchKernelGGL(guidance_stats_kernel, dim3(grid), dim3(256), 0, s, (const bf16_t*)vc, (const bf16_t*)vu, part, n / 8);
  hipLaunchKernelGGL(guidance_finish_kernel, dim3(1), dim3(320), 0, s, (const double*)part, grid, (double)n, w, zero_star, rescale, wvec, step,
                     sums, ab);
  return done();
}

const char* k5_tile_axis_refusal(const char* axis, int n, const int32_t* starts, int F, int total) {
  static thread_local char msg[160];
  if (n < 1 || F < 1 || total < 1 || !starts) { snprintf(msg, sizeof msg, "%s: %d windows of %d in %d, or no starts", axis, n, F, total); return msg; }
  for (int i = 0; i < n; ++i) {
    const int st = starts[i];
    if (st < 0 || (int64_t)st + F > total) {
      snprintf(msg, sizeof msg, "%s window %d (%d .. %lld) reaches outside 0 .. %d", axis, i, st, (long long)st + F - 1, total - 1);
      return msg;
    }
    if (i > 0 && st <= starts[i - 1]) { snprintf(msg, sizeof msg, "%s starts must ascend (starts[%d] = %d after %d)", axis, i, st, starts[i - 1]); return msg; }
    const int covered_to = i == 0 ? 0 : starts[i - 1] + F;   // the first coordinate the windows before i leave uncovered
    if (st > covered_to) { snprintf(msg, sizeof msg, "no %s window covers %d", axis, covered_to); return msg; }
  }
  if (starts[n - 1] + F < total) { snprintf(msg, sizeof msg, "no %s window covers %d", axis, starts[n - 1] + F); return msg; }
  return nullptr;
}

int k5_launch_cfg_euler_tiles(float* img, const void* vc, const void* vu, float w, float dt, const k5_tile_plan& p, int T, int H, int W, int C,
                              hipStream_t s) {
  if (!img || !vc || !p.starts_t || !p.starts_y || !p.starts_x || !p.wt || !p.wy || !p.wx) return K5_ERR_ARG;
  if (p.nt < 1 || p.ny < 1 || p.nx < 1 || p.Ft < 1 || p.Fh < 1 || p.Fw < 1 || T < 1 || H < 1 || W < 1 || C < 1) return K5_ERR_ARG;
  if ((int64_t)p.nt * p.ny * p.nx > 64) return K5_ERR_ARG;
  if ((int64_t)T * H > 0x7fffffff || (int64_t)W * C > 0x7fffffff) return K5_ERR_ARG;   // the kernel counts rows, and a row's elements, in an int
  const auto misaligned = [](const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
  if (misaligned(img, 4) || misaligned(vc, 2) || misaligned(vu, 2) || misaligned(p.starts_t, 4) || misaligned(p.starts_y, 4) ||
      misaligned(p.starts_x, 4) || misaligned(p.wt, 4) || misaligned(p.wy, 4) || misaligned(p.wx, 4))
    return K5_ERR_ARG;
  // a lane owns four channels of one cell: 16-byte latent accesses, 8-byte velocity accesses, when C is whole groups of four and the bases allow it
  const bool vec = (C & 3) == 0 && !misaligned(img, 16) && !misaligned(vc, 8) && !misaligned(vu, 8);
  const int64_t n = (int64_t)T * H * 256;   // a workgroup per row of cells
  if (vec)
    hipLaunchKernelGGL(cfg_euler_tiles_kernel<4>, dim3(grid_for(n)), dim3(256), 0, s, img, (const bf16_t*)vc, (const bf16_t*)vu, w, dt, p, T, H, W, C);
  else
    hipLaunchKernelGGL(cfg_euler_tiles_kernel<1>, dim3(grid_for(n)), dim3(256), 0, s, img, (const bf16_t*)vc, (const bf16_t*)vu, w, dt, p, T, H, W, C);
  return done();
}

namespace {
// weight packing on the device (k5_dit_finalize): src [rows][cols] of dtype sdt (K5_F32 / K5_BF16 / K5_F16) -> dst [rows][ld] bf16 (RNE)
// or fp32; the columns cols .. ld of a padded destination are zeroed
template <bool DST_BF16>
__global__ __launch_bounds__(256) void pack_matrix_kernel(const void* __restrict__ src, int sdt, void* __restrict__ dst, int64_t rows,
                                                          int cols, int ld) {
  const int64_t total = rows * ld;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int64_t r = g / ld;
    const int c = (int)(g - r * ld);
    float v = 0.f;
    if (c < cols) {
      const int64_t si = r * cols + c;
      if (sdt == K5_F32) v = reinterpret_cast<const float*>(src)[si];
      else if (sdt == K5_BF16) v = __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(src)[si] << 16);
      else v = (float)reinterpret_cast<const _Float16*>(src)[si];
    }
    if (DST_BF16) reinterpret_cast<bf16_t*>(dst)[g] = f2bf(v);
    else reinterpret_cast<float*>(dst)[g] = v;
  }
}
}  // namespace

int k5_launch_pack_matrix(const void* src, int src_dtype, void* dst, int dst_bf16, int64_t rows, int cols, int ld, hipStream_t s) {
  if (!src || !dst || rows <= 0 || cols <= 0 || ld < cols) return K5_ERR_ARG;
  if (src_dtype != K5_F32 && src_dtype != K5_BF16 && src_dtype != K5_F16) return K5_ERR_ARG;
  const int64_t total = rows * ld;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  if (dst_bf16) hipLaunchKernelGGL(pack_matrix_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, src, src_dtype, dst, rows, cols, ld);
  else hipLaunchKernelGGL(pack_matrix_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, src, src_dtype, dst, rows, cols, ld);
  return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP;
}

int k5_launch_cast_f32_bf16(const float* x, void* out, int64_t n, hipStream_t s) {
  if (n <= 0) return K5_ERR_ARG;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, (bf16_t*)out, n);
  return done();
}

namespace {
// LoRA merge (k5_dit_add_lora, k5_lora_merge): W[n][k] += s * sum_r B[n][r] A[r][k], in place on a packed [rows][ld] matrix.
// The bits are spelled out so that they depend neither on the tiling nor on -ffp-contract: acc = fma(B[n][r], A[r][k], acc) for r = 0 .. R-1 in
// that order from acc = 0, then fma(s, acc, W[n][k]), rounded to fp32 and from there to the matrix's type (nearest-even both; the fp32 step can turn a bf16
// rounding at an exact fp32 tie, 2^-16 of the elements, never past a neighbour).  The chain runs in
// FLOAT64 (the factors are exact in it; explicit builtins): the same chain in fp32 carries an absolute error of R * 2^-24 * sum|B||A|, and where W and
// the update cancel (|W'| ~ 1e-6 against terms of 1e-2) that is ten bf16 steps — 2 of 131 072 outputs of a 256 x 512, R = 128 merge then miss
// both bf16 neighbours of the exact value (measured, and reproduced by an fp32 emulation on the host).  v_fma_f64 runs at half the fp32 VALU rate
// on gfx950, and the pass is dominated by reading and writing W either way.  No MFMA: a bf16 MFMA would round the factors.
// A workgroup owns 64 rows x 128 columns; a thread 4 rows x 8 columns; the factors come through LDS as fp32 in slabs of 32 ranks.
//   As[r][slot]: column k of the tile sits at slot ((k >> 2) & 1) * 64 + (k >> 3) * 4 + (k & 3), so the two 16-byte reads of a thread's
//                8 columns are each contiguous over the 16 lanes that share a row group (a whole 256-byte bank row: no conflict)
//   Bs[r][n]:    transposed, 4 consecutive rows per 16-byte read (4 distinct addresses per wave, broadcast); row stride 68 floats keeps
//                the reads 16-byte aligned and spreads the transposing writes over 8 banks
constexpr int LM_ROWS = 64, LM_COLS = 128, LM_RC = 32, LM_BLD = 68;

K5_DEV float lora_factor(const void* p, int dt, int64_t i) {
  if (dt == K5_F32) return reinterpret_cast<const float*>(p)[i];
  if (dt == K5_BF16) return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(p)[i] << 16);
  return (float)reinterpret_cast<const _Float16*>(p)[i];
}

template <typename T>   // T = bf16_t or float: the packed matrix
__global__ __launch_bounds__(256) void lora_merge_kernel(T* W, int rows, int cols, int64_t ld, const void* __restrict__ A, int adt,
                                                         const void* __restrict__ B, int bdt, int R, float s, int tiles_n) {
  __shared__ __attribute__((aligned(16))) float As[LM_RC][LM_COLS];
  __shared__ __attribute__((aligned(16))) float Bs[LM_RC][LM_BLD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int tm = (int)blockIdx.x / tiles_n, tn = (int)blockIdx.x - tm * tiles_n;
  const int row0 = tm * LM_ROWS, col0 = tn * LM_COLS;
  double acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;
  for (int r0 = 0; r0 < R; r0 += LM_RC) {
    const int rc = R - r0 < LM_RC ? R - r0 : LM_RC;
    if (r0) __syncthreads();
    for (int i = tid; i < LM_RC * LM_COLS; i += 256) {
      const int r = i >> 7, k = i & (LM_COLS - 1);
      float v = 0.f;
      if (r < rc && col0 + k < cols) v = lora_factor(A, adt, (int64_t)(r0 + r) * cols + col0 + k);
      As[r][((k >> 2) & 1) * 64 + (k >> 3) * 4 + (k & 3)] = v;
    }
    for (int i = tid; i < LM_ROWS * LM_RC; i += 256) {
      const int n = i >> 5, r = i & (LM_RC - 1);
      float v = 0.f;
      if (r < rc && row0 + n < rows) v = lora_factor(B, bdt, (int64_t)(row0 + n) * R + r0 + r);
      Bs[r][n] = v;
    }
    __syncthreads();
    // exactly rc ranks: a padded rank would add a signed zero to the chain
#pragma unroll 4
    for (int r = 0; r < rc; ++r) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(&As[r][tx * 4]);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(&As[r][64 + tx * 4]);
      const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[r][ty * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = __builtin_fma((double)b[i], (double)a0[j], acc[i][j]);
          acc[i][4 + j] = __builtin_fma((double)b[i], (double)a1[j], acc[i][4 + j]);
        }
    }
  }
  const int c = col0 + tx * 8;
  const double sd = (double)s;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + ty * 4 + i;
    if (row >= rows || c >= cols) continue;
    T* p = W + (int64_t)row * ld + c;
    if (c + 8 <= cols && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {   // 16-byte accesses where the row start allows them
      if constexpr (sizeof(T) == 2) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(p);
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          o[q] = pack_bf16x2((float)__builtin_fma(sd, acc[i][2 * q], (double)__uint_as_float(w[q] << 16)),
                             (float)__builtin_fma(sd, acc[i][2 * q + 1], (double)__uint_as_float(w[q] & 0xffff0000u)));
        *reinterpret_cast<u32x4*>(p) = o;
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          f32x4 w = *reinterpret_cast<const f32x4*>(p + 4 * h);
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = (float)__builtin_fma(sd, acc[i][4 * h + j], (double)w[j]);
          *reinterpret_cast<f32x4*>(p + 4 * h) = w;
        }
      }
    } else {   // ragged edge, or a row that does not start on 16 bytes: element by element, never past column cols - 1
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c + j < cols) p[j] = (T)(float)__builtin_fma(sd, acc[i][j], (double)(float)p[j]);
    }
  }
}
}  // namespace

int k5_launch_lora_merge(void* W, int w_dtype, int rows, int cols, int ld, const void* A, int a_dtype, const void* B, int b_dtype, int R,
                         float scale, hipStream_t s) {
  if (!W || !A || !B || rows <= 0 || cols <= 0 || ld < cols || R < 1 || R > 256) return K5_ERR_ARG;
  if (w_dtype != K5_F32 && w_dtype != K5_BF16) return K5_ERR_ARG;
  for (int dt : {a_dtype, b_dtype})
    if (dt != K5_F32 && dt != K5_BF16 && dt != K5_F16) return K5_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(W) & (w_dtype == K5_F32 ? 3 : 1)) return K5_ERR_ALIGN;
  if ((reinterpret_cast<uintptr_t>(A) & (a_dtype == K5_F32 ? 3 : 1)) || (reinterpret_cast<uintptr_t>(B) & (b_dtype == K5_F32 ? 3 : 1))) return K5_ERR_ALIGN;
  if (scale == 0.f) return K5_OK;   // nothing to add: nothing launched
  const int tiles_n = (cols + LM_COLS - 1) / LM_COLS;
  const int64_t blocks = (int64_t)((rows + LM_ROWS - 1) / LM_ROWS) * tiles_n;
  if (blocks > 0x7fffffff) return K5_ERR_ARG;
  if (w_dtype == K5_BF16)
    hipLaunchKernelGGL(lora_merge_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, (bf16_t*)W, rows, cols, (int64_t)ld, A, a_dtype, B,
                       b_dtype, R, scale, tiles_n);
  else
    hipLaunchKernelGGL(lora_merge_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, (float*)W, rows, cols, (int64_t)ld, A, a_dtype, B,
                       b_dtype, R, scale, tiles_n);
  return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------
// (kept at the end of the file: the kernels above stay where they were in the code object)
namespace {

// Live preview of the sampler (the watch of k5_dit_set_watch, k5_x0_preview): after the update of a step the latent x sits at sigma_next and the
// velocity buffers still hold that step's velocities, so the denoised estimate of flow matching is x0 = x - sigma_next * v with v combined by
// cfg_velocity (the step kernel's combine).  The product and the difference round to fp32 each on its own
// (nothing contracted), sigma_next == 0 hands x through, and with a keep mask x0 = keep_blend(x0, source, m): kept cells show the source.
__device__ __forceinline__ float x0_estimate(float x, float sigma, float v) {
#pragma clang fp contract(off)
  const float p = sigma * v;
  return x - p;
}

// Four lanes per latent cell (a quad), one 16-byte load of the latent per lane and round: lane q of the quad owns the 4-channel chunks q, q + 4,
// q + 8, q + 12 of its cell, so a quad reads 64 consecutive bytes and (C = 16) a wave 1 KiB.  RGB: rgb[j] = sat_u8(rint((b[j] + sum_k W[k][j]
// x0[k]) * 127.5 + 127.5)), NaN -> 0.  The order of the sum is fixed: lane q runs acc = fma(W[k][j], x0[k], acc) from acc = 0 over its own
// channels in ascending k; then s = acc + acc(lane ^ 1), s = s + s(lane ^ 2) — the same bits in all four lanes, fp32 addition commutes —
// t = b[j] + s and one fma(t, 127.5, 127.5).  Lanes 0..2 of the quad store one byte each.  Every lane of a wave reaches the two exchanges (a
// lane past the last cell carries zeros and stores nothing): a wave-wide exchange must not sit under a lane-dependent branch.
__global__ __launch_bounds__(256) void x0_preview_kernel(const float* __restrict__ x, const bf16_t* __restrict__ vc,
                                                         const bf16_t* __restrict__ vu, float w, float sigma_next,
                                                         const float* __restrict__ source, const float* __restrict__ mask,
                                                         const float* __restrict__ rgb_w, const float* __restrict__ rgb_b,
                                                         float* __restrict__ x0_out, uint8_t* __restrict__ rgb, int C, int64_t cells) {
  __shared__ float sw[64 * 3 + 3];   // W [C][3], then b [3]
  for (int i = threadIdx.x; i < 3 * C + 3; i += 256)
    sw[i] = !rgb_w ? 0.f : (i < 3 * C ? rgb_w[i] : (rgb_b ? rgb_b[i - 3 * C] : 0.f));
  __syncthreads();
  const int q = threadIdx.x & 3, nch = C >> 2;
  const int64_t rounds = (cells + 63) / 64;   // 64 cells per workgroup and round
  for (int64_t r = blockIdx.x; r < rounds; r += gridDim.x) {
    const int64_t cell = r * 64 + (threadIdx.x >> 2);
    const bool live = cell < cells;
    float acc[3] = {0.f, 0.f, 0.f};
    if (live) {
      const float m = mask ? mask[cell] : 0.0f;
      for (int ch = q; ch < nch; ch += 4) {
        const int64_t e = cell * C + 4 * ch;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + e);
        const u32x2 cr = *reinterpret_cast<const u32x2*>(vc + e);
        u32x2 ur = {0u, 0u};
        if (vu) ur = *reinterpret_cast<const u32x2*>(vu + e);
        f32x4 sv = {0.f, 0.f, 0.f, 0.f};
        if (m != 0.0f) sv = *reinterpret_cast<const f32x4*>(source + e);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float v = bf16_at(cr, k);
          if (vu) v = cfg_velocity(w, v, bf16_at(ur, k));
          float z = sigma_next == 0.0f ? xv[k] : x0_estimate(xv[k], sigma_next, v);
          if (m != 0.0f) z = keep_blend(z, sv[k], m);
          o[k] = z;
          const float* wk = sw + (4 * ch + k) * 3;
          acc[0] = fmaf(wk[0], z, acc[0]); acc[1] = fmaf(wk[1], z, acc[1]); acc[2] = fmaf(wk[2], z, acc[2]);
        }
        if (x0_out) *reinterpret_cast<f32x4*>(x0_out + e) = o;
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      acc[j] = acc[j] + __shfl_xor(acc[j], 1);
      acc[j] = acc[j] + __shfl_xor(acc[j], 2);
    }
    if (live && rgb && q < 3) {
      const float s = q == 0 ? acc[0] : (q == 1 ? acc[1] : acc[2]);
      const float val = rintf(fmaf(sw[3 * C + q] + s, 127.5f, 127.5f));
      rgb[cell * 3 + q] = !(val >= 0.0f) ? (uint8_t)0 : (val > 255.0f ? (uint8_t)255 : (uint8_t)val);   // NaN fails the first test
    }
  }
}

}  // namespace

int k5_launch_x0_preview(const float* x, const void* vc, const void* vu, float w, float sigma_next, const float* source,
                         const float* keep_mask, const float* rgb_w, const float* rgb_b, float* x0_out, uint8_t* rgb, int64_t cells, int C,
                         hipStream_t s) {
  if (C <= 0 || (C & 3) || C > 64) return K5_ERR_UNSUPPORTED;   // a quad's 16-byte loads and the LDS copy of W
  if (!x || !vc || cells <= 0 || (!rgb && !x0_out) || ((rgb != nullptr) != (rgb_w != nullptr)) || (keep_mask && !source)) return K5_ERR_ARG;
  const auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  if (misaligned(x, 16) || misaligned(x0_out, 16) || (keep_mask && misaligned(source, 16)) || misaligned(vc, 8) || misaligned(vu, 8) ||
      misaligned(keep_mask, 4) || misaligned(rgb_w, 4) || misaligned(rgb_b, 4))
    return K5_ERR_ARG;
  hipLaunchKernelGGL(x0_preview_kernel, dim3(grid_for(cells, 64)), dim3(256), 0, s, x, (const bf16_t*)vc, (const bf16_t*)vu, w, sigma_next,
                     keep_mask ? source : nullptr, keep_mask, rgb_w, rgb_b, x0_out, rgb, C, cells);
  return done();
}

// ---------------------------------------------------------------------------------------------
namespace {

// Normalized attention guidance (k5_nag_combine_bf16): z_pos / z_neg are the outputs of one cross-attention against the positive
// and the negative text, same queries.  Per row, fp32, every operation rounded on its own except the one named fma:
//   d = zp - zn;  g = fma(s - 1, d, zp);  n_pos = sum |zp|,  n_g = sum |g| over the D channels;
//   f = n_g <= tau * n_pos ? 1 : (tau * n_pos) / n_g;  out = bf16(zp + alpha * (f * g - zp))
// zn == zp, s == 1 and alpha == 0 each give zp bit for bit (d or s - 1 is 0, so g is zp, the two sums are the same additions and f is 1; alpha *
// (f * g - zp) is then an exact 0, and an exact 0 hands zp through with its sign); finite inputs give no NaN (n_g > tau * n_pos >= 0 before the division).
// One wave per row (the ln_kernel shape): a lane's up to MAXC 16-byte chunks of both inputs are loaded in one burst, the row stays in
// registers between the sums and the store, so each input is read once and out written once; out may be z_pos (or z_neg): a lane has read a
// chunk before it writes it and no other lane touches it.  Order of the sums: a lane adds its elements in ascending column order from 0, then
// the xor butterfly of wave_sum — the same bits on every launch.  D = 128 keeps 16 of the 64 lanes busy: those rows are 256 bytes, nothing to win.
// The blend's product, difference, product and sum must not contract (nag_blend, under `#pragma clang fp contract(off)` like x0_estimate).
__device__ __forceinline__ float nag_blend(float p, float g, float f, float alpha) {
#pragma clang fp contract(off)
  const float fg = f * g;
  const float t = fg - p;
  const float at = alpha * t;
  return at == 0.0f ? p : p + at;   // p + 0 would turn a -0 of z_pos into +0
}

__global__ __launch_bounds__(256) void nag_combine_kernel(const bf16_t* zp, const bf16_t* zn, bf16_t* out, int rows, int D, int ld,
                                                          float sm1, float tau, float alpha) {
  const int lane = threadIdx.x & 63, nch = D >> 3;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;   // wave-uniform
  const size_t base = (size_t)row * ld;
  u32x4 rp[MAXC], rn[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int ch = lane + 64 * i;
    if (ch < nch) {
      rp[i] = *reinterpret_cast<const u32x4*>(zp + base + 8 * ch);
      rn[i] = *reinterpret_cast<const u32x4*>(zn + base + 8 * ch);
    }
  }
  float g[MAXC][8];
  float n_pos = 0.f, n_g = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    if (lane + 64 * i < nch) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = bf16_at(rp[i], j), q = bf16_at(rn[i], j);
        g[i][j] = fmaf(sm1, __fsub_rn(p, q), p);
        n_pos = __fadd_rn(n_pos, fabsf(p));
        n_g = __fadd_rn(n_g, fabsf(g[i][j]));
      }
    }
  }
  n_pos = wave_sum(n_pos); n_g = wave_sum(n_g);   // every lane of the wave is here (a lane without chunks carries zeros)
  const float cap = __fmul_rn(tau, n_pos);
  const float f = n_g <= cap ? 1.0f : __fdiv_rn(cap, n_g);
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int ch = lane + 64 * i;
    if (ch < nch) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o[j] = nag_blend(bf16_at(rp[i], j), g[i][j], f, alpha);
      }
      const u32x4 pk = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
      *reinterpret_cast<u32x4*>(out + base + 8 * ch) = pk;
    }
  }
}

}  // namespace

int k5_launch_nag_combine(const void* z_pos, const void* z_neg, void* out, int rows, int D, int ld, float s, float tau, float alpha,
                          hipStream_t stream) {
  if (!z_pos || !z_neg || !out || rows <= 0 || D <= 0 || ld < D || !(s >= 1.0f) || !(tau >= 1.0f) || !(alpha >= 0.0f && alpha <= 1.0f))
    return K5_ERR_ARG;
  const auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  if ((D & 7) || (ld & 7) || misaligned(z_pos) || misaligned(z_neg) || misaligned(out)) return K5_ERR_ARG;
  if (D > 64 * 8 * MAXC) return K5_ERR_UNSUPPORTED;   // the register-resident row
  hipLaunchKernelGGL(nag_combine_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, (const bf16_t*)z_pos, (const bf16_t*)z_neg, (bf16_t*)out,
                     rows, D, ld, s - 1.0f, tau, alpha);
  return done();
}

// ---------------------------------------------------------------------------------------------
namespace {

// Regional prompts (k5_region_combine_bf16): z_0 .. z_R are the outputs of one cross-attention against the base text and R region
// texts, same queries; w is the row's R + 1 token weights.  Per element, fp32: the first stream with a non-zero weight gives acc = w z (one
// rounded product), every later non-zero one acc = fmaf(w, z, acc), ascending from the base stream; out = bf16(acc) once.  A stream whose weight
// is exactly 0 for the row is not read (NaN there does not reach out); a row whose only non-zero weight is 1.0 is that stream's bits (1 z is z,
// the sign of a zero included, and a bf16 value rounds to itself); a row without a non-zero weight is +0.
// One wave per row (the nag_combine_kernel shape): the weights are per row, so the skip is wave-uniform; a used stream's up to MAXC 16-byte
// chunks per lane are loaded in one burst, the accumulator row stays in registers, out is written once.  out may be z_0 (or any z_r): a lane
// has read every chunk it writes and no other lane touches it.  The product and the fma must stay what they are written as (region_first /
// region_next, under `#pragma clang fp contract(off)` like nag_blend).
__device__ __forceinline__ float region_first(float w, float z) {
#pragma clang fp contract(off)
  return w * z;
}
__device__ __forceinline__ float region_next(float w, float z, float acc) {
#pragma clang fp contract(off)
  return fmaf(w, z, acc);
}

__global__ __launch_bounds__(256) void region_combine_kernel(const bf16_t* z0, const bf16_t* zr, long long zr_stride, int R, const float* w, int ldw,
                                                             bf16_t* out, int rows, int D, int ld) {
  const int lane = threadIdx.x & 63, nch = D >> 3;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;   // wave-uniform
  const size_t base = (size_t)row * ld;
  float acc[MAXC][8];
#pragma unroll
  for (int i = 0; i < MAXC; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  bool first = true;
  for (int k = 0; k <= R; ++k) {
    const float wk = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(w[(size_t)row * ldw + k])));   // one value per wave
    if (wk == 0.0f) continue;
    const bf16_t* z = (k == 0 ? z0 : zr + (size_t)(k - 1) * zr_stride) + base;
    u32x4 raw[MAXC];
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int ch = lane + 64 * i;
      if (ch < nch) raw[i] = *reinterpret_cast<const u32x4*>(z + 8 * ch);
    }
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      if (lane + 64 * i < nch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = bf16_at(raw[i], j);
          acc[i][j] = first ? region_first(wk, v) : region_next(wk, v, acc[i][j]);
        }
      }
    }
    first = false;
  }
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int ch = lane + 64 * i;
    if (ch < nch) {
      const u32x4 pk = {pack_bf16x2(acc[i][0], acc[i][1]), pack_bf16x2(acc[i][2], acc[i][3]), pack_bf16x2(acc[i][4], acc[i][5]),
                        pack_bf16x2(acc[i][6], acc[i][7])};
      *reinterpret_cast<u32x4*>(out + base + 8 * ch) = pk;
    }
  }
}

// Token weights of the regional prompts (k5_region_weights_f32): one thread per token i of the engine's order, token perm[i] (or i) of the
// row-major (T / pt, H / ph, W / pw) token grid.  m_r = mean of the token's pt ph pw cells of mask r, each cell clamped to [0, 1] (a NaN cell counts as 0), added
// in ascending (t, h, w) order and divided by the count; sm = m_1 + .. + m_R ascending; raw_0 = base_weight + max(0, 1 - sm);
// s = raw_0 + m_1 + .. + m_R ascending (>= 1); w_0 = raw_0 / s, w_r = m_r / s.  Every operation rounded on its own, no atomics.
__global__ __launch_bounds__(256) void region_weights_kernel(const float* masks, int R, int T, int H, int W, int pt, int ph, int pw, float bw,
                                                             const int32_t* perm, float* w, int N) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int Hp = H / ph, Wp = W / pw;
  const int tok = perm ? perm[i] : i;
  const int tw = tok % Wp, th = (tok / Wp) % Hp, tt = tok / (Wp * Hp);
  const float cells = (float)(pt * ph * pw);
  float m[8];
  float sm = 0.f;
  for (int r = 0; r < 8; ++r) {
    m[r] = 0.f;
    if (r < R) {
      float a = 0.f;
      for (int dt = 0; dt < pt; ++dt)
        for (int dh = 0; dh < ph; ++dh)
          for (int dw = 0; dw < pw; ++dw) {
            const float c = masks[(((size_t)r * T + (size_t)(tt * pt + dt)) * H + (size_t)(th * ph + dh)) * W + (size_t)(tw * pw + dw)];
            a += fminf(fmaxf(c, 0.f), 1.f);
          }
      m[r] = a / cells;
      sm += m[r];
    }
  }
  const float raw0 = bw + fmaxf(0.f, 1.f - sm);
  float s = raw0;
  for (int r = 0; r < 8; ++r)
    if (r < R) s += m[r];
  float* wi = w + (size_t)i * (R + 1);
  wi[0] = raw0 / s;
  for (int r = 0; r < 8; ++r)
    if (r < R) wi[r + 1] = m[r] / s;
}

}  // namespace

int k5_launch_region_combine(const void* z0, const void* zr, long long zr_stride, int R, const float* w, int ldw, void* out, int rows, int D,
                             int ld, hipStream_t stream) {
  if (!z0 || !zr || !w || !out || rows <= 0 || D <= 0 || ld < D || R < 1 || R > 8 || ldw < R + 1) return K5_ERR_ARG;
  const auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  if ((D & 7) || (ld & 7) || (zr_stride & 7) || misaligned(z0) || misaligned(zr) || misaligned(out) || (reinterpret_cast<uintptr_t>(w) & 3))
    return K5_ERR_ARG;
  if (D > 64 * 8 * MAXC) return K5_ERR_UNSUPPORTED;   // the register-resident row
  hipLaunchKernelGGL(region_combine_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, (const bf16_t*)z0, (const bf16_t*)zr, zr_stride, R, w, ldw,
                     (bf16_t*)out, rows, D, ld);
  return done();
}

int k5_launch_region_weights(const float* masks, int R, int T, int H, int W, int pt, int ph, int pw, float base_weight, const int32_t* perm,
                             float* w, hipStream_t stream) {
  if (!masks || !w || R < 1 || R > 8 || T < 1 || H < 1 || W < 1 || pt < 1 || ph < 1 || pw < 1 || (T % pt) || (H % ph) || (W % pw)) return K5_ERR_ARG;
  if (!(base_weight >= 0.0f && base_weight <= 1.0f)) return K5_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(masks) & 3) || (reinterpret_cast<uintptr_t>(w) & 3) || (reinterpret_cast<uintptr_t>(perm) & 3)) return K5_ERR_ARG;
  const long long N = (long long)(T / pt) * (H / ph) * (W / pw);
  if (N > 0x7fffffffLL || (long long)T * H * W > 0x7fffffffLL) return K5_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(region_weights_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, masks, R, T, H, W, pt, ph, pw, base_weight, perm,
                     w, (int)N);
  return done();
}
