// forecast.hip — the forecast cache (TaylorSeer "lite", Liu et al. 2025): the two passes around the visual blocks.  The rule is written once
// in include/k5.h (k5_forecast_update_bf16).
//   forecast_update_kernel   a full call: r = bf16(vis - ori) and the finite differences of r against the slot's history, one pass
//   forecast_apply_kernel    a forecast call: vis += F0 + c1 D1 + c2 D2 in place of the residual add (c1 = k, c2 = k (k + g) g / (g + gp))
// Both: 16 bytes of bf16 (8 elements) per lane and iteration, grid-stride, no atomics and no reduction, so equal inputs give equal bits.  vis is
// [rows][ld] (D columns used), the state and ori are [rows][D] flat.  Every product, quotient and sum is one fp32 operation rounded on its
// own.  __fmul_rn / __fadd_rn are plain * and + to hipcc, which contracts by default, so the one place where a product meets a sum
// (add_scaled) carries `#pragma clang fp contract(off)` — it holds under hipcc's default mode only; build.py adds no -ffp-contract (README,
// round 6).  The differences and quotients of the update pass have no product to fuse; x + (-1 * y) has an exact product.
#include "k5_common.h"
#include "k5_kernels.h"

namespace {

inline int done() { return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP; }
bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// one sweep covers 1024 x 256 lanes x 8 elements (2 097 152); the loop takes the rest.  16 waves per CU keep ~80 bytes per lane in flight.
inline unsigned grid_of(int64_t chunks) {
  const int64_t blocks = (chunks + 255) / 256;
  return (unsigned)(blocks > 1024 ? 1024 : blocks);
}

K5_DEV int64_t vis_offset(int64_t g, int nch, int ld) {
  if (ld == 8 * nch) return g * 8;   // flat rows (the engine's): no division
  const int64_t row = g / nch;
  return row * ld + (g - row * nch) * 8;
}

K5_DEV void unpack8(const u32x4& v, float (&o)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { o[2 * j] = __uint_as_float(v[j] << 16); o[2 * j + 1] = __uint_as_float(v[j] & 0xffff0000u); }
}

// p + c * d with the product and the sum rounded to fp32 each on its own
K5_DEV float add_scaled(float p, float c, float d) {
#pragma clang fp contract(off)
  const float q = c * d;
  return p + q;
}

// LEVEL = min(order, have): 0 writes F0 alone, 1 also D1 = (r - F0) / g, 2 also D2 = (D1' - D1) / g.  A lane reads its chunk of F0 / D1 before
// it writes that chunk and no other lane touches it, so the state is updated in place.
template <int LEVEL>
__global__ __launch_bounds__(256) void forecast_update_kernel(const bf16_t* __restrict__ vis, int ld, const bf16_t* __restrict__ ori, bf16_t* F0,
                                                              float* D1, float* D2, int64_t total, int nch, float g) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < total; c += (int64_t)gridDim.x * 256) {
    const u32x4 rv = *reinterpret_cast<const u32x4*>(vis + vis_offset(c, nch, ld));
    const u32x4 ro = *reinterpret_cast<const u32x4*>(ori + c * 8);
    u32x4 rf;
    f32x4 a0, a1;
    if (LEVEL >= 1) rf = *reinterpret_cast<const u32x4*>(F0 + c * 8);
    if (LEVEL >= 2) { a0 = *reinterpret_cast<const f32x4*>(D1 + c * 8); a1 = *reinterpret_cast<const f32x4*>(D1 + c * 8 + 4); }
    float v[8], o[8], r[8];
    unpack8(rv, v); unpack8(ro, o);
    u32x4 pk;
#pragma unroll
    for (int j = 0; j < 4; ++j)   // x + (-1 * y), as gate_sum_kernel forms it
      pk[j] = pack_bf16x2(__fadd_rn(v[2 * j], __fmul_rn(-1.0f, o[2 * j])), __fadd_rn(v[2 * j + 1], __fmul_rn(-1.0f, o[2 * j + 1])));
    *reinterpret_cast<u32x4*>(F0 + c * 8) = pk;
    if (LEVEL >= 1) {
      float f[8], d1[8];
      unpack8(pk, r); unpack8(rf, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) d1[j] = __fdiv_rn(__fsub_rn(r[j], f[j]), g);
      if (LEVEL >= 2) {
        f32x4 b0, b1;
#pragma unroll
        for (int j = 0; j < 4; ++j) { b0[j] = __fdiv_rn(__fsub_rn(d1[j], a0[j]), g); b1[j] = __fdiv_rn(__fsub_rn(d1[4 + j], a1[j]), g); }
        *reinterpret_cast<f32x4*>(D2 + c * 8) = b0;
        *reinterpret_cast<f32x4*>(D2 + c * 8 + 4) = b1;
      }
      *reinterpret_cast<f32x4*>(D1 + c * 8) = f32x4{d1[0], d1[1], d1[2], d1[3]};
      *reinterpret_cast<f32x4*>(D1 + c * 8 + 4) = f32x4{d1[4], d1[5], d1[6], d1[7]};
    }
  }
}

// M = min(order, have - 1) terms of the series.  M = 0 is gate_sum_kernel with a gate of +1: x + (1 * y), the product being exact.
template <int M>
__global__ __launch_bounds__(256) void forecast_apply_kernel(bf16_t* vis, int ld, const bf16_t* __restrict__ F0, const float* __restrict__ D1,
                                                             const float* __restrict__ D2, int64_t total, int nch, float c1, float c2) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < total; c += (int64_t)gridDim.x * 256) {
    const int64_t off = vis_offset(c, nch, ld);
    const u32x4 rv = *reinterpret_cast<const u32x4*>(vis + off);
    const u32x4 rf = *reinterpret_cast<const u32x4*>(F0 + c * 8);
    float v[8], p[8];
    unpack8(rv, v); unpack8(rf, p);
    if (M >= 1) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(D1 + c * 8), a1 = *reinterpret_cast<const f32x4*>(D1 + c * 8 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { p[j] = add_scaled(p[j], c1, a0[j]); p[4 + j] = add_scaled(p[4 + j], c1, a1[j]); }
    }
    if (M >= 2) {
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(D2 + c * 8), b1 = *reinterpret_cast<const f32x4*>(D2 + c * 8 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { p[j] = add_scaled(p[j], c2, b0[j]); p[4 + j] = add_scaled(p[4 + j], c2, b1[j]); }
    }
    u32x4 pk;
#pragma unroll
    for (int j = 0; j < 4; ++j) pk[j] = pack_bf16x2(__fadd_rn(v[2 * j], p[2 * j]), __fadd_rn(v[2 * j + 1], p[2 * j + 1]));
    *reinterpret_cast<u32x4*>(vis + off) = pk;
  }
}

bool bad_vis(const void* vis, int rows, int D, int ld) {
  return !vis || rows <= 0 || D <= 0 || (D & 7) || ld < D || (ld & 7) || misaligned16(vis);
}

}  // namespace

int k5_launch_forecast_update(const void* vis, int ld, const void* ori, void* F0, float* D1, float* D2, int rows, int D, int g, int order, int have,
                              hipStream_t stream) {
  if (bad_vis(vis, rows, D, ld) || !ori || !F0 || misaligned16(ori) || misaligned16(F0)) return K5_ERR_ARG;
  if (order < 0 || order > 2 || have < 0 || g < 1) return K5_ERR_ARG;
  const int level = have < order ? have : order;
  if ((level >= 1 && (!D1 || misaligned16(D1))) || (level >= 2 && (!D2 || misaligned16(D2)))) return K5_ERR_ARG;
  const int64_t total = (int64_t)rows * (D >> 3);
  const dim3 grid(grid_of(total)), block(256);
  const bf16_t* v = (const bf16_t*)vis; const bf16_t* o = (const bf16_t*)ori; bf16_t* f = (bf16_t*)F0;
  if (level == 0) hipLaunchKernelGGL(forecast_update_kernel<0>, grid, block, 0, stream, v, ld, o, f, D1, D2, total, D >> 3, (float)g);
  else if (level == 1) hipLaunchKernelGGL(forecast_update_kernel<1>, grid, block, 0, stream, v, ld, o, f, D1, D2, total, D >> 3, (float)g);
  else hipLaunchKernelGGL(forecast_update_kernel<2>, grid, block, 0, stream, v, ld, o, f, D1, D2, total, D >> 3, (float)g);
  return done();
}

int k5_launch_forecast_apply(void* vis, int ld, const void* F0, const float* D1, const float* D2, int rows, int D, int k, int g, int gp, int order,
                             int have, hipStream_t stream) {
  if (bad_vis(vis, rows, D, ld) || !F0 || misaligned16(F0)) return K5_ERR_ARG;
  if (order < 0 || order > 2 || have < 1 || k < 1) return K5_ERR_ARG;
  const int m = have - 1 < order ? have - 1 : order;
  if ((m >= 1 && (!D1 || misaligned16(D1))) || (m >= 2 && (!D2 || misaligned16(D2) || g < 1 || gp < 1))) return K5_ERR_ARG;
  const int64_t total = (int64_t)rows * (D >> 3);
  const dim3 grid(grid_of(total)), block(256);
  // Newton's backward form on the stored differences: D2 = (d1' - d1) / g is the second divided difference times (g + gp) / g
  const float c1 = (float)k, c2 = m >= 2 ? (float)((double)k * (double)(k + g) * (double)g / (double)(g + gp)) : 0.0f;
  bf16_t* v = (bf16_t*)vis; const bf16_t* f = (const bf16_t*)F0;
  if (m == 0) hipLaunchKernelGGL(forecast_apply_kernel<0>, grid, block, 0, stream, v, ld, f, D1, D2, total, D >> 3, c1, c2);
  else if (m == 1) hipLaunchKernelGGL(forecast_apply_kernel<1>, grid, block, 0, stream, v, ld, f, D1, D2, total, D >> 3, c1, c2);
  else hipLaunchKernelGGL(forecast_apply_kernel<2>, grid, block, 0, stream, v, ld, f, D1, D2, total, D >> 3, c1, c2);
  return done();
}
