// gemm_fp8.hip — W8A8 fp8 (OCP e4m3) GEMM for the feed-forward projections (BASELINE config 5: "fp8 MFMA weights"), opt-in.
//
//   C[m][n] = epilogue( w_scale[n] * sum_k A8[m][k] * W8[n][k] )        A8 [M][K] fp8, W8 [N][K] fp8, fp32 accumulate
//
// on v_mfma_scale_f32_16x16x128_f8f6f4 (2x the bf16 MFMA rate; block scales fixed to 2^0 — plain fp8 operands).  Operand
// layout verified on hardware (tools/probes/mfma_fp8_layout.hip): lane l holds row l&15, k = 32 (l>>4) .. +31 (32 bytes);
// D as for 16x16x32.  Structure = gemm_bf16_k8_kernel (gemm_bf16.hip): 256x256 tile, K-tile = 128 fp8 = 128 B per row (the
// same bytes as the bf16 kernel's K = 64), persistent workgroups, two groups of four waves ping-ponging by one barrier,
// LDS-DMA staging with counted vmcnt.  Because one MFMA consumes the whole K-tile, a phase is an output QUADRANT of the
// wave's 128 x 64 tile and the staging units are ROW halves laid out so that
//     ph1 (n-tiles 0-3, m-tiles 0-1) needs W-half0 + X-half0,  ph2 (.., m 2-3) X-half1,  ph3 (n 4-7, m 2-3) W-half1,  ph4 re-reads X-half0
// (a wave's n-tiles 0-3 are W rows [64 wn, +64), 4-7 rows [128 + 64 wn, +64); m-tiles 0-1 X rows [32 wm, +32), 2-3 rows
// [128 + 32 wm, +32)).  DMA issue, one half-tile (2 instructions per thread) per phase, >= 4 phases before first use:
//     ph1: X0(t+1)   ph2: X1(t+1)   ph3: W1(t+1)   ph4: W0(t+2)        every phase ends with s_waitcnt vmcnt(4) + barrier
// Restaging distances: X1 last read ph2, W1 ph3, W0 ph1 (>= 3 phases before the slot's next DMA); X0 is last read in ph4 and
// restaged in the next ph1 — legal because every phase retires its fragment reads (lgkmcnt(0)) BEFORE its first barrier.  LDS rows are 128 B with the chunk swizzle c ^ ((row>>1)&7) (a lane's 32 operand
// bytes are the chunk pair {2g, 2g+1}: two conflict-free ds_read_b128).
//
// Quantisation (k5_launch_quant_rows_fp8): weights per output channel (scale = max|w| / 448), activations with the static
// scale 1 (LayerNorm-modulated inputs and GELU outputs sit well inside e4m3's range; values beyond +-448 saturate).
#include <stdlib.h>

#include <type_traits>

#include "k5_common.h"
#include "k5_kernels.h"

void k5_set_error(const char* fmt, ...);   // engine.hip: the text behind k5_last_error

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;

constexpr int F8_BM = 256, F8_BN = 256, F8_BK = 128;          // BK in fp8 elements = bytes
constexpr int F8_UNIT = 16384, F8_XOFF = 65536, F8_LDS = 131072;   // W units at (2 stage + half) * 16 KB, X units 64 KB above

struct Gemm8P {
  const uint8_t* A; const uint8_t* W; void* C;
  const float* w_scale;   // per n (per m when scale_m: the operand-swapped V^T projection, whose weights are the "A" rows)
  const float* bias;      // nullable; per n, or per m when scale_m (fp32 holding bf16-rounded values, as in the bf16 GEMM)
  int scale_m;
  const bf16_t* resid; const float* gate;   // EPI_GATE
  int M, N, K, lda, ldw, ldc, ldr;
  int tiles_m, tiles_n, lid_limit;
};


// EPI: K5_EPI_BIAS -> bf16 out (no bias: FF layers have none), K5_EPI_GELU -> fp8 out = e4m3(GELU(bf16(acc * s))),
//      K5_EPI_GATE -> bf16 out = bf16(resid + gate * bf16(acc * s)) (in place on the residual stream)
template <int EPI>
__global__ __launch_bounds__(512) void gemm_fp8_k8_kernel(Gemm8P p) {
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2;
  const int wn = wave & 1, wm = ((wave >> 1) & 1) | (grp << 1);   // 2 waves along n, 4 along m
  const int l15 = lane & 15, g = lane >> 4;

  const int nblk = p.lid_limit;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = (gridDim.x + 7 - xcd) >> 3;
  const int q8 = nblk >> 3, r8 = nblk & 7;
  const int x_first = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8, x_cnt = q8 + (xcd < r8 ? 1 : 0);
  constexpr int GM = 4;
  const int per_group = GM * p.tiles_n;
  auto tile_origin = [&](int lid, int& m0, int& n0) {
    const int gg = lid / per_group, first_m = gg * GM;
    const int gsz = min(p.tiles_m - first_m, GM);
    m0 = (first_m + (lid % per_group) % gsz) * F8_BM;
    n0 = ((lid % per_group) / gsz) * F8_BN;
  };

  // DMA: a half-tile (128 rows x 128 B) is 16 pieces of 8 rows; this wave stages pieces `wave` and `wave + 8`
  const int prow = 8 * wave + (lane >> 3);
  const int pc = (lane & 7) ^ ((prow >> 1) & 7);     // same for prow + 64 q + 128 h
  uint32_t ow[2][2], ox[2][2];   // [half][q] byte offsets from the operand bases
  auto set_offsets = [&](int m0, int n0) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int r = 128 * h + 64 * q + prow;
        ow[h][q] = (uint32_t)min(n0 + r, p.N - 1) * (uint32_t)p.ldw + 16u * pc;
        ox[h][q] = (uint32_t)min(m0 + r, p.M - 1) * (uint32_t)p.lda + 16u * pc;
      }
  };
  const char* Wbase = reinterpret_cast<const char*>(p.W);
  const char* Xbase = reinterpret_cast<const char*>(p.A);
  const int kmax = p.K - F8_BK;
  auto dma_w = [&](int stage, int h, int k0) {
    const char* b = Wbase + min(k0, kmax);   // tail: clamped -> redundant, harmless loads keep the vmcnt arithmetic uniform
#pragma unroll
    for (int q = 0; q < 2; ++q)
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(b + ow[h][q]), (lds_void_t*)(dsm + (2 * stage + h) * F8_UNIT + (8 * q + wave) * 1024), 16, 0, 0);
  };
  auto dma_x = [&](int stage, int h, int k0) {
    const char* b = Xbase + min(k0, kmax);
#pragma unroll
    for (int q = 0; q < 2; ++q)
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(b + ox[h][q]), (lds_void_t*)(dsm + F8_XOFF + (2 * stage + h) * F8_UNIT + (8 * q + wave) * 1024), 16, 0, 0);
  };
  auto prologue = [&]() { dma_w(0, 0, 0); dma_x(0, 0, 0); dma_x(0, 1, 0); dma_w(0, 1, 0); dma_w(1, 0, F8_BK); };

  // fragment reads: lane (l15, g) needs the 32 bytes at k = 32 g of its row = chunk pair {2g, 2g+1}, swizzled positions
  const int sw = (l15 >> 1) & 7;
  const int c0 = ((2 * g) ^ sw) << 4, c1 = ((2 * g + 1) ^ sw) << 4;
  const char* wb = dsm + (64 * wn + l15) * 128;              // + unit, + 16 i rows: immediates
  const char* xb = dsm + F8_XOFF + (32 * wm + l15) * 128;
  auto frag = [&](const char* base) {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(base + c0), hi = *reinterpret_cast<const u32x4*>(base + c1);
    return v8i{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  };
  const int nk = p.K / F8_BK;

  int m0, n0;
  if (slot < x_cnt) { tile_origin(x_first + slot, m0, n0); set_offsets(m0, n0); prologue(); }
  for (int ti = slot; ti < x_cnt; ti += per_xcd) {
    f32x4 acc[8][4];   // [n-tile][m-tile]
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    v8i wf[4], xf[2];

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();   // group 1 runs one barrier behind group 0 from here on

#define F8_LOAD_END()                                       \
  __builtin_amdgcn_sched_barrier(0);                        \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        \
  __builtin_amdgcn_s_barrier();                             \
  __builtin_amdgcn_sched_barrier(0);                        \
  __builtin_amdgcn_s_setprio(1)
#define F8_PHASE_END()                                      \
  __builtin_amdgcn_s_setprio(0);                            \
  __builtin_amdgcn_sched_barrier(0);                        \
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");          \
  __builtin_amdgcn_s_barrier();                             \
  __builtin_amdgcn_sched_barrier(0)
#define F8_MMA(ACC, A, B) ACC = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, B, ACC, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f)

    auto ktile = [&](auto STC, int t) {
      constexpr int st = decltype(STC)::value;
      constexpr int w0 = (2 * st) * F8_UNIT, w1 = (2 * st + 1) * F8_UNIT;   // same offsets for the X region
      const int k1 = (t + 1) * F8_BK, k2 = (t + 2) * F8_BK;
      // ---- phase 1: (n-tiles 0-3, m-tiles 0-1) ----
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 2; ++j) xf[j] = frag(xb + w0 + j * 16 * 128);
#pragma unroll
      for (int i = 0; i < 4; ++i) wf[i] = frag(wb + w0 + i * 16 * 128);
      dma_x(st ^ 1, 0, k1);
      F8_LOAD_END();
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) F8_MMA(acc[i][j], wf[i], xf[j]);
      F8_PHASE_END();
      // ---- phase 2: (n-tiles 0-3, m-tiles 2-3) ----
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 2; ++j) xf[j] = frag(xb + w1 + j * 16 * 128);
      dma_x(st ^ 1, 1, k1);
      F8_LOAD_END();
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) F8_MMA(acc[i][2 + j], wf[i], xf[j]);
      F8_PHASE_END();
      // ---- phase 3: (n-tiles 4-7, m-tiles 2-3) ----
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) wf[i] = frag(wb + w1 + i * 16 * 128);
      dma_w(st ^ 1, 1, k1);
      F8_LOAD_END();
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) F8_MMA(acc[4 + i][2 + j], wf[i], xf[j]);
      F8_PHASE_END();
      // ---- phase 4: (n-tiles 4-7, m-tiles 0-1): the X-half0 fragments are read again (keeping them would not fit 256 VGPRs) ----
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 2; ++j) xf[j] = frag(xb + w0 + j * 16 * 128);
      dma_w(st, 0, k2);
      F8_LOAD_END();
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) F8_MMA(acc[4 + i][j], wf[i], xf[j]);
      F8_PHASE_END();
    };
    int t = 0;
    for (; t + 1 < nk; t += 2) {
      ktile(std::integral_constant<int, 0>{}, t);
      ktile(std::integral_constant<int, 1>{}, t + 1);
    }
    if (nk & 1) ktile(std::integral_constant<int, 0>{}, t);
#undef F8_LOAD_END
#undef F8_PHASE_END
#undef F8_MMA
    if (grp == 0) __builtin_amdgcn_s_barrier();   // balance group 1's extra barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const int cm0 = m0, cn0 = n0;
    if (ti + per_xcd < x_cnt) { tile_origin(x_first + ti + per_xcd, m0, n0); set_offsets(m0, n0); prologue(); }

    int tid2 = threadIdx.x;
    asm volatile("" : "+v"(tid2));
    const int e_l15 = tid2 & 15, e_g = (tid2 >> 4) & 3, e_wave = tid2 >> 6;
    const int e_wn = e_wave & 1, e_wm = ((e_wave >> 1) & 1) | ((e_wave >> 2) << 1);
    // accumulator (i, j): token row m = [j < 2 ? 32 wm : 128 + 32 wm] + 16 (j & 1) + lane&15,
    //                     columns n = [i < 4 ? 64 wn : 128 + 64 wn] + 16 (i & 3) + 4 (lane>>4) + 0..3
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = cm0 + 128 * (j >> 1) + 32 * e_wm + 16 * (j & 1) + e_l15;
      if (m >= p.M) continue;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int n = cn0 + 128 * (i >> 2) + 64 * e_wn + 16 * (i & 3) + 4 * e_g;
        if (n >= p.N) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (p.scale_m) v[e] = fmaf(acc[i][j][e], p.w_scale[m], p.bias ? p.bias[m] : 0.f);
          else v[e] = n + e < p.N ? fmaf(acc[i][j][e], p.w_scale[n + e], p.bias ? p.bias[n + e] : 0.f) : 0.f;
        }
        if (EPI == K5_EPI_GELU) {
          uint8_t* cp = reinterpret_cast<uint8_t*>(p.C) + (size_t)m * p.ldc + n;
          const uint32_t pk = pack_fp8x4(gelu_erf(bf_round(v[0])), gelu_erf(bf_round(v[1])), gelu_erf(bf_round(v[2])), gelu_erf(bf_round(v[3])));
          if (n + 3 < p.N && (p.ldc & 3) == 0) *reinterpret_cast<uint32_t*>(cp) = pk;
          else for (int e = 0; e < 4; ++e) if (n + e < p.N) cp[e] = (uint8_t)(pk >> (8 * e));
        } else {
          bf16_t* cp = reinterpret_cast<bf16_t*>(p.C) + (size_t)m * p.ldc + n;
          if (EPI == K5_EPI_GATE) {
            const bf16_t* rp = p.resid + (size_t)m * p.ldr + n;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (n + e < p.N) v[e] = bf2f(rp[e]) + p.gate[n + e] * bf_round(v[e]);
          }
          if (n + 3 < p.N && (p.ldc & 3) == 0) {
            u32x2 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
            *reinterpret_cast<u32x2*>(cp) = o;
          } else {
            for (int e = 0; e < 4; ++e) if (n + e < p.N) cp[e] = f2bf(v[e]);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Round 4: the FOUR-wave structure of gemm_bf16_w4_kernel (gemm_bf16.hip) for e4m3 operands.  A row of a 128-element K-tile is 128 B — the
// bytes of the bf16 kernel's 64-element K-tile — so the LDS image (1040-B pieces, 2 stages x 2 operands x 33 280 B), the LDS-DMA stream
// (16 `buffer_load_dwordx4 ... lds` per wave and K-tile, SGPR row offsets, range-checked rows) and the persistent tile walk are THE SAME;
// what changes is the matrix work: one v_mfma_scale_f32_16x16x128_f8f6f4 consumes a whole K-tile of a 16 x 16 tile pair (32 B per lane and
// operand = two ds_read_b128 into one 8-register tuple), 64 of them per wave and K-tile at 32 cycles each = the bf16 kernel's matrix time for
// twice the K.  Fragment registers: W double-buffered (2 x 64), X single (64) = the bf16 kernel's 192.  Schedule of K-tile t (MFMA q = 0..63
// walks m-tile j = q >> 3 outer, n-tile i = q & 7 inner, so X[j] is dead after q = 8 j + 7):
//     q = 7            lgkmcnt(0) + barrier: every wave holds all of K-tile t's fragments -> stage t & 1 is free
//     q = 8, 11, .. 53 the 16 DMAs of K-tile t + 2 into that stage
//     q = 31           vmcnt(8) + barrier: K-tile t + 1 has landed (its 16 DMAs are older than this K-tile's first 8)
//     q = 32 .. 47     the 16 reads of W(t + 1) into the idle W buffer;  q = 48 .. 55: X(t + 1)[0..3] into the slots X[0..3] left at q <= 31
//     q = 56 .. 61     X(t + 1)[4], [5], [6] (slots free since q = 39 / 47 / 55);  after q = 63: X(t + 1)[7] — it lands under the next K-tile's
//                      first eight MFMAs (m-tile 0), which is why the top-of-K-tile barrier sits at q = 7 and not at q = 0
// Measured / parity: tests/test_gpu_kernels.py::test_gemm_fp8_* (the 256-tile shapes take this kernel), DESIGN.md §4.2.
// ---------------------------------------------------------------------------------------------
// Round 6 — fragment reads without bank conflicts.  A lane's 32 operand bytes are two ds_read_b128; the hardware serves a b128 read in the lane groups
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+ 32) (profiles/r05_lds_conflicts.md), and with the 1040-B piece stride of round 4 two lanes of every group
// met on the same four banks (SQ_LDS_BANK_CONFLICT = half of SQ_LDS_IDX_ACTIVE, HISTORY §R5: "left").  Searched exhaustively over (stride, swizzle):
// a 1088-B piece stride (68 slots of 16 B = 4 mod 16) and the two 16-B halves of a lane's chunk pair SWAPPED in the pieces 8..15 of every 16 — the DMA of the
// odd waves fetches chunk c ^ 1 into position c, and a lane with l15 >= 8 reads its low half from + 16 and its high half from + 0 (two base registers per
// operand): all sixteen lanes of every group on sixteen different slots, for both halves.
constexpr int F4_PAD = 1088, F4_OP = 32 * F4_PAD, F4_STAGE = 2 * F4_OP, F4_LDS = 2 * F4_STAGE;
static_assert(F4_LDS <= 160 * 1024, "LDS budget of the four-wave fp8 kernel");
typedef __attribute__((address_space(3))) void f4_lds_t;
typedef int v4i __attribute__((ext_vector_type(4)));

template <int EPI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_fp8_w4_kernel(Gemm8P p) {
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave & 1, wm = wave >> 1;
  const int l15 = lane & 15, lc = lane >> 4;

  const int nblk = p.lid_limit;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = (gridDim.x + 7 - xcd) >> 3;
  const int q8 = nblk >> 3, r8 = nblk & 7;
  const int x_first = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8, x_cnt = q8 + (xcd < r8 ? 1 : 0);
  constexpr int GM = 4;
  const int per_group = GM * p.tiles_n;
  auto tile_origin = [&](int lid, int& m0, int& n0) {
    const int g = lid / per_group, first_m = g * GM;
    const int gsz = min(p.tiles_m - first_m, GM);
    m0 = (first_m + (lid % per_group) % gsz) * F8_BM;
    n0 = ((lid % per_group) / gsz) * F8_BN;
  };
  if (slot >= x_cnt) return;

  const int nk = p.K / F8_BK;                  // even, >= 4 (launcher)
  const uint32_t ldw1 = (uint32_t)p.ldw, lda1 = (uint32_t)p.lda;   // bytes per row
  const uint32_t dch = (uint32_t)((lane & 7) ^ (wave & 1)) * 16u;   // this wave's pieces are 8 (wave & 1) + d of every 16: the odd waves swap the chunk pairs
  const uint32_t vw0 = (uint32_t)(16 * (lane >> 3)) * ldw1 + dch;
  const uint32_t vx0 = (uint32_t)(16 * (lane >> 3)) * lda1 + dch;
  const int drow = 128 * (wave >> 1) + 8 * (wave & 1);
  const int dslot = 8 * wave;
  uint32_t vw = vw0, vx = vx0;
  __amdgpu_buffer_rsrc_t rW, rX;
  int d_ti = slot, d_kt = 0;
  auto set_dma_tile = [&](int ti) {
    int m0, n0;
    tile_origin(x_first + ti, m0, n0);
    const int rows_w = min(p.N - n0, F8_BN), rows_x = min(p.M - m0, F8_BM);
    rW = __builtin_amdgcn_make_buffer_rsrc((void*)(p.W + (size_t)n0 * ldw1), 0, (int)((uint32_t)(rows_w - 1) * ldw1 + (uint32_t)p.K), 0x00020000);
    rX = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + (size_t)m0 * lda1), 0, (int)((uint32_t)(rows_x - 1) * lda1 + (uint32_t)p.K), 0x00020000);
    d_kt = 0; vw = vw0; vx = vx0;
  };
  auto dma1 = [&](int stage, int d) {
    if (d < 8) __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (f4_lds_t*)(dsm + stage * F4_STAGE + (dslot + d) * F4_PAD), 16, vw, (uint32_t)(drow + d) * ldw1, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rX, (f4_lds_t*)(dsm + stage * F4_STAGE + F4_OP + (dslot + d - 8) * F4_PAD), 16, vx, (uint32_t)(drow + d - 8) * lda1, 0, 0);
  };
  auto dma_advance = [&]() {   // after a K-tile's 16 DMAs; past the last tile the cursor wraps onto the same tile (harmless loads keep the vmcnt arithmetic uniform)
    vw += F8_BK; vx += F8_BK;
    if (++d_kt == nk) {
      if (d_ti + per_xcd < x_cnt) d_ti += per_xcd;
      set_dma_tile(d_ti);
    }
  };

  const uint32_t lds0 = (uint32_t)(uintptr_t)(f4_lds_t*)dsm;
  uint32_t wbs[2], xbs[2], wbh[2], xbh[2];   // low / high half of the lane's 32 bytes: + 128 i each
  const uint32_t hsw = (uint32_t)(l15 >> 3) * 16u;
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    const uint32_t wb = lds0 + st * F4_STAGE + (16 * wn + l15) * F4_PAD + lc * 32, xb = lds0 + st * F4_STAGE + F4_OP + (16 * wm + l15) * F4_PAD + lc * 32;
    wbs[st] = wb + hsw; wbh[st] = wb + 16u - hsw;
    xbs[st] = xb + hsw; xbh[st] = xb + 16u - hsw;
    asm volatile("" : "+v"(wbs[st]), "+v"(xbs[st]), "+v"(wbh[st]), "+v"(xbh[st]));
  }
  v4i wl[2][8], wh[2][8], xl[8], xh[8];
  f32x4 acc[8][8];   // [n-tile][m-tile]
  const int one = 0x7f7f7f7f;   // E8M0 block scales 2^0
#define F4_RD(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF))
#define F4_OPA(B, I) __builtin_shufflevector(wl[B][I], wh[B][I], 0, 1, 2, 3, 4, 5, 6, 7)
#define F4_OPB(J) __builtin_shufflevector(xl[J], xh[J], 0, 1, 2, 3, 4, 5, 6, 7)
#define F4_MF(B, Q) asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %3 op_sel_hi:[0,0,0]" : "+a"(acc[(Q) & 7][(Q) >> 3]) : "v"(F4_OPA(B, (Q) & 7)), "v"(F4_OPB((Q) >> 3)), "v"(one))
#define F4_MF0(B, Q) asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, 0, %3, %3 op_sel_hi:[0,0,0]" : "=a"(acc[(Q) & 7][(Q) >> 3]) : "v"(F4_OPA(B, (Q) & 7)), "v"(F4_OPB((Q) >> 3)), "v"(one))

  set_dma_tile(slot);
#pragma unroll
  for (int d = 0; d < 16; ++d) dma1(0, d);
  dma_advance();
#pragma unroll
  for (int d = 0; d < 16; ++d) dma1(1, d);
  dma_advance();
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int i = 0; i < 8; ++i) { F4_RD(wl[0][i], wbs[0], i * 128); F4_RD(wh[0][i], wbh[0], i * 128); }
#pragma unroll
  for (int j = 0; j < 8; ++j) { F4_RD(xl[j], xbs[0], j * 128); F4_RD(xh[j], xbh[0], j * 128); }

  auto ktile = [&](auto STC, auto FIRSTC) {
    constexpr int st = decltype(STC)::value;        // K-tile parity: its stage, and the W buffer its fragments sit in
    constexpr bool first = decltype(FIRSTC)::value;
    const uint32_t wb_n = wbs[st ^ 1], xb_n = xbs[st ^ 1], wh_n = wbh[st ^ 1], xh_n = xbh[st ^ 1];   // the stage K-tile t + 1 lands in
    // (one flat loop: a nested generic lambda per 16 MFMAs, as in the bf16 kernel, trips a clang capture bug on the asm operands here)
#pragma unroll
    for (int q = 0; q < 64; ++q) {
      if (first) F4_MF0(st, q); else F4_MF(st, q);
      if (q == 7) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (q >= 8 && (q - 8) % 3 == 0 && (q - 8) / 3 < 16) dma1(st, (q - 8) / 3);
      if (q == 31) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
      if (q >= 32 && q < 48) {
        const int r = q - 32;
        if (r & 1) F4_RD(wh[st ^ 1][r >> 1], wh_n, (r >> 1) * 128); else F4_RD(wl[st ^ 1][r >> 1], wb_n, (r >> 1) * 128);
      }
      if (q >= 48 && q < 62) {                     // X(t+1)[0..3] at q = 48..55, [4] [5] [6] at 56..61
        const int r = q - 48;
        if (r & 1) F4_RD(xh[r >> 1], xh_n, (r >> 1) * 128); else F4_RD(xl[r >> 1], xb_n, (r >> 1) * 128);
      }
    }
    F4_RD(xl[7], xb_n, 7 * 128); F4_RD(xh[7], xh_n, 7 * 128);
    dma_advance();
  };

  for (int ti = slot; ti < x_cnt; ti += per_xcd) {
    ktile(std::integral_constant<int, 0>{}, std::true_type{});
    ktile(std::integral_constant<int, 1>{}, std::false_type{});
    for (int t = 2; t < nk; t += 2) {
      ktile(std::integral_constant<int, 0>{}, std::false_type{});
      ktile(std::integral_constant<int, 1>{}, std::false_type{});
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15" ::: "memory");   // the next tile's X[7] fragments + let the last asm MFMAs retire
    int m0, n0;
    tile_origin(x_first + ti, m0, n0);
    int tid2 = threadIdx.x;
    asm volatile("" : "+v"(tid2));
    const int e_l15 = tid2 & 15, e_lc = (tid2 >> 4) & 3, e_wave = tid2 >> 6;
    const int e_wn = e_wave & 1, e_wm = e_wave >> 1;
    const int nb = n0 + 128 * e_wn + 4 * e_lc;          // + 16 i: this lane's four columns of n-tile i
    f32x4 svec[8], bvec[8];
    const bool has_bias = p.bias != nullptr, scale_m = p.scale_m != 0;   // workgroup-uniform
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      svec[i] = scale_m ? f32x4{1.f, 1.f, 1.f, 1.f} : *reinterpret_cast<const f32x4*>(p.w_scale + min(nb + 16 * i, p.N - 4));
      bvec[i] = (has_bias && !scale_m) ? *reinterpret_cast<const f32x4*>(p.bias + min(nb + 16 * i, p.N - 4)) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int m = m0 + 128 * e_wm + 16 * j + e_l15;
      const int mc = min(m, p.M - 1);
      const float sm = scale_m ? p.w_scale[mc] : 1.f, bm = (scale_m && has_bias) ? p.bias[mc] : 0.f;
      if constexpr (EPI == K5_EPI_GELU) {
        // e4m3(GELU(bf16(acc * s))): four values per n-tile = one dword; a 4 x 4 dword transpose over the lanes that share the row (16 apart)
        // gives every lane 16 consecutive bytes -> 2 stores of 16 B per token tile
#pragma unroll
        for (int ih = 0; ih < 2; ++ih) {
          uint32_t dw[4];
#pragma unroll
          for (int ii = 0; ii < 4; ++ii) {
            const int i = 4 * ih + ii;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = bf_round(fmaf(acc[i][j][e], svec[i][e], bvec[i][e]));
            gelu_erf_x2(v[0], v[1]); gelu_erf_x2(v[2], v[3]);
            dw[ii] = pack_fp8x4(v[0], v[1], v[2], v[3]);
          }
          // lane (row, lc) holds columns 16 ii + 4 lc .. + 3 in dw[ii]  ->  after the transpose dw[ii] = columns 16 lc + 4 ii .. + 3
          { const auto s0 = __builtin_amdgcn_permlane16_swap(dw[0], dw[1], false, false); dw[0] = s0[0]; dw[1] = s0[1];
            const auto s1 = __builtin_amdgcn_permlane16_swap(dw[2], dw[3], false, false); dw[2] = s1[0]; dw[3] = s1[1];
            const auto s2 = __builtin_amdgcn_permlane32_swap(dw[0], dw[2], false, false); dw[0] = s2[0]; dw[2] = s2[1];
            const auto s3 = __builtin_amdgcn_permlane32_swap(dw[1], dw[3], false, false); dw[1] = s3[0]; dw[3] = s3[1]; }
          const int n = n0 + 128 * e_wn + 64 * ih + 16 * e_lc;
          if (m < p.M && n < p.N) *reinterpret_cast<u32x4*>(reinterpret_cast<uint8_t*>(p.C) + (size_t)m * p.ldc + n) = u32x4{dw[0], dw[1], dw[2], dw[3]};
        }
      } else {
        u32x2 rr[8];
        if constexpr (EPI == K5_EPI_GATE) {
#pragma unroll
          for (int i = 0; i < 8; ++i) rr[i] = *reinterpret_cast<const u32x2*>(p.resid + (size_t)mc * p.ldr + min(nb + 16 * i, p.N - 4));
        }
#pragma unroll
        for (int iq = 0; iq < 4; ++iq) {
          u32x2 o[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int i = 2 * iq + h;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaf(acc[i][j][e], svec[i][e] * sm, bvec[i][e] + bm);   // one of each pair is the identity: a single rounding, as in the 8-wave kernel
            if constexpr (EPI == K5_EPI_GATE) {
              const f32x4 gv = *reinterpret_cast<const f32x4*>(p.gate + min(nb + 16 * i, p.N - 4));
              v[0] = __uint_as_float(rr[i][0] << 16) + gv[0] * bf_round(v[0]);
              v[1] = __uint_as_float(rr[i][0] & 0xffff0000u) + gv[1] * bf_round(v[1]);
              v[2] = __uint_as_float(rr[i][1] << 16) + gv[2] * bf_round(v[2]);
              v[3] = __uint_as_float(rr[i][1] & 0xffff0000u) + gv[3] * bf_round(v[3]);
            }
            o[h] = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
          }
#pragma unroll
          for (int dd = 0; dd < 2; ++dd) {
            const auto sw = __builtin_amdgcn_permlane16_swap(o[0][dd], o[1][dd], false, false);
            o[0][dd] = sw[0]; o[1][dd] = sw[1];
          }
          const int n = n0 + 128 * e_wn + 16 * (2 * iq + (e_lc & 1)) + 8 * (e_lc >> 1);
          if (m < p.M && n < p.N) *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(p.C) + (size_t)m * p.ldc + n) = u32x4{o[0][0], o[0][1], o[1][0], o[1][1]};
        }
        asm volatile("" ::: "memory");
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): nothing may still be loading into a VGPR when the asm stream resumes
  }
#undef F4_MF
#undef F4_MF0
#undef F4_OPA
#undef F4_OPB
#undef F4_RD
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int EPI>
int launch_f8_w4(Gemm8P p, hipStream_t stream, int num_cu) {
  static const hipError_t attr_rc = hipFuncSetAttribute((const void*)gemm_fp8_w4_kernel<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, F4_LDS);   // once, thread-safe
  if (attr_rc != hipSuccess) return K5_ERR_HIP;
  p.tiles_m = (p.M + F8_BM - 1) / F8_BM; p.tiles_n = (p.N + F8_BN - 1) / F8_BN;
  p.lid_limit = p.tiles_m * p.tiles_n;
  hipLaunchKernelGGL(gemm_fp8_w4_kernel<EPI>, dim3(min(p.lid_limit, num_cu)), dim3(256), F4_LDS, stream, p);
  return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP;
}

// one wave per row: scale[r] = max|x| / 448 (or 1 when `scale` is null: static scale), out = e4m3(x / scale)
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ out, float* __restrict__ scale,
                                                             int rows, int K, int ldx, int ldo) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t* xr = x + (size_t)row * ldx;
  float inv = 1.f;
  if (scale) {
    float mx = 0.f;
    for (int k = 4 * lane; k < K; k += 256)
#pragma unroll
      for (int e = 0; e < 4; ++e) mx = fmaxf(mx, fabsf(bf2f(xr[k + e])));
    mx = wave_max(mx);
    const float sc = mx > 0.f ? mx * (1.f / 448.f) : 1.f;
    if (lane == 0) scale[row] = sc;
    inv = 1.f / sc;
  }
  for (int k = 4 * lane; k < K; k += 256)
    *reinterpret_cast<uint32_t*>(out + (size_t)row * ldo + k) = pack_fp8x4(bf2f(xr[k]) * inv, bf2f(xr[k + 1]) * inv, bf2f(xr[k + 2]) * inv, bf2f(xr[k + 3]) * inv);
}

template <int EPI>
int launch_f8(Gemm8P p, hipStream_t stream) {
  static const hipError_t attr_rc = hipFuncSetAttribute((const void*)gemm_fp8_k8_kernel<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, F8_LDS);   // once, thread-safe
  if (attr_rc != hipSuccess) return K5_ERR_HIP;
  static const int num_cu = [] { int dev = 0; hipDeviceProp_t prop; if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1; return prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256; }();   // once, thread-safe
  if (num_cu <= 0) return K5_ERR_HIP;
  p.tiles_m = (p.M + F8_BM - 1) / F8_BM; p.tiles_n = (p.N + F8_BN - 1) / F8_BN;
  p.lid_limit = p.tiles_m * p.tiles_n;
  // the four-wave kernel from one full round of tiles up (K in whole pairs of K-tiles; 16-B stores need N % 16 == 0 and aligned rows)
  static const int force = getenv("K5_GEMM_FP8_V") ? atoi(getenv("K5_GEMM_FP8_V")) : 0;   // A/B: 8 = the 8-wave kernel, 4 = this one
  const bool w4_ok = (p.K % (2 * F8_BK)) == 0 && p.K >= 4 * F8_BK && p.M >= 512 && p.N >= 256 && !(p.N & 15) && !(p.ldc & 15) &&
                     (EPI != K5_EPI_GATE || !(p.ldr & 3)) &&
                     255ll * p.lda + p.K < (1ll << 31) && 255ll * p.ldw + p.K < (1ll << 31);   // its per-tile 32-bit lane + row offsets and the signed buffer range (bytes)
  // the 8-wave kernel keeps each lane's operand row as a 32-bit byte offset from the operand base (gemm_bf16.hip has the same guard): operands
  // whose last byte lies at or past 4 GiB go to the four-wave kernel, which rebases per tile, or are refused — there is no third kernel here
  const bool k8_fits = (long long)(p.M - 1) * p.lda + p.K < (1ll << 32) && (long long)(p.N - 1) * p.ldw + p.K < (1ll << 32);
  if (w4_ok && (force == 4 || !k8_fits || (force == 0 && p.lid_limit >= num_cu))) return launch_f8_w4<EPI>(p, stream, num_cu);
  if (!k8_fits) {
    k5_set_error("k5_gemm_fp8: an operand's last row starts at or beyond 4 GiB from its base (M %d lda %d, N %d ldw %d) and the shape is not one the four-wave kernel takes", p.M, p.lda, p.N, p.ldw);
    return K5_ERR_ARG;
  }
  hipLaunchKernelGGL(gemm_fp8_k8_kernel<EPI>, dim3(min(p.lid_limit, num_cu)), dim3(512), F8_LDS, stream, p);
  return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP;
}

}  // namespace

// A8 [M][K] fp8, W8 [N][K] fp8 (K a multiple of 128, rows 16-B aligned), w_scale [N] fp32.
// epi: K5_EPI_BIAS -> C bf16 [M][ldc];  K5_EPI_GELU -> C fp8 [M][ldc] = e4m3(GELU(bf16(.)));  K5_EPI_GATE -> bf16, gated residual.
int k5_launch_gemm_fp8(const void* A8, const void* W8, const float* w_scale, void* C, int M, int N, int K, int lda, int ldw, int ldc,
                       int epi, const void* resid, int ldr, const float* gate, hipStream_t stream, const float* bias, int scale_m) {
  if (M <= 0 || N <= 0 || K <= 0 || !w_scale) return K5_ERR_ARG;
  if (scale_m && epi != K5_EPI_BIAS) return K5_ERR_ARG;   // per-row scale / bias: the plain bf16-out epilogue only (V^T projection)
  if ((K % F8_BK) || (lda & 15) || (ldw & 15) || K < 2 * F8_BK) return K5_ERR_ALIGN;
  if (epi == K5_EPI_GATE && (!resid || !gate)) return K5_ERR_ARG;
  Gemm8P p;
  p.A = (const uint8_t*)A8; p.W = (const uint8_t*)W8; p.C = C; p.w_scale = w_scale; p.resid = (const bf16_t*)resid; p.gate = gate;
  p.bias = bias; p.scale_m = scale_m;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldw = ldw; p.ldc = ldc; p.ldr = ldr;
  switch (epi) {
    case K5_EPI_BIAS: return launch_f8<K5_EPI_BIAS>(p, stream);
    case K5_EPI_GELU: return launch_f8<K5_EPI_GELU>(p, stream);
    case K5_EPI_GATE: return launch_f8<K5_EPI_GATE>(p, stream);
    default: return K5_ERR_ARG;
  }
}

// x [rows][K] bf16 -> out [rows][K] e4m3; scale: per-row dynamic scale written there, or nullptr for the static scale 1
int k5_launch_quant_rows_fp8(const void* x, void* out, float* scale, int rows, int K, int ldx, int ldo, hipStream_t s) {
  if (rows <= 0 || K <= 0) return K5_ERR_ARG;
  if ((K & 3) || (ldx & 3) || (ldo & 3)) return K5_ERR_ALIGN;
  hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, (const bf16_t*)x, (uint8_t*)out, scale, rows, K, ldx, ldo);
  return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP;
}
