// attn_fwd.hip — flash-style attention forward for gfx950: O = softmax(Q K^T / sqrt(64)) V,
// bf16 operands, fp32 softmax/accumulate, head_dim 64, non-causal, ragged q_len / kv_len.
//
// Replaces the three FA(q,k,v) call sites of the reference (kandinsky/models/nn.py:201 text
// self-attention, :254 visual self-attention, :336 cross-attention; flash-attn itself is a
// third-party wheel, not part of the reference tree).
//
// Data flow per wave (32 query rows, 64-key tiles):
//   S^T = K · Q^T   (MFMA A = K rows, B = Q^T)  -> lane (q = l&31) holds 32 scores of ITS query:
//                   row max / row sum are in-lane + one permlane32 exchange with lane^32.
//   K rows are fed with bits 2,3 of the row index swapped so that the accumulator registers
//   [8s, 8s+8) of a lane are 8 CONSECUTIVE keys 16s + 8*(l>>5) + j: they are directly the
//   B-operand fragment of P^T for the second MFMA — no permlane / LDS round trip for P.
//   O^T = V^T · P^T (MFMA A = V^T rows (d), B = P^T) -> lane again owns one query: the online
//                   softmax rescale is lane-local.
// V is consumed TRANSPOSED ([H*64][keys]); the engine produces it for free by running the V
// projection GEMM with operands swapped (W_v · X^T), so no transposing LDS reads are needed.
//
// Schedule: one workgroup = 8 waves = 256 query rows of one head; K tile [64][64] and V^T tile
// [64][64] double-buffered in LDS (swizzled 16-B chunks, zero bank conflicts measured), register
// staged (tile t+1's global loads are issued before tile t's MFMAs, written to LDS after them), one
// barrier per tile.  Measured on MI355X (profiles/): a SIMD's time is close to
// ADDITIVE in MFMA issue cycles (16 x 32 per wave-tile) and VALU issue cycles (~2 per op) — VALU of
// one wave does not hide under its partner's MFMAs — so phase-shifted ("ping-pong") wave groups
// bought nothing, while keeping the kernel at <=128 VGPRs (fragments streamed, not hoisted) so that
// TWO workgroups (4 waves/SIMD) are resident per CU raised issue-port utilisation from 66 % to 85 %.
// What is left is the VALU op count per score; BOUNDED=true drops the online running max (24 ops
// per tile + the rescale branch) when the caller proves |score| <= bound (RMS-normalised q, k).
#include <stdlib.h>

#include <type_traits>
#include "k5_common.h"
#include "k5_kernels.h"

namespace {

constexpr int QB = 256;   // query rows per workgroup
constexpr int KB = 64;    // keys per tile
constexpr int TILE = 64 * 128;  // bytes of one [64][64] bf16 tile

constexpr float K5_ATTN_EXP_LIMIT = 90.f;   // |exp2 argument| bound of the fixed-offset form: p <= 2^90, l <= 2^107, O <= 2^114
// 2^-88: a row sum below this (per-row offsets only) sends the job to the online form.  bf16 / fp32 flush below 2^-126, so a flushed term is
// < 2^-38 of such a sum and ALL N <= 2^18 of them together < 2^-20 of it — far below bf16 resolution (round 3 had 2^-100: N 2^-126 against
// 2^-100 is 2^-10.5 at 47 616 keys, next to bf16's 2^-9 — ADVICE r3; round 2 had 2^-60, needlessly early).  The centred offsets guarantee
// a row sum >= 2^(90 - |q| R) >= 2^-100 only; rows between 2^-100 and 2^-88 now take the (exact) fallback instead of a 1e-3 error.
constexpr float K5_ATTN_ROW_MIN = 3.2311743e-27f;
// heads whose bound exceeds this go to the online form right away.  With the centred offsets (AttnP::kcentre) the bound is |q|max R and
// 190 is where the guarantee ends: a row's sum is >= 2^(90 - |q| R) >= 2^-100, so a fixed-form head NEVER falls back.  With the plain
// offsets (sequence-parallel path) the bound is |q|max kmax and the number is empirical (round 2: 180): rows keep their sum while their
// best score lies within 190 of the bound; the per-job fallback below catches the rest.  Measured on data whose scores carry a large
// common component (bench.py --qk-gain 5): gambling on bounds up to 300 computed most jobs twice (947 ms per step against 688 for the
// online form everywhere), the centred bound below 190 never does (gain 4: 553 ms, all heads fixed; plain offsets: 583-613).
constexpr float K5_ATTN_ROWOFF_LIMIT = 190.f;
// ANCHORED offsets (AttnP::row_anchor) for the heads beyond that limit: the offset of a row is an ACHIEVED score — the maximum s over a
// sample of keys (the row's own 64-token block + a strided sample, attn_row_anchor_kernel) — plus e + K5_ATTN_ANCHOR_ADD, where
// e = min(K5_ATTN_ANCHOR_EXTRA_MAX, spread (s - sample mean)) places the window where the maximum over ALL keys is expected: for scores
// that scatter like a Gaussian, s - mean ~ c sigma with c = sqrt(2 ln 512) and the maximum of N keys lies (sqrt(2 ln N) - c) sigma above
// s (1.1 sigma at N = 47 616; 0.2 sigma at N = 1024), so spread = K5_ATTN_ANCHOR_SPREAD (sqrt(2 ln N) - c) / c: 0.44 at 47 616 keys.
// DENSE attention: the row's true maximum m satisfies m >= s, so its term is >= 2^-80 and the row sum cannot underflow whatever the
// norms are (a PART of a split job or one PASS of a schedule may: harmless, its terms are < 2^-20 of the row's — exempt from the
// check); the form is exact while m < s + e + 132 (row sum < 2^112).  Beyond that the row sum grows past K5_ATTN_ROW_MAX (or turns
// inf / NaN) and the job falls back to the online form like an underflowing one: below 2^112 the sum bounds every accumulator
// (|O| <= l max|v|), so nothing overflowed unnoticed.  SPARSE (NABLA): a row attends its kept blocks only (its own block is always
// among them, most of the sample is not), so its largest KEPT score may lie below s: no guarantee, the underflow check stays as it is
// for every part, and the job flags are the net in both directions.
constexpr float K5_ATTN_ANCHOR_ADD = 20.f, K5_ATTN_ANCHOR_SPREAD = 1.4f, K5_ATTN_ANCHOR_EXTRA_MAX = 60.f;
// s - mean ~ c sigma with c = sqrt(2 ln 512); the maximum of kv_total keys lies (sqrt(2 ln kv_total) - c) sigma above the sample's
inline float anchor_spread(int kv_total) {
  const float c = sqrtf(2.f * logf(512.f));
  return K5_ATTN_ANCHOR_SPREAD * (sqrtf(2.f * logf((float)(kv_total > 512 ? kv_total : 512))) - c) / c;
}
constexpr float K5_ATTN_ROW_MAX = 5.1922969e33f;   // 2^112
constexpr int K5_ANCHOR_TILES = 32;
#ifndef K5_ATTN_WAVE_ROWS_DEFAULT
#define K5_ATTN_WAVE_ROWS_DEFAULT 32   // query rows per wave of the dense fixed-offset launch (32: 8 waves per workgroup; 64: 4 — K5_ATTN_WAVE_ROWS overrides)
#endif
#ifndef K5_ATTN_PAIR
#define K5_ATTN_PAIR 1   // A/B switch (tools/build_variant.sh -DK5_ATTN_PAIR=0): one key tile per barrier
#endif                // 16-key sample tiles per row: 4 of the row's own block + 28 strided over all keys

struct AttnP {
  const bf16_t* Q; const bf16_t* K; const bf16_t* Vt; bf16_t* O;
  int H, q_len, kv_len, ldq, ldk, ldvt, ldo, nqb;
  float c;        // softmax scale * log2(e)
  // per-head variant selection (engine: decided on the device from the data, attn_flags_kernel): a workgroup whose head's
  // flag differs from my_flag exits at once, so a fixed-offset launch and an online-max launch over the same grid
  // partition the heads between them.  null = every head.
  const int* sp_begin;   // SPARSE + RANGE, nullable: per workgroup the list position this launch starts from (sp_cnt = where it ends)
  const int* head_flags; int my_flag;
  // per-JOB fallback of the per-row-offset form (round 3): job = (head, query block of this launch) = the `lid` of the kernel.  A fixed-form
  // workgroup that sees a row underflow marks ITS job only — 1: the online launch of the same call redoes the job; 2 (multi-pass
  // schedules): "late", every later launch skips it and the last pass's online launch recomputes it from scratch — instead of sending
  // the whole head (186 jobs at 47 616 tokens) to the online form because of one row in 47 616.  null: head-level flags as in round 2.
  // Lives at the end of the balance workspace (k5_attention_balance_bytes), zeroed by the first pass of a schedule.
  const int* job_flags;
  // fixed-offset form with PER-ROW offsets (pre-scaled keys): kmax[h] = max |k'_h| (with margin) -> query row q of head h runs with
  // the constant offset max(0, |q| kmax[h] - K5_ATTN_EXP_LIMIT): exp2(s - offset) <= 2^90 whatever the data, and exact unless the
  // row's whole sum underflows (l < 2^-60: the row's true maximum lies > 150 below its Cauchy-Schwarz bound) — a workgroup that
  // sees that on a row with a non-zero offset sets its head's flag to 0 and the online-max launch that follows redoes the head.
  // null = offset 0 for every row (what the flags then have to guarantee: bound <= K5_ATTN_EXP_LIMIT).
  const float* kmax;
  // CENTRED form of the same bound (round 3; single-GPU path): kcentre[h][64] = a convex combination c_h of the head's keys (sample mean,
  // key_centre_kernel), krad[h] = max_j |k'_j - c_h| (with margin).  For every key  q.k' = q.c + q.(k' - c) <= q.c + |q| R, and the row's
  // largest score is >= q.c (the centred keys' projections on q average to ~0, so their maximum is >= 0).  A row whose plain bound
  // |q| kmax exceeds 90 therefore runs with the offset q.c + |q| R - 90 (any sign): exp2 arguments <= 90, and the row sum is >= 2^(90 - |q| R)
  // — no underflow at all while |q| R <= 190, whatever common component the scores carry (keys sharing a large mean direction put every
  // score of a head near +-0.4 of its plain bound: with the plain offset such rows underflow wholesale).  null: plain offsets.
  const float* kcentre; const float* krad;
  // ANCHORED per-row offsets (K5_ATTN_ANCHOR_ADD above): row_anchor[h * q_len + row], read for the heads whose kmax entry is NEGATIVE
  // (k5_launch_attn_flags marks a head beyond the Cauchy-Schwarz window that way instead of sending it to the online form)
  const float* row_anchor;
  // multi-pass schedules (sequence parallelism) with per-row offsets: 0 = single launch group (an underflowing row writes flag 0 and
  // the online launch of the same call redoes the head), 1 = a pass that is not the last (the row writes flag 2 = "late": every
  // later fixed-offset launch skips the head, the online launches of non-final passes skip it too), 2 = the last pass (the online
  // launch recomputes a late head FROM SCRATCH over all late_total key tiles, ignoring the state the earlier passes left)
  int late_pass, late_total;
  // cross-attention (keys not pre-scaled): RMSNorm of the query rows fused into the Q-fragment load — q = bf16(v * rsqrt(mean v^2 + eps) * w),
  // nn.py:35-40 without RoPE — instead of a pass over the (N, 1792) projection; 64 weights, null = Q is used as it is
  const float* q_norm_w;
  // visual self-attention (pre-scaled keys): with q_cos / q_sin ([row][32] fp32) the same load also applies the rotary embedding
  // (apply_rotary, nn.py:193-197) — the whole norm_qk + RoPE of the QUERIES happens here, once per workgroup, and the pass over the
  // (N, 1792) query projection is gone.  There is then no max|q_h|^2 statistic before the launch, so the head-level choice
  // "bound <= 190 -> fixed-offset form" is taken by the fixed-offset workgroups themselves: a workgroup with a row whose bound
  // |q| max|k'| exceeds 190 sets its head's flag to 0 (the online-max launch that follows owns the head) and exits before any work.
  const float* q_cos; const float* q_sin;
  unsigned long long* variant_counters;   // [fixed, online] heads (diagnostics): moved when a head flips
  // sequence-parallel layout of V^T: keys are split in chunks of vt_chunk_keys (multiple of 64) and chunk c
  // starts at Vt + c * vt_chunk_stride ([rank][H*64][ldvt] after an in-place all-gather); 0 = one chunk
  int vt_chunk_keys; long long vt_chunk_stride;
  // SPARSE (NABLA): per workgroup (head, 256-query group) a list of kv-block ids | (4-bit membership << 24) and its length
  const int* sp_list; const int* sp_cnt; int sp_stride;
  int pair_stride = 0;       // SPARSE, 128-query workgroups: rows of a group = k5_pair_row(group, 0 / 1, pair_stride, q_len / 64) (0: adjacent rows)
  // key-tile range of this launch (dense): sequence position e -> tile e + tile_off0, plus tile_skip_n once that reaches
  // tile_skip_at (lets pass 2 of the sequence-parallel schedule walk "every chunk except mine").  state/flags: resume
  // from (flags & 1) and/or leave (flags & 2) the fp32 running state {O^T accumulators, m, l} instead of normalising.
  int tile_off0, tile_cnt, tile_skip_at, tile_skip_n;
  // segmented walk (seg_len > 0; sliced K / V^T exchange of the sequence-parallel schedule): position e -> segment e / seg_len
  // (segments >= seg_skip shift up by one: "every rank's slice except mine"), tile = tile_off0 + segment * seg_stride + e % seg_len
  int seg_len, seg_stride, seg_skip;
  float* state; int flags;
  // job = (head, 256-query block) = job0 + workgroup index; RANGE launches may split every job's tile sequence `splits`
  // ways (workgroup g -> job job0 + g / splits, part g % splits): part 0 uses `state` (and is the only one that resumes),
  // part s >= 1 leaves its state at split_state + (s - 1) * split_stride floats.  Used to cut the last, partially filled
  // round of workgroups into short pieces (k5_launch_attention_bf16_balanced).
  int job0, splits; float* split_state; long long split_stride;
};

// MFMA 16x16x32 bf16 (1962 TFLOP/s sustained on random operands vs 1695 for 32x32x16, tools/probes/mfma_peak.hip):
//   A operand: lane l holds A[i = l&15][k = 8*(l>>4) + 0..7];  B operand: lane l holds B[k = 8*(l>>4) + 0..7][j = l&15]
//   C/D: lane l, reg r holds D[i = 4*(l>>4) + r][j = l&15]
K5_DEV f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// K tile swizzle.  The S^T MFMA reads, per 16-lane group, the permuted key rows {8a + b (+4, +32) : a, b in 0..3} at one
// 16-B chunk: XOR the chunk with row bits (4,3,1) so that those 16 rows (x row&1) hit 16 distinct 16-B bank slots.
K5_DEV int lds_swz_k(int row, int chunk) { return row * 128 + ((chunk ^ (((row >> 1) & 1) | (((row >> 3) & 3) << 1))) << 4); }

// v_max3_f32.  Compiler-visible on purpose: the operands are MFMA results, and only the compiler's hazard recogniser
// knows how many wait states an XDL write needs before a VALU read (an inline-asm v_max3 read stale accumulators).
K5_DEV float max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

// RANGE: key-tile sub-range + resumable fp32 state (sequence-parallel two-pass schedule); kept out of the plain dense
// instantiation, whose loop is sensitive to every extra live value (128-VGPR budget for 2 workgroups per CU).
// PRE: K arrives pre-multiplied by log2(e)/8 (rounded to bf16 once, by the rmsnorm/RoPE kernel): the scores ARE the exp2
// arguments -> no per-score fma at all.
// BOUNDED: the caller proved |score| * log2(e)/8 <= 90 for every pair, so exp2 of the raw argument can neither overflow nor
// flush a whole row: the softmax offset is the constant 0 (any offset gives the same softmax; a CENTRED one needs only
// |s| <= 90 where an upper-bound offset needs 2|s| <= 90).  !BOUNDED (PRE only): lazy online max — the offset of a query
// rides in the accumulator's initial value, the tile maximum of (score - offset) is folded with v_max3 (16 ops per tile)
// and only when some lane sees it exceed ONLINE_THR does the wave take the rescale branch.
constexpr float ONLINE_THR = 60.f;
#ifndef K5_ONLINE_WPS
#define K5_ONLINE_WPS 2   // waves per SIMD the online-max instantiations are compiled for: 2 = up to 256 VGPRs, one workgroup per CU (at 4 = 128 VGPRs the allocator spills the cold path into the tile loop: 4x slower, measured)
#endif
// Layout of the resumable fp32 state (k5_attention_state_bytes): the accumulators of one (head, 256-query) job are 64 KB in the order
// the 16x16x32 kernel's lanes hold them — [16-row group][d tile of 16][lane group g = (d >> 2) & 3][row & 15][4 floats] — so that one
// store instruction of a wave is 1 KB contiguous (round 2 had [q][H * 64]: 64-B pieces at 7-KB strides, 0.56 TB/s measured; the state
// round trip of the sequence-parallel passes was 6 % of a shard's step).  (m, l) pairs follow: [16-row group][slot 0..3][row & 15][2].
// Every reader / writer — both kernel forms and the merge — goes through these two functions.
// (float indices; < 2^31 up to 1.6 M query rows x 28 heads)
__device__ __forceinline__ uint32_t st_o_off(int q, int h, int d, int nqb) {   // d % 4 == 0
  const uint32_t qb = (uint32_t)q >> 8, r = (uint32_t)q & 255u;
  return ((((uint32_t)(h * nqb) + qb) * 16u + (r >> 4)) * 4u + ((uint32_t)d >> 4)) * 256u + (((uint32_t)d >> 2) & 3u) * 64u + (r & 15u) * 4u;
}
__device__ __forceinline__ uint32_t st_ml_off(int q, int h, int slot, int nqb, int H) {
  const uint32_t qb = (uint32_t)q >> 8, r = (uint32_t)q & 255u;
  return (uint32_t)(H * nqb) * (256u * 64u) + ((((uint32_t)(h * nqb) + qb) * 16u + (r >> 4)) * 4u + (uint32_t)slot) * 32u + (r & 15u) * 2u;
}

// QN: the norm_qk + RoPE of the queries is fused into the Q load (K5QueryNorm, pre-scaled keys).  A template parameter and not a runtime
// branch: with the code merely PRESENT the compiler schedules the tile loop of the plain form differently (same instructions, +1 % time).
// HALF (NABLA on one GPU): the workgroup is launched with 256 threads = 4 waves = 128 query rows, i.e. TWO 64-query rows of the block
// map share a key-tile list instead of four — a wave only computes the tiles its own row selected, so the launch's efficiency is
// (sum of the rows' lists) / (rows x their union), and two rows' union is tighter than four rows'.  Every wave then brings in two
// 1-KB pieces of K and of V^T per tile (twice the L2 -> LDS traffic per FLOP; four workgroups per CU instead of two).
// GR (round 4, generalising round 2's HALF): 64-query rows of the block map per workgroup = per key-tile list.  4: 8 waves, 256 queries.
// 2: 4 waves (HALF above).  1: TWO waves, one row per list — the list IS the row's selection, nothing is stepped over for a neighbour's sake
// (measured union efficiency of the 2-row lists on the 10 s clip: 0.80 at kept density 0.048, 0.73 at 0.122, while the kernel executes its
// tiles at the dense kernel's rate — the union was the whole loss); each wave then brings in four 1-KB pieces of K and of V^T per tile.
// QT (round 4): 16-query MFMA tiles per wave.  2: 32 query rows per wave, 8 waves per 256-query workgroup, 4 waves per SIMD (every round so far).
// 4: 64 rows per wave, FOUR waves per 256-query workgroup, 2 waves per SIMD — every K / V^T fragment read from LDS feeds four MFMAs instead of
// two (half the ds_read_b128 per MFMA, the ledger's remaining non-essential class: profiles/r04_attention_issue_ledger.md), each wave stages
// two 1-KB pieces of a tile per operand.  Same arithmetic per query row in the same order: bit-identical outputs.
// PIPE (round 5; VERDICT r4 #4 — the one experiment the issue ledger pointed to): 64-row waves, ONE wave per SIMD (one 256-query workgroup per CU, up
// to 512 registers), software-pipelined over HALF key tiles: in every unit of 32 keys the wave issues three independent streams — the S^T MFMAs of the
// half tile one tile ahead (16), the exponentials + packs of the half tile before that (32 + 16 VALU), and the P V MFMAs + row sums of the half tile
// whose probabilities are ready (20) — so the exponentials of one tile run under the matrix work of its neighbours inside ONE wave instead of
// relying on four waves per SIMD to fall out of step.  K / V^T tiles in a ring of three PAIRS (6 slots per operand, 96 KB of dynamic LDS): pair p + 2
// is fetched while pair p is attended and the S^T of pair p + 1 is formed.  Same arithmetic per query row in the same order: bit-identical outputs.
template <bool BOUNDED, bool SPARSE, bool RANGE, bool PRE = false, bool QN = false, int GR = 4, int QT = 2, bool PIPE = false>
__global__ __launch_bounds__(QT == 4 ? 256 : 512, PIPE ? (QT == 4 ? 1 : 2) : (QT == 4 ? 2 : (BOUNDED ? 4 : K5_ONLINE_WPS))) void attn_fwd_kernel(AttnP p) {
  static_assert(QT == 2 || (QT == 4 && GR == 4), "64-row waves: the 256-query workgroups only");
  static_assert(!PIPE || (BOUNDED && PRE && !SPARSE && !QN && GR == 4), "the pipelined form: dense, fixed-offset softmax, pre-scaled keys, 256-query workgroups");
  constexpr int NW = 4 * GR / QT;     // waves per workgroup: 8 (256 queries, 32-row waves), 4 (128 queries, or 256 with 64-row waves), 2 (64 queries)
  constexpr int RW = 16 * QT;         // query rows per wave
  constexpr bool HALF = GR != 4;     // fewer than 8 waves: one tile per barrier, every wave stages several pieces
  static_assert(GR == 4 || GR == 2 || GR == 1, "rows per list: 4, 2 or 1");
  static_assert(BOUNDED || PRE, "the online-max form of this kernel takes pre-scaled keys (attn_fwd32_kernel serves the rest)");
  static_assert(!HALF || (SPARSE && PRE && !RANGE && !QN), "128- / 64-query workgroups: the list-driven single-launch form only");
  // K5_ATTN_PAIR: two key tiles per barrier (four LDS slots per operand instead of two) for the 256-query workgroups — same arithmetic in
  // the same order, half the barriers; the 128-query form keeps one tile per barrier (four workgroups per CU: 32 KB each)
  constexpr bool PAIR = K5_ATTN_PAIR && !HALF;
  constexpr int NBUF = PIPE ? 6 : (PAIR ? 4 : 2);
  extern __shared__ __attribute__((aligned(16))) char attn_dsm[];                         // PIPE: 96 KB, beyond the static limit
  __shared__ __attribute__((aligned(16))) char smem_static[PIPE ? 16 : 2 * NBUF * TILE];
  char* smem = PIPE ? attn_dsm : smem_static;
  char* sK = smem;
  char* sV = smem + NBUF * TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const int gid = xcd_remap(blockIdx.x, gridDim.x);
  const int part = RANGE ? gid % p.splits : 0;
  const int lid = p.job0 + (RANGE ? gid / p.splits : gid);
  const int h = lid / p.nqb, qb = lid % p.nqb;
  bool late = false;   // online form, last pass, head flagged late: walk ALL key tiles from a fresh state
  if (p.head_flags) {   // workgroup-uniform: the other variant's launch owns this head
    int hf = p.head_flags[h];
    if (p.job_flags && hf == 1) { const int jf = p.job_flags[lid]; if (jf) hf = jf == 2 ? 2 : 0; }   // this job alone left the fixed form
    if (BOUNDED) { if (hf != 1) return; }
    else {
      if (hf == 1) return;
      if (hf == 2) { if (p.late_pass != 2) return; late = true; }
    }
  }
  // this wave: queries q0 .. q0+31 = two 16-query MFMA tiles (qt = 0, 1); the two rows of a 128-query group need not be adjacent (frame pairing)
  const int q0 = (GR == 2 && p.pair_stride > 0) ? k5_pair_row(qb, wave >> 1, p.pair_stride, p.q_len >> 6) * 64 + (wave & 1) * 32
                                                : qb * (64 * GR) + wave * RW;

  // Q^T fragments (MFMA 16x16x32 B operand): lane (l15, g) holds Q[q0 + 16 qt + l15][32 ks + 8 g .. +8]
  bf16x8 qf[QT][2];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const bf16_t* qp = p.Q + (size_t)min(q0 + 16 * qt + l15, p.q_len - 1) * p.ldq + h * 64 + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[qt][ks] = *reinterpret_cast<const bf16x8*>(qp + 32 * ks);
  }
  if (PRE && QN) {   // fused norm_qk + apply_rotary of the queries, same arithmetic and rounding points as rmsnorm_rope_kernel
    // every load first (weights, both query tiles' table rows: none depends on q), so that the prologue is ONE memory round trip
    f32x4 wa[2], wb[2], cs[QT][2], sn[QT][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      wa[ks] = *reinterpret_cast<const f32x4*>(p.q_norm_w + 32 * ks + 8 * g);
      wb[ks] = *reinterpret_cast<const f32x4*>(p.q_norm_w + 32 * ks + 8 * g + 4);
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const int row = min(q0 + 16 * qt + l15, p.q_len - 1);
        cs[qt][ks] = *reinterpret_cast<const f32x4*>(p.q_cos + (size_t)row * 32 + 16 * ks + 4 * g);
        sn[qt][ks] = *reinterpret_cast<const f32x4*>(p.q_sin + (size_t)row * 32 + 16 * ks + 4 * g);
      }
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      // The sum of squares in rmsnorm_rope_kernel's ORDER (round 6): there a thread sums its 8-dimension chunk pair by pair, then the eight chunks of a head
      // combine as a tree (xor 1, 2, 4).  This lane holds chunks g (ks = 0) and 4 + g (ks = 1): each summed on its own with the same expression, chunks
      // g <-> g ^ 1 and g ^ 2 combined across the lanes 16 and 32 apart per ks, the two halves added last — the same fp32 value, so the normalised
      // queries, and with them the whole attention, are BIT-IDENTICAL to the standalone pass (before: one running sum over both chunks; the last bit of
      // 1 / rms differed now and then, and a bf16 rounding of q with it).
      float v[16], sq2[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const u32x4 w4 = __builtin_bit_cast(u32x4, qf[qt][ks]);
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[8 * ks + 2 * j] = __uint_as_float(w4[j] << 16);
          v[8 * ks + 2 * j + 1] = __uint_as_float(w4[j] & 0xffff0000u);
          sq = __fadd_rn(sq, fmaf(v[8 * ks + 2 * j + 1], v[8 * ks + 2 * j + 1], __fmul_rn(v[8 * ks + 2 * j], v[8 * ks + 2 * j])));   // operation for operation as rmsnorm_rope_kernel
        }
        const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(sq), __float_as_uint(sq), false, false);
        sq = __fadd_rn(__uint_as_float(s16[0]), __uint_as_float(s16[1]));
        const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(sq), __float_as_uint(sq), false, false);
        sq2[ks] = __fadd_rn(__uint_as_float(s32[0]), __uint_as_float(s32[1]));
      }
      const float ss = __fadd_rn(sq2[0], sq2[1]);
      const float rs = rsqrtf(fmaf(ss, 1.0f / 64.0f, 1.1920928955078125e-07f));
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        float y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = bf_round(__fmul_rn(__fmul_rn(v[8 * ks + j], rs), j < 4 ? wa[ks][j] : wb[ks][j - 4]));   // .type_as(q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float x0 = y[2 * j], x1 = y[2 * j + 1];   // the rotation operation for operation as rmsnorm_rope_kernel spells it (which product is fused matters)
          y[2 * j] = fmaf(cs[qt][ks][j], x0, -__fmul_rn(sn[qt][ks][j], x1));
          y[2 * j + 1] = fmaf(sn[qt][ks][j], x0, __fmul_rn(cs[qt][ks][j], x1));
        }
        const u32x4 pk = {pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]), pack_bf16x2(y[4], y[5]), pack_bf16x2(y[6], y[7])};
        qf[qt][ks] = __builtin_bit_cast(bf16x8, pk);
      }
    }
  }
  if (!PRE && p.q_norm_w) {   // fused RMSNorm(q): the query's 64 dimensions sit in its four lanes (l15 + 16 g), 16 each
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      float v[16], ss = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const u32x4 w4 = __builtin_bit_cast(u32x4, qf[qt][ks]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[8 * ks + 2 * j] = __uint_as_float(w4[j] << 16);
          v[8 * ks + 2 * j + 1] = __uint_as_float(w4[j] & 0xffff0000u);
          ss += v[8 * ks + 2 * j] * v[8 * ks + 2 * j] + v[8 * ks + 2 * j + 1] * v[8 * ks + 2 * j + 1];
        }
      }
      {
        const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(ss), __float_as_uint(ss), false, false);
        ss = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
        const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(ss), __float_as_uint(ss), false, false);
        ss = __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
      }
      const float rs = rsqrtf(ss * (1.0f / 64.0f) + 1.1920928955078125e-07f);   // eps = finfo(fp32).eps, as rmsnorm_rope_kernel
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const f32x4 wa = *reinterpret_cast<const f32x4*>(p.q_norm_w + 32 * ks + 8 * g), wb = *reinterpret_cast<const f32x4*>(p.q_norm_w + 32 * ks + 8 * g + 4);
        float y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = __fmul_rn(__fmul_rn(v[8 * ks + j], rs), j < 4 ? wa[j] : wb[j - 4]);
        const u32x4 pk = {pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]), pack_bf16x2(y[4], y[5]), pack_bf16x2(y[6], y[7])};
        qf[qt][ks] = __builtin_bit_cast(bf16x8, pk);
      }
    }
  }
  // loader mapping: 512 threads, one 16-B chunk of K and one of V^T each per tile
  const int lrow = tid >> 3, lc = tid & 7;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  // global addresses as uniform 64-bit base (SGPRs) + per-lane 32-bit byte offset: two VGPRs instead of two pointers
  const char* Kb = reinterpret_cast<const char*>(p.K);
  const char* Vb = reinterpret_cast<const char*>(p.Vt);
  // Tiles go global -> LDS by DMA (global_load_lds, 16 B per lane, wave w fills rows 8w..8w+7 = 1 KB): the LDS slot
  // (lrow, lc) receives SOURCE chunk lc ^ swizzle(lrow), so position p of a row holds logical chunk p ^ swizzle(row)
  const uint32_t kstride = (uint32_t)p.ldk * 2u;
  const uint32_t klane = (uint32_t)(h * 64 + 8 * (lc ^ (((lrow >> 1) & 1) | (((lrow >> 3) & 3) << 1)))) * 2u;
  const uint32_t vlane = ((uint32_t)(h * 64 + lrow) * (uint32_t)p.ldvt + 8u * (lc ^ ((lrow >> 1) & 7))) * 2u;
  const uint32_t vlane_lin = ((uint32_t)(h * 64 + lrow) * (uint32_t)p.ldvt + 8u * lc) * 2u;   // ragged tile: register path
  const int* sp_list = SPARSE ? p.sp_list + (size_t)(h * p.nqb + qb) * p.sp_stride : nullptr;
  const int Tall = SPARSE ? p.sp_cnt[h * p.nqb + qb] : ((!BOUNDED && late) ? p.late_total : p.tile_cnt);
  // this workgroup's share of the tile sequence: positions [E0, T)  (everything unless the job is split)
  // SPARSE + RANGE: the launch covers the list positions [B0, Tall) (B0 > 0: the second pass of a two-pass list walk)
  const int B0 = (SPARSE && RANGE && p.sp_begin && !(!BOUNDED && late)) ? min(p.sp_begin[h * p.nqb + qb], Tall) : 0;
  const int E0 = RANGE ? B0 + (int)(((long long)(Tall - B0) * part) / p.splits) : 0;
  const int T = RANGE ? B0 + (int)(((long long)(Tall - B0) * (part + 1)) / p.splits) : Tall;
  const int nfull = p.kv_len / KB;                    // key tiles with all 64 keys valid (NABLA: all of them)
  auto tile_of = [&](int e) -> int {                  // sequence position -> 64-key tile index (wave-uniform)
    if (SPARSE) return sp_list[e] & 0xffffff;   // scalar loads (s_load): keep every int* store / atomic of this kernel BEHIND the tile loop,
    if (!RANGE) return e;                       // or they become vector loads whose vmcnt wait drains the tile DMA as well
    if (!BOUNDED && late) return e;
    if (p.seg_len > 0) {
      int si = e / p.seg_len;
      const int j = e - si * p.seg_len;
      if (si >= p.seg_skip) ++si;
      return p.tile_off0 + si * p.seg_stride + j;
    }
    int t = e + p.tile_off0;
    if (t >= p.tile_skip_at) t += p.tile_skip_n;
    return t;
  };
  const int my_bit = 1 << (24 + ((wave * RW) >> 6));  // this wave's 64-query block inside the 256-query workgroup
  const int tiles_per_chunk = p.vt_chunk_keys > 0 ? p.vt_chunk_keys / KB : 0x7fffffff;
  typedef __attribute__((address_space(3))) void lds_void_t;
  typedef const __attribute__((address_space(1))) void gbl_void_t;
  const uint32_t kvoff = (uint32_t)lrow * kstride + klane;
  // GR == 1: lane offset of the pieces whose rows are lrow + 16 (mod 32): the swizzle term of row bit 4 flips
  const uint32_t kvoff16 = (uint32_t)lrow * kstride + (uint32_t)(h * 64 + 8 * (lc ^ ((((lrow + 16) >> 1) & 1) | ((((lrow + 16) >> 3) & 3) << 1)))) * 2u;
  const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc((void*)p.K, 0, -1, 0x00020000);   // 4 GB window from the base
  const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc((void*)p.Vt, 0, -1, 0x00020000);
  auto load_tile = [&](int e, int buf) {   // e = position in the tile sequence; tile t = tile_of(e) -> LDS buffer `buf`
    const int t = tile_of(e);
    const int kv0 = t * KB;
    const char* vsrc = Vb + 2 * (long long)kv0;     // uniform
    if (p.vt_chunk_keys > 0) {   // sequence-parallel V^T layout only (uniform branch): per-rank chunks
      const int chunk = t / tiles_per_chunk;
      vsrc = Vb + 2 * ((long long)chunk * p.vt_chunk_stride + (kv0 - chunk * tiles_per_chunk * KB));
    }
    if (PRE) {   // whole tiles only (launcher): constant per-lane offsets, the tile rides in the instruction's SGPR offset: no address VALU
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rK, (lds_void_t*)(sK + buf * TILE + wave_u * 1024), 16, kvoff, (uint32_t)kv0 * kstride, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rV, (lds_void_t*)(sV + buf * TILE + wave_u * 1024), 16, vlane, (uint32_t)(vsrc - Vb), 0, 0);
      if (NW == 4) {   // four waves: rows 32..63 of both tiles as well (the swizzles only involve row bits 1..4: same lane offsets + 32 rows)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rK, (lds_void_t*)(sK + buf * TILE + (wave_u + 4) * 1024), 16, kvoff + 32u * kstride,
                                                 (uint32_t)kv0 * kstride, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rV, (lds_void_t*)(sV + buf * TILE + (wave_u + 4) * 1024), 16, vlane + 64u * (uint32_t)p.ldvt,
                                                 (uint32_t)(vsrc - Vb), 0, 0);
      }
      if (NW == 2) {   // two waves (rows 0..15 between them): rows + 16, + 32, + 48 as well.  The K swizzle involves row bit 4, so the pieces at
                       // + 16 / + 48 rows take their own lane offset (kvoff16); V^T's only involves bits 1..3
#pragma unroll
        for (int j = 1; j < 4; ++j) {
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rK, (lds_void_t*)(sK + buf * TILE + (wave_u + 2 * j) * 1024), 16, ((j & 1) ? kvoff16 : kvoff) + (uint32_t)(16 * j) * kstride,
                                                   (uint32_t)kv0 * kstride, 0, 0);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rV, (lds_void_t*)(sV + buf * TILE + (wave_u + 2 * j) * 1024), 16, vlane + (uint32_t)(32 * j) * (uint32_t)p.ldvt,
                                                   (uint32_t)(vsrc - Vb), 0, 0);
        }
      }
      return;
    }
    __builtin_amdgcn_global_load_lds((gbl_void_t*)(Kb + ((uint32_t)min(kv0 + lrow, p.kv_len - 1) * kstride + klane)),
                                     (lds_void_t*)(sK + buf * TILE + wave_u * 1024), 16, 0, 0);
    if (SPARSE || PRE || t < nfull) {   // PRE launches require kv_len % 64 == 0 (checked by the launcher): no ragged tile
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(vsrc + vlane), (lds_void_t*)(sV + buf * TILE + wave_u * 1024), 16, 0, 0);
    } else {  // ragged last tile: never read past the padded row; zero the keys >= kv_len (P is exactly 0 there anyway)
      const int rem = p.kv_len - (kv0 + 8 * lc);    // valid keys in this lane's 8-key chunk (<= 0: none)
      u32x4 rv = {0u, 0u, 0u, 0u};
      if (rem > 0) rv = *reinterpret_cast<const u32x4*>(vsrc + vlane_lin);   // the chunk lies inside the 8-padded row
#pragma unroll
      for (int j = 0; j < 4; ++j) rv[j] = rem >= 2 * j + 2 ? rv[j] : (rem == 2 * j + 1 ? (rv[j] & 0xffffu) : 0u);
      *reinterpret_cast<u32x4*>(sV + buf * TILE + lds_swz(lrow, lc)) = rv;
    }
  };
  // K row permutation.  S^T tile kt (16 keys) row i of lane group g' = i>>2 must be the key that the P^T operand of the
  // second MFMA wants in this lane: P^T (B operand, k = 32 keys) lane (query, g) holds keys 8g..8g+7 of the 32-key group,
  // the accumulator lane (query, g) holds rows 4g..4g+3 of tiles 2ks2 and 2ks2+1 -> tile kt row i <-> key
  // 32 (kt>>1) + 8 (i>>2) + 4 (kt&1) + (i&3): the two tiles' registers of a lane ARE its 8 consecutive keys.
  const int krow = 8 * (l15 >> 2) + (l15 & 3);        // + 32 (kt>>1) + 4 (kt&1): immediates

  f32x4 ot[4][QT];   // O^T accumulators: [d tile of 16][query tile]: lane (l15, g) holds d = 16 dt + 4 g + r, query 16 qt + l15
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) ot[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float c = p.c;
  // !BOUNDED: nm[qt] = MINUS the softmax offset of the lane's query (exp2 domain), four copies = the S^T accumulators' start
  f32x4 nm[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) nm[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  bool fresh = true;             // !BOUNDED, wave-uniform: no tile processed yet -> the first one SETS the offset
  bool over_limit = false;
  bool anchored = false;   // workgroup-uniform: the head runs on anchored offsets (dense: a part's sum may underflow harmlessly; the row's cannot)
  if (BOUNDED && PRE && p.kmax) {   // per-row constant offsets from |q_row| * max|k'| (see AttnP::kmax); 0 when the bound is <= 90
    // a NEGATIVE entry marks a head beyond the Cauchy-Schwarz window (k5_launch_attn_flags, anchored offsets) and still carries the
    // magnitude: a caller of the public ABI that marks heads (k5_attention_flags_rows_anchored) and then attends WITHOUT row anchors gets
    // the plain per-row offsets of |entry| — exp2 arguments <= 90 whatever the data, and the underflow check + per-job fallback as the net
    const float km_raw = p.kmax[h];
    const float km = fabsf(km_raw);
    anchored = km_raw < 0.f && p.row_anchor;
    if (anchored) {   // workgroup-uniform
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const float off = p.row_anchor[(size_t)h * p.q_len + min(q0 + 16 * qt + l15, p.q_len - 1)];
        nm[qt] = f32x4{-off, -off, -off, -off};
      }
    } else {
    const bool centred = p.kcentre != nullptr;   // kernel-uniform
    const float kr = centred ? p.krad[h] : 0.f;
    f32x4 cc[2][2];   // the centre's entries at this lane's 16 query dimensions (32 ks + 8 g .. + 8)
    if (centred) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        cc[ks][0] = *reinterpret_cast<const f32x4*>(p.kcentre + h * 64 + 32 * ks + 8 * g);
        cc[ks][1] = *reinterpret_cast<const f32x4*>(p.kcentre + h * 64 + 32 * ks + 8 * g + 4);
      }
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      float ss = 0.f, tc = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const u32x4 w = __builtin_bit_cast(u32x4, qf[qt][ks]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float lo = __uint_as_float(w[j] << 16), hi = __uint_as_float(w[j] & 0xffff0000u);
          ss = fmaf(lo, lo, fmaf(hi, hi, ss));
          if (centred) tc = fmaf(lo, cc[ks][j >> 1][2 * (j & 1)], fmaf(hi, cc[ks][j >> 1][2 * (j & 1) + 1], tc));
        }
      }
      {   // the query's four lanes (l15 + 16 g) hold 16 of its 64 dimensions each
        const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(ss), __float_as_uint(ss), false, false);
        ss = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
        const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(ss), __float_as_uint(ss), false, false);
        ss = __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
      }
      if (centred) {
        const auto t16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(tc), __float_as_uint(tc), false, false);
        tc = __uint_as_float(t16[0]) + __uint_as_float(t16[1]);
        const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(tc), __float_as_uint(tc), false, false);
        tc = __uint_as_float(t32[0]) + __uint_as_float(t32[1]);
      }
      const float nq = sqrtf(ss);
      float bnd = nq * km;                                        // plain Cauchy-Schwarz bound: <= 90 -> offset 0, as without any of this
      float off = fmaxf(bnd - K5_ATTN_EXP_LIMIT, 0.f);
      if (centred && bnd > K5_ATTN_EXP_LIMIT) {
        // both are upper bounds of the row's scores: take the TIGHTER one (R may reach 2 kmax when the keys do not share a direction);
        // the row sum's survival depends on the distance between the offset and the row's largest score, which the smaller offset shortens
        const float bc = nq * kr;
        const float offc = tc + bc * 1.002f + 0.5f - K5_ATTN_EXP_LIMIT;   // margins: fp32 rounding of q.c and of the MFMA accumulation
        if (offc < off) { off = offc; bnd = bc; } else bnd = fminf(bnd, bc);
      }
      // an INTEGER offset: exp2(s - off) then differs between any two offset policies by an exact power of two, so the bf16 rounding of
      // every probability — and with it the whole result — is the same whichever policy chose the offset (0, plain, centred; one GPU or
      // the sequence-parallel schedule), as long as nothing under- or overflows
      off = ceilf(off);
      nm[qt] = f32x4{-off, -off, -off, -off};
      if (QN) over_limit |= (q0 + 16 * qt + l15 < p.q_len) && !(bnd <= K5_ATTN_ROWOFF_LIMIT);   // NaN counts as over
    }
    }
  }
  // Fused query norm: no max|q|^2 statistic preceded this launch, so the head-level choice is taken here — a wave that holds a row
  // above the limit flips its head's flag to the online form AFTER its tile loop (below), and whatever the fixed-offset launch wrote for
  // the head is overwritten by the online launch that follows.  Why not an early, workgroup-uniform exit: (a) the vote needs a static
  // LDS variable, and next to one the compiler waits for the tile DMA right after issuing it; (b) an atomic on an int* BEFORE the loop
  // turns the NABLA list loads (int*, scalar loads) into vector loads whose vmcnt wait drains the DMA as well.  Either costs 6-14 %
  // of the whole kernel (measured, same box) — tests/test_abi_and_host.py pins the prefetch distance in the ISA.
  const bool wave_over = BOUNDED && PRE && QN && p.kmax && __any(over_limit);
  f32x4 lt[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) lt[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 onesf = __builtin_bit_cast(bf16x8, u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u});
  // addresses of this lane's running state (recomputed where needed: not kept live across the main loop)
  auto state_base = [&]() { return part == 0 ? p.state : p.split_state + (size_t)(part - 1) * p.split_stride; };
  // st_o_off / st_ml_off of (q0 + 16 qt + l15, h, 4 g): everything but the lane term is wave-uniform
  const uint32_t st_job = ((uint32_t)(h * p.nqb + qb) * 16u + (uint32_t)QT * (uint32_t)wave) * 4u;
  auto state_o = [&](int qt) { return state_base() + ((st_job + 4u * (uint32_t)qt) * 256u + (uint32_t)lane * 4u); };   // + 256 dt: the d tile
  auto state_ml = [&](int qt, int slot) {
    return state_base() + ((uint32_t)(p.H * p.nqb) * (256u * 64u) + (st_job + 4u * (uint32_t)qt + (uint32_t)slot) * 32u + (uint32_t)l15 * 2u);
  };
  if (RANGE && (p.flags & 1) && part == 0 && !(!BOUNDED && late)) {   // resume: accumulators of an earlier launch over other key tiles
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
      if (q0 + 16 * qt + l15 < p.q_len) {
        const float* st_o = state_o(qt);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) ot[dt][qt] = *reinterpret_cast<const f32x4*>(st_o + 256 * dt);
        if (!BOUNDED) { const float m = state_ml(qt, g)[0]; nm[qt] = f32x4{-m, -m, -m, -m}; }
        { const float L = (state_ml(qt, 0)[1] + state_ml(qt, 1)[1]) + (state_ml(qt, 2)[1] + state_ml(qt, 3)[1]); lt[qt] = f32x4{L, L, L, L}; }   // the four slots' row sums
      }
    if (!BOUNDED) {   // a state left by a launch that saw no tile carries m = -1e30: still fresh (wave-uniform by construction:
      bool allf = true;                                       // every query of a wave sees the same tiles; rows >= q_len keep 0)
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) allf = allf && nm[qt][0] > 1e29f;
      fresh = __all(allf);
      if (fresh) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) nm[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }

  bool seen = !SPARSE && T > E0;   // wave-uniform: this wave's queries saw at least one key tile in this launch
  if constexpr (PIPE) {
    if (T > E0) {
      // S^T of two tiles in flight: S[parity][half h][kt2][qt] = key sub-tile kt = 2 h + kt2 (16 keys) x query tile qt; pf[h][qt] = the packed probabilities
      // of half h waiting for their P V MFMAs
      f32x4 S[2][2][2][QT];
      bf16x8 pf[2][QT];
      // K / V^T fragments of a unit are read from LDS ONE UNIT AHEAD into the other of two register sets: with one wave per SIMD nothing else hides the
      // ~100 cycles of a ds_read (first build: every 4 MFMAs waited for their fragment — 701 TFLOP/s)
      bf16x8 kfr[2][2][2], vfr[2][4];      // [set][kt2][k-step], [set][d tile]
      auto ld_k = [&](auto SETC, auto HC, auto SLOTC) {
        constexpr int set = decltype(SETC)::value, hh = decltype(HC)::value, slot = decltype(SLOTC)::value;
        const char* cK = sK + slot * TILE;
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2) {
          const int kt = 2 * hh + kt2;
          kfr[set][kt2][0] = *reinterpret_cast<const bf16x8*>(cK + lds_swz_k(krow + 32 * (kt >> 1) + 4 * (kt & 1), g));
          kfr[set][kt2][1] = *reinterpret_cast<const bf16x8*>(cK + lds_swz_k(krow + 32 * (kt >> 1) + 4 * (kt & 1), 4 + g));
        }
      };
      auto ld_v = [&](auto SETC, auto HC, auto SLOTC) {
        constexpr int set = decltype(SETC)::value, hh = decltype(HC)::value, slot = decltype(SLOTC)::value;
        const char* cV = sV + slot * TILE;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) vfr[set][dt] = *reinterpret_cast<const bf16x8*>(cV + lds_swz(16 * dt + l15, 4 * hh + g));
      };
      auto qk_half = [&](auto PARC, auto HC) {      // 16 MFMAs on fragment set HC
        constexpr int par = decltype(PARC)::value, hh = decltype(HC)::value;
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2) {
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) S[par][hh][kt2][qt] = mfma16(kfr[hh][kt2][0], qf[qt][0], nm[qt]);
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) S[par][hh][kt2][qt] = mfma16(kfr[hh][kt2][1], qf[qt][1], S[par][hh][kt2][qt]);
        }
      };
      auto exp_half = [&](auto PARC, auto HC) {                 // 32 exponentials + 16 packs per lane
        constexpr int par = decltype(PARC)::value, hh = decltype(HC)::value;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          float e[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) e[j] = __builtin_amdgcn_exp2f(S[par][hh][j >> 2][qt][j & 3]);
          const u32x4 pk = {pack_bf16x2(e[0], e[1]), pack_bf16x2(e[2], e[3]), pack_bf16x2(e[4], e[5]), pack_bf16x2(e[6], e[7])};
          pf[hh][qt] = __builtin_bit_cast(bf16x8, pk);
        }
      };
      auto pv_half = [&](auto HC) {                 // 4 + 16 MFMAs on fragment set HC
        constexpr int hh = decltype(HC)::value;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) lt[qt] = mfma16(onesf, pf[hh][qt], lt[qt]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) ot[dt][qt] = mfma16(vfr[hh][dt], pf[hh][qt], ot[dt][qt]);
        }
      };
      // a unit's three streams are independent: ask for them interleaved, 3 matrix instructions to 4 vector ones (36 : 48), the 8 fragment reads of
      // the next unit up front
      auto mix = [&]() {
#ifndef K5_ATTN_PIPE_NOMIX
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
        for (int i = 0; i < 3 * QT; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
        }
#endif
      };
      using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
      // tile e sits in ring slot J (its K was used one body earlier); the next tile's K in slot (J + 1) % 6, the one after in (J + 2) % 6.
      // Unit (J, h) computes on fragment set h and reads the next unit's fragments — (J, 1), or (J + 1, 0) — into set h ^ 1.
      auto body = [&](auto JC, int e) {
        constexpr int J = decltype(JC)::value, PAR = J & 1;
        using PC = std::integral_constant<int, PAR>; using PN = std::integral_constant<int, PAR ^ 1>;
        using SV_ = std::integral_constant<int, J>; using SK_ = std::integral_constant<int, (J + 1) % 6>;
        using SV1 = std::integral_constant<int, (J + 1) % 6>; using SK1 = std::integral_constant<int, (J + 2) % 6>;
        if ((J & 1) == 0) {   // a pair starts: the pair after this one has landed for every wave, the pair before it is dead — fetch the one after next
          __syncthreads();
          if (e + 4 < T) load_tile(e + 4, (J + 4) % 6);
          if (e + 5 < T) load_tile(e + 5, (J + 5) % 6);
        }
        const bool more = e + 1 < T;     // wave-uniform
        if (more) {      // two units, straight-line (one scheduling region): no branch inside — a fragment set read from a slot that holds no tile is never used
          ld_k(I1{}, I1{}, SK_{}); ld_v(I1{}, I1{}, SV_{});                                  // fragments of unit (J, 1)
          qk_half(PN{}, I0{}); exp_half(PC{}, I1{}); pv_half(I0{});
          ld_k(I0{}, I0{}, SK1{}); ld_v(I0{}, I0{}, SV1{});                                  // fragments of unit (J + 1, 0)
          qk_half(PN{}, I1{}); exp_half(PN{}, I0{}); pv_half(I1{});
          mix(); mix();
        } else {
          ld_v(I1{}, I1{}, SV_{});
          exp_half(PC{}, I1{}); pv_half(I0{});
          pv_half(I1{});
        }
      };
      load_tile(E0, 0);
      if (E0 + 1 < T) load_tile(E0 + 1, 1);
      if (E0 + 2 < T) load_tile(E0 + 2, 2);
      if (E0 + 3 < T) load_tile(E0 + 3, 3);
      __syncthreads();
      // prologue: S^T of the first tile (both halves) and the probabilities of its first half; the fragments of unit (0, 0)
      ld_k(I0{}, I0{}, I0{}); ld_k(I1{}, I1{}, I0{});
      qk_half(I0{}, I0{}); qk_half(I0{}, I1{}); exp_half(I0{}, I0{});
      if (E0 + 1 < T) ld_k(I0{}, I0{}, I1{});
      ld_v(I0{}, I0{}, I0{});
      for (int e = E0; e < T; e += 6) {
        body(std::integral_constant<int, 0>{}, e);
        if (e + 1 >= T) break;
        body(std::integral_constant<int, 1>{}, e + 1);
        if (e + 2 >= T) break;
        body(std::integral_constant<int, 2>{}, e + 2);
        if (e + 3 >= T) break;
        body(std::integral_constant<int, 3>{}, e + 3);
        if (e + 4 >= T) break;
        body(std::integral_constant<int, 4>{}, e + 4);
        if (e + 5 >= T) break;
        body(std::integral_constant<int, 5>{}, e + 5);
      }
    }
  } else {
  if (T > E0) load_tile(E0, 0);
  if (PAIR && T > E0 + 1) load_tile(E0 + 1, 1);
  __syncthreads();   // drains the DMA (vmcnt) and publishes the tile(s)
  // one key tile; BUF (LDS slot) is a compile-time constant so that every ds_read address is
  // lane_base + immediate (the loop below is unrolled over the slots): no per-tile address arithmetic on the VALU
  auto tile_step = [&](auto BUFC, int e) {
    constexpr int buf = decltype(BUFC)::value;
    if (!PAIR) { if (e + 1 < T) load_tile(e + 1, buf ^ 1); }   // buffer buf^1 was last read before the barrier that ended tile e-1
    else if ((buf & 1) == 0) {   // first tile of a pair: the NEXT pair goes into the other two slots (last read before the previous barrier)
      if (e + 2 < T) load_tile(e + 2, buf ^ 2);
      if (e + 3 < T) load_tile(e + 3, (buf ^ 2) + 1);
    }
    const int t = tile_of(e);
    const char* cK = sK + buf * TILE;
    const char* cV = sV + buf * TILE;
    if (!SPARSE || (sp_list[e] & my_bit)) {   // wave-uniform: skip kv blocks this query block did not select
    if (SPARSE) seen = true;
    {
    // ---- S^T = K Q^T : four 16-key x two 16-query MFMA tiles, two k-steps over d; K fragments streamed from LDS ----
    f32x4 st[4][QT];
    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {   // first k-step starts from the constant 0, or from minus the query's softmax offset
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(cK + lds_swz_k(krow + 32 * (kt >> 1) + 4 * (kt & 1), g));
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
#ifdef K5_ATTN_NO_ROW_OFFSETS   // A/B build (tools/build_variant.sh): the fixed form's S^T starts from the inline constant 0
        st[kt][qt] = mfma16(kf, qf[qt][0], BOUNDED ? zero4 : nm[qt]);
#else
        st[kt][qt] = mfma16(kf, qf[qt][0], (BOUNDED && !PRE) ? zero4 : nm[qt]);   // BOUNDED && PRE: nm = minus the row's constant offset (0 without kmax)
#endif
      }
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(cK + lds_swz_k(krow + 32 * (kt >> 1) + 4 * (kt & 1), 4 + g));
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) st[kt][qt] = mfma16(kf, qf[qt][1], st[kt][qt]);
    }
    // lane (query l15 of tile qt, g): st[kt][qt][r] is key  t*64 + 32 (kt>>1) + 8 g + 4 (kt&1) + r
    if (!SPARSE && !PRE && t >= nfull) {  // ragged last tile (wave-uniform branch)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = t * KB + 32 * (kt >> 1) + 8 * g + 4 * (kt & 1) + r;
          if (key >= p.kv_len) {
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) st[kt][qt][r] = -1e30f;
          }
        }
    }
    if (!BOUNDED) {
      // lazy online max: st = score - offset.  Fold the lane's 16 values per query tile; nothing else happens unless some
      // lane's maximum left the safe window (or this is the wave's first tile, which sets the offset).
      float mx[QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        mx[qt] = max3(-3.0e38f, st[0][qt][0], st[0][qt][1]);   // a constant first operand: no canonicalising v_max
        mx[qt] = max3(mx[qt], st[0][qt][2], st[0][qt][3]);
        mx[qt] = max3(mx[qt], st[1][qt][0], st[1][qt][1]);
        mx[qt] = max3(mx[qt], st[1][qt][2], st[1][qt][3]);
        mx[qt] = max3(mx[qt], st[2][qt][0], st[2][qt][1]);
        mx[qt] = max3(mx[qt], st[2][qt][2], st[2][qt][3]);
        mx[qt] = max3(mx[qt], st[3][qt][0], st[3][qt][1]);
        mx[qt] = max3(mx[qt], st[3][qt][2], st[3][qt][3]);
      }
      float mxa = mx[0];
#pragma unroll
      for (int qt = 1; qt < QT; ++qt) mxa = fmaxf(mxa, mx[qt]);
      if (fresh || __any(mxa > ONLINE_THR)) {   // wave-uniform, rare
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          float mf = mx[qt];   // the query's four lanes (l15 + 16 g) combine -> identical offsets in all of them
          {
            const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(mf), __float_as_uint(mf), false, false);
            mf = fmaxf(__uint_as_float(s16[0]), __uint_as_float(s16[1]));   // max with lane ^ 16
            const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mf), __float_as_uint(mf), false, false);
            mf = fmaxf(__uint_as_float(s32[0]), __uint_as_float(s32[1]));   // max with lane ^ 32
          }
          const float dlt = fresh ? mf : fmaxf(mf, 0.f);   // an established offset is never lowered
          const float alpha = fresh ? 1.f : __builtin_amdgcn_exp2f(-dlt);
          { const float n = nm[qt][0] - dlt; nm[qt] = f32x4{n, n, n, n}; }
#pragma unroll
          for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) st[kt][qt][r] -= dlt;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) ot[dt][qt][r] *= alpha;
#pragma unroll
          for (int r = 0; r < 4; ++r) lt[qt][r] *= alpha;
        }
        fresh = false;
      }
    }
    // ---- P = exp2(S c - m c) -> bf16 fragments; O^T += V^T P^T (two k-steps of 32 keys), V^T fragments streamed ----
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {   // both query tiles' probabilities first (8 live registers), V^T fragments streamed
        bf16x8 pf[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          float e[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            e[j] = PRE ? __builtin_amdgcn_exp2f(st[2 * ks2 + (j >> 2)][qt][j & 3])
                       : __builtin_amdgcn_exp2f(st[2 * ks2 + (j >> 2)][qt][j & 3] * c);
          }
          u32x4 pk = {pack_bf16x2(e[0], e[1]), pack_bf16x2(e[2], e[3]), pack_bf16x2(e[4], e[5]), pack_bf16x2(e[6], e[7])};
          pf[qt] = __builtin_bit_cast(bf16x8, pk);
#ifdef K5_ATTN_NO_ROWSUM_MFMA   // A/B build for the ledger (tools/build_variant.sh -DK5_ATTN_NO_ROWSUM_MFMA): results WRONG, timing only — what the four
          if (ks2 == 7) lt[qt] = mfma16(onesf, pf[qt], lt[qt]);   // ones-row MFMAs per wave-tile cost in time (and, through the clock, in energy)
          else lt[qt][0] += 1.0f;
#else
          lt[qt] = mfma16(onesf, pf[qt], lt[qt]);   // every row = sum over the 32 keys of bf16(p) for query l15
#endif
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(cV + lds_swz(16 * dt + l15, 4 * ks2 + g));
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) ot[dt][qt] = mfma16(vf, pf[qt], ot[dt][qt]);
        }
      }
    }
    }
#if defined(K5_ATTN_SGB)   // A/B builds (tools/build_variant.sh): ask the scheduler for an explicit MFMA / VALU interleave of the tile body
    if (BOUNDED && PRE && !SPARSE) {
#if K5_ATTN_SGB == 1      // one VALU behind every MFMA
#pragma unroll
      for (int i = 0; i < 18 * QT; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 1, 0); }
#elif K5_ATTN_SGB == 2    // S phase: MFMA + LDS read; then MFMA + 2 VALU
#pragma unroll
      for (int i = 0; i < 8; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, QT / 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
#pragma unroll
      for (int i = 0; i < 14 * QT; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 2, 0); }
#elif K5_ATTN_SGB == 3    // two MFMAs, then three VALU
#pragma unroll
      for (int i = 0; i < 9 * QT; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x002, 3, 0); }
#elif K5_ATTN_SGB == 4    // LDS reads up front in pairs with MFMAs, transcendental after each MFMA, converts wherever
#pragma unroll
      for (int i = 0; i < 18 * QT; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x400, 1, 0); }
#endif
    }
#endif
    if (!PAIR) __syncthreads();   // vmcnt(0) + barrier: tile e+1 has landed for every wave, tile e's buffer is free
  };
  if (!PAIR) {
    for (int e = E0; e < T; e += 2) {
      tile_step(std::integral_constant<int, 0>{}, e);
      if (e + 1 >= T) break;
      tile_step(std::integral_constant<int, 1>{}, e + 1);
    }
  } else {
    for (int e = E0; e < T; e += 4) {
      tile_step(std::integral_constant<int, 0>{}, e);
      if (e + 1 < T) tile_step(std::integral_constant<int, 1>{}, e + 1);
      __syncthreads();   // vmcnt(0) + barrier: the next pair has landed for every wave, this pair's slots are free
      if (e + 2 >= T) break;
      tile_step(std::integral_constant<int, NBUF - 2>{}, e + 2);
      if (e + 3 < T) tile_step(std::integral_constant<int, NBUF - 1>{}, e + 3);
      __syncthreads();
    }
  }
  }   // !PIPE
  // In a multi-pass schedule (late_pass != 0) the flip writes the LATE flag: the launches of a pass are balanced as fixed(full),
  // online(full), fixed(tail), online(tail), so a flip that comes from a tail job lands after online(full) has skipped the head —
  // its full jobs keep fixed-form state (relative to the per-row offsets), which the online form of a later pass must not resume
  // as offset 0.  Flag 2 = every later launch skips the head and the last pass's online launch recomputes it from scratch.
  if (BOUNDED && PRE && QN && wave_over && lane == 0 && atomicCAS(const_cast<int*>(p.head_flags) + h, 1, p.late_pass ? 2 : 0) == 1 && p.variant_counters) {
    atomicAdd(p.variant_counters + 1, 1ull);
    atomicAdd(p.variant_counters, ~0ull);   // - 1
  }
  if (RANGE && (p.flags & 2)) {   // leave the running state for a later launch; no output yet
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
      if (q0 + 16 * qt + l15 < p.q_len) {
        float* st_o = state_o(qt); float* st_ml = state_ml(qt, g);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(st_o + 256 * dt) = ot[dt][qt];
        st_ml[0] = BOUNDED ? 0.f : (fresh ? -1e30f : -nm[qt][0]);   // no tile seen: weight 0 in a merge, "still fresh" on resume
        st_ml[1] = g == 0 ? lt[qt][0] : 0.f;                    // slot 0 carries the whole row sum
        // per-row offsets: a part whose own sum underflows flags the head (conservative: the row's total is at least this part's)
        if (BOUNDED && PRE && p.kmax && nm[qt][0] != 0.f && !((lt[qt][0] >= K5_ATTN_ROW_MIN || (anchored && !SPARSE)) && lt[qt][0] < K5_ATTN_ROW_MAX) && seen) {
          if (p.job_flags) const_cast<int*>(p.job_flags)[lid] = p.late_pass ? 2 : 1;
          else const_cast<int*>(p.head_flags)[h] = p.late_pass ? 2 : 0;
        }
      }
    return;
  }

  // ---- epilogue: normalise, store O[q][h*64 + d] ----
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float l_tot = lt[qt][0];   // the ones-MFMA left the whole row sum in every lane of the query's column
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    const int q = q0 + 16 * qt + l15;
    if (BOUNDED && PRE && p.kmax && q < p.q_len && nm[qt][0] != 0.f && !(l_tot >= K5_ATTN_ROW_MIN && l_tot < K5_ATTN_ROW_MAX)) {
      if (p.job_flags) const_cast<int*>(p.job_flags)[lid] = p.late_pass ? 2 : 1;
      else const_cast<int*>(p.head_flags)[h] = p.late_pass ? 2 : 0;
    }
    if (q < p.q_len) {
      bf16_t* op = p.O + (size_t)q * p.ldo + h * 64 + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        u32x2 o = {pack_bf16x2(ot[dt][qt][0] * inv, ot[dt][qt][1] * inv), pack_bf16x2(ot[dt][qt][2] * inv, ot[dt][qt][3] * inv)};
        *reinterpret_cast<u32x2*>(op + 16 * dt) = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// MFMA 32x32x16 formulation (one query per lane: S^T = K Q^T with key rows permuted so that the accumulator registers
// of a lane are its P^T operand).  Used for the ONLINE-max instantiations only: with the running max the 16x16x32
// formulation above has to take its two query tiles one after the other (register budget) and loses to this one
// (832 vs 966 TFLOP/s on N(0,1) data); with the fixed softmax offset the 16x16x32 kernel wins (1095 vs 1032).
// Register-staged tile loads (global -> VGPR -> LDS) as before.  State: slots 0,1 of the four (m, l) pairs per (q, h).
// ---------------------------------------------------------------------------------------------
template <bool BOUNDED, bool SPARSE, bool RANGE>
__global__ __launch_bounds__(512, 4) void attn_fwd32_kernel(AttnP p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE];
  char* sK = smem;
  char* sV = smem + 2 * TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
  const int gid = xcd_remap(blockIdx.x, gridDim.x);
  const int part = RANGE ? gid % p.splits : 0;
  const int lid = p.job0 + (RANGE ? gid / p.splits : gid);
  const int h = lid / p.nqb, qb = lid % p.nqb;
  const int q0 = qb * QB + wave * 32;

  // Q^T fragments (B operand): lane holds Q[q0 + l31][16kk + 8hi .. +8]
  bf16x8 qf[4];
  {
    const bf16_t* qp = p.Q + (size_t)min(q0 + l31, p.q_len - 1) * p.ldq + h * 64 + 8 * hi;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(qp + 16 * kk);
  }
  // loader mapping: 512 threads, one 16-B chunk of K and one of V^T each per tile
  const int lrow = tid >> 3, lc = tid & 7;
  const bf16_t* kbase = p.K + h * 64 + 8 * lc;
  const bf16_t* vbase = p.Vt + (size_t)(h * 64 + lrow) * p.ldvt + 8 * lc;
  const int lds_off = lds_swz(lrow, lc);
  const int* sp_list = SPARSE ? p.sp_list + (size_t)(h * p.nqb + qb) * p.sp_stride : nullptr;
  const int Tall = SPARSE ? p.sp_cnt[h * p.nqb + qb] : p.tile_cnt;
  // this workgroup's share of the tile sequence: positions [E0, T)  (everything unless the job is split)
  const int E0 = RANGE ? (int)(((long long)Tall * part) / p.splits) : 0;
  const int T = RANGE ? (int)(((long long)Tall * (part + 1)) / p.splits) : Tall;
  const int nfull = p.kv_len / KB;                    // key tiles with all 64 keys valid (NABLA: all of them)
  auto tile_of = [&](int e) -> int {                  // sequence position -> 64-key tile index (wave-uniform)
    if (SPARSE) return sp_list[e] & 0xffffff;
    if (!RANGE) return e;
    if (p.seg_len > 0) {
      int si = e / p.seg_len;
      const int j = e - si * p.seg_len;
      if (si >= p.seg_skip) ++si;
      return p.tile_off0 + si * p.seg_stride + j;
    }
    int t = e + p.tile_off0;
    if (t >= p.tile_skip_at) t += p.tile_skip_n;
    return t;
  };
  const int my_bit = 1 << (24 + (wave >> 1));         // this wave's 64-query block inside the 256-query workgroup
  u32x4 rk, rv;
  const int tiles_per_chunk = p.vt_chunk_keys > 0 ? p.vt_chunk_keys / KB : 0x7fffffff;
  auto load_tile = [&](int e) {   // e = position in the tile sequence; t = 64-key tile index
    const int t = tile_of(e);
    const int kv0 = t * KB;
    const bf16_t* vsrc = vbase + kv0;
    if (p.vt_chunk_keys > 0) {   // sequence-parallel V^T layout only (uniform branch): per-rank chunks
      const int chunk = t / tiles_per_chunk;
      vsrc = vbase + (long long)chunk * p.vt_chunk_stride + (kv0 - chunk * tiles_per_chunk * KB);
    }
    rk = *reinterpret_cast<const u32x4*>(kbase + (size_t)min(kv0 + lrow, p.kv_len - 1) * p.ldk);
    if (SPARSE || t < nfull) {
      rv = *reinterpret_cast<const u32x4*>(vsrc);
    } else {  // ragged last tile: never read past kv_len; zero-fill V^T (P is exactly 0 there)
      const int key = kv0 + 8 * lc;
      uint16_t e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        e[j] = (key + j < p.kv_len) ? reinterpret_cast<const uint16_t*>(vsrc)[j] : (uint16_t)0;
      rv = u32x4{(uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16),
                 (uint32_t)e[4] | ((uint32_t)e[5] << 16), (uint32_t)e[6] | ((uint32_t)e[7] << 16)};
    }
  };
  auto store_tile = [&](int buf) {
    *reinterpret_cast<u32x4*>(sK + buf * TILE + lds_off) = rk;
    *reinterpret_cast<u32x4*>(sV + buf * TILE + lds_off) = rv;
  };
  // K row permutation: MFMA row i reads key row pi(i) = i with bits 2 and 3 swapped
  const int krow = (l31 & 0x13) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);

  f32x16 ot[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[d][r] = 0.f;
  const float c = p.c;
  float m_run = BOUNDED ? 0.f : -1e30f, l_run = 0.f;
  const float mc_fixed = 0.f;
  // addresses of this lane's running state (recomputed where needed: not kept live across the main loop)
  auto state_base = [&]() { return part == 0 ? p.state : p.split_state + (size_t)(part - 1) * p.split_stride; };
  auto state_o = [&](int d) { return state_base() + st_o_off(q0 + l31, h, d, p.nqb); };   // d = 32 dd + 8 rg + 4 hi: this lane's 4 floats
  auto state_ml = [&](int slot) { return state_base() + st_ml_off(q0 + l31, h, slot, p.nqb, p.H); };
  if (RANGE && (p.flags & 1) && part == 0 && q0 + l31 < p.q_len) {   // resume: accumulators of an earlier launch over other key tiles
    const float* st_ml = state_ml(hi);
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(state_o(32 * d + 8 * rg + 4 * hi));
#pragma unroll
        for (int e = 0; e < 4; ++e) ot[d][4 * rg + e] = v[e];
      }
    if (!BOUNDED) m_run = st_ml[0];
    l_run = st_ml[1];
  }

  if (T > E0) { load_tile(E0); store_tile(0); }
  __syncthreads();
  // one key tile; BUF (LDS double-buffer half) is a compile-time constant so that every ds_read address is
  // lane_base + immediate (the loop below is unrolled by two): no per-tile address arithmetic on the VALU
  auto tile_step = [&](auto BUFC, int e) {
    constexpr int buf = decltype(BUFC)::value;
    if (e + 1 < T) load_tile(e + 1);
    const int t = tile_of(e);
    const char* cK = sK + buf * TILE;
    const char* cV = sV + buf * TILE;
    if (!SPARSE || (sp_list[e] & my_bit)) {   // wave-uniform: skip kv blocks this query block did not select
    // ---- S^T = K Q^T : two 32-key MFMA tiles, K fragments streamed from LDS ----
    f32x16 st[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 16; ++r) st[tt][r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(cK + lds_swz(krow, 2 * kk + hi));
      const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(cK + lds_swz(32 + krow, 2 * kk + hi));
      st[0] = mfma32(k0, qf[kk], st[0]);
      st[1] = mfma32(k1, qf[kk], st[1]);
    }
    // lane (q = l31, hi): st[tt][r] is key  t*64 + 32tt + 16(r>>3) + 8hi + (r&7)
    if (!SPARSE && t >= nfull) {  // ragged last tile (wave-uniform branch)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = t * KB + 32 * tt + 16 * (r >> 3) + 8 * hi + (r & 7);
          if (key >= p.kv_len) st[tt][r] = -1e30f;
        }
    }
    float mc;
    if (BOUNDED) {
      mc = mc_fixed;
    } else {  // online softmax: raw-score running max, rescale only when some row's max grew
      float mt = fmaxf(st[0][0], st[1][0]);
#pragma unroll
      for (int r = 1; r < 16; ++r) mt = fmaxf(fmaxf(mt, st[0][r]), st[1][r]);
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mt), __float_as_uint(mt), false, false);
      mt = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));  // max with the partner lane (l ^ 32)
      const float m_new = fmaxf(m_run, mt);
      if (__any(m_new > m_run)) {
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
        l_run *= alpha;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) ot[d][r] *= alpha;
        m_run = m_new;
      }
      mc = m_run * c;
    }
    // ---- P = exp2(S c - m c) -> bf16 fragments; O^T += V^T P^T, V^T fragments streamed ----
    float ls = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        e[j] = __builtin_amdgcn_exp2f(fmaf(st[s >> 1][8 * (s & 1) + j], c, -mc));
        ls += e[j];
      }
      u32x4 pk = {pack_bf16x2(e[0], e[1]), pack_bf16x2(e[2], e[3]), pack_bf16x2(e[4], e[5]), pack_bf16x2(e[6], e[7])};
      const bf16x8 pfs = __builtin_bit_cast(bf16x8, pk);
      const bf16x8 v0 = *reinterpret_cast<const bf16x8*>(cV + lds_swz(l31, 2 * s + hi));
      const bf16x8 v1 = *reinterpret_cast<const bf16x8*>(cV + lds_swz(32 + l31, 2 * s + hi));
      ot[0] = mfma32(v0, pfs, ot[0]);
      ot[1] = mfma32(v1, pfs, ot[1]);
    }
    l_run += ls;
    }
    if (e + 1 < T) store_tile(buf ^ 1);
    __syncthreads();
  };
  for (int e = E0; e < T; e += 2) {
    tile_step(std::integral_constant<int, 0>{}, e);
    if (e + 1 >= T) break;
    tile_step(std::integral_constant<int, 1>{}, e + 1);
  }
  if (RANGE && (p.flags & 2)) {   // leave the running state for a later launch; no output yet
    if (q0 + l31 < p.q_len) {
      float* st_ml = state_ml(hi);
      float* st_m2 = state_ml(hi + 2);
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const f32x4 v = {ot[d][4 * rg], ot[d][4 * rg + 1], ot[d][4 * rg + 2], ot[d][4 * rg + 3]};
          *reinterpret_cast<f32x4*>(state_o(32 * d + 8 * rg + 4 * hi)) = v;
        }
      st_ml[0] = m_run; st_ml[1] = l_run;
      st_m2[0] = m_run; st_m2[1] = 0.f;   // slots 2, 3 (the 16x16 kernel's lane groups): no contribution
    }
    return;
  }

  // ---- epilogue: normalise, store O[q][h*64 + d] ----
  float l_tot;
  {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
    l_tot = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  }
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
  const int q = q0 + l31;
  if (q < p.q_len) {
    bf16_t* op = p.O + (size_t)q * p.ldo + h * 64;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        u32x2 o = {pack_bf16x2(ot[d][4 * rg] * inv, ot[d][4 * rg + 1] * inv),
                   pack_bf16x2(ot[d][4 * rg + 2] * inv, ot[d][4 * rg + 3] * inv)};
        *reinterpret_cast<u32x2*>(op + 32 * d + 8 * rg + 4 * hi) = o;
      }
  }
}

// Merge the per-part running states of the split jobs [job0, job0 + njobs) and write their normalised rows of O.
// One workgroup per job, one thread per query: O = sum_s w_s O_s / sum_s w_s l_s,  w_s = exp2((m_s - max m) c)  (w_s = 1 when
// the softmax offset is fixed).  State layout: st_o_off / st_ml_off — (m, l) per (q, h, slot 0..3): l is that lane group's partial
// sum, m is common to the four.
__global__ __launch_bounds__(256) void attn_merge_kernel(const float* state0, const float* split_state, long long split_stride,
                                                         int splits, int job0, int H, int q_len, int nqb, float c, bf16_t* O, int ldo,
                                                         int bounded_all, const int* head_flags, float* state_out, const int* job_flags) {
  const int job = job0 + blockIdx.x, h = job / nqb, qb = job % nqb;
  const bool bounded = head_flags ? (head_flags[h] == 1 && !(job_flags && job_flags[job])) : bounded_all != 0;   // fixed offset: every part's weight is 1
  const int q = qb * QB + threadIdx.x;
  if (q >= q_len) return;
  const size_t ml0 = st_ml_off(q, h, 0, nqb, H), ml1 = st_ml_off(q, h, 1, nqb, H), ml2 = st_ml_off(q, h, 2, nqb, H), ml3 = st_ml_off(q, h, 3, nqb, H);
  float w[8], m = -3.0e38f, l = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float* st = s == 0 ? state0 : split_state + (size_t)(s - 1) * split_stride;
    w[s] = st[ml0];                          // m_s for now
    if (!bounded) m = fmaxf(m, w[s]);
  }
  for (int s = 0; s < splits; ++s) {
    const float* st = s == 0 ? state0 : split_state + (size_t)(s - 1) * split_stride;
    w[s] = bounded ? 1.f : __builtin_amdgcn_exp2f((w[s] - m) * c);
    l += w[s] * ((st[ml0 + 1] + st[ml1 + 1]) + (st[ml2 + 1] + st[ml3 + 1]));
  }
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  bf16_t* op = O + (size_t)q * ldo + h * 64;
#pragma unroll 4
  for (int d = 0; d < 64; d += 4) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < splits; ++s) {
      const float* st = s == 0 ? state0 : split_state + (size_t)(s - 1) * split_stride;
      const f32x4 v = *reinterpret_cast<const f32x4*>(st + st_o_off(q, h, d, nqb));
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += w[s] * v[e];
    }
    if (state_out) { *reinterpret_cast<f32x4*>(state_out + st_o_off(q, h, d, nqb)) = a; continue; }   // an intermediate pass: the merged state, not O
    u32x2 o = {pack_bf16x2(a[0] * inv, a[1] * inv), pack_bf16x2(a[2] * inv, a[3] * inv)};
    *reinterpret_cast<u32x2*>(op + d) = o;
  }
  if (state_out) {   // (m, l) of the merged parts in the layout the kernels resume from: m in all four slots, the row sum in slot 0
    // (this thread read its own (q, h) entries above and is the only one to write them: state_out may be state0)
    const float mm = bounded ? 0.f : m;
    state_out[ml0] = mm; state_out[ml0 + 1] = l; state_out[ml1] = mm; state_out[ml1 + 1] = 0.f;
    state_out[ml2] = mm; state_out[ml2 + 1] = 0.f; state_out[ml3] = mm; state_out[ml3 + 1] = 0.f;
  }
}

// Per-head choice between the fixed-offset and the online-max softmax, decided on the device from the data: qstat / kstat
// hold max |q_h|^2 and max |k'_h|^2 (k' = log2(e)/8 * k, the pre-scaled keys) over all rows, left by rmsnorm_rope_kernel
// (kstat: nk partial maxima at stride kstride — one per sequence-parallel rank after the gather).  Cauchy-Schwarz:
// every exp2 argument of head h lies in [-B, B], B = |q|max |k'|max; B <= limit -> flag 1 (fixed offset 0), else 0.
// The statistics are consumed: reset to 0 for the next producer.  counters[0 / 1] count heads sent each way.
// prefer_online (nullable, [H]): heads that the per-row-offset form served badly the last time this layer ran (attn_pref_update_kernel).
// rstat / krad_out (nullable, [H]): squared radii of the keys around their centres (k5_launch_rmsnorm_rope key_centre) in, radii with margin
// out; the head-level bound is then the smaller of |q|max kmax and |q|max R (the centred offsets' survival depends on the latter).
__global__ void attn_flags_kernel(float* qstat, float* kstat, int nk, int kstride, int H, float limit, int force_online,
                                  int* flags, unsigned long long* counters, float* kmax_out, const int* prefer_online, float* rstat, float* krad_out,
                                  int nq, int qstride, int anchored, unsigned int* leave_sig) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= H) return;
  float q2 = 0.f;   // nq partial maxima at stride qstride (Ulysses: one per rank that holds rows of this head's queries; otherwise 1)
  for (int i = 0; i < nq; ++i) { const float v = qstat[(size_t)i * qstride + h]; q2 = v == v ? fmaxf(q2, v) : __uint_as_float(0x7f800000u); }
  float k2 = 0.f;
  for (int i = 0; i < nk; ++i) { const float v = kstat[(size_t)i * kstride + h]; k2 = v == v ? fmaxf(k2, v) : __uint_as_float(0x7f800000u); }
  float b = sqrtf(q2) * sqrtf(k2) * 1.002f;   // margin: fp32 rounding of the norms and of the MFMA accumulation
  if (rstat && krad_out) {
    const float r2 = rstat[h];
    const float rr = r2 == r2 ? sqrtf(r2) * 1.002f : __uint_as_float(0x7f800000u);
    krad_out[h] = rr;
    if (b > K5_ATTN_EXP_LIMIT) b = fminf(b, sqrtf(q2) * rr * 1.002f);   // NaN-safe: fminf keeps the finite operand only when b is finite too
    rstat[h] = 0.f;
  }
  const bool pref = prefer_online && b > K5_ATTN_EXP_LIMIT && prefer_online[h];
  // anchored: a head beyond the window keeps the fixed form on offsets anchored at achieved scores (AttnP::row_anchor; marked by a
  // negative kmax entry) unless its jobs kept falling back (prefer_online); inf / NaN statistics go to the online form as before
  const bool anchor = anchored && kmax_out && !force_online && !pref && b > limit && b < 3.0e38f;
  const int fast = ((!force_online && b <= limit && !pref) || anchor) ? 1 : 0;   // NaN / inf compare false -> online
  flags[h] = fast;
  if (leave_sig && (!fast || anchor)) *leave_sig = 1u;   // the engine's per-call choice of where the queries are normalised (k5_sample) reads it
  if (kmax_out) kmax_out[h] = (anchor ? -1.f : 1.f) * sqrtf(k2) * 1.002f;   // negative = anchored head (the magnitude stays usable)   // per-row offsets of the fixed-offset form: |q_row| * this - 90 (AttnP::kmax)
  if (counters) atomicAdd(counters + (fast ? 0 : 1), 1ull);
  for (int i = 0; i < nq; ++i) qstat[(size_t)i * qstride + h] = 0.f;
  for (int i = 0; i < nk; ++i) kstat[(size_t)i * kstride + h] = 0.f;
}

// The Cauchy-Schwarz bound says where exp2 cannot overflow, not where a row's sum survives the offset built from it: data with a large
// common component (every score of a head near -0.4 bound) underflows row after row however small the bound.  The per-job fallback
// keeps that correct at the price of computing such jobs twice; this makes it a one-time price: after a layer's attention, a head
// more than a quarter of whose jobs fell back is remembered, and k5_launch_attn_flags sends it to the online form directly the next
// time the layer runs (the next sampler step: the statistics of a layer change slowly along the trajectory).  Never reset within a
// handle's life: a head that lost the fixed form does not get it back (no evidence would ever arrive).
// One wave per head (one thread per head walking its 186 flags serially measured 24 us per block: 0.8 ms per step for nothing).
__global__ __launch_bounds__(64) void attn_pref_update_kernel(const int* job_flags, int nqb, int H, int* prefer_online, unsigned int* leave_sig) {
  const int h = blockIdx.x;
  int cnt = 0;
  for (int j = threadIdx.x; j < nqb; j += 64) cnt += job_flags[h * nqb + j] != 0;
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (threadIdx.x == 0 && 4 * cnt > nqb) { prefer_online[h] = 1; if (leave_sig) *leave_sig = 1u; }
}

// Anchored offsets (K5_ATTN_ANCHOR_ADD): for every query row of a head marked by a negative kmax entry, the maximum score over a sample
// of K5_ANCHOR_TILES 16-key tiles — the four tiles of the row's own 64-token block (key index = query index + key0: self-attention;
// with RoPE and a trained model the row's best keys are its neighbours) and a strided sample of the whole key range — rounded up to an
// integer (the softmax is offset-invariant, and an integer offset keeps every bf16 probability what any other integer offset gives),
// plus the constant.  One wave per 16 query rows: S^T = K Q^T on MFMA 16x16x32 with both operands straight from global memory
// (the sample is 32 x 2 KB per head: cache-resident), 64 MFMAs per wave.  Pre-scaled keys: the scores ARE the exp2 arguments.
__global__ __launch_bounds__(512) void attn_row_anchor_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, int q_len, int kv_len,
                                                              int ldq, int ldk, int key0, float spread, const float* __restrict__ kmax,
                                                              float* __restrict__ out) {
  // the strided part of the sample is the same for every row of a head: staged once per workgroup (28 tiles x 16 keys x 128 B = 56 KB)
  __shared__ __attribute__((aligned(16))) char sk[(K5_ANCHOR_TILES - 4) * 16 * 128];
  const int h = blockIdx.y;
  if (!(kmax[h] < 0.f)) return;   // (1024 rows per workgroup: at 47 616 tokens the launch that finds no marked head is 1316 workgroups that leave at once)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int ntile = kv_len / 16;   // kv_len is a multiple of 64 (pre-scaled keys)
  for (int c = threadIdx.x; c < (K5_ANCHOR_TILES - 4) * 16 * 8; c += 512) {   // 16-B chunk c of row r of tile i: row-major, chunk XOR row (conflict-free fragment reads)
    const int i = c >> 7, r = (c >> 3) & 15, ch = c & 7;
    const int t = (int)(((long long)i * ntile) / (K5_ANCHOR_TILES - 4));
    *reinterpret_cast<u32x4*>(sk + (i * 16 + r) * 128 + ((ch ^ (r & 7)) << 4)) =
        *reinterpret_cast<const u32x4*>(K + (size_t)(16 * t + r) * ldk + h * 64 + 8 * ch);
  }
  __syncthreads();
  for (int it = 0; it < 2; ++it) {   // eight waves (the 56 KB of LDS allow two workgroups per CU: four waves per SIMD hide the loads' latency)
    const int blk = 16 * blockIdx.x + 8 * it + wave;   // one wave per 64-token block: its four 16-row tiles share every key fragment
    if (64 * blk >= q_len) return;                       // (no barrier below)
    bf16x8 qf[4][2];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      const bf16_t* qp = Q + (size_t)min(64 * blk + 16 * qt + l15, q_len - 1) * ldq + h * 64 + 8 * g;
      qf[qt][0] = *reinterpret_cast<const bf16x8*>(qp); qf[qt][1] = *reinterpret_cast<const bf16x8*>(qp + 32);
    }
    const int own = min(max((64 * blk + key0) / 64, 0), ntile / 4 - 1);
    float mx[4], sum[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) { mx[qt] = -3.0e38f; sum[qt] = 0.f; }
    auto fold = [&](bf16x8 kf0, bf16x8 kf1) __attribute__((always_inline)) {
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) {
        f32x4 st = mfma16(kf0, qf[qt][0], f32x4{0.f, 0.f, 0.f, 0.f});
        st = mfma16(kf1, qf[qt][1], st);   // lane (query l15 of tile qt, g): keys 4 g .. 4 g + 3 of the tile
        mx[qt] = fmaxf(mx[qt], fmaxf(fmaxf(st[0], st[1]), fmaxf(st[2], st[3])));
        sum[qt] += (st[0] + st[1]) + (st[2] + st[3]);
      }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // the block's own four tiles, from global memory
      const bf16_t* kp = K + (size_t)(16 * (4 * own + i) + l15) * ldk + h * 64 + 8 * g;
      fold(*reinterpret_cast<const bf16x8*>(kp), *reinterpret_cast<const bf16x8*>(kp + 32));
    }
#pragma unroll 4
    for (int i = 0; i < K5_ANCHOR_TILES - 4; ++i) {   // the head's strided tiles, from LDS
      const char* kp = sk + (i * 16 + l15) * 128;
      fold(*reinterpret_cast<const bf16x8*>(kp + ((g ^ (l15 & 7)) << 4)), *reinterpret_cast<const bf16x8*>(kp + (((4 + g) ^ (l15 & 7)) << 4)));
    }
    const float inv_n = 1.0f / (float)(16 * K5_ANCHOR_TILES);
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      float m = mx[qt], sm = sum[qt];
      {   // the query's four lanes (l15 + 16 g)
        const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
        m = fmaxf(__uint_as_float(s16[0]), __uint_as_float(s16[1]));
        const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
        m = fmaxf(__uint_as_float(s32[0]), __uint_as_float(s32[1]));
        const auto t16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(sm), __float_as_uint(sm), false, false);
        sm = __uint_as_float(t16[0]) + __uint_as_float(t16[1]);
        const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(sm), __float_as_uint(sm), false, false);
        sm = __uint_as_float(t32[0]) + __uint_as_float(t32[1]);
      }
      const float extra = fminf(fmaxf(spread * (m - sm * inv_n), 0.f), K5_ATTN_ANCHOR_EXTRA_MAX);
      const int row = 64 * blk + 16 * qt + l15;
      if (g == 0 && row < q_len) out[(size_t)h * q_len + row] = ceilf(m + extra) + K5_ATTN_ANCHOR_ADD;
    }
  }
}

}  // namespace

// Softmax offset policy.  score_bound > 0: the caller guarantees |q.k| <= score_bound for every pair (e.g. RMS-normalised
// q, k: 64 * max|w_q| * max|w_k|).  If score_bound * log2(e)/8 <= K5_ATTN_EXP_LIMIT, exp2 of the raw argument can neither
// overflow nor flush a whole row, so the kernels run with the constant offset 0 and skip the online running max.
// head_flags (device, [H], pre-scaled keys only): the same decision per head, taken on the device from the data
// (k5_launch_attn_flags) — flag 1: fixed offset, flag 0: lazy online max; both variants are launched over the same grid and
// each workgroup exits at once unless its head is its variant's.

size_t k5_attention_state_bytes(int H, int q_len) { return (size_t)H * ((q_len + QB - 1) / QB) * QB * (64 + 8) * sizeof(float); }   // st_o_off / st_ml_off

// Workspace of the balanced launcher below: up to K5_ATTN_MAX_SPLITS - 1 extra states + (when the caller passes no state
// of its own) one base state.
constexpr int K5_ATTN_MAX_SPLITS = 6;
// + the per-job fallback flags of the per-row-offset form (AttnP::job_flags): one int per (head, 128-query group)
size_t k5_attention_balance_bytes(int H, int q_len) {
  return (size_t)K5_ATTN_MAX_SPLITS * k5_attention_state_bytes(H, q_len) + (size_t)H * ((q_len + 63) / 64 + 1) * sizeof(int);   // one flag per job; the smallest job is a 64-query row
}
namespace {
inline int* attn_job_flags(float* ws, int H, int q_len) { return reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + (size_t)K5_ATTN_MAX_SPLITS * k5_attention_state_bytes(H, q_len)); }
inline size_t attn_job_flags_bytes(int H, int q_len) { return (size_t)H * ((q_len + 63) / 64 + 1) * sizeof(int); }
}  // namespace

namespace {
int g_attn_slots = 0;   // concurrently resident attention workgroups on the device: 2 per CU (128 VGPRs x 8 waves)
int attn_slots() {
  if (!g_attn_slots) {
    int dev = 0; hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 512;
    g_attn_slots = 2 * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
  }
  static const bool pipe = getenv("K5_ATTN_WAVE_ROWS") && atoi(getenv("K5_ATTN_WAVE_ROWS")) > 100;   // the pipelined forms (132, 164): one workgroup per CU
  return pipe ? g_attn_slots / 2 : g_attn_slots;
}
}  // namespace

int k5_launch_attn_pref_update(float* balance_ws, int H, int q_len, int group_rows, int* prefer_online, hipStream_t stream, unsigned int* leave_sig) {
  if (!balance_ws || !prefer_online || H <= 0 || q_len <= 0) return K5_ERR_ARG;
  const int nqb = (q_len + 64 * group_rows - 1) / (64 * group_rows);
  hipLaunchKernelGGL(attn_pref_update_kernel, dim3(H), dim3(64), 0, stream, attn_job_flags(balance_ws, H, q_len), nqb, H, prefer_online, leave_sig);
  return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP;
}

int k5_launch_attn_flags(float* qstat, float* kstat, int nk, int kstride, int H, int force_online, int* flags,
                         unsigned long long* counters, hipStream_t stream, float* kmax_out, const int* prefer_online, float* rstat, float* krad_out,
                         int nq, int qstride, bool anchored, unsigned int* leave_sig) {
  if ((rstat == nullptr) != (krad_out == nullptr) || (rstat && !kmax_out) || nq < 1) return K5_ERR_ARG;
  if (!qstat || !kstat || !flags || H <= 0 || nk <= 0) return K5_ERR_ARG;
  // with kmax_out the attention runs per-row offsets: heads up to K5_ATTN_ROWOFF_LIMIT keep the fixed-offset form
  hipLaunchKernelGGL(attn_flags_kernel, dim3((H + 63) / 64), dim3(64), 0, stream, qstat, kstat, nk, kstride, H,
                     kmax_out ? K5_ATTN_ROWOFF_LIMIT : K5_ATTN_EXP_LIMIT, force_online, flags, counters, kmax_out, kmax_out ? prefer_online : nullptr,
                     rstat, krad_out, nq, qstride, anchored ? 1 : 0, leave_sig);
  return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP;
}

// anchored offsets of the heads k5_launch_attn_flags(anchored) marked (negative kmax entry): out [H][q_len]; Kc = the keys to sample
// (kv_len of them), key0 = the index among them of query row 0's token, kv_total = the number of keys the attention will see (>= kv_len:
// a rank samples its own shard).  Dense attention only: under NABLA a row attends its kept blocks, among which a strided sample of ALL
// keys says little about the kept ones, and the one attempt at sampling the kept set (own block + two kept blocks; QK-norm gain 6 on the
// 10 s clip) sent half the heads to the online form with most jobs computed twice (985 ms per step against 384 for the online form;
// not root-caused) — so NABLA heads beyond the window keep the online form.
// Other heads' rows are left untouched.
int k5_launch_attn_row_anchor(const void* Q, const void* Kc, int H, int q_len, int kv_len, int ldq, int ldk, int key0, int kv_total,
                              const float* kmax, float* out, hipStream_t stream) {
  if (!Q || !Kc || !kmax || !out || H <= 0 || q_len <= 0 || kv_len < KB || (kv_len % KB) || (ldq & 7) || (ldk & 7)) return K5_ERR_ARG;
  hipLaunchKernelGGL(attn_row_anchor_kernel, dim3((q_len + 1023) / 1024, H), dim3(512), 0, stream, (const bf16_t*)Q, (const bf16_t*)Kc, q_len, kv_len,
                     ldq, ldk, key0, anchor_spread(kv_total > kv_len ? kv_total : kv_len), kmax, out);
  return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP;
}

namespace {
// What both launchers check and fill the same way.  job_rows: query rows per (head, query block) job; state / flags / late_pass / qn: the
// launch's pass of a schedule (the range launcher's own arguments, the list launcher's K5SparsePass).
struct AttnForms { bool bounded, run_fixed, run_online; };   // which softmax form(s) run: fixed offset, online max; per head when head_flags is given
int attn_common(const K5AttnArgs& a, int job_rows, float* state, int flags, int late_pass, const K5QueryNorm* qn, AttnP& p, AttnForms& f) {
  if (a.H <= 0 || a.q_len <= 0 || a.kv_len <= 0) return K5_ERR_ARG;
  if ((a.ldq & 7) || (a.ldk & 7) || (a.ldvt & 7) || (a.ldo & 3)) return K5_ERR_ALIGN;
  if (a.vt_chunk_keys < 0 || (a.vt_chunk_keys % KB) || (a.vt_chunk_stride & 7)) return K5_ERR_ALIGN;
  if ((a.head_flags || a.variant != K5_ATTN_AUTO) && !a.k_prescaled) return K5_ERR_ARG;
  if (a.k_prescaled && (a.kv_len % KB)) return K5_ERR_ARG;      // pre-scaled keys: whole key tiles only (no ragged-tile code)
  const float* kmax = a.row_offset_kmax;
  const K5KeyCentre* kc = a.key_centre;
  p.Q = (const bf16_t*)a.Q; p.K = (const bf16_t*)a.K; p.Vt = (const bf16_t*)a.Vt; p.O = (bf16_t*)a.O;
  p.H = a.H; p.q_len = a.q_len; p.kv_len = a.kv_len; p.ldq = a.ldq; p.ldk = a.ldk; p.ldvt = a.ldvt; p.ldo = a.ldo;
  p.nqb = (a.q_len + job_rows - 1) / job_rows;
  p.c = 0.125f * 1.44269504088896340736f;
  if (kmax && (!a.head_flags || !a.k_prescaled || a.variant != K5_ATTN_AUTO)) return K5_ERR_ARG;   // per-row offsets need the per-head flags (late fallback)
  p.kmax = kmax;
  p.kcentre = (kc && kmax) ? kc->centre : nullptr; p.krad = (kc && kmax) ? kc->radius : nullptr;
  p.row_anchor = (kc && kmax) ? kc->row_anchor : nullptr;
  if ((p.kcentre == nullptr) != (p.krad == nullptr)) return K5_ERR_ARG;
  if ((flags & 3) && !state) return K5_ERR_ARG;
  if (late_pass < 0 || late_pass > 2 || (late_pass && !kmax)) return K5_ERR_ARG;
  p.late_pass = late_pass; p.late_total = (a.kv_len + KB - 1) / KB;
  p.job_flags = nullptr;
  if (kmax && a.balance_ws) {   // per-row offsets with a workspace: fallback per job; the first pass of a schedule (it does not resume) clears the flags
    p.job_flags = attn_job_flags(a.balance_ws, a.H, a.q_len);
    if (!(flags & 1) && hipMemsetAsync(const_cast<int*>(p.job_flags), 0, attn_job_flags_bytes(a.H, a.q_len), a.stream) != hipSuccess) return K5_ERR_HIP;
  }
  p.q_norm_w = qn ? qn->w : nullptr; p.q_cos = qn ? qn->cos : nullptr; p.q_sin = qn ? qn->sin : nullptr;
  p.variant_counters = qn ? qn->counters : nullptr;
  p.vt_chunk_keys = a.vt_chunk_keys; p.vt_chunk_stride = a.vt_chunk_stride;
  p.sp_list = nullptr; p.sp_cnt = nullptr; p.sp_stride = 0; p.sp_begin = nullptr;
  p.tile_off0 = 0; p.tile_cnt = 0; p.tile_skip_at = 0x7fffffff; p.tile_skip_n = 0;
  p.seg_len = 0; p.seg_stride = 0; p.seg_skip = 0x7fffffff;
  p.state = state; p.flags = flags;
  p.job0 = 0; p.splits = 1; p.split_state = nullptr; p.split_stride = 0;
  f.bounded = a.score_bound > 0.f && a.score_bound * p.c <= K5_ATTN_EXP_LIMIT;
  f.run_fixed = a.head_flags ? a.variant == K5_ATTN_AUTO : (a.variant == K5_ATTN_AUTO && f.bounded);
  f.run_online = a.head_flags ? true : !f.run_fixed;
  // pre-scaled keys: the two forms partition the heads by the device flags (my_flag is set per launch)
  p.head_flags = (f.run_fixed && f.run_online) ? a.head_flags : nullptr; p.my_flag = 0;
  return K5_OK;
}

// BALANCED launch (balance, a workspace, and at least two parts): the jobs that fill whole rounds of the device's resident-workgroup slots
// run as usual; the jobs of the last, partially filled round are split 2-6 ways (at most max_parts) along the key sequence / the lists
// into short workgroups that fill the slots, and a merge kernel combines their states.  5208 jobs on 512 slots: 10.25 rounds instead
// of 11; an 8-GPU shard's 672 jobs: 1.33 instead of 2; the 2576 list jobs of a 4-GPU shard of the 10 s clip: 5.03 instead of 6.
// launch(njobs, ranged) picks the kernel(s); `ranged`: what the unsplit launch needs, the split one always does.
template <class L>
int attn_launch_balanced(const K5AttnArgs& a, AttnP& p, const AttnForms& f, bool balance, int max_parts, bool ranged, L launch) {
  const int jobs = a.H * p.nqb, slots = attn_slots();
  const int full = jobs / slots * slots, rem = jobs - full;
  int S = rem > 0 ? slots / rem : 1;
  if (S > K5_ATTN_MAX_SPLITS) S = K5_ATTN_MAX_SPLITS;
  if (S > max_parts) S = max_parts;
  static const bool no_balance = getenv("K5_ATTN_NO_BALANCE") != nullptr;   // A/B switch for benchmarking
  float* ws = a.balance_ws;
  if (!balance || !ws || S < 2 || no_balance) {
    launch(jobs, ranged);
    return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP;
  }
  if (full > 0) launch(full, ranged);
  // tail jobs, S parts each: part 0 resumes the caller's state if there is one, every part leaves its state
  const long long stride = (long long)(k5_attention_state_bytes(a.H, a.q_len) / sizeof(float));
  const int flags = p.flags;
  float* state = p.state;
  const bool to_state = (flags & 2) != 0;
  float* base = (flags & 1) ? state : ws;
  p.job0 = full; p.splits = S; p.state = base; p.split_state = ws + stride; p.split_stride = stride;
  p.flags = (flags & 1) | 2;
  launch(rem * S, true);
  // merge weights: 1 for the fixed-offset heads, exp2(m_s - max m) for the online ones (exp2 domain when the keys are pre-scaled)
  hipLaunchKernelGGL(attn_merge_kernel, dim3(rem), dim3(256), 0, a.stream, base, ws + stride, stride, S, full, a.H, a.q_len, p.nqb,
                     a.k_prescaled ? 1.f : p.c, (bf16_t*)a.O, a.ldo, (a.k_prescaled ? (f.run_fixed && !f.run_online) : f.bounded) ? 1 : 0,
                     (a.k_prescaled && f.run_fixed && f.run_online) ? a.head_flags : nullptr, to_state ? state : nullptr, p.job_flags);
  return hipGetLastError() == hipSuccess ? K5_OK : K5_ERR_HIP;
}
}  // namespace

// Dense attention over a key-tile range (see AttnP).  With a workspace (k5_attention_balance_bytes) the launch is balanced; a pass that
// leaves its state (flags & 2) only when the keys are pre-scaled (the engine's path): its merge writes the merged state instead of O.
// variant (pre-scaled keys only): K5_ATTN_AUTO = by score_bound / head_flags, K5_ATTN_ONLINE = force the lazy online max.
int k5_launch_attention_bf16_range(const K5AttnRangeArgs& a) {
  AttnP p; AttnForms f;
  const int rc = attn_common(a, QB, a.state, a.flags, a.late_pass, a.query_norm, p, f);
  if (rc != K5_OK) return rc;
  hipStream_t stream = a.stream;
  if (p.q_norm_w) {
    if (a.k_prescaled) {   // visual self-attention: norm + RoPE; both forms carry it; with per-row offsets the fixed form decides per head
      if (!p.q_cos || !p.q_sin || (a.row_offset_kmax && !a.head_flags)) return K5_ERR_ARG;
    } else if (!f.bounded) {
      return K5_ERR_UNSUPPORTED;   // unscaled keys (cross-attention): only the fixed-offset 16x16x32 kernel carries the fused norm
    }
  }
  const dim3 block(512);
  const int total_tiles = (a.kv_len + KB - 1) / KB;
  int tile_off0 = a.tile_off0, tile_cnt = a.tile_cnt, tile_skip_at = a.tile_skip_at, tile_skip_n = a.tile_skip_n;
  if (tile_cnt < 0) tile_cnt = total_tiles - tile_off0;
  const K5TileSegments* seg = a.segments;
  if (seg && seg->len > 0) {   // segmented walk: the last position must still be a real tile
    if (tile_off0 < 0 || tile_cnt <= 0 || seg->stride < seg->len || seg->skip < 0) return K5_ERR_ARG;
    int si = (tile_cnt - 1) / seg->len;
    const int j = (tile_cnt - 1) - si * seg->len;
    if (si >= seg->skip) ++si;
    if ((long long)tile_off0 + (long long)si * seg->stride + j >= total_tiles) return K5_ERR_ARG;
    p.seg_len = seg->len; p.seg_stride = seg->stride; p.seg_skip = seg->skip;
    tile_skip_at = 0x7fffffff; tile_skip_n = 0;
  } else if (tile_off0 < 0 || tile_skip_n < 0 || tile_off0 + tile_cnt + (tile_skip_at < total_tiles ? tile_skip_n : 0) > total_tiles) return K5_ERR_ARG;
  p.tile_off0 = tile_off0; p.tile_cnt = tile_cnt; p.tile_skip_at = tile_skip_at; p.tile_skip_n = tile_skip_n;
  const bool range = tile_off0 != 0 || tile_cnt != total_tiles || (a.flags & 3) || p.seg_len > 0;
  const bool run_fixed = f.run_fixed, run_online = f.run_online;
  auto launch = [&](int njobs, bool use_range) {
    const dim3 grid(njobs);
    if (a.k_prescaled) {   // always the RANGE instantiation (a superset; with the plain one the register allocator spills)
      if (p.q_norm_w) {
        if (run_fixed) { p.my_flag = 1; hipLaunchKernelGGL((attn_fwd_kernel<true, false, true, true, true>), grid, block, 0, stream, p); }
        if (run_online) { p.my_flag = 0; hipLaunchKernelGGL((attn_fwd_kernel<false, false, true, true, true>), grid, block, 0, stream, p); }
      } else {
        // the fixed form in 64-row waves (QT = 4: four waves per 256-query workgroup) when asked for — same bits, see the kernel's header
        static const int wave_rows = getenv("K5_ATTN_WAVE_ROWS") ? atoi(getenv("K5_ATTN_WAVE_ROWS")) : K5_ATTN_WAVE_ROWS_DEFAULT;
        if (run_fixed) {
          p.my_flag = 1;
          if (wave_rows == 64) hipLaunchKernelGGL((attn_fwd_kernel<true, false, true, true, false, 4, 4>), grid, dim3(256), 0, stream, p);
          else if (wave_rows == 132) {   // 32-row waves, two per SIMD (one 256-query workgroup per CU), software-pipelined over half tiles
            static bool attr = false;
            if (!attr) {
              if (hipFuncSetAttribute((const void*)attn_fwd_kernel<true, false, true, true, false, 4, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 12 * TILE) != hipSuccess) return;
              attr = true;
            }
            hipLaunchKernelGGL((attn_fwd_kernel<true, false, true, true, false, 4, 2, true>), grid, block, 12 * TILE, stream, p);
          }
          else if (wave_rows == 164) {   // 64-row waves, one per SIMD, software-pipelined over half tiles (PIPE)
            static bool attr = false;
            if (!attr) {
              if (hipFuncSetAttribute((const void*)attn_fwd_kernel<true, false, true, true, false, 4, 4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 12 * TILE) != hipSuccess) return;
              attr = true;
            }
            hipLaunchKernelGGL((attn_fwd_kernel<true, false, true, true, false, 4, 4, true>), grid, dim3(256), 12 * TILE, stream, p);
          }
          else hipLaunchKernelGGL((attn_fwd_kernel<true, false, true, true>), grid, block, 0, stream, p);
        }
        if (run_online) { p.my_flag = 0; hipLaunchKernelGGL((attn_fwd_kernel<false, false, true, true>), grid, block, 0, stream, p); }
      }
    }
    else if (f.bounded) hipLaunchKernelGGL((attn_fwd_kernel<true, false, true>), grid, block, 0, stream, p);
    else if (use_range) hipLaunchKernelGGL((attn_fwd32_kernel<false, false, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((attn_fwd32_kernel<false, false, false>), grid, block, 0, stream, p);
  };
  return attn_launch_balanced(a, p, f, !(a.flags & 2) || a.k_prescaled, tile_cnt / 8 /* keep >= 8 key tiles per part */, range, launch);
}

// NABLA block-sparse attention (flex_attention(q,k,v,block_mask) nn.py:257-280): `list`/`cnt` are the per-workgroup
// union lists produced by k5_launch_nabla_select[_rect] (stride = number of 64-key blocks).  q_len, kv_len multiples of 64;
// V^T optionally in per-rank chunks (sequence parallel).  Balanced like the dense launches (256-query jobs, pre-scaled keys).
int k5_launch_attention_bf16_sparse(const K5AttnSparseArgs& a) {
  if ((a.q_len % KB) || (a.kv_len % KB) || !a.list || !a.cnt) return K5_ERR_ARG;
  if (a.pair_stride < 0 || (a.pair_stride > 0 && a.group_rows != 2)) return K5_ERR_ARG;
  const K5SparsePass* pass = a.pass;
  const int group_rows = a.group_rows;
  if (group_rows != 4 && ((group_rows != 2 && group_rows != 1) || !a.k_prescaled || pass)) return K5_ERR_ARG;   // lists of 2 rows / 1 row: 128- / 64-query workgroups (ws: job flags only)
  // one pass of a two-pass walk of the lists (sequence parallelism): [begin, cnt) of every list, fp32 state in / out
  if (pass && (!a.k_prescaled || !pass->state || (pass->flags & ~3))) return K5_ERR_ARG;
  AttnP p; AttnForms f;
  const int rc = attn_common(a, 64 * group_rows, pass ? pass->state : nullptr, pass ? pass->flags : 0, pass ? pass->late_pass : 0, nullptr, p, f);
  if (rc != K5_OK) return rc;
  hipStream_t stream = a.stream;
  p.sp_list = a.list; p.sp_cnt = a.cnt; p.sp_stride = a.list_stride; p.sp_begin = pass ? pass->begin : nullptr;
  p.pair_stride = a.pair_stride;
  const dim3 block(512);
  const bool run_fixed = f.run_fixed, run_online = f.run_online;
  auto launch = [&](int njobs, bool rangek) {
    const dim3 g(njobs);
    if (!a.k_prescaled) {
      if (f.bounded) hipLaunchKernelGGL((attn_fwd_kernel<true, true, false>), g, block, 0, stream, p);
      else hipLaunchKernelGGL((attn_fwd32_kernel<false, true, false>), g, block, 0, stream, p);
    } else if (group_rows == 1) {
      if (run_fixed) { p.my_flag = 1; hipLaunchKernelGGL((attn_fwd_kernel<true, true, false, true, false, 1>), g, dim3(128), 0, stream, p); }
      if (run_online) { p.my_flag = 0; hipLaunchKernelGGL((attn_fwd_kernel<false, true, false, true, false, 1>), g, dim3(128), 0, stream, p); }
    } else if (group_rows == 2) {
      if (run_fixed) { p.my_flag = 1; hipLaunchKernelGGL((attn_fwd_kernel<true, true, false, true, false, 2>), g, dim3(256), 0, stream, p); }
      if (run_online) { p.my_flag = 0; hipLaunchKernelGGL((attn_fwd_kernel<false, true, false, true, false, 2>), g, dim3(256), 0, stream, p); }
    } else if (rangek) {
      if (run_fixed) { p.my_flag = 1; hipLaunchKernelGGL((attn_fwd_kernel<true, true, true, true>), g, block, 0, stream, p); }
      if (run_online) { p.my_flag = 0; hipLaunchKernelGGL((attn_fwd_kernel<false, true, true, true>), g, block, 0, stream, p); }
    } else {
      if (run_fixed) { p.my_flag = 1; hipLaunchKernelGGL((attn_fwd_kernel<true, true, false, true>), g, block, 0, stream, p); }
      if (run_online) { p.my_flag = 0; hipLaunchKernelGGL((attn_fwd_kernel<false, true, false, true>), g, block, 0, stream, p); }
    }
  };
  return attn_launch_balanced(a, p, f, a.k_prescaled && group_rows == 4 && a.balance, K5_ATTN_MAX_SPLITS, pass != nullptr, launch);
}
