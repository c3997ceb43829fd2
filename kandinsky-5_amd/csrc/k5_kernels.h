// k5_kernels.h — internal C++ launchers shared by the C-ABI layer (k5_api.hip) and the engine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k5.h"  // status codes, epilogue ids (public C ABI)

// Operand footprint of the GEMMs (bf16 and e4m3): the four-wave kernels and the q4 tail fetch a ragged tile's operand rows with buffer loads whose
// per-instruction row offset is not range-checked, so up to 143 rows past an operand's last row are READ (never used: they land in accumulator
// rows that are not stored).  They must be mapped memory: whoever allocates an activation or weight buffer that a GEMM reads adds this many rows.
constexpr int K5_GEMM_GUARD_ROWS = 144;
int k5_launch_gemm_bf16(const void* A, const void* W, const float* bias, void* C, int M, int N, int K,
                        int lda, int ldw, int ldc, int epi, const void* resid, int ldr,
                        const float* gate, hipStream_t stream,
                        int force_kernel = 0,    // k5_gemm_bf16_variant's kernel ids 0 / 2 / 4 / 8 (anything else: K5_ERR_ARG); 2 = the 128 x 128 kernel whatever the shape (callers that must keep a summation order)
                        int force_mt = 0);       // four-wave kernel: 16-row token tiles per wave, 8 / 6 / 4 = 256- / 192- / 128-row workgroup tiles (0 = by cost)

// Attention: O[q][h*64+d] = softmax(Q K^T / 8) V, bf16, head_dim 64, non-causal.
//   Q  [q_len][ldq]  (head h at columns h*64..), K [kv_len][ldk], Vt [H*64][ldvt] = V transposed, O [q_len][ldo].
// General form: process key tiles  e -> e + tile_off0 (+ tile_skip_n once >= tile_skip_at), e < tile_cnt (-1 = to the end);
// flags & 1: resume from `state`, flags & 2: write `state` instead of O (k5_attention_state_bytes floats-as-bytes).
size_t k5_attention_state_bytes(int H, int q_len);
// segmented walk instead of the (offset, skip) one: position e -> tile_off0 + seg(e / len) * stride + e % len, where segments
// >= skip shift up by one (the sequence-parallel schedule's "slice s of every rank's slot except mine"); tile_cnt positions
struct K5TileSegments { int len, stride, skip; };
// one pass of a two-pass walk of the NABLA lists (pre-scaled keys): list positions [begin[w], cnt[w]) of workgroup w (begin null: 0);
// state (k5_attention_state_bytes) is resumed with flags & 1 and left — no output — with flags & 2; late_pass as in the range launcher
struct K5SparsePass { const int* begin; float* state; int flags; int late_pass; };
// norm_qk (+ apply_rotary) of the QUERY rows fused into the attention kernel's Q-fragment load: Q then holds the raw projection.
// w: 64 RMSNorm weights.  cos / sin null: cross-attention (unscaled keys; K5_ERR_UNSUPPORTED unless score_bound selects the fixed-offset
// kernel).  cos / sin [row][32] fp32: visual self-attention (pre-scaled keys); with row_offset_kmax the fixed-offset workgroups then
// decide per head themselves (a row bound above 190 flips the head's flag to the online form; counters [fixed, online] follow).
struct K5QueryNorm { const float* w; const float* cos; const float* sin; unsigned long long* counters; };
// Centred form of the per-row offsets (AttnP::kcentre): centre [H][64] = a convex combination of each head's keys (k5_launch_rmsnorm_rope
// key_centre), radius [H] = max |k' - centre| with margin (k5_launch_attn_flags krad_out).  Rows whose plain bound |q| kmax exceeds 90 run
// with the offset q.c + |q| R - 90: no overflow, and no row-sum underflow while |q| R <= 190 whatever common component the scores carry.
// row_anchor (nullable, [H][q_len]): anchored offsets of the heads k5_launch_attn_flags(anchored) marked with a negative kmax entry
// (k5_launch_attn_row_anchor) — AttnP::row_anchor
struct K5KeyCentre { const float* centre; const float* radius; const float* row_anchor = nullptr; };
// softmax form of the pre-scaled-key launches: AUTO = fixed offset where the bound (score_bound, or the per-head device
// flags) allows it and the lazy online max elsewhere; ONLINE = the online max everywhere
enum { K5_ATTN_AUTO = 0, K5_ATTN_ONLINE = 1 };
// Arguments of the attention launchers: what both take, then what only one of them does.  The defaults are a plain one-launch call.
struct K5AttnArgs {
  const void* Q = nullptr; const void* K = nullptr; const void* Vt = nullptr; void* O = nullptr;
  int H = 0, q_len = 0, kv_len = 0, ldq = 0, ldk = 0, ldvt = 0, ldo = 0;
  float score_bound = 0.f;                          // caller-proved bound |q.k| <= score_bound (0 = unknown -> online running max)
  int vt_chunk_keys = 0; long long vt_chunk_stride = 0;   // V^T stored as per-rank chunks (sequence parallelism): keys [c*chunk_keys, (c+1)*chunk_keys) live at Vt + c*chunk_stride, row stride ldvt
  hipStream_t stream = nullptr;
  float* balance_ws = nullptr;                      // k5_attention_balance_bytes: balanced launch + the per-job fallback flags of the per-row-offset form
  bool k_prescaled = false;
  const int* head_flags = nullptr; int variant = K5_ATTN_AUTO;
  const float* row_offset_kmax = nullptr;           // per-row offsets of the fixed-offset form (k5_launch_attn_flags kmax_out)
  const K5KeyCentre* key_centre = nullptr;          // centred / anchored per-row offsets (with row_offset_kmax), see K5KeyCentre
};
struct K5AttnRangeArgs : K5AttnArgs {
  int tile_off0 = 0, tile_cnt = -1, tile_skip_at = 0x7fffffff, tile_skip_n = 0;
  float* state = nullptr; int flags = 0;
  int late_pass = 0;                                // AttnP::late_pass (multi-pass + per-row offsets)
  const K5TileSegments* segments = nullptr;
  const K5QueryNorm* query_norm = nullptr;          // fused norm_qk (+ RoPE) of the query rows, see K5QueryNorm
};
int k5_launch_attention_bf16_range(const K5AttnRangeArgs& a);
size_t k5_attention_balance_bytes(int H, int q_len);
// per-head flags from the |q|^2 / |k'|^2 maxima that k5_launch_rmsnorm_rope(stats) left (consumed: reset to 0); kstat holds
// nk partial maxima at stride kstride floats; counters (optional, device u64[2]) += heads sent to {fixed, online}
// kmax_out (nullable, H floats): max |k'_h| with margin for the per-row offsets of the fixed-offset form (row_offset_kmax of the
// attention launchers); with it heads up to a bound of 190 (instead of 90) keep that form — a row whose sum underflows sends its
// head to the online form late (the flag is rewritten by the attention kernel)
// prefer_online (nullable, H ints, with kmax_out only): heads to send to the online form although their bound is within the per-row-offset
// window — k5_launch_attn_pref_update sets the entry of a head more than a quarter of whose (head, query block) jobs fell back the
// last time (job flags at the end of the balance workspace that run's attention launches used; group_rows 2: 128-query jobs)
int k5_launch_attn_flags(float* qstat, float* kstat, int nk, int kstride, int H, int force_online, int* flags,
                         unsigned long long* counters, hipStream_t stream, float* kmax_out = nullptr, const int* prefer_online = nullptr,
                         float* rstat = nullptr, float* krad_out = nullptr,   // squared radii in (consumed) / radii with margin out: K5KeyCentre::radius
                         int nq = 1, int qstride = 0,                          // qstat as nq partial maxima at stride qstride (Ulysses)
                         bool anchored = false,    // heads beyond the window: fixed form on anchored offsets (kmax_out entry < 0) instead of the online form
                         unsigned int* leave_sig = nullptr);   // nullable: set to 1 when any head leaves the plain fixed-offset form (online or anchored)
int k5_launch_attn_row_anchor(const void* Q, const void* Kc, int H, int q_len, int kv_len, int ldq, int ldk, int key0, int kv_total,
                              const float* kmax, float* out, hipStream_t stream);
int k5_launch_attn_pref_update(float* balance_ws, int H, int q_len, int group_rows, int* prefer_online, hipStream_t stream,
                               unsigned int* leave_sig = nullptr);   // nullable: set to 1 when a head is marked

// ---- fp8 (e4m3) feed-forward path, opt-in (gemm_fp8.hip) ----
int k5_launch_gemm_fp8(const void* A8, const void* W8, const float* w_scale, void* C, int M, int N, int K, int lda, int ldw, int ldc,
                       int epi, const void* resid, int ldr, const float* gate, hipStream_t stream, const float* bias = nullptr, int scale_m = 0);
int k5_launch_quant_rows_fp8(const void* x, void* out, float* scale, int rows, int K, int ldx, int ldo, hipStream_t stream);

// ---- NABLA (block-sparse) ----
size_t k5_nabla_workspace_bytes(int H, int nb, int nqb = 0, int list_rows = 0);   // nqb: query-block rows selected here (0 = all nb); list_rows: key-tile lists per head (0 = one per row)
int k5_launch_nabla_select(const void* q, const void* k, int ldq, int ldk, int H, int N, int T, int Hb, int Wb, int wT, int wH,
                           int wW, float P, void* workspace, hipStream_t s);
void k5_nabla_workspace_views(void* workspace, int H, int nb, const unsigned long long** bits, const int** kv_nb, const int** list,
                              const int** cnt, const int** cnt_local = nullptr, int nqb = 0);   // nqb as given to k5_nabla_workspace_bytes (the lists sit behind that many rows of logits)
int k5_launch_nabla_select_rect(const void* q, const void* k, int ldq, int ldk, int H, int Nq, int q_block0, int N, int T, int Hb,
                                int Wb, int wT, int wH, int wW, float P, void* workspace, hipStream_t s,
                                int local_block0 = 0, int local_blocks = 0,   // > 0: these key blocks lead every list (cnt_local of them)
                                int group_rows = 4,                           // 64-query rows per list (4, or 2 for the 128-query workgroups)
                                int pair_stride = 0);                         // group_rows 2: which two rows share a list (k5_pair_row; 0 = adjacent)
// sequence parallelism: a rank's key-block means (k5_launch_nabla_block_means into its slot of a [P][H][slot_blocks][64] buffer),
// gathered, re-laid into the workspace (k5_launch_nabla_key_means_from_slots); k5_launch_nabla_select_rect(k = nullptr) selects from them
int k5_launch_nabla_block_means(const void* x, int ld, int H, int nblocks, int stride_blocks, void* out, hipStream_t s);
void k5_nabla_workspace_means(void* workspace, int H, int nb, void** qa, void** ka);   // the means' regions (k5_launch_rmsnorm_rope mean_q / mean_k write them directly)
int k5_launch_nabla_key_means_from_slots(const void* gathered, int H, int nb, int slot_blocks, void* workspace, hipStream_t s);
int k5_launch_nabla_mask_u8(const void* workspace, int H, int nqb, int nb, void* out, hipStream_t s);
// *acc += number of kept (query block, key block) pairs of the map in `workspace` (H x nqb rows)
int k5_launch_nabla_count(const void* workspace, int H, int nqb, int nb, unsigned long long* acc, hipStream_t s);
int k5_launch_nabla_count_lists(const void* workspace, int H, int nqb, int nb, int group_rows, unsigned long long* acc, hipStream_t s);
struct K5AttnSparseArgs : K5AttnArgs {
  const int* list = nullptr; const int* cnt = nullptr; int list_stride = 0;
  const K5SparsePass* pass = nullptr;               // pre-scaled keys
  int group_rows = 4;    // 2: lists per TWO 64-query rows (k5_launch_nabla_select_rect group_rows = 2), 128-query workgroups
  bool balance = true;   // false: balance_ws only carries the per-job fallback flags of the per-row-offset form
  int pair_stride = 0;   // group_rows 2: rows of a group per k5_pair_row (the stride the lists were built with)
};
int k5_launch_attention_bf16_sparse(const K5AttnSparseArgs& a);

// K1: out = bf16( LayerNorm(x; eps 1e-5, no affine) * (scale + 1) + shift )
// out_e4m3 (nullable, [rows][D] bytes): also — or, with out == nullptr, only — e4m3(bf16(.)) at the static scale 1: the activation operand of
// the fp8 GEMMs without a separate quantisation pass (what k5_launch_quant_rows_fp8(scale = nullptr) makes of the bf16 rows, bit for bit)
int k5_launch_ln_modulate(const void* x, const float* scale, const float* shift, void* out, int rows,
                          int D, int ldx, int ldo, hipStream_t stream, void* out_e4m3 = nullptr);
// K5 + K3: in place over [rows][ld] (H heads of 64): RMSNorm(eps, weight) -> bf16 -> RoPE (optional)
//   x holds H heads per row; head h uses weight[(h / heads_per_weight)*64 ..]; RoPE (cos/sin [rows][32]) on heads
//   < rope_heads.  heads_cfg = host pointer to {heads_per_weight, rope_heads} or null (= {H, H}).
int k5_launch_rmsnorm_rope(void* x, const float* weight, const float* cos, const float* sin, int rows,
                           int H, int ld, const int32_t* heads_cfg, hipStream_t stream,
                           float out_scale = 1.f, int scale_from_head = 0x7fffffff, void* scaled_out = nullptr, int ld_scaled = 0,
                           float* stats = nullptr, float* stats_ws = nullptr,
                           float* key_centre = nullptr,    // OUT [H - scale_from_head][64]: sample-mean key per scaled head; stats then also gets H - scale_from_head squared radii |k' - c|^2
                           // NABLA (rows % 64 == 0): 64-token block means of the UNSCALED normalised + rotated heads, taken in this pass (what
                           // k5_launch_nabla_block_means computes from the stored tensor): heads < scale_from_head -> mean_q [head][mq_stride][64] bf16,
                           // the others -> mean_k [head - scale_from_head][mk_stride][64]
                           void* mean_q = nullptr, int mq_stride = 0, void* mean_k = nullptr, int mk_stride = 0);
size_t k5_rmsnorm_stats_workspace_bytes(int H);
// Ulysses sequence parallelism: (q | k) rows [rows][2 D] -> per-destination blocks [P][slot_rows][2 D / P]; outputs [P][slot_rows][D / P] -> [rows][D]
int k5_launch_ulysses_pack_qk(const void* x, void* out, int rows, int slot_rows, int D, int P, hipStream_t s);
int k5_launch_ulysses_unpack_o(const void* in, void* out, int rows, int slot_rows, int D, int P, hipStream_t s);   // stats_ws: scratch of this size whenever stats is given
int k5_launch_sp2d_pack_qk(const void* x, void* q_out, void* k_out, int rows, int slot_rows, int D, int G, hipStream_t s);   // two-level schedule: q / k' send planes [G][slot_rows][D / G]
// heads >= scale_from_head are multiplied by out_scale before the bf16 rounding — in place, or (scaled_out != null) into
// scaled_out[row][(head - scale_from_head) * 64 ...] while the unscaled values stay in place.
// stats (device, [H] floats, zeroed by the consumer): stats[h] = max(stats[h], |x_row,h|^2) over the rows of the call, of the
// values the softmax reads (the scaled ones for heads >= scale_from_head) -> data-derived softmax bound (k5_launch_attn_flags)
// K15: cos/sin tables [T*H*W][32] for RoPE3D, n0 + n1 + n2 = 32 (RoPE1D: H=W=1, n1=n2=0, p1 = p2 = null), optional token permutation
int k5_launch_rope_table(float* cosT, float* sinT, const int32_t* p0, const int32_t* p1, const int32_t* p2, int T,
                         int H, int W, int n0, int n1, int n2, float s0, float s1, float s2, const int32_t* tok_perm,
                         hipStream_t stream);
// K2 (standalone form): out = bf16(x + gate * y)
int k5_launch_gate_sum(const void* x, const void* y, const float* gate, void* out, int rows, int D,
                       hipStream_t stream);
// MagCache calibration: res = bf16(vis - ori) (the bits of k5_launch_gate_sum with the -1 gate; res may alias ori) and, when prev != null, over
// the rows with |res_i| > 0 and |prev_i| > 0: sums[0..3] = sum rho_i | sum rho_i^2 | sum (1 - cos(res_i, prev_i)) | rows counted, with
// rho_i = |res_i| / |prev_i| (fp32 row sums over the bf16 values of res as stored, float64 across rows in a fixed order: no atomics, the bits
// repeat).  part: device scratch of 4 * k5_magcache_stats_blocks(rows) doubles.  accumulate != 0: the four sums are ADDED to sums[].
// prev == null: only res is written; sums[] is zeroed (accumulate == 0) or left alone.  D any multiple of 8.
int k5_magcache_stats_blocks(int rows);
int k5_launch_magcache_stats(const void* vis, const void* ori, const void* prev, void* res, double* sums, double* part, int accumulate,
                             int rows, int D, hipStream_t stream);
// fp32 GEMV with optional SiLU on the input: y[n] = sum_k act(x[k]) * W[n][k] + b[n]   (K11, K12)
int k5_launch_gemv_f32(const float* x, const float* W, const float* b, float* y, int N, int K, int silu_in,
                       const float* add, hipStream_t stream);
// sinusoidal time features (K12): out[0..D/2) = cos(t f_i), out[D/2..D) = sin(t f_i)
// tvec/step (both or neither): read the time from tvec[*step] on the device (hipGraph-replayable sampler step)
int k5_launch_time_features(float t, float* out, int D, hipStream_t stream, const float* tvec = nullptr, const int* step = nullptr);
int k5_launch_step_inc(int* step, hipStream_t stream);
// LayerNorm with affine over bf16 rows (K13): out = bf16(LN(x) * w + b); also fp32 output option
int k5_launch_ln_affine(const void* x, const float* w, const float* b, void* out_bf16, float* out_f32, int rows,
                        int D, hipStream_t stream);
// patchify (K14) fp32 latent (T,H,W,C) [+ zero visual_cond channels] -> bf16 [Ntok][Kpad], optional
// token permutation (fractal order, K16)
int k5_launch_patchify(const float* x, void* out, int T, int H, int W, int C, int Cin_total, int Kpad,
                       const int32_t* tok_perm, hipStream_t stream);
// patchify of torch.cat([x, vcond], -1) from the two sources: x fp32 (T,H,W,C), vcond fp32 (T,H,W,Cin_total-C) (the visual_cond
// latent and mask); the same bits as k5_launch_patchify on the concatenated tensor
int k5_launch_patchify_cond(const float* x, const float* vcond, void* out, int T, int H, int W, int C, int Cin_total, int Kpad,
                            const int32_t* tok_perm, hipStream_t stream);
// patchify of a (T,H,W) box inside a larger tensor: x with its own frame and row strides (elements; cells of a row C apart), vcond (nullable:
// the conditioning channels are then zero) with its own.  Compact strides give k5_launch_patchify / k5_launch_patchify_cond bit for bit; only
// cells of the box are read.  K5_ERR_ARG, nothing launched: what they refuse, and a row stride < W cells or a frame stride < H rows.
int k5_launch_patchify_view(const float* x, int64_t x_frame, int64_t x_row, const float* vcond, int64_t vc_frame, int64_t vc_row, void* out,
                            int T, int H, int W, int C, int Cin_total, int Kpad, const int32_t* tok_perm, hipStream_t stream);
// un-patchify (K17 tail): [Ntok][C*4] bf16 (feature order c,ph,pw) -> (T,H,W,C) bf16, token perm optional
int k5_launch_unpatchify(const void* x, void* out, int T, int Hp, int Wp, int C, int ldx,
                         const int32_t* tok_perm, hipStream_t stream);
// K18: the sampler's update of one step on cells * C elements, one pass over img.  The rule, field by field, is written once, at
// k5_euler_step_args in include/k5.h; K5EulerStepArgs is that struct (w = 1, C = 1, scale = 1, the rest zero) plus what only the engine sets:
// dtvec / signext / step — the captured step reads dt (and, when signext is given, sigma_next) at the device step counter — scalevec / coefvec
// (both or neither, with step) — it reads scale and noise_coef there and draws from stream stream_id + *step — and the stream.
// K5_ERR_ARG, nothing launched: what k5_euler_step_args lists, and dtvec without step or step without dtvec, signext without dtvec,
// scalevec / coefvec one without the other, without step or without stochastic.
struct K5EulerStepArgs : k5_euler_step_args {
  const float* dtvec = nullptr; const float* signext = nullptr; const int* step = nullptr;
  const float* scalevec = nullptr; const float* coefvec = nullptr;
  hipStream_t stream = nullptr;
  K5EulerStepArgs() : k5_euler_step_args{} { w = 1.f; C = 1; scale = 1.f; }
  K5EulerStepArgs(const k5_euler_step_args& pub, hipStream_t s) : k5_euler_step_args(pub), stream(s) {}
};
int k5_launch_euler_step(const K5EulerStepArgs& a);
// FlowEdit's pass of one step (finish step i, prepare step i + 1) on cells * C elements; the rule is written once, at k5_flowedit_step_args in
// include/k5.h.  k5_flowedit_step_refusal names what the launcher refuses (nullptr: nothing); K5_ERR_ARG, nothing launched.
const char* k5_flowedit_step_refusal(const k5_flowedit_step_args& a);
int k5_launch_flowedit_step(const k5_flowedit_step_args& a, hipStream_t stream);
// Philox4x32-10 raw words: out [nblk][4] of blocks blk0 .. blk0 + nblk - 1 (mod 2^64) under key = seed and counter words 2 / 3 = c2 / c3
int k5_launch_philox_words(uint32_t* out, uint64_t blk0, int64_t nblk, uint64_t seed, uint32_t c2, uint32_t c3, hipStream_t stream);
// out[g] = normal g & 3 of Philox block g >> 2 (counter (blk lo, blk hi, stream_id, 0), key = seed; Box-Muller in fp32), any n >= 1
int k5_launch_noise_normal(float* out, int64_t n, uint64_t seed, uint32_t stream_id, hipStream_t stream);
// editing: out = rn(rn((1 - sigma) * source) + rn(sigma * noise)), nothing contracted
int k5_launch_edit_renoise(float* out, const float* source, const float* noise, float sigma, int64_t n, hipStream_t stream);
// guidance coefficients of one sample: the five float64 sums Sc, Su, Scc, Suu, Scu of the bf16 velocities v_cond / v_uncond [n] in a fixed order
// (no atomics: the same bits on every launch, rank and handle) into sums[5], then ab = {alpha, beta} (fp32) of v = alpha c + beta u:
// s = zero_star ? Scu / (Suu + 1e-8) : 1, alpha = w, beta = s (1 - w), both times rescale * sqrt(var c / var v) + 1 - rescale when rescale > 0.
// part: k5_guidance_blocks(n) x 5 doubles of scratch.  wvec / step: the captured step reads w at the device step counter.
// K5_ERR_ARG: a NULL or not 16-byte aligned pointer, n < 1, rescale outside [0, 1]; K5_ERR_ALIGN: n % 8.  Nothing is launched when it refuses.
int k5_guidance_blocks(int64_t n);
int k5_launch_guidance_coeffs(const void* v_cond, const void* v_uncond, int64_t n, float w, int zero_star, float rescale, double* part,
                              double* sums, float* ab, hipStream_t stream, const float* wvec = nullptr, const int* step = nullptr);
// One axis of a tile plan on the HOST: n windows of F at starts[] over 0 .. total - 1.  nullptr when the starts ascend, every window lies inside
// and every coordinate is covered; otherwise what is wrong, in words (a thread-local buffer).
const char* k5_tile_axis_refusal(const char* axis, int n, const int32_t* starts, int F, int total);
// K18 over a 3-D plan of context windows (tiles): img fp32 (T,H,W,C); v_cond / v_uncond (null = no guidance) bf16 [nwin][Ft][Fh][Fw][C]; the
// plan's tables on the device.  The rule is written once, at k5_cfg_euler_tiles in include/k5.h.  The only windowed update: a temporal plan
// is the plan with one row window and one column window of weight 1.0 (k5_cfg_euler_windows).  A lane owns four channels of a cell when
// C % 4 == 0 and img is 16-byte, the velocities 8-byte aligned; otherwise one.  A cell without a window stays as it is; only slots inside a
// window's box are read.  K5_ERR_ARG, nothing launched: a null pointer, a count or extent < 1, nt * ny * nx > 64, T * H or W * C beyond an int.
int k5_launch_cfg_euler_tiles(float* img, const void* v_cond, const void* v_uncond, float w, float dt, const k5_tile_plan& plan, int T, int H,
                              int W, int C, hipStream_t stream);
// sampler preview: with v combined as in K18, x0 = x - sigma_next * v (fp32, uncontracted; keep_blend(x0, source, m) under a keep mask) on cells * C
// elements, optionally stored as fp32 (x0_out), and rgb[cell][j] = sat_u8(rint((b[j] + sum_k W[k][j] x0[k]) * 127.5 + 127.5)), NaN -> 0, with
// W [C][3] / b [3] (null = zeros) fp32 on the device.  rgb and rgb_w come together or not at all; one of rgb / x0_out is needed.  C % 4 == 0 and
// C <= 64, otherwise K5_ERR_UNSUPPORTED; x, x0_out and source 16-byte aligned, the velocities 8-byte.  Nothing is launched when it refuses.
int k5_launch_x0_preview(const float* x, const void* v_cond, const void* v_uncond, float w, float sigma_next, const float* source,
                         const float* keep_mask, const float* rgb_w, const float* rgb_b, float* x0_out, uint8_t* rgb, int64_t cells, int C,
                         hipStream_t stream);
// normalized attention guidance on two cross-attention outputs of the same queries, bf16 [rows][ld] (D columns used): per row d = zp - zn,
// g = fma(s - 1, d, zp), f = sum|g| <= tau * sum|zp| ? 1 : tau * sum|zp| / sum|g|, out = bf16(zp + alpha * (f * g - zp)), fp32, one pass, out may be
// z_pos.  D % 8 == 0, ld >= D, ld % 8 == 0, 16-byte pointers, s >= 1, tau >= 1, 0 <= alpha <= 1 (K5_ERR_ARG); D <= 2048 (K5_ERR_UNSUPPORTED).
// Nothing is launched when it refuses.
int k5_launch_nag_combine(const void* z_pos, const void* z_neg, void* out, int rows, int D, int ld, float s, float tau, float alpha,
                          hipStream_t stream);
// regional prompts, the (R+1)-way weighted combine of cross-attention outputs of the same queries: z0 [rows][ld] bf16 (D columns used), region r
// at zr + r * zr_stride elements, w fp32 [rows][ldw] (column 0 the base stream's weight); per element acc = w z for the first non-zero weight,
// fmaf(w, z, acc) for every later one, ascending, out = bf16(acc); a zero-weight stream is not read.  out may be z0.  1 <= R <= 8, ldw >= R + 1,
// D % 8 == 0, ld >= D, ld % 8 == 0, zr_stride % 8 == 0, 16-byte pointers (w 4-byte) (K5_ERR_ARG); D <= 2048 (K5_ERR_UNSUPPORTED).  Nothing is
// launched when it refuses.
int k5_launch_region_combine(const void* z0, const void* zr, long long zr_stride, int R, const float* w, int ldw, void* out, int rows, int D,
                             int ld, hipStream_t stream);
// regional prompts, cell masks [R][T][H][W] fp32 -> token weights w [N][R + 1] fp32, row i = token perm[i] (perm NULL: i) of the row-major
// (T / pt, H / ph, W / pw) grid: m_r = mean of the token's cells (clamped to [0, 1]), raw_0 = base_weight + max(0, 1 - sum m), w = raw / sum raw
int k5_launch_region_weights(const float* masks, int R, int T, int H, int W, int pt, int ph, int pw, float base_weight, const int32_t* perm,
                             float* w, hipStream_t stream);
// Enhance-A-Video (enhance.hip; the rule is written at k5_enhance_scores_bf16 in include/k5.h): the cross-frame attention score of one forward
// and block from q | k after norm_qk + RoPE — one workgroup per spatial position, one wave per head, K·Qᵀ on the 32x32x16 MFMA, then a
// one-workgroup float64 reduction of part [k5_enhance_parts(Hh, S)] in fixed order into score_out[0].  No atomics: equal inputs, equal bits.
// K5_ERR_ARG: a NULL or misaligned pointer (Q, K 16 bytes), ld < 64 Hh or ld % 8, Hh / S < 1, T < 2, weight negative or not finite,
// qk_scale <= 0 or not finite; K5_ERR_UNSUPPORTED: T > 64.  Nothing is launched when it refuses.
long long k5_enhance_parts(int Hh, int S);
int k5_launch_enhance_scores(const void* Q, const void* K, int ldq, int ldk, int Hh, int T, int S, const int32_t* frame_rows, float qk_scale,
                             float weight, double* part, float* score_out, hipStream_t stream);
// x [rows][ld] bf16 (D columns used) *= *score_dev in place: bf16(float(x) * s), 16 bytes per lane, grid-stride; a workgroup that reads s == 1
// touches nothing.  Refusals as k5_launch_nag_combine's (without its D limit).
int k5_launch_scale_by_dev(void* x, int rows, int D, int ld, const float* score_dev, hipStream_t stream);
// The forecast cache's two passes (forecast.hip; the rule is written at k5_forecast_update_bf16 in include/k5.h).  vis bf16 [rows][ld] (D columns
// used), ori / F0 bf16 and D1 / D2 fp32 [rows][D]; 16 bytes per lane, grid-stride, no atomics.
// update: F0 = bf16(vis - ori) and, with level = min(order, have), level >= 1: D1 = (F0' - F0) / g, level >= 2: D2 = (D1' - D1) / g, in place;
// vis and ori are only read and alias nothing.  apply: vis = bf16(vis + F0 + k D1 + c2 D2) with m = min(order, have - 1) terms and
// c2 = k (k + g) g / (g + gp), g and gp the slot's last two gaps between full calls (read at m = 2 only).
// K5_ERR_ARG before any launch: a NULL or not 16-byte aligned pointer among those the level / m reads or writes (the others may be NULL),
// rows < 1, D % 8, ld < D, ld % 8, order outside 0..2, g < 1 (apply: g or gp < 1 at m = 2), k < 1, have < 0 (update) or < 1 (apply).
int k5_launch_forecast_update(const void* vis, int ld, const void* ori, void* F0, float* D1, float* D2, int rows, int D, int g, int order, int have,
                              hipStream_t stream);
int k5_launch_forecast_apply(void* vis, int ld, const void* F0, const float* D1, const float* D2, int rows, int D, int k, int g, int gp, int order,
                             int have, hipStream_t stream);
// fp32 -> bf16 cast, bf16 -> fp32
int k5_launch_cast_f32_bf16(const float* x, void* out, int64_t n, hipStream_t stream);
// weight packing: src [rows][cols] (K5_F32 / K5_BF16 / K5_F16, device) -> dst [rows][ld] bf16 (RNE) or fp32, pad columns zeroed
int k5_launch_pack_matrix(const void* src, int src_dtype, void* dst, int dst_bf16, int64_t rows, int cols, int ld, hipStream_t stream);
// LoRA merge in place: W[n][k] = W[n][k] + scale * sum_r B[n][r] A[r][k] on a packed [rows][ld] matrix (K5_BF16 or
// K5_F32), columns cols .. ld - 1 neither read nor written.  A [R][cols], B [rows][R] (K5_F32 / K5_BF16 / K5_F16, device), 1 <= R <= 256.  float64 fma
// chain over r = 0 .. R - 1, then fma(scale, acc, W), rounded to fp32 and from there to W's type: the bits do not depend on the tiling.  scale == 0 launches nothing.
int k5_launch_lora_merge(void* W, int w_dtype, int rows, int cols, int ld, const void* A, int a_dtype, const void* B, int b_dtype, int R,
                         float scale, hipStream_t stream);

// causal_hw > 0: frame-causal scores, tiles wholly at columns >= (row / causal_hw + 1) * causal_hw are skipped (left unwritten)
int k5_launch_gemm_bf16_f32out(const void* A, const void* W, float* C, int M, int N, int K, int lda, int ldw, int ldc,
                               float alpha, int causal_hw, hipStream_t stream);

// ---- VAE decoder kernels (channels-last bf16 activations) ----
// 4-wave 256-row variant (conv3d_w4.hip); K5_ERR_UNSUPPORTED outside its range (Cin % 128, Cout = 128 or % 256, >= one round of tiles)
// quad_stats (nullable): [2 ceil(M / 256)][Cout / 4][2] fp32 partial GroupNorm sums of the stored outputs (see conv3d_w4.hip)
int k5_launch_conv3d_w4(const void* X, const void* W, const float* bias, void* out, int Ts, int Hs, int Ws, int Cin, int Cout,
                        int up_t, int up_s, int ldc, const void* resid, int ldr, float* quad_stats, hipStream_t stream);
int k5_launch_conv3d_bf16(const void* X, const void* W, const float* bias, void* out, int Ts, int Hs, int Ws, int Cin,
                          int Cout, int up_t, int up_s, int ldc, const void* resid, int ldr, hipStream_t stream);
int k5_launch_conv3d_bf16_strided(const void* X, const void* W, const float* bias, void* out, int Ts, int Hs, int Ws, int Cin,
                                  int Cout, int up_t, int up_s, int st_t, int st_s, int ldc, const void* resid, int ldr, hipStream_t stream);
// which kernel the LAST conv launcher call of this host thread took (diagnostics: the VAE engine counts them per handle so that a
// parity test can assert the production kernels ran, tests/test_gpu_vae.py)
enum { K5_CONV_KIND_TILE128 = 0, K5_CONV_KIND_W4 = 1, K5_CONV_KIND_W4_STATS = 2, K5_CONV_KIND_OUT3 = 3 };
int k5_conv3d_last_kind();
void k5_conv3d_set_last_kind(int kind);
size_t k5_groupnorm_workspace_bytes(int M, int G);
int k5_launch_groupnorm_bf16(const void* x, const float* gamma, const float* beta, void* out, int M, int C, int G, float eps,
                             int silu, int ldx, int ldo, void* workspace, hipStream_t s);
// GroupNorm whose statistics were emitted by the producing conv: quad_stats [nblk][C / 4][2] (k5_launch_conv3d_w4); stats_ws: 2 G floats
int k5_launch_groupnorm_bf16_quads(const void* x, const float* gamma, const float* beta, void* out, int M, int C, int G, float eps,
                                   int silu, int ldx, int ldo, const float* quad_stats, int nblk, float* stats_ws, hipStream_t s);
int k5_launch_causal_softmax(const float* scores, void* P, int S, int hw, int lds, int ldp, hipStream_t s);
// the mid block's attention in one kernel for C = 512 (vae_attn.hip): q, k [S][ldqk], vt [512][ldvt >= ceil(S/32)*32], o [S][ldo]
int k5_launch_vae_attention512(const void* q, const void* k, const void* vt, void* o, int S, int hw, int ldqk, int ldvt, int ldo,
                               float scale, hipStream_t stream);
int k5_launch_nchw_to_mc(const float* z, void* out, int C, int64_t M, int Cpad, hipStream_t s, int64_t cstride = 0);   // cstride: elements between the channels of z (0 = M)
int k5_launch_blend_place_bf16(const void* a, int64_t a_stride, int len_a, const void* b, int64_t b_stride, int len_b, void* dst, int64_t dst_stride,
                               int64_t outer, int64_t inner, int extent, int keep, hipStream_t s);
int k5_launch_frames_to_uint8(const void* x, void* out, int64_t n, hipStream_t s);
int k5_launch_mc_to_nchw(const void* x, void* out, int C, int64_t M, int ldx, hipStream_t s);
int k5_launch_blend_bf16(const void* a, void* b, int64_t outer, int len_a, int len_b, int64_t inner, int extent, hipStream_t s);
