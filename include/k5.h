/* k5.h — C ABI of libk5.so, the MI355X (gfx950) denoising engine for Kandinsky-5 T2V Lite.
 *
 * The reference (ai-forever/Kandinsky-5) is pure Python/PyTorch and has NO FFI/plugin layer
 * (SURVEY.md §8b); its seams are Python call signatures.  Each entry point below therefore
 * cites the reference *Python interface* it stands behind (paths relative to the reference
 * repo).  The Python host mirror (kandinsky-5_amd/kandinsky/) binds these with ctypes and keeps
 * the reference's names/arguments/errors; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  `stream` is a hipStream_t passed as void*
 *     (NULL = the null stream).  All device work is enqueued asynchronously on that stream.
 *   - device pointers are BORROWED from the caller (torch owns activations); the engine OWNS its
 *     packed weights and workspaces (hipMalloc).
 *   - every function returns a k5_status; k5_last_error() gives a thread-local message.
 *   - a handle is not thread-safe; one handle per GPU per process (one process per GPU).
 *   - bf16 tensors are row-major with explicit leading dimensions in ELEMENTS.
 */
#ifndef K5_H
#define K5_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  K5_OK = 0, K5_ERR_ARG = 1, K5_ERR_ALIGN = 2, K5_ERR_HIP = 3, K5_ERR_STATE = 4, K5_ERR_KEY = 5,
  K5_ERR_UNSUPPORTED = 6
} k5_status;
typedef enum { K5_F32 = 0, K5_BF16 = 1, K5_F16 = 2 } k5_dtype;
typedef enum { K5_EPI_BIAS = 0, K5_EPI_BIAS_M = 1, K5_EPI_GELU = 2, K5_EPI_GATE = 3, K5_EPI_F32 = 4 /* internal */ } k5_epilogue;

/* bumped whenever an entry point is added or changes meaning; the host binding checks it BEFORE binding symbols, so that a stale
 * libk5.so fails with a clear message instead of a missing-symbol lookup (round 3: 4).  The MagCache calibration exports (k5_magcache_stats_bf16,
 * k5_dit_set_magcache_calibrate, k5_dit_magcache_calibration) were ADDED under 11: tests/test_gpu_vae.py pins the number 11, and nothing that existed
 * changed meaning.  The host binding names the missing symbol and the rebuild command when it meets a libk5.so from before them. */
#define K5_ABI_VERSION 11
int k5_abi_version(void);
const char* k5_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Kernel-level entry points (used by the parity tests and by torch-side glue).
 * ---------------------------------------------------------------------------------------- */

/* C[M][N] = A[M][K] . W[N][K]^T (+bias) with fused epilogue; bf16 in/out, fp32 accumulate.
 * Replaces autocast nn.Linear: kandinsky/models/nn.py:180-191 (get_qkv), :204-206 (out_l),
 * :352-361 (FeedForward incl. nn.GELU), :71 (TextEmbeddings), :96 (VisualEmbeddings), :382 (OutLayer);
 * K5_EPI_GATE additionally fuses apply_gate_sum nn.py:30-33: C = bf16(resid + gate[n]*bf16(acc+bias)).
 * K5_EPI_BIAS_M adds bias[m] (used to emit V^T = W_v . X^T directly). bias/gate are fp32.
 * Operand footprint: when K is a multiple of 128 and >= 256, M >= 512, N >= 128, N and ldc multiples of 8 (the four-wave kernel and its quadrant tail
 * may take the call), up to 143 rows PAST the last row of A (M not a multiple of the 256- / 192- / 128-row tile) and of W (N not a multiple of 256) are
 * read: 143 * lda resp. 143 * ldw elements beyond row M - 1 resp. N - 1.  Their values are never used (they feed outputs that are not stored), but they
 * must be MAPPED memory: keep the operand inside an allocation with that slack.  Every other shape reads rows 0 .. M - 1 / N - 1 only.
 * The padding columns K .. lda - 1 / ldw - 1 and C's columns N .. ldc - 1 and rows >= M are never read or written. */
int k5_gemm_bf16(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int lda,
                 int ldw, int ldc, int epilogue, const void* resid, int ldr, const float* gate, void* stream);
/* The same GEMM on a NAMED kernel (tests and A/B tools; k5_gemm_bf16 picks by shape and cost): kernel 0 = as k5_gemm_bf16, 2 = 128 x 128 tiles,
 * 4 = the four-wave persistent kernel, 8 = the eight-wave ping-pong kernel (a kernel whose shape conditions do not hold falls through to the
 * next one, as in the automatic choice); any other kernel id is K5_ERR_ARG (ABI 9: kernel 5 is gone).  token_tile 0 = by cost, 128 / 192 / 256
 * = rows of the four-wave kernel's workgroup tile (ABI 7).  Every kernel sums a K column in the same order: results are bit-identical across them. */
int k5_gemm_bf16_variant(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int lda, int ldw, int ldc,
                         int epilogue, const void* resid, int ldr, const float* gate, void* stream, int kernel, int token_tile);

/* S_f32[M][N] = alpha * A[M][K] . W[N][K]^T — the fp32 attention scores of the VAE mid block (diffusers Attention called from
 * HunyuanVideoMidBlock3D, kandinsky/models/vae.py:341-362, with prepare_causal_attention_mask vae.py:110-122).  causal_hw > 0:
 * row i is only ever read at columns < (i / causal_hw + 1) * causal_hw (its own and earlier frames); output tiles wholly beyond
 * that limit are not computed and left unwritten.  C is fp32 [M][ldc].  Operand footprint as k5_gemm_bf16: with K a multiple of 128 and >= 256, M >= 512,
 * N >= 256, N and ldc multiples of 4 and at least 256 kept 256 x 256 tiles, up to 143 rows past the last row of A and of W are read and must be mapped. */
int k5_gemm_bf16_f32out(const void* A, const void* W, float* C, int M, int N, int K, int lda, int ldw, int ldc,
                        float alpha, int causal_hw, void* stream);

/* P_bf16[i][j] = softmax_j(scores[i][j]) over the frame-causal columns j < (i / hw + 1) * hw, 0 elsewhere (j < ldp) — the masked
 * softmax of the same mid-block attention (mask: prepare_causal_attention_mask, vae.py:110-122).  scores fp32 [S][lds]. */
int k5_causal_softmax_bf16(const float* scores, void* P, int S, int hw, int lds, int ldp, void* stream);
/* The whole mid-block attention in one kernel for C = 512 (one head; the scores are never materialised):
 * O[i] = softmax_j<lim(i) (scale * q_i . k_j) V[j], lim(i) = (i / hw + 1) * hw — diffusers `Attention` + the frame-causal mask,
 * kandinsky/models/vae.py:110-122,341-362.  q, k: [S][ldqk] bf16 (512 columns each; k may be q + 512 of one [S][1024] buffer),
 * vt: V transposed [512][ldvt] bf16 with ldvt >= ceil(S / 32) * 32 (columns S .. ldvt must hold FINITE values — they are multiplied
 * by a probability of exactly 0; the engine zero-fills them), o: [S][ldo]. */
int k5_vae_attention512_bf16(const void* q, const void* k, const void* vt, void* o, int S, int hw, int ldqk, int ldvt, int ldo,
                             float scale, void* stream);

/* O[q][h*64+d] = softmax(Q K^T / 8) V per head (head_dim 64, non-causal, fp32 softmax).
 * Replaces FA(q,k,v): nn.py:201 (text self-attn), :254 (visual self-attn), :336 (cross-attn).
 * Q [q_len][ldq], K [kv_len][ldk] with head h at columns h*64..; Vt [H*64][ldvt] is V transposed
 * (row h*64+d, column key). */
int k5_attention_bf16(const void* Q, const void* K, const void* Vt, void* O, int H, int q_len, int kv_len,
                      int ldq, int ldk, int ldvt, int ldo, void* stream);

/* Split-key form of the dense attention (sequence-parallel overlap): process 64-key tiles e -> e + tile_off0
 * (+ tile_skip_n once the index reaches tile_skip_at) for e < tile_cnt (-1: to the last tile); flags & 1 resumes from
 * `state` (fp32 accumulators of an earlier call over other tiles), flags & 2 writes `state` instead of O.
 * state: k5_attention_state_size(H, q_len) bytes.  Two calls covering disjoint tile sets == one k5_attention_bf16 call. */
int64_t k5_attention_state_size(int H, int q_len);
int k5_attention_bf16_range(const void* Q, const void* K, const void* Vt, void* O, int H, int q_len, int kv_len,
                            int ldq, int ldk, int ldvt, int ldo, float score_bound, int tile_off0, int tile_cnt,
                            int tile_skip_at, int tile_skip_n, void* state, int flags, void* stream);
/* The same attention with the keys ALREADY multiplied by the softmax scale in the exp2 domain: Kc = bf16(log2(e)/8 * k)
 * (one rounding, done by the producer: the engine's rmsnorm/RoPE kernel).  The scores are then the exp2 arguments: no
 * per-score multiply-add.  Whole key tiles only (kv_len % 64 == 0: no ragged-tile masking; K5_ERR_ARG otherwise).
 * Softmax form: with score_bound > 0 and score_bound * log2(e)/8 <= 90 (score_bound bounds |q.k| in RAW units) the
 * constant offset 0 (exp2 can neither overflow nor flush a row); otherwise the lazy online max (the running offset rides
 * in the MFMA accumulator's initial value and is only revised when a tile's maximum leaves a 2^60 window). */
int k5_attention_bf16_prescaled(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len,
                                int ldq, int ldk, int ldvt, int ldo, float score_bound, void* stream);
/* What the engine runs for FA(q,k,v) of the visual self-attention (nn.py:254): the form is chosen PER HEAD on the device.
 * k5_rmsnorm_rope_stats_bf16 (below) leaves max |q_h|^2 / max |k'_h|^2 over the rows; k5_attention_flags turns them into
 * head_flags[h] = 1 (|q|max |k'|max <= 90: fixed offset) or 0 (online max) and resets the statistics (kstat: nk partial
 * maxima at stride kstride floats — one per sequence-parallel rank).  k5_attention_bf16_prescaled_auto launches both forms
 * over the same grid; a workgroup exits at once unless its head is its form's.  head_flags NULL: variant 1 = online max
 * everywhere.  workspace: NULL or k5_attention_balance_size bytes (balanced launch). */
int k5_attention_flags(float* qstat, float* kstat, int nk, int kstride, int H, int force_online, int* head_flags, void* stream);
/* The same pair with PER-ROW softmax offsets (what the engine's single-GPU path runs): k5_attention_flags_rows also writes
 * kmax[h] = max |k'_h| and keeps heads up to |q|max |k'|max <= 190 on the fixed-offset form; there query row q of head h runs on
 * the constant offset max(0, |q| kmax[h] - 90) — exp2 cannot overflow whatever the data, and the result is exact unless the row's
 * whole sum underflows (< 2^-60: its largest score lies more than 150 below its Cauchy-Schwarz bound).  A workgroup that meets
 * such a row sets head_flags[h] = 0 and the online-max launch that follows in the same call redoes that head: head_flags is
 * read and written. */
int k5_attention_flags_rows(float* qstat, float* kstat, int nk, int kstride, int H, int force_online, int* head_flags, float* kmax,
                            void* stream);
int k5_attention_bf16_prescaled_rows(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                     int ldk, int ldvt, int ldo, int* head_flags, const float* kmax, void* workspace, void* stream);
/* CENTRED per-row offsets (round 3; what the engine's single-GPU path runs).  The plain offset |q| max|k'| - 90 is built from a bound the
 * scores may sit far below: keys of a head that share a large mean direction put EVERY score of a row near +-0.4 of that bound, and the
 * row sums underflow wholesale.  With a centre c_h (any convex combination of the head's keys; k5_rmsnorm_rope_centre_bf16 takes the mean
 * of a strided sample in the pass that writes the keys) and the radius R_h = max |k' - c_h|:  q.k' <= q.c + |q| R  and  max_j q.k'_j >= q.c,
 * so a row whose plain bound exceeds 90 runs with the offset q.c + |q| R - 90 — exp2 arguments <= 90 and a row sum >= 2^(90 - |q| R): no
 * underflow at all while |q| R <= 190.  Same softmax (any offset gives the same softmax); rows with a plain bound <= 90 keep offset 0.
 * k5_rmsnorm_rope_centre_bf16: as k5_rmsnorm_rope_stats_bf16, plus centre [H - scale_from_head][64] out and H - scale_from_head squared radii
 * appended to stats.  k5_attention_flags_rows_centred: rstat (consumed) -> krad; a head keeps the fixed form while min(|q|max kmax,
 * |q|max R) <= 190.  k5_attention_bf16_prescaled_rows_centred: k5_attention_bf16_prescaled_rows with the centred offsets. */
int k5_rmsnorm_rope_centre_bf16(void* x, const float* weight, const float* cos_tab, const float* sin_tab, int rows, int H, int ld,
                                int heads_per_weight, int rope_heads, float out_scale, int scale_from_head, float* stats, float* centre,
                                void* stream);
int k5_attention_flags_rows_centred(float* qstat, float* kstat, int nk, int kstride, int H, int force_online, int* head_flags, float* kmax,
                                    float* rstat, float* krad, void* stream);
int k5_attention_bf16_prescaled_rows_centred(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                             int ldk, int ldvt, int ldo, int* head_flags, const float* kmax, const float* centre,
                                             const float* krad, void* workspace, void* stream);
/* ANCHORED offsets for the heads BEYOND that window (ABI 5; the engine's one-GPU path, option "attn_anchor").  The Cauchy-Schwarz offsets
 * end where min(|q| kmax, |q| R) exceeds 190 and the online-max form (0.39-0.41 of peak instead of 0.52) used to take over.  Instead the offset
 * of a row is anchored at a score the row ACHIEVES: the maximum s over a sample of keys (the four 16-key tiles of the row's own 64-token
 * block and 28 tiles strided over the kv_len keys given), plus e = min(60, spread (s - sample mean)) — where the maximum over ALL
 * kv_total keys is expected when the scores scatter: spread = 1.4 (sqrt(2 ln kv_total) - c) / c, c = sqrt(2 ln 512): 0.44 at 47 616 keys — rounded
 * up, + 20.  Dense attention: the row's true maximum is >= s, so its term is >= 2^-80 and the row sum cannot underflow whatever the
 * norms; the form is exact while the true maximum lies below s + e + 132.  (Dense attention only: under NABLA the largest KEPT score
 * may lie far below a sample of all keys — the engine leaves such heads on the online form there.)  Beyond that the row sum exceeds 2^112 (or is
 * inf / NaN): the job falls back to the online form exactly like an underflowing one, and below 2^112 the sum bounds every accumulator,
 * so nothing overflows unnoticed.
 * k5_attention_flags_rows_anchored: as _centred, but a head beyond the window keeps flag 1 and gets kmax[h] = -1 (the marker) unless
 * prefer_online[h] (nullable) is set.  k5_attention_row_anchor: anchor [H][q_len] for the marked heads (other rows untouched); key0 = the
 * index among the given keys of query row 0's token, kv_total >= kv_len (a rank of a sharded schedule samples its own keys).  k5_attention_bf16_prescaled_rows_anchored: _rows_centred reading the anchors of the marked heads. */
int k5_attention_flags_rows_anchored(float* qstat, float* kstat, int nk, int kstride, int H, int force_online, int* head_flags, float* kmax,
                                     float* rstat, float* krad, const int* prefer_online, void* stream);
int k5_attention_row_anchor(const void* Q, const void* Kc, int H, int q_len, int kv_len, int ldq, int ldk, int key0, int kv_total,
                            const float* kmax, float* anchor, void* stream);
int k5_attention_bf16_prescaled_rows_anchored(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                              int ldk, int ldvt, int ldo, int* head_flags, const float* kmax, const float* centre,
                                              const float* krad, const float* anchor, void* workspace, void* stream);
/* One pass of a multi-pass schedule (sequence parallelism: local keys first, gathered keys later) with per-row offsets: key tiles
 * [tile_off0, tile_off0 + tile_cnt), flags & 1 = resume `state`, & 2 = leave it instead of writing O (k5_attention_state_size
 * bytes).  late_pass 1 = not the last pass, 2 = the last: a row that underflows in any pass writes head_flags[h] = 2, every later
 * fixed-offset launch and the online launches of the non-final passes then skip the head, and the online launch of the last pass
 * recomputes it from scratch over all kv_len keys. */
int k5_attention_bf16_prescaled_rows_pass(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                          int ldk, int ldvt, int ldo, int* head_flags, const float* kmax, int tile_off0, int tile_cnt,
                                          float* state, int flags, int late_pass, void* workspace, void* stream);
/* The same pass with the reference's norm_qk + apply_rotary of the QUERIES (nn.py:193-197, 239-243) done inside the kernel's Q load:
 * Q holds the raw query projection, q_norm_w the 64 RMSNorm weights, q_cos / q_sin [q_len][32] fp32 the rotary table
 * (k5_rope_table).  There is no max|q|^2 statistic then: call k5_attention_flags_rows with a zero query statistic (every head
 * starts on the fixed form) and the fixed-offset workgroups decide per head — a row whose bound |q| max|k'| exceeds 190 sets
 * head_flags[h] = 0 and the online launch of the same call owns the head.  head_flags and kmax both null: online max everywhere.
 * tile_cnt -1 = all key tiles from tile_off0 (single pass: state null, flags 0, late_pass 0). */
int k5_attention_bf16_prescaled_qnorm_pass(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                           int ldk, int ldvt, int ldo, const float* q_norm_w, const float* q_cos, const float* q_sin,
                                           int* head_flags, const float* kmax, int tile_off0, int tile_cnt, float* state, int flags,
                                           int late_pass, void* workspace, void* stream);
int k5_attention_bf16_prescaled_auto(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len,
                                     int ldq, int ldk, int ldvt, int ldo, const int* head_flags, int variant, void* workspace,
                                     void* stream);
/* k5_attention_bf16[_bounded] with load balancing: the (head, 256-query) jobs that do not fill a whole round of the
 * device's resident workgroups are split 2-4 ways along the keys and merged (same result up to fp32 summation order).
 * workspace: k5_attention_balance_size(H, q_len) bytes.  The engine uses this for every large self-attention. */
int64_t k5_attention_balance_size(int H, int q_len);
int k5_attention_bf16_balanced(const void* Q, const void* K, const void* Vt, void* O, int H, int q_len, int kv_len,
                               int ldq, int ldk, int ldvt, int ldo, float score_bound, void* workspace, void* stream);

/* NABLA block-sparse attention = nablaT_v2 (kandinsky/models/utils.py:136-163, incl. the STA window of
 * fast_sta_nabla :108-133) + flex_attention(q,k,v,block_mask) (nn.py:257-280), tokens in fractal order
 * (utils.py:31-41): N = T*Hb*Wb*64.  k5_nabla_select_bf16 fills `workspace` (k5_nabla_workspace_size bytes) with the
 * block map of every (head, 64-query block); k5_attention_nabla_bf16 consumes it; k5_nabla_mask_u8 expands the map to
 * uint8 [H][N/64][N/64] (tests / diagnostics); k5_dit_nabla_block_counts reports an engine's kept-block totals.
 * P >= 1 keeps every block, as the reference's `cvals >= 1 - thr` does. */
int64_t k5_nabla_workspace_size(int H, int num_blocks);
int k5_nabla_select_bf16(const void* q, const void* k, int ldq, int ldk, int H, int N, int T, int Hb, int Wb, int wT,
                         int wH, int wW, float P, void* workspace, void* stream);
int k5_attention_nabla_bf16(const void* Q, const void* K, const void* Vt, void* O, int H, int N, int ldq, int ldk,
                            int ldvt, int ldo, float score_bound, const void* workspace, void* stream);
int k5_nabla_mask_u8(const void* workspace, int H, int num_blocks, void* out_u8, void* stream);
/* Sequence-parallel form (SURVEY.md §8e "NABLA under SP"): this rank holds the query rows of global blocks
 * [q_block0, q_block0 + Nq/64) and, after the K / V^T all-gather, all N keys; V^T optionally in per-rank chunks
 * [chunk][H*64][vt_chunk_keys] (vt_chunk_keys = 0: plain [H*64][ldvt]).  Map rows are indexed by the LOCAL query block;
 * the workspace is sized by k5_nabla_workspace_size(H, N/64) as above.  Row i of the map equals row q_block0 + i of the
 * square map. mask: uint8 [H][Nq/64][N/64].
 * COUPLING (since the round-5 workspace layout): the key-tile lists sit BEHIND the logits of the Nq/64 selected rows, so their
 * offset depends on Nq.  The attention / mask / count calls that follow a select on a workspace must be given the SAME Nq (and H, N)
 * as that select — k5_nabla_select_bf16 counts as Nq = N; nothing in the workspace records it, a different Nq reads another region
 * without an error. */
int k5_nabla_select_rect_bf16(const void* q, const void* k, int ldq, int ldk, int H, int Nq, int q_block0, int N, int T,
                              int Hb, int Wb, int wT, int wH, int wW, float P, void* workspace, void* stream);
int k5_attention_nabla_rect_bf16(const void* Q, const void* K, const void* Vt, void* O, int H, int Nq, int N, int ldq,
                                 int ldk, int ldvt, int ldo, float score_bound, const void* workspace, int vt_chunk_keys,
                                 int64_t vt_chunk_stride, void* stream);
/* Sequence-parallel NABLA as the engine runs it.  k5_nabla_select_rect_local_bf16: k5_nabla_select_rect_bf16 with the key blocks
 * [local_block0, + local_blocks) — the rank's own, in place before the gather — leading every (head, 256-query group) list.
 * k5_attention_nabla_rect_prescaled_pass: the list-driven attention on keys pre-multiplied by log2(e)/8, per-head flags and per-row
 * offsets as in k5_attention_bf16_prescaled_rows; pass 0 = the whole lists in one launch group; 1 = only the leading local entries,
 * leaving the fp32 state (k5_attention_state_size bytes) and no output; 2 = the remaining entries, resuming the state, writing O.
 * A row that underflows on its per-row offset in pass 1 sets head_flags[h] = 2 and the online launch of pass 2 recomputes the head
 * over its whole lists.  Replaces nablaT_v2 + flex_attention (kandinsky/models/utils.py:136-163, nn.py:257-280) on a token shard. */
int k5_nabla_select_rect_local_bf16(const void* q, const void* k, int ldq, int ldk, int H, int Nq, int q_block0, int N, int T, int Hb,
                                    int Wb, int wT, int wH, int wW, float P, void* workspace, int local_block0, int local_blocks,
                                    void* stream);
int k5_attention_nabla_rect_prescaled_pass(const void* Q, const void* Kc, const void* Vt, void* O, int H, int Nq, int N, int ldq, int ldk,
                                           int ldvt, int ldo, const void* workspace, int vt_chunk_keys, int64_t vt_chunk_stride,
                                           int* head_flags, const float* kmax, int pass, float* state, void* stream);
int k5_nabla_mask_rect_u8(const void* workspace, int H, int q_blocks, int num_blocks, void* out_u8, void* stream);

/* Dense k5_attention_bf16 with a caller-proved bound |q.k| <= score_bound for every (query, key) pair
 * (after norm_qk nn.py:193-197 every head vector has |x| <= 8*max|weight|).  When bound*log2(e)/8 <= 90 the
 * softmax runs with the constant offset 0 instead of the online running max (same softmax, fewer VALU ops);
 * otherwise, or with score_bound <= 0, the online-max kernel runs. */
int k5_attention_bf16_bounded(const void* Q, const void* K, const void* Vt, void* O, int H, int q_len,
                              int kv_len, int ldq, int ldk, int ldvt, int ldo, float score_bound, void* stream);

/* apply_scale_shift_norm nn.py:25-28: out = bf16(LayerNorm(x, eps 1e-5, no affine)*(scale+1)+shift). */
int k5_ln_modulate_bf16(const void* x, const float* scale, const float* shift, void* out, int rows, int D,
                        int ldx, int ldo, void* stream);
/* norm_qk nn.py:193-197 + apply_rotary nn.py:35-40, in place on [rows][ld] holding H heads of 64:
 * RMSNorm(eps=2^-23, weight[(h/heads_per_weight)*64..]) -> bf16 -> adjacent-pair rotation by
 * cos/sin[rows][32] (heads < rope_heads; cos==NULL: no rotation) -> bf16. */
int k5_rmsnorm_rope_bf16(void* x, const float* weight, const float* cos_tab, const float* sin_tab, int rows,
                         int H, int ld, int heads_per_weight, int rope_heads, void* stream);
/* The engine's form of the same op: heads >= scale_from_head are multiplied by out_scale before their (single) bf16
 * rounding (keys for the pre-scaled attention), and stats[h] (device fp32 [H], zero before the first use) receives
 * max(stats[h], |x_row,h|^2) over the rows, of the bf16 values written. */
int k5_rmsnorm_rope_stats_bf16(void* x, const float* weight, const float* cos_tab, const float* sin_tab, int rows, int H,
                               int ld, int heads_per_weight, int rope_heads, float out_scale, int scale_from_head,
                               float* stats, void* stream);
/* apply_gate_sum nn.py:30-33 (standalone form). */
int k5_gate_sum_bf16(const void* x, const void* y, const float* gate, void* out, int rows, int D, void* stream);
/* MagCache calibration pass (standalone form): res = bf16(vis - ori), the bits of k5_gate_sum_bf16 with a gate of -1; res may alias ori.
 * With prev != NULL (n x D bf16, aliasing nothing): sums[0..3] (device, float64) = sum rho_i, sum rho_i^2, sum (1 - cos(res_i, prev_i)) and the
 * number of rows counted, rho_i = |res_i| / |prev_i|, over the rows where both norms are non-zero.  Row sums are fp32 over the stored bf16
 * values, the sum over rows is float64 in a fixed order (repeatable bits).  prev == NULL: only res is written, sums[] = 0.  D % 8 == 0. */
int k5_magcache_stats_bf16(const void* vis, const void* ori, const void* prev, void* res, double* sums, int rows, int D, void* stream);
/* fp32-island GEMV (Modulation nn.py:161-164, TimeEmbeddings nn.py:56-61): y = W.act(x) + b (+add). */
int k5_gemv_f32(const float* x, const float* W, const float* b, float* y, int N, int K, int silu_in,
                const float* add, void* stream);
/* TimeEmbeddings sinusoid nn.py:57-58; t = 1000*sigma by value. */
int k5_time_features_f32(float t, float* out, int D, void* stream);
/* TextEmbeddings.norm nn.py:67,72 (LayerNorm affine on bf16 rows, bf16 and/or bf16-rounded fp32 out). */
int k5_ln_affine_bf16(const void* x, const float* w, const float* b, void* out_bf16, float* out_f32, int rows,
                      int D, void* stream);
/* RoPE3D/RoPE1D nn.py:99-150 cos/sin tables [T*H*W][32]: n0 | n1 | n2 columns for the three axes, n0 + n1 + n2 = 32 (the rotation
 * pairs of a 64-wide head; an axis of width 0 needs no positions: the 1-D table is 32 | 0 | 0 with H = W = 1); positions are device
 * int32.  K5_ERR_ARG for an extent < 1, widths that do not add up to 32, a NULL table or a NULL position vector of a used axis. */
int k5_rope_table_f32(float* cos_tab, float* sin_tab, const int32_t* pos_t, const int32_t* pos_h,
                      const int32_t* pos_w, int T, int H, int W, int n0, int n1, int n2, float s0, float s1,
                      float s2, const int32_t* tok_perm, void* stream);
/* VisualEmbeddings patchify nn.py:81-95 (patch (1,2,2)), fp32 (T,H,W,x_channels) -> bf16 [Ntok][Kpad];
 * channels in [x_channels, Cin_total) read as zero (generation_utils.py:107-112); tok_perm = fractal order. */
int k5_patchify_bf16(const float* x, void* out, int T, int H, int W, int x_channels, int Cin_total, int Kpad,
                     const int32_t* tok_perm, void* stream);
/* k5_patchify_bf16 of torch.cat([x, vcond], -1) read from the two sources: x fp32 (T,H,W,x_channels), vcond fp32
 * (T,H,W,Cin_total-x_channels), 0 < x_channels < Cin_total; bit-identical output. */
int k5_patchify_cond_bf16(const float* x, const float* vcond, void* out, int T, int H, int W, int x_channels, int Cin_total,
                          int Kpad, const int32_t* tok_perm, void* stream);
/* k5_patchify_bf16 / k5_patchify_cond_bf16 of a strided view (added under ABI 11, as the exports further down were): the (T,H,W) box of a
 * larger tensor, x with frame stride x_frame_stride and row stride x_row_stride (in elements; the cells of a row are x_channels apart), vcond
 * (NULL = k5_patchify_bf16's zero channels) likewise with cells Cin_total - x_channels apart.  With compact strides it equals the two entries
 * above bit for bit; on a view it equals them on a contiguous copy of the view.  Nothing outside the box is read.  K5_ERR_ARG, nothing
 * launched: a NULL x or out, an extent < 1, odd H or W, a row stride below W cells or a frame stride below H rows. */
int k5_patchify_view_bf16(const float* x, int64_t x_frame_stride, int64_t x_row_stride, const float* vcond, int64_t vc_frame_stride,
                          int64_t vc_row_stride, void* out, int T, int H, int W, int x_channels, int Cin_total, int Kpad,
                          const int32_t* tok_perm, void* stream);
/* OutLayer un-patchify nn.py:384-399: [Ntok][4C] (c,ph,pw) -> (T,2Hp,2Wp,C) bf16. */
int k5_unpatchify_bf16(const void* x, void* out, int T, int Hp, int Wp, int C, int ldx,
                       const int32_t* tok_perm, void* stream);
/* CFG combine + Euler, generation_utils.py:74-76,128.  v_uncond NULL => no guidance.  A fixed form of k5_euler_step (the rule is written at
 * k5_euler_step_args): img, v_cond, v_uncond, w, dt with cells = n, C = 1.  A NULL img or v_cond, or n < 1, is K5_ERR_ARG and nothing is launched. */
int k5_cfg_euler(float* img, const void* v_cond, const void* v_uncond, float w, float dt, int64_t n,
                 void* stream);
/* Editing kernels (added under ABI 11, as the LoRA and MagCache calibration exports were).  Flow matching: x_sigma = (1 - sigma) x0 + sigma eps.
 * k5_edit_renoise: out[i] = rn(rn(a * source[i]) + rn(sigma * noise[i])), a = fp32(1 - sigma), every operation rounded to fp32 on its own
 * (nothing contracted): the torch expression `a * x0 + sigma * eps` as separate ops, bit for bit; sigma = 1 gives noise, sigma = 0 source. */
int k5_edit_renoise(float* out, const float* source, const float* noise, float sigma, int64_t n, void* stream);
/* k5_cfg_euler on cells * C elements (the same bits), then the keep rule of k5_euler_step_args at sigma_next: the fixed form of k5_euler_step
 * with source, noise and keep_mask.  keep_mask NULL = k5_cfg_euler (source / noise then unused).  One pass over the latent. */
int k5_cfg_euler_edit(float* img, const void* v_cond, const void* v_uncond, float w, float dt, const float* source, const float* noise,
                      const float* keep_mask, float sigma_next, int64_t cells, int C, void* stream);
/* Guidance coefficients and the guided update (added under ABI 11, as the exports above were).  The guided velocity of a
 * step is v = alpha c + beta u with one (alpha, beta) per sample, formed on the device from five float64 sums over the step's two velocities:
 *   Sc = sum c, Su = sum u, Scc = sum c^2, Suu = sum u^2, Scu = sum c u          (each product exact: two bf16 factors)
 *   s = zero_star ? Scu / (Suu + 1e-8) : 1                                        (CFG-Zero*, Fan et al. 2025: the projection of c on u)
 *   alpha = w, beta = s (1 - w)                                                   (v = s u + w (c - s u))
 *   rescale > 0: var_c = Scc - Sc^2 / n, var_v = alpha^2 var_c + 2 alpha beta (Scu - Sc Su / n) + beta^2 (Suu - Su^2 / n),
 *                k = (var_v > 0 and var_c >= 0) ? rescale sqrt(var_c / var_v) + (1 - rescale) : 1, alpha *= k, beta *= k
 *                                                                                 (CFG rescale, Lin et al. 2024: std over the sample)
 * v_cond, v_uncond: bf16 [n] on the device; part: device scratch of k5_guidance_stats_blocks(n) x 5 doubles; sums: device double[5], receives
 * the five sums in the order above; ab: device float[2], receives {(float)alpha, (float)beta}.  The summation order is fixed (a lane its
 * 16-byte chunks in index order, an xor butterfly over the wave, the four waves in order, the blocks in index order) and nothing is atomic:
 * every launch, rank and handle gives the same bits.  K5_ERR_ARG: a NULL or not 16-byte aligned pointer, n < 1, rescale outside [0, 1];
 * K5_ERR_ALIGN: n % 8 != 0.  Nothing is launched when the call is refused. */
int k5_guidance_stats_blocks(int64_t n);
int k5_guidance_coeffs_bf16(const void* v_cond, const void* v_uncond, int64_t n, float w, int zero_star, float rescale, double* part,
                            double* sums, float* ab, void* stream);
/* k5_cfg_euler_edit with the combine replaced by the coefficients ab = {alpha, beta}, fp32 on the DEVICE (k5_guidance_coeffs_bf16 writes them):
 * the fixed form of k5_euler_step with ab, which this entry requires (K5_ERR_ARG without).  v_out on v_cond and then k5_x0_preview with
 * v_uncond = NULL is the preview of a guided step.  The rounding points differ from k5_cfg_euler's, so ab = {w, 1 - w} need not give its bits. */
int k5_guided_euler(float* img, const void* v_cond, const void* v_uncond, const float* ab, float dt, const float* source, const float* noise,
                    const float* keep_mask, float sigma_next, int64_t cells, int C, void* v_out, void* stream);
/* The three-velocity update of skip-layer guidance (added under ABI 11, as the exports above were): v_skip is the
 * conditional velocity of a forward with some visual blocks skipped (k5_dit_forward_skip), g > 0 the scale, by value.  The fixed form of
 * k5_euler_step with v_skip and skip_scale = g, which this entry requires (K5_ERR_ARG without v_skip); ab, v_uncond and v_out as there. */
int k5_skip_euler(float* img, const void* v_cond, const void* v_uncond /* nullable */, const void* v_skip, float w,
                  const float* ab /* nullable, device */, float g, float dt, const float* source, const float* noise, const float* keep_mask,
                  float sigma_next, int64_t cells, int C, void* v_out, void* stream);
/* Counter-based noise and the stochastic update (added under ABI 11, as the exports above were).  The generator is
 * Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds): key = (low, high word of seed),
 * counter = (low, high word of the block index, c2, c3).  Nothing is read from memory and no generator state exists: two launches, two ranks,
 * the two handles of a CFG pair and a replayed graph all form the same words from the same arguments.
 * k5_philox_words: the raw words of blocks blk0 .. blk0 + nblk - 1 (the index wraps mod 2^64) into out [nblk][4] (device).
 * k5_noise_normal_f32: out[g] = z[g & 3] of block g >> 2 with counter words (stream_id, 0): u_j = ((r_j >> 9) + 0.5) 2^-23 (exact, inside
 * (0, 1)), (z0, z1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1), (z2, z3) from (u2, u3) likewise; fp32 throughout, no fast-math intrinsic.  Any n >= 1;
 * nothing past out[n - 1] is written.  K5_ERR_ARG: a NULL out, nblk or n < 1. */
int k5_philox_words(uint32_t* out /* [nblk][4] */, uint64_t blk0, int64_t nblk, uint64_t seed, uint32_t c2, uint32_t c3, void* stream);
int k5_noise_normal_f32(float* out, int64_t n, uint64_t seed, uint32_t stream_id, void* stream);
/* The stochastic flow-matching step (x_sigma = (1 - sigma) x0 + sigma eps; from s to t with churn eta: sigma_down = t (1 + (t / s - 1) eta),
 * a = (1 - t) / (1 - sigma_down), c = s_noise sqrt(max(0, t^2 - (sigma_down a)^2)); kandinsky.generation_utils.stochastic_plan builds
 * dt_down = sigma_down - s, scale = a and noise_coef = c per step).  The fixed form of k5_euler_step with stochastic = 1, always (noise_coef == 0
 * included): dt = dt_down, skip_scale = g, noise = eps (the edit's noise), znoise = noise. */
int k5_stochastic_euler(float* img, const void* v_cond, const void* v_uncond /* nullable */, const void* v_skip /* nullable */, float w,
                        const float* ab /* nullable, device */, float g, float dt_down, const float* source, const float* eps,
                        const float* keep_mask, float sigma_next, int64_t cells, int C, void* v_out, float scale, float noise_coef,
                        const float* noise /* nullable, device fp32 [cells * C] */, uint64_t seed, uint32_t stream_id, void* stream);
/* The sampler's update of one step, one pass over the latent (added under ABI 11, as the exports above were): the one
 * entry, of which k5_cfg_euler, k5_cfg_euler_edit, k5_guided_euler, k5_skip_euler and k5_stochastic_euler are fixed forms.  A zeroed struct
 * with w = 1, C = 1 and scale = 1 is the starting point; every pointer is device memory and NULL where it says "NULL =".  Per element g of
 * cells * C, with c, u, s the bf16 values of v_cond, v_uncond, v_skip, every operation rounded on its own (nothing contracted):
 *   base = ab ? bf16(rn(rn(ab[0] c) + rn(ab[1] u)))  :  v_uncond ? bf16(u + bf16(w bf16(c - u)))  :  c
 *          (ab = {alpha, beta} fp32, written by k5_guidance_coeffs_bf16; the middle form is generation_utils.py:74-76, v_uncond NULL = no guidance)
 *   v    = v_skip ? bf16(rn(base + e)), d = bf16(rn(c - s)), e = bf16(rn(skip_scale d))  :  base
 *          (torch eager `base + g * (c - s)` on bf16 tensors, bit for bit; skip_scale > 0 goes with v_skip, 0 with NULL)
 *   x1   = rn(img + bf16(rn(dt v)))                                              (generation_utils.py:128; a stochastic step passes its dt_down)
 *   x2   = stochastic && noise_coef != 0 ? rn(rn(scale x1) + rn(noise_coef z))  :  x1
 *          (z = znoise ? znoise[g] : k5_noise_normal_f32(seed, stream_id)[g]; stochastic with noise_coef == 0 gives the bits of the plain form)
 *   img  = keep_mask ? keep rule(x2)  :  x2
 *          (keep_mask fp32 [cells] in [0, 1], one value per C channels; known = rn(rn((1 - sigma_next) source) + rn(sigma_next noise)), k5_edit_renoise's
 *          bits; m == 1 -> known, m == 0 -> x2, otherwise rn(x2 + rn(m rn(known - x2))); `noise` is the edit's eps, not z)
 * v_out (bf16 [cells * C], NULL = not wanted, may be v_cond) receives v; it goes with ab or v_skip.  `stochastic` != 0 selects the
 * instantiation in which a thread owns the four elements of one generator block.
 * K5_ERR_ARG with a message that names the condition, nothing launched: a NULL args, img or v_cond; cells or C < 1; ab without v_uncond;
 * v_out without ab or v_skip; keep_mask without source and noise; v_skip without a finite skip_scale > 0, a skip_scale != 0 without v_skip;
 * stochastic with a scale that is not finite or a noise_coef that is negative or not finite; znoise without stochastic. */
typedef struct k5_euler_step_args {
  float* img;              /* fp32 [cells * C], updated in place */
  const void* v_cond;
  const void* v_uncond;    /* NULL = no guidance */
  const void* v_skip;      /* NULL = no skip term */
  void* v_out;             /* NULL = not wanted */
  const float* ab;         /* NULL = the CFG combine with w */
  float w;
  float dt;
  float skip_scale;
  const float* source;
  const float* noise;
  const float* keep_mask;  /* NULL = no keep rule */
  float sigma_next;
  int64_t cells;
  int C;
  int stochastic;
  float scale;
  float noise_coef;
  const float* znoise;     /* NULL = the generator's normals */
  uint64_t seed;
  uint32_t stream_id;
} k5_euler_step_args;
int k5_euler_step(const k5_euler_step_args* args, void* stream);
/* FlowEdit (added under ABI 11, as the exports above were; Kulikov et al. 2024, "FlowEdit: Inversion-Free Text-Based Editing Using Pre-Trained
 * Flow Models", Algorithm 1 with n_avg = 1).  x_src is the clean source latent, z_fe starts as x_src.  With N steps,
 * first = edit_first_step(N, strength) and R = refine, steps first <= i < N - R are FlowEdit steps and steps N - R <= i < N plain steps.
 * A FlowEdit step i: s = sigmas[i], dt = sigmas[i + 1] - sigmas[i], z = k5_noise_normal_f32(seed, stream_id = i).  Per element, every operation
 * rounded on its own (nothing contracted):
 *   zs   = rn(rn((1 - s) x_src) + rn(s z))                                       (k5_edit_renoise's bits with z as the noise)
 *   zt   = rn(zs + rn(z_fe - x_src))                                             (this order: z_fe == x_src gives zt == zs exactly)
 *   v_s  = w_src != 1 ? bf16(u_s + bf16(w_src bf16(c_s - u_s))) : c_s            (the CFG combine as k5_euler_step forms it)
 *   v_t  = likewise from c_t, u_t, w_tar
 *   d    = bf16(rn(v_t - v_s)),  e = bf16(rn(dt d))
 *   z_fe = m == 1 ? z_fe : m == 0 ? rn(z_fe + e) : rn(z_fe + rn(rn(1 - m) e))    (m = keep_mask[cell], 0 without a mask)
 * c_s, u_s: the forwards on zs with the source and the negative prompt at time 1000 s; c_t, u_t: those on zt with the target and the negative
 * prompt; on the stream in this order, a forward whose weight is 1 is not run.  Refine: the first plain step forms zt at sigmas[N - R] with
 * stream id N - R as above, steps N - R .. N - 1 are k5_euler_step steps on that latent with the target prompt and w_tar, and that latent is
 * the result; with R = 0 the result is z_fe.
 * k5_flowedit_step is one pass over the latent that finishes step i (the last five lines, when the velocities are given: c_src and c_tar
 * both or neither) and prepares step i + 1 (the first two, when `prepare` != 0: sigma_next is that step's s, stream_id its stream, zs / zt
 * receive its inputs and are formed from the z_fe just written).  Without velocities the launch only prepares: the first launch of a run.
 * Every pointer is device memory, 4-byte aligned; z_fe, zs and zt must not overlap each other or an input.  znoise (fp32 [cells * C], NULL =
 * the generator's normals) replaces z.  A u_* at weight 1 and, in a launch that only prepares, the velocities and the mask are not read.
 * K5_ERR_ARG with a message that names the condition, nothing launched: a NULL args, z_fe or x_src; cells or C < 1; c_src without c_tar or the
 * reverse; neither velocities nor prepare; w_src != 1 without u_src, w_tar != 1 without u_tar; prepare without zs and zt; a pointer that is
 * not 4-byte aligned. */
typedef struct k5_flowedit_step_args {
  float* z_fe;             /* fp32 [cells * C], updated in place when the velocities are given */
  const float* x_src;      /* fp32 [cells * C] */
  const void* c_src;       /* bf16 [cells * C] each; NULL (both c_*) = prepare only */
  const void* u_src;       /* needed where w_src != 1 */
  const void* c_tar;
  const void* u_tar;       /* needed where w_tar != 1 */
  float w_src;
  float w_tar;
  float dt;
  const float* keep_mask;  /* fp32 [cells], NULL = no mask */
  int prepare;             /* != 0: form zs / zt of the next step */
  float sigma_next;        /* the next step's s */
  float* zs;               /* fp32 [cells * C] each, written when prepare != 0 */
  float* zt;
  const float* znoise;     /* NULL = the generator's normals */
  uint64_t seed;
  uint32_t stream_id;      /* of the next step */
  int64_t cells;
  int C;
} k5_flowedit_step_args;
int k5_flowedit_step(const k5_flowedit_step_args* args, void* stream);
/* k5_cfg_euler over temporal context windows (added under ABI 11, as the exports above were): a clip of T frames whose velocities come from
 * nwin <= 64 windows of F frames.  img fp32 [T][frame_elems]; v_cond / v_uncond (NULL = no guidance) bf16 [nwin][F][frame_elems]; starts_dev
 * DEVICE int32 [nwin], window i covers frames starts[i] .. starts[i] + F - 1; weights_dev DEVICE fp32 [nwin][F], the share of window i's local
 * frame j (kandinsky.generation_utils.context_windows builds both).  Every element of frame t walks the windows that cover t in window order:
 * v_i as k5_cfg_euler forms it (the same three bf16 roundings), acc = rn(wt_0 * v_0), then acc = rn(acc + rn(wt_i * v_i)), nothing contracted;
 * img = rn(img + bf16(rn(dt * acc))).  One window of weight 1 is k5_cfg_euler bit for bit.  One pass over img.  This entry IS k5_cfg_euler_tiles
 * below, on the clip (T, 1, 1, frame_elems) with one row window and one column window of weight 1.0, whose share rn(rn(wt * 1) * 1) is wt itself.
 * K5_ERR_ARG + message, nothing launched: a NULL pointer, nwin outside 1..64, F < 1, frame_elems outside 1 .. 2^31 - 1, starts that do not
 * ascend, a window reaching outside 0..T-1, or a frame no window covers (the nwin starts are read back once, which synchronises the stream). */
int k5_cfg_euler_windows(float* img, const void* v_cond, const void* v_uncond, float w, float dt, const int32_t* starts_dev,
                         const float* weights_dev, int nwin, int F, int T, int64_t frame_elems, void* stream);
/* k5_cfg_euler over a 3-D plan of context windows (spatial tiles; added under ABI 11, as the exports above were).  img fp32 (T,H,W,C); the
 * plan is the product of three 1-D plans (kandinsky.generation_utils.tile_windows): nt x ny x nx windows of (Ft,Fh,Fw) cells, window
 * k = (it * ny + iy) * nx + ix with its corner at (starts_t[it], starts_y[iy], starts_x[ix]); v_cond / v_uncond (NULL = no guidance) bf16
 * [nwin][Ft][Fh][Fw][C], nwin = nt * ny * nx <= 64.  The six tables are DEVICE memory.  The rule, with every rounding point:
 *   1. cell (t,y,x) walks the windows that cover it in ascending k;
 *   2. window k's share is s_k = rn(rn(wt[it][t - t0] * wy[iy][y - y0]) * wx[ix][x - x0]);
 *   3. v_k is formed as k5_cfg_euler forms it (the same three bf16 roundings);
 *   4. acc = rn(s_0 * v_0), then acc = rn(acc + rn(s_k * v_k));
 *   5. nothing is contracted;
 *   6. img = rn(img + bf16(rn(dt * acc))).
 * ny = nx = 1 with weights 1.0 is a temporal plan (k5_cfg_euler_windows), one window of weight 1 is k5_cfg_euler bit for bit.  One pass over img;
 * only velocity slots inside a window's box are read, whatever the tables hold.  K5_ERR_ARG + message, nothing launched: a NULL pointer, nwin
 * outside 1..64, an extent or window size < 1, starts of an axis that do not ascend, a window reaching outside the clip, or a cell no window
 * covers (the nt + ny + nx starts are read back once, which synchronises the stream). */
typedef struct k5_tile_plan {
  int nt, ny, nx, Ft, Fh, Fw;
  const int32_t* starts_t;   /* DEVICE [nt] */
  const int32_t* starts_y;   /* DEVICE [ny] */
  const int32_t* starts_x;   /* DEVICE [nx] */
  const float* wt;           /* DEVICE [nt][Ft] */
  const float* wy;           /* DEVICE [ny][Fh] */
  const float* wx;           /* DEVICE [nx][Fw] */
} k5_tile_plan;
int k5_cfg_euler_tiles(float* img, const void* v_cond, const void* v_uncond, float w, float dt, const k5_tile_plan* plan, int T, int H, int W,
                       int C, void* stream);
/* Sampler preview (added under ABI 11, as the exports above were): the denoised estimate of a flow-matching step and a cheap RGB view of it, one
 * pass.  After the update of a step the latent x (fp32, cells * C) sits at sigma_next and v_cond / v_uncond (bf16, v_uncond NULL = no guidance)
 * still hold that step's velocities: v is combined exactly as in k5_cfg_euler, x0 = rn(x - rn(sigma_next * v)) in fp32 (sigma_next == 0 gives
 * x bit for bit), and with keep_mask (fp32 [cells], as k5_cfg_euler_edit) x0 = keep rule(x0, source, m), so kept cells show the source.
 * x0_out (fp32 cells * C, or NULL) receives x0; rgb (uint8 cells * 3, or NULL) receives
 *   rgb[cell][j] = sat_u8(rint((b[j] + sum_k W[k][j] x0[k]) * 127.5 + 127.5)), NaN -> 0,
 * W = rgb_w [C][3] and b = rgb_b [3] (NULL = zeros), fp32 on the DEVICE.  The sum has a fixed order (deterministic bits): four lanes share a
 * cell, lane q takes channels 4(q + 4i) .. 4(q + 4i) + 3 for i = 0, 1, .. in ascending order as acc = fma(W[k][j], x0[k], acc) from 0; the four
 * partial sums add as (a0 + a1) + (a2 + a3); then fma(b[j] + sum, 127.5, 127.5).  rgb and rgb_w are given together or not at all and one of
 * rgb / x0_out is needed (K5_ERR_ARG); x, x0_out, source 16-byte and the velocities 8-byte aligned (K5_ERR_ARG); C % 4 == 0 and C <= 64,
 * anything else is K5_ERR_UNSUPPORTED.  Nothing is launched when the call is refused. */
int k5_x0_preview(const float* x, const void* v_cond, const void* v_uncond, float w, float sigma_next, const float* source,
                  const float* keep_mask, const float* rgb_w, const float* rgb_b, float* x0_out, uint8_t* rgb, int64_t cells, int C,
                  void* stream);
/* Normalized attention guidance, the combine (added under ABI 11, as the exports above were): z_pos and z_neg are the outputs of ONE cross-attention
 * against the positive and the negative text (the same queries), bf16 [rows][ld] of which D columns are used; out likewise, and out == z_pos is
 * allowed.  Per row, in fp32, every operation rounded on its own except the one written fma:
 *   d = zp - zn;  g = fma(s - 1, d, zp)                          (= zp + (s - 1)(zp - zn))
 *   n_pos = sum_k |zp_k|,  n_g = sum_k |g_k|                     over all D channels (all heads)
 *   f = 1 if n_g <= tau * n_pos (this includes 0 <= 0), else (tau * n_pos) / n_g
 *   out = bf16(zp + alpha * (f * g - zp))                         nearest-even
 * which is the published rule (Chen et al. 2025: extrapolate s zp - (s - 1) zn, clamp the growth of the row's L1 norm at tau, blend with alpha)
 * arranged so that finite inputs give no NaN (a zero row gives zero) and that z_neg == z_pos, s == 1 and alpha == 0 each return z_pos bit for
 * bit.  The two sums have a fixed order (one wave per row: a lane adds its 8-column chunks lane, lane + 64, .. in ascending column order, then an
 * xor butterfly over the 64 lanes), so equal inputs give equal bits.  One pass: both inputs read once, out written once, 16 bytes per lane.
 * K5_ERR_ARG: a NULL or not 16-byte aligned pointer, rows < 1, D % 8, ld < D, ld % 8, s < 1, tau < 1, alpha outside [0, 1]; K5_ERR_UNSUPPORTED:
 * D > 2048 (the row is held in registers).  Nothing is launched when the call is refused. */
int k5_nag_combine_bf16(const void* z_pos, const void* z_neg, void* out, int rows, int D, int ld, float s, float tau, float alpha,
                        void* stream);
/* Enhance-A-Video, the rule (added under ABI 11, as the exports above were; Luo et al. 2025, "FETA" in the Wan /
 * HunyuanVideo / CogVideoX wrappers).  For one forward and one visual block, let the latent have T frames and S = (H/2)(W/2) spatial
 * positions, Hh heads of 64 columns; q[t,p,h] and k[t,p,h] are the query and the key after norm_qk + RoPE, weight >= 0:
 *   z[t][u]  = (1/8) <q[t,p,h], k[u,p,h]>                  t, u in 0..T-1   (the block's own softmax scale)
 *   P[t][.]  = softmax over u of z[t][.]                   row maximum subtracted; fp32
 *   m(p,h)   = ( sum_{t != u} P[t][u] ) / (T (T - 1))
 *   mean     = ( sum_{p,h} m(p,h) ) / (S Hh)               float64, fixed order, no atomics
 *   score    = max(1, mean (T + weight))                   stored as fp32
 *   o'       = bf16( float(o) score )                      the attention output, before the out projection
 * This is the published feta_score / get_feta_scores form; ours: T < 2 (images) makes it inert, and the mean is per forward (the engine
 * runs the conditional and the unconditional forward separately).  With d the mean diagonal probability, mean = (1 - d) / (T - 1): uniform
 * attention gives score = 1 + weight / T.
 * k5_enhance_scores_bf16 computes the score: Q and K are bf16 with 64 columns per head (row strides ldq / ldk elements; both may point into
 * one fused [rows][2 * 64 Hh] buffer), the token row of (p, t) is frame_rows[p * T + t] (device int32 [S][T]; NULL: row = t * S + p; rows the
 * table does not name and columns beyond 64 Hh are never read).  qk_scale multiplies the dot product and the softmax is taken in base 2: 1.0
 * for keys already multiplied by log2(e) / 8, log2(e) / 8 for plain keys.  One workgroup per p, one wave per head; the T x T logits are K·Q^T
 * on v_mfma_f32_32x32x16_bf16 with T padded to 32 or 64 (a padded key adds exactly 0, a padded query nothing); every wave writes its column's
 * float64 sum to part[p * Hh + h] (part: device, k5_enhance_part_count(Hh, S) doubles) and a second, one-workgroup launch adds them in a fixed
 * order and writes score_out[0] (device fp32).  No atomics: equal inputs give equal bits on every launch.
 * K5_ERR_ARG: a NULL or not 16-byte aligned Q / K, a NULL part or score_out, ldq / ldk < 64 Hh or not a multiple of 8, Hh or S < 1, T < 2, a
 * negative or non-finite weight, qk_scale <= 0 or not finite.  K5_ERR_UNSUPPORTED: T > 64 (a wave holds the column's logits in four 32 x 32
 * accumulators).  Nothing is launched when the call is refused. */
long long k5_enhance_part_count(int Hh, int S);
int k5_enhance_scores_bf16(const void* Q, const void* K, int ldq, int ldk, int Hh, int T, int S,
                           const int32_t* frame_rows /* device [S][T], NULL: row = t*S + p */,
                           float qk_scale, float weight, double* part, float* score_out, void* stream);
/* x bf16 [rows][ld] (D columns used) times the fp32 scalar at score_dev (device), in place: bf16(float(x) * s), nearest-even — torch's x * s
 * for a bf16 tensor and a 0-dim fp32 tensor.  Grid-stride, 16 bytes per lane.  A workgroup that reads s == 1.0f returns without touching
 * memory (NaN payloads, -0 and the pad columns stay as they are): a clamped block costs a launch and no traffic.
 * K5_ERR_ARG: a NULL or not 16-byte aligned x, a NULL score_dev, rows < 1, D % 8, ld < D, ld % 8.  Nothing is launched when refused. */
int k5_scale_by_dev_bf16(void* x, int rows, int D, int ld, const float* score_dev, void* stream);
/* Regional prompts, the rule (added under ABI 11).  The base prompt is the forward's ordinary prompt; there are R region prompts,
 * 1 <= R <= 8, each with a mask m_r in [0, 1] on the latent cells (T, H, W), the grid of the keep mask.
 *   Token weights.  A token is a patch_size block of cells; m_r(token) is the fp32 mean of its cells.  raw_0 = base_weight + max(0, 1 - sum_r m_r)
 *   with base_weight in [0, 1]; raw_r = m_r; s = sum raw; w_i = raw_i / s.  s >= 1 always (sum m < 1: s = base_weight + 1, otherwise
 *   s = base_weight + sum m).  An uncovered token has the base prompt only; masks that partition the frame with base_weight 0 give each token
 *   exactly one prompt.
 *   Blend.  In every visual block, on the conditional forward only, the queries are projected and normalised once and attend to the base
 *   stream (z_0) and to each region stream (z_r); the out projection sees out = sum_i w_i z_i per token.
 * k5_region_combine_bf16 is the blend: z0 bf16 [rows][ld] of which D columns are used, region r at zr + r * zr_stride ELEMENTS (same layout), w
 * fp32 [rows][ldw] with ldw >= R + 1 (column 0 the base stream's weight), out like z0 and out == z0 is allowed.  Per element in fp32: the first
 * stream with a non-zero weight gives acc = w z (one rounded product), every later non-zero one acc = fmaf(w, z, acc), ascending from the base
 * stream; out = bf16(acc), nearest-even, once.  A stream whose weight is exactly 0 for a row is not read and not added (NaN there does not reach
 * out); a row whose only non-zero weight is 1.0 is that stream's bits, negative zeros included; a row without a non-zero weight is +0.  One wave
 * per row, 16 bytes per lane, each used input read once, out written once; equal inputs give equal bits.
 * K5_ERR_ARG: a NULL pointer, rows or D < 1, ld < D, D % 8, ld % 8, zr_stride % 8, a pointer not 16-byte aligned (w: 4-byte), R outside 1..8,
 * ldw < R + 1; K5_ERR_UNSUPPORTED: D > 2048 (the row is held in registers).  Nothing is launched when the call is refused.
 * k5_region_weights_f32 is the token weights: masks device fp32 [R][T][H][W], patch (pt, ph, pw) dividing (T, H, W), perm the order of the N =
 * (T / pt)(H / ph)(W / pw) tokens (row i of w is token perm[i] of the row-major grid; NULL: i), w fp32 [N][R + 1].  Every cell is clamped to
 * [0, 1] (NaN counts as 0); a token's cells are added in ascending (t, h, w) order and divided by their count; sm = m_1 + .. + m_R ascending;
 * raw_0 = base_weight + max(0, 1 - sm); s = raw_0 + m_1 + .. + m_R ascending; each operation rounded on its own, no atomics.  K5_ERR_ARG: a NULL
 * or not 4-byte aligned masks / w, R outside 1..8, a shape < 1 or not divisible by the patch, base_weight outside [0, 1] or NaN. */
int k5_region_combine_bf16(const void* z0, const void* zr, long long zr_stride, int R, const float* w, int ldw, void* out, int rows, int D,
                           int ld, void* stream);
int k5_region_weights_f32(const float* masks, int R, int T, int H, int W, int pt, int ph, int pw, float base_weight, const int32_t* perm,
                          float* w, void* stream);
/* LoRA merge, in place on a row-major matrix (added under ABI 11, as the MagCache calibration exports were): W'[n][k] = W[n][k] + scale *
 * sum_r B[n][r] A[r][k].  W [rows][ld] (cols <= ld) of w_dtype K5_BF16 or K5_F32;
 * A [R][cols], B [rows][R], each K5_F32 / K5_BF16 / K5_F16, device pointers, converted to fp32 on load; 1 <= R <= 256.  The arithmetic is
 * fixed: acc = fma(B[n][r], A[r][k], acc) for r = 0 .. R-1 from acc = 0, then fma(scale, acc, W[n][k]), both in float64 (an fp32 chain misses the
 * bf16 neighbours of the exact value where W and the update cancel), rounded to fp32 and, for a bf16 W, from there to bf16 (nearest-even).  Columns cols .. ld-1 are
 * neither read nor written; scale == 0 launches nothing.  Stands where a front end would merge `W + scale * (B @ A)` on the host before
 * load_state_dict (the reference has no adapter code of its own). */
int k5_lora_merge(void* W, int w_dtype, int rows, int cols, int ld, const void* A, int a_dtype, const void* B, int b_dtype, int R,
                  float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Engine: DiffusionTransformer3D (kandinsky/models/dit.py:82-181) + sampler loop
 * (kandinsky/generation_utils.py:39-129).
 * ---------------------------------------------------------------------------------------- */
typedef struct k5_dit k5_dit;

/* ctor kwargs of DiffusionTransformer3D, dit.py:83-97 */
typedef struct k5_dit_config {
  int in_visual_dim, in_text_dim, in_text_dim2, time_dim, out_visual_dim;
  int patch_size[3];
  int model_dim, ff_dim, num_text_blocks, num_visual_blocks;
  int axes_dims[3];
  int visual_cond;
} k5_dit_config;

/* arguments of DiffusionTransformer3D.forward, dit.py:155-165 (+ sparse_params of
 * generation_utils.py:10-36) */
typedef struct k5_text_cond {
  const void* text_embed;   /* device, [text_len][in_text_dim], dtype text_dtype */
  const void* pooled_embed; /* device, [1][in_text_dim2], dtype text_dtype */
  int text_dtype;           /* k5_dtype */
  int text_len;
  const int32_t* text_rope_pos; /* HOST, [text_len] */
} k5_text_cond;

typedef struct k5_forward_args {
  const float* x;           /* device fp32 (T,H,W,x_channels) */
  int T, H, W, x_channels;  /* x_channels = visual_embed_dim, or in_visual_dim (cond channels implied zero) */
  k5_text_cond cond;
  float time;               /* 1000*sigma (generation_utils.py:57) */
  const int32_t* pos_t;     /* HOST visual_rope_pos[0..2] (generation_utils.py:173-177) */
  const int32_t* pos_h;
  const int32_t* pos_w;
  float scale_factor[3];    /* conf.metrics.scale_factor */
  int attention_type;       /* 0 = flash (dense), 1 = nabla */
  float nabla_P; int nabla_wT, nabla_wH, nabla_wW;
} k5_forward_args;

typedef struct k5_sample_args {
  k5_forward_args fwd;      /* fwd.x ignored; fwd.time ignored */
  k5_text_cond null_cond;   /* used when |guidance_weight-1| > 1e-6 */
  float* latent;            /* device fp32 (T,H,W,in_visual_dim), in: noise, out: final latent */
  int num_steps;
  const float* sigmas;      /* HOST [num_steps+1] (generation_utils.py:102-103) */
  float guidance_weight;
} k5_sample_args;

int k5_dit_create(const k5_dit_config* cfg, k5_dit** out);
void k5_dit_destroy(k5_dit* dit);
/* state_dict entry (checkpoint layout SURVEY.md App. D): host pointer, any of f32/bf16/f16. */
int k5_dit_load_tensor(k5_dit* dit, const char* key, const void* host_ptr, int dtype, const int64_t* shape,
                       int rank);
/* all tensors loaded -> pack (concat Wq|Wk, pad, cast) ; must precede forward */
int k5_dit_finalize(k5_dit* dit);
/* number of state_dict keys still missing (0 after a complete load); names via k5_last_error() */
int k5_dit_missing_keys(k5_dit* dit);
/* velocity (T,H,W,out_visual_dim) bf16, device */
int k5_dit_forward(k5_dit* dit, const k5_forward_args* args, void* out_velocity, void* stream);
/* whole Euler loop on device (generate, generation_utils.py:80-129) */
int k5_sample(k5_dit* dit, const k5_sample_args* args, void* stream);
/* k5_sample with the conditioning channels of a visual_cond model filled (image-to-video, latent continuation): visual_cond is a
 * borrowed device fp32 (T,H,W,in_visual_dim+1) tensor — channels 0..in_visual_dim-1 the conditioning latent, the last one the mask —
 * constant for the call; every forward patchifies cat([latent, visual_cond], -1).  NULL = k5_sample.  K5_ERR_ARG when visual_cond is
 * given to a handle created with visual_cond = 0 or is not 4-byte aligned. */
int k5_sample_cond(k5_dit* dit, const k5_sample_args* args, const float* visual_cond, void* stream);

/* Video-to-video and masked editing (SDEdit / inpainting; extends the loop of generation_utils.py:102-128, which starts from pure noise only).
 * The latent starts as renoise(sigmas[0]) of `source` with `noise` (k5_edit_renoise) and after the CFG + Euler update of every step i the
 * kept region is put back at sigmas[i+1] (k5_cfg_euler_edit), on the device next to the update, so the captured step replays it.  After the
 * last step sigma = 0 and the cells with keep_mask == 1 hold `source` bit for bit.  A strength below 1 is a shorter schedule: the caller
 * hands sigmas[first:] and num_steps - first.  edit == NULL is k5_sample_cond.  Otherwise args->latent is OUTPUT ONLY; source, noise
 * (device fp32 (T,H,W,in_visual_dim)) and keep_mask (device fp32 (T,H,W,1), 1 = keep the source, or NULL) are borrowed and constant for
 * the call.  K5_ERR_ARG + message, before anything is enqueued: a NULL source or noise, a pointer that is not 4-byte aligned, or source /
 * noise / keep_mask overlapping latent.  Works in every mode of the loop (eager, captured step, MagCache, rank groups and the CFG pair). */
typedef struct k5_edit_args {
  const float* source;
  const float* noise;
  const float* keep_mask;   /* device; NULL = no mask */
} k5_edit_args;
int k5_sample_edit(k5_dit* dit, const k5_sample_args* args, const float* visual_cond /* nullable */, const k5_edit_args* edit, void* stream);

/* FlowEdit: prompt-driven editing of a clip (added under ABI 11; the rule is written at k5_flowedit_step_args).  `source` is the clean source
 * latent (device fp32 (T,H,W,in_visual_dim)), source_cond the prompt that describes it and source_weight its guidance weight; sample.fwd.cond,
 * sample.guidance_weight and sample.null_cond are the target side, the negative prompt is shared by both.  sample.latent is OUTPUT ONLY.  A
 * strength below 1 is a shorter schedule, as for k5_sample_edit: the caller hands sigmas[first:] and num_steps - first, and first_stream = first,
 * so that step i draws from stream first_stream + i — the noise of the full schedule.  The last `refine` steps are plain steps on the target
 * side.  keep_mask (device fp32 (T,H,W,1), 1 = keep the source, or NULL): kept cells hold `source` bit for bit.  A side whose weight is 1
 * (within 1e-6, as k5_sample decides) runs no unconditional forward: a step is two to four forwards — source cond, source uncond, target cond,
 * target uncond — and one k5_flowedit_step pass.  The text prologue of every distinct prompt is computed once per call.  Always eager, also with
 * k5_dit_set_graph on; never returns to the host between steps.  A watch without previews, Enhance-A-Video, visual_cond, NABLA, fp8 and LoRA
 * work as for a plain step.  Refused before anything is enqueued, with a message: K5_ERR_STATE on a handle in a sequence-parallel group or a
 * CFG pair, with MagCache or its calibration, a forecast plan that has forecast steps, skip-layer guidance, a guidance plan, a stochastic plan,
 * NAG or regions set, or a watch with previews; K5_ERR_ARG for a NULL source or source prompt, refine outside 0..num_steps, refine > 0 with a
 * keep_mask, a pointer that is not 4-byte aligned, or source / keep_mask / visual_cond overlapping latent.
 * k5_dit_flowedit_state: since the last reset, the FlowEdit steps and the forwards that k5_sample_flowedit calls enqueued and the text
 * prologues they computed (any out pointer may be NULL; reset != 0 zeroes the three after reading). */
typedef struct k5_flowedit_args {
  const float* source;
  k5_text_cond source_cond;
  float source_weight;
  const float* keep_mask;   /* device; NULL = no mask */
  int refine;
  uint64_t seed;
  uint32_t first_stream;
} k5_flowedit_args;
int k5_sample_flowedit(k5_dit* dit, const k5_sample_args* sample, const k5_flowedit_args* flowedit, const float* visual_cond /* nullable */,
                       void* stream);
int k5_dit_flowedit_state(k5_dit* dit, long long* steps, long long* forwards, long long* prologues, int reset);

/* Long clips: temporal context windows (added under ABI 11; extends the loop of generation_utils.py:102-128, which runs one forward over the whole
 * clip).  A clip of total_T latent frames, longer than the model's trained length, is sampled as nwin overlapping windows of sample.fwd.T frames:
 * at every step each window runs the forward(s) on its own contiguous slice of the latent (and of visual_cond) with the window's RoPE positions
 * sample.fwd.pos_t = 0 .. T-1, in window order and conditional before unconditional, and one k5_cfg_euler_windows pass cross-fades the
 * windows' velocities into the update of the whole latent.  The result is bit-identical to the same forwards issued one by one through
 * k5_dit_forward on a fresh softmax-form memory followed by k5_cfg_euler_windows per step.
 *   sample: as k5_sample, except that fwd.T (and pos_t) is the WINDOW and latent is device fp32 (total_T,H,W,in_visual_dim).
 *   starts HOST [nwin], ascending, 0 <= starts[i], starts[i] + fwd.T <= total_T, every frame covered; weights HOST [nwin][fwd.T].
 *   conds / null_conds: HOST [nwin] prompts, one per window, or NULL = sample.fwd.cond / sample.null_cond for every window.
 *   visual_cond (k5_sample_cond): device fp32 (total_T,H,W,in_visual_dim+1) or NULL.
 * This entry IS k5_sample_tiles below with one row window and one column window of weight 1.0 that span the clip (ny = nx = 1, total_H = fwd.H,
 * total_W = fwd.W): such windows are whole frames, so the forwards read their contiguous slices as they always did.
 * total_T <= fwd.T (one window) is k5_sample_cond on total_T frames.  Always eager, also with k5_dit_set_graph on.  A watch without previews
 * works (progress, cancel; info->T = total_T).  Refused before anything is enqueued, with a message: K5_ERR_STATE on a handle in a
 * sequence-parallel group or a CFG pair (any transport), with MagCache or its calibration set (the table is indexed by the call of a plain run),
 * with a watch that has previews (the preview reads one velocity pair per cell); K5_ERR_ARG for nwin outside 1..64, starts that do not ascend or
 * leave 0..total_T, a frame without a window, NULL starts / weights, odd fwd.H or fwd.W (the check of every window plan: an odd latent is
 * refused before anything is enqueued, not inside the first forward). */
typedef struct k5_sample_windows_args {
  k5_sample_args sample;
  int total_T, nwin;
  const int32_t* starts;             /* HOST [nwin] */
  const float* weights;              /* HOST [nwin][sample.fwd.T] */
  const k5_text_cond* conds;         /* HOST [nwin] or NULL */
  const k5_text_cond* null_conds;    /* HOST [nwin] or NULL */
} k5_sample_windows_args;
int k5_sample_windows(k5_dit* dit, const k5_sample_windows_args* args, const float* visual_cond /* nullable */, void* stream);

/* Large frames: spatial context windows (tiles; added under ABI 11).  k5_sample_windows in three axes: a clip of (total_T, total_H, total_W)
 * latent cells, larger than the model's trained size, is sampled as nt x ny x nx overlapping windows of (sample.fwd.T, fwd.H, fwd.W) cells.
 * A spatial window is not contiguous: each forward patchifies a strided view of the latent (k5_patchify_view_bf16) and writes the compact slot
 * k = (it * ny + iy) * nx + ix of the velocity buffers; at every step the windows run in order k, conditional before unconditional, with the
 * window's RoPE positions sample.fwd.pos_t / pos_h / pos_w, and one k5_cfg_euler_tiles pass cross-fades their velocities into the update of
 * the whole latent.  The result is bit-identical to the same forwards issued one by one through k5_dit_forward on contiguous copies of the
 * views, on a fresh softmax-form memory, followed by k5_cfg_euler_tiles per step.
 *   sample: as k5_sample, except that fwd.T / H / W (and pos_*, the NABLA geometry, Enhance-A-Video's T) are the WINDOW's and latent is device
 *           fp32 (total_T,total_H,total_W,in_visual_dim).
 *   starts_* HOST, ascending per axis, every window inside the clip, every cell covered, spatial starts even (patch-aligned);
 *   wt / wy / wx HOST [nt][fwd.T], [ny][fwd.H], [nx][fwd.W].
 *   conds / null_conds: HOST [nt * ny * nx] prompts, one per window, or NULL.
 *   visual_cond: device fp32 (total_T,total_H,total_W,in_visual_dim+1) or NULL; each window sees its slice through the view.
 * A clip no larger than the window in every axis is k5_sample_cond on the whole clip; ny = nx = 1 with total_H = fwd.H and total_W = fwd.W is
 * a temporal plan, what k5_sample_windows passes.  Always eager, also with k5_dit_set_graph on.  A watch without previews works (progress, cancel;
 * info reports the whole clip's extents).  NAG and Enhance-A-Video work.  Refused before anything is enqueued, by the same checks and error
 * codes as k5_sample_windows: rank groups, CFG pairs, MagCache or its calibration, a watch with previews, a forecast plan with forecast
 * steps, guidance plans, skip-layer guidance, a stochastic plan, regions; K5_ERR_ARG for a plan that does not hold (nwin outside 1..64, an
 * axis whose starts do not ascend or leave the clip, an uncovered cell, odd spatial starts or extents, NULL tables). */
typedef struct k5_sample_tiles_args {
  k5_sample_args sample;
  int total_T, total_H, total_W;
  int nt, ny, nx;
  const int32_t* starts_t;           /* HOST [nt] */
  const int32_t* starts_y;           /* HOST [ny] */
  const int32_t* starts_x;           /* HOST [nx] */
  const float* wt;                   /* HOST [nt][sample.fwd.T] */
  const float* wy;                   /* HOST [ny][sample.fwd.H] */
  const float* wx;                   /* HOST [nx][sample.fwd.W] */
  const k5_text_cond* conds;         /* HOST [nt * ny * nx] or NULL */
  const k5_text_cond* null_conds;    /* HOST [nt * ny * nx] or NULL */
} k5_sample_tiles_args;
int k5_sample_tiles(k5_dit* dit, const k5_sample_tiles_args* args, const float* visual_cond /* nullable */, void* stream);

/* Several samples in one call (generate_sample's shape = (bs, frames, h, w, c), reference generation_utils.py:150): a CONVENIENCE entry point,
 * not a batched kernel path.  The B samples of one (T, H, W) run ONE AFTER ANOTHER on the stream, each as k5_sample_cond on its own slice of
 * the latents and the conditioning with its own prompts: the launches, the kernels and the cost per sample are those of B separate calls
 * (DESIGN.md §5, §8), and every sample is bit-identical to the same sample (noise, prompt, negative prompt, conditioning) run alone through
 * k5_sample / k5_sample_cond on the same handle with the same options.
 * Refused (K5_ERR_STATE + message) on a handle in a sequence-parallel group or a CFG pair (any transport), with MagCache or its calibration set or with
 * k5_dit_set_graph on; K5_ERR_ARG for B < 1, a NULL or non-4-byte-aligned latents / visual_cond pointer, missing conds or null conds,
 * or visual_cond on a handle created with visual_cond = 0.  Nothing is enqueued when the call is refused. */
typedef struct k5_sample_many_args {
  int B;
  k5_forward_args fwd;               /* shared shape, RoPE positions, scale factor, attention type; fwd.x, fwd.cond, fwd.time ignored */
  const k5_text_cond* conds;         /* HOST [B]: the prompt of each sample */
  const k5_text_cond* null_conds;    /* HOST [B]: the negative prompt of each sample; used (and required) when |guidance_weight-1| > 1e-6 */
  float* latents;                    /* device fp32 [B][T][H][W][in_visual_dim], in: noise, out: final latents */
  const float* visual_cond;          /* device fp32 [B][T][H][W][in_visual_dim+1] (as k5_sample_cond, per sample) or NULL */
  int num_steps;
  const float* sigmas;               /* HOST [num_steps+1] */
  float guidance_weight;
} k5_sample_many_args;
int k5_sample_many(k5_dit* dit, const k5_sample_many_args* args, void* stream);
/* A watch on the handle (added under ABI 11): progress, cancel and live previews out of k5_sample / k5_sample_cond / k5_sample_edit /
 * k5_sample_many, which otherwise return only when the whole loop is done.  With a watch installed the engine calls `fn` once per completed
 * step, in order, on the thread that called k5_sample*, and a non-zero return stops the run.  Without one the sampler enqueues exactly what it
 * always did: not one launch, event or synchronisation more.
 *   After step i the engine enqueues on the sampler's stream — on preview steps only — k5_x0_preview (sigma_next = sigmas[i+1], the call's
 *   guidance weight, source / keep_mask of k5_sample_edit) and a device-to-host copy of the RGB into one of TWO pinned slots it owns, then
 *   records an event.  The callback of step i runs once that event has completed and only after step i+1 has been enqueued (one step of
 *   look-ahead): the GPU never waits for the host, and the slot (rgb and x0) the callback reads is not the one being written.  In the captured-step
 *   mode the preview launches sit between the graph launches; nothing is added to the captured graph.
 *   Stop: after a non-zero return nothing more is enqueued, the stream is synchronised, the callback is not called again and k5_sample* returns
 *   K5_OK.  The latent is then the state after `steps_done` steps (k5_dit_watch_state), at most one step past the one the callback saw;
 *   k5_sample_many leaves the remaining samples untouched (steps_done counts the steps of the sample that was stopped).
 *   info->rgb / info->x0 are valid during the callback only.  THE CALLBACK MUST NOT CALL INTO THE SAME HANDLE (another handle, or plain HIP work
 *   on another stream, is fine).
 * Works in eager mode, the captured step, with MagCache and its calibration, with visual conditioning and editing.  Refused with K5_ERR_STATE
 * and a message, by k5_dit_set_watch and — when the group was formed later — by k5_sample* before anything is enqueued, on a handle in a
 * sequence-parallel group or a CFG pair (any transport): a rank that stops alone would leave its peers inside a collective.  K5_ERR_ARG:
 * fn NULL, preview_every < 0, previews without rgb_w, want_x0 without previews; K5_ERR_UNSUPPORTED: previews on a handle whose in_visual_dim
 * is not a multiple of 4 or exceeds 64.  The pinned slots and the device buffers are freed by k5_dit_destroy. */
typedef struct k5_watch_info {
  int step, num_steps;      /* step just completed, 0-based */
  int sample, num_samples;  /* k5_sample_many; 0 / 1 otherwise */
  float sigma_next;
  const uint8_t* rgb;       /* HOST (pinned, engine-owned) (T,H,W,3) or NULL on a step without a preview */
  const float* x0;          /* DEVICE (engine-owned) (T,H,W,C) or NULL */
  int T, H, W, C;
} k5_watch_info;
typedef int (*k5_watch_fn)(void* user, const k5_watch_info* info);   /* non-zero = stop */
typedef struct k5_watch {
  k5_watch_fn fn; void* user;
  int preview_every;        /* 0 = never; k > 0 = steps with (step+1) % k == 0, and always the last step */
  int want_x0;
  const float* rgb_w;       /* HOST [C][3], copied at set time; NULL only when preview_every == 0 */
  const float* rgb_b;       /* HOST [3] or NULL = zeros */
} k5_watch;
int k5_dit_set_watch(k5_dit* dit, const k5_watch* watch /* NULL clears */);
/* of the last k5_sample* call: steps enqueued and completed, and whether the callback stopped it (0 / 1) */
int k5_dit_watch_state(k5_dit* dit, int* steps_done, int* stopped);

/* Normalized attention guidance on the handle (added under ABI 11): a negative prompt inside the cross-attention of ONE forward, for runs
 * without classifier-free guidance.  While set, every CONDITIONAL forward (k5_dit_forward, k5_dit_forward_many, the conditional branch of
 * k5_sample* — never the unconditional one) carries a second text stream: the negative prompt's tokens go through the text prologue and the
 * text blocks as the positive ones do, with their own RoPE positions and the forward's own time embedding (a forward has one: it is built from
 * the POSITIVE prompt's pooled embedding, negative->pooled_embed is not read); every visual block projects and normalises its queries once,
 * attends once to each stream and k5_nag_combine_bf16(scale, tau, alpha) joins the two outputs in front of the out projection.  Per block that
 * is one cross-attention launch and one memory-bound pass more; the text side runs twice.  Not set, a forward enqueues exactly what it always
 * did.  `negative` is BORROWED: the struct and what it points to stay valid until the guidance is cleared; its pointers are read at every
 * forward (k5_sample* caches the negative prologue per call, as it does for the two other prompts).  One negative prompt serves every sample of
 * k5_sample_many and every window of k5_sample_windows.  Works on sequence-parallel shards (the text is replicated, the rule is per token:
 * no collective is added), on the conditional handle of a CFG pair, in the captured step, under k5_sample_edit, and with MagCache (a skipped
 * step runs no visual block and so no guidance; the shipped ratio tables were measured without it — calibrate with it set).
 * K5_ERR_ARG: scale < 1, tau < 1, alpha outside [0, 1], text_len < 1, a NULL text_embed or text_rope_pos.  scale == 1 or alpha == 0 is accepted
 * and means off (the combine would return z_pos).  NULL clears.  k5_dit_nag_state: whether guidance is on, and how many combines the handle
 * has enqueued (num_visual_blocks per guided forward), optionally resetting the count. */
int k5_dit_set_nag(k5_dit* dit, const k5_text_cond* negative /* NULL clears */, float scale, float tau, float alpha);
int k5_dit_nag_state(k5_dit* dit, int* on, long long* combines, int reset);
/* Guidance plan (added under ABI 11, as the exports above were): what the sampler does with the two velocities of a step.
 *   weights          per-step guidance weight w_i, HOST [num_weights], copied by the call; NULL = the call's guidance_weight at every step.
 *   zero_star        CFG-Zero* (Fan et al. 2025): the unconditional velocity is scaled by s = <c, u> / (<u, u> + 1e-8) per sample.
 *   zero_init_steps  the first K steps have velocity 0: no forward and no update runs, the latent stays as it is.
 *   rescale          CFG rescale (Lin et al. 2024) phi in [0, 1]: v *= phi std(c) / std(v) + 1 - phi, std over the sample; 0 = off.
 * Step i of a k5_sample* call is then one of three kinds: zero (i < zero_init_steps); unguided (|w_i - 1| <= 1e-6): the conditional forward and
 * k5_cfg_euler[_edit] without v_uncond, the bits of a run at guidance 1; guided: both forwards, then — with zero_star or rescale —
 * k5_guidance_coeffs_bf16 and k5_guided_euler, otherwise k5_cfg_euler[_edit] with w_i, so a constant weights table is the plain run bit for
 * bit.  The reduction is deterministic and every rank of a sequence-parallel group and both handles of a CFG pair hold both whole velocities, so
 * they compute identical coefficients without a further collective.  A watch's preview of a guided step shows the guided velocity.
 * The captured step (k5_dit_set_graph) is used for uniform plans — every step guided or every step unguided, no zero-init; without zero_star /
 * rescale also one weight for all steps, since k5_cfg_euler takes it by value — with w_i read from a device table; any other plan runs eagerly.
 * Refused by k5_sample* before anything is enqueued, with a message: K5_ERR_ARG num_weights != num_steps, or zero_star / rescale at a call
 * whose every weight is 1; K5_ERR_STATE a plan with guided and unguided steps or with zero-init on a handle in a CFG pair (the unconditional
 * group would have steps with nothing to exchange) or with MagCache / its calibration (the ratio table is indexed by the call of a plain
 * run), and any plan at k5_sample_windows with more than one window (one statistic per window is not the published rule);
 * K5_ERR_UNSUPPORTED zero-init together with editing; K5_ERR_ALIGN zero_star / rescale on a latent that is not a multiple of 8 elements.
 * k5_dit_set_guidance itself: K5_ERR_ARG for a weight that is not finite, weights with num_weights < 1, zero_init_steps < 0, rescale outside
 * [0, 1]; NULL clears.  k5_dit_guidance_state: whether a plan is set and how many steps of each kind the handle has enqueued under one. */
typedef struct k5_guidance {
  const float* weights; int num_weights;  /* HOST [num_steps] per-step weight, copied at set time; NULL = the call's guidance_weight at every step */
  int zero_star;                          /* CFG-Zero* projected scale */
  int zero_init_steps;                    /* first K steps: velocity 0 */
  float rescale;                          /* phi in [0,1]; 0 = off */
} k5_guidance;
int k5_dit_set_guidance(k5_dit* dit, const k5_guidance* guidance /* NULL clears */);
int k5_dit_guidance_state(k5_dit* dit, int* on, long long* guided_steps, long long* unguided_steps, long long* zero_steps, int reset);

/* Skip-layer guidance on the handle (added under ABI 11, as the exports above were): at a skip step the model runs once
 * more with the listed visual blocks disabled (mode 0: the block is the identity on the visual stream; mode 1: only its self-attention residual
 * is dropped, its cross-attention and feed-forward run) and the step's velocity is pushed away from that weakened prediction,
 *   v = v_cfg + scale * (c - c_skip)                                              (k5_euler_step_args has the rounding points)
 * with v_cfg what the step would otherwise use (CFG, the guidance plan's coefficients, or c alone at guidance 1; a plan's statistics are over c
 * and u as always, the skip term is added after them).  The skip branch is the conditional forward up to the first listed block k0, so it
 * is not run from the start: k5_dit_forward_skip is ONE conditional forward that copies its visual stream (this rank's rows, bf16) aside when
 * it reaches block k0, finishes as k5_dit_forward does (the same bits), then restores the copy and runs blocks k0.. under the skip rule and an
 * out-layer epilogue of its own (under sequence parallelism its own all-gather) into out_velocity_skip.  Text streams, the modulation vector,
 * the stacked cross-attention K/V, NAG and regional prompts are the conditional forward's.  The skip branch's blocks keep their softmax-form
 * memory in a third row, so the two other branches decide as they would without it.  Option "skip_share_prefix" 0 (diagnostic) runs every
 * non-skipped block of the skip branch from the visual embedding on.
 * A step i of k5_sample* is a skip step when this is on (scale > 0), steps == NULL or steps[i] != 0, and it is not a zero-init step.  It
 * enqueues the forking forward, the unconditional forward when guided, the plan's coefficients when it has statistics, and k5_skip_euler's
 * kernel; any other step enqueues what it always did, and so does every run while this is off.  The captured step is used only when every
 * forward-running step is of one kind.  Works with editing, k5_sample_cond, k5_sample_many, sequence-parallel groups, NABLA, fp8 and LoRA.
 * Refused by k5_sample* before anything is enqueued, with a message: K5_ERR_STATE on a handle in a CFG pair (the pair exchanges two velocities),
 * with MagCache or its calibration (the table is indexed by the calls of a plain run), at k5_sample_windows with more than one window;
 * K5_ERR_ARG when num_steps differs from the call's.
 * k5_dit_set_skip_guidance: K5_ERR_ARG for a block index outside 0..num_visual_blocks-1 or repeated, num_blocks < 1, a mode outside {0, 1}, a
 * scale that is negative or not finite, steps with num_steps < 1; scale == 0 is accepted and means off; NULL clears.  blocks and steps are
 * copied.  k5_dit_skip_state: whether it is on, the skip steps enqueued so far, and how many visual blocks the skip branches took from the
 * conditional forward (blocks_shared) and ran themselves (blocks_run). */
typedef struct k5_skip_guidance {
  const int* blocks; int num_blocks;      /* HOST, copied */
  int mode;                               /* 0 = whole block is identity on the visual stream, 1 = only its self-attention residual is dropped */
  float scale;                            /* g */
  const unsigned char* steps; int num_steps;   /* HOST per-step 0/1 mask, copied; NULL = every step */
} k5_skip_guidance;
int k5_dit_set_skip_guidance(k5_dit* dit, const k5_skip_guidance* skip /* NULL clears */);
int k5_dit_skip_state(k5_dit* dit, int* on, long long* skip_steps, long long* blocks_shared, long long* blocks_run, int reset);
/* k5_dit_forward with the skip branch: out_velocity is k5_dit_forward's bit for bit, out_velocity_skip (bf16, the same shape) the skip
 * branch's.  K5_ERR_STATE without a skip set on the handle (a set with scale 0 still forks here), with MagCache or its calibration. */
int k5_dit_forward_skip(k5_dit* dit, const k5_forward_args* args, void* out_velocity, void* out_velocity_skip, void* stream);

/* Enhance-A-Video on the handle (added under ABI 11, as the exports above were; the rule is written at k5_enhance_scores_bf16): while set,
 * every visual block's self-attention of a forward — dense or NABLA, conditional and unconditional alike, the re-run blocks of the skip
 * branch too — enqueues k5_enhance_scores_bf16 on its normalised q | k after the norm + RoPE pass (into slot `block` of a per-handle device
 * array) and k5_scale_by_dev_bf16 on the attention output in front of the out projection.  While it applies the queries are normalised by
 * the standalone pass (the normalised q must exist in memory): "attn_fuse_qnorm" is not used for those launches and k5_sample* does not take
 * the "attn_fuse_qnorm_auto" decision ("attn_fuse_qnorm_used" reports 0); the two forms give the same bits.  Under NABLA the token rows are in
 * fractal order: the engine builds frame_rows on the host per shape.  In k5_sample* step i applies it when steps == NULL or steps[i] != 0
 * (k5_dit_forward / k5_dit_forward_skip / k5_dit_forward_many: every forward); any other step, and every run while this is off, enqueues what
 * it always did.  The captured step is used only when every step is of one kind.  T is the forward's frames (a context window's length under
 * k5_sample_windows); T == 1 is accepted and inert: nothing is launched.  A forward MagCache skips launches nothing.  Each handle of a CFG pair
 * computes its own forward's scores; nothing is exchanged.  Works with k5_sample_many, editing, visual_cond, fp8 and LoRA.
 * Refused before anything is enqueued, with a message: K5_ERR_ARG when num_steps differs from the call's; K5_ERR_STATE on a rank of a
 * sequence-parallel group of any transport and sp_mode (the frames of a column live on different ranks; the cross-rank reduction is not
 * built); K5_ERR_UNSUPPORTED for T > 64.
 * k5_dit_set_enhance: K5_ERR_ARG for a negative or non-finite weight, steps with num_steps < 1; weight 0 is a valid weight (score =
 * max(1, mean T)); steps is copied; NULL clears.  k5_dit_enhance_state: whether it is on, the score launches enqueued so far (one per visual
 * block and forward), and — after a synchronisation of the last forward's stream, one small copy — the last forward's per-block scores in
 * scores[0 .. min(cap, *nblocks)) (*nblocks: num_visual_blocks once a forward applied it, 0 before); diagnostic: score 1.0 means the clamp held. */
typedef struct k5_enhance { float weight; const unsigned char* steps; int num_steps; } k5_enhance;   /* steps HOST, copied; NULL: every step */
int k5_dit_set_enhance(k5_dit* dit, const k5_enhance* enhance /* NULL clears */);
int k5_dit_enhance_state(k5_dit* dit, int* on, long long* launches, float* scores /* host [cap], nullable */, int cap, int* nblocks, int reset);

/* The forecast cache (added under ABI 11, as the exports above were): skip the visual blocks on a fixed plan of steps and extrapolate their
 * residual instead.  This is TaylorSeer (Liu et al. 2025) in its "lite" form: one residual across all visual blocks, not one per block.  The
 * plan depends on the step index alone, so nothing is decided from data: no ratio table, no host round trip, every rank decides the same.
 *
 * THE RULE.  Per handle and per branch slot (0 conditional, 1 unconditional) the state is F0 bf16 [n][D], D1 and D2 fp32 [n][D] (allocated
 * only up to the order in use), j = the step of the slot's last full call, have = the slot's full calls so far in this run, and g, gp = the
 * steps between its last two full calls and between the two before; one bf16 [n][D] buffer `ori` per handle; n = the rows this rank holds.
 *   Full call at step i: the blocks run as always; ori = the visual stream as it enters them, vis = as it leaves them.  One pass
 *   (k5_forecast_update_bf16) computes r = bf16(vis - ori) — the bits of k5_gate_sum_bf16 with a gate of -1, MagCache's residual — and, with
 *   g = fp32(i - j): if have >= 1 (and order >= 1) d1 = (float(r) - float(F0)) / g; if have >= 2 (and order >= 2) d2 = (d1 - D1) / g; then
 *   F0 = r, D1 = d1, D2 = d2, gp = g, j = i, have += 1.  vis is not written: a full call's output is the plain forward's, bit for bit.
 *   Forecast call at step i: k = i - j, m = min(order, have - 1).  The call enqueues what a call MagCache skips enqueues, and one pass
 *   (k5_forecast_apply_bf16) stands in place of the residual add: p = float(F0); if m >= 1 p = p + c1 D1; if m >= 2 p = p + c2 D2;
 *   vis = bf16(float(vis) + p), with c1 = fp32(k) and c2 = fp32(k (k + g) g / (g + gp)) passed by value.  That is Newton's backward form on
 *   the stored differences (D1 is the slope half a gap behind j, D2 the second divided difference times (g + gp) / g), so order 2 reproduces a
 *   residual that is a quadratic in the step exactly, and order 1 a linear one; with equal gaps c2 = k (k + g) / 2.  The Taylor coefficient
 *   k k / 2 on the same differences would miss a quadratic a + b i + c i^2 by c k g.
 *   Every difference, quotient, product and sum is one fp32 operation rounded on its own; nothing is contracted into an FMA.  With m = 0 the
 *   forecast is k5_gate_sum_bf16 with a gate of +1 bit for bit (MagCache's order-0 re-application).
 * The plan is full[num_steps] of 0 / 1 with full[0] = 1 (kandinsky.generation_utils.forecast_plan builds it).
 *
 * The two passes, standalone: vis bf16 [rows][ld] (D columns used; ld >= D, ld % 8 == 0), ori / F0 bf16 and D1 / D2 fp32 [rows][D], D % 8 == 0,
 * every pointer 16-byte aligned.  update reads and writes its state in place and may alias nothing else; D1 / D2 beyond min(order, have)
 * (apply: min(order, have - 1)) are neither read nor written and may be NULL; apply reads g and gp with two terms only.  K5_ERR_ARG + message,
 * before any launch: a NULL or misaligned pointer, rows < 1, D % 8, a bad ld, g < 1 (apply: g or gp < 1 with two terms), k < 1, order outside
 * 0..2, have < 0 (apply: < 1). */
int k5_forecast_update_bf16(const void* vis, int ld, const void* ori, void* F0, float* D1, float* D2, int rows, int D, int g, int order, int have,
                            void* stream);
int k5_forecast_apply_bf16(void* vis, int ld, const void* F0, const float* D1, const float* D2, int rows, int D, int k, int g, int gp, int order,
                           int have, void* stream);
/* The cache on the handle.  k5_dit_set_forecast copies the plan (full is HOST memory) and clears the history; NULL clears and frees the
 * buffers.  K5_ERR_ARG: num_steps < 1, a NULL full, full[0] == 0, order outside 0..2; K5_ERR_STATE: MagCache or its calibration is set
 * (k5_dit_set_magcache / k5_dit_set_magcache_calibrate refuse likewise while a plan is set).
 * k5_sample, k5_sample_cond, k5_sample_edit and k5_sample_many drive it themselves: step i is a full or a forecast call, as full[i] says,
 * for both of its forwards (slot 0 the conditional, slot 1 the unconditional), and the history is cleared at the start of every call and
 * sample.  On a forecast call everything inside the blocks is skipped with them (NAG, regional prompts, Enhance-A-Video, NABLA maps, fp8,
 * LoRA), as under MagCache.  Works with stochastic sampling, editing, visual_cond, a watch, and sequence-parallel groups of either transport
 * and every sp_mode (the state is the rank's own rows).  A plan without a 0 is off: the forwards are plain ones that keep no history, only
 * counted as full calls, and the captured step is used; any other plan has steps of two kinds and runs eagerly.
 * Refused by k5_sample* before anything is enqueued, with a message: K5_ERR_ARG when num_steps differs from the call's; K5_ERR_STATE with
 * skip-layer guidance (its third branch has no slot), with a guidance plan that has guided and unguided steps or zero-init (the unconditional
 * slot would have gaps), at k5_sample_windows with more than one window, and on a handle in a CFG pair.
 * k5_dit_forecast_at is the cursor for callers outside k5_sample*: the next k5_dit_forward is the call (step, slot) of the plan, and that one
 * forward consumes the cursor.  A k5_dit_forward without a cursor is a plain forward and touches no state.  A full call whose step <= j, or
 * whose n x D differs from the slot's, starts the slot's history over.  K5_ERR_STATE without a plan; K5_ERR_ARG for a step outside
 * 0..num_steps-1 or a slot outside {0, 1}.  The forward itself refuses with K5_ERR_STATE, before anything is enqueued: a forecast call whose
 * slot has have == 0, whose residual has another n x D, or whose step is not after j; a handle in a CFG pair.
 * k5_dit_forecast_state: whether a plan is set, the full and forecast calls so far, and the bytes of F0 / D1 / D2 / ori now allocated. */
typedef struct k5_forecast { int order; const unsigned char* full; int num_steps; } k5_forecast;   /* full HOST [num_steps], copied */
int k5_dit_set_forecast(k5_dit* dit, const k5_forecast* forecast /* NULL clears */);
int k5_dit_forecast_at(k5_dit* dit, int step, int slot);
int k5_dit_forecast_state(k5_dit* dit, int* on, long long* full_calls, long long* forecast_calls, long long* state_bytes, int reset);

/* Stochastic sampling on the handle (added under ABI 11, as the exports above were; the rule is written at k5_euler_step_args): while a plan is
 * set, step i of k5_sample / k5_sample_cond / k5_sample_edit takes dt_down[i] as its dt and applies k5_stochastic_euler's kernel with scale[i],
 * noise_coef[i] and stream id first_stream + i; the time the forwards see is unchanged.  The noise is generated inside the update kernel: no
 * launch is added, a zero-init step of a guidance plan still does nothing, and the launch sequence does not depend on noise_coef, so the captured
 * step replays (it reads the three values and the stream id at the device step counter).  Every rank of a sequence-parallel group and both
 * handles of a CFG pair hold the same plan and so draw the same bits, with no exchange.  Works with editing (the keep rule comes last),
 * k5_sample_cond, guidance plans, skip-layer guidance, NAG and regional prompts.
 * Refused by k5_sample* before anything is enqueued, with a message: K5_ERR_ARG when num_steps differs from the call's; K5_ERR_STATE at
 * k5_sample_windows with more than one window, at k5_sample_many, with MagCache or its calibration (the tables were measured on ODE
 * trajectories), and with a watch that has previews (the preview reads x0 = x - sigma_next v, which no longer holds after the noise is added;
 * a watch with preview_every = 0 — progress and cancel — works).
 * k5_dit_set_stochastic: the three tables are HOST [num_steps] and are copied; K5_ERR_ARG for num_steps < 1, a NULL table, a value that is not
 * finite, a noise_coef < 0; NULL clears.  k5_dit_stochastic_state: whether a plan is set and how many steps so far drew noise (noise_coef != 0,
 * not a zero-init step); counted per step by the host loop, so it is right under graph replay. */
typedef struct k5_stochastic {
  int num_steps;
  const float* dt_down; const float* scale; const float* noise_coef;   /* HOST [num_steps], copied */
  uint64_t seed; uint32_t first_stream;
} k5_stochastic;
int k5_dit_set_stochastic(k5_dit* dit, const k5_stochastic* plan /* NULL clears */);
int k5_dit_stochastic_state(k5_dit* dit, int* on, long long* noisy_steps, int reset);

/* Regional prompts on the handle (added under ABI 11; the rule is written at k5_region_combine_bf16): a prompt per masked region inside the
 * cross-attention of ONE forward.  While set, every CONDITIONAL forward (as for k5_dit_set_nag: never the unconditional one) carries R more
 * text streams: each region's tokens go through the text prologue and the text blocks as the NAG negative stream does, with their own RoPE
 * positions and the forward's own time embedding (built from the BASE prompt's pooled embedding: regions[r].pooled_embed is not read); every
 * visual block projects and normalises its queries once, attends once to the base stream and once to each region stream, and
 * k5_region_combine_bf16 joins the R + 1 outputs by the token weights in front of the out projection.  With k5_dit_set_nag also set the
 * regional blend is the positive side: it is done in place, then k5_nag_combine_bf16 runs against the negative output.  Per block that is R
 * cross-attention launches and one memory-bound pass more; the text side runs R + 1 times.  The token weights are computed by
 * k5_region_weights_f32 at most once per k5_dit_set_regions call and token order (row-major; NABLA's fractal order) and kept.  Not set, a
 * forward enqueues exactly what it always did.  `regions` (HOST [R]), what its entries point to, and `masks` (device fp32 [R][T][H][W], the
 * latent cells) are BORROWED until cleared; k5_sample* caches each region's prologue per call.  One region set serves every sample of
 * k5_sample_many.  Works on sequence-parallel shards in every sp_mode (the text is replicated, the rule is per token, a rank reads its own
 * rows of the weights: no collective is added), on the conditional handle of a CFG pair, in the captured step, under k5_sample_edit and with
 * MagCache (a skipped step runs no visual block and so no blend).
 * K5_ERR_ARG: R > 8 or < 0, base_weight outside [0, 1] or NaN, a region with text_len < 1 or a NULL text_embed / text_rope_pos, a NULL or not
 * 4-byte aligned masks, T, H or W < 1 or not divisible by the patch; later, a forward or k5_sample* whose (T, H, W) is not the masks' (the message
 * names both shapes).  K5_ERR_STATE: k5_sample_windows while regions are set (the masks cover the clip, a window sees a slice: not built).  All
 * before anything is enqueued.  R == 0 or regions == NULL clears.  k5_dit_regions_state: whether regions are on, how many, and how many combines
 * the handle has enqueued (num_visual_blocks per regional forward), optionally resetting the count. */
int k5_dit_set_regions(k5_dit* dit, const k5_text_cond* regions /* HOST [R]; NULL clears */, int R, const float* masks, int T, int H, int W,
                       float base_weight);
int k5_dit_regions_state(k5_dit* dit, int* on, int* R, long long* combines, int reset);

/* S forwards of the same (T, H, W) in one call, one after another (a convenience entry point like k5_sample_many): args->x is device fp32
 * [S][T][H][W][args->x_channels], conds HOST [S], args->time shared; out_velocity bf16 [S][T][H][W][out_visual_dim].  Sequence i is
 * k5_dit_forward(x[i], conds[i]) — the same entry point — on the handle as it was when the call began: the softmax-form memory that
 * k5_dit_forward reads and updates is put back to its state at entry before every sequence and again at the end, so the call leaves the
 * handle as it found it.  Refusals as k5_sample_many (S < 1 is K5_ERR_ARG). */
int k5_dit_forward_many(k5_dit* dit, const k5_forward_args* args, int S, const k5_text_cond* conds, void* out_velocity, void* stream);

/* Sequence parallelism (replaces the reference's DTensor head-parallel plan, kandinsky/models/parallelize.py:11-102,
 * keeps its launch contract LOCAL_RANK/WORLD_SIZE, kandinsky/utils.py:40-55): one process per GPU, rank r owns the
 * visual-token rows [r*N/world, (r+1)*N/world) (N a multiple of 64*world); K and V^T of every block are
 * all-gathered over RCCL/xGMI.  rccl_lib_path: library to dlopen (NULL/"" = default names).  Rank 0 obtains a
 * 128-byte ncclUniqueId with k5_comm_unique_id, the host broadcasts it, every rank calls k5_dit_comm_init. */
int k5_comm_unique_id(const char* rccl_lib_path, void* out_unique_id_128);
int k5_dit_comm_init(k5_dit* dit, const char* rccl_lib_path, int rank, int world, const void* unique_id_128);
/* Token counts that do not divide: whole 64-token blocks, ceil(blocks / world) per rank, the last rank takes the rest
 * (3660 blocks over 8 ranks = 7 x 458 + 454); K5_ERR_UNSUPPORTED if a rank would be left without a block.
 *
 * Loopback group (tests): `world` handles of ONE process on ONE GPU act as the ranks of a sequence-parallel run.  Every rank
 * must be driven by its own host thread (a collective is a rendezvous of the threads around device-to-device copies), and
 * every rank runs exactly the code path / offsets / launch sequence of a real multi-GPU run.  Not with k5_dit_set_graph. */
/* CFG-parallel (reference semantics: the two forwards of get_velocity, generation_utils.py:53-76): the handle runs ONE
 * branch of classifier-free guidance inside k5_sample — branch 0 the conditional forward, 1 the unconditional one — and exchanges the
 * bf16 velocity with the paired handle (the same token shard of the other rank group) once per step: a 2-rank communicator of its own,
 * initialised AFTER the sequence-parallel one (both are collective: same order on every rank).  Both handles of a pair then apply the
 * identical bf16 combine + fp32 Euler update, so all ranks of both groups hold bit-identical latents.  The exchange runs on a side
 * stream between two events and is part of the captured step under k5_dit_set_graph.  With guidance_weight == 1 the pair is idle.
 * unique_id_128: from k5_comm_unique_id on branch 0, carried to branch 1 by the host.  k5_dit_cfg_branch: 0 / 1, or -1 without a pair. */
int k5_dit_cfg_pair_init(k5_dit* dit, const char* rccl_lib_path, int branch, const void* unique_id_128);
int k5_dit_cfg_branch(k5_dit* dit);
typedef struct k5_loopback k5_loopback;
int k5_loopback_create(int world, k5_loopback** out);
void k5_loopback_destroy(k5_loopback* group);
int k5_dit_comm_init_loopback(k5_dit* dit, k5_loopback* group, int rank);
/* the CFG pair as a loopback group of world 2 (tests: 2 x P handles on one GPU = two sequence-parallel groups + P pairs) */
int k5_dit_cfg_pair_init_loopback(k5_dit* dit, k5_loopback* group, int branch);
/* IPC group (ABI 8): the second transport of the sharded path, the one SURVEY.md §8(e) names beside RCCL ("direct peer writes over xGMI into
 * IPC-mapped buffers"); same launch contract (one process per rank, kandinsky/utils.py:40-55; README.md:269-276), same schedules, same bits
 * as a loopback group of the same size.  Every rank exports its K / V^T slots, velocity and statistics buffers with hipIpcGetMemHandle on
 * first use, peers map them and READ the slices they need with a copy kernel; ordering is by epoch flags in device memory (system-scope
 * release stores / bounded polling kernels), not by host rendezvous.  Unlike RCCL it accepts several ranks on ONE device — which is how the
 * process boundary of the sharded path is exercised on a one-GPU box (bench.py --gpus P --oversubscribe; tests/test_gpu_ipc_ranks.py) —
 * and on an xGMI node it needs no library at all.  shm_name: name of a POSIX shared-memory control block, unique per group and per run
 * (the host makes one up on the group's rank 0 and broadcasts it over torch.distributed); collective over the `world` processes of the
 * group (<= 16).  Works under k5_dit_set_graph: the collectives' epochs live on the device, so the captured step replays.  Options (k5_dit_get_option): "ipc_ranks", "ipc_pair_ranks"
 * (0 = another transport), "ipc_collectives", "ipc_pulled_mb", "ipc_errors" (synchronises; first flag wait that hit K5_IPC_TIMEOUT_S). */
int k5_dit_comm_init_ipc(k5_dit* dit, const char* shm_name, int rank, int world);
int k5_dit_cfg_pair_init_ipc(k5_dit* dit, const char* shm_name, int branch);
/* Engine options by name (all default 0): "attn_mode" 0 = softmax form per head from the data, 1 = online max everywhere;
 * "sp_pass1_tiles" local key tiles attended before the K / V^T gather has landed (0 = all); "emulate_world" P = TIMING
 * ONLY: rank 0's share of a P-rank run on a world = 1 communicator — collectives move nothing, results are garbage and
 * k5_dit_get_option("emulated") reads 1 so that a bench can refuse the number. */
int k5_dit_set_option(k5_dit* dit, const char* name, int value);
int k5_dit_get_option(k5_dit* dit, const char* name, int* value);
/* Self-tuning sequence-parallel schedule (replaces the fixed plan of parallelize_dit, kandinsky/models/parallelize.py:11-102, and the
 * launcher's world-size bookkeeping, kandinsky/utils.py:40-55).  Which exchange is fastest — one in-place K / V^T all-gather per block,
 * the same exchange in 2 slices, the Ulysses all-to-all (heads % ranks == 0); for NABLA one or two passes over the lists — depends on
 * the node.  The first sharded forward of a handle with more than one rank therefore times one block's self-attention section under
 * every admissible candidate on its own shapes; the ranks exchange their times, each candidate costs its slowest rank, the cheapest is
 * kept for the life of the handle (every rank decides alike from the same table).  Options set explicitly through k5_dit_set_option
 * ("sp_mode", "sp_slices", "sp_nabla_passes") are left alone, and a tuning run only assigns the options it varied (dense: "sp_mode" /
 * "sp_slices"; NABLA: "sp_nabla_passes").  The tuner is OPT-IN ("sp_autotune" 1; K5_SP_AUTOTUNE=1): its choice comes from timings and the
 * schedules sum in different orders, so with it on the same seed may give different bits on two nodes; off (the default) a handle runs the
 * all-gather schedule.  2 makes the next sharded forward tune again.  k5_dit_sp_schedule: JSON text of what was measured and chosen, incl. the bare gather's
 * bytes and GB/s ("{}" before the first tuning run); returns the text length, copies at most len - 1 characters + NUL (buf may be null).
 * k5_sp_pick_schedule: the selection rule alone (host arithmetic, no GPU): times[rank * ncand + cand] in ms, <= 0 / non-finite = did not
 * run on that rank; valid (nullable) masks candidates; returns the chosen candidate or -1, max-over-ranks per candidate in cost_out. */
/* Two-level sequence parallelism (ABI 10; "sp_mode" 2, or K5_SP_MODE=2 in the environment of the ranks at communicator init — an explicit
 * k5_dit_set_option still wins): G = gcd(heads, ranks) head groups x ranks / G query splits, for rank counts that do not divide the heads
 * (28 heads at 6 or 8 ranks).  Rank r attends head group r % G for the queries of the G consecutive token shards of ranks (r / G) G ..
 * (r / G) G + G - 1 against all keys, in one pass; k' and V^T reach every rank by one exchange over the whole world, q and the attention
 * output change hands inside the split.  G = ranks runs Ulysses ("sp_mode" 1), G = 1 and NABLA the all-gather; "sp_mode_used" (read-only)
 * says which schedule the last sharded forward ran (0 gather, 1 Ulysses, 2 two-level; -1 none yet).  The q | k | V^T projections stay bf16.
 * k5_sp_plan_2d: the exchange plan every rank derives from (heads, ranks, rows_pad, dim), host arithmetic only.  which: 0 k', 1 V^T, 2 q,
 * 3 attention output; table (nullable) gets ranks x ranks entries of three int64, table[(src * ranks + dst) * 3 + {0, 1, 2}] = offset in
 * src's send buffer, offset in dst's receive buffer, bytes (0 = nothing between the two).  Returns the schedule "sp_mode" 2 runs at
 * (heads, ranks) — 2 two-level, 1 Ulysses, 0 gather — with G in *groups (nullable), or -K5_ERR_ARG. */
int k5_sp_plan_2d(int heads, int ranks, int rows_pad, int dim, int which, int* groups, long long* table);
int k5_dit_sp_schedule(k5_dit* dit, char* buf, int len);
int k5_sp_pick_schedule(const float* times, int ncand, int world, const int* valid, float* cost_out);
/* (block, head) self-attention launches that took the fixed-offset / the online-max softmax since the last reset. */
int k5_dit_attn_variant_counts(k5_dit* dit, long long* fixed_heads, long long* online_heads, int reset);
/* kept / possible 64x64 blocks of the NABLA maps computed while profiling was on, since that reset (realised density). */
int k5_dit_nabla_block_counts(k5_dit* dit, long long* kept, long long* possible);
/* Diagnostics (ABI 7): while a tap is set, every NABLA map the handle computes on the one-GPU path — one per visual block and forward, in execution
 * order — is expanded to uint8 [H][N/64][N/64] (1 = kept; row = query block, fractal order) behind the ones already taken in the caller's device
 * buffer, as long as it fits; k5_dit_nabla_tap_count: maps computed since the tap was set (a count beyond capacity / map size = the buffer was
 * too small).  dev_u8 = NULL removes the tap.  Lets a test put the engine's map of block b at step s next to the reference's own
 * (nablaT_v2, kandinsky/models/utils.py:136-163, as nn.py:257-298 calls it inside every block): tests/test_gpu_fulldepth.py. */
int k5_dit_set_nabla_tap(k5_dit* dit, void* dev_u8, long long capacity_bytes);
int k5_dit_nabla_tap_count(k5_dit* dit, long long* maps);
/* ... and the blocks the list-driven attention executed for those maps (one-GPU path): the rows of a workgroup share ONE key-tile list, the
 * union of what they selected (replaces flex_attention's per-row block walk, nn.py:257-280), so a row also steps over tiles only its
 * neighbours wanted; kept / executed is the launch's union efficiency. */
int k5_dit_nabla_executed_blocks(k5_dit* dit, long long* executed);

/* ------------------------------------------------------------------------------------------
 * HunyuanVideo 3D-VAE decoder (kandinsky/models/vae.py): post_quant_conv + HunyuanVideoDecoder3D.forward
 * (vae.py:684-696, 870) on one latent tile; the tiling policy (vae.py:847-1204) stays on the host mirror.
 * ---------------------------------------------------------------------------------------- */
/* HunyuanVideoCausalConv3d (vae.py:125-163, k=3, replicate pad W(1,1) H(1,1) T(2,0)) with the nearest upsample of
 * HunyuanVideoUpsampleCausal3D (vae.py:187-205) optionally folded in (up_t, up_s in {1,2}); channels-last bf16:
 * X [Ts][Hs][Ws][Cin] (Cin % 64 == 0), W [Cout][27][Cin] (tap = (dt*3+dh)*3+dw), bias fp32, out [To*Ho*Wo][ldc];
 * resid (optional) [To*Ho*Wo][ldr]: out = bf16(bf16(conv+bias) + resid) (resnet skip, vae.py:274). */
int k5_conv3d_bf16(const void* X, const void* W, const float* bias, void* out, int Ts, int Hs, int Ws, int Cin, int Cout,
                   int up_t, int up_s, int ldc, const void* resid, int ldr, void* stream);
/* HunyuanVideoDownsampleCausal3D (vae.py:208-227; encoder): the same causal conv with an output stride st_t, st_s in {1, 2}
 * and padding 0: out [To*Ho*Wo][ldc], To = (Ts-1)/st_t + 1, Ho = (Hs-1)/st_s + 1, Wo = (Ws-1)/st_s + 1. */
int k5_conv3d_strided_bf16(const void* X, const void* W, const float* bias, void* out, int Ts, int Hs, int Ws, int Cin, int Cout,
                           int st_t, int st_s, int ldc, void* stream);
/* nn.GroupNorm(G, C, eps) (+SiLU) on channels-last bf16 rows [M][C] (vae.py:246-263,672-673): one-pass statistics (sums of
 * x and x^2: fp32 over 4 rows, double beyond), fp32 normalisation, bf16 out.  workspace: device scratch of k5_groupnorm_workspace_size(M, G) bytes. */
int64_t k5_groupnorm_workspace_size(int M, int G);
int k5_groupnorm_bf16(const void* x, const float* gamma, const float* beta, void* out, int M, int C, int G, float eps,
                      int silu, void* workspace, void* stream);

/* The production pairing of the two (vae.py:246-263: GroupNorm -> SiLU -> conv, the norm reading what the previous conv wrote): the
 * conv also emits the GroupNorm statistics of the outputs it STORES — per 128 rows and 4 consecutive channels (sum, sum of squares),
 * quad_stats: k5_conv3d_stats_size(M, Cout) bytes, M = To*Ho*Wo — and k5_groupnorm_bf16_quads normalises from them without a
 * statistics pass of its own (workspace as for k5_groupnorm_bf16).  Only the 4-wave implicit-GEMM kernel emits statistics:
 * K5_ERR_UNSUPPORTED (nothing launched) outside its range (Cin % 128, Cout = 128 or % 256, >= 5/8 of a round of 256-row tiles);
 * K5_ERR_ARG (nothing launched) for an extent < 1 or a factor outside {1, 2}.
 * quad_stats is [2 ceil(M / 256)][Cout / 4][2] fp32; rows past M count nothing.  Statistics block b holds output rows 128 b .. 128 b + 127,
 * except where the output frames split into whole 8 x 32 patches (Ho % 8 == 0 and Wo % 32 == 0): there blocks 2 j and 2 j + 1 are the upper
 * and the lower four pixel rows of patch j (frame-major, then row-major over the patches).  A consumer that folds all blocks need not care. */
int64_t k5_conv3d_stats_size(int M, int Cout);
int k5_conv3d_bf16_stats(const void* X, const void* W, const float* bias, void* out, int Ts, int Hs, int Ws, int Cin, int Cout,
                         int up_t, int up_s, int ldc, const void* resid, int ldr, float* quad_stats, void* stream);
int k5_groupnorm_bf16_quads(const void* x, const float* gamma, const float* beta, void* out, int M, int C, int G, float eps,
                            int silu, const float* quad_stats, void* workspace, void* stream);

typedef struct k5_vae k5_vae;
typedef struct k5_vae_config {   /* AutoencoderKLHunyuanVideo.__init__ kwargs, vae.py:709-731 */
  int latent_channels, out_channels;
  int block_out_channels[4];
  int layers_per_block, norm_num_groups;
} k5_vae_config;
int k5_vae_create(const k5_vae_config* cfg, k5_vae** out);
void k5_vae_destroy(k5_vae* vae);
/* checkpoint tensors by state_dict key (decoder.*, post_quant_conv.*; encoder.*, quant_conv.* enable k5_vae_encode_tile;
 * other keys are ignored), host or device ptr */
int k5_vae_load_tensor(k5_vae* vae, const char* key, const void* ptr, int dtype, const int64_t* shape, int rank);
int k5_vae_finalize(k5_vae* vae);
/* z: device fp32 (latent_channels,T,H,W) (already divided by scaling_factor, generation_utils.py:220) ->
 * out: device bf16 (out_channels, 4(T-1)+1, 8H, 8W) = self.decoder(self.post_quant_conv(z)) */
int k5_vae_decode_tile(k5_vae* vae, const float* z, int T, int H, int W, void* out, void* stream);
/* (ABI 8) the same with z read IN PLACE out of a longer latent: z_channel_stride = elements between the latent channels of z (0 = T*H*W), i.e. the
 * temporal slice z[:, :, t0 : t0 + T] of the tiling loop (vae.py:1144-1204 `_temporal_tiled_decode`) without a copy */
int k5_vae_decode_tile_strided(k5_vae* vae, const float* z, int64_t z_channel_stride, int T, int H, int W, void* out, void* stream);
/* Encoder half (SURVEY.md §8 f4 — image / video conditioning): quant_conv(HunyuanVideoEncoder3D.forward(x)) on ONE tile
 * (vae.py:574-586, 808-809); the tiling policy (tiled_encode :938-1010, _temporal_tiled_encode :1096-1142) stays on the
 * host mirror.  Needs the encoder.* / quant_conv.* tensors (k5_vae_has_encoder = 1; a decode-only load leaves them out).
 * x: device fp32 (3, T, H, W), T = 4k+1 frames, H, W multiples of 8 -> out: device bf16 (2*latent_channels, k+1, H/8, W/8)
 * = the moments [mean | logvar] the reference hands to DiagonalGaussianDistribution. */
int k5_vae_encode_tile(k5_vae* vae, const float* x, int T, int H, int W, void* out, void* stream);
int k5_vae_has_encoder(k5_vae* vae);
/* Diagnostics: launches per kernel route since the last reset — out8 = {conv on 128x128 tiles, conv 4-wave, conv 4-wave + GroupNorm
 * statistics, conv_out3, GroupNorm from the conv's statistics, GroupNorm with its own statistics pass, mid attention in one kernel
 * (C = 512), mid attention as GEMM-softmax-GEMM}.  Lets a parity test assert that the kernels the timed decode runs are the ones it
 * checked (tests/test_gpu_vae.py::test_production_tile_vs_reference_golden). */
int k5_vae_path_counts(k5_vae* vae, long long* out8, int reset);
/* blend_t / blend_v / blend_h (vae.py:908-936) on contiguous bf16 tensors viewed as [outer][len][inner]:
 * b[:, y, :] = a[:, len_a-extent+y, :]*(1-y/extent) + b[:, y, :]*(y/extent), y < extent (eager bf16 rounding) */
int k5_blend_bf16(const void* a, void* b, int64_t outer, int len_a, int len_b, int64_t inner, int extent, void* stream);
/* (ABI 8) blend_t + `tile[:, :, :keep]` + the `torch.cat` of `_temporal_tiled_decode` (vae.py:1185-1204) as ONE pass: views [outer][len][inner] with
 * explicit outer strides in elements (a decoded tile minus its first frame; the output video); dst[:, y] = y < extent ? the cross-fade of k5_blend_bf16
 * (a[:, len_a - extent + y], b[:, y]) : b[:, y], y < keep.  a = NULL: no cross-fade (the first tile).  inner a multiple of 8, 16-byte aligned pointers.
 * Neither a nor b is written: the previous tile's tail is read as the decoder left it, which is what the reference blends with while tiles are at
 * least 2 * extent long (the host mirror falls back to k5_blend_bf16 otherwise).  (ABI 11) len_b: the frames of b from the passed pointer on;
 * K5_ERR_ARG before any launch when keep > len_b, extent > len_b, extent > len_a or extent > keep. */
int k5_blend_place_bf16(const void* a, int64_t a_stride, int len_a, const void* b, int64_t b_stride, int len_b, void* dst, int64_t dst_stride,
                        int64_t outer, int64_t inner, int extent, int keep, void* stream);
/* (ABI 8) the pipeline's uint8 frames, ((x.clamp(-1, 1) + 1) * 127.5).to(torch.uint8) (reference generation_utils.py:222-224) in one pass with torch's
 * bf16 rounding after every elementwise op and the truncating conversion; n a multiple of 8 */
int k5_frames_to_uint8(const void* x_bf16, void* out_u8, int64_t n, void* stream);

/* fp8 (OCP e4m3) W8A8 GEMM, opt-in (BASELINE config 5 "fp8 MFMA weights"): C = epilogue(w_scale[n] * A8 . W8^T) with fp32
 * accumulation on v_mfma_scale_f32_16x16x128_f8f6f4.  A8 [M][lda] and W8 [N][ldw] are fp8 bytes (K a multiple of 128, >= 256,
 * rows 16-byte aligned).  epi: K5_EPI_BIAS -> C bf16 (no bias term: the feed-forward layers have none, nn.py:352-361);
 * K5_EPI_GELU -> C fp8 = e4m3(GELU(bf16(.))) (the input of the second feed-forward GEMM); K5_EPI_GATE -> gated residual as
 * k5_gemm_bf16.  k5_quant_rows_fp8: x bf16 [rows][K] -> e4m3 with a per-row scale max|x|/448 written to `scale`, or with the
 * static scale 1 when scale == NULL (activations).  This is a LOSSY mode (3 mantissa bits per operand); the engine uses it
 * only after k5_dit_set_fp8(dit, 1). */
int k5_gemm_fp8(const void* A8, const void* W8, const float* w_scale, void* C, int M, int N, int K, int lda, int ldw, int ldc,
                int epi, const void* resid, int ldr, const float* gate, void* stream);
/* (added under ABI 11) k5_gemm_fp8 with the launcher's two remaining arguments, as the engine's q | k | V^T projections use them: `bias` (nullable)
 * is fp32 per output column n and is added to acc * w_scale in one fma; scale_m != 0 is the operand-swapped form (weights as the A8 rows, tokens
 * as N) where w_scale and bias are indexed by the output ROW m — K5_EPI_BIAS only, K5_ERR_ARG otherwise.  bias == NULL and scale_m == 0 is
 * k5_gemm_fp8, bit for bit. */
int k5_gemm_fp8_ex(const void* A8, const void* W8, const float* w_scale, void* C, int M, int N, int K, int lda, int ldw, int ldc,
                   int epi, const void* resid, int ldr, const float* gate, void* stream, const float* bias, int scale_m);
int k5_quant_rows_fp8(const void* x_bf16, void* out_fp8, float* scale, int rows, int K, int ldx, int ldo, void* stream);

/* Run linear layers of the visual blocks in W8A8 e4m3 (weights quantised per output channel on first enable, activations with the
 * static scale 1).  `enabled` is a bit mask: 1 = the feed-forward GEMMs (nn.py:352-361), 2 = the q | k | V^T projections and 4 = the out
 * projection of the visual self-attention (nn.py:233-244, 282-284); 0 = off.  LOSSY and off by default: the distance to the bf16 path per
 * layer class is stated with the parity test tests/test_gpu_dit.py::test_fp8_feed_forward_mode and in DESIGN.md §4.2; from 256 tiles up the
 * GEMMs run on the four-wave e4m3 kernel (gemm_fp8.hip, round 4).  The sequence-parallel schedules keep the out projection in bf16 and the Ulysses
 * schedule also the q | k | V^T projections: k5_dit_get_option(dit, "fp8_effective") returns the mask that is in effect on the handle's path. */
int k5_dit_set_fp8(k5_dit* dit, int enabled);

/* LoRA adapters on a finalized handle (added under ABI 11): merged in place into the packed weights, and undone.
 * k5_dit_add_lora: `key` is a state_dict weight key with a rank-2 tensor; B is [rows][R] and A is [R][cols] for that key's
 * [rows][cols], host or device pointers of dtype K5_F32 / K5_BF16 / K5_F16.  The packed buffer the key went into receives k5_lora_merge:
 * self-attention to_query / to_key = rows 0..D-1 / D..2D-1 of the fused q|k buffer; cross-attention to_key / to_value = that block's rows of
 * the stacked buffers; visual_embeddings.in_layer with its padded leading dimension; time_embeddings.* and every *modulation.out_layer in
 * fp32 (no rounding), the latter at their rows of the stacked modulation matrix.  The first merge into a matrix saves its packed bits in a
 * device backup; later calls merge onto the current bits, one rounding per call, in call order.
 * k5_dit_clear_lora copies every backup back and frees it: the handle then gives the bits it gave before the first k5_dit_add_lora.
 * k5_dit_lora_state: matrices with a live backup and the bytes the backups hold.
 * add and clear run on the null stream and end with a device synchronise (a one-time operation, as finalize); no pointer moves, so a captured
 * step stays valid.  They also drop what was computed from the old weights: the text prologue cache, the softmax-form memory, the MagCache
 * counter and residuals (and a calibration's), and they re-make the e4m3 copy and scales of a touched matrix that has one (k5_dit_set_fp8).
 * Handles of a sequence-parallel group or a CFG pair are accepted: weights are replicated, every rank makes the same calls.
 * Refused with a message and nothing enqueued: before finalize K5_ERR_STATE; unknown key K5_ERR_KEY; a bias or norm key K5_ERR_UNSUPPORTED;
 * R outside 1..256, a bad dtype or a null pointer K5_ERR_ARG. */
int k5_dit_add_lora(k5_dit* dit, const char* key, const void* A, int a_dtype, const void* B, int b_dtype, int R, float scale);
int k5_dit_clear_lora(k5_dit* dit);
int k5_dit_lora_state(k5_dit* dit, int* matrices_touched, long long* backup_bytes);

/* k5_sample replays ONE hipGraph-captured sampler step (forwards + CFG/Euler, per-step scalars read from device tables at a
 * device-side step counter) instead of launching ~500 kernels per step from the host; results are bit-identical.  Ignored
 * while MagCache or profiling is on, and for fewer than 3 steps. */
int k5_dit_set_graph(k5_dit* dit, int enabled);

/* MagCache — replaces `set_magcache_params` + `magcache_forward` (reference kandinsky/magcache_utils.py:16-101).
 * `ratio_table` holds 2*num_steps float64 ratios (cond/uncond interleaved, already extended by the two leading 1.0 and
 * nearest-interpolated as :29-39 does — the host mirror kandinsky/magcache_utils.py does that); table_len == 0
 * disables.  Afterwards every k5_dit_forward / k5_sample forward runs the reference's decision: after the first
 * `retention_ratio` of the calls, skip the visual blocks and re-apply the cached bf16 residual of the call's slot
 * (call parity) while the accumulated |1 - prod ratio| < thresh for at most K consecutive calls.  no_cfg: the call
 * counter advances by 2 (slot 0 only), :91-94.  Defaults of the reference: thresh 0.12, K 2, retention_ratio 0.2. */
int k5_dit_set_magcache(k5_dit* dit, const double* ratio_table, int table_len, int no_cfg, double thresh, int K,
                        double retention_ratio);
/* Which calls of the reference's call sequence (cond, uncond, cond, ...) this handle executes: call indices
 * first_call, first_call + stride, ...  set_magcache installs (0, 1), or (0, 2) with no_cfg.  CFG-parallel rank groups
 *  run one branch each: conditional group (0, 2), unconditional group (1, 2). */
int k5_dit_magcache_calls(k5_dit* dit, int first_call, int stride);
/* introspection: current call counter and how many forwards ran / skipped the visual blocks since set_magcache */
int k5_dit_magcache_state(k5_dit* dit, int* cnt, long long* n_ran, long long* n_skipped);

/* MagCache calibration: measure the ratio table k5_dit_set_magcache consumes.  num_steps > 0 switches it on (num_steps == 0: off, the
 * buffers and the table are freed).  While it is on every forward runs its visual blocks (nothing is ever skipped) under MagCache's call counter
 * and slot rule (slot = cnt & 1; cnt advances by 1, by 2 with no_cfg, and wraps at 2 * num_steps) and leaves, in a device table
 * double[2 * num_steps][4] indexed by the call counter, the four sums of k5_magcache_stats_bf16 of the call's residual
 * bf16(visual_embed_out - visual_embed_in) against the previous residual of its slot.  A slot's first call of a run (cnt < 2) has no previous
 * residual and contributes nothing.  Nothing is copied to the host inside k5_sample; a second run over the same handle ADDS to the table (several
 * prompts / seeds are averaged by dividing the sums).  The final latent is bit-identical to a plain run's.  Memory: two residual buffers
 * (previous, current) of n x D bf16 per slot.  Graph replay is ignored while calibrating, as under MagCache.
 * Refused with K5_ERR_STATE, before anything is enqueued: together with k5_dit_set_magcache (either order), and on a handle in a
 * sequence-parallel group or a CFG pair of any transport — calibration is an offline one-GPU job (the 10 s clip fits one card), and per-rank
 * partial sums would need a reduction in rank order to stay repeatable.  k5_sample_many / k5_dit_forward_many refuse a calibrating handle as
 * they refuse MagCache.  A forward whose n x D differs from the previous call of its slot in the same run is K5_ERR_ARG. */
int k5_dit_set_magcache_calibrate(k5_dit* dit, int num_steps, int no_cfg);
/* Synchronises the stream of the handle's last forward, copies min(cap_rows, 2 * num_steps) rows of the table to out (host, [rows][4]:
 * sum rho, sum rho^2, sum (1 - cos), rows counted) and reports *rows = 2 * num_steps and *runs = complete runs (counter wrap-arounds)
 * the table holds.  out == NULL only reports.  K5_ERR_STATE when calibration is off. */
int k5_dit_magcache_calibration(k5_dit* dit, double* out, int cap_rows, int* rows, long long* runs);

/* per-kernel-family accumulated GPU time of the last forward(s), measured with hipEvents on the
 * engine's stream when profiling is enabled.  names: "attn_self","attn_cross","gemm","elementwise",...
 * level 0 = off, 1 = every family (an event pair per family switch: ~15 per block, the stream drains at each one),
 * 2 = only "attn_self", the roofline kernel (one pair per block) — what bench.py keeps on inside its timed region.
 * The pseudo-family "self_blocks" returns (0 ms, the number of visual blocks whose self-attention ran while profiling was on):
 * a block's attention is 1 timed scope on one GPU, 2 under sequence parallelism, 1 + S with a sliced exchange — FLOPs are per block. */
int k5_dit_set_profiling(k5_dit* dit, int level);
int k5_dit_get_profile(k5_dit* dit, const char* family, double* total_ms, int64_t* launches);
int k5_dit_reset_profile(k5_dit* dit);

#ifdef __cplusplus
}
#endif
#endif /* K5_H */
