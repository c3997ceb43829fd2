// k5_api.hip — kernel-level entry points of the C ABI (include/k5.h): thin extern "C" shims over the
// C++ launchers so that parity tests and host glue can call every kernel with raw device pointers.
#include "k5_kernels.h"

void k5_set_error(const char* fmt, ...);

static int ret(int st, const char* what) {
  if (st != K5_OK) {
    const hipError_t e = hipGetLastError();
    k5_set_error("%s: status %d (%s)", what, st, e == hipSuccess ? "argument/alignment" : hipGetErrorString(e));
  }
  return st;
}

// the tensors and their geometry, which every attention entry point passes on as it got them
template <class A>
static A attn_args(const void* Q, const void* K, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq, int ldk, int ldvt, int ldo,
                   void* stream) {
  A a;
  a.Q = Q; a.K = K; a.Vt = Vt; a.O = O;
  a.H = H; a.q_len = q_len; a.kv_len = kv_len; a.ldq = ldq; a.ldk = ldk; a.ldvt = ldvt; a.ldo = ldo;
  a.stream = (hipStream_t)stream;
  return a;
}

extern "C" {

int k5_gemm_bf16(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int lda, int ldw,
                 int ldc, int epilogue, const void* resid, int ldr, const float* gate, void* stream) {
  return ret(k5_launch_gemm_bf16(A, W, bias, C, M, N, K, lda, ldw, ldc, epilogue, resid, ldr, gate, (hipStream_t)stream),
             "k5_gemm_bf16");
}

int k5_gemm_bf16_variant(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int lda, int ldw,
                         int ldc, int epilogue, const void* resid, int ldr, const float* gate, void* stream, int kernel, int token_tile) {
  if (token_tile != 0 && token_tile != 128 && token_tile != 192 && token_tile != 256) return ret(K5_ERR_ARG, "k5_gemm_bf16_variant");
  return ret(k5_launch_gemm_bf16(A, W, bias, C, M, N, K, lda, ldw, ldc, epilogue, resid, ldr, gate, (hipStream_t)stream, kernel, token_tile / 32),
             "k5_gemm_bf16_variant");
}

int k5_causal_softmax_bf16(const float* scores, void* P, int S, int hw, int lds, int ldp, void* stream) {
  if (!scores || !P || lds < S) return K5_ERR_ARG;
  return ret(k5_launch_causal_softmax(scores, P, S, hw, lds, ldp, (hipStream_t)stream), "k5_causal_softmax_bf16");
}

int k5_vae_attention512_bf16(const void* q, const void* k, const void* vt, void* o, int S, int hw, int ldqk, int ldvt, int ldo,
                             float scale, void* stream) {
  return ret(k5_launch_vae_attention512(q, k, vt, o, S, hw, ldqk, ldvt, ldo, scale, (hipStream_t)stream), "k5_vae_attention512_bf16");
}

int k5_gemm_bf16_f32out(const void* A, const void* W, float* C, int M, int N, int K, int lda, int ldw, int ldc, float alpha,
                        int causal_hw, void* stream) {
  return ret(k5_launch_gemm_bf16_f32out(A, W, C, M, N, K, lda, ldw, ldc, alpha, causal_hw, (hipStream_t)stream), "k5_gemm_bf16_f32out");
}

int k5_attention_bf16(const void* Q, const void* K, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                      int ldk, int ldvt, int ldo, void* stream) {
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, K, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16");
}

int64_t k5_attention_state_size(int H, int q_len) { return (int64_t)k5_attention_state_bytes(H, q_len); }

int k5_attention_bf16_range(const void* Q, const void* K, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                            int ldk, int ldvt, int ldo, float score_bound, int tile_off0, int tile_cnt, int tile_skip_at,
                            int tile_skip_n, void* state, int flags, void* stream) {
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, K, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  a.score_bound = score_bound;
  a.tile_off0 = tile_off0; a.tile_cnt = tile_cnt; a.tile_skip_at = tile_skip_at; a.tile_skip_n = tile_skip_n;
  a.state = (float*)state; a.flags = flags;
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16_range");
}

int k5_gemm_fp8(const void* A8, const void* W8, const float* w_scale, void* C, int M, int N, int K, int lda, int ldw, int ldc, int epi,
                const void* resid, int ldr, const float* gate, void* stream) {
  return ret(k5_launch_gemm_fp8(A8, W8, w_scale, C, M, N, K, lda, ldw, ldc, epi, resid, ldr, gate, (hipStream_t)stream), "k5_gemm_fp8");
}

int k5_gemm_fp8_ex(const void* A8, const void* W8, const float* w_scale, void* C, int M, int N, int K, int lda, int ldw, int ldc, int epi,
                   const void* resid, int ldr, const float* gate, void* stream, const float* bias, int scale_m) {
  return ret(k5_launch_gemm_fp8(A8, W8, w_scale, C, M, N, K, lda, ldw, ldc, epi, resid, ldr, gate, (hipStream_t)stream, bias, scale_m),
             "k5_gemm_fp8_ex");
}

int k5_quant_rows_fp8(const void* x, void* out, float* scale, int rows, int K, int ldx, int ldo, void* stream) {
  return ret(k5_launch_quant_rows_fp8(x, out, scale, rows, K, ldx, ldo, (hipStream_t)stream), "k5_quant_rows_fp8");
}

int k5_attention_bf16_prescaled(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                int ldk, int ldvt, int ldo, float score_bound, void* stream) {
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, Kc, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  a.score_bound = score_bound; a.k_prescaled = true;
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16_prescaled");
}

int k5_attention_bf16_prescaled_auto(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                     int ldk, int ldvt, int ldo, const int* head_flags, int variant, void* workspace, void* stream) {
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, Kc, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  a.balance_ws = (float*)workspace; a.k_prescaled = true; a.head_flags = head_flags; a.variant = variant;
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16_prescaled_auto");
}

int k5_attention_flags(float* qstat, float* kstat, int nk, int kstride, int H, int force_online, int* flags, void* stream) {
  return ret(k5_launch_attn_flags(qstat, kstat, nk, kstride, H, force_online, flags, nullptr, (hipStream_t)stream), "k5_attention_flags");
}

// the same two with per-row offsets: k5_attention_flags_rows also writes kmax[H] and keeps heads up to a bound of 190 on the fixed
// form; k5_attention_bf16_prescaled_rows runs them with it (head_flags is read AND, on a late fallback, written)
int k5_attention_flags_rows(float* qstat, float* kstat, int nk, int kstride, int H, int force_online, int* flags, float* kmax, void* stream) {
  if (!kmax) return ret(K5_ERR_ARG, "k5_attention_flags_rows");
  return ret(k5_launch_attn_flags(qstat, kstat, nk, kstride, H, force_online, flags, nullptr, (hipStream_t)stream, kmax), "k5_attention_flags_rows");
}
// centred per-row offsets (K5KeyCentre): rstat = squared radii of the keys around `centre` (consumed), krad out
int k5_attention_flags_rows_centred(float* qstat, float* kstat, int nk, int kstride, int H, int force_online, int* flags, float* kmax, float* rstat,
                                    float* krad, void* stream) {
  if (!kmax || !rstat || !krad) return ret(K5_ERR_ARG, "k5_attention_flags_rows_centred");
  return ret(k5_launch_attn_flags(qstat, kstat, nk, kstride, H, force_online, flags, nullptr, (hipStream_t)stream, kmax, nullptr, rstat, krad),
             "k5_attention_flags_rows_centred");
}
int k5_attention_bf16_prescaled_rows_centred(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                             int ldk, int ldvt, int ldo, int* head_flags, const float* kmax, const float* centre, const float* krad,
                                             void* workspace, void* stream) {
  if (!head_flags || !kmax || !centre || !krad) return ret(K5_ERR_ARG, "k5_attention_bf16_prescaled_rows_centred");
  const K5KeyCentre kc{centre, krad};
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, Kc, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  a.balance_ws = (float*)workspace; a.k_prescaled = true; a.head_flags = head_flags; a.row_offset_kmax = kmax; a.key_centre = &kc;
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16_prescaled_rows_centred");
}
// anchored offsets for the heads beyond the window (include/k5.h): flags with the marker, the offsets, the attention that reads them
int k5_attention_flags_rows_anchored(float* qstat, float* kstat, int nk, int kstride, int H, int force_online, int* flags, float* kmax, float* rstat,
                                     float* krad, const int* prefer_online, void* stream) {
  if (!kmax || !rstat || !krad) return ret(K5_ERR_ARG, "k5_attention_flags_rows_anchored");
  return ret(k5_launch_attn_flags(qstat, kstat, nk, kstride, H, force_online, flags, nullptr, (hipStream_t)stream, kmax, prefer_online, rstat, krad, 1, 0, true),
             "k5_attention_flags_rows_anchored");
}
int k5_attention_row_anchor(const void* Q, const void* Kc, int H, int q_len, int kv_len, int ldq, int ldk, int key0, int kv_total, const float* kmax,
                            float* anchor, void* stream) {
  return ret(k5_launch_attn_row_anchor(Q, Kc, H, q_len, kv_len, ldq, ldk, key0, kv_total, kmax, anchor, (hipStream_t)stream), "k5_attention_row_anchor");
}
int k5_attention_bf16_prescaled_rows_anchored(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                              int ldk, int ldvt, int ldo, int* head_flags, const float* kmax, const float* centre, const float* krad,
                                              const float* anchor, void* workspace, void* stream) {
  if (!head_flags || !kmax || !centre || !krad || !anchor) return ret(K5_ERR_ARG, "k5_attention_bf16_prescaled_rows_anchored");
  const K5KeyCentre kc{centre, krad, anchor};
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, Kc, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  a.balance_ws = (float*)workspace; a.k_prescaled = true; a.head_flags = head_flags; a.row_offset_kmax = kmax; a.key_centre = &kc;
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16_prescaled_rows_anchored");
}
int k5_attention_bf16_prescaled_rows(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                     int ldk, int ldvt, int ldo, int* head_flags, const float* kmax, void* workspace, void* stream) {
  if (!head_flags || !kmax) return ret(K5_ERR_ARG, "k5_attention_bf16_prescaled_rows");
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, Kc, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  a.balance_ws = (float*)workspace; a.k_prescaled = true; a.head_flags = head_flags; a.row_offset_kmax = kmax;
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16_prescaled_rows");
}

// one pass of a multi-pass schedule with per-row offsets (what the sequence-parallel engine runs): key tiles tile_off0 .. +tile_cnt,
// flags & 1 resume / & 2 leave the state, late_pass 1 = not the last pass, 2 = the last (see include/k5.h)
int k5_attention_bf16_prescaled_rows_pass(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                          int ldk, int ldvt, int ldo, int* head_flags, const float* kmax, int tile_off0, int tile_cnt,
                                          float* state, int flags, int late_pass, void* workspace, void* stream) {
  if (!head_flags || !kmax) return ret(K5_ERR_ARG, "k5_attention_bf16_prescaled_rows_pass");
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, Kc, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  a.balance_ws = (float*)workspace; a.k_prescaled = true; a.head_flags = head_flags; a.row_offset_kmax = kmax;
  a.tile_off0 = tile_off0; a.tile_cnt = tile_cnt; a.state = state; a.flags = flags; a.late_pass = late_pass;
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16_prescaled_rows_pass");
}

// the same pass with norm_qk + apply_rotary of the QUERIES fused into the kernel's Q load (K5QueryNorm): Q holds the raw projection.
// head_flags + kmax (k5_attention_flags_rows with a ZERO query statistic: every head starts on the fixed form) -> the fixed-offset
// workgroups decide per head (a row bound above 190 flips the flag to 0); both null -> online max everywhere.
int k5_attention_bf16_prescaled_qnorm_pass(const void* Q, const void* Kc, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                                           int ldk, int ldvt, int ldo, const float* q_norm_w, const float* q_cos, const float* q_sin,
                                           int* head_flags, const float* kmax, int tile_off0, int tile_cnt, float* state, int flags,
                                           int late_pass, void* workspace, void* stream) {
  if (!q_norm_w || !q_cos || !q_sin || (!head_flags != !kmax)) return ret(K5_ERR_ARG, "k5_attention_bf16_prescaled_qnorm_pass");
  const K5QueryNorm qn{q_norm_w, q_cos, q_sin, nullptr};
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, Kc, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  a.balance_ws = (float*)workspace; a.k_prescaled = true; a.head_flags = head_flags; a.row_offset_kmax = kmax;
  a.tile_off0 = tile_off0; a.tile_cnt = tile_cnt; a.state = state; a.flags = flags; a.late_pass = late_pass;
  a.variant = head_flags ? K5_ATTN_AUTO : K5_ATTN_ONLINE; a.query_norm = &qn;
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16_prescaled_qnorm_pass");
}

int64_t k5_attention_balance_size(int H, int q_len) { return (int64_t)k5_attention_balance_bytes(H, q_len); }

int k5_attention_bf16_balanced(const void* Q, const void* K, const void* Vt, void* O, int H, int q_len, int kv_len, int ldq,
                               int ldk, int ldvt, int ldo, float score_bound, void* workspace, void* stream) {
  if (!workspace) return ret(K5_ERR_ARG, "k5_attention_bf16_balanced");
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, K, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  a.score_bound = score_bound; a.balance_ws = (float*)workspace;
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16_balanced");
}

int64_t k5_nabla_workspace_size(int H, int num_blocks) { return (int64_t)k5_nabla_workspace_bytes(H, num_blocks); }

int k5_nabla_select_bf16(const void* q, const void* k, int ldq, int ldk, int H, int N, int T, int Hb, int Wb, int wT, int wH,
                         int wW, float P, void* workspace, void* stream) {
  return ret(k5_launch_nabla_select(q, k, ldq, ldk, H, N, T, Hb, Wb, wT, wH, wW, P, workspace, (hipStream_t)stream),
             "k5_nabla_select_bf16");
}

int k5_attention_nabla_bf16(const void* Q, const void* K, const void* Vt, void* O, int H, int N, int ldq, int ldk, int ldvt,
                            int ldo, float score_bound, const void* workspace, void* stream) {
  if (!workspace || N <= 0 || (N % 64)) return ret(K5_ERR_ARG, "k5_attention_nabla_bf16");
  const int *list, *cnt;
  k5_nabla_workspace_views(const_cast<void*>(workspace), H, N / 64, nullptr, nullptr, &list, &cnt);
  K5AttnSparseArgs a = attn_args<K5AttnSparseArgs>(Q, K, Vt, O, H, N, N, ldq, ldk, ldvt, ldo, stream);
  a.score_bound = score_bound; a.list = list; a.cnt = cnt; a.list_stride = N / 64;
  return ret(k5_launch_attention_bf16_sparse(a), "k5_attention_nabla_bf16");
}

int k5_nabla_mask_u8(const void* workspace, int H, int num_blocks, void* out_u8, void* stream) {
  return ret(k5_launch_nabla_mask_u8(workspace, H, num_blocks, num_blocks, out_u8, (hipStream_t)stream), "k5_nabla_mask_u8");
}

int k5_nabla_select_rect_bf16(const void* q, const void* k, int ldq, int ldk, int H, int Nq, int q_block0, int N, int T, int Hb,
                              int Wb, int wT, int wH, int wW, float P, void* workspace, void* stream) {
  return ret(k5_launch_nabla_select_rect(q, k, ldq, ldk, H, Nq, q_block0, N, T, Hb, Wb, wT, wH, wW, P, workspace,
                                         (hipStream_t)stream), "k5_nabla_select_rect_bf16");
}

int k5_attention_nabla_rect_bf16(const void* Q, const void* K, const void* Vt, void* O, int H, int Nq, int N, int ldq, int ldk,
                                 int ldvt, int ldo, float score_bound, const void* workspace, int vt_chunk_keys,
                                 int64_t vt_chunk_stride, void* stream) {
  if (!workspace || N <= 0 || (N % 64) || Nq <= 0 || (Nq % 64)) return ret(K5_ERR_ARG, "k5_attention_nabla_rect_bf16");
  const int *list, *cnt;
  k5_nabla_workspace_views(const_cast<void*>(workspace), H, N / 64, nullptr, nullptr, &list, &cnt, nullptr, Nq / 64);   // as k5_nabla_select_rect_bf16 laid it out
  K5AttnSparseArgs a = attn_args<K5AttnSparseArgs>(Q, K, Vt, O, H, Nq, N, ldq, ldk, ldvt, ldo, stream);
  a.score_bound = score_bound; a.list = list; a.cnt = cnt; a.list_stride = N / 64;
  a.vt_chunk_keys = vt_chunk_keys; a.vt_chunk_stride = (long long)vt_chunk_stride;
  return ret(k5_launch_attention_bf16_sparse(a), "k5_attention_nabla_rect_bf16");
}

// what the sequence-parallel engine runs: the map with the rank's own key blocks leading every list, and the list-driven attention on
// pre-scaled keys with per-head flags / per-row offsets — in one pass (pass = 0) or two (1: the leading local entries, state out;
// 2: the rest, state in, normalise; a head whose row underflows in pass 1 goes late and is recomputed by the online form of pass 2)
int k5_nabla_select_rect_local_bf16(const void* q, const void* k, int ldq, int ldk, int H, int Nq, int q_block0, int N, int T, int Hb,
                                    int Wb, int wT, int wH, int wW, float P, void* workspace, int local_block0, int local_blocks,
                                    void* stream) {
  return ret(k5_launch_nabla_select_rect(q, k, ldq, ldk, H, Nq, q_block0, N, T, Hb, Wb, wT, wH, wW, P, workspace,
                                         (hipStream_t)stream, local_block0, local_blocks), "k5_nabla_select_rect_local_bf16");
}
int k5_attention_nabla_rect_prescaled_pass(const void* Q, const void* Kc, const void* Vt, void* O, int H, int Nq, int N, int ldq, int ldk,
                                           int ldvt, int ldo, const void* workspace, int vt_chunk_keys, int64_t vt_chunk_stride,
                                           int* head_flags, const float* kmax, int pass, float* state, void* stream) {
  if (!workspace || N <= 0 || (N % 64) || pass < 0 || pass > 2 || (pass && !state) || !head_flags || !kmax)
    return ret(K5_ERR_ARG, "k5_attention_nabla_rect_prescaled_pass");
  const int *list, *cnt, *cnt_local;
  if (Nq <= 0 || (Nq % 64)) return ret(K5_ERR_ARG, "k5_attention_nabla_rect_prescaled_pass");
  k5_nabla_workspace_views(const_cast<void*>(workspace), H, N / 64, nullptr, nullptr, &list, &cnt, &cnt_local, Nq / 64);
  const K5SparsePass p1{nullptr, state, 2, 1}, p2{cnt_local, state, 1, 2};
  K5AttnSparseArgs a = attn_args<K5AttnSparseArgs>(Q, Kc, Vt, O, H, Nq, N, ldq, ldk, ldvt, ldo, stream);
  a.list = list; a.cnt = pass == 1 ? cnt_local : cnt; a.list_stride = N / 64;
  a.vt_chunk_keys = vt_chunk_keys; a.vt_chunk_stride = (long long)vt_chunk_stride;
  a.k_prescaled = true; a.head_flags = head_flags; a.row_offset_kmax = kmax;
  a.pass = pass == 0 ? nullptr : (pass == 1 ? &p1 : &p2);
  return ret(k5_launch_attention_bf16_sparse(a), "k5_attention_nabla_rect_prescaled_pass");
}

int k5_nabla_mask_rect_u8(const void* workspace, int H, int q_blocks, int num_blocks, void* out_u8, void* stream) {
  return ret(k5_launch_nabla_mask_u8(workspace, H, q_blocks, num_blocks, out_u8, (hipStream_t)stream), "k5_nabla_mask_rect_u8");
}

int k5_attention_bf16_bounded(const void* Q, const void* K, const void* Vt, void* O, int H, int q_len, int kv_len,
                              int ldq, int ldk, int ldvt, int ldo, float score_bound, void* stream) {
  K5AttnRangeArgs a = attn_args<K5AttnRangeArgs>(Q, K, Vt, O, H, q_len, kv_len, ldq, ldk, ldvt, ldo, stream);
  a.score_bound = score_bound;
  return ret(k5_launch_attention_bf16_range(a), "k5_attention_bf16_bounded");
}

int k5_ln_modulate_bf16(const void* x, const float* scale, const float* shift, void* out, int rows, int D, int ldx,
                        int ldo, void* stream) {
  return ret(k5_launch_ln_modulate(x, scale, shift, out, rows, D, ldx, ldo, (hipStream_t)stream), "k5_ln_modulate_bf16");
}

int k5_rmsnorm_rope_bf16(void* x, const float* weight, const float* cos_tab, const float* sin_tab, int rows, int H,
                         int ld, int heads_per_weight, int rope_heads, void* stream) {
  const int32_t hc[2] = {heads_per_weight, rope_heads};
  return ret(k5_launch_rmsnorm_rope(x, weight, cos_tab, sin_tab, rows, H, ld, hc, (hipStream_t)stream),
             "k5_rmsnorm_rope_bf16");
}

int k5_rmsnorm_rope_stats_bf16(void* x, const float* weight, const float* cos_tab, const float* sin_tab, int rows, int H, int ld,
                               int heads_per_weight, int rope_heads, float out_scale, int scale_from_head, float* stats, void* stream) {
  const int32_t hc[2] = {heads_per_weight, rope_heads};
  static float* ws = nullptr; static size_t ws_bytes = 0;   // scratch of the kernel-level entry (the engine owns its own)
  const size_t need = k5_rmsnorm_stats_workspace_bytes(H);
  if (stats && need > ws_bytes) {
    if (ws) (void)hipFree(ws);
    ws = nullptr; ws_bytes = 0;
    if (hipMalloc((void**)&ws, need) != hipSuccess) return ret(K5_ERR_HIP, "k5_rmsnorm_rope_stats_bf16");
    ws_bytes = need;
  }
  return ret(k5_launch_rmsnorm_rope(x, weight, cos_tab, sin_tab, rows, H, ld, hc, (hipStream_t)stream, out_scale, scale_from_head,
                                    nullptr, 0, stats, ws), "k5_rmsnorm_rope_stats_bf16");
}

// the same with the centred statistics: centre [H - scale_from_head][64] out, stats = H squared norms then H - scale_from_head squared radii
int k5_rmsnorm_rope_centre_bf16(void* x, const float* weight, const float* cos_tab, const float* sin_tab, int rows, int H, int ld,
                                int heads_per_weight, int rope_heads, float out_scale, int scale_from_head, float* stats, float* centre, void* stream) {
  if (!stats || !centre || scale_from_head < 0 || scale_from_head >= H) return ret(K5_ERR_ARG, "k5_rmsnorm_rope_centre_bf16");
  const int32_t hc[2] = {heads_per_weight, rope_heads};
  static float* ws = nullptr; static size_t ws_bytes = 0;
  const size_t need = k5_rmsnorm_stats_workspace_bytes(H);
  if (need > ws_bytes) {
    if (ws) (void)hipFree(ws);
    ws = nullptr; ws_bytes = 0;
    if (hipMalloc((void**)&ws, need) != hipSuccess) return ret(K5_ERR_HIP, "k5_rmsnorm_rope_centre_bf16");
    ws_bytes = need;
  }
  return ret(k5_launch_rmsnorm_rope(x, weight, cos_tab, sin_tab, rows, H, ld, hc, (hipStream_t)stream, out_scale, scale_from_head,
                                    nullptr, 0, stats, ws, centre), "k5_rmsnorm_rope_centre_bf16");
}

int k5_gate_sum_bf16(const void* x, const void* y, const float* gate, void* out, int rows, int D, void* stream) {
  return ret(k5_launch_gate_sum(x, y, gate, out, rows, D, (hipStream_t)stream), "k5_gate_sum_bf16");
}

// the MagCache calibration pass on caller buffers (kernel tests): the scratch for the per-workgroup partials is kept here
int k5_magcache_stats_bf16(const void* vis, const void* ori, const void* prev, void* res, double* sums, int rows, int D, void* stream) {
  if (rows <= 0) return ret(K5_ERR_ARG, "k5_magcache_stats_bf16");
  static double* ws = nullptr; static size_t ws_bytes = 0;
  const size_t need = (size_t)k5_magcache_stats_blocks(rows) * 4 * sizeof(double);
  if (need > ws_bytes) {
    if (ws) (void)hipFree(ws);
    ws = nullptr; ws_bytes = 0;
    if (hipMalloc((void**)&ws, need) != hipSuccess) return ret(K5_ERR_HIP, "k5_magcache_stats_bf16");
    ws_bytes = need;
  }
  return ret(k5_launch_magcache_stats(vis, ori, prev, res, sums, ws, 0, rows, D, (hipStream_t)stream), "k5_magcache_stats_bf16");
}

int k5_lora_merge(void* W, int w_dtype, int rows, int cols, int ld, const void* A, int a_dtype, const void* B, int b_dtype, int R, float scale,
                  void* stream) {
  return ret(k5_launch_lora_merge(W, w_dtype, rows, cols, ld, A, a_dtype, B, b_dtype, R, scale, (hipStream_t)stream), "k5_lora_merge");
}

int k5_gemv_f32(const float* x, const float* W, const float* b, float* y, int N, int K, int silu_in, const float* add,
                void* stream) {
  return ret(k5_launch_gemv_f32(x, W, b, y, N, K, silu_in, add, (hipStream_t)stream), "k5_gemv_f32");
}

int k5_time_features_f32(float t, float* out, int D, void* stream) {
  return ret(k5_launch_time_features(t, out, D, (hipStream_t)stream), "k5_time_features_f32");
}

int k5_ln_affine_bf16(const void* x, const float* w, const float* b, void* out_bf16, float* out_f32, int rows, int D,
                      void* stream) {
  return ret(k5_launch_ln_affine(x, w, b, out_bf16, out_f32, rows, D, (hipStream_t)stream), "k5_ln_affine_bf16");
}

int k5_rope_table_f32(float* cos_tab, float* sin_tab, const int32_t* pos_t, const int32_t* pos_h, const int32_t* pos_w,
                      int T, int H, int W, int n0, int n1, int n2, float s0, float s1, float s2,
                      const int32_t* tok_perm, void* stream) {
  return ret(k5_launch_rope_table(cos_tab, sin_tab, pos_t, pos_h, pos_w, T, H, W, n0, n1, n2, s0, s1, s2, tok_perm,
                                  (hipStream_t)stream), "k5_rope_table_f32");
}

int k5_patchify_bf16(const float* x, void* out, int T, int H, int W, int x_channels, int Cin_total, int Kpad,
                     const int32_t* tok_perm, void* stream) {
  return ret(k5_launch_patchify(x, out, T, H, W, x_channels, Cin_total, Kpad, tok_perm, (hipStream_t)stream),
             "k5_patchify_bf16");
}

int k5_patchify_cond_bf16(const float* x, const float* vcond, void* out, int T, int H, int W, int x_channels, int Cin_total,
                          int Kpad, const int32_t* tok_perm, void* stream) {
  return ret(k5_launch_patchify_cond(x, vcond, out, T, H, W, x_channels, Cin_total, Kpad, tok_perm, (hipStream_t)stream),
             "k5_patchify_cond_bf16");
}

int k5_patchify_view_bf16(const float* x, int64_t x_frame_stride, int64_t x_row_stride, const float* vcond, int64_t vc_frame_stride,
                          int64_t vc_row_stride, void* out, int T, int H, int W, int x_channels, int Cin_total, int Kpad,
                          const int32_t* tok_perm, void* stream) {
  return ret(k5_launch_patchify_view(x, x_frame_stride, x_row_stride, vcond, vc_frame_stride, vc_row_stride, out, T, H, W, x_channels,
                                     Cin_total, Kpad, tok_perm, (hipStream_t)stream),
             "k5_patchify_view_bf16");
}

int k5_unpatchify_bf16(const void* x, void* out, int T, int Hp, int Wp, int C, int ldx, const int32_t* tok_perm,
                       void* stream) {
  return ret(k5_launch_unpatchify(x, out, T, Hp, Wp, C, ldx, tok_perm, (hipStream_t)stream), "k5_unpatchify_bf16");
}

int k5_cfg_euler(float* img, const void* v_cond, const void* v_uncond, float w, float dt, int64_t n, void* stream) {
  K5EulerStepArgs a;
  a.img = img; a.v_cond = v_cond; a.v_uncond = v_uncond; a.w = w; a.dt = dt;
  a.cells = n; a.C = 1;   // C only matters with a mask
  a.stream = (hipStream_t)stream;
  return ret(k5_launch_euler_step(a), "k5_cfg_euler");
}

int k5_edit_renoise(float* out, const float* source, const float* noise, float sigma, int64_t n, void* stream) {
  return ret(k5_launch_edit_renoise(out, source, noise, sigma, n, (hipStream_t)stream), "k5_edit_renoise");
}

int k5_cfg_euler_edit(float* img, const void* v_cond, const void* v_uncond, float w, float dt, const float* source, const float* noise,
                      const float* keep_mask, float sigma_next, int64_t cells, int C, void* stream) {
  K5EulerStepArgs a;
  a.img = img; a.v_cond = v_cond; a.v_uncond = v_uncond; a.w = w; a.dt = dt;
  a.source = source; a.noise = noise; a.keep_mask = keep_mask; a.sigma_next = sigma_next;
  a.cells = cells; a.C = C;
  a.stream = (hipStream_t)stream;
  return ret(k5_launch_euler_step(a), "k5_cfg_euler_edit");
}

int k5_guidance_stats_blocks(int64_t n) { return k5_guidance_blocks(n); }

int k5_guidance_coeffs_bf16(const void* v_cond, const void* v_uncond, int64_t n, float w, int zero_star, float rescale, double* part,
                            double* sums, float* ab, void* stream) {
  const int st = k5_launch_guidance_coeffs(v_cond, v_uncond, n, w, zero_star, rescale, part, sums, ab, (hipStream_t)stream);
  if (st == K5_ERR_ALIGN) { k5_set_error("k5_guidance_coeffs_bf16: n = %lld is not a multiple of 8", (long long)n); return st; }
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_guidance_coeffs_bf16: need 16-byte aligned non-null pointers, n >= 1, 0 <= rescale <= 1 (n %lld, rescale %g)", (long long)n,
                 (double)rescale);
    return st;
  }
  return ret(st, "k5_guidance_coeffs_bf16");
}

int k5_guided_euler(float* img, const void* v_cond, const void* v_uncond, const float* ab, float dt, const float* source, const float* noise,
                    const float* keep_mask, float sigma_next, int64_t cells, int C, void* v_out, void* stream) {
  K5EulerStepArgs a;
  a.img = img; a.v_cond = v_cond; a.v_uncond = v_uncond; a.ab = ab; a.dt = dt;
  a.source = source; a.noise = noise; a.keep_mask = keep_mask; a.sigma_next = sigma_next;
  a.cells = cells; a.C = C; a.v_out = v_out;
  a.stream = (hipStream_t)stream;
  const int st = ab ? k5_launch_euler_step(a) : K5_ERR_ARG;   // without ab the launcher would take the CFG combine
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_guided_euler: need img, v_cond, v_uncond and ab, cells and C >= 1, and source and noise with a keep_mask (cells %lld, C %d)",
                 (long long)cells, C);
    return st;
  }
  return ret(st, "k5_guided_euler");
}

int k5_skip_euler(float* img, const void* v_cond, const void* v_uncond, const void* v_skip, float w, const float* ab, float g, float dt,
                  const float* source, const float* noise, const float* keep_mask, float sigma_next, int64_t cells, int C, void* v_out,
                  void* stream) {
  K5EulerStepArgs a;
  a.img = img; a.v_cond = v_cond; a.v_uncond = v_uncond; a.w = w; a.ab = ab; a.dt = dt;
  a.source = source; a.noise = noise; a.keep_mask = keep_mask; a.sigma_next = sigma_next;
  a.cells = cells; a.C = C; a.v_out = v_out; a.v_skip = v_skip; a.skip_scale = g;
  a.stream = (hipStream_t)stream;
  const int st = v_skip ? k5_launch_euler_step(a) : K5_ERR_ARG;   // without v_skip the launcher would take a two-velocity update
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_skip_euler: need img, v_cond and v_skip, a finite g > 0, cells and C >= 1, v_uncond with ab, and source and noise with a "
                 "keep_mask (g %g, cells %lld, C %d)", (double)g, (long long)cells, C);
    return st;
  }
  return ret(st, "k5_skip_euler");
}

int k5_philox_words(uint32_t* out, uint64_t blk0, int64_t nblk, uint64_t seed, uint32_t c2, uint32_t c3, void* stream) {
  const int st = k5_launch_philox_words(out, blk0, nblk, seed, c2, c3, (hipStream_t)stream);
  if (st == K5_ERR_ARG) { k5_set_error("k5_philox_words: need a 4-byte aligned out and nblk >= 1 (nblk %lld)", (long long)nblk); return st; }
  return ret(st, "k5_philox_words");
}

int k5_noise_normal_f32(float* out, int64_t n, uint64_t seed, uint32_t stream_id, void* stream) {
  const int st = k5_launch_noise_normal(out, n, seed, stream_id, (hipStream_t)stream);
  if (st == K5_ERR_ARG) { k5_set_error("k5_noise_normal_f32: need a 4-byte aligned out and n >= 1 (n %lld)", (long long)n); return st; }
  return ret(st, "k5_noise_normal_f32");
}

int k5_stochastic_euler(float* img, const void* v_cond, const void* v_uncond, const void* v_skip, float w, const float* ab, float g, float dt_down,
                        const float* source, const float* eps, const float* keep_mask, float sigma_next, int64_t cells, int C, void* v_out,
                        float scale, float noise_coef, const float* noise, uint64_t seed, uint32_t stream_id, void* stream) {
  K5EulerStepArgs a;
  a.img = img; a.v_cond = v_cond; a.v_uncond = v_uncond; a.w = w; a.ab = ab; a.dt = dt_down;
  a.source = source; a.noise = eps; a.keep_mask = keep_mask; a.sigma_next = sigma_next;
  a.cells = cells; a.C = C; a.v_out = v_out; a.v_skip = v_skip; a.skip_scale = g;
  a.stochastic = true; a.scale = scale; a.noise_coef = noise_coef; a.znoise = noise; a.seed = seed; a.stream_id = stream_id;
  a.stream = (hipStream_t)stream;
  const int st = k5_launch_euler_step(a);
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_stochastic_euler: need img and v_cond, cells and C >= 1, v_uncond with ab, a finite g > 0 with v_skip and g = 0 without, v_out "
                 "only with ab or v_skip, source and eps with a keep_mask, a finite scale and a finite noise_coef >= 0 (g %g, scale %g, noise_coef "
                 "%g, cells %lld, C %d)", (double)g, (double)scale, (double)noise_coef, (long long)cells, C);
    return st;
  }
  return ret(st, "k5_stochastic_euler");
}

// The words for what k5_launch_euler_step refused: the launcher decides, this only names the condition among those a caller of the public
// struct can reach (the message of k5_euler_step).
static const char* euler_step_refusal(const k5_euler_step_args& a) {
  if (!a.img) return "img is NULL";
  if (!a.v_cond) return "v_cond is NULL";
  if (a.cells < 1 || a.C < 1) return "cells and C must be >= 1";
  if (a.ab && !a.v_uncond) return "ab needs v_uncond";
  if (a.v_out && !a.ab && !a.v_skip) return "v_out needs ab or v_skip";
  if (a.keep_mask && (!a.source || !a.noise)) return "keep_mask needs source and noise";
  if (a.v_skip && !(a.skip_scale > 0.0f && __builtin_isfinite(a.skip_scale))) return "v_skip needs a finite skip_scale > 0";
  if (!a.v_skip && a.skip_scale != 0.0f) return "a skip_scale != 0 needs v_skip";
  if (a.stochastic && !__builtin_isfinite(a.scale)) return "stochastic needs a finite scale";
  if (a.stochastic && !(a.noise_coef >= 0.0f && __builtin_isfinite(a.noise_coef))) return "stochastic needs a finite noise_coef >= 0";
  if (!a.stochastic && a.znoise) return "znoise needs stochastic";
  return "refused by the launcher";
}

int k5_euler_step(const k5_euler_step_args* args, void* stream) {
  if (!args) { k5_set_error("k5_euler_step: args is NULL"); return K5_ERR_ARG; }
  const int st = k5_launch_euler_step(K5EulerStepArgs(*args, (hipStream_t)stream));
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_euler_step: %s (cells %lld, C %d, skip_scale %g, scale %g, noise_coef %g)", euler_step_refusal(*args), (long long)args->cells,
                 args->C, (double)args->skip_scale, (double)args->scale, (double)args->noise_coef);
    return st;
  }
  return ret(st, "k5_euler_step");
}

int k5_flowedit_step(const k5_flowedit_step_args* args, void* stream) {
  if (!args) { k5_set_error("k5_flowedit_step: args is NULL"); return K5_ERR_ARG; }
  if (const char* why = k5_flowedit_step_refusal(*args)) {
    k5_set_error("k5_flowedit_step: %s (cells %lld, C %d, w_src %g, w_tar %g)", why, (long long)args->cells, args->C, (double)args->w_src,
                 (double)args->w_tar);
    return K5_ERR_ARG;
  }
  return ret(k5_launch_flowedit_step(*args, (hipStream_t)stream), "k5_flowedit_step");
}

// the row and column axes of a temporal plan: one window at 0 of weight 1.0 (never written)
__device__ int32_t k5_whole_axis_start = 0;
__device__ float k5_whole_axis_weight = 1.0f;

// A temporal plan is the 3-D plan over (T, 1, 1, frame_elems) with one row window and one column window of weight 1.0
int k5_cfg_euler_windows(float* img, const void* v_cond, const void* v_uncond, float w, float dt, const int32_t* starts_dev,
                         const float* weights_dev, int nwin, int F, int T, int64_t frame_elems, void* stream) {
  if (!img || !v_cond || !starts_dev || !weights_dev || nwin < 1 || nwin > 64 || F < 1 || T < 1 || frame_elems < 1 || frame_elems > 0x7fffffff) {
    k5_set_error("k5_cfg_euler_windows: null pointer, or nwin (1..64) / F / T / frame_elems (below 2^31) out of range");
    return K5_ERR_ARG;
  }
  // the plan is checked on the host: nwin ints come back once (this entry is the tests' and the tools'; the sampler holds its plan on the host)
  int32_t st[64];
  hipStream_t s = (hipStream_t)stream;
  const int32_t* zero = nullptr;
  const float* one = nullptr;
  if (hipMemcpyAsync(st, starts_dev, (size_t)nwin * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess ||
      hipGetSymbolAddress((void**)&zero, HIP_SYMBOL(k5_whole_axis_start)) != hipSuccess ||
      hipGetSymbolAddress((void**)&one, HIP_SYMBOL(k5_whole_axis_weight)) != hipSuccess)
    return ret(K5_ERR_HIP, "k5_cfg_euler_windows");
  if (const char* why = k5_tile_axis_refusal("frame", nwin, st, F, T)) {
    k5_set_error("k5_cfg_euler_windows: %s", why);
    return K5_ERR_ARG;
  }
  const k5_tile_plan p{nwin, 1, 1, F, 1, 1, starts_dev, zero, zero, weights_dev, one, one};
  return ret(k5_launch_cfg_euler_tiles(img, v_cond, v_uncond, w, dt, p, T, 1, 1, (int)frame_elems, s), "k5_cfg_euler_windows");
}

int k5_cfg_euler_tiles(float* img, const void* v_cond, const void* v_uncond, float w, float dt, const k5_tile_plan* p, int T, int H, int W, int C,
                       void* stream) {
  if (!img || !v_cond || !p || !p->starts_t || !p->starts_y || !p->starts_x || !p->wt || !p->wy || !p->wx) {
    k5_set_error("k5_cfg_euler_tiles: null pointer (img, v_cond, the plan or one of its six tables)");
    return K5_ERR_ARG;
  }
  if (T < 1 || H < 1 || W < 1 || C < 1 || p->Ft < 1 || p->Fh < 1 || p->Fw < 1) {
    k5_set_error("k5_cfg_euler_tiles: the clip (%d, %d, %d, %d) and the window (%d, %d, %d) must be >= 1", T, H, W, C, p->Ft, p->Fh, p->Fw);
    return K5_ERR_ARG;
  }
  if (p->nt < 1 || p->ny < 1 || p->nx < 1 || p->nt > 64 || p->ny > 64 || p->nx > 64 || p->nt * p->ny * p->nx > 64) {
    k5_set_error("k5_cfg_euler_tiles: nwin must be 1..64 (got %d x %d x %d)", p->nt, p->ny, p->nx);
    return K5_ERR_ARG;
  }
  // the plan is checked on the host: the three start vectors come back once (this entry is the per-step paths' and the tests'; k5_sample_tiles holds its plan on the host)
  int32_t st[3][64];
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(st[0], p->starts_t, (size_t)p->nt * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(st[1], p->starts_y, (size_t)p->ny * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(st[2], p->starts_x, (size_t)p->nx * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return ret(K5_ERR_HIP, "k5_cfg_euler_tiles");
  const struct { const char* name; int n, F, total; } ax[3] = {{"frame", p->nt, p->Ft, T}, {"row", p->ny, p->Fh, H}, {"column", p->nx, p->Fw, W}};
  for (int i = 0; i < 3; ++i)
    if (const char* why = k5_tile_axis_refusal(ax[i].name, ax[i].n, st[i], ax[i].F, ax[i].total)) {
      k5_set_error("k5_cfg_euler_tiles: %s", why);
      return K5_ERR_ARG;
    }
  return ret(k5_launch_cfg_euler_tiles(img, v_cond, v_uncond, w, dt, *p, T, H, W, C, s), "k5_cfg_euler_tiles");
}

int k5_x0_preview(const float* x, const void* v_cond, const void* v_uncond, float w, float sigma_next, const float* source,
                  const float* keep_mask, const float* rgb_w, const float* rgb_b, float* x0_out, uint8_t* rgb, int64_t cells, int C,
                  void* stream) {
  return ret(k5_launch_x0_preview(x, v_cond, v_uncond, w, sigma_next, source, keep_mask, rgb_w, rgb_b, x0_out, rgb, cells, C,
                                  (hipStream_t)stream), "k5_x0_preview");
}

int k5_nag_combine_bf16(const void* z_pos, const void* z_neg, void* out, int rows, int D, int ld, float s, float tau, float alpha,
                        void* stream) {
  const int st = k5_launch_nag_combine(z_pos, z_neg, out, rows, D, ld, s, tau, alpha, (hipStream_t)stream);
  if (st == K5_ERR_UNSUPPORTED) { k5_set_error("k5_nag_combine_bf16: D = %d is more than the register-resident row holds (2048)", D); return st; }
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_nag_combine_bf16: need 16-byte aligned non-null pointers, rows > 0, D %% 8 == 0, ld >= D, ld %% 8 == 0, s >= 1, tau >= 1, "
                 "0 <= alpha <= 1 (rows %d, D %d, ld %d, s %g, tau %g, alpha %g)", rows, D, ld, (double)s, (double)tau, (double)alpha);
    return st;
  }
  return ret(st, "k5_nag_combine_bf16");
}

long long k5_enhance_part_count(int Hh, int S) { return k5_enhance_parts(Hh, S); }

int k5_enhance_scores_bf16(const void* Q, const void* K, int ldq, int ldk, int Hh, int T, int S, const int32_t* frame_rows, float qk_scale,
                           float weight, double* part, float* score_out, void* stream) {
  const int st = k5_launch_enhance_scores(Q, K, ldq, ldk, Hh, T, S, frame_rows, qk_scale, weight, part, score_out, (hipStream_t)stream);
  if (st == K5_ERR_UNSUPPORTED) { k5_set_error("k5_enhance_scores_bf16: T = %d frames are more than the four 32 x 32 accumulators of a wave hold (64)", T); return st; }
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_enhance_scores_bf16: need 16-byte aligned non-null Q and K, non-null part and score_out, ld >= 64 Hh, ld %% 8 == 0, Hh >= 1, "
                 "S >= 1, T >= 2, a finite weight >= 0 and a finite qk_scale > 0 (ldq %d, ldk %d, Hh %d, T %d, S %d, weight %g, qk_scale %g)",
                 ldq, ldk, Hh, T, S, (double)weight, (double)qk_scale);
    return st;
  }
  return ret(st, "k5_enhance_scores_bf16");
}

int k5_scale_by_dev_bf16(void* x, int rows, int D, int ld, const float* score_dev, void* stream) {
  const int st = k5_launch_scale_by_dev(x, rows, D, ld, score_dev, (hipStream_t)stream);
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_scale_by_dev_bf16: need a 16-byte aligned non-null x, a non-null score_dev, rows > 0, D %% 8 == 0, ld >= D, ld %% 8 == 0 "
                 "(rows %d, D %d, ld %d)", rows, D, ld);
    return st;
  }
  return ret(st, "k5_scale_by_dev_bf16");
}

int k5_forecast_update_bf16(const void* vis, int ld, const void* ori, void* F0, float* D1, float* D2, int rows, int D, int g, int order, int have,
                            void* stream) {
  const int st = k5_launch_forecast_update(vis, ld, ori, F0, D1, D2, rows, D, g, order, have, (hipStream_t)stream);
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_forecast_update_bf16: need 16-byte aligned non-null vis, ori, F0 (and D1 / D2 up to min(order, have)), rows > 0, D %% 8 == 0, "
                 "ld >= D, ld %% 8 == 0, g >= 1, order in 0..2, have >= 0 (rows %d, D %d, ld %d, g %d, order %d, have %d)", rows, D, ld, g, order, have);
    return st;
  }
  return ret(st, "k5_forecast_update_bf16");
}

int k5_forecast_apply_bf16(void* vis, int ld, const void* F0, const float* D1, const float* D2, int rows, int D, int k, int g, int gp, int order,
                           int have, void* stream) {
  const int st = k5_launch_forecast_apply(vis, ld, F0, D1, D2, rows, D, k, g, gp, order, have, (hipStream_t)stream);
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_forecast_apply_bf16: need 16-byte aligned non-null vis, F0 (and D1 / D2 up to min(order, have - 1)), rows > 0, D %% 8 == 0, "
                 "ld >= D, ld %% 8 == 0, k >= 1, g and gp >= 1 at two terms, order in 0..2, have >= 1 (rows %d, D %d, ld %d, k %d, g %d, gp %d, order %d, "
                 "have %d)", rows, D, ld, k, g, gp, order, have);
    return st;
  }
  return ret(st, "k5_forecast_apply_bf16");
}

int k5_region_combine_bf16(const void* z0, const void* zr, long long zr_stride, int R, const float* w, int ldw, void* out, int rows, int D,
                           int ld, void* stream) {
  const int st = k5_launch_region_combine(z0, zr, zr_stride, R, w, ldw, out, rows, D, ld, (hipStream_t)stream);
  if (st == K5_ERR_UNSUPPORTED) { k5_set_error("k5_region_combine_bf16: D = %d is more than the register-resident row holds (2048)", D); return st; }
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_region_combine_bf16: need 16-byte aligned non-null pointers (w: 4-byte), rows > 0, D %% 8 == 0, ld >= D, ld %% 8 == 0, "
                 "zr_stride %% 8 == 0, 1 <= R <= 8, ldw >= R + 1 (rows %d, D %d, ld %d, R %d, ldw %d, zr_stride %lld)", rows, D, ld, R, ldw, zr_stride);
    return st;
  }
  return ret(st, "k5_region_combine_bf16");
}

int k5_region_weights_f32(const float* masks, int R, int T, int H, int W, int pt, int ph, int pw, float base_weight, const int32_t* perm,
                          float* w, void* stream) {
  const int st = k5_launch_region_weights(masks, R, T, H, W, pt, ph, pw, base_weight, perm, w, (hipStream_t)stream);
  if (st == K5_ERR_UNSUPPORTED) { k5_set_error("k5_region_weights_f32: %d x %d x %d cells are more than 2^31 - 1", T, H, W); return st; }
  if (st == K5_ERR_ARG) {
    k5_set_error("k5_region_weights_f32: need 4-byte aligned non-null masks and w, 1 <= R <= 8, T, H, W >= 1 and divisible by the patch, "
                 "0 <= base_weight <= 1 (R %d, shape %d x %d x %d, patch %d x %d x %d, base_weight %g)", R, T, H, W, pt, ph, pw, (double)base_weight);
    return st;
  }
  return ret(st, "k5_region_weights_f32");
}

int k5_conv3d_bf16(const void* X, const void* W, const float* bias, void* out, int Ts, int Hs, int Ws, int Cin, int Cout,
                   int up_t, int up_s, int ldc, const void* resid, int ldr, void* stream) {
  return ret(k5_launch_conv3d_bf16(X, W, bias, out, Ts, Hs, Ws, Cin, Cout, up_t, up_s, ldc, resid, ldr, (hipStream_t)stream),
             "k5_conv3d_bf16");
}

int k5_conv3d_strided_bf16(const void* X, const void* W, const float* bias, void* out, int Ts, int Hs, int Ws, int Cin, int Cout,
                           int st_t, int st_s, int ldc, void* stream) {
  return ret(k5_launch_conv3d_bf16_strided(X, W, bias, out, Ts, Hs, Ws, Cin, Cout, 1, 1, st_t, st_s, ldc, nullptr, 0, (hipStream_t)stream),
             "k5_conv3d_strided_bf16");
}

int64_t k5_conv3d_stats_size(int M, int Cout) { return (int64_t)2 * ((M + 255) / 256) * (Cout / 4) * 2 * (int64_t)sizeof(float); }

int k5_conv3d_bf16_stats(const void* X, const void* W, const float* bias, void* out, int Ts, int Hs, int Ws, int Cin, int Cout,
                         int up_t, int up_s, int ldc, const void* resid, int ldr, float* quad_stats, void* stream) {
  if (!quad_stats || (Cout & 3)) return K5_ERR_ARG;
  const int st = k5_launch_conv3d_w4(X, W, bias, out, Ts, Hs, Ws, Cin, Cout, up_t, up_s, ldc, resid, ldr, quad_stats, (hipStream_t)stream);
  return st == K5_ERR_UNSUPPORTED ? st : ret(st, "k5_conv3d_bf16_stats");   // outside the 4-wave kernel's range: no statistics, caller's business
}

int k5_groupnorm_bf16_quads(const void* x, const float* gamma, const float* beta, void* out, int M, int C, int G, float eps, int silu,
                            const float* quad_stats, void* workspace, void* stream) {
  if (!quad_stats || !workspace) return K5_ERR_ARG;
  return ret(k5_launch_groupnorm_bf16_quads(x, gamma, beta, out, M, C, G, eps, silu, C, C, quad_stats, 2 * ((M + 255) / 256), (float*)workspace,
                                            (hipStream_t)stream), "k5_groupnorm_bf16_quads");
}

int64_t k5_groupnorm_workspace_size(int M, int G) { return (int64_t)k5_groupnorm_workspace_bytes(M, G); }

int k5_groupnorm_bf16(const void* x, const float* gamma, const float* beta, void* out, int M, int C, int G, float eps,
                      int silu, void* workspace, void* stream) {
  return ret(k5_launch_groupnorm_bf16(x, gamma, beta, out, M, C, G, eps, silu, C, C, workspace, (hipStream_t)stream),
             "k5_groupnorm_bf16");
}

}  // extern "C"
