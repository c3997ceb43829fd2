// engine.hip — the denoising engine behind the C ABI: DiffusionTransformer3D forward
// (kandinsky/models/dit.py:155-181) and the flow-matching Euler / CFG loop
// (kandinsky/generation_utils.py:39-129), scheduled as a fixed sequence of gfx950 kernels on one
// HIP stream.  Weights are packed once (Wq|Wk concatenated, padded K, bf16 / fp32-island copies),
// workspaces are persistent, RoPE tables and the batched AdaLN modulation are computed once per
// forward.  No host synchronisation inside forward()/sample().
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <optional>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <pthread.h>
#include <rccl/rccl.h>  // types / enums only: the library is dlopen()ed (see Comm)

#include "k5_common.h"
#include "k5_kernels.h"
#include "ipc_comm.h"   // one-sided IPC transport of the sharded path (P processes on one device or on the devices of one node)

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
void k5_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* k5_last_error(void) { return g_err; }
extern "C" int k5_abi_version(void) { return K5_ABI_VERSION; }

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      k5_set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
      return K5_ERR_HIP;                                                                   \
    }                                                                                      \
  } while (0)
#define K5CHK(x)                                                             \
  do {                                                                       \
    int s_ = (x);                                                            \
    if (s_ != K5_OK) {                                                       \
      if (!g_err[0]) k5_set_error("%s -> status %d (%s:%d)", #x, s_, __FILE__, __LINE__); \
      return s_;                                                             \
    }                                                                        \
  } while (0)

namespace {

struct DevBuf {   // owning device buffer (move-only): freed with whatever holds it — the handle, a staged tensor, a block's weights
  void* p = nullptr;
  size_t bytes = 0;
  bool owned = true;   // false: a view into somebody else's buffer (alias), never freed from here
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), owned(o.owned) { o.p = nullptr; o.bytes = 0; o.owned = true; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; owned = o.owned; o.p = nullptr; o.bytes = 0; o.owned = true; } return *this; }
  ~DevBuf() { release(); }
  // slack: bytes allocated beyond n (GEMM operands: K5_GEMM_GUARD_ROWS rows, k5_kernels.h); never counted in `bytes`
  int ensure(size_t n, size_t slack = 0) {
    if (n <= bytes) return K5_OK;
    release();
    HIPCHK(hipMalloc(&p, n + slack));
    bytes = n;
    return K5_OK;
  }
  void release() { if (p && owned) { (void)hipFree(p); k5ipc::note_free(p); } p = nullptr; bytes = 0; owned = true; }   // note_free: an IPC export of this allocation is void from here on
  void alias(void* ptr, size_t n) { release(); p = ptr; bytes = n; owned = false; }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct HostTensor {  // staged state_dict entry: vectors (biases, norms) as fp32 on the host, matrices as a raw copy ON THE DEVICE in
  std::vector<float> data;          // the checkpoint's dtype — they are converted / padded / concatenated by a device kernel
  std::vector<int64_t> shape;       // (k5_launch_pack_matrix), so a checkpoint that already lives on the GPU never touches the host
  DevBuf dev; int dtype = K5_F32;   // and a host one costs its own bytes once (round 1: everything through host fp32, 4 B/param)
  size_t count() const { size_t n = 1; for (int64_t v : shape) n *= (size_t)v; return n; }
};

float half_to_float(uint16_t h) {
  const uint32_t s = (h >> 15) & 1, e = (h >> 10) & 31, m = h & 1023;
  uint32_t bits;
  if (e == 0) {
    if (m == 0) bits = s << 31;
    else {
      int ee = -1; uint32_t mm = m;
      do { ++ee; mm <<= 1; } while (!(mm & 1024));
      bits = (s << 31) | ((uint32_t)(112 - ee) << 23) | ((mm & 1023) << 13);
    }
  } else if (e == 31) bits = (s << 31) | 0x7f800000u | (m << 13);
  else bits = (s << 31) | ((e + 112) << 23) | (m << 13);
  float f; memcpy(&f, &bits, 4); return f;
}
uint16_t f32_to_bf16_rne(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1);
  return (uint16_t)(u >> 16);
}
float bf16_round_host(float f) { uint32_t u = (uint32_t)f32_to_bf16_rne(f) << 16; float r; memcpy(&r, &u, 4); return r; }

// One packed linear layer, or (rows()) a row range of one: bf16 weights [N][ld] (K <= ld input features; the GEMM runs over all ld columns, the
// padding is zero), the bias as fp32 of bf16-rounded values (absent: the feed-forward has none) and, once k5_dit_set_fp8 asked for it, an e4m3
// copy [N][K] with one fp32 scale per output channel.  load_linear fills it, linear() launches it.
struct Linear {
  DevBuf w, b, w8, sc;
  int N = 0, K = 0, ld = 0;
  bool has_e4m3() const { return w8.p != nullptr; }
  // non-owning view of output channels [row0, row0 + n): weights, bias, e4m3 copy and scales move together
  Linear rows(size_t row0, size_t n) const {
    Linear v;
    v.N = (int)n; v.K = K; v.ld = ld;
    v.w.alias(w.as<bf16_t>() + row0 * ld, n * ld * 2);
    if (b.p) v.b.alias(b.as<float>() + row0, n * 4);
    if (w8.p) { v.w8.alias(w8.as<uint8_t>() + row0 * K, n * K); v.sc.alias(sc.as<float>() + row0, n * 4); }
    return v;
  }
  // make (create) or refresh the e4m3 copy from the current bf16 bits; per output channel, so rows that did not change come out as they were
  int quantise(bool create) {
    if (!w8.p) {
      if (!create) return K5_OK;
      K5CHK(w8.ensure((size_t)N * K, (size_t)K5_GEMM_GUARD_ROWS * K)); K5CHK(sc.ensure((size_t)N * 4));
    }
    return k5_launch_quant_rows_fp8(w.p, w8.p, sc.as<float>(), N, K, ld, K, nullptr);
  }
};
// activation rows [rows][ld] in bf16 and, where the call runs in e4m3 (the shape rules sa_fp8_in / sa_sp_fp8_in / ff_fp8_in / f8_out decide,
// e4m3_rows provides), the same rows in e4m3 at the same stride
struct Act {
  const void* bf = nullptr; const void* e4 = nullptr; int rows = 0, ld = 0;
  Act from(size_t row0, int n) const { return Act{(const bf16_t*)bf + row0 * ld, e4 ? (const uint8_t*)e4 + row0 * ld : nullptr, n, ld}; }
};
// One linear layer on activation rows: out [x.rows][ldc] = epilogue(x W^T + bias).  weights_as_rows: the V^T form, out [N][ldc] = W x^T with
// the bias per output ROW.  x.e4 set: both operands in e4m3 (gemm_fp8.hip), otherwise bf16.
struct LinearArgs {
  const Linear* lin; Act x; void* out; int ldc; hipStream_t stream;
  LinearArgs(const Linear& l, const Act& x_, void* out_, int ldc_, hipStream_t s) : lin(&l), x(x_), out(out_), ldc(ldc_), stream(s) {}
  int epi = K5_EPI_BIAS;
  const void* resid = nullptr; int ldr = 0; const float* gate = nullptr;
  bool weights_as_rows = false;
  int force_kernel = 0;                // bf16 only: k5_launch_gemm_bf16's kernel id (2 keeps a summation order whatever the shape)
};
int linear(const LinearArgs& a) {
  const Linear& l = *a.lin;
  const bool t = a.weights_as_rows;
  const int M = t ? l.N : a.x.rows, N = t ? a.x.rows : l.N;
  if (a.x.e4) {
    // the scales belong to the weights' channels: rows of the output in the V^T form (scale_m), where the bias then follows them under K5_EPI_BIAS
    if (!l.has_e4m3()) { k5_set_error("internal: e4m3 activations for a layer without an e4m3 copy"); return K5_ERR_STATE; }
    return k5_launch_gemm_fp8(t ? l.w8.p : a.x.e4, t ? a.x.e4 : l.w8.p, l.sc.as<float>(), a.out, M, N, l.K, t ? l.K : a.x.ld, t ? a.x.ld : l.K, a.ldc, a.epi,
                              a.resid, a.ldr, a.gate, a.stream, l.b.as<float>(), t ? 1 : 0);
  }
  const int epi = (t && a.epi == K5_EPI_BIAS) ? K5_EPI_BIAS_M : a.epi;
  return k5_launch_gemm_bf16(t ? l.w.p : a.x.bf, t ? a.x.bf : l.w.p, l.b.as<float>(), a.out, M, N, l.ld, t ? l.ld : a.x.ld, t ? a.x.ld : l.ld, a.ldc, epi,
                             a.resid, a.ldr, a.gate, a.stream, a.force_kernel);
}

struct AttnW {  // one attention module, packed
  Linear wqk, wq, wk, wv, wo;       // self-attention: wqk (to_query stacked over to_key), wv, wo; cross-attention: wq, wo, and wk / wv as views
                                    // of the handle's stacks over all visual blocks (k5_dit::cx_k / cx_v)
  DevBuf norm;                      // fp32 [q_norm | k_norm]
  float score_bound = 0.f;          // |q.k| <= 64 max|w_q| max|w_k| after norm_qk (RoPE preserves norms)
  mutable DevBuf pref;              // visual self-attention: [3][H] heads the per-row-offset softmax served badly the last time this layer ran for
                                    // the cond (0) / uncond (1) / skip (2, k5_dit_forward_skip's own blocks) branch (k5_launch_attn_pref_update); zeroed at the start of every k5_sample and
                                    // by k5_dit_set_option("attn_pref_reset") — never carried from one sampling run, prompt or shape to the next
};
struct BlockW {
  AttnW self_attn, cross_attn;
  Linear w1, w2;  // feed_forward in/out (no bias)
  size_t mod_off = 0;  // offset (floats) of this block's modulation vector in mod_all
};

struct Prof { double ms = 0; int64_t n = 0; };

// RCCL over xGMI, one process per GPU.  The library is dlopen()ed (RTLD_LOCAL) from a path given by the
// host — normally the librccl.so that torch already mapped — so libk5 has no link-time RCCL dependency
// and never ends up with a second, conflicting copy of the nccl* symbols in the global namespace.
// Loopback group: P handles of ONE process on ONE GPU act as the P ranks of a sequence-parallel run (k5_loopback_create /
// k5_dit_comm_init_loopback).  Each rank is driven by its own host thread; a collective is a rendezvous of those threads
// (two pthread barriers) around device-to-device copies ordered by events, so every rank executes exactly the code path,
// offsets and launch sequence of a real multi-GPU run — what moves the bytes is hipMemcpyAsync instead of RCCL.
struct LoopGroup {
  int world = 0;
  pthread_barrier_t bar;
  std::vector<void*> ptr;
  std::vector<hipEvent_t> ready, pulled;
  std::vector<int> joined;
};

struct Comm {
  void* lib = nullptr;
  ncclComm_t comm = nullptr;
  LoopGroup* loop = nullptr;
  k5ipc::Group* ipc = nullptr;   // one process per rank, peers' buffers IPC-mapped (ipc_comm.h): k5_dit_comm_init_ipc / k5_dit_cfg_pair_init_ipc
  bool active() const { return comm != nullptr || loop != nullptr || ipc != nullptr; }
  int ipc_status(int r) { if (r) { k5_set_error("%s", ipc->err.c_str()); return K5_ERR_STATE; } return K5_OK; }
  int rank = 0, world = 1;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;   // optional: sliced exchange
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;   // optional: what the communicator itself says its size is (k5_dit_get_option "rccl_ranks")
  int open(const char* path) {
    if (lib) return K5_OK;
    const char* cands[] = {path, "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
    for (const char* c : cands) {
      if (!c || !c[0]) continue;
      lib = dlopen(c, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) { k5_set_error("cannot dlopen RCCL (%s): %s", path ? path : "default names", dlerror()); return K5_ERR_STATE; }
    GetUniqueId = (decltype(GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    CommInitRank = (decltype(CommInitRank))dlsym(lib, "ncclCommInitRank");
    CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
    AllGather = (decltype(AllGather))dlsym(lib, "ncclAllGather");
    GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
    Send = (decltype(Send))dlsym(lib, "ncclSend"); Recv = (decltype(Recv))dlsym(lib, "ncclRecv");
    GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart"); GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
    CommCount = (decltype(CommCount))dlsym(lib, "ncclCommCount");
    if (!GetUniqueId || !CommInitRank || !CommDestroy || !AllGather || !GetErrorString) {
      k5_set_error("RCCL library lacks a required nccl* symbol"); return K5_ERR_STATE;
    }
    return K5_OK;
  }
  // loopback rendezvous shared by the four collectives: publish my buffer, pull what `pull(p, peer's buffer)` names out of every peer's
  // (skip: nothing to trade with that peer, its ready event is not waited on); the call completes (stream-wise) only when every peer has
  // pulled mine, as an RCCL collective does — the caller may overwrite what it published afterwards
  struct Pull { void* dst; const void* src; size_t bytes; bool skip; };
  template <class F> int loop_pull(void* my_ptr, hipStream_t s, F pull) {
    loop->ptr[rank] = my_ptr;
    HIPCHK(hipEventRecord(loop->ready[rank], s));
    pthread_barrier_wait(&loop->bar);
    for (int p = 0; p < world; ++p) {
      if (p == rank) continue;
      const Pull c = pull(p, (const char*)loop->ptr[p]);
      if (c.skip) continue;
      HIPCHK(hipStreamWaitEvent(s, loop->ready[p], 0));
      HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipEventRecord(loop->pulled[rank], s));
    pthread_barrier_wait(&loop->bar);
    for (int p = 0; p < world; ++p)
      if (p != rank) HIPCHK(hipStreamWaitEvent(s, loop->pulled[p], 0));
    return K5_OK;
  }
  // one grouped send / recv per peer (all xGMI links at once): send_recv(p) issues what this rank trades with peer p
  template <class F> int rccl_group(const char* what, F send_recv) {
    if (!can_exchange()) { k5_set_error("RCCL library lacks ncclSend / ncclRecv / ncclGroup*"); return K5_ERR_STATE; }
    ncclResult_t r = GroupStart();
    for (int p = 0; p < world && r == ncclSuccess; ++p)
      if (p != rank) r = send_recv(p);
    const ncclResult_t e = GroupEnd();
    if (r == ncclSuccess) r = e;
    if (r != ncclSuccess) { k5_set_error("ncclSend/ncclRecv group%s: %s", what, GetErrorString(r)); return K5_ERR_HIP; }
    return K5_OK;
  }
  bool can_exchange() const { return loop || ipc || (Send && Recv && GroupStart && GroupEnd); }
  // in-place all-gather: every rank's chunk already sits at buf + rank*count*elem
  int all_gather_inplace(void* buf, size_t count_per_rank, size_t elem_bytes, hipStream_t s) {
    char* b = (char*)buf;
    const size_t chunk = count_per_rank * elem_bytes;
    if (ipc) return ipc_status(ipc->all_gather_inplace(buf, chunk, s));
    if (loop) return loop_pull(buf, s, [&](int p, const char* peer) { return Pull{b + (size_t)p * chunk, peer + (size_t)p * chunk, chunk, false}; });
    const ncclResult_t r = AllGather(b + (size_t)rank * chunk, b, chunk, ncclUint8, comm, s);
    if (r != ncclSuccess) { k5_set_error("ncclAllGather: %s", GetErrorString(r)); return K5_ERR_HIP; }
    return K5_OK;
  }
  // all-to-all (Ulysses): block p of `send` (block_bytes each) goes to rank p, block p of `recv` comes from rank p; send != recv.
  // The rank's own block is a device-to-device copy.
  int all_to_all(const void* send, void* recv, size_t block_bytes, hipStream_t s) {
    const char* sb = (const char*)send; char* rb = (char*)recv;
    HIPCHK(hipMemcpyAsync(rb + (size_t)rank * block_bytes, sb + (size_t)rank * block_bytes, block_bytes, hipMemcpyDeviceToDevice, s));
    if (world == 1) return K5_OK;
    if (ipc) return ipc_status(ipc->all_to_all(send, recv, block_bytes, s));
    if (loop) return loop_pull(const_cast<void*>(send), s, [&](int p, const char* peer) {
      return Pull{rb + (size_t)p * block_bytes, peer + (size_t)rank * block_bytes, block_bytes, false}; });
    return rccl_group(" (all-to-all)", [&](int p) {
      const ncclResult_t r = Send(sb + (size_t)p * block_bytes, block_bytes, ncclUint8, p, comm, s);
      return r == ncclSuccess ? Recv(rb + (size_t)p * block_bytes, block_bytes, ncclUint8, p, comm, s) : r; });
  }
  // part of an in-place all-gather: the bytes [off, off + cnt) of every rank's slot (slot_bytes each, rank p's at p * slot_bytes)
  // travel to every peer — all seven xGMI links of the GPU at once, so the first slice of ALL
  // peers has landed when a fraction cnt / slot_bytes of the gather time has passed (a ring all-gather completes nothing early).
  int slot_exchange(void* buf, size_t slot_bytes, size_t off, size_t cnt, hipStream_t s) {
    char* b = (char*)buf;
    if (cnt == 0 || world == 1) return K5_OK;
    if (ipc) return ipc_status(ipc->slot_exchange(buf, slot_bytes, off, cnt, s));
    if (loop) return loop_pull(buf, s, [&](int p, const char* peer) {
      return Pull{b + (size_t)p * slot_bytes + off, peer + (size_t)p * slot_bytes + off, cnt, false}; });
    return rccl_group("", [&](int p) {
      const ncclResult_t r = Send(b + (size_t)rank * slot_bytes + off, cnt, ncclUint8, p, comm, s);
      return r == ncclSuccess ? Recv(b + (size_t)p * slot_bytes + off, cnt, ncclUint8, p, comm, s) : r; });
  }
  // planned exchange (two-level schedule, sp_plan_2d): tab[src * world + dst] = (offset in src's `send`, offset in dst's `recv`, bytes) — the
  // same table on every rank; 0 bytes = the pair has nothing to trade (peers outside a sub-group).  Every rank of the world issues every call.
  // The rank's own entry is a device-to-device copy; RCCL: grouped send / recv to the listed peers only; loopback / IPC: pull copies.
  int exchange(const void* send, void* recv, const k5ipc::Xfer* tab, hipStream_t s) {
    const char* sb = (const char*)send; char* rb = (char*)recv;
    const k5ipc::Xfer& me = tab[(size_t)rank * world + rank];
    if (me.bytes > 0) HIPCHK(hipMemcpyAsync(rb + me.recv_off, sb + me.send_off, (size_t)me.bytes, hipMemcpyDeviceToDevice, s));
    if (world == 1) return K5_OK;
    if (ipc) return ipc_status(ipc->exchange(send, recv, tab, s));
    if (loop) return loop_pull(const_cast<void*>(send), s, [&](int p, const char* peer) {
      const k5ipc::Xfer& e = tab[(size_t)p * world + rank];
      return Pull{rb + e.recv_off, peer + e.send_off, (size_t)e.bytes, e.bytes <= 0}; });
    return rccl_group(" (planned exchange)", [&](int p) {
      const k5ipc::Xfer& out = tab[(size_t)rank * world + p];
      const k5ipc::Xfer& in = tab[(size_t)p * world + rank];
      ncclResult_t r = ncclSuccess;
      if (out.bytes > 0) r = Send(sb + out.send_off, (size_t)out.bytes, ncclUint8, p, comm, s);
      if (r == ncclSuccess && in.bytes > 0) r = Recv(rb + in.recv_off, (size_t)in.bytes, ncclUint8, p, comm, s);
      return r; });
  }
};

// ---- the two-level schedule's exchange plan ("sp_mode" = 2; run_self_attention_heads) ----
// G = gcd(heads, P) head groups of Hp = heads / G heads (Dp = D / G columns); S = P / G query splits.  Rank r serves head group r % G for the
// queries of split r / G = the token shards of ranks sG .. sG + G - 1 (one contiguous token range).  Every block below is rows_pad x Dp bf16.
//   SP_K   k' of the rank's rows, send [G][rows_pad][Dp] (block = head group) -> every peer p gets block g(p); recv [P][rows_pad][Dp] = token order
//   SP_VT  V^T, send [D][rows_pad] as the GEMM writes it (rows g Dp .. = block g) -> every peer p gets block g(p); recv [P][Dp][rows_pad]
//   SP_Q   q, send [G][rows_pad][Dp] -> only the ranks of the split: block g(p) to p; recv [G][rows_pad][Dp] = the split's rows of my heads
//   SP_O   attention output, send [G][rows_pad][Dp] (block j = rows of rank sG + j) -> back inside the split; recv [G][rows_pad][Dp] (block = head group)
enum { SP_K = 0, SP_VT = 1, SP_Q = 2, SP_O = 3 };
int sp_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }
// fills tab[src * P + dst]; returns G (0 on bad arguments)
int sp_plan_2d(int H, int P, int rows_pad, int D, int which, k5ipc::Xfer* tab) {
  if (H <= 0 || P <= 0 || rows_pad <= 0 || D <= 0 || D % H || which < SP_K || which > SP_O) return 0;
  const int G = sp_gcd(H, P), Dp = D / G;
  const long long B = (long long)rows_pad * Dp * 2;
  for (int src = 0; src < P; ++src)
    for (int dst = 0; dst < P; ++dst) {
      k5ipc::Xfer& e = tab[(size_t)src * P + dst];
      if (which == SP_K || which == SP_VT) e = k5ipc::Xfer{(dst % G) * B, src * B, B};
      else if (src / G == dst / G) e = k5ipc::Xfer{(dst % G) * B, (src % G) * B, B};
      else e = k5ipc::Xfer{0, 0, 0};
    }
  return G;
}

}  // namespace

namespace { struct SampleRun; }   // what one sample_impl call works on (defined with it)

struct k5_dit {
  k5_dit_config cfg{};
  int D = 0, FF = 0, TD = 0, Hh = 0, Kvis = 0, KvisPad = 0, Fout = 0;
  bool finalized = false;
  std::map<std::string, HostTensor> staged;
  std::vector<std::string> expected;

  // packed weights
  DevBuf time_w1, time_b1, time_w2, time_b2;                   // fp32
  Linear text_lin, pool_lin, vis_lin, out_lin;                 // the in_layers of the text / pooled / visual embeddings and the out layer
  DevBuf text_lnw, text_lnb, pool_lnw, pool_lnb;               // fp32
  DevBuf mod_w, mod_b;                                         // all Modulation layers stacked, fp32
  size_t mod_rows = 0, out_mod_off = 0;
  std::vector<BlockW> tblocks, vblocks;

  // workspaces
  DevBuf ws_text_in, ws_th, ws_tqk, ws_tvt, ws_to, ws_tff;       // the text side's scratch, shared by every text stream of a forward
  DevBuf ws_pool_in, ws_pool_lin, ws_pool_f32, ws_time, ws_tfeat, ws_th1, ws_temb, ws_mod;
  DevBuf ws_xp, ws_vis, ws_h, ws_qk, ws_vt, ws_o, ws_ff, ws_y;
  DevBuf ws_vcos, ws_vsin, ws_pos;
  DevBuf ws_vel_c, ws_vel_u;
  DevBuf ws_win;                                   // a windowed run: the call's plan, the three int32 start vectors then the three fp32 weight tables
  // sequence parallelism (token shards): this rank owns rows [sp_rank*n_loc, (sp_rank+1)*n_loc) of the N visual
  // tokens; K and V^T of every block are all-gathered in place into ws_kfull [N][D] / ws_vtfull [P][D][n_loc]
  Comm comm;
  int sp_rank = 0, sp_world = 1;
  DevBuf ws_q, ws_kfull, ws_vtfull, ws_attn_state;
  // CFG-parallel (reference semantics generation_utils.py:53-76): this handle runs ONE branch of classifier-free
  // guidance — 0 = conditional, 1 = unconditional — and is paired with the handle that runs the other one (a 2-rank communicator of
  // its own, next to the sequence-parallel one).  Inside k5_sample the pair exchanges the bf16 velocities (one in-place all-gather of
  // 2 x T H W 16 x 2 B per step on a side stream) and both apply the identical bf16 combine + fp32 Euler update.
  Comm pair;
  int cfg_branch = -1;
  hipStream_t pair_stream = nullptr;
  hipEvent_t ev_vel_ready = nullptr, ev_vel_done = nullptr;
  DevBuf ws_vel_pair;                              // [2][T H W 16] bf16: slot 0 = conditional, 1 = unconditional velocity
  int fp8_fuse_ln = 1;                             // fp8 modes: the LayerNorm in front of an fp8 projection writes e4m3 directly (same bits as LayerNorm + quantisation pass)
  int fp8_mask = 0;                                // k5_dit_set_fp8: bit 0 feed-forward, bit 1 q | k | V^T projections, bit 2 out projection of the visual self-attention
  DevBuf ws_h8, ws_ff8;                            // fp8 activations of that path
  // Cross-attention keys / values of ALL visual blocks in one go (round 4, "cross_kv_batched"): they depend on the text stream only, so the 2 x
  // num_visual_blocks projections of 256 text rows (34 + 32 us each: 28-tile launches) become two GEMMs against the stacked weights
  // [blocks * D][D] before the visual stack, the key RMSNorms one launch — same kernels on the same per-element sums: bit-identical.  Every text
  // stream keeps the result in its own TextStream::ck_all / cvt_all
  Linear cx_k, cx_v;                               // to_key / to_value of every visual block's cross-attention, stacked: [blocks * D][D]
  DevBuf cx_knorm_all;
  int cross_kv_batched = 1;
  DevBuf ws_sched;                                 // sampler tables on the device: t*1000 [steps] | dt [steps] | step counter
  bool use_graph = false;                          // k5_sample replays one captured step (k5_dit_set_graph)
  hipStream_t graph_stream = nullptr;              // capture needs a real stream: the caller's may be the legacy null stream
  hipEvent_t ev_graph = nullptr;
  // The watch of k5_dit_set_watch (progress / cancel / previews out of the sampler loop).  Two slots, used alternately by the
  // steps: the callback of step i reads slot i & 1 while the preview of step i + 1 is written into the other.
  struct Watch {
    bool on = false;
    k5_watch_fn fn = nullptr; void* user = nullptr;
    int every = 0; bool want_x0 = false;
    DevBuf wb;                                     // device copy of rgb_w [C][3] | rgb_b [3]
    DevBuf rgb[2], x0[2];                          // device RGB (T,H,W,3) uint8 and x0 (T,H,W,C) fp32 of a slot
    uint8_t* h_rgb[2] = {nullptr, nullptr};        // pinned host copies of rgb[]
    size_t h_bytes = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};         // "step i and its preview are complete"
    int steps_done = 0, stopped = 0;               // of the last k5_sample* call (k5_dit_watch_state)
    int sample = 0, num_samples = 1;               // set by k5_sample_many around each sample
    // the per-call side, driven by sample_impl (defined next to it): begin, step(i) after step i is enqueued, end
    int begin(const SampleRun& r, const char* who);   // resets steps_done / stopped; watching: sizes the two slots and the pinned buffers
    bool preview_at(const SampleRun& r, int i) const;
    int step(const SampleRun& r, int i);              // enqueues the preview, its copy to the host and the slot's event; delivers step i - 1
    int deliver(const SampleRun& r, int i);           // step i's callback
    int end(const SampleRun& r);                      // the last delivery, and the drain of a stopped run
  } watch;
  DevBuf ws_kc;                                    // NABLA: keys pre-multiplied by the softmax scale (separate from the map's keys);
                                                   // under sequence parallelism the reverse: the rank's UNSCALED keys (the scaled ones are gathered)
  DevBuf ws_kmeans;                                // NABLA under sequence parallelism: gathered key-block means [P][H][slot blocks][64]
  DevBuf ws_attn_bal;                              // states of the split tail jobs (k5_launch_attention_bf16_range, balanced)
  // data-derived softmax bound of the visual self-attention (pre-scaled keys): per-head max |q|^2 [Hh] | max |k'|^2 [P][Hh]
  // (fp32, filled by the rmsnorm/RoPE kernel, consumed by k5_launch_attn_flags), the per-head variant flags [Hh] (int) and
  // two u64 counters: heads that ran the fixed-offset / the online-max kernel since the last reset
  DevBuf ws_attn_stats, ws_attn_flags, ws_attn_cnt, ws_attn_part;   // ws_attn_part: per-block partial maxima of the norm kernel
  long long nabla_possible = 0;                    // profiling: 64x64 blocks the NABLA maps could have kept (kept: ws_attn_cnt[2])
  int nabla_list_rows = 4;                         // rows per key-tile list of the last profiled map (ws_attn_cnt[3] = sum of list lengths)
  int attn_mode = 0;                               // K5_ATTN_AUTO / K5_ATTN_ONLINE (k5_dit_set_option "attn_mode")
  int sp_pass1_tiles = 0;                          // k5_dit_set_option "sp_pass1_tiles" (0 = all local key tiles)
  // "nabla_group_rows": 64-query rows per key-tile list = per attention workgroup (one GPU).  4: 256-query workgroups; 2: 128-query
  // workgroups (tighter lists: -17 % attention at kept density 0.05, -8 % at 0.12, +3 % at 0.81; bit-identical results); 0 (default):
  // chosen per forward from the kept density of the PREVIOUS forward's first map (counted on the device, copied to pinned host memory
  // without a synchronisation: a stale or missing value only costs speed)
  int nabla_group_rows = 0, nabla_grp_now = 4;
  // "nabla_pair_frames" (round 4): the two 64-query rows of a 128-query list are the same spatial tile in ADJACENT FRAMES (k5_pair_row) instead
  // of adjacent tiles of one frame: their sliding-tile windows share 10 of 11 frames.  Same arithmetic per row (a row's key tiles are walked
  // in the same ascending order), so outputs are bit-identical with it on or off.
  int nabla_pair_frames = 1;
  void* nabla_tap = nullptr; long long nabla_tap_cap = 0, nabla_tap_n = 0;   // k5_dit_set_nabla_tap: caller's device buffer, its size, maps taken so far
  int nabla_fuse_means = 1;   // the q / k block means come out of the norm + RoPE pass (k5_launch_rmsnorm_rope mean_q / mean_k); 0: their own pass (rounds 1-3)
  DevBuf ws_nabla_kept;                            // u64 kept-block count of the forward's first NABLA map
  unsigned long long* h_nabla_kept = nullptr;      // its pinned host copy
  long long nabla_hint_possible = 0;               // blocks that map could have kept
  bool nabla_hint_pending = false;
  int sp_nabla_passes = 1;                         // "sp_nabla_passes" = 2: NABLA under sequence parallelism attends the rank's own key blocks during the gather
  int fuse_qnorm = 0;                              // "attn_fuse_qnorm": norm_qk + RoPE of the visual queries inside the attention kernel
  // "attn_fuse_qnorm_auto" (default 1): k5_sample decides per CALL.  Step 0 runs with the standalone norm pass and collects whether any head left
  // the plain fixed-offset form (online, anchored, or marked as falling back: leave_sig); if none did, steps 1.. normalise the queries inside the
  // attention kernel (fuse_now) — the same bits (both kernels spell the norm + rotation out operation for operation), half of the norm pass less per
  // block and a faster attention instantiation.  Heads that
  // leave the window keep today's routing (anchored offsets need the normalised queries in memory), so such calls stay as they were.
  int fuse_qnorm_auto = 1;
  bool fuse_now = false, leave_collect = false;
  int fuse_last = -1;                              // "attn_fuse_qnorm_used": what the last k5_sample decided (1 fused from step 1 on, 0 not, -1 not evaluated)
  DevBuf ws_leave_sig;
  DevBuf ws_pref_snap;                             // k5_dit_forward_many: every block's AttnW::pref as the call found it
  unsigned int* h_leave_sig = nullptr;             // pinned
  bool row_offsets = true;                         // "attn_row_offsets": per-row offsets of the fixed-offset softmax (bound up to 190)
  bool anchor = true;                              // "attn_anchor": heads beyond that window run the fixed form on anchored offsets (one-GPU path)
  DevBuf ws_attn_anchor;                           // [H][rows] anchored offsets (k5_launch_attn_row_anchor)
  int sp_slices = 1;                               // "sp_slices": the K / V^T exchange of a block in this many slices (dense attention)
  int sp_mode = 0;                                 // "sp_mode": 0 = K / V^T all-gather (any rank count), 1 = Ulysses all-to-all (heads % ranks == 0, dense attention)
  DevBuf ws_u_send, ws_u_recv, ws_u_vsend, ws_u_vrecv, ws_u_o, ws_u_orecv, ws_u_stats;   // Ulysses exchange buffers
  hipEvent_t ev_u_o = nullptr, ev_u_back = nullptr;
  // two-level schedule ("sp_mode" = 2, run_self_attention_heads): the split's queries of the rank's head group, and the exchange plans of the
  // current shape (sp_plan_2d: SP_K, SP_VT, SP_Q, SP_O) — the other buffers are the Ulysses ones, grown to this schedule's sizes
  DevBuf ws_u_qrecv;
  std::vector<k5ipc::Xfer> sp_plan[4];
  int sp_plan_key[2] = {0, 0};                     // (world, rows_pad) the plans were made for
  int sp_mode_used = -1;                           // "sp_mode_used" (read-only): schedule of the last sharded forward (0 gather, 1 Ulysses, 2 two-level; -1 none yet)
  hipEvent_t ev_slice[4] = {};                     // slice s of every peer has landed
  bool emulated = false;                           // "emulate_world": timing-only layout, results are garbage
  bool last_nabla = false;                         // attention type of the last forward ("fp8_effective": Ulysses, which keeps q | k | V^T in bf16, is a dense-attention schedule)
  // Self-tuning sequence-parallel schedule (round 4): which exchange wins — one in-place all-gather per block, the sliced exchange, Ulysses
  // all-to-all; for NABLA one or two passes over the lists — is a property of the NODE (xGMI link rates, how RCCL drives them) that no
  // single-GPU box can measure.  So the first sharded forward of a handle (world > 1) times one block's self-attention section under
  // every admissible candidate on its own shapes, the ranks agree on max-over-ranks per candidate, and the fastest is kept for the life
  // of the handle.  Knobs the caller set explicitly are left alone, and only the knobs a run VARIED are assigned from its winner.
  // OPT-IN since round 5 ("sp_autotune" = 1, K5_SP_AUTOTUNE=1, bench.py --sp-autotune): the winner comes from wall-clock timings and the schedules
  // sum in different orders (one or two NABLA passes, gather / sliced exchange / Ulysses), so with it on the same seed may give different bits on
  // two nodes or two runs; off, a handle always runs the all-gather schedule unless told otherwise.
  bool sp_autotune = false, sp_tuned = false;
  int sp_user_set = 0;                             // bit 0: sp_mode, 1: sp_slices, 2: sp_nabla_passes were set through k5_dit_set_option
  std::string sp_report;                           // JSON text of the last tuning run (k5_dit_sp_schedule)
  DevBuf ws_tune;
  hipStream_t comm_stream = nullptr;              // all-gathers run here, overlapped with pass 1 of the attention
  hipEvent_t ev_k = nullptr, ev_v = nullptr, ev_gathered = nullptr, ev_stats = nullptr, ev_means = nullptr;
  // NABLA: fractal token permutation (cached per shape) and the selection workspace
  DevBuf ws_perm, ws_nabla; int perm_shape[3] = {0, 0, 0}; bool key_fractal = false;
  // rope cache keys
  std::vector<int32_t> key_vpos; float key_scale[3] = {0, 0, 0}; int key_shape[3] = {0, 0, 0};
  struct TextRope { std::vector<int32_t> key; DevBuf cosT, sinT, pos; };
  std::vector<TextRope> text_rope;  // small cache: cond / null-cond position vectors

  // Step-invariant text prologue: TextEmbeddings(text) and the pooled projection (dit.py:132,134) depend on the
  // prompt only, so k5_sample computes them once per call and branch (slot 0 = cond, 1 = uncond) and every later step copies
  // 0.9 MB instead of re-running two GEMMs + two LayerNorms.  k5_dit_forward (one call per step, caller-owned buffers that
  // may change between calls) does not cache.
  struct TextCache { DevBuf text, pool; bool valid = false; int L = 0; } text_cache[3 + 8 + 2];   // [2]: the negative prompt of k5_dit_set_nag (text only); [3 + r]: region r of k5_dit_set_regions (likewise); [11], [12]: FlowEdit's source side (kFlowEditSlot)
  static constexpr int kFlowEditSlot = 3 + 8;      // the source prompt; the negative prompt is one prompt for both sides and keeps slot 1, so slot 12 stays empty
  void drop_text_cache() { for (auto& t : text_cache) t.valid = false; }

  // FlowEdit (k5_sample_flowedit): the call's workspaces — zs / zt, the two forwards' inputs of a step, and the source side's two
  // velocities (the target side's are ws_vel_c / ws_vel_u) — and what k5_dit_flowedit_state reports.  `active` brackets a call: the text
  // prologues computed meanwhile are counted.
  struct FlowEdit {
    DevBuf zs, zt, vel_c, vel_u;
    long long steps = 0, forwards = 0, prologues = 0;
    bool active = false;
  } fe;

  // What one prompt leaves behind in a forward: every prompt — the forward's own, the negative one of k5_dit_set_nag, a region's of
  // k5_dit_set_regions — goes through the text blocks into a stream of its own (text_stream_run) and from there into every visual block's
  // cross-attention (cross_view, run_cross_attention).  A stream's buffers are sized by its own L and exist once a forward has used it.
  struct TextStream {
    int L = 0;                                     // rows of the prompt that last went through
    DevBuf text;                                   // its rows after the text blocks, [L][D]
    DevBuf ck_all, cvt_all;                        // "cross_kv_batched": normalised keys [L][blocks * D] and V^T [blocks * D][rup(L, 8)] of all visual blocks
    DevBuf ck, cvt;                                // otherwise: one block's keys [L][D] and V^T [D][rup(L, 8)], projected by the block itself
    void release() { for (DevBuf* b : {&text, &ck_all, &cvt_all, &ck, &cvt}) b->release(); }
  } streams[1 + 1 + 8];                            // [0]: the forward's own prompt (cond and uncond alike); [1]: the negative prompt; [2 + r]: region r
  // the slot of text_cache that keeps stream k's TextEmbeddings during a k5_sample* call: stream 0 has one per CFG branch (text_slot 0 / 1)
  TextCache* stream_cache(int k, int text_slot) { return text_slot < 0 ? nullptr : &text_cache[k == 0 ? text_slot : 1 + k]; }

  // Normalized attention guidance (k5_dit_set_nag): the negative prompt is text stream 1 and, per visual block, a second
  // cross-attention of the same queries joined to the first by k5_launch_nag_combine.  Conditional forwards only (text_slot != 1).
  struct Nag {
    bool on = false;
    const k5_text_cond* neg = nullptr;             // borrowed: valid until cleared, read at every forward
    float scale = 1.f, tau = 1.f, alpha = 0.f;
    long long combines = 0;                        // k5_launch_nag_combine launches enqueued so far (k5_dit_nag_state)
    DevBuf o;                                      // the negative stream's attention output [n][D]; exists once a guided forward has run
  } nag;

  // Regional prompts (k5_dit_set_regions): region r's prompt is text stream 2 + r and, per visual block, one more cross-attention
  // of the same queries; k5_launch_region_combine joins the R + 1 outputs by per-token weights in front of the out projection (and of the NAG
  // combine, if that is set too).  Conditional forwards only.  o and w exist once such a forward has run.
  struct Regions {
    bool on = false;
    int R = 0;
    const k5_text_cond* conds = nullptr;           // HOST [R], borrowed: valid until cleared, read at every forward
    const float* masks = nullptr;                  // device fp32 [R][T][H][W], borrowed
    int T = 0, H = 0, W = 0;
    float base_weight = 0.f;
    long long combines = 0;                        // k5_launch_region_combine launches enqueued so far (k5_dit_regions_state)
    DevBuf o;                                      // the regions' attention outputs, [R][n][D]
    DevBuf w; int w_order = -1;                    // token weights [N][R + 1] of this region set; -1: not computed, 0: row-major tokens, 1: NABLA's perm order
  } regions;

  // The guidance plan of k5_dit_set_guidance: per-step weights, CFG-Zero* (projected scale, zero-init of the first steps) and
  // CFG rescale.  Read by sample_impl only; off = the call's guidance_weight at every step through the launches it always made.
  struct Guidance {
    bool on = false;
    std::vector<float> weights;                    // [num_steps] of the calls to come (copied at set time); empty: the call's guidance_weight
    bool zero_star = false; int zero_init = 0; float rescale = 0.f;
    long long guided = 0, unguided = 0, zero = 0;  // steps enqueued so far by kind (k5_dit_guidance_state)
    DevBuf ws;                                     // sums double[5] | ab float[2] at byte 48 | part [blocks][5] doubles at byte 64
    bool stats() const { return zero_star || rescale > 0.f; }   // the step needs the coefficients from the device
  } guide;

  // Skip-layer guidance (k5_dit_set_skip_guidance): a third velocity from the conditional forward with some visual blocks skipped.
  // ForwardRun forks at the first skipped block (visual_blocks / skip_branch); sample_impl decides per step.  on: a set is held; live(): it also has a scale.
  struct Skip {
    bool on = false;
    std::vector<char> skipped;                     // [num_visual_blocks] 0 / 1
    int k0 = 0, mode = 0; float scale = 0.f;       // k0: the smallest skipped index
    std::vector<unsigned char> steps;              // per-step mask of the calls to come; empty: every step
    int share_prefix = 1;                          // option "skip_share_prefix"
    long long skip_steps = 0, blocks_shared = 0, blocks_run = 0;
    DevBuf vis;                                    // the conditional forward's visual stream [n][D] as it entered block k0
    DevBuf vel;                                    // the sampler's third velocity
    bool live() const { return on && scale > 0.f; }
    bool at(int i) const { return live() && (steps.empty() || steps[i] != 0); }
  } skip;

  // Stochastic sampling (k5_dit_set_stochastic): per-step dt_down / scale / noise_coef and the key of the in-kernel generator.
  // sample_impl writes dt_down where the schedule's dt stands and hands the rest to the update kernel; no buffer, no state.
  struct Stochastic {
    bool on = false;
    std::vector<float> dt_down, scale, coef;       // [num_steps] of the calls to come
    uint64_t seed = 0; uint32_t first_stream = 0;
    long long noisy_steps = 0;
  } sto;

  // Enhance-A-Video (k5_dit_set_enhance): per visual block the cross-frame attention score of the normalised q | k, and the
  // attention output times that score in front of the out projection.  sample_impl sets `gate` per step; ForwardRun decides `live` for the
  // forward (and the column table under NABLA, token_order), its block() names the score's slot, run_self_attention enqueues.
  struct Enhance {
    bool on = false;
    float weight = 0.f;
    std::vector<unsigned char> steps;              // per-step mask of the calls to come; empty: every step
    int gate = -1;                                 // inside k5_sample*: whether the current step applies it (0 / 1); -1: a forward of its own
    bool live = false;                             // this forward applies it
    int T = 0, S = 0, block = 0;                   // the forward's frames and spatial positions; the visual block being run
    const int32_t* rows = nullptr;                 // the forward's frame_rows (NABLA's fractal order) or nullptr
    long long launches = 0;                        // score launches enqueued so far (k5_dit_enhance_state)
    int last_blocks = 0;                           // scores the last forward left
    hipStream_t last_stream = nullptr;
    DevBuf scores, part, frame_rows;               // fp32 [num_visual_blocks] | double [S Hh] | int32 [S][T]
    int rows_shape[3] = {0, 0, 0};                 // the (T, H/2, W/2) frame_rows was built for
    bool at(int i) const { return on && (steps.empty() || steps[i] != 0); }
    // a forward of `frames` frames applies it: it is set, the sampler's step (if any) has it on and there is more than one frame
    bool applies(int frames, int blocks) const { return on && gate != 0 && frames >= 2 && blocks > 0; }
  } enh;

  // MagCache (reference kandinsky/magcache_utils.py:16-101): skip the visual blocks on some calls and re-apply the
  // cached bf16 residual of the same cond / uncond slot.  Decisions depend on the ratio table and the call counter only.
  struct MagCache {
    bool on = false, no_cfg = false;
    std::vector<double> table;                     // [2 * num_steps], already interpolated by the host mirror
    double thresh = 0.12, retention = 0.2;
    int K = 2, cnt = 0;
    int first = 0, stride = 1;                     // which calls of the reference's sequence this handle sees
    double acc_err[2] = {0, 0}, acc_ratio[2] = {1, 1};
    int acc_steps[2] = {0, 0};
    DevBuf residual[2]; size_t res_elems[2] = {0, 0};
    DevBuf pm_one;                                 // fp32 [+1 x D | -1 x D]
    long long n_ran = 0, n_skipped = 0;
    int slot() const { return cnt & 1; }           // the cond / uncond slot of the call to come
    void reset_acc() { for (int j = 0; j < 2; ++j) { acc_ratio[j] = 1.0; acc_err[j] = 0; acc_steps[j] = 0; } }
    // does the call to come skip its visual blocks (magcache_utils.py:59-76)?  float64 like the reference's numpy scalars
    bool decide() {
      const int j = slot();
      if (cnt < (int)((double)table.size() * retention)) return false;
      acc_ratio[j] *= table[cnt]; acc_steps[j] += 1; acc_err[j] += std::fabs(1.0 - acc_ratio[j]);
      if (acc_err[j] < thresh && acc_steps[j] <= K) return true;
      acc_err[j] = 0; acc_steps[j] = 0; acc_ratio[j] = 1.0;
      return false;
    }
    void advance() { cnt += stride; if (cnt >= (int)table.size()) { cnt = first; reset_acc(); } }   // the end of a call (:91-100)
  } mag;

  // MagCache calibration (k5_dit_set_magcache_calibrate): every call runs its blocks and leaves the statistics of its residual against the
  // previous residual of its slot in table[cnt][4] (device, float64, accumulated over runs).  Per slot two residual buffers, previous | current.
  struct MagCalib {
    bool on = false, no_cfg = false;
    int num_steps = 0, cnt = 0;
    long long runs = 0;                            // complete runs (counter wrap-arounds) the table holds
    DevBuf res[2][2]; int prev[2] = {0, 0};        // res[slot][prev[slot]] = the slot's previous residual
    size_t res_elems[2] = {0, 0};
    DevBuf table, part;                            // [2 * num_steps][4] | per-workgroup partials of the pass
    hipStream_t last_stream = nullptr;
    int slot() const { return cnt & 1; }
    int cur() const { return prev[slot()] ^ 1; }   // the slot's buffer the call to come fills
  } cal;

  // The forecast cache (k5_dit_set_forecast; the rule is written at k5_forecast_update_bf16 in include/k5.h): on the plan's forecast steps
  // the visual blocks are skipped and their residual is extrapolated from the slot's finite differences.  Decisions depend on the step only.
  struct Forecast {
    bool on = false, mixed = false;                // mixed: the plan has a 0 (a plan of ones is off: k5_sample* runs plain forwards)
    int order = 1;
    std::vector<unsigned char> full;               // [num_steps], full[0] = 1
    DevBuf F0[2], D1[2], D2[2], ori;               // per slot bf16 | fp32 | fp32 [n][D]; ori bf16 [n][D], one per handle
    int j[2] = {-1, -1}, have[2] = {0, 0};         // per slot: the step of its last full call, its full calls so far in this run
    int gap[2] = {1, 1}, gap_prev[2] = {1, 1};     // per slot: the steps between its last two full calls, and between the two before
    size_t elems[2] = {0, 0};                      // n x D of the slot's state
    int at_step = -1, at_slot = 0;                 // k5_dit_forecast_at's cursor (-1: none)
    long long full_calls = 0, forecast_calls = 0;
    hipStream_t last_stream = nullptr;
    void clear_history() { for (int k = 0; k < 2; ++k) { j[k] = -1; have[k] = 0; gap[k] = gap_prev[k] = 1; } at_step = -1; }
    long long state_bytes() const {
      size_t b = ori.bytes;
      for (int k = 0; k < 2; ++k) b += F0[k].bytes + D1[k].bytes + D2[k].bytes;
      return (long long)b;
    }
  } fc;

  // LoRA adapters merged into the packed weights (k5_dit_add_lora): the packed bits of every touched matrix as they were before the first
  // merge, keyed by the matrix's address (a region of a fused / stacked buffer counts as its own matrix); k5_dit_clear_lora copies them back
  struct LoraBackup { DevBuf copy; size_t bytes = 0; Linear* lin = nullptr; };   // lin: the layer the matrix belongs to (its e4m3 copy follows the bf16 bits); null: an fp32 matrix
  std::map<void*, LoraBackup> lora_backup;

  // profiling
  int profiling = 0;                               // 0 off, 1 every kernel family, 2 only the visual self-attention (the roofline kernel)
  std::map<std::string, Prof> prof;
  long long prof_self_blocks = 0;                  // visual blocks whose self-attention ran while profiling was on ("self_blocks")
  struct Pending { std::string fam; hipEvent_t a, b; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> ev_pool;

  ~k5_dit() {
    for (auto& e : ev_pool) (void)hipEventDestroy(e);
    for (auto& pnd : pending) { (void)hipEventDestroy(pnd.a); (void)hipEventDestroy(pnd.b); }
  }
};

namespace {

// ---------------------------------------------------------------------------------------------
// profiling helpers: bracket a kernel family with events on the engine stream
// ---------------------------------------------------------------------------------------------
hipEvent_t get_event(k5_dit* d) {
  if (!d->ev_pool.empty()) { hipEvent_t e = d->ev_pool.back(); d->ev_pool.pop_back(); return e; }
  hipEvent_t e; (void)hipEventCreate(&e); return e;
}
struct Scope {
  k5_dit* d; hipStream_t s; const char* fam; hipEvent_t a{}, b{}; bool on;
  Scope(k5_dit* d_, hipStream_t s_, const char* f) : d(d_), s(s_), fam(f), on(d_->profiling == 1 || (d_->profiling == 2 && !strcmp(f, "attn_self"))) {
    if (on) { a = get_event(d); b = get_event(d); (void)hipEventRecord(a, s); }
  }
  ~Scope() { if (on) { (void)hipEventRecord(b, s); d->pending.push_back({fam, a, b}); } }
};
void drain_profile(k5_dit* d) {
  for (auto& p : d->pending) {
    (void)hipEventSynchronize(p.b);
    float ms = 0; (void)hipEventElapsedTime(&ms, p.a, p.b);
    auto& e = d->prof[p.fam]; e.ms += ms; e.n += 1;
    d->ev_pool.push_back(p.a); d->ev_pool.push_back(p.b);
  }
  d->pending.clear();
}

// ---------------------------------------------------------------------------------------------
// expected state_dict keys (dit.py:100-127)
// ---------------------------------------------------------------------------------------------
void expected_keys(const k5_dit_config& c, std::vector<std::string>& out) {
  auto lin = [&](const std::string& n, bool bias = true) {
    out.push_back(n + ".weight");
    if (bias) out.push_back(n + ".bias");
  };
  lin("time_embeddings.in_layer"); lin("time_embeddings.out_layer");
  lin("text_embeddings.in_layer"); out.push_back("text_embeddings.norm.weight"); out.push_back("text_embeddings.norm.bias");
  lin("pooled_text_embeddings.in_layer"); out.push_back("pooled_text_embeddings.norm.weight"); out.push_back("pooled_text_embeddings.norm.bias");
  lin("visual_embeddings.in_layer");
  auto attn = [&](const std::string& p) {
    lin(p + ".to_query"); lin(p + ".to_key"); lin(p + ".to_value");
    out.push_back(p + ".query_norm.weight"); out.push_back(p + ".key_norm.weight");
    lin(p + ".out_layer");
  };
  for (int i = 0; i < c.num_text_blocks; ++i) {
    const std::string p = "text_transformer_blocks." + std::to_string(i);
    lin(p + ".text_modulation.out_layer"); attn(p + ".self_attention");
    lin(p + ".feed_forward.in_layer", false); lin(p + ".feed_forward.out_layer", false);
  }
  for (int i = 0; i < c.num_visual_blocks; ++i) {
    const std::string p = "visual_transformer_blocks." + std::to_string(i);
    lin(p + ".visual_modulation.out_layer"); attn(p + ".self_attention"); attn(p + ".cross_attention");
    lin(p + ".feed_forward.in_layer", false); lin(p + ".feed_forward.out_layer", false);
  }
  lin("out_layer.modulation.out_layer"); lin("out_layer.out_layer");
}

// upload helpers ---------------------------------------------------------------------------
int upload_f32(DevBuf& b, const float* src, size_t n) {
  K5CHK(b.ensure(n * 4));
  HIPCHK(hipMemcpy(b.p, src, n * 4, hipMemcpyHostToDevice));
  return K5_OK;
}
int upload_bias_bf16r(DevBuf& b, const float* src, size_t n) {  // fp32 array of bf16-rounded values
  std::vector<float> tmp(n);
  for (size_t i = 0; i < n; ++i) tmp[i] = bf16_round_host(src[i]);
  return upload_f32(b, tmp.data(), n);
}

// staged matrix -> rows [row0, row0 + rows) of dst [total_rows][ld] (bf16 or fp32), on the device
int pack_rows(DevBuf& dst, bool bf16, const HostTensor* t, size_t rows, size_t cols, size_t ld, size_t row0 = 0, size_t total_rows = 0) {
  if (!t || !t->dev.p || t->count() != rows * cols) { k5_set_error("internal: matrix not staged on the device"); return K5_ERR_STATE; }
  if (total_rows == 0) total_rows = rows;
  const size_t es = bf16 ? 2 : 4;
  // packed bf16 weights are GEMM operands (the A side in the V^T form, where 1792 rows are ragged for the 192-row tile): guard rows behind them
  K5CHK(dst.ensure(total_rows * ld * es, bf16 ? (size_t)K5_GEMM_GUARD_ROWS * ld * es : 0));
  return k5_launch_pack_matrix(t->dev.p, t->dtype, (char*)dst.p + row0 * ld * es, bf16 ? 1 : 0, (int64_t)rows, (int)cols, (int)ld, nullptr);
}
int pack_f32(DevBuf& dst, const HostTensor* t, size_t rows, size_t cols, size_t row0 = 0, size_t total_rows = 0) {
  return pack_rows(dst, false, t, rows, cols, cols, row0, total_rows);
}

const HostTensor* find(k5_dit* d, const std::string& k) {
  auto it = d->staged.find(k);
  return it == d->staged.end() ? nullptr : &it->second;
}

// shape check of one staged tensor: [r][c], or [r] when c == 0 (a mismatched tensor handed through the C ABI must come back as
// K5_ERR_ARG, not as an out-of-bounds host read while packing)
bool shape_ok(k5_dit* d, const std::string& k, size_t r, size_t c) {
  const HostTensor* t = find(d, k);
  const bool ok = t && ((c == 0 && t->shape.size() == 1 && (size_t)t->shape[0] == r) ||
                        (c && t->shape.size() == 2 && (size_t)t->shape[0] == r && (size_t)t->shape[1] == c));
  if (!ok) k5_set_error("shape mismatch for %s", k.c_str());
  return ok;
}

// One packed layer from the staged state_dict: `<prefix>.weight` [n][K] into bf16 rows of ld >= K elements and, unless the layer has none,
// `<prefix>.bias` [n] bf16-rounded — both shape-checked.  Several prefixes: those layers stacked along the output channels in the order given
// (to_query over to_key; one matrix of every visual block).
int load_linear(k5_dit* d, Linear& l, const std::vector<std::string>& prefixes, size_t n, size_t K, size_t ld, bool bias = true) {
  const size_t total = prefixes.size() * n;
  std::vector<float> b(total);
  for (size_t i = 0; i < prefixes.size(); ++i) {
    const std::string& p = prefixes[i];
    if (!shape_ok(d, p + ".weight", n, K) || (bias && !shape_ok(d, p + ".bias", n, 0))) return K5_ERR_ARG;
    K5CHK(pack_rows(l.w, true, find(d, p + ".weight"), n, K, ld, i * n, total));
    if (bias) memcpy(b.data() + i * n, find(d, p + ".bias")->data.data(), n * 4);
  }
  if (bias) K5CHK(upload_bias_bf16r(l.b, b.data(), total));
  l.N = (int)total; l.K = (int)K; l.ld = (int)ld;
  return K5_OK;
}

// self: the module projects its own keys and values (q | k stacked); otherwise they come from the stacks of all visual blocks (k5_dit_finalize)
int pack_attn(k5_dit* d, const std::string& p, AttnW& a, bool self) {
  const size_t D = d->D;
  if (self) {
    K5CHK(load_linear(d, a.wqk, {p + ".to_query", p + ".to_key"}, D, D, D));
    K5CHK(load_linear(d, a.wv, {p + ".to_value"}, D, D, D));
  } else K5CHK(load_linear(d, a.wq, {p + ".to_query"}, D, D, D));
  K5CHK(load_linear(d, a.wo, {p + ".out_layer"}, D, D, D));
  if (!shape_ok(d, p + ".query_norm.weight", 64, 0) || !shape_ok(d, p + ".key_norm.weight", 64, 0)) return K5_ERR_ARG;
  const HostTensor *nq = find(d, p + ".query_norm.weight"), *nk = find(d, p + ".key_norm.weight");
  std::vector<float> n(128);
  memcpy(n.data(), nq->data.data(), 64 * 4); memcpy(n.data() + 64, nk->data.data(), 64 * 4);
  K5CHK(upload_f32(a.norm, n.data(), 128));
  float mq = 0.f, mk = 0.f;
  for (int i = 0; i < 64; ++i) { mq = fmaxf(mq, fabsf(n[i])); mk = fmaxf(mk, fabsf(n[64 + i])); }
  a.score_bound = 64.f * mq * mk * 1.05f;  // 5 % margin for the bf16 roundings after RMSNorm / RoPE
  return K5_OK;
}

inline size_t rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The visual self-attention runs with the keys pre-multiplied by log2(e)/8 (attn_fwd_kernel<.., PRE>: the scores are the exp2
// arguments) whenever the rows come in whole 64-key tiles.  Which softmax form a head takes — constant offset 0, or the lazy
// online max — is decided ON THE DEVICE from the data: the rmsnorm/RoPE kernel leaves max |q_h|^2 and max |k'_h|^2, and
// k5_launch_attn_flags turns |q|max |k'|max <= 90 into the per-head flag both attention launches read.  (Round 1 derived
// the bound from the QK-norm weights, 64 max|w_q| max|w_k|, which no trained checkpoint is known to satisfy.)
// Text and cross attention (tiny) keep the weight-derived bound + the 32x32 online kernel as their fallback.
constexpr float K5_SOFTMAX_C = 0.125f * 1.44269504088896340736f;

int ensure_zeroed(DevBuf& b, size_t n, hipStream_t s) {
  if (n <= b.bytes) return K5_OK;
  K5CHK(b.ensure(n));
  HIPCHK(hipMemsetAsync(b.p, 0, b.bytes, s));
  return K5_OK;
}
// statistics / flags / counters of the data-derived softmax bound; layout of ws_attn_stats: [q: Hh][k: sp_world x Hh]
int ensure_attn_flags(k5_dit* d, hipStream_t s) {
  K5CHK(ensure_zeroed(d->ws_attn_stats, (size_t)d->Hh * (2 + d->sp_world) * 4, s));   // + [r: Hh] squared key radii (one GPU: centred offsets)
  K5CHK(d->ws_attn_flags.ensure((size_t)d->Hh * (3 + 64) * 4));   // int flags[H] | float kmax[H] | krad[H] | centre[H][64] (per-row offsets of the fixed-offset form)
  K5CHK(d->ws_attn_part.ensure(k5_rmsnorm_stats_workspace_bytes(2 * d->Hh)));
  K5CHK(ensure_zeroed(d->ws_attn_cnt, 32, s));
  return K5_OK;
}

// ---------------------------------------------------------------------------------------------
// one attention module on `rows` tokens:  x_resid += gate * out_l(attn(...)) fused in the out GEMM
// ---------------------------------------------------------------------------------------------
struct NablaArgs { int T, Hb, Wb, wT, wH, wW; float P; };

// the forward's first NABLA map (nqb query-block rows x nb key blocks per head, in ws_nabla): its kept density steers the NEXT forward's
// attention workgroup size (nabla_group_rows = 0)
int nabla_density_hint(k5_dit* d, int H, int nqb, int nb, hipStream_t s) {
  if (!d->nabla_hint_pending || d->nabla_group_rows != 0) return K5_OK;
  d->nabla_hint_pending = false;
  K5CHK(d->ws_nabla_kept.ensure(8));
  if (!d->h_nabla_kept) { HIPCHK(hipHostMalloc((void**)&d->h_nabla_kept, 8, hipHostMallocDefault)); *d->h_nabla_kept = 0ull; }
  HIPCHK(hipMemsetAsync(d->ws_nabla_kept.p, 0, 8, s));
  K5CHK(k5_launch_nabla_count(d->ws_nabla.p, H, nqb, nb, d->ws_nabla_kept.as<unsigned long long>(), s));
  HIPCHK(hipMemcpyAsync(d->h_nabla_kept, d->ws_nabla_kept.p, 8, hipMemcpyDeviceToHost, s));
  d->nabla_hint_possible = (long long)H * nqb * nb;
  return K5_OK;
}

// do the q | k | V^T projections of the VISUAL self-attention take the e4m3 activations (k5_dit_set_fp8 bit 1)?  One rule for the callee and for
// the block loop, which then lets the LayerNorm write ws_h8 directly (h8_ready) instead of a bf16 h + a quantisation pass
bool sa_fp8_in(const k5_dit* d, const AttnW& a, int rows) {
  return (d->fp8_mask & 2) && a.wqk.has_e4m3() && rows >= 256 && !((int)rup(rows, 8) & 15);
}
bool sa_sp_fp8_in(const k5_dit* d, const AttnW& a, int rows, int rows_pad, bool nabla) {
  const int P = d->sp_world;
  return (d->fp8_mask & 2) && a.wqk.has_e4m3() && rows >= 256 && !((rows_pad / ((!nabla && d->sp_slices > 1 && P > 1) ? d->sp_slices : 1)) & 15);
}
// "nabla_fuse_means": the fused form gives every thread 64 consecutive rows of one 16-byte column chunk, i.e. the launch has rows / 64 x heads x 8
// threads — a sequence-parallel shard of the 10 s clip (366 blocks x 28 heads: 82 k threads, a sixth of the resident capacity) runs it latency-
// bound and loses 3 ms per step to gain 1 (measured, incl. an 8-deep prefetch ring); from ~150 k threads up it wins.  2 = always.
// bytes of the NABLA workspace for nqb selected rows of nb: the lists are per group of >= 2 rows unless "nabla_group_rows" = 1 was asked for
size_t nabla_ws_bytes(const k5_dit* d, int H, int nb, int nqb) {
  const int gmin = d->nabla_group_rows == 1 ? 1 : 2;
  return k5_nabla_workspace_bytes(H, nb, nqb, (nqb + gmin - 1) / gmin);
}
bool nabla_means_fused(const k5_dit* d, int rows, int heads) {
  return d->nabla_fuse_means == 2 || (d->nabla_fuse_means == 1 && (long long)(rows / 64) * heads * 8 >= 150000);
}
bool ff_fp8_in(const k5_dit* d, const BlockW& b, int rows) { return (d->fp8_mask & 1) && b.w1.has_e4m3() && rows >= 256; }

// ---- the steps the self-attention schedules share ----
// Softmax form per head, decided from the data (by_data): k5_launch_attn_flags turns the |q|^2 / |k'|^2 maxima the norm passes left into the
// per-head flags both attention launches read.  With per-row softmax offsets ("row_offsets") heads with a Cauchy-Schwarz bound up to 190 keep
// the fixed-offset kernel, each query row on its own constant offset |q| max|k'| - 90 (kmax), and the module's prefer-online table of this
// branch (pref) is read here and updated after the attention (attn_pref_update).  Heads beyond the window: anchored offsets (anchor), sampled
// by k5_launch_attn_row_anchor — dense attention only, and it needs the normalised queries in memory (not with the fused query norm).
struct SoftmaxFormIn {
  float* qstat = nullptr; float* kstat = nullptr;      // per head nq / nk partial maxima at strides qstride / kstride floats
  int nk = 1, kstride = 0, nq = 1, qstride = 0;
  int heads = 0, head0 = 0;                            // heads decided here; index of the first in the prefer-online table
  float* centre = nullptr; float* rstat = nullptr;     // one GPU: the keys' centre and squared radii the norm pass left -> centred offsets (K5KeyCentre)
  unsigned int* leave_sig = nullptr;                   // one GPU
  hipEvent_t stats_ready = nullptr;                    // sharded: the gathered statistics arrive with this event
  hipEvent_t data_ready = nullptr;                     // head-parallel: q / k' / V^T arrive with this event (waited for after the flags, by_data or not)
  bool anchor = false;
  const void* aq = nullptr; const void* ak = nullptr;  // the anchor's queries and the keys it samples (the gather: the rank's OWN keys, in place before
  int aq_rows = 0, ak_rows = 0, ldq = 0, ldk = 0, key0 = 0, kv_total = 0;   // the gather); key0 = key index of query row 0's token
  const char* anchor_fam = nullptr;                    // profiling family of the anchor launch where it does not sit inside a scope already
};
struct SoftmaxForm {
  const int* hflags = nullptr; const float* kmax = nullptr; int* pref = nullptr;
  K5KeyCentre kcen{nullptr, nullptr, nullptr};
  bool centred = false;                                // kcen carries a centre + radius and / or row anchors
  const K5KeyCentre* key_centre() const { return centred ? &kcen : nullptr; }
};
int softmax_form(k5_dit* d, hipStream_t s, const AttnW& a, int pref_slot, bool by_data, const SoftmaxFormIn& in, SoftmaxForm& f) {
  const int H = d->Hh;
  if (by_data) {
    if (in.stats_ready) HIPCHK(hipStreamWaitEvent(s, in.stats_ready, 0));
    f.hflags = d->ws_attn_flags.as<int>();
    float* kmax_w = d->row_offsets ? d->ws_attn_flags.as<float>() + H : nullptr;
    f.kmax = kmax_w;
    if (kmax_w) { K5CHK(ensure_zeroed(a.pref, (size_t)3 * H * 4, s)); f.pref = a.pref.as<int>() + (size_t)pref_slot * H + in.head0; }
    K5CHK(k5_launch_attn_flags(in.qstat, in.kstat, in.nk, in.kstride, in.heads, 0, d->ws_attn_flags.as<int>(), d->ws_attn_cnt.as<unsigned long long>(), s, kmax_w,
                               f.pref, in.centre ? in.rstat : nullptr, in.centre ? kmax_w + H : nullptr, in.nq, in.qstride, kmax_w && in.anchor, in.leave_sig));
    if (in.centre) { f.kcen.centre = in.centre; f.kcen.radius = kmax_w + H; f.centred = true; }
  }
  if (in.data_ready) HIPCHK(hipStreamWaitEvent(s, in.data_ready, 0));
  if (f.kmax && in.anchor) {
    K5CHK(d->ws_attn_anchor.ensure((size_t)in.heads * in.aq_rows * 4));
    std::optional<Scope> sc;
    if (in.anchor_fam) sc.emplace(d, s, in.anchor_fam);
    K5CHK(k5_launch_attn_row_anchor(in.aq, in.ak, in.heads, in.aq_rows, in.ak_rows, in.ldq, in.ldk, in.key0, in.kv_total, f.kmax, d->ws_attn_anchor.as<float>(), s));
    f.kcen.row_anchor = d->ws_attn_anchor.as<float>();
    f.centred = true;
  }
  return K5_OK;
}
// 64-query rows per key-tile list = per workgroup of a NABLA attention launch (4: the 256-query form, which every dense launch uses too).
// Sharded: the 128- / 64-query workgroups only without the two-pass machinery, which lives on the 256-query form.
int attn_group_rows(const k5_dit* d, bool nabla, bool sharded) {
  if (!nabla) return 4;
  return (!sharded || (d->nabla_grp_now < 4 && d->sp_nabla_passes == 1)) ? d->nabla_grp_now : 4;
}
// after the attention: a head more than a quarter of whose (head, query block) jobs fell back goes to the online form the next time
int attn_pref_update(k5_dit* d, hipStream_t s, const SoftmaxForm& f, int heads, int q_rows, int group_rows, unsigned int* leave_sig = nullptr) {
  if (!f.kmax) return K5_OK;
  return k5_launch_attn_pref_update(d->ws_attn_bal.as<float>(), heads, q_rows, group_rows, f.pref, s, leave_sig);
}
// The rows x [rows][D] as a projection takes them.  want (the caller's shape rule): in e4m3 too, in ws_h8 — quantised here unless the LayerNorm
// already wrote them there (ready; there is no bf16 x then).  A bf16 projection must not have been promised e4m3 rows.
int e4m3_rows(k5_dit* d, hipStream_t s, const void* x, int rows, bool want, bool ready, Act& act) {
  const int D = d->D;
  act = Act{x, nullptr, rows, D};
  if (ready && !want) { k5_set_error("internal: e4m3 activations handed to a bf16 projection"); return K5_ERR_ARG; }
  if (!want) return K5_OK;
  K5CHK(d->ws_h8.ensure((size_t)rows * D, (size_t)K5_GEMM_GUARD_ROWS * D));
  if (!ready) {
    Scope sc(d, s, "elementwise");
    K5CHK(k5_launch_quant_rows_fp8(x, d->ws_h8.p, nullptr, rows, D, D, D, s));
  }
  act.e4 = d->ws_h8.p;
  return K5_OK;
}
// x_resid += gate * out_l(o), fused in the out GEMM; f8_out: e4m3 activations (opt-in, k5_dit_set_fp8 bit 2)
int attn_out_projection(k5_dit* d, hipStream_t s, const AttnW& a, const void* o, int rows, void* resid, const float* gate, bool f8_out = false) {
  Act x;
  K5CHK(e4m3_rows(d, s, o, rows, f8_out, false, x));
  LinearArgs g(a.wo, x, resid, d->D, s);
  g.epi = K5_EPI_GATE; g.resid = resid; g.ldr = d->D; g.gate = gate;
  Scope sc(d, s, "gemm");
  return linear(g);
}

int run_self_attention(k5_dit* d, hipStream_t s, const AttnW& a, const void* h, int rows, void* qk, void* vt,
                       void* o, const float* cosT, const float* sinT, void* resid, const float* gate,
                       const char* fam_attn, const NablaArgs* nabla = nullptr, int pref_slot = 0, bool h8_ready = false) {
  const int D = d->D, H = d->Hh;
  const int ldvt = (int)rup(rows, 8);
  const bool vis = !strcmp(fam_attn, "attn_self");
  const bool f8_in = vis && sa_fp8_in(d, a, rows);   // opt-in lossy mode: e4m3 projections (gemm_fp8.hip)
  const bool f8_out = vis && (d->fp8_mask & 4) && a.wo.has_e4m3() && rows >= 256;
  {
    Act x;
    K5CHK(e4m3_rows(d, s, h, rows, f8_in, h8_ready, x));
    LinearArgs gv(a.wv, x, vt, ldvt, s);
    gv.weights_as_rows = true;
    Scope sc(d, s, "gemm");
    K5CHK(linear(LinearArgs(a.wqk, x, qk, 2 * D, s)));
    K5CHK(linear(gv));
  }
  const bool pre = vis && rows % 64 == 0;   // visual blocks only (not the text blocks)
  const bool by_data = pre && d->attn_mode == K5_ATTN_AUTO;            // per-head flags from the data
  SoftmaxForm sf;
  // dense visual blocks: norm_qk + RoPE of the queries happen in the attention kernel's Q load ("attn_fuse_qnorm")
  // Enhance-A-Video reads the normalised q from memory: the standalone pass, whatever "attn_fuse_qnorm" says (the same bits)
  const bool enhance = vis && d->enh.live;
  const bool fuse_q = pre && !nabla && !enhance && (d->fuse_qnorm || d->fuse_now) && ((by_data && d->row_offsets) || d->attn_mode == K5_ATTN_ONLINE);
  unsigned int* leave_sig = (d->leave_collect && d->ws_leave_sig.p) ? d->ws_leave_sig.as<unsigned int>() : nullptr;
  const bool fuse_means = pre && nabla && nabla_means_fused(d, rows, 2 * H);   // NABLA: the norm pass takes the block means itself
  const int grp = pre ? attn_group_rows(d, nabla != nullptr, false) : 4;
  if (by_data) K5CHK(ensure_attn_flags(d, s));   // before the counters' address is taken
  const K5QueryNorm qn{a.norm.as<float>(), cosT, sinT, by_data ? d->ws_attn_cnt.as<unsigned long long>() : nullptr};
  {
    Scope sc(d, s, "elementwise");
    const int32_t hc[2] = {H, 2 * H};
    // NABLA: the block map needs the 64-token means of the UNSCALED keys (and queries).  Round 4 ("nabla_fuse_means", default): the norm pass
    // takes them itself, so the keys are scaled in place as on the dense path — no second read of q | k, no scaled copy.  Otherwise (rounds
    // 1-3) the unscaled keys stay in place for k5_launch_nabla_select_rect's own means pass and the scaled copy goes to its own buffer.
    void* kc = nullptr;
    void *mq = nullptr, *mk = nullptr;
    if (fuse_means) {
      K5CHK(d->ws_nabla.ensure(nabla_ws_bytes(d, H, rows / 64, rows / 64)));
      k5_nabla_workspace_means(d->ws_nabla.p, H, rows / 64, &mq, &mk);
    } else if (pre && nabla) { K5CHK(d->ws_kc.ensure((size_t)rows * D * 2)); kc = d->ws_kc.p; }
    float* stats = nullptr;
    if (by_data) stats = d->ws_attn_stats.as<float>();   // [q heads | k' heads] = the call's 2H heads (| squared key radii with the centred offsets)
    // centred per-row offsets (K5KeyCentre): the keys' sample-mean centre and their radius around it come out of the same pass
    float* centre = (by_data && d->row_offsets) ? d->ws_attn_flags.as<float>() + 3 * H : nullptr;
    if (fuse_q)   // keys only; the query statistic stays 0 (the fixed-offset workgroups take the head-level decision, K5QueryNorm)
      K5CHK(k5_launch_rmsnorm_rope((bf16_t*)qk + D, a.norm.as<float>() + 64, cosT, sinT, rows, H, 2 * D, nullptr, s, K5_SOFTMAX_C, 0, nullptr, 0,
                                   stats ? stats + H : nullptr, d->ws_attn_part.as<float>(), centre));
    else
      K5CHK(k5_launch_rmsnorm_rope(qk, a.norm.as<float>(), cosT, sinT, rows, 2 * H, 2 * D, hc, s, K5_SOFTMAX_C, pre ? H : 0x7fffffff, kc, D, stats, d->ws_attn_part.as<float>(),
                                   pre ? centre : nullptr, mq, rows / 64, mk, rows / 64));
    if (by_data) {   // the only schedule with centred offsets and the leave signal; the anchor launch is booked under this scope
      SoftmaxFormIn in;
      in.qstat = stats; in.kstat = stats + H; in.nk = 1; in.kstride = H; in.heads = H;
      in.centre = centre; in.rstat = stats + 2 * H; in.leave_sig = leave_sig;
      in.anchor = d->anchor && !fuse_q && !nabla;
      in.aq = qk; in.ak = (const bf16_t*)qk + D; in.aq_rows = rows; in.ak_rows = rows; in.ldq = 2 * D; in.ldk = 2 * D; in.key0 = 0; in.kv_total = rows;
      K5CHK(softmax_form(d, s, a, pref_slot, true, in, sf));
    }
  }
  float* const enh_score = enhance ? d->enh.scores.as<float>() + d->enh.block : nullptr;
  if (enhance) {   // the block's cross-frame score, on the keys the attention launch below reads: pre-scaled (in place, or NABLA's copy when
                   // the unscaled ones stay for its own means pass) with qk_scale 1, plain ones (rows % 64) with the softmax constant
    Scope sc(d, s, "enhance");
    const bool kin = !pre || !nabla || fuse_means;
    K5CHK(k5_launch_enhance_scores(qk, kin ? (const bf16_t*)qk + D : d->ws_kc.as<bf16_t>(), 2 * D, kin ? 2 * D : D, H, d->enh.T, d->enh.S,
                                   d->enh.rows, pre ? 1.0f : K5_SOFTMAX_C, d->enh.weight, d->enh.part.as<double>(), enh_score, s));
    ++d->enh.launches;
  }
  const int variant = pre ? d->attn_mode : K5_ATTN_AUTO;
  if (nabla) {  // nablaT_v2 map (utils.py:136-163) + block-sparse attention (nn.py:257-280)
    const int nb = rows / 64;
    const int pair = (grp == 2 && d->nabla_pair_frames) ? nabla->Hb * nabla->Wb : 0;
    K5CHK(d->ws_nabla.ensure(nabla_ws_bytes(d, H, nb, nb)));
    {
      Scope sc(d, s, "nabla_map");
      // fuse_means: the means are in the workspace already
      K5CHK(k5_launch_nabla_select_rect(fuse_means ? nullptr : qk, fuse_means ? nullptr : (const bf16_t*)qk + D, 2 * D, 2 * D, H, rows, 0, rows, nabla->T, nabla->Hb, nabla->Wb, nabla->wT,
                                        nabla->wH, nabla->wW, nabla->P, d->ws_nabla.p, s, 0, 0, grp, pair));
    }
    if (d->nabla_tap) {   // diagnostics (k5_dit_set_nabla_tap): this launch's map, expanded, behind the ones already taken
      const long long sz = (long long)H * nb * nb;
      if ((d->nabla_tap_n + 1) * sz <= d->nabla_tap_cap)
        K5CHK(k5_launch_nabla_mask_u8(d->ws_nabla.p, H, nb, nb, (char*)d->nabla_tap + d->nabla_tap_n * sz, s));
      ++d->nabla_tap_n;
    }
    if (d->profiling) {   // realised density of the map (bench.py: attention FLOPs actually done) and tiles the launch executes for it
      K5CHK(ensure_zeroed(d->ws_attn_cnt, 32, s));
      K5CHK(k5_launch_nabla_count(d->ws_nabla.p, H, nb, nb, d->ws_attn_cnt.as<unsigned long long>() + 2, s));
      K5CHK(k5_launch_nabla_count_lists(d->ws_nabla.p, H, nb, nb, grp, d->ws_attn_cnt.as<unsigned long long>() + 3, s));
      d->nabla_possible += (long long)H * nb * nb;
      d->nabla_list_rows = grp;
    }
    K5CHK(nabla_density_hint(d, H, nb, nb, s));
    const int *list, *cnt;
    k5_nabla_workspace_views(d->ws_nabla.p, H, nb, nullptr, nullptr, &list, &cnt);
    K5CHK(d->ws_attn_bal.ensure(k5_attention_balance_bytes(H, rows)));   // here only for the per-job fallback flags of the per-row offsets
    Scope sc(d, s, fam_attn);
    // (no tail balancing here: 10 248 jobs are 20 rounds of unequal lists — measured -0.6 % at density 0.81, +1 % at 0.12, +2.4 % at
    // 0.05; a token shard's 5 rounds are another matter, run_self_attention_sp)
    const bool kin = !pre || fuse_means;   // keys in place in the fused q | k buffer (scaled there when pre)
    K5AttnSparseArgs at;
    at.Q = qk; at.K = kin ? (const bf16_t*)qk + D : d->ws_kc.as<bf16_t>(); at.Vt = vt; at.O = o;
    at.H = H; at.q_len = rows; at.kv_len = rows; at.ldq = 2 * D; at.ldk = kin ? 2 * D : D; at.ldvt = ldvt; at.ldo = D;
    at.score_bound = pre ? 0.f : a.score_bound; at.stream = s;
    at.k_prescaled = pre; at.head_flags = sf.hflags; at.variant = variant; at.row_offset_kmax = sf.kmax; at.key_centre = sf.key_centre();
    at.list = list; at.cnt = cnt; at.list_stride = nb;
    at.balance_ws = pre ? d->ws_attn_bal.as<float>() : nullptr; at.balance = false;
    at.group_rows = grp; at.pair_stride = pair;
    K5CHK(k5_launch_attention_bf16_sparse(at));
  } else {
    K5CHK(d->ws_attn_bal.ensure(k5_attention_balance_bytes(H, rows)));
    Scope sc(d, s, fam_attn);
    K5AttnRangeArgs at;
    at.Q = qk; at.K = (const bf16_t*)qk + D; at.Vt = vt; at.O = o;
    at.H = H; at.q_len = rows; at.kv_len = rows; at.ldq = 2 * D; at.ldk = 2 * D; at.ldvt = ldvt; at.ldo = D;
    at.score_bound = pre ? 0.f : a.score_bound; at.stream = s; at.balance_ws = d->ws_attn_bal.as<float>();
    at.k_prescaled = pre; at.head_flags = sf.hflags; at.variant = variant; at.row_offset_kmax = sf.kmax; at.key_centre = sf.key_centre();
    at.query_norm = fuse_q ? &qn : nullptr;
    K5CHK(k5_launch_attention_bf16_range(at));
  }
  K5CHK(attn_pref_update(d, s, sf, H, rows, grp, leave_sig));
  if (enhance) {
    Scope sc(d, s, "enhance");
    K5CHK(k5_launch_scale_by_dev(o, rows, D, D, enh_score, s));
  }
  return attn_out_projection(d, s, a, o, rows, resid, gate, f8_out);
}

// Sequence-parallel visual self-attention: `rows` = this rank's token rows, N = rows * world keys in total.
// q / k / v^T are projected for the local rows only; k and v^T land directly in this rank's slot of the
// gather buffers, one in-place all-gather each makes every rank hold all keys, then attention runs for the
// local query rows.  No head-count constraint (28 heads do not divide by 8), no activation all-reduce.
// Uneven shards: every rank's slot in the gather buffers holds rows_pad = ceil(blocks / P) * 64 rows; only the LAST rank may
// own fewer (rows < rows_pad), so the padded row index of every real key equals its global index and the unused tail of the
// last slot is never read (the key-tile ranges stop at N).
int run_self_attention_sp(k5_dit* d, hipStream_t s, const AttnW& a, const void* h, int rows, int rows_pad, int N, void* o,
                          const float* cosT, const float* sinT, void* resid, const float* gate, const NablaArgs* nabla = nullptr, int pref_slot = 0,
                          bool h8_ready = false) {
  const int D = d->D, H = d->Hh, P = d->sp_world, r = d->sp_rank;
  const int ldv = rows_pad;  // rows, rows_pad, N are multiples of 64 (checked by the caller)
  bf16_t* q = d->ws_q.as<bf16_t>();
  bf16_t* kfull = d->ws_kfull.as<bf16_t>();
  bf16_t* vtfull = d->ws_vtfull.as<bf16_t>();
  bf16_t* kloc = kfull + (size_t)r * rows_pad * D;
  bf16_t* vtloc = vtfull + (size_t)r * D * ldv;
  const Linear wq = a.wqk.rows(0, D), wk = a.wqk.rows(D, D);
  // pre-scaled keys, softmax form per head from the data (the |k'|^2 maxima of all ranks are gathered with the keys) — dense AND
  // NABLA.  The NABLA map is computed from the UNSCALED keys, of which it only needs the 64-token block means: the unscaled
  // keys stay local (ws_kc), their means (28 x 64 values per block) travel with the gather, and the gathered keys are the scaled ones —
  // the same kernels, flags and per-row offsets as on one GPU (round 1 / early round 2: unscaled keys, weight-derived bound, and
  // with it the online-max 32x32 kernel for any checkpoint whose QK-norm gains exceed max|w_q| max|w_k| = 3.96).
  const bool fuse_means = nabla && nabla_means_fused(d, rows, H);   // NABLA: the norm passes take the block means themselves
  const bool by_data = d->attn_mode == K5_ATTN_AUTO;
  float *qstat = nullptr, *kstat = nullptr;
  if (by_data) { K5CHK(ensure_attn_flags(d, s)); qstat = d->ws_attn_stats.as<float>(); kstat = qstat + H; }
  const int slot_blocks = rows_pad / 64;
  bf16_t* kun = kloc;                       // where the projection + norm + RoPE of the local keys happen
  bf16_t* kmeans = nullptr;                 // NABLA: [P][H][slot_blocks][64] key-block means, this rank's slot filled here
  if (nabla) {
    K5CHK(d->ws_kc.ensure((size_t)rows * D * 2));
    K5CHK(d->ws_kmeans.ensure((size_t)P * H * slot_blocks * 64 * 2));
    kun = d->ws_kc.as<bf16_t>();
    kmeans = d->ws_kmeans.as<bf16_t>();
  }
  // opt-in e4m3 projections (k5_dit_set_fp8 bit 1), as on one GPU: the rank's rows of h are quantised once and feed the K, V^T and Q GEMMs
  const bool f8_in = sa_sp_fp8_in(d, a, rows, rows_pad, nabla != nullptr);
  Act x;
  K5CHK(e4m3_rows(d, s, h, rows, f8_in, h8_ready, x));
  {
    Scope sc(d, s, "gemm");
    K5CHK(linear(LinearArgs(wk, x, kun, D, s)));
  }
  {
    Scope sc(d, s, "elementwise");
    // dense: scaled in place; NABLA: unscaled in place (kun), the scaled copy goes to this rank's slot of the gather buffer
    // NABLA: the unscaled keys' block means (all the map needs of them) come out of this pass ("nabla_fuse_means"; before: a second pass over kun)
    K5CHK(k5_launch_rmsnorm_rope(kun, a.norm.as<float>() + 64, cosT, sinT, rows, H, D, nullptr, s, K5_SOFTMAX_C, 0,
                                 nabla ? kloc : nullptr, nabla ? D : 0, by_data ? kstat + (size_t)r * H : nullptr, d->ws_attn_part.as<float>(), nullptr,
                                 nullptr, 0, fuse_means ? kmeans + (size_t)r * H * slot_blocks * 64 : nullptr, slot_blocks));
  }
  if (nabla && !fuse_means) {
    Scope sc(d, s, "nabla_map");
    K5CHK(k5_launch_nabla_block_means(kun, D, H, rows / 64, slot_blocks, kmeans + (size_t)r * H * slot_blocks * 64, s));
  }
  HIPCHK(hipEventRecord(d->ev_k, s));
  // sliced exchange (dense attention, "sp_slices" = S > 1): the slot of every rank is S slices of rows_pad / S tokens; V^T is laid
  // out slice-major inside the slot — [S][D][rows_pad / S] — so that a slice is contiguous on both operands (for the attention kernel
  // these are simply P S chunks of rows_pad / S keys) and is projected by one GEMM per slice
  const int S = (!nabla && d->sp_slices > 1 && P > 1) ? d->sp_slices : 1;
  const int cols = rows_pad / S;   // tokens per slice (the caller sized rows_pad as a multiple of 64 S)
  {
    Scope sc(d, s, "gemm");
    for (int sl = 0; sl < S; ++sl) {
      const int nsl = std::min(cols, rows - sl * cols);
      if (nsl <= 0) break;
      LinearArgs gv(a.wv, x.from((size_t)sl * cols, nsl), vtloc + (size_t)sl * D * cols, cols, s);
      gv.weights_as_rows = true;
      K5CHK(linear(gv));
    }
  }
  HIPCHK(hipEventRecord(d->ev_v, s));
  {
    Scope sc(d, s, "gemm");
    K5CHK(linear(LinearArgs(wq, x, q, D, s)));
  }
  // see run_self_attention; here only with "attn_fuse_qnorm" = 2: every pass of the schedule redoes the norm, and at shard sizes that
  // costs what the standalone pass over the local queries does (emulated P = 8: 82.8 vs 82.6 ms per step)
  const bool fuse_q = !nabla && d->fuse_qnorm > 1 && ((by_data && d->row_offsets) || d->attn_mode == K5_ATTN_ONLINE);
  const K5QueryNorm qn{a.norm.as<float>(), cosT, sinT, by_data ? d->ws_attn_cnt.as<unsigned long long>() : nullptr};
  const K5QueryNorm* qnp = fuse_q ? &qn : nullptr;
  if (!fuse_q) {
    void* mq = nullptr;
    if (fuse_means) {   // the query-block means of the rank's rows, straight into the map's workspace
      K5CHK(d->ws_nabla.ensure(nabla_ws_bytes(d, H, N / 64, rows / 64)));
      k5_nabla_workspace_means(d->ws_nabla.p, H, N / 64, &mq, nullptr);
    }
    Scope sc(d, s, "elementwise");
    K5CHK(k5_launch_rmsnorm_rope(q, a.norm.as<float>(), cosT, sinT, rows, H, D, nullptr, s, 1.f, 0x7fffffff, nullptr, 0, qstat, d->ws_attn_part.as<float>(), nullptr,
                                 mq, rows / 64, nullptr, 0));
  }
  // all-gathers on the side stream (they only need k / v^T, which are complete at ev_k / ev_v) ...
  hipStream_t cs = d->comm_stream;
  HIPCHK(hipStreamWaitEvent(cs, d->ev_k, 0));
  {
    Scope sc(d, cs, "comm");
    if (by_data) {   // H floats per rank, first: the flags must exist before pass 1 (both passes take the same form per head)
      K5CHK(d->comm.all_gather_inplace(kstat, (size_t)H, 4, cs));
      HIPCHK(hipEventRecord(d->ev_stats, cs));
    }
    if (nabla) {   // 28 x 64 values per block: lands long before the keys, and the map is computed while they travel
      K5CHK(d->comm.all_gather_inplace(kmeans, (size_t)H * slot_blocks * 64, 2, cs));
      HIPCHK(hipEventRecord(d->ev_means, cs));
    }
    if (S == 1) {
      K5CHK(d->comm.all_gather_inplace(kfull, (size_t)rows_pad * D, 2, cs));
      HIPCHK(hipStreamWaitEvent(cs, d->ev_v, 0));
      K5CHK(d->comm.all_gather_inplace(vtfull, (size_t)D * ldv, 2, cs));
    } else {
      const size_t slot = (size_t)rows_pad * D * 2, sl_bytes = (size_t)cols * D * 2;   // the same for K and for V^T
      for (int sl = 0; sl < S; ++sl) {
        K5CHK(d->comm.slot_exchange(kfull, slot, sl * sl_bytes, sl_bytes, cs));
        if (sl == 0) HIPCHK(hipStreamWaitEvent(cs, d->ev_v, 0));
        K5CHK(d->comm.slot_exchange(vtfull, slot, sl * sl_bytes, sl_bytes, cs));
        HIPCHK(hipEventRecord(d->ev_slice[sl], cs));
      }
    }
  }
  HIPCHK(hipEventRecord(d->ev_gathered, cs));
  // per-row softmax offsets (§4.1) across the passes: a row that underflows in ANY pass marks its head late (flag 2), the fixed
  // form then skips the head and the online form of the LAST pass recomputes it from scratch over all keys (late_pass 1 / 2)
  SoftmaxForm sf;
  {
    // plain offsets; heads beyond their window: anchored offsets, sampled from the rank's OWN keys (the row's own block is among them;
    // they are in place before the gather) — every pass of the schedule then runs the head on them
    SoftmaxFormIn in;
    in.qstat = qstat; in.kstat = kstat; in.nk = P; in.kstride = H; in.heads = H; in.stats_ready = d->ev_stats;
    in.anchor = d->anchor && !fuse_q && !nabla;
    in.aq = q; in.ak = kloc; in.aq_rows = rows; in.ak_rows = rows; in.ldq = D; in.ldk = D; in.key0 = 0; in.kv_total = N;
    K5CHK(softmax_form(d, s, a, pref_slot, by_data, in, sf));
  }
  const int grp = attn_group_rows(d, nabla != nullptr, true);
  // what every attention launch of the schedule shares: the rank's queries against the gathered K' / V^T (chunked per rank)
  K5AttnArgs common;
  common.Q = q; common.K = kfull; common.Vt = vtfull; common.O = o;
  common.H = H; common.q_len = rows; common.kv_len = N; common.ldq = D; common.ldk = D; common.ldvt = ldv; common.ldo = D;
  common.vt_chunk_keys = rows_pad; common.vt_chunk_stride = (long long)D * ldv;
  common.stream = s;   // balance_ws: set per branch once ws_attn_bal is sized
  common.k_prescaled = true; common.head_flags = sf.hflags; common.variant = d->attn_mode; common.row_offset_kmax = sf.kmax; common.key_centre = sf.key_centre();
  const float* kmax = sf.kmax;
  if (nabla) {
    // NABLA under sequence parallelism: the map rows of this rank's query blocks need the block means of
    // ALL keys -> wait for the gathered means, bring them into the map's layout, select (local query blocks x all key blocks)
    // while K' / V^T are still on their way; then the list-driven attention on the chunked V^T layout (single pass).
    HIPCHK(hipStreamWaitEvent(s, d->ev_means, 0));
    const int nb = N / 64;
    // sparse maps: 128-query workgroups (lists per two rows, see nabla_group_rows; attn_group_rows); dense maps: the 256-query form, balanced
    const int pair = (grp == 2 && d->nabla_pair_frames) ? nabla->Hb * nabla->Wb : 0;   // rows l and l + S of the rank's shard: same tile, next frame
    K5CHK(d->ws_nabla.ensure(nabla_ws_bytes(d, H, nb, rows / 64)));   // the logits and list regions by the rank's own query-block rows
    {
      Scope sc(d, s, "nabla_map");
      K5CHK(k5_launch_nabla_key_means_from_slots(kmeans, H, nb, slot_blocks, d->ws_nabla.p, s));
      K5CHK(k5_launch_nabla_select_rect(fuse_means ? nullptr : q, nullptr, D, 0, H, rows, r * slot_blocks, N, nabla->T, nabla->Hb, nabla->Wb, nabla->wT,
                                        nabla->wH, nabla->wW, nabla->P, d->ws_nabla.p, s, r * slot_blocks, rows / 64, grp, pair));   // own key blocks lead the lists
    }
    if (d->profiling) {
      K5CHK(ensure_zeroed(d->ws_attn_cnt, 32, s));
      K5CHK(k5_launch_nabla_count(d->ws_nabla.p, H, rows / 64, nb, d->ws_attn_cnt.as<unsigned long long>() + 2, s));
      d->nabla_possible += (long long)H * (rows / 64) * nb;
    }
    const int *list, *cnt, *cnt_local;
    k5_nabla_workspace_views(d->ws_nabla.p, H, nb, nullptr, nullptr, &list, &cnt, &cnt_local, rows / 64);
    K5CHK(d->ws_attn_bal.ensure(k5_attention_balance_bytes(H, rows)));
    K5CHK(nabla_density_hint(d, H, rows / 64, nb, s));
    K5AttnSparseArgs at;
    static_cast<K5AttnArgs&>(at) = common;
    at.balance_ws = d->ws_attn_bal.as<float>();
    at.list = list; at.cnt = cnt; at.list_stride = nb; at.group_rows = grp;
    if (grp < 4) {
      HIPCHK(hipStreamWaitEvent(s, d->ev_gathered, 0));
      Scope sc(d, s, "attn_self");
      at.pair_stride = pair;
      K5CHK(k5_launch_attention_bf16_sparse(at));
    } else if (d->sp_nabla_passes > 1 && P > 1) {
      // two passes over every list: the rank's own key blocks (they lead the lists; K' / V^T of them are in place) while the other
      // ranks' keys travel — state out —, then the rest once the gather has landed (resume, normalise); late fallback as in the dense
      // schedule (a head whose row underflows on its per-row offset in pass 1 is recomputed from scratch by the online form of pass 2)
      K5CHK(d->ws_attn_state.ensure(k5_attention_state_bytes(H, rows)));
      {
        const K5SparsePass p1{nullptr, d->ws_attn_state.as<float>(), 2, kmax ? 1 : 0};
        Scope sc(d, s, "attn_self");
        at.cnt = cnt_local; at.pass = &p1;
        K5CHK(k5_launch_attention_bf16_sparse(at));
      }
      HIPCHK(hipStreamWaitEvent(s, d->ev_gathered, 0));
      const K5SparsePass p2{cnt_local, d->ws_attn_state.as<float>(), 1, kmax ? 2 : 0};
      Scope sc(d, s, "attn_self");
      at.cnt = cnt; at.pass = &p2;
      K5CHK(k5_launch_attention_bf16_sparse(at));
    } else {
      HIPCHK(hipStreamWaitEvent(s, d->ev_gathered, 0));
      Scope sc(d, s, "attn_self");
      K5CHK(k5_launch_attention_bf16_sparse(at));
    }
  } else {
    // ... while the main stream attends the local query rows to the LOCAL key chunk (pass 1, leaves the fp32 state),
    // then, once every chunk has arrived, to all the other chunks (pass 2, resumes the state and normalises).
    const int tpc = rows / 64, tpc_pad = rows_pad / 64, total = N / 64;
    // Pass 1 exists to cover the gather (its tail jobs are split and merged back into the state like those of the final pass),
    // so it should be no longer than the gather.  How long the gather takes is a property of the node (one
    // xGMI link per GPU pair: ~341 MB / (P x link rate) per block, i.e. about 0.4 of a rank's attention time at any P if a link
    // gives ~70 GB/s each way, much less if RCCL drives several paths) and cannot be measured here, so the default is the
    // safe one — all local key tiles — and k5_dit_set_option("sp_pass1_tiles") sets it on a real node (emulated, P = 2: 41
    // tiles instead of 372 take the step from 282 to 259 ms).
    int k1 = (d->sp_pass1_tiles > 0 && S == 1) ? d->sp_pass1_tiles : tpc;   // the sliced schedule attends all local tiles first
    k1 = k1 > tpc ? tpc : k1;
    K5CHK(d->ws_attn_state.ensure(k5_attention_state_bytes(H, rows)));
    K5CHK(d->ws_attn_bal.ensure(k5_attention_balance_bytes(H, rows)));
    K5AttnRangeArgs at;
    static_cast<K5AttnArgs&>(at) = common;
    at.balance_ws = d->ws_attn_bal.as<float>();
    at.state = d->ws_attn_state.as<float>(); at.query_norm = qnp;
    if (S > 1) { at.ldvt = cols; at.vt_chunk_keys = cols; at.vt_chunk_stride = (long long)D * cols; }   // P S chunks of rows_pad / S keys
    {
      Scope sc(d, s, "attn_self");
      at.tile_off0 = r * tpc_pad; at.tile_cnt = k1; at.flags = 2; at.late_pass = kmax ? 1 : 0;
      K5CHK(k5_launch_attention_bf16_range(at));
    }
    if (S == 1) {
      HIPCHK(hipStreamWaitEvent(s, d->ev_gathered, 0));
      Scope sc(d, s, "attn_self");
      at.tile_off0 = 0; at.tile_cnt = total - k1; at.tile_skip_at = r * tpc_pad; at.tile_skip_n = k1; at.flags = 1; at.late_pass = kmax ? 2 : 0;
      K5CHK(k5_launch_attention_bf16_range(at));
    } else {
      // one pass per slice, as soon as that slice of every peer has landed: slice sl of rank p = key tiles [p tpc_pad + sl tps, + tps)
      // (P - 1 segments: mine was pass 1; the last rank's slot may end early — it is the last segment, so the count is cut short).
      // The state is resumed and saved between the passes (tail jobs balanced in every pass); the last one normalises.
      const int tps = tpc_pad / S;
      const int last_rank_tiles = total - (P - 1) * tpc_pad;                 // > 0 (checked by the caller)
      int cnts[4] = {0, 0, 0, 0}, last_pass = 0;
      for (int sl = 0; sl < S; ++sl) {
        cnts[sl] = (P - 1) * tps;
        if (r != P - 1) cnts[sl] -= tps - std::max(0, std::min(tps, last_rank_tiles - sl * tps));
        if (cnts[sl] > 0) last_pass = sl;                                     // slice 0 always has tiles
      }
      const K5TileSegments seg{tps, tpc_pad, r};
      at.segments = &seg;
      for (int sl = 0; sl < S; ++sl) {
        const int cnt = cnts[sl];
        HIPCHK(hipStreamWaitEvent(s, d->ev_slice[sl], 0));
        if (cnt <= 0) continue;
        const bool fin = sl == last_pass;
        Scope sc(d, s, "attn_self");
        at.tile_off0 = sl * tps; at.tile_cnt = cnt; at.flags = fin ? 1 : 3; at.late_pass = kmax ? (fin ? 2 : 1) : 0;
        K5CHK(k5_launch_attention_bf16_range(at));
      }
    }
  }
  K5CHK(attn_pref_update(d, s, sf, H, rows, grp));
  return attn_out_projection(d, s, a, o, rows, resid, gate);
}

// Ulysses-style sequence parallelism (north_star; "sp_mode" = 1): instead of gathering every rank's K / V^T, the ranks trade token rows for
// HEADS — an all-to-all turns (rows of this rank x all 28 heads) into (all N rows x the 28 / P heads of this rank) for q | k and V^T, the
// rank runs the ONE-GPU attention (a single balanced pass over all keys: no fp32 state between passes) for its heads, and a second
// all-to-all brings the outputs back to the token shards.  Per rank and block 4 x (P - 1) / P^2 x N x D x 2 B leave the GPU (3/16 of
// the 170 MB of a 5 s clip per tensor at P = 4) against 2 x (P - 1) / P x N x D x 2 B of ingress for the gather: a ratio of 2 / P —
// the same bytes at P = 2, half at P = 4, 2/7 at P = 7 — but the attention cannot start before q, k AND V^T have landed, where the gather hides behind pass 1.
// Needs heads % P == 0 (28 = 2 x 2 x 7: P in 2, 4, 7, 14) and dense attention; anything else keeps the gather.  Replaces the head split
// of the reference's tensor-parallel plan (parallelize.py:87-91) together with its all-reduces.
// Layouts: send [P][rows_pad][2 Dp] (block g: q | k' of the heads of rank g, this rank's rows) -> recv [P][rows_pad][2 Dp] = all rows
// (rank-major = token order: slots are contiguous token ranges) of this rank's heads; V^T [D][rows_pad] is destination-major as the GEMM
// writes it (block g = rows g Dp ..) -> vrecv [P][Dp][rows_pad] = the chunked V^T layout of the attention kernel; o [P rows_pad][Dp]
// -> orecv [P][rows_pad][Dp] (block g: the outputs of rank g's heads for this rank's rows) -> unpacked to [rows][D].
// Two-level sequence parallelism ("sp_mode" = 2): Ulysses needs heads % P == 0, which 28 heads at P = 8 (or 6) miss.  With G = gcd(heads, P)
// head groups and S = P / G query splits, rank r attends head group g = r % G for the queries of split s = r / G (the G consecutive token
// shards of ranks sG .. sG + G - 1) against all N keys in ONE pass — the one-GPU attention, no fp32 state between passes, as in Ulysses:
//   1. q | k projection and norm + RoPE of the rank's rows as in Ulysses (|q|^2 / |k'|^2 maxima gathered over the world: the S ranks of a head
//      group take the same softmax form, decided from all N rows); one pass packs q and k' into per-head-group send planes (sp2d_pack_qk)
//   2. k' and V^T by one exchange over the whole world, fan-out: every peer gets the block of ITS head group (no copy per destination);
//      received in token order, [P][rows_pad][Dp] / [P][Dp][rows_pad] — the chunked layout the Ulysses attention launch reads
//   3. q by an exchange inside the split: [G][rows_pad][Dp] = the split's rows of my heads
//   4. attention: Hp heads, the split's rows x all N keys (anchored offsets sampled around each row's own block, as in Ulysses)
//   5. o back inside the split, unpacked as in Ulysses with G head groups, gated out-projection.
// Per rank and block (P = 8, G = 4, config 2) 107 MB arrive instead of the gather's 299 MB.  Callers: G = 1 -> gather,
// G = P -> Ulysses (sp_schedule).
// Both are run_self_attention_heads: the same projections, norm + RoPE, softmax-form step, one balanced attention launch, unpack and
// out-projection; what differs is the layout below, the pack kernel and the collectives — Ulysses keeps its own wire pattern (one interleaved
// q | k' all-to-all of rows_pad x 2 Dp blocks, then V^T, then o back), the two-level schedule its planned exchanges (stats, k', q, V^T, o).
struct HeadsLayout {
  int G;                        // head groups (Ulysses: P); also the group count of the unpack
  int Hp, Dp, hg;               // heads / columns per group, and the group this rank attends
  int q0, Ms;                   // the query rows this rank attends: [q0, q0 + Ms) of the N tokens
  const bf16_t* q; const bf16_t* k; int ldq, ldk;   // where they and all N keys of the group land
};
int run_self_attention_heads(k5_dit* d, hipStream_t s, const AttnW& a, const void* h, int rows, int rows_pad, int N, void* o,
                             const float* cosT, const float* sinT, void* resid, const float* gate, bool two_level, int pref_slot = 0) {
  const int D = d->D, H = d->Hh, P = d->sp_world, r = d->sp_rank;
  HeadsLayout L;
  L.G = two_level ? sp_gcd(H, P) : P;
  L.Hp = H / L.G; L.Dp = D / L.G; L.hg = r % L.G;
  const int G = L.G, Hp = L.Hp, Dp = L.Dp;
  L.q0 = two_level ? (r / G) * G * rows_pad : 0;   // the split's token rows
  L.Ms = std::min(N, L.q0 + G * rows_pad) - L.q0;
  const size_t blk = (size_t)rows_pad * Dp * 2;   // bytes of one rows_pad x Dp block
  if (two_level) {
    if (L.Ms <= 0) { k5_set_error("internal: two-level split without rows"); return K5_ERR_STATE; }
    if (d->sp_plan_key[0] != P || d->sp_plan_key[1] != rows_pad) {
      for (int w = SP_K; w <= SP_O; ++w) { d->sp_plan[w].resize((size_t)P * P); sp_plan_2d(H, P, rows_pad, D, w, d->sp_plan[w].data()); }
      d->sp_plan_key[0] = P; d->sp_plan_key[1] = rows_pad;
    }
  }
  const bool by_data = d->attn_mode == K5_ATTN_AUTO;
  K5CHK(d->ws_qk.ensure((size_t)rows * 2 * D * 2));
  K5CHK(d->ws_u_send.ensure(2 * G * blk));       // Ulysses: [P][rows_pad][2 Dp]; two-level: q plane [G][rows_pad][Dp] | k' plane [G][rows_pad][Dp]
  K5CHK(d->ws_u_recv.ensure((two_level ? 1 : 2) * P * blk));   // Ulysses: q | k' of all N rows, my heads; two-level: k' only
  K5CHK(d->ws_u_vsend.ensure((size_t)D * rows_pad * 2)); K5CHK(d->ws_u_vrecv.ensure(P * blk));
  if (two_level) K5CHK(d->ws_u_qrecv.ensure(G * blk));
  K5CHK(d->ws_u_o.ensure(G * blk)); K5CHK(d->ws_u_orecv.ensure(G * blk));
  K5CHK(ensure_zeroed(d->ws_u_stats, (size_t)P * 2 * H * 4, s));
  if (!d->ev_u_o) { HIPCHK(hipEventCreateWithFlags(&d->ev_u_o, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&d->ev_u_back, hipEventDisableTiming)); }
  if (by_data) K5CHK(ensure_attn_flags(d, s));
  float* ustats = d->ws_u_stats.as<float>();         // [P][2 H]: rank p's maxima of |q_h|^2 (H) and |k'_h|^2 (H) over ITS rows
  if (by_data) HIPCHK(hipMemsetAsync(ustats + (size_t)r * 2 * H, 0, (size_t)2 * H * 4, s));   // the norm pass max-accumulates; only my heads' entries were consumed
  bf16_t* qk = d->ws_qk.as<bf16_t>();
  const Act x{h, nullptr, rows, D};   // these schedules keep q | k | V^T in bf16 whatever k5_dit_set_fp8 asked for ("fp8_effective" says so)
  bf16_t* qsend = d->ws_u_send.as<bf16_t>();
  bf16_t* ksend = qsend + (size_t)G * rows_pad * Dp;   // two-level
  if (two_level) { L.q = d->ws_u_qrecv.as<bf16_t>(); L.k = d->ws_u_recv.as<bf16_t>(); L.ldq = L.ldk = Dp; }
  else { L.q = d->ws_u_recv.as<bf16_t>(); L.k = L.q + Dp; L.ldq = L.ldk = 2 * Dp; }
  {
    Scope sc(d, s, "gemm");
    K5CHK(linear(LinearArgs(a.wqk, x, qk, 2 * D, s)));
  }
  {
    Scope sc(d, s, "elementwise");
    const int32_t hc[2] = {H, 2 * H};
    K5CHK(k5_launch_rmsnorm_rope(qk, a.norm.as<float>(), cosT, sinT, rows, 2 * H, 2 * D, hc, s, K5_SOFTMAX_C, H, nullptr, 0,
                                 by_data ? ustats + (size_t)r * 2 * H : nullptr, d->ws_attn_part.as<float>()));
    if (two_level) K5CHK(k5_launch_sp2d_pack_qk(qk, qsend, ksend, rows, rows_pad, D, G, s));
    else K5CHK(k5_launch_ulysses_pack_qk(qk, d->ws_u_send.p, rows, rows_pad, D, P, s));
  }
  HIPCHK(hipEventRecord(d->ev_k, s));
  hipStream_t cs = d->comm_stream;
  HIPCHK(hipStreamWaitEvent(cs, d->ev_k, 0));
  {
    Scope sc(d, cs, "comm");   // the same collectives in the same order on every rank
    if (by_data) { K5CHK(d->comm.all_gather_inplace(ustats, (size_t)2 * H, 4, cs)); HIPCHK(hipEventRecord(d->ev_stats, cs)); }
    if (two_level) {
      K5CHK(d->comm.exchange(ksend, d->ws_u_recv.p, d->sp_plan[SP_K].data(), cs));
      K5CHK(d->comm.exchange(qsend, d->ws_u_qrecv.p, d->sp_plan[SP_Q].data(), cs));
    } else K5CHK(d->comm.all_to_all(d->ws_u_send.p, d->ws_u_recv.p, 2 * blk, cs));
  }
  {
    Scope sc(d, s, "gemm");   // V^T of the rank's rows while q | k' travel
    LinearArgs gv(a.wv, x, d->ws_u_vsend.p, rows_pad, s);
    gv.weights_as_rows = true;
    K5CHK(linear(gv));
  }
  HIPCHK(hipEventRecord(d->ev_v, s));
  HIPCHK(hipStreamWaitEvent(cs, d->ev_v, 0));
  {
    Scope sc(d, cs, "comm");
    if (two_level) K5CHK(d->comm.exchange(d->ws_u_vsend.p, d->ws_u_vrecv.p, d->sp_plan[SP_VT].data(), cs));
    else K5CHK(d->comm.all_to_all(d->ws_u_vsend.p, d->ws_u_vrecv.p, blk, cs));
  }
  HIPCHK(hipEventRecord(d->ev_gathered, cs));
  K5CHK(d->ws_attn_bal.ensure(k5_attention_balance_bytes(Hp, L.Ms)));
  SoftmaxForm sf;
  {
    // flags of MY head group from every rank's maxima (each rank held some rows of them; the ranks of a head group take the same form);
    // anchored offsets: this rank holds all keys of its heads, each query row's own 64-token block sits at key index q0 + row
    SoftmaxFormIn in;
    in.qstat = ustats + (size_t)L.hg * Hp; in.kstat = ustats + H + (size_t)L.hg * Hp; in.nk = P; in.kstride = 2 * H; in.nq = P; in.qstride = 2 * H;
    in.heads = Hp; in.head0 = L.hg * Hp; in.stats_ready = d->ev_stats; in.data_ready = d->ev_gathered;
    in.anchor = d->anchor != 0; in.anchor_fam = "elementwise";
    in.aq = L.q; in.ak = L.k; in.aq_rows = L.Ms; in.ak_rows = N; in.ldq = L.ldq; in.ldk = L.ldk; in.key0 = L.q0; in.kv_total = N;
    K5CHK(softmax_form(d, s, a, pref_slot, by_data, in, sf));
  }
  {
    Scope sc(d, s, "attn_self");
    K5AttnRangeArgs at;
    at.Q = L.q; at.K = L.k; at.Vt = d->ws_u_vrecv.p; at.O = d->ws_u_o.p;
    at.H = Hp; at.q_len = L.Ms; at.kv_len = N; at.ldq = L.ldq; at.ldk = L.ldk; at.ldvt = rows_pad; at.ldo = Dp;
    at.vt_chunk_keys = rows_pad; at.vt_chunk_stride = (long long)Dp * rows_pad;
    at.stream = s; at.balance_ws = d->ws_attn_bal.as<float>();
    at.k_prescaled = true; at.head_flags = sf.hflags; at.variant = d->attn_mode; at.row_offset_kmax = sf.kmax; at.key_centre = sf.key_centre();
    K5CHK(k5_launch_attention_bf16_range(at));
  }
  K5CHK(attn_pref_update(d, s, sf, Hp, L.Ms, 4));
  HIPCHK(hipEventRecord(d->ev_u_o, s));
  HIPCHK(hipStreamWaitEvent(cs, d->ev_u_o, 0));
  {
    Scope sc(d, cs, "comm");
    if (two_level) K5CHK(d->comm.exchange(d->ws_u_o.p, d->ws_u_orecv.p, d->sp_plan[SP_O].data(), cs));
    else K5CHK(d->comm.all_to_all(d->ws_u_o.p, d->ws_u_orecv.p, blk, cs));
  }
  HIPCHK(hipEventRecord(d->ev_u_back, cs));
  HIPCHK(hipStreamWaitEvent(s, d->ev_u_back, 0));
  {
    Scope sc(d, s, "elementwise");
    K5CHK(k5_launch_ulysses_unpack_o(d->ws_u_orecv.p, o, rows, rows_pad, D, G, s));
  }
  return attn_out_projection(d, s, a, o, rows, resid, gate);
}

// keys and V^T of every visual block's cross-attention from a text stream (k5_dit::cross_kv_batched): st.ck_all [L][blocks * D] (normalised
// keys), st.cvt_all [blocks * D][rup(L, 8)].  The key projection is the launch it was per block (128 x 128 tiles for 256 rows); the V^T one is forced
// onto the same 128 x 128 kernel the per-block call took (57 344 weight rows would otherwise pick a 256-row kernel: another summation order).
int cross_kv_batched_run(k5_dit* d, hipStream_t s, k5_dit::TextStream& st) {
  const int D = d->D, H = d->Hh, nbv = (int)d->vblocks.size(), L = st.L;
  const int ldvt = (int)rup(L, 8);
  K5CHK(st.ck_all.ensure((size_t)L * nbv * D * 2)); K5CHK(st.cvt_all.ensure((size_t)nbv * D * ldvt * 2));
  {
    Scope sc(d, s, "gemm");
    const Act text{st.text.p, nullptr, L, D};
    LinearArgs gk(d->cx_k, text, st.ck_all.p, nbv * D, s), gv(d->cx_v, text, st.cvt_all.p, ldvt, s);
    gk.force_kernel = gv.force_kernel = 2;
    gv.weights_as_rows = true;
    K5CHK(linear(gk));
    K5CHK(linear(gv));
  }
  Scope sc(d, s, "elementwise");
  const int32_t hc[2] = {H, 0};   // one norm weight per block's H heads, no RoPE
  return k5_launch_rmsnorm_rope(st.ck_all.p, d->cx_knorm_all.as<float>(), nullptr, nullptr, L, nbv * H, nbv * D, hc, s);
}

// One text stream as a visual block's cross-attention sees it: its rows, where the block's normalised keys (row stride ldck) and V^T (row
// stride ldvt) are or go, and the rows its attention output goes to
struct CrossView { const void* text; int L; void* ck; void* cvt; int ldck, ldvt; void* o; };
// the view of stream st for visual block i.  stacked: what cross_kv_batched_run left (this is the only reader of that layout); otherwise the
// stream's per-block buffers, which run_cross_attention fills
CrossView cross_view(const k5_dit* d, const k5_dit::TextStream& st, int i, bool stacked, void* o) {
  const int D = d->D, nbv = (int)d->vblocks.size(), ldvt = (int)rup(st.L, 8);
  if (!stacked) return CrossView{st.text.p, st.L, st.ck.p, st.cvt.p, D, ldvt, o};
  return CrossView{st.text.p, st.L, st.ck_all.as<bf16_t>() + (size_t)i * D, st.cvt_all.as<bf16_t>() + (size_t)i * D * ldvt, nbv * D, ldvt, o};
}
// The streams of one cross-attention, in launch order: v[0] the forward's own prompt (its o receives the result), then the negative prompt if
// nag, then (last) R regions, whose outputs lie region_o_stride elements apart and are weighed per token by region_w [rows][R + 1]
struct CrossStreams { CrossView v[1 + 1 + 8]; int n = 0; bool kv_ready = false, nag = false; int R = 0; long long region_o_stride = 0; const float* region_w = nullptr; };

// The same queries (h through wq, into q) against every stream of cx.  kv_ready: the views already hold this block's normalised keys and V^T
// (cross_kv_batched_run); otherwise they are projected and normalised here.  k5_launch_region_combine (in place on v[0].o) makes the positive
// side of the regions' outputs, k5_launch_nag_combine (likewise) joins it to the negative stream's, in front of the out projection.
int run_cross_attention(k5_dit* d, hipStream_t s, const AttnW& a, const void* h, int rows, void* q, const CrossStreams& cx, void* resid, const float* gate) {
  const int D = d->D, H = d->Hh;
  void* o = cx.v[0].o;
  {
    Scope sc(d, s, "gemm");
    K5CHK(linear(LinearArgs(a.wq, Act{h, nullptr, rows, D}, q, D, s)));
    for (int k = 0; !cx.kv_ready && k < cx.n; ++k) {
      const CrossView& v = cx.v[k];
      const Act text{v.text, nullptr, v.L, D};
      LinearArgs gv(a.wv, text, v.cvt, v.ldvt, s);
      gv.weights_as_rows = true;
      K5CHK(linear(LinearArgs(a.wk, text, v.ck, v.ldck, s)));
      K5CHK(linear(gv));
    }
  }
  // RMSNorm of the queries (no RoPE in cross-attention, nn.py:330-334) is fused into the attention kernel's Q-fragment load when the
  // weight-derived bound admits the fixed-offset kernel: one pass over the (rows, D) projection less per block
  const bool fuse_qnorm = a.score_bound > 0.f && a.score_bound * K5_SOFTMAX_C <= 90.f;
  {
    Scope sc(d, s, "elementwise");
    if (!fuse_qnorm) K5CHK(k5_launch_rmsnorm_rope(q, a.norm.as<float>(), nullptr, nullptr, rows, H, D, nullptr, s));
    for (int k = 0; !cx.kv_ready && k < cx.n; ++k)
      K5CHK(k5_launch_rmsnorm_rope(cx.v[k].ck, a.norm.as<float>() + 64, nullptr, nullptr, cx.v[k].L, H, cx.v[k].ldck, nullptr, s));
  }
  {
    Scope sc(d, s, "attn_cross");
    const K5QueryNorm qn{a.norm.as<float>(), nullptr, nullptr, nullptr};
    K5AttnRangeArgs at;
    at.Q = q; at.H = H; at.q_len = rows; at.ldq = D; at.ldo = D;
    at.score_bound = a.score_bound; at.stream = s;
    at.query_norm = fuse_qnorm ? &qn : nullptr;
    for (int k = 0; k < cx.n; ++k) {   // the same (normalised or to-be-normalised) queries against every stream
      const CrossView& v = cx.v[k];
      at.K = v.ck; at.Vt = v.cvt; at.O = v.o;
      at.kv_len = v.L; at.ldk = v.ldck; at.ldvt = v.ldvt;
      K5CHK(k5_launch_attention_bf16_range(at));
    }
  }
  if (cx.R) {
    Scope sc(d, s, "elementwise");
    K5CHK(k5_launch_region_combine(o, cx.v[cx.n - cx.R].o, cx.region_o_stride, cx.R, cx.region_w, cx.R + 1, o, rows, D, D, s));
    ++d->regions.combines;
  }
  if (cx.nag) {
    Scope sc(d, s, "elementwise");
    K5CHK(k5_launch_nag_combine(o, cx.v[1].o, o, rows, D, D, d->nag.scale, d->nag.tau, d->nag.alpha, s));
    ++d->nag.combines;
  }
  return attn_out_projection(d, s, a, o, rows, resid, gate);
}

int run_ff(k5_dit* d, hipStream_t s, const BlockW& b, const void* h, int rows, void* ff, void* resid, const float* gate, bool h8_ready = false) {
  const int D = d->D, FF = d->FF;
  // opt-in lossy path (ff_fp8_in): h -> e4m3 (static scale; by the LayerNorm itself when h8_ready), FF1 on the fp8 MFMA with the GELU epilogue
  // writing e4m3 into ws_ff8, FF2 reading that, likewise with the gated-residual epilogue (gemm_fp8.hip)
  const bool f8 = ff_fp8_in(d, b, rows);
  if (f8) K5CHK(d->ws_ff8.ensure((size_t)rows * FF, (size_t)K5_GEMM_GUARD_ROWS * FF));
  Act x;
  K5CHK(e4m3_rows(d, s, h, rows, f8, h8_ready, x));
  LinearArgs g1(b.w1, x, f8 ? d->ws_ff8.p : ff, FF, s), g2(b.w2, Act{ff, f8 ? d->ws_ff8.p : nullptr, rows, FF}, resid, D, s);
  g1.epi = K5_EPI_GELU;
  g2.epi = K5_EPI_GATE; g2.resid = resid; g2.ldr = D; g2.gate = gate;
  Scope sc(d, s, "gemm");
  K5CHK(linear(g1));
  return linear(g2);
}

// forget which heads the per-row-offset softmax served badly (AttnW::pref): the memory is a speed hint for the NEXT step of the SAME sampling
// run; carried across runs it made results depend on what the handle had computed before
int reset_attn_pref(k5_dit* d, hipStream_t s, bool sync = false) {
  if (sync) HIPCHK(hipDeviceSynchronize());   // called outside any stream order (k5_dit_set_option): nothing may still be reading the flags
  for (auto& b : d->vblocks)
    if (b.self_attn.pref.p) HIPCHK(hipMemsetAsync(b.self_attn.pref.p, 0, b.self_attn.pref.bytes, s));
  if (sync) HIPCHK(hipDeviceSynchronize());
  return K5_OK;
}

int ln_mod(k5_dit* d, hipStream_t s, const void* x, const float* mod3, void* out, int rows, bool to_e4m3 = false) {
  // mod3 = [shift | scale | gate] (dit.py:36,40,64,69,74).  to_e4m3: every consumer of this h is an fp8 GEMM — the rows go to ws_h8 as e4m3
  // (the bf16 rounding, then the e4m3 one: what the separate quantisation pass made of the bf16 h), and no bf16 h is written at all
  if (to_e4m3) K5CHK(d->ws_h8.ensure((size_t)rows * d->D, (size_t)K5_GEMM_GUARD_ROWS * d->D));
  Scope sc(d, s, "elementwise");
  return k5_launch_ln_modulate(x, mod3 + d->D, mod3, to_e4m3 ? nullptr : out, rows, d->D, d->D, d->D, s, to_e4m3 ? d->ws_h8.p : nullptr);
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
// N visual tokens; L: the longest prompt of the forward, which sizes the text side's shared scratch (a text stream sizes what it keeps itself)
int ensure_workspaces(k5_dit* d, int N, int L) {
  const size_t D = d->D, FF = d->FF;
  const size_t Lr = rup(L, 8), Nr = rup(N, 8);
  const size_t gs = (size_t)K5_GEMM_GUARD_ROWS * 2;   // the rows a GEMM may read past an activation operand, in bytes per bf16 element of a row
  K5CHK(d->ws_text_in.ensure((size_t)L * d->cfg.in_text_dim * 2, gs * d->cfg.in_text_dim));
  K5CHK(d->ws_th.ensure(L * D * 2, gs * D)); K5CHK(d->ws_tqk.ensure(L * 2 * D * 2, gs * 2 * D));
  K5CHK(d->ws_tvt.ensure(D * Lr * 2, gs * Lr)); K5CHK(d->ws_to.ensure(L * D * 2, gs * D)); K5CHK(d->ws_tff.ensure(L * FF * 2, gs * FF));
  K5CHK(d->ws_pool_in.ensure((size_t)rup(d->cfg.in_text_dim2, 8) * 2)); K5CHK(d->ws_pool_lin.ensure(d->TD * 2));
  K5CHK(d->ws_pool_f32.ensure(d->TD * 4)); K5CHK(d->ws_time.ensure(16)); K5CHK(d->ws_tfeat.ensure(D * 4));
  K5CHK(d->ws_th1.ensure(d->TD * 4)); K5CHK(d->ws_temb.ensure(d->TD * 4)); K5CHK(d->ws_mod.ensure(d->mod_rows * 4));
  K5CHK(d->ws_xp.ensure((size_t)N * d->KvisPad * 2, gs * d->KvisPad)); K5CHK(d->ws_vis.ensure(N * D * 2, gs * D)); K5CHK(d->ws_h.ensure(N * D * 2, gs * D));
  K5CHK(d->ws_qk.ensure((size_t)N * 2 * D * 2, gs * 2 * D)); K5CHK(d->ws_vt.ensure(D * Nr * 2, gs * Nr)); K5CHK(d->ws_o.ensure(N * D * 2, gs * D));
  K5CHK(d->ws_ff.ensure((size_t)N * FF * 2, gs * FF));
  K5CHK(d->ws_y.ensure((size_t)N * d->Fout * 2));
  K5CHK(d->ws_vcos.ensure((size_t)N * 32 * 4)); K5CHK(d->ws_vsin.ensure((size_t)N * 32 * 4));
  return K5_OK;
}

int prepare_rope(k5_dit* d, hipStream_t s, const k5_forward_args* a, int Tp, int Hp, int Wp, const int32_t* tok_perm) {
  // visual tables: recompute only when the (shape, positions, scale) key changes — step-invariant (K15)
  std::vector<int32_t> key;
  key.insert(key.end(), a->pos_t, a->pos_t + Tp); key.insert(key.end(), a->pos_h, a->pos_h + Hp);
  key.insert(key.end(), a->pos_w, a->pos_w + Wp);
  const bool same = key == d->key_vpos && d->key_shape[0] == Tp && d->key_shape[1] == Hp && d->key_shape[2] == Wp &&
                    !memcmp(d->key_scale, a->scale_factor, 12) && d->key_fractal == (tok_perm != nullptr);
  if (!same) {
    K5CHK(d->ws_pos.ensure(key.size() * 4));
    HIPCHK(hipMemcpyAsync(d->ws_pos.p, key.data(), key.size() * 4, hipMemcpyHostToDevice, s));
    const int32_t* p = d->ws_pos.as<int32_t>();
    const int n0 = d->cfg.axes_dims[0] / 2, n1 = d->cfg.axes_dims[1] / 2, n2 = d->cfg.axes_dims[2] / 2;
    K5CHK(k5_launch_rope_table(d->ws_vcos.as<float>(), d->ws_vsin.as<float>(), p, p + Tp, p + Tp + Hp, Tp, Hp, Wp, n0, n1,
                               n2, a->scale_factor[0], a->scale_factor[1], a->scale_factor[2], tok_perm, s));
    HIPCHK(hipStreamSynchronize(s));  // key vector is host memory reused below; once per shape only
    d->key_fractal = tok_perm != nullptr;
    d->key_vpos = key; d->key_shape[0] = Tp; d->key_shape[1] = Hp; d->key_shape[2] = Wp;
    memcpy(d->key_scale, a->scale_factor, 12);
  }
  return K5_OK;
}

int prepare_text_rope(k5_dit* d, hipStream_t s, const k5_text_cond& c, const float** cosT, const float** sinT) {
  // RoPE1D tables (nn.py:99-116) are step-invariant: cache per position vector (cond / null cond)
  std::vector<int32_t> key(c.text_rope_pos, c.text_rope_pos + c.text_len);
  for (auto& e : d->text_rope)
    if (e.key == key) { *cosT = e.cosT.as<float>(); *sinT = e.sinT.as<float>(); return K5_OK; }
  if (d->text_rope.size() >= 16) {   // two prompts, a negative one and eight regions fit: a captured step must find its tables here
    HIPCHK(hipStreamSynchronize(s));
    for (auto& e : d->text_rope) { e.cosT.release(); e.sinT.release(); e.pos.release(); }
    d->text_rope.clear();
  }
  d->text_rope.emplace_back();
  auto& e = d->text_rope.back();
  e.key = key;
  K5CHK(e.pos.ensure(key.size() * 4)); K5CHK(e.cosT.ensure(key.size() * 32 * 4)); K5CHK(e.sinT.ensure(key.size() * 32 * 4));
  HIPCHK(hipMemcpyAsync(e.pos.p, e.key.data(), key.size() * 4, hipMemcpyHostToDevice, s));
  K5CHK(k5_launch_rope_table(e.cosT.as<float>(), e.sinT.as<float>(), e.pos.as<int32_t>(), nullptr, nullptr, c.text_len, 1,
                             1, 32, 0, 0, 1.f, 1.f, 1.f, nullptr, s));
  HIPCHK(hipStreamSynchronize(s));  // once per distinct prompt length
  *cosT = e.cosT.as<float>(); *sinT = e.sinT.as<float>();
  return K5_OK;
}

int to_bf16(k5_dit* d, hipStream_t s, const void* src, int dtype, size_t n, DevBuf& dst, const void** out) {
  (void)d;
  if (dtype == K5_BF16) { *out = src; return K5_OK; }
  if (dtype != K5_F32) { k5_set_error("text embeddings must be f32 or bf16"); return K5_ERR_UNSUPPORTED; }
  K5CHK(dst.ensure(n * 2));
  K5CHK(k5_launch_cast_f32_bf16((const float*)src, dst.p, (int64_t)n, s));
  *out = dst.p;
  return K5_OK;
}

// ---------------------------------------------------------------------------------------------
// self-tuning sequence-parallel schedule (see k5_dit::sp_autotune)
// ---------------------------------------------------------------------------------------------
struct SpCand { int mode, slices, passes; const char* name; };

// Token shards of a sequence-parallel forward: whole 64-token blocks, ceil(blocks / P) per rank in whole slices (the sliced K / V^T exchange,
// "sp_slices"); the last rank takes what is left (3660 blocks over 8 ranks: 7 x 458 + 454).  n_pad = slot size in the gather buffers, n = rows
// `rank` really owns from token tok0 on; idle: the slot size leaves a rank without rows.  The forward's layout and the autotune's candidates
struct Shard { int n, n_pad, tok0; bool idle; };
Shard shard_layout(int N, int P, int slices, int rank) {
  const int S = slices > 1 ? slices : 1;
  const int n_pad = ((N / 64 + P * S - 1) / (P * S)) * S * 64, tok0 = rank * n_pad;
  return {N - tok0 < n_pad ? N - tok0 : n_pad, n_pad, tok0, (long long)(P - 1) * n_pad >= N};
}

// pure host logic, exported for a CPU test (k5_sp_pick_schedule): candidate c costs max over ranks of times[r * ncand + c] (a collective
// schedule is as slow as its slowest rank); the cheapest valid one wins, ties to the lowest index (= the more conservative schedule);
// a non-finite or non-positive time disqualifies the candidate on every rank alike (all ranks see the same gathered table)
int sp_pick(const float* times, int ncand, int world, const int* valid, float* cost_out) {
  int best = -1; float best_t = 0.f;
  for (int c = 0; c < ncand; ++c) {
    float t = 0.f; bool ok = !valid || valid[c];
    for (int r = 0; r < world && ok; ++r) {
      const float v = times[(size_t)r * ncand + c];
      if (!(v > 0.f) || !(v < 3.0e38f)) ok = false; else t = v > t ? v : t;
    }
    if (cost_out) cost_out[c] = ok ? t : -1.f;
    if (ok && (best < 0 || t < best_t)) { best = c; best_t = t; }
  }
  return best;
}

// the workspaces of a sharded forward whose slots hold n_pad rows: the gather buffers take every rank's slot
int ensure_sp_workspaces(k5_dit* d, int n_pad, int L) {
  const size_t P = d->sp_world, slot = (size_t)n_pad * d->D * 2;
  K5CHK(ensure_workspaces(d, (int)P * n_pad, L));
  K5CHK(d->ws_q.ensure(slot)); K5CHK(d->ws_kfull.ensure(P * slot));
  return d->ws_vtfull.ensure(P * slot);
}

int sp_autotune_run(k5_dit* d, hipStream_t s, int N, int L, const NablaArgs* nabla) {
  const int P = d->sp_world, H = d->Hh, D = d->D;
  d->sp_tuned = true;                                  // once per handle; the guard below takes it back if the run does not complete
  std::vector<SpCand> cands;
  if (!nabla) {
    cands.push_back({0, 1, 1, "K / V^T all-gather"});
    if (!(d->sp_user_set & 3) && d->comm.can_exchange() && N / 64 >= 4 * P) cands.push_back({0, 2, 1, "K / V^T exchange in 2 slices"});
    if (!(d->sp_user_set & 3) && H % P == 0 && d->comm.can_exchange()) cands.push_back({1, 1, 1, "Ulysses all-to-all"});
  } else {
    cands.push_back({0, 1, 1, "all-gather, one pass over the lists"});
    if (!(d->sp_user_set & 4)) cands.push_back({0, 1, 2, "all-gather, own key blocks first (two passes)"});
  }
  const int nc = (int)cands.size();
  if (nc < 2) { d->sp_report = "{\"tuned\": false, \"reason\": \"one admissible schedule\"}"; return K5_OK; }
  const int save_mode = d->sp_mode, save_slices = d->sp_slices, save_passes = d->sp_nabla_passes, save_prof = d->profiling;
  // every exit path — the failure returns inside the candidate loop included — leaves the handle as it found it: the caller's options and profiling
  // level, no leaked events, the RoPE cache invalidated (the trial runs zeroed the tables), and "not tuned" unless the run completed
  struct Guard {
    k5_dit* d; int mode, slices, passes, prof; hipEvent_t e0 = nullptr, e1 = nullptr; bool done = false;
    ~Guard() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
      d->profiling = prof;
      d->key_vpos.clear(); d->key_shape[0] = d->key_shape[1] = d->key_shape[2] = 0;
      d->nabla_hint_pending = false;
      if (!done) { d->sp_mode = mode; d->sp_slices = slices; d->sp_nabla_passes = passes; d->sp_tuned = false; }
    }
  } guard{d, save_mode, save_slices, save_passes, save_prof};
  d->profiling = 0;
  unsigned long long cnt_save[4] = {0, 0, 0, 0};       // the trial launches must not show up in the softmax-form counters (k5_dit_attn_variant_counts)
  K5CHK(ensure_zeroed(d->ws_attn_cnt, 32, s));
  HIPCHK(hipMemcpyAsync(cnt_save, d->ws_attn_cnt.p, 32, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipEventCreate(&guard.e0)); HIPCHK(hipEventCreate(&guard.e1));
  const hipEvent_t e0 = guard.e0, e1 = guard.e1;
  std::vector<float> mine(nc, -1.f);
  double comm_ms = -1.0, comm_bytes = 0.0;
  const AttnW& a = d->vblocks[0].self_attn;
  for (int c = 0; c < nc; ++c) {
    d->sp_mode = cands[c].mode; d->sp_slices = cands[c].slices; d->sp_nabla_passes = cands[c].passes;
    const Shard sh = shard_layout(N, P, d->sp_slices, d->sp_rank);
    if (sh.idle) continue;       // this slot size leaves a rank without rows: not a candidate (time stays -1 everywhere)
    const int n = sh.n, n_pad = sh.n_pad, tok0 = sh.tok0;
    K5CHK(ensure_sp_workspaces(d, n_pad, L));
    // finite, harmless operands: activations 0.1 (bf16 0x3dcd), rotary tables and gates zero (the out projection then adds nothing)
    HIPCHK(hipMemsetD16Async((hipDeviceptr_t)d->ws_h.p, 0x3dcd, (size_t)n_pad * D, s));
    HIPCHK(hipMemsetD16Async((hipDeviceptr_t)d->ws_vis.p, 0x3dcd, (size_t)n_pad * D, s));
    HIPCHK(hipMemsetAsync(d->ws_vcos.p, 0, (size_t)N * 32 * 4, s)); HIPCHK(hipMemsetAsync(d->ws_vsin.p, 0, (size_t)N * 32 * 4, s));
    HIPCHK(hipMemsetAsync(d->ws_mod.p, 0, d->mod_rows * 4, s));
    const float* cosT = d->ws_vcos.as<float>() + (size_t)tok0 * 32; const float* sinT = d->ws_vsin.as<float>() + (size_t)tok0 * 32;
    const bool uly = d->sp_mode == 1;
    // a line per candidate BEFORE it runs: if an exchange never used on this node hangs, the log says which ("sp_autotune" = 0 / K5_SP_AUTOTUNE=0 skip the tuning)
    if (d->sp_rank == 0) fprintf(stderr, "libk5: sequence-parallel schedule: timing candidate %d of %d: %s\n", c + 1, nc, cands[c].name);
    int trial_rc = K5_OK;   // a candidate that REFUSES its arguments does so on every rank alike (argument checks only): it is disqualified, not fatal
    for (int it = 0; it < 3 && trial_rc == K5_OK; ++it) {
      if (it == 1) HIPCHK(hipEventRecord(e0, s));
      trial_rc = uly ? run_self_attention_heads(d, s, a, d->ws_h.p, n, n_pad, N, d->ws_o.p, cosT, sinT, d->ws_vis.p, d->ws_mod.as<float>(), false)
                     : run_self_attention_sp(d, s, a, d->ws_h.p, n, n_pad, N, d->ws_o.p, cosT, sinT, d->ws_vis.p, d->ws_mod.as<float>(), nabla);
    }
    if (trial_rc != K5_OK) {
      if (c == 0) return trial_rc;       // the default schedule itself fails: nothing to fall back to
      HIPCHK(hipStreamSynchronize(s));
      continue;
    }
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    mine[c] = ms / 2.f;
    if (c == 0) {   // the bare exchange of candidate 0 (both all-gathers back to back, nothing else running): achieved ingress bandwidth
      HIPCHK(hipEventRecord(e0, s));
      for (int it = 0; it < 2; ++it) {
        K5CHK(d->comm.all_gather_inplace(d->ws_kfull.p, (size_t)n_pad * D, 2, s));
        K5CHK(d->comm.all_gather_inplace(d->ws_vtfull.p, (size_t)D * n_pad, 2, s));
      }
      HIPCHK(hipEventRecord(e1, s)); HIPCHK(hipEventSynchronize(e1));
      HIPCHK(hipEventElapsedTime(&ms, e0, e1));
      comm_ms = ms / 2.0; comm_bytes = 2.0 * (double)(P - 1) * n_pad * D * 2.0;
    }
  }
  // every rank's table to every rank, then the same decision everywhere
  K5CHK(d->ws_tune.ensure((size_t)P * nc * 4));
  HIPCHK(hipMemcpyAsync(d->ws_tune.as<float>() + (size_t)d->sp_rank * nc, mine.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s));
  K5CHK(d->comm.all_gather_inplace(d->ws_tune.p, (size_t)nc, 4, s));
  std::vector<float> all((size_t)P * nc), cost(nc);
  HIPCHK(hipMemcpyAsync(all.data(), d->ws_tune.p, all.size() * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const int best = sp_pick(all.data(), nc, P, nullptr, cost.data());
  // the trial runs used the handle's workspaces with made-up operands: put back what outlives a forward
  HIPCHK(hipMemcpyAsync(d->ws_attn_cnt.p, cnt_save, 32, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));                     // cnt_save is a local
  K5CHK(reset_attn_pref(d, s));
  guard.done = true;                                   // from here on the run counts as tuned (the guard still restores profiling and drops the RoPE cache)
  d->sp_mode = save_mode; d->sp_slices = save_slices; d->sp_nabla_passes = save_passes;
  if (best < 0) { d->sp_report = "{\"tuned\": false, \"reason\": \"no candidate ran\"}"; return K5_OK; }
  // only what this run VARIED is taken from the winner (a dense run never touches "sp_nabla_passes", a NABLA run never "sp_mode" / "sp_slices"),
  // and a knob the caller set is never a varied one (the candidate lists above leave it out)
  if (!nabla) { d->sp_mode = cands[best].mode; d->sp_slices = cands[best].slices; }
  else d->sp_nabla_passes = cands[best].passes;
  char buf[256];
  std::string rep = "{\"tuned\": true, \"world\": " + std::to_string(P) + ", \"tokens\": " + std::to_string(N) + ", \"attention\": \"" + (nabla ? "nabla" : "dense") +
                    "\", \"chosen\": \"" + cands[best].name + "\", \"unit\": \"ms per block's self-attention section, max over ranks\", \"candidates\": [";
  for (int c = 0; c < nc; ++c) {
    snprintf(buf, sizeof(buf), "%s{\"name\": \"%s\", \"ms\": %.4f, \"ms_this_rank\": %.4f}", c ? ", " : "", cands[c].name, cost[c], mine[c]);
    rep += buf;
  }
  snprintf(buf, sizeof(buf), "], \"gather_bytes_in_per_block\": %.0f, \"gather_ms_alone\": %.4f, \"gather_GBps_in\": %.1f}", comm_bytes, comm_ms,
           comm_ms > 0 ? comm_bytes / comm_ms * 1e-6 : 0.0);
  rep += buf;
  d->sp_report = rep;
  if (d->sp_rank == 0) fprintf(stderr, "libk5: sequence-parallel schedule: %s\n", rep.c_str());
  return K5_OK;
}

// which self-attention schedule a sharded forward runs (0 gather, 1 Ulysses, 2 two-level): the dispatch's predicate, shared with "fp8_effective".
// "sp_mode" 2 runs Ulysses where G = gcd(heads, P) = P, the gather where G = 1; NABLA and the timing-only layout keep the gather as under "sp_mode" 1,
// except that the two-level schedule does run under "emulate_world" (rank 0's layout, collectives move nothing: its per-rank compute).
int sp_schedule(const k5_dit* d, bool nabla) {
  const int P = d->sp_world, H = d->Hh;
  if (!d->comm.active() || P <= 1 || nabla) return 0;
  if (d->sp_mode == 1) return (H % P == 0 && !d->emulated) ? 1 : 0;
  if (d->sp_mode == 2) {
    const int G = sp_gcd(H, P);
    if (G == P) return d->emulated ? 0 : 1;
    return G > 1 ? 2 : 0;
  }
  return 0;
}

// ---- a prompt's way through the text side of a forward, in three parts: text_stream_run is all of them ----
// TextEmbeddings of prompt c into st.text (dit.py:132), inside the caller's "prologue" bracket; pooled: with its pooled projection into
// ws_pool_f32 (dit.py:134).  tc: restored from there if it holds this prompt, otherwise left there for the later steps of the k5_sample* call
int text_embeddings(k5_dit* d, hipStream_t s, const k5_text_cond& c, k5_dit::TextStream& st, k5_dit::TextCache* tc, bool pooled) {
  const k5_dit_config& cfg = d->cfg;
  const int L = st.L = c.text_len, D = d->D;
  K5CHK(st.text.ensure((size_t)L * D * 2));
  if (tc && tc->valid && tc->L == L) {   // the text blocks update st.text in place: restore their input
    HIPCHK(hipMemcpyAsync(st.text.p, tc->text.p, (size_t)L * D * 2, hipMemcpyDeviceToDevice, s));
    if (pooled) HIPCHK(hipMemcpyAsync(d->ws_pool_f32.p, tc->pool.p, (size_t)d->TD * 4, hipMemcpyDeviceToDevice, s));
    return K5_OK;
  }
  if (d->fe.active) d->fe.prologues += 1;
  const void* text_bf; const void* pool_bf;
  K5CHK(to_bf16(d, s, c.text_embed, c.text_dtype, (size_t)L * cfg.in_text_dim, d->ws_text_in, &text_bf));
  if (pooled) K5CHK(to_bf16(d, s, c.pooled_embed, c.text_dtype, (size_t)cfg.in_text_dim2, d->ws_pool_in, &pool_bf));
  K5CHK(linear(LinearArgs(d->text_lin, Act{text_bf, nullptr, L, cfg.in_text_dim}, d->ws_th.p, D, s)));
  K5CHK(k5_launch_ln_affine(d->ws_th.p, d->text_lnw.as<float>(), d->text_lnb.as<float>(), st.text.p, nullptr, L, D, s));
  if (pooled) {
    K5CHK(linear(LinearArgs(d->pool_lin, Act{pool_bf, nullptr, 1, cfg.in_text_dim2}, d->ws_pool_lin.p, d->TD, s)));
    K5CHK(k5_launch_ln_affine(d->ws_pool_lin.p, d->pool_lnw.as<float>(), d->pool_lnb.as<float>(), nullptr,
                              d->ws_pool_f32.as<float>(), 1, d->TD, s));
  }
  if (tc) {
    K5CHK(tc->text.ensure((size_t)L * D * 2));
    if (pooled) K5CHK(tc->pool.ensure((size_t)d->TD * 4));
    HIPCHK(hipMemcpyAsync(tc->text.p, st.text.p, (size_t)L * D * 2, hipMemcpyDeviceToDevice, s));
    if (pooled) HIPCHK(hipMemcpyAsync(tc->pool.p, d->ws_pool_f32.p, (size_t)d->TD * 4, hipMemcpyDeviceToDevice, s));
    tc->valid = true; tc->L = L;
  }
  return K5_OK;
}

// the text blocks on st.text, in place (dit.py:170-171, 33-44); mod: the forward's modulation, whichever stream runs
int text_blocks_run(k5_dit* d, hipStream_t s, k5_dit::TextStream& st, const float* tcos, const float* tsin, const float* mod) {
  const int D = d->D, L = st.L;
  for (const BlockW& b : d->tblocks) {
    const float* m = mod + b.mod_off;
    K5CHK(ln_mod(d, s, st.text.p, m, d->ws_th.p, L));
    K5CHK(run_self_attention(d, s, b.self_attn, d->ws_th.p, L, d->ws_tqk.p, d->ws_tvt.p, d->ws_to.p, tcos, tsin, st.text.p, m + 2 * D, "attn_text"));
    K5CHK(ln_mod(d, s, st.text.p, m + 3 * D, d->ws_th.p, L));
    K5CHK(run_ff(d, s, b, d->ws_th.p, L, d->ws_tff.p, st.text.p, m + 5 * D));
  }
  return K5_OK;
}

// what the visual blocks' cross-attention needs of st: stacked, the keys / V^T of all blocks now; otherwise room for one block's
int text_cross_kv(k5_dit* d, hipStream_t s, k5_dit::TextStream& st, bool stacked) {
  if (stacked) return cross_kv_batched_run(d, s, st);
  K5CHK(st.ck.ensure((size_t)st.L * d->D * 2));
  return st.cvt.ensure((size_t)d->D * rup(st.L, 8) * 2);
}

// all of it for a prompt whose stream has nothing else in its prologue: its own RoPE positions, THIS forward's modulation (one time embedding
// per forward: that of the forward's own pooled embedding)
int text_stream_run(k5_dit* d, hipStream_t s, const k5_text_cond& c, k5_dit::TextStream& st, k5_dit::TextCache* tc, const float* mod, bool stacked) {
  const float *tcos = nullptr, *tsin = nullptr;
  K5CHK(prepare_text_rope(d, s, c, &tcos, &tsin));
  {
    Scope sc(d, s, "prologue");
    K5CHK(text_embeddings(d, s, c, st, tc, false));
  }
  K5CHK(text_blocks_run(d, s, st, tcos, tsin, mod));
  return text_cross_kv(d, s, st, stacked);
}

// which MagCache mode the handle is in, as the refusal messages say it ("... %s on the handle"); nullptr = neither
static const char* magcache_mode(const k5_dit* d) {
  return d->mag.on ? "MagCache is set" : d->cal.on ? "MagCache calibration is" : nullptr;
}

// NABLA's fractal token order (utils.py:31-41,54-78): 8 x 8 spatial tiles contiguous.  Row i of that order holds token (t, y, x)
struct Tok { int t, y, x; };
Tok fractal_token(int i, int Hp, int Wp) {
  const int Hb = Hp / 8, Wb = Wp / 8, b = i >> 6, r = i & 63;
  return {b / (Hb * Wb), (b / Wb) % Hb * 8 + (r >> 3), b % Wb * 8 + (r & 7)};
}
// A table over the rows of that order, cached per shape: put(v, i, the token of row i) fills it.  The upload is synchronous: the eager first step
// of a shape reaches it, a captured step finds the table
template <class Put> int token_table(DevBuf& buf, int (&shape)[3], int Tp, int Hp, int Wp, Put put) {
  if (shape[0] == Tp && shape[1] == Hp && shape[2] == Wp) return K5_OK;
  const int N = Tp * Hp * Wp;
  std::vector<int32_t> v((size_t)N);
  for (int i = 0; i < N; ++i) put(v.data(), i, fractal_token(i, Hp, Wp));
  K5CHK(buf.ensure((size_t)N * 4));
  HIPCHK(hipMemcpy(buf.p, v.data(), (size_t)N * 4, hipMemcpyHostToDevice));
  shape[0] = Tp; shape[1] = Hp; shape[2] = Wp;
  return K5_OK;
}

// One forward as its caller asks for it: k5_dit_forward, k5_dit_forward_skip (k5_dit_forward_many through the first) and SampleRun::forward fill it
struct ForwardCall {
  const k5_forward_args* a; const k5_text_cond& cond; float time;
  const float* x; int x_channels;
  void* out; hipStream_t s;
  const float* tvec = nullptr; const int* step = nullptr;   // a captured step reads its time through the device-side step tables and counter
  int text_slot = -1;                                        // the text cache slot of a k5_sample* call (0 cond, 1 uncond); -1: a forward of its own
  int cache_slot = -1;                                       // FlowEdit's source prompt: the text_cache entry of the forward's own prompt where it is not text_slot
  const float* vcond = nullptr;                              // visual conditioning beside an x of in_visual_dim channels
  void* out_skip = nullptr;                                  // the forking forward: where the skip branch's velocity goes
  int fc_step = -1, fc_slot = 0;                             // the forecast cache's cursor: this forward is call (step, slot) of the plan; -1: a plain forward
  int64_t x_frame = 0, x_row = 0, vc_frame = 0, vc_row = 0;  // a spatial window: x (and vcond) is a strided view, in elements; x_row == 0: compact
};

struct ForwardShape {   // patched frames / rows / columns, visual tokens, text rows, model width, input channels of the patch embedding
  int Tp, Hp, Wp, N, L, D, Cin;
  ForwardShape(const k5_dit* d, const ForwardCall& f)
      : Tp(f.a->T), Hp(f.a->H / 2), Wp(f.a->W / 2), N(Tp * Hp * Wp), L(f.cond.text_len), D(d->D),
        Cin(d->cfg.visual_cond ? 2 * d->cfg.in_visual_dim + 1 : d->cfg.in_visual_dim) {}
};

// Everything forward_impl refuses on its arguments and the handle's settings, before anything is enqueued or allocated and before any per-forward
// state is touched: no HIP call and no write to the handle here.  (One refusal depends on the run, not on the settings: ForwardRun::shard.)
static int forward_refusals(const k5_dit* d, const ForwardCall& f) {
  const k5_dit_config& c = d->cfg;
  const k5_forward_args* a = f.a;
  if (!d->finalized) { k5_set_error("k5_dit_forward before k5_dit_finalize"); return K5_ERR_STATE; }
  if (a->attention_type != 0 && a->attention_type != 1) { k5_set_error("attention_type must be 0 (flash) or 1 (nabla)"); return K5_ERR_ARG; }
  if (c.patch_size[0] != 1 || c.patch_size[1] != 2 || c.patch_size[2] != 2) return K5_ERR_UNSUPPORTED;
  const ForwardShape sh(d, f);
  if (sh.N <= 0 || sh.L <= 0 || (a->H & 1) || (a->W & 1)) { k5_set_error("bad shapes"); return K5_ERR_ARG; }
  if (f.x_channels != sh.Cin && f.x_channels != c.in_visual_dim) { k5_set_error("x_channels must be %d or %d", sh.Cin, c.in_visual_dim); return K5_ERR_ARG; }
  if (f.vcond && (!c.visual_cond || f.x_channels != c.in_visual_dim)) { k5_set_error("visual_cond needs a visual_cond model and x of in_visual_dim channels"); return K5_ERR_ARG; }
  const int P = d->sp_world;
  const bool sp = d->comm.active();  // a communicator (even of size 1) selects the sharded code path
  if (f.out_skip) {   // the forking forward (k5_dit_forward_skip, a skip step of k5_sample*)
    if (!d->skip.on) { k5_set_error("k5_dit_forward_skip: no skip set on the handle (k5_dit_set_skip_guidance)"); return K5_ERR_STATE; }
    if (const char* mode = magcache_mode(d)) {
      k5_set_error("k5_dit_forward_skip: %s on the handle: the ratio table is indexed by the calls of a plain run", mode);
      return K5_ERR_STATE;
    }
  }
  if (f.fc_step >= 0) {   // a call of the forecast plan (what depends on the shard: ForwardRun::shard)
    if (f.out_skip) { k5_set_error("k5_dit_forward_skip: a forecast plan is set (k5_dit_set_forecast): the skip branch has no slot"); return K5_ERR_STATE; }
    if (d->pair.active()) { k5_set_error("a forecast plan is set (k5_dit_set_forecast) and the handle is in a CFG pair: not built"); return K5_ERR_STATE; }
  }
  if (const k5_dit::MagCalib& cl = d->cal; cl.on) {
    if (sp || d->pair.active()) { k5_set_error("MagCache calibration is a one-GPU job: the handle is in a %s", sp ? "sequence-parallel group" : "CFG pair"); return K5_ERR_STATE; }
    if (cl.cnt >= 2 && cl.res_elems[cl.slot()] != (size_t)sh.N * sh.D) {
      k5_set_error("MagCache calibration: this forward has %d x %d residual elements, the previous call of its slot had %zu", sh.N, sh.D, cl.res_elems[cl.slot()]);
      return K5_ERR_ARG;
    }
  }
  if (sp) {   // with the slices the handle has now: a tuning run that follows only picks slot sizes that leave no rank without work
    if (sh.N % 64) { k5_set_error("sequence parallelism needs whole 64-token blocks (token count %d)", sh.N); return K5_ERR_UNSUPPORTED; }
    if (shard_layout(sh.N, P, d->sp_slices, d->sp_rank).idle) { k5_set_error("sequence parallel x%d: %d token blocks leave a rank without work", P, sh.N / 64); return K5_ERR_UNSUPPORTED; }
  }
  const k5_dit::Regions& rg = d->regions;
  if (rg.on && (a->T != rg.T || a->H != rg.H || a->W != rg.W)) {
    k5_set_error("regional prompts: the masks are (%d, %d, %d), this forward is (%d, %d, %d)", rg.T, rg.H, rg.W, a->T, a->H, a->W);
    return K5_ERR_ARG;
  }
  if (d->enh.applies(sh.Tp, c.num_visual_blocks)) {
    if (sp) {
      k5_set_error("Enhance-A-Video is set (k5_dit_set_enhance) and the handle is in a sequence-parallel group: the frames of a column live on different ranks");
      return K5_ERR_STATE;
    }
    if (sh.Tp > 64) {
      k5_set_error("Enhance-A-Video is set (k5_dit_set_enhance): %d frames are more than a wave's four 32 x 32 accumulators hold (64)", sh.Tp);
      return K5_ERR_UNSUPPORTED;
    }
  }
  if (a->attention_type == 1 && ((sh.Hp % 8) || (sh.Wp % 8))) { k5_set_error("nabla attention needs latent H, W divisible by 16 (got %d x %d)", a->H, a->W); return K5_ERR_ARG; }
  return K5_OK;
}

// What one forward_impl call works on: filled top to bottom by shard() and token_order() before the first launch, then read by the phases in the
// order forward_impl names them.
struct ForwardRun : ForwardShape {
  k5_dit* const d; const ForwardCall& f; const k5_forward_args* const a; const hipStream_t s;
  const bool sp, nabla;                     // sp: a communicator (even of size 1) selects the sharded code path
  // normalized attention guidance and regional prompts: the conditional branch only (slot 1 is the unconditional forward of k5_sample*)
  const k5_text_cond* const ncond; const int Rg;
  int n, n_pad, tok0 = 0, sched = 0;        // the shard (shard_layout) and its self-attention schedule (sp_schedule)
  NablaArgs na{}; const int32_t* perm = nullptr;   // NABLA: its arguments, and the permutation of the fractal order its tokens are processed in
  const float *mod = nullptr, *tcos = nullptr, *tsin = nullptr;   // every Modulation layer's output (one vector per forward); the prompt's RoPE tables
  // the text streams of this forward's cross-attentions, in launch order, and where each one's attention output goes: the forward's own prompt,
  // then the negative one of k5_dit_set_nag, then the regions' of k5_dit_set_regions; nothing but the first on a step MagCache skips
  struct { const k5_text_cond* cond; int stream; void* o; } act[1 + 1 + 8];   // stream: its index in k5_dit::streams
  CrossStreams cx; bool cx_all = false;     // cx_all: the streams hold the keys / V^T of all visual blocks ("cross_kv_batched")
  bool mag_skip = false;                    // MagCache skips this call's visual blocks
  int fc_kind = 0;                          // the forecast cache: 0 a plain forward, 1 a full call, 2 a forecast call (the blocks are skipped)
  bool no_blocks() const { return mag_skip || fc_kind == 2; }
  int fork_at = -1;                         // skip-layer guidance: the block whose input the skip branch starts from
  size_t vis_elems() const { return (size_t)n * D; }

  ForwardRun(k5_dit* d_, const ForwardCall& f_)
      : ForwardShape(d_, f_), d(d_), f(f_), a(f_.a), s(f_.s), sp(d_->comm.active()), nabla(f_.a->attention_type == 1),
        ncond(d_->nag.on && f_.text_slot != 1 ? d_->nag.neg : nullptr), Rg(d_->regions.on && f_.text_slot != 1 ? d_->regions.R : 0), n(N), n_pad(N) {}

  // ---- the shard, what the forward decides before its first launch, and the workspaces ----
  int shard() {
    if (nabla) {   // NABLA workgroup size of this forward (see nabla_group_rows)
      d->nabla_grp_now = d->nabla_group_rows ? d->nabla_group_rows : 4;
      if (d->nabla_group_rows == 0 && d->h_nabla_kept && d->nabla_hint_possible > 0) {
        const unsigned long long kept = *(volatile unsigned long long*)d->h_nabla_kept;   // whatever has landed: no synchronisation
        if (kept > 0 && (double)kept < 0.5 * (double)d->nabla_hint_possible) d->nabla_grp_now = 2;
      }
      d->nabla_hint_pending = true;
      na = NablaArgs{Tp, Hp / 8, Wp / 8, a->nabla_wT, a->nabla_wH, a->nabla_wW, a->nabla_P};
    }
    const int P = d->sp_world;
    if (sp && P > 1 && !d->emulated && d->sp_autotune && !d->sp_tuned && !d->vblocks.empty()) K5CHK(sp_autotune_run(d, s, N, L, nabla ? &na : nullptr));
    if (sp) { const Shard sh = shard_layout(N, P, d->sp_slices, d->sp_rank); n = sh.n; n_pad = sh.n_pad; tok0 = sh.tok0; }
    auto& mg = d->mag;   // the one refusal that depends on the run: made here, with nothing enqueued (what decide() did to the accumulators stays)
    if (mg.on && (mag_skip = mg.decide()) && mg.res_elems[mg.slot()] != vis_elems()) {
      k5_set_error("magcache: skip decided but no cached residual of this shape for the slot");
      return K5_ERR_ARG;
    }
    auto& fc = d->fc;   // likewise: a forecast call needs the slot's history at this shard's shape
    if (fc.on && f.fc_step >= 0) {
      const int k = f.fc_slot;
      fc_kind = fc.full[f.fc_step] ? 1 : 2;
      if (fc_kind == 2 && (fc.have[k] == 0 || fc.elems[k] != vis_elems() || f.fc_step <= fc.j[k])) {
        k5_set_error("forecast: step %d of slot %d is a forecast call but the slot has %s", f.fc_step, k,
                     fc.have[k] == 0 ? "no full call yet" : fc.elems[k] != vis_elems() ? "a residual of another shape" : "no full call before this step");
        return K5_ERR_STATE;
      }
    }
    d->enh.live = d->enh.applies(Tp, d->cfg.num_visual_blocks);
    int Lmax = ncond && ncond->text_len > L ? ncond->text_len : L;   // every stream borrows the text blocks' scratch: size it by the longest
    for (int r = 0; r < Rg; ++r) Lmax = d->regions.conds[r].text_len > Lmax ? d->regions.conds[r].text_len : Lmax;
    K5CHK(sp ? ensure_sp_workspaces(d, n_pad, Lmax) : ensure_workspaces(d, N, Lmax));
    mod = d->ws_mod.as<float>();
    return K5_OK;
  }

  // ---- token order: NABLA's permutation, the Enhance-A-Video score's workspaces (under NABLA the token row of every (position, frame)), RoPE ----
  int token_order() {
    auto& en = d->enh;
    d->last_nabla = nabla;
    if (nabla) {
      K5CHK(token_table(d->ws_perm, d->perm_shape, Tp, Hp, Wp, [this](int32_t* v, int i, Tok k) { v[i] = (k.t * Hp + k.y) * Wp + k.x; }));
      perm = d->ws_perm.as<int32_t>();
    }
    if (en.live) {
      const int S = Hp * Wp;
      K5CHK(en.scores.ensure((size_t)d->cfg.num_visual_blocks * 4));
      K5CHK(en.part.ensure((size_t)k5_enhance_parts(d->Hh, S) * sizeof(double)));
      en.T = Tp; en.S = S; en.rows = nullptr;
      if (nabla) {
        K5CHK(token_table(en.frame_rows, en.rows_shape, Tp, Hp, Wp, [this](int32_t* v, int i, Tok k) { v[(size_t)(k.y * Wp + k.x) * Tp + k.t] = i; }));
        en.rows = en.frame_rows.as<int32_t>();
      }
      en.last_stream = s;
    }
    K5CHK(prepare_rope(d, s, a, Tp, Hp, Wp, perm));
    return prepare_text_rope(d, s, f.cond, &tcos, &tsin);
  }

  // ---- before_text_transformer_blocks (dit.py:129-137) ----
  int prologue() {
    Scope sc(d, s, "prologue");
    K5CHK(text_embeddings(d, s, f.cond, d->streams[0], f.cache_slot >= 0 ? &d->text_cache[f.cache_slot] : d->stream_cache(0, f.text_slot), true));
    K5CHK(k5_launch_time_features(f.time, d->ws_tfeat.as<float>(), D, s, f.tvec, f.step));
    K5CHK(k5_launch_gemv_f32(d->ws_tfeat.as<float>(), d->time_w1.as<float>(), d->time_b1.as<float>(), d->ws_th1.as<float>(),
                             d->TD, D, 0, nullptr, s));
    K5CHK(k5_launch_gemv_f32(d->ws_th1.as<float>(), d->time_w2.as<float>(), d->time_b2.as<float>(), d->ws_temb.as<float>(),
                             d->TD, d->TD, 1, d->ws_pool_f32.as<float>(), s));
    // every Modulation layer of the network in one GEMV (they all consume the same time_embed)
    K5CHK(k5_launch_gemv_f32(d->ws_temb.as<float>(), d->mod_w.as<float>(), d->mod_b.as<float>(), d->ws_mod.as<float>(),
                             (int)d->mod_rows, d->TD, 1, nullptr, s));
    if (f.x_row) K5CHK(k5_launch_patchify_view(f.x, f.x_frame, f.x_row, f.vcond, f.vc_frame, f.vc_row, d->ws_xp.p, a->T, a->H, a->W, f.x_channels, Cin,
                                               d->KvisPad, perm, s));
    else if (f.vcond) K5CHK(k5_launch_patchify_cond(f.x, f.vcond, d->ws_xp.p, a->T, a->H, a->W, f.x_channels, Cin, d->KvisPad, perm, s));
    else K5CHK(k5_launch_patchify(f.x, d->ws_xp.p, a->T, a->H, a->W, f.x_channels, Cin, d->KvisPad, perm, s));
    return linear(LinearArgs(d->vis_lin, Act{d->ws_xp.as<bf16_t>() + (size_t)tok0 * d->KvisPad, nullptr, n, d->KvisPad}, d->ws_vis.p, D, s));
  }

  // ---- MagCache and its calibration where the visual stream enters the blocks: a skipped call adds the slot's cached residual, a running one
  // keeps ori_visual_embed ----
  int residual_begin() {
    auto& mg = d->mag;
    if (mg.on && mag_skip) {
      Scope sc(d, s, "elementwise");   // visual_embed + residual (bf16 add), :78-79
      K5CHK(k5_launch_gate_sum(d->ws_vis.p, mg.residual[mg.slot()].p, mg.pm_one.as<float>(), d->ws_vis.p, n, D, s));
      mg.n_skipped++;
    } else if (mg.on) {
      K5CHK(mg.residual[mg.slot()].ensure(vis_elems() * 2));
      HIPCHK(hipMemcpyAsync(mg.residual[mg.slot()].p, d->ws_vis.p, vis_elems() * 2, hipMemcpyDeviceToDevice, s));  // ori_visual_embed
      mg.n_ran++;
    }
    auto& fc = d->fc;
    if (fc_kind == 2) {   // the extrapolated residual in place of the blocks
      Scope sc(d, s, "elementwise");
      const int k = f.fc_slot;
      K5CHK(k5_launch_forecast_apply(d->ws_vis.p, D, fc.F0[k].p, fc.D1[k].as<float>(), fc.D2[k].as<float>(), n, D, f.fc_step - fc.j[k], fc.gap[k],
                                     fc.gap_prev[k], fc.order, fc.have[k], s));
      fc.forecast_calls++; fc.last_stream = s;
    } else if (fc_kind == 1) {
      const int k = f.fc_slot;
      K5CHK(fc.ori.ensure(vis_elems() * 2)); K5CHK(fc.F0[k].ensure(vis_elems() * 2));
      if (fc.order >= 1) K5CHK(fc.D1[k].ensure(vis_elems() * 4));
      if (fc.order >= 2) K5CHK(fc.D2[k].ensure(vis_elems() * 4));
      HIPCHK(hipMemcpyAsync(fc.ori.p, d->ws_vis.p, vis_elems() * 2, hipMemcpyDeviceToDevice, s));  // the stream as it enters the blocks
    }
    auto& cl = d->cal;
    if (cl.on) {
      DevBuf& cur = cl.res[cl.slot()][cl.cur()];
      K5CHK(cur.ensure(vis_elems() * 2)); K5CHK(cl.part.ensure((size_t)k5_magcache_stats_blocks(n) * 4 * sizeof(double)));
      HIPCHK(hipMemcpyAsync(cur.p, d->ws_vis.p, vis_elems() * 2, hipMemcpyDeviceToDevice, s));  // ori_visual_embed
    }
    return K5_OK;
  }

  // ---- the forward's streams: the base prompt's cross-attention keys / V^T, then every other active prompt through the text side ----
  int text_streams() {
    auto& rg = d->regions;
    const int blocks = d->cfg.num_visual_blocks;
    cx_all = !no_blocks() && d->cross_kv_batched && blocks > 1 && d->cx_k.w.p;
    if (!no_blocks()) K5CHK(text_cross_kv(d, s, d->streams[0], cx_all));
    act[0] = {&f.cond, 0, d->ws_o.p};
    cx.n = 1; cx.kv_ready = cx_all;
    if (!no_blocks() && blocks > 0) {
      if (ncond) {
        K5CHK(d->nag.o.ensure(vis_elems() * 2));
        act[cx.n++] = {ncond, 1, d->nag.o.p};
        cx.nag = true;
      }
      if (Rg) K5CHK(rg.o.ensure((size_t)Rg * vis_elems() * 2));
      for (int r = 0; r < Rg; ++r) act[cx.n++] = {&rg.conds[r], 2 + r, rg.o.as<bf16_t>() + (size_t)r * vis_elems()};
      cx.R = Rg; cx.region_o_stride = (long long)vis_elems();
    }
    for (int k = 1; k < cx.n; ++k)
      K5CHK(text_stream_run(d, s, *act[k].cond, d->streams[act[k].stream], d->stream_cache(act[k].stream, f.text_slot), mod, cx_all));
    // the regions' token weights in this forward's token order (computed once per region set and order; a sequence-parallel rank reads its rows
    // from tok0 on)
    if (cx.R) {
      if (rg.w_order != (nabla ? 1 : 0)) {
        Scope sc(d, s, "elementwise");
        const int* ps = d->cfg.patch_size;
        K5CHK(rg.w.ensure((size_t)N * (Rg + 1) * 4));
        K5CHK(k5_launch_region_weights(rg.masks, Rg, rg.T, rg.H, rg.W, ps[0], ps[1], ps[2], rg.base_weight, perm, rg.w.as<float>(), s));
        rg.w_order = nabla ? 1 : 0;
      }
      cx.region_w = rg.w.as<float>() + (size_t)tok0 * (Rg + 1);
    }
    sched = sp ? sp_schedule(d, nabla) : 0;
    if (sp) d->sp_mode_used = sched;
    return K5_OK;
  }

  // one visual block on ws_vis.  pref_slot: the row of the softmax-form memory (0 cond, 1 uncond, 2 the skip branch); drop_sa: skip-layer
  // guidance mode 1, the block without its self-attention residual (its first LayerNorm goes with it)
  int block(int i, int pref_slot, bool drop_sa) {
    const BlockW& b = d->vblocks[i];
    const float* m = mod + b.mod_off;
    const float* vcos = d->ws_vcos.as<float>() + (size_t)tok0 * 32;
    const float* vsin = d->ws_vsin.as<float>() + (size_t)tok0 * 32;
    d->enh.block = i;   // the slot of this block's Enhance-A-Video score
    // fp8 modes: the LayerNorm writes the e4m3 rows the projections read (no bf16 h, no quantisation pass) — "fp8_fuse_ln" = 0 keeps the two passes
    const bool h8_sa = d->fp8_fuse_ln && sched == 0 && (sp ? sa_sp_fp8_in(d, b.self_attn, n, n_pad, nabla) : sa_fp8_in(d, b.self_attn, n));
    if (!drop_sa) {
      K5CHK(ln_mod(d, s, d->ws_vis.p, m, d->ws_h.p, n, h8_sa));
      if (d->profiling) ++d->prof_self_blocks;   // bench.py: FLOPs of the roofline kernel = per-block FLOPs x the blocks that RAN
      if (sched) {   // 1 Ulysses, 2 two-level
        K5CHK(run_self_attention_heads(d, s, b.self_attn, d->ws_h.p, n, n_pad, N, d->ws_o.p, vcos, vsin, d->ws_vis.p, m + 2 * D, sched == 2, pref_slot));
      } else if (sp) {
        K5CHK(run_self_attention_sp(d, s, b.self_attn, d->ws_h.p, n, n_pad, N, d->ws_o.p, vcos, vsin, d->ws_vis.p, m + 2 * D, nabla ? &na : nullptr, pref_slot, h8_sa));
      } else {
        K5CHK(run_self_attention(d, s, b.self_attn, d->ws_h.p, n, d->ws_qk.p, d->ws_vt.p, d->ws_o.p, vcos, vsin, d->ws_vis.p,
                                 m + 2 * D, "attn_self", nabla ? &na : nullptr, pref_slot, h8_sa));
      }
    }
    K5CHK(ln_mod(d, s, d->ws_vis.p, m + 3 * D, d->ws_h.p, n));
    for (int k = 0; k < cx.n; ++k) cx.v[k] = cross_view(d, d->streams[act[k].stream], i, cx_all, act[k].o);
    K5CHK(run_cross_attention(d, s, b.cross_attn, d->ws_h.p, n, d->ws_qk.p, cx, d->ws_vis.p, m + 5 * D));
    const bool h8_ff = d->fp8_fuse_ln && ff_fp8_in(d, b, n);
    K5CHK(ln_mod(d, s, d->ws_vis.p, m + 6 * D, d->ws_h.p, n, h8_ff));
    return run_ff(d, s, b, d->ws_h.p, n, d->ws_ff.p, d->ws_vis.p, m + 8 * D, h8_ff);
  }

  // ---- visual blocks (dit.py:176-178, 61-79).  The fork of skip-layer guidance: the visual stream as it enters block `fork_at` (the first skipped
  // one; 0 with "skip_share_prefix" = 0) is copied aside, skip_branch starts from it ----
  int visual_blocks() {
    auto& sk = d->skip;
    if (f.out_skip) {
      fork_at = sk.share_prefix ? sk.k0 : 0;
      K5CHK(sk.vis.ensure(vis_elems() * 2));
    }
    const int blocks = no_blocks() ? 0 : d->cfg.num_visual_blocks;
    for (int i = 0; i < blocks; ++i) {
      if (i == fork_at) HIPCHK(hipMemcpyAsync(sk.vis.p, d->ws_vis.p, vis_elems() * 2, hipMemcpyDeviceToDevice, s));
      K5CHK(block(i, f.text_slot > 0 ? 1 : 0, false));
    }
    if (d->enh.live && !no_blocks()) d->enh.last_blocks = blocks;
    return K5_OK;
  }

  // ---- MagCache and its calibration where the visual stream leaves the blocks ----
  int residual_end() {
    auto& mg = d->mag;
    if (mg.on) {
      if (!mag_skip) {  // residual = visual_embed - ori_visual_embed (bf16), :84
        Scope sc(d, s, "elementwise");
        K5CHK(k5_launch_gate_sum(d->ws_vis.p, mg.residual[mg.slot()].p, mg.pm_one.as<float>() + D, mg.residual[mg.slot()].p, n, D, s));
        mg.res_elems[mg.slot()] = vis_elems();
      }
      mg.advance();
    }
    auto& fc = d->fc;
    if (fc_kind == 1) {   // the residual and its finite differences against the slot's history; a step at or before j, or another shape, starts over
      Scope sc(d, s, "elementwise");
      const int k = f.fc_slot;
      if (f.fc_step <= fc.j[k] || fc.elems[k] != vis_elems()) fc.have[k] = 0;
      const int g = fc.have[k] ? f.fc_step - fc.j[k] : 1;
      K5CHK(k5_launch_forecast_update(d->ws_vis.p, D, fc.ori.p, fc.F0[k].p, fc.D1[k].as<float>(), fc.D2[k].as<float>(), n, D, g, fc.order, fc.have[k], s));
      fc.gap_prev[k] = fc.gap[k]; fc.gap[k] = g;
      fc.j[k] = f.fc_step; fc.elems[k] = vis_elems(); fc.last_stream = s;
      if (fc.have[k] < 3) fc.have[k]++;   // the rule reads have only up to 3 (m = min(order, have - 1))
      fc.full_calls++;
    }
    auto& cl = d->cal;
    if (cl.on) {   // the residual MagCache would cache, and its statistics against the slot's previous one (none on the slot's first call of a run)
      const int slot = cl.slot(), cur = cl.cur();
      {
        Scope sc(d, s, "elementwise");
        K5CHK(k5_launch_magcache_stats(d->ws_vis.p, cl.res[slot][cur].p, cl.cnt < 2 ? nullptr : cl.res[slot][cur ^ 1].p, cl.res[slot][cur].p,
                                       cl.table.as<double>() + (size_t)cl.cnt * 4, cl.part.as<double>(), 1, n, D, s));
      }
      cl.prev[slot] = cur; cl.res_elems[slot] = vis_elems(); cl.last_stream = s;
      cl.cnt += cl.no_cfg ? 2 : 1;
      if (cl.cnt >= 2 * cl.num_steps) { cl.cnt = 0; cl.runs++; }
    }
    return K5_OK;
  }

  // ---- after_blocks / OutLayer (dit.py:149-153, nn.py:374-400) ----
  int out_layer(void* out) {
    Scope sc(d, s, "epilogue");
    const float* m = mod + d->out_mod_off;  // [shift | scale]
    K5CHK(k5_launch_ln_modulate(d->ws_vis.p, m + D, m, d->ws_h.p, n, D, D, D, s));
    K5CHK(linear(LinearArgs(d->out_lin, Act{d->ws_h.p, nullptr, n, D}, d->ws_y.as<bf16_t>() + (size_t)tok0 * d->Fout, d->Fout, s)));
    // every rank needs the whole velocity: the (replicated) latent is advanced identically on all ranks
    if (sp) K5CHK(d->comm.all_gather_inplace(d->ws_y.p, (size_t)n_pad * d->Fout, 2, s));
    return k5_launch_unpatchify(d->ws_y.p, out, Tp, Hp, Wp, d->cfg.out_visual_dim, d->Fout, perm, s);
  }

  // ---- the skip branch: the same latent, prompt and time, so the text streams, the modulation vector and the stacked cross-attention K/V are
  // its own; it restores the visual stream of the fork and runs the blocks from there under the skip rule, on row 2 of the form memory ----
  int skip_branch() {
    auto& sk = d->skip;
    HIPCHK(hipMemcpyAsync(d->ws_vis.p, sk.vis.p, vis_elems() * 2, hipMemcpyDeviceToDevice, s));
    for (int i = fork_at; i < d->cfg.num_visual_blocks; ++i) {
      if (sk.skipped[i] && sk.mode == 0) continue;   // the identity: nothing is launched
      K5CHK(block(i, 2, sk.skipped[i] != 0));
      ++sk.blocks_run;
    }
    sk.blocks_shared += fork_at;
    return out_layer(f.out_skip);
  }
};

int forward_impl(k5_dit* d, const ForwardCall& f) {
  K5CHK(forward_refusals(d, f));
  ForwardRun r(d, f);
  K5CHK(r.shard());
  K5CHK(r.token_order());
  K5CHK(r.prologue());
  K5CHK(text_blocks_run(d, r.s, d->streams[0], r.tcos, r.tsin, r.mod));
  K5CHK(r.residual_begin());
  K5CHK(r.text_streams());
  K5CHK(r.visual_blocks());
  K5CHK(r.residual_end());
  K5CHK(r.out_layer(f.out));
  return f.out_skip ? r.skip_branch() : K5_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI: engine
// ---------------------------------------------------------------------------------------------
extern "C" int k5_dit_create(const k5_dit_config* cfg, k5_dit** out) {
  g_err[0] = 0;
  if (!cfg || !out) return K5_ERR_ARG;
  const int hd = cfg->axes_dims[0] + cfg->axes_dims[1] + cfg->axes_dims[2];
  if (hd != 64) { k5_set_error("head_dim = sum(axes_dims) must be 64 (got %d)", hd); return K5_ERR_UNSUPPORTED; }
  if (cfg->model_dim % 64 || cfg->model_dim % 8 || cfg->ff_dim % 8 || cfg->time_dim % 8 || cfg->in_text_dim % 8 ||
      cfg->in_text_dim2 % 8) {
    k5_set_error("model_dim %% 64, ff_dim/time_dim/in_text_dim(2) %% 8 must be 0"); return K5_ERR_UNSUPPORTED;
  }
  k5_dit* d = new k5_dit();
  d->cfg = *cfg;
  d->D = cfg->model_dim; d->FF = cfg->ff_dim; d->TD = cfg->time_dim; d->Hh = cfg->model_dim / 64;
  const int Cin = cfg->visual_cond ? 2 * cfg->in_visual_dim + 1 : cfg->in_visual_dim;
  d->Kvis = cfg->patch_size[0] * cfg->patch_size[1] * cfg->patch_size[2] * Cin;
  d->KvisPad = (int)rup(d->Kvis, 8);
  d->Fout = cfg->patch_size[0] * cfg->patch_size[1] * cfg->patch_size[2] * cfg->out_visual_dim;
  expected_keys(*cfg, d->expected);
  *out = d;
  return K5_OK;
}

extern "C" void k5_dit_destroy(k5_dit* d) {
  if (!d) return;
  // DevBufs are released with the process; explicit frees for long-lived hosts:
  DevBuf* all[] = {&d->time_w1, &d->time_b1, &d->time_w2, &d->time_b2, &d->text_lnw, &d->text_lnb, &d->pool_lnw, &d->pool_lnb, &d->mod_w,
                   &d->mod_b, &d->ws_text_in, &d->ws_th, &d->ws_tqk, &d->ws_tvt, &d->ws_to, &d->ws_tff,
                   &d->ws_pool_in, &d->ws_pool_lin, &d->ws_pool_f32, &d->ws_time, &d->ws_tfeat, &d->ws_th1, &d->ws_temb,
                   &d->ws_mod, &d->ws_xp, &d->ws_vis, &d->ws_h, &d->ws_qk, &d->ws_vt, &d->ws_o, &d->ws_ff,
                   &d->ws_y, &d->ws_vcos, &d->ws_vsin, &d->ws_pos, &d->ws_vel_c,
                   &d->ws_vel_u};
  for (DevBuf* b : all) b->release();
  for (auto& e : d->text_rope) { e.cosT.release(); e.sinT.release(); e.pos.release(); }
  d->ws_q.release(); d->ws_kfull.release(); d->ws_vtfull.release(); d->ws_attn_state.release(); d->ws_attn_bal.release(); d->ws_kc.release(); d->ws_kmeans.release(); d->ws_nabla_kept.release(); if (d->h_nabla_kept) { (void)hipHostFree(d->h_nabla_kept); d->h_nabla_kept = nullptr; } d->ws_sched.release(); d->ws_h8.release(); d->ws_ff8.release();
  d->ws_attn_stats.release(); d->ws_attn_flags.release(); d->ws_attn_cnt.release(); d->ws_attn_part.release(); d->ws_leave_sig.release();
  if (d->h_leave_sig) { (void)hipHostFree(d->h_leave_sig); d->h_leave_sig = nullptr; }
  for (auto& t : d->text_cache) { t.text.release(); t.pool.release(); }
  for (auto& st : d->streams) st.release();
  for (DevBuf* b : {&d->fe.zs, &d->fe.zt, &d->fe.vel_c, &d->fe.vel_u}) b->release();
  d->nag.o.release(); d->regions.o.release(); d->regions.w.release(); d->skip.vis.release(); d->skip.vel.release();
  for (auto& kv : d->staged) kv.second.dev.release();   // a handle destroyed before finalize still holds its staged matrices
  d->mag.residual[0].release(); d->mag.residual[1].release(); d->mag.pm_one.release();
  if (d->graph_stream) { (void)hipStreamSynchronize(d->graph_stream); (void)hipStreamDestroy(d->graph_stream); (void)hipEventDestroy(d->ev_graph); }
  if (d->comm_stream) { (void)hipStreamSynchronize(d->comm_stream); (void)hipStreamDestroy(d->comm_stream); }
  for (hipEvent_t e : {d->ev_k, d->ev_v, d->ev_gathered, d->ev_stats, d->ev_means, d->ev_slice[0], d->ev_slice[1], d->ev_slice[2], d->ev_slice[3]}) if (e) (void)hipEventDestroy(e); d->ws_perm.release(); d->ws_nabla.release();
  if (d->comm.comm) (void)d->comm.CommDestroy(d->comm.comm);
  for (Comm* c : {&d->comm, &d->pair}) if (c->ipc) { c->ipc->close_all(); delete c->ipc; c->ipc = nullptr; }
  if (d->pair_stream) { (void)hipStreamSynchronize(d->pair_stream); (void)hipStreamDestroy(d->pair_stream); }
  for (hipEvent_t e : {d->ev_vel_ready, d->ev_vel_done, d->ev_u_o, d->ev_u_back}) if (e) (void)hipEventDestroy(e);
  if (d->pair.comm) (void)d->pair.CommDestroy(d->pair.comm);
  d->ws_vel_pair.release(); d->ws_win.release();
  d->watch.wb.release();
  for (int i = 0; i < 2; ++i) {
    d->watch.rgb[i].release(); d->watch.x0[i].release();
    if (d->watch.h_rgb[i]) (void)hipHostFree(d->watch.h_rgb[i]);
    if (d->watch.ev[i]) (void)hipEventDestroy(d->watch.ev[i]);
  }
  delete d;   // the layers (Linear) and everything else a DevBuf holds go with the handle
}

extern "C" int k5_dit_load_tensor(k5_dit* d, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int rank) {
  g_err[0] = 0;
  if (!d || !key || !host_ptr || rank < 1 || rank > 2) return K5_ERR_ARG;
  if (d->finalized) { k5_set_error("load_tensor after finalize"); return K5_ERR_STATE; }
  bool known = false;
  for (auto& e : d->expected) if (e == key) { known = true; break; }
  if (!known) { k5_set_error("unexpected key in state_dict: %s", key); return K5_ERR_KEY; }
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < rank; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
  if (dtype != K5_F32 && dtype != K5_BF16 && dtype != K5_F16) return K5_ERR_ARG;
  if (rank == 2) {   // a matrix: raw copy to the device (D2D for a checkpoint that is already there), packed by k5_dit_finalize
    const size_t bytes = n * (dtype == K5_F32 ? 4 : 2);
    t.dtype = dtype;
    K5CHK(t.dev.ensure(bytes));
    HIPCHK(hipMemcpy(t.dev.p, host_ptr, bytes, hipMemcpyDefault));
    d->staged[key] = std::move(t);
    return K5_OK;
  }
  t.data.resize(n);
  // hipMemcpyDefault: the source may be host memory (safetensors on CPU) or device memory
  if (dtype == K5_F32) HIPCHK(hipMemcpy(t.data.data(), host_ptr, n * 4, hipMemcpyDefault));
  else if (dtype == K5_BF16 || dtype == K5_F16) {
    std::vector<uint16_t> raw(n);
    HIPCHK(hipMemcpy(raw.data(), host_ptr, n * 2, hipMemcpyDefault));
    if (dtype == K5_BF16)
      for (size_t i = 0; i < n; ++i) { uint32_t u = (uint32_t)raw[i] << 16; memcpy(&t.data[i], &u, 4); }
    else
      for (size_t i = 0; i < n; ++i) t.data[i] = half_to_float(raw[i]);
  } else return K5_ERR_ARG;
  d->staged[key] = std::move(t);
  return K5_OK;
}

extern "C" int k5_dit_missing_keys(k5_dit* d) {
  if (!d) return -1;
  int miss = 0; std::string names;
  for (auto& e : d->expected)
    if (!d->staged.count(e)) { if (miss < 8) names += e + " "; ++miss; }
  if (miss) k5_set_error("missing %d key(s): %s", miss, names.c_str());
  return d->finalized ? 0 : miss;
}

extern "C" int k5_dit_finalize(k5_dit* d) {
  g_err[0] = 0;
  if (!d) return K5_ERR_ARG;
  if (d->finalized) return K5_OK;
  if (k5_dit_missing_keys(d)) return K5_ERR_KEY;
  const k5_dit_config& c = d->cfg;
  const size_t D = d->D, FF = d->FF, TD = d->TD;
  if (!shape_ok(d, "time_embeddings.in_layer.weight", TD, D) || !shape_ok(d, "time_embeddings.out_layer.weight", TD, TD) ||
      !shape_ok(d, "out_layer.modulation.out_layer.weight", 2 * D, TD) ||
      !shape_ok(d, "time_embeddings.in_layer.bias", TD, 0) || !shape_ok(d, "time_embeddings.out_layer.bias", TD, 0) ||
      !shape_ok(d, "text_embeddings.norm.weight", D, 0) || !shape_ok(d, "text_embeddings.norm.bias", D, 0) ||
      !shape_ok(d, "pooled_text_embeddings.norm.weight", TD, 0) || !shape_ok(d, "pooled_text_embeddings.norm.bias", TD, 0))
    return K5_ERR_ARG;
  K5CHK(pack_f32(d->time_w1, find(d, "time_embeddings.in_layer.weight"), TD, D));
  K5CHK(upload_f32(d->time_b1, find(d, "time_embeddings.in_layer.bias")->data.data(), TD));
  K5CHK(pack_f32(d->time_w2, find(d, "time_embeddings.out_layer.weight"), TD, TD));
  K5CHK(upload_f32(d->time_b2, find(d, "time_embeddings.out_layer.bias")->data.data(), TD));
  K5CHK(load_linear(d, d->text_lin, {"text_embeddings.in_layer"}, D, c.in_text_dim, c.in_text_dim));
  K5CHK(upload_f32(d->text_lnw, find(d, "text_embeddings.norm.weight")->data.data(), D));
  K5CHK(upload_f32(d->text_lnb, find(d, "text_embeddings.norm.bias")->data.data(), D));
  K5CHK(load_linear(d, d->pool_lin, {"pooled_text_embeddings.in_layer"}, TD, c.in_text_dim2, c.in_text_dim2));
  K5CHK(upload_f32(d->pool_lnw, find(d, "pooled_text_embeddings.norm.weight")->data.data(), TD));
  K5CHK(upload_f32(d->pool_lnb, find(d, "pooled_text_embeddings.norm.bias")->data.data(), TD));
  K5CHK(load_linear(d, d->vis_lin, {"visual_embeddings.in_layer"}, D, d->Kvis, d->KvisPad));
  K5CHK(load_linear(d, d->out_lin, {"out_layer.out_layer"}, d->Fout, D, D));

  // stacked modulation
  d->mod_rows = (size_t)c.num_text_blocks * 6 * D + (size_t)c.num_visual_blocks * 9 * D + 2 * D;
  std::vector<float> mb(d->mod_rows);
  size_t off = 0;
  auto put_mod = [&](const std::string& p, size_t rows) -> bool {
    const HostTensor *w = find(d, p + ".weight"), *b = find(d, p + ".bias");
    if (!w || !b || w->shape.size() != 2 || w->count() != rows * TD || b->data.size() != rows) { k5_set_error("shape mismatch for %s", p.c_str()); return false; }
    if (pack_f32(d->mod_w, w, rows, TD, off, d->mod_rows) != K5_OK) return false;
    memcpy(mb.data() + off, b->data.data(), rows * 4);
    off += rows;
    return true;
  };
  d->tblocks.resize(c.num_text_blocks); d->vblocks.resize(c.num_visual_blocks);
  for (int i = 0; i < c.num_text_blocks; ++i) {
    const std::string p = "text_transformer_blocks." + std::to_string(i);
    d->tblocks[i].mod_off = off;
    if (!put_mod(p + ".text_modulation.out_layer", 6 * D)) return K5_ERR_ARG;
    K5CHK(pack_attn(d, p + ".self_attention", d->tblocks[i].self_attn, true));
    K5CHK(load_linear(d, d->tblocks[i].w1, {p + ".feed_forward.in_layer"}, FF, D, D, false));
    K5CHK(load_linear(d, d->tblocks[i].w2, {p + ".feed_forward.out_layer"}, D, FF, FF, false));
  }
  for (int i = 0; i < c.num_visual_blocks; ++i) {
    const std::string p = "visual_transformer_blocks." + std::to_string(i);
    d->vblocks[i].mod_off = off;
    if (!put_mod(p + ".visual_modulation.out_layer", 9 * D)) return K5_ERR_ARG;
    K5CHK(pack_attn(d, p + ".self_attention", d->vblocks[i].self_attn, true));
    K5CHK(pack_attn(d, p + ".cross_attention", d->vblocks[i].cross_attn, false));
    K5CHK(load_linear(d, d->vblocks[i].w1, {p + ".feed_forward.in_layer"}, FF, D, D, false));
    K5CHK(load_linear(d, d->vblocks[i].w2, {p + ".feed_forward.out_layer"}, D, FF, FF, false));
  }
  // The cross-attention key / value layers of all visual blocks are packed once, stacked (4 nbv D^2 bytes, 411 MB on 2B-Lite, not
  // held twice); a block's own wk / wv are views of its rows, so the per-block path ("cross_kv_batched" = 0) reads the same memory
  if (const size_t nbv = (size_t)c.num_visual_blocks) {
    std::vector<std::string> pk, pv;
    for (size_t i = 0; i < nbv; ++i) {
      const std::string p = "visual_transformer_blocks." + std::to_string(i) + ".cross_attention";
      pk.push_back(p + ".to_key"); pv.push_back(p + ".to_value");
    }
    K5CHK(load_linear(d, d->cx_k, pk, D, D, D)); K5CHK(load_linear(d, d->cx_v, pv, D, D, D));
    K5CHK(d->cx_knorm_all.ensure(nbv * 64 * 4));
    for (size_t i = 0; i < nbv; ++i) {
      AttnW& a = d->vblocks[i].cross_attn;
      HIPCHK(hipMemcpy((char*)d->cx_knorm_all.p + i * 64 * 4, a.norm.as<float>() + 64, 64 * 4, hipMemcpyDeviceToDevice));
      a.wk = d->cx_k.rows(i * D, D); a.wv = d->cx_v.rows(i * D, D);
    }
  }
  d->out_mod_off = off;
  if (!put_mod("out_layer.modulation.out_layer", 2 * D)) return K5_ERR_ARG;
  K5CHK(upload_f32(d->mod_b, mb.data(), mb.size()));
  HIPCHK(hipDeviceSynchronize());   // the pack kernels read the staged device copies that are freed next
  for (auto& kv : d->staged) kv.second.dev.release();
  d->staged.clear();
  // the NABLA density hint's device counter and pinned host copy exist before any forward (no allocation inside a stream capture)
  K5CHK(d->ws_nabla_kept.ensure(8));
  if (!d->h_nabla_kept) { HIPCHK(hipHostMalloc((void**)&d->h_nabla_kept, 8, hipHostMallocDefault)); *d->h_nabla_kept = 0ull; }
  d->finalized = true;
  return K5_OK;
}

extern "C" int k5_dit_set_magcache(k5_dit* d, const double* ratio_table, int table_len, int no_cfg, double thresh, int K,
                                   double retention_ratio) {
  if (!d || !d->finalized) { k5_set_error("k5_dit_set_magcache: handle not finalized"); return K5_ERR_STATE; }
  if (table_len > 0 && d->cal.on) { k5_set_error("k5_dit_set_magcache: the handle is calibrating (k5_dit_set_magcache_calibrate)"); return K5_ERR_STATE; }
  if (table_len > 0 && d->fc.on) { k5_set_error("k5_dit_set_magcache: a forecast plan is set on the handle (k5_dit_set_forecast)"); return K5_ERR_STATE; }
  auto& mg = d->mag;
  mg.cnt = 0; mg.n_ran = mg.n_skipped = 0;
  mg.reset_acc(); mg.res_elems[0] = mg.res_elems[1] = 0;
  if (table_len <= 0) { mg.on = false; mg.table.clear(); return K5_OK; }
  if (!ratio_table || (table_len & 1) || K < 0) { k5_set_error("k5_dit_set_magcache: table of 2*num_steps ratios expected"); return K5_ERR_ARG; }
  mg.table.assign(ratio_table, ratio_table + table_len);
  mg.no_cfg = no_cfg != 0; mg.thresh = thresh; mg.K = K; mg.retention = retention_ratio;
  mg.first = 0; mg.stride = mg.no_cfg ? 2 : 1;
  std::vector<float> pm(2 * (size_t)d->D);
  for (int i = 0; i < d->D; ++i) { pm[i] = 1.f; pm[d->D + i] = -1.f; }
  K5CHK(mg.pm_one.ensure(pm.size() * 4));
  HIPCHK(hipMemcpy(mg.pm_one.p, pm.data(), pm.size() * 4, hipMemcpyHostToDevice));
  mg.on = true;
  return K5_OK;
}

extern "C" int k5_dit_magcache_calls(k5_dit* d, int first_call, int stride) {
  if (!d || !d->mag.on) { k5_set_error("k5_dit_magcache_calls: MagCache is not enabled on this handle"); return K5_ERR_STATE; }
  if (first_call < 0 || stride < 1 || first_call >= stride) { k5_set_error("k5_dit_magcache_calls: need 0 <= first < stride"); return K5_ERR_ARG; }
  d->mag.first = d->mag.cnt = first_call; d->mag.stride = stride;
  return K5_OK;
}

extern "C" int k5_dit_magcache_state(k5_dit* d, int* cnt, long long* n_ran, long long* n_skipped) {
  if (!d) { k5_set_error("k5_dit_magcache_state: null handle"); return K5_ERR_ARG; }
  if (cnt) *cnt = d->mag.cnt;
  if (n_ran) *n_ran = d->mag.n_ran;
  if (n_skipped) *n_skipped = d->mag.n_skipped;
  return K5_OK;
}

extern "C" int k5_dit_set_magcache_calibrate(k5_dit* d, int num_steps, int no_cfg) {
  g_err[0] = 0;
  if (!d || !d->finalized) { k5_set_error("k5_dit_set_magcache_calibrate: handle not finalized"); return K5_ERR_STATE; }
  if (num_steps < 0) { k5_set_error("k5_dit_set_magcache_calibrate: num_steps must be >= 0 (got %d)", num_steps); return K5_ERR_ARG; }
  auto& cl = d->cal;
  if (num_steps > 0) {
    if (d->mag.on) { k5_set_error("k5_dit_set_magcache_calibrate: MagCache is set on the handle"); return K5_ERR_STATE; }
    if (d->fc.on) { k5_set_error("k5_dit_set_magcache_calibrate: a forecast plan is set on the handle (k5_dit_set_forecast)"); return K5_ERR_STATE; }
    if (d->comm.active()) { k5_set_error("k5_dit_set_magcache_calibrate: the handle is in a sequence-parallel group (calibration is a one-GPU job)"); return K5_ERR_STATE; }
    if (d->pair.active()) { k5_set_error("k5_dit_set_magcache_calibrate: the handle is in a CFG pair (calibration is a one-GPU job)"); return K5_ERR_STATE; }
  }
  if (cl.on && cl.last_stream) HIPCHK(hipStreamSynchronize(cl.last_stream));   // the buffers freed below may still be read
  for (int j = 0; j < 2; ++j) { cl.res[j][0].release(); cl.res[j][1].release(); cl.prev[j] = 0; cl.res_elems[j] = 0; }
  cl.table.release(); cl.part.release();
  cl.on = false; cl.cnt = 0; cl.runs = 0; cl.num_steps = 0; cl.no_cfg = false; cl.last_stream = nullptr;
  if (num_steps == 0) return K5_OK;
  const size_t bytes = (size_t)2 * num_steps * 4 * sizeof(double);
  K5CHK(cl.table.ensure(bytes));
  HIPCHK(hipMemset(cl.table.p, 0, bytes));
  cl.num_steps = num_steps; cl.no_cfg = no_cfg != 0; cl.on = true;
  return K5_OK;
}

extern "C" int k5_dit_magcache_calibration(k5_dit* d, double* out, int cap_rows, int* rows, long long* runs) {
  g_err[0] = 0;
  if (!d || !d->cal.on) { k5_set_error("k5_dit_magcache_calibration: calibration is not on (k5_dit_set_magcache_calibrate)"); return K5_ERR_STATE; }
  auto& cl = d->cal;
  if (out && cap_rows < 0) { k5_set_error("k5_dit_magcache_calibration: cap_rows must be >= 0"); return K5_ERR_ARG; }
  if (cl.last_stream) HIPCHK(hipStreamSynchronize(cl.last_stream));
  const int nrows = 2 * cl.num_steps;
  if (out) {
    const int take = cap_rows < nrows ? cap_rows : nrows;
    if (take > 0) HIPCHK(hipMemcpy(out, cl.table.p, (size_t)take * 4 * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (rows) *rows = nrows;
  if (runs) *runs = cl.runs;
  return K5_OK;
}

extern "C" int k5_dit_set_forecast(k5_dit* d, const k5_forecast* p) {
  g_err[0] = 0;
  if (!d || !d->finalized) { k5_set_error("k5_dit_set_forecast: handle not finalized"); return K5_ERR_STATE; }
  auto& fc = d->fc;
  if (p) {   // every refusal before the handle is touched
    if (p->num_steps < 1 || !p->full) { k5_set_error("k5_dit_set_forecast: full with num_steps = %d", p->num_steps); return K5_ERR_ARG; }
    if (p->order < 0 || p->order > 2) { k5_set_error("k5_dit_set_forecast: order must be 0, 1 or 2 (got %d)", p->order); return K5_ERR_ARG; }
    if (!p->full[0]) { k5_set_error("k5_dit_set_forecast: full[0] must be 1: the first step has nothing to extrapolate from"); return K5_ERR_ARG; }
    if (const char* mode = magcache_mode(d)) { k5_set_error("k5_dit_set_forecast: %s on the handle", mode); return K5_ERR_STATE; }
  }
  if (fc.last_stream) HIPCHK(hipStreamSynchronize(fc.last_stream));   // the buffers freed below may still be read
  fc.last_stream = nullptr;
  for (int k = 0; k < 2; ++k) { fc.F0[k].release(); fc.D1[k].release(); fc.D2[k].release(); fc.elems[k] = 0; }
  fc.ori.release();
  fc.clear_history();   // (the call counts stay: k5_dit_forecast_state resets them)
  fc.on = fc.mixed = false; fc.full.clear();
  if (!p) return K5_OK;
  fc.full.resize((size_t)p->num_steps);
  for (int i = 0; i < p->num_steps; ++i) { fc.full[i] = p->full[i] ? 1 : 0; fc.mixed = fc.mixed || !p->full[i]; }
  fc.order = p->order; fc.on = true;
  return K5_OK;
}

extern "C" int k5_dit_forecast_at(k5_dit* d, int step, int slot) {
  g_err[0] = 0;
  if (!d || !d->fc.on) { k5_set_error("k5_dit_forecast_at: no forecast plan on the handle (k5_dit_set_forecast)"); return K5_ERR_STATE; }
  if (step < 0 || step >= (int)d->fc.full.size()) { k5_set_error("k5_dit_forecast_at: step %d is outside 0..%d", step, (int)d->fc.full.size() - 1); return K5_ERR_ARG; }
  if (slot != 0 && slot != 1) { k5_set_error("k5_dit_forecast_at: slot must be 0 (conditional) or 1 (unconditional), got %d", slot); return K5_ERR_ARG; }
  d->fc.at_step = step; d->fc.at_slot = slot;
  return K5_OK;
}

extern "C" int k5_dit_forecast_state(k5_dit* d, int* on, long long* full_calls, long long* forecast_calls, long long* state_bytes, int reset) {
  if (!d) { k5_set_error("k5_dit_forecast_state: null handle"); return K5_ERR_ARG; }
  if (on) *on = d->fc.on ? 1 : 0;
  if (full_calls) *full_calls = d->fc.full_calls;
  if (forecast_calls) *forecast_calls = d->fc.forecast_calls;
  if (state_bytes) *state_bytes = d->fc.state_bytes();
  if (reset) d->fc.full_calls = d->fc.forecast_calls = 0;
  return K5_OK;
}

extern "C" int k5_dit_forward(k5_dit* d, const k5_forward_args* a, void* out_velocity, void* stream) {
  g_err[0] = 0;
  if (!d || !a || !out_velocity || !a->x) return K5_ERR_ARG;
  ForwardCall f{a, a->cond, a->time, a->x, a->x_channels, out_velocity, (hipStream_t)stream};
  if (d->fc.on && d->fc.at_step >= 0) { f.fc_step = d->fc.at_step; f.fc_slot = d->fc.at_slot; d->fc.at_step = -1; }   // one forward consumes the cursor
  return forward_impl(d, f);
}

// "sequence-parallel group" or "CFG pair": the rank group the handle is in (nullptr: none), for the refusals of what is single-rank only
static const char* rank_group(const k5_dit* d) {
  return d->comm.active() ? "sequence-parallel group" : d->pair.active() ? "CFG pair" : nullptr;
}

// The latent of an editing mode (`mode`: "edit" / "FlowEdit") is output only: it is 4-byte aligned, and so is every borrowed input, none of
// which overlaps it
struct Borrowed { const float* p; int64_t elems; const char* name; };
static int borrowed_refusal(const char* who, const char* mode, const float* latent, int64_t n, std::initializer_list<Borrowed> in) {
  const uintptr_t l0 = reinterpret_cast<uintptr_t>(latent), l1 = l0 + (uintptr_t)n * 4;
  if (l0 & 3) { k5_set_error("%s: latent is not 4-byte aligned", who); return K5_ERR_ARG; }
  for (const auto& t : in) {
    if (!t.p) continue;
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(t.p), p1 = p0 + (uintptr_t)t.elems * 4;
    if (p0 & 3) { k5_set_error("%s: %s %s is not 4-byte aligned", who, mode, t.name); return K5_ERR_ARG; }
    if (p0 < l1 && l0 < p1) { k5_set_error("%s: %s %s overlaps latent (latent is output only)", who, mode, t.name); return K5_ERR_ARG; }
  }
  return K5_OK;
}

// Everything sample_impl refuses, before anything is enqueued or allocated and before any per-call state is touched: no HIP call and no
// write to the handle here (the forward's side of the same contract: forward_refusals).  (A watched call's shape check comes later, where it always was: Watch::begin.)
// `tile`: the window plan of k5_sample_tiles / k5_sample_windows (nullptr: a plain run).  A temporal plan is a 3-D plan with one row window and
// one column window, so it meets the 3-D checks: among them "rows and columns must be even", which refuses a temporal plan on an odd latent
// here, before anything is enqueued, and not inside its first forward.
static int sample_refusals(const k5_dit* d, const k5_sample_args* a, const float* vcond, const k5_edit_args* edit,
                           const k5_sample_tiles_args* tile, const char* who, const k5_flowedit_args* fe = nullptr) {
  if (!d || !a || !a->latent || !a->sigmas || a->num_steps <= 0) return K5_ERR_ARG;
  const k5_dit_config& c = d->cfg;
  const char* const mag = magcache_mode(d);
  if (vcond && !c.visual_cond) { k5_set_error("%s: the handle was created with visual_cond = 0", who); return K5_ERR_ARG; }
  if (vcond && (reinterpret_cast<uintptr_t>(vcond) & 3)) { k5_set_error("%s: visual_cond is not 4-byte aligned", who); return K5_ERR_ARG; }
  const int64_t n = (int64_t)a->fwd.T * a->fwd.H * a->fwd.W * c.out_visual_dim;
  if (c.in_visual_dim != c.out_visual_dim) return K5_ERR_UNSUPPORTED;
  if (edit) {   // the latent is output only and must not be one of the borrowed inputs
    if (!edit->source || !edit->noise) { k5_set_error("%s: edit needs source and noise", who); return K5_ERR_ARG; }
    if (n <= 0) { k5_set_error("%s: bad shapes", who); return K5_ERR_ARG; }
    K5CHK(borrowed_refusal(who, "edit", a->latent, n, {{edit->source, n, "source"}, {edit->noise, n, "noise"},
                                                       {edit->keep_mask, n / c.out_visual_dim, "keep_mask"}}));
  }
  if (fe) {   // FlowEdit: every forward and update of a step is this mode's own, so what changes either is refused, not half honoured
    if (!fe->source || !fe->source_cond.text_embed) { k5_set_error("%s: FlowEdit needs a source latent and a source prompt", who); return K5_ERR_ARG; }
    if (n <= 0) { k5_set_error("%s: bad shapes", who); return K5_ERR_ARG; }
    if (fe->refine < 0 || fe->refine > a->num_steps) {
      k5_set_error("%s: refine must be in 0..num_steps (got %d of %d)", who, fe->refine, a->num_steps);
      return K5_ERR_ARG;
    }
    if (fe->refine > 0 && fe->keep_mask) {
      k5_set_error("%s: refine = %d with a keep_mask: the keep rule of a plain step needs an eps this mode does not have", who, fe->refine);
      return K5_ERR_ARG;
    }
    K5CHK(borrowed_refusal(who, "FlowEdit", a->latent, n, {{fe->source, n, "source"}, {fe->keep_mask, n / c.out_visual_dim, "keep_mask"},
                                                           {vcond, n / c.out_visual_dim * (c.in_visual_dim + 1), "visual_cond"}}));
    if (rank_group(d)) {
      k5_set_error("%s: the handle is in a %s: the forwards of a FlowEdit step are not split over ranks", who, rank_group(d));
      return K5_ERR_STATE;
    }
    if (mag) { k5_set_error("%s: %s on the handle: the ratio table is indexed by the calls of a plain run", who, mag); return K5_ERR_STATE; }
    const char* why = d->fc.on && d->fc.mixed ? "a forecast plan with forecast steps is set (k5_dit_set_forecast): the cache holds two slots, a step has four forwards"
                      : d->skip.live() ? "skip-layer guidance is set (k5_dit_set_skip_guidance): the update has no skip term"
                      : d->guide.on ? "a guidance plan is set (k5_dit_set_guidance): one plan, two guided sides"
                      : d->sto.on ? "a stochastic plan is set (k5_dit_set_stochastic): FlowEdit draws its own noise"
                      : d->nag.on ? "normalized attention guidance is set (k5_dit_set_nag): two conditional forwards, whose is it?"
                      : d->regions.on ? "regional prompts are set (k5_dit_set_regions): two conditional forwards, whose are they?"
                      : d->watch.on && d->watch.every > 0 ? "the watch has previews: z_fe is not on the model's path, x0 = x - sigma v does not hold; install the watch with preview_every = 0"
                      : nullptr;
    if (why) { k5_set_error("%s: %s", who, why); return K5_ERR_STATE; }
  }
  const k5_dit::Watch& wt = d->watch;
  if (wt.on && rank_group(d)) {
    k5_set_error("%s: a watch is installed (k5_dit_set_watch) and the handle is in a %s: a rank that stops alone would leave its peers inside a "
                 "collective", who, rank_group(d));
    return K5_ERR_STATE;
  }
  const k5_dit::Regions& rg = d->regions;
  if (rg.on && tile) {
    k5_set_error("%s: regional prompts are set (k5_dit_set_regions): the masks cover the clip, a context window sees a slice of it", who);
    return K5_ERR_STATE;
  }
  if (rg.on && (a->fwd.T != rg.T || a->fwd.H != rg.H || a->fwd.W != rg.W)) {
    k5_set_error("%s: regional prompts: the masks are (%d, %d, %d), this sample is (%d, %d, %d)", who, rg.T, rg.H, rg.W, a->fwd.T, a->fwd.H, a->fwd.W);
    return K5_ERR_ARG;
  }
  const k5_dit::Guidance& gd = d->guide;
  int guided = 0, unguided = 0;   // the steps of the guidance plan, by kind
  if (gd.on) {
    const int N = a->num_steps;
    if (!gd.weights.empty() && (int)gd.weights.size() != N) {
      k5_set_error("%s: the guidance plan has %d weights, this call %d steps", who, (int)gd.weights.size(), N);
      return K5_ERR_ARG;
    }
    for (int i = 0; i < N; ++i) (fabsf((gd.weights.empty() ? a->guidance_weight : gd.weights[i]) - 1.0f) > 1e-6f ? guided : unguided) += 1;
    const bool mixed = guided && unguided, zinit = gd.zero_init > 0;
    const char* what = zinit ? "zero-init steps" : "guided and unguided steps";
    if (tile) {
      k5_set_error("%s: a guidance plan is set (k5_dit_set_guidance): one statistic per window is not the published rule", who);
      return K5_ERR_STATE;
    }
    if (gd.stats() && !guided) {
      k5_set_error("%s: the guidance plan has %s but every weight of this call is 1: there is nothing to guide", who,
                   gd.zero_star ? "zero_star" : "rescale");
      return K5_ERR_ARG;
    }
    if ((mixed || zinit) && d->pair.active()) {
      k5_set_error("%s: the guidance plan has %s and the handle is in a CFG pair: the unconditional group would have steps with nothing to exchange",
                   who, what);
      return K5_ERR_STATE;
    }
    if ((mixed || zinit) && mag) {
      k5_set_error("%s: the guidance plan has %s and %s on the handle: the ratio table is indexed by the call of a plain run", who, what, mag);
      return K5_ERR_STATE;
    }
    if (zinit && edit) { k5_set_error("%s: zero-init steps together with editing are not supported", who); return K5_ERR_UNSUPPORTED; }
    if (gd.stats() && (n < 1 || (n & 7))) { k5_set_error("%s: zero_star / rescale need a latent of a multiple of 8 elements (got %lld)", who, (long long)n); return K5_ERR_ALIGN; }
  }
  const k5_dit::Skip& sg = d->skip;
  if (sg.live()) {
    if (!sg.steps.empty() && (int)sg.steps.size() != a->num_steps) {
      k5_set_error("%s: the skip-guidance mask has %d steps, this call %d", who, (int)sg.steps.size(), a->num_steps);
      return K5_ERR_ARG;
    }
    if (d->pair.active()) {
      k5_set_error("%s: skip-layer guidance is set (k5_dit_set_skip_guidance) and the handle is in a CFG pair: the pair exchanges two velocities, a skip step has three", who);
      return K5_ERR_STATE;
    }
    if (mag) {
      k5_set_error("%s: skip-layer guidance is set (k5_dit_set_skip_guidance) and %s on the handle: the ratio table is indexed by the calls of a plain run",
                   who, mag);
      return K5_ERR_STATE;
    }
    if (tile) {
      k5_set_error("%s: skip-layer guidance is set (k5_dit_set_skip_guidance): a windowed step has one velocity pair per window, the skip branch is not built for it", who);
      return K5_ERR_STATE;
    }
  }
  const k5_dit::Forecast& fc = d->fc;
  if (fc.on) {
    if ((int)fc.full.size() != a->num_steps) {
      k5_set_error("%s: the forecast plan has %d steps, this call %d", who, (int)fc.full.size(), a->num_steps);
      return K5_ERR_ARG;
    }
    if (sg.live()) {
      k5_set_error("%s: a forecast plan is set (k5_dit_set_forecast) and skip-layer guidance (k5_dit_set_skip_guidance): the skip branch has no slot", who);
      return K5_ERR_STATE;
    }
    if (gd.on && ((guided && unguided) || gd.zero_init > 0)) {
      k5_set_error("%s: a forecast plan is set (k5_dit_set_forecast) and the guidance plan has %s: the unconditional slot would have gaps", who,
                   gd.zero_init > 0 ? "zero-init steps" : "guided and unguided steps");
      return K5_ERR_STATE;
    }
    if (tile) {
      k5_set_error("%s: a forecast plan is set (k5_dit_set_forecast): a windowed step makes nwin calls per slot, the cache holds one residual per slot", who);
      return K5_ERR_STATE;
    }
    if (d->pair.active()) {
      k5_set_error("%s: a forecast plan is set (k5_dit_set_forecast) and the handle is in a CFG pair: not built", who);
      return K5_ERR_STATE;
    }
  }
  const k5_dit::Enhance& en = d->enh;
  if (en.on) {
    if (!en.steps.empty() && (int)en.steps.size() != a->num_steps) {
      k5_set_error("%s: the Enhance-A-Video mask has %d steps, this call %d", who, (int)en.steps.size(), a->num_steps);
      return K5_ERR_ARG;
    }
    if (d->comm.active()) {
      k5_set_error("%s: Enhance-A-Video is set (k5_dit_set_enhance) and the handle is in a sequence-parallel group: the frames of a column live on "
                   "different ranks, the cross-rank reduction is not built", who);
      return K5_ERR_STATE;
    }
    if (a->fwd.T > 64) {
      k5_set_error("%s: Enhance-A-Video is set (k5_dit_set_enhance): %d frames per forward are more than a wave's four 32 x 32 accumulators hold (64)",
                   who, a->fwd.T);
      return K5_ERR_UNSUPPORTED;
    }
  }
  const k5_dit::Stochastic& so = d->sto;
  if (so.on) {
    if ((int)so.dt_down.size() != a->num_steps) {
      k5_set_error("%s: the stochastic plan has %d steps, this call %d", who, (int)so.dt_down.size(), a->num_steps);
      return K5_ERR_ARG;
    }
    if (tile) {
      k5_set_error("%s: a stochastic plan is set (k5_dit_set_stochastic): the windowed update blends one velocity pair per window and has no noise term", who);
      return K5_ERR_STATE;
    }
    if (mag) {
      k5_set_error("%s: a stochastic plan is set (k5_dit_set_stochastic) and %s on the handle: the ratio table was measured on ODE trajectories", who, mag);
      return K5_ERR_STATE;
    }
    if (wt.on && wt.every > 0) {
      k5_set_error("%s: a stochastic plan is set (k5_dit_set_stochastic) and the watch has previews (preview_every = %d): the preview reads "
                   "x0 = x - sigma_next v, which no longer holds after the noise is added; install the watch with preview_every = 0", who, wt.every);
      return K5_ERR_STATE;
    }
  }
  if (tile) {
    if (edit) { k5_set_error("%s: editing with context windows is not supported", who); return K5_ERR_UNSUPPORTED; }
    if (rank_group(d)) { k5_set_error("%s: the handle is in a %s (context windows are single-rank only)", who, rank_group(d)); return K5_ERR_STATE; }
    if (mag) {
      k5_set_error("%s: %s on the handle: the ratio table is indexed by the call of a plain run, a windowed run makes nwin calls per step", who, mag);
      return K5_ERR_STATE;
    }
    if (wt.on && wt.every > 0) {
      k5_set_error("%s: the watch has previews (preview_every = %d): the preview reads one velocity pair per cell, a windowed step has up to nwin; "
                   "install the watch with preview_every = 0", who, wt.every);
      return K5_ERR_STATE;
    }
    // the plan: each axis on its own, by one rule (k5_tile_axis_refusal); spatial windows start on a patch
    if (tile->nt < 1 || tile->ny < 1 || tile->nx < 1 || tile->nt > 64 || tile->ny > 64 || tile->nx > 64 || tile->nt * tile->ny * tile->nx > 64 ||
        !tile->wt || !tile->wy || !tile->wx || n <= 0) {
      k5_set_error("%s: nwin must be 1..64 (got %d x %d x %d) with starts, weights and a window shape", who, tile->nt, tile->ny, tile->nx);
      return K5_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(a->latent) & 3) { k5_set_error("%s: latent is not 4-byte aligned", who); return K5_ERR_ARG; }
    if ((tile->total_H & 1) || (tile->total_W & 1) || (a->fwd.H & 1) || (a->fwd.W & 1)) {
      k5_set_error("%s: the clip's and the window's rows and columns must be even (clip %d x %d, window %d x %d)", who, tile->total_H, tile->total_W,
                   a->fwd.H, a->fwd.W);
      return K5_ERR_ARG;
    }
    const struct { const char* name; int n; const int32_t* st; int F, total; bool even; } ax[3] = {
        {"frame", tile->nt, tile->starts_t, a->fwd.T, tile->total_T, false}, {"row", tile->ny, tile->starts_y, a->fwd.H, tile->total_H, true},
        {"column", tile->nx, tile->starts_x, a->fwd.W, tile->total_W, true}};
    for (const auto& x : ax) {
      if (const char* why = k5_tile_axis_refusal(x.name, x.n, x.st, x.F, x.total)) { k5_set_error("%s: %s", who, why); return K5_ERR_ARG; }
      for (int i = 0; x.even && i < x.n; ++i)
        if (x.st[i] & 1) { k5_set_error("%s: %s window %d starts at %d: spatial windows start on a patch (an even cell)", who, x.name, i, x.st[i]); return K5_ERR_ARG; }
    }
  }
  return K5_OK;
}

namespace {

// What one sample_impl call works on: filled top to bottom by sample_impl before the first step, read by step(i) and by the watch.
struct SampleRun {
  k5_dit* d; const k5_sample_args* a; const float* vcond; const k5_edit_args* edit;
  const k5_sample_tiles_args* tile;         // the window plan (nullptr: a plain run): a->fwd is the window, a->latent / vcond the whole clip
  int nwin = 1;                             //   ... its nt * ny * nx windows
  k5_tile_plan tile_dev{};                  //   ... its tables on the device
  int64_t x_frame = 0, x_row = 0, vc_frame = 0, vc_row = 0;   //   ... and the strides of a window's view of the latent and of vcond (0: the window spans the rows and columns)
  const k5_flowedit_args* fe = nullptr;     // k5_sample_flowedit: steps below fe_steps are FlowEdit steps, the rest plain steps on the target side
  int fe_steps = 0;
  bool fe_src_cfg = false;                  //   the source side runs its unconditional forward
  int fe_src_slot = 0;                      //   the text cache slot of the source prompt (0: it is the target prompt)
  hipStream_t s = nullptr;
  int64_t n = 0, cells = 0;                 // elements and cells of the latent one forward sees (with a plan: a window's)
  bool cfg_on = false, pair = false;        // pair: CFG-parallel, one branch here, the other on the paired handle
  void* vel_c = nullptr; void* vel_u = nullptr;
  void* vel_s = nullptr;                    // skip-layer guidance: the skip branch's velocity (sized when the call has a skip step)
  std::vector<float> host_tab;              // the schedule, three tables of num_steps entries:
  const float* t1000 = nullptr;             //   t * 1000, fp32 (:57)
  const float* dt = nullptr;                //   torch.diff(timesteps) (:105)
  const float* sigma_next = nullptr;        //   where the kept region is re-noised to after step i (k5_sample_edit)
  const float* tvec = nullptr; const float* dtvec = nullptr; const float* signext = nullptr;   // graph mode: the same tables on the device ...
  int* step_ctr = nullptr;                                                                      // ... and the device-side step counter
  const void* slot_prompt[2] = {nullptr, nullptr};   // windows with prompts of their own: whose prologue each text cache slot holds
  // the guidance plan (k5_dit_set_guidance; nullptr: none, every step is of the call's one kind and enqueues what it always did)
  const k5_dit::Guidance* plan = nullptr;
  bool stats = false, want_v = false;       // stats: guided steps take their coefficients from the device; want_v: ... and leave v in vel_c (previews)
  const float* wvec = nullptr;              // graph mode: the per-step weights on the device, next to dtvec
  double* g_sums = nullptr; float* g_ab = nullptr; double* g_part = nullptr;
  // the stochastic plan (k5_dit_set_stochastic; nullptr: none).  Its dt_down stands in `dt` / `dtvec`; graph mode: scale and noise_coef on the device
  const k5_dit::Stochastic* sto = nullptr;
  const float* scalevec = nullptr; const float* coefvec = nullptr;
  bool noisy_at(int i) const { return sto && sto->coef[i] != 0.0f && kind(i) != ZERO; }
  enum Kind { GUIDED, UNGUIDED, ZERO };
  float w_at(int i) const { return plan && !plan->weights.empty() ? plan->weights[i] : a->guidance_weight; }
  Kind kind(int i) const {
    if (plan && i < plan->zero_init) return ZERO;
    return fabsf(w_at(i) - 1.0f) > 1e-6f ? GUIDED : UNGUIDED;   // generation_utils.py:63
  }
  // a skip step (k5_dit_set_skip_guidance): the conditional forward forks and the update reads three velocities
  bool skip_at(int i) const { return !tile && d->skip.at(i) && kind(i) != ZERO; }
  // what the watch's preview of step i combines: a guided step with coefficients and a skip step left their v in vel_c, a zero step has velocity 0 there
  const void* preview_vu(int i) const { return tile ? (cfg_on ? vel_u : nullptr) : kind(i) == GUIDED && !stats && !skip_at(i) ? vel_u : nullptr; }

  // One forward of step i: the text condition through text cache slot `slot`, on the latent slice `x` with its conditioning slice `vc`, into
  // `vel`.  `tables`: the forward reads its time through the device-side step tables when the step is captured; windows pass none.
  // `skip_vel`: the forward forks and leaves the skip branch's velocity there.
  int forward(int i, const k5_text_cond& cond, int slot, const float* x, void* vel, const float* vc, bool tables = true, void* skip_vel = nullptr,
              int cache_slot = -1) {
    ForwardCall f{&a->fwd, cond, t1000[i], x, d->cfg.in_visual_dim, vel, s};
    if (tables) { f.tvec = tvec; f.step = step_ctr; }
    f.text_slot = slot; f.vcond = vc; f.out_skip = skip_vel; f.cache_slot = cache_slot;
    f.x_frame = x_frame; f.x_row = x_row; f.vc_frame = vc_frame; f.vc_row = vc_row;
    if (fe) d->fe.forwards += 1;
    // the forecast cache: step i's forwards are the plan's calls (i, slot); a plan of ones is off — plain forwards, counted as full calls
    if (d->fc.on && d->fc.mixed) { f.fc_step = i; f.fc_slot = slot; }
    else if (d->fc.on) d->fc.full_calls++;
    return forward_impl(d, f);
  }

  // The launch that finishes FlowEdit step i (i < 0: none, the call's first launch) and prepares step i + 1 when there is one to prepare: a
  // further FlowEdit step, or the first plain step, whose latent is zt
  int flowedit_pass(int i) {
    Scope sc(d, s, "elementwise");
    const int nx = i + 1;
    k5_flowedit_step_args e{};
    e.z_fe = a->latent; e.x_src = fe->source; e.w_src = 1.0f; e.w_tar = 1.0f;
    if (i >= 0) {
      e.c_src = d->fe.vel_c.p; e.c_tar = vel_c; e.dt = dt[i]; e.keep_mask = fe->keep_mask;
      if (fe_src_cfg) { e.u_src = d->fe.vel_u.p; e.w_src = fe->source_weight; }
      if (cfg_on) { e.u_tar = vel_u; e.w_tar = a->guidance_weight; }
    }
    e.prepare = nx < a->num_steps;   // past the last step nothing reads them
    if (e.prepare) {
      e.sigma_next = a->sigmas[nx]; e.zs = d->fe.zs.as<float>(); e.zt = d->fe.zt.as<float>();
      e.seed = fe->seed; e.stream_id = fe->first_stream + (uint32_t)nx;
    }
    e.cells = cells; e.C = d->cfg.out_visual_dim;
    if (i < 0 && !e.prepare) return K5_OK;
    return k5_launch_flowedit_step(e, s);
  }

  // FlowEdit step i: source cond, source uncond on zs, target cond, target uncond on zt (a side of weight 1 runs no unconditional forward), then
  // the pass.  After the last FlowEdit step of a call with refine steps the latent becomes zt.
  int flowedit_step(int i) {
    const float* zs = d->fe.zs.as<float>(); const float* zt = d->fe.zt.as<float>();
    K5CHK(forward(i, fe->source_cond, 0, zs, d->fe.vel_c.p, vcond, false, nullptr, fe_src_slot));
    if (fe_src_cfg) K5CHK(forward(i, a->null_cond, 1, zs, d->fe.vel_u.p, vcond, false));
    K5CHK(forward(i, a->fwd.cond, 0, zt, vel_c, vcond, false));
    if (cfg_on) K5CHK(forward(i, a->null_cond, 1, zt, vel_u, vcond, false));
    K5CHK(flowedit_pass(i));
    d->fe.steps += 1;
    if (i + 1 == fe_steps && fe_steps < a->num_steps) return flowedit_to_plain();
    return K5_OK;
  }
  int flowedit_to_plain() {   // the plain steps that close the run start from zt
    HIPCHK(hipMemcpyAsync(a->latent, d->fe.zt.p, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return K5_OK;
  }

  int64_t tile_corner(int k) const {   // the cell of the whole clip at which window k = (it * ny + iy) * nx + ix of the plan begins
    const int ix = k % tile->nx, iy = (k / tile->nx) % tile->ny, it = k / (tile->nx * tile->ny);
    return ((int64_t)tile->starts_t[it] * tile->total_H + tile->starts_y[iy]) * tile->total_W + tile->starts_x[ix];
  }

  int step(int i) {   // enqueue step i: the forwards, then CFG + Euler
    const k5_dit_config& c = d->cfg;
    d->enh.gate = d->enh.at(i) ? 1 : 0;   // Enhance-A-Video: this step's forwards apply it or enqueue what they always did
    void* const vu = (tile ? cfg_on : kind(i) == GUIDED) ? vel_u : nullptr;
    if (tile) {
      // every window on its own box of the latent, from its corner cell (the view strides do the rest; a window of whole frames is contiguous),
      // cond then uncond, into slot k of the velocity buffers; then one pass over the whole clip blends the windows and applies the step
      for (int k = 0; k < nwin; ++k) {
        const k5_text_cond& ck = tile->conds ? tile->conds[k] : a->fwd.cond;
        const k5_text_cond& uk = tile->null_conds ? tile->null_conds[k] : a->null_cond;
        const float* xk = a->latent + tile_corner(k) * c.out_visual_dim;
        const float* vk = vcond ? vcond + tile_corner(k) * (c.in_visual_dim + 1) : nullptr;
        if (slot_prompt[0] != ck.text_embed) { d->text_cache[0].valid = false; slot_prompt[0] = ck.text_embed; }
        K5CHK(forward(i, ck, 0, xk, static_cast<bf16_t*>(vel_c) + k * n, vk, false));
        if (cfg_on) {
          if (slot_prompt[1] != uk.text_embed) { d->text_cache[1].valid = false; slot_prompt[1] = uk.text_embed; }
          K5CHK(forward(i, uk, 1, xk, static_cast<bf16_t*>(vel_u) + k * n, vk, false));
        }
      }
      Scope sc(d, s, "elementwise");
      return k5_launch_cfg_euler_tiles(a->latent, vel_c, vu, a->guidance_weight, dt[i], tile_dev, tile->total_T, tile->total_H, tile->total_W,
                                       c.out_visual_dim, s);
    }
    if (kind(i) == ZERO) return K5_OK;   // velocity 0: no forward, no update
    if (fe && i < fe_steps) return flowedit_step(i);
    const bool skip = skip_at(i);
    if (pair) {
      // my branch only; then the pair's velocities change hands on the side stream (fork / join by events: capturable) and both
      // handles hold [v_cond | v_uncond] — every rank of both groups applies the same update to the same numbers
      if (d->cfg_branch == 0) K5CHK(forward(i, a->fwd.cond, 0, a->latent, vel_c, vcond));
      else K5CHK(forward(i, a->null_cond, 1, a->latent, vel_u, vcond));
      Scope sc(d, s, "comm");
      HIPCHK(hipEventRecord(d->ev_vel_ready, s));
      HIPCHK(hipStreamWaitEvent(d->pair_stream, d->ev_vel_ready, 0));
      K5CHK(d->pair.all_gather_inplace(d->ws_vel_pair.p, (size_t)n, 2, d->pair_stream));
      HIPCHK(hipEventRecord(d->ev_vel_done, d->pair_stream));
      HIPCHK(hipStreamWaitEvent(s, d->ev_vel_done, 0));
    } else {
      K5CHK(forward(i, a->fwd.cond, 0, a->latent, vel_c, vcond, true, skip ? vel_s : nullptr));
      if (vu) K5CHK(forward(i, a->null_cond, 1, a->latent, vel_u, vcond));
    }
    {
      Scope sc(d, s, "elementwise");
      const bool coeffs = vu && stats;   // the sample's coefficients, reduced and applied on the device
      if (coeffs) K5CHK(k5_launch_guidance_coeffs(vel_c, vel_u, n, w_at(i), plan->zero_star, plan->rescale, g_part, g_sums, g_ab, s, wvec, step_ctr));
      K5EulerStepArgs e;
      e.img = a->latent; e.v_cond = vel_c; e.v_uncond = vu; e.w = w_at(i); e.dt = dt[i];
      if (coeffs) { e.ab = g_ab; e.v_out = want_v ? vel_c : nullptr; }
      if (skip) { e.v_skip = vel_s; e.skip_scale = d->skip.scale; e.v_out = want_v ? vel_c : nullptr; }   // the skip term comes after the coefficients
      if (edit) { e.source = edit->source; e.noise = edit->noise; e.keep_mask = edit->keep_mask; e.sigma_next = sigma_next[i]; e.signext = signext; }
      if (sto) {   // the same launch whatever noise_coef is; the captured step adds the device step counter to the stream id itself
        e.stochastic = true; e.scale = sto->scale[i]; e.noise_coef = sto->coef[i]; e.seed = sto->seed;
        e.stream_id = sto->first_stream + (step_ctr ? 0u : (uint32_t)i);
        e.scalevec = scalevec; e.coefvec = coefvec;
      }
      e.cells = cells; e.C = c.out_visual_dim;
      e.dtvec = dtvec; e.step = step_ctr; e.stream = s;
      K5CHK(k5_launch_euler_step(e));
    }
    if (step_ctr) K5CHK(k5_launch_step_inc(step_ctr, s));
    return K5_OK;
  }
};

// The captured step and its executable.  On every way out the stream is drained before they go: the executable graph must outlive its
// launches (this also orders the caller's stream after the sampler).  An eager run holds neither and is not synchronised.
// The handle's launch counters that a step advances from host code.  A replay of the captured step enqueues the same launches without that
// host code, so sample_impl takes the difference over the capture and adds it per further replay.  A new counter is one more entry of `of` (and of K).
struct ReplayCounts {
  static constexpr int K = 6;
  long long per_step[K] = {};
  static void of(k5_dit* d, long long* (&c)[K]) { c[0] = &d->nag.combines; c[1] = &d->regions.combines; c[2] = &d->skip.blocks_shared; c[3] = &d->skip.blocks_run; c[4] = &d->enh.launches; c[5] = &d->fc.full_calls; }
  void snapshot(k5_dit* d) { long long* c[K]; of(d, c); for (int i = 0; i < K; ++i) per_step[i] = *c[i]; }
  void difference(k5_dit* d) { long long* c[K]; of(d, c); for (int i = 0; i < K; ++i) per_step[i] = *c[i] - per_step[i]; }
  void add(k5_dit* d) const { long long* c[K]; of(d, c); for (int i = 0; i < K; ++i) *c[i] += per_step[i]; }
};

struct GraphGuard {
  hipStream_t s; hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
  ~GraphGuard() {
    if (ge) { (void)hipStreamSynchronize(s); (void)hipGraphExecDestroy(ge); }
    if (g) (void)hipGraphDestroy(g);
  }
};

}  // namespace

// The watch's side of a sample_impl call.  step(i) follows the launches of step i on the stream (on a preview step the preview kernel and the
// copy of its RGB to the slot's pinned buffer, then the slot's event); deliver(i) waits for that event on the host and calls back.  step(i)
// runs deliver(i - 1) only once step i is enqueued, so the GPU has a step of work queued while the host waits and calls.
int k5_dit::Watch::begin(const SampleRun& r, const char* who) {
  steps_done = 0; stopped = 0;
  if (!on) return K5_OK;   // nothing below runs, here or in step: the call enqueues what it always did
  if (r.n <= 0) { k5_set_error("%s: bad shapes", who); return K5_ERR_ARG; }
  for (hipEvent_t& e : ev) if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (every > 0) {
    const size_t rb = (size_t)r.cells * 3;
    for (int i = 0; i < 2; ++i) {
      K5CHK(rgb[i].ensure(rb));
      if (want_x0) K5CHK(x0[i].ensure((size_t)r.n * 4));
    }
    if (h_bytes < rb) {
      for (uint8_t*& h : h_rgb) { if (h) (void)hipHostFree(h); h = nullptr; }
      h_bytes = 0;
      for (uint8_t*& h : h_rgb) HIPCHK(hipHostMalloc((void**)&h, rb, hipHostMallocDefault));
      h_bytes = rb;
    }
  }
  return K5_OK;
}

bool k5_dit::Watch::preview_at(const SampleRun& r, int i) const { return every > 0 && ((i + 1) % every == 0 || i == r.a->num_steps - 1); }

int k5_dit::Watch::step(const SampleRun& r, int i) {   // after step i is enqueued; the caller leaves its loop when `stopped`
  const int slot = i & 1;
  if (preview_at(r, i)) {
    Scope sc(r.d, r.s, "elementwise");
    const int C = r.d->cfg.in_visual_dim;
    const float* w = wb.as<float>();
    if (!r.tile && r.kind(i) == SampleRun::ZERO) HIPCHK(hipMemsetAsync(r.vel_c, 0, (size_t)r.n * 2, r.s));   // a zero-init step: x0 = x
    K5CHK(k5_launch_x0_preview(r.a->latent, r.vel_c, r.preview_vu(i), r.w_at(i), r.sigma_next[i],
                               r.edit ? r.edit->source : nullptr, r.edit ? r.edit->keep_mask : nullptr, w, w + 3 * C,
                               want_x0 ? x0[slot].as<float>() : nullptr, rgb[slot].as<uint8_t>(), r.cells, C, r.s));
    HIPCHK(hipMemcpyAsync(h_rgb[slot], rgb[slot].p, (size_t)r.cells * 3, hipMemcpyDeviceToHost, r.s));
  }
  HIPCHK(hipEventRecord(ev[slot], r.s));
  steps_done = i + 1;
  if (i > 0) K5CHK(deliver(r, i - 1));
  return K5_OK;
}

int k5_dit::Watch::deliver(const SampleRun& r, int i) {
  const int slot = i & 1;
  HIPCHK(hipEventSynchronize(ev[slot]));
  const bool pv = preview_at(r, i);
  k5_watch_info info{};
  info.step = i; info.num_steps = r.a->num_steps; info.sample = sample; info.num_samples = num_samples;
  info.sigma_next = r.sigma_next[i];
  info.rgb = pv ? h_rgb[slot] : nullptr;
  info.x0 = pv && want_x0 ? x0[slot].as<float>() : nullptr;
  info.T = r.tile ? r.tile->total_T : r.a->fwd.T; info.H = r.tile ? r.tile->total_H : r.a->fwd.H; info.W = r.tile ? r.tile->total_W : r.a->fwd.W;
  info.C = r.d->cfg.in_visual_dim;
  if (fn(user, &info) != 0) stopped = 1;
  return K5_OK;
}

int k5_dit::Watch::end(const SampleRun& r) {   // the last step's callback; a stopped run ends with the stream drained
  if (!on) { steps_done = r.a->num_steps; return K5_OK; }
  if (!stopped) K5CHK(deliver(r, steps_done - 1));
  if (stopped) HIPCHK(hipStreamSynchronize(r.s));
  return K5_OK;
}

// The sampler loop behind k5_sample / k5_sample_cond (edit == nullptr: their launches, their bits), k5_sample_edit, k5_sample_flowedit and
// the windowed entries (tile != nullptr: a->fwd is the window, a->latent / vcond the whole clip of the plan; never together with edit or fe).
static int sample_impl(k5_dit* d, const k5_sample_args* a, const float* vcond, const k5_edit_args* edit, void* stream, const char* who,
                       const k5_sample_tiles_args* tile = nullptr, const k5_flowedit_args* fe = nullptr) {
  g_err[0] = 0;
  K5CHK(sample_refusals(d, a, vcond, edit, tile, who, fe));
  const k5_dit_config& c = d->cfg;
  k5_dit::Watch& wt = d->watch;
  SampleRun r{d, a, vcond, edit, tile};
  r.fe = fe;
  if (tile) r.nwin = tile->nt * tile->ny * tile->nx;
  r.s = (hipStream_t)stream;
  r.cells = (int64_t)a->fwd.T * a->fwd.H * a->fwd.W;
  r.n = r.cells * c.out_visual_dim;
  K5CHK(wt.begin(r, who));
  const int N = a->num_steps;
  k5_dit::Guidance& gd = d->guide;
  r.cfg_on = fabsf(a->guidance_weight - 1.0f) > 1e-6f;  // generation_utils.py:63
  int first = 0;          // the first step that runs a forward (N: none does)
  bool uniform = true;    // every step enqueues the same launches, so one captured step can stand for all of them
  if (gd.on) {
    r.plan = &gd;
    int guided = 0, unguided = 0;
    bool const_w = true;
    first = gd.zero_init < N ? gd.zero_init : N;
    for (int i = first; i < N; ++i) {
      (r.kind(i) == SampleRun::GUIDED ? guided : unguided) += 1;
      const_w = const_w && r.w_at(i) == r.w_at(first);
    }
    r.cfg_on = guided > 0;   // the unconditional side is sized before the loop, wherever its first step is
    r.stats = gd.stats() && guided > 0;
    r.want_v = r.stats && wt.on && wt.every > 0;
    // euler_step_kernel takes its CFG weight by value: without coefficients only a constant weight replays
    uniform = first == 0 && !(guided && unguided) && (r.stats || !guided || const_w);
    if (r.stats) {
      K5CHK(gd.ws.ensure(64 + (size_t)k5_guidance_blocks(r.n) * 5 * sizeof(double)));
      r.g_sums = gd.ws.as<double>(); r.g_ab = reinterpret_cast<float*>(static_cast<char*>(gd.ws.p) + 48);
      r.g_part = reinterpret_cast<double*>(static_cast<char*>(gd.ws.p) + 64);
    }
  }
  int nskip = 0;
  for (int i = first; i < N; ++i) nskip += r.skip_at(i) ? 1 : 0;
  if (nskip) {   // the third velocity, sized before the loop; the captured step stands for every step only when all of them fork or none does
    K5CHK(d->skip.vel.ensure(r.n * 2));
    r.vel_s = d->skip.vel.p;
    r.want_v = r.want_v || (wt.on && wt.every > 0);
    uniform = uniform && nskip == N - first;
  }
  // Enhance-A-Video: the steps whose forwards carry the score and scale launches; one captured step stands for all only when all or none do
  int nenh = 0;
  for (int i = first; i < N; ++i) nenh += d->enh.at(i) && a->fwd.T >= 2 ? 1 : 0;
  uniform = uniform && (nenh == 0 || nenh == N - first);
  struct EnhanceGuard { k5_dit* d; ~EnhanceGuard() { d->enh.gate = -1; } } enhance_guard{d};
  // the forecast cache: every call and every sample starts without history; a plan with forecast steps has steps of two kinds
  d->fc.clear_history();
  uniform = uniform && !(d->fc.on && d->fc.mixed);
  r.pair = r.cfg_on && d->pair.active();
  if (r.pair) K5CHK(d->ws_vel_pair.ensure(2 * r.n * 2));
  else {   // one slot per window
    K5CHK(d->ws_vel_c.ensure(r.nwin * r.n * 2));
    if (r.cfg_on) K5CHK(d->ws_vel_u.ensure(r.nwin * r.n * 2));
  }
  r.vel_c = r.pair ? d->ws_vel_pair.p : d->ws_vel_c.p;
  r.vel_u = r.pair ? (void*)(d->ws_vel_pair.as<bf16_t>() + r.n) : d->ws_vel_u.p;
  // hipGraph mode (BASELINE config 5 "hipGraph-captured step"): the per-step scalars live in device tables indexed by a
  // device-side step counter, so ONE captured step (forward(s) + CFG/Euler + counter increment) replays for every step.
  // Step 0 runs eagerly (it sizes every workspace and fills the RoPE / permutation caches), step 1 is captured, steps 1..
  // are launches of the instantiated graph.
  // Not replayed: MagCache (host decisions: its skip pattern changes the launch sequence per step) and its calibration (host-side call
  // counter and buffer swap), profiling (events), the NABLA map tap (its destination advances on the host per launch: a replay would
  // overwrite the slots baked at capture — ADVICE r5), loopback groups (their collectives are host rendezvous), windows (the captured step
  // holds one forward pair).  The IPC transport IS replayable: its epochs live on the device and the peers' buffers were mapped by the eager
  // first step (ipc_comm.h)
  const bool graph = d->use_graph && !d->mag.on && !d->cal.on && !d->profiling && a->num_steps > 2 && !d->nabla_tap && !d->comm.loop && !d->pair.loop &&
                     !tile && !fe && uniform;   // FlowEdit: steps of two kinds, and the pass reads its scalars by value
  if (d->sto.on) r.sto = &d->sto;
  const size_t sto_at = (gd.on ? 4 : 3) * (size_t)N;   // with a stochastic plan two more tables: scale and noise_coef
  r.host_tab.resize(sto_at + (r.sto ? 2 : 0) * (size_t)N);
  for (int i = 0; i < N; ++i) {
    r.host_tab[i] = a->sigmas[i] * 1000.0f;
    r.host_tab[N + i] = r.sto ? r.sto->dt_down[i] : a->sigmas[i + 1] - a->sigmas[i];   // a step without noise has dt_down == this difference
    r.host_tab[2 * N + i] = a->sigmas[i + 1];
    if (gd.on) r.host_tab[3 * N + i] = r.w_at(i);   // a fourth table with a plan: the weight the coefficients read in the captured step
    if (r.sto) { r.host_tab[sto_at + i] = r.sto->scale[i]; r.host_tab[sto_at + N + i] = r.sto->coef[i]; }
  }
  r.t1000 = r.host_tab.data(); r.dt = r.t1000 + N; r.sigma_next = r.dt + N;
  if (graph) {
    if (!d->graph_stream) {
      HIPCHK(hipStreamCreateWithFlags(&d->graph_stream, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&d->ev_graph, hipEventDisableTiming));
    }
    HIPCHK(hipEventRecord(d->ev_graph, r.s));             // everything the caller enqueued so far happens before the sampler
    r.s = d->graph_stream;
    HIPCHK(hipStreamWaitEvent(r.s, d->ev_graph, 0));
    K5CHK(d->ws_sched.ensure(r.host_tab.size() * 4 + 16));
    HIPCHK(hipMemcpyAsync(d->ws_sched.p, r.host_tab.data(), r.host_tab.size() * 4, hipMemcpyHostToDevice, r.s));
    r.step_ctr = reinterpret_cast<int*>(d->ws_sched.as<float>() + r.host_tab.size());
    HIPCHK(hipMemsetAsync(r.step_ctr, 0, 4, r.s));
    HIPCHK(hipStreamSynchronize(r.s));   // host_tab lives in this call only
    r.tvec = d->ws_sched.as<float>(); r.dtvec = r.tvec + N; r.signext = r.dtvec + N;
    if (gd.on) r.wvec = r.signext + N;
    if (r.sto) { r.scalevec = r.tvec + sto_at; r.coefvec = r.scalevec + N; }
  }
  const hipStream_t s = r.s;
  if (edit) {   // the start latent: the source at sigmas[0] everywhere, whatever the mask
    Scope sc(d, s, "elementwise");
    K5CHK(k5_launch_edit_renoise(a->latent, edit->source, edit->noise, a->sigmas[0], r.n, s));
  }
  if (tile) {   // the plan, uploaded once per call: the three int32 start vectors, then the three fp32 weight tables
    const int cnt[3] = {tile->nt, tile->ny, tile->nx}, ext[3] = {a->fwd.T, a->fwd.H, a->fwd.W};
    const int32_t* st[3] = {tile->starts_t, tile->starts_y, tile->starts_x};
    const float* wg[3] = {tile->wt, tile->wy, tile->wx};
    std::vector<int32_t> host((size_t)cnt[0] + cnt[1] + cnt[2]);
    size_t at = 0, off[6];
    for (int i = 0; i < 3; ++i) { off[i] = at; memcpy(host.data() + at, st[i], (size_t)cnt[i] * 4); at += cnt[i]; }
    for (int i = 0; i < 3; ++i) {
      off[3 + i] = at;
      host.resize(at + (size_t)cnt[i] * ext[i]);
      memcpy(host.data() + at, wg[i], (size_t)cnt[i] * ext[i] * 4);
      at += (size_t)cnt[i] * ext[i];
    }
    K5CHK(d->ws_win.ensure(host.size() * 4));
    HIPCHK(hipMemcpyAsync(d->ws_win.p, host.data(), host.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // `host` lives in this block only
    const int32_t* base = d->ws_win.as<int32_t>();
    r.tile_dev = k5_tile_plan{tile->nt, tile->ny, tile->nx, a->fwd.T, a->fwd.H, a->fwd.W, base + off[0], base + off[1], base + off[2],
                              reinterpret_cast<const float*>(base + off[3]), reinterpret_cast<const float*>(base + off[4]),
                              reinterpret_cast<const float*>(base + off[5])};
    // the one place the plan's shape is looked at: a window that spans the clip's rows and columns is whole frames, contiguous, and its
    // forwards take the compact patchify kernels; any other window is a strided view
    if (a->fwd.H != tile->total_H || a->fwd.W != tile->total_W) {
      r.x_row = (int64_t)tile->total_W * c.out_visual_dim; r.x_frame = r.x_row * tile->total_H;
      r.vc_row = (int64_t)tile->total_W * (c.in_visual_dim + 1); r.vc_frame = r.vc_row * tile->total_H;
    }
  }
  struct FlowEditGuard { k5_dit* d; ~FlowEditGuard() { d->fe.active = false; } } flowedit_guard{d};
  if (fe) {   // z_fe = x_src lives in the latent; the first launch forms zs / zt of step 0 (with no FlowEdit step: the first plain step's latent)
    const k5_text_cond& sc = fe->source_cond; const k5_text_cond& tc = a->fwd.cond;
    r.fe_steps = N - fe->refine;
    r.fe_src_cfg = fabsf(fe->source_weight - 1.0f) > 1e-6f;
    r.fe_src_slot = sc.text_embed == tc.text_embed && sc.pooled_embed == tc.pooled_embed && sc.text_len == tc.text_len ? 0 : k5_dit::kFlowEditSlot;
    K5CHK(d->fe.zs.ensure((size_t)r.n * 4));
    K5CHK(d->fe.zt.ensure((size_t)r.n * 4));
    K5CHK(d->fe.vel_c.ensure((size_t)r.n * 2));
    if (r.fe_src_cfg) K5CHK(d->fe.vel_u.ensure((size_t)r.n * 2));
    d->fe.active = true;
    HIPCHK(hipMemcpyAsync(a->latent, fe->source, (size_t)r.n * 4, hipMemcpyDeviceToDevice, s));
    K5CHK(r.flowedit_pass(-1));
    if (r.fe_steps == 0) K5CHK(r.flowedit_to_plain());
  }
  d->drop_text_cache();                                      // the prompt tensors are constant for THIS call only
  K5CHK(reset_attn_pref(d, s));                              // ... and so is what the softmax-form memory of the layers is worth
  // where the visual queries are normalised (see k5_dit::fuse_qnorm_auto): a plain one-handle dense run decides after its first step
  struct FuseGuard { k5_dit* d; ~FuseGuard() { d->fuse_now = false; d->leave_collect = false; } } fuse_guard{d};
  d->fuse_now = false; d->leave_collect = false; d->fuse_last = -1;
  const bool auto_fuse = d->fuse_qnorm_auto && !d->fuse_qnorm && !d->comm.active() && d->attn_mode == K5_ATTN_AUTO && d->row_offsets &&   // (a CFG pair's handles decide each for itself)
                         a->fwd.attention_type == 0 && N - first >= 2 && !nenh;   // Enhance-A-Video needs the normalised q in memory
  if (nenh) d->fuse_last = 0;
  if (auto_fuse) {
    K5CHK(d->ws_leave_sig.ensure(4));
    if (!d->h_leave_sig) HIPCHK(hipHostMalloc((void**)&d->h_leave_sig, 4, hipHostMallocDefault));
    HIPCHK(hipMemsetAsync(d->ws_leave_sig.p, 0, 4, s));
    d->leave_collect = true;
  }
  auto decide_fuse = [&]() -> int {   // after the first step that ran a forward
    if (!auto_fuse) return K5_OK;
    d->leave_collect = false;
    *d->h_leave_sig = 1u;
    HIPCHK(hipMemcpyAsync(d->h_leave_sig, d->ws_leave_sig.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   // once per call: the host runs a step ahead otherwise
    d->fuse_now = *d->h_leave_sig == 0u;
    d->fuse_last = d->fuse_now ? 1 : 0;
    return K5_OK;
  };
  // Step 0 is always eager.  In graph mode step 1 is captured and instantiated (after the watch has followed step 0: those launches are not
  // part of the graph) and steps 1.. are launches of the executable; between them the watch reads sigma_next as a host scalar.
  GraphGuard cap{s};
  ReplayCounts counts;
  for (int i = 0; i < N; ++i) {
    if (i == 0 || !graph) K5CHK(r.step(i));
    else {
      if (i == 1) {
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        counts.snapshot(d);
        const int rc = r.step(1);
        counts.difference(d);   // the state getters count launches: the capture stands for step 1's, every further replay adds as many
        const hipError_t ec = hipStreamEndCapture(s, &cap.g);
        if (rc != K5_OK) return rc;
        if (ec != hipSuccess || !cap.g) { k5_set_error("hipStreamEndCapture: %s", hipGetErrorString(ec)); return K5_ERR_HIP; }
        if (hipGraphInstantiate(&cap.ge, cap.g, nullptr, nullptr, 0) != hipSuccess) { k5_set_error("hipGraphInstantiate failed"); return K5_ERR_HIP; }
      }
      if (hipGraphLaunch(cap.ge, s) != hipSuccess) { k5_set_error("hipGraphLaunch failed"); return K5_ERR_HIP; }
      if (i > 1) counts.add(d);
    }
    if (i == first) K5CHK(decide_fuse());
    if (gd.on) (r.kind(i) == SampleRun::GUIDED ? gd.guided : r.kind(i) == SampleRun::UNGUIDED ? gd.unguided : gd.zero) += 1;
    if (r.skip_at(i)) d->skip.skip_steps += 1;
    // per step on the host, not through ReplayCounts: the captured step's difference would count the last step, which draws nothing, as step 1
    if (r.noisy_at(i)) d->sto.noisy_steps += 1;
    if (wt.on) {
      K5CHK(wt.step(r, i));
      if (wt.stopped) break;
    }
  }
  return wt.end(r);
}

extern "C" int k5_sample_cond(k5_dit* d, const k5_sample_args* a, const float* vcond, void* stream) {
  return sample_impl(d, a, vcond, nullptr, stream, "k5_sample_cond");
}

extern "C" int k5_sample(k5_dit* d, const k5_sample_args* a, void* stream) { return k5_sample_cond(d, a, nullptr, stream); }

extern "C" int k5_sample_edit(k5_dit* d, const k5_sample_args* a, const float* vcond, const k5_edit_args* edit, void* stream) {
  return sample_impl(d, a, vcond, edit, stream, edit ? "k5_sample_edit" : "k5_sample_cond");
}

extern "C" int k5_sample_flowedit(k5_dit* d, const k5_sample_args* a, const k5_flowedit_args* fe, const float* vcond, void* stream) {
  if (!fe) { g_err[0] = 0; k5_set_error("k5_sample_flowedit: null FlowEdit arguments"); return K5_ERR_ARG; }
  return sample_impl(d, a, vcond, nullptr, stream, "k5_sample_flowedit", nullptr, fe);
}

extern "C" int k5_dit_flowedit_state(k5_dit* d, long long* steps, long long* forwards, long long* prologues, int reset) {
  if (!d) { k5_set_error("k5_dit_flowedit_state: null handle"); return K5_ERR_ARG; }
  if (steps) *steps = d->fe.steps;
  if (forwards) *forwards = d->fe.forwards;
  if (prologues) *prologues = d->fe.prologues;
  if (reset) d->fe.steps = d->fe.forwards = d->fe.prologues = 0;
  return K5_OK;
}

// The windowed run behind k5_sample_tiles and k5_sample_windows (`who`).  A clip no larger than the window in every axis is the plain run on the
// whole clip (the first entries of pos_* are its positions).
static int sample_windowed(k5_dit* d, const k5_sample_tiles_args* t, const float* vcond, void* stream, const char* who) {
  g_err[0] = 0;
  if (t->total_T < 1 || t->total_H < 1 || t->total_W < 1) {
    k5_set_error("%s: the clip must be >= 1 in every axis (got %d, %d, %d)", who, t->total_T, t->total_H, t->total_W);
    return K5_ERR_ARG;
  }
  const k5_forward_args& f = t->sample.fwd;
  if (t->total_T <= f.T && t->total_H <= f.H && t->total_W <= f.W) {
    k5_sample_args one = t->sample;
    one.fwd.T = t->total_T; one.fwd.H = t->total_H; one.fwd.W = t->total_W;
    if (t->conds) one.fwd.cond = t->conds[0];
    if (t->null_conds) one.null_cond = t->null_conds[0];
    return sample_impl(d, &one, vcond, nullptr, stream, who);
  }
  return sample_impl(d, &t->sample, vcond, nullptr, stream, who, t);
}

// A temporal plan is the 3-D plan with one row window and one column window of weight 1 that span the clip
extern "C" int k5_sample_windows(k5_dit* d, const k5_sample_windows_args* w, const float* vcond, void* stream) {
  g_err[0] = 0;
  if (!d || !w) { k5_set_error("k5_sample_windows: null handle or arguments"); return K5_ERR_ARG; }
  const k5_forward_args& f = w->sample.fwd;
  static const int32_t zero = 0;
  const std::vector<float> ones((size_t)std::max(1, std::max(f.H, f.W)), 1.0f);
  const k5_sample_tiles_args t{w->sample, w->total_T, f.H, f.W, w->nwin, 1, 1, w->starts, &zero, &zero, w->weights, ones.data(), ones.data(),
                               w->conds, w->null_conds};
  return sample_windowed(d, &t, vcond, stream, "k5_sample_windows");
}

extern "C" int k5_sample_tiles(k5_dit* d, const k5_sample_tiles_args* t, const float* vcond, void* stream) {
  g_err[0] = 0;
  if (!d || !t) { k5_set_error("k5_sample_tiles: null handle or arguments"); return K5_ERR_ARG; }
  return sample_windowed(d, t, vcond, stream, "k5_sample_tiles");
}

// What k5_sample_many / k5_dit_forward_many refuse before anything is enqueued: handle states whose per-call bookkeeping is not per sample (rank
// groups exchange per forward, MagCache counts calls, a captured step is per call).
static int many_state_ok(const k5_dit* d, const char* who) {
  if (!d->finalized) { k5_set_error("%s before k5_dit_finalize", who); return K5_ERR_STATE; }
  if (rank_group(d)) { k5_set_error("%s: the handle is in a %s", who, rank_group(d)); return K5_ERR_STATE; }
  if (d->mag.on) { k5_set_error("%s: MagCache is set on the handle", who); return K5_ERR_STATE; }
  if (d->cal.on) { k5_set_error("%s: the handle is calibrating MagCache", who); return K5_ERR_STATE; }
  if (d->use_graph) { k5_set_error("%s: graph capture is on (k5_dit_set_graph)", who); return K5_ERR_STATE; }
  if (d->sto.on && !strcmp(who, "k5_sample_many")) {
    k5_set_error("%s: a stochastic plan is set (k5_dit_set_stochastic): it holds one seed, the samples of a batch need one each — run them one at a time", who);
    return K5_ERR_STATE;
  }
  return K5_OK;
}

// Several samples in one call, one after another: sample b is k5_sample_cond on its own slice of the latents / conditioning with its own
// prompts, so it resets exactly the per-call state a call of its own would (text prologue cache, softmax-form memory, the query-norm
// decision) and moves no bits.  No launch is shared between samples: the cost per sample is that of a separate call.
extern "C" int k5_sample_many(k5_dit* d, const k5_sample_many_args* a, void* stream) {
  g_err[0] = 0;
  if (!d || !a) { k5_set_error("k5_sample_many: null handle or arguments"); return K5_ERR_ARG; }
  K5CHK(many_state_ok(d, "k5_sample_many"));
  const k5_dit_config& c = d->cfg;
  if (a->B < 1) { k5_set_error("k5_sample_many: B must be >= 1 (got %d)", a->B); return K5_ERR_ARG; }
  if (!a->latents || (reinterpret_cast<uintptr_t>(a->latents) & 3)) { k5_set_error("k5_sample_many: latents is NULL or not 4-byte aligned"); return K5_ERR_ARG; }
  if (a->visual_cond && !c.visual_cond) { k5_set_error("k5_sample_many: visual_cond given to a handle created with visual_cond = 0"); return K5_ERR_ARG; }
  if (a->visual_cond && (reinterpret_cast<uintptr_t>(a->visual_cond) & 3)) { k5_set_error("k5_sample_many: visual_cond is not 4-byte aligned"); return K5_ERR_ARG; }
  if (!a->sigmas || a->num_steps <= 0) { k5_set_error("k5_sample_many: sigmas / num_steps"); return K5_ERR_ARG; }
  const bool cfg_on = fabsf(a->guidance_weight - 1.0f) > 1e-6f;
  if (!a->conds || (cfg_on && !a->null_conds)) { k5_set_error("k5_sample_many: conds%s missing", cfg_on ? " / null_conds" : ""); return K5_ERR_ARG; }
  if (a->fwd.T <= 0 || a->fwd.H <= 0 || a->fwd.W <= 0) { k5_set_error("k5_sample_many: bad shapes"); return K5_ERR_ARG; }
  const size_t thw = (size_t)a->fwd.T * a->fwd.H * a->fwd.W;
  for (int b = 0; b < a->B; ++b) {
    k5_sample_args one{};
    one.fwd = a->fwd;
    one.fwd.x = nullptr;
    one.fwd.cond = a->conds[b];
    if (cfg_on || (d->guide.on && a->null_conds)) one.null_cond = a->null_conds[b];   // a guidance plan may guide where the call's weight is 1
    one.latent = a->latents + (size_t)b * thw * c.in_visual_dim;
    one.num_steps = a->num_steps;
    one.sigmas = a->sigmas;
    one.guidance_weight = a->guidance_weight;
    const float* vc = a->visual_cond ? a->visual_cond + (size_t)b * thw * (c.in_visual_dim + 1) : nullptr;
    d->watch.sample = b; d->watch.num_samples = a->B;
    const int st = k5_sample_cond(d, &one, vc, stream);
    d->watch.sample = 0; d->watch.num_samples = 1;
    if (st != K5_OK) {
      if (!g_err[0]) k5_set_error("k5_sample_many: sample %d failed with status %d", b, st);
      return st;
    }
    if (d->watch.stopped) break;   // the callback stopped sample b: the samples after it stay as they came
  }
  return K5_OK;
}

extern "C" int k5_dit_set_watch(k5_dit* d, const k5_watch* w) {
  g_err[0] = 0;
  if (!d) { k5_set_error("k5_dit_set_watch: null handle"); return K5_ERR_ARG; }
  k5_dit::Watch& wt = d->watch;
  if (!w) { wt.on = false; wt.fn = nullptr; wt.user = nullptr; wt.every = 0; wt.want_x0 = false; return K5_OK; }
  if (!w->fn) { k5_set_error("k5_dit_set_watch: fn is NULL (pass a NULL watch to clear)"); return K5_ERR_ARG; }
  if (w->preview_every < 0) { k5_set_error("k5_dit_set_watch: preview_every must be >= 0 (got %d)", w->preview_every); return K5_ERR_ARG; }
  if (w->preview_every > 0 && !w->rgb_w) { k5_set_error("k5_dit_set_watch: previews (preview_every = %d) need rgb_w", w->preview_every); return K5_ERR_ARG; }
  if (w->want_x0 && w->preview_every == 0) { k5_set_error("k5_dit_set_watch: want_x0 needs preview_every > 0 (x0 comes with the preview steps)"); return K5_ERR_ARG; }
  if (rank_group(d)) {
    k5_set_error("k5_dit_set_watch: the handle is in a %s: a rank that stops alone would leave its peers inside a collective", rank_group(d));
    return K5_ERR_STATE;
  }
  if (w->preview_every > 0) {
    const int C = d->cfg.in_visual_dim;
    if (C <= 0 || (C & 3) || C > 64) { k5_set_error("k5_dit_set_watch: previews need in_visual_dim %% 4 == 0 and <= 64 (got %d)", C); return K5_ERR_UNSUPPORTED; }
    std::vector<float> h((size_t)3 * C + 3, 0.0f);
    memcpy(h.data(), w->rgb_w, (size_t)3 * C * sizeof(float));
    if (w->rgb_b) memcpy(h.data() + 3 * C, w->rgb_b, 3 * sizeof(float));
    K5CHK(wt.wb.ensure(h.size() * sizeof(float)));
    HIPCHK(hipMemcpy(wt.wb.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  wt.fn = w->fn; wt.user = w->user; wt.every = w->preview_every; wt.want_x0 = w->want_x0 != 0; wt.on = true;
  return K5_OK;
}

namespace {
// a prompt the handle borrows until it is cleared (k5_dit_set_nag, k5_dit_set_regions).  who: the refusing call; whose: the prompt in the
// sentence about its pointers; len_of: what stands in front of "text_len" in the one about its length
int check_borrowed_prompt(const k5_text_cond& c, const char* who, const char* whose, const char* len_of) {
  if (c.text_len < 1) { k5_set_error("%s: %stext_len must be >= 1 (got %d)", who, len_of, c.text_len); return K5_ERR_ARG; }
  if (!c.text_embed || !c.text_rope_pos) { k5_set_error("%s: %s needs text_embed and text_rope_pos", who, whose); return K5_ERR_ARG; }
  return K5_OK;
}
}  // namespace

extern "C" int k5_dit_set_nag(k5_dit* d, const k5_text_cond* negative, float scale, float tau, float alpha) {
  g_err[0] = 0;
  if (!d) { k5_set_error("k5_dit_set_nag: null handle"); return K5_ERR_ARG; }
  k5_dit::Nag& ng = d->nag;
  if (!negative) { ng.on = false; ng.neg = nullptr; d->text_cache[2].valid = false; return K5_OK; }
  if (!(scale >= 1.0f)) { k5_set_error("k5_dit_set_nag: scale must be >= 1 (got %g)", (double)scale); return K5_ERR_ARG; }
  if (!(tau >= 1.0f)) { k5_set_error("k5_dit_set_nag: tau must be >= 1 (got %g)", (double)tau); return K5_ERR_ARG; }
  if (!(alpha >= 0.0f && alpha <= 1.0f)) { k5_set_error("k5_dit_set_nag: alpha must be in [0, 1] (got %g)", (double)alpha); return K5_ERR_ARG; }
  K5CHK(check_borrowed_prompt(*negative, "k5_dit_set_nag", "the negative prompt", ""));
  ng.neg = negative; ng.scale = scale; ng.tau = tau; ng.alpha = alpha;
  ng.on = scale != 1.0f && alpha != 0.0f;   // otherwise the combine hands z_pos through: run nothing
  d->text_cache[2].valid = false;
  return K5_OK;
}

extern "C" int k5_dit_set_regions(k5_dit* d, const k5_text_cond* regions, int R, const float* masks, int T, int H, int W, float base_weight) {
  g_err[0] = 0;
  if (!d) { k5_set_error("k5_dit_set_regions: null handle"); return K5_ERR_ARG; }
  k5_dit::Regions& rg = d->regions;
  const auto clear = [&]() {
    rg.on = false; rg.R = 0; rg.conds = nullptr; rg.masks = nullptr; rg.w_order = -1;
    for (int r = 0; r < 8; ++r) d->text_cache[3 + r].valid = false;
  };
  if (!regions || R == 0) { clear(); return K5_OK; }
  if (R < 0 || R > 8) { k5_set_error("k5_dit_set_regions: R must be 1..8 (got %d)", R); return K5_ERR_ARG; }
  if (!(base_weight >= 0.0f && base_weight <= 1.0f)) { k5_set_error("k5_dit_set_regions: base_weight must be in [0, 1] (got %g)", (double)base_weight); return K5_ERR_ARG; }
  if (!masks) { k5_set_error("k5_dit_set_regions: masks is NULL"); return K5_ERR_ARG; }
  if (reinterpret_cast<uintptr_t>(masks) & 3) { k5_set_error("k5_dit_set_regions: masks is not 4-byte aligned"); return K5_ERR_ARG; }
  const int* ps = d->cfg.patch_size;
  if (T < 1 || H < 1 || W < 1 || ps[0] < 1 || ps[1] < 1 || ps[2] < 1 || (T % ps[0]) || (H % ps[1]) || (W % ps[2])) {
    k5_set_error("k5_dit_set_regions: the masks' shape (%d, %d, %d) must be positive and divisible by the patch (%d, %d, %d)", T, H, W, ps[0], ps[1], ps[2]);
    return K5_ERR_ARG;
  }
  for (int r = 0; r < R; ++r) {
    char whose[16], len_of[20];
    snprintf(whose, sizeof whose, "region %d", r); snprintf(len_of, sizeof len_of, "region %d: ", r);
    K5CHK(check_borrowed_prompt(regions[r], "k5_dit_set_regions", whose, len_of));
  }
  clear();
  rg.conds = regions; rg.R = R; rg.masks = masks; rg.T = T; rg.H = H; rg.W = W; rg.base_weight = base_weight;
  rg.on = true;
  return K5_OK;
}

extern "C" int k5_dit_regions_state(k5_dit* d, int* on, int* R, long long* combines, int reset) {
  if (!d) { k5_set_error("k5_dit_regions_state: null handle"); return K5_ERR_ARG; }
  if (on) *on = d->regions.on ? 1 : 0;
  if (R) *R = d->regions.on ? d->regions.R : 0;
  if (combines) *combines = d->regions.combines;
  if (reset) d->regions.combines = 0;
  return K5_OK;
}

extern "C" int k5_dit_set_guidance(k5_dit* d, const k5_guidance* g) {
  g_err[0] = 0;
  if (!d) { k5_set_error("k5_dit_set_guidance: null handle"); return K5_ERR_ARG; }
  k5_dit::Guidance& gd = d->guide;
  if (!g) { gd.on = false; gd.weights.clear(); gd.zero_star = false; gd.zero_init = 0; gd.rescale = 0.f; return K5_OK; }
  if (g->weights && g->num_weights < 1) { k5_set_error("k5_dit_set_guidance: weights with num_weights = %d", g->num_weights); return K5_ERR_ARG; }
  for (int i = 0; g->weights && i < g->num_weights; ++i)
    if (!isfinite(g->weights[i])) { k5_set_error("k5_dit_set_guidance: weights[%d] is not finite", i); return K5_ERR_ARG; }
  if (g->zero_init_steps < 0) { k5_set_error("k5_dit_set_guidance: zero_init_steps must be >= 0 (got %d)", g->zero_init_steps); return K5_ERR_ARG; }
  if (!(g->rescale >= 0.0f && g->rescale <= 1.0f)) { k5_set_error("k5_dit_set_guidance: rescale must be in [0, 1] (got %g)", (double)g->rescale); return K5_ERR_ARG; }
  gd.weights.assign(g->weights, g->weights ? g->weights + g->num_weights : g->weights);
  gd.zero_star = g->zero_star != 0; gd.zero_init = g->zero_init_steps; gd.rescale = g->rescale;
  gd.on = true;
  return K5_OK;
}

extern "C" int k5_dit_guidance_state(k5_dit* d, int* on, long long* guided_steps, long long* unguided_steps, long long* zero_steps, int reset) {
  if (!d) { k5_set_error("k5_dit_guidance_state: null handle"); return K5_ERR_ARG; }
  k5_dit::Guidance& gd = d->guide;
  if (on) *on = gd.on ? 1 : 0;
  if (guided_steps) *guided_steps = gd.guided;
  if (unguided_steps) *unguided_steps = gd.unguided;
  if (zero_steps) *zero_steps = gd.zero;
  if (reset) gd.guided = gd.unguided = gd.zero = 0;
  return K5_OK;
}

extern "C" int k5_dit_set_skip_guidance(k5_dit* d, const k5_skip_guidance* g) {
  g_err[0] = 0;
  if (!d) { k5_set_error("k5_dit_set_skip_guidance: null handle"); return K5_ERR_ARG; }
  k5_dit::Skip& sk = d->skip;
  if (!g) { sk.on = false; sk.skipped.clear(); sk.steps.clear(); sk.k0 = 0; sk.mode = 0; sk.scale = 0.f; return K5_OK; }
  const int nb = d->cfg.num_visual_blocks;
  if (!g->blocks || g->num_blocks < 1) { k5_set_error("k5_dit_set_skip_guidance: blocks with num_blocks = %d", g->num_blocks); return K5_ERR_ARG; }
  if (g->mode != 0 && g->mode != 1) { k5_set_error("k5_dit_set_skip_guidance: mode must be 0 (block) or 1 (attention), got %d", g->mode); return K5_ERR_ARG; }
  if (!(g->scale >= 0.0f) || !isfinite(g->scale)) { k5_set_error("k5_dit_set_skip_guidance: scale must be finite and >= 0 (got %g)", (double)g->scale); return K5_ERR_ARG; }
  if (g->steps && g->num_steps < 1) { k5_set_error("k5_dit_set_skip_guidance: steps with num_steps = %d", g->num_steps); return K5_ERR_ARG; }
  std::vector<char> skipped((size_t)nb, 0);
  int k0 = nb;
  for (int j = 0; j < g->num_blocks; ++j) {
    const int b = g->blocks[j];
    if (b < 0 || b >= nb) { k5_set_error("k5_dit_set_skip_guidance: block %d is outside 0..%d", b, nb - 1); return K5_ERR_ARG; }
    if (skipped[b]) { k5_set_error("k5_dit_set_skip_guidance: block %d is listed twice", b); return K5_ERR_ARG; }
    skipped[b] = 1;
    k0 = b < k0 ? b : k0;
  }
  sk.skipped.swap(skipped); sk.k0 = k0; sk.mode = g->mode; sk.scale = g->scale;
  sk.steps.assign(g->steps, g->steps ? g->steps + g->num_steps : g->steps);
  sk.on = true;
  return K5_OK;
}

extern "C" int k5_dit_skip_state(k5_dit* d, int* on, long long* skip_steps, long long* blocks_shared, long long* blocks_run, int reset) {
  if (!d) { k5_set_error("k5_dit_skip_state: null handle"); return K5_ERR_ARG; }
  k5_dit::Skip& sk = d->skip;
  if (on) *on = sk.live() ? 1 : 0;
  if (skip_steps) *skip_steps = sk.skip_steps;
  if (blocks_shared) *blocks_shared = sk.blocks_shared;
  if (blocks_run) *blocks_run = sk.blocks_run;
  if (reset) sk.skip_steps = sk.blocks_shared = sk.blocks_run = 0;
  return K5_OK;
}

extern "C" int k5_dit_set_stochastic(k5_dit* d, const k5_stochastic* p) {
  g_err[0] = 0;
  if (!d) { k5_set_error("k5_dit_set_stochastic: null handle"); return K5_ERR_ARG; }
  k5_dit::Stochastic& so = d->sto;
  if (!p) { so.on = false; so.dt_down.clear(); so.scale.clear(); so.coef.clear(); so.seed = 0; so.first_stream = 0; return K5_OK; }
  if (p->num_steps < 1 || !p->dt_down || !p->scale || !p->noise_coef) {
    k5_set_error("k5_dit_set_stochastic: dt_down, scale and noise_coef with num_steps = %d", p->num_steps);
    return K5_ERR_ARG;
  }
  for (int i = 0; i < p->num_steps; ++i) {
    if (!isfinite(p->dt_down[i]) || !isfinite(p->scale[i]) || !isfinite(p->noise_coef[i]) || p->noise_coef[i] < 0.0f) {
      k5_set_error("k5_dit_set_stochastic: step %d: dt_down %g, scale %g, noise_coef %g must be finite and noise_coef >= 0", i, (double)p->dt_down[i],
                   (double)p->scale[i], (double)p->noise_coef[i]);
      return K5_ERR_ARG;
    }
  }
  so.dt_down.assign(p->dt_down, p->dt_down + p->num_steps);
  so.scale.assign(p->scale, p->scale + p->num_steps);
  so.coef.assign(p->noise_coef, p->noise_coef + p->num_steps);
  so.seed = p->seed; so.first_stream = p->first_stream;
  so.on = true;
  return K5_OK;
}

extern "C" int k5_dit_stochastic_state(k5_dit* d, int* on, long long* noisy_steps, int reset) {
  if (!d) { k5_set_error("k5_dit_stochastic_state: null handle"); return K5_ERR_ARG; }
  if (on) *on = d->sto.on ? 1 : 0;
  if (noisy_steps) *noisy_steps = d->sto.noisy_steps;
  if (reset) d->sto.noisy_steps = 0;
  return K5_OK;
}

extern "C" int k5_dit_set_enhance(k5_dit* d, const k5_enhance* e) {
  g_err[0] = 0;
  if (!d) { k5_set_error("k5_dit_set_enhance: null handle"); return K5_ERR_ARG; }
  k5_dit::Enhance& en = d->enh;
  if (!e) { en.on = false; en.weight = 0.f; en.steps.clear(); return K5_OK; }
  if (!(e->weight >= 0.0f) || !isfinite(e->weight)) { k5_set_error("k5_dit_set_enhance: weight must be finite and >= 0 (got %g)", (double)e->weight); return K5_ERR_ARG; }
  if (e->steps && e->num_steps < 1) { k5_set_error("k5_dit_set_enhance: steps with num_steps = %d", e->num_steps); return K5_ERR_ARG; }
  en.weight = e->weight;
  en.steps.assign(e->steps, e->steps ? e->steps + e->num_steps : e->steps);
  en.on = true;
  return K5_OK;
}

extern "C" int k5_dit_enhance_state(k5_dit* d, int* on, long long* launches, float* scores, int cap, int* nblocks, int reset) {
  if (!d) { k5_set_error("k5_dit_enhance_state: null handle"); return K5_ERR_ARG; }
  k5_dit::Enhance& en = d->enh;
  if (scores && cap < 0) { k5_set_error("k5_dit_enhance_state: cap = %d", cap); return K5_ERR_ARG; }
  if (on) *on = en.on ? 1 : 0;
  if (launches) *launches = en.launches;
  if (nblocks) *nblocks = en.last_blocks;
  const int n = en.last_blocks < cap ? en.last_blocks : cap;
  if (scores && n > 0) {   // diagnostic: the last forward's scores, once its stream has drained
    HIPCHK(hipStreamSynchronize(en.last_stream));
    HIPCHK(hipMemcpy(scores, en.scores.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  if (reset) en.launches = 0;
  return K5_OK;
}

extern "C" int k5_dit_forward_skip(k5_dit* d, const k5_forward_args* a, void* out_velocity, void* out_velocity_skip, void* stream) {
  g_err[0] = 0;
  if (!d || !a || !out_velocity || !out_velocity_skip || !a->x) return K5_ERR_ARG;
  ForwardCall f{a, a->cond, a->time, a->x, a->x_channels, out_velocity, (hipStream_t)stream};
  f.out_skip = out_velocity_skip;
  return forward_impl(d, f);
}

extern "C" int k5_dit_nag_state(k5_dit* d, int* on, long long* combines, int reset) {
  if (!d) { k5_set_error("k5_dit_nag_state: null handle"); return K5_ERR_ARG; }
  if (on) *on = d->nag.on ? 1 : 0;
  if (combines) *combines = d->nag.combines;
  if (reset) d->nag.combines = 0;
  return K5_OK;
}

extern "C" int k5_dit_watch_state(k5_dit* d, int* steps_done, int* stopped) {
  if (!d) { k5_set_error("k5_dit_watch_state: null handle"); return K5_ERR_ARG; }
  if (steps_done) *steps_done = d->watch.steps_done;
  if (stopped) *stopped = d->watch.stopped;
  return K5_OK;
}

// S forwards of one (T, H, W), one after another: sequence i is k5_dit_forward on x[i] / conds[i] with the handle as the call found it.
// k5_dit_forward reads and updates the softmax-form memory (AttnW::pref, which decides bits), so every block's memory is saved at entry and
// put back before every sequence after the first and once more at the end.  A block whose memory was not allocated yet holds zeros in
// effect (ensure_zeroed allocates it zeroed), so putting it back means zeroing what a sequence allocated.
extern "C" int k5_dit_forward_many(k5_dit* d, const k5_forward_args* a, int S, const k5_text_cond* conds, void* out_velocity,
                                    void* stream) {
  g_err[0] = 0;
  if (!d || !a) { k5_set_error("k5_dit_forward_many: null handle or arguments"); return K5_ERR_ARG; }
  K5CHK(many_state_ok(d, "k5_dit_forward_many"));
  if (S < 1) { k5_set_error("k5_dit_forward_many: S must be >= 1 (got %d)", S); return K5_ERR_ARG; }
  if (!conds || !out_velocity) { k5_set_error("k5_dit_forward_many: conds / out_velocity missing"); return K5_ERR_ARG; }
  if (!a->x || (reinterpret_cast<uintptr_t>(a->x) & 3)) { k5_set_error("k5_dit_forward_many: x is NULL or not 4-byte aligned"); return K5_ERR_ARG; }
  if (reinterpret_cast<uintptr_t>(out_velocity) & 1) { k5_set_error("k5_dit_forward_many: out_velocity is not 2-byte aligned"); return K5_ERR_ARG; }
  if (a->T <= 0 || a->H <= 0 || a->W <= 0 || a->x_channels <= 0) { k5_set_error("k5_dit_forward_many: bad shapes"); return K5_ERR_ARG; }
  hipStream_t s = (hipStream_t)stream;
  const size_t slot = (size_t)3 * d->Hh * 4;           // AttnW::pref of one block: [3][H] int
  std::vector<char> had(d->vblocks.size(), 0);
  size_t saved = 0;
  for (size_t j = 0; j < d->vblocks.size(); ++j) had[j] = d->vblocks[j].self_attn.pref.p != nullptr;
  for (char h : had) saved += h ? slot : 0;
  if (saved) K5CHK(d->ws_pref_snap.ensure(d->vblocks.size() * slot));
  auto put_back = [&](bool save) -> int {
    for (size_t j = 0; j < d->vblocks.size(); ++j) {
      DevBuf& pref = d->vblocks[j].self_attn.pref;
      if (had[j]) {
        char* snap = static_cast<char*>(d->ws_pref_snap.p) + j * slot;
        HIPCHK(save ? hipMemcpyAsync(snap, pref.p, slot, hipMemcpyDeviceToDevice, s)
                              : hipMemcpyAsync(pref.p, snap, slot, hipMemcpyDeviceToDevice, s));
      } else if (!save && pref.p) HIPCHK(hipMemsetAsync(pref.p, 0, pref.bytes, s));
    }
    return K5_OK;
  };
  K5CHK(put_back(true));
  const size_t thw = (size_t)a->T * a->H * a->W;
  for (int i = 0; i < S; ++i) {
    if (i) K5CHK(put_back(false));
    k5_forward_args one = *a;
    one.x = a->x + (size_t)i * thw * a->x_channels;
    one.cond = conds[i];
    const int st = k5_dit_forward(d, &one, static_cast<bf16_t*>(out_velocity) + (size_t)i * thw * d->cfg.out_visual_dim, stream);
    if (st != K5_OK) {
      if (!g_err[0]) k5_set_error("k5_dit_forward_many: sequence %d failed with status %d", i, st);
      return st;
    }
  }
  return put_back(false);
}

// W8A8 e4m3 feed-forward (BASELINE config 5).  Quantises W1 / W2 of every visual block per output channel on first enable.
extern "C" int k5_dit_set_fp8(k5_dit* d, int enabled) {
  g_err[0] = 0;
  if (!d || !d->finalized) { k5_set_error("k5_dit_set_fp8: handle not finalized"); return K5_ERR_STATE; }
  if (enabled < 0 || enabled > 7) { k5_set_error("k5_dit_set_fp8: a bit mask 0..7 (1 feed-forward, 2 q|k|v projections, 4 out projection)"); return K5_ERR_ARG; }
  if (enabled && ((d->D % 128) || (d->FF % 128) || d->D < 256 || d->FF < 256)) {
    k5_set_error("k5_dit_set_fp8: model_dim and ff_dim must be multiples of 128 and >= 256"); return K5_ERR_UNSUPPORTED;
  }
  // a copy that exists is current (the LoRA paths refresh it) and is kept when its bit goes away: only the mask decides what runs in e4m3
  for (auto& b : d->vblocks) {
    auto ensure_e4m3 = [](Linear& l) { return l.has_e4m3() ? K5_OK : l.quantise(true); };
    if (enabled & 1) { K5CHK(ensure_e4m3(b.w1)); K5CHK(ensure_e4m3(b.w2)); }
    if (enabled & 2) { K5CHK(ensure_e4m3(b.self_attn.wqk)); K5CHK(ensure_e4m3(b.self_attn.wv)); }
    if (enabled & 4) K5CHK(ensure_e4m3(b.self_attn.wo));
  }
  HIPCHK(hipDeviceSynchronize());
  d->fp8_mask = enabled;
  return K5_OK;
}

// ---------------------------------------------------------------------------------------------
// LoRA adapters: merge into the packed weights in place, and undo (include/k5.h)
// ---------------------------------------------------------------------------------------------
namespace {
// lin: the layer the matrix is (a row range of), whose e4m3 copy has to follow the merge; null: one of the fp32 matrices
struct LoraTarget { void* p = nullptr; bool bf16 = true; size_t rows = 0, cols = 0, ld = 0; Linear* lin = nullptr; };

// state_dict weight key -> the packed matrix it went into (k5_dit_finalize / pack_attn).  K5_ERR_KEY: not a key of this layout;
// K5_ERR_UNSUPPORTED: a rank-1 tensor (bias, norm)
int lora_target(k5_dit* d, const std::string& key, LoraTarget& t) {
  bool known = false;
  for (auto& e : d->expected) if (e == key) { known = true; break; }
  if (!known) { k5_set_error("k5_dit_add_lora: %s is not a state_dict key of this model", key.c_str()); return K5_ERR_KEY; }
  const std::string w = ".weight";
  const bool is_weight = key.size() > w.size() && key.compare(key.size() - w.size(), w.size(), w) == 0;
  if (!is_weight || key.find("norm.weight") != std::string::npos) {
    k5_set_error("k5_dit_add_lora: %s is a rank-1 tensor (bias / norm): LoRA applies to linear weights only", key.c_str()); return K5_ERR_UNSUPPORTED;
  }
  const size_t D = d->D, TD = d->TD;
  auto f32 = [&](void* p, size_t rows, size_t cols) { t.p = p; t.bf16 = false; t.rows = rows; t.cols = t.ld = cols; };
  auto mod = [&](size_t off, size_t rows) { f32(d->mod_w.as<float>() + off * TD, rows, TD); };
  // rows [row0, row0 + n) of a layer; n = 0: all of it
  auto lin = [&](Linear& l, size_t row0 = 0, size_t n = 0) {
    t.p = l.w.as<bf16_t>() + row0 * l.ld; t.bf16 = true; t.rows = n ? n : (size_t)l.N; t.cols = l.K; t.ld = l.ld; t.lin = &l;
  };
  if (key == "time_embeddings.in_layer.weight") f32(d->time_w1.p, TD, D);
  else if (key == "time_embeddings.out_layer.weight") f32(d->time_w2.p, TD, TD);
  else if (key == "text_embeddings.in_layer.weight") lin(d->text_lin);
  else if (key == "pooled_text_embeddings.in_layer.weight") lin(d->pool_lin);
  else if (key == "visual_embeddings.in_layer.weight") lin(d->vis_lin);
  else if (key == "out_layer.out_layer.weight") lin(d->out_lin);
  else if (key == "out_layer.modulation.out_layer.weight") mod(d->out_mod_off, 2 * D);
  else {
    const bool text = key.rfind("text_transformer_blocks.", 0) == 0, vis = key.rfind("visual_transformer_blocks.", 0) == 0;
    const size_t pre = text ? strlen("text_transformer_blocks.") : strlen("visual_transformer_blocks.");
    const size_t dot = (text || vis) ? key.find('.', pre) : std::string::npos;
    if (dot == std::string::npos) { k5_set_error("k5_dit_add_lora: no packed matrix for %s", key.c_str()); return K5_ERR_KEY; }
    const int i = atoi(key.substr(pre, dot - pre).c_str());
    auto& blocks = text ? d->tblocks : d->vblocks;
    if (i < 0 || (size_t)i >= blocks.size()) { k5_set_error("k5_dit_add_lora: no packed matrix for %s", key.c_str()); return K5_ERR_KEY; }
    BlockW& b = blocks[i];
    const std::string rest = key.substr(dot + 1);
    if (rest == "text_modulation.out_layer.weight") mod(b.mod_off, 6 * D);
    else if (rest == "visual_modulation.out_layer.weight") mod(b.mod_off, 9 * D);
    else if (rest == "self_attention.to_query.weight") lin(b.self_attn.wqk, 0, D);
    else if (rest == "self_attention.to_key.weight") lin(b.self_attn.wqk, D, D);
    else if (rest == "self_attention.to_value.weight") lin(b.self_attn.wv);
    else if (rest == "self_attention.out_layer.weight") lin(b.self_attn.wo);
    else if (rest == "cross_attention.to_query.weight") lin(b.cross_attn.wq);
    else if (rest == "cross_attention.to_key.weight") lin(b.cross_attn.wk);      // a view into cx_k: the merge writes the stacked memory
    else if (rest == "cross_attention.to_value.weight") lin(b.cross_attn.wv);    // a view into cx_v
    else if (rest == "cross_attention.out_layer.weight") lin(b.cross_attn.wo);
    else if (rest == "feed_forward.in_layer.weight") lin(b.w1);
    else if (rest == "feed_forward.out_layer.weight") lin(b.w2);
    else { k5_set_error("k5_dit_add_lora: no packed matrix for %s", key.c_str()); return K5_ERR_KEY; }
  }
  if (!t.p) { k5_set_error("k5_dit_add_lora: internal: %s is not packed", key.c_str()); return K5_ERR_STATE; }
  return K5_OK;
}

// everything the handle keeps that was computed from the weights as they were
int lora_drop_derived(k5_dit* d) {
  d->drop_text_cache();
  K5CHK(reset_attn_pref(d, nullptr));
  auto& mg = d->mag;
  mg.cnt = mg.first;
  mg.reset_acc(); mg.res_elems[0] = mg.res_elems[1] = 0;
  auto& cl = d->cal;
  if (cl.on) {
    cl.cnt = 0; cl.runs = 0;
    for (int j = 0; j < 2; ++j) { cl.prev[j] = 0; cl.res_elems[j] = 0; }
    HIPCHK(hipMemsetAsync(cl.table.p, 0, (size_t)2 * cl.num_steps * 4 * sizeof(double), nullptr));
  }
  return K5_OK;
}
}  // namespace

extern "C" int k5_dit_add_lora(k5_dit* d, const char* key, const void* A, int a_dtype, const void* B, int b_dtype, int R, float scale) {
  g_err[0] = 0;
  if (!d) { k5_set_error("k5_dit_add_lora: null handle"); return K5_ERR_ARG; }
  if (!d->finalized) { k5_set_error("k5_dit_add_lora before k5_dit_finalize"); return K5_ERR_STATE; }
  if (!key || !A || !B) { k5_set_error("k5_dit_add_lora: null key or factor pointer"); return K5_ERR_ARG; }
  if (R < 1 || R > 256) { k5_set_error("k5_dit_add_lora: rank %d outside 1..256", R); return K5_ERR_ARG; }
  for (int dt : {a_dtype, b_dtype})
    if (dt != K5_F32 && dt != K5_BF16 && dt != K5_F16) { k5_set_error("k5_dit_add_lora: factor dtype %d is none of f32 / bf16 / f16", dt); return K5_ERR_ARG; }
  LoraTarget t;
  K5CHK(lora_target(d, key, t));
  HIPCHK(hipDeviceSynchronize());   // forwards still in flight on other streams read the weights
  const size_t es = t.bf16 ? 2 : 4, bytes = t.rows * t.ld * es;
  if (!d->lora_backup.count(t.p)) {
    k5_dit::LoraBackup bk;
    K5CHK(bk.copy.ensure(bytes));
    HIPCHK(hipMemcpyAsync(bk.copy.p, t.p, bytes, hipMemcpyDeviceToDevice, nullptr));
    bk.bytes = bytes; bk.lin = t.lin;
    d->lora_backup[t.p] = std::move(bk);
  }
  // the factors: device copies of whatever memory they are in (hipMemcpyDefault, as k5_dit_load_tensor)
  DevBuf fa, fb;
  const size_t abytes = (size_t)R * t.cols * (a_dtype == K5_F32 ? 4 : 2), bbytes = t.rows * (size_t)R * (b_dtype == K5_F32 ? 4 : 2);
  K5CHK(fa.ensure(abytes)); K5CHK(fb.ensure(bbytes));
  HIPCHK(hipMemcpy(fa.p, A, abytes, hipMemcpyDefault));
  HIPCHK(hipMemcpy(fb.p, B, bbytes, hipMemcpyDefault));
  K5CHK(k5_launch_lora_merge(t.p, t.bf16 ? K5_BF16 : K5_F32, (int)t.rows, (int)t.cols, (int)t.ld, fa.p, a_dtype, fb.p, b_dtype, R, scale, nullptr));
  if (t.lin) K5CHK(t.lin->quantise(false));   // where k5_dit_set_fp8 made an e4m3 copy, it follows the merged bits
  K5CHK(lora_drop_derived(d));
  HIPCHK(hipDeviceSynchronize());   // fa / fb are freed on return
  return K5_OK;
}

extern "C" int k5_dit_clear_lora(k5_dit* d) {
  g_err[0] = 0;
  if (!d) { k5_set_error("k5_dit_clear_lora: null handle"); return K5_ERR_ARG; }
  if (!d->finalized) { k5_set_error("k5_dit_clear_lora before k5_dit_finalize"); return K5_ERR_STATE; }
  if (d->lora_backup.empty()) return K5_OK;
  HIPCHK(hipDeviceSynchronize());
  for (auto& kv : d->lora_backup)
    HIPCHK(hipMemcpyAsync(kv.first, kv.second.copy.p, kv.second.bytes, hipMemcpyDeviceToDevice, nullptr));
  for (auto& kv : d->lora_backup) if (kv.second.lin) K5CHK(kv.second.lin->quantise(false));
  K5CHK(lora_drop_derived(d));
  HIPCHK(hipDeviceSynchronize());
  d->lora_backup.clear();
  return K5_OK;
}

extern "C" int k5_dit_lora_state(k5_dit* d, int* matrices_touched, long long* backup_bytes) {
  g_err[0] = 0;
  if (!d) { k5_set_error("k5_dit_lora_state: null handle"); return K5_ERR_ARG; }
  long long bytes = 0;
  for (auto& kv : d->lora_backup) bytes += (long long)kv.second.bytes;
  if (matrices_touched) *matrices_touched = (int)d->lora_backup.size();
  if (backup_bytes) *backup_bytes = bytes;
  return K5_OK;
}

extern "C" int k5_dit_set_graph(k5_dit* d, int enabled) { if (!d) return K5_ERR_ARG; d->use_graph = enabled != 0; return K5_OK; }

// ---------------------------------------------------------------------------------------------
// C ABI: sequence parallelism over RCCL
// ---------------------------------------------------------------------------------------------
extern "C" int k5_comm_unique_id(const char* rccl_lib_path, void* out128) {
  g_err[0] = 0;
  if (!out128) return K5_ERR_ARG;
  static Comm probe;  // library handle only
  K5CHK(probe.open(rccl_lib_path));
  ncclUniqueId id;
  const ncclResult_t r = probe.GetUniqueId(&id);
  if (r != ncclSuccess) { k5_set_error("ncclGetUniqueId: %s", probe.GetErrorString(r)); return K5_ERR_HIP; }
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  memcpy(out128, &id, 128);
  return K5_OK;
}

static int comm_common_init(k5_dit* d, int rank, int world) {
  d->comm.rank = rank; d->comm.world = world;
  if (const char* e = getenv("K5_SP_AUTOTUNE")) d->sp_autotune = atoi(e) != 0;   // K5_SP_AUTOTUNE=1: time the admissible exchanges at the first sharded forward (opt-in)
  const char* spm = (d->sp_user_set & 1) ? nullptr : getenv("K5_SP_MODE");
  if (const char* e = spm) {   // K5_SP_MODE=0/1/2: the schedule of "sp_mode" from the launch line (k5_dit_set_option, before or after, wins)
    const int v = atoi(e);
    if (v < 0 || v > 2 || !e[0]) { k5_set_error("K5_SP_MODE must be 0, 1 or 2 (got '%s')", e); return K5_ERR_ARG; }
    d->sp_mode = v; d->sp_user_set |= 1;
  }
  if (d->comm.loop) d->sp_autotune = false;   // loopback ranks (tests of specific schedules on one GPU) tune only when asked to ("sp_autotune" = 1)
  d->sp_rank = rank; d->sp_world = world;
  HIPCHK(hipStreamCreateWithFlags(&d->comm_stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&d->ev_k, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&d->ev_v, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&d->ev_gathered, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&d->ev_stats, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&d->ev_means, hipEventDisableTiming));
  for (auto& e : d->ev_slice) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return K5_OK;
}

extern "C" int k5_dit_comm_init(k5_dit* d, const char* rccl_lib_path, int rank, int world, const void* unique_id128) {
  g_err[0] = 0;
  if (!d || !unique_id128 || world < 1 || rank < 0 || rank >= world) return K5_ERR_ARG;
  if (d->comm.active()) { k5_set_error("communicator already initialised"); return K5_ERR_STATE; }
  K5CHK(d->comm.open(rccl_lib_path));
  ncclUniqueId id;
  memcpy(&id, unique_id128, 128);
  const ncclResult_t r = d->comm.CommInitRank(&d->comm.comm, world, id, rank);
  if (r != ncclSuccess) { k5_set_error("ncclCommInitRank: %s", d->comm.GetErrorString(r)); return K5_ERR_HIP; }
  return comm_common_init(d, rank, world);
}

// CFG-parallel pair (see k5_dit::pair): a 2-rank communicator of its own; branch = this handle's rank in it (0 = conditional forward,
// 1 = unconditional).  Collective over the two handles of the pair; independent of (and initialised after) the sequence-parallel one.
static int pair_common_init(k5_dit* d, int branch) {
  d->pair.rank = branch; d->pair.world = 2; d->cfg_branch = branch;
  HIPCHK(hipStreamCreateWithFlags(&d->pair_stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&d->ev_vel_ready, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&d->ev_vel_done, hipEventDisableTiming));
  return K5_OK;
}
extern "C" int k5_dit_cfg_pair_init(k5_dit* d, const char* rccl_lib_path, int branch, const void* unique_id128) {
  g_err[0] = 0;
  if (!d || !unique_id128 || branch < 0 || branch > 1) return K5_ERR_ARG;
  if (d->pair.active()) { k5_set_error("CFG pair communicator already initialised"); return K5_ERR_STATE; }
  K5CHK(d->pair.open(rccl_lib_path));
  ncclUniqueId id;
  memcpy(&id, unique_id128, 128);
  const ncclResult_t r = d->pair.CommInitRank(&d->pair.comm, 2, id, branch);
  if (r != ncclSuccess) { k5_set_error("ncclCommInitRank (CFG pair): %s", d->pair.GetErrorString(r)); return K5_ERR_HIP; }
  return pair_common_init(d, branch);
}

// ---- loopback group: P handles of one process on one GPU as the P ranks of a sequence-parallel run (tests) ----
struct k5_loopback { LoopGroup g; };
extern "C" int k5_loopback_create(int world, k5_loopback** out) {
  g_err[0] = 0;
  if (!out || world < 1 || world > 64) return K5_ERR_ARG;
  k5_loopback* lb = new k5_loopback();
  lb->g.world = world;
  if (pthread_barrier_init(&lb->g.bar, nullptr, (unsigned)world)) { delete lb; k5_set_error("pthread_barrier_init failed"); return K5_ERR_STATE; }
  lb->g.ptr.assign(world, nullptr); lb->g.joined.assign(world, 0);
  lb->g.ready.resize(world); lb->g.pulled.resize(world);
  for (int i = 0; i < world; ++i) {
    HIPCHK(hipEventCreateWithFlags(&lb->g.ready[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&lb->g.pulled[i], hipEventDisableTiming));
  }
  *out = lb;
  return K5_OK;
}
extern "C" void k5_loopback_destroy(k5_loopback* lb) {
  if (!lb) return;
  for (auto e : lb->g.ready) (void)hipEventDestroy(e);
  for (auto e : lb->g.pulled) (void)hipEventDestroy(e);
  pthread_barrier_destroy(&lb->g.bar);
  delete lb;
}
extern "C" int k5_dit_comm_init_loopback(k5_dit* d, k5_loopback* lb, int rank) {
  g_err[0] = 0;
  if (!d || !lb || rank < 0 || rank >= lb->g.world) return K5_ERR_ARG;
  if (d->comm.active()) { k5_set_error("communicator already initialised"); return K5_ERR_STATE; }
  if (lb->g.joined[rank]) { k5_set_error("loopback rank %d is already taken", rank); return K5_ERR_STATE; }
  lb->g.joined[rank] = 1;
  d->comm.loop = &lb->g;
  return comm_common_init(d, rank, lb->g.world);
}

extern "C" int k5_dit_cfg_pair_init_loopback(k5_dit* d, k5_loopback* lb, int branch) {
  g_err[0] = 0;
  if (!d || !lb || lb->g.world != 2 || branch < 0 || branch > 1) return K5_ERR_ARG;
  if (d->pair.active()) { k5_set_error("CFG pair communicator already initialised"); return K5_ERR_STATE; }
  if (lb->g.joined[branch]) { k5_set_error("loopback pair rank %d is already taken", branch); return K5_ERR_STATE; }
  lb->g.joined[branch] = 1;
  d->pair.loop = &lb->g;
  return pair_common_init(d, branch);
}
extern "C" int k5_dit_cfg_branch(k5_dit* d) { return d && d->pair.active() ? d->cfg_branch : -1; }

// ---- IPC group: one PROCESS per rank, peers' buffers mapped through hipIpc handles, epoch flags in device memory (ipc_comm.h) ----
static int ipc_open(Comm& c, const char* shm_name, int rank, int world) {
  if (c.active()) { k5_set_error("communicator already initialised"); return K5_ERR_STATE; }
  k5ipc::Group* g = new k5ipc::Group();
  if (g->open(shm_name, rank, world)) { k5_set_error("%s", g->err.c_str()); g->close_all(); delete g; return K5_ERR_STATE; }
  c.ipc = g;
  return K5_OK;
}
extern "C" int k5_dit_comm_init_ipc(k5_dit* d, const char* shm_name, int rank, int world) {
  g_err[0] = 0;
  if (!d || !shm_name || world < 1 || world > k5ipc::MAXR || rank < 0 || rank >= world) return K5_ERR_ARG;
  K5CHK(ipc_open(d->comm, shm_name, rank, world));
  K5CHK(comm_common_init(d, rank, world));
  d->sp_autotune = false;   // several ranks may share one device: timings of the candidates would measure the oversubscription
  return K5_OK;
}
extern "C" int k5_dit_cfg_pair_init_ipc(k5_dit* d, const char* shm_name, int branch) {
  g_err[0] = 0;
  if (!d || !shm_name || branch < 0 || branch > 1) return K5_ERR_ARG;
  K5CHK(ipc_open(d->pair, shm_name, branch, 2));
  return pair_common_init(d, branch);
}

// Engine options (all default 0).
//   "attn_mode"       0 = softmax form per head from the data (fixed offset where |q||k'| <= 90, online max elsewhere),
//                     1 = online max everywhere (what a checkpoint with large QK-norm gains gets; bench.py --attn-online)
//   "sp_pass1_tiles"  local key tiles attended before the K/V^T gather has landed (0 = all of the rank's own tiles)
//   "attn_row_offsets" 1 (default) / 0: fixed-offset softmax with per-row offsets — heads whose bound max|q| max|k'| lies in (90, 190]
//                     stay on the fast kernel (a row whose sum underflows sends its head to the online form late); 0 = the plain <= 90 rule
//   "attn_anchor"     1 (default) / 0: heads beyond that window keep the fixed form on offsets anchored at achieved scores (the row's maximum
//                     over a sample of keys + 20; attn_row_anchor_kernel) — no underflow whatever the norms, a job whose row sum
//                     overflows falls back to the online form like an underflowing one; 0 = such heads take the online form (one-GPU path)
//   "attn_pref_reset" (write-only action) forget which heads kept falling back from the per-row-offset form (k5_sample does it at the start of
//                     every call; a caller stepping k5_dit_forward itself does it at the start of a sampling run)
//   "attn_fuse_qnorm" 0 (default): norm_qk + RoPE of the visual queries is a standalone pass; 1 = dense visual self-attention on ONE rank
//                     applies it inside the attention kernel's Q-fragment load (K5QueryNorm; needs attn_row_offsets or attn_mode 1);
//                     2 = under sequence parallelism too.  Measured neutral (elementwise -2.0 ms, attention +0.6 .. +3.4 ms per step
//                     depending on how the compiler schedules the tile loop of the extra instantiation), hence opt-in.
//   "attn_fuse_qnorm_auto" 1 (default) / 0: with attn_fuse_qnorm = 0, k5_sample on a handle without a sequence-parallel communicator decides per call:
//                     step 0 as above (standalone pass) while it records whether any head left the plain fixed-offset form; if none did, steps 1.. run as
//                     attn_fuse_qnorm = 1.  BIT-IDENTICAL either way since round 6 (the two kernels' norm + rotation arithmetic is spelled out operation
//                     for operation: tools/probes/qn_arith_probe.hip); final build, alternating on one box: 522.8-523.1 -> 516.5 ms per step
//                     (elementwise -1.4, attention -4).  "attn_fuse_qnorm_used" (read-only): the last call's decision (1 / 0; -1 = not evaluated)
//   "nabla_group_rows" 0 (default) / 2 / 4: 64-query rows per NABLA key-tile list = per attention workgroup on one GPU; 0 picks 2 (128-query
//                     workgroups) when the previous forward's first map kept less than half of its blocks, else 4; same bits either way
//   "ipc_flags_finegrained" (read-only): 1 when the IPC group's flag page is fine-grained device memory (csrc/ipc_comm.h Group::open; K5_IPC_COARSE_FLAGS=1 forces plain memory)
//   "cross_kv_batched" 1 (default) / 0: the cross-attention key / V^T projections of all visual blocks as two GEMMs against stacked weights before
//                     the visual stack (they depend on the text stream only), their key norms as one launch; same bits as the per-block launches
//   "skip_share_prefix" 1 (default) / 0 (diagnostic): the skip branch of k5_dit_forward_skip starts from the conditional forward's visual stream at the
//                     first skipped block; 0 = it runs every non-skipped block itself from the visual embedding on (the text side is still shared)
//   "nabla_fuse_means" 1 (default: where the launch has >= 150 k threads) / 2 (always) / 0: the 64-token block means NABLA's map is built from are taken by the norm + RoPE pass itself (one read of q | k
//                     less per block, and on one GPU the keys are scaled in place: no scaled copy); same bits as with 0
//   "fp8_fuse_ln"     1 (default) / 0: under k5_dit_set_fp8 the LayerNorm in front of an e4m3 projection writes the e4m3 rows itself (no bf16 h, no
//                     quantisation pass: two passes of N x D less per block); same bits as with 0
//   "nabla_pair_frames" 1 (default) / 0: which two 64-query rows share a 128-query list — the same spatial tile of adjacent frames, or adjacent
//                     tiles of one frame (round 3); same bits, tighter unions under the sliding-tile window (k5_pair_row)
//   "sp_nabla_passes" 1 (default) / 2: NABLA under sequence parallelism walks every list in one pass after the gather, or in two — the
//                     rank's own key blocks while the other ranks' keys travel, the rest after the gather (costs 12 % of the attention
//                     in compute, emulated P = 4; pays when the exposed part of the gather is longer than that — a property of the node)
//   "sp_mode"         0 (default): every rank gathers all K / V^T (any rank count, dense and NABLA); 1: Ulysses — two all-to-alls trade token rows
//                     for heads and back (run_self_attention_heads; needs heads % ranks == 0 and dense attention, else the gather is used);
//                     2: two-level — G = gcd(heads, ranks) head groups x ranks / G query splits (the same routine, two_level; dense attention; G = ranks
//                     runs Ulysses, G = 1 the gather).  K5_SP_MODE=0/1/2 sets it at communicator init; this call still wins.
//   "sp_mode_used"    (read-only) what the last sharded forward ran: 0 gather, 1 Ulysses, 2 two-level (-1: none yet)
//   "sp_autotune"     0 (default since round 5) / 1: the first sharded forward of a handle with more than one rank times one block's self-attention section under
//                     every admissible schedule (all-gather; 2 slices; Ulysses — NABLA: one / two passes) and keeps the fastest (max over ranks; every
//                     rank takes the same decision from the gathered table).  A knob set explicitly through this call is left alone, and a run only assigns
//                     the knobs it varied.  The winner depends on timings and the schedules differ in fp32 summation order: with tuning on, bits may
//                     differ between nodes / runs.  2 = tune again.
//                     k5_dit_sp_schedule returns what was measured and chosen.
//   "sp_slices"       S in 1..4: exchange K / V^T of a block in S slices (grouped send/recv to every peer at once) and attend each
//                     slice as it lands — the gather hides behind the attention of the slices before it (dense attention; NABLA and
//                     S = 1 keep the single in-place all-gather).  Token slots become multiples of 64 S.
//   "emulate_world"   TIMING ONLY, one GPU: lay the work out as rank 0 of a P-rank group while the communicator has one rank —
//                     collectives move nothing, the other ranks' keys are never filled, RESULTS ARE GARBAGE; the handle is
//                     marked (k5_dit_get_option "emulated" = 1) so that a bench can refuse to report it as a measurement
extern "C" int k5_dit_set_option(k5_dit* d, const char* name, int value) {
  g_err[0] = 0;
  if (!d || !name) return K5_ERR_ARG;
  if (!strcmp(name, "attn_mode")) {
    if (value != K5_ATTN_AUTO && value != K5_ATTN_ONLINE) { k5_set_error("attn_mode must be 0 or 1"); return K5_ERR_ARG; }
    d->attn_mode = value; return K5_OK;
  }
  if (!strcmp(name, "sp_pass1_tiles")) { if (value < 0) return K5_ERR_ARG; d->sp_pass1_tiles = value; return K5_OK; }
  if (!strcmp(name, "sp_mode")) { if (value < 0 || value > 2) return K5_ERR_ARG; d->sp_mode = value; d->sp_user_set |= 1; return K5_OK; }
  if (!strcmp(name, "sp_autotune")) { d->sp_autotune = value != 0; if (value > 1) d->sp_tuned = false; return K5_OK; }   // 2 = tune again at the next sharded forward
  if (!strcmp(name, "attn_row_offsets")) { d->row_offsets = value != 0; return K5_OK; }
  if (!strcmp(name, "attn_anchor")) { d->anchor = value != 0; return K5_OK; }
  if (!strcmp(name, "attn_pref_reset")) return reset_attn_pref(d, nullptr, true);   // an action, not a state: the per-step path (k5_dit_forward) calls it per run
  if (!strcmp(name, "cross_kv_batched")) { if (value != 0 && value != 1) return K5_ERR_ARG; d->cross_kv_batched = value; return K5_OK; }
  if (!strcmp(name, "skip_share_prefix")) { if (value != 0 && value != 1) return K5_ERR_ARG; d->skip.share_prefix = value; return K5_OK; }
  if (!strcmp(name, "nabla_fuse_means")) { if (value < 0 || value > 2) return K5_ERR_ARG; d->nabla_fuse_means = value; return K5_OK; }
  if (!strcmp(name, "fp8_fuse_ln")) { if (value != 0 && value != 1) return K5_ERR_ARG; d->fp8_fuse_ln = value; return K5_OK; }
  if (!strcmp(name, "nabla_pair_frames")) { if (value != 0 && value != 1) return K5_ERR_ARG; d->nabla_pair_frames = value; return K5_OK; }
  if (!strcmp(name, "nabla_group_rows")) { if (value != 0 && value != 1 && value != 2 && value != 4) return K5_ERR_ARG; d->nabla_group_rows = value; return K5_OK; }
  if (!strcmp(name, "sp_nabla_passes")) { if (value < 1 || value > 2) return K5_ERR_ARG; d->sp_nabla_passes = value; d->sp_user_set |= 4; return K5_OK; }
  if (!strcmp(name, "attn_fuse_qnorm")) { if (value < 0 || value > 2) return K5_ERR_ARG; d->fuse_qnorm = value; return K5_OK; }
  if (!strcmp(name, "attn_fuse_qnorm_auto")) { if (value != 0 && value != 1) return K5_ERR_ARG; d->fuse_qnorm_auto = value; return K5_OK; }
  if (!strcmp(name, "sp_slices")) {
    if (value < 1 || value > 4) return K5_ERR_ARG;
    if (value > 1 && d->comm.comm && !d->comm.can_exchange()) { k5_set_error("sp_slices > 1 needs ncclSend / ncclRecv / ncclGroup* in the RCCL library"); return K5_ERR_STATE; }
    d->sp_slices = value; d->sp_user_set |= 2; return K5_OK;
  }
  if (!strcmp(name, "emulate_world")) {
    if (!d->comm.active() || d->comm.world != 1 || value < 1) { k5_set_error("emulate_world needs a world = 1 communicator"); return K5_ERR_STATE; }
    d->sp_world = value; d->emulated = value > 1;
    if (d->emulated) fprintf(stderr, "libk5: emulate_world=%d — timing-only layout, the results of this handle are garbage\n", value);
    return K5_OK;
  }
  k5_set_error("unknown option %s", name);
  return K5_ERR_ARG;
}
extern "C" int k5_dit_get_option(k5_dit* d, const char* name, int* value) {
  if (!d || !name || !value) return K5_ERR_ARG;
  if (!strcmp(name, "attn_mode")) *value = d->attn_mode;
  else if (!strcmp(name, "sp_pass1_tiles")) *value = d->sp_pass1_tiles;
  else if (!strcmp(name, "sp_mode")) *value = d->sp_mode;
  else if (!strcmp(name, "sp_mode_used")) *value = d->sp_mode_used;
  else if (!strcmp(name, "sp_slices")) *value = d->sp_slices;
  else if (!strcmp(name, "attn_row_offsets")) *value = d->row_offsets ? 1 : 0;
  else if (!strcmp(name, "attn_anchor")) *value = d->anchor ? 1 : 0;
  else if (!strcmp(name, "attn_fuse_qnorm")) *value = d->fuse_qnorm;
  else if (!strcmp(name, "attn_fuse_qnorm_auto")) *value = d->fuse_qnorm_auto;
  else if (!strcmp(name, "attn_fuse_qnorm_used")) *value = d->fuse_last;
  else if (!strcmp(name, "sp_nabla_passes")) *value = d->sp_nabla_passes;
  else if (!strcmp(name, "sp_autotune")) *value = d->sp_autotune ? 1 : 0;
  else if (!strcmp(name, "sp_tuned")) *value = d->sp_tuned ? 1 : 0;
  else if (!strcmp(name, "fp8_effective")) {   // the classes of k5_dit_set_fp8 that RUN in e4m3 on this handle's path — the sharded schedules keep the out
    int m = d->fp8_mask;                       // projection in bf16 (bit 4), Ulysses also the q | k | V^T projections (bit 2); a bench must label its line with THIS mask
    if (d->comm.active()) { m &= ~4; if (sp_schedule(d, d->last_nabla) != 0) m &= ~2; }   // the dispatch's own predicate (ForwardRun::text_streams: sp_schedule), with the attention type of the LAST forward
    *value = m;
  }
  else if (!strcmp(name, "rccl_ranks")) {   // the size the RCCL communicator reports (ncclCommCount): 0 = no communicator, -1 = a loopback group / no such symbol
    *value = 0;
    if (d->comm.comm && d->comm.CommCount) { int n = 0; *value = d->comm.CommCount(d->comm.comm, &n) == ncclSuccess ? n : -1; }
    else if (d->comm.active()) *value = -1;
  }
  else if (!strcmp(name, "ipc_ranks")) *value = d->comm.ipc ? d->comm.ipc->world : 0;   // processes of the IPC group this handle is a rank of (0 = not that transport)
  else if (!strcmp(name, "ipc_pair_ranks")) *value = d->pair.ipc ? d->pair.ipc->world : 0;
  else if (!strcmp(name, "ipc_collectives")) *value = (int)((d->comm.ipc ? d->comm.ipc->collectives : 0) + (d->pair.ipc ? d->pair.ipc->collectives : 0));
  else if (!strcmp(name, "ipc_pulled_mb")) *value = (int)(((d->comm.ipc ? d->comm.ipc->bytes_pulled : 0) + (d->pair.ipc ? d->pair.ipc->bytes_pulled : 0)) >> 20);
  else if (!strcmp(name, "ipc_flags_finegrained")) *value = (d->comm.ipc && d->comm.ipc->flags_fine) ? 1 : 0;   // the IPC group's flag page is fine-grained device memory
  else if (!strcmp(name, "ipc_errors")) {   // synchronises the device: the first flag wait that ran into its time limit (0 = none; bit 31 | which << 24 | peer << 16 | epoch)
    *value = 0;
    for (Comm* c : {&d->comm, &d->pair}) if (c->ipc) { uint32_t w = 0; if (c->ipc->error_word(&w)) { k5_set_error("%s", c->ipc->err.c_str()); return K5_ERR_HIP; } if (w && !*value) *value = (int)w; }
  }
  else if (!strcmp(name, "nabla_group_rows")) *value = d->nabla_group_rows;
  else if (!strcmp(name, "nabla_pair_frames")) *value = d->nabla_pair_frames;
  else if (!strcmp(name, "fp8_fuse_ln")) *value = d->fp8_fuse_ln;
  else if (!strcmp(name, "nabla_fuse_means")) *value = d->nabla_fuse_means;
  else if (!strcmp(name, "cross_kv_batched")) *value = d->cross_kv_batched;
  else if (!strcmp(name, "skip_share_prefix")) *value = d->skip.share_prefix;
  else if (!strcmp(name, "emulate_world")) *value = d->emulated ? d->sp_world : 0;
  else if (!strcmp(name, "emulated")) *value = d->emulated ? 1 : 0;
  else { k5_set_error("unknown option %s", name); return K5_ERR_ARG; }
  return K5_OK;
}

// How many (block, head) self-attention launches took the fixed-offset / the online-max softmax since the last reset
// (synchronises the device; bench.py reports it as roofline.variant).  reset != 0 clears the counters.
extern "C" int k5_dit_attn_variant_counts(k5_dit* d, long long* fixed_heads, long long* online_heads, int reset) {
  if (!d) return K5_ERR_ARG;
  unsigned long long c[4] = {0, 0, 0, 0};
  if (d->ws_attn_cnt.p) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(c, d->ws_attn_cnt.p, 32, hipMemcpyDeviceToHost));
    if (reset) { HIPCHK(hipMemset(d->ws_attn_cnt.p, 0, 32)); d->nabla_possible = 0; }
  }
  if (fixed_heads) *fixed_heads = (long long)c[0];
  if (online_heads) *online_heads = (long long)c[1];
  return K5_OK;
}
// NABLA maps computed while profiling was on: kept / possible 64x64 blocks since the last k5_dit_attn_variant_counts reset
extern "C" int k5_dit_set_nabla_tap(k5_dit* d, void* dev_u8, long long capacity_bytes) {
  if (!d || capacity_bytes < 0 || (dev_u8 && capacity_bytes == 0)) return K5_ERR_ARG;
  d->nabla_tap = dev_u8; d->nabla_tap_cap = dev_u8 ? capacity_bytes : 0; d->nabla_tap_n = 0;
  return K5_OK;
}
extern "C" int k5_dit_nabla_tap_count(k5_dit* d, long long* maps) {
  if (!d || !maps) return K5_ERR_ARG;
  *maps = d->nabla_tap_n;
  return K5_OK;
}
extern "C" int k5_dit_nabla_block_counts(k5_dit* d, long long* kept, long long* possible) {
  if (!d) return K5_ERR_ARG;
  unsigned long long c[4] = {0, 0, 0, 0};
  if (d->ws_attn_cnt.p) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(c, d->ws_attn_cnt.p, 32, hipMemcpyDeviceToHost));
  }
  if (kept) *kept = (long long)c[2];
  if (possible) *possible = d->nabla_possible;
  return K5_OK;
}
// ... and the blocks the list-driven attention EXECUTED for them: sum of the union lists' lengths x rows per list (one GPU path) — the
// launch's union efficiency is kept / executed
extern "C" int k5_dit_nabla_executed_blocks(k5_dit* d, long long* executed) {
  if (!d || !executed) return K5_ERR_ARG;
  unsigned long long c[4] = {0, 0, 0, 0};
  if (d->ws_attn_cnt.p) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(c, d->ws_attn_cnt.p, 32, hipMemcpyDeviceToHost));
  }
  if (d->comm.active()) { k5_set_error("k5_dit_nabla_executed_blocks: the sharded path does not count its lists"); return K5_ERR_UNSUPPORTED; }
  *executed = (long long)c[3];      // summed on the device per launch as list length x rows of the group (the group size may change between forwards)
  return K5_OK;
}

// What the self-tuning sequence-parallel schedule measured and chose (JSON text; "{}" before the first sharded forward of a multi-rank handle).
// Returns the length of the text; copies at most len - 1 characters + NUL into buf (buf may be null to query the length).
extern "C" int k5_dit_sp_schedule(k5_dit* d, char* buf, int len) {
  if (!d) return K5_ERR_ARG;
  const std::string& r = d->sp_report.empty() ? std::string("{}") : d->sp_report;
  if (buf && len > 0) { const int n = (int)r.size() < len - 1 ? (int)r.size() : len - 1; memcpy(buf, r.data(), (size_t)n); buf[n] = 0; }
  return (int)(d->sp_report.empty() ? 2 : d->sp_report.size());
}
// The selection rule of that tuner as a plain function (tests): times[rank * ncand + cand] in ms (<= 0 or non-finite = did not run), valid
// (nullable) = admissible candidates; returns the chosen candidate or -1, and max-over-ranks per candidate in cost_out (nullable, -1 = out).
// the two-level schedule's exchange plan (sp_plan_2d), for tests without a GPU: table[(src * ranks + dst) * 3 + {0, 1, 2}] = (offset in src's send
// buffer, offset in dst's receive buffer, bytes) of exchange `which` (0 k', 1 V^T, 2 q, 3 o); returns the schedule "sp_mode" 2 runs at this
// (heads, ranks): 2 two-level, 1 Ulysses (G = ranks), 0 the gather (G = 1); G in *groups.  table and groups may be null.
extern "C" int k5_sp_plan_2d(int heads, int ranks, int rows_pad, int dim, int which, int* groups, long long* table) {
  g_err[0] = 0;
  if (ranks < 1 || ranks > 64) return -K5_ERR_ARG;
  std::vector<k5ipc::Xfer> tab((size_t)ranks * ranks);
  const int G = sp_plan_2d(heads, ranks, rows_pad, dim, which, tab.data());
  if (G <= 0 || (dim / G) % 8) { k5_set_error("k5_sp_plan_2d: bad arguments"); return -K5_ERR_ARG; }
  if (groups) *groups = G;
  if (table) for (size_t i = 0; i < tab.size(); ++i) { table[3 * i] = tab[i].send_off; table[3 * i + 1] = tab[i].recv_off; table[3 * i + 2] = tab[i].bytes; }
  return G == 1 ? 0 : (G == ranks ? 1 : 2);
}

extern "C" int k5_sp_pick_schedule(const float* times, int ncand, int world, const int* valid, float* cost_out) {
  if (!times || ncand <= 0 || world <= 0) return -1;
  return sp_pick(times, ncand, world, valid, cost_out);
}

extern "C" int k5_dit_set_profiling(k5_dit* d, int level) { if (!d || level < 0 || level > 2) return K5_ERR_ARG; d->profiling = level; return K5_OK; }
extern "C" int k5_dit_reset_profile(k5_dit* d) { if (!d) return K5_ERR_ARG; drain_profile(d); d->prof.clear(); d->prof_self_blocks = 0; return K5_OK; }
extern "C" int k5_dit_get_profile(k5_dit* d, const char* family, double* total_ms, int64_t* launches) {
  if (!d || !family) return K5_ERR_ARG;
  drain_profile(d);
  if (!strcmp(family, "self_blocks")) {   // not a kernel family: how many visual blocks ran their self-attention under profiling
    if (total_ms) *total_ms = 0.0;
    if (launches) *launches = d->prof_self_blocks;
    return K5_OK;
  }
  auto it = d->prof.find(family);
  if (total_ms) *total_ms = it == d->prof.end() ? 0.0 : it->second.ms;
  if (launches) *launches = it == d->prof.end() ? 0 : it->second.n;
  return K5_OK;
}
