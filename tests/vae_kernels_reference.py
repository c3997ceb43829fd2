"""Float64 references of the VAE decoder's hand-written kernels besides the convolutions — the frame-causal softmax and the two GroupNorm
forms of csrc/vae_ops.hip, the C = 512 mid-block attention of csrc/vae_attn.hip — with the seeded inputs of their tests, the tolerances,
the host-made quad statistics, and a float64 model of the attention kernel's lazy softmax offset.

Every reference is written from the definition of the operation (diffusers Attention + prepare_causal_attention_mask, nn.GroupNorm + SiLU)
in float64 and works on whatever device its inputs are on: the large softmax cases are built and checked on the GPU in row blocks, the
CPU-only file evaluates the same functions on samples of their rows.  Inputs come from a CPU generator, or (the softmax scores, up to
32 769^2 of them) from an integer hash of (row, column, seed) that is exact in int64 and so gives the same fp32 values on both devices.

Shared by tests/test_vae_kernels_host.py (the conditions every case claims: which branch of a kernel it reaches, what share of each
tolerance a plain fp32 evaluation already uses, that the offset model with the accumulator rescale left out fails where it should) and
tests/test_gpu_vae_kernels.py (the kernels).  The offset model is only ever run on the CPU."""
import math
from types import SimpleNamespace as NS

import torch

from small_ops_reference import BF, F64, NAN16, NAN32, bfr, guarded, guards_intact, r16  # noqa: F401  (re-exported to the two test files)

LOG2E = 1.4426950408889634


def cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


def frame_limit(S, hw, rows=None, device="cpu"):
    """lim[i] = min(S, (i // hw + 1) * hw): query / row i sees keys / columns j < lim[i] (prepare_causal_attention_mask)"""
    rows = torch.arange(S, device=device) if rows is None else rows
    return ((rows // hw + 1) * hw).clamp(max=S)


# ------------------------------------------------------------------------------------------ tolerances
def attn_tol(ref):
    """tests/test_gpu_vae.py test_mid_block_attention_kernel_c512: bf16 probabilities and outputs on top of the reference"""
    return 2.0 ** -6 * ref.abs() + 6e-3


def probe_tol(p):
    """a probability read through a one-hot V, 2^-7 relative: a bf16 rounding (8 significant bits) moves a value by up to 2^-8 of itself,
    and there are two, of the probability and of the output — see attn_probe_case for what that leaves"""
    return 2.0 ** -7 * p + 2.0 ** -100


def softmax_tol(p):
    """2^-8 relative: the most one bf16 rounding (8 significant bits) can move a value, so the fp32 arithmetic before it has to fit into
    what a rounding falls short of that — an fp32 torch evaluation uses 1e-4 of it before its rounding and 0.996 after (host file);
    2^-120 covers probabilities the fp32 arithmetic flushes to zero"""
    return 2.0 ** -8 * p + 2.0 ** -120


def gn_tol(ref, x, sc, sh):
    """2^-8 of the result (the most its bf16 rounding can move it) plus 256 fp32 roundings of the two terms of y = x * sc + sh"""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -16 * ((x * sc).abs() + sh.abs())


def worst_share(got, ref, tol):
    """max of |got - ref| / tol; anything not finite counts as infinitely far"""
    share = (got.double() - ref).abs() / tol
    share = torch.where(torch.isfinite(share), share, torch.full_like(share, float("inf")))
    return float(share.max()) if share.numel() else 0.0


# ------------------------------------------------------------------------------------------ frame-causal softmax
SOFTMAX_STRUCTURE = ("spike", "equal", "huge")


def softmax_structured_rows(S):
    """row -> kind for S >= 8: the last three rows (most columns valid) and three in the middle"""
    if S < 8:
        return {}
    out = {}
    for base in (S - 3, S // 2 - 1):
        for i, kind in enumerate(SOFTMAX_STRUCTURE):
            out[base + i] = kind
    return out


def _hash24(r, c, seed):
    """24 well-mixed bits of (row, column, seed); every intermediate stays below 2^63, so int64 arithmetic is exact on every device"""
    h = (r * 0x9E3779B1 + c * 0x85EBCA77 + seed * 0x632BE5AB + 0x7F4A7C15) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h = h ^ (h >> 12)
    h = (h * 0x297A2D39) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    return h >> 8


def softmax_scores(S, rows, ncols, seed, device="cpu"):
    """fp32 scores [len(rows)][ncols] of the given rows: uniform on a 2^-20 grid in [-8, 8) from the hash; structured rows get one
    score 120 above the rest (column 0, valid in every row), all scores equal, or scores of magnitude 1e4"""
    rows = torch.as_tensor(rows, dtype=torch.int64, device=device)
    cols = torch.arange(ncols, dtype=torch.int64, device=device)
    u = _hash24(rows[:, None], cols[None, :], seed).float()            # < 2^24: exact
    s = u * 2.0 ** -20 - 8.0
    host_rows = rows.tolist()
    for r, kind in softmax_structured_rows(S).items():
        if r in host_rows:
            _structure(s, host_rows.index(r), kind)
    return s


def _structure(s, i, kind):
    if kind == "spike":
        s[i, 0] += 120.0
    elif kind == "equal":
        s[i] = 2.5
    elif kind == "huge":
        s[i] *= 1250.0


def causal_softmax_ref(scores, rows, S, hw, ncols_out):
    """float64 [len(rows)][ncols_out]: softmax over the columns j < lim(row) of the fp32 scores, exactly 0 elsewhere"""
    lim = frame_limit(S, hw, torch.as_tensor(rows, dtype=torch.int64, device=scores.device))
    cols = torch.arange(ncols_out, device=scores.device)
    keep = cols[None, :] < lim[:, None]
    s = torch.zeros(len(lim), ncols_out, dtype=F64, device=scores.device)
    n = min(ncols_out, scores.shape[1])
    s[:, :n] = scores[:, :n].double()
    s = s.masked_fill(~keep, float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True), keep


def causal_softmax_fp32(scores, rows, S, hw, ncols_out):
    """the same formula in torch fp32 (what a plain fp32 kernel computes before its bf16 rounding)"""
    lim = frame_limit(S, hw, torch.as_tensor(rows, dtype=torch.int64, device=scores.device))
    cols = torch.arange(ncols_out, device=scores.device)
    s = torch.zeros(len(lim), ncols_out, dtype=torch.float32, device=scores.device)
    n = min(ncols_out, scores.shape[1])
    s[:, :n] = scores[:, :n]
    s = s.masked_fill(cols[None, :] >= lim[:, None], float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_kernel_of(S):
    """k5_launch_causal_softmax: values per thread of the register kernel, 0 = the three-pass kernel"""
    return 8 if 4096 < S <= 8192 else 16 if 8192 < S <= 16384 else 32 if 16384 < S <= 32768 else 0


# ------------------------------------------------------------------------------------------ frame-causal attention
def attention_scores64(q, k, scale):
    return (q.double() @ k.double().t()) * scale


def causal_probs_ref(q, k, hw, scale):
    """float64 [S][S] probabilities of softmax(scale q k^T + frame-causal mask)"""
    S = q.shape[0]
    s = attention_scores64(q, k, scale)
    lim = frame_limit(S, hw, device=q.device)
    s = s.masked_fill(torch.arange(S, device=q.device)[None, :] >= lim[:, None], float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def causal_attention_ref(q, k, v, hw, scale):
    return causal_probs_ref(q, k, hw, scale) @ v.double()


def attention_ref_of(c):
    return causal_attention_ref(c.q, c.k, c.v, c.hw, c.scale)


def attn_inputs(S, seed, C=512, q_std=1.5):
    """q, k ~ N(0, q_std^2), v ~ N(0, 1), bf16-valued fp32 [S][C], CPU generator"""
    g = cpu_gen(seed)
    q = bfr(torch.randn(S, C, generator=g) * q_std)
    k = bfr(torch.randn(S, C, generator=g) * q_std)
    v = bfr(torch.randn(S, C, generator=g))
    return q, k, v


def hot_rows(S):
    """one hot query per 16-query wave, at a different lane each wave"""
    i = torch.arange(S)
    return i % 16 == (5 * (i // 16) + 3) % 16


def attn_rescale_case(S, hw, gain, seed):
    q, k, v = attn_inputs(S, seed)
    hot = hot_rows(S)
    q = bfr(torch.where(hot[:, None], q * gain, q))                   # gains are small integers: still bf16-valued
    return NS(S=S, hw=hw, q=q, k=k, v=v, hot=hot, scale=1.0 / math.sqrt(512))


def attn_staircase_case(S, hw, rise, seed, cold_gain=None):
    """rank-1 scores: k_j = beta(tile of j) u + noise, q_i = alpha_i u with u in {-1, +1}^512, so that (exp2 domain) the keys of tile t sit
    near the level rise * t * alpha_i.  alpha = 1, or with cold_gain: 1 on rows i % 4 == 0 and cold_gain elsewhere — rows whose levels rise
    too slowly to trigger anything, and which every trigger of their wave rescales by a factor that matters."""
    g = cpu_gen(seed)
    C = 512
    scale = 1.0 / math.sqrt(C)
    u = (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    per_unit = C * scale * LOG2E                                       # exp2-domain score of alpha * beta = 1
    beta = bfr(torch.arange((S + 31) // 32).float() * (rise / per_unit))
    k = bfr(beta[torch.arange(S) // 32][:, None] * u[None, :] + 0.05 * torch.randn(S, C, generator=g))
    alpha = torch.ones(S)
    if cold_gain is not None:
        alpha = torch.where(torch.arange(S) % 4 == 0, alpha, torch.full((S,), cold_gain))
    q = bfr(alpha[:, None] * u[None, :] + 0.02 * torch.randn(S, C, generator=g))
    v = bfr(torch.randn(S, C, generator=g))
    return NS(S=S, hw=hw, q=q, k=k, v=v, hot=torch.arange(S) % 4 == 0, scale=scale)


def attn_probe_case(S, hw, seed):
    """V is one-hot, v_j = e_(j mod 512): output column c of row i is the probability of key c (plus that of key c + 512).

    q, k ~ N(0, 0.5^2): scores of standard deviation 0.25, a flat softmax.  The reason is the probe tolerance, 2^-7 relative: a bf16
    rounding moves a value by up to 2^-8 of itself (8 significant bits), so the two roundings the tolerance names can use all of it
    and nothing is left for a third term — and there is one, the row sum, which is a sum of ROUNDED probabilities and moves every
    element of its row by sum_k p_k delta_k.  Where one key holds half of the weight that term reaches 2^-9, and the float64 model of
    the kernel already sits at 1.2 times the tolerance (q, k ~ N(0, 1.5^2), measured over these cases); where the weights are
    alike the deltas average out, and the model stays below 1 (tests/test_vae_kernels_host.py asserts it)."""
    q, k, _ = attn_inputs(S, seed, q_std=0.5)
    v = torch.zeros(S, 512)
    v[torch.arange(S), torch.arange(S) % 512] = 1.0
    return NS(S=S, hw=hw, q=q, k=k, v=v, scale=1.0 / math.sqrt(512))


def attn_random_case(S, hw, seed):
    q, k, v = attn_inputs(S, seed)
    return NS(S=S, hw=hw, q=q, k=k, v=v, scale=1.0 / math.sqrt(512))


def probe_expected(c):
    """float64 [S][512]: what a one-hot V makes of the probabilities"""
    p = causal_probs_ref(c.q, c.k, c.hw, c.scale)
    out = torch.zeros(c.S, 512, dtype=F64)
    for b in range(0, c.S, 512):
        n = min(512, c.S - b)
        out[:, :n] += p[:, b:b + n]
    return out


def probe_zero_mask(S, hw):
    """[S][512] True where the output must be exactly 0.0: no key j = c (mod 512) below the row's frame limit"""
    lim = frame_limit(S, hw)
    return torch.arange(512)[None, :] >= lim[:, None]                  # key c itself is the smallest of its residue class


THRESHOLD = 40.0


def attn_offset_model(c, rescale_acc=True, round_p=True):
    """float64 model of vae_attn512_kernel's softmax bookkeeping: workgroups of 64 queries walk the 32-key tiles below the frame limit of
    their last query; each wave of 16 queries keeps an offset per query (exp2 domain).  The first tile sets it to the query's tile
    maximum.  Afterwards, if ANY query of the wave has tile max - offset > 40, EVERY query of the wave takes max(tile max, offset) and
    scales its row sum and its accumulator by 2^(old - new).  Probabilities 2^(s - offset) are rounded to bf16 before the sum and the
    product.  rescale_acc=False leaves the accumulator unscaled (the row sum still is): the mutant a test has to catch.

    Returns (out [S][C] float64, triggers = [(wave's first query, tile)] after the first tile, factor [S] = the smallest single rescale
    factor each row received (1 where none), headroom = max over untriggered tiles of tile max - offset)."""
    S, hw = c.S, c.hw
    s2 = attention_scores64(c.q, c.k, c.scale * LOG2E)
    lim = frame_limit(S, hw)
    s2 = s2.masked_fill(torch.arange(S)[None, :] >= lim[:, None], -1.0e30)
    v = c.v.double()
    out = torch.zeros(S, v.shape[1], dtype=F64)
    factor = torch.ones(S, dtype=F64)
    triggers, headroom = [], -float("inf")
    for q0 in range(0, S, 16):
        q1 = min(q0 + 16, S)
        block_last = min(q0 // 64 * 64 + 63, S - 1)
        T = (int(lim[block_last]) + 31) // 32
        acc = torch.zeros(q1 - q0, v.shape[1], dtype=F64)
        lsum = torch.zeros(q1 - q0, dtype=F64)
        moff = None
        for t in range(T):
            k0, k1 = 32 * t, min(32 * t + 32, S)
            st = s2[q0:q1, k0:k1]
            mx = st.max(-1).values
            if moff is None:
                moff = mx.clone()
            elif bool((mx - moff > THRESHOLD).any()):
                mnew = torch.maximum(mx, moff)
                al = torch.exp2(moff - mnew)
                factor[q0:q1] = torch.minimum(factor[q0:q1], al)
                lsum = lsum * al
                if rescale_acc:
                    acc = acc * al[:, None]
                moff = mnew
                triggers.append((q0, t))
            else:
                headroom = max(headroom, float((mx - moff).max()))
            e = torch.exp2(st - moff[:, None])
            if round_p:
                e = r16(e)
            lsum = lsum + e.sum(-1)
            acc = acc + e @ v[k0:k1]
        out[q0:q1] = acc / lsum[:, None]
    return out, triggers, factor, headroom


# ------------------------------------------------------------------------------------------ GroupNorm (+ SiLU)
GN_DATA = ("wide", "offset", "const_group")
GN_EPS = float(torch.tensor(1e-6, dtype=torch.float32))               # the fp32 value the entry point receives


def gn_case(M, C, G, data, seed=None):
    """x [M][C] bf16-valued: N(0.5, 2^2); N(32, 1) (a mean 32 standard deviations from 0: the single-pass variance cancels five bits);
    or N(0.5, 2^2) with every channel of one group constant at 0.5.  gamma = 1 + 0.2 randn, beta = 0.1 randn."""
    g = cpu_gen(1000 * GN_DATA.index(data) + 7 * M + C + G if seed is None else seed)
    x = torch.randn(M, C, generator=g)
    x = x + 32.0 if data == "offset" else x * 2 + 0.5
    const_g = None
    if data == "const_group":
        const_g = (M + 3) % G
        cg = C // G
        x[:, const_g * cg:(const_g + 1) * cg] = 0.5
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    return NS(M=M, C=C, G=G, data=data, x=bfr(x), gamma=gamma, beta=beta, const_g=const_g)


def group_stats64(x, G):
    """mean and biased variance per group over (M, C / G) in float64, two-pass"""
    M, C = x.shape
    xg = x.double().view(M, G, C // G)
    mean = xg.mean((0, 2))
    var = ((xg - mean[None, :, None]) ** 2).mean((0, 2))
    return mean, var


def groupnorm_ref(x, gamma, beta, G, silu, eps=GN_EPS):
    """nn.GroupNorm(G, C, eps) over channels-last rows [M][C] (+ SiLU) in float64 -> (ref, tolerance)"""
    M, C = x.shape
    mean, var = group_stats64(x, G)
    rstd = 1.0 / torch.sqrt(var + eps)
    cg = C // G
    sc = rstd.repeat_interleave(cg) * gamma.double().to(x.device)
    sh = beta.double().to(x.device) - mean.repeat_interleave(cg) * sc
    x64 = x.double()
    y = (x64 - mean.repeat_interleave(cg)[None, :]) * sc[None, :] + beta.double().to(x.device)[None, :]
    if silu:
        y = y / (1.0 + torch.exp(-y))
    return y, gn_tol(y, x64, sc[None, :], sh[None, :])


def groupnorm_fp32(x, gamma, beta, G, silu, eps=GN_EPS):
    """the same in plain torch fp32 with float64 statistics rounded to fp32: y = fma-free x * sc + sh, SiLU by exp"""
    M, C = x.shape
    mean, var = group_stats64(x, G)
    cg = C // G
    mean32, rstd32 = mean.float(), (1.0 / torch.sqrt(var + eps)).float()
    sc = rstd32.repeat_interleave(cg) * gamma.float()
    sh = beta.float() - mean32.repeat_interleave(cg) * sc
    y = x.float() * sc[None, :] + sh[None, :]
    if silu:
        y = y / (1.0 + torch.exp(-y))
    return y


def quad_stats(x):
    """the statistics the four-wave conv emits, made on the host: [2 ceil(M / 256)][C / 4][2] fp32, entry (b, c) = (sum, sum of squares) of
    rows 128 b .. 128 b + 127 x channels 4 c .. 4 c + 3 in float64, rounded to fp32; rows >= M count nothing (include/k5.h)"""
    M, C = x.shape
    nblk = 2 * ((M + 255) // 256)
    xp = torch.zeros(nblk * 128, C, dtype=F64, device=x.device)
    xp[:M] = x.double()
    xp = xp.view(nblk, 128, C // 4, 4)
    return torch.stack([xp.sum((1, 3)), (xp * xp).sum((1, 3))], -1).float().contiguous()


def quad_rounding_flips(c, silu):
    """share of the bf16 outputs that the fp32 rounding of the quad entries alone moves: GroupNorm in float64 from the (rounded) quad
    statistics against GroupNorm in float64 from the tensor.  No kernel takes part.  On data with mean / sigma = 32 an entry's sum of
    squares is 1025 times the variance's share of it, and its fp32 rounding reaches the outputs."""
    cg = c.C // c.G
    ref, _ = groupnorm_ref(c.x, c.gamma, c.beta, c.G, silu)
    q = quad_stats(c.x).double().sum(0).view(c.G, cg // 4, 2).sum(1)
    mean = q[:, 0] / (c.M * cg)
    var = (q[:, 1] / (c.M * cg) - mean * mean).clamp(min=0)
    sc = (1.0 / torch.sqrt(var + GN_EPS)).repeat_interleave(cg) * c.gamma.double()
    y = (c.x.double() - mean.repeat_interleave(cg)) * sc + c.beta.double()
    if silu:
        y = y / (1.0 + torch.exp(-y))
    return float((r16(y) != r16(ref)).double().mean())


GN_STAT_ROWS, GNQ_SPLIT, GNQ_STRIDE = 512, 16, 1024     # vae_ops.hip: rows per statistics block; first-level slices and their loop stride
GN_TRIP_ROWS = 4                                        # vae_ops.hip GN_LOADS: rows a thread of the statistics pass adds in fp32


def quad_slices(M, C, G):
    """gn_fold_quads_kernel: entries per group and per first-level slice"""
    n = 2 * ((M + 255) // 256) * (C // G // 4)
    return n, [n * (s + 1) // GNQ_SPLIT - n * s // GNQ_SPLIT for s in range(GNQ_SPLIT)]


def gn_apply_rows_per_block(C):
    return 32 * (2048 // C)


def emulate_two_pass_stats(x, G, eps=GN_EPS, long_fp32_runs=False):
    """gn_partial_kernel + gn_finalize_kernel on the CPU: a thread owns one 16-byte chunk column and every rows_par-th row of a 512-row
    block, lower and upper half of the chunk apart.  It adds the values (and their squares — exact in fp32 for bf16 inputs) of one loop
    trip, GN_TRIP_ROWS rows x 4 channels, one by one in fp32; trips, the threads of a group and the blocks are added in double.
    -> (mean, rstd) as fp32.

    long_fp32_runs=True is the accumulation the kernel had before: all of a thread's rows in ONE fp32 run (up to 2048 addends), the
    threads of a group in fp32 as well, the block's sums kept in fp32.  On bf16 data with a large mean such a run stalls: the squares lie
    on a coarse grid, and once the running sum is large enough every other addend ends in exactly half an ulp — a tie, rounded to the
    same side each time."""
    M, C = x.shape
    nch, cg = C // 8, C // G
    rows_par = max(256 // nch, 1)
    nblk = (M + GN_STAT_ROWS - 1) // GN_STAT_ROWS
    xp = torch.zeros(nblk * GN_STAT_ROWS, C)
    xp[:M] = x.float()
    per = GN_STAT_ROWS // rows_par
    xv = xp.view(nblk, per, rows_par, nch, 2, 4)                       # [block][k][rsub][chunk][half][j]: thread (rsub, chunk), k-th row
    acc = torch.float32 if long_fp32_runs else F64
    trip = per if long_fp32_runs else GN_TRIP_ROWS
    s = torch.zeros(nblk, rows_par, nch, 2, dtype=acc)
    q = torch.zeros(nblk, rows_par, nch, 2, dtype=acc)
    for k0 in range(0, per, trip):
        ts_, tq_ = torch.zeros(nblk, rows_par, nch, 2), torch.zeros(nblk, rows_par, nch, 2)
        for k in range(k0, min(per, k0 + trip)):
            for j in range(4):
                val = xv[:, k, :, :, :, j]
                ts_ = ts_ + val
                tq_ = tq_ + val * val
        s, q = s + ts_.to(acc), q + tq_.to(acc)
    if cg == 4:                                                        # the two halves are two groups
        ts, tq = s.reshape(nblk, rows_par, nch * 2), q.reshape(nblk, rows_par, nch * 2)
        per_group = 1
    else:
        ts, tq = s[..., 0] + s[..., 1], q[..., 0] + q[..., 1]
        per_group = cg // 8
    # thread t = rsub * nch + chunk; a group's threads in increasing t: rsub major, chunk minor
    ts = ts.reshape(nblk, rows_par, G, per_group)
    tq = tq.reshape(nblk, rows_par, G, per_group)
    gs, gq = torch.zeros(nblk, G, dtype=acc), torch.zeros(nblk, G, dtype=acc)
    for r in range(rows_par):
        for i in range(per_group):
            gs = gs + ts[:, r, :, i]
            gq = gq + tq[:, r, :, i]
    count = float(M * cg)
    mean = gs.double().sum(0) / count
    var = (gq.double().sum(0) / count - mean * mean).clamp(min=0)
    return mean.float(), (1.0 / torch.sqrt(var + eps)).float()
