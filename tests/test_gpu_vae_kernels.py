"""GPU parity tests (MI355X) of the VAE decoder's kernels besides the convolutions, through the public C ABI: the C = 512 mid-block
attention (csrc/vae_attn.hip) and the frame-causal softmax and the two GroupNorm forms (csrc/vae_ops.hip), each against a float64
reference of the operation (tests/vae_kernels_reference.py) at the branches, edges and masks where such kernels go wrong:

  attention  the lazy-offset rescale (one hot query per wave; a staircase that triggers in every tile; one that stops 1 short of the
             threshold), exact zeros and per-probability errors read through a one-hot V for S from 1 to 700, small random shapes
  softmax    both sides of every boundary between its four kernels, NaN wherever the score GEMM leaves tiles unwritten, a
             per-probability tolerance, rows with structure; the GEMM - softmax - GEMM chain as the engine runs it
  GroupNorm  every accepted width, M around the statistics block and the apply kernel's block, data with a mean far from 0, a constant
             group; the quad-statistics form on host-made statistics (empty slices, slices longer than the loop stride)

Every output has NaN-pattern guard rows before and after (and guard columns where the row stride exceeds the width) that must come back
untouched; every call is run twice and must give the same bits.  tests/test_vae_kernels_host.py imports the case tables below and
proves on the CPU that each case reaches the path it claims."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from kit import BF, E  # noqa: E402

import vae_kernels_reference as R  # noqa: E402

OK, ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = 0, 1, 2, 6

# ------------------------------------------------------------------------------------------ case tables (shared with the host file)
# (S, hw, gain of the hot queries, seed)
ATTN_RESCALE_CASES = [(160, 160, 32, 1), (200, 48, 32, 1), (333, 100, 24, 1)]
# name -> (S, hw, rise of the score level per 32-key tile in the exp2 domain, seed, gain of the cold queries)
ATTN_STAIR_CASES = {"rising": (128, 128, 45.0, 11, 0.03), "flat39": (128, 128, 13.0, 12, None)}
PROBE_S = (1, 31, 32, 33, 63, 64, 65, 100, 512)
PROBE_CASES = sorted({(S, hw) for S in PROBE_S for hw in (1, 7, 32, 37, S, S + 5)}) + [(700, 100)]
PROBE_SEED = 21
ATTN_RANDOM_CASES = sorted({(S, hw) for S in (1, 33, 65, 130) for hw in (1, 20, S)})
ATTN_RANDOM_SEED = 31
PROBE_LDO = 512 + 8

SOFTMAX_S = (1, 7, 255, 256, 257, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769)
SOFTMAX_SEED = 41


def softmax_hws(S):
    """1; S; S + 3; one value that does not divide S; values that put a row's limit at 1023 / 1024 / 1025 (register kernels) or at
    255 / 256 / 257 (three-pass kernel), where S has such rows"""
    hws = {1, S, S + 3}
    nd = next((h for h in range(max(2, S // 3 + 1), S) if S % h), None)
    if nd is not None:
        hws.add(nd)
    edges = (1023, 1024, 1025) if R.softmax_kernel_of(S) else (255, 256, 257)
    hws.update(h for h in edges if h < S)
    return sorted(hws)


SOFTMAX_CASES = [(S, hw) for S in SOFTMAX_S for hw in softmax_hws(S)]
# (C, S, hw): the engine's GEMM - softmax - GEMM chain; at C = 512 also the one-kernel attention on the same inputs
CHAIN_CASES = [(128, 200, 48), (128, 700, 100), (512, 200, 48), (512, 700, 100)]
CHAIN_SEED = 51

GN_WIDTHS = [(64, 16), (128, 32), (256, 32), (512, 32), (1024, 64), (2048, 64)]


def gn_rows(C):
    B = R.gn_apply_rows_per_block(C)
    return sorted({1, 2, 511, 512, 513, B - 1, B, B + 1, 2100})


GN_CASES = [(M, C, G) for C, G in GN_WIDTHS for M in gn_rows(C)]
GN_QUAD_CASES = [(100, 128, 32), (300, 512, 32), (1100000, 32, 4)]
# seeds of the quad cases whose data the default seed does not suit: the quad entries are fp32, and on the data with a mean of 32 that
# rounding alone moves 0.1 % to 0.5 % of the outputs by a bf16 ulp where a group has one or two entries — against the 0.2 % by which the
# quad form and the two-pass form may differ.  These draws leave half of that to the kernels (the host file asserts it, without a kernel).
GN_QUAD_SEEDS = {(100, 128, 32, "offset"): 1, (300, 512, 32, "offset"): 4}
# (M, C, G) -> status, nothing launched
GN_REFUSALS = [((4, 520, 65), ERR_ARG), ((4, 128, 24), ERR_ARG), ((4, 36, 9), ERR_UNSUPPORTED), ((4, 96, 8), ERR_UNSUPPORTED),
               ((4, 4096, 32), ERR_UNSUPPORTED)]


def ids(v):
    return str(v).replace(" ", "")


_cache = {}


def cached(fn, *key):
    """a case and its reference are built once and shared by the tests that use them (never modified)"""
    k = (fn.__name__,) + tuple(id(a) if isinstance(a, R.NS) else a for a in key)       # a cached case stands for itself
    if k not in _cache:
        _cache[k] = fn(*key)
    return _cache[k]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def assert_within(got, ref, tol, what):
    """|got - ref| <= tol for every element; NaN and inf fail"""
    bad = ~((got.double() - ref).abs() <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.numel()} off, worst {R.worst_share(got, ref, tol):.3f} of the tolerance"


# ------------------------------------------------------------------------------------------ mid-block attention
def run_attention(E, c, ldo=PROBE_LDO, what="k5_vae_attention512_bf16"):
    """q | k interleaved in one [S][1024] buffer as the engine's q|k GEMM leaves them, V^T [512][ceil(S / 32) * 32] with 3e30 in the pad
    columns, the output between guards; run twice into two buffers"""
    S = c.S
    qk = torch.cat([c.q, c.k], 1).to(BF).cuda().contiguous()
    ldvt = (S + 31) // 32 * 32
    vt = torch.full((512, ldvt), 3.0e30, dtype=BF, device="cuda")
    vt[:, :S] = c.v.t().to(BF).cuda()
    outs = []
    for _ in range(2):
        buf, out = R.guarded(S, 512, BF, ldo, device="cuda")
        E.check(E.lib().k5_vae_attention512_bf16(qk.data_ptr(), qk.data_ptr() + 2 * 512, vt.data_ptr(), out.data_ptr(), S, c.hw, 1024, ldvt, ldo,
                                                 c.scale, E.stream_ptr()), what)
        torch.cuda.synchronize()
        assert R.guards_intact(buf, S, 512), what
        outs.append(out)
    assert same_bits(outs[0], outs[1]), what
    return outs[0].float().cpu()


@pytest.mark.parametrize("case", ATTN_RESCALE_CASES, ids=ids)
def test_attention_lazy_offset_rescale_branch(E, case):
    """One hot query per wave (its scores 24 to 32 times the others') makes the wave revise its offsets after the first tile; the cold
    queries of that wave are rescaled by factors down to 2^-30.  The host file shows that a kernel which missed the accumulator in that
    rescale would leave the tolerance in every cold row with a factor <= 1/2."""
    c = cached(R.attn_rescale_case, *case)
    out = run_attention(E, c)
    ref = cached(R.attention_ref_of, c)
    assert_within(out, ref, R.attn_tol(ref), f"attention rescale {case}")


@pytest.mark.parametrize("name", list(ATTN_STAIR_CASES), ids=ids)
def test_attention_staircase_scores(E, name):
    """rising: every tile after the first lifts the hot rows' maximum by 45 (exp2 domain), so every wave rescales three times, and its cold
    rows (levels rising by 1.35) carry every tile's weight through all three.  flat39: 13 per tile, 39 in all — no rescale, unnormalised
    probabilities up to 2^39."""
    c = cached(R.attn_staircase_case, *ATTN_STAIR_CASES[name])
    out = run_attention(E, c, 512)
    ref = cached(R.attention_ref_of, c)
    assert_within(out, ref, R.attn_tol(ref), f"attention staircase {name}")


@pytest.mark.parametrize("S,hw", PROBE_CASES, ids=ids)
def test_attention_mask_and_probabilities_by_probes(E, S, hw):
    """V one-hot: out[i][c] is the probability of key c (at S = 700 plus that of key c + 512).  A masked key contributes exactly 0; every
    other probability is within two bf16 roundings of float64."""
    c = cached(R.attn_probe_case, S, hw, PROBE_SEED)
    out = run_attention(E, c, PROBE_LDO)
    want = cached(R.probe_expected, c)
    zero = R.probe_zero_mask(S, hw)
    assert (out[zero] == 0).all(), f"probe {S},{hw}: {int((out[zero] != 0).sum())} masked keys weigh something"
    assert_within(out, want, R.probe_tol(want), f"probe {S},{hw}")


@pytest.mark.parametrize("S,hw", ATTN_RANDOM_CASES, ids=ids)
def test_attention_small_shapes(E, S, hw):
    c = cached(R.attn_random_case, S, hw, ATTN_RANDOM_SEED)
    out = run_attention(E, c, PROBE_LDO)
    ref = cached(R.attention_ref_of, c)
    assert_within(out, ref, R.attn_tol(ref), f"attention {S},{hw}")


def test_attention_refusals(E):
    """nothing is launched: the status and an untouched output"""
    S = 40
    qk = torch.zeros(S, 1032, dtype=BF, device="cuda")
    vt = torch.zeros(512, 64, dtype=BF, device="cuda")
    buf, out = R.guarded(S, 512, BF, 520, device="cuda")
    f = E.lib().k5_vae_attention512_bf16

    def call(S=S, hw=8, ldqk=1024, ldvt=64, ldo=520):
        return f(qk.data_ptr(), qk.data_ptr() + 1024, vt.data_ptr(), out.data_ptr(), S, hw, ldqk, ldvt, ldo, 0.044, E.stream_ptr())

    assert call(S=0) == ERR_ARG and call(S=-3) == ERR_ARG and call(hw=0) == ERR_ARG and call(hw=-1) == ERR_ARG
    assert call(ldvt=56) == ERR_ALIGN                      # a multiple of 8 below ceil(40 / 32) * 32
    assert call(ldvt=32) == ERR_ALIGN
    assert call(ldqk=1028) == ERR_ALIGN and call(ldo=518) == ERR_ALIGN
    torch.cuda.synchronize()
    assert R.guards_intact(buf, 0, 0)                      # the whole buffer still holds the fill


# ------------------------------------------------------------------------------------------ frame-causal softmax
def softmax_blocks(S):
    step = S if S <= 4096 else 1024
    return [(r0, min(r0 + step, S)) for r0 in range(0, S, step)]


@pytest.mark.parametrize("S,hw", SOFTMAX_CASES, ids=ids)
def test_causal_softmax_boundaries_and_unwritten_scores(E, S, hw):
    """lds != ldp, both > S.  Scores at columns >= the row's limit are NaN (what the frame-causal score GEMM leaves of a NaN-filled
    buffer); P is pre-filled with the NaN pattern and must come back with every one of its ldp columns written, exact zeros from the
    limit on, and every probability within a bf16 half ulp, doubled, of float64."""
    lds, ldp = S + 5, S + 3
    sc = torch.empty(S, lds, device="cuda")
    cols = torch.arange(lds, device="cuda")
    for r0, r1 in softmax_blocks(S):
        rows = torch.arange(r0, r1, device="cuda")
        blk = R.softmax_scores(S, rows, lds, SOFTMAX_SEED, "cuda")
        sc[r0:r1] = blk.masked_fill(cols[None, :] >= R.frame_limit(S, hw, rows)[:, None], float("nan"))
    bufs = []
    for _ in range(2):
        buf, P = R.guarded(S, ldp, BF, device="cuda")
        E.check(E.lib().k5_causal_softmax_bf16(sc.data_ptr(), P.data_ptr(), S, hw, lds, ldp, E.stream_ptr()), "k5_causal_softmax_bf16")
        torch.cuda.synchronize()
        assert guard_rows_intact(buf, S)
        bufs.append(P)
    P = bufs[0]
    assert same_bits(P, bufs[1])
    off = nonzero = 0
    worst = 0.0
    for r0, r1 in softmax_blocks(S):
        rows = torch.arange(r0, r1, device="cuda")
        p64, keep = R.causal_softmax_ref(sc[r0:r1], rows, S, hw, ldp)
        got = P[r0:r1].double()
        off += int((~((got - p64).abs() <= R.softmax_tol(p64))).sum())
        nonzero += int((got[~keep] != 0).sum())
        worst = max(worst, R.worst_share(got, p64, R.softmax_tol(p64)))
    print(f"causal_softmax S {S} hw {hw} (kernel {R.softmax_kernel_of(S) or 'three-pass'}): worst {worst:.3f} of the tolerance")
    assert nonzero == 0, f"{nonzero} values past the frame limit are not exactly 0"
    assert off == 0, f"{off} probabilities off, worst {worst:.3f} of the tolerance"


def guard_rows_intact(buf, rows, guard_rows=3):
    """guards_intact for buffers too large to copy to the host: the guard rows, on the device"""
    bits = buf.view(torch.int16)
    return bool((bits[:guard_rows] == R.NAN16).all()) and bool((bits[guard_rows + rows:] == R.NAN16).all())


def test_causal_softmax_refusals(E):
    S = 16
    sc = torch.zeros(S, 24, device="cuda")
    buf, P = R.guarded(S, 24, BF, device="cuda")
    f = E.lib().k5_causal_softmax_bf16
    assert f(sc.data_ptr(), P.data_ptr(), S, 4, 24, S - 1, E.stream_ptr()) == ERR_ARG          # ldp < S
    assert f(sc.data_ptr(), P.data_ptr(), S, 4, S - 1, 24, E.stream_ptr()) == ERR_ARG          # lds < S
    assert f(sc.data_ptr(), P.data_ptr(), 0, 4, 24, 24, E.stream_ptr()) == ERR_ARG
    assert f(sc.data_ptr(), P.data_ptr(), S, 0, 24, 24, E.stream_ptr()) == ERR_ARG
    torch.cuda.synchronize()
    assert R.guards_intact(buf, 0, 0)


def chain_case(C, S, hw):
    q, k, v = R.attn_inputs(S, CHAIN_SEED + C + S, C)
    return R.NS(S=S, hw=hw, q=q, k=k, v=v, scale=1.0 / math.sqrt(C))


@pytest.mark.parametrize("C,S,hw", CHAIN_CASES, ids=ids)
def test_attention_chain_as_the_engine_runs_it(E, C, S, hw):
    """k5_gemm_bf16_f32out (frame-causal: tiles beyond the limit stay unwritten, here NaN) -> k5_causal_softmax_bf16 -> k5_gemm_bf16
    (P V^T with K = ldp), buffers laid out as vae_engine.hip's mid_attention lays them out.  At C = 512 the one-kernel attention
    runs on the same inputs; both sit within the attention tolerance of float64."""
    L = E.lib()
    c = cached(chain_case, C, S, hw)
    q, k, v, scale = c.q, c.k, c.v, c.scale
    ref = cached(R.attention_ref_of, c)
    ld = (S + 7) // 8 * 8 + 8
    qk = torch.cat([q, k], 1).to(BF).cuda().contiguous()
    vt = torch.zeros(C, ld, dtype=BF, device="cuda")
    vt[:, :S] = v.t().to(BF).cuda()
    outs = []
    for _ in range(2):
        sbuf, sc = R.guarded(S, ld, torch.float32, device="cuda")
        pbuf, P = R.guarded(S, ld, BF, device="cuda")
        obuf, out = R.guarded(S, C, BF, device="cuda")
        E.check(L.k5_gemm_bf16_f32out(qk.data_ptr(), qk.data_ptr() + 2 * C, sc.data_ptr(), S, S, C, 2 * C, 2 * C, ld, scale, hw, E.stream_ptr()),
                "k5_gemm_bf16_f32out")
        E.check(L.k5_causal_softmax_bf16(sc.data_ptr(), P.data_ptr(), S, hw, ld, ld, E.stream_ptr()), "k5_causal_softmax_bf16")
        E.check(L.k5_gemm_bf16(P.data_ptr(), vt.data_ptr(), None, out.data_ptr(), S, C, ld, ld, ld, C, 0, None, 0, None, E.stream_ptr()),
                "k5_gemm_bf16")
        torch.cuda.synchronize()
        assert R.guards_intact(sbuf, S, S) and R.guards_intact(pbuf, S, ld) and R.guards_intact(obuf, S, C)
        lim = R.frame_limit(S, hw)
        assert torch.isfinite(sc.cpu()[:, :S][torch.arange(S)[None, :] < lim[:, None]]).all()          # every score a row reads was written
        outs.append(out)
    assert same_bits(outs[0], outs[1])
    assert_within(outs[0].float().cpu(), ref, R.attn_tol(ref), f"chain C {C} S {S} hw {hw}")
    if C == 512:
        one = run_attention(E, c)
        assert_within(one, ref, R.attn_tol(ref), f"one-kernel attention S {S} hw {hw}")


# ------------------------------------------------------------------------------------------ GroupNorm
def run_groupnorm(E, c, silu, xd=None, quads=None):
    L = E.lib()
    xd = c.x.to(BF).cuda() if xd is None else xd
    gd, bd = c.gamma.cuda(), c.beta.cuda()
    ws = torch.empty(L.k5_groupnorm_workspace_size(c.M, c.G), dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        buf, out = R.guarded(c.M, c.C, BF, device="cuda")
        if quads is None:
            E.check(L.k5_groupnorm_bf16(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr(), c.M, c.C, c.G, 1e-6, silu, ws.data_ptr(),
                                        E.stream_ptr()), "k5_groupnorm_bf16")
        else:
            E.check(L.k5_groupnorm_bf16_quads(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr(), c.M, c.C, c.G, 1e-6, silu,
                                              quads.data_ptr(), ws.data_ptr(), E.stream_ptr()), "k5_groupnorm_bf16_quads")
        torch.cuda.synchronize()
        assert guard_rows_intact(buf, c.M)
        outs.append(out)
    assert same_bits(outs[0], outs[1])
    return outs[0]


def check_groupnorm(c, out, xd, silu, what):
    ref, tol = R.groupnorm_ref(xd.float(), c.gamma, c.beta, c.G, silu)                   # float64 on the device
    bad = ~((out.double() - ref).abs() <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.numel()} off, worst {R.worst_share(out, ref, tol):.3f} of the tolerance"


@pytest.mark.parametrize("data", R.GN_DATA)
@pytest.mark.parametrize("M,C,G", GN_CASES, ids=ids)
def test_groupnorm_widths_rows_and_offsets(E, M, C, G, data):
    c = cached(R.gn_case, M, C, G, data)
    xd = c.x.to(BF).cuda()
    for silu in (0, 1):
        out = run_groupnorm(E, c, silu, xd)
        check_groupnorm(c, out, xd, silu, f"groupnorm {M}x{C}/{G} {data} silu {silu}")


def quad_case(M, C, G, data):
    if M >= 10000:                                                     # (70 MB of activations are not kept)
        return R.gn_case(M, C, G, data)
    return cached(R.gn_case, M, C, G, data, GN_QUAD_SEEDS.get((M, C, G, data)))


@pytest.mark.parametrize("data", R.GN_DATA)
@pytest.mark.parametrize("M,C,G", GN_QUAD_CASES, ids=ids)
def test_groupnorm_from_host_made_quad_statistics(E, M, C, G, data):
    """k5_groupnorm_bf16_quads on statistics made on the host in the layout of include/k5.h: 2 entries per group (14 of the 16
    first-level slices empty), 3 per slice, and 1074 per slice (a second trip of the 1024-entry stride).  Same tolerance as the
    two-pass form, and agreement with it on the same tensor as test_conv_statistics_feed_groupnorm_vs_oracle demands."""
    c = quad_case(M, C, G, data)
    xd = c.x.to(BF).cuda()
    quads = R.quad_stats(xd.float())
    assert quads.numel() * 4 == E.lib().k5_conv3d_stats_size(M, C)
    for silu in (0, 1):
        y = run_groupnorm(E, c, silu, xd, quads)
        check_groupnorm(c, y, xd, silu, f"groupnorm from quads {M}x{C}/{G} {data} silu {silu}")
        y2 = run_groupnorm(E, c, silu, xd)
        d = (y.float() - y2.float()).abs()
        assert d.max().item() <= 2.0 ** -7 * max(1.0, y2.float().abs().max().item()) and (d > 0).float().mean().item() < 2e-3, \
            (float(d.max()), float((d > 0).float().mean()))


@pytest.mark.parametrize("shape,status", GN_REFUSALS, ids=ids)
def test_groupnorm_refusals(E, shape, status):
    L = E.lib()
    M, C, G = shape
    x = torch.zeros(M, C, dtype=BF, device="cuda")
    gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    ws = torch.zeros(max(L.k5_groupnorm_workspace_size(M, G), 1 << 16), dtype=torch.uint8, device="cuda")
    quads = torch.zeros(max(L.k5_conv3d_stats_size(M, C), 64) // 4, device="cuda")
    buf, out = R.guarded(M, C, BF, device="cuda")
    assert L.k5_groupnorm_bf16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), M, C, G, 1e-6, 1, ws.data_ptr(), E.stream_ptr()) == status
    assert L.k5_groupnorm_bf16_quads(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), M, C, G, 1e-6, 1, quads.data_ptr(),
                                     ws.data_ptr(), E.stream_ptr()) == status
    torch.cuda.synchronize()
    assert R.guards_intact(buf, 0, 0)
