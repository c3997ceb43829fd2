"""CPU-only checks of the small-op tests (tests/small_ops_reference.py, tests/test_gpu_small_ops.py), over the GPU file's own case tables:

1. the oracle the GPU tests compare with (oracle/k5_oracle.py, bf16-island arithmetic) sits within HALF of each GPU tolerance of the float64
   reference, so that what a kernel is allowed is not already spent before it runs;
2. every case that claims to go beyond the first trip of a grid-stride loop does, by the launch constants of small_ops.hip;
3. every case tells the true index rule from every mutated rule that can apply to it: the mutated reference differs from the true one by
   more than the GPU tolerance somewhere (at all, for the bit-exact ops) — a kernel that implemented the mutated rule would fail that case;
   a rule that cannot apply to a case changes nothing there;
4. the integer GEMV probes are exact in fp32 in any order of summation.

How 1. is measured.  The distance is taken from the oracle's bf16 value to the float64 value BEFORE its last rounding: the oracle's own last
rounding is part of what it spends — at most half an ulp, which is half of a 1-ulp tolerance by itself — and the rest is its fp32 arithmetic,
which has to fit into half of the absolute term.  Comparing two ROUNDED values instead cannot be made a condition: where the fp32 and the
float64 value straddle a rounding tie the two differ by one whole ulp, 1 / m of a 1-ulp tolerance for a significand m in [1, 2), always more
than half; at 16.8 million elements (gate-sum, 9400 x 1792) that happens 138 times, and in 39 elements of the LayerNorm cases, whatever the
inputs.  The rounded comparison is held to the whole tolerance here."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_ops_reference as R  # noqa: E402
import test_gpu_small_ops as G  # noqa: E402

from oracle import k5_oracle as O  # noqa: E402

BF = torch.bfloat16


def ids(v):
    return str(v).replace(" ", "")


def oracle_within_half(oracle, exact, op, what):
    tol = R.tol_of(op, oracle.double())
    share = float(((oracle.double() - exact).abs() / tol).max())
    print(f"{what}: the oracle uses {share:.3f} of the tolerance")
    assert share <= 0.5, (what, share)
    assert ((oracle.double() - R.r16(exact)).abs() <= tol).all(), what


def tells_apart(true, mutated, op=None):
    """more than the GPU tolerance apart somewhere; for a bit-exact op (op None): different at all"""
    if op is None:
        return not R.same_bits(true, mutated)
    return bool(((mutated - true).abs() > R.tol_of(op, true)).any())


def check_power(family, case, ref, applicable, op=None):
    true = ref(case)
    told = []
    for rule in R.MUTATIONS[family]:
        mutated = ref(case, rule)
        if not applicable(case, rule):
            assert not tells_apart(true, mutated, op) and (op is None or torch.equal(true, mutated)), (family, rule)
            continue
        assert tells_apart(true, mutated, op), (family, rule)
        told.append(rule)
    print(f"{family}: told apart from {', '.join(told) or 'nothing (no rule applies)'}")
    return told


# ------------------------------------------------------------------------------------------ gate-sum
@pytest.mark.parametrize("rows,D", G.GATE_CASES, ids=ids)
def test_gate_sum_case(rows, D):
    c = G.cached(R.gate_case, rows, D)
    assert c.gate.unique().numel() == D                                # gates differ per column
    oracle_within_half(O.gate_sum(c.x, c.y, c.gate, "bf16"), R.gate_sum_ref(c), "gate", f"gate_sum {rows}x{D}")
    told = check_power("gate", c, lambda c, rule=None: R.r16(R.gate_sum_ref(c, rule)), R.gate_applicable, "gate")
    beyond = rows * (D // 8) > R.GRID_FOR_BLOCKS * R.THREADS          # one thread per 16-byte chunk
    assert beyond == ((rows, D) == G.GATE_CASES[-1]) and beyond == ("gate_trip_local" in told)


# ------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("rows,D", G.LN_CASES, ids=ids)
def test_layer_norm_case(rows, D):
    c = G.cached(R.ln_case, rows, D)
    assert list(c.edge) == list(R.LN_EDGE_ROWS[:max(min(rows - 1, 5), 0)])
    if rows >= 6:
        x = c.x
        assert (x[c.edge["const"]] == 1.5).all() and not x[c.edge["zero"]].any() and 39 < float(x[c.edge["offset"]].mean()) < 41
        assert float(x[c.edge["small"]].abs().max()) < 1e-2 and float(x[c.edge["large"]].abs().max()) > 5e3
    oracle_within_half(G.ln_oracle_modulate(rows, D), R.ln_modulate_ref(c), "ln", f"ln_modulate {rows}x{D}")
    oracle_within_half(G.ln_oracle_affine(rows, D), R.ln_affine_ref(c), "ln", f"ln_affine {rows}x{D}")


# ------------------------------------------------------------------------------------------ RMSNorm + RoPE
@pytest.mark.parametrize("case", G.NORM_CASES, ids=ids)
def test_norm_case(case):
    c = G.cached(R.norm_case, *case)
    rows, H = c.rows, c.H
    oracle_within_half(G.norm_oracle_plain(*case), R.norm_rope_ref(c, last_rounding=False), "norm", f"rmsnorm_rope {case}")
    told = check_power("norm", c, R.norm_rope_ref, R.norm_applicable, "norm")
    unit = 8 * H // math.gcd(R.THREADS, 8 * H)
    cap = R.NORM_BLOCKS // unit * unit                                 # blocks of 256 threads; 8 threads per head vector
    beyond = rows * H * 8 > cap * R.THREADS
    assert beyond == (case in G.NORM_TRIP_CASES)
    assert R.norm_trip_rows(H) == (cap * R.THREADS // (8 * H), cap)
    if beyond and c.rope_heads > 0:
        assert "cs_row_lag" in told and "cs_row_mod" in told
    if c.G > 1:
        assert len({tuple(w.tolist()) for w in c.weight}) == c.G and "group_mod" in told and "group_ignored" in told
    if c.cos is not None:
        assert c.cos.unique(dim=0).shape[0] > rows // 2                # tables differ per row
    y = R.norm_rope_ref(c)
    assert torch.isfinite(y).all() and not y.view(rows, H, 64)[0, 0].any()            # the all-zero head vector stays zero


def test_norm_case_with_scaled_heads():
    c = G.cached(R.norm_case, *G.STATS_CASE)
    sf = G.STATS_SCALE_FROM
    exact = R.norm_rope_ref(c, None, O.SOFTMAX_C, sf, last_rounding=False)
    oracle_within_half(G.norm_oracle_scaled(*G.STATS_CASE), exact, "norm", "rmsnorm_rope with scaled heads")
    assert c.rows * c.H * 8 > R.norm_trip_rows(c.H)[1] * R.THREADS and 0 < sf < c.H
    plain, scaled = R.norm_rope_ref(c), R.norm_rope_ref(c, None, O.SOFTMAX_C, sf)
    assert torch.equal(plain.view(c.rows, c.H, 64)[:, :sf], scaled.view(c.rows, c.H, 64)[:, :sf])
    assert tells_apart(scaled, plain, "norm")                          # a kernel that forgot the scale would fail
    # the row of the NaN test lies on the second trip
    assert c.rows - 7 >= R.norm_trip_rows(c.H)[0]


# ------------------------------------------------------------------------------------------ fp32 GEMV
@pytest.mark.parametrize("N,K", G.GEMV_INT_CASES, ids=ids)
def test_gemv_integer_probes_are_exact_in_fp32(N, K):
    for has_b in (0, 1):
        for has_add in (0, 1):
            c = G.cached(R.gemv_int_case, N, K, has_b, has_add)
            assert R.gemv_int_bound(c) < 2 ** 24
            assert int(c.x.abs().max()) <= 8 and int(c.W.abs().max()) <= 8
            want, _ = R.gemv_ref(c.x, c.W, c.b, c.add)
            fp32 = c.W.float() @ c.x.float() + (0 if c.b is None else c.b.float()) + (0 if c.add is None else c.add.float())
            assert torch.equal(fp32.double(), want)
    c = G.cached(R.gemv_int_case, N, K, 1, 1)
    full = R.gemv_ref(c.x, c.W, c.b, c.add)[0]
    for b, add in ((None, c.add), (c.b, None), (None, None)):         # a dropped bias or addend shows
        assert not torch.equal(full, R.gemv_ref(c.x, c.W, b, add)[0])


@pytest.mark.parametrize("N,K", G.GEMV_SILU_CASES, ids=ids)
def test_gemv_silu_reference_agrees_with_the_oracle(N, K):
    c = G.cached(R.gemv_silu_case, N, K)
    want, mag = R.gemv_ref(c.x, c.W, c.b, c.add, silu=True)
    sd = {"m.out_layer.weight": c.W, "m.out_layer.bias": c.b}
    oracle = O.modulation(sd, "m", c.x[None])[0] + c.add
    share = float(((oracle.double() - want).abs() / R.gemv_silu_tol(K, mag)).max())
    print(f"gemv silu {N}x{K}: the oracle uses {share:.3f} of the bound")
    assert share <= 0.5


# ------------------------------------------------------------------------------------------ sinusoids
def angle_share(a32, a64):
    tol = R.angle_tol(a64)
    return float(torch.maximum((torch.cos(a32).double() - torch.cos(a64)).abs() / tol, (torch.sin(a32).double() - torch.sin(a64)).abs() / tol).max())


@pytest.mark.parametrize("t", G.TIME_T)
@pytest.mark.parametrize("D", G.TIME_D)
def test_time_feature_angles(D, t):
    """O.get_freqs (fp32, as the model computes it) against the float64 angles, at half of 2e-6 + |a| 2^-21.

    The float64 frequencies are those of the model's fp32 exponent argument (small_ops_reference.freqs64 says why): what is left to the
    oracle is its fp32 exp and product, 0.19 of the tolerance at most.  Against the mathematical frequencies (argument in float64 too)
    the same oracle uses 0.547 at D = 1792, t = 731.25 and 0.693 at t = 1000 — the fp32 argument alone, which the tolerance's derivation
    (angle rounding |a| 2^-24 and a few ulps of expf) does not count; the whole tolerance still covers it, and is held to it here."""
    a32 = torch.outer(torch.tensor([t], dtype=torch.float32), O.get_freqs(D // 2))[0]
    share = angle_share(a32, R.time_angles(t, D))
    print(f"time features D {D} t {t}: the oracle uses {share:.3f} of the tolerance")
    assert share <= 0.5
    assert angle_share(a32, R.time_angles(t, D, exact=True)) <= 1.0


@pytest.mark.parametrize("case", G.ROPE_CASES, ids=ids)
def test_rope_table_case(case):
    c = G.cached(R.rope_case, *case[0], *case[1:])
    a64 = G.cached(R.rope_angles_ref, c)
    assert sum(c.axes) == 32 and all(int(v.max()) <= 127 and not torch.equal(v, torch.arange(v.numel()).int()) for v in c.pos)
    a32 = O.rope_3d_args((c.T, c.H, c.W), c.pos, tuple(2 * n for n in c.axes), c.scales).reshape(-1, 32)[c.perm.long()]
    share = angle_share(a32, a64)
    print(f"rope table {case}: the oracle uses {share:.3f} of the tolerance")
    assert share <= 0.5
    assert angle_share(a32, R.rope_angles_ref(c, exact=True)) <= 1.0                # the mathematical frequencies: the whole tolerance
    if c.perm_kind == "fractal":
        assert torch.equal(c.perm.long(), O.fractal_perm((c.T, c.H, c.W)))
    assert not torch.equal(torch.argsort(c.perm.long()), c.perm.long())             # not an involution
    tol = R.angle_tol(a64)
    for rule in R.MUTATIONS["rope_table"]:
        am = R.rope_angles_ref(c, rule)
        apart = bool((((torch.cos(am) - torch.cos(a64)).abs() > tol) | ((torch.sin(am) - torch.sin(a64)).abs() > tol)).any())
        assert apart == R.rope_applicable(c, rule), rule                              # (equal scales on axes 1 and 2: that rule cannot show)


# ------------------------------------------------------------------------------------------ patchify / unpatchify
@pytest.mark.parametrize("case", G.PATCH_CASES, ids=ids)
def test_patchify_case(case):
    c = G.cached(R.patch_case, *case, 7000 + G.PATCH_CASES.index(case))
    Hp, Wp, n = c.H // 2, c.W // 2, c.T * (c.H // 2) * (c.W // 2)
    assert c.H != c.W or c.perm is not None
    full = torch.zeros(c.T, c.H, c.W, c.Cin)
    full[..., :c.Cx] = c.x
    if c.vc is not None:
        full[..., c.Cx:] = c.vc
    tok = O.patchify(full, (1, 2, 2)).reshape(n, 4 * c.Cin)
    if c.perm is not None:
        tok = tok[(O.fractal_perm((c.T, Hp, Wp)) if c.perm_kind == "fractal" else c.perm.long())]
        assert not torch.equal(torch.argsort(c.perm.long()), c.perm.long())         # not an involution
    want = torch.zeros(n, c.Kpad)
    want[:, :4 * c.Cin] = tok
    assert R.same_bits(G.cached(R.patchify_ref, c), want.to(BF))
    told = check_power("patchify", c, R.patchify_ref, R.patch_applicable)
    assert (n * c.Kpad > R.GRID_FOR_BLOCKS * R.THREADS) == (case in G.PATCH_TRIP_CASES)   # one thread per output element
    assert ("perm_inverse" in told) == (c.perm is not None)


@pytest.mark.parametrize("case", G.UNPATCH_CASES, ids=ids)
def test_unpatchify_case(case):
    c = G.cached(R.unpatch_case, *case, 8000 + G.UNPATCH_CASES.index(case))
    n, F = c.T * c.Hp * c.Wp, 4 * c.C
    assert c.Hp != c.Wp or c.perm is not None
    assert c.ldx == F or torch.isnan(c.x[:, F:].float()).all()                      # NaN in the pad columns of x
    raster = torch.zeros(n, F)
    raster[torch.arange(n) if c.perm is None else c.perm.long()] = c.x[:, :F].float()
    want = O.unpatchify(raster.reshape(c.T, c.Hp, c.Wp, F), (1, 2, 2))
    got = G.cached(R.unpatchify_ref, c)
    assert R.same_bits(got, want.to(BF)) and torch.isfinite(got.float()).all()
    told = check_power("unpatchify", c, R.unpatchify_ref, R.patch_applicable)
    assert (n * F > R.GRID_FOR_BLOCKS * R.THREADS) == (case in G.UNPATCH_TRIP_CASES)
    assert ("ldx_4c" in told) == (c.ldx != F) and ("perm_inverse" in told) == (c.perm is not None)


def test_guard_helpers_see_one_changed_bit():
    for dtype in (BF, torch.float32):
        buf, view = R.guarded(4, 16, dtype, 24)
        view.zero_()
        assert R.guards_intact(buf, 4, 16)
        for r, col in ((0, 0), (2, 23), (3, 16), (9, 5)):
            b2 = buf.clone()
            b2[r, col] = float("nan")                                  # another NaN than the fill: only the bits tell
            assert not R.guards_intact(b2, 4, 16), (dtype, r, col)
    with pytest.raises(AssertionError):
        R.assert_bf16_close(torch.tensor([float("nan")]), torch.tensor([float("nan")]), 2, 1e-4)
    with pytest.raises(AssertionError):
        R.assert_bf16_close(torch.tensor([float("inf")]), torch.tensor([float("inf")]), 2, 1e-4)
