"""CPU-only checks of the VAE kernel tests (tests/vae_kernels_reference.py, tests/test_gpu_vae_kernels.py), over the GPU file's own case tables:

1. attention: a float64 model of the kernel's lazy softmax offset (64-query blocks, 16-query waves, 32-key tiles, threshold 40 in the
   exp2 domain, bf16 probabilities) says how often each case makes a wave revise its offsets and by what factors; the model stays inside
   the tolerance, and the same model with the accumulator left out of the rescale leaves it in every cold row whose factor is <= 1/2;
   the staircases trigger in every tile, or never; the probes' zero pattern covers every masked key and every column >= S;
2. softmax: every S lies on the side of a kernel boundary it claims, the hw values put row limits where they claim, and an fp32 torch
   evaluation of the same formula uses a small share of the per-probability tolerance on the rows with structure and at the edges;
3. GroupNorm: the widths reach the branches they claim, an fp32 evaluation uses at most half of the tolerance, an emulation of the
   two-pass kernel's fp32 partial sums keeps the error of rstd below 2^-12 on the data with a mean 32 deviations from 0, a constant
   group comes out as beta, and the quad cases have the entry counts per slice they claim.

Every figure is printed (pytest -s)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_kernels_reference as R  # noqa: E402
import test_gpu_vae_kernels as G  # noqa: E402

ids = G.ids


def out_of_tolerance_rows(out, ref):
    return ((out - ref).abs() > R.attn_tol(ref)).any(-1)


# ------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("case", G.ATTN_RESCALE_CASES, ids=ids)
def test_attention_rescale_case_reaches_the_branch(case):
    c = G.cached(R.attn_rescale_case, *case)
    ref = G.cached(R.attention_ref_of, c)
    out, triggers, factor, _ = R.attn_offset_model(c)
    mutant = R.attn_offset_model(c, rescale_acc=False)[0]
    cold = ~c.hot & (factor <= 0.5)
    share = R.worst_share(out, ref, R.attn_tol(ref))
    print(f"attention rescale {case}: {len(triggers)} triggers after the first tile, {int(cold.sum())} cold rows rescaled by <= 1/2 "
          f"(smallest factor 2^{float(torch.log2(factor[~c.hot].min())):.1f}); the model uses {share:.3f} of the tolerance, "
          f"the mutant leaves it in {int(out_of_tolerance_rows(mutant, ref).sum())} rows")
    assert int(c.hot.sum()) == (c.S + 15) // 16 or int(c.hot.sum()) == c.S // 16         # one hot query per (whole) wave
    assert len(triggers) >= 2 and int(cold.sum()) >= 10
    assert share <= 1.0
    assert out_of_tolerance_rows(mutant, ref)[cold].all()


def test_attention_plain_random_inputs_never_rescale():
    """what the older test draws (q, k ~ N(0, 1.5^2)) never leaves the 2^40 window after the first tile: the reason for the cases above"""
    for S, hw in ((1000, 37), (640, 640)):
        q, k, v = R.attn_inputs(S, S + hw)
        _, triggers, _, headroom = R.attn_offset_model(R.NS(S=S, hw=hw, q=q, k=k, v=v[:, :8], scale=512 ** -0.5))
        print(f"plain random S {S} hw {hw}: {len(triggers)} triggers, largest tile max - offset {headroom:.1f}")
        assert not triggers


@pytest.mark.parametrize("name", list(G.ATTN_STAIR_CASES), ids=ids)
def test_attention_staircase_case(name):
    c = G.cached(R.attn_staircase_case, *G.ATTN_STAIR_CASES[name])
    ref = G.cached(R.attention_ref_of, c)
    out, triggers, factor, headroom = R.attn_offset_model(c)
    share = R.worst_share(out, ref, R.attn_tol(ref))
    waves = range(0, c.S, 16)
    per_wave = [sum(1 for q0, _ in triggers if q0 == w) for w in waves]
    s2 = R.attention_scores64(c.q, c.k, c.scale * R.LOG2E)
    span = float((s2.max(-1).values - s2[:, :32].max(-1).values).max())
    print(f"staircase {name}: triggers per wave {per_wave}, largest untriggered tile max - offset {headroom:.2f}, largest score above the "
          f"first tile's maximum 2^{span:.2f}; the model uses {share:.3f} of the tolerance")
    assert share <= 1.0
    if name == "rising":
        assert min(per_wave) >= 3
        mutant = R.attn_offset_model(c, rescale_acc=False)[0]
        cold = ~c.hot & (factor <= 0.5)
        assert int(cold.sum()) == int((~c.hot).sum())                  # every cold row takes part ...
        assert out_of_tolerance_rows(mutant, ref)[cold].all()          # ... and would show a missed accumulator
    else:
        assert not triggers and 38.0 <= span and headroom <= 39.9      # no rescale although probabilities reach 2^38 and more


@pytest.mark.parametrize("S,hw", G.PROBE_CASES, ids=ids)
def test_attention_probe_case(S, hw):
    c = G.cached(R.attn_probe_case, S, hw, G.PROBE_SEED)
    want = G.cached(R.probe_expected, c)
    zero = R.probe_zero_mask(S, hw)
    lim = R.frame_limit(S, hw)
    assert zero[:, S:].all() and (want[zero] == 0).all() and (want[~zero] > 0).all()
    assert all(int(lim[i]) == min(S, (i // hw + 1) * hw) for i in range(S))
    assert torch.allclose(want.sum(-1), torch.ones(S, dtype=R.F64), rtol=0, atol=1e-12)
    model = R.r16(R.attn_offset_model(c)[0])                           # the kernel's two roundings on float64 arithmetic
    assert (model[zero] == 0).all()
    share = R.worst_share(model, want, R.probe_tol(want))
    print(f"probe S {S} hw {hw}: {int(zero.sum())} exact zeros; two bf16 roundings use {share:.3f} of the tolerance")
    assert share <= 1.0


@pytest.mark.parametrize("S,hw", G.ATTN_RANDOM_CASES, ids=ids)
def test_attention_small_shape_case(S, hw):
    c = G.cached(R.attn_random_case, S, hw, G.ATTN_RANDOM_SEED)
    ref = G.cached(R.attention_ref_of, c)
    share = R.worst_share(R.r16(R.attn_offset_model(c)[0]), ref, R.attn_tol(ref))
    print(f"attention S {S} hw {hw}: the model uses {share:.3f} of the tolerance")
    assert share <= 0.5


# ------------------------------------------------------------------------------------------ softmax
def test_softmax_cases_sit_on_both_sides_of_every_kernel_boundary():
    kern = {S: R.softmax_kernel_of(S) for S in G.SOFTMAX_S}
    assert [kern[S] for S in (4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769)] == [0, 8, 8, 16, 16, 32, 32, 0]
    assert all(kern[S] == 0 for S in (1, 7, 255, 256, 257))
    for S in G.SOFTMAX_S:
        hws = G.softmax_hws(S)
        assert {1, S, S + 3} <= set(hws) and (S < 3 or any(S % h for h in hws if h < S))
        lims = {int(v) for hw in hws for v in R.frame_limit(S, hw, torch.arange(0, S, max(1, hw))).tolist()}
        for edge in ((1023, 1024, 1025) if kern[S] else (255, 256, 257)):
            assert (edge in lims) == (edge <= S), (S, edge)
        assert S + 5 != S + 3                                         # lds != ldp, both > S (the GPU test's strides)


def softmax_sample_rows(S, hw):
    rows = {0, S - 1, S // 3} | set(R.softmax_structured_rows(S))
    for edge in (255, 256, 257, 1023, 1024, 1025):
        rows |= {r for r in (edge - 1, (edge // hw) * hw - 1, edge // hw * hw) if 0 <= r < S}
    return sorted(r for r in rows if 0 <= r < S)


@pytest.mark.parametrize("S", G.SOFTMAX_S)
def test_softmax_fp32_evaluation_uses_a_small_share(S):
    worst = worst16 = 0.0
    for hw in G.softmax_hws(S):
        rows = softmax_sample_rows(S, hw)
        sc = R.softmax_scores(S, rows, S + 5, G.SOFTMAX_SEED)
        p64, keep = R.causal_softmax_ref(sc, rows, S, hw, S + 3)
        p32 = R.causal_softmax_fp32(sc, rows, S, hw, S + 3)
        tol = R.softmax_tol(p64)
        assert (p64[~keep] == 0).all() and (p32[~keep] == 0).all()
        assert torch.allclose(p64.sum(-1), torch.ones(len(rows), dtype=R.F64), rtol=0, atol=1e-12)
        worst = max(worst, R.worst_share(p32, p64, tol))
        worst16 = max(worst16, R.worst_share(p32.to(R.BF), p64, tol))
    kinds = R.softmax_structured_rows(S)
    if kinds:                                                          # the structure is what it claims
        rows = sorted(kinds)
        sc = R.softmax_scores(S, rows, S, G.SOFTMAX_SEED)
        for i, r in enumerate(rows):
            rest = sc[i, 1:] if S > 1 else sc[i]
            if kinds[r] == "spike":
                assert float(sc[i, 0] - rest.max()) >= 104.0
            elif kinds[r] == "equal":
                assert (sc[i] == 2.5).all()
            else:
                assert float(sc[i].abs().max()) > 5e3
    print(f"softmax S {S}: fp32 torch uses {worst:.4f} of the tolerance before its bf16 rounding, {worst16:.3f} after it")
    assert worst <= 0.5 and worst16 <= 1.0


def test_softmax_scores_are_the_same_numbers_wherever_they_are_made():
    a = R.softmax_scores(300, torch.arange(300), 305, 7)
    b = torch.cat([R.softmax_scores(300, torch.arange(r, min(r + 64, 300)), 305, 7) for r in range(0, 300, 64)])
    assert torch.equal(a, b) and float(a[:140].min()) >= -8.0 and float(a[:140].max()) < 8.0 and a[:140].unique().numel() > 40000
    assert not torch.equal(a, R.softmax_scores(300, torch.arange(300), 305, 8))


# ------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("C,G_", G.GN_WIDTHS, ids=ids)
def test_groupnorm_width_reaches_its_branch_and_fp32_uses_half(C, G_):
    cg, nch = C // G_, C // 8
    rows_par = 256 // nch
    assert cg >= 4 and cg & (cg - 1) == 0 and nch & (nch - 1) == 0 and nch <= 256 and G_ <= 64
    assert (cg == 4) == ((C, G_) in ((64, 16), (128, 32)))             # two groups per 16-byte chunk
    assert rows_par == {64: 32, 128: 16, 256: 8, 512: 4, 1024: 2, 2048: 1}[C]            # rows per pass of a 256-thread block
    B = R.gn_apply_rows_per_block(C)
    assert B == 32 * rows_par and {1, 2, 511, 512, 513, B - 1, B, B + 1, 2100} == set(G.gn_rows(C))
    worst = 0.0
    for M in G.gn_rows(C):
        if M * C > 1100000:
            continue
        for data in R.GN_DATA:
            c = G.cached(R.gn_case, M, C, G_, data)
            for silu in (0, 1):
                ref, tol = R.groupnorm_ref(c.x, c.gamma, c.beta, G_, silu)
                worst = max(worst, R.worst_share(R.groupnorm_fp32(c.x, c.gamma, c.beta, G_, silu), ref, tol))
                if c.const_g is not None:                              # a constant group comes out as beta (or silu(beta))
                    b = c.beta.double()[c.const_g * cg:(c.const_g + 1) * cg]
                    want = b / (1.0 + torch.exp(-b)) if silu else b
                    assert (c.x[:, c.const_g * cg:(c.const_g + 1) * cg] == 0.5).all()
                    assert torch.equal(ref[:, c.const_g * cg:(c.const_g + 1) * cg], want[None, :].expand(M, cg))
    print(f"groupnorm C {C} G {G_}: fp32 torch uses {worst:.3f} of the tolerance before its bf16 rounding")
    assert worst <= 0.5


@pytest.mark.parametrize("C,G_", G.GN_WIDTHS, ids=ids)
def test_groupnorm_single_pass_variance_on_offset_data(C, G_):
    """the two-pass kernel's statistics are ONE pass over x and x^2: at mean / sigma = 32 the variance is what is left of sums 1025 times
    as large.  Short fp32 runs added up in double keep rstd within 2^-12; the long fp32 runs the kernel had until these tests did not
    from C = 512 up (5e-3 at C = 2048: every output of such a tensor off by up to half a percent of its distance from beta)."""
    out = []
    for M in (513, 2100):
        for data in ("offset", "wide"):
            c = G.cached(R.gn_case, M, C, G_, data)
            mean, var = R.group_stats64(c.x, G_)
            rstd = 1.0 / torch.sqrt(var + R.GN_EPS)
            m32, r32 = R.emulate_two_pass_stats(c.x, G_)
            err = float(((r32.double() - rstd) / rstd).abs().max())
            merr = float(((m32.double() - mean).abs() * rstd).max())
            old = float(((R.emulate_two_pass_stats(c.x, G_, long_fp32_runs=True)[1].double() - rstd) / rstd).abs().max())
            out.append(f"M {M} {data}: rstd {err:.1e} (long fp32 runs {old:.1e}), mean {merr:.1e} sigma")
            assert err < 2.0 ** -12 and merr < 2.0 ** -12, (M, data, err, merr)
            if data == "offset":
                assert 25.0 < float(mean.min() * rstd.min())
                assert (old > 2.0 ** -12) == (C >= 512), (C, old)       # what these cases would have caught
    print(f"groupnorm C {C} G {G_}: relative error of the emulated fp32-partial-sum statistics: " + "; ".join(out))


def test_emulated_statistics_are_the_tensor_s_statistics():
    c = R.gn_case(700, 128, 32, "wide")
    mean, var = R.group_stats64(c.x, 32)
    m32, r32 = R.emulate_two_pass_stats(c.x, 32)
    assert torch.allclose(m32.double(), mean, rtol=0, atol=1e-5) and torch.allclose(r32.double(), 1 / torch.sqrt(var + R.GN_EPS), rtol=1e-5)
    ref, _ = R.groupnorm_ref(c.x, c.gamma, c.beta, 32, 0)
    want = torch.nn.functional.group_norm(c.x.double().t()[None], 32, c.gamma.double(), c.beta.double(), R.GN_EPS)[0].t()
    assert torch.allclose(ref, want, rtol=0, atol=1e-10)


def test_quad_cases_have_the_entry_counts_they_claim():
    n, per = R.quad_slices(*G.GN_QUAD_CASES[0])
    assert n == 2 and sorted(per) == [0] * 14 + [1, 1]                 # 14 of the 16 first-level slices are empty
    n, per = R.quad_slices(*G.GN_QUAD_CASES[1])
    assert n == 16 and per == [1] * 16
    n, per = R.quad_slices(*G.GN_QUAD_CASES[2])
    assert n == 17188 > 16384 and min(per) > R.GNQ_STRIDE and max(per) < 2 * R.GNQ_STRIDE   # a second trip of the stride in every slice
    print(f"quad entries per group / per slice: {[R.quad_slices(*c)[0] for c in G.GN_QUAD_CASES]} / "
          f"{[sorted(set(R.quad_slices(*c)[1])) for c in G.GN_QUAD_CASES]}")


@pytest.mark.parametrize("M,C,G_", G.GN_QUAD_CASES[:2], ids=ids)
def test_quad_case_data_leaves_room_for_the_kernels(M, C, G_):
    """the fp32 rounding of the host-made quad entries alone moves at most 0.1 % of the outputs: half of what the quad form and the
    two-pass form may differ by.  (The third case has 17 188 entries per group: their roundings average out.)"""
    for data in R.GN_DATA:
        c = G.quad_case(M, C, G_, data)
        flips = [R.quad_rounding_flips(c, silu) for silu in (0, 1)]
        print(f"quad case {M}x{C}/{G_} {data}: the entries' fp32 rounding moves {flips[0]:.5f} / {flips[1]:.5f} of the outputs (SiLU off / on)")
        assert max(flips) <= 1e-3


def test_quad_statistics_layout():
    c = R.gn_case(300, 64, 16, "wide")
    q = R.quad_stats(c.x)
    assert tuple(q.shape) == (4, 16, 2) and q.dtype == torch.float32
    x = c.x.double()
    assert torch.equal(q[1, 5, 0], x[128:256, 20:24].sum().float()) and torch.equal(q[2, 0, 1], (x[256:300, 0:4] ** 2).sum().float())
    assert not q[3].any()                                              # rows >= M count nothing
    xg = x.view(300, 16, 4)
    assert torch.allclose(q.double().sum(0)[:, 0], xg.sum((0, 2)), rtol=1e-6, atol=1e-3)


def test_refusal_table_breaks_one_rule_each():
    broken = []
    for (M, C, G_), status in G.GN_REFUSALS:
        arg = G_ > 64 or C % G_ != 0
        cg = C // G_ if not arg else 0
        unsupported = not arg and (C % 8 != 0 or cg < 4 or cg & (cg - 1) != 0 or C // 8 > 256 or (C // 8) & (C // 8 - 1) != 0)
        assert status == (G.ERR_ARG if arg else G.ERR_UNSUPPORTED) and (arg or unsupported)
        broken.append("G > 64" if G_ > 64 else "C % G" if arg else "C % 8" if C % 8 else "group width" if cg & (cg - 1) else "C > 2048")
    assert sorted(broken) == sorted(["G > 64", "C % G", "C % 8", "group width", "C > 2048"])
