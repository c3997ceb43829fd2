"""CPU-only checks of the integer-exact convolution probes (tests/conv_probe_reference.py): the int64 gather reference equals the oracle
(oracle/vae_oracle.py, fp32 mode, widened to float64) for every legal combination of upsample and stride, degenerate extents included;
every case of the GPU file's tables keeps the exactness and coverage conditions; and every such case tells the true index rule from each
mutated rule that can apply to its geometry — so a kernel that implemented the mutated rule would fail the GPU test of that case."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_probe_reference import MUTATIONS, applicable, block_stats_ref, explain, int_ref, make_case, pack_weights, source_index  # noqa: E402
from test_gpu_conv_probes import OUT3_CASES, STRIDED_CASES, TILE_CASES, W4_CASES, probe_case  # noqa: E402

from oracle import vae_oracle as V  # noqa: E402

COMBOS = [((ut, us), (1, 1)) for ut in (1, 2) for us in (1, 2)] + [((1, 1), st) for st in ((1, 2), (2, 1), (2, 2))]
GPU_CASES = ([(d, ci, co, up, (1, 1)) for d, ci, co, up in TILE_CASES] + [(d, ci, co, (1, 1), st) for d, ci, co, st in STRIDED_CASES]
             + [(d, ci, 3, (1, 1), (1, 1)) for d, ci in OUT3_CASES])
W4_KEYS = [(d, ci, co, up, (1, 1)) for _, d, ci, co, up in W4_CASES]


def oracle_conv(case):
    """the oracle on the same integers: dense weights, fp32 mode, [M][Cout] in float64"""
    Ts, Hs, Ws = case.dims
    w = pack_weights(case).float().view(case.Cout, 3, 3, 3, case.Cin).permute(0, 4, 1, 2, 3).contiguous()
    sd = {"c.conv.weight": w, "c.conv.bias": case.bias.float()}
    sd.update({"u.conv.conv.weight": w, "u.conv.conv.bias": sd["c.conv.bias"]})       # upsample() names its conv <p>.conv
    x = case.x.float().permute(3, 0, 1, 2)[None]
    if case.st != (1, 1):
        y = V.causal_conv3d_strided(sd, "c", x, (case.st[0], case.st[1], case.st[1]), "fp32")
    elif case.up != (1, 1):
        y = V.upsample(sd, "u", x, (case.up[0], case.up[1], case.up[1]), "fp32")
    else:
        y = V.causal_conv3d(sd, "c", x, "fp32")
    assert tuple(y.shape[2:]) == case.grid
    return y[0].permute(1, 2, 3, 0).reshape(-1, case.Cout).double()


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 3), (3, 5, 9), (1, 4, 6), (4, 9, 8)])
def test_int_ref_equals_the_oracle(dims):
    for up, st in COMBOS:
        case = make_case(*dims, 128, 40, seed=sum(dims) + 10 * up[0] + 20 * up[1] + 40 * st[0] + 80 * st[1], up=up, st=st)
        want = int_ref(case)
        assert torch.equal(want.double(), oracle_conv(case)), (dims, up, st)
        assert torch.equal(int_ref(case, resid=True), want + case.resid)


def differing_rows(case, rule, limit=2048):
    """output rows whose source position (or its validity) changes under `rule` for some tap"""
    diff = torch.zeros(case.M, dtype=torch.bool)
    for tap in range(27):
        i0, _ = source_index(case, tap)
        i1, ok = source_index(case, tap, rule)
        diff |= (i0 != i1) | ~ok
    return diff.nonzero()[:, 0][:limit]


def check_power(key):
    """every mutation either cannot apply to the geometry (listed by `applicable`, and then it changes no index) or changes the
    expected output; compared on the rows it touches, which decides the whole tensor"""
    case = probe_case(*key)
    for rule in MUTATIONS:
        rows = differing_rows(case, rule)
        if not applicable(case, rule):
            # the explicit list of (case family, mutation) pairs that cannot be told apart: nothing to gather differently, except where
            # the changed index reads the same pixel value by construction (none of the rules above does)
            assert rows.numel() == 0, (key, rule)
            continue
        assert rows.numel() > 0, (key, rule)
        assert not torch.equal(int_ref(case, rule=rule, rows=rows), int_ref(case, rows=rows)), (key, rule)


@pytest.mark.parametrize("chunk", range(8))
def test_every_small_gpu_case_is_exact_covered_and_tells_the_mutations_apart(chunk):
    for key in GPU_CASES[chunk::8]:
        case = probe_case(*key)                    # make_case asserts the coverage of taps and slabs
        int_ref(case, resid=True)                  # asserts |conv + bias| <= 80 and |out| <= 256
        check_power(key)


@pytest.mark.parametrize("key", W4_KEYS, ids=lambda v: str(v).replace(" ", ""))
def test_every_four_wave_case_is_exact_covered_and_tells_the_mutations_apart(key):
    case = probe_case(*key)
    want = int_ref(case, resid=True)
    To, Ho, Wo = case.grid
    block_stats_ref(want, case.M, case.Cout, case.grid if Ho % 8 == 0 and Wo % 32 == 0 else None)   # asserts < 2^24
    check_power(key)


def test_mutations_that_cannot_apply_are_the_listed_ones():
    """the pairs `applicable` rules out, by family: no stride -> no stride phase; no temporal upsample or one frame -> no frame-0 rule;
    one pixel per frame -> no dh / dw swap and no far clamp; stride 2 over an even extent -> no far-side padding to zero"""
    one = probe_case((1, 1, 1), 64, 72, (2, 2), (1, 1))
    assert [r for r in MUTATIONS if not applicable(one, r)] == ["no_frame0", "swap_hw", "stride_phase", "clamp_far"]
    up = probe_case((3, 5, 9), 64, 72, (2, 2), (1, 1))
    assert [r for r in MUTATIONS if not applicable(up, r)] == ["stride_phase"]
    even = probe_case((4, 8, 7), 64, 64, (1, 1), (2, 2))
    assert [r for r in MUTATIONS if not applicable(even, r)] == ["no_frame0", "zero_bottom"]
    plain = probe_case((2, 9, 33), 64, 3, (1, 1), (1, 1))
    assert [r for r in MUTATIONS if not applicable(plain, r)] == ["no_frame0", "stride_phase"]


def test_block_stats_layouts_and_explain():
    out = torch.arange(2 * 8 * 32 * 8).view(512, 8) % 7 - 3
    lin = block_stats_ref(out[:300], 300, 8)
    assert lin.shape == (4, 2, 2) and torch.equal(lin[2, 1, 0], out[256:300, 4:].sum().float()) and not lin[3].any()
    pat = block_stats_ref(out, 512, 8, (1, 8, 64))
    rows = (torch.arange(4)[:, None] * 64 + 32 + torch.arange(32)[None, :]).reshape(-1)      # upper half of the second patch
    assert torch.equal(pat[2, 0, 1], (out[rows, :4] ** 2).sum().float())
    case = probe_case((2, 9, 33), 64, 3, (1, 1), (1, 1))
    want = int_ref(case).float()
    got = want.clone()
    m = (1 * 9 + 8) * 33 + 32
    got[m, 2] += 1
    msg = explain(got, want, case)
    assert "(t=1, h=8, w=32) c=2" in msg and "last row" in msg and "last column" in msg and "patch seam" in msg and "tap" in msg
    assert explain(want, want, case) == "no mismatch"
