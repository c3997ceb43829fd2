"""Host tests of oracle/parity.py: the comparison the GPU attention tests rely on CAN fail.

A host model of the kernel (fp32 scores, P rounded to bf16 before P.V, fp32 sums of the rounded P, one bf16 rounding of the output)
stands in for the kernel.  It must pass at margin 2; an all-NaN output, one NaN element and four plausible kernel defects must be
rejected even at the largest margin any form may be given (parity.MARGIN_LIMIT); and the NaN-blind form of the older helpers
(`not (err > tol).any()`) must be gone from assert_bf16_close and close.

One defect is EXPECTED TO PASS (test_zero_valued_pad_keys_are_invisible_on_random_data): three unmasked padding keys of score 0 and value 0
only add 3 to a denominator of ~ 1600 at 1000 keys, far inside the bf16 rounding of the output.  No tolerance on random data can see
that; tests/test_gpu_attention_edges.py exists for it (poisoned padding, probe rows)."""
import importlib.util
import os

import pytest
import torch

from oracle import k5_oracle as O
from oracle import parity as P
from kit import bfr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(72, 72), (300, 77), (513, 7), (1000, 1000), (64, 640), (10, 4096)]
DEFECT_KEYS = [77, 1000, 4096]


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def kernel_model(q, k, v, *, keep=None, twice=0, scale=0.125, pad_keys=0):
    """(Sq, H, 64), (Sk, H, 64) x 2 -> (Sq, H * 64) as the kernel computes it, with optional defects:
    keep = use only the first `keep` keys; twice = count the first `twice` keys two times; scale = the softmax scale used;
    pad_keys = that many extra keys of score 0 and value 0 (unmasked padding)."""
    Sq, H, d = q.shape
    if keep is not None:
        k, v = k[:keep], v[:keep]
    if twice:
        k, v = torch.cat([k, k[:twice]]), torch.cat([v, v[:twice]])
    if pad_keys:
        k, v = torch.cat([k, torch.zeros(pad_keys, H, d)]), torch.cat([v, torch.zeros(pad_keys, H, d)])
    out = torch.empty(Sq, H, d)
    for h in range(H):
        s = (q[:, h] @ k[:, h].t()) * scale
        p = bfr(torch.exp(s - s.amax(-1, keepdim=True)))
        out[:, h] = (p @ v[:, h]) / p.sum(-1, keepdim=True)
    return bfr(out.reshape(Sq, H * d))


@pytest.fixture(scope="module")
def cases():
    """one problem per (Sq, Sk): inputs, the bf16-island oracle and the float64 reference — computed once, shared, never modified"""
    out = {}
    for Sq, Sk in SHAPES + [(48, n) for n in DEFECT_KEYS]:
        H = 2 if Sk < 2000 else 1
        q, k, v = bfr(rnd(Sq, H, 64, seed=1)), bfr(rnd(Sk, H, 64, seed=2)), bfr(rnd(Sk, H, 64, seed=3))
        out[(Sq, Sk)] = (q, k, v, P.AttentionRef(q, k, v))
    return out


def test_float64_reference_agrees_with_the_oracle_and_its_options():
    q, k, v = bfr(rnd(128, 2, 64, seed=4)), bfr(rnd(192, 2, 64, seed=5)), bfr(rnd(192, 2, 64, seed=6))
    ref = P.attention_f64(q, k, v)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (128, 128)
    assert (ref - O.sdpa(q, k, v, "fp32").double()).abs().max().item() < 1e-5
    kc = bfr(k * torch.tensor(O.SOFTMAX_C))                        # pre-scaled keys, exp2 domain
    assert (P.attention_f64(q, kc, v, base2=True) - O.sdpa(q, kc, v, "fp32", None, base2=True).double()).abs().max().item() < 1e-5
    mask = torch.rand(2, 2, 3, generator=torch.Generator().manual_seed(7)) < 0.5
    mask[:, :, 0] = True                                            # every row keeps a block
    assert (P.attention_f64(q, k, v, block_mask=mask) - O.sdpa(q, k, v, "fp32", mask).double()).abs().max().item() < 1e-5
    # a masked key does not count: the same as attending the kept blocks only
    only0 = torch.zeros(1, 2, 3, dtype=torch.bool)
    only0[:, :, 0] = True
    assert torch.allclose(P.attention_f64(q[:, :1], k[:, :1], v[:, :1], block_mask=only0), P.attention_f64(q[:, :1], k[:64, :1], v[:64, :1]), rtol=1e-12, atol=0)
    e = P.row_rel_err(ref.float() * 1.01, ref, 2)
    assert tuple(e.shape) == (128, 2) and torch.allclose(e, torch.full_like(e, 0.01), rtol=1e-4)


@pytest.mark.parametrize("Sq,Sk", SHAPES)
def test_kernel_model_passes_at_margin_two(cases, Sq, Sk):
    q, k, v, ref = cases[(Sq, Sk)]
    ratio = ref.close(kernel_model(q, k, v), 2.0, f"kernel model {Sq}x{Sk}")
    assert ratio > 0.5                                             # ... and the measure is not vacuous: bf16 rounding is really there
    y = P.yardstick(ref.bf16, ref.f64, q.shape[1])
    assert 1.5e-3 < y < 3e-3, y                                     # the oracle's own distance: the bf16 rounding of 64 values


def test_non_finite_outputs_are_rejected(cases):
    q, k, v, ref = cases[(72, 72)]
    good = kernel_model(q, k, v)
    with pytest.raises(AssertionError, match=r"9216 of 9216 output elements are not finite \(9216 NaN\)"):
        ref.close(torch.full_like(good, float("nan")), P.MARGIN_LIMIT, "all NaN")
    one = good.clone()
    one[71, 127] = float("nan")
    with pytest.raises(AssertionError, match="1 of 9216 output elements are not finite"):
        ref.close(one, P.MARGIN_LIMIT, "one NaN")
    inf = good.clone()
    inf[0, 0] = float("inf")
    with pytest.raises(AssertionError, match=r"1 of 9216 output elements are not finite \(0 NaN\)"):
        ref.close(inf, P.MARGIN_LIMIT, "one inf")
    with pytest.raises(AssertionError, match="finding"):            # no margin beyond the limit, whatever the data
        ref.close(good, P.MARGIN_LIMIT + 0.5, "margin 4.5")
    zero_row = ref.f64.clone()
    zero_row[3, :64] = 0.0
    with pytest.raises(AssertionError, match="no norm"):            # rows are never masked out of the measure
        P.assert_attention_close(good, zero_row, ref.bf16, 2.0, "zero reference row")


def test_canary_sees_a_write_outside_the_output(cases):
    q, k, v, ref = cases[(72, 72)]
    buf = torch.full((75, 136), 7.0)
    buf[:72, :128] = kernel_model(q, k, v)
    ref.close(buf[:72, :128], 2.0, "canary intact", canary=(buf, 72, 128, 7.0))
    for r, c in ((72, 0), (0, 128), (74, 135)):
        b = buf.clone()
        b[r, c] = 0.0
        with pytest.raises(AssertionError, match="outside"):
            ref.close(b[:72, :128], 2.0, "canary hit", canary=(b, 72, 128, 7.0))


@pytest.mark.parametrize("Sk", DEFECT_KEYS)
@pytest.mark.parametrize("defect", ["last key dropped", "last 16 keys dropped", "first 32 keys counted twice", "scale 1/8 -> 1/7.5"])
def test_kernel_defects_are_rejected(cases, defect, Sk):
    q, k, v, ref = cases[(48, Sk)]
    ref.close(kernel_model(q, k, v), 2.0, f"sound model, {Sk} keys")
    bad = {"last key dropped": dict(keep=Sk - 1), "last 16 keys dropped": dict(keep=Sk - 16),
           "first 32 keys counted twice": dict(twice=32), "scale 1/8 -> 1/7.5": dict(scale=1.0 / 7.5)}[defect]
    with pytest.raises(AssertionError, match="beyond"):
        ref.close(kernel_model(q, k, v, **bad), P.MARGIN_LIMIT, f"{defect}, {Sk} keys")


def test_zero_valued_pad_keys_are_invisible_on_random_data(cases):
    """EXPECTED TO PASS, and asserted to: three unmasked pad keys (score 0, V = 0) at 1000 keys shrink every output by 3 / sum_j exp(s_j - 0)
    ~ 0.2 % — below the bf16 rounding of the output, so the relative measure (like any tolerance on random data) lets it through.
    The defect is visible only when the padding holds data that hurts (tests/test_gpu_attention_edges.py: poisoned K rows and V^T columns)."""
    q, k, v, ref = cases[(1000, 1000)]
    ref.close(kernel_model(q, k, v, pad_keys=3), 2.0, "3 zero-valued pad keys, 1000 keys")


def _load(name):
    spec = importlib.util.spec_from_file_location("_parity_probe_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("module,helper", [("test_gpu_kernels", "assert_bf16_close"), ("test_gpu_softmax_variants", "close")])
def test_elementwise_helpers_reject_nan(module, helper):
    fn = getattr(_load(module), helper)
    ref = bfr(rnd(8, 64, seed=9))
    fn(ref.clone(), ref, what="equal")
    with pytest.raises(AssertionError):
        fn(torch.full_like(ref, float("nan")), ref, what="all NaN")
    one = ref.clone()
    one[5, 5] = float("nan")
    with pytest.raises(AssertionError):
        fn(one, ref, what="one NaN")
    off = ref.clone()
    off[2, 3] += 1.0
    with pytest.raises(AssertionError):
        fn(off, ref, what="one value off")
