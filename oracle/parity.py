"""One float64 reference and one comparison for every attention parity test.

Why not `abs(got - oracle) <= atol`: with random V an attention output shrinks with the key count (RMS 0.19 at 72 keys, 0.027 at
4096, 0.008 at 47 616), so an absolute 5e-3 .. 2e-2 is 10-60 % of the signal at the sizes that matter, and `not (err > tol).any()`
is satisfied by NaN.  Here the error of a (query row, head) is measured RELATIVE to that row's own reference, the reference is plain
float64 arithmetic, and a non-finite output fails before anything is compared.

The YARDSTICK is never the kernel under test: it is the distance of the bf16-island oracle (`k5_oracle.sdpa(..., "bf16")`: fp32 softmax,
one bf16 rounding of the output) from float64 on the same rows, computed by the test at run time — 2.1e-3 .. 2.4e-3 for every shape
and RMS-norm gain tried on the host (7 .. 47 616 keys, gains 1 .. 3.7): essentially the bf16 rounding of 64 output values.
A kernel additionally rounds P to bf16 before P.V and sums in another order, hence a MARGIN > 1 on the yardstick, one constant per
softmax form.  Rule: 1.5 x the largest ratio `max row_rel_err(kernel) / yardstick` measured over the form's tests on an MI355X,
rounded up to the next 0.5; a form that would need more than MARGIN_LIMIT is not given a margin — that is a finding to run down.
(Host model of the kernel — P -> bf16, fp32 sums, bf16 out: 1.1-1.5 x for the online form, 1.3-2.4 x for fixed offsets.  The defects
of tests/test_parity_helpers.py sit at >= 4.5 x in the median row and >= 50 x in the worst one up to 4096 keys.)
"""
import math
from typing import Optional

import torch
from torch import Tensor

from . import k5_oracle as O

MARGIN_LIMIT = 4.0

# Measured `max row_rel_err / yardstick` per form (MI355X, the kernels as they stood when this file was introduced; the largest value over
# every test that uses the form's margin, with the test that gave it) and the margin derived from it, ceil_to_0.5(1.5 x measured):
#   online   1.82  tests/test_gpu_softmax_variants.py centred-offsets test, 768 x 1088, heads 0 / 1 of the plain call (online form)  -> 3.0
#            (others: mixed launch, balanced, online heads 1.77; forced-online fused query norm 1.73; k5_attention_bf16 1000 x 1000 1.56; 47 616 keys 1.3-1.5)
#   fixed    1.94  tests/test_gpu_attention_edges.py poisoned padding, k5_attention_bf16_bounded 257 x 77                              -> 3.0
#            (others of the converted tests: balanced / single launch 300 x 640 1.55, bounded 700 x 700 1.53, window edge 1.50, config 2 / 5 rows 1.41)
#   rows     1.91  tests/test_gpu_softmax_variants.py per-row offsets 704 x 1088                                                       -> 3.0
#            (others: late fallback across passes 1.80, per job 1.74, fused query norm 1.72, anchored 1.66-1.68, centred 1.64)
#   sparse   1.72  tests/test_gpu_nabla.py two-pass list walk, "late", rank 1                                                          -> 3.0
#            (others: "gain3" 1.68, sparse attention bounded 1.47 / online 1.35)
# The worst row of 10^2 .. 10^5 rows is an extreme value: 1.2-1.9 over all 160 cases, against 1.1-1.5 (online) and 1.3-2.4 (fixed) of the host model.
MARGIN_ONLINE = 3.0     # online running max (k5_attention_bf16, variant ONLINE, heads sent to the online launch)
MARGIN_FIXED = 3.0      # constant offset 0 (k5_attention_bf16_bounded, _prescaled with a bound, flags = 1 heads of _auto)
MARGIN_ROWS = 3.0       # per-row / centred / anchored offsets (k5_attention_bf16_prescaled_rows*, _qnorm_pass), their fallbacks included
MARGIN_SPARSE = 3.0     # block-sparse list walk (k5_attention_nabla*)


def attention_f64(q: Tensor, k: Tensor, v: Tensor, *, base2: bool = False, block_mask: Optional[Tensor] = None) -> Tensor:
    """softmax(q k^T scale) v per head in float64 on the values given (the bf16-valued inputs of the kernel), nothing rounded.
    Layouts and mask as k5_oracle.sdpa: q (Sq, H, d), k / v (Sk, H, d) -> (Sq, H * d) float64; block_mask (H, Sq / 64, Sk / 64) bool.
    base2: the keys already carry log2(e) / sqrt(d) (the pre-scaled ABI): the scores are exp2 arguments."""
    Sq, H, d = q.shape
    qh, kh, vh = q.double().transpose(0, 1), k.double().transpose(0, 1), v.double().transpose(0, 1)
    scale = math.log(2.0) if base2 else 1.0 / math.sqrt(d)
    out = torch.empty(H, Sq, d, dtype=torch.float64)
    chunk = max(1, min(Sq, (1 << 24) // max(1, k.shape[0])))       # <= 128 MB of float64 scores at a time
    for h in range(H):
        bm = None if block_mask is None else block_mask[h].repeat_interleave(64, 0).repeat_interleave(64, 1)
        for s0 in range(0, Sq, chunk):
            s = (qh[h, s0:s0 + chunk] @ kh[h].t()) * scale
            if bm is not None:
                s = s.masked_fill(~bm[s0:s0 + chunk], float("-inf"))
            out[h, s0:s0 + chunk] = torch.softmax(s, dim=-1) @ vh[h]
    return out.transpose(0, 1).reshape(Sq, H * d)


def row_rel_err(got: Tensor, ref64: Tensor, H: int) -> Tensor:
    """(Sq, H): |got - ref|_2 / |ref|_2 over the 64 values of every (query row, head)."""
    Sq = ref64.shape[0]
    g = got.detach().cpu().double().reshape(Sq, H, -1)
    r = ref64.double().reshape(Sq, H, -1)
    return (g - r).norm(dim=-1) / r.norm(dim=-1)


def yardstick(yardstick_rows: Tensor, ref64: Tensor, H: int) -> float:
    """the bf16-island oracle's own worst row against float64"""
    return row_rel_err(yardstick_rows, ref64, H).max().item()


def assert_attention_close(got: Tensor, ref64: Tensor, yardstick_rows: Tensor, margin: float, what: str, canary=None) -> float:
    """got (Sq, H * 64) from the kernel, ref64 = attention_f64 of the same rows, yardstick_rows = k5_oracle.sdpa(..., "bf16") of the same rows.
    Fails on any non-finite element of got, then requires max over ALL (row, head) of row_rel_err <= margin * yardstick.
    canary = (buffer, rows, cols, value): every element of `buffer` outside [:rows, :cols] must still hold `value`.
    Returns the ratio max row_rel_err / yardstick (printed: the figures next to the margins above come from these lines)."""
    assert 0.0 < margin <= MARGIN_LIMIT, f"{what}: margin {margin} (a form that needs more than {MARGIN_LIMIT} is a finding, not a tolerance)"
    got = got.detach().float().cpu()
    assert got.shape == ref64.shape == yardstick_rows.shape, f"{what}: shapes {tuple(got.shape)} / {tuple(ref64.shape)} / {tuple(yardstick_rows.shape)}"
    H = ref64.shape[1] // 64
    finite = torch.isfinite(got)
    assert finite.all(), f"{what}: {int((~finite).sum())} of {got.numel()} output elements are not finite ({int(torch.isnan(got).sum())} NaN)"
    norms = ref64.reshape(ref64.shape[0], H, -1).norm(dim=-1)
    assert (norms > 0).all() and torch.isfinite(norms).all(), f"{what}: a reference row has no norm to measure against"
    y = yardstick(yardstick_rows, ref64, H)
    err = row_rel_err(got, ref64, H)
    worst = err.max().item()
    ratio = worst / y if y > 0.0 else (0.0 if worst == 0.0 else float("inf"))
    print(f"parity {what}: max row_rel_err {worst:.3e} / yardstick {y:.3e} = {ratio:.2f} (margin {margin})")
    if not worst <= margin * y:
        r, h = divmod(int(err.argmax()), H)
        over = int((err > margin * y).sum())
        raise AssertionError(f"{what}: {over} of {err.numel()} (row, head) pairs beyond {margin} x yardstick {y:.3e}; worst {worst:.3e} "
                             f"({ratio:.2f} x) at row {r} head {h}; median {err.median().item():.3e}")
    if canary is not None:
        buf, rows, cols, value = canary
        b = buf.detach().float().cpu()
        outside = torch.ones_like(b, dtype=torch.bool)
        outside[:rows, :cols] = False
        touched = outside & ~(b == value)
        assert not touched.any(), f"{what}: {int(touched.sum())} elements outside the {rows} x {cols} output were written, first at {touched.nonzero()[0].tolist()}"
    return ratio


class AttentionRef:
    """The three things every converted test needs of one problem, computed once: the bf16-island oracle (`.bf16`, what the older
    assertions compare with), the float64 reference (`.f64`) and, through `close`, the yardstick between them."""

    def __init__(self, q: Tensor, k: Tensor, v: Tensor, *, base2: bool = False, block_mask: Optional[Tensor] = None):
        self.bf16 = O.sdpa(q, k, v, "bf16", block_mask, base2=base2)
        self.f64 = attention_f64(q, k, v, base2=base2, block_mask=block_mask)

    def close(self, got: Tensor, margin: float, what: str, heads=None, canary=None) -> float:
        """heads: compare only these heads' columns (a launch that runs some heads in one softmax form and some in another: each form
        is held to its own margin; together the calls cover every head)"""
        if heads is None:
            return assert_attention_close(got, self.f64, self.bf16, margin, what, canary)
        cols = torch.cat([torch.arange(64 * h, 64 * h + 64) for h in heads])
        return assert_attention_close(got.detach().float().cpu()[:, cols], self.f64[:, cols], self.bf16[:, cols], margin, what, canary)
