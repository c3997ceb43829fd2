"""Attention at its edges, on data that make a wrong key visible (MI355X, through the C ABI).

Random q / k / V cannot see a key that is skipped, doubled or read from the padding: its weight is ~ 1 / Sk of a row that is compared
with a tolerance (tests/test_parity_helpers.py: three zero-valued pad keys pass at 1000 keys).  Here

1. PROBE rows: q_i = g k_j(i) with |k| = 8 puts key j(i) 40 nats (g = 5) above a field of N(0, 5^2) scores, and V[j] is a bf16-exact code
   of (j, column) — the float64 output of the row IS V[j(i)] to < 1e-6 (asserted of the reference), so a key that is misread, skipped,
   doubled or taken from another head's columns is an O(1) error of its probe row.  Probes sit at every tile edge of the 64-key tile
   and at the ragged end, for key counts around the tile size.
2. POISON: every buffer is allocated larger than the problem and the surplus is filled with finite values that would wreck the result
   (keys 1000 q_0, values 3e4, queries 1e3) or, for O, with 7.0 canaries: the result must be bit-identical to the call on tight,
   zero-padded buffers and no canary may change.
3. the block-sparse kernel on a hand-made map: probes at the first and last key of a kept and of a dropped block.

Bounds.  Probe rows: the kernel's output is one bf16 rounding (unit roundoff 2^-9 per element, hence <= 2^-9 of the row norm) of a value
within 1e-6 of V[j]; allowed 2^-8 = two roundings.  Ordinary rows: oracle.parity's yardstick and per-form margins."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
from oracle import parity as P  # noqa: E402
from kit import BF, E, bfr  # noqa: E402

C = O.SOFTMAX_C
PROBE_TOL = 2.0 ** -8


def rms8(x):
    return x / x.pow(2).mean(-1, keepdim=True).sqrt()          # |x| = 8 over 64 dimensions


@functools.lru_cache(maxsize=None)
def _vtable():
    """641 keys x 192 columns of integers / 128 in [-125, 125] / 128 (exact in bf16) from a fixed seed; every pair of rows differs in every head"""
    t = torch.randint(-125, 126, (641, 192), generator=torch.Generator().manual_seed(641)).float() / 128.0
    assert len({tuple(r.tolist()) for h in range(3) for r in t[:, 64 * h:64 * h + 64]}) == 3 * 641
    return t


def vcode(Sk, H):
    """V[j][64 h + d]: a bf16-exact code of (key, column) — a value row names its key and its head.  A TABLE of random codes rather than a
    formula such as ((64 j + d) % 251 - 125) / 128: that one is a low-discrepancy sequence along j, its weighted sums cancel far better
    than random values do, the ordinary rows' outputs come out 2-3 x smaller than their summands' noise and the bf16 rounding of P — harmless,
    the host model of the kernel shows the same — reads as 3.2 x the yardstick instead of 1.4 x (measured on both)."""
    return _vtable()[:Sk, :H * 64].reshape(Sk, H, 64).clone()


def probe_keys(Sk):
    return sorted({j for j in (0, 1, 15, 16, 31, 32, 63, 64, 65, 127, 128, Sk - 65, Sk - 64, Sk - 2, Sk - 1) if 0 <= j < Sk})


@functools.lru_cache(maxsize=None)
def probe_case(Sq, Sk, H, gain, prescaled):
    """inputs (bf16-valued fp32, host), the probe keys (row i < len(js) probes key js[i], the same key in every head) and the references;
    computed once per shape and shared by the forms — never modified"""
    g = torch.Generator().manual_seed(1000 * Sk + 10 * Sq + H)
    k = bfr(rms8(torch.randn(Sk, H, 64, generator=g)))
    q = bfr(rms8(torch.randn(Sq, H, 64, generator=g)))
    js = probe_keys(Sk)[:Sq]
    q[:len(js)] = bfr(gain * k[js])
    v = vcode(Sk, H)
    kk = bfr(k * torch.tensor(C)) if prescaled else k
    R = P.AttentionRef(q, kk, v, base2=prescaled)
    want = v[js].reshape(len(js), H * 64).double()
    assert (R.f64[:len(js)] - want).abs().max().item() < 1e-6        # the reference of a probe row IS the value row of its key
    assert torch.equal(bfr(v), v)
    return q, kk, v, js, R


def check_probes(got, case, margin, what):
    q, k, v, js, R = case
    H, n = q.shape[1], len(js)
    got = got.float().cpu()
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    err = P.row_rel_err(got[:n], R.f64[:n], H)
    worst = int(err.argmax())
    assert err.max().item() <= PROBE_TOL, (f"{what}: probe of key {js[worst // H]} (row {worst // H}, head {worst % H}) is off by {err.max().item():.3g} "
                                           f"of its row; probe keys {js}, errors per row {err.amax(1).tolist()}")
    if q.shape[0] > n:                                                # the ordinary rows: the form's margin on the yardstick
        P.assert_attention_close(got[n:], R.f64[n:], R.bf16[n:], margin, what + ", ordinary rows")


def dev(x):
    return x.reshape(x.shape[0], -1).cuda().to(BF).contiguous()


def vt_padded(v, ld=None, fill=0.0):
    Sk, H = v.shape[0], v.shape[1]
    ld = (Sk + 7) // 8 * 8 if ld is None else ld
    vt = torch.full((H * 64, ld), fill, dtype=BF, device="cuda")
    vt[:, :Sk] = v.reshape(Sk, H * 64).t().to(BF)
    return vt


def data_bound(q, k):
    """Cauchy-Schwarz bound on |q . k| from the tensors themselves (with the rounding slack the engine uses)"""
    return float(q.norm(dim=-1).amax() * k.norm(dim=-1).amax()) * 1.002


# ------------------------------------------------------------------------------------------ 1. key probes
@pytest.mark.parametrize("Sq", [15, 257])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("Sk", [1, 7, 63, 64, 65, 77, 128, 129, 200, 641])
def test_key_probes_plain_and_bounded(E, Sk, H, Sq):
    """k5_attention_bf16 (online max) and k5_attention_bf16_bounded (constant offset 0: the probe score 40 nats = 57.7 in the exp2 domain, the
    bound computed from the data stays inside the window of 90)."""
    case = probe_case(Sq, Sk, H, 5.0, False)
    q, k, v, js, R = case
    qd, kd, vt = dev(q), dev(k), vt_padded(v)
    check_probes(E.attention(qd, kd, vt, H, kv_len=Sk), case, P.MARGIN_ONLINE, f"plain {Sq}x{Sk}x{H}")
    bound = data_bound(q, k)
    assert 300.0 < bound and bound * C <= 90.0, bound               # the fixed-offset kernel really runs
    check_probes(E.attention(qd, kd, vt, H, kv_len=Sk, score_bound=bound), case, P.MARGIN_FIXED, f"bounded {Sq}x{Sk}x{H}")


def run_auto(E, qd, kd, vt, H, q_len, kv_len, out, flags, variant):
    L = E.lib()
    ws = torch.empty(L.k5_attention_balance_size(H, q_len), dtype=torch.uint8, device="cuda")
    E.check(L.k5_attention_bf16_prescaled_auto(qd.data_ptr(), kd.data_ptr(), vt.data_ptr(), out.data_ptr(), H, q_len, kv_len, qd.stride(0), kd.stride(0),
                                               vt.stride(0), out.stride(0), None if flags is None else flags.data_ptr(), variant, ws.data_ptr(),
                                               E.stream_ptr()), "k5_attention_bf16_prescaled_auto")
    torch.cuda.synchronize()
    return out


def flags_rows(E, q, k, H):
    """k5_attention_flags_rows on the statistics of the tensors: flags (1 = fixed form) and kmax"""
    qstat, kstat = (q * q).sum(-1).amax(0).contiguous().cuda(), (k * k).sum(-1).amax(0).contiguous().cuda()
    flags, kmax = torch.zeros(H, dtype=torch.int32, device="cuda"), torch.zeros(H, device="cuda")
    E.check(E.lib().k5_attention_flags_rows(qstat.data_ptr(), kstat.data_ptr(), 1, H, H, 0, flags.data_ptr(), kmax.data_ptr(), E.stream_ptr()))
    torch.cuda.synchronize()
    return flags, kmax


def run_rows(E, qd, kd, vt, H, q_len, kv_len, out, flags, kmax):
    L = E.lib()
    ws = torch.empty(L.k5_attention_balance_size(H, q_len), dtype=torch.uint8, device="cuda")
    E.check(L.k5_attention_bf16_prescaled_rows(qd.data_ptr(), kd.data_ptr(), vt.data_ptr(), out.data_ptr(), H, q_len, kv_len, qd.stride(0), kd.stride(0),
                                               vt.stride(0), out.stride(0), flags.data_ptr(), kmax.data_ptr(), ws.data_ptr(), E.stream_ptr()),
            "k5_attention_bf16_prescaled_rows")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Sq", [15, 257])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("Sk", [64, 128, 192, 640])
def test_key_probes_prescaled_forms(E, Sk, H, Sq):
    """The pre-scaled ABI (whole key tiles): _auto with every head forced to the fixed offset, _auto with variant ONLINE, and _rows — there at
    probe gain 10, which puts the probe rows' bound |q| max|k'| at 116 (inside the per-row window of 190, beyond 90): those rows run on a
    NON-ZERO per-row offset of ~ 26 and their probe score sits exactly at the bound, the ordinary rows on offset 0."""
    case = probe_case(Sq, Sk, H, 5.0, True)
    q, kc, v, js, R = case
    qd, kd, vt = dev(q), dev(kc), vt_padded(v)
    new = lambda: torch.full((Sq, H * 64), float("nan"), dtype=BF, device="cuda")     # noqa: E731  (an unwritten row is not finite)
    assert data_bound(q, kc) <= 90.0                                   # what forcing the fixed form requires of the data
    ones = torch.ones(H, dtype=torch.int32, device="cuda")
    check_probes(run_auto(E, qd, kd, vt, H, Sq, Sk, new(), ones, 0), case, P.MARGIN_FIXED, f"prescaled fixed {Sq}x{Sk}x{H}")
    check_probes(run_auto(E, qd, kd, vt, H, Sq, Sk, new(), None, 1), case, P.MARGIN_ONLINE, f"prescaled online {Sq}x{Sk}x{H}")
    case = probe_case(Sq, Sk, H, 10.0, True)
    q, kc, v, js, R = case
    flags, kmax = flags_rows(E, q, kc, H)
    bound = q.norm(dim=-1).amax(0) * kmax.cpu()
    assert flags.tolist() == [1] * H and (bound > 100.0).all() and (bound <= 190.0).all(), (flags, bound)
    out = run_rows(E, dev(q), dev(kc), vt, H, Sq, Sk, new(), flags, kmax)
    assert flags.tolist() == [1] * H, flags                            # no row underflowed: nothing fell back
    check_probes(out, case, P.MARGIN_ROWS, f"prescaled per-row offsets {Sq}x{Sk}x{H}")


# ------------------------------------------------------------------------------------------ 2. nothing beyond the edges is read or written
class Poisoned:
    """One allocation per operand, larger than the problem, the surplus filled with FINITE values that would wreck the result if read:
    K: 64 more rows of 1000 q_0;  V^T: ldvt = ceil8(Sk) + 64 with 3e4 in every column >= kv_len;  Q: 8 more rows of 1e3;
    O: ldo = H * 64 + 8 and 3 more rows, everything 7.0 beforehand."""

    def __init__(self, q, k, v):
        Sq, H = q.shape[0], q.shape[1]
        Sk = k.shape[0]
        self.Sq, self.Sk, self.H = Sq, Sk, H
        self.q = torch.full((Sq + 8, H * 64), 1e3, dtype=BF, device="cuda")
        self.q[:Sq] = dev(q)
        self.k = (1000.0 * q[0].reshape(1, H * 64)).expand(Sk + 64, H * 64).cuda().to(BF).contiguous()
        self.k[:Sk] = dev(k)
        self.vt = vt_padded(v, ld=(Sk + 7) // 8 * 8 + 64, fill=3e4)
        assert float(self.vt[0, Sk]) > 2.9e4 and float(self.k[Sk].float().abs().max()) > 100.0

    def out(self):
        return torch.full((self.Sq + 3, self.H * 64 + 8), 7.0, dtype=BF, device="cuda")

    def check(self, o, tight, R, margin, what):
        """bit-identical to the tight call inside, canaries intact outside, and (so that 'identical' is not 'identically wrong') float64 parity"""
        torch.cuda.synchronize()
        inside = o[:self.Sq, :self.H * 64]
        assert torch.isfinite(inside.float()).all(), f"{what}: {int((~torch.isfinite(inside.float())).sum())} non-finite values"
        diff = inside != tight
        assert not diff.any(), f"{what}: {int(diff.sum())} values differ from the call on tight buffers, first at {diff.nonzero()[0].tolist()}"
        R.close(inside, margin, what, canary=(o, self.Sq, self.H * 64, 7.0))


@functools.lru_cache(maxsize=None)
def random_case(Sq, Sk, H, prescaled):
    g = torch.Generator().manual_seed(7000 + 1000 * Sk + Sq)
    q, k = bfr(rms8(torch.randn(Sq, H, 64, generator=g))), bfr(rms8(torch.randn(Sk, H, 64, generator=g)))
    v = bfr(torch.randn(Sk, H, 64, generator=g))
    if prescaled:
        k = bfr(k * torch.tensor(C))
    return q, k, v, P.AttentionRef(q, k, v, base2=prescaled)


@pytest.mark.parametrize("q_len", [1, 31, 33, 255, 257, 513])
@pytest.mark.parametrize("kv_len", [1, 7, 63, 65, 77, 129])
def test_poisoned_padding_plain_and_bounded(E, kv_len, q_len):
    H = 2
    q, k, v, R = random_case(q_len, kv_len, H, False)
    pz = Poisoned(q, k, v)
    qd, kd, vt = dev(q), dev(k), vt_padded(v)
    bound = data_bound(q, k)
    assert bound * C <= 90.0
    for name, sb, margin in (("plain", None, P.MARGIN_ONLINE), ("bounded", bound, P.MARGIN_FIXED)):
        tight = E.attention(qd, kd, vt, H, kv_len=kv_len, score_bound=sb)
        o = E.attention(pz.q, pz.k, pz.vt, H, q_len=q_len, kv_len=kv_len, out=pz.out(), score_bound=sb)
        pz.check(o, tight, R, margin, f"poisoned padding, {name} {q_len}x{kv_len}")


@pytest.mark.parametrize("q_len", [1, 31, 33, 255, 257, 513])
@pytest.mark.parametrize("kv_len", [64, 192])
def test_poisoned_padding_prescaled_forms(E, kv_len, q_len):
    H = 2
    q, kc, v, R = random_case(q_len, kv_len, H, True)
    pz = Poisoned(q, kc, v)
    qd, kd, vt = dev(q), dev(kc), vt_padded(v)
    tight_out = lambda: torch.full((q_len, H * 64), float("nan"), dtype=BF, device="cuda")     # noqa: E731
    ones = torch.ones(H, dtype=torch.int32, device="cuda")
    for name, flags, variant, margin in (("fixed", ones, 0, P.MARGIN_FIXED), ("online", None, 1, P.MARGIN_ONLINE)):
        tight = run_auto(E, qd, kd, vt, H, q_len, kv_len, tight_out(), flags, variant)
        o = run_auto(E, pz.q, pz.k, pz.vt, H, q_len, kv_len, pz.out(), flags, variant)
        pz.check(o, tight, R, margin, f"poisoned padding, prescaled {name} {q_len}x{kv_len}")
    flags, kmax = flags_rows(E, q, kc, H)
    assert flags.tolist() == [1] * H
    tight = run_rows(E, qd, kd, vt, H, q_len, kv_len, tight_out(), flags, kmax)
    o = run_rows(E, pz.q, pz.k, pz.vt, H, q_len, kv_len, pz.out(), flags, kmax)
    assert flags.tolist() == [1] * H, flags
    pz.check(o, tight, R, P.MARGIN_ROWS, f"poisoned padding, prescaled rows {q_len}x{kv_len}")


# ------------------------------------------------------------------------------------------ 3. the block-sparse kernel on a hand-made map
def test_sparse_probes_on_kept_and_dropped_blocks(E):
    """N = 512: an 8 x 8 block map per head, made by k5_nabla_select_bf16 itself from data built for it (grid (8, 1, 1), window (1, 1, 1): the STA
    window is the diagonal; P = 0.95): the queries AND keys of block A share a large component along one direction u, so A's logit row is
    ~ 8 on its own block and ~ 0 elsewhere (p_own = 0.998: only the own block survives the cut), every other query block sees ~ uniform
    probabilities (all >= 1 - P: every block is kept).  The map is read back and asserted to be exactly that before anything relies on it.
    Probes (q_i = 8 k_j: 64 nats and more above the rest) from query block A at the first and last key of its own (kept) block — they must land on V[j] — and of a DROPPED
    block — the masked float64 reference ignores that key, so a kernel that walks it anyway is off by O(1); from an all-keeping query block B
    at the first and last key of blocks 0, 7 and A."""
    N, H, nb = 512, 2, 8
    AB = [(2, 6), (5, 1)]                                            # (A, B) per head
    DROPPED = [4, 0]                                                 # the dropped block A's probes aim at, per head
    g = torch.Generator().manual_seed(512)
    q, k = rms8(torch.randn(N, H, 64, generator=g)), rms8(torch.randn(N, H, 64, generator=g))
    probes = []                                                      # (row, head, key, kept)
    for h, (A, B) in enumerate(AB):
        u = torch.randn(64, generator=g)
        u = u / u.norm()
        blkA = slice(64 * A, 64 * A + 64)
        k[blkA, h] += 8.0 * u
        q[blkA, h] += 8.0 * u
    k = bfr(k)
    for h, (A, B) in enumerate(AB):
        D = DROPPED[h]
        for i, (j, kept) in enumerate([(64 * A, True), (64 * A + 63, True), (64 * D, False), (64 * D + 63, False)]):
            probes.append((64 * A + 7 + 13 * i, h, j, kept))
        for i, j in enumerate([0, 63, 448, 511, 64 * A, 64 * A + 63]):
            probes.append((64 * B + 3 + 9 * i, h, j, True))
    for row, h, j, _ in probes:
        q[row, h] = 8.0 * k[j, h]
    q = bfr(q)
    v = vcode(N, H)
    qd, kd, vt = dev(q), dev(k), vt_padded(v)
    ws = E.nabla_select(qd, kd, H, (8, 1, 1), (1, 1, 1), 0.95)
    mask = E.nabla_mask(ws, H, nb).cpu()
    for h, (A, B) in enumerate(AB):
        assert mask[h, A].tolist() == [b == A for b in range(nb)], (h, mask[h, A])
        assert mask[h, B].all(), (h, mask[h, B])
    R = P.AttentionRef(q, k, v, block_mask=mask)
    got = E.attention_nabla(qd, kd, vt, H, ws)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    err = P.row_rel_err(got, R.f64, H)
    for row, h, j, kept in probes:
        ref_row = R.f64[row, 64 * h:64 * h + 64]
        if kept:
            assert (ref_row - v[j, h].double()).abs().max().item() < 1e-6, (row, h, j)       # the reference IS the key's value row
        else:
            assert (ref_row - v[j, h].double()).norm().item() > 0.1 * ref_row.norm().item(), (row, h, j)   # ... and here it is NOT: the key is masked
        tol = PROBE_TOL if kept else P.MARGIN_SPARSE * P.yardstick(R.bf16, R.f64, H)
        assert err[row, h].item() <= tol, f"probe row {row} head {h} at {'kept' if kept else 'DROPPED'} key {j}: off by {err[row, h].item():.3g} of its row"
    R.close(got, P.MARGIN_SPARSE, "sparse probes, all rows")
