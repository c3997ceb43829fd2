"""Integer-exact probes of every kernel behind k5_conv3d_bf16 / k5_conv3d_strided_bf16 / k5_conv3d_bf16_stats (conv3d.hip, conv3d_w4.hip):
every tap, every border (replicate padding on four sides, two replicated frames in front, frame 0 under the folded upsample), the output
stride, ragged last tiles and patch seams.  Inputs, sparse weights, bias and residual are small integers (tests/conv_probe_reference.py), so
the expected output is one bit pattern: every assertion here is torch.equal, there is no tolerance in this file.

Buffers: the output is [M + 64][Cout + 8] inside a larger allocation — payload NaN (an unwritten element fails the comparison), pad columns,
the 64 extra rows and the elements in front 7.0 (must still be 7.0 afterwards); X, W and the residual (ldr = Cout + 8, pad columns NaN) each
sit between 4096 NaN elements, which no output may have seen.  tests/test_conv_probe_host.py proves on the CPU that the reference is the
oracle's and that every case below tells the right index rule from each wrong one it could be confused with."""
import functools
import os
import sys
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_probe_reference import block_stats_ref, explain, int_ref, make_case, pack_weights  # noqa: E402

UPS = [(1, 1), (1, 2), (2, 1), (2, 2)]
# the 128 x 128 tile kernel: Cin % 128 != 0 or Cout not in {128, % 256} keeps the four-wave kernel out; Cout 136 = a second, ragged N-tile;
# (3, 5, 9) at up (2, 2) is M = 900: eight M-tiles, the last one ragged
TILE_CASES = [(dims, Cin, Cout, up) for Cin in (64, 192) for Cout in (72, 136) for dims in ((1, 1, 1), (2, 1, 3), (3, 1, 5), (3, 5, 9)) for up in UPS]
# the same kernel with an output stride: odd and even extents, one frame, one pixel
STRIDED_CASES = [(dims, Cin, Cout, st) for st in ((1, 2), (2, 2), (2, 1)) for dims in ((1, 1, 1), (2, 2, 2), (3, 1, 5), (4, 8, 7), (5, 9, 8))
                 for Cin in (64, 128) for Cout in (64, 136)]
# the three-output kernel (8 x 32 pixel patches): one pixel, an exact patch, one short, one past, several patches ragged both ways;
# Cin = 192 is outside its range and takes the tile kernel with three output channels
OUT3_CASES = [(dims, Cin) for Cin in (64, 128) for dims in ((1, 1, 1), (3, 8, 32), (2, 7, 31), (2, 9, 33), (4, 17, 70))] + [((2, 9, 33), 192)]
# the four-wave kernel (>= 256 tiles of 256 rows x Cout / bn each): (form, dims, Cin, Cout, up); halo = output frames of whole 8 x 32 patches
W4_CASES = [("halo", (8, 64, 128), 128, 128, (1, 1)), ("halo", (8, 32, 64), 256, 128, (1, 2)), ("halo", (3, 44, 80), 256, 256, (2, 2)),
            ("halo", (4, 64, 128), 512, 512, (1, 1)), ("halo", (1, 256, 256), 128, 128, (1, 1)), ("halo", (1, 128, 128), 128, 128, (2, 2)),
            ("gather", (5, 113, 127), 128, 128, (1, 1)), ("gather", (4, 65, 66), 256, 256, (1, 2))]
GUARD = 4096


def probe_case(dims, Cin, Cout, up=(1, 1), st=(1, 1)):
    """the case of one table row (also what the host test examines): seeded by the row itself; three output channels need nine
    weights each to cover the 27 taps"""
    seed = zlib.crc32(repr((dims, Cin, Cout, up, st)).encode()) & 0x7fffffff
    return make_case(*dims, Cin, Cout, seed, nnz=9 if Cout == 3 else 6, up=up, st=st)


@functools.lru_cache(maxsize=2)
def _case_and_want(dims, Cin, Cout, up, st):
    case = probe_case(dims, Cin, Cout, up, st)
    return case, int_ref(case)


def expected(key, resid):
    """(case, expected [M][Cout] int64): the reference is computed once per table row and left unchanged"""
    case, want = _case_and_want(*key)
    if resid:
        want = want + case.resid
        assert int(want.abs().max()) <= 256
    return case, want


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    from kandinsky import _engine as E
    return E.lib()


def guarded(t, fill=float("nan")):
    """t on the device in the middle of an allocation with GUARD elements of `fill` on both sides (offset: a multiple of 16 bytes)"""
    buf = torch.full((GUARD + t.numel() + GUARD,), fill, dtype=t.dtype, device="cuda")
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return buf, view


class Probe:
    """device buffers of one case; check() compares the payload bit for bit and looks at every canary and at the inputs"""

    def __init__(self, case, use_res, ldc=None):
        self.case, M, Cout = case, case.M, case.Cout
        self.ldc = ldc or Cout + 8
        self.ldr = Cout + 8
        self.xb, self.x = guarded(case.x.to(torch.bfloat16))
        self.wb, self.w = guarded(pack_weights(case))
        self.bias = case.bias.float().cuda()
        self.rb = self.r = None
        if use_res:
            r = torch.full((M, self.ldr), float("nan"), dtype=torch.bfloat16)
            r[:, :Cout] = case.resid.to(torch.bfloat16)
            self.rb, self.r = guarded(r)
        self.snap = [b.clone() for b in (self.xb, self.wb, self.rb) if b is not None]

    def fresh_out(self):
        M, Cout = self.case.M, self.case.Cout
        self.ob, self.out = guarded(torch.full((M + 64, self.ldc), 7.0, dtype=torch.bfloat16), fill=7.0)
        self.out[:M, :Cout] = float("nan")
        return self.out

    def check(self, want_int, what):
        torch.cuda.synchronize()
        case, M, Cout = self.case, self.case.M, self.case.Cout
        want = want_int.to(torch.bfloat16).cuda()
        payload = self.out[:M, :Cout]
        assert torch.equal(payload, want), f"{what}: {explain(payload, want, case)}"
        assert bool((self.out[:M, Cout:] == 7.0).all()), f"{what}: pad columns written"
        assert bool((self.out[M:] == 7.0).all()), f"{what}: rows past M written"
        assert bool((self.ob[:GUARD] == 7.0).all()) and bool((self.ob[-GUARD:] == 7.0).all()), f"{what}: written outside the output"
        for b, s in zip((b for b in (self.xb, self.wb, self.rb) if b is not None), self.snap):
            assert torch.equal(b.view(torch.int16), s.view(torch.int16)), f"{what}: an input buffer changed"

    def args(self, up_or_st):
        from kandinsky import _engine as E
        c = self.case
        return (self.x.data_ptr(), self.w.data_ptr(), self.bias.data_ptr(), self.out.data_ptr(), *c.dims, c.Cin, c.Cout, *up_or_st, self.ldc), E.stream_ptr()


@pytest.mark.parametrize("dims,Cin,Cout,up", TILE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_tile_kernel_probe(L, dims, Cin, Cout, up):
    for use_res in (False, True):
        case, want = expected((dims, Cin, Cout, up, (1, 1)), use_res)
        p = Probe(case, use_res)
        p.fresh_out()
        a, s = p.args(up)
        assert L.k5_conv3d_bf16(*a, p.r.data_ptr() if use_res else None, p.ldr, s) == 0
        p.check(want, f"resid {use_res}")


@pytest.mark.parametrize("dims,Cin,Cout,st", STRIDED_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_strided_probe(L, dims, Cin, Cout, st):
    case, want = expected((dims, Cin, Cout, (1, 1), st), False)
    p = Probe(case, False)
    p.fresh_out()
    a, s = p.args(st)
    assert L.k5_conv3d_strided_bf16(*a, s) == 0
    p.check(want, "strided")


@pytest.mark.parametrize("dims,Cin", OUT3_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_three_output_probe(L, dims, Cin):
    case, want = expected((dims, Cin, 3, (1, 1), (1, 1)), False)
    p = Probe(case, False, ldc=8)
    p.fresh_out()
    a, s = p.args((1, 1))
    assert L.k5_conv3d_bf16(*a, None, 0, s) == 0
    p.check(want, "out3")


@pytest.mark.parametrize("use_res", [False, True], ids=["plain", "resid"])
@pytest.mark.parametrize("form,dims,Cin,Cout,up", W4_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_four_wave_probe(L, form, dims, Cin, Cout, up, use_res):
    """the statistics variant first: its status 0 is the proof, on the machine at hand, that the shape is in the four-wave range (6 = it
    is not), so the plain call that follows runs the same kernel without the statistics.  quad_stats must equal the per-block sums of
    the expected output element for element: a sum that lands in the neighbouring block does not cancel here."""
    case, want = expected((dims, Cin, Cout, up, (1, 1)), use_res)
    To, Ho, Wo = case.grid
    assert (form == "halo") == (Ho % 8 == 0 and Wo % 32 == 0)
    assert (case.M + 255) // 256 * (Cout // (128 if Cout == 128 else 256)) >= 256
    p = Probe(case, use_res)
    assert p.ldc % 8 == 0 and p.ldr % 4 == 0                 # or the launcher leaves the four-wave kernel
    n_stats = L.k5_conv3d_stats_size(case.M, Cout) // 4
    want_stats = block_stats_ref(want, case.M, Cout, case.grid if form == "halo" else None)
    assert want_stats.numel() == n_stats
    qb, qs = guarded(torch.full((n_stats,), float("nan")), fill=7.0)
    p.fresh_out()
    a, s = p.args(up)
    rp = p.r.data_ptr() if use_res else None
    assert L.k5_conv3d_bf16_stats(*a, rp, p.ldr, qs.data_ptr(), s) == 0, "outside the four-wave kernel's range on this machine"
    p.check(want, "stats variant")
    got_stats = qs.view(want_stats.shape).cpu()
    bad = (got_stats != want_stats).nonzero()
    assert torch.equal(got_stats, want_stats), (f"{len(bad)} statistics differ; first [block, quad, sum|sq] = {bad[0].tolist()}: got "
                                                f"{float(got_stats[tuple(bad[0])])}, want {float(want_stats[tuple(bad[0])])}")
    assert bool((qb[:GUARD] == 7.0).all()) and bool((qb[-GUARD:] == 7.0).all()), "written outside quad_stats"
    p.fresh_out()
    a, s = p.args(up)
    assert L.k5_conv3d_bf16(*a, rp, p.ldr, s) == 0
    p.check(want, "plain variant")


def test_refused_calls_launch_nothing(L):
    """Cin % 64 != 0 is K5_ERR_ALIGN; a factor outside {1, 2} is K5_ERR_ARG, for the upsample, the stride and the statistics entry alike;
    the payload keeps its fill.  (An upsample together with a stride is K5_ERR_ARG in the launcher, but no exported entry can ask for it:
    k5_conv3d_bf16 has no stride and k5_conv3d_strided_bf16 no upsample.)"""
    from kandinsky import _engine as E
    x = torch.zeros(2 * 4 * 4 * 128, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(128 * 27 * 128, dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(128, device="cuda")
    out = torch.full((4 * 8 * 8 * 136,), 7.0, dtype=torch.bfloat16, device="cuda")
    qs = torch.full((4096,), 7.0, device="cuda")
    s = E.stream_ptr()
    head = (x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), 2, 4, 4)
    assert L.k5_conv3d_bf16(*head, 96, 128, 1, 1, 136, None, 0, s) == 2
    assert L.k5_conv3d_strided_bf16(*head, 32, 128, 2, 2, 136, s) == 2
    for up in ((3, 1), (1, 3), (0, 1), (1, 0), (1, 4), (-1, 2)):
        assert L.k5_conv3d_bf16(*head, 128, 128, *up, 136, None, 0, s) == 1, up
        assert L.k5_conv3d_strided_bf16(*head, 128, 128, *up, 136, s) == 1, up
        assert L.k5_conv3d_bf16_stats(*head, 128, 128, *up, 136, None, 0, qs.data_ptr(), s) == 1, up
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((qs == 7.0).all())
