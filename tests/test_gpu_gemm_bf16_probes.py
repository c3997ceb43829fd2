"""Integer-exact probes of every path of the bf16 GEMM (k5_gemm_bf16_variant / k5_gemm_bf16_f32out: the five kernels of gemm_bf16.hip, their
five epilogues, the launcher's choices).  Operands, bias, residual and gate come from tests/gemm_bf16_probe_reference.py, where the expected
output is ONE bit pattern: every comparison here is torch.equal on bits, there is no tolerance in this file (+0 and -0 count as the same
value under GELU only).

Buffers: every buffer sits between 4096 guard elements inside a larger allocation.  Outputs are [M + 64][ldc] with the payload NaN — an
unwritten element fails the comparison — and the pad columns, the 64 rows past M and the guards a sentinel that must survive.  A and W have
lda = K + 8 and ldw = K + 72; pad columns, 160 rows past the last one and the guards are NaN: a NaN operand poisons its whole output row or
column, so a NaN in a kept output is a misread.  (160 rows: the four-wave and the q4 kernel keep a DMA piece's row offset in the buffer
instruction's scalar offset, next to the range-checked lane offset; up to 143 rows past the last valid one of a ragged tile are fetched into
accumulator rows that are never stored — R.w4_dma_rows — and stay inside the allocation here.)  The inputs are compared with a snapshot after
every launch, and every launch is made three times into freshly poisoned outputs: the race screen of the multi-tile rows.

Every row asserts with the launcher mirror of the reference module which kernel, tile height and tail form the launcher takes on the machine
at hand — it cannot pass on another path.  tests/test_gemm_bf16_probe_host.py proves on the CPU that the cases tell right from wrong."""
import collections
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gemm_bf16_probe_reference as R  # noqa: E402
from gemm_bf16_probe_reference import EPI_BIAS, EPI_BIAS_M, EPI_F32, EPI_GATE, EPI_GELU  # noqa: E402

BF = torch.bfloat16
GUARD = 4096
OUT_ROWS_PAST = 64
SENTINEL = 7.0
TALLY = collections.Counter()          # (kernel, rows, tail, epilogue) -> launches checked
RAN = set()


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    from kandinsky import _engine as E
    return E.lib()


def stream():
    from kandinsky import _engine as E
    return E.stream_ptr()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def embed(t, ld=None, rows_past=0, fill=float("nan"), col0=0):
    """t ([rows][cols] or a vector) on the device at columns col0 .. of [rows + rows_past][ld], everything else `fill`, with GUARD elements of
    `fill` on both sides.  Returns (whole allocation, the [rows + rows_past][ld] view, the payload view)."""
    t2 = t if t.dim() == 2 else t[None, :]
    rows, cols = t2.shape
    ld = ld or cols
    assert ld >= col0 + cols and col0 % 8 == 0
    n = (rows + rows_past) * ld
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=t.dtype, device="cuda")
    view = buf[GUARD:GUARD + n].view(rows + rows_past, ld)
    payload = view[:rows, col0:col0 + cols]
    payload.copy_(t2)
    assert payload.data_ptr() % 16 == 0
    return buf, view, payload


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Probe:
    """device buffers of one case; run() launches into a fresh poisoned output, check() compares the payload bit for bit and looks at every
    sentinel and at the inputs"""

    def __init__(self, case, ldr, off=0):
        self.case, self.off = case, off
        self.lda, self.ldw, self.ldr = case.K + R.LDA_PAD + off, case.K + R.LDW_PAD, ldr + off
        self.ab, _, self.a = embed(case.A.to(BF), self.lda, R.OPERAND_GUARD_ROWS, col0=off)
        self.wb, _, self.w = embed(case.W.to(BF), self.ldw, R.OPERAND_GUARD_ROWS)
        self.bb, _, self.b = embed(case.bias)
        self.mb, _, self.bm = embed(case.bias_m)
        self.gb, _, self.g = embed(case.gate)
        self.inputs = [self.ab, self.wb, self.bb, self.mb, self.gb]
        self.snap = [b.clone() for b in self.inputs]

    @functools.cached_property
    def r(self):
        """the residual, on the device from its first use on"""
        rb, _, r = embed(self.case.resid, self.ldr, col0=self.off)
        self.inputs.append(rb)
        self.snap.append(rb.clone())
        return r

    def out_buffer(self, init, ldc, dtype):
        c = self.case
        assert ldc >= c.N + self.off
        self.ob, self.out, self.payload = embed(init.to(dtype), ldc, OUT_ROWS_PAST, SENTINEL, col0=self.off)

    def run(self, L, epi, ldc, use_bias, inplace, kernel, tile):
        c = self.case
        blank = c.resid if inplace else torch.full((c.M, c.N), float("nan"), dtype=BF)
        self.out_buffer(blank, ldc, BF)
        resid, ldr, gate = None, 0, None
        if epi == EPI_GATE:
            resid, ldr, gate = (self.payload.data_ptr(), ldc, self.g.data_ptr()) if inplace else (self.r.data_ptr(), self.ldr, self.g.data_ptr())
        bias = (self.bm if epi == EPI_BIAS_M else self.b).data_ptr() if use_bias else None
        return L.k5_gemm_bf16_variant(self.a.data_ptr(), self.w.data_ptr(), bias, self.payload.data_ptr(), c.M, c.N, c.K, self.lda, self.ldw, ldc, epi,
                                      resid, ldr, gate, stream(), kernel, tile)

    def run_f32(self, L, ldc, hw):
        c = self.case
        self.out_buffer(torch.full((c.M, c.N), float("nan")), ldc, torch.float32)
        return L.k5_gemm_bf16_f32out(self.a.data_ptr(), self.w.data_ptr(), self.payload.data_ptr(), c.M, c.N, c.K, self.lda, self.ldw, ldc, R.ALPHA, hw, stream())

    def check(self, want, what, explain):
        torch.cuda.synchronize()
        c, M, N, off = self.case, self.case.M, self.case.N, self.off
        got = bits(self.payload)
        same = R.same_up_to_zero_sign(got, want) if c.kind == "gelu" else torch.equal(got, want)
        assert same, f"{what}: {explain(got)}"
        assert bool((self.out[:M, off + N:] == SENTINEL).all()) and bool((self.out[:M, :off] == SENTINEL).all()), f"{what}: pad columns written"
        assert bool((self.out[M:] == SENTINEL).all()), f"{what}: rows past M written"
        assert bool((self.ob[:GUARD] == SENTINEL).all()) and bool((self.ob[-GUARD:] == SENTINEL).all()), f"{what}: written outside the output"
        for b, s in zip(self.inputs, self.snap):
            assert torch.equal(bits(b), bits(s)), f"{what}: an input buffer changed"


@functools.lru_cache(maxsize=2)
def case_and_probe(M, N, K, kind, a_tile, ldr, off=0):
    """the case of a table row and its device buffers, made once and left unchanged"""
    case = R.probe_case(M, N, K, kind, a_tile)
    return case, Probe(case, ldr, off)


@functools.lru_cache(maxsize=4)
def want_bits(M, N, K, kind, a_tile, epi, use_bias):
    return R.int_ref(R.probe_case(M, N, K, kind, a_tile), epi, use_bias).cuda()


def assert_plan(p, expect, what):
    assert (p.kernel, p.rows, p.tail) == tuple(expect), f"{what}: expected {expect}, the launcher takes {p} on {cus()} CUs"


def run_form(L, row, form, a_tile=None, off=0):
    """one epilogue form of a table row: the path asserted, three launches into fresh poisoned outputs"""
    name, epi, use_bias, inplace = form
    kind = "gelu" if epi == EPI_GELU else ("int" if row.sig else row.kind)
    ldc = row.N + row.pad + off
    case, p = case_and_probe(row.M, row.N, row.K, kind, a_tile, row.N + row.ldr_pad, off)
    ldr = ldc if inplace else p.ldr
    assert inplace or epi != EPI_GATE or ldr != ldc
    pl = R.plan(row.M, row.N, row.K, p.lda, p.ldw, ldc, ldr, epi, cus(), row.kernel, row.tile)
    what = f"{row.id} {name}{f' K-tile {a_tile}' if a_tile is not None else ''}"
    assert_plan(pl, row.expect, what)
    assert R.footprint_of_call(pl, row.M, row.N, row.K, p.lda, p.ldw) < R.OPERAND_GUARD_ROWS
    want = want_bits(row.M, row.N, row.K, kind, a_tile, epi, use_bias)
    for rep in range(3):
        assert p.run(L, epi, ldc, use_bias, inplace, row.kernel, row.tile) == 0
        p.check(want, f"{what} launch {rep}", lambda got: R.explain(got, want, case, pl, epi, use_bias, ldc, ldr))
    TALLY[(pl.kernel, pl.rows, pl.tail, R.EPI_NAMES[epi])] += 1
    return pl


@pytest.mark.parametrize("row", R.ALL_ROWS, ids=lambda r: r.id)
def test_table_row(L, row):
    """every epilogue form of one row of the reference module's table (R.forms_of: bias / null bias, bias per row, GELU, gated residual out of
    place and in place, with and without bias; K-tile signature rows: A nonzero in one K-tile at a time)"""
    if row.sig:
        for t in R.signature_tiles(row.K):
            run_form(L, row, R.FORMS[0], a_tile=t)
    else:
        for form in R.forms_of(row):
            run_form(L, row, form)
    RAN.add(row)


def test_second_tile_rows_run_a_second_tile(L):
    """the rows named for 'more tiles than CUs' do make some workgroup walk on to a second tile on this machine"""
    for row in R.W4_MANY + [R.HAND_ON[0]]:
        pl = R.row_plan(row, EPI_BIAS, False, cus())
        assert pl.second_tile, (row.id, pl)


# ------------------------------------------------------------------------------------------------ fp32 scores
@pytest.mark.parametrize("spec", R.F32_ROWS, ids=lambda s: "x".join(map(str, s[:3])) + f"-ldc+{s[3]}-hw{s[4]}-{s[5]}")
def test_f32_scores(L, spec):
    """alpha * A W^T in fp32, exact; under a frame-causal limit the skipped tiles keep their NaN payload and every kept element is written"""
    M, N, K, pad, hw, kernel = spec
    case, p = case_and_probe(M, N, K, "int", None, N + R.LDR_PAD)
    pl = R.plan_f32(M, N, K, p.lda, p.ldw, N + pad, hw, cus())
    assert pl.kernel == kernel, f"expected {kernel}, the launcher takes {pl} on {cus()} CUs"
    assert R.footprint_of_call(pl, M, N, K, p.lda, p.ldw) < R.OPERAND_GUARD_ROWS
    want = R.f32_ref(case, hw, pl.rows).cuda()
    if hw:
        assert bool(torch.isnan(want.view(torch.float32)).any()) and not bool(torch.isnan(want.view(torch.float32)).all())
    for rep in range(3):
        assert p.run_f32(L, N + pad, hw) == 0
        p.check(want, f"f32 {spec} launch {rep}", lambda got: R.explain(got, want, case, pl, EPI_F32))
    TALLY[(pl.kernel, pl.rows, pl.tail, "f32")] += 1


@pytest.mark.parametrize("S,C,hw,kernel", [(300, 128, 100, "glds"), (200, 72, 0, "reg")])
def test_f32_scores_of_the_halves_of_one_buffer(L, S, C, hw, kernel):
    """the VAE's mid-block attention (vae_engine.hip, mid_attention): q and k are the two halves of ONE [S][2 C] buffer, A at column 0 and W at
    column C with lda = ldw = 2 C — each operand's pad columns are the other operand, and W is a column slice"""
    case = R.probe_case(S, S, C, "int")
    qb, _, qk = embed(torch.cat([case.A, case.W], 1).to(BF), 2 * C, R.OPERAND_GUARD_ROWS)
    snap = qb.clone()
    pl = R.plan_f32(S, S, C, 2 * C, 2 * C, S + 4, hw, cus())
    assert pl.kernel == kernel
    want = R.f32_ref(case, hw, pl.rows).cuda()
    for rep in range(3):
        ob, out, payload = embed(torch.full((S, S), float("nan")), S + 4, OUT_ROWS_PAST, SENTINEL)
        assert L.k5_gemm_bf16_f32out(qk.data_ptr(), qk[:, C:].data_ptr(), payload.data_ptr(), S, S, C, 2 * C, 2 * C, S + 4, R.ALPHA, hw, stream()) == 0
        torch.cuda.synchronize()
        got = bits(payload)
        assert torch.equal(got, want), R.explain(got, want, case, pl, EPI_F32)
        assert bool((out[:S, S:] == SENTINEL).all()) and bool((out[S:] == SENTINEL).all()) and bool((ob[:GUARD] == SENTINEL).all()) and bool((ob[-GUARD:] == SENTINEL).all())
        assert torch.equal(bits(qb), bits(snap))
    TALLY[(pl.kernel, pl.rows, pl.tail, "f32")] += 1


# ------------------------------------------------------------------------------------------------ pointer offsets
@pytest.mark.parametrize("row", [R.Row(700, 511, 192, 9, 8, 0, ("k8", 192, None)), R.Row(700, 264, 512, 8, 4, 256, ("w4", 256, None), ldr_pad=12),
                                 R.Row(700, 264, 512, 8, 4, 128, ("w4", 128, None), ldr_pad=12)], ids=lambda r: r.id)
def test_operands_and_output_as_column_slices(L, row):
    """A, C and the residual as column slices of wider buffers, 512 columns in (a whole number of 16-byte chunks, as every column offset of the
    engine's callers is: they are multiples of the model width or of the VAE's attention width — test_f32_scores_of_the_halves_of_one_buffer takes
    that caller's own layout): the columns before the slice are NaN (operand) or sentinels (output)"""
    for form in [f for f in R.FORMS if f[0] in ("bias", "gelu", "gate", "gate null in place")]:
        run_form(L, row, form, off=512)


# ------------------------------------------------------------------------------------------------ 32-bit offsets
@pytest.mark.parametrize("kernel", [0, 8])
@pytest.mark.parametrize("which", ["lda", "ldw"])
def test_rows_beyond_4_gib_leave_the_8_wave_kernel(L, which, kernel):
    """a few rows at a stride that puts the last one beyond 4 GiB from the operand base: the 8-wave kernel's 32-bit lane offsets would wrap
    (onto memory of the same allocation), so the launcher hands the call to the glds kernel; expected: the exact integer product"""
    if torch.cuda.mem_get_info()[0] < 12 * 2 ** 30:
        pytest.skip("needs 12 GB of free device memory for a 4.3-GB operand")
    M, N, K = (600, 256, 128)
    case = R.probe_case(M, N, K, "int")
    rows = M if which == "lda" else N
    ld = (2 ** 32 // (2 * (rows - 1)) + 8) // 8 * 8
    assert 2 * (rows - 1) * ld > 2 ** 32 and 2 * (rows - 2) * ld < 2 ** 32
    big = torch.empty(rows * ld, dtype=BF, device="cuda")
    view = big.view(rows, ld)
    view[:, :K] = (case.A if which == "lda" else case.W).to(BF).cuda()
    _, _, other = embed((case.W if which == "lda" else case.A).to(BF), K + 8, R.OPERAND_GUARD_ROWS)
    a, w, lda, ldw = (view, other, ld, K + 8) if which == "lda" else (other, view, K + 8, ld)
    pl = R.plan(M, N, K, lda, ldw, N + 8, 0, EPI_BIAS, cus(), kernel, 0)
    assert pl.kernel == "glds" and not R.k8_fits(M, N, K, lda, ldw) and R.k8_fits(M, N, K, K + 8, K + 8)
    want = R.int_ref(case, EPI_BIAS, False).cuda()
    # wrapped offsets would misread the last row of A (output row M - 1) or of W (output column N - 1): neither may be all zero
    assert bool((want[-1] != 0).any()) and bool((want[:, -1] != 0).any())
    snaps = [(view[:, :K].clone(), view[:, :K]), (other.clone(), other)]
    for rep in range(3):
        ob, out, payload = embed(torch.full((M, N), float("nan"), dtype=BF), N + 8, OUT_ROWS_PAST, SENTINEL)
        assert L.k5_gemm_bf16_variant(a.data_ptr(), w.data_ptr(), None, payload.data_ptr(), M, N, K, lda, ldw, N + 8, EPI_BIAS, None, 0, None, stream(), kernel, 0) == 0
        torch.cuda.synchronize()
        got = bits(payload)
        assert torch.equal(got, want), f"launch {rep}: {R.explain(got, want, case, pl)}"
        assert bool((out[:M, N:] == SENTINEL).all()) and bool((out[M:] == SENTINEL).all()) and bool((ob[:GUARD] == SENTINEL).all()) and bool((ob[-GUARD:] == SENTINEL).all())
        for snap, live in snaps:
            assert torch.equal(bits(snap), bits(live)), "an input changed"
    del big, view, snaps
    torch.cuda.empty_cache()
    TALLY[(pl.kernel, pl.rows, pl.tail, "bias")] += 1


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_calls_launch_nothing(L):
    case, p = case_and_probe(512, 128, 256, "int", None, 128 + 12)
    out = torch.full((600 * 272,), SENTINEL, dtype=BF, device="cuda")
    a, w, b, g, r, o = (t.data_ptr() for t in (p.a, p.w, p.b, p.g, p.r, out))   # (W: 128 rows + 160 NaN guard rows)
    st = stream()

    def call(M=512, N=128, K=256, lda=p.lda, ldw=p.ldw, epi=EPI_BIAS, resid=None, gate=None, kernel=0, tile=0):
        return L.k5_gemm_bf16_variant(a, w, b, o, M, N, K, lda, ldw, 136, epi, resid, p.ldr, gate, st, kernel, tile)

    def f32(M=512, N=128, K=256, lda=p.lda, ldw=p.ldw, hw=0):
        return L.k5_gemm_bf16_f32out(a, w, o, M, N, K, lda, ldw, 136, R.ALPHA, hw, st)
    assert call() == 0 and call(epi=EPI_GATE, resid=r, gate=g) == 0 and f32() == 0          # the arguments the refusals below vary are valid
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    for kw in (dict(K=252), dict(K=4), dict(lda=p.lda + 4), dict(ldw=p.ldw + 4), dict(lda=p.lda + 1)):
        assert call(**kw) == 2 and f32(**kw) == 2, kw                                        # K5_ERR_ALIGN
    for kw in (dict(M=0), dict(N=0), dict(K=0), dict(M=-1), dict(N=-128), dict(K=-64)):
        assert call(**kw) == 1 and f32(**kw) == 1, kw                                        # K5_ERR_ARG
    for kw in (dict(epi=EPI_GATE, gate=g), dict(epi=EPI_GATE, resid=r), dict(epi=EPI_F32), dict(epi=7), dict(epi=-1), dict(kernel=3), dict(kernel=5),
               dict(tile=64), dict(tile=32), dict(epi=7, kernel=2), dict(epi=7, kernel=4), dict(epi=7, M=600, N=256, kernel=8)):
        assert call(**kw) == 1, kw
    assert f32(hw=-1) == 1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ tally
def test_zz_rows_per_path():
    """what ran on which kernel, tile height, tail form and epilogue; when the whole table ran, every one of them must appear"""
    for key in sorted(TALLY, key=str):
        print("rows checked", key, TALLY[key])
    if RAN != set(R.ALL_ROWS):
        return
    seen = {k[:3] for k in TALLY}
    for path in (("reg", 128, None), ("glds", 128, None), ("k8", 192, None), ("k8", 256, None), ("k8", 256, "glds"), ("w4", 256, None), ("w4", 192, None),
                 ("w4", 128, None), ("w4", 256, "q4"), ("w4", 256, "glds")):
        assert path in seen, path
        assert {k[3] for k in TALLY if k[:3] == path} >= {"bias", "bias_m", "gelu", "gate"}, path
