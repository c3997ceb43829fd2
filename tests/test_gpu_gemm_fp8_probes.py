"""Integer-exact probes of every path of the e4m3 GEMM (k5_gemm_fp8 / k5_gemm_fp8_ex: the 8-wave and the 4-wave persistent kernel of
gemm_fp8.hip, their three epilogues, bias and the per-row scale of the operand-swapped V^T projection) and of k5_quant_rows_fp8.
Operands, scales, bias, residual and gate come from tests/gemm_fp8_probe_reference.py, where the expected output is ONE bit pattern:
every comparison here is torch.equal on bits, there is no tolerance in this file (+0 and -0 of an e4m3 byte count as the same value).

Buffers: every buffer sits between 4096 guard elements inside a larger allocation.  Outputs are [M + 64][ldc] with the payload NaN (bf16)
or 0x7f (e4m3) — an unwritten element fails the comparison — and the pad columns, the 64 rows past M and the guards a sentinel that must
survive.  A8 and W8 have lda = K + 16 and ldw = K + 128; pad columns, 160 rows past the last one and the guards hold the e4m3 NaN byte: a
NaN operand poisons its whole output row, so a NaN in a kept output is a misread.  (160 rows: the four-wave kernel's DMA keeps a piece's row
offset in the buffer instruction's scalar offset, next to the range-checked vector offset; rows up to 143 past the first of a ragged tile
may be fetched into accumulator rows that are never stored, and stay inside the allocation here.)  Every launch is made three times into
freshly poisoned outputs and each result compared: the race screen of the multi-tile rows.

Every row asserts which kernel the launcher picks on the machine at hand (tiles >= CUs, the w4_ok terms) — it cannot pass on the other one.
tests/test_gemm_fp8_probe_host.py proves on the CPU that each small case tells the right indexing from the wrong ones."""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gemm_fp8_probe_reference as R  # noqa: E402
from gemm_fp8_probe_reference import EPI_BIAS, EPI_GATE, EPI_GELU  # noqa: E402

BF = torch.bfloat16
GUARD = 4096
OPERAND_GUARD_ROWS = 160
OUT_ROWS_PAST = 64
SENTINEL_BF, SENTINEL_U8 = 7.0, 0x55
EPIS = [EPI_BIAS, EPI_GELU, EPI_GATE]
epi_id = lambda e: R.EPI_NAMES[e]
shape_id = lambda s: "x".join(map(str, s))


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


def embed(t, ld=None, rows_past=0, fill=float("nan")):
    """t ([rows][cols] or a vector) on the device as the top left corner of [rows + rows_past][ld], everything else `fill`, with GUARD
    elements of `fill` on both sides (offset: a multiple of 16 bytes).  Returns (whole allocation, the [rows + rows_past][ld] view)."""
    t2 = t if t.dim() == 2 else t[None, :]
    rows, cols = t2.shape
    ld = ld or cols
    n = (rows + rows_past) * ld
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=t.dtype, device="cuda")
    view = buf[GUARD:GUARD + n].view(rows + rows_past, ld)
    view[:rows, :cols] = t2.cuda()
    assert view.data_ptr() % 16 == 0
    return buf, view


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Probe:
    """device buffers of one case; run() launches into a fresh poisoned output, check() compares the payload bit for bit and looks at
    every sentinel and at the inputs"""

    def __init__(self, case):
        self.case = case
        self.lda, self.ldw, self.ldr = case.K + 16, case.K + 128, case.N + 12
        self.ab, self.a = embed(R.int_to_e4m3(case.A), self.lda, OPERAND_GUARD_ROWS, R.E4M3_NAN)
        self.wb, self.w = embed(R.int_to_e4m3(case.W), self.ldw, OPERAND_GUARD_ROWS, R.E4M3_NAN)
        self.sb, self.s = embed(case.scale)
        self.bb, self.b = embed(case.bias)
        self.gb, self.g = embed(case.gate)
        self.rb, self.r = embed(case.resid, self.ldr)
        self.inputs = (self.ab, self.wb, self.sb, self.bb, self.gb, self.rb)
        self.snap = [b.clone() for b in self.inputs]

    def run(self, L, epi, ldc, use_bias=False, ex=False, inplace=False):
        c = self.case
        assert ldc >= c.N
        u8 = epi == EPI_GELU
        self.fill = SENTINEL_U8 if u8 else SENTINEL_BF
        blank = torch.full((c.M, c.N), R.E4M3_NAN, dtype=torch.uint8) if u8 else torch.full((c.M, c.N), float("nan"), dtype=BF)
        self.ob, self.out = embed(c.resid if inplace else blank, ldc, OUT_ROWS_PAST, self.fill)
        resid, ldr, gate = None, 0, None
        if epi == EPI_GATE:
            resid, ldr, gate = (self.out.data_ptr(), ldc, self.g.data_ptr()) if inplace else (self.r.data_ptr(), self.ldr, self.g.data_ptr())
        head = (self.a.data_ptr(), self.w.data_ptr(), self.s.data_ptr(), self.out.data_ptr(), c.M, c.N, c.K, self.lda, self.ldw, ldc, epi,
                resid, ldr, gate, stream())
        if ex:
            return L.k5_gemm_fp8_ex(*head, self.b.data_ptr() if use_bias else None, int(c.scale_m))
        assert not use_bias and not c.scale_m
        return L.k5_gemm_fp8(*head)

    def check(self, want, what):
        torch.cuda.synchronize()
        c, M, N = self.case, self.case.M, self.case.N
        payload = bits(self.out[:M, :N])
        same = R.same_up_to_zero_sign(payload, want) if payload.dtype == torch.uint8 else torch.equal(payload, want)
        assert same, f"{what}: {R.explain(payload, want, c)}"
        assert bool((self.out[:M, N:] == self.fill).all()), f"{what}: pad columns written"
        assert bool((self.out[M:] == self.fill).all()), f"{what}: rows past M written"
        assert bool((self.ob[:GUARD] == self.fill).all()) and bool((self.ob[-GUARD:] == self.fill).all()), f"{what}: written outside the output"
        for b, s in zip(self.inputs, self.snap):
            assert torch.equal(bits(b), bits(s)), f"{what}: an input buffer changed"


@functools.lru_cache(maxsize=2)
def case_and_probe(M, N, K, kind, a_tile=None):
    """the case of a table row and its device buffers, made once and left unchanged"""
    case = R.probe_case(M, N, K, kind, a_tile)
    return case, Probe(case)


@functools.lru_cache(maxsize=2)
def want_bits(M, N, K, kind, a_tile, epi, use_bias):
    case, _ = case_and_probe(M, N, K, kind, a_tile)
    return R.int_ref(case, epi, use_bias).cuda()


def assert_kernel(kernel, forced, M, N, K, ldc, ldr, epi):
    """the row's precondition: which kernel the launcher's rule (launch_f8 in gemm_fp8.hip) picks for these arguments"""
    ok = R.w4_ok(M, N, K, ldc, ldr, epi)
    if forced is None:
        assert not os.environ.get("K5_GEMM_FP8_V"), "K5_GEMM_FP8_V overrides the selection these rows rely on"
        picks_w4 = ok and R.tiles(M, N) >= cus()
    else:
        assert os.environ.get("K5_GEMM_FP8_V") == str(forced)
        picks_w4 = ok and forced == 4
    assert picks_w4 == (kernel == "w4"), (f"{M}x{N}x{K} ldc {ldc} ldr {ldr} {R.EPI_NAMES[epi]}: expected the {kernel} kernel, the launcher takes "
                                          f"{'w4' if picks_w4 else 'k8'} ({R.tiles(M, N)} tiles, {cus()} CUs, w4_ok {ok})")


def run_row(L, shape, epi, ldc, kernel, use_bias=False, ex=False, kind=None, a_tile=None, forced=None):
    """one table row: every form of the epilogue, three launches each into fresh poisoned outputs"""
    M, N, K = shape
    kind = kind or ("gelu" if epi == EPI_GELU else "int")
    case, p = case_and_probe(M, N, K, kind, a_tile)
    want = want_bits(M, N, K, kind, a_tile, epi, use_bias)
    for inplace in ((True, False) if epi == EPI_GATE else (False,)):
        assert_kernel(kernel, forced, M, N, K, ldc, ldc if inplace else p.ldr, epi)
        assert not inplace or p.ldr != ldc
        for rep in range(3):
            assert p.run(L, epi, ldc, use_bias, ex, inplace) == 0
            p.check(want, f"{R.EPI_NAMES[epi]}{' in place' if inplace else ''} ldc {ldc} bias {use_bias} launch {rep}")


# ------------------------------------------------------------------------------------------------ the 8-wave kernel
@pytest.mark.parametrize("epi", EPIS, ids=epi_id)
@pytest.mark.parametrize("shape", R.K8_ONE_TILE, ids=shape_id)
def test_k8_one_tile(L, shape, epi):
    """nk = 2 (the launcher's minimum: the prologue's second W half is already the last K-tile), nk odd (the single trailing K-tile on
    stage 0), nk = 5"""
    run_row(L, shape, epi, shape[1] + 8, "k8")


@pytest.mark.parametrize("epi", EPIS, ids=epi_id)
@pytest.mark.parametrize("pad", [3, 4], ids=["scalar-stores", "vector-stores"])
@pytest.mark.parametrize("shape", R.K8_RAGGED, ids=shape_id)
def test_k8_ragged(L, shape, pad, epi):
    """clamped operand rows, one row, one and three columns (N < 4: no vector store at all), N = 255 (the last store group is partial);
    ldc & 3 != 0 takes the element-wise stores everywhere"""
    run_row(L, shape, epi, shape[1] + pad, "k8")


@pytest.mark.parametrize("epi", EPIS, ids=epi_id)
@pytest.mark.parametrize("shape", R.K8_WALK, ids=shape_id)
def test_k8_tile_walk(L, shape, epi):
    """2 tiles (six of eight XCD slices idle); 5 x 3 tiles (the last m-group is one tile tall); 272 tiles with odd nk — more tiles than
    workgroups, so some workgroups issue the next tile's prologue under the epilogue, and odd nk keeps the 4-wave kernel out"""
    M, N, K = shape
    if R.tiles(M, N) > 16:
        assert R.tiles(M, N) > cus(), "no workgroup runs a second tile on this machine"
    run_row(L, shape, epi, N + 8, "k8")


@pytest.mark.parametrize("epi", EPIS, ids=epi_id)
def test_k8_takes_the_rows_the_w4_kernel_cannot_store(L, epi):
    """the 4-wave kernel's first natural row at ldc = N + 8: rows that are not 16-element aligned leave it (the ldc term of w4_ok), so
    the 8-wave kernel walks 272 tiles with an even nk, a second tile on some workgroups"""
    M, N, K = R.W4_NATURAL[0]
    assert R.tiles(M, N) > cus() and R.w4_ok(M, N, K, N + 16, N + 12, epi) and not R.w4_ok(M, N, K, N + 8, N + 12, epi)
    run_row(L, (M, N, K), epi, N + 8, "k8")


# ------------------------------------------------------------------------------------------------ the 4-wave kernel
@pytest.mark.parametrize("epi", EPIS, ids=epi_id)
@pytest.mark.parametrize("shape", R.W4_NATURAL, ids=shape_id)
def test_w4_natural_selection(L, shape, epi):
    """272 tiles: ragged M at nk = 4 (the minimum: the DMA cursor wraps onto the next tile inside the first K-tile pair), and a last N
    tile of 16 columns; some workgroups run a second tile"""
    M, N, K = shape
    assert R.tiles(M, N) > cus(), "no workgroup runs a second tile on this machine"
    run_row(L, shape, epi, N + 16, "w4")


def forced_rows(L, forced):
    """what a child process runs under K5_GEMM_FP8_V=forced: the small shapes on either kernel, and on the 4-wave kernel its K-tile
    signature rows.  The expected bits are the same for both kernels."""
    kernel = "w4" if forced == 4 else "k8"
    n = 0
    for shape in R.FORCED:
        for epi in EPIS:
            run_row(L, shape, epi, shape[1] + 16, kernel, forced=forced)
            n += 1
    if forced == 4:
        for shape in R.SIGNATURE_W4:
            for t in R.signature_tiles(shape[2]):
                run_row(L, shape, EPI_BIAS, shape[1] + 16, kernel, a_tile=t, forced=forced)
                n += 1
    return n


@pytest.mark.parametrize("forced", [4, 8])
def test_forced_kernel_in_a_child_process(forced):
    """K5_GEMM_FP8_V is read once per process, hence a fresh child per value (one at a time, each with its own time limit): the small
    shapes (2, 6 and 12 tiles, ragged M, N = 272 and 528) on the 4-wave kernel, which natural selection only reaches from one tile per CU
    up, and the same rows on the 8-wave kernel against the same bits"""
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_gemm_fp8_probes as T; from kandinsky import _engine as E; "
            "print('PROBE_OK', T.forced_rows(E.lib(), %d))" % (HERE, os.path.join(os.path.dirname(HERE), "kandinsky-5_amd"), forced))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, K5_GEMM_FP8_V=str(forced)), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-1500:] + out.stderr[-3000:])
    rows = 3 * len(R.FORCED) + (sum(len(R.signature_tiles(s[2])) for s in R.SIGNATURE_W4) if forced == 4 else 0)
    assert f"PROBE_OK {rows}" in out.stdout, out.stdout[-1500:]


# ------------------------------------------------------------------------------------------------ bias and the per-row scale
@pytest.mark.parametrize("shape,pad,kernel", [(R.SCALE_M_K8[0], 4, "k8"), (R.SCALE_M_K8[0], 3, "k8"), (R.SCALE_M_K8[1], 3, "k8"), (R.SCALE_M_K8[1], 8, "k8"),
                                              (R.SCALE_M_W4[0], 16, "w4")], ids=lambda v: shape_id(v) if isinstance(v, tuple) else str(v))
def test_scale_m_with_bias(L, shape, pad, kernel):
    """the operand-swapped V^T projection as the engine calls it: weight rows as M, tokens as N, scale and bias per output ROW"""
    for use_bias in (True, False):
        run_row(L, shape, EPI_BIAS, shape[1] + pad, kernel, use_bias=use_bias, ex=True, kind="scale_m")


@pytest.mark.parametrize("epi", EPIS, ids=epi_id)
@pytest.mark.parametrize("shape,pad,kernel", [(R.BIAS_N_K8, 3, "k8"), (R.BIAS_N_K8, 4, "k8"), (R.BIAS_N_W4, 16, "w4")],
                         ids=lambda v: shape_id(v) if isinstance(v, tuple) else str(v))
def test_bias_per_column(L, shape, pad, kernel, epi):
    """bias per output column under every epilogue (it enters before the bf16 rounding that GELU and the gate see)"""
    run_row(L, shape, epi, shape[1] + pad, kernel, use_bias=True, ex=True)


@pytest.mark.parametrize("shape,pad,kernel", [((300, 130, 384), 3, "k8"), ((4100, 4096, 512), 16, "w4")], ids=lambda v: shape_id(v) if isinstance(v, tuple) else str(v))
def test_ex_without_bias_is_the_plain_entry(L, shape, pad, kernel):
    M, N, K = shape
    for epi in (EPI_BIAS, EPI_GATE, EPI_GELU):
        case, p = case_and_probe(M, N, K, "gelu" if epi == EPI_GELU else "int")
        assert_kernel(kernel, None, M, N, K, N + pad, p.ldr, epi)
        assert p.run(L, epi, N + pad) == 0
        torch.cuda.synchronize()
        plain = p.ob.clone()
        assert p.run(L, epi, N + pad, ex=True) == 0
        torch.cuda.synchronize()
        assert torch.equal(bits(p.ob), bits(plain)), R.EPI_NAMES[epi]
        p.check(want_bits(M, N, K, "gelu" if epi == EPI_GELU else "int", None, epi, False), R.EPI_NAMES[epi])


# ------------------------------------------------------------------------------------------------ K-tile signatures
@pytest.mark.parametrize("shape", R.SIGNATURE_K8, ids=shape_id)
def test_k8_k_tile_signature(L, shape):
    """A is nonzero in one K-tile only and W differs from K-tile to K-tile: a K-tile that is dropped, fetched twice or taken from a
    neighbouring offset (what a wrong clamp of the tail DMA would do) gives a different output in every element that is not zero"""
    for t in R.signature_tiles(shape[2]):
        run_row(L, shape, EPI_BIAS, shape[1] + 8, "k8", a_tile=t)


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_calls_launch_nothing(L):
    case, p = case_and_probe(256, 256, 256, "int")
    out = torch.full((320 * 264,), SENTINEL_BF, dtype=BF, device="cuda")
    a, w, s, b, g, r, o = (t.data_ptr() for t in (p.a, p.w, p.s, p.b, p.g, p.r, out))
    st = stream()
    lda, ldw, ldr = p.lda, p.ldw, p.ldr

    def call(M=256, N=256, K=256, lda=lda, ldw=ldw, epi=EPI_BIAS, scale=s, resid=None, gate=None, scale_m=0):
        return L.k5_gemm_fp8_ex(a, w, scale, o, M, N, K, lda, ldw, 264, epi, resid, ldr, gate, st, b, scale_m)
    assert call() == 0                                                       # the arguments the refusals below vary are valid
    out.fill_(SENTINEL_BF)
    for kw in (dict(K=128), dict(K=300), dict(K=320), dict(lda=lda + 8), dict(ldw=ldw + 8)):
        assert call(**kw) == 2, kw                                           # K5_ERR_ALIGN
    for kw in (dict(scale_m=1, epi=EPI_GELU), dict(scale_m=1, epi=EPI_GATE, resid=r, gate=g), dict(epi=EPI_GATE, gate=g), dict(epi=EPI_GATE, resid=r),
               dict(scale=None), dict(M=0), dict(N=0), dict(M=-1), dict(N=-256), dict(epi=1)):
        assert call(**kw) == 1, kw                                           # K5_ERR_ARG
    assert L.k5_gemm_fp8(a, w, s, o, 256, 256, 128, lda, ldw, 264, EPI_BIAS, None, 0, None, st) == 2
    assert L.k5_gemm_fp8(a, w, s, o, 256, 256, 256, lda, ldw, 264, EPI_GATE, None, 0, None, st) == 1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL_BF).all())


# ------------------------------------------------------------------------------------------------ the row quantiser
def quantise(L, x, per_row, rows=None):
    """x bf16 [rows][K] at ldx = K + 4 (pads NaN) -> codes at ldo = K + 8 and the scales, each with four sentinel rows below"""
    rows, K = (rows or x.shape[0]), x.shape[1]
    xb, xv = embed(x, K + 4)
    ob, ov = embed(torch.full((rows, K), R.E4M3_NAN, dtype=torch.uint8), K + 8, 4, SENTINEL_U8)
    sb, sv = embed(torch.full((rows,), float("nan")), rows + 4, 0, SENTINEL_BF)
    snap = xb.clone()
    assert L.k5_quant_rows_fp8(xv.data_ptr(), ov.data_ptr(), sv.data_ptr() if per_row else None, rows, K, K + 4, K + 8, stream()) == 0
    torch.cuda.synchronize()
    assert bool((ov[:rows, K:] == SENTINEL_U8).all()) and bool((ov[rows:] == SENTINEL_U8).all()), "codes written outside [rows][K]"
    assert bool((ob[:GUARD] == SENTINEL_U8).all()) and bool((ob[-GUARD:] == SENTINEL_U8).all())
    assert bool((sv[0, rows:] == SENTINEL_BF).all()) and bool((sb[:GUARD] == SENTINEL_BF).all()) and bool((sb[-GUARD:] == SENTINEL_BF).all()), "scales written past `rows`"
    assert torch.equal(bits(xb), bits(snap))
    return ov[:rows, :K].cpu(), sv[0, :rows].cpu()


def first_diff(got, want):
    z = lambda t: torch.where(t == 0x80, torch.zeros_like(t), t)
    bad = (z(got) != z(want)).nonzero()
    return "equal" if len(bad) == 0 else f"{len(bad)} codes differ; first at (row, k) = {bad[0].tolist()}: got 0x{int(got[tuple(bad[0])]):02x}, want 0x{int(want[tuple(bad[0])]):02x}"


@pytest.mark.parametrize("rows", [1, 5])
def test_quantiser_static_scale(L, rows):
    """scale == nullptr: the RNE, saturating e4m3 of the bf16 value — zeros, ties, every subnormal, +-448 and everything beyond"""
    v, _ = R.quant_static_rows()
    K = (len(v) + 3) // 4 * 4 + 4
    x = torch.zeros(rows, K, dtype=BF)
    for r in range(rows):
        x[r, :len(v)] = v
        x[r] = x[r].roll(7 * r)                                   # the same values in other lanes and other dwords
    codes, scale = quantise(L, x, per_row=False)
    want = R.quant_static_ref(x)
    assert R.same_up_to_zero_sign(codes, want), first_diff(codes, want)
    assert bool(torch.isnan(scale).all()), "a scale was written under the static scale"


@pytest.mark.parametrize("K", [4, 252, 256, 260, 1792])
@pytest.mark.parametrize("rows", [1, 4, 5, 7])
def test_quantiser_per_row_scale(L, rows, K):
    """the rows % 4 tail of the last workgroup, K < 256 (idle lanes) and partial last chunks, strides; scale within 2 fp32 ulps of
    max|x| / 448 (one rounding of 1 / 448, one of the product), exactly 1 for a zero row; codes = e4m3(fp32(x * fp32(1 / scale)))"""
    for shift in (range(6) if rows == 1 else (0, 3)):
        x, kinds = R.quant_rows_case(rows, K, shift, R.seed_of(rows, K, shift))
        codes, scale = quantise(L, x, per_row=True)
        mx = x.double().abs().amax(1)
        ref = torch.where(mx > 0, mx / 448.0, torch.ones_like(mx)).float()
        print(f"rows {rows} K {K} shift {shift}: scale ulps off {R.ulps_apart(scale, ref).tolist()}")
        assert bool((scale > 0).all()) and bool(torch.isfinite(scale).all())
        assert bool((R.ulps_apart(scale, ref) <= 2).all()), (scale.tolist(), ref.tolist())
        for r, kind in enumerate(kinds):
            if kind == 1:
                assert float(scale[r]) == 1.0 and bool((codes[r] & 0x7f == 0).all()), "zero row"
        want = R.quant_row_ref(x, scale)
        assert R.same_up_to_zero_sign(codes, want), f"kinds {kinds}: {first_diff(codes, want)}"
        nz = mx > 0
        assert bool((codes[nz].view(R.F8).float().abs().amax(1) == 448.0).all()), "a row's maximum is not the code 448"


def test_quantiser_gemm_round_trip(L):
    """integer activations through the static quantiser, weights +-2^p (row maximum a power of two, so every w * 448 / max is an e4m3 value)
    through the per-row quantiser, then k5_gemm_fp8: the product of the integer matrices, exactly.  (acc * scale = S * 448 fl(1 / 448) is
    within 2^-21 of S relative, S has at most 8 significant bits: the bf16 rounding returns S.)"""
    M, N, K = 300, 130, 256
    g = torch.Generator().manual_seed(R.seed_of("round trip"))
    A = (torch.randint(-3, 4, (M, K), generator=g) * (torch.rand(M, K, generator=g) < 0.125)).float()
    p = torch.randint(0, 3, (N, K), generator=g)
    Wt = ((torch.randint(0, 2, (N, K), generator=g) * 2 - 1) * 2.0 ** p * (torch.rand(N, K, generator=g) < 0.125)).float()
    Wt[:, 0] = 4.0
    Wt *= 2.0 ** (torch.arange(N) % 3 - 1).float()[:, None]
    S = A.double() @ Wt.double().t()
    assert torch.equal(S.to(BF).double(), S), "the product must be exact in bf16"
    a8, _ = quantise(L, A.to(BF), per_row=False)
    w8, ws = quantise(L, Wt.to(BF), per_row=True)
    assert torch.equal(a8.view(R.F8).float(), A) and torch.equal(w8.view(R.F8).float(), Wt * (448.0 / Wt.abs().amax(1))[:, None])
    ad, wd, sd = a8.cuda(), w8.cuda(), ws.cuda()
    out = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    assert L.k5_gemm_fp8(ad.data_ptr(), wd.data_ptr(), sd.data_ptr(), out.data_ptr(), M, N, K, K, K, N, EPI_BIAS, None, 0, None, stream()) == 0
    torch.cuda.synchronize()
    want = S.to(BF)
    assert torch.equal(bits(out.cpu()), bits(want)), R.explain(bits(out.cpu()), bits(want))
