"""CPU reference of the integer-exact probes of the e4m3 GEMM and row quantiser (gemm_fp8.hip).  No GPU import.

The operands are small integers, which e4m3 holds exactly; the MFMA accumulates in fp32 and every partial sum stays below 2^24, so the
accumulator is the same integer in any summation order.  Scales are powers of two, bias an integer multiple of the channel's scale, the
residual integer bf16 and the gate a small dyadic number: acc * s + bias, gate * bf16(.) and the sum with the residual are all exact in
fp32 (asserted), fused or not, so the expected output of every epilogue is ONE bit pattern.

The GELU epilogue runs Abramowitz-Stegun 7.1.26 in fp32 on the device; its cases keep the pre-activations on the lattice k / 8 and only
use values whose float64 GELU is at least 16 error bounds away from every e4m3 rounding boundary (gelu_alphabet), so the byte is fixed too.

tests/test_gemm_fp8_probe_host.py examines this file on the CPU; tests/test_gpu_gemm_fp8_probes.py runs the kernels against it."""
import dataclasses
import functools
import math
import zlib

import torch

F8 = torch.float8_e4m3fn
BF = torch.bfloat16
BM, BN, BK = 256, 256, 128
EPI_BIAS, EPI_GELU, EPI_GATE = 0, 2, 3                      # kandinsky._engine.EPI_*
EPI_NAMES = {EPI_BIAS: "bias", EPI_GELU: "gelu", EPI_GATE: "gate"}
GATES = (0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 2.0, -2.0)
E4M3_NAN = 0x7f

# ------------------------------------------------------------------------------------------------ e4m3
_POS = torch.arange(127, dtype=torch.uint8).view(F8).double()     # codes 0 .. 126: 0, the subnormals k 2^-9, ... 448 (127 is NaN)
_MID = (_POS[1:] + _POS[:-1]) / 2                                  # the 126 rounding boundaries, 2^-10 (0 <-> 2^-9) first


def e4m3_rne(x):
    """codes of round-to-nearest-even, saturating at +-448 (+-inf included), of a float64 tensor without NaN; -0 keeps its sign bit"""
    x = x.double()
    assert not torch.isnan(x).any()
    a = x.abs().clamp(max=448.0)
    idx = torch.searchsorted(_MID, a.contiguous())                 # boundaries strictly below a
    tie = (idx < 126) & (_MID[idx.clamp(max=125)] == a)
    code = idx + (tie & (idx % 2 == 1)).long()                     # a tie goes to the even code = the even mantissa
    return (code + 128 * torch.signbit(x).long()).to(torch.uint8)


def e4m3_value(codes):
    return codes.view(F8).double()


def same_up_to_zero_sign(a, b):
    """byte tensors equal, with +0 (0x00) and -0 (0x80) counted as the same value"""
    z = lambda t: torch.where(t == 0x80, torch.zeros_like(t), t)
    return torch.equal(z(a), z(b))


def int_to_e4m3(ints):
    codes = ints.float().to(F8).view(torch.uint8)
    assert torch.equal(codes.view(F8).float(), ints.float()), "operand alphabet is not exact in e4m3"
    return codes


# ------------------------------------------------------------------------------------------------ GELU alphabet
GELU_STEP, GELU_MAX = 0.125, 8.0
ERF_MARGIN = 16.0


def gelu64(x):
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))       # erfc: no cancellation on the negative side


@functools.lru_cache(maxsize=1)
def gelu_alphabet():
    """(x, code, safe) over the lattice k / 8, |x| <= 8.  The device evaluates erf with |error| <= 1.5e-7 in fp32:
    |dGELU| <= 2e-7 |x| + 2^-22 |GELU(x)|.  safe: the float64 GELU lies at least 16 such bounds away from every e4m3 rounding boundary
    (the boundary 2^-10 between 0 and the first subnormal included), so any evaluation within the bound rounds to the same byte.
    The unsafe ones are the odd multiples of 1/4 from 4.75 up: GELU(x) ~ x there, which IS the boundary between two codes 1/2 apart."""
    x = torch.arange(-64, 65).double() * GELU_STEP
    g = gelu64(x)
    bound = 2e-7 * x.abs() + 2.0 ** -22 * g.abs()
    dist = (g.abs()[:, None] - _MID[None, :]).abs().min(1).values
    return x, e4m3_rne(g), dist >= ERF_MARGIN * bound


def gelu_lookup(pre):
    """pre-activations (exact multiples of 1/8 within +-8) -> (codes, safe)"""
    k = pre.double() / GELU_STEP
    assert torch.equal(k, k.round()) and float(pre.abs().max()) <= GELU_MAX, "GELU pre-activation off the lattice"
    _, code, safe = gelu_alphabet()
    i = k.long() + 64
    return code[i], safe[i]


# per scale exponent of a GELU column: (largest |pre-activation|, largest |w|) with max row sum of |A| = 7 and |bias| <= one scale:
# 7 wmax + 1 <= bound / s.  The columns with steps of 1/8 and 1/4 stay below 4.75, where the unsafe values start.
GELU_A_L1 = 7
GELU_COL = {-3: (4.5, 4), -2: (4.5, 2), -1: (8.0, 2), 0: (8.0, 1)}
for _e, (_b, _w) in GELU_COL.items():
    assert GELU_A_L1 * _w + 1 <= _b / 2.0 ** _e


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass
class Case:
    M: int
    N: int
    K: int
    seed: int
    gelu: bool
    scale_m: bool
    a_tile: object
    A: torch.Tensor          # [M][K] int8
    W: torch.Tensor          # [N][K] int8
    scale: torch.Tensor      # fp32 [N] (or [M] under scale_m), powers of two
    bias: torch.Tensor       # fp32, an integer multiple of the channel's scale
    resid: torch.Tensor      # [M][N] integer values as bf16
    gate: torch.Tensor       # fp32 [N]
    acc: torch.Tensor        # [M][N] fp32 holding the exact integer accumulator


def accumulate(A, W):
    """the exact accumulator: every partial sum of |a||w| is below 2^24, so an fp32 matmul is exact in any order"""
    K = A.shape[1]
    assert W.shape[1] == K
    assert K * int(A.abs().max()) * int(W.abs().max()) < 2 ** 24
    return A.float() @ W.float().t()


def _signed(g, shape, hi):
    """integers in +-1 .. +-hi (hi a number or a broadcastable tensor)"""
    mag = 1 + (torch.rand(shape, generator=g) * torch.as_tensor(hi, dtype=torch.float32)).floor()
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).to(torch.int8)


def make_case(M, N, K, seed, gelu=False, scale_m=False, a_tile=None):
    """A in -3..3, W in -4..4, about half zeros; w_scale 2^-3..2^2 per channel (n, or m under scale_m); bias = integer * scale;
    residual integer bf16; gate in GATES.  gelu: the sparse alphabet of GELU_COL / GELU_A_L1 (three nonzeros per A row) that keeps the
    pre-activations on the safe lattice.  a_tile: A is nonzero in that 128-wide K-tile only (W differs from K-tile to K-tile)."""
    assert K % BK == 0 and not (gelu and scale_m)
    g = torch.Generator().manual_seed(seed)
    nchan = M if scale_m else N
    if gelu:
        e = torch.randint(-3, 1, (nchan,), generator=g)
        wmax = torch.tensor([GELU_COL[int(v)][1] for v in e], dtype=torch.float32)
        W = _signed(g, (N, K), wmax[:, None]) * (torch.rand(N, K, generator=g) < 0.5)
        pos = torch.rand(M, K, generator=g).topk(3, dim=1).indices
        A = torch.zeros(M, K, dtype=torch.int8)
        A.scatter_(1, pos, torch.cat([_signed(g, (M, 1), 3), _signed(g, (M, 2), 2)], 1))
        assert int(A.abs().sum(1).max()) <= GELU_A_L1
        bias_int = torch.randint(-1, 2, (nchan,), generator=g)
    else:
        e = torch.randint(-3, 3, (nchan,), generator=g)
        A = _signed(g, (M, K), 3) * (torch.rand(M, K, generator=g) < 0.5)
        W = _signed(g, (N, K), 4) * (torch.rand(N, K, generator=g) < 0.5)
        bias_int = torch.randint(-64, 65, (nchan,), generator=g)
    A, W = A.to(torch.int8), W.to(torch.int8)
    if a_tile is not None:
        keep = torch.zeros(K, dtype=torch.bool)
        keep[a_tile * BK:(a_tile + 1) * BK] = True
        A = A * keep
    scale = (2.0 ** e.double()).float()
    bias = (bias_int.double() * scale.double()).float()
    resid = torch.randint(-128, 129, (M, N), generator=g).to(BF)
    gate = torch.tensor(GATES)[torch.randint(0, len(GATES), (N,), generator=g)]
    gate[0], gate[-1] = (gate[0] or 1.5), (gate[-1] or -0.5)       # a zero gate hides its column: not in the first and the last one
    case = Case(M, N, K, seed, gelu, scale_m, a_tile, A, W, scale, bias, resid, gate, accumulate(A, W))
    assert int(A.abs().max()) <= 3 and int(W.abs().max()) <= 4
    for epi in ((EPI_GELU,) if gelu else (EPI_BIAS,) if scale_m else (EPI_BIAS, EPI_GATE)):
        for use_bias in (False, True):
            int_ref(case, epi, use_bias)           # asserts that every intermediate is exact in fp32 (and the GELU margin)
    return case


def _exact_f32(x64, what):
    assert torch.equal(x64.float().double(), x64), f"{what} is not exact in fp32"
    return x64.float()


def finish(acc, epi, scale2d, bias2d, resid=None, gate2d=None, strict=True):
    """the epilogue formulas on an exact accumulator; scale2d / bias2d / gate2d broadcast against [M][N].  Returns the expected bits:
    int16 for the bf16 outputs, uint8 for GELU.  strict = False (the host test's wrong-index mutants, which may leave the exact ranges):
    the same formulas with fp32 roundings and the GELU alphabet's margins not asserted."""
    if not strict:
        pre = (acc.double() * scale2d.double() + (0.0 if bias2d is None else bias2d.double())).float()
        if epi == EPI_BIAS:
            return pre.to(BF).view(torch.int16)
        if epi == EPI_GATE:
            return (resid.double() + gate2d.double() * pre.to(BF).double()).float().to(BF).view(torch.int16)
        return e4m3_rne(gelu64(pre.to(BF)))
    pre = _exact_f32(acc.double() * scale2d.double() + (0.0 if bias2d is None else bias2d.double()), "acc * s + bias")
    if epi == EPI_BIAS:
        return pre.to(BF).view(torch.int16)
    if epi == EPI_GATE:
        inner = pre.to(BF).double()
        prod = _exact_f32(gate2d.double() * inner, "gate * bf16(acc * s)")
        return _exact_f32(resid.double() + prod.double(), "resid + gate * bf16(acc * s)").to(BF).view(torch.int16)
    assert epi == EPI_GELU
    assert torch.equal(pre.to(BF).float(), pre), "GELU pre-activation is not exact in bf16"
    code, safe = gelu_lookup(pre)
    assert bool(safe.all()), "GELU pre-activation too close to an e4m3 rounding boundary"
    return code


def channel2d(case, v):
    return v[:, None] if case.scale_m else v[None, :]


def int_ref(case, epi, use_bias=False):
    """expected output bits of one launch: bf16(acc s (+ bias)); bf16(resid + gate bf16(acc s (+ bias))); e4m3(GELU(bf16(acc s (+ bias))))"""
    return finish(case.acc, epi, channel2d(case, case.scale), channel2d(case, case.bias) if use_bias else None, case.resid, case.gate[None, :])


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


# ------------------------------------------------------------------------------------------------ the table of the GPU test
# (M, N, K) per group; every group runs BIAS, GELU and GATE unless said otherwise.  tests/test_gpu_gemm_fp8_probes.py asserts per row which
# kernel the launcher picks on the machine at hand.
K8_ONE_TILE = [(256, 256, 256), (256, 256, 384), (256, 256, 640)]            # nk = 2 (the minimum), odd, 5
K8_RAGGED = [(1, 256, 256), (257, 255, 256), (300, 130, 384), (256, 1, 256), (256, 3, 256)]   # each at ldc = N + 3 and N + 4
K8_WALK = [(512, 256, 256), (1100, 520, 384), (4100, 4096, 384)]            # 2 tiles; 5 x 3 tiles (last m-group of one); 272 tiles, odd nk
W4_NATURAL = [(4100, 4096, 512), (4096, 4112, 768)]                         # ragged M at nk = 4; a last N tile of 16 columns
FORCED = [(512, 256, 512), (513, 272, 1024), (777, 528, 512)]               # both kernels by K5_GEMM_FP8_V, in child processes
SCALE_M_K8 = [(256, 200, 256), (768, 1000, 512)]                            # M = weight rows, N = tokens (not a multiple of 16)
SCALE_M_W4 = [(4096, 4096, 512)]
BIAS_N_K8, BIAS_N_W4 = (300, 130, 384), (4100, 4096, 512)                   # scale_m = 0 with bias, one ragged shape per kernel
SIGNATURE_K8 = [(256, 256, 256), (256, 256, 384), (256, 256, 1792)]         # A nonzero in the first / the last K-tile only
SIGNATURE_W4 = [(512, 256, 512), (512, 256, 1792)]                          # forced, in the child processes
SMALL_ROWS = K8_ONE_TILE + K8_RAGGED + K8_WALK[:2] + FORCED                 # what the host test examines mutation by mutation


def signature_tiles(K):
    nk = K // BK
    return sorted({0, nk // 2, nk - 1})


def probe_case(M, N, K, kind="int", a_tile=None):
    """the case of one table row: kind "int" (BIAS and GATE), "gelu", "scale_m"; seeded by the row itself"""
    assert kind in ("int", "gelu", "scale_m")
    return make_case(M, N, K, seed_of(M, N, K, kind, a_tile), gelu=kind == "gelu", scale_m=kind == "scale_m", a_tile=a_tile)


def w4_ok(M, N, K, ldc, ldr, epi):
    """the launcher's condition for the four-wave kernel (gemm_fp8.hip, launch_f8), besides tiles >= CUs or the forcing switch"""
    return K % (2 * BK) == 0 and K >= 4 * BK and M >= 512 and N >= 256 and N % 16 == 0 and ldc % 16 == 0 and (epi != EPI_GATE or ldr % 4 == 0)


def tiles(M, N):
    return ((M + BM - 1) // BM) * ((N + BN - 1) // BN)


# ------------------------------------------------------------------------------------------------ diagnosis
def explain(got, want, case=None):
    """names the first wrong (m, n), its 256 x 256 tile, and the wave, lane and accumulator indices (i = n-tile, j = m-tile) that hold it
    in either kernel (the epilogue comments of gemm_fp8.hip)"""
    got, want = got.detach().cpu(), want.detach().cpu()
    bad = got != want
    if not bad.any():
        return "no mismatch"
    m, n = [int(v) for v in bad.nonzero()[0]]
    r, c = m % BM, n % BN
    # 8-wave: row = 128 (j >> 1) + 32 wm + 16 (j & 1) + l15, wm = ((wave >> 1) & 1) | (group << 1); col = 128 (i >> 2) + 64 wn + 16 (i & 3) + 4 g + e
    wm8, wn8 = (r % 128) // 32, (c % 128) // 64
    k8 = dict(wave=4 * (wm8 >> 1) + 2 * (wm8 & 1) + wn8, lane=16 * ((c % 16) // 4) + r % 16, i=4 * (c // 128) + (c % 64) // 16,
              j=2 * (r // 128) + (r % 32) // 16, e=c % 4)
    # 4-wave: row = 128 wm + 16 j + l15, col = 128 wn + 16 i + 4 lc + e, wave = wn + 2 wm
    w4 = dict(wave=c // 128 + 2 * (r // 128), lane=16 * ((c % 16) // 4) + r % 16, i=(c % 128) // 16, j=(r % 128) // 16, e=c % 4)
    rows, cols = int(bad.any(1).sum()), int(bad.any(0).sum())
    def show(t):
        v = t[m, n]
        return f"0x{int(v) & (0xff if t.dtype == torch.uint8 else 0xffff):x} ({float(v.view(F8 if t.dtype == torch.uint8 else BF))})"
    tail = "" if case is None else f" [{case.M}x{case.N}x{case.K} seed {case.seed} gelu {case.gelu} scale_m {case.scale_m} a_tile {case.a_tile}]"
    return (f"{int(bad.sum())} mismatches in {rows} rows and {cols} columns; first at (m={m}, n={n}): got {show(got)}, want {show(want)}; "
            f"tile (m {m // BM}, n {n // BN}), row {r} column {c} in it; 8-wave kernel: {k8}; 4-wave kernel: {w4}{tail}")


# ------------------------------------------------------------------------------------------------ quantiser
def quant_static_ref(x_bf16):
    """codes of the static scale 1: the RNE, saturating e4m3 of the bf16 value"""
    return e4m3_rne(x_bf16.double())


def quant_row_ref(x_bf16, scale_dev):
    """codes under the scale the device returned: e4m3(fp32(x * fp32(1 / scale)))"""
    inv = torch.ones_like(scale_dev) / scale_dev                      # fp32, correctly rounded
    return e4m3_rne((x_bf16.float() * inv[:, None]).double())


def ulps_apart(a, b):
    """distance in fp32 ulps of two positive finite fp32 tensors"""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


def quant_rows_case(rows, K, shift, seed):
    """bf16 [rows][K]; row r is of type (r + shift) % 6: 0 maximum at k = K - 1, 1 all zero, 2 a negative maximum, 3 maximum at k = 0,
    4 maximum in the last (partial) 256-chunk, 5 plain"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, K, generator=g) * torch.logspace(-2, 2, rows)[:, None]).to(BF)
    kinds = []
    for r in range(rows):
        kind = (r + shift) % 6
        kinds.append(kind)
        top = (x[r].float().abs().max() * 3 + 1).to(BF)
        if kind == 0:
            x[r, K - 1] = top
        elif kind == 1:
            x[r] = 0
        elif kind == 2:
            x[r, K // 2] = -top
        elif kind == 3:
            x[r, 0] = top
        elif kind == 4:
            x[r, (K - 1) // 256 * 256 + min(1, K - 1 - (K - 1) // 256 * 256)] = top
    return x, kinds


def quant_static_rows():
    """the static-scale rows: zeros of both signs, the RNE ties, every subnormal, saturation"""
    v = [0.0, -0.0, 17.0, 19.0, -17.0, -19.0, 2.0 ** -10, 3 * 2.0 ** -10, -(2.0 ** -10), -3 * 2.0 ** -10]
    v += [k * 2.0 ** -9 for k in range(1, 8)] + [-k * 2.0 ** -9 for k in range(1, 8)]
    v += [448.0, -448.0, 464.0, -464.0, 480.0, -480.0, 1e4, float("inf"), float("-inf")]
    v += [1.0, 1.0625, 1.1875, 0.3, -0.7, 100.0, 239.0, 241.0, 2.0 ** -11, 5 * 2.0 ** -11]
    x = torch.tensor(v).to(BF)
    want = {17.0: 16.0, 19.0: 20.0, 2.0 ** -10: 0.0, 3 * 2.0 ** -10: 2.0 ** -8, 464.0: 448.0, 480.0: 448.0, 1e4: 448.0, float("inf"): 448.0}
    return x, want
