"""CPU reference of the integer-exact probes of the bf16 GEMM (gemm_bf16.hip: five kernels, five epilogues, one launcher).  No GPU import.

Operands are small integers (A in -3..3, W in -4..4, about half of them zero), which bf16 holds exactly; every partial sum stays below
2^24, so the fp32 accumulator is the same integer in any summation order and on any MFMA shape.  Bias is an integer, the residual integer
bf16, the gate a small dyadic number, alpha a power of two: acc + bias, gate * bf16(.), the sum with the residual and alpha * acc are exact
in fp32 (asserted), fused or not, so the expected output of every epilogue is ONE bit pattern.

kind "ties": W row n is scaled by 2^(n % 6), except its first 8 elements, which keep the sum's low bits alive: the accumulators go far
beyond 256 and many of them are exact bf16 ties (odd 9-bit integers and their multiples by powers of two) — the round-to-nearest-even of both
store paths (f2bf element by element, pack_bf16x2 in the vector stores) is pinned.

kind "gelu": the device computes gelu_erf(bf_round(v)) with the fp32 Abramowitz-Stegun 7.1.26 form; these cases keep the pre-activations on
the lattice k / 8 and only on values whose float64 GELU lies at least 16 error bounds away from every bf16 rounding boundary
(gelu_alphabet), so the bf16 bits are fixed too (+0 and -0 count as equal there).

The launcher mirror (plan, plan_f32) says which kernel, tile height and tail form the launcher takes for a call on a machine with a given
CU count; the footprint model (w4_dma_rows) says which operand rows the buffer-load-to-LDS kernels touch in a ragged tile.

tests/test_gemm_bf16_probe_host.py examines this file on the CPU; tests/test_gpu_gemm_bf16_probes.py runs the kernels against it."""
import dataclasses
import functools
import math
import zlib

import torch

BF = torch.bfloat16
BM, BN, BK = 128, 128, 64
EPI_BIAS, EPI_BIAS_M, EPI_GELU, EPI_GATE, EPI_F32 = 0, 1, 2, 3, 4          # kandinsky._engine.EPI_* (4: k5_gemm_bf16_f32out)
EPI_NAMES = {EPI_BIAS: "bias", EPI_BIAS_M: "bias_m", EPI_GELU: "gelu", EPI_GATE: "gate", EPI_F32: "f32"}
GATES = (0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 2.0, -2.0)
ALPHA = 2.0 ** -3
A_MAX, W_MAX, TIE_SHIFTS = 3, 4, 6
LDA_PAD, LDW_PAD, LDR_PAD = 8, 72, 6          # lda = K + 8, ldw = K + 72, ldr = N + 6 (N + 8 where the four-wave kernel must take the row)
OPERAND_GUARD_ROWS = 160                      # rows of NaN below every operand of the GPU test (w4_dma_rows: at most 143 are touched)


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def bf_bits(x):
    """bf16 bits (int16) of a float tensor whose values must not depend on double rounding: fp32 -> bf16, round to nearest even"""
    return x.float().to(BF).view(torch.int16)


def is_bf16_tie(x):
    """fp32-exact values that lie exactly midway between two bf16 values"""
    return (x.float().contiguous().view(torch.int32) & 0xffff) == 0x8000


def same_up_to_zero_sign(a, b):
    z = lambda t: torch.where(t == -0x8000, torch.zeros_like(t), t)
    return torch.equal(z(a), z(b))


# ------------------------------------------------------------------------------------------------ GELU alphabet
GELU_STEP, GELU_MAX = 0.125, 8.0
ERF_MARGIN = 16.0


def gelu64(x):
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))       # erfc: no cancellation on the negative side


def bf16_boundary_distance(g):
    """distance of float64 values to the nearest bf16 rounding boundary (the midpoints of neighbouring bf16 values)"""
    a = g.double().abs()
    out = torch.full_like(a, 2.0 ** -134)                          # 0: half of the smallest subnormal
    nz = a > 0
    e = torch.floor(torch.log2(a[nz]))
    ulp = 2.0 ** (e - 7)
    q = a[nz] / ulp
    d = ((q - torch.floor(q)) - 0.5).abs() * ulp
    below = (a[nz] - 2.0 ** e) + ulp / 4                           # the boundary just below a power of two is half as far
    out[nz] = torch.minimum(d, below)
    return out


@functools.lru_cache(maxsize=1)
def gelu_alphabet():
    """(x, bits, safe) over the lattice k / 8, |x| <= 8.  The device evaluates erf with |error| <= 1.5e-7 in fp32:
    |dGELU| <= 2e-7 |x| + 2^-22 |GELU(x)| (the bound of tests/gemm_fp8_probe_reference.py).  safe: the float64 GELU lies at least 16 such
    bounds away from every bf16 rounding boundary, so any evaluation within the bound rounds to the same bf16."""
    x = torch.arange(-64, 65).double() * GELU_STEP
    g = gelu64(x)
    bound = 2e-7 * x.abs() + 2.0 ** -22 * g.abs()
    return x, bf_bits(g), bf16_boundary_distance(g) >= ERF_MARGIN * bound


def gelu_safe_range():
    """[lo, hi]: the safe lattice points form one interval (asserted by the host test); derived, not written down"""
    x, _, safe = gelu_alphabet()
    return float(x[safe].min()), float(x[safe].max())


def gelu_all_safe(pre):
    """every pre-activation is a safe lattice point — by range, which is the same thing because the safe points form one interval"""
    lo, hi = gelu_safe_range()
    k = pre / GELU_STEP
    return bool((k == k.round()).all()) and float(pre.min()) >= lo and float(pre.max()) <= hi


def gelu_lookup(pre):
    k = pre.double() / GELU_STEP
    assert torch.equal(k, k.round()) and float(pre.abs().max()) <= GELU_MAX, "GELU pre-activation off the lattice"
    _, bits, safe = gelu_alphabet()
    i = k.long() + 64
    return bits[i], safe[i]


# A GELU row of A has three nonzeros 3, 2, 2 (L1 = 7), all positive.  Column n of W is of type n % 2 (in eighths): 0: 0 .. 8 (acc in
# [0, 7]), bias in eighths within [lo, 1]; 1: -3 .. 3 (|acc| <= 2.625), bias -1/8, 0, 1/8.  With the safe set [lo, 8], lo <= -2.75.
GELU_A_L1 = 7


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass
class Case:
    M: int
    N: int
    K: int
    seed: int
    kind: str
    a_tile: object
    A: torch.Tensor          # [M][K] fp32 holding the bf16-exact operand
    W: torch.Tensor          # [N][K]
    bias: torch.Tensor       # fp32 [N]
    bias_m: torch.Tensor     # fp32 [M]
    gate: torch.Tensor       # fp32 [N]
    acc: torch.Tensor        # [M][N] fp32 holding the exact accumulator

    @functools.cached_property
    def resid(self):
        g = torch.Generator().manual_seed(self.seed ^ 0x5a5a5a)
        return torch.randint(-128, 129, (self.M, self.N), generator=g, dtype=torch.int16).to(BF)


def accumulate(A, W):
    """the exact accumulator: in units of the operands' common lattice every partial sum is below 2^24, so an fp32 matmul is exact"""
    K = A.shape[1]
    unit = 0.125
    assert torch.equal((A / unit).round() * unit, A) and torch.equal((W / unit).round() * unit, W)
    assert K * float(A.abs().max() / 1.0) * float(W.abs().max() / unit) < 2 ** 24, "accumulator not exact in fp32"
    return A @ W.t()


def _signed(g, shape, hi):
    mag = 1 + (torch.rand(shape, generator=g) * hi).floor()
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return mag * sign


def make_case(M, N, K, seed, kind="int", a_tile=None):
    assert kind in ("int", "ties", "gelu") and K % 8 == 0
    g = torch.Generator().manual_seed(seed)
    if kind == "gelu":
        lo, hi = gelu_safe_range()
        assert lo <= -2.75 and hi >= 8.0
        typ = torch.arange(N) % 2
        wpos = torch.randint(0, 9, (N, K), generator=g).float()
        wmix = torch.randint(-3, 4, (N, K), generator=g).float()
        W = torch.where(typ[:, None] == 0, wpos, wmix) * GELU_STEP
        nz = min(3, K)
        pos = torch.rand(M, K, generator=g).topk(nz, dim=1).indices
        A = torch.zeros(M, K)
        A.scatter_(1, pos, torch.tensor([3.0, 2.0, 2.0])[:nz].expand(M, nz).contiguous())
        bpos = -torch.randint(-8, int(-lo / GELU_STEP) + 1, (N,), generator=g).float() * GELU_STEP      # [lo, 1]
        bmix = torch.randint(-1, 2, (N,), generator=g).float() * GELU_STEP
        bias = torch.where(typ == 0, bpos, bmix)
        bias_m = torch.zeros(M)
    else:
        A = _signed(g, (M, K), A_MAX) * (torch.rand(M, K, generator=g) < 0.5)
        W = _signed(g, (N, K), W_MAX) * (torch.rand(N, K, generator=g) < 0.5)
        if kind == "ties":
            scale = 2.0 ** (torch.arange(N) % TIE_SHIFTS).float()
            W[:, 8:] *= scale[:, None]
        bias = torch.randint(-64, 65, (N,), generator=g).float()
        bias_m = torch.randint(-64, 65, (M,), generator=g).float()
    if a_tile is not None:
        keep = torch.zeros(K, dtype=torch.bool)
        keep[a_tile * BK:(a_tile + 1) * BK] = True
        A = A * keep
    gate = torch.tensor(GATES)[torch.randint(0, len(GATES), (N,), generator=g)]
    gate[0], gate[-1] = (gate[0] or 1.5), (gate[-1] or -0.5)       # a zero gate hides its column: not in the first and the last one
    for t in (A, W, bias, bias_m):
        assert torch.equal(t.to(BF).float(), t), "operand alphabet is not exact in bf16"
    return Case(M, N, K, seed, kind, a_tile, A, W, bias, bias_m, gate, accumulate(A, W))


@functools.lru_cache(maxsize=8)
def probe_case(M, N, K, kind="int", a_tile=None):
    """the case of one table row, seeded by the row itself"""
    return make_case(M, N, K, seed_of(M, N, K, kind, a_tile), kind, a_tile)


def _exact_f32(x64, what):
    assert torch.equal(x64.float().double(), x64), f"{what} is not exact in fp32"
    return x64.float()


def finish(acc, epi, bias2d=None, resid=None, gate2d=None, strict=True, bias_late=False, gate_unrounded=False):
    """the epilogue formulas on an exact accumulator; bias2d / gate2d broadcast against [M][N].  Returns the expected bits (int16).
    strict = False (the host test's mutants, which may leave the exact ranges): fp32 roundings, nothing asserted.  bias_late: the bias is
    added AFTER the inner rounding; gate_unrounded: the gate multiplies the unrounded accumulator (two of the mutants)."""
    b = 0.0 if bias2d is None else bias2d.double()
    if not strict:
        if bias_late:
            pre = (acc.float().to(BF).double() + b).float()
        else:
            pre = (acc.double() + b).float()
        if epi in (EPI_BIAS, EPI_BIAS_M):
            return bf_bits(pre)
        if epi == EPI_GATE:
            inner = pre.double() if gate_unrounded else pre.to(BF).double()
            return bf_bits((resid.double() + gate2d.double() * inner).float())
        return bf_bits(gelu64(pre.to(BF)))
    pre = _exact_f32(acc.double() + b, "acc + bias")
    if epi in (EPI_BIAS, EPI_BIAS_M):
        return bf_bits(pre)
    if epi == EPI_GATE:
        inner = pre.to(BF).double()
        prod = _exact_f32(gate2d.double() * inner, "gate * bf16(acc + bias)")
        return bf_bits(_exact_f32(resid.double() + prod.double(), "resid + gate * bf16(acc + bias)"))
    assert epi == EPI_GELU
    assert torch.equal(pre.to(BF).float(), pre), "GELU pre-activation is not exact in bf16"
    bits, safe = gelu_lookup(pre)
    assert bool(safe.all()), "GELU pre-activation too close to a bf16 rounding boundary"
    return bits


def bias2d_of(case, epi, use_bias):
    if not use_bias:
        return None
    return case.bias_m[:, None] if epi == EPI_BIAS_M else case.bias[None, :]


def int_ref(case, epi, use_bias=False):
    """expected bf16 bits of one launch"""
    assert (epi == EPI_GELU) == (case.kind == "gelu")
    return finish(case.acc, epi, bias2d_of(case, epi, use_bias), case.resid if epi == EPI_GATE else None, case.gate[None, :])


# fp32 scores ------------------------------------------------------------------------------------
def kept_counts(M, N, hw):
    """k5_launch_gemm_bf16_f32out: n-tiles of 256 kept per m-tile of 256 (all of them without a frame-causal limit)"""
    tm, tn = (M + 255) // 256, (N + 255) // 256
    out = []
    for i in range(tm):
        last = min((i + 1) * 256, M) - 1
        out.append(min(tn, (min(N, (last // hw + 1) * hw) + 255) // 256) if hw > 0 else tn)
    return out


def f32_written(M, N, hw, tile, shift=0):
    """bool [M][N]: the elements the frame-causal tile skipping writes with tiles of `tile` rows and columns (128: the two 128 x 128 kernels,
    256: the four-wave kernel).  shift: the limit moved by that many tiles (the host test's off-by-one mutants)"""
    w = torch.zeros(M, N, dtype=torch.bool)
    for m0 in range(0, M, tile):
        last = min(m0 + tile, M) - 1
        lim = N if hw <= 0 else min(N, (last // hw + 1) * hw)
        cols = N if hw <= 0 else min(N, max(0, (lim + tile - 1) // tile + shift) * tile)
        w[m0:m0 + tile, :cols] = True
    return w


def f32_ref(case, hw, tile, shift=0):
    """expected fp32 bits (int32): alpha * acc where a tile is computed, the NaN payload of the test's poisoned output elsewhere"""
    val = _exact_f32(case.acc.double() * ALPHA, "alpha * acc")
    out = torch.where(f32_written(case.M, case.N, hw, tile, shift), val, torch.full_like(val, float("nan")))
    return out.view(torch.int32)


# ------------------------------------------------------------------------------------------------ launcher mirror
def k8_fits(M, N, K, lda, ldw):
    """the 8-wave kernel's lane offsets are 32-bit byte offsets from the operand bases"""
    return 2 * (M - 1) * lda + 2 * K < 2 ** 32 and 2 * (N - 1) * ldw + 2 * K < 2 ** 32


def w4_ld_ok(K, ld):
    """the four-wave kernel's per-tile 32-bit terms (lane offset + row offset, the signed buffer range)"""
    return 255 * 2 * ld + 2 * K < 2 ** 31


def w4_ok(M, N, K, lda, ldw, ldc, ldr, epi):
    return (K % (2 * BK) == 0 and K >= 4 * BK and M >= 512 and N >= 128 and N % 8 == 0 and ldc % 8 == 0
            and (epi != EPI_GATE or ldr % 4 == 0) and w4_ld_ok(K, lda) and w4_ld_ok(K, ldw))


def split_tail(tiles, cus, tall):
    """(full, rem, split): whole rounds of the CUs stay on the persistent kernel, a last round under half of the CUs leaves it (tallest tile only)"""
    full = tiles // cus * cus
    rem = tiles - full
    return full, rem, bool(tall and full > 0 and rem > 0 and 2 * rem < cus)


def w4_pick_mt(M, N, cus, force_mt=0):
    tn = (N + 255) // 256
    best, best_cost = 8, 1e30
    for mt, rel in ((8, 1.0), (6, 0.85), (4, 0.63)):
        tiles = ((M + 32 * mt - 1) // (32 * mt)) * tn
        full, rem = tiles // cus, tiles % cus
        c = rel * (full + (0.0 if rem == 0 else (0.85 if mt == 8 and full > 0 and 2 * rem < cus else 1.0)))
        if force_mt == mt:
            c = -1.0
        if c < best_cost - 1e-9:
            best_cost, best = c, mt
    return best


def k8_rows(M, N, cus):
    def cost(bm, w, tail_ok):
        tiles = ((M + bm - 1) // bm) * ((N + 255) // 256)
        full, rem = tiles // cus, tiles % cus
        return w * (full + (0.0 if rem == 0 else (0.3 if tail_ok and full > 0 and 2 * rem < cus else 1.0)))
    return 192 if cost(192, 0.75, False) < 0.97 * cost(256, 1.0, True) else 256


def tail_kind(K, rem):
    """launch_tail of the four-wave kernel: the 4-stage quadrant kernel, or the glds kernel"""
    return "glds" if K % (2 * BK) or K < 4 * BK or 4 * rem > 256 else "q4"


@dataclasses.dataclass(frozen=True)
class Plan:
    kernel: str              # "reg" (128 x 128, register staged), "glds", "k8", "w4"
    rows: int                # token rows of the workgroup tile
    tail: object = None      # None, "glds" or "q4"
    tiles: int = 0           # logical tiles of the launch
    rem: int = 0             # of them in the tail
    grid: int = 0            # workgroups of the main kernel

    @property
    def second_tile(self):
        return self.kernel in ("k8", "w4") and self.tiles - self.rem > self.grid


def plan(M, N, K, lda, ldw, ldc, ldr, epi, cus, kernel=0, token_tile=0):
    """what k5_launch_gemm_bf16 (k5_gemm_bf16_variant: kernel, token_tile) launches"""
    assert kernel in (0, 2, 4, 8) and token_tile in (0, 128, 192, 256) and epi in (EPI_BIAS, EPI_BIAS_M, EPI_GELU, EPI_GATE)
    ok = w4_ok(M, N, K, lda, ldw, ldc, ldr, epi)
    mt = w4_pick_mt(M, N, cus, token_tile // 32) if ok else 8
    tn = (N + 255) // 256
    tiles_pick = ((M + 32 * mt - 1) // (32 * mt)) * tn
    if ok and (kernel == 4 or (kernel == 0 and tiles_pick >= 96)):
        full, rem, split = split_tail(tiles_pick, cus, mt == 8)
        limit = full if split else tiles_pick
        return Plan("w4", 32 * mt, tail_kind(K, rem) if split else None, tiles_pick, rem if split else 0, min(limit, cus))
    tiles256 = ((M + 255) // 256) * tn
    if k8_fits(M, N, K, lda, ldw) and K % BK == 0 and K >= 2 * BK and M >= 512 and N >= 256 and (kernel == 8 or (kernel == 0 and tiles256 >= 128)):
        rows = k8_rows(M, N, cus)
        tiles = ((M + rows - 1) // rows) * tn
        full, rem, split = split_tail(tiles, cus, rows == 256)
        return Plan("k8", rows, "glds" if split else None, tiles, rem if split else 0, min(full if split else tiles, cus))
    t = ((M + BM - 1) // BM) * ((N + BN - 1) // BN)
    return Plan("glds" if K % BK == 0 else "reg", 128, None, t, 0, t)


def plan_f32(M, N, K, lda, ldw, ldc, hw, cus):
    kept = sum(kept_counts(M, N, hw))
    if (K % (2 * BK) == 0 and K >= 4 * BK and M >= 512 and N >= 256 and N % 4 == 0 and ldc % 4 == 0 and 256 <= kept < 2 ** 30
            and w4_ld_ok(K, lda) and w4_ld_ok(K, ldw)):
        return Plan("w4", 256, None, kept, 0, min(kept, cus))
    t = ((M + BM - 1) // BM) * ((N + BN - 1) // BN)
    return Plan("glds" if K % BK == 0 else "reg", 128, None, t, 0, t)


def tail_quadrants(tiles_m, tiles_n, full, rem, M, N, short_group=True):
    """(m0, n0) of every 128 x 128 quadrant the tail launch computes: workgroup b is quadrant b & 3 of the logical 256 x 256 tile full + b / 4, in
    the persistent kernels' walk (groups of 4 m-tiles).  short_group = False: the map with pgsz = 4 in a short last group (a mutant)"""
    out = []
    for b in range(4 * rem):
        plid, q = full + b // 4, b & 3
        pg = plid // (4 * tiles_n)
        pgsz = min(tiles_m - 4 * pg, 4) if short_group else 4
        m0 = (4 * pg + (plid % (4 * tiles_n)) % pgsz) * 256 + 128 * (q >> 1)
        n0 = ((plid % (4 * tiles_n)) // pgsz) * 256 + 128 * (q & 1)
        if m0 < M and n0 < N:
            out.append((m0, n0))
    return out


def walk_tile(lid, tiles_m, tiles_n, rows):
    """logical tile -> (m0, n0) of the persistent kernels' walk"""
    g = lid // (4 * tiles_n)
    gsz = min(tiles_m - 4 * g, 4)
    return (4 * g + (lid % (4 * tiles_n)) % gsz) * rows, ((lid % (4 * tiles_n)) // gsz) * 256


# ------------------------------------------------------------------------------------------------ DMA footprint model
def w4_dma_rows(form, operand, rows, ld, K):
    """The operand rows, counted from the first row of the tile, that the buffer-load-to-LDS instructions of one workgroup fetch from MEMORY for a
    tile with `rows` valid rows: form 256 / 192 / 128 (gemm_bf16_w4_kernel, MT = 8 / 6 / 4) or "q4"; operand "w" or "x".  A lane's vector offset
    (16 (lane >> 3) rows + its 16-byte chunk + the K advance) is range-checked against ((rows - 1) ld + K) 2 bytes; the instruction's row offset
    (drow + jj, drow_x + jj; 4 wave + jj in q4) travels in the scalar offset, which the range check does not see.  Returns {memory row: LDS image
    row}; the image row equals the memory row in every form (asserted), so a row past the valid ones lands in an accumulator row that is never stored."""
    assert form in (256, 192, 128, "q4") and operand in ("w", "x") and rows >= 1
    limit = ((rows - 1) * ld + K) * 2
    out = {}
    for wave in range(4):
        if form == "q4" or (form == 128 and operand == "x"):
            srows = [4 * wave + jj for jj in range(4)]
            pieces = srows
        else:
            drow, dslot = 128 * (wave >> 1) + 8 * (wave & 1), 8 * wave
            srows = [drow + jj for jj in range(8)]
            pieces = [dslot + jj for jj in range(8)]
        for s, piece in zip(srows, pieces):
            for i in range(8):                                   # lane >> 3; a row is touched as soon as its first chunk of the first K-tile is in range
                if 16 * i * ld * 2 + 16 <= limit:
                    image = 128 * (piece >> 4) + 16 * i + (piece & 15)      # piece 16 h + r, slot i: row 128 h + 16 i + r
                    assert image == 16 * i + s
                    out[16 * i + s] = image
    return out


@functools.lru_cache(maxsize=None)
def w4_rows_past(form, operand, rows, ld, K):
    """rows past the last valid one that are read from memory"""
    return max(0, max(w4_dma_rows(form, operand, rows, ld, K)) - (rows - 1))


def footprint_of_call(p, M, N, K, lda, ldw):
    """largest number of rows past the end of either operand that a planned launch reads (0 for the kernels that clamp their rows)"""
    return max(footprint_per_operand(p, M, N, K, lda, ldw))


def footprint_per_operand(p, M, N, K, lda, ldw):
    """(rows read past the end of A, rows read past the end of W) of a planned launch"""
    worst_x = worst_w = 0
    forms = []
    if p.kernel == "w4":
        forms.append(p.rows)
    if p.tail == "q4":
        forms.append("q4")
    for form in forms:
        tile_m = 128 if form == "q4" else p.rows
        tile_n = 128 if form == "q4" else 256
        span_x = 128 if form in ("q4", 128) else 256       # rows_x: the 192-row form still ranges over 256 rows
        for m0 in sorted({0, max(0, (M - 1) // tile_m - 1) * tile_m, (M - 1) // tile_m * tile_m}):      # the full, the last but one and the last tile
            worst_x = max(worst_x, w4_rows_past(form, "x", min(M - m0, span_x), lda, K) - max(0, M - m0 - span_x))
        last_n0 = (N - 1) // tile_n * tile_n
        worst_w = max(worst_w, w4_rows_past(form, "w", min(N - last_n0, tile_n), ldw, K))
    return worst_x, worst_w


# ------------------------------------------------------------------------------------------------ mutants
def embed_rows(t, ld, fill=float("nan")):
    out = torch.full((t.shape[0], ld), fill, dtype=torch.float32)
    out[:, :t.shape[1]] = t.float()
    return out


def mutants(c, epi, use_bias, ldc=None, ldr=None):
    """(name, output bits) of the wrong kernels a case can tell from the right one; a mutant that cannot apply to the case is not yielded"""
    M, N, K = c.M, c.N, c.K
    nk = (K + BK - 1) // BK
    b2 = bias2d_of(c, epi, use_bias)
    resid = c.resid if epi == EPI_GATE else None
    g2 = c.gate[None, :]
    out = lambda acc=c.acc, b=b2, r=resid, **kw: finish(acc, epi, b, r, g2, strict=False, **kw)
    A, W = c.A, c.W
    for size in (16, 32):
        perm = torch.arange(M) ^ (size // 2)
        perm = torch.where(perm < M, perm, torch.arange(M))
        if not torch.equal(perm, torch.arange(M)):
            yield f"rows swapped within a {size}-row MFMA tile", out(acc=c.acc[perm])
    s = min(M, N, 128)
    if s >= 2:
        t = c.acc.clone()
        t[:s, :s] = c.acc[:s, :s].t()
        yield "transposed 128 x 128 quadrant", out(acc=t)
    cols = torch.arange(N) ^ 32
    cols = torch.where(cols < N, cols, torch.arange(N))
    if N > 32:
        yield "the two N halves of a wave exchanged", out(acc=c.acc[:, cols])
    part = lambda t, u=None: A[:, t * BK:(t + 1) * BK] @ W[:, (t if u is None else u) * BK:((t if u is None else u) + 1) * BK].t()
    for t in range(nk):
        if bool((A[:, t * BK:(t + 1) * BK] != 0).any()):
            yield f"K-tile {t} dropped", out(acc=c.acc - part(t))
            yield f"K-tile {t} doubled", out(acc=c.acc + part(t))
    if nk >= 2 and K % BK == 0:
        yield "last K-tile clamped onto the one before it", out(acc=c.acc - part(nk - 1) + part(nk - 2))
    if use_bias and epi != EPI_BIAS_M and M >= 2 and N >= 2:
        yield "bias indexed by m instead of n", out(b=c.bias[torch.arange(M) % N][:, None])
    if use_bias and epi == EPI_BIAS_M and M >= 2 and N >= 2:
        yield "bias indexed by n instead of m", out(b=c.bias_m[torch.arange(N) % M][None, :])
    if use_bias and c.kind == "ties" and M * N >= 64:          # (a handful of elements may hold no inexact accumulator)
        yield "bias added after the inner rounding", out(bias_late=True)
    if epi == EPI_GATE and c.kind == "ties" and M * N >= 64:
        yield "gate applied to the unrounded accumulator", out(gate_unrounded=True)
    if epi == EPI_GATE and ldr is not None and ldc is not None and ldr != ldc and M >= 2:
        flat = embed_rows(c.resid, ldr).flatten()
        idx = torch.arange(M)[:, None] * ldc + torch.arange(N)[None, :]
        yield "residual read with ldc instead of ldr", out(r=flat[idx.clamp(max=len(flat) - 1)])
    if M >= 2:
        flat = embed_rows(A, K + LDA_PAD).flatten()
        yield "A read with ld = K instead of lda", out(acc=flat[:M * K].view(M, K) @ W.t())
    if N >= 2:
        flat = embed_rows(W, K + LDW_PAD).flatten()
        yield "W read with ld = K instead of ldw", out(acc=A @ flat[:N * K].view(N, K).t())


# ------------------------------------------------------------------------------------------------ diagnosis
def owner(p, m, n):
    """the tile, quadrant, wave, lane and accumulator indices that hold output (m, n) on the planned kernel"""
    if p.kernel in ("reg", "glds"):
        r, c = m % 128, n % 128
        return dict(kernel=p.kernel, tile=(m // 128, n // 128), wave=2 * (r // 64) + c // 64, lane=32 * ((c % 8) // 4) + r % 32, i=(c % 64) // 32,
                    j=(r % 64) // 32, rg=(c % 32) // 8, e=c % 4, lane_row=m)
    r, c = m % p.rows, n % 256
    per_wave = p.rows // (4 if p.kernel == "k8" else 2)          # token rows per wave along m
    wm, wn = r // per_wave, c // 128
    wave = (wn | ((wm & 1) << 1) | ((wm >> 1) << 2)) if p.kernel == "k8" else wn + 2 * wm
    d = dict(kernel=p.kernel, tile=(m // p.rows, n // 256), quadrant=2 * ((m % 256) // 128) + c // 128, wave=wave, lane=16 * ((c % 16) // 4) + r % 16,
             i=(c % 128) // 16, j=(r % per_wave) // 16, e=c % 4, lane_row=m)
    if p.tail:
        d["tail"] = p.tail
    return d


def explain(got, want, case=None, p=None, epi=None, use_bias=False, ldc=None, ldr=None):
    """names the first wrong (m, n), its tile, quadrant and lane-owned row, and — for a small case — the single mutants of the host test that
    reproduce the wrong output"""
    got, want = got.detach().cpu(), want.detach().cpu()
    bad = got != want
    if not bad.any():
        return "no mismatch"
    m, n = [int(v) for v in bad.nonzero()[0]]
    rows, cols = int(bad.any(1).sum()), int(bad.any(0).sum())
    text = f"{int(bad.sum())} mismatches in {rows} rows and {cols} columns; first at (m={m}, n={n}): got 0x{int(got[m, n]) & 0xffffffff:x}, want 0x{int(want[m, n]) & 0xffffffff:x}"
    if p is not None:
        text += f"; held by {owner(p, m, n)}"
    if case is not None:
        text += f" [{case.M}x{case.N}x{case.K} seed {case.seed} kind {case.kind} a_tile {case.a_tile}]"
        if epi is not None and epi != EPI_F32 and case.M * case.N * case.K <= 2 ** 27:
            hits = [name for name, bits in mutants(case, epi, use_bias, ldc, ldr) if torch.equal(bits, got)]
            text += f"; reproduced by the mutant(s): {hits}" if hits else "; no single mutant of the host test reproduces it"
    return text


# ------------------------------------------------------------------------------------------------ the table of the GPU test
# A row: (M, N, K, pad = ldc - N, kernel id, token tile) and what the launcher must make of it at the machine's CU count.
@dataclasses.dataclass(frozen=True)
class Row:
    M: int
    N: int
    K: int
    pad: int                      # ldc = N + pad
    kernel: int = 0               # k5_gemm_bf16_variant's kernel id
    tile: int = 0                 # ... and token tile
    expect: tuple = ("glds", 128, None)      # (kernel, rows, tail) at 256 CUs
    big: bool = False             # fewer epilogue forms (the reference of a large case costs seconds)
    ldr_pad: int = LDR_PAD
    sig: bool = False             # K-tile signature row: BIAS only, A nonzero in one K-tile
    pin: str = ""                 # the kind of the row's integer case where the table must not leave it to the hash: "int" or "ties"

    @property
    def id(self):
        return f"{self.M}x{self.N}x{self.K}-ldc+{self.pad}-k{self.kernel}-t{self.tile}{'-sig' if self.sig else ''}"

    @property
    def kind(self):
        if self.pin:
            return self.pin
        if self.K < 40:
            return "int"                      # eight products cannot leave bf16's eight bits: no ties to be had
        return ("int", "ties")[seed_of(self.M, self.N, self.K) & 1]


# (name, epilogue, bias, in place) — every form of every epilogue; the big rows run the starred ones
FORMS = [("bias", EPI_BIAS, True, False), ("bias null", EPI_BIAS, False, False), ("bias_m", EPI_BIAS_M, True, False), ("bias_m null", EPI_BIAS_M, False, False),
         ("gelu", EPI_GELU, True, False), ("gelu null", EPI_GELU, False, False), ("gate", EPI_GATE, True, False), ("gate in place", EPI_GATE, True, True),
         ("gate null", EPI_GATE, False, False), ("gate null in place", EPI_GATE, False, True)]
BIG_FORMS = [f for f in FORMS if f[0] in ("bias", "bias_m", "gelu null", "gate", "gate null in place")]


def forms_of(row):
    if row.sig:
        return [FORMS[0]]
    return BIG_FORMS if row.big else FORMS


REG_SHAPES = [(1, 1), (7, 130), (129, 129), (200, 72), (5, 3)]
REG_KS = [8, 40, 72, 136, 200]
PADS = [1, 3, 4]
REG_ROWS = [Row(M, N, K, PADS[(i + j) % 3], (0, 2)[(i + j) & 1], 0, ("reg", 128, None)) for i, (M, N) in enumerate(REG_SHAPES) for j, K in enumerate(REG_KS)]
GLDS_SHAPES = [(128, 128), (200, 300), (1100, 260), (1, 1), (130, 3)]            # one tile; ragged 2 x 3; 9 x 3 = 27 tiles: the XCD ranges wrap
GLDS_KS = [64, 128, 192, 320]
GLDS_ROWS = [Row(M, N, K, PADS[(i + j) % 3], (0, 2)[(i + j) & 1], 0, ("glds", 128, None)) for i, (M, N) in enumerate(GLDS_SHAPES) for j, K in enumerate(GLDS_KS)]
K8_ROWS = [  # 192-row form: under one round of the CUs
    Row(513, 256, 128, 4, 8, 0, ("k8", 192, None)), Row(513, 257, 192, 3, 8, 0, ("k8", 192, None)), Row(700, 511, 320, 1, 8, 0, ("k8", 192, None)),
    Row(700, 256, 192, 8, 8, 0, ("k8", 192, None)), Row(512, 511, 128, 4, 8, 0, ("k8", 192, None)),
    # 256-row form: exactly one round (16 x 16); 33 x 8 tiles: one round, 8 tiles to the glds tail, odd nk
    Row(4096 - 40, 4096 - 24, 192, 4, 0, 0, ("k8", 256, None), big=True, pin="ties"), Row(4096 - 40, 4096 - 24, 192, 3, 8, 0, ("k8", 256, None), big=True, pin="ties"),
    Row(33 * 256 - 100, 2048 - 9, 192, 4, 0, 0, ("k8", 256, "glds"), big=True, pin="ties"), Row(33 * 256 - 100, 2048 - 9, 192, 3, 8, 0, ("k8", 256, "glds"), big=True, pin="ties")]
W4_SMALL = [Row(M, N, K, 8, 4, tile, ("w4", tile, None), ldr_pad=12) for tile in (256, 192, 128)
            for M, N, K in ((512, 128, 256), (513, 136, 384), (700, 264, 512), (513, 264, 640))]
W4_MANY = [Row(4100, 2056, 256, 8, 4, 128, ("w4", 128, None), big=True, ldr_pad=12, pin="ties"),           # 33 x 9 = 297 tiles of 128 rows
           Row(6000, 2056, 256, 8, 4, 192, ("w4", 192, None), big=True, ldr_pad=12, pin="ties"),           # 32 x 9 = 288 of 192
           Row(6100, 4072, 256, 8, 4, 256, ("w4", 256, None), big=True, ldr_pad=12, pin="int")]           # 24 x 16 = 384 of 256, no tail: 128 workgroups run two
W4_Q4 = [Row(tm * 256 - 77, 2040, K, 8, 4, 256, ("w4", 256, "q4"), big=True, ldr_pad=12, pin=pin) for tm, K, pin in ((33, 256, "ties"), (34, 256, "int"), (35, 256, "ties"), (35, 384, "ties"))]
W4_GLDS_TAIL = [Row(41 * 256 - 200, 2040, 256, 8, 4, 256, ("w4", 256, "glds"), big=True, ldr_pad=12, pin="ties")]   # 328 tiles: 72 in the tail, 4 * 72 > 256
W4_NATURAL = [Row(3000, 2056, 256, 8, 0, 0, ("w4", 128, None), big=True, ldr_pad=12)]           # by cost: 24 x 9 = 216 tiles of 128 rows
W4_SIG = [Row(512, 128, 256, 8, 4, 256, ("w4", 256, None), sig=True), Row(512, 128, 384, 8, 4, 128, ("w4", 128, None), sig=True),
          Row(33 * 256 - 77, 2040, 256, 8, 4, 256, ("w4", 256, "q4"), sig=True), Row(33 * 256 - 77, 2040, 384, 8, 4, 256, ("w4", 256, "q4"), sig=True)]
# rows the four-wave kernel must hand on: a four-wave shape with ldc = N + 4 (and ldr = N + 6)
HAND_ON = [Row(6100, 4072, 256, 4, 0, 0, ("k8", 192, None), big=True), Row(4100, 2056, 256, 4, 4, 128, ("glds", 128, None), big=True),
           Row(33 * 256 - 77, 2040, 256, 4, 0, 0, ("k8", 256, "glds"), big=True)]
SMALL_ROWS = REG_ROWS + GLDS_ROWS + K8_ROWS[:5] + W4_SMALL
ALL_ROWS = REG_ROWS + GLDS_ROWS + K8_ROWS + W4_SMALL + W4_MANY + W4_Q4 + W4_GLDS_TAIL + W4_NATURAL + W4_SIG + HAND_ON

# fp32 scores: (M, N, K, pad, hw, expected kernel); hw 0 = no frame-causal limit, 64 divides the tile, 48 and 100 do not
F32_ROWS = [(130, 130, 40, 1, 0, "reg"), (300, 290, 72, 4, 48, "reg"), (300, 300, 136, 1, 64, "reg"), (256, 256, 64, 4, 64, "glds"), (300, 300, 128, 1, 100, "glds"),
            (257, 130, 192, 4, 0, "glds"), (520, 520, 128, 4, 48, "glds"), (5000, 5000, 256, 4, 1000, "w4"), (5000, 5000, 256, 1, 1000, "glds")]


def signature_tiles(K):
    nk = K // BK
    return sorted({0, nk // 2, nk - 1})


def row_plan(row, epi, inplace, cus):
    """the launcher's choice for one form of a row"""
    ldc = row.N + row.pad
    return plan(row.M, row.N, row.K, row.K + LDA_PAD, row.K + LDW_PAD, ldc, ldc if inplace else row.N + row.ldr_pad, epi, cus, row.kernel, row.tile)
