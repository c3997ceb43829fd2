"""CPU checks of tests/gemm_bf16_probe_reference.py, the reference of tests/test_gpu_gemm_bf16_probes.py: the expected bits equal an
independent float64 evaluation and every step is exact in fp32; mutation by mutation, the small cases of the GPU table give a DIFFERENT
output under each wrong indexing a kernel could have; the launcher mirror reproduces a written table of choices; the GELU alphabet is safe;
the DMA footprint of the buffer-load kernels stays inside the guard rows the GPU test allocates."""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_bf16_probe_reference as R  # noqa: E402
from gemm_bf16_probe_reference import BF, BK, EPI_BIAS, EPI_BIAS_M, EPI_F32, EPI_GATE, EPI_GELU  # noqa: E402

CUS = 256          # an MI355X; the GPU test asserts the same against the machine's own count
SMALL = R.SMALL_ROWS


def case_of(row, epi, a_tile=None):
    kind = "gelu" if epi == EPI_GELU else ("int" if row.sig else row.kind)
    return R.probe_case(row.M, row.N, row.K, kind, a_tile)


def differs(a, b, gelu=False):
    return not (R.same_up_to_zero_sign(a, b) if gelu else torch.equal(a, b))


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("row", SMALL, ids=lambda r: r.id)
def test_int_ref_is_the_float64_product_and_every_step_is_exact(row):
    for name, epi, use_bias, _ in R.FORMS:
        c = case_of(row, epi)
        for t in (c.A, c.W, c.bias, c.bias_m, c.gate):
            assert torch.equal(t.to(BF).float(), t)                               # what the device holds is what the case says
        assert torch.equal(c.resid.float(), c.resid.float().round()) and set(c.gate.tolist()) <= set(R.GATES)
        if c.kind != "gelu":
            assert float(c.A.abs().max()) <= R.A_MAX and float(c.W.abs().max()) <= R.W_MAX * 2 ** (R.TIE_SHIFTS - 1)
            assert c.K * float(c.A.abs().max()) * float(c.W.abs().max()) < 2 ** 24
            if c.M * c.K >= 512:
                assert 0.35 < float((c.A == 0).float().mean()) < 0.65
        acc = c.A.double() @ c.W.double().t()
        assert torch.equal(acc, c.acc.double()) and float(acc.abs().max()) < 2 ** 24
        b = (c.bias_m.double()[:, None] if epi == EPI_BIAS_M else c.bias.double()[None, :]) if use_bias else 0.0
        pre = acc + b
        assert torch.equal(pre.float().double(), pre)                             # acc + bias: exact in fp32, fused or not
        want = R.int_ref(c, epi, use_bias)                                        # (asserts its own exactness conditions)
        bf = lambda t: t.float().to(BF)
        if epi in (EPI_BIAS, EPI_BIAS_M):
            assert torch.equal(bf(pre).view(torch.int16), want)
        elif epi == EPI_GATE:
            prod = c.gate.double()[None, :] * bf(pre).double()
            total = c.resid.double() + prod
            assert torch.equal(prod.float().double(), prod) and torch.equal(total.float().double(), total)
            assert torch.equal(bf(total).view(torch.int16), want)
        else:
            assert torch.equal(bf(pre).double(), pre)
            got = bf(torch.nn.functional.gelu(pre)).view(torch.int16)
            assert not differs(got, want, gelu=True)
    c = case_of(row, EPI_BIAS)
    s = c.acc.double() * R.ALPHA
    assert torch.equal(s.float().double(), s)                                     # the fp32 scores


def vector_stored(row, N):
    """bool [N]: columns the 128 x 128, 8-wave and q4 epilogues store with a packed 8-byte store (the four-wave kernel: all of them)"""
    v = torch.zeros(N, dtype=torch.bool)
    if (row.N + row.pad) % 4 == 0:
        v[:N // 4 * 4] = True
    return v


def test_tie_cases_hold_ties_under_both_store_paths():
    """the 'ties' cases — every one of the table, the large rows of the tail forms included — round exact bf16 ties (odd 9-bit integers and their
    like) through the packed stores and through the scalar ones"""
    seen = collections.Counter()
    for row in {(r.M, r.N, r.K, r.pad): r for r in R.ALL_ROWS if not r.sig and r.kind == "ties"}.values():
        c = case_of(row, EPI_BIAS)
        for pre in (c.acc + c.bias[None, :], c.acc, c.acc + c.bias_m[:, None]):
            tie = R.is_bf16_tie(pre)
            assert bool(tie.any()) or c.M * c.N < 64, row.id
            vec = vector_stored(row, c.N)
            if c.M >= 100 and c.K >= 40 and int(vec.sum()) >= 64:
                assert bool(tie[:, vec].any()), row.id
            if c.M >= 100 and c.K >= 40 and int((~vec).sum()) >= 1:
                assert bool(tie[:, ~vec].any()), row.id
            seen["vector"] += int(tie[:, vec].sum())
            seen["scalar"] += int(tie[:, ~vec].sum())
            up = R.bf_bits(pre)[tie].view(BF).float().abs() > pre[tie].abs()
            assert bool((R.bf_bits(pre)[tie] & 1 == 0).all())                    # ties go to the even mantissa ...
            seen["up"] += int(up.sum())
            seen["down"] += int((~up).sum())
    assert min(seen.values()) >= 200, seen                                        # ... in both directions, under both store paths
    plans = [R.row_plan(r, EPI_BIAS, False, CUS) for r in R.ALL_ROWS if r.kind == "ties" and not r.sig]
    assert {(p.kernel, p.rows, p.tail) for p in plans} >= {("reg", 128, None), ("glds", 128, None), ("k8", 192, None), ("k8", 256, None), ("k8", 256, "glds"),
                                                           ("w4", 256, None), ("w4", 192, None), ("w4", 128, None), ("w4", 256, "q4"), ("w4", 256, "glds")}
    # the kinds of the large rows are written into the table, not left to the hash
    assert all(r.pin for r in R.K8_ROWS[5:] + R.W4_MANY + R.W4_Q4 + R.W4_GLDS_TAIL) and {r.pin for r in R.W4_Q4} == {"int", "ties"}


# ------------------------------------------------------------------------------------------------ mutants
MUTANT_KINDS = ["rows swapped within a 16-row", "rows swapped within a 32-row", "transposed 128 x 128 quadrant", "N halves of a wave exchanged", "dropped", "doubled",
                "last K-tile clamped", "bias indexed by m instead of n", "bias indexed by n instead of m", "bias added after the inner rounding", "gate applied to the unrounded accumulator",
                "residual read with ldc instead of ldr", "A read with ld = K", "W read with ld = K"]


@pytest.mark.parametrize("row", list({(r.M, r.N, r.K, r.pad, r.ldr_pad): r for r in SMALL}.values()), ids=lambda r: r.id)
def test_every_mutant_changes_the_expected_output(row):
    for name, epi, use_bias, inplace in R.FORMS:
        c = case_of(row, epi)
        want = R.int_ref(c, epi, use_bias)
        ldc = row.N + row.pad
        ldr = ldc if inplace else row.N + row.ldr_pad
        right = R.finish(c.acc, epi, R.bias2d_of(c, epi, use_bias), c.resid if epi == EPI_GATE else None, c.gate[None, :], strict=False)
        assert not differs(right, want, epi == EPI_GELU)                          # the unasserted formulas agree with the strict ones
        n = 0
        for mname, got in R.mutants(c, epi, use_bias, ldc, ldr):
            if c.M * c.N >= 4 or "K-tile" not in mname or bool(c.acc.any()):
                assert differs(got, want, epi == EPI_GELU), f"{row.id} {name}: '{mname}' gives the expected output"
            assert any(k in mname for k in MUTANT_KINDS), mname
            n += 1
        assert n >= 2 + (c.M >= 2) + (c.N >= 2)


def test_every_kind_of_mutant_is_applied():
    """the mutants are not vacuous: on a 'ties' row and an 'int' row of either 128 x 128 kernel every kind of them is generated"""
    seen = collections.Counter()
    picked = []
    for group in (R.REG_ROWS, R.GLDS_ROWS):          # K % 64 != 0 and whole K-tiles
        rows = [r for r in group if r.M >= 100 and r.N >= 100]
        picked += [r for r in rows if r.kind == "ties"][:1] + [r for r in rows if r.kind == "int"][:1]
    assert len(picked) == 4
    for row in picked:
        for name, epi, use_bias, inplace in R.FORMS:
            ldc = row.N + row.pad
            for mname, _ in R.mutants(case_of(row, epi), epi, use_bias, ldc, ldc if inplace else row.N + row.ldr_pad):
                seen[[k for k in MUTANT_KINDS if k in mname][0]] += 1
    for k in MUTANT_KINDS:
        assert seen[k] >= 2, (k, seen)


@pytest.mark.parametrize("row", R.W4_Q4 + R.W4_GLDS_TAIL + R.K8_ROWS[7:8], ids=lambda r: r.id)
def test_tail_map_covers_the_tail_and_a_full_last_group_does_not(row):
    """the quadrant-to-tile map of the tail launch: with pgsz = min(tiles_m - first, 4) it covers exactly the 128 x 128 quadrants of the logical tiles the
    persistent kernel leaves; with pgsz = 4 in a short last m-group (tiles_m = 33, 34, 35, 41) some quadrants are computed twice and others never"""
    p = R.row_plan(row, EPI_BIAS, False, CUS)
    tm, tn = (row.M + 255) // 256, (row.N + 255) // 256
    assert p.tail and p.rem > 0 and tm % 4 != 0 and p.tiles == tm * tn
    full = p.tiles - p.rem
    need = set()
    for lid in range(full, p.tiles):
        m0, n0 = R.walk_tile(lid, tm, tn, 256)
        need |= {(m0 + dm, n0 + dn) for dm in (0, 128) for dn in (0, 128) if m0 + dm < row.M and n0 + dn < row.N}
    main = {R.walk_tile(lid, tm, tn, 256) for lid in range(full)}
    assert len(main) == full and len(main | {(m // 256 * 256, n // 256 * 256) for m, n in need}) == p.tiles        # the two launches share no tile and miss none
    right = R.tail_quadrants(tm, tn, full, p.rem, row.M, row.N)
    assert len(right) == len(set(right)) and set(right) == need
    wrong = R.tail_quadrants(tm, tn, full, p.rem, row.M, row.N, short_group=False)
    assert set(wrong) != need and (need - set(wrong)), "the mutant leaves no quadrant unwritten"
    assert (tm % 4) in (1, 2, 3)
    assert {(33 + i) % 4 for i in range(3)} == {1, 2, 3} and {(r.M + 255) // 256 for r in R.W4_Q4} == {33, 34, 35}


def test_frame_causal_limit_off_by_one_tile_changes_the_bits():
    n = 0
    for M, N, K, pad, hw, kernel in R.F32_ROWS:
        if hw == 0 or M > 1000:
            continue
        c = R.probe_case(M, N, K, "int")
        want = R.f32_ref(c, hw, 128)
        for shift in (-1, 1):
            assert not torch.equal(R.f32_ref(c, hw, 128, shift), want), (M, N, hw, shift)
        w = R.f32_written(M, N, hw, 128)
        i, j = torch.arange(M)[:, None], torch.arange(N)[None, :]
        assert bool(w[j < (i // hw + 1) * hw].all()) and not bool(w.all())         # everything the softmax reads is written; something is skipped
        n += 1
    assert n >= 5
    # the four-wave row: kept 256 x 256 tiles as the launcher counts them, a frame edge inside a tile
    M, N, K, pad, hw, kernel = [r for r in R.F32_ROWS if r[5] == "w4"][0]
    kept = R.kept_counts(M, N, hw)
    w = R.f32_written(M, N, hw, 256)
    assert sum(kept) >= 256 and hw % 256 != 0 and [int(w[i * 256].sum() + 255) // 256 for i in range(len(kept))] == kept
    assert not torch.equal(R.f32_written(M, N, hw, 256, 1), w) and not torch.equal(R.f32_written(M, N, hw, 256, -1), w)


@pytest.mark.parametrize("row", R.W4_SIG, ids=lambda r: r.id)
def test_k_tile_signature_cases_name_their_k_tile(row):
    nk = row.K // BK
    tiles = R.signature_tiles(row.K)
    assert 0 in tiles and nk - 1 in tiles and nk in (4, 6)
    if row.M > 1000:
        row = R.Row(700, 264, row.K, 8, 4, 256)             # the same K-tiles on a shape the CPU turns over quickly
    for t in tiles:
        c = R.probe_case(row.M, row.N, row.K, "int", t)
        assert not bool(c.A[:, :t * BK].any()) and not bool(c.A[:, (t + 1) * BK:].any()) and bool(c.A.any())
        want = R.int_ref(c, EPI_BIAS, True)
        b2 = c.bias[None, :]
        At = c.A[:, t * BK:(t + 1) * BK]
        assert differs(R.finish(torch.zeros_like(c.acc), EPI_BIAS, b2, strict=False), want)
        assert differs(R.finish(2 * c.acc, EPI_BIAS, b2, strict=False), want)
        for u in range(nk):
            got = R.finish(At @ c.W[:, u * BK:(u + 1) * BK].t(), EPI_BIAS, b2, strict=False)
            assert differs(got, want) == (u != t), (t, u)
            if u != t:
                assert float((got != want).float().mean()) > 0.5


# ------------------------------------------------------------------------------------------------ GELU alphabet
def test_gelu_alphabet_margin_and_the_values_actually_used():
    x, bits, safe = R.gelu_alphabet()
    g = R.gelu64(x)
    bound = 2e-7 * x.abs() + 2.0 ** -22 * g.abs()
    # the rounding boundaries written out again: midpoints of neighbouring bf16 values around g
    lo = (g.float().view(torch.int32) & ~0xffff).view(torch.float32)
    cand = []
    for step in (-2, -1, 0, 1, 2):
        a = (lo.view(torch.int32) + step * 0x10000).view(torch.float32).double()
        b = (lo.view(torch.int32) + (step + 1) * 0x10000).view(torch.float32).double()
        cand.append((a + b) / 2)
    dist = torch.stack([(g - m).abs() for m in cand]).min(0).values
    nz = g != 0
    assert torch.allclose(dist[nz], R.bf16_boundary_distance(g)[nz], rtol=1e-12, atol=0)
    assert torch.equal(safe[nz], (dist >= 16 * bound)[nz]) and bool(safe[~nz].all())
    # the safe set is one interval: [-2.75, 8], 87 of the 129 lattice points
    lo_x, hi_x = R.gelu_safe_range()
    assert (lo_x, hi_x) == (-2.75, 8.0) and int(safe.sum()) == 87 and torch.equal(safe, (x >= lo_x) & (x <= hi_x))
    # an evaluation that is off by the whole bound, either way, still rounds to the same bf16 on every safe value
    for sgn in (-1, 1):
        assert torch.equal(R.bf_bits(g + sgn * bound)[safe], bits[safe])
    used, total, compared = set(), 0, 0
    for row in {(r.M, r.N, r.K): r for r in R.ALL_ROWS if not r.sig}.values():
        c = case_of(row, EPI_GELU)
        if row.big:          # by range: the safe set is the interval asserted above (the exact lookup of 17 M elements twice costs seconds per row)
            assert R.gelu_all_safe(c.acc) and R.gelu_all_safe(c.acc + c.bias[None, :]), row.id
            continue
        for use_bias in (False, True):
            pre = c.acc.double() + (c.bias.double()[None, :] if use_bias else 0.0)
            assert R.gelu_all_safe(pre.float())
            _, ok = R.gelu_lookup(pre)
            assert bool(ok.all()), row.id                                             # every pre-activation of every GELU case is safe ...
            total += pre.numel()
            compared += R.int_ref(c, EPI_GELU, use_bias).numel()                      # ... so no element is left out of the comparison
            used |= set(pre.unique().tolist())
    assert compared == total
    assert len(used) >= 40 and sum(v < 0 for v in used) >= 10 and sum(v > 0 for v in used) >= 10 and min(used) <= -2.5 and max(used) >= 6


# ------------------------------------------------------------------------------------------------ launcher mirror
def test_launcher_mirror_against_a_written_table():
    P = lambda *a, **k: (lambda p: (p.kernel, p.rows, p.tail, p.tiles, p.rem))(R.plan(*a, **k))
    ld = lambda M, N, K, ldc=None, ldr=None: (M, N, K, K, K, ldc or N, ldr or N, EPI_BIAS)
    # the model's own launches on 256 CUs (launcher comments): 1302 tiles of an N = 1792 projection = 5 rounds + 22 tiles to the quadrant kernel
    assert P(*ld(47616, 1792, 1792), 256) == ("w4", 256, "q4", 1302, 22)
    assert P(*ld(47616, 7168, 1792), 256)[:3] == ("w4", 256, "glds")                 # FF1: 5208 tiles, 88 in the tail, 4 * 88 > 256
    assert P(*ld(5952, 1792, 1792), 256)[:2] == ("w4", 192) and P(*ld(3328, 1792, 1792), 256)[:2] == ("w4", 128)
    assert P(*ld(3328, 1792, 1792), 304)[:2] == ("w4", 128) and P(*ld(5952, 1792, 1792), 304)[:2] == ("w4", 192)       # still one round each on 304 CUs
    assert P(*ld(47616, 1792, 1792), 304) == ("w4", 256, "glds", 1302, 86)            # 4 rounds of 304 + 86 tiles, 4 * 86 > 256: the tail goes to glds
    assert P(512, 128, 256, 256, 256, 128, 128, EPI_BIAS, 256) == ("glds", 128, None, 4, 0)
    assert P(512, 128, 256, 256, 256, 128, 128, EPI_BIAS, 256, kernel=4)[:2] == ("w4", 128)
    assert P(512, 128, 256, 256, 256, 128, 128, EPI_BIAS, 256, kernel=4, token_tile=192)[:2] == ("w4", 192)
    assert P(512, 256, 128, 128, 128, 256, 256, EPI_BIAS, 256, kernel=8)[:2] == ("k8", 192)
    assert P(512, 256, 136, 136, 136, 256, 256, EPI_BIAS, 256, kernel=8)[:2] == ("reg", 128)
    assert P(4096, 4096, 192, 192, 192, 4096, 4096, EPI_BIAS, 256)[:3] == ("k8", 256, None)
    assert P(4096, 4096, 192, 192, 192, 4096, 4096, EPI_BIAS, 304)[:3] == ("k8", 256, None)      # 256 tiles: one partial round of 304 at cost 1 against two of 192 rows at 3/4
    # each w4_ok term on its own
    ok = dict(M=4096, N=4096, K=256, lda=256, ldw=256, ldc=4096, ldr=4096, epi=EPI_GATE)
    assert R.w4_ok(**ok)
    for kw in (dict(K=192), dict(K=128), dict(K=320), dict(M=511), dict(N=120), dict(N=4100), dict(ldc=4100), dict(ldr=4098), dict(lda=2 ** 23), dict(ldw=2 ** 23)):
        assert not R.w4_ok(**{**ok, **kw}), kw
    assert R.w4_ok(**{**ok, "ldr": 4098, "epi": EPI_BIAS})
    # the four-wave kernel's 32-bit terms: 16 * 7 + 143 = 255 rows of ld elements plus the K advance, as bytes in a signed int
    for K, ld in ((256, 4210000), (256, 4210752 - 8), (1792, 4200000)):
        assert R.w4_ld_ok(K, ld) == ((16 * 7 * ld * 2 + 143 * ld * 2 + 2 * K) < 2 ** 31)
    assert R.w4_ld_ok(256, 4210000) and not R.w4_ld_ok(256, 4210752)
    # the 8-wave kernel's 32-bit row offsets
    assert R.k8_fits(600, 256, 128, 136, 200) and not R.k8_fits(600, 256, 128, 3585120, 200) and not R.k8_fits(600, 256, 128, 136, 8421512)
    assert R.plan(600, 256, 128, 3585120, 200, 264, 0, EPI_BIAS, 256, kernel=8).kernel == "glds" and R.plan(600, 256, 128, 136, 200, 264, 0, EPI_BIAS, 256, kernel=8).kernel == "k8"
    # split_tail, tail_kind, the 8-wave cost rule
    assert R.split_tail(264, 256, True) == (256, 8, True) and R.split_tail(264, 256, False) == (256, 8, False) and R.split_tail(384, 256, True) == (256, 128, False)
    assert R.split_tail(200, 256, True) == (0, 200, False) and R.split_tail(512, 256, True) == (512, 0, False) and R.split_tail(264, 304, True) == (0, 264, False)
    assert R.tail_kind(256, 8) == "q4" and R.tail_kind(256, 64) == "q4" and R.tail_kind(256, 65) == "glds" and R.tail_kind(192, 8) == "glds" and R.tail_kind(320, 8) == "glds"
    assert R.k8_rows(5952, 1792, 256) == 192 and R.k8_rows(4096, 4096, 256) == 256 and R.k8_rows(8348, 2039, 256) == 256 and R.k8_rows(8348, 2039, 304) == 256 and R.k8_rows(700, 511, 304) == 192
    # kept tiles of the frame-causal scores
    assert R.kept_counts(5000, 5000, 0) == [20] * 20 and R.kept_counts(5000, 5000, 1000) == [4] * 3 + [8] * 4 + [12] * 4 + [16] * 4 + [20] * 5
    assert R.plan_f32(5000, 5000, 256, 264, 328, 5004, 1000, 256).kernel == "w4" and R.plan_f32(5000, 5000, 256, 264, 328, 5001, 1000, 256).kernel == "glds"
    assert R.plan_f32(1500, 1500, 256, 264, 328, 1504, 0, 256).kernel == "glds" and R.plan_f32(5000, 5000, 192, 200, 264, 5004, 1000, 256).kernel == "glds"


def test_table_rows_reach_the_paths_they_are_named_for():
    """at 256 CUs: every row's expectation is what the mirror says, and the table as a whole reaches every kernel, tile height, tail form and
    epilogue with a ragged row, strided operands, scalar stores and vector stores where the launcher lets that kernel take them"""
    seen = collections.defaultdict(set)
    for row in R.ALL_ROWS:
        for name, epi, use_bias, inplace in R.forms_of(row):
            p = R.row_plan(row, epi, inplace, CUS)
            assert (p.kernel, p.rows, p.tail) == row.expect, (row.id, name, p)
            path = (p.kernel, p.rows, p.tail)
            tile_m, tile_n = p.rows, (128 if p.kernel in ("reg", "glds") else 256)
            seen[path] |= {R.EPI_NAMES[epi], "strided"}
            if row.M % tile_m or row.N % tile_n:
                seen[path].add("ragged")
            seen[path].add("vector" if (row.N + row.pad) % 4 == 0 else "scalar")
            if p.second_tile:
                seen[path].add("second tile")
    every = {"bias", "bias_m", "gelu", "gate", "ragged", "strided", "vector"}
    for path in (("reg", 128, None), ("glds", 128, None), ("k8", 192, None), ("k8", 256, None), ("k8", 256, "glds")):
        assert seen[path] >= every | {"scalar"}, (path, seen[path])
    for path in (("w4", 256, None), ("w4", 192, None), ("w4", 128, None), ("w4", 256, "q4"), ("w4", 256, "glds")):
        assert seen[path] >= every and "scalar" not in seen[path], (path, seen[path])      # ldc % 8 == 0 is a condition of the kernel
    assert all("second tile" in seen[p] for p in (("w4", 256, None), ("w4", 192, None), ("w4", 128, None), ("k8", 192, None)))
    assert {r.K for r in R.REG_ROWS} == {8, 40, 72, 136, 200} and {r.K // BK for r in R.GLDS_ROWS} == {1, 2, 3, 5}
    assert {r.pad for r in R.REG_ROWS} == {1, 3, 4} == {r.pad for r in R.GLDS_ROWS} and {r.N for r in R.REG_ROWS} >= {1, 3}
    assert {r.K // BK for r in R.K8_ROWS} == {2, 3, 5} and {r.K // BK for r in R.W4_SMALL} == {4, 6, 8, 10}
    assert {(r.K // BK) % 3 for r in R.W4_SMALL if r.tile == 128} == {0, 1, 2}
    assert {((r.M + 255) // 256) % 4 for r in R.W4_Q4} == {1, 2, 3} and {r.K // BK for r in R.W4_Q4} == {4, 6}
    p = R.row_plan(R.W4_GLDS_TAIL[0], EPI_BIAS, False, CUS)
    assert 4 * p.rem > 256 and 2 * p.rem < CUS
    p = R.row_plan(R.W4_NATURAL[0], EPI_BIAS, False, CUS)
    assert p.tiles >= 96 and R.W4_NATURAL[0].kernel == 0
    for row in R.HAND_ON:
        twin = R.Row(row.M, row.N, row.K, 8, 4 if row.kernel == 4 else 0, row.tile, ldr_pad=12)
        assert R.row_plan(twin, EPI_GATE, False, CUS).kernel == "w4" and R.row_plan(row, EPI_GATE, False, CUS).kernel != "w4"
    for M, N, K, pad, hw, kernel in R.F32_ROWS:
        assert R.plan_f32(M, N, K, K + R.LDA_PAD, K + R.LDW_PAD, N + pad, hw, CUS).kernel == kernel
    assert {r[5] for r in R.F32_ROWS} == {"reg", "glds", "w4"} and {r[3] for r in R.F32_ROWS} == {1, 4}
    assert any(128 % r[4] == 0 for r in R.F32_ROWS if r[4]) and any(128 % r[4] for r in R.F32_ROWS if r[4])
    # a second CU count: the mirror is not a constant
    assert any((lambda p: (p.kernel, p.rows, p.tail))(R.row_plan(r, EPI_BIAS, False, 304)) != r.expect for r in R.ALL_ROWS)


# ------------------------------------------------------------------------------------------------ DMA footprint
def test_dma_footprint_stays_inside_the_guard_rows():
    worst = {}
    for form in (256, 192, 128, "q4"):
        for operand in ("w", "x"):
            span = 128 if form == "q4" or (form == 128 and operand == "x") else 256
            for ld, K in ((264, 256), (328, 256), (1800, 1792)):
                for rows in range(1, span + 1):
                    touched = R.w4_dma_rows(form, operand, rows, ld, K)
                    assert set(range(rows)) <= set(touched)                           # every valid row is fetched
                    for mem, image in touched.items():
                        assert image == mem and (mem < rows or image >= rows)         # a row past the valid ones lands in an image row that is never stored
                    past = R.w4_rows_past(form, operand, rows, ld, K)
                    worst[(form, operand)] = max(worst.get((form, operand), 0), past)
    assert worst == {(256, "w"): 143, (256, "x"): 143, (192, "w"): 143, (192, "x"): 143, (128, "w"): 143, (128, "x"): 15, ("q4", "w"): 15, ("q4", "x"): 15}, worst
    assert R.w4_rows_past(256, "x", 1, 264, 256) == 143 and R.w4_rows_past(256, "x", 113, 264, 256) == 143 and R.w4_rows_past(256, "x", 256, 264, 256) == 0
    assert max(worst.values()) < R.OPERAND_GUARD_ROWS
    for row in R.ALL_ROWS:
        for name, epi, use_bias, inplace in R.forms_of(row):
            p = R.row_plan(row, epi, inplace, CUS)
            assert R.footprint_of_call(p, row.M, row.N, row.K, row.K + R.LDA_PAD, row.K + R.LDW_PAD) < R.OPERAND_GUARD_ROWS
    # the engine's V^T projection: the weight matrix W_v is the A operand, D = 1792 rows.  1792 = 9 * 192 + 64: on the 192-row tile, which the
    # launcher picks for the token-shard shapes, 128 rows past the END OF THE WEIGHTS are read — packed weights need guard rows as activations do
    guard = int(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kandinsky-5_amd", "csrc", "k5_kernels.h")).read().split("K5_GEMM_GUARD_ROWS =")[1].split(";")[0])
    assert guard == 144
    picked = set()
    for tokens in (3328, 5952, 11904, 47616):
        for tile in (0, 128, 192, 256):
            p = R.plan(1792, tokens, 1792, 1792, 1792, (tokens + 7) // 8 * 8, 0, EPI_BIAS_M, CUS, 4 if tile else 0, tile)
            past_x, past_w = R.footprint_per_operand(p, 1792, tokens, 1792, 1792, 1792)
            assert p.kernel == "w4" and past_x < guard and past_w < guard
            assert past_x == (128 if p.rows == 192 else 0), (tokens, tile, p, past_x)
            picked.add((tokens, p.rows) if tile == 0 else None)
    assert (5952, 192) in picked and (11904, 192) in picked
    # a NaN in a guard row cannot reach a stored element: an MFMA output (m, n) only sums products of image row m of X and image row n of W, and
    # the rows fetched from beyond the valid ones sit at image rows >= rows, whose outputs fail the epilogue's m < M / n < N predicate (above)


# ------------------------------------------------------------------------------------------------ diagnosis
def test_explain_names_the_element_its_owner_and_the_mutant():
    row = [r for r in R.K8_ROWS if (r.M, r.N, r.K) == (700, 511, 320)][0]
    c = case_of(row, EPI_BIAS)
    want = R.int_ref(c, EPI_BIAS, True)
    p = R.row_plan(row, EPI_BIAS, False, CUS)
    assert R.explain(want, want, c, p) == "no mismatch"
    got = want.clone()
    got[283, 77] ^= 1
    got[699, 510] ^= 1
    text = R.explain(got, want, c, p, EPI_BIAS, True)
    assert "2 mismatches in 2 rows and 2 columns" in text and "(m=283, n=77)" in text and "no single mutant" in text
    # 192-row tiles: row 283 = 192 + 91 -> tile 1, wave row 91 // 48 = 1, j = (91 % 48) // 16 = 2, lane row 11; column 77: wn 0, i = 4, lc = 3, e = 1
    assert "'tile': (1, 0)" in text and "'wave': 2" in text and "'lane': 59" in text and "'i': 4, 'j': 2, 'e': 1" in text and "'lane_row': 283" in text
    name, bits = [m for m in R.mutants(c, EPI_BIAS, True) if "K-tile 4 dropped" in m[0]][0]
    assert "K-tile 4 dropped" in R.explain(bits, want, c, p, EPI_BIAS, True) and "last K-tile" not in R.explain(bits, want, c, p, EPI_BIAS, True)
    small = R.Row(129, 129, 72, 3)
    cs = case_of(small, EPI_GATE)
    ws = R.int_ref(cs, EPI_GATE, True)
    bad = [b for n, b in R.mutants(cs, EPI_GATE, True, 132, 135) if "ldc instead of ldr" in n][0]
    assert "residual read with ldc instead of ldr" in R.explain(bad, ws, cs, R.row_plan(small, EPI_GATE, False, CUS), EPI_GATE, True, 132, 135)
    q = R.owner(R.Plan("w4", 256, "q4"), 300, 200)
    assert q["quadrant"] == 1 and q["tile"] == (1, 0) and q["tail"] == "q4"
