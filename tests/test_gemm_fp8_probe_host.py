"""CPU checks of tests/gemm_fp8_probe_reference.py, the reference of tests/test_gpu_gemm_fp8_probes.py: the expected bits equal an
independent float64 evaluation, the operands are what the bytes say, and — mutation by mutation — every small case of the GPU table gives a
DIFFERENT output under each wrong indexing a kernel could have, so a GPU run that passes is known to tell them apart."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fp8_probe_reference as R  # noqa: E402
from gemm_fp8_probe_reference import BF, BK, EPI_BIAS, EPI_GATE, EPI_GELU, F8  # noqa: E402

shape_id = lambda s: "x".join(map(str, s))
# (shape, kind, epilogue, bias): every small row of the GPU table under every epilogue it runs there
ROWS = [(s, "gelu" if e == EPI_GELU else "int", e, False) for s in R.SMALL_ROWS for e in (EPI_BIAS, EPI_GELU, EPI_GATE)]
ROWS += [(R.BIAS_N_K8, "gelu" if e == EPI_GELU else "int", e, True) for e in (EPI_BIAS, EPI_GELU, EPI_GATE)]
ROWS += [(s, "scale_m", EPI_BIAS, b) for s in R.SCALE_M_K8 for b in (True, False)]
row_id = lambda r: f"{shape_id(r[0])}-{r[1]}-{R.EPI_NAMES[r[2]]}{'-bias' if r[3] else ''}"
_cases = {}


def case_of(shape, kind, a_tile=None):
    key = (shape, kind, a_tile)
    if key not in _cases:
        _cases[key] = R.probe_case(*shape, kind, a_tile)
    return _cases[key]


def zero_sign(t):
    return torch.where(t == 0x80, torch.zeros_like(t), t) if t.dtype == torch.uint8 else t


def differs(a, b):
    return not torch.equal(zero_sign(a), zero_sign(b))


# ------------------------------------------------------------------------------------------------ the number formats
def test_e4m3_rounding_matches_torch_and_the_named_ties():
    codes = torch.arange(256, dtype=torch.uint8)
    finite = codes[(codes & 0x7f) != 0x7f]
    assert torch.equal(R.e4m3_rne(R.e4m3_value(finite)), finite)                      # every value is its own code, -0 included
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(20000, generator=g) * s for s in (0.003, 0.05, 1.0, 30.0, 150.0)]).clamp(-448, 448)
    assert torch.equal(R.e4m3_rne(x.double()), x.to(F8).view(torch.uint8))
    mids = ((R._POS[1:] + R._POS[:-1]) / 2)                                            # exact in fp32: every tie against torch's rounding
    assert torch.equal(R.e4m3_rne(mids), mids.float().to(F8).view(torch.uint8)) and torch.equal(R.e4m3_rne(-mids), (-mids).float().to(F8).view(torch.uint8))
    val = lambda v: float(R.e4m3_value(R.e4m3_rne(torch.tensor([v], dtype=torch.float64)))[0])
    for v, w in ((17.0, 16.0), (19.0, 20.0), (2.0 ** -10, 0.0), (3 * 2.0 ** -10, 2.0 ** -8), (448.0, 448.0), (464.0, 448.0), (480.0, 448.0),
                 (1e4, 448.0), (math.inf, 448.0), (2.0 ** -10 * 1.001, 2.0 ** -9), (463.0, 448.0)):
        assert val(v) == w and val(-v) == -w, v
    assert int(R.e4m3_rne(torch.tensor([-0.0]))[0]) == 0x80 and int(R.e4m3_rne(torch.tensor([0.0]))[0]) == 0


def test_static_quantiser_rows_hold_every_edge():
    x, want = R.quant_static_rows()
    got = R.e4m3_value(R.quant_static_ref(x))
    xs = x.double()
    for v, w in want.items():
        assert bool((xs == float(torch.tensor(v).to(BF))).any()), v
        assert bool((got[xs == float(torch.tensor(v).to(BF))] == w).all()), v
    for k in range(1, 8):
        assert bool((got[xs == k * 2.0 ** -9] == k * 2.0 ** -9).all()) and bool((xs == -k * 2.0 ** -9).any())
    assert bool(torch.signbit(xs[xs == 0]).any()) and not bool(torch.signbit(xs[xs == 0]).all())          # both zeros
    assert bool((got[xs == -math.inf] == -448.0).all()) and bool((xs == -464.0).any()) and bool((xs == -480.0).any())
    inside = xs.abs() <= 448
    assert torch.equal(R.quant_static_ref(x)[inside], x[inside].to(F8).view(torch.uint8))


def test_per_row_quantiser_cases_hold_every_row_shape():
    seen = set()
    for rows in (1, 4, 5, 7):
        for K in (4, 252, 256, 260, 1792):
            for shift in (range(6) if rows == 1 else (0, 3)):
                x, kinds = R.quant_rows_case(rows, K, shift, R.seed_of(rows, K, shift))
                seen |= set(kinds)
                a = x.double().abs()
                for r, kind in enumerate(kinds):
                    top = int(a[r].argmax())
                    if kind == 0:
                        assert top == K - 1
                    elif kind == 1:
                        assert float(a[r].max()) == 0
                    elif kind == 2:
                        assert float(x[r, top]) < 0 and int((a[r] == a[r].max()).sum()) == 1
                    elif kind == 3:
                        assert top == 0
                    elif kind == 4:
                        assert top >= (K - 1) // 256 * 256
                s = torch.where(a.amax(1) > 0, a.amax(1) / 448, torch.ones(rows, dtype=torch.float64)).float()
                codes = R.quant_row_ref(x, s)
                assert bool((R.e4m3_value(codes).abs().amax(1)[a.amax(1) > 0] == 448).all())
    assert seen == set(range(6))
    assert int(R.ulps_apart(torch.tensor([1.0]), torch.tensor([1.0 + 2.0 ** -22]))[0]) == 2


# ------------------------------------------------------------------------------------------------ the reference against float64
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_int_ref_is_the_float64_product_and_the_bytes_are_the_operands(row):
    shape, kind, epi, use_bias = row
    c = case_of(shape, kind)
    a8, w8 = R.int_to_e4m3(c.A), R.int_to_e4m3(c.W)
    for codes, ints in ((a8, c.A), (w8, c.W)):
        assert torch.equal(codes.view(F8).float().to(F8).view(torch.uint8), codes) and torch.equal(codes.view(F8).to(torch.int8), ints)
    assert int(c.A.abs().max()) <= 3 and int(c.W.abs().max()) <= 4
    if kind != "gelu":
        assert 0.35 < float((c.A == 0).float().mean()) < 0.65 and 0.35 < float((c.W == 0).float().mean()) < 0.65
    e = torch.log2(c.scale.double())
    assert torch.equal(e, e.round()) and -3 <= float(e.min()) and float(e.max()) <= 2 and (len(e) < 8 or len(e.unique()) >= 3)
    q = c.bias.double() / c.scale.double()
    assert torch.equal(q, q.round())
    assert torch.equal(c.resid.double(), c.resid.double().round()) and set(c.gate.tolist()) <= set(R.GATES)
    # float64 matmul of the de-quantised operands, the epilogue formulas written out again
    acc = a8.view(F8).double() @ w8.view(F8).double().t()
    assert torch.equal(acc, c.acc.double()) and float(acc.abs().max()) < 2 ** 24
    s = c.scale.double()[:, None] if c.scale_m else c.scale.double()[None, :]
    b = (c.bias.double()[:, None] if c.scale_m else c.bias.double()[None, :]) if use_bias else 0.0
    bf = lambda t: t.float().to(BF)
    pre = bf(acc * s + b)
    want = R.int_ref(c, epi, use_bias)
    if epi == EPI_BIAS:
        assert torch.equal(pre.view(torch.int16), want)
    elif epi == EPI_GATE:
        assert torch.equal(bf(c.resid.double() + c.gate.double()[None, :] * pre.double()).view(torch.int16), want)
    else:
        gelu = torch.nn.functional.gelu(pre.double())
        assert not differs(gelu.float().to(F8).view(torch.uint8), want)
        assert len(want.unique()) >= (20 if min(shape[:2]) >= 16 else 3)           # a rich byte alphabet, not a few values


# ------------------------------------------------------------------------------------------------ mutants
def mutants(c, epi, use_bias):
    """(name, output bits) of every wrong kernel this case must tell from the right one"""
    M, N, K, nk = c.M, c.N, c.K, c.K // BK
    s2, b2 = R.channel2d(c, c.scale), (R.channel2d(c, c.bias) if use_bias else None)
    g2 = c.gate[None, :]
    out = lambda acc=c.acc, s=s2, b=b2, g=g2: R.finish(acc, epi, s, b, c.resid, g, strict=False)
    A, W = c.A.float(), c.W.float()
    for t in range(nk):
        if bool((c.A[:, t * BK:(t + 1) * BK] != 0).any()):
            drop = A.clone()
            drop[:, t * BK:(t + 1) * BK] = 0
            yield f"K-tile {t} dropped", out(acc=drop @ W.t())
    yield "last K-tile counted twice", out(acc=c.acc + A[:, -BK:] @ W[:, -BK:].t())
    swap = torch.arange(K) ^ 16
    yield "16-byte halves of A's 32-byte chunks swapped", out(acc=A[:, swap] @ W.t())
    yield "16-byte halves of W's 32-byte chunks swapped", out(acc=A @ W[:, swap].t())
    if M >= 2:
        yield "A row clamped to M - 2", out(acc=torch.cat([A[:-1], A[-2:-1]]) @ W.t())
    if N >= 2:
        yield "W row clamped to N - 2", out(acc=A @ torch.cat([W[:-1], W[-2:-1]]).t())
    mine, other = (M, N) if c.scale_m else (N, M)
    if mine >= 2:
        idx = torch.arange(other) % mine
        wrong = lambda v: v[idx][None, :] if c.scale_m else v[idx][:, None]
        yield "scale indexed by the other dimension", out(s=wrong(c.scale))
        if use_bias:
            yield "bias indexed by the other dimension", out(b=wrong(c.bias))
    if use_bias:
        yield "bias omitted", out(b=None)
        if mine >= 2:
            yield "bias of the next channel", out(b=R.channel2d(c, c.bias.roll(-1)))
    if epi == EPI_GATE and N >= 2:
        yield "gate taken from column n + 1", out(g=c.gate.roll(-1)[None, :])
        yield "residual taken from column n + 1", R.finish(c.acc, epi, s2, b2, c.resid.roll(-1, 1), g2, strict=False)
    base = out()
    group = 16 if epi == EPI_GELU else 8                     # elements of a 16-byte store group
    full = N // group * group
    for x in (1, 2, 4, 8):
        if x < group and full:
            cols = torch.arange(N)
            cols[:full] ^= x
            yield f"columns n ^ {x} within a 16-byte store group", base[:, cols]
    if full:
        cols = torch.arange(N)
        cols[:full] = (cols[:full] & ~3) | ((cols[:full] + 1) & 3)
        yield "columns rotated within a dword", base[:, cols]


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_every_mutant_changes_the_expected_output(row):
    shape, kind, epi, use_bias = row
    c = case_of(shape, kind)
    want = R.int_ref(c, epi, use_bias)
    assert not differs(R.finish(c.acc, epi, R.channel2d(c, c.scale), R.channel2d(c, c.bias) if use_bias else None, c.resid, c.gate[None, :], strict=False), want)
    names = []
    for name, got in mutants(c, epi, use_bias):
        assert differs(got, want), f"{row_id(row)}: '{name}' gives the expected output"
        names.append(name)
    assert len(names) >= 4 + (c.M >= 2) + (c.N >= 2)       # a dropped K-tile, the doubled one, the two half swaps, the clamps


@pytest.mark.parametrize("shape", R.SIGNATURE_K8 + R.SIGNATURE_W4, ids=shape_id)
def test_k_tile_signature_cases_name_their_k_tile(shape):
    """A lives in K-tile t only: the output must differ from what ANY other K-tile of W would give with those A values (a shifted or
    clamped K offset in one operand), from all zeros (tile dropped) and from twice the value (tile fetched twice)"""
    M, N, K = shape
    nk = K // BK
    tiles = R.signature_tiles(K)
    assert 0 in tiles and nk - 1 in tiles
    for t in tiles:
        c = case_of(shape, "int", t)
        assert not bool(c.A[:, :t * BK].any()) and not bool(c.A[:, (t + 1) * BK:].any()) and bool(c.A.any())
        want = R.int_ref(c, EPI_BIAS)
        s2 = c.scale[None, :]
        At = c.A[:, t * BK:(t + 1) * BK].float()
        assert differs(R.finish(torch.zeros_like(c.acc), EPI_BIAS, s2, None, strict=False), want)
        assert differs(R.finish(2 * c.acc, EPI_BIAS, s2, None, strict=False), want)
        for u in range(nk):
            got = R.finish(At @ c.W[:, u * BK:(u + 1) * BK].float().t(), EPI_BIAS, s2, None, strict=False)
            assert differs(got, want) == (u != t), (t, u)
            if u != t:
                assert float((got != want).float().mean()) > 0.5       # not a few elements: most of the output names the K-tile


# ------------------------------------------------------------------------------------------------ GELU alphabet
def test_gelu_alphabet_margin_and_the_values_actually_used():
    x, code, safe = R.gelu_alphabet()
    g = R.gelu64(x)
    bound = 2e-7 * x.abs() + 2.0 ** -22 * g.abs()
    mids = torch.cat([R._MID, -R._MID])
    dist = (g[:, None] - mids[None, :]).abs().min(1).values
    assert torch.equal(safe, dist >= 16 * bound)
    assert torch.equal(code, R.e4m3_rne(g)) and not differs(code[safe], g.float().to(F8).view(torch.uint8)[safe])
    unsafe = x[~safe]
    assert bool((unsafe >= 4.75).all()) and torch.equal(unsafe * 4 % 2, torch.ones_like(unsafe))       # the odd quarters where GELU(x) ~ x is a tie
    assert bool(safe[x == 0].all()) and float(dist[x == 0][0]) == 2.0 ** -10                              # the 0 <-> 2^-9 boundary is in the list
    # an evaluation that is off by the whole bound, either way, still rounds to the same byte on every safe value
    for sgn in (-1, 1):
        assert not differs(R.e4m3_rne(g + sgn * bound)[safe], code[safe])
    used = set()
    for shape in R.SMALL_ROWS + [R.BIAS_N_K8]:
        c = case_of(shape, "gelu")
        for use_bias in (False, True):
            pre = c.acc.double() * c.scale.double()[None, :] + (c.bias.double()[None, :] if use_bias else 0.0)
            assert float(pre.abs().max()) <= 8.0
            codes, ok = R.gelu_lookup(pre)
            assert bool(ok.all())
            used |= set(pre.unique().tolist())
    assert len(used) >= 60 and min(used) <= -4 and max(used) >= 6
    for e, (top, wmax) in R.GELU_COL.items():
        assert top < 4.75 or 2.0 ** e >= 0.5                  # the fine lattices stop below the first unsafe value


# ------------------------------------------------------------------------------------------------ table and diagnosis
def test_table_rows_reach_the_paths_they_are_named_for():
    """at the 256 CUs of an MI355X (the GPU test asserts the same against the machine's own count)"""
    for M, N, K in R.K8_ONE_TILE + R.K8_RAGGED + R.K8_WALK + R.SCALE_M_K8 + R.SIGNATURE_K8 + [R.BIAS_N_K8]:
        assert not (R.w4_ok(M, N, K, (N + 16) // 16 * 16, N + 12, EPI_BIAS) and R.tiles(M, N) >= 256), (M, N, K)
        assert K >= 2 * BK and K % BK == 0
    assert [K // BK for _, _, K in R.K8_ONE_TILE] == [2, 3, 5]
    assert R.tiles(*R.K8_WALK[0][:2]) == 2 and R.tiles(*R.K8_WALK[1][:2]) == 15 and (1100 + 255) // 256 % 4 == 1 and R.tiles(*R.K8_WALK[2][:2]) == 272
    for M, N, K in R.W4_NATURAL + R.SCALE_M_W4 + [R.BIAS_N_W4]:
        assert all(R.w4_ok(M, N, K, N + 16, ldr, e) for e in (EPI_BIAS, EPI_GELU, EPI_GATE) for ldr in (N + 16, N + 12)) and R.tiles(M, N) >= 256
    assert R.W4_NATURAL[0][0] % 256 == 4 and R.W4_NATURAL[0][2] == 4 * BK and R.W4_NATURAL[1][1] % 256 == 16
    for M, N, K in R.FORCED + R.SIGNATURE_W4:
        assert all(R.w4_ok(M, N, K, N + 16, ldr, e) for e in (EPI_BIAS, EPI_GELU, EPI_GATE) for ldr in (N + 16, N + 12)) and R.tiles(M, N) < 256
    assert all(N % 16 for _, N, _ in R.SCALE_M_K8)


def test_explain_names_the_element_and_its_owner():
    c = case_of((300, 130, 384), "int")
    want = R.int_ref(c, EPI_BIAS)
    assert R.explain(want, want, c) == "no mismatch"
    got = want.clone()
    got[283, 77] ^= 1
    got[299, 129] ^= 1
    text = R.explain(got, want, c)
    assert "2 mismatches in 2 rows and 2 columns" in text and "(m=283, n=77)" in text and "tile (m 1, n 0), row 27 column 77" in text
    # row 27 = 32 * 0 + 16 * 1 + 11, column 77 = 64 * 1 + 16 * 0 + 4 * 3 + 1
    assert "8-wave kernel: {'wave': 1, 'lane': 59, 'i': 0, 'j': 1, 'e': 1}" in text
    assert "4-wave kernel: {'wave': 0, 'lane': 59, 'i': 4, 'j': 1, 'e': 1}" in text
    g8 = R.int_ref(case_of((300, 130, 384), "gelu"), EPI_GELU)
    bad = g8.clone()
    bad[0, 0] ^= 0x10
    assert "first at (m=0, n=0)" in R.explain(bad, g8)
