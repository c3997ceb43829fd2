"""The NABLA map and the list walk on DESIGNED maps, bit for bit (MI355X, through the C ABI).

tests/nabla_probe_reference.py builds q / k whose block map is known in advance (hot colour sets, a margin >= 1e-3 between every entry's
cumulative mass and the cut — asserted on the CPU by tests/test_nabla_probe_host.py), so k5_nabla_select_bf16 must give `want` with NO
allowance: a select kernel that is wrong for one lane, one word or one tie rank differs in a known entry.  The same maps then drive the
list walk of the block-sparse attention on census codes (Q = 0, one-hot values: every output element is a ratio of integer counts, a
skipped / doubled / foreign block moves it by O(1 / kept)) and on key probes (tests/test_gpu_attention_edges.py's construction).

What each test reaches:
  test_map_bit_for_bit       nabla_select_row_kernel<NV> for NV = 4, 8, 16, 24, 32, 48, 64 (the table's row lengths), block_mean_kernel on
                             strided rows, both special-cased STA divisions, tie ranks, the "smallest positive value" bracket, P = 1
  test_rect_rows             the rect select: global / local query index, rows_per_head padding, the second head's row stride
  test_refusals              K5_ERR_UNSUPPORTED above SEL_MAXNB = 4096 blocks, K5_ERR_ARG on a grid that is not N / 64
  test_census_square         nabla_union_kernel (no local sweep: lm = 0) + the sparse walk, online (attn_fwd32 SPARSE) and fixed-offset form
  test_census_rect           the same on rect lists (ragged last group of rows) with V^T in chunks of 33 blocks
  test_census_two_pass       the local-first sweep (lm inside a word, lm = ~0 for hi - lo == 64, a local range of one bit at either end, a
                             range no row of a group keeps) + the prescaled list walk in one pass and in two, fixed and online launches
  test_key_probes            the sparse walk's key / value addressing at the first and last key of kept, word-edge and dropped blocks"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import nabla_probe_reference as R  # noqa: E402
from oracle import parity  # noqa: E402
from test_gpu_attention_edges import PROBE_TOL, dev, rms8  # noqa: E402
from kit import BF, E, K5_ERR_ARG, K5_ERR_UNSUPPORTED, bfr  # noqa: E402


def wide(x):
    """(N, H, 64) -> the middle third of the columns of an (N, 3 H 64) bf16 buffer whose other columns hold 1000.0"""
    N, H, _ = x.shape
    buf = torch.full((N, 3 * H * 64), 1000.0, dtype=BF, device="cuda")
    view = buf[:, H * 64:2 * H * 64]
    view.copy_(x.reshape(N, H * 64))
    assert view.stride(0) == 3 * H * 64
    return view


def assert_map(got, want, what):
    want = want.to(got.device)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        h, i, j = bad[0].tolist()
        raise AssertionError(f"{what}: {len(bad)} of {want.numel()} map entries differ; first at head {h}, row {i}, key block {j} "
                             f"(word {j // 64}, bit {j % 64}): got {bool(got[h, i, j])}, want {bool(want[h, i, j])}; rows {sorted(set(bad[:, 1].tolist()))[:8]}")


# ------------------------------------------------------------------------------------------ 1. the map, bit for bit
@pytest.mark.parametrize("layout", ["flat", "spike"])
@pytest.mark.parametrize("name", list(R.MAP_ROWS))
def test_map_bit_for_bit(E, name, layout):
    case = R.table_case(name, layout)
    H, nb = case["H"], case["nb"]
    ws = E.nabla_select(wide(case["q"]), wide(case["k"]), H, case["grid"], case["window"], case["P"])
    assert_map(E.nabla_mask(ws, H, nb), case["want"], f"{name} ({nb} blocks, {layout})")


@functools.lru_cache(maxsize=None)
def _square(name):
    """the square select of a table row, its map asserted: (case, workspace)"""
    from kandinsky import _engine as E
    case = R.table_case(name)
    ws = E.nabla_select(dev(case["q"]), dev(case["k"]), case["H"], case["grid"], case["window"], case["P"])
    assert_map(E.nabla_mask(ws, case["H"], case["nb"]), case["want"], name)
    return case, ws


def rect_select(E, case, q0, nqb, local=None):
    """k5_nabla_select_rect[_local]_bf16 on query blocks [q0, q0 + nqb) + k5_nabla_mask_rect_u8, asserted equal to those rows of `want`"""
    L = E.lib()
    H, nb, N = case["H"], case["nb"], case["N"]
    qd, kd = dev(case["q"][64 * q0:64 * (q0 + nqb)]), dev(case["k"])
    ws = torch.empty(L.k5_nabla_workspace_size(H, nb), dtype=torch.uint8, device="cuda")
    args = (qd.data_ptr(), kd.data_ptr(), qd.stride(0), kd.stride(0), H, nqb * 64, q0, N, *case["grid"], *case["window"], case["P"], ws.data_ptr())
    if local is None:
        E.check(L.k5_nabla_select_rect_bf16(*args, E.stream_ptr()), "k5_nabla_select_rect_bf16")
    else:
        E.check(L.k5_nabla_select_rect_local_bf16(*args, local[0], local[1], E.stream_ptr()), "k5_nabla_select_rect_local_bf16")
    m = torch.empty(H, nqb, nb, dtype=torch.uint8, device="cuda")
    E.check(L.k5_nabla_mask_rect_u8(ws.data_ptr(), H, nqb, nb, m.data_ptr(), E.stream_ptr()), "k5_nabla_mask_rect_u8")
    assert_map(m.bool(), case["want"][:, q0:q0 + nqb], f"rect rows {q0}..{q0 + nqb} of {nb}, local {local}")
    return ws


@pytest.mark.parametrize("rect", range(5))
@pytest.mark.parametrize("name", R.RECT_ROWS)
def test_rect_rows(E, name, rect):
    case = R.table_case(name)
    rect_select(E, case, *R.rects(case["nb"])[rect])


def test_refusals(E):
    L = E.lib()
    T, Hb, Wb = 17, 241, 1                                              # 4097 blocks: one beyond SEL_MAXNB
    N = T * Hb * Wb * 64
    q = torch.zeros(N, 64, dtype=BF, device="cuda")
    ws = torch.full((L.k5_nabla_workspace_size(1, N // 64),), 0x5A, dtype=torch.uint8, device="cuda")
    rc = L.k5_nabla_select_bf16(q.data_ptr(), q.data_ptr(), 64, 64, 1, N, T, Hb, Wb, 3, 3, 1, 0.9, ws.data_ptr(), E.stream_ptr())
    torch.cuda.synchronize()
    assert rc == K5_ERR_UNSUPPORTED, rc
    assert bool((ws == 0x5A).all())
    n = 65 * 64
    ws = torch.full((L.k5_nabla_workspace_size(1, 65),), 0x5A, dtype=torch.uint8, device="cuda")
    rc = L.k5_nabla_select_bf16(q.data_ptr(), q.data_ptr(), 64, 64, 1, n, 13, 5, 2, 3, 3, 1, 0.9, ws.data_ptr(), E.stream_ptr())
    torch.cuda.synchronize()
    assert rc == K5_ERR_ARG, rc
    assert bool((ws == 0x5A).all())


# ------------------------------------------------------------------------------------------ 2. census of the list walk
@functools.lru_cache(maxsize=2)
def _codes(N, H):
    """V^T [H * 64][N] per census code, on the device"""
    return {c: v.reshape(N, H * 64).cuda().t().contiguous() for c, v in R.census_codes(N, H).items()}


def _chunked(vt, blocks=33):
    """[H * 64][N] -> per-rank chunks [chunk][H * 64][blocks * 64], the last one short; the buffer is allocated whole and its tail holds 3.0"""
    D, N = vt.shape
    ck = blocks * 64
    nch = (N + ck - 1) // ck
    full = torch.full((D, nch * ck), 3.0, dtype=BF, device="cuda")
    full[:, :N] = vt
    return full.reshape(D, nch, ck).permute(1, 0, 2).contiguous(), ck, D * ck


def _random_keys(N, H, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(N + H)
    return (scale * torch.randn(N, H * 64, device="cuda", generator=g)).to(BF)


def check_census(o, mask_rows, code, what, other=None):
    """o [rows * 64][H * 64] from the kernel against census_expect of mask_rows (H, rows, nb): finite, |got - want| <= 2^-8 want, exact zeros;
    other: a second result that must agree with o to the same bound"""
    H, rows, _ = mask_rows.shape
    got = o.float()
    assert torch.isfinite(got).all(), f"{what}, code {code}: {int((~torch.isfinite(got)).sum())} non-finite values"
    for h in range(H):
        want = R.census_expect(mask_rows[h], code, h).cuda()[:, None, :]                  # (rows, 1, 64)
        g = got[:, 64 * h:64 * h + 64].reshape(rows, 64, 64)
        ok = R.census_close(g, want)
        if not ok.all():
            r, i, d = (~ok).nonzero()[0].tolist()
            raise AssertionError(f"{what}, code {code}, head {h}: {int((~ok).sum())} elements off; first at query block {r}, row {i}, digit {d}: "
                                 f"got {g[r, i, d].item():.6g}, want {want[r, 0, d].item():.6g} (kept {int(mask_rows[h, r].sum())} blocks)")
        if other is not None:
            g2 = other.float()[:, 64 * h:64 * h + 64].reshape(rows, 64, 64)
            assert ((g - g2).abs().double() <= R.CENSUS_TOL * want).all(), f"{what}, code {code}, head {h}: the two schedules disagree"


@pytest.mark.parametrize("score_bound", [0.0, 1.0])
@pytest.mark.parametrize("name", R.ATTN_ROWS)
def test_census_square(E, name, score_bound):
    """k5_attention_nabla_bf16 on the square map: score_bound 0 = the online kernel, 1.0 = the fixed-offset kernel (Q = 0: |q.k| = 0)"""
    case, ws = _square(name)
    H, nb, N = case["H"], case["nb"], case["N"]
    q, k = torch.zeros(N, H * 64, dtype=BF, device="cuda"), _random_keys(N, H)
    for code, vt in _codes(N, H).items():
        o = torch.full((N, H * 64), float("nan"), dtype=BF, device="cuda")
        E.attention_nabla(q, k, vt, H, ws, score_bound=score_bound, out=o)
        check_census(o, case["want"], code, f"{name}, score_bound {score_bound}")


@pytest.mark.parametrize("rect", range(5))
@pytest.mark.parametrize("name", R.RECT_ROWS)
def test_census_rect(E, name, rect):
    """k5_attention_nabla_rect_bf16 on rect lists, V^T in chunks of 33 blocks, both softmax forms"""
    case = R.table_case(name)
    H, nb, N = case["H"], case["nb"], case["N"]
    q0, nqb = R.rects(nb)[rect]
    ws = rect_select(E, case, q0, nqb)
    L, n = E.lib(), nqb * 64
    q, k = torch.zeros(n, H * 64, dtype=BF, device="cuda"), _random_keys(N, H)
    for code, vt in _codes(N, H).items():
        chunks, ck, cstride = _chunked(vt)
        for sb in (0.0, 1.0):
            o = torch.full((n, H * 64), float("nan"), dtype=BF, device="cuda")
            E.check(L.k5_attention_nabla_rect_bf16(q.data_ptr(), k.data_ptr(), chunks.data_ptr(), o.data_ptr(), H, n, N, q.stride(0), k.stride(0),
                                                   ck, o.stride(0), sb, ws.data_ptr(), ck, cstride, E.stream_ptr()), "k5_attention_nabla_rect_bf16")
            check_census(o, case["want"][:, q0:q0 + nqb], code, f"{name} rows {q0}..{q0 + nqb}, score_bound {sb}")


def _far_range(case, q0, nqb):
    """a local range of 3 blocks that the LAST group of four query rows of head 0 does not keep at all: no entry in pass 1 for that group"""
    rows = case["want"][0, q0 + (nqb - 1) // 4 * 4:q0 + nqb]
    free = ~rows.any(0)
    return next((s, 3) for s in range(case["nb"] - 3, -1, -1) if free[s:s + 3].all())


@pytest.mark.parametrize("force_online", [0, 1])
@pytest.mark.parametrize("pair", range(5))
@pytest.mark.parametrize("name", R.RECT_ROWS)
def test_census_two_pass(E, name, pair, force_online):
    """k5_nabla_select_rect_local_bf16 + k5_attention_nabla_rect_prescaled_pass: pass 0, and passes 1 + 2 on one state buffer; flags from
    k5_attention_flags_rows.  Local ranges: inside / across words, exactly one word (hi - lo == 64), one bit at either end, and one that the
    last row group does not keep (nothing to do in pass 1)."""
    case = R.table_case(name)
    H, nb, N = case["H"], case["nb"], case["N"]
    (q0, nqb), local = [(R.rects(nb)[0], None), (R.rects(nb)[1], (60, 10)), (R.rects(nb)[2], (nb - 1, 1)), (R.rects(nb)[3], (0, 1)),
                        (R.rects(nb)[4], (64, 64))][pair]
    if local is None:
        local = _far_range(case, q0, nqb)
    ws = rect_select(E, case, q0, nqb, local)
    L, n = E.lib(), nqb * 64
    q, kc = torch.zeros(n, H * 64, dtype=BF, device="cuda"), _random_keys(N, H, 0.18)
    mask_rows = case["want"][:, q0:q0 + nqb]

    def run(passes, chunks, ck, cstride):
        qstat = torch.zeros(H, device="cuda")
        kstat = kc.float().reshape(N, H, 64).pow(2).sum(-1).amax(0).contiguous()
        flags, kmax = torch.zeros(H, dtype=torch.int32, device="cuda"), torch.zeros(H, device="cuda")
        E.check(L.k5_attention_flags_rows(qstat.data_ptr(), kstat.data_ptr(), 1, H, H, force_online, flags.data_ptr(), kmax.data_ptr(), E.stream_ptr()))
        torch.cuda.synchronize()
        assert flags.tolist() == [0 if force_online else 1] * H, flags
        o = torch.full((n, H * 64), float("nan"), dtype=BF, device="cuda")
        state = torch.zeros(L.k5_attention_state_size(H, n) // 4, device="cuda")
        for ps in passes:
            E.check(L.k5_attention_nabla_rect_prescaled_pass(q.data_ptr(), kc.data_ptr(), chunks.data_ptr(), o.data_ptr(), H, n, N, q.stride(0),
                                                             kc.stride(0), ck, o.stride(0), ws.data_ptr(), ck, cstride, flags.data_ptr(),
                                                             kmax.data_ptr(), ps, state.data_ptr(), E.stream_ptr()),
                    "k5_attention_nabla_rect_prescaled_pass")
            torch.cuda.synchronize()
            print(f"{name} rows {q0}..{q0 + nqb}, local {local}, force_online {force_online}: head flags after pass {ps}: {flags.tolist()}")
        return o

    for code, vt in _codes(N, H).items():
        cargs = _chunked(vt)
        one, two = run([0], *cargs), run([1, 2], *cargs)
        what = f"{name} rows {q0}..{q0 + nqb}, local {local}, force_online {force_online}"
        check_census(one, mask_rows, code, what + ", one pass")
        check_census(two, mask_rows, code, what + ", two passes", other=one)


# ------------------------------------------------------------------------------------------ 3. key probes on the designed maps
@functools.lru_cache(maxsize=None)
def _vtable(N, H):
    """as test_gpu_attention_edges.vcode, N rows long: integers / 128 in [-125, 125] / 128 (bf16-exact) from a fixed seed"""
    return (torch.randint(-125, 126, (N, H * 64), generator=torch.Generator().manual_seed(641 + N)).float() / 128.0).reshape(N, H, 64)


@pytest.mark.parametrize("name", R.RECT_ROWS)
def test_key_probes(E, name):
    """From up to 8 query blocks (the first, the last, those around the word edge): q_i = 8 k_j at the first and last key of the block's first and
    last kept block, of a kept block at a word edge and of a DROPPED block next to a kept one.  A kept probe must land on V[j]; a dropped one
    must match the masked float64 reference, which ignores that key.  The reference covers the probed query blocks only."""
    case, ws = _square(name)
    H, nb, N, want = case["H"], case["nb"], case["N"], case["want"]
    qblocks = [0, 1, 62, 63, 64, 65, nb - 2, nb - 1]
    g = torch.Generator().manual_seed(nb)
    k = bfr(rms8(torch.randn(N, H, 64, generator=g)))
    q = rms8(torch.randn(N, H, 64, generator=g))
    probes = []                                                         # (row, head, key, kept)
    for h in range(H):
        seen = {}
        for r, j, kept in R.probe_rows(want[h], qblocks):
            seen[r] = seen.get(r, -1) + 1
            probes.append((64 * r + 3 + 7 * seen[r], h, j, kept))
    assert any(not kept for *_, kept in probes) and any(j // 64 in (63, 64, 127, 128) for _, _, j, kept in probes if kept)
    for row, h, j, _ in probes:
        q[row, h] = 8.0 * k[j, h]
    q = bfr(q)
    v = _vtable(N, H)
    vt = v.reshape(N, H * 64).t().contiguous().cuda().to(BF)
    got = E.attention_nabla(dev(q), dev(k), vt, H, ws)
    torch.cuda.synchronize()
    sel = torch.cat([torch.arange(64 * r, 64 * r + 64) for r in qblocks])
    got = got[sel.cuda()].float().cpu()
    assert torch.isfinite(got).all()
    Rf = parity.AttentionRef(q[sel], k, v, block_mask=want[:, qblocks])
    err = parity.row_rel_err(got, Rf.f64, H)
    yard = parity.yardstick(Rf.bf16, Rf.f64, H)
    pos = {int(r): i for i, r in enumerate(sel.tolist())}
    for row, h, j, kept in probes:
        ref_row = Rf.f64[pos[row], 64 * h:64 * h + 64]
        if kept:
            assert (ref_row - v[j, h].double()).abs().max().item() < 1e-6, (row, h, j)       # the reference IS the key's value row
        else:
            assert (ref_row - v[j, h].double()).norm().item() > 0.1 * ref_row.norm().item(), (row, h, j)   # and here it is not: the key is masked
        tol = PROBE_TOL if kept else parity.MARGIN_SPARSE * yard
        e = err[pos[row], h].item()
        assert e <= tol, f"{name}: probe row {row} head {h} at {'kept' if kept else 'DROPPED'} key {j} (block {j // 64}): off by {e:.3g} of its row"
    Rf.close(got, parity.MARGIN_SPARSE, f"{name}: key probes, all rows of the probed blocks")
