"""The designed NABLA maps and census codes checked on the CPU (no GPU): every table row is what it claims to be, and the expectations of
tests/test_gpu_nabla_probes.py would notice the wrong kernels they are meant for."""
import pytest
import torch

import nabla_probe_reference as R
from oracle import k5_oracle as O

BF = torch.bfloat16


@pytest.mark.parametrize("name", list(R.MAP_ROWS))
def test_table_row_is_admissible_and_equals_the_oracle(name):
    """inputs bf16-exact, both token layouts give the same exact block means, margin >= 1e-3 with no tie group across the cut, and
    oracle.nabla_block_mask == want.  P = 1 rows: the oracle gives all ones, admissibility does not apply.  Tie rows: the margin holds for
    every entry, a tie group straddles the cut by design, and want is the stable-sort rule (the oracle's sort promises no order among equals)."""
    case = R.table_case(name)
    spike = R.table_case(name, "spike")
    H, nb = case["H"], case["nb"]
    for c in (case, spike):
        for t in (c["q"], c["k"]):
            assert t.shape == (nb * 64, H, 64) and torch.equal(t.to(BF).float(), t)
    for t in ("q", "k"):
        mean = lambda x: x.double().reshape(nb, 64, H, 64).mean(1)      # noqa: E731
        assert torch.equal(mean(case[t]), mean(spike[t]))
        assert not torch.equal(case[t], spike[t])
    m, straddle, warm = R.margin(case)
    hot = case["S"].sum(-1)
    print(f"{name}: {nb} blocks, margin {m:.3e}, hot sets of {int(hot.min())}-{int(hot.max())} blocks ({len(hot.unique())} sizes), "
          f"dropped warm mass >= {warm:.2e}, map density {case['want'].float().mean():.4f}")
    assert hot.min() >= 1
    assert torch.equal(case["want"] & case["sta"][None], case["sta"][None].expand(H, nb, nb))
    ref = O.nabla_block_mask(case["q"], case["k"], case["sta"], case["P"], "bf16")
    if case["P"] >= 1.0:
        assert ref.all() and case["want"].all()
        return
    if case["ties"]:
        assert m >= R.MARGIN and straddle
        assert not ((ref != case["want"]) & ~case["S"]).any()           # the oracle may differ only inside the hot tie group
        return
    assert R.admissible(case), (m, straddle)
    assert torch.equal(ref, case["want"])
    assert torch.equal(O.nabla_block_mask(spike["q"], spike["k"], spike["sta"], spike["P"], "bf16"), case["want"])


def test_table_covers_what_it_must():
    nbs = {n: r[0][0] * r[0][1] * r[0][2] for n, r in R.MAP_ROWS.items()}
    assert {64, 65, 258, 512, 513, 1025, 1537, 2050, 3075, 4096} <= set(nbs.values())
    nv = lambda nb: next(v for v in (4, 8, 16, 24, 32, 48, 64) if (nb + 63) // 64 <= v)      # noqa: E731  sel_row_nv of csrc/nabla.hip
    assert {nv(nb) for nb in nbs.values()} == {4, 8, 16, 24, 32, 48, 64}
    assert all(R.MAP_ROWS[n][3] == (2 if nb <= 513 else 1) for n, nb in nbs.items())
    assert {r[4] for r in R.MAP_ROWS.values()} >= {"bit", "word", "affine", "quad"}
    geo = [(r[0], r[1]) for n, r in R.MAP_ROWS.items() if 65 <= nbs[n] <= 258]
    assert any(Hb * Wb == 1 for (_, Hb, Wb), _ in geo) and any(Wb == 1 and Hb > 1 for (_, Hb, Wb), _ in geo)
    assert any((Hb * Wb) & (Hb * Wb - 1) and Wb & (Wb - 1) for (_, Hb, Wb), _ in geo)
    assert ((13, 5, 2), (4, 2, 2)) in geo and any(w == (1, 1, 1) for _, w in geo)
    assert any(w[1] // 2 >= g[1] and w[2] // 2 >= g[2] for g, w in geo)
    warm = [R.margin(R.table_case(n))[2] for n, r in R.MAP_ROWS.items() if isinstance(r[6], tuple)]
    assert warm and min(warm) >= 5e-3, warm
    assert any(r[6] == "deep" and r[2] < 1.0 for r in R.MAP_ROWS.values())
    assert {r[6] for r in R.MAP_ROWS.values() if r[2] >= 1.0} == {"two", "deep"}
    for n in R.MAP_ROWS:                                                # hot-set sizes vary by row and by head
        S = R.table_case(n)["S"].sum(-1)
        if R.MAP_ROWS[n][5][0] != R.MAP_ROWS[n][5][1]:
            assert len(S.unique()) > 1 and (S.shape[0] == 1 or not torch.equal(S[0], S[-1])), n


# ---------------------------------------------------------------------------------------------- wrong select kernels are seen
@pytest.mark.parametrize("name", R.SMALL_ROWS)
def test_select_model_gives_the_designed_map(name):
    case = R.table_case(name)
    assert torch.equal(R.select_model(case), R.padded(case["want"], case["nb"]))


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_a_wrong_select_changes_the_expected_map(mutation):
    """each mutation of the CPU model of the select differs from `want` in at least one entry of at least one small row (rect rows for the
    mutation that only a rect call can show)"""
    seen = []
    for name in (R.RECT_ROWS if mutation == "local_i" else R.SMALL_ROWS):
        case = R.table_case(name)
        q0, nqb = (61, 6) if mutation == "local_i" else (0, None)
        got = R.select_model(case, q0, nqb, mutation)
        want = R.padded(case["want"][:, q0:q0 + got.shape[1]], case["nb"])
        if not torch.equal(got, want):
            seen.append((name, int((got != want).sum())))
            break
    print(f"{mutation}: first seen on {seen}")
    assert seen, mutation


def test_rect_cases_fit():
    for name in R.RECT_ROWS:
        nb = R.table_case(name)["nb"]
        for q0, nqb in R.rects(nb):
            assert 0 <= q0 and q0 + nqb <= nb
        assert any(nqb % 4 for _, nqb in R.rects(nb)) and any(q0 < 64 < q0 + nqb for q0, nqb in R.rects(nb))


# ---------------------------------------------------------------------------------------------- wrong list walks are seen
def _seen(want, mutated):
    return bool(((mutated - want).abs() > 4 * R.CENSUS_TOL * want).any() or ((want == 0) != (mutated == 0)).any())


@pytest.mark.parametrize("name", R.ATTN_ROWS)
def test_a_wrong_list_walk_changes_the_expected_census(name):
    """On the query block with the fewest kept blocks of every head: a skipped, a doubled and a dropped-but-walked block, two blocks with
    swapped values, one skipped key and (two heads) the other head's columns each move some element of some code by more than 4 x the
    tolerance or flip a zero.  A kept set of one block could not show a doubled block: no such row may be in the table."""
    case = R.table_case(name)
    H, nb, want = case["H"], case["nb"], case["want"]
    assert want.sum(-1).min() >= 2
    for h in range(H):
        r = int(want[h].sum(-1).argmin())
        kept = want[h, r].nonzero().flatten().tolist()
        dropped = (~want[h, r]).nonzero().flatten().tolist()
        assert 2 <= len(kept) <= 60 and dropped
        base = {c: R.census_walk(kept, c, h, nb) for c in "ABC"}
        for c in "ABC":                                                 # the walk model and the closed form agree
            assert torch.allclose(base[c], R.census_expect(want[h, r:r + 1], c, h)[0], rtol=0, atol=1e-15)
            assert R.census_close(base[c].to(BF), base[c]).all()        # a correctly rounded result passes ...
            assert not R.census_close(base[c] * (1 + 3 * R.CENSUS_TOL), base[c]).all()      # ... and one 3 x the tolerance off does not
        other = next(b for b in dropped if b % 64 != kept[0] % 64)
        walks = {
            "skipped": dict(blocks=kept[1:]),
            "doubled": dict(blocks=kept + [kept[-1]]),
            "dropped walked": dict(blocks=sorted(kept + [dropped[0]])),
            "values swapped": dict(blocks=kept, value_of={kept[0]: other, other: kept[0]}),
            "key skipped": dict(blocks=kept, skip_key=(kept[len(kept) // 2], 17)),
        }
        if H > 1:
            walks["other head's columns"] = dict(blocks=kept, value_head=1 - h)
        for what, kw in walks.items():
            assert any(_seen(base[c], R.census_walk(code=c, h=h, nb=nb, **kw)) for c in "ABC"), (name, h, r, what)


def test_probe_rows_name_kept_and_dropped_edges():
    case = R.table_case("b258")
    mask = case["want"][0]
    rows = R.probe_rows(mask, [0, 62, 63, 64, 128, 257])
    assert all(bool(mask[r, j // 64]) == kept for r, j, kept in rows)
    assert any(not kept for _, _, kept in rows) and any(j // 64 in (63, 64, 127, 128) for _, j, kept in rows if kept)
    assert {j % 64 for _, j, _ in rows} == {0, 63}
