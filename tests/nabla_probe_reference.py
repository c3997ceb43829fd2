"""Designed block maps for the NABLA path (csrc/nabla.hip, the SPARSE list walk of csrc/attn_fwd.hip) — CPU only.

A block map cannot be written into the workspace through the C ABI, but it can be FORCED through the real select kernel:

  block means   key block j gets a colour c(j) in [0, 64) and the mean ka_j = a e_c(j); query block i gets a set of hot colours C_i and
                the mean qa_i = a sum_{c in C_i} e_c.  With a = 16 the block logit qa.ka / 8 is 32 on the hot set S_i = {j : c(j) in C_i}
                and 0 elsewhere; every mean, dot product and bf16 logit is exact in any summation order.
  probabilities the cold entries together carry ~ 1e-11 of the row, every hot entry exactly 1 / |S_i|.
  the cut       for any P with  cold mass + margin < 1 - P < 1 / |S_i| - margin  every cold entry is dropped and the FIRST hot entry of the
                ascending order already crosses the cut: the map is S_i | STA whatever the order among ties and whatever the fp32
                summation order.
  warm level    a = 12 on the query side (logit 24): mass the bisection has to drop, allowed while it stays a margin below 1 - P.
  deep level    a = 32 on both sides (logit 128): the cold entries' fp32 exp is exactly 0 — the "smallest positive value" bracket.
  tie rows      NOT of that kind, and marked so: a hot tie group that straddles the cut (|S_i| entries of 1 / |S_i|, the cut a margin
                away from every multiple of it).  nabla.hip ranks entries equal to the cut value by index like a STABLE ascending
                sort, so the expected map keeps the highest indices of the group; `want` comes from that rule (stable_cut).  These rows
                are what makes a wrong tie rank visible — on an admissible row every order among ties gives the same map.

`margin` measures, on the float64 softmax of the exact logits, how far every entry's cumulative mass lies from the cut; a table row is
ADMISSIBLE iff that is >= 1e-3 (100 x the 1e-5 tests/test_gpu_nabla.py grants fp32 exp / cumsum order on exact logits) and no tie group
has members on both sides of the cut (the span of a group = the cumulative masses of its members, first to last: a group whose first
member already crosses is kept whole in any order).

The census codes turn the list walk of the sparse attention into integer counts: with Q = 0 every score is equal, the value rows are
one-hot, and row i of query block r must give n_d / kept_r — n_d of the kept blocks carry digit d.  The kernel's partial sums are integers
< 2^24 (exact in fp32 in any order); the only roundings are the final division and the bf16 store: |got - want| <= 2^-8 want, and
got == 0 exactly where want == 0."""
import functools
import math

import torch

from oracle import k5_oracle as O

HOT, WARM, DEEP = 16.0, 12.0, 32.0
MARGIN = 1e-3
CENSUS_TOL = 2.0 ** -8
HEAD_SHIFT = 29                      # head h's census digits are rotated by 29 h: another head's columns are another code

COLOURINGS = {
    "bit": lambda j, h: j % 64,                                  # one bit in every word
    "word": lambda j, h: (j // 64) % 64,                         # whole words
    "affine": lambda j, h: (37 * j + h) % 64,
    "quad": lambda j, h: (j // 4) % 64,
    "half": lambda j, h: torch.clamp(j // 32, max=63),           # half words; beyond 2016 blocks the last colour takes the rest and is never hot
}


def colours(nb, H, colouring):
    j = torch.arange(nb)
    return torch.stack([COLOURINGS[colouring](j, h) for h in range(H)])                  # (H, nb)


def _sets(nb, H, col, hot_sets, nwarm):
    """hot / warm colour sets per (head, query block) as (H, nb, 64) bool.  hot_sets = (kmin, kmax): block i of head h is hot on
    kmin + (i + h) % (kmax - kmin + 1) colours, consecutive in the list of the head's usable colours (those that <= 64 key blocks carry)
    from position (7 i + 13 h); the nwarm colours that follow are warm."""
    kmin, kmax = hot_sets
    hot, warm = torch.zeros(H, nb, 64, dtype=torch.bool), torch.zeros(H, nb, 64, dtype=torch.bool)
    i = torch.arange(nb)
    for h in range(H):
        cnt = torch.bincount(col[h], minlength=64)
        usable = ((cnt > 0) & (cnt <= 64)).nonzero().flatten()
        nu = len(usable)
        assert kmax + nwarm <= nu, (kmax, nwarm, nu)
        k = kmin + (i + h) % (kmax - kmin + 1)
        base = 7 * i + 13 * h
        for t in range(kmax + nwarm):
            c = usable[(base + t) % nu]
            is_hot, is_warm = t < k, (t >= k) & (t < k + nwarm)
            hot[h, i[is_hot], c[is_hot]] = True
            warm[h, i[is_warm], c[is_warm]] = True
    return hot, warm


def tokens(means, layout):
    """(H, nb, 64) block means -> (nb * 64, H, 64) tokens.  "flat": every token of a block equals the mean; "spike": the token at position
    (7 b + h) % 64 of block b carries 64 x the mean and the rest are 0 (64 x 12, 16, 32 are bf16-exact): the mean is still exact, and
    depends on reading exactly the block's own 64 rows."""
    H, nb, _ = means.shape
    m = means.permute(1, 0, 2)                                                          # (nb, H, 64)
    if layout == "flat":
        return m[:, None].expand(nb, 64, H, 64).reshape(nb * 64, H, 64).contiguous()
    assert layout == "spike", layout
    tok = torch.zeros(nb, 64, H, 64)
    b, h = torch.arange(nb)[:, None], torch.arange(H)[None, :]
    tok[b, (7 * b + h) % 64, h] = 64.0 * m
    return tok.reshape(nb * 64, H, 64)


def stable_cut(p, thr):
    """the reference's rule `cvals >= 1 - thr` on an ascending sort that is STABLE (equal values in index order): (.., nb) bool"""
    vals, inds = p.sort(dim=-1, stable=True)
    keep = torch.zeros_like(vals, dtype=torch.bool)
    keep.scatter_(-1, inds, vals.cumsum(-1) >= thr)
    return keep


def map_case(grid, window, P, H, colouring, hot_sets, levels, token_layout, ties=False):
    """levels: "two" | ("three", nwarm) | "deep".  Returns a dict: q / k tokens (N, H, 64) fp32 with bf16-exact values, the designed sets
    S (H, nb, nb), the exact logits (float64), sta and want = S | sta — for P = 1 all ones (the reference keeps every block: cvals >= 0),
    for a tie row stable_cut of the exact probabilities | sta."""
    T, Hb, Wb = grid
    nb = T * Hb * Wb
    nwarm = levels[1] if isinstance(levels, tuple) else 0
    a = DEEP if levels == "deep" else HOT
    col = colours(nb, H, colouring)
    hot, warm = _sets(nb, H, col, hot_sets, nwarm)
    ka = a * torch.nn.functional.one_hot(col, 64).float()                               # (H, nb, 64)
    qa = a * hot.float() + WARM * warm.float()
    idx = col[:, None, :].expand(H, nb, nb)
    S, W = hot.gather(2, idx), warm.gather(2, idx)                                      # [h, i, j] = set_i has c(j)
    logits = (a * a / 8.0) * S.double() + (WARM * a / 8.0) * W.double()
    sta = O.fast_sta(T, Hb, Wb, *window)
    if P >= 1.0:
        want = torch.ones(H, nb, nb, dtype=torch.bool)
    elif ties:
        want = stable_cut(torch.softmax(logits, -1), 1.0 - P) | sta[None]
    else:
        want = S | sta[None]
    return dict(grid=grid, window=window, P=P, H=H, nb=nb, N=nb * 64, q=tokens(qa, token_layout), k=tokens(ka, token_layout), S=S, W=W,
                logits=logits, sta=sta, want=want, ties=ties)


def margin(case):
    """(min over entries of |cdf - (1 - P)|, whether a tie group has members on both sides of the cut within that margin, the smallest
    warm mass of a row) on the float64 softmax of the exact logits"""
    thr = 1.0 - case["P"]
    p = torch.softmax(case["logits"], -1)
    vals, _ = p.sort(-1)
    cs = vals.cumsum(-1)
    m = (cs - thr).abs().min().item()
    new = torch.ones_like(vals, dtype=torch.bool)
    new[..., 1:] = vals[..., 1:] != vals[..., :-1]
    gid = new.long().cumsum(-1) - 1
    first = torch.full_like(vals, float("inf")).scatter_reduce(-1, gid, cs, "amin", include_self=True)
    last = torch.full_like(vals, float("-inf")).scatter_reduce(-1, gid, cs, "amax", include_self=True)
    cnt = torch.zeros_like(vals).scatter_add(-1, gid, torch.ones_like(vals))
    straddle = bool(((cnt > 1) & (first <= thr + MARGIN) & (last >= thr - MARGIN)).any())
    warm_mass = (p * case["W"]).sum(-1).min().item() if case["W"].any() else 0.0
    return m, straddle, warm_mass


def admissible(case):
    m, straddle, _ = margin(case)
    return m >= MARGIN and not straddle


# ---------------------------------------------------------------------------------------------------------------- the case table
# name: (grid, window, P, H, colouring, hot_sets, levels, ties).  NV = values per lane of the nabla_select_row_kernel instantiation.
# P = 1 rows: the expected map is all ones (the reference's rule), admissibility does not apply.  Tie rows: see the module docstring.
MAP_ROWS = {
    # row lengths: one or more per instantiation, and the word edges
    "b64": ((16, 2, 2), (3, 3, 3), 0.9, 2, "bit", (1, 8), "two", False),               # NV 4, one full word
    "b65": ((13, 5, 1), (3, 3, 1), 0.9, 2, "affine", (1, 6), "two", False),            # NV 4, a last word with one valid bit; Wb = 1, Hb > 1
    "b130": ((13, 5, 2), (3, 3, 3), 0.95, 2, "quad", (1, 4), "two", False),            # NV 4; rect and census case; Hb Wb = 10
    "b258": ((43, 3, 2), (3, 3, 3), 0.99, 2, "bit", (1, 12), "two", False),            # NV 8; rect and census case; Hb Wb = 6
    "b512": ((8, 8, 8), (3, 3, 3), 0.99, 2, "quad", (1, 2), "two", False),             # NV 8 with a full last word
    "b513": ((19, 9, 3), (5, 3, 3), 0.99, 2, "word", (1, 1), "two", False),            # NV 16; Wb = 3
    "b1025": ((41, 5, 5), (3, 3, 3), 0.99, 1, "affine", (1, 5), "two", False),         # NV 24
    "b1537": ((53, 29, 1), (3, 5, 1), 0.99, 1, "quad", (1, 3), "two", False),          # NV 32
    "b2050": ((41, 10, 5), (3, 3, 3), 0.99, 1, "bit", (1, 2), "two", False),           # NV 48; census case
    "b3075": ((41, 15, 5), (3, 3, 3), 0.99, 1, "word", (1, 1), "two", False),          # NV 64
    "b4096": ((64, 8, 8), (3, 3, 3), 0.99, 1, "half", (1, 2), "two", False),           # NV 64, SEL_MAXNB, every word full; census case
    # STA geometry at 65-258 blocks
    "sta_line": ((65, 1, 1), (5, 1, 1), 0.9, 2, "bit", (1, 7), "two", False),          # Hb Wb = 1 (no division at all)
    "sta_w3": ((7, 3, 5), (3, 3, 3), 0.9, 2, "affine", (1, 4), "two", False),          # 105 blocks: Hb Wb = 15, Wb = 5, neither a power of two
    "sta_w6": ((11, 2, 6), (3, 3, 5), 0.95, 2, "quad", (1, 4), "two", False),          # 132 blocks: Hb Wb = 12, Wb = 6
    "sta_even": ((13, 5, 2), (4, 2, 2), 0.95, 2, "bit", (1, 6), "two", False),         # even windows: w / 2 truncates ((4,2,2) = (5,3,3) - 1)
    "sta_one": ((43, 3, 2), (1, 1, 1), 0.99, 2, "word", (1, 1), "two", False),         # window 1: the diagonal
    "sta_wide": ((33, 2, 2), (3, 5, 5), 0.95, 2, "affine", (1, 5), "two", False),      # a window larger than the grid in h and w
    # levels
    "warm130": ((13, 5, 2), (3, 3, 3), 0.9, 2, "bit", (1, 2), ("three", 50), False),   # three levels: the warm mass is dropped
    "warm258": ((43, 3, 2), (3, 3, 3), 0.95, 2, "bit", (1, 2), ("three", 50), False),
    "deep130": ((13, 5, 2), (3, 3, 3), 0.95, 2, "affine", (1, 5), "deep", False),       # the cold entries' exp is exactly 0
    "deep513": ((19, 9, 3), (3, 3, 3), 0.99, 2, "bit", (1, 4), "deep", False),
    # P = 1: everything is kept
    "p1_two": ((13, 5, 2), (3, 3, 3), 1.0, 2, "bit", (1, 3), "two", False),
    "p1_deep": ((43, 3, 2), (3, 3, 3), 1.0, 2, "affine", (1, 5), "deep", False),        # entries that underflowed to 0 are kept too
    # ties at the cut, ranked by index
    "tie65": ((13, 5, 1), (1, 1, 1), 0.7, 2, "bit", (4, 8), "two", True),              # 4-9 ties of one word (+ the 65th block)
    "tie258": ((43, 3, 2), (3, 3, 3), 0.65, 2, "quad", (1, 2), "two", True),            # 4-10 ties in runs of 4 across the word edges (P = 0.65: no multiple of 1/4 .. 1/10 near 0.35)
}
SMALL_ROWS = [n for n, r in MAP_ROWS.items() if r[0][0] * r[0][1] * r[0][2] <= 258]
ATTN_ROWS = ["b130", "b258", "b2050", "b4096"]                                          # the census / list-walk table
RECT_ROWS = ["b130", "b258"]


def rects(nb):
    """(q_block0, nqb): nqb not a multiple of 4 or 16, rows across the word edge, the last rows, the second head's row stride"""
    return [(0, 5), (61, 6), (nb - 3, 3), (17, 16), (64, 64)]


@functools.lru_cache(maxsize=4)
def table_case(name, layout="flat"):
    grid, window, P, H, colouring, hot_sets, levels, ties = MAP_ROWS[name]
    return map_case(grid, window, P, H, colouring, hot_sets, levels, layout, ties)


# ---------------------------------------------------------------------------------------------- CPU model of the select kernel
MUTATIONS = ["tie_low", "rank_gt", "sta_lt", "div_hb", "word63", "padding", "local_i"]


def select_model(case, q_block0=0, nqb=None, mutation=None):
    """nabla_select_row_kernel + the bitmap layout on the exact logits, in float64: (H, nqb, nw * 64) bool — the row's bitmap words, the
    padding bits of the last word included (they must be 0: the union kernel lists every set bit as a key block).
    mutation: one of MUTATIONS, a wrong kernel."""
    T, Hb, Wb = case["grid"]
    wT, wH, wW = case["window"]
    H, nb = case["H"], case["nb"]
    nqb = nb - q_block0 if nqb is None else nqb
    nw = (nb + 63) // 64
    target = 1.0 - case["P"]
    out = torch.zeros(H, nqb, nw * 64, dtype=torch.bool)
    j = torch.arange(nb)
    tj, hj_ok, hj_bad = j // (Hb * Wb), (j % (Hb * Wb)) // Wb, (j % (Hb * Wb)) // Hb
    hj = hj_bad if mutation == "div_hb" else hj_ok
    wj = j % (Hb * Wb) - hj * Wb
    near = (lambda d, w: d.abs() < w // 2) if mutation == "sta_lt" else (lambda d, w: d.abs() <= w // 2)
    p_all = torch.softmax(case["logits"], -1)
    for h in range(H):
        for il in range(nqb):
            i = il if mutation == "local_i" else q_block0 + il
            p = p_all[h, q_block0 + il]
            if target <= 0.0:
                keep = torch.ones(nb, dtype=torch.bool)                                # the reference's rule: cvals >= 0 keeps everything
            else:
                vals = p.sort().values
                cs = vals.cumsum(0)
                at = int((cs >= target).nonzero()[0]) if (cs >= target).any() else None
                if at is None:
                    keep = torch.zeros(nb, dtype=torch.bool)
                else:
                    vstar = vals[at]
                    base = p[p < vstar].sum()
                    m0 = max(1, math.ceil(float((target - base) / vstar) - 1e-9))
                    tie = p == vstar
                    rank = tie.long().cumsum(0)                                        # 1.. in index order
                    if mutation == "tie_low":
                        rank = int(tie.sum()) + 1 - rank
                    keep = (p > vstar) | (tie & ((rank > m0) if mutation == "rank_gt" else (rank >= m0)))
            ti, hi, wi = i // (Hb * Wb), (i // Wb) % Hb, i % Wb
            keep = keep | (near(tj - ti, wT) & near(hj - hi, wH) & near(wj - wi, wW))
            row = out[h, il]
            row[:nb] = keep
            if mutation == "word63":                                                   # bit 63 of word c lands in word c + 1
                b63 = j[(j % 64 == 63)]
                vals63 = row[b63].clone()
                row[b63] = False
                ok = b63 + 64 < nw * 64
                row[b63[ok] + 64] |= vals63[ok]
            if mutation == "padding":
                row[nb:] = True
    return out


def padded(want_rows, nb):
    """(H, rows, nb) -> (H, rows, nw * 64) with clear padding bits: what select_model must give"""
    nw = (nb + 63) // 64
    out = torch.zeros(*want_rows.shape[:2], nw * 64, dtype=torch.bool)
    out[..., :nb] = want_rows
    return out


# ---------------------------------------------------------------------------------------------------------------- census codes
def census_digit(code, b, t, h):
    """digit of key t of key block b in head h's code (b, t: ints or tensors)"""
    d = {"A": b % 64, "B": b // 64, "C": t}[code]
    return (d + HEAD_SHIFT * h) % 64


def census_codes(N, H):
    """{"A" | "B" | "C": V (N, H, 64) bf16 one-hot}.  With j the key, b = j // 64 its block: A: V[j][d] = 1 iff b % 64 == d (the bit of the
    block in its bitmap word), B: iff b // 64 == d (the word), C: iff j % 64 == d (the key inside its tile) — head h's digits rotated by
    29 h, so that another head's columns are a different code."""
    j = torch.arange(N)
    out = {}
    for code in "ABC":
        v = torch.zeros(N, H, 64, dtype=torch.bfloat16)
        for h in range(H):
            v[j, h, census_digit(code, j // 64, j % 64, h)] = 1.0
        out[code] = v
    return out


def census_walk(blocks, code, h, nb, value_of=None, value_head=None, skip_key=None):
    """what a row that walks `blocks` (key-block ids, with multiplicity) must give on code `code`: (64,) float64.
    value_of: {block: block whose values it reads}; value_head: the head whose columns are read; skip_key = (block, t): that key is left out."""
    vh = h if value_head is None else value_head
    o = torch.zeros(64, dtype=torch.float64)
    total = 0
    for b in blocks:
        vb = b if value_of is None else value_of.get(b, b)
        for_keys = [t for t in range(64) if skip_key != (b, t)] if code == "C" or (skip_key and skip_key[0] == b) else None
        if for_keys is None:
            o[census_digit(code, vb, 0, vh)] += 64
            total += 64
        else:
            for t in for_keys:
                o[census_digit(code, vb, t, vh)] += 1
            total += len(for_keys)
    return o / total


def census_expect(mask_rows, code, h):
    """mask_rows (rows, nb) bool of head h -> (rows, 64) float64: n_d / kept for A and B, 1 / 64 for C"""
    rows, nb = mask_rows.shape
    kept = mask_rows.sum(-1, keepdim=True).double()
    if code == "C":
        return torch.full((rows, 64), 1.0 / 64.0, dtype=torch.float64)
    digit = census_digit(code, torch.arange(nb), 0, h)
    n = mask_rows.double() @ torch.nn.functional.one_hot(digit, 64).double()
    return n / kept


def census_close(got, want):
    """elementwise bool: |got - want| <= 2^-8 want and got == 0 exactly where want == 0"""
    got, want = got.double(), want.double()
    return ((got - want).abs() <= CENSUS_TOL * want) & ((want != 0) | (got == 0))


# ---------------------------------------------------------------------------------------------------------------- key probes
def probe_rows(mask_h, qblocks):
    """mask_h (nb, nb) bool of one head.  For each query block: target keys (qblock, key, kept) at the first and last key of its first
    kept block, its last kept block, a kept block at a word edge (63 / 64 / 127 / 128 where kept) and a dropped block adjacent to a kept one."""
    nb = mask_h.shape[1]
    out = []
    for r in qblocks:
        kept = mask_h[r].nonzero().flatten().tolist()
        blocks = [(kept[0], True), (kept[-1], True)]
        edge = [b for b in (63, 64, 127, 128) if b < nb and mask_h[r, b] and b not in (kept[0], kept[-1])]
        if edge:
            blocks.append((edge[(r // 4) % len(edge)], True))
        dropped = [b for b in range(nb) if not mask_h[r, b] and ((b > 0 and mask_h[r, b - 1]) or (b + 1 < nb and mask_h[r, b + 1]))]
        if dropped:
            blocks.append((dropped[(r // 4) % len(dropped)], False))
        for b, k in blocks:
            out += [(r, 64 * b, k), (r, 64 * b + 63, k)]
    return out
