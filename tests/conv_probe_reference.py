"""Integer-exact probes of the causal 3x3x3 convolution (include/k5.h: k5_conv3d_bf16, k5_conv3d_strided_bf16, k5_conv3d_bf16_stats).

Inputs are integers in [-6, 6], weights are sparse integers (at most 6 non-zeros of {+-1, +-2} per output channel, or more of +-1 only),
the bias is an integer in [-8, 8] and the residual an integer in [-40, 40]: every partial sum, in any order, is an integer of magnitude
below 256 and therefore exact in bf16 and in fp32, so the expected output is ONE bit pattern and the comparison is torch.equal.
Shared by tests/test_conv_probe_host.py (the reference against the oracle, and the power of the probes against mutated index rules)
and tests/test_gpu_conv_probes.py (the kernels)."""
from types import SimpleNamespace as NS

import torch

# the index rules a kernel could implement instead of the right one (int_ref(rule=...)); only the host test uses them
MUTATIONS = ("no_frame0", "zero_front_t", "zero_top", "zero_bottom", "zero_left", "zero_right", "swap_hw", "stride_phase", "clamp_far")


def out_grid(Ts, Hs, Ws, up=(1, 1), st=(1, 1)):
    """(To, Ho, Wo) as include/k5.h documents them: the folded nearest upsample repeats every frame but the first; a stride keeps
    every st-th position of the padded grid"""
    if st != (1, 1):
        return (Ts - 1) // st[0] + 1, (Hs - 1) // st[1] + 1, (Ws - 1) // st[1] + 1
    return (2 * Ts - 1 if up[0] == 2 else Ts), up[1] * Hs, up[1] * Ws


def make_case(Ts, Hs, Ws, Cin, Cout, seed, nnz=6, up=(1, 1), st=(1, 1)):
    """Seeded integer tensors: x [Ts][Hs][Ws][Cin] in [-6, 6]; per output channel nnz triples (tap, cin, val), val in {+-1, +-2}
    (+-1 only for nnz > 6, so that nnz * max|val| * 6 + 8 <= 80 either way); bias in [-8, 8]; resid [M][Cout] in [-40, 40].
    Taps and 64-channel slabs are dealt out from shuffled decks, so every tap and every slab carries a non-zero (asserted)."""
    assert up[0] in (1, 2) and up[1] in (1, 2) and st[0] in (1, 2) and st[1] in (1, 2) and (up == (1, 1) or st == (1, 1))
    assert Cin % 64 == 0 and 1 <= nnz <= 12
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-6, 7, (Ts, Hs, Ws, Cin), generator=g)
    n, slabs = Cout * nnz, Cin // 64

    def deck(size):
        return torch.cat([torch.randperm(size, generator=g) for _ in range(n // size + 1)])[:n]

    tap = deck(27).view(Cout, nnz)
    cin = (deck(slabs) * 64 + torch.randint(0, 64, (n,), generator=g)).view(Cout, nnz)
    mag = torch.randint(1, 3 if nnz <= 6 else 2, (Cout, nnz), generator=g)
    val = mag * (2 * torch.randint(0, 2, (Cout, nnz), generator=g) - 1)
    bias = torch.randint(-8, 9, (Cout,), generator=g)
    To, Ho, Wo = out_grid(Ts, Hs, Ws, up, st)
    M = To * Ho * Wo
    resid = torch.randint(-40, 41, (M, Cout), generator=g)
    assert tap.unique().numel() == 27, "a tap carries no weight: raise nnz"
    assert (cin // 64).unique().numel() == slabs, "a 64-channel slab carries no weight"
    assert int(val.abs().sum(1).max()) * 6 + 8 <= 80
    return NS(x=x, tap=tap, cin=cin, val=val, bias=bias, resid=resid, dims=(Ts, Hs, Ws), Cin=Cin, Cout=Cout, up=tuple(up), st=tuple(st),
              grid=(To, Ho, Wo), M=M, seed=seed)


def _axis(n_out, d, stride, pad, n_src, upf, time, rule, lo_rule, hi_rule):
    """source index and validity of output positions 0..n_out-1 along one axis for tap offset d: o * stride + d - pad, clamped to the
    virtually upsampled extent, then mapped to the source (H / W: // 2; T: 0 -> 0, else 1 + (t - 1) // 2)"""
    ext = (2 * n_src - 1 if upf == 2 else n_src) if time else upf * n_src
    u = torch.arange(n_out) * stride + d - pad
    if rule == "stride_phase" and stride > 1:
        u = u + 1
    ok = torch.ones(n_out, dtype=torch.bool)
    if rule == lo_rule:
        ok &= u >= 0
    if rule == hi_rule:
        ok &= u <= ext - 1
    hi = ext - 1
    if rule == "clamp_far" and not time:
        hi = max(ext - 1 - upf, 0)            # one source position short
    u = u.clamp(0, hi)
    if upf == 2:
        if time:
            u = u // 2 if rule == "no_frame0" else torch.where(u == 0, u, 1 + (u - 1) // 2)
        else:
            u = u // 2
    return u, ok


def source_index(case, tap, rule=None):
    """flat source position [M] (into x viewed [Ts*Hs*Ws][Cin]) that output position m reads for `tap`, and whether it counts at all
    (always, under the true rule: replicate padding has no zeros)"""
    Ts, Hs, Ws = case.dims
    To, Ho, Wo = case.grid
    dt, dh, dw = tap // 9, (tap // 3) % 3, tap % 3
    if rule == "swap_hw":
        dh, dw = dw, dh
    t, okt = _axis(To, dt, case.st[0], 2, Ts, case.up[0], True, rule, "zero_front_t", None)
    h, okh = _axis(Ho, dh, case.st[1], 1, Hs, case.up[1], False, rule, "zero_top", "zero_bottom")
    w, okw = _axis(Wo, dw, case.st[1], 1, Ws, case.up[1], False, rule, "zero_left", "zero_right")
    idx = ((t[:, None, None] * Hs + h[None, :, None]) * Ws + w[None, None, :]).reshape(-1)
    ok = (okt[:, None, None] & okh[None, :, None] & okw[None, None, :]).reshape(-1)
    return idx, ok


def applicable(case, rule):
    """can `rule` change anything on this case's geometry at all?  (the host test lists the cases where it cannot)"""
    Ts, Hs, Ws = case.dims
    _, Ho, Wo = case.grid
    if rule == "no_frame0":
        return case.up[0] == 2 and Ts > 1            # one frame: every tap reads frame 0 under both rules
    if rule == "zero_front_t":
        return True
    if rule in ("zero_top", "zero_left"):
        return True
    if rule == "zero_bottom":                        # an even extent under stride 2 never reaches past the far side
        return (Ho - 1) * case.st[1] + 1 > case.up[1] * Hs - 1
    if rule == "zero_right":
        return (Wo - 1) * case.st[1] + 1 > case.up[1] * Ws - 1
    if rule == "swap_hw":
        return Hs > 1 or Ws > 1                      # a single pixel per frame: dh and dw read the same one
    if rule == "stride_phase":
        return (case.st[0] == 2 and Ts > 1) or (case.st[1] == 2 and (Hs > 1 or Ws > 1))
    if rule == "clamp_far":
        return Hs > 1 or Ws > 1
    raise ValueError(rule)


def int_ref(case, resid=False, rule=None, rows=None):
    """expected output [M][Cout] (or its `rows`) in int64 by index gather, bias added, residual on request.  Asserts the exactness
    conditions: |conv + bias| <= 80 and |out| <= 256."""
    Cin, Cout = case.Cin, case.Cout
    xT = case.x.reshape(-1, Cin).t().contiguous()                 # [Cin][positions]
    n_rows = case.M if rows is None else rows.numel()
    outT = torch.zeros(Cout, n_rows, dtype=torch.int64)
    chan = torch.arange(Cout)[:, None].expand_as(case.tap)
    for tap in range(27):
        sel = case.tap == tap
        if not sel.any():
            continue
        idx, ok = source_index(case, tap, rule)
        if rows is not None:
            idx, ok = idx[rows], ok[rows]
        g = xT[case.cin[sel]][:, idx] * case.val[sel][:, None]    # [entries of this tap][rows]
        if not ok.all():
            g = g * ok[None, :]
        outT.index_add_(0, chan[sel], g)
    out = outT.t().contiguous() + case.bias[None, :]
    if rule is None:
        assert int(out.abs().max()) <= 80, int(out.abs().max())
    if resid:
        out = out + (case.resid if rows is None else case.resid[rows])
    if rule is None:
        assert int(out.abs().max()) <= 256
    return out


def pack_weights(case):
    """dense [Cout][27 * Cin] bf16, tap order (dt * 3 + dh) * 3 + dw (two triples on one element add up, as they do in int_ref)"""
    w = torch.zeros(case.Cout, 27 * case.Cin, dtype=torch.int64)
    chan = torch.arange(case.Cout)[:, None].expand_as(case.tap)
    w.index_put_((chan.reshape(-1), (case.tap * case.Cin + case.cin).reshape(-1)), case.val.reshape(-1), accumulate=True)
    assert int(w.abs().max()) <= 256
    return w.to(torch.bfloat16)


def block_stats_ref(out_int, M, Cout, patch_grid=None):
    """[2 ceil(M / 256)][Cout / 4][2] fp32 = (sum, sum of squares) of the stored outputs per statistics block and channel quad, as
    include/k5.h lays out quad_stats.  Block b holds rows 128 b .. 128 b + 127; with patch_grid = (To, Ho, Wo) (output frames of whole
    8 x 32 patches) 256-row tile j is patch j of the frame-major, row-major patch order and its two blocks are the patch's upper and
    lower four pixel rows.  Rows past M count nothing.  Every value is below 2^24: exact in fp32 in any order (asserted)."""
    assert out_int.shape == (M, Cout) and Cout % 4 == 0
    tiles = (M + 255) // 256
    o = out_int.to(torch.int64)
    if patch_grid is not None:
        To, Ho, Wo = patch_grid
        assert To * Ho * Wo == M and Ho % 8 == 0 and Wo % 32 == 0
        o = o.view(To, Ho // 8, 8, Wo // 32, 32, Cout).permute(0, 1, 3, 2, 4, 5).reshape(M, Cout)
    o = torch.cat([o, torch.zeros(tiles * 256 - M, Cout, dtype=torch.int64)]).view(2 * tiles, 128, Cout // 4, 4)
    st = torch.stack([o.sum((1, 3)), (o * o).sum((1, 3))], -1)
    assert int(o.abs().sum((1, 3)).max()) < 2 ** 24 and int(st.max()) < 2 ** 24
    return st.float()


def explain(got, want, case):
    """names the first mismatching (t, h, w, c), the taps and input channels that feed channel c, and the border classes of the pixel"""
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    if not bad.any():
        return "no mismatch"
    To, Ho, Wo = case.grid
    m, c = [int(v) for v in bad.nonzero()[0]]
    t, h, w = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
    cls = []
    if t == 0:
        cls.append("first frame")
    for name, v, n in (("row", h, Ho), ("column", w, Wo)):
        if v == 0:
            cls.append("first " + name)
        if v == n - 1:
            cls.append("last " + name)
    if h % 8 in (0, 7) or w % 32 in (0, 31):
        cls.append("patch seam")
    if m >= (case.M - 1) // 256 * 256:
        cls.append("last 256-row tile")
    feeds = []
    if c < case.Cout:
        feeds = [f"tap {int(tp)} (dt {int(tp) // 9}, dh {int(tp) // 3 % 3}, dw {int(tp) % 3}) cin {int(ci)} x {int(v)}"
                 for tp, ci, v in zip(case.tap[c], case.cin[c], case.val[c])]
    rows = int(bad.any(1).sum())
    return (f"{int(bad.sum())} mismatches in {rows} of {case.M} rows; first at m={m} (t={t}, h={h}, w={w}) c={c}: got {float(got[m, c])}, "
            f"want {float(want[m, c])}; classes: {', '.join(cls) or 'interior'}; channel {c} is fed by: {'; '.join(feeds)} "
            f"[dims {case.dims} up {case.up} stride {case.st} {case.Cin}->{case.Cout} seed {case.seed}]")
