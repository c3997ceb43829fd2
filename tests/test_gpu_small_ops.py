"""GPU parity tests (MI355X) of the DiT's elementwise and normalisation kernels (csrc/small_ops.hip) through the public C ABI, at the sizes
where their index arithmetic works hardest: past the first trip of every grid-stride loop, under the block cap of the norm kernel, on
strided views, with token permutations, and on edge rows.  bf16 outputs are compared with the CPU oracle (oracle/k5_oracle.py,
bf16-island arithmetic) under the tolerances of tests/test_gpu_kernels.py; the ops that only move values, the guard regions and the
integer GEMV are compared bit for bit with tests/small_ops_reference.py.  tests/test_small_ops_host.py imports the case tables below and
proves on the CPU that each case reaches the path it claims and tells the true index rule from every mutated one.

Every output buffer has guard rows before and after (and guard columns where there is a row stride), filled with a NaN bit pattern
that must come back untouched."""
import itertools

from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

from kit import BF, E  # noqa: E402

import small_ops_reference as R  # noqa: E402

from oracle import k5_oracle as O  # noqa: E402

OK, ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = 0, 1, 2, 6

# ------------------------------------------------------------------------------------------ case tables (shared with the host file)
GATE_CASES = [(1, 8), (77, 264), (9400, 1792)]                       # the last: 2 105 600 chunks, just past one trip of 2 097 152
LN_CASES = [(rows, D) for D in (8, 520, 1792, 2048) for rows in (1, 9, 301)]
# (rows, H, heads_per_weight, rope_heads, tables given)
NORM_CASES = [(2401, 56, 28, 56, True), (4700, 28, 28, 28, True), (26500, 5, 2, 3, True), (70, 5, 2, 0, True), (150, 6, 6, 6, False)]
NORM_TRIP_CASES = NORM_CASES[:3]                                      # the block cap binds: a second trip
STATS_CASE, STATS_SCALE_FROM = (2401, 56, 28, 56, True), 28
GEMV_INT_CASES = [(1, 4), (5, 260), (10753, 1792)]
GEMV_SILU_CASES = [(5, 260), (1027, 1792)]
TIME_D, TIME_T = (2, 64, 1792), (0.0, 1e-3, 1.0, 731.25, 1000.0)
# (T, H, W) of the token grid, permutation, axis widths, scales
ROPE_CASES = [(g, p, a, s, 6000 + i) for i, ((g, p), a, s) in enumerate(itertools.product(
    [((6, 16, 16), "fractal"), ((3, 4, 6), "random")], [(8, 12, 12), (4, 14, 14)], [(1.0, 2.0, 2.0), (1.5, 1.0, 3.0)]))]
# (T, H, W, x channels, Cin, Kpad, permutation, conditioning given)
PATCH_CASES = [(2, 4, 6, 16, 33, 136, None, False), (6, 32, 32, 16, 33, 136, "fractal", False), (3, 8, 12, 16, 33, 144, "random", False),
               (2, 4, 6, 16, 33, 144, None, True), (6, 32, 32, 16, 33, 136, "fractal", True), (3, 8, 12, 16, 33, 136, "random", True),
               # 16 384 tokens x 136: past one trip (the 8 x 8 block order of a 64 x 64 token grid is its own inverse: a random order instead)
               (4, 128, 128, 16, 33, 136, "random", False), (4, 128, 128, 16, 33, 136, "random", True)]
PATCH_TRIP_CASES = PATCH_CASES[-2:]
# (T, Hp, Wp, C, ldx, permutation)
UNPATCH_CASES = [(2, 2, 3, 16, 64, None), (2, 2, 3, 16, 72, None), (6, 16, 16, 16, 72, "fractal"), (3, 4, 6, 16, 64, "random"),
                 (3, 4, 6, 16, 72, "random"), (9, 64, 64, 16, 72, "random")]                                # 36 864 tokens x 64: past one trip
UNPATCH_TRIP_CASES = UNPATCH_CASES[-1:]


def ids(v):
    return str(v).replace(" ", "")


_cache = {}


def cached(fn, *key):
    """a case and its reference are built once and shared by the tests that use them (never modified)"""
    k = (fn.__name__,) + tuple(id(a) if isinstance(a, NS) else a for a in key)      # a case stands for itself: it is cached too
    if k not in _cache:
        _cache[k] = fn(*key)
    return _cache[k]


def dev(t, dtype=None):
    return None if t is None else (t.to(dtype) if dtype else t).cuda().contiguous()


def p(t):
    return None if t is None else t.data_ptr()


def bf16_out(rows, cols, ld=None):
    return R.guarded(rows, cols, BF, ld, device="cuda")


# ------------------------------------------------------------------------------------------ gate-sum
@pytest.mark.parametrize("rows,D", GATE_CASES, ids=ids)
def test_gate_sum_grid_stride(E, rows, D):
    c = cached(R.gate_case, rows, D)
    xd, yd, gd = dev(c.x, BF), dev(c.y, BF), dev(c.gate)
    buf, out = bf16_out(rows, D)
    E.check(E.lib().k5_gate_sum_bf16(xd.data_ptr(), yd.data_ptr(), gd.data_ptr(), out.data_ptr(), rows, D, E.stream_ptr()), "k5_gate_sum_bf16")
    torch.cuda.synchronize()
    R.assert_bf16_close(out, O.gate_sum(c.x, c.y, c.gate, "bf16"), *R.TOL["gate"], what=f"gate_sum {rows}x{D}")
    assert R.guards_intact(buf, rows, D)


# ------------------------------------------------------------------------------------------ LayerNorm
def ln_oracle_modulate(rows, D):
    c = cached(R.ln_case, rows, D)
    return O.scale_shift_norm(c.x, c.scale[None], c.shift[None], "bf16")


def ln_oracle_affine(rows, D):
    c = cached(R.ln_case, rows, D)
    return torch.nn.functional.layer_norm(c.x, (D,), c.w, c.b, eps=1e-5).to(BF).float()


@pytest.mark.parametrize("layout", ["contiguous", "strided"])
@pytest.mark.parametrize("rows,D", LN_CASES, ids=ids)
def test_ln_modulate_edges_and_strides(E, rows, D, layout):
    c = cached(R.ln_case, rows, D)
    ldx, ldo = (D, D) if layout == "contiguous" else (D + 8, D + 24)
    xbuf = torch.full((rows, ldx), float("nan"), dtype=BF, device="cuda")      # NaN in the gap columns of the input: never read
    xbuf[:, :D] = c.x.to(BF).cuda()
    sd, hd = dev(c.scale), dev(c.shift)
    buf, out = bf16_out(rows, D, ldo)
    E.check(E.lib().k5_ln_modulate_bf16(xbuf.data_ptr(), sd.data_ptr(), hd.data_ptr(), out.data_ptr(), rows, D, ldx, ldo, E.stream_ptr()),
            "k5_ln_modulate_bf16")
    torch.cuda.synchronize()
    R.assert_bf16_close(out, cached(ln_oracle_modulate, rows, D), *R.TOL["ln"], what=f"ln_modulate {rows}x{D} {layout}")
    assert R.guards_intact(buf, rows, D)


@pytest.mark.parametrize("rows,D", LN_CASES, ids=ids)
def test_ln_affine_edges(E, rows, D):
    c = cached(R.ln_case, rows, D)
    xd, wd, bd = dev(c.x, BF), dev(c.w), dev(c.b)
    buf, o16 = bf16_out(rows, D)
    buf32, o32 = R.guarded(rows, D, torch.float32, device="cuda")
    E.check(E.lib().k5_ln_affine_bf16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), o16.data_ptr(), o32.data_ptr(), rows, D, E.stream_ptr()),
            "k5_ln_affine_bf16")
    torch.cuda.synchronize()
    R.assert_bf16_close(o16, cached(ln_oracle_affine, rows, D), *R.TOL["ln"], what=f"ln_affine {rows}x{D}")
    assert torch.equal(o32.cpu(), o16.float().cpu())
    assert R.guards_intact(buf, rows, D) and R.guards_intact(buf32, rows, D)


def test_ln_width_limits(E):
    x = torch.zeros(2, 2064, dtype=BF, device="cuda")
    v = torch.zeros(2064, device="cuda")
    buf, out = bf16_out(2, 2064)
    L = E.lib()
    for D, want in ((2056, ERR_UNSUPPORTED), (12, ERR_ALIGN)):
        assert L.k5_ln_modulate_bf16(x.data_ptr(), v.data_ptr(), v.data_ptr(), out.data_ptr(), 2, D, 2064, 2064, E.stream_ptr()) == want
        assert E.last_error()
        assert L.k5_ln_affine_bf16(x.data_ptr(), v.data_ptr(), v.data_ptr(), out.data_ptr(), None, 2, D, E.stream_ptr()) == want
        assert E.last_error()
    torch.cuda.synchronize()
    assert R.guards_intact(buf, 0, 0)


# ------------------------------------------------------------------------------------------ RMSNorm + RoPE
def norm_oracle(case, out_scale=1.0, scale_from=None):
    """O.rms_norm_heads per weight group, O.apply_rotary on the heads < rope_heads (with out_scale on the heads >= scale_from), one more
    bf16 rounding of out_scale * n on the scaled heads that are not rotated"""
    c = cached(R.norm_case, *case)
    x = c.x.view(c.rows, c.H, 64)
    n = torch.cat([O.rms_norm_heads(x[:, g * c.hpw:(g + 1) * c.hpw], c.weight[g], "bf16") for g in range(c.G)], 1)
    sf = c.H if scale_from is None else scale_from
    out = n.clone()
    out[:, sf:] = (n[:, sf:] * torch.tensor(out_scale, dtype=torch.float32)).to(BF).float()
    nr = c.rope_heads if c.cos is not None else 0
    lo, hi = min(nr, sf), nr
    if lo > 0:
        out[:, :lo] = O.apply_rotary(n[:, :lo], c.cos, c.sin, "bf16")
    if hi > lo:
        out[:, lo:hi] = O.apply_rotary(n[:, lo:hi], c.cos, c.sin, "bf16", out_scale=out_scale)
    return out.reshape(c.rows, c.H * 64)


def norm_oracle_plain(*case):
    return norm_oracle(case)


def norm_oracle_scaled(*case):
    return norm_oracle(case, O.SOFTMAX_C, STATS_SCALE_FROM)


def norm_buffer(c, extra):
    """the rows as a view of a wider buffer: guard rows around, `extra` gap columns of NaN bits after the H heads"""
    ld = 64 * c.H + extra
    buf, view = bf16_out(c.rows, 64 * c.H, ld)
    view.copy_(c.x.to(BF).cuda())
    return buf, view, ld


@pytest.mark.parametrize("extra", [0, 64])
@pytest.mark.parametrize("case", NORM_CASES, ids=ids)
def test_rmsnorm_rope_block_cap_strides_and_groups(E, case, extra):
    c = cached(R.norm_case, *case)
    buf, x, ld = norm_buffer(c, extra)
    wd, cd, sd = dev(c.weight), dev(c.cos), dev(c.sin)
    E.check(E.lib().k5_rmsnorm_rope_bf16(x.data_ptr(), wd.data_ptr(), p(cd), p(sd), c.rows, c.H, ld, c.hpw, c.rope_heads, E.stream_ptr()),
            "k5_rmsnorm_rope_bf16")
    torch.cuda.synchronize()
    R.assert_bf16_close(x, cached(norm_oracle_plain, *case), *R.TOL["norm"], what=f"rmsnorm_rope {case} ld {ld}")   # finite, edge vectors included
    assert R.guards_intact(buf, c.rows, 64 * c.H)


def stats_inputs(c):
    buf, x, ld = norm_buffer(c, 64)
    return buf, x, ld, dev(c.weight), dev(c.cos), dev(c.sin)


def written_norms(x, rows, H):
    y = x.float().cpu().reshape(rows, H, 64)
    return y, (y * y).sum(-1).amax(0)


def test_rmsnorm_rope_stats_under_the_block_cap(E):
    c = cached(R.norm_case, *STATS_CASE)
    rows, H, sf = c.rows, c.H, STATS_SCALE_FROM
    buf, x, ld, wd, cd, sd = stats_inputs(c)
    stats = torch.zeros(H, device="cuda")
    stats[3] = 1e9                                                     # a larger value from before survives
    E.check(E.lib().k5_rmsnorm_rope_stats_bf16(x.data_ptr(), wd.data_ptr(), cd.data_ptr(), sd.data_ptr(), rows, H, ld, c.hpw, c.rope_heads,
                                               float(O.SOFTMAX_C), sf, stats.data_ptr(), E.stream_ptr()), "k5_rmsnorm_rope_stats_bf16")
    torch.cuda.synchronize()
    R.assert_bf16_close(x, cached(norm_oracle_scaled, *STATS_CASE), *R.TOL["norm"], what="rmsnorm_rope_stats values")
    assert R.guards_intact(buf, rows, 64 * H)
    _, n2 = written_norms(x, rows, H)
    n2[3] = 1e9
    assert torch.allclose(stats.cpu(), n2, rtol=1e-5), (stats, n2)


def test_rmsnorm_rope_stats_nan_marks_one_head(E):
    c = cached(R.norm_case, *STATS_CASE)
    rows, H = c.rows, c.H
    buf, x, ld, wd, cd, sd = stats_inputs(c)
    row, head = rows - 7, 41                                           # a row of the second trip
    x[row, head * 64 + 9] = float("nan")
    stats = torch.zeros(H, device="cuda")
    E.check(E.lib().k5_rmsnorm_rope_stats_bf16(x.data_ptr(), wd.data_ptr(), cd.data_ptr(), sd.data_ptr(), rows, H, ld, c.hpw, c.rope_heads,
                                               float(O.SOFTMAX_C), STATS_SCALE_FROM, stats.data_ptr(), E.stream_ptr()), "k5_rmsnorm_rope_stats_bf16")
    torch.cuda.synchronize()
    s = stats.cpu()
    others = torch.arange(H) != head
    assert s[head] == float("inf") and torch.isfinite(s[others]).all(), s
    y = x.float().cpu().reshape(rows, H, 64)
    keep = torch.ones(rows, H, dtype=torch.bool)
    keep[row, head] = False
    want = cached(norm_oracle_scaled, *STATS_CASE).reshape(rows, H, 64)
    R.assert_bf16_close(y[keep], want[keep], *R.TOL["norm"], what="every other head vector")
    assert torch.allclose(s[others], (y * y).sum(-1).amax(0)[others], rtol=1e-5)


def test_rmsnorm_rope_centre_under_the_block_cap(E):
    c = cached(R.norm_case, *STATS_CASE)
    rows, H, sf = c.rows, c.H, STATS_SCALE_FROM
    buf, x, ld, wd, cd, sd = stats_inputs(c)
    stats = torch.zeros(H + H - sf, device="cuda")
    centre = torch.full((H - sf, 64), float("nan"), device="cuda")
    E.check(E.lib().k5_rmsnorm_rope_centre_bf16(x.data_ptr(), wd.data_ptr(), cd.data_ptr(), sd.data_ptr(), rows, H, ld, c.hpw, c.rope_heads,
                                                float(O.SOFTMAX_C), sf, stats.data_ptr(), centre.data_ptr(), E.stream_ptr()),
            "k5_rmsnorm_rope_centre_bf16")
    torch.cuda.synchronize()
    R.assert_bf16_close(x, cached(norm_oracle_scaled, *STATS_CASE), *R.TOL["norm"], what="rmsnorm_rope_centre values")
    assert R.guards_intact(buf, rows, 64 * H)
    y, n2 = written_norms(x, rows, H)
    kp = y[:, sf:]
    idx = (torch.arange(256) * rows) // 256                            # K5_CENTRE_SAMPLE rows, spread over the sequence
    want_c = kp[idx].mean(0)
    assert (centre.cpu() - want_c).abs().max().item() <= 2e-3 * want_c.abs().max().item() + 1e-4
    r2 = ((kp - centre.cpu()[None]) ** 2).sum(-1).amax(0)
    assert torch.allclose(stats[:H].cpu(), n2, rtol=1e-5) and torch.allclose(stats[H:].cpu(), r2, rtol=1e-4), (stats, n2, r2)


# ------------------------------------------------------------------------------------------ fp32 GEMV
def run_gemv(E, x, W, b, add, silu):
    N, K = W.shape
    xd, Wd, bd, ad = dev(x.float()), dev(W.float()), dev(None if b is None else b.float()), dev(None if add is None else add.float())
    buf, y = R.guarded(1, N, torch.float32, N + 5, guard_rows=1, device="cuda")       # guard elements before and after y
    st = E.lib().k5_gemv_f32(xd.data_ptr(), Wd.data_ptr(), p(bd), y.data_ptr(), N, K, int(silu), p(ad), E.stream_ptr())
    torch.cuda.synchronize()
    assert R.guards_intact(buf, 1, N, guard_rows=1)
    return st, y.reshape(-1).cpu()


@pytest.mark.parametrize("has_b,has_add", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("N,K", GEMV_INT_CASES, ids=ids)
def test_gemv_integer_probes_are_exact(E, N, K, has_b, has_add):
    c = cached(R.gemv_int_case, N, K, has_b, has_add)
    st, y = run_gemv(E, c.x, c.W, c.b, c.add, False)
    E.check(st, "k5_gemv_f32")
    want, _ = R.gemv_ref(c.x, c.W, c.b, c.add)
    assert torch.equal(y.double(), want)


@pytest.mark.parametrize("N,K", GEMV_SILU_CASES, ids=ids)
def test_gemv_silu_within_the_summation_bound(E, N, K):
    c = cached(R.gemv_silu_case, N, K)
    st, y = run_gemv(E, c.x, c.W, c.b, c.add, True)
    E.check(st, "k5_gemv_f32")
    want, mag = R.gemv_ref(c.x, c.W, c.b, c.add, silu=True)
    err, tol = (y.double() - want).abs(), R.gemv_silu_tol(K, mag)
    assert torch.isfinite(y).all() and (err <= tol).all(), f"{int((err > tol).sum())} off, worst err / tol {float((err / tol).max()):.3g}"


def test_gemv_k_alignment(E):
    c = cached(R.gemv_int_case, 5, 260, 1, 1)
    st, _ = run_gemv(E, c.x[:6], c.W[:, :6].contiguous(), c.b, c.add, False)
    assert st == ERR_ALIGN and E.last_error()


# ------------------------------------------------------------------------------------------ sinusoids
@pytest.mark.parametrize("D", TIME_D)
def test_time_features(E, D):
    for t in TIME_T:
        buf, out = R.guarded(1, D, torch.float32, D + 3, guard_rows=1, device="cuda")
        E.check(E.lib().k5_time_features_f32(t, out.data_ptr(), D, E.stream_ptr()), "k5_time_features_f32")
        torch.cuda.synchronize()
        got = out.reshape(-1).cpu().double()
        assert torch.isfinite(got).all()
        for exact in (False, True):                  # the model's frequencies (fp32 exponent argument), and the mathematical ones
            a = R.time_angles(t, D, exact)
            want, tol = torch.cat([torch.cos(a), torch.sin(a)]), R.angle_tol(torch.cat([a, a]))
            assert ((got - want).abs() <= tol).all(), (D, t, exact, float(((got - want).abs() / tol).max()))
        assert R.guards_intact(buf, 1, D, guard_rows=1)


@pytest.mark.parametrize("case", ROPE_CASES, ids=ids)
def test_rope_table_permuted_positions(E, case):
    c = cached(R.rope_case, *case[0], *case[1:])
    n = c.T * c.H * c.W
    pos = [dev(v) for v in c.pos]
    perm = dev(c.perm)
    bc, cos = R.guarded(n, 32, torch.float32, device="cuda")
    bs, sin = R.guarded(n, 32, torch.float32, device="cuda")
    E.check(E.lib().k5_rope_table_f32(cos.data_ptr(), sin.data_ptr(), pos[0].data_ptr(), pos[1].data_ptr(), pos[2].data_ptr(), c.T, c.H, c.W,
                                      *c.axes, *c.scales, p(perm), E.stream_ptr()), "k5_rope_table_f32")
    torch.cuda.synchronize()
    for a in (cached(R.rope_angles_ref, c), R.rope_angles_ref(c, exact=True)):      # the model's frequencies, and the mathematical ones
        tol = R.angle_tol(a)
        for got, want, name in ((cos, torch.cos(a), "cos"), (sin, torch.sin(a), "sin")):
            got = got.cpu().double()
            assert torch.isfinite(got).all() and ((got - want).abs() <= tol).all(), (name, float(((got - want).abs() / tol).max()))
    assert R.guards_intact(bc, n, 32) and R.guards_intact(bs, n, 32)


# ------------------------------------------------------------------------------------------ patchify / unpatchify
@pytest.mark.parametrize("case", PATCH_CASES, ids=ids)
def test_patchify_is_the_gather(E, case):
    c = cached(R.patch_case, *case, 7000 + PATCH_CASES.index(case))
    n = c.T * (c.H // 2) * (c.W // 2)
    xd, vd, perm = dev(c.x), dev(c.vc), dev(c.perm)
    buf, out = bf16_out(n, c.Kpad)
    if c.vc is None:
        st = E.lib().k5_patchify_bf16(xd.data_ptr(), out.data_ptr(), c.T, c.H, c.W, c.Cx, c.Cin, c.Kpad, p(perm), E.stream_ptr())
    else:
        st = E.lib().k5_patchify_cond_bf16(xd.data_ptr(), vd.data_ptr(), out.data_ptr(), c.T, c.H, c.W, c.Cx, c.Cin, c.Kpad, p(perm), E.stream_ptr())
    E.check(st, "k5_patchify")
    torch.cuda.synchronize()
    assert R.same_bits(out.cpu(), cached(R.patchify_ref, c))           # pad columns zero included
    assert R.guards_intact(buf, n, c.Kpad)


@pytest.mark.parametrize("case", UNPATCH_CASES, ids=ids)
def test_unpatchify_is_the_scatter(E, case):
    c = cached(R.unpatch_case, *case, 8000 + UNPATCH_CASES.index(case))
    xd, perm = dev(c.x), dev(c.perm)
    rows, cols = c.T * 2 * c.Hp, 2 * c.Wp * c.C
    buf, out = bf16_out(rows, cols)
    E.check(E.lib().k5_unpatchify_bf16(xd.data_ptr(), out.data_ptr(), c.T, c.Hp, c.Wp, c.C, c.ldx, p(perm), E.stream_ptr()), "k5_unpatchify_bf16")
    torch.cuda.synchronize()
    assert R.same_bits(out.cpu().view(c.T, 2 * c.Hp, 2 * c.Wp, c.C), cached(R.unpatchify_ref, c))
    assert R.guards_intact(buf, rows, cols)


def test_permutations_are_the_projects(golden):
    """the "fractal" order of the cases above is the project's: O.fractal_perm and the golden vector of the reference's fractal_flatten"""
    assert torch.equal(R.make_perm("fractal", 6, 16, 16, None).long(), golden["fractal.perm.6x16x16"].long())
    assert torch.equal(R.make_perm("fractal", 3, 8, 24, None).long(), O.fractal_perm((3, 8, 24)))


# ------------------------------------------------------------------------------------------ refusals: status, message, nothing launched
def refusal_calls(E):
    """name -> (call, expected status).  Every other argument of a call is valid and points at real device memory."""
    L, s = E.lib(), E.stream_ptr()
    keep = NS_keep()
    H, rows = 4, 8
    x = keep(torch.zeros(rows, 64 * H + 64, dtype=BF, device="cuda"))
    w = keep(torch.ones(2, 64, device="cuda"))
    cs = keep(torch.ones(rows, 32, device="cuda"))
    f = keep(torch.zeros(4096, device="cuda"))
    o = keep(torch.zeros(4096, dtype=BF, device="cuda"))
    i32 = keep(torch.zeros(64, dtype=torch.int32, device="cuda"))
    X, Wt, CS, F, Ob, I = x.data_ptr(), w.data_ptr(), cs.data_ptr(), f.data_ptr(), o.data_ptr(), i32.data_ptr()

    def norm(x=X, w=Wt, c=CS, sn=CS, ld=64 * H, hpw=2, rh=H):
        return lambda: L.k5_rmsnorm_rope_bf16(x, w, c, sn, rows, H, ld, hpw, rh, s)

    def lnm(x=Ob, a=F, b=F, ldx=16, ldo=16):
        return lambda: L.k5_ln_modulate_bf16(x, a, b, X, 4, 16, ldx, ldo, s)

    def unp(x=Ob, out=X, T=1, Hp=2, Wp=2, C=2, ldx=8):
        return lambda: L.k5_unpatchify_bf16(x, out, T, Hp, Wp, C, ldx, None, s)

    def rope(c=F, sn=F, p0=I, T=1, Hh=2, W=2, n=(8, 12, 12)):
        return lambda: L.k5_rope_table_f32(c, sn, p0, I, I, T, Hh, W, *n, 1.0, 1.0, 1.0, None, s)

    def pat(x=F, out=Ob, T=1, Hh=2, W=2):
        return lambda: L.k5_patchify_bf16(x, out, T, Hh, W, 2, 3, 16, None, s)

    def gemv(x=F, Wm=F, y=F):
        return lambda: L.k5_gemv_f32(x, Wm, None, y, 2, 8, 0, None, s)

    calls = {
        "norm heads_per_weight 0": norm(hpw=0), "norm heads_per_weight -1": norm(hpw=-1), "norm rope_heads -1": norm(rh=-1),
        "norm null x": norm(x=None), "norm null weight": norm(w=None), "norm cos only": norm(sn=None), "norm sin only": norm(c=None),
        "norm ld < 64 H": norm(ld=64 * H - 8),
        "ln null x": lnm(x=None), "ln null scale": lnm(a=None), "ln null shift": lnm(b=None), "ln ldx < D": lnm(ldx=8), "ln ldo < D": lnm(ldo=8),
        "unpatchify T -1 Hp -2": unp(T=-1, Hp=-2), "unpatchify T 0": unp(T=0), "unpatchify Hp 0": unp(Hp=0), "unpatchify Wp -1": unp(Wp=-1),
        "unpatchify C 0": unp(C=0), "unpatchify null x": unp(x=None), "unpatchify null out": unp(out=None), "unpatchify ldx < 4 C": unp(ldx=4),
        "rope T -1 H -2": rope(T=-1, Hh=-2), "rope W 0": rope(W=0), "rope widths 31": rope(n=(8, 12, 11)), "rope width -4": rope(n=(-4, 18, 18)),
        "rope null cos": rope(c=None), "rope null sin": rope(sn=None), "rope null positions": rope(p0=None),
        "patchify T -1 H -2": pat(T=-1, Hh=-2), "patchify W 0": pat(W=0), "patchify null x": pat(x=None), "patchify null out": pat(out=None),
        "gemv null x": gemv(x=None), "gemv null W": gemv(Wm=None), "gemv null y": gemv(y=None),
    }
    return calls, keep


class NS_keep(list):
    """keeps the device tensors of the refusal calls alive"""
    def __call__(self, t):
        self.append(t)
        return t


REFUSALS = ["norm heads_per_weight 0", "norm heads_per_weight -1", "norm rope_heads -1", "norm null x", "norm null weight", "norm cos only",
            "norm sin only", "norm ld < 64 H", "ln null x", "ln null scale", "ln null shift", "ln ldx < D", "ln ldo < D",
            "unpatchify T -1 Hp -2", "unpatchify T 0", "unpatchify Hp 0", "unpatchify Wp -1", "unpatchify C 0", "unpatchify null x",
            "unpatchify null out", "unpatchify ldx < 4 C", "rope T -1 H -2", "rope W 0", "rope widths 31", "rope width -4", "rope null cos",
            "rope null sin", "rope null positions", "patchify T -1 H -2", "patchify W 0", "patchify null x", "patchify null out",
            "gemv null x", "gemv null W", "gemv null y"]


@pytest.mark.parametrize("name", REFUSALS, ids=lambda v: v.replace(" ", "_"))
def test_launchers_refuse_before_any_launch(E, name):
    calls, keep = refusal_calls(E)
    assert sorted(calls) == sorted(REFUSALS)
    assert calls[name]() == ERR_ARG
    assert E.last_error()
    torch.cuda.synchronize()
