"""Float64 references of the DiT's elementwise and normalisation kernels (csrc/small_ops.hip, public entries of include/k5.h), the seeded
inputs of their tests, and the index rules a kernel could implement instead of the right one.

Every reference is written from the definition of the operation (kandinsky/models/nn.py, as include/k5.h cites it) in float64, or as a pure
index gather for the ops that only move values; none restates a kernel.  Each takes `rule=`: None is the true rule, a name from MUTATIONS
a wrong one.  Shared by tests/test_small_ops_host.py (the references against the oracle, the reach of every case that claims a second
grid trip, and the power of every case against the mutated rules) and tests/test_gpu_small_ops.py (the kernels)."""
import math
from types import SimpleNamespace as NS

import torch

BF = torch.bfloat16
F64 = torch.float64

# launch geometry of small_ops.hip: grid_for() caps a grid-stride launch at 8192 blocks of 256 threads; the norm kernel at 4096 blocks
# rounded down to a multiple of `unit`, the number of blocks after which the grid stride is a whole number of rows (H * 8 threads each)
GRID_FOR_BLOCKS, THREADS, NORM_BLOCKS = 8192, 256, 4096
GRID_TRIP = GRID_FOR_BLOCKS * THREADS          # elements (or 16-byte chunks) one trip of a grid-stride loop covers

# tolerances of the bf16 outputs (tests/test_gpu_kernels.py: the same ops, the same figures)
TOL = {"ln": (1, 1e-4), "norm": (2, 1e-4), "gate": (1, 1e-5)}

MUTATIONS = {
    "gate": ("gate_no_modulo", "gate_wrong_width", "gate_trip_local"),
    "norm": ("group_mod", "group_ignored", "rope_le", "rope_all", "cs_row_lag", "cs_row_mod"),
    "patchify": ("feature_cphpw", "swap_hw", "perm_inverse"),
    "unpatchify": ("feature_phpwc", "swap_hw", "perm_inverse", "ldx_4c"),
    "rope_table": ("swap_hw", "perm_inverse", "axis_shift", "scale_1_on_2"),
}


def norm_trip_rows(H):
    """rows one trip of rmsnorm_rope_kernel covers under its block cap, and the cap: k5_launch_rmsnorm_rope"""
    unit = 8 * H // math.gcd(THREADS, 8 * H)
    cap = NORM_BLOCKS // unit * unit
    assert cap >= unit and (cap * THREADS) % (8 * H) == 0
    return cap * THREADS // (8 * H), cap


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bfr(x):
    return x.to(BF).float()


def r16(x):
    """bf16 rounding point of a float64 value (through fp32: the double rounding moves a value only when it sits within 2^-29 of a tie)"""
    return x.float().to(BF).to(F64)


def tol_of(op, ref):
    ulps, atol = TOL[op]
    return atol + ulps * 2.0 ** -7 * ref.abs()


def assert_bf16_close(got, ref, ulps, atol, what=""):
    """tests/test_gpu_kernels.py assert_bf16_close, restated: non-finite values are rejected before anything is compared"""
    got, ref = got.float().cpu(), ref.float()
    tol = atol + ulps * 2.0 ** -7 * ref.abs()
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} / {got.numel()} values are not finite"
    err = (got - ref).abs()
    assert (err <= tol).all(), f"{what}: {int((~(err <= tol)).sum())} / {err.numel()} off; max abs err {err.max():.4g}"


# ------------------------------------------------------------------------------------------ guarded output buffers
NAN16 = 0x7FD5           # a bf16 NaN no arithmetic produces; int16 view
NAN32 = 0x7FC0D5D5       # the same for fp32; int32 view


def guarded(rows, cols, dtype, ld=None, guard_rows=3, device="cpu"):
    """([guard_rows + rows + guard_rows][ld] buffer filled with NaN bits, its [rows][cols] view): guard rows before and after, guard
    columns [cols, ld) in every row"""
    ld = cols if ld is None else ld
    assert ld >= cols and dtype in (BF, torch.float32)
    buf = torch.empty(rows + 2 * guard_rows, ld, dtype=dtype, device=device)
    if dtype == BF:
        buf.view(torch.int16).fill_(NAN16)
    else:
        buf.view(torch.int32).fill_(NAN32)
    return buf, buf[guard_rows:guard_rows + rows, :cols]


def guards_intact(buf, rows, cols, guard_rows=3):
    """every guard element still holds the fill pattern, bit for bit"""
    bits = buf.view(torch.int16 if buf.dtype == BF else torch.int32).cpu()
    want = NAN16 if buf.dtype == BF else NAN32
    mask = torch.ones_like(bits, dtype=torch.bool)
    mask[guard_rows:guard_rows + rows, :cols] = False
    return bool((bits[mask] == want).all())


# ------------------------------------------------------------------------------------------ gate-sum
def gate_case(rows, D):
    """x, y bf16-valued, one fp32 gate per column — all different, so a wrong column shows"""
    seed = 1000 + 3 * rows + D
    return NS(rows=rows, D=D, x=bfr(rnd(rows, D, seed=seed)), y=bfr(rnd(rows, D, seed=seed + 1)), gate=rnd(D, seed=seed + 2) + 0.25)


def gate_sum_ref(c, rule=None):
    """apply_gate_sum: x + gate[column] * y.  The kernel works on 16-byte chunks g of the flat tensor and has to recover the column from g:
    gate_no_modulo takes chunk g of the gate as it is, gate_wrong_width takes g modulo one chunk too many, gate_trip_local restarts
    the count on every trip of the grid-stride loop (a gate read past its end counts as zero)"""
    rows, D = c.rows, c.D
    if rule is None:
        return c.x.double() + c.gate.double()[None, :] * c.y.double()
    cpr = D // 8
    g = torch.arange(rows * cpr)
    ch = {"gate_no_modulo": g, "gate_wrong_width": g % (cpr + 1), "gate_trip_local": (g % GRID_TRIP) % cpr}[rule]
    chunks = torch.cat([c.gate.view(cpr, 8), torch.zeros(1, 8)])
    gsel = chunks[ch.clamp(max=cpr)].view(rows, D)
    return c.x.double() + gsel.double() * c.y.double()


def gate_applicable(c, rule):
    n = c.rows * (c.D // 8)
    if rule == "gate_trip_local":
        return n > GRID_TRIP and GRID_TRIP % (c.D // 8) != 0
    return c.rows > 1            # one row: the chunk index is the column


# ------------------------------------------------------------------------------------------ LayerNorm
LN_EDGE_ROWS = ("const", "zero", "offset", "small", "large")


def ln_case(rows, D):
    """seeded rows, with (from row 1 on, as far as the rows go) a constant row of 1.5, an all-zero row, a row 40 + noise, a row of scale
    1e-3 and one of scale 1e4; modulation vectors and affine weights that differ per column"""
    seed = 2000 + 7 * rows + D
    x = rnd(rows, D, seed=seed, scale=2.0) + 0.3
    edge = {}
    for i, kind in enumerate(LN_EDGE_ROWS):
        r = 1 + i
        if r >= rows:
            break
        noise = rnd(D, seed=seed + 10 + i)
        x[r] = {"const": torch.full((D,), 1.5), "zero": torch.zeros(D), "offset": 40.0 + noise, "small": 1e-3 * noise, "large": 1e4 * noise}[kind]
        edge[kind] = r
    return NS(rows=rows, D=D, x=bfr(x), scale=rnd(D, seed=seed + 1, scale=0.3), shift=rnd(D, seed=seed + 2, scale=0.3),
              w=rnd(D, seed=seed + 3, scale=0.4) + 1.0, b=rnd(D, seed=seed + 4, scale=0.3), edge=edge)


def layer_norm_ref(x, a, b, eps=1e-5):
    """LayerNorm over the last axis (biased variance about the mean), then * a + b"""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * a.double() + b.double()


def ln_modulate_ref(c):
    return layer_norm_ref(c.x, c.scale.double() + 1.0, c.shift)


def ln_affine_ref(c):
    return layer_norm_ref(c.x, c.w, c.b)


# ------------------------------------------------------------------------------------------ RMSNorm per head + RoPE + scale
NORM_EDGE_HEADS = ("zero", "tiny", "huge", "one_hot")


def norm_case(rows, H, hpw, rope_heads, tables=True):
    """x [rows][H * 64] bf16-valued, one weight row per group of hpw heads (groups differ), cos/sin [rows][32] that differ per row.
    Head vectors (row r, head r % H) for r = 0..3 are the edge vectors: all zero, scale 1e-20, scale 1e15, one non-zero element.

    The tables are quarter turns (cos, sin in {0, +-1}, drawn per row and column) except in rows 0..7 and the last 4 rows, which
    add an angle of scale 0.01.  Reason: the tolerance of this op, 2 bf16 ulps, is that of two chained roundings.  A rotation by a generic angle
    forms c * n0 - s * n1, which cancels; when the FIRST rounding (of n0) falls the other way — fp32 summation order and the last bit
    of rsqrt decide that in roughly 1 element in 10^5 — the difference |c| ulp(n0) is not bounded by any number of ulps of the small
    result.  At 57 600 elements (the generic-angle case of test_gpu_kernels.py) that is rare; at the 8.6 million of these cases it is not.
    A quarter turn moves and negates values without mixing them, so the bound holds for every element, and every wrong row, head
    or sign still moves a value to another place."""
    seed = 3000 + rows + 11 * H + hpw + rope_heads
    G = (H + hpw - 1) // hpw
    x = rnd(rows, H, 64, seed=seed, scale=3.0)
    for r, kind in enumerate(NORM_EDGE_HEADS):
        if r >= rows:
            break
        v = rnd(64, seed=seed + 20 + r)
        one = torch.zeros(64)
        one[(7 * r + 3) % 64] = 5.0
        x[r, r % H] = {"zero": torch.zeros(64), "tiny": 1e-20 * v, "huge": 1e15 * v, "one_hot": one}[kind]
    weight = rnd(G, 64, seed=seed + 1, scale=0.2) + 1.0 + 0.35 * torch.arange(G)[:, None]
    x = settle_first_rounding(bfr(x), weight, hpw, seed + 40)
    cos = sin = None
    if tables:
        g = torch.Generator().manual_seed(seed + 2)
        q = torch.randint(0, 4, (rows, 32), generator=g)
        cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[q]
        sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[q]
        soft = torch.cat([torch.arange(min(8, rows)), torch.arange(max(rows - 4, 0), rows)]).unique()
        ang = q[soft].float() * (math.pi / 2) + rnd(soft.numel(), 32, seed=seed + 3, scale=0.01)
        cos[soft], sin[soft] = torch.cos(ang), torch.sin(ang)
    return NS(rows=rows, H=H, hpw=hpw, rope_heads=rope_heads, G=G, x=x.reshape(rows, H * 64), weight=weight, cos=cos, sin=sin)


def rms_norm64(x, w):
    """RMSNorm over the last axis in float64: x * rsqrt(mean(x^2) + eps) * w, eps = finfo(fp32).eps; not rounded"""
    x = x.double()
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 2.0 ** -23) * w.double()


def settle_first_rounding(x, weight, hpw, seed):
    """x [rows][H][64] with every head vector whose normalised values round to bf16 differently in fp32 (the oracle's rms_norm_heads)
    and in float64 drawn again, until none is left (an edge vector that does is kept).  The op has two chained roundings; the second
    one, of out_scale * n, doubles a first one that fell the other way to as much as three quarters of the op's tolerance — in the
    reference itself, before any kernel has run.  fp32 and float64 disagree on about 1 head vector in 2000 (65 of 134 456 at 2401 x 56), so a redraw or two settles it.
    What a kernel's own fp32 arithmetic does with the same inputs is not looked at: its first rounding may still fall either way."""
    from oracle import k5_oracle as O
    rows, H, _ = x.shape
    grp = (torch.arange(H) // hpw)
    edge = torch.zeros(rows, H, dtype=torch.bool)
    for r in range(min(len(NORM_EDGE_HEADS), rows)):
        edge[r, r % H] = True
    for it in range(16):
        n32 = torch.cat([O.rms_norm_heads(x[:, g * hpw:(g + 1) * hpw], weight[g], "bf16") for g in range(weight.shape[0])], 1)
        bad = (n32.double() != r16(rms_norm64(x, weight[grp][None]))).any(-1) & ~edge
        if not bad.any():
            return x
        x[bad] = bfr(rnd(int(bad.sum()), 64, seed=seed + it, scale=3.0))
    raise AssertionError("head vectors keep rounding differently in fp32 and float64")


def norm_rope_ref(c, rule=None, out_scale=1.0, scale_from_head=None, last_rounding=True):
    """norm_qk + apply_rotary on [rows][H][64]: n = bf16(x * rsqrt(mean(x^2) + eps) * weight[head // hpw]); heads < rope_heads (tables given)
    are rotated pairwise, (x0, x1) -> (c x0 - s x1, s x0 + c x1), with row r's table row; heads >= scale_from_head are multiplied by
    out_scale.  A rotated head gets one rounding of scale * rot, an unrotated one one more rounding of scale * n (last_rounding=False
    leaves that last rounding out).  Returns float64 [rows][H * 64]."""
    rows, H = c.rows, c.H
    x = c.x.double().view(rows, H, 64)
    head = torch.arange(H)
    grp = {"group_mod": head % c.hpw, "group_ignored": head * 0}.get(rule, head // c.hpw).clamp(max=c.G - 1)
    n = r16(rms_norm64(x, c.weight[grp][None]))
    last = r16 if last_rounding else (lambda v: v)
    sc = torch.ones(H, dtype=F64)
    if scale_from_head is not None:
        sc[scale_from_head:] = out_scale
    out = last(n * sc[None, :, None])
    if c.cos is not None:
        rot_heads = {"rope_le": head <= c.rope_heads, "rope_all": head >= 0}.get(rule, head < c.rope_heads)
        trip = norm_trip_rows(H)[0]
        r = torch.arange(rows)
        ri = {"cs_row_lag": torch.where(r >= trip, r - trip, r), "cs_row_mod": r % trip}.get(rule, r)
        cs, sn = c.cos.double()[ri][:, None, :], c.sin.double()[ri][:, None, :]
        p = n.view(rows, H, 32, 2)
        rot = torch.stack([cs * p[..., 0] - sn * p[..., 1], sn * p[..., 0] + cs * p[..., 1]], -1).view(rows, H, 64)
        out = torch.where(rot_heads[None, :, None], last(rot * sc[None, :, None]), out)
    return out.reshape(rows, H * 64)


def norm_applicable(c, rule):
    if rule in ("group_mod", "group_ignored"):
        return c.G > 1
    if c.cos is None:
        return False
    if rule == "rope_le":
        return c.rope_heads < c.H
    if rule == "rope_all":
        return c.rope_heads < c.H
    return c.rope_heads > 0 and c.rows > norm_trip_rows(c.H)[0]        # the two table-row rules: only a later trip can tell


# ------------------------------------------------------------------------------------------ fp32 GEMV
def gemv_int_case(N, K, has_b, has_add):
    """integers: x, W in [-8, 8], b, add in [-64, 64] — every partial sum in any order is an integer below 2^24, exact in fp32"""
    g = torch.Generator().manual_seed(4000 + N + 3 * K + 2 * has_b + has_add)
    x = torch.randint(-8, 9, (K,), generator=g)
    W = torch.randint(-8, 9, (N, K), generator=g)
    b = torch.randint(-64, 65, (N,), generator=g) if has_b else None
    add = torch.randint(-64, 65, (N,), generator=g) if has_add else None
    return NS(N=N, K=K, x=x, W=W, b=b, add=add)


def gemv_int_bound(c):
    """max over rows of sum |W x| + |b| + |add|: below 2^24, every order of summation is exact"""
    m = (c.W.abs() * c.x.abs()[None, :]).sum(1)
    if c.b is not None:
        m = m + c.b.abs()
    if c.add is not None:
        m = m + c.add.abs()
    return int(m.max())


def gemv_silu_case(N, K):
    s = 5000 + N + K
    return NS(N=N, K=K, x=rnd(K, seed=s), W=rnd(N, K, seed=s + 1, scale=0.05), b=rnd(N, seed=s + 2, scale=0.1), add=rnd(N, seed=s + 3, scale=0.1))


def gemv_ref(x, W, b=None, add=None, silu=False):
    """y = W act(x) + b + add in float64, and the sum of the absolute values of the terms (the scale of any summation order's error)"""
    x = x.double()
    if silu:
        x = x / (1.0 + torch.exp(-x))
    terms = W.double() * x[None, :]
    y, mag = terms.sum(1), terms.abs().sum(1)
    for v in (b, add):
        if v is not None:
            y, mag = y + v.double(), mag + v.double().abs()
    return y, mag


def gemv_silu_tol(K, mag):
    """any summation order of K + 2 fp32 terms is within gamma_K * sum |terms|; 32 more units cover expf and the division of the SiLU"""
    return (K + 32) * 2.0 ** -24 * mag


# ------------------------------------------------------------------------------------------ sinusoids
def freqs64(n, exact=False):
    """get_freqs: exp(-ln(1e4) * i / n), i = 0..n-1, in float64.  The model (models/utils.py get_freqs) forms the ARGUMENT in fp32 — an
    fp32 product, then an fp32 quotient — and that argument is what defines its frequencies: a relative 2^-23 of an argument of 4 to 9
    moves a frequency by up to 2^-20 of itself, more than the whole tolerance of a large angle allows, and an implementation that
    rounded the argument differently would compute another model's frequencies.  So the reference takes the exact exponential of the
    fp32 argument.  exact=True: the argument in float64 as well (the mathematical frequencies)."""
    if exact:
        return torch.exp(-math.log(10000.0) * torch.arange(n, dtype=F64) / n)
    arg = torch.tensor(-math.log(10000.0), dtype=torch.float32) * torch.arange(n, dtype=torch.float32) / n
    return torch.exp(arg.double())


def time_angles(t, D, exact=False):
    """t * freq_i in float64; t is the fp32 value the entry point receives"""
    return torch.tensor(t, dtype=torch.float32).double() * freqs64(D // 2, exact)


def angle_tol(a):
    """fp32 rounding of the angle is |a| 2^-24, a few ulps of expf in the frequency scale with it; 2e-6 is the tolerance of a table of small
    angles.  Against the mathematical frequencies (exact=True) the fp32 argument adds up to |a| 2^-20 where the argument is large, which
    is where the angle is small: at most 0.85 of this tolerance for positions and times up to 1000."""
    return 2e-6 + a.abs() * 2.0 ** -21


def rope_case(T, H, W, perm_kind, axes, scales, seed):
    """positions offset and strided up to 127 (not arange), a token permutation: "fractal" = the 8 x 8 block order, "random" = seeded"""
    g = torch.Generator().manual_seed(seed)

    def positions(n):
        step = (127 - 3) // max(n - 1, 1)
        step = min(step, 1 + int(torch.randint(1, 6, (1,), generator=g)))
        off = int(torch.randint(1, 127 - step * (n - 1) + 1, (1,), generator=g))
        return (off + step * torch.arange(n)).int()

    pos = [positions(T), positions(H), positions(W)]
    assert all(int(v.min()) >= 1 and int(v.max()) <= 127 for v in pos)          # offset, strided, inside the table of 128 positions
    return NS(T=T, H=H, W=W, pos=pos, axes=tuple(axes), scales=tuple(scales), perm=make_perm(perm_kind, T, H, W, g), perm_kind=perm_kind)


def make_perm(kind, T, H, W, g):
    if kind is None:
        return None
    if kind == "fractal":              # models/utils.py fractal_flatten: token i = ((t Hb + hb) Wb + wb) 64 + hi 8 + wi <-> raster (t, hb 8 + hi, wb 8 + wi)
        return torch.arange(T * H * W).reshape(T, H // 8, 8, W // 8, 8).permute(0, 1, 3, 2, 4).reshape(-1).int()
    assert kind == "random"
    return torch.randperm(T * H * W, generator=g).int()


def token_coords(rows, H, W, perm, rule):
    """(t, h, w) of the raster token that row `rows[i]` of the flattened sequence holds: flat[i] = raster[perm[i]]"""
    if perm is None:
        tok = rows
    elif rule == "perm_inverse":
        tok = torch.argsort(perm.long())[rows]
    else:
        tok = perm.long()[rows]
    if rule == "swap_hw":
        return tok // (W * H), tok % H, (tok // H) % W
    return tok // (W * H), (tok // W) % H, tok % W


def freq_at(i, n, exact=False):
    """frequency i of n as freqs64 forms it, for any integer i (a mutated column split can ask for i = -1 or i = n)"""
    if exact:
        return math.exp(-math.log(10000.0) * i / n)
    arg = torch.tensor(-math.log(10000.0), dtype=torch.float32) * torch.tensor(float(i), dtype=torch.float32) / n
    return math.exp(float(arg))


def rope_angles_ref(c, rule=None, exact=False):
    """RoPE3D angles [T * H * W][32] in float64: columns [0, n0) = pos_t * freq / s0, [n0, n0 + n1) the h axis, the rest the w axis;
    frequencies as freqs64 defines them"""
    n0, n1, n2 = c.axes
    t, h, w = token_coords(torch.arange(c.T * c.H * c.W), c.H, c.W, c.perm, rule)
    t, h, w = t.clamp(max=c.T - 1), h.clamp(max=c.H - 1), w.clamp(max=c.W - 1)      # (a mutated decomposition can leave the grid)
    s = list(c.scales)
    if rule == "scale_1_on_2":
        s[2] = s[1]
    b0, b1 = (n0 + 1, n0 + n1 + 1) if rule == "axis_shift" else (n0, n0 + n1)
    cols = []
    for j in range(32):
        if j < b0:
            p, i, n, sc = c.pos[0].long()[t], j, n0, s[0]
        elif j < b1:
            p, i, n, sc = c.pos[1].long()[h], j - n0, n1, s[1]
        else:
            p, i, n, sc = c.pos[2].long()[w], j - n0 - n1, n2, s[2]
        cols.append(p.double() * freq_at(i, n, exact) / sc)
    return torch.stack(cols, 1)


def rope_applicable(c, rule):
    if rule == "perm_inverse":
        return c.perm is not None
    if rule == "scale_1_on_2":
        return c.scales[1] != c.scales[2]
    return True


# ------------------------------------------------------------------------------------------ patchify / unpatchify
def patch_case(T, H, W, Cx, Cin, Kpad, perm_kind, cond, seed):
    """fp32 latent (T, H, W, Cx); with cond the conditioning (T, H, W, Cin - Cx), otherwise channels [Cx, Cin) read as zero"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H, W, Cx, generator=g)
    vc = torch.randn(T, H, W, Cin - Cx, generator=g) if cond else None
    return NS(T=T, H=H, W=W, Cx=Cx, Cin=Cin, Kpad=Kpad, x=x, vc=vc, perm=make_perm(perm_kind, T, H // 2, W // 2, g), perm_kind=perm_kind)


def patchify_ref(c, rule=None):
    """VisualEmbeddings patchify, patch (1, 2, 2): row i = raster token perm[i] = (t, hp, wp); feature (ph * 2 + pw) * Cin + ch holds
    pixel (t, 2 hp + ph, 2 wp + pw) channel ch; columns [4 Cin, Kpad) are zero.  A gather of the bf16-rounded source: [Ntok][Kpad] bf16."""
    Hp, Wp, Cin = c.H // 2, c.W // 2, c.Cin
    n = c.T * Hp * Wp
    full = torch.zeros(c.T, c.H, c.W, Cin)
    full[..., :c.Cx] = c.x
    if c.vc is not None:
        full[..., c.Cx:] = c.vc
    src = torch.cat([full.reshape(-1).to(BF), torch.zeros(1, dtype=BF)])
    t, hp, wp = token_coords(torch.arange(n), Hp, Wp, c.perm, rule)
    f = torch.arange(4 * Cin)
    if rule == "feature_cphpw":
        ch, ph, pw = f // 4, (f // 2) % 2, f % 2
    else:
        ch, ph, pw = f % Cin, f // (2 * Cin), (f // Cin) % 2
    pix = (t[:, None] * c.H + 2 * hp[:, None] + ph[None, :]) * c.W + 2 * wp[:, None] + pw[None, :]
    idx = (pix * Cin + ch[None, :]) % (src.numel() - 1)                 # (a mutated decomposition can leave the tensor)
    idx = torch.cat([idx, torch.full((n, c.Kpad - 4 * Cin), src.numel() - 1)], 1)
    return src[idx]


def unpatch_case(T, Hp, Wp, C, ldx, perm_kind, seed):
    """x [Ntok][ldx] bf16: features (c, ph, pw) in columns [0, 4 C), NaN in the pad columns"""
    g = torch.Generator().manual_seed(seed)
    n = T * Hp * Wp
    x = torch.full((n, ldx), float("nan"), dtype=BF)
    x[:, :4 * C] = torch.randn(n, 4 * C, generator=g).to(BF)
    return NS(T=T, Hp=Hp, Wp=Wp, C=C, ldx=ldx, x=x, perm=make_perm(perm_kind, T, Hp, Wp, g), perm_kind=perm_kind)


def unpatchify_ref(c, rule=None):
    """OutLayer un-patchify: out (T, 2 Hp, 2 Wp, C); pixel (t, 2 hp + ph, 2 wp + pw) channel ch = feature ch * 4 + ph * 2 + pw of the row
    that holds raster token (t, hp, wp)"""
    Hp, Wp, C = c.Hp, c.Wp, c.C
    n = c.T * Hp * Wp
    t, hp, wp = token_coords(torch.arange(n), Hp, Wp, c.perm, rule)
    f = torch.arange(4 * C)
    if rule == "feature_phpwc":
        ch, ph, pw = f % C, f // (2 * C), (f // C) % 2
    else:
        ch, ph, pw = f // 4, (f // 2) % 2, f % 2
    dst = ((t[:, None] * 2 * Hp + 2 * hp[:, None] + ph[None, :]) * (2 * Wp) + 2 * wp[:, None] + pw[None, :]) * C + ch[None, :]
    ld = 4 * C if rule == "ldx_4c" else c.ldx
    src = c.x.reshape(-1)[(torch.arange(n)[:, None] * ld + f[None, :])]
    out = torch.zeros(n * 4 * C, dtype=BF)
    out[dst.reshape(-1) % out.numel()] = src.reshape(-1)
    return out.view(c.T, 2 * Hp, 2 * Wp, C)


def patch_applicable(c, rule):
    if rule == "perm_inverse":
        return c.perm is not None
    if rule == "ldx_4c":
        return c.ldx != 4 * c.C
    return True


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
