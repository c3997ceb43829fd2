"""GPU parity of the NABLA path: block-map selection (nablaT_v2 + STA window), block-sparse attention, and the
whole DiT forward / sampler with `attention.type: nabla`, against the CPU oracle and the reference's golden vectors.

The map is a discrete decision taken on bf16-rounded block means: the GPU and CPU agree except for entries whose
cumulative probability sits within fp32 summation noise of the 1-P cut (and exact ties, resolved by index like a
stable sort).  test_nabla_map_matches_oracle checks WHERE every differing entry sits (|cdf - (1-P)| <= 1e-5 on data whose
logits are summation-order independent, <= 0.05 where a bf16 logit may flip); everything downstream of an agreed map is
held to the dense-path tolerances."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
from oracle import parity  # noqa: E402
from kit import BF, E, bfr, rel  # noqa: E402


def _cdf_at_entries(q, k, mode="bf16"):
    """The oracle's ascending cumulative sum evaluated AT every (head, row, key block) entry, plus the entry's own p:
    an entry is kept iff its cdf >= 1 - P (utils.py:151-156)."""
    import math
    S, H, d = q.shape
    nb = S // 64
    r = bfr if mode == "bf16" else (lambda t: t)
    qa = r(q.float().transpose(0, 1).reshape(H, nb, 64, d).mean(-2))
    ka = r(k.float().transpose(0, 1).reshape(H, nb, 64, d).mean(-2))
    p = torch.softmax(r(r(qa @ ka.transpose(-2, -1)) / math.sqrt(d)), dim=-1)
    vals, inds = p.sort(-1)
    cdf = torch.zeros_like(p)
    cdf.scatter_(-1, inds, vals.cumsum(-1))
    return cdf, p


def _may_differ(q, k, P, tol, mode="bf16"):
    """(H, nb, nb) bool: entries where two correct implementations of nablaT_v2's cut (utils.py:151-156) may disagree —
    * the entry's cumulative mass, or the mass just below it, is within `tol` of the threshold 1 - P (fp32 exp / cumsum order; on
      random data a bf16 logit one ulp off), or
    * it belongs to a group of EXACTLY tied probabilities whose cumulative span [below the group, top of the group] contains the
      threshold: which members of such a group are kept depends on the sort's order among equals (the reference's torch.sort is not
      stable; the kernel ranks ties by index).
    Vectorised (a 3660-block row set has 13 M entries)."""
    cdf, p = _cdf_at_entries(q, k, mode)
    thr = 1.0 - P
    near = ((cdf - thr).abs() <= tol) | ((cdf - p - thr).abs() <= tol)
    vals, inds = p.sort(-1)
    cs = vals.cumsum(-1)
    new_grp = torch.ones_like(vals, dtype=torch.bool)
    new_grp[..., 1:] = vals[..., 1:] != vals[..., :-1]
    gid = new_grp.long().cumsum(-1) - 1                                   # tie-group index along the sorted row
    lo = torch.full_like(vals, float("inf")).scatter_reduce(-1, gid, cs - vals, "amin", include_self=True)
    hi = torch.full_like(vals, float("-inf")).scatter_reduce(-1, gid, cs, "amax", include_self=True)
    cnt = torch.zeros_like(vals).scatter_add(-1, gid, torch.ones_like(vals))
    g_ok = (cnt > 1) & (lo - tol <= thr) & (thr <= hi + tol)              # per group
    ok_sorted = g_ok.gather(-1, gid)
    tie_ok = torch.zeros_like(ok_sorted).scatter(-1, inds, ok_sorted)
    return near | tie_ok


@pytest.mark.parametrize("grid,window,P,H", [((6, 2, 2), (3, 1, 1), 0.7, 2), ((10, 3, 4), (5, 3, 3), 0.9, 3),
                                             ((4, 2, 3), (11, 3, 3), 0.5, 1), ((3, 1, 1), (1, 1, 1), 0.9, 2),
                                             # one case per register-resident instantiation of the select kernel (values per lane x rows
                                             # per wave): 600 blocks <16,4>, 1464 (the 10 s clip) <24,4>, 1600 <32,4>, 2100 = NV 48 (33 words; NV 64 starts at 3073 blocks)
                                             ((25, 4, 6), (5, 3, 3), 0.9, 2), ((61, 4, 6), (11, 3, 3), 0.9, 2),
                                             ((25, 8, 8), (11, 3, 3), 0.9, 1), ((35, 6, 10), (5, 3, 3), 0.8, 1),
                                             # BASELINE config 5's own row length: (61, 96, 160) latent = 61 x 6 x 10 = 3660 blocks (<64,2>)
                                             ((61, 6, 10), (11, 3, 3), 0.9, 1)])
@pytest.mark.parametrize("data", ["exact", "random"])
def test_nabla_map_matches_oracle(E, grid, window, P, H, data):
    """k5_nabla_select_bf16 vs oracle.nabla_block_mask, entry by entry.
    data = "exact": small-integer q / k — block means, their dot products and hence the bf16 logits are the same numbers
      whatever the summation order, so the two maps may differ ONLY where the cumulative mass sits within 1e-5 of the
      threshold 1 - P (fp32 exp / cumsum order).
    data = "random": the bf16 rounding of a logit (qa . ka summed in another order) can flip by one ulp = 2^-8 |logit|,
      which moves that block's p — and the cumulative mass of everything sorted above it — by a percent or two: a differing
      entry must still sit within 0.05 of the threshold in cumulative mass (the reference on a GPU has the same ambiguity:
      its logits are a bf16 matmul whose accumulation order is the library's)."""
    T, Hb, Wb = grid
    nb = T * Hb * Wb
    N = nb * 64
    g = torch.Generator().manual_seed(nb)
    if data == "exact":
        # every token of a block carries the same vector with entries in {-1, 0, 1}: the block means ARE those vectors,
        # their dot products are integers in [-64, 64] -> exact in fp32 in any order, bf16-exact, logits = multiples of 1/8
        q = torch.randint(-1, 2, (nb, 1, H, 64), generator=g).float().expand(nb, 64, H, 64).reshape(N, H, 64).contiguous()
        k = torch.randint(-1, 2, (nb, 1, H, 64), generator=g).float().expand(nb, 64, H, 64).reshape(N, H, 64).contiguous()
        tol = 1e-5
    else:
        q = bfr(torch.randn(N, H, 64, generator=g))
        k = bfr(torch.randn(N, H, 64, generator=g) + 0.5 * q)
        tol = 0.05
    sta = O.fast_sta(T, Hb, Wb, *window)
    ref = O.nabla_block_mask(q, k, sta, P, "bf16")                      # (H, nb, nb) bool
    ws = E.nabla_select(q.reshape(N, -1).cuda().to(BF), k.reshape(N, -1).cuda().to(BF), H, grid, window, P)
    got = E.nabla_mask(ws, H, nb).cpu()
    diff = (got != ref)
    if diff.any():
        bad = diff & ~_may_differ(q, k, P, tol)
        assert not bad.any(), (int(bad.sum()), bad.nonzero()[:5].tolist())
    # how MANY entries may differ: integer logits make large tie groups (every member of a group straddling the cut may flip,
    # checked one by one above), random logits at most a few entries next to the cut per row
    # (the tie groups of integer logits grow with the row length: up to a tenth of a 2100-block row ties at the cut)
    print(f"nabla map {grid} {data}: {int(diff.sum())} of {diff.numel()} entries differ from the oracle (every one at the cut, checked above)")
    assert diff.float().mean().item() <= ((3e-2 if nb < 1000 else 1e-1) if data == "exact" else 5e-3), (int(diff.sum()), diff.numel())
    assert (got & sta[None]).sum() == sta.sum() * H                     # the STA window is always kept
    assert got.any(-1).all()                                            # every row keeps at least one block


def test_nabla_map_low_entropy_rows_and_ties(E):
    """Identical key blocks -> exact ties in the softmax: tie entries are kept from the highest index down (stable sort)."""
    T, Hb, Wb, H = 8, 1, 1, 1
    nb, N = 8, 512
    q = bfr(torch.randn(N, H, 64, generator=torch.Generator().manual_seed(1)))
    kblock = bfr(torch.randn(64, H, 64, generator=torch.Generator().manual_seed(2)))
    k = kblock.repeat(nb, 1, 1)                                        # every kv block has the same mean -> uniform softmax
    sta = O.fast_sta(T, Hb, Wb, 1, 1, 1)
    ref = O.nabla_block_mask(q, k, sta, 0.6, "bf16")
    ws = E.nabla_select(q.reshape(N, -1).cuda().to(BF), k.reshape(N, -1).cuda().to(BF), H, (T, Hb, Wb), (1, 1, 1), 0.6)
    got = E.nabla_mask(ws, H, nb).cpu()
    # uniform p = 1/8: ascending cumsum reaches 0.4 at the 4th entry -> 5 kept (ranks 4..8) + the diagonal
    assert (got.sum(-1) >= 5).all() and (got.sum(-1) <= 6).all()
    assert (got.float().mean() - ref.float().mean()).abs() <= 0.15      # CPU sort order among exact ties may differ


def test_sparse_attention_matches_masked_sdpa(E):
    T, Hb, Wb, H = 6, 2, 2, 2
    nb, N = 24, 1536
    g = torch.Generator().manual_seed(7)
    q, k, v = bfr(torch.randn(N, H, 64, generator=g)), bfr(torch.randn(N, H, 64, generator=g)), bfr(torch.randn(N, H, 64, generator=g))
    qd, kd = q.reshape(N, -1).cuda().to(BF), k.reshape(N, -1).cuda().to(BF)
    vt = v.reshape(N, -1).t().contiguous().cuda().to(BF)
    ws = E.nabla_select(qd, kd, H, (T, Hb, Wb), (3, 1, 1), 0.6)
    mask = E.nabla_mask(ws, H, nb).cpu()
    assert 0.2 < mask.float().mean().item() < 0.9
    R = parity.AttentionRef(q, k, v, block_mask=mask)
    ref = R.bf16
    got = E.attention_nabla(qd, kd, vt, H, ws)
    assert torch.isfinite(got.float()).all()
    err = (got.float().cpu() - ref).abs().max().item()
    assert err <= 2e-2, err
    R.close(got, parity.MARGIN_SPARSE, "sparse attention, online max")
    # bounded-score variant of the sparse kernel (RMS-normalised inputs)
    def rmsn(x):
        return bfr(x / x.pow(2).mean(-1, keepdim=True).sqrt())
    qn, kn = rmsn(q), rmsn(k)
    qd, kd = qn.reshape(N, -1).cuda().to(BF), kn.reshape(N, -1).cuda().to(BF)
    ws = E.nabla_select(qd, kd, H, (T, Hb, Wb), (3, 1, 1), 0.6)
    mask = E.nabla_mask(ws, H, nb).cpu()
    a = E.attention_nabla(qd, kd, vt, H, ws, score_bound=64 * 1.05)
    R = parity.AttentionRef(qn, kn, v, block_mask=mask)
    assert torch.isfinite(a.float()).all()
    assert (a.float().cpu() - R.bf16).abs().max().item() <= 2e-2
    R.close(a, parity.MARGIN_SPARSE, "sparse attention, bounded scores")


@pytest.fixture(scope="module")
def tiny(golden_meta, tiny_sd):
    from kandinsky.models.dit import DiffusionTransformer3D
    c = dict(golden_meta["tiny_config"])
    dit = DiffusionTransformer3D(**c)
    dit.load_state_dict(tiny_sd, assign=True)
    c["patch_size"], c["axes_dims"] = tuple(c["patch_size"]), tuple(c["axes_dims"])
    return dit.to("cuda:0"), O.DitConfig(**c)


def test_forward_nabla_vs_oracle_and_golden(tiny, tiny_sd, golden, golden_meta):
    dit, cfg = tiny
    attn = golden_meta["nabla_attention"]
    sparse = {"P": attn["P"], "wT": attn["wT"], "wH": attn["wH"], "wW": attn["wW"], "to_fractal": True}
    pos = [torch.arange(6), torch.arange(16), torch.arange(16)]
    out = dit(golden["nabla.fwd.x"].cuda(), golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), golden["fwd.time"], pos,
              torch.arange(7), scale_factor=(1.0, 2.0, 2.0), sparse_params=sparse)
    osp = O.get_sparse_params(attn, (6, 32, 32), cfg.patch_size)
    ref16 = O.dit_forward(tiny_sd, cfg, golden["nabla.fwd.x"], golden["fwd.text"], golden["fwd.pooled"], golden["fwd.time"], pos,
                          torch.arange(7), (1.0, 2.0, 2.0), osp, "bf16")
    assert rel(out, ref16) <= 2.5e-2, rel(out, ref16)
    assert rel(out, golden["nabla.fwd.out"]) <= 4e-2, rel(out, golden["nabla.fwd.out"])
    # NABLA really changes the result (the map is not all-ones) and dense != sparse
    dense = dit(golden["nabla.fwd.x"].cuda(), golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), golden["fwd.time"], pos,
                torch.arange(7), scale_factor=(1.0, 2.0, 2.0))
    assert rel(out, dense) > 1e-3


def test_generate_nabla_cfg(tiny, tiny_sd, golden, golden_meta):
    from kandinsky.config import Conf
    from kandinsky.generation_utils import generate
    dit, cfg = tiny
    attn = golden_meta["nabla_attention"]
    conf = Conf({"model": {"dit_params": {"patch_size": [1, 2, 2]}, "attention": attn}, "metrics": {"scale_factor": [1.0, 2.0, 2.0]}})
    pos = [torch.arange(6), torch.arange(16), torch.arange(16)]
    te = {"text_embeds": golden["fwd.text"].cuda(), "pooled_embed": golden["fwd.pooled"].cuda()}
    ne = {"text_embeds": golden["gen.null_text"].cuda(), "pooled_embed": golden["gen.null_pooled"].cuda()}
    out = generate(dit, "cuda:0", (6, 32, 32, 16), 2, te, ne, pos, torch.arange(7), torch.arange(4), 2.0, 5.0, conf,
                   noise=golden["gen.nabla.noise"])
    assert rel(out, golden["gen.nabla.final"]) <= 3e-2, rel(out, golden["gen.nabla.final"])


def test_nabla_rejects_unaligned_latent(tiny, golden):
    dit, _ = tiny
    sparse = {"P": 0.9, "wT": 3, "wH": 3, "wW": 3}
    with pytest.raises(RuntimeError, match="divisible by 16"):
        dit(golden["fwd.x"].cuda(), golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), golden["fwd.time"],
            [torch.arange(3), torch.arange(4), torch.arange(6)], torch.arange(7), sparse_params=sparse)


# ------------------------------------------------------------------------------------------ NABLA under sequence parallelism
def test_rect_map_and_chunked_sparse_attention_equal_the_square_rows(E):
    """A rank holding query blocks [qb0, qb0+nqb) and all keys (V^T in per-rank chunks) gets exactly the rows of the
    single-GPU map and of the single-GPU block-sparse attention (bit for bit: same kernels, same key order)."""
    T, Hb, Wb, H, P = 8, 2, 2, 2, 4                      # 32 blocks, 4 "ranks" of 8 blocks
    nb, N = 32, 2048
    g = torch.Generator().manual_seed(21)
    def rmsn(x):
        return bfr(x / x.pow(2).mean(-1, keepdim=True).sqrt())
    q, k, v = rmsn(torch.randn(N, H, 64, generator=g)), rmsn(torch.randn(N, H, 64, generator=g)), bfr(torch.randn(N, H, 64, generator=g))
    qd, kd = q.reshape(N, -1).cuda().to(BF), k.reshape(N, -1).cuda().to(BF)
    vt = v.reshape(N, -1).t().contiguous().cuda().to(BF)                       # [H*64][N]
    n = N // P
    vt_chunks = vt.reshape(H * 64, P, n).permute(1, 0, 2).contiguous()         # [P][H*64][n]
    ws = E.nabla_select(qd, kd, H, (T, Hb, Wb), (3, 1, 1), 0.6)
    full_mask = E.nabla_mask(ws, H, nb)
    full_out = E.attention_nabla(qd, kd, vt, H, ws, score_bound=64 * 1.05)
    L = E.lib()
    for r in (0, 2, 3):
        qb0, nqb = r * (n // 64), n // 64
        qloc = qd[r * n:(r + 1) * n]
        wsr = torch.empty(L.k5_nabla_workspace_size(H, nb), dtype=torch.uint8, device="cuda")
        E.check(L.k5_nabla_select_rect_bf16(qloc.data_ptr(), kd.data_ptr(), qloc.stride(0), kd.stride(0), H, n, qb0, N, T, Hb, Wb,
                                            3, 1, 1, 0.6, wsr.data_ptr(), E.stream_ptr()))
        m = torch.empty(H, nqb, nb, dtype=torch.uint8, device="cuda")
        E.check(L.k5_nabla_mask_rect_u8(wsr.data_ptr(), H, nqb, nb, m.data_ptr(), E.stream_ptr()))
        assert torch.equal(m.bool(), full_mask[:, qb0:qb0 + nqb])
        o = torch.empty(n, H * 64, dtype=BF, device="cuda")
        E.check(L.k5_attention_nabla_rect_bf16(qloc.data_ptr(), kd.data_ptr(), vt_chunks.data_ptr(), o.data_ptr(), H, n, N,
                                               qloc.stride(0), kd.stride(0), n, o.stride(0), 64 * 1.05, wsr.data_ptr(), n,
                                               H * 64 * n, E.stream_ptr()))
        assert torch.equal(o, full_out[r * n:(r + 1) * n])


def test_engine_nabla_sharded_path_world1_matches_fused(tiny, golden, golden_meta):
    """world = 1 RCCL communicator: the sequence-parallel NABLA branch of the engine vs the fused NABLA path.  Same block map
    and same attention kernel; the fused path hands the attention keys pre-multiplied by the softmax scale (one bf16 rounding
    of c*k instead of k), the sharded path keeps one set of (unscaled) gathered keys for map and attention -> bf16-level
    differences only."""
    from kandinsky.models.dit import DiffusionTransformer3D
    dit, _ = tiny
    attn = golden_meta["nabla_attention"]
    sparse = {"P": attn["P"], "wT": attn["wT"], "wH": attn["wH"], "wW": attn["wW"], "to_fractal": True}
    pos = [torch.arange(6), torch.arange(16), torch.arange(16)]
    args = (golden["nabla.fwd.x"].cuda(), golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), golden["fwd.time"], pos, torch.arange(7))
    a = dit(*args, scale_factor=(1.0, 2.0, 2.0), sparse_params=sparse)
    c = dict(golden_meta["tiny_config"])
    sp = DiffusionTransformer3D(**c)
    sp.load_state_dict(dit.state_dict(), assign=True)
    sp = sp.to("cuda:0").enable_sequence_parallel(0, 1, device="cuda:0")
    b = sp(*args, scale_factor=(1.0, 2.0, 2.0), sparse_params=sparse)
    assert rel(b, a) <= 5e-3, rel(b, a)


def test_nabla_config4_size_properties(E):
    """BASELINE config 4 shape: 768x512 10 s latent -> 93 696 tokens = 1464 blocks (61 frames x 4 x 6 spatial tiles), window
    (11,3,3), on 2 heads.  Size-independent properties of map + sparse attention: every row keeps >= 1 block, the STA window
    is a subset of the map, the map's density is between the STA floor (4.8 %) and 1, softmax rows sum to one over the
    kept blocks (V = const -> O = const on all 93 696 rows), and P = 0 (top-1 + STA) is sparser than P = 0.9."""
    T, Hb, Wb, H = 61, 4, 6, 2
    nb = T * Hb * Wb
    N = nb * 64
    assert N == 93696
    g = torch.Generator(device="cuda").manual_seed(3)
    q = torch.randn(N, H * 64, device="cuda", generator=g).to(BF)
    k = (torch.randn(N, H * 64, device="cuda", generator=g) + 0.5 * q.float()).to(BF)
    vt = torch.full((H * 64, N), 0.75, dtype=BF, device="cuda")
    sta = O.fast_sta(T, Hb, Wb, 11, 3, 3)
    floor = sta.float().mean().item()
    assert abs(floor - 0.048) < 0.004
    dens = {}
    for P in (0.0, 0.9):
        ws = E.nabla_select(q, k, H, (T, Hb, Wb), (11, 3, 3), P)
        m = E.nabla_mask(ws, H, nb).cpu()
        assert m.any(-1).all()
        assert (m & sta[None]).sum() == sta.sum() * H
        dens[P] = m.float().mean().item()
        out = E.attention_nabla(q, k, vt, H, ws)
        assert (out.float() - 0.75).abs().max().item() <= 2 ** -8
    assert floor <= dens[0.0] <= floor + 1.0 / nb + 1e-6          # STA window + at most the top-1 block per row
    assert dens[0.0] < dens[0.9] <= 1.0
    print(f"config-4 map density: STA floor {floor:.4f}, P=0 {dens[0.0]:.4f}, P=0.9 {dens[0.9]:.4f}")


def _flags_rows(E, qf, kf, H):
    qstat, kstat = (qf * qf).sum(-1).amax(0).contiguous().cuda(), (kf * kf).sum(-1).amax(0).contiguous().cuda()
    flags = torch.zeros(H, dtype=torch.int32, device="cuda")
    kmax = torch.zeros(H, device="cuda")
    E.check(E.lib().k5_attention_flags_rows(qstat.data_ptr(), kstat.data_ptr(), 1, H, H, 0, flags.data_ptr(), kmax.data_ptr(), E.stream_ptr()))
    torch.cuda.synchronize()
    return flags, kmax


@pytest.mark.parametrize("case", ["gain1", "gain3", "late"])
def test_two_pass_list_walk_on_prescaled_keys(E, case):
    """The sequence-parallel engine's NABLA attention at kernel level: rank r's own key blocks lead every list
    (k5_nabla_select_rect_local_bf16), pass 1 attends them and leaves the fp32 state, pass 2 resumes over the rest — against the
    one-pass walk of the same lists and against the oracle's masked attention.  "gain3": bound 104, the fixed form on per-row
    offsets in both passes.  "late": head 0's LOCAL keys point away from every query — its rows underflow in pass 1 (flag 2), and the
    online launch of pass 2 must recompute the head over its whole lists, ignoring the state pass 1 left."""
    T, Hb, Wb, H, P = 8, 2, 2, 2, 4
    nb, N = 32, 2048
    n = N // P
    g = torch.Generator().manual_seed(33)
    gain = {"gain1": 1.0, "gain3": 3.0, "late": 3.0}[case]
    def rmsn(x):
        return gain * x / x.pow(2).mean(-1, keepdim=True).sqrt()
    L = E.lib()
    for r in (1, 3):
        q, k, v = bfr(rmsn(torch.randn(N, H, 64, generator=g))), bfr(rmsn(torch.randn(N, H, 64, generator=g))), bfr(torch.randn(N, H, 64, generator=g))
        if case == "late":      # head 0: queries along u, the rank's own keys along -u (scores ~ -|q||k'| = -140), the others ordinary
            u = torch.randn(64, generator=g); u = u / u.norm()
            q[:, 0] = bfr(28.0 * u + 0.5 * torch.randn(N, 64, generator=g))
            k[r * n:(r + 1) * n, 0] = bfr((-5.0 * u + 0.1 * torch.randn(n, 64, generator=g)) / O.SOFTMAX_C)
        kc = bfr(k * O.SOFTMAX_C)
        qloc = q[r * n:(r + 1) * n]
        qd, kd, kcd = qloc.reshape(n, -1).cuda().to(BF), k.reshape(N, -1).cuda().to(BF), kc.reshape(N, -1).cuda().to(BF)
        vt = v.reshape(N, -1).t().contiguous().cuda().to(BF)
        vt_chunks = vt.reshape(H * 64, P, n).permute(1, 0, 2).contiguous()
        ws = torch.empty(L.k5_nabla_workspace_size(H, nb), dtype=torch.uint8, device="cuda")
        E.check(L.k5_nabla_select_rect_local_bf16(qd.data_ptr(), kd.data_ptr(), qd.stride(0), kd.stride(0), H, n, r * (n // 64), N, T, Hb, Wb,
                                                  3, 1, 1, 0.5, ws.data_ptr(), r * (n // 64), n // 64, E.stream_ptr()))
        nqb = n // 64
        m = torch.empty(H, nqb, nb, dtype=torch.uint8, device="cuda")
        E.check(L.k5_nabla_mask_rect_u8(ws.data_ptr(), H, nqb, nb, m.data_ptr(), E.stream_ptr()))
        m = m.bool().cpu()
        assert m.any(-1).all()
        if case == "late":      # the scenario needs local blocks in head 0's lists (the STA window guarantees them)
            assert m[0, :, r * nqb:(r + 1) * nqb].any(-1).all()

        def run(passes):
            flags, kmax = _flags_rows(E, qloc, kc, H)
            assert flags.tolist() == [1, 1]
            o = torch.full((n, H * 64), float("nan"), dtype=BF, device="cuda")
            state = torch.zeros(L.k5_attention_state_size(H, n) // 4, device="cuda")
            for ps in passes:
                E.check(L.k5_attention_nabla_rect_prescaled_pass(qd.data_ptr(), kcd.data_ptr(), vt_chunks.data_ptr(), o.data_ptr(), H, n, N,
                                                                 qd.stride(0), kcd.stride(0), n, o.stride(0), ws.data_ptr(), n, H * 64 * n,
                                                                 flags.data_ptr(), kmax.data_ptr(), ps, state.data_ptr(), E.stream_ptr()))
                torch.cuda.synchronize()
                if ps == 1 and case == "late":
                    assert flags.tolist() == [2, 1], flags          # head 0 went late in the first pass
            return o, flags.tolist()
        one, f1 = run([0])
        two, f2 = run([1, 2])
        assert f1 == ([1, 1] if case != "late" else f1) and f2 == ([1, 1] if case != "late" else [2, 1]), (f1, f2)
        # oracle: softmax over the kept blocks of each 64-query row, exp2 domain on the pre-scaled keys
        mask = m.repeat_interleave(64, 1).repeat_interleave(64, 2)                  # [H][n][N]
        s = torch.einsum("qhd,khd->hqk", qloc, kc)
        s = s.masked_fill(~mask, float("-inf"))
        pr = torch.exp2(s - s.amax(-1, keepdim=True))
        ref = torch.einsum("hqk,khd->qhd", bfr(pr) / bfr(pr).sum(-1, keepdim=True), v).reshape(n, -1)
        R = parity.AttentionRef(qloc, kc, v, base2=True, block_mask=m)
        for name, got in (("one pass", one), ("two passes", two)):
            assert torch.isfinite(got.float()).all(), (case, r, name)
            err = (got.float().cpu() - ref).abs()
            assert err.max().item() <= 2e-2 + 2 ** -6 * ref.abs().max().item(), (case, r, name, err.max().item())
            R.close(got, parity.MARGIN_SPARSE, f"sparse list walk, {case}, rank {r}, {name}")
        assert (one.float() - two.float()).abs().max().item() <= 2e-2


@pytest.mark.parametrize("gain,anchor", [(1.0, 1), (3.0, 1), (6.0, 1), (6.0, 0)])
def test_lists_per_two_rows_give_the_same_bits(gain, anchor):
    """"nabla_group_rows" = 2: key-tile lists per TWO 64-query rows and 128-query attention workgroups instead of four / 256.  A
    64-query row attends its own kept blocks in ascending order either way (the other rows' blocks of the shared list are skipped),
    so the result must be BIT-identical to the default — at gain 1 (offset 0), gain 3 (per-row offsets) and gain 6 (bound 415 > 190: online
    form — the anchored offsets of the dense path are not used under NABLA, whatever "attn_anchor" says)."""
    from kandinsky.models.dit import DiffusionTransformer3D
    c = dict(O.LITE_2B, num_visual_blocks=2, num_text_blocks=1)
    sd = O.synthetic_state_dict(O.DitConfig(**c), seed=3)
    if gain != 1.0:
        for k in sd:
            if k.endswith(("query_norm.weight", "key_norm.weight")):
                sd[k] = sd[k] * gain
    g = torch.Generator().manual_seed(19)
    x = torch.randn(9, 16, 32, 16, generator=g)                      # 18 blocks of 64 tokens: an odd count of 128-query groups' rows
    text, pooled = torch.randn(37, 3584, generator=g), torch.randn(1, 768, generator=g)
    pos = [torch.arange(9), torch.arange(8), torch.arange(16)]
    t = torch.tensor([875.0])
    sp = {"P": 0.6, "wT": 3, "wH": 3, "wW": 3, "to_fractal": True}
    outs = []
    # 1 (round 4): one list per 64-query row, 64-query workgroups of two waves.  "nabla_pair_frames" (round 4, default 1): the two rows of a
    # 128-query list are the same spatial tile in adjacent frames (2 blocks per frame here: rows b and b + 2; 4 whole chunks of 4 rows and a
    # 2-row remainder that pairs adjacent rows) instead of rows 2g, 2g + 1 — a row still walks its own tiles in ascending order
    # "nabla_fuse_means" (round 4, default 1): the block means come out of the norm + RoPE pass and the keys are scaled in place; 0 = the means'
    # own pass over the stored unscaled tensor + a scaled key copy (rounds 1-3) — the same bits
    for grp, pair, fuse in ((4, 1, 2), (2, 1, 2), (2, 0, 2), (1, 1, 2), (4, 1, 0), (4, 1, 1)):   # fuse 2 = always (1 keeps small launches on the separate pass)
        d = DiffusionTransformer3D(**c)
        d.load_state_dict(sd, assign=True)
        d = d.to("cuda:0")
        d.engine("cuda:0")
        d.set_option("nabla_group_rows", grp)
        d.set_option("nabla_pair_frames", pair)
        d.set_option("nabla_fuse_means", fuse)
        d.set_option("attn_anchor", anchor)
        outs.append(d(x.cuda(), text.cuda(), pooled.cuda(), t, pos, torch.arange(37), scale_factor=(1.0, 2.0, 2.0), sparse_params=sp))
        n_fixed, n_online = d.attn_variant_counts()
        assert (n_online == 0) if gain <= 3.0 else (n_fixed == 0), (gain, grp, n_fixed, n_online)
        del d
    assert torch.isfinite(outs[0].float()).all()
    assert all(torch.equal(outs[0], o) for o in outs[1:])


def test_nabla_graph_captured_step_is_bit_identical(tiny_sd, golden, golden_meta):
    """NABLA through k5_dit_set_graph: the captured step contains the map kernels, the density-hint count and its device-to-pinned-host
    copy (buffers allocated at finalize, nothing inside the capture) — the replayed steps must equal the eager loop bit for bit (the
    hint only picks the attention workgroup size, which does not change the result)."""
    from kandinsky.config import Conf
    from kandinsky.generation_utils import generate
    from kandinsky.models.dit import DiffusionTransformer3D
    attn = golden_meta["nabla_attention"]
    conf = Conf({"model": {"dit_params": {"patch_size": [1, 2, 2]}, "attention": attn}, "metrics": {"scale_factor": [1.0, 2.0, 2.0]}})
    pos = [torch.arange(6), torch.arange(16), torch.arange(16)]
    te = {"text_embeds": golden["fwd.text"].cuda(), "pooled_embed": golden["fwd.pooled"].cuda()}
    ne = {"text_embeds": golden["gen.null_text"].cuda(), "pooled_embed": golden["gen.null_pooled"].cuda()}
    outs = []
    for graph in (False, True):
        dit = DiffusionTransformer3D(**dict(golden_meta["tiny_config"]))
        dit.load_state_dict(tiny_sd, assign=True)
        dit = dit.to("cuda:0")
        dit.engine("cuda:0")
        dit.set_graph(graph)
        outs.append(generate(dit, "cuda:0", (6, 32, 32, 16), 5, te, ne, pos, torch.arange(7), torch.arange(4), 2.0, 5.0, conf,
                             noise=golden["gen.nabla.noise"]))
        del dit
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def test_reference_nabla_golden_through_the_gpu_kernel(E):
    """The committed reference vector (oracle/gen_golden.py: nablaT_v2 itself, fp32, on fixed q / k with the (6,2,2) STA mask, P = 0.7)
    fed to k5_nabla_select_bf16 — entry by entry against the REFERENCE's mask, not the oracle's.  The kernel sees bf16 q / k and
    bf16 logits (the reference's GPU arithmetic under autocast), the golden is the fp32 evaluation: entries may only differ where
    the cumulative mass sits within a bf16 logit flip of the cut; the exact count is reported."""
    import json
    import os
    from safetensors.torch import load_file
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    G = load_file(os.path.join(here, "dit_tiny.safetensors"))
    meta = json.load(open(os.path.join(here, "dit_tiny_meta.json")))
    at = meta["nabla_attention"]
    q, k, ref = G["nabla.q"], G["nabla.k"], G["nabla.mask"].bool()       # (N, H, 64) fp32, (H, nb, nb)
    N, H, _ = q.shape
    T, Hp, Wp = meta["nabla_patched_shape"]
    grid, window = (T, Hp // 8, Wp // 8), (at["wT"], at["wH"], at["wW"])
    nb = N // 64
    assert tuple(ref.shape) == (H, nb, nb) and torch.equal(G["nabla.sta"].bool(), O.fast_sta(*grid, *window))
    ws = E.nabla_select(q.reshape(N, -1).cuda().to(BF), k.reshape(N, -1).cuda().to(BF), H, grid, window, at["P"])
    got = E.nabla_mask(ws, H, nb).cpu()
    diff = got != ref
    print(f"reference nabla.mask golden vs k5_nabla_select_bf16: {int(diff.sum())} of {diff.numel()} entries differ "
          f"(golden density {ref.float().mean():.3f}, kernel {got.float().mean():.3f})")
    ok = _may_differ(bfr(q), bfr(k), at["P"], 0.05) | _may_differ(q, k, at["P"], 0.05, mode="fp32")
    assert not (diff & ~ok).any(), (diff & ~ok).nonzero()[:5].tolist()
    assert int(diff.sum()) <= 12, int(diff.sum())                       # 1152 entries; a handful of rows have an entry within one bf16 flip of the cut
