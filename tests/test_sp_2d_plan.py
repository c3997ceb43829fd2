"""Two-level sequence parallelism ("sp_mode" = 2), CPU side.

k5_sp_plan_2d is the exchange plan every rank derives from (heads, ranks, rows_pad, dim): G = gcd(heads, ranks) head groups, ranks / G query
splits; k' and V^T go from every rank to every rank (the block of the receiver's head group), q and the attention output only inside a split.
Checked through ctypes: what a rank plans to receive from p is exactly what p plans to send to it, the blocks of a buffer do not overlap and stay
inside it, and the admissibility report (gather / Ulysses / two-level).  Then the schedule itself, restated on the oracle arithmetic by 4 gloo ranks
that move their data by the ENGINE's plan tables (tiny model: 2 heads, so G = 2, two splits), equals the single-process oracle forward."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import k5_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP_K, SP_VT, SP_Q, SP_O = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, os.path.join(ROOT, "kandinsky-5_amd"))
    import build as k5build
    k5build.build(verbose=False)
    from kandinsky import _engine as E
    return E.lib()


def plan(lib, H, P, rows_pad, D, which):
    """-> (mode, G, table[src][dst] = (send_off, recv_off, bytes))"""
    g = C.c_int(0)
    tab = (C.c_longlong * (3 * P * P))()
    mode = lib.k5_sp_plan_2d(H, P, rows_pad, D, which, C.byref(g), tab)
    assert mode >= 0, mode
    t = [[tuple(tab[3 * (s * P + d) + i] for i in range(3)) for d in range(P)] for s in range(P)]
    return mode, g.value, t


@pytest.mark.parametrize("H", [2, 24, 28])
def test_plan_is_consistent_for_every_rank_count(lib, H):
    D, rows_pad = H * 64, 192
    for P in range(2, 17):
        G = math.gcd(H, P)
        Dp, blk = D // G, rows_pad * (D // G) * 2
        send_size = {SP_K: G * blk, SP_VT: D * rows_pad * 2, SP_Q: G * blk, SP_O: G * blk}
        recv_size = {SP_K: P * blk, SP_VT: P * blk, SP_Q: G * blk, SP_O: G * blk}
        for which in (SP_K, SP_VT, SP_Q, SP_O):
            mode, g, t = plan(lib, H, P, rows_pad, D, which)
            assert g == G, (H, P, g)
            assert mode == (0 if G == 1 else 1 if G == P else 2), (H, P, mode)
            for dst in range(P):
                spans = []
                for src in range(P):
                    so, ro, nb = t[src][dst]
                    # the table is the ONE both sides read: src sends (so, nb) of its send buffer, dst receives it at ro — same entry, same size
                    if nb == 0:
                        continue
                    assert nb == blk, (H, P, which, src, dst, nb)
                    assert 0 <= so and so + nb <= send_size[which], (H, P, which, src, dst)
                    assert 0 <= ro and ro + nb <= recv_size[which], (H, P, which, src, dst)
                    if which in (SP_K, SP_VT):
                        assert so == (dst % G) * blk and ro == src * blk          # fan-out: the receiver's head group, token order
                    spans.append((ro, ro + nb))
                spans.sort()
                for a, b in zip(spans, spans[1:]):
                    assert a[1] <= b[0], (H, P, which, dst, spans)                # receive blocks do not overlap
                if which in (SP_K, SP_VT):
                    assert len(spans) == P                                        # every rank's rows of my head group arrive
                else:
                    assert len(spans) == G                                        # only from the G ranks of my split
                    for src in range(P):
                        assert (t[src][dst][2] > 0) == (src // G == dst // G)
            # bytes a rank pulls from its peers: the per-rank ingress of DESIGN.md §6
            ingress = sum(t[s][0][2] for s in range(1, P))
            assert ingress == ((P - 1) if which in (SP_K, SP_VT) else (G - 1)) * blk


def test_plan_rejects_bad_arguments(lib):
    g = C.c_int(0)
    assert lib.k5_sp_plan_2d(28, 8, 576, 1790, SP_K, C.byref(g), None) < 0   # dim not a multiple of heads
    assert lib.k5_sp_plan_2d(28, 8, 576, 1792, 4, C.byref(g), None) < 0      # no such exchange
    assert lib.k5_sp_plan_2d(28, 0, 576, 1792, SP_K, C.byref(g), None) < 0
    assert lib.k5_sp_plan_2d(28, 8, 576, 1792, SP_Q, C.byref(g), None) == 2 and g.value == 4   # the headline case: 4 groups of 7 heads x 2 splits
    assert lib.k5_sp_plan_2d(28, 6, 576, 1792, SP_Q, C.byref(g), None) == 2 and g.value == 2


# ------------------------------------------------------------------------------------------------ the schedule on the oracle, 4 gloo ranks
def _exchange(send, tabs, rank, world, recv_elems):
    """the engine's planned exchange (Comm::exchange) on flat fp32 buffers whose offsets are counted in bf16 elements of the plan: every rank
    gathers every send buffer (gloo) and keeps exactly the spans the plan addresses to it"""
    mine = send.reshape(-1)
    sizes = [torch.zeros(1, dtype=torch.long) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([mine.numel()]))
    n = int(max(s.item() for s in sizes))
    pad = torch.zeros(n)
    pad[:mine.numel()] = mine
    everyone = [torch.empty(n) for _ in range(world)]
    dist.all_gather(everyone, pad)
    recv = torch.full((recv_elems,), float("nan"))
    for p in range(world):
        so, ro, nb = tabs[p][rank]
        so, ro, ne = so // 2, ro // 2, nb // 2
        recv[ro:ro + ne] = everyone[p][so:so + ne]
    return recv


def _sp2d_forward(sd, cfg, x, text, pooled, time, vpos, tpos, rank, world, tabs):
    from kandinsky.models.parallelize import shard_slot, token_shard
    mode = "fp32"
    txt = O.text_embeddings(sd, "text_embeddings", text, mode)
    temb = O.time_embeddings(sd, time, cfg) + O.text_embeddings(sd, "pooled_text_embeddings", pooled, mode)
    vis = O.visual_embeddings(sd, x, cfg, mode)
    ta = O.rope_1d_args(tpos, cfg.head_dim)
    for i in range(cfg.num_text_blocks):
        txt = O.encoder_block(sd, f"text_transformer_blocks.{i}", txt, temb, torch.cos(ta), torch.sin(ta), cfg, mode)
    Tp, Hp, Wp, D = vis.shape
    va = O.rope_3d_args((Tp, Hp, Wp), vpos, cfg.axes_dims, (1.0, 2.0, 2.0)).reshape(-1, 32)
    N = Tp * Hp * Wp
    t0, n = token_shard(N, world, rank)
    slot = shard_slot(N, world)
    vis = vis.reshape(N, D)[t0:t0 + n]
    cos, sin = torch.cos(va)[t0:t0 + n], torch.sin(va)[t0:t0 + n]
    H = cfg.num_heads
    G = math.gcd(H, world)
    Hg, Dp, g, s = H // G, D // G, rank % G, rank // G
    q0 = s * G * slot
    Ms = min(N, q0 + G * slot) - q0
    for i in range(cfg.num_visual_blocks):
        p = f"visual_transformer_blocks.{i}"
        mod = O.modulation(sd, f"{p}.visual_modulation", temb)
        sa, ca, ff = torch.chunk(mod, 3, dim=-1)
        shift, scale, gate = torch.chunk(sa, 3, dim=-1)
        h = O.scale_shift_norm(vis, scale, shift, mode)
        q, k, v = O._attn_qkv(sd, f"{p}.self_attention", h, h, mode, H)
        q, k = O.apply_rotary(q, cos, sin, mode), O.apply_rotary(k, cos, sin, mode)

        def planes(t):   # (n, H, 64) -> send planes [G][slot][Dp] (block = head group), sp2d_pack_qk
            pl = torch.zeros(G, slot, Dp)
            pl[:, :n] = t.reshape(n, G, Dp).permute(1, 0, 2)
            return pl
        kall = _exchange(planes(k), tabs[SP_K], rank, world, world * slot * Dp).reshape(world * slot, Hg, 64)[:N]
        vt = torch.zeros(D, slot)
        vt[:, :n] = v.reshape(n, D).t()                          # V^T as the GEMM writes it: rows g Dp .. = head group g
        vr = _exchange(vt, tabs[SP_VT], rank, world, world * slot * Dp).reshape(world, Dp, slot)
        vall = vr.permute(0, 2, 1).reshape(world * slot, Hg, 64)[:N]
        qs = _exchange(planes(q), tabs[SP_Q], rank, world, G * slot * Dp).reshape(G * slot, Hg, 64)[:Ms]
        osp = O.sdpa(qs, kall, vall, mode).reshape(Ms, Dp)      # the split's rows, my head group, all N keys
        opad = torch.zeros(G * slot, Dp)
        opad[:Ms] = osp
        orecv = _exchange(opad, tabs[SP_O], rank, world, G * slot * Dp).reshape(G, slot, Dp)
        o = orecv[:, :n].permute(1, 0, 2).reshape(n, D)          # ulysses_unpack_o with G head groups
        o = O._linear(o, sd[f"{p}.self_attention.out_layer.weight"], sd[f"{p}.self_attention.out_layer.bias"], mode)
        vis = O.gate_sum(vis, o, gate, mode)
        shift, scale, gate = torch.chunk(ca, 3, dim=-1)
        vis = O.gate_sum(vis, O.cross_attention(sd, f"{p}.cross_attention", O.scale_shift_norm(vis, scale, shift, mode),
                                                txt, cfg, mode), gate, mode)
        shift, scale, gate = torch.chunk(ff, 3, dim=-1)
        vis = O.gate_sum(vis, O.feed_forward(sd, f"{p}.feed_forward", O.scale_shift_norm(vis, scale, shift, mode), mode),
                         gate, mode)
    y = O.out_layer(sd, vis, temb, cfg, mode)
    ypad = torch.zeros(slot, y.shape[1])
    ypad[:n] = y
    yall = [torch.empty_like(ypad) for _ in range(world)]
    dist.all_gather(yall, ypad)
    return O.unpatchify(torch.cat(yall, 0)[:N].reshape(Tp, Hp, Wp, -1), cfg.patch_size)


def _worker(rank, world, port, q, T, tabs):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "kandinsky-5_amd"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    cfg = O.DitConfig(in_visual_dim=16, in_text_dim=96, in_text_dim2=48, time_dim=64, out_visual_dim=16,
                      patch_size=(1, 2, 2), model_dim=128, ff_dim=256, num_text_blocks=1, num_visual_blocks=2,
                      axes_dims=(16, 24, 24), visual_cond=True)
    sd = O.synthetic_state_dict(cfg, seed=5, std=0.05)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(T, 16, 16, 33, generator=g)
    text, pooled = torch.randn(9, 96, generator=g), torch.randn(1, 48, generator=g)
    t = torch.tensor([432.0])
    vpos = [torch.arange(T), torch.arange(8), torch.arange(8)]
    out = _sp2d_forward(sd, cfg, x, text, pooled, t, vpos, torch.arange(9), rank, world, tabs)
    ref = O.dit_forward(sd, cfg, x, text, pooled, t, vpos, torch.arange(9), (1.0, 2.0, 2.0), None, "fp32")
    q.put((rank, float((out - ref).abs().max()), float(ref.abs().max()), bool(torch.isfinite(out).all())))
    dist.destroy_process_group()


@pytest.mark.parametrize("T", [4, 7])
def test_two_level_schedule_four_ranks_gloo(lib, T):
    """4 ranks on the tiny model (2 heads): G = 2 head groups x 2 query splits.  T = 4: 4 blocks of 64 tokens, one per rank; T = 7: 7 blocks,
    2 + 2 + 2 + 1 — the last rank's shard is short, so the last split's query range and the last key chunk are short."""
    from kandinsky.models.parallelize import shard_slot
    world = 4
    N = T * 64
    slot = shard_slot(N, world)
    tabs = [plan(lib, 2, world, slot, 128, w)[2] for w in (SP_K, SP_VT, SP_Q, SP_O)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000) + T
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, T, tabs)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(60)
    assert sorted(r[0] for r in res) == list(range(world))
    for rank, err, scale, finite in res:
        assert finite, rank
        assert err <= 1e-5 * max(scale, 1.0), (rank, err, scale)
