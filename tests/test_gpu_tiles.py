"""Spatial context windows (tiles) on the MI355X: the 3-D blend + CFG + Euler kernel and the view patchify bit for bit against torch and
against the existing entries, k5_sample_tiles against the same forwards issued step by step, parity with the oracle and the reference golden,
locality, refusals, and the pipeline end to end.

Tolerances are those of tests/test_gpu_windows.py: a final latent within relative L2 1e-2 of the bf16-island oracle, composed here over the same
plan, and 3e-2 of the reference's fp32 golden (tools/gen_golden_tiles.py).  Everything that claims "the same computation" is asserted bit for
bit."""
import json
import os
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
import kit  # noqa: E402
from kit import BF, GOLDEN, POS, Wrapped, cfg, f32, make_dit, prompts, rel, tiny_dit  # noqa: E402
from test_gpu_windows import _tiny_pipeline, other_prompt  # noqa: E402

WINDOW = (3, 8, 12)
CASES = ("s14", "s22", "t2s2")


@pytest.fixture(scope="module")
def tile_golden():
    from safetensors.torch import load_file
    return dict(load_file(os.path.join(GOLDEN, "dit_tiny_tiles.safetensors"))), json.load(open(os.path.join(GOLDEN, "dit_tiny_tiles_meta.json")))


def run_generate(model, golden, noise, w, steps=4, pos=None, **kw):
    return kit.run_generate(model, golden, w, steps=steps, shape=tuple(noise.shape), pos=pos or POS, noise=noise, **kw)


def tile_kw(meta, tag):
    ot, oh, ow = meta["cases"][tag]["overlap"]
    return dict(context_frames=WINDOW[0], context_overlap=ot, context_height=WINDOW[1], context_width=WINDOW[2], context_overlap_hw=(oh, ow))


def run_tiles(model, golden, tile_golden, tag, w, noise=None, **kw):
    g, meta = tile_golden
    return run_generate(model, golden, g[f"tile.{tag}.noise"] if noise is None else noise, w, **tile_kw(meta, tag), **kw)


def index_of(plan, k):
    _, ny, nx = plan.counts
    return k // (ny * nx), (k // nx) % ny, k % nx


# ------------------------------------------------------------------------------------------ kernels
def tiles_ref(img, c, u, w, dt, plan, tabs):
    """the torch expression the kernel is held to: v per window as eager bf16 ops; the share (wt * wy) * wx, its product with v and every sum
    of the blend an fp32 op of its own, in window order.  img (T, H, W, C); c / u (nwin, Ft, Fh, Fw, C); the tables fp32 on the device"""
    wt, wy, wx = tabs.weights
    acc = torch.zeros_like(img)
    seen = torch.zeros(img.shape[:3], dtype=torch.bool, device=img.device)
    for k in range(plan.nwin):
        it, iy, ix = index_of(plan, k)
        box = plan.box(k)
        v = c[k] if u is None else u[k] + w * (c[k] - u[k])
        share = (wt[it][:, None, None] * wy[iy][None, :, None]) * wx[ix][None, None, :]
        p = share[..., None] * v.float()
        acc[box] = torch.where(seen[box][..., None], acc[box] + p, p)
        seen[box] = True
    assert seen.all()
    return img + (dt * acc).to(BF).float()


def padded(shape, g, pad=64):
    """a bf16 tensor of `shape` with NaN in front of it and behind it"""
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + 2 * pad,), float("nan"), dtype=BF, device="cuda")
    t = buf[pad:pad + n].view(*shape)
    t.copy_(torch.randn(*shape, generator=g).to(BF))
    return t


@pytest.mark.parametrize("plan", [((4, 10, 14), (3, 6, 8), (2, 2, 4)), ((3, 8, 16), (3, 8, 8), (0, 0, 6))])
@pytest.mark.parametrize("C", [16, 3])            # a lane owns four channels of a cell / the scalar path
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_cfg_euler_tiles_bit_exact(plan, C, w):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import tile_windows
    p = tile_windows(*plan)
    T, H, W = p.clip
    g = torch.Generator().manual_seed(T * H * W + C + int(w))
    img = torch.randn(T, H, W, C, generator=g).cuda()
    c = padded((p.nwin,) + p.window + (C,), g)
    u = padded((p.nwin,) + p.window + (C,), g) if w != 1.0 else None
    dt = f32(-0.0625 * 1.3)
    tabs = E.tile_tables(p, "cuda")
    want = tiles_ref(img, c, u, w, dt, p, tabs)
    n = img.numel()
    buf = torch.full((n + 64,), 7.0, device="cuda")                       # a guard region after the latent
    buf[:n] = img.view(-1)
    E.cfg_euler_tiles_(buf[:n].view(T, H, W, C), c, u, w, dt, tabs)
    torch.cuda.synchronize()
    assert torch.isfinite(buf).all()                                        # none of the NaN around the velocities was read
    assert torch.equal(buf[:n].view(T, H, W, C), want)
    assert (buf[n:] == 7.0).all()


@pytest.mark.parametrize("C", [16, 3])
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_a_temporal_plan_is_k5_cfg_euler_windows(C, w):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import context_windows
    T, F, H, W = 7, 3, 4, 6
    starts, weights = context_windows(T, F, 2)
    g = torch.Generator().manual_seed(C + int(w))
    img = torch.randn(T, H, W, C, generator=g).cuda()
    c = torch.randn(len(starts), F, H, W, C, generator=g).cuda().to(BF)
    u = torch.randn(len(starts), F, H, W, C, generator=g).cuda().to(BF) if w != 1.0 else None
    dt = f32(-0.21)
    tabs = E.tile_tables(NS(starts=(starts, [0], [0]), weights=(weights, torch.ones(1, H), torch.ones(1, W))), "cuda")
    a, b = img.clone(), img.clone()
    E.cfg_euler_windows_(a, c, u, w, dt, *E.window_tables(starts, weights, "cuda"))
    E.cfg_euler_tiles_(b, c, u, w, dt, tabs)
    assert torch.equal(a, b) and not torch.equal(a, img)


@pytest.mark.parametrize("C", [16, 3])
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_one_window_of_weight_one_is_k5_cfg_euler(C, w):
    from kandinsky import _engine as E
    T, H, W = 3, 6, 10
    g = torch.Generator().manual_seed(C + int(w))
    img = torch.randn(T, H, W, C, generator=g).cuda()
    c = torch.randn(1, T, H, W, C, generator=g).cuda().to(BF)
    u = torch.randn(1, T, H, W, C, generator=g).cuda().to(BF) if w != 1.0 else None
    dt = f32(-0.21)
    tabs = E.tile_tables(NS(starts=([0], [0], [0]), weights=(torch.ones(1, T), torch.ones(1, H), torch.ones(1, W))), "cuda")
    plain, tiled = img.clone(), img.clone()
    E.cfg_euler_(plain, c, u, w, dt)
    E.cfg_euler_tiles_(tiled, c, u, w, dt, tabs)
    assert torch.equal(tiled, plain)


def test_kernel_entry_refusals():
    from kandinsky import _engine as E
    from kandinsky.generation_utils import tile_windows
    L = E.lib()
    p = tile_windows((3, 8, 16), (3, 8, 8), (0, 0, 4))                      # columns 0, 4, 8
    img = torch.zeros(3, 8, 16, 4, device="cuda")
    c = torch.zeros(p.nwin, 3, 8, 8, 4, dtype=BF, device="cuda")
    tabs = E.tile_tables(p, "cuda")

    def call(tabs=tabs, img=img, c=c, shape=(3, 8, 16, 4), plan=True):
        import ctypes
        return L.k5_cfg_euler_tiles(E.ptr(img), E.ptr(c), None, 1.0, 0.1, ctypes.byref(tabs.plan) if plan else None, *shape, E.stream_ptr())

    assert call() == 0
    assert call(img=None) == 1 and call(c=None) == 1 and call(plan=False) == 1
    assert call(shape=(3, 8, 12, 4)) == 1 and b"reaches outside" in L.k5_last_error()       # the last window would end at column 15 of 12
    assert call(shape=(3, 8, 18, 4)) == 1 and b"covers 16" in L.k5_last_error()
    bare = E.tile_tables(NS(starts=([0], [0], [0, 10]), weights=(torch.ones(1, 3), torch.ones(1, 8), torch.ones(2, 8))), "cuda")
    assert call(tabs=bare, shape=(3, 8, 18, 4)) == 1 and b"covers 8" in L.k5_last_error()
    many = E.tile_tables(NS(starts=([0], list(range(9)), list(range(9))), weights=(torch.ones(1, 3), torch.ones(9, 8), torch.ones(9, 8))), "cuda")
    assert call(tabs=many) == 1 and b"nwin must be" in L.k5_last_error()
    x = torch.zeros(2, 4, 6, 16, device="cuda")
    out = torch.zeros(2 * 2 * 3, 64, dtype=BF, device="cuda")

    def patch(x_=x, fs=4 * 6 * 16, rs=6 * 16, T=2, H=4, W=6):
        return L.k5_patchify_view_bf16(E.ptr(x_), fs, rs, None, 0, 0, out.data_ptr(), T, H, W, 16, 16, 64, None, E.stream_ptr())

    assert patch() == 0
    assert patch(x_=None) == 1 and patch(T=0) == 1 and patch(H=3) == 1 and patch(W=5) == 1
    assert patch(rs=6 * 16 - 1) == 1 and patch(fs=4 * 6 * 16 - 1) == 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_cond", [False, True])
@pytest.mark.parametrize("with_perm", [False, True])
def test_patchify_view_equals_the_compact_kernels_on_a_copy(with_cond, with_perm):
    from kandinsky import _engine as E
    L = E.lib()
    g = torch.Generator().manual_seed(5)
    Cx, T, H, W, Kpad = 16, 2, 6, 8, 160
    Cin = 2 * Cx + 1
    box = (slice(1, 1 + T), slice(2, 2 + H), slice(4, 4 + W))              # a non-zero frame, row and column
    parent = torch.full((4, 10, 14, Cx), float("nan")).cuda()
    parent[box] = torch.randn(T, H, W, Cx, generator=g).cuda()
    vparent = torch.full((4, 10, 14, Cx + 1), float("nan")).cuda()
    vparent[box] = torch.randn(T, H, W, Cx + 1, generator=g).cuda()
    ntok = T * (H // 2) * (W // 2)
    perm = torch.randperm(ntok, generator=g).to(torch.int32).cuda() if with_perm else None
    xv, vv = parent[box], vparent[box] if with_cond else None
    assert not xv.is_contiguous()
    got = E.patchify_view_(xv, vv, Cin, Kpad, tok_perm=perm)
    want, compact = torch.empty_like(got), torch.empty_like(got)
    xc = xv.contiguous()
    if with_cond:
        vc = vv.contiguous()
        E.check(L.k5_patchify_cond_bf16(xc.data_ptr(), vc.data_ptr(), want.data_ptr(), T, H, W, Cx, Cin, Kpad, E.ptr(perm), E.stream_ptr()), "cond")
        compact = E.patchify_view_(xc, vc, Cin, Kpad, tok_perm=perm)
    else:
        E.check(L.k5_patchify_bf16(xc.data_ptr(), want.data_ptr(), T, H, W, Cx, Cin, Kpad, E.ptr(perm), E.stream_ptr()), "plain")
        compact = E.patchify_view_(xc, None, Cin, Kpad, tok_perm=perm)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()                                # nothing outside the view was read
    assert torch.equal(got, want) and torch.equal(compact, want)
    assert got.float().abs().sum() > 0


# ------------------------------------------------------------------------------------------ sampler: same bits
@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_fused_equals_step_by_step(tiny_dit, golden, tile_golden, tag, w):
    a = run_tiles(tiny_dit, golden, tile_golden, tag, w)
    b = run_tiles(Wrapped(tiny_dit), golden, tile_golden, tag, w)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert not torch.equal(a.cpu(), tile_golden[0][f"tile.{tag}.noise"])


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_a_tile_as_large_as_the_frame_is_the_plain_run(tiny_dit, golden, w):
    noise = golden["gen.noise"]                                             # (3, 8, 12, 16)
    plain = run_generate(tiny_dit, golden, noise, w)
    assert torch.equal(run_generate(tiny_dit, golden, noise, w, context_height=8, context_width=12), plain)
    assert torch.equal(run_generate(tiny_dit, golden, noise, w, context_height=16, context_width=24, context_overlap_hw=4), plain)
    assert torch.equal(run_generate(Wrapped(tiny_dit), golden, noise, w, context_height=8, context_width=12, context_overlap_hw=(2, 4)), plain)


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_a_temporal_plan_through_the_new_keywords_is_context_frames(tiny_dit, golden, w):
    noise = torch.randn(6, 8, 12, 16, generator=torch.Generator().manual_seed(606))
    want = run_generate(tiny_dit, golden, noise, w, context_frames=3, context_overlap=1)
    assert torch.equal(run_generate(tiny_dit, golden, noise, w, context_frames=3, context_overlap=1, context_height=8, context_width=12), want)
    assert torch.equal(run_generate(tiny_dit, golden, noise, w, context_frames=3, context_overlap=1, context_height=8), want)


def test_the_engine_entry_with_a_temporal_plan_is_k5_sample_windows(tiny_dit, golden):
    from kandinsky.generation_utils import sigma_schedule, tile_windows
    te, ne = prompts(golden)
    noise = torch.randn(6, 8, 12, 16, generator=torch.Generator().manual_seed(606))
    p = tile_windows((6, 8, 12), WINDOW, (1, 0, 0))
    assert p.counts == (3, 1, 1)
    lat = noise.cuda().contiguous()
    tiny_dit.sample(lat, sigma_schedule(4, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0), tiles=p)
    assert torch.equal(lat, run_generate(tiny_dit, golden, noise, 5.0, context_frames=3, context_overlap=1))


def test_fused_equals_step_by_step_with_a_prompt_per_window(tiny_dit, golden, tile_golden):
    te, _ = prompts(golden)
    tb = other_prompt(golden)
    text = [(te, torch.arange(7)), (tb, torch.arange(5)), (te, torch.arange(7)), (tb, torch.arange(5))]
    a = run_tiles(tiny_dit, golden, tile_golden, "s22", 5.0, context_text=text)
    b = run_tiles(Wrapped(tiny_dit), golden, tile_golden, "s22", 5.0, context_text=text)
    assert torch.equal(a, b)
    assert not torch.equal(a, run_tiles(tiny_dit, golden, tile_golden, "s22", 5.0))
    with pytest.raises(ValueError, match="nwin = 4"):
        run_tiles(tiny_dit, golden, tile_golden, "s22", 5.0, context_text=text[:2])


def test_visual_cond_through_tiles(tiny_dit, golden, tile_golden):
    clip = tuple(tile_golden[1]["cases"]["t2s2"]["clip"])
    g = torch.Generator().manual_seed(11)
    vc, vm = torch.zeros(*clip, 16), torch.zeros(*clip, 1)
    vc[0], vm[0] = torch.randn(*clip[1:], 16, generator=g), 1.0             # image-to-video: the whole first frame, every window sees its slice
    for w in (1.0, 5.0):
        a = run_tiles(tiny_dit, golden, tile_golden, "t2s2", w, visual_cond=vc, visual_cond_mask=vm)
        b = run_tiles(Wrapped(tiny_dit), golden, tile_golden, "t2s2", w, visual_cond=vc, visual_cond_mask=vm)
        assert torch.equal(a, b)
        assert not torch.equal(a, run_tiles(tiny_dit, golden, tile_golden, "t2s2", w))


def test_nag_and_enhance_work_through_tiles(tiny_dit, golden, tile_golden):
    _, ne = prompts(golden)
    plain = run_tiles(tiny_dit, golden, tile_golden, "t2s2", 5.0)
    nb, nwin = tiny_dit.num_visual_blocks, 4
    # Enhance-A-Video: T is the window's; every forward of every window carries the score and scale launches
    tiny_dit.enhance_state(reset=True)
    out = run_tiles(tiny_dit, golden, tile_golden, "t2s2", 5.0, enhance_weight=4.0)
    assert tiny_dit.enhance_state(reset=True)[1] == 4 * nwin * 2 * nb       # steps x windows x forwards x blocks
    assert torch.isfinite(out).all() and not torch.equal(out, plain)
    from test_gpu_enhance import Wrapped as WrappedWithEnhance            # a wrapped model that hands the setting on
    assert torch.equal(out, run_tiles(WrappedWithEnhance(tiny_dit), golden, tile_golden, "t2s2", 5.0, enhance_weight=4.0))
    # NAG: one negative prompt for every window's conditional forward
    kw = dict(nag_text_embeds=ne, nag_text_rope_pos=torch.arange(4), nag_scale=5.0, nag_tau=2.5, nag_alpha=0.25)
    tiny_dit.nag_state(reset=True)
    guided = run_tiles(tiny_dit, golden, tile_golden, "t2s2", 5.0, **kw)
    assert tiny_dit.nag_state(reset=True) == (False, 4 * nwin * nb)
    assert torch.isfinite(guided).all() and not torch.equal(guided, plain)


def test_a_change_stays_inside_the_windows_that_see_it(tiny_dit, golden, tile_golden):
    """Case s14 after ONE step: columns 20 .. 23 lie in the last window alone (columns 12 .. 23), so noise changed there moves the output only
    inside that window's box; no single forward over the whole frame would keep the change local."""
    noise = tile_golden[0]["tile.s14.noise"]
    other = noise.clone()
    other[:, :, 20:24] = torch.randn(3, 8, 4, 16, generator=torch.Generator().manual_seed(3))
    a = run_tiles(tiny_dit, golden, tile_golden, "s14", 5.0, steps=1)
    b = run_tiles(tiny_dit, golden, tile_golden, "s14", 5.0, steps=1, noise=other)
    assert torch.equal(a[:, :, :12], b[:, :, :12])
    assert not torch.equal(a[:, :, 12:16], b[:, :, 12:16]) and not torch.equal(a[:, :, 20:], b[:, :, 20:])
    pos = [torch.arange(3), torch.arange(4), torch.arange(12)]
    fa, fb = (run_generate(tiny_dit, golden, n, 5.0, steps=1, pos=pos) for n in (noise, other))
    assert not torch.equal(fa[:, :, :12], fb[:, :, :12])


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_the_tiles_matter(tiny_dit, golden, tile_golden, w):
    noise = tile_golden[0]["tile.s22.noise"]
    tiled = run_tiles(tiny_dit, golden, tile_golden, "s22", w)
    full = run_generate(tiny_dit, golden, noise, w, pos=[torch.arange(3), torch.arange(6), torch.arange(10)])   # one forward over the whole frame
    assert torch.isfinite(full).all()
    assert not torch.equal(tiled, full)
    assert rel(tiled, full) > 1e-3, rel(tiled, full)


# ------------------------------------------------------------------------------------------ parity
def oracle_tiles(sd, cfg, noise, plan, steps, w, s, te, ne, mode):
    """the tiled loop written around the oracle's get_velocity (conditioning channels zero, as the reference's loop has them)"""
    sig = O.sigma_schedule(steps, s)
    wt, wy, wx = plan.weights
    zeros = torch.zeros(*plan.window, noise.shape[-1]), torch.zeros(*plan.window, 1)
    img = noise.clone()
    for i in range(steps):
        acc = torch.zeros_like(img)
        for k in range(plan.nwin):
            it, iy, ix = index_of(plan, k)
            box = plan.box(k)
            v = O.get_velocity(sd, cfg, torch.cat([img[box], *zeros], -1), sig[i].unsqueeze(0), te, ne, POS, torch.arange(7), torch.arange(4), w,
                               (1.0, 2.0, 2.0), None, mode)
            share = wt[it][:, None, None] * wy[iy][None, :, None] * wx[ix][None, None, :]
            acc[box] += share[..., None] * v.float()
        img = img + O._r((sig[i + 1] - sig[i]) * acc, mode)
    return img


@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_parity_with_the_oracle_and_the_reference_golden(tiny_dit, tiny_sd, cfg, golden, tile_golden, tag, w):
    """Measured on the MI355X, engine vs bf16 oracle / vs reference golden: s14 w=1 1.52e-3 / 2.35e-3, s22 w=1 1.60e-3 / 2.42e-3,
    t2s2 w=1 1.66e-3 / 2.45e-3, s14 w=5 5.32e-3 / 6.97e-3, s22 w=5 5.96e-3 / 7.31e-3, t2s2 w=5 6.08e-3 / 7.35e-3.  The bounds stay the
    project's fixed ones (1e-2 / 3e-2)."""
    from kandinsky.generation_utils import tile_windows
    g, meta = tile_golden
    case = meta["cases"][tag]
    plan = tile_windows(case["clip"], meta["window"], case["overlap"])
    assert [list(s) for s in plan.starts] == case["starts"]
    assert all(torch.equal(a, g[f"tile.{tag}.{n}"]) for a, n in zip(plan.weights, ("wt", "wy", "wx")))
    out = run_tiles(tiny_dit, golden, tile_golden, tag, w, steps=meta["steps"])
    te, ne = prompts(golden)
    tec, nec = {k: v.cpu() for k, v in te.items()}, {k: v.cpu() for k, v in ne.items()}
    ref16 = oracle_tiles(tiny_sd, O.DitConfig(**cfg), g[f"tile.{tag}.noise"], plan, meta["steps"], w, meta["scheduler_scale"], tec, nec, "bf16")
    r16, r32 = rel(out, ref16), rel(out, g[f"tile.{tag}.{w}.final"])
    print(f"tiles {tag} w={w}: engine vs bf16 oracle {r16:.3e}, vs reference golden {r32:.3e}")
    assert r16 <= 1e-2, r16
    assert r32 <= 3e-2, r32


# ------------------------------------------------------------------------------------------ watch, refusals
def test_progress_and_cancel(tiny_dit, golden, tile_golden):
    from kandinsky.models.dit import SamplingInterrupted
    seen = []
    out = run_tiles(tiny_dit, golden, tile_golden, "s22", 5.0, callback=lambda info: seen.append((info.step, info.num_steps, info.preview)) and False)
    assert seen == [(i, 4, None) for i in range(4)]
    assert torch.equal(out, run_tiles(tiny_dit, golden, tile_golden, "s22", 5.0))
    with pytest.raises(SamplingInterrupted) as e:
        run_tiles(tiny_dit, golden, tile_golden, "s22", 5.0, callback=lambda info: info.step == 0)
    assert 1 <= e.value.steps_done <= 2                                     # the engine runs one step ahead of the callback
    with pytest.raises(ValueError, match="preview_every"):
        run_tiles(tiny_dit, golden, tile_golden, "s22", 5.0, callback=lambda info: False, preview_every=1, preview_factors=(torch.zeros(16, 3), None))
    assert tiny_dit._watch is None


def test_refusals_touch_nothing(tiny_dit, cfg, tiny_sd, golden, tile_golden):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule, tile_windows
    from kandinsky.magcache_utils import disable_magcache, set_magcache_params
    te, ne = prompts(golden)
    g, meta = tile_golden
    noise = g["tile.s22.noise"]
    plain = run_tiles(tiny_dit, golden, tile_golden, "s22", 5.0)
    sig = sigma_schedule(4, 5.0).tolist()
    good = tile_windows((3, 12, 20), WINDOW, (0, 4, 4))
    lat = noise.cuda().contiguous()
    before = lat.clone()

    def call(d, tiles=good, **kw):
        return d.sample(lat, sig, te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0), tiles=tiles, **kw)

    def refused(d, match, **kw):
        with pytest.raises(RuntimeError, match=match):
            call(d, **kw)
        torch.cuda.synchronize()
        assert torch.equal(lat, before)

    def with_starts(sy, sx):
        wy, wx = torch.ones(len(sy), 8), torch.ones(len(sx), 12)
        return NS(clip=good.clip, window=good.window, starts=([0], sy, sx), weights=(good.weights[0], wy, wx))

    # plans: a column without a window, starts that do not ascend, a window past the edge, a window off the patch grid, too many windows
    refused(tiny_dit, "no column window covers 12", tiles=with_starts([0, 4], [0]))
    refused(tiny_dit, "no row window covers 8", tiles=with_starts([0], [0, 8]))
    refused(tiny_dit, "must ascend", tiles=with_starts([0, 0], [0, 8]))
    refused(tiny_dit, "reaches outside", tiles=with_starts([0, 6], [0, 8]))
    refused(tiny_dit, "start on a patch", tiles=with_starts([0, 3, 4], [0, 8]))
    refused(tiny_dit, "nwin must be", tiles=with_starts([0, 2, 4], list(range(0, 44, 2))))
    with pytest.raises(ValueError, match="tiles together with edit"):
        call(tiny_dit, edit=(lat, lat, None))
    # a watch with previews (installed on the handle itself, past generate's own check)
    tiny_dit.set_watch(lambda info: False, preview_every=1, rgb_factors=torch.zeros(16, 3))
    try:
        refused(tiny_dit, "previews")
    finally:
        tiny_dit.clear_watch()
    # MagCache, and a sequence-parallel group, on handles of their own
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    mag = make_dit(cfg, tiny_sd)
    mag.engine("cuda:0")
    set_magcache_params(mag, c["ratios"], c["num_steps"], c["no_cfg"])
    refused(mag, "MagCache")
    disable_magcache(mag)
    sp = make_dit(cfg, tiny_sd)
    sp.engine("cuda:0")
    sp.enable_sequence_parallel(0, 1, device="cuda:0")
    refused(sp, "sequence-parallel")
    del sp
    # the handles work afterwards
    out = call(mag)
    assert out is lat and torch.equal(lat, plain)
    lat.copy_(before)
    assert torch.equal(call(tiny_dit), plain)
    # graph replay on: the tiled call runs eagerly, the same bits
    gr = make_dit(cfg, tiny_sd)
    gr.engine("cuda:0")
    gr.set_graph(True)
    lat.copy_(before)
    assert torch.equal(call(gr), plain)
    # NULL arguments at the C entry
    assert E.lib().k5_sample_tiles(tiny_dit.engine(lat.device), None, None, E.stream_ptr()) == 1


def test_the_engine_refuses_every_handle_setting_the_windows_refuse(tiny_dit, cfg, tiny_sd, golden, tile_golden):
    """k5_sample_tiles itself (past generate's own checks): each setting is installed on the handle, the call returns its error under the entry's
    own name with nothing enqueued, and the handle gives the plain tiled run's bits afterwards.  Editing and FlowEdit have no argument at this
    entry (k5_sample_edit / k5_sample_flowedit are entries of their own): `sample(tiles=, edit= / flowedit=)` is a ValueError, tested above and
    in tests/test_tiles_host.py."""
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule, stochastic_plan, tile_windows
    from kandinsky.magcache_utils import start_magcache_calibration, stop_magcache_calibration
    K5_ERR_STATE = 4
    te, ne = prompts(golden)
    plain = run_tiles(tiny_dit, golden, tile_golden, "s22", 5.0)
    sig = sigma_schedule(4, 5.0).tolist()
    good = tile_windows((3, 12, 20), WINDOW, (0, 4, 4))
    lat = tile_golden[0]["tile.s22.noise"].cuda().contiguous()
    before = lat.clone()

    def call(d):
        return d.sample(lat, sig, te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0), tiles=good)

    def refused(d, word):
        with pytest.raises(RuntimeError, match=f"k5_sample_tiles failed with status {K5_ERR_STATE}: k5_sample_tiles: ") as e:
            call(d)
        assert word in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(lat, before)

    region = other_prompt(golden)
    settings = (
        ("guidance plan", lambda d: d.set_guidance([5.0, 4.0, 3.0, 2.0]), lambda d: d.clear_guidance()),
        ("guidance plan", lambda d: d.set_guidance(None, rescale=0.5), lambda d: d.clear_guidance()),
        ("skip-layer guidance", lambda d: d.set_skip_guidance([1], 3.0), lambda d: d.clear_skip_guidance()),
        ("stochastic plan", lambda d: d.set_stochastic(*stochastic_plan(sig, 1.0), seed=1), lambda d: d.clear_stochastic()),
        ("forecast plan", lambda d: d.set_forecast(1, [1, 1, 0, 1]), lambda d: d.clear_forecast()),
        ("regional prompts", lambda d: d.set_regions([{"text_embeds": region["text_embeds"]}], [torch.arange(5)], torch.ones(1, *WINDOW).cuda()),
         lambda d: d.clear_regions()),
    )
    for word, install, clear in settings:
        install(tiny_dit)
        try:
            refused(tiny_dit, word)
        finally:
            clear(tiny_dit)
    # MagCache calibration and a CFG pair, on handles of their own (a lone pair handle: the call is refused before any exchange, no peer is needed)
    cal = make_dit(cfg, tiny_sd)
    cal.engine("cuda:0")
    start_magcache_calibration(cal, 4, False)
    try:
        refused(cal, "MagCache calibration")
    finally:
        stop_magcache_calibration(cal)
    pair = make_dit(cfg, tiny_sd)
    pair.engine("cuda:0")
    group = E.LoopbackGroup(2)
    pair.enable_cfg_pair_loopback(group, 0)
    refused(pair, "CFG pair")
    pair._destroy_engine(force=True)
    # nothing was left behind: both handles that can still run give the plain bits
    assert torch.equal(call(cal), plain)
    lat.copy_(before)
    assert torch.equal(call(tiny_dit), plain)


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_the_engine_entry_with_one_window_is_the_plain_run(tiny_dit, golden, w):
    """k5_sample_tiles on a clip no larger than the window (through `sample(tiles=)`, not `generate`, which resolves such a plan itself): the
    plain run on the whole clip, with the first window's prompt where there is a prompt per window"""
    from kandinsky.generation_utils import sigma_schedule, tile_windows
    te, ne = prompts(golden)
    tb = other_prompt(golden)
    noise = golden["gen.noise"]                                             # (3, 8, 12, 16): the window itself
    sig = sigma_schedule(4, 5.0).tolist()
    one = tile_windows((3, 8, 12), WINDOW, (0, 0, 0))
    assert one.nwin == 1

    def sample(text, pos, **kw):
        lat = noise.cuda().contiguous()
        return tiny_dit.sample(lat, sig, text, ne, POS, pos, torch.arange(4), w, scale_factor=(1.0, 2.0, 2.0), **kw)

    assert torch.equal(sample(te, torch.arange(7), tiles=one), sample(te, torch.arange(7)))
    assert torch.equal(sample(te, torch.arange(7), tiles=one), run_generate(tiny_dit, golden, noise, w))
    other = sample(te, torch.arange(7), tiles=one, window_text=[(tb, torch.arange(5))])      # the window's own prompt replaces the call's
    assert torch.equal(other, sample(tb, torch.arange(5))) and not torch.equal(other, sample(te, torch.arange(7)))


def test_the_watch_reports_the_whole_clips_extents(tiny_dit, golden, tile_golden):
    """a raw k5_watch on the handle: every step's info carries (total_T, total_H, total_W, C) of the tiled clip, not the window's"""
    import ctypes
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule, tile_windows
    te, ne = prompts(golden)
    seen = []
    fn = E.WATCH_FN(lambda user, info: seen.append((info.contents.step, info.contents.num_steps, info.contents.T, info.contents.H, info.contents.W,
                                                    info.contents.C, bool(info.contents.rgb))) or 0)
    k = E.Watch()
    k.fn, k.preview_every = fn, 0
    h = tiny_dit.engine("cuda:0")
    lat = tile_golden[0]["tile.t2s2.noise"].cuda().contiguous()
    plan = tile_windows((5, 8, 20), WINDOW, (1, 0, 4))
    assert E.lib().k5_dit_set_watch(h, ctypes.byref(k)) == 0
    try:
        tiny_dit.sample(lat, sigma_schedule(4, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0), tiles=plan)
        torch.cuda.synchronize()
    finally:
        assert E.lib().k5_dit_set_watch(h, None) == 0
    assert seen == [(i, 4, 5, 8, 20, 16, False) for i in range(4)]
    assert torch.equal(lat, run_tiles(tiny_dit, golden, tile_golden, "t2s2", 5.0))


# ------------------------------------------------------------------------------------------ pipeline end to end
def test_pipeline_with_tiles_end_to_end():
    pipe, dit, vae = _tiny_pipeline()
    seen = {}
    samp = dit.sample

    def spy_sample(*a, **k):
        seen["tiles"], seen["pos"] = k.get("tiles"), [len(p) for p in a[4]]
        return samp(*a, **k)

    dit.sample = spy_sample
    pipe._save = lambda images, time_length, save_path: images             # the uint8 frames themselves, not the PIL pictures of an image run
    out = pipe("a cat in a blue hat", time_length=0, height=768, width=768, tile_height=512, tile_width=512, tile_overlap=256, num_steps=2, seed=7,
               expand_prompts=False, scheduler_scale=5.0)
    dit.sample = samp
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, 3, 1, 768, 768)
    p = seen["tiles"]
    assert p.counts == (1, 2, 2) and p.window == (1, 64, 64) and p.starts == ([0], [0, 32], [0, 32]) and seen["pos"] == [1, 32, 32]
