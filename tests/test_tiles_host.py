"""CPU-only checks of spatial context windows (tiles): the 3-D plan, the per-step path of `generate` on a duck-typed model (which forwards run, on
which boxes, in which order), every refusal that needs no GPU, the pipeline's size check and the CLI's keywords, and header / binding / library
agreement on the new entry points."""
import ctypes as C
import functools
import os
import shutil
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tile_kernels_reference import cpu_cfg_euler_tiles, cpu_tile_tables  # noqa: E402
import kit  # noqa: E402
from kit import PKG, POS, ROOT, assert_abi_entries, built_lib, flash_conf, host_tiny  # noqa: E402

CONF = flash_conf()
WINDOW = (3, 8, 12)
ISSUE_CASES = {"s22": ((3, 12, 20), (0, 4, 4), (1, 2, 2), ([0], [0, 4], [0, 8])),
               "s14": ((3, 8, 24), (0, 0, 8), (1, 1, 4), ([0], [0], [0, 4, 8, 12])),
               "t2s2": ((5, 8, 20), (1, 0, 4), (2, 1, 2), ([0, 2], [0], [0, 8]))}


def shares(plan):
    """per cell, the sum over the covering windows of rn(rn(wt * wy) * wx), added in window order in fp32: what the kernel composes"""
    wt, wy, wx = plan.weights
    nt, ny, nx = plan.counts
    total = torch.zeros(plan.clip, dtype=torch.float32)
    count = torch.zeros(plan.clip, dtype=torch.int64)
    for k in range(plan.nwin):
        it, iy, ix = k // (ny * nx), (k // nx) % ny, k % nx
        s = (wt[it][:, None, None] * wy[iy][None, :, None]) * wx[ix][None, None, :]
        total[plan.box(k)] += s
        count[plan.box(k)] += 1
    return total, count


# ------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("tag", sorted(ISSUE_CASES))
def test_plans_of_the_issue(tag):
    from kandinsky.generation_utils import tile_windows
    clip, overlap, counts, starts = ISSUE_CASES[tag]
    p = tile_windows(clip, WINDOW, overlap)
    assert p.counts == counts and tuple(list(s) for s in p.starts) == starts and p.nwin == counts[0] * counts[1] * counts[2]
    assert p.window == WINDOW and p.clip == clip
    for w, n, F in zip(p.weights, counts, WINDOW):
        assert w.dtype == torch.float32 and tuple(w.shape) == (n, F)
    assert p.corner(p.nwin - 1) == (starts[0][-1], starts[1][-1], starts[2][-1])
    total, count = shares(p)
    assert (count >= 1).all() and int(count.max()) == {"s22": 4, "s14": 3, "t2s2": 4}[tag]
    assert (total - 1.0).abs().max().item() <= 4 * float(np.finfo(np.float32).eps)


def test_both_cells_of_a_patch_carry_its_weight_and_starts_are_patch_aligned():
    from kandinsky.generation_utils import context_windows, tile_windows
    p = tile_windows((3, 12, 20), WINDOW, (0, 4, 4))
    ps, pw = context_windows(10, 6, 2)                                      # the columns in patches
    assert p.starts[2] == [2 * s for s in ps]
    assert torch.equal(p.weights[2][:, 0::2], pw) and torch.equal(p.weights[2][:, 1::2], pw)
    assert all(s % 2 == 0 for axis in p.starts[1:] for s in axis)


def test_random_plans_cover_every_cell_and_sum_to_one():
    from kandinsky.generation_utils import tile_windows
    rng = np.random.default_rng(11)
    ulp = float(np.finfo(np.float32).eps)
    seen = 0
    while seen < 60:
        win = (int(rng.integers(1, 5)), 2 * int(rng.integers(1, 6)), 2 * int(rng.integers(1, 6)))
        clip = (int(rng.integers(1, 9)), 2 * int(rng.integers(1, 12)), 2 * int(rng.integers(1, 12)))
        ov = (int(rng.integers(0, win[0])), 2 * int(rng.integers(0, win[1] // 2)), 2 * int(rng.integers(0, win[2] // 2)))
        try:
            p = tile_windows(clip, win, ov)
        except ValueError as e:
            assert "at most 64" in str(e)
            continue
        seen += 1
        total, count = shares(p)
        assert (count >= 1).all(), (clip, win, ov)
        assert (total - 1.0).abs().max().item() <= 4 * ulp, (clip, win, ov)
        for st, F, n in zip(p.starts, p.window, p.clip):
            assert st[0] == 0 and st[-1] + F == n and all(b > a for a, b in zip(st, st[1:]))


def test_plan_refusals():
    from kandinsky.generation_utils import tile_windows
    for clip, win, ov in (((3, 9, 20), WINDOW, (0, 4, 4)), ((3, 12, 21), WINDOW, (0, 4, 4)), ((3, 12, 20), (3, 7, 12), (0, 4, 4)),
                          ((3, 12, 20), (3, 8, 11), (0, 4, 4)), ((3, 12, 20), WINDOW, (0, 3, 4)), ((3, 12, 20), WINDOW, (0, 4, 5))):
        with pytest.raises(ValueError, match="odd"):
            tile_windows(clip, win, ov)
    with pytest.raises(ValueError, match="overlap"):
        tile_windows((3, 12, 20), WINDOW, (0, 8, 4))
    assert tile_windows((1, 18, 18), (1, 4, 4), (0, 2, 2)).nwin == 64      # 8 x 8
    with pytest.raises(ValueError, match=r"nwin = 1 x 9 x 8 = 72") as e:
        tile_windows((1, 20, 18), (1, 4, 4), (0, 2, 2))
    assert "(1, 20, 18)" in str(e.value) and "(1, 4, 4)" in str(e.value)   # the message names the plan


def test_a_window_at_least_as_large_as_the_clip_is_one_window_of_weight_one():
    from kandinsky.generation_utils import tile_windows
    for win, ov in ((WINDOW, (0, 0, 0)), ((5, 16, 24), (2, 4, 8)), ((3, 8, 12), (2, 6, 10))):
        p = tile_windows((3, 8, 12), win, ov)
        assert p.nwin == 1 and p.window == (3, 8, 12) and p.starts == ([0], [0], [0])
        assert all(torch.equal(w, torch.ones(1, n)) for w, n in zip(p.weights, (3, 8, 12)))
    p = tile_windows((3, 8, 24), (3, 16, 12), (0, 4, 4))                   # one axis whole, one tiled
    assert p.counts == (1, 1, 3) and p.window == (3, 8, 12) and torch.equal(p.weights[1], torch.ones(1, 8))


def test_a_temporal_plan_reproduces_context_windows():
    from kandinsky.generation_utils import context_windows, tile_windows
    for T, F, o in ((7, 3, 2), (6, 3, 1), (121, 61, 15)):
        st, wt = context_windows(T, F, o)
        p = tile_windows((T, 8, 12), (F, 8, 12), (o, 0, 0))
        assert p.counts == (len(st), 1, 1) and p.starts[0] == st and torch.equal(p.weights[0], wt)
        assert torch.equal(p.weights[1], torch.ones(1, 8)) and torch.equal(p.weights[2], torch.ones(1, 12))


# ------------------------------------------------------------------------------------------ per-step path on a duck-typed model
class FakeDit:
    """duck-typed model: a velocity that depends on the latent, the prompt and the time; every call is logged"""
    visual_cond = False

    def __init__(self):
        self.calls = []

    def __call__(self, x, text_embed, pooled, t, visual_rope_pos, text_rope_pos, scale_factor=None, sparse_params=None):
        self.calls.append((x.clone(), text_embed, x.is_contiguous(), [len(p) for p in visual_rope_pos]))
        return (0.5 * x + text_embed.mean() + pooled.mean() * float(t.reshape(-1)[0]) / 1000).to(torch.bfloat16)


prompt = functools.partial(kit.host_prompt, dims=(8, 4))


@pytest.fixture()
def cpu_kernels(monkeypatch):
    import euler_step_reference as ER
    from kandinsky import generation_utils as G
    monkeypatch.setattr(G.E, "euler_step_", ER.euler_step_)
    monkeypatch.setattr(G.E, "cfg_euler_tiles_", cpu_cfg_euler_tiles)
    monkeypatch.setattr(G.E, "tile_tables", cpu_tile_tables)
    return G


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_per_step_path_runs_every_window_on_a_contiguous_copy_of_its_box(cpu_kernels, w):
    G = cpu_kernels
    clip, steps = (5, 8, 20), 2
    noise = torch.randn(*clip, 16, generator=torch.Generator().manual_seed(5))
    te, ne = prompt(4, 1), prompt(2, 2)
    pos = [torch.arange(5), torch.arange(4), torch.arange(10)]            # the clip's positions: the window's are their first entries
    model = FakeDit()
    kw = dict(context_frames=3, context_overlap=1, context_height=8, context_width=12, context_overlap_hw=(0, 4))
    out = G.generate(model, "cpu", (*clip, 16), steps, te, ne, pos, torch.arange(4), torch.arange(2), w, 5.0, CONF, noise=noise, **kw)
    plan = G.tile_windows(clip, WINDOW, (1, 0, 4))
    per = 2 if w != 1.0 else 1
    assert plan.nwin == 4 and len(model.calls) == steps * plan.nwin * per
    for k in range(plan.nwin):                                            # step 0: window k saw its own box of the noise, t-major then columns
        call = model.calls[k * per]
        assert torch.equal(call[0], noise[plan.box(k)]) and call[1] is te["text_embeds"] and call[2] and call[3] == [3, 4, 6]
        if per == 2:
            assert model.calls[k * per + 1][1] is ne["text_embeds"] and torch.equal(model.calls[k * per + 1][0], noise[plan.box(k)])
    assert out.shape == noise.shape and not torch.equal(out, noise)
    full = G.generate(FakeDit(), "cpu", (*clip, 16), steps, te, ne, pos, torch.arange(4), torch.arange(2), w, 5.0, CONF, noise=noise)
    one = G.generate(FakeDit(), "cpu", (*clip, 16), steps, te, ne, pos, torch.arange(4), torch.arange(2), w, 5.0, CONF, noise=noise,
                     context_height=8, context_width=20)
    assert torch.equal(one, full)                                         # a tile as large as the frame is the plain run


def test_per_window_prompts_and_batches(cpu_kernels):
    G = cpu_kernels
    clip = (3, 8, 20)
    noise = torch.randn(2 * clip[0], *clip[1:], 16, generator=torch.Generator().manual_seed(6))
    te, tb, ne = prompt(4, 1), prompt(3, 3), prompt(2, 2)
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    args = (1, te, ne, pos, torch.arange(4), torch.arange(2), 5.0, 5.0, CONF)
    kw = dict(context_width=12, context_overlap_hw=4)
    model = FakeDit()
    G.generate(model, "cpu", (*clip, 16), *args, noise=noise[:3], context_text=[(te, torch.arange(4)), (tb, torch.arange(3))], **kw)
    assert [c[1] is t["text_embeds"] for c, t in zip(model.calls, (te, ne, tb, ne))] == [True] * 4
    with pytest.raises(ValueError, match="nwin = 2"):
        G.generate(FakeDit(), "cpu", (*clip, 16), *args, noise=noise[:3], context_text=[(te, torch.arange(4))] * 3, **kw)
    both = G.generate(FakeDit(), "cpu", (6, 8, 20, 16), *args, noise=noise, batch=2, **kw)   # a batch: every sample is the tiled call of its own
    for b in range(2):
        alone = G.generate(FakeDit(), "cpu", (*clip, 16), *args, noise=noise[3 * b:3 * b + 3], **kw)
        assert torch.equal(both[3 * b:3 * b + 3], alone)


def test_the_default_overlap_is_a_quarter_of_the_window_rounded_down_to_even(cpu_kernels):
    G = cpu_kernels
    tiles = G._plan_for(NS(visual_cond=False), (3, 16, 40), (None, None, None, 8, 12, None), None, 0)
    assert tiles.overlap == (0, 2, 2) and tiles.window == (3, 8, 12)       # 8 // 4 = 2; 12 // 4 = 3 -> 2
    tiles = G._plan_for(NS(visual_cond=False), (3, 16, 40), (None, None, None, 8, 12, 4), None, 0)
    assert tiles.overlap == (0, 4, 4)
    tiles = G._plan_for(NS(visual_cond=False), (3, 16, 40), (None, None, None, 8, 12, (2, 6)), None, 0)
    assert tiles.overlap == (0, 2, 6)


def test_context_frames_alone_is_the_3d_plan_with_one_row_and_one_column_window():
    from kandinsky import generation_utils as G
    model = NS(visual_cond=False)
    for T, F, o in ((7, 3, 2), (6, 3, 1), (5, 3, None)):
        st, wt = G.context_windows(T, F, F // 4 if o is None else o)
        p = G._plan_for(model, (T, 8, 12), (F, o, None, None, None, None), None, 0)
        assert isinstance(p, G.TileWindows) and p.counts == (len(st), 1, 1) and p.nwin == len(st)
        assert p.clip == (T, 8, 12) and p.window == (F, 8, 12)
        assert p.starts[0] == st and torch.equal(p.weights[0], wt) and list(p.starts[1]) == [0] and list(p.starts[2]) == [0]
        assert p.weights[1].dtype == torch.float32 and tuple(p.weights[1].shape) == (1, 8) and tuple(p.weights[2].shape) == (1, 12)
        assert (p.weights[1] == 1.0).all() and (p.weights[2] == 1.0).all()
    assert G._plan_for(model, (3, 8, 12), (3, None, None, None, None, None), None, 0) is None          # one window: the plain run
    one = G._plan_for(model, (3, 8, 12), (5, 1, [None], None, None, None), None, 0)                      # ... kept for its one prompt
    assert one.nwin == 1 and one.window == (3, 8, 12)
    ctx = (3, 1, None, None, None, None)
    for refused in (lambda: G._plan_for(model, (6, 8, 12), ctx, torch.zeros(1), 0),
                    lambda: G._plan_for(model, (6, 8, 12), ctx, None, 2),
                    lambda: G._plan_for(NS(visual_cond=False, mag_ratios=[1.0] * 8), (6, 8, 12), ctx, None, 0),
                    lambda: G._plan_for(NS(visual_cond=False, _cfg_parallel=(0, None)), (6, 8, 12), ctx, None, 0)):
        with pytest.raises(ValueError, match="context_frames") as e:
            refused()
        assert "context_height" not in str(e.value)
    with pytest.raises(ValueError, match="context_height / context_width") as e:                       # the keywords the caller gave
        G._plan_for(model, (6, 8, 24), (3, 1, None, None, 12, None), torch.zeros(1), 0)
    assert "context_frames" not in str(e.value)


# ------------------------------------------------------------------------------------------ refusals
SHAPE = (3, 12, 20, 16)
TILED = dict(context_height=8, context_width=12)


Wrapped = functools.partial(kit.Wrapped, blocks=True, hand_on=("forward_skip",), refuse=True)


def big_prompt(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"text_embeds": torch.randn(n, 96, generator=g), "pooled_embed": torch.randn(1, 48, generator=g)}


call_generate = functools.partial(kit.call_generate, w=5.0, steps=4, shape=SHAPE, pos=POS, conf=CONF, prompt=big_prompt)


def test_generate_refuses_every_refused_combination_before_the_model_is_touched(golden_meta):
    m = host_tiny(golden_meta)
    m.sample = lambda *a, **k: pytest.fail("refused calls must not sample")
    src = torch.zeros(SHAPE)
    W, b = torch.zeros(16, 3), torch.zeros(3)
    regions = dict(region_text_embeds=[big_prompt(5, 10)], region_text_rope_pos=[torch.arange(5)], region_masks=torch.rand(1, *SHAPE[:3]))
    for model in (m, Wrapped(m)):
        for kw, word in ((dict(init_latent=src), "init_latent"),
                         (dict(init_latent=src, source_text_embeds=big_prompt(5, 2), source_text_rope_pos=torch.arange(5)), "init_latent"),
                         (dict(callback=lambda i: None, preview_every=1, preview_factors=(W, b)), "preview_every"),
                         (dict(cfg_rescale=0.5), "context windows"), (dict(guidance_schedule=[5.0] * 4), "context windows"),
                         (dict(guidance_interval=(0.0, 0.9)), "context windows"), (dict(cfg_zero_star=True), "context windows"),
                         (dict(slg_blocks=[1], slg_scale=3.0), "context windows"),
                         (dict(eta=1.0), "context windows"),
                         (dict(forecast_interval=2, forecast_warmup=1), "context windows"),
                         (dict(context_text=[None] * 3), "nwin = 4"),
                         (dict(context_overlap_hw=(3, 4)), "odd"), (dict(context_overlap_hw=(8, 4)), "overlap"),
                         (dict(context_height=7), "odd")):
            with pytest.raises(ValueError, match=word):
                call_generate(model, **{**TILED, **kw})
    with pytest.raises(ValueError, match="window"):
        call_generate(m, **TILED, **regions)
    with pytest.raises(ValueError, match="context_height"):
        call_generate(m, context_overlap_hw=4)
    with pytest.raises(ValueError, match="context_frames"):
        call_generate(m, context_overlap=1, **TILED)
    for state in (dict(mag_ratios=[1.0] * 8), dict(mag_ratios=None, _magcache_calibrate=(4, False))):
        with pytest.raises(ValueError, match="MagCache"):
            call_generate(NS(visual_cond=True, **state), **TILED)
    with pytest.raises(ValueError, match="single-rank"):
        call_generate(NS(visual_cond=True, _cfg_parallel=(0, None)), **TILED)
    assert m._guidance is None and m._regions is None


def test_model_sample_refusals():
    from kandinsky.generation_utils import tile_windows
    from kandinsky.models.dit import DiffusionTransformer3D
    d = DiffusionTransformer3D.__new__(DiffusionTransformer3D)
    p = tile_windows((3, 12, 20), WINDOW, (0, 4, 4))
    with pytest.raises(ValueError, match="tiles together with edit"):
        d.sample(None, [1.0, 0.0], None, None, None, None, None, 1.0, tiles=p, edit=(1, 2, 3))
    with pytest.raises(ValueError, match="tiles together with edit or windows"):
        d.sample(None, [1.0, 0.0], None, None, None, None, None, 1.0, tiles=p, windows=([0], [[1.0]]))
    with pytest.raises(ValueError, match="flowedit together with"):
        d.sample(None, [1.0, 0.0], None, None, None, None, None, 1.0, tiles=p, flowedit=(None,) * 8)
    with pytest.raises(ValueError, match="planned for a clip"):
        d.sample(torch.zeros(3, 12, 22, 16), [1.0, 0.0], None, None, None, None, None, 1.0, tiles=p)
    with pytest.raises(ValueError, match="tiles must hold"):
        d.sample(torch.zeros(3, 12, 20, 16), [1.0, 0.0], None, None, None, None, None, 1.0,
                 tiles=NS(clip=p.clip, window=p.window, starts=p.starts, weights=(p.weights[0], p.weights[1][:1], p.weights[2])))


def test_generate_sample_checks_the_prompt_list_against_the_plan():
    from kandinsky.generation_utils import generate_sample
    with pytest.raises(ValueError, match="nwin = 4"):
        generate_sample((1, 3, 12, 20, 16), ["a", "b"], None, None, CONF, None, context_height=8, context_width=12, context_overlap_hw=4)
    with pytest.raises(ValueError, match="context_height"):
        generate_sample((1, 3, 12, 20, 16), "a", None, None, CONF, None, context_overlap_hw=4)
    with pytest.raises(ValueError, match="init_latent"):
        generate_sample((1, 3, 12, 20, 16), "a", NS(), None, CONF, None, context_height=8, context_width=12, video=torch.zeros(9, 3, 96, 160))


# ------------------------------------------------------------------------------------------ pipeline and CLI
@pytest.fixture()
def pipe_and_seen(monkeypatch):
    from kandinsky import t2v_pipeline as P
    seen = {}

    def fake_generate_sample(shape, caption, *a, **k):
        seen.update(shape=shape, caption=caption, kw=k)
        return torch.zeros(shape[0], 3, 4 * (shape[1] - 1) + 1, 8, 8, dtype=torch.uint8)

    monkeypatch.setattr(P, "generate_sample", fake_generate_sample)
    conf = NS(model=NS(num_steps=4, guidance_weight=5.0))
    return P.Kandinsky5T2VPipeline({"dit": "cpu", "vae": "cpu", "text_embedder": "cpu"}, None, None, None, conf=conf), seen


def test_pipeline_size_check_with_and_without_tiles(pipe_and_seen):
    pipe, seen = pipe_and_seen
    kw = dict(expand_prompts=False, seed=1, time_length=5)
    pipe("a cat", height=1024, width=1024, tile_height=512, tile_width=768, tile_overlap=128, **kw)
    assert seen["shape"] == (1, 31, 128, 128, 16)
    assert (seen["kw"]["context_height"], seen["kw"]["context_width"], seen["kw"]["context_overlap_hw"]) == (64, 96, 16)
    pipe("a cat", height=768, width=768, tile_height=512, tile_width=512, **kw)   # below 900: any multiple of 16 that is at least the tile
    assert "context_overlap_hw" not in seen["kw"] and seen["kw"]["context_height"] == 64
    pipe("a cat", height=528, width=800, tile_height=512, tile_width=768, **kw)
    assert seen["shape"][2:4] == (66, 100)
    pipe(["a", "b", "c", "d"], height=768, width=768, tile_height=512, tile_width=512, **kw)
    assert seen["shape"][0] == 1 and seen["caption"] == ["a", "b", "c", "d"]     # one frame, a prompt per window
    pipe("a cat", height=512, width=768, **kw)                                     # without tile_*: the sizes it always took, nothing new passed on
    assert not any(k.startswith("context_") for k in seen["kw"])
    for bad, word in ((dict(height=1024, width=1024), "Wrong height, width pair"),
                      (dict(height=1024, width=1024, tile_height=512, tile_width=640), "Available .tile_height, tile_width. are"),
                      (dict(height=1024, width=1024, tile_height=512), "Available .tile_height, tile_width. are"),
                      (dict(height=520, width=768, tile_height=512, tile_width=768), "multiples of 16"),
                      (dict(height=512, width=512, tile_height=512, tile_width=768), "at least the tile"),
                      (dict(height=1040, width=1024, tile_height=512, tile_width=768), r"tiling table: \[160, .*1408\]"),
                      (dict(height=1024, width=1024, tile_height=512, tile_width=768, tile_overlap=100), "tile_overlap"),
                      (dict(height=1024, width=1024, tile_height=512, tile_width=768, tile_overlap=512), "tile_overlap"),
                      (dict(height=512, width=768, tile_overlap=128), "tile_overlap needs")):
        seen.clear()
        with pytest.raises(ValueError, match=word):
            pipe("a cat", **kw, **bad)
        assert not seen                                                              # raised before anything ran
    tiled = dict(height=1024, width=1024, tile_height=512, tile_width=768)           # what the temporal windows refuse, the tiles refuse
    for extra, word in ((dict(eta=1.0), "context windows"), (dict(slg_blocks=[1], slg_scale=3.0), "context windows"),
                        (dict(cfg_rescale=0.5), "tile_height"), (dict(regions=[("a", torch.ones(8, 8))]), "tile_height")):
        with pytest.raises(ValueError, match=word):
            pipe("a cat", **kw, **tiled, **extra)
        assert not seen


def test_cli_flags_reach_the_pipeline_keywords():
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_cli_tiles", os.path.join(PKG, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    assert cli.tile_keywords(p.parse_args([])) == {}
    a = p.parse_args(["--height", "1024", "--width", "1024", "--tile", "512", "768"])
    assert cli.tile_keywords(a) == {"tile_height": 512, "tile_width": 768} and (a.height, a.width) == (1024, 1024)
    cli.validate_args(a)
    a = p.parse_args(["--height", "1024", "--width", "1024", "--tile", "512", "768", "--tile_overlap", "128"])
    assert cli.tile_keywords(a) == {"tile_height": 512, "tile_width": 768, "tile_overlap": 128}
    with pytest.raises(ValueError, match="--tile"):
        cli.tile_keywords(p.parse_args(["--tile_overlap", "128"]))
    with pytest.raises(SystemExit):
        p.parse_args(["--height", "1024", "--width", "1024"])                           # a large frame needs --tile: the usage error it always was
    assert p.parse_args(["--height", "768", "--width", "512"]).height == 768
    with pytest.raises(NotImplementedError, match="tile"):
        cli.validate_args(p.parse_args(["--height", "1024", "--width", "1024", "--tile", "640", "640"]))
    cli.validate_args(p.parse_args([]))
    with pytest.raises(SystemExit):
        p.parse_args(["--tile", "512"])


# ------------------------------------------------------------------------------------------ ABI
def test_header_binding_and_library_agree_on_the_new_entries(built_lib):
    from kandinsky import _engine as E
    assert_abi_entries(built_lib, ("k5_cfg_euler_tiles", "k5_patchify_view_bf16", "k5_sample_tiles"),
                       [("k5_tile_plan", E.TilePlan), ("k5_sample_tiles_args", E.SampleTilesArgs)])


def test_struct_sizes_match_a_compiled_c_program(tmp_path):
    from kandinsky import _engine as E
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler: the struct sizes cannot be checked")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "k5.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(k5_tile_plan), '
                   'sizeof(k5_sample_tiles_args), sizeof(k5_sample_args), sizeof(k5_sample_windows_args)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(E.TilePlan), C.sizeof(E.SampleTilesArgs), C.sizeof(E.SampleArgs), C.sizeof(E.SampleWindowsArgs)]


def test_entries_refuse_bad_arguments_without_a_gpu(built_lib):
    from kandinsky import _engine as E
    L = E.lib()
    plan = E.TilePlan(1, 1, 1, 3, 8, 12)
    assert L.k5_cfg_euler_tiles(None, None, None, 1.0, 0.1, None, 3, 8, 12, 16, None) == 1
    assert "k5_cfg_euler_tiles" in E.last_error()
    assert L.k5_cfg_euler_tiles(None, None, None, 1.0, 0.1, C.byref(plan), 3, 8, 12, 16, None) == 1       # NULL tables
    assert L.k5_patchify_view_bf16(None, 0, 0, None, 0, 0, None, 1, 2, 2, 16, 16, 64, None, None) == 1
    assert L.k5_sample_tiles(None, None, None, None) == 1
    host = (C.c_float * 64)()
    for bad in (dict(T=0), dict(H=3), dict(W=5), dict(rs=31), dict(fs=63)):   # extents < 1, odd rows or columns, strides below what they span
        a = dict(T=1, H=2, W=2, rs=32, fs=64)
        a.update(bad)
        assert L.k5_patchify_view_bf16(host, a["fs"], a["rs"], None, 0, 0, host, a["T"], a["H"], a["W"], 16, 16, 64, None, None) == 1, bad
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.cfg_euler_tiles_(torch.zeros(3, 8, 12, 4), torch.zeros(1, 3, 8, 12, 4, dtype=torch.bfloat16), None, 1.0, 0.1, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.patchify_view_(torch.zeros(1, 2, 2, 16), None, 16, 64)
