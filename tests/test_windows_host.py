"""CPU-only checks of temporal context windows: the window plan, the decode tiling beyond the table's last row, the per-step path of
`generate` on a duck-typed model (which forwards run, on which slices, in which order), every refusal that needs no GPU, the pipeline's and
the CLI's keywords, and header / binding / library agreement on the new entry points."""
import ctypes as C
import functools
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import euler_step_reference as ER  # noqa: E402
from tile_kernels_reference import cpu_cfg_euler_tiles, cpu_tile_tables  # noqa: E402
import kit  # noqa: E402
from kit import PKG, assert_abi_entries, built_lib, flash_conf  # noqa: E402

CONF = flash_conf()


# ------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("T,F,overlap,starts", [(5, 3, 1, [0, 2]), (6, 3, 1, [0, 1, 3]), (7, 3, 2, [0, 1, 2, 3, 4]), (121, 61, 15, [0, 30, 60])])
def test_plans_of_the_issue(T, F, overlap, starts):
    from kandinsky.generation_utils import context_windows
    st, wt = context_windows(T, F, overlap)
    assert st == starts
    assert wt.dtype == torch.float32 and tuple(wt.shape) == (len(starts), F)


def test_plan_weights_are_the_normalised_triangle():
    from kandinsky.generation_utils import context_windows
    st, wt = context_windows(6, 3, 1)                     # raw 1 2 1; frame 1: windows 0 (2) and 1 (1); frame 2: 0 (1), 1 (2); frame 3: 1 (1), 2 (1)
    f32 = lambda a, b: float(np.float32(np.float64(a) / np.float64(b)))   # noqa: E731
    want = [[1.0, f32(2, 3), f32(1, 3)], [f32(1, 3), f32(2, 3), 0.5], [0.5, 1.0, 1.0]]
    assert wt.tolist() == want
    st, wt = context_windows(7, 3, 2)                     # three-fold in the middle: frame 2 = 1 + 2 + 1
    assert [wt[0][2].item(), wt[1][1].item(), wt[2][0].item()] == [0.25, 0.5, 0.25]


def test_one_window_when_the_clip_fits():
    from kandinsky.generation_utils import context_windows
    for T, F, o in ((3, 3, 1), (2, 5, 4), (1, 1, 0)):
        st, wt = context_windows(T, F, o)
        assert st == [0] and torch.equal(wt, torch.ones(1, T))


def test_random_plans_cover_every_frame_and_sum_to_one():
    from kandinsky.generation_utils import context_windows
    rng = np.random.default_rng(7)
    ulp = float(np.finfo(np.float32).eps)
    seen = 0
    while seen < 300:
        F = int(rng.integers(1, 40))
        o = int(rng.integers(0, F))
        T = int(rng.integers(1, 400))
        if T > F and -(-(T - o) // (F - o)) > 64:
            continue
        seen += 1
        st, wt = context_windows(T, F, o)
        n = len(st)
        assert st[0] == 0 and st[-1] + wt.shape[1] == T and all(b > a for a, b in zip(st, st[1:]))
        total, count = np.zeros(T, dtype=np.float64), np.zeros(T, dtype=np.int64)
        for i in range(n):
            w = wt[i].double().numpy()
            assert (w > 0).all()
            total[st[i]:st[i] + len(w)] += w
            count[st[i]:st[i] + len(w)] += 1
        assert (count >= 1).all(), (T, F, o)
        assert np.abs(total - 1.0).max() <= 2 * ulp, (T, F, o, np.abs(total - 1.0).max())


def test_plan_refusals():
    from kandinsky.generation_utils import context_windows
    for F, o in ((3, 3), (3, 4), (3, -1)):
        with pytest.raises(ValueError, match="overlap"):
            context_windows(10, F, o)
    assert len(context_windows(65, 2, 1)[0]) == 64                    # T - F + 1 windows at overlap F - 1: 64 is the most
    with pytest.raises(ValueError, match="nwin = 65"):
        context_windows(66, 2, 1)
    with pytest.raises(ValueError):
        context_windows(0, 3, 1)


# ------------------------------------------------------------------------------------------ decode tiling past 241 frames
def _temporal_tiles(vae, nf_latent, H=64, W=96):
    """(tile, stride, starts, held) of a decode of nf_latent frames, from the policy alone"""
    (_, ft, _, _), (fs, _, _) = vae.get_dec_optimal_tiling((1, 16, nf_latent, H, W))
    mf, sf = (ft - 1) // 4, fs // 4
    starts = list(range(0, nf_latent - mf + 1, sf))
    return (ft, fs), starts, [min(mf + 1, nf_latent - i) for i in starts], mf


def test_decode_tiling_repeats_with_the_period_and_keeps_tiles_full():
    from kandinsky.models import vae as V
    vae = V.AutoencoderKLHunyuanVideo.__new__(V.AutoencoderKLHunyuanVideo)
    for frames in range(245, 722, 4):
        nf = (frames - 1) // 4 + 1
        key = V.temporal_tiling_key(frames)
        assert 193 <= key <= 240 and (frames - key) % 48 == 0 and key in V.OPT_TEMPORAL_TILING
        lower = frames - 48
        assert vae.get_dec_optimal_tiling((1, 16, nf, 64, 96))[0][1] == V.OPT_TEMPORAL_TILING[V.temporal_tiling_key(lower)][0]
        assert vae.get_enc_optimal_tiling((1, 3, frames, 512, 768)) == vae.get_enc_optimal_tiling((1, 3, lower, 512, 768))
        _, starts, held, mf = _temporal_tiles(vae, nf)
        assert all(h == mf + 1 for h in held), (frames, starts, held)       # every tile is full ...
        assert starts[-1] + mf + 1 == nf                                     # ... and the last one ends the clip
    for frames in (289, 361, 481, 721):
        nf = (frames - 1) // 4 + 1
        _, starts, held, mf = _temporal_tiles(vae, nf)
        assert starts[-1] + mf + 1 == nf


def test_decode_tiling_up_to_241_frames_is_untouched():
    from kandinsky.models import vae as V
    vae = V.AutoencoderKLHunyuanVideo.__new__(V.AutoencoderKLHunyuanVideo)
    for frames in V.OPT_TEMPORAL_TILING:
        assert V.temporal_tiling_key(frames) == frames
        if frames > 97:
            assert vae.get_enc_optimal_tiling((1, 3, frames, 512, 768))[0][1] == V.OPT_TEMPORAL_TILING[frames][0]
    with pytest.raises(KeyError):
        vae.get_enc_optimal_tiling((1, 3, 99, 512, 768))                     # a length the table never had still raises


# ------------------------------------------------------------------------------------------ per-step path on a duck-typed model
class FakeDit:
    """duck-typed model: a velocity that depends on the latent, the prompt and the time; every call is logged"""
    visual_cond = False

    def __init__(self):
        self.calls = []

    def __call__(self, x, text_embed, pooled, t, visual_rope_pos, text_rope_pos, scale_factor=None, sparse_params=None):
        self.calls.append((x.clone(), text_embed, len(text_rope_pos), len(visual_rope_pos[0])))
        return (0.5 * x + text_embed.mean() + pooled.mean() * float(t.reshape(-1)[0]) / 1000).to(torch.bfloat16)


prompt = functools.partial(kit.host_prompt, dims=(8, 4))


@pytest.fixture()
def cpu_kernels(monkeypatch):
    from kandinsky import generation_utils as G
    monkeypatch.setattr(G.E, "euler_step_", ER.euler_step_)
    monkeypatch.setattr(G.E, "cfg_euler_tiles_", cpu_cfg_euler_tiles)
    monkeypatch.setattr(G.E, "tile_tables", cpu_tile_tables)
    return G


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_per_step_path_runs_every_window_on_its_slice(cpu_kernels, w):
    G = cpu_kernels
    T, F, o, steps = 6, 3, 1, 2
    noise = torch.randn(T, 4, 6, 16, generator=torch.Generator().manual_seed(5))
    te, ne = prompt(4, 1), prompt(2, 2)
    pos = [torch.arange(T), torch.arange(2), torch.arange(3)]            # the clip's positions: the window's are taken from them
    model = FakeDit()
    out = G.generate(model, "cpu", (T, 4, 6, 16), steps, te, ne, pos, torch.arange(4), torch.arange(2), w, 5.0, CONF, noise=noise,
                     context_frames=F, context_overlap=o)
    starts = [0, 1, 3]
    per = 2 if w != 1.0 else 1
    assert len(model.calls) == steps * len(starts) * per
    for k, st in enumerate(starts):                                       # step 0: window k saw its own slice of the noise
        call = model.calls[k * per]
        assert torch.equal(call[0], noise[st:st + F]) and call[1] is te["text_embeds"] and call[3] == F
        if per == 2:
            assert model.calls[k * per + 1][1] is ne["text_embeds"] and torch.equal(model.calls[k * per + 1][0], noise[st:st + F])
    assert out.shape == noise.shape and not torch.equal(out, noise)
    full = G.generate(FakeDit(), "cpu", (T, 4, 6, 16), steps, te, ne, pos, torch.arange(4), torch.arange(2), w, 5.0, CONF, noise=noise)
    one = G.generate(FakeDit(), "cpu", (T, 4, 6, 16), steps, te, ne, pos, torch.arange(4), torch.arange(2), w, 5.0, CONF, noise=noise,
                     context_frames=T)
    assert torch.equal(one, full)                                         # a window as long as the clip is the plain run


def test_per_window_prompts_and_batches(cpu_kernels):
    G = cpu_kernels
    T, F, o = 5, 3, 1
    noise = torch.randn(2 * T, 4, 6, 16, generator=torch.Generator().manual_seed(6))
    te, tb, ne = prompt(4, 1), prompt(3, 3), prompt(2, 2)
    pos = [torch.arange(F), torch.arange(2), torch.arange(3)]
    args = (1, te, ne, pos, torch.arange(4), torch.arange(2), 5.0, 5.0, CONF)
    model = FakeDit()
    G.generate(model, "cpu", (T, 4, 6, 16), *args, noise=noise[:T], context_frames=F, context_overlap=o,
               context_text=[(te, torch.arange(4)), (tb, torch.arange(3))])
    assert [c[1] is t["text_embeds"] for c, t in zip(model.calls, (te, ne, tb, ne))] == [True] * 4
    assert [c[2] for c in model.calls] == [4, 2, 3, 2]
    with pytest.raises(ValueError, match="nwin = 2"):
        G.generate(FakeDit(), "cpu", (T, 4, 6, 16), *args, noise=noise[:T], context_frames=F, context_overlap=o,
                   context_text=[(te, torch.arange(4))] * 3)
    # a batch: every sample is the windowed call of its own
    both = G.generate(FakeDit(), "cpu", (2 * T, 4, 6, 16), *args, noise=noise, batch=2, context_frames=F, context_overlap=o)
    for b in range(2):
        alone = G.generate(FakeDit(), "cpu", (T, 4, 6, 16), *args, noise=noise[b * T:(b + 1) * T], context_frames=F, context_overlap=o)
        assert torch.equal(both[b * T:(b + 1) * T], alone)


def test_progress_callback_and_cancel_on_the_per_step_path(cpu_kernels):
    G = cpu_kernels
    from kandinsky.models.dit import SamplingInterrupted
    noise = torch.randn(5, 4, 6, 16, generator=torch.Generator().manual_seed(8))
    te, ne = prompt(4, 1), prompt(2, 2)
    pos = [torch.arange(3), torch.arange(2), torch.arange(3)]
    seen = []
    G.generate(FakeDit(), "cpu", (5, 4, 6, 16), 3, te, ne, pos, torch.arange(4), torch.arange(2), 1.0, 5.0, CONF, noise=noise,
               context_frames=3, context_overlap=1, callback=lambda info: seen.append((info.step, info.num_steps)) and False)
    assert seen == [(0, 3), (1, 3), (2, 3)]
    with pytest.raises(SamplingInterrupted) as e:
        G.generate(FakeDit(), "cpu", (5, 4, 6, 16), 3, te, ne, pos, torch.arange(4), torch.arange(2), 1.0, 5.0, CONF, noise=noise,
                   context_frames=3, context_overlap=1, callback=lambda info: info.step == 1)
    assert e.value.steps_done == 2


# ------------------------------------------------------------------------------------------ refusals
SHAPE = (7, 8, 12, 16)


def call_generate(model=None, **kw):
    from kandinsky.generation_utils import generate
    return generate(model or NS(visual_cond=True), "cpu", SHAPE, 4, None, None, None, None, None, 5.0, 5.0, None, noise=torch.zeros(SHAPE), **kw)


def test_generate_refusals():
    with pytest.raises(ValueError, match="context_frames"):
        call_generate(context_overlap=1)
    with pytest.raises(ValueError, match="context_frames"):
        call_generate(context_text=[None])
    with pytest.raises(ValueError, match="overlap"):
        call_generate(context_frames=3, context_overlap=3)
    from kandinsky.generation_utils import generate
    with pytest.raises(ValueError, match="nwin = 65"):
        generate(NS(visual_cond=True), "cpu", (66, 8, 12, 16), 4, None, None, None, None, None, 5.0, 5.0, None, noise=torch.zeros(66, 8, 12, 16),
                 context_frames=2, context_overlap=1)
    with pytest.raises(ValueError, match="init_latent"):
        call_generate(context_frames=3, init_latent=torch.zeros(SHAPE))
    with pytest.raises(ValueError, match="preview_every"):
        call_generate(context_frames=3, preview_every=2, callback=lambda info: False, preview_factors=(torch.zeros(16, 3), None))
    for model in (NS(visual_cond=True, mag_ratios=[1.0] * 8), NS(visual_cond=True, mag_ratios=None, _magcache_calibrate=(4, False))):
        with pytest.raises(ValueError, match="MagCache"):
            call_generate(model, context_frames=3)
    with pytest.raises(ValueError, match="single-rank"):
        call_generate(NS(visual_cond=True, _cfg_parallel=(0, None)), context_frames=3)


def test_model_sample_refusals():
    from kandinsky.models.dit import DiffusionTransformer3D
    d = DiffusionTransformer3D.__new__(DiffusionTransformer3D)
    with pytest.raises(ValueError, match="window_text needs windows"):
        d.sample(None, [1.0, 0.0], None, None, None, None, None, 1.0, window_text=[None])
    with pytest.raises(ValueError, match="edit together with windows"):
        d.sample(None, [1.0, 0.0], None, None, None, None, None, 1.0, windows=([0], [[1.0]]), edit=(1, 2, 3))


def test_generate_sample_checks_the_prompt_list_against_the_plan():
    from kandinsky.generation_utils import generate_sample
    with pytest.raises(ValueError, match="nwin = 3"):
        generate_sample((1, 6, 8, 12, 16), ["a", "b"], None, None, CONF, None, context_frames=3, context_overlap=1)
    with pytest.raises(ValueError, match="context_frames"):
        generate_sample((1, 6, 8, 12, 16), "a", None, None, CONF, None, context_overlap=1)


# ------------------------------------------------------------------------------------------ pipeline and CLI
def test_pipeline_maps_seconds_to_latent_frames(monkeypatch):
    from kandinsky import t2v_pipeline as P
    seen = {}

    def fake_generate_sample(shape, caption, *a, **k):
        seen.update(shape=shape, caption=caption, kw=k)
        return torch.zeros(shape[0], 3, 4 * (shape[1] - 1) + 1, 8, 8, dtype=torch.uint8)

    monkeypatch.setattr(P, "generate_sample", fake_generate_sample)
    conf = NS(model=NS(num_steps=4, guidance_weight=5.0))
    pipe = P.Kandinsky5T2VPipeline({"dit": "cpu", "vae": "cpu", "text_embedder": "cpu"}, None, None, None, conf=conf)
    pipe("a cat", time_length=20, context_seconds=10, context_overlap_seconds=2.5, expand_prompts=False, seed=1)
    assert seen["shape"][:2] == (1, 121) and seen["kw"]["context_frames"] == 61 and seen["kw"]["context_overlap"] == 15
    pipe(["a", "b", "c"], time_length=20, context_seconds=10, context_overlap_seconds=2.5, expand_prompts=False, seed=1)
    assert seen["shape"][0] == 1 and seen["caption"] == ["a", "b", "c"]      # one clip, a prompt per window
    pipe("a cat", time_length=20, context_seconds=10, expand_prompts=False, seed=1)
    assert "context_overlap" not in seen["kw"]
    pipe("a cat", time_length=5, expand_prompts=False, seed=1)
    assert "context_frames" not in seen["kw"]
    with pytest.raises(ValueError, match="context_seconds"):
        pipe("a cat", time_length=20, context_overlap_seconds=2.5, expand_prompts=False, seed=1)
    with pytest.raises(ValueError, match="context_seconds"):
        pipe("a cat", time_length=0, context_seconds=5, expand_prompts=False, seed=1)


def test_cli_flags_reach_the_pipeline_keywords():
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_cli_windows", os.path.join(PKG, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    assert cli.context_keywords(p.parse_args([])) == {}
    assert cli.context_keywords(p.parse_args(["--context_seconds", "10"])) == {"context_seconds": 10.0}
    assert cli.context_keywords(p.parse_args(["--context_seconds", "10", "--context_overlap_seconds", "2.5"])) == {
        "context_seconds": 10.0, "context_overlap_seconds": 2.5}
    with pytest.raises(ValueError, match="--context_seconds"):
        cli.context_keywords(p.parse_args(["--context_overlap_seconds", "2.5"]))


# ------------------------------------------------------------------------------------------ ABI
def test_header_binding_and_library_agree_on_the_new_entries(built_lib):
    from kandinsky import _engine as E
    assert_abi_entries(built_lib, ("k5_cfg_euler_windows", "k5_sample_windows"), [("k5_sample_windows_args", E.SampleWindowsArgs)])
    assert C.sizeof(E.SampleWindowsArgs) == C.sizeof(E.SampleArgs) + 8 + 4 * C.sizeof(C.c_void_p)


def test_entries_refuse_bad_arguments_without_a_gpu(built_lib):
    from kandinsky import _engine as E
    L = E.lib()
    assert L.k5_cfg_euler_windows(None, None, None, 1.0, 0.1, None, None, 1, 3, 3, 16, None) == 1
    assert "k5_cfg_euler_windows" in E.last_error()
    assert L.k5_sample_windows(None, None, None, None) == 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.cfg_euler_windows_(torch.zeros(3, 4), torch.zeros(1, 3, 4, dtype=torch.bfloat16), None, 1.0, 0.1,
                             torch.zeros(1, dtype=torch.int32), torch.ones(1, 3))
