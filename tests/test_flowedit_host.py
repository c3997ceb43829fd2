"""FlowEdit on the host: the step classification, every ValueError of `generate` before a model runs, the restatement's two exact properties
(z_fe == x_src gives zt == zs bit for bit; equal velocities return the source), and the new entries of the C ABI: header, binding and
library agree, and every refusal of k5_flowedit_step / k5_sample_flowedit's NULL arguments is made before anything is launched, so without
a GPU.  No GPU."""
import ctypes as C
import functools
import os
from types import SimpleNamespace as NS

import pytest
import torch

import kit  # noqa: E402
from kit import PKG, POS, assert_abi_entries, built_lib, flash_conf, host_tiny  # noqa: E402

CONF = flash_conf()
SHAPE = (3, 8, 12, 16)

import flowedit_reference as FR  # noqa: E402
import stochastic_reference as SR  # noqa: E402
from kandinsky.generation_utils import edit_first_step, flowedit_plan, sigma_schedule  # noqa: E402


prompt = functools.partial(kit.host_prompt, dims=(96, 48))


call_generate = functools.partial(kit.call_generate, w=5.0, steps=4, shape=SHAPE, pos=POS, conf=CONF, prompt=prompt)


# ------------------------------------------------------------------------------------------ the step classification
@pytest.mark.parametrize("steps, strength, refine, want", [
    (6, 1.0, 0, (0, 6, 0)), (6, 1.0, 2, (0, 4, 2)), (6, 0.7, 0, (2, 4, 0)), (6, 0.7, 4, (2, 0, 4)), (50, 0.66, 0, (17, 33, 0)),
    (50, 0.66, 5, (17, 28, 5)), (4, 0.01, 1, (3, 0, 1)), (1, 1.0, 0, (0, 1, 0))])
def test_step_classification(steps, strength, refine, want):
    kinds = flowedit_plan(steps, strength, refine)
    first, n_fe, n_plain = want
    assert kinds == ["skipped"] * first + ["flowedit"] * n_fe + ["plain"] * n_plain and len(kinds) == steps
    assert first == edit_first_step(steps, strength) and FR.plan(steps, strength, refine) == want


def test_step_classification_refuses_a_refine_outside_the_steps_that_run():
    for steps, strength, refine in ((6, 1.0, 7), (6, 1.0, -1), (6, 0.5, 4), (6, 1.0, 1.5), (6, 1.0, True)):
        with pytest.raises(ValueError, match="flowedit_refine"):
            flowedit_plan(steps, strength, refine)


# ------------------------------------------------------------------------------------------ generate's refusals
Wrapped = functools.partial(kit.Wrapped, blocks=True, hand_on=("forward_skip",), refuse=True)


def test_generate_refusals(golden_meta):
    m = host_tiny(golden_meta)
    m.sample = lambda *a, **k: pytest.fail("refused calls must not sample")
    src, mask = torch.zeros(SHAPE), torch.zeros(*SHAPE[:-1], 1)
    fe = dict(init_latent=src, source_text_embeds=prompt(5, 2), source_text_rope_pos=torch.arange(5))
    W, b = torch.zeros(16, 3), torch.zeros(3)
    for model in (m, Wrapped(m)):
        for kw, word in ((dict(source_text_embeds=prompt(5, 2), source_text_rope_pos=torch.arange(5)), "needs init_latent"),
                         (dict(init_latent=src, source_text_embeds=prompt(5, 2)), "source_text_rope_pos"),
                         (dict(init_latent=src, source_guidance_weight=3.5), "need source_text_embeds"),
                         (dict(init_latent=src, flowedit_refine=1), "need source_text_embeds"),
                         (dict(init_latent=src, flowedit_seed=1), "need source_text_embeds"),
                         (dict(init_latent=src, source_text_rope_pos=torch.arange(5)), "need source_text_embeds"),
                         (dict(fe, flowedit_refine=5), "flowedit_refine"), (dict(fe, flowedit_refine=-1), "flowedit_refine"),
                         (dict(fe, strength=0.5, flowedit_refine=3), "flowedit_refine"),
                         (dict(fe, flowedit_refine=1, keep_mask=mask), "keep_mask"),
                         (dict(fe, source_guidance_weight=float("nan")), "source_guidance_weight"),
                         (dict(fe, context_frames=2, context_overlap=1), "context_frames"),
                         (dict(fe, forecast_interval=2, forecast_warmup=1), "forecast_interval"),
                         (dict(fe, slg_blocks=[1], slg_scale=2.0), "slg_blocks"),
                         (dict(fe, guidance_interval=(0.5, 0.9)), "guidance_schedule"), (dict(fe, cfg_zero_star=True), "guidance_schedule"),
                         (dict(fe, eta=1.0), "eta > 0"),
                         (dict(fe, callback=lambda i: None, preview_every=1, preview_factors=(W, b)), "preview_every")):
            with pytest.raises(ValueError, match=word):
                call_generate(model, **kw)
    for kw, word in ((dict(fe, nag_scale=5.0, nag_text_embeds=prompt(4, 3), nag_text_rope_pos=torch.arange(4)), "nag_scale"),
                     (dict(fe, region_text_embeds=[prompt(4, 3)], region_text_rope_pos=[torch.arange(4)],
                           region_masks=torch.ones(1, *SHAPE[:-1])), "region_text_embeds")):
        with pytest.raises(ValueError, match=word + ".*FlowEdit"):
            call_generate(m, **kw)
    m.mag_ratios = [1.0] * 8
    with pytest.raises(ValueError, match="MagCache"):
        call_generate(m, **fe)
    m.mag_ratios = None
    m._cfg_parallel = (0, None)
    with pytest.raises(ValueError, match="single-rank"):
        call_generate(m, **fe)
    m._cfg_parallel = None
    assert m._nag is None and m._regions is None and m._stochastic is None and m._guidance is None


def test_generate_sample_pipeline_and_cli_keywords(golden_meta, monkeypatch):
    import importlib.util
    from kandinsky import generation_utils as G
    from kandinsky import t2v_pipeline as P
    m = host_tiny(golden_meta)
    shape = (1, 3, 8, 12, 16)
    for kw, word in ((dict(source_caption="a cat"), "needs a source video"), (dict(source_guidance_weight=3.5), "need source_caption"),
                     (dict(flowedit_refine=1), "need source_caption"), (dict(flowedit_seed=1), "need source_caption"),
                     (dict(source_caption="a cat", video=torch.zeros(9, 64, 96, 3, dtype=torch.uint8), flowedit_refine=30), "flowedit_refine"),
                     (dict(source_caption=["a", "b"], video=torch.zeros(9, 64, 96, 3, dtype=torch.uint8)), "one prompt")):
        with pytest.raises(ValueError, match=word):
            G.generate_sample(shape, "a dog", m, None, CONF, None, **kw)
    seen = {}

    def fake_generate_sample(shape, caption, *a, **k):
        seen.clear()
        seen.update(k)
        return torch.zeros(shape[0], 3, 4 * (shape[1] - 1) + 1, 8, 8, dtype=torch.uint8)

    monkeypatch.setattr(P, "generate_sample", fake_generate_sample)
    pipe = P.Kandinsky5T2VPipeline({"dit": "cpu", "vae": "cpu", "text_embedder": "cpu"}, m, None, None,
                                   conf=NS(model=NS(num_steps=4, guidance_weight=5.0)))
    names = ("source_caption", "source_guidance_weight", "flowedit_refine", "flowedit_seed")
    clip = torch.zeros(5, 64, 64, 3, dtype=torch.uint8)
    pipe("a dog", time_length=1, expand_prompts=False, seed=1, video=clip)
    assert not any(k in seen for k in names)                               # without a source prompt: the SDEdit path's keywords, exactly
    pipe("a dog", time_length=1, expand_prompts=False, seed=1, video=clip, source_caption="a cat", source_guidance_weight=3.5, flowedit_refine=1)
    assert {k: seen[k] for k in names} == dict(source_caption="a cat", source_guidance_weight=3.5, flowedit_refine=1, flowedit_seed=None)
    with pytest.raises(ValueError, match="need source_caption"):
        pipe("a dog", time_length=1, expand_prompts=False, seed=1, video=clip, flowedit_refine=1)

    spec = importlib.util.spec_from_file_location("k5_cli_flowedit", os.path.join(PKG, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    assert cli.flowedit_keywords(p.parse_args([])) == {}
    a = p.parse_args(["--video", "c.mp4", "--source_prompt", "a cat", "--source_guidance", "3.5", "--flowedit_refine", "2", "--flowedit_seed", "7"])
    assert cli.flowedit_keywords(a) == dict(source_caption="a cat", source_guidance_weight=3.5, flowedit_refine=2, flowedit_seed=7)
    assert cli.flowedit_keywords(p.parse_args(["--video", "c.mp4", "--source_prompt", "a cat"])) == dict(source_caption="a cat")
    for argv, word in ((["--source_guidance", "2"], "need --source_prompt"), (["--flowedit_refine", "1"], "need --source_prompt"),
                       (["--source_prompt", "a cat"], "needs --video"),
                       (["--video", "c.mp4", "--source_prompt", "a", "--flowedit_refine", "-1"], "flowedit_refine"),
                       (["--video", "c.mp4", "--source_prompt", "a", "--eta", "1"], "--eta"),
                       (["--video", "c.mp4", "--source_prompt", "a", "--magcache"], "magcache")):
        with pytest.raises(ValueError, match=word):
            cli.flowedit_keywords(p.parse_args(argv))


# ------------------------------------------------------------------------------------------ the restatement
def test_zt_equals_zs_bit_for_bit_while_z_fe_is_the_source():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(SHAPE, generator=g) * 3.0
    for i, s in enumerate((1.0, 0.962, 0.5, 0.123, 1e-3)):
        z = SR.normals_f32(SHAPE, 11, i)
        z_fe, zs, zt = FR.flowedit_pass(x.clone(), x, sigma_next=s, z=z)
        assert torch.equal(zt, zs) and torch.equal(z_fe, x)
        assert torch.equal(zs, (1.0 - torch.tensor(s)) * x + torch.tensor(s) * z)     # k5_edit_renoise's expression, op by op
    # the other order of the same sum does not have the property: that is why the rule fixes it
    z_fe = x + 1e-3
    s = 0.5
    zs = FR.renoise(x, SR.normals_f32(SHAPE, 11, 0), s)
    assert not torch.equal((zs + z_fe) - x, FR.target(zs, z_fe, x))


def test_update_rounding_points_and_the_mask():
    g = torch.Generator().manual_seed(6)
    BF = torch.bfloat16
    z = torch.randn(SHAPE, generator=g)
    cs, us, ct, ut = (torch.randn(SHAPE, generator=g).to(BF) for _ in range(4))
    dt = -0.0384
    out = FR.update(z, cs, us, ct, ut, 3.5, 13.5, dt)
    v = lambda c, u, w: (u.float() + (FR.f32(w) * (c.float() - u.float()).to(BF).float()).to(BF).float()).to(BF).float()   # noqa: E731
    d = (v(ct, ut, 13.5) - v(cs, us, 3.5)).to(BF).float()
    assert torch.equal(out, z + (FR.f32(dt) * d).to(BF).float())
    assert torch.equal(FR.update(z, cs, None, ct, None, 1.0, 1.0, dt), z + (FR.f32(dt) * (ct.float() - cs.float()).to(BF).float()).to(BF).float())
    assert torch.equal(FR.update(z, cs, us, cs, us, 5.0, 5.0, dt), z)                 # equal velocities: nothing moves
    m = torch.zeros(*SHAPE[:-1], 1)
    m[0], m[1, :, :3] = 1.0, 0.25
    masked = FR.update(z, cs, us, ct, ut, 3.5, 13.5, dt, m)
    assert torch.equal(masked[0], z[0]) and torch.equal(masked[2], out[2])
    e = (FR.f32(dt) * d).to(BF).float()
    assert torch.equal(masked[1, :, :3], z[1, :, :3] + 0.75 * e[1, :, :3])


def test_published_loop_with_equal_velocities_returns_the_source():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(SHAPE, generator=g)
    sig = sigma_schedule(6, 5.0).tolist()
    z_at = SR.step_noise(SHAPE, 3)
    vel = lambda x, s: torch.tanh(x) * s                   # noqa: E731 — any velocity field, the same for both prompts
    null = lambda x, s: torch.cos(x) - s                   # noqa: E731
    for w, first, refine in ((1.0, 0, 0), (5.0, 0, 0), (5.0, 2, 0)):
        out = FR.published_loop(vel, null, vel, x, sig, w, w, z_at, first, refine)
        assert torch.equal(out, x), (w, first)
    # ... and the engine's loop restated: bit for bit as well, through the order of zt's sum
    bvel = lambda x, s: FR.bf(torch.tanh(x) * s)           # noqa: E731
    bnull = lambda x, s: FR.bf(torch.cos(x) - s)           # noqa: E731
    for w, first in ((1.0, 0), (5.0, 0), (5.0, 2)):
        assert torch.equal(FR.bf16_loop(bvel, bnull, bvel, x, sig, w, w, z_at, first, 0), x)
    # different prompts move it, the mask holds the kept cells, refine steps run on zt
    other = lambda x, s: FR.bf(torch.tanh(x) * s + 0.5)    # noqa: E731
    m = torch.zeros(*SHAPE[:-1], 1)
    m[0] = 1.0
    out = FR.bf16_loop(bvel, bnull, other, x, sig, 2.0, 5.0, z_at, 2, 0, m)
    assert torch.equal(out[0], x[0]) and not torch.equal(out[1], x[1])
    a, b = (f(lambda x, s: torch.tanh(x) * s, null, lambda x, s: torch.tanh(x) * s + 0.5, x, sig, 2.0, 5.0, z_at, 1, 2)
            for f in (FR.published_loop, lambda *a: FR.bf16_loop(bvel, bnull, other, *a[3:])))
    assert ((a - b).norm() / (a - x).norm()).item() < 2e-2                           # the two loops describe the same run


# ------------------------------------------------------------------------------------------ ABI
NEW = ("k5_flowedit_step", "k5_sample_flowedit", "k5_dit_flowedit_state")


def test_header_binding_and_library_agree_on_the_new_entries(built_lib):
    from kandinsky import _engine as E
    assert_abi_entries(built_lib, NEW, [("k5_flowedit_step_args", E.FlowEditStep), ("k5_flowedit_args", E.FlowEditArgs)])


def test_entries_refuse_bad_arguments_without_a_gpu(built_lib, golden_meta):
    from kandinsky import _engine as E
    L = E.lib()
    p = 0x10000

    def good(**kw):
        a = dict(z_fe=p, x_src=p, c_src=p, u_src=p, c_tar=p, u_tar=p, w_src=3.5, w_tar=13.5, dt=-0.1, keep_mask=p, prepare=1, sigma_next=0.5, zs=p,
                 zt=p, znoise=None, seed=1, stream_id=0, cells=288, C=16)
        a.update(kw)
        return E.FlowEditStep(**a)

    assert L.k5_flowedit_step(None, None) == 1 and "args is NULL" in E.last_error()
    for kw, word in ((dict(z_fe=None), "z_fe is NULL"), (dict(x_src=None), "x_src is NULL"), (dict(cells=0), "cells and C"), (dict(C=0), "cells and C"),
                     (dict(c_src=None), "go together"), (dict(c_tar=None), "go together"),
                     (dict(c_src=None, c_tar=None, prepare=0), "nothing to do"),
                     (dict(u_src=None), "w_src != 1 needs u_src"), (dict(u_tar=None), "w_tar != 1 needs u_tar"),
                     (dict(zs=None), "needs zs and zt"), (dict(zt=None), "needs zs and zt"),
                     (dict(z_fe=p + 2), "4-byte aligned"), (dict(x_src=p + 1), "4-byte aligned"), (dict(c_src=p + 2), "4-byte aligned"),
                     (dict(u_tar=p + 2), "4-byte aligned"), (dict(keep_mask=p + 2), "4-byte aligned"), (dict(zs=p + 3), "4-byte aligned"),
                     (dict(znoise=p + 2), "4-byte aligned")):
        assert L.k5_flowedit_step(C.byref(good(**kw)), None) == 1, kw
        assert "k5_flowedit_step" in E.last_error() and word in E.last_error(), (kw, E.last_error())
    assert L.k5_dit_flowedit_state(None, None, None, None, 0) == 1 and "null handle" in E.last_error()
    h = host_tiny(golden_meta)._create_handle()           # a handle is host memory until weights arrive
    try:
        s, f, t = C.c_longlong(7), C.c_longlong(7), C.c_longlong(7)
        assert L.k5_dit_flowedit_state(h, C.byref(s), C.byref(f), C.byref(t), 1) == 0 and (s.value, f.value, t.value) == (0, 0, 0)
        assert L.k5_sample_flowedit(h, None, None, None, None) == 1 and "k5_sample_flowedit" in E.last_error()
    finally:
        L.k5_dit_destroy(h)
    with pytest.raises(ValueError, match="flowedit_step_"):
        E.flowedit_step_(torch.zeros(8), torch.zeros(8, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="flowedit_step_"):
        E.flowedit_step_(torch.zeros(8), torch.zeros(8), torch.zeros(8), None, torch.zeros(8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="GPU only"):
        E.flowedit_step_(torch.zeros(8), torch.zeros(8), sigma_next=0.5, zs=torch.zeros(8), zt=torch.zeros(8))
