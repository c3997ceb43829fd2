"""Skip-layer guidance, the parts that need no GPU: the per-step mask (`skip_plan`), the oracle with a skip set against itself and against the
reference's golden, the host surface (`set_skip_guidance`, `generate`, `generate_sample`, the pipeline, the CLI) with every refusal before a
model runs, and the new entries of the C ABI: header, binding and library agree, and they refuse bad arguments without a device."""
import ctypes as C
import functools
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import kit  # noqa: E402
from kit import GOLDEN, PKG, POS, assert_abi_entries, built_lib, flash_conf  # noqa: E402

CONF = flash_conf()
SHAPE = (3, 8, 12, 16)

import skip_reference as S  # noqa: E402
from kandinsky.generation_utils import edit_first_step, sigma_schedule, skip_plan  # noqa: E402
from oracle import k5_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def cfg4(golden_meta):
    return S.tiny4_config(golden_meta["tiny_config"])


def tiny4(cfg4):
    from kandinsky.models.dit import DiffusionTransformer3D
    return DiffusionTransformer3D(**cfg4)


prompt = functools.partial(kit.host_prompt, dims=(96, 48))


call_generate = functools.partial(kit.call_generate, w=5.0, steps=4, shape=SHAPE, pos=POS, conf=CONF, prompt=prompt)


# ------------------------------------------------------------------------------------------ skip_plan
def test_plan_masks():
    sig = sigma_schedule(6, 5.0).tolist()            # 1, .962, .909, .833, .714, .5, 0
    assert skip_plan(sig) == [1] * 6 == skip_plan(sig, None)
    assert skip_plan(sig, (0.6, 0.97)) == [0, 1, 1, 1, 1, 0]
    assert skip_plan(sig, (sig[2], sig[2])) == [0, 0, 1, 0, 0, 0]          # both ends belong to the interval
    assert skip_plan(sig, (2.0, 3.0)) == [0] * 6
    assert skip_plan(sig, (0.0, 1.0)) == [1] * 6
    for bad in ((0.9, 0.1), (0.5,), "ab", 3):
        with pytest.raises(ValueError, match="slg_interval"):
            skip_plan(sig, bad)
    with pytest.raises(ValueError, match="num_steps"):
        skip_plan([1.0])


def test_plan_is_cut_with_the_schedule_under_strength(cfg4):
    m = tiny4(cfg4)
    seen = []
    m.sample = lambda img, *a, **k: seen.append(m._skip)
    first = edit_first_step(6, 0.5)
    assert first == 3
    call_generate(m, steps=6, slg_blocks=[1], slg_scale=2.0, slg_interval=(0.6, 0.97), init_latent=torch.zeros(SHAPE), strength=0.5)
    assert seen[0] == ([1], 2.0, "block", [1, 1, 0]) and m._skip is None     # steps 3, 4, 5 of [0, 1, 1, 1, 1, 0]


# ------------------------------------------------------------------------------------------ oracle identities
@pytest.fixture(scope="module")
def oracle_case(golden, cfg4):
    ocfg = O.DitConfig(**cfg4)
    sd = S.tiny4_weights(cfg4)
    noise = golden["gen.noise"]
    x = torch.cat([noise, torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)], -1)
    args = (x, golden["fwd.text"], golden["fwd.pooled"], torch.tensor([700.0]), POS, torch.arange(7), (1.0, 2.0, 2.0), None, "bf16")
    return ocfg, sd, args


def test_oracle_without_a_skip_set_is_the_oracle(oracle_case):
    ocfg, sd, args = oracle_case
    assert torch.equal(S.dit_forward_skip(sd, ocfg, *args), O.dit_forward(sd, ocfg, *args))


@pytest.mark.parametrize("mode", ["block", "attention"])
def test_oracle_skip_equals_cond_when_the_skipped_gates_are_zero(oracle_case, mode):
    ocfg, sd, args = oracle_case
    D = ocfg.model_dim
    z = dict(sd)
    for b in (1, 2):   # rows of the modulation's output: [shift scale gate] x (self-attention, cross-attention, feed-forward); zero the gates
        w, bias = z[f"visual_transformer_blocks.{b}.visual_modulation.out_layer.weight"].clone(), z[f"visual_transformer_blocks.{b}.visual_modulation.out_layer.bias"].clone()
        for part in ((0,) if mode == "attention" else (0, 1, 2)):
            w[(3 * part + 2) * D:(3 * part + 3) * D] = 0
            bias[(3 * part + 2) * D:(3 * part + 3) * D] = 0
        z[f"visual_transformer_blocks.{b}.visual_modulation.out_layer.weight"], z[f"visual_transformer_blocks.{b}.visual_modulation.out_layer.bias"] = w, bias
    c = O.dit_forward(z, ocfg, *args)
    assert torch.equal(S.dit_forward_skip(z, ocfg, *args, skip=[1, 2], skip_mode=mode), c)
    assert not torch.equal(S.dit_forward_skip(sd, ocfg, *args, skip=[1, 2], skip_mode=mode), O.dit_forward(sd, ocfg, *args))


def test_loops_with_an_empty_mask_are_the_plain_loops():
    import guidance_reference as R
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(2, 4, 4, 8, generator=g)
    sig = sigma_schedule(4, 5.0)
    A, B = torch.randn(8, 8, generator=g) * 0.3, torch.randn(8, 8, generator=g) * 0.3
    c = lambda x, s: (x @ A * s).to(torch.bfloat16).float()   # noqa: E731
    u = lambda x, s: (x @ B * s).to(torch.bfloat16).float()   # noqa: E731
    never = lambda x, s: pytest.fail("an empty mask runs no skip forward")   # noqa: E731
    for kw in (dict(), dict(zero_star=True, rescale=0.7)):
        for w in (5.0, 1.0):
            if w == 1.0 and kw:
                continue
            assert torch.equal(S.bf16_loop(c, u, never, noise, sig, [w] * 4, 3.0, [0] * 4, **kw), R.bf16_loop(c, u, noise, sig, [w] * 4, **kw))
            assert torch.equal(S.published_loop(c, u, never, noise, sig, [w] * 4, 3.0, [0] * 4, **kw), R.published_loop(c, u, noise, sig, [w] * 4, **kw))
    # g = 0 on every step is the plain loop too (bf16: v + bf16(0 * d) = v)
    assert torch.equal(S.bf16_loop(c, u, u, noise, sig, [5.0] * 4, 0.0, [1] * 4), R.bf16_loop(c, u, noise, sig, [5.0] * 4))


def test_the_update_rule_in_eager_bf16_is_the_three_roundings():
    g = torch.Generator().manual_seed(5)
    c, u, s = (torch.randn(4096, generator=g).to(torch.bfloat16) for _ in range(3))
    img = torch.randn(4096, generator=g)
    for uu, w in ((u, 5.0), (None, 1.0)):
        x, v = S.skip_update(img, c, uu, s, w, 3.0, -0.037)
        base = c.float() if uu is None else S.bf(u.float() + S.bf(w * S.bf(c.float() - u.float())))
        ref = S.bf(base + S.bf(3.0 * S.bf(c.float() - s.float())))
        assert torch.equal(v.float(), ref)
        assert torch.equal(x, img + S.bf(float(np.float32(-0.037)) * ref))


def test_oracle_loop_within_tolerance_of_the_reference_golden(golden, cfg4):
    """the generator's own check, repeated from the committed files: the weights are the ones the golden was made with and each case's
    oracle-vs-golden distance is the recorded one, at most 1.5e-2"""
    from safetensors.torch import load_file
    meta = json.load(open(os.path.join(GOLDEN, "dit_tiny_skip_meta.json")))
    gold = load_file(os.path.join(GOLDEN, "dit_tiny_skip.safetensors"))
    sd = S.tiny4_weights(cfg4)
    assert S.weights_sha256(sd) == meta["weights_sha256"], "the synthetic weights drifted: regenerate tests/golden/dit_tiny_skip.*"
    assert meta["num_visual_blocks"] == 4 and meta["weight_seed"] == S.WEIGHT_SEED
    assert set(meta["cases"]) == {"block_mid", "block_first_nocfg", "attention_interval", "with_zero_star_rescale"}
    assert meta["cases"]["attention_interval"]["mask"] == [0, 1, 1, 1, 1, 0]
    assert all(d <= 1.5e-2 for d in meta["oracle_vs_golden"].values())
    ocfg = O.DitConfig(**cfg4)
    noise = golden["gen.noise"]
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)
    sig = torch.tensor(meta["sigmas"])
    te, ne = (golden["fwd.text"], golden["fwd.pooled"]), (golden["gen.null_text"], golden["gen.null_pooled"])

    def vel(cond, n, skip=(), mode="block"):
        return lambda x, s: S.dit_forward_skip(sd, ocfg, torch.cat([x, *zeros], -1), cond[0], cond[1], s.unsqueeze(0) * 1000, POS, torch.arange(n),
                                               (1.0, 2.0, 2.0), None, "bf16", skip, mode)
    name = "block_first_nocfg"          # one case here (one forward per step and branch); the GPU suite holds the engine to all four
    c = meta["cases"][name]
    x = S.bf16_loop(vel(te, 7), vel(ne, 4), vel(te, 7, c["blocks"], c["mode"]), noise, sig, [c["w"]] * meta["steps"], c["g"], c["mask"])
    d = ((x - gold[f"skip.{name}.final"]).norm() / gold[f"skip.{name}.final"].norm()).item()
    assert abs(d - meta["oracle_vs_golden"][name]) < 1e-6 and d <= 1.5e-2


# ------------------------------------------------------------------------------------------ the host surface
@pytest.mark.parametrize("bad, word", [
    (dict(blocks=[4]), "0..3"), (dict(blocks=[-1]), "0..3"), (dict(blocks=[1, 1]), "twice"), (dict(blocks=[]), "at least one"),
    (dict(blocks=[1.5]), "integer"), (dict(blocks="x"), "block"), (dict(scale=-1.0), "scale"), (dict(scale=float("nan")), "scale"),
    (dict(scale=float("inf")), "scale"), (dict(scale="much"), "scale"), (dict(mode="layer"), "mode"), (dict(steps=[]), "steps")])
def test_set_skip_guidance_refuses_bad_numbers(cfg4, bad, word):
    m = tiny4(cfg4)
    kw = dict(dict(blocks=[1], scale=3.0), **bad)
    with pytest.raises(ValueError, match=word):
        m.set_skip_guidance(kw.pop("blocks"), kw.pop("scale"), **kw)
    assert m._skip is None


def test_set_skip_guidance_is_remembered_until_the_engine_exists(cfg4):
    m = tiny4(cfg4)
    assert m.skip_state() == (False, 0, 0, 0)
    m.set_skip_guidance([2, 1], 3, mode="attention", steps=[1, 0, 2])
    assert m._skip == ([2, 1], 3.0, "attention", [1, 0, 1]) and m._handle is None
    m.clear_skip_guidance()
    assert m._skip is None
    with pytest.raises(ValueError, match="no skip set"):
        m.forward_skip(torch.zeros(SHAPE), None, None, 0.0, POS, None)
    m.set_skip_guidance([1], 3.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_skip(torch.zeros(SHAPE), None, None, 0.0, POS, None)


def test_generate_with_the_defaults_passes_nothing_to_the_model(cfg4):
    m = tiny4(cfg4)
    seen = []
    m.sample = lambda img, *a, **k: seen.append(m._skip)
    m.set_skip_guidance = m.clear_skip_guidance = lambda *a, **k: pytest.fail("the defaults must not touch the model")
    call_generate(m)
    call_generate(m, slg_blocks=None, slg_scale=0.0, slg_interval=None, slg_mode="block")
    call_generate(m, slg_blocks=[1], slg_scale=0.0)                       # scale 0, no blocks, an interval without a step: off
    call_generate(m, slg_blocks=[], slg_scale=3.0)
    call_generate(m, slg_blocks=[1], slg_scale=3.0, slg_interval=(2.0, 3.0))
    assert seen == [None] * 5


def test_generate_sets_the_skip_set_for_the_call_and_clears_it_also_on_an_exception(cfg4):
    m = tiny4(cfg4)
    seen = []

    def sample(img, *a, **k):
        seen.append(m._skip)
        if len(seen) == 2:
            raise RuntimeError("boom")

    m.sample = sample
    kw = dict(slg_blocks=[1, 2], slg_scale=3.0, slg_mode="attention", slg_interval=(0.6, 0.97))
    call_generate(m, steps=6, **kw)
    assert seen[0] == ([1, 2], 3.0, "attention", [0, 1, 1, 1, 1, 0]) and m._skip is None
    with pytest.raises(RuntimeError, match="boom"):
        call_generate(m, steps=6, **kw)
    assert m._skip is None
    m.set_skip_guidance([0], 1.5)                                          # a set that was on the model before the call is back after it
    call_generate(m, slg_blocks=[3], slg_scale=2.0)
    assert seen[2] == ([3], 2.0, "block", [1, 1, 1, 1]) and m._skip == ([0], 1.5, "block", None)


Wrapped = functools.partial(kit.Wrapped, blocks=True, refuse=True)


def test_generate_refusals(cfg4):
    m = tiny4(cfg4)
    m.sample = lambda *a, **k: pytest.fail("refused calls must not sample")
    on = dict(slg_blocks=[1], slg_scale=3.0)
    for model in (m, Wrapped(m)):
        for kw, word in ((dict(slg_blocks=[4], slg_scale=3.0), "0..3"), (dict(slg_blocks=[1, 1], slg_scale=3.0), "twice"),
                         (dict(slg_blocks=[1], slg_scale=-2.0), "scale"), (dict(slg_blocks=[1], slg_scale=float("nan")), "scale"),
                         (dict(slg_scale=-1.0), "scale"), (dict(on, slg_mode="half"), "mode"), (dict(on, slg_interval=(0.9, 0.1)), "slg_interval"),
                         (dict(on, context_frames=2, context_overlap=1), "context windows")):
            with pytest.raises(ValueError, match=word):
                call_generate(model, **kw)
    with pytest.raises(ValueError, match="forward_skip"):                  # a wrapped callable without one cannot take the skip branch
        call_generate(Wrapped(m), **on)
    m.mag_ratios = [1.0] * 8
    with pytest.raises(ValueError, match="MagCache"):
        call_generate(m, **on)
    m.mag_ratios = None
    m._cfg_pair = 0
    with pytest.raises(ValueError, match="CFG pair"):
        call_generate(m, **on)
    m._cfg_pair = None
    assert m._skip is None


def test_generate_sample_and_pipeline_keywords(cfg4, monkeypatch):
    from kandinsky import generation_utils as G
    from kandinsky import t2v_pipeline as P
    m = tiny4(cfg4)
    for kw, word in ((dict(slg_blocks=[7], slg_scale=3.0), "0..3"), (dict(slg_blocks=[1], slg_scale=-3.0), "scale"),
                     (dict(slg_blocks=[1], slg_scale=3.0, slg_mode="x"), "mode"), (dict(slg_blocks=[1], slg_scale=3.0, slg_interval=(1.0, 0.0)), "slg_interval"),
                     (dict(slg_blocks=[1], slg_scale=3.0, context_frames=2, context_overlap=1), "context windows")):
        with pytest.raises(ValueError, match=word):
            G.generate_sample((1, 3, 8, 12, 16), "a", m, None, CONF, None, **kw)
    m.mag_ratios = [1.0] * 8
    with pytest.raises(ValueError, match="MagCache"):
        G.generate_sample((1, 3, 8, 12, 16), "a", m, None, CONF, None, slg_blocks=[1], slg_scale=3.0)
    m.mag_ratios = None
    m._cfg_pair = 0
    with pytest.raises(ValueError, match="CFG pair"):
        G.generate_sample((1, 3, 8, 12, 16), "a", m, None, CONF, None, slg_blocks=[1], slg_scale=3.0)
    m._cfg_pair = None
    seen = {}

    class Embedder:
        def encode(self, prompts, type_of_content):
            return {"text_embeds": torch.zeros(4, 96), "pooled_embed": torch.zeros(1, 48)}, torch.tensor([0, 4])

        def to(self, *a):
            return self

    monkeypatch.setattr(G, "generate", lambda *a, **k: seen.update(k) or torch.zeros(3, 8, 12, 16))
    monkeypatch.setattr(G, "latent_to_uint8", lambda latent, *a: latent)
    names = ("slg_blocks", "slg_scale", "slg_interval", "slg_mode")
    G.generate_sample((1, 3, 8, 12, 16), "a cat", m, None, CONF, Embedder(), device="cpu")
    assert not any(k in seen for k in names)
    G.generate_sample((1, 3, 8, 12, 16), "a cat", m, None, CONF, Embedder(), device="cpu", slg_blocks=[1, 2], slg_scale=2.5, slg_interval=(0.2, 0.99),
                      slg_mode="attention")
    assert {k: seen[k] for k in names} == dict(slg_blocks=[1, 2], slg_scale=2.5, slg_interval=(0.2, 0.99), slg_mode="attention")

    def fake_generate_sample(shape, caption, *a, **k):
        seen.clear()
        seen.update(k)
        return torch.zeros(shape[0], 3, 4 * (shape[1] - 1) + 1, 8, 8, dtype=torch.uint8)

    monkeypatch.setattr(P, "generate_sample", fake_generate_sample)
    pipe = P.Kandinsky5T2VPipeline({"dit": "cpu", "vae": "cpu", "text_embedder": "cpu"}, m, None, None,
                                   conf=NS(model=NS(num_steps=4, guidance_weight=5.0)))
    pipe("a cat", time_length=1, expand_prompts=False, seed=1)
    assert not any(k in seen for k in names)
    pipe("a cat", time_length=1, expand_prompts=False, seed=1, slg_blocks=[2, 3], slg_scale=3.0, slg_interval=(0.2, 0.99))
    assert {k: seen[k] for k in names} == dict(slg_blocks=[2, 3], slg_scale=3.0, slg_interval=(0.2, 0.99), slg_mode="block")
    for kw, word in ((dict(slg_blocks=[9], slg_scale=3.0), "0..3"), (dict(slg_blocks=[1], slg_scale=-1.0), "scale"),
                     (dict(slg_blocks=[1], slg_scale=3.0, slg_mode="none"), "mode")):
        with pytest.raises(ValueError, match=word):
            pipe("a cat", time_length=1, expand_prompts=False, seed=1, **kw)
    with pytest.raises(ValueError, match="context"):
        pipe("a cat", time_length=2, expand_prompts=False, seed=1, slg_blocks=[1], slg_scale=3.0, context_seconds=1)


def test_cli_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_cli_skip", os.path.join(PKG, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    names = ("slg_blocks", "slg_scale", "slg_interval", "slg_mode")
    none = p.parse_args([])
    assert not any(hasattr(none, n) for n in names) and cli.skip_keywords(none) == {}
    a = p.parse_args(["--slg_blocks", "9", "10", "--slg_scale", "3.0", "--slg_interval", "0.2", "0.99", "--slg_mode", "attention"])
    assert cli.skip_keywords(a) == dict(slg_blocks=[9, 10], slg_scale=3.0, slg_interval=(0.2, 0.99), slg_mode="attention")
    assert cli.skip_keywords(p.parse_args(["--slg_blocks", "4", "--slg_scale", "2"])) == dict(slg_blocks=[4], slg_scale=2.0, slg_mode="block")
    for argv, word in ((["--slg_scale", "3"], "need --slg_blocks"), (["--slg_mode", "block"], "need --slg_blocks"), (["--slg_blocks", "9"], "needs --slg_scale"),
                       (["--slg_blocks", "9", "9", "--slg_scale", "3"], "distinct"), (["--slg_blocks", "-1", "--slg_scale", "3"], "distinct"),
                       (["--slg_blocks", "9", "--slg_scale", "-3"], "slg_scale"), (["--slg_blocks", "9", "--slg_scale", "3", "--slg_interval", "0.9", "0.2"], "LO <= HI"),
                       (["--slg_blocks", "9", "--slg_scale", "3", "--context_seconds", "5"], "context_seconds"),
                       (["--slg_blocks", "9", "--slg_scale", "3", "--magcache"], "magcache")):
        with pytest.raises(ValueError, match=word):
            cli.skip_keywords(p.parse_args(argv))
    for argv in (["--slg_interval", "0.5"], ["--slg_scale", "high"], ["--slg_blocks"], ["--slg_blocks", "a"], ["--slg_mode", "layer"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)


# ------------------------------------------------------------------------------------------ ABI
NEW = ("k5_skip_euler", "k5_dit_set_skip_guidance", "k5_dit_skip_state", "k5_dit_forward_skip")


def test_header_binding_and_library_agree_on_the_new_entries(built_lib):
    from kandinsky import _engine as E
    assert_abi_entries(built_lib, NEW, [("k5_skip_guidance", E.SkipGuidance)])


def test_entries_refuse_bad_arguments_without_a_gpu(built_lib, cfg4):
    from kandinsky import _engine as E
    L = E.lib()
    h = tiny4(cfg4)._create_handle()           # a handle is host memory until weights arrive
    try:
        blocks = (C.c_int * 3)(1, 2, 3)
        bp = C.cast(blocks, C.POINTER(C.c_int))
        steps = (C.c_ubyte * 4)(1, 0, 1, 1)
        sp = C.cast(steps, C.POINTER(C.c_ubyte))
        assert L.k5_dit_set_skip_guidance(None, C.byref(E.SkipGuidance(bp, 3, 0, 3.0, None, 0))) == 1 and "null handle" in E.last_error()
        bad = [(E.SkipGuidance(bp, 0, 0, 3.0, None, 0), "num_blocks"), (E.SkipGuidance(None, 1, 0, 3.0, None, 0), "num_blocks"),
               (E.SkipGuidance(bp, 3, 2, 3.0, None, 0), "mode"), (E.SkipGuidance(bp, 3, -1, 3.0, None, 0), "mode"),
               (E.SkipGuidance(bp, 3, 0, -1.0, None, 0), "scale"), (E.SkipGuidance(bp, 3, 0, float("nan"), None, 0), "scale"),
               (E.SkipGuidance(bp, 3, 0, float("inf"), None, 0), "scale"), (E.SkipGuidance(bp, 3, 0, 3.0, sp, 0), "num_steps")]
        for g, word in bad:
            assert L.k5_dit_set_skip_guidance(h, C.byref(g)) == 1
            assert word in E.last_error(), (word, E.last_error())
        for vals, word in (((1, 4, 2), "outside"), ((1, -1, 2), "outside"), ((1, 2, 1), "twice")):
            blocks[:] = vals
            assert L.k5_dit_set_skip_guidance(h, C.byref(E.SkipGuidance(bp, 3, 0, 3.0, None, 0))) == 1 and word in E.last_error()
        on, a, b, r = C.c_int(7), C.c_longlong(7), C.c_longlong(7), C.c_longlong(7)
        assert L.k5_dit_skip_state(h, C.byref(on), C.byref(a), C.byref(b), C.byref(r), 0) == 0
        assert (on.value, a.value, b.value, r.value) == (0, 0, 0, 0)                        # nothing of the refused calls stuck
        blocks[:] = (3, 1, 2)
        assert L.k5_dit_set_skip_guidance(h, C.byref(E.SkipGuidance(bp, 3, 1, 0.0, sp, 4))) == 0     # scale 0 is accepted and means off
        assert L.k5_dit_skip_state(h, C.byref(on), None, None, None, 0) == 0 and on.value == 0
        assert L.k5_dit_set_skip_guidance(h, C.byref(E.SkipGuidance(bp, 3, 1, 2.5, sp, 4))) == 0
        assert L.k5_dit_skip_state(h, C.byref(on), None, None, None, 0) == 0 and on.value == 1
        v = C.c_int(7)
        assert L.k5_dit_get_option(h, b"skip_share_prefix", C.byref(v)) == 0 and v.value == 1
        assert L.k5_dit_set_option(h, b"skip_share_prefix", 2) == 1
        assert L.k5_dit_set_option(h, b"skip_share_prefix", 0) == 0 and L.k5_dit_get_option(h, b"skip_share_prefix", C.byref(v)) == 0 and v.value == 0
        assert L.k5_dit_set_skip_guidance(h, None) == 0                                        # NULL clears
        assert L.k5_dit_skip_state(h, C.byref(on), None, None, None, 1) == 0 and on.value == 0
        assert L.k5_dit_skip_state(None, None, None, None, None, 0) == 1
        assert L.k5_dit_forward_skip(h, None, None, None, None) == 1
    finally:
        L.k5_dit_destroy(h)
    # the kernel entry: refused before anything is launched
    p = 0x10000
    good = [p, p, p, p, 5.0, None, 3.0, -0.1, p, p, p, 0.5, 288, 16, None, None]

    def with_(args, i, v):
        a = list(args)
        a[i] = v
        return a

    for a in ([with_(good, i, None) for i in (0, 1, 3)] + [with_(good, 6, g) for g in (0.0, -1.0, float("nan"), float("inf"))] +
              [with_(good, 12, 0), with_(good, 13, 0), with_(good, 8, None), with_(good, 9, None), with_(with_(good, 2, None), 5, p)]):
        assert L.k5_skip_euler(*a) == 1, a
        assert "k5_skip_euler" in E.last_error()
    with pytest.raises(ValueError, match="skip_euler_"):
        E.skip_euler_(torch.zeros(8), torch.zeros(8, dtype=torch.bfloat16), None, torch.zeros(8), 1.0, 3.0, -0.1)
    with pytest.raises(RuntimeError, match="GPU only"):
        z = torch.zeros(8, dtype=torch.bfloat16)
        E.skip_euler_(torch.zeros(8), z, None, z, 1.0, 3.0, -0.1)
