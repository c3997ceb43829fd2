"""Stochastic sampling, the parts that need no GPU: known answers of the Philox4x32-10 restatement, the per-step rule (`stochastic_plan`)
against its float64 restatement, the host surface (`set_stochastic`, `generate`, `generate_sample`, the pipeline, the CLI) with every
ValueError before a model runs, the settings round trip on a model without an engine, and the new entries of the C ABI: header, binding and
library agree, and they refuse bad arguments without a device."""
import ctypes as C
import functools
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import kit  # noqa: E402
from kit import GOLDEN, PKG, POS, assert_abi_entries, built_lib, flash_conf, host_tiny  # noqa: E402

CONF = flash_conf()
SHAPE = (3, 8, 12, 16)

import stochastic_reference as SR  # noqa: E402
from kandinsky.generation_utils import edit_first_step, sigma_schedule, stochastic_plan  # noqa: E402


prompt = functools.partial(kit.host_prompt, dims=(96, 48))


call_generate = functools.partial(kit.call_generate, w=5.0, steps=4, shape=SHAPE, pos=POS, conf=CONF, prompt=prompt)


# ------------------------------------------------------------------------------------------ the generator's restatement
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr, key, want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    got = " ".join("%08x" % int(w) for w in SR.philox4x32_10(*ctr, *key))
    assert got == want
    # ... and through the block / seed layout of k5_philox_words
    words = SR.philox_words(ctr[0] | (ctr[1] << 32), 1, key[0] | (key[1] << 32), ctr[2], ctr[3])
    assert words.dtype == np.uint32 and " ".join("%08x" % int(w) for w in words[0]) == want


def test_block_index_wraps_and_carries():
    w = SR.philox_words(2 ** 64 - 2, 4, 5)                              # ... 2^64 - 1, then 0, 1
    assert np.array_equal(w[2:], SR.philox_words(0, 2, 5))
    w = SR.philox_words(2 ** 32 - 1, 2, 5)                              # the carry into the high counter word
    assert " ".join("%08x" % int(x) for x in w[1]) == " ".join("%08x" % int(x) for x in SR.philox4x32_10(0, 1, 0, 0, 5, 0))


def test_normals_are_the_blocks_in_order_and_look_normal():
    z = SR.normals_f64(2 ** 16 + 3, 6554)
    assert np.array_equal(z[:1001], SR.normals_f64(1001, 6554)) and z.shape == (2 ** 16 + 3,)
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.8              # u >= 2^-24: sqrt(-2 ln u) <= 5.77
    se = 2.0 ** -8
    assert abs(z.mean()) < 4 * se and abs(z.var() - 1) / np.sqrt(2) < 4 * se
    assert not np.array_equal(z[:64], SR.normals_f64(64, 6554, 1)) and not np.array_equal(z[:64], SR.normals_f64(64, 6555))


# ------------------------------------------------------------------------------------------ stochastic_plan
def test_eta_zero_is_the_plain_step_exactly():
    sig = sigma_schedule(6, 5.0).tolist()
    f = np.asarray(sig, dtype=np.float32)
    want = ([float(f[i + 1] - f[i]) for i in range(6)], [1.0] * 6, [0.0] * 6)
    assert stochastic_plan(sig, 0.0) == want
    assert stochastic_plan(sig, 1.0, interval=(2.0, 3.0)) == want       # an interval without a step
    assert stochastic_plan(sig, 1.0, s_noise=0.0) == want               # c == 0: the plain step
    assert stochastic_plan(sig, 0.0, 3.0, (0.0, 1.0)) == want


def test_the_rule_and_its_rounding():
    sig = sigma_schedule(6, 5.0).tolist()
    for eta, s_noise, interval in ((1.0, 1.0, None), (0.5, 1.0, (0.6, 0.97)), (0.3, 0.7, None), (1.0, 1.3, (0.0, 0.95))):
        got = stochastic_plan(sig, eta, s_noise, interval)
        assert got == SR.tables_f32(sig, eta, s_noise, interval)
        assert all(float(np.float32(v)) == v for t in got for v in t)   # fp32 values
        assert got[1][-1] == 1.0 and got[2][-1] == 0.0                  # the last step ends at 0: never stochastic
        noisy = [c != 0.0 for c in got[2]]
        lo, hi = interval if interval else (0.0, 2.0)
        assert noisy == [lo <= sig[i] <= hi and i < 5 for i in range(6)]
    dt, a, c = stochastic_plan(sig, 1.0)
    assert all(abs(dt[i] - (sig[i + 1] ** 2 / sig[i] - sig[i])) < 1e-6 for i in range(5))    # eta = 1: sigma_down = t^2 / s


def test_variance_identity_and_ranges_on_every_config():
    configs = json.load(open(os.path.join(GOLDEN, "configs_parsed.json")))
    assert len(configs) == 8
    # the config's own scale where it names one, and the defaults of the CLI (5) and of the pipeline (10)
    runs = {(c["model"]["num_steps"], s) for c in configs.values() for s in (float(c["metrics"].get("scheduler_scale", 10.0)), 5.0, 10.0)}
    for steps, scale in sorted(runs):
        sig = sigma_schedule(steps, scale).tolist()
        for eta in (0.25, 1.0):
            for i, (down, a, c) in enumerate(SR.plan_f64(sig, eta)):
                t = sig[i + 1]
                assert c >= 0.0 and 1.0 - down > 0.0, (steps, scale, i)
                assert abs(a * a * down * down + c * c - t * t) <= 1e-12, (steps, scale, i)
            dt, sc, co = stochastic_plan(sig, eta)
            assert all(v >= 0.0 for v in co) and all(np.isfinite(v) for t in (dt, sc, co) for v in t)
            assert sum(1 for v in co if v != 0.0) == len(co) - 1


def test_plan_refuses_bad_numbers():
    sig = sigma_schedule(4, 5.0).tolist()
    for eta in (-0.1, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="eta"):
            stochastic_plan(sig, eta)
    for s in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="s_noise"):
            stochastic_plan(sig, 1.0, s)
    for bad in ((0.9, 0.1), (0.5,), "ab", 3):
        with pytest.raises(ValueError, match="sde_interval"):
            stochastic_plan(sig, 1.0, 1.0, bad)
    with pytest.raises(ValueError, match="num_steps"):
        stochastic_plan([1.0], 1.0)


def test_plan_is_cut_with_the_schedule_under_strength(golden_meta):
    m = host_tiny(golden_meta)
    seen = []
    m.sample = lambda img, *a, **k: seen.append(m._stochastic)
    assert edit_first_step(6, 0.5) == 3
    call_generate(m, steps=6, eta=1.0, sde_interval=(0.6, 0.97), sde_seed=9, init_latent=torch.zeros(SHAPE), strength=0.5)
    full = stochastic_plan(sigma_schedule(6, 5.0).tolist(), 1.0, 1.0, (0.6, 0.97))
    assert seen[0] == (full[0][3:], full[1][3:], full[2][3:], 9, 0) and m._stochastic is None
    assert [c != 0.0 for c in seen[0][2]] == [True, True, False]        # steps 3, 4, 5 of the full plan [0, 1, 1, 1, 1, 0]


# ------------------------------------------------------------------------------------------ the loops' identities
def test_loops_without_noise_are_the_plain_loops():
    import guidance_reference as R
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(2, 4, 4, 16, generator=g)
    A, B = torch.randn(16, 16, generator=g) * 0.2, torch.randn(16, 16, generator=g) * 0.2
    cond = lambda x, s: (x @ A) * float(s)          # noqa: E731
    unc = lambda x, s: (x @ B) * float(s)           # noqa: E731
    sig = sigma_schedule(4, 5.0)
    z_at = lambda i: pytest.fail("no step draws noise")   # noqa: E731
    got = SR.published_loop(cond, unc, None, noise, sig, [5.0] * 4, SR.plan_f64(sig.tolist(), 0.0), z_at)
    assert torch.allclose(got, R.published_loop(cond, unc, noise, sig, [5.0] * 4), rtol=0, atol=1e-6)
    bcond, bunc = (lambda x, s: SR.bf(cond(x, s))), (lambda x, s: SR.bf(unc(x, s)))
    got = SR.bf16_loop(bcond, bunc, None, noise, sig, [5.0] * 4, SR.tables_f32(sig.tolist(), 0.0), z_at)
    assert torch.equal(got, R.bf16_loop(bcond, bunc, noise, sig, [5.0] * 4))
    # eta = 1 at a velocity that is exact for x0 = 0 (v = x / sigma): the latent stays pure noise of standard deviation sigma
    x = SR.published_loop(lambda x, s: x / float(s), None, None, torch.randn(64, 64, generator=g), sig, [1.0] * 4, SR.plan_f64(sig.tolist(), 1.0),
                          SR.step_noise((64, 64), 7))
    assert float(x.abs().max()) < 1e-6                                   # the last step lands on x0 = 0
    sig3 = sig[:4]                                                       # ... and one step earlier its spread is sigmas[3]
    x = SR.published_loop(lambda x, s: x / float(s), None, None, torch.randn(64, 64, generator=g), sig3, [1.0] * 3,
                          SR.plan_f64(sig.tolist(), 1.0)[:3], SR.step_noise((64, 64), 7))
    assert abs(float(x.std()) / float(sig[3]) - 1.0) < 0.05


# ------------------------------------------------------------------------------------------ the host surface
def test_set_stochastic_checks_and_round_trip_without_an_engine(golden_meta):
    from kandinsky.models.dit import _SETTINGS, check_stochastic_args
    m = host_tiny(golden_meta)
    assert "stochastic" in _SETTINGS and _SETTINGS["stochastic"][:2] == ("_stochastic", "k5_dit_set_stochastic")
    assert m.stochastic_state() == (False, 0)
    m.set_stochastic([-0.1, -0.2], [0.5, 1], [0.25, 0], seed=2 ** 64 + 5, first_stream=3)
    assert m._stochastic == ([-0.1, -0.2], [0.5, 1.0], [0.25, 0.0], 5, 3) and m._handle is None
    kept = m._stochastic
    with m.setting_for_call("stochastic", ([-0.3], [1.0], [0.0], 7)):
        assert m._stochastic == ([-0.3], [1.0], [0.0], 7, 0)
    assert m._stochastic is kept                                         # the stored object itself is back
    with m.setting_for_call("stochastic", None):
        assert m._stochastic is kept
    m.clear_stochastic()
    assert m._stochastic is None
    with pytest.raises(RuntimeError, match="boom"):
        with m.setting_for_call("stochastic", ([-0.3], [1.0], [0.5], 7)):
            raise RuntimeError("boom")
    assert m._stochastic is None
    args, keep = m._marshal_stochastic(check_stochastic_args([-0.5, -0.25], [0.5, 1.0], [0.75, 0.0], 2 ** 40 + 1, 2))
    p = args[0]._obj
    assert (p.num_steps, p.seed, p.first_stream) == (2, 2 ** 40 + 1, 2)
    assert [p.dt_down[i] for i in range(2)] == [-0.5, -0.25] and [p.noise_coef[i] for i in range(2)] == [0.75, 0.0] and p.scale[0] == 0.5
    for bad, word in ((([], [], [], 1), "one value per step"), (([-0.1], [1.0, 1.0], [0.0], 1), "one value per step"),
                      (([float("nan")], [1.0], [0.0], 1), "finite"), (([-0.1], [float("inf")], [0.0], 1), "finite"),
                      (([-0.1], [1.0], [-0.5], 1), ">= 0"), (("ab", [1.0], [0.0], 1), "sequences of numbers"),
                      (([-0.1], [1.0], [0.0], 1.5), "integers"), (([-0.1], [1.0], [0.0], "x"), "integers"),
                      (([-0.1], [1.0], [0.0], 1, -1), "first_stream"), (([-0.1], [1.0], [0.0], 1, 2 ** 32 - 1), "first_stream")):
        with pytest.raises(ValueError, match=word):
            m.set_stochastic(*bad)
    assert m._stochastic is None


def test_generate_with_the_defaults_passes_nothing_to_the_model(golden_meta):
    m = host_tiny(golden_meta)
    seen = []
    m.sample = lambda img, *a, **k: seen.append(m._stochastic)
    m.set_stochastic = m.clear_stochastic = lambda *a, **k: pytest.fail("the defaults must not touch the model")
    call_generate(m)
    call_generate(m, eta=0.0, s_noise=1.0, sde_interval=None, sde_seed=None)
    call_generate(m, eta=0.0, s_noise=2.0, sde_seed=3)                  # eta 0, an interval without a step, noise scale 0: off
    call_generate(m, eta=1.0, sde_interval=(2.0, 3.0))
    call_generate(m, eta=1.0, s_noise=0.0)
    assert seen == [None] * 5


def test_generate_sets_the_plan_for_the_call_and_clears_it_also_on_an_exception(golden_meta):
    m = host_tiny(golden_meta)
    seen = []

    def sample(img, *a, **k):
        seen.append(m._stochastic)
        if len(seen) == 2:
            raise RuntimeError("boom")

    m.sample = sample
    sig = sigma_schedule(6, 5.0).tolist()
    call_generate(m, steps=6, eta=0.5, s_noise=0.9, sde_interval=(0.6, 0.97))
    assert seen[0] == (*stochastic_plan(sig, 0.5, 0.9, (0.6, 0.97)), 6554, 0) and m._stochastic is None     # sde_seed defaults to seed
    with pytest.raises(RuntimeError, match="boom"):
        call_generate(m, steps=6, eta=1.0, sde_seed=11)
    assert seen[1][3] == 11 and m._stochastic is None
    m.set_stochastic([-1.0], [1.0], [0.0], 4)                            # a plan that was on the model before the call is back after it
    call_generate(m, steps=6, eta=1.0, sde_seed=2 ** 64 + 1)
    assert seen[2] == (*stochastic_plan(sig, 1.0), 1, 0) and m._stochastic == ([-1.0], [1.0], [0.0], 4, 0)


def test_a_batch_runs_one_sample_at_a_time_with_a_seed_each(golden_meta):
    from kandinsky.generation_utils import generate
    m = host_tiny(golden_meta)
    seen = []
    m.sample = lambda img, *a, **k: seen.append(m._stochastic[3])
    m.sample_many = lambda *a, **k: pytest.fail("one plan holds one seed: the batch must not go through sample_many")
    m.many_ready = lambda: True
    generate(m, "cpu", (9, 8, 12, 16), 4, prompt(7), prompt(4, 1), POS, torch.arange(7), torch.arange(4), 5.0, 5.0, CONF, noise=torch.zeros(9, 8, 12, 16),
             batch=3, eta=1.0, sde_seed=2 ** 64 - 1)
    assert seen == [2 ** 64 - 1, 0, 1]


Wrapped = functools.partial(kit.Wrapped, blocks=True, refuse=True)


def test_generate_refusals(golden_meta):
    m = host_tiny(golden_meta)
    m.sample = lambda *a, **k: pytest.fail("refused calls must not sample")
    W, b = torch.zeros(16, 3), torch.zeros(3)
    for model in (m, Wrapped(m)):
        for kw, word in ((dict(eta=-0.5), "eta"), (dict(eta=1.5), "eta"), (dict(eta=float("nan")), "eta"), (dict(eta=1.0, s_noise=-1.0), "s_noise"),
                         (dict(eta=1.0, s_noise=float("inf")), "s_noise"), (dict(eta=0.0, s_noise=float("nan")), "s_noise"),
                         (dict(eta=1.0, sde_interval=(0.9, 0.1)), "sde_interval"), (dict(eta=0.0, sde_interval=(0.5,)), "sde_interval"),
                         (dict(eta=1.0, sde_seed=1.5), "integers"),
                         (dict(eta=1.0, context_frames=2, context_overlap=1), "context windows"),
                         (dict(eta=1.0, callback=lambda i: None, preview_every=1, preview_factors=(W, b)), "preview")):
            with pytest.raises(ValueError, match=word):
                call_generate(model, **kw)
    m.mag_ratios = [1.0] * 8
    with pytest.raises(ValueError, match="MagCache"):
        call_generate(m, eta=1.0)
    m.mag_ratios = None
    m._magcache_calibrate = object()
    with pytest.raises(ValueError, match="MagCache"):
        call_generate(m, eta=1.0)
    m._magcache_calibrate = None
    assert m._stochastic is None


def test_generate_sample_and_pipeline_keywords(golden_meta, monkeypatch):
    from kandinsky import generation_utils as G
    from kandinsky import t2v_pipeline as P
    m = host_tiny(golden_meta)
    for kw, word in ((dict(eta=2.0), "eta"), (dict(eta=1.0, s_noise=-3.0), "s_noise"), (dict(eta=1.0, sde_interval=(1.0, 0.0)), "sde_interval"),
                     (dict(eta=1.0, context_frames=2, context_overlap=1), "context windows"), (dict(eta=1.0, preview_every=2), "preview")):
        with pytest.raises(ValueError, match=word):
            G.generate_sample((1, 3, 8, 12, 16), "a", m, None, CONF, None, **kw)
    m.mag_ratios = [1.0] * 8
    with pytest.raises(ValueError, match="MagCache"):
        G.generate_sample((1, 3, 8, 12, 16), "a", m, None, CONF, None, eta=0.5)
    m.mag_ratios = None
    seen = {}

    class Embedder:
        def encode(self, prompts, type_of_content):
            return {"text_embeds": torch.zeros(4, 96), "pooled_embed": torch.zeros(1, 48)}, torch.tensor([0, 4])

        def to(self, *a):
            return self

    monkeypatch.setattr(G, "generate", lambda *a, **k: seen.update(k) or torch.zeros(3, 8, 12, 16))
    monkeypatch.setattr(G, "latent_to_uint8", lambda latent, *a: latent)
    names = ("eta", "s_noise", "sde_interval", "sde_seed")
    G.generate_sample((1, 3, 8, 12, 16), "a cat", m, None, CONF, Embedder(), device="cpu")
    assert not any(k in seen for k in names)
    G.generate_sample((1, 3, 8, 12, 16), "a cat", m, None, CONF, Embedder(), device="cpu", eta=0.5, s_noise=0.9, sde_interval=(0.2, 0.99), sde_seed=4)
    assert {k: seen[k] for k in names} == dict(eta=0.5, s_noise=0.9, sde_interval=(0.2, 0.99), sde_seed=4)

    def fake_generate_sample(shape, caption, *a, **k):
        seen.clear()
        seen.update(k)
        return torch.zeros(shape[0], 3, 4 * (shape[1] - 1) + 1, 8, 8, dtype=torch.uint8)

    monkeypatch.setattr(P, "generate_sample", fake_generate_sample)
    pipe = P.Kandinsky5T2VPipeline({"dit": "cpu", "vae": "cpu", "text_embedder": "cpu"}, m, None, None,
                                   conf=NS(model=NS(num_steps=4, guidance_weight=5.0)))
    pipe("a cat", time_length=1, expand_prompts=False, seed=1)
    assert not any(k in seen for k in names)
    pipe("a cat", time_length=1, expand_prompts=False, seed=1, eta=1.0, sde_interval=(0.2, 0.99))
    assert {k: seen[k] for k in names} == dict(eta=1.0, s_noise=1.0, sde_interval=(0.2, 0.99), sde_seed=None)
    for kw, word in ((dict(eta=-1.0), "eta"), (dict(eta=1.0, s_noise=-1.0), "s_noise"), (dict(eta=1.0, sde_interval=(2.0, 1.0)), "sde_interval")):
        with pytest.raises(ValueError, match=word):
            pipe("a cat", time_length=1, expand_prompts=False, seed=1, **kw)
    with pytest.raises(ValueError, match="context"):
        pipe("a cat", time_length=2, expand_prompts=False, seed=1, eta=1.0, context_seconds=1)


def test_cli_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_cli_stochastic", os.path.join(PKG, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    names = ("eta", "s_noise", "sde_interval", "sde_seed")
    none = p.parse_args([])
    assert not any(hasattr(none, n) for n in names) and cli.stochastic_keywords(none) == {}
    a = p.parse_args(["--eta", "0.5", "--s_noise", "0.9", "--sde_interval", "0.2", "0.99", "--sde_seed", "7"])
    assert cli.stochastic_keywords(a) == dict(eta=0.5, s_noise=0.9, sde_interval=(0.2, 0.99), sde_seed=7)
    assert cli.stochastic_keywords(p.parse_args(["--eta", "1"])) == dict(eta=1.0)
    for argv, word in ((["--s_noise", "1"], "need --eta"), (["--sde_seed", "1"], "need --eta"), (["--sde_interval", "0", "1"], "need --eta"),
                       (["--eta", "1.5"], "eta"), (["--eta", "-0.1"], "eta"), (["--eta", "1", "--s_noise", "-1"], "s_noise"),
                       (["--eta", "1", "--sde_interval", "0.9", "0.2"], "LO <= HI"), (["--eta", "1", "--context_seconds", "5"], "context_seconds"),
                       (["--eta", "1", "--magcache"], "magcache"), (["--eta", "1", "--preview", "dir"], "preview")):
        with pytest.raises(ValueError, match=word):
            cli.stochastic_keywords(p.parse_args(argv))
    for argv in (["--sde_interval", "0.5"], ["--eta", "high"], ["--eta"], ["--sde_seed", "1.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)


# ------------------------------------------------------------------------------------------ ABI
NEW = ("k5_philox_words", "k5_noise_normal_f32", "k5_stochastic_euler", "k5_dit_set_stochastic", "k5_dit_stochastic_state")


def test_header_binding_and_library_agree_on_the_new_entries(built_lib):
    from kandinsky import _engine as E
    assert_abi_entries(built_lib, NEW, [("k5_stochastic", E.Stochastic)])


def test_entries_refuse_bad_arguments_without_a_gpu(built_lib, golden_meta):
    from kandinsky import _engine as E
    L = E.lib()
    fl = lambda *v: C.cast((C.c_float * len(v))(*v), C.POINTER(C.c_float))   # noqa: E731
    good = lambda: E.Stochastic(2, fl(-0.5, -0.5), fl(0.5, 1.0), fl(0.7, 0.0), 9, 0)   # noqa: E731
    assert L.k5_dit_set_stochastic(None, C.byref(good())) == 1 and "null handle" in E.last_error()      # a NULL handle, without a GPU
    assert L.k5_dit_stochastic_state(None, None, None, 0) == 1 and "null handle" in E.last_error()
    h = host_tiny(golden_meta)._create_handle()           # a handle is host memory until weights arrive
    try:
        bad = [(E.Stochastic(0, fl(0.0), fl(1.0), fl(0.0), 1, 0), "num_steps"), (E.Stochastic(2, None, fl(1.0, 1.0), fl(0.0, 0.0), 1, 0), "num_steps"),
               (E.Stochastic(2, fl(-0.5, -0.5), None, fl(0.0, 0.0), 1, 0), "num_steps"), (E.Stochastic(2, fl(-0.5, -0.5), fl(1.0, 1.0), None, 1, 0), "num_steps"),
               (E.Stochastic(2, fl(-0.5, float("nan")), fl(1.0, 1.0), fl(0.0, 0.0), 1, 0), "step 1"),
               (E.Stochastic(2, fl(-0.5, -0.5), fl(float("inf"), 1.0), fl(0.0, 0.0), 1, 0), "step 0"),
               (E.Stochastic(2, fl(-0.5, -0.5), fl(1.0, 1.0), fl(0.0, -0.25), 1, 0), "noise_coef >= 0")]
        for p, word in bad:
            assert L.k5_dit_set_stochastic(h, C.byref(p)) == 1
            assert word in E.last_error(), (word, E.last_error())
        on, n = C.c_int(7), C.c_longlong(7)
        assert L.k5_dit_stochastic_state(h, C.byref(on), C.byref(n), 0) == 0 and (on.value, n.value) == (0, 0)     # nothing of the refused calls stuck
        assert L.k5_dit_set_stochastic(h, C.byref(good())) == 0
        assert L.k5_dit_stochastic_state(h, C.byref(on), None, 0) == 0 and on.value == 1
        assert L.k5_dit_set_stochastic(h, None) == 0                                                                  # NULL clears
        assert L.k5_dit_stochastic_state(h, C.byref(on), C.byref(n), 1) == 0 and (on.value, n.value) == (0, 0)
    finally:
        L.k5_dit_destroy(h)
    # the kernel entries: refused before anything is launched
    p = 0x10000
    assert L.k5_philox_words(None, 0, 4, 1, 0, 0, None) == 1 and "k5_philox_words" in E.last_error()
    assert L.k5_philox_words(p, 0, 0, 1, 0, 0, None) == 1
    assert L.k5_noise_normal_f32(None, 4, 1, 0, None) == 1 and "k5_noise_normal_f32" in E.last_error()
    assert L.k5_noise_normal_f32(p, 0, 1, 0, None) == 1
    #        img cond unc skip  w   ab    g   dt_down src eps mask sig  cells C  v_out scale coef noise seed stream hipstream
    good = [p, p, p, p, 5.0, None, 3.0, -0.1, p, p, p, 0.5, 288, 16, None, 0.5, 0.7, None, 1, 0, None]

    def with_(args, i, v):
        a = list(args)
        a[i] = v
        return a

    cases = ([with_(good, i, None) for i in (0, 1)] + [with_(good, 6, g) for g in (0.0, -1.0, float("nan"), float("inf"))] +
             [with_(with_(good, 3, None), 6, 3.0)] + [with_(good, 12, 0), with_(good, 13, 0), with_(good, 8, None), with_(good, 9, None),
                                                      with_(with_(good, 2, None), 5, p)] +
             [with_(good, 15, s) for s in (float("nan"), float("inf"), -float("inf"))] +
             [with_(good, 16, c) for c in (-0.5, float("nan"), float("inf"))])
    for a in cases:
        assert L.k5_stochastic_euler(*a) == 1, a
        assert "k5_stochastic_euler" in E.last_error()
    with pytest.raises(ValueError, match="stochastic_euler_"):
        E.stochastic_euler_(torch.zeros(8), torch.zeros(8), None, 1.0, -0.1, 1.0, 0.5, 1, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        E.stochastic_euler_(torch.zeros(8), torch.zeros(8, dtype=torch.bfloat16), None, 1.0, -0.1, 1.0, 0.5, 1, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        E.noise_normal_(torch.zeros(8), 1)
