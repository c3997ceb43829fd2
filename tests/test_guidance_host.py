"""CPU-only checks of the sampler's guidance controls (per-step weights, guidance interval, CFG-Zero*, CFG rescale): `guidance_plan`, the
coefficient rule from five sums against the published tensor forms, the bf16 oracle loop against the reference's golden, every refusal that
needs no GPU (set_guidance, generate, the pipeline, the CLI, the library entries), that the defaults change nothing, and header / binding /
library agreement on the new entries."""
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

import guidance_reference as R  # noqa: E402
from kandinsky.generation_utils import edit_first_step, guidance_plan, sigma_schedule  # noqa: E402


prompt = functools.partial(kit.host_prompt, dims=(96, 48))


call_generate = functools.partial(kit.call_generate, w=5.0, steps=4, shape=SHAPE, pos=POS, conf=CONF, prompt=prompt)


# ------------------------------------------------------------------------------------------ guidance_plan
def test_plan_forms():
    sig = sigma_schedule(6, 5.0).tolist()
    assert guidance_plan(sig, 5.0) == [5.0] * 6
    assert guidance_plan(sig, 5.0, [5, 4, 3, 2, 1, 1.5]) == [5.0, 4.0, 3.0, 2.0, 1.0, 1.5]
    assert guidance_plan(sig, 5.0, lambda i, s: 1.0 + 4.0 * s) == [1.0 + 4.0 * s for s in sig[:-1]]
    seen = []
    guidance_plan(sig, 5.0, lambda i, s: seen.append((i, s)) or 2.0)
    assert seen == list(enumerate(sig[:-1]))                                  # the sigma a step starts from; the final 0 is no step
    for bad in ([5.0] * 5, [5.0] * 7, []):
        with pytest.raises(ValueError, match="6 steps"):
            guidance_plan(sig, 5.0, bad)
    with pytest.raises(ValueError, match="finite"):
        guidance_plan(sig, 5.0, [5.0] * 5 + [float("nan")])
    with pytest.raises(ValueError, match="sigmas"):
        guidance_plan([1.0], 5.0)


def test_plan_interval_edges():
    sig = [1.0, 0.75, 0.5, 0.25, 0.0]
    assert guidance_plan(sig, 5.0, None, (0.5, 0.75)) == [1.0, 5.0, 5.0, 1.0]        # both ends belong to the interval
    assert guidance_plan(sig, 5.0, None, (0.5000001, 0.7499999)) == [1.0] * 4
    assert guidance_plan(sig, 5.0, None, (0.0, 0.0)) == [1.0] * 4                    # sigma 0 is where the last step ENDS
    assert guidance_plan(sig, 5.0, None, (0.0, 1.0)) == [5.0] * 4
    assert guidance_plan(sig, 5.0, [2.0, 3.0, 4.0, 5.0], (0.25, 0.5)) == [1.0, 1.0, 4.0, 5.0]   # the interval cuts a schedule
    assert guidance_plan(sig, 5.0, lambda i, s: 2.0 + i, (0.75, 1.0)) == [2.0, 3.0, 1.0, 1.0]
    for bad in ((0.6, 0.4), (0.5,), 0.5, (0.1, 0.2, 0.3), ("a", "b")):
        with pytest.raises(ValueError, match="guidance_interval"):
            guidance_plan(sig, 5.0, None, bad)


def test_plan_is_cut_with_the_schedule_under_strength(golden_meta):
    """strength < 1 runs the tail of the schedule: the plan is the full run's, cut at the same step"""
    m = host_tiny(golden_meta)
    seen = []
    m.sample = lambda img, sigmas, *a, **k: seen.append((list(sigmas), m._guidance))
    sched = [5.0, 4.0, 3.0, 2.0, 1.5, 1.0, 2.5, 3.5]
    src = torch.zeros(SHAPE)
    call_generate(m, steps=8, guidance_schedule=sched, init_latent=src, strength=0.5)
    first = edit_first_step(8, 0.5)
    full = sigma_schedule(8, 5.0).tolist()
    assert first == 4 and seen[0][0] == full[first:]
    assert seen[0][1] == (sched[first:], False, 0, 0.0)
    call_generate(m, steps=8, guidance_interval=(full[6], full[5]), init_latent=src, strength=0.5)
    assert seen[1][1][0] == [1.0, 5.0, 5.0, 1.0]
    call_generate(m, steps=8, guidance_schedule=lambda i, s: float(i), init_latent=src, strength=0.25)
    assert seen[2][1][0] == [6.0, 7.0]                                        # the callable sees the full run's step numbers
    assert m._guidance is None


# ------------------------------------------------------------------------------------------ the rule: five sums against the tensor forms
def rule_inputs():
    g = torch.Generator().manual_seed(5)
    n = 4608
    base = torch.randn(n, generator=g)
    sets = {"randn": (base, 0.6 * base + 0.8 * torch.randn(n, generator=g)),
            "offset": (base + 2.0, 0.5 * base + torch.randn(n, generator=g) + 2.0),
            "integers": (torch.randint(-128, 129, (n,), generator=g) / 16.0, torch.randint(-128, 129, (n,), generator=g) / 16.0)}
    return {k: (c.to(torch.bfloat16).double(), u.to(torch.bfloat16).double()) for k, (c, u) in sets.items()}


@pytest.mark.parametrize("w", [1.5, 5.0])
@pytest.mark.parametrize("zero_star", [False, True])
@pytest.mark.parametrize("rescale", [0.0, 0.7, 1.0])
def test_rule_from_the_sums_is_the_published_rule(w, zero_star, rescale):
    for name, (c, u) in rule_inputs().items():
        sums = R.five_sums(c, u)
        alpha, beta = R.coeffs_from_sums(sums, c.numel(), w, zero_star, rescale)
        # float64 tensors through st_star / rescale_noise_cfg, with phi as the fp32 number the kernel is handed
        want = R.guided_velocity(c, u, w, zero_star, float(np.float32(rescale)))
        got = alpha * c + beta * u
        err = ((got - want).norm() / want.norm()).item()
        assert err <= 1e-10, (name, err)
        if zero_star and rescale == 0.0:
            assert abs(beta / (1.0 - w) - R.st_star(c, u).item()) <= 1e-10 * abs(R.st_star(c, u).item()), name
        if rescale == 1.0:                                                       # the guided velocity has the conditional one's std
            assert abs(got.std().item() / c.std().item() - 1.0) <= 1e-10, name


def test_rule_identities():
    c, u = rule_inputs()["randn"]
    n = c.numel()
    assert R.coeffs_from_sums(R.five_sums(c, u), n, 5.0, False, 0.0) == (5.0, -4.0)
    a, b = R.coeffs_from_sums(R.five_sums(c, c), n, 5.0, True, 0.0)            # u == c: the projection is 1
    assert a == 5.0 and abs(b + 4.0) <= 1e-10
    phi = float(np.float32(0.7))                                               # the fp32 number the kernel is handed
    a, b = R.coeffs_from_sums(R.five_sums(c, torch.zeros_like(c)), n, 5.0, True, 0.7)   # u == 0: finite, v = w c rescaled
    assert np.isfinite(a) and b == 0.0 and abs(a - (phi + (1.0 - phi) * 5.0)) <= 1e-12
    const = torch.full_like(c, 3.0)
    assert R.coeffs_from_sums(R.five_sums(const, const), n, 5.0, False, 0.7) == (5.0, -4.0)   # no variance: the rescale leaves v alone
    assert R.ulp_distance_f32(1.0, np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
    assert R.ulp_distance_f32(-1.0, 1.0) > 2 ** 30 and R.ulp_distance_f32(0.5, 0.5) == 0


# ------------------------------------------------------------------------------------------ the bf16 oracle loop against the golden
def test_oracle_loop_within_tolerance_of_the_reference_golden(golden, golden_meta, tiny_sd):
    from safetensors.torch import load_file
    from oracle import k5_oracle as O
    gold = load_file(os.path.join(GOLDEN, "dit_tiny_guidance.safetensors"))
    meta = json.load(open(os.path.join(GOLDEN, "dit_tiny_guidance_meta.json")))
    cfg = O.DitConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in golden_meta["tiny_config"].items()})
    noise = golden["gen.noise"]
    sig = O.sigma_schedule(meta["steps"], meta["scheduler_scale"])
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)

    def vel(text, pooled, tpos):
        return lambda x, s: O.dit_forward(tiny_sd, cfg, torch.cat([x, *zeros], -1), golden[text], golden[pooled], s.unsqueeze(0) * 1000, POS,
                                          tpos, (1.0, 2.0, 2.0), None, "bf16")
    assert set(meta["cases"]) == {"schedule", "interval", "zero_star_init", "rescale", "all"}
    for name, case in meta["cases"].items():
        assert case["weights"] == guidance_plan(sig.tolist(), meta["guidance_weight"], case.get("schedule"), case.get("interval")), name
        out = R.bf16_loop(vel("fwd.text", "fwd.pooled", torch.arange(7)), vel("gen.null_text", "gen.null_pooled", torch.arange(4)), noise, sig,
                          case["weights"], case.get("zero_star", False), case.get("zero_init", 0), case.get("rescale", 0.0))
        want = gold[f"guidance.{name}.final"]
        r = ((out - want).norm() / want.norm()).item()
        print(f"{name}: bf16 oracle vs golden {r:.3e} (recorded {meta['oracle_vs_golden'][name]:.3e})")
        assert r <= 2e-2, (name, r)
    kinds = [R.is_guided(w) for w in meta["cases"]["interval"]["weights"]]
    assert any(kinds) and not all(kinds)                                       # the interval case is a mixed plan


# ------------------------------------------------------------------------------------------ set_guidance / generate
BAD = [dict(weights=[]), dict(weights=[5.0, float("nan")]), dict(weights="abc"), dict(weights=[[1.0]]), dict(zero_init_steps=-1),
       dict(zero_init_steps=1.5), dict(zero_init_steps="x"), dict(rescale=-0.1), dict(rescale=1.1), dict(rescale=float("nan")), dict(rescale="x")]


@pytest.mark.parametrize("bad", BAD)
def test_set_guidance_refuses_bad_numbers(golden_meta, bad):
    m = host_tiny(golden_meta)
    with pytest.raises(ValueError, match="guidance"):
        m.set_guidance(**bad)
    assert m._guidance is None and m.guidance_state() == (False, 0, 0, 0)


def test_set_guidance_is_remembered_until_the_engine_exists(golden_meta):
    m = host_tiny(golden_meta)
    assert m.set_guidance([5, 4, 1], zero_star=1, zero_init_steps=1, rescale=0.5) is m
    assert m._guidance == ([5.0, 4.0, 1.0], True, 1, 0.5)
    assert m.set_guidance()._guidance == (None, False, 0, 0.0)
    assert m.clear_guidance() is m and m._guidance is None


def test_generate_with_the_defaults_passes_nothing_to_the_model(golden_meta):
    m = host_tiny(golden_meta)
    seen = []
    m.sample = lambda img, *a, **k: seen.append(m._guidance)
    m.set_guidance = m.clear_guidance = lambda *a, **k: pytest.fail("the defaults must not touch the model")
    call_generate(m)
    call_generate(m, guidance_schedule=None, guidance_interval=None, cfg_zero_star=False, cfg_zero_init=0, cfg_rescale=0.0)
    assert seen == [None, None]


def test_generate_sets_the_plan_for_the_call_and_clears_it_also_on_an_exception(golden_meta):
    m = host_tiny(golden_meta)
    seen = []

    def sample(img, *a, **k):
        seen.append(m._guidance)
        if len(seen) == 2:
            raise RuntimeError("boom")

    m.sample = sample
    kw = dict(guidance_schedule=[5, 4, 3, 1], cfg_zero_star=True, cfg_zero_init=1, cfg_rescale=0.7)
    call_generate(m, **kw)
    assert seen[0] == ([5.0, 4.0, 3.0, 1.0], True, 1, 0.7) and m._guidance is None
    with pytest.raises(RuntimeError, match="boom"):
        call_generate(m, **kw)
    assert m._guidance is None
    m.set_guidance(None, rescale=0.25)                                           # a plan that was on the model before the call is back after it
    call_generate(m, cfg_rescale=0.5)
    assert seen[2] == (None, False, 0, 0.5) and m._guidance == (None, False, 0, 0.25)
    call_generate(m, guidance_interval=(0.0, 0.9))
    assert seen[3][0] == guidance_plan(sigma_schedule(4, 5.0).tolist(), 5.0, None, (0.0, 0.9)) and seen[3][1:] == (False, 0, 0.0)


Wrapped = functools.partial(kit.Wrapped, refuse=True)


def test_generate_refusals(golden_meta):
    m = host_tiny(golden_meta)
    m.sample = lambda *a, **k: pytest.fail("refused calls must not sample")
    for model in (m, Wrapped(m)):
        for kw, word in ((dict(guidance_schedule=[5.0] * 3), "4 steps"), (dict(cfg_rescale=1.5), "rescale"), (dict(cfg_zero_init=-1), "zero_init"),
                         (dict(guidance_interval=(0.9, 0.1)), "guidance_interval"),
                         (dict(cfg_zero_star=True, guidance_interval=(2.0, 3.0)), "nothing to guide"),
                         (dict(cfg_rescale=0.5, guidance_schedule=[1.0] * 4), "nothing to guide"),
                         (dict(cfg_zero_init=1, init_latent=torch.zeros(SHAPE)), "init_latent"),
                         (dict(cfg_rescale=0.5, context_frames=2), "context windows"),
                         (dict(guidance_schedule=[5.0] * 4, context_frames=2, context_overlap=1), "context windows")):
            with pytest.raises(ValueError, match=word):
                call_generate(model, **kw)
        with pytest.raises(ValueError, match="nothing to guide"):
            call_generate(model, w=1.0, cfg_zero_star=True)
    assert m._guidance is None
    # a plan with guided and unguided steps, or with zero-init: not with MagCache, not on a CFG pair
    mixed = (dict(guidance_interval=(0.0, 0.9)), dict(cfg_zero_init=1), dict(guidance_schedule=[5.0, 1.0, 5.0, 5.0]))
    m.mag_ratios = [1.0] * 8
    for kw in mixed:
        with pytest.raises(ValueError, match="MagCache"):
            call_generate(m, **kw)
    m.mag_ratios = None
    m._cfg_pair = 0
    for kw in mixed:
        with pytest.raises(ValueError, match="CFG pair"):
            call_generate(m, **kw)
    m._cfg_pair = None


def test_generate_sample_and_pipeline_keywords(golden_meta, monkeypatch):
    from kandinsky import generation_utils as G
    from kandinsky import t2v_pipeline as P
    m = host_tiny(golden_meta)
    for kw in (dict(cfg_rescale=2.0), dict(cfg_zero_init=-2), dict(guidance_schedule=[1.0, float("inf")]), dict(guidance_interval=(1.0, 0.0))):
        with pytest.raises(ValueError, match="guidance"):
            G.generate_sample((1, 3, 8, 12, 16), "a", m, None, CONF, None, **kw)
    seen = {}

    class Embedder:
        def encode(self, prompts, type_of_content):
            return {"text_embeds": torch.zeros(4, 96), "pooled_embed": torch.zeros(1, 48)}, torch.tensor([0, 4])

        def to(self, *a):
            return self

    monkeypatch.setattr(G, "generate", lambda *a, **k: seen.update(k) or torch.zeros(3, 8, 12, 16))
    monkeypatch.setattr(G, "latent_to_uint8", lambda latent, *a: latent)
    names = ("guidance_schedule", "guidance_interval", "cfg_zero_star", "cfg_zero_init", "cfg_rescale")
    G.generate_sample((1, 3, 8, 12, 16), "a cat", m, None, CONF, Embedder(), device="cpu")
    assert not any(k in seen for k in names)
    fn = lambda i, s: 3.0    # noqa: E731
    G.generate_sample((1, 3, 8, 12, 16), "a cat", m, None, CONF, Embedder(), device="cpu", guidance_schedule=fn, guidance_interval=(0.2, 0.8),
                      cfg_zero_star=True, cfg_zero_init=2, cfg_rescale=0.7)
    assert seen["guidance_schedule"] is fn and {k: seen[k] for k in names[1:]} == dict(guidance_interval=(0.2, 0.8), cfg_zero_star=True,
                                                                                     cfg_zero_init=2, cfg_rescale=0.7)

    def fake_generate_sample(shape, caption, *a, **k):
        seen.clear()
        seen.update(k)
        return torch.zeros(shape[0], 3, 4 * (shape[1] - 1) + 1, 8, 8, dtype=torch.uint8)

    monkeypatch.setattr(P, "generate_sample", fake_generate_sample)
    pipe = P.Kandinsky5T2VPipeline({"dit": "cpu", "vae": "cpu", "text_embedder": "cpu"}, None, None, None,
                                   conf=NS(model=NS(num_steps=4, guidance_weight=5.0)))
    pipe("a cat", time_length=1, expand_prompts=False, seed=1)
    assert not any(k in seen for k in names)
    pipe("a cat", time_length=1, expand_prompts=False, seed=1, guidance_schedule=[5, 4, 3, 2], cfg_rescale=0.5)
    assert seen["guidance_schedule"] == [5, 4, 3, 2] and seen["cfg_rescale"] == 0.5 and "cfg_zero_star" not in seen
    pipe("a cat", time_length=1, expand_prompts=False, seed=1, guidance_interval=(0.3, 0.9), cfg_zero_star=True, cfg_zero_init=1)
    assert (seen["guidance_interval"], seen["cfg_zero_star"], seen["cfg_zero_init"]) == ((0.3, 0.9), True, 1)
    for kw in (dict(cfg_rescale=-1), dict(cfg_zero_init=-1), dict(guidance_schedule=["x"])):
        with pytest.raises(ValueError, match="guidance"):
            pipe("a cat", time_length=1, expand_prompts=False, seed=1, **kw)
    with pytest.raises(ValueError, match="context_seconds"):
        pipe("a cat", time_length=2, expand_prompts=False, seed=1, cfg_zero_star=True, context_seconds=1)


def test_cli_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_cli_guidance", os.path.join(PKG, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    names = ("guidance_schedule", "guidance_interval", "cfg_zero_star", "cfg_zero_init", "cfg_rescale")
    none = p.parse_args([])
    assert not any(hasattr(none, n) for n in names) and cli.guidance_keywords(none) == {}
    a = p.parse_args(["--guidance_schedule", "5", "4", "3", "--guidance_interval", "0.2", "0.9", "--cfg_zero_star", "--cfg_zero_init", "1",
                      "--cfg_rescale", "0.7", "--sample_steps", "3"])
    assert cli.guidance_keywords(a) == dict(guidance_schedule=[5.0, 4.0, 3.0], guidance_interval=(0.2, 0.9), cfg_zero_star=True, cfg_zero_init=1,
                                            cfg_rescale=0.7)
    assert cli.guidance_keywords(p.parse_args(["--cfg_rescale", "0.5"])) == {"cfg_rescale": 0.5}
    for argv, word in ((["--guidance_schedule", "5", "4", "--sample_steps", "3"], "sample_steps"), (["--guidance_interval", "0.9", "0.2"], "LO <= HI"),
                       (["--cfg_zero_init", "-1"], "cfg_zero_init"), (["--cfg_rescale", "1.5"], "cfg_rescale"),
                       (["--cfg_zero_star", "--context_seconds", "5"], "context_seconds")):
        with pytest.raises(ValueError, match=word):
            cli.guidance_keywords(p.parse_args(argv))
    for argv in (["--guidance_interval", "0.5"], ["--cfg_rescale", "high"], ["--guidance_schedule"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)


# ------------------------------------------------------------------------------------------ ABI
NEW = ("k5_guidance_stats_blocks", "k5_guidance_coeffs_bf16", "k5_guided_euler", "k5_dit_set_guidance", "k5_dit_guidance_state")


def test_header_binding_and_library_agree_on_the_new_entries(built_lib):
    from kandinsky import _engine as E
    assert_abi_entries(built_lib, NEW, [("k5_guidance", E.Guidance)])


def test_entries_refuse_bad_arguments_without_a_gpu(built_lib, golden_meta):
    from kandinsky import _engine as E
    L = E.lib()
    h = host_tiny(golden_meta)._create_handle()           # a handle is host memory until weights arrive
    try:
        w = (C.c_float * 3)(5.0, 4.0, 1.0)
        wp = C.cast(w, C.POINTER(C.c_float))
        assert L.k5_dit_set_guidance(None, C.byref(E.Guidance(wp, 3, 0, 0, 0.0))) == 1 and "null handle" in E.last_error()
        w[1] = float("inf")
        for g, word in ((E.Guidance(wp, 0, 0, 0, 0.0), "num_weights"), (E.Guidance(wp, 3, 0, 0, 0.0), "finite"), (E.Guidance(None, 0, 0, -1, 0.0), "zero_init"),
                        (E.Guidance(None, 0, 0, 0, 1.5), "rescale"), (E.Guidance(None, 0, 0, 0, -0.5), "rescale"),
                        (E.Guidance(None, 0, 0, 0, float("nan")), "rescale")):
            assert L.k5_dit_set_guidance(h, C.byref(g)) == 1
            assert word in E.last_error()
        on, a, b, z = C.c_int(7), C.c_longlong(7), C.c_longlong(7), C.c_longlong(7)
        assert L.k5_dit_guidance_state(h, C.byref(on), C.byref(a), C.byref(b), C.byref(z), 0) == 0
        assert (on.value, a.value, b.value, z.value) == (0, 0, 0, 0)                        # nothing of the refused calls stuck
        w[1] = 4.0
        assert L.k5_dit_set_guidance(h, C.byref(E.Guidance(wp, 3, 1, 1, 0.7))) == 0
        assert L.k5_dit_guidance_state(h, C.byref(on), None, None, None, 0) == 0 and on.value == 1
        assert L.k5_dit_set_guidance(h, None) == 0                                            # NULL clears
        assert L.k5_dit_guidance_state(h, C.byref(on), None, None, None, 1) == 0 and on.value == 0
        assert L.k5_dit_guidance_state(None, None, None, None, None, 0) == 1
    finally:
        L.k5_dit_destroy(h)
    # the kernel entries: refused before anything is launched
    p = 0x10000
    good = [p, p, 4608, 5.0, 1, 0.7, p, p, p, None]

    def with_(args, i, v):
        a = list(args)
        a[i] = v
        return a

    for a in ([with_(good, i, None) for i in (0, 1, 6, 7, 8)] + [with_(good, i, p + 8) for i in (0, 1, 6, 7, 8)] +
              [with_(good, 2, 0), with_(good, 2, -8), with_(good, 5, -0.1), with_(good, 5, 1.1), with_(good, 5, float("nan"))]):
        assert L.k5_guidance_coeffs_bf16(*a) == 1, a
        assert "k5_guidance_coeffs_bf16" in E.last_error()
    for n in (4, 4607, 4612):
        assert L.k5_guidance_coeffs_bf16(*with_(good, 2, n)) == 2 and "multiple of 8" in E.last_error()
    assert [L.k5_guidance_stats_blocks(n) for n in (8, 2048, 2056, 4608, 11200)] == [1, 1, 2, 3, 6]
    cap = L.k5_guidance_stats_blocks(1 << 40)
    assert L.k5_guidance_stats_blocks(8 * 256 * cap) == cap == L.k5_guidance_stats_blocks(8 * 256 * cap + 4608)
    euler = [p, p, p, p, -0.1, p, p, p, 0.5, 288, 16, None, None]
    for a in ([with_(euler, i, None) for i in (0, 1, 2, 3)] + [with_(euler, 9, 0), with_(euler, 10, 0), with_(euler, 5, None), with_(euler, 6, None)]):
        assert L.k5_guided_euler(*a) == 1, a
        assert "k5_guided_euler" in E.last_error()
    with pytest.raises(ValueError, match="guidance_coeffs"):
        E.guidance_coeffs(torch.zeros(8, dtype=torch.bfloat16), torch.zeros(8), 5.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        E.guidance_coeffs(torch.zeros(8, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.bfloat16), 5.0)
