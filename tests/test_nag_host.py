"""CPU-only checks of normalized attention guidance (NAG): every refusal that needs no GPU (set_nag, generate, generate_sample, the pipeline,
the CLI, the library entries), that `nag_scale=None` changes nothing, that `generate` removes the guidance it set also when the run raises,
header / binding / library agreement on the new entries, and the identities of the float64 definition the GPU tests compare against."""
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

from nag_reference import nag_inputs, nag_reference  # noqa: E402


prompt = functools.partial(kit.host_prompt, dims=(96, 48))


call_generate = functools.partial(kit.call_generate, w=1.0, steps=4, shape=SHAPE, pos=POS, conf=CONF, prompt=prompt)


# ------------------------------------------------------------------------------------------ the float64 definition
def test_float64_definition_identities():
    zp, zn = nag_inputs(9, 128)
    for s, tau, alpha in ((5.0, 2.5, 0.25), (11.0, 1.0, 1.0), (1.5, 4.0, 0.5)):
        assert torch.equal(nag_reference(zp, zp, s, tau, alpha)[0], zp.double())            # z- == z+
        assert not nag_reference(zp, zp, s, tau, alpha)[2].any()
    assert torch.equal(nag_reference(zp, zn, 1.0, 2.5, 0.25)[0], zp.double())               # s == 1
    assert torch.equal(nag_reference(zp, zn, 5.0, 2.5, 0.0)[0], zp.double())                # alpha == 0
    out, fg, clamped = nag_reference(zp, zn, 5.0, 2.5, 0.25)
    assert torch.isfinite(out).all() and (out[3] == 0).all() and clamped[3]                 # a zero row gives zero, no NaN
    assert torch.equal(out[4], zp[4].double())
    assert clamped.tolist() == [r % 2 == 1 for r in range(9)]
    # the clamp holds the row's L1 norm at tau times the positive one
    assert torch.allclose(fg[clamped].abs().sum(-1), 2.5 * zp.double()[clamped].abs().sum(-1), rtol=1e-12, atol=0)


def test_float64_definition_is_the_published_rule():
    zp, zn = nag_inputs(8, 64)
    s, tau, alpha = 5.0, 2.5, 0.25
    z, p = s * zp.double() - (s - 1.0) * zn.double(), zp.double()
    ratio = z.abs().sum(-1, keepdim=True) / p.abs().sum(-1, keepdim=True)
    zhat = z * torch.minimum(ratio, torch.full_like(ratio, tau)) / ratio
    want = alpha * zhat + (1 - alpha) * p
    live = torch.tensor([r != 3 for r in range(8)])                                         # the published form divides by the zero row's norm
    assert torch.allclose(nag_reference(zp, zn, s, tau, alpha)[0][live], want[live], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------ set_nag / generate
BAD = [dict(scale=0.5), dict(tau=0.9), dict(alpha=-0.1), dict(alpha=1.5), dict(scale=float("nan")), dict(tau=float("inf")), dict(scale="x")]


@pytest.mark.parametrize("bad", BAD)
def test_set_nag_refuses_bad_numbers(golden_meta, bad):
    m = host_tiny(golden_meta)
    with pytest.raises(ValueError, match="nag"):
        m.set_nag(prompt(4), torch.arange(4), **bad)
    assert m._nag is None


def test_set_nag_refuses_bad_prompts(golden_meta):
    m = host_tiny(golden_meta)
    for te, pos in ((None, torch.arange(4)), ({"pooled_embed": torch.zeros(1, 48)}, torch.arange(4)), (prompt(4), torch.arange(3)),
                    (prompt(4), None), ({"text_embeds": torch.zeros(0, 96)}, []), ({"text_embeds": torch.zeros(4, 80)}, torch.arange(4)),
                    ({"text_embeds": torch.zeros(96)}, [0])):
        with pytest.raises(ValueError, match="nag"):
            m.set_nag(te, pos)
    assert m._nag is None and m.nag_state() == (False, 0)


def test_set_nag_is_remembered_until_the_engine_exists(golden_meta):
    m = host_tiny(golden_meta)
    ne = prompt(4)
    assert m.set_nag(ne, torch.arange(4)) is m
    assert m._nag["args"] == (5.0, 2.5, 0.25) and m._nag["text"] is ne["text_embeds"]       # the model keeps the tensors alive
    assert m.set_nag(ne, torch.arange(4), scale=1.0, alpha=0.0)._nag["args"] == (1.0, 2.5, 0.0)   # accepted: means off
    assert m.clear_nag() is m and m._nag is None


def test_generate_without_nag_scale_passes_nothing_to_the_model(golden_meta):
    m = host_tiny(golden_meta)
    seen = []
    m.sample = lambda img, *a, **k: seen.append(m._nag)
    m.set_nag = m.clear_nag = lambda *a, **k: pytest.fail("nag_scale=None must not touch the model")
    call_generate(m)
    call_generate(m, nag_text_embeds=prompt(4), nag_text_rope_pos=torch.arange(4), nag_tau=3.0)   # without nag_scale the rest is idle
    assert seen == [None, None]


def test_generate_sets_nag_for_the_call_and_clears_it_also_on_an_exception(golden_meta):
    m = host_tiny(golden_meta)
    ne = prompt(4, 3)
    seen = []

    def sample(img, *a, **k):
        seen.append(dict(m._nag))
        if len(seen) == 2:
            raise RuntimeError("boom")

    m.sample = sample
    kw = dict(nag_text_embeds=ne, nag_text_rope_pos=torch.arange(4), nag_scale=4.0, nag_tau=2.0, nag_alpha=0.5)
    call_generate(m, **kw)
    assert seen[0]["args"] == (4.0, 2.0, 0.5) and seen[0]["text"] is ne["text_embeds"] and m._nag is None
    with pytest.raises(RuntimeError, match="boom"):
        call_generate(m, **kw)
    assert m._nag is None
    # guidance that was on the model before the call is back after it
    mine = prompt(5, 4)
    m.set_nag(mine, torch.arange(5), 3.0, 1.5, 1.0)
    call_generate(m, **kw)
    assert seen[2]["args"] == (4.0, 2.0, 0.5)
    assert m._nag["args"] == (3.0, 1.5, 1.0) and m._nag["text"] is mine["text_embeds"]


def test_generate_refusals(golden_meta):
    m = host_tiny(golden_meta)
    m.sample = lambda *a, **k: pytest.fail("refused calls must not sample")
    ne = prompt(4)
    for kw in (dict(nag_scale=0.5), dict(nag_scale=5.0, nag_tau=0.5), dict(nag_scale=5.0, nag_alpha=2.0)):
        with pytest.raises(ValueError, match="nag"):
            call_generate(m, nag_text_embeds=ne, nag_text_rope_pos=torch.arange(4), **kw)
    with pytest.raises(ValueError, match="nag"):
        call_generate(m, nag_scale=5.0)                                                     # no negative prompt
    with pytest.raises(ValueError, match="nag"):
        call_generate(m, nag_scale=5.0, nag_text_embeds=ne, nag_text_rope_pos=torch.arange(3))
    assert m._nag is None


Wrapped = functools.partial(kit.Wrapped, refuse=True)


def test_a_model_without_the_engine_raises(golden_meta):
    kw = dict(nag_text_embeds=prompt(4), nag_text_rope_pos=torch.arange(4), nag_scale=5.0)
    with pytest.raises(ValueError, match="engine"):
        call_generate(Wrapped(host_tiny(golden_meta)), **kw)
    with pytest.raises(ValueError, match="engine"):
        call_generate(NS(visual_cond=True), **kw)
    from kandinsky.generation_utils import generate_sample
    with pytest.raises(ValueError, match="engine"):
        generate_sample((1, 3, 8, 12, 16), "a", NS(visual_cond=True), None, CONF, None, nag_scale=5.0)


def test_generate_sample_refusals_and_the_negative_caption(golden_meta, monkeypatch):
    from kandinsky import generation_utils as G
    m = host_tiny(golden_meta)
    for kw in (dict(nag_scale=0.0), dict(nag_scale=5.0, nag_tau=0.0), dict(nag_scale=5.0, nag_alpha=-1.0)):
        with pytest.raises(ValueError, match="nag"):
            G.generate_sample((1, 3, 8, 12, 16), "a", m, None, CONF, None, **kw)
    seen = {}

    class Embedder:
        def encode(self, prompts, type_of_content):
            n = 7 if prompts[0] == "a cat" else 4
            return {"text_embeds": torch.full((n, 96), float(n)), "pooled_embed": torch.zeros(1, 48)}, torch.tensor([0, n])

        def to(self, *a):
            return self

    monkeypatch.setattr(G, "generate", lambda *a, **k: seen.update(k) or torch.zeros(3, 8, 12, 16))
    monkeypatch.setattr(G, "latent_to_uint8", lambda latent, *a: latent)
    G.generate_sample((1, 3, 8, 12, 16), "a cat", m, None, CONF, Embedder(), negative_caption="blurry", device="cpu", guidance_weight=1.0,
                      nag_scale=6.0, nag_tau=2.0)
    assert seen["nag_scale"] == 6.0 and seen["nag_tau"] == 2.0 and seen["nag_alpha"] == 0.25
    assert tuple(seen["nag_text_embeds"]["text_embeds"].shape) == (4, 96) and seen["nag_text_rope_pos"].tolist() == [0, 1, 2, 3]
    seen.clear()
    G.generate_sample((1, 3, 8, 12, 16), "a cat", m, None, CONF, Embedder(), negative_caption="blurry", device="cpu")
    assert not any(k.startswith("nag") for k in seen)


# ------------------------------------------------------------------------------------------ pipeline and CLI
def test_pipeline_keywords(monkeypatch):
    from kandinsky import t2v_pipeline as P
    seen = {}

    def fake_generate_sample(shape, caption, *a, **k):
        seen.clear()
        seen.update(k)
        return torch.zeros(shape[0], 3, 4 * (shape[1] - 1) + 1, 8, 8, dtype=torch.uint8)

    monkeypatch.setattr(P, "generate_sample", fake_generate_sample)
    pipe = P.Kandinsky5T2VPipeline({"dit": "cpu", "vae": "cpu", "text_embedder": "cpu"}, None, None, None,
                                   conf=NS(model=NS(num_steps=4, guidance_weight=1.0)))
    pipe("a cat", time_length=1, expand_prompts=False, seed=1)
    assert not any(k.startswith("nag") for k in seen)
    pipe("a cat", time_length=1, expand_prompts=False, seed=1, nag_scale=5)
    assert (seen["nag_scale"], seen["nag_tau"], seen["nag_alpha"]) == (5.0, 2.5, 0.25)
    pipe("a cat", time_length=1, expand_prompts=False, seed=1, nag_scale=3, nag_tau=1.5, nag_alpha=1)
    assert (seen["nag_scale"], seen["nag_tau"], seen["nag_alpha"]) == (3.0, 1.5, 1.0)
    for kw in (dict(nag_scale=0.9), dict(nag_scale=5, nag_tau=0.5), dict(nag_scale=5, nag_alpha=1.01)):
        with pytest.raises(ValueError, match="nag"):
            pipe("a cat", time_length=1, expand_prompts=False, seed=1, **kw)


def test_cli_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_cli_nag", os.path.join(PKG, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    none = p.parse_args([])
    assert not any(hasattr(none, n) for n in ("nag_scale", "nag_tau", "nag_alpha")) and cli.nag_keywords(none) == {}
    assert cli.nag_keywords(p.parse_args(["--nag_scale", "5"])) == {"nag_scale": 5.0, "nag_tau": 2.5, "nag_alpha": 0.25}
    assert cli.nag_keywords(p.parse_args(["--nag_scale", "3", "--nag_tau", "2", "--nag_alpha", "0.5"])) == {
        "nag_scale": 3.0, "nag_tau": 2.0, "nag_alpha": 0.5}
    for argv in (["--nag_tau", "2"], ["--nag_alpha", "0.5"]):
        with pytest.raises(ValueError, match="--nag_scale"):
            cli.nag_keywords(p.parse_args(argv))
    for argv in (["--nag_scale", "0.5"], ["--nag_scale", "5", "--nag_tau", "0.5"], ["--nag_scale", "5", "--nag_alpha", "1.5"]):
        with pytest.raises(ValueError, match="nag"):
            cli.nag_keywords(p.parse_args(argv))
    with pytest.raises(SystemExit):
        p.parse_args(["--nag_scale", "high"])


# ------------------------------------------------------------------------------------------ ABI
NEW = ("k5_nag_combine_bf16", "k5_dit_set_nag", "k5_dit_nag_state")


def test_header_binding_and_library_agree_on_the_new_entries(built_lib):
    assert_abi_entries(built_lib, NEW)


def test_entries_refuse_bad_arguments_without_a_gpu(built_lib, golden_meta):
    from kandinsky import _engine as E
    L = E.lib()
    m = host_tiny(golden_meta)
    h = m._create_handle()           # a handle is host memory until weights arrive
    try:
        pos = (C.c_int32 * 4)(0, 1, 2, 3)
        ok = E.TextCond(0x1000, 0x1000, E.K5_BF16 if hasattr(E, "K5_BF16") else 1, 4, pos)
        assert L.k5_dit_set_nag(None, C.byref(ok), 5.0, 2.5, 0.25) == 1 and "null handle" in E.last_error()
        for args, word in (((0.5, 2.5, 0.25), "scale"), ((5.0, 0.5, 0.25), "tau"), ((5.0, 2.5, -0.1), "alpha"), ((5.0, 2.5, 1.1), "alpha"),
                           ((float("nan"), 2.5, 0.25), "scale")):
            assert L.k5_dit_set_nag(h, C.byref(ok), *args) == 1, args
            assert word in E.last_error()
        for cond, word in ((E.TextCond(0x1000, 0x1000, 1, 0, pos), "text_len"), (E.TextCond(None, 0x1000, 1, 4, pos), "text_embed"),
                           (E.TextCond(0x1000, 0x1000, 1, 4, None), "text_rope_pos")):
            assert L.k5_dit_set_nag(h, C.byref(cond), 5.0, 2.5, 0.25) == 1
            assert word in E.last_error()
        on, n = C.c_int(7), C.c_longlong(7)
        assert L.k5_dit_nag_state(h, C.byref(on), C.byref(n), 0) == 0 and (on.value, n.value) == (0, 0)   # nothing of the refused calls stuck
        assert L.k5_dit_set_nag(h, C.byref(ok), 5.0, 2.5, 0.25) == 0
        assert L.k5_dit_nag_state(h, C.byref(on), None, 0) == 0 and on.value == 1
        for args in ((1.0, 2.5, 0.25), (5.0, 2.5, 0.0)):                                    # accepted, and off
            assert L.k5_dit_set_nag(h, C.byref(ok), *args) == 0
            assert L.k5_dit_nag_state(h, C.byref(on), None, 0) == 0 and on.value == 0
        assert L.k5_dit_set_nag(h, C.byref(ok), 5.0, 2.5, 0.25) == 0 and L.k5_dit_set_nag(h, None, 0.0, 0.0, 0.0) == 0   # NULL clears, whatever the numbers
        assert L.k5_dit_nag_state(h, C.byref(on), None, 0) == 0 and on.value == 0
        assert L.k5_dit_nag_state(None, None, None, 0) == 1
    finally:
        L.k5_dit_destroy(h)
    # the kernel entry: refused before anything is launched
    p = 0x10000
    good = (p, p, p, 4, 128, 128, 5.0, 2.5, 0.25, None)

    def with_(i, v):
        a = list(good)
        a[i] = v
        return a

    for a in (with_(0, None), with_(1, None), with_(2, None), with_(0, p + 8), with_(2, p + 2), with_(3, 0), with_(4, 0), with_(4, 132),
              with_(5, 120), with_(5, 132), with_(6, 0.5), with_(7, 0.99), with_(8, -0.5), with_(8, 1.5), with_(6, float("nan"))):
        assert L.k5_nag_combine_bf16(*a) == 1, a
        assert "k5_nag_combine_bf16" in E.last_error()
    assert L.k5_nag_combine_bf16(p, p, p, 4, 2056, 2056, 5.0, 2.5, 0.25, None) == 6            # more than the register-resident row holds
    assert "2048" in E.last_error()
    with pytest.raises(ValueError, match="nag_combine_"):
        E.nag_combine_(torch.zeros(4, 128), torch.zeros(4, 128, dtype=torch.bfloat16), 5.0, 2.5, 0.25)
