"""CPU-only checks of several samples per call: `generate(batch=B)` splits one noise draw and the prompts per sample and equals B calls of
its own on a duck-typed model, the argument errors fire before any work, the pipeline hands a prompt list through as one batch,
and libk5.so exports (and refuses, without a GPU) the two many-sample entry points."""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import pytest
import torch

import euler_step_reference as ER  # noqa: E402
import kit  # noqa: E402
from kit import built_lib, flash_conf  # noqa: E402

CONF = flash_conf()


class FakeDit:
    """duck-typed model: a velocity that depends on the latent, the prompt and the time; every call is logged"""
    visual_cond = False

    def __init__(self):
        self.calls = []

    def __call__(self, x, text_embed, pooled, t, visual_rope_pos, text_rope_pos, scale_factor=None, sparse_params=None):
        self.calls.append((x.clone(), text_embed, len(text_rope_pos)))
        return (0.5 * x + text_embed.mean() + pooled.mean() * float(t.reshape(-1)[0]) / 1000).to(torch.bfloat16)


prompt = functools.partial(kit.host_prompt, dims=(8, 4))


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_generate_batch_splits_noise_and_prompts(monkeypatch, w):
    from kandinsky import generation_utils as G
    monkeypatch.setattr(G.E, "euler_step_", ER.euler_step_)
    B, T = 3, 2
    noise = torch.randn(B * T, 4, 6, 16, generator=torch.Generator().manual_seed(5))
    tes = [prompt(3 + b, b) for b in range(B)]
    ne = prompt(2, 99)
    pos = [torch.arange(T), torch.arange(2), torch.arange(3)]
    tps = [torch.arange(3 + b) for b in range(B)]
    model = FakeDit()
    out = G.generate(model, "cpu", (B * T, 4, 6, 16), 3, tes, ne, pos, tps, torch.arange(2), w, 5.0, CONF, noise=noise, batch=B)
    steps, per = 3, 2 if w != 1.0 else 1
    assert len(model.calls) == B * steps * per
    for b in range(B):
        first = model.calls[b * steps * per]
        assert torch.equal(first[0], noise[b * T:(b + 1) * T])          # its own noise slice
        assert first[1] is tes[b]["text_embeds"] and first[2] == 3 + b  # its own prompt and positions
        if per == 2:
            assert model.calls[b * steps * per + 1][1] is ne["text_embeds"]
        alone = G.generate(FakeDit(), "cpu", (T, 4, 6, 16), 3, tes[b], ne, pos, tps[b], torch.arange(2), w, 5.0, CONF,
                           noise=noise[b * T:(b + 1) * T])
        assert torch.equal(out[b * T:(b + 1) * T], alone)
    # one shared prompt = the same prompt for every sample
    model = FakeDit()
    G.generate(model, "cpu", (B * T, 4, 6, 16), 2, tes[0], ne, pos, tps[0], torch.arange(2), w, 5.0, CONF, noise=noise, batch=B)
    assert all(c[1] is tes[0]["text_embeds"] or c[1] is ne["text_embeds"] for c in model.calls)


def test_generate_batch_one_is_the_plain_call(monkeypatch):
    from kandinsky import generation_utils as G
    monkeypatch.setattr(G.E, "euler_step_", ER.euler_step_)
    noise = torch.randn(2, 4, 6, 16, generator=torch.Generator().manual_seed(1))
    te, ne = prompt(4, 1), prompt(2, 2)
    pos = [torch.arange(2), torch.arange(2), torch.arange(3)]
    a = G.generate(FakeDit(), "cpu", (2, 4, 6, 16), 2, te, ne, pos, torch.arange(4), torch.arange(2), 5.0, 5.0, CONF, noise=noise)
    b = G.generate(FakeDit(), "cpu", (2, 4, 6, 16), 2, [te], [ne], pos, [torch.arange(4)], [torch.arange(2)], 5.0, 5.0, CONF,
                   noise=noise, batch=1)
    assert torch.equal(a, b)


def test_batch_argument_errors():
    from kandinsky import generation_utils as G
    te, ne = prompt(4, 1), prompt(2, 2)
    pos = [torch.arange(2), torch.arange(2), torch.arange(3)]
    with pytest.raises(ValueError, match="batch=2"):
        G.generate(FakeDit(), "cpu", (3, 4, 6, 16), 2, te, ne, pos, torch.arange(4), torch.arange(2), 5.0, 5.0, CONF,
                   noise=torch.zeros(3, 4, 6, 16), batch=2)
    with pytest.raises(ValueError, match="2 entries for batch=3"):
        G.generate(FakeDit(), "cpu", (6, 4, 6, 16), 2, [te, te], ne, pos, torch.arange(4), torch.arange(2), 5.0, 5.0, CONF,
                   noise=torch.zeros(6, 4, 6, 16), batch=3)
    with pytest.raises(ValueError, match="2 captions for bs=3"):
        G.generate_sample((3, 1, 4, 6, 16), ["a", "b"], None, None, CONF, None)


def test_pipeline_passes_a_prompt_list_as_one_batch(monkeypatch):
    from kandinsky import t2v_pipeline as P
    seen = {}

    def fake_generate_sample(shape, caption, *a, **k):
        seen["shape"], seen["caption"], seen["seed"] = shape, caption, k["seed"]
        return torch.zeros(shape[0], 3, 4 * (shape[1] - 1) + 1, 8 * shape[2], 8 * shape[3], dtype=torch.uint8)

    monkeypatch.setattr(P, "generate_sample", fake_generate_sample)
    conf = NS(model=NS(num_steps=2, guidance_weight=5.0))
    pipe = P.Kandinsky5T2VPipeline({"dit": "cpu", "vae": "cpu", "text_embedder": "cpu"}, None, None, None, conf=conf)
    out = pipe(["a cat", "a dog", "a fox"], time_length=1, width=512, height=512, seed=3, expand_prompts=False)
    assert seen["shape"] == (3, 7, 64, 64, 16) and seen["caption"] == ["a cat", "a dog", "a fox"] and seen["seed"] == 3
    assert out.shape[0] == 3
    pics = pipe(["a cat", "a dog"], time_length=0, width=512, height=512, seed=3, expand_prompts=False)
    assert isinstance(pics, list) and len(pics) == 2 and seen["shape"][0] == 2
    pipe("a cat", time_length=1, width=512, height=512, seed=3, expand_prompts=False)
    assert seen["shape"][0] == 1 and seen["caption"] == "a cat"
    with pytest.raises(ValueError, match="at least one prompt"):
        pipe([], time_length=1, width=512, height=512, seed=3, expand_prompts=False)


def test_batch_entry_points_exported_and_refuse_without_gpu(built_lib):
    lib = C.CDLL(built_lib)
    assert hasattr(lib, "k5_sample_many") and hasattr(lib, "k5_dit_forward_many")
    from kandinsky import _engine as E
    L = E.lib()
    s = E.SampleManyArgs()
    s.B = 1
    assert L.k5_sample_many(None, C.byref(s), None) == 1 and "null handle" in E.last_error()
    cc = E.DitConfig(16, 96, 48, 64, 16, (C.c_int * 3)(1, 2, 2), 128, 256, 1, 2, (C.c_int * 3)(16, 24, 24), 1)
    h = C.c_void_p()
    assert L.k5_dit_create(C.byref(cc), C.byref(h)) == 0
    try:
        assert L.k5_sample_many(h, C.byref(s), None) == 4 and "finalize" in E.last_error()
        a = E.ForwardArgs()
        assert L.k5_dit_forward_many(h, C.byref(a), 1, None, None, None) == 4 and "finalize" in E.last_error()
    finally:
        L.k5_dit_destroy(h)
