"""CPU-only checks of regional prompts: the identities of the float64 definition the GPU tests compare against, `region_masks_to_latent`
against a loop, that `generate` sets the regions for exactly one call (and not at all by default), the CLI flags, header / binding / library
agreement on the new entries, and every refusal of the library entries that needs no GPU."""
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

from regions_reference import combine_inputs, combine_reference, mask_cases, nabla_perm, token_weights_reference  # noqa: E402


prompt = functools.partial(kit.host_prompt, dims=(96, 48))


call_generate = functools.partial(kit.call_generate, w=1.0, steps=4, shape=SHAPE, pos=POS, conf=CONF, prompt=prompt)


def region_kw(R=2, bw=0.25):
    return dict(region_text_embeds=[prompt(5 + r, 10 + r) for r in range(R)], region_text_rope_pos=[torch.arange(5 + r) for r in range(R)],
                region_masks=torch.rand(R, *SHAPE[:3], generator=torch.Generator().manual_seed(3)), region_base_weight=bw)


# ------------------------------------------------------------------------------------------ the float64 definition
@pytest.mark.parametrize("R", [1, 2, 8])
def test_token_weights_identities(R):
    T, H, W = 3, 8, 12
    for bw in (0.0, 0.5, 1.0):
        w = token_weights_reference(mask_cases(R, T, H, W), bw, (1, 2, 2))
        assert w.shape == (T * (H // 2) * (W // 2), R + 1)
        assert torch.allclose(w.sum(1), torch.ones(w.shape[0], dtype=torch.float64), rtol=0, atol=1e-15) and (w >= 0).all()
        grid = w.reshape(T, H // 2, W // 2, R + 1)
        hole = grid[:, H // 8: H // 4]                                     # cells no mask reaches: the base prompt only
        assert (hole[..., 0] == 1).all() and (hole[..., 1:] == 0).all()
        alone = grid[:, H // 4: 3 * H // 8, : W // 4]                      # region 0 alone at 1: base_weight / (base_weight + 1) is left to the base
        assert torch.allclose(alone[..., 0], torch.full_like(alone[..., 0], bw / (bw + 1.0)), atol=1e-15)
        if R >= 2:                                                         # overlap, sum m = 0.9 R > 1: s = base_weight + sum m
            over = grid[:, : H // 8]
            assert torch.allclose(over[..., 1], torch.full_like(over[..., 1], 0.9 / (bw + 0.9 * R)), atol=1e-7)
    # masks that partition the frame at base_weight 0: one prompt per token, exactly
    col = torch.arange(W).expand(T, H, W)
    part = torch.stack([(col < 6).float(), (col >= 6).float()])
    w = token_weights_reference(part, 0.0, (1, 2, 2)).reshape(T, H // 2, W // 2, 3)
    assert (w[..., 0] == 0).all() and (w[:, :, :3, 1] == 1).all() and (w[:, :, 3:, 2] == 1).all() and ((w == 0) | (w == 1)).all()
    # all-zero masks: the base prompt only, whatever base_weight
    for bw in (0.0, 0.3, 1.0):
        w = token_weights_reference(torch.zeros(R, T, H, W), bw, (1, 2, 2))
        assert (w[:, 0] == 1).all() and (w[:, 1:] == 0).all()


def test_token_weights_in_the_nabla_order():
    perm = nabla_perm(2, 8, 8)
    assert sorted(perm.tolist()) == list(range(128)) and perm[:9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8] and perm[64] == 64
    perm = nabla_perm(1, 8, 16)
    assert perm[8] == 16 and perm[64] == 8                                 # a tile's rows are 16 apart; the second tile starts at column 8
    m = mask_cases(2, 1, 16, 32)
    w, wp = token_weights_reference(m, 0.5, (1, 2, 2)), token_weights_reference(m, 0.5, (1, 2, 2), perm)
    assert torch.equal(wp, w[perm.long()]) and not torch.equal(wp, w)


def test_combine_definition_identities():
    z0, zr, w = combine_inputs(13, 64, 3)
    out, mag = combine_reference(z0, zr, w)
    for i in range(13):
        if i % 3 == 1:                                                     # one-hot rows are that stream
            k = i % 4
            assert torch.equal(out[i], (z0[i] if k == 0 else zr[k - 1, i]).double())
    poisoned = zr.clone()
    for r in range(3):
        poisoned[r, w[:, r + 1] == 0] = float("nan")
    out2, _ = combine_reference(z0, poisoned, w)
    assert torch.equal(out2, out) and not torch.isnan(out2).any()          # a zero-weight stream does not reach the output
    assert (mag >= out.abs() - 1e-12).all()


# ------------------------------------------------------------------------------------------ conditioning
def test_region_masks_to_latent_against_a_loop():
    from kandinsky.conditioning import region_masks_to_latent
    g = torch.Generator().manual_seed(4)
    R, T, H, W = 2, 3, 16, 24
    m = torch.rand(R, 9, H, W, generator=g)
    out = region_masks_to_latent(m, T, H, W)
    assert out.shape == (R, T, H // 8, W // 8) and out.dtype == torch.float32
    for r in range(R):
        for t in range(T):
            frames = [0] if t == 0 else list(range(4 * t - 3, 4 * t + 1))
            for h in range(H // 8):
                for w in range(W // 8):
                    want = m[r, frames, 8 * h:8 * h + 8, 8 * w:8 * w + 8].double().mean().item()
                    assert abs(out[r, t, h, w].item() - want) <= 1e-6
    still = region_masks_to_latent(m[:, 0], T, H, W)                       # (R, H, W): all frames
    assert torch.equal(still[:, 0], out[:, 0]) and torch.equal(still[:, 1], still[:, 0]) and torch.equal(still[:, 2], still[:, 0])
    assert torch.equal(region_masks_to_latent(m[:, 0] >= 0.5, T, H, W), region_masks_to_latent((m[:, 0] >= 0.5).to(torch.uint8), T, H, W))
    assert region_masks_to_latent(m * 3.0 - 1.0, T, H, W).min() >= 0 and region_masks_to_latent(m * 3.0 - 1.0, T, H, W).max() <= 1
    assert torch.equal(region_masks_to_latent(m.numpy(), T, H, W), out)
    for bad, word in ((lambda: region_masks_to_latent(m, T, 20, W), "multiples of 8"), (lambda: region_masks_to_latent(m[:, :5], T, H, W), "pixel frames"),
                      (lambda: region_masks_to_latent(m[0, 0], T, H, W), "masks must be"), (lambda: region_masks_to_latent(m[..., :16], T, H, W), "masks must be")):
        with pytest.raises(ValueError, match=word):
            bad()


# ------------------------------------------------------------------------------------------ set_regions / generate
def test_set_regions_refusals(golden_meta):
    m = host_tiny(golden_meta)
    ok = region_kw()
    te, pos, masks = ok["region_text_embeds"], ok["region_text_rope_pos"], ok["region_masks"]
    for args in ((te, pos, masks, -0.1), (te, pos, masks, 1.5), (te, pos, masks, float("nan")), (te, pos, masks, "x"),
                 (te * 5, pos * 5, masks.repeat(5, 1, 1, 1), 0.0), ([], [], masks[:0], 0.0), (te, pos[:1], masks, 0.0), (te[0], pos[0], masks, 0.0),
                 ([None, te[1]], pos, masks, 0.0), ([{"text_embeds": torch.zeros(0, 96)}, te[1]], [[], pos[1]], masks, 0.0),
                 (te, [torch.arange(4), pos[1]], masks, 0.0), (te, [None, pos[1]], masks, 0.0), (te, pos, masks[:1], 0.0), (te, pos, masks[0], 0.0),
                 (te, pos, None, 0.0), ([{"text_embeds": torch.zeros(5, 80)}, te[1]], pos, masks, 0.0), (te, pos, masks[:, :, :7], 0.0)):
        with pytest.raises(ValueError, match="regions"):
            m.set_regions(*args)
    assert m._regions is None and m.regions_state() == (False, 0, 0)


def test_set_regions_is_remembered_until_the_engine_exists(golden_meta):
    m = host_tiny(golden_meta)
    kw = region_kw()
    assert m.set_regions(kw["region_text_embeds"], kw["region_text_rope_pos"], kw["region_masks"]) is m
    assert m._regions["base_weight"] == 0.0 and m._regions["text"][1] is kw["region_text_embeds"][1]["text_embeds"]   # the model keeps the tensors
    assert m._regions["masks"] is kw["region_masks"]
    assert m.clear_regions() is m and m._regions is None


def test_generate_by_default_passes_nothing_to_the_model(golden_meta):
    m = host_tiny(golden_meta)
    seen = []
    m.sample = lambda img, *a, **k: seen.append(m._regions)
    m.set_regions = m.clear_regions = lambda *a, **k: pytest.fail("without region_text_embeds the model must not be touched")
    call_generate(m)
    call_generate(m, region_masks=torch.zeros(2, 3, 8, 12), region_base_weight=0.5)   # without the prompts the rest is idle
    assert seen == [None, None]


def test_generate_sets_the_regions_for_the_call_and_clears_them_also_on_an_exception(golden_meta):
    m = host_tiny(golden_meta)
    seen = []

    def sample(img, *a, **k):
        seen.append(dict(m._regions))
        if len(seen) == 2:
            raise RuntimeError("boom")

    m.sample = sample
    kw = region_kw()
    call_generate(m, **kw)
    assert seen[0]["base_weight"] == 0.25 and seen[0]["text"][0] is kw["region_text_embeds"][0]["text_embeds"] and m._regions is None
    assert seen[0]["masks"] is kw["region_masks"]
    with pytest.raises(RuntimeError, match="boom"):
        call_generate(m, **kw)
    assert m._regions is None
    mine = region_kw(1, 1.0)                                               # regions that were on the model before the call are back after it
    m.set_regions(mine["region_text_embeds"], mine["region_text_rope_pos"], mine["region_masks"], 1.0)
    call_generate(m, **kw)
    assert len(seen[2]["text"]) == 2
    assert len(m._regions["text"]) == 1 and m._regions["base_weight"] == 1.0 and m._regions["masks"] is mine["region_masks"]
    # together with NAG: both are set for the call and both are gone afterwards
    both = []
    m.clear_regions()
    m.sample = lambda img, *a, **k: both.append((m._nag is not None, m._regions is not None))
    call_generate(m, nag_text_embeds=prompt(4), nag_text_rope_pos=torch.arange(4), nag_scale=5.0, **kw)
    assert both == [(True, True)] and m._nag is None and m._regions is None


def test_generate_refusals(golden_meta):
    m = host_tiny(golden_meta)
    m.sample = lambda *a, **k: pytest.fail("refused calls must not sample")
    kw = region_kw()
    for bad in (dict(region_base_weight=2.0), dict(region_masks=None), dict(region_text_rope_pos=None), dict(region_masks=kw["region_masks"][:1])):
        with pytest.raises(ValueError, match="regions"):
            call_generate(m, **{**kw, **bad})
    with pytest.raises(ValueError, match="window"):
        call_generate(m, context_frames=2, **kw)
    assert m._regions is None

    class Wrapped(torch.nn.Module):
        visual_cond = True

        def forward(self, *a, **k):
            pytest.fail("refused calls must not run the model")

    with pytest.raises(ValueError, match="engine"):
        call_generate(Wrapped(), **kw)
    from kandinsky.generation_utils import generate_sample
    with pytest.raises(ValueError, match="engine"):
        generate_sample((1, 3, 8, 12, 16), "a", NS(visual_cond=True), None, CONF, None, **kw)
    with pytest.raises(ValueError, match="regions"):
        generate_sample((1, 3, 8, 12, 16), "a", m, None, CONF, None, **{**kw, "region_masks": torch.zeros(2, 3, 8, 10)})


def test_generate_sample_encodes_region_prompts_with_the_caption(golden_meta, monkeypatch):
    from kandinsky import generation_utils as G
    m = host_tiny(golden_meta)
    seen, calls = {}, []

    class Embedder:
        def encode(self, prompts, type_of_content):
            calls.append(prompts[0])
            n = len(prompts[0])
            return {"text_embeds": torch.full((n, 96), float(n)), "pooled_embed": torch.zeros(1, 48)}, torch.tensor([0, n])

        def to(self, *a):
            return self

    monkeypatch.setattr(G, "generate", lambda *a, **k: seen.update(k) or torch.zeros(3, 8, 12, 16))
    monkeypatch.setattr(G, "latent_to_uint8", lambda latent, *a: latent)
    masks = torch.zeros(2, 3, 8, 12)
    G.generate_sample((1, 3, 8, 12, 16), "a cat", m, None, CONF, Embedder(), negative_caption="blurry", device="cpu",
                      region_text_embeds=["red car", "lighthouse"], region_masks=masks, region_base_weight=0.5)
    assert calls == ["a cat", "blurry", "red car", "lighthouse"]
    assert [tuple(e["text_embeds"].shape) for e in seen["region_text_embeds"]] == [(7, 96), (10, 96)]
    assert all("pooled_embed" not in e for e in seen["region_text_embeds"])   # only the token embeddings are used
    assert [p.tolist() for p in seen["region_text_rope_pos"]] == [list(range(7)), list(range(10))]
    assert seen["region_masks"] is masks and seen["region_base_weight"] == 0.5
    seen.clear()
    G.generate_sample((1, 3, 8, 12, 16), "a cat", m, None, CONF, Embedder(), negative_caption="blurry", device="cpu")
    assert not any(k.startswith("region") for k in seen)


# ------------------------------------------------------------------------------------------ pipeline and CLI
def test_pipeline_keywords(monkeypatch):
    from kandinsky import t2v_pipeline as P
    seen = {}

    def fake_generate_sample(shape, caption, *a, **k):
        seen.clear()
        seen.update(k, shape=shape)
        return torch.zeros(shape[0], 3, 4 * (shape[1] - 1) + 1, 8, 8, dtype=torch.uint8)

    monkeypatch.setattr(P, "generate_sample", fake_generate_sample)
    pipe = P.Kandinsky5T2VPipeline({"dit": "cpu", "vae": "cpu", "text_embedder": "cpu"}, None, None, None,
                                   conf=NS(model=NS(num_steps=4, guidance_weight=1.0)))
    pipe("a cat", time_length=1, expand_prompts=False, seed=1)
    assert not any(k.startswith("region") for k in seen)
    left = torch.zeros(512, 768)
    left[:, :384] = 1.0
    pipe("a street", time_length=1, expand_prompts=False, seed=1, regions=[("a red car", left), ("a lighthouse", 1.0 - left)], region_base_weight=0.25)
    assert seen["region_text_embeds"] == ["a red car", "a lighthouse"] and seen["region_base_weight"] == 0.25
    lat = seen["region_masks"]
    assert tuple(lat.shape) == (2, 7, 64, 96) and (lat[0, :, :, :48] == 1).all() and (lat[0, :, :, 48:] == 0).all() and torch.equal(lat[1], 1 - lat[0])
    pipe(["a street", "a beach"], time_length=1, expand_prompts=False, seed=1, regions=[("a red car", left)])   # a list of texts shares one region set
    assert seen["shape"][0] == 2 and tuple(seen["region_masks"].shape) == (1, 7, 64, 96)
    for kw, word in ((dict(regions=[("a", left)] * 9), "1 to 8"), (dict(regions=[]), "1 to 8"), (dict(regions=[(left, "a")]), "pairs"),
                     (dict(regions=[("a", left)], region_base_weight=1.5), "base_weight"), (dict(regions=[("a", left[:100])]), "masks must be"),
                     (dict(regions=[("a", left)], context_seconds=1), "context_seconds")):
        with pytest.raises(ValueError, match=word):
            pipe("a cat", time_length=2 if "context_seconds" in kw else 1, expand_prompts=False, seed=1, **kw)


def test_cli_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_cli_regions", os.path.join(PKG, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    none = p.parse_args([])
    assert not hasattr(none, "region") and not hasattr(none, "region_base_weight") and cli.region_keywords(none) == {}
    load = lambda path: "mask:" + path    # noqa: E731
    a = p.parse_args(["--region", "a red car", "left.png", "--region", "a lighthouse", "right.png"])
    assert cli.region_keywords(a, load) == {"regions": [("a red car", "mask:left.png"), ("a lighthouse", "mask:right.png")], "region_base_weight": 0.0}
    a = p.parse_args(["--region", "a red car", "left.png", "--region_base_weight", "0.5"])
    assert cli.region_keywords(a, load) == {"regions": [("a red car", "mask:left.png")], "region_base_weight": 0.5}
    with pytest.raises(ValueError, match="--region"):
        cli.region_keywords(p.parse_args(["--region_base_weight", "0.5"]), load)
    with pytest.raises(ValueError, match="region_base_weight"):
        cli.region_keywords(p.parse_args(["--region", "a", "m.png", "--region_base_weight", "1.5"]), load)
    with pytest.raises(ValueError, match="at most 8"):
        cli.region_keywords(p.parse_args(sum((["--region", "a", "m.png"] for _ in range(9)), [])), load)
    with pytest.raises(ValueError, match="context_seconds"):
        cli.region_keywords(p.parse_args(["--region", "a", "m.png", "--context_seconds", "5"]), load)
    with pytest.raises(SystemExit):
        p.parse_args(["--region", "only a prompt"])
    with pytest.raises(SystemExit):
        p.parse_args(["--region", "a", "m.png", "--region_base_weight", "much"])


# ------------------------------------------------------------------------------------------ ABI
NEW = ("k5_region_combine_bf16", "k5_region_weights_f32", "k5_dit_set_regions", "k5_dit_regions_state")


def test_header_binding_and_library_agree_on_the_new_entries(built_lib):
    assert_abi_entries(built_lib, NEW)


def test_entries_refuse_bad_arguments_without_a_gpu(built_lib, golden_meta):
    from kandinsky import _engine as E
    L = E.lib()
    m = host_tiny(golden_meta)
    h = m._create_handle()           # a handle is host memory until weights arrive
    try:
        pos = (C.c_int32 * 4)(0, 1, 2, 3)
        ok = (E.TextCond * 2)(E.TextCond(0x1000, 0x1000, 1, 4, pos), E.TextCond(0x1000, None, 1, 4, pos))   # pooled_embed is not read
        good = [h, ok, 2, 0x1000, 3, 8, 12, 0.5]

        def with_(i, v):
            a = list(good)
            a[i] = v
            return a

        def conds(second):
            return (E.TextCond * 2)(E.TextCond(0x1000, 0x1000, 1, 4, pos), second)

        for a, word in ((with_(0, None), "null handle"), (with_(2, 9), "R must be"), (with_(2, -1), "R must be"), (with_(7, -0.5), "base_weight"),
                        (with_(7, 1.5), "base_weight"), (with_(7, float("nan")), "base_weight"), (with_(3, None), "masks"), (with_(3, 0x1002), "aligned"),
                        (with_(5, 7), "divisible"), (with_(6, 11), "divisible"), (with_(4, 0), "divisible"),
                        (with_(1, conds(E.TextCond(0x1000, 0x1000, 1, 0, pos))), "text_len"), (with_(1, conds(E.TextCond(None, 0x1000, 1, 4, pos))), "text_embed"),
                        (with_(1, conds(E.TextCond(0x1000, 0x1000, 1, 4, None))), "text_rope_pos")):
            assert L.k5_dit_set_regions(*a) == 1, word
            assert word in E.last_error(), (word, E.last_error())
        on, R, n = C.c_int(7), C.c_int(7), C.c_longlong(7)
        assert L.k5_dit_regions_state(h, C.byref(on), C.byref(R), C.byref(n), 0) == 0 and (on.value, R.value, n.value) == (0, 0, 0)   # nothing stuck
        assert L.k5_dit_set_regions(*good) == 0
        assert L.k5_dit_regions_state(h, C.byref(on), C.byref(R), None, 0) == 0 and (on.value, R.value) == (1, 2)
        assert L.k5_dit_set_regions(*with_(7, 2.0)) == 1                    # a refused call leaves what was set
        assert L.k5_dit_regions_state(h, C.byref(on), C.byref(R), None, 0) == 0 and (on.value, R.value) == (1, 2)
        assert L.k5_dit_set_regions(*with_(2, 0)) == 0                      # R = 0 clears
        assert L.k5_dit_regions_state(h, C.byref(on), C.byref(R), None, 0) == 0 and (on.value, R.value) == (0, 0)
        assert L.k5_dit_set_regions(*good) == 0 and L.k5_dit_set_regions(h, None, 5, None, 0, 0, 0, 9.0) == 0   # NULL clears, whatever the rest
        assert L.k5_dit_regions_state(h, C.byref(on), None, None, 0) == 0 and on.value == 0
        assert L.k5_dit_regions_state(None, None, None, None, 0) == 1
    finally:
        L.k5_dit_destroy(h)
    # the kernel entries: refused before anything is launched
    p = 0x10000
    good = (p, p, 4 * 128, 3, p, 4, p, 4, 128, 128, None)

    def kw_(i, v):
        a = list(good)
        a[i] = v
        return a

    for a in (kw_(0, None), kw_(1, None), kw_(4, None), kw_(6, None), kw_(0, p + 8), kw_(1, p + 2), kw_(6, p + 4), kw_(4, p + 2), kw_(2, 4 * 128 + 4),
              kw_(3, 0), kw_(3, 9), kw_(5, 3), kw_(7, 0), kw_(8, 0), kw_(8, 132), kw_(9, 120), kw_(9, 132)):
        assert L.k5_region_combine_bf16(*a) == 1, a
        assert "k5_region_combine_bf16" in E.last_error()
    assert L.k5_region_combine_bf16(p, p, 4 * 2056, 3, p, 4, p, 4, 2056, 2056, None) == 6   # more than the register-resident row holds
    assert "2048" in E.last_error()
    goodw = (p, 2, 3, 8, 12, 1, 2, 2, 0.5, None, p, None)
    for i, v in ((0, None), (10, None), (0, p + 2), (10, p + 1), (9, p + 2), (1, 0), (1, 9), (2, 0), (3, 7), (4, 11), (5, 0), (5, 2), (8, -0.1), (8, 1.1),
                 (8, float("nan"))):
        a = list(goodw)
        a[i] = v
        assert L.k5_region_weights_f32(*a) == 1, (i, v)
        assert "k5_region_weights_f32" in E.last_error()
    with pytest.raises(ValueError, match="region_combine_"):
        E.region_combine_(torch.zeros(4, 128), torch.zeros(2, 4, 128, dtype=torch.bfloat16), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="region_weights"):
        E.region_weights(torch.zeros(2, 3, 8, 12, dtype=torch.float64), (1, 2, 2), 0.0)
