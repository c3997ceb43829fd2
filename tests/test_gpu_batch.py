"""Several samples per call on the MI355X: k5_sample_many / k5_dit_forward_many and `generate(batch=B)` / `generate_sample(bs=B)` above them.

The invariant of the whole feature, asserted bit for bit everywhere: every sample of a many-sample call equals the same sample (same noise,
prompt, negative prompt, conditioning) run alone through k5_sample / k5_sample_cond on the same handle with the same options."""
import ctypes as C
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
from kit import make_dit, need_gpu, tiny_config  # noqa: E402

NABLA = {"P": 0.8, "wT": 3, "wH": 3, "wW": 3}


@pytest.fixture(scope="module")
def tiny_cfg(golden_meta):
    return tiny_config(golden_meta)


@pytest.fixture(scope="module")
def tiny_dit(tiny_cfg, tiny_sd):
    need_gpu()
    return make_dit(tiny_cfg, tiny_sd)


def wide_dit(qk_gain=1.0, seed=4):
    """production width (model_dim 1792, 28 heads), two visual blocks, weights drawn on the device"""
    need_gpu()
    from kandinsky.models.dit import DiffusionTransformer3D
    d = DiffusionTransformer3D(**dict(O.LITE_2B, num_visual_blocks=2, num_text_blocks=1))
    return d.init_synthetic("cuda:0", seed=seed, std=0.03, qk_gain=qk_gain)


def prompts(dit, B, seed):
    """B prompts of different token lengths and B negative prompts (also of different lengths)"""
    g = torch.Generator().manual_seed(seed)
    tes, nes = [], []
    for b in range(B):
        for out, n in ((tes, 5 + 7 * b), (nes, 3 + 2 * b)):
            out.append({"text_embeds": torch.randn(n, dit._cfg["in_text_dim"], generator=g).cuda(),
                        "pooled_embed": torch.randn(1, dit._cfg["in_text_dim2"], generator=g).cuda()})
    return tes, nes


def run_pair(dit, shape, B, w, sparse=None, vcond=None, steps=3, seed=0):
    """(batched latents, alone latents), both (B, T, H, W, C)"""
    from kandinsky.generation_utils import sigma_schedule
    T, H, W = shape
    tes, nes = prompts(dit, B, seed)
    tps = [torch.arange(t["text_embeds"].shape[0]) for t in tes]
    nps = [torch.arange(t["text_embeds"].shape[0]) for t in nes]
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    noise = torch.randn(B, T, H, W, dit.in_visual_dim, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    sig = sigma_schedule(steps, 5.0).tolist()
    batched = noise.clone()
    dit.sample_many(batched, sig, tes, nes, pos, tps, nps, w, scale_factor=(1.0, 2.0, 2.0), sparse_params=sparse, visual_cond=vcond)
    alone = noise.clone()
    for b in range(B):
        lat = alone[b].contiguous()
        dit.sample(lat, sig, tes[b], nes[b], pos, tps[b], nps[b], w, scale_factor=(1.0, 2.0, 2.0), sparse_params=sparse,
                   visual_cond=None if vcond is None else vcond[b].contiguous())
        alone[b] = lat
    torch.cuda.synchronize()
    return batched, alone


def assert_same(batched, alone):
    assert torch.isfinite(batched).all()
    for b in range(batched.shape[0]):
        assert torch.equal(batched[b], alone[b]), f"sample {b}: max |diff| {(batched[b] - alone[b]).abs().max().item()}"
    if batched.shape[0] > 1:
        assert not torch.equal(batched[0], batched[1])        # the samples really differ (own noise, own prompt)


# ------------------------------------------------------------------------------------------ k5_sample_many, tiny checkpoint
@pytest.mark.parametrize("attn", ["dense", "nabla"])
@pytest.mark.parametrize("w", [1.0, 5.0])
@pytest.mark.parametrize("B", [1, 2, 3, 8])
def test_sample_many_tiny_bit_identical(tiny_dit, B, w, attn):
    batched, alone = run_pair(tiny_dit, (2, 16, 32), B, w, NABLA if attn == "nabla" else None, seed=B)
    assert_same(batched, alone)


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_sample_many_visual_cond_one_conditioned_one_not(tiny_dit, w):
    """sample 0 carries a conditioning latent on frame 0 (mask 1), sample 1 none (zeros); each equals k5_sample_cond alone, and the
    unconditioned one also equals plain k5_sample (no conditioning tensor at all)"""
    from kandinsky.generation_utils import sigma_schedule
    T, H, W = 3, 16, 16
    g = torch.Generator().manual_seed(7)
    vc = torch.zeros(2, T, H, W, 17)
    vc[0, 0, :, :, :16] = torch.randn(H, W, 16, generator=g)
    vc[0, 0, :, :, 16] = 1.0
    vc = vc.cuda()
    batched, alone = run_pair(tiny_dit, (T, H, W), 2, w, vcond=vc, seed=11)
    assert_same(batched, alone)
    tes, nes = prompts(tiny_dit, 2, 11)
    plain = torch.randn(2, T, H, W, 16, generator=torch.Generator().manual_seed(12)).cuda()[1].contiguous()
    tiny_dit.sample(plain, sigma_schedule(3, 5.0).tolist(), tes[1], nes[1], [torch.arange(T), torch.arange(8), torch.arange(8)],
                    torch.arange(12), torch.arange(5), w, scale_factor=(1.0, 2.0, 2.0))
    assert torch.equal(plain, batched[1])


# ------------------------------------------------------------------------------------------ k5_sample_many, production width
@pytest.fixture(scope="module")
def wide_dits():
    """production-width handles by QK-norm gain (1: the plain fixed-offset softmax; 5: the anchored route)"""
    d = {qk: wide_dit(qk_gain=qk) for qk in (1.0, 5.0)}
    yield d
    for m in d.values():
        m._destroy_engine()


WIDE = [((13, 32, 32), B, w, attn, qk, fp8) for B in (1, 2, 3, 8) for w in (1.0, 5.0) for attn in ("dense", "nabla")
        for qk in (1.0, 5.0) for fp8 in (0, 7)]                     # config 1's token grid 13 x 16 x 16
WIDE += [((1, 64, 96), B, w, "dense", qk, fp8) for B in (1, 2, 3, 8) for w in (1.0, 5.0) for qk in (1.0, 5.0)
         for fp8 in (0, 7)]                                          # one 512 x 768 frame (1536 tokens)


@pytest.mark.parametrize("shape,B,w,attn,qk,fp8", WIDE)
def test_sample_many_production_width_bit_identical(wide_dits, shape, B, w, attn, qk, fp8):
    dit = wide_dits[qk]
    dit.set_fp8(fp8)
    try:
        batched, alone = run_pair(dit, shape, B, w, NABLA if attn == "nabla" else None, steps=2, seed=3 * B + int(w))
    finally:
        dit.set_fp8(0)
    assert_same(batched, alone)


# ------------------------------------------------------------------------------------------ k5_dit_forward_many
def _forward_many_case(dit, attn, shape, S=4, seed=21):
    T, H, W = shape
    tes, _ = prompts(dit, S, seed)
    tps = [torch.arange(t["text_embeds"].shape[0]) for t in tes]
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    x = torch.randn(S, T, H, W, dit.visual_embed_dim, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    sp = NABLA if attn == "nabla" else None

    def one(i):
        return dit(x[i], tes[i]["text_embeds"], tes[i]["pooled_embed"], torch.tensor([731.0]), pos, tps[i], scale_factor=(1.0, 2.0, 2.0),
                   sparse_params=sp)

    def prime():   # a softmax-form memory that is not empty: what one forward of sequence 0 leaves behind
        dit.reset_softmax_memory()
        one(0)

    alone = []
    for i in range(S):
        prime()
        alone.append(one(i))
    prime()
    out = dit.forward_many(x, tes, 731.0, pos, tps, scale_factor=(1.0, 2.0, 2.0), sparse_params=sp)
    after = one(1)                       # the call left the memory as it found it: as after prime()
    torch.cuda.synchronize()
    for i in range(S):
        assert torch.equal(out[i], alone[i]), i
    assert torch.equal(after, alone[1])
    assert not torch.equal(out[0], out[1])


@pytest.mark.parametrize("attn", ["dense", "nabla"])
def test_forward_many_each_sequence_equals_forward_tiny(tiny_dit, attn):
    _forward_many_case(tiny_dit, attn, (2, 16, 32))


@pytest.mark.parametrize("qk", [1.0, 5.0])
def test_forward_many_each_sequence_equals_forward_production_width(wide_dits, qk):
    _forward_many_case(wide_dits[qk], "dense", (13, 32, 32))


# ------------------------------------------------------------------------------------------ refusals
def _c_args(dit, B, lat, keep, vcond=None):
    from kandinsky import _engine as E
    tes, nes = prompts(dit, max(B, 1), 5)
    s = E.SampleManyArgs()
    s.B = B
    s.fwd = dit._forward_args((2, 16, 32), None, 16, tes[0]["text_embeds"], tes[0]["pooled_embed"], 0.0,
                              [torch.arange(2), torch.arange(8), torch.arange(16)], torch.arange(5), (1.0, 2.0, 2.0), None, keep)
    conds = (E.TextCond * max(B, 1))(*[dit._text_cond(t["text_embeds"], t["pooled_embed"], torch.arange(t["text_embeds"].shape[0]), keep)
                                       for t in tes])
    keep.append(conds)
    s.conds, s.null_conds = conds, None
    sig = (C.c_float * 3)(1.0, 0.5, 0.0)
    keep.append(sig)
    s.latents, s.visual_cond, s.num_steps, s.sigmas, s.guidance_weight = lat, vcond, 2, sig, 1.0
    return s


def test_refusals(tiny_dit, tiny_cfg, tiny_sd):
    from kandinsky import _engine as E
    from kandinsky.magcache_utils import disable_magcache, set_magcache_params
    from kandinsky.models.dit import DiffusionTransformer3D
    L = E.lib()
    lat = torch.randn(2, 2, 16, 32, 16).cuda()
    before = lat.clone()
    h = tiny_dit.engine(lat.device)
    keep = []

    def status(dit, B=2, ptr=None, vcond=None):
        s = _c_args(dit, B, lat.data_ptr() if ptr is None else ptr, keep, vcond)
        return L.k5_sample_many(dit.engine(lat.device), C.byref(s), E.stream_ptr()), E.last_error()

    assert status(tiny_dit, B=0) == (1, "k5_sample_many: B must be >= 1 (got 0)")
    st, msg = status(tiny_dit, ptr=lat.data_ptr() + 2)
    assert st == 1 and "aligned" in msg
    st, msg = status(tiny_dit, vcond=lat.data_ptr() + 2)
    assert st == 1 and "aligned" in msg
    a = E.ForwardArgs()
    a.x = lat.data_ptr()
    assert L.k5_dit_forward_many(h, C.byref(a), 0, None, None, None) == 1 and "S must be >= 1" in E.last_error()
    # visual conditioning on a handle without it
    nc = DiffusionTransformer3D(**dict(tiny_cfg, visual_cond=False))
    sd = dict(tiny_sd)
    sd["visual_embeddings.in_layer.weight"] = sd["visual_embeddings.in_layer.weight"][:, :64].contiguous()
    nc.load_state_dict(sd, assign=True)
    nc = nc.to("cuda:0")
    vc = torch.zeros(2, 2, 16, 32, 17, device="cuda")
    st, msg = status(nc, vcond=vc.data_ptr())
    assert st == 1 and "visual_cond = 0" in msg
    with pytest.raises(ValueError, match="visual_cond"):
        nc.sample_many(lat, [1.0, 0.0], prompts(nc, 2, 1)[0], None, [torch.arange(2), torch.arange(8), torch.arange(16)],
                        [torch.arange(5), torch.arange(12)], None, 1.0, visual_cond=vc)
    # graph capture, MagCache
    tiny_dit.set_graph(True)
    try:
        st, msg = status(tiny_dit)
        assert st == 4 and "graph capture" in msg
    finally:
        tiny_dit.set_graph(False)
    set_magcache_params(tiny_dit, [1.0] * 8, 2, False)
    try:
        st, msg = status(tiny_dit)
        assert st == 4 and "MagCache" in msg
        assert L.k5_dit_forward_many(h, C.byref(a), 1, None, None, None) == 4 and "MagCache" in E.last_error()
    finally:
        disable_magcache(tiny_dit)
    # a sequence-parallel group and a CFG pair (loopback transport: the handle's state is what is refused)
    for kind in ("sp", "pair"):
        d = DiffusionTransformer3D(**tiny_cfg)
        d.load_state_dict(tiny_sd, assign=True)
        d = d.to("cuda:0")
        d.engine("cuda:0")
        group = E.LoopbackGroup(2)
        if kind == "sp":
            d.enable_loopback(group, 0)
        else:
            d.enable_cfg_pair_loopback(group, 0)
        st, msg = status(d)
        assert st == 4 and ("sequence-parallel" if kind == "sp" else "CFG pair") in msg
        keep.append((d, group))
    torch.cuda.synchronize()
    assert torch.equal(lat, before)          # nothing ran


# ------------------------------------------------------------------------------------------ generate / generate_sample
def test_generate_batch_routes_to_one_engine_call(tiny_dit, monkeypatch):
    """generate(batch=3) on a single-rank engine DiT: one sample_many call, each sample = generate(noise=slice) alone"""
    from kandinsky.generation_utils import generate
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    B, T = 3, 2
    tes, nes = prompts(tiny_dit, B, 31)
    tps = [torch.arange(t["text_embeds"].shape[0]) for t in tes]
    pos = [torch.arange(T), torch.arange(8), torch.arange(8)]
    noise = torch.randn(B * T, 16, 16, 16, generator=torch.Generator().manual_seed(32))
    calls = []
    orig = type(tiny_dit).sample_many
    monkeypatch.setattr(type(tiny_dit), "sample_many", lambda self, *a, **k: calls.append(1) or orig(self, *a, **k))
    out = generate(tiny_dit, "cuda:0", (B * T, 16, 16, 16), 3, tes, nes[0], pos, tps, torch.arange(3), 5.0, 5.0, conf, noise=noise,
                   batch=B)
    assert calls == [1]
    for b in range(B):
        one = generate(tiny_dit, "cuda:0", (T, 16, 16, 16), 3, tes[b], nes[0], pos, tps[b], torch.arange(3), 5.0, 5.0, conf,
                       noise=noise[b * T:(b + 1) * T])
        assert torch.equal(out[b * T:(b + 1) * T], one), b


def test_generate_sample_bs3_equals_three_single_samples():
    """the pipeline's generate_sample with bs = 3 and three captions (tiny DiT + tiny VAE, stub text encoder): uint8 frames bit-identical
    to three single-sample runs of the same pipeline stages on the same noise slices"""
    need_gpu()
    from test_pipeline import StubTextEmbedder, make_conf
    from kandinsky import generation_utils as G
    from kandinsky.models.dit import get_dit
    from kandinsky.models.vae import AutoencoderKLHunyuanVideo
    dev = "cuda:0"
    conf = make_conf()
    dit = get_dit(conf.model.dit_params)
    g = torch.Generator().manual_seed(0)
    sd = {k: (torch.ones_like(v) if k.endswith("norm.weight") else torch.randn(v.shape, generator=g) * 0.05)
          for k, v in dit.state_dict().items()}
    dit.load_state_dict(sd, assign=True)
    dit = dit.to(dev)
    vae = AutoencoderKLHunyuanVideo(block_out_channels=(64, 64, 128, 128), norm_num_groups=16)
    vsd = {}
    for k, p in vae.state_dict().items():
        if "norm" in k and k.endswith("weight"):
            vsd[k] = torch.ones(p.shape)
        elif k.endswith("bias"):
            vsd[k] = torch.zeros(p.shape)
        else:
            vsd[k] = torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5)
    vae.load_state_dict(vsd, assign=True)
    vae = vae.eval().to(dev)
    te = StubTextEmbedder()
    caps = ["a cat", "a red fox in the snow", "two dogs"]
    shape = (3, 2, 16, 16, 16)
    out = G.generate_sample(shape, caps, dit, vae, conf, te, num_steps=3, guidance_weight=4.0, scheduler_scale=5.0,
                            negative_caption="ugly", seed=9, device=dev, vae_device=dev, progress=False)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 3, 5, 128, 128)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    noise = torch.randn(6, 16, 16, 16, device=dev, generator=gen)      # the one draw generate makes for the whole batch
    (neg, n_neg), = G._encode_prompts(te, ["ugly"], "video", dev)
    grid = [torch.arange(2), torch.arange(8), torch.arange(8)]
    for b, cap in enumerate(caps):
        (cond, n), = G._encode_prompts(te, [cap], "video", dev)
        lat = G.generate(dit, dev, (2, 16, 16, 16), 3, cond, neg, grid, torch.arange(n), torch.arange(n_neg), 4.0, 5.0, conf,
                         noise=noise[2 * b:2 * b + 2])
        one = G.latent_to_uint8(lat, vae, 1, dev)
        assert torch.equal(out[b:b + 1], one), b
    assert not torch.equal(out[0], out[1])
