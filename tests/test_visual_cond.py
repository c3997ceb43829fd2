"""Visual conditioning (image-to-video), CPU side: the C entry point k5_sample_cond is exported and declared, the oracle's
conditioned loop is pinned to the reference's own conditioned trajectories (tools/gen_golden_visual_cond.py), and the image
helper's resize / crop / normalise rule holds on small synthetic pictures."""
import ctypes
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import k5_oracle as O
from kit import GOLDEN, ROOT, built_lib, rel, tiny_config  # noqa: E402


@pytest.fixture(scope="module")
def vc_golden(golden):
    """tests/golden/dit_tiny_visual_cond.safetensors expanded: the full conditioning tensors (the stored latent on frame 0, mask 1
    there, zeros elsewhere), the inputs in fp32 and the w = 5 trajectory ending at its final latent."""
    from safetensors.torch import load_file
    g = dict(load_file(os.path.join(GOLDEN, "dit_tiny_visual_cond.safetensors")))
    for pre, shape in (("cond", golden["gen.noise"].shape), ("nabla", golden["gen.nabla.noise"].shape)):
        vc, mask = torch.zeros(shape), torch.zeros(*shape[:-1], 1)
        vc[0], mask[0] = g[pre + ".visual_cond0"].float(), 1.0
        g[pre + ".visual_cond"], g[pre + ".mask"] = vc, mask
    g["enc.x"], g["enc.tiled.x"] = g["enc.x"].float(), g["enc.tiled.x"].float()
    tag = "cond.4_5.0_5.0"
    g[tag + ".latents"] = torch.cat([g[tag + ".latents"], g[tag + ".final"][None]])
    return g


@pytest.fixture(scope="module")
def vc_meta():
    with open(os.path.join(GOLDEN, "dit_tiny_visual_cond_meta.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cfg(golden_meta):
    return O.DitConfig(**tiny_config(golden_meta))


def conditioned_oracle(sd, cfg, noise, steps, w, s, te, ne, pos, vc, mask, mode, attention=None):
    """O.generate's loop with the conditioning channels filled (the reference loop body, zeros replaced)."""
    img = noise.clone().float()
    sparse = O.get_sparse_params(attention or {"type": "flash"}, img.shape, cfg.patch_size)
    sig = O.sigma_schedule(steps, s)
    traj = []
    for i in range(steps):
        x = torch.cat([img, vc, mask], dim=-1)
        v = O.get_velocity(sd, cfg, x, sig[i].unsqueeze(0), te, ne, pos, torch.arange(7), torch.arange(4), w, (1.0, 2.0, 2.0),
                           sparse, mode)
        img = img + O._r((sig[i + 1] - sig[i]) * v, mode)
        traj.append(img.clone())
    return img, torch.stack(traj)


# ------------------------------------------------------------------------------------------ C ABI
def test_sample_cond_exported_declared_and_refuses_null_handle(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "k5.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+k5_sample_cond\s*\(\s*k5_dit\s*\*", src)
    assert re.search(r"\bint\s+k5_patchify_cond_bf16\s*\(", src)
    lib = ctypes.CDLL(built_lib)
    for name in ("k5_sample_cond", "k5_patchify_cond_bf16"):
        assert hasattr(lib, name), name
    from kandinsky import _engine as E
    assert "k5_sample_cond" in E.SYMBOLS and "k5_patchify_cond_bf16" in E.SYMBOLS
    s = E.SampleArgs()
    assert E.lib().k5_sample_cond(None, ctypes.byref(s), None, None) == 1          # K5_ERR_ARG
    assert E.lib().k5_sample_cond(None, ctypes.byref(s), ctypes.c_void_p(64), None) == 1


def test_sample_and_generate_refuse_conditioning_without_visual_cond_channels():
    from types import SimpleNamespace as NS
    from kandinsky.generation_utils import generate

    class NoCond(torch.nn.Module):
        visual_cond = False

    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    with pytest.raises(ValueError, match="visual_cond"):
        generate(NoCond(), "cpu", (1, 4, 4, 16), 1, {}, {}, None, None, None, 1.0, 5.0, conf, noise=torch.zeros(1, 4, 4, 16),
                 visual_cond_mask=torch.ones(1, 4, 4, 1))


# ------------------------------------------------------------------------------------------ oracle vs the reference's conditioned loop
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_oracle_conditioned_loop_vs_reference_golden(golden, tiny_sd, cfg, vc_golden, w):
    te = {"text_embeds": golden["fwd.text"], "pooled_embed": golden["fwd.pooled"]}
    ne = {"text_embeds": golden["gen.null_text"], "pooled_embed": golden["gen.null_pooled"]}
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    vc, mask = vc_golden["cond.visual_cond"], vc_golden["cond.mask"]
    assert vc[1:].abs().sum() == 0 and vc[0].abs().sum() > 0 and mask[0].eq(1).all() and mask[1:].eq(0).all()
    tag = f"cond.4_5.0_{w}"
    final, traj = conditioned_oracle(tiny_sd, cfg, golden["gen.noise"], 4, w, 5.0, te, ne, pos, vc, mask, "fp32")
    if tag + ".latents" in vc_golden:
        torch.testing.assert_close(traj, vc_golden[tag + ".latents"], atol=2e-4, rtol=2e-4)
    torch.testing.assert_close(final, vc_golden[tag + ".final"], atol=2e-4, rtol=2e-4)
    final16, _ = conditioned_oracle(tiny_sd, cfg, golden["gen.noise"], 4, w, 5.0, te, ne, pos, vc, mask, "bf16")
    assert rel(final16, vc_golden[tag + ".final"]) <= 3e-2
    # the conditioning really moves the trajectory: the unconditioned golden is elsewhere
    assert rel(vc_golden[tag + ".final"], golden[f"gen.4_5.0_{w}.final"]) > 1e-3


def test_oracle_conditioned_nabla_vs_reference_golden(golden, tiny_sd, cfg, vc_golden, vc_meta):
    c = vc_meta["nabla_case"]
    te = {"text_embeds": golden["fwd.text"], "pooled_embed": golden["fwd.pooled"]}
    ne = {"text_embeds": golden["gen.null_text"], "pooled_embed": golden["gen.null_pooled"]}
    pos = [torch.arange(6), torch.arange(16), torch.arange(16)]
    final, _ = conditioned_oracle(tiny_sd, cfg, golden["gen.nabla.noise"], c["steps"], c["guidance_weight"], c["scheduler_scale"], te,
                                  ne, pos, vc_golden["nabla.visual_cond"], vc_golden["nabla.mask"], "fp32", c["attention"])
    torch.testing.assert_close(final[:, ::4, ::4], vc_golden["nabla.final.sample"], atol=2e-4, rtol=2e-4)
    assert abs(final.double().pow(2).sum().item() - c["final_sumsq"]) <= 1e-5 * c["final_sumsq"]


def test_oracle_one_frame_encode_vs_reference_golden(vc_golden, vc_meta):
    """1 frame -> 1 latent frame through the reference's encoder, untiled and through its spatial tiling (tiny encoder weights of
    vae_enc_tiny.safetensors)."""
    from safetensors.torch import load_file
    from oracle import vae_oracle as V
    enc = load_file(os.path.join(GOLDEN, "vae_enc_tiny.safetensors"))
    cfg = json.load(open(os.path.join(GOLDEN, "vae_enc_meta.json")))["config"]
    cfg = dict(cfg, block_out_channels=tuple(cfg["block_out_channels"]))
    sd = {k[2:]: v for k, v in enc.items() if k.startswith("w.")}
    got = V.encoder_forward(sd, vc_golden["enc.x"], cfg, "fp32")
    assert tuple(got.shape) == (1, 32, 1, 4, 6)
    torch.testing.assert_close(got, vc_golden["enc.moments"], atol=1e-4, rtol=1e-4)
    c = vc_meta["enc_tiled_case"]
    tiled = V.tiled_encode(sd, vc_golden["enc.tiled.x"], cfg, tuple(c["tile"]), tuple(c["stride"]), "fp32")
    assert tuple(tiled.shape) == (1, 32, 1, 10, 10)
    torch.testing.assert_close(tiled, vc_golden["enc.tiled.moments"], atol=1e-4, rtol=1e-4)


# ------------------------------------------------------------------------------------------ image helper
def _rule(x, height, width):
    """The documented rule, restated: cover (height, width) at the input's aspect ratio, bicubic + antialias, centre crop."""
    h, w = x.shape[1:]
    s = max(height / h, width / w)
    nh, nw = max(height, round(h * s)), max(width, round(w * s))
    y = F.interpolate(x[None], size=(nh, nw), mode="bicubic", antialias=True, align_corners=False)[0] if (nh, nw) != (h, w) else x
    top, left = (nh - height) // 2, (nw - width) // 2
    return y[:, top:top + height, left:left + width].clamp(-1, 1)


@pytest.mark.parametrize("src,dst", [((24, 60), (16, 24)),     # wider than the target: width cropped
                                     ((60, 20), (16, 24)),     # taller: height cropped
                                     ((32, 48), (16, 24)),     # same aspect: no crop
                                     ((16, 24), (16, 24)),     # same size: untouched
                                     ((9, 13), (16, 24))])     # upscaled
def test_preprocess_resize_crop_normalise(src, dst):
    from kandinsky.conditioning import preprocess_image
    g = torch.Generator().manual_seed(src[0] * 100 + src[1])
    u8 = torch.randint(0, 256, (src[0], src[1], 3), generator=g, dtype=torch.uint8)          # HWC
    out = preprocess_image(u8, *dst)
    assert out.shape == (3,) + dst and out.dtype == torch.float32
    assert out.min() >= -1 and out.max() <= 1
    f = u8.permute(2, 0, 1).float() / 127.5 - 1.0
    torch.testing.assert_close(out, _rule(f, *dst), atol=0, rtol=0)
    assert torch.equal(preprocess_image(u8.permute(2, 0, 1).contiguous(), *dst), out)      # uint8 CHW
    assert torch.equal(preprocess_image(f, *dst), out)                                       # float CHW in [-1, 1]
    if src == dst:
        assert torch.equal(out, f)


def test_preprocess_crop_is_centred_and_pil_matches_tensor():
    from PIL import Image
    from kandinsky.conditioning import preprocess_image
    # 16 x 40 picture whose columns encode their index; target 16 x 24 needs no resize -> columns 8..31 survive
    cols = torch.arange(40, dtype=torch.uint8).mul(6)
    u8 = cols.view(1, 40, 1).expand(16, 40, 3).contiguous()
    out = preprocess_image(u8, 16, 24)
    torch.testing.assert_close(out[0, 0], cols[8:32].float() / 127.5 - 1.0, atol=0, rtol=0)
    pic = Image.fromarray(u8.numpy())
    assert torch.equal(preprocess_image(pic, 16, 24), out)
    tall = u8.transpose(0, 1).contiguous()                      # 40 x 16 -> 24 x 16: rows 8..31
    torch.testing.assert_close(preprocess_image(tall, 24, 16)[0, :, 0], cols[8:32].float() / 127.5 - 1.0, atol=0, rtol=0)


def test_latents_to_visual_cond_places_frames():
    from kandinsky.conditioning import latents_to_visual_cond
    z = torch.randn(2, 4, 6, 16)
    vc, mask = latents_to_visual_cond(z, 5)
    assert vc.shape == (5, 4, 6, 16) and mask.shape == (5, 4, 6, 1)
    assert torch.equal(vc[:2], z) and vc[2:].abs().sum() == 0
    assert mask[:2].eq(1).all() and mask[2:].eq(0).all()
    with pytest.raises(ValueError):
        latents_to_visual_cond(z, 1)


def test_pipeline_refuses_image_for_a_still():
    from kandinsky.config import Conf
    from kandinsky.t2v_pipeline import Kandinsky5T2VPipeline
    conf = Conf({"model": {"num_steps": 3, "guidance_weight": 4.0, "dit_params": {}, "attention": {"type": "flash"}},
                 "metrics": {"scale_factor": [1.0, 2.0, 2.0]}})
    pipe = Kandinsky5T2VPipeline("cpu", dit=None, text_embedder=None, vae=None, conf=conf)
    with pytest.raises(ValueError, match="time_length"):
        pipe("a cat", time_length=0, width=512, height=512, seed=1, expand_prompts=False, image=torch.zeros(3, 8, 8))
