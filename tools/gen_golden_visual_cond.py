"""Golden vectors for visual conditioning (image-to-video): the reference's own arithmetic with the conditioning channels filled.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_visual_cond.py

Writes tests/golden/dit_tiny_visual_cond.safetensors + dit_tiny_visual_cond_meta.json (data only):
  * cond.*   conditioned trajectories of the tiny DiT (weights, noise and prompts of dit_tiny.safetensors), 4 steps, s = 5, w = 1
             and w = 5.  Each step is the reference's loop body (generation_utils.py:104-128) with its `get_velocity`, the zero
             `visual_cond` / `visual_cond_mask` replaced by the fixture's: a latent and mask 1 on frame 0, zeros elsewhere (stored:
             frame 0's latent; the final latent, and for w = 5 the latents after steps 1..3).
  * nabla.*  the same at the NABLA shape of `gen.nabla` (6 x 32 x 32, 2 steps, w = 2), conditioning on frame 0 (stored: that frame's
             latent; the final latent at every fourth row and column, and its sum of squares).
  * enc.*    1-frame encodes (moments = quant_conv(encoder(x))) by the reference VAE with the tiny encoder weights of
             vae_enc_tiny.safetensors (not copied here): one untiled, one through the reference's spatial tiling.
Inputs are bf16-representable and stored as bf16; outputs are fp32.  The reference runs in fp32 on the CPU under the patches of oracle/_ref_import.py and the diffusers shims of
oracle/gen_golden_vae.py.
"""
import json
import os
import sys
import types
from types import SimpleNamespace as NS

os.environ["TORCH_COMPILE_DISABLE"] = "1"
sys.dont_write_bytecode = True

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402
from safetensors.torch import load_file, save_file  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STEPS, SCALE, WEIGHTS = 4, 5.0, (1.0, 5.0)
NABLA_STEPS, NABLA_SCALE, NABLA_W = 2, 5.0, 2.0


def conf_ns(attn):
    return NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(**attn)), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))


def frame0_cond(shape, gen):
    """(visual_cond, visual_cond_mask): a random bf16-representable latent on frame 0 with mask 1 there, zeros elsewhere."""
    vc = torch.zeros(shape)
    vc[0] = torch.randn(shape[1:], generator=gen).bfloat16().float()
    mask = torch.zeros(*shape[:-1], 1)
    mask[0] = 1.0
    return vc, mask


def conditioned_loop(kgen, model, noise, steps, scale, w, te, ne, pos, tpos, ntpos, conf, vc, mask):
    """reference generate (generation_utils.py:80-129) from explicit noise, conditioning channels from the fixture."""
    img = noise.clone()
    sparse_params = kgen.get_sparse_params(conf, {"visual": img}, "cpu")
    timesteps = torch.linspace(1, 0, steps + 1)
    timesteps = scale * timesteps / (1 + (scale - 1) * timesteps)
    traj = []
    for timestep, timestep_diff in zip(timesteps[:-1], torch.diff(timesteps)):
        time = timestep.unsqueeze(0)
        model_input = torch.cat([img, vc, mask], dim=-1)
        pred_velocity = kgen.get_velocity(model, model_input, time, te, ne, pos, tpos, ntpos, w, conf, sparse_params=sparse_params)
        img = img + timestep_diff * pred_velocity
        traj.append(img.clone())
    return img, torch.stack(traj)


def dit_goldens(T, meta):
    from _ref_import import import_reference
    r = import_reference()
    g = load_file(os.path.join(GOLD, "dit_tiny.safetensors"))
    gmeta = json.load(open(os.path.join(GOLD, "dit_tiny_meta.json")))
    cfg = {k: (tuple(v) if isinstance(v, list) else v) for k, v in gmeta["tiny_config"].items()}
    assert cfg["visual_cond"]
    dit = r.dit.DiffusionTransformer3D(**cfg).eval()
    dit.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    te = {"text_embeds": g["fwd.text"], "pooled_embed": g["fwd.pooled"]}
    ne = {"text_embeds": g["gen.null_text"], "pooled_embed": g["gen.null_pooled"]}
    gen = torch.Generator().manual_seed(2024)
    with torch.no_grad():
        pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
        vc, mask = frame0_cond(tuple(g["gen.noise"].shape), gen)
        T["cond.visual_cond0"] = vc[0].bfloat16()                        # frame 0 (exact in bf16); the rest and the mask follow from it
        for w in WEIGHTS:
            final, traj = conditioned_loop(r.gen, dit, g["gen.noise"], STEPS, SCALE, w, te, ne, pos, torch.arange(7), torch.arange(4),
                                           conf_ns(dict(type="flash")), vc, mask)
            assert torch.equal(traj[-1], final)                          # the last latent of the trajectory is the final one
            T[f"cond.{STEPS}_{SCALE}_{w}.final"] = final
            if w != 1.0:                                                 # the CFG case also keeps its trajectory
                T[f"cond.{STEPS}_{SCALE}_{w}.latents"] = traj[:-1]
        meta["cond_cases"] = [[STEPS, SCALE, w] for w in WEIGHTS]

        attn = gmeta["nabla_attention"]
        npos = [torch.arange(6), torch.arange(16), torch.arange(16)]
        nvc, nmask = frame0_cond(tuple(g["gen.nabla.noise"].shape), gen)
        T["nabla.visual_cond0"] = nvc[0].bfloat16()                      # frame 0 (exact in bf16); the rest and the mask follow from it
        final, _ = conditioned_loop(r.gen, dit, g["gen.nabla.noise"], NABLA_STEPS, NABLA_SCALE, NABLA_W, te, ne, npos, torch.arange(7),
                                    torch.arange(4), conf_ns(attn), nvc, nmask)
        T["nabla.final.sample"] = final[:, ::4, ::4].contiguous()       # every 4th row and column keeps the fixture small
        meta["nabla_case"] = {"steps": NABLA_STEPS, "scheduler_scale": NABLA_SCALE, "guidance_weight": NABLA_W, "attention": attn,
                              "sample": "final[:, ::4, ::4]", "final_sumsq": float(final.double().pow(2).sum())}
        meta["rope_pos"] = {"dense": [3, 4, 6], "nabla": [6, 16, 16], "text": 7, "null_text": 4}


def encode_goldens(T, meta):
    import gen_golden_vae as G
    G._install_shims()
    for name in ("kandinsky", "kandinsky.models"):
        sys.modules.pop(name, None)
    for name, sub in (("kandinsky", "/kandinsky"), ("kandinsky.models", "/kandinsky/models")):
        m = types.ModuleType(name)
        m.__path__ = [G.REF + sub]
        sys.modules[name] = m
    import kandinsky.models.vae as kvae
    g = load_file(os.path.join(GOLD, "vae_enc_tiny.safetensors"))
    cfg = json.load(open(os.path.join(GOLD, "vae_enc_meta.json")))["config"]
    vae = kvae.AutoencoderKLHunyuanVideo(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in cfg.items()}).eval()
    missing, _ = vae.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")}, strict=False)
    assert not [k for k in missing if k.startswith("encoder.") or k.startswith("quant_conv")], missing
    gen = torch.Generator().manual_seed(31)
    with torch.no_grad():
        x = (torch.rand(1, 3, 1, 32, 48, generator=gen) * 2 - 1).bfloat16().float()      # bf16-representable: stored as bf16
        vae.apply_tiling((1, 1, 32, 48), (1, 32, 48))                  # one tile = the whole picture
        T["enc.x"], T["enc.moments"] = x.bfloat16(), vae._encode(x)
        xs = (torch.rand(1, 3, 1, 80, 80, generator=gen) * 2 - 1).bfloat16().float()
        vae.apply_tiling((1, 1, 48, 48), (1, 32, 32))                  # 1 frame through tiled_encode
        T["enc.tiled.x"], T["enc.tiled.moments"] = xs.bfloat16(), vae._encode(xs)
        meta["enc_tiled_case"] = {"tile": [1, 1, 48, 48], "stride": [1, 32, 32]}


def main():
    T, meta = {}, {}
    dit_goldens(T, meta)
    encode_goldens(T, meta)
    out = os.path.join(GOLD, "dit_tiny_visual_cond.safetensors")
    save_file({k: v.contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_visual_cond_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
