"""Golden vectors for regional prompts: the reference's fp32 DiT with the rule of include/k5.h (k5_region_combine_bf16, k5_region_weights_f32)
applied in float32 around its own cross-attention modules.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_regions.py

Writes tests/golden/dit_tiny_regions.safetensors + dit_tiny_regions_meta.json (data only).  The tiny DiT, inputs, noise and prompts of
dit_tiny.safetensors, shape (3, 8, 12, 16); the base prompt is fwd.text / fwd.pooled.  The two region prompts come from
torch.Generator().manual_seed(31): randn(5, 96) then randn(6, 96), positions arange(5) and arange(6).  Per visual block, on the conditional
forward only:

    z_0 = attention(q, k_0, v_0),  z_r = attention(q, k_r, v_r)     the module's own get_qkv / norm_qk / attention, the same queries
    m_r(token) = mean of the token's patch_size cells of mask r;  raw_0 = base_weight + max(0, 1 - sum_r m_r);  raw_r = m_r;  w = raw / sum raw
    out = sum_i w_i z_i per token;  then the module's out_l

The region tokens go through text_embeddings and the text blocks with their own RoPE positions and the forward's own time embedding (the
base prompt's pooled embedding).  The token weights are put in the blocks' token order by the reference's own fractal_flatten.

Set A (hard): region 0 = columns < 6, region 1 = columns >= 6, base_weight 0.  Set B (soft): ramp = linspace(0, 1, 12) over the columns,
region 0 = 0.8 (1 - ramp) on all frames, region 1 = 0.8 ramp on frames 1.. and zero on frame 0, base_weight 0.5.  For each: one forward
velocity (the fwd.* inputs) and the final latent of the 4-step loop at guidance 1 and 5 (scheduler_scale 5, gen.noise).  One NABLA case: the
existing NABLA golden's setup (golden_meta["nabla_attention"], shape (6, 32, 32, 16), gen.nabla.noise, 2 steps, guidance 2.0) with hard left /
right masks at column 16.  Asserted and recorded: delta, the relative L2 of each result against the plain result of the same run, >= 0.04.
"""
import json
import os
import sys
from types import SimpleNamespace as NS

os.environ["TORCH_COMPILE_DISABLE"] = "1"
sys.dont_write_bytecode = True

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402
from safetensors.torch import load_file, save_file  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STEPS, SCALE, WEIGHTS, DELTA_MIN = 4, 5.0, (1.0, 5.0), 0.04
PATCH = (1, 2, 2)


def token_weights(masks, base_weight, patch):
    """the definition, float32: masks (R, T, H, W) -> (T/pt, H/ph, W/pw, R + 1)"""
    R, T, H, W = masks.shape
    pt, ph, pw = patch
    m = masks.float().reshape(R, T // pt, pt, H // ph, ph, W // pw, pw).mean(dim=(2, 4, 6))
    sm = m.sum(0)
    raw0 = base_weight + (1.0 - sm).clamp_min(0.0)
    raw = torch.cat([raw0[None], m], 0)
    return (raw / raw.sum(0, keepdim=True)).permute(1, 2, 3, 0).contiguous()


class Regions:
    """Regional prompts on a reference DiT: while `params` = (masks, base_weight) is set, a forward whose text tokens are `base` attends every
    visual block to the region streams as well.  Only the modules' own methods are called."""

    def __init__(self, ref, dit, base, texts, positions):
        self.ref, self.dit, self.base, self.texts, self.positions = ref, dit, base, texts, positions
        self.params, self.active, self.busy, self.streams, self.w = None, False, False, None, None
        dit.register_forward_pre_hook(self.on_forward, with_kwargs=True)
        dit.text_transformer_blocks[0].register_forward_pre_hook(self.on_first_text_block)
        for b in dit.visual_transformer_blocks:
            ca = b.cross_attention
            ca.forward = lambda x, cond, ca=ca: self.cross(ca, x, cond)

    def on_forward(self, module, args, kwargs):
        self.active = self.params is not None and args[1] is self.base   # the unconditional forward stays as it is
        self.streams = None
        if self.active:
            masks, bw = self.params
            w = token_weights(masks, bw, PATCH)
            sp = kwargs.get("sparse_params")
            to_fractal = sp["to_fractal"] if sp is not None else False
            self.w, _ = self.ref.utils.fractal_flatten(w, w, w.shape[:-1], block_mask=to_fractal)   # the blocks' token order

    def on_first_text_block(self, module, args):
        if not self.active or self.busy:
            return
        time_embed = args[1]   # one per forward: the base prompt's pooled embedding went into it
        self.busy = True
        self.streams = []
        for text, pos in zip(self.texts, self.positions):
            t = self.dit.text_embeddings(text)
            rope = self.dit.text_rope_embeddings(pos)
            for blk in self.dit.text_transformer_blocks:
                t = blk(t, time_embed, rope)
            self.streams.append(t)
        self.busy = False

    def cross(self, ca, x, cond):
        q, k, v = ca.get_qkv(x, cond)
        q, k = ca.norm_qk(q, k)
        z = ca.attention(q, k, v)
        if self.active:
            out = self.w[:, :1] * z.float()
            for r, stream in enumerate(self.streams):
                _, kr, vr = ca.get_qkv(x, stream)
                _, kr = ca.norm_qk(q, kr)          # q is normalised already and not used again
                out = out + self.w[:, r + 1:r + 2] * ca.attention(q, kr, vr).float()
            z = out
        return ca.out_l(z)


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def conf_ns(attn):
    return NS(model=NS(dit_params=NS(patch_size=PATCH), attention=NS(**attn)), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))


def main():
    from _ref_import import import_reference
    r = import_reference()
    g = load_file(os.path.join(GOLD, "dit_tiny.safetensors"))
    gmeta = json.load(open(os.path.join(GOLD, "dit_tiny_meta.json")))
    cfg = {k: (tuple(v) if isinstance(v, list) else v) for k, v in gmeta["tiny_config"].items()}
    assert tuple(cfg["patch_size"]) == PATCH
    dit = r.dit.DiffusionTransformer3D(**cfg).eval()
    dit.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    te = {"text_embeds": g["fwd.text"], "pooled_embed": g["fwd.pooled"]}
    ne = {"text_embeds": g["gen.null_text"], "pooled_embed": g["gen.null_pooled"]}
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    gen = torch.Generator().manual_seed(31)
    texts = [torch.randn(5, 96, generator=gen), torch.randn(6, 96, generator=gen)]
    reg = Regions(r, dit, te["text_embeds"], texts, [torch.arange(5), torch.arange(6)])

    T, H, W = 3, 8, 12
    col = torch.arange(W).expand(T, H, W)
    ramp = torch.linspace(0, 1, W).expand(T, H, W)
    b1 = (0.8 * ramp).clone()
    b1[0] = 0.0
    sets = {"A": (torch.stack([(col < 6).float(), (col >= 6).float()]), 0.0),
            "B": (torch.stack([0.8 * (1 - ramp), b1]).contiguous(), 0.5)}

    def run_all(params):
        out = {}
        reg.params = params
        with torch.no_grad():
            out["fwd"] = dit(g["fwd.x"], te["text_embeds"], te["pooled_embed"], g["fwd.time"], pos, torch.arange(7), scale_factor=(1.0, 2.0, 2.0))
            for w in WEIGHTS:
                out[f"gen.{w}"] = r.gen.generate(dit, "cpu", tuple(g["gen.noise"].shape), STEPS, te, ne, pos, torch.arange(7), torch.arange(4), w,
                                                 SCALE, conf_ns(dict(type="flash")), seed=gmeta["gen_seed"])
        reg.params = None
        return out

    plain = run_all(None)
    # the hooks are idle without parameters: the plain runs are the goldens of dit_tiny.safetensors
    assert torch.equal(plain["fwd"], g["fwd.out"])
    for w in WEIGHTS:
        assert torch.equal(plain[f"gen.{w}"], g[f"gen.{STEPS}_{SCALE}_{w}.final"])

    out_t = {"regions.text0": texts[0], "regions.text1": texts[1]}
    meta = {"steps": STEPS, "scheduler_scale": SCALE, "weights": list(WEIGHTS), "delta_min": DELTA_MIN, "prompt_seed": 31,
            "rope_pos": {"dense": [3, 4, 6], "text": 7, "regions": [5, 6]}, "sets": {}}
    for name, (masks, bw) in sets.items():
        res = run_all((masks, bw))
        deltas = {k: rel(res[k], plain[k]) for k in res}
        print(name, "delta", {k: round(d, 4) for k, d in deltas.items()})
        assert min(deltas.values()) >= DELTA_MIN, (name, deltas)
        meta["sets"][name] = {"base_weight": bw, "delta": deltas}
        out_t[f"regions.{name}.masks"] = masks
        out_t[f"regions.{name}.fwd.out"] = res["fwd"]
        for w in WEIGHTS:
            out_t[f"regions.{name}.gen.{w}.final"] = res[f"gen.{w}"]

    # the NABLA case: the existing NABLA golden's run with hard left / right masks
    attn = gmeta["nabla_attention"]
    nshape = tuple(g["gen.nabla.noise"].shape)
    npos = [torch.arange(nshape[0]), torch.arange(nshape[1] // 2), torch.arange(nshape[2] // 2)]
    ncol = torch.arange(nshape[2]).expand(*nshape[:3])
    nmasks = torch.stack([(ncol < 16).float(), (ncol >= 16).float()])

    def run_nabla(params):
        reg.params = params
        with torch.no_grad():
            x = r.gen.generate(dit, "cpu", nshape, 2, te, ne, npos, torch.arange(7), torch.arange(4), 2.0, 5.0, conf_ns(attn), seed=gmeta["gen_seed"])
        reg.params = None
        return x

    assert torch.equal(run_nabla(None), g["gen.nabla.final"])
    nres = run_nabla((nmasks, 0.0))
    ndelta = rel(nres, g["gen.nabla.final"])
    print("nabla delta", round(ndelta, 4))
    assert ndelta >= DELTA_MIN, ndelta
    meta["nabla"] = {"base_weight": 0.0, "steps": 2, "guidance_weight": 2.0, "split_column": 16, "delta": ndelta}
    out_t["regions.nabla.masks"] = nmasks
    out_t["regions.nabla.final"] = nres

    out = os.path.join(GOLD, "dit_tiny_regions.safetensors")
    save_file({k: v.float().contiguous() for k, v in out_t.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_regions_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
