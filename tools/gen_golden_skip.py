"""Golden vectors for skip-layer guidance: the reference's fp32 DiT inside a loop with a third, block-skipping forward.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_skip.py

Writes tests/golden/dit_tiny_skip.safetensors + dit_tiny_skip_meta.json (data only).  The model is the tiny config with FOUR visual blocks
(the shipped tiny weights have two: too few for a prefix, a skipped block and a suffix at once) on synthetic weights
(oracle/k5_oracle.py synthetic_state_dict, tests/skip_reference.py WEIGHT_SEED; the meta records their SHA-256 so that a drifted generator
fails loudly); noise and prompts are those of dit_tiny.safetensors.  Per case the final latent in fp32 of

    for i in 0 .. steps-1:   c = v(x, s[i] | prompt);  v_cfg as tools/gen_golden_guidance.py forms it (w == 1: c)
                             on the steps of the case's interval: c_skip = v(x, s[i] | prompt) with the listed blocks skipped,
                                                                   v = v_cfg + g (c - c_skip)
                             x = x + (s[i+1] - s[i]) v

with c, u and c_skip from the reference's get_velocity at guidance 1 on the reference's own DiffusionTransformer3D.  For the third call the
listed blocks' `forward` is replaced: mode "block" by the identity on the visual stream, mode "attention" by a forward that runs the block's
own submodules without the self-attention branch.  Finals only.  The meta records, per case, the relative L2 distance of the bf16 oracle
loop (tests/skip_reference.py: the oracle's forwards, the engine's rounding points) from the golden; the parity tests hold the engine to
1e-2 of the oracle and 3e-2 of the golden, so g is chosen per case such that this distance is at most 1.5e-2 here.
"""
import json
import os
import sys
from types import SimpleNamespace as NS

os.environ["TORCH_COMPILE_DISABLE"] = "1"
sys.dont_write_bytecode = True

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from safetensors.torch import load_file, save_file  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STEPS, SCALE = 6, 5.0
INTERVAL = (0.6, 0.97)          # of the sigmas 1, .962, .909, .833, .714, .5 of scale 5 the steps 1..4 lie inside
CASES = {
    "block_mid": dict(blocks=[1], mode="block", g=3.0, w=5.0),
    "block_first_nocfg": dict(blocks=[0], mode="block", g=3.0, w=1.0),
    "attention_interval": dict(blocks=[1, 2], mode="attention", g=3.0, w=5.0, interval=INTERVAL),
    "with_zero_star_rescale": dict(blocks=[2], mode="block", g=3.0, w=5.0, zero_star=True, rescale=0.7),
}
MAX_ORACLE_DISTANCE = 1.5e-2


def case_mask(sig, case):
    """skip_plan of kandinsky/generation_utils.py, spelt out so that this tool needs no engine"""
    if "interval" not in case:
        return [1] * (len(sig) - 1)
    lo, hi = case["interval"]
    return [1 if lo <= float(sig[i]) <= hi else 0 for i in range(len(sig) - 1)]


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def main():
    import guidance_reference  # noqa: F401  (skip_reference composes with it)
    import skip_reference as S
    from oracle import k5_oracle as O
    g = load_file(os.path.join(GOLD, "dit_tiny.safetensors"))
    gmeta = json.load(open(os.path.join(GOLD, "dit_tiny_meta.json")))
    te = {"text_embeds": g["fwd.text"], "pooled_embed": g["fwd.pooled"]}
    ne = {"text_embeds": g["gen.null_text"], "pooled_embed": g["gen.null_pooled"]}
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    noise = g["gen.noise"]
    sig = torch.linspace(1, 0, STEPS + 1)
    sig = SCALE * sig / (1 + (SCALE - 1) * sig)
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)
    cfg = S.tiny4_config(gmeta["tiny_config"])
    ocfg = O.DitConfig(**cfg)
    sd = S.tiny4_weights(cfg)
    sha = S.weights_sha256(sd)

    # the bf16 oracle first: importing the reference turns torch.bfloat16 into torch.float32 for the rest of the process
    def o_vel(cond, tpos, skip=(), mode="block"):
        return lambda x, s: S.dit_forward_skip(sd, ocfg, torch.cat([x, *zeros], -1), cond["text_embeds"], cond["pooled_embed"],
                                               s.unsqueeze(0) * 1000, pos, tpos, (1.0, 2.0, 2.0), None, "bf16", skip, mode)
    oracle = {}
    with torch.no_grad():
        for name, c in CASES.items():
            oracle[name] = S.bf16_loop(o_vel(te, torch.arange(7)), o_vel(ne, torch.arange(4)), o_vel(te, torch.arange(7), c["blocks"], c["mode"]),
                                       noise, sig, [c["w"]] * STEPS, c["g"], case_mask(sig, c), c.get("zero_star", False), 0,
                                       c.get("rescale", 0.0))

    from _ref_import import import_reference
    r = import_reference()
    dit = r.dit.DiffusionTransformer3D(**cfg).eval()
    dit.load_state_dict(sd)
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))

    def identity(visual_embed, text_embed, time_embed, rope, sparse_params):
        return visual_embed

    def without_self_attention(block):
        def forward(visual_embed, text_embed, time_embed, rope, sparse_params):
            _, cross_attn_params, ff_params = torch.chunk(block.visual_modulation(time_embed), 3, dim=-1)
            shift, scale, gate = torch.chunk(cross_attn_params, 3, dim=-1)
            out = r.dit.apply_scale_shift_norm(block.cross_attention_norm, visual_embed, scale, shift)
            out = block.cross_attention(out, text_embed)
            visual_embed = r.dit.apply_gate_sum(visual_embed, out, gate)
            shift, scale, gate = torch.chunk(ff_params, 3, dim=-1)
            out = r.dit.apply_scale_shift_norm(block.feed_forward_norm, visual_embed, scale, shift)
            out = block.feed_forward(out)
            return r.dit.apply_gate_sum(visual_embed, out, gate)
        return forward

    def r_vel(cond, tpos, skip=(), mode="block"):   # one forward: the reference's get_velocity at guidance 1
        def vel(x, s):
            blocks = [dit.visual_transformer_blocks[b] for b in skip]
            for b in blocks:
                b.forward = identity if mode == "block" else without_self_attention(b)
            try:
                return r.gen.get_velocity(dit, torch.cat([x, *zeros], -1), s.unsqueeze(0), cond, cond, pos, tpos, tpos, 1.0, conf,
                                          sparse_params=None)
            finally:
                for b in blocks:
                    del b.forward          # the instance attribute: the class's forward is back
        return vel
    T, dist = {}, {}
    with torch.no_grad():
        for name, c in CASES.items():
            T[f"skip.{name}.final"] = S.published_loop(r_vel(te, torch.arange(7)), r_vel(ne, torch.arange(4)),
                                                       r_vel(te, torch.arange(7), c["blocks"], c["mode"]), noise, sig, [c["w"]] * STEPS, c["g"],
                                                       case_mask(sig, c), c.get("zero_star", False), 0, c.get("rescale", 0.0))
            dist[name] = rel(oracle[name], T[f"skip.{name}.final"])
            print(f"{name}: bf16 oracle vs golden {dist[name]:.3e}")
    bad = {n: d for n, d in dist.items() if not d <= MAX_ORACLE_DISTANCE}
    if bad:
        raise SystemExit(f"oracle vs golden above {MAX_ORACLE_DISTANCE}: {bad} — lower g of those cases")
    meta = {"steps": STEPS, "scheduler_scale": SCALE, "sigmas": [float(s) for s in sig], "num_visual_blocks": cfg["num_visual_blocks"],
            "weight_seed": S.WEIGHT_SEED, "weights_sha256": sha,
            "cases": {n: dict(c, mask=case_mask(sig, c)) for n, c in CASES.items()}, "oracle_vs_golden": dist,
            "noise": "dit_tiny.safetensors gen.noise", "rope_pos": {"dense": [3, 4, 6], "text": 7, "null_text": 4}}
    out = os.path.join(GOLD, "dit_tiny_skip.safetensors")
    save_file({k: v.contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_skip_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
