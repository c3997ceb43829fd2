"""Golden vectors for the forecast cache: the reference's fp32 DiT with the rule of include/k5.h (k5_forecast_update_bf16) around its visual
blocks, in fp32 throughout.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_forecast.py

Writes tests/golden/dit_tiny_forecast.safetensors + dit_tiny_forecast_meta.json (data only).  The model is the tiny config with four visual
blocks on the synthetic weights of tests/skip_reference.py (the meta records their SHA-256); noise and prompts are those of
dit_tiny.safetensors.  Per case the final latent in fp32 of the Euler / CFG loop whose forwards are the reference's own
before_text_transformer_blocks / text blocks / before_visual_transformer_blocks / after_blocks with, in place of the loop over the visual
blocks, tests/forecast_reference.py's Cache in mode "fp32" (a full step runs the reference's blocks, a forecast step extrapolates).
The meta records per case `oracle_vs_golden`, the relative L2 distance of the bf16 oracle loop (the oracle's forwards, the engine's rounding
points) from the golden — the parity test holds the engine to 1.5 x that — and, for information only, the fp32 distance of the forecast run
from the full run at orders 0, 1 and 2 under the case's plan: on random weights it says nothing about quality.
"""
import json
import os
import sys

os.environ["TORCH_COMPILE_DISABLE"] = "1"
sys.dont_write_bytecode = True

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from safetensors.torch import load_file, save_file  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SCALE = 5.0
PLANS = {9: (3, 2, 1), 8: (2, 3, 1)}     # steps -> (interval, warmup, tail): forecasts with k = 1, 2 and an update with g = 3 | the alternating plan
CASES = {"p9_w5_o2": dict(steps=9, w=5.0, order=2), "p9_w1_o1": dict(steps=9, w=1.0, order=1),
         "p8_w5_o1": dict(steps=8, w=5.0, order=1), "p8_w1_o2": dict(steps=8, w=1.0, order=2)}


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def main():
    import forecast_reference as FR
    import skip_reference as S
    from oracle import k5_oracle as O
    g = load_file(os.path.join(GOLD, "dit_tiny.safetensors"))
    gmeta = json.load(open(os.path.join(GOLD, "dit_tiny_meta.json")))
    conds = [(g["fwd.text"], g["fwd.pooled"], torch.arange(7)), (g["gen.null_text"], g["gen.null_pooled"], torch.arange(4))]
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    noise = g["gen.noise"]
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)
    cfg = S.tiny4_config(gmeta["tiny_config"])
    ocfg = O.DitConfig(**cfg)
    sd = S.tiny4_weights(cfg)

    def sigmas(steps):
        t = torch.linspace(1, 0, steps + 1)
        return SCALE * t / (1 + (SCALE - 1) * t)

    # the bf16 oracle first: importing the reference turns torch.bfloat16 into torch.float32 for the rest of the process
    def o_vel(cache):
        def vel(x, s, step, slot):
            text, pooled, tpos = conds[slot]
            return FR.dit_forward_forecast(sd, ocfg, torch.cat([x, *zeros], -1), text, pooled, s.unsqueeze(0) * 1000, pos, tpos, (1.0, 2.0, 2.0),
                                           None, "bf16", cache, step, slot)
        return vel
    oracle = {}
    for name, c in CASES.items():
        full = FR.plan(c["steps"], *PLANS[c["steps"]])
        oracle[name] = FR.bf16_loop(o_vel(FR.Cache(c["order"], full, "bf16")), noise, sigmas(c["steps"]), c["w"])

    from _ref_import import import_reference
    r = import_reference()
    dit = r.dit.DiffusionTransformer3D(**cfg).eval()
    dit.load_state_dict(sd)

    def r_vel(cache):   # the reference's forward (dit.py:155-181) with the cache around its loop over the visual blocks
        def vel(x, s, step, slot):
            text, pooled, tpos = conds[slot]
            text_embed, time_embed, text_rope, visual_embed = dit.before_text_transformer_blocks(text, s.unsqueeze(0) * 1000, pooled,
                                                                                                 torch.cat([x, *zeros], -1), tpos)
            for block in dit.text_transformer_blocks:
                text_embed = block(text_embed, time_embed, text_rope)
            visual_embed, visual_shape, to_fractal, visual_rope = dit.before_visual_transformer_blocks(visual_embed, pos, (1.0, 2.0, 2.0), None)

            def blocks(v):
                for block in dit.visual_transformer_blocks:
                    v = block(v, text_embed, time_embed, visual_rope, None)
                return v
            visual_embed = blocks(visual_embed) if cache is None else cache.around(visual_embed, blocks, step, slot)
            return dit.after_blocks(visual_embed, visual_shape, to_fractal, text_embed, time_embed)
        return vel
    T, dist, info = {}, {}, {}
    with torch.no_grad():
        plain = {}
        for name, c in CASES.items():
            steps, w = c["steps"], c["w"]
            full = FR.plan(steps, *PLANS[steps])
            sig = sigmas(steps)
            if (steps, w) not in plain:
                plain[(steps, w)] = FR.published_loop(r_vel(None), noise, sig, w)
            by_order = {o: FR.published_loop(r_vel(FR.Cache(o, full, "fp32")), noise, sig, w) for o in (0, 1, 2)}
            T[f"forecast.{name}.final"] = by_order[c["order"]]
            dist[name] = rel(oracle[name], by_order[c["order"]])
            info[name] = {f"order{o}": rel(by_order[o], plain[(steps, w)]) for o in (0, 1, 2)}
            print(f"{name}: bf16 oracle vs golden {dist[name]:.3e}; fp32 forecast vs full run {info[name]}")
    meta = {"scheduler_scale": SCALE, "plans": {str(k): list(v) for k, v in PLANS.items()}, "num_visual_blocks": cfg["num_visual_blocks"],
            "weight_seed": S.WEIGHT_SEED, "weights_sha256": S.weights_sha256(sd),
            "cases": {n: dict(c, full=FR.plan(c["steps"], *PLANS[c["steps"]])) for n, c in CASES.items()}, "oracle_vs_golden": dist,
            "fp32_forecast_vs_full_run": info, "noise": "dit_tiny.safetensors gen.noise", "rope_pos": {"dense": [3, 4, 6], "text": 7, "null_text": 4}}
    out = os.path.join(GOLD, "dit_tiny_forecast.safetensors")
    save_file({k: v.contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_forecast_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
