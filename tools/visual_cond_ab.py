"""A/B: what visual conditioning costs per sampler step at config 2 (2B Lite, 768x512 5 s latent (31, 64, 96), guidance 1).

One process, one handle: legs of `--steps` Euler steps through k5_sample (no conditioning) and k5_sample_cond (a frame-0 conditioning
latent + mask), alternating which leg goes first, `--rounds` times.  Each leg starts from the same noise and runs the same steps of the
50-step schedule; its wall time is taken between two device synchronisations.  Prints one JSON line: the median ms per step of each
leg, their difference and its share of a step.

    python tools/visual_cond_ab.py [--steps 3] [--rounds 5] [--blocks 32]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "kandinsky-5_amd"))

import torch  # noqa: E402

LITE = dict(in_visual_dim=16, out_visual_dim=16, time_dim=512, patch_size=(1, 2, 2), model_dim=1792, ff_dim=7168, num_text_blocks=2,
            num_visual_blocks=32, axes_dims=(16, 24, 24), visual_cond=True, in_text_dim=3584, in_text_dim2=768)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="Euler steps per leg")
    ap.add_argument("--rounds", type=int, default=5, help="alternations (each runs both legs)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    args = ap.parse_args()
    from kandinsky.generation_utils import sigma_schedule
    from kandinsky.models.dit import DiffusionTransformer3D

    dev = torch.device("cuda", 0)
    T, H, W, L = 31, 64, 96, 256
    with torch.device("meta"):
        dit = DiffusionTransformer3D(**dict(LITE, num_visual_blocks=args.blocks))
    dit.init_synthetic(dev, seed=0, host_rng=True)
    noise = torch.randn(T, H, W, 16, generator=torch.Generator().manual_seed(6554)).to(dev)
    g = torch.Generator().manual_seed(6555)
    te = {"text_embeds": torch.randn(L, 3584, generator=g).bfloat16().to(dev), "pooled_embed": torch.randn(1, 768, generator=g).bfloat16().to(dev)}
    cond = torch.zeros(T, H, W, 17)
    cond[0, ..., :16] = torch.randn(H, W, 16, generator=g)
    cond[0, ..., 16] = 1.0
    cond = cond.to(dev).contiguous()
    vpos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    sig = sigma_schedule(50, 5.0).tolist()
    latent = torch.empty_like(noise)

    def leg(conditioned):
        latent.copy_(noise)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dit.sample(latent, sig[:args.steps + 1], te, te, vpos, torch.arange(L), torch.arange(L), 1.0, scale_factor=(1.0, 2.0, 2.0),
                   visual_cond=cond if conditioned else None)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / args.steps

    leg(False)
    leg(True)                                    # warm-up: workspaces, RoPE tables, kernels' first launches
    ms = {False: [], True: []}
    for r in range(args.rounds):
        for c in ((False, True) if r % 2 == 0 else (True, False)):
            ms[c].append(leg(c))
    plain, condm = statistics.median(ms[False]), statistics.median(ms[True])
    print(json.dumps({"tool": "visual_cond_ab", "config": "2 (31,64,96) w=1", "blocks": args.blocks, "steps_per_leg": args.steps,
                      "rounds": args.rounds, "k5_sample_ms_per_step": round(plain, 3), "k5_sample_cond_ms_per_step": round(condm, 3),
                      "delta_ms_per_step": round(condm - plain, 3), "delta_pct": round(100.0 * (condm - plain) / plain, 3),
                      "legs_plain_ms": [round(v, 2) for v in ms[False]], "legs_cond_ms": [round(v, 2) for v in ms[True]]}))


if __name__ == "__main__":
    main()
