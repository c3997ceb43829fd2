"""Several samples per call vs one sample at a time: ms per sample-step of k5_sample_many over B samples against B sequential k5_sample calls
on the same handle (2B Lite, random-init weights, full depth by default).

Cases: config 1's shape (latent (13, 32, 32), 3328 tokens) at guidance 1 and 5 for B = 1, 2, 4, 8; one 512 x 768 frame (latent
(1, 64, 96), 1536 tokens) at guidance 1 and 5 for the same B; config 2's shape (latent (31, 64, 96), 47 616 tokens) at guidance 5 for
B = 1.  Each case alternates the two legs (which one goes first alternates too), `--rounds` times; a leg's wall time is taken between
two device synchronisations and divided by B * steps.  Every round also checks that the two legs give the same bits.  One JSON line
per case: the median ms per sample-step of each leg, the spread (max - min) of each, and batch / sequential.

    python tools/batch_bench.py [--steps 3] [--rounds 3] [--blocks 32] [--cases c1,img,c2] [--guidance 1,5] [--batches 1,2,4,8]
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
SHAPES = {"c1": (13, 32, 32), "img": (1, 64, 96), "c2": (31, 64, 96)}


def cases(which, guidances, batches):
    out = []
    for name in which:
        if name == "c2":
            out.append((name, 5.0, 1))
            continue
        for w in guidances:
            for B in batches:
                out.append((name, w, B))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="Euler steps per leg")
    ap.add_argument("--rounds", type=int, default=3, help="alternations (each runs both legs)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--cases", default="c1,img,c2")
    ap.add_argument("--guidance", default="1,5", help="guidance weights of the c1 / img cases")
    ap.add_argument("--batches", default="1,2,4,8", help="B of the c1 / img cases")
    args = ap.parse_args()
    from kandinsky.generation_utils import sigma_schedule
    from kandinsky.models.dit import DiffusionTransformer3D

    dev = torch.device("cuda", 0)
    with torch.device("meta"):
        dit = DiffusionTransformer3D(**dict(LITE, num_visual_blocks=args.blocks))
    dit.init_synthetic(dev, seed=0)
    g = torch.Generator().manual_seed(1)
    te_all = [{"text_embeds": torch.randn(64 + 24 * b, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
              for b in range(8)]
    ne = {"text_embeds": torch.randn(32, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
    sig = sigma_schedule(50, 5.0).tolist()[:args.steps + 1]

    for name, w, B in cases(args.cases.split(","), [float(v) for v in args.guidance.split(",")],
                             [int(v) for v in args.batches.split(",")]):
        T, H, W = SHAPES[name]
        pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
        tes = te_all[:B]
        tps = [torch.arange(t["text_embeds"].shape[0]) for t in tes]
        noise = torch.randn(B, T, H, W, 16, generator=g).to(dev)

        def leg(batched):
            lat = noise.clone()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if batched:
                dit.sample_many(lat, sig, tes, ne, pos, tps, torch.arange(32), w, scale_factor=(1.0, 2.0, 2.0))
            else:
                for b in range(B):
                    dit.sample(lat[b], sig, tes[b], ne, pos, tps[b], torch.arange(32), w, scale_factor=(1.0, 2.0, 2.0))
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3 / (B * args.steps), lat

        leg(True)   # warm-up: workspaces, RoPE tables
        seq, bat, same = [], [], True
        for r in range(args.rounds):
            order = (False, True) if r % 2 == 0 else (True, False)
            got = {}
            for batched in order:
                ms, lat = leg(batched)
                (bat if batched else seq).append(ms)
                got[batched] = lat
            same = same and torch.equal(got[True], got[False])
        line = {"case": name, "latent": [T, H, W], "tokens": T * (H // 2) * (W // 2), "guidance": w, "B": B, "steps": args.steps,
                "blocks": args.blocks, "rounds": args.rounds,
                "ms_per_sample_step_sequential": round(statistics.median(seq), 3),
                "ms_per_sample_step_batched": round(statistics.median(bat), 3),
                "spread_sequential": round(max(seq) - min(seq), 3), "spread_batched": round(max(bat) - min(bat), 3),
                "batched_over_sequential": round(statistics.median(bat) / statistics.median(seq), 4), "bit_identical": same}
        print(json.dumps(line), flush=True)
        if not same:
            sys.exit("batched and sequential legs differ")


if __name__ == "__main__":
    main()
