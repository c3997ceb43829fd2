"""What regional prompts cost: ms per step of DiffusionTransformer3D.sample at guidance 1 with regions off and with R = 1, 2 and 4 regions,
hard (a partition of the frame into vertical strips, base_weight 0: every token has one prompt) and soft (overlapping ramps, base_weight
0.5: every token blends all R + 1 streams), on the 5 s clip's latent (31, 64, 96) with synthetic weights (2B Lite, random-init, full depth
by default), next to the estimate by traffic.

The legs alternate (the order flips every round), `--rounds` times; a leg's wall time is taken between two device synchronisations and
divided by the steps.  The combine kernel is also timed on its own with events over `--kernel_iters` launches at the clip's [tokens][1792],
in place as the engine runs it, for every R, hard and soft.  Estimate: a soft combine reads R + 1 streams and writes one, (R + 2) x tokens x
1792 x 2 bytes per block, a hard one reads one stream and writes one, at `--bandwidth` TB/s (default the figure DESIGN.md §4 gives for
`ln_kernel`).  One JSON line, appended to profiles/region_bench.jsonl.

    python tools/region_bench.py [--steps 4] [--rounds 2] [--blocks 32] [--kernel_iters 50] [--bandwidth 5.3]
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
RS = (1, 2, 4)
LEGS = ("off",) + tuple(f"{kind}{R}" for R in RS for kind in ("hard", "soft"))


def region_masks(kind, R, T, H, W):
    """hard: R vertical strips that partition the frame (R = 1: the left half; the right half is uncovered and sees the base prompt);
    soft: R overlapping ramps over the columns, 0.8 at most"""
    col = torch.arange(W, dtype=torch.float32).expand(T, H, W)
    if kind == "hard":
        if R == 1:
            return (col < W // 2).float()[None].contiguous()
        edges = [round(r * W / R) for r in range(R + 1)]
        return torch.stack([((col >= edges[r]) & (col < edges[r + 1])).float() for r in range(R)])
    centres = [(r + 0.5) * W / R for r in range(R)]
    return torch.stack([0.8 * (1.0 - (col - c).abs() / W).clamp(0.05, 1.0) for c in centres])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4, help="Euler steps per leg")
    ap.add_argument("--rounds", type=int, default=2, help="rotations (each runs every leg)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--kernel_iters", type=int, default=50, help="launches per kernel timing")
    ap.add_argument("--bandwidth", type=float, default=5.3, help="TB/s the estimate is computed at")
    ap.add_argument("--shape", type=int, nargs=3, default=(31, 64, 96), metavar=("T", "H", "W"), help="latent shape (default: the 5 s clip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_bench.jsonl"))
    args = ap.parse_args()
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule
    from kandinsky.models.dit import DiffusionTransformer3D

    dev = torch.device("cuda", 0)
    with torch.device("meta"):
        dit = DiffusionTransformer3D(**dict(LITE, num_visual_blocks=args.blocks))
    dit.init_synthetic(dev, seed=0)
    g = torch.Generator().manual_seed(1)
    te = {"text_embeds": torch.randn(64, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
    ne = {"text_embeds": torch.randn(32, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
    region_text = [{"text_embeds": torch.randn(48, 3584, generator=g).to(dev)} for _ in range(max(RS))]
    sig = sigma_schedule(50, 5.0).tolist()[:args.steps + 1]
    T, H, W = args.shape
    tokens, D = T * (H // 2) * (W // 2), LITE["model_dim"]
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    noise = torch.randn(T, H, W, 16, generator=g).to(dev)

    def leg(name):
        if name == "off":
            dit.clear_regions()
        else:
            kind, R = name[:4], int(name[4:])
            dit.set_regions(region_text[:R], [torch.arange(48)] * R, region_masks(kind, R, T, H, W), 0.0 if kind == "hard" else 0.5)
        dit.regions_state(reset=True)
        lat = noise.clone()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), 1.0, scale_factor=(1.0, 2.0, 2.0))
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        combines = dit.regions_state()[2]
        dit.clear_regions()
        assert combines == (0 if name == "off" else args.steps * args.blocks), (name, combines)
        return ms, lat

    leg(f"soft{max(RS)}")   # warm-up: workspaces, RoPE tables, every region stream's buffers
    series = {k: [] for k in LEGS}
    final = {}
    for r in range(args.rounds):
        for name in (LEGS if r % 2 == 0 else LEGS[::-1]):
            ms, lat = leg(name)
            series[name].append(ms)
            final[name] = lat
    for name in LEGS[1:]:
        assert torch.isfinite(final[name]).all() and not torch.equal(final[name], final["off"]), f"{name} left the latent as it was"

    L, st = E.lib(), E.stream_ptr(dev)
    z0 = torch.randn(tokens, D, generator=g).to(dev).bfloat16()
    zr = torch.randn(max(RS), tokens, D, generator=g).to(dev).bfloat16()

    def kernel_us(fn):
        fn()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.kernel_iters):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e3 / args.kernel_iters

    kernel, expected = {}, {}
    for name in LEGS[1:]:
        kind, R = name[:4], int(name[4:])
        w = E.region_weights(region_masks(kind, R, T, H, W).to(dev), (1, 2, 2), 0.0 if kind == "hard" else 0.5)
        kernel[name] = round(kernel_us(lambda: L.k5_region_combine_bf16(z0.data_ptr(), zr.data_ptr(), tokens * D, R, w.data_ptr(), R + 1, z0.data_ptr(),
                                                                         tokens, D, D, st)), 2)
        streams = 1 if kind == "hard" else R + 1
        expected[name] = round((streams + 1) * tokens * D * 2 / (args.bandwidth * 1e12) * 1e6, 2)
    us_weights = kernel_us(lambda: E.region_weights(region_masks("soft", 4, T, H, W).to(dev), (1, 2, 2), 0.5))
    med = {k: statistics.median(v) for k, v in series.items()}
    line = {"latent": [T, H, W], "tokens": tokens, "guidance": 1.0, "steps": args.steps, "blocks": args.blocks, "rounds": args.rounds,
            "bandwidth_TBps": args.bandwidth, "region_text_len": 48,
            "ms_per_step": {k: round(med[k], 3) for k in LEGS},
            "series": {k: [round(v, 3) for v in series[k]] for k in LEGS},
            "spread": {k: round(max(series[k]) - min(series[k]), 3) for k in LEGS},
            "extra_ms_per_step": {k: round(med[k] - med["off"], 3) for k in LEGS[1:]},
            "extra_percent": {k: round(100 * (med[k] - med["off"]) / med["off"], 3) for k in LEGS[1:]},
            "us_combine_in_place": kernel, "expected_us_combine": expected, "stream_MB": round(tokens * D * 2 / 1e6, 2),
            "us_weights_with_upload": round(us_weights, 2)}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
