"""What spatial context windows (tiles) cost, at a 1024 x 1024 x 5 s latent (31, 128, 128, 16) sampled as windows of 512 x 768 = (31, 64, 96)
overlapping by a quarter of the window: 3 x 2 = 6 windows.  Synthetic weights (2B Lite, random-init, full depth by default), guidance 5.

1. The two new passes alone, events around `--reps` launches after a warm-up, next to the existing entries on the same data in this process:
   - k5_cfg_euler_tiles over the whole latent, next to k5_cfg_euler_windows over the same latent (31 frames as 2 windows of 16 frames).
     Traffic, stated per pass: the fp32 latent read and written once, every bf16 velocity slot (cond and uncond) read once.
   - k5_patchify_view_bf16 of the window at (0, 32, 32) with its conditioning view, next to k5_patchify_cond_bf16 on a contiguous copy.
     Traffic: the window's fp32 latent and conditioning cells read once, the bf16 [Ntok][Kpad] rows written once.
2. One tiled step: ms per step of k5_sample_tiles against nwin times the ms per step of plain k5_sample at the window's shape, and (unless
   `--no_whole`) one plain run over the whole large frame, which the tiled run replaces.  The legs alternate in one process, `--rounds` times;
   medians are reported, every series is kept.

One JSON line, appended to profiles/tile_bench.jsonl.

    python tools/tile_bench.py [--steps 2] [--rounds 5] [--blocks 32] [--reps 20] [--no_whole]
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
CLIP, WINDOW, C = (31, 128, 128), (31, 64, 96), 16


def event_us(fn, reps):
    """median microseconds of one call of fn, events around each of `reps` calls after two warm-up calls"""
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def passes(dev, plan, reps):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import context_windows
    L = E.lib()
    g = torch.Generator().manual_seed(2)
    img = torch.randn(*CLIP, C, generator=g).to(dev)
    vc = torch.randn(plan.nwin, *WINDOW, C, generator=g).to(dev).to(torch.bfloat16)
    vu = torch.randn(plan.nwin, *WINDOW, C, generator=g).to(dev).to(torch.bfloat16)
    tabs = E.tile_tables(plan, dev)
    out = {}
    tile_bytes = 2 * 4 * img.numel() + 2 * 2 * vc.numel()
    us = event_us(lambda: E.cfg_euler_tiles_(img, vc, vu, 5.0, -1e-3, tabs), reps)
    out["cfg_euler_tiles"] = {"us": round(us, 2), "bytes": tile_bytes, "TBps": round(tile_bytes / us / 1e6, 3)}
    starts, weights = context_windows(CLIP[0], 16, 1)
    st, wt = E.window_tables(starts, weights, dev)
    frame = CLIP[1] * CLIP[2] * C
    wc = torch.randn(len(starts), 16, frame, generator=g).to(dev).to(torch.bfloat16)
    wu = torch.randn(len(starts), 16, frame, generator=g).to(dev).to(torch.bfloat16)
    win_bytes = 2 * 4 * img.numel() + 2 * 2 * wc.numel()
    us = event_us(lambda: E.cfg_euler_windows_(img, wc, wu, 5.0, -1e-3, st, wt), reps)
    out["cfg_euler_windows"] = {"us": round(us, 2), "bytes": win_bytes, "TBps": round(win_bytes / us / 1e6, 3), "nwin": len(starts), "frames": 16}
    cond = torch.randn(*CLIP, C + 1, generator=g).to(dev)
    box = (slice(0, WINDOW[0]), slice(32, 32 + WINDOW[1]), slice(32, 32 + WINDOW[2]))
    Cin, ntok = 2 * C + 1, WINDOW[0] * (WINDOW[1] // 2) * (WINDOW[2] // 2)
    Kpad = (4 * Cin + 7) // 8 * 8
    rows = torch.empty(ntok, Kpad, dtype=torch.bfloat16, device=dev)
    xv, cv = img[box], cond[box]
    xc, cc = xv.contiguous(), cv.contiguous()
    patch_bytes = 4 * (xc.numel() + cc.numel()) + 2 * rows.numel()
    us = event_us(lambda: E.patchify_view_(xv, cv, Cin, Kpad, out=rows), reps)
    out["patchify_view"] = {"us": round(us, 2), "bytes": patch_bytes, "TBps": round(patch_bytes / us / 1e6, 3)}
    s = E.stream_ptr(dev)
    us = event_us(lambda: E.check(L.k5_patchify_cond_bf16(xc.data_ptr(), cc.data_ptr(), rows.data_ptr(), *WINDOW, C, Cin, Kpad, None, s),
                                  "k5_patchify_cond_bf16"), reps)
    out["patchify_cond_compact"] = {"us": round(us, 2), "bytes": patch_bytes, "TBps": round(patch_bytes / us / 1e6, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2, help="Euler steps per leg")
    ap.add_argument("--rounds", type=int, default=5, help="alternations (each runs every leg)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--reps", type=int, default=20, help="timed launches of each pass")
    ap.add_argument("--no_whole", action="store_true", help="skip the plain run over the whole large frame")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_bench.jsonl"))
    args = ap.parse_args()
    from kandinsky.generation_utils import sigma_schedule, tile_windows
    from kandinsky.models.dit import DiffusionTransformer3D

    dev = torch.device("cuda", 0)
    plan = tile_windows(CLIP, WINDOW, (0, WINDOW[1] // 4, WINDOW[2] // 4))
    line = {"clip": list(CLIP), "window": list(WINDOW), "overlap": list(plan.overlap), "counts": list(plan.counts), "nwin": plan.nwin,
            "starts": [list(s) for s in plan.starts], "reps": args.reps, "passes": passes(dev, plan, args.reps)}
    with torch.device("meta"):
        dit = DiffusionTransformer3D(**dict(LITE, num_visual_blocks=args.blocks))
    dit.init_synthetic(dev, seed=0)
    g = torch.Generator().manual_seed(1)
    te = {"text_embeds": torch.randn(64, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
    ne = {"text_embeds": torch.randn(32, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
    sig = sigma_schedule(50, 5.0).tolist()[:args.steps + 1]
    noise = torch.randn(*CLIP, C, generator=g).to(dev)
    pos_of = lambda shape: [torch.arange(shape[0]), torch.arange(shape[1] // 2), torch.arange(shape[2] // 2)]   # noqa: E731
    w = 5.0

    def leg(kind):
        lat = noise.clone() if kind != "window" else noise[:WINDOW[0], :WINDOW[1], :WINDOW[2]].contiguous()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dit.sample(lat, sig, te, ne, pos_of(CLIP if kind == "whole" else WINDOW), torch.arange(64), torch.arange(32), w, scale_factor=(1.0, 2.0, 2.0),
                   tiles=plan if kind == "tiled" else None)
        torch.cuda.synchronize(dev)
        assert torch.isfinite(lat).all()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    kinds = ["window", "tiled"] + ([] if args.no_whole else ["whole"])
    for k in kinds:   # warm-up: workspaces, RoPE tables
        leg(k)
    series = {k: [] for k in kinds}
    for r in range(args.rounds):
        for k in (kinds if r % 2 == 0 else kinds[::-1]):
            series[k].append(leg(k))
    med = {k: statistics.median(v) for k, v in series.items()}
    line.update({"guidance": w, "steps": args.steps, "blocks": args.blocks, "rounds": args.rounds,
                 "ms_per_step_k5_sample_tiles": round(med["tiled"], 3), "ms_per_step_k5_sample_window_shape": round(med["window"], 3),
                 "ms_per_step_nwin_times_plain": round(plan.nwin * med["window"], 3),
                 "overhead_ms_per_step": round(med["tiled"] - plan.nwin * med["window"], 3),
                 "overhead_pct": round(100.0 * (med["tiled"] - plan.nwin * med["window"]) / (plan.nwin * med["window"]), 3),
                 "ms_per_step_whole_frame": round(med["whole"], 3) if "whole" in med else None,
                 "series": {k: [round(v, 3) for v in vals] for k, vals in series.items()},
                 "spread": {k: round(max(vals) - min(vals), 3) for k, vals in series.items()}})
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
