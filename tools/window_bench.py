"""What temporal context windows cost: ms per step of k5_sample_windows on a 20 s clip at 512 x 768 (121 latent frames as windows of 61
overlapping by 15: three windows) against nwin times the ms per step of plain k5_sample at the window's shape (61, 64, 96), on the same handle
in the same process, with synthetic weights (2B Lite, random-init, full depth by default), guidance 5.  The difference is what the windows
add: the blend pass over the whole clip (k5_cfg_euler_windows instead of nwin k5_cfg_euler passes) and the eager launch of every step.

The two legs alternate (which one goes first alternates too), `--rounds` times; a leg's wall time is taken between two device
synchronisations and divided by the steps.  The two elementwise passes are then read from the engine's profile (events around each
launch) in one more run of each leg.
By traffic the blend pass reads the fp32 latent once and at most `max coverage` bf16 velocity pairs per cell and writes the latent;
`--bandwidth` (TB/s, default the figure DESIGN.md §4 gives for `ln_kernel`) turns that into the expected time.  One JSON line, appended to
profiles/window_bench.jsonl.

    python tools/window_bench.py [--steps 6] [--rounds 3] [--blocks 32] [--bandwidth 5.3]
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
CLIP, WINDOW, OVERLAP, HW = 121, 61, 15, (64, 96)   # 20 s as windows of 10 s overlapping by 2.5 s, 512 x 768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6, help="Euler steps per leg")
    ap.add_argument("--rounds", type=int, default=3, help="alternations (each runs both legs)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--bandwidth", type=float, default=5.3, help="TB/s the expected figure is computed at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_bench.jsonl"))
    args = ap.parse_args()
    from kandinsky.generation_utils import context_windows, sigma_schedule
    from kandinsky.models.dit import DiffusionTransformer3D

    dev = torch.device("cuda", 0)
    with torch.device("meta"):
        dit = DiffusionTransformer3D(**dict(LITE, num_visual_blocks=args.blocks))
    dit.init_synthetic(dev, seed=0)
    g = torch.Generator().manual_seed(1)
    te = {"text_embeds": torch.randn(64, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
    ne = {"text_embeds": torch.randn(32, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
    sig = sigma_schedule(50, 5.0).tolist()[:args.steps + 1]
    H, W = HW
    pos = [torch.arange(WINDOW), torch.arange(H // 2), torch.arange(W // 2)]
    starts, weights = context_windows(CLIP, WINDOW, OVERLAP)
    nwin = len(starts)
    noise = torch.randn(CLIP, H, W, 16, generator=g).to(dev)
    w = 5.0

    def leg(windowed):
        lat = noise.clone() if windowed else noise[:WINDOW].clone()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), w, scale_factor=(1.0, 2.0, 2.0),
                   windows=(starts, weights) if windowed else None)
        torch.cuda.synchronize(dev)
        assert torch.isfinite(lat).all()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    leg(True)   # warm-up: workspaces, RoPE tables
    plain, windowed = [], []
    for r in range(args.rounds):
        for win in ((False, True) if r % 2 == 0 else (True, False)):
            (windowed if win else plain).append(leg(win))

    def kernel_us(win):   # the step's elementwise pass as the engine's own profile sees it (events around the launch), in a run of its own
        dit.set_profiling(True)
        dit.reset_profile()
        leg(win)
        ms, n = dit.get_profile("elementwise")
        dit.set_profiling(False)
        return ms * 1e3 / max(n, 1)

    us_windows, us_plain = kernel_us(True), kernel_us(False)
    frame = H * W * 16
    covered = sum(min(CLIP, s + WINDOW) - s for s in starts)               # velocity frames read: every (window, local frame) once
    blend_bytes = 2 * 4 * CLIP * frame + 2 * 2 * covered * frame
    ms_plain, ms_win = statistics.median(plain), statistics.median(windowed)
    line = {"clip": [CLIP, H, W], "window": WINDOW, "overlap": OVERLAP, "nwin": nwin, "starts": starts, "guidance": w, "steps": args.steps,
            "blocks": args.blocks, "rounds": args.rounds,
            "ms_per_step_k5_sample_windows": round(ms_win, 3), "ms_per_step_k5_sample_window_shape": round(ms_plain, 3),
            "ms_per_step_nwin_times_plain": round(nwin * ms_plain, 3), "overhead_ms_per_step": round(ms_win - nwin * ms_plain, 3),
            "overhead_pct": round(100.0 * (ms_win - nwin * ms_plain) / (nwin * ms_plain), 3),
            "series_k5_sample_windows": [round(v, 3) for v in windowed], "series_k5_sample_window_shape": [round(v, 3) for v in plain],
            "spread_k5_sample_windows": round(max(windowed) - min(windowed), 3), "spread_k5_sample_window_shape": round(max(plain) - min(plain), 3),
            "us_cfg_euler_windows": round(us_windows, 2), "us_cfg_euler_window_shape": round(us_plain, 2),
            "blend_traffic_MB": round(blend_bytes / 1e6, 2), "bandwidth_TBps": args.bandwidth,
            "expected_blend_us": round(blend_bytes / (args.bandwidth * 1e12) * 1e6, 2)}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
