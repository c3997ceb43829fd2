"""What the sampler watch costs: ms per step of DiffusionTransformer3D.sample with no watch, with a progress-only callback and with a preview
(+ x0) on every step, at BASELINE config 1's latent (13, 32, 32) — launch-bound, where host-side work shows first — and at the 5 s clip's
(31, 64, 96), with synthetic weights (2B Lite, random-init, full depth by default) and guidance 5; plus the preview kernel on its own.

The three legs rotate (the order shifts every round), `--rounds` times; a leg's wall time is taken between two device synchronisations and
divided by the steps, so the preview leg includes its copies to the host and the callbacks.  The kernel is timed with events over
`--kernel_iters` back-to-back launches through the C entry point (a kernel of a few microseconds: the figure is bounded below by the rate at
which the host can issue launches).  Its traffic is the fp32 latent, the bf16 velocities, the RGB bytes and (with x0) one more fp32
latent; `--bandwidth` (TB/s, default the figure DESIGN.md §4 gives for `ln_kernel`) turns that into the expected time.  The final latents of
the three legs are compared bit for bit.  One JSON line, appended to profiles/watch_bench.jsonl.

    python tools/watch_bench.py [--steps 6] [--rounds 3] [--blocks 32] [--kernel_iters 200] [--bandwidth 5.3]
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
SHAPES = {"config1_2s_256": (13, 32, 32), "5s_clip": (31, 64, 96)}
LEGS = ("off", "progress", "preview")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6, help="Euler steps per leg")
    ap.add_argument("--rounds", type=int, default=3, help="rotations (each runs the three legs)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--kernel_iters", type=int, default=200, help="launches per kernel timing")
    ap.add_argument("--bandwidth", type=float, default=5.3, help="TB/s the expected figure is computed at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "watch_bench.jsonl"))
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
    sig = sigma_schedule(50, 5.0).tolist()[:args.steps + 1]
    Wf, bf = (torch.rand(16, 3, generator=g) - 0.5) * 0.5, torch.zeros(3)
    w = 5.0
    line = {"guidance": w, "steps": args.steps, "blocks": args.blocks, "rounds": args.rounds, "bandwidth_TBps": args.bandwidth, "shapes": {}}
    for name, (T, H, W) in SHAPES.items():
        pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
        noise = torch.randn(T, H, W, 16, generator=g).to(dev)
        calls = [0]

        def count(info):
            calls[0] += 1

        def leg(kind):
            if kind == "off":
                dit.clear_watch()
            elif kind == "progress":
                dit.set_watch(count)
            else:
                dit.set_watch(count, preview_every=1, rgb_factors=Wf, rgb_bias=bf, want_x0=True)
            lat = noise.clone()
            calls[0] = 0
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), w, scale_factor=(1.0, 2.0, 2.0))
            torch.cuda.synchronize(dev)
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            dit.clear_watch()
            assert calls[0] == (0 if kind == "off" else args.steps), (kind, calls[0])
            return ms, lat

        leg("preview")   # warm-up: workspaces, RoPE tables, the pinned slots
        series = {k: [] for k in LEGS}
        final = {}
        for r in range(args.rounds):
            for kind in LEGS[r % 3:] + LEGS[:r % 3]:
                ms, lat = leg(kind)
                series[kind].append(ms)
                final[kind] = lat
        assert torch.equal(final["off"], final["progress"]) and torch.equal(final["off"], final["preview"]), "the watch moved the latent"

        vc = torch.randn(T, H, W, 16, generator=g).to(dev).bfloat16()
        vu = torch.randn(T, H, W, 16, generator=g).to(dev).bfloat16()
        Wd, bd = Wf.to(dev), bf.to(dev)
        rgb = torch.empty(T, H, W, 3, dtype=torch.uint8, device=dev)
        x0 = torch.empty_like(noise)
        n = noise.numel()

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

        L, st = E.lib(), E.stream_ptr(dev)
        raw = [noise.data_ptr(), vc.data_ptr(), vu.data_ptr(), w, 0.5, None, None, Wd.data_ptr(), bd.data_ptr()]
        us_rgb = kernel_us(lambda: L.k5_x0_preview(*raw, None, rgb.data_ptr(), n // 16, 16, st))
        us_both = kernel_us(lambda: L.k5_x0_preview(*raw, x0.data_ptr(), rgb.data_ptr(), n // 16, 16, st))
        bytes_rgb = 4 * n + 2 * 2 * n + 3 * (n // 16)
        med = {k: statistics.median(v) for k, v in series.items()}
        line["shapes"][name] = {
            "latent": [T, H, W], "tokens": T * (H // 2) * (W // 2),
            "ms_per_step": {k: round(med[k], 3) for k in LEGS},
            "series": {k: [round(v, 3) for v in series[k]] for k in LEGS},
            "spread": {k: round(max(series[k]) - min(series[k]), 3) for k in LEGS},
            "extra_ms_per_step_progress": round(med["progress"] - med["off"], 3),
            "extra_ms_per_step_preview": round(med["preview"] - med["off"], 3),
            "us_x0_preview_rgb": round(us_rgb, 2), "us_x0_preview_rgb_x0": round(us_both, 2),
            "traffic_MB_rgb": round(bytes_rgb / 1e6, 2), "traffic_MB_rgb_x0": round((bytes_rgb + 4 * n) / 1e6, 2),
            "expected_us_rgb": round(bytes_rgb / (args.bandwidth * 1e12) * 1e6, 2),
            "expected_us_rgb_x0": round((bytes_rgb + 4 * n) / (args.bandwidth * 1e12) * 1e6, 2)}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
