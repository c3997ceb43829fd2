"""What the sampler's guidance controls cost: ms per step of DiffusionTransformer3D.sample at guidance 5 on the 5 s clip's latent (31, 64, 96)
with synthetic weights (2B Lite, random-init, full depth by default), four legs:

    plain             no plan
    weights           a per-step weight table (k5_cfg_euler with w_i: the launches of the plain run)
    zero_star_rescale CFG-Zero* + CFG rescale: k5_guidance_coeffs_bf16 + k5_guided_euler on every step
    interval_half     a guidance interval that covers half the steps: the other half runs one forward

The legs alternate (the order flips every round), `--rounds` times; a leg's wall time is taken between two device synchronisations and
divided by the steps.  The two statistics launches and the guided update are also timed on their own with events over `--kernel_iters`
launches at the clip's size, next to k5_cfg_euler.  Estimate by traffic: the statistics pass reads the two bf16 velocities once, 4 bytes per
latent element, at `--bandwidth` TB/s (default the figure DESIGN.md §4 gives for `ln_kernel`) — expect launch cost, not bandwidth.  One JSON
line, appended to profiles/guidance_bench.jsonl.

    python tools/guidance_bench.py [--steps 4] [--rounds 2] [--blocks 32] [--kernel_iters 50] [--bandwidth 5.3]
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
LEGS = ("plain", "weights", "zero_star_rescale", "interval_half")
W = 5.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4, help="Euler steps per leg (even: the interval leg guides half of them)")
    ap.add_argument("--rounds", type=int, default=2, help="rotations (each runs every leg)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--kernel_iters", type=int, default=50, help="launches per kernel timing")
    ap.add_argument("--bandwidth", type=float, default=5.3, help="TB/s the estimate is computed at")
    ap.add_argument("--shape", type=int, nargs=3, default=(31, 64, 96), metavar=("T", "H", "W"), help="latent shape (default: the 5 s clip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_bench.jsonl"))
    args = ap.parse_args()
    if args.steps < 2 or args.steps % 2:
        ap.error("--steps must be even and >= 2")
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
    T, H, Wd = args.shape
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(Wd // 2)]
    noise = torch.randn(T, H, Wd, 16, generator=g).to(dev)
    n = noise.numel()
    half = args.steps // 2
    plans = {"plain": None,
             "weights": dict(weights=[W - 0.25 * i for i in range(args.steps)]),
             "zero_star_rescale": dict(zero_star=True, rescale=0.7),
             "interval_half": dict(weights=[1.0] * (args.steps - half) + [W] * half)}
    want = {"plain": (0, 0, 0), "weights": (args.steps, 0, 0), "zero_star_rescale": (args.steps, 0, 0), "interval_half": (half, args.steps - half, 0)}

    def leg(name):
        if plans[name] is None:
            dit.clear_guidance()
        else:
            dit.set_guidance(**plans[name])
        dit.guidance_state(reset=True)
        lat = noise.clone()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), W, scale_factor=(1.0, 2.0, 2.0))
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        counts = dit.guidance_state()[1:]
        dit.clear_guidance()
        assert counts == want[name], (name, counts)
        return ms, lat

    leg("zero_star_rescale")   # warm-up: workspaces, RoPE tables, both text streams, the statistics scratch
    series = {k: [] for k in LEGS}
    final = {}
    for r in range(args.rounds):
        for name in (LEGS if r % 2 == 0 else LEGS[::-1]):
            ms, lat = leg(name)
            series[name].append(ms)
            final[name] = lat
    for name in LEGS[1:]:
        assert torch.isfinite(final[name]).all() and not torch.equal(final[name], final["plain"]), f"{name} left the run as it was"

    L, st = E.lib(), E.stream_ptr(dev)
    c, u = (torch.randn(n, generator=g).to(dev).bfloat16() for _ in range(2))
    img = torch.randn(n, generator=g).to(dev)
    part = torch.empty(L.k5_guidance_stats_blocks(n) * 5, dtype=torch.float64, device=dev)
    sums, ab = torch.empty(5, dtype=torch.float64, device=dev), torch.empty(2, dtype=torch.float32, device=dev)

    def kernel_us(fn):
        fn()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.kernel_iters):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return round(a.elapsed_time(b) * 1e3 / args.kernel_iters, 2)

    kernel = {
        "coeffs_two_launches": kernel_us(lambda: L.k5_guidance_coeffs_bf16(c.data_ptr(), u.data_ptr(), n, W, 1, 0.7, part.data_ptr(), sums.data_ptr(),
                                                                           ab.data_ptr(), st)),
        "guided_euler": kernel_us(lambda: L.k5_guided_euler(img.data_ptr(), c.data_ptr(), u.data_ptr(), ab.data_ptr(), -1e-3, None, None, None, 0.5,
                                                            n // 16, 16, None, st)),
        "cfg_euler": kernel_us(lambda: L.k5_cfg_euler(img.data_ptr(), c.data_ptr(), u.data_ptr(), W, -1e-3, n, st)),
    }
    med = {k: statistics.median(v) for k, v in series.items()}
    line = {"latent": [T, H, Wd], "elements": n, "guidance": W, "steps": args.steps, "blocks": args.blocks, "rounds": args.rounds,
            "bandwidth_TBps": args.bandwidth,
            "ms_per_step": {k: round(med[k], 3) for k in LEGS},
            "series": {k: [round(v, 3) for v in series[k]] for k in LEGS},
            "spread": {k: round(max(series[k]) - min(series[k]), 3) for k in LEGS},
            "extra_ms_per_step": {k: round(med[k] - med["plain"], 3) for k in LEGS[1:]},
            "extra_percent": {k: round(100 * (med[k] - med["plain"]) / med["plain"], 3) for k in LEGS[1:]},
            "us_kernels": kernel, "stats_read_MB": round(n * 4 / 1e6, 2), "expected_us_stats_by_traffic": round(n * 4 / (args.bandwidth * 1e12) * 1e6, 2)}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
