"""What the forecast cache saves: ms per step of DiffusionTransformer3D.sample on the 5 s clip's latent (31, 64, 96) with synthetic weights (2B
Lite, random-init, full depth by default) at guidance 1 and 5 — plain, and with the plan of `generation_utils.forecast_plan(steps, interval,
warmup, tail)` at interval 2 and 3, orders 1 and 2 — next to the two passes' own time against their traffic, and the bytes the history holds.

Per guidance the five legs alternate in one process (the order flips every round), `--rounds` times; a leg's wall time is taken between two
device synchronisations and divided by the steps; the medians are reported with every series.  The "plain" leg is the parent commit's step: with
the feature off a run enqueues what it always did.  A leg's share of full steps is reported with it: the saving cannot exceed the skipped share.
The two kernels are timed with events over `--kernel_iters` launches at the clip's [tokens][1792]: update at order 2 (reads vis, ori, F0, D1 and
writes F0, D1, D2: 20 bytes per element) and apply at order 2 (reads vis, F0, D1, D2, writes vis: 14), each against `--bandwidth` TB/s (default
the figure DESIGN.md quotes for `ln_kernel`).  On random weights the outputs say nothing about quality; only time and memory are reported.
One JSON line, appended to profiles/forecast_bench.jsonl.

    python tools/forecast_bench.py [--steps 10] [--warmup 3] [--tail 1] [--rounds 5] [--blocks 32] [--kernel_iters 50] [--bandwidth 5.3]
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
LEGS = {"plain": None, "interval2_order1": (2, 1), "interval2_order2": (2, 2), "interval3_order1": (3, 1), "interval3_order2": (3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="Euler steps per leg")
    ap.add_argument("--warmup", type=int, default=3, help="full steps at the start of every plan")
    ap.add_argument("--tail", type=int, default=1, help="full steps at the end of every plan")
    ap.add_argument("--rounds", type=int, default=5, help="rotations (each runs every leg)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--kernel_iters", type=int, default=50, help="launches per kernel timing")
    ap.add_argument("--bandwidth", type=float, default=5.3, help="TB/s the estimate is computed at")
    ap.add_argument("--shape", type=int, nargs=3, default=(31, 64, 96), metavar=("T", "H", "W"), help="latent shape (default: the 5 s clip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forecast_bench.jsonl"))
    args = ap.parse_args()
    from kandinsky import _engine as E
    from kandinsky.generation_utils import forecast_plan, sigma_schedule
    from kandinsky.models.dit import DiffusionTransformer3D

    dev = torch.device("cuda", 0)
    with torch.device("meta"):
        dit = DiffusionTransformer3D(**dict(LITE, num_visual_blocks=args.blocks))
    dit.init_synthetic(dev, seed=0)
    g = torch.Generator().manual_seed(1)
    te = {"text_embeds": torch.randn(64, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
    ne = {"text_embeds": torch.randn(32, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
    sig = sigma_schedule(50, 5.0).tolist()[:args.steps + 1]
    T, H, W = args.shape
    tokens, D = T * (H // 2) * (W // 2), LITE["model_dim"]
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    noise = torch.randn(T, H, W, 16, generator=g).to(dev)
    plans = {k: None if v is None else (v[1], forecast_plan(args.steps, v[0], args.warmup, args.tail, v[1])) for k, v in LEGS.items()}

    def leg(kind, w):
        plan = plans[kind]
        if plan is not None:
            dit.set_forecast(*plan)
        dit.forecast_state(reset=True)
        lat = noise.clone()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), w, scale_factor=(1.0, 2.0, 2.0))
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        _, full, fore, nbytes = dit.forecast_state()
        dit.clear_forecast()
        forwards = 2 if w != 1.0 else 1
        want = (0, 0) if plan is None else (forwards * sum(plan[1]), forwards * (args.steps - sum(plan[1])))
        assert (full, fore) == want, (kind, full, fore, want)
        return ms, lat, nbytes

    result = {}
    for w in (1.0, 5.0):
        leg("interval2_order2", w)   # warm-up: workspaces, RoPE tables
        series = {k: [] for k in LEGS}
        final, nbytes = {}, {}
        for r in range(args.rounds):
            for kind in (list(LEGS) if r % 2 == 0 else list(LEGS)[::-1]):
                ms, lat, nb = leg(kind, w)
                series[kind].append(ms)
                final[kind], nbytes[kind] = lat, nb
        med = {k: statistics.median(v) for k, v in series.items()}
        assert all(torch.isfinite(v).all() for v in final.values()), "a forecast run is not finite"
        result[f"guidance_{w:g}"] = {
            "ms_per_step": {k: round(med[k], 3) for k in LEGS}, "series": {k: [round(v, 3) for v in series[k]] for k in LEGS},
            "spread": {k: round(max(series[k]) - min(series[k]), 3) for k in LEGS},
            "saved_percent": {k: round(100 * (med["plain"] - med[k]) / med["plain"], 3) for k in LEGS if k != "plain"},
            "full_step_share": {k: round(sum(plans[k][1]) / args.steps, 3) for k in LEGS if k != "plain"},
            "state_bytes": nbytes}

    vis, ori, F0 = (torch.randn(tokens, D, generator=g).to(dev).bfloat16() for _ in range(3))
    D1, D2 = torch.randn(tokens, D, generator=g).to(dev), torch.randn(tokens, D, generator=g).to(dev)
    L, st = E.lib(), E.stream_ptr(dev)

    def kernel_us(fn):
        assert fn() == 0
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.kernel_iters):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e3 / args.kernel_iters

    us_update = kernel_us(lambda: L.k5_forecast_update_bf16(vis.data_ptr(), D, ori.data_ptr(), F0.data_ptr(), D1.data_ptr(), D2.data_ptr(), tokens, D,
                                                            3, 2, 2, st))
    for t, fill in ((F0, 0.01), (D1, 0.0), (D2, 0.0)):   # a near-zero series: vis stays finite over the launches
        t.fill_(fill)
    us_apply = kernel_us(lambda: L.k5_forecast_apply_bf16(vis.data_ptr(), D, F0.data_ptr(), D1.data_ptr(), D2.data_ptr(), tokens, D, 2, 2, 2, 2, 3, st))
    b_update, b_apply = tokens * D * 20, tokens * D * 14
    line = {"latent": [T, H, W], "tokens": tokens, "steps": args.steps, "warmup": args.warmup, "tail": args.tail, "blocks": args.blocks,
            "rounds": args.rounds, "bandwidth_TBps": args.bandwidth, "plans": {k: None if v is None else v[1] for k, v in plans.items()}, **result,
            "us_update": round(us_update, 2), "update_TBps": round(b_update / us_update / 1e6, 3), "update_MB": round(b_update / 1e6, 1),
            "expected_us_update": round(b_update / (args.bandwidth * 1e12) * 1e6, 2),
            "us_apply": round(us_apply, 2), "apply_TBps": round(b_apply / us_apply / 1e6, 3), "apply_MB": round(b_apply / 1e6, 1),
            "expected_us_apply": round(b_apply / (args.bandwidth * 1e12) * 1e6, 2),
            "expected_state_bytes_order2": {"per_slot": tokens * D * 10, "ori": tokens * D * 2}}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
