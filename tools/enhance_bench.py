"""What Enhance-A-Video costs: ms per step of DiffusionTransformer3D.sample with it off and on (weight 4, every step) at guidance 1 and 5, on the
5 s clip's latent (31, 64, 96) with synthetic weights (2B Lite, random-init, full depth by default), next to the estimate by traffic.

Per guidance the two legs alternate in one process (the order flips every round), `--rounds` times; a leg's wall time is taken between two
device synchronisations and divided by the steps; the medians are reported with every series.  The "off" leg is the parent commit's step:
with the feature off a run enqueues what it always did.  The two kernels are also timed on their own with events over `--kernel_iters`
launches at the clip's shapes: the score on a fused [tokens][2 x 1792] q | k buffer (one read of it: 341 MB) and the in-place scale of
[tokens][1792] (171 MB read + written), each against `--bandwidth` TB/s (default the figure DESIGN.md §4 gives for `ln_kernel`).
One JSON line, appended to profiles/enhance_bench.jsonl.

    python tools/enhance_bench.py [--steps 3] [--rounds 5] [--blocks 32] [--kernel_iters 50] [--bandwidth 5.3]
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
LEGS = ("off", "on")
WEIGHT = 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="Euler steps per leg")
    ap.add_argument("--rounds", type=int, default=5, help="rotations (each runs both legs)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--kernel_iters", type=int, default=50, help="launches per kernel timing")
    ap.add_argument("--bandwidth", type=float, default=5.3, help="TB/s the estimate is computed at")
    ap.add_argument("--shape", type=int, nargs=3, default=(31, 64, 96), metavar=("T", "H", "W"), help="latent shape (default: the 5 s clip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enhance_bench.jsonl"))
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
    T, H, W = args.shape
    S = (H // 2) * (W // 2)
    tokens, D, Hh = T * S, LITE["model_dim"], LITE["model_dim"] // 64
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    noise = torch.randn(T, H, W, 16, generator=g).to(dev)

    def leg(kind, w):
        if kind == "on":
            dit.set_enhance(WEIGHT)
        else:
            dit.clear_enhance()
        dit.enhance_state(reset=True)
        lat = noise.clone()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), w, scale_factor=(1.0, 2.0, 2.0))
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        _, launches, scores = dit.enhance_state()
        used = dit.get_option("attn_fuse_qnorm_used")
        dit.clear_enhance()
        forwards = 2 if w != 1.0 else 1
        assert launches == (args.steps * forwards * args.blocks if kind == "on" else 0), (kind, launches)
        return ms, lat, scores, used

    result = {}
    for w in (1.0, 5.0):
        leg("on", w)   # warm-up: workspaces, RoPE tables
        series = {k: [] for k in LEGS}
        final, scores, used = {}, [], {}
        for r in range(args.rounds):
            for kind in (LEGS if r % 2 == 0 else LEGS[::-1]):
                ms, lat, sc, u = leg(kind, w)
                series[kind].append(ms)
                final[kind], used[kind] = lat, u
                if kind == "on":
                    scores = sc
        assert torch.isfinite(final["on"]).all(), "the enhanced run is not finite"
        med = {k: statistics.median(v) for k, v in series.items()}
        result[f"guidance_{w:g}"] = {
            "ms_per_step": {k: round(med[k], 3) for k in LEGS}, "series": {k: [round(v, 3) for v in series[k]] for k in LEGS},
            "spread": {k: round(max(series[k]) - min(series[k]), 3) for k in LEGS},
            "extra_ms_per_step": round(med["on"] - med["off"], 3), "extra_percent": round(100 * (med["on"] - med["off"]) / med["off"], 3),
            "attn_fuse_qnorm_used": used, "latent_changed": not torch.equal(final["on"], final["off"]),
            "last_forward_scores_min_max": [round(min(scores), 4), round(max(scores), 4)] if scores else None}

    qk = torch.randn(tokens, 2 * D, generator=g).to(dev).bfloat16()
    o = torch.randn(tokens, D, generator=g).to(dev).bfloat16()
    part = torch.zeros(S * Hh, dtype=torch.float64, device=dev)
    score = torch.zeros(1, dtype=torch.float32, device=dev)
    near_one = torch.full((1,), 1.0009765625, dtype=torch.float32, device=dev)   # not 1: the scale really runs; close to 1: o stays finite over the launches
    one = torch.ones(1, dtype=torch.float32, device=dev)
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

    us_score = kernel_us(lambda: L.k5_enhance_scores_bf16(qk.data_ptr(), qk.data_ptr() + 2 * D, 2 * D, 2 * D, Hh, T, S, None, 1.0, WEIGHT,
                                                          part.data_ptr(), score.data_ptr(), st))
    us_scale = kernel_us(lambda: L.k5_scale_by_dev_bf16(o.data_ptr(), tokens, D, D, near_one.data_ptr(), st))
    us_scale_clamped = kernel_us(lambda: L.k5_scale_by_dev_bf16(o.data_ptr(), tokens, D, D, one.data_ptr(), st))
    read_qk, rw_o = tokens * 2 * D * 2, 2 * tokens * D * 2
    line = {"latent": [T, H, W], "tokens": tokens, "weight": WEIGHT, "steps": args.steps, "blocks": args.blocks, "rounds": args.rounds,
            "bandwidth_TBps": args.bandwidth, **result,
            "us_scores": round(us_score, 2), "scores_TBps": round(read_qk / us_score / 1e6, 3), "scores_read_MB": round(read_qk / 1e6, 1),
            "expected_us_scores": round(read_qk / (args.bandwidth * 1e12) * 1e6, 2),
            "us_scale": round(us_scale, 2), "scale_TBps": round(rw_o / us_scale / 1e6, 3), "scale_read_write_MB": round(rw_o / 1e6, 1),
            "expected_us_scale": round(rw_o / (args.bandwidth * 1e12) * 1e6, 2), "us_scale_clamped": round(us_scale_clamped, 2),
            "expected_ms_per_forward": round(args.blocks * (read_qk + rw_o) / (args.bandwidth * 1e12) * 1e3, 3)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
