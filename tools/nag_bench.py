"""What normalized attention guidance (NAG) costs: ms per step of DiffusionTransformer3D.sample at guidance 1 with NAG off and on, on the
5 s clip's latent (31, 64, 96) with synthetic weights (2B Lite, random-init, full depth by default), next to the estimate by traffic.

The two legs alternate (the order flips every round), `--rounds` times; a leg's wall time is taken between two device synchronisations and
divided by the steps.  After that each leg runs once more with the engine's profiling on (events around every kernel family): the deltas of
`attn_cross` (the second cross-attention launch of every block) and `elementwise` (the combine) per step are reported.  The combine kernel is
also timed on its own with events over `--kernel_iters` launches at the clip's [tokens][1792].  Estimate: the combine reads z+ and z- and
writes the result, 3 x tokens x 1792 x 2 bytes per block, at `--bandwidth` TB/s (default the figure DESIGN.md §4 gives for `ln_kernel`).
One JSON line, appended to profiles/nag_bench.jsonl.

    python tools/nag_bench.py [--steps 4] [--rounds 3] [--blocks 32] [--kernel_iters 100] [--bandwidth 5.3]
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
FAMILIES = ("attn_cross", "elementwise", "gemm", "attn_text", "prologue")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4, help="Euler steps per leg")
    ap.add_argument("--rounds", type=int, default=3, help="rotations (each runs both legs)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--kernel_iters", type=int, default=100, help="launches per kernel timing")
    ap.add_argument("--bandwidth", type=float, default=5.3, help="TB/s the estimate is computed at")
    ap.add_argument("--shape", type=int, nargs=3, default=(31, 64, 96), metavar=("T", "H", "W"), help="latent shape (default: the 5 s clip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nag_bench.jsonl"))
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
    tokens, D = T * (H // 2) * (W // 2), LITE["model_dim"]
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    noise = torch.randn(T, H, W, 16, generator=g).to(dev)
    params = (5.0, 2.5, 0.25)

    def leg(kind, profile=False):
        if kind == "on":
            dit.set_nag(ne, torch.arange(32), *params)
        else:
            dit.clear_nag()
        dit.nag_state(reset=True)
        lat = noise.clone()
        if profile:
            dit.set_profiling(True)
            dit.reset_profile()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), 1.0, scale_factor=(1.0, 2.0, 2.0))
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        prof = None
        if profile:
            prof = {f: dit.get_profile(f)[0] / args.steps for f in FAMILIES}
            dit.set_profiling(False)
        combines = dit.nag_state()[1]
        dit.clear_nag()
        assert combines == (args.steps * args.blocks if kind == "on" else 0), (kind, combines)
        return ms, lat, prof

    leg("on")   # warm-up: workspaces, RoPE tables, the negative stream's buffers
    series = {k: [] for k in LEGS}
    final = {}
    for r in range(args.rounds):
        for kind in (LEGS if r % 2 == 0 else LEGS[::-1]):
            ms, lat, _ = leg(kind)
            series[kind].append(ms)
            final[kind] = lat
    assert torch.isfinite(final["on"]).all() and not torch.equal(final["on"], final["off"]), "NAG left the latent as it was"
    prof = {k: leg(k, profile=True)[2] for k in LEGS}

    zp = torch.randn(tokens, D, generator=g).to(dev).bfloat16()
    zn = torch.randn(tokens, D, generator=g).to(dev).bfloat16()
    out = torch.empty_like(zp)
    L, st = E.lib(), E.stream_ptr(dev)

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

    us = kernel_us(lambda: L.k5_nag_combine_bf16(zp.data_ptr(), zn.data_ptr(), out.data_ptr(), tokens, D, D, *params, st))
    us_in_place = kernel_us(lambda: L.k5_nag_combine_bf16(zp.data_ptr(), zn.data_ptr(), zp.data_ptr(), tokens, D, D, *params, st))
    traffic = 3 * tokens * D * 2
    med = {k: statistics.median(v) for k, v in series.items()}
    line = {"latent": [T, H, W], "tokens": tokens, "guidance": 1.0, "nag": list(params), "steps": args.steps, "blocks": args.blocks,
            "rounds": args.rounds, "bandwidth_TBps": args.bandwidth,
            "ms_per_step": {k: round(med[k], 3) for k in LEGS},
            "series": {k: [round(v, 3) for v in series[k]] for k in LEGS},
            "spread": {k: round(max(series[k]) - min(series[k]), 3) for k in LEGS},
            "extra_ms_per_step": round(med["on"] - med["off"], 3), "extra_percent": round(100 * (med["on"] - med["off"]) / med["off"], 3),
            "profiled_ms_per_step": {k: {f: round(v, 3) for f, v in prof[k].items()} for k in LEGS},
            "profiled_delta_ms_per_step": {f: round(prof["on"][f] - prof["off"][f], 3) for f in FAMILIES},
            "us_combine": round(us, 2), "us_combine_in_place": round(us_in_place, 2), "combine_TBps": round(traffic / us / 1e6, 3),
            "traffic_MB_per_block": round(traffic / 1e6, 2), "expected_us_combine": round(traffic / (args.bandwidth * 1e12) * 1e6, 2),
            "expected_ms_per_step_combines": round(args.blocks * traffic / (args.bandwidth * 1e12) * 1e3, 3)}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
