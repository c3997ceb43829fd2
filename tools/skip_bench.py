"""What skip-layer guidance costs: ms per step of DiffusionTransformer3D.sample on the 5 s clip's latent (31, 64, 96) with synthetic weights
(2B Lite, random-init, full depth by default), guidance 5 and guidance 1, each with three legs:

    off               no skip set
    slg               skip-layer guidance on blocks {9, 10} (mode "block") on every step: the conditional forward forks at block 9
    slg_noshare       the same with "skip_share_prefix" = 0: the skip branch runs every non-skipped block from the visual embedding on

The legs alternate (the order flips every round), `--rounds` times; a leg's wall time is taken between two device synchronisations and
divided by the steps.  The three-velocity update is also timed on its own with events over `--kernel_iters` launches at the clip's size, next
to k5_cfg_euler.  Estimate: a skip step costs one more forward minus k0 / num_visual_blocks of its visual blocks (k0 = the first skipped
block), plus one copy of the visual stream each way (n x D bf16; 171 MB at the 5 s clip, about 65 us at `--bandwidth` TB/s, default the
figure DESIGN.md §4 gives for `ln_kernel`).  One JSON line, appended to profiles/skip_bench.jsonl.

    python tools/skip_bench.py [--steps 4] [--rounds 2] [--blocks 32] [--skip 9 10] [--kernel_iters 50] [--bandwidth 5.3]
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
LEGS = ("off", "slg", "slg_noshare")
G = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4, help="Euler steps per leg")
    ap.add_argument("--rounds", type=int, default=2, help="rotations (each runs every leg at both guidance weights)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--skip", type=int, nargs="+", default=(9, 10), help="the skipped visual blocks")
    ap.add_argument("--kernel_iters", type=int, default=50, help="launches per kernel timing")
    ap.add_argument("--bandwidth", type=float, default=5.3, help="TB/s the estimate is computed at")
    ap.add_argument("--shape", type=int, nargs=3, default=(31, 64, 96), metavar=("T", "H", "W"), help="latent shape (default: the 5 s clip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skip_bench.jsonl"))
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
    T, H, Wd = args.shape
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(Wd // 2)]
    noise = torch.randn(T, H, Wd, 16, generator=g).to(dev)
    n = noise.numel()
    skip, k0 = sorted(args.skip), min(args.skip)
    ran = sum(1 for b in range(k0, args.blocks) if b not in skip)          # blocks a sharing skip branch runs itself (mode "block")
    want = {"off": (0, 0, 0), "slg": (args.steps, args.steps * k0, args.steps * ran),
            "slg_noshare": (args.steps, 0, args.steps * (args.blocks - len(skip)))}

    def leg(name, w):
        dit.set_option("skip_share_prefix", 0 if name == "slg_noshare" else 1)
        if name == "off":
            dit.clear_skip_guidance()
        else:
            dit.set_skip_guidance(skip, G)
        dit.skip_state(reset=True)
        lat = noise.clone()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), w, scale_factor=(1.0, 2.0, 2.0))
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        counts = dit.skip_state()[1:]
        dit.clear_skip_guidance()
        dit.set_option("skip_share_prefix", 1)
        assert counts == want[name], (name, counts, want[name])
        return ms, lat

    weights = (5.0, 1.0)
    leg("slg", 5.0)   # warm-up: workspaces, RoPE tables, both text streams, the fork's buffers
    series = {(k, w): [] for k in LEGS for w in weights}
    final = {}
    for r in range(args.rounds):
        for w in weights:
            for name in (LEGS if r % 2 == 0 else LEGS[::-1]):
                ms, lat = leg(name, w)
                series[(name, w)].append(ms)
                final[(name, w)] = lat
    for w in weights:
        assert torch.isfinite(final[("slg", w)]).all() and not torch.equal(final[("slg", w)], final[("off", w)]), "skip guidance left the run as it was"

    L, st = E.lib(), E.stream_ptr(dev)
    c, u, s = (torch.randn(n, generator=g).to(dev).bfloat16() for _ in range(3))
    img = torch.randn(n, generator=g).to(dev)

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
        "skip_euler_cfg": kernel_us(lambda: L.k5_skip_euler(img.data_ptr(), c.data_ptr(), u.data_ptr(), s.data_ptr(), 5.0, None, G, -1e-3, None, None,
                                                            None, 0.5, n // 16, 16, None, st)),
        "skip_euler_nocfg": kernel_us(lambda: L.k5_skip_euler(img.data_ptr(), c.data_ptr(), None, s.data_ptr(), 1.0, None, G, -1e-3, None, None,
                                                              None, 0.5, n // 16, 16, None, st)),
        "cfg_euler": kernel_us(lambda: L.k5_cfg_euler(img.data_ptr(), c.data_ptr(), u.data_ptr(), 5.0, -1e-3, n, st)),
        "cfg_euler_nocfg": kernel_us(lambda: L.k5_cfg_euler(img.data_ptr(), c.data_ptr(), None, 1.0, -1e-3, n, st)),
    }
    med = {k: statistics.median(v) for k, v in series.items()}
    tokens = T * (H // 2) * (Wd // 2)
    copy_mb = tokens * LITE["model_dim"] * 2 / 1e6

    def key(name, w):
        return f"{name}_w{w:g}"

    line = {"latent": [T, H, Wd], "elements": n, "steps": args.steps, "blocks": args.blocks, "skip": skip, "scale": G, "rounds": args.rounds,
            "bandwidth_TBps": args.bandwidth,
            "ms_per_step": {key(k, w): round(med[(k, w)], 3) for w in weights for k in LEGS},
            "series": {key(k, w): [round(v, 3) for v in series[(k, w)]] for w in weights for k in LEGS},
            "spread": {key(k, w): round(max(series[(k, w)]) - min(series[(k, w)]), 3) for w in weights for k in LEGS},
            "extra_ms_per_step": {key(k, w): round(med[(k, w)] - med[("off", w)], 3) for w in weights for k in LEGS[1:]},
            "extra_percent": {key(k, w): round(100 * (med[(k, w)] - med[("off", w)]) / med[("off", w)], 3) for w in weights for k in LEGS[1:]},
            # one forward = the off leg at guidance 1; the design figure for the sharing branch: (1 - k0 / blocks) of a forward's visual blocks
            "expected_extra_ms_by_design": round(med[("off", 1.0)] * (1.0 - k0 / args.blocks), 3),
            "us_kernels": kernel, "fork_copy_MB_each_way": round(copy_mb, 2),
            "expected_us_per_copy_by_traffic": round(2 * copy_mb * 1e6 / (args.bandwidth * 1e12) * 1e6, 2)}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
