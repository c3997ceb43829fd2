"""What the edit step costs: ms per step of k5_sample_edit with a keep mask against k5_sample on the same handle, and the two elementwise
kernels (k5_cfg_euler, k5_cfg_euler_edit) on their own, at the 5 s clip's latent shape (31, 64, 96) with synthetic weights (2B Lite,
random-init, full depth by default), guidance 5.

The two sampler legs alternate (which one goes first alternates too), `--rounds` times; a leg's wall time is taken between two device
synchronisations and divided by the steps.  The edit leg includes its one start pass (k5_edit_renoise).  The kernels are timed with
events over `--kernel_iters` back-to-back launches.  The extra traffic of the edit kernel is two fp32 latents and one mask value per 16
elements; `--bandwidth` (TB/s, default the figure DESIGN.md §4 gives for `ln_kernel`) turns it into the expected extra time.  One JSON
line, appended to profiles/edit_bench.jsonl.

    python tools/edit_bench.py [--steps 3] [--rounds 3] [--blocks 32] [--kernel_iters 200] [--bandwidth 5.3]
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
SHAPE = (31, 64, 96)   # config 2: the 5 s clip at 512 x 768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="Euler steps per leg")
    ap.add_argument("--rounds", type=int, default=3, help="alternations (each runs both legs)")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--kernel_iters", type=int, default=200, help="launches per kernel timing")
    ap.add_argument("--bandwidth", type=float, default=5.3, help="TB/s the expected figure is computed at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_bench.jsonl"))
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
    T, H, W = SHAPE
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    noise = torch.randn(T, H, W, 16, generator=g).to(dev)
    source = torch.randn(T, H, W, 16, generator=g).to(dev)
    mask = torch.zeros(T, H, W, 1, device=dev)
    mask[0] = 1.0
    mask[1:, :, :W // 2] = 1.0
    mask[1:, :, W // 2:W // 2 + 2] = 0.25
    w = 5.0

    def leg(edit):
        lat = noise.clone()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), w, scale_factor=(1.0, 2.0, 2.0),
                   edit=(source, noise, mask) if edit else None)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / args.steps, lat

    leg(True)   # warm-up: workspaces, RoPE tables
    plain, edited = [], []
    for r in range(args.rounds):
        for edit in ((False, True) if r % 2 == 0 else (True, False)):
            ms, lat = leg(edit)
            (edited if edit else plain).append(ms)
            if edit:   # the schedule is cut short, so the kept cells sit at the source re-noised to the last sigma
                keep = (mask == 1).expand_as(source)
                assert torch.equal(lat[keep], E.renoise(source, noise, sig[-1])[keep]), "kept cells are not the re-noised source"

    vc = torch.randn(T, H, W, 16, generator=g).to(dev).bfloat16()
    vu = torch.randn(T, H, W, 16, generator=g).to(dev).bfloat16()
    img = noise.clone()

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

    us_plain = kernel_us(lambda: E.cfg_euler_(img, vc, vu, w, -1e-3))
    us_edit = kernel_us(lambda: E.cfg_euler_edit_(img, vc, vu, w, -1e-3, source, noise, mask, 0.5))
    us_renoise = kernel_us(lambda: E.renoise(source, noise, 0.5, out=img))
    n = noise.numel()
    extra_bytes = 2 * 4 * n + 4 * (n // 16)
    line = {"latent": [T, H, W], "tokens": T * (H // 2) * (W // 2), "guidance": w, "steps": args.steps, "blocks": args.blocks,
            "rounds": args.rounds,
            "ms_per_step_k5_sample": round(statistics.median(plain), 3), "ms_per_step_k5_sample_edit": round(statistics.median(edited), 3),
            "series_k5_sample": [round(v, 3) for v in plain], "series_k5_sample_edit": [round(v, 3) for v in edited],
            "spread_k5_sample": round(max(plain) - min(plain), 3), "spread_k5_sample_edit": round(max(edited) - min(edited), 3),
            "us_cfg_euler": round(us_plain, 2), "us_cfg_euler_edit": round(us_edit, 2), "us_edit_renoise": round(us_renoise, 2),
            "extra_read_MB": round(extra_bytes / 1e6, 2), "bandwidth_TBps": args.bandwidth,
            "expected_extra_us": round(extra_bytes / (args.bandwidth * 1e12) * 1e6, 2),
            "measured_extra_us": round(us_edit - us_plain, 2)}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
