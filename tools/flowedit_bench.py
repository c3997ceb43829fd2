"""What FlowEdit costs, on the 5 s clip's latent (31, 64, 96, 16) — 3.0 M elements.

Per launch (HIP events over `--kernel_iters` launches, the legs alternating, the order flipping every round, `--rounds` times, medians):

    plain             k5_euler_step's plain form (k5_cfg_euler at guidance 5): the update every run without a plan enqueues
    flowedit_both     k5_flowedit_step finishing a step and preparing the next, four velocity streams, a mask, noise from the generator
    flowedit_nocfg    the same at weights 1 / 1: two velocity streams
    flowedit_memory   flowedit_both with the noise read from an fp32 buffer
    flowedit_update   the last step's launch: no next sigma, nothing prepared
    flowedit_prepare  the first launch: no velocities

For flowedit_both the traffic is counted — reads: two fp32 latents, four bf16 velocities and the mask; writes: three fp32 latents — and
set against the time: GB/s next to the 5.3 TB/s that DESIGN.md quotes for ln_kernel.

Per step: ms per step of DiffusionTransformer3D.sample with synthetic weights (2B Lite, random-init, full depth by default): `plain` (the
parent commit's step, guidance 5: two forwards) against a FlowEdit step at guidance 1 / 1 (two forwards) and 5 / 5 (four forwards),
alternating likewise; a leg's wall time is taken between two device synchronisations and divided by the steps.  `--steps 0` leaves this
part out.  One JSON line, appended to profiles/flowedit_bench.jsonl.

    python tools/flowedit_bench.py [--steps 4] [--rounds 5] [--blocks 32] [--kernel_iters 200]
"""
import argparse
import ctypes as C
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4, help="steps per leg of the per-step part (0: leave it out)")
    ap.add_argument("--rounds", type=int, default=5, help="rotations of the legs")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--kernel_iters", type=int, default=200, help="launches per kernel timing")
    ap.add_argument("--shape", type=int, nargs=3, default=(31, 64, 96), metavar=("T", "H", "W"), help="latent shape (default: the 5 s clip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowedit_bench.jsonl"))
    args = ap.parse_args()
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    T, H, Wd = args.shape
    cells = T * H * Wd
    n = cells * 16
    L, st = E.lib(), E.stream_ptr(dev)
    cs, us, ct, ut = (torch.randn(n, generator=g).to(dev).bfloat16() for _ in range(4))
    zfe, src, z, zs, zt = (torch.randn(n, generator=g).to(dev) for _ in range(5))
    mask = (torch.rand(cells, generator=g) < 0.25).float().to(dev)
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def fe(vel=True, cfg=True, prepare=True, noise=None):
        a = E.FlowEditStep(z_fe=p(zfe), x_src=p(src), c_src=p(cs) if vel else None, u_src=p(us) if vel and cfg else None,
                           c_tar=p(ct) if vel else None, u_tar=p(ut) if vel and cfg else None, w_src=3.5 if cfg else 1.0,
                           w_tar=5.0 if cfg else 1.0, dt=-1e-3, keep_mask=p(mask) if vel else None, prepare=int(prepare), sigma_next=0.5,
                           zs=p(zs), zt=p(zt), znoise=p(noise), seed=6554, stream_id=3, cells=cells, C=16)
        return lambda: L.k5_flowedit_step(C.byref(a), st)

    legs = {"plain": lambda: L.k5_cfg_euler(p(zfe), p(ct), p(ut), 5.0, -1e-3, n, st),
            "flowedit_both": fe(), "flowedit_nocfg": fe(cfg=False), "flowedit_memory": fe(noise=z), "flowedit_update": fe(prepare=False),
            "flowedit_prepare": fe(vel=False)}

    def kernel_us(fn):
        assert fn() == 0, E.last_error()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.kernel_iters):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e3 / args.kernel_iters

    names = list(legs)
    for k in names:
        kernel_us(legs[k])   # warm-up: code objects, clocks
    kseries = {k: [] for k in names}
    for r in range(args.rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            kseries[k].append(kernel_us(legs[k]))
        zfe.normal_()        # thousands of updates later the latent is still finite
    assert torch.isfinite(zfe).all() and torch.isfinite(zt).all()
    med = {k: statistics.median(v) for k, v in kseries.items()}
    traffic = n * (2 * 4 + 4 * 2 + 3 * 4) + cells * 4     # reads: z_fe, x_src fp32, four bf16 velocities, the mask; writes: z_fe, zs, zt fp32
    line = {"latent": [T, H, Wd], "elements": n, "rounds": args.rounds, "kernel_iters": args.kernel_iters,
            "us_per_launch": {k: round(v, 3) for k, v in med.items()},
            "us_series": {k: [round(x, 3) for x in v] for k, v in kseries.items()},
            "us_spread": {k: round(max(v) - min(v), 3) for k, v in kseries.items()},
            "flowedit_both_bytes": traffic, "flowedit_both_GBps": round(traffic / med["flowedit_both"] * 1e-3, 1),
            "flowedit_memory_GBps": round((traffic + n * 4) / med["flowedit_memory"] * 1e-3, 1), "quoted_peak_GBps": 5300}

    if args.steps > 0:
        from kandinsky.models.dit import DiffusionTransformer3D
        with torch.device("meta"):
            dit = DiffusionTransformer3D(**dict(LITE, num_visual_blocks=args.blocks))
        dit.init_synthetic(dev, seed=0)
        te, se = ({"text_embeds": torch.randn(64, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
                  for _ in range(2))
        ne = {"text_embeds": torch.randn(32, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
        sig = sigma_schedule(50, 5.0).tolist()[17:17 + args.steps + 1]   # 33 of 50: where an edit at strength 0.66 starts
        pos = [torch.arange(T), torch.arange(H // 2), torch.arange(Wd // 2)]
        noise = torch.randn(T, H, Wd, 16, generator=g).to(dev)
        source = torch.randn(T, H, Wd, 16, generator=g).to(dev)
        forwards = {"plain": 2, "flowedit_1_1": 2, "flowedit_5_5": 4}

        def leg(name):
            w = 1.0 if name == "flowedit_1_1" else 5.0
            flow = None if name == "plain" else (source, se, torch.arange(64), w, None, 0, 6554, 17)
            dit.flowedit_state(reset=True)
            lat = noise.clone()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), w, scale_factor=(1.0, 2.0, 2.0), flowedit=flow)
            torch.cuda.synchronize(dev)
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            want = (0, 0, 0) if flow is None else (args.steps, args.steps * forwards[name], 2 if w == 1.0 else 3)
            assert dit.flowedit_state() == want, (name, dit.flowedit_state())
            return ms, lat

        for name in forwards:
            leg(name)   # warm-up: workspaces, RoPE tables, the text streams
        series, final = {k: [] for k in forwards}, {}
        order = list(forwards)
        for r in range(args.rounds):
            for name in (order if r % 2 == 0 else order[::-1]):
                ms, final[name] = leg(name)
                series[name].append(ms)
        assert all(torch.isfinite(v).all() for v in final.values())
        smed = {k: statistics.median(v) for k, v in series.items()}
        line.update({"steps": args.steps, "blocks": args.blocks, "forwards_per_step": forwards,
                     "ms_per_step": {k: round(v, 3) for k, v in smed.items()},
                     "ms_series": {k: [round(x, 3) for x in v] for k, v in series.items()},
                     "ms_spread": {k: round(max(v) - min(v), 3) for k, v in series.items()},
                     "ms_per_forward": {k: round(v / forwards[k], 3) for k, v in smed.items()}})
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
