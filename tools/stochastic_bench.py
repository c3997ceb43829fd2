"""What stochastic sampling costs, on the 5 s clip's latent (31, 64, 96, 16) — 3.0 M elements.

Per launch (HIP events over `--kernel_iters` launches, the legs alternating, the order flipping every round, `--rounds` times):

    plain             k5_cfg_euler, the update every run without a plan enqueues
    sto_kernel        k5_stochastic_euler with noise_coef != 0 and the noise generated inside the kernel (Philox4x32-10 + Box-Muller)
    sto_memory        k5_stochastic_euler with the same coefficients and the noise read from an fp32 buffer
    sto_no_noise      k5_stochastic_euler with noise_coef = 0 (the last step of every run)
    noise_only        k5_noise_normal_f32 alone: the generator and one fp32 store per element

each at guidance 5 (two velocity streams) and, for the update legs, at guidance 1.  `--other_lib PATH`: another build of the library (the
parent commit's, say) whose k5_cfg_euler joins the rotation as `plain_other` on the same buffers, for the question whether the plain launch
changed.

Per step: ms per step of DiffusionTransformer3D.sample with synthetic weights (2B Lite, random-init, full depth by default) at guidance 5,
`off` (no plan) against `eta1` (stochastic_plan at eta = 1), alternating likewise; a leg's wall time is taken between two device
synchronisations and divided by the steps.  `--steps 0` leaves this part out.  One JSON line, appended to profiles/stochastic_bench.jsonl.

    python tools/stochastic_bench.py [--steps 4] [--rounds 5] [--blocks 32] [--kernel_iters 200] [--other_lib PATH]
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
    ap.add_argument("--steps", type=int, default=4, help="Euler steps per leg of the per-step part (0: leave it out)")
    ap.add_argument("--rounds", type=int, default=5, help="rotations of the legs")
    ap.add_argument("--blocks", type=int, default=32, help="visual blocks (32 = the real model)")
    ap.add_argument("--kernel_iters", type=int, default=200, help="launches per kernel timing")
    ap.add_argument("--other_lib", default=None, help="another build of libk5.so whose k5_cfg_euler is timed next to this one's")
    ap.add_argument("--shape", type=int, nargs=3, default=(31, 64, 96), metavar=("T", "H", "W"), help="latent shape (default: the 5 s clip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stochastic_bench.jsonl"))
    args = ap.parse_args()
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule, stochastic_plan

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    T, H, Wd = args.shape
    n = T * H * Wd * 16
    L, st = E.lib(), E.stream_ptr(dev)
    c, u = (torch.randn(n, generator=g).to(dev).bfloat16() for _ in range(2))
    img, z = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def sto(uu, w, coef, noise):
        return lambda: L.k5_stochastic_euler(p(img), p(c), p(uu), None, w, None, 0.0, -1e-3, None, None, None, 0.5, n // 16, 16, None, 0.999, coef, p(noise),
                                             6554, 3, st)

    legs = {"plain": lambda: L.k5_cfg_euler(p(img), p(c), p(u), 5.0, -1e-3, n, st),
            "sto_kernel": sto(u, 5.0, 1e-3, None), "sto_memory": sto(u, 5.0, 1e-3, z), "sto_no_noise": sto(u, 5.0, 0.0, None),
            "plain_nocfg": lambda: L.k5_cfg_euler(p(img), p(c), None, 1.0, -1e-3, n, st),
            "sto_kernel_nocfg": sto(None, 1.0, 1e-3, None), "sto_memory_nocfg": sto(None, 1.0, 1e-3, z),
            "noise_only": lambda: L.k5_noise_normal_f32(p(z), n, 6554, 3, st)}
    if args.other_lib:
        other = C.CDLL(os.path.abspath(args.other_lib))
        sig_ = E.SYMBOLS["k5_cfg_euler"]
        other.k5_cfg_euler.restype, other.k5_cfg_euler.argtypes = sig_
        legs["plain_other"] = lambda: other.k5_cfg_euler(p(img), p(c), p(u), 5.0, -1e-3, n, st)
        legs["plain_other_nocfg"] = lambda: other.k5_cfg_euler(p(img), p(c), None, 1.0, -1e-3, n, st)

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
        z.normal_()   # the memory leg's buffer was overwritten by noise_only: fresh values, the same traffic
        img.normal_()               # thousands of updates later the latent is still finite
    assert torch.isfinite(img).all()

    line = {"latent": [T, H, Wd], "elements": n, "rounds": args.rounds, "kernel_iters": args.kernel_iters,
            "us_per_launch": {k: round(statistics.median(v), 3) for k, v in kseries.items()},
            "us_series": {k: [round(x, 3) for x in v] for k, v in kseries.items()},
            "us_spread": {k: round(max(v) - min(v), 3) for k, v in kseries.items()}}
    if args.other_lib:
        line["other_lib"] = args.other_lib
        line["plain_minus_other_us"] = {k: round(line["us_per_launch"]["plain" + k] - line["us_per_launch"]["plain_other" + k], 3)
                                        for k in ("", "_nocfg")}

    if args.steps > 0:
        from kandinsky.models.dit import DiffusionTransformer3D
        with torch.device("meta"):
            dit = DiffusionTransformer3D(**dict(LITE, num_visual_blocks=args.blocks))
        dit.init_synthetic(dev, seed=0)
        te = {"text_embeds": torch.randn(64, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
        ne = {"text_embeds": torch.randn(32, 3584, generator=g).to(dev), "pooled_embed": torch.randn(1, 768, generator=g).to(dev)}
        sig = sigma_schedule(50, 5.0).tolist()[:args.steps + 1]
        pos = [torch.arange(T), torch.arange(H // 2), torch.arange(Wd // 2)]
        noise = torch.randn(T, H, Wd, 16, generator=g).to(dev)
        plan = stochastic_plan(sig, 1.0)

        def leg(name):
            if name == "eta1":
                dit.set_stochastic(*plan, seed=6554)
            dit.stochastic_state(reset=True)
            lat = noise.clone()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            dit.sample(lat, sig, te, ne, pos, torch.arange(64), torch.arange(32), 5.0, scale_factor=(1.0, 2.0, 2.0))
            torch.cuda.synchronize(dev)
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            count = dit.stochastic_state()[1]
            dit.clear_stochastic()
            assert count == (sum(1 for v in plan[2] if v != 0.0) if name == "eta1" else 0), (name, count)
            return ms, lat

        leg("eta1")   # warm-up: workspaces, RoPE tables, both text streams
        series, final = {"off": [], "eta1": []}, {}
        for r in range(args.rounds):
            for name in (("off", "eta1") if r % 2 == 0 else ("eta1", "off")):
                ms, final[name] = leg(name)
                series[name].append(ms)
        assert torch.isfinite(final["eta1"]).all() and not torch.equal(final["eta1"], final["off"]), "the plan left the run as it was"
        med = {k: statistics.median(v) for k, v in series.items()}
        line.update({"steps": args.steps, "blocks": args.blocks,
                     "ms_per_step": {k: round(v, 3) for k, v in med.items()},
                     "ms_series": {k: [round(x, 3) for x in v] for k, v in series.items()},
                     "ms_spread": {k: round(max(v) - min(v), 3) for k, v in series.items()},
                     "extra_ms_per_step": round(med["eta1"] - med["off"], 3),
                     "extra_percent": round(100 * (med["eta1"] - med["off"]) / med["off"], 3)})
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
