"""MagCache calibration at BASELINE config 2's size (47 616 tokens, D = 1792): what the statistics pass and the calibrating mode cost.

    python tools/magcache_calib_bench.py kernel                      # the fused residual + statistics pass against ln_kernel, same run
    python tools/magcache_calib_bench.py overhead [--steps 20 --warmup 5]   # plain / calibrating / plain sampling, bench.py's 5s_nocfg workload
    python tools/magcache_calib_bench.py table --out profiles/FILE.json     # a 50-step calibration on the bench's SYNTHETIC weights

`overhead` and `table` build the model exactly as bench.py does (LITE, 32 blocks, init_synthetic(seed 0, host_rng), seed-6554 noise, seed-6555
prompts, the 50-step schedule with s = 5) and time k5_sample calls the same way (profiling level 2 inside the timed region), so that the plain
figure is comparable with `bench.py --steps K --warmup W`.  The table of `table` comes from random weights: a record that the full-size path
runs and counts every row, NOT a table to sample with."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kandinsky-5_amd"))
import torch  # noqa: E402
from kandinsky import _engine as E  # noqa: E402

N, D = 47616, 1792
LITE = dict(in_visual_dim=16, out_visual_dim=16, time_dim=512, patch_size=(1, 2, 2), model_dim=1792, ff_dim=7168, num_text_blocks=2,
            num_visual_blocks=32, axes_dims=(16, 24, 24), visual_cond=True, in_text_dim=3584, in_text_dim2=768)


def event_ms(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel():
    """Back-to-back launches on one stream, HIP events around `iters` of them.  Each launch streams 4 x 170 MB (ln: 2 x 170 MB), more than the
    256 MB of Infinity Cache, and the next launch starts on the rows that were evicted first: every launch reads from HBM ("cold" in the sense
    that matters for a pass that runs once per forward behind 32 blocks of other traffic).  The small case fits the cache: "hot"."""
    out = {}
    for n, tag in ((N, "config2_47616x1792"), (4096, "hot_4096x1792")):
        g = torch.Generator(device="cuda").manual_seed(1)
        vis, ori, prev = (torch.randn(n, D, device="cuda", generator=g).bfloat16() for _ in range(3))
        res = torch.empty_like(vis)
        scale, shift = torch.randn(D, device="cuda", generator=g), torch.randn(D, device="cuda", generator=g)
        gate = torch.full((D,), -1.0, device="cuda")
        sums = torch.zeros(4, dtype=torch.float64, device="cuda")
        L, s = E.lib(), E.stream_ptr()
        lnout = torch.empty_like(vis)
        runs = {
            "magcache_stats": (lambda: L.k5_magcache_stats_bf16(vis.data_ptr(), ori.data_ptr(), prev.data_ptr(), res.data_ptr(), sums.data_ptr(), n, D, s), 4),
            "magcache_stats_no_prev": (lambda: L.k5_magcache_stats_bf16(vis.data_ptr(), ori.data_ptr(), None, res.data_ptr(), sums.data_ptr(), n, D, s), 3),
            "gate_sum_minus_one": (lambda: L.k5_gate_sum_bf16(vis.data_ptr(), ori.data_ptr(), gate.data_ptr(), res.data_ptr(), n, D, s), 3),
            "ln_modulate": (lambda: L.k5_ln_modulate_bf16(vis.data_ptr(), scale.data_ptr(), shift.data_ptr(), lnout.data_ptr(), n, D, D, D, s), 2),
        }
        rec = {}
        for rep in range(3):   # alternate the kernels: three rounds each, the median is reported with the range
            for name, (fn, passes) in runs.items():
                ms = event_ms(fn, iters=20, warm=3)
                rec.setdefault(name, {"bytes": passes * n * D * 2, "ms": []})["ms"].append(ms)
        for name, r in rec.items():
            ms = sorted(r["ms"])
            r["ms_median"], r["TBps_median"] = ms[1], r["bytes"] / ms[1] / 1e9
            print(f"{tag:22s} {name:24s} {ms[1] * 1e3:8.1f} us (range {ms[0] * 1e3:.1f}-{ms[2] * 1e3:.1f})  {r['bytes'] / 1e6:7.1f} MB  {r['TBps_median']:.2f} TB/s", flush=True)
        out[tag] = rec
    return out


def build_model():
    from kandinsky.models.dit import DiffusionTransformer3D
    from kandinsky.generation_utils import sigma_schedule
    dev = torch.device("cuda", 0)
    with torch.device("meta"):
        dit = DiffusionTransformer3D(**LITE)
    dit.init_synthetic(dev, seed=0, host_rng=True)
    T, H, W, Lt, Ln = 31, 64, 96, 256, 32
    noise = torch.randn(T, H, W, 16, generator=torch.Generator().manual_seed(6554))
    g = torch.Generator().manual_seed(6555)
    te = {"text_embeds": torch.randn(Lt, 3584, generator=g).bfloat16().to(dev), "pooled_embed": torch.randn(1, 768, generator=g).bfloat16().to(dev)}
    ne = {"text_embeds": torch.randn(Ln, 3584, generator=g).bfloat16().to(dev), "pooled_embed": torch.randn(1, 768, generator=g).bfloat16().to(dev)}
    vpos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]

    def run(latent, sig):
        dit.sample(latent, sig, te, ne, vpos, torch.arange(Lt), torch.arange(Ln), 1.0, scale_factor=(1.0, 2.0, 2.0))
    return dit, noise, dev, run, sigma_schedule


def timed(dit, run, latent, sig, warmup, steps, dev):
    run(latent, sig[:warmup + 1])
    torch.cuda.synchronize(dev)
    dit.set_profiling(2)
    dit.reset_profile()
    t0 = time.perf_counter()
    run(latent, sig[warmup:warmup + steps + 1])
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    dit.set_profiling(0)
    return dt / steps * 1e3


def overhead(steps, warmup):
    from kandinsky.magcache_utils import start_magcache_calibration, stop_magcache_calibration
    dit, noise, dev, run, sigma_schedule = build_model()
    sig = sigma_schedule(max(50, warmup + steps), 5.0).tolist()
    rec = {"steps": steps, "warmup": warmup, "ms_per_step": []}
    for mode in ("plain", "calibrating", "plain", "calibrating"):
        latent = noise.to(dev)
        if mode == "calibrating":
            free0 = torch.cuda.mem_get_info(dev)[0]          # after a plain run: the workspaces are sized, what follows is the mode's own memory
            start_magcache_calibration(dit, len(sig) - 1, True)
        ms = timed(dit, run, latent, sig, warmup, steps, dev)
        extra = None
        if mode == "calibrating":
            extra = (free0 - torch.cuda.mem_get_info(dev)[0]) / 1e6
            stop_magcache_calibration(dit)
        rec["ms_per_step"].append({"mode": mode, "ms": ms, "device_memory_added_MB": extra})
        print(f"{mode:12s} {ms:8.2f} ms per step" + (f"   (+{extra:.0f} MB of device memory while calibrating)" if extra is not None else ""), flush=True)
    return rec


def table(steps):
    from kandinsky.magcache_utils import magcache_calibration, start_magcache_calibration, stop_magcache_calibration
    dit, noise, dev, run, sigma_schedule = build_model()
    sig = sigma_schedule(steps, 5.0).tolist()
    latent = noise.to(dev)
    free0 = torch.cuda.mem_get_info(dev)[0]
    run(latent, sig[:2])                                   # sizes the workspaces, so that the difference below is the mode's own memory
    torch.cuda.synchronize(dev)
    free1 = torch.cuda.mem_get_info(dev)[0]
    latent = noise.to(dev)
    start_magcache_calibration(dit, steps, True)
    t0 = time.perf_counter()
    run(latent, sig)
    d = magcache_calibration(dit)
    dt = time.perf_counter() - t0
    d["device_memory_added_MB"] = (free1 - torch.cuda.mem_get_info(dev)[0]) / 1e6
    stop_magcache_calibration(dit)
    d.update(seconds=dt, tokens=N, workload="5s_nocfg shape (31, 64, 96, 16), guidance 1.0, 50-step schedule s = 5, bench.py's synthetic weights (seed 0)",
             warning="RANDOM WEIGHTS: not a table to sample with; a record that the full-size path runs end to end and counts every row",
             latent_finite=bool(torch.isfinite(latent).all()), workspace_MB=(free0 - free1) / 1e6)
    print(f"{steps}-step calibration: {dt:.1f} s, rows counted {d['rows_counted']} of {d['rows_total']}, +{d['device_memory_added_MB']:.0f} MB; "
          f"ratios {d['mag_ratios'][0]:.4f} ... {d['mag_ratios'][-2]:.4f}", flush=True)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "overhead", "table"))
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="", help="write the record as JSON")
    a = ap.parse_args()
    rec = kernel() if a.what == "kernel" else overhead(a.steps or 20, a.warmup) if a.what == "overhead" else table(a.steps or 50)
    rec = {"tool": "tools/magcache_calib_bench.py " + a.what, "device": torch.cuda.get_device_name(0), "record": rec}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps({"what": a.what, "ok": True}))


if __name__ == "__main__":
    main()
