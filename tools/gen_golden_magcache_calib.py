"""Golden vectors for MagCache calibration: per-call residual statistics FROM THE REFERENCE'S OWN forward.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_magcache_calib.py

The reference ships ratio tables and not the code that measured them; what it does have is the residual it caches.  This script
installs the reference's `set_magcache_params` on the tiny DiT of tests/golden/dit_tiny.safetensors (imported under the patches of
oracle/_ref_import.py, `torch.compile` replaced by the identity) and sets `dit.magcache_thresh = 0.0`: the reference's own
condition `accumulated_err < thresh` then never holds, so no call is skipped and every call caches a fresh residual.  A spy on
`after_blocks` — called right after `residual_cache[cnt % 2]` was written and before the counter advances — snapshots that residual
and the counter, and per call the script stores, in float64 over the rows of the residual against the previous residual of the slot,
the estimator of the MagCache paper's calibration script:
    ratio = mean_i |res_i| / |prev_i|,   std = unbiased standard deviation of the same (torch `.std()`),   cos = mean_i 1 - cos(res_i, prev_i).
Cases (latent (3, 8, 12, 16), 10 steps, scheduler scale 5): guidance 2.0 (CFG: 20 calls), guidance 1.0 (no_cfg: 10 calls, slot 0 only),
both through the reference's own `generate`; and one conditioned case, guidance 2.0, with the conditioning inputs of
tests/golden/dit_tiny_visual_cond.safetensors (latent + mask 1 on frame 0) through the reference's loop body, as
tools/gen_golden_visual_cond.py runs it.  Writes data only: tests/golden/magcache_calib_tiny.safetensors + magcache_calib_tiny.json.
"""
import json
import os
import sys

os.environ["TORCH_COMPILE_DISABLE"] = "1"
sys.dont_write_bytecode = True

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from safetensors.torch import load_file, save_file  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STEPS, SCALE, SHAPE = 10, 5.0, (3, 8, 12, 16)


def row_stats(res, prev):
    """(mean ratio, unbiased std, mean cosine distance, smallest row norm) in float64 over the rows of (n, D) residuals"""
    r, p = res.double().reshape(-1, res.shape[-1]), prev.double().reshape(-1, prev.shape[-1])
    nr, npv = r.norm(dim=-1), p.norm(dim=-1)
    rho = nr / npv
    cos = (r * p).sum(-1) / (nr * npv)
    return float(rho.mean()), float(rho.std()), float((1.0 - cos).mean()), float(torch.minimum(nr, npv).min())


def main():
    from _ref_import import import_reference
    from gen_golden_visual_cond import conditioned_loop, conf_ns
    vc0 = load_file(os.path.join(GOLD, "dit_tiny_visual_cond.safetensors"))["cond.visual_cond0"].float()   # stored as bf16: read before the patches
    r = import_reference()                                                                                 # (torch.bfloat16 := torch.float32 from here)
    torch.compile = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    import kandinsky.magcache_utils as kmag

    g = load_file(os.path.join(GOLD, "dit_tiny.safetensors"))
    gmeta = json.load(open(os.path.join(GOLD, "dit_tiny_meta.json")))
    cfg = {k: (tuple(v) if isinstance(v, list) else v) for k, v in gmeta["tiny_config"].items()}
    dit = r.dit.DiffusionTransformer3D(**cfg).eval()
    dit.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    te = {"text_embeds": g["fwd.text"], "pooled_embed": g["fwd.pooled"]}
    ne = {"text_embeds": g["gen.null_text"], "pooled_embed": g["gen.null_pooled"]}
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    noise = g["gen.noise"]
    assert tuple(noise.shape) == SHAPE
    assert torch.equal(torch.randn(*SHAPE, generator=torch.Generator().manual_seed(6554)), noise)   # what the reference's generate draws

    snaps = []
    orig_after = dit.after_blocks

    def spy_after(*a, **k):
        snaps.append((dit.cnt, dit.residual_cache[dit.cnt % 2].clone()))
        return orig_after(*a, **k)
    dit.after_blocks = spy_after

    vc = torch.zeros(SHAPE)
    vc[0] = vc0
    mask = torch.zeros(*SHAPE[:-1], 1)
    mask[0] = 1.0
    conf = conf_ns(dict(type="flash"))
    T, meta = {}, {"estimator": "float64 over rows: mean |res_i|/|prev_i|, unbiased std of it, mean 1 - cos(res_i, prev_i)", "cases": []}
    with torch.no_grad():
        for tag, w, conditioned in (("cfg", 2.0, False), ("nocfg", 1.0, False), ("cond", 2.0, True)):
            no_cfg = abs(w - 1.0) <= 1e-6
            kmag.set_magcache_params(dit, [1.0] * (2 * STEPS - 2), STEPS, no_cfg)   # the table is never consulted to skip ...
            dit.magcache_thresh = 0.0                                               # ... because accumulated_err < 0 never holds
            snaps.clear()
            if conditioned:
                final, _ = conditioned_loop(r.gen, dit, noise, STEPS, SCALE, w, te, ne, pos, torch.arange(7), torch.arange(4), conf, vc, mask)
            else:
                final = r.gen.generate(dit, "cpu", SHAPE, STEPS, te, ne, pos, torch.arange(7), torch.arange(4), w, SCALE, conf, seed=6554)
            assert dit.cnt == 0 and len(snaps) == (STEPS if no_cfg else 2 * STEPS)
            assert [c for c, _ in snaps] == list(range(0, 2 * STEPS, 2 if no_cfg else 1))
            last, calls, stats = {}, [], []
            for cnt, res in snaps:
                slot = cnt % 2
                if slot in last:
                    calls.append(cnt)
                    stats.append(row_stats(res, last[slot]))
                last[slot] = res
            st = np.asarray(stats, dtype=np.float64)
            assert st[:, 3].min() > 0, "a residual row with zero norm: pick other inputs"
            T[f"calib.{tag}.ratio"] = torch.from_numpy(st[:, 0].copy())
            T[f"calib.{tag}.std"] = torch.from_numpy(st[:, 1].copy())
            T[f"calib.{tag}.cos"] = torch.from_numpy(st[:, 2].copy())
            T[f"calib.{tag}.final"] = final.float()
            meta["cases"].append({"tag": tag, "num_steps": STEPS, "scheduler_scale": SCALE, "guidance_weight": w, "no_cfg": no_cfg,
                                  "conditioned": conditioned, "latent_shape": list(SHAPE), "calls": calls,
                                  "rows_per_call": int(snaps[0][1].reshape(-1, snaps[0][1].shape[-1]).shape[0]),
                                  "min_row_norm": float(st[:, 3].min())})
            print(tag, "calls", len(snaps), "ratios", np.round(st[:4, 0], 4), "...", np.round(st[-2:, 0], 4))
    save_file({k: v.contiguous() for k, v in T.items()}, os.path.join(GOLD, "magcache_calib_tiny.safetensors"))
    with open(os.path.join(GOLD, "magcache_calib_tiny.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
