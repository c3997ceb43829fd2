"""Golden vectors for stochastic sampling: the reference's fp32 DiT inside the stochastic loop.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_stochastic.py

Writes tests/golden/dit_tiny_stochastic.safetensors + dit_tiny_stochastic_meta.json (data only).  Model, weights, noise and prompts are those
of dit_tiny.safetensors.  Per case the final latent in fp32 of

    for i in 0 .. steps-1:   v as tools/gen_golden_guidance.py / tools/gen_golden_skip.py form it (CFG, CFG-Zero*, the skip term)
                             sigma_down = t (1 + (t / s - 1) eta),  a = (1 - t) / (1 - sigma_down),  c = sqrt(t^2 - (sigma_down a)^2)
                             x = x + (sigma_down - s) v;   on the stochastic steps x = a x + c z_i

with s = sigmas[i], t = sigmas[i + 1], the rule in float64 (tests/stochastic_reference.py plan_f64) and z_i the normals of (seed, stream i)
from the float64 restatement of the generator rounded to fp32 — the engine forms them in fp32 inside its update kernel, to within 1e-5.
Velocities come from the reference's get_velocity at guidance 1 on the reference's own DiffusionTransformer3D; for the skip case the listed
block's `forward` is replaced by the identity on the visual stream.  Finals only.  The meta records, per case, the relative L2 distance of the
bf16 oracle loop (tests/stochastic_reference.py bf16_loop: the oracle's forwards, the engine's rounding points) from the golden; the parity
tests hold the engine to 1e-2 of the oracle and 3e-2 of the golden, so this distance must be at most 1.5e-2 here.
"""
import json
import os
import sys
from types import SimpleNamespace as NS

os.environ["TORCH_COMPILE_DISABLE"] = "1"
sys.dont_write_bytecode = True

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from safetensors.torch import load_file, save_file  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STEPS, SCALE, SEED = 6, 5.0, 6554
INTERVAL = (0.6, 0.97)          # of the sigmas 1, .962, .909, .833, .714, .5 of scale 5 the steps 1..4 lie inside
CASES = {
    "eta1_cfg": dict(w=5.0, eta=1.0),
    "eta_half_interval_nocfg": dict(w=1.0, eta=0.5, interval=INTERVAL),
    "eta1_zero_star_skip": dict(w=5.0, eta=1.0, zero_star=True, blocks=[1], g=2.0),
}
MAX_ORACLE_DISTANCE = 1.5e-2


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def main():
    import skip_reference as S
    import stochastic_reference as SR
    from oracle import k5_oracle as O
    g = load_file(os.path.join(GOLD, "dit_tiny.safetensors"))
    gmeta = json.load(open(os.path.join(GOLD, "dit_tiny_meta.json")))
    te = {"text_embeds": g["fwd.text"], "pooled_embed": g["fwd.pooled"]}
    ne = {"text_embeds": g["gen.null_text"], "pooled_embed": g["gen.null_pooled"]}
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    noise = g["gen.noise"]
    sig = torch.linspace(1, 0, STEPS + 1)
    sig = SCALE * sig / (1 + (SCALE - 1) * sig)
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)
    cfg = dict(gmeta["tiny_config"])
    cfg["patch_size"], cfg["axes_dims"] = tuple(cfg["patch_size"]), tuple(cfg["axes_dims"])
    ocfg = O.DitConfig(**cfg)
    sd = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    z_at = SR.step_noise(tuple(noise.shape), SEED)

    def mask(c):
        return [1] * STEPS if c.get("blocks") else None

    # the bf16 oracle first: importing the reference turns torch.bfloat16 into torch.float32 for the rest of the process
    def o_vel(cond, tpos, skip=()):
        return lambda x, s: S.dit_forward_skip(sd, ocfg, torch.cat([x, *zeros], -1), cond["text_embeds"], cond["pooled_embed"],
                                               s.unsqueeze(0) * 1000, pos, tpos, (1.0, 2.0, 2.0), None, "bf16", skip, "block")
    oracle = {}
    with torch.no_grad():
        for name, c in CASES.items():
            oracle[name] = SR.bf16_loop(o_vel(te, torch.arange(7)), o_vel(ne, torch.arange(4)), o_vel(te, torch.arange(7), c.get("blocks", ())),
                                        noise, sig, [c["w"]] * STEPS, SR.tables_f32(sig.tolist(), c["eta"], 1.0, c.get("interval")), z_at,
                                        c.get("g", 0.0), mask(c), c.get("zero_star", False))

    from _ref_import import import_reference
    r = import_reference()
    dit = r.dit.DiffusionTransformer3D(**cfg).eval()
    dit.load_state_dict(sd)
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))

    def identity(visual_embed, text_embed, time_embed, rope, sparse_params):
        return visual_embed

    def r_vel(cond, tpos, skip=()):   # one forward: the reference's get_velocity at guidance 1
        def vel(x, s):
            blocks = [dit.visual_transformer_blocks[b] for b in skip]
            for b in blocks:
                b.forward = identity
            try:
                return r.gen.get_velocity(dit, torch.cat([x, *zeros], -1), s.unsqueeze(0), cond, cond, pos, tpos, tpos, 1.0, conf,
                                          sparse_params=None)
            finally:
                for b in blocks:
                    del b.forward          # the instance attribute: the class's forward is back
        return vel
    T, dist = {}, {}
    with torch.no_grad():
        for name, c in CASES.items():
            T[f"stochastic.{name}.final"] = SR.published_loop(r_vel(te, torch.arange(7)), r_vel(ne, torch.arange(4)),
                                                              r_vel(te, torch.arange(7), c.get("blocks", ())), noise, sig, [c["w"]] * STEPS,
                                                              SR.plan_f64(sig.tolist(), c["eta"], 1.0, c.get("interval")), z_at, c.get("g", 0.0),
                                                              mask(c), c.get("zero_star", False))
            dist[name] = rel(oracle[name], T[f"stochastic.{name}.final"])
            print(f"{name}: bf16 oracle vs golden {dist[name]:.3e}")
    bad = {n: d for n, d in dist.items() if not d <= MAX_ORACLE_DISTANCE}
    if bad:
        raise SystemExit(f"oracle vs golden above {MAX_ORACLE_DISTANCE}: {bad}")
    meta = {"steps": STEPS, "scheduler_scale": SCALE, "seed": SEED, "first_stream": 0, "sigmas": [float(s) for s in sig],
            "cases": {n: dict(c, noise_coef=SR.tables_f32(sig.tolist(), c["eta"], 1.0, c.get("interval"))[2]) for n, c in CASES.items()},
            "oracle_vs_golden": dist, "noise": "dit_tiny.safetensors gen.noise", "weights": "dit_tiny.safetensors w.*",
            "rope_pos": {"dense": [3, 4, 6], "text": 7, "null_text": 4}}
    out = os.path.join(GOLD, "dit_tiny_stochastic.safetensors")
    save_file({k: v.contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_stochastic_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
