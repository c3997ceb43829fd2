"""Golden vectors for the sampler's guidance controls: the reference's fp32 DiT inside a loop with per-step weights, CFG-Zero* and CFG rescale.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_guidance.py

Writes tests/golden/dit_tiny_guidance.safetensors + dit_tiny_guidance_meta.json (data only).  The tiny DiT, noise and prompts of
dit_tiny.safetensors; per case the final latent in fp32 of

    for i in 0 .. steps-1:   skip when i < zero_init                                          (CFG-Zero*: zero-init)
                             c = v(x, s[i] | prompt);  w_i == 1:  v = c
                             otherwise u = v(x, s[i] | null prompt) and, in the published tensor forms (tests/guidance_reference.py),
                                 zero_star:  st = <c, u> / (<u, u> + 1e-8),  v = u st + w_i (c - u st)   else  v = u + w_i (c - u)
                                 rescale:    v = phi v std(c) / std(v) + (1 - phi) v                       (torch.std over the sample)
                             x = x + (s[i+1] - s[i]) v

with c and u from the reference's get_velocity at guidance 1 (one forward each).  The meta file records the cases and, per case, the relative
L2 distance of the bf16 oracle loop (oracle/k5_oracle.py forwards, the engine's rounding points) from the golden: the parity tests hold the
oracle to 2e-2 of the golden and the engine to 1e-2 of the oracle, so a case must sit inside that here.
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
STEPS, SCALE, W = 6, 5.0, 5.0
SCHEDULE = [5.0, 4.5, 4.0, 3.5, 3.0, 2.5]
INTERVAL = (0.6, 0.97)          # of the sigmas 1, .962, .909, .833, .714, .5 of scale 5 the steps 1..4 lie inside: steps 0 and 5 run one forward
CASES = {
    "schedule": dict(schedule=SCHEDULE),
    "interval": dict(interval=INTERVAL),
    "zero_star_init": dict(zero_star=True, zero_init=1),
    "rescale": dict(rescale=0.7),
    "all": dict(schedule=SCHEDULE, interval=INTERVAL, zero_star=True, zero_init=1, rescale=0.7),
}


def case_weights(sig, case):
    """guidance_plan of kandinsky/generation_utils.py, spelt out so that this tool needs no engine"""
    w = list(case.get("schedule", [W] * (len(sig) - 1)))
    if "interval" in case:
        lo, hi = case["interval"]
        w = [wi if lo <= float(sig[i]) <= hi else 1.0 for i, wi in enumerate(w)]
    return w


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def main():
    import guidance_reference as R
    import k5_oracle as O
    g = load_file(os.path.join(GOLD, "dit_tiny.safetensors"))
    gmeta = json.load(open(os.path.join(GOLD, "dit_tiny_meta.json")))
    te = {"text_embeds": g["fwd.text"], "pooled_embed": g["fwd.pooled"]}
    ne = {"text_embeds": g["gen.null_text"], "pooled_embed": g["gen.null_pooled"]}
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    noise = g["gen.noise"]
    sig = torch.linspace(1, 0, STEPS + 1)
    sig = SCALE * sig / (1 + (SCALE - 1) * sig)
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)
    sd = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    ocfg = O.DitConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in gmeta["tiny_config"].items()})

    # the bf16 oracle first: importing the reference turns torch.bfloat16 into torch.float32 for the rest of the process
    def o_vel(cond, tpos):
        return lambda x, s: O.dit_forward(sd, ocfg, torch.cat([x, *zeros], -1), cond["text_embeds"], cond["pooled_embed"], s.unsqueeze(0) * 1000,
                                          pos, tpos, (1.0, 2.0, 2.0), None, "bf16")
    oracle = {}
    with torch.no_grad():
        for name, case in CASES.items():
            oracle[name] = R.bf16_loop(o_vel(te, torch.arange(7)), o_vel(ne, torch.arange(4)), noise, sig, case_weights(sig, case),
                                       case.get("zero_star", False), case.get("zero_init", 0), case.get("rescale", 0.0))

    from _ref_import import import_reference
    r = import_reference()
    cfg = {k: (tuple(v) if isinstance(v, list) else v) for k, v in gmeta["tiny_config"].items()}
    dit = r.dit.DiffusionTransformer3D(**cfg).eval()
    dit.load_state_dict(sd)
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))

    def r_vel(cond, tpos):   # one forward: the reference's get_velocity at guidance 1
        return lambda x, s: r.gen.get_velocity(dit, torch.cat([x, *zeros], -1), s.unsqueeze(0), cond, cond, pos, tpos, tpos, 1.0, conf,
                                               sparse_params=None)
    T, dist = {}, {}
    with torch.no_grad():
        for name, case in CASES.items():
            T[f"guidance.{name}.final"] = R.published_loop(r_vel(te, torch.arange(7)), r_vel(ne, torch.arange(4)), noise, sig,
                                                           case_weights(sig, case), case.get("zero_star", False), case.get("zero_init", 0),
                                                           case.get("rescale", 0.0))
            dist[name] = rel(oracle[name], T[f"guidance.{name}.final"])
            print(f"{name}: bf16 oracle vs golden {dist[name]:.3e}")
    meta = {"steps": STEPS, "scheduler_scale": SCALE, "guidance_weight": W, "sigmas": [float(s) for s in sig],
            "cases": {n: dict(c, weights=case_weights(sig, c)) for n, c in CASES.items()}, "oracle_vs_golden": dist,
            "noise": "dit_tiny.safetensors gen.noise", "rope_pos": {"dense": [3, 4, 6], "text": 7, "null_text": 4}}
    out = os.path.join(GOLD, "dit_tiny_guidance.safetensors")
    save_file({k: v.contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_guidance_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
