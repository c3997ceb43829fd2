"""Golden vectors for FlowEdit: the reference's fp32 DiT inside the paper's loop (Kulikov et al. 2024, Algorithm 1 with n_avg = 1).

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_flowedit.py

Writes tests/golden/dit_tiny_flowedit.safetensors + dit_tiny_flowedit_meta.json (data only).  Model, weights and the target / negative prompts
are those of dit_tiny.safetensors; the source latent and the source prompt are tests/flowedit_reference.py's seeded draws (the prompt scaled
to the golden prompt's std) and are stored in the fixture.  Per case (source weight / target weight 1 / 1, 2 / 5, 1 / 5 at strength 0.7 of 6
steps, scale 5) the final latent in fp32 of flowedit_reference.published_loop — velocities from the reference's get_velocity at guidance 1
on the reference's own DiffusionTransformer3D, the rule's scalars in float64, z_i the normals of (seed, stream i) from the float64
restatement of the generator rounded to fp32 — and the final latent of the bf16 oracle loop (flowedit_reference.bf16_loop: the oracle's
forwards, the engine's rounding points).

The meta records, per case, the oracle loop's distance from the golden ON THE EDIT, |(out - src) - (gold - src)| / |gold - src|: the source
dominates the full latent and would hide an error.  Conditions, not measurements: nothing is written if that distance exceeds 3e-2 or if an
edit is smaller than 0.1 |src|.  The parity test holds the engine to 1.5 x the recorded distance.
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
STEPS, SCALE, SEED, STRENGTH = 6, 5.0, 6554, 0.7
CASES = {"g1_1": dict(w_src=1.0, w_tar=1.0), "g2_5": dict(w_src=2.0, w_tar=5.0), "g1_5": dict(w_src=1.0, w_tar=5.0)}
MAX_ORACLE_DISTANCE = 3e-2
MIN_EDIT = 0.1


def main():
    import flowedit_reference as FR
    import skip_reference as S
    import stochastic_reference as SR
    from oracle import k5_oracle as O
    g = load_file(os.path.join(GOLD, "dit_tiny.safetensors"))
    gmeta = json.load(open(os.path.join(GOLD, "dit_tiny_meta.json")))
    te = {"text_embeds": g["fwd.text"], "pooled_embed": g["fwd.pooled"]}
    ne = {"text_embeds": g["gen.null_text"], "pooled_embed": g["gen.null_pooled"]}
    se = FR.source_prompt(g)
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    shape = tuple(g["gen.noise"].shape)
    src = FR.source_latent(shape)
    sig = torch.linspace(1, 0, STEPS + 1)
    sig = SCALE * sig / (1 + (SCALE - 1) * sig)
    first = FR.plan(STEPS, STRENGTH)[0]
    zeros = torch.zeros_like(src), torch.zeros(*shape[:-1], 1)
    cfg = dict(gmeta["tiny_config"])
    cfg["patch_size"], cfg["axes_dims"] = tuple(cfg["patch_size"]), tuple(cfg["axes_dims"])
    ocfg = O.DitConfig(**cfg)
    sd = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    z_at = SR.step_noise(shape, SEED)
    prompts = ((se, torch.arange(FR.SOURCE_TEXT_LEN)), (ne, torch.arange(4)), (te, torch.arange(7)))

    # the bf16 oracle first: importing the reference turns torch.bfloat16 into torch.float32 for the rest of the process
    def o_vel(cond, tpos):
        return lambda x, s: S.dit_forward_skip(sd, ocfg, torch.cat([x, *zeros], -1), cond["text_embeds"], cond["pooled_embed"],
                                               s.unsqueeze(0) * 1000, pos, tpos, (1.0, 2.0, 2.0), None, "bf16", (), "block")
    T = {"flowedit.source": src, "flowedit.source_text": se["text_embeds"], "flowedit.source_pooled": se["pooled_embed"]}
    with torch.no_grad():
        for name, c in CASES.items():
            T[f"flowedit.{name}.oracle"] = FR.bf16_loop(*(o_vel(*p) for p in prompts), src, sig.tolist(), c["w_src"], c["w_tar"], z_at, first)

    from _ref_import import import_reference
    r = import_reference()
    dit = r.dit.DiffusionTransformer3D(**cfg).eval()
    dit.load_state_dict(sd)
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))

    def r_vel(cond, tpos):   # one forward: the reference's get_velocity at guidance 1
        return lambda x, s: r.gen.get_velocity(dit, torch.cat([x, *zeros], -1), s.unsqueeze(0), cond, cond, pos, tpos, tpos, 1.0, conf,
                                               sparse_params=None)
    dist, size = {}, {}
    with torch.no_grad():
        for name, c in CASES.items():
            gold = FR.published_loop(*(r_vel(*p) for p in prompts), src, sig.tolist(), c["w_src"], c["w_tar"], z_at, first).float()
            T[f"flowedit.{name}.final"] = gold
            edit = (gold - src).norm()
            dist[name] = ((T[f"flowedit.{name}.oracle"].float() - gold).norm() / edit).item()
            size[name] = (edit / src.norm()).item()
            print(f"{name}: on the edit, bf16 oracle vs golden {dist[name]:.3e}; edit / source {size[name]:.3f}")
    bad = {n: (dist[n], size[n]) for n in CASES if not dist[n] <= MAX_ORACLE_DISTANCE or not size[n] >= MIN_EDIT}
    if bad:
        raise SystemExit(f"oracle vs golden on the edit above {MAX_ORACLE_DISTANCE}, or an edit below {MIN_EDIT} of the source: {bad}")
    meta = {"steps": STEPS, "scheduler_scale": SCALE, "seed": SEED, "strength": STRENGTH, "first": first, "sigmas": [float(s) for s in sig],
            "cases": CASES, "oracle_vs_golden": dist, "edit_over_source": size, "weights": "dit_tiny.safetensors w.*",
            "source": "flowedit_reference.source_latent / source_prompt", "rope_pos": {"dense": [3, 4, 6], "text": 7, "null_text": 4,
                                                                                      "source_text": FR.SOURCE_TEXT_LEN}}
    out = os.path.join(GOLD, "dit_tiny_flowedit.safetensors")
    save_file({k: v.float().contiguous() if "final" in k or "oracle" in k else v.contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_flowedit_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
