"""Golden vectors for temporal context windows: the reference's fp32 DiT inside the windowed loop.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_windows.py

Writes tests/golden/dit_tiny_windows.safetensors + dit_tiny_windows_meta.json (data only).  The tiny DiT and prompts of
dit_tiny.safetensors; a seeded noise per case drawn here; the plan of kandinsky.generation_utils.context_windows; for w = 1 and w = 5
the final latent of the windowed loop in fp32:

    for i in 0 .. steps-1:   acc = 0
                             for every window k:  acc[starts[k] : starts[k] + F] += weights[k][:, None, None, None] * v(x[starts[k] : starts[k] + F], s[i])
                             x = x + (s[i+1] - s[i]) * acc

with v the reference's get_velocity (loop body :104-128) on the window's slice and the window's own RoPE positions 0 .. F-1.  Cases:
T = 7 as windows of 3 overlapping by 2 (three-fold coverage) and T = 6 as windows of 3 overlapping by 1 (ragged overlaps of 2 and 1).
"""
import json
import os
import sys
from types import SimpleNamespace as NS

os.environ["TORCH_COMPILE_DISABLE"] = "1"
sys.dont_write_bytecode = True

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402
from safetensors.torch import load_file, save_file  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STEPS, SCALE, WEIGHTS = 4, 5.0, (1.0, 5.0)
CASES = {"t7": (7, 3, 2, 707), "t6": (6, 3, 1, 606)}   # tag -> (T, F, overlap, noise seed)
HW = (8, 12, 16)


def windowed_loop(velocity, noise, starts, weights, sig):
    F = weights.shape[1]
    x = noise.clone()
    for i in range(len(sig) - 1):
        acc = torch.zeros_like(x)
        for k, st in enumerate(starts):
            acc[st:st + F] += weights[k][:, None, None, None] * velocity(x[st:st + F], sig[i])
        x = x + (sig[i + 1] - sig[i]) * acc
    return x


def plans():
    """{tag: (starts, weights)} from this project's context_windows; its package is dropped again, the reference takes the name `kandinsky` next"""
    pkg = os.path.join(ROOT, "kandinsky-5_amd")
    sys.path.insert(0, pkg)
    from kandinsky.generation_utils import context_windows
    out = {tag: context_windows(frames, F, overlap) for tag, (frames, F, overlap, _) in CASES.items()}
    for name in [m for m in sys.modules if m == "kandinsky" or m.startswith("kandinsky.")]:
        del sys.modules[name]
    sys.path.remove(pkg)
    return out


def main():
    from _ref_import import import_reference
    plan = plans()
    r = import_reference()
    g = load_file(os.path.join(GOLD, "dit_tiny.safetensors"))
    gmeta = json.load(open(os.path.join(GOLD, "dit_tiny_meta.json")))
    cfg = {k: (tuple(v) if isinstance(v, list) else v) for k, v in gmeta["tiny_config"].items()}
    dit = r.dit.DiffusionTransformer3D(**cfg).eval()
    dit.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    te = {"text_embeds": g["fwd.text"], "pooled_embed": g["fwd.pooled"]}
    ne = {"text_embeds": g["gen.null_text"], "pooled_embed": g["gen.null_pooled"]}
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    sig = torch.linspace(1, 0, STEPS + 1)
    sig = SCALE * sig / (1 + (SCALE - 1) * sig)
    T, meta_cases = {}, {}
    with torch.no_grad():
        for tag, (frames, F, overlap, seed) in CASES.items():
            starts, weights = plan[tag]
            noise = torch.randn(frames, *HW, generator=torch.Generator().manual_seed(seed))
            pos = [torch.arange(F), torch.arange(HW[0] // 2), torch.arange(HW[1] // 2)]
            zeros = torch.zeros(F, *HW), torch.zeros(F, *HW[:2], 1)
            T[f"win.{tag}.noise"] = noise
            T[f"win.{tag}.weights"] = weights
            for w in WEIGHTS:
                def velocity(x, s, w=w):
                    return r.gen.get_velocity(dit, torch.cat([x, *zeros], -1), s.unsqueeze(0), te, ne, pos, torch.arange(7), torch.arange(4), w,
                                              conf, sparse_params=None)
                T[f"win.{tag}.{w}.final"] = windowed_loop(velocity, noise, starts, weights, sig)
            meta_cases[tag] = {"T": frames, "frames": F, "overlap": overlap, "starts": starts, "seed": seed}
    meta = {"steps": STEPS, "scheduler_scale": SCALE, "weights": list(WEIGHTS), "cases": meta_cases,
            "rope_pos": {"window": [3, 4, 6], "text": 7, "null_text": 4}}
    out = os.path.join(GOLD, "dit_tiny_windows.safetensors")
    save_file({k: v.contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_windows_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
