"""Golden vectors for spatial context windows (tiles): the reference's fp32 DiT inside the tiled loop.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_tiles.py

Writes tests/golden/dit_tiny_tiles.safetensors + dit_tiny_tiles_meta.json (data only).  The tiny DiT and prompts of dit_tiny.safetensors; a
seeded noise per case drawn here; the plan of kandinsky.generation_utils.tile_windows; for w = 1 and w = 5 the final latent of the tiled loop in
fp32:

    for i in 0 .. steps-1:   acc = 0
                             for every window k = (it * ny + iy) * nx + ix, with its box B_k of the clip:
                                 acc[B_k] += (wt[it][:, None, None] * wy[iy][None, :, None] * wx[ix][None, None, :])[..., None] * v(x[B_k], s[i])
                             x = x + (s[i+1] - s[i]) * acc

with v the reference's get_velocity (loop body :104-128) on the window's slice and the window's own RoPE positions, [3, 4, 6] patches.  Every
case is a latent (T, H, W, 16) with the window (3, 8, 12):
  s22   (3, 12, 20), rows and columns overlapping by 4: 1 x 2 x 2 windows, corner cells in four windows
  s14   (3, 8, 24), columns overlapping by 8: 1 x 1 x 4 windows, three-fold coverage along one axis
  t2s2  (5, 8, 20), frames overlapping by 1 and columns by 4: 2 x 1 x 2 windows, a temporal and a spatial axis together
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
WINDOW, C = (3, 8, 12), 16
CASES = {"s22": ((3, 12, 20), (0, 4, 4), 2201), "s14": ((3, 8, 24), (0, 0, 8), 1401), "t2s2": ((5, 8, 20), (1, 0, 4), 2202)}   # tag -> (clip, overlap, noise seed)


def boxes(starts):
    """[(it, iy, ix, (slice t, slice y, slice x))] in window order"""
    st, sy, sx = starts
    return [(it, iy, ix, (slice(t, t + WINDOW[0]), slice(y, y + WINDOW[1]), slice(x, x + WINDOW[2])))
            for it, t in enumerate(st) for iy, y in enumerate(sy) for ix, x in enumerate(sx)]


def tiled_loop(velocity, noise, starts, weights, sig):
    wt, wy, wx = weights
    x = noise.clone()
    for i in range(len(sig) - 1):
        acc = torch.zeros_like(x)
        for it, iy, ix, box in boxes(starts):
            share = wt[it][:, None, None] * wy[iy][None, :, None] * wx[ix][None, None, :]
            acc[box] += share[..., None] * velocity(x[box].contiguous(), sig[i])
        x = x + (sig[i + 1] - sig[i]) * acc
    return x


def plans():
    """{tag: (starts, weights)} from this project's tile_windows; its package is dropped again, the reference takes the name `kandinsky` next"""
    pkg = os.path.join(ROOT, "kandinsky-5_amd")
    sys.path.insert(0, pkg)
    from kandinsky.generation_utils import tile_windows
    out = {}
    for tag, (clip, overlap, _) in CASES.items():
        p = tile_windows(clip, WINDOW, overlap)
        assert p.window == WINDOW
        out[tag] = ([list(s) for s in p.starts], [w.clone() for w in p.weights])
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
    pos = [torch.arange(WINDOW[0]), torch.arange(WINDOW[1] // 2), torch.arange(WINDOW[2] // 2)]
    zeros = torch.zeros(*WINDOW, C), torch.zeros(*WINDOW, 1)
    T, meta_cases = {}, {}
    with torch.no_grad():
        for tag, (clip, overlap, seed) in CASES.items():
            starts, weights = plan[tag]
            noise = torch.randn(*clip, C, generator=torch.Generator().manual_seed(seed))
            T[f"tile.{tag}.noise"] = noise
            for name, w in zip(("wt", "wy", "wx"), weights):
                T[f"tile.{tag}.{name}"] = w
            for w in WEIGHTS:
                def velocity(x, s, w=w):
                    return r.gen.get_velocity(dit, torch.cat([x, *zeros], -1), s.unsqueeze(0), te, ne, pos, torch.arange(7), torch.arange(4), w,
                                              conf, sparse_params=None)
                T[f"tile.{tag}.{w}.final"] = tiled_loop(velocity, noise, starts, weights, sig)
            meta_cases[tag] = {"clip": list(clip), "overlap": list(overlap), "starts": starts, "seed": seed}
    meta = {"steps": STEPS, "scheduler_scale": SCALE, "weights": list(WEIGHTS), "window": list(WINDOW), "cases": meta_cases,
            "rope_pos": {"window": [3, 4, 6], "text": 7, "null_text": 4}}
    out = os.path.join(GOLD, "dit_tiny_tiles.safetensors")
    save_file({k: v.contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_tiles_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
