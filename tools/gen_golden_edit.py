"""Golden vectors for video-to-video / masked editing: the reference's fp32 DiT inside the edit loop.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_edit.py

Writes tests/golden/dit_tiny_edit.safetensors + dit_tiny_edit_meta.json (data only).  The tiny DiT, noise and prompts of
dit_tiny.safetensors; a source latent and a keep mask drawn here; for w = 1 and w = 5 the final latent of the edit loop in fp32:

    x = (1 - s[first]) * source + s[first] * noise
    for i in first .. steps-1:   x = x + (s[i+1] - s[i]) * v(x, s[i])          (the reference's get_velocity, loop body :104-128)
                                 known = (1 - s[i+1]) * source + s[i+1] * noise
                                 x = known where mask == 1, x where mask == 0, x + mask * (known - x) elsewhere

with first = steps - min(steps, max(1, floor(steps * strength + 0.5))).  The mask keeps frame 0 and the left half of the other
frames, with a band of 0.25 next to the kept half.  The source is bf16-representable and stored as bf16, the mask as fp32.
"""
import json
import math
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
STEPS, SCALE, STRENGTH, WEIGHTS = 4, 5.0, 0.75, (1.0, 5.0)


def edit_mask(shape):
    """(T,H,W,1): frame 0 and the left half of the other frames kept, then two columns of 0.25, the rest free"""
    T, H, W, _ = shape
    m = torch.zeros(T, H, W, 1)
    m[0] = 1.0
    m[1:, :, :W // 2] = 1.0
    m[1:, :, W // 2:W // 2 + 2] = 0.25
    return m


def edit_loop(velocity, source, noise, mask, sig, first):
    def known_at(s):
        return (1 - s) * source + s * noise
    x = known_at(sig[first])
    for i in range(first, len(sig) - 1):
        x = x + (sig[i + 1] - sig[i]) * velocity(x, sig[i])
        known = known_at(sig[i + 1])
        x = torch.where(mask == 1, known, torch.where(mask == 0, x, x + mask * (known - x)))
    return x


def main():
    from _ref_import import import_reference
    r = import_reference()
    g = load_file(os.path.join(GOLD, "dit_tiny.safetensors"))
    gmeta = json.load(open(os.path.join(GOLD, "dit_tiny_meta.json")))
    cfg = {k: (tuple(v) if isinstance(v, list) else v) for k, v in gmeta["tiny_config"].items()}
    dit = r.dit.DiffusionTransformer3D(**cfg).eval()
    dit.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    te = {"text_embeds": g["fwd.text"], "pooled_embed": g["fwd.pooled"]}
    ne = {"text_embeds": g["gen.null_text"], "pooled_embed": g["gen.null_pooled"]}
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    noise = g["gen.noise"]
    gen = torch.Generator().manual_seed(4242)
    source = torch.randn(noise.shape, generator=gen).bfloat16().float()
    mask = edit_mask(tuple(noise.shape))
    sig = torch.linspace(1, 0, STEPS + 1)
    sig = SCALE * sig / (1 + (SCALE - 1) * sig)
    first = STEPS - min(STEPS, max(1, math.floor(STEPS * STRENGTH + 0.5)))
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)
    T = {"edit.source": source.bfloat16(), "edit.mask": mask}
    with torch.no_grad():
        for w in WEIGHTS:
            def velocity(x, s, w=w):
                return r.gen.get_velocity(dit, torch.cat([x, *zeros], -1), s.unsqueeze(0), te, ne, pos, torch.arange(7), torch.arange(4), w,
                                          conf, sparse_params=None)
            T[f"edit.{w}.final"] = edit_loop(velocity, source, noise, mask, sig, first)
    meta = {"steps": STEPS, "scheduler_scale": SCALE, "strength": STRENGTH, "first": first, "weights": list(WEIGHTS),
            "noise": "dit_tiny.safetensors gen.noise", "rope_pos": {"dense": [3, 4, 6], "text": 7, "null_text": 4}}
    out = os.path.join(GOLD, "dit_tiny_edit.safetensors")
    save_file({k: v.contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_edit_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
