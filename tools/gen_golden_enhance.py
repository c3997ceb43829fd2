"""Golden vectors for Enhance-A-Video: the reference's fp32 DiT with the rule of include/k5.h (k5_enhance_scores_bf16) applied in float32
around the self-attention of its own visual blocks.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_enhance.py

Writes tests/golden/dit_tiny_enhance.safetensors + dit_tiny_enhance_meta.json (data only).  The tiny DiT, inputs, noise and prompts of
dit_tiny.safetensors.  Per visual block and forward (conditional and unconditional alike), with q, k what the module hands its attention
(after norm_qk and the rotation), T the latent frames and S the spatial positions of the token grid:

    z[t][u] = <q[t,p,h], k[u,p,h]> / 8;  P = softmax over u;  m(p,h) = sum_{t != u} P[t][u] / (T (T - 1))
    score = max(1, mean_{p,h} m * (T + weight));  the attention's output times score, then the module's out_l

Two sets: A with weight 4.0 (the scores well above 1) and B with weight 0.0 (on these weights the single forward has mean * T < 1 in both
blocks: the clamp holds and its fp32 velocity is the plain golden exactly; some forwards of the 4-step loops do rise above 1).  For each: one forward velocity (the fwd.* inputs) with its per-block scores, and the final
latent of the 4-step loop at guidance 1 and 5 (scheduler_scale 5, gen.noise).  Asserted and recorded: delta, the relative L2 of each result
against the plain result of the same run (A: >= 0.04 on every case, every forward score > 1.5; B: exactly 0 for the forward), and per block bf16_spread, the
relative change of the forward's score when q and k are rounded to bf16 before the rule — the yardstick of the engine's score tolerance.
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
STEPS, SCALE, WEIGHTS, DELTA_MIN, SCORE_MIN = 4, 5.0, (1.0, 5.0), 0.04, 1.5
SETS = {"A": 4.0, "B": 0.0}
BF16 = torch.bfloat16   # the real one, taken before import_reference turns torch.bfloat16 into float32 (fp32 oracle mode)


def cross_frame_mean(q, k, T):
    """the definition, in the dtype of q and k ([T S][Hh][64], token row = t * S + p): mean over (p, h) of the off-diagonal mass"""
    N, Hh, hd = q.shape
    S = N // T
    qq, kk = q.reshape(T, S, Hh, hd), k.reshape(T, S, Hh, hd)
    z = torch.einsum("tphd,uphd->phtu", qq, kk) / 8.0
    P = torch.softmax(z, dim=-1)
    off = P.sum((-1, -2)) - P.diagonal(dim1=-2, dim2=-1).sum(-1)
    return (off / (T * (T - 1))).double().mean()


class Enhance:
    """The rule on a reference DiT: while `weight` is set every visual block's self-attention output is scaled.  Only the modules' own
    methods are called; `scores` and `spread` collect (forward, block) values in call order."""

    def __init__(self, dit):
        self.dit, self.weight, self.T = dit, None, 0
        self.scores, self.spread, self.mean_T = [], [], []
        dit.register_forward_pre_hook(self.on_forward)
        for b in dit.visual_transformer_blocks:
            sa = b.self_attention
            inner = sa.attention
            sa.attention = lambda q, k, v, inner=inner: self.attend(inner, q, k, v)

    def on_forward(self, module, args):
        self.T = args[0].shape[0]

    def attend(self, inner, q, k, v):
        out = inner(q, k, v)
        if self.weight is None or self.T < 2:
            return out
        T = self.T
        mean = cross_frame_mean(q.float(), k.float(), T)
        score = max(1.0, float(mean) * (T + self.weight))
        rounded = max(1.0, float(cross_frame_mean(q.to(BF16).float(), k.to(BF16).float(), T)) * (T + self.weight))
        self.scores.append(score)
        self.mean_T.append(float(mean) * T)
        self.spread.append(abs(rounded - score) / score)
        return out * torch.tensor(score, dtype=torch.float32)


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


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
    enh = Enhance(dit)
    nb = len(dit.visual_transformer_blocks)

    def run_all(weight):
        """{case: result} with the rule at `weight` (None = plain), and the single forward's (scores, spreads, mean * T)"""
        out = {}
        enh.weight = weight
        with torch.no_grad():
            enh.scores, enh.spread, enh.mean_T = [], [], []
            out["fwd"] = dit(g["fwd.x"], te["text_embeds"], te["pooled_embed"], g["fwd.time"], pos, torch.arange(7), scale_factor=(1.0, 2.0, 2.0))
            fwd = (list(enh.scores), list(enh.spread), list(enh.mean_T))
            for w in WEIGHTS:
                out[f"gen.{w}"] = r.gen.generate(dit, "cpu", tuple(g["gen.noise"].shape), STEPS, te, ne, pos, torch.arange(7), torch.arange(4), w,
                                                 SCALE, conf, seed=gmeta["gen_seed"])
        enh.weight = None
        return out, fwd

    plain, _ = run_all(None)
    # the wrapper is idle without a weight: the plain runs are the goldens of dit_tiny.safetensors
    assert torch.equal(plain["fwd"], g["fwd.out"])
    for w in WEIGHTS:
        assert torch.equal(plain[f"gen.{w}"], g[f"gen.{STEPS}_{SCALE}_{w}.final"])

    T, meta = {}, {"steps": STEPS, "scheduler_scale": SCALE, "weights": list(WEIGHTS), "delta_min": DELTA_MIN, "score_min": SCORE_MIN,
                   "rope_pos": {"dense": [3, 4, 6], "text": 7, "null_text": 4}, "sets": {}}
    for name, weight in SETS.items():
        res, (scores, spread, mean_T) = run_all(weight)
        assert len(scores) == nb
        deltas = {k: rel(res[k], plain[k]) for k in res}
        print(name, "weight", weight, "scores", [round(s, 4) for s in scores], "mean*T", [round(m, 4) for m in mean_T], "delta",
              {k: round(d, 4) for k, d in deltas.items()}, "bf16_spread", ["%.2e" % s for s in spread])
        if name == "A":
            assert min(deltas.values()) >= DELTA_MIN and min(scores) > SCORE_MIN
        else:
            assert all(s == 1.0 for s in scores) and max(mean_T) < 1.0 and torch.equal(res["fwd"], plain["fwd"])
        meta["sets"][name] = {"weight": weight, "scores": scores, "mean_T": mean_T, "bf16_spread": spread, "delta": deltas}
        T[f"enhance.{name}.fwd.out"] = res["fwd"]
        T[f"enhance.{name}.fwd.scores"] = torch.tensor(scores, dtype=torch.float32)
        for w in WEIGHTS:
            T[f"enhance.{name}.gen.{w}.final"] = res[f"gen.{w}"]
    out = os.path.join(GOLD, "dit_tiny_enhance.safetensors")
    save_file({k: v.float().contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_enhance_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
