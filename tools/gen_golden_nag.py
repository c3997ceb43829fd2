"""Golden vectors for normalized attention guidance (NAG): the reference's fp32 DiT with the rule of include/k5.h (k5_nag_combine_bf16)
applied in float32 around its own cross-attention modules.

Run once where the reference tree is present:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_nag.py

Writes tests/golden/dit_tiny_nag.safetensors + dit_tiny_nag_meta.json (data only).  The tiny DiT, inputs, noise and prompts of
dit_tiny.safetensors; the negative prompt is gen.null_text / gen.null_pooled with positions arange(4).  Per visual block, on the
conditional forward only:

    z+ = attention(q, k+, v+),  z- = attention(q, k-, v-)        the module's own get_qkv / norm_qk / attention, the same queries
    d = z+ - z-;  g = z+ + (s - 1) d;  n+ = sum|z+|, n_g = sum|g| per token over all channels
    f = 1 if n_g <= tau n+ else tau n+ / n_g;  out = z+ + alpha (f g - z+);  then the module's out_l

The negative tokens go through text_embeddings and the text blocks with their own RoPE positions and the forward's own time embedding
(the positive prompt's pooled embedding).  Two parameter sets: A with the clamp active on most tokens, B with it mostly idle.  For each:
one forward velocity (the fwd.* inputs) and the final latent of the 4-step loop at guidance 1 and 5 (scheduler_scale 5, gen.noise).
Asserted and recorded: the share of (block, token) pairs that were clamped (A >= 0.5, B <= 0.5, on every stored case) and delta, the
relative L2 of each result against the plain result of the same run (>= 0.04).  The starting values (5, 2.5, 0.25) / (1.5, 2.5, 0.5) are
moved within s in [1, 11], tau in [1, 4], alpha in (0, 1] until both hold; what was used is stored.
"""
import itertools
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
STEPS, SCALE, WEIGHTS, DELTA_MIN = 4, 5.0, (1.0, 5.0), 0.04
START = {"A": (5.0, 2.5, 0.25), "B": (1.5, 2.5, 0.5)}


def nag_combine(zp, zn, s, tau, alpha):
    """the definition, float32; returns (out, clamped rows)"""
    d = zp - zn
    g = zp + (s - 1.0) * d
    n_pos, n_g = zp.abs().sum(-1, keepdim=True), g.abs().sum(-1, keepdim=True)
    clamped = n_g > tau * n_pos
    f = torch.where(clamped, tau * n_pos / torch.where(clamped, n_g, torch.ones_like(n_g)), torch.ones_like(n_g))
    return zp + alpha * (f * g - zp), clamped.squeeze(-1)


class Nag:
    """NAG on a reference DiT: while `params` is set, a forward whose text tokens are `positive` attends every visual block to the
    negative stream as well.  Only the modules' own methods are called."""

    def __init__(self, dit, positive, neg_text, neg_pos):
        self.dit, self.positive, self.neg_text, self.neg_pos = dit, positive, neg_text, neg_pos
        self.params, self.active, self.busy, self.neg_stream = None, False, False, None
        self.rows = self.clamped = 0
        dit.register_forward_pre_hook(self.on_forward)
        dit.text_transformer_blocks[0].register_forward_pre_hook(self.on_first_text_block)
        for b in dit.visual_transformer_blocks:
            ca = b.cross_attention
            ca.forward = lambda x, cond, ca=ca: self.cross(ca, x, cond)

    def on_forward(self, module, args):
        self.active = self.params is not None and args[1] is self.positive   # the unconditional forward stays as it is
        self.neg_stream = None

    def on_first_text_block(self, module, args):
        if not self.active or self.busy:
            return
        time_embed = args[1]   # one per forward: the positive prompt's pooled embedding went into it
        self.busy = True
        neg = self.dit.text_embeddings(self.neg_text)
        rope = self.dit.text_rope_embeddings(self.neg_pos)
        for blk in self.dit.text_transformer_blocks:
            neg = blk(neg, time_embed, rope)
        self.busy = False
        self.neg_stream = neg

    def cross(self, ca, x, cond):
        q, k, v = ca.get_qkv(x, cond)
        q, k = ca.norm_qk(q, k)
        zp = ca.attention(q, k, v)
        if self.active:
            _, kn, vn = ca.get_qkv(x, self.neg_stream)
            _, kn = ca.norm_qk(q, kn)          # q is normalised already and not used again
            zn = ca.attention(q, kn, vn)
            zp, cl = nag_combine(zp.float(), zn.float(), *self.params)
            self.rows += cl.numel()
            self.clamped += int(cl.sum())
        return ca.out_l(zp)


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
    nag = Nag(dit, te["text_embeds"], ne["text_embeds"], torch.arange(4))

    def run_all(params):
        """{case: (result, clamped share)} with NAG `params` (None = plain)"""
        out = {}
        nag.params = params
        with torch.no_grad():
            nag.rows = nag.clamped = 0
            v = dit(g["fwd.x"], te["text_embeds"], te["pooled_embed"], g["fwd.time"], pos, torch.arange(7), scale_factor=(1.0, 2.0, 2.0))
            out["fwd"] = (v, nag.clamped / max(nag.rows, 1))
            for w in WEIGHTS:
                nag.rows = nag.clamped = 0
                x = r.gen.generate(dit, "cpu", tuple(g["gen.noise"].shape), STEPS, te, ne, pos, torch.arange(7), torch.arange(4), w, SCALE,
                                   conf, seed=gmeta["gen_seed"])
                out[f"gen.{w}"] = (x, nag.clamped / max(nag.rows, 1))
        nag.params = None
        return out

    plain = run_all(None)
    # the hooks are idle without parameters: the plain runs are the goldens of dit_tiny.safetensors
    assert torch.equal(plain["fwd"][0], g["fwd.out"])
    for w in WEIGHTS:
        assert torch.equal(plain[f"gen.{w}"][0], g[f"gen.{STEPS}_{SCALE}_{w}.final"])

    def ok(name, res):
        shares = [c for _, c in res.values()]
        deltas = [rel(res[k][0], plain[k][0]) for k in res]
        share_ok = all(c >= 0.5 for c in shares) if name == "A" else all(c <= 0.5 for c in shares)
        return share_ok and min(deltas) >= DELTA_MIN, shares, deltas

    def candidates(name):
        yield START[name]
        s0, t0, a0 = START[name]
        scales = [5.0, 7.0, 9.0, 11.0, 3.0] if name == "A" else [1.5, 2.0, 2.5, 3.0, 4.0, 1.25]
        taus = [2.5, 2.0, 1.5, 1.25, 1.0] if name == "A" else [2.5, 3.0, 4.0]
        alphas = [a0, 0.5, 0.75, 1.0]
        for a, s, t in itertools.product(alphas, scales, taus):   # alpha last to move: the smallest change first
            if (s, t, a) != START[name]:
                yield (s, t, a)

    T, meta = {}, {"steps": STEPS, "scheduler_scale": SCALE, "weights": list(WEIGHTS), "delta_min": DELTA_MIN,
                   "negative": "dit_tiny.safetensors gen.null_text, positions arange(4)", "rope_pos": {"dense": [3, 4, 6], "text": 7, "neg_text": 4},
                   "sets": {}}
    for name in ("A", "B"):
        best = None
        for params in candidates(name):
            res = run_all(params)
            good, shares, deltas = ok(name, res)
            print(name, params, "clamped", [round(c, 3) for c in shares], "delta", [round(d, 4) for d in deltas], "ok" if good else "")
            share_ok = all(c >= 0.5 for c in shares) if name == "A" else all(c <= 0.5 for c in shares)
            if share_ok and (best is None or min(deltas) > min(best[3])):
                best = (params, res, shares, deltas)
            if good:
                break
        assert best is not None, f"set {name}: no parameters with the clamped share on the right side of 0.5"
        params, res, shares, deltas = best
        reached = min(deltas) >= DELTA_MIN
        if not reached:
            print(f"set {name}: delta >= {DELTA_MIN} not reached on the tiny weights; storing the largest found, {min(deltas):.4f}")
        keys = list(res)
        meta["sets"][name] = {"scale": params[0], "tau": params[1], "alpha": params[2], "delta_reached": reached,
                              "clamped_share": dict(zip(keys, shares)), "delta": dict(zip(keys, deltas))}
        T[f"nag.{name}.fwd.out"] = res["fwd"][0]
        for w in WEIGHTS:
            T[f"nag.{name}.gen.{w}.final"] = res[f"gen.{w}"][0]
    out = os.path.join(GOLD, "dit_tiny_nag.safetensors")
    save_file({k: v.float().contiguous() for k, v in T.items()}, out)
    with open(os.path.join(GOLD, "dit_tiny_nag_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("golden written:", out, f"{os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
