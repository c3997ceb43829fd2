"""The forecast cache on the host: the two passes of include/k5.h (k5_forecast_update_bf16 / k5_forecast_apply_bf16) in torch with the stated
rounding points, the oracle's DiT forward split at the visual blocks out of the oracle's public pieces with the rule around them, and the
sampler loops that the golden generator (tools/gen_golden_forecast.py) and the parity tests share.  No GPU, no engine.

The rule, per branch slot: a full call at step i keeps r = vis_out - vis_in and, against the slot's last full call at step j with g = i - j,
d1 = (r - F0) / g (from the second full call on) and d2 = (d1 - D1) / g (from the third); a forecast call at step i, k = i - j, adds
F0 + k D1 + c2 D2 with m = min(order, have - 1) terms instead of running the blocks, c2 = k (k + g) g / (g + gp) with g, gp the slot's last two
gaps between full calls (Newton's backward form: exact for a quadratic in the step).  Every operation is one fp32 operation."""
import numpy as np
import torch

from oracle import k5_oracle as O

BF = torch.bfloat16


def bf(t):
    return t.to(BF).float()


def plan(num_steps, interval, warmup, tail):
    """generation_utils.forecast_plan, restated"""
    return [1 if i < warmup or i >= num_steps - tail or (i - warmup) % interval == 0 else 0 for i in range(num_steps)]


# ------------------------------------------------------------------------------------------ the two passes on tensors
def update_ref(vis, ori, F0, D1, D2, g, order, have):
    """(F0', D1', D2') of k5_forecast_update_bf16: vis, ori, F0 bf16, D1, D2 fp32 (None where the level does not reach); what the level does not
    write comes back as it went in."""
    r = (vis.float() + (-1.0) * ori.float()).to(BF)
    level = min(order, have)
    gf = torch.tensor(np.float32(g))
    if level >= 1:
        d1 = (r.float() - F0.float()) / gf
        if level >= 2:
            D2 = (d1 - D1) / gf
        D1 = d1
    return r, D1, D2


def c2_of(k, g, gp):
    return torch.tensor(np.float32(float(k) * float(k + g) * float(g) / float(g + gp)))


def apply_ref(vis, F0, D1, D2, k, order, have, g=1, gp=1):
    """vis' of k5_forecast_apply_bf16"""
    m = min(order, have - 1)
    p = F0.float()
    if m >= 1:
        p = p + torch.tensor(np.float32(k)) * D1
    if m >= 2:
        p = p + c2_of(k, g, gp) * D2
    return (vis.float() + p).to(BF)


# ------------------------------------------------------------------------------------------ the rule as state around any blocks
class Cache:
    """The state of one run: per slot F0, D1, D2, j, have.  mode "bf16": r is rounded to bf16 and so is the forecast sum (the engine);
    "fp32": nothing is rounded (the golden)."""

    def __init__(self, order, full, mode):
        self.order, self.full, self.mode = int(order), [int(v) for v in full], mode
        self.slots = [dict(F0=None, D1=None, D2=None, j=-1, have=0, g=1, gp=1) for _ in range(2)]
        self.full_calls = self.forecast_calls = 0

    def around(self, vis, blocks, step, slot):
        """the visual stream after the blocks of call (step, slot): `blocks(vis)` on a full call, the extrapolation on a forecast call"""
        s = self.slots[slot]
        if self.full[step]:
            out = blocks(vis)
            r = O._r(out + (-1.0) * vis, self.mode)
            gap = step - s["j"] if s["have"] else 1
            g = torch.tensor(np.float32(gap))
            s["gp"], s["g"] = s["g"], gap
            if s["have"] >= 1 and self.order >= 1:
                d1 = (r - s["F0"]) / g
                if s["have"] >= 2 and self.order >= 2:
                    s["D2"] = (d1 - s["D1"]) / g
                s["D1"] = d1
            s["F0"], s["j"], s["have"] = r, step, s["have"] + 1
            self.full_calls += 1
            return out
        assert s["have"] >= 1 and step > s["j"]
        k, m = step - s["j"], min(self.order, s["have"] - 1)
        p = s["F0"]
        if m >= 1:
            p = p + torch.tensor(np.float32(k)) * s["D1"]
        if m >= 2:
            p = p + c2_of(k, s["g"], s["gp"]) * s["D2"]
        self.forecast_calls += 1
        return O._r(vis + p, self.mode)


def dit_forward_forecast(sd, cfg, x, text_embed, pooled_text_embed, time, visual_rope_pos, text_rope_pos, scale_factor=(1.0, 1.0, 1.0),
                         sparse_params=None, mode="fp32", cache=None, step=0, slot=0):
    """O.dit_forward split at the visual blocks, the rule of `cache` around them (cache None: O.dit_forward, the same ops in the same order)"""
    with torch.no_grad():
        text = O.text_embeddings(sd, "text_embeddings", text_embed.float(), mode)
        temb = O.time_embeddings(sd, time, cfg)
        temb = temb + O.text_embeddings(sd, "pooled_text_embeddings", pooled_text_embed.float(), mode)
        vis = O.visual_embeddings(sd, x, cfg, mode)
        ta = O.rope_1d_args(text_rope_pos, cfg.head_dim)
        tcos, tsin = torch.cos(ta), torch.sin(ta)
        for i in range(cfg.num_text_blocks):
            text = O.encoder_block(sd, f"text_transformer_blocks.{i}", text, temb, tcos, tsin, cfg, mode)
        Tp, Hp, Wp, D = vis.shape
        va = O.rope_3d_args((Tp, Hp, Wp), visual_rope_pos, cfg.axes_dims, scale_factor)
        vcos, vsin = torch.cos(va).reshape(-1, va.shape[-1]), torch.sin(va).reshape(-1, va.shape[-1])
        vis = vis.reshape(-1, D)
        to_fractal = sparse_params is not None and sparse_params.get("to_fractal", False)
        if to_fractal:
            perm = O.fractal_perm((Tp, Hp, Wp))
            vis, vcos, vsin = vis[perm], vcos[perm], vsin[perm]

        def blocks(v):
            for i in range(cfg.num_visual_blocks):
                v = O.decoder_block(sd, f"visual_transformer_blocks.{i}", v, text, temb, vcos, vsin, cfg, mode, sparse_params)
            return v
        vis = blocks(vis) if cache is None else cache.around(vis, blocks, step, slot)
        if to_fractal:
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(perm.numel())
            vis = vis[inv]
        o = O.out_layer(sd, vis, temb, cfg, mode)
        return O.unpatchify(o.reshape(Tp, Hp, Wp, -1), cfg.patch_size)


# ------------------------------------------------------------------------------------------ sampler loops; velocity(x, sigma_i, step, slot)
def is_guided(w):
    return abs(float(w) - 1.0) > 1e-6


def published_loop(velocity, noise, sig, w):
    """the Euler / CFG loop in the arithmetic of the callable (the golden: the reference's fp32 DiT)"""
    x = noise.clone()
    for i in range(len(sig) - 1):
        c = velocity(x, sig[i], i, 0)
        v = c
        if is_guided(w):
            u = velocity(x, sig[i], i, 1)
            v = u + w * (c - u)
        x = x + (sig[i + 1] - sig[i]) * v
    return x


def bf16_loop(velocity, noise, sig, w):
    """the engine's loop on the host: bf16 velocities stored as fp32, the reference's eager bf16 combine, the update's rounding points"""
    x = noise.clone().float()
    for i in range(len(sig) - 1):
        c = velocity(x, sig[i], i, 0)
        v = c
        if is_guided(w):
            u = velocity(x, sig[i], i, 1)
            v = bf(u + bf(float(w) * bf(c - u)))
        x = x + bf((sig[i + 1] - sig[i]) * v)
    return x
