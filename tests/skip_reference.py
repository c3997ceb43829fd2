"""Skip-layer guidance on the host: the oracle's DiT forward restated with a skip set out of the oracle's public pieces, the three-velocity
update of k5_skip_euler in torch eager, and the sampler loops that the golden generator (tools/gen_golden_skip.py) and the parity tests
share.  No GPU, no engine.

The rule: v = v_cfg + g (c - c_skip), c_skip the conditional velocity with the listed visual blocks skipped — mode "block": the block is
the identity on the visual stream; mode "attention": only its self-attention residual is dropped, its cross-attention and feed-forward
run.  v_cfg is what the step would otherwise use (tests/guidance_reference.py: CFG, CFG-Zero* / rescale, or c alone at guidance 1); a
plan's statistics are over c and u, the skip term is added after them."""
import numpy as np
import torch

from oracle import k5_oracle as O

import guidance_reference as R

BF = torch.bfloat16
TINY4 = dict(num_visual_blocks=4)       # the shipped tiny weights have two blocks: too few for a prefix, a skipped block and a suffix at once
WEIGHT_SEED = 11


def tiny4_config(tiny_config):
    """the tests' model: the tiny config with four visual blocks, as keyword arguments"""
    c = dict(tiny_config, **TINY4)
    c["patch_size"], c["axes_dims"] = tuple(c["patch_size"]), tuple(c["axes_dims"])
    return c


def tiny4_weights(cfg, seed=WEIGHT_SEED):
    return O.synthetic_state_dict(O.DitConfig(**cfg), seed)


def weights_sha256(sd):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------ the forward with a skip set
def decoder_block_without_self_attention(sd, p, x, text, temb, cfg, mode):
    """O.decoder_block minus its self-attention residual (and the LayerNorm in front of it)"""
    mod = O.modulation(sd, f"{p}.visual_modulation", temb)
    _, ca, ff = torch.chunk(mod, 3, dim=-1)
    shift, scale, gate = torch.chunk(ca, 3, dim=-1)
    out = O.scale_shift_norm(x, scale, shift, mode)
    out = O.cross_attention(sd, f"{p}.cross_attention", out, text, cfg, mode)
    x = O.gate_sum(x, out, gate, mode)
    shift, scale, gate = torch.chunk(ff, 3, dim=-1)
    out = O.scale_shift_norm(x, scale, shift, mode)
    out = O.feed_forward(sd, f"{p}.feed_forward", out, mode)
    return O.gate_sum(x, out, gate, mode)


def dit_forward_skip(sd, cfg, x, text_embed, pooled_text_embed, time, visual_rope_pos, text_rope_pos, scale_factor=(1.0, 1.0, 1.0),
                     sparse_params=None, mode="fp32", skip=(), skip_mode="block"):
    """O.dit_forward with the visual blocks `skip` skipped (an empty set: O.dit_forward, the same ops in the same order)"""
    assert skip_mode in ("block", "attention")
    skip = set(int(b) for b in skip)
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
        for i in range(cfg.num_visual_blocks):
            p = f"visual_transformer_blocks.{i}"
            if i not in skip:
                vis = O.decoder_block(sd, p, vis, text, temb, vcos, vsin, cfg, mode, sparse_params)
            elif skip_mode == "attention":
                vis = decoder_block_without_self_attention(sd, p, vis, text, temb, cfg, mode)
        if to_fractal:
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(perm.numel())
            vis = vis[inv]
        o = O.out_layer(sd, vis, temb, cfg, mode)
        return O.unpatchify(o.reshape(Tp, Hp, Wp, -1), cfg.patch_size)


# ------------------------------------------------------------------------------------------ the update, torch eager on bf16 tensors
def bf(t):
    return t.to(BF).float()


def skip_update(img, c, u, s, w, g, dt, ab=None, source=None, noise=None, keep_mask=None, sigma_next=0.0):
    """(img', v) of k5_skip_euler: c, u (None: no guidance), s bf16 tensors; ab (alpha, beta) as fp32 numbers or None; the keep rule as the
    editing tests spell it, each op rounded to fp32 on its own"""
    f32 = lambda t: float(np.float32(t))   # noqa: E731
    if ab is not None:
        base = (f32(ab[0]) * c.float() + f32(ab[1]) * u.float()).to(BF)     # two fp32 products, one fp32 sum, then bf16
    elif u is not None:
        base = (u.float() + (f32(w) * (c.float() - u.float()).to(BF).float()).to(BF).float()).to(BF)
    else:
        base = c
    # the eager expression `base + g * (c - s)` on bf16 tensors, each of its three ops spelt out in fp32 and rounded to bf16 (on the GPU the
    # literal expression gives these bits; on the CPU torch rounds a scalar factor to bf16 first, so it is not used here)
    d = (c.float() - s.float()).to(BF)
    e = (f32(g) * d.float()).to(BF)
    v = (base.float() + e.float()).to(BF)
    x = img + (f32(dt) * v.float()).to(BF).float()
    if keep_mask is not None:
        known = f32(np.float32(1.0) - np.float32(sigma_next)) * source + f32(sigma_next) * noise
        m = keep_mask
        blend = x + m * (known - x)
        x = torch.where(m == 1.0, known, torch.where(m == 0.0, x, blend))
    return x, v


# ------------------------------------------------------------------------------------------ sampler loops
def published_loop(cond_velocity, uncond_velocity, skip_velocity, noise, sig, weights, g, mask, zero_star=False, zero_init=0, rescale=0.0):
    """tests/guidance_reference.py's published_loop with the skip term: on the steps of `mask` v = v_cfg + g (c - c_skip), in the arithmetic of
    the callables ((x, sigma_i) -> velocity)"""
    x = noise.clone()
    for i in range(len(sig) - 1):
        if i < zero_init:
            continue
        c = cond_velocity(x, sig[i])
        s = skip_velocity(x, sig[i]) if mask[i] else None
        v = R.guided_velocity(c, uncond_velocity(x, sig[i]), weights[i], zero_star, rescale) if R.is_guided(weights[i]) else c
        if s is not None:
            v = v + g * (c - s)
        x = x + (sig[i + 1] - sig[i]) * v
    return x


def bf16_loop(cond_velocity, uncond_velocity, skip_velocity, noise, sig, weights, g, mask, zero_star=False, zero_init=0, rescale=0.0):
    """The engine's loop on the host, as tests/guidance_reference.py's bf16_loop: bf16 velocities stored as fp32, the skip term with the
    kernel's rounding points (d = bf16(c - s), e = bf16(g d), v = bf16(base + e))"""
    x = noise.clone().float()
    gf = float(np.float32(g))
    for i in range(len(sig) - 1):
        if i < zero_init:
            continue
        c = cond_velocity(x, sig[i])
        s = skip_velocity(x, sig[i]) if mask[i] else None
        w = float(weights[i])
        if not R.is_guided(w):
            v = c
        else:
            u = uncond_velocity(x, sig[i])
            if zero_star or rescale > 0:
                alpha, beta = (torch.tensor(np.float32(t)) for t in R.coeffs_from_sums(R.five_sums(c, u), c.numel(), w, zero_star, rescale))
                v = bf(alpha * c + beta * u)
            else:
                v = bf(u + bf(w * bf(c - u)))
        if s is not None:
            v = bf(v + bf(gf * bf(c - s)))
        x = x + bf((sig[i + 1] - sig[i]) * v)
    return x
