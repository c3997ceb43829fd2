"""The guidance rule of k5_guidance_coeffs_bf16 / k5_guided_euler, written twice on the host: from the five sums, as the kernel forms it
(numpy float64), and in the published tensor forms — CFG-Zero* (Fan et al. 2025: the projected scale `st_star`, zero-init of the first
steps) and CFG rescale (Lin et al. 2024, as diffusers' `rescale_noise_cfg`, std by torch.std) — plus the sampler loops built on them that
the golden generator (tools/gen_golden_guidance.py) and the parity tests share.  No GPU, no engine."""
import numpy as np
import torch


def is_guided(w):
    return abs(float(w) - 1.0) > 1e-6


# ------------------------------------------------------------------------------------------ the kernel's form: five sums -> (alpha, beta)
def five_sums(c, u):
    """(Sc, Su, Scc, Suu, Scu) of two tensors, float64"""
    c, u = c.detach().double().reshape(-1), u.detach().double().reshape(-1)
    return np.array([c.sum().item(), u.sum().item(), (c * c).sum().item(), (u * u).sum().item(), (c * u).sum().item()], dtype=np.float64)


def coeffs_from_sums(sums, n, w, zero_star, rescale):
    """(alpha, beta) in float64 of v = alpha c + beta u, the rule of include/k5.h"""
    Sc, Su, Scc, Suu, Scu = (np.float64(v) for v in sums)
    n, w, phi = np.float64(n), np.float64(np.float32(w)), np.float64(np.float32(rescale))
    s = Scu / (Suu + np.float64(1e-8)) if zero_star else np.float64(1.0)
    alpha, beta = w, s * (1.0 - w)
    if phi > 0:
        var_c = Scc - Sc * Sc / n
        var_v = alpha * alpha * var_c + 2.0 * alpha * beta * (Scu - Sc * Su / n) + beta * beta * (Suu - Su * Su / n)
        k = phi * np.sqrt(var_c / var_v) + (1.0 - phi) if (var_v > 0 and var_c >= 0) else np.float64(1.0)
        alpha, beta = alpha * k, beta * k
    return np.float64(alpha), np.float64(beta)


def ulp_distance_f32(a, b):
    """how many fp32 values apart two finite floats are (0: equal after rounding to fp32)"""
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    ia, ib = (i if i >= 0 else -(i & 0x7fffffff) for i in (ia, ib))
    return abs(ia - ib)


# ------------------------------------------------------------------------------------------ the published tensor forms
def st_star(c, u):
    """CFG-Zero*'s optimised scale of one sample: <c, u> / (<u, u> + 1e-8) over the flattened tensors"""
    c, u = c.reshape(1, -1), u.reshape(1, -1)
    dot = torch.sum(c * u, dim=1, keepdim=True)
    sq = torch.sum(u ** 2, dim=1, keepdim=True) + 1e-8
    return (dot / sq).reshape(())


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale):
    """diffusers' rescale_noise_cfg on one sample: std over every dimension of the sample, torch.std"""
    std_text = noise_pred_text.std()
    std_cfg = noise_cfg.std()
    rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * rescaled + (1 - guidance_rescale) * noise_cfg


def guided_velocity(c, u, w, zero_star, rescale):
    """the guided velocity of one sample in the published forms, in the dtype of c / u"""
    if zero_star:
        s = st_star(c, u)
        v = u * s + w * (c - u * s)
    else:
        v = u + w * (c - u)
    if rescale > 0:
        v = rescale_noise_cfg(v, c, rescale)
    return v


# ------------------------------------------------------------------------------------------ sampler loops
def published_loop(cond_velocity, uncond_velocity, noise, sig, weights, zero_star=False, zero_init=0, rescale=0.0):
    """The Euler loop with the rule in the published tensor forms, in the arithmetic of the callables (the golden: the reference's fp32 DiT).
    cond_velocity / uncond_velocity: (x, sigma_i) -> velocity; a step of weight 1 uses the conditional one alone, the first zero_init
    steps have velocity 0."""
    x = noise.clone()
    for i in range(len(sig) - 1):
        if i < zero_init:
            continue
        c = cond_velocity(x, sig[i])
        v = guided_velocity(c, uncond_velocity(x, sig[i]), weights[i], zero_star, rescale) if is_guided(weights[i]) else c
        x = x + (sig[i + 1] - sig[i]) * v
    return x


def bf16_loop(cond_velocity, uncond_velocity, noise, sig, weights, zero_star=False, zero_init=0, rescale=0.0):
    """The engine's loop on the host: bf16 velocities (stored as fp32), coefficients from the float64 sums rounded to fp32, the guided
    velocity and the update with the kernels' rounding points.  Without zero_star / rescale a guided step is the eager bf16 combine of the
    reference (u + w (c - u), every op rounded)."""
    def bf(t):
        return t.to(torch.bfloat16).float()

    x = noise.clone().float()
    for i in range(len(sig) - 1):
        if i < zero_init:
            continue
        c = cond_velocity(x, sig[i])
        w = float(weights[i])
        if not is_guided(w):
            v = c
        else:
            u = uncond_velocity(x, sig[i])
            if zero_star or rescale > 0:
                alpha, beta = (torch.tensor(np.float32(t)) for t in coeffs_from_sums(five_sums(c, u), c.numel(), w, zero_star, rescale))
                v = bf(alpha * c + beta * u)
            else:
                v = bf(u + bf(w * bf(c - u)))
        x = x + bf((sig[i + 1] - sig[i]) * v)
    return x
