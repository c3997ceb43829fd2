"""The sampler's update of one step (k5_euler_step, `E.euler_step_`) on the host, in torch eager with every fp32 / bf16 op rounded on its own:
the CFG combine, the coefficients `ab`, the skip term, the noise term (a given `z`, or the generator restated in stochastic_reference) and the
keep rule.  The one CPU stand-in the host tests patch over `E.euler_step_`, next to those for `E.renoise` and `E.guidance_coeffs`, so that
`generate`'s per-step loop runs without a GPU.  No GPU, no engine."""
import numpy as np
import torch

import guidance_reference as R
import stochastic_reference as SR

BF = torch.bfloat16


def bf(t):
    return t.to(BF).float()


def f32(x):
    return float(np.float32(float(x)))


def renoise(source, noise, sigma, out=None):
    """k5_edit_renoise: rn(rn((1 - sigma) source) + rn(sigma noise)), 1 - sigma formed in fp32"""
    known = f32(np.float32(1.0) - np.float32(sigma)) * source + f32(sigma) * noise
    return known if out is None else out.copy_(known)


def guidance_coeffs(v_cond, v_uncond, w, zero_star=False, rescale=0.0, ab=None, sums=None):
    """(ab, sums) as `E.guidance_coeffs` returns them, from guidance_reference's float64 sums and rule"""
    s = R.five_sums(v_cond.float(), v_uncond.float())
    return torch.tensor([np.float32(t) for t in R.coeffs_from_sums(s, v_cond.numel(), w, zero_star, rescale)]), torch.from_numpy(s)


def euler_step_(img, v_cond, v_uncond=None, *, w=1.0, dt, ab=None, v_skip=None, g=0.0, source=None, noise=None, keep_mask=None, sigma_next=0.0,
                v_out=None, stochastic=None):
    """`E.euler_step_` on CPU tensors, in place on img: the rule of k5_euler_step_args (include/k5.h), one line per rounding point"""
    c = v_cond.float()
    if ab is not None:
        v = bf(f32(ab[0]) * c + f32(ab[1]) * v_uncond.float())
    elif v_uncond is not None:
        u = v_uncond.float()
        v = bf(u + bf(f32(w) * bf(c - u)))
    else:
        v = c
    if v_skip is not None:
        v = bf(v + bf(f32(g) * bf(c - v_skip.float())))
    x = img + bf(f32(dt) * v)
    if stochastic is not None:
        scale, noise_coef, seed, stream_id, *z = stochastic
        if f32(noise_coef) != 0.0:
            z = z[0] if z and z[0] is not None else SR.normals_f32(tuple(img.shape), seed, stream_id)
            p = f32(scale) * x
            q = f32(noise_coef) * z
            x = p + q
    if keep_mask is not None:
        known = renoise(source, noise, sigma_next)
        blend = x + keep_mask * (known - x)
        x = torch.where(keep_mask == 1.0, known, torch.where(keep_mask == 0.0, x, blend))
    if v_out is not None:
        v_out.copy_(v)   # v holds bf16 values: exact
    return img.copy_(x)
