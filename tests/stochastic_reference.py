"""Stochastic sampling on the host: Philox4x32-10 restated in NumPy, its Box-Muller normals and the per-step rule in float64, the update of
k5_stochastic_euler in torch eager with separate fp32 ops, and the sampler loops that the golden generator
(tools/gen_golden_stochastic.py) and the parity tests share.  No GPU, no engine.

The rule (flow matching, x_sigma = (1 - sigma) x0 + sigma eps; step i from s = sigmas[i] to t = sigmas[i + 1], churn eta, noise scale s_noise):
    sigma_down = t (1 + (t / s - 1) eta)      a = (1 - t) / (1 - sigma_down)      c = s_noise sqrt(max(0, t^2 - (sigma_down a)^2))
    x1 = x + (sigma_down - s) v               x2 = a x1 + c z,  z ~ N(0, 1)       (only where c != 0)
The generator: key = (low, high word of the seed), counter = (low, high word of the block index g >> 2, stream id, 0); element g takes normal
g & 3 of its block; step i of a run draws from stream first_stream + i."""
import math

import numpy as np
import torch

import guidance_reference as R

BF = torch.bfloat16
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ the generator
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """(r0, r1, r2, r3) uint64 arrays holding 32-bit words: ten rounds on uint64 arithmetic masked to 32 bits.  The counter and key words are
    arrays (or scalars) that broadcast."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def philox_words(blk0, nblk, seed, c2=0, c3=0):
    """uint32 [nblk][4]: the words of blocks blk0 .. blk0 + nblk - 1 (mod 2^64), as k5_philox_words lays them out"""
    blk = [(int(blk0) + i) & (2 ** 64 - 1) for i in range(int(nblk))]
    lo = np.array([b & 0xFFFFFFFF for b in blk], dtype=np.uint64)
    hi = np.array([b >> 32 for b in blk], dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    r = philox4x32_10(lo, hi, np.uint64(int(c2) & 0xFFFFFFFF), np.uint64(int(c3) & 0xFFFFFFFF), np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    return np.stack([np.broadcast_to(w, lo.shape) for w in r], axis=1).astype(np.uint32)


def normals_f64(n, seed, stream_id=0):
    """float64 [n]: element g = normal g & 3 of block g >> 2 — u_j = ((r_j >> 9) + 0.5) 2^-23, (z0, z1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1),
    (z2, z3) from (u2, u3) likewise"""
    nblk = (int(n) + 3) // 4
    r = philox_words(0, nblk, seed, stream_id, 0).astype(np.float64)
    u = (np.floor(r / 512.0) + 0.5) * 2.0 ** -23
    z = np.empty((nblk, 4), dtype=np.float64)
    for j in (0, 2):
        rad = np.sqrt(-2.0 * np.log(u[:, j]))
        ang = 2.0 * np.pi * u[:, j + 1]
        z[:, j], z[:, j + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return z.reshape(-1)[:int(n)]


def normals_f32(shape, seed, stream_id=0):
    """the float64 normals rounded once to fp32, as a torch tensor of `shape`"""
    n = int(np.prod(shape))
    return torch.from_numpy(normals_f64(n, seed, stream_id).astype(np.float32)).reshape(shape)


# ------------------------------------------------------------------------------------------ the per-step rule, float64
def plan_f64(sig, eta, s_noise=1.0, interval=None):
    """[(sigma_down, a, c)] per step in float64; a step that is not stochastic has (t, 1, 0)"""
    sig = [float(v) for v in sig]
    lo, hi = (-math.inf, math.inf) if interval is None else (float(interval[0]), float(interval[1]))
    out = []
    for i in range(len(sig) - 1):
        s, t = sig[i], sig[i + 1]
        if eta > 0.0 and lo <= s <= hi:
            down = t * (1.0 + (t / s - 1.0) * eta)
            a = (1.0 - t) / (1.0 - down)
            c = s_noise * math.sqrt(max(0.0, t * t - (down * a) ** 2))
            if c != 0.0:
                out.append((down, a, c))
                continue
        out.append((t, 1.0, 0.0))
    return out


def tables_f32(sig, eta, s_noise=1.0, interval=None):
    """(dt_down, scale, noise_coef) as lists of fp32 values: what generation_utils.stochastic_plan must return.  A step without noise has the
    fp32 difference of the fp32 sigmas as dt_down, scale 1, coefficient 0."""
    f = np.asarray([float(v) for v in sig], dtype=np.float32)
    dt, sc, co = [], [], []
    for i, (down, a, c) in enumerate(plan_f64(sig, eta, s_noise, interval)):
        if np.float32(c) == 0.0:
            row = (float(f[i + 1] - f[i]), 1.0, 0.0)
        else:
            row = (float(np.float32(down - float(sig[i]))), float(np.float32(a)), float(np.float32(c)))
        for table, value in zip((dt, sc, co), row):
            table.append(value)
    return dt, sc, co


# ------------------------------------------------------------------------------------------ the update, torch eager
def bf(t):
    return t.to(BF).float()


def f32(x):
    return float(np.float32(x))


def velocity(c, u, s, w, g, ab):
    """the step's velocity (a bf16 tensor) with the kernels' rounding points: c, u (None: no guidance), s (None: no skip term) bf16 tensors"""
    if ab is not None:
        v = (f32(ab[0]) * c.float() + f32(ab[1]) * u.float()).to(BF)
    elif u is not None:
        v = (u.float() + (f32(w) * (c.float() - u.float()).to(BF).float()).to(BF).float()).to(BF)
    else:
        v = c
    if s is not None:
        d = (c.float() - s.float()).to(BF)
        e = (f32(g) * d.float()).to(BF)
        v = (v.float() + e.float()).to(BF)
    return v


def stochastic_update(img, c, u, s, w, g, dt_down, scale, noise_coef, z, ab=None, source=None, eps=None, keep_mask=None, sigma_next=0.0):
    """(img', v) of k5_stochastic_euler, every fp32 op on its own: x1 = img + bf16(dt_down v); x2 = scale x1 + noise_coef z where
    noise_coef != 0; then the keep rule as the editing tests spell it (keep_mask per element)"""
    v = velocity(c, u, s, w, g, ab)
    x = img + (f32(dt_down) * v.float()).to(BF).float()
    if f32(noise_coef) != 0.0:
        p = f32(scale) * x
        q = f32(noise_coef) * z
        x = p + q
    if keep_mask is not None:
        known = f32(np.float32(1.0) - np.float32(sigma_next)) * source + f32(sigma_next) * eps
        m = keep_mask
        blend = x + m * (known - x)
        x = torch.where(m == 1.0, known, torch.where(m == 0.0, x, blend))
    return x, v


# ------------------------------------------------------------------------------------------ sampler loops
def step_noise(shape, seed, first_stream=0):
    """i -> the fp32 noise of step i: the float64 restatement rounded to fp32"""
    return lambda i: normals_f32(shape, seed, first_stream + i)


def published_loop(cond_velocity, uncond_velocity, skip_velocity, noise, sig, weights, plan, z_at, g=0.0, mask=None, zero_star=False,
                   zero_init=0, rescale=0.0):
    """The rule in the arithmetic of the callables ((x, sigma_i) -> velocity): `plan` is plan_f64's list, z_at(i) the step's noise"""
    x = noise.clone()
    for i in range(len(sig) - 1):
        if i < zero_init:
            continue
        c = cond_velocity(x, sig[i])
        s = skip_velocity(x, sig[i]) if mask is not None and mask[i] else None
        v = R.guided_velocity(c, uncond_velocity(x, sig[i]), weights[i], zero_star, rescale) if R.is_guided(weights[i]) else c
        if s is not None:
            v = v + g * (c - s)
        down, a, cf = plan[i]
        x = x + (down - float(sig[i])) * v
        if cf != 0.0:
            x = a * x + cf * z_at(i)
    return x


def bf16_loop(cond_velocity, uncond_velocity, skip_velocity, noise, sig, weights, tables, z_at, g=0.0, mask=None, zero_star=False, zero_init=0,
              rescale=0.0):
    """The engine's loop on the host: bf16 velocities stored as fp32, the kernel's rounding points; `tables` = tables_f32's three lists"""
    x = noise.clone().float()
    gf = f32(g)
    dt_down, scale, coef = tables
    for i in range(len(sig) - 1):
        if i < zero_init:
            continue
        c = cond_velocity(x, sig[i])
        s = skip_velocity(x, sig[i]) if mask is not None and mask[i] else None
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
        x = x + bf(f32(dt_down[i]) * v)
        if coef[i] != 0.0:
            p = f32(scale[i]) * x
            q = f32(coef[i]) * z_at(i)
            x = p + q
    return x
