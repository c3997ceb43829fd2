"""FlowEdit on the host (Kulikov et al. 2024, "FlowEdit: Inversion-Free Text-Based Editing Using Pre-Trained Flow Models", Algorithm 1 with
n_avg = 1): the pass of k5_flowedit_step in torch eager with every fp32 / bf16 op rounded on its own, the engine's loop with the oracle's forwards
at the engine's rounding points (`bf16_loop`) and the paper's loop in the arithmetic of its callables with the rule in float64
(`published_loop`).  The golden generator (tools/gen_golden_flowedit.py) and the tests share them.  No GPU, no engine.

The rule (flow matching, x_sigma = (1 - sigma) x0 + sigma eps; N steps, first = edit_first_step(N, strength), R = refine; z_fe starts as x_src):
    a FlowEdit step first <= i < N - R, s = sigmas[i], dt = sigmas[i + 1] - s, z of (seed, stream i):
        zs = (1 - s) x_src + s z        zt = zs + (z_fe - x_src)
        v_s = CFG(c_s, u_s, w_src) on zs with the source / negative prompt,   v_t = CFG(c_t, u_t, w_tar) on zt with the target / negative prompt
        z_fe = z_fe + (1 - m) dt (v_t - v_s)                                    m: the keep mask, 0 without one
    refine: zt is formed at sigmas[N - R] with stream N - R, steps N - R .. N - 1 are plain CFG + Euler steps on it with the target prompt.
The noise comes from stochastic_reference.step_noise (the float64 restatement of the generator rounded to fp32)."""
import numpy as np
import torch

BF = torch.bfloat16


def bf(t):
    return t.to(BF).float()


def f32(x):
    return float(np.float32(float(x)))


def is_guided(w):
    return abs(float(w) - 1.0) > 1e-6


def plan(num_steps, strength, refine=0):
    """(first, number of FlowEdit steps, number of plain steps): run = min(num_steps, max(1, floor(num_steps strength + 0.5))) steps run, the
    tail of the schedule, as generation_utils.edit_first_step states it"""
    first = num_steps - min(num_steps, max(1, int(np.floor(num_steps * float(strength) + 0.5))))
    assert 0 <= refine <= num_steps - first
    return first, num_steps - first - refine, refine


SOURCE_TEXT_LEN = 5


def source_prompt(golden, seed=4711):
    """The source prompt of the golden cases: a seeded draw of SOURCE_TEXT_LEN text rows and a pooled row, scaled to the golden prompt's std.
    tools/gen_golden_flowedit.py stores it in the fixture; the parity test checks that it is this one."""
    g = torch.Generator().manual_seed(seed)
    text, pooled = golden["fwd.text"].float(), golden["fwd.pooled"].float()
    return {"text_embeds": (torch.randn(SOURCE_TEXT_LEN, text.shape[1], generator=g) * text.std()).to(golden["fwd.text"].dtype),
            "pooled_embed": (torch.randn(*pooled.shape, generator=g) * pooled.std()).to(golden["fwd.pooled"].dtype)}


def source_latent(shape, seed=77):
    """The source clip's latent of the golden cases: a seeded standard normal draw"""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------ the pass, torch eager
def cfg(c, u, w):
    """the CFG combine as k5_euler_step forms it: bf16 after the difference, the product and the sum; u None (weight 1): c itself"""
    if u is None:
        return c.float()
    c, u = c.float(), u.float()
    return bf(u + bf(f32(w) * bf(c - u)))


def renoise(x_src, z, sigma):
    """zs: k5_edit_renoise's bits with z as the noise"""
    p = f32(np.float32(1.0) - np.float32(sigma)) * x_src
    q = f32(sigma) * z
    return p + q


def target(zs, z_fe, x_src):
    """zt = zs + (z_fe - x_src), the difference first"""
    d = z_fe - x_src
    return zs + d


def update(z_fe, c_src, u_src, c_tar, u_tar, w_src, w_tar, dt, keep_mask=None):
    """z_fe after the update of one step; keep_mask broadcasts over the channels (one value per cell)"""
    d = bf(cfg(c_tar, u_tar, w_tar) - cfg(c_src, u_src, w_src))
    e = bf(f32(dt) * d)
    if keep_mask is None:
        return z_fe + e
    m = keep_mask.expand_as(z_fe)
    k = 1.0 - m
    ke = k * e
    return torch.where(m == 1.0, z_fe, torch.where(m == 0.0, z_fe + e, z_fe + ke))


def flowedit_pass(z_fe, x_src, vel=None, *, w_src=1.0, w_tar=1.0, dt=0.0, keep_mask=None, sigma_next=None, z=None):
    """(z_fe', zs, zt) of one k5_flowedit_step launch: vel = (c_src, u_src | None, c_tar, u_tar | None) finishes a step, sigma_next with the
    noise z prepares the next one (zs / zt None without)"""
    if vel is not None:
        z_fe = update(z_fe, vel[0], vel[1], vel[2], vel[3], w_src, w_tar, dt, keep_mask)
    if sigma_next is None:
        return z_fe, None, None
    zs = renoise(x_src, z, sigma_next)
    return z_fe, zs, target(zs, z_fe, x_src)


# ------------------------------------------------------------------------------------------ sampler loops
def bf16_loop(src_velocity, null_velocity, tar_velocity, x_src, sig, w_src, w_tar, z_at, first=0, refine=0, keep_mask=None):
    """The engine's loop on the host: the callables ((x, sigma_i) -> bf16 velocity stored as fp32 or bf16) at the kernel's rounding points.
    `sig` is the FULL schedule (N + 1 values), z_at(i) the noise of step i of the full schedule."""
    sig = [f32(s) for s in sig]
    N = len(sig) - 1
    fe_end = N - refine
    z_fe = x_src.clone().float()
    z_fe, zs, zt = flowedit_pass(z_fe, x_src, sigma_next=sig[first], z=z_at(first))
    for i in range(first, fe_end):
        s = torch.tensor(sig[i])
        vel = (src_velocity(zs, s), null_velocity(zs, s) if is_guided(w_src) else None,
               tar_velocity(zt, s), null_velocity(zt, s) if is_guided(w_tar) else None)
        nx = i + 1
        z_fe, zs, zt = flowedit_pass(z_fe, x_src, vel, w_src=w_src, w_tar=w_tar, dt=f32(np.float32(sig[nx]) - np.float32(sig[i])),
                                     keep_mask=keep_mask, sigma_next=sig[nx] if nx < N else None, z=z_at(nx) if nx < N else None)
    if refine == 0:
        return z_fe
    x = zt
    for i in range(fe_end, N):
        s = torch.tensor(sig[i])
        v = cfg(tar_velocity(x, s), null_velocity(x, s) if is_guided(w_tar) else None, w_tar)
        x = x + bf(f32(np.float32(sig[i + 1]) - np.float32(sig[i])) * v)
    return x


def published_loop(src_velocity, null_velocity, tar_velocity, x_src, sig, w_src, w_tar, z_at, first=0, refine=0, keep_mask=None):
    """Algorithm 1 in the arithmetic of the callables, the rule's scalars in float64"""
    sig = [float(s) for s in sig]
    N = len(sig) - 1
    fe_end = N - refine

    def guided(cond, x, s, w):
        c = cond(x, s)
        if not is_guided(w):
            return c
        u = null_velocity(x, s)
        return u + float(w) * (c - u)

    z_fe = x_src.clone()
    for i in range(first, fe_end):
        s = torch.tensor(sig[i])
        zs = (1.0 - sig[i]) * x_src + sig[i] * z_at(i)
        zt = zs + (z_fe - x_src)            # the paper's Z_FE + Z_src - X_src, summed so that z_fe == x_src gives zs itself
        d = (sig[i + 1] - sig[i]) * (guided(tar_velocity, zt, s, w_tar) - guided(src_velocity, zs, s, w_src))
        z_fe = z_fe + (d if keep_mask is None else (1.0 - keep_mask) * d)
    if refine == 0:
        return z_fe
    x = ((1.0 - sig[fe_end]) * x_src + sig[fe_end] * z_at(fe_end)) + (z_fe - x_src)
    for i in range(fe_end, N):
        x = x + (sig[i + 1] - sig[i]) * guided(tar_velocity, x, torch.tensor(sig[i]), w_tar)
    return x
