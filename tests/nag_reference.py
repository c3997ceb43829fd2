"""The definition of normalized attention guidance (include/k5.h, k5_nag_combine_bf16) in float64: what the kernel tests hold the GPU to.
Shared by tests/test_nag_host.py (its identities) and tests/test_gpu_nag.py (the kernel's error bound)."""
import torch


def nag_reference(z_pos, z_neg, s, tau, alpha):
    """z_pos, z_neg [rows][D] (any float dtype, taken as they are) -> (out, f * g, clamped rows), float64, nothing rounded to bf16"""
    zp, zn = z_pos.double(), z_neg.double()
    g = zp + (float(s) - 1.0) * (zp - zn)
    n_pos, n_g = zp.abs().sum(-1, keepdim=True), g.abs().sum(-1, keepdim=True)
    clamped = n_g > float(tau) * n_pos
    f = torch.where(clamped, float(tau) * n_pos / torch.where(clamped, n_g, torch.ones_like(n_g)), torch.ones_like(n_g))
    fg = f * g
    return zp + float(alpha) * (fg - zp), fg, clamped.squeeze(-1)


def nag_inputs(rows, D, seed=0):
    """the kernel tests' recipe: z+ ~ N(0, 1) in bf16; even rows z- = bf16(z+ + 0.05 N) (not clamped at (5, 2.5, 0.25)), odd rows independent
    noise (clamped); row 3: z+ = 0; row 4: z- = z+"""
    g = torch.Generator().manual_seed(1000 * D + rows + seed)
    zp = torch.randn(rows, D, generator=g).bfloat16()
    near = (zp.float() + 0.05 * torch.randn(rows, D, generator=g)).bfloat16()
    far = torch.randn(rows, D, generator=g).bfloat16()
    odd = (torch.arange(rows) % 2 == 1)[:, None]
    zn = torch.where(odd, far, near)
    if rows > 3:
        zp[3] = 0
    if rows > 4:
        zn[4] = zp[4]
    return zp, zn
