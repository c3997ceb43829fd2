"""CPU stand-ins for `_engine.tile_tables` / `_engine.cfg_euler_tiles_`, shared by the host tests of temporal and spatial context windows: the
blend of the windows' velocities over a `TileWindows` plan and the Euler update, in torch on the plan's host tables."""
import torch


def cpu_tile_tables(plan, device):
    return plan


def cpu_cfg_euler_tiles(img, vc, vu, w, dt, plan):
    wt, wy, wx = plan.weights
    nt, ny, nx = plan.counts
    acc = torch.zeros_like(img)
    for k in range(plan.nwin):
        it, iy, ix = k // (ny * nx), (k // nx) % ny, k % nx
        v = vc[k] if vu is None else vu[k] + w * (vc[k] - vu[k])
        acc[plan.box(k)] += ((wt[it][:, None, None] * wy[iy][None, :, None]) * wx[ix][None, None, :])[..., None] * v.float()
    img.add_((dt * acc).to(torch.bfloat16).float())
    return img
