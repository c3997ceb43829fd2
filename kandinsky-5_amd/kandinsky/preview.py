"""Latent -> RGB factors for the sampler's live previews (`generate(callback=, preview_every=, preview_factors=)`,
`DiffusionTransformer3D.set_watch`).

The preview kernel maps every latent cell to one RGB value, rgb = b + sum_k W[k] x0[k] in [-1, 1], shown as uint8.  W [C][3] and b [3] belong
to a VAE: they are fitted here from one generation of the checkpoint in use (`fit_rgb_factors`, `test.py --fit_preview_factors OUT.json`) and
kept in a small JSON file.  No default table ships: asking for previews without factors is an error that points here.
"""
import json

import torch

TEMPORAL, SPATIAL = 4, 8   # pixels a latent cell covers: 8 x 8 over 4 frames, the first latent frame 1 frame (the VAE's causal layout)


def cell_means(frames, T, H, W):
    """Mean RGB of the pixels every latent cell covers: `frames` (F,3,Hp,Wp) or (F,Hp,Wp,3), float in [-1, 1] or uint8 (mapped to [-1, 1] as
    v / 127.5 - 1), F = 1 + 4 (T - 1), Hp = 8 H, Wp = 8 W  ->  float64 (T,H,W,3).  Latent frame 0 covers frame 0, latent frame t >= 1 the
    frames 4 t - 3 .. 4 t."""
    frames = torch.as_tensor(frames)
    if frames.dim() != 4:
        raise ValueError(f"frames must be (F,3,H,W) or (F,H,W,3), got {tuple(frames.shape)}")
    if frames.shape[-1] == 3 and frames.shape[1] != 3:
        frames = frames.permute(0, 3, 1, 2)
    elif frames.shape[1] != 3:
        raise ValueError(f"frames must have 3 colour channels, got {tuple(frames.shape)}")
    x = frames.cpu()
    x = x.double() / 127.5 - 1.0 if x.dtype == torch.uint8 else x.double()
    F = 1 + TEMPORAL * (T - 1)
    if tuple(x.shape) != (F, 3, SPATIAL * H, SPATIAL * W):
        raise ValueError(f"a latent of (T,H,W) = {(T, H, W)} covers frames of shape {(F, 3, SPATIAL * H, SPATIAL * W)}, got {tuple(x.shape)}")
    blocks = x.reshape(F, 3, H, SPATIAL, W, SPATIAL).mean(dim=(3, 5))          # (F,3,H,W)
    per_t = [blocks[:1].mean(dim=0)]
    if T > 1:
        per_t += list(blocks[1:].reshape(T - 1, TEMPORAL, 3, H, W).mean(dim=1))
    return torch.stack(per_t).permute(0, 2, 3, 1).contiguous()                  # (T,H,W,3)


def fit_rgb_factors(latent, frames):
    """Least-squares (W [C][3], b [3]), fp32, with b + latent_cell @ W ~ the mean RGB in [-1, 1] of the pixels the cell covers.
    `latent` (T,H,W,C) is the final latent of a generation as `generate` returns it (the preview kernel sees the latent in that scale),
    `frames` its decoded frames (see `cell_means`)."""
    latent = torch.as_tensor(latent)
    if latent.dim() != 4:
        raise ValueError(f"latent must be (T,H,W,C), got {tuple(latent.shape)}")
    T, H, W, C = latent.shape
    y = cell_means(frames, T, H, W).reshape(-1, 3)
    A = torch.cat([latent.detach().cpu().double().reshape(-1, C), torch.ones(T * H * W, 1, dtype=torch.float64)], dim=1)
    if A.shape[0] < C + 1:
        raise ValueError(f"{A.shape[0]} latent cells cannot determine {C + 1} coefficients per colour")
    sol = torch.linalg.lstsq(A, y).solution                                      # (C+1, 3)
    return sol[:C].float().contiguous(), sol[C].float().contiguous()


def save_factors(path, factors, bias=None, note=None):
    """Write (W [C][3], b [3]) as JSON: {"channels": C, "factors": [[r, g, b] x C], "bias": [r, g, b]}."""
    W = torch.as_tensor(factors, dtype=torch.float32)
    if W.dim() != 2 or W.shape[1] != 3:
        raise ValueError(f"factors must be [C][3], got {tuple(W.shape)}")
    b = torch.zeros(3) if bias is None else torch.as_tensor(bias, dtype=torch.float32).reshape(-1)
    if b.numel() != 3:
        raise ValueError("bias must hold 3 values")
    doc = {"channels": int(W.shape[0]), "factors": [[float(v) for v in row] for row in W.tolist()], "bias": [float(v) for v in b.tolist()]}
    if note:
        doc["note"] = str(note)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    return path


def load_factors(path):
    """(W [C][3], b [3]) fp32 from a file `save_factors` wrote (float32 values survive the round trip bit for bit)."""
    with open(path) as f:
        doc = json.load(f)
    W = torch.tensor(doc["factors"], dtype=torch.float32)
    b = torch.tensor(doc.get("bias", [0.0, 0.0, 0.0]), dtype=torch.float32)
    if W.dim() != 2 or W.shape[1] != 3 or b.numel() != 3 or int(doc.get("channels", W.shape[0])) != W.shape[0]:
        raise ValueError(f"{path} does not hold [C][3] factors and a bias of 3")
    return W, b


def as_factors(value):
    """What `preview_factors=` accepts -> (W, b | None): the path of a JSON file `save_factors` wrote, a (W, b) pair, or W alone."""
    if value is None:
        return None, None
    if isinstance(value, (str, bytes)) or hasattr(value, "__fspath__"):
        return load_factors(value)
    if isinstance(value, (tuple, list)) and len(value) == 2 and torch.as_tensor(value[0]).dim() == 2:
        return value[0], value[1]
    return value, None


def preview_to_image(preview, frame=None):
    """A PIL image of one frame of a (T,H,W,3) uint8 preview (`frame` None = the middle one); a (H,W,3) preview is taken as it is."""
    from PIL import Image
    p = torch.as_tensor(preview).cpu()
    if p.dtype != torch.uint8 or p.shape[-1] != 3 or p.dim() not in (3, 4):
        raise ValueError(f"a preview is a uint8 (T,H,W,3) tensor, got {p.dtype} {tuple(p.shape)}")
    if p.dim() == 4:
        p = p[p.shape[0] // 2 if frame is None else int(frame)]
    return Image.fromarray(p.contiguous().numpy(), "RGB")


def fit_from_pipeline(pipe, text, **pipe_kw):
    """One generation of `pipe` (a single-rank Kandinsky5T2VPipeline; `pipe_kw` are its call's keywords) and the factors fitted from its own
    final latent and decoded frames: (W [C][3], b [3]).  The latent is taken from the sampler's last step through a watch on the DiT (the
    denoised estimate at sigma = 0 is the latent itself), so the pipeline runs exactly as it always does."""
    dit = pipe.dit
    got = {}

    def tap(info):
        if info.x0 is not None and info.step == info.num_steps - 1:
            got["latent"] = info.x0.clone()

    every = 1 << 30   # no step but the last carries a preview
    dit.set_watch(tap, preview_every=every, rgb_factors=torch.zeros(dit.in_visual_dim, 3), want_x0=True)
    try:
        frames = pipe(text, progress=False, **pipe_kw)
    finally:
        dit.clear_watch()
    if "latent" not in got or not torch.is_tensor(frames):
        raise RuntimeError("fit_from_pipeline needs a video generation (time_length > 0) of one prompt on a single-rank pipeline")
    return fit_rgb_factors(got["latent"], frames[0].permute(1, 0, 2, 3))
