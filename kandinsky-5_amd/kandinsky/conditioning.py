"""Visual conditioning of the DiT (image-to-video, latent continuation).

Every shipped config builds the DiT with `visual_cond: true`: its input is `cat([latent, visual_cond, visual_cond_mask], -1)`,
16 + 16 + 1 channels (reference dit.py / generation_utils.py:107-112, where the last 17 are always zero).  The helpers here fill
them: `image_to_visual_cond` puts the VAE latent of a picture on latent frame 0, `latents_to_visual_cond` puts k given latent
frames on frames 0..k-1.  Both return `(visual_cond (T,H,W,16), visual_cond_mask (T,H,W,1))` fp32, the keyword arguments of
`generate`.

Video-to-video and masked editing start from a source clip instead: `encode_video` gives `generate`'s `init_latent`,
`pixel_mask_to_latent` its `keep_mask`.
"""
import torch
import torch.nn.functional as F


def _to_float_chw(image):
    """PIL image | uint8 HWC / CHW tensor | float CHW tensor in [-1, 1] -> float32 (3, h, w) in [-1, 1] on the CPU."""
    if not torch.is_tensor(image):
        import numpy as np
        arr = np.asarray(image.convert("RGB"), dtype=np.uint8)        # PIL: RGB, HWC
        image = torch.from_numpy(arr.copy())
    x = image.detach().cpu()
    if x.dim() != 3:
        raise ValueError(f"image must be a 3-D HWC or CHW tensor, got shape {tuple(x.shape)}")
    if x.dtype == torch.uint8:
        if x.shape[-1] == 3 and x.shape[0] != 3:
            x = x.permute(2, 0, 1)
        if x.shape[0] != 3:
            raise ValueError(f"uint8 image must have 3 channels (HWC or CHW), got shape {tuple(x.shape)}")
        return x.float() / 127.5 - 1.0
    if not x.is_floating_point():
        raise ValueError(f"image tensors must be uint8 or floating point, got {x.dtype}")
    if x.shape[0] != 3:
        raise ValueError(f"float image must be CHW with 3 channels, got shape {tuple(x.shape)}")
    return x.float()


def preprocess_image(image, height, width):
    """The picture as the VAE sees it: float32 (3, height, width) in [-1, 1].

    Rule: with (h, w) the input size, s = max(height / h, width / w); the image is resized to
    (max(height, round(h * s)), max(width, round(w * s))) — the smallest size that covers (height, width) at the input's aspect
    ratio — by bicubic interpolation with antialiasing (`F.interpolate(mode="bicubic", antialias=True, align_corners=False)`),
    then centre-cropped: rows [(H' - height) // 2, + height), columns [(W' - width) // 2, + width).  Values are clamped to [-1, 1].
    uint8 input u maps to u / 127.5 - 1 before the resize, so a uint8 image and its float twin give the same result."""
    x = _to_float_chw(image)
    h, w = x.shape[1:]
    s = max(height / h, width / w)
    nh, nw = max(height, round(h * s)), max(width, round(w * s))
    if (nh, nw) != (h, w):
        x = F.interpolate(x[None], size=(nh, nw), mode="bicubic", antialias=True, align_corners=False)[0]
    top, left = (nh - height) // 2, (nw - width) // 2
    return x[:, top:top + height, left:left + width].clamp(-1.0, 1.0).contiguous()


@torch.no_grad()
def encode_image(image, vae, height, width, vae_device="cuda"):
    """Posterior mean of the VAE encoder on the preprocessed picture, times `scaling_factor`: fp32 (1, height/8, width/8, C) on
    `vae_device`."""
    x = preprocess_image(image, height, width).to(vae_device)[None, :, None]      # (1, 3, 1, H, W)
    mean = vae.encode(x).latent_dist.mean                                   # (1, C, 1, H/8, W/8)
    return (mean.float() * vae.config.scaling_factor)[:, :, 0].permute(0, 2, 3, 1).contiguous()


def preprocess_video(frames, height, width):
    """The clip as the VAE sees it: float32 (F, 3, height, width) in [-1, 1], `preprocess_image`'s rule applied to every frame.
    `frames`: uint8 (F, h, w, 3) or float (F, 3, h, w) in [-1, 1]."""
    if not torch.is_tensor(frames):
        import numpy as np
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dim() != 4:
        raise ValueError(f"video must be uint8 (F, H, W, 3) or float (F, 3, H, W), got shape {tuple(frames.shape)}")
    if frames.dtype == torch.uint8:
        if frames.shape[-1] != 3:
            raise ValueError(f"uint8 video must be (F, H, W, 3), got shape {tuple(frames.shape)}")
    elif not frames.is_floating_point() or frames.shape[1] != 3:
        raise ValueError(f"float video must be (F, 3, H, W), got {frames.dtype} of shape {tuple(frames.shape)}")
    if frames.shape[0] < 1:
        raise ValueError("video has no frames")
    return torch.stack([preprocess_image(f, height, width) for f in frames])


@torch.no_grad()
def encode_video(video, vae, num_frames, height, width, vae_device="cuda"):
    """Clean latent of a source clip for video-to-video: posterior mean of the VAE encoder (through `vae.encode` and its tiling) on the
    first 4 * (num_frames - 1) + 1 preprocessed pixel frames, times `scaling_factor`: fp32 (num_frames, height/8, width/8, C) on
    `vae_device`.  ValueError when the clip is shorter."""
    if height % 8 or width % 8:
        raise ValueError(f"height and width must be multiples of 8, got {height} x {width}")
    need = 4 * (int(num_frames) - 1) + 1
    if len(video) < need:
        raise ValueError(f"a {num_frames}-frame latent needs {need} pixel frames, the video has {len(video)}")
    x = preprocess_video(video[:need], height, width).to(vae_device).permute(1, 0, 2, 3)[None]   # (1, 3, F, H, W)
    mean = vae.encode(x).latent_dist.mean                                                    # (1, C, T, H/8, W/8)
    return (mean.float() * vae.config.scaling_factor)[0].permute(1, 2, 3, 0).contiguous()


def pixel_mask_to_latent(mask, T, H, W):
    """Pixel keep mask -> latent keep mask fp32 (T, H/8, W/8, 1), pooled conservatively: a latent cell is 1 only if every pixel of its
    8x8 block is >= 0.5 in every pixel frame it covers (latent frame 0 = pixel frame 0, latent frame t >= 1 = pixel frames
    4t-3 .. 4t), otherwise 0 — nothing is kept that the mask did not cover entirely.  `mask`: (H, W), applied to all frames, or
    (F, H, W) with F >= 4 * (T - 1) + 1; bool, integer or float."""
    if not torch.is_tensor(mask):
        import numpy as np
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    if H % 8 or W % 8:
        raise ValueError(f"height and width must be multiples of 8, got {H} x {W}")
    need = 4 * (int(T) - 1) + 1
    m = mask.detach().cpu().float() >= 0.5
    if m.dim() == 2:
        m = m[None].expand(need, -1, -1)
    if m.dim() != 3 or tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"mask must be ({H}, {W}) or (F, {H}, {W}), got shape {tuple(mask.shape)}")
    if m.shape[0] < need:
        raise ValueError(f"a {T}-frame latent needs a mask of {need} pixel frames, got {m.shape[0]}")
    cell = m[:need].reshape(need, H // 8, 8, W // 8, 8).all(dim=4).all(dim=2)            # (F, H/8, W/8)
    out = torch.empty((T, H // 8, W // 8), dtype=torch.bool)
    out[0] = cell[0]
    if T > 1:
        out[1:] = cell[1:].reshape(T - 1, 4, H // 8, W // 8).all(dim=1)
    return out.float()[..., None].contiguous()


def region_masks_to_latent(masks, T, H, W):
    """Pixel region masks -> latent region masks fp32 (R, T, H/8, W/8) for `set_regions` / `generate(region_masks=)`: the mean over each 8x8
    block and over the pixel frames of each latent frame (`pixel_mask_to_latent`'s frame rule — latent frame 0 = pixel frame 0, latent frame
    t >= 1 = pixel frames 4t-3 .. 4t — with a mean where that function takes `all`), clamped to [0, 1].  `masks`: (R, H, W), applied to all
    frames, or (R, F, H, W) with F >= 4 * (T - 1) + 1; any real dtype (bool: False / True = 0 / 1)."""
    if not torch.is_tensor(masks):
        import numpy as np
        masks = torch.from_numpy(np.ascontiguousarray(masks))
    if H % 8 or W % 8:
        raise ValueError(f"height and width must be multiples of 8, got {H} x {W}")
    need = 4 * (int(T) - 1) + 1
    m = masks.detach().cpu().float()
    if m.dim() == 3:
        m = m[:, None].expand(-1, need, -1, -1)
    if m.dim() != 4 or tuple(m.shape[2:]) != (H, W):
        raise ValueError(f"masks must be (R, {H}, {W}) or (R, F, {H}, {W}), got shape {tuple(masks.shape)}")
    if m.shape[1] < need:
        raise ValueError(f"a {T}-frame latent needs masks of {need} pixel frames, got {m.shape[1]}")
    R = m.shape[0]
    cell = m[:, :need].reshape(R, need, H // 8, 8, W // 8, 8).mean(dim=(3, 5))            # (R, F, H/8, W/8)
    out = torch.empty((R, T, H // 8, W // 8), dtype=torch.float32)
    out[:, 0] = cell[:, 0]
    if T > 1:
        out[:, 1:] = cell[:, 1:].reshape(R, T - 1, 4, H // 8, W // 8).mean(dim=2)
    return out.clamp_(0.0, 1.0).contiguous()


def latents_to_visual_cond(latents, num_frames):
    """k latent frames (k, H, W, C) -> (visual_cond (num_frames, H, W, C), mask (num_frames, H, W, 1)): frames 0..k-1 hold the
    given latents with mask 1, the rest are zero."""
    if latents.dim() != 4:
        raise ValueError(f"latents must be (k, H, W, C), got shape {tuple(latents.shape)}")
    k = latents.shape[0]
    if not 0 < k <= num_frames:
        raise ValueError(f"{k} conditioning frames for a {num_frames}-frame latent")
    vc = torch.zeros((num_frames,) + tuple(latents.shape[1:]), dtype=torch.float32, device=latents.device)
    vc[:k] = latents.float()
    mask = torch.zeros((num_frames,) + tuple(latents.shape[1:3]) + (1,), dtype=torch.float32, device=latents.device)
    mask[:k] = 1.0
    return vc, mask


def image_to_visual_cond(image, vae, num_frames, height, width, device=None, vae_device="cuda"):
    """Image-to-video conditioning: the picture's latent (`encode_image` on `vae_device`) on latent frame 0 of `num_frames`, mask 1
    there; moved to `device` if given.  `height`, `width` in pixels (multiples of 8)."""
    if height % 8 or width % 8:
        raise ValueError(f"height and width must be multiples of 8, got {height} x {width}")
    z = encode_image(image, vae, height, width, vae_device)
    vc, mask = latents_to_visual_cond(z, num_frames)
    if device is not None:
        vc, mask = vc.to(device), mask.to(device)
    return vc, mask


__all__ = ["preprocess_image", "encode_image", "latents_to_visual_cond", "image_to_visual_cond", "preprocess_video", "encode_video",
           "pixel_mask_to_latent"]
