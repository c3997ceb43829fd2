"""Kandinsky5T2VPipeline — host mirror of kandinsky/t2v_pipeline.py:10-189 (same ctor, same __call__)."""
from typing import Union

import torch

from .generation_utils import generate_sample

_NEG = ("Static, 2D cartoon, cartoon, 2d animation, paintings, images, worst quality, low quality, ugly, "
        "deformed, walking backwards")


class Kandinsky5T2VPipeline:
    def __init__(self, device_map: Union[str, torch.device, dict], dit, text_embedder, vae, resolution: int = 512,
                 local_dit_rank: int = 0, world_size: int = 1, conf=None, offload: bool = False):
        if resolution not in [512]:
            raise ValueError("Resolution can be only 512")
        self.dit, self.text_embedder, self.vae = dit, text_embedder, vae
        self.resolution = resolution
        self.device_map = device_map
        self.local_dit_rank, self.world_size = local_dit_rank, world_size
        self.conf = conf
        self.num_steps = conf.model.num_steps
        self.guidance_weight = conf.model.guidance_weight
        self.offload = offload
        self.RESOLUTIONS = {512: [(512, 512), (512, 768), (768, 512)]}

    def expand_prompt(self, prompt):
        """Prompt beautification through the Qwen2.5-VL chat model (reference t2v_pipeline.py:47-88).
        Delegated to the text embedder wrapper, which owns the HF model."""
        return self.text_embedder.expand_prompt(prompt)

    def set_lora(self, lora=None, lora_scale=1.0):
        """(extension) The LoRA adapters in effect from now on: every earlier one is removed (`dit.clear_lora()`), then `lora` — a
        .safetensors path / state dict, or a list of them — is merged with `lora_scale` (one strength, or one per adapter).  None removes
        them all.  Every rank of a multi-GPU run makes the same call."""
        from .lora import as_list
        loras, scales = as_list(lora, lora_scale)
        self.dit.clear_lora()
        for adapter, s in zip(loras, scales):
            self.dit.add_lora(adapter, strength=s)
        return self

    # ------------------------------------------------------------------ helpers of __call__
    def _agree_on(self, value_fn, as_object=False):
        """rank 0 computes `value_fn()`, every rank returns the same value (reference t2v_pipeline.py:108-118,131-141)."""
        mine = value_fn() if self.local_dit_rank == 0 else None
        if self.world_size <= 1:
            return mine
        if as_object:
            box = [mine]
            torch.distributed.broadcast_object_list(box, 0)
            return box[0]
        # the reference moves the scalar to cuda:LOCAL_RANK (t2v_pipeline.py:112); here the rank's device is whatever the factory assigned it
        # (K5_OVERSUBSCRIBE wraps ranks around the devices that exist) and a host-side process group (gloo: the IPC transport) takes it on the CPU
        host = torch.distributed.get_backend() == "gloo"
        t = torch.tensor([mine], dtype=torch.int64) if mine is not None else torch.empty(1, dtype=torch.int64)
        if not host:
            t = t.to(torch.device(self.device_map["dit"]))
        torch.distributed.broadcast(t, 0)
        return int(t.item())

    def _check_size(self, height, width):
        if self.resolution != 512:
            raise NotImplementedError("Only 512 resolution is available for now")
        allowed = self.RESOLUTIONS[self.resolution]
        if (height, width) not in allowed:
            raise ValueError(f"Wrong height, width pair. Available (height, width) are: {allowed}")

    def _check_tiles(self, height, width, tile_height, tile_width, tile_overlap):
        """The tile keywords (pixels) -> `generate`'s spatial context keywords (latent cells), or None without them.  The tile must be one of
        the allowed sizes, the frame multiples of 16 that are at least the tile and, when sqrt(height * width) > 900, keys of the VAE's spatial
        tiling table (the decode tiles there); ValueError naming the allowed values otherwise."""
        if tile_height is None and tile_width is None:
            if tile_overlap is not None:
                raise ValueError("tile_overlap needs tile_height and tile_width")
            return None
        if self.resolution != 512:
            raise NotImplementedError("Only 512 resolution is available for now")
        allowed = self.RESOLUTIONS[self.resolution]
        if (tile_height, tile_width) not in allowed:
            raise ValueError(f"Wrong tile_height, tile_width pair. Available (tile_height, tile_width) are: {allowed}")
        if height % 16 or width % 16 or height < tile_height or width < tile_width:
            raise ValueError(f"With tiles, height and width must be multiples of 16 that are at least the tile ({tile_height}, {tile_width}), "
                             f"got ({height}, {width})")
        if (height * width) ** 0.5 > 900:
            from .models.vae import OPT_SPATIAL_TILING
            keys = sorted(OPT_SPATIAL_TILING)
            if height not in keys or width not in keys:
                raise ValueError(f"With tiles and sqrt(height * width) > 900, height and width must be keys of the VAE's spatial tiling table: "
                                 f"{keys}, got ({height}, {width})")
        out = dict(context_height=tile_height // 8, context_width=tile_width // 8)
        if tile_overlap is not None:
            if tile_overlap < 0 or tile_overlap % 16 or tile_overlap >= min(tile_height, tile_width):
                raise ValueError(f"tile_overlap must be a multiple of 16 in [0, {min(tile_height, tile_width)}), got {tile_overlap}")
            out["context_overlap_hw"] = tile_overlap // 8
        return out

    def _beautified(self, prompt):
        if self.offload:
            self.text_embedder = self.text_embedder.to(self.device_map["text_embedder"])
        return self.expand_prompt(prompt)

    @staticmethod
    def _save(images, time_length, save_path):
        """uint8 (B,3,F,H,W) -> PIL list (image mode) or the tensor itself; optional PNG / video files (reference :166-189)."""
        paths = None if save_path is None else ([save_path] if isinstance(save_path, str) else list(save_path))
        if time_length == 0:
            from .video_io import to_pil_images
            pics = to_pil_images(images.squeeze(2).cpu())
            if paths is not None and len(paths) == len(pics):
                for path, pic in zip(paths, pics):
                    pic.save(path)
            return pics
        if paths is not None and len(paths) == len(images):
            from .video_io import write_video
            for path, clip in zip(paths, images):
                write_video(path, clip.permute(1, 2, 3, 0).cpu(), fps=24)
        return images

    def __call__(self, text: Union[str, list], time_length: int = 5, width: int = 768, height: int = 512, seed: int = None,
                 num_steps: int = None, guidance_weight: float = None, scheduler_scale: float = 10.0,
                 negative_caption: str = _NEG, expand_prompts: bool = True, save_path: str = None,
                 progress: bool = True, image=None, video=None, strength: float = None, mask=None, callback=None,
                 preview_every: int = 0, preview_factors=None, context_seconds: float = None, context_overlap_seconds: float = None,
                 nag_scale: float = None, nag_tau: float = 2.5, nag_alpha: float = 0.25, regions=None, region_base_weight: float = 0.0,
                 guidance_schedule=None, guidance_interval=None, cfg_zero_star: bool = False, cfg_zero_init: int = 0, cfg_rescale: float = 0.0,
                 slg_blocks=None, slg_scale: float = 0.0, slg_interval=None, slg_mode: str = "block", eta: float = 0.0, s_noise: float = 1.0,
                 sde_interval=None, sde_seed: int = None, enhance_weight: float = None, enhance_interval=None,
                 forecast_interval: int = None, forecast_order: int = 1, forecast_warmup: int = None, forecast_tail: int = 1,
                 source_caption: str = None, source_guidance_weight: float = None, flowedit_refine: int = 0, flowedit_seed: int = None,
                 tile_height: int = None, tile_width: int = None, tile_overlap: int = None):
        """reference t2v_pipeline.py:90-189 (same arguments, defaults, errors and return values: uint8 tensor (1,3,F,H,W) on
        rank 0 / list of PIL images for time_length = 0, None on the other ranks).  `image` (optional, extension): image-to-video,
        the clip starts from this picture (PIL image or tensor, resized to cover (height, width) and centre-cropped); every rank
        passes the same picture.  `text` (extension) may be a list of prompts: they are sampled together (generate_sample with
        bs = len(text), one seed) and one output is returned per prompt — uint8 (len(text),3,F,H,W) / a PIL list of len(text).
        `video`, `strength`, `mask` (optional, extension): video-to-video and masked editing.  `video` is the source clip (uint8
        (F,H,W,3) or float (F,3,H,W) frames, at least as long as the output; resized and cropped per frame like `image`), `strength`
        in (0, 1] (None = 1) the part of the schedule that runs on it, `mask` a pixel keep mask (height, width) or (F, height, width),
        >= 0.5 = keep the source there.  Every rank passes the same inputs, as with `image`.
        `progress` draws a tqdm bar over the sampling steps (single-rank, tqdm installed).  `callback`, `preview_every`,
        `preview_factors` (optional, extension; single-rank only): `callback(info)` after every sampling step (a truthy return stops
        the run with `kandinsky.models.dit.SamplingInterrupted`), with a uint8 (T,H,W,3) `info.preview` of the denoised latent on every
        `preview_every`-th step through the latent -> RGB factors `preview_factors` (`kandinsky.preview`), see `generate`.
        `context_seconds`, `context_overlap_seconds` (optional, extension): a clip longer than the checkpoint's trained length, e.g.
        `pipe(text, time_length=20, context_seconds=10, context_overlap_seconds=2.5)`: the model runs on overlapping windows of
        `context_seconds` (s * 24 // 4 + 1 latent frames, overlapping by s * 6; default a quarter of the window) whose velocities are
        cross-faded at every step.  `text` may then be a list of nwin prompts, one per window in order (one clip comes back).
        Single-rank, without `video`, previews or MagCache.
        `nag_scale`, `nag_tau`, `nag_alpha` (optional, extension): normalized attention guidance — `negative_caption` steers inside the
        cross-attention of the one conditional forward, which is what makes it count on the checkpoints that run without classifier-free
        guidance (nocfg, distil).  `nag_scale` None (default) is off; 5 / 2.5 / 0.25 are the commonly quoted values, starting points that
        were not tuned on any Kandinsky checkpoint.  See `generate`.
        `regions`, `region_base_weight` (optional, extension): regional prompts, `pipe(text, regions=[(prompt, mask), ...])` — 1 to 8 pairs of
        a prompt and a pixel mask in [0, 1], (height, width) or (F, height, width), that says where the prompt applies; `text` is the base
        prompt, which the uncovered pixels see alone and which weighs `region_base_weight` in [0, 1] under the regions.  The masks are
        pooled to the latent cells by their mean (`conditioning.region_masks_to_latent`), the region prompts are encoded with the caption
        (not expanded) and every visual block blends its cross-attention to the prompts per token (`DiffusionTransformer3D.set_regions`).  A
        list of texts shares one region set.  Not together with `context_seconds`.  No checkpoint was at hand when this was written:
        what it does to a picture is not claimed.
        `guidance_schedule`, `guidance_interval`, `cfg_zero_star`, `cfg_zero_init`, `cfg_rescale` (optional, extension): a guidance weight
        per step (a list of num_steps values or a callable `(i, sigma_i)`), a sigma interval outside which the unconditional forward is
        not run, CFG-Zero* with its zero-init of the first K steps, and CFG rescale in [0, 1]; see `generate`.  All off by default, every
        rank passes the same values.  Not together with `context_seconds`.  No checkpoint was at hand when this was written: the rules are
        the published ones, what they do to a picture is not claimed.
        `slg_blocks`, `slg_scale`, `slg_interval`, `slg_mode` (optional, extension): skip-layer guidance,
        `pipe(text, slg_blocks=[9, 10], slg_scale=3.0, slg_interval=(0.2, 0.99))` — on the steps whose sigma lies in the interval the model
        runs once more with the listed visual blocks (mode "attention": only their self-attention) skipped and the velocity is pushed away
        from that weakened prediction; see `generate`.  Off by default, every rank passes the same values.  Not together with
        `context_seconds`, MagCache or a CFG pair.  The values shown are the ones commonly quoted for other models: no Kandinsky checkpoint
        was at hand when this was written, what they do to a picture is not claimed.
        `eta`, `s_noise`, `sde_interval`, `sde_seed` (optional, extension): stochastic sampling, `pipe(text, eta=1.0)` — on the steps whose
        sigma lies in `sde_interval` (None = all) the Euler step stops short and the latent is re-noised to the next sigma with noise
        generated inside the update kernel from (`sde_seed`, step, element) (`sde_seed` None = `seed`); see `generate`.  eta 0 (default) is
        off, every rank passes the same values.  Not together with `context_seconds`, MagCache or previews.  No checkpoint was at hand when
        this was written: visual quality is not claimed.
        `enhance_weight`, `enhance_interval` (optional, extension): Enhance-A-Video, `pipe(text, enhance_weight=4.0)` — on the steps whose
        sigma lies in `enhance_interval` (None = all) every visual block scales its self-attention output by the cross-frame attention
        score of its own queries and keys; see `generate`.  None (default) is off, 0.0 is a valid weight.  Not on a sequence-parallel
        group, not with more than 64 latent frames per forward.  No checkpoint was at hand when this was written: visual quality is not
        claimed.
        `source_caption`, `source_guidance_weight`, `flowedit_refine`, `flowedit_seed` (optional, extension): FlowEdit,
        `pipe("a dog on a sofa", video=clip, source_caption="a cat on a sofa", strength=0.7)` — "the same clip, but the cat is a dog": the
        difference between the two prompts' velocities is integrated along a noisy path tied to the clip, nothing is inverted and the clip
        stays where the prompts agree; see `generate`.  `source_caption` is not expanded.  None (default) is off and `video` is the SDEdit
        path.  Single-rank, without MagCache, previews or the other sampler extensions.  SD3's published values (33 of 50 steps, source
        guidance 3.5, target 13.5) are examples: no Kandinsky checkpoint was at hand when this was written, visual quality is not claimed.
        `tile_height`, `tile_width`, `tile_overlap` (optional, extension; pixels): a frame larger than the checkpoint's trained size,
        `pipe(text, height=1024, width=1024, tile_height=512, tile_width=768, tile_overlap=128)` — the model runs on overlapping spatial
        windows of the trained size (one of the allowed (height, width) pairs) whose velocities are cross-faded at every step; see
        `generate`.  height and width are then multiples of 16 that are at least the tile and, beyond sqrt(height * width) = 900, keys of the
        VAE's spatial tiling table.  `tile_overlap` None = a quarter of the tile.  Works with `image` and with `context_seconds`; single-rank,
        without `video`, previews or MagCache.  No checkpoint was at hand when this was written: visual quality is not claimed."""
        ctx = {}
        tiled = self._check_tiles(height, width, tile_height, tile_width, tile_overlap)
        if tiled is not None:
            ctx.update(tiled)
        windowed = context_seconds is not None or tiled is not None   # what the windows refuse, the tiles refuse
        windows_kw = "context_seconds" if context_seconds is not None else "tile_height / tile_width"
        flow_kw = {}
        if source_caption is not None:
            flow_kw = dict(source_caption=source_caption, source_guidance_weight=source_guidance_weight, flowedit_refine=flowedit_refine,
                           flowedit_seed=flowedit_seed)
        elif source_guidance_weight is not None or flowedit_refine or flowedit_seed is not None:
            raise ValueError("source_guidance_weight / flowedit_refine / flowedit_seed need source_caption (the prompt that describes the clip)")
        forecast_kw = {}
        if forecast_interval is not None:   # `generate` documents it; None or 1 is off
            forecast_kw = dict(forecast_interval=forecast_interval, forecast_order=forecast_order, forecast_warmup=forecast_warmup,
                               forecast_tail=forecast_tail)
        enhance_kw = {}
        if enhance_weight is not None or enhance_interval is not None:
            from .generation_utils import _enhance_for_run, enhance_plan
            enhance_plan([1.0, 0.0], enhance_interval)
            lat = 1 if time_length == 0 else time_length * 24 // 4 + 1
            _enhance_for_run(self.dit, [1.0, 0.0], 0, enhance_weight, None, lat if context_seconds is None else min(lat, int(context_seconds * 24 // 4 + 1)))
            if enhance_weight is None:
                raise ValueError("enhance_interval needs enhance_weight")
            enhance_kw = dict(enhance_weight=float(enhance_weight), enhance_interval=enhance_interval)
        sto_kw = {}
        if eta or sde_interval is not None or float(s_noise) != 1.0:
            from .generation_utils import _stochastic_for_run, stochastic_plan
            stochastic_plan([1.0, 0.0], eta, s_noise, sde_interval)
            _stochastic_for_run(self.dit, [1.0, 0.5, 0.0], 0, eta, s_noise, None, 0 if sde_seed is None else sde_seed, windowed, preview_every)
            sto_kw = dict(eta=eta, s_noise=s_noise, sde_interval=sde_interval, sde_seed=sde_seed)
        skip_kw = {}
        if slg_blocks is not None or slg_scale or slg_interval is not None:
            from .generation_utils import _skip_for_run, skip_plan
            skip_plan([1.0, 0.0], slg_interval)
            _skip_for_run(self.dit, [1.0, 0.0], 0, slg_blocks, slg_scale, None, slg_mode, windowed)
            skip_kw = dict(slg_blocks=slg_blocks, slg_scale=slg_scale, slg_interval=slg_interval, slg_mode=slg_mode)
        guide_kw = {k: v for k, v in dict(guidance_schedule=guidance_schedule, guidance_interval=guidance_interval, cfg_zero_star=cfg_zero_star,
                                          cfg_zero_init=cfg_zero_init, cfg_rescale=cfg_rescale).items() if v}
        if guide_kw:
            from .models.dit import check_guidance_args
            if windowed:
                raise ValueError("guidance_schedule / guidance_interval / cfg_zero_star / cfg_zero_init / cfg_rescale together with "
                                 f"{windows_kw} are not supported: one statistic per window is not the published rule")
            check_guidance_args(None if guidance_schedule is None or callable(guidance_schedule) else guidance_schedule, cfg_zero_star,
                                cfg_zero_init, cfg_rescale)
        region_kw = {}
        if regions is not None:
            from .conditioning import region_masks_to_latent
            from .models.dit import check_region_args
            if windowed:
                raise ValueError(f"regions together with {windows_kw} is not supported: the masks cover the clip, a window sees a slice")
            pairs = list(regions)
            if not 1 <= len(pairs) <= 8 or not all(isinstance(p, (list, tuple)) and len(p) == 2 and isinstance(p[0], str) for p in pairs):
                raise ValueError("regions must be a list of 1 to 8 (prompt, mask) pairs")
            self._check_size(height, width)
            lat_frames = 1 if time_length == 0 else time_length * 24 // 4 + 1
            masks = [torch.as_tensor(m) for _, m in pairs]
            if any(m.dim() != masks[0].dim() or m.shape != masks[0].shape for m in masks):
                raise ValueError("regions: the masks must all have one shape, (height, width) or (F, height, width)")
            lat = region_masks_to_latent(torch.stack([m.float() for m in masks]), lat_frames, height, width)
            check_region_args([{"text_embeds": torch.zeros(1, 1)}] * len(pairs), [[0]] * len(pairs), lat, region_base_weight)
            region_kw = dict(region_text_embeds=[p for p, _ in pairs], region_masks=lat, region_base_weight=float(region_base_weight))
        if nag_scale is not None:
            from .models.dit import check_nag_numbers
            check_nag_numbers(nag_scale, nag_tau, nag_alpha)
            ctx.update(nag_scale=float(nag_scale), nag_tau=float(nag_tau), nag_alpha=float(nag_alpha))
        if context_seconds is not None:
            if time_length == 0:
                raise ValueError("context_seconds needs a video (time_length > 0)")
            if context_seconds <= 0:
                raise ValueError(f"context_seconds must be > 0, got {context_seconds}")
            ctx["context_frames"] = int(context_seconds * 24 // 4 + 1)
            if context_overlap_seconds is not None:
                ctx["context_overlap"] = int(context_overlap_seconds * 6)
        elif context_overlap_seconds is not None:
            raise ValueError("context_overlap_seconds needs context_seconds")
        strength = 1.0 if strength is None else float(strength)
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"strength must be in (0, 1], got {strength}")
        if video is None and (strength < 1.0 or mask is not None):
            raise ValueError("strength and mask need a source video")
        if image is not None and time_length == 0:
            raise ValueError("image conditioning needs a video (time_length > 0)")
        steps = self.num_steps if num_steps is None else num_steps
        weight = self.guidance_weight if guidance_weight is None else guidance_weight
        if seed is None:
            seed = self._agree_on(lambda: int(torch.randint(2 ** 63 - 1, (1,)).item()))
        if tiled is None:
            self._check_size(height, width)
        frames = 1 if time_length == 0 else time_length * 24 // 4 + 1
        if isinstance(text, (list, tuple)):
            if len(text) == 0:
                raise ValueError("text must hold at least one prompt")
            texts = list(text)
            caption = (self._agree_on(lambda: [self._beautified(t) for t in texts], as_object=True) if expand_prompts
                       else texts)
        else:
            caption = self._agree_on(lambda: self._beautified(text), as_object=True) if expand_prompts else text
        bs = len(caption) if isinstance(caption, list) and not ctx else 1   # with context windows a list is one prompt per window of ONE clip

        images = generate_sample((bs, frames, height // 8, width // 8, 16), caption, self.dit, self.vae, self.conf,
                                 text_embedder=self.text_embedder, num_steps=steps, guidance_weight=weight,
                                 scheduler_scale=scheduler_scale, negative_caption=negative_caption, seed=seed,
                                 device=self.device_map["dit"], vae_device=self.device_map["vae"],
                                 text_embedder_device=self.device_map["text_embedder"], progress=progress, offload=self.offload,
                                 image=image, video=video, strength=strength, mask=mask, callback=callback,
                                 preview_every=preview_every, preview_factors=preview_factors, **ctx, **region_kw, **guide_kw, **skip_kw, **sto_kw,
                                 **enhance_kw, **forecast_kw, **flow_kw)
        torch.cuda.empty_cache()
        return self._save(images, time_length, save_path) if self.local_dit_rank == 0 else None
