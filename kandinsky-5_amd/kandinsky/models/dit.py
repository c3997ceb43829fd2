"""DiffusionTransformer3D — host mirror of the reference class (kandinsky/models/dit.py:82-186).

Same constructor kwargs, same `state_dict` keys, same `forward` signature and
`visual_cond` attribute, so `get_T2V_pipeline`, `generate` and the ComfyUI nodes can use it unchanged.
The arithmetic is NOT here: `forward` hands raw device pointers to the gfx950 engine in libk5.so
(kandinsky-5_amd/csrc/engine.hip) through the C ABI (include/k5.h).  There is no eager fallback: without
the library, or with CPU tensors, `forward` raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import torch
from torch import nn

from .. import _engine as E
from .nn import (FeedForward, Modulation, MultiheadCrossAttention, MultiheadSelfAttentionDec,
                 MultiheadSelfAttentionEnc, NormWeight, OutLayer, TextEmbeddings, TimeEmbeddings,
                 VisualEmbeddings, _NoMath)


class TransformerEncoderBlock(_NoMath):  # reference dit.py:22-44
    def __init__(self, model_dim, time_dim, ff_dim, head_dim):
        super().__init__()
        self.text_modulation = Modulation(time_dim, model_dim, 6)
        self.self_attention = MultiheadSelfAttentionEnc(model_dim, head_dim)
        self.feed_forward = FeedForward(model_dim, ff_dim)


class TransformerDecoderBlock(_NoMath):  # reference dit.py:47-79
    def __init__(self, model_dim, time_dim, ff_dim, head_dim):
        super().__init__()
        self.visual_modulation = Modulation(time_dim, model_dim, 9)
        self.self_attention = MultiheadSelfAttentionDec(model_dim, head_dim)
        self.cross_attention = MultiheadCrossAttention(model_dim, head_dim)
        self.feed_forward = FeedForward(model_dim, ff_dim)


def sp_transport(transport=None):
    """"rccl" | "ipc": explicit argument, else K5_SP_TRANSPORT, else RCCL (the transport of a one-rank-per-GPU node)."""
    import os
    t = (transport or os.environ.get("K5_SP_TRANSPORT", "rccl")).lower()
    if t not in ("rccl", "ipc"):
        raise ValueError(f"unknown sequence-parallel transport {t!r} (rccl | ipc)")
    return t


def _broadcast_ipc_name(kind, is_root, world, group, src):
    """The name of an IPC group's shared-memory control block: made up on the group's rank 0, carried by torch.distributed."""
    import os
    import uuid
    payload = [f"/k5ipc_{kind}_{os.getpid()}_{uuid.uuid4().hex[:12]}" if is_root else None]
    if world > 1:
        import torch.distributed as dist
        dist.broadcast_object_list(payload, src=src, group=group)
    return payload[0]


def split_per_sample(value, n, name):
    """One value per sample for the many-sample paths (`sample_many`, `generate(batch=)`): a list / tuple of `n` entries is taken as
    it is; anything else — a dict of embeddings, a tensor of positions, a plain list of int positions — is shared by every sample."""
    if isinstance(value, (list, tuple)) and not (len(value) > 0 and isinstance(value[0], int)):
        if len(value) != n:
            raise ValueError(f"{name} has {len(value)} entries for batch={n}")
        return list(value)
    return [value] * n


class SamplingInterrupted(RuntimeError):
    """A watch callback (`DiffusionTransformer3D.set_watch`, `generate(callback=)`) returned a truthy value: the run stopped after
    `steps_done` steps — at most one past the step the callback saw — and `latent` holds the state at that point (of sample `sample` of a
    `sample_many` call; the samples after it are as they came)."""

    def __init__(self, steps_done, latent, sample=0):
        super().__init__(f"sampling interrupted by the callback after {steps_done} steps" + (f" of sample {sample}" if sample else ""))
        self.steps_done, self.latent, self.sample = int(steps_done), latent, int(sample)


class StepInfo:
    """What a watch callback receives after every step: `step` (0-based, just completed) of `num_steps`, `sample` of `num_samples`
    (`sample_many` / `generate(batch=)`; 0 of 1 otherwise), `sigma` the latent now sits at, `preview` a CPU uint8 tensor (T,H,W,3) on a
    preview step (None otherwise) and `x0` the denoised estimate, a device fp32 (T,H,W,C) tensor valid ONLY during the call (clone it to
    keep it; None unless asked for with want_x0, and on steps without a preview)."""
    __slots__ = ("step", "num_steps", "sample", "num_samples", "sigma", "preview", "x0")

    def __init__(self, step, num_steps, sample, num_samples, sigma, preview, x0):
        self.step, self.num_steps, self.sample, self.num_samples = int(step), int(num_steps), int(sample), int(num_samples)
        self.sigma, self.preview, self.x0 = float(sigma), preview, x0

    def __repr__(self):
        return (f"StepInfo(step={self.step}/{self.num_steps}, sample={self.sample}/{self.num_samples}, sigma={self.sigma:.4f}, "
                f"preview={'yes' if self.preview is not None else 'no'}, x0={'yes' if self.x0 is not None else 'no'})")


class _DeviceView:
    """A raw device pointer as something torch.as_tensor can view without a copy (the CUDA array interface)."""

    def __init__(self, address, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(address), False), "version": 2,
                                         "strides": None}


def check_nag_numbers(scale, tau, alpha):
    """The ValueErrors of the three numbers of normalized attention guidance; returns them as floats."""
    try:
        scale, tau, alpha = float(scale), float(tau), float(alpha)
    except (TypeError, ValueError):
        raise ValueError("nag: scale, tau and alpha must be numbers") from None
    if not math.isfinite(scale) or scale < 1.0:
        raise ValueError(f"nag: scale must be a finite number >= 1 (got {scale})")
    if not math.isfinite(tau) or tau < 1.0:
        raise ValueError(f"nag: tau must be a finite number >= 1 (got {tau})")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"nag: alpha must be in [0, 1] (got {alpha})")
    return scale, tau, alpha


def check_guidance_args(weights, zero_star, zero_init_steps, rescale):
    """The ValueErrors of `set_guidance` / `generate(guidance_schedule=, cfg_zero_star=, cfg_zero_init=, cfg_rescale=)`; returns
    (weights as a list of floats or None, zero_star, zero_init_steps, rescale)."""
    if weights is not None:
        try:
            weights = [float(w) for w in weights]
        except (TypeError, ValueError):
            raise ValueError("guidance: weights must be a sequence of numbers, one per step") from None
        if not weights or not all(math.isfinite(w) for w in weights):
            raise ValueError("guidance: weights must hold one finite number per step")
    try:
        k, phi = int(zero_init_steps), float(rescale)
    except (TypeError, ValueError):
        raise ValueError("guidance: zero_init_steps must be an integer and rescale a number") from None
    if k < 0 or k != zero_init_steps:
        raise ValueError(f"guidance: zero_init_steps must be an integer >= 0 (got {zero_init_steps})")
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"guidance: rescale must be in [0, 1] (got {rescale})")
    return weights, bool(zero_star), k, phi


SKIP_MODES = {"block": 0, "attention": 1}


def check_skip_args(blocks, scale, mode, steps, num_visual_blocks):
    """The ValueErrors of `set_skip_guidance` / `generate(slg_blocks=, slg_scale=, slg_mode=)`; returns (blocks as a list of ints, scale, mode
    name, steps as a list of 0 / 1 or None)."""
    try:
        idx = [int(b) for b in blocks]
        ok = all(i == b for i, b in zip(idx, blocks))
    except (TypeError, ValueError):
        raise ValueError("skip guidance: blocks must be a sequence of visual block indices") from None
    if not idx or not ok:
        raise ValueError("skip guidance: blocks must hold at least one integer block index")
    if any(i < 0 or i >= int(num_visual_blocks) for i in idx):
        raise ValueError(f"skip guidance: block indices must be in 0..{int(num_visual_blocks) - 1} (got {idx})")
    if len(set(idx)) != len(idx):
        raise ValueError(f"skip guidance: a block is listed twice ({idx})")
    try:
        scale = float(scale)
    except (TypeError, ValueError):
        raise ValueError("skip guidance: scale must be a number") from None
    if not math.isfinite(scale) or scale < 0.0:
        raise ValueError(f"skip guidance: scale must be a finite number >= 0 (got {scale})")
    if mode not in SKIP_MODES:
        raise ValueError(f"skip guidance: mode must be 'block' or 'attention' (got {mode!r})")
    if steps is not None:
        steps = [1 if bool(v) else 0 for v in steps]
        if not steps:
            raise ValueError("skip guidance: steps must hold one 0 / 1 per step")
    return idx, scale, mode, steps


def check_enhance_args(weight, steps):
    """The ValueErrors of `set_enhance` / `generate(enhance_weight=, enhance_interval=)`; returns (weight as a float, steps as a list of 0 / 1
    or None).  0.0 is a valid weight (score = max(1, mean * T)); off is `clear_enhance`, not a weight."""
    try:
        ok = not isinstance(weight, bool)
        weight = float(weight)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("enhance: weight must be a number")
    if not math.isfinite(weight) or weight < 0.0:
        raise ValueError(f"enhance: weight must be a finite number >= 0 (got {weight})")
    if steps is not None:
        steps = [1 if bool(v) else 0 for v in steps]
        if not steps:
            raise ValueError("enhance: steps must hold one 0 / 1 per step")
    return weight, steps


def check_forecast_args(order, full):
    """The ValueErrors of `set_forecast`; returns (order as an int, full as a list of 0 / 1)."""
    if isinstance(order, bool) or not isinstance(order, int) or not 0 <= order <= 2:
        raise ValueError(f"forecast: order must be 0, 1 or 2 (got {order!r})")
    full = [1 if bool(v) else 0 for v in full]
    if not full:
        raise ValueError("forecast: full must hold one 0 / 1 per step")
    if not full[0]:
        raise ValueError("forecast: full[0] must be 1: the first step has nothing to extrapolate from")
    return order, full


def check_stochastic_args(dt_down, scale, noise_coef, seed, first_stream=0):
    """The ValueErrors of `set_stochastic`; returns (dt_down, scale, noise_coef as lists of floats, seed as a 64-bit and first_stream as a
    32-bit unsigned int)."""
    try:
        tabs = [[float(v) for v in t] for t in (dt_down, scale, noise_coef)]
    except (TypeError, ValueError):
        raise ValueError("stochastic: dt_down, scale and noise_coef must be sequences of numbers, one per step") from None
    n = len(tabs[0])
    if n < 1 or any(len(t) != n for t in tabs):
        raise ValueError(f"stochastic: dt_down, scale and noise_coef must hold one value per step each (got {[len(t) for t in tabs]})")
    if not all(math.isfinite(v) for t in tabs for v in t):
        raise ValueError("stochastic: every dt_down, scale and noise_coef must be a finite number")
    if any(v < 0.0 for v in tabs[2]):
        raise ValueError("stochastic: noise_coef must be >= 0")
    try:
        seed_i, first_i = int(seed), int(first_stream)
        ok = seed_i == seed and first_i == first_stream
    except (TypeError, ValueError):
        ok = False
    if not ok or isinstance(seed, bool):
        raise ValueError(f"stochastic: seed and first_stream must be integers (got {seed!r}, {first_stream!r})")
    if not 0 <= first_i <= 0xffffffff - n:
        raise ValueError(f"stochastic: first_stream must be in 0..2^32 - 1 - num_steps (got {first_stream})")
    return tabs[0], tabs[1], tabs[2], seed_i & (2 ** 64 - 1), first_i


def check_nag_args(text_embeds, text_rope_pos, scale, tau, alpha):
    """The ValueErrors of `set_nag` / `generate(nag_scale=, nag_tau=, nag_alpha=, nag_text_embeds=)`; returns (scale, tau, alpha) as floats."""
    scale, tau, alpha = check_nag_numbers(scale, tau, alpha)
    if not isinstance(text_embeds, dict) or not torch.is_tensor(text_embeds.get("text_embeds")):
        raise ValueError('nag: the negative prompt must be a dict with a "text_embeds" tensor (what `generate` takes)')
    te = text_embeds["text_embeds"]
    if te.dim() != 2 or te.shape[0] < 1:
        raise ValueError(f"nag: text_embeds must be [tokens][in_text_dim] with at least one token (got {tuple(te.shape)})")
    if text_rope_pos is None or len(torch.as_tensor(text_rope_pos).reshape(-1)) != te.shape[0]:
        raise ValueError("nag: text_rope_pos must have one position per token of the negative prompt")
    return scale, tau, alpha


def check_region_args(text_embeds_list, rope_pos_list, masks, base_weight):
    """The ValueErrors of `set_regions` / `generate(region_text_embeds=, region_text_rope_pos=, region_masks=, region_base_weight=)`; returns
    base_weight as a float."""
    try:
        base_weight = float(base_weight)
    except (TypeError, ValueError):
        raise ValueError("regions: base_weight must be a number") from None
    if math.isnan(base_weight) or not 0.0 <= base_weight <= 1.0:
        raise ValueError(f"regions: base_weight must be in [0, 1] (got {base_weight})")
    if not isinstance(text_embeds_list, (list, tuple)) or not isinstance(rope_pos_list, (list, tuple)):
        raise ValueError("regions: the prompts and their positions must be lists, one entry per region")
    R = len(text_embeds_list)
    if not 1 <= R <= 8:
        raise ValueError(f"regions: 1 to 8 regions (got {R})")
    if len(rope_pos_list) != R:
        raise ValueError(f"regions: {R} prompts but {len(rope_pos_list)} position vectors")
    for r, (te, pos) in enumerate(zip(text_embeds_list, rope_pos_list)):
        if not isinstance(te, dict) or not torch.is_tensor(te.get("text_embeds")):
            raise ValueError(f'regions: prompt {r} must be a dict with a "text_embeds" tensor (what `generate` takes)')
        t = te["text_embeds"]
        if t.dim() != 2 or t.shape[0] < 1:
            raise ValueError(f"regions: prompt {r}: text_embeds must be [tokens][in_text_dim] with at least one token (got {tuple(t.shape)})")
        if pos is None or len(torch.as_tensor(pos).reshape(-1)) != t.shape[0]:
            raise ValueError(f"regions: prompt {r}: text_rope_pos must have one position per token")
    if not torch.is_tensor(masks) or masks.dim() != 4 or masks.shape[0] != R or masks.is_complex():
        raise ValueError(f"regions: masks must be a real (R, T, H, W) tensor on the latent cells with R = {R} "
                         f"(got {tuple(masks.shape) if torch.is_tensor(masks) else type(masks).__name__})")
    return base_weight


def check_watch_args(callback, preview_every, rgb_factors, want_x0, channels):
    """The ValueErrors of `set_watch` / `generate(callback=, preview_every=, preview_factors=)`; returns (W [C][3], preview_every)."""
    preview_every = int(preview_every)
    if callback is not None and not callable(callback):
        raise ValueError("callback must be callable")
    if preview_every < 0:
        raise ValueError(f"preview_every must be >= 0, got {preview_every}")
    if preview_every > 0 and callback is None:
        raise ValueError("preview_every needs a callback to hand the previews to")
    if preview_every > 0 and rgb_factors is None:
        raise ValueError("previews need latent -> RGB factors and no default table ships: fit one from a generation of your checkpoint "
                         "with kandinsky.preview.fit_rgb_factors (test.py --fit_preview_factors OUT.json) and pass it")
    if want_x0 and preview_every == 0:
        raise ValueError("want_x0 needs preview_every > 0: x0 is computed on the preview steps")
    W = None
    if preview_every > 0:
        W = torch.as_tensor(rgb_factors, dtype=torch.float32).cpu().contiguous()
        if tuple(W.shape) != (channels, 3):
            raise ValueError(f"rgb_factors must be [{channels}][3], got {tuple(W.shape)}")
        if channels % 4 or channels > 64:
            raise ValueError(f"previews need a latent of C % 4 == 0 and C <= 64 channels, got {channels}")
    return W, preview_every


def _is_guided(w):
    return abs(w - 1.0) > 1e-6   # the engine's rule (reference generation_utils.py:63)


def _needs_uncond(guidance_weight, plan):
    """Whether a sampling call reads the unconditional prompt: its own weight guides, or a weight of the guidance plan `plan` (`_guidance`) does."""
    return _is_guided(guidance_weight) or (plan is not None and plan[0] is not None and any(_is_guided(w) for w in plan[0]))


# The values the model keeps and pushes into the engine handle, in the order they are re-installed after a rebuild:
# name -> (attribute of the stored value, library setter, the setter's clearing arguments); `_marshal_<name>` turns the stored value into the
# setter's arguments and `set_<name>` is the public method that validates and stores one
_SETTINGS = {
    "watch":         ("_watch",    "k5_dit_set_watch",         (None,)),
    "nag":           ("_nag",      "k5_dit_set_nag",           (None, 1.0, 1.0, 0.0)),
    "regions":       ("_regions",  "k5_dit_set_regions",       (None, 0, None, 0, 0, 0, 0.0)),
    "guidance":      ("_guidance", "k5_dit_set_guidance",      (None,)),
    "skip_guidance": ("_skip",     "k5_dit_set_skip_guidance", (None,)),
    "stochastic":    ("_stochastic", "k5_dit_set_stochastic",  (None,)),
    "enhance":       ("_enhance",  "k5_dit_set_enhance",       (None,)),
    "forecast":      ("_forecast", "k5_dit_set_forecast",      (None,)),
}


class DiffusionTransformer3D(nn.Module):
    def __init__(
        self,
        in_visual_dim=4,
        in_text_dim=3584,
        in_text_dim2=768,
        time_dim=512,
        out_visual_dim=4,
        patch_size=(1, 2, 2),
        model_dim=2048,
        ff_dim=5120,
        num_text_blocks=2,
        num_visual_blocks=32,
        axes_dims=(16, 24, 24),
        visual_cond=False,
    ):
        super().__init__()
        head_dim = sum(axes_dims)
        self.in_visual_dim = in_visual_dim
        self.out_visual_dim = out_visual_dim
        self.model_dim = model_dim
        self.patch_size = tuple(patch_size)
        self.num_visual_blocks = int(num_visual_blocks)
        self.visual_cond = visual_cond
        self._cfg = dict(in_visual_dim=in_visual_dim, in_text_dim=in_text_dim, in_text_dim2=in_text_dim2,
                         time_dim=time_dim, out_visual_dim=out_visual_dim, patch_size=tuple(patch_size),
                         model_dim=model_dim, ff_dim=ff_dim, num_text_blocks=num_text_blocks,
                         num_visual_blocks=num_visual_blocks, axes_dims=tuple(axes_dims), visual_cond=bool(visual_cond))

        visual_embed_dim = 2 * in_visual_dim + 1 if visual_cond else in_visual_dim
        self.visual_embed_dim = visual_embed_dim
        self.time_embeddings = TimeEmbeddings(model_dim, time_dim)
        self.text_embeddings = TextEmbeddings(in_text_dim, model_dim)
        self.pooled_text_embeddings = TextEmbeddings(in_text_dim2, time_dim)
        self.visual_embeddings = VisualEmbeddings(visual_embed_dim, model_dim, patch_size)
        self.text_transformer_blocks = nn.ModuleList(
            [TransformerEncoderBlock(model_dim, time_dim, ff_dim, head_dim) for _ in range(num_text_blocks)])
        self.visual_transformer_blocks = nn.ModuleList(
            [TransformerDecoderBlock(model_dim, time_dim, ff_dim, head_dim) for _ in range(num_visual_blocks)])
        self.out_layer = OutLayer(model_dim, time_dim, out_visual_dim, patch_size)

        self._handle = None          # k5_dit*
        self._handle_device = None
        self._keepalive = []
        self._sp = None              # (rank, world) once a communicator lives on the handle
        self._cfg_pair = None        # CFG-parallel branch (0 / 1) once the pair communicator lives on the handle
        self._settings = {"fp8": False, "graph": False, "options": {}}   # re-applied when the engine is rebuilt
        self._lora = []              # (entries, strength) merged into the ENGINE's packed weights: re-added when the engine is rebuilt
        self._lora_saved = {}        # parameters as they were before a merge done in torch (no engine yet): key -> tensor
        self._watch = None           # (trampoline, k5_watch and the arrays it points to) of set_watch: re-installed when the engine is rebuilt
        self._nag = None             # the negative prompt of set_nag and its three numbers: re-installed likewise
        self._regions = None         # the prompts, masks and base weight of set_regions: likewise
        self._skip = None            # the set of set_skip_guidance (blocks, scale, mode, steps | None): likewise
        self._stochastic = None      # the plan of set_stochastic (dt_down, scale, noise_coef, seed, first_stream): likewise
        self._enhance = None         # (weight, steps | None) of set_enhance: likewise
        self._forecast = None        # (order, full) of set_forecast: likewise
        self._guidance = None        # the plan of set_guidance (weights list | None, zero_star, zero_init_steps, rescale): likewise
        self._borrowed = {}          # setting name -> what the live handle borrows from the stored value (structs, device copies, ctypes arrays)

    # ---------------------------------------------------------------- engine lifetime
    def _destroy_engine(self, force=False):
        if self._handle is not None:
            if (getattr(self, "_sp", None) is not None or getattr(self, "_cfg_pair", None) is not None) and not force:
                # a rank that silently rebuilt its engine would run the unsharded forward while its peers wait in a collective
                raise RuntimeError("this DiffusionTransformer3D holds a live sequence-parallel communicator: replacing its "
                                   "weights or moving it to another device would desynchronise the ranks")
            E.lib().k5_dit_destroy(self._handle)
        self._handle, self._handle_device, self._sp, self._cfg_pair = None, None, None, None
        self._borrowed = {}          # nothing reads them any more

    def __del__(self):
        try:
            self._destroy_engine(force=True)
        except Exception:
            pass

    def _create_handle(self):
        c = self._cfg
        cc = E.DitConfig(c["in_visual_dim"], c["in_text_dim"], c["in_text_dim2"], c["time_dim"], c["out_visual_dim"],
                         (C.c_int * 3)(*c["patch_size"]), c["model_dim"], c["ff_dim"], c["num_text_blocks"],
                         c["num_visual_blocks"], (C.c_int * 3)(*c["axes_dims"]), int(c["visual_cond"]))
        h = C.c_void_p()
        E.check(E.lib().k5_dit_create(C.byref(cc), C.byref(h)), "k5_dit_create")
        return h

    @staticmethod
    def _load_one(handle, name, t):
        t = t.detach()
        if t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            t = t.float()
        t = t.contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        E.check(E.lib().k5_dit_load_tensor(handle, name.encode(), t.data_ptr(), E.k5_dtype(t), shape, t.dim()),
                f"k5_dit_load_tensor({name})")

    def _build_engine(self, device):
        """Pack the current parameters into the HIP engine on `device` (once; rebuilt if the
        parameters are replaced or the module is moved)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the Kandinsky-5 HIP engine runs on an MI355X only (device 'cuda:N'); no CPU path")
        self._destroy_engine()
        with torch.cuda.device(device):
            h = self._create_handle()
            for name, t in self.state_dict().items():
                if t.is_meta:
                    E.lib().k5_dit_destroy(h)
                    raise RuntimeError(f"parameter {name} is on the meta device: load a checkpoint first")
                self._load_one(h, name, t)
            E.check(E.lib().k5_dit_finalize(h), "k5_dit_finalize")
        self._handle, self._handle_device = h, device
        self._reapply_settings()

    def _reapply_settings(self):
        """Engine state that lives on the handle (not in the parameters) survives a rebuild."""
        st = self._settings
        if st["fp8"]:
            E.check(E.lib().k5_dit_set_fp8(self._handle, int(st["fp8"])), "k5_dit_set_fp8")
        if st["graph"]:
            E.check(E.lib().k5_dit_set_graph(self._handle, 1), "k5_dit_set_graph")
        for k, v in st["options"].items():
            if k != "emulate_world":
                E.check(E.lib().k5_dit_set_option(self._handle, k.encode(), int(v)), f"k5_dit_set_option({k})")
        for entries, strength in getattr(self, "_lora", []):   # the rebuilt engine packed the parameters, which an engine-side merge never touched
            self._engine_add_lora(entries, strength)
        for name, (attr, _, _) in _SETTINGS.items():
            if getattr(self, attr, None) is not None:
                self._put(name, getattr(self, attr))
        if getattr(self, "mag_ratios", None) is not None or getattr(self, "_magcache_calibrate", None) is not None:   # set before the weights were loaded / the handle rebuilt
            from ..magcache_utils import _apply
            _apply(self)

    def init_synthetic(self, device, seed=0, std=0.02, qk_gain=1.0, host_rng=False):
        """Random-init weights of this architecture generated tensor by tensor and handed straight to the engine (no 8 GB host
        copy).  Linear ~ N(0,std^2) incl. Modulation (reference zero-inits it, nn.py:158-159, which would make every block an
        identity), norm weights 1, biases N(0,std^2).  Drawn ON DEVICE by default; `host_rng=True` draws every tensor from its own
        CPU generator seeded (seed * 1000003 + index in state_dict order) — the streams a CPU process can reproduce, so that a
        reference run on the host sees the very same weights (bench.py's parity check against tests/golden/dit_fulldepth_c2.*)."""
        device = torch.device(device)
        self._destroy_engine()
        with torch.cuda.device(device):
            h = self._create_handle()
            g = torch.Generator(device="cpu" if host_rng else device)
            for idx, (name, p) in enumerate(self.state_dict().items()):
                g.manual_seed(seed * 1000003 + idx)
                if name.endswith("norm.weight") and len(p.shape) == 1:
                    t = torch.ones(p.shape, device=device)
                    if name.endswith(("query_norm.weight", "key_norm.weight")):
                        t = t * float(qk_gain)   # QK-norm gains of a trained checkpoint are not 1: bench.py --qk-gain
                else:
                    s = std * (2.5 if "modulation" in name else 1.0)
                    if host_rng:
                        t = (torch.randn(p.shape, generator=g) * s).to(device)
                    else:
                        t = torch.randn(p.shape, device=device, generator=g) * s
                self._load_one(h, name, t)
            torch.cuda.synchronize(device)
            E.check(E.lib().k5_dit_finalize(h), "k5_dit_finalize")
        self._handle, self._handle_device = h, device
        self._reapply_settings()
        return self

    def load_state_dict(self, state_dict, strict=True, assign=False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._destroy_engine()
        self._lora, self._lora_saved = [], {}   # adapters belonged to the weights that were just replaced
        return out

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        if self._handle is not None:
            p = next(self.parameters(), None)
            # the engine owns packed copies of the weights: `.to("cpu")` (the pipeline's offload, t2v_pipeline.py) keeps the
            # handle — the next forward on the same GPU costs nothing; only a move to ANOTHER GPU rebuilds
            if p is not None and p.device.type == "cuda" and p.device != self._handle_device:
                self._destroy_engine()
        return out

    def engine(self, device):
        device = torch.device(device)
        if device.index is None and device.type == "cuda":
            device = torch.device("cuda", torch.cuda.current_device())
        if self._handle is None or self._handle_device != device:
            self._build_engine(device)
        return self._handle

    # ---------------------------------------------------------------- argument marshalling
    def _text_cond(self, text_embed, pooled_text_embed, text_rope_pos, keep):
        if text_embed.dtype != pooled_text_embed.dtype:
            pooled_text_embed = pooled_text_embed.to(text_embed.dtype)
        if text_embed.dtype not in (torch.float32, torch.bfloat16):
            text_embed, pooled_text_embed = text_embed.float(), pooled_text_embed.float()
        text_embed, pooled_text_embed = text_embed.contiguous(), pooled_text_embed.contiguous()
        pos = E.i32_array(torch.as_tensor(text_rope_pos).tolist())
        keep += [text_embed, pooled_text_embed, pos]
        if len(pos) != text_embed.shape[0]:
            raise ValueError("text_rope_pos must have one position per text token")
        return E.TextCond(text_embed.data_ptr(), pooled_text_embed.data_ptr(), E.k5_dtype(text_embed),
                          text_embed.shape[0], pos)

    def _forward_args(self, x_shape, x_ptr, x_channels, text_embed, pooled_text_embed, time, visual_rope_pos,
                      text_rope_pos, scale_factor, sparse_params, keep):
        T, H, W = x_shape
        pt, ph, pw = self.patch_size
        pos = [E.i32_array(torch.as_tensor(p).tolist()) for p in visual_rope_pos]
        if (len(pos[0]), len(pos[1]), len(pos[2])) != (T // pt, H // ph, W // pw):
            raise ValueError("visual_rope_pos does not match the latent shape")
        keep += pos
        a = E.ForwardArgs()
        a.x, a.T, a.H, a.W, a.x_channels = x_ptr, T, H, W, x_channels
        a.cond = self._text_cond(text_embed, pooled_text_embed, text_rope_pos, keep)
        a.time = float(time)
        a.pos_t, a.pos_h, a.pos_w = pos
        a.scale_factor = (C.c_float * 3)(*[float(s) for s in scale_factor])
        if sparse_params is not None:
            a.attention_type = 1
            a.nabla_P = float(sparse_params["P"])
            a.nabla_wT, a.nabla_wH, a.nabla_wW = int(sparse_params["wT"]), int(sparse_params["wH"]), int(sparse_params["wW"])
        return a

    # ---------------------------------------------------------------- reference API
    @torch.no_grad()
    def forward(self, x, text_embed, pooled_text_embed, time, visual_rope_pos, text_rope_pos,
                scale_factor=(1.0, 1.0, 1.0), sparse_params=None):
        """Reference signature dit.py:155-165.  x (T,H,W,C_in) ; returns velocity (T,H,W,out_visual_dim) bf16."""
        a, out, keep = self._forward_prologue("forward", x, (), text_embed, pooled_text_embed, time, visual_rope_pos, text_rope_pos, scale_factor,
                                              sparse_params)
        cursor, self._forecast_cursor = getattr(self, "_forecast_cursor", None), None
        if cursor is not None:       # a `forecast_at` from before the engine was built
            self.forecast_at(*cursor)
        return self._call("k5_dit_forward", out, C.byref(a), out.data_ptr())

    def _forward_prologue(self, who, x, lead, text_embed, pooled_text_embed, time, visual_rope_pos, text_rope_pos, scale_factor, sparse_params):
        """What `forward`, `forward_skip` and `forward_many` share for x (..., T, H, W, C_in): the CUDA check, the engine, and (the
        k5_forward_args of x as contiguous fp32 with the prompt moved to its device, the bf16 output `lead` + (T, H, W, out_visual_dim), what
        must stay alive until the call has been made)."""
        if not x.is_cuda:
            raise RuntimeError(f"DiffusionTransformer3D.{who} needs CUDA (HIP) tensors; there is no CPU fallback")
        self.engine(x.device)
        x = x.float().contiguous()
        T, H, W, Cx = x.shape[-4:]
        self._last_tokens = T * (H // self.patch_size[1]) * (W // self.patch_size[2])   # rows of a residual (magcache_calibration)
        t_val = float(time.reshape(-1)[0]) if torch.is_tensor(time) else float(time)
        keep = [x]
        a = self._forward_args((T, H, W), x.data_ptr(), Cx, text_embed.to(x.device), pooled_text_embed.to(x.device), t_val, visual_rope_pos,
                               text_rope_pos, scale_factor, sparse_params, keep)
        return a, torch.empty(*lead, T, H, W, self.out_visual_dim, dtype=torch.bfloat16, device=x.device), keep

    def _call(self, name, on, *args):
        """The library call `name`(handle, *args, stream) on the device and stream of the tensor `on`, which it returns."""
        with torch.cuda.device(on.device):
            E.check(getattr(E.lib(), name)(self._handle, *args, E.stream_ptr(on.device)), name)
        return on

    @torch.no_grad()
    def sample(self, latent, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos,
               null_text_rope_pos, guidance_weight, scale_factor=(1.0, 1.0, 1.0), sparse_params=None, visual_cond=None, edit=None,
               windows=None, window_text=None, flowedit=None, tiles=None):
        """Whole Euler/CFG loop on device (generation_utils.py:80-129) in one C call.  `latent` fp32
        (T,H,W,in_visual_dim) is updated in place; `sigmas` = the sigma schedule (num_steps+1 floats, host).
        `visual_cond` (optional, a model with visual_cond only): contiguous fp32 (T,H,W,in_visual_dim+1) on the latent's device, the
        conditioning latent and its mask that fill the input channels the reference leaves zero (k5_sample_cond); None = k5_sample.
        `edit` (optional): `(source, noise, keep_mask | None)`, contiguous fp32 on the latent's device, source and noise of the latent's
        shape and keep_mask (T,H,W,1): video-to-video / masked editing (k5_sample_edit).  `latent` is then output only: it starts as
        the source noised to sigmas[0] and the kept region (mask 1) is held on the source through every step.
        `windows` (optional): `(starts, weights)` of `generation_utils.context_windows(T, F, overlap)`: a clip longer than the model's trained
        length runs as overlapping temporal windows of F frames whose velocities are cross-faded at every step (k5_sample_windows).
        `visual_rope_pos[0]` and `sparse_params` are then the WINDOW's (F positions), `latent` and `visual_cond` the whole clip's.
        `window_text` (optional, with `windows`): a prompt per window, a list of nwin `(text_embeds, text_rope_pos)` pairs that replaces
        `text_embeds` / `text_rope_pos`.  Not with `edit`; a single-rank model without MagCache only, and a watch without previews.
        `flowedit` (optional): `(source, source_text_embeds, source_text_rope_pos, source_weight, keep_mask | None, refine, seed, first_stream)`:
        FlowEdit (k5_sample_flowedit; the rule is written at k5_flowedit_step_args in include/k5.h).  `source` is the clean source latent,
        the source prompt describes it; `text_embeds` / `guidance_weight` are the target side and the negative prompt serves both.  `sigmas`
        is the cut schedule sigmas[first:] and `first_stream` = first.  `latent` is output only.  Not with `edit` or `windows`.
        `tiles` (optional): the plan of `generation_utils.tile_windows` (anything with its `clip`, `window`, `starts`, `weights`): a frame
        larger than the model's trained size runs as overlapping windows in three axes (k5_sample_tiles).  `visual_rope_pos` and
        `sparse_params` are then the WINDOW's in every axis, `latent` and `visual_cond` the whole clip's; `window_text` is a prompt per window
        of the 3-D plan.  Not with `edit`, `windows` or `flowedit`; refused where `windows` is."""
        if flowedit is not None:
            if edit is not None or windows is not None or tiles is not None:
                raise ValueError("flowedit together with edit, windows or tiles is not supported")
            return self._sample_flowedit(latent, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos,
                                         guidance_weight, scale_factor, sparse_params, visual_cond, flowedit)
        if tiles is not None:
            if edit is not None or windows is not None:
                raise ValueError("tiles together with edit or windows is not supported")
            return self._sample_tiles(latent, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos,
                                      guidance_weight, scale_factor, sparse_params, visual_cond, tiles, window_text)
        if windows is None and window_text is not None:
            raise ValueError("window_text needs windows or tiles")
        if windows is not None:
            if edit is not None:
                raise ValueError("edit together with windows is not supported")
            return self._sample_windows(latent, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos,
                                        guidance_weight, scale_factor, sparse_params, visual_cond, windows, window_text)
        s = E.SampleArgs()
        keep, edit = self._fill_sample_args(s, latent, None, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos,
                                            null_text_rope_pos, guidance_weight, scale_factor, sparse_params, visual_cond, edit)
        if edit is not None:
            ea = E.EditArgs(edit[0].data_ptr(), edit[1].data_ptr(), E.ptr(edit[2]))
            return self._run_sampler("k5_sample_edit", latent, C.byref(s), E.ptr(visual_cond), C.byref(ea))
        if visual_cond is None:
            return self._run_sampler("k5_sample", latent, C.byref(s))
        return self._run_sampler("k5_sample_cond", latent, C.byref(s), visual_cond.data_ptr())

    def _fill_sample_args(self, s, latent, frames, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos,
                          guidance_weight, scale_factor, sparse_params, visual_cond, edit=None, window_hw=None):
        """Check what a k5_sample* call borrows and fill its SampleArgs `s`, for a forward that sees `frames` frames: the latent's T in a plain
        run (`frames` None), F in a window; `window_hw`: the rows and columns it sees where they are not the latent's (a tile).  Returns (what must stay alive as long as `s` is used, the checked `edit` triple or None)."""
        if not latent.is_cuda or latent.dtype != torch.float32 or not latent.is_contiguous():
            raise RuntimeError("latent must be a contiguous fp32 CUDA tensor")
        T, H, W, _ = latent.shape
        frames = T if frames is None else frames
        if window_hw is not None:
            H, W = window_hw
        self._last_tokens = frames * (H // self.patch_size[1]) * (W // self.patch_size[2])   # rows of a residual (magcache_calibration)
        self._check_visual_cond(visual_cond, latent)
        edit = self._check_edit(edit, latent)
        dev = latent.device
        self.engine(dev)
        keep = []
        s.fwd = self._forward_args((frames, H, W), None, self.in_visual_dim, text_embeds["text_embeds"].to(dev), text_embeds["pooled_embed"].to(dev),
                                   0.0, visual_rope_pos, text_rope_pos, scale_factor, sparse_params, keep)
        if _needs_uncond(guidance_weight, getattr(self, "_guidance", None)):
            s.null_cond = self._text_cond(null_text_embeds["text_embeds"].to(dev), null_text_embeds["pooled_embed"].to(dev),
                                          null_text_rope_pos, keep)
        sig = [float(v) for v in sigmas]
        arr = (C.c_float * len(sig))(*sig)
        keep.append(arr)
        s.latent, s.num_steps, s.sigmas, s.guidance_weight = latent.data_ptr(), len(sig) - 1, arr, float(guidance_weight)
        return keep, edit

    def _sample_flowedit(self, latent, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos, guidance_weight,
                         scale_factor, sparse_params, visual_cond, flowedit):
        """`sample(flowedit=...)`: the k5_sample_flowedit call."""
        if not isinstance(flowedit, (tuple, list)) or len(flowedit) != 8:
            raise ValueError("flowedit must be (source, source_text_embeds, source_text_rope_pos, source_weight, keep_mask or None, refine, seed, "
                             "first_stream)")
        source, src_text, src_pos, src_w, keep_mask, refine, seed, first_stream = flowedit
        source, _, keep_mask = self._check_edit((source, source, keep_mask), latent)   # the shape, dtype and device rules of an edit's tensors
        s = E.SampleArgs()
        keep, _ = self._fill_sample_args(s, latent, None, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos,
                                         null_text_rope_pos, guidance_weight, scale_factor, sparse_params, visual_cond)
        dev = latent.device
        if _is_guided(src_w) and not _is_guided(guidance_weight):    # the negative prompt serves the source side alone
            s.null_cond = self._text_cond(null_text_embeds["text_embeds"].to(dev), null_text_embeds["pooled_embed"].to(dev), null_text_rope_pos, keep)
        fa = E.FlowEditArgs(source=source.data_ptr(), source_weight=float(src_w), keep_mask=E.ptr(keep_mask), refine=int(refine),
                            seed=int(seed) & (2 ** 64 - 1), first_stream=int(first_stream) & 0xffffffff)
        # the same tensors as the target prompt give the same pointers: the engine then computes that prompt's prologue once
        fa.source_cond = self._text_cond(src_text["text_embeds"].to(dev), src_text["pooled_embed"].to(dev), src_pos, keep)
        return self._run_sampler("k5_sample_flowedit", latent, C.byref(s), C.byref(fa), E.ptr(visual_cond))

    def flowedit_state(self, reset=False):
        """(steps, forwards, prologues): the FlowEdit steps and forwards the engine has enqueued in `sample(flowedit=...)` calls and the text
        prologues it computed for them, since the last reset (k5_dit_flowedit_state)."""
        return tuple(self._state("k5_dit_flowedit_state", (C.c_longlong, C.c_longlong, C.c_longlong), int(bool(reset))))

    def _run_sampler(self, name, latent, *args):
        """The k5_sample* call `name` on the latent's device and stream, between the watch's begin and end."""
        self._watch_begin()
        self._call(name, latent, *args)
        self._watch_end(latent)
        return latent

    def _sample_windows(self, latent, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos,
                        guidance_weight, scale_factor, sparse_params, visual_cond, windows, window_text):
        """`sample(windows=...)`: the k5_sample_windows call."""
        starts, weights = windows
        starts = [int(v) for v in starts]
        weights = [[float(v) for v in row] for row in weights]
        nwin = len(starts)
        if nwin < 1 or len(weights) != nwin or len({len(r) for r in weights}) != 1:
            raise ValueError("windows must be (starts [nwin], weights [nwin][F])")
        F = len(weights[0])
        if window_text is not None and len(window_text) != nwin:
            raise ValueError(f"window_text holds {len(window_text)} prompts, the plan has nwin = {nwin} windows")
        if window_text is not None:
            text_embeds, text_rope_pos = window_text[0]
        a = E.SampleWindowsArgs()
        keep, _ = self._fill_sample_args(a.sample, latent, F, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos,
                                         null_text_rope_pos, guidance_weight, scale_factor, sparse_params, visual_cond)
        if window_text is not None:
            dev = latent.device
            conds = (E.TextCond * nwin)()
            for i, (te, tp) in enumerate(window_text):
                conds[i] = self._text_cond(te["text_embeds"].to(dev), te["pooled_embed"].to(dev), tp, keep)
            a.conds = conds
        st = E.i32_array(starts)
        wt = (C.c_float * (nwin * F))(*[v for row in weights for v in row])
        a.total_T, a.nwin, a.starts, a.weights = latent.shape[0], nwin, st, wt
        return self._run_sampler("k5_sample_windows", latent, C.byref(a), E.ptr(visual_cond))

    def _sample_tiles(self, latent, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos,
                      guidance_weight, scale_factor, sparse_params, visual_cond, tiles, window_text):
        """`sample(tiles=...)`: the k5_sample_tiles call."""
        starts = [[int(v) for v in s] for s in tiles.starts]
        weights = [torch.as_tensor(w, dtype=torch.float32) for w in tiles.weights]
        window = tuple(int(v) for v in tiles.window)
        if len(starts) != 3 or len(weights) != 3 or any(len(s) < 1 or tuple(w.shape) != (len(s), f) for s, w, f in zip(starts, weights, window)):
            raise ValueError("tiles must hold, per axis (t, y, x), starts [n] and weights [n][F] with F the window's extent")
        if tuple(latent.shape[:3]) != tuple(int(v) for v in tiles.clip):
            raise ValueError(f"tiles were planned for a clip of {tuple(tiles.clip)}, the latent is {tuple(latent.shape[:3])}")
        nwin = len(starts[0]) * len(starts[1]) * len(starts[2])
        if window_text is not None and len(window_text) != nwin:
            raise ValueError(f"window_text holds {len(window_text)} prompts, the plan has nwin = {nwin} windows")
        if window_text is not None:
            text_embeds, text_rope_pos = window_text[0]
        a = E.SampleTilesArgs()
        keep, _ = self._fill_sample_args(a.sample, latent, window[0], sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos,
                                         null_text_rope_pos, guidance_weight, scale_factor, sparse_params, visual_cond, window_hw=window[1:])
        if window_text is not None:
            dev = latent.device
            conds = (E.TextCond * nwin)()
            for i, (te, tp) in enumerate(window_text):
                conds[i] = self._text_cond(te["text_embeds"].to(dev), te["pooled_embed"].to(dev), tp, keep)
            a.conds = conds
        a.total_T, a.total_H, a.total_W = (int(v) for v in latent.shape[:3])
        a.nt, a.ny, a.nx = (len(s) for s in starts)
        st = [E.i32_array(s) for s in starts]
        wt = [(C.c_float * w.numel())(*w.reshape(-1).tolist()) for w in weights]
        a.starts_t, a.starts_y, a.starts_x = st
        a.wt, a.wy, a.wx = wt
        return self._run_sampler("k5_sample_tiles", latent, C.byref(a), E.ptr(visual_cond))

    # ---------------------------------------------------------------- settings on the handle (_SETTINGS): put, clear, state, for one call
    def _put(self, name, value):
        """Store `value` as setting `name`, installed on the handle if there is one.  A refused install raises and changes nothing: the engine
        setters check before they write, so the handle, the stored value and what the handle borrows stay those of the previous setting."""
        attr, fn, _ = _SETTINGS[name]
        if self._handle is not None:     # no engine yet: installed when it is built (_reapply_settings)
            args, keep = getattr(self, "_marshal_" + name)(value)
            with torch.cuda.device(self._handle_device):
                E.check(getattr(E.lib(), fn)(self._handle, *args), fn)
            self._borrowed[name] = (args, keep)     # only now may the previous setting's go
        setattr(self, attr, value)
        return self

    def _clear(self, name):
        attr, fn, clear_args = _SETTINGS[name]
        setattr(self, attr, None)
        if self._handle is not None:
            E.check(getattr(E.lib(), fn)(self._handle, *clear_args), fn)
            self._borrowed.pop(name, None)
        return self

    def _state(self, fn, types, *tail):
        """The out-parameters of the state getter `fn` (ctypes `types`, followed by the arguments `tail`) as values; zeros without a handle."""
        out = [t(0) for t in types]
        if self._handle is not None:
            E.check(getattr(E.lib(), fn)(self._handle, *[C.byref(o) for o in out], *tail), fn)
        return [o.value for o in out]

    @contextlib.contextmanager
    def setting_for_call(self, name, args):
        """Context: setting `name` ("watch", "nag", "regions", "guidance", "skip_guidance", "stochastic", "enhance", "forecast") as `set_<name>(*args)` makes it, for one call; what was
        stored before is installed again afterwards (the stored object itself, not a copy) or the setting is cleared, also on an exception.
        args None: nothing is touched."""
        if args is None:
            yield
            return
        before = getattr(self, _SETTINGS[name][0])
        try:
            getattr(self, "set_" + name)(*args)
            yield
        finally:
            if before is not None:
                self._put(name, before)
            else:
                getattr(self, "clear_" + name)()

    # ---------------------------------------------------------------- watch: progress, cancel, previews
    def set_watch(self, callback=None, preview_every=0, rgb_factors=None, rgb_bias=None, want_x0=False):
        """Progress, cancel and live previews out of `sample` / `sample_many` (k5_dit_set_watch).  `callback(info)` runs after every step on
        the calling thread with a `StepInfo`; a truthy return stops the run and `sample` raises `SamplingInterrupted(steps_done, latent)`,
        an exception raised in the callback stops it too and comes out of `sample` as itself.  `preview_every` = k > 0: the steps with
        (step + 1) % k == 0 and always the last one carry `info.preview`, a CPU uint8 (T,H,W,3) view of the denoised estimate through
        `rgb_factors` [C][3] and `rgb_bias` [3] (`kandinsky.preview.fit_rgb_factors`; no default table ships), and with `want_x0` also
        `info.x0`.  The engine runs one step ahead of the callback, so the GPU never waits for it; the callback must not use this model.
        A single-rank model only: a rank that stops alone would leave its peers inside a collective.  callback None = `clear_watch`."""
        if callback is None:
            return self.clear_watch()
        W, every = check_watch_args(callback, preview_every, rgb_factors, want_x0, self.in_visual_dim)
        if self._sp is not None or self._cfg_pair is not None:
            raise RuntimeError("set_watch: this model is a rank of a sequence-parallel group or a CFG pair; watching is single-rank only "
                               "(a rank that stops alone would leave its peers inside a collective)")
        keep = []
        w = E.Watch()
        tr = E.WatchTrampoline(callback, self._step_info)
        w.fn, w.user, w.preview_every, w.want_x0 = tr.c_fn, None, every, int(bool(want_x0))
        if every > 0:
            wa = (C.c_float * W.numel())(*W.reshape(-1).tolist())
            keep.append(wa)
            w.rgb_w = C.cast(wa, C.POINTER(C.c_float))
            if rgb_bias is not None:
                b = [float(v) for v in torch.as_tensor(rgb_bias, dtype=torch.float32).reshape(-1).tolist()]
                if len(b) != 3:
                    raise ValueError("rgb_bias must hold 3 values")
                ba = (C.c_float * 3)(*b)
                keep.append(ba)
                w.rgb_b = C.cast(ba, C.POINTER(C.c_float))
        return self._put("watch", (tr, w, keep))

    def _marshal_watch(self, watch):
        return (C.byref(watch[1]),), None    # the stored value holds the struct and its arrays itself

    def clear_watch(self):
        """Remove the watch: `sample` enqueues exactly what it did before `set_watch`."""
        return self._clear("watch")

    def watch_state(self):
        """(steps_done, stopped) of the last `sample` / `sample_many` call (k5_dit_watch_state)."""
        n, st = self._state("k5_dit_watch_state", (C.c_int, C.c_int))
        return n, bool(st)

    # ---------------------------------------------------------------- normalized attention guidance: a negative prompt without CFG
    def set_nag(self, text_embeds, text_rope_pos, scale=5.0, tau=2.5, alpha=0.25):
        """A negative prompt inside the cross-attention of ONE forward (k5_dit_set_nag; Normalized Attention Guidance, Chen et al. 2025), for
        runs at guidance 1 where `null_text_embeds` is never read.  `text_embeds` is the dict `generate` takes ("text_embeds" [L][in_text_dim];
        "pooled_embed" is not read: a forward has one time embedding, the positive prompt's) and `text_rope_pos` its L positions.  Every
        conditional forward — `forward`, `forward_many`, the conditional branch of `sample*` — then attends each visual block's queries to the
        positive and to the negative text and joins the outputs: g = z+ + (scale - 1)(z+ - z-), the growth of the token's L1 norm clamped at
        `tau`, blended back with `alpha`.  scale >= 1, tau >= 1, 0 <= alpha <= 1; scale == 1 or alpha == 0 is accepted and means off.  The
        defaults are the values commonly quoted for NAG — starting points, not tuned on any Kandinsky checkpoint.  The model keeps the tensors
        alive until `clear_nag`."""
        scale, tau, alpha = check_nag_args(text_embeds, text_rope_pos, scale, tau, alpha)
        if text_embeds["text_embeds"].shape[1] != self._cfg["in_text_dim"]:
            raise ValueError(f"nag: text_embeds has {text_embeds['text_embeds'].shape[1]} features, the model takes {self._cfg['in_text_dim']}")
        return self._put("nag", {"text": text_embeds["text_embeds"], "pooled": text_embeds.get("pooled_embed"), "pos": text_rope_pos,
                                 "args": (scale, tau, alpha)})

    def _marshal_nag(self, n):
        te = n["text"].to(self._handle_device)
        pe = n["pooled"].to(self._handle_device) if n["pooled"] is not None else te.new_zeros(1, self._cfg["in_text_dim2"])
        keep = []
        cond = self._text_cond(te, pe, n["pos"], keep)
        return (C.byref(cond), *n["args"]), keep     # the engine borrows the struct and what it points to

    def clear_nag(self):
        """Remove the guidance: a forward enqueues exactly what it did before `set_nag`."""
        return self._clear("nag")

    def nag_state(self, reset=False):
        """(on, combines): whether guidance is on, and how many combine launches the engine has enqueued — num_visual_blocks per guided
        forward (k5_dit_nag_state).  `reset` zeroes the count afterwards."""
        on, n = self._state("k5_dit_nag_state", (C.c_int, C.c_longlong), int(bool(reset)))
        return bool(on), n

    # ---------------------------------------------------------------- guidance plan: per-step weights, CFG-Zero*, CFG rescale
    def set_guidance(self, weights=None, zero_star=False, zero_init_steps=0, rescale=0.0):
        """What `sample` / `sample_many` do with the two velocities of a step (k5_dit_set_guidance).  `weights`: one guidance weight per step of
        the calls to come (`generation_utils.guidance_plan` builds it; None = the call's guidance_weight at every step): a step whose weight is
        1 runs the conditional forward alone.  `zero_star`: CFG-Zero* — the unconditional velocity is scaled by <c, u> / <u, u> per sample —
        and `zero_init_steps` = K: the first K steps leave the latent as it is, without a forward.  `rescale` = phi in [0, 1]: CFG rescale,
        v *= phi std(c) / std(v) + 1 - phi.  The statistics are reduced on the device in a fixed order.  `sample` refuses, before anything
        runs: a `weights` list of another length than its steps; a plan with guided and unguided steps, or with zero-init, on a CFG pair or
        with MagCache or its calibration; zero-init with `edit`; any plan with `windows`; zero_star / rescale when every weight is 1.
        No checkpoint was at hand when this was built: the rules are the published ones, their effect on quality is not measured here."""
        return self._put("guidance", check_guidance_args(weights, zero_star, zero_init_steps, rescale))

    def _marshal_guidance(self, plan):
        weights, zero_star, zero_init_steps, rescale = plan
        g = E.Guidance()
        arr = None
        if weights is not None:
            arr = (C.c_float * len(weights))(*weights)    # copied by the call
            g.weights, g.num_weights = C.cast(arr, C.POINTER(C.c_float)), len(weights)
        g.zero_star, g.zero_init_steps, g.rescale = int(zero_star), int(zero_init_steps), float(rescale)
        return (C.byref(g),), arr

    def clear_guidance(self):
        """Remove the plan: `sample` enqueues exactly what it did before `set_guidance`."""
        return self._clear("guidance")

    def guidance_state(self, reset=False):
        """(on, guided, unguided, zero): whether a plan is set, and how many steps of each kind the engine has enqueued under one
        (k5_dit_guidance_state).  `reset` zeroes the counts afterwards."""
        on, *counts = self._state("k5_dit_guidance_state", (C.c_int,) + (C.c_longlong,) * 3, int(bool(reset)))
        return (bool(on), *counts)

    # ---------------------------------------------------------------- skip-layer guidance: a third, block-skipping forward
    def set_skip_guidance(self, blocks, scale, mode="block", steps=None):
        """Skip-layer guidance (k5_dit_set_skip_guidance): at a skip step the conditional forward forks at the first of `blocks` (visual block
        indices) into a branch that skips them — mode "block": the whole block is the identity on the visual stream; "attention": only its
        self-attention residual is dropped — and the step's velocity becomes v_cfg + scale * (c - c_skip).  `steps`: one 0 / 1 per step of the
        calls to come (`generation_utils.skip_plan` builds it; None = every step).  scale == 0 is accepted and means off.  `sample` refuses,
        before anything runs: a `steps` list of another length than its steps, a CFG pair, MagCache or its calibration, and `windows`.
        No checkpoint was at hand when this was built: the rule is the published one, its effect on quality is not measured here."""
        return self._put("skip_guidance", check_skip_args(blocks, scale, mode, steps, self.num_visual_blocks))

    def _marshal_skip_guidance(self, skip):
        blocks, scale, mode, steps = skip
        g = E.SkipGuidance()
        barr = (C.c_int * len(blocks))(*blocks)           # both copied by the call
        g.blocks, g.num_blocks = C.cast(barr, C.POINTER(C.c_int)), len(blocks)
        g.mode, g.scale = SKIP_MODES[mode], float(scale)
        sarr = None
        if steps is not None:
            sarr = (C.c_ubyte * len(steps))(*steps)
            g.steps, g.num_steps = C.cast(sarr, C.POINTER(C.c_ubyte)), len(steps)
        return (C.byref(g),), (barr, sarr)

    def clear_skip_guidance(self):
        """Remove the skip set: `sample` enqueues exactly what it did before `set_skip_guidance`."""
        return self._clear("skip_guidance")

    def skip_state(self, reset=False):
        """(on, skip_steps, blocks_shared, blocks_run): whether skip guidance is on, how many skip steps the engine has enqueued, and how many
        visual blocks the skip branches took from the conditional forward / ran themselves (k5_dit_skip_state).  `reset` zeroes the counts."""
        on, *counts = self._state("k5_dit_skip_state", (C.c_int,) + (C.c_longlong,) * 3, int(bool(reset)))
        return (bool(on), *counts)

    # ---------------------------------------------------------------- stochastic sampling: noise from a counter-based generator inside the update
    def set_stochastic(self, dt_down, scale, noise_coef, seed, first_stream=0):
        """Stochastic sampling in `sample` (k5_dit_set_stochastic): step i takes `dt_down[i]` as its dt and then re-noises,
        x = scale[i] * x + noise_coef[i] * z with z ~ N(0, 1) per element, where noise_coef[i] != 0 (`generation_utils.stochastic_plan` builds the
        three tables from the schedule, a churn eta and a noise scale).  z is not read from anywhere: element g of step i is a pure function of
        (`seed`, `first_stream` + i, g), computed by a Philox4x32-10 generator inside the update kernel, so a captured step replays, every rank
        of a group and both handles of a CFG pair draw the same bits, and a run repeats exactly.  `sample` refuses, before anything runs:
        tables of another length than its steps, `windows`, MagCache or its calibration, a watch with previews; `sample_many` refuses the
        plan (one seed).  No checkpoint was at hand when this was built: the rule is the published one, visual quality is not claimed."""
        return self._put("stochastic", check_stochastic_args(dt_down, scale, noise_coef, seed, first_stream))

    def _marshal_stochastic(self, plan):
        dt_down, scale, coef, seed, first = plan
        p = E.Stochastic()
        arrs = tuple((C.c_float * len(t))(*t) for t in (dt_down, scale, coef))    # copied by the call
        p.num_steps = len(dt_down)
        p.dt_down, p.scale, p.noise_coef = (C.cast(a, C.POINTER(C.c_float)) for a in arrs)
        p.seed, p.first_stream = seed, first
        return (C.byref(p),), arrs

    def clear_stochastic(self):
        """Remove the plan: `sample` enqueues exactly what it did before `set_stochastic`."""
        return self._clear("stochastic")

    def stochastic_state(self, reset=False):
        """(on, noisy_steps): whether a plan is set and how many steps the engine has enqueued that drew noise (k5_dit_stochastic_state).
        `reset` zeroes the count afterwards."""
        on, n = self._state("k5_dit_stochastic_state", (C.c_int, C.c_longlong), int(bool(reset)))
        return bool(on), n

    # ---------------------------------------------------------------- Enhance-A-Video: the cross-frame attention score scales each visual block
    def set_enhance(self, weight, steps=None):
        """Enhance-A-Video (k5_dit_set_enhance; Luo et al. 2025): in every visual block the mean off-diagonal mass of the frame-by-frame
        attention of each spatial position, times (frames + `weight`) and clamped at 1 from below, multiplies the self-attention output.
        Every forward — conditional and unconditional, `forward*` and `sample*` — computes its own scores.  `steps`: one 0 / 1 per step of
        the calls to come (`generation_utils.enhance_plan` builds it; None = every step).  `weight` 0 is a valid weight.  One frame is
        accepted and inert.  `sample` and `forward` refuse, before anything runs: a `steps` list of another length than the call's steps, a
        rank of a sequence-parallel group, more than 64 latent frames per forward.
        No checkpoint was at hand when this was built: the rule is the published one, visual quality is not claimed."""
        return self._put("enhance", check_enhance_args(weight, steps))

    def _marshal_enhance(self, enhance):
        weight, steps = enhance
        e = E.Enhance()
        e.weight = float(weight)
        sarr = None
        if steps is not None:
            sarr = (C.c_ubyte * len(steps))(*steps)           # copied by the call
            e.steps, e.num_steps = C.cast(sarr, C.POINTER(C.c_ubyte)), len(steps)
        return (C.byref(e),), sarr

    def clear_enhance(self):
        """Remove it: a forward enqueues exactly what it did before `set_enhance`."""
        return self._clear("enhance")

    def enhance_state(self, reset=False):
        """(on, launches, scores): whether it is on, how many score launches the engine has enqueued — one per visual block and forward that
        applied it — and the last such forward's per-block scores as a list of floats (k5_dit_enhance_state; it waits for that forward).  A
        score of 1.0 means the clamp held.  `reset` zeroes the count afterwards."""
        if self._handle is None:
            return False, 0, []
        on, n, nb = C.c_int(0), C.c_longlong(0), C.c_int(0)
        cap = self.num_visual_blocks
        buf = (C.c_float * max(cap, 1))()
        with torch.cuda.device(self._handle_device):
            E.check(E.lib().k5_dit_enhance_state(self._handle, C.byref(on), C.byref(n), buf, cap, C.byref(nb), int(bool(reset))),
                    "k5_dit_enhance_state")
        return bool(on.value), n.value, [float(v) for v in buf[:min(nb.value, cap)]]

    # ---------------------------------------------------------------- the forecast cache: skip the visual blocks on a fixed plan of steps
    def set_forecast(self, order, full):
        """The forecast cache (k5_dit_set_forecast; TaylorSeer "lite", Liu et al. 2025).  `full`: one 0 / 1 per step of the calls to come
        (`generation_utils.forecast_plan` builds it), full[0] = 1.  A step with 1 runs its forwards as always and keeps finite differences of
        the residual across the visual blocks, per branch (conditional / unconditional), up to `order` (0, 1 or 2); a step with 0 skips the
        blocks and adds the residual extrapolated to that step.  `sample` / `sample_many` drive it themselves; `forecast_at` is the cursor for
        forwards made one at a time.  A plan without a 0 is off.  Refused, before anything runs: MagCache or its calibration on the model
        (either order); by `sample`: a plan of another length than its steps, skip-layer guidance, a guidance plan with steps of different
        kinds or zero-init, `windows`, a CFG pair.  Memory per branch: n x D x (2 + 4 order) bytes, plus n x D x 2 once.
        No checkpoint was at hand when this was built: the rule is the published one, visual quality is not claimed."""
        return self._put("forecast", check_forecast_args(order, full))

    def _marshal_forecast(self, plan):
        order, full = plan
        p = E.Forecast()
        arr = (C.c_ubyte * len(full))(*full)                  # copied by the call
        p.order, p.full, p.num_steps = order, C.cast(arr, C.POINTER(C.c_ubyte)), len(full)
        return (C.byref(p),), arr

    def clear_forecast(self):
        """Remove the plan and free its buffers: a forward enqueues exactly what it did before `set_forecast`."""
        return self._clear("forecast")

    def forecast_at(self, step, slot=0):
        """The next `forward` is call (`step`, `slot`) of the plan (k5_dit_forecast_at; slot 0 conditional, 1 unconditional); that one forward
        consumes the cursor.  A forward without it is a plain forward and touches no state."""
        if self._forecast is None:
            raise ValueError("forecast_at: no forecast plan (set_forecast)")
        if self._handle is None:     # no engine yet: `forward` builds it and then sets the cursor
            self._forecast_cursor = (int(step), int(slot))
        else:
            E.check(E.lib().k5_dit_forecast_at(self._handle, int(step), int(slot)), "k5_dit_forecast_at")
        return self

    def forecast_state(self, reset=False):
        """(on, full_calls, forecast_calls, state_bytes): whether a plan is set, how many forwards ran their blocks / extrapolated under one,
        and the bytes the history holds now (k5_dit_forecast_state).  `reset` zeroes the counts afterwards."""
        on, *counts = self._state("k5_dit_forecast_state", (C.c_int,) + (C.c_longlong,) * 3, int(bool(reset)))
        return (bool(on), *counts)

    @torch.no_grad()
    def forward_skip(self, x, text_embed, pooled_text_embed, time, visual_rope_pos, text_rope_pos,
                     scale_factor=(1.0, 1.0, 1.0), sparse_params=None):
        """`forward` with the skip branch of `set_skip_guidance` (k5_dit_forward_skip): returns (v_cond, v_skip), v_cond being `forward`'s bits."""
        if getattr(self, "_skip", None) is None:
            raise ValueError("forward_skip: no skip set (set_skip_guidance)")
        a, out, keep = self._forward_prologue("forward_skip", x, (2,), text_embed, pooled_text_embed, time, visual_rope_pos, text_rope_pos,
                                              scale_factor, sparse_params)
        self._call("k5_dit_forward_skip", out, C.byref(a), out[0].data_ptr(), out[1].data_ptr())
        return out[0], out[1]

    # ---------------------------------------------------------------- regional prompts: a prompt per masked region in one forward
    def set_regions(self, text_embeds_list, rope_pos_list, masks, base_weight=0.0):
        """A prompt per masked region inside the cross-attention of ONE forward (k5_dit_set_regions; "attention couple").  `text_embeds_list`:
        1 to 8 dicts as `generate` takes ("text_embeds" [L][in_text_dim]; "pooled_embed" is not read: a forward has one time embedding, the
        base prompt's), `rope_pos_list` their positions, `masks` (R, T, H, W) in [0, 1] on the latent cells (the grid of `keep_mask`;
        `conditioning.region_masks_to_latent` pools pixel masks to it).  Every conditional forward — `forward`, `forward_many`, the
        conditional branch of `sample*` — then attends each visual block's queries to the base prompt and to every region prompt and blends
        the outputs per token: a token's mask value is the mean of its cells, the base prompt weighs base_weight + max(0, 1 - sum of the
        masks), the weights are normalised to sum 1.  An uncovered token sees the base prompt only; masks that partition the frame at
        base_weight 0 give every token exactly one prompt.  The model keeps the tensors alive until `clear_regions`.  `sample(windows=)`
        refuses while regions are set.  No checkpoint was at hand when this was written: what it does to a picture is not claimed."""
        base_weight = check_region_args(text_embeds_list, rope_pos_list, masks, base_weight)
        for r, te in enumerate(text_embeds_list):
            if te["text_embeds"].shape[1] != self._cfg["in_text_dim"]:
                raise ValueError(f"regions: prompt {r} has {te['text_embeds'].shape[1]} features, the model takes {self._cfg['in_text_dim']}")
        pt, ph, pw = self.patch_size
        if masks.shape[1] % pt or masks.shape[2] % ph or masks.shape[3] % pw:
            raise ValueError(f"regions: the masks' shape {tuple(masks.shape[1:])} is not divisible by the patch {(pt, ph, pw)}")
        return self._put("regions", {"text": [te["text_embeds"] for te in text_embeds_list], "pos": list(rope_pos_list), "masks": masks,
                                     "base_weight": base_weight})

    def _marshal_regions(self, g):
        dev = self._handle_device
        keep = []
        R = len(g["text"])
        conds = (E.TextCond * R)()
        for r in range(R):
            te = g["text"][r].to(dev)
            conds[r] = self._text_cond(te, te.new_zeros(1, self._cfg["in_text_dim2"]), g["pos"][r], keep)
        masks = g["masks"].to(device=dev, dtype=torch.float32).contiguous()
        keep.append(masks)
        return (conds, R, E.ptr(masks), *masks.shape[1:], g["base_weight"]), keep    # the engine borrows the array and what it points to

    def clear_regions(self):
        """Remove the regions: a forward enqueues exactly what it did before `set_regions`."""
        return self._clear("regions")

    def regions_state(self, reset=False):
        """(on, R, combines): whether regions are on, how many, and how many combine launches the engine has enqueued — num_visual_blocks per
        regional forward (k5_dit_regions_state).  `reset` zeroes the count afterwards."""
        on, R, n = self._state("k5_dit_regions_state", (C.c_int, C.c_int, C.c_longlong), int(bool(reset)))
        return bool(on), R, n

    def _step_info(self, info):
        shape = (info.T, info.H, info.W)
        preview = x0 = None
        if info.rgb:
            import numpy as np
            preview = torch.from_numpy(np.ctypeslib.as_array(info.rgb, shape=shape + (3,)).copy())   # the pinned slot is reused two steps on
        if info.x0:
            x0 = torch.as_tensor(_DeviceView(C.cast(info.x0, C.c_void_p).value, shape + (info.C,)), device=self._handle_device)
        return StepInfo(info.step, info.num_steps, info.sample, info.num_samples, info.sigma_next, preview, x0)

    def _watch_begin(self):
        if self._watch is not None:
            self._watch[0].reset()

    def _watch_end(self, latent):
        """After a k5_sample* call that returned K5_OK: re-raise what the callback raised, or SamplingInterrupted if it asked to stop."""
        if self._watch is None:
            return
        tr = self._watch[0]
        tr.reraise()
        if tr.stop_requested:
            steps, _ = self.watch_state()
            raise SamplingInterrupted(steps, latent, tr.last_sample)

    def _check_visual_cond(self, visual_cond, latent):
        """visual_cond must be a contiguous fp32 tensor of latent.shape[:-1] + (in_visual_dim + 1,) on the latent's device."""
        if visual_cond is None:
            return
        if not self.visual_cond:
            raise ValueError("visual_cond given to a model built with visual_cond=False")
        want = tuple(latent.shape[:-1]) + (self.in_visual_dim + 1,)
        if not torch.is_tensor(visual_cond) or tuple(visual_cond.shape) != want:
            raise ValueError(f"visual_cond must have shape {want}, got {tuple(getattr(visual_cond, 'shape', ()))}")
        if visual_cond.dtype != torch.float32:
            raise ValueError(f"visual_cond must be float32, got {visual_cond.dtype}")
        if visual_cond.device != latent.device:
            raise ValueError(f"visual_cond must be on {latent.device}, got {visual_cond.device}")
        if not visual_cond.is_contiguous():
            raise ValueError("visual_cond must be contiguous")

    def _check_edit(self, edit, latent):
        """edit = (source, noise, keep_mask | None): contiguous fp32 tensors on the latent's device, source and noise of the latent's shape,
        keep_mask of latent.shape[:-1] + (1,).  Returns the triple (or None)."""
        if edit is None:
            return None
        if not isinstance(edit, (tuple, list)) or len(edit) != 3:
            raise ValueError("edit must be (source, noise, keep_mask or None)")
        want = {"source": tuple(latent.shape), "noise": tuple(latent.shape), "keep_mask": tuple(latent.shape[:-1]) + (1,)}
        for (name, shape), t in zip(want.items(), edit):
            if t is None:
                if name == "keep_mask":
                    continue
                raise ValueError(f"edit {name} is missing")
            if not torch.is_tensor(t) or tuple(t.shape) != shape:
                raise ValueError(f"edit {name} must have shape {shape}, got {tuple(getattr(t, 'shape', ()))}")
            if t.dtype != torch.float32:
                raise ValueError(f"edit {name} must be float32, got {t.dtype}")
            if t.device != latent.device:
                raise ValueError(f"edit {name} must be on {latent.device}, got {t.device}")
            if not t.is_contiguous():
                raise ValueError(f"edit {name} must be contiguous")
        return tuple(edit)

    def many_ready(self):
        """True when `sample_many` / `forward_many` are accepted: a single-rank handle without MagCache or graph replay."""
        return (self._sp is None and self._cfg_pair is None and getattr(self, "mag_ratios", None) is None
                and getattr(self, "_magcache_calibrate", None) is None and not self._settings["graph"])

    @torch.no_grad()
    def sample_many(self, latents, sigmas, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos,
                     guidance_weight, scale_factor=(1.0, 1.0, 1.0), sparse_params=None, visual_cond=None):
        """B samples of one shape in one C call (k5_sample_many).  The samples run one after another inside the engine, at the cost of B
        `sample` calls: a convenience, not a batched kernel path.  `latents` contiguous fp32 (B,T,H,W,in_visual_dim), updated in
        place.  `text_embeds` / `text_rope_pos`: a list of B (a single dict / positions = the same prompt for every sample); likewise
        `null_text_embeds` / `null_text_rope_pos`.  `visual_cond` (optional): fp32 (B,T,H,W,in_visual_dim+1).  Sample b is
        bit-identical to `sample(latents[b], ...)` with its own prompts."""
        if not torch.is_tensor(latents) or latents.dim() != 5:
            raise ValueError(f"latents must be a (B,T,H,W,C) tensor, got {tuple(getattr(latents, 'shape', ()))}")
        if not latents.is_cuda or latents.dtype != torch.float32 or not latents.is_contiguous():
            raise RuntimeError("latents must be a contiguous fp32 CUDA tensor")
        B, T, H, W, _ = latents.shape
        if B < 1:
            raise ValueError("latents must hold at least one sample")
        self._check_visual_cond(visual_cond, latents)

        cfg_on = _needs_uncond(guidance_weight, getattr(self, "_guidance", None))   # a plan's weights may guide where the call's weight is 1
        tes, tps = split_per_sample(text_embeds, B, "text_embeds"), split_per_sample(text_rope_pos, B, "text_rope_pos")
        dev = latents.device
        self.engine(dev)
        keep = []
        conds = (E.TextCond * B)()
        nulls = (E.TextCond * B)() if cfg_on else None
        for b in range(B):
            conds[b] = self._text_cond(tes[b]["text_embeds"].to(dev), tes[b]["pooled_embed"].to(dev), tps[b], keep)
        if cfg_on:
            nes, nps = split_per_sample(null_text_embeds, B, "null_text_embeds"), split_per_sample(null_text_rope_pos, B, "null_text_rope_pos")
            for b in range(B):
                nulls[b] = self._text_cond(nes[b]["text_embeds"].to(dev), nes[b]["pooled_embed"].to(dev), nps[b], keep)
        s = E.SampleManyArgs()
        s.B = B
        s.fwd = self._forward_args((T, H, W), None, self.in_visual_dim, tes[0]["text_embeds"].to(dev), tes[0]["pooled_embed"].to(dev),
                                   0.0, visual_rope_pos, tps[0], scale_factor, sparse_params, keep)
        s.conds, s.null_conds = conds, nulls
        sig = [float(v) for v in sigmas]
        arr = (C.c_float * len(sig))(*sig)
        s.latents, s.visual_cond = latents.data_ptr(), E.ptr(visual_cond)
        s.num_steps, s.sigmas, s.guidance_weight = len(sig) - 1, arr, float(guidance_weight)
        return self._run_sampler("k5_sample_many", latents, C.byref(s))

    @torch.no_grad()
    def forward_many(self, x, text_embeds, time, visual_rope_pos, text_rope_pos, scale_factor=(1.0, 1.0, 1.0),
                      sparse_params=None):
        """S forwards in one C call, one after another (k5_dit_forward_many): x (S,T,H,W,C_in), `text_embeds` / `text_rope_pos` lists
        of S.  Returns velocities (S,T,H,W,out_visual_dim) bf16; sequence i is bit-identical to `forward(x[i], ...)` on the model as it
        was when the call began, and the call leaves the softmax-form memory as it found it."""
        S = x.shape[0]
        if len(text_embeds) != S or len(text_rope_pos) != S:
            raise ValueError(f"text_embeds / text_rope_pos need {S} entries")
        a, out, keep = self._forward_prologue("forward_many", x, (S,), text_embeds[0]["text_embeds"], text_embeds[0]["pooled_embed"], time,
                                              visual_rope_pos, text_rope_pos[0], scale_factor, sparse_params)
        conds = (E.TextCond * S)()
        for i in range(S):
            conds[i] = self._text_cond(text_embeds[i]["text_embeds"].to(x.device), text_embeds[i]["pooled_embed"].to(x.device),
                                       text_rope_pos[i], keep)
        return self._call("k5_dit_forward_many", out, C.byref(a), S, conds, out.data_ptr())

    # ---------------------------------------------------------------- multi-GPU
    def enable_sequence_parallel(self, rank, world, device=None, group=None, src=0, transport=None):
        """Token-sharded sequence parallelism (one process per rank; replaces the reference's DTensor plan,
        kandinsky/models/parallelize.py).  transport "rccl" (default): rank 0 creates the ncclUniqueId inside libk5,
        torch.distributed (already initialised by the launcher, kandinsky/utils.py:40-55 contract) only carries its 128 bytes.
        transport "ipc" (or K5_SP_TRANSPORT=ipc): peers read each other's IPC-mapped slots (k5_dit_comm_init_ipc) — no RCCL, and
        several ranks may share one device; torch.distributed carries the name of the group's shared-memory control block."""
        import os
        if self._handle is None:
            if device is None:
                raise RuntimeError("build the engine first (forward / init_synthetic) or pass device=")
            self.engine(device)
        transport = sp_transport(transport)
        if transport == "ipc":
            name = _broadcast_ipc_name("sp", rank == 0, world, group, src)
            with torch.cuda.device(self._handle_device):
                E.check(E.lib().k5_dit_comm_init_ipc(self._handle, name.encode(), int(rank), int(world)), "k5_dit_comm_init_ipc")
            self._sp = (rank, world)
            return self
        lib_path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        path = lib_path.encode() if os.path.exists(lib_path) else None
        payload = [None]
        if rank == 0:
            uid = C.create_string_buffer(128)
            E.check(E.lib().k5_comm_unique_id(path, uid), "k5_comm_unique_id")
            payload = [uid.raw]
        if world > 1:
            import torch.distributed as dist
            dist.broadcast_object_list(payload, src=src, group=group)   # src = global rank of the group's rank 0
        with torch.cuda.device(self._handle_device):
            E.check(E.lib().k5_dit_comm_init(self._handle, path, int(rank), int(world), payload[0]), "k5_dit_comm_init")
        self._sp = (rank, world)
        return self

    def sp_schedule(self):
        """What the self-tuning sequence-parallel schedule measured and chose on this handle (dict; {} before the first sharded forward
        of a multi-rank handle): k5_dit_sp_schedule."""
        import json
        if self._handle is None:
            return {}
        buf = C.create_string_buffer(8192)
        E.lib().k5_dit_sp_schedule(self._handle, buf, 8192)
        return json.loads(buf.value.decode() or "{}")

    def enable_loopback(self, group, rank):
        """Tests: this handle becomes rank `rank` of a loopback group (`kandinsky._engine.LoopbackGroup`) — several handles of
        one process on one GPU run the sequence-parallel code path of a multi-GPU job, one host thread per rank."""
        if self._handle is None:
            raise RuntimeError("build the engine first")
        with torch.cuda.device(self._handle_device):
            E.check(E.lib().k5_dit_comm_init_loopback(self._handle, group.handle, int(rank)), "k5_dit_comm_init_loopback")
        self._sp = (rank, group.world)
        self._keepalive.append(group)
        return self

    def enable_cfg_pair(self, branch, group=None, src=0, device=None, transport=None):
        """CFG-parallel inside the engine (k5_dit_cfg_pair_init): this rank runs ONE branch of classifier-free guidance in `sample`
        (0 = conditional, 1 = unconditional) and exchanges the velocity with its partner — `group` = the 2-rank torch.distributed
        group of the pair (it only carries the 128-byte id from `src`, the global rank of branch 0).  Call after
        enable_sequence_parallel (both are collective).  transport as in enable_sequence_parallel."""
        import os
        if self._handle is None:
            if device is None:
                raise RuntimeError("build the engine first (forward / init_synthetic) or pass device=")
            self.engine(device)
        if sp_transport(transport) == "ipc":
            name = _broadcast_ipc_name("pair", branch == 0, 2, group, src)
            with torch.cuda.device(self._handle_device):
                E.check(E.lib().k5_dit_cfg_pair_init_ipc(self._handle, name.encode(), int(branch)), "k5_dit_cfg_pair_init_ipc")
            self._cfg_pair = int(branch)
            return self
        lib_path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        path = lib_path.encode() if os.path.exists(lib_path) else None
        payload = [None]
        if branch == 0:
            uid = C.create_string_buffer(128)
            E.check(E.lib().k5_comm_unique_id(path, uid), "k5_comm_unique_id")
            payload = [uid.raw]
        import torch.distributed as dist
        dist.broadcast_object_list(payload, src=src, group=group)
        with torch.cuda.device(self._handle_device):
            E.check(E.lib().k5_dit_cfg_pair_init(self._handle, path, int(branch), payload[0]), "k5_dit_cfg_pair_init")
        self._cfg_pair = int(branch)
        return self

    def enable_cfg_pair_loopback(self, group, branch):
        """Tests: the pair as a loopback group of world 2 (`kandinsky._engine.LoopbackGroup(2)`)."""
        if self._handle is None:
            raise RuntimeError("build the engine first")
        with torch.cuda.device(self._handle_device):
            E.check(E.lib().k5_dit_cfg_pair_init_loopback(self._handle, group.handle, int(branch)), "k5_dit_cfg_pair_init_loopback")
        self._cfg_pair = int(branch)
        self._keepalive.append(group)
        return self

    def set_option(self, name, value):
        """k5_dit_set_option: "attn_mode" (0 = softmax form per head from the data, 1 = online max everywhere),
        "attn_row_offsets" (1 = per-row offsets keep heads with a bound up to 190 on the fixed-offset kernel; default),
        "attn_anchor" (1 = heads beyond that bound keep it too, on offsets anchored at achieved scores; default),
        "attn_fuse_qnorm" (1 = norm_qk + RoPE of the visual queries inside the attention kernel, 2 = under sequence parallelism too;
        default 0, measured neutral),
        "nabla_group_rows" (NABLA on one GPU: 64-query rows per key-tile list / attention workgroup; 0 = by the previous forward's
        kept density (default), 2, 4 — same bits), "sp_nabla_passes" (NABLA under sequence parallelism: 2 = attend the rank's own
        key blocks while the gather is in flight; default 1),
        "sp_slices" (sequence parallelism: exchange K / V^T in this many slices, attend each as it lands; default 1),
        "sp_mode" (sequence parallelism: 0 = K / V^T all-gather (default), 1 = Ulysses all-to-all — token rows traded for heads and back;
        needs heads % ranks == 0 and dense attention, otherwise the gather is used; 2 = two-level — gcd(heads, ranks) head groups x
        ranks / gcd query splits, e.g. 28 heads at 8 ranks: 4 groups of 7 heads x 2 splits; Ulysses where the heads divide, the gather
        where gcd = 1 or for NABLA; K5_SP_MODE=0/1/2 in the ranks' environment sets it at communicator init, this call wins;
        get_option("sp_mode_used") reads what the last sharded forward ran: 0 gather, 1 Ulysses, 2 two-level),
        "sp_pass1_tiles", "emulate_world" (timing only)."""
        if self._handle is not None:     # no engine yet: remembered and applied when it is built (_reapply_settings)
            E.check(E.lib().k5_dit_set_option(self._handle, name.encode(), int(value)), f"k5_dit_set_option({name})")
        self._settings["options"][name] = int(value)
        return self

    def reset_softmax_memory(self):
        """Forget which heads the per-row-offset softmax served badly ("attn_pref_reset"): a speed hint that is valid from one step to
        the next of ONE sampling run.  `sample` (k5_sample) does it by itself; a caller stepping `forward` itself calls this per run,
        so that the same seed on the same handle gives the same bits whatever the handle computed before."""
        if self._handle is not None:
            E.check(E.lib().k5_dit_set_option(self._handle, b"attn_pref_reset", 1), "k5_dit_set_option(attn_pref_reset)")
        return self

    def get_option(self, name):
        if self._handle is None:
            if name in self._settings["options"]:
                return self._settings["options"][name]
            raise RuntimeError("get_option before the engine is built: only options set through set_option are known")
        v = C.c_int()
        E.check(E.lib().k5_dit_get_option(self._handle, name.encode(), C.byref(v)), f"k5_dit_get_option({name})")
        return v.value

    def attn_variant_counts(self, reset=False):
        """(fixed-offset, online-max) head launches of the visual self-attention since the last reset."""
        a, b = C.c_longlong(), C.c_longlong()
        E.check(E.lib().k5_dit_attn_variant_counts(self._handle, C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value

    def nabla_block_counts(self):
        """(kept, possible) 64x64 blocks of the NABLA maps computed while profiling was on (bench.py: realised density)."""
        a, b = C.c_longlong(), C.c_longlong()
        E.check(E.lib().k5_dit_nabla_block_counts(self._handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_nabla_tap(self, buf=None):
        """Diagnostics: every NABLA map computed from now on (one-GPU path) is expanded to uint8 [H][nb][nb] into `buf` (a CUDA uint8 tensor the
        caller keeps alive), one after the other; None removes the tap."""
        if buf is not None and (not buf.is_cuda or buf.dtype != torch.uint8 or not buf.is_contiguous()):
            raise ValueError("the NABLA tap needs a contiguous CUDA uint8 tensor")
        self._nabla_tap = buf
        E.check(E.lib().k5_dit_set_nabla_tap(self._handle, E.ptr(buf), 0 if buf is None else buf.numel()), "k5_dit_set_nabla_tap")

    def nabla_tap_count(self):
        a = C.c_longlong()
        E.check(E.lib().k5_dit_nabla_tap_count(self._handle, C.byref(a)), "k5_dit_nabla_tap_count")
        return a.value

    def nabla_executed_blocks(self):
        """64x64 blocks the list-driven attention executed for those maps (union lists x rows per list): kept / executed = union efficiency."""
        a = C.c_longlong()
        E.check(E.lib().k5_dit_nabla_executed_blocks(self._handle, C.byref(a)))
        return a.value

    def set_fp8(self, on=True):
        """opt-in, lossy: linear layers of the visual blocks in W8A8 e4m3 (k5_dit_set_fp8; BASELINE config 5).  `on`: True / 1 = the
        feed-forward GEMMs; a bit mask adds 2 = the q | k | V^T projections and 4 = the out projection of the visual self-attention
        (7 = all three); False / 0 = off."""
        mask = int(on) if not isinstance(on, bool) else (1 if on else 0)
        E.check(E.lib().k5_dit_set_fp8(self._handle, mask), "k5_dit_set_fp8")
        self._settings["fp8"] = mask
        return self

    # ---------------------------------------------------------------- LoRA adapters
    def _engine_add_lora(self, entries, strength):
        from ..lora import lora_scale
        with torch.cuda.device(self._handle_device):
            for key, (A, B, alpha) in entries.items():
                A, B = [t.detach() if t.dtype in E._DT else t.detach().float() for t in (A, B)]
                A, B = A.contiguous(), B.contiguous()
                E.check(E.lib().k5_dit_add_lora(self._handle, key.encode(), A.data_ptr(), E.k5_dtype(A), B.data_ptr(), E.k5_dtype(B),
                                                int(A.shape[0]), lora_scale(strength, alpha, A.shape[0])), f"k5_dit_add_lora({key})")

    @torch.no_grad()
    def add_lora(self, adapter, strength=1.0):
        """Merge a LoRA adapter into the weights: `adapter` is a .safetensors path, a state dict of adapter tensors (peft, diffusers or kohya
        names, kandinsky/lora.py) or what `load_lora` returned; the scale is strength * alpha / R (strength alone without an alpha).  With the
        engine built, the packed weights are updated in place (k5_dit_add_lora: no upload, no re-pack; the parameters stay as loaded).  Before
        the engine exists the same merge is done on the parameters in torch, in fp32, and the engine packs the merged weights when it is
        built.  Several adapters add up in call order; `clear_lora` undoes them all."""
        from ..lora import load_lora, lora_scale, merge_torch
        sd = self.state_dict()
        entries = adapter if _is_loaded_lora(adapter) else load_lora(adapter, known_keys=sd.keys())
        for key, (A, B, alpha) in entries.items():
            if key not in sd:
                raise KeyError(f"LoRA module {key[:-7]!r}: the model has no {key}")
            want = tuple(sd[key].shape)
            if sd[key].dim() != 2 or (B.shape[0], A.shape[1]) != want or not 1 <= A.shape[0] <= 256:
                raise ValueError(f"LoRA adapter for {key}: A {tuple(A.shape)} / B {tuple(B.shape)} do not fit the weight {want} "
                                 "(B [out][R], A [R][in], 1 <= R <= 256)")
        if self._handle is not None:
            self._engine_add_lora(entries, strength)
            self._lora.append((entries, float(strength)))
            return self
        for key, (A, B, alpha) in entries.items():
            p = sd[key]
            if p.is_meta:
                raise RuntimeError(f"parameter {key} is on the meta device: load a checkpoint first")
            self._lora_saved.setdefault(key, p.detach().clone())
            p.copy_(merge_torch(p, A, B, lora_scale(strength, alpha, A.shape[0])))
        return self

    @torch.no_grad()
    def clear_lora(self):
        """Undo every `add_lora`: the engine copies its backups of the packed weights back (k5_dit_clear_lora), parameters merged in torch get
        their saved values back (an engine packed from them in between is rebuilt on next use)."""
        if self._handle is not None and self._lora:
            with torch.cuda.device(self._handle_device):
                E.check(E.lib().k5_dit_clear_lora(self._handle), "k5_dit_clear_lora")
        self._lora = []
        if self._lora_saved:
            sd = self.state_dict()
            for key, saved in self._lora_saved.items():
                sd[key].copy_(saved)
            self._lora_saved = {}
            self._destroy_engine()
        return self

    def lora_state(self):
        """{"adapters": add_lora calls in effect, "matrices": weights with a saved copy, "backup_bytes": what those copies hold} —
        the engine's own count (k5_dit_lora_state) plus the parameters saved by a merge in torch."""
        n, b = self._state("k5_dit_lora_state", (C.c_int, C.c_longlong))
        saved = self._lora_saved
        return {"adapters": len(self._lora) + (1 if saved else 0), "matrices": n + len(saved),
                "backup_bytes": b + sum(t.numel() * t.element_size() for t in saved.values())}

    def set_graph(self, on=True):
        """sample() replays one hipGraph-captured step (k5_dit_set_graph); bit-identical results"""
        E.check(E.lib().k5_dit_set_graph(self._handle, int(on)))
        self._settings["graph"] = bool(on)
        return self

    # ---------------------------------------------------------------- profiling (bench.py roofline)
    def set_profiling(self, on=True):
        E.check(E.lib().k5_dit_set_profiling(self._handle, int(on)))

    def reset_profile(self):
        E.check(E.lib().k5_dit_reset_profile(self._handle))

    def get_profile(self, family):
        ms, n = C.c_double(), C.c_int64()
        E.check(E.lib().k5_dit_get_profile(self._handle, family.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


def _is_loaded_lora(adapter):
    """what `kandinsky.lora.load_lora` returns: {engine key: (A, B, alpha)}"""
    return isinstance(adapter, dict) and all(isinstance(v, tuple) and len(v) == 3 for v in adapter.values()) and len(adapter) > 0


def get_dit(conf):
    """reference dit.py:184-186"""
    conf = dict(conf) if not isinstance(conf, dict) else conf
    return DiffusionTransformer3D(**conf)
