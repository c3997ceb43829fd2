"""Sampler — host mirror of kandinsky/generation_utils.py (same function names and signatures).

`generate` keeps the reference's positional signature (generation_utils.py:81-96) and its noise /
sigma-schedule construction, but runs the Euler / CFG loop on the MI355X engine: in one C call
(`DiffusionTransformer3D.sample` -> k5_sample, k5_sample_cond with visual conditioning) when `model` is the engine-backed
DiT, otherwise step by
step through `model(...)` (duck-typed models, e.g. a MagCache wrapper) with the fused CFG+Euler kernel.
"""
import contextlib
import math
import os

os.environ.setdefault("TOKENIZERS_PARALLELISM", "False")

import torch

from . import _engine as E
from .models.dit import (DiffusionTransformer3D, SamplingInterrupted, StepInfo, _is_guided, check_guidance_args, check_nag_args,
                         check_enhance_args, check_nag_numbers, check_region_args, check_skip_args, check_stochastic_args, check_watch_args, split_per_sample)


def _attr(obj, name, default=None):
    if isinstance(obj, dict):
        return obj.get(name, default)
    return getattr(obj, name, default)


def get_sparse_params(conf, batch_embeds, device):
    """reference generation_utils.py:10-36.  The STA mask itself is rebuilt on device by the engine from
    (wT, wH, wW); the dict keeps the reference's keys so callers can introspect it."""
    patch = conf.model.dit_params.patch_size
    assert patch[0] == 1
    T, H, W, _ = batch_embeds["visual"].shape
    T, H, W = T // patch[0], H // patch[1], W // patch[2]
    attn = conf.model.attention
    if _attr(attn, "type") == "nabla":
        if H % 8 or W % 8:
            raise ValueError("nabla attention needs latent height/width divisible by 16 (8x8 token tiles)")
        return {
            "sta_mask": None,  # built inside the engine
            "attention_type": _attr(attn, "type"),
            "to_fractal": True,
            "P": _attr(attn, "P"),
            "wT": _attr(attn, "wT"),
            "wW": _attr(attn, "wW"),
            "wH": _attr(attn, "wH"),
            "add_sta": _attr(attn, "add_sta"),
            "visual_shape": (T, H, W),
            "method": _attr(attn, "method", "topcdf"),
        }
    return None


@torch.no_grad()
def get_velocity(dit, x, t, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos,
                 guidance_weight, conf, sparse_params=None):
    """reference generation_utils.py:39-77 (two forwards + bf16 CFG combine)."""
    pred_velocity = dit(x, text_embeds["text_embeds"], text_embeds["pooled_embed"], t * 1000, visual_rope_pos,
                        text_rope_pos, scale_factor=conf.metrics.scale_factor, sparse_params=sparse_params)
    if _is_guided(guidance_weight):
        uncond_pred_velocity = dit(x, null_text_embeds["text_embeds"], null_text_embeds["pooled_embed"], t * 1000,
                                   visual_rope_pos, null_text_rope_pos, scale_factor=conf.metrics.scale_factor,
                                   sparse_params=sparse_params)
        pred_velocity = uncond_pred_velocity + guidance_weight * (pred_velocity - uncond_pred_velocity)
    return pred_velocity


def sigma_schedule(num_steps, scheduler_scale, device="cpu"):
    """reference generation_utils.py:102-103"""
    timesteps = torch.linspace(1, 0, num_steps + 1, device=device)
    return scheduler_scale * timesteps / (1 + (scheduler_scale - 1) * timesteps)


def edit_first_step(num_steps, strength):
    """Video-to-video `strength` in (0, 1] -> the first step that runs: run = min(num_steps, max(1, floor(num_steps * strength + 0.5)))
    steps, the tail of the schedule, so first = num_steps - run (strength 1 = the whole schedule)."""
    strength = float(strength)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength must be in (0, 1], got {strength}")
    run = min(int(num_steps), max(1, int(math.floor(num_steps * strength + 0.5))))
    return int(num_steps) - run


def _interval(name, interval):
    """`(lo, hi)` of the keyword `name` as two floats with lo <= hi; None = every sigma."""
    if interval is None:
        return -math.inf, math.inf
    try:
        lo, hi = (float(v) for v in interval)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be (lo, hi)") from None
    if not lo <= hi:
        raise ValueError(f"{name} must be (lo, hi) with lo <= hi, got ({lo}, {hi})")
    return lo, hi


def guidance_plan(sigmas, guidance_weight, guidance_schedule=None, guidance_interval=None):
    """The per-step guidance weights of a run over `sigmas` (num_steps + 1 values, step i goes from sigmas[i] to sigmas[i + 1]): a list of
    num_steps floats.  `guidance_schedule`: a list of num_steps weights, or a callable `(i, sigma_i) -> weight`; None = `guidance_weight` at
    every step.  `guidance_interval` = (lo, hi) (Kynkaanniemi et al. 2024): the weight stays on the steps with lo <= sigmas[i] <= hi and is
    1 elsewhere, where the sampler then runs the conditional forward alone.  Host only."""
    sig = [float(v) for v in sigmas]
    n = len(sig) - 1
    if n < 1:
        raise ValueError("guidance_plan: sigmas must hold num_steps + 1 >= 2 values")
    if guidance_schedule is None:
        weights = [float(guidance_weight)] * n
    elif callable(guidance_schedule):
        weights = [float(guidance_schedule(i, sig[i])) for i in range(n)]
    else:
        weights = [float(w) for w in guidance_schedule]
        if len(weights) != n:
            raise ValueError(f"guidance_schedule holds {len(weights)} weights, the run has {n} steps")
    if not all(math.isfinite(w) for w in weights):
        raise ValueError("guidance_plan: every weight must be a finite number")
    lo, hi = _interval("guidance_interval", guidance_interval)
    return [w if lo <= sig[i] <= hi else 1.0 for i, w in enumerate(weights)]


def _guidance_for_run(model, sigmas, first, guidance_weight, guidance_schedule, guidance_interval, cfg_zero_star, cfg_zero_init, cfg_rescale,
                      init_latent, windowed):
    """`generate`'s guidance keywords -> None when all are off (nothing changes), otherwise (weights of the steps that run | None, zero_star,
    zero_init_steps, rescale) with the ValueErrors of what the engine refuses.  `sigmas`: the full schedule, of which steps `first`.. run."""
    if guidance_schedule is None and guidance_interval is None and not cfg_zero_star and not cfg_zero_init and not cfg_rescale:
        return None
    weights = None
    if guidance_schedule is not None or guidance_interval is not None:
        weights = guidance_plan(sigmas, guidance_weight, guidance_schedule, guidance_interval)[first:]   # cut with the schedule
    weights, zero_star, zero_init, rescale = check_guidance_args(weights, cfg_zero_star, cfg_zero_init, cfg_rescale)
    per_step = weights if weights is not None else [float(guidance_weight)] * (len(sigmas) - 1 - first)
    guided = [_is_guided(w) for w in per_step]
    if windowed:
        raise ValueError("guidance_schedule / guidance_interval / cfg_zero_star / cfg_zero_init / cfg_rescale together with context windows "
                         "are not supported: one statistic per window is not the published rule")
    if (zero_star or rescale > 0.0) and not any(guided):
        raise ValueError("cfg_zero_star / cfg_rescale at a run whose every guidance weight is 1: there is nothing to guide")
    if zero_init > 0 and init_latent is not None:
        raise ValueError("cfg_zero_init together with init_latent (editing) is not supported")
    if zero_init > 0 or (any(guided) and not all(guided)):
        if _has_magcache(model):
            raise ValueError("a guidance plan with guided and unguided steps, or with cfg_zero_init, with MagCache: the ratio table is indexed "
                             "by the call of a plain run")
        if _is_cfg_pair(model):
            raise ValueError("a guidance plan with guided and unguided steps, or with cfg_zero_init, on a CFG pair: the unconditional group "
                             "would have steps with nothing to exchange")
    return weights, zero_star, zero_init, rescale


def skip_plan(sigmas, slg_interval=None):
    """The per-step mask of skip-layer guidance over `sigmas` (num_steps + 1 values): a list of num_steps 0 / 1, 1 on the steps with
    lo <= sigmas[i] <= hi of `slg_interval` = (lo, hi); None = every step.  Host only, like `guidance_plan`."""
    sig = [float(v) for v in sigmas]
    n = len(sig) - 1
    if n < 1:
        raise ValueError("skip_plan: sigmas must hold num_steps + 1 >= 2 values")
    lo, hi = _interval("slg_interval", slg_interval)
    return [1 if lo <= sig[i] <= hi else 0 for i in range(n)]


def _skip_for_run(model, sigmas, first, slg_blocks, slg_scale, slg_interval, slg_mode, windowed):
    """`generate`'s skip-layer-guidance keywords -> None when they are off (no blocks, scale 0 or an interval without a step: nothing changes),
    otherwise (blocks, scale, mode, mask of the steps that run) with the ValueErrors of what the engine refuses.  `sigmas`: the full schedule,
    of which steps `first`.. run."""
    if slg_blocks is None and not slg_scale and slg_interval is None:
        return None
    nb = getattr(model, "num_visual_blocks", None)   # a wrapped model that does not say is checked by the engine
    mask = skip_plan(sigmas, slg_interval)[first:]   # cut with the schedule
    if slg_blocks is None or len(slg_blocks) == 0:
        check_skip_args([0], slg_scale, slg_mode, mask, 1)   # the numbers are still checked
        return None
    blocks, scale, mode, mask = check_skip_args(slg_blocks, slg_scale, slg_mode, mask, nb if nb is not None else max(int(b) for b in slg_blocks) + 1)
    if scale == 0.0 or not any(mask):
        return None
    if windowed:
        raise ValueError("slg_blocks together with context windows is not supported: a windowed step has one velocity pair per window")
    if _has_magcache(model):
        raise ValueError("slg_blocks with MagCache: the ratio table is indexed by the call of a plain run")
    if _is_cfg_pair(model):
        raise ValueError("slg_blocks on a CFG pair: the pair exchanges two velocities, a skip step has three")
    return blocks, scale, mode, mask


def forecast_plan(num_steps, interval, warmup=None, tail=1, order=1):
    """The forecast cache's plan: full[num_steps] of 0 / 1, 1 = the step runs its visual blocks, 0 = their residual is extrapolated
    (`DiffusionTransformer3D.set_forecast`).  full[i] = 1 if i < warmup, or i >= num_steps - tail, or (i - warmup) % interval == 0.
    `warmup` None = max(order + 1, int(0.2 * num_steps)), MagCache's retention share and enough full steps for the differences of `order`.
    warmup >= 1, tail >= 0, interval >= 1.  interval == 1, or a plan without a 0, means off.  Host only, like `guidance_plan`."""
    num_steps, interval, tail, order = int(num_steps), int(interval), int(tail), int(order)
    if num_steps < 1:
        raise ValueError(f"forecast_plan: num_steps must be >= 1 (got {num_steps})")
    if interval < 1:
        raise ValueError(f"forecast_interval must be >= 1 (got {interval})")
    if not 0 <= order <= 2:
        raise ValueError(f"forecast_order must be 0, 1 or 2 (got {order})")
    warmup = max(order + 1, int(0.2 * num_steps)) if warmup is None else int(warmup)
    if warmup < 1:
        raise ValueError(f"forecast_warmup must be >= 1 (got {warmup}): the first step has nothing to extrapolate from")
    if tail < 0:
        raise ValueError(f"forecast_tail must be >= 0 (got {tail})")
    return [1 if i < warmup or i >= num_steps - tail or (i - warmup) % interval == 0 else 0 for i in range(num_steps)]


def _forecast_for_run(model, steps_run, forecast_interval, forecast_order, forecast_warmup, forecast_tail, guide, skip, windowed):
    """`generate`'s forecast keywords -> None when they are off (no interval, interval 1, or a plan without a 0: nothing changes), otherwise
    (order, full) over the `steps_run` steps the run executes (an edit run: those after its cut) with the ValueErrors of what the engine
    refuses.  `guide`, `skip`: the run's checked guidance plan and skip set; `windowed`: more than one context window."""
    if forecast_interval is None:
        return None
    order = forecast_order
    if isinstance(order, bool) or not isinstance(order, int) or not 0 <= order <= 2:
        raise ValueError(f"forecast_order must be 0, 1 or 2 (got {order!r})")
    full = forecast_plan(steps_run, forecast_interval, forecast_warmup, forecast_tail, order)
    if all(full):
        return None
    if _has_magcache(model):
        raise ValueError("forecast_interval with MagCache (or its calibration) on the model: one cache at a time")
    if skip is not None:
        raise ValueError("forecast_interval together with slg_blocks is not supported: the skip branch has no slot in the cache")
    if guide is not None and (guide[2] > 0 or (guide[0] is not None and len({_is_guided(w) for w in guide[0]}) > 1)):
        raise ValueError("forecast_interval together with a guidance plan that has guided and unguided steps (guidance_schedule / "
                         "guidance_interval) or cfg_zero_init is not supported: the unconditional slot would have gaps")
    if windowed:
        raise ValueError("forecast_interval together with context windows (context_frames) is not supported: a windowed step makes a call "
                         "per window, the cache holds one residual per branch")
    if _is_cfg_pair(model):
        raise ValueError("forecast_interval on a CFG pair is not supported")
    if not (hasattr(model, "set_forecast") and hasattr(model, "forecast_at")):
        raise ValueError("forecast_interval needs a model with set_forecast and forecast_at (the engine-backed DiffusionTransformer3D has "
                         "them): the cache lives inside its forward, a wrapped callable without them cannot take it")
    return order, full


@contextlib.contextmanager
def _forecast_for_call(model, forecast):
    """The plan on the model for exactly one run; what was there before comes back, also on an exception.  forecast None: nothing is touched.
    The engine-backed model does it itself (`setting_for_call`); a wrapper that hands `set_forecast`, `clear_forecast` and `_forecast` on to
    one is served through those."""
    if forecast is None:
        yield
    elif hasattr(model, "setting_for_call"):
        with model.setting_for_call("forecast", forecast):
            yield
    else:
        before = getattr(model, "_forecast", None)
        try:
            model.set_forecast(*forecast)
            yield
        finally:
            if before is not None:
                model.set_forecast(*before)
            else:
                model.clear_forecast()


def enhance_plan(sigmas, interval=None):
    """The per-step mask of Enhance-A-Video over `sigmas` (num_steps + 1 values): a list of num_steps 0 / 1, 1 on the steps with
    lo <= sigmas[i] <= hi of `interval` = (lo, hi); None = every step.  Host only, like `skip_plan`."""
    sig = [float(v) for v in sigmas]
    n = len(sig) - 1
    if n < 1:
        raise ValueError("enhance_plan: sigmas must hold num_steps + 1 >= 2 values")
    lo, hi = _interval("enhance_interval", interval)
    return [1 if lo <= sig[i] <= hi else 0 for i in range(n)]


def _enhance_for_run(model, sigmas, first, enhance_weight, enhance_interval, frames):
    """`generate`'s Enhance-A-Video keywords -> None when they are off (no weight, or an interval without a step: nothing changes), otherwise
    (weight, mask of the steps that run) with the ValueErrors of what the engine refuses.  `sigmas`: the full schedule, of which steps
    `first`.. run; `frames`: the latent frames one forward sees (a context window's length).  0.0 is a valid weight."""
    if enhance_weight is None:
        if enhance_interval is not None:
            raise ValueError("enhance_interval needs enhance_weight")
        return None
    weight, mask = check_enhance_args(enhance_weight, enhance_plan(sigmas, enhance_interval)[first:])   # cut with the schedule
    if not any(mask):
        return None
    if getattr(model, "_sp", None) is not None:
        raise ValueError("enhance_weight on a rank of a sequence-parallel group: the frames of a column live on different ranks")
    if int(frames) > 64:
        raise ValueError(f"enhance_weight: {int(frames)} latent frames per forward are more than the score kernel holds (64)")
    if not hasattr(model, "set_enhance"):
        raise ValueError("enhance_weight needs a model with set_enhance (the engine-backed DiffusionTransformer3D has it): the score is taken "
                         "inside its self-attention, a wrapped callable without one cannot take it")
    return weight, mask


@contextlib.contextmanager
def _enhance_for_call(model, enhance):
    """What `set_enhance` left on a model comes back after a run that set it step by step or for the call, also on an exception.  enhance None:
    nothing is touched.  A wrapper that only hands `set_enhance`, `clear_enhance` and `_enhance` on to an engine-backed model is served too."""
    if enhance is None:
        yield
        return
    before = getattr(model, "_enhance", None)
    try:
        yield
    finally:
        if before is not None:
            model.set_enhance(*before)
        else:
            model.clear_enhance()


def _enhance_at(model, enhance, i):
    """The per-step paths' side: step i's forwards apply the score (weight, every forward) or are the plain forwards, as the engine's loop
    decides it from the mask."""
    if enhance is None:
        return
    if enhance[1][i]:
        model.set_enhance(enhance[0])
    else:
        model.clear_enhance()


@contextlib.contextmanager
def _skip_for_call(model, skip):
    """A skip set on a model that takes one (`set_skip_guidance`) for exactly one run; what was there before comes back, also on an exception.
    skip None, or a model without `set_skip_guidance`: nothing is touched.  The engine-backed model does it itself (`setting_for_call`); a
    wrapper that only hands `set_skip_guidance`, `clear_skip_guidance` and `_skip` on to one is served through those."""
    if skip is None or not hasattr(model, "set_skip_guidance"):
        yield
    elif hasattr(model, "setting_for_call"):
        with model.setting_for_call("skip_guidance", skip):
            yield
    else:
        before = getattr(model, "_skip", None)
        try:
            model.set_skip_guidance(*skip)
            yield
        finally:
            if before is not None:
                model.set_skip_guidance(*before)
            else:
                model.clear_skip_guidance()


def stochastic_plan(sigmas, eta, s_noise=1.0, interval=None):
    """The per-step tables of stochastic sampling over `sigmas` (num_steps + 1 values): `(dt_down, scale, noise_coef)`, three lists of
    num_steps fp32 values.  Flow matching is x_sigma = (1 - sigma) x0 + sigma eps; step i goes from s = sigmas[i] to t = sigmas[i + 1] and,
    with churn `eta` in [0, 1] and noise scale `s_noise`,
        sigma_down = t (1 + (t / s - 1) eta)        a = (1 - t) / (1 - sigma_down)        c = s_noise sqrt(max(0, t^2 - (sigma_down a)^2))
    the sampler takes the Euler step to sigma_down (dt_down = sigma_down - s) and then x = a x + c z with z ~ N(0, 1): at eta = s_noise = 1
    the marginal is that of x_t.  Computed in float64 and rounded once to fp32.  `interval` = (lo, hi): only the steps with
    lo <= sigmas[i] <= hi are stochastic; None = every step.  A step that is not (eta 0, outside the interval, c == 0 — the last step, where
    t = 0, always) gets scale exactly 1, noise_coef 0 and as dt_down the fp32 difference sigmas[i + 1] - sigmas[i] the engine forms itself: the
    plain step, bit for bit.  Host only, like `guidance_plan`."""
    sig = [float(v) for v in sigmas]
    n = len(sig) - 1
    if n < 1:
        raise ValueError("stochastic_plan: sigmas must hold num_steps + 1 >= 2 values")
    try:
        eta, s_noise = float(eta), float(s_noise)
    except (TypeError, ValueError):
        raise ValueError("stochastic_plan: eta and s_noise must be numbers") from None
    if not 0.0 <= eta <= 1.0:   # also a NaN
        raise ValueError(f"eta must be in [0, 1], got {eta}")
    if not math.isfinite(s_noise) or s_noise < 0.0:
        raise ValueError(f"s_noise must be a finite number >= 0, got {s_noise}")
    lo, hi = _interval("sde_interval", interval)
    f32 = torch.tensor(sig, dtype=torch.float32)
    dt = (f32[1:] - f32[:-1]).tolist()   # the engine's own fp32 difference
    dt_down, scale, coef = [], [], []
    for i in range(n):
        s, t = sig[i], sig[i + 1]
        a = c = 0.0
        if eta > 0.0 and lo <= s <= hi and s > 0.0:
            down = t * (1.0 + (t / s - 1.0) * eta)
            if 1.0 - down > 0.0:
                a = (1.0 - t) / (1.0 - down)
                c = s_noise * math.sqrt(max(0.0, t * t - (down * a) ** 2))
                c = float(torch.tensor(c, dtype=torch.float64).to(torch.float32))
        if c == 0.0:
            step = (dt[i], 1.0, 0.0)
        else:
            step = (float(torch.tensor(down - s, dtype=torch.float64).to(torch.float32)), float(torch.tensor(a, dtype=torch.float64).to(torch.float32)), c)
        for table, value in zip((dt_down, scale, coef), step):
            table.append(value)
    return dt_down, scale, coef


def _stochastic_for_run(model, sigmas, first, eta, s_noise, sde_interval, sde_seed, windowed, preview_every):
    """`generate`'s stochastic keywords -> None when they are off (eta 0, or no step draws noise: nothing changes), otherwise the checked plan
    (dt_down, scale, noise_coef of the steps that run, seed, first stream 0) with the ValueErrors of what the engine refuses.  `sigmas`: the
    full schedule, of which steps `first`.. run."""
    dt_down, scale, coef = (t[first:] for t in stochastic_plan(sigmas, eta, s_noise, sde_interval))   # cut with the schedule
    plan = check_stochastic_args(dt_down, scale, coef, sde_seed, 0)
    if not any(coef):
        return None
    if windowed:
        raise ValueError("eta > 0 together with context windows is not supported: the windowed update has no noise term")
    if _has_magcache(model):
        raise ValueError("eta > 0 with MagCache: the ratio table was measured on ODE trajectories")
    if preview_every:
        raise ValueError("eta > 0 with preview_every > 0: the preview reads x0 = x - sigma_next v, which no longer holds after the noise is added "
                         "(a callback with preview_every = 0 — progress and cancel — works)")
    return plan


def context_windows(T, frames, overlap):
    """The plan of a long clip sampled as temporal context windows: `(starts, weights)` for T latent frames, windows of `frames` = F frames
    and 0 <= `overlap` < F.  T <= F: one window of T frames with weight 1.  Otherwise nwin = ceil((T - overlap) / (F - overlap)) windows
    evenly spread, starts[i] = (i * (T - F)) // (nwin - 1), so the first starts at 0 and the last ends at T.  weights (float32 tensor
    [nwin][F]): local frame j of a window weighs the triangle min(j + 1, F - j), normalised over the windows that cover the frame (float64,
    rounded once), so the shares of every frame sum to 1 and the windows cross-fade where they overlap.  ValueError for nwin > 64."""
    T, F, overlap = int(T), int(frames), int(overlap)
    if T < 1 or F < 1:
        raise ValueError(f"context_windows: T and frames must be >= 1, got T={T}, frames={F}")
    if not 0 <= overlap < F:
        raise ValueError(f"context_windows: overlap must be in [0, frames), got overlap={overlap} with frames={F}")
    if T <= F:
        return [0], torch.ones(1, T, dtype=torch.float32)
    nwin = -(-(T - overlap) // (F - overlap))
    if nwin > 64:
        raise ValueError(f"context_windows: T={T}, frames={F}, overlap={overlap} needs nwin = {nwin} windows, at most 64 are supported")
    starts = [(i * (T - F)) // (nwin - 1) for i in range(nwin)]
    raw = torch.tensor([min(j + 1, F - j) for j in range(F)], dtype=torch.float64)
    total = torch.zeros(T, dtype=torch.float64)
    for st in starts:
        total[st:st + F] += raw
    weights = torch.stack([raw / total[st:st + F] for st in starts]).to(torch.float32)
    return starts, weights


class TileWindows:
    """The plan of `tile_windows`: `clip` = (T, H, W) and `window` = (Ft, Fh, Fw) in latent cells (a window never exceeds the clip), `starts` =
    (st, sy, sx) lists of cell starts, `weights` = (wt [nt][Ft], wy [ny][Fh], wx [nx][Fw]) float32 tensors, `counts` = (nt, ny, nx), `nwin`.
    Window k = (it * ny + iy) * nx + ix: t-major, then rows, then columns."""

    def __init__(self, clip, window, overlap, starts, weights):
        self.clip, self.window, self.overlap, self.starts, self.weights = tuple(clip), tuple(window), tuple(overlap), tuple(starts), tuple(weights)
        self.counts = tuple(len(s) for s in self.starts)
        self.nwin = self.counts[0] * self.counts[1] * self.counts[2]

    def corner(self, k):
        """(t0, y0, x0): the cell at which window k begins."""
        nt, ny, nx = self.counts
        return self.starts[0][k // (ny * nx)], self.starts[1][(k // nx) % ny], self.starts[2][k % nx]

    def box(self, k):
        """The three slices of window k in the clip."""
        return tuple(slice(s, s + f) for s, f in zip(self.corner(k), self.window))

    def __repr__(self):
        return f"TileWindows(clip={self.clip}, window={self.window}, overlap={self.overlap}, counts={self.counts})"


def tile_windows(clip, window, overlap):
    """The plan of a large clip sampled as overlapping windows in three axes: the product of three `context_windows` plans.  `clip` = (T, H, W),
    `window` = (Ft, Fh, Fw), `overlap` = (ot, oh, ow), all in latent cells.  The temporal axis is planned in frames.  The two spatial axes are
    planned in PATCHES of 2 cells — extents, windows and overlaps must be even — so `context_windows(H / 2, Fh / 2, oh / 2)` gives patch starts and
    per-patch weights: a cell start is twice the patch start and both cells of a patch carry its weight.  An axis whose window is at least the
    extent has one window of weight 1.  Each axis is normalised on its own, so the shares rn(rn(wt wy) wx) of a cell sum to 1 up to fp32
    rounding.  ValueError for odd spatial sizes and for nwin = nt ny nx > 64.  Returns a TileWindows."""
    (T, H, W), (Ft, Fh, Fw), (ot, oh, ow) = (tuple(int(v) for v in a) for a in (clip, window, overlap))
    for name, v in (("H", H), ("W", W), ("window height", Fh), ("window width", Fw), ("overlap (rows)", oh), ("overlap (columns)", ow)):
        if v & 1:
            raise ValueError(f"tile_windows: {name} = {v} is odd: the spatial axes are planned in patches of 2 cells")
    Ft, Fh, Fw = min(Ft, T), min(Fh, H), min(Fw, W)
    st, wt = context_windows(T, Ft, ot if T > Ft else 0)
    axes = []
    for n, F, o in ((H, Fh, oh), (W, Fw, ow)):
        ps, pw = context_windows(n // 2, F // 2, o // 2 if n > F else 0)
        axes.append(([2 * s for s in ps], pw.repeat_interleave(2, dim=1).contiguous()))
    plan = TileWindows((T, H, W), (Ft, Fh, Fw), (ot, oh, ow), (list(st), axes[0][0], axes[1][0]), (wt, axes[0][1], axes[1][1]))
    if plan.nwin > 64:
        raise ValueError(f"tile_windows: clip {plan.clip} as windows of {plan.window} with overlap {plan.overlap} needs nwin = "
                         f"{plan.counts[0]} x {plan.counts[1]} x {plan.counts[2]} = {plan.nwin} windows, at most 64 are supported")
    return plan


def _even_down(v):
    return int(v) // 2 * 2


def _plan_for(model, clip, context, init_latent, preview_every):
    """`generate`'s context keywords `context` = (frames, overlap, text, height, width, overlap_hw) for a sample of `clip` = (T, H, W) latent
    cells -> the TileWindows of the run, or None for a plain run: no keyword, or one window and no `context_text`.  `context_frames` alone
    is the 3-D plan with one row window and one column window of weight 1 over `context_windows(T, frames, overlap)`.  The ValueErrors of the
    combinations that are refused name the keywords the caller gave and are raised before the model is touched."""
    frames, overlap, text, height, width, overlap_hw = context
    T, H, W = (int(v) for v in clip)
    if height is None and width is None:
        if overlap_hw is not None:
            raise ValueError("context_overlap_hw needs context_height / context_width")
        if frames is None:
            if overlap is not None or text is not None:
                raise ValueError("context_overlap / context_text need context_frames")
            return None
        what, F = "context_frames", int(frames)
        ot = F // 4 if overlap is None else int(overlap)
        starts, weights = context_windows(T, F, ot)
        tiles = TileWindows((T, H, W), (min(F, T), H, W), (ot, 0, 0), (starts, [0], [0]), (weights, torch.ones(1, H), torch.ones(1, W)))
    else:
        what = "context_height / context_width"
        if overlap is not None and frames is None:
            raise ValueError("context_overlap needs context_frames")
        Ft = T if frames is None else min(int(frames), T)
        Fh, Fw = (n if v is None else min(int(v), n) for v, n in ((height, H), (width, W)))
        if overlap_hw is None:   # a quarter of the window, rounded down to even
            oh, ow = _even_down(Fh // 4), _even_down(Fw // 4)
        else:
            oh, ow = (int(v) for v in ((overlap_hw, overlap_hw) if isinstance(overlap_hw, int) else overlap_hw))
        tiles = tile_windows((T, H, W), (Ft, Fh, Fw), (Ft // 4 if overlap is None else int(overlap), oh, ow))
    if text is not None and len(text) != tiles.nwin:
        raise ValueError(f"context_text holds {len(text)} prompts, the plan {tiles!r} has nwin = {tiles.nwin} windows")
    if tiles.nwin == 1:   # the plain run; with context_text the plan stays, for its one prompt
        return None if text is None else tiles
    if init_latent is not None:
        raise ValueError(f"init_latent (editing) together with {what} is not supported")
    if int(preview_every) > 0:
        raise ValueError(f"preview_every > 0 together with {what} is not supported: the preview reads one velocity pair per cell")
    if _has_magcache(model):
        raise ValueError(f"{what} with MagCache: the ratio table is indexed by the call of a plain run")
    if _is_multi_rank_engine(model) or getattr(model, "_cfg_parallel", None) is not None:
        raise ValueError(f"{what} needs a single-rank model (no sequence-parallel group, no CFG pair)")
    return tiles


def _has_magcache(model):
    """True when the model (or a module inside a wrapper) carries a MagCache ratio table or is calibrating one."""
    mods = list(model.modules()) if isinstance(model, torch.nn.Module) else [model]
    return any(getattr(m, "mag_ratios", None) is not None or getattr(m, "_magcache_calibrate", None) is not None for m in mods)


def _is_cfg_pair(model):
    """True when the model is one branch of classifier-free guidance: an engine-side CFG pair or the CFG-parallel of a wrapped model."""
    return getattr(model, "_cfg_pair", None) is not None or getattr(model, "_cfg_parallel", None) is not None


def _check_edit_args(model, shape, init_latent, strength, keep_mask):
    """The ValueErrors of `generate`'s editing keywords."""
    edit_first_step(1, strength)   # strength in (0, 1]
    if init_latent is None:
        if float(strength) < 1.0:
            raise ValueError("strength < 1 needs init_latent (the clip to start from)")
        if keep_mask is not None:
            raise ValueError("keep_mask needs init_latent (the clip whose region is kept)")
        return
    if tuple(init_latent.shape) != tuple(shape):
        raise ValueError(f"init_latent must be {tuple(shape)}, got {tuple(init_latent.shape)}")
    if keep_mask is not None and tuple(keep_mask.shape) != tuple(shape[:-1]) + (1,):
        raise ValueError(f"keep_mask must be {tuple(shape[:-1]) + (1,)}, got {tuple(keep_mask.shape)}")
    if float(strength) < 1.0 and _has_magcache(model):
        raise ValueError("strength < 1 with MagCache: the ratio table is indexed by the step of a full run, a truncated schedule would "
                         "read the wrong rows (a keep_mask at strength 1 is allowed)")


def _is_multi_rank_engine(model):
    return type(model) is DiffusionTransformer3D and (model._sp is not None or model._cfg_pair is not None)


def flowedit_plan(num_steps, strength, refine=0):
    """The kind of every step of a FlowEdit run (Kulikov et al. 2024; the rule is written at k5_flowedit_step_args in include/k5.h): "skipped"
    for i < first = edit_first_step(num_steps, strength), "flowedit" for first <= i < num_steps - refine, "plain" for the last `refine`
    steps.  ValueError for a refine outside 0 .. num_steps - first."""
    first = edit_first_step(num_steps, strength)
    if isinstance(refine, bool) or not isinstance(refine, int) or not 0 <= refine <= num_steps - first:
        raise ValueError(f"flowedit_refine must be an integer in 0..{num_steps - first} (the steps that run), got {refine!r}")
    return ["skipped"] * first + ["flowedit"] * (num_steps - first - refine) + ["plain"] * refine


def _flowedit_for_run(model, num_steps, strength, init_latent, keep_mask, guidance_weight, seed, source_text_embeds, source_text_rope_pos,
                      source_guidance_weight, flowedit_refine, flowedit_seed, refused):
    """The ValueErrors of `generate`'s FlowEdit keywords; returns None without a source prompt, otherwise (source_text_embeds,
    source_text_rope_pos, source weight, refine, seed).  `refused`: (name, whether it was asked for) of what does not go with FlowEdit."""
    if source_text_embeds is None:
        if source_text_rope_pos is not None or source_guidance_weight is not None or flowedit_refine or flowedit_seed is not None:
            raise ValueError("source_text_rope_pos / source_guidance_weight / flowedit_refine / flowedit_seed need source_text_embeds (the prompt "
                             "that describes the source clip)")
        return None
    if init_latent is None:
        raise ValueError("source_text_embeds (FlowEdit) needs init_latent (the clip to edit)")
    if source_text_rope_pos is None:
        raise ValueError("source_text_embeds needs source_text_rope_pos")
    refine = flowedit_plan(num_steps, strength, flowedit_refine).count("plain")
    if refine > 0 and keep_mask is not None:
        raise ValueError("flowedit_refine > 0 together with keep_mask is not supported: the keep rule of a plain step needs an eps this mode "
                         "does not have")
    w_src = float(guidance_weight if source_guidance_weight is None else source_guidance_weight)
    if not math.isfinite(w_src):
        raise ValueError(f"source_guidance_weight must be a finite number, got {source_guidance_weight}")
    for name, asked in refused:
        if asked:
            raise ValueError(f"{name} together with source_text_embeds (FlowEdit) is not supported: a FlowEdit step runs the source and the "
                             "target side's forwards and its own update")
    if _has_magcache(model):
        raise ValueError("source_text_embeds (FlowEdit) with MagCache: the ratio table is indexed by the call of a plain run")
    if _is_multi_rank_engine(model) or _is_cfg_pair(model):
        raise ValueError("source_text_embeds (FlowEdit) needs a single-rank model (no sequence-parallel group, no CFG pair)")
    return source_text_embeds, source_text_rope_pos, w_src, refine, int(seed if flowedit_seed is None else flowedit_seed)


class _StepWatch:
    """`generate`'s progress bar and callback as one per-step hook, shared by the fused path (installed as the engine's watch) and the
    per-step Python paths (called from the loop), so a callback sees the same sequence whichever ran."""

    def __init__(self, model, callback, preview_every, preview_factors, want_x0, progress, total, channels):
        from .preview import as_factors
        W, b = as_factors(preview_factors)
        self.W, self.every = check_watch_args(callback, preview_every, W, want_x0, channels)
        self.b = None if (b is None or self.W is None) else torch.as_tensor(b, dtype=torch.float32).reshape(-1)
        self.callback, self.want_x0 = callback, bool(want_x0)
        self.sample, self.num_samples = 0, 1
        self.bar = None
        if _is_multi_rank_engine(model):
            if callback is not None:
                raise ValueError("callback= needs a single-rank model: on a sequence-parallel group or a CFG pair a rank that stops alone "
                                 "would leave its peers inside a collective (watching is single-rank only)")
        elif progress:
            try:
                from tqdm import tqdm
                self.bar = tqdm(total=int(total))
            except ImportError:   # progress is a courtesy: without tqdm there is simply no bar
                self.bar = None
        self.active = callback is not None or self.bar is not None

    def preview_at(self, i, n):
        return self.every > 0 and ((i + 1) % self.every == 0 or i == n - 1)

    def step(self, info):
        if self.num_samples > 1 and info.num_samples == 1:   # samples that run as calls of their own (generate(batch=) off the many-sample path)
            info.sample, info.num_samples = self.sample, self.num_samples
        if self.bar is not None:
            self.bar.update(1)
        return bool(self.callback(info)) if self.callback is not None else False

    def close(self):
        if self.bar is not None:
            self.bar.close()
            self.bar = None

    def watch_args(self):
        """This hook as the arguments of `set_watch` for one sample / sample_many call of an engine-backed model (`setting_for_call`); None
        when there is nothing to watch."""
        return (self.step, self.every, self.W, self.b, self.want_x0) if self.active else None


def _nag_for_call(model, nag_text_embeds, nag_text_rope_pos, nag_scale, nag_tau, nag_alpha):
    """`generate`'s NAG keywords, checked, as the model's context for exactly one call.  nag_scale None: nothing is touched."""
    if nag_scale is None:
        return contextlib.nullcontext()
    check_nag_args(nag_text_embeds, nag_text_rope_pos, nag_scale, nag_tau, nag_alpha)
    if type(model) is not DiffusionTransformer3D:
        raise ValueError("nag_scale needs the engine-backed DiffusionTransformer3D: normalized attention guidance runs inside its "
                         "forward, a wrapped or duck-typed model has no hook for it")
    return model.setting_for_call("nag", (nag_text_embeds, nag_text_rope_pos, nag_scale, nag_tau, nag_alpha))


def _regions_for_call(model, region_text_embeds, region_text_rope_pos, region_masks, region_base_weight):
    """`generate`'s region keywords, checked, as the model's context for exactly one call.  region_text_embeds None: nothing is touched."""
    if region_text_embeds is None:
        return contextlib.nullcontext()
    check_region_args(region_text_embeds, region_text_rope_pos, region_masks, region_base_weight)
    if type(model) is not DiffusionTransformer3D:
        raise ValueError("region_text_embeds needs the engine-backed DiffusionTransformer3D: regional prompts run inside its forward, a "
                         "wrapped or duck-typed model has no hook for them")
    return model.setting_for_call("regions", (region_text_embeds, region_text_rope_pos, region_masks, region_base_weight))


def _conditioning(model, img, visual_cond, visual_cond_mask):
    """`(vc, vm)` of img's shape and of img.shape[:-1] + (1,), fp32 on img's device, from `visual_cond` / `visual_cond_mask` (zeros for the one
    that is missing); None when neither is given."""
    if visual_cond is None and visual_cond_mask is None:
        return None
    if not getattr(model, "visual_cond", False):
        raise ValueError("visual_cond / visual_cond_mask need a model built with visual_cond=True")
    mask_shape = tuple(img.shape[:-1]) + (1,)
    vc = torch.zeros_like(img) if visual_cond is None else visual_cond.to(device=img.device, dtype=torch.float32)
    vm = (torch.zeros(mask_shape, dtype=torch.float32, device=img.device) if visual_cond_mask is None
          else visual_cond_mask.to(device=img.device, dtype=torch.float32))
    if tuple(vc.shape) != tuple(img.shape) or tuple(vm.shape) != mask_shape:
        raise ValueError(f"visual_cond must be {tuple(img.shape)} and visual_cond_mask {mask_shape}, got {tuple(vc.shape)} and "
                         f"{tuple(vm.shape)}")
    return vc, vm


def _model_input(model, img, cond_in, frames=slice(None)):
    """What a per-step forward is given for `frames` of the latent: latent | conditioning | mask (zeros for the last two when none was
    given) for a visual_cond model, the bare latent otherwise."""
    x = img[frames]
    if not getattr(model, "visual_cond", False):
        return x
    if cond_in is None:
        return torch.cat([x, torch.zeros_like(x), torch.zeros([*x.shape[:-1], 1], dtype=x.dtype, device=x.device)], dim=-1)
    return torch.cat([x, cond_in[0][frames], cond_in[1][frames]], dim=-1)


@torch.no_grad()
def generate(model, device, shape, num_steps, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos,
             null_text_rope_pos, guidance_weight, scheduler_scale, conf, progress=False, seed=6554, noise=None, *,
             visual_cond=None, visual_cond_mask=None, batch=1, init_latent=None, strength=1.0, keep_mask=None,
             callback=None, preview_every=0, preview_factors=None, preview_x0=False, context_frames=None, context_overlap=None,
             context_text=None, nag_text_embeds=None, nag_text_rope_pos=None, nag_scale=None, nag_tau=2.5, nag_alpha=0.25,
             region_text_embeds=None, region_text_rope_pos=None, region_masks=None, region_base_weight=0.0,
             guidance_schedule=None, guidance_interval=None, cfg_zero_star=False, cfg_zero_init=0, cfg_rescale=0.0,
             slg_blocks=None, slg_scale=0.0, slg_interval=None, slg_mode="block", eta=0.0, s_noise=1.0, sde_interval=None, sde_seed=None,
             enhance_weight=None, enhance_interval=None, forecast_interval=None, forecast_order=1, forecast_warmup=None, forecast_tail=1,
             source_text_embeds=None, source_text_rope_pos=None, source_guidance_weight=None, flowedit_refine=0, flowedit_seed=None,
             context_height=None, context_width=None, context_overlap_hw=None):
    """reference generation_utils.py:80-129.  `noise` (optional, extension) overrides the seeded draw.
    `context_height`, `context_width`, `context_overlap_hw` (optional, extension): a frame larger than the model's trained size, next to
    `context_frames` / `context_overlap` and in the same unit, latent cells.  The sample runs at every step on the overlapping windows of
    `tile_windows((T, H, W), (context_frames, context_height, context_width), overlaps)` — `context_overlap_hw` an int or a (rows, columns)
    pair, default a quarter of the window rounded down to even — each window with the first entries of `visual_rope_pos` as its positions,
    and one k5_cfg_euler_tiles pass cross-fades the windows' velocities into the update.  `context_text` is then one prompt per window of
    the 3-D plan (t-major, rows, columns).  The engine-backed model runs the whole loop in one call (k5_sample_tiles), any other callable
    runs each forward on a contiguous copy of its window and gives the same bits.  Refused in the combinations `context_frames` refuses;
    `context_frames` alone is this plan with one row window and one column window of weight 1, on the same path.
    `visual_cond` (T,H,W,in_visual_dim) and `visual_cond_mask` (T,H,W,1) (optional, extension; `conditioning.py` builds them) fill
    the conditioning channels of a visual_cond model that the reference's loop leaves zero; either alone means zeros for the other.
    `batch` (extension): `shape` = (batch*T, H, W, C) holds `batch` samples of T frames, sample b = frames [bT, (b+1)T) of the
    one noise draw of the full shape (and of visual_cond / visual_cond_mask).  `text_embeds`, `null_text_embeds` and their rope
    positions are then one value shared by all samples or a list of `batch`.  Every sample is bit-identical to a call of its own
    with its noise slice: a single-rank engine DiT runs them in one k5_sample_many call, any other model one after another.
    `init_latent`, `strength`, `keep_mask` (optional, extension): video-to-video and masked editing.  `init_latent` (shape) is the clean
    latent of the source clip (`conditioning.encode_video`), the drawn or passed `noise` is the eps it is noised with: the loop starts
    from (1 - sigma) * init_latent + sigma * noise at step `first = edit_first_step(num_steps, strength)` and runs the tail of the
    schedule.  `keep_mask` (shape[:-1] + (1,)) in [0, 1]: where it is 1 the result is `init_latent` bit for bit, the rest is
    generated around it (the kept region is re-imposed at every step's sigma on the device).  strength = 1 without a mask is the
    plain run on `noise`, bit for bit.  With batch > 1 the samples run one at a time.
    `progress` draws a tqdm bar over batch x steps when tqdm is installed (nothing otherwise, and nothing on a multi-rank engine model).
    `callback`, `preview_every`, `preview_factors`, `preview_x0` (optional, extension): `callback(info)` runs after every step with a
    `kandinsky.models.dit.StepInfo`; a truthy return stops the run (`SamplingInterrupted` carries steps_done and the latent), an exception
    comes out as itself.  `preview_every` = k > 0 puts a CPU uint8 (T,H,W,3) `info.preview` of the denoised estimate on the steps with
    (step + 1) % k == 0 and on the last one, through `preview_factors` (a JSON path or (W [C][3], b [3]); `kandinsky.preview`;
    no default table ships), and with `preview_x0` the estimate itself as `info.x0` (device, valid during the call).  The engine-backed
    model keeps its in-engine loop (k5_dit_set_watch: the callback runs one step behind the GPU); the per-step paths call back from their
    Python loop with the same kernel, so the sequence and the preview bits are the same.  ValueError on a multi-rank engine model.
    `context_frames`, `context_overlap`, `context_text` (optional, extension): a clip longer than the model's trained length.  With
    `context_frames` = F below the sample's T frames the model runs at every step on the overlapping windows of `context_windows(T, F,
    context_overlap)` (overlap default F // 4) and the windows' velocities are cross-faded into one update (k5_cfg_euler_tiles);
    `visual_rope_pos[0]` (its first F entries when it holds the clip's) and the NABLA parameters are the window's.  `context_text`: a
    list of nwin `(text_embeds, text_rope_pos)` pairs, a prompt per window in order, instead of `text_embeds` / `text_rope_pos`.  F >= T
    is the plain run, bit for bit.  The engine-backed model runs the whole loop in one call (k5_sample_tiles), any other callable the
    same forwards in the same order from Python.  ValueError with init_latent, preview_every > 0, MagCache or a multi-rank model.
    `nag_scale`, `nag_tau`, `nag_alpha`, `nag_text_embeds`, `nag_text_rope_pos` (optional, extension): normalized attention guidance, a
    negative prompt inside the cross-attention of the conditional forward (`DiffusionTransformer3D.set_nag`) — the way to a negative
    prompt at guidance_weight 1, where `null_text_embeds` is never read.  `nag_scale` None (default) is off and nothing changes;
    otherwise `nag_text_embeds` (a dict like `text_embeds`) and `nag_text_rope_pos` are the negative prompt, one for every sample and
    window.  Set on the model for this call and removed afterwards, also when the call raises; every rank of a group or a CFG pair
    passes the same values.  The unconditional forward of a CFG run is not touched.  5 / 2.5 / 0.25 are the values commonly quoted for
    NAG: starting points, not tuned on any Kandinsky checkpoint.  ValueError on a model without the engine (wrapped or duck-typed).
    `region_text_embeds`, `region_text_rope_pos`, `region_masks`, `region_base_weight` (optional, extension): regional prompts, a prompt
    per masked region inside the cross-attention of the conditional forward (`DiffusionTransformer3D.set_regions`).  `region_text_embeds`
    None (default) is off and nothing changes; otherwise a list of 1 to 8 dicts like `text_embeds`, `region_text_rope_pos` their positions
    and `region_masks` (R, T, H, W) in [0, 1] on one sample's latent cells (`conditioning.region_masks_to_latent`); `text_embeds` is the base
    prompt, which uncovered cells see alone and which weighs `region_base_weight` in [0, 1] under the regions.  One region set for every
    sample of a batch.  Set on the model for this call and removed afterwards, also when the call raises; every rank of a group or a CFG
    pair passes the same values.  The unconditional forward of a CFG run is not touched.  ValueError on a model without the engine and
    together with `context_frames` below the clip's length (the masks cover the clip, a window sees a slice).
    `guidance_schedule`, `guidance_interval`, `cfg_zero_star`, `cfg_zero_init`, `cfg_rescale` (optional, extension): what the sampler does
    with the two velocities of a step; all off (default) nothing changes.  `guidance_schedule` (a list of num_steps weights or a callable
    `(i, sigma_i)`) and `guidance_interval` = (lo, hi) give every step its own weight (`guidance_plan`); a step whose weight is 1 runs the
    conditional forward alone, so an interval saves one forward on every step outside it.  With strength < 1 the plan is that of the full
    schedule, cut with it.  `cfg_zero_star`: CFG-Zero* (Fan et al. 2025), the unconditional velocity scaled by <c, u> / <u, u> per sample,
    and `cfg_zero_init` = K: the first K steps leave the latent as it is.  `cfg_rescale` = phi in [0, 1]: CFG rescale (Lin et al. 2024),
    v *= phi std(c) / std(v) + 1 - phi.  The engine-backed model runs them inside its loop (`DiffusionTransformer3D.set_guidance`, set for
    this call and removed afterwards), any other model through the same two kernels from the per-step loop: the same bits.  ValueError
    together with context windows; for cfg_zero_star / cfg_rescale when every weight is 1; for cfg_zero_init with init_latent; for a plan
    with guided and unguided steps or cfg_zero_init with MagCache or on a CFG pair.  No checkpoint was at hand when this was built: the
    rules are the published ones, their effect on quality is not measured here.

    `slg_blocks`, `slg_scale`, `slg_interval`, `slg_mode` (optional, extension): skip-layer guidance.  On the steps with
    lo <= sigma_i <= hi of `slg_interval` (None = every step) the conditional forward forks at the first of the visual blocks `slg_blocks`
    into a branch that skips them (`slg_mode` "block": the whole block; "attention": only its self-attention) and the step's velocity is
    v_cfg + slg_scale * (c - c_skip), v_cfg being what the step would otherwise use (CFG, the guidance plan's coefficients — computed over
    c and u, the skip term is added after them — or c alone at guidance 1).  No blocks, scale 0 or an interval without a step is off and
    nothing changes.  A `strength < 1` run cuts the mask with the schedule.  ValueError, before anything runs: bad indices, scale or mode;
    together with MagCache, context windows or a CFG pair; at a wrapped model without `forward_skip`.  The values commonly quoted for other
    models (blocks 9, 10 at scale 3 on 0.2 <= sigma <= 0.99) are examples: no Kandinsky checkpoint was at hand, visual quality is not claimed.
    `eta`, `s_noise`, `sde_interval`, `sde_seed` (optional, extension): stochastic sampling ("euler ancestral" for rectified flow).  On the
    steps with lo <= sigma_i <= hi of `sde_interval` (None = every step) the Euler step goes only to sigma_down = t (1 + (t / s - 1) eta) and
    the latent is re-noised to t = sigma_{i+1}: x = a x + c z with a = (1 - t) / (1 - sigma_down), c = s_noise sqrt(t^2 - (sigma_down a)^2)
    (`stochastic_plan`); the last step, which ends at 0, never is.  z comes from a counter-based generator inside the update kernel: element
    g of step i is a pure function of (`sde_seed`, i, g) (`sde_seed` None = `seed`), so a run repeats exactly, a captured step replays and
    the ranks of a group or a CFG pair draw the same bits without an exchange.  eta 0 (default), or an interval that holds no step, is off
    and nothing changes.  A `strength < 1` run cuts the plan with the schedule; with batch > 1 the samples run one at a time, sample b with
    seed sde_seed + b.  The engine-backed model runs it inside its loop (`DiffusionTransformer3D.set_stochastic`, set for this call and
    removed afterwards), any other model through the same kernel from the per-step loop: the same bits.  ValueError, before anything runs:
    eta outside [0, 1], a negative or non-finite s_noise, a bad interval; together with context windows, MagCache or preview_every > 0
    (the preview's x0 = x - sigma v does not hold after the noise; a callback without previews works).  No checkpoint was at hand, visual
    quality is not claimed.
    `enhance_weight`, `enhance_interval` (optional, extension): Enhance-A-Video (Luo et al. 2025).  On the steps with lo <= sigma_i <= hi of
    `enhance_interval` (None = every step) every visual block of every forward multiplies its self-attention output by
    max(1, mean * (frames + enhance_weight)), mean being the mean attention mass the frames of one spatial position send to each other's
    frames rather than to themselves (`DiffusionTransformer3D.set_enhance`).  `enhance_weight` None (default) is off and nothing changes; 0.0
    is a valid weight.  A `strength < 1` run cuts the mask with the schedule; with context windows the frames are the window's; one frame is
    inert.  The engine-backed model runs it inside its loop (set for this call and removed afterwards), a model that hands `set_enhance` on
    step by step from the per-step loop: the same bits.  ValueError, before anything runs: a bad weight or interval; a rank of a
    sequence-parallel group; more than 64 latent frames per forward; a model without `set_enhance`.  No checkpoint was at hand, visual
    quality is not claimed.
    `forecast_interval`, `forecast_order`, `forecast_warmup`, `forecast_tail` (optional, extension): the forecast cache (TaylorSeer "lite",
    Liu et al. 2025).  After `forecast_warmup` full steps only every `forecast_interval`-th step (and the last `forecast_tail`) runs the visual
    blocks; the others add the blocks' residual extrapolated from the finite differences of the full steps, up to `forecast_order` (0, 1, 2),
    per CFG branch (`forecast_plan`, `DiffusionTransformer3D.set_forecast`).  The plan depends on the step index alone: no ratio table, and
    it works with `strength` < 1 (the plan covers the steps that run), `eta`, NAG, regions and sequence-parallel groups.  None or 1 (default)
    is off and nothing changes.  ValueError, before anything runs: MagCache on the model, `slg_blocks`, a guidance plan with steps of
    different kinds or `cfg_zero_init`, more than one context window, a CFG pair, a model without `set_forecast` / `forecast_at`.  No
    checkpoint was at hand, visual quality is not claimed.
    `source_text_embeds`, `source_text_rope_pos`, `source_guidance_weight`, `flowedit_refine`, `flowedit_seed` (optional, extension): FlowEdit
    (Kulikov et al. 2024), prompt-driven editing of `init_latent`: "the same clip, but the cat is a dog".  `source_text_embeds` (a dict like
    `text_embeds`) describes the source clip and selects the mode; without it `init_latent` is the SDEdit path above, exactly as before.
    Steps first = edit_first_step(num_steps, strength) .. num_steps - flowedit_refine - 1 integrate the difference between the target and the
    source prompt's guided velocities along a noisy path tied to the source, with fresh noise at every step from the update kernel's
    counter-based generator (`flowedit_seed` None = `seed`; step i draws stream i, so a cut schedule draws the noise of the full one); the
    last `flowedit_refine` steps are plain steps on the target prompt.  Nothing is inverted, and the result stays on the source wherever the
    two prompts agree.  `source_guidance_weight` None = `guidance_weight`; `null_text_embeds` is the negative prompt of both sides; a side
    of weight 1 runs no unconditional forward.  `keep_mask` cells of 1 hold the source bit for bit.  `noise` is not read.  The
    engine-backed model runs the one call (k5_sample_flowedit), any other callable the same forwards in the same order from the per-step
    loop through `E.flowedit_step_`: the same bits.  With batch > 1 the samples run one at a time, sample b with seed flowedit_seed + b.
    ValueError, before anything runs: without init_latent or source_text_rope_pos; flowedit_refine outside 0 .. the steps that run, or > 0
    with keep_mask; together with context windows, MagCache, a multi-rank model, forecast steps, slg_blocks, a guidance plan, eta > 0, NAG,
    regions or preview_every > 0.  SD3's published values (33 of 50 steps, source guidance 3.5, target 13.5) are examples: no Kandinsky
    checkpoint was at hand, visual quality is not claimed."""
    batch = int(batch)
    if batch < 1 or shape[0] % batch:
        raise ValueError(f"shape[0] = {shape[0]} frames do not divide into batch={batch} samples")
    _check_edit_args(model, shape, init_latent, strength, keep_mask)
    context = (context_frames, context_overlap, context_text, context_height, context_width, context_overlap_hw)
    tiles = _plan_for(model, (shape[0] // batch, shape[1], shape[2]), context, init_latent, preview_every)
    many = any(isinstance(v, (list, tuple)) for v in (text_embeds, null_text_embeds))
    if batch == 1 and many:
        text_embeds, null_text_embeds, text_rope_pos, null_text_rope_pos = (
            split_per_sample(v, 1, n)[0] for v, n in ((text_embeds, "text_embeds"), (null_text_embeds, "null_text_embeds"),
                                                 (text_rope_pos, "text_rope_pos"), (null_text_rope_pos, "null_text_rope_pos")))
    first = edit_first_step(num_steps, strength) if init_latent is not None else 0
    steps_run = num_steps - first
    guide_kw = (guidance_schedule, guidance_interval, cfg_zero_star, cfg_zero_init, cfg_rescale)
    guide = skip = None
    windowed = tiles is not None and tiles.nwin > 1
    wants_guide = any(v is not None for v in guide_kw[:2]) or any(guide_kw[2:])
    wants_skip = slg_blocks is not None or slg_scale or slg_interval is not None
    sto = None
    wants_sto = bool(eta) or sde_interval is not None or float(s_noise) != 1.0
    enhance = None
    wants_enhance = enhance_weight is not None or enhance_interval is not None
    if wants_guide or wants_skip or wants_sto or wants_enhance:   # the schedule as `_generate_one` draws it: the same bits
        sigmas = sigma_schedule(num_steps, scheduler_scale, device=device).cpu().tolist()
    if wants_guide:
        guide = _guidance_for_run(model, sigmas, first, guidance_weight, *guide_kw, init_latent, windowed)
    if wants_skip:
        skip = _skip_for_run(model, sigmas, first, slg_blocks, slg_scale, slg_interval, slg_mode, windowed)
        if skip is not None and not (type(model) is DiffusionTransformer3D or hasattr(model, "forward_skip")):
            raise ValueError("slg_blocks needs a model with forward_skip (the engine-backed DiffusionTransformer3D has it): the skip branch runs "
                             "inside its forward, a wrapped callable without one cannot take it")
    if wants_sto:
        sto = _stochastic_for_run(model, sigmas, first, eta, s_noise, sde_interval, seed if sde_seed is None else sde_seed, windowed, preview_every)
    if wants_enhance:
        enhance = _enhance_for_run(model, sigmas, first, enhance_weight, enhance_interval,
                                   shape[0] // batch if tiles is None else tiles.window[0])
    forecast = _forecast_for_run(model, steps_run, forecast_interval, forecast_order, forecast_warmup, forecast_tail, guide, skip, windowed)
    flow = _flowedit_for_run(model, num_steps, strength, init_latent, keep_mask, guidance_weight, seed, source_text_embeds, source_text_rope_pos,
                             source_guidance_weight, flowedit_refine, flowedit_seed,
                             (("forecast_interval", forecast is not None), ("slg_blocks", skip is not None),
                              ("guidance_schedule / guidance_interval / cfg_zero_star / cfg_zero_init / cfg_rescale", guide is not None),
                              ("eta > 0", sto is not None), ("nag_scale", nag_scale is not None),
                              ("region_text_embeds", region_text_embeds is not None), ("preview_every > 0", int(preview_every or 0) > 0)))
    if region_text_embeds is not None and windowed:
        raise ValueError("region_text_embeds together with context windows is not supported: the masks cover the clip, a window sees a slice")
    with _skip_for_call(model, skip), _forecast_for_call(model, forecast), _enhance_for_call(model, enhance), _nag_for_call(model, nag_text_embeds, nag_text_rope_pos, nag_scale, nag_tau, nag_alpha), \
            _regions_for_call(model, region_text_embeds, region_text_rope_pos, region_masks, region_base_weight):
        # one hook for the whole call (it owns the bar): the samples of a batch share it
        watch = _StepWatch(model, callback, preview_every, preview_factors, preview_x0, progress, batch * steps_run, shape[-1])
        try:
            if noise is None:
                g = torch.Generator(device="cuda")
                g.manual_seed(seed)
                img = torch.randn(*shape, device=device, generator=g)
            else:
                img = noise.to(device=device, dtype=torch.float32).clone()
            run = (model, device, img.contiguous(), num_steps, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos,
                   null_text_rope_pos, guidance_weight, scheduler_scale, conf, watch)
            what = (context, visual_cond, visual_cond_mask, init_latent, strength, keep_mask)
            if batch > 1:
                return _generate_batch(*run, batch, *what, guide=guide, skip=skip, sto=sto, enhance=enhance, forecast=forecast, flow=flow)
            return _generate_one(*run, *what, guide=guide, skip=skip, sto=sto, enhance=enhance, forecast=forecast, flow=flow, tiles=tiles)
        finally:
            watch.close()


def _generate_one(model, device, img, num_steps, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos,
                  guidance_weight, scheduler_scale, conf, watch, context, visual_cond, visual_cond_mask, init_latent, strength,
                  keep_mask, guide=None, skip=None, sto=None, enhance=None, forecast=None, flow=None, tiles=None):
    """`generate` for one sample on its drawn noise `img` (contiguous fp32 on the device), with the hook `watch`, the checked window plan
    `tiles` of `_plan_for`, the checked guidance plan `guide` of `_guidance_for_run`, the checked skip set `skip` of `_skip_for_run` (installed on
    the model by `generate`), the checked stochastic plan `sto` of `_stochastic_for_run` and the checked Enhance-A-Video set `enhance` of
    `_enhance_for_run` (`generate` puts back what the model held) and the checked forecast plan `forecast` of `_forecast_for_run` (installed
    on the model by `generate`) and the checked FlowEdit side `flow` of `_flowedit_for_run`; returns the latent."""
    context_text = context[2]
    if tiles is not None:
        if context_text is not None:   # the first window's prompt stands where the one prompt of a plain run does
            text_embeds, text_rope_pos = context_text[0]
        if tiles.nwin == 1:
            tiles = None
        else:   # the window's positions are the first entries of the clip's, in every axis
            visual_rope_pos = [torch.as_tensor(p)[:n] for p, n in zip(visual_rope_pos, (tiles.window[0], tiles.window[1] // 2, tiles.window[2] // 2))]
    edit = None
    if init_latent is not None:   # img (the draw) is eps from here on; the latent is a buffer of its own that the engine fills
        src = init_latent.to(device=img.device, dtype=torch.float32).contiguous()
        km = None if keep_mask is None else keep_mask.to(device=img.device, dtype=torch.float32).contiguous()
        edit = (src, img, km) if flow is None else None
        img = torch.empty_like(img) if flow is None else src.clone()   # FlowEdit: the latent is z_fe, which starts as the source
    fe_km = km if flow is not None else None
    cond_in = _conditioning(model, img, visual_cond, visual_cond_mask)

    one_window = img if tiles is None else img[:tiles.window[0], :tiles.window[1], :tiles.window[2]]
    sparse_params = get_sparse_params(conf, {"visual": one_window}, device)
    timesteps = sigma_schedule(num_steps, scheduler_scale, device=device).cpu()  # one sync, before the loop
    first = edit_first_step(num_steps, strength) if init_latent is not None else 0
    timesteps = timesteps[first:]   # strength is a truncation of the schedule, nothing more

    if isinstance(model, torch.nn.Module):      # per-step paths below: a new sampling run starts with no softmax-form memory (k5_sample resets its own)
        for m in model.modules():
            if isinstance(m, DiffusionTransformer3D):
                m.reset_softmax_memory()
    cfg_on = _is_guided(guidance_weight)
    g_weights, g_zero_star, g_zero_init, g_rescale = guide if guide is not None else (None, False, 0, 0.0)
    if g_weights is not None:   # some step is guided: the pair exchanges, the buffers of the unconditional side exist
        cfg_on = any(_is_guided(w) for w in g_weights)
    cfg_parallel = getattr(model, "_cfg_parallel", None)
    # CFG-parallel for a model WITHOUT the engine-side pair (a wrapped / duck-typed model): this rank's group
    # runs ONE of the two forwards; the pair exchanges the velocities (6 MB at 5 s) over torch.distributed and every rank applies
    # the identical bf16 combine + Euler update.  A DiffusionTransformer3D set up by parallelize_dit does the same INSIDE
    # k5_sample (k5_dit_cfg_pair_init) and takes the fused path below.
    exchange = cfg_parallel is not None and cfg_on and getattr(model, "_cfg_pair", None) is None
    if not exchange and type(model) is DiffusionTransformer3D and model.visual_cond in (True, False):
        # whole loop inside the engine: no per-step host work at all
        with model.setting_for_call("watch", watch.watch_args()), model.setting_for_call("guidance", guide), \
                model.setting_for_call("stochastic", sto), model.setting_for_call("enhance", enhance):
            model.sample(img, timesteps.tolist(), text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos,
                         null_text_rope_pos, guidance_weight, scale_factor=conf.metrics.scale_factor,
                         sparse_params=sparse_params,
                         visual_cond=None if cond_in is None else torch.cat(cond_in, dim=-1).contiguous(), edit=edit,
                         flowedit=None if flow is None else (src, flow[0], flow[1], flow[2], fe_km, flow[3], flow[4], first),
                         tiles=tiles, window_text=None if tiles is None else context_text)
        return img

    # The per-step loop.  Each step takes (v_cond, v_uncond, v_skip) from one of three sources (a windowed run: its per-window buffers), makes
    # the one update call and calls the hook.
    def forward(x, te, tp, t1000, slot=0):
        if forecast is not None:   # this forward is call (step, slot) of the plan, as the engine's loop makes it
            model.forecast_at(step_now, slot)
        return model(x, te["text_embeds"], te["pooled_embed"], t1000, visual_rope_pos, tp, scale_factor=conf.metrics.scale_factor,
                     sparse_params=sparse_params)

    def plain_velocities(t1000, guided):   # cond, then uncond
        x = _model_input(model, img, cond_in)
        v = forward(x, text_embeds, text_rope_pos, t1000)
        u = forward(x, null_text_embeds, null_text_rope_pos, t1000, 1) if guided else None
        return v.contiguous(), None if u is None else u.contiguous(), None

    def skip_velocities(t1000, guided):   # cond + skip in one forking forward, then uncond: the engine's order
        x = _model_input(model, img, cond_in)
        v, sv = model.forward_skip(x, text_embeds["text_embeds"], text_embeds["pooled_embed"], t1000, visual_rope_pos, text_rope_pos,
                                   scale_factor=conf.metrics.scale_factor, sparse_params=sparse_params)
        u = forward(x, null_text_embeds, null_text_rope_pos, t1000) if guided else None
        return v.contiguous(), None if u is None else u.contiguous(), sv.contiguous()

    def pair_velocities(t1000, guided):   # my branch, then the pair's exchange into the reused buffer
        nonlocal both
        v = forward(_model_input(model, img, cond_in), *mine, t1000)
        if both is None:
            both = torch.empty((2,) + tuple(v.shape), dtype=v.dtype, device=v.device)
        return (*exchange_velocity(v, cfg_parallel[1], out=both), None)

    def tile_velocities(t1000, guided):
        # the forwards of k5_sample_tiles / k5_sample_windows in their order: window by window, cond then uncond, each on a contiguous copy of its box of the latent
        for k in range(tiles.nwin):
            x = _model_input(model, img, cond_in, tiles.box(k)).contiguous()
            vbuf[k] = forward(x, *((text_embeds, text_rope_pos) if context_text is None else context_text[k]), t1000)
            if cfg_on:
                ubuf[k] = forward(x, null_text_embeds, null_text_rope_pos, t1000)
        return vbuf, ubuf

    if exchange:
        from .models.parallelize import exchange_velocity
        mine = (text_embeds, text_rope_pos) if cfg_parallel[0] == 0 else (null_text_embeds, null_text_rope_pos)
        both = None
    elif tiles is not None:
        tile_dev = E.tile_tables(tiles, img.device)
        vbuf = torch.empty((tiles.nwin,) + tiles.window + (img.shape[-1],), dtype=torch.bfloat16, device=img.device)
        ubuf = torch.empty_like(vbuf) if cfg_on else None

    n = len(timesteps) - 1
    step_now = 0
    if forecast is not None and hasattr(model, "set_forecast"):
        model.set_forecast(*forecast)   # every run starts without history, as every k5_sample* call does
    km = None if edit is None else edit[2]
    keep = {} if km is None else dict(source=edit[0], noise=edit[1], keep_mask=km)
    if edit is not None:
        E.renoise(edit[0], edit[1], float(timesteps[0]), out=img)
    fe_steps = 0
    if flow is not None:
        # FlowEdit as the engine's loop runs it: img is z_fe; one pass finishes step i and forms zs / zt, the forwards' inputs of step i + 1
        # (of the first plain step: its latent), with that step's sigma and noise stream
        src_te, src_pos, w_src, refine, fe_seed = flow
        src_guided, fe_steps = _is_guided(w_src), n - refine
        zs, zt = torch.empty_like(img), torch.empty_like(img)

        def prepare(nx):
            return dict(sigma_next=float(timesteps[nx]), zs=zs, zt=zt, seed=fe_seed, stream_id=first + nx) if nx < n else {}

        E.flowedit_step_(img, src, **prepare(0))
        if fe_steps == 0:
            img.copy_(zt)
    for i, (timestep, timestep_diff, sigma_next) in enumerate(zip(timesteps[:-1].tolist(), torch.diff(timesteps).tolist(),
                                                                  timesteps[1:].tolist())):
        # the step's weight, kind and fork, as the engine's loop (SampleRun in engine.hip) decides them: zero (no forward, no update), unguided
        # (the conditional forward alone), guided; without a plan every step is of the call's one kind.  A skip step forks the conditional forward
        w_at = guidance_weight if g_weights is None else g_weights[i]
        kind = "zero" if i < g_zero_init else "guided" if (cfg_on if guide is None else _is_guided(w_at)) else "unguided"
        skip_at = kind != "zero" and skip is not None and bool(skip[3][i])
        step_now = i
        wants_preview = watch.active and watch.preview_at(i, n)
        _enhance_at(model, enhance, i)
        t1000 = torch.tensor([timestep]) * 1000
        if kind == "zero":
            v, u = (torch.zeros(img.shape, dtype=torch.bfloat16, device=img.device) if wants_preview else None), None   # velocity 0: x0 = x
        elif i < fe_steps:             # source cond, source uncond on zs; target cond, target uncond on zt; then the pass
            xs, xt = _model_input(model, zs, cond_in), _model_input(model, zt, cond_in)
            cs = forward(xs, src_te, src_pos, t1000).contiguous()
            us = forward(xs, null_text_embeds, null_text_rope_pos, t1000, 1).contiguous() if src_guided else None
            v = forward(xt, text_embeds, text_rope_pos, t1000).contiguous()
            u = forward(xt, null_text_embeds, null_text_rope_pos, t1000, 1).contiguous() if cfg_on else None
            E.flowedit_step_(img, src, cs, us, v, u, w_src=w_src if src_guided else 1.0, w_tar=guidance_weight if cfg_on else 1.0,
                             dt=timestep_diff, keep_mask=fe_km, **prepare(i + 1))
            if i + 1 == fe_steps and fe_steps < n:
                img.copy_(zt)          # the plain steps that close the run start from zt
        elif tiles is not None:        # every window's pair, then the one blend + Euler pass over the clip: a kernel of its own
            v, u = tile_velocities(t1000, kind == "guided")
            E.cfg_euler_tiles_(img, v, u, guidance_weight, timestep_diff, tile_dev)
        else:
            v, u, sv = (skip_velocities if skip_at else pair_velocities if exchange else plain_velocities)(t1000, kind == "guided")
            # the plan's coefficients are reduced on the device and read there; the skip term comes after them
            ab = E.guidance_coeffs(v, u, w_at, g_zero_star, g_rescale)[0] if kind == "guided" and (g_zero_star or g_rescale > 0.0) else None
            v_out = v if wants_preview and (ab is not None or skip_at) else None
            # a stochastic run takes its dt_down as dt and says so at every step, also where noise_coef is 0: the engine's one launch
            E.euler_step_(img, v, u, w=w_at, dt=timestep_diff if sto is None else sto[0][i], ab=ab, v_skip=sv, g=skip[1] if skip_at else 0.0,
                          sigma_next=sigma_next, v_out=v_out, stochastic=None if sto is None else (sto[1][i], sto[2][i], sto[3], sto[4] + i),
                          **keep)
            if v_out is not None:
                u = None               # v now holds the step's velocity, where the preview reads it
        if not watch.active:
            continue
        # the per-step paths' side of the watch: the preview of the step just applied (the engine's kernel, the engine's rule for which steps
        # carry one; never on a windowed run, whose preview_every is refused) and the callback
        preview = x0 = None
        if wants_preview:
            rgb, x0 = E.x0_preview(img, v, u, w_at, sigma_next, watch.W, watch.b, source=None if km is None else edit[0],
                                   keep_mask=km, want_x0=watch.want_x0)
            preview = rgb.cpu()
        if watch.step(StepInfo(i, n, watch.sample, watch.num_samples, sigma_next, preview, x0)):
            raise SamplingInterrupted(i + 1, img, watch.sample)
    return img


def _generate_batch(model, device, img, num_steps, text_embeds, null_text_embeds, visual_rope_pos, text_rope_pos, null_text_rope_pos,
                    guidance_weight, scheduler_scale, conf, watch, batch, context, visual_cond, visual_cond_mask, init_latent, strength,
                    keep_mask, guide=None, skip=None, sto=None, enhance=None, forecast=None, flow=None):
    """`generate` for batch > 1 on the drawn noise `img` (batch*T, H, W, C), updated in place sample by sample"""
    T = img.shape[0] // batch
    tes, nes = split_per_sample(text_embeds, batch, "text_embeds"), split_per_sample(null_text_embeds, batch, "null_text_embeds")
    tps = split_per_sample(text_rope_pos, batch, "text_rope_pos")
    nps = split_per_sample(null_text_rope_pos, batch, "null_text_rope_pos")
    for v, n in ((visual_cond, "visual_cond"), (visual_cond_mask, "visual_cond_mask")):
        if v is not None and v.shape[0] != img.shape[0]:
            raise ValueError(f"{n} must have {img.shape[0]} frames (batch={batch} x {T}), got {v.shape[0]}")

    if sto is None and init_latent is None and all(v is None for v in (context[0], context[3], context[4])) and type(model) is DiffusionTransformer3D and model.visual_cond in (True, False) \
            and model.many_ready() and getattr(model, "_cfg_parallel", None) is None:
        cond = _conditioning(model, img, visual_cond, visual_cond_mask)
        if cond is not None:
            cond = torch.cat(cond, dim=-1).reshape(batch, T, *img.shape[1:-1], img.shape[-1] + 1).contiguous()
        sparse_params = get_sparse_params(conf, {"visual": img[:T]}, device)
        timesteps = sigma_schedule(num_steps, scheduler_scale, device=device).cpu()
        with model.setting_for_call("watch", watch.watch_args()), model.setting_for_call("guidance", guide), \
                model.setting_for_call("enhance", enhance):
            model.sample_many(img.view(batch, T, *img.shape[1:]), timesteps.tolist(), tes, nes, visual_rope_pos, tps, nps,
                               guidance_weight, scale_factor=conf.metrics.scale_factor, sparse_params=sparse_params, visual_cond=cond)
        return img
    # any other model (rank groups, MagCache, graph replay, wrapped or duck-typed models), editing and context windows: one sample at a time,
    # each checked and planned as the call of its own that it equals
    watch.num_samples = batch
    for b in range(batch):
        rows = slice(b * T, (b + 1) * T)
        vc, vm, src, km = (None if v is None else v[rows] for v in (visual_cond, visual_cond_mask, init_latent, keep_mask))
        _check_edit_args(model, img[rows].shape, src, strength, km)
        tiles = _plan_for(model, (T, img.shape[1], img.shape[2]), context, src, watch.every)
        watch.sample = b
        img[rows] = _generate_one(model, device, img[rows].clone(), num_steps, tes[b], nes[b], visual_rope_pos, tps[b], nps[b], guidance_weight,
                                  scheduler_scale, conf, watch, context, vc, vm, src, strength, km, guide=guide, skip=skip, enhance=enhance,
                                  tiles=tiles, forecast=forecast, flow=None if flow is None else (*flow[:4], (flow[4] + b) & (2 ** 64 - 1)),
                                  sto=None if sto is None else (*sto[:3], (sto[3] + b) & (2 ** 64 - 1), sto[4]))   # a seed per sample
    return img


def _encode_prompts(text_embedder, prompts, kind, device):
    """[(embeds dict on `device`, number of text tokens)] for each prompt (reference generation_utils.py:153-176)."""
    out = []
    with torch.no_grad():
        for prompt in prompts:
            embeds, cu = text_embedder.encode([prompt], type_of_content=kind)
            out.append(({name: t.to(device=device) for name, t in embeds.items()}, int(cu[-1])))
    return out


def latent_to_uint8(latent, vae, batch, vae_device):
    """Latent (batch*T, H, W, C) -> uint8 frames (batch, 3, F, 8H, 8W): un-scale, channels first, VAE decode, clamp to [-1, 1],
    map to 0..255 (reference generation_utils.py:209-222)."""
    T = latent.shape[0] // batch
    z = latent.reshape(batch, T, *latent.shape[1:]).to(device=vae_device)
    z = (z / vae.config.scaling_factor).permute(0, 4, 1, 2, 3)
    frames = vae.decode(z).sample
    return frames_to_uint8(frames)


def frames_to_uint8(frames):
    """((frames.clamp(-1, 1) + 1) * 127.5).to(torch.uint8) (reference generation_utils.py:222-224).  bf16 frames on the GPU: one pass of the engine's
    kernel with torch's rounding after every elementwise op (k5_frames_to_uint8) instead of four over the whole video; anything else: torch."""
    if frames.is_cuda and frames.dtype == torch.bfloat16 and frames.numel() % 8 == 0:
        from . import _engine as E
        x = frames if frames.is_contiguous() else frames.contiguous()
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            E.check(E.lib().k5_frames_to_uint8(x.data_ptr(), out.data_ptr(), x.numel(), E.stream_ptr(x.device)), "k5_frames_to_uint8")
        return out
    return ((frames.clamp(-1.0, 1.0) + 1.0) * 127.5).to(torch.uint8)


def generate_sample(shape, caption, dit, vae, conf, text_embedder, num_steps=25, guidance_weight=5.0,
                    scheduler_scale=1, negative_caption="", seed=6554, device="cuda", vae_device="cuda",
                    text_embedder_device="cuda", progress=True, offload=False, image=None, video=None, strength=1.0, mask=None,
                    callback=None, preview_every=0, preview_factors=None, context_frames=None, context_overlap=None,
                    nag_scale=None, nag_tau=2.5, nag_alpha=0.25, region_text_embeds=None, region_text_rope_pos=None, region_masks=None,
                    region_base_weight=0.0, guidance_schedule=None, guidance_interval=None, cfg_zero_star=False, cfg_zero_init=0,
                    cfg_rescale=0.0, slg_blocks=None, slg_scale=0.0, slg_interval=None, slg_mode="block", eta=0.0, s_noise=1.0,
                    sde_interval=None, sde_seed=None, enhance_weight=None, enhance_interval=None, forecast_interval=None, forecast_order=1,
                    forecast_warmup=None, forecast_tail=1, source_caption=None, source_guidance_weight=None, flowedit_refine=0,
                    flowedit_seed=None, context_height=None, context_width=None, context_overlap_hw=None):
    """reference generation_utils.py:132-228 (same signature): text encode -> generate -> VAE decode -> uint8.
    With `offload` each of the three models visits the GPU only for its own stage.  `image` (optional, extension: PIL image or
    tensor, see conditioning.preprocess_image): image-to-video, the picture's VAE latent conditions latent frame 0 of every
    sample.  `caption` (extension): one prompt for every sample, or a list of `bs` prompts, one per sample; the samples come from
    one noise draw of the whole shape (see `generate`).  `video`, `strength`, `mask` (optional, extension): video-to-video and masked
    editing.  `video` is the source clip (uint8 (F,H,W,3) or float (F,3,H,W) frames, see conditioning.preprocess_video), `strength`
    in (0, 1] how much of the schedule runs on it and `mask` a pixel keep mask ((H,W) or (F,H,W), >= 0.5 = keep the source there, at
    8 * height x 8 * width, see conditioning.pixel_mask_to_latent); every sample of the batch edits the same clip.
    `progress` draws a tqdm bar over the sampling steps when tqdm is installed; `callback`, `preview_every`, `preview_factors`
    (optional, extension): per-step callback, cancel and live previews, see `generate`.  `context_frames`, `context_overlap` (optional,
    extension): a clip longer than the model's trained length, sampled as overlapping temporal windows of `context_frames` latent frames
    (see `generate` and `context_windows`).  With bs = 1 `caption` may then be a list of nwin prompts, one per window in order.
    `nag_scale`, `nag_tau`, `nag_alpha` (optional, extension): normalized attention guidance with the already encoded `negative_caption` as
    the negative prompt (see `generate`); what makes `negative_caption` count at guidance_weight 1.  None (default) is off.
    `region_text_embeds`, `region_text_rope_pos`, `region_masks`, `region_base_weight` (optional, extension): regional prompts (see
    `generate`): `caption` is the base prompt, `region_masks` (R, frames, height, width) lies on the latent cells of one sample
    (`conditioning.region_masks_to_latent`).  `region_text_embeds` is a list of already encoded dicts with their `region_text_rope_pos`, or
    a list of R prompt strings: those are encoded by the same embedder call as the caption (only their token embeddings are used) and take
    positions 0 .. n-1.  One region set for every sample of a batch.
    `guidance_schedule`, `guidance_interval`, `cfg_zero_star`, `cfg_zero_init`, `cfg_rescale` (optional, extension): per-step guidance
    weights, a guidance interval, CFG-Zero* and CFG rescale, passed to `generate` (see there).  All off by default.
    `slg_blocks`, `slg_scale`, `slg_interval`, `slg_mode` (optional, extension): skip-layer guidance, passed to `generate` (see there).  Off by
    default.
    `eta`, `s_noise`, `sde_interval`, `sde_seed` (optional, extension): stochastic sampling, passed to `generate` (see there).  Off by default.
    `enhance_weight`, `enhance_interval` (optional, extension): Enhance-A-Video, passed to `generate` (see there).  None (default) is off.
    `forecast_interval`, `forecast_order`, `forecast_warmup`, `forecast_tail` (optional, extension): the forecast cache, passed to `generate`
    (see there).  None or 1 (default) is off.
    `source_caption`, `source_guidance_weight`, `flowedit_refine`, `flowedit_seed` (optional, extension): FlowEdit (see `generate`): with
    `video`, `source_caption` describes the source clip, `caption` the result; `strength` and `mask` keep their meaning.  None (default)
    is off: `video` alone is the SDEdit path.
    `context_height`, `context_width`, `context_overlap_hw` (optional, extension): a frame larger than the model's trained size, sampled as
    overlapping spatial windows of that many latent cells (see `generate` and `tile_windows`); `image` conditions the whole frame and each
    window sees its slice.  With bs = 1 `caption` may then be a list of nwin prompts, one per window of the 3-D plan."""
    batch, frames, height, width, channels = shape
    flow_kw = {}
    if source_caption is None:
        if source_guidance_weight is not None or flowedit_refine or flowedit_seed is not None:
            raise ValueError("source_guidance_weight / flowedit_refine / flowedit_seed need source_caption (the prompt that describes the clip)")
    else:   # before any model runs: the numbers (what depends on the run is checked by `generate`)
        if video is None:
            raise ValueError("source_caption (FlowEdit) needs a source video")
        if not isinstance(source_caption, str):
            raise ValueError("source_caption must be one prompt: every sample of the batch edits the same clip")
        if flowedit_plan(num_steps, strength, flowedit_refine).count("plain") and mask is not None:
            raise ValueError("flowedit_refine > 0 together with mask is not supported (see `generate`)")
        flow_kw = dict(source_guidance_weight=source_guidance_weight, flowedit_refine=flowedit_refine, flowedit_seed=flowedit_seed)
    forecast_kw = {}
    if forecast_interval is not None:   # before any model runs: the numbers (what depends on the run is checked by `generate`)
        forecast_plan(num_steps, forecast_interval, forecast_warmup, forecast_tail, forecast_order)
        forecast_kw = dict(forecast_interval=forecast_interval, forecast_order=forecast_order, forecast_warmup=forecast_warmup,
                           forecast_tail=forecast_tail)
    enhance_kw = {}
    if enhance_weight is not None or enhance_interval is not None:   # before any model runs: the numbers and what the handle's state refuses
        fwd_frames = frames if context_frames is None else min(int(frames), int(context_frames))
        _enhance_for_run(dit, [1.0, 0.0], 0, enhance_weight, None, fwd_frames)
        enhance_plan([1.0, 0.0], enhance_interval)   # (what depends on the schedule is checked by `generate`)
        if enhance_weight is None:
            raise ValueError("enhance_interval needs enhance_weight")
        enhance_kw = dict(enhance_weight=enhance_weight, enhance_interval=enhance_interval)
    sto_kw = {}
    wants_sto = eta or sde_interval is not None or float(s_noise) != 1.0
    wants_skip = slg_blocks is not None or slg_scale or slg_interval is not None
    # before any model runs: the window plan and what it is refused with; more than one context window is what both pre-checks below refuse
    context = (context_frames, context_overlap, None, context_height, context_width, context_overlap_hw)
    tiles = _plan_for(dit, (frames, height, width), context, video, preview_every)
    windowed = tiles is not None
    if wants_sto:   # before any model runs: the numbers and what the handle's state refuses
        _stochastic_for_run(dit, [1.0, 0.5, 0.0], 0, eta, s_noise, None, seed if sde_seed is None else sde_seed, windowed, preview_every)
        stochastic_plan([1.0, 0.0], eta, s_noise, sde_interval)   # (what depends on the schedule is checked by `generate`)
        sto_kw = dict(eta=eta, s_noise=s_noise, sde_interval=sde_interval, sde_seed=sde_seed)
    skip_kw = {}
    if wants_skip:   # before any model runs: the numbers and what the handle's state refuses
        skip_plan([1.0, 0.0], slg_interval)   # (what depends on the schedule is checked by `generate`)
        _skip_for_run(dit, [1.0, 0.0], 0, slg_blocks, slg_scale, None, slg_mode, windowed)
        skip_kw = dict(slg_blocks=slg_blocks, slg_scale=slg_scale, slg_interval=slg_interval, slg_mode=slg_mode)
    guide_kw = {k: v for k, v in dict(guidance_schedule=guidance_schedule, guidance_interval=guidance_interval, cfg_zero_star=cfg_zero_star,
                                      cfg_zero_init=cfg_zero_init, cfg_rescale=cfg_rescale).items() if v}
    if guide_kw:   # before any model runs: the numbers (what depends on the schedule is checked by `generate`)
        check_guidance_args(None if guidance_schedule is None or callable(guidance_schedule) else guidance_schedule, cfg_zero_star,
                            cfg_zero_init, cfg_rescale)
        if guidance_interval is not None:
            guidance_plan([1.0, 0.0], guidance_weight, None, guidance_interval)
    ctx_kw, window_captions = {}, None
    if any(v is not None for v in context):
        nwin = 1 if tiles is None else tiles.nwin
        ctx_kw = {k: v for k, v in zip(("context_frames", "context_overlap", "", "context_height", "context_width", "context_overlap_hw"), context)
                  if k and v is not None}
        if batch == 1 and isinstance(caption, (list, tuple)):
            if len(caption) != nwin:
                raise ValueError(f"{len(caption)} prompts for a plan of nwin = {nwin} windows ({tiles!r}): pass one prompt, or one per window")
            window_captions, caption = list(caption), caption[0]
    region_kw, region_prompts = {}, []
    if region_text_embeds is not None:   # before any model runs
        if isinstance(region_text_embeds, (list, tuple)) and region_text_embeds and all(isinstance(p, str) for p in region_text_embeds):
            if region_text_rope_pos is not None:
                raise ValueError("regions: prompts given as strings take positions 0 .. n-1, region_text_rope_pos must be None")
            region_prompts = list(region_text_embeds)   # checked now with stand-ins of one token, encoded with the caption below
            check_region_args([{"text_embeds": torch.zeros(1, 1)}] * len(region_prompts), [[0]] * len(region_prompts), region_masks,
                              region_base_weight)
        else:
            check_region_args(region_text_embeds, region_text_rope_pos, region_masks, region_base_weight)
        if context_frames is not None or ctx_kw:
            raise ValueError("regions together with context_frames is not supported: the masks cover the clip, a window sees a slice")
        if tuple(region_masks.shape[1:]) != (frames, height, width):
            raise ValueError(f"regions: the masks are {tuple(region_masks.shape[1:])}, one sample's latent is {(frames, height, width)}")
        if type(dit) is not DiffusionTransformer3D:
            raise ValueError("region_text_embeds needs the engine-backed DiffusionTransformer3D (see `generate`)")
        region_kw = dict(region_text_embeds=region_text_embeds, region_text_rope_pos=region_text_rope_pos, region_masks=region_masks,
                         region_base_weight=region_base_weight)
    if nag_scale is not None:   # before any model runs
        check_nag_numbers(nag_scale, nag_tau, nag_alpha)
        if type(dit) is not DiffusionTransformer3D:
            raise ValueError("nag_scale needs the engine-backed DiffusionTransformer3D (see `generate`)")
    captions = list(caption) if isinstance(caption, (list, tuple)) else [caption] * batch
    if len(captions) != batch:
        raise ValueError(f"{len(captions)} captions for bs={batch} samples")
    edit_first_step(num_steps, strength)
    if video is None and (float(strength) < 1.0 or mask is not None):
        raise ValueError("strength < 1 and mask need a source video")
    cond_kw = {}
    if video is not None:
        from .conditioning import encode_video, pixel_mask_to_latent
        if offload:
            vae.to(vae_device)
        z = encode_video(video, vae, frames, 8 * height, 8 * width, vae_device=vae_device).to(device)
        if offload:
            vae.to("cpu")
            torch.cuda.empty_cache()
        cond_kw.update(init_latent=z.repeat(batch, 1, 1, 1), strength=strength)
        if mask is not None:
            cond_kw["keep_mask"] = pixel_mask_to_latent(mask, frames, 8 * height, 8 * width).to(device).repeat(batch, 1, 1, 1)
    if image is not None:
        from .conditioning import image_to_visual_cond
        if offload:
            vae.to(vae_device)
        vc, vm = image_to_visual_cond(image, vae, frames, 8 * height, 8 * width, device=device, vae_device=vae_device)
        if offload:
            vae.to("cpu")
            torch.cuda.empty_cache()
        cond_kw.update(visual_cond=vc.repeat(batch, 1, 1, 1), visual_cond_mask=vm.repeat(batch, 1, 1, 1))
    kind = "image" if frames == 1 else "video"
    if window_captions is not None:
        distinct = list(dict.fromkeys(window_captions))
        *encoded, (uncond, n_uncond) = _encode_prompts(text_embedder, distinct + [negative_caption], kind, device)
        by_prompt = dict(zip(distinct, encoded))
        ctx_kw["context_text"] = [(by_prompt[p][0], torch.arange(by_prompt[p][1])) for p in window_captions]
        cond, text_pos = ctx_kw["context_text"][0]
    elif batch == 1:
        (cond, n_cond), (uncond, n_uncond), *region_enc = _encode_prompts(text_embedder, [captions[0], negative_caption] + region_prompts, kind,
                                                                          device)
        text_pos = torch.arange(n_cond)
    else:
        distinct = list(dict.fromkeys(captions))   # a prompt shared by several samples is encoded once
        *encoded, (uncond, n_uncond) = _encode_prompts(text_embedder, distinct + region_prompts + [negative_caption], kind, device)
        encoded, region_enc = encoded[:len(distinct)], encoded[len(distinct):]
        by_prompt = dict(zip(distinct, encoded))
        cond = [by_prompt[p][0] for p in captions]
        text_pos = [torch.arange(by_prompt[p][1]) for p in captions]
    if source_caption is not None:
        (src_cond, n_src), = _encode_prompts(text_embedder, [source_caption], kind, device)
        flow_kw.update(source_text_embeds=src_cond, source_text_rope_pos=torch.arange(n_src))
    if offload:
        text_embedder = text_embedder.to("cpu")

    if region_prompts:
        region_kw.update(region_text_embeds=[{"text_embeds": e["text_embeds"]} for e, _ in region_enc],
                         region_text_rope_pos=[torch.arange(n) for _, n in region_enc])
    nag_kw = {} if nag_scale is None else dict(nag_text_embeds=uncond, nag_text_rope_pos=torch.arange(n_uncond), nag_scale=nag_scale,
                                               nag_tau=nag_tau, nag_alpha=nag_alpha)
    patch = conf.model.dit_params.patch_size
    grid = [torch.arange(frames), torch.arange(height // patch[1]), torch.arange(width // patch[2])]
    if offload:
        dit.to(device, non_blocking=True)
    with torch.no_grad():
        latent = generate(dit, device, (batch * frames, height, width, channels), num_steps, cond, uncond, grid,
                          text_pos, torch.arange(n_uncond), guidance_weight, scheduler_scale, conf, seed=seed,
                          progress=progress, batch=batch, callback=callback, preview_every=preview_every,
                          preview_factors=preview_factors, **cond_kw, **ctx_kw, **nag_kw, **region_kw, **guide_kw, **skip_kw, **sto_kw,
                          **enhance_kw, **forecast_kw, **flow_kw)
    if offload:
        dit.to("cpu", non_blocking=True)
        torch.cuda.empty_cache()
        vae.to(vae_device, non_blocking=True)
    with torch.no_grad():
        images = latent_to_uint8(latent, vae, batch, vae_device)
    if offload:
        vae.to("cpu", non_blocking=True)
        torch.cuda.empty_cache()
    return images
