"""MagCache — host mirror of the reference module (kandinsky/magcache_utils.py).

Same entry point and arguments (`set_magcache_params(dit, mag_ratios, num_steps, no_cfg)`, called by
`get_T2V_pipeline(magcache=True)`, reference utils.py:107-113).  The reference swaps `DiffusionTransformer3D.forward`
for `magcache_forward` class-wide; here the decision state machine and the cached residuals live in the engine
(`k5_dit_set_magcache`, include/k5.h), so both `dit(...)` and the fused `dit.sample(...)` loop honour it.  This module
only prepares the ratio table exactly as the reference does (two leading 1.0, nearest-index interpolation with
numpy's round-half-to-even when the checkpoint's table was calibrated for another step count).

Calibration (no counterpart in the reference, which ships its tables without the code that made them):
`start_magcache_calibration` / `magcache_calibration` / `stop_magcache_calibration` drive the engine's measuring mode
(`k5_dit_set_magcache_calibrate`), `calibrate_magcache(pipe, prompts, ...)` runs the pipeline under it and returns a
table in the schema of the YAML field `magcache.mag_ratios`, and `load_mag_ratios` reads one back from a list or a
JSON / YAML file.
"""
import ctypes as C

import numpy as np

from . import _engine as E


def nearest_interp(src_array, target_length):
    """reference magcache_utils.py:6-13"""
    src_array = np.asarray(src_array)
    src_length = len(src_array)
    if target_length == 1:
        return np.array([src_array[-1]])
    scale = (src_length - 1) / (target_length - 1)
    mapped_indices = np.round(np.arange(target_length) * scale).astype(int)
    return src_array[mapped_indices]


def ratio_table(mag_ratios, num_steps):
    """reference magcache_utils.py:28-39: [1, 1] + ratios, re-sampled per cond / uncond half to 2*num_steps entries."""
    table = np.array([1.0] * 2 + list(mag_ratios), dtype=np.float64)
    if len(table) != num_steps * 2:
        print(f'interpolate MAG RATIOS: curr len {len(table)}')
        con = nearest_interp(table[0::2], num_steps)
        ucon = nearest_interp(table[1::2], num_steps)
        table = np.concatenate([con.reshape(-1, 1), ucon.reshape(-1, 1)], axis=1).reshape(-1)
    return np.ascontiguousarray(table, dtype=np.float64)


def _apply(dit):
    """push the stored parameters into the engine handle (called when the handle is (re)built)"""
    if dit._handle is None:
        return
    cal = getattr(dit, "_magcache_calibrate", None)
    if cal is not None:   # a rebuilt handle starts a new, empty table
        E.check(E.lib().k5_dit_set_magcache_calibrate(dit._handle, int(cal[0]), int(cal[1])), "set_magcache_calibrate")
        return
    if getattr(dit, "mag_ratios", None) is None:
        return
    t = dit.mag_ratios
    E.check(E.lib().k5_dit_set_magcache(dit._handle, t.ctypes.data_as(C.POINTER(C.c_double)), len(t), int(dit.no_cfg),
                                        float(dit.magcache_thresh), int(dit.K), float(dit.retention_ratio)), "set_magcache")
    cfgp = getattr(dit, "_cfg_parallel", None)
    if cfgp is not None and not dit.no_cfg:   # this rank group runs one CFG branch only: calls branch, branch+2, ...
        E.check(E.lib().k5_dit_magcache_calls(dit._handle, int(cfgp[0]), 2), "magcache_calls")


def set_magcache_params(dit, mag_ratios, num_steps, no_cfg):
    """reference magcache_utils.py:16-39 (same attribute names on `dit`)."""
    print('using Magcache')
    dit.num_steps = num_steps * 2
    dit.magcache_thresh = 0.12
    dit.K = 2
    dit.retention_ratio = 0.2
    dit.mag_ratios = ratio_table(mag_ratios, num_steps)
    dit.no_cfg = no_cfg
    try:
        _apply(dit)
    except Exception:   # refused by the engine (a forecast plan is set, the handle is calibrating): the model carries no table
        dit.mag_ratios = None
        raise


def disable_magcache(dit):
    dit.mag_ratios = None
    if dit._handle is not None:
        E.check(E.lib().k5_dit_set_magcache(dit._handle, None, 0, 0, 0.12, 2, 0.2))


def magcache_state(dit):
    """(call counter, forwards that ran the visual blocks, forwards that skipped them) since set_magcache_params"""
    cnt, ran, skipped = C.c_int(), C.c_int64(), C.c_int64()
    E.check(E.lib().k5_dit_magcache_state(dit._handle, C.byref(cnt), C.byref(ran), C.byref(skipped)))
    return cnt.value, ran.value, skipped.value


# ------------------------------------------------------------------------------------------ calibration
def start_magcache_calibration(dit, num_steps, no_cfg):
    """Every forward from here on runs its visual blocks and leaves the norm-ratio statistics of its residual against the
    previous residual of its cond / uncond slot in a device table; runs over the same handle add up.  One GPU, no
    MagCache at the same time (the engine refuses both)."""
    if num_steps < 2:
        raise ValueError(f"calibration needs at least 2 steps (a ratio compares two consecutive steps), got {num_steps}")
    if getattr(dit, "mag_ratios", None) is not None:
        raise RuntimeError("MagCache is set on this model: disable_magcache(dit) first (calibration measures the un-cached residuals)")
    dit._magcache_calibrate = (int(num_steps), bool(no_cfg))
    try:
        _apply(dit)
    except Exception:
        dit._magcache_calibrate = None
        raise


def stop_magcache_calibration(dit):
    """Leave the measuring mode; the engine frees its residual buffers and the table."""
    dit._magcache_calibrate = None
    if dit._handle is not None:
        E.check(E.lib().k5_dit_set_magcache_calibrate(dit._handle, 0, 0), "set_magcache_calibrate")


def calibration_from_sums(sums, num_steps, no_cfg, runs, rows_per_call=None):
    """The calibration dict from the table of sums [2 * num_steps][4] = (sum rho, sum rho^2, sum (1 - cos), rows counted)
    per call.  `mag_ratios` has the schema of the YAML field: length 2 * (num_steps - 1), cond / uncond interleaved from
    step 1 on (`set_magcache_params` prepends the two 1.0), float64 mean = sum rho / count; with `no_cfg` the uncond
    entries repeat the cond ones, as the shipped no-CFG tables do.  `mag_ratio_std` is the unbiased standard deviation
    over the counted rows (torch's `.std()`), `mag_cos_dis` the mean cosine distance."""
    sums = np.asarray(sums, dtype=np.float64).reshape(2 * num_steps, 4)
    t = sums[2:].copy()
    if no_cfg:
        t[1::2] = t[0::2]
    cnt = t[:, 3]
    if not np.all(cnt > 0):
        raise RuntimeError("calibration table has calls without counted rows: run at least one complete sampling run first")
    mean = t[:, 0] / cnt
    var = np.maximum(t[:, 1] - cnt * mean * mean, 0.0) / np.maximum(cnt - 1.0, 1.0)
    out = {"mag_ratios": mean.tolist(), "mag_ratio_std": np.sqrt(var).tolist(), "mag_cos_dis": (t[:, 2] / cnt).tolist(),
           "rows_counted": int(round(cnt.sum())), "rows_total": None, "runs": int(runs), "num_steps": int(num_steps),
           "no_cfg": bool(no_cfg)}
    if rows_per_call is not None:
        out["rows_total"] = int(rows_per_call) * int(runs) * len(cnt)
    return out


def magcache_calibration(dit, rows_per_call=None):
    """What the handle has measured so far (complete runs only make a usable table).  `rows_total` = rows a complete
    table would count if no row had a zero norm: tokens per forward x runs x calls; the tokens per forward are taken
    from the handle's last forward unless `rows_per_call` gives them."""
    cal = getattr(dit, "_magcache_calibrate", None)
    if cal is None or dit._handle is None:
        raise RuntimeError("calibration is not running on this model: start_magcache_calibration(dit, num_steps, no_cfg) first")
    num_steps, no_cfg = cal
    buf = np.zeros((2 * num_steps, 4), dtype=np.float64)
    rows, runs = C.c_int(), C.c_int64()
    E.check(E.lib().k5_dit_magcache_calibration(dit._handle, buf.ctypes.data_as(C.POINTER(C.c_double)), 2 * num_steps,
                                                C.byref(rows), C.byref(runs)), "magcache_calibration")
    assert rows.value == 2 * num_steps
    if runs.value < 1:
        raise RuntimeError("no complete calibration run yet")
    if rows_per_call is None:
        rows_per_call = getattr(dit, "_last_tokens", None)
    return calibration_from_sums(buf, num_steps, no_cfg, runs.value, rows_per_call)


def magcache_calibration_sums(dit):
    """The raw device table [2 * num_steps][4] and the number of complete runs (tests, averaging by hand)."""
    num_steps, _ = dit._magcache_calibrate
    buf = np.zeros((2 * num_steps, 4), dtype=np.float64)
    rows, runs = C.c_int(), C.c_int64()
    E.check(E.lib().k5_dit_magcache_calibration(dit._handle, buf.ctypes.data_as(C.POINTER(C.c_double)), 2 * num_steps,
                                                C.byref(rows), C.byref(runs)), "magcache_calibration")
    return buf, runs.value


def calibrate_magcache(pipe, prompts, **generate_kwargs):
    """Measure a MagCache ratio table for the pipeline's checkpoint: `pipe(prompt, **generate_kwargs)` once per prompt
    with the DiT in calibration mode (so `image=`, the clip length, the size, `num_steps`, `guidance_weight` are part of
    the workload; defaults come from the pipeline's config as in a normal call).  The pipeline has no way to stop after
    the latent, so each run decodes and the frames are discarded (`save_path` is forced to None).  Returns the dict of
    `magcache_calibration`; the DiT's previous MagCache state is restored."""
    if isinstance(prompts, str):
        prompts = [prompts]
    if not prompts:
        raise ValueError("calibrate_magcache needs at least one prompt")
    dit, conf = pipe.dit, pipe.conf
    if getattr(pipe, "world_size", 1) > 1:
        raise RuntimeError("calibrate_magcache is a one-GPU job (the engine refuses rank groups while calibrating)")
    num_steps = generate_kwargs.get("num_steps") or conf.model.num_steps
    guidance = generate_kwargs.get("guidance_weight")
    guidance = conf.model.guidance_weight if guidance is None else guidance
    no_cfg = abs(guidance - 1.0) <= 1e-6
    kwargs = dict(generate_kwargs, save_path=None)
    saved = None
    if getattr(dit, "mag_ratios", None) is not None:
        saved = {k: getattr(dit, k) for k in ("num_steps", "magcache_thresh", "K", "retention_ratio", "mag_ratios", "no_cfg")}
        disable_magcache(dit)
    try:
        start_magcache_calibration(dit, num_steps, no_cfg)
        for prompt in prompts:
            pipe(prompt, **kwargs)
        return magcache_calibration(dit)
    finally:
        stop_magcache_calibration(dit)
        if saved is not None:
            for k, v in saved.items():
                setattr(dit, k, v)
            _apply(dit)


def load_mag_ratios(source):
    """`magcache_ratios=` of get_T2V_pipeline: a list of ratios, a dict holding `mag_ratios` (what calibrate_magcache
    returns, or a config's `magcache` section), or the path of a JSON / YAML file holding either."""
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        import os
        path = os.fspath(source)
        with open(path) as f:
            text = f.read()
        if path.lower().endswith(".json"):
            import json
            source = json.loads(text)
        else:
            import yaml
            source = yaml.safe_load(text)
    if isinstance(source, dict) or hasattr(source, "keys"):
        if "mag_ratios" in source:
            source = source["mag_ratios"]
        elif "magcache" in source and "mag_ratios" in source["magcache"]:
            source = source["magcache"]["mag_ratios"]
        else:
            raise ValueError("no `mag_ratios` in the MagCache ratio file / dict")
    ratios = [float(v) for v in source]
    if len(ratios) < 2 or len(ratios) % 2:
        raise ValueError(f"mag_ratios must hold an even number (cond / uncond interleaved) of at least 2 ratios, got {len(ratios)}")
    return ratios
