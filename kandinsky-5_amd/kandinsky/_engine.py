"""ctypes binding of libk5.so (C ABI: include/k5.h).

The product path has NO fallback: if the HIP library is missing or fails to load, importing a
function from here raises RuntimeError.  torch is used only for device memory and streams; every
call passes raw device pointers (`tensor.data_ptr()`) and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("K5_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libk5.so"))

K5_OK = 0
ABI_VERSION = 11         # include/k5.h K5_ABI_VERSION
K5_F32, K5_BF16, K5_F16 = 0, 1, 2
EPI_BIAS, EPI_BIAS_M, EPI_GELU, EPI_GATE = 0, 1, 2, 3

_DT = {torch.float32: K5_F32, torch.bfloat16: K5_BF16, torch.float16: K5_F16}


class DitConfig(C.Structure):
    _fields_ = [("in_visual_dim", C.c_int), ("in_text_dim", C.c_int), ("in_text_dim2", C.c_int),
                ("time_dim", C.c_int), ("out_visual_dim", C.c_int), ("patch_size", C.c_int * 3),
                ("model_dim", C.c_int), ("ff_dim", C.c_int), ("num_text_blocks", C.c_int),
                ("num_visual_blocks", C.c_int), ("axes_dims", C.c_int * 3), ("visual_cond", C.c_int)]


class TextCond(C.Structure):
    _fields_ = [("text_embed", C.c_void_p), ("pooled_embed", C.c_void_p), ("text_dtype", C.c_int),
                ("text_len", C.c_int), ("text_rope_pos", C.POINTER(C.c_int32))]


class ForwardArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("T", C.c_int), ("H", C.c_int), ("W", C.c_int), ("x_channels", C.c_int),
                ("cond", TextCond), ("time", C.c_float), ("pos_t", C.POINTER(C.c_int32)),
                ("pos_h", C.POINTER(C.c_int32)), ("pos_w", C.POINTER(C.c_int32)), ("scale_factor", C.c_float * 3),
                ("attention_type", C.c_int), ("nabla_P", C.c_float), ("nabla_wT", C.c_int), ("nabla_wH", C.c_int),
                ("nabla_wW", C.c_int)]


class SampleArgs(C.Structure):
    _fields_ = [("fwd", ForwardArgs), ("null_cond", TextCond), ("latent", C.c_void_p), ("num_steps", C.c_int),
                ("sigmas", C.POINTER(C.c_float)), ("guidance_weight", C.c_float)]


class SampleManyArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("fwd", ForwardArgs), ("conds", C.POINTER(TextCond)), ("null_conds", C.POINTER(TextCond)),
                ("latents", C.c_void_p), ("visual_cond", C.c_void_p), ("num_steps", C.c_int), ("sigmas", C.POINTER(C.c_float)),
                ("guidance_weight", C.c_float)]


class SampleWindowsArgs(C.Structure):   # k5_sample_windows_args
    _fields_ = [("sample", SampleArgs), ("total_T", C.c_int), ("nwin", C.c_int), ("starts", C.POINTER(C.c_int32)),
                ("weights", C.POINTER(C.c_float)), ("conds", C.POINTER(TextCond)), ("null_conds", C.POINTER(TextCond))]


class TilePlan(C.Structure):   # k5_tile_plan: the tables are device memory
    _fields_ = [("nt", C.c_int), ("ny", C.c_int), ("nx", C.c_int), ("Ft", C.c_int), ("Fh", C.c_int), ("Fw", C.c_int),
                ("starts_t", C.c_void_p), ("starts_y", C.c_void_p), ("starts_x", C.c_void_p),
                ("wt", C.c_void_p), ("wy", C.c_void_p), ("wx", C.c_void_p)]


class SampleTilesArgs(C.Structure):   # k5_sample_tiles_args: the tables are host memory
    _fields_ = [("sample", SampleArgs), ("total_T", C.c_int), ("total_H", C.c_int), ("total_W", C.c_int),
                ("nt", C.c_int), ("ny", C.c_int), ("nx", C.c_int),
                ("starts_t", C.POINTER(C.c_int32)), ("starts_y", C.POINTER(C.c_int32)), ("starts_x", C.POINTER(C.c_int32)),
                ("wt", C.POINTER(C.c_float)), ("wy", C.POINTER(C.c_float)), ("wx", C.POINTER(C.c_float)),
                ("conds", C.POINTER(TextCond)), ("null_conds", C.POINTER(TextCond))]


class EditArgs(C.Structure):
    _fields_ = [("source", C.c_void_p), ("noise", C.c_void_p), ("keep_mask", C.c_void_p)]


class WatchInfo(C.Structure):   # k5_watch_info
    _fields_ = [("step", C.c_int), ("num_steps", C.c_int), ("sample", C.c_int), ("num_samples", C.c_int), ("sigma_next", C.c_float),
                ("rgb", C.POINTER(C.c_uint8)), ("x0", C.POINTER(C.c_float)), ("T", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int)]


WATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(WatchInfo))   # k5_watch_fn: non-zero = stop


class Watch(C.Structure):       # k5_watch
    _fields_ = [("fn", WATCH_FN), ("user", C.c_void_p), ("preview_every", C.c_int), ("want_x0", C.c_int),
                ("rgb_w", C.POINTER(C.c_float)), ("rgb_b", C.POINTER(C.c_float))]


class WatchTrampoline:
    """The C side of a Python watch callback.  ctypes prints and swallows an exception that escapes a callback, so the trampoline catches
    it, keeps it in `error` for the caller of k5_sample* to re-raise, and answers "stop".  `stop_requested` tells a stop the callback asked
    for (a truthy return) from one forced by an exception.  `wrap(info)` turns the k5_watch_info into what the callback receives."""

    def __init__(self, callback, wrap=None):
        self.callback, self.wrap = callback, (wrap or (lambda info: info))
        self.error, self.stop_requested, self.last_sample = None, False, 0
        self.c_fn = WATCH_FN(self._call)   # kept alive with the trampoline: the engine holds the raw pointer

    def reset(self):
        self.error, self.stop_requested, self.last_sample = None, False, 0

    def _call(self, user, info):
        try:
            self.last_sample = int(getattr(info.contents, "sample", 0))   # which sample of a k5_sample_many call the callback last saw
            if self.callback(self.wrap(info.contents)):
                self.stop_requested = True
                return 1
            return 0
        except BaseException as e:   # noqa: BLE001 — KeyboardInterrupt too: it must come out of sample(), not vanish in ctypes
            self.error = e
            return 1

    def reraise(self):
        """Raise what the callback raised during the last call, once."""
        e, self.error = self.error, None
        if e is not None:
            raise e


class Guidance(C.Structure):
    """k5_guidance: the plan of k5_dit_set_guidance (weights is HOST memory, copied by the call)."""
    _fields_ = [("weights", C.POINTER(C.c_float)), ("num_weights", C.c_int), ("zero_star", C.c_int), ("zero_init_steps", C.c_int),
                ("rescale", C.c_float)]


class SkipGuidance(C.Structure):
    """k5_skip_guidance: the set of k5_dit_set_skip_guidance (blocks and steps are HOST memory, copied by the call)."""
    _fields_ = [("blocks", C.POINTER(C.c_int)), ("num_blocks", C.c_int), ("mode", C.c_int), ("scale", C.c_float),
                ("steps", C.POINTER(C.c_ubyte)), ("num_steps", C.c_int)]


class Enhance(C.Structure):
    """k5_enhance: the set of k5_dit_set_enhance (steps is HOST memory, copied by the call)."""
    _fields_ = [("weight", C.c_float), ("steps", C.POINTER(C.c_ubyte)), ("num_steps", C.c_int)]


class Forecast(C.Structure):
    """k5_forecast: the plan of k5_dit_set_forecast (full is HOST memory, copied by the call)."""
    _fields_ = [("order", C.c_int), ("full", C.POINTER(C.c_ubyte)), ("num_steps", C.c_int)]


class Stochastic(C.Structure):
    """k5_stochastic: the plan of k5_dit_set_stochastic (the three tables are HOST memory, copied by the call)."""
    _fields_ = [("num_steps", C.c_int), ("dt_down", C.POINTER(C.c_float)), ("scale", C.POINTER(C.c_float)),
                ("noise_coef", C.POINTER(C.c_float)), ("seed", C.c_uint64), ("first_stream", C.c_uint32)]


class EulerStep(C.Structure):
    """k5_euler_step_args: the sampler's update of one step, field for field (every pointer is device memory)."""
    _fields_ = [("img", C.c_void_p), ("v_cond", C.c_void_p), ("v_uncond", C.c_void_p), ("v_skip", C.c_void_p), ("v_out", C.c_void_p),
                ("ab", C.c_void_p), ("w", C.c_float), ("dt", C.c_float), ("skip_scale", C.c_float),
                ("source", C.c_void_p), ("noise", C.c_void_p), ("keep_mask", C.c_void_p), ("sigma_next", C.c_float),
                ("cells", C.c_int64), ("C", C.c_int),
                ("stochastic", C.c_int), ("scale", C.c_float), ("noise_coef", C.c_float), ("znoise", C.c_void_p), ("seed", C.c_uint64),
                ("stream_id", C.c_uint32)]


class FlowEditStep(C.Structure):
    """k5_flowedit_step_args: FlowEdit's pass of one step, field for field (every pointer is device memory)."""
    _fields_ = [("z_fe", C.c_void_p), ("x_src", C.c_void_p), ("c_src", C.c_void_p), ("u_src", C.c_void_p), ("c_tar", C.c_void_p),
                ("u_tar", C.c_void_p), ("w_src", C.c_float), ("w_tar", C.c_float), ("dt", C.c_float), ("keep_mask", C.c_void_p),
                ("prepare", C.c_int), ("sigma_next", C.c_float), ("zs", C.c_void_p), ("zt", C.c_void_p), ("znoise", C.c_void_p),
                ("seed", C.c_uint64), ("stream_id", C.c_uint32), ("cells", C.c_int64), ("C", C.c_int)]


class FlowEditArgs(C.Structure):
    """k5_flowedit_args: the source side of k5_sample_flowedit."""
    _fields_ = [("source", C.c_void_p), ("source_cond", TextCond), ("source_weight", C.c_float), ("keep_mask", C.c_void_p),
                ("refine", C.c_int), ("seed", C.c_uint64), ("first_stream", C.c_uint32)]


class VaeConfig(C.Structure):
    _fields_ = [("latent_channels", C.c_int), ("out_channels", C.c_int), ("block_out_channels", C.c_int * 4),
                ("layers_per_block", C.c_int), ("norm_num_groups", C.c_int)]


_lib: Optional[C.CDLL] = None

# name -> (restype, argtypes); every symbol declared in include/k5.h
_P, _I, _F, _I64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
SYMBOLS = {
    "k5_abi_version": (_I, []),
    "k5_last_error": (C.c_char_p, []),
    "k5_gemm_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P]),
    "k5_gemm_bf16_variant": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P, _I, _I]),
    "k5_gemm_bf16_f32out": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _P]),
    "k5_causal_softmax_bf16": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "k5_vae_attention512_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    "k5_attention_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "k5_attention_state_size": (_I64, [_I, _I]),
    "k5_attention_bf16_range": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _I, _I, _I, _I, _P, _I, _P]),
    "k5_gemm_fp8": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P]),
    "k5_gemm_fp8_ex": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _I]),
    "k5_quant_rows_fp8": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "k5_attention_bf16_prescaled": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P]),
    "k5_attention_bf16_prescaled_auto": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P]),
    "k5_attention_flags": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "k5_attention_flags_rows": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "k5_attention_bf16_prescaled_rows": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "k5_attention_bf16_prescaled_rows_pass": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _I, _P, _I, _I, _P, _P]),
    "k5_attention_bf16_prescaled_qnorm_pass": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _P, _I, _I, _P, _P]),
    "k5_rmsnorm_rope_centre_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P, _P, _P]),
    "k5_attention_flags_rows_centred": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "k5_attention_bf16_prescaled_rows_centred": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "k5_attention_flags_rows_anchored": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "k5_attention_row_anchor": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "k5_attention_bf16_prescaled_rows_anchored": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "k5_rmsnorm_rope_stats_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P, _P]),
    "k5_loopback_create": (_I, [_I, C.POINTER(_P)]),
    "k5_loopback_destroy": (None, [_P]),
    "k5_dit_comm_init_loopback": (_I, [_P, _P, _I]),
    "k5_dit_cfg_pair_init": (_I, [_P, C.c_char_p, _I, _P]),
    "k5_dit_cfg_pair_init_loopback": (_I, [_P, _P, _I]),
    "k5_dit_comm_init_ipc": (_I, [_P, C.c_char_p, _I, _I]),
    "k5_dit_cfg_pair_init_ipc": (_I, [_P, C.c_char_p, _I]),
    "k5_dit_cfg_branch": (_I, [_P]),
    "k5_dit_set_option": (_I, [_P, C.c_char_p, _I]),
    "k5_dit_get_option": (_I, [_P, C.c_char_p, C.POINTER(_I)]),
    "k5_dit_sp_schedule": (_I, [_P, C.c_char_p, _I]),
    "k5_sp_pick_schedule": (_I, [C.POINTER(C.c_float), _I, _I, C.POINTER(_I), C.POINTER(C.c_float)]),
    "k5_sp_plan_2d": (_I, [_I, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(C.c_longlong)]),
    "k5_dit_attn_variant_counts": (_I, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), _I]),
    "k5_dit_nabla_block_counts": (_I, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "k5_dit_set_nabla_tap": (_I, [_P, _P, C.c_longlong]),
    "k5_dit_nabla_tap_count": (_I, [_P, C.POINTER(C.c_longlong)]),
    "k5_dit_nabla_executed_blocks": (_I, [_P, C.POINTER(C.c_longlong)]),
    "k5_attention_balance_size": (_I64, [_I, _I]),
    "k5_attention_bf16_balanced": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "k5_nabla_workspace_size": (_I64, [_I, _I]),
    "k5_nabla_select_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "k5_attention_nabla_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "k5_nabla_mask_u8": (_I, [_P, _I, _I, _P, _P]),
    "k5_nabla_select_rect_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "k5_attention_nabla_rect_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _I, _I64, _P]),
    "k5_nabla_select_rect_local_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _I, _I, _P]),
    "k5_attention_nabla_rect_prescaled_pass": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _I64, _P, _P, _I, _P, _P]),
    "k5_nabla_mask_rect_u8": (_I, [_P, _I, _I, _I, _P, _P]),
    "k5_attention_bf16_bounded": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P]),
    "k5_ln_modulate_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "k5_rmsnorm_rope_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "k5_gate_sum_bf16": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "k5_magcache_stats_bf16": (_I, [_P, _P, _P, _P, _P, _I, _I, _P]),
    "k5_gemv_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "k5_time_features_f32": (_I, [_F, _P, _I, _P]),
    "k5_ln_affine_bf16": (_I, [_P, _P, _P, _P, _P, _I, _I, _P]),
    "k5_rope_table_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _F, _F, _P, _P]),
    "k5_patchify_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "k5_patchify_cond_bf16": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "k5_unpatchify_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "k5_cfg_euler": (_I, [_P, _P, _P, _F, _F, _I64, _P]),
    "k5_dit_create": (_I, [C.POINTER(DitConfig), C.POINTER(_P)]),
    "k5_dit_destroy": (None, [_P]),
    "k5_dit_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(_I64), _I]),
    "k5_dit_finalize": (_I, [_P]),
    "k5_dit_missing_keys": (_I, [_P]),
    "k5_dit_forward": (_I, [_P, C.POINTER(ForwardArgs), _P, _P]),
    "k5_sample": (_I, [_P, C.POINTER(SampleArgs), _P]),
    "k5_sample_cond": (_I, [_P, C.POINTER(SampleArgs), _P, _P]),
    "k5_sample_many": (_I, [_P, C.POINTER(SampleManyArgs), _P]),
    "k5_sample_edit": (_I, [_P, C.POINTER(SampleArgs), _P, C.POINTER(EditArgs), _P]),
    "k5_edit_renoise": (_I, [_P, _P, _P, _F, _I64, _P]),
    "k5_cfg_euler_edit": (_I, [_P, _P, _P, _F, _F, _P, _P, _P, _F, _I64, _I, _P]),
    "k5_guidance_stats_blocks": (_I, [_I64]),
    "k5_guidance_coeffs_bf16": (_I, [_P, _P, _I64, _F, _I, _F, _P, _P, _P, _P]),
    "k5_guided_euler": (_I, [_P, _P, _P, _P, _F, _P, _P, _P, _F, _I64, _I, _P, _P]),
    "k5_skip_euler": (_I, [_P, _P, _P, _P, _F, _P, _F, _F, _P, _P, _P, _F, _I64, _I, _P, _P]),
    "k5_philox_words": (_I, [_P, C.c_uint64, _I64, C.c_uint64, C.c_uint32, C.c_uint32, _P]),
    "k5_noise_normal_f32": (_I, [_P, _I64, C.c_uint64, C.c_uint32, _P]),
    "k5_stochastic_euler": (_I, [_P, _P, _P, _P, _F, _P, _F, _F, _P, _P, _P, _F, _I64, _I, _P, _F, _F, _P, C.c_uint64, C.c_uint32, _P]),
    "k5_euler_step": (_I, [C.POINTER(EulerStep), _P]),
    "k5_flowedit_step": (_I, [C.POINTER(FlowEditStep), _P]),
    "k5_sample_flowedit": (_I, [_P, C.POINTER(SampleArgs), C.POINTER(FlowEditArgs), _P, _P]),
    "k5_dit_flowedit_state": (_I, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), _I]),
    "k5_dit_set_stochastic": (_I, [_P, C.POINTER(Stochastic)]),
    "k5_dit_stochastic_state": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_longlong), _I]),
    "k5_cfg_euler_windows": (_I, [_P, _P, _P, _F, _F, _P, _P, _I, _I, _I, _I64, _P]),
    "k5_sample_windows": (_I, [_P, C.POINTER(SampleWindowsArgs), _P, _P]),
    "k5_cfg_euler_tiles": (_I, [_P, _P, _P, _F, _F, C.POINTER(TilePlan), _I, _I, _I, _I, _P]),
    "k5_patchify_view_bf16": (_I, [_P, _I64, _I64, _P, _I64, _I64, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "k5_sample_tiles": (_I, [_P, C.POINTER(SampleTilesArgs), _P, _P]),
    "k5_x0_preview": (_I, [_P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P, _I64, _I, _P]),
    "k5_dit_set_watch": (_I, [_P, C.POINTER(Watch)]),
    "k5_dit_watch_state": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "k5_nag_combine_bf16": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _F, _P]),
    "k5_dit_set_nag": (_I, [_P, C.POINTER(TextCond), _F, _F, _F]),
    "k5_dit_nag_state": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_longlong), _I]),
    "k5_dit_set_guidance": (_I, [_P, C.POINTER(Guidance)]),
    "k5_dit_guidance_state": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), _I]),
    "k5_dit_set_skip_guidance": (_I, [_P, C.POINTER(SkipGuidance)]),
    "k5_dit_skip_state": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), _I]),
    "k5_dit_forward_skip": (_I, [_P, C.POINTER(ForwardArgs), _P, _P, _P]),
    "k5_enhance_part_count": (C.c_longlong, [_I, _I]),
    "k5_enhance_scores_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _F, _F, _P, _P, _P]),
    "k5_scale_by_dev_bf16": (_I, [_P, _I, _I, _I, _P, _P]),
    "k5_dit_set_enhance": (_I, [_P, C.POINTER(Enhance)]),
    "k5_dit_enhance_state": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_longlong), C.POINTER(C.c_float), _I, C.POINTER(_I), _I]),
    "k5_forecast_update_bf16": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "k5_forecast_apply_bf16": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "k5_dit_set_forecast": (_I, [_P, C.POINTER(Forecast)]),
    "k5_dit_forecast_at": (_I, [_P, _I, _I]),
    "k5_dit_forecast_state": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), _I]),
    "k5_region_combine_bf16": (_I, [_P, _P, C.c_longlong, _I, _P, _I, _P, _I, _I, _I, _P]),
    "k5_region_weights_f32": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P]),
    "k5_dit_set_regions": (_I, [_P, C.POINTER(TextCond), _I, _P, _I, _I, _I, _F]),
    "k5_dit_regions_state": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_longlong), _I]),
    "k5_dit_forward_many": (_I, [_P, C.POINTER(ForwardArgs), _I, C.POINTER(TextCond), _P, _P]),
    "k5_comm_unique_id": (_I, [C.c_char_p, _P]),
    "k5_dit_comm_init": (_I, [_P, C.c_char_p, _I, _I, _P]),
    "k5_conv3d_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "k5_conv3d_strided_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "k5_groupnorm_workspace_size": (_I64, [_I, _I]),
    "k5_groupnorm_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _I, _P, _P]),
    "k5_conv3d_stats_size": (_I64, [_I, _I]),
    "k5_conv3d_bf16_stats": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P]),
    "k5_groupnorm_bf16_quads": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _I, _P, _P, _P]),
    "k5_vae_path_counts": (_I, [_P, C.POINTER(C.c_longlong), _I]),
    "k5_vae_create": (_I, [C.POINTER(VaeConfig), C.POINTER(_P)]),
    "k5_vae_destroy": (None, [_P]),
    "k5_vae_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(_I64), _I]),
    "k5_vae_finalize": (_I, [_P]),
    "k5_vae_decode_tile": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "k5_vae_encode_tile": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "k5_vae_has_encoder": (_I, [_P]),
    "k5_blend_bf16": (_I, [_P, _P, _I64, _I, _I, _I64, _I, _P]),
    "k5_blend_place_bf16": (_I, [_P, _I64, _I, _P, _I64, _I, _P, _I64, _I64, _I64, _I, _I, _P]),
    "k5_frames_to_uint8": (_I, [_P, _P, _I64, _P]),
    "k5_vae_decode_tile_strided": (_I, [_P, _P, _I64, _I, _I, _I, _P, _P]),
    "k5_dit_set_graph": (_I, [_P, _I]),
    "k5_dit_set_fp8": (_I, [_P, _I]),
    "k5_lora_merge": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _F, _P]),
    "k5_dit_add_lora": (_I, [_P, C.c_char_p, _P, _I, _P, _I, _I, _F]),
    "k5_dit_clear_lora": (_I, [_P]),
    "k5_dit_lora_state": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_longlong)]),
    "k5_dit_set_magcache": (_I, [_P, C.POINTER(C.c_double), _I, _I, C.c_double, _I, C.c_double]),
    "k5_dit_magcache_calls": (_I, [_P, _I, _I]),
    "k5_dit_magcache_state": (_I, [_P, C.POINTER(_I), C.POINTER(_I64), C.POINTER(_I64)]),
    "k5_dit_set_magcache_calibrate": (_I, [_P, _I, _I]),
    "k5_dit_magcache_calibration": (_I, [_P, C.POINTER(C.c_double), _I, C.POINTER(_I), C.POINTER(_I64)]),
    "k5_dit_set_profiling": (_I, [_P, _I]),
    "k5_dit_get_profile": (_I, [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_I64)]),
    "k5_dit_reset_profile": (_I, [_P]),
}


def lib() -> C.CDLL:
    """Load libk5.so once; raise loudly if it is not there (no CPU / eager fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libk5.so not found at {LIB_PATH}: build it with `python kandinsky-5_amd/build.py` "
            "(hipcc --offload-arch=gfx950). There is no fallback path.")
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise RuntimeError(f"failed to load {LIB_PATH}: {e}") from e
    try:
        L.k5_abi_version.restype = C.c_int
        have = L.k5_abi_version()
    except AttributeError as e:
        raise RuntimeError(f"{LIB_PATH} is not a libk5.so (no k5_abi_version)") from e
    if have != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} has C ABI version {have}, this host binding needs {ABI_VERSION}: rebuild it with "
                           "`python kandinsky-5_amd/build.py`")
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:   # a libk5.so of the same ABI number from before an added export (the MagCache calibration, LoRA, editing and watch ones)
            raise RuntimeError(f"{LIB_PATH} does not export {name}: rebuild it with `python kandinsky-5_amd/build.py`") from e
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


class LoopbackGroup:
    """k5_loopback: `world` engine handles of this process act as the ranks of one sequence-parallel group on one GPU
    (each rank driven by its own host thread).  Test infrastructure for the multi-GPU code path."""

    def __init__(self, world: int):
        h = C.c_void_p()
        check(lib().k5_loopback_create(int(world), C.byref(h)), "k5_loopback_create")
        self.handle, self.world = h, int(world)

    def __del__(self):
        try:
            if self.handle:
                lib().k5_loopback_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def last_error() -> str:
    return (lib().k5_last_error() or b"").decode()


def check(status: int, what: str = "libk5"):
    if status != K5_OK:
        raise RuntimeError(f"{what} failed with status {status}: {last_error()}")


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def k5_dtype(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}")


def i32_array(values):
    vals = [int(v) for v in values]
    return (C.c_int32 * len(vals))(*vals)


# ------------------------------------------------------------------------------------------
# thin op wrappers over torch device tensors (parity tests, host glue)
# ------------------------------------------------------------------------------------------
def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("libk5 kernels run on the GPU only: got a CPU tensor (no CPU fallback)")


def gemm(a, w, bias=None, epilogue=EPI_BIAS, resid=None, gate=None, out=None, kernel=0, token_tile=0):
    """out[M,N] = a[M,K] @ w[N,K]^T (+bias) with fused epilogue. a, w bf16; bias/gate fp32.
    kernel / token_tile != 0: the named kernel / tile height (k5_gemm_bf16_variant; tests and A/B tools): kernel 2 = 128 x 128 tiles,
    4 = the four-wave persistent kernel, 8 = the eight-wave kernel; any other kernel id raises.  token_tile 128 / 192 / 256 = rows of the
    four-wave kernel's workgroup tile."""
    _need_cuda(a, w, bias, resid, gate)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    if kernel or token_tile:
        check(lib().k5_gemm_bf16_variant(ptr(a), ptr(w), ptr(bias), ptr(out), M, N, K, a.stride(0), w.stride(0), out.stride(0),
                                         epilogue, ptr(resid), 0 if resid is None else resid.stride(0), ptr(gate),
                                         stream_ptr(a.device), int(kernel), int(token_tile)), "k5_gemm_bf16_variant")
        return out
    check(lib().k5_gemm_bf16(ptr(a), ptr(w), ptr(bias), ptr(out), M, N, K, a.stride(0), w.stride(0), out.stride(0),
                             epilogue, ptr(resid), 0 if resid is None else resid.stride(0), ptr(gate),
                             stream_ptr(a.device)), "k5_gemm_bf16")
    return out


def attention(q, k, vt, num_heads, q_len=None, kv_len=None, out=None, score_bound=None):
    """q [Sq, >=H*64] , k [Sk, >=H*64], vt [H*64, >=Sk] bf16 -> out [Sq, H*64]."""
    _need_cuda(q, k, vt)
    q_len = q.shape[0] if q_len is None else q_len
    kv_len = k.shape[0] if kv_len is None else kv_len
    if out is None:
        out = torch.empty(q_len, num_heads * 64, dtype=torch.bfloat16, device=q.device)
    if score_bound is not None:
        check(lib().k5_attention_bf16_bounded(ptr(q), ptr(k), ptr(vt), ptr(out), num_heads, q_len, kv_len, q.stride(0),
                                              k.stride(0), vt.stride(0), out.stride(0), float(score_bound),
                                              stream_ptr(q.device)), "k5_attention_bf16_bounded")
        return out
    check(lib().k5_attention_bf16(ptr(q), ptr(k), ptr(vt), ptr(out), num_heads, q_len, kv_len, q.stride(0), k.stride(0),
                                  vt.stride(0), out.stride(0), stream_ptr(q.device)), "k5_attention_bf16")
    return out


def nabla_select(q, k, num_heads, grid, window, P):
    """q, k [N, >=H*64] bf16 (fractal order); grid = (T, Hb, Wb); window = (wT, wH, wW).  Returns the workspace."""
    _need_cuda(q, k)
    N, nb = q.shape[0], q.shape[0] // 64
    ws = torch.empty(lib().k5_nabla_workspace_size(num_heads, nb), dtype=torch.uint8, device=q.device)
    check(lib().k5_nabla_select_bf16(ptr(q), ptr(k), q.stride(0), k.stride(0), num_heads, N, grid[0], grid[1], grid[2],
                                     window[0], window[1], window[2], float(P), ptr(ws), stream_ptr(q.device)),
          "k5_nabla_select_bf16")
    return ws


def nabla_mask(ws, num_heads, nb):
    out = torch.empty(num_heads, nb, nb, dtype=torch.uint8, device=ws.device)
    check(lib().k5_nabla_mask_u8(ptr(ws), num_heads, nb, ptr(out), stream_ptr(ws.device)), "k5_nabla_mask_u8")
    return out.bool()


def attention_nabla(q, k, vt, num_heads, ws, score_bound=0.0, out=None):
    _need_cuda(q, k, vt, ws)
    N = q.shape[0]
    if out is None:
        out = torch.empty(N, num_heads * 64, dtype=torch.bfloat16, device=q.device)
    check(lib().k5_attention_nabla_bf16(ptr(q), ptr(k), ptr(vt), ptr(out), num_heads, N, q.stride(0), k.stride(0),
                                        vt.stride(0), out.stride(0), float(score_bound), ptr(ws), stream_ptr(q.device)),
          "k5_attention_nabla_bf16")
    return out


def ln_modulate(x, scale, shift):
    _need_cuda(x, scale, shift)
    out = torch.empty_like(x)
    check(lib().k5_ln_modulate_bf16(ptr(x), ptr(scale), ptr(shift), ptr(out), x.shape[0], x.shape[1], x.stride(0),
                                    out.stride(0), stream_ptr(x.device)), "k5_ln_modulate_bf16")
    return out


def rmsnorm_rope_(x, weight, cos=None, sin=None, heads=None, heads_per_weight=None, rope_heads=None):
    _need_cuda(x, weight, cos, sin)
    heads = x.shape[1] // 64 if heads is None else heads
    check(lib().k5_rmsnorm_rope_bf16(ptr(x), ptr(weight), ptr(cos), ptr(sin), x.shape[0], heads, x.stride(0),
                                     heads if heads_per_weight is None else heads_per_weight,
                                     heads if rope_heads is None else rope_heads, stream_ptr(x.device)),
          "k5_rmsnorm_rope_bf16")
    return x


def gate_sum(x, y, gate):
    _need_cuda(x, y, gate)
    out = torch.empty_like(x)
    check(lib().k5_gate_sum_bf16(ptr(x), ptr(y), ptr(gate), ptr(out), x.shape[0], x.shape[1], stream_ptr(x.device)),
          "k5_gate_sum_bf16")
    return out


def magcache_stats(vis, ori, prev=None, out=None):
    """(res, sums): res = bf16(vis - ori) and the four float64 sums of the MagCache calibration pass against `prev` (k5_magcache_stats_bf16);
    `out` may be `ori` itself."""
    _need_cuda(vis, ori, prev, out)
    res = torch.empty_like(vis) if out is None else out
    sums = torch.empty(4, dtype=torch.float64, device=vis.device)
    check(lib().k5_magcache_stats_bf16(ptr(vis), ptr(ori), ptr(prev), ptr(res), ptr(sums), vis.shape[0], vis.shape[1],
                                       stream_ptr(vis.device)), "k5_magcache_stats_bf16")
    return res, sums


def lora_merge_(w, a, b, scale, cols=None):
    """In place: w[:, :cols] += scale * (b @ a) (k5_lora_merge).  w bf16 or fp32 [rows][ld] with a unit inner stride, a [R][cols], b [rows][R],
    each f32 / bf16 / f16 and contiguous; fixed float64 fma order, one rounding to w's dtype."""
    _need_cuda(w, a, b)
    cols = a.shape[1] if cols is None else int(cols)
    if w.stride(1) != 1 or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError("lora_merge_: w needs a unit inner stride, a and b must be contiguous")
    check(lib().k5_lora_merge(ptr(w), k5_dtype(w), w.shape[0], cols, w.stride(0), ptr(a), k5_dtype(a), ptr(b), k5_dtype(b), a.shape[0],
                              float(scale), stream_ptr(w.device)), "k5_lora_merge")
    return w


def gemv_f32(x, w, b=None, silu_in=False, add=None):
    _need_cuda(x, w, b, add)
    y = torch.empty(w.shape[0], dtype=torch.float32, device=x.device)
    check(lib().k5_gemv_f32(ptr(x), ptr(w), ptr(b), ptr(y), w.shape[0], w.shape[1], int(silu_in), ptr(add),
                            stream_ptr(x.device)), "k5_gemv_f32")
    return y


def _check_step(name, img, v_cond, v_uncond=None, v_skip=None, v_out=None, ab=None, source=None, noise=None, keep_mask=None, z=None, need=()):
    """The checks that every wrapper of the sampler's update shares, raised under the wrapper's `name`: img, source, noise and z contiguous fp32
    tensors of one size, the velocities contiguous bf16 tensors of that size, ab fp32 [2], a keep_mask with one value per cell together with
    source and noise, v_cond and the tensors named in `need` given, all of them on one device, which is a GPU.  Returns (cells, C) of an img
    (..., C)."""
    given = dict(v_cond=v_cond, v_uncond=v_uncond, v_skip=v_skip, v_out=v_out, ab=ab, source=source, noise=noise, keep_mask=keep_mask, z=z)
    C_ = img.shape[-1]
    cells = img.numel() // C_
    for t in (img, source, noise, z):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != img.numel()):
            raise ValueError(f"{name}: img, source, noise and z must be contiguous fp32 tensors of one size")
    for v in (v_cond, v_uncond, v_skip, v_out):
        if v is not None and (v.dtype != torch.bfloat16 or not v.is_contiguous() or v.numel() != img.numel()):
            raise ValueError(f"{name}: the velocities must be contiguous bf16 tensors of img's size")
    missing = [k for k in ("v_cond",) + tuple(need) if given[k] is None]
    if missing:
        raise ValueError(f"{name}: this update needs {' and '.join(missing)}")
    if ab is not None and (ab.dtype != torch.float32 or ab.numel() != 2 or not ab.is_contiguous()):
        raise ValueError(f"{name}: ab must be a contiguous fp32 [2] tensor on the device")
    if keep_mask is not None and (source is None or noise is None or keep_mask.dtype != torch.float32 or not keep_mask.is_contiguous()
                                  or keep_mask.numel() != cells):
        raise ValueError(f"{name}: keep_mask must be a contiguous fp32 tensor with one value per cell and needs source and noise")
    if any(t is not None and t.device != img.device for t in given.values()):
        raise ValueError(f"{name}: img and every other tensor must be on one device")
    _need_cuda(img)
    return cells, C_


def euler_step_(img, v_cond, v_uncond=None, *, w=1.0, dt, ab=None, v_skip=None, g=0.0, source=None, noise=None, keep_mask=None, sigma_next=0.0,
                v_out=None, stochastic=None):
    """The sampler's update of one step, in place on img fp32 (..., C) (k5_euler_step; the rule is written at k5_euler_step_args in
    include/k5.h).  The velocity: v_cond itself, with v_uncond the CFG combine at weight w or, with ab (fp32 [2] on the device, from
    `guidance_coeffs`), ab[0] v_cond + ab[1] v_uncond; with v_skip, + g (v_cond - v_skip).  img += bf16(dt v).  stochastic = (scale, noise_coef,
    seed, stream_id[, z]): then, where noise_coef != 0, img = scale img + noise_coef z with z the fp32 tensor `z` or, without one, the
    generator's normals of (seed, stream_id) — `noise_normal_`'s bits; dt is then the step's dt_down.  Last, with a keep_mask (fp32 (..., 1), with
    source and noise, the edit's eps), the keep rule at sigma_next.  v_out (bf16 of img's size, may be v_cond; with ab or v_skip) receives v.
    The five wrappers below are fixed forms of this call."""
    scale, noise_coef, seed, stream_id, z = (1.0, 0.0, 0, 0, None) if stochastic is None else (*stochastic, None)[:5]
    cells, C_ = _check_step("euler_step_", img, v_cond, v_uncond, v_skip, v_out, ab, source, noise, keep_mask, z)
    a = EulerStep(img=ptr(img), v_cond=ptr(v_cond), v_uncond=ptr(v_uncond), v_skip=ptr(v_skip), v_out=ptr(v_out), ab=ptr(ab), w=float(w),
                  dt=float(dt), skip_scale=float(g), source=ptr(source), noise=ptr(noise), keep_mask=ptr(keep_mask), sigma_next=float(sigma_next),
                  cells=cells, C=C_, stochastic=int(stochastic is not None), scale=float(scale), noise_coef=float(noise_coef), znoise=ptr(z),
                  seed=int(seed) & (2 ** 64 - 1), stream_id=int(stream_id) & 0xffffffff)
    with torch.cuda.device(img.device):
        check(lib().k5_euler_step(C.byref(a), stream_ptr(img.device)), "k5_euler_step")
    return img


def flowedit_step_(z_fe, x_src, c_src=None, u_src=None, c_tar=None, u_tar=None, *, w_src=1.0, w_tar=1.0, dt=0.0, keep_mask=None, sigma_next=None,
                   zs=None, zt=None, seed=0, stream_id=0, z=None):
    """FlowEdit's pass of one step (k5_flowedit_step; the rule is written at k5_flowedit_step_args in include/k5.h).  With the velocities (bf16,
    c_src and c_tar both; u_src / u_tar where the side's weight is not 1): z_fe += bf16(dt bf16(v_tar - v_src)) in place, under keep_mask (fp32,
    one value per cell).  With sigma_next (the next step's sigma): zs = (1 - sigma_next) x_src + sigma_next z and zt = zs + (z_fe - x_src) are
    written for the next step, z the fp32 tensor `z` or the generator's normals of (seed, stream_id).  Without velocities the call only
    prepares.  Returns z_fe."""
    for t in (z_fe, x_src, zs, zt, z):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != z_fe.numel()):
            raise ValueError("flowedit_step_: z_fe, x_src, zs, zt and z must be contiguous fp32 tensors of one size")
    for v in (c_src, u_src, c_tar, u_tar):
        if v is not None and (v.dtype != torch.bfloat16 or not v.is_contiguous() or v.numel() != z_fe.numel()):
            raise ValueError("flowedit_step_: the velocities must be contiguous bf16 tensors of z_fe's size")
    C_ = z_fe.shape[-1]
    cells = z_fe.numel() // C_
    if keep_mask is not None and (keep_mask.dtype != torch.float32 or not keep_mask.is_contiguous() or keep_mask.numel() != cells):
        raise ValueError("flowedit_step_: keep_mask must be a contiguous fp32 tensor with one value per cell")
    if any(t is not None and t.device != z_fe.device for t in (x_src, c_src, u_src, c_tar, u_tar, keep_mask, zs, zt, z)):
        raise ValueError("flowedit_step_: z_fe and every other tensor must be on one device")
    _need_cuda(z_fe)
    a = FlowEditStep(z_fe=ptr(z_fe), x_src=ptr(x_src), c_src=ptr(c_src), u_src=ptr(u_src), c_tar=ptr(c_tar), u_tar=ptr(u_tar), w_src=float(w_src),
                     w_tar=float(w_tar), dt=float(dt), keep_mask=ptr(keep_mask), prepare=int(sigma_next is not None),
                     sigma_next=float(sigma_next or 0.0), zs=ptr(zs), zt=ptr(zt), znoise=ptr(z), seed=int(seed) & (2 ** 64 - 1),
                     stream_id=int(stream_id) & 0xffffffff, cells=cells, C=C_)
    with torch.cuda.device(z_fe.device):
        check(lib().k5_flowedit_step(C.byref(a), stream_ptr(z_fe.device)), "k5_flowedit_step")
    return z_fe


def cfg_euler_(img, v_cond, v_uncond, w, dt):
    """euler_step_(img, v_cond, v_uncond, w=w, dt=dt) through its own entry (k5_cfg_euler)."""
    _check_step("cfg_euler_", img, v_cond, v_uncond)
    with torch.cuda.device(img.device):
        check(lib().k5_cfg_euler(ptr(img), ptr(v_cond), ptr(v_uncond), float(w), float(dt), img.numel(), stream_ptr(img.device)), "k5_cfg_euler")
    return img


def window_tables(starts, weights, device):
    """The plan of `generation_utils.context_windows` as the device tables of `cfg_euler_windows_`: (int32 [nwin], fp32 [nwin][F])."""
    st = torch.tensor([int(v) for v in starts], dtype=torch.int32, device=device)
    wt = torch.tensor([[float(v) for v in row] for row in weights], dtype=torch.float32, device=device)
    if wt.dim() != 2 or wt.shape[0] != st.numel():
        raise ValueError("window_tables: weights must hold one row of F values per window")
    return st, wt.contiguous()


def cfg_euler_windows_(img, v_cond, v_uncond, w, dt, starts, weights):
    """cfg_euler_ over temporal context windows (k5_cfg_euler_windows): img fp32 (T, ...), v_cond / v_uncond (None = no guidance) bf16
    (nwin, F, ...) with the frame shape of img, `starts` int32 [nwin] and `weights` fp32 [nwin][F] on img's device (`window_tables`)."""
    _need_cuda(img, v_cond, v_uncond, starts, weights)
    if img.dtype != torch.float32 or not img.is_contiguous() or img.dim() < 2:
        raise ValueError("cfg_euler_windows_: img must be a contiguous fp32 tensor (T, ...)")
    if starts.dtype != torch.int32 or weights.dtype != torch.float32 or not starts.is_contiguous() or not weights.is_contiguous() \
            or weights.dim() != 2 or weights.shape[0] != starts.numel():
        raise ValueError("cfg_euler_windows_: starts must be int32 [nwin] and weights fp32 [nwin][F], contiguous")
    nwin, F = weights.shape
    T, frame = img.shape[0], img[0].numel()
    for v in (v_cond, v_uncond):
        if v is not None and (v.dtype != torch.bfloat16 or not v.is_contiguous() or v.numel() != nwin * F * frame):
            raise ValueError("cfg_euler_windows_: the velocities must be contiguous bf16 tensors (nwin, F) + img's frame shape")
    check(lib().k5_cfg_euler_windows(ptr(img), ptr(v_cond), ptr(v_uncond), float(w), float(dt), ptr(starts), ptr(weights), int(nwin), int(F),
                                     int(T), int(frame), stream_ptr(img.device)), "k5_cfg_euler_windows")
    return img


class TileTables:
    """The plan of `generation_utils.tile_windows` as the device tables of `cfg_euler_tiles_`: `.plan` is the k5_tile_plan, `.window` =
    (Ft, Fh, Fw), `.nwin`; the six tensors stay alive with the object."""

    def __init__(self, starts, weights, device):
        if len(starts) != 3 or len(weights) != 3:
            raise ValueError("tile_tables: starts and weights hold one entry per axis (t, y, x)")
        self.starts = [torch.tensor([int(v) for v in s], dtype=torch.int32, device=device) for s in starts]
        self.weights = [torch.as_tensor(w, dtype=torch.float32).to(device).contiguous() for w in weights]
        for s, w in zip(self.starts, self.weights):
            if w.dim() != 2 or w.shape[0] != s.numel() or s.numel() < 1:
                raise ValueError("tile_tables: the weights of an axis hold one row of F values per window of that axis")
        self.counts = tuple(int(s.numel()) for s in self.starts)
        self.window = tuple(int(w.shape[1]) for w in self.weights)
        self.nwin = self.counts[0] * self.counts[1] * self.counts[2]
        self.device = self.starts[0].device
        self.plan = TilePlan(*self.counts, *self.window, *(ptr(s) for s in self.starts), *(ptr(w) for w in self.weights))


def tile_tables(plan, device):
    """`generation_utils.tile_windows`' plan (anything with `.starts` and `.weights`, one entry per axis t, y, x) on `device`: a TileTables."""
    return TileTables(plan.starts, plan.weights, device)


def cfg_euler_tiles_(img, v_cond, v_uncond, w, dt, tables):
    """cfg_euler_ over a 3-D plan of context windows (k5_cfg_euler_tiles; the rule is written there in include/k5.h): img fp32 (T, H, W, C),
    v_cond / v_uncond (None = no guidance) bf16 (nwin, Ft, Fh, Fw, C), `tables` a TileTables on img's device."""
    _need_cuda(img, v_cond, v_uncond)
    if img.dtype != torch.float32 or not img.is_contiguous() or img.dim() != 4:
        raise ValueError("cfg_euler_tiles_: img must be a contiguous fp32 tensor (T, H, W, C)")
    if not isinstance(tables, TileTables) or tables.device != img.device:
        raise ValueError("cfg_euler_tiles_: tables must be the TileTables of `tile_tables` on img's device")
    T, H, W, C_ = img.shape
    n = tables.nwin * tables.window[0] * tables.window[1] * tables.window[2] * C_
    for v in (v_cond, v_uncond):
        if v is not None and (v.dtype != torch.bfloat16 or not v.is_contiguous() or v.numel() != n or v.device != img.device):
            raise ValueError("cfg_euler_tiles_: the velocities must be contiguous bf16 tensors (nwin, Ft, Fh, Fw, C) on img's device")
    with torch.cuda.device(img.device):
        check(lib().k5_cfg_euler_tiles(ptr(img), ptr(v_cond), ptr(v_uncond), float(w), float(dt), C.byref(tables.plan), int(T), int(H), int(W),
                                       int(C_), stream_ptr(img.device)), "k5_cfg_euler_tiles")
    return img


def patchify_view_(x, vcond, Cin_total, Kpad, tok_perm=None, out=None):
    """Patchify of a strided view (k5_patchify_view_bf16): x fp32 (T, H, W, Cx), a box sliced out of a larger contiguous tensor (its channel
    stride 1 and its column stride Cx), vcond (optional) likewise; channels up to Cin_total read as zero without one.  Returns bf16
    [T * H/2 * W/2][Kpad], rows in `tok_perm` order (int32, optional)."""
    _need_cuda(x, vcond, tok_perm, out)
    for name, t in (("x", x), ("vcond", vcond)):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.dim() != 4 or t.stride(3) != 1 or t.stride(2) != t.shape[3]:
            raise ValueError(f"patchify_view_: {name} must be an fp32 (T, H, W, C) view whose cells are contiguous and C apart along a row")
    T, H, W, Cx = x.shape
    if vcond is not None and (tuple(vcond.shape[:3]) != (T, H, W) or vcond.device != x.device):
        raise ValueError("patchify_view_: vcond must cover the cells of x, on its device")
    if out is None:
        out = torch.empty((T * (H // 2) * (W // 2), int(Kpad)), dtype=torch.bfloat16, device=x.device)
    vs = (0, 0) if vcond is None else (vcond.stride(0), vcond.stride(1))
    with torch.cuda.device(x.device):
        check(lib().k5_patchify_view_bf16(ptr(x), x.stride(0), x.stride(1), ptr(vcond), vs[0], vs[1], ptr(out), int(T), int(H), int(W), int(Cx),
                                          int(Cin_total), int(Kpad), ptr(tok_perm), stream_ptr(x.device)), "k5_patchify_view_bf16")
    return out


def renoise(source, noise, sigma, out=None):
    """rn(rn((1 - sigma) * source) + rn(sigma * noise)) (k5_edit_renoise): contiguous fp32 tensors of one shape; a new tensor unless `out`."""
    _need_cuda(source, noise, out)
    if out is None:
        out = torch.empty_like(source)
    for t in (source, noise, out):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != source.shape:
            raise ValueError("renoise: source, noise and out must be contiguous fp32 tensors of one shape")
    check(lib().k5_edit_renoise(ptr(out), ptr(source), ptr(noise), float(sigma), source.numel(), stream_ptr(source.device)),
          "k5_edit_renoise")
    return out


def cfg_euler_edit_(img, v_cond, v_uncond, w, dt, source, noise, keep_mask, sigma_next):
    """cfg_euler_ followed by the keep rule at sigma_next (k5_cfg_euler_edit): img, source, noise fp32 (..., C), keep_mask fp32 (..., 1) or
    None (= cfg_euler_)."""
    cells, C_ = _check_step("cfg_euler_edit_", img, v_cond, v_uncond, source=source, noise=noise, keep_mask=keep_mask)
    with torch.cuda.device(img.device):
        check(lib().k5_cfg_euler_edit(ptr(img), ptr(v_cond), ptr(v_uncond), float(w), float(dt), ptr(source), ptr(noise), ptr(keep_mask),
                                      float(sigma_next), cells, C_, stream_ptr(img.device)), "k5_cfg_euler_edit")
    return img


def guidance_coeffs(v_cond, v_uncond, w, zero_star=False, rescale=0.0, ab=None, sums=None):
    """(ab, sums) of one sample's two velocities (k5_guidance_coeffs_bf16): sums = float64 [5] (sum c, sum u, sum c^2, sum u^2, sum c u) in a fixed
    order, ab = fp32 [2] = (alpha, beta) of the guided velocity v = alpha c + beta u — alpha = w, beta = s (1 - w) with s = <c, u> / (<u, u> + 1e-8)
    under zero_star (else 1), both times rescale * std(c) / std(v) + 1 - rescale when rescale > 0.  Contiguous bf16 tensors of one size, a multiple
    of 8 elements; both results stay on the device (`ab`, `sums`: buffers to fill instead of new ones)."""
    for v in (v_cond, v_uncond):
        if v.dtype != torch.bfloat16 or not v.is_contiguous() or v.numel() != v_cond.numel():
            raise ValueError("guidance_coeffs: the velocities must be contiguous bf16 tensors of one size")
    _need_cuda(v_cond, v_uncond, ab, sums)
    n = v_cond.numel()
    if ab is None:
        ab = torch.empty(2, dtype=torch.float32, device=v_cond.device)
    if sums is None:
        sums = torch.empty(5, dtype=torch.float64, device=v_cond.device)
    if ab.dtype != torch.float32 or ab.numel() != 2 or sums.dtype != torch.float64 or sums.numel() != 5:
        raise ValueError("guidance_coeffs: ab must be fp32 [2] and sums float64 [5]")
    with torch.cuda.device(v_cond.device):
        part = torch.empty(max(1, lib().k5_guidance_stats_blocks(n)) * 5, dtype=torch.float64, device=v_cond.device)
        check(lib().k5_guidance_coeffs_bf16(ptr(v_cond), ptr(v_uncond), n, float(w), int(bool(zero_star)), float(rescale), ptr(part), ptr(sums),
                                            ptr(ab), stream_ptr(v_cond.device)), "k5_guidance_coeffs_bf16")
    return ab, sums


def guided_euler_(img, v_cond, v_uncond, ab, dt, source=None, noise=None, keep_mask=None, sigma_next=0.0, v_out=None):
    """The update of a guided step with coefficients from the device (k5_guided_euler): euler_step_ with both velocities and ab."""
    cells, C_ = _check_step("guided_euler_", img, v_cond, v_uncond, None, v_out, ab, source, noise, keep_mask, need=("v_uncond", "ab"))
    with torch.cuda.device(img.device):
        check(lib().k5_guided_euler(ptr(img), ptr(v_cond), ptr(v_uncond), ptr(ab), float(dt), ptr(source), ptr(noise), ptr(keep_mask),
                                    float(sigma_next), cells, C_, ptr(v_out), stream_ptr(img.device)), "k5_guided_euler")
    return img


def skip_euler_(img, v_cond, v_uncond, v_skip, w, g, dt, ab=None, source=None, noise=None, keep_mask=None, sigma_next=0.0, v_out=None):
    """The update of a skip-layer-guidance step (k5_skip_euler): euler_step_ with v_skip and g."""
    cells, C_ = _check_step("skip_euler_", img, v_cond, v_uncond, v_skip, v_out, ab, source, noise, keep_mask, need=("v_skip",))
    with torch.cuda.device(img.device):
        check(lib().k5_skip_euler(ptr(img), ptr(v_cond), ptr(v_uncond), ptr(v_skip), float(w), ptr(ab), float(g), float(dt), ptr(source),
                                  ptr(noise), ptr(keep_mask), float(sigma_next), cells, C_, ptr(v_out), stream_ptr(img.device)), "k5_skip_euler")
    return img


def philox_words(blk0, nblk, seed, c2=0, c3=0, device="cuda"):
    """The raw Philox4x32-10 words of blocks blk0 .. blk0 + nblk - 1 (mod 2^64) under key `seed` and counter words 2 / 3 = c2 / c3
    (k5_philox_words): an int32 [nblk][4] tensor holding the uint32 bit patterns."""
    out = torch.empty((int(nblk), 4), dtype=torch.int32, device=device)
    _need_cuda(out)
    with torch.cuda.device(out.device):
        check(lib().k5_philox_words(ptr(out), int(blk0) & (2 ** 64 - 1), int(nblk), int(seed) & (2 ** 64 - 1), int(c2) & 0xffffffff,
                                    int(c3) & 0xffffffff, stream_ptr(out.device)), "k5_philox_words")
    return out


def noise_normal_(out, seed, stream_id=0, n=None):
    """out.view(-1)[g] = standard normal g of stream `stream_id` under `seed` for g < n (default: all of out), from the counter-based generator
    (k5_noise_normal_f32): a pure function of (seed, stream_id, g).  out: a contiguous fp32 tensor on the device."""
    _need_cuda(out)
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("noise_normal_: out must be a contiguous fp32 tensor")
    n = out.numel() if n is None else int(n)
    if not 1 <= n <= out.numel():
        raise ValueError(f"noise_normal_: n must be in 1..{out.numel()} (got {n})")
    with torch.cuda.device(out.device):
        check(lib().k5_noise_normal_f32(ptr(out), n, int(seed) & (2 ** 64 - 1), int(stream_id) & 0xffffffff, stream_ptr(out.device)),
              "k5_noise_normal_f32")
    return out


def stochastic_euler_(img, v_cond, v_uncond, w, dt_down, scale, noise_coef, seed, stream_id, z=None, v_skip=None, g=0.0, ab=None, source=None,
                      noise=None, keep_mask=None, sigma_next=0.0, v_out=None):
    """The update of a stochastic step (k5_stochastic_euler): euler_step_ with dt = dt_down and stochastic = (scale, noise_coef, seed, stream_id,
    z).  noise_coef == 0 is the matching plain update bit for bit."""
    cells, C_ = _check_step("stochastic_euler_", img, v_cond, v_uncond, v_skip, v_out, ab, source, noise, keep_mask, z)
    with torch.cuda.device(img.device):
        check(lib().k5_stochastic_euler(ptr(img), ptr(v_cond), ptr(v_uncond), ptr(v_skip), float(w), ptr(ab), float(g), float(dt_down),
                                        ptr(source), ptr(noise), ptr(keep_mask), float(sigma_next), cells, C_, ptr(v_out), float(scale),
                                        float(noise_coef), ptr(z), int(seed) & (2 ** 64 - 1), int(stream_id) & 0xffffffff,
                                        stream_ptr(img.device)), "k5_stochastic_euler")
    return img


def nag_combine_(z_pos, z_neg, s, tau, alpha, out=None, D=None):
    """Normalized attention guidance on two cross-attention outputs, in place on z_pos unless `out` is given (k5_nag_combine_bf16): per row
    g = z_pos + (s - 1)(z_pos - z_neg), the growth of the row's L1 norm clamped at tau, blended back with alpha.  bf16 [rows][ld] tensors with
    a unit column stride; D (default: all ld columns) of each row are used, the rest is not touched."""
    out = z_pos if out is None else out
    for x in (z_pos, z_neg, out):
        if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1 or x.shape != z_pos.shape or x.stride(0) != z_pos.stride(0):
            raise ValueError("nag_combine_: z_pos, z_neg and out must be bf16 [rows][ld] tensors of one shape and row stride")
    rows, ld = z_pos.shape[0], z_pos.stride(0)
    D = z_pos.shape[1] if D is None else int(D)
    with torch.cuda.device(z_pos.device):
        check(lib().k5_nag_combine_bf16(ptr(z_pos), ptr(z_neg), ptr(out), rows, D, ld, float(s), float(tau), float(alpha),
                                        stream_ptr(z_pos.device)), "k5_nag_combine_bf16")
    return out


def enhance_scores(Q, K, Hh, T, S, weight, qk_scale, frame_rows=None):
    """The Enhance-A-Video score of one block (k5_enhance_scores_bf16): Q and K bf16 [rows][ld] tensors with a unit column stride (views of one
    fused buffer are fine) whose first 64 Hh columns are the heads, frame_rows int32 [S][T] on the device or None for row = t * S + p.  Returns
    (score_out fp32 [1], part float64 [S * Hh]) on the device, not synchronised."""
    for x in (Q, K):
        if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
            raise ValueError("enhance_scores: Q and K must be bf16 [rows][ld] tensors with a unit column stride")
    if frame_rows is not None and (frame_rows.dtype != torch.int32 or not frame_rows.is_contiguous()):
        raise ValueError("enhance_scores: frame_rows must be a contiguous int32 tensor")
    n = lib().k5_enhance_part_count(int(Hh), int(S))
    part = torch.zeros(max(int(n), 1), dtype=torch.float64, device=Q.device)
    score = torch.zeros(1, dtype=torch.float32, device=Q.device)
    with torch.cuda.device(Q.device):
        check(lib().k5_enhance_scores_bf16(ptr(Q), ptr(K), Q.stride(0), K.stride(0), int(Hh), int(T), int(S), ptr(frame_rows), float(qk_scale),
                                           float(weight), ptr(part), ptr(score), stream_ptr(Q.device)), "k5_enhance_scores_bf16")
    return score, part


def scale_by_dev_(x, score, D=None):
    """x *= score in place (k5_scale_by_dev_bf16): x bf16 [rows][ld] with a unit column stride of which D columns (default: all) are used,
    score a fp32 tensor of one element on the device; bf16(float(x) * s), and nothing is touched when s == 1."""
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1 or score.dtype != torch.float32:
        raise ValueError("scale_by_dev_: x must be a bf16 [rows][ld] tensor with a unit column stride, score fp32")
    with torch.cuda.device(x.device):
        check(lib().k5_scale_by_dev_bf16(ptr(x), x.shape[0], x.shape[1] if D is None else int(D), x.stride(0), ptr(score), stream_ptr(x.device)),
              "k5_scale_by_dev_bf16")
    return x


def region_combine_(z0, zr, w, out=None, D=None):
    """The regional-prompt blend, in place on z0 unless `out` is given (k5_region_combine_bf16): out = sum_i w_i z_i per row, stream 0 = z0
    (bf16 [rows][ld]), streams 1..R = zr (bf16 [R][rows][ld], the same row stride), w fp32 [rows][ldw] with ldw >= R + 1; a stream whose
    weight is 0 for a row is not read.  D (default: all ld columns) of each row are used, the rest is not touched."""
    out = z0 if out is None else out
    for x in (z0, out):
        if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1 or x.shape != z0.shape or x.stride(0) != z0.stride(0):
            raise ValueError("region_combine_: z0 and out must be bf16 [rows][ld] tensors of one shape and row stride")
    if (zr.dtype != torch.bfloat16 or zr.dim() != 3 or zr.shape[1:] != z0.shape or zr.stride(2) != 1 or zr.stride(1) != z0.stride(0)):
        raise ValueError("region_combine_: zr must be bf16 [R][rows][ld] with z0's row stride")
    if w.dtype != torch.float32 or w.dim() != 2 or w.shape[0] != z0.shape[0] or w.stride(1) != 1:
        raise ValueError("region_combine_: w must be fp32 [rows][ldw]")
    rows, ld = z0.shape[0], z0.stride(0)
    D = z0.shape[1] if D is None else int(D)
    with torch.cuda.device(z0.device):
        check(lib().k5_region_combine_bf16(ptr(z0), ptr(zr), zr.stride(0) if zr.shape[0] > 1 else rows * ld, zr.shape[0], ptr(w), w.stride(0),
                                           ptr(out), rows, D, ld, stream_ptr(z0.device)), "k5_region_combine_bf16")
    return out


def region_weights(masks, patch, base_weight, perm=None):
    """Token weights of regional prompts (k5_region_weights_f32): masks fp32 (R, T, H, W) on the device, patch (pt, ph, pw); returns fp32
    (N, R + 1), row i = token perm[i] (int32 tensor on the device; None: i) of the row-major token grid."""
    if masks.dtype != torch.float32 or masks.dim() != 4 or not masks.is_contiguous():
        raise ValueError("region_weights: masks must be a contiguous fp32 (R, T, H, W) tensor")
    R, T, H, W = masks.shape
    pt, ph, pw = (int(p) for p in patch)
    if pt < 1 or ph < 1 or pw < 1 or T % pt or H % ph or W % pw:
        raise ValueError(f"region_weights: ({T}, {H}, {W}) is not divisible by the patch {(pt, ph, pw)}")
    N = (T // pt) * (H // ph) * (W // pw)
    if perm is not None and (perm.dtype != torch.int32 or perm.numel() != N or not perm.is_contiguous() or perm.device != masks.device):
        raise ValueError("region_weights: perm must be a contiguous int32 tensor of N tokens on the masks' device")
    w = torch.empty(N, R + 1, dtype=torch.float32, device=masks.device)
    with torch.cuda.device(masks.device):
        check(lib().k5_region_weights_f32(ptr(masks), R, T, H, W, pt, ph, pw, float(base_weight), ptr(perm) if perm is not None else None, ptr(w),
                                          stream_ptr(masks.device)), "k5_region_weights_f32")
    return w


def x0_preview(img, v_cond, v_uncond, w, sigma_next, rgb_factors=None, rgb_bias=None, source=None, keep_mask=None, want_x0=False,
               out_rgb=None, out_x0=None):
    """(preview, x0) of the latent `img` (fp32 (..., C), C % 4 == 0 and <= 64) just after the update of a step that took it to sigma_next, with
    the step's velocities still in v_cond / v_uncond (k5_x0_preview): x0 = img - sigma_next * v, v combined as in cfg_euler_; under a
    keep_mask ((..., 1), with `source`) kept cells show the source.  preview: uint8 (..., 3) from rgb_factors [C][3] / rgb_bias [3] (fp32, moved
    to the device), None without factors; x0: fp32 like img, None unless want_x0.  out_rgb / out_x0: buffers to fill instead of new ones."""
    _need_cuda(img, v_cond, v_uncond, source, keep_mask, out_rgb, out_x0)
    C_ = img.shape[-1]
    cells = img.numel() // C_
    for t in (img, source):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape != img.shape):
            raise ValueError("x0_preview: img and source must be contiguous fp32 tensors of one shape")
    if keep_mask is not None and (source is None or keep_mask.dtype != torch.float32 or not keep_mask.is_contiguous() or keep_mask.numel() != cells):
        raise ValueError("x0_preview: keep_mask must be a contiguous fp32 tensor with one value per cell and needs source")
    for v in (v_cond, v_uncond):
        if v is not None and (v.dtype != torch.bfloat16 or not v.is_contiguous() or v.numel() != img.numel()):
            raise ValueError("x0_preview: the velocities must be contiguous bf16 tensors of img's size")
    wd = bd = None
    if rgb_factors is not None:
        wd = torch.as_tensor(rgb_factors, dtype=torch.float32).to(img.device).contiguous()
        if tuple(wd.shape) != (C_, 3):
            raise ValueError(f"x0_preview: rgb_factors must be [{C_}][3], got {tuple(wd.shape)}")
        if rgb_bias is not None:
            bd = torch.as_tensor(rgb_bias, dtype=torch.float32).to(img.device).contiguous()
            if bd.numel() != 3:
                raise ValueError("x0_preview: rgb_bias must hold 3 values")
        if out_rgb is None:
            out_rgb = torch.empty(tuple(img.shape[:-1]) + (3,), dtype=torch.uint8, device=img.device)
    else:
        out_rgb = None
    if want_x0 and out_x0 is None:
        out_x0 = torch.empty_like(img)
    if not want_x0:
        out_x0 = None
    if out_rgb is not None and (out_rgb.dtype != torch.uint8 or not out_rgb.is_contiguous() or out_rgb.numel() != cells * 3):
        raise ValueError("x0_preview: out_rgb must be a contiguous uint8 tensor of 3 values per cell")
    if out_x0 is not None and (out_x0.dtype != torch.float32 or not out_x0.is_contiguous() or out_x0.numel() != img.numel()):
        raise ValueError("x0_preview: out_x0 must be a contiguous fp32 tensor of img's size")
    with torch.cuda.device(img.device):
        check(lib().k5_x0_preview(ptr(img), ptr(v_cond), ptr(v_uncond), float(w), float(sigma_next), ptr(source if keep_mask is not None else None),
                                  ptr(keep_mask), ptr(wd), ptr(bd), ptr(out_x0), ptr(out_rgb), cells, C_, stream_ptr(img.device)),
              "k5_x0_preview")
    return out_rgb, out_x0
