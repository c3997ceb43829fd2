"""The refusal contract of the engine's forward (csrc/engine.hip forward_refusals): a forward that is refused on its arguments or
on the handle's settings returns its status and message with nothing enqueued and nothing changed on the handle.  One forward per case on the
tiny golden model, through ctypes (the Python wrapper checks some of these itself): the status and the message word for word, with profiling on
no launch of any kernel family, and a valid forward right after it gives the bits of the same forward made before it.

The MagCache case is the one refusal that depends on the handle's run state: a skip decided for a call whose slot holds no residual of the
call's shape.  The decision reads the ratio table, the call counter and the accumulators only, so it is made in front of the first launch."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kit import GOLDEN, K5_ERR_ARG, K5_ERR_STATE, K5_ERR_UNSUPPORTED  # noqa: E402

FAMILIES = ("elementwise", "gemm", "attn_self", "attn_cross", "nabla_map", "prologue", "epilogue", "comm", "attn_text")
SF = (1.0, 2.0, 2.0)
SHAPE, OTHER = (3, 8, 12), (2, 8, 12)       # the golden forward's latent (72 tokens) and another one (48 tokens)


@pytest.fixture(scope="module")
def dit(golden_meta, tiny_sd):
    from kandinsky.models.dit import DiffusionTransformer3D
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    d = DiffusionTransformer3D(**golden_meta["tiny_config"])
    d.load_state_dict(tiny_sd, assign=True)
    d = d.to("cuda:0")
    d.engine("cuda:0")
    return d


def positions(shape):
    return [torch.arange(shape[0]), torch.arange(shape[1] // 2), torch.arange(shape[2] // 2)]


def valid_forward(dit, golden):
    """the golden forward, from an empty softmax-form memory: the same call gives the same bits"""
    dit.reset_softmax_memory()
    out = dit(golden["fwd.x"].cuda(), golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), golden["fwd.time"], positions(SHAPE), torch.arange(7),
              scale_factor=SF)
    torch.cuda.synchronize()
    return out.clone()


def refused_forward(dit, golden, shape, entry="k5_dit_forward", sparse=None, **fields):
    """(status, message, {family: launches}) of one `entry` call at latent `shape` with the k5_forward_args fields `fields` overwritten"""
    from kandinsky import _engine as E
    L = E.lib()
    x = torch.zeros(*shape, golden["fwd.x"].shape[-1], device="cuda:0")
    a, out, keep = dit._forward_prologue("forward", x, (2,) if entry == "k5_dit_forward_skip" else (), golden["fwd.text"], golden["fwd.pooled"],
                                         golden["fwd.time"], positions(shape), torch.arange(7), SF, sparse)
    for name, value in fields.items():
        setattr(a, name, value)
    outs = (out[0].data_ptr(), out[1].data_ptr()) if entry == "k5_dit_forward_skip" else (out.data_ptr(),)
    dit.set_profiling(True)
    try:
        dit.reset_profile()
        with torch.cuda.device(x.device):
            status = getattr(L, entry)(dit._handle, C.byref(a), *outs, E.stream_ptr(x.device))
        message = (L.k5_last_error() or b"").decode()
        torch.cuda.synchronize()
        return status, message, {f: dit.get_profile(f)[1] for f in FAMILIES}
    finally:
        dit.set_profiling(False)


def set_magcache(dit, table, thresh=0.12, K=2, retention=0.2):
    from kandinsky import _engine as E
    t = np.ascontiguousarray(table, dtype=np.float64)
    E.check(E.lib().k5_dit_set_magcache(dit._handle, t.ctypes.data_as(C.POINTER(C.c_double)) if len(t) else None, len(t), 0, thresh, K, retention),
            "set_magcache")


def region_set():
    from safetensors.torch import load_file
    rg = load_file(os.path.join(GOLDEN, "dit_tiny_regions.safetensors"))
    assert tuple(rg["regions.B.masks"].shape[1:]) == SHAPE
    return ([{"text_embeds": rg["regions.text0"].cuda()}, {"text_embeds": rg["regions.text1"].cuda()}], [torch.arange(5), torch.arange(6)],
            rg["regions.B.masks"].contiguous(), 0.5)


def nabla_params():
    at = json.load(open(os.path.join(GOLDEN, "dit_tiny_meta.json")))["nabla_attention"]
    return {"P": at["P"], "wT": at["wT"], "wH": at["wH"], "wW": at["wW"], "to_fractal": True}


# case -> (what is set on the model, what is taken back, the refused call, its status, its message)
CASES = {
    "attention_type": (None, None, dict(shape=SHAPE, attention_type=2), K5_ERR_ARG, "attention_type must be 0 (flash) or 1 (nabla)"),
    "odd_H": (None, None, dict(shape=(3, 7, 12)), K5_ERR_ARG, "bad shapes"),
    "x_channels": (None, None, dict(shape=SHAPE, x_channels=5), K5_ERR_ARG, "x_channels must be 33 or 16"),
    "nabla_not_16": (None, None, dict(shape=SHAPE, sparse=True), K5_ERR_ARG, "nabla attention needs latent H, W divisible by 16 (got 8 x 12)"),
    "region_masks_shape": (lambda d: d.set_regions(*region_set()), lambda d: d.clear_regions(), dict(shape=OTHER), K5_ERR_ARG,
                           "regional prompts: the masks are (3, 8, 12), this forward is (2, 8, 12)"),
    "enhance_65_frames": (lambda d: d.set_enhance(4.0), lambda d: d.clear_enhance(), dict(shape=(65, 2, 2)), K5_ERR_UNSUPPORTED,
                          "Enhance-A-Video is set (k5_dit_set_enhance): 65 frames are more than a wave's four 32 x 32 accumulators hold (64)"),
    "forward_skip_no_set": (None, None, dict(shape=SHAPE, entry="k5_dit_forward_skip"), K5_ERR_STATE,
                            "k5_dit_forward_skip: no skip set on the handle (k5_dit_set_skip_guidance)"),
    "forward_skip_magcache": (lambda d: (d.set_skip_guidance([1], 3.0), set_magcache(d, [1.0] * 20)),
                              lambda d: (set_magcache(d, []), d.clear_skip_guidance()), dict(shape=SHAPE, entry="k5_dit_forward_skip"), K5_ERR_STATE,
                              "k5_dit_forward_skip: MagCache is set on the handle: the ratio table is indexed by the calls of a plain run"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_refused_forward_enqueues_nothing_and_changes_nothing(dit, golden, case):
    setup, teardown, call, status, message = CASES[case]
    call = dict(call)
    if call.pop("sparse", False):
        call["sparse"] = nabla_params()
    if setup:
        setup(dit)
    try:
        before = valid_forward(dit, golden)
        got = refused_forward(dit, golden, **call)
        print(case, got)
        assert got[:2] == (status, message)
        assert got[2] == dict.fromkeys(FAMILIES, 0)
        assert torch.equal(valid_forward(dit, golden), before)
    finally:
        if teardown:
            teardown(dit)


def test_calibration_shape_mismatch_enqueues_nothing_and_changes_nothing(dit, golden):
    """two calls of a calibration run at the golden shape, the third — its slot's second — at another: refused, and the run goes on as if it
    had not been made"""
    from kandinsky.magcache_utils import magcache_calibration_sums, start_magcache_calibration, stop_magcache_calibration
    start_magcache_calibration(dit, 4, False)
    try:
        before = valid_forward(dit, golden)
        valid_forward(dit, golden)
        sums = magcache_calibration_sums(dit)[0].copy()
        got = refused_forward(dit, golden, OTHER)
        print(got)
        assert got[:2] == (K5_ERR_ARG, "MagCache calibration: this forward has 48 x 128 residual elements, the previous call of its slot had 9216")
        assert got[2] == dict.fromkeys(FAMILIES, 0)
        assert np.array_equal(magcache_calibration_sums(dit)[0], sums)
        assert torch.equal(valid_forward(dit, golden), before)      # call 2 of the run, now at its slot's shape
        assert magcache_calibration_sums(dit)[0][2, 3] == 72        # ... and it counted its rows against call 0's residual
    finally:
        stop_magcache_calibration(dit)


def test_magcache_skip_without_a_residual_of_the_shape_is_refused_before_the_first_launch(dit, golden):
    """a table of ones under a large threshold: the first eligible call (call 2 of 8 at retention 0.25) decides to skip.  Calls 0 and 1 ran at
    the golden shape, call 2 comes at another: its slot's residual is not of its shape, and the forward is refused with nothing enqueued"""
    from kandinsky.magcache_utils import magcache_state
    set_magcache(dit, [1.0] * 8, thresh=1e9, K=2, retention=0.25)
    try:
        valid_forward(dit, golden)
        valid_forward(dit, golden)
        assert magcache_state(dit) == (2, 2, 0)
        got = refused_forward(dit, golden, OTHER)
        print(got)
        assert got[:2] == (K5_ERR_ARG, "magcache: skip decided but no cached residual of this shape for the slot")
        assert got[2] == dict.fromkeys(FAMILIES, 0)
        assert magcache_state(dit) == (2, 2, 0)                     # the call did not count
    finally:
        set_magcache(dit, [])
