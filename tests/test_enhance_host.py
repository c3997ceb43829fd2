"""Enhance-A-Video, the parts that need no GPU: the float64 rule's identities, the per-step mask (`enhance_plan`), the host surface
(`set_enhance`, `generate`, `generate_sample`, the CLI) with every refusal before a model runs, and the new entries of the C ABI, which
refuse bad arguments without a device."""
import ctypes as C
import functools
import os

import pytest
import torch

import kit  # noqa: E402
from kit import K5_ERR_ARG, K5_ERR_UNSUPPORTED, PKG, POS, built_lib, cfg, flash_conf  # noqa: E402

CONF = flash_conf()
SHAPE = (3, 8, 12, 16)

import enhance_reference as R  # noqa: E402
from kandinsky.generation_utils import edit_first_step, enhance_plan, sigma_schedule  # noqa: E402
from kandinsky.models.dit import check_enhance_args  # noqa: E402


def tiny(cfg):
    from kandinsky.models.dit import DiffusionTransformer3D
    return DiffusionTransformer3D(**cfg)


prompt = functools.partial(kit.host_prompt, dims=(96, 48))


call_generate = functools.partial(kit.call_generate, w=5.0, steps=4, shape=SHAPE, pos=POS, conf=CONF, prompt=prompt)


# ------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("T,weight", [(2, 0.0), (3, 4.0), (31, 4.0), (61, 2.5)])
def test_uniform_attention_scores_one_plus_weight_over_T(T, weight):
    S, Hh = 3, 2
    _, k = R.enhance_inputs(T, S, Hh)
    q = torch.zeros_like(k)
    assert R.enhance_mean(q, k, T, S, Hh, R.K5_SOFTMAX_C) == pytest.approx(1.0 / T, rel=1e-12)
    assert R.enhance_score(q, k, T, S, Hh, R.K5_SOFTMAX_C, weight) == pytest.approx(1.0 + weight / T, rel=1e-12)


@pytest.mark.parametrize("T", [2, 31, 64])
def test_self_attending_frames_clamp_at_exactly_one(T):
    q, k = R.onehot_inputs(T, 3, 2)
    assert R.enhance_mean(q, k, T, 3, 2, R.K5_SOFTMAX_C) < 1e-80
    assert R.enhance_score(q, k, T, 3, 2, R.K5_SOFTMAX_C, 4.0) == 1.0


def test_the_table_and_the_key_scale_are_honoured():
    T, S, Hh = 5, 4, 2
    q, k = R.enhance_inputs(T, S, Hh)
    plain = R.enhance_mean(q, k, T, S, Hh, R.K5_SOFTMAX_C)
    for fused in (True, False):
        L = R.lay_out(q, k, T, S, Hh, fused, True, False, fill=float("nan"))
        b = L["back"]
        Q, K = (b[0][:, :L["D"]], b[0][:, L["D"]:]) if fused else b
        assert R.enhance_mean(Q, K, T, S, Hh, L["qk_scale"], L["frame_rows"]) == pytest.approx(plain, rel=1e-12)
    pre = R.lay_out(q, k, T, S, Hh, True, False, True)
    assert pre["qk_scale"] == 1.0 and R.enhance_mean(pre["q"], pre["k"], T, S, Hh, 1.0) == pytest.approx(plain, rel=2e-3)   # bf16 rounding of k * c
    for variant in ("transposed", "shuffled", "flipped"):
        assert abs(R.enhance_mean(q, k, T, S, Hh, R.K5_SOFTMAX_C, variant=variant) - plain) / plain > 1e-4


# ------------------------------------------------------------------------------------------ arguments and the plan
def test_check_enhance_args():
    assert check_enhance_args(4, None) == (4.0, None)
    assert check_enhance_args(0.0, [1, 0, 2]) == (0.0, [1, 0, 1])           # 0.0 is a valid weight
    for bad in (-1.0, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="weight"):
            check_enhance_args(bad, None)
    with pytest.raises(ValueError, match="steps"):
        check_enhance_args(4.0, [])


def test_plan_masks():
    sig = sigma_schedule(6, 5.0).tolist()            # 1, .962, .909, .833, .714, .5, 0
    assert enhance_plan(sig) == [1] * 6 == enhance_plan(sig, None)
    assert enhance_plan(sig, (0.6, 0.97)) == [0, 1, 1, 1, 1, 0]
    assert enhance_plan(sig, (sig[2], sig[2])) == [0, 0, 1, 0, 0, 0]        # both ends belong to the interval
    assert enhance_plan(sig, (2.0, 3.0)) == [0] * 6
    for bad in ((0.9, 0.1), (0.5,), "ab", 3):
        with pytest.raises(ValueError, match="enhance_interval"):
            enhance_plan(sig, bad)
    with pytest.raises(ValueError, match="num_steps"):
        enhance_plan([1.0])


def test_generate_sets_it_for_the_call_cuts_it_with_the_schedule_and_clears_it(cfg):
    m = tiny(cfg)
    seen = []

    def sample(img, *a, **k):
        seen.append(m._enhance)
        if len(seen) == 3:
            raise RuntimeError("boom")

    m.sample = sample
    call_generate(m, steps=6, enhance_weight=4.0, enhance_interval=(0.6, 0.97))
    assert seen[0] == (4.0, [0, 1, 1, 1, 1, 0]) and m._enhance is None
    first = edit_first_step(6, 0.5)
    call_generate(m, steps=6, enhance_weight=0.0, enhance_interval=(0.6, 0.97), init_latent=torch.zeros(SHAPE), strength=0.5)
    assert first == 3 and seen[1] == (0.0, [1, 1, 0])                       # the steps 3, 4, 5 of the full plan
    m.set_enhance(2.0)
    with pytest.raises(RuntimeError, match="boom"):
        call_generate(m, enhance_weight=4.0)
    assert seen[2] == (4.0, [1, 1, 1, 1]) and m._enhance == (2.0, None)     # what was there before comes back, also on an exception
    m.clear_enhance()
    assert m._enhance is None and m.enhance_state() == (False, 0, [])


def test_generate_with_the_defaults_passes_nothing_to_the_model(cfg):
    m = tiny(cfg)
    seen = []
    m.sample = lambda img, *a, **k: seen.append(m._enhance)
    m.set_enhance = m.clear_enhance = lambda *a, **k: pytest.fail("the defaults must not touch the model")
    call_generate(m)
    call_generate(m, enhance_weight=None, enhance_interval=None)
    call_generate(m, enhance_weight=4.0, enhance_interval=(2.0, 3.0))      # an interval without a step: off
    assert seen == [None] * 3


def test_generate_refusals(cfg):
    from kandinsky import generation_utils as G
    m = tiny(cfg)
    m.sample = lambda *a, **k: pytest.fail("refused calls must not sample")
    for kw, word in ((dict(enhance_weight=-1.0), "weight"), (dict(enhance_weight=float("nan")), "weight"), (dict(enhance_weight="much"), "weight"),
                     (dict(enhance_interval=(0.2, 0.9)), "needs enhance_weight"), (dict(enhance_weight=4.0, enhance_interval=(0.9, 0.1)), "enhance_interval")):
        with pytest.raises(ValueError, match=word):
            call_generate(m, **kw)
        with pytest.raises(ValueError, match=word):
            G.generate_sample((1, 3, 8, 12, 16), "a", m, None, CONF, None, **kw)
    long = (65, 4, 4, 16)
    with pytest.raises(ValueError, match="65 latent frames"):
        call_generate(m, shape=long, pos=[torch.arange(65), torch.arange(2), torch.arange(2)], enhance_weight=4.0)
    with pytest.raises(ValueError, match="65 latent frames"):
        G.generate_sample((1,) + long, "a", m, None, CONF, None, enhance_weight=4.0)
    m._sp = (0, 2)                                                         # a rank of a sequence-parallel group
    with pytest.raises(ValueError, match="sequence-parallel"):
        call_generate(m, enhance_weight=4.0)
    m._sp = None

    class Bare(torch.nn.Module):                                           # a wrapped callable that cannot take the setting
        visual_cond = True

        def forward(self, *a, **k):
            pytest.fail("refused calls must not run the model")
    with pytest.raises(ValueError, match="set_enhance"):
        call_generate(Bare(), enhance_weight=4.0)
    assert m._enhance is None


def test_setting_for_call_restores_or_clears(cfg):
    m = tiny(cfg)
    with m.setting_for_call("enhance", (4.0, [1, 0])):
        assert m._enhance == (4.0, [1, 0])
    assert m._enhance is None
    m.set_enhance(1.5)
    kept = m._enhance
    with pytest.raises(RuntimeError):
        with m.setting_for_call("enhance", (4.0, None)):
            assert m._enhance == (4.0, None)
            raise RuntimeError("x")
    assert m._enhance is kept
    with m.setting_for_call("enhance", None):
        assert m._enhance is kept
    with pytest.raises(ValueError, match="weight"):
        with m.setting_for_call("enhance", (-4.0, None)):
            pytest.fail("a refused setting must not run the body")
    assert m._enhance is kept


def test_cli_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_cli_enhance", os.path.join(PKG, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    none = p.parse_args([])
    assert not hasattr(none, "enhance_weight") and not hasattr(none, "enhance_interval") and cli.enhance_keywords(none) == {}
    a = p.parse_args(["--enhance_weight", "4", "--enhance_interval", "0.2", "0.99"])
    assert cli.enhance_keywords(a) == dict(enhance_weight=4.0, enhance_interval=(0.2, 0.99))
    assert cli.enhance_keywords(p.parse_args(["--enhance_weight", "0"])) == dict(enhance_weight=0.0)
    for argv, word in ((["--enhance_interval", "0.2", "0.9"], "needs --enhance_weight"), (["--enhance_weight", "-1"], "enhance_weight"),
                       (["--enhance_weight", "inf"], "enhance_weight"), (["--enhance_weight", "nan"], "enhance_weight"),
                       (["--enhance_weight", "4", "--enhance_interval", "0.9", "0.2"], "LO <= HI")):
        with pytest.raises(ValueError, match=word):
            cli.enhance_keywords(p.parse_args(argv))
    for argv in (["--enhance_interval", "0.5"], ["--enhance_weight", "much"], ["--enhance_weight"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)


# ------------------------------------------------------------------------------------------ ABI
def test_kernel_entries_refuse_without_gpu(built_lib):
    """every documented refusal of the two kernel entries returns before any HIP call: the pointers are host memory, a refusal never reads
    them, and nothing here may launch"""
    from kandinsky import _engine as E
    L = E.lib()
    bufs = [C.create_string_buffer(4096 + 16) for _ in range(4)]
    q, k, part, score = ((C.addressof(b) + 15) & ~15 for b in bufs)
    good = [q, k, 128, 128, 2, 3, 4, None, 1.0, 4.0, part, score, None]
    bad = [(0, None), (1, None), (0, q + 8), (1, k + 2), (2, 120), (3, 127), (2, 132), (3, 260), (4, 0), (4, -1), (6, 0), (5, 1), (5, 0), (5, -3),
           (9, -1.0), (9, float("inf")), (9, float("nan")), (8, 0.0), (8, -1.0), (8, float("nan")), (10, None), (11, None)]
    for i, v in bad:
        a = list(good)
        a[i] = v
        assert L.k5_enhance_scores_bf16(*a) == K5_ERR_ARG, (i, v)
        assert "k5_enhance_scores_bf16" in E.last_error()
    for T in (65, 1000):
        a = list(good)
        a[5] = T
        assert L.k5_enhance_scores_bf16(*a) == K5_ERR_UNSUPPORTED and "64" in E.last_error()
    assert L.k5_enhance_part_count(28, 1536) == 28 * 1536 and L.k5_enhance_part_count(0, 4) == 0 and L.k5_enhance_part_count(4, -1) == 0
    good = [q, 8, 128, 128, score, None]
    for i, v in ((0, None), (0, q + 8), (1, 0), (1, -2), (2, 0), (2, 124), (3, 120), (3, 132), (4, None)):
        a = list(good)
        a[i] = v
        assert L.k5_scale_by_dev_bf16(*a) == K5_ERR_ARG, (i, v)
        assert "k5_scale_by_dev_bf16" in E.last_error()


def test_handle_entries_refuse_without_gpu(built_lib, cfg):
    from kandinsky import _engine as E
    L = E.lib()
    assert L.k5_dit_set_enhance(None, None) == K5_ERR_ARG and L.k5_dit_enhance_state(None, None, None, None, 0, None, 0) == K5_ERR_ARG
    cc = E.DitConfig(16, 96, 48, 64, 16, (C.c_int * 3)(1, 2, 2), 128, 256, 1, 2, (C.c_int * 3)(16, 24, 24), 1)
    h = C.c_void_p()
    assert L.k5_dit_create(C.byref(cc), C.byref(h)) == 0
    steps = (C.c_ubyte * 3)(1, 0, 1)
    sp = C.cast(steps, C.POINTER(C.c_ubyte))
    for e, word in ((E.Enhance(-1.0, None, 0), "weight"), (E.Enhance(float("nan"), None, 0), "weight"), (E.Enhance(float("inf"), None, 0), "weight"),
                    (E.Enhance(4.0, sp, 0), "num_steps")):
        assert L.k5_dit_set_enhance(h, C.byref(e)) == K5_ERR_ARG and word in E.last_error()
    on, n, nb = C.c_int(7), C.c_longlong(7), C.c_int(7)
    assert L.k5_dit_enhance_state(h, C.byref(on), C.byref(n), None, 0, C.byref(nb), 0) == 0 and (on.value, n.value, nb.value) == (0, 0, 0)
    assert L.k5_dit_set_enhance(h, C.byref(E.Enhance(0.0, sp, 3))) == 0     # weight 0 is a weight, not "off"
    assert L.k5_dit_enhance_state(h, C.byref(on), None, None, 0, None, 0) == 0 and on.value == 1
    assert L.k5_dit_set_enhance(h, None) == 0
    assert L.k5_dit_enhance_state(h, C.byref(on), None, None, 0, None, 1) == 0 and on.value == 0
    L.k5_dit_destroy(h)
