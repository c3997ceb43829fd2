"""`generate`'s per-step loop and its one update call, without a GPU.

Characterisation: a fake model with `forward_skip` runs through the per-step path with a guidance interval, CFG-Zero*, skip-layer guidance with an
interval, stochastic steps with an interval and either `cfg_zero_init` or an edit with a fractional keep mask (`generate` refuses those two
together, so they are two cases), and a recorder in place of `E.euler_step_` sees exactly the steps that `guidance_plan`, `skip_plan`,
`stochastic_plan` and `sigma_schedule` describe.  A further case without noise has previews, which decide `v_out`.

The stand-in: with tests/euler_step_reference.py in place of the kernels the same loop reproduces the bf16 loops of guidance_reference,
skip_reference and stochastic_reference bit for bit.

The wrapper and the entry: `E.euler_step_` raises before any library call, `k5_euler_step` refuses before any launch, and the header's struct
and the binding's agree field for field."""
import ctypes as C
import functools

import pytest
import torch


import euler_step_reference as ER  # noqa: E402
import guidance_reference as R  # noqa: E402
import skip_reference as S  # noqa: E402
import stochastic_reference as SR  # noqa: E402
from kandinsky import generation_utils as G  # noqa: E402
import kit  # noqa: E402
from kit import BF, assert_abi_entries, built_lib, flash_conf  # noqa: E402

CONF = flash_conf()
SHAPE, STEPS, SCALE = (3, 4, 6, 16), 6, 5.0
POS = [torch.arange(3), torch.arange(2), torch.arange(3)]


prompt = functools.partial(kit.host_prompt, dims=(8, 4))


TE, NE = prompt(4, 1), prompt(2, 2)


class FakeDit:
    """duck-typed model with a skip branch: velocities that depend on the latent, the prompt and the time; every forward is logged by kind"""
    visual_cond = False
    num_visual_blocks = 4

    def __init__(self):
        self.calls = []

    @staticmethod
    def velocity(x, te, pooled, t, skip=False):
        return ((0.25 if skip else 0.5) * x + te.mean() + pooled.mean() * float(t.reshape(-1)[0]) / 1000).to(BF)

    def __call__(self, x, te, pooled, t, visual_rope_pos, text_rope_pos, scale_factor=None, sparse_params=None):
        self.calls.append("cond" if te is TE["text_embeds"] else "uncond")
        return self.velocity(x, te, pooled, t)

    def forward_skip(self, x, te, pooled, t, visual_rope_pos, text_rope_pos, scale_factor=None, sparse_params=None):
        self.calls.append("cond+skip")
        return self.velocity(x, te, pooled, t), self.velocity(x, te, pooled, t, skip=True)


class Recorder:
    """`E.euler_step_`: notes how the step was described, then applies the stand-in's update"""

    def __init__(self):
        self.steps = []

    def __call__(self, img, v_cond, v_uncond=None, *, w=1.0, dt, ab=None, v_skip=None, g=0.0, source=None, noise=None, keep_mask=None, sigma_next=0.0,
                 v_out=None, stochastic=None):
        assert stochastic is None or (len(stochastic) == 4 or stochastic[4] is None)   # the loop draws in the kernel
        self.steps.append(dict(uncond=v_uncond is not None, skip=v_skip is not None, w=w, dt=dt, ab=ab is not None, g=g, sigma_next=sigma_next,
                               keep=(source is not None, noise is not None, keep_mask is not None),
                               stochastic=None if stochastic is None else tuple(stochastic[:4]),
                               v_out=None if v_out is None else ("v_cond" if v_out is v_cond else "other")))
        return ER.euler_step_(img, v_cond, v_uncond, w=w, dt=dt, ab=ab, v_skip=v_skip, g=g, source=source, noise=noise, keep_mask=keep_mask,
                              sigma_next=sigma_next, v_out=v_out, stochastic=stochastic)


@pytest.fixture()
def stand_ins(monkeypatch):
    monkeypatch.setattr(G.E, "euler_step_", ER.euler_step_)
    monkeypatch.setattr(G.E, "guidance_coeffs", ER.guidance_coeffs)
    monkeypatch.setattr(G.E, "renoise", ER.renoise)
    return monkeypatch


# ------------------------------------------------------------------------------------------ characterisation of the step loop
W, G_INTERVAL, SLG_SCALE, SLG_INTERVAL, SDE_INTERVAL, SEED = 4.0, (0.6, 0.95), 2.5, (0.8, 0.97), (0.75, 1.0), 77
ON = dict(guidance_interval=G_INTERVAL, cfg_zero_star=True, slg_blocks=[1, 2], slg_scale=SLG_SCALE, slg_interval=SLG_INTERVAL)
NOISY = dict(eta=1.0, sde_interval=SDE_INTERVAL, sde_seed=SEED)


def edit_kw(batch=1):
    g = torch.Generator().manual_seed(9)
    shape = (batch * SHAPE[0],) + SHAPE[1:]
    mask = torch.rand(*shape[:-1], 1, generator=g)
    mask[0, 0, 0], mask[0, 0, 1], mask[0, 0, 2] = 0.0, 1.0, 0.25
    return dict(init_latent=torch.randn(*shape, generator=g), keep_mask=mask)


def described(zero_init=0, noisy=True, edit=False, sample=0, preview_every=0):
    """(steps, forwards) of one sample from the plans, which the loop under test does not compute"""
    sig32 = G.sigma_schedule(STEPS, SCALE)
    sig = sig32.tolist()
    weights, mask = G.guidance_plan(sig, W, None, G_INTERVAL), G.skip_plan(sig, SLG_INTERVAL)
    dt_down, scale, coef = G.stochastic_plan(sig, 1.0, 1.0, SDE_INTERVAL) if noisy else (torch.diff(sig32).tolist(), None, None)
    steps, forwards = [], []
    for i in range(STEPS):
        if i < zero_init:
            continue
        guided, skip = R.is_guided(weights[i]), bool(mask[i])
        forwards += ["cond+skip" if skip else "cond"] + ["uncond"] * guided
        preview = preview_every > 0 and ((i + 1) % preview_every == 0 or i == STEPS - 1)
        steps.append(dict(uncond=guided, skip=skip, w=weights[i], dt=dt_down[i], ab=guided, g=SLG_SCALE if skip else 0.0, sigma_next=sig[i + 1],
                          keep=(edit,) * 3, stochastic=(scale[i], coef[i], SEED + sample, i) if noisy else None,
                          v_out="v_cond" if preview and (guided or skip) else None))
    return steps, forwards


def test_the_plans_of_the_characterisation_mix_every_kind_of_step():
    steps, _ = described(zero_init=1)
    assert [(s["uncond"], s["skip"], s["stochastic"][1] != 0.0) for s in steps] == [
        (False, True, True), (True, True, True), (True, True, True), (True, False, False), (False, False, False)]


def run(model, batch=1, **kw):
    shape = (batch * SHAPE[0],) + SHAPE[1:]
    noise = torch.randn(*shape, generator=torch.Generator().manual_seed(5))
    return G.generate(model, "cpu", shape, STEPS, TE, NE, POS, torch.arange(4), torch.arange(2), W, SCALE, CONF, noise=noise, batch=batch, **kw)


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("case", ["zero_init", "edit"])
def test_the_step_loop_describes_every_step_as_the_plans_do(stand_ins, case, batch):
    rec, model = Recorder(), FakeDit()
    stand_ins.setattr(G.E, "euler_step_", rec)
    kw = dict(cfg_zero_init=1) if case == "zero_init" else edit_kw(batch)
    run(model, batch, **ON, **NOISY, **kw)
    want = [described(zero_init=int(case == "zero_init"), edit=case == "edit", sample=b) for b in range(batch)]
    assert rec.steps == [s for steps, _ in want for s in steps]
    assert model.calls == [f for _, forwards in want for f in forwards]


def test_the_step_loop_hands_the_velocity_of_a_preview_step_back_in_v_cond(stand_ins):
    rec, model, previews = Recorder(), FakeDit(), []

    def x0_preview(img, v, u, w, sigma_next, W_, b, source=None, keep_mask=None, want_x0=False):
        previews.append((v.dtype, u is not None, source is not None, keep_mask is not None))
        return torch.zeros(tuple(img.shape[:-1]) + (3,), dtype=torch.uint8), None

    stand_ins.setattr(G.E, "euler_step_", rec)
    stand_ins.setattr(G.E, "x0_preview", x0_preview)
    seen = []
    run(model, **ON, **edit_kw(), callback=lambda info: seen.append((info.step, info.preview is not None)) and False, preview_every=2,
        preview_factors=torch.zeros(16, 3))
    steps, forwards = described(noisy=False, edit=True, preview_every=2)
    assert rec.steps == steps and model.calls == forwards
    assert seen == [(i, i % 2 == 1) for i in range(STEPS)]
    # steps 1, 3, 5 carry a preview: 1 and 3 left their velocity in v_cond (no second velocity to combine), 5 is a plain unguided step
    assert previews == [(BF, False, True, True)] * 3


# ------------------------------------------------------------------------------------------ the stand-in against the references
def velocities(model):
    def of(prompt_, skip=False):
        return lambda x, s: model.velocity(x, prompt_["text_embeds"], prompt_["pooled_embed"], torch.tensor([s]) * 1000, skip).float()
    return of(TE), of(NE), of(TE, skip=True)


@pytest.mark.parametrize("case", ["guidance", "skip", "stochastic"])
def test_the_step_loop_on_the_stand_in_is_the_reference_bf16_loop(stand_ins, case):
    sig = G.sigma_schedule(STEPS, SCALE).tolist()
    noise = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(5))
    weights, mask = G.guidance_plan(sig, W, None, G_INTERVAL), G.skip_plan(sig, SLG_INTERVAL)
    cond, uncond, skip = velocities(FakeDit)
    guide = dict(zero_star=True, zero_init=1)
    if case == "guidance":
        kw = dict(guidance_interval=G_INTERVAL, cfg_zero_star=True, cfg_zero_init=1)
        want = R.bf16_loop(cond, uncond, noise, sig, weights, **guide)
    elif case == "skip":
        kw = dict(ON, cfg_zero_init=1)
        want = S.bf16_loop(cond, uncond, skip, noise, sig, weights, SLG_SCALE, mask, **guide)
    else:
        kw = dict(ON, **NOISY, cfg_zero_init=1)
        want = SR.bf16_loop(cond, uncond, skip, noise, sig, weights, SR.tables_f32(sig, 1.0, 1.0, SDE_INTERVAL), SR.step_noise(SHAPE, SEED),
                            g=SLG_SCALE, mask=mask, **guide)
    got = run(FakeDit(), **kw)
    assert torch.equal(got, want) and not torch.equal(got, noise)


# ------------------------------------------------------------------------------------------ header, binding, entry and wrapper
def test_header_and_binding_agree_on_the_step_struct(built_lib):
    from kandinsky import _engine as E
    assert_abi_entries(built_lib, ("k5_euler_step",), [("k5_euler_step_args", E.EulerStep)])


def test_the_entry_refuses_bad_arguments_without_a_gpu(built_lib):
    from kandinsky import _engine as E
    L = E.lib()
    host = (C.c_float * 64)()                    # host memory as the pointers: nothing is launched, nothing is read
    p = C.cast(host, C.c_void_p).value
    nan, inf = float("nan"), float("inf")

    def args(**kw):
        a = E.EulerStep(img=p, v_cond=p, w=1.0, dt=-0.1, cells=4, C=2, scale=1.0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.k5_euler_step(None, None) == 1 and "k5_euler_step" in E.last_error()
    bad = [dict(img=None), dict(v_cond=None), dict(cells=0), dict(C=0), dict(ab=p), dict(v_out=p), dict(keep_mask=p),
           dict(keep_mask=p, source=p), dict(keep_mask=p, noise=p), dict(skip_scale=3.0), dict(znoise=p)]
    bad += [dict(v_skip=p, skip_scale=g) for g in (0.0, -1.0, nan, inf)]
    bad += [dict(stochastic=1, scale=s) for s in (nan, inf)] + [dict(stochastic=1, noise_coef=c) for c in (-0.5, nan, inf)]
    words = set()
    for kw in bad:
        assert L.k5_euler_step(C.byref(args(**kw)), None) == 1, kw
        assert E.last_error().startswith("k5_euler_step: "), (kw, E.last_error())
        words.add(E.last_error().split(" (cells")[0])
    assert len(words) == 11 and not any("launcher" in w for w in words)      # each condition is named


def test_the_wrapper_refuses_before_any_library_call():
    from kandinsky import _engine as E
    img, v = torch.zeros(4, 2), torch.zeros(4, 2, dtype=BF)
    mask = torch.zeros(4, 1)
    for kw in (dict(v_cond=v.float()), dict(v_skip=v.float(), g=1.0), dict(img=torch.zeros(2, 4).t()), dict(keep_mask=torch.zeros(3, 1), source=img, noise=img),
               dict(keep_mask=mask, noise=img), dict(keep_mask=mask, source=img), dict(ab=torch.zeros(3), v_uncond=v),
               dict(v_uncond=torch.zeros(4, 2, dtype=BF, device="meta")), dict(stochastic=(1.0, 0.5, 1, 0, torch.zeros(7)))):
        a = dict(dict(img=img, v_cond=v, dt=-0.1), **kw)
        with pytest.raises(ValueError, match="euler_step_"):
            E.euler_step_(a.pop("img"), a.pop("v_cond"), **a)
    with pytest.raises(RuntimeError, match="GPU only"):
        E.euler_step_(img, v, dt=-0.1)
