"""CPU-only checks of `generate`'s per-step loop on a duck-typed model: the CFG-parallel exchange (one forward per step on this side, the
pair's velocities through `exchange_velocity`) against the plain two-forward run, and what a batch off the many-sample path hands to the
callback, the progress bar and the per-sample checks."""
import functools
import sys
import types

import pytest
import torch

import kit  # noqa: E402
from kit import flash_conf  # noqa: E402

import euler_step_reference as ER  # noqa: E402

CONF = flash_conf()
SHAPE, STEPS = (3, 4, 6, 16), 3


class FakeDit:
    """duck-typed model: a velocity that depends on the latent, the prompt and the time; every call is logged with all it was given"""
    visual_cond = False

    def __init__(self, cfg_parallel=None):
        self.calls = []
        if cfg_parallel is not None:
            self._cfg_parallel = cfg_parallel

    def __call__(self, x, text_embed, pooled, t, visual_rope_pos, text_rope_pos, scale_factor=None, sparse_params=None):
        self.calls.append((x.clone(), text_embed, pooled, t, visual_rope_pos, text_rope_pos))
        return (0.5 * x + text_embed.mean() + pooled.mean() * float(t.reshape(-1)[0]) / 1000).to(torch.bfloat16)


prompt = functools.partial(kit.host_prompt, dims=(8, 4))


@pytest.fixture()
def cpu_kernels(monkeypatch):
    from kandinsky import generation_utils as G
    monkeypatch.setattr(G.E, "euler_step_", ER.euler_step_)
    monkeypatch.setattr(G.E, "renoise", ER.renoise)
    return G


TE, NE = prompt(4, 1), prompt(2, 2)
POS = [torch.arange(3), torch.arange(2), torch.arange(3)]


def run(G, model, **kw):
    noise = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(5))
    return G.generate(model, "cpu", SHAPE, STEPS, TE, NE, POS, torch.arange(4), torch.arange(2), 5.0, 5.0, CONF, noise=noise, **kw)


def pair_exchange(monkeypatch, model, branch):
    """`exchange_velocity` of a pair whose other side is a second copy of the fake: it runs the other branch's forward on what this side's
    model was just given"""
    from kandinsky.models import parallelize
    other, (oe, op) = FakeDit(), ((NE, torch.arange(2)) if branch == 0 else (TE, torch.arange(4)))

    def exchange(v_mine, pair_group, out=None):
        assert pair_group is None and out is not None and out.shape == (2,) + tuple(v_mine.shape)
        x, _, _, t, vpos, _ = model.calls[-1]
        out[branch], out[1 - branch] = v_mine, other(x, oe["text_embeds"], oe["pooled_embed"], t, vpos, op)
        return out[0], out[1]

    monkeypatch.setattr(parallelize, "exchange_velocity", exchange)
    return other


def edit_kw():
    g = torch.Generator().manual_seed(9)
    return dict(init_latent=torch.randn(*SHAPE, generator=g), keep_mask=(torch.rand(*SHAPE[:-1], 1, generator=g) > 0.5).float())


# ------------------------------------------------------------------------------------------ the CFG-parallel exchange loop
@pytest.mark.parametrize("branch", [0, 1])
@pytest.mark.parametrize("edit", [False, True])
def test_cfg_parallel_loop_is_the_plain_run_with_one_forward_per_step(cpu_kernels, monkeypatch, branch, edit):
    G = cpu_kernels
    kw = edit_kw() if edit else {}
    plain = FakeDit()
    want = run(G, plain, **kw)
    assert len(plain.calls) == 2 * STEPS
    model = FakeDit(cfg_parallel=(branch, None))
    other = pair_exchange(monkeypatch, model, branch)
    got = run(G, model, **kw)
    assert torch.equal(got, want)
    assert len(model.calls) == STEPS == len(other.calls)                  # one forward per step on this side
    mine = TE if branch == 0 else NE
    assert all(c[1] is mine["text_embeds"] and len(c[5]) == mine["text_embeds"].shape[0] for c in model.calls)
    for i in range(STEPS):                                                # ... on the latent the plain run's two forwards saw
        assert torch.equal(model.calls[i][0], plain.calls[2 * i][0]) and torch.equal(model.calls[i][0], plain.calls[2 * i + 1][0])


@pytest.mark.parametrize("branch", [0, 1])
def test_cfg_parallel_loop_calls_back_and_cancels(cpu_kernels, monkeypatch, branch):
    G = cpu_kernels
    from kandinsky.models.dit import SamplingInterrupted
    model = FakeDit(cfg_parallel=(branch, None))
    pair_exchange(monkeypatch, model, branch)
    seen = []
    run(G, model, callback=lambda info: seen.append((info.step, info.num_steps)) and False)
    assert seen == [(i, STEPS) for i in range(STEPS)]
    model = FakeDit(cfg_parallel=(branch, None))
    pair_exchange(monkeypatch, model, branch)
    with pytest.raises(SamplingInterrupted) as e:
        run(G, model, callback=lambda info: info.step == 1)
    assert e.value.steps_done == 2 and len(model.calls) == 2


# ------------------------------------------------------------------------------------------ a batch off the many-sample path
def run_batch(G, model, **kw):
    noise = torch.randn(2 * SHAPE[0], *SHAPE[1:], generator=torch.Generator().manual_seed(6))
    return G.generate(model, "cpu", tuple(noise.shape), STEPS, TE, NE, POS, torch.arange(4), torch.arange(2), 5.0, 5.0, CONF, noise=noise,
                      batch=2, **kw)


def test_batch_callback_sees_every_sample_and_step_in_order(cpu_kernels):
    seen = []
    model = FakeDit()
    run_batch(cpu_kernels, model, callback=lambda info: seen.append((info.sample, info.step, info.num_steps, info.num_samples)) and False)
    assert seen == [(b, i, STEPS, 2) for b in range(2) for i in range(STEPS)]
    assert len(model.calls) == 2 * STEPS * 2


@pytest.mark.parametrize("strength,steps_run", [(1.0, STEPS), (0.4, 1)])
def test_progress_bar_of_a_batch_counts_batch_times_the_steps_that_run(cpu_kernels, monkeypatch, strength, steps_run):
    bars = []

    class Bar:
        def __init__(self, total):
            self.total, self.n, self.closed = total, 0, False
            bars.append(self)

        def update(self, k):
            self.n += k

        def close(self):
            self.closed = True

    fake = types.ModuleType("tqdm")
    fake.tqdm = Bar
    monkeypatch.setitem(sys.modules, "tqdm", fake)
    kw = {} if strength == 1.0 else dict(init_latent=torch.zeros(2 * SHAPE[0], *SHAPE[1:]), strength=strength)
    run_batch(cpu_kernels, FakeDit(), progress=True, **kw)
    assert len(bars) == 1                                                 # one bar for the whole batch, closed by the call that made it
    assert (bars[0].total, bars[0].n, bars[0].closed) == (2 * steps_run, 2 * steps_run, True)


def test_nag_on_a_model_without_the_engine_raises_before_any_model_call(cpu_kernels):
    model = FakeDit()
    kw = dict(nag_text_embeds=prompt(4, 3), nag_text_rope_pos=torch.arange(4), nag_scale=5.0)
    with pytest.raises(ValueError, match="nag_scale needs the engine-backed DiffusionTransformer3D"):
        run(cpu_kernels, model, **kw)
    with pytest.raises(ValueError, match="nag_scale needs the engine-backed DiffusionTransformer3D"):
        run_batch(cpu_kernels, model, **kw)
    assert model.calls == []
