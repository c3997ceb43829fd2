"""The forecast cache on the MI355X: the two passes (k5_forecast_update_bf16 / k5_forecast_apply_bf16) bit for bit against their torch
restatement (tests/forecast_reference.py) over shapes, strides, orders and history lengths with poisoned guard bands; k5_sample* with a plan
through the modes of the fused sampler (the plain run's bits where the plan is off, MagCache's bits at order 0 under MagCache's own mask,
the per-step loop's bits everywhere); parity with the bf16 oracle and the reference's golden; rank groups; every refusal.

The model is the tiny config with four visual blocks on synthetic weights (tests/skip_reference.py), latent (3, 8, 12, 16), 8 or 9 steps:
plan (9, interval 3, warmup 2, tail 1) has forecasts with k = 1 and 2 and an update with g = 3, plan (8, 2, 3, 1) alternates."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402

import forecast_reference as FR  # noqa: E402
import skip_reference as S  # noqa: E402
import kit  # noqa: E402
from kit import BF, GOLDEN, K5_ERR_ARG, K5_ERR_STATE, POS, edit_mask, make_dit, prompts, rel, source_latent  # noqa: E402
from test_gpu_skip import BIG, FLASH, SHAPE, Recorder, run_generate  # noqa: E402

PLANS = {9: dict(forecast_interval=3, forecast_warmup=2, forecast_tail=1), 8: dict(forecast_interval=2, forecast_warmup=3, forecast_tail=1)}
FULL = {9: [1, 1, 1, 0, 0, 1, 0, 0, 1], 8: [1, 1, 1, 1, 0, 1, 0, 1]}


@pytest.fixture(scope="module")
def cfg(golden_meta):
    return S.tiny4_config(golden_meta["tiny_config"])


@pytest.fixture(scope="module")
def sd4(cfg):
    return S.tiny4_weights(cfg)


@pytest.fixture(scope="module")
def dit(cfg, sd4):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    d = make_dit(cfg, sd4)
    d.engine("cuda:0")
    return d


# ------------------------------------------------------------------------------------------ kernels
def guarded(t, poison, ld=None):
    """(buffer, view): `t` [rows][D] inside a buffer poisoned before, after and (ld > D) between the rows"""
    rows, D = t.shape
    ld = D if ld is None else ld
    buf = torch.full((64 + rows * ld + 64,), poison, dtype=t.dtype, device="cuda")
    view = buf[64:64 + rows * ld].view(rows, ld)[:, :D]
    view.copy_(t)
    return buf, view


def intact(buf, view, poison):
    """every element of the buffer outside the view still holds the poison"""
    mask = torch.ones_like(buf, dtype=torch.bool)
    rows, D = view.shape
    ld = view.stride(0)
    mask[64:64 + rows * ld].view(rows, ld)[:, :D] = False
    return bool((buf[mask] == poison).all())


def kernel_inputs(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    vis, ori, F0 = ((torch.randn(rows, D, generator=g) * 2).to(BF) for _ in range(3))
    D1, D2 = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g) * 0.5
    return vis, ori, F0, D1, D2


def same(a, b):
    return torch.equal(a.cpu(), b.cpu()) and rel(a, b) == 0.0            # rel is NaN for a NaN anywhere: NaN does not pass


def run_update(vis, ori, F0, D1, D2, g, order, have, ld=None):
    from kandinsky import _engine as E
    bv, vv = guarded(vis, 3.0, ld)
    bo, vo = guarded(ori, 3.0)
    bf, vf = guarded(F0, 3.0)
    b1, v1 = guarded(D1, 7.0)
    b2, v2 = guarded(D2, 7.0)
    st = E.lib().k5_forecast_update_bf16(vv.data_ptr(), vv.stride(0), vo.data_ptr(), vf.data_ptr(), v1.data_ptr(), v2.data_ptr(), vis.shape[0],
                                         vis.shape[1], g, order, have, E.stream_ptr())
    torch.cuda.synchronize()
    assert intact(bv, vv, 3.0) and intact(bo, vo, 3.0) and intact(bf, vf, 3.0) and intact(b1, v1, 7.0) and intact(b2, v2, 7.0)
    assert torch.equal(vv.cpu(), vis) and torch.equal(vo.cpu(), ori)      # vis and ori are only read
    return st, vf, v1, v2


def run_apply(vis, F0, D1, D2, k, order, have, ld=None, g=1, gp=1):
    from kandinsky import _engine as E
    bv, vv = guarded(vis, 3.0, ld)
    bf, vf = guarded(F0, 3.0)
    b1, v1 = guarded(D1, 7.0)
    b2, v2 = guarded(D2, 7.0)
    st = E.lib().k5_forecast_apply_bf16(vv.data_ptr(), vv.stride(0), vf.data_ptr(), v1.data_ptr(), v2.data_ptr(), vis.shape[0], vis.shape[1], k, g,
                                        gp, order, have, E.stream_ptr())
    torch.cuda.synchronize()
    assert intact(bv, vv, 3.0) and intact(bf, vf, 3.0) and intact(b1, v1, 7.0) and intact(b2, v2, 7.0)
    assert torch.equal(vf.cpu(), F0) and torch.equal(v1.cpu(), D1) and torch.equal(v2.cpu(), D2)   # the state is only read
    return st, vv


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("rows,D,ld", [(1, 8, None), (3, 24, None), (257, 64, None), (3, 24, 40), (257, 64, 72)])
def test_kernels_bit_exact(rows, D, ld, order):
    from kandinsky import _engine as E
    vis, ori, F0, D1, D2 = kernel_inputs(rows, D, 100 * rows + order)
    for have in (0, 1, 2):
        for g in (1, 3):
            st, f0, d1, d2 = run_update(vis, ori, F0, D1, D2, g, order, have, ld)
            assert st == 0, E.last_error()
            w0, w1, w2 = FR.update_ref(vis, ori, F0, D1, D2, g, order, have)
            assert same(f0, w0) and same(d1, w1) and same(d2, w2), (have, g)
            level = min(order, have)
            assert (level >= 1) != torch.equal(d1.cpu(), D1) and (level >= 2) != torch.equal(d2.cpu(), D2)   # what the level does not reach is not written
    for have in (1, 2, 3):
        for k in (1, 3):
            for g, gp in ((1, 1), (3, 1), (2, 3)):                         # c2 = k (k + g) g / (g + gp): 1, 4.5 and 0.8 k (k + 2) — not all exact
                st, out = run_apply(vis, F0, D1, D2, k, order, have, ld, g, gp)
                assert st == 0, E.last_error()
                assert same(out, FR.apply_ref(vis, F0, D1, D2, k, order, have, g, gp)), (have, k, g, gp)


def test_kernels_past_the_grid():
    """BIG elements are just more than one sweep of the capped grid (1024 workgroups x 256 lanes x 8 elements): the loop takes its second pass"""
    from kandinsky import _engine as E
    n = int(np.prod(BIG))
    D, rows = 16, n // 16
    assert rows * D == n and n > 1024 * 256 * 8 and n - 1024 * 256 * 8 < 1024 * 256 * 8
    vis, ori, F0, D1, D2 = kernel_inputs(rows, D, 5)
    st, f0, d1, d2 = run_update(vis, ori, F0, D1, D2, 3, 2, 2)
    assert st == 0, E.last_error()
    w0, w1, w2 = FR.update_ref(vis, ori, F0, D1, D2, 3, 2, 2)
    assert same(f0, w0) and same(d1, w1) and same(d2, w2)
    edge = 1024 * 256 * 8 // D
    assert torch.equal(d2.cpu()[edge - 4:edge + 4], w2[edge - 4:edge + 4]) and torch.equal(d2.cpu()[-4:], w2[-4:])
    st, out = run_apply(vis, F0, D1, D2, 3, 2, 3, g=3, gp=1)
    assert st == 0, E.last_error()
    want = FR.apply_ref(vis, F0, D1, D2, 3, 2, 3, 3, 1)
    assert same(out, want) and torch.equal(out.cpu()[edge - 4:edge + 4], want[edge - 4:edge + 4]) and torch.equal(out.cpu()[-4:], want[-4:])


def poly(n=24 * 5, seed=3):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randint(-8, 9, (n,), generator=g).float(), torch.randint(-3, 4, (n,), generator=g).float()
    c = torch.randint(-2, 3, (n,), generator=g).float()
    c[0], c[1] = 2.0, -1.0
    ori = torch.randint(-32, 33, (n,), generator=g).float()
    return a, b, c, ori


def gpu_history(r, ori, order, fulls=(0, 2, 4)):
    """full calls at `fulls` through the update export; returns the state on the host and (j, have, g, gp)"""
    rows, D = 5, 24
    F0, D1, D2 = torch.zeros(rows, D, dtype=BF), torch.zeros(rows, D), torch.zeros(rows, D)
    j, have, g, gp = -1, 0, 1, 1
    for i in fulls:
        vis = (ori + r(i)).view(rows, D).to(BF)
        gp, g = g, i - j if have else 1
        st, f0, d1, d2 = run_update(vis, ori.view(rows, D).to(BF), F0, D1, D2, g, order, have)
        assert st == 0
        F0, D1, D2, j, have = f0.cpu().clone(), d1.cpu().clone(), d2.cpu().clone(), i, have + 1
    return F0, D1, D2, j, have, g, gp


def gpu_forecast(state, order, step):
    F0, D1, D2, j, have, g, gp = state
    st, out = run_apply(torch.zeros_like(F0), F0, D1, D2, step - j, order, have, g=g, gp=gp)
    assert st == 0
    return out.cpu().float().view(-1)


@pytest.mark.parametrize("step", [5, 7])
def test_order_2_reproduces_the_quadratic(step):
    """residuals of small integers that follow a + b i + c i^2, full calls at steps 0, 2 and 4: the order-2 forecasts at steps 5 and 7 equal
    the polynomial exactly"""
    a, b, c, ori = poly()
    r = lambda i: a + b * i + c * i * i   # noqa: E731
    got = gpu_forecast(gpu_history(r, ori, 2), 2, step)
    print(f"step {step}: largest deviation from the polynomial {(got - r(step)).abs().max().item()}")
    assert torch.equal(got, r(step))


def test_order_2_reproduces_the_quadratic_over_unequal_gaps():
    """full calls at 0, 2 and 3 (gaps 2 then 1): D2 = 3 c and c2 = k (k + 1) / 3 = 2 and 4 at k = 2 and 3, all exact in fp32"""
    a, b, c, ori = poly()
    r = lambda i: a + b * i + c * i * i   # noqa: E731
    state = gpu_history(r, ori, 2, (0, 2, 3))
    for step in (5, 6):
        assert torch.equal(gpu_forecast(state, 2, step), r(step))


def test_polynomial_lower_orders():
    a, b, c, ori = poly()
    lin = lambda i: a + b * i             # noqa: E731
    quad = lambda i: a + b * i + c * i * i   # noqa: E731
    for order in (1, 2):                                                   # exact when c = 0
        state = gpu_history(lin, ori, order)
        for step in (5, 7):
            assert torch.equal(gpu_forecast(state, order, step), lin(step))
    state = gpu_history(quad, ori, 0)                                      # order 0 returns F0
    for step in (5, 7):
        assert torch.equal(gpu_forecast(state, 0, step), quad(4))


def test_against_gate_sum():
    from kandinsky import _engine as E
    vis, ori, F0, D1, D2 = kernel_inputs(257, 64, 9)
    one = torch.ones(64, device="cuda")
    for order, have in ((0, 1), (0, 3), (2, 1)):                          # m = 0
        st, out = run_apply(vis, F0, D1, D2, 3, order, have)
        assert st == 0 and torch.equal(out, E.gate_sum(vis.cuda(), F0.cuda(), one))
    st, f0, _, _ = run_update(vis, ori, F0, D1, D2, 1, 2, 2)
    assert st == 0 and torch.equal(f0, E.gate_sum(vis.cuda(), ori.cuda(), -one))


def test_launcher_refusals_launch_nothing():
    from kandinsky import _engine as E
    L = E.lib()
    rows, D = 3, 24
    vis, ori, F0, D1, D2 = (t.cuda() for t in kernel_inputs(rows, D, 4))
    keep = [t.clone() for t in (vis, ori, F0, D1, D2)]
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def update(vis=vis, ld=D, ori=ori, F0=F0, D1=D1, D2=D2, rows=rows, D=D, g=1, order=2, have=2):
        return L.k5_forecast_update_bf16(p(vis), ld, p(ori), p(F0), p(D1), p(D2), rows, D, g, order, have, E.stream_ptr())

    def apply(vis=vis, ld=D, F0=F0, D1=D1, D2=D2, rows=rows, D=D, k=1, g=2, gp=2, order=2, have=3):
        return L.k5_forecast_apply_bf16(p(vis), ld, p(F0), p(D1), p(D2), rows, D, k, g, gp, order, have, E.stream_ptr())

    off = lambda t: t.view(-1)[1:]   # noqa: E731  (2 or 4 bytes past a 16-byte boundary)
    for kw in (dict(vis=None), dict(ori=None), dict(F0=None), dict(D1=None), dict(D2=None), dict(D=20), dict(D=0), dict(rows=0), dict(g=0), dict(g=-1),
               dict(order=3), dict(order=-1), dict(have=-1), dict(ld=16), dict(ld=28), dict(vis=off(vis)), dict(ori=off(ori)), dict(F0=off(F0)),
               dict(D1=off(D1)), dict(D2=off(D2))):
        assert update(**kw) == K5_ERR_ARG and "k5_forecast_update_bf16" in E.last_error(), kw
    for kw in (dict(vis=None), dict(F0=None), dict(D1=None), dict(D2=None), dict(D=20), dict(rows=0), dict(k=0), dict(g=0), dict(gp=0), dict(order=3), dict(order=-1),
               dict(have=0), dict(ld=16), dict(ld=28), dict(vis=off(vis)), dict(F0=off(F0)), dict(D1=off(D1)), dict(D2=off(D2))):
        assert apply(**kw) == K5_ERR_ARG and "k5_forecast_apply_bf16" in E.last_error(), kw
    torch.cuda.synchronize()
    for t, k in zip((vis, ori, F0, D1, D2), keep):
        assert torch.equal(t, k)                                           # nothing was launched
    assert update(D1=None, D2=None, order=0) == 0 and update(D2=None, order=1) == 0 and apply(D1=None, D2=None, have=1) == 0   # unused state may be NULL
    assert apply(D2=None, g=0, gp=0, order=1) == 0                         # ... and the gaps are read with two terms only
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the sampler: same bits
@pytest.fixture(scope="module")
def plain_runs(dit, golden):
    return {(n, w): run_generate(dit, golden, w, steps=n) for n in (8, 9) for w in (1.0, 5.0)}


def forecast_run(model, golden, n, w, order, **kw):
    return run_generate(model, golden, w, steps=n, forecast_order=order, **PLANS[n], **kw)


@pytest.fixture(scope="module")
def fused_runs(dit, golden):
    out = {}
    for n, w, order in ((9, 5.0, 2), (9, 1.0, 1), (8, 5.0, 1), (8, 1.0, 2)):
        dit.forecast_state(reset=True)
        out[(n, w, order)] = (forecast_run(dit, golden, n, w, order), dit.forecast_state(reset=True))
    return out


def test_off_and_a_plan_of_ones_are_the_plain_run(dit, golden, plain_runs):
    from kandinsky.generation_utils import sigma_schedule
    te, ne = prompts(golden)
    for w in (1.0, 5.0):
        for kw in (dict(forecast_interval=None), dict(forecast_interval=1), dict(forecast_interval=3, forecast_tail=9), dict(forecast_order=2)):
            assert torch.equal(run_generate(dit, golden, w, steps=9, **kw), plain_runs[(9, w)]), (w, kw)
        assert dit.forecast_state(reset=True) == (False, 0, 0, 0)
        dit.set_forecast(2, [1] * 9)                                       # below generate, in the engine: a plan without a 0
        try:
            lat = golden["gen.noise"].cuda().contiguous().clone()
            dit.sample(lat, sigma_schedule(9, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), w, scale_factor=(1.0, 2.0, 2.0))
            assert torch.equal(lat, plain_runs[(9, w)])
            assert dit.forecast_state(reset=True) == (True, 9 * (2 if w == 5.0 else 1), 0, 0)
        finally:
            dit.clear_forecast()
    assert dit.forecast_state() == (False, 0, 0, 0)


def test_counts_and_the_plan_does_something(fused_runs, plain_runs):
    for (n, w, order), (out, state) in fused_runs.items():
        branches = 2 if w == 5.0 else 1
        assert state[:3] == (False, branches * sum(FULL[n]), branches * (n - sum(FULL[n]))), (n, w, order, state)
        assert torch.isfinite(out).all() and 1e-5 < rel(out, plain_runs[(n, w)]) < 0.1


def test_state_bytes(dit, golden, cfg):
    """the bytes while a plan is held: ori once, F0 + D1 + D2 up to the order per slot that ran"""
    from kandinsky.generation_utils import sigma_schedule
    te, ne = prompts(golden)
    elems = SHAPE[0] * (SHAPE[1] // 2) * (SHAPE[2] // 2) * cfg["model_dim"]
    for order, w in ((0, 1.0), (1, 5.0), (2, 5.0)):
        dit.set_forecast(order, FULL[9])
        try:
            lat = golden["gen.noise"].cuda().contiguous().clone()
            dit.sample(lat, sigma_schedule(9, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), w, scale_factor=(1.0, 2.0, 2.0))
            assert dit.forecast_state()[3] == elems * (2 + (2 if w == 5.0 else 1) * (2 + 4 * order))
        finally:
            dit.clear_forecast()
        assert dit.forecast_state()[3] == 0


def magcache_decisions(table, no_cfg, thresh=0.12, K=2, retention=0.2):
    """MagCache::decide of engine.hip over the calls of one run: {call index: skipped}"""
    err, ratio, steps, out = [0.0, 0.0], [1.0, 1.0], [0, 0], {}
    for cnt in range(0, len(table), 2 if no_cfg else 1):
        j, skip = cnt & 1, False
        if cnt >= int(len(table) * retention):
            ratio[j] *= table[cnt]
            steps[j] += 1
            err[j] += abs(1.0 - ratio[j])
            if err[j] < thresh and steps[j] <= K:
                skip = True
            else:
                err[j], steps[j], ratio[j] = 0.0, 0, 1.0
        out[cnt] = skip
    return out


@pytest.mark.parametrize("no_cfg", [False, True])
def test_order_0_under_magcaches_mask_is_magcache(cfg, sd4, golden, no_cfg):
    from kandinsky.generation_utils import sigma_schedule
    from kandinsky.magcache_utils import disable_magcache, magcache_state, ratio_table, set_magcache_params
    n, w = 10, 1.0 if no_cfg else 5.0
    per_step = [1.0, 0.98, 0.97, 1.05, 0.99, 0.9, 0.99, 1.0, 0.98]       # steps 1..9; both slots the same, so both decide the same
    ratios = [v for r in per_step for v in (r, r)]
    dec = magcache_decisions(ratio_table(ratios, n), no_cfg)
    full = [0 if dec[2 * i] else 1 for i in range(n)]
    assert no_cfg or all(dec[2 * i] == dec[2 * i + 1] for i in range(n))
    assert full[0] == 1 and 2 <= sum(full) < n and any(full[i] == 0 and full[i + 1] == 0 for i in range(n - 1))   # a run of two skipped calls too
    te, ne = prompts(golden)
    d = make_dit(cfg, sd4)
    d.engine("cuda:0")

    def sample():
        lat = golden["gen.noise"].cuda().contiguous().clone()
        d.sample(lat, sigma_schedule(n, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), w, scale_factor=(1.0, 2.0, 2.0))
        return lat
    set_magcache_params(d, ratios, n, no_cfg)
    try:
        mag = sample()
        branches = 1 if no_cfg else 2
        assert magcache_state(d)[1:] == (branches * sum(full), branches * (n - sum(full)))
    finally:
        disable_magcache(d)
    d.set_forecast(0, full)
    got = sample()
    assert d.forecast_state()[1:3] == (branches * sum(full), branches * (n - sum(full)))
    d.clear_forecast()
    assert torch.equal(got, mag)
    assert not torch.equal(got, sample())                                  # ... and the plain run is another
    d._destroy_engine(force=True)


Wrapped = functools.partial(kit.Wrapped, blocks=True,          # this one hands the plan on
                            hand_on=("set_forecast", "clear_forecast", "forecast_at", "_forecast"))


@pytest.mark.parametrize("case", [(9, 5.0, 2), (9, 1.0, 1), (8, 5.0, 1), (8, 1.0, 2)])
def test_fused_equals_stepwise(dit, golden, fused_runs, case):
    n, w, order = case
    dit.forecast_state(reset=True)
    assert torch.equal(forecast_run(Wrapped(dit), golden, n, w, order), fused_runs[case][0])
    assert dit.forecast_state(reset=True) == fused_runs[case][1]


def test_fused_equals_stepwise_with_editing_and_a_watch(dit, golden):
    g = torch.Generator().manual_seed(5)
    Wf, bf = (torch.rand(16, 3, generator=g) - 0.5) * 0.5, (torch.rand(3, generator=g) - 0.5) * 0.4
    src, mask = source_latent(), edit_mask()
    kw = dict(init_latent=src, strength=1.0, keep_mask=mask)
    bare = forecast_run(dit, golden, 9, 5.0, 2, **kw)
    recs, outs = [], []
    for model in (dit, Wrapped(dit)):
        rec = Recorder()
        outs.append(forecast_run(model, golden, 9, 5.0, 2, callback=rec, preview_every=1, preview_factors=(Wf, bf), preview_x0=True, **kw))
        recs.append(rec)
    assert torch.equal(outs[0], bare) and torch.equal(outs[0], outs[1])
    keep = (mask == 1).expand_as(src)
    assert torch.equal(bare.cpu()[keep], src[keep])
    assert len(recs[0].seen) == len(recs[1].seen) == 9
    for a, c in zip(recs[0].seen, recs[1].seen):
        assert a.step == c.step and torch.equal(a.preview, c.preview) and torch.equal(a.x0, c.x0)


def test_the_captured_step_equals_the_eager_run(dit, cfg, sd4, golden, plain_runs, fused_runs):
    from kandinsky.generation_utils import sigma_schedule
    te, ne = prompts(golden)
    gdit = make_dit(cfg, sd4)
    gdit.engine("cuda:0")
    gdit.set_graph(True)
    assert torch.equal(forecast_run(gdit, golden, 9, 5.0, 2), fused_runs[(9, 5.0, 2)][0])     # steps of two kinds: eager on the graph handle too
    gdit.forecast_state(reset=True)
    gdit.set_forecast(2, [1] * 9)                                          # a plan of one kind: the capture is used, the replays are counted
    lat = golden["gen.noise"].cuda().contiguous().clone()
    gdit.sample(lat, sigma_schedule(9, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0))
    assert torch.equal(lat, plain_runs[(9, 5.0)]) and gdit.forecast_state() == (True, 18, 0, 0)
    gdit._destroy_engine(force=True)


def test_sample_many_equals_separate_calls(dit, golden):
    from kandinsky.generation_utils import generate
    g = torch.Generator().manual_seed(41)
    te, ne = prompts(golden)
    te2 = {"text_embeds": torch.randn(5, 96, generator=g).cuda(), "pooled_embed": torch.randn(1, 48, generator=g).cuda()}
    noise = torch.cat([golden["gen.noise"], torch.randn(*SHAPE, generator=g)])
    tes, tps = [te, te2], [torch.arange(7), torch.arange(5)]
    kw = dict(forecast_order=2, **PLANS[9])
    dit.forecast_state(reset=True)
    out = generate(dit, "cuda:0", (2 * SHAPE[0],) + SHAPE[1:], 9, tes, ne, POS, tps, torch.arange(4), 5.0, 5.0, FLASH, noise=noise, batch=2, **kw)
    assert dit.forecast_state(reset=True)[1:3] == (2 * 2 * 5, 2 * 2 * 4)
    for b in range(2):
        one = generate(dit, "cuda:0", SHAPE, 9, tes[b], ne, POS, tps[b], torch.arange(4), 5.0, 5.0, FLASH, noise=noise[b * 3:(b + 1) * 3], **kw)
        assert torch.equal(out[b * 3:(b + 1) * 3], one), b


def test_stochastic_and_cut_edit_runs_complete_and_repeat(dit, cfg, sd4, golden, plain_runs):
    """what MagCache refuses: eta = 1, and strength 0.6 with a mask (the plan covers the steps that run)"""
    from kandinsky.generation_utils import edit_first_step
    from kandinsky.magcache_utils import set_magcache_params
    runs = (dict(eta=1.0, sde_seed=7), dict(init_latent=source_latent(), strength=0.6, keep_mask=edit_mask()))
    for kw in runs:
        dit.forecast_state(reset=True)
        a = run_generate(dit, golden, 5.0, steps=9, forecast_interval=2, forecast_warmup=2, forecast_order=2, **kw)
        state = dit.forecast_state(reset=True)
        steps_run = 9 - edit_first_step(9, 0.6) if "strength" in kw else 9
        full = FR.plan(steps_run, 2, 2, 1)
        assert state[:3] == (False, 2 * sum(full), 2 * (steps_run - sum(full))) and sum(full) < steps_run
        assert torch.isfinite(a).all() and torch.equal(a, run_generate(dit, golden, 5.0, steps=9, forecast_interval=2, forecast_warmup=2,
                                                                       forecast_order=2, **kw))
        assert torch.equal(a, run_generate(Wrapped(dit), golden, 5.0, steps=9, forecast_interval=2, forecast_warmup=2, forecast_order=2, **kw))
        assert not torch.equal(a, run_generate(dit, golden, 5.0, steps=9, **kw))
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    d = make_dit(cfg, sd4)
    d.engine("cuda:0")
    set_magcache_params(d, c["ratios"], 9, False)
    for kw in runs:
        with pytest.raises((ValueError, RuntimeError)):
            run_generate(d, golden, 5.0, steps=9, **kw)
    d._destroy_engine(force=True)


# ------------------------------------------------------------------------------------------ parity
@pytest.fixture(scope="module")
def forecast_golden():
    from safetensors.torch import load_file
    return load_file(os.path.join(GOLDEN, "dit_tiny_forecast.safetensors")), json.load(open(os.path.join(GOLDEN, "dit_tiny_forecast_meta.json")))


@pytest.mark.parametrize("name", ["p9_w5_o2", "p9_w1_o1", "p8_w5_o1", "p8_w1_o2"])
def test_parity_with_the_oracle_and_the_reference_golden(fused_runs, sd4, cfg, golden, forecast_golden, name):
    """The engine's final latent within 1e-2 of the bf16 oracle loop, and within 1.5 x what that oracle loop itself is from the reference's
    fp32 golden (recorded by tools/gen_golden_forecast.py): extrapolation multiplies the bf16 realisation error by up to 1 + 2 k, so the
    bound scales with what the host-side bf16 oracle loses under the same plan."""
    gold, meta = forecast_golden
    case = meta["cases"][name]
    n, w, order = case["steps"], case["w"], case["order"]
    assert meta["weights_sha256"] == S.weights_sha256(sd4) and meta["scheduler_scale"] == 5.0
    assert case["full"] == FULL[n] == FR.plan(n, *meta["plans"][str(n)])
    out = fused_runs[(n, w, order)][0]
    ocfg = O.DitConfig(**cfg)
    noise = golden["gen.noise"]
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)
    conds = [(golden["fwd.text"], golden["fwd.pooled"], torch.arange(7)), (golden["gen.null_text"], golden["gen.null_pooled"], torch.arange(4))]
    cache = FR.Cache(order, case["full"], "bf16")

    def vel(x, s, step, slot):
        text, pooled, tpos = conds[slot]
        return FR.dit_forward_forecast(sd4, ocfg, torch.cat([x, *zeros], -1), text, pooled, s.unsqueeze(0) * 1000, POS, tpos, (1.0, 2.0, 2.0), None,
                                       "bf16", cache, step, slot)
    ref16 = FR.bf16_loop(vel, noise, O.sigma_schedule(n, 5.0), w)
    r16, r32, o32 = rel(out, ref16), rel(out, gold[f"forecast.{name}.final"]), meta["oracle_vs_golden"][name]
    print(f"forecast {name}: engine vs bf16 oracle {r16:.3e}, vs reference golden {r32:.3e} (oracle vs golden {o32:.3e}, bound {1.5 * o32:.3e})")
    assert r16 <= 1e-2, r16
    assert r32 <= 1.5 * o32, (r32, o32)


# ------------------------------------------------------------------------------------------ ranks
@pytest.mark.timeout(600)
def test_loopback_ranks(sd4, cfg):
    from edit_rank_worker import case
    from test_gpu_loopback import run_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne, _, _ = case()
    te, ne = {k: v.cuda() for k, v in te.items()}, {k: v.cuda() for k, v in ne.items()}
    pos = [torch.arange(8)] * 3
    kw = dict(forecast_interval=2, forecast_order=2, forecast_warmup=3, forecast_tail=1)   # 6 steps: 1 1 1 1 0 1

    def call(d, r):
        out = generate(d, "cuda:0", shape, 6, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, **kw)
        assert d.forecast_state()[:3] == (False, 10, 2)
        return out

    make = lambda: make_dit(cfg, sd4)    # noqa: E731
    fused = call(make(), 0)
    outs = run_ranks(2, make, call)
    assert torch.equal(outs[1], outs[0])
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(dit, cfg, sd4, golden, plain_runs):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import context_windows, sigma_schedule
    from kandinsky.magcache_utils import disable_magcache, set_magcache_params, start_magcache_calibration, stop_magcache_calibration
    te, ne = prompts(golden)
    lat = golden["gen.noise"].cuda().contiguous()
    before = lat.clone()
    L = E.lib()

    def refused(d, status, word, steps=9, w=5.0, pos=POS, **kw):
        state = d.forecast_state()
        with pytest.raises(RuntimeError, match=f"status {status}") as e:
            d.sample(lat, sigma_schedule(steps, 5.0).tolist(), te, ne, pos, torch.arange(7), torch.arange(4), w, scale_factor=(1.0, 2.0, 2.0), **kw)
        assert word in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(lat, before) and d.forecast_state() == state

    # the setter itself: a refused plan leaves the handle without one
    h = dit.engine(lat.device)
    ones, zero_first = (C.c_ubyte * 3)(1, 0, 1), (C.c_ubyte * 3)(0, 1, 1)
    ptr = lambda a: C.cast(a, C.POINTER(C.c_ubyte))   # noqa: E731
    for plan, word in ((E.Forecast(1, ptr(zero_first), 3), b"full[0]"), (E.Forecast(3, ptr(ones), 3), b"order"), (E.Forecast(-1, ptr(ones), 3), b"order"),
                       (E.Forecast(1, ptr(ones), 0), b"num_steps"), (E.Forecast(1, None, 3), b"num_steps")):
        assert L.k5_dit_set_forecast(h, C.byref(plan)) == K5_ERR_ARG and word in L.k5_last_error()
        assert dit.forecast_state()[0] is False
    assert L.k5_dit_forecast_at(h, 0, 0) == K5_ERR_STATE                   # no plan: no cursor

    dit.forecast_state(reset=True)
    dit.set_forecast(1, FULL[9])
    try:
        refused(dit, K5_ERR_ARG, "9 steps", steps=8)                       # a plan of another length than the call
        assert L.k5_dit_forecast_at(h, 9, 0) == K5_ERR_ARG and L.k5_dit_forecast_at(h, -1, 0) == K5_ERR_ARG and L.k5_dit_forecast_at(h, 0, 2) == K5_ERR_ARG
        dit.set_skip_guidance([1], 3.0)
        refused(dit, K5_ERR_STATE, "skip")
        dit.clear_skip_guidance()
        dit.set_guidance([5.0] * 5 + [1.0] * 4)
        refused(dit, K5_ERR_STATE, "guided and unguided")
        dit.set_guidance(None, True, 2)
        refused(dit, K5_ERR_STATE, "zero-init")
        dit.clear_guidance()
        starts, weights = context_windows(3, 2, 1)
        refused(dit, K5_ERR_STATE, "window", pos=[torch.arange(2), POS[1], POS[2]], windows=(starts, weights))
        # a forecast call whose slot has no full call yet, and one whose residual has another shape
        x = torch.cat([golden["gen.noise"], torch.zeros(*SHAPE[:3], SHAPE[3] + 1)], -1).cuda()
        args = (golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), torch.tensor([700.0]), POS, torch.arange(7))
        plain = dit(x, *args, scale_factor=(1.0, 2.0, 2.0)).clone()
        dit.forecast_at(3, 0)
        with pytest.raises(RuntimeError, match=f"status {K5_ERR_STATE}") as e:
            dit(x, *args, scale_factor=(1.0, 2.0, 2.0))
        assert "no full call" in str(e.value)
        dit.forecast_at(2, 0)
        assert torch.equal(dit(x, *args, scale_factor=(1.0, 2.0, 2.0)), plain)    # a full call's output is the plain forward's
        assert torch.equal(dit(x, *args, scale_factor=(1.0, 2.0, 2.0)), plain)    # the cursor is spent: a plain forward, no state touched
        assert dit.forecast_state()[1:3] == (1, 0)
        dit.forecast_at(3, 0)
        fc = dit(x, *args, scale_factor=(1.0, 2.0, 2.0)).clone()            # a forecast call: order 0 worth of history
        assert dit.forecast_state()[1:3] == (1, 1) and torch.isfinite(fc.float()).all() and not torch.equal(fc, plain)
        dit.forecast_at(3, 1)                                              # the other slot has nothing
        with pytest.raises(RuntimeError, match=f"status {K5_ERR_STATE}"):
            dit(x, *args, scale_factor=(1.0, 2.0, 2.0))
        x2 = torch.cat([x, x], 0)[:4].contiguous()
        dit.forecast_at(4, 0)
        with pytest.raises(RuntimeError, match=f"status {K5_ERR_STATE}") as e:
            dit(x2, args[0], args[1], args[2], [torch.arange(4), POS[1], POS[2]], args[4], scale_factor=(1.0, 2.0, 2.0))
        assert "another shape" in str(e.value)
        dit.forecast_at(2, 0)                                              # a full call at step <= j starts the history over; then step 3 forecasts again
        assert torch.equal(dit(x, *args, scale_factor=(1.0, 2.0, 2.0)), plain)
        dit.forecast_at(3, 0)
        assert torch.equal(dit(x, *args, scale_factor=(1.0, 2.0, 2.0)), fc)
    finally:
        dit.clear_skip_guidance()
        dit.clear_guidance()
        dit.clear_forecast()
    assert dit.forecast_state(reset=True)[0] is False

    # MagCache and its calibration, in either order
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    d = make_dit(cfg, sd4)
    d.engine("cuda:0")
    set_magcache_params(d, c["ratios"], c["num_steps"], c["no_cfg"])
    try:
        with pytest.raises(RuntimeError, match=f"status {K5_ERR_STATE}"):
            d.set_forecast(1, FULL[9])
        assert d._forecast is None and d.forecast_state()[0] is False
    finally:
        disable_magcache(d)
    start_magcache_calibration(d, 2, False)
    try:
        with pytest.raises(RuntimeError, match=f"status {K5_ERR_STATE}"):
            d.set_forecast(1, FULL[9])
    finally:
        stop_magcache_calibration(d)
    d.set_forecast(1, FULL[9])
    with pytest.raises(RuntimeError, match="forecast"):
        set_magcache_params(d, c["ratios"], c["num_steps"], c["no_cfg"])
    assert d.mag_ratios is None
    with pytest.raises(RuntimeError, match="forecast"):
        start_magcache_calibration(d, 2, False)
    d._destroy_engine(force=True)
    pair = make_dit(cfg, sd4)
    pair.engine("cuda:0")
    group = E.LoopbackGroup(2)
    pair.enable_cfg_pair_loopback(group, 0)
    pair.set_forecast(1, FULL[9])
    refused(pair, K5_ERR_STATE, "CFG pair")
    pair._destroy_engine(force=True)

    # every refusal left the handle usable: the next plain run's bits are unchanged
    assert torch.equal(run_generate(dit, golden, 5.0, steps=9), plain_runs[(9, 5.0)])


def test_keyword_refusals_name_the_keyword(dit, golden):
    for kw, word in ((dict(slg_blocks=[1], slg_scale=3.0), "slg_blocks"), (dict(guidance_interval=(0.6, 0.97)), "guidance_interval"),
                     (dict(cfg_zero_star=True, cfg_zero_init=2), "cfg_zero_init")):
        with pytest.raises(ValueError, match=word):
            run_generate(dit, golden, 5.0, steps=9, forecast_order=1, **PLANS[9], **kw)

    class Bare(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m, self.visual_cond = m, m.visual_cond

        def forward(self, *a, **k):
            return self.m(*a, **k)
    with pytest.raises(ValueError, match="forecast_at"):
        run_generate(Bare(dit), golden, 5.0, steps=9, forecast_order=1, **PLANS[9])
    assert dit.forecast_state()[0] is False
