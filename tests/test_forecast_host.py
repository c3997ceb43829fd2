"""The forecast cache on the host: the plan, its default warm-up, the keyword refusals of `generate`, and the restatement of the rule
(tests/forecast_reference.py) on residuals that follow a polynomial in the step.  No GPU."""
import os
import sys
from types import SimpleNamespace as NS

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import forecast_reference as FR  # noqa: E402

from kandinsky import _engine as E  # noqa: E402
from kandinsky import generation_utils as G  # noqa: E402
from kandinsky.models.dit import check_forecast_args  # noqa: E402

BF = torch.bfloat16


def test_plans():
    assert G.forecast_plan(9, 3, 2, 1) == [1, 1, 1, 0, 0, 1, 0, 0, 1]      # forecasts with k = 1 and 2, an update with g = 3
    assert G.forecast_plan(8, 2, 3, 1) == [1, 1, 1, 1, 0, 1, 0, 1]
    assert G.forecast_plan(9, 1, 2, 1) == [1] * 9                          # interval 1: off
    assert G.forecast_plan(9, 3, 2, 9) == [1] * 9 and G.forecast_plan(9, 3, 2, 20) == [1] * 9   # a tail that covers every step
    assert G.forecast_plan(9, 3, 2, 0) == [1, 1, 1, 0, 0, 1, 0, 0, 1] and G.forecast_plan(10, 3, 2, 0)[-1] == 0
    for n, i, w, t in ((9, 3, 2, 1), (8, 2, 3, 1), (50, 4, 10, 2), (5, 7, 1, 0)):
        assert G.forecast_plan(n, i, w, t) == FR.plan(n, i, w, t) and G.forecast_plan(n, i, w, t)[0] == 1


def test_default_warmup():
    assert G.forecast_plan(9, 3, order=2) == G.forecast_plan(9, 3, 3)      # max(order + 1, int(1.8))
    assert G.forecast_plan(9, 3, order=0) == G.forecast_plan(9, 3, 1)
    assert G.forecast_plan(50, 3, order=1) == G.forecast_plan(50, 3, 10)   # MagCache's retention share
    assert G.forecast_plan(50, 3) == G.forecast_plan(50, 3, 10)


def test_bad_numbers():
    for kw, word in ((dict(interval=0), "forecast_interval"), (dict(interval=2, warmup=0), "forecast_warmup"), (dict(interval=2, tail=-1), "forecast_tail"),
                     (dict(interval=2, order=3), "forecast_order"), (dict(interval=2, order=-1), "forecast_order")):
        with pytest.raises(ValueError, match=word):
            G.forecast_plan(9, **kw)
    with pytest.raises(ValueError, match="num_steps"):
        G.forecast_plan(0, 2)
    assert check_forecast_args(2, [1, 0, 5]) == (2, [1, 0, 1])
    for order, full, word in ((3, [1], "order"), (True, [1], "order"), (1.0, [1], "order"), (1, [], "full"), (1, [0, 1], r"full\[0\]")):
        with pytest.raises(ValueError, match=word):
            check_forecast_args(order, full)


class Takes:   # a model that takes a plan
    def set_forecast(self, *a):
        pass

    def forecast_at(self, *a):
        pass


def test_keyword_refusals():
    run = lambda model=None, n=9, interval=3, order=1, warmup=2, tail=1, guide=None, skip=None, windowed=False: G._forecast_for_run(   # noqa: E731
        Takes() if model is None else model, n, interval, order, warmup, tail, guide, skip, windowed)
    assert run() == (1, [1, 1, 1, 0, 0, 1, 0, 0, 1])
    assert run(interval=None) is None and run(interval=1) is None and run(tail=9) is None     # off: nothing is installed
    assert run(n=5, interval=3, warmup=2, tail=1) == (1, [1, 1, 1, 0, 1])                      # an edit run: the plan over the steps it executes
    mag, cal, pair = Takes(), Takes(), Takes()
    mag.mag_ratios, cal._magcache_calibrate, pair._cfg_pair = [1.0], (9, False), 0
    for kw, word in ((dict(model=mag), "MagCache"), (dict(model=cal), "MagCache"), (dict(skip=([1], 3.0, "block", None)), "slg_blocks"),
                     (dict(guide=([5.0] * 5 + [1.0] * 4, False, 0, 0.0)), "guidance_schedule"), (dict(guide=(None, True, 2, 0.0)), "cfg_zero_init"),
                     (dict(windowed=True), "context_frames"), (dict(model=pair), "CFG pair"), (dict(model=NS()), "forecast_at"),
                     (dict(order=3), "forecast_order"), (dict(interval=0), "forecast_interval")):
        with pytest.raises(ValueError, match=word):
            run(**kw)
    assert run(guide=([5.0] * 9, True, 0, 0.7)) is not None              # a plan of one kind is served
    assert run(guide=(None, False, 0, 0.0)) is not None


def test_the_exports_are_bound():
    for name in ("k5_forecast_update_bf16", "k5_forecast_apply_bf16", "k5_dit_set_forecast", "k5_dit_forecast_at", "k5_dit_forecast_state"):
        assert name in E.SYMBOLS and hasattr(E.lib(), name)


# ------------------------------------------------------------------------------------------ the rule on a polynomial
def poly_case(c_on, seed=3, n=40):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randint(-8, 9, (n,), generator=g).float(), torch.randint(-3, 4, (n,), generator=g).float()
    c = torch.randint(-2, 3, (n,), generator=g).float() if c_on else torch.zeros(n)
    if c_on:
        c[0], c[1] = 2.0, -1.0
    ori = torch.randint(-32, 33, (n,), generator=g).float()
    return lambda i: a + b * i + c * i * i, ori, c


def run_rule(r, ori, order, fulls=(0, 2, 4)):
    """the state after full calls at `fulls` on residuals r(i): every value is a small integer, exact in bf16"""
    F0 = D1 = D2 = None
    j, have, g, gp = -1, 0, 1, 1
    for i in fulls:
        vis = (ori + r(i)).to(BF)
        assert torch.equal(vis.float(), ori + r(i))
        gp, g = g, i - j if have else 1
        F0, D1, D2 = FR.update_ref(vis, ori.to(BF), F0, D1, D2, g, order, have)
        j, have = i, have + 1
    return F0, D1, D2, j, have, g, gp


def forecast(state, order, i, base):
    F0, D1, D2, j, have, g, gp = state
    return FR.apply_ref(base.to(BF), F0, D1, D2, i - j, order, have, g, gp).float() - base


@pytest.mark.parametrize("step", [5, 7])
def test_order_2_reproduces_the_quadratic(step):
    """full calls at steps 0, 2 and 4 of r(i) = a + b i + c i^2, then the order-2 forecasts at steps 5 and 7 equal the polynomial exactly"""
    r, ori, c = poly_case(True)
    got = forecast(run_rule(r, ori, 2), 2, step, torch.zeros_like(ori))
    print(f"step {step}: largest deviation from the polynomial {(got - r(step)).abs().max().item()}")
    assert torch.equal(got, r(step))


@pytest.mark.parametrize("step", [5, 6])
def test_order_2_reproduces_the_quadratic_over_unequal_gaps(step):
    """full calls at 0, 2 and 3 (gaps 2 then 1): D2 = 3 c and c2 = k (k + 1) / 3 = 2 and 4 at k = 2 and 3, all exact in fp32"""
    r, ori, c = poly_case(True)
    assert torch.equal(forecast(run_rule(r, ori, 2, (0, 2, 3)), 2, step, torch.zeros_like(ori)), r(step))


def test_order_1_misses_a_quadratic():
    """... by the curvature the slope half a gap back leaves out: c k (k + g)"""
    r, ori, c = poly_case(True)
    for step in (5, 7):
        k = step - 4
        assert torch.equal(forecast(run_rule(r, ori, 1), 1, step, torch.zeros_like(ori)), r(step) - c * k * (k + 2))


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("step", [5, 7])
def test_linear_residuals_are_exact(order, step):
    r, ori, _ = poly_case(False)
    base = torch.arange(40).float() - 20
    assert torch.equal(forecast(run_rule(r, ori, order), order, step, base), r(step))


def test_order_0_returns_F0():
    r, ori, _ = poly_case(True)
    for step in (5, 7):
        assert torch.equal(forecast(run_rule(r, ori, 0), 0, step, torch.zeros_like(ori)), r(4))
    F0, D1, D2, j, have, g, gp = run_rule(r, ori, 0)
    assert D1 is None and D2 is None and (j, have, g, gp) == (4, 3, 2, 2)


def test_the_cache_is_the_two_passes():
    """FR.Cache around `blocks` in bf16 mode holds the state update_ref / apply_ref give"""
    r, ori, _ = poly_case(True)
    full = [1, 0, 1, 0, 1, 0, 0, 0]
    cache = FR.Cache(2, full, "bf16")
    for i in range(8):
        out = cache.around(ori, lambda v: v + r(i), i, 0)
        if full[i]:
            assert torch.equal(out, ori + r(i))
        else:
            fulls = tuple(k for k in range(i) if full[k])
            assert torch.equal(out - ori, forecast(run_rule(r, ori, 2, fulls), 2, i, ori)), i
    assert (cache.full_calls, cache.forecast_calls) == (3, 5)
