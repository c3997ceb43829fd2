"""The sampler's guidance controls on the MI355X: the statistics kernel integer-exact, the coefficients within 1 fp32 ulp of the float64 rule,
the guided update bit for bit against the torch expression, k5_sample* with a guidance plan through every mode of the fused sampler (the
same bits as the plain run where the plan is one, as the per-step loop everywhere), parity with the bf16 oracle and the reference's golden,
rank groups, and every refusal.

Tolerances are those of tests/test_gpu_dit.py and tests/test_gpu_edit.py: a final latent within relative L2 1e-2 of the bf16-island oracle
and 3e-2 of the reference's fp32 golden (tools/gen_golden_guidance.py).  Everything that claims "the same computation" is asserted bit for bit."""
import ctypes as C
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402

import guidance_reference as R  # noqa: E402
import kit  # noqa: E402
from kit import (GOLDEN, K5_ERR_ARG, K5_ERR_STATE, K5_ERR_UNSUPPORTED, POS, _sp_case, cfg,  # noqa: E402
                 edit_mask, f32, flash_conf, make_dit, prompts, rel, source_latent, tiny_dit, Wrapped)

FLASH = flash_conf()
BF = torch.bfloat16
SHAPE = (3, 8, 12, 16)
STEPS = 6
SCHEDULE = [5.0, 4.5, 4.0, 3.5, 3.0, 2.5]
INTERVAL = (0.6, 0.97)      # of the sigmas 1, .962, .909, .833, .714, .5 (6 steps, scale 5) steps 1..4 lie inside: a mixed plan
PLANS = {"schedule": dict(guidance_schedule=SCHEDULE),
         "interval": dict(guidance_interval=INTERVAL),
         "zero_star_init": dict(cfg_zero_star=True, cfg_zero_init=1),
         "rescale": dict(cfg_rescale=0.7),
         "all": dict(guidance_schedule=SCHEDULE, guidance_interval=INTERVAL, cfg_zero_star=True, cfg_zero_init=1, cfg_rescale=0.7)}


def run_generate(model, golden, w=5.0, steps=STEPS, **kw):
    return kit.run_generate(model, golden, w, steps=steps, shape=SHAPE, pos=POS, **kw)


# ------------------------------------------------------------------------------------------ kernels: the statistics
def stats_sizes():
    from kandinsky import _engine as E
    cap = E.lib().k5_guidance_stats_blocks(1 << 40)
    big = 8 * 256 * cap + 4608
    assert E.lib().k5_guidance_stats_blocks(big) == cap          # the grid-stride loop takes a second sweep
    return [8, 4608, 11200, big]


def integer_inputs(n, seed):
    """integers in [-128, 128] over 16: exact in bf16, every product a multiple of 1 / 256, so float64 sums are exact in any order"""
    g = torch.Generator().manual_seed(seed)
    c, u = (torch.randint(-128, 129, (n,), generator=g).float() / 16.0 for _ in range(2))
    return c.to(BF).cuda(), u.to(BF).cuda()


def launch_coeffs(c, u, w, zero_star, rescale):
    """the raw entry with guard doubles after part, sums and ab; returns (ab fp32 [2], sums float64 [5]) on the CPU"""
    from kandinsky import _engine as E
    n = c.numel()
    nb = E.lib().k5_guidance_stats_blocks(n)
    part = torch.full((nb * 5 + 8,), 7.0, dtype=torch.float64, device="cuda")
    sums = torch.full((5 + 8,), 7.0, dtype=torch.float64, device="cuda")
    ab = torch.full((1 + 8,), 7.0, dtype=torch.float64, device="cuda")              # two floats in the first double
    E.check(E.lib().k5_guidance_coeffs_bf16(c.data_ptr(), u.data_ptr(), n, w, int(zero_star), rescale, part.data_ptr(), sums.data_ptr(),
                                            ab.data_ptr(), E.stream_ptr()), "k5_guidance_coeffs_bf16")
    torch.cuda.synchronize()
    assert (part[nb * 5:] == 7.0).all() and (sums[5:] == 7.0).all() and (ab[1:] == 7.0).all()
    assert torch.isfinite(part[:nb * 5]).all()
    return ab[:1].view(torch.float32).cpu().clone(), sums[:5].cpu().clone()


def test_sums_are_integer_exact():
    for n in stats_sizes():
        c, u = integer_inputs(n, n % 1000)
        _, sums = launch_coeffs(c, u, 5.0, 1, 0.7)
        cd, ud = c.double(), u.double()
        want = torch.stack([cd.sum(), ud.sum(), (cd * cd).sum(), (ud * ud).sum(), (cd * ud).sum()]).cpu()
        print(f"n={n}: sums {sums.tolist()}")
        assert torch.equal(sums, want), (n, sums.tolist(), want.tolist())
        assert float(sums[2]) * 256 == int(float(sums[2]) * 256)


def coeff_inputs():
    g = torch.Generator().manual_seed(31)
    sets = {}
    for n in (4608, 11200):
        base = torch.randn(n, generator=g)
        sets[f"randn{n}"] = (base.to(BF).cuda(), (0.6 * base + 0.8 * torch.randn(n, generator=g)).to(BF).cuda())
    base = torch.randn(4608, generator=g)
    sets["offset2"] = ((base + 2.0).to(BF).cuda(), (0.5 * base + torch.randn(4608, generator=g) + 2.0).to(BF).cuda())
    for n in stats_sizes():
        sets[f"int{n}"] = integer_inputs(n, 7 + n % 1000)
    return sets


def test_coefficients_within_one_ulp_of_the_float64_rule():
    from kandinsky import _engine as E
    worst = 0
    for name, (c, u) in coeff_inputs().items():
        want_sums = R.five_sums(c.cpu(), u.cpu())
        for w in (1.5, 5.0):
            for zero_star in (0, 1):
                for rescale in (0.0, 0.7, 1.0):
                    ab, sums = launch_coeffs(c, u, w, zero_star, rescale)
                    alpha, beta = R.coeffs_from_sums(want_sums, c.numel(), w, zero_star, rescale)
                    d = max(R.ulp_distance_f32(ab[0].item(), alpha), R.ulp_distance_f32(ab[1].item(), beta))
                    worst = max(worst, d)
                    assert torch.isfinite(ab).all()
                    assert d <= 1, (name, w, zero_star, rescale, ab.tolist(), (alpha, beta))
                    if not zero_star and rescale == 0.0:
                        assert ab.tolist() == [f32(w), f32(1.0 - w)]
                    ab2, sums2 = launch_coeffs(c, u, w, zero_star, rescale)              # no atomics: two launches, the same bits
                    assert torch.equal(ab.view(torch.int32), ab2.view(torch.int32)) and torch.equal(sums, sums2)
        hab, hsums = E.guidance_coeffs(c.view(-1, 8), u.view(-1, 8), 5.0, True, 0.7)  # the helper: the same launch
        ab, sums = launch_coeffs(c, u, 5.0, 1, 0.7)
        assert torch.equal(hab.cpu(), ab) and torch.equal(hsums.cpu(), sums)
    print(f"worst distance from the float64 rule: {worst} ulp")


def test_coefficient_edge_cases():
    c, u = coeff_inputs()["randn4608"]
    ab, _ = launch_coeffs(c, c.clone(), 5.0, 1, 0.0)                                     # u == c: the projection is 1 to fp32 precision
    assert R.ulp_distance_f32(ab[0].item(), 5.0) == 0 and R.ulp_distance_f32(ab[1].item(), -4.0) <= 1
    for rescale in (0.0, 0.7, 1.0):
        ab, sums = launch_coeffs(c, torch.zeros_like(c), 5.0, 1, rescale)                # u == 0: finite
        assert torch.isfinite(ab).all() and ab[1].item() == 0.0 and sums[3].item() == 0.0
        ab, _ = launch_coeffs(torch.zeros_like(c), torch.zeros_like(c), 5.0, 1, rescale)   # nothing at all: still finite
        assert torch.isfinite(ab).all()


# ------------------------------------------------------------------------------------------ kernels: the update
def renoise_ref(x0, eps, sigma):
    a = f32(np.float32(1.0) - np.float32(sigma))
    return a * x0 + f32(sigma) * eps


@pytest.mark.parametrize("dims", [(3, 8, 12, 16), (5, 10, 14, 16)])
@pytest.mark.parametrize("sigma", [0.0, 0.37, 1.0])
@pytest.mark.parametrize("ab", [(5.0, -4.0), (2.2, -1.3137)])
def test_guided_euler_bit_exact(dims, sigma, ab):
    from kandinsky import _engine as E
    n, cells, Cc = int(np.prod(dims)), int(np.prod(dims[:-1])), dims[-1]
    g = torch.Generator().manual_seed(n + int(ab[0]))
    img, x0, eps = torch.randn(n, generator=g).cuda(), (torch.randn(n, generator=g) * 3).cuda(), torch.randn(n, generator=g).cuda()
    c, u = torch.randn(n, generator=g).cuda().to(BF), torch.randn(n, generator=g).cuda().to(BF)
    mask = torch.tensor([0.0, 1.0, 0.25])[torch.randint(0, 3, (cells,), generator=g)].cuda()
    assert all((mask == v).any() for v in (0.0, 1.0, 0.25))
    al, be = f32(ab[0]), f32(ab[1])                                     # what the coefficient kernel would have left: fp32 numbers
    abd = torch.tensor([al, be], dtype=torch.float32, device="cuda")
    dt = f32(-0.0625 * 1.3)
    v = (al * c.float() + be * u.float()).to(BF)                        # three separately rounded fp32 ops, then bf16
    x = img + (dt * v.float()).to(BF).float()
    known = renoise_ref(x0, eps, sigma)
    m = mask.repeat_interleave(Cc)
    want = torch.where(m == 1, known, torch.where(m == 0, x, x + m * (known - x)))
    L = E.lib()

    def run(maskp, vout_of):
        buf = torch.full((n + 64,), 7.0, device="cuda")                 # a guard region after the latent
        buf[:n] = img
        cc = torch.full((n + 64,), 3.0, dtype=BF, device="cuda")        # ... and after the velocity that v_out may alias
        cc[:n] = c
        vo = vout_of(cc)
        E.check(L.k5_guided_euler(buf.data_ptr(), cc.data_ptr(), u.data_ptr(), abd.data_ptr(), dt, x0.data_ptr() if maskp else None,
                                  eps.data_ptr() if maskp else None, maskp, sigma, cells, Cc, None if vo is None else vo.data_ptr(), E.stream_ptr()),
                "k5_guided_euler")
        torch.cuda.synchronize()
        assert (buf[n:] == 7.0).all() and (cc[n:] == 3.0).all()
        return buf[:n], cc[:n], vo

    out, cc, _ = run(mask.data_ptr(), lambda cc: None)                   # with mask, no v_out: v_cond is not written
    assert torch.equal(out, want) and torch.equal(cc, c)
    if sigma == 0.0:
        assert torch.equal(out[m == 1], x0[m == 1])
    out, cc, _ = run(mask.data_ptr(), lambda cc: cc)                     # v_out aliasing v_cond
    assert torch.equal(out, want) and torch.equal(cc, v)
    sep = torch.full((n + 64,), 3.0, dtype=BF, device="cuda")
    out, cc, vo = run(None, lambda cc: sep)                              # without mask, v_out apart
    assert torch.equal(out, x) and torch.equal(cc, c) and torch.equal(vo[:n], v) and (vo[n:] == 3.0).all()
    # the helper
    helper, vv = img.clone().view(dims), c.clone().view(dims)
    E.guided_euler_(helper, vv, u.view(dims), abd, dt, x0.view(dims), eps.view(dims), mask.view(*dims[:-1], 1), sigma, v_out=vv)
    assert torch.equal(helper.view(-1), want) and torch.equal(vv.view(-1), v)
    # x0_preview with v_uncond = NULL on the guided velocity is the preview of the guided step
    _, p0 = E.x0_preview(helper, vv, None, 1.0, sigma, want_x0=True)
    assert torch.equal(p0.view(-1), want - f32(sigma) * v.float())


# ------------------------------------------------------------------------------------------ sampler: same bits
@pytest.fixture(scope="module")
def plain_runs(tiny_dit, golden):
    """the runs without a plan that the tests below compare against, each computed once"""
    return {w: run_generate(tiny_dit, golden, w) for w in (1.0, 5.0)}


def test_a_constant_schedule_is_the_plain_run(tiny_dit, golden, plain_runs):
    tiny_dit.guidance_state(reset=True)
    out = run_generate(tiny_dit, golden, 5.0, guidance_schedule=[5.0] * STEPS)
    assert torch.equal(out, plain_runs[5.0])
    assert tiny_dit.guidance_state() == (False, STEPS, 0, 0)             # counted under the plan, which generate removed again
    assert torch.equal(run_generate(tiny_dit, golden, 1.0, guidance_schedule=lambda i, s: 5.0), plain_runs[5.0])   # the plan's weights, not the call's
    assert torch.equal(run_generate(tiny_dit, golden, 5.0), plain_runs[5.0])
    assert tiny_dit.guidance_state(reset=True) == (False, 2 * STEPS, 0, 0)


def test_an_empty_interval_is_the_run_at_guidance_one(tiny_dit, golden, plain_runs):
    tiny_dit.guidance_state(reset=True)
    out = run_generate(tiny_dit, golden, 5.0, guidance_interval=(0.0, 0.0))
    assert torch.equal(out, plain_runs[1.0])
    assert tiny_dit.guidance_state(reset=True) == (False, 0, STEPS, 0)


@pytest.mark.parametrize("name", list(PLANS))
def test_fused_equals_stepwise(tiny_dit, golden, plain_runs, name):
    tiny_dit.guidance_state(reset=True)
    a = run_generate(tiny_dit, golden, 5.0, **PLANS[name])
    counts = tiny_dit.guidance_state(reset=True)
    b = run_generate(Wrapped(tiny_dit), golden, 5.0, **PLANS[name])
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert rel(a, plain_runs[5.0]) > 1e-3                                # the plan did something
    want = {"schedule": (6, 0, 0), "interval": (4, 2, 0), "zero_star_init": (5, 0, 1), "rescale": (6, 0, 0), "all": (4, 1, 1)}[name]
    assert counts == (False,) + want


def without_zero_init(plan):
    return {k: v for k, v in plan.items() if k != "cfg_zero_init"}


class Recorder:
    def __init__(self):
        self.seen = []

    def __call__(self, info):
        self.seen.append(NS(step=info.step, preview=None if info.preview is None else info.preview.clone(),
                            x0=None if info.x0 is None else info.x0.clone()))


@pytest.mark.parametrize("name", list(PLANS))
def test_fused_equals_stepwise_with_editing_and_a_watch(tiny_dit, golden, name):
    g = torch.Generator().manual_seed(5)
    Wf, bf = (torch.rand(16, 3, generator=g) - 0.5) * 0.5, (torch.rand(3, generator=g) - 0.5) * 0.4
    src, mask = source_latent(), edit_mask()
    plan = without_zero_init(PLANS[name])                                # zero-init with editing is refused
    kw = dict(init_latent=src, strength=1.0, keep_mask=mask, **plan)
    bare = run_generate(tiny_dit, golden, 5.0, **kw)
    recs, outs = [], []
    for model in (tiny_dit, Wrapped(tiny_dit)):
        rec = Recorder()
        outs.append(run_generate(model, golden, 5.0, callback=rec, preview_every=1, preview_factors=(Wf, bf), preview_x0=True, **kw))
        recs.append(rec)
    assert torch.equal(outs[0], bare)                                    # the watch (and the v it asks the update to leave) moves no bit
    assert torch.equal(outs[0], outs[1])
    keep = (mask == 1).expand_as(src)
    assert torch.equal(bare.cpu()[keep], src[keep])
    assert len(recs[0].seen) == len(recs[1].seen) == STEPS
    for a, c in zip(recs[0].seen, recs[1].seen):
        assert a.step == c.step and torch.equal(a.preview, c.preview) and torch.equal(a.x0, c.x0)
    # ... and without editing, zero-init included: the preview of a zero step is the latent itself
    recs, outs = [], []
    for model in (tiny_dit, Wrapped(tiny_dit)):
        rec = Recorder()
        outs.append(run_generate(model, golden, 5.0, callback=rec, preview_every=1, preview_factors=(Wf, bf), preview_x0=True, **PLANS[name]))
        recs.append(rec)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], run_generate(tiny_dit, golden, 5.0, **PLANS[name]))
    for a, c in zip(recs[0].seen, recs[1].seen):
        assert torch.equal(a.preview, c.preview) and torch.equal(a.x0, c.x0)
    if PLANS[name].get("cfg_zero_init"):
        assert torch.equal(recs[0].seen[0].x0.cpu(), golden["gen.noise"])


UNIFORM = {"constant": dict(guidance_schedule=[3.0] * STEPS), "schedule": dict(guidance_schedule=SCHEDULE),
           "zero_star_rescale_schedule": dict(guidance_schedule=SCHEDULE, cfg_zero_star=True, cfg_rescale=0.7),
           "rescale": dict(cfg_rescale=1.0), "unguided": dict(guidance_interval=(0.0, 0.0))}


def test_the_captured_step_equals_the_eager_run(tiny_dit, cfg, tiny_sd, golden):
    gdit = make_dit(cfg, tiny_sd)
    gdit.engine("cuda:0")
    gdit.set_graph(True)
    mask_kw = dict(init_latent=source_latent(), keep_mask=edit_mask())
    for name, plan in list(UNIFORM.items()) + [("mixed", PLANS["interval"]), ("mixed_all", PLANS["all"])]:
        eager = run_generate(tiny_dit, golden, 5.0, **plan)
        assert torch.equal(run_generate(gdit, golden, 5.0, **plan), eager), name
        if "cfg_zero_init" not in plan:
            assert torch.equal(run_generate(gdit, golden, 5.0, **plan, **mask_kw), run_generate(tiny_dit, golden, 5.0, **plan, **mask_kw)), name
    gdit._destroy_engine(force=True)


def test_zero_init_leaves_the_noise(tiny_dit, golden):
    tiny_dit.guidance_state(reset=True)
    out = run_generate(tiny_dit, golden, 5.0, steps=1, cfg_zero_star=True, cfg_zero_init=1)
    assert torch.equal(out.cpu(), golden["gen.noise"])
    assert tiny_dit.guidance_state(reset=True) == (False, 0, 0, 1)
    assert torch.equal(run_generate(Wrapped(tiny_dit), golden, 5.0, steps=1, cfg_zero_star=True, cfg_zero_init=1).cpu(), golden["gen.noise"])
    out = run_generate(tiny_dit, golden, 5.0, steps=3, cfg_zero_init=5)   # more than the run has: every step is a zero step
    assert torch.equal(out.cpu(), golden["gen.noise"])
    assert tiny_dit.guidance_state(reset=True) == (False, 0, 0, 3)


def test_magcache_with_a_uniform_plan(cfg, tiny_sd, golden):
    from kandinsky.generation_utils import generate
    from kandinsky.magcache_utils import set_magcache_params, disable_magcache, magcache_state
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    te, ne = prompts(golden)
    n = c["num_steps"]
    args = ("cuda:0", SHAPE, n, te, ne, POS, torch.arange(7), torch.arange(4), c["guidance_weight"], c["scheduler_scale"], FLASH)
    plan = dict(guidance_schedule=[c["guidance_weight"] + 0.1 * i for i in range(n)], cfg_zero_star=True, cfg_rescale=0.7)
    try:
        set_magcache_params(dit, c["ratios"], n, c["no_cfg"])
        out = generate(dit, *args, noise=golden["gen.noise"], **plan)
        _, ran, skipped = magcache_state(dit)
        assert skipped > 0 and ran > 0
        assert dit.guidance_state(reset=True) == (False, n, 0, 0)
        with pytest.raises(ValueError, match="MagCache"):
            generate(dit, *args, noise=golden["gen.noise"], cfg_zero_init=1)
    finally:
        disable_magcache(dit)
    assert torch.isfinite(out).all()
    assert rel(out, generate(dit, *args, noise=golden["gen.noise"], **plan)) > 1e-4     # the cache was really applied
    dit._destroy_engine(force=True)


# ------------------------------------------------------------------------------------------ parity
@pytest.fixture(scope="module")
def guidance_golden():
    from safetensors.torch import load_file
    return (load_file(os.path.join(GOLDEN, "dit_tiny_guidance.safetensors")),
            json.load(open(os.path.join(GOLDEN, "dit_tiny_guidance_meta.json"))))


@pytest.mark.parametrize("name", list(PLANS))
def test_parity_with_the_oracle_and_the_reference_golden(tiny_dit, tiny_sd, cfg, golden, guidance_golden, name):
    gold, meta = guidance_golden
    case = meta["cases"][name]
    assert (meta["steps"], meta["scheduler_scale"], meta["guidance_weight"]) == (STEPS, 5.0, 5.0)
    plan = PLANS[name]
    assert (case.get("schedule"), tuple(case["interval"]) if "interval" in case else None, case.get("zero_star", False), case.get("zero_init", 0),
            case.get("rescale", 0.0)) == (plan.get("guidance_schedule"), plan.get("guidance_interval"), plan.get("cfg_zero_star", False),
                                          plan.get("cfg_zero_init", 0), plan.get("cfg_rescale", 0.0))
    out = run_generate(tiny_dit, golden, 5.0, **plan)
    ocfg = O.DitConfig(**cfg)
    noise = golden["gen.noise"]
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)

    def vel(text, pooled, tpos):
        return lambda x, s: O.dit_forward(tiny_sd, ocfg, torch.cat([x, *zeros], -1), golden[text], golden[pooled], s.unsqueeze(0) * 1000, POS,
                                          tpos, (1.0, 2.0, 2.0), None, "bf16")
    ref16 = R.bf16_loop(vel("fwd.text", "fwd.pooled", torch.arange(7)), vel("gen.null_text", "gen.null_pooled", torch.arange(4)), noise,
                        O.sigma_schedule(STEPS, 5.0), case["weights"], case.get("zero_star", False), case.get("zero_init", 0),
                        case.get("rescale", 0.0))
    r16, r32 = rel(out, ref16), rel(out, gold[f"guidance.{name}.final"])
    print(f"guidance {name}: engine vs bf16 oracle {r16:.3e}, vs reference golden {r32:.3e}")
    assert r16 <= 1e-2, r16
    assert r32 <= 3e-2, r32


# ------------------------------------------------------------------------------------------ ranks


@pytest.mark.timeout(600)
def test_loopback_ranks_with_a_mixed_plan(tiny_sd, cfg):
    from test_gpu_loopback import run_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne = _sp_case()[:4]
    pos = [torch.arange(8)] * 3
    plan = dict(guidance_interval=(0.6, 0.95), cfg_zero_star=True, cfg_rescale=0.7)     # 4 steps of scale 5: sigmas 1, .938, .833, .625

    def call(d, r):
        out = generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, **plan)
        assert d.guidance_state() == (False, 3, 1, 0)
        return out

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    fused = call(make(), 0)
    outs = run_ranks(2, make, call)
    assert torch.equal(outs[1], outs[0])
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)


@pytest.mark.timeout(900)
def test_cfg_pair_in_the_engine_with_a_uniform_plan(tiny_sd, cfg):
    from test_gpu_loopback import run_cfg_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne = _sp_case()[:4]
    pos = [torch.arange(8)] * 3
    plan = dict(guidance_schedule=[5.0, 4.0, 3.0, 2.0], cfg_zero_star=True, cfg_rescale=0.7)

    def call(d, i):
        return generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, **plan)

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    fused = call(make(), 0)
    outs = run_cfg_ranks(1, make, call)
    assert torch.equal(outs[1], outs[0]), "the two handles of the pair differ"
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(tiny_dit, cfg, tiny_sd, golden):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import context_windows, sigma_schedule
    from kandinsky.magcache_utils import set_magcache_params, disable_magcache
    te, ne = prompts(golden)
    lat = golden["gen.noise"].cuda().contiguous()
    before = lat.clone()
    src, eps = source_latent().cuda(), golden["gen.noise"].cuda().contiguous()

    def refused(d, status, word, steps=2, w=5.0, pos=POS, **kw):
        state = d.guidance_state()
        with pytest.raises(RuntimeError, match=f"status {status}") as e:
            d.sample(lat, sigma_schedule(steps, 5.0).tolist(), te, ne, pos, torch.arange(7), torch.arange(4), w, scale_factor=(1.0, 2.0, 2.0), **kw)
        assert word in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(lat, before) and d.guidance_state() == state

    tiny_dit.guidance_state(reset=True)
    try:
        tiny_dit.set_guidance([5.0, 4.0, 3.0])
        refused(tiny_dit, K5_ERR_ARG, "3 weights")                                       # num_weights != num_steps
        tiny_dit.set_guidance([1.0, 1.0], zero_star=True)
        refused(tiny_dit, K5_ERR_ARG, "nothing to guide")                                # zero_star at a call whose every weight is 1
        tiny_dit.set_guidance(None, rescale=0.5)
        refused(tiny_dit, K5_ERR_ARG, "nothing to guide", w=1.0)
        tiny_dit.set_guidance(None, zero_init_steps=1)
        refused(tiny_dit, K5_ERR_UNSUPPORTED, "editing", edit=(src, eps, None))          # zero-init together with editing
        starts, weights = context_windows(3, 2, 1)
        for plan in (dict(weights=[5.0, 4.0]), dict(rescale=0.5), dict()):               # any plan with context windows
            tiny_dit.set_guidance(**plan)
            refused(tiny_dit, K5_ERR_STATE, "window", pos=[torch.arange(2), POS[1], POS[2]], windows=(starts, weights))
    finally:
        tiny_dit.clear_guidance()
    assert tiny_dit.guidance_state() == (False, 0, 0, 0)

    # a mixed or zero-init plan with MagCache, and on a CFG pair (a handle of its own each: the refusal comes before any exchange)
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    n = c["num_steps"]
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    set_magcache_params(dit, c["ratios"], n, c["no_cfg"])
    try:
        for plan in (dict(weights=[5.0] * (n - 1) + [1.0]), dict(zero_init_steps=1)):
            dit.set_guidance(**plan)
            refused(dit, K5_ERR_STATE, "MagCache", steps=n)
    finally:
        disable_magcache(dit)
    dit._destroy_engine(force=True)
    pair = make_dit(cfg, tiny_sd)
    pair.engine("cuda:0")
    group = E.LoopbackGroup(2)
    pair.enable_cfg_pair_loopback(group, 0)
    for plan in (dict(weights=[5.0, 1.0]), dict(zero_init_steps=1)):
        pair.set_guidance(**plan)
        refused(pair, K5_ERR_STATE, "CFG pair")
    pair._destroy_engine(force=True)

    # the C entry point itself, and that a refused call is no state: the next plain call runs
    assert E.lib().k5_dit_set_guidance(tiny_dit.engine(lat.device), C.byref(E.Guidance(None, 0, 0, 0, 2.0))) == K5_ERR_ARG
    assert b"rescale" in E.lib().k5_last_error() and tiny_dit.guidance_state()[0] is False
    torch.cuda.synchronize()
    assert torch.equal(lat, before)
