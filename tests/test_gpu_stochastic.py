"""Stochastic sampling on the MI355X: the in-kernel Philox4x32-10 generator bit for bit against its NumPy restatement, its normals against the
float64 restatement and a few moments, the stochastic update bit for bit against separate fp32 ops in torch eager and against the existing
entries where no noise is drawn, k5_sample* with a plan through the modes of the fused sampler (the plain run's bits where the plan is off,
the per-step loop's bits everywhere), graph replay, rank groups, parity with the bf16 oracle loop and the reference's golden, and every refusal.

The model, shape, steps and prompts are those of tests/test_gpu_guidance.py.  Tolerances are the project's: a final latent within relative L2
1e-2 of the bf16-island oracle loop and 3e-2 of the reference's fp32 golden (tools/gen_golden_stochastic.py).  Everything that claims "the same
computation" is asserted bit for bit.

The bound on the normals, 1e-5 absolute against float64, is derived and not measured: |z| <= 5.8 (u >= 2^-24); the angle 2 pi u1 of the
float64 side has no fp32 counterpart (sincospif takes 2 u1 exactly) but the radius and the two factors each carry a few fp32 ulp of log, sqrt,
sin / cos and the final product, 5.8 * a few * 6e-8 ~ 2e-6, and near u0 -> 1 the log's absolute error of ~1 ulp(1e-7) under the square root
adds the same order: about 4e-6 in all, capped at 1e-5.  Measured on the MI355X: 6.4e-7 at n = 2^20 (the test prints it)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402

import stochastic_reference as SR  # noqa: E402
import kit  # noqa: E402
from kit import (GOLDEN, K5_ERR_ARG, K5_ERR_STATE, POS, _sp_case, cfg, edit_mask,  # noqa: E402
                 f32, flash_conf, make_dit, need_gpu, prompts, rel, source_latent, tiny_dit)

FLASH = flash_conf()
BF = torch.bfloat16
SHAPE = (3, 8, 12, 16)
STEPS = 6
INTERVAL = (0.6, 0.97)      # of the sigmas 1, .962, .909, .833, .714, .5 (6 steps, scale 5) steps 1..4 lie inside
SEED = 6554
CASES = {"eta1_cfg": (5.0, dict(eta=1.0)),
         "eta_half_interval_nocfg": (1.0, dict(eta=0.5, sde_interval=INTERVAL)),
         "eta1_zero_star_skip": (5.0, dict(eta=1.0, cfg_zero_star=True, slg_blocks=[1], slg_scale=2.0))}
NOISY = {"eta1_cfg": 5, "eta_half_interval_nocfg": 4, "eta1_zero_star_skip": 5}


def u32(t):
    """an int32 tensor of bit patterns as a uint32 array"""
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------ raw words


@pytest.mark.parametrize("blk0, seed, c2, c3, want", [
    (0, 0, 0, 0, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    (2 ** 64 - 1, 2 ** 64 - 1, 0xffffffff, 0xffffffff, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    (0x85a308d3243f6a88, 0x299f31d0a4093822, 0x13198a2e, 0x03707344, "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_words_known_answers(blk0, seed, c2, c3, want):
    need_gpu()
    from kandinsky import _engine as E
    w = u32(E.philox_words(blk0, 1, seed, c2, c3))
    assert " ".join("%08x" % int(x) for x in w[0]) == want


def test_philox_words_equal_the_restatement_across_the_carry():
    need_gpu()
    from kandinsky import _engine as E
    blk0, n = 2 ** 32 - 7, 4096                                          # crosses the carry into the high counter word
    got = u32(E.philox_words(blk0, n, SEED, 3, 0))
    assert np.array_equal(got, SR.philox_words(blk0, n, SEED, 3, 0))
    assert np.array_equal(u32(E.philox_words(2 ** 64 - 2, 4, SEED))[2:], SR.philox_words(0, 2, SEED))   # the block index wraps mod 2^64


# ------------------------------------------------------------------------------------------ normals
def gpu_normals(n, seed, stream=0, pad=64):
    from kandinsky import _engine as E
    buf = torch.full((n + pad,), 7.0, device="cuda")                     # poisoned: nothing past n may be written
    E.noise_normal_(buf, seed, stream, n=n)
    torch.cuda.synchronize()
    assert (buf[n:] == 7.0).all()
    return buf[:n]


@pytest.fixture(scope="module")
def big_normals():
    """2^20 normals of seed 6554, stream 0, from the GPU and from the float64 restatement: computed once, left unchanged"""
    need_gpu()
    n = 2 ** 20
    return gpu_normals(n, SEED).cpu().numpy().astype(np.float64), SR.normals_f64(n, SEED)


@pytest.mark.parametrize("n", [1, 3, 4, 1023])
def test_normals_agree_with_float64_small(n):
    need_gpu()
    z = gpu_normals(n, SEED, 2).cpu().numpy().astype(np.float64)
    err = np.abs(z - SR.normals_f64(n, SEED, 2)).max()
    print(f"normals n={n}: max |fp32 - float64| = {err:.3e}")
    assert err <= 1e-5, err


def test_normals_agree_with_float64_big(big_normals):
    z, ref = big_normals
    err = np.abs(z - ref).max()
    print(f"normals n=2^20: max |fp32 - float64| = {err:.3e} (|z| max {np.abs(ref).max():.3f})")
    assert np.isfinite(z).all()
    assert err <= 1e-5, err
    again = gpu_normals(2 ** 20, SEED).cpu().numpy().astype(np.float64)
    assert np.array_equal(again, z)                                      # two launches, equal bits
    # the launcher caps its grid at 1024 workgroups of 256 threads, a block of four normals each: past 2^20 the stride loop runs twice
    n = 2 ** 20 + 4099
    z2 = gpu_normals(n, SEED).cpu().numpy().astype(np.float64)
    assert np.array_equal(z2[:2 ** 20], z)
    assert np.abs(z2[2 ** 20:] - SR.normals_f64(n, SEED)[2 ** 20:]).max() <= 1e-5


def test_normals_statistics(big_normals):
    z, _ = big_normals
    n = z.size
    se = 2.0 ** -10                                                      # 1 / sqrt(n)
    other_stream = gpu_normals(n, SEED, 1).cpu().numpy().astype(np.float64)
    other_seed = gpu_normals(n, SEED + 1).cpu().numpy().astype(np.float64)
    stats = {"mean": z.mean(), "variance": (z.var() - 1.0) / np.sqrt(2.0), "fourth moment": ((z ** 4).mean() - 3.0) / np.sqrt(96.0),
             "lag 1": (z[1:] * z[:-1]).mean(), "lag 4": (z[4:] * z[:-4]).mean(), "stream 1": (z * other_stream).mean(),
             "seed 6555": (z * other_seed).mean()}
    for name, v in stats.items():
        print(f"normals {name}: {v / se:+.2f} se")
    for name, v in stats.items():
        assert abs(v) <= 4 * se, (name, v / se)


# ------------------------------------------------------------------------------------------ the update
def update_inputs(dims, seed):
    n, cells = int(np.prod(dims)), int(np.prod(dims[:-1]))
    g = torch.Generator().manual_seed(seed)
    img, x0, eps, z = (torch.randn(n, generator=g).cuda() * k for k in (1.0, 3.0, 1.0, 1.0))
    c, u, s = (torch.randn(n, generator=g).cuda().to(BF) for _ in range(3))
    mask = torch.tensor([0.0, 1.0, 0.25])[torch.randint(0, 3, (cells,), generator=g)].cuda()
    assert all((mask == v).any() for v in (0.0, 1.0, 0.25))
    return img, x0, eps, z, c, u, s, mask


def launch(img, c, u=None, s=None, w=1.0, abd=None, g=0.0, dt=-0.1, x0=None, eps=None, mask=None, sigma=0.0, cells=None, Cc=16, scale=1.0,
           coef=0.0, z=None, seed=0, stream=0):
    """the raw entry on guarded buffers; returns (status, latent)"""
    from kandinsky import _engine as E
    n = img.numel()
    buf = torch.full((n + 64,), 7.0, device="cuda")
    buf[:n] = img
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    cells = n // max(Cc, 1) if cells is None else cells
    st = E.lib().k5_stochastic_euler(buf.data_ptr(), p(c), p(u), p(s), w, p(abd), g, dt, p(x0), p(eps), p(mask), sigma, cells, Cc, None, scale, coef,
                                     p(z), seed, stream, E.stream_ptr())
    torch.cuda.synchronize()
    assert (buf[n:] == 7.0).all()
    return st, buf[:n]


FORMS = ["plain", "cfg", "ab", "skip", "skip_ab"]


@pytest.mark.parametrize("dims", [(3, 8, 12, 16), (5, 10, 14, 16)])
@pytest.mark.parametrize("sigma", [0.0, 0.37])
@pytest.mark.parametrize("form", FORMS)
def test_stochastic_euler_bit_exact(dims, sigma, form):
    need_gpu()
    from kandinsky import _engine as E
    n, cells, Cc = int(np.prod(dims)), int(np.prod(dims[:-1])), dims[-1]
    img, x0, eps, z, c, u, s, mask = update_inputs(dims, n + len(form))
    w, g, dt = f32(4.3), f32(2.3), f32(-0.0625 * 1.3)
    scale, coef = f32(0.7368421), f32(0.5537940)
    al, be = f32(2.2), f32(-1.3137)
    abd = torch.tensor([al, be], dtype=torch.float32, device="cuda") if form in ("ab", "skip_ab") else None
    uu = None if form in ("plain", "skip") else u
    ss = s if form in ("skip", "skip_ab") else None
    gg = g if ss is not None else 0.0
    ab = (al, be) if abd is not None else None
    m = mask.repeat_interleave(Cc)
    common = dict(u=uu, s=ss, w=w, abd=abd, g=gg, dt=dt, Cc=Cc)
    edit = dict(x0=x0, eps=eps, mask=mask, sigma=sigma)

    def want(zz, coef_, keep):   # torch eager, every fp32 op on its own (the GPU's eager ops round exactly like that)
        x, _ = SR.stochastic_update(img, c, uu, ss, w, gg, dt, scale, coef_, zz, ab, x0 if keep else None, eps if keep else None, m if keep else None,
                                    sigma)
        return x

    # given noise, with and without the keep mask
    for keep in (False, True):
        st, out = launch(img, c, scale=scale, coef=coef, z=z, **common, **(edit if keep else {}))
        assert st == 0, E.last_error()
        assert torch.equal(out, want(z, coef, keep)), (form, keep)
        if keep and sigma == 0.0:
            assert torch.equal(out[m == 1], x0[m == 1])                   # kept cells at sigma_next 0 are the source
    # the host restatement on the CPU gives the same bits as the eager ops on the GPU
    hx, _ = SR.stochastic_update(img.cpu(), c.cpu(), None if uu is None else u.cpu(), None if ss is None else s.cpu(), w, gg, dt, scale, coef, z.cpu(),
                                 ab, x0.cpu(), eps.cpu(), m.cpu(), sigma)
    assert torch.equal(hx, want(z, coef, True).cpu())
    # noise = NULL: the generator's values, the same call fed k5_noise_normal_f32
    zg = torch.empty(n, device="cuda")
    E.noise_normal_(zg, SEED + 1, 5)
    st, a = launch(img, c, scale=scale, coef=coef, z=None, seed=SEED + 1, stream=5, **common, **edit)
    st2, b = launch(img, c, scale=scale, coef=coef, z=zg, **common, **edit)
    assert st == 0 and st2 == 0 and torch.equal(a, b) and torch.equal(a, want(zg, coef, True))
    assert not torch.equal(a, launch(img, c, scale=scale, coef=coef, z=None, seed=SEED + 1, stream=6, **common, **edit)[1])
    # noise_coef = 0: the matching existing entry, bit for bit (scale is not applied)
    st, out0 = launch(img, c, scale=scale, coef=0.0, z=None, seed=3, **common, **edit)
    assert st == 0
    ref = img.clone()
    L, sp = E.lib(), E.stream_ptr()
    if form == "plain" or form == "cfg":
        L.k5_cfg_euler_edit(ref.data_ptr(), c.data_ptr(), None if uu is None else u.data_ptr(), w, dt, x0.data_ptr(), eps.data_ptr(), mask.data_ptr(),
                            sigma, cells, Cc, sp)
    elif form == "ab":
        L.k5_guided_euler(ref.data_ptr(), c.data_ptr(), u.data_ptr(), abd.data_ptr(), dt, x0.data_ptr(), eps.data_ptr(), mask.data_ptr(), sigma, cells,
                          Cc, None, sp)
    else:
        L.k5_skip_euler(ref.data_ptr(), c.data_ptr(), None if uu is None else u.data_ptr(), s.data_ptr(), w, None if abd is None else abd.data_ptr(),
                        g, dt, x0.data_ptr(), eps.data_ptr(), mask.data_ptr(), sigma, cells, Cc, None, sp)
    torch.cuda.synchronize()
    assert torch.equal(out0, ref)
    if form in ("plain", "cfg"):                                         # ... and without a mask k5_cfg_euler
        st, out0 = launch(img, c, scale=scale, coef=0.0, **common)
        ref = img.clone()
        E.cfg_euler_(ref, c, uu, w, dt)
        assert st == 0 and torch.equal(out0, ref)


def test_stochastic_euler_tail_and_helper():
    """n % 4 != 0: the thread of the last, partial generator block updates exactly its elements; the Python helper is the entry"""
    need_gpu()
    from kandinsky import _engine as E
    for n in (1, 3, 4, 1023, 4 * 256 * 3 + 2):
        g = torch.Generator().manual_seed(n)
        img, c = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda().to(BF)
        zg = torch.empty(n, device="cuda")
        E.noise_normal_(zg, 9, 1)
        st, out = launch(img, c, dt=f32(-0.3), Cc=1, scale=f32(0.9), coef=f32(0.4), seed=9, stream=1)
        assert st == 0, E.last_error()
        x, _ = SR.stochastic_update(img, c, None, None, 1.0, 0.0, f32(-0.3), f32(0.9), f32(0.4), zg)
        assert torch.equal(out, x), n
        helper = img.clone().view(n, 1)
        E.stochastic_euler_(helper, c.view(n, 1), None, 1.0, f32(-0.3), f32(0.9), f32(0.4), 9, 1)
        assert torch.equal(helper.view(-1), x)


def test_stochastic_euler_refusals_launch_nothing():
    need_gpu()
    from kandinsky import _engine as E
    dims = (3, 8, 12, 16)
    img, x0, eps, z, c, u, s, mask = update_inputs(dims, 9)
    abd = torch.tensor([2.0, -1.0], dtype=torch.float32, device="cuda")

    def refused(**kw):
        a = dict(u=u, s=s, w=5.0, g=3.0, dt=-0.1, x0=x0, eps=eps, mask=mask, sigma=0.5, scale=0.7, coef=0.5, z=z)
        a.update(kw)
        st, out = launch(img, c, **a)
        assert st == K5_ERR_ARG and "k5_stochastic_euler" in E.last_error()
        assert torch.equal(out, img)                                     # the latent is as it was

    for g in (0.0, -1.0, float("nan"), float("inf")):
        refused(g=g)                                                      # the refusals of k5_skip_euler: v_skip without a finite g > 0 ...
    refused(s=None, g=3.0)                                                # ... a g without v_skip
    refused(u=None, abd=abd)                                              # ab without v_uncond
    refused(cells=0)
    refused(Cc=0)
    refused(x0=None)                                                      # a keep_mask without source
    for scale in (float("nan"), float("inf"), -float("inf")):
        refused(scale=scale)
    for coef in (-0.5, -0.0 - 1e-30, float("nan"), float("inf")):
        refused(coef=coef)
    assert E.lib().k5_stochastic_euler(None, c.data_ptr(), None, None, 1.0, None, 0.0, -0.1, None, None, None, 0.5, 288, 16, None, 1.0, 0.5, None, 1, 0,
                                       E.stream_ptr()) == K5_ERR_ARG
    # a refused call left no state: the plain entry's bits are the eager expression
    out = img.clone()
    E.cfg_euler_(out, c, u, 5.0, -0.1)
    assert torch.equal(out, img + (f32(-0.1) * (u + 5.0 * (c - u)).float()).to(BF).float())


# ------------------------------------------------------------------------------------------ the tiny model


def run_generate(model, golden, w=5.0, steps=STEPS, **kw):
    return kit.run_generate(model, golden, w, steps=steps, shape=SHAPE, pos=POS, **kw)


Wrapped = functools.partial(kit.Wrapped, blocks=True,          # this one can fork
                            hand_on=("forward_skip", "set_skip_guidance", "clear_skip_guidance", "_skip"))


@pytest.fixture(scope="module")
def plain_runs(tiny_dit, golden):
    """the runs without a plan that the tests below compare against, each computed once"""
    return {w: run_generate(tiny_dit, golden, w) for w in (1.0, 5.0)}


@pytest.fixture(scope="module")
def fused_runs(tiny_dit, golden):
    """the three cases through the fused loop with their noisy-step counts, each computed once"""
    out = {}
    for name, (w, kw) in CASES.items():
        tiny_dit.stochastic_state(reset=True)
        lat = run_generate(tiny_dit, golden, w, sde_seed=SEED, **kw)
        out[name] = (lat, tiny_dit.stochastic_state(reset=True))
    return out


def test_eta_zero_and_an_empty_interval_are_the_plain_run(tiny_dit, golden, plain_runs):
    tiny_dit.stochastic_state(reset=True)
    for w in (1.0, 5.0):
        assert torch.equal(run_generate(tiny_dit, golden, w, eta=0.0, s_noise=2.0, sde_seed=3), plain_runs[w])
        assert torch.equal(run_generate(tiny_dit, golden, w, eta=1.0, sde_interval=(2.0, 3.0)), plain_runs[w])
    assert tiny_dit.stochastic_state() == (False, 0)
    # a plan whose every step is without noise goes through the stochastic instantiation and still gives the plain run's bits
    from kandinsky.generation_utils import sigma_schedule, stochastic_plan
    tiny_dit.set_stochastic(*stochastic_plan(sigma_schedule(STEPS, 5.0).tolist(), 0.0), seed=1)
    try:
        assert tiny_dit.stochastic_state() == (True, 0)
        assert torch.equal(run_generate(tiny_dit, golden, 5.0), plain_runs[5.0])
        assert tiny_dit.stochastic_state() == (True, 0)
    finally:
        tiny_dit.clear_stochastic()


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_stepwise_and_counts(tiny_dit, golden, plain_runs, fused_runs, name):
    w, kw = CASES[name]
    a, state = fused_runs[name]
    assert state == (False, NOISY[name])                                 # counted under the plan, which generate removed again
    b = run_generate(Wrapped(tiny_dit), golden, w, sde_seed=SEED, **kw)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert rel(a, plain_runs[w]) > 1e-2                                  # the noise did something


def test_seeds(tiny_dit, golden, fused_runs):
    again = run_generate(tiny_dit, golden, 5.0, sde_seed=SEED, eta=1.0)
    assert torch.equal(again, fused_runs["eta1_cfg"][0])                 # two runs with one seed are equal
    other = run_generate(tiny_dit, golden, 5.0, sde_seed=SEED + 1, eta=1.0)
    assert rel(other, again) > 1e-2                                      # two seeds differ
    assert torch.equal(run_generate(tiny_dit, golden, 5.0, seed=SEED, eta=1.0), again)   # sde_seed defaults to seed


def test_fused_equals_stepwise_with_editing_and_a_progress_watch(tiny_dit, golden):
    src, mask = source_latent(), edit_mask()
    for name, strength in (("eta1_cfg", 1.0), ("eta1_zero_star_skip", 0.5)):
        w, kw = CASES[name]
        kw = dict(kw, sde_seed=SEED, init_latent=src, strength=strength, keep_mask=mask)
        bare = run_generate(tiny_dit, golden, w, **kw)
        seen, outs = [], []
        for model in (tiny_dit, Wrapped(tiny_dit)):
            steps = []
            outs.append(run_generate(model, golden, w, callback=lambda info: steps.append(info.step), **kw))
            seen.append(steps)
        assert torch.equal(outs[0], bare) and torch.equal(outs[0], outs[1])
        assert seen[0] == seen[1] and len(seen[0]) == (STEPS if strength == 1.0 else 3)   # progress, step by step
        keep = (mask == 1).expand_as(src)
        assert torch.equal(bare.cpu()[keep], src[keep])                  # the keep rule comes last: the source bit for bit
    # cancel still works
    from kandinsky.models.dit import SamplingInterrupted
    with pytest.raises(SamplingInterrupted) as e:
        run_generate(tiny_dit, golden, 5.0, eta=1.0, callback=lambda info: info.step == 1)
    assert 2 <= e.value.steps_done <= 3                                  # the engine runs at most one step ahead of the callback


def test_the_captured_step_equals_the_eager_run(tiny_dit, cfg, tiny_sd, golden, fused_runs):
    gdit = make_dit(cfg, tiny_sd)
    gdit.engine("cuda:0")
    gdit.set_graph(True)
    mask_kw = dict(init_latent=source_latent(), keep_mask=edit_mask())
    for name, (w, kw) in CASES.items():
        gdit.stochastic_state(reset=True)
        assert torch.equal(run_generate(gdit, golden, w, sde_seed=SEED, **kw), fused_runs[name][0]), name
        assert gdit.stochastic_state(reset=True) == (False, NOISY[name]), name      # right after replay
    w, kw = CASES["eta1_cfg"]
    assert torch.equal(run_generate(gdit, golden, w, sde_seed=SEED, **kw, **mask_kw), run_generate(tiny_dit, golden, w, sde_seed=SEED, **kw, **mask_kw))
    gdit._destroy_engine(force=True)


def test_visual_cond_nag_and_regions(tiny_dit, golden):
    """the plan in the other modes of the fused loop: fused equals stepwise"""
    g = torch.Generator().manual_seed(4)
    vc, vm = torch.randn(*SHAPE, generator=g), torch.zeros(*SHAPE[:-1], 1)
    vm[0] = 1.0
    masks = torch.zeros(1, *SHAPE[:-1])
    masks[0, :, :, :6] = 1.0
    te, ne = prompts(golden)
    modes = {"visual_cond": dict(visual_cond=vc, visual_cond_mask=vm),
             "nag": dict(nag_scale=4.0, nag_text_embeds=ne, nag_text_rope_pos=torch.arange(4)),
             "regions": dict(region_text_embeds=[{"text_embeds": ne["text_embeds"]}], region_text_rope_pos=[torch.arange(4)], region_masks=masks)}
    for name, kw in modes.items():
        w = 1.0 if name == "nag" else 5.0
        a = run_generate(tiny_dit, golden, w, eta=1.0, sde_seed=SEED, **kw)
        if name == "visual_cond":
            b = run_generate(Wrapped(tiny_dit), golden, w, eta=1.0, sde_seed=SEED, **kw)
            assert torch.equal(a, b), name
        assert torch.isfinite(a).all() and rel(a, run_generate(tiny_dit, golden, w, **kw)) > 1e-2, name
        assert torch.equal(a, run_generate(tiny_dit, golden, w, eta=1.0, sde_seed=SEED, **kw)), name


# ------------------------------------------------------------------------------------------ parity
@pytest.fixture(scope="module")
def stochastic_golden():
    from safetensors.torch import load_file
    return (load_file(os.path.join(GOLDEN, "dit_tiny_stochastic.safetensors")),
            json.load(open(os.path.join(GOLDEN, "dit_tiny_stochastic_meta.json"))))


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_oracle_and_the_reference_golden(tiny_sd, cfg, golden, stochastic_golden, fused_runs, name):
    import skip_reference as S
    gold, meta = stochastic_golden
    case = meta["cases"][name]
    w, kw = CASES[name]
    assert (meta["steps"], meta["scheduler_scale"], meta["seed"]) == (STEPS, 5.0, SEED)
    assert (case["w"], case["eta"], tuple(case["interval"]) if "interval" in case else None, case.get("zero_star", False), case.get("blocks"),
            case.get("g", 0.0)) == (w, kw["eta"], kw.get("sde_interval"), kw.get("cfg_zero_star", False), kw.get("slg_blocks"), kw.get("slg_scale", 0.0))
    out = fused_runs[name][0]
    ocfg = O.DitConfig(**cfg)
    noise = golden["gen.noise"]
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)
    sig = O.sigma_schedule(STEPS, 5.0)

    def vel(text, pooled, tpos, skip=()):
        return lambda x, s: S.dit_forward_skip(tiny_sd, ocfg, torch.cat([x, *zeros], -1), golden[text], golden[pooled], s.unsqueeze(0) * 1000, POS,
                                               tpos, (1.0, 2.0, 2.0), None, "bf16", skip, "block")
    blocks = case.get("blocks")
    ref16 = SR.bf16_loop(vel("fwd.text", "fwd.pooled", torch.arange(7)), vel("gen.null_text", "gen.null_pooled", torch.arange(4)),
                         vel("fwd.text", "fwd.pooled", torch.arange(7), blocks or ()), noise, sig, [w] * STEPS,
                         SR.tables_f32(sig.tolist(), case["eta"], 1.0, case.get("interval")), SR.step_noise(SHAPE, SEED), case.get("g", 0.0),
                         [1] * STEPS if blocks else None, case.get("zero_star", False))
    r16, r32 = rel(out, ref16), rel(out, gold[f"stochastic.{name}.final"])
    print(f"stochastic {name}: engine vs bf16 oracle {r16:.3e}, vs reference golden {r32:.3e}")
    assert r16 <= 1e-2, r16
    assert r32 <= 3e-2, r32


# ------------------------------------------------------------------------------------------ ranks


@pytest.mark.timeout(600)
def test_loopback_ranks(tiny_sd, cfg):
    from test_gpu_loopback import run_ranks
    from kandinsky.generation_utils import generate
    need_gpu()
    shape, noise, te, ne = _sp_case()[:4]
    pos = [torch.arange(8)] * 3

    def call(d, r):
        out = generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, eta=1.0, sde_seed=SEED)
        assert d.stochastic_state() == (False, 3)
        return out

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    fused = call(make(), 0)
    outs = run_ranks(2, make, call)
    assert torch.equal(outs[1], outs[0])                                 # the same seed, the same bits, no exchange
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)


@pytest.mark.timeout(900)
def test_cfg_pair_in_the_engine(tiny_sd, cfg):
    from test_gpu_loopback import run_cfg_ranks
    from kandinsky.generation_utils import generate
    need_gpu()
    shape, noise, te, ne = _sp_case()[:4]
    pos = [torch.arange(8)] * 3

    def call(d, i):
        return generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, eta=1.0, sde_seed=SEED)

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    fused = call(make(), 0)
    outs = run_cfg_ranks(1, make, call)
    assert torch.equal(outs[1], outs[0]), "the two handles of the pair differ"
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(tiny_dit, cfg, tiny_sd, golden, plain_runs):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import context_windows, sigma_schedule, stochastic_plan
    from kandinsky.magcache_utils import set_magcache_params, disable_magcache
    te, ne = prompts(golden)
    lat = golden["gen.noise"].cuda().contiguous()
    before = lat.clone()

    def plan(steps, eta=1.0):
        return stochastic_plan(sigma_schedule(steps, 5.0).tolist(), eta)

    def refused(d, status, word, steps=2, pos=POS, call="sample", **kw):
        state = d.stochastic_state()
        with pytest.raises(RuntimeError, match=f"status {status}") as e:
            if call == "sample":
                d.sample(lat, sigma_schedule(steps, 5.0).tolist(), te, ne, pos, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0), **kw)
            else:
                d.sample_many(lat.view(1, *SHAPE), sigma_schedule(steps, 5.0).tolist(), te, ne, pos, torch.arange(7), torch.arange(4), 5.0,
                              scale_factor=(1.0, 2.0, 2.0))
        assert word in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(lat, before) and d.stochastic_state() == state

    tiny_dit.stochastic_state(reset=True)
    try:
        tiny_dit.set_stochastic(*plan(3), seed=1)
        refused(tiny_dit, K5_ERR_ARG, "3 steps")                                         # a plan of another length than the steps
        tiny_dit.set_stochastic(*plan(2), seed=1)
        starts, weights = context_windows(3, 2, 1)
        refused(tiny_dit, K5_ERR_STATE, "window", pos=[torch.arange(2), POS[1], POS[2]], windows=(starts, weights))
        refused(tiny_dit, K5_ERR_STATE, "one seed", call="sample_many")
        g = torch.Generator().manual_seed(5)
        tiny_dit.set_watch(lambda info: None, preview_every=1, rgb_factors=torch.rand(16, 3, generator=g))
        try:
            refused(tiny_dit, K5_ERR_STATE, "preview")
        finally:
            tiny_dit.clear_watch()
    finally:
        tiny_dit.clear_stochastic()
    assert tiny_dit.stochastic_state() == (False, 0)

    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    n = c["num_steps"]
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    set_magcache_params(dit, c["ratios"], n, c["no_cfg"])
    try:
        dit.set_stochastic(*plan(n), seed=1)
        refused(dit, K5_ERR_STATE, "MagCache", steps=n)
    finally:
        disable_magcache(dit)
    dit._destroy_engine(force=True)

    # the C entry point itself, and that a refused call is no state: the handle is usable and the next plain run has the plain run's bits
    bad = E.Stochastic(2, None, None, None, 1, 0)
    assert E.lib().k5_dit_set_stochastic(tiny_dit.engine(lat.device), C.byref(bad)) == K5_ERR_ARG
    assert b"num_steps" in E.lib().k5_last_error() and tiny_dit.stochastic_state()[0] is False
    torch.cuda.synchronize()
    assert torch.equal(run_generate(tiny_dit, golden, 5.0), plain_runs[5.0])
