"""Sampler progress, cancel and live x0 previews on the MI355X: the preview kernel against a float64 restatement, the watch through every mode
of the fused sampler (the final latent never moves a bit), the callback sequence, stop and exceptions, the refusals, and the pipeline's
`callback=` / `preview_every=` / `preview_factors=` end to end.

Kernel bounds (written down before the kernel ran):
  x0   |kernel - float64| <= 2^-22 (|x| + |sigma v|): two fp32 roundings (the product, the difference; one if the compiler fused them), each at
       most 2^-24 of a magnitude no larger than |x| + |sigma v|, with a factor 2 to spare.  The bf16 CFG combine is reproduced exactly in the
       reference (torch's bf16 ops round after every operation, as the kernel does).  Under a keep mask the unmasked x0 is held to that bound
       and the keep rule is then checked exactly: mask 0 = the unmasked x0, mask 1 = the source, otherwise rn(x0 + rn(m rn(source - x0))) bit
       for bit on the kernel's own x0 — stricter than a float64 bound on the blended value.
  RGB  never more than one code from the float64 value, and equal wherever float64 +- the dot-product bound
       (C + 2) 2^-24 127.5 (|b_j| + sum_k |W_kj| |x0_k|) rounds to one code."""
import ctypes as C
import functools
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kit  # noqa: E402
from kit import (GOLDEN, K5_ERR_ARG, K5_ERR_STATE, K5_ERR_UNSUPPORTED, POS, cfg,  # noqa: E402
                 edit_mask, f32, flash_conf, make_dit, need_gpu, prompts, source_latent, Wrapped)

FLASH = flash_conf()
BF = torch.bfloat16
SHAPE = (3, 8, 12, 16)


def factors(Cc=16, seed=5, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    W = (torch.rand(Cc, 3, generator=g) - 0.5) * 0.5 * scale       # |W| <= 0.25
    b = (torch.rand(3, generator=g) - 0.5) * 0.4
    return W, b


# ------------------------------------------------------------------------------------------ kernel
def preview_reference(x, c, u, w, sigma, W, b, source=None, mask=None):
    """float64 restatement: (x0 unmasked, x0 with the keep rule, value before rounding to a code, the dot-product bound), all on the CPU"""
    v = c if u is None else u + w * (c - u)                        # eager bf16: every op rounds, as cfg_velocity in small_ops.hip does
    sv = np.float64(f32(sigma)) * v.double()
    x0 = x.double() - sv
    x0_bound = 2.0 ** -22 * (x.double().abs() + sv.abs())
    x0m = x0
    if mask is not None:
        m = mask.double().reshape(*x.shape[:-1], 1)
        x0m = torch.where(m == 1, source.double(), torch.where(m == 0, x0, x0 + m * (source.double() - x0)))
    Wd, bd = W.double(), (torch.zeros(3, dtype=torch.float64) if b is None else b.double())
    val = (bd + x0m @ Wd) * 127.5 + 127.5
    bound = (x.shape[-1] + 2) * 2.0 ** -24 * 127.5 * (bd.abs() + x0m.abs() @ Wd.abs())
    return x0, x0_bound, x0m, val, bound


def codes(val):
    return torch.nan_to_num(torch.round(val), nan=0.0).clamp(0, 255)   # torch.round is round-half-even, as rint


def launch_preview(x, c, u, w, sigma, W, b, source, mask, want_x0, poison, Cc=None):
    """the raw entry point on poisoned outputs with guard bytes behind them; returns (status, rgb incl. guard, x0 incl. guard)"""
    from kandinsky import _engine as E
    cells, Cc = x.numel() // x.shape[-1], (x.shape[-1] if Cc is None else Cc)
    rgb = torch.full((cells * 3 + 64,), poison, dtype=torch.uint8, device="cuda")
    x0 = torch.full((x.numel() + 64,), float(poison), device="cuda")
    Wd, bd = W.cuda().contiguous(), (None if b is None else b.cuda().contiguous())
    st = E.lib().k5_x0_preview(x.data_ptr(), c.data_ptr(), E.ptr(u), w, sigma, E.ptr(source), E.ptr(mask), Wd.data_ptr(), E.ptr(bd),
                               x0.data_ptr() if want_x0 else None, rgb.data_ptr(), cells, Cc, E.stream_ptr())
    torch.cuda.synchronize()
    return st, rgb, x0


def kernel_case(thw, Cc, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    dims = (*thw, Cc)
    x, src = torch.randn(dims, generator=g), torch.randn(dims, generator=g) * 1.5
    c, u = torch.randn(dims, generator=g).to(BF), torch.randn(dims, generator=g).to(BF)
    cells = int(np.prod(thw))
    mask = torch.tensor([0.0, 1.0, 0.25])[torch.arange(cells) % 3][torch.randperm(cells, generator=g)].reshape(*thw, 1)
    assert all((mask == v).any() for v in (0.0, 1.0, 0.25))
    W, b = factors(Cc, seed + 1, scale)
    return x, src, c, u, mask, W, b


def check_preview(x, src, c, u, w, sigma, W, b, mask, label):
    """one launch configuration against the reference, with every assertion of the module docstring"""
    from kandinsky import _engine as E
    n, cells = x.numel(), x.numel() // x.shape[-1]
    xd, cd, ud = x.cuda(), c.cuda(), (None if u is None else u.cuda())
    sd, md = (None, None) if mask is None else (src.cuda(), mask.cuda().contiguous())
    x0, x0_bound, x0m, val, bound = preview_reference(x, c, u, w, sigma, W, b, src, mask)
    assert float(bound.max()) < 0.25, "the inputs must keep the dot-product bound far below half a code"
    runs = [launch_preview(xd, cd, ud, w, sigma, W, b, sd, md, True, p) for p in (0xA5, 0x5A)]
    for (st, rgb, out), p in zip(runs, (0xA5, 0x5A)):
        assert st == 0, (label, E.last_error())
        assert (rgb[cells * 3:] == p).all() and (out[n:] == float(p)).all(), f"{label}: guard bytes changed"
    # every output byte written: two runs over different poison agree everywhere
    assert torch.equal(runs[0][1][:cells * 3], runs[1][1][:cells * 3]) and torch.equal(runs[0][2][:n], runs[1][2][:n]), label
    rgb, out = runs[0][1][:cells * 3].cpu().reshape(*x.shape[:-1], 3), runs[0][2][:n].cpu().reshape(x.shape)
    # x0 without the mask, against float64; with sigma 0 the latent itself
    _, _, plain = launch_preview(xd, cd, ud, w, sigma, W, b, None, None, True, 0xA5)
    plain = plain[:n].cpu().reshape(x.shape)
    err = (plain.double() - x0).abs()
    print(f"{label}: x0 max err / bound {float((err / x0_bound.clamp_min(1e-300)).max()):.3f}")
    assert (err <= x0_bound).all(), label
    if sigma == 0.0:
        assert torch.equal(plain, x), label
    if mask is None:
        assert torch.equal(out, plain)
    else:   # the keep rule, exactly, on the kernel's own x0
        m = mask.expand_as(x)
        blend = plain + m * (src - plain)                          # three separately rounded fp32 ops on the CPU
        want = torch.where(m == 1, src, torch.where(m == 0, plain, blend))
        assert torch.equal(out, want), label
        assert torch.equal(out[m == 1], src[m == 1])
    # RGB
    want_codes = codes(val)
    diff = (rgb.double() - want_codes).abs()
    assert diff.max() <= 1, (label, float(diff.max()))
    firm = codes(val - bound) == codes(val + bound)
    assert firm.double().mean() > 0.9, label                        # the bound leaves nearly every value decided
    assert torch.equal(rgb.double()[firm], want_codes[firm]), (label, int((diff[firm] != 0).sum()))
    # without x0_out the same RGB; the helper gives the same bits
    _, rgb_only, untouched = launch_preview(xd, cd, ud, w, sigma, W, b, sd, md, False, 0xA5)
    assert torch.equal(rgb_only[:cells * 3].cpu().reshape(rgb.shape), rgb) and (untouched == float(0xA5)).all()
    h_rgb, h_x0 = E.x0_preview(xd, cd, ud, w, sigma, W, b, source=sd, keep_mask=md, want_x0=True)
    assert torch.equal(h_rgb.cpu(), rgb) and torch.equal(h_x0.cpu(), out)
    return rgb, want_codes


@pytest.mark.parametrize("Cc", [4, 16, 64])
@pytest.mark.parametrize("thw", [(1, 2, 6), (3, 5, 7), (3, 8, 12)])
def test_x0_preview_kernel_against_float64(thw, Cc):
    x, src, c, u, mask, W, b = kernel_case(thw, Cc, seed=1000 * Cc + int(np.prod(thw)))
    for with_u in (False, True):
        for w in (1.0, 5.0):
            for sigma in (0.0, 0.37, 1.0):
                for with_mask in (False, True):
                    check_preview(x, src, c, u if with_u else None, w, sigma, W, b, mask if with_mask else None,
                                  f"thw={thw} C={Cc} u={with_u} w={w} sigma={sigma} mask={with_mask}")
    check_preview(x, src, c, u, 5.0, 0.37, W, None, None, "no bias")


def test_x0_preview_saturates_and_maps_nan_to_zero():
    x, src, c, u, mask, W, b = kernel_case((3, 5, 7), 16, seed=77, scale=6.0)
    _, _, _, val, _ = preview_reference(x, c, u, 5.0, 0.37, W, b)
    ref = codes(val)
    assert (ref == 0).any() and (ref == 255).any() and (val < -10).any() and (val > 265).any()      # the reference itself saturates both ways
    rgb, want = check_preview(x, src, c, u, 5.0, 0.37, W, b, None, "saturation")
    assert (rgb == 0).any() and (rgb == 255).any()
    # a NaN latent cell gives 0 in all three colours, its neighbours are untouched
    xn = x.clone()
    xn[1, 2, 3] = float("nan")
    st, out, _ = launch_preview(xn.cuda(), c.cuda(), u.cuda(), 5.0, 0.37, W, b, None, None, False, 0xA5)
    assert st == 0
    out = out[:3 * 5 * 7 * 3].cpu().reshape(3, 5, 7, 3)
    assert (out[1, 2, 3] == 0).all()
    keep = torch.ones(3, 5, 7, dtype=torch.bool)
    keep[1, 2, 3] = False
    assert torch.equal(out[keep], rgb[keep])
    # a single NaN channel is enough
    xn = x.clone()
    xn[0, 0, 0, 5] = float("nan")
    _, out, _ = launch_preview(xn.cuda(), c.cuda(), u.cuda(), 5.0, 0.37, W, b, None, None, False, 0xA5)
    assert (out[:3].cpu() == 0).all()


@pytest.mark.parametrize("Cc", [6, 68])
def test_x0_preview_refuses_other_channel_counts(Cc):
    from kandinsky import _engine as E
    g = torch.Generator().manual_seed(Cc)
    x, c = torch.randn(2, 3, 4, Cc, generator=g).cuda(), torch.randn(2, 3, 4, Cc, generator=g).to(BF).cuda()
    W = torch.zeros(Cc, 3)
    st, rgb, x0 = launch_preview(x, c, None, 1.0, 0.5, W, None, None, None, True, 0xA5)
    assert st == K5_ERR_UNSUPPORTED
    assert (rgb == 0xA5).all() and (x0 == float(0xA5)).all()
    with pytest.raises(RuntimeError, match="k5_x0_preview"):
        E.x0_preview(x, c, None, 1.0, 0.5, W, None)


# ------------------------------------------------------------------------------------------ engine


@pytest.fixture(scope="module")
def tiny_dit(cfg, tiny_sd):
    need_gpu()
    return make_dit(cfg, tiny_sd, engine=True)


run_generate = functools.partial(kit.run_generate, steps=4, shape=SHAPE, pos=POS)


class Recorder:
    """a callback that keeps what it is shown"""

    def __init__(self, stop_at=None, raise_at=None):
        self.seen, self.stop_at, self.raise_at = [], stop_at, raise_at

    def __call__(self, info):
        self.seen.append(NS(step=info.step, num_steps=info.num_steps, sample=info.sample, num_samples=info.num_samples, sigma=info.sigma,
                            preview=None if info.preview is None else info.preview.clone(),
                            x0=None if info.x0 is None else info.x0.clone()))
        if self.raise_at is not None and info.step == self.raise_at:
            raise KeyError(f"callback failed at step {info.step}")
        return self.stop_at is not None and info.step == self.stop_at


def watched(dit, rec=None, every=1):
    W, b = factors()
    rec = Recorder() if rec is None else rec
    dit.set_watch(rec, preview_every=every, rgb_factors=W, rgb_bias=b, want_x0=True)
    return rec


def check_sequence(seen, steps, every, samples=1, first=0):
    from kandinsky.generation_utils import sigma_schedule
    sig = sigma_schedule(steps, 5.0)[first:].tolist()
    n = len(sig) - 1
    assert [(s.sample, s.step) for s in seen] == [(b, i) for b in range(samples) for i in range(n)]
    for s in seen:
        assert (s.num_steps, s.num_samples) == (n, samples)
        assert s.sigma == sig[s.step + 1]                           # the schedule's fp32 value, exactly
        has = every > 0 and ((s.step + 1) % every == 0 or s.step == n - 1)
        assert (s.preview is not None) == has and (s.x0 is not None) == has, (s.step, every)
        if has:
            assert s.preview.dtype == torch.uint8 and tuple(s.preview.shape) == SHAPE[:3] + (3,) and not s.preview.is_cuda
            assert s.x0.dtype == torch.float32 and tuple(s.x0.shape) == SHAPE and s.x0.is_cuda


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_watch_leaves_the_eager_run_bit_identical(tiny_dit, golden, w):
    plain = run_generate(tiny_dit, golden, w)
    assert tiny_dit.watch_state() == (4, False)
    rec = watched(tiny_dit)
    try:
        seen = run_generate(tiny_dit, golden, w)
    finally:
        tiny_dit.clear_watch()
    assert torch.equal(seen, plain)
    check_sequence(rec.seen, 4, 1)
    assert tiny_dit.watch_state() == (4, False)
    assert torch.equal(rec.seen[-1].x0, plain)                       # sigma = 0 after the last step: x0 is the returned latent
    assert not torch.equal(rec.seen[0].x0, rec.seen[1].x0)
    assert torch.equal(run_generate(tiny_dit, golden, w), plain)     # and the handle is as it was once the watch is gone


def test_watch_leaves_the_captured_step_bit_identical(cfg, tiny_sd, golden):
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    eager = run_generate(dit, golden, 5.0)
    dit.set_graph(True)
    plain = run_generate(dit, golden, 5.0)
    rec = watched(dit)
    seen = run_generate(dit, golden, 5.0)
    assert torch.equal(plain, eager) and torch.equal(seen, plain)
    check_sequence(rec.seen, 4, 1)
    assert torch.equal(rec.seen[-1].x0, plain)
    # the captured step shows what the eager loop shows
    dit.set_graph(False)
    rec2 = watched(dit)
    run_generate(dit, golden, 5.0)
    for a, b in zip(rec.seen, rec2.seen):
        assert torch.equal(a.preview, b.preview) and torch.equal(a.x0, b.x0)
    dit._destroy_engine(force=True)


def test_watch_leaves_an_edit_bit_identical(tiny_dit, golden):
    src, mask = source_latent(), edit_mask()
    kw = dict(init_latent=src, strength=0.75, keep_mask=mask)
    plain = run_generate(tiny_dit, golden, 5.0, **kw)
    rec = watched(tiny_dit)
    try:
        seen = run_generate(tiny_dit, golden, 5.0, **kw)
    finally:
        tiny_dit.clear_watch()
    assert torch.equal(seen, plain)
    check_sequence(rec.seen, 4, 1, first=1)
    keep = (mask == 1).expand(SHAPE)
    for s in rec.seen:                                               # kept cells show the source at every step
        assert torch.equal(s.x0.cpu()[keep], src[keep])


def test_watch_leaves_magcache_bit_identical(cfg, tiny_sd, golden):
    from kandinsky.generation_utils import generate
    from kandinsky.magcache_utils import disable_magcache, magcache_state, set_magcache_params
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    te, ne = prompts(golden)
    src, mask = source_latent(), edit_mask()
    args = ("cuda:0", SHAPE, c["num_steps"], te, ne, POS, torch.arange(7), torch.arange(4), c["guidance_weight"], c["scheduler_scale"], FLASH)
    outs = []
    try:
        for watch in (False, True):
            set_magcache_params(dit, c["ratios"], c["num_steps"], c["no_cfg"])
            rec = watched(dit) if watch else None
            outs.append(generate(dit, *args, noise=golden["gen.noise"], init_latent=src, keep_mask=mask))
            assert magcache_state(dit)[2] > 0                        # steps were skipped in both runs
    finally:
        disable_magcache(dit)
    assert torch.equal(outs[0], outs[1])
    assert [s.step for s in rec.seen] == list(range(c["num_steps"]))
    dit._destroy_engine(force=True)


def test_watch_leaves_sample_many_bit_identical(tiny_dit, golden):
    g = torch.Generator().manual_seed(21)
    noise = torch.cat([golden["gen.noise"], torch.randn(*SHAPE, generator=g)])
    shape = (2 * SHAPE[0],) + SHAPE[1:]
    plain = run_generate(tiny_dit, golden, 5.0, shape=shape, noise=noise, batch=2)
    rec = watched(tiny_dit, every=2)
    try:
        seen = run_generate(tiny_dit, golden, 5.0, shape=shape, noise=noise, batch=2)
    finally:
        tiny_dit.clear_watch()
    assert torch.equal(seen, plain)
    check_sequence(rec.seen, 4, 2, samples=2)
    for b in range(2):
        assert torch.equal(rec.seen[4 * b + 3].x0, plain[3 * b:3 * b + 3])


@pytest.mark.parametrize("every", [1, 2, 3])
def test_callback_sequence_and_preview_steps(tiny_dit, golden, every):
    W, b = factors()
    rec = Recorder()
    out = run_generate(tiny_dit, golden, 5.0, steps=6, callback=rec, preview_every=every, preview_factors=(W, b), preview_x0=True)
    check_sequence(rec.seen, 6, every)
    assert [s.step for s in rec.seen if s.preview is not None] == {1: [0, 1, 2, 3, 4, 5], 2: [1, 3, 5], 3: [2, 5]}[every]
    assert torch.equal(rec.seen[-1].x0, out)
    assert tiny_dit._watch is None                                   # generate took its hook off the model again
    rec0 = Recorder()                                                # progress only: every step, never a preview
    run_generate(tiny_dit, golden, 5.0, steps=6, callback=rec0)
    check_sequence(rec0.seen, 6, 0)


@pytest.mark.parametrize("w,edit", [(1.0, False), (5.0, False), (5.0, True)])
def test_fused_and_per_step_paths_show_the_same_bits(tiny_dit, golden, w, edit):
    W, b = factors()
    kw = dict(init_latent=source_latent(), strength=0.75, keep_mask=edit_mask()) if edit else {}
    recs, outs = [], []
    for model in (tiny_dit, Wrapped(tiny_dit)):
        rec = Recorder()
        outs.append(run_generate(model, golden, w, callback=rec, preview_every=1, preview_factors=(W, b), preview_x0=True, **kw))
        recs.append(rec)
    assert torch.equal(outs[0], outs[1])
    assert len(recs[0].seen) == len(recs[1].seen) == (3 if edit else 4)
    for a, c in zip(recs[0].seen, recs[1].seen):
        assert (a.step, a.num_steps, a.sample, a.num_samples, a.sigma) == (c.step, c.num_steps, c.sample, c.num_samples, c.sigma)
        assert torch.equal(a.preview, c.preview) and torch.equal(a.x0, c.x0)
    assert len({bytes(s.preview.numpy().tobytes()) for s in recs[0].seen}) > 1    # the previews move from step to step


def test_stop_from_the_callback(tiny_dit, golden):
    from kandinsky.generation_utils import sigma_schedule
    from kandinsky.models.dit import SamplingInterrupted
    te, ne = prompts(golden)
    full = run_generate(tiny_dit, golden, 5.0, steps=6)
    rec = Recorder(stop_at=2)
    with pytest.raises(SamplingInterrupted) as ei:
        run_generate(tiny_dit, golden, 5.0, steps=6, callback=rec)
    e = ei.value
    assert e.steps_done in (3, 4)
    assert [s.step for s in rec.seen] == [0, 1, 2]                   # nothing after the stop
    assert tiny_dit.watch_state() == (e.steps_done, True)
    sig = sigma_schedule(6, 5.0).tolist()
    part = golden["gen.noise"].cuda().clone().contiguous()
    tiny_dit.sample(part, sig[:e.steps_done + 1], te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0))
    assert torch.equal(e.latent, part)
    assert torch.equal(run_generate(tiny_dit, golden, 5.0, steps=6), full)
    # the per-step path stops on the step the callback saw
    rec2 = Recorder(stop_at=2)
    with pytest.raises(SamplingInterrupted) as ei2:
        run_generate(Wrapped(tiny_dit), golden, 5.0, steps=6, callback=rec2)
    assert ei2.value.steps_done == 3 and [s.step for s in rec2.seen] == [0, 1, 2]
    # sample_many: the samples after the stopped one are as they came
    g = torch.Generator().manual_seed(21)
    noise = torch.cat([golden["gen.noise"], torch.randn(*SHAPE, generator=g)])
    rec3 = Recorder(stop_at=1)
    with pytest.raises(SamplingInterrupted) as ei3:
        run_generate(tiny_dit, golden, 5.0, shape=(6,) + SHAPE[1:], noise=noise, batch=2, callback=rec3)
    assert ei3.value.sample == 0 and [(s.sample, s.step) for s in rec3.seen] == [(0, 0), (0, 1)]
    assert torch.equal(ei3.value.latent.reshape(6, *SHAPE[1:])[3:].cpu(), noise[3:])


def test_an_exception_in_the_callback_comes_out_of_generate(tiny_dit, golden):
    plain = run_generate(tiny_dit, golden, 5.0)
    rec = Recorder(raise_at=1)
    with pytest.raises(KeyError, match="callback failed at step 1"):
        run_generate(tiny_dit, golden, 5.0, callback=rec)
    assert [s.step for s in rec.seen] == [0, 1]
    assert tiny_dit._watch is None
    assert torch.equal(run_generate(tiny_dit, golden, 5.0), plain)   # the handle works afterwards
    with pytest.raises(KeyError):
        run_generate(Wrapped(tiny_dit), golden, 5.0, callback=Recorder(raise_at=1))


def test_refusals_carry_a_message_and_touch_nothing(tiny_dit, cfg, tiny_sd, golden):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule
    te, ne = prompts(golden)
    W, b = factors()
    sig = sigma_schedule(2, 5.0).tolist()
    lat = golden["gen.noise"].cuda().contiguous()
    before = lat.clone()
    cb = lambda info: None   # noqa: E731
    L = E.lib()
    tr = E.WatchTrampoline(cb)
    wa = (C.c_float * 48)(*W.reshape(-1).tolist())

    def c_watch(every=0, want_x0=0, w=None):
        k = E.Watch()
        k.fn, k.preview_every, k.want_x0 = tr.c_fn, every, want_x0
        if w is not None:
            k.rgb_w = C.cast(w, C.POINTER(C.c_float))
        return C.byref(k)

    h = tiny_dit.engine("cuda:0")
    # arguments: the Python surface names the way out, the C entry point answers K5_ERR_ARG with a message
    with pytest.raises(ValueError, match="preview_every"):
        tiny_dit.set_watch(cb, preview_every=-1, rgb_factors=W)
    with pytest.raises(ValueError, match="fit_rgb_factors"):
        tiny_dit.set_watch(cb, preview_every=2)
    with pytest.raises(ValueError, match="fit_rgb_factors"):
        run_generate(tiny_dit, golden, 5.0, callback=cb, preview_every=2)
    with pytest.raises(ValueError, match="preview_every"):
        run_generate(tiny_dit, golden, 5.0, callback=cb, preview_every=-1, preview_factors=(W, b))
    for msg, arg in {"preview_every must be >= 0": c_watch(-1, 0, wa), "need rgb_w": c_watch(2), "want_x0 needs": c_watch(0, 1)}.items():
        assert L.k5_dit_set_watch(h, arg) == K5_ERR_ARG, msg
        assert msg.encode() in L.k5_last_error(), (msg, L.k5_last_error())
    assert tiny_dit._watch is None
    call = lambda d: d.sample(lat, sig, te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0))   # noqa: E731
    # a rank of a loopback group of 2, and a handle of an in-engine CFG pair
    for kind in ("sequence-parallel group", "CFG pair"):
        group = E.LoopbackGroup(2)
        dits = [make_dit(cfg, tiny_sd) for _ in range(2)]
        for d in dits:
            d.engine("cuda:0")
        dits[1].set_watch(cb)                                       # installed while the handle was still on its own
        for r, d in enumerate(dits):
            d.enable_loopback(group, r) if kind == "sequence-parallel group" else d.enable_cfg_pair_loopback(group, r)
        with pytest.raises(RuntimeError, match="single-rank"):
            dits[0].set_watch(cb)
        assert L.k5_dit_set_watch(dits[0]._handle, c_watch()) == K5_ERR_STATE
        assert kind.encode() in L.k5_last_error() and b"collective" in L.k5_last_error()
        with pytest.raises(ValueError, match="single-rank"):
            run_generate(dits[0], golden, 5.0, callback=cb)
        with pytest.raises(RuntimeError, match=kind):               # k5_sample refuses before anything is enqueued: no peer is needed
            call(dits[1])
        for d in dits:
            d._destroy_engine(force=True)
    torch.cuda.synchronize()
    assert torch.equal(lat, before)


# ------------------------------------------------------------------------------------------ pipeline end to end
def test_pipeline_callback_and_previews_end_to_end():
    from test_pipeline import StubTextEmbedder, make_conf
    from kandinsky.models.dit import get_dit
    from kandinsky.models.vae import AutoencoderKLHunyuanVideo
    from kandinsky.t2v_pipeline import Kandinsky5T2VPipeline
    dev = "cuda:0"
    conf = make_conf()
    dit = get_dit(conf.model.dit_params)
    g = torch.Generator().manual_seed(0)
    sd = {k: (torch.ones_like(v) if k.endswith("norm.weight") else torch.randn(v.shape, generator=g) * 0.05) for k, v in dit.state_dict().items()}
    dit.load_state_dict(sd, assign=True)
    dit = dit.to(dev)
    vae = AutoencoderKLHunyuanVideo(block_out_channels=(64, 64, 128, 128), norm_num_groups=16)
    vsd = {}
    for k, p in vae.state_dict().items():
        if "norm" in k and k.endswith("weight"):
            vsd[k] = torch.ones(p.shape)
        elif k.endswith("bias"):
            vsd[k] = torch.zeros(p.shape)
        else:
            vsd[k] = torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5)
    vae.load_state_dict(vsd, assign=True)
    vae = vae.eval().to(dev)
    frames = 24 // 4 + 1
    pipe = Kandinsky5T2VPipeline({"dit": dev, "vae": dev, "text_embedder": dev}, dit=dit, text_embedder=StubTextEmbedder(), vae=vae, conf=conf)
    kw = dict(time_length=1, width=512, height=512, seed=7, expand_prompts=False, scheduler_scale=5.0, num_steps=4)
    plain = pipe("a cat in a blue hat", progress=False, **kw)
    rec = Recorder()
    seen = pipe("a cat in a blue hat", callback=rec, preview_every=2, preview_factors=factors(), **kw)
    assert torch.equal(seen, plain)
    assert [s.step for s in rec.seen] == [0, 1, 2, 3]
    got = [s.preview for s in rec.seen if s.preview is not None]
    assert [s.step for s in rec.seen if s.preview is not None] == [1, 3]
    for p in got:
        assert p.dtype == torch.uint8 and tuple(p.shape) == (frames, 64, 64, 3)
    assert not torch.equal(got[0], got[1]) and all(s.x0 is None for s in rec.seen)
