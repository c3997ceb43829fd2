"""Temporal context windows on the MI355X: the blend + CFG + Euler kernel bit for bit against the torch expression, k5_sample_windows against
the same forwards issued step by step, parity with the oracle and the reference golden, refusals, and the pipeline end to end.

Tolerances are those of tests/test_gpu_edit.py (tests/test_gpu_dit.py, tests/test_gpu_visual_cond.py): a final latent within relative L2
1e-2 of the bf16-island oracle, composed here over the same plan, and 3e-2 of the reference's fp32 golden (tools/gen_golden_windows.py).
Everything that claims "the same computation" is asserted bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
import kit  # noqa: E402
from kit import BF, GOLDEN, cfg, f32, make_dit, prompts, rel, tiny_dit, Wrapped  # noqa: E402

HW = (8, 12, 16)
PLANS = {"t5": (5, 3, 1), "t6": (6, 3, 1), "t7": (7, 3, 2)}     # single / double coverage; ragged overlaps of 2 and 1; three-fold


def pos_for(F):
    return [torch.arange(F), torch.arange(HW[0] // 2), torch.arange(HW[1] // 2)]


@pytest.fixture(scope="module")
def win_golden():
    from safetensors.torch import load_file
    return dict(load_file(os.path.join(GOLDEN, "dit_tiny_windows.safetensors"))), json.load(open(os.path.join(GOLDEN, "dit_tiny_windows_meta.json")))


def other_prompt(golden, L=5):
    g = torch.Generator().manual_seed(31)
    return {"text_embeds": torch.randn(L, golden["fwd.text"].shape[1], generator=g).cuda(),
            "pooled_embed": torch.randn(tuple(golden["fwd.pooled"].shape), generator=g).cuda()}


def noise_of(tag, win_golden):
    g, _ = win_golden
    if f"win.{tag}.noise" in g:
        return g[f"win.{tag}.noise"]
    T = PLANS[tag][0]
    return torch.randn(T, *HW, generator=torch.Generator().manual_seed(100 * T + T))


def run_generate(model, golden, noise, w, steps=4, pos=None, **kw):
    return kit.run_generate(model, golden, w, steps=steps, shape=tuple(noise.shape), pos=pos or pos_for(3), noise=noise, **kw)


def run_windows(model, golden, win_golden, tag, w, **kw):
    T, F, o = PLANS[tag]
    return run_generate(model, golden, noise_of(tag, win_golden), w, context_frames=F, context_overlap=o, **kw)


# ------------------------------------------------------------------------------------------ kernel
def windows_ref(img, c, u, w, dt, starts, weights):
    """the torch expression the kernel is held to: v per window as eager bf16 ops, every product and sum of the blend an fp32 op of its own, in
    window order; img (T, n), c / u (nwin, F, n), weights fp32 (nwin, F) on the device"""
    T, F = img.shape[0], weights.shape[1]
    acc = [None] * T
    for i, st in enumerate(starts):
        v = c[i] if u is None else u[i] + w * (c[i] - u[i])
        for j in range(F):
            p = weights[i, j] * v[j].float()
            acc[st + j] = p if acc[st + j] is None else acc[st + j] + p
    return torch.stack([img[t] + (dt * acc[t]).to(BF).float() for t in range(T)])


@pytest.mark.parametrize("frame", [(8, 12, 16), (5, 7, 16), (5, 7, 3)])            # whole groups of four twice, and an odd frame on the scalar path
@pytest.mark.parametrize("plan", [(7, 3, 2), (6, 3, 1)])
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_cfg_euler_windows_bit_exact(frame, plan, w):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import context_windows
    T, F, o = plan
    starts, weights = context_windows(T, F, o)
    nwin, n = len(starts), int(np.prod(frame))
    g = torch.Generator().manual_seed(n + T + int(w))
    img = torch.randn(T, n, generator=g).cuda()
    pad = 64                                                               # NaN in front of and behind the velocities: outside every window's reach
    cbuf = torch.full((nwin * F * n + 2 * pad,), float("nan"), dtype=BF, device="cuda")
    ubuf = torch.full((nwin * F * n + 2 * pad,), float("nan"), dtype=BF, device="cuda")
    c = cbuf[pad:pad + nwin * F * n].view(nwin, F, n)
    c.copy_(torch.randn(nwin, F, n, generator=g).to(BF))
    u = None
    if w != 1.0:
        u = ubuf[pad:pad + nwin * F * n].view(nwin, F, n)
        u.copy_(torch.randn(nwin, F, n, generator=g).to(BF))
    dt = f32(-0.0625 * 1.3)
    st_dev, wt_dev = E.window_tables(starts, weights, "cuda")
    want = windows_ref(img, c, u, w, dt, starts, wt_dev)
    buf = torch.full((T * n + 64,), 7.0, device="cuda")                     # a guard region after the latent
    buf[:T * n] = img.view(-1)
    E.check(E.lib().k5_cfg_euler_windows(buf.data_ptr(), c.data_ptr(), E.ptr(u), w, dt, st_dev.data_ptr(), wt_dev.data_ptr(), nwin, F, T, n,
                                         E.stream_ptr()), "k5_cfg_euler_windows")
    torch.cuda.synchronize()
    assert torch.isfinite(buf).all()                                        # none of the NaN around the velocities was read
    assert torch.equal(buf[:T * n].view(T, n), want)
    assert (buf[T * n:] == 7.0).all()
    helper = img.clone().view(T, *frame)
    E.cfg_euler_windows_(helper, c.view(nwin, F, *frame), None if u is None else u.view(nwin, F, *frame), w, dt, st_dev, wt_dev)
    assert torch.equal(helper.view(T, n), want)


@pytest.mark.parametrize("w", [1.0, 5.0])
@pytest.mark.parametrize("n", [8 * 12 * 16, 5 * 7 * 3])
def test_one_window_of_weight_one_is_k5_cfg_euler(w, n):
    from kandinsky import _engine as E
    T = 3
    g = torch.Generator().manual_seed(n + int(w))
    img = torch.randn(T, n, generator=g).cuda()
    c = torch.randn(1, T, n, generator=g).cuda().to(BF)
    u = torch.randn(1, T, n, generator=g).cuda().to(BF) if w != 1.0 else None
    dt = f32(-0.21)
    st_dev, wt_dev = E.window_tables([0], torch.ones(1, T), "cuda")
    plain, win = img.clone(), img.clone()
    E.cfg_euler_(plain, c, u, w, dt)
    E.cfg_euler_windows_(win, c, u, w, dt, st_dev, wt_dev)
    assert torch.equal(win, plain)


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_cfg_euler_windows_on_a_misaligned_base_takes_the_scalar_path(w):
    """img one float into a larger buffer: 4-byte but not 16-byte aligned, so a frame of whole groups of four (5 * 7 * 16) still runs a lane
    per element.  The same torch oracle, the same guards as test_cfg_euler_windows_bit_exact."""
    from kandinsky import _engine as E
    from kandinsky.generation_utils import context_windows
    T, F, o = 7, 3, 2
    starts, weights = context_windows(T, F, o)
    nwin, n = len(starts), 5 * 7 * 16
    g = torch.Generator().manual_seed(n + T + int(w) + 1)
    img = torch.randn(T, n, generator=g).cuda()
    pad = 64
    bufs = [torch.full((nwin * F * n + 2 * pad,), float("nan"), dtype=BF, device="cuda") for _ in range(2)]   # NaN around the velocities
    c = bufs[0][pad:pad + nwin * F * n].view(nwin, F, n)
    c.copy_(torch.randn(nwin, F, n, generator=g).to(BF))
    u = None
    if w != 1.0:
        u = bufs[1][pad:pad + nwin * F * n].view(nwin, F, n)
        u.copy_(torch.randn(nwin, F, n, generator=g).to(BF))
    dt = f32(-0.0625 * 1.3)
    st_dev, wt_dev = E.window_tables(starts, weights, "cuda")
    want = windows_ref(img, c, u, w, dt, starts, wt_dev)
    buf = torch.full((1 + T * n + 64,), 7.0, device="cuda")                 # a guard float in front of the latent and a guard region after it
    lat = buf[1:1 + T * n]
    lat.copy_(img.view(-1))
    assert buf.data_ptr() % 16 == 0 and lat.data_ptr() % 16 == 4 and n % 4 == 0
    E.check(E.lib().k5_cfg_euler_windows(lat.data_ptr(), c.data_ptr(), E.ptr(u), w, dt, st_dev.data_ptr(), wt_dev.data_ptr(), nwin, F, T, n,
                                         E.stream_ptr()), "k5_cfg_euler_windows")
    torch.cuda.synchronize()
    assert torch.isfinite(buf).all()                                        # none of the NaN around the velocities was read
    assert torch.equal(lat.view(T, n), want)
    assert buf[0] == 7.0 and (buf[1 + T * n:] == 7.0).all()


def test_kernel_entry_refusals():
    from kandinsky import _engine as E
    L = E.lib()
    img = torch.zeros(5, 64, device="cuda")
    c = torch.zeros(2, 3, 64, dtype=BF, device="cuda")
    st, wt = E.window_tables([0, 2], torch.ones(2, 3), "cuda")
    call = lambda *a: L.k5_cfg_euler_windows(*a, E.stream_ptr())   # noqa: E731
    good = (img.data_ptr(), c.data_ptr(), None, 1.0, 0.1, st.data_ptr(), wt.data_ptr(), 2, 3, 5, 64)
    assert call(*good) == 0
    for i, bad in ((0, None), (1, None), (5, None), (6, None), (7, 0), (7, 65), (8, 0)):
        a = list(good)
        a[i] = bad
        assert call(*a) == 1, (i, bad)
    assert call(*good[:9], 4, 64) == 1 and b"reaches outside" in L.k5_last_error()       # the last window would end at frame 4 of 4
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ sampler: same bits
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_a_window_as_long_as_the_clip_is_the_plain_run(tiny_dit, golden, w):
    noise = golden["gen.noise"]
    plain = run_generate(tiny_dit, golden, noise, w)
    assert torch.equal(run_generate(tiny_dit, golden, noise, w, context_frames=3), plain)
    assert torch.equal(run_generate(tiny_dit, golden, noise, w, context_frames=8, context_overlap=2, pos=pos_for(3)), plain)
    assert torch.equal(run_generate(Wrapped(tiny_dit), golden, noise, w, context_frames=3, context_overlap=1), plain)


@pytest.mark.parametrize("tag", sorted(PLANS))
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_fused_equals_step_by_step(tiny_dit, golden, win_golden, tag, w):
    a = run_windows(tiny_dit, golden, win_golden, tag, w)
    b = run_windows(Wrapped(tiny_dit), golden, win_golden, tag, w)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert not torch.equal(a.cpu(), noise_of(tag, win_golden))


def test_fused_equals_step_by_step_with_a_prompt_per_window(tiny_dit, golden, win_golden):
    te, _ = prompts(golden)
    tb = other_prompt(golden)
    text = [(te, torch.arange(7)), (tb, torch.arange(5)), (te, torch.arange(7))]
    a = run_windows(tiny_dit, golden, win_golden, "t6", 5.0, context_text=text)
    b = run_windows(Wrapped(tiny_dit), golden, win_golden, "t6", 5.0, context_text=text)
    assert torch.equal(a, b)
    assert not torch.equal(a, run_windows(tiny_dit, golden, win_golden, "t6", 5.0))
    with pytest.raises(ValueError, match="nwin = 3"):
        run_windows(tiny_dit, golden, win_golden, "t6", 5.0, context_text=text[:2])


def test_visual_cond_through_windows(tiny_dit, golden, win_golden):
    T = 6
    g = torch.Generator().manual_seed(11)
    vc, vm = torch.zeros(T, *HW), torch.zeros(T, *HW[:2], 1)
    vc[0], vm[0] = torch.randn(HW, generator=g), 1.0                      # image-to-video: the picture lies in window 0's slice
    vc[4], vm[4] = torch.randn(HW, generator=g), 1.0                      # and a frame only the last window sees
    for w in (1.0, 5.0):
        a = run_windows(tiny_dit, golden, win_golden, "t6", w, visual_cond=vc, visual_cond_mask=vm)
        b = run_windows(Wrapped(tiny_dit), golden, win_golden, "t6", w, visual_cond=vc, visual_cond_mask=vm)
        assert torch.equal(a, b)
        assert not torch.equal(a, run_windows(tiny_dit, golden, win_golden, "t6", w))


def test_prompt_of_one_window_reaches_only_its_frames_in_one_step(tiny_dit, golden, win_golden):
    """Prompts A,A,A,A,B against all-A after ONE step: the frames that only A-windows cover are equal bit for bit (after later steps every
    frame has seen window 4 through the overlaps, so only one step is asserted)."""
    te, _ = prompts(golden)
    tb = other_prompt(golden)
    A, B = (te, torch.arange(7)), (tb, torch.arange(5))
    all_a = run_windows(tiny_dit, golden, win_golden, "t7", 5.0, steps=1, context_text=[A] * 5)
    last_b = run_windows(tiny_dit, golden, win_golden, "t7", 5.0, steps=1, context_text=[A] * 4 + [B])
    assert torch.equal(all_a, run_windows(tiny_dit, golden, win_golden, "t7", 5.0, steps=1))
    assert torch.equal(all_a[:4], last_b[:4])                               # window 4 covers frames 4, 5, 6
    for t in (4, 5, 6):
        assert not torch.equal(all_a[t], last_b[t])


# ------------------------------------------------------------------------------------------ parity
def oracle_windows(sd, cfg, noise, starts, weights, steps, w, s, te, ne, mode):
    """the windowed loop written around the oracle's get_velocity (conditioning channels zero, as the reference's loop has them)"""
    sig = O.sigma_schedule(steps, s)
    F = weights.shape[1]
    zeros = torch.zeros(F, *noise.shape[1:]), torch.zeros(F, *noise.shape[1:-1], 1)
    img = noise.clone()
    for i in range(steps):
        acc = torch.zeros_like(img)
        for k, st in enumerate(starts):
            v = O.get_velocity(sd, cfg, torch.cat([img[st:st + F], *zeros], -1), sig[i].unsqueeze(0), te, ne, pos_for(F), torch.arange(7),
                               torch.arange(4), w, (1.0, 2.0, 2.0), None, mode)
            acc[st:st + F] += weights[k][:, None, None, None] * v.float()
        img = img + O._r((sig[i + 1] - sig[i]) * acc, mode)
    return img


@pytest.mark.parametrize("tag", ["t6", "t7"])
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_parity_with_the_oracle_and_the_reference_golden(tiny_dit, tiny_sd, cfg, golden, win_golden, tag, w):
    """Measured on the MI355X, engine vs bf16 oracle / vs reference golden: t6 w=1 1.59e-3 / 2.38e-3, t7 w=1 1.53e-3 / 2.32e-3,
    t6 w=5 5.82e-3 / 7.29e-3, t7 w=5 5.23e-3 / 6.77e-3.  The bounds stay the project's fixed ones (1e-2 / 3e-2)."""
    from kandinsky.generation_utils import context_windows
    g, meta = win_golden
    case = meta["cases"][tag]
    starts, weights = context_windows(case["T"], case["frames"], case["overlap"])
    assert starts == case["starts"] and torch.equal(weights, g[f"win.{tag}.weights"])
    out = run_windows(tiny_dit, golden, win_golden, tag, w, steps=meta["steps"])
    te, ne = prompts(golden)
    tec, nec = {k: v.cpu() for k, v in te.items()}, {k: v.cpu() for k, v in ne.items()}
    ref16 = oracle_windows(tiny_sd, O.DitConfig(**cfg), g[f"win.{tag}.noise"], starts, weights, meta["steps"], w, meta["scheduler_scale"],
                           tec, nec, "bf16")
    r16, r32 = rel(out, ref16), rel(out, g[f"win.{tag}.{w}.final"])
    print(f"windows {tag} w={w}: engine vs bf16 oracle {r16:.3e}, vs reference golden {r32:.3e}")
    assert r16 <= 1e-2, r16
    assert r32 <= 3e-2, r32


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_the_windows_matter(tiny_dit, golden, win_golden, w):
    noise = noise_of("t7", win_golden)
    windowed = run_windows(tiny_dit, golden, win_golden, "t7", w)
    full = run_generate(tiny_dit, golden, noise, w, pos=pos_for(7))       # one forward over all 7 frames, positions 0 .. 6
    assert torch.isfinite(full).all()
    assert not torch.equal(windowed, full)
    assert rel(windowed, full) > 1e-3, rel(windowed, full)


# ------------------------------------------------------------------------------------------ watch, refusals
def test_progress_and_cancel(tiny_dit, golden, win_golden):
    from kandinsky.models.dit import SamplingInterrupted
    seen = []
    out = run_windows(tiny_dit, golden, win_golden, "t6", 5.0, callback=lambda info: seen.append((info.step, info.num_steps, info.preview)) and False)
    assert seen == [(i, 4, None) for i in range(4)]
    assert torch.equal(out, run_windows(tiny_dit, golden, win_golden, "t6", 5.0))
    with pytest.raises(SamplingInterrupted) as e:
        run_windows(tiny_dit, golden, win_golden, "t6", 5.0, callback=lambda info: info.step == 0)
    assert 1 <= e.value.steps_done <= 2                                     # the engine runs one step ahead of the callback
    with pytest.raises(ValueError, match="preview_every"):
        run_windows(tiny_dit, golden, win_golden, "t6", 5.0, callback=lambda info: False, preview_every=1, preview_factors=(torch.zeros(16, 3), None))
    assert tiny_dit._watch is None


def test_refusals_touch_nothing(tiny_dit, cfg, tiny_sd, golden, win_golden):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import context_windows, sigma_schedule
    from kandinsky.magcache_utils import disable_magcache, set_magcache_params
    te, ne = prompts(golden)
    noise = noise_of("t6", win_golden)
    plain = run_windows(tiny_dit, golden, win_golden, "t6", 5.0)
    sig = sigma_schedule(4, 5.0).tolist()
    starts, weights = context_windows(6, 3, 1)
    lat = noise.cuda().contiguous()
    before = lat.clone()

    lat7 = noise_of("t7", win_golden).cuda().contiguous()
    before7 = lat7.clone()

    def call(d, windows=(starts, weights), x=lat, **kw):
        return d.sample(x, sig, te, ne, pos_for(3), torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0), windows=windows, **kw)

    def refused(d, match, **kw):
        with pytest.raises(RuntimeError, match=match):
            call(d, **kw)
        torch.cuda.synchronize()
        assert torch.equal(lat, before) and torch.equal(lat7, before7)

    # plans: a frame without a window, starts that do not ascend, a window past the end, too many windows
    refused(tiny_dit, "no frame window covers 3", windows=([0, 4], weights[:2]), x=lat7)     # 7 frames, windows of 3 at 0 and 4: frame 3 is bare
    refused(tiny_dit, "no frame window covers 5", windows=([0, 2], weights[:2]))
    refused(tiny_dit, "no frame window covers 0", windows=([1, 3], weights[:2]))
    refused(tiny_dit, "must ascend", windows=([0, 3, 1], weights))
    refused(tiny_dit, "must ascend", windows=([0, 0, 3], weights))
    refused(tiny_dit, "reaches outside", windows=([0, 1, 4], weights))
    refused(tiny_dit, "nwin must be", windows=(list(range(65)), torch.ones(65, 3)))
    with pytest.raises(ValueError, match="edit together with windows"):
        call(tiny_dit, edit=(lat, lat, None))
    # a watch with previews (installed on the handle itself, past generate's own check)
    tiny_dit.set_watch(lambda info: False, preview_every=1, rgb_factors=torch.zeros(16, 3))
    try:
        refused(tiny_dit, "previews")
    finally:
        tiny_dit.clear_watch()
    # MagCache, and a sequence-parallel group, on handles of their own
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    mag = make_dit(cfg, tiny_sd)
    mag.engine("cuda:0")
    set_magcache_params(mag, c["ratios"], c["num_steps"], c["no_cfg"])
    refused(mag, "MagCache")
    disable_magcache(mag)
    sp = make_dit(cfg, tiny_sd)
    sp.engine("cuda:0")
    sp.enable_sequence_parallel(0, 1, device="cuda:0")
    refused(sp, "sequence-parallel")
    del sp
    # the handles work afterwards
    out = call(mag)
    assert out is lat and torch.equal(lat, plain)
    lat.copy_(before)
    assert torch.equal(call(tiny_dit), plain)
    # graph replay on: the windowed call runs eagerly, the same bits
    gr = make_dit(cfg, tiny_sd)
    gr.engine("cuda:0")
    gr.set_graph(True)
    lat.copy_(before)
    assert torch.equal(call(gr), plain)
    # NULL arguments at the C entry
    assert E.lib().k5_sample_windows(tiny_dit.engine(lat.device), None, None, E.stream_ptr()) == 1


def test_an_odd_latent_is_refused_before_anything_is_enqueued(tiny_dit, golden):
    """rows and columns must be even: a temporal plan meets the check of every window plan, with the latent untouched"""
    from kandinsky.generation_utils import context_windows, sigma_schedule
    te, ne = prompts(golden)
    starts, weights = context_windows(6, 3, 1)
    lat = torch.randn(6, 7, 12, 16, generator=torch.Generator().manual_seed(77)).cuda().contiguous()
    before = lat.clone()
    pos = [torch.arange(3), torch.arange(7 // 2), torch.arange(6)]
    with pytest.raises(RuntimeError, match="must be even"):
        tiny_dit.sample(lat, sigma_schedule(4, 5.0).tolist(), te, ne, pos, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0),
                        windows=(starts, weights))
    torch.cuda.synchronize()
    assert torch.equal(lat, before)


# ------------------------------------------------------------------------------------------ pipeline end to end
def _tiny_pipeline():
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
    return Kandinsky5T2VPipeline({"dit": dev, "vae": dev, "text_embedder": dev}, dit=dit, text_embedder=StubTextEmbedder(), vae=vae, conf=conf), dit, vae


def test_pipeline_with_context_windows_end_to_end():
    pipe, dit, vae = _tiny_pipeline()
    seen = {}
    samp = dit.sample

    def spy_sample(*a, **k):
        seen["tiles"], seen["window_text"], seen["pos_t"] = k.get("tiles"), k.get("window_text"), len(a[4][0])
        return samp(*a, **k)

    dit.sample = spy_sample
    kw = dict(time_length=1, width=512, height=512, seed=7, expand_prompts=False, scheduler_scale=5.0, num_steps=2)
    # 1 s = 7 latent frames as windows of 0.5 s = 4 frames overlapping by 0.25 s = 1 frame: starts 0 and 3
    out = pipe("a cat in a blue hat", context_seconds=0.5, context_overlap_seconds=0.25, **kw)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, 3, 25, 512, 512)
    assert seen["tiles"].starts[0] == [0, 3] and seen["tiles"].counts == (2, 1, 1) and seen["pos_t"] == 4 and seen["window_text"] is None
    two = pipe(["a cat in a blue hat", "a dog"], context_seconds=0.5, context_overlap_seconds=0.25, **kw)
    assert tuple(two.shape) == (1, 3, 25, 512, 512) and len(seen["window_text"]) == 2
    assert not torch.equal(two, out)
    with pytest.raises(ValueError, match="nwin = 2"):
        pipe(["a", "b", "c"], context_seconds=0.5, context_overlap_seconds=0.25, **kw)
    dit.sample = samp
    # a latent longer than the tiling table's last row (61 latent frames) decodes: 73 latent frames = 289 pixel frames
    z = torch.randn(1, 16, 73, 4, 4, generator=torch.Generator().manual_seed(3)).cuda()
    frames = vae.decode(z).sample
    assert tuple(frames.shape) == (1, 3, 289, 32, 32) and torch.isfinite(frames.float()).all()
