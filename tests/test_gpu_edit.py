"""Video-to-video and masked editing on the MI355X: the renoise and CFG + Euler + keep kernels bit for bit against the torch expression,
k5_sample_edit through every mode of the fused sampler, and the pipeline's `video=` / `strength=` / `mask=` end to end.

Tolerances are those of tests/test_gpu_dit.py and tests/test_gpu_visual_cond.py: a final latent within relative L2 1e-2 of the
bf16-island oracle and 3e-2 of the reference's fp32 golden (tools/gen_golden_edit.py).  Everything that claims "the same computation"
is asserted bit for bit, and so is the kept region: cells of keep mask 1 end as the source."""
import ctypes as C
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
import kit  # noqa: E402
from kit import BF, GOLDEN, POS, ROOT, _sp_case, cfg, edit_mask, f32, flash_conf, make_dit, prompts, rel, source_latent, tiny_dit, Wrapped  # noqa: E402

FLASH = flash_conf()
SHAPE = (3, 8, 12, 16)


@pytest.fixture(scope="module")
def edit_golden():
    from safetensors.torch import load_file
    g = dict(load_file(os.path.join(GOLDEN, "dit_tiny_edit.safetensors")))
    g["edit.source"] = g["edit.source"].float()
    return g, json.load(open(os.path.join(GOLDEN, "dit_tiny_edit_meta.json")))


run_generate = functools.partial(kit.run_generate, steps=4, shape=SHAPE, pos=POS)


def kept_exact(out, source, mask):
    keep = (mask == 1).expand_as(source)
    return torch.equal(out.cpu()[keep], source[keep])


# ------------------------------------------------------------------------------------------ kernels


def renoise_ref(x0, eps, sigma):
    """the torch expression the kernel is held to: three separately rounded fp32 ops"""
    a = f32(np.float32(1.0) - np.float32(sigma))
    return a * x0 + f32(sigma) * eps


@pytest.mark.parametrize("dims", [(3, 8, 12, 16), (5, 10, 14, 16)])
@pytest.mark.parametrize("sigma", [0.0, 0.37, 1.0])
def test_renoise_bit_exact(dims, sigma):
    from kandinsky import _engine as E
    n = int(np.prod(dims))
    g = torch.Generator().manual_seed(n)
    x0, eps = (torch.randn(n, generator=g) * 3).cuda(), torch.randn(n, generator=g).cuda()
    out = torch.full((n + 64,), 7.0, device="cuda")                     # a guard region after the output
    E.check(E.lib().k5_edit_renoise(out.data_ptr(), x0.data_ptr(), eps.data_ptr(), sigma, n, E.stream_ptr()), "k5_edit_renoise")
    torch.cuda.synchronize()
    assert torch.equal(out[:n], renoise_ref(x0, eps, sigma))
    assert (out[n:] == 7.0).all()
    if sigma == 1.0:
        assert torch.equal(out[:n], eps)
    if sigma == 0.0:
        assert torch.equal(out[:n], x0)
    assert torch.equal(E.renoise(x0.view(dims), eps.view(dims), sigma).view(-1), out[:n])


@pytest.mark.parametrize("dims", [(3, 8, 12, 16), (5, 10, 14, 16)])
@pytest.mark.parametrize("sigma", [0.0, 0.37, 1.0])
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_cfg_euler_edit_bit_exact(dims, sigma, w):
    from kandinsky import _engine as E
    n, cells, Cc = int(np.prod(dims)), int(np.prod(dims[:-1])), dims[-1]
    g = torch.Generator().manual_seed(n + int(w))
    img, x0, eps = torch.randn(n, generator=g).cuda(), (torch.randn(n, generator=g) * 3).cuda(), torch.randn(n, generator=g).cuda()
    c, u = torch.randn(n, generator=g).cuda().to(BF), (torch.randn(n, generator=g).cuda().to(BF) if w != 1.0 else None)
    mask = torch.tensor([0.0, 1.0, 0.25])[torch.randint(0, 3, (cells,), generator=g)].cuda()
    assert all((mask == v).any() for v in (0.0, 1.0, 0.25))
    dt = f32(-0.0625 * 1.3)
    v = c if u is None else u + w * (c - u)                             # eager bf16: every op rounds
    x = img + (dt * v.float()).to(BF).float()
    known = renoise_ref(x0, eps, sigma)
    m = mask.repeat_interleave(Cc)
    want = torch.where(m == 1, known, torch.where(m == 0, x, x + m * (known - x)))
    buf = torch.full((n + 64,), 7.0, device="cuda")
    buf[:n] = img
    E.check(E.lib().k5_cfg_euler_edit(buf.data_ptr(), c.data_ptr(), E.ptr(u), w, dt, x0.data_ptr(), eps.data_ptr(), mask.data_ptr(), sigma,
                                      cells, Cc, E.stream_ptr()), "k5_cfg_euler_edit")
    torch.cuda.synchronize()
    assert torch.equal(buf[:n], want)
    assert (buf[n:] == 7.0).all()
    if sigma == 0.0:
        assert torch.equal(buf[:n][m == 1], x0[m == 1])
    # no mask: the bits of k5_cfg_euler, through the raw entry point and the helper
    plain, nomask = img.clone(), img.clone()
    E.cfg_euler_(plain, c, u, w, dt)
    assert torch.equal(plain, x)
    E.check(E.lib().k5_cfg_euler_edit(nomask.data_ptr(), c.data_ptr(), E.ptr(u), w, dt, None, None, None, sigma, cells, Cc, E.stream_ptr()),
            "k5_cfg_euler_edit")
    assert torch.equal(nomask, plain)
    helper = img.clone().view(dims)
    E.cfg_euler_edit_(helper, c.view(dims), None if u is None else u.view(dims), w, dt, x0.view(dims), eps.view(dims), mask.view(*dims[:-1], 1), sigma)
    assert torch.equal(helper.view(-1), want)
    # a mask without source / noise is refused
    assert E.lib().k5_cfg_euler_edit(nomask.data_ptr(), c.data_ptr(), E.ptr(u), w, dt, None, None, mask.data_ptr(), sigma, cells, Cc, E.stream_ptr()) == 1


# ------------------------------------------------------------------------------------------ sampler: same bits
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_full_strength_without_a_mask_is_the_plain_run(tiny_dit, golden, w):
    plain = run_generate(tiny_dit, golden, w)
    edited = run_generate(tiny_dit, golden, w, init_latent=source_latent(), strength=1.0)
    assert torch.equal(edited, plain)


@pytest.mark.parametrize("cond", [False, True])
def test_fused_equals_stepwise_and_kept_cells_are_the_source(tiny_dit, golden, cond):
    src, mask = source_latent(), edit_mask()
    kw = dict(init_latent=src, strength=0.5, keep_mask=mask)
    if cond:
        g = torch.Generator().manual_seed(11)
        vc, vm = torch.zeros(SHAPE), torch.zeros(*SHAPE[:-1], 1)
        vc[0], vm[0] = torch.randn(SHAPE[1:], generator=g), 1.0
        kw.update(visual_cond=vc, visual_cond_mask=vm)
    for w in (1.0, 5.0):
        a = run_generate(tiny_dit, golden, w, **kw)
        b = run_generate(Wrapped(tiny_dit), golden, w, **kw)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)
        assert kept_exact(a, src, mask)
        free = (mask == 0).expand_as(src)
        assert rel(a.cpu()[free], src[free]) > 1e-2                       # the free region was generated, not copied
        if cond:
            assert not torch.equal(a, run_generate(tiny_dit, golden, w, init_latent=src, strength=0.5, keep_mask=mask))


def oracle_edit(sd, cfg, noise, source, mask, steps, first, w, s, te, ne, mode):
    """the edit loop written around the oracle's get_velocity (conditioning channels zero, as the reference's loop has them)"""
    sig = O.sigma_schedule(steps, s)
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)

    def known_at(sg):
        return (1 - sg) * source + sg * noise
    img = known_at(sig[first])
    for i in range(first, steps):
        v = O.get_velocity(sd, cfg, torch.cat([img, *zeros], -1), sig[i].unsqueeze(0), te, ne, POS, torch.arange(7), torch.arange(4), w,
                           (1.0, 2.0, 2.0), None, mode)
        img = img + O._r((sig[i + 1] - sig[i]) * v, mode)
        known = known_at(sig[i + 1])
        img = torch.where(mask == 1, known, torch.where(mask == 0, img, img + mask * (known - img)))
    return img


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_parity_with_the_oracle_and_the_reference_golden(tiny_dit, tiny_sd, cfg, golden, edit_golden, w):
    from kandinsky.generation_utils import edit_first_step
    g, meta = edit_golden
    src, mask = g["edit.source"], g["edit.mask"]
    steps, s, strength = meta["steps"], meta["scheduler_scale"], meta["strength"]
    assert edit_first_step(steps, strength) == meta["first"]
    out = run_generate(tiny_dit, golden, w, steps=steps, init_latent=src, strength=strength, keep_mask=mask)
    te, ne = prompts(golden)
    tec, nec = {k: v.cpu() for k, v in te.items()}, {k: v.cpu() for k, v in ne.items()}
    ref16 = oracle_edit(tiny_sd, O.DitConfig(**cfg), golden["gen.noise"], src, mask, steps, meta["first"], w, s, tec, nec, "bf16")
    r16, r32 = rel(out, ref16), rel(out, g[f"edit.{w}.final"])
    print(f"edit w={w}: engine vs bf16 oracle {r16:.3e}, vs reference golden {r32:.3e}")
    assert r16 <= 1e-2, r16
    assert r32 <= 3e-2, r32
    assert kept_exact(out, src, mask)


# ------------------------------------------------------------------------------------------ modes
@pytest.mark.parametrize("w,sp", [(1.0, False), (5.0, False), (3.0, True)])
def test_graph_captured_edit_step_is_bit_identical(cfg, tiny_sd, golden, w, sp):
    from kandinsky.generation_utils import generate
    te, ne = prompts(golden)
    shape, pos = (SHAPE, POS) if not sp else ((2, 16, 16, 16), [torch.arange(2), torch.arange(8), torch.arange(8)])
    g = torch.Generator().manual_seed(9)
    noise = golden["gen.noise"] if not sp else torch.randn(*shape, generator=g)
    src, mask = source_latent(shape), edit_mask(shape)
    outs = []
    for graph in (False, True):
        dit = make_dit(cfg, tiny_sd)
        dit.engine("cuda:0")
        if sp:
            dit.enable_sequence_parallel(0, 1, device="cuda:0")
        dit.set_graph(graph)
        outs.append(generate(dit, "cuda:0", shape, 6, te, ne, pos, torch.arange(7), torch.arange(4), w, 5.0, FLASH, noise=noise,
                             init_latent=src, keep_mask=mask))
        del dit
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    assert kept_exact(outs[1], src, mask)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("P,w,mode", [(2, 1.0, 0), (4, 5.0, 0), (2, 5.0, 1)])     # mode: engine option sp_mode (0 gather, 1 Ulysses)
def test_loopback_ranks_edit(tiny_sd, cfg, P, w, mode):
    from test_gpu_loopback import run_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne, src, mask = _sp_case()
    pos = [torch.arange(8)] * 3

    def call(d, r):
        return generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), w, 5.0, FLASH, noise=noise, init_latent=src,
                        strength=0.75, keep_mask=mask)

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    fused = call(make(), 0)
    outs = run_ranks(P, make, call, options={"sp_mode": mode} if mode else None)
    for r in range(P):
        assert torch.equal(outs[r], outs[0])
        assert kept_exact(outs[r], src, mask)
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("Psp", [1, 2])
def test_cfg_pair_in_the_engine_edit(tiny_sd, cfg, Psp):
    from test_gpu_loopback import run_cfg_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne, src, mask = _sp_case()
    pos = [torch.arange(8)] * 3

    def call(d, i):
        return generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, init_latent=src,
                        strength=0.75, keep_mask=mask)

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    fused = call(make(), 0)
    outs = run_cfg_ranks(Psp, make, call)
    for i in range(2 * Psp):
        assert torch.equal(outs[i], outs[0]), f"handle {i} differs from handle 0"
        assert kept_exact(outs[i], src, mask)
    if Psp == 1:
        assert torch.equal(outs[0], fused)
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)


@pytest.mark.timeout(600)
def test_two_ipc_processes_edit(tmp_path, cfg, tiny_sd):
    """Two processes under torch.distributed.run (IPC transport): both ranks end with the same latent, the kept cells are the source,
    within the suite's tolerance of the single-handle run."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from edit_rank_worker import STEPS, STRENGTH
    from kandinsky.generation_utils import generate
    out = str(tmp_path / "ipc")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port",
           str(port), os.path.join(ROOT, "tests", "edit_rank_worker.py"), "--out", out]
    env = dict(os.environ, K5_SP_TRANSPORT="ipc", K5_OVERSUBSCRIBE="1", K5_IPC_TIMEOUT_S="120",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    pr = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        log, _ = pr.communicate(timeout=420)
    except subprocess.TimeoutExpired:
        import signal
        os.killpg(pr.pid, signal.SIGKILL)
        log, _ = pr.communicate()
        pytest.fail(f"2 ranks did not finish:\n{log[-3000:]}")
    assert pr.returncode == 0, f"torch.distributed.run exited with {pr.returncode}:\n{log[-4000:]}"
    lat = [torch.load(os.path.join(out, f"latent_rank{r}.pt")) for r in range(2)]
    assert torch.equal(lat[0], lat[1])
    shape, noise, te, ne, src, mask = _sp_case()
    assert kept_exact(lat[0], src, mask)
    fused = generate(make_dit(cfg, tiny_sd), "cuda:0", shape, STEPS, te, ne, [torch.arange(8)] * 3, torch.arange(9), torch.arange(4), 5.0, 5.0,
                     FLASH, noise=noise, init_latent=src, strength=STRENGTH, keep_mask=mask)
    assert rel(lat[0], fused) <= 1e-2, rel(lat[0], fused)


def test_magcache_with_a_mask(tiny_sd, cfg, golden):
    from kandinsky.generation_utils import generate
    from kandinsky.magcache_utils import set_magcache_params, disable_magcache, magcache_state
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    te, ne = prompts(golden)
    src, mask = source_latent(), edit_mask()
    args = ("cuda:0", SHAPE, c["num_steps"], te, ne, POS, torch.arange(7), torch.arange(4), c["guidance_weight"], c["scheduler_scale"], FLASH)
    try:
        set_magcache_params(dit, c["ratios"], c["num_steps"], c["no_cfg"])
        out = generate(dit, *args, noise=golden["gen.noise"], init_latent=src, keep_mask=mask)
        _, ran, skipped = magcache_state(dit)
        assert skipped > 0
        with pytest.raises(ValueError, match="step of a full run"):
            generate(dit, *args, noise=golden["gen.noise"], init_latent=src, strength=0.5, keep_mask=mask)
    finally:
        disable_magcache(dit)
    assert torch.isfinite(out).all() and kept_exact(out, src, mask)
    plain = generate(dit, *args, noise=golden["gen.noise"], init_latent=src, keep_mask=mask)
    assert rel(out, plain) > 1e-4                                     # the cache was really applied


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(tiny_dit, cfg, tiny_sd, golden):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule
    from kandinsky.models.dit import DiffusionTransformer3D
    te, ne = prompts(golden)
    sig = sigma_schedule(2, 5.0).tolist()
    lat = golden["gen.noise"].cuda().contiguous()
    before = lat.clone()
    src, eps, mask = source_latent().cuda(), golden["gen.noise"].cuda().contiguous(), edit_mask().cuda()
    call = lambda d, **kw: d.sample(lat, sig, te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0), **kw)   # noqa: E731
    bad = {"missing source": (None, eps, mask), "shape": (src[:2].contiguous(), eps, mask), "cpu": (src.cpu(), eps, mask),
           "dtype": (src, eps.bfloat16(), mask), "strided": (src.transpose(1, 2).contiguous().transpose(1, 2), eps, mask),
           "mask channels": (src, eps, mask.expand(-1, -1, -1, 16).contiguous()), "pair": (src, eps)}
    for name, e in bad.items():
        with pytest.raises(ValueError):
            call(tiny_dit, edit=e)
    # the C entry point itself
    s = E.SampleArgs()
    keepalive = []
    s.fwd = tiny_dit._forward_args((3, 8, 12), None, 16, te["text_embeds"], te["pooled_embed"], 0.0, POS, torch.arange(7), (1.0, 2.0, 2.0), None,
                                   keepalive)
    arr = (C.c_float * 3)(*sig)
    s.latent, s.num_steps, s.sigmas, s.guidance_weight = lat.data_ptr(), 2, arr, 1.0
    h = tiny_dit.engine(lat.device)
    edit = lambda a, b, m: C.byref(E.EditArgs(a, b, m))    # noqa: E731
    cases = {"source and noise": edit(None, eps.data_ptr(), None), "source and noise ": edit(src.data_ptr(), None, mask.data_ptr()),
             "source overlaps latent": edit(lat.data_ptr(), eps.data_ptr(), None),
             "noise overlaps latent": edit(src.data_ptr(), lat.data_ptr() + 4 * (lat.numel() - 1), None),
             "keep_mask overlaps latent": edit(src.data_ptr(), eps.data_ptr(), lat.data_ptr() + 64),
             "aligned": edit(src.data_ptr() + 2, eps.data_ptr(), None)}
    for msg, e in cases.items():
        assert E.lib().k5_sample_edit(h, C.byref(s), None, e, E.stream_ptr()) == 1, msg
        assert msg.strip().encode() in E.lib().k5_last_error(), (msg, E.lib().k5_last_error())
    # visual_cond on a visual_cond = 0 handle
    nc = DiffusionTransformer3D(**dict(cfg, visual_cond=False))
    sd = dict(tiny_sd)
    sd["visual_embeddings.in_layer.weight"] = sd["visual_embeddings.in_layer.weight"][:, :64].contiguous()
    nc.load_state_dict(sd, assign=True)
    nc = nc.to("cuda:0")
    c17 = torch.zeros(3, 8, 12, 17, device="cuda")
    with pytest.raises(ValueError, match="visual_cond"):
        call(nc, visual_cond=c17, edit=(src, eps, mask))
    assert E.lib().k5_sample_edit(nc.engine(lat.device), C.byref(s), c17.data_ptr(), edit(src.data_ptr(), eps.data_ptr(), None), E.stream_ptr()) == 1
    assert b"visual_cond = 0" in E.lib().k5_last_error()
    torch.cuda.synchronize()
    assert torch.equal(lat, before)


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_null_edit_is_k5_sample_cond(tiny_dit, golden, w):
    from kandinsky import _engine as E
    plain = run_generate(tiny_dit, golden, w)
    orig = E.lib().k5_sample
    E.lib().k5_sample = lambda h, s, st: E.lib().k5_sample_edit(h, s, None, None, st)
    try:
        via_null = run_generate(tiny_dit, golden, w)
    finally:
        E.lib().k5_sample = orig
    assert torch.equal(via_null, plain)


# ------------------------------------------------------------------------------------------ pipeline end to end
def test_pipeline_video_to_video_end_to_end():
    from test_pipeline import StubTextEmbedder, make_conf
    from kandinsky.conditioning import pixel_mask_to_latent, preprocess_video
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
    F = 4 * (frames - 1) + 1
    clip = torch.randint(0, 256, (F + 3, 150, 210, 3), generator=g, dtype=torch.uint8)    # longer than needed, another size
    keep = torch.zeros(512, 512)
    keep[:, :256] = 1.0

    seen = {}
    enc, samp = vae.encode, dit.sample

    def spy_encode(x, *a, **k):
        seen.setdefault("enc_x", x.clone())
        return enc(x, *a, **k)

    def spy_sample(*a, **k):
        seen["edit"] = k.get("edit")
        seen["sigmas"] = list(a[1])
        return samp(*a, **k)

    vae.encode, dit.sample = spy_encode, spy_sample
    pipe = Kandinsky5T2VPipeline({"dit": dev, "vae": dev, "text_embedder": dev}, dit=dit, text_embedder=StubTextEmbedder(), vae=vae, conf=conf)
    kw = dict(time_length=1, width=512, height=512, seed=7, expand_prompts=False, scheduler_scale=5.0, num_steps=4)
    out = pipe("a cat in a blue hat", video=clip, strength=0.5, mask=keep, **kw)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, 3, F, 512, 512)
    assert torch.equal(seen["enc_x"].cpu(), preprocess_video(clip[:F], 512, 512).permute(1, 0, 2, 3)[None])
    src, eps, km = seen["edit"]
    assert tuple(src.shape) == (frames, 64, 64, 16) and tuple(eps.shape) == tuple(src.shape)
    assert torch.equal(km.cpu(), pixel_mask_to_latent(keep, frames, 512, 512))
    assert len(seen["sigmas"]) == 3                                   # 2 of the 4 steps run
    full = pipe("a cat in a blue hat", video=clip, strength=1, mask=None, **kw)
    assert len(seen["sigmas"]) == 5 and seen["edit"][2] is None
    plain = pipe("a cat in a blue hat", **kw)
    assert seen["edit"] is None
    vae.encode, dit.sample = enc, samp
    assert torch.equal(full, plain)
    assert not torch.equal(out, plain)
    with pytest.raises(ValueError, match="video"):
        pipe("a cat in a blue hat", strength=0.5, **kw)
    with pytest.raises(ValueError, match="pixel frames"):
        pipe("a cat in a blue hat", video=clip[:F - 1], **kw)
