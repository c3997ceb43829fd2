"""Visual conditioning (image-to-video) on the MI355X: the two-source patchify kernel, k5_sample_cond through every mode of the fused
sampler, the 1-frame VAE encode and the pipeline's `image=` end to end.

Tolerances are those of tests/test_gpu_dit.py: a final latent within relative L2 1e-2 of the bf16-island oracle and 3e-2 of the
reference's fp32 golden (tools/gen_golden_visual_cond.py); a VAE encode within 2e-2 (tests/test_gpu_vae_enc.py).  Everything that
claims "the same computation" is asserted bit for bit."""
import json
import os
import socket
import subprocess
import sys
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
import kit  # noqa: E402
from kit import GOLDEN, POS, ROOT, cfg, flash_conf, make_dit, prompts, rel, tiny_dit, Wrapped  # noqa: E402

FLASH = flash_conf()


@pytest.fixture(scope="module")
def vc_golden(golden):
    """tests/golden/dit_tiny_visual_cond.safetensors expanded: the full conditioning tensors (the stored latent on frame 0, mask 1
    there, zeros elsewhere), the inputs in fp32 and the w = 5 trajectory ending at its final latent."""
    from safetensors.torch import load_file
    g = dict(load_file(os.path.join(GOLDEN, "dit_tiny_visual_cond.safetensors")))
    for pre, shape in (("cond", golden["gen.noise"].shape), ("nabla", golden["gen.nabla.noise"].shape)):
        vc, mask = torch.zeros(shape), torch.zeros(*shape[:-1], 1)
        vc[0], mask[0] = g[pre + ".visual_cond0"].float(), 1.0
        g[pre + ".visual_cond"], g[pre + ".mask"] = vc, mask
    g["enc.x"], g["enc.tiled.x"] = g["enc.x"].float(), g["enc.tiled.x"].float()
    tag = "cond.4_5.0_5.0"
    g[tag + ".latents"] = torch.cat([g[tag + ".latents"], g[tag + ".final"][None]])
    return g


@pytest.fixture(scope="module")
def vc_meta():
    return json.load(open(os.path.join(GOLDEN, "dit_tiny_visual_cond_meta.json")))


def cond17(vc_golden, prefix="cond"):
    return torch.cat([vc_golden[f"{prefix}.visual_cond"], vc_golden[f"{prefix}.mask"]], -1).cuda().contiguous()


def run_generate(model, golden, vc_golden, w, steps=4, **kw):
    return kit.run_generate(model, golden, w, steps=steps, shape=(3, 8, 12, 16), pos=POS, **kw)


def conditioned_oracle(sd, cfg, noise, steps, w, s, te, ne, pos, vc, mask, mode, attention=None):
    img = noise.clone().float()
    sparse = O.get_sparse_params(attention or {"type": "flash"}, img.shape, cfg.patch_size)
    sig = O.sigma_schedule(steps, s)
    for i in range(steps):
        v = O.get_velocity(sd, cfg, torch.cat([img, vc, mask], -1), sig[i].unsqueeze(0), te, ne, pos, torch.arange(7), torch.arange(4), w,
                           (1.0, 2.0, 2.0), sparse, mode)
        img = img + O._r((sig[i + 1] - sig[i]) * v, mode)
    return img


# ------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("T,H,W,fractal", [(3, 8, 12, False),       # 72 tokens: not a multiple of 256
                                           (5, 10, 14, False),      # 175 tokens, odd patch grid
                                           (6, 32, 32, True),       # NABLA fractal order
                                           (6, 32, 32, False)])
def test_patchify_cond_bit_exact_vs_patchify_of_the_concatenation(golden, T, H, W, fractal):
    from kandinsky import _engine as E
    g = torch.Generator().manual_seed(T * 1000 + H)
    x = (torch.randn(T, H, W, 16, generator=g) * 3).cuda()
    vc = (torch.randn(T, H, W, 17, generator=g) * 3).cuda()
    cat = torch.cat([x, vc], -1).contiguous()
    N, Kpad = T * (H // 2) * (W // 2), 136
    perm = golden["fractal.perm.6x16x16"].to(torch.int32).cuda() if fractal else None
    pptr = perm.data_ptr() if fractal else None
    want = torch.full((N, Kpad), 7.0, dtype=torch.bfloat16, device="cuda")
    got = torch.full((N + 1, Kpad), 7.0, dtype=torch.bfloat16, device="cuda")     # one guard row after the output
    E.check(E.lib().k5_patchify_bf16(cat.data_ptr(), want.data_ptr(), T, H, W, 33, 33, Kpad, pptr, E.stream_ptr()), "k5_patchify_bf16")
    E.check(E.lib().k5_patchify_cond_bf16(x.data_ptr(), vc.data_ptr(), got.data_ptr(), T, H, W, 16, 33, Kpad, pptr, E.stream_ptr()),
            "k5_patchify_cond_bf16")
    torch.cuda.synchronize()
    assert torch.equal(got[:N].view(torch.int16), want.view(torch.int16))
    assert (got[N] == 7.0).all()                                              # nothing written past the last row
    assert (got[:N, 132:] == 0).all()                                         # pad columns zeroed
    # refusals: no conditioning pointer, conditioning wider than the input layer, odd H
    assert E.lib().k5_patchify_cond_bf16(x.data_ptr(), None, got.data_ptr(), T, H, W, 16, 33, Kpad, pptr, E.stream_ptr()) == 1
    assert E.lib().k5_patchify_cond_bf16(x.data_ptr(), vc.data_ptr(), got.data_ptr(), T, H, W, 33, 33, Kpad, pptr, E.stream_ptr()) == 1
    assert E.lib().k5_patchify_cond_bf16(x.data_ptr(), vc.data_ptr(), got.data_ptr(), T, H - 1, W, 16, 33, Kpad, pptr, E.stream_ptr()) == 1


# ------------------------------------------------------------------------------------------ sampler: same bits, parity, no change without it
@pytest.mark.parametrize("w", [1.0, 5.0])
def test_fused_sample_equals_stepwise_generate_and_parity(tiny_dit, tiny_sd, cfg, golden, vc_golden, w):
    vc, mask = vc_golden["cond.visual_cond"], vc_golden["cond.mask"]
    a = run_generate(tiny_dit, golden, vc_golden, w, visual_cond=vc.cuda(), visual_cond_mask=mask.cuda())
    b = run_generate(Wrapped(tiny_dit), golden, vc_golden, w, visual_cond=vc.cuda(), visual_cond_mask=mask.cuda())
    assert torch.equal(a, b)
    # the same through DiffusionTransformer3D.sample directly
    te, ne = prompts(golden)
    lat = golden["gen.noise"].cuda().contiguous()
    from kandinsky.generation_utils import sigma_schedule
    tiny_dit.sample(lat, sigma_schedule(4, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), w, scale_factor=(1.0, 2.0, 2.0),
                    visual_cond=cond17(vc_golden))
    assert torch.equal(lat, a)
    tec, nec = {k: v.cpu() for k, v in te.items()}, {k: v.cpu() for k, v in ne.items()}
    ref16 = conditioned_oracle(tiny_sd, O.DitConfig(**cfg), golden["gen.noise"], 4, w, 5.0, tec, nec, POS, vc, mask, "bf16")
    r16, r32 = rel(a, ref16), rel(a, vc_golden[f"cond.4_5.0_{w}.final"])
    print(f"conditioned w={w}: engine vs bf16 oracle {r16:.3e}, vs reference golden {r32:.3e}")
    assert r16 <= 1e-2, r16
    assert r32 <= 3e-2, r32


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_no_conditioning_changes_nothing(tiny_dit, golden, vc_golden, w):
    from kandinsky import _engine as E
    plain = run_generate(tiny_dit, golden, vc_golden, w)
    # k5_sample_cond(NULL) == k5_sample: swap the entry point under sample() for this call
    orig = E.lib().k5_sample
    E.lib().k5_sample = lambda h, s, st: E.lib().k5_sample_cond(h, s, None, st)
    try:
        via_null = run_generate(tiny_dit, golden, vc_golden, w)
    finally:
        E.lib().k5_sample = orig
    assert torch.equal(via_null, plain)
    zeros = run_generate(tiny_dit, golden, vc_golden, w, visual_cond=torch.zeros(3, 8, 12, 16), visual_cond_mask=torch.zeros(3, 8, 12, 1))
    assert torch.equal(zeros, plain)
    only_mask = run_generate(tiny_dit, golden, vc_golden, w, visual_cond_mask=vc_golden["cond.mask"])
    cond = run_generate(tiny_dit, golden, vc_golden, w, visual_cond=vc_golden["cond.visual_cond"], visual_cond_mask=vc_golden["cond.mask"])
    assert rel(only_mask, plain) > 1e-4 and rel(cond, plain) > 1e-3 and rel(cond, only_mask) > 1e-3


def test_refusals(tiny_dit, cfg, tiny_sd, golden, vc_golden):
    from kandinsky.generation_utils import sigma_schedule
    te, ne = prompts(golden)
    sig = sigma_schedule(2, 5.0).tolist()
    lat = golden["gen.noise"].cuda().contiguous()
    keep = lat.clone()
    c = cond17(vc_golden)
    bad = {"channels": c[..., :16].contiguous(), "shape": c[:2].contiguous(), "cpu": c.cpu(), "dtype": c.bfloat16(),
           "strided": c.transpose(1, 2).contiguous().transpose(1, 2)}
    for name, v in bad.items():
        with pytest.raises(ValueError):
            tiny_dit.sample(lat, sig, te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0), visual_cond=v)
    assert torch.equal(lat, keep)                                    # nothing ran
    from kandinsky.models.dit import DiffusionTransformer3D
    nc = DiffusionTransformer3D(**dict(cfg, visual_cond=False))
    sd = dict(tiny_sd)
    sd["visual_embeddings.in_layer.weight"] = sd["visual_embeddings.in_layer.weight"][:, :64].contiguous()
    nc.load_state_dict(sd, assign=True)
    nc = nc.to("cuda:0")
    with pytest.raises(ValueError, match="visual_cond"):
        nc.sample(lat, sig, te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0), visual_cond=c)
    with pytest.raises(ValueError, match="visual_cond"):
        run_generate(nc, golden, vc_golden, 5.0, visual_cond=vc_golden["cond.visual_cond"])
    # the C entry point itself: a visual_cond=0 handle and a misaligned pointer are K5_ERR_ARG with a message
    import ctypes as C
    from kandinsky import _engine as E
    s = E.SampleArgs()
    keepalive = []
    s.fwd = nc._forward_args((3, 8, 12), None, 16, te["text_embeds"], te["pooled_embed"], 0.0, POS, torch.arange(7), (1.0, 2.0, 2.0), None,
                             keepalive)
    arr = (C.c_float * 3)(*sig)
    s.latent, s.num_steps, s.sigmas, s.guidance_weight = lat.data_ptr(), 2, arr, 1.0
    assert E.lib().k5_sample_cond(nc.engine(lat.device), C.byref(s), c.data_ptr(), E.stream_ptr()) == 1
    assert b"visual_cond = 0" in E.lib().k5_last_error()
    assert E.lib().k5_sample_cond(tiny_dit.engine(lat.device), C.byref(s), c.data_ptr() + 2, E.stream_ptr()) == 1
    assert b"aligned" in E.lib().k5_last_error()
    torch.cuda.synchronize()
    assert torch.equal(lat, keep)


# ------------------------------------------------------------------------------------------ modes
def test_nabla_conditioned_vs_reference_golden(cfg, tiny_sd, golden, vc_golden, vc_meta):
    from kandinsky.generation_utils import generate
    c = vc_meta["nabla_case"]
    dit = make_dit(cfg, tiny_sd)
    te, ne = prompts(golden)
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(**c["attention"])), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    pos = [torch.arange(6), torch.arange(16), torch.arange(16)]
    out = generate(dit, "cuda:0", (6, 32, 32, 16), c["steps"], te, ne, pos, torch.arange(7), torch.arange(4), c["guidance_weight"],
                   c["scheduler_scale"], conf, noise=golden["gen.nabla.noise"], visual_cond=vc_golden["nabla.visual_cond"],
                   visual_cond_mask=vc_golden["nabla.mask"])
    plain = generate(dit, "cuda:0", (6, 32, 32, 16), c["steps"], te, ne, pos, torch.arange(7), torch.arange(4), c["guidance_weight"],
                     c["scheduler_scale"], conf, noise=golden["gen.nabla.noise"])
    r = rel(out[:, ::4, ::4], vc_golden["nabla.final.sample"])          # every 4th row and column of the reference's final latent
    ss = out.double().pow(2).sum().item()
    assert abs(ss - c["final_sumsq"]) <= 3e-2 * c["final_sumsq"], (ss, c["final_sumsq"])
    print(f"NABLA conditioned: engine vs reference golden {r:.3e}; unconditioned vs its golden {rel(plain, golden['gen.nabla.final']):.3e}")
    assert r <= 3e-2, r
    assert rel(out, plain) > 1e-3


def test_magcache_conditioned(tiny_sd, cfg, golden, vc_golden):
    """The conditioned twin of test_gpu_dit.py::test_magcache_generate ("hand_10"): the engine under MagCache against the bf16-island
    oracle running the same state machine on the conditioned input."""
    from kandinsky.magcache_utils import set_magcache_params, disable_magcache, magcache_state
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    vc, mask = vc_golden["cond.visual_cond"], vc_golden["cond.mask"]
    from kandinsky.generation_utils import generate
    te, ne = prompts(golden)
    try:
        set_magcache_params(dit, c["ratios"], c["num_steps"], c["no_cfg"])
        out = generate(dit, "cuda:0", (3, 8, 12, 16), c["num_steps"], te, ne, POS, torch.arange(7), torch.arange(4), c["guidance_weight"],
                       c["scheduler_scale"], FLASH, noise=golden["gen.noise"], visual_cond=vc, visual_cond_mask=mask)
        _, ran, skipped = magcache_state(dit)
        assert skipped > 0
    finally:
        disable_magcache(dit)
    mc = O.MagCache(c["ratios"], c["num_steps"], c["no_cfg"])
    ocfg = O.DitConfig(**cfg)
    img = golden["gen.noise"].clone()
    sig = O.sigma_schedule(c["num_steps"], c["scheduler_scale"])
    tec, nec = {k: v.cpu() for k, v in te.items()}, {k: v.cpu() for k, v in ne.items()}
    for i in range(c["num_steps"]):
        v = O.get_velocity(tiny_sd, ocfg, torch.cat([img, vc, mask], -1), sig[i].unsqueeze(0), tec, nec, POS, torch.arange(7),
                           torch.arange(4), c["guidance_weight"], (1.0, 2.0, 2.0), None, "bf16", magcache=mc)
        img = img + O._r((sig[i + 1] - sig[i]) * v, "bf16")
    assert rel(out, img) <= 1e-2, rel(out, img)
    plain = generate(dit, "cuda:0", (3, 8, 12, 16), c["num_steps"], te, ne, POS, torch.arange(7), torch.arange(4), c["guidance_weight"],
                     c["scheduler_scale"], FLASH, noise=golden["gen.noise"], visual_cond=vc, visual_cond_mask=mask)
    assert rel(out, plain) > 1e-4                                     # the cache was really applied


@pytest.mark.parametrize("w,sp", [(1.0, False), (5.0, False), (3.0, True)])
def test_graph_captured_conditioned_step_is_bit_identical(cfg, tiny_sd, golden, vc_golden, w, sp):
    from kandinsky.generation_utils import generate
    te, ne = prompts(golden)
    shape, pos = ((3, 8, 12, 16), POS) if not sp else ((2, 16, 16, 16), [torch.arange(2), torch.arange(8), torch.arange(8)])
    g = torch.Generator().manual_seed(9)
    noise = golden["gen.noise"] if not sp else torch.randn(*shape, generator=g)
    vc = vc_golden["cond.visual_cond"] if not sp else torch.randn(*shape, generator=g)
    mask = vc_golden["cond.mask"] if not sp else torch.rand(*shape[:-1], 1, generator=g)
    outs = []
    for graph in (False, True):
        dit = make_dit(cfg, tiny_sd)
        dit.engine("cuda:0")
        if sp:
            dit.enable_sequence_parallel(0, 1, device="cuda:0")
        dit.set_graph(graph)
        outs.append(generate(dit, "cuda:0", shape, 6, te, ne, pos, torch.arange(7), torch.arange(4), w, 5.0, FLASH, noise=noise,
                             visual_cond=vc, visual_cond_mask=mask))
        del dit
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def _sp_case():
    g = torch.Generator().manual_seed(5)
    shape = (8, 16, 16, 16)
    noise = torch.randn(*shape, generator=g)
    te = {"text_embeds": torch.randn(9, 96, generator=g).cuda(), "pooled_embed": torch.randn(1, 48, generator=g).cuda()}
    ne = {"text_embeds": torch.randn(4, 96, generator=g).cuda(), "pooled_embed": torch.randn(1, 48, generator=g).cuda()}
    vc = torch.zeros(shape)
    vc[0] = torch.randn(shape[1:], generator=g)
    mask = torch.zeros(*shape[:-1], 1)
    mask[0] = 1.0
    return shape, noise, te, ne, vc, mask


@pytest.mark.timeout(600)
@pytest.mark.parametrize("P,w,mode", [(2, 1.0, 0), (4, 5.0, 0), (2, 5.0, 1)])     # mode: engine option sp_mode (0 gather, 1 Ulysses)
def test_loopback_ranks_conditioned(golden_meta, tiny_sd, cfg, P, w, mode):
    """The conditioned twin of test_gpu_loopback.py::test_tiny_sampler_P_ranks_on_one_gpu: every rank ends with the same latent, within
    the suite's tolerance of the single-handle run, and away from the unconditioned one."""
    from test_gpu_loopback import run_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne, vc, mask = _sp_case()
    pos = [torch.arange(8)] * 3

    def call(d, r, cond=True):
        kw = dict(visual_cond=vc, visual_cond_mask=mask) if cond else {}
        return generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), w, 5.0, FLASH, noise=noise, **kw)

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    fused = call(make(), 0)
    outs = run_ranks(P, make, call, options={"sp_mode": mode} if mode else None)
    for r in range(1, P):
        assert torch.equal(outs[r], outs[0])
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)
    assert rel(fused, call(make(), 0, cond=False)) > 1e-3


@pytest.mark.timeout(900)
@pytest.mark.parametrize("Psp", [1, 2])
def test_cfg_pair_in_the_engine_conditioned(tiny_sd, cfg, Psp):
    """The conditioned twin of test_gpu_loopback.py::test_tiny_cfg_parallel_inside_the_engine: both branches see the conditioning;
    Psp = 1 equals the single-handle CFG run bit for bit."""
    from test_gpu_loopback import run_cfg_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne, vc, mask = _sp_case()
    pos = [torch.arange(8)] * 3

    def call(d, i):
        return generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise,
                        visual_cond=vc, visual_cond_mask=mask)

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    fused = call(make(), 0)
    outs = run_cfg_ranks(Psp, make, call)
    for i in range(1, 2 * Psp):
        assert torch.equal(outs[i], outs[0]), f"handle {i} differs from handle 0"
    if Psp == 1:
        assert torch.equal(outs[0], fused)
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)


@pytest.mark.timeout(600)
def test_two_ipc_processes_conditioned(tmp_path, cfg, tiny_sd):
    """Two processes under torch.distributed.run (IPC transport), conditioned: both ranks end with the same latent, within the suite's
    tolerance of the single-handle run."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from visual_cond_rank_worker import case
    from kandinsky.generation_utils import generate
    out = str(tmp_path / "ipc")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port",
           str(port), os.path.join(ROOT, "tests", "visual_cond_rank_worker.py"), "--out", out]
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
    shape, noise, te, ne, vc, mask = case()
    te = {k: v.cuda() for k, v in te.items()}
    ne = {k: v.cuda() for k, v in ne.items()}
    fused = generate(make_dit(cfg, tiny_sd), "cuda:0", shape, 4, te, ne, [torch.arange(8)] * 3, torch.arange(9), torch.arange(4), 5.0, 5.0,
                     FLASH, noise=noise, visual_cond=vc, visual_cond_mask=mask)
    assert rel(lat[0], fused) <= 1e-2, rel(lat[0], fused)


# ------------------------------------------------------------------------------------------ 1-frame VAE encode
ENC_CFG = dict(latent_channels=16, out_channels=3, block_out_channels=(64, 64, 128, 128), layers_per_block=2, norm_num_groups=16)


@pytest.fixture(scope="module")
def enc_vae():
    """The engine packs channels in multiples of 64, so the golden's 16 / 32-channel encoder cannot run on it: the engine is held to the
    oracle at 64 / 128 channels (as in tests/test_gpu_vae_enc.py), and the oracle to the reference's 1-frame goldens at the tiny widths
    (tests/test_visual_cond.py).  Same inputs and tilings as those goldens."""
    from kandinsky.models.vae import AutoencoderKLHunyuanVideo
    m = AutoencoderKLHunyuanVideo(**ENC_CFG)
    g = torch.Generator().manual_seed(15)
    sd = {}
    for k, p in m.state_dict().items():
        if "norm" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.2 * torch.randn(p.shape, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(p.shape, generator=g)
        else:
            sd[k] = torch.randn(p.shape, generator=g) * (1.2 / (p[0].numel() ** 0.5))
    m.load_state_dict(sd, assign=True)
    return m.to("cuda:0"), sd


@pytest.mark.parametrize("tiled", [False, True])
def test_one_frame_encode_vs_oracle(enc_vae, vc_golden, vc_meta, tiled):
    from oracle import vae_oracle as V
    m, sd = enc_vae
    x = vc_golden["enc.tiled.x" if tiled else "enc.x"]
    tile, stride = (tuple(vc_meta["enc_tiled_case"]["tile"]), tuple(vc_meta["enc_tiled_case"]["stride"])) if tiled else \
        ((1, 1) + tuple(x.shape[3:]), (1,) + tuple(x.shape[3:]))
    m.apply_tiling(tile, stride)
    got = m._encode(x.cuda())
    assert tuple(got.shape) == (1, 32, 1, x.shape[3] // 8, x.shape[4] // 8)
    ref16 = V.tiled_encode(sd, x, ENC_CFG, tile, stride, "bf16") if tiled else V.encoder_forward(sd, x, ENC_CFG, "bf16")
    print(f"1-frame encode tiled={tiled}: engine vs bf16 oracle {rel(got, ref16):.3e}")
    assert rel(got, ref16) <= 2e-2, rel(got, ref16)
    if tiled:   # the glue is the oracle's, fed the engine's own tiles: bit for bit
        ref = V.tiled_encode(sd, x, ENC_CFG, tile, stride, "bf16", encode_tile=lambda t: m._encode_tile(t.cuda()).float().cpu())
        assert torch.equal(got.float().cpu(), ref)
    # encode() with the default policy at T = 1 picks one untiled tile here and returns the same moments
    post = m.encode(x.cuda()).latent_dist
    assert torch.equal(post.mean, m._encode_tile(x.cuda())[:, :16])


def test_one_frame_encode_production_width():
    """A 512 x 768 picture through encode() with the default tiling policy at the production channel widths (random weights)."""
    from kandinsky.models.vae import AutoencoderKLHunyuanVideo
    m = AutoencoderKLHunyuanVideo()
    g = torch.Generator().manual_seed(4)
    sd = {}
    for k, p in m.state_dict().items():
        if "norm" in k and k.endswith("weight"):
            sd[k] = torch.ones(p.shape)
        elif k.endswith("bias"):
            sd[k] = torch.zeros(p.shape)
        else:
            sd[k] = torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5)
    m.load_state_dict(sd, assign=True)
    m = m.to("cuda:0")
    x = (torch.rand(1, 3, 1, 512, 768, generator=g) * 2 - 1).cuda()
    post = m.encode(x).latent_dist
    assert tuple(post.mean.shape) == (1, 16, 1, 64, 96)
    assert torch.isfinite(post.mean.float()).all() and post.mean.float().std() > 0


# ------------------------------------------------------------------------------------------ pipeline end to end
def test_pipeline_image_to_video_end_to_end(tmp_path):
    from test_pipeline import StubTextEmbedder, make_conf
    from kandinsky.conditioning import preprocess_image
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
    image = torch.randint(0, 256, (300, 420, 3), generator=g, dtype=torch.uint8)

    seen = {}
    enc, samp = vae.encode, dit.sample

    def spy_encode(x, *a, **k):
        out = enc(x, *a, **k)
        seen.setdefault("enc_x", x.clone())
        seen.setdefault("enc_mean", out.latent_dist.mean.clone())
        return out

    def spy_sample(*a, **k):
        seen["visual_cond"] = None if k.get("visual_cond") is None else k["visual_cond"].clone()
        return samp(*a, **k)

    vae.encode, dit.sample = spy_encode, spy_sample
    pipe = Kandinsky5T2VPipeline({"dit": dev, "vae": dev, "text_embedder": dev}, dit=dit, text_embedder=StubTextEmbedder(), vae=vae, conf=conf)
    kw = dict(time_length=1, width=512, height=512, seed=7, expand_prompts=False, scheduler_scale=5.0)
    out = pipe("a cat in a blue hat", image=image, **kw)
    frames = 24 // 4 + 1
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, 3, 4 * (frames - 1) + 1, 512, 512)
    assert torch.equal(seen["enc_x"].cpu(), preprocess_image(image, 512, 512)[None, :, None])
    vc = seen["visual_cond"]
    assert tuple(vc.shape) == (frames, 64, 64, 17)
    z = (seen["enc_mean"].float() * vae.config.scaling_factor)[0, :, 0].permute(1, 2, 0)
    assert torch.equal(vc[0, ..., :16], z) and vc[1:, ..., :16].abs().sum() == 0
    assert vc[0, ..., 16].eq(1).all() and vc[1:, ..., 16].eq(0).all()
    seen.clear()
    plain = pipe("a cat in a blue hat", **kw)
    assert seen["visual_cond"] is None and "enc_x" not in seen
    vae.encode, dit.sample = enc, samp
    ref = pipe("a cat in a blue hat", **kw)
    assert torch.equal(plain, ref)
    assert not torch.equal(plain, out)
