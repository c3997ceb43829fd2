"""MagCache calibration on the MI355X: the fused residual + statistics pass against numpy, and the engine's calibrating mode on the
tiny model against the bf16 oracle and the fixture made from the reference's own residuals (tests/golden/magcache_calib_tiny.*),
through both sampler paths, with averaging, the refusals, image-to-video through the pipeline, and once at full width.

Yardstick of the ratio comparisons (DESIGN.md §2 form): dist(a, b) = |a - b|_2 / |b|_2 over the table of mean ratios;
    engine vs bf16 oracle          <= 1.5 x dist(bf16 oracle, fp32 reference)   — a second bf16 realisation of the same function
    engine vs the fp32 reference   <= 3   x dist(bf16 oracle, fp32 reference)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
from test_magcache_calib_host import POS, case_inputs, load_fixture, oracle_calibration  # noqa: E402
from kit import K5_ERR_ALIGN, K5_ERR_ARG, K5_ERR_STATE, cfg, rel  # noqa: E402


def dist(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def bf(x):
    return x.bfloat16().cuda()


# ------------------------------------------------------------------------------------------ kernel
def numpy_stats(res, prev):
    """float64 on the bf16 values: (sum rho, sum rho^2, sum (1 - cos), rows counted) over the rows with both norms non-zero"""
    r, p = res.float().cpu().double().numpy(), prev.float().cpu().double().numpy()
    nr, npv = np.sqrt((r * r).sum(-1)), np.sqrt((p * p).sum(-1))
    ok = (nr > 0) & (npv > 0)
    rho = nr[ok] / npv[ok]
    cos = (r[ok] * p[ok]).sum(-1) / (nr[ok] * npv[ok])
    return np.array([rho.sum(), (rho * rho).sum(), (1.0 - cos).sum(), float(ok.sum())])


KERNEL_CASES = [(n, D, has_prev, alias, False) for n, D in ((72, 128), (1000, 1792), (4099, 1792)) for has_prev in (True, False)
                for alias in (False, True)] + [(1000, 1792, True, False, True)]   # the last: 5 all-zero rows planted in prev, 3 in vis - ori


@pytest.mark.parametrize("n,D,has_prev,alias,planted", KERNEL_CASES)
def test_stats_kernel_vs_numpy(n, D, has_prev, alias, planted):
    from kandinsky import _engine as E
    g = torch.Generator().manual_seed(n + D + 7 * alias)
    vis, ori, prev = (torch.randn(n, D, generator=g).bfloat16() for _ in range(3))
    prev = prev * 1.3
    if planted:
        zp, zr = torch.randperm(n, generator=g)[:8].split([5, 3])
        prev[zp] = 0
        vis[zr] = ori[zr]                                   # vis - ori = 0 on 3 other rows
    vis, ori, prev = vis.cuda(), ori.cuda(), (prev.cuda() if has_prev else None)
    gate = torch.full((D,), -1.0, device="cuda")
    want_res = E.gate_sum(vis, ori, gate)                   # today's MagCache residual: bf16(vis + (-1) * ori)
    assert torch.equal(want_res, (vis.float() - ori.float()).bfloat16())
    ori_in = ori.clone()
    res, sums = E.magcache_stats(vis, ori_in, prev, out=ori_in if alias else None)
    torch.cuda.synchronize()
    assert torch.equal(res.view(torch.int16), want_res.view(torch.int16))
    if alias:
        assert res.data_ptr() == ori_in.data_ptr()
    else:
        assert torch.equal(ori_in, ori)
    got = sums.cpu().numpy()
    if not has_prev:
        assert np.array_equal(got, np.zeros(4))
        return
    want = numpy_stats(want_res, prev)
    assert got[3] == want[3] == (n - 8 if planted else n)
    errs = np.abs(got[:3] - want[:3]) / np.abs(want[:3])
    print(f"stats ({n}, {D}) alias={alias} planted={planted}: relative error of sum rho / sum rho^2 / sum (1 - cos) = "
          f"{errs[0]:.2e} / {errs[1]:.2e} / {errs[2]:.2e}")
    # fp32 row sums over D terms: at most ~D * 2^-24 relative per row (1.1e-4 at D = 1792); the float64 sum over rows adds nothing visible
    assert errs.max() <= 2e-4, errs
    res2, sums2 = E.magcache_stats(vis, ori.clone(), prev)   # a second launch: identical bits
    assert torch.equal(sums2.view(torch.int64), sums.view(torch.int64)) and torch.equal(res2.view(torch.int16), res.view(torch.int16))


def test_stats_kernel_odd_width_and_arguments():
    """D a multiple of 8 that is no multiple of 64, and one above the four-chunk burst (2048): the chunk loop's tail and second round"""
    from kandinsky import _engine as E
    g = torch.Generator().manual_seed(5)
    for n, D in ((37, 8), (130, 200), (9, 2560)):
        vis, ori, prev = (bf(torch.randn(n, D, generator=g)) for _ in range(3))
        res, sums = E.magcache_stats(vis, ori, prev)
        assert torch.equal(res, (vis.float() - ori.float()).bfloat16())
        want = numpy_stats(res, prev)
        got = sums.cpu().numpy()
        assert got[3] == n and (np.abs(got[:3] - want[:3]) / np.abs(want[:3])).max() <= 2e-4
    x = bf(torch.randn(4, 12))
    s = torch.zeros(4, dtype=torch.float64, device="cuda")
    assert E.lib().k5_magcache_stats_bf16(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), s.data_ptr(), 4, 12, E.stream_ptr()) == K5_ERR_ALIGN
    assert E.lib().k5_magcache_stats_bf16(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), s.data_ptr(), 0, 16, E.stream_ptr()) == K5_ERR_ARG


# ------------------------------------------------------------------------------------------ engine, tiny model


def fresh_dit(cfg, tiny_sd):
    from kandinsky.models.dit import DiffusionTransformer3D
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    dit = DiffusionTransformer3D(**cfg)
    dit.load_state_dict(tiny_sd, assign=True)
    dit = dit.to("cuda:0")
    dit.engine("cuda:0")
    return dit


def conf_ns():
    from types import SimpleNamespace as NS
    return NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))


def run_generate(dit, c, te, ne, noise, vc, mask, steps=None):
    from kandinsky.generation_utils import generate
    return generate(dit, "cuda:0", tuple(noise.shape), steps or c["num_steps"], {k: v.cuda() for k, v in te.items()},
                    {k: v.cuda() for k, v in ne.items()}, POS, torch.arange(7), torch.arange(4), c["guidance_weight"],
                    c["scheduler_scale"], conf_ns(), noise=noise, visual_cond=None if vc is None else vc.cuda(),
                    visual_cond_mask=None if mask is None else mask.cuda())


def run_stepwise(dit, c, te, ne, noise, vc, mask):
    """generate's per-step path: dit(...) per forward through k5_dit_forward, the fused CFG + Euler kernel between"""
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule
    img = noise.clone().cuda().contiguous()
    sig = sigma_schedule(c["num_steps"], c["scheduler_scale"]).tolist()
    zc = torch.zeros_like(img) if vc is None else vc.cuda()
    zm = torch.zeros(*img.shape[:-1], 1, device="cuda") if mask is None else mask.cuda()
    dit.reset_softmax_memory()
    for i in range(c["num_steps"]):
        x = torch.cat([img, zc, zm], dim=-1)
        t = torch.tensor([sig[i]]) * 1000
        v = dit(x, te["text_embeds"].cuda(), te["pooled_embed"].cuda(), t, POS, torch.arange(7), scale_factor=(1.0, 2.0, 2.0))
        u = None
        if not c["no_cfg"]:
            u = dit(x, ne["text_embeds"].cuda(), ne["pooled_embed"].cuda(), t, POS, torch.arange(4), scale_factor=(1.0, 2.0, 2.0))
        E.cfg_euler_(img, v.contiguous(), u, c["guidance_weight"], sig[i + 1] - sig[i])
    return img


def cond_ratios(table, c):
    """the entries of a `mag_ratios` list the fixture has values for: all of them, or the cond half with no_cfg"""
    t = np.asarray(table, dtype=np.float64)
    assert len(t) == 2 * (c["num_steps"] - 1)
    if c["no_cfg"]:
        assert np.array_equal(t[0::2], t[1::2])
        return t[0::2]
    return t


@pytest.mark.parametrize("tag", ["cfg", "nocfg", "cond"])
def test_engine_calibration_vs_oracle_and_reference(cfg, tiny_sd, golden, tag):
    from kandinsky.magcache_utils import (magcache_calibration, magcache_calibration_sums, start_magcache_calibration,
                                          stop_magcache_calibration)
    T, meta = load_fixture()
    c = [c for c in meta["cases"] if c["tag"] == tag][0]
    te, ne, noise, vc, mask = case_inputs(golden, c)
    # the bf16 oracle first: no row of any residual is zero, so every row must be counted
    calls, st16, final16, _ = oracle_calibration(tiny_sd, O.DitConfig(**cfg), noise, c["num_steps"], te, ne, c["guidance_weight"],
                                                 c["scheduler_scale"], "bf16", vc, mask)
    assert calls == c["calls"] and st16[:, 3].sum() == 0

    plain = run_generate(fresh_dit(cfg, tiny_sd), c, te, ne, noise, vc, mask)
    dit = fresh_dit(cfg, tiny_sd)
    start_magcache_calibration(dit, c["num_steps"], c["no_cfg"])
    out = run_generate(dit, c, te, ne, noise, vc, mask)
    assert torch.equal(out, plain)                                     # calibrating changes no bit of the result
    d = magcache_calibration(dit)
    fused_sums, runs = magcache_calibration_sums(dit)
    assert runs == 1 == d["runs"]
    assert d["rows_counted"] == d["rows_total"] == c["rows_per_call"] * 2 * (c["num_steps"] - 1)
    assert np.array_equal(fused_sums[:2], np.zeros((2, 4)))            # a slot's first call has nothing to compare with
    if c["no_cfg"]:
        assert np.array_equal(fused_sums[1::2], np.zeros((c["num_steps"], 4)))
    got = cond_ratios(d["mag_ratios"], c)
    ref32 = T[f"calib.{tag}.ratio"].numpy()
    yard = dist(st16[:, 0], ref32)
    d16, d32 = dist(got, st16[:, 0]), dist(got, ref32)
    print(f"calibration {tag}: bf16 oracle vs fp32 reference {yard:.3e} (yardstick), engine vs bf16 oracle {d16:.3e} "
          f"({d16 / yard:.2f} x), engine vs fp32 reference {d32:.3e} ({d32 / yard:.2f} x)")
    assert d16 <= 1.5 * yard, (d16, yard)
    assert d32 <= 3.0 * yard, (d32, yard)
    assert rel(out, final16) <= 1e-2 and rel(out, T[f"calib.{tag}.final"]) <= 3e-2

    # stepwise (k5_dit_forward per call) == fused (k5_sample): the same table, bit for bit
    stop_magcache_calibration(dit)
    start_magcache_calibration(dit, c["num_steps"], c["no_cfg"])
    out_sw = run_stepwise(dit, c, te, ne, noise, vc, mask)
    step_sums, runs = magcache_calibration_sums(dit)
    assert runs == 1 and np.array_equal(step_sums.view(np.int64), fused_sums.view(np.int64))
    assert rel(out_sw, out) <= 1e-2
    stop_magcache_calibration(dit)
    with pytest.raises(RuntimeError, match="start_magcache_calibration"):
        magcache_calibration(dit)
    assert torch.equal(run_generate(dit, c, te, ne, noise, vc, mask), plain)   # and off again: the plain path


def test_two_runs_are_averaged(cfg, tiny_sd, golden):
    from kandinsky.magcache_utils import magcache_calibration, magcache_calibration_sums, start_magcache_calibration
    T, meta = load_fixture()
    c = [c for c in meta["cases"] if c["tag"] == "cfg"][0]
    te, ne, noise, _, _ = case_inputs(golden, c)
    noise2 = torch.randn(noise.shape, generator=torch.Generator().manual_seed(99))
    single = []
    for nz in (noise, noise2):
        dit = fresh_dit(cfg, tiny_sd)
        start_magcache_calibration(dit, c["num_steps"], False)
        run_generate(dit, c, te, ne, nz, None, None)
        s, runs = magcache_calibration_sums(dit)
        assert runs == 1
        single.append(s)
    assert not np.array_equal(single[0], single[1])
    dit = fresh_dit(cfg, tiny_sd)
    start_magcache_calibration(dit, c["num_steps"], False)
    run_generate(dit, c, te, ne, noise, None, None)
    run_generate(dit, c, te, ne, noise2, None, None)
    both, runs = magcache_calibration_sums(dit)
    assert runs == 2
    np.testing.assert_allclose(both, single[0] + single[1], rtol=1e-14, atol=0)   # float64 additions of the same per-call sums
    d = magcache_calibration(dit)
    want = (single[0][2:, 0] + single[1][2:, 0]) / (single[0][2:, 3] + single[1][2:, 3])
    np.testing.assert_allclose(d["mag_ratios"], want, rtol=1e-14)
    assert d["runs"] == 2 and d["rows_counted"] == d["rows_total"] == 2 * 72 * 18


def test_calibrate_then_use(cfg, tiny_sd, golden):
    """the measured table fed to set_magcache_params: the engine's ran / skipped pattern is O.MagCache's on the same table and the final latent
    meets the oracle tolerance of tests/test_gpu_dit.py::test_magcache_generate (1e-2 on a final latent)"""
    from kandinsky.magcache_utils import (disable_magcache, magcache_calibration, magcache_state, set_magcache_params,
                                          start_magcache_calibration, stop_magcache_calibration)
    T, meta = load_fixture()
    c = [c for c in meta["cases"] if c["tag"] == "cfg"][0]
    te, ne, noise, _, _ = case_inputs(golden, c)
    dit = fresh_dit(cfg, tiny_sd)
    start_magcache_calibration(dit, c["num_steps"], False)
    run_generate(dit, c, te, ne, noise, None, None)
    table = magcache_calibration(dit)["mag_ratios"]
    stop_magcache_calibration(dit)
    set_magcache_params(dit, table, c["num_steps"], False)
    try:
        out = run_generate(dit, c, te, ne, noise, None, None)
        cnt, ran, skipped = magcache_state(dit)
    finally:
        disable_magcache(dit)
    mc = O.MagCache(table, c["num_steps"], False)
    ref16 = O.generate(tiny_sd, O.DitConfig(**cfg), noise, c["num_steps"], te, ne, POS, torch.arange(7), torch.arange(4), c["guidance_weight"],
                       c["scheduler_scale"], (1.0, 2.0, 2.0), None, "bf16", magcache=mc)
    print(f"calibrate then use: ran {ran}, skipped {skipped}; oracle ran {sum(mc.ran_blocks)} of {len(mc.ran_blocks)}; latent vs oracle {rel(out, ref16):.3e}")
    assert (cnt, ran, skipped) == (0, sum(mc.ran_blocks), len(mc.ran_blocks) - sum(mc.ran_blocks))
    assert rel(out, ref16) <= 1e-2, rel(out, ref16)


def test_refusals_enqueue_nothing(cfg, tiny_sd, golden):
    from kandinsky import _engine as E
    from kandinsky.magcache_utils import magcache_calibration_sums, set_magcache_params, start_magcache_calibration, stop_magcache_calibration
    L = E.lib()
    T, meta = load_fixture()
    c = [c for c in meta["cases"] if c["tag"] == "cfg"][0]
    te, ne, noise, _, _ = case_inputs(golden, c)
    # calibrate + MagCache, either order
    dit = fresh_dit(cfg, tiny_sd)
    start_magcache_calibration(dit, 10, False)
    t = np.ones(20)
    assert L.k5_dit_set_magcache(dit._handle, t.ctypes.data_as(C.POINTER(C.c_double)), 20, 0, 0.12, 2, 0.2) == K5_ERR_STATE
    assert b"calibrat" in L.k5_last_error()
    stop_magcache_calibration(dit)
    set_magcache_params(dit, [1.0] * 18, 10, False)
    assert L.k5_dit_set_magcache_calibrate(dit._handle, 10, 0) == K5_ERR_STATE
    assert b"MagCache" in L.k5_last_error()
    with pytest.raises(RuntimeError, match="disable_magcache"):
        start_magcache_calibration(dit, 10, False)
    assert L.k5_dit_magcache_calibration(dit._handle, None, 0, None, None) == K5_ERR_STATE
    # a sequence-parallel loopback group
    group = E.LoopbackGroup(1)
    sp = fresh_dit(cfg, tiny_sd)
    sp.enable_loopback(group, 0)
    assert L.k5_dit_set_magcache_calibrate(sp._handle, 10, 0) == K5_ERR_STATE
    assert b"sequence-parallel" in L.k5_last_error()
    # k5_sample_many / k5_dit_forward_many on a calibrating handle: refused, the latents keep their bits and the table stays empty
    dit = fresh_dit(cfg, tiny_sd)
    start_magcache_calibration(dit, c["num_steps"], False)
    assert not dit.many_ready()
    lat = noise.clone().cuda()[None].contiguous()
    before = lat.clone()
    with pytest.raises(RuntimeError, match="calibrating"):
        dit.sample_many(lat, [1.0, 0.5, 0.0], [{k: v.cuda() for k, v in te.items()}], [{k: v.cuda() for k, v in ne.items()}], POS,
                        [torch.arange(7)], [torch.arange(4)], 2.0, scale_factor=(1.0, 2.0, 2.0))
    torch.cuda.synchronize()
    assert torch.equal(lat, before)
    sums, runs = magcache_calibration_sums(dit)
    assert runs == 0 and not sums.any()
    # a forward of another token count in the middle of a run
    x = torch.cat([noise, torch.zeros(3, 8, 12, 17)], dim=-1).cuda()
    args = (te["text_embeds"].cuda(), te["pooled_embed"].cuda(), torch.tensor([900.0]))
    for _ in range(2):
        dit(x, *args, POS, torch.arange(7), scale_factor=(1.0, 2.0, 2.0))
    with pytest.raises(RuntimeError, match="residual elements"):
        dit(x[:2].contiguous(), *args, [torch.arange(2), torch.arange(4), torch.arange(6)], torch.arange(7), scale_factor=(1.0, 2.0, 2.0))
    stop_magcache_calibration(dit)


def test_pipeline_image_to_video_calibration():
    """calibrate_magcache(pipe, [prompt], image=...) on the tiny checkpoints of the pipeline tests: a table of the right length, every row counted,
    and the DiT's MagCache state as it was found (off -> off; a table set before -> the same table, still in force)"""
    from test_pipeline import StubTextEmbedder, make_conf
    from kandinsky import _engine as E
    from kandinsky.magcache_utils import calibrate_magcache, disable_magcache, magcache_state, set_magcache_params
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
    pipe = Kandinsky5T2VPipeline({"dit": dev, "vae": dev, "text_embedder": dev}, dit=dit, text_embedder=StubTextEmbedder(), vae=vae, conf=conf)
    kw = dict(time_length=1, width=512, height=512, seed=7, expand_prompts=False, scheduler_scale=5.0)
    steps = conf.model.num_steps                                       # 3 steps, guidance 4: CFG
    d = calibrate_magcache(pipe, ["a cat in a blue hat"], image=image, **kw)
    assert len(d["mag_ratios"]) == 2 * (steps - 1) and d["runs"] == 1 and not d["no_cfg"]
    assert d["rows_counted"] == d["rows_total"] == 7 * 32 * 32 * 2 * (steps - 1)
    assert all(0.2 < r < 5.0 for r in d["mag_ratios"])
    assert getattr(dit, "mag_ratios", None) is None and getattr(dit, "_magcache_calibrate", None) is None
    plain = calibrate_magcache(pipe, ["a cat in a blue hat"], **kw)    # text-to-video: another workload, another table
    assert plain["mag_ratios"] != d["mag_ratios"]
    two = calibrate_magcache(pipe, ["a cat in a blue hat", "a dog"], image=image, **kw)
    assert two["runs"] == 2 and two["rows_counted"] == 2 * d["rows_counted"]
    set_magcache_params(dit, d["mag_ratios"], steps, False)
    try:
        table = dit.mag_ratios.copy()
        again = calibrate_magcache(pipe, ["a cat in a blue hat"], image=image, **kw)
        assert again["mag_ratios"] == d["mag_ratios"]                  # the same workload measures the same table, bit for bit
        assert np.array_equal(dit.mag_ratios, table) and dit._magcache_calibrate is None
        # MagCache is in force again on the handle: it answers for its state, with fresh counters, and refuses a second calibration mode
        # (a 3-step table is nothing to sample with: its first eligible call is a slot's first call, which has no residual to re-apply)
        assert magcache_state(dit) == (0, 0, 0)
        assert E.lib().k5_dit_set_magcache_calibrate(dit._handle, steps, 0) == K5_ERR_STATE
    finally:
        disable_magcache(dit)


def test_full_width_calibration_vs_oracle():
    """D = 1792, 2 visual blocks, the (5, 16, 16) latent of test_gpu_dit.py's full-width forward, 4 steps without CFG: the production row length
    through the engine path.  Rule (a) with the fp32 oracle as the fp32 reference (no reference fixture exists at this width)."""
    from kandinsky.models.dit import DiffusionTransformer3D
    from kandinsky.generation_utils import generate
    from kandinsky.magcache_utils import magcache_calibration, start_magcache_calibration
    c = dict(O.LITE_2B, num_visual_blocks=2, num_text_blocks=1)
    ocfg = O.DitConfig(**c)
    sd = O.synthetic_state_dict(ocfg, seed=3)
    dit = DiffusionTransformer3D(**c)
    dit.load_state_dict(sd, assign=True)
    dit = dit.to("cuda:0")
    g = torch.Generator().manual_seed(11)
    noise = torch.randn(5, 16, 16, 16, generator=g)
    te = {"text_embeds": torch.randn(37, 3584, generator=g), "pooled_embed": torch.randn(1, 768, generator=g)}
    pos = [torch.arange(5), torch.arange(8), torch.arange(8)]
    steps, w, s = 4, 1.0, 5.0
    stats = {}
    for mode in ("bf16", "fp32"):
        calls, st, _, _ = oracle_calibration(sd, ocfg, noise, steps, te, te, w, s, mode, pos=pos, tpos=torch.arange(37), ntpos=torch.arange(37))
        assert calls == [2, 4, 6] and st[:, 3].sum() == 0
        stats[mode] = st[:, 0]
    start_magcache_calibration(dit, steps, True)
    tec = {k: v.cuda() for k, v in te.items()}
    generate(dit, "cuda:0", tuple(noise.shape), steps, tec, tec, pos, torch.arange(37), torch.arange(37), w, s, conf_ns(), noise=noise)
    d = magcache_calibration(dit)
    assert d["rows_counted"] == d["rows_total"] == 320 * 2 * (steps - 1)
    got = np.asarray(d["mag_ratios"])[0::2]
    yard, d16 = dist(stats["bf16"], stats["fp32"]), dist(got, stats["bf16"])
    print(f"full-width calibration: bf16 oracle vs fp32 oracle {yard:.3e} (yardstick), engine vs bf16 oracle {d16:.3e} ({d16 / yard:.2f} x)")
    assert d16 <= 1.5 * yard, (d16, yard)
