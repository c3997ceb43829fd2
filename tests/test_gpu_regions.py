"""Regional prompts on the MI355X: the combine kernel and the token-weights pass against their float64 definitions and bit-for-bit
identities, and the regional forward through every way the engine runs it — against the reference's fp32 goldens
(tools/gen_golden_regions.py), against the plain run where the rule is an identity, and against itself where two paths claim the same
computation.

Combine bound, per element: |out - ref| <= 2^-8 |ref| + 2^-20 sum_i |w_i z_i| — bf16's rounding, plus at most 9 fp32 roundings (one product and
up to 8 fmas, each within 2^-24 of a partial sum that sum_i |w_i z_i| bounds).  Weights bound: absolute 16 * 2^-24 — the values lie in [0, 1] and
at most R + 8 <= 16 roundings occur (4 cells and their division, R + 1 additions twice, one subtraction, one division).  Engine parity:
relative L2 <= min(3e-2, delta / 4), 3e-2 being the project's bound against fp32 goldens and delta the golden's own distance from the plain
run, so a build that ignores the regions fails; the run with the two masks swapped must be farther away than delta / 4, so a build with the
wrong token order fails."""
import functools
import json
import os
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

import kit  # noqa: E402
from kit import BF, GOLDEN, POS, cfg, flash_conf, make_dit, prompts, rank_case, rel, tiny_dit  # noqa: E402

FLASH = flash_conf()
SHAPE = (3, 8, 12, 16)

from regions_reference import combine_inputs, combine_reference, mask_cases, nabla_perm, token_weights_reference  # noqa: E402


def bits(t):
    return t.cpu().view(torch.int16)


# ------------------------------------------------------------------------------------------ the combine kernel
def combine(z0, zr, w, D=None, out=None):
    from kandinsky import _engine as E
    r = E.region_combine_(z0, zr, w, out=out, D=D)
    torch.cuda.synchronize()
    return r


def check_against_float64(out, z0, zr, w, what):
    ref, mag = combine_reference(z0, zr, w)
    o = out.double().cpu()
    assert not torch.isnan(o).any()
    err = (o - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * mag
    worst = (err / bound.clamp_min(1e-300)).max().item() if (err > 0).any() else 0.0
    print(f"{what}: worst error / bound {worst:.3f}")
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("rows", [1, 7, 130])
@pytest.mark.parametrize("D", [64, 128, 1792])
def test_combine_against_float64(D, rows, R):
    z0, zr, w = combine_inputs(rows, D, R)
    if rows > 1:
        z0[1, :8] = -0.0                                                   # row 1 is one-hot: the sign of a zero survives
        zr[:, 1, :8] = -0.0
    out = combine(z0.cuda().clone(), zr.cuda(), w.cuda())
    check_against_float64(out, z0, zr, w, f"rows {rows} D {D} R {R}")
    for i in range(1, rows, 3):                                            # one-hot rows: that stream bit for bit
        k = i % (R + 1)
        assert torch.equal(bits(out[i]), bits(z0[i] if k == 0 else zr[k - 1, i])), i


@pytest.mark.parametrize("R", [1, 8])
def test_combine_in_place_twice_and_with_a_row_stride(R):
    rows, D = 130, 1792
    z0, zr, w = combine_inputs(rows, D, R, seed=1)
    z0_d, zr_d, w_d = z0.cuda(), zr.cuda(), w.cuda()
    out_of_place = torch.empty_like(z0_d)
    combine(z0_d, zr_d, w_d, out=out_of_place)
    again = torch.empty_like(z0_d)
    combine(z0_d, zr_d, w_d, out=again)
    assert torch.equal(bits(again), bits(out_of_place))                    # two runs
    in_place = z0_d.clone()
    combine(in_place, zr_d, w_d)
    assert torch.equal(bits(in_place), bits(out_of_place))                 # in place
    assert torch.equal(bits(z0_d), bits(z0)) and torch.equal(bits(zr_d), bits(zr)) and not torch.equal(in_place, z0_d)
    # ld = D + 8, ldw = R + 3: the padding is neither read nor written, and the stride moves no bits
    b0 = torch.full((rows, D + 8), 7.0, dtype=BF, device="cuda")
    br = torch.full((R, rows, D + 8), float("nan"), dtype=BF, device="cuda")
    bo = torch.full((rows, D + 8), 11.0, dtype=BF, device="cuda")
    bw = torch.full((rows, R + 3), float("nan"), device="cuda")
    b0[:, :D], br[:, :, :D], bw[:, :R + 1] = z0_d, zr_d, w_d
    combine(b0, br, bw, D=D, out=bo)
    assert torch.equal(bits(bo[:, :D]), bits(out_of_place))
    assert (bo[:, D:] == 11.0).all() and (b0[:, D:] == 7.0).all() and torch.equal(bits(b0[:, :D]), bits(z0)) and torch.isnan(br[:, :, D:]).all()
    combine(b0, br, bw, D=D)                                               # in place: the bytes between D and ld stay
    assert torch.equal(bits(b0[:, :D]), bits(out_of_place)) and (b0[:, D:] == 7.0).all() and torch.isnan(bw[:, R + 1:]).all()


@pytest.mark.parametrize("D", [128, 1792])
def test_a_zero_weight_stream_is_not_read(D):
    rows, R = 130, 3
    z0, zr, w = combine_inputs(rows, D, R, seed=2)
    clean = combine(z0.cuda().clone(), zr.cuda(), w.cuda())
    poisoned0, poisoned = z0.clone(), zr.clone()
    poisoned0[w[:, 0] == 0] = float("nan")
    for r in range(R):
        poisoned[r, w[:, r + 1] == 0] = float("nan")
    assert torch.isnan(poisoned).any() and torch.isnan(poisoned0).any()
    out = combine(poisoned0.cuda(), poisoned.cuda(), w.cuda(), out=torch.empty(rows, D, dtype=BF, device="cuda"))
    assert not torch.isnan(out).any() and torch.equal(bits(out), bits(clean))


def test_combine_refusals_launch_nothing():
    from kandinsky import _engine as E
    L = E.lib()
    z0 = torch.randn(8, 256, device="cuda").to(BF)
    zr = torch.randn(2, 8, 256, device="cuda").to(BF)
    w = torch.full((8, 3), 1.0 / 3.0, device="cuda")
    out = torch.full((8, 256), 9.0, dtype=BF, device="cuda")
    st = E.stream_ptr()
    good = [z0.data_ptr(), zr.data_ptr(), 8 * 256, 2, w.data_ptr(), 3, out.data_ptr(), 8, 256, 256, st]
    for i, v in ((7, 0), (8, 0), (8, 252), (9, 248), (9, 260), (3, 0), (3, 9), (5, 2), (6, out.data_ptr() + 2), (0, z0.data_ptr() + 8), (1, None),
                 (0, None), (4, None), (6, None), (4, w.data_ptr() + 2), (2, 8 * 256 + 4)):
        a = list(good)
        a[i] = v
        assert L.k5_region_combine_bf16(*a) == 1, (i, v)
        assert "k5_region_combine_bf16" in E.last_error()
    a = list(good)
    a[8] = a[9] = 2056
    assert L.k5_region_combine_bf16(*a) == 6
    torch.cuda.synchronize()
    assert (out == 9.0).all()
    assert L.k5_region_combine_bf16(*good) == 0
    torch.cuda.synchronize()
    assert not (out == 9.0).all()


# ------------------------------------------------------------------------------------------ the token weights
@pytest.mark.parametrize("R", [1, 2, 8])
@pytest.mark.parametrize("shape,order", [((3, 8, 12), "rows"), ((3, 8, 12), "shuffled"), ((2, 16, 16), "rows"), ((2, 16, 16), "nabla"),
                                         ((1, 16, 32), "nabla")])   # (2, 16, 16) is one tile per frame, NABLA's order is the rows'; (1, 16, 32) is two tiles
def test_token_weights_against_float64(shape, order, R):
    from kandinsky import _engine as E
    T, H, W = shape
    N = T * (H // 2) * (W // 2)
    perm = {"rows": None, "nabla": nabla_perm(T, H // 2, W // 2) if order == "nabla" else None,
            "shuffled": torch.randperm(N, generator=torch.Generator().manual_seed(9)).int()}[order]
    masks = mask_cases(R, T, H, W)
    worst = 0.0
    for bw in (0.0, 0.5, 1.0):
        w = E.region_weights(masks.cuda(), (1, 2, 2), bw, perm=None if perm is None else perm.cuda())
        torch.cuda.synchronize()
        ref = token_weights_reference(masks, bw, (1, 2, 2), perm)
        assert w.shape == ref.shape and not torch.isnan(w).any()
        err = (w.double().cpu() - ref).abs().max().item()
        worst = max(worst, err)
        assert err <= 16 * 2.0 ** -24, (bw, err)
    print(f"token weights {shape} {order} R {R}: worst absolute error {worst:.3e} (bound {16 * 2.0 ** -24:.3e})")
    if order == "nabla" and W > 16:
        assert not torch.equal(ref, token_weights_reference(masks, 1.0, (1, 2, 2)))   # the order is there to be lost
    # exact cases: a partition at base_weight 0 is one-hot; all-zero masks are the base prompt only
    if R == 2:
        col = torch.arange(W).expand(T, H, W)
        part = torch.stack([(col < W // 2).float(), (col >= W // 2).float()]).contiguous()
        w = E.region_weights(part.cuda(), (1, 2, 2), 0.0, perm=None if perm is None else perm.cuda()).cpu()
        assert torch.equal(w.double(), token_weights_reference(part, 0.0, (1, 2, 2), perm)) and ((w == 0) | (w == 1)).all()
    w = E.region_weights(torch.zeros(R, T, H, W, device="cuda"), (1, 2, 2), 0.3).cpu()
    assert (w[:, 0] == 1).all() and (w[:, 1:] == 0).all()


def test_token_weights_with_a_temporal_patch():
    from kandinsky import _engine as E
    masks = mask_cases(2, 4, 8, 12, seed=5)
    w = E.region_weights(masks.cuda(), (2, 2, 4), 0.25)
    ref = token_weights_reference(masks, 0.25, (2, 2, 4))
    assert (w.double().cpu() - ref).abs().max().item() <= 24 * 2.0 ** -24    # 16 cells per token: R + 20 <= 24 roundings


# ------------------------------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def reg_golden():
    from safetensors.torch import load_file
    return (dict(load_file(os.path.join(GOLDEN, "dit_tiny_regions.safetensors"))),
            json.load(open(os.path.join(GOLDEN, "dit_tiny_regions_meta.json"))))


def region_kw(g, masks, bw=0.0, swap=False, only=None):
    """generate()'s keywords for the fixture's two region prompts on `masks` (2, T, H, W)"""
    texts = [{"text_embeds": g["regions.text0"].cuda()}, {"text_embeds": g["regions.text1"].cuda()}]
    pos = [torch.arange(5), torch.arange(6)]
    if swap:
        masks = masks.flip(0)
    if only is not None:
        texts, pos, masks = [texts[only]], [pos[only]], masks[only:only + 1]
    return dict(region_text_embeds=texts, region_text_rope_pos=pos, region_masks=masks.contiguous(), region_base_weight=bw)


def set_regions(model, kw):
    return model.set_regions(kw["region_text_embeds"], kw["region_text_rope_pos"], kw["region_masks"], kw["region_base_weight"])


run_generate = functools.partial(kit.run_generate, steps=4, shape=SHAPE, pos=POS)


def forward(model, golden, x=None, neg=False, time=None, te=None, n=None):
    base, ne = prompts(golden)
    p, k = (ne, 4) if neg else (base, 7)
    if te is not None:
        p, k = te, n
    x = golden["fwd.x"].cuda() if x is None else x
    return model(x, p["text_embeds"], p["pooled_embed"], golden["fwd.time"] if time is None else time, POS, torch.arange(k),
                 scale_factor=(1.0, 2.0, 2.0))


def hard_masks():
    col = torch.arange(SHAPE[2]).expand(*SHAPE[:3])
    return torch.stack([(col < 6).float(), (col >= 6).float()])


@pytest.mark.parametrize("case", ["fwd", "gen.1.0", "gen.5.0"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_parity_with_the_fp32_golden(tiny_dit, golden, reg_golden, name, case):
    g, meta = reg_golden
    m = meta["sets"][name]
    delta = m["delta"][case]
    assert delta >= meta["delta_min"] == 0.04, (name, case, delta)
    masks = g[f"regions.{name}.masks"]

    def run(swap):
        kw = region_kw(g, masks, m["base_weight"], swap=swap)
        if case != "fwd":
            return run_generate(tiny_dit, golden, float(case[4:]), **kw)
        set_regions(tiny_dit, kw)
        try:
            return forward(tiny_dit, golden)
        finally:
            tiny_dit.clear_regions()

    out = run(False)
    want = g[f"regions.{name}.fwd.out"] if case == "fwd" else g[f"regions.{name}.{case}.final"]
    plain = golden["fwd.out"] if case == "fwd" else golden[f"gen.4_5.0_{float(case[4:])}.final"]
    assert torch.isfinite(out.float()).all()
    assert abs(rel(want, plain) - delta) <= 1e-6                           # delta is what the fixture says it is
    err, swapped = rel(out, want), rel(run(True), want)
    print(f"regions set {name} {case}: rel L2 to the fp32 golden {err:.3e} (bound {min(3e-2, delta / 4):.3e}, delta {delta:.4f}), masks swapped {swapped:.3e}")
    assert err <= min(3e-2, delta / 4), (err, delta)
    assert swapped > delta / 4, (swapped, delta)
    assert tiny_dit.regions_state()[0] is False and tiny_dit._regions is None


def test_nabla_parity_with_the_fp32_golden(cfg, tiny_sd, golden, golden_meta, reg_golden):
    """the token weights follow the blocks' fractal token order"""
    from kandinsky.generation_utils import generate
    g, meta = reg_golden
    c = meta["nabla"]
    delta = c["delta"]
    assert delta >= meta["delta_min"]
    dit = make_dit(cfg, tiny_sd)
    te, ne = prompts(golden)
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(**golden_meta["nabla_attention"])), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    pos = [torch.arange(6), torch.arange(16), torch.arange(16)]

    def run(**kw):
        return generate(dit, "cuda:0", (6, 32, 32, 16), c["steps"], te, ne, pos, torch.arange(7), torch.arange(4), c["guidance_weight"], 5.0, conf,
                        noise=golden["gen.nabla.noise"], **kw)

    want, plain = g["regions.nabla.final"], golden["gen.nabla.final"]
    assert abs(rel(want, plain) - delta) <= 1e-6
    out = run(**region_kw(g, g["regions.nabla.masks"]))
    err, swapped = rel(out, want), rel(run(**region_kw(g, g["regions.nabla.masks"], swap=True)), want)
    print(f"regions NABLA: rel L2 to the fp32 golden {err:.3e} (bound {min(3e-2, delta / 4):.3e}, delta {delta:.4f}), masks swapped {swapped:.3e}, "
          f"plain run to its golden {rel(run(), plain):.3e}")
    assert torch.isfinite(out).all() and err <= min(3e-2, delta / 4), (err, delta)
    assert swapped > delta / 4, (swapped, delta)
    dit._destroy_engine(force=True)


def test_all_zero_masks_are_the_plain_run(tiny_dit, golden, reg_golden):
    g, _ = reg_golden
    plain_v = forward(tiny_dit, golden)
    plain = {w: run_generate(tiny_dit, golden, w) for w in (1.0, 5.0)}
    kw = region_kw(g, torch.zeros(2, *SHAPE[:3]), 0.5)
    tiny_dit.regions_state(reset=True)
    set_regions(tiny_dit, kw)
    try:
        assert tiny_dit.regions_state() == (True, 2, 0)
        assert torch.equal(forward(tiny_dit, golden), plain_v)
        assert tiny_dit.regions_state() == (True, 2, 2)                    # it ran: one combine per visual block
    finally:
        tiny_dit.clear_regions()
    for w in (1.0, 5.0):
        assert torch.equal(run_generate(tiny_dit, golden, w, **kw), plain[w])
    assert tiny_dit.regions_state(reset=True) == (False, 0, 2 + 2 * 4 * 2)   # the conditional forwards only


def test_a_full_mask_is_a_plain_run_on_the_regions_prompt(tiny_dit, golden, reg_golden):
    g, _ = reg_golden
    base, _ = prompts(golden)
    for r, n in ((0, 5), (1, 6)):
        te = {"text_embeds": g[f"regions.text{r}"].cuda(), "pooled_embed": base["pooled_embed"]}   # the time embedding stays the base prompt's
        plain_v = forward(tiny_dit, golden, te=te, n=n)
        plain = {w: run_generate(tiny_dit, golden, w, te=te, text_pos=torch.arange(n)) for w in (1.0, 5.0)}
        kw = region_kw(g, torch.ones(2, *SHAPE[:3]), 0.0, only=r)
        set_regions(tiny_dit, kw)
        try:
            assert torch.equal(forward(tiny_dit, golden), plain_v)
        finally:
            tiny_dit.clear_regions()
        for w in (1.0, 5.0):
            assert torch.equal(run_generate(tiny_dit, golden, w, **kw), plain[w]), (r, w)
    assert not torch.equal(plain_v, forward(tiny_dit, golden))


def test_clear_restores_the_plain_bits(tiny_dit, golden, reg_golden):
    g, _ = reg_golden
    plain_v, plain = forward(tiny_dit, golden), run_generate(tiny_dit, golden, 1.0)
    kw = region_kw(g, hard_masks())
    set_regions(tiny_dit, kw)
    assert not torch.equal(forward(tiny_dit, golden), plain_v)
    tiny_dit.clear_regions()
    assert tiny_dit.regions_state()[:2] == (False, 0)
    assert torch.equal(forward(tiny_dit, golden), plain_v)
    assert torch.equal(run_generate(tiny_dit, golden, 1.0), plain)
    assert not torch.equal(run_generate(tiny_dit, golden, 1.0, **kw), plain)
    tiny_dit.regions_state(reset=True)
    run_generate(tiny_dit, golden, 5.0)
    forward(tiny_dit, golden)
    assert tiny_dit.regions_state() == (False, 0, 0)                       # without regions the counter stays 0
    run_generate(tiny_dit, golden, 5.0, **kw)
    assert tiny_dit.regions_state(reset=True) == (False, 0, 4 * 2)         # num_visual_blocks per conditional forward, none per unconditional one


def per_step(model, golden, w, steps, kw, regional_uncond=False):
    """the forwards of k5_sample issued one by one through k5_dit_forward, and k5_cfg_euler: the conditional one with the regions, the
    unconditional one plain (regional_uncond: not — the control)"""
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule
    img = golden["gen.noise"].cuda().clone().contiguous()
    ts = sigma_schedule(steps, 5.0, device="cuda:0").cpu()
    zeros = torch.zeros_like(img), torch.zeros(*img.shape[:-1], 1, device="cuda")
    model.reset_softmax_memory()
    u0 = None
    for t, dt in zip(ts[:-1].tolist(), torch.diff(ts).tolist()):
        x = torch.cat([img, *zeros], dim=-1)
        t1000 = torch.tensor([t]) * 1000
        set_regions(model, kw)
        try:
            v = forward(model, golden, x, time=t1000)
            if not regional_uncond:
                model.clear_regions()
            u = forward(model, golden, x, neg=True, time=t1000) if abs(w - 1.0) > 1e-6 else None
        finally:
            model.clear_regions()
        u0 = u if u0 is None else u0
        E.cfg_euler_(img, v.contiguous(), None if u is None else u.contiguous(), w, dt)
    return img, u0


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_one_sample_call_equals_its_forwards_step_by_step(tiny_dit, golden, reg_golden, w):
    g, _ = reg_golden
    for kw in (region_kw(g, hard_masks()), region_kw(g, g["regions.B.masks"], 0.5)):
        fused = run_generate(tiny_dit, golden, w, **kw)
        stepped, _ = per_step(tiny_dit, golden, w, 4, kw)
        assert torch.equal(fused, stepped)


def test_the_unconditional_velocity_is_the_plain_one(tiny_dit, golden, reg_golden):
    """one step at guidance 5: the update k5_sample applied is built from the PLAIN run's unconditional velocity of step 0"""
    g, _ = reg_golden
    kw = region_kw(g, hard_masks())
    fused = run_generate(tiny_dit, golden, 5.0, steps=1, **kw)
    stepped, u = per_step(tiny_dit, golden, 5.0, 1, kw)
    x0 = torch.cat([golden["gen.noise"].cuda(), torch.zeros(*SHAPE[:-1], 17, device="cuda")], dim=-1)
    from kandinsky.generation_utils import sigma_schedule
    t0 = sigma_schedule(1, 5.0, device="cuda:0").cpu()[:1] * 1000
    assert torch.equal(u, forward(tiny_dit, golden, x0, neg=True, time=t0))   # what a plain run computes
    assert torch.equal(fused, stepped)
    control, ug = per_step(tiny_dit, golden, 5.0, 1, kw, regional_uncond=True)
    assert not torch.equal(ug, u) and not torch.equal(control, fused)


def test_the_captured_step_equals_eager(cfg, tiny_sd, golden, reg_golden):
    g, _ = reg_golden
    kw = region_kw(g, g["regions.B.masks"], 0.5)
    outs = []
    for graph in (False, True):
        dit = make_dit(cfg, tiny_sd)
        dit.engine("cuda:0")
        dit.set_graph(graph)
        outs.append([run_generate(dit, golden, w, steps=6, **kw) for w in (1.0, 5.0)])
        assert dit.regions_state() == (False, 0, 2 * 6 * 2)
        dit._destroy_engine(force=True)
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_each_sample_of_a_batch_equals_its_own_call(tiny_dit, golden, reg_golden):
    g, _ = reg_golden
    kw = region_kw(g, hard_masks())
    B = 2
    noise = torch.randn(B * SHAPE[0], *SHAPE[1:], generator=torch.Generator().manual_seed(11))
    for w in (1.0, 5.0):
        tiny_dit.regions_state(reset=True)
        many = run_generate(tiny_dit, golden, w, shape=(B * SHAPE[0],) + SHAPE[1:], noise=noise, batch=B, **kw)
        assert tiny_dit.regions_state(reset=True) == (False, 0, B * 4 * 2)
        for b in range(B):
            own = run_generate(tiny_dit, golden, w, noise=noise[b * SHAPE[0]:(b + 1) * SHAPE[0]], **kw)
            assert torch.equal(many[b * SHAPE[0]:(b + 1) * SHAPE[0]], own), (w, b)
    assert not torch.equal(many, run_generate(tiny_dit, golden, 5.0, shape=(B * SHAPE[0],) + SHAPE[1:], noise=noise, batch=B))


def test_per_block_cross_projections_take_the_same_path(cfg, tiny_sd, golden, reg_golden):
    """engine option cross_kv_batched = 0: the regions' keys / values are projected block by block, like the base prompt's"""
    g, _ = reg_golden
    kw = region_kw(g, g["regions.B.masks"], 0.5)
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    batched = run_generate(dit, golden, 1.0, **kw)
    plain = run_generate(dit, golden, 1.0)
    dit.set_option("cross_kv_batched", 0)
    assert torch.equal(run_generate(dit, golden, 1.0, **kw), batched)
    assert torch.equal(run_generate(dit, golden, 1.0, **region_kw(g, torch.zeros(2, *SHAPE[:3]), 0.5)), plain)
    dit._destroy_engine(force=True)


def test_editing_carries_the_regions(tiny_dit, golden, reg_golden):
    g, _ = reg_golden
    src = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(77))
    mask = torch.zeros(*SHAPE[:-1], 1)
    mask[0] = 1.0
    kw = dict(init_latent=src, strength=0.75, keep_mask=mask)
    plain = run_generate(tiny_dit, golden, 5.0, **kw)
    tiny_dit.regions_state(reset=True)
    assert torch.equal(run_generate(tiny_dit, golden, 5.0, **kw, **region_kw(g, torch.zeros(2, *SHAPE[:3]))), plain)
    assert tiny_dit.regions_state(reset=True) == (False, 0, 3 * 2)         # strength 0.75: 3 of the 4 steps
    out = run_generate(tiny_dit, golden, 5.0, **kw, **region_kw(g, hard_masks()))
    assert not torch.equal(out, plain) and torch.equal(out.cpu()[0], src[0])   # the kept frame is the source


def test_magcache_skips_the_regions_with_the_blocks(cfg, tiny_sd, golden, reg_golden):
    from kandinsky.generation_utils import generate
    from kandinsky.magcache_utils import disable_magcache, magcache_state, set_magcache_params
    g, _ = reg_golden
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "nocfg_9"][0]
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    te, ne = prompts(golden)
    try:
        set_magcache_params(dit, c["ratios"], c["num_steps"], c["no_cfg"])
        out = generate(dit, "cuda:0", SHAPE, c["num_steps"], te, ne, POS, torch.arange(7), torch.arange(4), c["guidance_weight"],
                       c["scheduler_scale"], FLASH, noise=golden["gen.noise"], **region_kw(g, hard_masks()))
        _, ran, skipped = magcache_state(dit)
    finally:
        disable_magcache(dit)
    assert torch.isfinite(out).all() and skipped > 0 and ran + skipped == c["num_steps"]
    assert dit.regions_state() == (False, 0, 2 * ran)                      # a skipped step runs no visual block and so no combine
    dit._destroy_engine(force=True)


def test_with_nag_and_zero_masks_the_run_is_the_nag_run(tiny_dit, golden, reg_golden):
    g, _ = reg_golden
    _, ne = prompts(golden)
    nag = dict(nag_text_embeds=ne, nag_text_rope_pos=torch.arange(4), nag_scale=5.0, nag_tau=2.5, nag_alpha=0.25)
    for w in (1.0, 5.0):
        want = run_generate(tiny_dit, golden, w, **nag)
        tiny_dit.regions_state(reset=True)
        tiny_dit.nag_state(reset=True)
        assert torch.equal(run_generate(tiny_dit, golden, w, **nag, **region_kw(g, torch.zeros(2, *SHAPE[:3]), 1.0)), want)
        assert tiny_dit.regions_state()[2] == 4 * 2 and tiny_dit.nag_state()[1] == 4 * 2
    both = run_generate(tiny_dit, golden, 1.0, **nag, **region_kw(g, hard_masks()))
    assert torch.isfinite(both).all() and not torch.equal(both, want) and not torch.equal(both, run_generate(tiny_dit, golden, 1.0, **region_kw(g, hard_masks())))


# ------------------------------------------------------------------------------------------ ranks


def rank_regions():
    g = torch.Generator().manual_seed(6)
    col = torch.arange(16).expand(8, 16, 16)
    soft = torch.rand(8, 16, 16, generator=g)
    return dict(region_text_embeds=[{"text_embeds": torch.randn(5, 96, generator=g).cuda()}, {"text_embeds": torch.randn(6, 96, generator=g).cuda()}],
                region_text_rope_pos=[torch.arange(5), torch.arange(6)], region_masks=torch.stack([(col < 7).float(), soft * (col >= 5).float()]),
                region_base_weight=0.25)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("P,w,mode", [(2, 5.0, 0), (4, 1.0, 2)])           # sp_mode: 0 gather, 2 two-level (2 heads over 4 ranks)
def test_loopback_ranks(tiny_sd, cfg, P, w, mode):
    from test_gpu_loopback import run_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne = rank_case()
    pos = [torch.arange(8)] * 3
    counts = {}

    def call(d, r, **kw):
        out = generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), w, 5.0, FLASH, noise=noise, **rank_regions(), **kw)
        counts[r] = (d.regions_state()[2], d.get_option("sp_mode_used"))
        return out

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    single = call(make(), -1)
    outs = run_ranks(P, make, call, options={"sp_mode": mode} if mode else None)
    for r in range(P):
        assert torch.equal(outs[r], outs[0]), f"rank {r} differs from rank 0"
        assert counts[r] == (4 * 2, mode), counts
    assert rel(outs[0], single) <= 1e-2, rel(outs[0], single)
    plain = generate(make(), "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), w, 5.0, FLASH, noise=noise)
    assert not torch.equal(single, plain) and not torch.equal(outs[0], plain)   # the regions are there to be lost


@pytest.mark.timeout(900)
def test_cfg_pair_in_the_engine(tiny_sd, cfg):
    """Psp = 1: both handles of the pair end with the single handle's latent bit for bit; both carry the regions, only the conditional one
    runs them"""
    from test_gpu_loopback import run_cfg_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne = rank_case()
    pos = [torch.arange(8)] * 3
    counts = {}

    def call(d, i):
        out = generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, **rank_regions())
        counts[i] = d.regions_state()[2]
        return out

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    fused = call(make(), -1)
    outs = run_cfg_ranks(1, make, call)
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[0], fused)
    assert [counts[0], counts[1]] == [4 * 2, 0]                            # branch 0 = conditional


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_as_it_was(tiny_dit, golden, reg_golden):
    from kandinsky import _engine as E
    g, _ = reg_golden
    plain = run_generate(tiny_dit, golden, 1.0)
    kw = region_kw(g, hard_masks())
    # context windows: the masks cover the clip, a window sees a slice (K5_ERR_STATE from k5_sample_windows)
    shape5 = (5,) + SHAPE[1:]
    noise5 = torch.randn(*shape5, generator=torch.Generator().manual_seed(12))
    set_regions(tiny_dit, region_kw(g, torch.zeros(2, 3, *SHAPE[1:3])))
    try:
        with pytest.raises(RuntimeError, match="regional prompts") as e:
            run_generate(tiny_dit, golden, 1.0, shape=shape5, noise=noise5, context_frames=3, context_overlap=1)
        assert "window" in str(e.value)
    finally:
        tiny_dit.clear_regions()
    with pytest.raises(ValueError, match="window"):
        run_generate(tiny_dit, golden, 1.0, shape=shape5, noise=noise5, context_frames=3, context_overlap=1, **region_kw(g, torch.zeros(2, 5, *SHAPE[1:3])))
    assert torch.equal(run_generate(tiny_dit, golden, 1.0), plain)
    # a shape that is not the masks': the message names both
    other = region_kw(g, torch.zeros(2, 3, 8, 16))
    with pytest.raises(RuntimeError, match=r"\(3, 8, 16\).*\(3, 8, 12\)"):
        run_generate(tiny_dit, golden, 1.0, **other)
    set_regions(tiny_dit, other)
    try:
        with pytest.raises(RuntimeError, match=r"\(3, 8, 16\).*\(3, 8, 12\)"):
            forward(tiny_dit, golden)
    finally:
        tiny_dit.clear_regions()
    assert torch.equal(run_generate(tiny_dit, golden, 1.0), plain)
    # every argument error of k5_dit_set_regions, on a live handle
    h = tiny_dit._handle
    keep = []
    conds = (E.TextCond * 2)(*[tiny_dit._text_cond(t["text_embeds"], torch.zeros(1, 48, device="cuda"), p, keep)
                               for t, p in zip(kw["region_text_embeds"], kw["region_text_rope_pos"])])
    masks = hard_masks().cuda().contiguous()
    good = [h, conds, 2, masks.data_ptr(), 3, 8, 12, 0.0]
    bad_len = (E.TextCond * 2)(conds[0], E.TextCond(conds[1].text_embed, conds[1].pooled_embed, conds[1].text_dtype, 0, conds[1].text_rope_pos))
    no_embed = (E.TextCond * 2)(conds[0], E.TextCond(None, conds[1].pooled_embed, conds[1].text_dtype, 6, conds[1].text_rope_pos))
    no_pos = (E.TextCond * 2)(conds[0], E.TextCond(conds[1].text_embed, conds[1].pooled_embed, conds[1].text_dtype, 6, None))
    for i, v, word in ((2, 9, "R must be"), (7, -0.5, "base_weight"), (7, 1.5, "base_weight"), (7, float("nan"), "base_weight"), (3, None, "masks"),
                       (5, 7, "divisible"), (6, 11, "divisible"), (1, bad_len, "text_len"), (1, no_embed, "text_embed"), (1, no_pos, "text_rope_pos")):
        a = list(good)
        a[i] = v
        assert E.lib().k5_dit_set_regions(*a) == 1, word
        assert word in E.last_error()
        assert tiny_dit.regions_state()[:2] == (False, 0)
        assert torch.equal(run_generate(tiny_dit, golden, 1.0), plain), word
    assert E.lib().k5_dit_set_regions(*good) == 0 and tiny_dit.regions_state()[:2] == (True, 2)
    assert not torch.equal(run_generate(tiny_dit, golden, 1.0), plain)
    tiny_dit.clear_regions()
    assert torch.equal(run_generate(tiny_dit, golden, 1.0), plain)
