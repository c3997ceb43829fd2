"""Normalized attention guidance (NAG) on the MI355X: the combine kernel against the float64 definition and its bit-for-bit identities,
and the guided forward through every way the engine runs it — against the reference's fp32 goldens (tools/gen_golden_nag.py), against
the plain run where the rule is an identity, and against itself where two paths claim the same computation.

Kernel bound, per element: |out - ref| <= 2^-8 |ref| + 2^-12 (|z+| + |f g|) — bf16's half ulp, plus the fp32 chain with worst-case row sums
(D 2^-24 ~ 1.1e-4 at D = 1792, the figure DESIGN.md uses for the row LayerNorm).  Engine parity: relative L2 <= min(3e-2, delta / 4), 3e-2 being
the project's bound against fp32 goldens and delta the golden's own distance from the plain run, so a build that ignores NAG fails."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import kit  # noqa: E402
from kit import BF, GOLDEN, POS, cfg, flash_conf, make_dit, prompts, rank_case, rel, tiny_dit  # noqa: E402

FLASH = flash_conf()
SHAPE = (3, 8, 12, 16)
PARAMS = (5.0, 2.5, 0.25)

from nag_reference import nag_inputs, nag_reference  # noqa: E402


# ------------------------------------------------------------------------------------------ the kernel
def combine(zp, zn, s, tau, alpha, D=None, out=None):
    from kandinsky import _engine as E
    r = E.nag_combine_(zp, zn, s, tau, alpha, out=out, D=D)
    torch.cuda.synchronize()
    return r


def check_against_float64(out, zp, zn, params, rows):
    ref, fg, clamped = nag_reference(zp, zn, *params)
    o = out.double().cpu()
    assert not torch.isnan(o).any()
    err = (o - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -12 * (zp.double().abs() + fg.abs())
    worst = (err / bound.clamp_min(1e-300)).max().item() if (err > 0).any() else 0.0
    print(f"rows {rows} D {zp.shape[1]}: worst error / bound {worst:.3f}, clamped rows {int(clamped.sum())} of {rows}")
    assert (err <= bound).all(), worst
    if rows >= 7:   # both regimes are exercised
        assert clamped.float().mean() >= 0.4 and (~clamped).float().mean() >= 0.4


@pytest.mark.parametrize("rows", [1, 7, 130])
@pytest.mark.parametrize("D", [64, 128, 1792])
def test_combine_against_float64(D, rows):
    zp, zn = nag_inputs(rows, D)
    out = combine(zp.cuda().clone(), zn.cuda(), *PARAMS)
    check_against_float64(out, zp, zn, PARAMS, rows)
    if rows > 3:
        assert (out[3] == 0).all()                                        # z+ = 0: a zero row, not NaN
    if rows > 4:
        assert torch.equal(out[4].cpu(), zp[4])                           # z- = z+


def test_combine_with_a_row_stride():
    rows, D = 130, 1792
    zp, zn = nag_inputs(rows, D)
    bp, bn = torch.full((rows, D + 8), 7.0, dtype=BF, device="cuda"), torch.full((rows, D + 8), -3.0, dtype=BF, device="cuda")
    bp[:, :D], bn[:, :D] = zp.cuda(), zn.cuda()
    bo = torch.full((rows, D + 8), 11.0, dtype=BF, device="cuda")
    combine(bp, bn, *PARAMS, D=D, out=bo)
    check_against_float64(bo[:, :D], zp, zn, PARAMS, rows)
    assert (bo[:, D:] == 11.0).all() and (bp[:, D:] == 7.0).all() and torch.equal(bp[:, :D].cpu(), zp)
    dense = combine(zp.cuda().clone(), zn.cuda(), *PARAMS)
    assert torch.equal(dense, bo[:, :D])                                  # the stride moves no bits
    combine(bp, bn, *PARAMS, D=D)                                         # in place: the bytes between D and ld stay
    assert torch.equal(bp[:, :D], dense) and (bp[:, D:] == 7.0).all() and (bn[:, D:] == -3.0).all()


@pytest.mark.parametrize("D", [128, 1792])
def test_combine_identities_bit_for_bit(D):
    rows = 130
    zp, zn = nag_inputs(rows, D)
    zp[5, :8] = -0.0                                                     # a negative zero keeps its sign
    zp_d, zn_d = zp.cuda(), zn.cuda()

    def bits(t):
        return t.cpu().view(torch.int16)

    for params, neg in (((5.0, 2.5, 0.25), zp_d), ((11.0, 1.0, 1.0), zp_d), ((1.0, 2.5, 0.25), zn_d), ((1.0, 1.0, 1.0), zn_d),
                        ((5.0, 2.5, 0.0), zn_d), ((11.0, 1.0, 0.0), zn_d)):
        out = torch.empty_like(zp_d)
        combine(zp_d, neg, *params, out=out)
        assert torch.equal(bits(out), bits(zp)), params
    out_of_place = torch.empty_like(zp_d)
    combine(zp_d, zn_d, *PARAMS, out=out_of_place)
    again = torch.empty_like(zp_d)
    combine(zp_d, zn_d, *PARAMS, out=again)
    assert torch.equal(bits(again), bits(out_of_place))                   # two runs
    in_place = zp_d.clone()
    combine(in_place, zn_d, *PARAMS)
    assert torch.equal(bits(in_place), bits(out_of_place))                # in place
    assert torch.equal(bits(zp_d), bits(zp)) and not torch.equal(in_place, zp_d)


def test_combine_refusals_launch_nothing():
    from kandinsky import _engine as E
    L = E.lib()
    zp = torch.randn(8, 256, device="cuda").to(BF)
    zn = torch.randn(8, 256, device="cuda").to(BF)
    out = torch.full((8, 256), 9.0, dtype=BF, device="cuda")
    st = E.stream_ptr()
    good = [zp.data_ptr(), zn.data_ptr(), out.data_ptr(), 8, 256, 256, 5.0, 2.5, 0.25, st]
    for i, v in ((3, 0), (4, 252), (5, 248), (5, 260), (6, 0.5), (7, 0.5), (8, 1.5), (8, -0.1), (2, out.data_ptr() + 2), (0, zp.data_ptr() + 8), (1, None)):
        a = list(good)
        a[i] = v
        assert L.k5_nag_combine_bf16(*a) == 1, (i, v)
        assert "k5_nag_combine_bf16" in E.last_error()
    a = list(good)
    a[4] = a[5] = 2056
    assert L.k5_nag_combine_bf16(*a) == 6
    with pytest.raises(RuntimeError, match="k5_nag_combine_bf16"):
        E.nag_combine_(zp, zn, 0.5, 2.5, 0.25, out=out)
    torch.cuda.synchronize()
    assert (out == 9.0).all()
    assert L.k5_nag_combine_bf16(*good) == 0
    torch.cuda.synchronize()
    assert not (out == 9.0).all()


# ------------------------------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def nag_golden():
    from safetensors.torch import load_file
    return dict(load_file(os.path.join(GOLDEN, "dit_tiny_nag.safetensors"))), json.load(open(os.path.join(GOLDEN, "dit_tiny_nag_meta.json")))


def nag_kw(golden, params=PARAMS, positive=False):
    te, ne = prompts(golden)
    s, tau, alpha = params
    return dict(nag_text_embeds=te if positive else ne, nag_text_rope_pos=torch.arange(7 if positive else 4), nag_scale=s, nag_tau=tau, nag_alpha=alpha)


run_generate = functools.partial(kit.run_generate, steps=4, shape=SHAPE, pos=POS)


def forward(model, golden, x=None, neg=False, time=None):
    te, ne = prompts(golden)
    p, n = (ne, 4) if neg else (te, 7)
    x = golden["fwd.x"].cuda() if x is None else x
    return model(x, p["text_embeds"], p["pooled_embed"], golden["fwd.time"] if time is None else time, POS, torch.arange(n),
                 scale_factor=(1.0, 2.0, 2.0))


def set_nag(model, golden, params=PARAMS, positive=False, kw=None):
    k = nag_kw(golden, params, positive) if kw is None else kw
    return model.set_nag(k["nag_text_embeds"], k["nag_text_rope_pos"], k["nag_scale"], k["nag_tau"], k["nag_alpha"])


@pytest.mark.parametrize("case", ["fwd", "gen.1.0", "gen.5.0"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_parity_with_the_fp32_golden(tiny_dit, golden, nag_golden, name, case):
    g, meta = nag_golden
    m = meta["sets"][name]
    delta = m["delta"][case]
    assert delta >= meta["delta_min"] == 0.04, (name, case, delta)
    assert (m["clamped_share"][case] >= 0.5) if name == "A" else (m["clamped_share"][case] <= 0.5)
    params = (m["scale"], m["tau"], m["alpha"])
    if case == "fwd":
        set_nag(tiny_dit, golden, params)
        try:
            out, want = forward(tiny_dit, golden), g[f"nag.{name}.fwd.out"]
        finally:
            tiny_dit.clear_nag()
        plain = golden["fwd.out"]
    else:
        w = float(case[4:])
        out, want = run_generate(tiny_dit, golden, w, **nag_kw(golden, params)), g[f"nag.{name}.{case}.final"]
        plain = golden[f"gen.4_5.0_{w}.final"]
    assert torch.isfinite(out.float()).all()
    assert abs(rel(want, plain) - delta) <= 1e-6                          # delta is what the fixture says it is
    err = rel(out, want)
    print(f"NAG set {name} {case}: rel L2 to the fp32 golden {err:.3e} (bound {min(3e-2, delta / 4):.3e}, delta {delta:.4f})")
    assert err <= min(3e-2, delta / 4), (err, delta)
    assert tiny_dit.nag_state()[0] is False and tiny_dit._nag is None


def test_the_positive_prompt_as_the_negative_is_the_plain_run(tiny_dit, golden):
    plain_v = forward(tiny_dit, golden)
    plain = {w: run_generate(tiny_dit, golden, w) for w in (1.0, 5.0)}
    tiny_dit.nag_state(reset=True)
    set_nag(tiny_dit, golden, positive=True)
    try:
        assert tiny_dit.nag_state() == (True, 0)
        assert torch.equal(forward(tiny_dit, golden), plain_v)
        assert tiny_dit.nag_state() == (True, 2)                          # it ran: one combine per visual block
    finally:
        tiny_dit.clear_nag()
    for w in (1.0, 5.0):
        assert torch.equal(run_generate(tiny_dit, golden, w, **nag_kw(golden, positive=True)), plain[w])
    assert tiny_dit.nag_state(reset=True) == (False, 2 + 2 * 4 * 2)


def test_clear_and_scale_one_restore_the_plain_bits(tiny_dit, golden):
    plain_v, plain = forward(tiny_dit, golden), run_generate(tiny_dit, golden, 1.0)
    set_nag(tiny_dit, golden)
    guided_v = forward(tiny_dit, golden)
    assert not torch.equal(guided_v, plain_v)
    tiny_dit.clear_nag()
    assert torch.equal(forward(tiny_dit, golden), plain_v)
    assert torch.equal(run_generate(tiny_dit, golden, 1.0), plain)
    tiny_dit.nag_state(reset=True)
    for params in ((1.0, 2.5, 0.25), (5.0, 2.5, 0.0)):                    # accepted, and off: nothing runs
        set_nag(tiny_dit, golden, params)
        assert tiny_dit.nag_state() == (False, 0)
        assert torch.equal(forward(tiny_dit, golden), plain_v)
        assert torch.equal(run_generate(tiny_dit, golden, 1.0, **nag_kw(golden, params)), plain)
        tiny_dit.clear_nag()
    assert tiny_dit.nag_state() == (False, 0)
    assert not torch.equal(run_generate(tiny_dit, golden, 1.0, **nag_kw(golden)), plain)


def test_state_counts_the_conditional_forwards_only(tiny_dit, golden):
    tiny_dit.nag_state(reset=True)
    run_generate(tiny_dit, golden, 5.0)
    forward(tiny_dit, golden)
    assert tiny_dit.nag_state() == (False, 0)                             # without NAG the counter stays 0
    run_generate(tiny_dit, golden, 1.0, **nag_kw(golden))
    assert tiny_dit.nag_state(reset=True) == (False, 4 * 2)               # num_visual_blocks per conditional forward
    run_generate(tiny_dit, golden, 5.0, **nag_kw(golden))
    assert tiny_dit.nag_state(reset=True) == (False, 4 * 2)               # ... and none per unconditional one
    assert tiny_dit.nag_state() == (False, 0)


def per_step(model, golden, w, steps, kw=None, guided_uncond=False):
    """the forwards of k5_sample issued one by one through k5_dit_forward, and k5_cfg_euler: the conditional one guided, the
    unconditional one plain (guided_uncond: not — the control)"""
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
        set_nag(model, golden, kw=kw)
        try:
            v = forward(model, golden, x, time=t1000)
            if not guided_uncond:
                model.clear_nag()
            u = forward(model, golden, x, neg=True, time=t1000) if abs(w - 1.0) > 1e-6 else None
        finally:
            model.clear_nag()
        u0 = u if u0 is None else u0
        E.cfg_euler_(img, v.contiguous(), None if u is None else u.contiguous(), w, dt)
    return img, u0


def other_negative(golden):
    """a negative prompt that is not the null prompt (against itself the rule is an identity, and the unconditional forward could hide)"""
    g = torch.Generator().manual_seed(21)
    return dict(nag_kw(golden), nag_text_embeds={"text_embeds": torch.randn(5, 96, generator=g).cuda()}, nag_text_rope_pos=torch.arange(5))


@pytest.mark.parametrize("w", [1.0, 5.0])
def test_one_sample_call_equals_its_forwards_step_by_step(tiny_dit, golden, w):
    for kw in (nag_kw(golden), other_negative(golden)):
        fused = run_generate(tiny_dit, golden, w, **kw)
        stepped, _ = per_step(tiny_dit, golden, w, 4, kw)
        assert torch.equal(fused, stepped)


def test_the_unconditional_velocity_is_the_plain_one(tiny_dit, golden):
    """one step at guidance 5: the update k5_sample applied is the one built from the PLAIN run's unconditional velocity of step 0 (and
    not from a guided one)"""
    kw = other_negative(golden)
    fused = run_generate(tiny_dit, golden, 5.0, steps=1, **kw)
    stepped, u = per_step(tiny_dit, golden, 5.0, 1, kw)
    x0 = torch.cat([golden["gen.noise"].cuda(), torch.zeros(*SHAPE[:-1], 17, device="cuda")], dim=-1)
    from kandinsky.generation_utils import sigma_schedule
    t0 = sigma_schedule(1, 5.0, device="cuda:0").cpu()[:1] * 1000
    assert torch.equal(u, forward(tiny_dit, golden, x0, neg=True, time=t0))   # what a plain run computes
    assert torch.equal(fused, stepped)
    control, ug = per_step(tiny_dit, golden, 5.0, 1, kw, guided_uncond=True)
    assert not torch.equal(ug, u) and not torch.equal(control, fused)


def test_the_captured_step_equals_eager(cfg, tiny_sd, golden):
    outs = []
    for graph in (False, True):
        dit = make_dit(cfg, tiny_sd)
        dit.engine("cuda:0")
        dit.set_graph(graph)
        outs.append([run_generate(dit, golden, w, steps=6, **nag_kw(golden)) for w in (1.0, 5.0)])
        assert dit.nag_state() == (False, 2 * 6 * 2)
        dit._destroy_engine(force=True)
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_each_sample_of_a_batch_equals_its_own_call(tiny_dit, golden):
    B = 2
    noise = torch.randn(B * SHAPE[0], *SHAPE[1:], generator=torch.Generator().manual_seed(11))
    for w in (1.0, 5.0):
        tiny_dit.nag_state(reset=True)
        many = run_generate(tiny_dit, golden, w, shape=(B * SHAPE[0],) + SHAPE[1:], noise=noise, batch=B, **nag_kw(golden))
        assert tiny_dit.nag_state(reset=True) == (False, B * 4 * 2)
        for b in range(B):
            own = run_generate(tiny_dit, golden, w, noise=noise[b * SHAPE[0]:(b + 1) * SHAPE[0]], **nag_kw(golden))
            assert torch.equal(many[b * SHAPE[0]:(b + 1) * SHAPE[0]], own), (w, b)
    assert not torch.equal(many, run_generate(tiny_dit, golden, 5.0, shape=(B * SHAPE[0],) + SHAPE[1:], noise=noise, batch=B))


def test_per_block_cross_projections_take_the_same_path(cfg, tiny_sd, golden):
    """engine option cross_kv_batched = 0: the negative keys / values are projected block by block, like the positive ones"""
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    batched = run_generate(dit, golden, 1.0, **nag_kw(golden))
    plain = run_generate(dit, golden, 1.0)
    dit.set_option("cross_kv_batched", 0)
    assert torch.equal(run_generate(dit, golden, 1.0, **nag_kw(golden)), batched)
    assert torch.equal(run_generate(dit, golden, 1.0, **nag_kw(golden, positive=True)), plain)
    dit._destroy_engine(force=True)


def test_editing_and_context_windows_carry_the_guidance(tiny_dit, golden):
    src = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(77))
    mask = torch.zeros(*SHAPE[:-1], 1)
    mask[0] = 1.0
    kw = dict(init_latent=src, strength=0.75, keep_mask=mask)
    plain = run_generate(tiny_dit, golden, 5.0, **kw)
    tiny_dit.nag_state(reset=True)
    assert torch.equal(run_generate(tiny_dit, golden, 5.0, **kw, **nag_kw(golden, positive=True)), plain)
    assert tiny_dit.nag_state(reset=True) == (False, 3 * 2)               # strength 0.75: 3 of the 4 steps
    guided = run_generate(tiny_dit, golden, 5.0, **kw, **nag_kw(golden))
    assert not torch.equal(guided, plain) and torch.equal(guided.cpu()[0], src[0])   # the kept frame is the source
    # two windows of 3 frames over 5: one negative prompt for both
    shape5 = (5,) + SHAPE[1:]
    noise = torch.randn(*shape5, generator=torch.Generator().manual_seed(12))
    wkw = dict(shape=shape5, noise=noise, context_frames=3, context_overlap=1)
    plain = run_generate(tiny_dit, golden, 5.0, **wkw)
    tiny_dit.nag_state(reset=True)
    assert torch.equal(run_generate(tiny_dit, golden, 5.0, **wkw, **nag_kw(golden, positive=True)), plain)
    assert tiny_dit.nag_state(reset=True) == (False, 4 * 2 * 2)
    guided = run_generate(tiny_dit, golden, 5.0, **wkw, **nag_kw(golden))
    assert torch.isfinite(guided).all() and not torch.equal(guided, plain)


def test_magcache_skips_the_guidance_with_the_blocks(cfg, tiny_sd, golden):
    from kandinsky.generation_utils import generate
    from kandinsky.magcache_utils import disable_magcache, magcache_state, set_magcache_params
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "nocfg_9"][0]
    dit = make_dit(cfg, tiny_sd)
    dit.engine("cuda:0")
    te, ne = prompts(golden)
    try:
        set_magcache_params(dit, c["ratios"], c["num_steps"], c["no_cfg"])
        out = generate(dit, "cuda:0", SHAPE, c["num_steps"], te, ne, POS, torch.arange(7), torch.arange(4), c["guidance_weight"],
                       c["scheduler_scale"], FLASH, noise=golden["gen.noise"], **nag_kw(golden))
        _, ran, skipped = magcache_state(dit)
    finally:
        disable_magcache(dit)
    assert torch.isfinite(out).all() and skipped > 0 and ran + skipped == c["num_steps"]
    assert dit.nag_state() == (False, 2 * ran)                            # a skipped step runs no visual block and so no combine
    dit._destroy_engine(force=True)


# ------------------------------------------------------------------------------------------ ranks


@pytest.mark.timeout(600)
@pytest.mark.parametrize("P,w,mode", [(2, 1.0, 0), (2, 5.0, 1), (4, 1.0, 2)])     # sp_mode: 0 gather, 1 Ulysses, 2 two-level (2 heads over 4 ranks)
def test_loopback_ranks(tiny_sd, cfg, P, w, mode):
    from test_gpu_loopback import run_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne = rank_case()
    pos = [torch.arange(8)] * 3
    counts = {}

    def call(d, r, **kw):
        out = generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), w, 5.0, FLASH, noise=noise, nag_text_embeds=ne,
                       nag_text_rope_pos=torch.arange(4), nag_scale=5.0, **kw)
        counts[r] = (d.nag_state()[1], d.get_option("sp_mode_used"))
        return out

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    single = call(make(), -1)
    outs = run_ranks(P, make, call, options={"sp_mode": mode} if mode else None)
    for r in range(P):
        assert torch.equal(outs[r], outs[0]), f"rank {r} differs from rank 0"
        assert counts[r] == (4 * 2, mode), counts
    assert rel(outs[0], single) <= 1e-2, rel(outs[0], single)
    plain = generate(make(), "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), w, 5.0, FLASH, noise=noise)
    assert not torch.equal(single, plain)                                 # the guidance is there to be lost


@pytest.mark.timeout(900)
@pytest.mark.parametrize("Psp", [1, 2])
def test_cfg_pair_in_the_engine(tiny_sd, cfg, Psp):
    """what tests/test_gpu_loopback.py asserts for the plain pair: every handle of both groups ends with the same latent bit for bit; Psp = 1
    equals the single-handle run bit for bit; Psp > 1 within the suite's tolerance on a final latent.  Both handles of a pair carry the
    guidance, only the conditional one runs it."""
    from test_gpu_loopback import run_cfg_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne = rank_case()
    pos = [torch.arange(8)] * 3
    counts = {}

    def call(d, i):
        out = generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, nag_text_embeds=ne,
                       nag_text_rope_pos=torch.arange(4), nag_scale=5.0)
        counts[i] = d.nag_state()[1]
        return out

    make = lambda: make_dit(cfg, tiny_sd)    # noqa: E731
    fused = call(make(), -1)
    outs = run_cfg_ranks(Psp, make, call)
    for i in range(1, 2 * Psp):
        assert torch.equal(outs[i], outs[0]), f"handle {i} differs from handle 0"
    assert [counts[i] for i in range(2 * Psp)] == [4 * 2] * Psp + [0] * Psp   # branch 0 = conditional
    if Psp == 1:
        assert torch.equal(outs[0], fused)
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)
    assert rel(fused, noise.cuda()) > 0.05
