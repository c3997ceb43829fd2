"""Enhance-A-Video on the MI355X: the score kernel against the float64 rule (tests/enhance_reference.py) on every pad edge, layout and key
scaling, the in-place scale against torch, and the engine through every way it runs a forward — against the reference's fp32 goldens
(tools/gen_golden_enhance.py), against the plain run where the feature is off, and against itself where two paths claim one computation.

Kernel bound: relative error <= 1e-5 on the mean and on the score, the bound the project holds its fp32 transcendental chain to
(k5_noise_normal_f32).  The products of bf16 values are exact in the MFMA's fp32 accumulator; what is left is 64 fp32 additions per logit, one
v_exp_f32 per probability and up to 64 fp32 additions per row sum, each a few 2^-24 relative, averaged over T S Hh rows."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import kit  # noqa: E402
from kit import BF, GOLDEN, K5_ERR_ARG, K5_ERR_STATE, K5_ERR_UNSUPPORTED, POS, cfg, flash_conf, need_gpu, prompts, rel  # noqa: E402

BOUND = 1e-5
WEIGHT = 4.0

from enhance_reference import (K5_SOFTMAX_C, SHAPES, enhance_inputs, enhance_mean, enhance_score, lay_out, onehot_inputs)  # noqa: E402


# ------------------------------------------------------------------------------------------ the score kernel
def launch(L, T, S, Hh, weight=WEIGHT):
    """k5_enhance_scores_bf16 on the layout L of enhance_reference.lay_out; returns (score, mean from part, part, score tensor) after a sync"""
    from kandinsky import _engine as E
    dev = [b.cuda() for b in L["back"]]
    D = L["D"]
    Q, K = (dev[0][:, :D], dev[0][:, D:]) if L["fused"] else (dev[0], dev[1])
    rows = None if L["frame_rows"] is None else L["frame_rows"].to(torch.int32).contiguous().cuda()
    score, part = E.enhance_scores(Q, K, Hh, T, S, weight, L["qk_scale"], rows)
    torch.cuda.synchronize()
    assert part.numel() == S * Hh
    mean = float(part.cpu().sum() / (T * (T - 1)) / (S * Hh))
    return float(score.cpu()[0]), mean, part.cpu(), score.cpu()


def relerr(a, b):
    return abs(a - b) / abs(b)


@pytest.fixture(scope="module")
def references():
    """float64 mean per (shape, prescaled): computed once, shared"""
    out = {}
    for T, S, Hh in SHAPES:
        q, k = enhance_inputs(T, S, Hh)
        for pre in (False, True):
            L = lay_out(q, k, T, S, Hh, True, False, pre)
            out[(T, S, Hh, pre)] = enhance_mean(L["q"], L["k"], T, S, Hh, L["qk_scale"])
    return out


@pytest.mark.parametrize("permuted", [False, True], ids=["natural", "permuted"])
@pytest.mark.parametrize("prescaled", [False, True], ids=["plain_keys", "prescaled_keys"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_S%d_H%d" % s)
def test_score_against_float64(references, shape, fused, prescaled, permuted):
    T, S, Hh = shape
    q, k = enhance_inputs(T, S, Hh)
    L = lay_out(q, k, T, S, Hh, fused, permuted, prescaled)
    ref_mean = references[(T, S, Hh, prescaled)]
    ref_score = max(1.0, ref_mean * (T + WEIGHT))
    assert ref_score > 1.02                                               # the clamp hides nothing
    for variant in ("transposed", "shuffled", "flipped"):                 # the inputs tell the wrong rules from the right one
        if (variant == "shuffled" and S < 2) or (variant == "flipped" and Hh < 2):
            continue                                                      # the identity on this shape
        wrong = enhance_mean(L["q"], L["k"], T, S, Hh, L["qk_scale"], variant=variant)
        assert relerr(wrong, ref_mean) >= 100 * BOUND, (variant, relerr(wrong, ref_mean))
    score, mean, _, _ = launch(L, T, S, Hh)
    print(f"T {T} S {S} Hh {Hh}: mean {mean:.9g} ref {ref_mean:.9g} rel {relerr(mean, ref_mean):.2e}; score {score:.9g} rel {relerr(score, ref_score):.2e}")
    assert relerr(mean, ref_mean) <= BOUND
    assert relerr(score, ref_score) <= BOUND


@pytest.mark.parametrize("shape", [(3, 24, 2), (33, 3, 2), (61, 3, 2)], ids=lambda s: "T%d_S%d_H%d" % s)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_score_reads_nothing_it_was_not_given(shape, fused):
    """every buffer row the table does not name and every column past 64 Hh up to ld hold NaN: finite, and the bits of the clean run"""
    T, S, Hh = shape
    q, k = enhance_inputs(T, S, Hh)
    clean = launch(lay_out(q, k, T, S, Hh, fused, True, False), T, S, Hh)
    dirty = launch(lay_out(q, k, T, S, Hh, fused, True, False, fill=float("nan")), T, S, Hh)
    assert torch.isfinite(dirty[2]).all() and torch.isfinite(dirty[3]).all()
    assert torch.equal(clean[2].view(torch.int64), dirty[2].view(torch.int64))
    assert torch.equal(clean[3].view(torch.int32), dirty[3].view(torch.int32))


@pytest.mark.parametrize("shape", [(3, 24, 2), (61, 3, 2)], ids=lambda s: "T%d_S%d_H%d" % s)
def test_score_with_large_logits(shape):
    """q gain 40: logits of hundreds in log2 units; finite and within the bound only when the row maximum is subtracted"""
    T, S, Hh = shape
    q, k = enhance_inputs(T, S, Hh, gain=40.0)
    L = lay_out(q, k, T, S, Hh, True, False, False)
    z = (q.double() @ k.double().T).abs().max().item() * K5_SOFTMAX_C
    assert z > 200.0
    ref = enhance_mean(L["q"], L["k"], T, S, Hh, L["qk_scale"])
    score, mean, part, _ = launch(L, T, S, Hh)
    assert torch.isfinite(part).all()
    print(f"T {T}: largest logit {z:.0f}, mean {mean:.9g} ref {ref:.9g} rel {relerr(mean, ref):.2e}")
    assert relerr(mean, ref) <= BOUND and relerr(score, max(1.0, ref * (T + WEIGHT))) <= BOUND


@pytest.mark.parametrize("shape", [(2, 1, 1), (31, 5, 3), (64, 2, 1)], ids=lambda s: "T%d_S%d_H%d" % s)
def test_score_clamps_at_exactly_one(shape):
    T, S, Hh = shape
    q, k = onehot_inputs(T, S, Hh)
    assert enhance_score(q, k, T, S, Hh, K5_SOFTMAX_C, WEIGHT) == 1.0
    _, _, _, score = launch(lay_out(q, k, T, S, Hh, True, False, False), T, S, Hh)
    assert score.view(torch.int32).item() == 0x3F800000


def test_score_identity_uniform_attention():
    """q = 0: uniform attention, score = 1 + weight / T"""
    T, S, Hh = 5, 3, 2
    _, k = enhance_inputs(T, S, Hh)
    score, _, _, _ = launch(lay_out(torch.zeros_like(k), k, T, S, Hh, True, False, False), T, S, Hh)
    assert relerr(score, 1.0 + WEIGHT / T) <= BOUND


def test_score_is_deterministic():
    T, S, Hh = 33, 3, 2
    q, k = enhance_inputs(T, S, Hh)
    L = lay_out(q, k, T, S, Hh, True, True, True)
    a, b = launch(L, T, S, Hh), launch(L, T, S, Hh)
    assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64)) and torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))


def test_score_refusals_launch_nothing():
    from kandinsky import _engine as E
    L = E.lib()
    T, S, Hh = 3, 4, 2
    buf = torch.randn(T * S, 256, device="cuda").to(BF)
    part = torch.full((S * Hh,), 9.0, dtype=torch.float64, device="cuda")
    score = torch.full((1,), 9.0, dtype=torch.float32, device="cuda")
    st = E.stream_ptr()
    assert L.k5_enhance_part_count(Hh, S) == S * Hh and L.k5_enhance_part_count(0, S) == 0
    good = [buf.data_ptr(), buf.data_ptr() + 256, 256, 256, Hh, T, S, None, 1.0, 4.0, part.data_ptr(), score.data_ptr(), st]
    bad = [(0, None), (1, None), (0, buf.data_ptr() + 8), (1, buf.data_ptr() + 8), (2, 120), (3, 120), (2, 252), (3, 260), (4, 0), (6, 0), (5, 1), (5, 0),
           (9, -1.0), (9, float("inf")), (9, float("nan")), (8, 0.0), (8, -1.0), (10, None), (11, None)]
    for i, v in bad:
        a = list(good)
        a[i] = v
        assert L.k5_enhance_scores_bf16(*a) == 1, (i, v)
        assert "k5_enhance_scores_bf16" in E.last_error()
    a = list(good)
    a[5] = 65
    assert L.k5_enhance_scores_bf16(*a) == 6 and "64" in E.last_error()
    torch.cuda.synchronize()
    assert (part == 9.0).all() and (score == 9.0).all()
    assert L.k5_enhance_scores_bf16(*good) == 0
    torch.cuda.synchronize()
    assert not (part == 9.0).any() and score.item() >= 1.0


# ------------------------------------------------------------------------------------------ the scale kernel
@pytest.mark.parametrize("s", [1.3254, 2.3195])
@pytest.mark.parametrize("D", [64, 128, 1792])
@pytest.mark.parametrize("rows", [1, 63, 65, 257])
def test_scale_is_torch_bit_for_bit(rows, D, s):
    from kandinsky import _engine as E
    g = torch.Generator().manual_seed(rows * 10000 + D)
    x = (3.0 * torch.randn(rows, D + 8, generator=g)).to(BF)
    sd = torch.tensor([s], dtype=torch.float32, device="cuda")
    want = (x[:, :D].float() * sd.cpu()[0]).to(BF)
    buf = x.cuda()
    E.scale_by_dev_(buf, sd, D=D)                                          # ld = D + 8: the pad columns stay
    dense = x[:, :D].contiguous().cuda()
    E.scale_by_dev_(dense, sd)                                             # ld = D: the flat path
    torch.cuda.synchronize()
    assert torch.equal(buf[:, :D].cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(dense.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(buf[:, D:].cpu().view(torch.int16), x[:, D:].view(torch.int16))


def test_scale_by_one_touches_nothing():
    from kandinsky import _engine as E
    bits = torch.randint(-32768, 32767, (65, 136), dtype=torch.int16)      # every pattern: NaN payloads, infinities, -0, denormals
    bits[0, :4] = torch.tensor([-32768, 0x7FC1, -63, 0x7F80], dtype=torch.int16)   # -0, two NaNs with payloads, +inf
    buf = bits.cuda().view(BF)
    E.scale_by_dev_(buf, torch.ones(1, dtype=torch.float32, device="cuda"), D=128)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int16).cpu(), bits)


def test_scale_refusals_launch_nothing():
    from kandinsky import _engine as E
    L = E.lib()
    x = torch.full((8, 256), 3.0, dtype=BF, device="cuda")
    s = torch.full((1,), 2.0, dtype=torch.float32, device="cuda")
    good = [x.data_ptr(), 8, 256, 256, s.data_ptr(), E.stream_ptr()]
    for i, v in ((0, None), (0, x.data_ptr() + 8), (1, 0), (2, 0), (2, 252), (3, 248), (3, 260), (4, None)):
        a = list(good)
        a[i] = v
        assert L.k5_scale_by_dev_bf16(*a) == 1, (i, v)
        assert "k5_scale_by_dev_bf16" in E.last_error()
    torch.cuda.synchronize()
    assert (x == 3.0).all()
    assert L.k5_scale_by_dev_bf16(*good) == 0
    torch.cuda.synchronize()
    assert (x == 6.0).all()


# ------------------------------------------------------------------------------------------ the engine
FLASH = flash_conf()
SHAPE = (3, 8, 12, 16)                     # 72 tokens: T = 3, S = 24; not a multiple of 64, so the keys in memory are plain
STEPS = 4
INTERVAL = (0.7, 0.95)                     # of the sigmas 1, .938, .833, .625 (4 steps, scale 5) steps 1 and 2 lie inside


@pytest.fixture(scope="module")
def enh_golden():
    from safetensors.torch import load_file
    return (dict(load_file(os.path.join(GOLDEN, "dit_tiny_enhance.safetensors"))),
            json.load(open(os.path.join(GOLDEN, "dit_tiny_enhance_meta.json"))))


make_dit = functools.partial(kit.make_dit, engine=True)


@pytest.fixture(scope="module")
def tiny_dit(cfg, tiny_sd):
    need_gpu()
    return make_dit(cfg, tiny_sd)


run_generate = functools.partial(kit.run_generate, steps=STEPS, shape=SHAPE, pos=POS)


def forward(model, golden, **kw):
    te, _ = prompts(golden)
    return model(golden["fwd.x"].cuda(), te["text_embeds"], te["pooled_embed"], golden["fwd.time"], POS, torch.arange(7), scale_factor=(1.0, 2.0, 2.0),
                 **kw)


def inputs_at(shape, seed=21):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(*shape, generator=g)
    x = torch.cat([lat, torch.zeros_like(lat), torch.zeros(*shape[:-1], 1)], -1)
    text, pooled, t = torch.randn(7, 96, generator=g), torch.randn(1, 48, generator=g), torch.tensor([600.0])
    pos = [torch.arange(shape[0]), torch.arange(shape[1] // 2), torch.arange(shape[2] // 2)]
    return (x.cuda(), text.cuda(), pooled.cuda(), t, pos, torch.arange(7))


Wrapped = functools.partial(kit.Wrapped, blocks=True, hand_on=("set_enhance", "clear_enhance", "_enhance"))   # hands the setting on


@pytest.fixture(scope="module")
def plain_runs(tiny_dit, golden):
    return {w: run_generate(tiny_dit, golden, w) for w in (1.0, 5.0)}


@pytest.fixture(scope="module")
def enhanced_runs(tiny_dit, golden, enh_golden):
    """the in-engine runs of both sets (every step), each computed once: {(set, w): (latent, launches)}"""
    out = {}
    for name, m in enh_golden[1]["sets"].items():
        for w in (1.0, 5.0):
            tiny_dit.enhance_state(reset=True)
            lat = run_generate(tiny_dit, golden, w, enhance_weight=m["weight"])
            out[(name, w)] = (lat, tiny_dit.enhance_state(reset=True)[1])
    return out


@pytest.mark.parametrize("case", ["fwd", "gen.1.0", "gen.5.0"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_parity_with_the_fp32_golden(tiny_dit, golden, enh_golden, enhanced_runs, name, case):
    """A: rel <= min(3e-2, delta / 4), delta being the golden's own distance from the plain run, so a build that ignores the feature fails.
    B (weight 0: the single forward clamps, its golden IS the plain golden): the project's 3e-2 against the set's golden."""
    g, meta = enh_golden
    m = meta["sets"][name]
    if name == "A":
        assert m["delta"][case] >= meta["delta_min"] == 0.04 and min(m["scores"]) > meta["score_min"] == 1.5
    else:
        assert m["delta"]["fwd"] == 0.0 and torch.equal(g["enhance.B.fwd.out"], golden["fwd.out"])
    if case == "fwd":
        tiny_dit.set_enhance(m["weight"])
        try:
            tiny_dit.reset_softmax_memory()
            out = forward(tiny_dit, golden).clone()
        finally:
            tiny_dit.clear_enhance()
        ref = g[f"enhance.{name}.fwd.out"]
    else:
        out = enhanced_runs[(name, float(case[4:]))][0]
        ref = g[f"enhance.{name}.{case}.final"]
    bound = min(3e-2, m["delta"][case] / 4) if name == "A" else 3e-2
    r = rel(out, ref)
    print(f"enhance {name} {case}: engine vs fp32 golden {r:.3e} (bound {bound:.3e}, delta {m['delta'][case]:.3e})")
    assert torch.isfinite(out.float()).all() and r <= bound, r


def test_block_scores_against_the_fixture(tiny_dit, golden, enh_golden):
    """the forward's per-block scores against the reference's: 4 x the largest recorded bf16_spread (the engine's stream is bf16 up to there)"""
    g, meta = enh_golden
    m = meta["sets"]["A"]
    bound = 4 * max(m["bf16_spread"])
    tiny_dit.set_enhance(m["weight"])
    try:
        tiny_dit.reset_softmax_memory()
        tiny_dit.enhance_state(reset=True)
        forward(tiny_dit, golden)
        on, launches, scores = tiny_dit.enhance_state(reset=True)
    finally:
        tiny_dit.clear_enhance()
    assert on and launches == len(scores) == tiny_dit.num_visual_blocks == len(m["scores"])
    devs = [relerr(s, r) for s, r in zip(scores, m["scores"])]
    print(f"enhance scores: engine {scores} reference {m['scores']} deviation {['%.2e' % d for d in devs]} bound {bound:.2e}")
    assert all(s > 1.5 for s in scores) and max(devs) <= bound, devs


def test_off_is_the_plain_run(tiny_dit, golden, plain_runs):
    from kandinsky.generation_utils import sigma_schedule
    te, ne = prompts(golden)
    tiny_dit.enhance_state(reset=True)
    for w in (1.0, 5.0):
        assert torch.equal(run_generate(tiny_dit, golden, w, enhance_weight=4.0, enhance_interval=(2.0, 3.0)), plain_runs[w])   # no step inside
        assert torch.equal(run_generate(tiny_dit, golden, w, enhance_weight=None), plain_runs[w])
    for setup in (lambda: tiny_dit.set_enhance(4.0, steps=[0] * STEPS), lambda: tiny_dit.set_enhance(4.0).clear_enhance()):
        setup()
        try:
            lat = golden["gen.noise"].cuda().contiguous().clone()
            tiny_dit.sample(lat, sigma_schedule(STEPS, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0))
            assert torch.equal(lat, plain_runs[5.0])
        finally:
            tiny_dit.clear_enhance()
    assert tiny_dit.enhance_state(reset=True)[:2] == (False, 0)


@pytest.mark.parametrize("w", [1.0, 5.0])
@pytest.mark.parametrize("interval", [None, INTERVAL], ids=["every_step", "interval"])
def test_one_sample_call_equals_its_forwards_step_by_step(tiny_dit, golden, plain_runs, enhanced_runs, w, interval):
    """the in-engine loop against generate's per-step path on a wrapped model (its forwards issued one by one, the setting put and cleared per
    step), and the launch counts: forwards per step x visual blocks on every step that has it on"""
    fwd, nb = (2 if w == 5.0 else 1), tiny_dit.num_visual_blocks
    if interval is None:
        a, launches = enhanced_runs[("A", w)]
        on_steps = STEPS
    else:
        tiny_dit.enhance_state(reset=True)
        a = run_generate(tiny_dit, golden, w, enhance_weight=4.0, enhance_interval=interval)
        launches = tiny_dit.enhance_state(reset=True)[1]
        on_steps = 2
    assert launches == on_steps * fwd * nb
    b = run_generate(Wrapped(tiny_dit), golden, w, enhance_weight=4.0, enhance_interval=interval)
    assert tiny_dit._enhance is None and tiny_dit.enhance_state(reset=True)[:2] == (False, on_steps * fwd * nb)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert rel(a, plain_runs[w]) > 1e-2                                   # it did something
    if interval is not None:
        assert not torch.equal(a, enhanced_runs[("A", w)][0])


def test_the_captured_step_equals_the_eager_run(cfg, tiny_sd, golden, tiny_dit, enhanced_runs):
    gdit = make_dit(cfg, tiny_sd)
    gdit.set_graph(True)
    for w in (1.0, 5.0):
        gdit.enhance_state(reset=True)
        assert torch.equal(run_generate(gdit, golden, w, enhance_weight=4.0), enhanced_runs[("A", w)][0]), w     # one kind of step: the capture is used
        assert gdit.enhance_state(reset=True)[1] == enhanced_runs[("A", w)][1]                                # replays are counted as eager launches are
        mixed = run_generate(gdit, golden, w, enhance_weight=4.0, enhance_interval=INTERVAL)                     # mixed: eager on this handle too
        assert torch.equal(mixed, run_generate(tiny_dit, golden, w, enhance_weight=4.0, enhance_interval=INTERVAL)), w
    gdit._destroy_engine(force=True)


def test_each_sample_of_a_batch_equals_its_own_call(tiny_dit, golden):
    from kandinsky.generation_utils import generate
    g = torch.Generator().manual_seed(41)
    te, ne = prompts(golden)
    te2 = {"text_embeds": torch.randn(5, 96, generator=g).cuda(), "pooled_embed": torch.randn(1, 48, generator=g).cuda()}
    noise = torch.cat([golden["gen.noise"], torch.randn(*SHAPE, generator=g)])
    tes, tps = [te, te2], [torch.arange(7), torch.arange(5)]
    kw = dict(enhance_weight=4.0, enhance_interval=INTERVAL)
    tiny_dit.enhance_state(reset=True)
    out = generate(tiny_dit, "cuda:0", (2 * SHAPE[0],) + SHAPE[1:], STEPS, tes, ne, POS, tps, torch.arange(4), 5.0, 5.0, FLASH, noise=noise, batch=2, **kw)
    assert tiny_dit.enhance_state(reset=True)[1] == 2 * 2 * 2 * tiny_dit.num_visual_blocks
    for b in range(2):
        one = generate(tiny_dit, "cuda:0", SHAPE, STEPS, tes[b], ne, POS, tps[b], torch.arange(4), 5.0, 5.0, FLASH, noise=noise[b * 3:(b + 1) * 3], **kw)
        assert torch.equal(out[b * 3:(b + 1) * 3], one), b


def test_query_norm_fusion_moves_no_bits_and_is_not_used(cfg, tiny_sd):
    """1536 tokens, dense: "attn_fuse_qnorm" 1 and 0 give the same bits with enhance on (the queries are normalised by the standalone pass
    either way), and a sample call reports attn_fuse_qnorm_used 0"""
    from kandinsky.generation_utils import sigma_schedule
    shape = (6, 32, 32, 16)
    args = inputs_at(shape)
    d = make_dit(cfg, tiny_sd)
    outs, scores = [], []
    d.set_enhance(4.0)
    for fuse in (0, 1):
        d.set_option("attn_fuse_qnorm", fuse)
        d.reset_softmax_memory()
        outs.append(d(*args, scale_factor=(1.0, 2.0, 2.0)).clone())
        scores.append(d.enhance_state()[2])
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1]) and scores[0] == scores[1]
    assert all(s >= 1.0 for s in scores[0]) and len(scores[0]) == d.num_visual_blocks
    d.set_option("attn_fuse_qnorm", 0)
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(*shape, generator=g).cuda()
    te = {"text_embeds": args[1], "pooled_embed": args[2]}

    def sample():
        lat = noise.clone()
        d.sample(lat, sigma_schedule(3, 5.0).tolist(), te, te, args[4], torch.arange(7), torch.arange(7), 1.0, scale_factor=(1.0, 2.0, 2.0))
        return lat, d.get_option("attn_fuse_qnorm_used")
    on, used_on = sample()
    d.clear_enhance()
    off, used_off = sample()
    assert used_on == 0 and used_off in (0, 1) and torch.isfinite(on).all() and not torch.equal(on, off)
    d._destroy_engine(force=True)


@pytest.mark.parametrize("shape", [(6, 16, 16, 16), (6, 16, 32, 16)], ids=["6x16x16", "6x16x32"])
def test_nabla_fractal_order_gives_the_dense_score(cfg, tiny_sd, golden_meta, shape):
    """the first block's q and k of a NABLA forward are the dense forward's in another row order (6x16x32: two 8 x 8 tiles side by side, so
    the fractal order really differs from the row-major one; at 6x16x16 the two coincide): the same score to 1e-5 — a wrong frame_rows pairs
    frames of different positions and moves it by far more.  Both forms of the NABLA norm pass; every score finite and >= 1"""
    attn = golden_meta["nabla_attention"]
    sparse = {"P": attn["P"], "wT": attn["wT"], "wH": attn["wH"], "wW": attn["wW"], "to_fractal": True}
    args = inputs_at(shape)
    d = make_dit(cfg, tiny_sd)
    d.set_enhance(4.0)
    dense = d(*args, scale_factor=(1.0, 2.0, 2.0)).clone()
    s_dense = d.enhance_state()[2]
    runs = {}
    for fuse_means in (1, 2, 0):                                          # by size (here: its own means pass) | the fused means | its own means pass
        d.set_option("nabla_fuse_means", fuse_means)
        d.reset_softmax_memory()
        out = d(*args, scale_factor=(1.0, 2.0, 2.0), sparse_params=sparse).clone()
        runs[fuse_means] = (out, d.enhance_state()[2])
    torch.cuda.synchronize()
    print(f"enhance scores {shape}: dense {s_dense} nabla { {k: v[1] for k, v in runs.items()} }")
    assert s_dense[0] > 1.01                                              # not clamped: the comparison sees the mean
    assert torch.isfinite(dense.float()).all() and len(s_dense) == d.num_visual_blocks
    for fuse_means, (out, s) in runs.items():
        assert len(s) == d.num_visual_blocks and all(1.0 <= v < float("inf") for v in s), (fuse_means, s)
        assert torch.isfinite(out.float()).all()
        assert relerr(s[0], s_dense[0]) <= 1e-5, (fuse_means, s[0], s_dense[0])
    d._destroy_engine(force=True)


def test_magcache_and_skip_guidance_launch_counts(cfg, tiny_sd, golden):
    from kandinsky.generation_utils import generate
    from kandinsky.magcache_utils import disable_magcache, magcache_state, set_magcache_params
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "nocfg_9"][0]
    d = make_dit(cfg, tiny_sd)
    te, ne = prompts(golden)
    try:
        set_magcache_params(d, c["ratios"], c["num_steps"], c["no_cfg"])
        out = generate(d, "cuda:0", SHAPE, c["num_steps"], te, ne, POS, torch.arange(7), torch.arange(4), c["guidance_weight"],
                       c["scheduler_scale"], FLASH, noise=golden["gen.noise"], enhance_weight=4.0)
        _, ran, skipped = magcache_state(d)
    finally:
        disable_magcache(d)
    assert torch.isfinite(out).all() and skipped > 0 and ran + skipped == c["num_steps"]
    assert d.enhance_state(reset=True)[:2] == (False, d.num_visual_blocks * ran)      # a skipped forward launches nothing
    # skip-layer guidance: block 0 skipped, so the skip branch re-runs block 1 and computes its own score there
    out = run_generate(d, golden, 1.0, enhance_weight=4.0, slg_blocks=[0], slg_scale=3.0)
    assert torch.isfinite(out).all()
    assert d.enhance_state(reset=True)[1] == STEPS * (d.num_visual_blocks + 1) and d.skip_state(reset=True)[3] == STEPS
    d._destroy_engine(force=True)


def test_editing_and_context_windows(tiny_dit, golden):
    src = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(77))
    mask = torch.zeros(*SHAPE[:-1], 1)
    mask[0] = 1.0
    kw = dict(init_latent=src, strength=0.75, keep_mask=mask)             # 3 of the 4 steps run, of which steps 1 and 2 lie in the interval
    nb = tiny_dit.num_visual_blocks
    plain = run_generate(tiny_dit, golden, 5.0, **kw)
    tiny_dit.enhance_state(reset=True)
    out = run_generate(tiny_dit, golden, 5.0, **kw, enhance_weight=4.0, enhance_interval=INTERVAL)
    assert tiny_dit.enhance_state(reset=True)[1] == 2 * 2 * nb
    assert torch.isfinite(out).all() and not torch.equal(out, plain) and torch.equal(out.cpu()[0], src[0])
    assert torch.equal(out, run_generate(Wrapped(tiny_dit), golden, 5.0, **kw, enhance_weight=4.0, enhance_interval=INTERVAL))
    # two windows of 3 frames over 5: T is the window's
    shape5 = (5,) + SHAPE[1:]
    noise = torch.randn(*shape5, generator=torch.Generator().manual_seed(12))
    wkw = dict(shape=shape5, noise=noise, context_frames=3, context_overlap=1)
    plain = run_generate(tiny_dit, golden, 5.0, **wkw)
    tiny_dit.enhance_state(reset=True)
    out = run_generate(tiny_dit, golden, 5.0, **wkw, enhance_weight=4.0)
    assert tiny_dit.enhance_state(reset=True)[1] == STEPS * 2 * 2 * nb    # steps x windows x forwards x blocks
    assert torch.isfinite(out).all() and not torch.equal(out, plain)
    assert torch.equal(out, run_generate(Wrapped(tiny_dit), golden, 5.0, **wkw, enhance_weight=4.0))


def test_frame_limits(cfg, tiny_sd, golden):
    d = make_dit(cfg, tiny_sd)
    d.set_enhance(4.0)
    # T = 33: the two-tile path through the engine
    out = d(*inputs_at((33, 4, 4, 16)), scale_factor=(1.0, 2.0, 2.0))
    on, launches, scores = d.enhance_state(reset=True)
    assert torch.isfinite(out.float()).all() and launches == len(scores) == d.num_visual_blocks and all(s >= 1.0 and s < 40.0 for s in scores)
    # T = 1 is accepted and inert
    args = inputs_at((1, 8, 12, 16))
    one = d(*args, scale_factor=(1.0, 2.0, 2.0)).clone()
    assert d.enhance_state(reset=True)[1] == 0
    d.clear_enhance()
    d.reset_softmax_memory()
    assert torch.equal(one, d(*args, scale_factor=(1.0, 2.0, 2.0)))
    # T = 65 raises before anything runs
    d.set_enhance(4.0)
    with pytest.raises(RuntimeError, match=f"status {K5_ERR_UNSUPPORTED}") as e:
        d(*inputs_at((65, 4, 4, 16)), scale_factor=(1.0, 2.0, 2.0))
    assert "65 frames" in str(e.value) and d.enhance_state()[1] == 0
    with pytest.raises(ValueError, match="65 latent frames"):
        run_generate(d, golden, 1.0, shape=(65, 4, 4, 16), noise=torch.zeros(65, 4, 4, 16), pos=[torch.arange(65), torch.arange(2), torch.arange(2)],
                     enhance_weight=4.0)
    d.clear_enhance()
    assert torch.isfinite(d(*inputs_at((65, 4, 4, 16)), scale_factor=(1.0, 2.0, 2.0)).float()).all()   # off: the long clip runs
    d._destroy_engine(force=True)


def test_sample_refusals_touch_nothing(tiny_dit, golden):
    from kandinsky.generation_utils import sigma_schedule
    te, ne = prompts(golden)
    lat = golden["gen.noise"].cuda().contiguous()
    before = lat.clone()
    tiny_dit.enhance_state(reset=True)
    tiny_dit.set_enhance(4.0, steps=[1, 0, 1])
    try:
        with pytest.raises(RuntimeError, match=f"status {K5_ERR_ARG}") as e:
            tiny_dit.sample(lat, sigma_schedule(2, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0))
        assert "3 steps" in str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(lat, before) and tiny_dit.enhance_state()[1] == 0
    finally:
        tiny_dit.clear_enhance()
    with pytest.raises(ValueError, match="weight"):
        tiny_dit.set_enhance(-1.0)
    assert tiny_dit._enhance is None


@pytest.mark.timeout(600)
def test_rank_groups_are_refused_and_work_afterwards(cfg, tiny_sd):
    from edit_rank_worker import case
    from test_gpu_loopback import run_ranks
    from kandinsky.generation_utils import generate, sigma_schedule
    shape, noise, te, ne, _, _ = case()
    te, ne = {k: v.cuda() for k, v in te.items()}, {k: v.cuda() for k, v in ne.items()}
    pos = [torch.arange(8)] * 3

    def call(d, r):
        lat = noise.cuda().contiguous().clone()
        d.set_enhance(4.0)
        with pytest.raises(RuntimeError, match=f"status {K5_ERR_STATE}") as e:
            d.sample(lat, sigma_schedule(4, 5.0).tolist(), te, ne, pos, torch.arange(9), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0))
        assert "sequence-parallel" in str(e.value) and torch.equal(lat.cpu(), noise)
        with pytest.raises(ValueError, match="sequence-parallel"):
            generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, enhance_weight=4.0)
        d.clear_enhance()
        assert d.enhance_state()[1] == 0
        return generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise)

    outs = run_ranks(2, lambda: make_dit(cfg, tiny_sd), call)
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()


@pytest.mark.timeout(600)
def test_cfg_pair_equals_the_single_handle_run(cfg, tiny_sd):
    from edit_rank_worker import case
    from test_gpu_loopback import run_cfg_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne, _, _ = case()
    te, ne = {k: v.cuda() for k, v in te.items()}, {k: v.cuda() for k, v in ne.items()}
    pos = [torch.arange(8)] * 3

    def call(d, i):
        out = generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, enhance_weight=4.0)
        return out, d.enhance_state()[1]

    single = make_dit(cfg, tiny_sd)
    fused, n_single = call(single, 0)
    single._destroy_engine(force=True)
    outs = run_cfg_ranks(1, lambda: make_dit(cfg, tiny_sd), call)
    nb = cfg["num_visual_blocks"]
    assert n_single == 4 * 2 * nb and outs[0][1] == outs[1][1] == 4 * nb      # each handle of the pair runs its own forward's scores
    assert torch.equal(outs[1][0], outs[0][0]), "the two handles of the pair differ"
    assert torch.equal(outs[0][0], fused)
