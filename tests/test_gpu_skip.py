"""Skip-layer guidance on the MI355X: the three-velocity update bit for bit against the torch bf16 expression, the forking forward
(k5_dit_forward_skip) against k5_dit_forward and the bf16 oracle, k5_sample* with a skip set through every mode of the fused sampler (the
same bits as the plain run where the set is off, as the per-step loop everywhere), parity with the bf16 oracle and the reference's golden,
rank groups, and every refusal.

The model is the tiny config with four visual blocks on synthetic weights (tests/skip_reference.py): a prefix, a skipped block and a suffix
at once.  Tolerances are the project's (tests/test_gpu_dit.py, tests/test_gpu_guidance.py): a velocity or a final latent within relative L2
1e-2 of the bf16-island oracle and 3e-2 of the reference's fp32 golden (tools/gen_golden_skip.py), the NABLA forward included.  Everything
that claims "the same computation" is asserted bit for bit."""
import ctypes as C
import functools
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402

import skip_reference as S  # noqa: E402
import kit  # noqa: E402
from kit import BF, GOLDEN, K5_ERR_ARG, K5_ERR_STATE, POS, edit_mask, f32, flash_conf, make_dit, prompts, rel, source_latent  # noqa: E402

FLASH = flash_conf()
SHAPE = (3, 8, 12, 16)
STEPS = 6
INTERVAL = (0.6, 0.97)      # of the sigmas 1, .962, .909, .833, .714, .5 (6 steps, scale 5) steps 1..4 lie inside: a mixed run
CASES = {"block_mid": (5.0, dict(slg_blocks=[1], slg_scale=3.0)),
         "block_first_nocfg": (1.0, dict(slg_blocks=[0], slg_scale=3.0)),
         "attention_interval": (5.0, dict(slg_blocks=[1, 2], slg_scale=3.0, slg_mode="attention", slg_interval=INTERVAL)),
         "with_zero_star_rescale": (5.0, dict(slg_blocks=[2], slg_scale=3.0, cfg_zero_star=True, cfg_rescale=0.7))}


@pytest.fixture(scope="module")
def cfg(golden_meta):
    return S.tiny4_config(golden_meta["tiny_config"])


@pytest.fixture(scope="module")
def sd4(cfg):
    return S.tiny4_weights(cfg)


@pytest.fixture(scope="module")
def dit(cfg, sd4):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    d = make_dit(cfg, sd4)
    d.engine("cuda:0")
    return d


def run_generate(model, golden, w=5.0, steps=STEPS, **kw):
    return kit.run_generate(model, golden, w, steps=steps, shape=SHAPE, pos=POS, **kw)


Wrapped = functools.partial(kit.Wrapped, blocks=True,          # this one can fork
                            hand_on=("forward_skip", "set_skip_guidance", "clear_skip_guidance", "_skip"))


# ------------------------------------------------------------------------------------------ kernel: the three-velocity update
BIG = (5, 163, 161, 16)     # 2 099 440 elements, just past 8192 blocks x 256 threads: the grid-stride loop takes a second sweep


def renoise_ref(x0, eps, sigma):
    a = f32(np.float32(1.0) - np.float32(sigma))
    return a * x0 + f32(sigma) * eps


def update_inputs(dims, seed):
    n, cells = int(np.prod(dims)), int(np.prod(dims[:-1]))
    g = torch.Generator().manual_seed(seed)
    img, x0, eps = torch.randn(n, generator=g).cuda(), (torch.randn(n, generator=g) * 3).cuda(), torch.randn(n, generator=g).cuda()
    c, u, s = (torch.randn(n, generator=g).cuda().to(BF) for _ in range(3))
    mask = torch.tensor([0.0, 1.0, 0.25])[torch.randint(0, 3, (cells,), generator=g)].cuda()
    assert all((mask == v).any() for v in (0.0, 1.0, 0.25))
    return img, x0, eps, c, u, s, mask


def launch_update(img, c, u, s, w, abd, g, dt, x0, eps, mask, sigma, cells, Cc, vout_of):
    """the raw entry on guarded buffers; returns (latent, v_cond buffer, v_out buffer)"""
    from kandinsky import _engine as E
    n = img.numel()
    buf = torch.full((n + 64,), 7.0, device="cuda")                 # a guard region after the latent
    buf[:n] = img
    cc = torch.full((n + 64,), 3.0, dtype=BF, device="cuda")        # ... and after the velocity that v_out may alias
    cc[:n] = c
    vo = vout_of(cc)
    st = E.lib().k5_skip_euler(buf.data_ptr(), cc.data_ptr(), None if u is None else u.data_ptr(), None if s is None else s.data_ptr(), w,
                               None if abd is None else abd.data_ptr(), g, dt, None if mask is None else x0.data_ptr(),
                               None if mask is None else eps.data_ptr(), None if mask is None else mask.data_ptr(), sigma, cells, Cc,
                               None if vo is None else vo.data_ptr(), E.stream_ptr())
    torch.cuda.synchronize()
    assert (buf[n:] == 7.0).all() and (cc[n:] == 3.0).all()
    return st, buf[:n], cc[:n], vo


@pytest.mark.parametrize("dims", [(3, 8, 12, 16), (5, 10, 14, 16)])
@pytest.mark.parametrize("sigma", [0.0, 0.37, 1.0])
@pytest.mark.parametrize("base", ["cond", "cfg", "ab"])
def test_skip_euler_bit_exact(dims, sigma, base):
    from kandinsky import _engine as E
    n, cells, Cc = int(np.prod(dims)), int(np.prod(dims[:-1])), dims[-1]
    img, x0, eps, c, u, s, mask = update_inputs(dims, n + len(base))
    w, g, dt = f32(4.3), f32(2.3), f32(-0.0625 * 1.3)              # g and w not representable in bf16: a scale rounded early would show
    al, be = f32(2.2), f32(-1.3137)
    abd = torch.tensor([al, be], dtype=torch.float32, device="cuda") if base == "ab" else None
    uu = None if base == "cond" else u
    vb = c if base == "cond" else (u + w * (c - u)) if base == "cfg" else (al * c.float() + be * u.float()).to(BF)
    v = vb + g * (c - s)                                           # the oracle: torch eager on bf16 tensors (a GPU scalar factor stays fp32)
    assert v.dtype == BF
    x = img + (dt * v.float()).to(BF).float()
    known = renoise_ref(x0, eps, sigma)
    m = mask.repeat_interleave(Cc)
    want = torch.where(m == 1, known, torch.where(m == 0, x, x + m * (known - x)))
    # the host restatement that the sampler loops of tests/skip_reference.py are built on gives the same bits
    hx, hv = S.skip_update(img.cpu(), c.cpu(), None if uu is None else u.cpu(), s.cpu(), w, g, dt, (al, be) if base == "ab" else None, x0.cpu(),
                           eps.cpu(), m.cpu(), sigma)
    assert torch.equal(hv, v.cpu()) and torch.equal(hx, want.cpu())

    def run(maskp, vout_of):
        st, out, cc, vo = launch_update(img, c, uu, s, w, abd, g, dt, x0, eps, maskp, sigma, cells, Cc, vout_of)
        assert st == 0, E.last_error()
        return out, cc, vo

    out, cc, _ = run(mask, lambda cc: None)                              # with mask, no v_out: v_cond is not written
    assert torch.equal(out, want) and torch.equal(cc, c)
    if sigma == 0.0:
        assert torch.equal(out[m == 1], x0[m == 1])
    out, cc, _ = run(mask, lambda cc: cc)                                # v_out aliasing v_cond, with or without ab
    assert torch.equal(out, want) and torch.equal(cc, v)
    sep = torch.full((n + 64,), 3.0, dtype=BF, device="cuda")
    out, cc, vo = run(None, lambda cc: sep)                              # without mask, v_out apart
    assert torch.equal(out, x) and torch.equal(cc, c) and torch.equal(vo[:n], v) and (vo[n:] == 3.0).all()
    # the helper
    helper, vv = img.clone().view(dims), c.clone().view(dims)
    E.skip_euler_(helper, vv, None if uu is None else u.view(dims), s.view(dims), w, g, dt, abd, x0.view(dims), eps.view(dims),
                  mask.view(*dims[:-1], 1), sigma, v_out=vv)
    assert torch.equal(helper.view(-1), want) and torch.equal(vv.view(-1), v)
    # x0_preview with v_uncond = NULL on that velocity is the preview of a skip step
    _, p0 = E.x0_preview(helper, vv, None, 1.0, sigma, want_x0=True)
    assert torch.equal(p0.view(-1), want - f32(sigma) * v.float())


def test_skip_euler_past_the_grid():
    """more elements than one sweep of the capped grid covers: every element is updated once, the last ones included"""
    from kandinsky import _engine as E
    dims = BIG
    n, cells, Cc = int(np.prod(dims)), int(np.prod(dims[:-1])), dims[-1]
    assert n > 8192 * 256 and n - 8192 * 256 < 8192 * 256
    img, x0, eps, c, u, s, mask = update_inputs(dims, 5)
    w, g, dt, sigma = f32(4.3), f32(2.3), f32(-0.07), 0.37
    for uu in (u, None):
        v = (c if uu is None else u + w * (c - u)) + g * (c - s)
        x = img + (dt * v.float()).to(BF).float()
        known = renoise_ref(x0, eps, sigma)
        m = mask.repeat_interleave(Cc)
        want = torch.where(m == 1, known, torch.where(m == 0, x, x + m * (known - x)))
        st, out, cc, _ = launch_update(img, c, uu, s, w, None, g, dt, x0, eps, mask, sigma, cells, Cc, lambda cc: cc)
        assert st == 0, E.last_error()
        assert torch.equal(out, want) and torch.equal(cc, v)
        assert torch.equal(out[-4096:], want[-4096:]) and torch.equal(out[8192 * 256 - 64:8192 * 256 + 64], want[8192 * 256 - 64:8192 * 256 + 64])


def test_skip_euler_refusals_launch_nothing():
    from kandinsky import _engine as E
    dims = (3, 8, 12, 16)
    n, cells, Cc = int(np.prod(dims)), int(np.prod(dims[:-1])), dims[-1]
    img, x0, eps, c, u, s, mask = update_inputs(dims, 9)
    abd = torch.tensor([2.0, -1.0], dtype=torch.float32, device="cuda")

    def refused(**kw):
        a = dict(img=img, c=c, u=u, s=s, w=5.0, abd=None, g=3.0, dt=-0.1, x0=x0, eps=eps, mask=mask, sigma=0.5, cells=cells, Cc=Cc)
        a.update(kw)
        st, out, cc, _ = launch_update(a["img"], a["c"], a["u"], a["s"], a["w"], a["abd"], a["g"], a["dt"], a["x0"], a["eps"], a["mask"], a["sigma"],
                                       a["cells"], a["Cc"], lambda cc: cc)
        assert st == K5_ERR_ARG and "k5_skip_euler" in E.last_error()
        assert torch.equal(out, img[:out.numel()]) and torch.equal(cc, c[:cc.numel()])      # the buffers are as they were

    for g in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        refused(g=g)                                                    # v_skip without g > 0; a g that is not finite or is negative
    refused(s=None)                                                     # the three-velocity entry without its third velocity
    refused(u=None, abd=abd)                                            # the existing refusals stay: ab without v_uncond ...
    refused(cells=0)
    refused(Cc=0)
    L = E.lib()
    buf = img.clone()
    assert L.k5_skip_euler(buf.data_ptr(), c.data_ptr(), None, s.data_ptr(), 1.0, None, 3.0, -0.1, None, eps.data_ptr(), mask.data_ptr(), 0.5,
                           cells, Cc, None, E.stream_ptr()) == K5_ERR_ARG                   # ... a keep_mask without source
    assert L.k5_skip_euler(None, c.data_ptr(), None, s.data_ptr(), 1.0, None, 3.0, -0.1, None, None, None, 0.5, cells, Cc, None,
                           E.stream_ptr()) == K5_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(buf, img)
    # the two-velocity entries are what they were: a refused skip call left no state, and their bits are the eager expressions
    out = img.clone()
    E.cfg_euler_(out, c, u, 5.0, -0.1)
    assert torch.equal(out, img + (f32(-0.1) * (u + 5.0 * (c - u)).float()).to(BF).float())


# ------------------------------------------------------------------------------------------ the forking forward
def forward_args(golden):
    noise = golden["gen.noise"]
    x = torch.cat([noise, torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)], -1)
    return x, golden["fwd.text"], golden["fwd.pooled"], torch.tensor([700.0])


def engine_pair(d, golden, blocks, mode, **kw):
    x, text, pooled, t = forward_args(golden)
    d.set_skip_guidance(blocks, 3.0, mode)
    try:
        d.reset_softmax_memory()
        c, s = d.forward_skip(x.cuda(), text.cuda(), pooled.cuda(), t, POS, torch.arange(7), scale_factor=(1.0, 2.0, 2.0), **kw)
        torch.cuda.synchronize()
        return c.clone(), s.clone()
    finally:
        d.clear_skip_guidance()


@pytest.fixture(scope="module")
def plain_forward(dit, golden):
    x, text, pooled, t = forward_args(golden)
    dit.reset_softmax_memory()
    return dit(x.cuda(), text.cuda(), pooled.cuda(), t, POS, torch.arange(7), scale_factor=(1.0, 2.0, 2.0)).clone()


@pytest.fixture(scope="module")
def oracle_cond(cfg, sd4, golden):
    x, text, pooled, t = forward_args(golden)
    return O.dit_forward(sd4, O.DitConfig(**cfg), x, text, pooled, t, POS, torch.arange(7), (1.0, 2.0, 2.0), None, "bf16")


@pytest.mark.parametrize("mode", ["block", "attention"])
@pytest.mark.parametrize("blocks", [[0], [1], [3], [1, 2]])
def test_forward_skip_vs_forward_and_the_oracle(dit, cfg, sd4, golden, plain_forward, oracle_cond, blocks, mode):
    c, s = engine_pair(dit, golden, blocks, mode)
    assert torch.equal(c, plain_forward)                                 # the conditional output is k5_dit_forward's, bit for bit
    x, text, pooled, t = forward_args(golden)
    ref = S.dit_forward_skip(sd4, O.DitConfig(**cfg), x, text, pooled, t, POS, torch.arange(7), (1.0, 2.0, 2.0), None, "bf16", blocks, mode)
    r = rel(s, ref)
    print(f"forward_skip blocks {blocks} mode {mode}: v_skip vs bf16 oracle {r:.3e}, cond vs oracle {rel(c, oracle_cond):.3e}, "
          f"skip vs cond {rel(s, c):.3e}")
    assert torch.isfinite(s.float()).all()
    assert r <= 1e-2, r
    assert rel(s, c) > 1e-3 and rel(ref, oracle_cond) > 1e-3              # skipping did something, in the engine and in the oracle


def inputs_at(shape, seed=21):
    """a forward's inputs at another latent shape (64-token multiples: the data-derived softmax forms and their memory are in play)"""
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(*shape, generator=g)
    x = torch.cat([lat, torch.zeros_like(lat), torch.zeros(*shape[:-1], 1)], -1)
    text, pooled, t = torch.randn(7, 96, generator=g), torch.randn(1, 48, generator=g), torch.tensor([600.0])
    pos = [torch.arange(shape[0]), torch.arange(shape[1] // 2), torch.arange(shape[2] // 2)]
    return x, text, pooled, t, pos


def test_share_prefix_on_and_off_give_the_same_bits(dit, golden, plain_forward):
    for blocks, mode in (([2], "block"), ([1, 3], "attention"), ([0], "block")):
        dit.attn_variant_counts(reset=True)
        c1, s1 = engine_pair(dit, golden, blocks, mode)
        dit.set_option("skip_share_prefix", 0)
        try:
            c0, s0 = engine_pair(dit, golden, blocks, mode)
        finally:
            dit.set_option("skip_share_prefix", 1)
        assert dit.attn_variant_counts(reset=True)[1] == 0                # no head took the online form: the form memory cannot have mattered
        assert torch.equal(c0, plain_forward) and torch.equal(c1, plain_forward)
        assert torch.equal(s0, s1), (blocks, mode)
    # ... and at 128 tokens, where every visual self-attention decides its softmax form from the data and keeps its memory (72 tokens do not)
    x, text, pooled, t, pos = inputs_at((2, 16, 16, 16))
    args = (x.cuda(), text.cuda(), pooled.cuda(), t, pos, torch.arange(7))
    dit.reset_softmax_memory()
    plain = dit(*args, scale_factor=(1.0, 2.0, 2.0)).clone()
    dit.set_skip_guidance([2], 3.0)
    try:
        outs = []
        for share in (1, 0):
            dit.set_option("skip_share_prefix", share)
            dit.reset_softmax_memory()
            dit.attn_variant_counts(reset=True)
            c, s = dit.forward_skip(*args, scale_factor=(1.0, 2.0, 2.0))
            fixed, online = dit.attn_variant_counts(reset=True)
            assert online == 0 and fixed > 0
            outs.append((c.clone(), s.clone()))
    finally:
        dit.set_option("skip_share_prefix", 1)
        dit.clear_skip_guidance()
    assert torch.equal(outs[0][0], plain) and torch.equal(outs[1][0], plain)
    assert torch.equal(outs[0][1], outs[1][1]) and rel(outs[0][1], plain) > 1e-3


def test_skip_state_counts(dit, golden):
    dit.skip_state(reset=True)
    engine_pair(dit, golden, [2], "block")
    assert dit.skip_state(reset=True) == (False, 0, 2, 1)                # blocks 0, 1 from the conditional forward; 3 run (2 is the identity)
    engine_pair(dit, golden, [2], "attention")
    assert dit.skip_state(reset=True) == (False, 0, 2, 2)                # block 2 runs without its self-attention
    engine_pair(dit, golden, [0, 3], "block")
    assert dit.skip_state(reset=True) == (False, 0, 0, 2)
    dit.set_option("skip_share_prefix", 0)
    try:
        engine_pair(dit, golden, [2], "block")
    finally:
        dit.set_option("skip_share_prefix", 1)
    assert dit.skip_state(reset=True) == (False, 0, 0, 3)
    dit.set_skip_guidance([1], 2.0)
    assert dit.skip_state()[0] is True
    dit.set_skip_guidance([1], 0.0)                                      # scale 0 is accepted and means off
    assert dit.skip_state()[0] is False
    dit.clear_skip_guidance()


def test_forward_skip_without_a_set_is_refused(dit, golden):
    from kandinsky import _engine as E
    x, text, pooled, t = forward_args(golden)
    with pytest.raises(ValueError, match="no skip set"):
        dit.forward_skip(x.cuda(), text.cuda(), pooled.cuda(), t, POS, torch.arange(7))
    keep = [x.cuda()]
    a = dit._forward_args(SHAPE[:3], keep[0].data_ptr(), x.shape[-1], text.cuda(), pooled.cuda(), 700.0, POS, torch.arange(7), (1.0, 2.0, 2.0), None, keep)
    out = torch.full((2,) + SHAPE, 3.0, dtype=BF, device="cuda")
    assert E.lib().k5_dit_forward_skip(dit.engine("cuda:0"), C.byref(a), out[0].data_ptr(), out[1].data_ptr(), E.stream_ptr()) == K5_ERR_STATE
    assert "k5_dit_set_skip_guidance" in E.last_error()
    torch.cuda.synchronize()
    assert (out == 3.0).all()


def test_forward_skip_nabla(cfg, sd4, golden_meta):
    attn = golden_meta["nabla_attention"]
    sparse = {"P": attn["P"], "wT": attn["wT"], "wH": attn["wH"], "wW": attn["wW"], "to_fractal": True}
    shape = (3, 16, 16, 16)
    x, text, pooled, t, pos = inputs_at(shape)
    d = make_dit(cfg, sd4)
    d.engine("cuda:0")
    args = (x.cuda(), text.cuda(), pooled.cuda(), t, pos, torch.arange(7))
    plain = d(*args, scale_factor=(1.0, 2.0, 2.0), sparse_params=sparse).clone()
    d.set_skip_guidance([1], 3.0)
    d.reset_softmax_memory()
    c, s = d.forward_skip(*args, scale_factor=(1.0, 2.0, 2.0), sparse_params=sparse)
    d.set_option("skip_share_prefix", 0)
    d.reset_softmax_memory()
    c0, s0 = d.forward_skip(*args, scale_factor=(1.0, 2.0, 2.0), sparse_params=sparse)
    torch.cuda.synchronize()
    assert torch.equal(c, plain) and torch.equal(c0, plain) and torch.equal(s0, s)
    ocfg = O.DitConfig(**cfg)
    osp = O.get_sparse_params(attn, shape[:3], ocfg.patch_size)
    ref = S.dit_forward_skip(sd4, ocfg, x, text, pooled, t, pos, torch.arange(7), (1.0, 2.0, 2.0), osp, "bf16", [1], "block")
    r = rel(s, ref)
    print(f"forward_skip nabla: v_skip vs bf16 oracle {r:.3e}")
    assert r <= 1e-2, r
    assert rel(s, c) > 1e-3
    d._destroy_engine(force=True)


def test_forward_skip_with_fp8_and_a_lora_adapter(cfg):
    """model_dim 256 / ff_dim 512 is the smallest width k5_dit_set_fp8 takes, 256 tokens make the e4m3 GEMMs really run (tests/test_gpu_lora.py):
    with both on the conditional output is still the plain forward's and the branch does not depend on how its prefix was obtained, bit for
    bit.  The distances from the bf16 oracle on the merged weights are printed, not asserted: the oracle does not model e4m3."""
    c = dict(cfg, model_dim=256, ff_dim=512)
    ocfg = O.DitConfig(**c)
    sd = O.synthetic_state_dict(ocfg, seed=5)
    g = torch.Generator().manual_seed(77)
    ent, merged = {}, dict(sd)
    for i, m in enumerate(("visual_transformer_blocks.0.feed_forward.in_layer", "visual_transformer_blocks.2.self_attention.to_query",
                           "visual_transformer_blocks.3.cross_attention.to_key")):
        rows, cols = sd[m + ".weight"].shape
        R = 2 + 3 * i
        ent[m + ".weight"] = (torch.randn(R, cols, generator=g) * 0.05, (torch.randn(rows, R, generator=g) * 0.05).bfloat16(), None)
    x, text, pooled, t, pos = inputs_at((4, 16, 16, 16), seed=78)
    args = (x.cuda(), text.cuda(), pooled.cuda(), t, pos, torch.arange(7))
    d = make_dit(c, sd)
    d.engine("cuda:0")
    bf16_plain = d(*args, scale_factor=(1.0, 2.0, 2.0)).clone()
    d.set_fp8(7)
    d.add_lora(ent)
    d.reset_softmax_memory()
    plain = d(*args, scale_factor=(1.0, 2.0, 2.0)).clone()
    assert not torch.equal(plain, bf16_plain)                            # the e4m3 path and the adapter are really on
    d.set_skip_guidance([1, 2], 3.0, "attention")
    outs = []
    for share in (1, 0):
        d.set_option("skip_share_prefix", share)
        d.reset_softmax_memory()
        cnd, s = d.forward_skip(*args, scale_factor=(1.0, 2.0, 2.0))
        outs.append((cnd.clone(), s.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], plain) and torch.equal(outs[1][0], plain) and torch.equal(outs[0][1], outs[1][1])
    s = outs[0][1]
    assert torch.isfinite(s.float()).all() and rel(s, plain) > 1e-3
    for k, (A, B, _) in ent.items():                                     # W' = W + B A, as k5_lora_merge forms it (strength 1, no alpha)
        merged[k] = sd[k] + B.float() @ A.float()
    ref_c = O.dit_forward(merged, ocfg, x, text, pooled, t, pos, torch.arange(7), (1.0, 2.0, 2.0), None, "bf16")
    ref_s = S.dit_forward_skip(merged, ocfg, x, text, pooled, t, pos, torch.arange(7), (1.0, 2.0, 2.0), None, "bf16", [1, 2], "attention")
    rc, rs = rel(plain, ref_c), rel(s, ref_s)
    print(f"forward_skip fp8 + lora: cond vs bf16 oracle {rc:.3e}, v_skip vs bf16 oracle {rs:.3e}")
    d._destroy_engine(force=True)


# ------------------------------------------------------------------------------------------ sampler: same bits
@pytest.fixture(scope="module")
def plain_runs(dit, golden):
    """the runs without a skip set that the tests below compare against, each computed once"""
    return {w: run_generate(dit, golden, w) for w in (1.0, 5.0)}


def test_off_is_the_plain_run(dit, golden, plain_runs):
    dit.skip_state(reset=True)
    for w in (1.0, 5.0):
        for kw in (dict(slg_blocks=[1], slg_scale=0.0), dict(slg_blocks=[1], slg_scale=3.0, slg_interval=(2.0, 3.0)), dict(slg_blocks=None, slg_scale=3.0),
                   dict(slg_blocks=[], slg_scale=3.0)):
            assert torch.equal(run_generate(dit, golden, w, **kw), plain_runs[w]), (w, kw)
    # ... and below generate, in the engine: a set with scale 0, and one whose mask has no step
    te, ne = prompts(golden)
    from kandinsky.generation_utils import sigma_schedule
    for setup in (lambda: dit.set_skip_guidance([1], 0.0), lambda: dit.set_skip_guidance([1], 3.0, steps=[0] * STEPS)):
        setup()
        try:
            lat = golden["gen.noise"].cuda().contiguous().clone()
            dit.sample(lat, sigma_schedule(STEPS, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0))
            assert torch.equal(lat, plain_runs[5.0])
        finally:
            dit.clear_skip_guidance()
    assert dit.skip_state(reset=True) == (False, 0, 0, 0)


@pytest.fixture(scope="module")
def fused_runs(dit, golden):
    out = {}
    for name, (w, kw) in CASES.items():
        dit.skip_state(reset=True)
        out[name] = (run_generate(dit, golden, w, **kw), dit.skip_state(reset=True))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_stepwise(dit, golden, plain_runs, fused_runs, name):
    w, kw = CASES[name]
    a, counts = fused_runs[name]
    b = run_generate(Wrapped(dit), golden, w, **kw)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    base = run_generate(dit, golden, w, **{k: v for k, v in kw.items() if not k.startswith("slg_")}) if name == "with_zero_star_rescale" else plain_runs[w]
    assert rel(a, base) > 1e-3                                           # the skip term did something
    # skip steps, blocks taken from the conditional forward, blocks run: 4 visual blocks, k0 shared per skip step
    want = {"block_mid": (6, 6 * 1, 6 * 2), "block_first_nocfg": (6, 0, 6 * 3), "attention_interval": (4, 4 * 1, 4 * 3),
            "with_zero_star_rescale": (6, 6 * 2, 6 * 1)}[name]
    assert counts == (False,) + want


class Recorder:
    def __init__(self):
        self.seen = []

    def __call__(self, info):
        self.seen.append(NS(step=info.step, preview=None if info.preview is None else info.preview.clone(),
                            x0=None if info.x0 is None else info.x0.clone()))


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_stepwise_with_editing_and_a_watch(dit, golden, name):
    w, plan = CASES[name]
    g = torch.Generator().manual_seed(5)
    Wf, bf = (torch.rand(16, 3, generator=g) - 0.5) * 0.5, (torch.rand(3, generator=g) - 0.5) * 0.4
    src, mask = source_latent(), edit_mask()
    kw = dict(init_latent=src, strength=1.0, keep_mask=mask, **plan)
    bare = run_generate(dit, golden, w, **kw)
    recs, outs = [], []
    for model in (dit, Wrapped(dit)):
        rec = Recorder()
        outs.append(run_generate(model, golden, w, callback=rec, preview_every=1, preview_factors=(Wf, bf), preview_x0=True, **kw))
        recs.append(rec)
    assert torch.equal(outs[0], bare)                                    # the watch (and the v it asks the update to leave) moves no bit
    assert torch.equal(outs[0], outs[1])
    keep = (mask == 1).expand_as(src)
    assert torch.equal(bare.cpu()[keep], src[keep])
    assert len(recs[0].seen) == len(recs[1].seen) == STEPS
    for a, c in zip(recs[0].seen, recs[1].seen):
        assert a.step == c.step and torch.equal(a.preview, c.preview) and torch.equal(a.x0, c.x0)
    # a strength < 1 run cuts the mask with the schedule: steps 3, 4, 5 of which the interval holds 3 and 4
    if "slg_interval" in plan:
        dit.skip_state(reset=True)
        cut = dict(kw, strength=0.5)
        a = run_generate(dit, golden, w, **cut)
        assert dit.skip_state(reset=True)[1] == 2
        assert torch.equal(a, run_generate(Wrapped(dit), golden, w, **cut))


def test_the_captured_step_equals_the_eager_run(dit, cfg, sd4, golden, fused_runs):
    gdit = make_dit(cfg, sd4)
    gdit.engine("cuda:0")
    gdit.set_graph(True)
    mask_kw = dict(init_latent=source_latent(), keep_mask=edit_mask())
    every = dict(slg_interval=(0.0, 1.0))                                # an interval covering all steps: one kind of step, the capture is used
    for name, (w, kw) in CASES.items():
        gdit.skip_state(reset=True)
        if "slg_interval" in kw:                                         # mixed: runs eagerly on the graph handle too, and matches
            assert torch.equal(run_generate(gdit, golden, w, **kw), fused_runs[name][0]), name
            assert gdit.skip_state(reset=True) == fused_runs[name][1]
        kw = dict(kw, **every)
        dit.skip_state(reset=True)
        eager = run_generate(dit, golden, w, **kw)
        counts = dit.skip_state(reset=True)
        assert torch.equal(run_generate(gdit, golden, w, **kw), eager), name
        assert gdit.skip_state(reset=True) == counts and counts[1] == STEPS   # the replays are counted as the eager launches are
        assert torch.equal(run_generate(gdit, golden, w, **kw, **mask_kw), run_generate(dit, golden, w, **kw, **mask_kw)), name
    gdit._destroy_engine(force=True)


def test_sample_many_equals_two_calls(dit, golden):
    from kandinsky.generation_utils import generate
    g = torch.Generator().manual_seed(41)
    te, ne = prompts(golden)
    te2 = {"text_embeds": torch.randn(5, 96, generator=g).cuda(), "pooled_embed": torch.randn(1, 48, generator=g).cuda()}
    noise = torch.cat([golden["gen.noise"], torch.randn(*SHAPE, generator=g)])
    tes, tps = [te, te2], [torch.arange(7), torch.arange(5)]
    kw = dict(slg_blocks=[1], slg_scale=3.0, slg_interval=INTERVAL)
    dit.skip_state(reset=True)
    out = generate(dit, "cuda:0", (2 * SHAPE[0],) + SHAPE[1:], STEPS, tes, ne, POS, tps, torch.arange(4), 5.0, 5.0, FLASH, noise=noise, batch=2, **kw)
    assert dit.skip_state(reset=True)[1] == 2 * 4
    for b in range(2):
        one = generate(dit, "cuda:0", SHAPE, STEPS, tes[b], ne, POS, tps[b], torch.arange(4), 5.0, 5.0, FLASH, noise=noise[b * 3:(b + 1) * 3], **kw)
        assert torch.equal(out[b * 3:(b + 1) * 3], one), b


# ------------------------------------------------------------------------------------------ parity
@pytest.fixture(scope="module")
def skip_golden():
    from safetensors.torch import load_file
    return load_file(os.path.join(GOLDEN, "dit_tiny_skip.safetensors")), json.load(open(os.path.join(GOLDEN, "dit_tiny_skip_meta.json")))


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_oracle_and_the_reference_golden(fused_runs, sd4, cfg, golden, skip_golden, name):
    gold, meta = skip_golden
    case = meta["cases"][name]
    w, plan = CASES[name]
    assert (meta["steps"], meta["scheduler_scale"], meta["weights_sha256"]) == (STEPS, 5.0, S.weights_sha256(sd4))
    assert (case["blocks"], case["mode"], case["g"], case["w"], tuple(case["interval"]) if "interval" in case else None, case.get("zero_star", False),
            case.get("rescale", 0.0)) == (plan["slg_blocks"], plan.get("slg_mode", "block"), plan["slg_scale"], w, plan.get("slg_interval"),
                                          plan.get("cfg_zero_star", False), plan.get("cfg_rescale", 0.0))
    out = fused_runs[name][0]
    ocfg = O.DitConfig(**cfg)
    noise = golden["gen.noise"]
    zeros = torch.zeros_like(noise), torch.zeros(*noise.shape[:-1], 1)

    def vel(text, pooled, tpos, skip=(), mode="block"):
        return lambda x, s: S.dit_forward_skip(sd4, ocfg, torch.cat([x, *zeros], -1), golden[text], golden[pooled], s.unsqueeze(0) * 1000, POS,
                                               tpos, (1.0, 2.0, 2.0), None, "bf16", skip, mode)
    ref16 = S.bf16_loop(vel("fwd.text", "fwd.pooled", torch.arange(7)), vel("gen.null_text", "gen.null_pooled", torch.arange(4)),
                        vel("fwd.text", "fwd.pooled", torch.arange(7), case["blocks"], case["mode"]), noise, O.sigma_schedule(STEPS, 5.0),
                        [w] * STEPS, case["g"], case["mask"], case.get("zero_star", False), 0, case.get("rescale", 0.0))
    r16, r32 = rel(out, ref16), rel(out, gold[f"skip.{name}.final"])
    print(f"skip {name}: engine vs bf16 oracle {r16:.3e}, vs reference golden {r32:.3e} (oracle vs golden {meta['oracle_vs_golden'][name]:.3e})")
    assert r16 <= 1e-2, r16
    assert r32 <= 3e-2, r32


# ------------------------------------------------------------------------------------------ ranks
@pytest.mark.timeout(600)
def test_loopback_ranks(sd4, cfg):
    from edit_rank_worker import case
    from test_gpu_loopback import run_ranks
    from kandinsky.generation_utils import generate
    shape, noise, te, ne, _, _ = case()
    te, ne = {k: v.cuda() for k, v in te.items()}, {k: v.cuda() for k, v in ne.items()}
    pos = [torch.arange(8)] * 3
    plan = dict(slg_blocks=[1], slg_scale=3.0, slg_interval=(0.6, 0.95))       # 4 steps of scale 5: sigmas 1, .938, .833, .625 -> steps 1, 2, 3

    def call(d, r):
        out = generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, FLASH, noise=noise, **plan)
        assert d.skip_state() == (False, 3, 3, 6)                         # per skip step: block 0 shared, blocks 2 and 3 run
        return out

    make = lambda: make_dit(cfg, sd4)    # noqa: E731
    fused = call(make(), 0)
    outs = run_ranks(2, make, call)
    assert torch.equal(outs[1], outs[0])
    assert rel(outs[0], fused) <= 1e-2, rel(outs[0], fused)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(dit, cfg, sd4, golden):
    from kandinsky import _engine as E
    from kandinsky.generation_utils import context_windows, sigma_schedule
    from kandinsky.magcache_utils import disable_magcache, set_magcache_params, start_magcache_calibration, stop_magcache_calibration
    te, ne = prompts(golden)
    lat = golden["gen.noise"].cuda().contiguous()
    before = lat.clone()

    def refused(d, status, word, steps=2, w=5.0, pos=POS, **kw):
        state = d.skip_state()
        with pytest.raises(RuntimeError, match=f"status {status}") as e:
            d.sample(lat, sigma_schedule(steps, 5.0).tolist(), te, ne, pos, torch.arange(7), torch.arange(4), w, scale_factor=(1.0, 2.0, 2.0), **kw)
        assert word in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(lat, before) and d.skip_state() == state

    dit.skip_state(reset=True)
    try:
        dit.set_skip_guidance([1], 3.0, steps=[1, 0, 1])
        refused(dit, K5_ERR_ARG, "3 steps")                                              # a mask of the wrong length
        dit.set_skip_guidance([1], 3.0)
        starts, weights = context_windows(3, 2, 1)
        refused(dit, K5_ERR_STATE, "window", pos=[torch.arange(2), POS[1], POS[2]], windows=(starts, weights))
    finally:
        dit.clear_skip_guidance()
    assert dit.skip_state() == (False, 0, 0, 0)

    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    n = c["num_steps"]
    d = make_dit(cfg, sd4)
    d.engine("cuda:0")
    d.set_skip_guidance([2], 3.0)
    set_magcache_params(d, c["ratios"], n, c["no_cfg"])
    try:
        refused(d, K5_ERR_STATE, "MagCache is set", steps=n)
    finally:
        disable_magcache(d)
    start_magcache_calibration(d, 2, False)
    try:
        refused(d, K5_ERR_STATE, "calibration")
    finally:
        stop_magcache_calibration(d)
    d._destroy_engine(force=True)
    pair = make_dit(cfg, sd4)
    pair.engine("cuda:0")
    group = E.LoopbackGroup(2)
    pair.enable_cfg_pair_loopback(group, 0)
    pair.set_skip_guidance([2], 3.0)
    refused(pair, K5_ERR_STATE, "CFG pair")
    pair._destroy_engine(force=True)

    # the C entry point itself, and that a refused call is no state: the next plain call runs
    blocks = (C.c_int * 1)(4)
    assert E.lib().k5_dit_set_skip_guidance(dit.engine(lat.device), C.byref(E.SkipGuidance(C.cast(blocks, C.POINTER(C.c_int)), 1, 0, 3.0, None, 0))) == K5_ERR_ARG
    assert b"outside" in E.lib().k5_last_error() and dit.skip_state()[0] is False
    dit.sample(lat, sigma_schedule(2, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0))
    torch.cuda.synchronize()
    assert torch.isfinite(lat).all() and not torch.equal(lat, before)
