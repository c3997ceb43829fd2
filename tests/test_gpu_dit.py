"""GPU parity of the whole engine (C ABI k5_dit_forward / k5_sample) against the CPU oracle in
bf16-island mode and against the golden vectors produced by the reference (fp32).

Stated tolerances (north_star: "within a stated fp tolerance on the final latent"):
  * engine vs bf16-island oracle (same rounding points, different fp32 summation order):
      relative L2 <= 1.5e-2 on a velocity, <= 1e-2 on a final latent
  * engine vs the reference's fp32 vectors: relative L2 <= 3e-2 (this is the bf16 autocast noise the
      reference itself has on a GPU; the bf16-island oracle sits at the same distance)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
from kit import POS, cfg, make_dit, need_gpu, rel  # noqa: E402


@pytest.fixture(scope="module")
def tiny_dit(cfg, tiny_sd):
    need_gpu()
    return make_dit(cfg, tiny_sd)


def test_forward_tiny_vs_oracle_and_golden(tiny_dit, tiny_sd, cfg, golden):
    out = tiny_dit(golden["fwd.x"].cuda(), golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), golden["fwd.time"],
                   POS, torch.arange(7), scale_factor=(1.0, 2.0, 2.0))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (3, 8, 12, 16)
    ref16 = O.dit_forward(tiny_sd, O.DitConfig(**cfg), golden["fwd.x"], golden["fwd.text"], golden["fwd.pooled"],
                          golden["fwd.time"], POS, torch.arange(7), (1.0, 2.0, 2.0), None, "bf16")
    assert rel(out, ref16) <= 1.5e-2, rel(out, ref16)
    assert rel(out, golden["fwd.out"]) <= 3e-2, rel(out, golden["fwd.out"])
    assert rel(ref16, golden["fwd.out"]) <= 3e-2


def test_weights_pack_identically_from_host_or_device_in_any_dtype(tiny_sd, cfg, golden):
    """k5_dit_load_tensor stages a matrix as a raw copy on the device (D2D for a checkpoint that already lives there) and
    k5_dit_finalize converts / pads / concatenates it with a device kernel: the same bf16-representable checkpoint loaded from CPU
    fp32, GPU fp32, GPU bf16, CPU bf16 and GPU fp16-of-the-bf16-values must give bit-identical forwards (the packed weights are the
    same bits).  fp16 cannot hold every bf16 value, so its source is the fp16-AND-bf16 representable rounding of the checkpoint."""
    from kandinsky.models.dit import DiffusionTransformer3D
    base = {k: v.half().bfloat16().float() for k, v in tiny_sd.items()}     # representable in both 16-bit formats (tiny weights: no overflow)
    assert all(torch.equal(v.half().float(), v) and torch.equal(v.bfloat16().float(), v) for v in base.values())
    args = (golden["fwd.x"].cuda(), golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), golden["fwd.time"], POS, torch.arange(7))

    def run(sd, to_cuda):
        d = DiffusionTransformer3D(**cfg)
        d.load_state_dict(sd, assign=True)
        if to_cuda:
            d = d.to("cuda:0")
        else:
            d.engine("cuda:0")                       # parameters stay on the host: H2D of the raw bytes, then the same device pack
        return d(*args, scale_factor=(1.0, 2.0, 2.0))

    ref = run(base, False)
    assert torch.isfinite(ref.float()).all()
    for name, sd, to_cuda in (("gpu fp32", base, True), ("gpu bf16", {k: v.bfloat16() for k, v in base.items()}, True),
                              ("cpu bf16", {k: v.bfloat16() for k, v in base.items()}, False),
                              ("gpu fp16", {k: v.half() for k, v in base.items()}, True)):
        out = run(sd, to_cuda)
        assert torch.equal(out, ref), name


def test_forward_accepts_bf16_text_and_16_channel_x(tiny_dit, golden):
    a = tiny_dit(golden["fwd.x"].cuda(), golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), golden["fwd.time"],
                 POS, torch.arange(7), scale_factor=(1.0, 2.0, 2.0))
    x = golden["fwd.x"].clone()
    assert torch.count_nonzero(x[..., 16:]) > 0  # golden x has random cond channels -> zero them for this check
    x[..., 16:] = 0
    b = tiny_dit(x.cuda(), golden["fwd.text"].cuda().bfloat16(), golden["fwd.pooled"].cuda().bfloat16(),
                 golden["fwd.time"], POS, torch.arange(7), scale_factor=(1.0, 2.0, 2.0))
    c = tiny_dit(x[..., :16].contiguous().cuda(), golden["fwd.text"].cuda().bfloat16(),
                 golden["fwd.pooled"].cuda().bfloat16(), golden["fwd.time"], POS, torch.arange(7),
                 scale_factor=(1.0, 2.0, 2.0))
    assert torch.equal(b, c)          # implied-zero cond channels == explicit zeros
    assert rel(b, a) > 1e-3           # and the cond channels do matter when non-zero


@pytest.mark.parametrize("case", [(4, 5.0, 1.0), (4, 5.0, 5.0), (3, 10.0, 3.0), (16, 5.0, 1.0)])
def test_generate_trajectory(tiny_dit, tiny_sd, cfg, golden, case):
    from types import SimpleNamespace as NS
    from kandinsky.generation_utils import generate
    steps, s, w = case
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")),
              metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    te = {"text_embeds": golden["fwd.text"].cuda(), "pooled_embed": golden["fwd.pooled"].cuda()}
    ne = {"text_embeds": golden["gen.null_text"].cuda(), "pooled_embed": golden["gen.null_pooled"].cuda()}
    out = generate(tiny_dit, "cuda:0", (3, 8, 12, 16), steps, te, ne, POS, torch.arange(7), torch.arange(4), w, s, conf,
                   noise=golden["gen.noise"])
    assert out.dtype == torch.float32
    tag = f"gen.{steps}_{s}_{w}"
    tec = {k: v.cpu() for k, v in te.items()}
    nec = {k: v.cpu() for k, v in ne.items()}
    ref16 = O.generate(tiny_sd, O.DitConfig(**cfg), golden["gen.noise"], steps, tec, nec, POS, torch.arange(7),
                       torch.arange(4), w, s, (1.0, 2.0, 2.0), None, "bf16")
    assert rel(out, ref16) <= 1e-2, rel(out, ref16)
    assert rel(out, golden[tag + ".final"]) <= 3e-2, rel(out, golden[tag + ".final"])


def test_stepwise_generate_equals_fused_sample(tiny_dit, golden):
    """The duck-typed per-step path (model(...) + k5_cfg_euler) and the one-call k5_sample agree bit for bit."""
    from types import SimpleNamespace as NS
    from kandinsky.generation_utils import generate

    class Wrapped(torch.nn.Module):  # any non-DiffusionTransformer3D callable takes the per-step path
        def __init__(self, m):
            super().__init__()
            self.m, self.visual_cond = m, m.visual_cond

        def forward(self, *a, **k):
            return self.m(*a, **k)

    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")),
              metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    te = {"text_embeds": golden["fwd.text"].cuda(), "pooled_embed": golden["fwd.pooled"].cuda()}
    ne = {"text_embeds": golden["gen.null_text"].cuda(), "pooled_embed": golden["gen.null_pooled"].cuda()}
    args = ("cuda:0", (3, 8, 12, 16), 4, te, ne, POS, torch.arange(7), torch.arange(4), 5.0, 5.0, conf)
    a = generate(tiny_dit, *args, noise=golden["gen.noise"])
    b = generate(Wrapped(tiny_dit), *args, noise=golden["gen.noise"])
    assert torch.equal(a, b)


def test_full_width_two_blocks_vs_oracle():
    """Full 2B-Lite width (D=1792, 28 heads, FF=7168, text 3584/768) with 2 visual blocks on a
    (5,16,16) latent (320 tokens, ragged vs every tile size): engine vs the bf16-island oracle."""
    from kandinsky.models.dit import DiffusionTransformer3D
    c = dict(O.LITE_2B, num_visual_blocks=2, num_text_blocks=1)
    cfg = O.DitConfig(**c)
    sd = O.synthetic_state_dict(cfg, seed=3)
    dit = DiffusionTransformer3D(**c)
    dit.load_state_dict(sd, assign=True)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(5, 16, 16, 16, generator=g)
    text, pooled = torch.randn(37, 3584, generator=g), torch.randn(1, 768, generator=g)
    pos = [torch.arange(5), torch.arange(8), torch.arange(8)]
    t = torch.tensor([875.0])
    out = dit.to("cuda:0")(x.cuda(), text.cuda(), pooled.cuda(), t, pos, torch.arange(37), scale_factor=(1.0, 2.0, 2.0))
    xin = torch.cat([x, torch.zeros(5, 16, 16, 17)], dim=-1)
    ref = O.dit_forward(sd, cfg, xin, text, pooled, t, pos, torch.arange(37), (1.0, 2.0, 2.0), None, "bf16")
    assert rel(out, ref) <= 1.5e-2, rel(out, ref)
    ref32 = O.dit_forward(sd, cfg, xin, text, pooled, t, pos, torch.arange(37), (1.0, 2.0, 2.0), None, "fp32")
    assert rel(out, ref32) <= 3e-2, rel(out, ref32)
    # the engine's dense visual self-attention uses keys pre-multiplied by log2(e)/8 (one bf16 rounding): the oracle with the
    # same rounding point is closer still
    O.PRESCALE_K = True
    try:
        refp = O.dit_forward(sd, cfg, xin, text, pooled, t, pos, torch.arange(37), (1.0, 2.0, 2.0), None, "bf16")
    finally:
        O.PRESCALE_K = False
    print(f"full width: engine vs bf16-island oracle {rel(out, ref):.3e}, vs oracle with pre-scaled keys {rel(out, refp):.3e}, vs fp32 {rel(out, ref32):.3e}")
    assert rel(out, refp) <= 1.5e-2, rel(out, refp)
    # and against the REFERENCE's own output on the same inputs / seeded weights (tests/golden/dit_fullwidth.*)
    import json
    import os
    from safetensors.torch import load_file
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    G, meta = load_file(os.path.join(here, "dit_fullwidth.safetensors")), json.load(open(os.path.join(here, "dit_fullwidth_meta.json")))
    assert meta["weights_seed"] == 3 and torch.equal(G["x"], x) and torch.equal(G["text"], text)
    got = out.float().cpu().reshape(-1)[G["sample_idx"]]
    assert rel(got, G["sample_val"]) <= 3e-2, rel(got, G["sample_val"])


# ------------------------------------------------------------------------------------------ QK-norm gains != 1
def _qk_gain_sd(cfg, case):
    """seed-3 synthetic weights with the QK-norm gains (query_norm / key_norm, 64 each) of every attention replaced"""
    sd = O.synthetic_state_dict(cfg, seed=3)
    g = torch.Generator().manual_seed(77)
    for k in sorted(sd):
        if k.endswith(("query_norm.weight", "key_norm.weight")):
            if case == "n05":
                sd[k] = 1.0 + 0.5 * torch.randn(64, generator=g)
            elif case == "x3":
                sd[k] = torch.full((64,), 3.0)
            elif case == "ch8":
                w = torch.ones(64); w[int(torch.randint(0, 64, (1,), generator=g))] = 8.0
                sd[k] = w
            elif case == "x2":
                sd[k] = torch.full((64,), 2.0)
            elif case == "x5":
                sd[k] = torch.full((64,), 5.0)
            elif case == "x6":
                sd[k] = torch.full((64,), 6.0)
            else:
                raise ValueError(case)
    return sd


@pytest.mark.parametrize("case,w,graph,expect_used", [("x2", 1.0, 0, 1), ("n05", 5.0, 0, 1), ("x2", 5.0, 1, 1), ("x6", 1.0, 0, 0), ("x5", 5.0, 1, 0)])
def test_sample_decides_where_the_queries_are_normalised_same_bits(case, w, graph, expect_used):
    """k5_sample's per-call choice ("attn_fuse_qnorm_auto", default on): step 0 runs the standalone norm + RoPE pass and records whether any head left
    the plain fixed-offset form; if none did, steps 1.. normalise the queries inside the attention kernel.  Demanded here: the decision is the
    one the data call for (gains 2 / N(1, 0.5): fused; gains 5 / 6, beyond the window — anchored offsets need the stored queries: not fused), and
    the latent is BIT-IDENTICAL to the run with the choice switched off either way, eagerly and with the hipGraph-captured step, with and without CFG."""
    from kandinsky.generation_utils import sigma_schedule
    from kandinsky.models.dit import DiffusionTransformer3D
    c = dict(O.LITE_2B, num_visual_blocks=2, num_text_blocks=1)
    sd = _qk_gain_sd(O.DitConfig(**c), case)
    dit = DiffusionTransformer3D(**c)
    dit.load_state_dict(sd, assign=True)
    dit = dit.to("cuda:0")
    dit.engine("cuda:0")
    g = torch.Generator().manual_seed(21)
    noise = torch.randn(5, 16, 16, 16, generator=g)
    te = {"text_embeds": torch.randn(37, 3584, generator=g).cuda(), "pooled_embed": torch.randn(1, 768, generator=g).cuda()}
    ne = {"text_embeds": torch.randn(9, 3584, generator=g).cuda(), "pooled_embed": torch.randn(1, 768, generator=g).cuda()}
    pos = [torch.arange(5), torch.arange(8), torch.arange(8)]
    sig = sigma_schedule(4, 5.0).tolist()
    outs, used = {}, {}
    for auto in (0, 1):
        dit.set_option("attn_fuse_qnorm_auto", auto)
        dit.set_graph(bool(graph))
        lat = noise.clone().cuda()
        dit.sample(lat, sig, te, ne, pos, torch.arange(37), torch.arange(9), w, scale_factor=(1.0, 2.0, 2.0))
        torch.cuda.synchronize()
        outs[auto], used[auto] = lat.clone(), dit.get_option("attn_fuse_qnorm_used")
    assert used[0] == -1 and used[1] == expect_used, used
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1]), f"max |diff| {(outs[0] - outs[1]).abs().max().item():.3e}"
    # a forward outside k5_sample is never affected by the last call's decision
    dit.set_graph(False)
    x = noise.cuda()
    a = dit(x, te["text_embeds"], te["pooled_embed"], torch.tensor([500.0]), pos, torch.arange(37), scale_factor=(1.0, 2.0, 2.0))
    dit.set_option("attn_fuse_qnorm_auto", 0)
    b = dit(x, te["text_embeds"], te["pooled_embed"], torch.tensor([500.0]), pos, torch.arange(37), scale_factor=(1.0, 2.0, 2.0))
    assert torch.equal(a, b)


@pytest.mark.parametrize("case,expect,row_offsets,qfuse,anchor", [("n05", "fixed", 1, 0, 1), ("x2", "fixed", 1, 0, 1), ("ch8", "fixed", 1, 0, 1),
                                                                  ("x3", "fixed", 1, 0, 1), ("x3", "online", 0, 0, 1), ("x5", "fixed", 1, 0, 1),
                                                                  ("x5", "any", 1, 0, 0), ("x6", "fixed", 1, 0, 1), ("x6", "online", 1, 0, 0),
                                                                  ("ch8", "any", 1, 1, 1), ("x3", "fixed", 1, 1, 1), ("x6", "online", 1, 1, 1)])
def test_full_width_qk_norm_gains_vs_oracle(case, expect, row_offsets, qfuse, anchor):
    """The engine on QK-norm gains a trained checkpoint could have: N(1, 0.5), every gain 2 (|q||k'| = 64 * 4 * 0.18 = 46),
    every gain 3 (104: outside the offset-0 window of 90, inside the per-row-offset one of 190 — fixed form with the engine's
    default, online max with "attn_row_offsets" = 0), every gain 5 (288) / 6 (415) / one channel at 8 (the bound depends on how much of a
    row's energy sits in that channel) — beyond the Cauchy-Schwarz window: the fixed form on ANCHORED offsets with the engine's default
    ("attn_anchor"; with the fused query norm there are no normalised queries to anchor on), the online max / either form without.  The softmax form is chosen per head ON THE
    DEVICE from the data; the test states which one must have run and demands oracle parity either way (round 1 derived the
    bound from max|w| and never left the fixed-offset branch in any engine-level test).
    qfuse = 1 ("attn_fuse_qnorm"): the queries are normalised inside the attention kernel and the fixed-offset workgroups take the
    head-level decision themselves (no max|q|^2 statistic exists then) — same expectations."""
    from kandinsky.models.dit import DiffusionTransformer3D
    c = dict(O.LITE_2B, num_visual_blocks=2, num_text_blocks=1)
    cfg = O.DitConfig(**c)
    sd = _qk_gain_sd(cfg, case)
    dit = DiffusionTransformer3D(**c)
    dit.load_state_dict(sd, assign=True)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(5, 16, 16, 16, generator=g)
    text, pooled = torch.randn(37, 3584, generator=g), torch.randn(1, 768, generator=g)
    pos = [torch.arange(5), torch.arange(8), torch.arange(8)]
    t = torch.tensor([875.0])
    dit = dit.to("cuda:0")
    dit.engine("cuda:0")
    dit.set_option("attn_row_offsets", row_offsets)
    dit.set_option("attn_fuse_qnorm", qfuse)
    dit.set_option("attn_anchor", anchor)
    args = (x.cuda(), text.cuda(), pooled.cuda(), t, pos, torch.arange(37))
    out = dit(*args, scale_factor=(1.0, 2.0, 2.0))
    n_fixed, n_online = dit.attn_variant_counts(reset=True)
    assert n_fixed + n_online == 2 * 28                                  # 2 visual blocks x 28 heads were flagged
    if expect == "fixed":
        assert n_online == 0, (n_fixed, n_online)
    elif expect == "online":
        assert n_fixed == 0, (n_fixed, n_online)
    xin = torch.cat([x, torch.zeros(5, 16, 16, 17)], dim=-1)
    O.PRESCALE_K = True
    try:
        refp = O.dit_forward(sd, cfg, xin, text, pooled, t, pos, torch.arange(37), (1.0, 2.0, 2.0), None, "bf16")
    finally:
        O.PRESCALE_K = False
    ref32 = O.dit_forward(sd, cfg, xin, text, pooled, t, pos, torch.arange(37), (1.0, 2.0, 2.0), None, "fp32")
    noise = rel(refp, ref32)   # what bf16 storage of q, k, P costs the ORACLE on these weights: larger gains = peakier softmax
    print(f"qk gains {case}: fixed/online heads {n_fixed}/{n_online}; engine vs bf16 oracle {rel(out, refp):.3e}, vs fp32 "
          f"{rel(out, ref32):.3e}; bf16 oracle vs fp32 oracle {noise:.3e}")
    # tolerance: the suite's 1.5e-2 / 3e-2, or the bf16 noise floor of the case itself where that is larger (gain 3: logits 9x)
    tol16, tol32 = max(1.5e-2, 0.75 * noise), max(3e-2, 1.5 * noise)
    assert rel(out, refp) <= tol16, rel(out, refp)
    assert rel(out, ref32) <= tol32, rel(out, ref32)
    # the other form on the same weights: online max everywhere — same velocity up to the softmax's bf16 noise
    dit.set_option("attn_mode", 1)
    out_on = dit(*args, scale_factor=(1.0, 2.0, 2.0))
    dit.set_option("attn_mode", 0)
    assert dit.attn_variant_counts(reset=True) == (0, 0)                 # forced mode: no flags are computed
    assert rel(out_on, refp) <= tol16, rel(out_on, refp)
    assert rel(out_on, out) <= max(1e-2, 0.5 * noise), rel(out_on, out)    # two valid forms: apart by at most the case's own bf16 noise


# ------------------------------------------------------------------------------------------ MagCache
@pytest.mark.parametrize("tag", ["sft_12", "nocfg_9", "hand_10", "sft_50", "nocfg_50"])   # the 50-step cases: the configs' own schedules and ratio tables
def test_magcache_generate(tiny_dit, tiny_sd, cfg, golden, tag):
    """`set_magcache_params` + generate: the engine's skip pattern is the reference's, the final latent matches the
    bf16-island oracle running the same state machine and the reference's own fp32 result."""
    import json
    import os
    from types import SimpleNamespace as NS
    from safetensors.torch import load_file
    from kandinsky.generation_utils import generate
    from kandinsky.magcache_utils import set_magcache_params, disable_magcache, magcache_state
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    T = load_file(os.path.join(here, "magcache_tiny.safetensors"))
    c = [c for c in json.load(open(os.path.join(here, "magcache_meta.json")))["cases"] if c["tag"] == tag][0]
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")),
              metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    te = {"text_embeds": golden["fwd.text"].cuda(), "pooled_embed": golden["fwd.pooled"].cuda()}
    ne = {"text_embeds": golden["gen.null_text"].cuda(), "pooled_embed": golden["gen.null_pooled"].cuda()}
    tiny_dit.engine("cuda:0")
    try:
        set_magcache_params(tiny_dit, c["ratios"], c["num_steps"], c["no_cfg"])
        assert torch.equal(torch.from_numpy(tiny_dit.mag_ratios), T[f"mag.{tag}.table"])
        out = generate(tiny_dit, "cuda:0", (3, 8, 12, 16), c["num_steps"], te, ne, POS, torch.arange(7), torch.arange(4),
                       c["guidance_weight"], c["scheduler_scale"], conf, noise=golden["gen.noise"])
        cnt, ran, skipped = magcache_state(tiny_dit)
        assert (cnt, ran, skipped) == (0, sum(c["ran_blocks"]), len(c["ran_blocks"]) - sum(c["ran_blocks"]))
    finally:
        disable_magcache(tiny_dit)
    mc = O.MagCache(c["ratios"], c["num_steps"], c["no_cfg"])
    ref16 = O.generate(tiny_sd, O.DitConfig(**cfg), golden["gen.noise"], c["num_steps"], {k: v.cpu() for k, v in te.items()},
                       {k: v.cpu() for k, v in ne.items()}, POS, torch.arange(7), torch.arange(4), c["guidance_weight"],
                       c["scheduler_scale"], (1.0, 2.0, 2.0), None, "bf16", magcache=mc)
    assert rel(out, ref16) <= 1e-2, rel(out, ref16)
    assert rel(out, T[f"mag.{tag}.final"]) <= 3e-2, rel(out, T[f"mag.{tag}.final"])
    # and it is a different result from the un-cached run (the cache is really applied)
    plain = generate(tiny_dit, "cuda:0", (3, 8, 12, 16), c["num_steps"], te, ne, POS, torch.arange(7), torch.arange(4),
                     c["guidance_weight"], c["scheduler_scale"], conf, noise=golden["gen.noise"])
    assert rel(out, plain) > 1e-4


# ------------------------------------------------------------------------------------------ hipGraph-captured step
@pytest.mark.parametrize("w,sp", [(1.0, False), (5.0, False), (3.0, True)])
def test_graph_captured_step_is_bit_identical(cfg, tiny_sd, golden, w, sp):
    """k5_dit_set_graph: one captured sampler step replayed for steps 1..n-1 (device-side step counter) == the eager loop,
    bit for bit; also through the sequence-parallel path (side stream + RCCL inside the capture, world = 1 communicator)."""
    from types import SimpleNamespace as NS
    from kandinsky.generation_utils import generate
    from kandinsky.models.dit import DiffusionTransformer3D
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    te = {"text_embeds": golden["fwd.text"].cuda(), "pooled_embed": golden["fwd.pooled"].cuda()}
    ne = {"text_embeds": golden["gen.null_text"].cuda(), "pooled_embed": golden["gen.null_pooled"].cuda()}
    shape, pos = ((3, 8, 12, 16), POS) if not sp else ((2, 16, 16, 16), [torch.arange(2), torch.arange(8), torch.arange(8)])
    noise = golden["gen.noise"] if not sp else torch.randn(*shape, generator=torch.Generator().manual_seed(9))
    outs = []
    for graph in (False, True):
        dit = DiffusionTransformer3D(**cfg)
        dit.load_state_dict(tiny_sd, assign=True)
        dit = dit.to("cuda:0")
        dit.engine("cuda:0")
        if sp:
            dit.enable_sequence_parallel(0, 1, device="cuda:0")
        dit.set_graph(graph)
        outs.append(generate(dit, "cuda:0", shape, 6, te, ne, pos, torch.arange(7), torch.arange(4), w, 5.0, conf, noise=noise))
        del dit
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def test_text_rope_cache_eviction_keeps_the_handle_intact(tiny_dit, golden):
    """More than 8 distinct prompt lengths on one handle evict the RoPE1D cache — and nothing else (regression: the
    eviction once released the sequence-parallel buffers and the communicator)."""
    x = golden["fwd.x"].cuda()
    g = torch.Generator().manual_seed(4)
    first = None
    for L in list(range(3, 14)) + [3]:
        out = tiny_dit(x, torch.randn(L, 96, generator=g).cuda() if L != 3 else golden["fwd.text"][:3].cuda(),
                       golden["fwd.pooled"].cuda(), golden["fwd.time"], POS, torch.arange(L), scale_factor=(1.0, 2.0, 2.0))
        assert torch.isfinite(out.float()).all()
        if L == 3:
            if first is None:
                first = out.clone()
            else:
                assert torch.equal(out, first)


# ------------------------------------------------------------------------------------------ fp8 feed-forward (opt-in, lossy)
@pytest.mark.parametrize("mask", [1, 3, 7])
def test_fp8_feed_forward_mode(mask):
    """k5_dit_set_fp8 (BASELINE config 5 "fp8 MFMA weights"): linear layers of the visual blocks in W8A8 e4m3 — mask 1 the feed-forward GEMMs,
    3 + the q | k | V^T projections, 7 + the out projection of the self-attention.  Parity with the oracle restating the same quantisation
    (per-channel weight scales, static activation scale, e4m3 GELU output); the distance to the bf16 path is what the mode costs — stated
    here per layer class, it is why the mode is opt-in."""
    from kandinsky.models.dit import DiffusionTransformer3D
    c = dict(O.LITE_2B, num_visual_blocks=2, num_text_blocks=1)
    cfg = O.DitConfig(**c)
    sd = O.synthetic_state_dict(cfg, seed=3)
    dit = DiffusionTransformer3D(**c)
    dit.load_state_dict(sd, assign=True)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(5, 16, 16, 16, generator=g)
    text, pooled = torch.randn(37, 3584, generator=g), torch.randn(1, 768, generator=g)
    pos = [torch.arange(5), torch.arange(8), torch.arange(8)]
    t = torch.tensor([875.0])
    dit = dit.to("cuda:0")
    args = (x.cuda(), text.cuda(), pooled.cuda(), t, pos, torch.arange(37))
    plain = dit(*args, scale_factor=(1.0, 2.0, 2.0))
    dit.set_fp8(mask)
    out8 = dit(*args, scale_factor=(1.0, 2.0, 2.0))
    dit.set_option("fp8_fuse_ln", 0)     # LayerNorm -> bf16 h -> quantisation pass, instead of the LayerNorm writing the e4m3 rows itself: the same bits
    assert torch.equal(dit(*args, scale_factor=(1.0, 2.0, 2.0)), out8)
    dit.set_option("fp8_fuse_ln", 1)
    dit.set_fp8(False)
    assert torch.equal(dit(*args, scale_factor=(1.0, 2.0, 2.0)), plain)          # switching back restores the bf16 path exactly
    xin = torch.cat([x, torch.zeros(5, 16, 16, 17)], dim=-1)
    O.FP8_FF, O.FP8_QKV, O.FP8_OUT = bool(mask & 1), bool(mask & 2), bool(mask & 4)
    try:
        ref8 = O.dit_forward(sd, cfg, xin, text, pooled, t, pos, torch.arange(37), (1.0, 2.0, 2.0), None, "bf16")
    finally:
        O.FP8_FF = O.FP8_QKV = O.FP8_OUT = False
    # same quantisation in both; bf16-ulp differences upstream flip e4m3 roundings (6 % steps), so the two agree to a few
    # 1e-2 only — the kernels themselves are checked exactly in tests/test_gpu_kernels.py::test_gemm_fp8_*
    cost = rel(out8, plain)
    print(f"fp8 mode, mask {mask}: engine vs fp8 oracle {rel(out8, ref8):.3e}; engine fp8 vs engine bf16 {cost:.3e}; fp8 oracle vs bf16 engine {rel(ref8, plain):.3e}")
    assert rel(out8, ref8) <= (4e-2 if mask == 1 else 6e-2), rel(out8, ref8)
    assert 1e-3 < cost <= (8e-2 if mask == 1 else 1.5e-1), cost                   # the price of 3 mantissa bits


# ------------------------------------------------------------------------------------------ BASELINE configs at their own sizes
def _two_block_model(gain):
    from kandinsky.models.dit import DiffusionTransformer3D
    c = dict(O.LITE_2B, num_visual_blocks=2, num_text_blocks=1)
    cfg = O.DitConfig(**c)
    sd = O.synthetic_state_dict(cfg, seed=3)
    if gain != 1.0:
        for k in sd:
            if k.endswith(("query_norm.weight", "key_norm.weight")):
                sd[k] = torch.full((64,), gain)
    dit = DiffusionTransformer3D(**c)
    dit.load_state_dict(sd, assign=True)
    return dit.to("cuda:0"), sd, cfg


def test_config2_length_forward_vs_reference_golden():
    """k5_dit_forward at the length bench.py times — BASELINE config 2's (31, 64, 96) latent = 47 616 tokens, 256 text tokens, full
    width, 2 visual blocks — against the REFERENCE's own forward (dit.py:155-181, fp32; oracle/gen_golden_fullwidth_long.py) on the
    same seeded weights and inputs: 16384 sampled outputs and the whole-tensor sums.  Tolerance: the bf16-vs-fp32 distance of the
    short full-width case (3e-2); the balanced dense launch (5208 jobs: full rounds + split tail + merge), the per-head softmax-form
    choice and every workspace are the ones of the timed configuration."""
    import json
    import os
    from safetensors.torch import load_file
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    G, meta = load_file(os.path.join(here, "dit_fullwidth_long.safetensors")), json.load(open(os.path.join(here, "dit_fullwidth_long_meta.json")))
    dit, _, _ = _two_block_model(meta["qk_gain"])
    T, H, W = meta["latent"]
    L = meta["text_len"]
    g = torch.Generator().manual_seed(meta["input_seed"])
    x = torch.randn(T, H, W, 16, generator=g)
    text, pooled = torch.randn(L, 3584, generator=g), torch.randn(1, 768, generator=g)
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    dit.engine("cuda:0")
    dit.attn_variant_counts(reset=True)
    out = dit(x.cuda(), text.cuda(), pooled.cuda(), torch.tensor([meta["time"]]), pos, torch.arange(L), scale_factor=(1.0, 2.0, 2.0))
    torch.cuda.synchronize()
    assert list(out.shape) == meta["out_shape"]
    n_fixed, n_online = dit.attn_variant_counts()
    flat = out.float().reshape(-1)
    got = flat[G["sample_idx"].cuda()].cpu()
    r = rel(got, G["sample_val"])
    s, ss = flat.double().sum().item(), flat.double().pow(2).sum().item()
    print(f"config-2 length (N = {T * H * W // 4}): engine vs reference fp32 {r:.3e} on {got.numel()} samples; sum {s:.4e} / {meta['out_sum']:.4e}, "
          f"sumsq {ss:.5e} / {meta['out_sumsq']:.5e}; heads fixed / online {n_fixed} / {n_online}")
    assert r <= 3e-2, r
    assert abs(ss - meta["out_sumsq"]) <= 3e-2 * meta["out_sumsq"]
    assert abs(s - meta["out_sum"]) <= 3e-2 * (meta["out_sumsq"] * flat.numel()) ** 0.5
    assert n_fixed == 2 * 28 and n_online == 0           # gain 1.5: |q||k'| = 64 * 2.25 * 0.18 = 26 -> offset-0 fixed form on every head


def test_config1_plumbing_run_vs_oracle():
    """BASELINE config 1 (config_5s_distil: 256x256, 2 s -> latent (13, 32, 32) = 3328 tokens, NFE 16, guidance 1 -> one forward per
    step): the whole 16-step sampler through generate() at full width with 2 visual blocks, against the bf16-island oracle's
    generate on the host (the oracle is pinned to the reference's trajectories by the G4 goldens).  `generate` is called directly, as
    SURVEY §8d prescribes — the pipeline itself rejects 256x256 (t2v_pipeline.py:43-45)."""
    from types import SimpleNamespace as NS
    from kandinsky.generation_utils import generate
    dit, sd, cfg = _two_block_model(1.0)
    T, H, W, L, Ln = 13, 32, 32, 48, 8
    g = torch.Generator().manual_seed(21)
    noise = torch.randn(T, H, W, 16, generator=g)
    te = {"text_embeds": torch.randn(L, 3584, generator=g), "pooled_embed": torch.randn(1, 768, generator=g)}
    ne = {"text_embeds": torch.randn(Ln, 3584, generator=g), "pooled_embed": torch.randn(1, 768, generator=g)}
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))
    cu = lambda d: {k: v.cuda() for k, v in d.items()}   # noqa: E731
    lat = generate(dit, "cuda:0", (T, H, W, 16), 16, cu(te), cu(ne), pos, torch.arange(L), torch.arange(Ln), 1.0, 5.0, conf, noise=noise)
    ref = O.generate(sd, cfg, noise, 16, te, ne, pos, torch.arange(L), torch.arange(Ln), 1.0, 5.0, (1.0, 2.0, 2.0), None, "bf16")
    r = rel(lat, ref)
    print(f"config 1 (13,32,32) x 16 steps, w = 1: final latent engine vs bf16-island oracle {r:.3e}; moved {rel(ref, noise):.3f} from the noise")
    assert r <= 1e-2, r
    assert rel(ref, noise) > 0.05                         # the sampler really moved the latent (the check is not noise vs noise)


def test_config3_cfg_step_at_full_length_vs_reference_golden():
    """BASELINE config 3 (config_5s_sft: CFG, two forwards per step) at its own size: ONE Euler step of the reference's own generate()
    (generation_utils.py:80-129: seeded noise, sigma schedule, get_velocity with guidance 5, Euler update; fp32, oracle/
    gen_golden_fullwidth_long.py cfg) on the (31, 64, 96) latent = 47 616 tokens, full width, 2 blocks — through k5_sample (cond forward,
    uncond forward, bf16 combine, fp32 Euler in one C call).  Compared on 16384 samples of the UPDATE the step applied (latent - noise:
    the velocity's bf16 noise is not hidden behind the unit-variance noise) and of the latent itself."""
    import json
    import os
    from safetensors.torch import load_file
    from kandinsky.generation_utils import sigma_schedule
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    G, meta = load_file(os.path.join(here, "dit_fullwidth_long_cfg.safetensors")), json.load(open(os.path.join(here, "dit_fullwidth_long_meta.json")))
    c = meta["cfg"]
    dit, _, _ = _two_block_model(meta["qk_gain"])
    T, H, W = meta["latent"]
    L = meta["text_len"]
    g = torch.Generator().manual_seed(meta["input_seed"])
    torch.randn(T, H, W, 16, generator=g)                                    # the forward golden's latent: same generator stream as the generator script
    text, pooled = torch.randn(L, 3584, generator=g), torch.randn(1, 768, generator=g)
    g2 = torch.Generator().manual_seed(c["null_seed"])
    ntext, npooled = torch.randn(c["null_text_len"], 3584, generator=g2), torch.randn(1, 768, generator=g2)
    noise = torch.randn(T, H, W, 16, generator=torch.Generator().manual_seed(c["seed"]))
    lat = noise.clone().cuda()
    sig = sigma_schedule(c["num_steps"], c["scheduler_scale"]).tolist()
    pos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    dit.sample(lat, sig[:2], {"text_embeds": text.cuda(), "pooled_embed": pooled.cuda()}, {"text_embeds": ntext.cuda(), "pooled_embed": npooled.cuda()},
               pos, torch.arange(L), torch.arange(c["null_text_len"]), c["guidance_weight"], scale_factor=(1.0, 2.0, 2.0))
    torch.cuda.synchronize()
    idx = G["sample_idx"]
    got_lat = lat.reshape(-1)[idx.cuda()].cpu()
    got_upd = got_lat - noise.reshape(-1)[idx]
    r_upd, r_lat = rel(got_upd, G["update_val"]), rel(got_lat, G["latent_val"])
    ss = (lat.cpu() - noise).double().pow(2).sum().item()
    print(f"config 3 (CFG step at N = {T * H * W // 4}): update vs reference fp32 {r_upd:.3e}, latent {r_lat:.3e}; |update|^2 {ss:.5e} / {c['update_sumsq']:.5e}")
    assert r_upd <= 3e-2, r_upd
    assert r_lat <= 3e-2, r_lat
    assert abs(ss - c["update_sumsq"]) <= 5e-2 * c["update_sumsq"]


def test_cross_attention_keys_of_all_blocks_in_one_go_same_bits():
    """"cross_kv_batched" (round 4, default 1): the cross-attention key / V^T projections of all visual blocks are two GEMMs against stacked
    weights before the visual stack (they depend on the text stream only) and their key RMSNorms one launch — same kernels, same per-element
    sums: the velocity must equal the per-block launches' bit for bit, for a 37-token and a 256-token prompt (ragged / whole key tiles)."""
    dit, _, _ = _two_block_model(1.0)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(5, 16, 16, 16, generator=g)
    pooled = torch.randn(1, 768, generator=g)
    pos = [torch.arange(5), torch.arange(8), torch.arange(8)]
    dit.engine("cuda:0")
    for L in (37, 256):
        text = torch.randn(L, 3584, generator=g)
        args = (x.cuda(), text.cuda(), pooled.cuda(), torch.tensor([625.0]), pos, torch.arange(L))
        assert dit.get_option("cross_kv_batched") == 1
        a = dit(*args, scale_factor=(1.0, 2.0, 2.0))
        dit.set_option("cross_kv_batched", 0)
        b = dit(*args, scale_factor=(1.0, 2.0, 2.0))
        dit.set_option("cross_kv_batched", 1)
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), L
