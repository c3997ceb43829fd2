"""LoRA adapters on the GPU: the merge kernel against float64, and the engine plumbing bit for bit.

Kernel (k5_lora_merge): W' = W + s * (B @ A) with a fixed fma order, one round-to-nearest-even for a bf16 destination.
  * bf16 destination: every output is one of the two bf16 neighbours of the float64 value, no NaN, and at most 1e-3 of the elements differ
    from the round-to-nearest-even of the float64 value.  (An fp32 fma chain meets the cap — an emulation of it stays at <= 2e-4 on these
    inputs — but not the neighbour condition: where W and the update cancel its error of up to R * 2^-24 * sum|B||A| spans several bf16 steps
    of the small result; 2 of 131 072 outputs of the 256 x 512, R = 128 case, s = 2, fp32 factors.  The kernel therefore sums in float64.)
  * fp32 destination: |out - exact| <= R * 2^-23 * (|W| + |s| sum|B||A|);
  * pad columns keep their bit pattern; s = 0 leaves W bit-identical.
Engine (k5_dit_add_lora / k5_dit_clear_lora / k5_dit_lora_state): handle X gets the adapters of tests/golden/lora_tiny.safetensors
(tools/gen_golden_lora.py), handle Y is loaded with a checkpoint whose matrices were merged beforehand by k5_lora_merge on torch tensors in
the packed dtype.  X and Y must agree bit for bit wherever the engine is deterministic, and differ from the un-adapted handle."""
import ctypes as C
import functools
import os
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
import kit  # noqa: E402
from kit import E, GOLDEN, POS, rel  # noqa: E402

make_dit = functools.partial(kit.make_dit, engine=True)

NPOS = [torch.arange(6), torch.arange(16), torch.arange(16)]
SF = (1.0, 2.0, 2.0)


# ------------------------------------------------------------------------------------------ 1. kernel against float64
def bf16_step(c, up):
    """the next bf16 value above (up) / below c, through the bit pattern"""
    bits = c.view(torch.int16).to(torch.int32) & 0xFFFF
    neg = bits >= 0x8000
    mag = bits & 0x7FFF
    grow = neg != up                                   # moving away from zero
    mag2 = torch.where(grow, mag + 1, mag - 1)
    sign = torch.where(neg, 0x8000, 0)
    cross = (mag == 0) & ~grow                         # +-0 stepping through zero: the smallest value of the other sign
    out = torch.where(cross, torch.where(up, 0x0001, 0x8001), sign | mag2)
    out = torch.where(out >= 0x8000, out - 0x10000, out)
    return out.to(torch.int16).view(torch.bfloat16)


def bf16_neighbours(exact):
    """(lo, hi, rne): the bf16 values around the float64 `exact` and its round-to-nearest-even"""
    c = exact.float().bfloat16()
    c64 = c.double()
    below = c64 <= exact
    lo = torch.where(below, c, bf16_step(c, torch.zeros_like(below)))
    hi = torch.where(below, bf16_step(c, torch.ones_like(below)), c)
    hi = torch.where(c64 == exact, c, hi)
    dlo, dhi = exact - lo.double(), hi.double() - exact
    even_lo = (lo.view(torch.int16).to(torch.int32) & 1) == 0
    rne = torch.where(dlo < dhi, lo, torch.where(dhi < dlo, hi, torch.where(even_lo, lo, hi)))
    return lo, hi, rne


def test_bf16_neighbour_helper():
    x = torch.tensor([1.0, 1.00390625, 1.001, -1.001, 3.0e-3, -0.0203], dtype=torch.float64)
    lo, hi, rne = bf16_neighbours(x)
    assert (lo.double() <= x).all() and (hi.double() >= x).all()
    assert lo[0] == hi[0] == 1.0 and lo[1].item() == 1.0 and hi[1].item() == 1.0078125 and rne[1].item() == 1.0   # a tie goes to even
    assert hi[3].item() == -1.0 and lo[3].item() == -1.0078125


SHAPES = [(64, 64, 64, 1, "bf16"), (65, 132, 136, 7, "bf16"), (192, 320, 320, 16, "bf16"), (256, 512, 512, 128, "bf16"),
          (64, 72, 72, 256, "bf16"), (96, 64, 64, 4, "f32")]
PAD_BITS = 0x5A5B


@pytest.mark.parametrize("rows,cols,ld,R,dst", SHAPES)
def test_merge_kernel_against_float64(E, rows, cols, ld, R, dst):
    g = torch.Generator().manual_seed(rows * 1000 + cols + R)
    W0 = torch.randn(rows, cols, generator=g) * 0.02
    A0, B0 = torch.randn(R, cols, generator=g) * 0.05, torch.randn(rows, R, generator=g) * 0.05
    wdt = torch.bfloat16 if dst == "bf16" else torch.float32
    W0 = W0.to(wdt)
    worst = 0.0
    for fdt in (torch.float32, torch.bfloat16, torch.float16):
        A, B = A0.to(fdt), B0.to(fdt)
        prod = B.double() @ A.double()
        mag = B.double().abs() @ A.double().abs()
        for s in (1.0, -0.5, 2.0):
            buf = torch.empty(rows, ld, dtype=wdt)
            if ld > cols:
                buf.view(torch.int16 if dst == "bf16" else torch.int32)[:] = PAD_BITS
            buf[:, :cols] = W0
            dev = buf.cuda()
            E.lora_merge_(dev, A.cuda(), B.cuda(), s, cols=cols)
            torch.cuda.synchronize()
            got = dev.cpu()
            if ld > cols:
                assert (got[:, cols:].view(torch.int16) == PAD_BITS).all() if dst == "bf16" else (got[:, cols:].view(torch.int32) == PAD_BITS).all()
            out = got[:, :cols]
            assert not torch.isnan(out.float()).any()
            exact = W0.double() + s * prod
            if dst == "bf16":
                lo, hi, rne = bf16_neighbours(exact)
                ok = (out == lo) | (out == hi)
                assert ok.all(), f"{(~ok).sum().item()} outputs are not a bf16 neighbour of the exact value ({fdt}, s = {s})"
                frac = (out != rne).float().mean().item()
                worst = max(worst, frac)
                assert frac <= 1e-3, f"{frac:.2e} of the elements differ from the RNE of the exact value ({fdt}, s = {s})"
            else:
                bound = R * 2.0 ** -23 * (W0.double().abs() + abs(s) * mag)
                err = (out.double() - exact).abs()
                assert (err <= bound).all(), f"max err/bound {(err / bound).max().item():.3f} ({fdt}, s = {s})"
                worst = max(worst, (err / bound).max().item())
        # s = 0: nothing launched, W bit-identical
        dev = W0.cuda()
        E.lora_merge_(dev, A.cuda(), B.cuda(), 0.0)
        torch.cuda.synchronize()
        assert torch.equal(dev.cpu().view(torch.int16 if dst == "bf16" else torch.int32), W0.view(torch.int16 if dst == "bf16" else torch.int32))
    print(f"({rows}, {cols}, {ld}, R = {R}, {dst}): worst " + (f"fraction off RNE {worst:.2e}" if dst == "bf16" else f"err / bound {worst:.3f}"))


def test_merge_kernel_refuses_bad_arguments(E):
    W = torch.zeros(64, 64, dtype=torch.bfloat16, device="cuda")
    A, B = torch.zeros(4, 64, device="cuda"), torch.zeros(64, 4, device="cuda")
    L = E.lib()
    for args in ((W.data_ptr(), 1, 64, 64, 64, A.data_ptr(), 0, B.data_ptr(), 0, 0, 1.0, None),      # R = 0
                 (W.data_ptr(), 1, 64, 64, 64, A.data_ptr(), 0, B.data_ptr(), 0, 257, 1.0, None),    # R = 257
                 (W.data_ptr(), 2, 64, 64, 64, A.data_ptr(), 0, B.data_ptr(), 0, 4, 1.0, None),      # f16 destination
                 (W.data_ptr(), 1, 64, 64, 32, A.data_ptr(), 0, B.data_ptr(), 0, 4, 1.0, None),      # ld < cols
                 (W.data_ptr(), 1, 64, 64, 64, None, 0, B.data_ptr(), 0, 4, 1.0, None),
                 (W.data_ptr(), 1, 64, 64, 64, A.data_ptr(), 5, B.data_ptr(), 0, 4, 1.0, None)):
        assert L.k5_lora_merge(*args) == 1 and E.last_error()
    torch.cuda.synchronize()
    assert not W.float().any()


# ------------------------------------------------------------------------------------------ engine: shared handles and runs
F32_KEYS = ("time_embeddings.", "modulation.out_layer.")


def packed_dtype(key):
    return torch.float32 if any(p in key for p in F32_KEYS) else torch.bfloat16


def merged_on_gpu(E, sd, adapters):
    """the checkpoint with every adapter of `adapters` ([(entries, strength)], in order) merged beforehand by k5_lora_merge on torch tensors in
    the packed dtype of the key: what handle Y is loaded with"""
    from kandinsky.lora import lora_scale
    out = dict(sd)
    for entries, strength in adapters:
        for key, (A, B, alpha) in entries.items():
            W = out[key].cuda().to(packed_dtype(key)).contiguous()
            E.lora_merge_(W, A.cuda().contiguous(), B.cuda().contiguous(), lora_scale(strength, alpha, A.shape[0]))
            out[key] = W.float().cpu()
    torch.cuda.synchronize()
    return out


def sigmas(steps, scale=5.0):
    t = torch.linspace(1, 0, steps + 1)
    return (scale * t / (1 + (scale - 1) * t)).tolist()


def forward_dense(d, golden):
    return d(golden["fwd.x"].cuda(), golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), golden["fwd.time"], POS, torch.arange(7),
             scale_factor=SF)


def forward_nabla(d, golden, golden_meta):
    at = golden_meta["nabla_attention"]
    sparse = {"P": at["P"], "wT": at["wT"], "wH": at["wH"], "wW": at["wW"], "to_fractal": True}
    return d(golden["nabla.fwd.x"].cuda(), golden["fwd.text"].cuda(), golden["fwd.pooled"].cuda(), golden["fwd.time"], NPOS, torch.arange(7),
             scale_factor=SF, sparse_params=sparse)


def sample(d, golden, w, graph=False, steps=4):
    te = {"text_embeds": golden["fwd.text"].cuda(), "pooled_embed": golden["fwd.pooled"].cuda()}
    ne = {"text_embeds": golden["gen.null_text"].cuda(), "pooled_embed": golden["gen.null_pooled"].cuda()}
    d.set_graph(graph)
    lat = golden["gen.noise"].clone().cuda()
    d.sample(lat, sigmas(steps), te, ne, POS, torch.arange(7), torch.arange(4), w, scale_factor=SF)
    torch.cuda.synchronize()
    d.set_graph(False)
    return lat


def all_runs(d, golden, golden_meta):
    out = {"dense": forward_dense(d, golden), "nabla": forward_nabla(d, golden, golden_meta)}
    for w in (1.0, 5.0):
        out[f"sample w={w}"] = sample(d, golden, w)
        out[f"sample w={w} graph"] = sample(d, golden, w, graph=True)
    return out


@pytest.fixture(scope="module")
def cfg(golden_meta):
    return dict(golden_meta["tiny_config"])


@pytest.fixture(scope="module")
def entries(tiny_sd):
    from kandinsky.lora import load_lora
    return load_lora(os.path.join(GOLDEN, "lora_tiny.safetensors"), known_keys=tiny_sd.keys())


@pytest.fixture(scope="module")
def base(E, cfg, tiny_sd, golden, golden_meta):
    """the un-adapted handle and its runs (computed once, never changed)"""
    d = make_dit(cfg, tiny_sd)
    return d, all_runs(d, golden, golden_meta)


@pytest.fixture(scope="module")
def y_runs(E, cfg, tiny_sd, entries, golden, golden_meta):
    return all_runs(make_dit(cfg, merged_on_gpu(E, tiny_sd, [(entries, 1.0)])), golden, golden_meta)


def lora_state(E, d):
    n, b = C.c_int(-1), C.c_longlong(-1)
    E.check(E.lib().k5_dit_lora_state(d._handle, C.byref(n), C.byref(b)))
    return n.value, b.value


# ------------------------------------------------------------------------------------------ 2. plumbing, bit for bit  + 3. undo
def test_adapted_handle_equals_premerged_checkpoint_and_undo(E, cfg, tiny_sd, entries, base, y_runs, golden, golden_meta):
    kinds = {packed_dtype(k) for k in entries}
    assert kinds == {torch.float32, torch.bfloat16} and len({v[0].shape[0] for v in entries.values()}) >= 6   # both islands, differing R
    _, base_runs = base
    x = make_dit(cfg, tiny_sd)
    assert lora_state(E, x) == (0, 0)
    x.add_lora(entries)
    n, nbytes = lora_state(E, x)
    D, TD = cfg["model_dim"], cfg["time_dim"]
    Kvis = 4 * (2 * cfg["in_visual_dim"] + 1)
    want = 0
    for k in entries:
        r, c = tiny_sd[k].shape
        want += r * ((c + 7) // 8 * 8 if k.startswith("visual_embeddings") else c) * (4 if packed_dtype(k) == torch.float32 else 2)
    assert Kvis == 132 and n == len(entries) and nbytes == want, (n, nbytes, want)
    x_runs = all_runs(x, golden, golden_meta)
    for name in y_runs:
        assert torch.isfinite(x_runs[name].float()).all(), name
        assert torch.equal(x_runs[name], y_runs[name]), f"{name}: adapted handle vs pre-merged checkpoint, rel {rel(x_runs[name], y_runs[name]):.3e}"
        assert rel(x_runs[name], base_runs[name]) > 1e-3, f"{name}: the adapter changed nothing"
    # undo: the un-adapted bits, nothing kept
    x.clear_lora()
    assert lora_state(E, x) == (0, 0) and x.lora_state() == {"adapters": 0, "matrices": 0, "backup_bytes": 0}
    for name, ref in all_runs(x, golden, golden_meta).items():
        assert torch.equal(ref, base_runs[name]), f"{name} after clear_lora"
    # add, clear, add again == a single add
    x.add_lora(entries)
    assert torch.equal(forward_dense(x, golden), y_runs["dense"]) and torch.equal(sample(x, golden, 5.0), y_runs["sample w=5.0"])
    x.clear_lora()
    # two adapters on the same keys == two sequential merges (one rounding per call, in call order)
    x.add_lora(entries, strength=0.5)
    x.add_lora(entries, strength=-1.25)
    assert lora_state(E, x)[0] == len(entries)
    y2 = make_dit(cfg, merged_on_gpu(E, tiny_sd, [(entries, 0.5), (entries, -1.25)]))
    assert torch.equal(forward_dense(x, golden), forward_dense(y2, golden))
    assert torch.equal(sample(x, golden, 5.0), sample(y2, golden, 5.0))
    x.clear_lora()
    assert torch.equal(forward_dense(x, golden), base_runs["dense"])


# ------------------------------------------------------------------------------------------ 4. caches
def test_caches_are_dropped(E, cfg, tiny_sd, entries, base, golden):
    key = "text_transformer_blocks.0.self_attention.to_query.weight"
    one = {key: entries[key], "text_embeddings.in_layer.weight": entries["text_embeddings.in_layer.weight"]}
    y = make_dit(cfg, merged_on_gpu(E, tiny_sd, [(one, 1.0)]))
    y_fwd, y_lat = forward_dense(y, golden), sample(y, golden, 5.0, steps=3)
    z = make_dit(cfg, tiny_sd)
    assert torch.equal(forward_dense(z, golden), base[1]["dense"])
    sample(z, golden, 5.0, steps=3)                       # fills the text prologue cache of both branches
    z.add_lora(one)
    assert torch.equal(forward_dense(z, golden), y_fwd)   # the stepwise path
    assert torch.equal(sample(z, golden, 5.0, steps=3), y_lat)
    assert rel(y_fwd, base[1]["dense"]) > 1e-4
    # MagCache: the call counter goes back to 0
    table = (C.c_double * 8)(*[1.0] * 8)
    E.check(E.lib().k5_dit_set_magcache(z._handle, table, 8, 0, 0.12, 2, 0.2))
    forward_dense(z, golden)
    cnt = C.c_int(-1)
    E.check(E.lib().k5_dit_magcache_state(z._handle, C.byref(cnt), None, None))
    assert cnt.value == 1
    z.add_lora(one, strength=0.5)
    E.check(E.lib().k5_dit_magcache_state(z._handle, C.byref(cnt), None, None))
    assert cnt.value == 0
    forward_dense(z, golden)
    z.clear_lora()
    E.check(E.lib().k5_dit_magcache_state(z._handle, C.byref(cnt), None, None))
    assert cnt.value == 0
    E.check(E.lib().k5_dit_set_magcache(z._handle, None, 0, 0, 0.12, 2, 0.2))
    assert torch.equal(forward_dense(z, golden), base[1]["dense"])


# ------------------------------------------------------------------------------------------ 5. fp8
def test_fp8_copies_follow_the_adapter(E, cfg):
    """model_dim 256 / ff_dim 512: the smallest width k5_dit_set_fp8 takes; 256 tokens so that the e4m3 GEMMs really run."""
    c = dict(cfg, model_dim=256, ff_dim=512)
    ocfg = O.DitConfig(**dict(c, patch_size=tuple(c["patch_size"]), axes_dims=tuple(c["axes_dims"])))
    sd = O.synthetic_state_dict(ocfg, seed=5)
    g = torch.Generator().manual_seed(77)
    ent = {}
    for i, m in enumerate(("visual_transformer_blocks.0.feed_forward.in_layer", "visual_transformer_blocks.1.feed_forward.out_layer",
                           "visual_transformer_blocks.0.self_attention.to_query", "visual_transformer_blocks.1.self_attention.to_key",
                           "visual_transformer_blocks.1.self_attention.to_value", "visual_transformer_blocks.0.self_attention.out_layer",
                           "visual_transformer_blocks.0.cross_attention.to_key", "text_transformer_blocks.0.feed_forward.in_layer")):
        rows, cols = sd[m + ".weight"].shape
        R = 2 + 3 * i
        ent[m + ".weight"] = (torch.randn(R, cols, generator=g) * 0.05, (torch.randn(rows, R, generator=g) * 0.05).bfloat16(), None)
    x_in = torch.randn(4, 16, 16, 33, generator=g)
    text, pooled = torch.randn(9, c["in_text_dim"], generator=g), torch.randn(1, c["in_text_dim2"], generator=g)
    pos = [torch.arange(4), torch.arange(8), torch.arange(8)]

    def fwd(d):
        return d(x_in.cuda(), text.cuda(), pooled.cuda(), torch.tensor([600.0]), pos, torch.arange(9), scale_factor=SF)

    x = make_dit(c, sd)
    bf16_plain = fwd(x)
    x.set_fp8(7)
    fp8_plain = fwd(x)
    assert not torch.equal(fp8_plain, bf16_plain)        # the e4m3 path is really on
    x.add_lora(ent)
    y = make_dit(c, merged_on_gpu(E, sd, [(ent, 1.0)]))
    y.set_fp8(7)
    fx, fy = fwd(x), fwd(y)
    assert torch.isfinite(fx.float()).all() and torch.equal(fx, fy), rel(fx, fy)
    assert rel(fx, fp8_plain) > 1e-3
    x.clear_lora()
    assert torch.equal(fwd(x), fp8_plain)
    x.set_fp8(0)
    assert torch.equal(fwd(x), bf16_plain)


# ------------------------------------------------------------------------------------------ 6. ranks
@pytest.mark.timeout(600)
def test_two_loopback_ranks_add_the_adapters(E, cfg, tiny_sd, entries):
    from test_gpu_loopback import run_ranks
    g = torch.Generator().manual_seed(108)
    x_in = torch.randn(8, 16, 16, 33, generator=g)
    text, pooled = torch.randn(9, 96, generator=g), torch.randn(1, 48, generator=g)
    pos = [torch.arange(8), torch.arange(8), torch.arange(8)]
    gate = threading.Barrier(2)

    def fwd(d):
        return d(x_in.cuda(), text.cuda(), pooled.cuda(), torch.tensor([432.0]), pos, torch.arange(9), scale_factor=SF)

    def adapted(d, r):                                    # a handle that already sits in the group takes the adapters
        d.add_lora(entries)
        gate.wait(120)
        return fwd(d)

    merged = merged_on_gpu(E, tiny_sd, [(entries, 1.0)])
    xs = run_ranks(2, lambda: make_dit(cfg, tiny_sd), adapted)
    ys = run_ranks(2, lambda: make_dit(cfg, merged), lambda d, r: fwd(d))
    plain = run_ranks(2, lambda: make_dit(cfg, tiny_sd), lambda d, r: fwd(d))
    assert torch.isfinite(xs[0].float()).all()
    for r in range(2):
        assert torch.equal(xs[r], ys[r]), f"rank {r}: {rel(xs[r], ys[r]):.3e}"
    assert torch.equal(xs[0], xs[1]) and rel(xs[0], plain[0]) > 1e-3


# ------------------------------------------------------------------------------------------ 7. parity with the CPU oracle
def test_adapted_generate_vs_oracle_on_host_merged_weights(E, cfg, tiny_sd, entries, golden):
    """the oracle, unchanged, fed a state dict merged on the host in float64; tolerance of tests/test_gpu_dit.py::test_generate_trajectory
    for the engine against the bf16-island oracle on a final latent: relative L2 <= 1e-2"""
    from types import SimpleNamespace as NS
    from kandinsky.generation_utils import generate
    from kandinsky.lora import lora_scale
    sd64 = dict(tiny_sd)
    for k, (A, B, alpha) in entries.items():
        sd64[k] = (tiny_sd[k].double() + lora_scale(1.0, alpha, A.shape[0]) * (B.double() @ A.double())).float()
    steps, s, w = 4, 5.0, 5.0
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=SF))
    te = {"text_embeds": golden["fwd.text"].cuda(), "pooled_embed": golden["fwd.pooled"].cuda()}
    ne = {"text_embeds": golden["gen.null_text"].cuda(), "pooled_embed": golden["gen.null_pooled"].cuda()}
    x = make_dit(cfg, tiny_sd)
    x.add_lora(entries)
    out = generate(x, "cuda:0", (3, 8, 12, 16), steps, te, ne, POS, torch.arange(7), torch.arange(4), w, s, conf, noise=golden["gen.noise"])
    ocfg = O.DitConfig(**dict(cfg, patch_size=tuple(cfg["patch_size"]), axes_dims=tuple(cfg["axes_dims"])))
    tec, nec = {k: v.cpu() for k, v in te.items()}, {k: v.cpu() for k, v in ne.items()}
    ref = O.generate(sd64, ocfg, golden["gen.noise"], steps, tec, nec, POS, torch.arange(7), torch.arange(4), w, s, SF, None, "bf16")
    plain = O.generate(tiny_sd, ocfg, golden["gen.noise"], steps, tec, nec, POS, torch.arange(7), torch.arange(4), w, s, SF, None, "bf16")
    print(f"adapted engine vs oracle on float64-merged weights {rel(out, ref):.3e}; the adapter moved the oracle's latent by {rel(ref, plain):.3e}")
    assert rel(out, ref) <= 1e-2, rel(out, ref)
    assert rel(ref, plain) > 1e-3                          # ... and the comparison is not adapter-blind


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handle_alone(E, cfg, tiny_sd, base, golden):
    L = E.lib()
    A, B = torch.zeros(4, 128, device="cuda") + 0.1, torch.zeros(128, 4, device="cuda") + 0.1
    key = b"visual_transformer_blocks.0.self_attention.to_query.weight"
    d = make_dit(cfg, tiny_sd)
    h = d._handle

    def refused(status, *args):
        got = L.k5_dit_add_lora(*args)
        assert got == status and E.last_error(), (got, status, E.last_error())

    raw = d._create_handle()                               # created, nothing loaded, not finalized
    refused(4, raw, key, A.data_ptr(), 0, B.data_ptr(), 0, 4, 1.0)
    assert L.k5_dit_clear_lora(raw) == 4 and E.last_error()
    L.k5_dit_destroy(raw)
    refused(5, h, b"visual_transformer_blocks.0.self_attention.to_gate.weight", A.data_ptr(), 0, B.data_ptr(), 0, 4, 1.0)
    refused(5, h, b"visual_transformer_blocks.9.self_attention.to_query.weight", A.data_ptr(), 0, B.data_ptr(), 0, 4, 1.0)
    refused(6, h, b"visual_transformer_blocks.0.self_attention.to_query.bias", A.data_ptr(), 0, B.data_ptr(), 0, 4, 1.0)
    refused(6, h, b"visual_transformer_blocks.0.self_attention.query_norm.weight", A.data_ptr(), 0, B.data_ptr(), 0, 4, 1.0)
    refused(6, h, b"text_embeddings.norm.weight", A.data_ptr(), 0, B.data_ptr(), 0, 4, 1.0)
    refused(1, h, key, A.data_ptr(), 0, B.data_ptr(), 0, 0, 1.0)
    refused(1, h, key, A.data_ptr(), 0, B.data_ptr(), 0, 257, 1.0)
    refused(1, h, key, A.data_ptr(), 3, B.data_ptr(), 0, 4, 1.0)
    refused(1, h, key, A.data_ptr(), 0, B.data_ptr(), -1, 4, 1.0)
    refused(1, h, key, None, 0, B.data_ptr(), 0, 4, 1.0)
    refused(1, h, key, A.data_ptr(), 0, None, 0, 4, 1.0)
    refused(1, h, None, A.data_ptr(), 0, B.data_ptr(), 0, 4, 1.0)
    assert lora_state(E, d) == (0, 0)
    assert torch.equal(forward_dense(d, golden), base[1]["dense"])
    # the Python surface refuses what does not fit before anything reaches the engine
    with pytest.raises(ValueError, match="do not fit"):
        d.add_lora({key.decode(): (torch.zeros(4, 64), torch.zeros(128, 4), None)})
    with pytest.raises(KeyError, match="to_gate"):
        d.add_lora({"transformer.visual_transformer_blocks.0.self_attention.to_gate.lora_A.weight": torch.zeros(4, 128)})
    assert torch.equal(forward_dense(d, golden), base[1]["dense"])
