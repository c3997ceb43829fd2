"""FlowEdit on the MI355X: the pass of k5_flowedit_step bit for bit against separate fp32 / bf16 ops in torch eager (tests/flowedit_reference.py)
over its forms, sizes and access paths; k5_sample_flowedit against the per-step loop of `generate` bit for bit, its counters, its exact
properties (equal prompts return the source, kept cells are the source, a seed repeats), the watch, what it leaves on the handle, every
refusal; and parity with the reference's fp32 golden on the edit (tools/gen_golden_flowedit.py).

The model, shape, steps and prompts are those of tests/test_gpu_stochastic.py; the source prompt and latent are flowedit_reference's seeded
draws.  Everything that claims "the same computation" is asserted bit for bit.  Parity is measured on the EDIT,
|(out - src) - (gold - src)| / |gold - src|: the source dominates the full latent and would hide an error.  The engine is held to 1.5 x the
distance of the bf16 oracle loop from the golden that the generator recorded (the forecast cache's margin: the engine's rounding points are
the oracle's, its reduction orders are not)."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import flowedit_reference as FR  # noqa: E402
import kit  # noqa: E402
from kit import BF, GOLDEN, K5_ERR_ARG, K5_ERR_STATE, POS, cfg, flash_conf, make_dit, need_gpu, rel, tiny_dit  # noqa: E402

FLASH = flash_conf()
SHAPE = (3, 8, 12, 16)
STEPS = 6
STRENGTH = 0.7            # first = 2: four of the six steps run
SEED = 6554
CASES = {"g1_1": (1.0, 1.0), "g2_5": (2.0, 5.0), "g1_5": (1.0, 5.0)}      # (source weight, target weight)
FORWARDS = {"g1_1": 2, "g2_5": 4, "g1_5": 3}
PROMPTS = {"g1_1": 2, "g2_5": 3, "g1_5": 3}                               # distinct prompts of a call
GRID_TRIP = 2048 * 256 * 4                                                 # elements of one trip of the launcher's capped grid


# ------------------------------------------------------------------------------------------ the kernel
PAD = 16


class Buffers:
    """The streams of one launch over `dims` (..., C), each inside a poisoned allocation `off` elements in (fp32: 4 off bytes, bf16: 2 off
    bytes), so that a write past n or in front of the base shows"""

    def __init__(self, dims, seed, off32=0, off16=0):
        g = torch.Generator().manual_seed(seed)
        self.dims, self.n = dims, int(torch.tensor(dims).prod())
        self.host, self.raw = {}, {}
        self.off = {}
        for name in ("z_fe", "x_src", "z", "zs", "zt"):
            self._put(name, torch.randn(self.n, generator=g) * (0.0 if name in ("zs", "zt") else 1.5), off32, 7.0)
        for name in ("cs", "us", "ct", "ut"):
            self._put(name, torch.randn(self.n, generator=g).to(BF), off16, 7.0)
        cells = self.n // dims[-1]
        m = (torch.rand(cells, generator=g) * 3).floor() / 2.0               # 0, 0.5 or 1 per cell
        self._put("hard", (m == 1.0).float(), 0, 7.0)
        self._put("frac", m, 0, 7.0)

    def _put(self, name, t, off, poison):
        raw = torch.full((t.numel() + off + PAD,), poison, dtype=t.dtype)
        raw[off:off + t.numel()] = t
        self.host[name], self.raw[name], self.off[name] = t.clone(), raw.cuda(), off

    def dev(self, name):
        t = self.raw[name][self.off[name]:self.off[name] + self.host[name].numel()]
        return t.view(*self.dims[:-1], -1) if name in ("hard", "frac") else t.view(self.dims)

    def cpu(self, name):
        t = self.host[name]
        return t.view(*self.dims[:-1], -1) if name in ("hard", "frac") else t.view(self.dims)

    def untouched_outside(self, names=("z_fe", "zs", "zt")):
        for name in names:
            raw, off, n = self.raw[name].cpu(), self.off[name], self.host[name].numel()
            if not ((raw[:off] == 7.0).all() and (raw[off + n:] == 7.0).all()):
                return False
        return True


def launch(b, form, w_src=2.0, w_tar=5.0, mask=None, z="given", dt=-0.0625, sigma=0.75, seed=SEED, stream=3, poison=()):
    """One E.flowedit_step_ on fresh copies of b's streams; returns (z_fe, zs, zt) on the host.  form: "prepare", "update" or "both"."""
    from kandinsky import _engine as E
    for name in ("z_fe", "zs", "zt"):   # every launch starts from the same state
        b.raw[name][b.off[name]:b.off[name] + b.n] = b.host[name].cuda()
    for name in poison:
        b.raw[name][b.off[name]:b.off[name] + b.host[name].numel()] = float("nan")
    kw = {}
    if form != "prepare":
        kw.update(c_src=b.dev("cs"), c_tar=b.dev("ct"))
    if form != "prepare" or poison:    # a prepare-only launch is one without c_*: what else it is handed must not be read
        kw.update(u_src=b.dev("us") if w_src != 1.0 or "us" in poison else None, u_tar=b.dev("ut") if w_tar != 1.0 or "ut" in poison else None,
                  w_src=w_src, w_tar=w_tar, dt=dt, keep_mask=None if mask is None else b.dev(mask))
    if form != "update":
        kw.update(sigma_next=sigma, zs=b.dev("zs"), zt=b.dev("zt"), seed=seed, stream_id=stream, z=b.dev("z") if z == "given" else None)
    E.flowedit_step_(b.dev("z_fe"), b.dev("x_src"), **kw)
    torch.cuda.synchronize()
    for name in poison:
        b.raw[name][b.off[name]:b.off[name] + b.host[name].numel()] = b.host[name].cuda()
    return tuple(b.dev(k).cpu().clone() for k in ("z_fe", "zs", "zt"))


def want(b, form, w_src=2.0, w_tar=5.0, mask=None, z=None, dt=-0.0625, sigma=0.75):
    vel = None if form == "prepare" else (b.cpu("cs"), b.cpu("us") if w_src != 1.0 else None, b.cpu("ct"), b.cpu("ut") if w_tar != 1.0 else None)
    z_fe, zs, zt = FR.flowedit_pass(b.cpu("z_fe").clone(), b.cpu("x_src"), vel, w_src=w_src, w_tar=w_tar, dt=dt,
                                    keep_mask=None if mask is None else b.cpu(mask), sigma_next=None if form == "update" else sigma,
                                    z=b.cpu("z") if z is None else z)
    return z_fe, b.cpu("zs") if zs is None else zs, b.cpu("zt") if zt is None else zt


def same(got, exp):
    return all(torch.equal(g, e) for g, e in zip(got, exp))


LAYOUTS = [((3, 8, 12, 16), 0, 0), ((5, 10, 14, 16), 0, 0),       # n % 4 == 0, aligned bases: 16-byte / 8-byte accesses
           ((7, 3), 0, 0), ((5, 3), 0, 0),                        # n = 21, 15: n % 4 = 1, 3 — a partial generator block, element by element
           ((3, 8, 12, 16), 1, 2), ((5, 10, 14, 16), 1, 0), ((3, 8, 12, 16), 0, 2)]   # bases 4 bytes off: element by element


@pytest.fixture(scope="module", params=LAYOUTS, ids=lambda p: "x".join(map(str, p[0])) + f"+{p[1]}+{p[2]}")
def bufs(request):
    need_gpu()
    dims, o32, o16 = request.param
    return Buffers(dims, 100 + len(dims) + o32 + 2 * o16, o32, o16)


def test_forms_weights_and_masks_bit_for_bit(bufs):
    b = bufs
    for form in ("prepare", "update", "both"):
        for w_src, w_tar in ((2.0, 5.0), (1.0, 5.0), (3.5, 1.0), (1.0, 1.0)):
            for mask in (None, "hard", "frac"):
                if form == "prepare" and (mask or (w_src, w_tar) != (2.0, 5.0)):
                    continue
                got = launch(b, form, w_src, w_tar, mask)
                assert same(got, want(b, form, w_src, w_tar, mask)), (form, w_src, w_tar, mask)
                assert b.untouched_outside(), (form, w_src, w_tar, mask)
                if form == "update":                                       # zs / zt are not written without a next sigma
                    assert torch.equal(got[1], b.cpu("zs")) and torch.equal(got[2], b.cpu("zt"))
                if form == "prepare":                                      # z_fe is not written without velocities, and zt == zs + (z_fe - x_src)
                    assert torch.equal(got[0], b.cpu("z_fe"))
                if mask and form != "prepare":
                    kept = (b.cpu(mask) == 1.0).expand_as(got[0])
                    assert torch.equal(got[0][kept], b.cpu("z_fe")[kept])  # m == 1 leaves z_fe as it was


def test_the_generator_inside_equals_the_noise_handed_in(bufs):
    from kandinsky import _engine as E
    b = bufs
    zg = torch.empty(b.n, device="cuda")
    E.noise_normal_(zg, SEED + 1, 5)
    for form in ("prepare", "both"):
        inside = launch(b, form, z="inside", seed=SEED + 1, stream=5)
        assert same(inside, want(b, form, z=zg.cpu().view(b.dims))), form
        assert b.untouched_outside()
        assert not torch.equal(inside[1], launch(b, form, z="inside", seed=SEED + 1, stream=6)[1])
        assert not torch.equal(inside[1], launch(b, form, z="inside", seed=SEED + 2, stream=5)[1])


def test_equal_velocities_and_an_unmoved_latent(bufs):
    from kandinsky import _engine as E
    b = bufs
    for name in ("z_fe", "zs", "zt"):
        b.raw[name][b.off[name]:b.off[name] + b.n] = b.host[name].cuda()
    # v_t == v_s: z_fe is the input, bit for bit
    E.flowedit_step_(b.dev("z_fe"), b.dev("x_src"), b.dev("cs"), b.dev("us"), b.dev("cs"), b.dev("us"), w_src=5.0, w_tar=5.0, dt=-0.25)
    torch.cuda.synchronize()
    assert torch.equal(b.dev("z_fe").cpu(), b.cpu("z_fe"))
    # z_fe == x_src: zt == zs, bit for bit
    E.flowedit_step_(b.dev("x_src").clone(), b.dev("x_src"), sigma_next=0.6, zs=b.dev("zs"), zt=b.dev("zt"), seed=3, stream_id=1)
    torch.cuda.synchronize()
    assert torch.equal(b.dev("zs"), b.dev("zt")) and b.untouched_outside()


def test_poison_in_what_must_not_be_read_stays_out(bufs):
    b = bufs
    got = launch(b, "prepare", mask="hard", poison=("us", "ut", "hard"))    # a prepare-only launch: what it is handed besides (c_* select the form)
    assert same(got, want(b, "prepare")) and all(torch.isfinite(t).all() for t in got)
    for w_src, w_tar, poison in ((1.0, 5.0, ("us",)), (3.5, 1.0, ("ut",)), (1.0, 1.0, ("us", "ut"))):                # u_* at weight 1
        got = launch(b, "both", w_src, w_tar, poison=poison)
        assert same(got, want(b, "both", w_src, w_tar)), (w_src, w_tar)
        assert all(torch.isfinite(t).all() for t in got)


def test_the_stride_loop_wraps_past_the_grid_cap():
    need_gpu()
    n = GRID_TRIP + 4 * 256 * 3 + 8                                         # a second, partial trip
    b = Buffers((n // 8, 8), 9)
    for form, z in (("both", "given"), ("both", "inside"), ("update", "given")):
        got = launch(b, form, mask="frac", z=z, seed=SEED, stream=2)
        zz = None
        if z == "inside":
            from kandinsky import _engine as E
            zg = torch.empty(n, device="cuda")
            E.noise_normal_(zg, SEED, 2)
            zz = zg.cpu().view(b.dims)
        assert same(got, want(b, form, mask="frac", z=zz)), (form, z)
        assert b.untouched_outside()


def test_every_refusal_launches_nothing():
    import ctypes as C
    from kandinsky import _engine as E
    need_gpu()
    b = Buffers((4, 6, 16), 21)
    p = {k: b.dev(k).data_ptr() for k in ("z_fe", "x_src", "cs", "us", "ct", "ut", "zs", "zt", "z", "frac")}

    def args(**kw):
        a = dict(z_fe=p["z_fe"], x_src=p["x_src"], c_src=p["cs"], u_src=p["us"], c_tar=p["ct"], u_tar=p["ut"], w_src=2.0, w_tar=5.0, dt=-0.1,
                 keep_mask=p["frac"], prepare=1, sigma_next=0.5, zs=p["zs"], zt=p["zt"], znoise=p["z"], seed=1, stream_id=0, cells=24, C=16)
        a.update(kw)
        return E.FlowEditStep(**a)

    bad = [dict(z_fe=None), dict(x_src=None), dict(c_src=None), dict(c_tar=None), dict(c_src=None, c_tar=None, prepare=0), dict(u_src=None),
           dict(u_tar=None), dict(zs=None), dict(zt=None), dict(cells=0), dict(C=0), dict(cells=-3), dict(z_fe=p["z_fe"] + 2),
           dict(c_src=p["cs"] + 2), dict(keep_mask=p["frac"] + 1), dict(zt=p["zt"] + 2), dict(znoise=p["z"] + 2)]
    for kw in bad:
        assert E.lib().k5_flowedit_step(C.byref(args(**kw)), E.stream_ptr()) == 1, kw
        assert b"k5_flowedit_step" in E.lib().k5_last_error()
    assert E.lib().k5_flowedit_step(None, E.stream_ptr()) == 1
    torch.cuda.synchronize()
    for name in ("z_fe", "zs", "zt"):
        assert torch.equal(b.dev(name).cpu(), b.cpu(name)), name
    assert b.untouched_outside()
    assert E.lib().k5_flowedit_step(C.byref(args()), E.stream_ptr()) == 0   # and the arguments they were derived from are good


# ------------------------------------------------------------------------------------------ the engine


Wrapped = functools.partial(kit.Wrapped, blocks=True)


def prompts(golden):
    """the kit's two prompts and the source clip's"""
    return (*kit.prompts(golden), {k: v.cuda() for k, v in FR.source_prompt(golden).items()})


def run_generate(model, golden, w=5.0, steps=STEPS, **kw):
    return kit.run_generate(model, golden, w, steps=steps, shape=SHAPE, pos=POS, **kw)


def run_flowedit(model, golden, name="g2_5", source=None, **kw):
    w_src, w_tar = CASES[name]
    _, _, se = prompts(golden)
    kw.setdefault("strength", STRENGTH)
    kw.setdefault("flowedit_seed", SEED)
    kw.setdefault("source_text_embeds", se)
    kw.setdefault("source_text_rope_pos", torch.arange(FR.SOURCE_TEXT_LEN))
    return run_generate(model, golden, w_tar, init_latent=FR.source_latent(SHAPE) if source is None else source, source_guidance_weight=w_src, **kw)


def hard_mask():
    m = torch.zeros(*SHAPE[:-1], 1)
    m[0] = 1.0
    m[1:, :, :SHAPE[2] // 2] = 1.0
    return m


def cond_kw():
    g = torch.Generator().manual_seed(11)
    vc, vm = torch.zeros(SHAPE), torch.zeros(*SHAPE[:-1], 1)
    vc[0], vm[0] = torch.randn(SHAPE[1:], generator=g), 1.0
    return dict(visual_cond=vc, visual_cond_mask=vm)


@pytest.fixture(scope="module")
def fused_runs(tiny_dit, golden):
    """the three guidance cases through the one engine call with their counters, each computed once and left unchanged"""
    out = {}
    for name in CASES:
        tiny_dit.flowedit_state(reset=True)
        lat = run_flowedit(tiny_dit, golden, name)
        out[name] = (lat, tiny_dit.flowedit_state(reset=True))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_stepwise_and_counts(tiny_dit, golden, fused_runs, name):
    lat, (steps, forwards, prologues) = fused_runs[name]
    assert torch.isfinite(lat).all()
    assert torch.equal(lat, run_flowedit(Wrapped(tiny_dit), golden, name))
    assert (steps, forwards, prologues) == (4, 4 * FORWARDS[name], PROMPTS[name])
    assert rel(lat, FR.source_latent(SHAPE)) > 1e-2                      # an edit happened


@pytest.mark.parametrize("variant", ["mask", "refine", "visual_cond", "full_strength"])
def test_fused_equals_stepwise_variants(tiny_dit, golden, fused_runs, variant):
    kw = {"mask": dict(keep_mask=hard_mask()), "refine": dict(flowedit_refine=2), "visual_cond": cond_kw(), "full_strength": dict(strength=1.0)}[variant]
    tiny_dit.flowedit_state(reset=True)
    a = run_flowedit(tiny_dit, golden, "g2_5", **kw)
    state = tiny_dit.flowedit_state(reset=True)
    assert torch.equal(a, run_flowedit(Wrapped(tiny_dit), golden, "g2_5", **kw))
    assert not torch.equal(a, fused_runs["g2_5"][0])
    # the step count does not change the prologues: three distinct prompts
    assert state == {"mask": (4, 16, 3), "refine": (2, 2 * 4 + 2 * 2, 3), "visual_cond": (4, 16, 3), "full_strength": (6, 24, 3)}[variant]
    if variant == "mask":
        src, keep = FR.source_latent(SHAPE), (hard_mask() == 1.0).expand(SHAPE)
        assert torch.equal(a.cpu()[keep], src[keep])                     # masked cells equal the source
        assert rel(a.cpu()[~keep], src[~keep]) > 1e-2


def test_a_guided_source_with_an_unguided_target(tiny_dit, cfg, tiny_sd, golden):
    """3.5 / 1: the negative prompt serves the source side alone — its forward runs, the target side's unconditional velocity is never sized"""
    _, _, se = prompts(golden)
    kw = dict(init_latent=FR.source_latent(SHAPE), strength=STRENGTH, source_text_embeds=se, source_text_rope_pos=torch.arange(FR.SOURCE_TEXT_LEN),
              source_guidance_weight=3.5, flowedit_seed=SEED)
    fresh = make_dit(cfg, tiny_sd)   # a handle that has never run a guided step: ws_vel_u does not exist
    fresh.flowedit_state(reset=True)
    a = run_generate(fresh, golden, 1.0, **kw)
    assert fresh.flowedit_state(reset=True) == (4, 4 * 3, 3) and torch.isfinite(a).all()
    assert torch.equal(a, run_generate(Wrapped(tiny_dit), golden, 1.0, **kw))
    assert torch.equal(a, run_generate(tiny_dit, golden, 1.0, **kw))
    assert not torch.equal(a, run_generate(tiny_dit, golden, 1.0, **dict(kw, source_guidance_weight=1.0)))
    fresh._destroy_engine(force=True)


def test_a_batch_runs_one_sample_at_a_time_with_a_seed_each(tiny_dit, golden, fused_runs):
    from kandinsky.generation_utils import generate
    te, ne, se = prompts(golden)
    src = FR.source_latent(SHAPE)
    shape2 = (2 * SHAPE[0],) + SHAPE[1:]
    args = ("cuda:0", shape2, STEPS, te, ne, POS, torch.arange(7), torch.arange(4), 5.0, 5.0, FLASH)
    kw = dict(batch=2, init_latent=src.repeat(2, 1, 1, 1), strength=STRENGTH, source_text_embeds=se,
              source_text_rope_pos=torch.arange(FR.SOURCE_TEXT_LEN), source_guidance_weight=2.0, flowedit_seed=SEED)
    both = generate(tiny_dit, *args, noise=torch.zeros(shape2), **kw)
    assert torch.equal(both[:SHAPE[0]], fused_runs["g2_5"][0])                                       # sample 0: the seed itself
    assert torch.equal(both[SHAPE[0]:], run_flowedit(tiny_dit, golden, "g2_5", flowedit_seed=SEED + 1))   # sample 1: seed + 1
    assert torch.equal(both, generate(Wrapped(tiny_dit), *args, noise=torch.zeros(shape2), **kw))


def test_equal_prompts_and_weights_return_the_source(tiny_dit, golden):
    te, _, _ = prompts(golden)
    src = FR.source_latent(SHAPE)
    for name in ("g1_1", "g2_5"):
        w = CASES[name][1]
        tiny_dit.flowedit_state(reset=True)
        # the same tensors on both sides: one prompt to the engine, which tells prompts apart by their addresses
        out = run_generate(tiny_dit, golden, w, te=te, init_latent=src, strength=STRENGTH, source_text_embeds=te,
                           source_text_rope_pos=torch.arange(7), source_guidance_weight=w, flowedit_seed=SEED)
        assert torch.equal(out.cpu(), src), name
        assert tiny_dit.flowedit_state(reset=True) == (4, 4 * (2 if w == 1.0 else 4), 1 if w == 1.0 else 2)


def test_a_seed_repeats_and_another_differs(tiny_dit, golden, fused_runs):
    assert torch.equal(run_flowedit(tiny_dit, golden, "g2_5"), fused_runs["g2_5"][0])
    assert not torch.equal(run_flowedit(tiny_dit, golden, "g2_5", flowedit_seed=SEED + 1), fused_runs["g2_5"][0])
    # flowedit_seed defaults to seed
    assert torch.equal(run_flowedit(tiny_dit, golden, "g2_5", flowedit_seed=None, seed=SEED), fused_runs["g2_5"][0])


def test_a_watch_sees_every_step_and_can_cancel(tiny_dit, golden, fused_runs):
    from kandinsky.models.dit import SamplingInterrupted
    for model in (tiny_dit, Wrapped(tiny_dit)):
        seen = []
        out = run_flowedit(model, golden, "g2_5", callback=lambda info: seen.append((info.step, info.num_steps)) and False)
        assert seen == [(i, 4) for i in range(4)] and torch.equal(out, fused_runs["g2_5"][0])
        with pytest.raises(SamplingInterrupted) as stop:
            run_flowedit(model, golden, "g2_5", callback=lambda info: info.step == 1)
        assert 2 <= stop.value.steps_done <= 3
    assert tiny_dit._watch is None


def test_other_calls_on_the_handle_keep_their_bits(tiny_dit, golden, fused_runs):
    src = FR.source_latent(SHAPE)

    def others():
        return (run_generate(tiny_dit, golden, 5.0), run_generate(tiny_dit, golden, 5.0, init_latent=src, strength=0.5, keep_mask=hard_mask()),
                run_generate(tiny_dit, golden, 5.0, eta=1.0, sde_seed=SEED))
    before = others()
    assert torch.equal(run_flowedit(tiny_dit, golden, "g2_5", flowedit_refine=1), run_flowedit(tiny_dit, golden, "g2_5", flowedit_refine=1))
    after = others()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert torch.equal(run_flowedit(tiny_dit, golden, "g2_5"), fused_runs["g2_5"][0])
    assert all(getattr(tiny_dit, a) is None for a in ("_watch", "_nag", "_regions", "_guidance", "_skip", "_stochastic", "_enhance", "_forecast"))


def test_c_level_refusals_leave_the_latent_untouched(tiny_dit, cfg, tiny_sd, golden):
    import ctypes as C
    from kandinsky import _engine as E
    from kandinsky.generation_utils import sigma_schedule, stochastic_plan
    from kandinsky.magcache_utils import disable_magcache, set_magcache_params, start_magcache_calibration, stop_magcache_calibration
    te, ne, se = prompts(golden)
    lat = golden["gen.noise"].cuda().contiguous()
    before = lat.clone()
    src, mask = FR.source_latent(SHAPE).cuda(), hard_mask().cuda()
    spos = torch.arange(FR.SOURCE_TEXT_LEN)
    good = dict(source=src, text=se, pos=spos, w=2.0, mask=None, refine=0, seed=SEED, first=0)

    def call(d, steps=4, **kw):
        return d.sample(lat, sigma_schedule(steps, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0),
                        flowedit=tuple(dict(good, **kw).values()))

    def refused(d, status, word, steps=4, **kw):
        """the call fails with `status` and a message holding `word`; nothing ran: the latent and the counters are as they were"""
        d.flowedit_state(reset=True)
        with pytest.raises(RuntimeError, match=f"status {status}") as e:
            call(d, steps, **kw)
        assert "k5_sample_flowedit" in str(e.value) and word in str(e.value), (word, str(e.value))
        torch.cuda.synchronize()
        assert torch.equal(lat, before) and d.flowedit_state() == (0, 0, 0), word

    # K5_ERR_ARG through the host binding
    refused(tiny_dit, K5_ERR_ARG, "refine must be in 0..num_steps", refine=5)
    refused(tiny_dit, K5_ERR_ARG, "refine must be in 0..num_steps", refine=-1)
    refused(tiny_dit, K5_ERR_ARG, "with a keep_mask", mask=mask, refine=1)
    refused(tiny_dit, K5_ERR_ARG, "source overlaps latent", source=lat)
    with pytest.raises(ValueError):
        tiny_dit.sample(lat, sigma_schedule(4, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0, flowedit=tuple(good.values())[:7])
    with pytest.raises(ValueError):
        tiny_dit.sample(lat, sigma_schedule(4, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0, flowedit=tuple(good.values()),
                        edit=(src, src, None))

    # K5_ERR_ARG that the binding cannot form: the C entry point itself
    s, keep = E.SampleArgs(), []
    keep += tiny_dit._fill_sample_args(s, lat, None, sigma_schedule(4, 5.0).tolist(), te, ne, POS, torch.arange(7), torch.arange(4), 5.0,
                                       (1.0, 2.0, 2.0), None, None)[0]
    h = tiny_dit.engine(lat.device)
    scond = tiny_dit._text_cond(se["text_embeds"], se["pooled_embed"], spos, keep)
    vcond = torch.zeros(*SHAPE[:-1], 17, device="cuda")

    def c_call(word, vc=None, **kw):
        a = dict(source=src.data_ptr(), source_cond=scond, source_weight=2.0, keep_mask=None, refine=0, seed=SEED, first_stream=0)
        a.update(kw)
        tiny_dit.flowedit_state(reset=True)
        assert E.lib().k5_sample_flowedit(h, C.byref(s), C.byref(E.FlowEditArgs(**a)), vc, E.stream_ptr()) == K5_ERR_ARG, word
        assert word.encode() in E.lib().k5_last_error(), (word, E.lib().k5_last_error())
        torch.cuda.synchronize()
        assert torch.equal(lat, before) and tiny_dit.flowedit_state() == (0, 0, 0), word

    c_call("needs a source latent and a source prompt", source=None)
    c_call("needs a source latent and a source prompt", source_cond=E.TextCond())
    c_call("keep_mask overlaps latent", keep_mask=lat.data_ptr() + 64)
    c_call("visual_cond overlaps latent", vc=lat.data_ptr())
    c_call("source is not 4-byte aligned", source=src.data_ptr() + 2)
    c_call("keep_mask is not 4-byte aligned", keep_mask=mask.data_ptr() + 2)
    c_call("visual_cond is not 4-byte aligned", vc=vcond.data_ptr() + 2)
    assert E.lib().k5_sample_flowedit(h, C.byref(s), None, None, E.stream_ptr()) == K5_ERR_ARG and b"null FlowEdit arguments" in E.lib().k5_last_error()

    # K5_ERR_STATE: what is set on the handle
    W, b = torch.zeros(16, 3), torch.zeros(3)
    settings = [(lambda: tiny_dit.set_stochastic(*stochastic_plan(sigma_schedule(4, 5.0).tolist(), 1.0), seed=1), tiny_dit.clear_stochastic, "stochastic plan"),
                (lambda: tiny_dit.set_guidance(zero_star=True), tiny_dit.clear_guidance, "guidance plan"),
                (lambda: tiny_dit.set_skip_guidance([1], 2.0), tiny_dit.clear_skip_guidance, "skip-layer guidance"),
                (lambda: tiny_dit.set_nag(ne, torch.arange(4)), tiny_dit.clear_nag, "normalized attention guidance"),
                (lambda: tiny_dit.set_regions([ne], [torch.arange(4)], torch.ones(1, *SHAPE[:-1], device="cuda")), tiny_dit.clear_regions, "regional prompts"),
                (lambda: tiny_dit.set_forecast(1, [1, 1, 0, 1]), tiny_dit.clear_forecast, "forecast plan"),
                (lambda: tiny_dit.set_watch(lambda info: False, 1, W, b), tiny_dit.clear_watch, "previews")]
    for put, clear, word in settings:
        put()
        try:
            refused(tiny_dit, K5_ERR_STATE, word)
        finally:
            clear()
    # MagCache, its calibration, a sequence-parallel group and a CFG pair, each on a handle of its own (loopback transport: the handle's state
    # is what is refused, no peer is needed)
    c = [c for c in json.load(open(os.path.join(GOLDEN, "magcache_meta.json")))["cases"] if c["tag"] == "hand_10"][0]
    d = make_dit(cfg, tiny_sd)
    d.engine("cuda:0")
    set_magcache_params(d, c["ratios"], c["num_steps"], c["no_cfg"])
    try:
        refused(d, K5_ERR_STATE, "MagCache is set", steps=c["num_steps"])
    finally:
        disable_magcache(d)
    start_magcache_calibration(d, 4, False)
    try:
        refused(d, K5_ERR_STATE, "MagCache calibration")
    finally:
        stop_magcache_calibration(d)
    d._destroy_engine(force=True)
    for kind in ("sequence-parallel group", "CFG pair"):
        d = make_dit(cfg, tiny_sd)
        d.engine("cuda:0")
        group = E.LoopbackGroup(2)
        d.enable_loopback(group, 0) if kind == "sequence-parallel group" else d.enable_cfg_pair_loopback(group, 0)
        refused(d, K5_ERR_STATE, kind)
        d._destroy_engine(force=True)

    # a refused call is no state: the arguments they were derived from are good and run
    tiny_dit.flowedit_state(reset=True)
    call(tiny_dit)
    assert tiny_dit.flowedit_state(reset=True) == (4, 16, 3) and not torch.equal(lat, before)


# ------------------------------------------------------------------------------------------ parity
@pytest.fixture(scope="module")
def flowedit_golden():
    from safetensors.torch import load_file
    return (load_file(os.path.join(GOLDEN, "dit_tiny_flowedit.safetensors")),
            json.load(open(os.path.join(GOLDEN, "dit_tiny_flowedit_meta.json"))))


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_reference_golden_on_the_edit(golden, flowedit_golden, fused_runs, name):
    """Measured on the MI355X, on the edit, for guidance 1 / 1, 2 / 5, 1 / 5: engine vs golden 9.42e-3 / 1.026e-2 / 9.66e-3, recorded oracle vs
    golden 9.41e-3 / 1.013e-2 / 9.79e-3, engine vs oracle 7.2e-3 / 9.4e-3 / 8.5e-3; the test prints them."""
    gold, meta = flowedit_golden
    case = meta["cases"][name]
    assert (meta["steps"], meta["scheduler_scale"], meta["seed"], meta["strength"]) == (STEPS, 5.0, SEED, STRENGTH)
    assert (case["w_src"], case["w_tar"]) == CASES[name]
    src = FR.source_latent(SHAPE)
    sp = FR.source_prompt(golden)
    assert torch.equal(gold["flowedit.source"], src)
    assert torch.equal(gold["flowedit.source_text"], sp["text_embeds"]) and torch.equal(gold["flowedit.source_pooled"], sp["pooled_embed"])
    out, g, o = fused_runs[name][0].cpu(), gold[f"flowedit.{name}.final"], gold[f"flowedit.{name}.oracle"]
    edit = (g - src).norm()
    d_engine, d_oracle, d_eo = ((out - g).norm() / edit).item(), ((o - g).norm() / edit).item(), ((out - o).norm() / edit).item()
    print(f"flowedit {name}: on the edit, engine vs golden {d_engine:.3e}, oracle vs golden {d_oracle:.3e} (recorded "
          f"{meta['oracle_vs_golden'][name]:.3e}), engine vs oracle {d_eo:.3e}; edit / source {(edit / src.norm()).item():.3f}")
    assert abs(d_oracle - meta["oracle_vs_golden"][name]) <= 1e-6
    assert meta["oracle_vs_golden"][name] <= 3e-2 and edit >= 0.1 * src.norm()       # the generator's conditions
    assert d_engine <= 1.5 * meta["oracle_vs_golden"][name], (d_engine, meta["oracle_vs_golden"][name])
