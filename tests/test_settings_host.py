"""The settings a DiffusionTransformer3D keeps and pushes into its engine handle — watch, NAG, regions, guidance plan, skip set — as library
call sequences, without a GPU and without libk5.so: the library is a recorder that notes (name, args) and answers K5_OK or a scripted
status, the handle is a stand-in.  set / clear / state, the re-install after a rebuild, `generate`'s "for this call only" and the model's
`setting_for_call`, and what a refused install leaves behind."""
import contextlib
import ctypes as C
import functools

import pytest
import torch

import kit  # noqa: E402
from kit import K5_ERR_ARG, POS, flash_conf, host_tiny  # noqa: E402

CONF = flash_conf()
SHAPE = (3, 8, 12, 16)
SETTERS = ["k5_dit_set_watch", "k5_dit_set_nag", "k5_dit_set_regions", "k5_dit_set_guidance", "k5_dit_set_skip_guidance"]   # the re-install order
ATTRS = ["_watch", "_nag", "_regions", "_guidance", "_skip"]


class Recorder:
    """Stands where `_engine.lib()` does: every attribute is a function that appends (name, args) to `calls` and returns K5_OK, or the next
    status scripted for it in `script`; `fill[name]` is written into the out-parameters (the `byref` arguments) of a state getter."""

    def __init__(self):
        self.calls, self.script, self.fill = [], {}, {}

    def __getattr__(self, name):
        def fn(*args):
            if name == "k5_last_error":
                return b"scripted"
            self.calls.append((name, args))
            outs = [a._obj for a in args if type(a).__name__ == "CArgObject"]
            for o, v in zip(outs, self.fill.get(name, ())):
                o.value = v
            queue = self.script.get(name)
            return queue.pop(0) if queue else 0
        return fn

    def setters(self):
        """(name, is it the clearing call) of the setter calls so far, in order"""
        return [(n, a[1] is None) for n, a in self.calls if n in SETTERS]

    def last(self, name):
        return [a for n, a in self.calls if n == name][-1]


@pytest.fixture
def rig(monkeypatch, golden_meta):
    from kandinsky import _engine as E
    rec = Recorder()
    monkeypatch.setattr(E, "lib", lambda: rec)
    monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)   # torch.cuda.device(...) raises without a GPU
    made = []

    def make(handle=True):
        m = host_tiny(golden_meta)
        if handle:
            m._handle, m._handle_device = C.c_void_p(0x5e77), torch.device("cpu")
        made.append(m)
        return m

    yield rec, make
    for m in made:          # before the patches are undone: __del__ must not hand the stand-in handle to a real library
        m._handle = None


prompt = functools.partial(kit.host_prompt, dims=(96, 48))


def half_mask(R=1):
    m = torch.zeros(R, 3, 8, 12)
    m[:, :, :, :6] = 1.0
    return m


def set_all(m, seed=0):
    """every setting at once, each with values of its own; returns the callback"""
    cb = lambda info: False   # noqa: E731
    m.set_watch(cb)
    m.set_nag(prompt(4, seed + 1), torch.arange(4), 4.0, 2.0, 0.5)
    m.set_regions([prompt(5, seed + 2), prompt(3, seed + 3)], [torch.arange(5), torch.arange(3)], half_mask(2), 0.25)
    m.set_guidance([5.0, 4.0, 1.0], True, 1, 0.5)
    m.set_skip_guidance([1, 0], 3, mode="attention", steps=[1, 0, 1])
    return cb


call_generate = functools.partial(kit.call_generate, w=5.0, steps=3, shape=SHAPE, pos=POS, conf=CONF, prompt=prompt)


def per_call_keywords(seed=10):
    """`generate` keywords that install each of the five settings for the call, by setter"""
    return {"k5_dit_set_watch": dict(callback=lambda info: False),
            "k5_dit_set_nag": dict(nag_text_embeds=prompt(6, seed), nag_text_rope_pos=torch.arange(6), nag_scale=3.0, nag_tau=1.5, nag_alpha=1.0),
            "k5_dit_set_regions": dict(region_text_embeds=[prompt(2, seed + 1)], region_text_rope_pos=[torch.arange(2)], region_masks=half_mask(),
                                       region_base_weight=0.5),
            "k5_dit_set_guidance": dict(cfg_rescale=0.7),
            "k5_dit_set_skip_guidance": dict(slg_blocks=[1], slg_scale=2.0)}


# ------------------------------------------------------------------------------------------ set, clear, state
def test_set_marshals_each_setting_into_its_setter(rig):
    from kandinsky import _engine as E
    rec, make = rig
    m = make()
    set_all(m)
    assert rec.setters() == [(n, False) for n in SETTERS]
    h = m._handle
    assert all(a[0] is h for _, a in rec.calls)
    w = rec.last("k5_dit_set_watch")[1]._obj
    assert isinstance(w, E.Watch) and (w.preview_every, w.want_x0) == (0, 0) and w is m._watch[1]
    cond, *numbers = rec.last("k5_dit_set_nag")[1:]
    assert numbers == [4.0, 2.0, 0.5] and cond._obj.text_len == 4 and list(cond._obj.text_rope_pos[:4]) == [0, 1, 2, 3]
    conds, R, masks, T, H, W, base = rec.last("k5_dit_set_regions")[1:]
    assert (R, T, H, W, base) == (2, 3, 8, 12, 0.25) and [conds[0].text_len, conds[1].text_len] == [5, 3] and isinstance(masks, int)
    g = rec.last("k5_dit_set_guidance")[1]._obj
    assert list(g.weights[:3]) == [5.0, 4.0, 1.0] and (g.num_weights, g.zero_star, g.zero_init_steps, g.rescale) == (3, 1, 1, 0.5)
    s = rec.last("k5_dit_set_skip_guidance")[1]._obj
    assert list(s.blocks[:2]) == [1, 0] and list(s.steps[:3]) == [1, 0, 1] and (s.num_blocks, s.mode, s.scale, s.num_steps) == (2, 1, 3.0, 3)
    # the stored values keep their shape
    assert m._nag["args"] == (4.0, 2.0, 0.5) and m._regions["base_weight"] == 0.25 and len(m._regions["text"]) == 2
    assert m._guidance == ([5.0, 4.0, 1.0], True, 1, 0.5) and m._skip == ([1, 0], 3.0, "attention", [1, 0, 1])


def test_clear_makes_the_clearing_call_and_forgets(rig):
    rec, make = rig
    m = make()
    set_all(m)
    del rec.calls[:]
    assert m.clear_watch() is m and m.clear_nag() is m and m.clear_regions() is m and m.clear_guidance() is m and m.clear_skip_guidance() is m
    assert m.set_watch(None) is m                                   # callback None = clear_watch
    assert [(n, a[1:]) for n, a in rec.calls] == [
        ("k5_dit_set_watch", (None,)), ("k5_dit_set_nag", (None, 1.0, 1.0, 0.0)), ("k5_dit_set_regions", (None, 0, None, 0, 0, 0, 0.0)),
        ("k5_dit_set_guidance", (None,)), ("k5_dit_set_skip_guidance", (None,)), ("k5_dit_set_watch", (None,))]
    assert all(getattr(m, a) is None for a in ATTRS)


def test_without_a_handle_nothing_calls_the_library(rig):
    rec, make = rig
    m = make(handle=False)
    cb = set_all(m)
    assert m._watch[0].callback is cb and all(getattr(m, a) is not None for a in ATTRS)
    assert m.watch_state() == (0, False) and m.nag_state() == (False, 0) and m.regions_state() == (False, 0, 0)
    assert m.guidance_state() == (False, 0, 0, 0) and m.skip_state() == (False, 0, 0, 0)
    m.clear_watch().clear_nag().clear_regions().clear_guidance().clear_skip_guidance()
    assert all(getattr(m, a) is None for a in ATTRS) and rec.calls == []


def test_state_getters_return_the_out_parameters(rig):
    rec, make = rig
    m = make()
    rec.fill = {"k5_dit_watch_state": (3, 1), "k5_dit_nag_state": (1, 8), "k5_dit_regions_state": (1, 2, 6),
                "k5_dit_guidance_state": (1, 5, 4, 3), "k5_dit_skip_state": (1, 2, 7, 9)}
    got = [m.watch_state(), m.nag_state(), m.regions_state(reset=True), m.guidance_state(), m.skip_state(reset=True)]
    assert got == [(3, True), (True, 8), (True, 2, 6), (True, 5, 4, 3), (True, 2, 7, 9)]
    assert all(type(g) is tuple for g in got) and type(got[0][1]) is bool and all(type(g[0]) is bool for g in got[1:])
    assert [(n, len(a), a[-1]) for n, a in rec.calls[1:]] == [("k5_dit_nag_state", 4, 0), ("k5_dit_regions_state", 5, 1),
                                                             ("k5_dit_guidance_state", 6, 0), ("k5_dit_skip_state", 6, 1)]
    assert rec.calls[0][0] == "k5_dit_watch_state" and len(rec.calls[0][1]) == 3


# ------------------------------------------------------------------------------------------ after a rebuild
def test_reapply_installs_every_setting_once_in_order(rig):
    rec, make = rig
    m = make(handle=False)
    set_all(m)
    m._handle, m._handle_device = C.c_void_p(0x5e77), torch.device("cpu")    # the engine was just built
    m._reapply_settings()
    assert rec.setters() == [(n, False) for n in SETTERS] and len(rec.calls) == 5
    assert rec.last("k5_dit_set_nag")[2:] == (4.0, 2.0, 0.5) and rec.last("k5_dit_set_regions")[2] == 2


def test_reapply_skips_what_is_not_set(rig):
    rec, make = rig
    m = make()
    m._reapply_settings()
    assert rec.calls == []
    m.set_guidance(rescale=0.5)
    m.set_nag(prompt(4), torch.arange(4))
    del rec.calls[:]
    m._reapply_settings()
    assert rec.setters() == [("k5_dit_set_nag", False), ("k5_dit_set_guidance", False)] and len(rec.calls) == 2


# ------------------------------------------------------------------------------------------ for one call
@pytest.mark.parametrize("setter", SETTERS)
@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("boom", [False, True])
def test_generate_installs_for_the_call_and_puts_back_what_was_there(rig, setter, held, boom):
    """over a setting the model holds: the new one, then the old one again; over none: the new one, then the clearing call; also when the
    run raises"""
    rec, make = rig
    m = make()
    if held:
        set_all(m)
    attr = ATTRS[SETTERS.index(setter)]
    seen = []

    def sample(img, *a, **k):
        seen.append(getattr(m, attr))
        if boom:
            raise RuntimeError("boom")

    m.sample = sample
    del rec.calls[:]
    with (pytest.raises(RuntimeError, match="boom") if boom else contextlib.nullcontext()):
        call_generate(m, **per_call_keywords()[setter])
    assert [c for c in rec.setters() if c[0] == setter] == [(setter, False), (setter, not held)]
    assert [c for c in rec.setters() if c[0] != setter] == []
    assert len(seen) == 1 and seen[0] is not None
    assert (getattr(m, attr) is not None) == held
    if held:    # what the engine holds again is the setting from before the call
        want = {"k5_dit_set_nag": lambda a: a[2:] == (4.0, 2.0, 0.5), "k5_dit_set_regions": lambda a: a[2] == 2 and a[-1] == 0.25,
                "k5_dit_set_guidance": lambda a: a[1]._obj.num_weights == 3, "k5_dit_set_skip_guidance": lambda a: a[1]._obj.num_blocks == 2,
                "k5_dit_set_watch": lambda a: a[1]._obj is m._watch[1]}[setter]
        assert want(rec.last(setter))


@pytest.mark.parametrize("setter", SETTERS)
def test_generate_puts_back_the_very_object_it_found(rig, setter):
    rec, make = rig
    m = make()
    set_all(m)
    attr = ATTRS[SETTERS.index(setter)]
    before = getattr(m, attr)
    m.sample = lambda img, *a, **k: None
    call_generate(m, **per_call_keywords()[setter])
    assert getattr(m, attr) is before


@pytest.mark.parametrize("boom", [False, True])
def test_setting_for_call_on_the_model(rig, boom):
    rec, make = rig
    m = make()
    m.set_guidance(rescale=0.25)
    before = m._guidance
    del rec.calls[:]
    with (pytest.raises(RuntimeError, match="boom") if boom else contextlib.nullcontext()):
        with m.setting_for_call("guidance", (None, True, 0, 0.5)), m.setting_for_call("nag", (prompt(4), torch.arange(4), 3.0)), \
                m.setting_for_call("regions", None), m.setting_for_call("watch", None):
            assert m._guidance == (None, True, 0, 0.5) and m._nag["args"] == (3.0, 2.5, 0.25) and m._regions is None
            if boom:
                raise RuntimeError("boom")
    assert m._guidance is before and m._nag is None
    assert rec.setters() == [("k5_dit_set_guidance", False), ("k5_dit_set_nag", False), ("k5_dit_set_nag", True), ("k5_dit_set_guidance", False)]
    assert rec.last("k5_dit_set_guidance")[1]._obj.rescale == 0.25


# ------------------------------------------------------------------------------------------ a refused install
def refused_installs(m, rec):
    """the ways an install can fail once the arguments have passed the Python checks, as (what, call that must raise)"""
    def refuse(name):
        rec.script[name] = [K5_ERR_ARG]
    return [("the library refuses set_nag", lambda: (refuse("k5_dit_set_nag"), m.set_nag(prompt(6, 9), torch.arange(6), 2.0))),
            ("the library refuses set_regions", lambda: (refuse("k5_dit_set_regions"), m.set_regions([prompt(2, 8)], [torch.arange(2)], half_mask()))),
            ("the library refuses set_guidance", lambda: (refuse("k5_dit_set_guidance"), m.set_guidance(rescale=1.0))),
            ("the library refuses set_skip_guidance", lambda: (refuse("k5_dit_set_skip_guidance"), m.set_skip_guidance([0], 1.0))),
            ("the library refuses set_watch", lambda: (refuse("k5_dit_set_watch"), m.set_watch(lambda info: True))),
            ("marshalling NAG raises", lambda: m._put("nag", {"text": torch.zeros(4, 96), "pooled": None, "pos": torch.arange(3), "args": (2.0, 2.0, 1.0)})),
            ("marshalling regions raises", lambda: m._put("regions", {"text": [torch.zeros(4, 96)], "pos": [torch.arange(5)], "masks": half_mask(),
                                                                      "base_weight": 0.0}))]


def test_a_refused_install_keeps_the_previous_setting_and_what_the_engine_borrows(rig):
    rec, make = rig
    m = make()
    set_all(m)
    stored = [getattr(m, a) for a in ATTRS]
    borrowed = dict(m._borrowed)
    assert set(borrowed) == {"watch", "nag", "regions", "guidance", "skip_guidance"}
    nag_cond = rec.last("k5_dit_set_nag")[1]._obj            # the struct and array the engine reads at the next forward
    region_conds = rec.last("k5_dit_set_regions")[1]
    for what, attempt in refused_installs(m, rec):
        del rec.calls[:]
        with pytest.raises((RuntimeError, ValueError)):
            attempt()
        assert all(getattr(m, a) is s for a, s in zip(ATTRS, stored)), what
        assert all(m._borrowed[k] is v for k, v in borrowed.items()) and len(m._borrowed) == 5, what
        assert not any(cleared for _, cleared in rec.setters()), what
    assert m._borrowed["nag"][0][0]._obj is nag_cond and m._borrowed["regions"][0][0] is region_conds
    assert any(t.data_ptr() == nag_cond.text_embed for t in m._borrowed["nag"][1] if torch.is_tensor(t))


def test_a_refused_install_over_nothing_leaves_nothing(rig):
    rec, make = rig
    m = make()
    for what, attempt in refused_installs(m, rec):
        with pytest.raises((RuntimeError, ValueError)):
            attempt()
        assert all(getattr(m, a) is None for a in ATTRS) and m._borrowed == {}, what
    assert not any(cleared for _, cleared in rec.setters())


def test_a_refused_install_inside_generate_still_puts_the_previous_setting_back(rig):
    rec, make = rig
    m = make()
    set_all(m)
    before = m._nag
    m.sample = lambda *a, **k: pytest.fail("the refused call must not sample")
    del rec.calls[:]
    rec.script["k5_dit_set_nag"] = [K5_ERR_ARG]
    with pytest.raises(RuntimeError, match="k5_dit_set_nag"):
        call_generate(m, **per_call_keywords()["k5_dit_set_nag"])
    assert m._nag is before and rec.setters() == [("k5_dit_set_nag", False), ("k5_dit_set_nag", False)]
    assert rec.last("k5_dit_set_nag")[2:] == (4.0, 2.0, 0.5)
