"""CPU-only checks of the sampler watch (progress, cancel, previews): the ctypes mirror of k5_watch / k5_watch_info against the header, the
exports, the factor fit and its file format, the callback trampoline, and `progress=True` without tqdm."""
import builtins
import ctypes as C
import os
import re
import sys

import pytest
import torch

from kit import ABI_VERSION_PIN, ROOT, built_lib  # noqa: E402


def header():
    src = open(os.path.join(ROOT, "include", "k5.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def struct_fields(name):
    """[(C type, field name)] of `typedef struct name { ... } name;` in include/k5.h, declaration order, `int a, b;` expanded"""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), header(), flags=re.S).group(1)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*(?:\s*,\s*[A-Za-z_][A-Za-z0-9_]*)*)$", decl, flags=re.S)
        ctype = " ".join(m.group(1).split())
        out += [(ctype, n.strip()) for n in m.group(2).split(",")]
    return out


CTYPE = {"int": C.c_int, "float": C.c_float, "const uint8_t*": C.POINTER(C.c_uint8), "const float*": C.POINTER(C.c_float),
         "void*": C.c_void_p}


def test_ctypes_structs_match_the_header():
    from kandinsky import _engine as E
    CTYPE["k5_watch_fn"] = E.WATCH_FN
    for name, cls in (("k5_watch_info", E.WatchInfo), ("k5_watch", E.Watch)):
        want = struct_fields(name)
        assert [n for _, n in want] == [n for n, _ in cls._fields_], name
        for (ctype, n), (_, have) in zip(want, cls._fields_):
            assert CTYPE[ctype] is have, (name, n, ctype, have)
    assert [n for _, n in struct_fields("k5_watch_info")] == ["step", "num_steps", "sample", "num_samples", "sigma_next", "rgb", "x0", "T", "H", "W", "C"]
    # the callback type: int (*)(void* user, const k5_watch_info* info)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*k5_watch_fn\s*\)\s*\(\s*void\s*\*\s*user\s*,\s*const\s+k5_watch_info\s*\*\s*info\s*\)\s*;", header())
    assert E.WATCH_FN._restype_ is C.c_int and E.WATCH_FN._argtypes_ == (C.c_void_p, C.POINTER(E.WatchInfo))


def test_library_exports_the_watch_and_keeps_the_abi_number(built_lib):
    from kandinsky import _engine as E
    lib = C.CDLL(built_lib)
    for n in ("k5_dit_set_watch", "k5_dit_watch_state", "k5_x0_preview"):
        assert hasattr(lib, n), n
        assert n in E.SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % n, header()), n
    lib.k5_abi_version.restype = C.c_int
    assert lib.k5_abi_version() == ABI_VERSION_PIN == E.ABI_VERSION
    # null handles are refused with a message, not dereferenced
    L = E.lib()
    assert L.k5_dit_set_watch(None, None) != 0 and b"null handle" in L.k5_last_error()
    assert L.k5_dit_watch_state(None, None, None) != 0


def test_x0_preview_refuses_unsupported_channel_counts_without_a_gpu(built_lib):
    """the launcher decides before any launch: nothing here touches a device"""
    from kandinsky import _engine as E
    L = E.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    K5_ERR_ARG, K5_ERR_UNSUPPORTED = 1, 6
    assert re.search(r"K5_ERR_ARG\s*=\s*1\b", header()) and re.search(r"K5_ERR_UNSUPPORTED\s*=\s*6\b", header())
    for Cc in (6, 68, 0, -4):
        assert L.k5_x0_preview(p, p, None, 1.0, 0.5, None, None, p, None, None, p, 4, Cc, None) == K5_ERR_UNSUPPORTED, Cc
    assert L.k5_x0_preview(p, p, None, 1.0, 0.5, None, None, None, None, None, None, 4, 16, None) == K5_ERR_ARG      # no output asked for
    assert L.k5_x0_preview(p, p, None, 1.0, 0.5, None, None, None, None, None, p, 4, 16, None) == K5_ERR_ARG         # rgb without factors
    assert L.k5_x0_preview(p, p, None, 1.0, 0.5, None, p, p, None, None, p, 4, 16, None) == K5_ERR_ARG               # a mask without a source
    assert L.k5_x0_preview(p + 4, p, None, 1.0, 0.5, None, None, p, None, None, p, 4, 16, None) == K5_ERR_ARG        # latent not 16-byte aligned
    assert L.k5_x0_preview(p, p, None, 1.0, 0.5, None, None, p, None, None, p, 0, 16, None) == K5_ERR_ARG            # no cells


# ------------------------------------------------------------------------------------------ factors
def synthetic_pair(T, H, W, Cc, seed, noise=0.0):
    """latent (T,H,W,C) and frames (F,3,8H,8W) whose cell means are exactly b + latent @ Wt; within a cell the pixels vary (zero-mean per
    cell and frame group), so a fit against a single pixel or a single frame of the group would miss"""
    g = torch.Generator().manual_seed(seed)
    Wt = (torch.rand(Cc, 3, generator=g, dtype=torch.float64) - 0.5) * 0.5
    b = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.2
    lat = torch.randn(T, H, W, Cc, generator=g, dtype=torch.float64)
    mean = lat @ Wt + b                                            # (T,H,W,3)
    F = 1 + 4 * (T - 1)
    frames = torch.empty(F, 3, 8 * H, 8 * W, dtype=torch.float64)
    for t in range(T):
        fr = [0] if t == 0 else list(range(4 * t - 3, 4 * t + 1))
        tex = torch.randn(len(fr), 3, H, 8, W, 8, generator=g, dtype=torch.float64) * 0.3
        tex = tex - tex.mean(dim=(0, 3, 5), keepdim=True)          # zero mean over the cell's pixels AND its frames together
        frames[fr] = (mean[t].permute(2, 0, 1)[None, :, :, None, :, None] + tex).reshape(len(fr), 3, 8 * H, 8 * W)
    return lat, frames, Wt, b


@pytest.mark.parametrize("T,H,W,Cc", [(3, 4, 5, 16), (1, 6, 6, 4), (2, 3, 7, 8)])
def test_fit_rgb_factors_recovers_a_known_affine_map(T, H, W, Cc):
    from kandinsky.preview import cell_means, fit_rgb_factors
    lat, frames, Wt, b = synthetic_pair(T, H, W, Cc, seed=T * 100 + Cc)
    assert torch.allclose(cell_means(frames, T, H, W), lat @ Wt + b, atol=1e-12, rtol=0)
    Wf, bf = fit_rgb_factors(lat.float(), frames.float())
    assert Wf.dtype == torch.float32 and tuple(Wf.shape) == (Cc, 3) and tuple(bf.shape) == (3,)
    assert (Wf.double() - Wt).abs().max() <= 1e-5, (Wf.double() - Wt).abs().max()
    assert (bf.double() - b).abs().max() <= 1e-5
    # channels-last frames are the same picture; uint8 frames map to [-1, 1] as v / 127.5 - 1
    Wl, bl = fit_rgb_factors(lat.float(), frames.float().permute(0, 2, 3, 1))
    assert torch.equal(Wl, Wf) and torch.equal(bl, bf)
    u8 = torch.full((frames.shape[0], 8 * H, 8 * W, 3), 255, dtype=torch.uint8)
    u8[..., 1] = 0
    assert torch.equal(cell_means(u8, T, H, W), torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64).expand(T, H, W, 3))
    if T > 1:   # the temporal grouping is 1 frame, then 4 per latent frame: a uniform grouping of the same frames does not reproduce the means
        wrong = frames[:-1].reshape(T - 1, 4, 3, H, 8, W, 8).mean(dim=(1, 4, 6)).permute(0, 2, 3, 1)
        assert not torch.allclose(wrong, (lat @ Wt + b)[1:], atol=1e-3)
    with pytest.raises(ValueError, match="covers frames"):
        fit_rgb_factors(lat.float(), frames[:, :, :-8])


def test_factors_round_trip_through_json(tmp_path):
    from kandinsky.preview import as_factors, load_factors, save_factors
    g = torch.Generator().manual_seed(3)
    W, b = torch.randn(16, 3, generator=g) * 0.1234567, torch.randn(3, generator=g)
    path = save_factors(str(tmp_path / "f.json"), W, b, note="unit test")
    W2, b2 = load_factors(path)
    assert torch.equal(W, W2) and torch.equal(b, b2)             # float32 -> repr -> float32 is exact
    W3, b3 = as_factors(path)
    assert torch.equal(W3, W) and torch.equal(b3, b)
    assert as_factors((W, b))[0] is W and as_factors((W, b))[1] is b and as_factors(W) == (W, None) and as_factors(None) == (None, None)
    save_factors(path, W)                                          # no bias = zeros
    assert torch.equal(load_factors(path)[1], torch.zeros(3))
    with pytest.raises(ValueError):
        save_factors(path, torch.zeros(16, 4))
    (tmp_path / "bad.json").write_text('{"channels": 4, "factors": [[1, 2, 3]], "bias": [0, 0, 0]}')
    with pytest.raises(ValueError):
        load_factors(str(tmp_path / "bad.json"))


def test_preview_to_image_picks_the_middle_frame():
    from kandinsky.preview import preview_to_image
    p = torch.arange(5 * 2 * 3 * 3, dtype=torch.uint8).reshape(5, 2, 3, 3)
    im = preview_to_image(p)
    assert im.size == (3, 2) and im.mode == "RGB"
    assert im.getpixel((0, 0)) == tuple(p[2, 0, 0].tolist())
    assert preview_to_image(p, frame=4).getpixel((2, 1)) == tuple(p[4, 1, 2].tolist())
    with pytest.raises(ValueError):
        preview_to_image(p.float())


# ------------------------------------------------------------------------------------------ trampoline
def test_trampoline_turns_an_exception_into_stop_and_reraise():
    from kandinsky import _engine as E

    def stub_sample(c_fn, steps):
        """what the engine does with the function pointer: call per step, stop at the first non-zero return"""
        done = 0
        for i in range(steps):
            info = E.WatchInfo(step=i, num_steps=steps, sample=0, num_samples=1, sigma_next=1.0 - (i + 1) / steps)
            done = i + 1
            if c_fn(None, C.byref(info)):
                break
        return done

    seen = []

    def cb(info):
        seen.append((info.step, round(info.sigma_next, 6)))
        if info.step == 2:
            raise KeyError("boom at 2")

    tr = E.WatchTrampoline(cb)
    fn = C.cast(tr.c_fn, E.WATCH_FN)                               # through the C function pointer, as the engine calls it
    assert stub_sample(fn, 6) == 3
    assert [s for s, _ in seen] == [0, 1, 2] and seen[1][1] == round(1.0 - 2 / 6, 6)
    assert isinstance(tr.error, KeyError) and not tr.stop_requested
    with pytest.raises(KeyError, match="boom at 2"):
        tr.reraise()
    tr.reraise()                                                   # raised once
    # a truthy return is a stop the callback asked for, not an error
    tr2 = E.WatchTrampoline(lambda info: info.step == 1)
    assert stub_sample(C.cast(tr2.c_fn, E.WATCH_FN), 6) == 2
    assert tr2.stop_requested and tr2.error is None
    tr2.reset()
    assert not tr2.stop_requested
    # None / 0 / False keep going; `wrap` decides what the callback sees
    got = []
    tr3 = E.WatchTrampoline(lambda s: got.append(s), wrap=lambda info: info.step * 10)
    assert stub_sample(C.cast(tr3.c_fn, E.WATCH_FN), 3) == 3 and got == [0, 10, 20]


def test_watch_argument_errors_name_the_way_out():
    from kandinsky.models.dit import SamplingInterrupted, StepInfo, check_watch_args
    cb = lambda info: None   # noqa: E731
    with pytest.raises(ValueError, match="fit_rgb_factors"):
        check_watch_args(cb, 2, None, False, 16)
    with pytest.raises(ValueError, match="preview_every"):
        check_watch_args(cb, -1, None, False, 16)
    with pytest.raises(ValueError, match=r"\[16\]\[3\]"):
        check_watch_args(cb, 1, torch.zeros(8, 3), False, 16)
    with pytest.raises(ValueError, match="want_x0"):
        check_watch_args(cb, 0, None, True, 16)
    with pytest.raises(ValueError, match="C % 4"):
        check_watch_args(cb, 1, torch.zeros(6, 3), False, 6)
    W, every = check_watch_args(cb, 3, [[0.1, 0.2, 0.3]] * 16, True, 16)
    assert every == 3 and W.dtype == torch.float32 and tuple(W.shape) == (16, 3)
    assert check_watch_args(None, 0, None, False, 16) == (None, 0)
    e = SamplingInterrupted(3, "latent")
    assert e.steps_done == 3 and e.latent == "latent" and "3 steps" in str(e)
    assert "step=1/4" in repr(StepInfo(1, 4, 0, 1, 0.5, None, None))


# ------------------------------------------------------------------------------------------ progress without tqdm
class CountingModel:
    """a duck-typed model for generate's per-step path that never reaches a kernel: the call raises a marker once the hook is set up"""
    visual_cond = False


def test_progress_is_silent_and_harmless_without_tqdm(monkeypatch, capsys):
    from kandinsky import generation_utils as G
    real_import = builtins.__import__

    def no_tqdm(name, *a, **k):
        if name == "tqdm" or name.startswith("tqdm."):
            raise ImportError("No module named 'tqdm'")
        return real_import(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_tqdm)
    monkeypatch.delitem(sys.modules, "tqdm", raising=False)
    w = G._StepWatch(CountingModel(), None, 0, None, False, True, 8, 16)
    assert w.bar is None and not w.active
    from kandinsky.models.dit import StepInfo
    assert w.step(StepInfo(0, 4, 0, 1, 0.5, None, None)) is False
    w.close()
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""
    # with a callback the hook is live, still without a bar
    calls = []
    w2 = G._StepWatch(CountingModel(), lambda i: calls.append(i.step) or (i.step == 1), 0, None, False, True, 8, 16)
    assert w2.active and w2.bar is None
    assert w2.step(StepInfo(0, 4, 0, 1, 0.5, None, None)) is False and w2.step(StepInfo(1, 4, 0, 1, 0.2, None, None)) is True
    assert calls == [0, 1]


def test_progress_bar_counts_batch_times_steps_when_tqdm_is_there(capsys):
    tqdm = pytest.importorskip("tqdm")
    from kandinsky import generation_utils as G
    from kandinsky.models.dit import StepInfo
    w = G._StepWatch(CountingModel(), None, 0, None, False, True, 2 * 3, 16)
    assert isinstance(w.bar, tqdm.tqdm) and w.bar.total == 6 and w.active
    for b in range(2):
        w.sample, w.num_samples = b, 2
        for i in range(3):
            info = StepInfo(i, 3, 0, 1, 0.1, None, None)
            assert w.step(info) is False
            assert (info.sample, info.num_samples) == (b, 2)
    assert w.bar.n == 6
    w.close()
    assert w.bar is None
    capsys.readouterr()


def test_generate_refuses_a_callback_on_a_multi_rank_model():
    from kandinsky import generation_utils as G
    from kandinsky.models.dit import DiffusionTransformer3D
    m = DiffusionTransformer3D(in_visual_dim=16, out_visual_dim=16, model_dim=128, ff_dim=256, num_text_blocks=1, num_visual_blocks=1,
                               in_text_dim=32, in_text_dim2=16, time_dim=64, axes_dims=(16, 24, 24))
    m._sp = (0, 2)
    with pytest.raises(ValueError, match="single-rank"):
        G._StepWatch(m, lambda i: None, 0, None, False, False, 4, 16)
    quiet = G._StepWatch(m, None, 0, None, False, True, 4, 16)     # progress stays silent there, as before
    assert quiet.bar is None and not quiet.active
    with pytest.raises(RuntimeError, match="single-rank"):
        m.set_watch(lambda i: None)
    m._sp = None
