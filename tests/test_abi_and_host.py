"""CPU-only checks: the C-ABI library loads and exports every symbol include/k5.h declares, the host
mirror keeps the reference's checkpoint layout / config schema, and the product path refuses to run
without the HIP library or on CPU tensors (no silent fallback)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from kit import PKG, ROOT, built_lib  # noqa: E402

LIB = os.path.join(PKG, "lib", "libk5.so")


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "k5.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(k5_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_all_exported(built_lib):
    import ctypes
    lib = ctypes.CDLL(built_lib)
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/k5.h but not exported by libk5.so"


def test_ctypes_table_matches_header(built_lib):
    from kandinsky import _engine as E
    assert sorted(E.SYMBOLS) == declared_symbols()
    L = E.lib()
    import re
    assert L.k5_abi_version() == E.ABI_VERSION == int(re.search(r'#define K5_ABI_VERSION (\d+)', open(os.path.join(ROOT, 'include', 'k5.h')).read()).group(1))


def test_sp_schedule_selection_rule(built_lib):
    """k5_sp_pick_schedule: the rule by which the self-tuning sequence-parallel schedule decides (pure host arithmetic, shared by all ranks):
    a candidate costs its SLOWEST rank, the cheapest wins, ties go to the lower index (the more conservative schedule), a candidate that did
    not run on some rank (<= 0, inf, NaN) or is masked out is not eligible, nothing eligible -> -1."""
    import ctypes as C
    import math
    from kandinsky import _engine as E
    L = E.lib()

    def pick(table, valid=None):
        world, nc = len(table), len(table[0])
        t = (C.c_float * (world * nc))(*[v for row in table for v in row])
        cost = (C.c_float * nc)()
        va = None if valid is None else (C.c_int * nc)(*valid)
        return L.k5_sp_pick_schedule(t, nc, world, va, cost), list(cost)

    # 4 ranks, 3 candidates: candidate 1 is fastest on three ranks but one rank is slow on it -> candidate 2 wins on the max
    best, cost = pick([[2.0, 1.0, 1.5], [2.0, 1.0, 1.4], [2.1, 3.0, 1.6], [2.0, 1.0, 1.5]])
    assert best == 2 and cost == pytest.approx([2.1, 3.0, 1.6])
    assert pick([[1.0, 1.0], [1.0, 1.0]])[0] == 0                                   # tie: the lower index
    assert pick([[2.0, -1.0], [2.0, 0.5]])[0] == 0                                  # candidate 1 did not run on rank 0
    assert pick([[2.0, float("nan")], [2.0, 0.5]])[0] == 0 and pick([[2.0, math.inf], [2.0, 0.5]])[0] == 0
    assert pick([[2.0, 0.5], [2.0, 0.5]], valid=[1, 0])[0] == 0                     # masked
    best, cost = pick([[-1.0, 0.0]])
    assert best == -1 and cost == [-1.0, -1.0]
    assert L.k5_sp_pick_schedule(None, 2, 2, None, None) == -1


def test_engine_rejects_bad_config_without_gpu(built_lib):
    """k5_dit_create validates on the host (no GPU work): head_dim must be 64."""
    import ctypes as C
    from kandinsky import _engine as E
    cc = E.DitConfig(16, 96, 48, 64, 16, (C.c_int * 3)(1, 2, 2), 128, 256, 1, 2, (C.c_int * 3)(16, 16, 16), 1)
    h = C.c_void_p()
    st = E.lib().k5_dit_create(C.byref(cc), C.byref(h))
    assert st != 0 and "head_dim" in E.last_error()
    cc = E.DitConfig(16, 96, 48, 64, 16, (C.c_int * 3)(1, 2, 2), 128, 256, 1, 2, (C.c_int * 3)(16, 24, 24), 1)
    assert E.lib().k5_dit_create(C.byref(cc), C.byref(h)) == 0
    # unknown key is rejected before any device work
    shape = (C.c_int64 * 1)(4)
    buf = (C.c_float * 4)()
    assert E.lib().k5_dit_load_tensor(h, b"not.a.key", buf, 0, shape, 1) == 5
    assert E.lib().k5_dit_missing_keys(h) > 0
    E.lib().k5_dit_destroy(h)


def test_step_update_entries_refuse_without_gpu(built_lib):
    """The three entries of the sampler's update share one launcher and one set of refusals: a NULL img, a NULL v_cond and a keep mask without
    its source are K5_ERR_ARG before any HIP call.  The pointers are host memory: a refusal never reads them, and nothing here may launch."""
    import ctypes as C
    from kandinsky import _engine as E
    L = E.lib()
    buf = [C.create_string_buffer(64) for _ in range(6)]
    img, vc, vu, ab, noise, mask = (C.addressof(b) for b in buf)
    cfg = lambda img, vc: L.k5_cfg_euler(img, vc, vu, 5.0, -0.0625, 8, None)
    edit = lambda img, vc, m=None: L.k5_cfg_euler_edit(img, vc, vu, 5.0, -0.0625, None, noise, m, 0.5, 4, 2, None)
    guided = lambda img, vc, m=None: L.k5_guided_euler(img, vc, vu, ab, -0.0625, None, noise, m, 0.5, 4, 2, None, None)
    for entry in (cfg, edit, guided):
        assert entry(None, vc) == 1 and entry(img, None) == 1
    assert edit(img, vc, mask) == 1 and guided(img, vc, mask) == 1
    assert "k5_guided_euler: need img, v_cond, v_uncond and ab" in E.last_error()


def test_state_dict_layout_matches_reference_manifest():
    from kandinsky.models.dit import DiffusionTransformer3D
    from oracle import k5_oracle as O
    with open(os.path.join(ROOT, "tests", "golden", "dit_lite_manifest.json")) as f:
        ref = json.load(f)
    with torch.device("meta"):
        dit = DiffusionTransformer3D(**O.LITE_2B)
    sd = dit.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k, v in sd.items():
        assert list(v.shape) == ref[k], k
    assert sum(v.numel() for v in sd.values()) == sum(int(torch.tensor(s).prod()) for s in ref.values())
    assert dit.visual_cond is True and dit.visual_transformer_blocks[0].self_attention.num_heads == 28


def test_load_state_dict_assign_and_no_cpu_fallback(tiny_sd, golden_meta, golden):
    from kandinsky.models.dit import DiffusionTransformer3D
    c = dict(golden_meta["tiny_config"])
    dit = DiffusionTransformer3D(**c)
    dit.load_state_dict(tiny_sd, assign=True)
    assert torch.equal(dit.state_dict()["out_layer.out_layer.weight"], tiny_sd["out_layer.out_layer.weight"])
    pos = [torch.arange(3), torch.arange(4), torch.arange(6)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dit(golden["fwd.x"], golden["fwd.text"], golden["fwd.pooled"], golden["fwd.time"], pos, torch.arange(7))
    with pytest.raises(RuntimeError, match="parameter container"):
        dit.visual_transformer_blocks[0].feed_forward(golden["op.ssn.x"])


def test_missing_library_fails_loudly():
    code = ("import os, sys; sys.path.insert(0, %r); os.environ['K5_LIB']='/nonexistent/libk5.so';"
            "from kandinsky import _engine as E\n"
            "try:\n E.lib()\nexcept RuntimeError as e:\n print('LOUD', e)\n") % PKG
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert "LOUD" in out.stdout and "no fallback" in out.stdout, out.stdout + out.stderr


def test_config_loader_matches_reference_parse(tmp_path):
    from kandinsky.config import load_config, write_default_configs
    with open(os.path.join(ROOT, "tests", "golden", "configs_parsed.json")) as f:
        ref = json.load(f)
    cdir = str(tmp_path / "configs")
    write_default_configs(cdir)
    assert sorted(os.listdir(cdir)) == sorted(ref.keys())
    for fn, parsed in ref.items():
        conf = load_config(os.path.join(cdir, fn))
        assert conf.to_dict() == parsed, fn
        assert conf.model.dit_params.patch_size == [1, 2, 2]
        assert conf.model.attention.type in ("flash", "nabla")
        assert conf["metrics"]["scale_factor"] == [1.0, 2.0, 2.0]


def test_sigma_schedule_host():
    from kandinsky.generation_utils import sigma_schedule
    from oracle import k5_oracle as O
    for n, s in ((4, 5.0), (50, 5.0), (100, 10.0)):
        assert torch.equal(sigma_schedule(n, s), O.sigma_schedule(n, s))
    assert torch.allclose(sigma_schedule(4, 5.0), torch.tensor([1, .9375, .8333333, .625, 0]), atol=1e-6)


def test_magcache_ratio_table_matches_reference_goldens():
    """Host mirror of set_magcache_params' table preparation (reference magcache_utils.py:6-13,28-39) against the tables
    the reference derived (tests/golden/magcache_tiny.safetensors, made by oracle/gen_golden_magcache.py)."""
    import json
    from safetensors.torch import load_file
    from kandinsky.magcache_utils import ratio_table, nearest_interp
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    T = load_file(os.path.join(here, "magcache_tiny.safetensors"))
    for c in json.load(open(os.path.join(here, "magcache_meta.json")))["cases"]:
        t = ratio_table(c["ratios"], c["num_steps"])
        assert t.dtype == np.float64 and len(t) == 2 * c["num_steps"]
        assert np.array_equal(t, T[f"mag.{c['tag']}.table"].numpy()), c["tag"]
    assert np.array_equal(nearest_interp(np.arange(5.0), 1), np.array([4.0]))
    assert np.array_equal(nearest_interp(np.arange(5.0), 3), np.array([0.0, 2.0, 4.0]))


def test_cli_keeps_the_reference_flags():
    """kandinsky-5_amd/test.py: flags / defaults of the reference CLI (reference test.py:32-122) and its size check."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_cli", os.path.join(ROOT, "kandinsky-5_amd", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.build_parser().parse_args([])
    assert (a.config, a.prompt, a.width, a.height, a.video_duration, a.expand_prompt, a.sample_steps, a.guidance_weight,
            a.scheduler_scale, a.output_filename, a.offload, a.magcache) == \
        ("./configs/config_5s_sft.yaml", "a cat in a blue hat", 768, 512, 5, 1, None, None, 5.0, "./test.mp4", False, False)
    a = cli.build_parser().parse_args(["--local-rank", "3", "--magcache", "--width", "512", "--height", "512"])
    assert a.local_rank == 3 and a.magcache
    cli.validate_args(a)
    a.width, a.height = 768, 768
    with pytest.raises(NotImplementedError):
        cli.validate_args(a)


def test_package_surface_used_by_the_reference_comfyui_nodes_and_cli():
    """Drop-in seams: every name the reference's comfyui/nodes_kandinsky.py:3-7,26,49-52,98-99,102-106,131 and
    test.py:8,131-151 import or call exists here with a compatible call shape."""
    import inspect
    import kandinsky
    from kandinsky import get_T2V_pipeline
    from kandinsky.generation_utils import generate, generate_sample, get_velocity, get_sparse_params
    from kandinsky.models.dit import get_dit, DiffusionTransformer3D
    from kandinsky.models.text_embedders import Kandinsky5TextEmbedder, get_text_embedder
    from kandinsky.models.vae import build_vae, AutoencoderKLHunyuanVideo
    from kandinsky.magcache_utils import set_magcache_params
    from kandinsky.t2v_pipeline import Kandinsky5T2VPipeline
    assert kandinsky.get_T2V_pipeline is get_T2V_pipeline
    p = inspect.signature(get_T2V_pipeline).parameters
    assert list(p)[:1] == ["device_map"] and {"conf_path", "offload", "magcache", "cache_dir", "dit_path", "vae_path"} <= set(p)
    g = list(inspect.signature(generate).parameters)
    assert g[:12] == ["model", "device", "shape", "num_steps", "text_embeds", "null_text_embeds", "visual_rope_pos", "text_rope_pos",
                      "null_text_rope_pos", "guidance_weight", "scheduler_scale", "conf"]
    assert list(inspect.signature(Kandinsky5TextEmbedder.__init__).parameters)[:3] == ["self", "conf", "device"]
    for name in ("encode", "to"):
        assert callable(getattr(Kandinsky5TextEmbedder, name))
    c = inspect.signature(Kandinsky5T2VPipeline.__call__).parameters
    assert {"time_length", "width", "height", "num_steps", "guidance_weight", "scheduler_scale", "expand_prompts", "save_path",
            "seed", "negative_caption"} <= set(c)
    # get_dit(conf.model.dit_params) -> .to(device=) -> .load_state_dict(sd) (no assign=) ; attributes touched by callers
    with torch.device("meta"):
        dit = get_dit(dict(in_visual_dim=16, out_visual_dim=16, time_dim=64, patch_size=(1, 2, 2), model_dim=128, ff_dim=256,
                           num_text_blocks=1, num_visual_blocks=1, axes_dims=(16, 24, 24), visual_cond=True, in_text_dim=96,
                           in_text_dim2=48))
    assert isinstance(dit, DiffusionTransformer3D) and dit.visual_cond is True
    for attr in ("visual_transformer_blocks", "text_transformer_blocks", "time_embeddings", "text_embeddings",
                 "pooled_text_embeddings", "visual_embeddings", "out_layer"):
        assert hasattr(dit, attr), attr
    assert "assign" in inspect.signature(dit.load_state_dict).parameters
    with torch.device("meta"):
        vae = AutoencoderKLHunyuanVideo()
    assert hasattr(vae, "decode") and hasattr(vae.config, "scaling_factor") and callable(vae.eval)
    assert callable(build_vae) and callable(get_text_embedder) and callable(set_magcache_params)
    assert callable(generate_sample) and callable(get_velocity) and callable(get_sparse_params)


def test_default_configs_equal_the_reference_configs_and_materialise(tmp_path):
    """kandinsky/default_configs.json == the parsed reference YAMLs (tests/golden/configs_parsed.json, G10); a missing default
    config path is written on first load."""
    from kandinsky.config import default_configs, load_config, DEFAULT_CONFIG_NAMES
    with open(os.path.join(ROOT, "tests", "golden", "configs_parsed.json")) as f:
        ref = json.load(f)
    assert default_configs() == ref and set(DEFAULT_CONFIG_NAMES) == set(ref)
    conf = load_config(str(tmp_path / "configs" / "config_10s_sft.yaml"))
    assert conf.model.attention.type == "nabla" and conf.model.num_steps == 50 and len(conf.magcache.mag_ratios) == 98
    assert conf.to_dict() == ref["config_10s_sft.yaml"]
    assert sorted(os.listdir(tmp_path / "configs")) == sorted(DEFAULT_CONFIG_NAMES)


def test_hot_kernels_keep_their_register_budget():
    """The hand-scheduled kernels live or die by their register allocation: an innocent source edit once sent the 256
    accumulators of the 4-wave GEMM to scratch (2416 B/lane, 40x slower, every parity test still green).  build.py records
    the compiler's per-kernel resource report; this pins the budgets the performance numbers in DESIGN.md rest on."""
    import json
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    if not os.path.exists(b.RESOURCES):
        b.build(force=True, verbose=False)
    res = json.load(open(b.RESOURCES))

    def kernels(tag):
        ks = {k: v for k, v in res.items() if tag in k}
        assert ks, tag
        return ks
    import re
    for k, v in kernels("gemm_bf16_w4_kernel").items():       # 32 MT accumulators in AGPRs (MT = 8 / 6 / 4 token tiles per wave), one wave per SIMD
        mt = int(re.search(r"ILi\d+ELi(\d+)E", k).group(1))
        assert 32 * mt <= v["AGPRs"] <= min(256, 32 * mt + 8) and v["ScratchSize [bytes/lane]"] <= 64 and v["VGPRs Spill"] <= 12, (k, v)   # (the few spilled dwords sit in the prologue / epilogue, none inside the MFMA stream: checked on the ISA)
    for k, v in kernels("conv3d_w4_kernel").items():
        assert v["ScratchSize [bytes/lane]"] <= 128, (k, v)
    for k, v in kernels("attn_fwd_kernelILb1E").items():        # fixed-offset forms: two workgroups per CU
        cap = 256 if ("ELi4ELi4ELb" in k or k.endswith("ELb1EEEvNS_5AttnPE")) else 128   # 64-row waves (opt-in): two waves per SIMD by design; the pipelined forms (opt-in, last flag): one or two
        assert v["VGPRs"] <= cap and v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
    for k, v in kernels("attn_fwd_kernelILb0E").items():        # online-max forms: no spills at their (larger) budget
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
    for k, v in kernels("attn_fwd32_kernel").items():
        assert v["VGPRs"] <= 128 and v["VGPRs Spill"] == 0, (k, v)
    for k, v in kernels("nabla_select_row_kernel").items():     # one row per wave: >= 4 waves per SIMD hide the DPP reductions; the few
        assert v["VGPRs"] <= 128 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] <= 32, (k, v)   # spilled dwords sit outside the bisection loop


def test_gemm_accumulators_stay_invisible_to_the_compiler():
    """Round 6: the four-wave GEMM keeps its accumulators in PHYSICAL AGPRs that only its own asm statements name (a[4 q : 4 q + 3] in the MFMA text,
    v_accvgpr_read in the epilogue) — the register allocator never sees them, which is
    what lets a second consumer of the accumulators exist at all (rounds 2-5: 150-500 spilled registers).  That only works while the COMPILER never
    touches an AGPR of its own accord (a VGPR spilled into the AGPR file would land on an accumulator).  This compiles the kernel to ISA and demands:
    no AGPR mentioned outside an inline-asm block, every MFMA of a kernel on its own quads with C = 0 or C = D, all 8 MT quads read back by the epilogue."""
    import re
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(PKG, "csrc", "gemm_bf16.hip")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(PKG, "csrc"), "-fno-slp-vectorize", "-Wno-unused-result", "--cuda-device-only", "-S", src, "-o", "-"],
                         check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^(_Z\w*gemm_bf16_w4_kernel\w*):", line)
        if m:
            cur = m.group(1); kernels[cur] = []
        elif cur and line.startswith(".Lfunc_end"):
            cur = None
        elif cur:
            kernels[cur].append(line.strip())
    assert len(kernels) == 13, sorted(kernels)            # 4 epilogues x 3 tile heights + the fp32-score form
    for k, body in kernels.items():
        mt = int(re.search(r"ILi\d+ELi(\d+)E", k).group(1))
        inasm, stray, mfma, reads = False, [], [], set()
        for t in body:
            if "ASMSTART" in t:
                inasm = True
            elif "ASMEND" in t:
                inasm = False
            elif t.startswith(";") or not t:
                continue
            elif not inasm and re.search(r"\ba\d+\b|\ba\[", t):
                stray.append(t)
            elif inasm:
                m = re.match(r"v_mfma_f32_16x16x32_bf16 a\[(\w+):(\w+)\], v\[\d+:\d+\], v\[\d+:\d+\], (\S+)", t)
                if m:
                    mfma.append((int(m.group(1), 0), int(m.group(2), 0), m.group(3)))
                m = re.match(r"v_accvgpr_read_b32 v\d+, a\[(\w+)\]", t)
                if m:
                    reads.add(int(m.group(1), 0))
        assert not stray, (k, stray[:3])
        assert len(mfma) == 4 * 16 * mt, (k, len(mfma))                     # four K-tile bodies (two stages x first / steady) of 16 MT MFMAs
        assert {lo for lo, _, _ in mfma} == {4 * q for q in range(8 * mt)} and all(hi == lo + 3 for lo, hi, _ in mfma), k
        assert all(c == "0" or re.fullmatch(r"a\[(\w+):(\w+)\]", c) and int(re.fullmatch(r"a\[(\w+):(\w+)\]", c).group(1), 0) == lo for lo, _, c in mfma), k
        assert reads == set(range(32 * mt)), (k, len(reads))


def test_attention_tile_prefetch_survives_the_compiler():
    """The attention kernels issue the DMA of key tile e+1 at the top of tile e and drain it (`s_waitcnt vmcnt(0)`) just before the
    barrier that ends the tile.  Nothing in the source pins that distance: the compiler places the wait, and it moved it right behind the
    DMA twice — a static LDS variable next to the tile buffers (__syncthreads_or), and an int atomic ahead of the loop (the NABLA list
    loads became vector loads whose wait drains the DMA) — 6-14 % on the whole kernel with every parity test green.  This compiles the
    kernel to ISA and demands >= 24 MFMAs between every in-loop tile DMA and the next vmcnt(0), for the forms the engine runs."""
    import re
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(PKG, "csrc", "attn_fwd.hip")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(PKG, "csrc"), "-fno-slp-vectorize", "-Wno-unused-result", "--cuda-device-only", "-S", src, "-o", "-"],
                         check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^(_Z\w*attn_fwd_kernel\w*):", line)
        if m:
            cur = m.group(1); kernels[cur] = []
        elif cur and line.startswith(".Lfunc_end"):
            cur = None
        elif cur:
            kernels[cur].append(line.strip())

    def mfma_before_drain(body, pick):
        """basic blocks + successors; from every in-loop block that issues tile DMAs: the MFMAs on the way to the next vmcnt(0) —
        pick = min over the paths (dense), max (NABLA: a wave whose 64-query block did not select the tile skips its MFMAs by design)"""
        blocks, order = {"entry": {"ins": [], "loop": False}}, ["entry"]
        for t in body:
            m = re.match(r"^(\.LBB\d+_\d+):", t)
            if m:
                blocks[m.group(1)] = {"ins": [], "loop": "in Loop" in t}; order.append(m.group(1))
            elif t and not t.startswith((";", ".")):
                blocks[order[-1]]["ins"].append(t)
        for i, name in enumerate(order):
            ins = blocks[name]["ins"]
            succ = [x.split()[-1] for x in ins if x.startswith("s_cbranch")]
            if ins and ins[-1].startswith("s_branch"):
                succ.append(ins[-1].split()[-1])
            elif not (ins and ins[-1].startswith("s_endpgm")) and i + 1 < len(order):
                succ.append(order[i + 1])
            blocks[name]["succ"] = succ

        def walk(name, start, seen):
            n = 0
            for t in blocks[name]["ins"][start:]:
                if "vmcnt(0)" in t:
                    return n
                n += "mfma" in t
            nxt = [walk(s_, 0, seen | {s_}) for s_ in blocks[name]["succ"] if s_ not in seen and s_ in blocks]
            return n + (pick(nxt) if nxt else 10 ** 6)
        res = []
        for name in order:
            ins = blocks[name]["ins"]
            dma = [i for i, t in enumerate(ins) if "lds" in t and t.startswith(("buffer_load", "global_load"))]
            if dma and blocks[name]["loop"]:
                res.append(walk(name, dma[-1] + 1, {name}))
        return res
    # <BOUNDED, SPARSE, RANGE, PRE, QN, GR>: dense fixed / online, the same with the fused query norm, NABLA fixed: one launch, one pass of
    # the sharded schedule, 128-query workgroups (all on pre-scaled keys)
    # (round 4: the last parameter is GR, the 64-query rows per list — 4: 256-query workgroups, 2: 128, 1: 64)
    # (the parameter after GR is QT, the 16-query tiles per wave: 2 everywhere, 4 = the opt-in 64-row-wave form of the dense fixed-offset launch)
    for tag, pick in (("ILb1ELb0ELb1ELb1ELb0ELi4ELi2E", min), ("ILb0ELb0ELb1ELb1ELb0ELi4ELi2E", min), ("ILb1ELb0ELb1ELb1ELb1ELi4ELi2E", min),
                      ("ILb0ELb0ELb1ELb1ELb1ELi4ELi2E", min), ("ILb1ELb1ELb0ELb1ELb0ELi4ELi2E", max), ("ILb1ELb1ELb1ELb1ELb0ELi4ELi2E", max),
                      ("ILb1ELb1ELb0ELb1ELb0ELi2ELi2E", max), ("ILb1ELb1ELb0ELb1ELb0ELi1ELi2E", max), ("ILb1ELb0ELb1ELb1ELb0ELi4ELi4E", min)):
        need = 24
        body = [v for k, v in kernels.items() if tag + "Lb0EEEv" in k]       # the shipped forms (last flag: the opt-in software-pipelined variants of round 5, not pinned)
        assert len(body) == 1, tag
        dist = mfma_before_drain(body[0], pick)
        assert len(dist) >= 2 and min(dist) >= need, (tag, dist)      # both halves of the unrolled tile loop


def test_committed_bench_line_keeps_the_contract():
    """profiles/r02_bench.json is the JSON line `python bench.py` printed on an MI355X at the end of the round: the keys the driver
    reads (task statement, bench.py contract) and the two blocks this tier adds must all be there and consistent with each other."""
    import json
    d = json.load(open(os.path.join(ROOT, "profiles", "r02_bench.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "steps/s" and d["higher_is_better"] is True and d["dtype"] == "bf16" and d["data"] == "synthetic" and d["n_gpus"] == 1
    assert "workload" in d["config"] and "INVALID_AS_BENCH" not in d
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-6                       # value = steps / time
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert abs(r["achieved"] - r["flop_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e12) < 1e-6 * r["achieved"]
    assert r["traffic"] is None or r["traffic"] > 4 * 47616 * 28 * 64 * 2                 # HBM-side bytes >= the algorithmic ones
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    # round 4: the line also carries the check of the TIMED configuration against the reference's generate() at full size and the latent pin
    d4 = json.load(open(os.path.join(ROOT, "profiles", "r04_bench.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "roofline_gemm", "cpu_baseline", "parity_check", "latent_pin"):
        assert k in d4, k
    assert d4["dtype"] == "bf16" and "INVALID_AS_BENCH" not in d4 and d4["config"]["visual_blocks"] == 32
    pc = d4["parity_check"]
    assert pc["status"] == "ok" and len(pc["steps"]) == 2 and all(st["rel_l2_update"] <= pc["tolerance_rel_l2_update"] for st in pc["steps"])
    assert d4["latent_pin"]["status"] == "ok"
    r4 = d4["roofline"]
    assert r4["kernel"].startswith("attn_fwd_kernel") and abs(r4["frac"] - r4["achieved"] / r4["peak"]) < 1e-9 and r4["blocks_run"] == 32 * d4["steps"]
    assert "16 torch threads" in d4["cpu_baseline"]["sample"] or "torch threads" in d4["cpu_baseline"]["sample"]
