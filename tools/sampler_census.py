"""What the sampler enqueues, counted by the engine's own profile: the launches of every kernel family after one `generate` of 4 steps on the
tiny model of tests/golden/dit_tiny.safetensors at the golden shape (3, 8, 12, 16), in the modes of the in-engine loop listed in MODES: nine
of the sampler's own, then nine that reach the parts of the engine's forward the first nine never do (NABLA's token order alone and with
Enhance-A-Video, which needs both token-order tables, at (3, 16, 16, 16), the smallest shape NABLA takes; the forking forward of skip-layer
guidance in both modes; Enhance-A-Video dense; MagCache skipping and running; MagCache calibration; visual conditioning).  Bit-identity of the
latent does not catch a launch that was enqueued twice or a per-call reset that moved; these counts do.  Profiling turns graph replay off, so
this is the eager loop.  Public Python API only: the same script runs on any commit that has the modes.

    python tools/sampler_census.py [--write]      (--write: tests/golden/sampler_census.json, what tests/test_gpu_census.py asserts)
"""
import contextlib
import json
import os
import sys
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kandinsky-5_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CENSUS = os.path.join(GOLDEN, "sampler_census.json")
FAMILIES = ("elementwise", "gemm", "attn_self", "attn_cross", "nabla_map", "prologue", "epilogue", "comm", "attn_text")
MODES = ("plain_w1", "plain_w5", "edit_mask_w5", "windows_t6_w5", "watch_preview_x0_w5", "nag_A_w1", "regions_B_w5", "nag_regions_w1",
         "regions_B_w5_per_block_kv", "nabla_w5", "nabla_enhance_A_w5", "skip_block_w5", "skip_attention_interval_w5", "enhance_A_w5",
         "magcache_hand_w2", "magcache_calibrate_w2", "visual_cond_w5")
STEPS, HW = 4, (8, 12, 16)
NABLA_HW = (16, 16, 16)   # the smallest latent whose H and W are divisible by 16: one 8 x 8 token tile per frame
FLASH = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))


def meta(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def mode_conf(mode):
    """the `conf` of a mode's `generate`: NABLA attention with the `nabla_attention` block of dit_tiny_meta.json, dense otherwise"""
    if not mode.startswith("nabla_"):
        return FLASH
    return NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(**meta("dit_tiny_meta.json")["nabla_attention"])),
              metrics=NS(scale_factor=(1.0, 2.0, 2.0)))


def tiny_model(device="cuda:0"):
    from safetensors.torch import load_file
    from kandinsky.models.dit import DiffusionTransformer3D
    g = load_file(os.path.join(GOLDEN, "dit_tiny.safetensors"))
    cfg = dict(json.load(open(os.path.join(GOLDEN, "dit_tiny_meta.json")))["tiny_config"])
    dit = DiffusionTransformer3D(**cfg)
    dit.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")}, assign=True)
    return dit.to(device), g


def mode_keywords(mode, g):
    """(noise, guidance, keywords of `generate`) of a mode"""
    rnd = torch.Generator().manual_seed(11)
    if mode == "plain_w1":
        return g["gen.noise"], 1.0, {}
    if mode == "plain_w5":
        return g["gen.noise"], 5.0, {}
    if mode == "edit_mask_w5":
        src = torch.randn(3, *HW, generator=rnd)
        return g["gen.noise"], 5.0, dict(init_latent=src, keep_mask=(torch.rand(3, *HW[:2], 1, generator=rnd) > 0.5).float())
    if mode == "windows_t6_w5":
        plan = json.load(open(os.path.join(GOLDEN, "dit_tiny_windows_meta.json")))["cases"]["t6"]
        noise = torch.randn(plan["T"], *HW, generator=torch.Generator().manual_seed(plan["seed"]))
        return noise, 5.0, dict(context_frames=plan["frames"], context_overlap=plan["overlap"])
    if mode == "watch_preview_x0_w5":
        factors = ((torch.rand(16, 3, generator=rnd) - 0.5) * 0.5, torch.zeros(3))
        return g["gen.noise"], 5.0, dict(callback=lambda info: False, preview_every=1, preview_factors=factors, preview_x0=True)
    nag, regions = {}, {}
    if mode in ("nag_A_w1", "nag_regions_w1"):
        sets = json.load(open(os.path.join(GOLDEN, "dit_tiny_nag_meta.json")))["sets"]["A"]
        neg = {"text_embeds": g["gen.null_text"].cuda(), "pooled_embed": g["gen.null_pooled"].cuda()}
        nag = dict(nag_text_embeds=neg, nag_text_rope_pos=torch.arange(4), nag_scale=sets["scale"], nag_tau=sets["tau"], nag_alpha=sets["alpha"])
    if mode in ("regions_B_w5", "nag_regions_w1", "regions_B_w5_per_block_kv"):
        from safetensors.torch import load_file
        rg = load_file(os.path.join(GOLDEN, "dit_tiny_regions.safetensors"))
        regions = dict(region_text_embeds=[{"text_embeds": rg["regions.text0"].cuda()}, {"text_embeds": rg["regions.text1"].cuda()}],
                       region_text_rope_pos=[torch.arange(5), torch.arange(6)], region_masks=rg["regions.B.masks"].contiguous(),
                       region_base_weight=0.5)
    if mode in ("nag_A_w1", "nag_regions_w1"):
        return g["gen.noise"], 1.0, {**nag, **regions}
    if mode in ("regions_B_w5", "regions_B_w5_per_block_kv"):   # guidance 5: the unconditional forwards, which must not grow, are counted too
        return g["gen.noise"], 5.0, regions
    enhance = dict(enhance_weight=meta("dit_tiny_enhance_meta.json")["sets"]["A"]["weight"])
    if mode in ("nabla_w5", "nabla_enhance_A_w5"):
        return torch.randn(3, *NABLA_HW, generator=rnd), 5.0, enhance if mode == "nabla_enhance_A_w5" else {}
    if mode == "enhance_A_w5":
        return g["gen.noise"], 5.0, enhance
    if mode in ("skip_block_w5", "skip_attention_interval_w5"):   # the tiny model has two visual blocks: the second is skipped, the first is the shared prefix
        case = meta("dit_tiny_skip_meta.json")["cases"]["block_mid" if mode == "skip_block_w5" else "attention_interval"]
        kw = dict(slg_blocks=[1], slg_scale=case["g"], slg_mode=case["mode"])
        if "interval" in case:   # of the 4 steps' sigmas 1, .9375, .833, .625 three lie inside: steps that fork and one that does not
            kw["slg_interval"] = tuple(case["interval"])
        return g["gen.noise"], case["w"], kw
    if mode == "magcache_hand_w2":
        return g["gen.noise"], [c for c in meta("magcache_meta.json")["cases"] if c["tag"] == "hand_10"][0]["guidance_weight"], {}
    if mode == "magcache_calibrate_w2":
        return g["gen.noise"], [c for c in meta("magcache_calib_tiny.json")["cases"] if c["tag"] == "cfg"][0]["guidance_weight"], {}
    if mode == "visual_cond_w5":
        return g["gen.noise"], 5.0, dict(visual_cond=torch.randn(3, *HW, generator=rnd).cuda(),
                                         visual_cond_mask=(torch.rand(3, *HW[:2], 1, generator=rnd) > 0.5).float().cuda())
    raise KeyError(mode)


@contextlib.contextmanager
def mode_handle(dit, mode):
    """what a mode sets on the model around its `generate` and takes back after it"""
    from kandinsky import magcache_utils as M
    if mode == "magcache_hand_w2":
        # the hand-made table of magcache_meta.json, re-sampled to the 4 steps: [1, 1, .97, .96, 1, .99, .99, .98].  The reference's retention of
        # 0.2 would let call 1 of 8 decide before its slot has a residual, so the first half of the run is retained: calls 0..3 run, 4..7 skip
        M.set_magcache_params(dit, [c for c in meta("magcache_meta.json")["cases"] if c["tag"] == "hand_10"][0]["ratios"], STEPS, False)
        dit.retention_ratio = 0.5
        M._apply(dit)
        try:
            yield
            assert M.magcache_state(dit)[1:] == (4, 4), M.magcache_state(dit)
        finally:
            M.disable_magcache(dit)
    elif mode == "magcache_calibrate_w2":
        M.start_magcache_calibration(dit, STEPS, False)
        try:
            yield
        finally:
            M.stop_magcache_calibration(dit)
    else:
        yield


def census(dit, g, mode):
    """{family: launches} of one `generate` in `mode`"""
    from kandinsky.generation_utils import generate
    noise, w, kw = mode_keywords(mode, g)
    te = {"text_embeds": g["fwd.text"].cuda(), "pooled_embed": g["fwd.pooled"].cuda()}
    ne = {"text_embeds": g["gen.null_text"].cuda(), "pooled_embed": g["gen.null_pooled"].cuda()}
    pos = [torch.arange(3), torch.arange(noise.shape[1] // 2), torch.arange(noise.shape[2] // 2)]
    dit.engine(torch.device("cuda", 0))
    dit.set_profiling(True)
    per_block_kv = mode.endswith("_per_block_kv")   # every visual block projects its own cross-attention keys / V^T
    try:
        if per_block_kv:
            dit.set_option("cross_kv_batched", 0)
        with mode_handle(dit, mode):
            dit.reset_profile()
            generate(dit, "cuda:0", tuple(noise.shape), STEPS, te, ne, pos, torch.arange(7), torch.arange(4), w, 5.0, mode_conf(mode), noise=noise, **kw)
            torch.cuda.synchronize()
        return {f: dit.get_profile(f)[1] for f in FAMILIES}
    finally:
        if per_block_kv:
            dit.set_option("cross_kv_batched", 1)
        dit.set_profiling(False)


def main():
    dit, g = tiny_model()
    counts = {mode: census(dit, g, mode) for mode in MODES}
    print(json.dumps(counts), flush=True)
    if "--write" in sys.argv[1:]:
        with open(CENSUS, "w") as f:
            json.dump(counts, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
