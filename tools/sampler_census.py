"""What the sampler enqueues, counted by the engine's own profile: the launches of every kernel family after one `generate` of 4 steps on the
tiny model of tests/golden/dit_tiny.safetensors at the golden shape (3, 8, 12, 16), in nine modes of the in-engine loop.  Bit-identity of the
latent does not catch a launch that was enqueued twice or a per-call reset that moved; these counts do.  Profiling turns graph replay off, so
this is the eager loop.  Public Python API only: the same script runs on any commit that has the nine modes.

    python tools/sampler_census.py [--write]      (--write: tests/golden/sampler_census.json, what tests/test_gpu_census.py asserts)
"""
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
         "regions_B_w5_per_block_kv")
STEPS, HW = 4, (8, 12, 16)
FLASH = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))


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
    raise KeyError(mode)


def census(dit, g, mode):
    """{family: launches} of one `generate` in `mode`"""
    from kandinsky.generation_utils import generate
    noise, w, kw = mode_keywords(mode, g)
    te = {"text_embeds": g["fwd.text"].cuda(), "pooled_embed": g["fwd.pooled"].cuda()}
    ne = {"text_embeds": g["gen.null_text"].cuda(), "pooled_embed": g["gen.null_pooled"].cuda()}
    pos = [torch.arange(3), torch.arange(HW[0] // 2), torch.arange(HW[1] // 2)]
    dit.engine(torch.device("cuda", 0))
    dit.set_profiling(True)
    per_block_kv = mode.endswith("_per_block_kv")   # every visual block projects its own cross-attention keys / V^T
    try:
        if per_block_kv:
            dit.set_option("cross_kv_batched", 0)
        dit.reset_profile()
        generate(dit, "cuda:0", tuple(noise.shape), STEPS, te, ne, pos, torch.arange(7), torch.arange(4), w, 5.0, FLASH, noise=noise, **kw)
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
