"""Command-line entry point — same flags and defaults as the reference's test.py (reference test.py:32-147) so that the
README launch lines keep working against this package:

    python test.py --prompt "a cat in a blue hat" --config ./configs/config_5s_sft.yaml
    python test.py --prompt "the cat turns its head" --image cat.png     # image-to-video: the clip starts from cat.png
    python test.py --prompt "the same street at night" --video clip.mp4 --strength 0.6 --mask keep.png   # video-to-video, masked
    python test.py --prompt "a dog on a sofa" --video clip.mp4 --source_prompt "a cat on a sofa" --strength 0.7   # FlowEdit
    python test.py --config ./configs/config_5s_distil.yaml --calibrate_magcache ratios.json   # measure a MagCache table, then:
    python test.py --config ./configs/config_5s_distil.yaml --magcache --magcache_ratios ratios.json
    python test.py --prompt "a cat in a blue hat" --lora style.safetensors --lora_scale 0.8   # LoRA adapter(s) merged into the DiT
    python test.py --fit_preview_factors factors.json                      # fit latent -> RGB preview factors from one generation, then:
    python test.py --preview ./steps --preview_every 5 --preview_factors factors.json   # a PNG of the denoised estimate every 5 steps
    PYTHONPATH=. torchrun --nproc-per-node 8 --master-addr 127.0.0.1 test.py --config ./configs/config_10s_sft.yaml ...

Multi-GPU: one process per GPU (LOCAL_RANK / WORLD_SIZE from the launcher); `get_T2V_pipeline` sets up token-sharded
sequence parallelism (+ CFG-parallel rank groups, VAE tile distribution) over RCCL.
"""
import argparse
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SUPPORTED_SIZES = [(512, 512), (512, 768), (768, 512)]
NEGATIVE = ("Static, 2D cartoon, cartoon, 2d animation, paintings, images, worst quality, low quality, ugly, deformed, "
            "walking backwards")


class _Parser(argparse.ArgumentParser):
    """--width / --height take the trained sizes only, as they always did; the choice is lifted for a command line that has --tile, whose frame
    the pipeline checks (multiples of 16 that are at least the tile)."""
    size_actions = ()

    def parse_known_args(self, args=None, namespace=None):
        argv = sys.argv[1:] if args is None else list(args)
        tiled = any(a == "--tile" or a.startswith("--tile=") for a in argv)
        for action in self.size_actions:
            action.choices = None if tiled else [768, 512]
        return super().parse_known_args(args, namespace)


def build_parser():
    p = _Parser(description="Generate a video with Kandinsky 5 (MI355X engine)")
    p.add_argument("--local-rank", type=int, help="set by the launcher (one process per GPU)")
    p.add_argument("--config", type=str, default="./configs/config_5s_sft.yaml", help="YAML config (reference schema); a missing default name is created")
    p.add_argument("--prompt", type=str, default="a cat in a blue hat", help="text prompt")
    p.add_argument("--negative_prompt", type=str, default=NEGATIVE, help="negative prompt of the unconditional branch")
    p.size_actions = (p.add_argument("--width", type=int, default=768, choices=[768, 512], help="frame width in pixels; with --tile a larger multiple of 16"),
                      p.add_argument("--height", type=int, default=512, choices=[768, 512], help="frame height in pixels; with --tile a larger multiple of 16"))
    p.add_argument("--video_duration", type=int, default=5, help="clip length in seconds (0 = a single image)")
    p.add_argument("--expand_prompt", type=int, default=1, help="1 = rewrite the prompt with the Qwen2.5-VL chat model first")
    p.add_argument("--sample_steps", type=int, default=None, help="number of Euler steps (default: the config's)")
    p.add_argument("--guidance_weight", type=float, default=None, help="classifier-free guidance weight (default: the config's)")
    p.add_argument("--scheduler_scale", type=float, default=5.0, help="sigma-schedule scale s in s*t/(1+(s-1)*t)")
    p.add_argument("--output_filename", type=str, default="./test.mp4", help="output path (.mp4 / .avi / .png)")
    p.add_argument("--offload", action="store_true", default=False, help="keep only the active model on the GPU")
    p.add_argument("--image", type=str, default=None, help="image-to-video: a picture (PNG / JPEG) the clip starts from")
    p.add_argument("--magcache", action="store_true", default=False, help="MagCache: skip the visual blocks on low-error steps (50-step configs)")
    p.add_argument("--magcache_ratios", type=str, default=None, help="MagCache ratio table (JSON / YAML with mag_ratios) used instead of the config's; with --magcache")
    p.add_argument("--calibrate_magcache", type=str, default=None, metavar="OUT.json",
                   help="measure the MagCache ratio table of this checkpoint on the given prompt (and --image) and write it to OUT.json; no video is saved")
    # absent from the namespace unless given (argparse.SUPPRESS): the flags the reference's CLI has keep their exact set of defaults
    p.add_argument("--lora", action="append", default=argparse.SUPPRESS, metavar="FILE",
                   help="LoRA adapter (.safetensors; peft, diffusers or kohya names) merged into the DiT; repeat the flag for several")
    p.add_argument("--lora_scale", type=float, nargs="+", default=argparse.SUPPRESS, metavar="S",
                   help="adapter strength: one value for all --lora files or one per file (default 1.0)")
    p.add_argument("--video", type=str, default=argparse.SUPPRESS, metavar="PATH",
                   help="video-to-video: the source clip (container, animated PNG / GIF, .npy / .pt of uint8 frames, or a directory of images)")
    p.add_argument("--strength", type=float, default=argparse.SUPPRESS, metavar="S",
                   help="with --video: the part of the schedule that runs on the source, in (0, 1] (default 1.0 = only --mask ties the result to it)")
    p.add_argument("--mask", type=str, default=argparse.SUPPRESS, metavar="PATH",
                   help="with --video: keep mask (an image, or a clip as for --video); white = keep the source there, black = generate; "
                        "resized and centre-cropped to the output size like the frames of --video")
    p.add_argument("--fit_preview_factors", type=str, default=argparse.SUPPRESS, metavar="OUT.json",
                   help="fit the latent -> RGB factors of the live previews from one generation of the given prompt (its own latent and decoded "
                        "frames) and write them to OUT.json; no video is saved")
    p.add_argument("--preview", type=str, default=argparse.SUPPRESS, metavar="DIR",
                   help="write DIR/step_###.png, the middle frame of the denoised estimate, while sampling; needs --preview_factors")
    p.add_argument("--preview_every", type=int, default=argparse.SUPPRESS, metavar="K", help="with --preview: a picture every K steps and after the last (default 1)")
    p.add_argument("--preview_factors", type=str, default=argparse.SUPPRESS, metavar="FILE", help="with --preview: factors written by --fit_preview_factors")
    p.add_argument("--context_seconds", type=float, default=argparse.SUPPRESS, metavar="S",
                   help="a clip longer than the checkpoint's trained length: sample --video_duration as overlapping temporal windows of S seconds "
                        "(e.g. --video_duration 20 --context_seconds 10)")
    p.add_argument("--context_overlap_seconds", type=float, default=argparse.SUPPRESS, metavar="S",
                   help="with --context_seconds: how far neighbouring windows overlap (default a quarter of the window)")
    p.add_argument("--tile", type=int, nargs=2, default=argparse.SUPPRESS, metavar=("HEIGHT", "WIDTH"),
                   help="a frame larger than the checkpoint's trained size: sample --height x --width as overlapping spatial windows of HEIGHT x "
                        "WIDTH pixels, one of the trained sizes (e.g. --height 1024 --width 1024 --tile 512 768)")
    p.add_argument("--tile_overlap", type=int, default=argparse.SUPPRESS, metavar="PX",
                   help="with --tile: how far neighbouring windows overlap, a multiple of 16 pixels (default a quarter of the window)")
    p.add_argument("--nag_scale", type=float, default=argparse.SUPPRESS, metavar="S",
                   help="normalized attention guidance: --negative_prompt steers inside the cross-attention of the one forward (what makes it "
                        "count without classifier-free guidance); S >= 1, commonly 5 — a starting point, not tuned on these checkpoints")
    p.add_argument("--nag_tau", type=float, default=argparse.SUPPRESS, metavar="T", help="with --nag_scale: clamp on the growth of a token's L1 norm, >= 1 (default 2.5)")
    p.add_argument("--nag_alpha", type=float, default=argparse.SUPPRESS, metavar="A", help="with --nag_scale: blend of the guided output, in [0, 1] (default 0.25)")
    p.add_argument("--region", nargs=2, action="append", default=argparse.SUPPRESS, metavar=("PROMPT", "MASKFILE"),
                   help="regional prompt (repeatable, up to 8): PROMPT applies where MASKFILE (an image, or a clip as for --video) is white; "
                        "--prompt is the base prompt and holds alone where no mask reaches")
    p.add_argument("--region_base_weight", type=float, default=argparse.SUPPRESS, metavar="W",
                   help="with --region: weight of --prompt under the regions, in [0, 1] (default 0)")
    p.add_argument("--guidance_schedule", type=float, nargs="+", default=argparse.SUPPRESS, metavar="W",
                   help="a guidance weight per sampling step (as many values as steps); a step of weight 1 runs the conditional forward alone")
    p.add_argument("--guidance_interval", type=float, nargs=2, default=argparse.SUPPRESS, metavar=("LO", "HI"),
                   help="guide only on the steps whose sigma lies in [LO, HI] (weight 1, one forward, elsewhere)")
    p.add_argument("--cfg_zero_star", action="store_true", default=argparse.SUPPRESS,
                   help="CFG-Zero*: scale the unconditional velocity by its projection on the conditional one, per sample")
    p.add_argument("--cfg_zero_init", type=int, default=argparse.SUPPRESS, metavar="K", help="CFG-Zero* zero-init: the first K steps leave the latent as it is")
    p.add_argument("--cfg_rescale", type=float, default=argparse.SUPPRESS, metavar="PHI",
                   help="CFG rescale: pull the guided velocity's std towards the conditional one's, PHI in [0, 1]")
    p.add_argument("--slg_blocks", type=int, nargs="+", default=argparse.SUPPRESS, metavar="B",
                   help="skip-layer guidance: the visual blocks a third forward skips (e.g. 9 10); needs --slg_scale")
    p.add_argument("--slg_scale", type=float, default=argparse.SUPPRESS, metavar="G",
                   help="with --slg_blocks: how far the velocity is pushed away from the block-skipping prediction, >= 0 (commonly 3 — not tuned "
                        "on these checkpoints)")
    p.add_argument("--slg_interval", type=float, nargs=2, default=argparse.SUPPRESS, metavar=("LO", "HI"),
                   help="with --slg_blocks: only on the steps whose sigma lies in [LO, HI] (default every step)")
    p.add_argument("--slg_mode", choices=("block", "attention"), default=argparse.SUPPRESS,
                   help="with --slg_blocks: skip the whole block (default) or only its self-attention")
    p.add_argument("--eta", type=float, default=argparse.SUPPRESS, metavar="E",
                   help="stochastic sampling: churn in [0, 1]; 1 re-noises every step to the next sigma (euler ancestral), 0 is the plain run")
    p.add_argument("--s_noise", type=float, default=argparse.SUPPRESS, metavar="S", help="with --eta: scale of the added noise, >= 0 (default 1)")
    p.add_argument("--sde_interval", type=float, nargs=2, default=argparse.SUPPRESS, metavar=("LO", "HI"),
                   help="with --eta: only on the steps whose sigma lies in [LO, HI] (default every step)")
    p.add_argument("--sde_seed", type=int, default=argparse.SUPPRESS, metavar="N", help="with --eta: seed of the step noise (default: the run's seed)")
    p.add_argument("--source_prompt", type=str, default=argparse.SUPPRESS, metavar="TEXT",
                   help="with --video: FlowEdit — TEXT describes the source clip, --prompt the result; the clip stays where the two agree "
                        "(without it --video is the SDEdit path)")
    p.add_argument("--source_guidance", type=float, default=argparse.SUPPRESS, metavar="W",
                   help="with --source_prompt: guidance weight of the source side (default: --guidance_weight)")
    p.add_argument("--flowedit_refine", type=int, default=argparse.SUPPRESS, metavar="R",
                   help="with --source_prompt: the last R steps are plain steps on --prompt (default 0)")
    p.add_argument("--flowedit_seed", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="with --source_prompt: seed of the per-step noise (default: the run's seed)")
    p.add_argument("--enhance_weight", type=float, default=argparse.SUPPRESS, metavar="W",
                   help="Enhance-A-Video: every visual block scales its self-attention output by max(1, mean cross-frame attention * (frames + W)); "
                        "W >= 0, 0 is a valid weight (commonly 2 to 5 — not tuned on these checkpoints)")
    p.add_argument("--enhance_interval", type=float, nargs=2, default=argparse.SUPPRESS, metavar=("LO", "HI"),
                   help="with --enhance_weight: only on the steps whose sigma lies in [LO, HI] (default every step)")
    p.add_argument("--forecast_interval", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="forecast cache: after the warm-up only every N-th step runs the visual blocks, the others extrapolate their residual "
                        "(1 is off)")
    p.add_argument("--forecast_order", type=int, choices=(0, 1, 2), default=argparse.SUPPRESS, metavar="M",
                   help="with --forecast_interval: order of the extrapolation, 0, 1 or 2 (default 1)")
    p.add_argument("--forecast_warmup", type=int, default=argparse.SUPPRESS, metavar="W",
                   help="with --forecast_interval: full steps at the start (default max(order + 1, a fifth of the steps))")
    p.add_argument("--forecast_tail", type=int, default=argparse.SUPPRESS, metavar="L",
                   help="with --forecast_interval: full steps at the end (default 1)")
    return p


def forecast_keywords(args):
    """--forecast_interval / --forecast_order / --forecast_warmup / --forecast_tail -> the pipeline's keywords"""
    rest = [k for k in ("forecast_order", "forecast_warmup", "forecast_tail") if hasattr(args, k)]
    if not hasattr(args, "forecast_interval"):
        if rest:
            raise ValueError(f"--{rest[0]} needs --forecast_interval")
        return {}
    if args.forecast_interval < 1:
        raise ValueError(f"--forecast_interval must be >= 1 (got {args.forecast_interval})")
    if getattr(args, "forecast_warmup", 1) < 1 or getattr(args, "forecast_tail", 0) < 0:
        raise ValueError("--forecast_warmup must be >= 1 and --forecast_tail >= 0")
    return {"forecast_interval": args.forecast_interval, **{k: getattr(args, k) for k in rest}}


def enhance_keywords(args):
    """--enhance_weight / --enhance_interval -> the pipeline's keywords"""
    if not hasattr(args, "enhance_weight"):
        if hasattr(args, "enhance_interval"):
            raise ValueError("--enhance_interval needs --enhance_weight")
        return {}
    kw = {"enhance_weight": args.enhance_weight}
    if not kw["enhance_weight"] >= 0.0 or kw["enhance_weight"] == float("inf"):
        raise ValueError(f"--enhance_weight must be a finite number >= 0 (got {kw['enhance_weight']})")
    if hasattr(args, "enhance_interval"):
        lo, hi = args.enhance_interval
        if not lo <= hi:
            raise ValueError(f"--enhance_interval needs LO <= HI (got {lo}, {hi})")
        kw["enhance_interval"] = (lo, hi)
    return kw


def flowedit_keywords(args):
    """--source_prompt / --source_guidance / --flowedit_refine / --flowedit_seed -> the pipeline's keywords"""
    if not hasattr(args, "source_prompt"):
        if hasattr(args, "source_guidance") or hasattr(args, "flowedit_refine") or hasattr(args, "flowedit_seed"):
            raise ValueError("--source_guidance, --flowedit_refine and --flowedit_seed need --source_prompt")
        return {}
    if not hasattr(args, "video"):
        raise ValueError("--source_prompt needs --video (the clip it describes)")
    kw = {"source_caption": args.source_prompt}
    if hasattr(args, "source_guidance"):
        kw["source_guidance_weight"] = args.source_guidance
    if hasattr(args, "flowedit_refine"):
        if args.flowedit_refine < 0:
            raise ValueError(f"--flowedit_refine must be >= 0 (got {args.flowedit_refine})")
        if args.flowedit_refine > 0 and hasattr(args, "mask"):
            raise ValueError("--flowedit_refine together with --mask is not supported")
        kw["flowedit_refine"] = args.flowedit_refine
    if hasattr(args, "flowedit_seed"):
        kw["flowedit_seed"] = args.flowedit_seed
    for flag in ("context_seconds", "eta", "slg_blocks", "nag_scale", "regions", "region", "preview", "forecast_interval", "guidance_interval",
                 "cfg_zero_star", "cfg_zero_init", "cfg_rescale"):
        if getattr(args, flag, None):
            raise ValueError(f"--source_prompt together with --{flag} is not supported")
    if getattr(args, "magcache", False) or getattr(args, "calibrate_magcache", None):
        raise ValueError("--source_prompt together with --magcache is not supported: the ratio table is indexed by the call of a plain run")
    return kw


def stochastic_keywords(args):
    """--eta / --s_noise / --sde_interval / --sde_seed -> the pipeline's keywords"""
    if not hasattr(args, "eta"):
        if hasattr(args, "s_noise") or hasattr(args, "sde_interval") or hasattr(args, "sde_seed"):
            raise ValueError("--s_noise, --sde_interval and --sde_seed need --eta")
        return {}
    kw = {"eta": args.eta}
    if not 0.0 <= args.eta <= 1.0:
        raise ValueError(f"--eta must be in [0, 1] (got {args.eta})")
    if hasattr(args, "s_noise"):
        if not args.s_noise >= 0.0 or args.s_noise == float("inf"):
            raise ValueError(f"--s_noise must be a finite number >= 0 (got {args.s_noise})")
        kw["s_noise"] = args.s_noise
    if hasattr(args, "sde_interval"):
        lo, hi = args.sde_interval
        if not lo <= hi:
            raise ValueError(f"--sde_interval needs LO <= HI (got {lo}, {hi})")
        kw["sde_interval"] = (lo, hi)
    if hasattr(args, "sde_seed"):
        kw["sde_seed"] = args.sde_seed
    if args.eta > 0.0:
        if hasattr(args, "context_seconds"):
            raise ValueError("--eta together with --context_seconds is not supported")
        if getattr(args, "magcache", False) or getattr(args, "calibrate_magcache", None):
            raise ValueError("--eta together with --magcache is not supported: the ratio table was measured on ODE trajectories")
        if hasattr(args, "preview"):
            raise ValueError("--eta together with --preview is not supported: the preview's x0 does not hold after the noise is added")
    return kw


def skip_keywords(args):
    """--slg_blocks / --slg_scale / --slg_interval / --slg_mode -> the pipeline's keywords"""
    if not hasattr(args, "slg_blocks"):
        if hasattr(args, "slg_scale") or hasattr(args, "slg_interval") or hasattr(args, "slg_mode"):
            raise ValueError("--slg_scale, --slg_interval and --slg_mode need --slg_blocks")
        return {}
    if not hasattr(args, "slg_scale"):
        raise ValueError("--slg_blocks needs --slg_scale")
    kw = {"slg_blocks": list(args.slg_blocks), "slg_scale": args.slg_scale, "slg_mode": getattr(args, "slg_mode", "block")}
    if any(b < 0 for b in kw["slg_blocks"]) or len(set(kw["slg_blocks"])) != len(kw["slg_blocks"]):
        raise ValueError(f"--slg_blocks must be distinct block indices >= 0 (got {kw['slg_blocks']})")
    if not kw["slg_scale"] >= 0.0 or kw["slg_scale"] == float("inf"):
        raise ValueError(f"--slg_scale must be a finite number >= 0 (got {kw['slg_scale']})")
    if hasattr(args, "slg_interval"):
        lo, hi = args.slg_interval
        if not lo <= hi:
            raise ValueError(f"--slg_interval needs LO <= HI (got {lo}, {hi})")
        kw["slg_interval"] = (lo, hi)
    if hasattr(args, "context_seconds"):
        raise ValueError("--slg_blocks together with --context_seconds is not supported")
    if getattr(args, "magcache", False):
        raise ValueError("--slg_blocks together with --magcache is not supported: the ratio table is indexed by the call of a plain run")
    return kw


def guidance_keywords(args):
    """--guidance_schedule / --guidance_interval / --cfg_zero_star / --cfg_zero_init / --cfg_rescale -> the pipeline's keywords"""
    kw = {k: getattr(args, k) for k in ("guidance_schedule", "guidance_interval", "cfg_zero_star", "cfg_zero_init", "cfg_rescale") if hasattr(args, k)}
    if "guidance_schedule" in kw and args.sample_steps is not None and len(kw["guidance_schedule"]) != args.sample_steps:
        raise ValueError(f"--guidance_schedule holds {len(kw['guidance_schedule'])} weights, --sample_steps is {args.sample_steps}")
    if "guidance_interval" in kw:
        lo, hi = kw["guidance_interval"]
        if not lo <= hi:
            raise ValueError(f"--guidance_interval needs LO <= HI (got {lo}, {hi})")
        kw["guidance_interval"] = (lo, hi)
    if kw.get("cfg_zero_init", 0) < 0:
        raise ValueError(f"--cfg_zero_init must be >= 0 (got {kw['cfg_zero_init']})")
    if not 0.0 <= kw.get("cfg_rescale", 0.0) <= 1.0:
        raise ValueError(f"--cfg_rescale must be in [0, 1] (got {kw['cfg_rescale']})")
    if kw and hasattr(args, "context_seconds"):
        raise ValueError("--guidance_schedule / --guidance_interval / --cfg_zero_star / --cfg_zero_init / --cfg_rescale together with "
                         "--context_seconds are not supported")
    return kw


def region_keywords(args, load_mask=None):
    """--region PROMPT MASKFILE (repeatable) / --region_base_weight -> the pipeline's keywords; the mask files go through --mask's resize
    and centre-crop (`load_mask(path)` -> (height, width) or (F, height, width) in [0, 1])"""
    if not hasattr(args, "region"):
        if hasattr(args, "region_base_weight"):
            raise ValueError("--region_base_weight needs --region")
        return {}
    w = getattr(args, "region_base_weight", 0.0)
    if not 0.0 <= w <= 1.0:
        raise ValueError(f"--region_base_weight must be in [0, 1] (got {w})")
    if len(args.region) > 8:
        raise ValueError(f"at most 8 --region arguments (got {len(args.region)})")
    if hasattr(args, "context_seconds"):
        raise ValueError("--region together with --context_seconds is not supported")
    load_mask = load_mask or (lambda path: pixel_mask_file(path, args.height, args.width))
    return {"regions": [(prompt, load_mask(path)) for prompt, path in args.region], "region_base_weight": w}


def pixel_mask_file(path, height, width):
    """a mask file (an image, or a clip) through the frames' own resize-and-crop rule: (height, width) or (F, height, width) in [0, 1]"""
    from kandinsky.conditioning import preprocess_video
    from kandinsky.video_io import read_video
    m = (preprocess_video(read_video(path), height, width).mean(dim=1) + 1.0) / 2.0
    return m[0] if m.shape[0] == 1 else m


def nag_keywords(args):
    """--nag_scale / --nag_tau / --nag_alpha -> the pipeline's keywords"""
    if not hasattr(args, "nag_scale"):
        if hasattr(args, "nag_tau") or hasattr(args, "nag_alpha"):
            raise ValueError("--nag_tau and --nag_alpha need --nag_scale")
        return {}
    kw = {"nag_scale": args.nag_scale, "nag_tau": getattr(args, "nag_tau", 2.5), "nag_alpha": getattr(args, "nag_alpha", 0.25)}
    if not kw["nag_scale"] >= 1.0 or not kw["nag_tau"] >= 1.0 or not 0.0 <= kw["nag_alpha"] <= 1.0:
        raise ValueError(f"--nag_scale and --nag_tau must be >= 1 and --nag_alpha in [0, 1] (got {kw['nag_scale']}, {kw['nag_tau']}, {kw['nag_alpha']})")
    return kw


def context_keywords(args):
    """--context_seconds / --context_overlap_seconds -> the pipeline's keywords"""
    if not hasattr(args, "context_seconds"):
        if hasattr(args, "context_overlap_seconds"):
            raise ValueError("--context_overlap_seconds needs --context_seconds")
        return {}
    kw = {"context_seconds": args.context_seconds}
    if hasattr(args, "context_overlap_seconds"):
        kw["context_overlap_seconds"] = args.context_overlap_seconds
    return kw


def tile_keywords(args):
    """--tile / --tile_overlap -> the pipeline's keywords"""
    if not hasattr(args, "tile"):
        if hasattr(args, "tile_overlap"):
            raise ValueError("--tile_overlap needs --tile HEIGHT WIDTH")
        return {}
    kw = {"tile_height": args.tile[0], "tile_width": args.tile[1]}
    if hasattr(args, "tile_overlap"):
        kw["tile_overlap"] = args.tile_overlap
    return kw


def preview_keywords(args):
    """--preview / --preview_every / --preview_factors -> the pipeline's keywords"""
    if not hasattr(args, "preview"):
        if hasattr(args, "preview_every") or hasattr(args, "preview_factors"):
            raise ValueError("--preview_every and --preview_factors need --preview DIR")
        return {}
    if not hasattr(args, "preview_factors"):
        raise ValueError("--preview needs --preview_factors FILE (no default table ships: make one with --fit_preview_factors OUT.json)")
    from kandinsky.preview import load_factors, preview_to_image
    os.makedirs(args.preview, exist_ok=True)

    def save(info):
        if info.preview is not None:
            preview_to_image(info.preview).save(os.path.join(args.preview, f"step_{info.step:03d}.png"))

    return {"callback": save, "preview_every": getattr(args, "preview_every", 1), "preview_factors": load_factors(args.preview_factors)}


def load_edit_inputs(args):
    """--video / --strength / --mask -> the pipeline's keywords"""
    kw = {}
    if getattr(args, "video", None) is None:
        if hasattr(args, "strength") or hasattr(args, "mask"):
            raise ValueError("--strength and --mask need --video")
        return kw
    from kandinsky.video_io import read_video
    kw["video"] = read_video(args.video)
    if hasattr(args, "strength"):
        kw["strength"] = args.strength
    if hasattr(args, "mask"):
        # the mask goes through the frames' own resize-and-crop rule, so a mask drawn on the source clip lands where the clip does
        from kandinsky.conditioning import preprocess_video
        m = (preprocess_video(read_video(args.mask), args.height, args.width).mean(dim=1) + 1.0) / 2.0   # (F, height, width) in [0, 1]
        kw["mask"] = m[0] if m.shape[0] == 1 else m
    return kw


def validate_args(args):
    if hasattr(args, "tile"):   # the frame is the pipeline's to check: multiples of 16 that are at least the tile
        if (args.tile[1], args.tile[0]) not in SUPPORTED_SIZES:
            raise NotImplementedError(f"Provided size of tile is not supported: {(args.tile[1], args.tile[0])}")
        return
    if (args.width, args.height) not in SUPPORTED_SIZES:
        raise NotImplementedError(f"Provided size of video is not supported: {(args.width, args.height)}")


def main(argv=None):
    warnings.filterwarnings("ignore")
    args = build_parser().parse_args(argv)
    validate_args(args)
    nag_kw = nag_keywords(args)   # refused before the models load
    region_kw = region_keywords(args)
    guide_kw = guidance_keywords(args)
    skip_kw = skip_keywords(args)
    sto_kw = stochastic_keywords(args)
    enhance_kw = enhance_keywords(args)
    forecast_kw = forecast_keywords(args)
    flow_kw = flowedit_keywords(args)
    from kandinsky import get_T2V_pipeline
    pipe = get_T2V_pipeline(device_map={"dit": "cuda:0", "vae": "cuda:0", "text_embedder": "cuda:0"}, conf_path=args.config,
                            offload=args.offload, magcache=args.magcache and not args.calibrate_magcache,
                            magcache_ratios=args.magcache_ratios, lora=getattr(args, "lora", None),
                            lora_scale=getattr(args, "lora_scale", 1.0))
    if args.output_filename is None:
        args.output_filename = "./" + args.prompt.replace(" ", "_") + ".mp4"
    image = None
    if args.image is not None:
        from PIL import Image
        image = Image.open(args.image).convert("RGB")
    edit_kw = load_edit_inputs(args)
    if args.calibrate_magcache:
        import json
        from kandinsky.magcache_utils import calibrate_magcache
        table = calibrate_magcache(pipe, [args.prompt], time_length=args.video_duration, width=args.width, height=args.height,
                                   num_steps=args.sample_steps, guidance_weight=args.guidance_weight, scheduler_scale=args.scheduler_scale,
                                   expand_prompts=args.expand_prompt, negative_caption=args.negative_prompt, image=image)
        with open(args.calibrate_magcache, "w") as f:
            json.dump(table, f, indent=1)
        print(f"MagCache ratio table ({len(table['mag_ratios'])} ratios, {table['rows_counted']} of {table['rows_total']} rows counted) "
              f"is saved to {args.calibrate_magcache}; use it with --magcache --magcache_ratios {args.calibrate_magcache}")
        return
    if hasattr(args, "fit_preview_factors"):
        from kandinsky.preview import fit_from_pipeline, save_factors
        W, b = fit_from_pipeline(pipe, args.prompt, time_length=args.video_duration, width=args.width, height=args.height,
                                 num_steps=args.sample_steps, guidance_weight=args.guidance_weight, scheduler_scale=args.scheduler_scale,
                                 expand_prompts=args.expand_prompt, negative_caption=args.negative_prompt, image=image, **edit_kw)
        save_factors(args.fit_preview_factors, W, b, note=f"fitted on one generation of {args.config}")
        print(f"Preview factors ({W.shape[0]} channels) are saved to {args.fit_preview_factors}; use them with --preview DIR "
              f"--preview_factors {args.fit_preview_factors}")
        return
    edit_kw.update(preview_keywords(args))
    edit_kw.update(context_keywords(args))
    edit_kw.update(tile_keywords(args))
    edit_kw.update(nag_kw)
    edit_kw.update(region_kw)
    edit_kw.update(guide_kw)
    edit_kw.update(skip_kw)
    edit_kw.update(sto_kw)
    edit_kw.update(enhance_kw)
    edit_kw.update(forecast_kw)
    edit_kw.update(flow_kw)
    t0 = time.perf_counter()
    pipe(args.prompt, time_length=args.video_duration, width=args.width, height=args.height, num_steps=args.sample_steps,
         guidance_weight=args.guidance_weight, scheduler_scale=args.scheduler_scale, expand_prompts=args.expand_prompt,
         negative_caption=args.negative_prompt, save_path=args.output_filename, image=image, **edit_kw)
    print(f"TIME ELAPSED: {time.perf_counter() - t0}")
    print(f"Generated video is saved to {args.output_filename}")


if __name__ == "__main__":
    main()
