#!/usr/bin/env python
"""bench.py — DiT denoising steps/sec of the MI355X engine on BASELINE.json's metric/config.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run does only what the headline needs: set up, warm up, time the K steps, write --dump-outputs, print the line (with the
`roofline` block from the HIP events inside the timed region).  `--full` adds everything that costs time of its own: the parity check
against the reference golden, the latent pin, the per-family breakdown pass, the VAE decode leg, the live rocprofv3 traffic passes and
the CPU baseline (each can still be skipped with its --no-* flag).

N > 1: one process per GPU under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment, the reference's launch
contract: README.md:269-276, kandinsky/utils.py:40-55).  Called WITHOUT that environment, `python bench.py --gpus N` launches itself:
it re-executes under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free>` with every
flag forwarded, rank 0 prints the one JSON line, and the exit code is the launcher's (non-zero if any rank failed).

A "step" = one Euler update of the flow-matching sampler = one DiT forward (guidance_weight = 1,
config_5s_nocfg) over the synthetic 5 s 768x512 latent (31,64,96,16) -> N = 47 616 visual tokens,
L = 256 text tokens, 2B-Lite architecture with random-init weights (no checkpoints offline).
The latent, text embeddings and weights are resident in HBM before the timed region.
Prints ONE JSON line (rank 0) with `roofline` (dominant kernel: dense self-attention, MFMA-bound) and, with --full,
`cpu_baseline` (the fp32 CPU oracle on the host cores, bounded sample).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "kandinsky-5_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

LITE = dict(in_visual_dim=16, out_visual_dim=16, time_dim=512, patch_size=(1, 2, 2), model_dim=1792, ff_dim=7168,
            num_text_blocks=2, num_visual_blocks=32, axes_dims=(16, 24, 24), visual_cond=True, in_text_dim=3584,
            in_text_dim2=768)
WORKLOADS = {
    # name: latent (T,H,W), text len, null text len, guidance, attention
    "5s_nocfg": dict(latent=(31, 64, 96), L=256, Lnull=32, w=1.0, attn="flash",
                     desc="config_5s_nocfg.yaml: 2B Lite, 768x512 5 s latent (31,64,96,16), 47616 tokens, L=256, "
                          "guidance 1.0 (1 DiT forward per step), NFE=50"),
    "5s_sft": dict(latent=(31, 64, 96), L=256, Lnull=32, w=5.0, attn="flash",
                   desc="config_5s_sft.yaml: as 5s_nocfg with CFG (cond + uncond forward per step), NFE=100"),
    "10s_nabla": dict(latent=(61, 64, 96), L=256, Lnull=32, w=1.0, attn="nabla",
                      desc="config_10s_sft.yaml attention (NABLA P=0.9, wT=11, wH=wW=3) on the 768x512 10 s latent (61,64,96,16), "
                           "93696 tokens, guidance 1.0; map density depends on the (random) weights and is reported"),
    "10s_hd_nabla": dict(latent=(61, 96, 160), L=256, Lnull=32, w=1.0, attn="nabla",
                         desc="BASELINE config 5's shape: NABLA on the 1280x768 10 s latent (61,96,160,16), 234240 tokens = 3660 blocks, guidance "
                              "1.0 (meant for --emulate-shard 4 / real ranks: one CFG branch of the SP x 4 + CFG x 2 plan)"),
    "10s_hd_sft": dict(latent=(61, 96, 160), L=256, Lnull=32, w=5.0, attn="nabla",
                       desc="BASELINE config 5: config_10s_sft.yaml (NABLA P=0.9, wT=11, wH=wW=3, CFG: cond + uncond forward per step, NFE=100) on the "
                            "1280x768 10 s latent (61,96,160,16), 234240 tokens = 3660 blocks; with --gpus 8 --cfg-parallel: sequence-parallel x 4 inside "
                            "each CFG branch + the velocity exchange of the pair, all inside k5_sample"),
    "2s_256": dict(latent=(13, 32, 32), L=256, Lnull=32, w=1.0, attn="flash",
                   desc="config_5s_distil.yaml plumbing case: 256x256 2 s latent (13,32,32,16), 3328 tokens"),
}
PEAK_BF16_TFLOPS = 2500.0  # dense MFMA bf16, /opt/skills/guides/MI355X_MICROARCH.md


def flops_forward(N, L, D=1792, FF=7168, blocks=32):
    """F_fwd = 32*[2N(6D^2+2D*FF) + 2L*2D^2 + 4N^2 D + 4NLD] + small."""
    return blocks * (2 * N * (6 * D * D + 2 * D * FF) + 2 * L * 2 * D * D + 4 * N * N * D + 4 * N * L * D) + 0.2e12


def cpu_baseline(N, budget_s=3.0):   # the full-size sample runs ~3.5x slower than the 1024-token calibration predicts
    """The CPU oracle (own fp32 restatement pinned against the reference, oracle/k5_oracle.py) on the host
    cores: ONE full-width decoder block of the 32 at the workload's token count, extrapolated x32 (the text
    blocks / embeddings are <0.1 % of the FLOPs).  If one block at N would exceed the budget, a query-row
    slice of the attention is timed and scaled (stated in `sample`)."""
    from oracle import k5_oracle as O
    ncpu = os.cpu_count() or 1
    cfg = O.DitConfig(**dict(LITE, num_visual_blocks=1, num_text_blocks=0))
    names = [k for k in O.state_dict_manifest(cfg) if k.startswith("visual_transformer_blocks.0.")]
    man = O.state_dict_manifest(cfg)
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(man[k], generator=g) * 0.02 for k in names}
    D, L = cfg.model_dim, 256
    # calibrate on a small token count to pick the row fraction that fits the budget
    n_cal = 1024
    x = torch.randn(n_cal, D, generator=g)
    text, temb = torch.randn(L, D, generator=g), torch.randn(1, cfg.time_dim, generator=g)
    cs = torch.ones(n_cal, 32), torch.zeros(n_cal, 32)
    # thread count: the container may be CPU-limited far below os.cpu_count() (256 torch threads on the 2x64-core GPU
    # host ran 100x slower than 16) -> pick the fastest of a few candidates on the calibration problem
    best = None
    for th in sorted({min(ncpu, c) for c in (8, 16, 32, 64)}):
        torch.set_num_threads(th)
        O.decoder_block(sd, "visual_transformer_blocks.0", x[:128], text, temb, cs[0][:128], cs[1][:128], cfg, "fp32")
        t0 = time.perf_counter()
        O.decoder_block(sd, "visual_transformer_blocks.0", x, text, temb, cs[0], cs[1], cfg, "fp32")
        dtc = time.perf_counter() - t0
        if best is None or dtc < best[0]:
            best = (dtc, th)
        if dtc > 3 * best[0]:
            break
    t_cal, cores = best
    torch.set_num_threads(cores)
    fl = lambda n, nq: 2 * nq * (6 * D * D + 2 * D * cfg.ff_dim) + 4 * nq * n * D + 4 * nq * L * D  # noqa: E731
    rate = fl(n_cal, n_cal) / t_cal
    frac = min(1.0, budget_s * rate / fl(N, N))
    nq = max(256, int(N * frac) // 256 * 256)
    # timed sample: nq query rows of one block against all N keys (all linears on nq rows)
    x = torch.randn(N, D, generator=g)
    cos, sin = torch.ones(N, 32), torch.zeros(N, 32)
    t0 = time.perf_counter()
    mod = O.modulation(sd, "visual_transformer_blocks.0.visual_modulation", temb)
    shift, scale, gate = torch.chunk(torch.chunk(mod, 3, dim=-1)[0], 3, dim=-1)
    h = O.scale_shift_norm(x, scale, shift, "fp32")
    p = "visual_transformer_blocks.0.self_attention"
    q, k, v = O._attn_qkv(sd, p, h[:nq], h, "fp32", cfg.num_heads)
    q, k = O.apply_rotary(q, cos[:nq], sin[:nq], "fp32"), O.apply_rotary(k, cos, sin, "fp32")
    o = O.sdpa(q, k, v, "fp32")
    xs = O.gate_sum(x[:nq], O._linear(o, sd[p + ".out_layer.weight"], sd[p + ".out_layer.bias"], "fp32"), gate, "fp32")
    xs = xs + O.cross_attention(sd, "visual_transformer_blocks.0.cross_attention", xs, text, cfg, "fp32")
    xs = xs + O.feed_forward(sd, "visual_transformer_blocks.0.feed_forward", xs, "fp32")
    t_s = time.perf_counter() - t0
    # k/v projections were done on all N rows; scale the row-proportional part only
    t_block = t_s * (fl(N, N) / (fl(N, nq) + 2 * (N - nq) * 2 * D * D))
    # BASELINE config 1 (config_5s_distil: (13,32,32) latent = 3328 tokens, the reference's own CPU-runnable case) IN FULL, no
    # extrapolation: 32 complete decoder-block evaluations at N = 3328 (one block's weights reused: the arithmetic and its cost are
    # those of the 32 distinct blocks; the two text blocks / embeddings are < 0.2 % of a forward)
    n1 = 13 * 16 * 16
    x1, c1 = torch.randn(n1, D, generator=g), (torch.ones(n1, 32), torch.zeros(n1, 32))
    t0 = time.perf_counter()
    for _ in range(32):
        x1 = O.decoder_block(sd, "visual_transformer_blocks.0", x1, text, temb, c1[0], c1[1], cfg, "fp32")
    t_c1 = time.perf_counter() - t0
    return {"value": 1.0 / (32 * t_block), "unit": "steps/s", "cores": cores, "host_cpus": ncpu, "kind": "port",
            "sample": f"fp32 torch-CPU oracle, 1 of 32 decoder blocks, {nq} of {N} query rows against all {N} keys "
                      f"({t_s:.1f} s measured), scaled to the full block and x32 blocks; {cores} torch threads = the fastest of {{8, 16, 32, 64}} "
                      f"calibrated on this host ({ncpu} logical CPUs; more threads measured slower: the container's CPU quota is below the host's core count)",
            "ms_per_step": 32 * t_block * 1e3,
            "config1_forward_s": t_c1,
            "config1_sample": f"BASELINE config 1 (256x256 2 s latent (13,32,32), {n1} tokens): 32 full decoder blocks timed in full, "
                              f"{cores} threads; x16 steps (NFE 16) = {16 * t_c1:.0f} s per clip on this host"}


PIN_FILE = os.path.join(ROOT, "tests", "golden", "bench_latent_pins.json")
PIN_TOL = 3e-2             # two builds of the engine differ by fp32 summation order; through 25 steps of 32 blocks that stays below 1e-2 (measured)


def latent_pin(latent, noise, args, world):
    if args.qk_gain != 1.0 or args.blocks != 32 or args.fp8 or args.emulate_shard > 1 or args.magcache or args.attn_online or args.nabla_p != 0.9:
        return None
    key = f"{args.workload}:{args.warmup + args.steps}"
    idx = torch.randperm(noise.numel(), generator=torch.Generator().manual_seed(12))[:512].sort().values
    upd = (latent.reshape(-1)[idx.to(latent.device)].float().cpu() - noise.reshape(-1)[idx])
    ss = float((latent.cpu() - noise).double().pow(2).sum())
    out = {"key": key, "update_sumsq": ss, "status": "no committed pin for this (workload, steps)"}
    if args.write_pin:
        os.makedirs(os.path.dirname(args.write_pin) or ".", exist_ok=True)
        with open(args.write_pin, "w") as f:
            json.dump({key: {"update_samples": [float(v) for v in upd], "update_sumsq": ss, "n_gpus": world}}, f)
    try:
        pins = json.load(open(PIN_FILE))
    except Exception:   # noqa: BLE001
        pins = {}
    if key in pins:
        ref = torch.tensor(pins[key]["update_samples"])
        r = float((upd - ref).norm() / ref.norm())
        out.update({"rel_l2_update_vs_pinned": r, "pinned_update_sumsq": pins[key]["update_sumsq"], "tolerance": PIN_TOL,
                    "status": "ok" if r <= PIN_TOL and abs(ss - pins[key]["update_sumsq"]) <= 2 * PIN_TOL * pins[key]["update_sumsq"] else "FAILED"})
    return out


PARITY_TOL_UPDATE = 4e-2   # on (latent - noise) after 1 / 2 steps: one 32-block bf16 forward sits 1.9e-2 from the fp32 reference (the bf16-island
                           # ORACLE's own distance, tests/golden/dit_fulldepth_meta.json f32.bf16_oracle_vs_ref); 2 x that as the gate


def parity_check(dit, noise, dev, sig, te, ne, vpos, tpos, ntpos, wl, sparse):
    from safetensors.torch import load_file
    gdir = os.path.join(ROOT, "tests", "golden")
    try:
        G = load_file(os.path.join(gdir, "dit_fulldepth_c2.safetensors"))
        meta = json.load(open(os.path.join(gdir, "dit_fulldepth_meta.json")))["c2"]
    except Exception as e:   # noqa: BLE001
        return {"status": "golden missing", "error": str(e)}
    idx = G["sample_idx"].to(dev)
    nz = noise.reshape(-1)[G["sample_idx"]]
    lat = noise.to(dev).clone()
    out = {"reference": "the reference's generate() (generation_utils.py:80-129, fp32 on the host) on the same seeded weights / noise / prompt, "
                        "32 visual blocks, NFE 50 schedule: oracle/gen_golden_fulldepth.py c2", "samples": int(idx.numel()), "steps": []}
    ok = True
    for i in range(1, meta["steps_kept"] + 1):
        dit.sample(lat, sig[i - 1:i + 1], te, ne, vpos, tpos, ntpos, wl["w"], scale_factor=(1.0, 2.0, 2.0), sparse_params=sparse)
        got = lat.reshape(-1)[idx].float().cpu()
        ref = G[f"latent_after_{i}"]
        ru = float(((got - nz) - (ref - nz)).norm() / (ref - nz).norm())
        rl = float((got - ref).norm() / ref.norm())
        ss = float((lat.cpu() - noise).double().pow(2).sum())
        out["steps"].append({"after_step": i, "rel_l2_update": ru, "rel_l2_latent": rl, "update_sumsq": ss,
                             "update_sumsq_reference": meta["after_step"][i - 1]["update_sumsq"]})
        ok = ok and ru <= PARITY_TOL_UPDATE
    out["tolerance_rel_l2_update"] = PARITY_TOL_UPDATE
    out["status"] = "ok" if ok else "FAILED"
    return out


def live_traffic(tokens, timeout_s=150):
    """HBM-side bytes of ONE dense self-attention launch, measured by THIS bench run (the line used to quote a committed file):
    two child runs of this script (2 visual blocks, 1 + 1 steps: the per-launch figure does not depend on the depth) under
    `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` — one counter per pass, kernel trace only, no sys / hip / hsa trace domains, exactly the
    collection /opt/skills/guides/MI355X_MICROARCH.md prescribes — FETCH_SIZE doubled (gfx950 reports half of a wide coalesced stream), KB units.
    The launch taken is the main dense launch (largest fetch among attn_fwd_kernel dispatches; the balanced call's tail launches are smaller);
    `traffic` = the MAX over its dispatches.  Returns (bytes or None, source string).  Never raises: a missing profiler, a timeout or an
    unreadable CSV leaves the caller on the committed figure, and says why."""
    import csv, glob, shutil, subprocess, tempfile
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if prof is None:
        return None, "rocprofv3 not found"
    tmp = tempfile.mkdtemp(prefix="k5_pmc_", dir="/tmp")
    got = {}
    try:
        for c in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, c)
            cmd = [prof, "--pmc", c, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
                   "--steps", "1", "--warmup", "1", "--blocks", "2"]   # a plain run: none of the --full extras
            env = dict(os.environ, TMPDIR="/tmp")
            for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
                env.pop(k, None)
            # own session: on a timeout the WHOLE group goes (rocprofv3 and the bench it launched — subprocess.run would kill only the
            # profiler and leave a grandchild on the GPU under the VAE leg: ADVICE r5)
            pr = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, start_new_session=True)
            try:
                _, err_txt = pr.communicate(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                import signal
                try:
                    os.killpg(pr.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                pr.communicate()
                return None, f"the {c} pass did not finish within {timeout_s} s (process group killed)"
            r = subprocess.CompletedProcess(cmd, pr.returncode, None, err_txt)
            per, names = {}, {}
            for fn in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                with open(fn) as f:
                    for row in csv.DictReader(f):
                        if row.get("Counter_Name") == c:
                            per[row["Dispatch_Id"]] = per.get(row["Dispatch_Id"], 0.0) + float(row["Counter_Value"])
                            names[row["Dispatch_Id"]] = row["Kernel_Name"]
            vals = [v for i, v in per.items() if "attn_fwd_kernel" in names[i]]
            if not vals:
                return None, f"the {c} pass produced no attention dispatch (rc {r.returncode}: {(r.stderr or '')[-200:]!r})"
            got[c] = vals
        f_main = max(got["FETCH_SIZE"])
        main_f = [v for v in got["FETCH_SIZE"] if v > 0.5 * f_main]       # the main launches (tail / text launches fetch far less)
        w_main = max(got["WRITE_SIZE"])
        return 2.0 * f_main * 1024 + w_main * 1024, (
            f"THIS run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, separate child passes of bench.py --blocks 2 ({len(main_f)} main launches; max taken), "
            f"FETCH x2 per MI355X_MICROARCH.md; fabric-side counter (Infinity-Cache hits included); algorithmic bytes {4 * tokens * 28 * 64 * 2}")
    except Exception as e:     # noqa: BLE001 — the bench line must still be printed
        return None, f"live PMC pass failed: {type(e).__name__}: {str(e)[:200]}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def self_launch_command(argv, gpus, port=None):
    """`python bench.py --gpus N ...` outside torch.distributed.run: the command that runs the same flags as N ranks on this node."""
    if port is None:
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="5s_nocfg", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need (off by default): parity check, latent pin, per-family breakdown pass, VAE "
                         "decode leg, live rocprofv3 traffic passes, CPU baseline; the --no-* flags below skip single ones of these")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-parity-check", action="store_true", help="with --full: skip the untimed 2-step check against the reference golden (5s_nocfg only)")
    ap.add_argument("--write-pin", default="", metavar="FILE", help="write this run's latent pin entry (to be merged into tests/golden/bench_latent_pins.json)")
    ap.add_argument("--no-live-traffic", action="store_true", help="with --full: do not run the two rocprofv3 --pmc child passes that measure `roofline.traffic` "
                    "(the line then quotes the committed profile, and says so)")
    ap.add_argument("--no-vae", action="store_true", help="with --full: skip the (untimed-for-`value`) VAE decode leg")
    ap.add_argument("--force-sp", action="store_true", help="debug: drive the sharded code path through a world=1 RCCL communicator")
    ap.add_argument("--magcache", action="store_true", help="MagCache with the config's ratio table (changes the work per step: not the headline metric)")
    ap.add_argument("--fp8", type=int, nargs="?", const=1, default=0, metavar="MASK",
                    help="opt-in lossy mode, W8A8 e4m3 linear layers (k5_dit_set_fp8 mask: 1 feed-forward (default when given without a value), 2 q|k|v "
                         "projections, 4 out projection; 7 = all): NOT the headline number, reported as dtype bf16+fp8")
    ap.add_argument("--profile-level", type=int, default=2, choices=(0, 1, 2),
                    help="HIP events inside the timed region: 2 = around the roofline kernel only (default), 1 = every kernel family, 0 = none")
    ap.add_argument("--no-breakdown", action="store_true", help="with --full: skip the separate per-family timing pass")
    ap.add_argument("--sp-slices", type=int, default=1, help="sequence parallelism: exchange K / V^T of a block in this many slices and attend "
                    "each slice as it lands (engine option sp_slices; 1 = one in-place all-gather per block)")
    ap.add_argument("--sp-autotune", action="store_true",
                    help="N > 1: let the engine time the admissible exchanges at the first sharded forward and keep the fastest (opt-in: the choice depends "
                         "on timings and the schedules differ in summation order; recorded in the line as sp_schedule)")
    ap.add_argument("--cfg-parallel", action="store_true",
                    help="N even, a workload with guidance (5s_sft, 10s_hd_sft): ranks [0, N/2) run the conditional forward, [N/2, N) the unconditional "
                         "one, each group sequence-parallel inside; the pair exchange lives in the engine (k5_dit_cfg_pair_init)")
    ap.add_argument("--transport", default=None, choices=("rccl", "ipc"),
                    help="N > 1: what moves K / V^T between the ranks — RCCL (default) or the engine's own IPC transport (peers read each other's "
                         "hipIpc-mapped slots, flags in device memory; k5_dit_comm_init_ipc).  Also K5_SP_TRANSPORT")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="N > 1 ranks on the devices that exist (rank r on device r %% count; one GPU: all on device 0) over the IPC transport — runs the "
                         "process boundary of the sharded path on a one-GPU box.  INVALID as a bench (the ranks time-slice one GPU); rank_check and "
                         "ipc_ranks_seen are what it is for")
    ap.add_argument("--graph", action="store_true", help="replay one hipGraph-captured step (k5_dit_set_graph; needs --profile-level 0: events cannot be captured)")
    ap.add_argument("--emulate-shard", type=int, default=0, metavar="P",
                    help="debug only (INVALID as a bench): per-rank compute of a P-GPU run on one GPU, collectives move nothing")
    ap.add_argument("--engine-option", action="append", default=[], metavar="NAME=INT",
                    help="A/B switch: k5_dit_set_option(NAME, INT) before the run (recorded in config.engine_options)")
    ap.add_argument("--blocks", type=int, default=32, help="debug only: fewer visual blocks => INVALID as a bench")
    ap.add_argument("--attn-online", action="store_true",
                    help="run every self-attention head on the online-max softmax kernel (what heads whose |q||k| bound exceeds "
                         "the fixed-offset window get); reported as roofline.variant")
    ap.add_argument("--qk-gain", type=float, default=1.0,
                    help="multiply the synthetic QK-norm weights (query_norm / key_norm) by this factor: > ~2.9 pushes the "
                         "data-derived softmax bound past the fixed-offset window")
    ap.add_argument("--nabla-p", type=float, default=0.9, help="NABLA cumulative-mass threshold P (config: 0.9); with random weights the "
                    "block softmax is near uniform, so kept density ~ P: 0.0 = STA window only, 0.15 ~ 20 %% density")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what they returned (the fp32 latent) as DIR/latent.npy, so that two builds can be compared "
                         "output for output (the inputs depend only on the arguments)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")

    if args.oversubscribe:
        os.environ["K5_OVERSUBSCRIBE"] = "1"
        args.transport = args.transport or "ipc"
        if args.transport != "ipc":
            raise SystemExit("--oversubscribe needs the IPC transport (RCCL refuses two ranks on one device)")
    if args.transport:
        os.environ["K5_SP_TRANSPORT"] = args.transport
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # not under a launcher: become one (the ranks then take the branch below); every flag is forwarded verbatim
        import subprocess
        cmd = self_launch_command(sys.argv[1:], args.gpus)
        print("bench.py: launching " + " ".join(cmd), file=sys.stderr, flush=True)
        raise SystemExit(subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))).returncode)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE = {world}: launch with --nproc-per-node {args.gpus} (or call bench.py without a launcher)")
    ndev = torch.cuda.device_count()
    from kandinsky.utils import init_rank_process_group, rank_device_index
    dev_index = rank_device_index(local_rank)     # cuda:LOCAL_RANK (reference utils.py:40-45); --oversubscribe wraps around the devices that exist
    if dev_index >= ndev:
        raise SystemExit(f"bench.py rank {rank}: needs {args.gpus} devices on this node, found {ndev} (--oversubscribe runs the ranks on the devices there are)")
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    host_group = False
    if world > 1:
        import torch.distributed as dist
        init_rank_process_group(local_rank)       # nccl bound to the device, or gloo under the IPC transport
        host_group = dist.get_backend() == "gloo"

    from kandinsky.models.dit import DiffusionTransformer3D
    wl = WORKLOADS[args.workload]
    T, H, W = wl["latent"]
    N, L = T * (H // 2) * (W // 2), wl["L"]
    # the configs' 50-step schedule; a run of more warm-up + timed steps stretches it, so that every one of --steps is a real Euler step
    nfe_steps = max(50, args.warmup + args.steps)
    cfgd = dict(LITE, num_visual_blocks=args.blocks)
    with torch.device("meta"):
        dit = DiffusionTransformer3D(**cfgd)
    # weights from per-tensor CPU generator streams (seed 0): the ones oracle/gen_golden_fulldepth.py c2 gave the REFERENCE, so that the
    # timed configuration itself can be checked against the reference's generate() (parity_check below), not just for finiteness
    dit.init_synthetic(dev, seed=0, qk_gain=args.qk_gain, host_rng=True)
    if args.magcache:
        from kandinsky.config import default_configs
        from kandinsky.magcache_utils import set_magcache_params
        cname = {"5s_nocfg": "config_5s_nocfg.yaml", "5s_sft": "config_5s_sft.yaml", "10s_nabla": "config_10s_sft.yaml"}.get(args.workload)
        if cname is None:
            raise SystemExit("--magcache needs a 50-step workload (5s_nocfg, 5s_sft, 10s_nabla)")
        dit.engine(dev)
        set_magcache_params(dit, default_configs()[cname]["magcache"]["mag_ratios"], nfe_steps, abs(wl["w"] - 1.0) <= 1e-6)
    if args.fp8:
        dit.set_fp8(int(args.fp8))
    sp_world = world
    if args.cfg_parallel:
        if world < 2 or world % 2 or abs(wl["w"] - 1.0) <= 1e-6:
            raise SystemExit("--cfg-parallel needs an even number of ranks and a workload with guidance (5s_sft, 10s_hd_sft)")
        from kandinsky.models.parallelize import parallelize_dit
        dit.engine(dev)
        parallelize_dit(dit, rank, world, device=dev, cfg_parallel=True)
        sp_world = world // 2
    elif world > 1 or args.force_sp or args.emulate_shard > 1:
        dit.enable_sequence_parallel(rank, world)
    if args.graph:
        dit.set_graph(True)
    if args.emulate_shard > 1:
        dit.set_option("emulate_world", args.emulate_shard)
    if args.sp_slices > 1:
        dit.set_option("sp_slices", args.sp_slices)
    if args.sp_autotune:
        dit.set_option("sp_autotune", 1)
    for kv in args.engine_option:
        dit.set_option(kv.split("=")[0], int(kv.split("=")[1]))
    if args.attn_online:
        dit.set_option("attn_mode", 1)

    # inputs from CPU generators (reproducible by the golden generator): the reference's own seeded noise (generation_utils.py:97-99, seed
    # 6554) and bf16-representable text embeddings
    noise = torch.randn(T, H, W, 16, generator=torch.Generator().manual_seed(6554))
    latent = noise.to(dev)
    g = torch.Generator().manual_seed(6555)
    te = {"text_embeds": torch.randn(L, 3584, generator=g).bfloat16().to(dev), "pooled_embed": torch.randn(1, 768, generator=g).bfloat16().to(dev)}
    ne = {"text_embeds": torch.randn(wl["Lnull"], 3584, generator=g).bfloat16().to(dev),
          "pooled_embed": torch.randn(1, 768, generator=g).bfloat16().to(dev)}
    vpos = [torch.arange(T), torch.arange(H // 2), torch.arange(W // 2)]
    tpos, ntpos = torch.arange(L), torch.arange(wl["Lnull"])
    from kandinsky.generation_utils import sigma_schedule
    sig = sigma_schedule(nfe_steps, 5.0).tolist()

    sparse = None
    if wl["attn"] == "nabla":
        sparse = {"P": args.nabla_p, "wT": 11, "wH": 3, "wW": 3, "to_fractal": True}

    def run(k0, k):  # k consecutive Euler steps of the 50-step schedule starting at step k0
        dit.sample(latent, sig[k0:k0 + k + 1], te, ne, vpos, tpos, ntpos, wl["w"], scale_factor=(1.0, 2.0, 2.0),
                   sparse_params=sparse)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    # ---- --full: parity of the timed configuration (untimed, before the warm-up): the first two Euler steps of this very model / latent / prompt
    # through k5_sample against the REFERENCE's generate() on the same seeded weights and inputs (fp32 on the host, 32 blocks, 47 616
    # tokens: tests/golden/dit_fulldepth_c2.*, made by oracle/gen_golden_fulldepth.py c2).  Compared on the UPDATE the steps applied
    # (latent - noise): two of fifty steps move the latent by a few percent, the unit-variance noise would hide any error.
    parity = None
    if (args.full and args.workload == "5s_nocfg" and args.blocks == 32 and args.qk_gain == 1.0 and not args.fp8 and args.emulate_shard <= 1
            and not args.magcache and not args.no_parity_check):
        parity = parity_check(dit, noise, dev, sigma_schedule(50, 5.0).tolist(), te, ne, vpos, tpos, ntpos, wl, sparse)   # the golden's NFE 50
    if args.warmup > 0:
        run(0, args.warmup)
    barrier()
    dit.set_profiling(args.profile_level)   # 2: HIP events around the roofline kernel only (one pair per block) inside the timed region
    dit.reset_profile()
    dit.attn_variant_counts(reset=True)
    t0 = time.perf_counter()
    run(args.warmup, args.steps)
    barrier()
    dt = time.perf_counter() - t0
    fuse_used = dit.get_option("attn_fuse_qnorm_used")   # the timed call's choice of where the visual queries are normalised (1: inside the attention kernel from its second step on)
    # ---- the latent the TIMED steps left (before the breakdown pass below moves it on): pinned against a committed value of the same
    # (workload, warm-up + steps) — 512 samples of (latent - noise) + its sum of squares, produced by this engine on an MI355X and tied to
    # the reference through parity_check (same model, same noise, first two steps) and tests/test_gpu_fulldepth.py
    pin = latent_pin(latent, noise, args, world) if args.full or args.write_pin else None
    if args.dump_outputs and rank == 0:   # every rank holds the same latent (rank_check); fp32, 60 MB at most (the 10s_hd latent)
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "latent.npy"), latent.cpu().numpy())
    if world > 1:
        tt = torch.tensor([dt], device="cpu" if host_group else dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = tt.item()
    dit.set_profiling(0)

    sp_on_early = sp_world > 1 or args.force_sp or args.emulate_shard > 1
    FAMS = ("attn_self", "attn_cross", "attn_text", "gemm", "elementwise", "prologue", "epilogue", "comm", "nabla_map")
    fam = {f: dit.get_profile(f) for f in FAMS}
    self_blocks = dit.get_profile("self_blocks")[1]      # visual blocks whose self-attention ran inside the timed region
    fam_steps = args.steps
    n_fixed, n_online = dit.attn_variant_counts()
    nabla_counts = dit.nabla_block_counts() if wl["attn"] == "nabla" else None
    nabla_exec = dit.nabla_executed_blocks() if wl["attn"] == "nabla" and not sp_on_early else None
    if args.full and args.profile_level == 2 and not args.no_breakdown:
        # per-family breakdown from a SEPARATE short pass: an event pair at every family switch (~15 per block) drains the stream
        # each time, which costs the step 1-2 % at one GPU and ~8 % at 8-GPU shard sizes — not something to leave inside `value`
        fam_steps = min(args.steps, 2)
        dit.set_profiling(1)
        dit.reset_profile()
        run(args.warmup, fam_steps)
        barrier()
        dit.set_profiling(0)
        fam_b = {f: dit.get_profile(f) for f in FAMS}
        fam_b["attn_self"] = (fam["attn_self"][0] / args.steps * fam_steps, fam_b["attn_self"][1])   # keep the timed region's figure
        fam_break = fam_b
    else:
        fam_break = fam
    # --full: end-to-end leg (not part of `value`): HunyuanVideo VAE decode of the final latent on the same GPU
    vae_s = None
    if rank == 0 and args.full and not args.no_vae:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from vae_bench import synthetic_vae
        vae = synthetic_vae(dev)
        z = (latent / 0.476986).permute(3, 0, 1, 2)[None].contiguous()      # generation_utils.py:220
        vae._decode_tile(z[:, :, :5]); torch.cuda.synchronize(dev)            # warm-up on one tile (no tiling state touched)
        tv = time.perf_counter()
        img = vae.decode(z).sample
        u8 = ((img.clamp(-1.0, 1.0) + 1.0) * 127.5).to(torch.uint8)          # generation_utils.py:222
        torch.cuda.synchronize(dev)
        vae_s = time.perf_counter() - tv
        assert tuple(u8.shape) == (1, 3, 4 * (T - 1) + 1, 8 * H, 8 * W)
        del vae, img, u8
    attn_ms, attn_n = fam["attn_self"]
    fwd_per_step = 2 if abs(wl["w"] - 1.0) > 1e-6 else 1
    sp_on = sp_world > 1 or args.force_sp or args.emulate_shard > 1
    shard = sp_world if world > 1 else max(args.emulate_shard, 1)      # token shards of ONE forward (CFG-parallel: half of the ranks each)
    # algorithmic FLOPs of the self-attention on THIS rank, from the launches actually MADE (MagCache skips whole block
    # stacks; under sequence parallelism a block's attention is two timed launches: local chunk, then the gathered chunks):
    #   dense: 4 * N^2 * 64 * 28 / shard per block;  NABLA: that times the kept fraction of 64x64 blocks, counted on the device
    #   the number of blocks comes from the engine's own counter (a block is 1 timed launch group on one GPU, 2 under sequence
    #   parallelism, 1 + S with a sliced exchange, 2 with the two-pass NABLA list walk: dividing launches by a guess inflated `frac`)
    blocks_run = self_blocks
    density = None
    if wl["attn"] == "nabla":
        kept, possible = nabla_counts
        density = kept / possible if possible else None
    attn_flop = 4.0 * N * N * 64 * 28 / shard * (density if density is not None else 1.0)
    achieved = attn_flop * blocks_run / (attn_ms * 1e-3) / 1e12 if attn_ms else 0.0
    if args.attn_online:
        variant = "online-max softmax on every head (forced: --attn-online)"
    elif n_fixed + n_online == 0:
        variant = "n/a (no data-derived flags on this path)"
    else:
        variant = (f"fixed-offset softmax on {n_fixed} and online-max on {n_online} of {n_fixed + n_online} (block, head) "
                   f"launches, chosen per head on the device: max|q|*max|k'| <= 190 (centred: max|q|*R) keeps the fixed form (per-row offsets |q|*max|k'| - 90, "
                   f"all zero when the bound is <= 90); beyond 190 the fixed form runs on offsets anchored at sampled scores (one-GPU path) "
                   f"unless the layer's jobs kept falling back")
    traffic, traffic_source = None, None   # HBM-side bytes per attention launch: NOT measured in this run (PMC counters need their own
    for tf in ("r05_attention_traffic.json", "r04_attention_traffic.json", "r03_attention_traffic.json", "r02_attention_traffic.json"):   # rocprofv3 --pmc passes) but read from the committed profile,
        try:                                                                  # and only quoted for the exact workload it was measured on
            with open(os.path.join(ROOT, "profiles", tf)) as f:
                tj = json.load(f)
            if tj.get("tokens") == N and world == 1 and wl["attn"] == "flash" and not args.attn_online and n_online == 0:
                traffic, traffic_source = tj["bytes_per_launch"], f"profiles/{tf} (rocprofv3 --pmc passes of an earlier run of this command, not this run)"
                break
        except Exception:
            pass
    # ... unless this run can measure it itself: --full on the default single-GPU dense workload, on rank 0, after the timed region (nothing here is timed)
    if (rank == 0 and world == 1 and args.full and not args.no_live_traffic and wl["attn"] == "flash" and not args.attn_online and n_online == 0 and args.blocks == 32
            and args.workload == "5s_nocfg" and not args.emulate_shard and not args.fp8 and not args.force_sp and args.qk_gain == 1.0
            and not args.engine_option and not args.magcache and not args.graph
            and not any(k.startswith(("ROCPROF", "ROCPROFILER")) for k in os.environ) and "rocprof" not in os.environ.get("LD_PRELOAD", "")):   # (not under a profiler already)
        lt, lsrc = live_traffic(N)
        if lt is not None:
            traffic, traffic_source = lt, lsrc
        else:
            traffic_source = (traffic_source or "none") + f" [live measurement unavailable: {lsrc}]"
    # the GEMM family (q|k, V^T, out, cross q/out, FF1, FF2 of the visual blocks: 2 * rows * (6 D^2 + 2 D FF) per block on this rank's
    # rows; text-side projections are < 0.1 %) — on the sparse configurations it, not the attention, is the largest family
    g_ms, g_n = fam_break["gemm"]
    rows_rank = N / shard
    gemm_flop_step = self_blocks / max(args.steps, 1) * 2 * rows_rank * (6 * 1792 * 1792 + 2 * 1792 * 7168)   # blocks per step x FLOPs per block
    gemm_roof = None
    if g_ms and gemm_flop_step:
        g_ach = gemm_flop_step / (g_ms / fam_steps * 1e-3) / 1e12
        gemm_roof = {"bound": "mfma", "kernel": "gemm_bf16_w4_kernel / k8 / glds (all linear layers of the visual blocks)", "achieved": g_ach,
                     "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": g_ach / PEAK_BF16_TFLOPS, "ms_per_step": g_ms / fam_steps,
                     "source": "separate per-family pass" if fam_break is not fam else "timed region"}
    invalid = []
    if args.emulate_shard > 1 or dit.get_option("emulated"):
        invalid.append("emulated shard layout (timing only, results garbage)")
    if args.blocks != 32:
        invalid.append("fewer visual blocks than the model")
    fp8_eff = dit.get_option("fp8_effective") if args.fp8 else 0   # the layer classes that really ran in e4m3 (the sharded schedules keep some in bf16)
    if args.fp8:
        invalid.append(f"reduced precision (fp8 linear layers, mask {args.fp8} asked, {fp8_eff} in effect)")
    step_flop = fwd_per_step * flops_forward(N, L, blocks=args.blocks)
    if not torch.isfinite(latent).all():
        invalid.append("the latent holds non-finite values after the timed steps")
    rank_check = None
    if world > 1:   # every rank applies the same Euler update to the same gathered velocity: the latents must be BIT-identical
        cs = torch.stack([latent.double().sum(), latent.double().abs().sum(), latent.view(torch.int32).sum(dtype=torch.int64).double()])
        if host_group:
            cs = cs.cpu()
        allcs = [torch.empty_like(cs) for _ in range(world)]
        torch.distributed.all_gather(allcs, cs)
        same = all(torch.equal(allcs[0], c) for c in allcs)
        rank_check = {"latent_checksums_identical_on_all_ranks": bool(same), "checksum": [float(v) for v in allcs[0].tolist()]}
        if not same:   # a wrong multi-GPU result is not a measurement — but say so in the line instead of dying without one
            rank_check["per_rank"] = [[float(v) for v in c.tolist()] for c in allcs]
            invalid.append("the ranks hold DIFFERENT latents after the timed steps (rank_check.per_rank): the sharded run is wrong")

    if rank == 0:
        out = {
            "metric": "DiT denoising steps/sec (2B Lite, 5s 768x512 latent)", "value": args.steps / dt, "unit": "steps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": f"bf16+fp8 mask {fp8_eff} in effect of {args.fp8} asked (REDUCED PRECISION, not the headline)" if args.fp8 else "bf16", "data": "synthetic",
            "config": {"workload": wl["desc"], "tokens": N, "text_len": L, "forwards_per_step": fwd_per_step,
                       "parallelism": "single GPU" if world == 1 else (
                           (f"CFG-parallel x2 (cond / uncond rank groups, velocity exchange inside k5_sample) x " if args.cfg_parallel else "") +
                           (f"sequence-parallel x{sp_world} (token shards, K/V all-gather)" if args.sp_slices < 2 else
                            f"sequence-parallel x{sp_world} (token shards, K/V exchange in {args.sp_slices} slices)")),
                       **({"hipgraph_step": True} if args.graph else {}),
                       "visual_blocks": args.blocks, "magcache": bool(args.magcache),
                       **({"emulated_shard": args.emulate_shard} if args.emulate_shard > 1 else {}),
                       **({"sp_slices": args.sp_slices} if args.sp_slices > 1 or args.emulate_shard > 1 else {}),
                       **({"engine_options": args.engine_option} if args.engine_option else {}),
                       **({"qk_gain": args.qk_gain} if args.qk_gain != 1.0 else {})},
            "nfe_per_s": fwd_per_step * args.steps / dt,
            "step_tflop": step_flop / 1e12,
            "model_tflops_per_gpu": step_flop * args.steps / dt / 1e12 / world,
            "roofline": {"bound": "mfma", "kernel": "attn_fwd_kernel (visual self-attention, one balanced launch group per block)",
                         "variant": variant, "achieved": achieved, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_BF16_TFLOPS, "traffic": traffic, "traffic_source": traffic_source,
                         "flop_per_launch": attn_flop * blocks_run / max(attn_n, 1), "avg_launch_ms": attn_ms / max(attn_n, 1),
                         "launches": attn_n, "blocks_run": blocks_run, "launches_per_block": attn_n / max(blocks_run, 1),
                         "kept_block_density": density,
                         **({"executed_block_density": nabla_exec / nabla_counts[1], "union_efficiency": nabla_counts[0] / nabla_exec,
                             "achieved_on_executed_tiles": achieved * nabla_exec / nabla_counts[0]} if nabla_exec and nabla_counts and nabla_counts[0] else {})},
            "roofline_gemm": gemm_roof,
            "roofline_attention": None,     # set below when the GEMM family, not the attention, is what bounds this workload's step
            "kernel_time_ms_per_step": {k: v[0] / fam_steps for k, v in fam_break.items() if v[1]},
            "kernel_time_source": ("HIP events inside the timed region" if fam_break is fam else
                                   f"attn_self: HIP events inside the timed region; other families: separate {fam_steps}-step pass with an "
                                   "event pair at every family switch (not part of `value`)"),
            "e2e_clip_s": {"denoise_50_steps_s": 50 * dt / args.steps, "vae_decode_s": vae_s,
                           "total_s": None if vae_s is None else 50 * dt / args.steps + vae_s,
                           "note": "50 x measured ms_per_step + measured HunyuanVideo VAE decode (14 temporal tiles, uint8 out); "
                                   "text encoding excluded (no weights offline); reference README: 77 s on 1xH100 incl. text encoder"},
        }
        # `roofline` names the STEP-DOMINANT kernel family of THIS workload: the attention on the dense configurations, the
        # linear layers' GEMM family on the NABLA configurations at their operating densities — the other one stays in the line under its own key
        attn_ms_step = attn_ms / max(args.steps, 1)
        if gemm_roof is not None and gemm_roof["ms_per_step"] > attn_ms_step:
            out["roofline_attention"] = out["roofline"]
            out["roofline"] = dict(gemm_roof, traffic=None, dominant_because=f"GEMM family {gemm_roof['ms_per_step']:.1f} ms per step > visual self-attention {attn_ms_step:.1f} ms")
        else:
            out.pop("roofline_attention")
        out["full"] = bool(args.full)   # False: a plain run, none of the --full extras ran
        out["parity_check"] = parity
        out["latent_pin"] = pin
        if pin is not None and pin.get("status") == "FAILED":
            invalid.append("the latent after the timed steps differs from the committed pin of this (workload, steps) beyond the stated tolerance (latent_pin)")
        if parity is not None and parity.get("status") == "FAILED":
            invalid.append("the first two steps of this configuration differ from the reference golden beyond the stated tolerance (parity_check)")
        out["attn_fuse_qnorm_used"] = fuse_used   # engine option "attn_fuse_qnorm_auto" (default on): k5_sample's per-call decision after its first step; same bits either way (latent_pin)
        out["ipc_ranks_seen"] = dit.get_option("ipc_ranks")     # processes of the engine's IPC group (k5_dit_comm_init_ipc): N under --transport ipc, else 0
        if out["ipc_ranks_seen"]:
            out["ipc_transport"] = {"collectives": dit.get_option("ipc_collectives"), "pulled_mb_this_rank": dit.get_option("ipc_pulled_mb"),
                                    "flag_wait_timeouts": dit.get_option("ipc_errors"), "ranks_per_device": -(-world // max(ndev, 1))}
            if out["ipc_transport"]["flag_wait_timeouts"]:
                invalid.append("an IPC flag wait ran into its time limit (ipc_transport.flag_wait_timeouts): a peer never signalled")
        if args.oversubscribe and world > ndev:
            invalid.append(f"{world} ranks time-slice {ndev} device(s) (--oversubscribe): a run of the process boundary, not a measurement of a {world}-GPU node")
        out["rccl_ranks_seen"] = dit.get_option("rccl_ranks")   # ncclCommCount of the engine's communicator: N under RCCL, 0 on one GPU, -1 for a loopback / emulated group
        if world > 1:
            out["sp_schedule"] = dit.sp_schedule()     # which exchange the engine's self-tuning picked on this node, and what it measured
        if rank_check is not None:
            out["rank_check"] = rank_check
        if invalid:
            out["INVALID_AS_BENCH"] = invalid
        if args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(N) if world == 1 else None
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
