"""Two-level sequence parallelism ("sp_mode" = 2) on the GPU: G = gcd(28, P) head groups x P / G query splits — the head-split schedule that
is admissible at P = 8 (4 groups of 7 heads x 2 splits) and P = 6 (2 x 3), where Ulysses needs heads % P == 0.  Loopback ranks (P handles, P
host threads, one process) and the IPC transport (P processes on the one device, torch.distributed.run)."""
import json
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import k5_oracle as O  # noqa: E402
from kit import rel  # noqa: E402
from test_gpu_loopback import run_cfg_ranks, run_ranks, tiny_cfg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "golden")


def _full_width(gain, T, W, seed=3):
    from kandinsky.models.dit import DiffusionTransformer3D
    c = dict(O.LITE_2B, num_visual_blocks=2, num_text_blocks=1)
    cfg = O.DitConfig(**c)
    sd = O.synthetic_state_dict(cfg, seed=seed)
    if gain != 1.0:
        for k in sd:
            if k.endswith(("query_norm.weight", "key_norm.weight")):
                sd[k] = sd[k] * gain
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, 16, W, 16, generator=g)
    text, pooled = torch.randn(37, 3584, generator=g), torch.randn(1, 768, generator=g)
    pos = [torch.arange(T), torch.arange(8), torch.arange(W // 2)]
    t = torch.tensor([875.0])

    def make():
        d = DiffusionTransformer3D(**c)
        d.load_state_dict(sd, assign=True)
        return d.to("cuda:0")

    def fwd(d):
        return d(x.cuda(), text.cuda(), pooled.cuda(), t, pos, torch.arange(37), scale_factor=(1.0, 2.0, 2.0))

    def oracle():   # keys pre-scaled before their bf16 rounding, as the engine does
        xin = torch.cat([x, torch.zeros(T, 16, W, 17)], dim=-1)
        O.PRESCALE_K = True
        try:
            return O.dit_forward(sd, cfg, xin, text, pooled, t, pos, torch.arange(37), (1.0, 2.0, 2.0), None, "bf16")
        finally:
            O.PRESCALE_K = False
    return make, fwd, oracle


# ------------------------------------------------------------------------------------------ 1. full width, loopback ranks
@pytest.mark.timeout(900)
@pytest.mark.parametrize("P,T,W,gain", [(8, 5, 48, 1.0), (8, 5, 48, 3.0), (8, 5, 48, 6.0), (6, 11, 16, 1.0), (6, 11, 16, 3.0), (6, 11, 16, 6.0)])
def test_full_width_forward_two_level(P, T, W, gain):
    """28 heads, 2 visual blocks.  P = 8: 15 blocks of 64 tokens, 7 x 2 + 1 (G = 4, splits of ranks 0-3 / 4-7, the second split's last shard short);
    P = 6: 11 blocks, 5 x 2 + 1 (G = 2, three splits).  gain 1 / 3 / 6 on the QK norms: fixed offsets, per-row offsets, anchored offsets — the
    head-group flags come from the world-wide maxima.  Every rank attends only its head group (2 blocks x 28 / G heads counted)."""
    make, fwd, oracle = _full_width(gain, T, W)
    G = math.gcd(28, P)

    def call(d, r):
        return fwd(d), d.attn_variant_counts(), d.get_option("sp_mode_used")

    one = make()
    fused = fwd(one)
    one._destroy_engine(force=True)
    res = run_ranks(P, make, call, options={"sp_mode": 2})
    outs = [o for o, _, _ in res]
    assert all(m == 2 for _, _, m in res), [m for _, _, m in res]
    for r in range(1, P):
        assert torch.equal(outs[r], outs[0]), f"rank {r} differs from rank 0"
    for r, (_, (n_fixed, n_online), _) in enumerate(res):
        assert n_fixed + n_online == 2 * 28 // G, (r, n_fixed, n_online)
    ref = oracle()
    print(f"two-level P={P} (G={G}) gain={gain}: vs single handle {rel(outs[0], fused):.3e}; vs oracle {rel(outs[0], ref):.3e} "
          f"(single handle vs oracle {rel(fused, ref):.3e}); "
          f"rank-0 heads fixed / online {res[0][1]}")
    assert rel(outs[0], fused) <= {1.0: 3e-3, 3.0: 1.5e-2, 6.0: 6e-2}[gain], rel(outs[0], fused)
    assert rel(outs[0], ref) <= {1.0: 1.5e-2, 3.0: 3e-2, 6.0: 1.2e-1}[gain], (rel(outs[0], ref), rel(fused, ref))


# ------------------------------------------------------------------------------------------ 2. fallbacks and edges
@pytest.mark.timeout(900)
def test_two_level_runs_ulysses_where_the_heads_divide():
    """P = 4 (G = 4 = P): "sp_mode" 2 is the Ulysses routine — the same bits as "sp_mode" 1."""
    make, fwd, _ = _full_width(1.0, 5, 32)

    def call(d, r):
        return fwd(d), d.get_option("sp_mode_used")
    a = run_ranks(4, make, call, options={"sp_mode": 1})
    b = run_ranks(4, make, call, options={"sp_mode": 2})
    assert all(m == 1 for _, m in a) and all(m == 1 for _, m in b)
    assert torch.equal(a[0][0], b[0][0])


@pytest.mark.timeout(900)
def test_two_level_falls_back_to_the_gather():
    """P = 3 (gcd(28, 3) = 1) on the full-width model: "sp_mode" 2 runs the gather — the bits of "sp_mode" 0, and "sp_mode_used" says so."""
    make, fwd, _ = _full_width(1.0, 5, 32)

    def call(d, r):
        return fwd(d), d.get_option("sp_mode_used")
    a = run_ranks(3, make, call, options={"sp_mode": 0})
    b = run_ranks(3, make, call, options={"sp_mode": 2})
    assert all(m == 0 for _, m in a) and all(m == 0 for _, m in b)
    assert torch.equal(a[0][0], b[0][0])


@pytest.mark.timeout(900)
def test_two_level_nabla_keeps_the_gather(golden_meta, tiny_sd):
    """NABLA at P = 8 on the tiny model (2 heads: G = 2 would be two-level for dense attention): the gather, as under "sp_mode" 0."""
    from kandinsky.models.dit import DiffusionTransformer3D
    c = tiny_cfg(golden_meta)
    T = 8
    g = torch.Generator().manual_seed(108)
    x = torch.randn(T, 16, 16, 33, generator=g)
    text, pooled = torch.randn(9, 96, generator=g), torch.randn(1, 48, generator=g)
    pos = [torch.arange(T), torch.arange(8), torch.arange(8)]
    sp = {"P": 0.6, "wT": 3, "wH": 3, "wW": 3, "to_fractal": True}

    def make():
        d = DiffusionTransformer3D(**c)
        d.load_state_dict(tiny_sd, assign=True)
        return d.to("cuda:0")

    def call(d, r):
        out = d(x.cuda(), text.cuda(), pooled.cuda(), torch.tensor([432.0]), pos, torch.arange(9), scale_factor=(1.0, 2.0, 2.0), sparse_params=sp)
        return out, d.get_option("sp_mode_used")
    a = run_ranks(8, make, call, options={"sp_mode": 0})
    b = run_ranks(8, make, call, options={"sp_mode": 2})
    assert all(m == 0 for _, m in a) and all(m == 0 for _, m in b)
    assert torch.equal(a[0][0], b[0][0])


@pytest.mark.timeout(900)
def test_fp8_effective_follows_the_two_level_dispatch():
    """k5_dit_set_fp8 mask 3 (feed-forward + q | k | V^T): the two-level schedule keeps the q | k | V^T projections in bf16 like Ulysses, so
    "fp8_effective" reads 1 at P = 8 (two-level) and 3 at P = 3 (gather)."""
    make, fwd, _ = _full_width(1.0, 5, 48)

    def call(d, r):
        d.set_fp8(3)
        out = fwd(d)
        return d.get_option("sp_mode_used"), d.get_option("fp8_effective"), bool(torch.isfinite(out.float()).all())
    for P, mode, eff in ((8, 2, 1), (3, 0, 3)):
        res = run_ranks(P, make, call, options={"sp_mode": 2})
        assert all(r == (mode, eff, True) for r in res), (P, res)


@pytest.mark.timeout(900)
def test_two_level_emulated_world_8():
    """emulate_world 8 (timing-only layout of rank 0, a world = 1 communicator): the two-level schedule runs, the handle is marked emulated, and it
    attends 7 heads per block (G = 4)."""
    make, fwd, _ = _full_width(1.0, 5, 48)

    def call(d, r):
        fwd(d)
        return d.get_option("emulated"), d.get_option("sp_mode_used"), d.attn_variant_counts()
    (emu, used, (n_fixed, n_online)), = run_ranks(1, make, call, options={"emulate_world": 8, "sp_mode": 2})
    assert emu == 1 and used == 2
    assert n_fixed + n_online == 2 * 7, (n_fixed, n_online)


# ------------------------------------------------------------------------------------------ 3. config 1 in full, 8 loopback ranks
@pytest.mark.timeout(1500)
def test_config1_full_depth_two_level_8_loopback_ranks():
    """BASELINE config 1 in full (32 visual blocks x 16 steps, the reference's generate() golden dit_fulldepth_c1) as 8 loopback ranks on the
    two-level schedule (G = 4: 7 heads per rank, 2 query splits); ranks bit-identical (loopback_latent checks it)."""
    from safetensors.torch import load_file
    from test_gpu_ipc_ranks import loopback_latent
    meta = json.load(open(os.path.join(HERE, "dit_fulldepth_meta.json")))
    c, G = meta["c1"], load_file(os.path.join(HERE, "dit_fulldepth_c1.safetensors"))
    lat = loopback_latent(8, c, c["w"], None, meta, options={"sp_mode": 2})
    got = lat.reshape(-1)[G["sample_idx"]]
    r_ref, r_16, yard = rel(got, G["final_ref"]), rel(got, G["final_bf16_oracle"]), c["bf16_oracle_vs_ref_final"]
    print(f"config 1, 8 loopback ranks, two-level: vs reference fp32 {r_ref:.3e}, vs bf16-island oracle {r_16:.3e} (oracle vs reference {yard:.3e})")
    assert r_ref <= max(1.5 * yard, 1e-2) and r_16 <= max(1.5 * yard, 1e-2), (r_ref, r_16, yard)


# ------------------------------------------------------------------------------------------ 4. sampler with the CFG pair
@pytest.mark.timeout(900)
def test_tiny_sampler_two_level_with_cfg_pair(golden_meta, tiny_sd):
    """k5_sample, 4 steps, guidance 5, as 2 x 4 handles: the tiny model's 2 heads over 4 ranks = G 2 x 2 splits inside each CFG branch + the
    pairs' velocity exchange — all 8 handles hold the same latent, within 1e-2 of the single handle."""
    from types import SimpleNamespace as NS
    from kandinsky.generation_utils import generate
    from kandinsky.models.dit import DiffusionTransformer3D
    c = tiny_cfg(golden_meta)
    g = torch.Generator().manual_seed(7)
    shape = (8, 16, 16, 16)
    noise = torch.randn(*shape, generator=g)
    te = {"text_embeds": torch.randn(9, 96, generator=g).cuda(), "pooled_embed": torch.randn(1, 48, generator=g).cuda()}
    ne = {"text_embeds": torch.randn(4, 96, generator=g).cuda(), "pooled_embed": torch.randn(1, 48, generator=g).cuda()}
    pos = [torch.arange(8), torch.arange(8), torch.arange(8)]
    conf = NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))

    def make():
        d = DiffusionTransformer3D(**c)
        d.load_state_dict(tiny_sd, assign=True)
        return d.to("cuda:0")

    def call(d, i):
        lat = generate(d, "cuda:0", shape, 4, te, ne, pos, torch.arange(9), torch.arange(4), 5.0, 5.0, conf, noise=noise)
        return lat, d.get_option("sp_mode_used")

    fused, _ = call(make(), 0)
    outs = run_cfg_ranks(4, make, call, options={"sp_mode": 2})
    assert all(m == 2 for _, m in outs), [m for _, m in outs]
    for i in range(1, 8):
        assert torch.equal(outs[i][0], outs[0][0]), i
    assert rel(outs[0][0], fused) <= 1e-2, rel(outs[0][0], fused)


# ------------------------------------------------------------------------------------------ 5. processes over IPC
def _launch(P, case, out, sp_mode, extra=(), timeout=1200):
    """tests/ipc_rank_worker.py under torch.distributed.run, the schedule chosen the way a user's launch line chooses it: K5_SP_MODE"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={P}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "ipc_rank_worker.py"), "--case", case, "--out", out] + list(extra)
    env = dict(os.environ, K5_SP_TRANSPORT="ipc", K5_OVERSUBSCRIBE="1", K5_IPC_TIMEOUT_S="120", K5_SP_MODE=str(sp_mode),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    pr = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        log, _ = pr.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        import signal
        os.killpg(pr.pid, signal.SIGKILL)
        log, _ = pr.communicate()
        pytest.fail(f"{P} ranks did not finish within {timeout} s:\n{log[-3000:]}")
    assert pr.returncode == 0, f"torch.distributed.run exited with {pr.returncode}:\n{log[-4000:]}"
    rc = json.load(open(os.path.join(out, "rank_check.json")))
    assert rc["rank_check"]["latent_checksums_identical_on_all_ranks"], rc
    assert all(r["ipc_ranks"] == P and r["ipc_errors"] == 0 for r in rc["ranks"]), rc["ranks"]
    return rc["ranks"], torch.load(os.path.join(out, "latent_rank0.pt"))


def _predicted_bytes(P, blocks, n_pad, sched, collectives):
    """bytes a rank pulls over a sampling run (the first rank: every rank pulls the same here), from the plan: per forward and visual block the
    self-attention exchanges + the |q|^2 / |k'|^2 maxima, per forward the velocity gather.  Forwards = collectives / collectives per forward."""
    from kandinsky import _engine as E
    import ctypes as C
    H, D, Fout = 28, 1792, 64
    vel = (P - 1) * n_pad * Fout * 2
    if sched == 2:
        sa = 0
        for which in range(4):
            tab = (C.c_longlong * (3 * P * P))()
            assert E.lib().k5_sp_plan_2d(H, P, n_pad, D, which, None, tab) == 2
            sa += sum(tab[3 * (s * P + 0) + 2] for s in range(1, P))      # what rank 0 pulls from its peers
        stats, per_fwd = (P - 1) * 2 * H * 4, 5 * blocks + 1
    else:
        sa, stats, per_fwd = 2 * (P - 1) * n_pad * D * 2, (P - 1) * H * 4, 3 * blocks + 1
    F = collectives // per_fwd
    return F, sa, F * (blocks * (sa + stats) + vel)


@pytest.mark.timeout(1500)
def test_processes_two_level_config1_full_depth():
    """config 1 in full as 6 PROCESSES with K5_SP_MODE=2 (G = 2, three splits): bit for bit what 6 loopback ranks give, within the reference bound,
    and each rank pulls what the plan predicts."""
    import tempfile
    from safetensors.torch import load_file
    from test_gpu_ipc_ranks import loopback_latent
    meta = json.load(open(os.path.join(HERE, "dit_fulldepth_meta.json")))
    c, G = meta["c1"], load_file(os.path.join(HERE, "dit_fulldepth_c1.safetensors"))
    with tempfile.TemporaryDirectory() as tmp:
        ranks, lat = _launch(6, "c1", os.path.join(tmp, "c1"), 2)
    T, H, W = c["latent"]
    N = T * (H // 2) * (W // 2)
    n_pad = -(-(N // 64) // 6) * 64
    F, _, pred = _predicted_bytes(6, 32, n_pad, 2, ranks[0]["ipc_collectives"])
    print(f"6 processes, two-level, config 1: {F} forwards, {ranks[0]['ipc_pulled_mb']} MB pulled per rank, plan {pred / 2**20:.1f} MB")
    assert all(abs(r["ipc_pulled_mb"] - pred / 2**20) <= F for r in ranks), [r["ipc_pulled_mb"] for r in ranks]
    got = lat.reshape(-1)[G["sample_idx"]]
    r_ref, r_16, yard = rel(got, G["final_ref"]), rel(got, G["final_bf16_oracle"]), c["bf16_oracle_vs_ref_final"]
    print(f"  vs reference fp32 {r_ref:.3e}, vs bf16-island oracle {r_16:.3e} (oracle vs reference {yard:.3e})")
    assert r_ref <= max(1.5 * yard, 1e-2) and r_16 <= max(1.5 * yard, 1e-2), (r_ref, r_16, yard)
    loop = loopback_latent(6, c, c["w"], None, meta, options={"sp_mode": 2})
    assert torch.equal(loop, lat), f"the processes and the loopback ranks disagree: {rel(lat, loop):.3e}"


@pytest.mark.timeout(1500)
def test_processes_two_level_bytes_and_captured_step():
    """The 2-block model on config 1's shapes as 6 processes (rows_pad = 576, Dp = 896): the two-level run pulls what its plan says, its
    self-attention share is 0.60 of a gather run's (per block 12 against 20 blocks of 576 x 896 x 2 B), and a captured step replays to the eager bits."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        r2, lat2 = _launch(6, "c1", os.path.join(tmp, "two"), 2, ["--tiny"])
        r0, lat0 = _launch(6, "c1", os.path.join(tmp, "gather"), 0, ["--tiny"])
        rg, latg = _launch(6, "c1", os.path.join(tmp, "graph"), 2, ["--tiny", "--graph"])
    n_pad = 576
    F2, sa2, pred2 = _predicted_bytes(6, 2, n_pad, 2, r2[0]["ipc_collectives"])
    F0, sa0, pred0 = _predicted_bytes(6, 2, n_pad, 0, r0[0]["ipc_collectives"])
    assert F2 == F0
    assert sa2 * 5 == sa0 * 3 and sa2 == 12 * n_pad * 896 * 2, (sa2, sa0)   # 12 against 20 blocks of 576 x 896 x 2 B
    m2, m0 = r2[0]["ipc_pulled_mb"], r0[0]["ipc_pulled_mb"]
    print(f"6 processes, 2 blocks x {F2} forwards: two-level {m2} MB (plan {pred2 / 2**20:.1f}), gather {m0} MB (plan {pred0 / 2**20:.1f})")
    assert all(abs(r["ipc_pulled_mb"] - pred2 / 2**20) <= F2 for r in r2)
    assert all(abs(r["ipc_pulled_mb"] - pred0 / 2**20) <= F0 for r in r0)
    vel = F2 * 5 * n_pad * 64 * 2 / 2**20
    share = (m2 - vel) / (m0 - vel)
    assert abs(share - 0.6) <= 0.01, share
    assert torch.equal(latg, lat2), f"captured-step replay differs from eager: {rel(latg, lat2):.3e}"
