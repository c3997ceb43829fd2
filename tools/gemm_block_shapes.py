"""The seven projections of one visual block with their real epilogues, at the token counts of one GPU and of 2/4/8-GPU token shards and
of BASELINE config 1, microseconds per call and per block, for each kernel the dispatch can pick:

    python tools/gemm_block_shapes.py [--tokens 47616,11904,5952,3328] [--kernels auto,4,8] [--token-tile 0] [--iters 20]

(--kernels names kernels as E.gemm(kernel=...): auto = the dispatch's choice, 4 = four-wave persistent, 8 = eight-wave ping-pong, 2 = 128x128;
--token-tile 128 / 192 / 256 forces the four-wave kernel's tile height, 0 = by cost.)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, FF = 1792, 7168


def shapes(M):
    # (name, M, N, K, epilogue)
    return [("q|k", M, 2 * D, D, "bias"), ("V^T", D, M, D, "bias_m"), ("out+gate", M, D, D, "gate"), ("xq", M, D, D, "bias"),
            ("xout+gate", M, D, D, "gate"), ("FF1+GELU", M, FF, D, "gelu"), ("FF2+gate", M, D, FF, "gate")]


def run(M, kernel, tile, iters):
    sys.path.insert(0, os.path.join(ROOT, "kandinsky-5_amd"))
    import torch
    from kandinsky import _engine as E
    BF = torch.bfloat16
    epi = {"bias": E.EPI_BIAS, "bias_m": E.EPI_BIAS_M, "gelu": E.EPI_GELU, "gate": E.EPI_GATE}
    row = {}
    for name, m, n, k, e in shapes(M):
        a = torch.randn(m, k, device="cuda").to(BF)
        w = (torch.randn(n, k, device="cuda") * 0.05).to(BF)
        bias = torch.randn(m if e == "bias_m" else n, device="cuda").to(BF).float()
        resid = torch.randn(m, n, device="cuda").to(BF) if e == "gate" else None
        gate = torch.randn(n, device="cuda") if e == "gate" else None
        out = resid.clone() if e == "gate" else torch.empty(m, n, dtype=BF, device="cuda")
        call = lambda: E.gemm(a, w, bias, epi[e], resid=out if e == "gate" else None, gate=gate, out=out, kernel=kernel, token_tile=tile)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            call()
        t.record()
        torch.cuda.synchronize()
        row[name] = s.elapsed_time(t) / iters * 1e3
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="47616,23808,11904,5952,3328")
    ap.add_argument("--kernels", default="auto,4,8")
    ap.add_argument("--token-tile", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    toks = [int(v) for v in a.tokens.split(",")]
    names = [s[0] for s in shapes(1)]
    print("# us per call; block = sum of the seven; TF = TFLOP/s of the block")
    for kern in a.kernels.split(","):
        for M in toks:
            row = run(M, 0 if kern == "auto" else int(kern), a.token_tile, a.iters)
            tot = sum(row.values())
            flop = sum(2.0 * m * n * k for _, m, n, k, _ in shapes(M))
            print(f"{kern:>5} M={M:6d} " + " ".join(f"{n}:{row[n]:7.1f}" for n in names) + f"  block:{tot:8.1f} us  {flop / tot / 1e6:7.1f} TF")
