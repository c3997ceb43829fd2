"""Kernels of the GEMM dispatch on small token counts (BASELINE config 1's shapes):  python tools/gemm_small.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kandinsky-5_amd"))
import torch
from kandinsky import _engine as E
BF = torch.bfloat16
for name, kernel in (("auto   ", 0), ("128x128", 2), ("k8     ", 8), ("w4     ", 4)):
    res = []
    for (M, N, K) in ((3328, 3584, 1792), (1792, 3328, 1792), (3328, 1792, 1792), (3328, 7168, 1792), (3328, 1792, 7168)):
        a, w = torch.randn(M, K, device="cuda").to(BF), (torch.randn(N, K, device="cuda") * 0.05).to(BF)
        out = torch.empty(M, N, dtype=BF, device="cuda")
        for _ in range(3): E.gemm(a, w, None, E.EPI_BIAS, out=out, kernel=kernel)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20): E.gemm(a, w, None, E.EPI_BIAS, out=out, kernel=kernel)
        e.record(); torch.cuda.synchronize()
        res.append(f"{M}x{N}x{K}:{s.elapsed_time(e) / 20 * 1e3:.0f}us")
    print(name, " ".join(res))
