"""Enhance-A-Video: the rule of include/k5.h (k5_enhance_scores_bf16) in float64, and the input recipe of the kernel tests.

    z[t][u] = qk_scale <q[t,p,h], k[u,p,h]>        in base-2 units: P = 2^(z - max) normalised over u
    m(p,h)  = sum_{t != u} P[t][u] / (T (T - 1));   mean = mean over (p, h);   score = max(1, mean (T + weight))

`qk_scale` is log2(e) / 8 for plain keys and 1 for keys that already carry that factor, exactly as the kernel takes it.  Host only."""
import math

import torch

K5_SOFTMAX_C = float(torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32))
SHAPES = [(2, 1, 1), (3, 24, 2), (31, 5, 3), (32, 4, 2), (33, 3, 2), (61, 3, 2), (64, 2, 1)]   # (T, S, Hh)
BF = torch.bfloat16


def natural_rows(T, S):
    """frame_rows [S][T] of the natural token order: row = t * S + p"""
    return (torch.arange(T)[None, :] * S + torch.arange(S)[:, None]).long()


def enhance_mean(q, k, T, S, Hh, qk_scale, frame_rows=None, variant=None):
    """The mean off-diagonal mass in float64.  q, k: [rows][>= 64 Hh] (any float dtype; only the rows frame_rows names and the first 64 Hh
    columns are read).  variant (the wrong rules the tests must tell from the right one): "transposed" = softmax over the query axis,
    "shuffled" = the keys of the next spatial column, "flipped" = the keys' heads in reverse order."""
    rows = natural_rows(T, S) if frame_rows is None else frame_rows.long()
    qq = q[rows.reshape(-1)][:, :64 * Hh].double().reshape(S, T, Hh, 64)
    kk = k[rows.reshape(-1)][:, :64 * Hh].double().reshape(S, T, Hh, 64)
    if variant == "shuffled":
        kk = kk.roll(1, 0)
    if variant == "flipped":
        kk = kk.flip(2)
    z = torch.einsum("pthd,puhd->phtu", qq, kk) * float(qk_scale)
    dim = -2 if variant == "transposed" else -1
    P = torch.softmax(z * math.log(2.0), dim=dim)
    off = P.sum((-1, -2)) - P.diagonal(dim1=-2, dim2=-1).sum(-1)
    return float((off / (T * (T - 1))).mean())


def enhance_score(q, k, T, S, Hh, qk_scale, weight, frame_rows=None, variant=None):
    """score = max(1, mean (T + weight)), float64"""
    return max(1.0, enhance_mean(q, k, T, S, Hh, qk_scale, frame_rows, variant) * (T + float(weight)))


# The draw of each kernel-test shape: 1000 T + 10 S + Hh + 100000 n with the smallest n at which, in the float64 rule alone, every wrong variant
# that is not the identity on the shape moves the mean by >= 2e-3 relative and the score at weight 4 is > 1.02 (so the clamp hides nothing).
SEED_N = {(2, 1, 1): 1, (3, 24, 2): 0, (31, 5, 3): 1, (32, 4, 2): 3, (33, 3, 2): 2, (61, 3, 2): 6, (64, 2, 1): 3}


def enhance_inputs(T, S, Hh, gain=3.0):
    """q = bf16(gain N(0,1)), k = bf16(N(0,1)), [T S][64 Hh], seeded per shape.  The gain matters: at gain 1 the logits are so flat that a wrong
    softmax axis or a wrong column pairing moves the mean by less than the bound."""
    g = torch.Generator().manual_seed(1000 * T + 10 * S + Hh + 100000 * SEED_N.get((T, S, Hh), 0))
    q = (gain * torch.randn(T * S, 64 * Hh, generator=g)).to(BF)
    k = torch.randn(T * S, 64 * Hh, generator=g).to(BF)
    return q, k


def onehot_inputs(T, S, Hh, value=40.0):
    """q = k = value * onehot(t): every frame attends to itself alone, the mean is 0 (to 2^-288) and the score clamps at exactly 1"""
    q = torch.zeros(T, S, Hh, 64)
    for t in range(T):
        q[t, :, :, t] = value
    q = q.reshape(T * S, 64 * Hh).to(BF)
    return q, q.clone()


def lay_out(q, k, T, S, Hh, fused, permuted, prescaled, fill=0.0):
    """The buffers as a kernel test hands them over: (Q view, K view, ldq, ldk, frame_rows | None, qk_scale, backing tensors).  fused: one
    [rows][2 * 64 Hh] buffer, otherwise two with 16 columns to spare; permuted: the token rows at random places of a buffer with 7 rows more;
    prescaled: the keys multiplied by K5_SOFTMAX_C on the host (fp32 product, rounded to bf16) and qk_scale 1.  Everything the table does not
    name, and every column past 64 Hh of the separate buffers, holds `fill` (NaN in the poison test)."""
    N, D = T * S, 64 * Hh
    if prescaled:
        k = (k.float() * K5_SOFTMAX_C).to(BF)
    total = N + 7 if permuted else N
    g = torch.Generator().manual_seed(7 + T)
    place = torch.randperm(total, generator=g)[:N] if permuted else torch.arange(N)
    if fused:
        buf = torch.full((total, 2 * D), fill, dtype=BF)
        buf[place, :D], buf[place, D:] = q, k
        back = (buf,)
        ldq = ldk = 2 * D
    else:
        bq, bk = torch.full((total, D + 16), fill, dtype=BF), torch.full((total, D + 24), fill, dtype=BF)
        bq[place, :D], bk[place, :D] = q, k
        back = (bq, bk)
        ldq, ldk = D + 16, D + 24
    rows = place[natural_rows(T, S)] if permuted else None
    return dict(back=back, fused=fused, D=D, ldq=ldq, ldk=ldk, frame_rows=rows, qk_scale=1.0 if prescaled else K5_SOFTMAX_C, q=q, k=k)
