"""The float64 definition of regional prompts (include/k5.h: k5_region_weights_f32, k5_region_combine_bf16) and the inputs the kernel tests
share.  No GPU here."""
import torch

BF = torch.bfloat16


def token_weights_reference(masks, base_weight, patch, perm=None):
    """masks (R, T, H, W) in [0, 1] -> float64 (N, R + 1): m_r(token) = mean of the token's patch cells, raw_0 = base_weight +
    max(0, 1 - sum m), raw_r = m_r, w = raw / sum raw; row i = token perm[i] of the row-major (T/pt, H/ph, W/pw) grid (perm None: i)."""
    R, T, H, W = masks.shape
    pt, ph, pw = patch
    m = masks.double().clamp(0.0, 1.0).reshape(R, T // pt, pt, H // ph, ph, W // pw, pw).mean(dim=(2, 4, 6)).reshape(R, -1)
    sm = m.sum(0)
    raw = torch.cat([(float(base_weight) + (1.0 - sm).clamp_min(0.0))[None], m], 0)
    w = (raw / raw.sum(0, keepdim=True)).t().contiguous()
    return w if perm is None else w[torch.as_tensor(perm).long()]


def combine_reference(z0, zr, w):
    """float64 (out, mag): out = sum_i w_i z_i per row over z0 (rows, D) and zr (R, rows, D) with w (rows, >= R + 1); a stream whose weight is 0
    contributes nothing whatever it holds; mag = sum_i |w_i z_i|."""
    z = torch.cat([z0[None], zr], 0).double()
    R1 = z.shape[0]
    wt = w.double()[:, :R1].t()[:, :, None]                                # (R + 1, rows, 1)
    terms = torch.where(wt == 0, torch.zeros_like(z), wt * torch.where(wt == 0, torch.zeros_like(z), z))
    return terms.sum(0), terms.abs().sum(0)


def nabla_perm(Tp, Hp, Wp):
    """the engine's token order under NABLA (forward_impl): 8 x 8 spatial tiles contiguous"""
    Hb, Wb = Hp // 8, Wp // 8
    out = []
    for i in range(Tp * Hp * Wp):
        b, r = i >> 6, i & 63
        t, hb, wb = b // (Hb * Wb), (b // Wb) % Hb, b % Wb
        out.append((t * Hp + hb * 8 + (r >> 3)) * Wp + wb * 8 + (r & 7))
    return torch.tensor(out, dtype=torch.int32)


def combine_inputs(rows, D, R, seed=0, ldw=None):
    """(z0 (rows, D), zr (R, rows, D)) bf16 and w fp32 (rows, ldw): rows cycle through soft weights over all streams, a one-hot row (weight
    exactly 1.0 on stream row % (R + 1)), and a row with some weights exactly 0; every row sums to 1 within fp32."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + D + R)
    z0 = torch.randn(rows, D, generator=g).to(BF)
    zr = (torch.randn(R, rows, D, generator=g) * 1.5).to(BF)
    ldw = R + 1 if ldw is None else ldw
    w = torch.full((rows, ldw), 123.0)                                     # what lies beyond R + 1 columns is not read
    for i in range(rows):
        kind = i % 3
        if kind == 1:
            row = torch.zeros(R + 1)
            row[i % (R + 1)] = 1.0
        else:
            row = torch.rand(R + 1, generator=g) + 0.05
            if kind == 2:
                row[torch.rand(R + 1, generator=g) < 0.5] = 0.0
                if row.sum() == 0:
                    row[0] = 1.0
            row = row / row.sum()
        w[i, :R + 1] = row
    return z0, zr, w


def mask_cases(R, T, H, W, seed=0):
    """masks (R, T, H, W) fp32 that hold every case of the rule: random soft values, a block where the masks overlap with sum > 1, a hole
    (all zero), a block of exact ones on region 0 alone."""
    g = torch.Generator().manual_seed(seed + 31 * R + T + H + W)
    m = torch.rand(R, T, H, W, generator=g) * (1.5 / R)
    m[:, :, : H // 4] = 0.9                                                # overlap: sum = 0.9 R (> 1 for R >= 2)
    m[:, :, H // 4: H // 2] = 0.0                                          # a hole
    m[:, :, H // 2: 3 * H // 4, : W // 2] = 0.0
    m[0, :, H // 2: 3 * H // 4, : W // 2] = 1.0                            # region 0 alone
    return m.clamp_(0.0, 1.0).contiguous()
