"""The three LEDITS++ rules (`csrc/ledits.hip`) restated in torch on the CPU, sort-based, every operation a separate rounded torch
op in the kernels' order -- in fp32 the restatement and the kernels agree bit for bit on the same inputs.  Imported by
`test_ledits_host.py` and `test_gpu_ledits.py`; not a test file."""
import numpy as np
import torch


def quantile_threshold(v, lo, frac):
    """t = v_(lo) + frac (v_(hi) - v_(lo)), hi = min(lo + 1, n - 1), over the flat tensor v, in v's dtype; -> (t, v_(lo), v_(hi))"""
    sv = torch.sort(v.flatten()).values
    n = sv.numel()
    lo = int(lo)
    hi = min(lo + 1, n - 1)
    vlo, vhi = sv[lo], sv[hi]
    return vlo + torch.tensor(float(frac), dtype=v.dtype) * (vhi - vlo), vlo, vhi


def attn_mask(acc, taps, rank, padding="reflect"):
    """acc fp32 [E, 256], taps fp32 [9], rank [E, 2] -> (m1 fp32 [E, 256] of 0 / 1, smoothed fp32 [E, 256], thresholds fp32 [E]).
    padding: the rule is REFLECT; "replicate" / "constant" exist so a test can show that the border decides bits"""
    E = acc.shape[0]
    img = acc.reshape(E, 1, 16, 16)
    pad = torch.nn.functional.pad(img, (1, 1, 1, 1), mode=padding)[:, 0]
    sm = torch.zeros(E, 16, 16, dtype=acc.dtype)
    for dy in range(3):
        for dx in range(3):
            sm = sm + taps[dy * 3 + dx] * pad[:, dy:dy + 16, dx:dx + 16]
    sm = sm.reshape(E, 256)
    ts = torch.stack([quantile_threshold(sm[e], rank[e, 0].item(), rank[e, 1].item())[0] for e in range(E)])
    return (sm >= ts[:, None]).to(acc.dtype), sm, ts


def spread(m1, H, W):
    """m1 [E, 256] -> [E, H, W]: pixel (y, x) reads cell (floor(16 y / H), floor(16 x / W)); H, W multiples of 16"""
    E = m1.shape[0]
    ys = torch.arange(H) // (H // 16)
    xs = torch.arange(W) // (W // 16)
    return m1.reshape(E, 16, 16)[:, ys][:, :, xs]


def guidance_scores(eps, m1):
    """eps [1 + E, C, H, W] -> s [E, H, W] = sum over channels, in order, of |eps[1 + e] - eps[0]| m"""
    E, C, H, W = eps.shape[0] - 1, eps.shape[1], eps.shape[2], eps.shape[3]
    m = torch.ones(E, H, W, dtype=eps.dtype) if m1 is None else spread(m1, H, W)
    s = torch.zeros(E, H, W, dtype=eps.dtype)
    for c in range(C):
        s = s + (eps[1:, c] - eps[0, c]).abs() * m
    return s, m


def guidance_mask(eps, m1, rank):
    """-> (mask fp32 [E, H, W] of 0 / 1, thresholds fp32 [E] or None, s [E, H, W]); rank None: the spread cell mask"""
    s, m = guidance_scores(eps, m1)
    if rank is None:
        return m.clone(), None, s
    E = s.shape[0]
    ts = torch.stack([quantile_threshold(s[e], rank[e, 0].item(), rank[e, 1].item())[0] for e in range(E)])
    return ((s >= ts[:, None, None]) & (m != 0)).to(eps.dtype), ts, s


def ddpm_step(eps, mask, scale, x, coef, z, dtype=torch.float32):
    """the masked multi-concept guidance and the eta = 1 update on one latent x [C, H, W] in `dtype`: eps [1 + E, C, H, W], mask
    [E, H, W] or None, scale fp32 [E], coef = fp32 [a_from, a_to, sigma, dir], z [C, H, W] the noise row; -> (x_out, x0).  fp32:
    the kernel's operations one by one (tensor divisors: an IEEE division); fp64: the reference of the error bounds."""
    t = lambda v: torch.tensor(float(np.float32(v)), dtype=dtype)
    e = eps.to(dtype)
    u = e[0]
    g = torch.zeros_like(u)
    for k in range(e.shape[0] - 1):
        sc = float(scale[k])
        if sc == 0.0:
            continue
        m = torch.ones((), dtype=dtype) if mask is None else mask[k].to(dtype)[None]
        g = g + (t(sc) * m) * (e[1 + k] - u)
    ee = u + g
    a, p, sigma, dirc = (t(v) for v in coef.tolist())
    # the three square roots through numpy (IEEE, correctly rounded, as the kernel's): torch.sqrt on the CPU was measured one ulp
    # off for sqrt(1 - 0.55f) on one machine, which moved half of the x0 bits
    nt = np.float32 if dtype == torch.float32 else np.float64
    root = lambda v: torch.tensor(float(np.sqrt(nt(v))), dtype=dtype)
    sb_f, sa_f, sa_t = root(nt(1) - nt(float(a))), root(float(a)), root(float(p))
    x0 = (x.to(dtype) - sb_f * ee) / sa_f
    mu = sa_t * x0 + dirc * ee
    return (mu if float(sigma) == 0.0 else mu + sigma * z.to(dtype)), x0
