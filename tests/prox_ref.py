"""The rule of proximal guidance on a negative-prompt-inversion edit, restated with torch on the CPU (tests only).

    d = eps_c - eps_u;   lambda_b = the q-quantile of |d| over row b (linear rule, exact order statistics, `control.ledits_rank`)
    rows b >= 1, prox_on:   l0  d' = |d| > lambda_b ? d : 0        l1  d' = d > lambda_b ? d - lambda_b : (d < -lambda_b ? d + lambda_b : 0)
    eps = eps_u + g d';   x0 = (x - sqrt(1 - a_from) eps) / sqrt(a_from)
    rows b >= 1, eta != 0:  m = prox_on ? dilate_r(|d| > lambda_b), per row and channel, zero padding : 1;   x0 = m ? x0 : x0 - eta (x0 - z0)
    x_out = sqrt(a_to) x0 + sqrt(1 - a_to) eps;   row 0 is the plain step

Every comparison is made ONCE, on the fp32 difference fl(eps_c - eps_u) the device forms (a correctly rounded subtraction is the
same number everywhere), and shared by the fp32 and the fp64 restatement: the two differ in the arithmetic only, never in a decision.
"""
import math

import torch
import torch.nn.functional as F

from ief_amd.control import ledits_rank


def quantile_f32(absd, q):
    """absd fp32 [B, n] -> fp32 [B]: sort, the two order statistics, one un-fused interpolation"""
    n = absd.shape[1]
    lo, frac = ledits_rank(q, n)
    s = torch.sort(absd.float(), dim=1).values
    vlo, vhi = s[:, lo], s[:, min(lo + 1, n - 1)]
    return vlo + torch.tensor(frac, dtype=torch.float32) * (vhi - vlo)


def thresholds(eu, ec, q):
    B = eu.shape[0]
    return quantile_f32((ec.float() - eu.float()).abs().reshape(B, -1), q)


def decisions(eu, ec, lam, radius):
    """-> (keep, m) bool [Bp, C, h, w]: |d| > lambda_b on the fp32 difference, and its Chebyshev dilation inside each channel"""
    d = ec.float() - eu.float()
    keep = d.abs() > lam.float().view(-1, 1, 1, 1)
    k = 2 * radius + 1
    m = F.max_pool2d(F.pad(keep.float(), (radius,) * 4, value=0.0), k, stride=1) > 0
    return keep, m


def sqrt_of(v):
    """the correctly rounded square root of a 0-dim tensor in its own dtype: the root is taken in double and rounded once (for fp32
    that is the correctly rounded fp32 root, 53 >= 2 x 24 + 2 bits) -- some CPUs' torch takes a scalar fp32 root an ulp off"""
    return torch.tensor(math.sqrt(float(v)), dtype=v.dtype)


def step(eu, ec, x, coef, lam, z0, mode, radius, dtype):
    """-> (x_out, x0) in `dtype`; coef = the five fp32 numbers {a_from, a_to, g, prox_on, eta}; eu, ec, x fp32 [Bp, C, h, w]"""
    c = torch.tensor([float(v) for v in coef], dtype=torch.float32).to(dtype)
    a_f, a_t, g, on, eta = c[0], c[1], c[2], bool(c[3] != 0), c[4]
    sb_f, sa_f, sa_t, sb_t = sqrt_of(1 - a_f), sqrt_of(a_f), sqrt_of(a_t), sqrt_of(1 - a_t)
    T = lambda t: t.float().to(dtype)
    d32 = ec.float() - eu.float()
    lam32 = lam.float().view(-1, 1, 1, 1)
    keep, m = decisions(eu, ec, lam, radius)
    d, lamv = T(ec) - T(eu), T(lam).view(-1, 1, 1, 1)
    dd = d.clone()
    if on:
        zero = torch.zeros_like(d)
        if mode == "l0":
            dd = torch.where(keep, d, zero)
        else:
            dd = torch.where(d32 > lam32, d - lamv, torch.where(d32 < -lam32, d + lamv, zero))
        dd[0] = d[0]
    eps = T(eu) + g * dd
    x0 = (T(x) - sb_f * eps) / sa_f
    if bool(eta != 0):
        mm = m.clone() if on else torch.ones_like(m)
        mm[0] = True
        x0 = torch.where(mm, x0, x0 - eta * (x0 - T(z0).reshape(1, *x.shape[1:])))
    return sa_t * x0 + sb_t * eps, x0
