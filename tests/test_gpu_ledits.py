"""LEDITS++ on a real MI355X: the three launches of `csrc/ledits.hip` (`ief_ledits_attn_mask_f32`, `ief_ledits_guidance_mask_f32`,
`ief_ledits_ddpm_step_f32`), the unconditional-only noise-map extraction, the captured loop, the sampler and the PIE driver.

The kernel tests compare with the torch fp32 restatement (`tests/ledits_ref.py`, sort-based, on the CPU) fed the SAME inputs, so they
are exact: every threshold and every mask bit equal bit for bit, no pixel excluded.  Stated checks (every test prints its figures):
    attention mask      E = 3, q in {0, 0.5, 0.9, 1}, peaks at the cells (0, 0) and (15, 15): bit-equal
    guidance mask       (C, H, W) in {(4, 16, 16), (4, 32, 32), (4, 32, 48)}, E in {1, 3}, with / without m1, with / without rank,
                        ranks with frac == 0, frac != 0, q = 1, a rank inside the zeros m1 creates (t = 0), tied inputs: bit-equal;
                        distinct values: n - lo - (frac != 0) set pixels
    step                E = 1 without a mask == `cfg_ddpm_step` bit for bit; all scales 0 == that call with g = 0; E = 3 against
                        fp64: max |kernel - fp64| <= 4 x max |restatement - fp64|; outside the union of the masks bit-equal to
                        the all-zero-scale step; 256 and 1024 + 256 elements
    refusals            each returns its code and leaves the outputs untouched
    sampler (`small`, f16x3, 4 steps): reconstruction with no concept active within 4 x the same run with extraction and step written
                        out in torch fp32; graph == eager; a pooled loop run twice and re-pointed == fresh runs; the masks and x_out of
                        one eager step == the restatement on the dumped accumulator and eps; the unconditional-only extraction
                        against both halves at K = 1 and K = 3; `ledits/test.py --synthetic 2`
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
import ledits_ref as ref  # noqa: E402
from ief_amd import hip  # noqa: E402
from ief_amd.control import ledits_rank, ledits_rank_table, ledits_taps  # noqa: E402
from _procs import run_mixed  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "image-editing-framework_amd")
IEF_EINVAL, IEF_ESHAPE, IEF_EALIGN = -1, -2, -3          # csrc/ief_common.h
A_F, A_T = 0.55, 0.71
STEPS = 4
CONCEPTS = ["a red hat", "glasses", "snow on the mountain"]


def ddpm_sigma_dir(a, p):
    """fp64 on the host, rounded to fp32 once (`DDIMScheduler.ddpm_coeffs`)"""
    a, p = np.float64(np.float32(a)), np.float64(np.float32(p))
    v = (1 - p) / (1 - a) * (1 - a / p)
    return float(np.float32(np.sqrt(v))), float(np.float32(np.sqrt(1 - p - v)))


def rank_rows(rows):
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------- a. the attention mask
@pytest.mark.parametrize("q", [0.0, 0.5, 0.9, 1.0])
def test_attn_mask_kernel_equals_the_restatement(q):
    g = torch.Generator().manual_seed(int(100 * q) + 1)
    acc = torch.rand(3, 256, generator=g) + 0.25
    acc[0, 0] = 40.0                       # the peak at cell (0, 0): its neighbours are smoothed through the reflected border
    acc[1, 255] = 40.0                     # and at (15, 15)
    taps, rank = ledits_taps(), ledits_rank_table([q] * 3, 256)
    want, sm, ts = ref.attn_mask(acc, taps, rank)
    got = hip.ledits_attn_mask(acc.to(DEV), taps.to(DEV), rank.to(DEV), out=torch.full((3, 256), float("nan"), device=DEV)).cpu()
    print(f"q = {q}: set cells per concept {[int(v) for v in got.sum(1)]}, thresholds {[f'{v:.6g}' for v in ts.tolist()]}")
    assert torch.equal(got, want), f"{int((got != want).sum())} cells differ"
    if q == 0.0:
        assert (got == 1).all(), "q = 0: every cell is set"
    if q == 1.0:
        assert torch.equal(got, (sm == sm.max(1, keepdim=True).values).float()), "q = 1: only the maxima"
        assert got[0, 0] == 1 and got[1, 255] == 1
    if q in (0.5, 0.9):
        # the border decides bits: the same rule with another padding gives other masks on these inputs
        for other in ("replicate", "constant"):
            assert not torch.equal(ref.attn_mask(acc, taps, rank, padding=other)[0], want), other
    acc16 = acc.reshape(3, 16, 16).to(DEV)
    assert torch.equal(hip.ledits_attn_mask(acc16, taps.to(DEV), rank.to(DEV)).cpu().reshape(3, 256), want)


# ------------------------------------------------------------------------------------------------------------- b. the guidance mask
def guidance_case(E, C, H, W, seed, tied=False):
    g = torch.Generator().manual_seed(seed)
    if tied:          # s takes 32 levels exactly: eps_u = 0, every channel of concept e holds +- level / C (C = 4: exact)
        level = torch.randint(0, 32, (E, 1, H, W), generator=g).float()
        sign = torch.where(torch.rand(E, C, H, W, generator=g) > 0.5, 1.0, -1.0)
        eps = torch.cat([torch.zeros(1, C, H, W), sign * (level / C)])
    else:
        eps = torch.randn(1 + E, C, H, W, generator=g)
        s, _ = ref.guidance_scores(eps, None)
        if any(s[e].unique().numel() != H * W for e in range(E)):          # two of a thousand fp32 sums can coincide: the next seed
            return guidance_case(E, C, H, W, seed + 1)
    m1 = (torch.rand(E, 256, generator=g) > 0.45).float()
    return eps, m1


@pytest.mark.parametrize("use_m1", [False, True])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("shape", [(4, 16, 16), (4, 32, 32), (4, 32, 48)])
def test_guidance_mask_kernel_equals_the_restatement(shape, E, use_m1):
    C, H, W = shape
    n = H * W
    eps, m1 = guidance_case(E, C, H, W, 7 * n + E)
    m1 = m1 if use_m1 else None
    zeros = 0 if m1 is None else int((ref.spread(m1, H, W) == 0).sum(dim=(1, 2)).min())
    variants = {"frac == 0": (n // 2, 0.0), "frac != 0": ledits_rank(0.9, n), "q = 1": (n - 1, 0.0), "small rank": (n // 8, 0.5)}
    if m1 is not None:
        assert zeros > n // 8 + 1, "the small rank must fall inside the zeros m1 creates"
    d_eps, d_m1 = eps.to(DEV), None if m1 is None else m1.to(DEV)
    for name, (lo, frac) in variants.items():
        if name == "frac != 0":
            assert frac != 0.0
        rank = rank_rows([[lo, frac]] * E)
        want, ts, s = ref.guidance_mask(eps, m1, rank)
        got, th = hip.ledits_guidance_mask(d_eps, d_m1, rank.to(DEV), out=torch.full((E, H, W), float("nan"), device=DEV))
        got, th = got.cpu(), th.cpu()
        print(f"{shape} E = {E} m1 = {use_m1} {name} (lo {lo}, frac {frac}): set {[int(v) for v in got.sum((1, 2))]}, t {[f'{v:.6g}' for v in th.tolist()]}")
        assert torch.equal(th, ts), "the thresholds must be equal bit for bit"
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} pixels differ"
        if m1 is None:
            for e in range(E):
                assert s[e].unique().numel() == n, "the seeded scores are distinct"
                assert int(got[e].sum()) == n - lo - (1 if frac != 0 else 0)
        elif name == "small rank":
            assert (th == 0).all() and torch.equal(got, ref.spread(m1, H, W)), "t = 0: every pixel under m1 is set, none outside"
    # without a rank there is no threshold: m1 spread to the pixels (all ones without m1); thres_out is not touched
    want, none, _ = ref.guidance_mask(eps, m1, None)
    th = torch.full((E,), float("nan"), device=DEV)
    got, ret = hip.ledits_guidance_mask(d_eps, d_m1, None, thres_out=th)
    assert ret is None and none is None and torch.equal(got.cpu(), want) and torch.isnan(th).all()


@pytest.mark.parametrize("use_m1", [False, True])
def test_guidance_mask_sets_every_tie(use_m1):
    E, C, H, W = 3, 4, 32, 48
    n = H * W
    eps, m1 = guidance_case(E, C, H, W, 99, tied=True)
    m1 = m1 if use_m1 else None
    rank = rank_rows([[n // 2, 0.5], [n - 40, 0.25], [n // 2 + n // 4, 0.0]])
    want, ts, s = ref.guidance_mask(eps, m1, rank)
    assert s.unique().numel() <= 32
    got, th = hip.ledits_guidance_mask(eps.to(DEV), None if m1 is None else m1.to(DEV), rank.to(DEV))
    got, th = got.cpu(), th.cpu()
    assert torch.equal(th, ts) and torch.equal(got, want)
    for e in range(E):
        ties = int((s[e] == ts[e]).sum())
        lo = int(rank[e, 0])
        print(f"tied scores, m1 = {use_m1}, concept {e}: t = {ts[e].item()}, {ties} elements equal t, {int(got[e].sum())} set (n - lo = {n - lo})")
        assert ties > 1, "v_(lo) == v_(hi): the threshold is a level many elements sit on"
        under = torch.ones(H, W, dtype=torch.bool) if m1 is None else ref.spread(m1, H, W)[e] != 0
        assert bool(got[e][(s[e] == ts[e]) & under].eq(1).all()), "all ties are set"
        assert int(got[e].sum()) >= (n - lo if m1 is None else 0)


# ------------------------------------------------------------------------------------------------------------- c. the step
def step_case(E, C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    eps, x = r(1 + E, C, h, w), r(1, C, h, w)
    noise = torch.stack([r(C, h, w), 1e-3 * r(C, h, w), 50 * r(C, h, w)])
    mask = (torch.rand(E, h, w, generator=g) > 0.6).float()
    return eps, x, noise, mask


@pytest.mark.parametrize("shape", [(4, 8, 8), (4, 16, 20)])          # 256 elements; 1024 + 256 (a tail)
def test_step_kernel(shape):
    """Measured on an MI355X, E = 3 with masks, scales (5, -3, 0), max |kernel - fp64| and max |torch fp32 restatement on the CPU -
    fp64| (bound 4 x): 256 elements 1.672e-6 and 1.672e-6 with the unit noise row and with the 1e-3 row, 3.805e-6 and 3.805e-6 with
    the 50 x row; 1280 elements 2.330e-6, 2.540e-6, 4.759e-6, the restatement's the same (1.00 x: the two agree bit for bit)."""
    C, h, w = shape
    sigma, dirc = ddpm_sigma_dir(A_F, A_T)
    coef_h = torch.tensor([A_F, A_T, sigma, dirc])
    coef = coef_h.to(DEV)
    eps_h, x_h, noise_h, mask_h = step_case(3, C, h, w, C * h * w)
    eps, x, noise, mask = (t.to(DEV) for t in (eps_h, x_h, noise_h, mask_h))
    nan = lambda t: torch.full_like(t, float("nan"))
    for dev_step, row in ((0, 0), (1, 1), (7, 2), (-1, 0)):
        step = torch.tensor([dev_step], dtype=torch.int32, device=DEV)
        # E = 1, no mask, scale = [g]: the existing CFG + DDPM step, bit for bit
        for gscale in (7.5, -2.0, 0.0):
            x0a, x0b = nan(x), nan(x)
            old = hip.cfg_ddpm_step(eps[:1], eps[1:2], x, coef, torch.tensor([gscale], device=DEV), noise, step, out=nan(x), x0_out=x0a)
            new = hip.ledits_ddpm_step(eps[:2].contiguous(), None, torch.tensor([gscale], device=DEV), x, coef, noise, step, out=nan(x),
                                       x0_out=x0b)
            assert torch.equal(new, old) and torch.equal(x0a, x0b), f"E = 1 without a mask must be cfg_ddpm_step (g = {gscale}, step {dev_step})"
        # all scales 0: that call with g = 0, whatever the masks
        zero = hip.ledits_ddpm_step(eps, mask, torch.zeros(3, device=DEV), x, coef, noise, step)
        assert torch.equal(zero, hip.cfg_ddpm_step(eps[:1], eps[1:2], x, coef, torch.zeros(1, device=DEV), noise, step))
        # E = 3 with masks, one negative scale and one gated concept, against fp64
        scale_h = torch.tensor([5.0, -3.0, 0.0])
        x0k = nan(x)
        out = hip.ledits_ddpm_step(eps, mask, scale_h.to(DEV), x, coef, noise, step, out=nan(x), x0_out=x0k).cpu()[0]
        r32, x032 = ref.ddpm_step(eps_h, mask_h, scale_h, x_h[0], coef_h, noise_h[row])
        r64, _ = ref.ddpm_step(eps_h, mask_h, scale_h, x_h[0], coef_h, noise_h[row], dtype=torch.float64)
        e_k, e_r = (out.double() - r64).abs().max().item(), (r32.double() - r64).abs().max().item()
        print(f"{C * h * w} elements, step {dev_step} (row {row}): max |kernel - fp64| = {e_k:.3e}, restatement {e_r:.3e} ({e_k / e_r:.2f} x, bound 4)")
        assert e_r > 0 and e_k <= 4 * e_r
        assert torch.equal(out, r32) and torch.equal(x0k.cpu()[0], x032), "the restatement states the kernel's operations one by one"
        # a gated concept is skipped, not multiplied: its estimate may hold anything
        poisoned = eps.clone()
        poisoned[3] = float("nan")
        assert torch.equal(hip.ledits_ddpm_step(poisoned, mask, scale_h.to(DEV), x, coef, noise, step).cpu()[0], out)
        # outside the union of the (active) masks nothing but the plain step happens
        outside = ((mask_h[0] + mask_h[1]) == 0)[None].expand(C, h, w)
        assert outside.any() and not outside.all()
        assert torch.equal(out[outside], zero.cpu()[0][outside]) and not torch.equal(out[~outside], zero.cpu()[0][~outside])
        # in place, and a latent without its batch dimension
        xin = x.clone()
        assert hip.ledits_ddpm_step(eps, mask, scale_h.to(DEV), xin, coef, noise, step, out=xin) is xin and torch.equal(xin.cpu()[0], out)
        assert torch.equal(hip.ledits_ddpm_step(eps, mask, scale_h.to(DEV), x[0].contiguous(), coef, noise, step).cpu(), out)
    # sigma = 0: the noise is not read into the result
    coef0 = torch.tensor([A_F, A_T, 0.0, dirc], device=DEV)
    a = hip.ledits_ddpm_step(eps, mask, scale_h.to(DEV), x, coef0, noise, step)
    b = hip.ledits_ddpm_step(eps, mask, scale_h.to(DEV), x, coef0, nan(noise), step)
    assert torch.equal(a, b) and torch.isfinite(a).all()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    lib = hip.load()
    p = lambda t: t.data_ptr()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    nanf = lambda *s: torch.full(s, float("nan"), device=DEV)
    acc, taps, rank = torch.rand(2, 256, device=DEV), ledits_taps().to(DEV), ledits_rank_table([0.9, 0.9], 256).to(DEV)
    m1 = nanf(2, 256)
    a = lambda ac=p(acc), tp=p(taps), rk=p(rank), mo=p(m1), E=2: lib.ief_ledits_attn_mask_f32(ac, tp, rk, mo, E, stream())
    assert a(ac=None) == a(tp=None) == a(rk=None) == a(mo=None) == IEF_EINVAL
    assert a(E=0) == a(E=9) == a(E=-1) == IEF_ESHAPE
    assert a(ac=p(acc) + 2) == a(tp=p(taps) + 1) == a(rk=p(rank) + 3) == a(mo=p(m1) + 2) == IEF_EALIGN

    eps = torch.randn(3, 4, 16, 16, device=DEV)
    cell = torch.ones(2, 256, device=DEV)
    rk = ledits_rank_table([0.9, 0.9], 256).to(DEV)
    mask, th = nanf(2, 16, 16), nanf(2)
    b = lambda ep=p(eps), mm=p(cell), r=p(rk), mo=p(mask), to=p(th), E=2, C=4, H=16, W=16: lib.ief_ledits_guidance_mask_f32(
        ep, mm, r, mo, to, E, C, H, W, stream())
    assert b(mo=None) == b(ep=None) == b(to=None) == IEF_EINVAL
    assert b(E=0) == b(E=9) == b(C=0) == b(C=17) == b(H=0) == b(W=-16) == b(H=256, W=128) == b(H=24, W=16) == b(H=16, W=40) == IEF_ESHAPE
    assert b(mm=None, H=16385, W=1) == b(mm=None, H=1 << 20, W=1 << 20) == IEF_ESHAPE
    assert b(ep=p(eps) + 1) == b(mm=p(cell) + 2) == b(r=p(rk) + 3) == b(mo=p(mask) + 1) == b(to=p(th) + 2) == IEF_EALIGN

    x, noise = torch.randn(1, 4, 16, 16, device=DEV), torch.randn(2, 4, 16, 16, device=DEV)
    sigma, dirc = ddpm_sigma_dir(A_F, A_T)
    coef, scale = torch.tensor([A_F, A_T, sigma, dirc], device=DEV), torch.tensor([5.0, 3.0], device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    pmask = torch.ones(2, 16, 16, device=DEV)
    out, x0 = nanf(1, 4, 16, 16), nanf(1, 4, 16, 16)
    good = dict(eps=p(eps), mask=p(pmask), scale=p(scale), x=p(x), x_out=p(out), x0_out=p(x0), coef=p(coef), row_elems=1024, hw=256,
                noise=p(noise), noise_rows=2, step=p(step), E=2)
    c = lambda **kw: lib.ief_ledits_ddpm_step_f32(*{**good, **kw}.values(), stream())
    for name in ("eps", "scale", "x", "x_out", "coef", "noise", "step"):
        assert c(**{name: None}) == IEF_EINVAL, name
    for kw in (dict(E=0), dict(E=9), dict(hw=0), dict(hw=16385, row_elems=16385), dict(row_elems=1000), dict(row_elems=128),
               dict(row_elems=17 * 256), dict(noise_rows=0)):
        assert c(**kw) == IEF_ESHAPE, kw
    for name in ("eps", "mask", "scale", "x", "x_out", "x0_out", "coef", "noise", "step"):
        assert c(**{name: good[name] + 2}) == IEF_EALIGN, name
    torch.cuda.synchronize()
    for t in (m1, mask, th, out, x0):
        assert torch.isnan(t).all(), "a refused call must not launch"

    # the binding's own checks, in front of the library
    with pytest.raises(ValueError):
        hip.ledits_attn_mask(acc, taps, rank[:1].contiguous())
    with pytest.raises(ValueError):
        hip.ledits_attn_mask(acc, taps, rank, out=acc)
    with pytest.raises(ValueError):
        hip.ledits_guidance_mask(eps, cell[:1].contiguous(), rk)
    with pytest.raises(ValueError):
        hip.ledits_guidance_mask(eps[:1].contiguous(), None, None)
    with pytest.raises(ValueError):
        hip.ledits_ddpm_step(eps, pmask[:1].contiguous(), scale, x, coef, noise, step)
    with pytest.raises(ValueError):
        hip.ledits_ddpm_step(eps, pmask, scale, torch.zeros(2, 4, 16, 16, device=DEV), coef, noise, step)
    with pytest.raises(TypeError):
        hip.ledits_ddpm_step(eps, pmask, scale, x, coef, noise, step.long())
    assert a() == 0 and b() == 0 and b(mm=None) == 0 and b(r=None, ep=None, to=None) == 0 and c() == 0 and c(mask=None, x0_out=None) == 0
    torch.cuda.synchronize()
    for t in (m1, mask, th, out, x0):
        assert torch.isfinite(t).all()


# ------------------------------------------------------------------------------------------------------------- the sampler
@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.pipeline import StableDiffusionPipeline
    return StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")


def seeded_x0(pipe, seed):
    s = pipe.cfg.sample_size
    return torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(seed)).to(DEV)


def invert(pipe, seed, skip, K=3, **kw):
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    x0 = seeded_x0(pipe, seed)
    pipe.scheduler.set_timesteps(STEPS)
    y, maps, _ = DDPMInversion().noise_maps(pipe, x0, [""], skip=skip, rows_per_launch=K, generator=torch.Generator().manual_seed(seed + 1),
                                            **kw)
    return x0, y, maps


def edit(pipe, y, maps, skip, concepts=CONCEPTS[:2], use_graph=True, **kw):
    from ief_amd.ledits.model.sd_utils import LEDITS
    pipe.scheduler.set_timesteps(STEPS)
    args = dict(edit_guidance_scale=[5.0, 7.0][:len(concepts)] if len(concepts) <= 2 else 5.0, edit_threshold=0.75)
    args.update(kw)
    lat, masks = LEDITS(pipe, STEPS).edit(pipe, y, maps, skip, concepts, use_graph=use_graph, **args)
    assert pipe.unet._plan is None, "the plan is unregistered when the edit returns"
    return lat.float().cpu(), masks


def torch_rule(monkeypatch):
    """the unconditional-only extraction and the step written out with torch fp32 operations on the device (one rounded operation
    each, a DEVICE divisor: torch divides by a host scalar through its reciprocal), in place of the two kernels"""
    dev = lambda v: torch.full((), float(v), dtype=torch.float32, device=DEV)

    def mu_of(e, x, c):
        a, p, sigma, dirc = (float(v) for v in c[:4].tolist())
        one = torch.tensor(1.0)
        sb_f, sa_f, sa_t = torch.sqrt(one - torch.tensor(a)).item(), torch.sqrt(torch.tensor(a)).item(), torch.sqrt(torch.tensor(p)).item()
        x0 = (x - sb_f * e) / dev(sa_f)
        return sa_t * x0 + dirc * e, sigma

    def maps_t(eps_u, eps_c, x_t, x_prev, coef_rows, out=None):
        assert eps_u is None, "an empty source prompt runs the unconditional-only extraction"
        rows = []
        for r in range(x_t.shape[0]):
            mu, sigma = mu_of(eps_c[r], x_t[r], coef_rows[r])
            rows.append((x_prev[r] - mu) / dev(sigma))
        z = torch.stack(rows)
        return z if out is None else out.copy_(z)

    def step_t(eps, mask, scale, x, coef, noise, step, out=None, x0_out=None):
        g = torch.zeros_like(eps[0])
        for e, sc in enumerate(scale.tolist()):
            if sc != 0.0:
                g = g + (sc * (1.0 if mask is None else mask[e][None])) * (eps[1 + e] - eps[0])
        mu, sigma = mu_of(eps[0] + g, x[0], coef)
        r = min(max(int(step.item()), 0), noise.shape[0] - 1)
        res = (mu + sigma * noise[r])[None]
        return res if out is None else out.copy_(res)

    monkeypatch.setattr(hip, "ddpm_noise_maps", maps_t)
    monkeypatch.setattr(hip, "ledits_ddpm_step", step_t)


@pytest.mark.parametrize("skip", [0, 1])
def test_reconstruction_with_no_concept_active(small_x3, skip, monkeypatch):
    """Measured on an MI355X (`small`, f16x3, 4 steps, empty source prompt, warm-up 4): |x_final - x0| / max |x0| = 9.619e-7 on the
    kernels and 1.058e-6 with extraction and step written out in torch fp32 at skip 0; 4.489e-7 and 4.489e-7 at skip 1 (bound 4 x);
    with two active concepts the result ends 1.4e-1 / 4.8e-2 away."""
    from ief_amd import denoise
    pipe = small_x3
    denoise.drop_pool()
    x0, y, maps = invert(pipe, 8888, skip)
    lat, _ = edit(pipe, y, maps, skip, edit_warmup_steps=STEPS)
    x0c = x0.float().cpu()
    scale = x0c.abs().max().item()
    e_kernel = (lat - x0c).abs().max().item() / scale
    with monkeypatch.context() as m:
        torch_rule(m)
        _, yt, mapst = invert(pipe, 8888, skip)
        ruled, _ = edit(pipe, yt, mapst, skip, edit_warmup_steps=STEPS, use_graph=False)
    e_torch = (ruled - x0c).abs().max().item() / scale
    active, _ = edit(pipe, y, maps, skip)
    moved = (active - x0c).abs().max().item() / scale
    print(f"small f16x3, {STEPS} steps, skip {skip}, no concept active: |x_final - x0| / max |x0| = {e_kernel:.3e} on the kernels, "
          f"{e_torch:.3e} written out in torch fp32 (bound 4 x); with two active concepts the result is {moved:.3e} away")
    assert e_torch > 0 and e_kernel <= 4 * e_torch
    assert moved >= 100 * e_kernel, "active concepts must move the image"
    denoise.drop_pool()


@pytest.mark.parametrize("mode", [(True, True), (True, False), (False, True), (False, False)])
def test_graph_equals_eager_in_the_four_mask_modes(small_x3, mode):
    from ief_amd import denoise
    pipe = small_x3
    cross, intersect = mode
    denoise.drop_pool()
    _, y, maps = invert(pipe, 8888, 1)
    kw = dict(cross_attn_mask=cross, intersect_mask=intersect, reverse=[1], edit_warmup_steps=[1, 0], keep_masks=True)
    graph, gm = edit(pipe, y, maps, 1, use_graph=True, **kw)
    eager, em = edit(pipe, y, maps, 1, use_graph=False, **kw)
    assert torch.equal(graph, eager), "the captured graph must equal eager stepping bit for bit"
    if cross or intersect:
        assert gm.shape == (STEPS - 1, 2, *y.shape[-2:]) and torch.equal(gm, em) and set(gm.unique().tolist()) <= {0.0, 1.0}
        print(f"cross {cross}, intersect {intersect}: set pixels per step and concept {gm.sum((2, 3)).int().tolist()}")
        assert gm.sum() > 0
    else:
        assert gm is None and em is None
    denoise.drop_pool()


def test_modes_differ_and_the_f16_f32_modes_run_without_the_cross_mask():
    from ief_amd import denoise
    from ief_amd.pipeline import StableDiffusionPipeline
    for precision in ("f16", "f32"):
        pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", precision=precision)
        denoise.drop_pool()
        _, y, maps = invert(pipe, 8888, 1)
        with pytest.raises(ValueError, match="f16x3 mode only"):
            edit(pipe, y, maps, 1)
        assert pipe.unet._plan is None
        graph, _ = edit(pipe, y, maps, 1, cross_attn_mask=False)
        eager, _ = edit(pipe, y, maps, 1, cross_attn_mask=False, use_graph=False)
        plain, _ = edit(pipe, y, maps, 1, cross_attn_mask=False, intersect_mask=False)
        assert torch.equal(graph, eager) and torch.isfinite(graph).all() and not torch.equal(graph, plain)
        denoise.drop_pool()


def test_pooled_loop_run_twice_and_repointed(small_x3):
    from ief_amd import denoise
    from ief_amd.ledits.model import sd_utils
    pipe = small_x3
    _, ya, mapsa = invert(pipe, 8888, 1)
    _, yb, mapsb = invert(pipe, 4242, 1)
    kwa = dict(concepts=CONCEPTS[:2], edit_guidance_scale=[5.0, 7.0], edit_threshold=0.75)
    kwb = dict(concepts=[CONCEPTS[2], CONCEPTS[0]], edit_guidance_scale=[3.0, 9.0], edit_threshold=[0.5, 0.9], reverse=[0])
    denoise.drop_pool()
    real, seen = sd_utils.acquire, []

    def spy(*a, **kw):
        seen.append(real(*a, **kw))
        return seen[-1]

    sd_utils.acquire = spy
    try:
        fresh_a, _ = edit(pipe, ya, mapsa, 1, **kwa)
        denoise.drop_pool()
        fresh_b, _ = edit(pipe, yb, mapsb, 1, **kwb)
        denoise.drop_pool()
        first, _ = edit(pipe, ya, mapsa, 1, **kwa)
        again, _ = edit(pipe, ya, mapsa, 1, **kwa)
        second, _ = edit(pipe, yb, mapsb, 1, **kwb)
        back, _ = edit(pipe, ya, mapsa, 1, **kwa)
        three, _ = edit(pipe, ya, mapsa, 1, concepts=CONCEPTS, edit_guidance_scale=5.0, edit_threshold=0.75)
    finally:
        sd_utils.acquire = real
    assert seen[2] is seen[3] is seen[4] is seen[5] and seen[2].graph is not None, "equal signatures: one captured loop serves them all"
    assert seen[6] is not seen[2], "another E is another pool entry"
    assert torch.equal(first, fresh_a) and torch.equal(again, first), "the same pooled loop run twice"
    assert torch.equal(second, fresh_b), "re-pointed at other concepts, scales, thresholds and maps == that job's fresh run"
    assert torch.equal(back, first) and not torch.equal(first, second) and not torch.equal(three, first)
    denoise.drop_pool()


def test_one_eager_step_is_the_restatement_on_its_own_accumulator_and_eps(small_x3, monkeypatch):
    """the wiring: batch rows, token windows, the per-step zeroing, the rank tables, the scale row.  The synthetic weights give nearly
    flat maps, so masks are compared on the DUMPED accumulator and eps, never across two independently computed paths."""
    from ief_amd import denoise
    from ief_amd.control import ControlPlan, ledits_scale_table, ledits_token_weights
    from ief_amd.ledits.model.sd_utils import concept_token_counts
    pipe = small_x3
    denoise.drop_pool()
    _, y, maps = invert(pipe, 8888, 1)
    dumps = []
    real = ControlPlan.ledits_step

    def spy(self, eps, lat, coef_cur, maps_, step):
        before = lat.clone()
        real(self, eps, lat, coef_cur, maps_, step)
        led = self.led
        dumps.append({k: v.clone().cpu() for k, v in dict(eps=eps, x=before, out=lat, coef=coef_cur, step=step, acc=led["acc"], m1=led["m1"],
                                                          mask=led["mask"], thres=led["thres"], scale=led["scale_cur"], w=led["w"],
                                                          rank_attn=led["rank_attn"], rank_pix=led["rank_pix"]).items()})

    monkeypatch.setattr(ControlPlan, "ledits_step", spy)
    q = [0.75, 0.6]
    edit(pipe, y, maps, 1, use_graph=False, edit_threshold=q, reverse=[1], edit_warmup_steps=[1, 0])
    assert len(dumps) == STEPS - 1
    h, w = y.shape[-2:]
    counts = concept_token_counts(pipe.tokenizer, CONCEPTS[:2])
    table = ledits_scale_table(STEPS - 1, [5.0, 7.0], [1], [1, 0])
    for i, d in enumerate(dumps):
        assert int(d["step"]) == i and torch.equal(d["scale"], table[i]), "the loop's step counter picks the scale row"
        assert torch.equal(d["w"], ledits_token_weights(counts))
        assert torch.equal(d["rank_attn"], ledits_rank_table(q, 256)) and torch.equal(d["rank_pix"], ledits_rank_table(q, h * w))
        m1, _, _ = ref.attn_mask(d["acc"], ledits_taps(), d["rank_attn"])
        mask, ts, _ = ref.guidance_mask(d["eps"], m1, d["rank_pix"])
        out, _ = ref.ddpm_step(d["eps"], mask, d["scale"], d["x"][0], d["coef"], maps[i].cpu())
        assert torch.equal(d["m1"], m1) and torch.equal(d["mask"], mask) and torch.equal(d["thres"], ts)
        assert torch.equal(d["out"][0], out), f"step {i}: x_out must be the restatement's bit for bit"
        assert (d["acc"] > 0).all()
    # the accumulator is emptied every step: five modules' head-mean mass over a concept's tokens stays below 5 per cell, and the
    # per-step sums do not grow with the step as a running sum would
    sums = [d["acc"].sum().item() for d in dumps]
    print(f"accumulator sums per step {[f'{s:.4f}' for s in sums]} (a running sum would grow by one of them per step)")
    assert all(d["acc"].max() <= 5.0 for d in dumps) and max(sums) < 1.5 * min(sums)
    denoise.drop_pool()


def test_unconditional_only_extraction_equals_both_halves(small_x3):
    """Measured on an MI355X: `small` f16x3 maps of the unconditional-only form against both halves differ by 3.268e-7 (K = 1) and
    6.537e-7 (K = 3) of their size (bound 2.3e-6, the distance between chunk sizes `test_gpu_ddpm_inversion.py` states); `tiny` f16:
    bit-equal."""
    from ief_amd.pipeline import StableDiffusionPipeline
    for K in (1, 3):
        _, y1, one = invert(small_x3, 8888, 1, K=K)
        _, y2, two = invert(small_x3, 8888, 1, K=K, uncond_only=False)
        d = (one - two).abs().max().item() / two.abs().max().item()
        print(f"small f16x3, K = {K}: unconditional-only maps vs both halves differ by {d:.3e} of their size (bound 2.3e-6)")
        assert torch.equal(y1, y2) and d <= 2.3e-6
    tiny = StableDiffusionPipeline.from_pretrained("synthetic:tiny", precision="f16")
    for K in (1, 3):
        _, _, one = invert(tiny, 8888, 1, K=K)
        _, _, two = invert(tiny, 8888, 1, K=K, uncond_only=False)
        assert torch.equal(one, two), f"tiny f16, K = {K}: the unconditional-only form must give the same bits"
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    with pytest.raises(ValueError, match="EMPTY source prompt"):
        DDPMInversion().noise_maps(tiny, seeded_x0(tiny, 1), ["a house"], uncond_only=True)


# ------------------------------------------------------------------------------------------------------------- the PIE driver
def test_pie_driver_writes_its_images(tmp_path):
    script = os.path.join(PKG, "ledits", "test.py")
    base = ["--sd_version", "small", "--synthetic", "2", "--seed", "7", "--edit_prompt", "glasses", "a red hat", "--remove", "1"]
    a, b = tmp_path / "a", tmp_path / "b"
    one, two = run_mixed([([script] + base + ["--exp_path", str(a)], tmp_path / "cwd_a"),
                          ([script] + base + ["--exp_path", str(b)], tmp_path / "cwd_b")], in_process=(1,))
    assert one.last_json()["images"] == 2 and two.last_json()["images"] == 2
    dirs = sorted(x for x in os.listdir(a) if x.startswith("syn_"))
    assert len(dirs) == 2 and sorted(x for x in os.listdir(b) if x.startswith("syn_")) == dirs
    for d in dirs:
        for name in ("source.png", "inversion.png", "edit.png"):
            with open(a / d / name, "rb") as fa, open(b / d / name, "rb") as fb:
                assert fa.read() == fb.read(), (d, name)
        inv, ed = (np.array(Image.open(a / d / n)).astype(int) for n in ("inversion.png", "edit.png"))
        assert inv.shape == ed.shape and np.abs(inv - ed).max() > 0, "the edit must differ from the reconstruction"
