"""The second-order multistep SDE-DPM-Solver++ on the edit-friendly DDPM noise space, on a real MI355X: the three entry points
(`ief_cfg_dpmpp_step_f32`, `ief_ledits_dpmpp_step_f32`, `ief_dpmpp_noise_maps_f32`), the captured edit loops of `p2p/ --inversion_type
ddpm` and `ledits/` at order 2, the samplers and the two PIE drivers.

The rule (`csrc/ddpm_step.h`, dpmpp_mu_of), every operation rounded in fp32 in this order:
    x0 = (x - sqrt(1 - a) e) / sqrt(a);  mu1 = sqrt(p) x0 + dir e;  mu = c2 == 0 ? mu1 : mu1 + c2 (x0 - x0_prev);  x' = mu + sigma z
Stated checks (every test prints its figures):
    c2 = 0                      each entry point bit-equal to its sibling (x_out, x0_out, maps) over a NaN x0_prev / x0_carry, which
                                afterwards holds the step's x0 bit for bit
    c2 != 0 (S = 20 table)      max |kernel - fp64| <= 4 x max |the same expression in torch fp32 on the CPU - fp64|; in place == out
                                of place; row b of a mixed-scale launch == a launch whose rows all carry g_b
    extraction                  five rows: a sigma = 0 row is exactly zero, the first has c2 = 0 over a NaN carry; launched as (5),
                                (2, 2, 1) and (1 x 5) the maps and the carry are bit-identical; `noise_maps` then `step` returns
                                x_prev within 2^-24 (4 |x_prev - mu| + 2 |x_prev|) elementwise, the order-1 bound of
                                test_gpu_ddpm_inversion.py: the step reads the x0_prev bits the extraction had in its register (the
                                previous row's step wrote them from the same x and eps through the same device function), so mu --
                                c2 term included -- is the same bits in both kernels and the c2 term adds nothing to the bound
    whole loops                 captured graph == eager stepping == the sampler's eager branch, bit for bit; the source row ends on
                                x0 within 4 x the same loop written out in torch fp32; the order-2 target row differs from order 1's
                                by more than 100 x the graph-vs-torch difference
    pooled loops, edit_many, the two drivers at --num_steps 20 --solver_order 2: bit for bit / the same pixels / the same bytes
Measured on an MI355X: at c2 = 0.028 / 0.41 / 1.98 the CFG step's max |. - fp64| is 3.507e-5 ... 1.157e-4 and the LEDITS++ step's
8.700e-6 ... 3.179e-5, torch fp32 on the CPU the same figures (1.00 x, bound 4); round trip at most 0.585 of its bound; `small`, f16x3,
5 steps, g = (3.5, 15), order 2: |row 0 - x0| / max |x0| = 4.688e-5 on the kernels and 4.688e-5 written out in torch fp32 at skip 0 (order
1 on its own maps 2.246e-5), 1.523e-5 and 1.523e-5 at skip 1 (order 1: 8.401e-6); graph and torch loop agree bit for bit, the order-2
target row is 1.033 / 0.3205 of max |x0| from order 1's; LEDITS++ with no concept active 1.812e-6 and 1.812e-6, two active concepts 5.7e-2;
tiny f32 5.551e-5 / 1.426e-5, tiny f16 3.2e-2 / 1.5e-2 (fp16 activations; printed, not bounded).
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip  # noqa: E402
from ief_amd.scheduler import DDIMScheduler  # noqa: E402
from _procs import run_mixed  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "image-editing-framework_amd")
U = 2.0 ** -24
IEF_EINVAL, IEF_ESHAPE, IEF_EALIGN = -1, -2, -3          # csrc/ief_common.h
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]
CONCEPTS = ["a red hat", "glasses"]
STEPS, G_SRC, G_TAR = 5, 3.5, 15.0
GUIDANCE = (G_SRC, G_TAR)
NAN = float("nan")
nan_like = lambda t: torch.full_like(t, NAN)


def table20():
    """{timestep: (a, p, sigma, dir, c2)} of the 20-step schedule at order 2"""
    s = DDIMScheduler()
    s.set_timesteps(20)
    return dict(zip(s.timesteps.tolist(), s.dpmpp_table(0, 2)))


T20 = table20()
ROWS20 = [T20[901], T20[101], T20[51]]          # c2 = 0.028, 0.41, 1.98
assert abs(ROWS20[0][4] - 0.028) < 1e-3 and abs(ROWS20[1][4] - 0.41) < 1e-2 and abs(ROWS20[2][4] - 1.98) < 1e-2
STEP_ROWS = ((-1, 0), (0, 0), (2, 2), (7, 2), (5, 2))          # (device step, the row of three it clamps to); 5 = last + 3


def roots(a, p, dtype):
    """sqrt(1 - a), sqrt(a), sqrt(p) as the kernel takes them (IEEE, correctly rounded, from the fp32 table values) in `dtype`"""
    nt = np.float32 if dtype == torch.float32 else np.float64
    a, p = nt(np.float32(a)), nt(np.float32(p))
    return float(np.sqrt(nt(1) - a)), float(np.sqrt(a)), float(np.sqrt(p))


def mu2_torch(e, x, coef, x0_prev):
    """the order-2 mean in torch on the CPU in the dtype of the inputs, in the kernel's operation order (tensor divisors: an IEEE
    division); -> (mu, x0)"""
    dt = x.dtype
    a, p, sigma, dirc, c2 = (float(np.float32(v)) for v in coef)
    sb_f, sa_f, sa_t = roots(a, p, dt)
    x0 = (x - sb_f * e) / torch.tensor(sa_f, dtype=dt)
    mu = sa_t * x0 + dirc * e
    if c2 != 0.0:
        mu = mu + c2 * (x0 - x0_prev)
    return mu, x0


def guided(eu, ec, g_rows):
    if eu is None:
        return ec
    g = g_rows.to(ec.dtype).reshape(-1, *([1] * (ec.dim() - 1)))
    return eu + g * (ec - eu)


def kernel_inputs(Bp, row_elems, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    eu, ec, x, x0p = r(Bp, row_elems), r(Bp, row_elems), r(Bp, row_elems), r(Bp, row_elems)
    noise = torch.stack([r(row_elems), 1e-3 * r(row_elems), 50 * r(row_elems)])          # three rows, three scales
    return eu, ec, x, x0p, noise


# ------------------------------------------------------------------------------------------------------------- the CFG step
@pytest.mark.parametrize("Bp", [2, 3])
@pytest.mark.parametrize("row_elems", [256, 252, 16384])
def test_cfg_dpmpp_step_kernel(Bp, row_elems):
    eu_h, ec_h, x_h, x0p_h, noise_h = kernel_inputs(Bp, row_elems, 17 * Bp + row_elems)
    eu, ec, x, x0p, noise = (t.to(DEV) for t in (eu_h, ec_h, x_h, x0p_h, noise_h))
    g_h = torch.tensor([G_SRC, G_TAR, 7.5][:Bp])
    g_rows = g_h.to(DEV)
    worst = (0.0, 0.0, 0.0)
    for s, r in STEP_ROWS:
        step = torch.tensor([s], dtype=torch.int32, device=DEV)
        # c2 = 0: the sibling bit for bit over a NaN x0_prev, which then holds the step's x0
        for row in ROWS20:
            c4 = torch.tensor(row[:4], dtype=torch.float32, device=DEV)
            c5 = torch.tensor([*row[:4], 0.0], dtype=torch.float32, device=DEV)
            for cfg in (True, False):
                u, gr = (eu, g_rows) if cfg else (None, None)
                x0a, x0b, carry = nan_like(x), nan_like(x), nan_like(x)
                old = hip.cfg_ddpm_step(u, ec, x, c4, gr, noise, step, out=nan_like(x), x0_out=x0a)
                new = hip.cfg_dpmpp_step(u, ec, x, c5, gr, noise, step, carry, out=nan_like(x), x0_out=x0b)
                assert torch.equal(new, old) and torch.equal(x0a, x0b), f"c2 = 0 must be the DDPM step (step={s}, cfg={cfg})"
                assert torch.equal(carry, x0a), "x0_prev holds the step's x0 bit for bit"
        # c2 != 0 against fp64; the yardstick is the same expression in torch fp32 on the CPU
        for row in ROWS20:
            c5 = torch.tensor(row, dtype=torch.float32, device=DEV)
            carry, x0o = x0p.clone(), nan_like(x)
            out = hip.cfg_dpmpp_step(eu, ec, x, c5, g_rows, noise, step, carry, out=nan_like(x), x0_out=x0o)
            torch.cuda.synchronize()
            assert int(step.item()) == s, "the kernel only reads the step"
            assert torch.equal(carry, x0o), "x0_prev := x0"
            for b in range(Bp):
                uni = hip.cfg_dpmpp_step(eu, ec, x, c5, torch.full((Bp,), float(g_h[b]), device=DEV), noise, step, x0p.clone())
                assert torch.equal(uni[b], out[b]), f"row {b} must not depend on the other rows' scales (step={s})"
            assert not torch.equal(uni[0], out[0]), "the scales must act"
            xc, cc = x.clone(), x0p.clone()
            assert hip.cfg_dpmpp_step(eu, ec, xc, c5, g_rows, noise, step, cc, out=xc) is xc
            assert torch.equal(xc, out) and torch.equal(cc, x0o), "in place == out of place"
            sig = float(np.float32(row[2]))
            mu64, x064 = mu2_torch(guided(eu_h.double(), ec_h.double(), g_h), x_h.double(), row, x0p_h.double())
            mu32, x032 = mu2_torch(guided(eu_h, ec_h, g_h), x_h, row, x0p_h)
            want64, want32 = mu64 + sig * noise_h[r].double(), mu32 + sig * noise_h[r]
            err_k = max((out.cpu().double() - want64).abs().max().item(), (x0o.cpu().double() - x064).abs().max().item())
            err_y = max((want32.double() - want64).abs().max().item(), (x032.double() - x064).abs().max().item())
            assert err_y > 0 and err_k <= 4 * err_y, f"step={s} c2={row[4]:.3g}: kernel {err_k:.3e} vs fp64, torch fp32 {err_y:.3e} (bound 4 x)"
            if err_k / err_y > worst[0]:
                worst = (err_k / err_y, err_k, err_y)
            # the correction is read: the same launch at c2 = 0 is far away
            plain = hip.cfg_dpmpp_step(eu, ec, x, torch.tensor([*row[:4], 0.0], device=DEV), g_rows, noise, step, x0p.clone())
            assert (plain.cpu().double() - want64).abs().max().item() > 100 * err_k
    # no CFG: eps = eps_c, g_rows may be missing
    row = ROWS20[2]
    out = hip.cfg_dpmpp_step(None, ec, x, torch.tensor(row, device=DEV), None, noise, torch.zeros(1, dtype=torch.int32, device=DEV), x0p.clone())
    sig = float(np.float32(row[2]))
    w64 = mu2_torch(ec_h.double(), x_h.double(), row, x0p_h.double())[0] + sig * noise_h[0].double()
    w32 = mu2_torch(ec_h, x_h, row, x0p_h)[0] + sig * noise_h[0]
    e_k, e_y = (out.cpu().double() - w64).abs().max().item(), (w32.double() - w64).abs().max().item()
    assert e_k <= 4 * e_y
    print(f"dpmpp step Bp={Bp} row_elems={row_elems}: worst max |kernel - fp64| {worst[1]:.3e}, torch fp32 on the CPU {worst[2]:.3e}: "
          f"{worst[0]:.2f} x (bound 4); without eps_u at c2 = {row[4]:.3f}: {e_k:.3e} vs {e_y:.3e}")


# ------------------------------------------------------------------------------------------------------------- the LEDITS++ step
def ledits_ref(eps, mask, scale, x, coef, z, x0_prev, dtype):
    """the masked multi-concept guidance (`ledits_ref.ddpm_step`'s, operation for operation) and the order-2 update on one latent"""
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
    mu, x0 = mu2_torch(u + g, x.to(dtype), coef, x0_prev.to(dtype))
    sig = float(np.float32(coef[2]))
    return (mu if sig == 0.0 else mu + sig * z.to(dtype)), x0


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("shape", [(4, 8, 8), (4, 7, 9), (4, 64, 64)])          # 256, 252 and 16384 elements
def test_ledits_dpmpp_step_kernel(shape, E):
    C, h, w = shape
    g = torch.Generator().manual_seed(C * h * w + E)
    r = lambda *s: torch.randn(*s, generator=g)
    eps_h, x_h, x0p_h = r(1 + E, C, h, w), r(1, C, h, w), r(C, h, w)
    noise_h = torch.stack([r(C, h, w), 1e-3 * r(C, h, w), 50 * r(C, h, w)])
    mask_h = (torch.rand(E, h, w, generator=g) > 0.6).float()
    scale_h = torch.tensor([5.0, -3.0, 0.0][:E])
    eps, x, x0p, noise, mask, scale = (t.to(DEV) for t in (eps_h, x_h, x0p_h, noise_h, mask_h, scale_h))
    worst = (0.0, 0.0, 0.0)
    for s, row_i in STEP_ROWS:
        step = torch.tensor([s], dtype=torch.int32, device=DEV)
        for use_mask in (True, False):
            m, mh = (mask, mask_h) if use_mask else (None, None)
            for row in ROWS20:
                c4 = torch.tensor(row[:4], dtype=torch.float32, device=DEV)
                c5z = torch.tensor([*row[:4], 0.0], dtype=torch.float32, device=DEV)
                x0a, x0b, carry = nan_like(x), nan_like(x), nan_like(x0p)
                old = hip.ledits_ddpm_step(eps, m, scale, x, c4, noise, step, out=nan_like(x), x0_out=x0a)
                new = hip.ledits_dpmpp_step(eps, m, scale, x, c5z, noise, step, carry, out=nan_like(x), x0_out=x0b)
                assert torch.equal(new, old) and torch.equal(x0a, x0b), f"c2 = 0 must be the DDPM step (step={s}, mask={use_mask})"
                assert torch.equal(carry, x0a[0]), "x0_prev holds the step's x0 bit for bit"
                c5 = torch.tensor(row, dtype=torch.float32, device=DEV)
                carry, x0o = x0p.clone(), nan_like(x)
                out = hip.ledits_dpmpp_step(eps, m, scale, x, c5, noise, step, carry, out=nan_like(x), x0_out=x0o)
                assert torch.equal(carry, x0o[0]), "x0_prev := x0"
                xin, cin = x.clone(), x0p.clone()
                assert hip.ledits_dpmpp_step(eps, m, scale, xin, c5, noise, step, cin, out=xin) is xin
                assert torch.equal(xin, out) and torch.equal(cin, carry), "in place == out of place"
                r64, x064 = ledits_ref(eps_h, mh, scale_h, x_h[0], row, noise_h[row_i], x0p_h, torch.float64)
                r32, x032 = ledits_ref(eps_h, mh, scale_h, x_h[0], row, noise_h[row_i], x0p_h, torch.float32)
                e_k = max((out.cpu()[0].double() - r64).abs().max().item(), (x0o.cpu()[0].double() - x064).abs().max().item())
                e_y = max((r32.double() - r64).abs().max().item(), (x032.double() - x064).abs().max().item())
                assert e_y > 0 and e_k <= 4 * e_y, f"step={s} c2={row[4]:.3g}: kernel {e_k:.3e} vs fp64, torch fp32 {e_y:.3e} (bound 4 x)"
                if e_k / e_y > worst[0]:
                    worst = (e_k / e_y, e_k, e_y)
                if E == 3:          # a gated concept is skipped, not multiplied: its estimate may hold anything
                    poisoned = eps.clone()
                    poisoned[3] = NAN
                    assert torch.equal(hip.ledits_dpmpp_step(poisoned, m, scale, x, c5, noise, step, x0p.clone()), out)
    # E = 1, no mask, scale = [g]: the CFG form of the same step, bit for bit
    c5 = torch.tensor(ROWS20[2], dtype=torch.float32, device=DEV)
    ca, cb = x0p.clone(), x0p.clone()[None].contiguous()
    a = hip.ledits_dpmpp_step(eps[:2].contiguous(), None, torch.tensor([7.5], device=DEV), x, c5, noise, step, ca)
    b = hip.cfg_dpmpp_step(eps[:1], eps[1:2], x, c5, torch.tensor([7.5], device=DEV), noise, step, cb)
    assert torch.equal(a, b) and torch.equal(ca, cb[0])
    print(f"ledits dpmpp step {C * h * w} elements, E = {E}: worst max |kernel - fp64| {worst[1]:.3e}, torch fp32 on the CPU "
          f"{worst[2]:.3e}: {worst[0]:.2f} x (bound 4)")


# ------------------------------------------------------------------------------------------------------------- the extraction
def extraction_case(row_elems):
    g = torch.Generator().manual_seed(row_elems)
    R = 5
    eu, ec, xt = (torch.randn(R, row_elems, generator=g).to(DEV) for _ in range(3))
    scales = [1.0, 1e-3, 1e2, 1.0, 10.0]
    xprev = torch.stack([s * torch.randn(row_elems, generator=g) for s in scales]).to(DEV)
    rows = [[*T20[951][:4], 3.5, 0.0],                      # the first row: order 1, over a NaN carry
            [*T20[901][:4], 15.0, T20[901][4]],
            [*T20[101][:4], 1.0, T20[101][4]],
            [*T20[51][:4], 7.5, T20[51][4]],
            [*T20[1][:4], 0.0, 0.0]]
    rows[2][2], rows[2][3] = 0.0, float(np.float32(np.sqrt(1 - np.float64(np.float32(rows[2][1])))))          # the sigma = 0 row
    return eu, ec, xt, xprev, rows, scales


@pytest.mark.parametrize("row_elems", [252, 4096])
def test_extraction_chunking_and_round_trip(row_elems):
    eu, ec, xt, xprev, rows, scales = extraction_case(row_elems)
    R = len(rows)
    coef_rows = torch.tensor(rows, dtype=torch.float32, device=DEV)

    def launch(chunks, u=eu):
        carry, z, r0 = torch.full((row_elems,), NAN, device=DEV), nan_like(xt), 0
        for k in chunks:
            sl = slice(r0, r0 + k)
            hip.dpmpp_noise_maps(None if u is None else u[sl], ec[sl], xt[sl], xprev[sl], coef_rows[sl].contiguous(), carry, out=z[sl])
            r0 += k
        return z, carry

    z, carry = launch((5,))
    torch.cuda.synchronize()
    assert torch.isfinite(z).all() and torch.isfinite(carry).all(), "c2 = 0 on the first row: the NaN carry is not read into the result"
    assert (z[2] == 0).all(), "a sigma = 0 row is exactly zero"
    for chunks in ((2, 2, 1), (1, 1, 1, 1, 1)):
        z2, carry2 = launch(chunks)
        assert torch.equal(z2, z) and torch.equal(carry2, carry), f"rows dealt as {chunks} must give the bits of one launch"
    # c2 = 0 in every row: the sibling, bit for bit, over a NaN carry
    c0 = coef_rows.clone()
    c0[:, 5] = 0.0
    zc, cc = nan_like(xt), torch.full((row_elems,), NAN, device=DEV)
    hip.dpmpp_noise_maps(eu, ec, xt, xprev, c0, cc, out=zc)
    assert torch.equal(zc, hip.ddpm_noise_maps(eu, ec, xt, xprev, c0[:, :5].contiguous())), "c2 = 0 must be ief_ddpm_noise_maps_f32"
    assert not torch.equal(zc[1], z[1]) and not torch.equal(zc[3], z[3]), "the correction acts"
    # the step over those rows: row r's step reads the x0 the step of row r - 1 wrote
    x0_prev, worst = torch.full((1, row_elems), NAN, device=DEV), 0.0
    for r in range(R):
        step = torch.tensor([r], dtype=torch.int32, device=DEV)
        args = (eu[r:r + 1], ec[r:r + 1], xt[r:r + 1])
        c5 = torch.tensor([*rows[r][:4], rows[r][5]], dtype=torch.float32, device=DEV)
        cm = c5.clone()
        cm[2] = 0.0
        g1 = coef_rows[r, 4:5].contiguous()
        mu = hip.cfg_dpmpp_step(*args, cm, g1, z, step, x0_prev.clone())[0]          # the mean's own bits
        back = hip.cfg_dpmpp_step(*args, c5, g1, z, step, x0_prev)[0]                # and x0_prev := x0 of row r
        if r == 2:
            assert torch.equal(back, mu), "sigma = 0 adds nothing"
            continue
        xp = xprev[r].double()
        bound = U * (4 * (xp - mu.double()).abs() + 2 * xp.abs())
        ratio = ((back.double() - xp).abs() / bound.clamp_min(1e-300)).max().item()
        assert ratio <= 1, f"row {r} (c2 = {rows[r][5]:.3g}, scale {scales[r]}): |round trip - x_prev| / bound = {ratio:.3f}"
        worst = max(worst, ratio)
        z64 = (xp - mu.double()) / np.float64(np.float32(rows[r][2]))
        assert ((z[r].double() - z64).abs() <= 2.01 * U * z64.abs() + 1e-45).all(), "the map on the kernel's own mean: two rounded operations"
    assert torch.equal(x0_prev[0], carry), "the last row's x0 is what the extraction wrote back"
    # without eps_u the scale column is not read
    z1, _ = launch((5,), u=None)
    coef_rows[:, 4] = 99.0
    assert torch.equal(launch((2, 3), u=None)[0], z1)
    print(f"dpmpp noise_maps -> step, 5 rows x {row_elems} elements: worst |x' - x_prev| / (2^-24 (4 |x_prev - mu| + 2 |x_prev|)) = "
          f"{worst:.3f} (bound 1)")


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    lib = hip.load()
    p = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    eu, ec, x, x0p, noise = (t.to(DEV) for t in kernel_inputs(2, 256, 5))
    coef = torch.tensor(ROWS20[1], dtype=torch.float32, device=DEV)
    g_rows = torch.tensor([G_SRC, G_TAR], device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, x0, carry = nan_like(x), nan_like(x), nan_like(x)
    good = dict(eps_u=p(eu), eps_c=p(ec), x=p(x), x_out=p(out), x0_out=p(x0), x0_prev=p(carry), coef=p(coef), g_rows=p(g_rows),
                n=x.numel(), row_elems=256, noise=p(noise), noise_rows=3, step=p(step))
    call = lambda **kw: lib.ief_cfg_dpmpp_step_f32(*{**good, **kw}.values(), stream)
    for name in ("eps_c", "x", "x_out", "x0_prev", "coef", "noise", "step", "g_rows"):
        assert call(**{name: None}) == IEF_EINVAL, name
    for kw in (dict(n=0), dict(n=-512), dict(row_elems=0), dict(row_elems=-256), dict(row_elems=200), dict(noise_rows=0), dict(noise_rows=-1)):
        assert call(**kw) == IEF_ESHAPE, kw
    for name in ("eps_u", "eps_c", "x", "x_out", "x0_out", "x0_prev", "coef", "g_rows", "noise", "step"):
        assert call(**{name: good[name] + 2}) == IEF_EALIGN, name

    coef_rows = torch.tensor([[*ROWS20[0][:4], G_SRC, 0.0], [*ROWS20[1][:4], G_SRC, ROWS20[1][4]]], dtype=torch.float32, device=DEV)
    z, mcarry = nan_like(x), torch.full((256,), NAN, device=DEV)
    goodm = dict(eps_u=p(eu), eps_c=p(ec), x_t=p(x), x_prev=p(x), z_out=p(z), coef_rows=p(coef_rows), x0_carry=p(mcarry), R=2, row_elems=256)
    callm = lambda **kw: lib.ief_dpmpp_noise_maps_f32(*{**goodm, **kw}.values(), stream)
    for name in ("eps_c", "x_t", "x_prev", "z_out", "coef_rows", "x0_carry"):
        assert callm(**{name: None}) == IEF_EINVAL, name
    for kw in (dict(R=0), dict(R=-2), dict(row_elems=0), dict(row_elems=-256)):
        assert callm(**kw) == IEF_ESHAPE, kw
    for name in ("eps_u", "eps_c", "x_t", "x_prev", "z_out", "coef_rows", "x0_carry"):
        assert callm(**{name: goodm[name] + 1}) == IEF_EALIGN, name

    eps = torch.randn(3, 4, 16, 16, device=DEV)
    lx, lnoise = torch.randn(1, 4, 16, 16, device=DEV), torch.randn(2, 4, 16, 16, device=DEV)
    scale, pmask = torch.tensor([5.0, 3.0], device=DEV), torch.ones(2, 16, 16, device=DEV)
    lout, lx0, lcarry = nan_like(lx), nan_like(lx), nan_like(lx[0])
    goodl = dict(eps=p(eps), mask=p(pmask), scale=p(scale), x=p(lx), x_out=p(lout), x0_out=p(lx0), x0_prev=p(lcarry), coef=p(coef),
                 row_elems=1024, hw=256, noise=p(lnoise), noise_rows=2, step=p(step), E=2)
    calll = lambda **kw: lib.ief_ledits_dpmpp_step_f32(*{**goodl, **kw}.values(), stream)
    for name in ("eps", "scale", "x", "x_out", "x0_prev", "coef", "noise", "step"):
        assert calll(**{name: None}) == IEF_EINVAL, name
    for kw in (dict(E=0), dict(E=9), dict(hw=0), dict(hw=16385, row_elems=16385), dict(row_elems=1000), dict(row_elems=128),
               dict(row_elems=17 * 256), dict(noise_rows=0)):
        assert calll(**kw) == IEF_ESHAPE, kw
    for name in ("eps", "mask", "scale", "x", "x_out", "x0_out", "x0_prev", "coef", "noise", "step"):
        assert calll(**{name: goodl[name] + 2}) == IEF_EALIGN, name
    torch.cuda.synchronize()
    for t in (out, x0, carry, z, mcarry, lout, lx0, lcarry):
        assert torch.isnan(t).all(), "a refused call must not launch"

    # the bindings' own checks, in front of the library
    with pytest.raises(ValueError):
        hip.cfg_dpmpp_step(eu, ec, x, coef[:4].contiguous(), g_rows, noise, step, carry)
    with pytest.raises(ValueError):
        hip.cfg_dpmpp_step(eu, ec, x, coef, g_rows, noise, step, carry[:1].contiguous())
    with pytest.raises(ValueError):
        hip.cfg_dpmpp_step(eu, ec, x, coef, g_rows, noise, step, None)
    with pytest.raises(TypeError):
        hip.cfg_dpmpp_step(eu, ec, x, coef, g_rows, noise, step.long(), carry)
    with pytest.raises(ValueError):
        hip.dpmpp_noise_maps(eu, ec, x, x, coef_rows[:, :5].contiguous(), mcarry)
    with pytest.raises(ValueError):
        hip.dpmpp_noise_maps(eu, ec, x, x, coef_rows, mcarry[:128].contiguous())
    with pytest.raises(ValueError):
        hip.ledits_dpmpp_step(eps, pmask, scale, lx, coef[:4].contiguous(), lnoise, step, lcarry)
    with pytest.raises(ValueError):
        hip.ledits_dpmpp_step(eps, pmask, scale, lx, coef, lnoise, step, lcarry[:2].contiguous())
    carry.zero_(), lcarry.zero_()          # the good calls below are order-2 steps: they read x0_prev
    assert call() == 0 and call(eps_u=None, g_rows=None, x0_out=None) == 0 and callm() == 0 and callm(eps_u=None) == 0
    assert calll() == 0 and calll(mask=None, x0_out=None) == 0
    torch.cuda.synchronize()
    for t in (out, x0, carry, z, mcarry, lout, lx0, lcarry):
        assert torch.isfinite(t).all()


# ------------------------------------------------------------------------------------------------------------- the P2P sampler
@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.pipeline import StableDiffusionPipeline
    return StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")


def invert(pipe, seed, skip, K=3, order=2, prompt=PROMPTS[0]):
    """the noise maps of a seeded latent -> (x0 [1,4,s,s], y_skip, maps [STEPS - skip,4,s,s])"""
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    s = pipe.cfg.sample_size
    x0 = torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(seed)).to(DEV)
    pipe.scheduler.set_timesteps(STEPS)
    y, maps, xts = DDPMInversion().noise_maps(pipe, x0, [prompt], guidance_scale=G_SRC, skip=skip, rows_per_launch=K,
                                              generator=torch.Generator().manual_seed(seed + 1), solver_order=order)
    assert maps.shape == (STEPS - skip, 4, s, s) and torch.equal(y[0], xts[skip]) and torch.isfinite(maps).all()
    return x0, y, maps


class P2PRuns:
    """the ways to run one Prompt-to-Prompt edit on noise maps at a solver order"""

    def __init__(self, pipe, skip, order=2, blend=None):
        from ief_amd.p2p.model.sd_utils import P2P, _encode_prompts
        self.pipe, self.skip, self.order, self.blend = pipe, skip, order, blend
        self.n = STEPS - skip
        self.editor = P2P(pipe, STEPS)
        with torch.no_grad():
            self.context = torch.cat(_encode_prompts(pipe, PROMPTS))
        self.hw = (pipe.cfg.sample_size,) * 2

    def controller(self):
        from ief_amd.p2p.model.attention_control import AttentionRefine
        from ief_amd.p2p.model.ptp_utils import LocalBlend
        lb = None if self.blend is None else LocalBlend(self.pipe.tokenizer, PROMPTS, self.blend[0], threshold=self.blend[1], device=DEV)
        return AttentionRefine(PROMPTS, self.pipe.tokenizer, self.n, 0.8, 0.4, local_blend=lb, device=DEV)

    def sampler(self, y, maps, guidance=GUIDANCE):
        from ief_amd.p2p.model.register import unregister_attention_control as unreg
        c = self.controller()
        lat, _ = self.editor.text2image_ldm_stable(self.pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=guidance,
                                                   latent=y.clone(), return_latents=True, noise_maps=maps, skip=self.skip,
                                                   solver_order=self.order)
        assert c.cur_step == self.n, "the controller counts the edit's own steps from 0"
        unreg(self.pipe, c)
        return lat.float().cpu()

    def loop(self, y, maps, use_graph, pooled=False, guidance=GUIDANCE):
        from ief_amd import denoise
        from ief_amd.p2p.model.register import register_attention_control, unregister_attention_control as unreg
        c = self.controller()
        register_attention_control(self.pipe, c, fused=True)
        self.pipe.scheduler.set_timesteps(STEPS)
        make = denoise.acquire if pooled else denoise.FusedDenoiser
        loop = make(self.pipe, self.context, 2, self.hw, guidance, use_graph=use_graph, noise_maps=maps, skip=self.skip,
                    solver_order=self.order)
        try:
            width = 5 if self.order == 2 else 4
            assert loop.num_steps == self.n and loop.coef_table.shape == (self.n, width) and loop.coef_cur.shape == (width,)
            assert (loop.x0_prev is None) == (self.order == 1)
            if self.order == 2:
                assert loop.x0_prev.shape == loop.lat.shape
                c2 = loop.coef_table[:, 4].tolist()
                assert c2[0] == 0.0 and c2[-1] == 0.0 and all(v > 0 for v in c2[1:-1]), "order 1 on the first and the last step run"
                loop.x0_prev.fill_(NAN)          # nothing needs zeroing: the first step does not read it
            lat = loop.run(y.clone()).float().cpu()
            with pytest.raises(IndexError):
                loop.step_once()
        finally:
            loop.release()
            unreg(self.pipe, c)
        return lat, loop


def torch_rule(monkeypatch):
    """extraction and step at order 2 written out with torch fp32 operations on the device (one rounded operation each, a DEVICE
    divisor: torch divides by a host scalar through its reciprocal), in place of the kernels: the yardstick of the reconstruction"""
    dev = lambda v: torch.full((), float(v), dtype=torch.float32, device=DEV)

    def mu_of(e, x, c, c2, x0_prev):
        a, p, sigma, dirc = (float(v) for v in c[:4].tolist())
        sb_f, sa_f, sa_t = roots(a, p, torch.float32)
        x0 = (x - sb_f * e) / dev(sa_f)
        mu = sa_t * x0 + dirc * e
        if c2 != 0.0:
            mu = mu + c2 * (x0 - x0_prev)
        return mu, sigma, x0

    def maps_t(eps_u, eps_c, x_t, x_prev, coef_rows, x0_carry, out=None):
        rows, x0p = [], x0_carry.clone()
        for r in range(x_t.shape[0]):
            e = eps_c[r] if eps_u is None else eps_u[r] + float(coef_rows[r, 4]) * (eps_c[r] - eps_u[r])
            mu, sigma, x0p = mu_of(e, x_t[r], coef_rows[r], float(coef_rows[r, 5]), x0p)
            rows.append((x_prev[r] - mu) / dev(sigma))
        x0_carry.copy_(x0p)
        z = torch.stack(rows)
        return z if out is None else out.copy_(z)

    def step_t(eps_u, eps_c, x, coef, g_rows, noise, step, x0_prev, out=None, x0_out=None):
        e = eps_u + g_rows.reshape(-1, 1, 1, 1) * (eps_c - eps_u)
        mu, sigma, x0 = mu_of(e, x, coef, float(coef[4]), x0_prev.clone())
        x0_prev.copy_(x0)
        r = min(max(int(step.item()), 0), noise.shape[0] - 1)
        res = mu + sigma * noise[r]
        return res if out is None else out.copy_(res)

    def ledits_t(eps, mask, scale, x, coef, noise, step, x0_prev, out=None, x0_out=None):
        g = torch.zeros_like(eps[0])
        for k, sc in enumerate(scale.tolist()):
            if sc != 0.0:
                g = g + (sc * (1.0 if mask is None else mask[k][None])) * (eps[1 + k] - eps[0])
        mu, sigma, x0 = mu_of(eps[0] + g, x[0], coef, float(coef[4]), x0_prev.clone())
        x0_prev.copy_(x0)
        r = min(max(int(step.item()), 0), noise.shape[0] - 1)
        res = (mu + sigma * noise[r])[None]
        return res if out is None else out.copy_(res)

    monkeypatch.setattr(hip, "dpmpp_noise_maps", maps_t)
    monkeypatch.setattr(hip, "cfg_dpmpp_step", step_t)
    monkeypatch.setattr(hip, "ledits_dpmpp_step", ledits_t)


@pytest.mark.parametrize("skip", [0, 1])
def test_p2p_graph_eager_sampler_branch_and_source_row_reconstruction(small_x3, skip, monkeypatch):
    """`small`, f16x3, S = 5, AttentionRefine, g = (3.5, 15), order 2.  The figures are printed; DESIGN.md section 7 records them."""
    from ief_amd import denoise
    from ief_amd.p2p.model import sd_utils
    pipe = small_x3
    denoise.drop_pool()
    x0, y, maps = invert(pipe, 8888, skip)
    runs = P2PRuns(pipe, skip)
    graph = runs.sampler(y, maps)
    eager, _ = runs.loop(y, maps, use_graph=False)
    assert torch.equal(graph, eager), "the captured loop must equal eager stepping bit for bit"
    with monkeypatch.context() as m:
        m.setattr(sd_utils, "_fusable", lambda *a: False)            # the sampler's eager branch, under the same lowered plan
        branch = runs.sampler(y, maps)
    assert torch.equal(graph, branch), "the sampler's eager branch (`diffusion_step`) must give the same bits"

    x0c = x0[0].float().cpu()
    scale = x0c.abs().max().item()
    e_kernel = (graph[0] - x0c).abs().max().item() / scale
    with monkeypatch.context() as m:
        torch_rule(m)
        _, yt, mapst = invert(pipe, 8888, skip)
        ruled, _ = P2PRuns(pipe, skip).loop(yt, mapst, use_graph=False)
    e_torch = (ruled[0] - x0c).abs().max().item() / scale
    d_rule = (graph - ruled).abs().max().item() / scale
    # order 1 on its own maps: the term must move the target row
    _, y1, maps1 = invert(pipe, 8888, skip, order=1)
    first, _ = P2PRuns(pipe, skip, order=1).loop(y1, maps1, use_graph=True)
    e_first = (first[0] - x0c).abs().max().item() / scale
    moved = (graph[1] - first[1]).abs().max().item() / scale
    d_maps = (maps[1:-1] - maps1[1:-1]).abs().max().item() / maps1.abs().max().item() if STEPS - skip > 2 else 0.0
    print(f"small f16x3, {STEPS} steps, skip {skip}, g = {GUIDANCE}, order 2: |row 0 - x0| / max |x0| = {e_kernel:.3e} on the kernels, "
          f"{e_torch:.3e} written out in torch fp32 (bound 4 x); order 1 on its own maps {e_first:.3e}; graph vs torch loop {d_rule:.3e}; "
          f"order-2 target row - order-1 target row {moved:.3e} = {moved / max(d_rule, 1e-300):.3e} x that (floor 100); the maps of the "
          f"order-2 rows differ from order 1's by {d_maps:.3e} of their size")
    assert e_torch > 0 and e_kernel <= 4 * e_torch
    assert moved > 100 * d_rule, "the second-order term must be exercised"
    assert torch.equal(maps[0], maps1[0]) and torch.equal(maps[-1], maps1[-1]), "rows skip and S - 1 are order 1"
    denoise.drop_pool()


WORDS, THRES = [["house"], ["fall"]], 0.9905          # tests/test_gpu_local_blend.py: the threshold at which `small`'s flat maps split


def test_lowered_local_blend_runs_after_the_dpmpp_step(small_x3):
    from ief_amd import denoise
    pipe = small_x3
    _, y, maps = invert(pipe, 8888, 0)
    runs, plain = P2PRuns(pipe, 0, blend=(WORDS, THRES)), P2PRuns(pipe, 0)
    denoise.drop_pool()
    eager, _ = runs.loop(y, maps, use_graph=False)
    graph, loop = runs.loop(y, maps, use_graph=True)
    assert loop.plan.blend_w is not None
    assert torch.equal(graph, eager), "captured-graph replay must equal eager stepping bit for bit"
    assert torch.equal(graph, runs.sampler(y, maps))
    noblend, _ = plain.loop(y, maps, use_graph=True)
    assert torch.equal(graph[0], noblend[0]), "the blend leaves the source row alone"
    assert not torch.equal(graph[1], noblend[1]), "the blend must act on the target row"
    denoise.drop_pool()


@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_p2p_graph_eager_and_sampler_branch_on_tiny(precision, monkeypatch):
    from ief_amd import denoise
    from ief_amd.p2p.model import sd_utils
    from ief_amd.pipeline import StableDiffusionPipeline
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", precision=precision)
    denoise.drop_pool()
    for skip in (0, 1):
        x0, y, maps = invert(pipe, 8888, skip)
        runs = P2PRuns(pipe, skip)
        graph = runs.sampler(y, maps)
        eager, _ = runs.loop(y, maps, use_graph=False)
        assert torch.equal(graph, eager), "the captured loop must equal eager stepping bit for bit"
        with monkeypatch.context() as m:
            m.setattr(sd_utils, "_fusable", lambda *a: False)
            assert torch.equal(graph, runs.sampler(y, maps)), "the sampler's eager branch must give the same bits"
        assert not torch.equal(graph[0], graph[1])
        e = (graph[0] - x0[0].cpu()).abs().max().item() / x0.abs().max().item()
        print(f"tiny {precision}, skip {skip}, order 2: |row 0 - x0| / max |x0| = {e:.3e}")
    denoise.drop_pool()


def test_pooled_loop_repointed_and_edit_many(small_x3):
    from ief_amd import denoise
    from ief_amd.p2p.model.register import unregister_attention_control as unreg
    pipe = small_x3
    _, ya, mapsa = invert(pipe, 8888, 1)
    _, yb, mapsb = invert(pipe, 4242, 1)
    ga, gb = GUIDANCE, (2.0, 9.0)
    runs = P2PRuns(pipe, 1)
    denoise.drop_pool()
    fresh_b, _ = runs.loop(yb, mapsb, use_graph=True, guidance=gb)                 # never pooled: its own capture
    first, loop1 = runs.loop(ya, mapsa, use_graph=True, pooled=True, guidance=ga)
    second, loop2 = runs.loop(yb, mapsb, use_graph=True, pooled=True, guidance=gb)
    assert loop2 is loop1 and loop2.graph is not None, "equal signatures: the captured loop is taken from the pool, not rebuilt"
    assert not torch.equal(first, second)
    assert torch.equal(second, fresh_b), "a pooled loop re-pointed at the second image's maps and scales must give that image's fresh run"
    # the other order is another pool entry, and a loop refuses a job of the other order
    _, y1, maps1 = invert(pipe, 8888, 1, order=1)
    _, loop3 = P2PRuns(pipe, 1, order=1).loop(y1, maps1, use_graph=True, pooled=True)
    assert loop3 is not loop1 and loop3.solver_order == 1 and loop1.solver_order == 2
    with pytest.raises(ValueError, match="solver order"):
        loop3.rebind(runs.context, ga, None, None, None, mapsa, 1, None, None, 2)
    with pytest.raises(ValueError, match="solver order"):
        loop1.rebind(runs.context, ga, None, None, None, mapsa, 1)
    again, loop4 = runs.loop(ya, mapsa, use_graph=True, pooled=True, guidance=ga)
    assert loop4 is loop1 and torch.equal(again, first)
    denoise.drop_pool()

    # edit_many with two jobs == one call per job
    jobs = [(PROMPTS, runs.controller(), ya.clone(), None, None, (mapsa, 1, ga, 2)), (PROMPTS, runs.controller(), yb.clone(), None, None, (mapsb, 1, gb, 2))]
    many = runs.editor.edit_many(pipe, jobs, num_inference_steps=STEPS)
    for (img, _), (y, maps, g) in zip(many, ((ya, mapsa, ga), (yb, mapsb, gb))):
        c = runs.controller()
        one, _ = runs.editor.text2image_ldm_stable(pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=g, latent=y.clone(),
                                                   noise_maps=maps, skip=1, solver_order=2)
        unreg(pipe, c)
        assert (img == one).all(), "edit_many must give what one call per job gives"
    unreg(pipe, None)
    denoise.drop_pool()


def test_pie_driver_20_second_order_steps_in_flight_match_per_image(tmp_path):
    script = os.path.join(PKG, "p2p", "test.py")
    base = ["--sd_version", "small", "--synthetic", "2", "--inversion_type", "ddpm", "--num_steps", "20", "--solver_order", "2",
            "--invert_batch", "4"]
    a, b = tmp_path / "a", tmp_path / "b"
    one, many = run_mixed([([script] + base + ["--exp_path", str(a)], tmp_path / "cwd_a"),
                           ([script] + base + ["--in_flight", "2", "--exp_path", str(b)], tmp_path / "cwd_b")],
                          in_process=(1,))
    assert one.last_json()["images"] == 2 and many.last_json()["images"] == 2
    dirs = sorted(x for x in os.listdir(a) if x.startswith("syn_"))
    assert len(dirs) == 2 and sorted(x for x in os.listdir(b) if x.startswith("syn_")) == dirs
    for d in dirs:
        for name in ("inversion.png", "edit.png"):
            pa, pb = np.array(Image.open(a / d / name)).astype(int), np.array(Image.open(b / d / name)).astype(int)
            assert pa.shape == pb.shape and np.abs(pa - pb).max() == 0, (d, name, np.abs(pa - pb).max())
        src, inv = (np.array(Image.open(a / d / n)).astype(int) for n in ("inversion.png", "edit.png"))
        assert np.abs(src - inv).max() > 0, "the edit must differ from the reconstruction"


# ------------------------------------------------------------------------------------------------------------- LEDITS++
def ledits_edit(pipe, y, maps, skip, order=2, use_graph=True, **kw):
    from ief_amd.ledits.model.sd_utils import LEDITS
    args = dict(edit_guidance_scale=[5.0, 7.0], edit_threshold=0.75)
    args.update(kw)
    lat, masks = LEDITS(pipe, STEPS, order).edit(pipe, y, maps, skip, CONCEPTS, use_graph=use_graph, **args)
    assert pipe.unet._plan is None, "the plan is unregistered when the edit returns"
    return lat.float().cpu(), masks


def test_ledits_graph_equals_eager_and_reconstruction_with_no_concept_active(small_x3, monkeypatch):
    """`small`, f16x3, S = 5, skip 1, E = 2, order 2, empty source prompt.  The figures are printed; DESIGN.md section 7 records them."""
    from ief_amd import denoise
    pipe = small_x3
    denoise.drop_pool()
    x0, y, maps = invert(pipe, 8888, 1, prompt="")
    kw = dict(reverse=[1], edit_warmup_steps=[1, 0], keep_masks=True)
    graph, gm = ledits_edit(pipe, y, maps, 1, use_graph=True, **kw)
    eager, em = ledits_edit(pipe, y, maps, 1, use_graph=False, **kw)
    assert torch.equal(graph, eager) and torch.equal(gm, em), "the captured graph must equal eager stepping bit for bit"
    _, y1, maps1 = invert(pipe, 8888, 1, prompt="", order=1)
    first, _ = ledits_edit(pipe, y1, maps1, 1, order=1, **kw)
    assert not torch.equal(graph, first), "the second-order term must act"
    # every scale 0: the latent ends on x0
    x0c = x0.float().cpu()
    scale = x0c.abs().max().item()
    lat, _ = ledits_edit(pipe, y, maps, 1, edit_warmup_steps=STEPS)
    e_kernel = (lat - x0c).abs().max().item() / scale
    with monkeypatch.context() as m:
        torch_rule(m)
        _, yt, mapst = invert(pipe, 8888, 1, prompt="")
        ruled, _ = ledits_edit(pipe, yt, mapst, 1, edit_warmup_steps=STEPS, use_graph=False)
    e_torch = (ruled - x0c).abs().max().item() / scale
    moved = (graph - x0c).abs().max().item() / scale
    print(f"ledits small f16x3, {STEPS} steps, skip 1, order 2, no concept active: |x_final - x0| / max |x0| = {e_kernel:.3e} on the "
          f"kernels, {e_torch:.3e} written out in torch fp32 (bound 4 x); with two active concepts the result is {moved:.3e} away")
    assert e_torch > 0 and e_kernel <= 4 * e_torch
    assert moved >= 100 * e_kernel, "active concepts must move the image"
    denoise.drop_pool()


def test_ledits_f16_f32_modes_run_without_the_cross_mask():
    from ief_amd import denoise
    from ief_amd.pipeline import StableDiffusionPipeline
    for precision in ("f16", "f32"):
        pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", precision=precision)
        denoise.drop_pool()
        _, y, maps = invert(pipe, 8888, 1, prompt="")
        graph, _ = ledits_edit(pipe, y, maps, 1, cross_attn_mask=False)
        eager, _ = ledits_edit(pipe, y, maps, 1, cross_attn_mask=False, use_graph=False)
        _, y1, maps1 = invert(pipe, 8888, 1, prompt="", order=1)
        first, _ = ledits_edit(pipe, y1, maps1, 1, order=1, cross_attn_mask=False)
        assert torch.equal(graph, eager) and torch.isfinite(graph).all() and not torch.equal(graph, first)
        denoise.drop_pool()


def test_ledits_pie_driver_20_second_order_steps_writes_its_images(tmp_path):
    script = os.path.join(PKG, "ledits", "test.py")
    base = ["--sd_version", "small", "--synthetic", "2", "--seed", "7", "--num_steps", "20", "--solver_order", "2",
            "--edit_prompt", "glasses", "a red hat", "--remove", "1"]
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
