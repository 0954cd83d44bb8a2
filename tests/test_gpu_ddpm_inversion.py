"""Edit-friendly DDPM inversion on a real MI355X: the per-row CFG + eta = 1 step (`ief_cfg_ddpm_step_f32`), the extraction of the
noise maps (`ief_ddpm_noise_maps_f32`), the mixed-timestep UNet forward the extraction rests on, the captured edit loop, the samplers
and the PIE driver.

The rule (`p2p/inversion/ddpm.py`): mu = sqrt(a_to) (x - sqrt(1 - a_from) eps) / sqrt(a_from) + dir eps with eps = eps_u + g_b (eps_c -
eps_u), x' = mu + sigma z, z = (x_prev - mu) / sigma; all fp32, every operation rounded.  Stated checks (every test prints its figures):
    sigma = 0, dir = fp32 sqrt(1 - a_to)     x_out and x0_out bit-equal to `ief_cfg_ddim_step_f32` (uniform scale, with / without eps_u)
    mixed g_rows                             row b bit-equal to a launch whose rows all carry g_b; in place == out of place
    against fp64                             max |kernel - fp64| <= 4 x max |the same expression in torch fp32 on the CPU - fp64|
    round trip of the kernel pair            |step(noise_maps(x_t, x_prev, eps)) - x_prev| <= 2^-24 (4 |x_prev - mu| + 2 |x_prev|) elementwise:
                                             d = fl(x_prev - mu), q = fl(d / sigma), r = fl(sigma q) are three rounded operations on d
                                             (|r - (x_prev - mu)| <= (3 u + O(u^2)) |d|, u = 2^-24) and fl(mu + r) adds at most
                                             u |mu + r| <= u (|x_prev| + 3 u |d|): 3 |d| + |x_prev| to first order, stated with the slack
                                             of the issue; mu is the same bits in both kernels (one device function)
    mixed-timestep forward                   one batched forward with one `temb_row` row per batch row == the batch-1 forwards, bit for
                                             bit in f16; in f16x3 within 4 x the distance of a batched forward at ONE timestep
    whole loop                               captured graph == eager stepping == the sampler's eager branch, bit for bit; the source
                                             row ends on x0 within 4 x the error of the same run with extraction and step written out
                                             in torch fp32; the plain DDIM edit's source row at the target guidance is >= 100 x
                                             farther from x0; the target row is >= 100 x that error away from the source row
    pooled loop re-pointed, edit_many, --invert_batch / --in_flight: bit for bit / the same pixels
Measured on an MI355X: step kernel max |. - fp64| 8.1e-6 ... 1.6e-5 against 5.4e-6 ... 1.6e-5 of torch fp32 on the CPU (1.00 ... 1.58 x,
bound 4); round trip at most 0.570 of its bound; mixed-timestep forward: tiny f16 0 (bit-equal), small f16x3 1.000e-6 of max |eps| against
1.032e-6 for the same rows at one timestep; `small`, f16x3, 4 steps, g = (3.5, 15): |row 0 - x0| / max |x0| = 1.871e-5 on the kernels and
1.871e-5 written out in torch fp32 at skip 0, 4.914e-6 and 4.914e-6 at skip 1; the plain ddim edit's source row at guidance 15 is 1.334
away (7.1e4 x / 2.7e5 x), the target row 0.775 / 0.220 from the source row (4.1e4 x / 4.5e4 x); maps at 3 and at 1 rows per launch differ by
2.3e-6 of their size; tiny f32 1.6e-5 / 6.5e-6, tiny f16 1.0e-2 / 3.5e-3 (fp16 activations; printed, not bounded).
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip  # noqa: E402
from _procs import run_mixed  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "image-editing-framework_amd")
U = 2.0 ** -24
IEF_EINVAL, IEF_ESHAPE = -1, -2          # csrc/ief_common.h
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]
STEPS, G_SRC, G_TAR = 4, 3.5, 15.0
GUIDANCE = (G_SRC, G_TAR)


def ddpm_sigma_dir(a, p):
    """fp64 on the host, rounded to fp32 once (`DDIMScheduler.ddpm_coeffs`)"""
    a, p = np.float64(np.float32(a)), np.float64(np.float32(p))
    v = (1 - p) / (1 - a) * (1 - a / p)
    return float(np.float32(np.sqrt(v))), float(np.float32(np.sqrt(1 - p - v)))


def mu_torch(eu, ec, x, a, p, dirc, g_rows):
    """the mean in torch, in the kernel's operation order, in the dtype of the inputs (fp32: every operation rounded once; the
    coefficients' square roots are taken in that dtype from the fp32 values); -> (mu, x0)"""
    dt = x.dtype
    t = lambda v: torch.tensor(float(np.float32(v)), dtype=dt)
    one = torch.tensor(1.0, dtype=dt)
    sb_f, sa_f, sa_t = torch.sqrt(one - t(a)).item(), torch.sqrt(t(a)).item(), torch.sqrt(t(p)).item()
    e = ec
    if eu is not None:
        g = g_rows.to(dt).reshape(-1, *([1] * (x.dim() - 1)))
        e = eu + g * (ec - eu)
    x0 = (x - sb_f * e) / sa_f
    return sa_t * x0 + float(np.float32(dirc)) * e, x0


# ------------------------------------------------------------------------------------------------------------- the step kernel
def kernel_inputs(Bp, row_elems, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    eu, ec, x = r(Bp, row_elems), r(Bp, row_elems), r(Bp, row_elems)
    noise = torch.stack([r(row_elems), 1e-3 * r(row_elems), 50 * r(row_elems)])          # three rows, three scales
    return eu, ec, x, noise


A_F, A_T = 0.55, 0.71
STEP_ROWS = ((0, 0), (1, 1), (2, 2), (7, 2), (-1, 0))          # (device step, the row it clamps to)


@pytest.mark.parametrize("Bp", [2, 3])
@pytest.mark.parametrize("row_elems", [256, 252, 16384])
def test_ddpm_step_kernel(Bp, row_elems):
    eu_h, ec_h, x_h, noise_h = kernel_inputs(Bp, row_elems, 31 * Bp + row_elems)
    eu, ec, x, noise = (t.to(DEV) for t in (eu_h, ec_h, x_h, noise_h))
    sigma, dirc = ddpm_sigma_dir(A_F, A_T)
    g_h = torch.tensor([G_SRC, G_TAR, 7.5][:Bp])
    g_rows = g_h.to(DEV)
    coef = torch.tensor([A_F, A_T, sigma, dirc], device=DEV)
    step0 = torch.zeros(1, dtype=torch.int32, device=DEV)

    # sigma = 0 and dir = fp32 sqrt(1 - a_to): the plain kernel, bit for bit
    dir_plain = torch.sqrt(torch.tensor(1.0) - torch.tensor(A_T)).item()
    coef0 = torch.tensor([A_F, A_T, 0.0, dir_plain], device=DEV)
    for cfg in (True, False):
        u = eu if cfg else None
        x0p = torch.empty_like(x)
        xp = hip.cfg_ddim_step(u, ec, x, torch.tensor([A_F, A_T, 7.5, 0.0], device=DEV), x0_out=x0p)
        x0d = torch.full_like(x, float("nan"))
        out = hip.cfg_ddpm_step(u, ec, x, coef0, torch.full((Bp,), 7.5, device=DEV) if cfg else None, noise, step0,
                                out=torch.full_like(x, float("nan")), x0_out=x0d)
        torch.cuda.synchronize()
        assert torch.equal(out, xp) and torch.equal(x0d, x0p), f"sigma = 0 must be the plain CFG + DDIM step (cfg={cfg})"

    worst_ratio, worst_k, worst_y = 0.0, 0.0, 0.0
    for s, r in STEP_ROWS:
        step = torch.tensor([s], dtype=torch.int32, device=DEV)
        x0o = torch.full_like(x, float("nan"))
        out = hip.cfg_ddpm_step(eu, ec, x, coef, g_rows, noise, step, out=torch.full_like(x, float("nan")), x0_out=x0o)
        torch.cuda.synchronize()
        assert int(step.item()) == s, "the kernel only reads the step"
        # row b of the mixed launch == a launch whose rows all carry g_b
        for b in range(Bp):
            uni = hip.cfg_ddpm_step(eu, ec, x, coef, torch.full((Bp,), float(g_h[b]), device=DEV), noise, step)
            assert torch.equal(uni[b], out[b]), f"row {b} must not depend on the other rows' scales (step={s})"
        if Bp > 1:
            assert not torch.equal(uni[0], out[0]), "the scales must act"
        xc = x.clone()
        assert hip.cfg_ddpm_step(eu, ec, xc, coef, g_rows, noise, step, out=xc) is xc
        assert torch.equal(xc, out), "in place == out of place"
        assert torch.equal(hip.cfg_ddpm_step(eu, ec, x, coef, g_rows, noise, step), out), "x0_out is optional"
        # fp64 restatement; the yardstick is the same expression in torch fp32 on the CPU
        mu64, x064 = mu_torch(eu_h.double(), ec_h.double(), x_h.double(), A_F, A_T, dirc, g_h)
        want64 = mu64 + float(np.float32(sigma)) * noise_h[r].double()
        mu32, x032 = mu_torch(eu_h, ec_h, x_h, A_F, A_T, dirc, g_h)
        want32 = mu32 + float(np.float32(sigma)) * noise_h[r]
        err_k = max((out.cpu().double() - want64).abs().max().item(), (x0o.cpu().double() - x064).abs().max().item())
        err_y = max((want32.double() - want64).abs().max().item(), (x032.double() - x064).abs().max().item())
        assert err_y > 0
        assert err_k <= 4 * err_y, f"step={s}: kernel {err_k:.3e} vs fp64, torch fp32 {err_y:.3e} (bound 4 x)"
        if err_k / err_y > worst_ratio:
            worst_ratio, worst_k, worst_y = err_k / err_y, err_k, err_y
        other = noise_h[(r + 1) % 3].double()
        assert (out.cpu().double() - (mu64 + float(np.float32(sigma)) * other)).abs().max().item() > 100 * err_k, "the clamped row is read"
    # no CFG: eps = eps_c, g_rows may be missing
    out = hip.cfg_ddpm_step(None, ec, x, coef, None, noise, step0)
    mu64, _ = mu_torch(None, ec_h.double(), x_h.double(), A_F, A_T, dirc, None)
    mu32, _ = mu_torch(None, ec_h, x_h, A_F, A_T, dirc, None)
    w64 = mu64 + float(np.float32(sigma)) * noise_h[0].double()
    e_k = (out.cpu().double() - w64).abs().max().item()
    e_y = ((mu32 + float(np.float32(sigma)) * noise_h[0]).double() - w64).abs().max().item()
    assert e_k <= 4 * e_y
    print(f"ddpm step Bp={Bp} row_elems={row_elems}: max |kernel - fp64| {worst_k:.3e}, torch fp32 on the CPU {worst_y:.3e}: "
          f"{worst_ratio:.2f} x (bound 4); without eps_u {e_k:.3e} vs {e_y:.3e}")


# ------------------------------------------------------------------------------------------------------------- the kernel pair
def test_noise_maps_then_step_returns_x_prev_within_the_derived_bound():
    sets = [(0.55, 0.71), (0.9, 0.95), (0.02, 0.05), (0.3, 0.9991), (0.6, 0.62)]
    scales = [1.0, 1e-3, 1e2, 1.0, 10.0]
    gs = [3.5, 15.0, 1.0, 7.5, 0.0]
    worst = 0.0
    for row_elems in (252, 4096):
        g = torch.Generator().manual_seed(row_elems)
        R = len(sets)
        eu, ec, xt = (torch.randn(R, row_elems, generator=g).to(DEV) for _ in range(3))
        xprev = torch.stack([s * torch.randn(row_elems, generator=g) for s in scales]).to(DEV)
        rows = []
        for k, ((a, p), gk) in enumerate(zip(sets, gs)):
            sigma, dirc = ddpm_sigma_dir(a, p)
            if k == 3:
                sigma, dirc = 0.0, float(np.float32(np.sqrt(1 - np.float64(np.float32(p)))))          # the sigma = 0 row
            rows.append([a, p, sigma, dirc, gk])
        coef_rows = torch.tensor(rows, dtype=torch.float32, device=DEV)
        z = hip.ddpm_noise_maps(eu, ec, xt, xprev, coef_rows, out=torch.full_like(xt, float("nan")))
        torch.cuda.synchronize()
        assert torch.isfinite(z).all()
        assert (z[3] == 0).all(), "a sigma = 0 row is exactly zero"
        for r in range(R):
            step = torch.tensor([r], dtype=torch.int32, device=DEV)
            args = (eu[r:r + 1], ec[r:r + 1], xt[r:r + 1])
            c0 = coef_rows[r, :4].clone()
            c0[2] = 0.0
            mu = hip.cfg_ddpm_step(*args, c0.contiguous(), coef_rows[r, 4:5].contiguous(), z, step)[0]          # the mean's own bits
            back = hip.cfg_ddpm_step(*args, coef_rows[r, :4].contiguous(), coef_rows[r, 4:5].contiguous(), z, step)[0]
            if r == 3:
                assert torch.equal(back, mu), "sigma = 0 adds nothing"
                continue
            xp = xprev[r].double()
            bound = U * (4 * (xp - mu.double()).abs() + 2 * xp.abs())
            ratio = ((back.double() - xp).abs() / bound.clamp_min(1e-300)).max().item()
            assert ratio <= 1, f"row {r} (a, p, g = {sets[r]}, {gs[r]}; scale {scales[r]}): |round trip - x_prev| / bound = {ratio:.3f}"
            worst = max(worst, ratio)
            # the map itself against fp64 on the kernel's own mean: two rounded operations
            z64 = (xp - mu.double()) / np.float64(np.float32(rows[r][2]))
            assert ((z[r].double() - z64).abs() <= 2.01 * U * z64.abs() + 1e-45).all()
        # without eps_u the scale column is not read
        z1 = hip.ddpm_noise_maps(None, ec, xt, xprev, coef_rows)
        cr = coef_rows.clone()
        cr[:, 4] = 99.0
        assert torch.equal(hip.ddpm_noise_maps(None, ec, xt, xprev, cr), z1)
    print(f"noise_maps -> step, 5 rows x (252, 4096) elements: worst |x' - x_prev| / (2^-24 (4 |x_prev - mu| + 2 |x_prev|)) = {worst:.3f} (bound 1)")


def test_refusals_launch_nothing():
    lib = hip.load()
    eu, ec, x, noise = (t.to(DEV) for t in kernel_inputs(2, 256, 5))
    coef = torch.tensor([A_F, A_T, *ddpm_sigma_dir(A_F, A_T)], device=DEV)
    g_rows = torch.tensor([G_SRC, G_TAR], device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, x0 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    p = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(eps_u=p(eu), eps_c=p(ec), x=p(x), x_out=p(out), x0_out=p(x0), coef=p(coef), g_rows=p(g_rows), n=x.numel(),
                row_elems=256, noise=p(noise), noise_rows=3, step=p(step))

    def call(**kw):
        a = dict(good, **kw)
        return lib.ief_cfg_ddpm_step_f32(a["eps_u"], a["eps_c"], a["x"], a["x_out"], a["x0_out"], a["coef"], a["g_rows"], a["n"],
                                         a["row_elems"], a["noise"], a["noise_rows"], a["step"], stream)

    for name in ("eps_c", "x", "x_out", "coef", "noise", "step", "g_rows"):
        assert call(**{name: None}) == IEF_EINVAL, name
    for kw in (dict(n=0), dict(n=-512), dict(row_elems=0), dict(row_elems=-256), dict(row_elems=200), dict(noise_rows=0),
               dict(noise_rows=-1)):
        assert call(**kw) == IEF_ESHAPE, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(x0).all(), "a refused step must not launch"

    coef_rows = torch.tensor([[A_F, A_T, *ddpm_sigma_dir(A_F, A_T), G_SRC]] * 2, device=DEV)
    z = torch.full_like(x, float("nan"))
    goodm = dict(eps_u=p(eu), eps_c=p(ec), x_t=p(x), x_prev=p(x), z_out=p(z), coef_rows=p(coef_rows), R=2, row_elems=256)

    def callm(**kw):
        a = dict(goodm, **kw)
        return lib.ief_ddpm_noise_maps_f32(a["eps_u"], a["eps_c"], a["x_t"], a["x_prev"], a["z_out"], a["coef_rows"], a["R"],
                                           a["row_elems"], stream)

    for name in ("eps_c", "x_t", "x_prev", "z_out", "coef_rows"):
        assert callm(**{name: None}) == IEF_EINVAL, name
    for kw in (dict(R=0), dict(R=-2), dict(row_elems=0), dict(row_elems=-256)):
        assert callm(**kw) == IEF_ESHAPE, kw
    torch.cuda.synchronize()
    assert torch.isnan(z).all(), "a refused extraction must not launch"

    # the bindings' own checks, in front of the library
    with pytest.raises(ValueError):
        hip.cfg_ddpm_step(eu, ec, x, coef, g_rows, noise[:, :128].contiguous(), step)
    with pytest.raises(ValueError):
        hip.cfg_ddpm_step(eu, ec, x, coef, g_rows[:1].contiguous(), noise, step)
    with pytest.raises(ValueError):
        hip.cfg_ddpm_step(eu, ec, x, coef[:3].contiguous(), g_rows, noise, step)
    with pytest.raises(TypeError):
        hip.cfg_ddpm_step(eu, ec, x, coef, g_rows, noise, step.long())
    with pytest.raises(TypeError):
        hip.cfg_ddpm_step(eu, ec, x, coef, None, noise, step)
    with pytest.raises(TypeError):
        hip.cfg_ddpm_step(eu, ec, x, coef, g_rows, noise.double(), step)
    with pytest.raises(ValueError):
        hip.ddpm_noise_maps(eu, ec, x, x, coef_rows[:, :4].contiguous())
    with pytest.raises(ValueError):
        hip.ddpm_noise_maps(eu, ec, x, x[:1], coef_rows)
    assert call() == 0 and call(eps_u=None, g_rows=None, x0_out=None) == 0 and callm() == 0 and callm(eps_u=None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(z).all()


# ------------------------------------------------------------------------------------------------------------- mixed timesteps
def _mixed_forward_distances(pipe):
    """four rows at four timesteps: one batched forward with one temb row per batch row against four batch-1 forwards, and -- the
    existing case -- the same four rows at ONE timestep, batched against batch-1; -> (mixed, existing) max |.| / max |eps|"""
    from ief_amd.p2p.model.sd_utils import _encode_prompts
    unet = pipe.unet
    s = pipe.cfg.sample_size
    pipe.scheduler.set_timesteps(STEPS)
    ts = pipe.scheduler.timesteps.tolist()
    y = torch.randn(4, 4, s, s, generator=torch.Generator().manual_seed(11)).to(DEV)
    with torch.no_grad():
        _, cond = _encode_prompts(pipe, PROMPTS[:1])
        ctx = unet._act(cond.expand(4, -1, -1).contiguous())
        ctx1 = unet._act(cond.contiguous())
        rows = unet.time_rows(torch.tensor(ts, dtype=torch.float32, device=DEV)).contiguous()
        mixed = unet(y, encoder_hidden_states=ctx, temb_row=rows)["sample"].clone()
        single = torch.cat([unet(y[i:i + 1], encoder_hidden_states=ctx1, temb_row=rows[i:i + 1].contiguous())["sample"] for i in range(4)])
        one_t = unet(y, encoder_hidden_states=ctx, temb_row=rows[1:2].contiguous())["sample"].clone()
        one_t_single = torch.cat([unet(y[i:i + 1], encoder_hidden_states=ctx1, temb_row=rows[1:2].contiguous())["sample"]
                                  for i in range(4)])
    assert not torch.equal(mixed, one_t), "the rows' own timesteps must act"
    scale = single.abs().max().item()
    return (mixed - single).abs().max().item() / scale, (one_t - one_t_single).abs().max().item() / scale


def test_mixed_timestep_forward_f16_is_the_batch_1_forwards_bit_for_bit():
    from ief_amd.pipeline import StableDiffusionPipeline
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", precision="f16")
    mixed, existing = _mixed_forward_distances(pipe)
    print(f"tiny f16, four rows at four timesteps: batched vs batch-1 max |.| / max |eps| = {mixed:.3e} (one timestep: {existing:.3e}); bound 0")
    assert mixed == 0.0


# ------------------------------------------------------------------------------------------------------------- the P2P sampler
@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.pipeline import StableDiffusionPipeline
    return StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")


def test_mixed_timestep_forward_f16x3_within_the_existing_batched_distance(small_x3):
    mixed, existing = _mixed_forward_distances(small_x3)
    print(f"small f16x3, four rows at four timesteps: batched vs batch-1 max |.| / max |eps| = {mixed:.3e}; the same rows at one "
          f"timestep (the batched DDIM inversion's case) {existing:.3e}; bound 4 x that")
    assert mixed <= 4 * existing


def invert(pipe, seed, skip, K=3, steps=STEPS):
    """the noise maps of a seeded latent -> (x0 [1,4,s,s], y_skip, maps [steps - skip,4,s,s], xts)"""
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    s = pipe.cfg.sample_size
    x0 = torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(seed)).to(DEV)
    pipe.scheduler.set_timesteps(steps)
    y, maps, xts = DDPMInversion().noise_maps(pipe, x0, [PROMPTS[0]], guidance_scale=G_SRC, skip=skip, rows_per_launch=K,
                                              generator=torch.Generator().manual_seed(seed + 1))
    assert maps.shape == (steps - skip, 4, s, s) and xts.shape == (steps + 1, 4, s, s) and torch.equal(xts[-1], x0[0])
    assert torch.equal(y[0], xts[skip]) and torch.isfinite(maps).all()
    return x0, y, maps, xts


def p2p_context(pipe):
    from ief_amd.p2p.model.sd_utils import _encode_prompts
    with torch.no_grad():
        u, c = _encode_prompts(pipe, PROMPTS)
    return torch.cat([u, c])


class P2PRuns:
    """the ways to run one Prompt-to-Prompt edit on noise maps"""

    def __init__(self, pipe, skip, blend=None, guidance=GUIDANCE):
        from ief_amd.p2p.model.sd_utils import P2P
        self.pipe, self.skip, self.blend, self.guidance = pipe, skip, blend, guidance
        self.n = STEPS - skip
        self.editor = P2P(pipe, STEPS)
        self.context = p2p_context(pipe)
        self.hw = (pipe.cfg.sample_size,) * 2

    def controller(self, cls=None, n=None):
        from ief_amd.p2p.model.attention_control import AttentionRefine
        from ief_amd.p2p.model.ptp_utils import LocalBlend
        lb = None if self.blend is None else LocalBlend(self.pipe.tokenizer, PROMPTS, self.blend[0], threshold=self.blend[1], device=DEV)
        return (cls or AttentionRefine)(PROMPTS, self.pipe.tokenizer, n or self.n, 0.8, 0.4, local_blend=lb, device=DEV)

    def sampler(self, y, maps, guidance=None, cls=None):
        """`P2P.text2image_ldm_stable`: the captured loop (or, with `_fusable` patched / a generic controller, its eager branch)"""
        from ief_amd.p2p.model.register import unregister_attention_control as unreg
        c = self.controller(cls)
        lat, _ = self.editor.text2image_ldm_stable(self.pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=guidance or self.guidance,
                                                   latent=y.clone(), return_latents=True, noise_maps=maps, skip=self.skip)
        assert c.cur_step == self.n, "the controller counts the edit's own steps from 0"
        unreg(self.pipe, c)
        return lat.float().cpu()

    def loop(self, y, maps, use_graph, pooled=False, guidance=None):
        from ief_amd import denoise
        from ief_amd.p2p.model.register import register_attention_control, unregister_attention_control as unreg
        c = self.controller()
        register_attention_control(self.pipe, c, fused=True)
        self.pipe.scheduler.set_timesteps(STEPS)
        make = denoise.acquire if pooled else denoise.FusedDenoiser
        loop = make(self.pipe, self.context, 2, self.hw, guidance or self.guidance, use_graph=use_graph, noise_maps=maps, skip=self.skip)
        try:
            assert loop.num_steps == self.n and loop.coef_table.shape == (self.n, 4) and loop.temb_table.shape[0] == self.n
            lat = loop.run(y.clone()).float().cpu()
            with pytest.raises(IndexError):
                loop.step_once()
        finally:
            loop.release()
            unreg(self.pipe, c)
        assert c.cur_step == self.n
        return lat, loop


def torch_rule(monkeypatch):
    """extraction and step written out with torch fp32 operations (on the device, one rounded operation each), in place of the two
    kernels: the yardstick of the source-row reconstruction"""
    def coefs(c):
        a, p, sigma, dirc = (float(v) for v in c[:4].tolist())
        one = torch.tensor(1.0)
        return (torch.sqrt(one - torch.tensor(a)).item(), torch.sqrt(torch.tensor(a)).item(), torch.sqrt(torch.tensor(p)).item(),
                sigma, dirc)

    dev = lambda v: torch.full((), v, dtype=torch.float32, device=DEV)      # a DEVICE divisor: torch divides by a host scalar through
    # its reciprocal, which is not the kernel's (correctly rounded) division

    def mu_of(eu, ec, x, c, g):
        sb_f, sa_f, sa_t, sigma, dirc = coefs(c)
        e = eu + g * (ec - eu)
        x0 = (x - sb_f * e) / dev(sa_f)
        return sa_t * x0 + dirc * e, sigma

    def maps_t(eps_u, eps_c, x_t, x_prev, coef_rows, out=None):
        rows = []
        for r in range(x_t.shape[0]):
            mu, sigma = mu_of(eps_u[r], eps_c[r], x_t[r], coef_rows[r], float(coef_rows[r, 4]))
            rows.append((x_prev[r] - mu) / dev(sigma))
        z = torch.stack(rows)
        return z if out is None else out.copy_(z)

    def step_t(eps_u, eps_c, x, coef, g_rows, noise, step, out=None, x0_out=None):
        g = g_rows.reshape(-1, 1, 1, 1)
        mu, sigma = mu_of(eps_u, eps_c, x, coef, g)
        r = min(max(int(step.item()), 0), noise.shape[0] - 1)
        res = mu + sigma * noise[r]
        return res if out is None else out.copy_(res)

    monkeypatch.setattr(hip, "ddpm_noise_maps", maps_t)
    monkeypatch.setattr(hip, "cfg_ddpm_step", step_t)


def ddim_plain_source_row(pipe, x0, guidance):
    """the existing `ddim` route: DDIM inversion of x0, then the plain P2P edit at `guidance` -> its source row"""
    from ief_amd.p2p.inversion.ddim import ddim_inversion
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.register import unregister_attention_control as unreg
    from ief_amd.p2p.model.sd_utils import P2P
    pipe.scheduler.set_timesteps(STEPS)
    latents, _ = ddim_inversion().ddim_inversion_loop(pipe, x0, [PROMPTS[0]])
    c = AttentionRefine(PROMPTS, pipe.tokenizer, STEPS, 0.8, 0.4, device=DEV)
    lat, _ = P2P(pipe, STEPS).text2image_ldm_stable(pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=guidance,
                                                    latent=latents[-1].clone(), return_latents=True)
    unreg(pipe, c)
    return lat[0].float().cpu()


@pytest.mark.parametrize("skip", [0, 1])
def test_p2p_graph_eager_sampler_branch_and_source_row_reconstruction(small_x3, skip, monkeypatch):
    """Measured on an MI355X, |row 0 - x0| / max |x0|: skip 0: 1.871e-5 on the kernels, 1.871e-5 with extraction and step written out
    in torch fp32 (the yardstick; bound 4 x); skip 1: 4.914e-6 and 4.914e-6."""
    from ief_amd import denoise
    from ief_amd.p2p.model import sd_utils
    pipe = small_x3
    denoise.drop_pool()
    x0, y, maps, xts = invert(pipe, 8888, skip)
    _, y1, maps1, _ = invert(pipe, 8888, skip, K=1)
    d_k = (maps - maps1).abs().max().item() / maps1.abs().max().item()
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
        _, yt, mapst, _ = invert(pipe, 8888, skip)
        ruled, _ = P2PRuns(pipe, skip).loop(yt, mapst, use_graph=False)
    e_torch = (ruled[0] - x0c).abs().max().item() / scale
    plain0 = ddim_plain_source_row(pipe, x0, G_TAR)
    e_plain = (plain0 - x0c).abs().max().item() / scale
    moved = (graph[1] - graph[0]).abs().max().item() / scale
    print(f"small f16x3, {STEPS} steps, skip {skip}, g = {GUIDANCE}: |row 0 - x0| / max |x0| = {e_kernel:.3e} on the kernels, {e_torch:.3e} "
          f"written out in torch fp32 (bound 4 x); plain ddim edit at guidance {G_TAR}: {e_plain:.3e} = {e_plain / max(e_kernel, 1e-300):.3e} x "
          f"(floor 100); target row - source row {moved:.3e} = {moved / max(e_kernel, 1e-300):.3e} x (floor 100); maps at 3 vs 1 rows per "
          f"launch differ by {d_k:.3e} of their size")
    assert e_torch > 0 and e_kernel <= 4 * e_torch
    assert e_plain >= 100 * e_kernel
    assert moved >= 100 * e_kernel, "the edit must act on the target row"
    denoise.drop_pool()


@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_p2p_graph_eager_and_sampler_branch_on_tiny(precision, monkeypatch):
    from ief_amd import denoise
    from ief_amd.p2p.model import sd_utils
    from ief_amd.pipeline import StableDiffusionPipeline
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", precision=precision)
    denoise.drop_pool()
    for skip in (0, 1):
        x0, y, maps, _ = invert(pipe, 8888, skip)
        runs = P2PRuns(pipe, skip)
        graph = runs.sampler(y, maps)
        eager, _ = runs.loop(y, maps, use_graph=False)
        assert torch.equal(graph, eager), "the captured loop must equal eager stepping bit for bit"
        with monkeypatch.context() as m:
            m.setattr(sd_utils, "_fusable", lambda *a: False)
            assert torch.equal(graph, runs.sampler(y, maps)), "the sampler's eager branch must give the same bits"
        assert not torch.equal(graph[0], graph[1])
        assert not torch.equal(graph, runs.sampler(y, maps, guidance=(G_SRC, 7.5))), "the target row's scale must act"
        e = (graph[0] - x0[0].cpu()).abs().max().item() / x0.abs().max().item()
        print(f"tiny {precision}, skip {skip}: |row 0 - x0| / max |x0| = {e:.3e}")
    denoise.drop_pool()


def test_generic_controller_steps_through_diffusion_step_with_the_host_step_index(small_x3, monkeypatch):
    """a controller on the generic path (lowering goes by class name) steps eagerly through `P2P.diffusion_step`: the same kernel with
    a host step index, in front of `step_callback`; its source row reconstructs x0 too"""
    from ief_amd.p2p.model.attention_control import AttentionRefine

    class RefineOnTheGenericPath(AttentionRefine):
        pass

    pipe = small_x3
    x0, y, maps, _ = invert(pipe, 8888, 1)
    real, calls = hip.cfg_ddpm_step, []

    def spy(eps_u, eps_c, x, coef, g_rows, noise, step, out=None, x0_out=None):
        calls.append((int(step.item()), g_rows.tolist(), noise.shape[0], out is None))
        return real(eps_u, eps_c, x, coef, g_rows, noise, step, out=out, x0_out=x0_out)

    monkeypatch.setattr(hip, "cfg_ddpm_step", spy)
    runs = P2PRuns(pipe, 1)
    lat = runs.sampler(y, maps, cls=RefineOnTheGenericPath)
    assert pipe.unet._plan is None
    assert calls == [(i, [G_SRC, G_TAR], STEPS - 1, True) for i in range(STEPS - 1)]
    e = (lat[0] - x0[0].cpu()).abs().max().item() / x0.abs().max().item()
    print(f"eager sampler, generic controller, skip 1: |row 0 - x0| / max |x0| = {e:.3e}")
    assert torch.isfinite(lat).all() and not torch.equal(lat[0], lat[1])


WORDS, THRES = [["house"], ["fall"]], 0.9905          # tests/test_gpu_local_blend.py: the threshold at which `small`'s flat maps split


def test_lowered_local_blend_runs_after_the_ddpm_step(small_x3):
    from ief_amd import denoise
    pipe = small_x3
    x0, y, maps, _ = invert(pipe, 8888, 0)
    runs, plain = P2PRuns(pipe, 0, blend=(WORDS, THRES)), P2PRuns(pipe, 0)
    denoise.drop_pool()
    eager, _ = runs.loop(y, maps, use_graph=False)
    graph, loop = runs.loop(y, maps, use_graph=True)
    assert loop.plan.blend_w is not None
    assert torch.equal(graph, eager), "captured-graph replay must equal eager stepping bit for bit"
    assert torch.equal(graph, runs.sampler(y, maps))
    noblend, _ = plain.loop(y, maps, use_graph=True)
    assert torch.equal(graph[0], noblend[0]), "the blend leaves the source row alone"
    moved = ((graph[1] - noblend[1]).abs().max() / noblend[1].abs().max()).item()
    print(f"with a lowered LocalBlend: the blend moves the target row by {moved:.3e} of its size; source row unchanged")
    assert not torch.equal(graph[1], noblend[1]), "the blend must act on the target row"
    denoise.drop_pool()


def test_pooled_loop_repointed_at_other_maps_and_scales_and_edit_many(small_x3):
    from ief_amd import denoise
    from ief_amd.p2p.model.register import unregister_attention_control as unreg
    pipe = small_x3
    _, ya, mapsa, _ = invert(pipe, 8888, 1)
    _, yb, mapsb, _ = invert(pipe, 4242, 1)
    ga, gb = GUIDANCE, (2.0, 9.0)
    runs = P2PRuns(pipe, 1)
    denoise.drop_pool()
    fresh_b, _ = runs.loop(yb, mapsb, use_graph=True, guidance=gb)                 # never pooled: its own capture
    first, loop1 = runs.loop(ya, mapsa, use_graph=True, pooled=True, guidance=ga)
    second, loop2 = runs.loop(yb, mapsb, use_graph=True, pooled=True, guidance=gb)
    assert loop2 is loop1 and loop2.graph is not None, "equal signatures: the captured loop is taken from the pool, not rebuilt"
    assert not torch.equal(first, second)
    assert torch.equal(second, fresh_b), "a pooled loop re-pointed at the second image's maps and scales must give that image's fresh run"
    assert torch.equal(loop2.maps.cpu(), mapsb.cpu()) and loop2.g_rows.tolist() == list(gb)
    # another skip, or no maps, is another pool entry
    _, y0, maps0, _ = invert(pipe, 8888, 0)
    _, loop3 = P2PRuns(pipe, 0).loop(y0, maps0, use_graph=True, pooled=True)
    assert loop3 is not loop1 and loop3.skip == 0 and loop3.num_steps == STEPS
    with pytest.raises(ValueError):
        loop3.rebind(runs.context, ga, None, None, None, mapsa, 1)
    with pytest.raises(ValueError):
        loop3.rebind(runs.context, 7.5, None, None, None, None, 0)
    again, loop4 = runs.loop(ya, mapsa, use_graph=True, pooled=True, guidance=ga)
    assert loop4 is loop1 and torch.equal(again, first)
    denoise.drop_pool()

    # edit_many with two jobs == one call per job
    jobs = [(PROMPTS, runs.controller(), ya.clone(), None, None, (mapsa, 1, ga)), (PROMPTS, runs.controller(), yb.clone(), None, None, (mapsb, 1, gb))]
    many = runs.editor.edit_many(pipe, jobs, num_inference_steps=STEPS)
    for (img, _), (y, maps, g) in zip(many, ((ya, mapsa, ga), (yb, mapsb, gb))):
        c = runs.controller()
        one, _ = runs.editor.text2image_ldm_stable(pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=g, latent=y.clone(),
                                                   noise_maps=maps, skip=1)
        unreg(pipe, c)
        assert (img == one).all(), "edit_many must give what one call per job gives"
    with pytest.raises(ValueError):
        runs.editor.edit_many(pipe, [(PROMPTS, runs.controller(), ya.clone(), None, mapsa, (mapsa, 1, ga))], num_inference_steps=STEPS)
    unreg(pipe, None)
    denoise.drop_pool()


# ------------------------------------------------------------------------------------------------------------- the PIE driver
def test_pie_driver_ddpm_rows_per_launch_and_in_flight_match_per_image(tmp_path):
    """images in flight (`edit_many`, pooled loops, per-image seeds) against one image at a time, both at 4 rows per launch: the
    same pixels.  The rows per launch themselves are part of the numerics in f16x3 -- a batched forward differs from batch-1
    forwards by 1e-6 of eps (measured above), maps at 3 and 1 rows per launch by 2.3e-6 of their size, a grey level here and
    there -- as README states for the batched DDIM inversion."""
    script = os.path.join(PKG, "p2p", "test.py")
    base = ["--sd_version", "small", "--synthetic", "2", "--inversion_type", "ddpm", "--invert_batch", "4"]
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
