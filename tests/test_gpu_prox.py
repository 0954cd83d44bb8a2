"""Negative-prompt inversion with proximal guidance on a real MI355X: the per-row quantile threshold (`ief_prox_threshold_f32`), the
proximal CFG + DDIM step (`ief_cfg_ddim_step_prox_f32`), the captured loop that runs both in place of the plain step, and the CLIs.

The rule is restated in `tests/prox_ref.py`.  Stated checks (every test prints what it measured):
    threshold     bit-equal to the fp32 restatement (sort of |eps_c - eps_u|, the two order statistics, one un-fused interpolation)
    step          prox_on = 0 and eta = 0, and row 0 always: bit-equal to `hip.cfg_ddim_step` on the same inputs
                  every threshold decision: x_out equals the plain step's exactly where |d| > lambda_b (l0, eta = 0) and nowhere else
                  every mask decision: x0_out equals the eta = 0 launch's exactly where the dilated mask is set and nowhere else
                  max |x - ref64| / max |ref64| at most 4 x the same figure of the fp32 CPU restatement (the project's yardstick
                  rule); the fp64 restatement is fed the device's own lambda_b
                  eta = 1: unedited elements land on z0 within 2^-23 (|z0| + |x0|), the bound of two correctly rounded operations
    loop          captured graph == eager stepping == UNet forward + `hip.prox_threshold` + the step launched by the test, bit for
                  bit; a pooled loop re-pointed at another plan == that plan's eager run; the source row == plain NPI's
Measured on an MI355X: every threshold bit-equal; the step's max |x - ref64| / max |ref64| 2.2e-7 .. 7.2e-7 on the device and the same
on a CPU restatement that rounds every operation on its own (the two agree bit for bit; the restatement takes its square roots in
double and rounds once, because a CPU whose torch takes the scalar fp32 root an ulp off gave 5.4e-8 .. 2.5e-7 and, on the
one-element shape, 3.3e-9 against 7.4e-8); eta = 1 within the bound; `small`, f16x3, 4 steps, guidance 7.5, l0, q 0.7, r 1: the target
row moves by 0.775 of its size (P2P) / 0.722 (MasaCtrl), the source row by 0.
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import denoise, hip  # noqa: E402
from ief_amd.control import ledits_rank  # noqa: E402
from _procs import call_main  # noqa: E402
import prox_ref  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "image-editing-framework_amd")
IEF_EINVAL, IEF_ESHAPE, IEF_EALIGN = -1, -2, -3          # csrc/ief_common.h
QS = (0.0, 0.5, 0.7, 0.999, 1.0)
A_FROM, A_TO, G = 0.55, 0.71, 7.5


def rank_of(q, n):
    return torch.tensor(list(ledits_rank(q, n)), dtype=torch.float32, device=DEV)


def check_threshold(eu, ec, what):
    """eu, ec fp32 CPU [B, n]: the launch against the restatement at every quantile, bit for bit, twice (the same bits from run to run)"""
    B, n = eu.shape
    absd = (ec - eu).abs()
    du, dc = eu.to(DEV), ec.to(DEV)
    for q in QS:
        want = prox_ref.quantile_f32(absd, q)
        out = torch.full((B,), float("nan"), device=DEV)
        assert hip.prox_threshold(du, dc, rank_of(q, n), out=out) is out
        again = hip.prox_threshold(du, dc, rank_of(q, n))
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want), f"{what}: B={B} n={n} q={q}: {out.cpu().tolist()} != {want.tolist()}"
        assert torch.equal(again, out)


# ------------------------------------------------------------------------------------------------------------- the threshold
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4 * 8 * 8, 4 * 7 * 9, 16384, 36864, 65536])
def test_threshold_bit_equal_to_the_restatement(B, n):
    g = torch.Generator().manual_seed(1000 * B + n)
    check_threshold(torch.randn(B, n, generator=g), torch.randn(B, n, generator=g), "unit Gaussian")


@pytest.mark.parametrize("n", [257, 16384, 36864])
def test_threshold_structured_rows(n):
    g = torch.Generator().manual_seed(n)
    r = lambda *s: torch.randn(*s, generator=g)
    eu = r(3, n)
    check_threshold(eu, eu + 0.375, "all-equal values")
    check_threshold(torch.zeros(2, n), torch.full((2, n), -2.5), "all-equal values, negative difference")
    ec = eu.clone()
    idx = torch.randperm(n, generator=g)[: n // 10]
    ec[:, idx] += r(3, idx.numel())
    check_threshold(eu, ec, "90 % exact zeros")
    # the bracketing order statistics are tied: differences from a set of eight values, every rank sits inside a run of equals
    ties = torch.randint(0, 8, (3, n), generator=g).float() * 0.25
    srt = torch.sort(ties, dim=1).values
    lo = ledits_rank(0.7, n)[0]
    assert (srt[:, lo] == srt[:, min(lo + 1, n - 1)]).all()
    check_threshold(torch.zeros(3, n), ties * torch.where(r(3, n) > 0, 1.0, -1.0), "tied order statistics")
    scale = torch.tensor([1.0, 1e4, 1e-4]).view(3, 1)
    check_threshold(r(3, n) * scale, r(3, n) * scale, "rows that differ in scale by 1e4")


def test_threshold_refusals_launch_nothing():
    lib = hip.load()
    eu, ec = torch.randn(2, 256, device=DEV), torch.randn(2, 256, device=DEV)
    rank, out = rank_of(0.7, 256), torch.full((2,), float("nan"), device=DEV)
    p = lambda t: t.data_ptr()
    good = dict(eps_u=p(eu), eps_c=p(ec), rank=p(rank), thres_out=p(out), B=2, row_elems=256)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ief_prox_threshold_f32(a["eps_u"], a["eps_c"], a["rank"], a["thres_out"], a["B"], a["row_elems"],
                                          torch.cuda.current_stream().cuda_stream)

    for name in ("eps_u", "eps_c", "rank", "thres_out"):
        assert call(**{name: None}) == IEF_EINVAL, name
        assert call(**{name: good[name] + 2}) == IEF_EALIGN, name
    for kw in (dict(B=0), dict(B=-1), dict(row_elems=0), dict(row_elems=-4), dict(row_elems=65537)):
        assert call(**kw) == IEF_ESHAPE, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call must not launch"
    with pytest.raises(ValueError):
        hip.prox_threshold(eu, ec[:, :128].contiguous(), rank)
    with pytest.raises(ValueError):
        hip.prox_threshold(eu, ec, torch.zeros(2, 2, device=DEV))
    with pytest.raises(ValueError):
        hip.prox_threshold(torch.zeros(1, 65537, device=DEV), torch.zeros(1, 65537, device=DEV), rank)
    with pytest.raises(TypeError):
        hip.prox_threshold(eu.double(), ec.double(), rank)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------------- the step
def coef_of(on, eta):
    return torch.tensor([A_FROM, A_TO, G, on, eta], dtype=torch.float32, device=DEV)


def step_inputs(Bp, C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(Bp, C, h, w), r(Bp, C, h, w), r(Bp, C, h, w), r(C, h, w)


def figures(dev, cpu32, ref64):
    scale = ref64.abs().max().item()
    return (dev.double().cpu() - ref64).abs().max().item() / scale, (cpu32.double() - ref64).abs().max().item() / scale


@pytest.mark.parametrize("mode", ["l0", "l1"])
@pytest.mark.parametrize("radius", [0, 1, 3])
@pytest.mark.parametrize("Bp", [1, 2, 3])
def test_step_against_the_restatement(mode, radius, Bp):
    for C, h, w in ((4, 8, 8), (4, 7, 9), (4, 64, 64), (1, 1, 1)):
        eu, ec, x, z0 = step_inputs(Bp, C, h, w, seed=100 * Bp + 10 * radius + h)
        du, dc, dx, dz = (t.to(DEV) for t in (eu, ec, x, z0))
        lam = hip.prox_threshold(du, dc, rank_of(0.7, C * h * w))
        assert torch.equal(lam.cpu(), prox_ref.thresholds(eu, ec, 0.7))
        prox = (lam, dz, mode, radius)
        plain0 = torch.empty_like(dx)
        plain = hip.cfg_ddim_step(du, dc, dx, coef_of(0.0, 0.0)[:3].contiguous(), x0_out=plain0)
        keep, m = prox_ref.decisions(eu, ec, lam.cpu(), radius)
        d32 = ec - eu
        outs = {}
        for on, eta in ((0.0, 0.0), (1.0, 0.0), (1.0, 0.7), (0.0, 0.7), (1.0, 1.0)):
            coef = coef_of(on, eta)
            x0 = torch.full_like(dx, float("nan"))
            out = hip.cfg_ddim_step(du, dc, dx, coef, out=torch.full_like(dx, float("nan")), x0_out=x0, prox=prox)
            xc = dx.clone()
            assert hip.cfg_ddim_step(du, dc, xc, coef, out=xc, prox=prox) is xc
            no_x0 = hip.cfg_ddim_step(du, dc, dx, coef, prox=prox)
            torch.cuda.synchronize()
            assert torch.equal(xc, out), "in place == out of place"
            assert torch.equal(no_x0, out), "x0_out is optional"
            assert torch.equal(out[0], plain[0]) and torch.equal(x0[0], plain0[0]), "row 0 is the plain step, always"
            outs[(on, eta)] = (out.cpu(), x0.cpu())
            ref64, ref64_0 = prox_ref.step(eu, ec, x, coef.cpu(), lam.cpu(), z0, mode, radius, torch.float64)
            cpu32, cpu32_0 = prox_ref.step(eu, ec, x, coef.cpu(), lam.cpu(), z0, mode, radius, torch.float32)
            fd, fc = figures(out, cpu32, ref64)
            fd0, fc0 = figures(x0, cpu32_0, ref64_0)
            print(f"{mode} r={radius} Bp={Bp} ({C},{h},{w}) prox_on={on} eta={eta}: max |x - ref64| / max |ref64| device {fd:.3e}, fp32 "
                  f"CPU {fc:.3e}; x0: device {fd0:.3e}, fp32 CPU {fc0:.3e} (bound: 4 x the CPU figure)")
            assert fd <= 4 * fc and fd0 <= 4 * fc0
        off, off0 = outs[(0.0, 0.0)]
        assert torch.equal(off, plain.cpu()) and torch.equal(off0, plain0.cpu()), "prox_on = 0, eta = 0: the plain step bit for bit"
        assert torch.equal(outs[(0.0, 0.7)][0], plain.cpu()), "without thresholding the mask is 1 everywhere: nothing is pulled"
        if Bp == 1:
            continue
        # every threshold decision, through where x_out is the plain step's
        thr, thr0 = outs[(1.0, 0.0)]
        same = thr[1:] == plain.cpu()[1:]
        if mode == "l0":
            assert torch.equal(same, keep[1:] | (d32[1:] == 0)), "l0: d is kept exactly where |d| > lambda_b"
        else:
            assert not same[d32[1:] != 0].any(), "l1: every nonzero difference is shrunk or dropped"
            l0 = hip.cfg_ddim_step(du, dc, dx, coef_of(1.0, 0.0), prox=(lam, dz, "l0", radius)).cpu()
            assert torch.equal(thr[1:] == l0[1:], ~keep[1:]), "l1 and l0 agree exactly where the difference is dropped"
        # every mask decision, through where x0 is the un-pulled one's
        for eta in (0.7, 1.0):
            pulled0 = outs[(1.0, eta)][1]
            assert torch.equal(pulled0[1:] == thr0[1:], m[1:] | (thr0[1:] == z0[None])), f"eta={eta}: x0 is pulled exactly outside the dilated mask"
        one0 = outs[(1.0, 1.0)][1]
        offm = ~m[1:]
        bound = 2.0 ** -23 * (z0.abs()[None] + thr0[1:].abs())
        worst = ((one0[1:] - z0[None]).abs() / bound)[offm].max().item() if offm.any() else 0.0
        print(f"{mode} r={radius} Bp={Bp} ({C},{h},{w}) eta=1: unedited x0 vs z0, worst |x0 - z0| / (2^-23 (|z0| + |x0|)) = {worst:.3f} (bound 1)")
        assert worst <= 1.0


@pytest.mark.parametrize("radius", [0, 1, 3])
def test_step_hand_made_corners_and_edge(radius):
    """edited elements only in the four corners of one channel and along one edge of another: the zero padding and the row / channel
    boundaries of the stencil.  The expected mask is written out with slices, not with the restatement's pooling"""
    Bp, C, h, w = 3, 4, 7, 9
    g = torch.Generator().manual_seed(77)
    eu = torch.randn(Bp, C, h, w, generator=g)
    d = 0.01 * torch.randn(Bp, C, h, w, generator=g)
    edited = [(1, 0, 0, 0), (1, 0, 0, w - 1), (1, 0, h - 1, 0), (1, 0, h - 1, w - 1)] + [(1, 2, h - 1, xx) for xx in range(w)] + \
             [(0, 1, 3, 4)]                                     # and one on the source row, which must change nothing
    for b, c, y, xx in edited:
        d[b, c, y, xx] = 10.0 if (y + xx) % 2 == 0 else -10.0
    ec = eu + d
    assert ((ec - eu).abs() > 1.0).sum() == len(edited)
    x, z0 = torch.randn(Bp, C, h, w, generator=g), torch.randn(C, h, w, generator=g)
    want = torch.zeros(Bp, C, h, w, dtype=torch.bool)
    for b, c, y, xx in edited:
        want[b, c, max(0, y - radius): y + radius + 1, max(0, xx - radius): xx + radius + 1] = True
    assert not want[2].any() and not want[1, 1].any() and not want[1, 3].any(), "dilation must not cross a channel or a batch row"
    assert torch.equal(prox_ref.decisions(eu, ec, torch.ones(Bp), radius)[1], want)
    du, dc, dx, dz = (t.to(DEV) for t in (eu, ec, x, z0))
    lam = torch.ones(Bp, device=DEV)                              # a hand-made threshold between 0.01 and 10
    for mode in ("l0", "l1"):
        thr0, one0 = torch.empty_like(dx), torch.empty_like(dx)
        hip.cfg_ddim_step(du, dc, dx, coef_of(1.0, 0.0), x0_out=thr0, prox=(lam, dz, mode, radius))
        out = hip.cfg_ddim_step(du, dc, dx, coef_of(1.0, 1.0), x0_out=one0, prox=(lam, dz, mode, radius))
        plain = hip.cfg_ddim_step(du, dc, dx, coef_of(0.0, 0.0)[:3].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(out[0], plain[0]), "the source row is never thresholded or pulled"
        got = (one0 == thr0).cpu()
        assert torch.equal(got[1:], want[1:]), f"{mode} r={radius}: mask\n{got[1, 0].int()}\n{got[1, 2].int()}\n{got[1, 1].int()}"
        ref64, _ = prox_ref.step(eu, ec, x, coef_of(1.0, 1.0).cpu(), lam.cpu(), z0, mode, radius, torch.float64)
        cpu32, _ = prox_ref.step(eu, ec, x, coef_of(1.0, 1.0).cpu(), lam.cpu(), z0, mode, radius, torch.float32)
        fd, fc = figures(out, cpu32, ref64)
        print(f"hand-made {mode} r={radius}: {int(want[1:].sum())} mask elements; max |x - ref64| / max |ref64| device {fd:.3e}, fp32 CPU {fc:.3e}")
        assert fd <= 4 * fc


def test_step_refusals_launch_nothing():
    lib = hip.load()
    eu, ec, x, z0 = (t.to(DEV) for t in step_inputs(2, 4, 8, 8, 3))
    lam, coef = torch.ones(2, device=DEV), coef_of(1.0, 1.0)
    out, x0 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    p = lambda t: t.data_ptr()
    good = dict(eps_u=p(eu), eps_c=p(ec), x=p(x), x_out=p(out), x0_out=p(x0), coef=p(coef), thres=p(lam), z0=p(z0), n=x.numel(),
                row_elems=256, h=8, w=8, mode=0, radius=1)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ief_cfg_ddim_step_prox_f32(a["eps_u"], a["eps_c"], a["x"], a["x_out"], a["x0_out"], a["coef"], a["thres"], a["z0"],
                                              a["n"], a["row_elems"], a["h"], a["w"], a["mode"], a["radius"],
                                              torch.cuda.current_stream().cuda_stream)

    for name in ("eps_u", "eps_c", "x", "x_out", "coef", "thres", "z0"):
        assert call(**{name: None}) == IEF_EINVAL, name
    for name in ("eps_u", "eps_c", "x", "x_out", "x0_out", "coef", "thres", "z0"):
        assert call(**{name: good[name] + 2}) == IEF_EALIGN, name
    for kw in (dict(n=0), dict(n=-512), dict(row_elems=0), dict(row_elems=200), dict(row_elems=131072, n=131072), dict(h=0),
               dict(w=-1), dict(h=7), dict(mode=2), dict(mode=-1), dict(radius=4), dict(radius=-1)):
        assert call(**kw) == IEF_ESHAPE, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(x0).all(), "a refused call must not launch"
    ok = (lam, z0, "l0", 1)
    for bad in ((lam[:1], z0, "l0", 1), (lam, z0[:, :4].contiguous(), "l0", 1), (lam, z0, "l2", 1), (lam, z0, "l0", 4), (lam, z0, "l0", 1.0)):
        with pytest.raises(ValueError):
            hip.cfg_ddim_step(eu, ec, x, coef, prox=bad)
    with pytest.raises(ValueError):
        hip.cfg_ddim_step(eu, ec, x, coef[:3].contiguous(), prox=ok)
    with pytest.raises(ValueError):
        hip.cfg_ddim_step(None, ec, x, coef, prox=ok)
    with pytest.raises(ValueError):
        hip.cfg_ddim_step(eu, ec, x, coef, prox=ok, rect=(x, torch.zeros(1, dtype=torch.int32, device=DEV)))
    assert call() == 0 and call(x0_out=None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------------- the loop
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]
STEPS, GUIDANCE, Q, RADIUS = 4, 7.5, 0.7, 1


@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.pipeline import StableDiffusionPipeline
    return StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")


@pytest.fixture(scope="module")
def inversion(small_x3):
    """one image's NPI inversion, computed once and left unchanged: (z0 [C,h,w], x_T, the NPI context [4,77,C])"""
    from ief_amd.p2p.inversion.npi import NPI
    from ief_amd.p2p.model.sd_utils import _encode_prompts, npi_context
    pipe = small_x3
    s = pipe.cfg.sample_size
    z = torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(8888)).to(DEV)
    pipe.scheduler.set_timesteps(STEPS)
    inv = NPI()
    latents, context = inv.ddim_inversion_loop(pipe, z, [PROMPTS[0]])
    neg = inv.negative_prompt_embeds(context)
    with torch.no_grad():
        _, cond = _encode_prompts(pipe, PROMPTS)
    unc = npi_context(neg, cond)
    assert torch.equal(unc[0], cond[0]) and torch.equal(unc[1], cond[0]), "every unconditional row is the source embedding"
    return inv.source_latent(latents), latents[-1].clone(), torch.cat([unc, cond]), neg


def plan_of(pipe, q=Q, eta=1.0, late=1):
    """eta switches on after step `late`"""
    pipe.scheduler.set_timesteps(STEPS)
    ts = pipe.scheduler.timesteps.tolist()
    plan = denoise.ProxGuidance.from_schedule(ts, "l0", q, RADIUS, None, eta, recon_t=ts[late])
    assert plan.eta == [0.0] * (late + 1) + [eta] * (STEPS - late - 1) and plan.prox_on == [1.0] * STEPS
    return plan


def run_loop(pipe, inversion, plan, how, monkeypatch=None):
    """one Prompt-to-Prompt edit on the NPI context -> (latents [2,C,h,w] on the CPU, the loop).  how: "graph" / "eager" (a fresh
    loop), "pooled" (`denoise.acquire`), "hand": a loop WITHOUT a plan whose plain step the test replaces by its own launches of
    `hip.prox_threshold` and the proximal step on the loop's eps"""
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.register import register_attention_control, unregister_attention_control as unreg
    z0, x_T, context, _ = inversion
    hw = (pipe.cfg.sample_size,) * 2
    c = AttentionRefine(PROMPTS, pipe.tokenizer, STEPS, 0.8, 0.4, device=DEV)
    register_attention_control(pipe, c, fused=True)
    pipe.scheduler.set_timesteps(STEPS)
    kw = {} if plan is None or how == "hand" else dict(prox=plan, source_latent=z0)
    if how == "pooled":
        loop = denoise.acquire(pipe, context, 2, hw, GUIDANCE, use_graph=True, **kw)
    else:
        loop = denoise.FusedDenoiser(pipe, context, 2, hw, GUIDANCE, use_graph=how == "graph", **kw)
    if how == "hand":
        real, rank, calls = hip.cfg_ddim_step, plan.rank(z0.numel()).to(DEV), []

        def by_hand(eps_u, eps_c, x, coef, out=None, **rest):
            assert all(v is None for v in rest.values()) and coef.numel() == 4
            i = len(calls)
            coef5 = torch.cat([coef[:3], torch.tensor([plan.prox_on[i], plan.eta[i]], device=DEV)])
            lam = hip.prox_threshold(eps_u, eps_c, rank)
            calls.append(lam.clone())
            return real(eps_u, eps_c, x, coef5, out=out, prox=(lam, z0.to(DEV), plan.mode, plan.radius))

        monkeypatch.setattr(hip, "cfg_ddim_step", by_hand)
    try:
        lat = loop.run(x_T.clone()).float().cpu()
    finally:
        if how == "hand":
            monkeypatch.setattr(hip, "cfg_ddim_step", real)
            assert len(calls) == STEPS
        loop.release()
        unreg(pipe, c)
    assert c.cur_step == STEPS
    return lat, loop


def test_loop_graph_eager_by_hand_pooled_and_source_row(small_x3, inversion, monkeypatch):
    pipe = small_x3
    denoise.drop_pool()
    plan = plan_of(pipe)
    graph, gl = run_loop(pipe, inversion, plan, "graph")
    assert gl.coef_table.shape == (STEPS, 5) and gl.coef_table[:, 3].tolist() == plan.prox_on and gl.coef_table[:, 4].tolist() == plan.eta
    eager, _ = run_loop(pipe, inversion, plan, "eager")
    hand, _ = run_loop(pipe, inversion, plan, "hand", monkeypatch)
    assert torch.equal(graph, eager), "the captured graph must equal eager stepping bit for bit"
    assert torch.equal(graph, hand), "both must equal UNet forward + hip.prox_threshold + the proximal step launched by hand"
    npi, nl = run_loop(pipe, inversion, None, "graph")
    assert nl.coef_table.shape == (STEPS, 4) and nl.prox is None
    assert torch.equal(graph[0], npi[0]), "the source row is plain NPI's bit for bit"
    moved = ((graph[1] - npi[1]).abs().max() / npi[1].abs().max()).item()
    z0 = inversion[0].cpu()
    print(f"small f16x3, {STEPS} steps, guidance {GUIDANCE}, l0 q={Q} r={RADIUS}: proximal guidance moves the target row by {moved:.3e} of "
          f"its size; max |target - z0|: {(graph[1] - z0).abs().max():.3e} with, {(npi[1] - z0).abs().max():.3e} without; source row vs "
          f"z0: {(graph[0] - z0).abs().max():.3e}")
    assert moved > 0, "the target row moves relative to plain NPI"

    # a pooled loop re-pointed at another quantile / eta table == that plan's eager run; mode and radius select the pool entry
    denoise.drop_pool()
    other = plan_of(pipe, q=0.4, eta=0.5, late=0)
    want_other, _ = run_loop(pipe, inversion, other, "eager")
    first, l1 = run_loop(pipe, inversion, plan, "pooled")
    second, l2 = run_loop(pipe, inversion, other, "pooled")
    assert l2 is l1 and l2.graph is not None, "equal mode and radius: the captured loop is taken from the pool, not rebuilt"
    assert torch.equal(first, graph) and torch.equal(second, want_other) and not torch.equal(first, second)
    assert l2.coef_table[:, 4].tolist() == other.eta and l2.prox_rank.tolist() == other.rank(z0.numel()).tolist()
    _, l3 = run_loop(pipe, inversion, None, "pooled")
    assert l3 is not l1, "a loop without proximal guidance is another pool entry"
    with pytest.raises(ValueError):
        l3.rebind(inversion[2], GUIDANCE, None, prox=plan, source_latent=inversion[0])
    with pytest.raises(ValueError, match="prox together with source_trajectory"):
        denoise.FusedDenoiser(pipe, inversion[2], 2, (pipe.cfg.sample_size,) * 2, GUIDANCE, prox=plan, source_latent=inversion[0],
                              source_trajectory=torch.zeros(STEPS, *inversion[0].shape))
    denoise.drop_pool()


def test_samplers_take_the_npi_context_and_the_plan(small_x3, inversion):
    from ief_amd.masactrl.model.attention_control import MutualSelfAttentionControl
    from ief_amd.masactrl.model.register import regiter_attention_editor_diffusers, unregister_attention_control as unreg_m
    from ief_amd.masactrl.model.sd_utils import MasaCtrl
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.register import unregister_attention_control as unreg
    from ief_amd.p2p.model.sd_utils import P2P
    pipe = small_x3
    z0, x_T, _, neg = inversion
    plan = plan_of(pipe)
    denoise.drop_pool()
    want, _ = run_loop(pipe, inversion, plan, "eager")
    c = AttentionRefine(PROMPTS, pipe.tokenizer, STEPS, 0.8, 0.4, device=DEV)
    lat, _ = P2P(pipe, STEPS).text2image_ldm_stable(pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=GUIDANCE,
                                                     latent=x_T.clone(), return_latents=True, negative_prompt_embeds=neg, prox=plan,
                                                     source_latent=z0)
    unreg(pipe, c)
    assert torch.equal(lat.float().cpu(), want), "P2P.text2image_ldm_stable runs the loop of the test"
    with pytest.raises(ValueError, match="prox without negative_prompt_embeds"):
        P2P(pipe, STEPS).text2image_ldm_stable(pipe, PROMPTS, None, num_inference_steps=STEPS, latent=x_T.clone(), prox=plan, source_latent=z0)
    size = pipe.cfg.sample_size * 8
    outs = []
    for p in (plan, None):
        m = MutualSelfAttentionControl(1, 2, layer_idx=list(range(2, 11)), total_steps=STEPS)
        regiter_attention_editor_diffusers(pipe, m)
        try:
            lat, _ = MasaCtrl(pipe, STEPS)(prompt=PROMPTS, latents=torch.cat([x_T, x_T]), guidance_scale=GUIDANCE, num_inference_steps=STEPS,
                                           height=size, width=size, return_latents=True, negative_prompt_embeds=neg, prox=p,
                                           source_latent=None if p is None else z0)
        finally:
            unreg_m(pipe, m)
        outs.append(lat.float().cpu())
    assert torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][1], outs[1][1])
    print(f"MasaCtrl small f16x3: proximal guidance moves the target row by "
          f"{((outs[0][1] - outs[1][1]).abs().max() / outs[1][1].abs().max()).item():.3e} of its size, the source row by 0")
    denoise.drop_pool()


# ------------------------------------------------------------------------------------------------------------- the CLIs
def _jpg(path):
    rng = np.random.RandomState(0)
    Image.fromarray(np.kron(rng.randint(0, 255, (8, 8, 3)), np.ones((16, 16, 1))).astype(np.uint8)).save(path)


@pytest.mark.parametrize("folder", ["p2p", "masactrl"])
def test_clis_npi_with_proximal_guidance(tmp_path, folder):
    _jpg(tmp_path / "test.jpg")
    flags = ["--sd_version", "tiny", "--inversion_type", "npi"] + (["--prox", "l0"] if folder == "p2p" else [])
    call_main(os.path.join(PKG, folder, "edit_real.py"), flags + ["--source_image", str(tmp_path / "test.jpg")], tmp_path)
    pngs = {n: np.array(Image.open(tmp_path / "exp" / n)).astype(int) for n in ("source.png", "inversion.png", "edit.png")}
    assert pngs["source.png"].shape == pngs["inversion.png"].shape == pngs["edit.png"].shape
    assert np.abs(pngs["inversion.png"] - pngs["edit.png"]).max() > 0
    out = tmp_path / "pie"
    done = call_main(os.path.join(PKG, folder, "test.py"), flags + ["--synthetic", "2", "--exp_path", str(out)], tmp_path / "cwd")
    assert done.last_json()["images"] == 2
    dirs = sorted(x for x in os.listdir(out) if x.startswith("syn_"))
    assert len(dirs) == 2 and all(os.path.exists(out / d / "edit.png") for d in dirs)


def test_pie_driver_npi_batched_in_flight_matches_per_image(tmp_path):
    """plain NPI is only a context: --invert_batch / --in_flight change the schedule, not the pixels; with --prox the batched
    inversion feeds one edit at a time"""
    script = os.path.join(PKG, "p2p", "test.py")
    base = ["--sd_version", "tiny", "--synthetic", "2", "--inversion_type", "npi"]
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    one = call_main(script, base + ["--exp_path", str(a)], tmp_path / "cwd_a")
    many = call_main(script, base + ["--invert_batch", "2", "--in_flight", "2", "--exp_path", str(b)], tmp_path / "cwd_b")
    prox = call_main(script, base + ["--prox", "l0", "--invert_batch", "2", "--exp_path", str(c)], tmp_path / "cwd_c")
    assert one.last_json()["images"] == many.last_json()["images"] == prox.last_json()["images"] == 2
    dirs = sorted(x for x in os.listdir(a) if x.startswith("syn_"))
    assert len(dirs) == 2 and sorted(x for x in os.listdir(b) if x.startswith("syn_")) == dirs
    for d in dirs:
        for name in ("inversion.png", "edit.png"):
            pa, pb = np.array(Image.open(a / d / name)).astype(int), np.array(Image.open(b / d / name)).astype(int)
            assert pa.shape == pb.shape and np.abs(pa - pb).max() == 0, (d, name, np.abs(pa - pb).max())
        pa, pc = np.array(Image.open(a / d / "inversion.png")).astype(int), np.array(Image.open(c / d / "inversion.png")).astype(int)
        assert np.abs(pa - pc).max() == 0, "proximal guidance leaves the source row alone"
        assert os.path.exists(c / d / "edit.png")
