"""Upsample2D of the f16x3 mode in PHASE form (`planes.conv3x3(..., upsample=True, tile=13)`, csrc/conv_halo_x3p.hip) on a real MI355X.

Nearest-2x followed by a 3x3 / pad 1 convolution makes output pixel (2y + py, 2x + px) a 2x2 convolution of the low-resolution
image whose four weights are sums of the nine (`ief_x3_upsample_phase_weights`); the kernel runs the four phases as one launch.
The reference computes the layer in fp32 as `conv(interpolate(x, 2, "nearest"))` (`/root/reference/pnp/model/register.py:139-175`
calls the diffusers Upsample2D).

Stated tolerances (every test prints what it measured):
    phase weight planes        == ief_x3_split_weights of the fp32 phase weights summed in increasing (ky, kx) order, bit for bit
    kernel vs fp64 on the host <= 4e-6 of max |reference|  (the bound of tests/test_gpu_x3p.py, unchanged)
    planes out                 == split of the stored fp32 value, bit for bit
    vs today's nine-tap form   <= 2 x 4e-6 (both sit within 4e-6 of fp64)
"""
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ief_amd import hip, planes  # noqa: E402
from ief_amd.planes import Planes  # noqa: E402

XTOL = 4e-6
PHASE = 13
IEF_ESHAPE = -2         # include/ief_hip.h


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max()).item()


def ref_ups_conv(x, w, bias):
    """fp64: conv2d(interpolate(x, 2, "nearest"), w, b, padding=1) over NHWC x and [Cout, 3, 3, C] w"""
    xin = F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2.0, mode="nearest")
    y = F.conv2d(xin, w.permute(0, 3, 1, 2).double(), None if bias is None else bias.double(), padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(autouse=True)
def _x3():
    with hip.f32_contraction("x3"):
        yield


def _case(B, Hi, Wi, C, Cout, seed=0):
    x = f32(B, Hi, Wi, C, seed=seed + 1)
    w = f32(Cout, 3, 3, C, seed=seed + 2, scale=(9 * C) ** -0.5)
    bias = f32(Cout, seed=seed + 3, scale=0.1)
    return x, w, bias


def test_phase_weights_are_the_fp32_sums_split():
    C, Cout = 32, 16
    w = f32(Cout, 3, 3, C, seed=2, scale=(9 * C) ** -0.5).cuda()
    fold = {0: ([0], [1, 2]), 1: ([0, 1], [2])}           # phase -> original taps behind its two low-res taps
    ph = torch.empty(4, Cout, 4, C, dtype=torch.float32, device="cuda")
    for py in range(2):
        for px in range(2):
            for sy in range(2):
                for sx in range(2):
                    acc = None
                    for ky in fold[py][sy]:                # increasing (ky, kx), plain fp32 adds
                        for kx in fold[px][sx]:
                            acc = w[:, ky, kx, :].clone() if acc is None else acc + w[:, ky, kx, :]
                    ph[2 * py + px, :, 2 * sy + sx, :] = acc
    want = torch.empty(2, 4, Cout, 4 * C, dtype=torch.float16, device="cuda")
    lib = hip.load()
    hip._check(lib.ief_x3_split_weights(ph.data_ptr(), want.data_ptr(), ph.numel(), float(planes.W_SCALE), hip._stream()), "split")
    got = hip.x3_upsample_phase_planes(w, planes.W_SCALE)
    assert tuple(got.shape) == (2, 4, Cout, 4 * C)
    assert torch.equal(got, want), "phase planes differ from the split of the fp32-summed taps"
    again = torch.empty_like(got)
    hip._check(lib.ief_x3_upsample_phase_weights(w.data_ptr(), again.data_ptr(), Cout, C, float(planes.W_SCALE), hip._stream()), "phase")
    assert torch.equal(again, got), "two calls give different bits"
    assert hip.x3_upsample_phase_planes(w, planes.W_SCALE) is got, "the planes are cached per weight tensor"


@pytest.mark.parametrize("B,Hi,Wi,C,Cout,splits", [
    (3, 8, 8, 32, 80, 1),       # several images inside one 256-pixel tile, a partial tile, one channel block
    (2, 5, 6, 96, 160, 1),      # odd sizes, an odd block count, two column tiles
    (1, 16, 16, 64, 80, 2),     # split-K
    (1, 16, 16, 96, 80, 3),     # split-K, uneven
    (1, 4, 64, 32, 80, 1),      # the widest row
    (2, 20, 16, 64, 80, 1),     # tile edges inside an image
])
def test_phase_kernel_against_fp64(B, Hi, Wi, C, Cout, splits):
    x, w, bias = _case(B, Hi, Wi, C, Cout)
    out = planes.conv3x3(planes.split(x.cuda()), w.cuda(), bias.cuda(), upsample=True, tile=PHASE, splits=splits)
    assert tuple(out.shape) == (B, 2 * Hi, 2 * Wi, Cout)
    e = rel_err(out, ref_ups_conv(x, w, bias))
    print(f"upsample phases {B}x{Hi}x{Wi} {C}->{Cout} s{splits}: {e:.2e} vs fp64")
    assert e < XTOL


def test_phase_kernel_channel_concat():
    B, Hi, Wi, C1, C2, Cout = 2, 8, 8, 32, 32, 80
    x, w, bias = _case(B, Hi, Wi, C1 + C2, Cout, seed=10)
    x1, x2 = x[..., :C1].contiguous(), x[..., C1:].contiguous()
    out = planes.conv3x3(planes.split(x1.cuda()), w.cuda(), bias.cuda(), x2=planes.split(x2.cuda()), upsample=True, tile=PHASE)
    e = rel_err(out, ref_ups_conv(x, w, bias))
    print(f"upsample phases concat {C1}+{C2}: {e:.2e} vs fp64")
    assert e < XTOL


@pytest.mark.parametrize("splits", [1, 2])
def test_phase_kernel_outputs_agree_at_the_output_pixel(splits):
    """fp32 and planes out are the same values; residual and a per-image rowvec land on the OUTPUT pixel (a wrong row remap
    moves them)"""
    B, Hi, Wi, C, Cout = 2, 6, 8, 64, 80
    x, w, bias = _case(B, Hi, Wi, C, Cout, seed=20)
    rv, res = f32(B, Cout, seed=24), f32(B, 2 * Hi, 2 * Wi, Cout, seed=25)
    out, op = planes.conv3x3(planes.split(x.cuda()), w.cuda(), bias.cuda(), upsample=True, rowvec=rv.cuda(), residual=res.cuda(),
                             out=True, out_planes=True, tile=PHASE, splits=splits)
    assert isinstance(op, Planes)
    o = out.float().cpu()
    hi = o.half()
    lo = (o - hi.float()).half()
    assert torch.equal(op.hi.cpu(), hi), "hi plane differs from fp16(stored fp32)"
    assert torch.equal(op.lo.cpu(), lo), "lo plane differs from fp16(x - hi)"
    e = rel_err(out, ref_ups_conv(x, w, bias) + rv.double()[:, None, None, :] + res.double())
    print(f"upsample phases + rowvec + residual s{splits}: {e:.2e} vs fp64")
    assert e < XTOL


def test_phase_form_matches_the_nine_tap_form():
    B, Hi, Wi, C, Cout = 1, 16, 16, 64, 80
    x, w, bias = _case(B, Hi, Wi, C, Cout, seed=30)
    xp = planes.split(x.cuda())
    ph = planes.conv3x3(xp, w.cuda(), bias.cuda(), upsample=True, tile=PHASE)
    nine = planes.conv3x3(xp, w.cuda(), bias.cuda(), upsample=True, tile=12)
    ref = ref_ups_conv(x, w, bias)
    e, e_ph, e_9 = rel_err(ph, nine), rel_err(ph, ref), rel_err(nine, ref)
    print(f"phase vs nine-tap: {e:.2e}; vs fp64: phase {e_ph:.2e}, nine-tap {e_9:.2e}")
    assert e < 2 * XTOL and e_ph < XTOL and e_9 < XTOL


def _raw_params(x, w, wp, out, Hi, Wi, C, Cout):
    p = hip.IefGemmX3pParams()
    p.A, p.planeA = x.t.data_ptr(), x.plane
    p.W, p.planeW, p.ldw = wp.data_ptr(), wp.stride(0), 4 * C
    p.Out, p.ldo = out.data_ptr(), Cout
    B = x.shape[0]
    p.M, p.N, p.K = B * 4 * Hi * Wi, Cout, 4 * C
    p.conv, p.H, p.Wd, p.C1, p.Ho, p.Wo = 1, 2 * Hi, 2 * Wi, C, 2 * Hi, 2 * Wi
    p.stride, p.ups, p.batch_images = 1, 1, B
    p.out_scale, p.inv_scale, p.zeros = 1.0, 1.0 / (planes.ACT_SCALE * planes.W_SCALE), hip._zeros(out.device)
    p.tile, p.splits = PHASE, 1
    return p


def test_phase_tile_rejects_geometry_it_cannot_run():
    """a source row of 65 pixels, or a fused 1x1 source, returns IEF_ESHAPE and launches nothing (the output keeps its fill)"""
    lib = hip.load()
    C, Cout = 32, 80
    w = f32(Cout, 3, 3, C, seed=2, scale=(9 * C) ** -0.5).cuda()
    wp = hip.x3_upsample_phase_planes(w, planes.W_SCALE)
    for Hi, Wi, extra in ((2, 65, False), (4, 8, True)):
        x = planes.split(f32(1, Hi, Wi, C, seed=1).cuda())
        out = torch.full((1, 2 * Hi, 2 * Wi, Cout), 7.0, dtype=torch.float32, device="cuda")
        p = _raw_params(x, w, wp, out, Hi, Wi, C, Cout)
        e1 = None
        if extra:
            e1 = planes.split(f32(1, 2 * Hi, 2 * Wi, 32, seed=3).cuda())
            p.E1, p.planeE1, p.CE1 = e1.t.data_ptr(), e1.plane, 32
            p.K = 4 * C + 32
            p.ldw = p.K
        rc = lib.ief_gemm_x3p(byref(p), hip._stream())
        torch.cuda.synchronize()
        assert rc == IEF_ESHAPE, rc
        assert bool((out == 7.0).all()), "a rejected launch wrote to its output"
    with pytest.raises(ValueError):
        planes.conv3x3(planes.split(f32(1, 2, 65, C, seed=1).cuda()), w, upsample=True, tile=PHASE)
