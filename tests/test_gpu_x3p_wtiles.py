"""The TILED order of the weight planes (`ief_x3_tile_weights`, `IefGemmX3pParams.w_tiled`, `planes.W_TILES`) on a real MI355X.

Only the global address a lane fetches a weight chunk from differs between a `w_tiled = 1` launch and a `w_tiled = 0` launch: the
same halves land in the same LDS bytes, so every comparison here is BITWISE (`torch.equal` on fp32 outputs and on both output
planes) between the two launches with the same operands, tile and splits.  The row-major path is pinned to fp64 by the other
planes tests (test_gpu_x3p*.py).  Shapes: the smallest at which the addressing can go wrong -- row tails, column tails that end
inside a piece and inside a pair, fewer K tiles than ring slots, uneven split-K ranges, a K-concatenated range that straddles K1,
both super-tile buffers and a wrapping weight ring of the halo kernel, the four phase matrices.
"""
import functools
from ctypes import byref

import pytest
import torch

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import denoise, hip, planes  # noqa: E402
from ief_amd.planes import Planes  # noqa: E402

DEV = torch.device("cuda:0")
EINVAL, ESHAPE, EALIGN = -1, -2, -3


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(autouse=True)
def _x3():
    with hip.f32_contraction("x3"):
        yield


def tiled_index(N, K):
    """the index-arithmetic restatement: element [pl][n][32 kt + kk] of row-major planes [2][N][K] -> its half index in the tiled order"""
    nk = K // 32
    pl = torch.arange(2).view(2, 1, 1)
    n = torch.arange(N).view(1, N, 1)
    k = torch.arange(K).view(1, 1, K)
    kt, kk = k // 32, k % 32
    return pl * (N * K) + ((((n >> 2) * nk + kt) * 4 + (n & 3)) * 32 + kk)


def tiled_ref(rowmajor):
    """CPU: planes [2, N, K] -> the tiled order, by scattering every half to its restated index"""
    _, N, K = rowmajor.shape
    out = torch.empty(2 * N * K, dtype=rowmajor.dtype)
    idx = tiled_index(N, K).reshape(-1)
    assert idx.unique().numel() == 2 * N * K, "the tiled order must be a permutation"
    out[idx] = rowmajor.reshape(-1)
    return out.view(2, N, K)


def on_and_off(monkeypatch, launch):
    """launch() with planes.W_TILES on, then off -> the two results as tuples of tensors; checks that the launches really were
    w_tiled = 1 and w_tiled = 0"""
    seen = []
    real = planes._weight_arg

    def spy(p, *a, **kw):
        r = real(p, *a, **kw)
        seen.append(int(p.w_tiled))
        return r
    monkeypatch.setattr(planes, "_weight_arg", spy)
    res = []
    for on in (True, False):
        monkeypatch.setattr(planes, "W_TILES", on)
        mark = len(seen)
        r = launch()
        assert seen[mark:] and all(v == (1 if on else 0) for v in seen[mark:]), (on, seen[mark:])
        r = r if isinstance(r, tuple) else (r,)
        res.append(tuple(t.t if isinstance(t, Planes) else t for t in r))
    monkeypatch.setattr(planes, "_weight_arg", real)
    return res


def assert_same_bits(res, what):
    a, b = res
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype
        assert torch.isfinite(x.float()).all(), f"{what}: NaN / inf in output {i} of the tiled launch"
        assert x.float().abs().max() > 0, f"{what}: output {i} is all zero"
        assert torch.equal(x, y), f"{what}: output {i} of the w_tiled launch differs from the row-major launch"


# ---------------------------------------------------------------------------------------------------------------- 1. the copy
@pytest.mark.parametrize("N,K", [(4, 32), (20, 64), (84, 96), (164, 320)])
def test_tile_weights_is_the_restated_permutation(N, K):
    lib = hip.load()
    src = f32(2, N, K, seed=N + K).half()
    d_src = src.to(DEV)
    d_out = torch.full((2, N, K), -3.0, dtype=torch.float16, device=DEV)
    assert d_out.data_ptr() % 256 == 0
    hip._check(lib.ief_x3_tile_weights(d_src.data_ptr(), d_out.data_ptr(), N, K, hip._stream()), "ief_x3_tile_weights")
    want = tiled_ref(src)
    got = d_out.cpu()
    assert torch.equal(got[0], want[0]), "hi plane"
    assert torch.equal(got[1], want[1]), "lo plane"
    # four consecutive rows x one K tile = 256 contiguous bytes: rows 0..3 of K tile 0 open the buffer
    assert torch.equal(got.reshape(-1)[:128].view(4, 32), src[0, :4, :32])


def test_tile_weights_refusals_launch_nothing():
    lib = hip.load()
    src = f32(2, 8, 64, seed=1).half().to(DEV)
    buf = torch.full((2 * 8 * 64 + 128,), -3.0, dtype=torch.float16, device=DEV)
    for args, code in (((src.data_ptr(), buf.data_ptr(), 6, 64), ESHAPE),            # N % 4
                       ((src.data_ptr(), buf.data_ptr(), 8, 48), ESHAPE),            # K % 32
                       ((src.data_ptr(), buf.data_ptr() + 16, 8, 64), EALIGN),       # output not on 256 bytes
                       ((src.data_ptr(), buf.data_ptr() + 128, 8, 64), EALIGN),
                       ((src.data_ptr() + 8, buf.data_ptr(), 8, 64), EALIGN),        # input not on 16 bytes
                       ((None, buf.data_ptr(), 8, 64), EINVAL),
                       ((src.data_ptr(), None, 8, 64), EINVAL)):
        rc = lib.ief_x3_tile_weights(*args, hip._stream())
        torch.cuda.synchronize()
        assert rc == code, (args[2:], rc, code)
        assert bool((buf == -3.0).all()), "a refused copy wrote its output"


def test_cached_tiles_of_a_weight_and_of_its_phase_form():
    w = f32(84, 96, seed=5, scale=0.1).to(DEV)
    rm = hip.x3_weight_planes(w, planes.W_SCALE)
    t = hip.x3_weight_tiles(w, planes.W_SCALE)
    assert t is hip.x3_weight_tiles(w, planes.W_SCALE) and planes.weight_tiles(w) is t, "cached per weight tensor"
    assert hip.x3_weight_planes(w, planes.W_SCALE) is rm and tuple(rm.shape) == (2, 84, 96), "the row-major planes stay what they were"
    assert torch.equal(t.cpu(), tiled_ref(rm.cpu()))
    w.add_(1.0)
    assert hip.x3_weight_tiles(w, planes.W_SCALE) is not t, "an in-place update of the weight re-makes the copy"
    # phase form [2, 4, Cout, 4 C]: every phase matrix of every plane is tiled on its own
    Cout, C = 80, 32
    wc = f32(Cout, 3, 3, C, seed=6, scale=0.1).to(DEV)
    ph = hip.x3_upsample_phase_planes(wc, planes.W_SCALE).cpu()
    pt = hip.x3_upsample_phase_tiles(wc, planes.W_SCALE)
    assert pt is hip.x3_upsample_phase_tiles(wc, planes.W_SCALE) and tuple(pt.shape) == (2, 4, Cout, 4 * C)
    pt = pt.cpu()
    for f in range(4):
        assert torch.equal(pt[:, f].contiguous(), tiled_ref(ph[:, f].contiguous())), f"phase {f}"


# ---------------------------------------------------------------------------------------------------------------- 2. linear
@functools.lru_cache(maxsize=None)
def _lin(M, N, K, seed=0):
    a, w = f32(M, K, seed=seed + 1), f32(N, K, seed=seed + 2, scale=K ** -0.5)
    bias, res = f32(N, seed=seed + 3, scale=0.1), f32(M, N, seed=seed + 4)
    return planes.split(a.to(DEV)), w.to(DEV), bias.to(DEV), res.to(DEV)


LINEAR = [(t, n) for t in (1, 2, 3, 4, 5, 7, 8) for n in (84, 164, 324)] + [(6, 128), (6, 192)]


@pytest.mark.parametrize("K", [96, 320])
@pytest.mark.parametrize("tile,N", LINEAR)
def test_linear_every_tile(tile, N, K, monkeypatch):
    ap, w, bias, res = _lin(130, N, K)
    r = on_and_off(monkeypatch, lambda: planes.gemm(ap, w, bias=bias, residual=res, out=True, out_planes=True, tile=tile, splits=1))
    assert_same_bits(r, f"linear t{tile} 130x{N}x{K}")


# ---------------------------------------------------------------------------------------------------------------- 3. GEGLU
@pytest.mark.parametrize("N", [96, 352])
@pytest.mark.parametrize("tile", [4, 8])
def test_geglu_rows_land_on_whole_blocks(tile, N, monkeypatch):
    ap, w, bias, _ = _lin(130, N, 64, seed=10)
    r = on_and_off(monkeypatch, lambda: planes.gemm(ap, w, bias=bias, geglu=True, out=True, out_planes=True, tile=tile))
    assert r[0][0].shape == (130, N // 2)
    assert_same_bits(r, f"geglu t{tile} N={N}")


# ---------------------------------------------------------------------------------------------------------------- 4. split-K
@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("tile,N", [(1, 164), (3, 84)])
def test_split_k_ranges_start_at_their_own_tile(tile, N, splits, monkeypatch):
    ap, w, bias, res = _lin(130, N, 320)
    r = on_and_off(monkeypatch, lambda: planes.gemm(ap, w, bias=bias, residual=res, out=True, out_planes=True, tile=tile, splits=splits))
    assert_same_bits(r, f"split-K t{tile} s{splits}")


# ---------------------------------------------------------------------------------------------------------------- 5. KCAT
@pytest.mark.parametrize("K1,K2,splits", [(64, 32, 1), (32, 96, 2)])
@pytest.mark.parametrize("tile,N", [(1, 164), (3, 84), (4, 164), (6, 128)])
def test_k_concatenated(tile, N, K1, K2, splits, monkeypatch):
    ap, w, bias, res = _lin(130, N, K1 + K2, seed=20)
    a1 = Planes(ap.t[..., :K1].contiguous())
    a2 = ap[:, K1:]                                    # a column slice: lda2 > K2
    r = on_and_off(monkeypatch, lambda: planes.gemm(a1, w, a2=a2, bias=bias, residual=res, out=True, out_planes=True, tile=tile,
                                                    splits=splits))
    assert_same_bits(r, f"kcat t{tile} {K1}+{K2} s{splits}")
    monkeypatch.setattr(planes, "W_TILES", True)
    plain = planes.gemm(ap, w, bias=bias, residual=res, out=True, tile=tile, splits=splits)
    assert torch.equal(plain, r[0][0]), "the K-concatenated launch must keep the bits of the plain launch over [A | A2]"


# ---------------------------------------------------------------------------------------------------------------- 6. implicit-GEMM conv
@functools.lru_cache(maxsize=None)
def _conv(B, H, W, C1, C2, N, CE1=0, CE2=0, seed=30):
    K = 9 * (C1 + C2) + CE1 + CE2
    x = planes.split(f32(B, H, W, C1, seed=seed + 1).to(DEV))
    x2 = planes.split(f32(B, H, W, C2, seed=seed + 2).to(DEV)) if C2 else None
    wf = f32(N, K, seed=seed + 3, scale=K ** -0.5)
    w = (wf if CE1 else wf.reshape(N, 3, 3, C1 + C2)).contiguous().to(DEV)
    bias = f32(N, seed=seed + 4, scale=0.1).to(DEV)
    extra = None
    if CE1:
        extra = (planes.split(f32(B, H, W, CE1, seed=seed + 5).to(DEV)), planes.split(f32(B, H, W, CE2, seed=seed + 6).to(DEV)) if CE2 else None)
    return x, x2, w, bias, extra


@pytest.mark.parametrize("form", ["s1", "s2", "extra"])
@pytest.mark.parametrize("tile", [1, 3])
def test_implicit_gemm_conv(tile, form, monkeypatch):
    ce = 32 if form == "extra" else 0
    x, x2, w, bias, extra = _conv(1, 8, 8, 32, 32, 84, ce, ce)
    r = on_and_off(monkeypatch, lambda: planes.conv3x3(x, w, bias, x2=x2, stride=2 if form == "s2" else 1, extra=extra, out=True,
                                                       out_planes=True, tile=tile, splits=1))
    assert tuple(r[0][0].shape) == ((1, 4, 4, 84) if form == "s2" else (1, 8, 8, 84))
    assert_same_bits(r, f"igemm conv t{tile} {form}")


# ---------------------------------------------------------------------------------------------------------------- 7. halo kernel
def _raw_halo(x, wp, tiled, bias, out, outp, N, splits, ws):
    """tile 11 through the C ABI (`planes.conv3x3` keeps the halo form to widths that are multiples of 80)"""
    B, H, W, C = x.shape
    p = hip.IefGemmX3pParams()
    p.A, p.planeA = x.t.data_ptr(), x.plane
    p.W, p.planeW, p.ldw, p.w_tiled = wp.data_ptr(), wp.stride(0), 9 * C, 1 if tiled else 0
    p.Out, p.ldo = out.data_ptr(), N
    p.OutP, p.planeO, p.ldp = outp.t.data_ptr(), outp.plane, N
    p.bias = bias.data_ptr()
    p.M, p.N, p.K = B * H * W, N, 9 * C
    p.conv, p.H, p.Wd, p.C1, p.Ho, p.Wo = 1, H, W, C, H, W
    p.stride, p.ups, p.batch_images = 1, 0, B
    p.out_scale, p.inv_scale, p.zeros = 1.0, 1.0 / (planes.ACT_SCALE * planes.W_SCALE), hip._zeros(DEV)
    p.tile, p.splits = 11, splits
    if splits > 1:
        p.ws = ws.data_ptr()
    return p


@pytest.mark.parametrize("splits", [1, 2])
def test_halo_plain_two_channel_blocks_column_tail(splits):
    lib = hip.load()
    B, H, W, C, N = 1, 16, 16, 64, 84
    x, _, w, bias, _ = _conv(B, H, W, C, 0, N, seed=40)
    rm, tl = planes.weight_planes(w), planes.weight_tiles(w)
    res = []
    for tiled in (True, False):
        out = torch.full((B, H, W, N), float("nan"), dtype=torch.float32, device=DEV)
        outp = Planes.empty(B, H, W, N, device=DEV)
        outp.t.fill_(float("nan"))
        ws = torch.full((splits * B * H * W * N,), float("nan"), dtype=torch.float32, device=DEV)
        p = _raw_halo(x, tl if tiled else rm, tiled, bias, out, outp, N, splits, ws)
        hip._check(lib.ief_gemm_x3p(byref(p), hip._stream()), "ief_gemm_x3p (tile 11)")
        res.append((out, outp.t))
    assert_same_bits(res, f"halo t11 s{splits}")


def test_halo_refuses_tiled_planes_it_cannot_address():
    """w_tiled needs planeW == N K and a 256-byte aligned W: IEF_ESHAPE / IEF_EALIGN, nothing launched"""
    lib = hip.load()
    B, H, W, C, N = 1, 16, 16, 64, 84
    x, _, w, bias, _ = _conv(B, H, W, C, 0, N, seed=40)
    tl = planes.weight_tiles(w)
    for change, code in ((lambda p: setattr(p, "planeW", p.planeW + 8), ESHAPE), (lambda p: setattr(p, "W", p.W + 16), EALIGN)):
        out = torch.full((B, H, W, N), 7.0, dtype=torch.float32, device=DEV)
        outp = Planes.empty(B, H, W, N, device=DEV)
        p = _raw_halo(x, tl, True, bias, out, outp, N, 1, None)
        change(p)
        rc = lib.ief_gemm_x3p(byref(p), hip._stream())
        torch.cuda.synchronize()
        assert rc == code, (rc, code)
        assert bool((out == 7.0).all()), "a refused launch wrote its output"


@pytest.mark.parametrize("tile", [12, 13])
def test_halo_nearest_2x_nine_taps_and_phase_form(tile, monkeypatch):
    x, _, w, bias, _ = _conv(1, 8, 8, 32, 0, 80, seed=50)
    r = on_and_off(monkeypatch, lambda: planes.conv3x3(x, w, bias, upsample=True, out=True, out_planes=True, tile=tile, splits=1))
    assert r[0][0].shape == (1, 16, 16, 80)
    assert_same_bits(r, f"halo t{tile}")


# ---------------------------------------------------------------------------------------------------------------- 8. as the model drives it
def test_plans_pick_the_tile_gemm_and_every_conv_form(monkeypatch):
    ap, w, bias, res = _lin(130, 160, 320, seed=60)
    assert_same_bits(on_and_off(monkeypatch, lambda: planes.gemm(ap, w, bias=bias, residual=res, out=True, out_planes=True)), "gemm")
    a1, a2 = Planes(ap.t[..., :256].contiguous()), ap[:, 256:]
    assert_same_bits(on_and_off(monkeypatch, lambda: planes.gemm(a1, w, a2=a2, bias=bias, out=True)), "gemm kcat")
    x, _, wc, cb, _ = _conv(1, 16, 16, 64, 0, 80, seed=61)
    assert_same_bits(on_and_off(monkeypatch, lambda: planes.conv3x3(x, wc, cb, out=True, out_planes=True)), "conv halo")
    assert_same_bits(on_and_off(monkeypatch, lambda: planes.conv3x3(x, wc, cb, stride=2, out=True)), "conv implicit GEMM")
    assert_same_bits(on_and_off(monkeypatch, lambda: planes.conv3x3(x, wc, cb, upsample=True, out=True)), "conv nearest-2x")
    assert_same_bits(on_and_off(monkeypatch, lambda: planes.conv3x3(x, wc, cb, upsample=True, out=True, tile=13)), "conv phase")
    x, x2, we, eb, extra = _conv(1, 8, 8, 32, 32, 80, 32, 32, seed=62)
    assert_same_bits(on_and_off(monkeypatch, lambda: planes.conv3x3(x, we, eb, x2=x2, extra=extra, out=True, out_planes=True)), "conv fused shortcut")


@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.p2p.model.sd_utils import _encode_prompts
    from ief_amd.pipeline import StableDiffusionPipeline
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")
    with torch.no_grad():
        u, c = _encode_prompts(pipe, ["a photo of a house on a mountain"])
    hw = pipe.cfg.sample_size
    x_T = torch.randn(1, 4, hw, hw, generator=torch.Generator().manual_seed(8888))
    return pipe, torch.cat([u, c]), x_T


def _one_step(small, use_graph):
    pipe, ctx, x_T = small
    pipe.scheduler.set_timesteps(1)
    hw = pipe.cfg.sample_size
    loop = denoise.FusedDenoiser(pipe, ctx, 1, (hw, hw), 7.5, use_graph=use_graph)
    try:
        return loop.run(x_T.to(DEV)).float().cpu()
    finally:
        loop.release()


def test_small_unet_cfg_step_same_latents(small_x3, monkeypatch):
    """one CFG step of the `small` UNet in f16x3, eager and from the captured graph, tiled and row-major: the same latents bit for bit"""
    monkeypatch.setattr(denoise, "REUSE_GRAPHS", False)          # every loop captures its own graph under its own setting
    lat = {}
    for on in (True, False):
        monkeypatch.setattr(planes, "W_TILES", on)
        for use_graph in (False, True):
            lat[on, use_graph] = _one_step(small_x3, use_graph)
    assert torch.isfinite(lat[True, False]).all() and not torch.equal(lat[True, False], small_x3[2]), "the step did not run"
    assert torch.equal(lat[True, True], lat[True, False]), "tiled: graph replay differs from eager"
    assert torch.equal(lat[False, True], lat[False, False]), "row-major: graph replay differs from eager"
    assert torch.equal(lat[True, False], lat[False, False]), "tiled and row-major latents differ"
