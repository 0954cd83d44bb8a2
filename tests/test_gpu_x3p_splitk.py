"""Split-K on the planes kernels at the slab edges the plans run (`csrc/gemm_x3p.hip`, `csrc/conv_halo_x3p.hip`,
`x3p_reduce_kernel`) on a real MI355X.

The f16x3 step runs most convolutions and many linears as split-K launches whose (tile, splits) come from
`tuned_plans_x3.json`, `planes.heuristic_plan` or `planes.halo_fallback_plan`.  `igemm_x3p_kernel` cuts the K / 32 K tiles, the
halo kernels the channel blocks, as per = ceil(n / splits) (`tests/x3p_slab_classes.py`): slabs start in the middle of a tap --
inside x2, on the tap -> fused-1x1 boundary, inside E1 / E2 --, are shorter than the staging ring, or are empty and must still
write zeros.  Every case below states its slab picture, asserts it, and then compares with fp64 on the host.  CASES is also
what `test_x3p_plan_classes.py` (CPU) holds every plan the library can pick against: this module imports without a GPU.

Stated tolerances (every test prints what it measured):
    single contractions vs fp64 on the host   <= 4e-6 of max |reference|   (the bound of tests/test_gpu_x3p.py, unchanged)
    planes written by the epilogue / reducer  == split of the fp32 value, bit for bit
    two runs of one split launch              bit-identical (the reducer adds in slab order)

Unwritten memory: the workspace and the outputs are `torch.empty`.  Before every launch NaN-filled tensors of their sizes are
allocated and freed, so the caching allocator hands those blocks to the launch: a slab or an M-tail row nobody writes is a NaN
(`rel_err` asserts finiteness), not stale plausible data.  `_poison_works` checks once that the allocator does so.
"""
import collections
import functools
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ief_amd import hip, planes  # noqa: E402
from ief_amd.planes import Planes  # noqa: E402

from x3p_slab_classes import plan_class, slabs, start_sites  # noqa: E402

XTOL = 4e-6

# ---------------------------------------------------------------------------------------------------------------- the cases
# geometry of each family and the slab pictures its split counts give (asserted by every case before it launches)
CONV_IMG = (3, 9, 7)                                  # M = 189: a ragged 256-row tile, or one full and one ragged 128-row tile
CONV_LAYOUTS = {"concat": (96, 64), "plain": (160, 0)}        # 5 K tiles per tap, nk = 45
CONV_COUT = {6: 128, 8: 320}                          # every other tile: 160
CONV_SLABS = {1: [45], 3: [15] * 3, 4: [12, 12, 12, 9], 16: [3] * 15 + [0], 32: [2] * 22 + [1] + [0] * 9}
CONV_SITES = {3: [(0, 0, "tap"), (15, 3, "tap"), (30, 6, "tap")],
              4: [(0, 0, "tap"), (12, 2, "in_x"), (24, 4, "in_x2"), (36, 7, "in_x")]}           # of the concat layout

EXTRA_IMG, EXTRA_C, EXTRA_COUT = (2, 16, 16), 64, 160  # h: 18 K tiles; + CE1 = 96, CE2 = 64: nk = 23; M = 512
EXTRA_SLABS = {(96, 64): {1: [23], 5: [5, 5, 5, 5, 3], 8: [3] * 7 + [2], 12: [2] * 11 + [1], 16: [2] * 11 + [1] + [0] * 4},
               (96, 0): {4: [6, 6, 6, 3]}}
EXTRA_SITES = {((96, 64), 5): [(20, 9, "in_e1")],                                       # ... and that slab crosses into E2
               ((96, 64), 8): [(18, 9, "extras_boundary"), (21, 9, "e2_start")],
               ((96, 64), 12): [(22, 9, "in_e2")],
               ((96, 64), 16): [(22, 9, "in_e2")],
               ((96, 0), 4): [(18, 9, "extras_boundary")]}                              # the last slab is the extras alone

STRIDE_C, STRIDE_COUT = 160, 160                      # nk = 45
STRIDE_SRC = {"s2": (3, 18, 14), "pad_hi": (3, 18, 14), "u": (3, 5, 4)}         # M = 189, 189, 240
STRIDE_SLABS = {1: [45], 3: [15] * 3, 4: [12, 12, 12, 9], 16: [3] * 15 + [0], 23: [2] * 22 + [1]}

HALO_COUT = 160
HALO_SRC = {11: (3, 9, 7), 12: (3, 4, 16), 13: (3, 2, 2)}     # 12 / 13: the smallest source image with a halo / phase form
HALO_SLABS = {1: [5], 2: [3, 2], 3: [2, 2, 1], 4: [2, 2, 1, 0], 5: [1] * 5}     # ncb = 5 channel blocks

GEMM_MNK = (300, 320, 288)                            # nk = 9
GEMM_SLABS = {1: [9], 3: [3, 3, 3], 4: [3, 3, 3, 0], 8: [2, 2, 2, 2, 1, 0, 0, 0]}

Case = collections.namedtuple("Case", "family name kind variant tile splits M N K geo")


def _conv_out_hw(H, W, variant):
    if variant == "u":
        return 2 * H, 2 * W
    if variant == "s2":
        return (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if variant == "pad_hi":
        return (H - 2) // 2 + 1, (W - 2) // 2 + 1
    return H, W


def _build_cases():
    out = []
    B, H, W = CONV_IMG
    for layout, (C1, C2) in CONV_LAYOUTS.items():
        for tile in (1, 2, 3, 4, 5, 6, 7, 8):
            for sp in CONV_SLABS:
                out.append(Case("conv", f"{layout}-t{tile}-s{sp}", "conv", "", tile, sp, B * H * W, CONV_COUT.get(tile, 160),
                                9 * (C1 + C2), dict(img=CONV_IMG, C1=C1, C2=C2, layout=layout)))
    B, H, W = EXTRA_IMG
    for (CE1, CE2), pictures in EXTRA_SLABS.items():
        for tile in (1, 2, 3, 4, 5):
            for sp in pictures:
                out.append(Case("extra", f"e{CE1}+{CE2}-t{tile}-s{sp}", "conv", "e", tile, sp, B * H * W, EXTRA_COUT,
                                9 * EXTRA_C + CE1 + CE2, dict(img=EXTRA_IMG, C1=EXTRA_C, C2=0, CE1=CE1, CE2=CE2)))
    for form, (B, H, W) in STRIDE_SRC.items():
        Ho, Wo = _conv_out_hw(H, W, form)
        for tile in (1, 2, 3, 4, 5):
            for sp in STRIDE_SLABS:
                out.append(Case("stride", f"{form}-t{tile}-s{sp}", "conv", "u" if form == "u" else "s2", tile, sp, B * Ho * Wo,
                                STRIDE_COUT, 9 * STRIDE_C, dict(img=(B, H, W), C1=STRIDE_C, C2=0, form=form)))
    for tile, (B, H, W) in HALO_SRC.items():
        Ho, Wo = _conv_out_hw(H, W, "" if tile == 11 else "u")
        for sp in HALO_SLABS:
            out.append(Case("halo", f"t{tile}-s{sp}", "conv", "" if tile == 11 else "u", tile, sp, B * Ho * Wo, HALO_COUT, 9 * 160,
                            dict(img=(B, H, W), C1=96, C2=64)))
    B, H, W = HALO_SRC[11]
    out.append(Case("halo", "t11-s3-one-source", "conv", "", 11, 3, B * H * W, HALO_COUT, 9 * 160, dict(img=(B, H, W), C1=160, C2=0)))
    M, N, K = GEMM_MNK
    for tile in (1, 2, 3, 4, 5, 7, 8):
        for sp in GEMM_SLABS:
            out.append(Case("gemm", f"t{tile}-s{sp}", "gemm", "", tile, sp, M, N, K, {}))
    for tile in (1, 2, 3, 4, 7, 8):                  # the GEGLU epilogue never splits: one unsplit case per tile the plans give it
        out.append(Case("geglu", f"t{tile}-s1", "gemm", "g", tile, 1, M, N, K, {}))
    return out


CASES = _build_cases()


def case_class(c):
    return plan_class(c.kind, c.variant, c.M, c.N, c.K, c.tile, c.splits)


def _family(name):
    return pytest.mark.parametrize("c", [c for c in CASES if c.family == name], ids=lambda c: c.name)


# ------------------------------------------------------------------------------------------------------------------ helpers
def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return None if t is None else t.cuda()


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "NaN / inf in the result: a slab or an output row was never written"
    return ((got - ref).abs().max() / ref.abs().max()).item()


def ref_split(x):
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi, lo


def assert_planes_equal_split(pl, x32):
    hi, lo = ref_split(x32.float().cpu())
    assert torch.equal(pl.hi.cpu(), hi), "hi plane differs from fp16(x)"
    assert torch.equal(pl.lo.cpu(), lo), "lo plane differs from fp16(x - hi)"


@pytest.fixture(autouse=True)
def _x3():
    with hip.f32_contraction("x3"):
        yield


def _poison(*numels):
    """NaN-filled fp32 blocks of these sizes, alive together, then freed: the allocator's next same-size requests get them"""
    torch.cuda.empty_cache()
    blocks = [torch.full((n,), float("nan"), dtype=torch.float32, device="cuda") for n in numels if n]
    del blocks


@functools.lru_cache(maxsize=None)
def _poison_works():
    M, N = 189, 160
    sizes = (M * N, M * N, 4 * M * N)
    _poison(*sizes)
    back = [torch.empty(n, dtype=torch.float32, device="cuda") for n in sizes]
    ok = all(bool(torch.isnan(t).all()) for t in back)
    if not ok:
        print("x3p-splitk: POISONING INACTIVE -- torch.empty did not return the NaN-filled blocks; unwritten memory may go unseen")
    return ok


def _run_twice(launch, M, N, splits, n_out):
    """launch() twice, each into poisoned outputs and a poisoned workspace; the two results must be the same bits"""
    _poison_works()
    runs = []
    for _ in range(2):
        _poison(*([M * N] * n_out), splits * M * N if splits > 1 else 0)
        r = launch()
        runs.append(r if isinstance(r, tuple) else (r,))
    for a, b in zip(*runs):
        ta, tb = (a.t, b.t) if isinstance(a, Planes) else (a, b)
        assert torch.isfinite(ta).all() and torch.isfinite(tb).all(), "NaN / inf in the result: a slab or an output row was never written"
        assert torch.equal(ta, tb), "two runs of one split launch differ"
    return runs[0]


def _sizes(n, splits):
    return [hi - lo for lo, hi in slabs(n, splits)]


def _conv_ref(x, w, bias, x2=None, stride=1, upsample=False, pad_hi_only=False):
    xin = x if x2 is None else torch.cat([x, x2], -1)
    xin = xin.permute(0, 3, 1, 2).double()
    if upsample:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    wt = w.permute(0, 3, 1, 2).double()
    if pad_hi_only:
        xin = F.pad(xin, (0, 1, 0, 1))
        y = F.conv2d(xin, wt, None if bias is None else bias.double(), stride=stride)
    else:
        y = F.conv2d(xin, wt, None if bias is None else bias.double(), stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


_FORM_KW = {"": {}, "s2": dict(stride=2), "pad_hi": dict(stride=2, pad_hi_only=True), "u": dict(upsample=True)}

Problem = collections.namedtuple("Problem", "ref rv res xp x2p w bias rvd resd extra kw")


@functools.lru_cache(maxsize=None)
def _conv_problem(img, C1, C2, Cout, form="", CE1=0, CE2=0):
    """one seeded convolution (a seed per source, weights at K ** -0.5), its fp64 reference with bias, and its device operands;
    built once per geometry and shared by the cases, which leave it unchanged"""
    B, H, W = img
    kw = _FORM_KW[form]
    K = 9 * (C1 + C2) + CE1 + CE2
    x, x2 = f32(B, H, W, C1, seed=1), (f32(B, H, W, C2, seed=4) if C2 else None)
    wf, bias = f32(Cout, K, seed=2, scale=K ** -0.5), f32(Cout, seed=3, scale=0.1)
    w9 = wf[:, :9 * (C1 + C2)].reshape(Cout, 3, 3, C1 + C2).contiguous()
    ref = _conv_ref(x, w9, bias, x2, **kw)
    extra = None
    if CE1:
        e1, e2 = f32(B, H, W, CE1, seed=7), (f32(B, H, W, CE2, seed=8) if CE2 else None)
        e = e1 if e2 is None else torch.cat([e1, e2], -1)
        ref = ref + e.double() @ wf[:, 9 * (C1 + C2):].double().t()
        extra = (planes.split(dev(e1)), None if e2 is None else planes.split(dev(e2)))
    rv, res = f32(B, Cout, seed=5), f32(*ref.shape, seed=6)
    wd = dev(wf if CE1 else w9)
    planes.weight_planes(wd)                          # made now: their allocation must not take a poisoned block later
    if form == "u":
        hip.x3_upsample_phase_planes(wd, planes.W_SCALE)
    return Problem(ref, rv, res, planes.split(dev(x)), None if x2 is None else planes.split(dev(x2)), wd, dev(bias), dev(rv), dev(res),
                   extra, kw)


def _conv_forms(c, pb, forms):
    """the epilogue forms the model launches with split-K: 'rowvec' = bias + rowvec [B, Cout], fp32 out (ResnetBlock conv1);
    'residual' = bias + residual, fp32 + planes (conv2); 'bias' = bias, fp32 + planes (fused shortcut, Downsample2D, Upsample2D)"""
    errs = {}
    for form in forms:
        if form == "rowvec":
            (out,) = _run_twice(lambda: planes.conv3x3(pb.xp, pb.w, pb.bias, x2=pb.x2p, rowvec=pb.rvd, extra=pb.extra, tile=c.tile,
                                                       splits=c.splits, **pb.kw), c.M, c.N, c.splits, 1)
            errs[form] = rel_err(out, pb.ref + pb.rv.double()[:, None, None, :])
            continue
        res, ref = (pb.resd, pb.ref + pb.res.double()) if form == "residual" else (None, pb.ref)
        out, op = _run_twice(lambda: planes.conv3x3(pb.xp, pb.w, pb.bias, x2=pb.x2p, residual=res, extra=pb.extra, out=True,
                                                    out_planes=True, tile=c.tile, splits=c.splits, **pb.kw), c.M, c.N, c.splits, 2)
        errs[form] = rel_err(out, ref)
        assert_planes_equal_split(op, out)
    return errs


def _report(c, picture, errs):
    print(f"x3p-splitk {c.family} {c.name} {case_class(c)}: {picture}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + " vs fp64")
    for k, v in errs.items():
        assert v < XTOL, (k, v)


# ------------------------------------------------------------------------------------------------------------------ the tests
@_family("conv")
def test_conv_plain_and_concat_slabs_start_mid_tap(c):
    """implicit-GEMM convolution of [x | x2] (and of x alone): slabs that start inside x, inside x2 and on a tap boundary, slabs
    below every ring depth, empty trailing slabs; conv1's and conv2's epilogue through the reducer"""
    C1, C2 = c.geo["C1"], c.geo["C2"]
    sizes = _sizes(c.K // 32, c.splits)
    assert c.M == 189 and c.K // 32 == 45 and sizes == CONV_SLABS[c.splits]
    sites = start_sites(c.splits, C1, C2)
    assert len(sites) == sum(1 for s in sizes if s)
    if c.geo["layout"] == "concat" and c.splits in CONV_SITES:
        assert sites == CONV_SITES[c.splits]
    if c.splits in (16, 32):
        assert max(sizes) <= 3 and sizes.count(0) == {16: 1, 32: 9}[c.splits]
        assert {s for _, _, s in sites} == ({"tap", "in_x", "in_x2"} if C2 else {"tap", "in_x"})
    pb = _conv_problem(c.geo["img"], C1, C2, c.N)
    _report(c, f"slabs {sizes} start at {sites[:4]}{' ...' if len(sites) > 4 else ''}", _conv_forms(c, pb, ("rowvec", "residual")))


@_family("extra")
def test_conv_fused_shortcut_slabs_start_in_the_extras(c):
    """conv3x3(h) + conv1x1([e1 | e2]) in one launch: every split slab starts mid-tap; slabs that start on the tap -> extras
    boundary, inside E1 (crossing into E2), at the first tile of E2 and inside E2; tiles 2 and 4 unsplit as well"""
    CE1, CE2 = c.geo["CE1"], c.geo["CE2"]
    sizes = _sizes(c.K // 32, c.splits)
    assert c.M == 512 and c.K // 32 == 21 + CE2 // 32 and sizes == EXTRA_SLABS[(CE1, CE2)][c.splits]
    sites = start_sites(c.splits, c.geo["C1"], 0, CE1, CE2)
    for want in EXTRA_SITES.get(((CE1, CE2), c.splits), []):
        assert want in sites, (want, sites)
    if c.splits > 1:
        assert any(s != "tap" for _, _, s in sites[1:])       # h has two K tiles per tap: odd starts are mid-tap
    if (CE2, c.splits) == (64, 5):
        lo, hi = slabs(23, 5)[-1]
        assert lo == 20 and lo < 21 < hi                      # starts inside E1, ends inside E2
    if (CE2, c.splits) == (0, 4):
        assert slabs(21, 4)[-1] == (18, 21) and sites[-1] == (18, 9, "extras_boundary")
    pb = _conv_problem(c.geo["img"], c.geo["C1"], 0, c.N, CE1=CE1, CE2=CE2)
    _report(c, f"slabs {sizes} start at {[s for s in sites if s[1] >= 8]} (last two taps and the extras)", _conv_forms(c, pb, ("bias",)))


@_family("stride")
def test_conv_stride2_pad_hi_and_upsample_slabs(c):
    """Downsample2D (stride 2, and the pad-high-only form) and Upsample2D on the implicit GEMM under split-K"""
    form = c.geo["form"]
    sizes = _sizes(c.K // 32, c.splits)
    assert c.M == (240 if form == "u" else 189) and c.K // 32 == 45 and sizes == STRIDE_SLABS[c.splits]
    sites = start_sites(c.splits, c.geo["C1"])
    if c.splits == 4:
        assert sites == [(0, 0, "tap"), (12, 2, "in_x"), (24, 4, "in_x"), (36, 7, "in_x")]
    pb = _conv_problem(c.geo["img"], c.geo["C1"], 0, c.N, form=form)
    assert pb.ref.shape[0] * pb.ref.shape[1] * pb.ref.shape[2] == c.M
    _report(c, f"slabs {sizes}", _conv_forms(c, pb, ("bias",)))


@_family("halo")
def test_conv_halo_ragged_single_block_and_empty_slabs(c):
    """the halo forms cut channel blocks: 3 + 2 (slab 1 is x2 alone), 2 + 2 + 1 (slab 1 crosses x -> x2: an odd block count on
    the two-buffer ring, a one-block slab), the same plus an empty slab, five one-block slabs"""
    B, H, W = c.geo["img"]
    C1, C2 = c.geo["C1"], c.geo["C2"]
    ncb = (C1 + C2) // 32
    sl = slabs(ncb, c.splits)
    sizes = [hi - lo for lo, hi in sl]
    assert ncb == 5 and c.splits <= ncb and sizes == HALO_SLABS[c.splits]
    if C2 and c.splits == 2:
        assert sl[1][0] * 32 == C1                            # slab 1 is x2 alone
    if C2 and c.splits in (3, 4):
        assert sl[1][0] * 32 < C1 < sl[1][1] * 32             # slab 1 crosses x -> x2
    ups = c.tile != 11
    g = hip.conv_geometry((B, H, W, C1), (c.N, 3, 3, C1 + C2), (B, H, W, C2) if C2 else None, upsample=ups)
    assert B % 2 == 1 and g.M == c.M
    if c.tile == 11:
        assert g.halo_geom
    elif c.tile == 12:           # no smaller source image has the fused nearest-2x halo form
        assert g.halo_geom and not any(hip.conv_geometry((B, h, w, C1), (c.N, 3, 3, C1 + C2), (B, h, w, C2), upsample=True).halo_geom
                                       for h in range(1, 65) for w in range(1, 65) if h * w < H * W)
    else:
        assert g.phase_geom and not any(hip.conv_geometry((B, h, w, C1), (c.N, 3, 3, C1 + C2), (B, h, w, C2), upsample=True).phase_geom
                                        for h in range(1, 3) for w in range(1, 3) if h * w < H * W)
    pb = _conv_problem(c.geo["img"], C1, C2, c.N, form="u" if ups else "")
    _report(c, f"channel-block slabs {sizes}", _conv_forms(c, pb, ("residual",) if c.tile == 11 else ("bias",)))


def test_conv_halo_refuses_more_slabs_than_channel_blocks():
    """`planes.conv3x3` clamps splits to the channel blocks (7 asked for run as the five one-block slabs); the library itself
    refuses a halo plan with more slabs than channel blocks (IEF_ESHAPE) and launches nothing"""
    B, H, W = HALO_SRC[11]
    M = B * H * W
    pb = _conv_problem(HALO_SRC[11], 96, 64, HALO_COUT)
    (out,) = _run_twice(lambda: planes.conv3x3(pb.xp, pb.w, pb.bias, x2=pb.x2p, tile=11, splits=7), M, HALO_COUT, 5, 1)
    e = rel_err(out, pb.ref)
    print(f"x3p-splitk halo t11 splits 7 clamped to 5: {e:.2e} vs fp64")
    assert e < XTOL
    o, ws = torch.zeros(M, HALO_COUT, device="cuda"), torch.zeros(6 * M * HALO_COUT, device="cuda")
    wp = planes.weight_planes(pb.w)
    p = hip.IefGemmX3pParams()
    p.A, p.planeA, p.A2, p.planeA2 = pb.xp.t.data_ptr(), pb.xp.plane, pb.x2p.t.data_ptr(), pb.x2p.plane
    p.W, p.planeW, p.ldw = wp.data_ptr(), wp.stride(0), 1440
    p.Out, p.ldo, p.M, p.N, p.K = o.data_ptr(), HALO_COUT, M, HALO_COUT, 1440
    p.conv, p.H, p.Wd, p.C1, p.C2, p.Ho, p.Wo, p.stride, p.batch_images = 1, H, W, 96, 64, H, W, 1, B
    p.out_scale, p.inv_scale, p.zeros = 1.0, 1.0 / (planes.ACT_SCALE * planes.W_SCALE), hip._zeros(o.device)
    p.tile, p.splits, p.ws = 11, 6, ws.data_ptr()
    assert hip.load().ief_gemm_x3p(byref(p), hip._stream()) == -2            # IEF_ESHAPE
    assert o.abs().max() == 0 and ws.abs().max() == 0


@functools.lru_cache(maxsize=None)
def _gemm_problem():
    M, N, K = GEMM_MNK
    a, w = f32(M, K, seed=1), f32(N, K, seed=2, scale=K ** -0.5)
    bias, res, rv = f32(N, seed=3, scale=0.1), f32(M, N, seed=4), f32(2, N, seed=5)
    wide = f32(M, K + 64, seed=6)
    wd = dev(w)
    planes.weight_planes(wd)
    return dict(a=a, w=w, bias=bias, res=res, rv=rv, wide=wide, ap=planes.split(dev(a)), widep=planes.split(dev(wide)), wd=wd,
                biasd=dev(bias), resd=dev(res), rvd=dev(rv), acc=a.double() @ w.double().t())


@_family("gemm")
def test_gemm_empty_and_short_slabs_through_the_reducer(c):
    """linear GEMM with nk = 9: 3 + 3 + 3 + an empty slab; 2 + 2 + 2 + 2 + 1 + three empty slabs.  Forms: bias + residual +
    out_scale into fp32 + planes; bias + rowvec [2, N] into planes alone; a column slice of wider planes into a column slice of a
    wider zeroed tensor whose spare columns stay 0"""
    M, N, K = GEMM_MNK
    sizes = _sizes(K // 32, c.splits)
    assert (c.M, c.N, c.K) == GEMM_MNK and K // 32 == 9 and sizes == GEMM_SLABS[c.splits]
    g = _gemm_problem()
    errs = {}
    out, op = _run_twice(lambda: planes.gemm(g["ap"], g["wd"], bias=g["biasd"], residual=g["resd"], out_scale=0.5, out=True,
                                             out_planes=True, tile=c.tile, splits=c.splits), M, N, c.splits, 2)
    errs["residual+scale"] = rel_err(out, (g["acc"] + g["bias"].double() + g["res"].double()) * 0.5)
    assert_planes_equal_split(op, out)
    (o2,) = _run_twice(lambda: planes.gemm(g["ap"], g["wd"], bias=g["biasd"], rowvec=g["rvd"], rows_per_batch=150, out=False,
                                           out_planes=True, tile=c.tile, splits=c.splits), M, N, c.splits, 1)
    assert isinstance(o2, Planes)
    errs["rowvec->planes"] = rel_err(o2.to_f32(), g["acc"] + g["bias"].double() + g["rv"].double().repeat_interleave(150, 0))
    owides = []
    for _ in range(2):
        owide = torch.zeros(M, N + 4, device="cuda")
        _poison(c.splits * M * N if c.splits > 1 else 0)
        planes.gemm(g["widep"][:, 32:32 + K], g["wd"], out=owide[:, :N], tile=c.tile, splits=c.splits)
        owides.append(owide)
    assert torch.equal(owides[0], owides[1]), "two runs of one split launch differ"
    errs["strided"] = rel_err(owides[0][:, :N], g["widep"][:, 32:32 + K].to_f32().double().cpu() @ g["w"].double().t())
    assert owides[0][:, N:].abs().max() == 0, "the launch wrote past the N columns of its output view"
    _report(c, f"slabs {sizes}", errs)


@_family("geglu")
def test_gemm_geglu_unsplit_on_every_tile_the_plans_give_it(c):
    """the `|g` plans: the fused GEGLU epilogue never splits (`planes.gemm` forces splits = 1); one launch per tile the table names"""
    M, N, K = GEMM_MNK
    assert c.splits == 1 and _sizes(K // 32, 1) == [9]
    g = _gemm_problem()
    out, op = _run_twice(lambda: planes.gemm(g["ap"], g["wd"], bias=g["biasd"], geglu=True, out=True, out_planes=True, tile=c.tile,
                                             splits=4), M, N // 2, 1, 2)         # splits asked for, not run
    pre = (g["acc"] + g["bias"].double()).reshape(M, N // 16, 2, 8)
    ref = (pre[:, :, 0] * F.gelu(pre[:, :, 1])).reshape(M, N // 2)
    assert_planes_equal_split(op, out)
    _report(c, "slabs [9]", {"geglu": rel_err(out, ref)})
