"""The K-concatenated A operand of the planes GEMM and the transformer tail folded onto it (`csrc/gemm_x3p.hip` KCAT,
`ief_x3_fold_linear_pair`, `Transformer2DModel.tail_fold`) on a real MI355X.

A K-concatenated launch computes [A | A2] . W^T with W one [N, K1 + K2] tensor: K tiles below K1 / 32 are staged from A, the rest
from A2; a split-K range may end exactly at K1 or straddle it.  The tail of every Transformer2DModel,
    r = g W2^T + b2 + h,   out = r Wp^T + bp + x,
runs as ONE such launch over [g | h] with the folded weight [Wp W2 | Wp] and bias Wp b2 + bp.

Stated tolerances (every test prints what it measured):
    a K-concatenated launch vs fp64 on the host            <= 4e-6 of max |reference|   (the bound of tests/test_gpu_x3p.py)
    planes written by the epilogue / reducer               == split of the fp32 value, bit for bit
    K-concatenated vs one plain launch over [A | A2]       bit for bit, per tile and split count
    library fold vs the fp64 host reference                one rounding to fp32 (half an ulp of every element)
    folded tail vs fp64                                    <= 2 x the error of the two-launch chain, measured in the same test
    one UNet forward (eps), fold on and off, vs the oracle <= 1e-4   (the bound of tests/test_gpu_x3.py)
    captured step graph vs eager stepping, fold on         bit for bit
"""
import functools
from ctypes import byref

import pytest
import torch

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip, planes  # noqa: E402
from ief_amd.planes import Planes  # noqa: E402

from x3p_slab_classes import slabs  # noqa: E402

DEV = torch.device("cuda:0")
XTOL = 4e-6
KS = [(64, 32), (32, 64), (128, 32)]
SPLITS = [1, 2, 3]
TILES_N = [(3, 80), (3, 160), (1, 160), (4, 160), (6, 128)]       # (tile, N): every tile with a K-concatenated instantiation


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "NaN / inf in the result"
    return ((got - ref).abs().max() / ref.abs().max()).item()


def assert_planes_equal_split(pl, x32):
    x = x32.float().cpu()
    hi = x.half()
    lo = (x - hi.float()).half()
    assert torch.equal(pl.hi.cpu(), hi), "hi plane differs from fp16(x)"
    assert torch.equal(pl.lo.cpu(), lo), "lo plane differs from fp16(x - hi)"


@pytest.fixture(autouse=True)
def _x3():
    with hip.f32_contraction("x3"):
        yield


@functools.lru_cache(maxsize=None)
def _problem(M, N, K1, K2):
    """one seeded problem, its fp64 reference and its device operands; A2 is a column slice of a wider planes tensor (lda2 > K2);
    shared by the cases, which leave it unchanged"""
    a, a2 = f32(M, K1, seed=1), f32(M, K2, seed=2)
    w = f32(N, K1 + K2, seed=3, scale=(K1 + K2) ** -0.5)
    bias, res = f32(N, seed=4, scale=0.1), f32(M, N, seed=5)
    ref = a.double() @ w[:, :K1].double().t() + a2.double() @ w[:, K1:].double().t() + bias.double() + res.double()
    wide = torch.zeros(M, K2 + 64)
    wide[:, 32:32 + K2] = a2
    ap, widep = planes.split(a.to(DEV)), planes.split(wide.to(DEV))
    a2p = widep[:, 32:32 + K2]
    assert a2p.rows_ld()[2] == K2 + 64
    catp = Planes(torch.cat([ap.t, a2p.t], -1).contiguous())
    return ref, ap, a2p, catp, w.to(DEV), bias.to(DEV), res.to(DEV)


def test_the_split_counts_cut_at_k1_and_across_it():
    """of the (K1, K2) x splits cases below, some slab ends exactly on K1 and some slab straddles it"""
    ends, straddles = set(), set()
    for K1, K2 in KS:
        for sp in SPLITS[1:]:
            for lo, hi in slabs((K1 + K2) // 32, sp):
                if hi == K1 // 32 and hi > lo:
                    ends.add((K1, K2, sp))
                if lo < K1 // 32 < hi:
                    straddles.add((K1, K2, sp))
    print(f"kcat: slab ends at K1 in {sorted(ends)}, straddles K1 in {sorted(straddles)}")
    assert ends and straddles and {k[:2] for k in ends | straddles} == set(KS)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("K1,K2", KS)
@pytest.mark.parametrize("tile,N", TILES_N)
@pytest.mark.parametrize("M", [192, 64])
def test_kcat_vs_fp64_and_the_plain_launch(M, tile, N, K1, K2, splits):
    ref, ap, a2p, catp, w, bias, res = _problem(M, N, K1, K2)
    kw = dict(bias=bias, residual=res, tile=tile, splits=splits)
    o32 = planes.gemm(ap, w, a2=a2p, out=True, **kw)
    e = rel_err(o32, ref)
    print(f"kcat M={M} N={N} K={K1}+{K2} t{tile} s{splits}: rel err {e:.3e}")
    assert e < XTOL
    op = planes.gemm(ap, w, a2=a2p, out=False, out_planes=True, **kw)
    assert isinstance(op, Planes)
    assert_planes_equal_split(op, o32)
    b32, bp = planes.gemm(ap, w, a2=a2p, out=True, out_planes=True, **kw)
    assert torch.equal(b32, o32)
    assert_planes_equal_split(bp, o32)
    plain = planes.gemm(catp, w, out=True, **kw)
    assert torch.equal(plain, o32), "the K-concatenated launch must give the bits of one plain launch over [A | A2]"


def _raw(M=64, N=80, K1=64, K2=32):
    """the parameter block of a valid K-concatenated launch on tile 3 and the tensors it points to"""
    ref, ap, a2p, catp, w, bias, res = _problem(M, N, K1, K2)
    wp = planes.weight_planes(w)
    out = torch.full((M, N), -7.0, dtype=torch.float32, device=DEV)
    p = hip.IefGemmX3pParams()
    p.A, p.planeA, p.lda = ap.t.data_ptr(), ap.plane, K1
    p.A2, p.planeA2, p.lda2, p.K1 = a2p.t.data_ptr(), a2p.plane, a2p.rows_ld()[2], K1
    p.W, p.planeW, p.ldw = wp.data_ptr(), wp.stride(0), K1 + K2
    p.Out, p.ldo = out.data_ptr(), N
    p.M, p.N, p.K = M, N, K1 + K2
    p.out_scale, p.inv_scale = 1.0, 1.0 / (planes.ACT_SCALE * planes.W_SCALE)
    p.tile, p.splits, p.zeros = 3, 1, hip._zeros(DEV)
    return p, out, (ap, a2p, w, wp, ref)


def test_front_end_refusals_launch_nothing():
    lib = hip.load()
    EINVAL, ESHAPE, EALIGN = -1, -2, -3

    def refused(change, code):
        p, out, keep = _raw()
        change(p)
        rc = lib.ief_gemm_x3p(byref(p), hip._stream())
        torch.cuda.synchronize()
        assert rc == code, (rc, code)
        assert bool((out == -7.0).all()), "a refused launch wrote its output"

    p, out, keep = _raw()
    assert lib.ief_gemm_x3p(byref(p), hip._stream()) == 0
    torch.cuda.synchronize()
    assert rel_err(out, keep[4] - _problem(64, 80, 64, 32)[6].double().cpu() - _problem(64, 80, 64, 32)[5].double().cpu()) < XTOL

    def misaligned(p):
        p.A2 = p.A2 + 8
    refused(misaligned, EALIGN)

    def odd_lda2(p):
        p.lda2 = p.lda2 + 4
    refused(odd_lda2, EALIGN)

    def k1_not_32(p):
        p.K1 = 48
    refused(k1_not_32, ESHAPE)

    def k1_is_k(p):
        p.K1 = p.K
    refused(k1_is_k, ESHAPE)

    def with_geglu(p):
        p.geglu = 1
    refused(with_geglu, EINVAL)

    def with_conv(p):
        p.conv = 1
    refused(with_conv, EINVAL)

    def no_a2(p):
        p.A2 = None
    refused(no_a2, EINVAL)

    def other_tile(p):
        p.tile = 8
    refused(other_tile, EINVAL)


def test_fold_library_vs_host_reference():
    C, K = 64, 256
    wp, w2 = f32(C, C, seed=11, scale=C ** -0.5), f32(C, K, seed=12, scale=K ** -0.5)
    b2, bp = f32(C, seed=13, scale=0.1), f32(C, seed=14, scale=0.1)
    d = [t.to(DEV) for t in (wp, w2, b2, bp)]
    wcat, bcat = hip.x3_fold_linear_pair(*d)
    assert hip.x3_fold_linear_pair(*d)[0] is wcat, "the folded weight is cached per weight pair"
    rw, rb = hip.fold_linear_pair_ref(wp, w2, b2, bp)
    assert wcat.shape == (C, K + C) and bcat.shape == (C,) and wcat.dtype == torch.float32
    for got, ref in ((wcat, rw), (bcat, rb)):
        err = (got.double().cpu() - ref).abs()
        assert bool((err <= ref.abs() * 2.0 ** -24 * (1 + 1e-6) + 1e-45).all()), "more than one rounding to fp32"
    assert torch.equal(wcat[:, K:].cpu(), wp)
    d[1].mul_(2.0)                                    # an in-place update of a source re-derives the fold
    w2b = hip.x3_fold_linear_pair(*d)[0]
    assert w2b is not wcat and rel_err(w2b[:, :K], 2.0 * rw[:, :K]) < 1e-6
    nb = hip.x3_fold_linear_pair(d[0], d[1], None, None)
    assert float(nb[1].abs().max()) == 0.0


def test_fold_vs_the_two_launch_chain():
    """one transformer tail at C = 64, K = 256, M = 192, gaussian weights at fan-in scaling: the folded launch and today's two
    launches each against fp64"""
    C, K, M = 64, 256, 192
    wp, w2 = f32(C, C, seed=21, scale=C ** -0.5), f32(C, K, seed=22, scale=K ** -0.5)
    b2, bp = f32(C, seed=23, scale=0.1), f32(C, seed=24, scale=0.1)
    g, h, x = f32(M, K, seed=25), f32(M, C, seed=26), f32(M, C, seed=27)
    r = g.double() @ w2.double().t() + b2.double() + h.double()
    ref = r @ wp.double().t() + bp.double() + x.double()
    dwp, dw2, db2, dbp, dx = (t.to(DEV) for t in (wp, w2, b2, bp, x))
    gp, hp = planes.split(g.to(DEV)), planes.split(h.to(DEV))
    rp = planes.gemm(gp, dw2, bias=db2, residual=h.to(DEV), out=False, out_planes=True)
    chain = planes.gemm(rp, dwp, bias=dbp, residual=dx, out=True)
    wcat, bcat = hip.x3_fold_linear_pair(dwp, dw2, db2, dbp)
    fold = planes.gemm(gp, wcat, a2=hp, bias=bcat, residual=dx, out=True)
    e_chain, e_fold = rel_err(chain, ref), rel_err(fold, ref)
    print(f"transformer tail C={C} K={K} M={M}: two launches {e_chain:.3e}, folded {e_fold:.3e} of max |ref|")
    assert e_fold <= 2.0 * e_chain


# ----------------------------------------------------------------------------------------------- whole UNet
@pytest.fixture(scope="module")
def smallx3():
    from ief_amd.pipeline import StableDiffusionPipeline
    return StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")


def test_unet_forward_fold_on_and_off_vs_oracle(smallx3, monkeypatch):
    from oracle import unet_ref
    pipe, B, t = smallx3, 4, 981
    assert pipe.unet.x3p, "the small family runs on operand planes"
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 4, pipe.cfg.sample_size, pipe.cfg.sample_size, generator=gen)
    ctx = torch.randn(B, 77, pipe.cfg.cross_attention_dim, generator=gen)
    ref = unet_ref.unet_forward(pipe._state_dict, pipe.cfg, x, torch.tensor(t), ctx)
    n_tr = sum(1 for m in pipe.unet.modules() if m.__class__.__name__ == "Transformer2DModel")
    for on in (True, False):
        monkeypatch.setattr(planes, "FOLD_TAIL", on)
        hip.profile_begin()
        eps = pipe.unet(x.to(DEV), t, encoder_hidden_states=ctx.to(DEV))["sample"]
        rows = hip.profile_end()
        kcat = sum(1 for r in rows if "kcat" in r[0])
        e = rel_err(eps, ref)
        print(f"f16x3 small B={B} t={t} fold {'on' if on else 'off'}: rel err {e:.3e}, {kcat} K-concatenated launches, {len(rows)} launches")
        assert kcat == (n_tr if on else 0)
        assert e < 1e-4


def test_graph_equals_eager_with_the_fold_on(smallx3, monkeypatch):
    from ief_amd.denoise import FusedDenoiser
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.register import register_attention_control, unregister_attention_control
    from ief_amd.p2p.model.sd_utils import _encode_prompts
    pipe, steps = smallx3, 2
    prompts = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]
    monkeypatch.setattr(planes, "FOLD_TAIL", True)
    with torch.no_grad():
        u, c = _encode_prompts(pipe, prompts)
    ctx, hw = torch.cat([u, c]), pipe.cfg.sample_size
    x_T = torch.randn(1, 4, hw, hw, generator=torch.Generator().manual_seed(8888))
    lat = {}
    for use_graph in (True, False):
        ctl = AttentionRefine(prompts, pipe.tokenizer, steps, 0.8, 0.4, device=DEV)
        register_attention_control(pipe, ctl)
        pipe.scheduler.set_timesteps(steps)
        loop = FusedDenoiser(pipe, ctx, 2, (hw, hw), 7.5, use_graph=use_graph)
        try:
            lat[use_graph] = loop.run(x_T.to(DEV)).float().cpu()
        finally:
            loop.release()
            unregister_attention_control(pipe, ctl)
    assert torch.isfinite(lat[True]).all()
    assert torch.equal(lat[True], lat[False]), "captured-graph replay must equal eager stepping bit for bit"
