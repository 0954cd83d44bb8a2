"""The MFMA padding of the planes attention (`attn_flash_x3p_kernel`, `csrc/split_x3.hip`) on a real MI355X: where the head
dim is no multiple of 32 the padding rows of the last O^T tile carry V's lo plane and (d = 40) a row of ones whose product with
P is the softmax row sum; at d = 40 the score product's padding column 40 carries the exponent's bias (Q scaled to log2 units once,
an integer running maximum that the first tile of a walk may move DOWN).  Every case compares `planes.attn_flash` with an fp64 host reference computed from the planes' own
values (hi + lo), so the split of the inputs is not part of the error.

Shapes (B = 2, heads = 2; the smallest at which each path can go wrong):
    d = 40, key tile 64:  N = L = 96 (one full tile and a masked tail), N = 70 (rows past N inside a wave), L = 192 (three tiles:
                          the single launch with lse, and two key splits with lse -- the row sum travels through the workspace)
    d = 80, key tile 32:  N = L = 48, and L = 80 (a masked tail of 16 keys)
    d = 64:               N = L = 96, the path without padding rows
Inputs: unit gaussians; q and k scaled by 3; planted keys that move the row maximum in every tile (the rows of
tests/test_gpu_x3.py::test_attention_x3_peaky_rows_force_the_rescale); every score of a row around -300 in log2 units (q = a u +
noise, k = -a u + noise: the running maximum starts far below zero and the row sum is a sum of small integers' worth of 2^10);
one output batch row redirected through k_src / v_src.

Stated tolerances (every test prints what it measured before it asserts):
    output vs fp64                      <= 4e-6 of max |reference|   (one contraction: the bound of tests/test_gpu_x3p.py)
    lse vs fp64 logsumexp (log2 units)  <= 1e-5 absolute             (the bound of tests/test_gpu_grad_f32.py)
    split vs single launch              <= 2 * 4e-6                  (each within 4e-6 of the same reference)
    planes out                          == split of the fp32 out, bit for bit
    two launches on equal inputs        bit-equal
What fp32 itself allows, where the project's bounds (set on scores and lse of a few tens at most) cannot hold:
  * a score lives in an fp32 accumulator.  One rounding of a score of magnitude |s| (log2 units) moves it by up to 2^-24 |s|
    and its P by the factor ln 2 times that; the 3 * ceil(d / 16) MFMA partial sums and the scale count as ROUNDINGS = 4
    full-magnitude roundings.  The far-below-zero rows (|s| up to 350: 5.8e-5 in P) are therefore held to being finite and to
    4e-6 + ln2 * ROUNDINGS * 2^-24 * max |s|; every other input to 4e-6.  (The kernel measured 1e-5 .. 1.9e-5 there before its padding was put to work, 1.0e-5 .. 1.4e-5 after.)
  * the lse is an fp32 output, m + log2 l - 10: three roundings at half the fp32 spacing of its magnitude, on top of the score's
    own error, which it inherits.  1e-5 absolute is representable below 32 (half spacing 9.5e-7); an input whose |lse| reaches 32
    is held to 1e-5 + 3 * 2^(floor(log2 |lse|) - 24) + ROUNDINGS * 2^-24 * max |s| instead.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from ief_amd import hip, planes  # noqa: E402

DEV = torch.device("cuda:0")
XTOL = 4e-6
LSETOL = 1e-5
ROUNDINGS = 4
LOG2E = 1.4426950408889634
B, HEADS = 2, 2

#          name         N    L    d   key splits, lse
SHAPES = {"d40":       (96,  96,  40, 1, False),
          "d40_n70":   (70,  96,  40, 1, False),
          "d40_l192":  (96,  192, 40, 2, True),
          "d80":       (48,  48,  80, 1, False),
          "d80_l80":   (48,  80,  80, 1, False),
          "d64":       (96,  96,  64, 1, False)}
INPUTS = ("gauss", "scaled3", "peaky", "low", "src")


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def ref_split(x):
    """the definition of the planes: two round-to-nearest conversions"""
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi, lo


def _inputs(kind, N, L, d):
    C = HEADS * d
    q, k, v = f32(B, N, C, seed=1), f32(B, L, C, seed=2), f32(B, L, C, seed=3)
    scale = d ** -0.5
    if kind == "scaled3":
        q, k = q * 3.0, k * 3.0
    elif kind == "peaky":                       # a planted key in every 32: the maximum of query 5 moves in every tile
        for t in range(L // 32):
            k[0, 32 * t + 7, :] = q[0, 5, :] * (0.5 + 0.25 * t)
        scale = scale * 4.0
    elif kind == "low":                         # scale * q . k = -a^2 scale + O(a scale): -300 / log2(e) with a^2 = 208 sqrt(d)
        u = f32(1, 1, HEADS, d, seed=4)
        u = (u / u.norm(dim=-1, keepdim=True)).reshape(1, 1, C)
        a = (208.0 * d ** 0.5) ** 0.5
        q, k = a * u + q, -a * u + k
    return q, k, v, scale


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """device planes, the launch's arguments and the fp64 reference (out, lse in log2 units) of one (shape, input) pair: made
    once and shared by the tests below, which leave it unchanged"""
    N, L, d, S, want_lse = SHAPES[shape]
    C = HEADS * d
    q, k, v, scale = _inputs(kind, N, L, d)
    if N == L:                                  # column slices of one q|k|v planes tensor, as the transformer block passes them
        qkv = planes.split(torch.cat([q, k, v], -1).to(DEV))
        qp, kp, vp = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    else:
        qp, kp, vp = planes.split(q.to(DEV)), planes.split(k.to(DEV)), planes.split(v.to(DEV))
    ks = torch.arange(B, dtype=torch.int32)
    if kind == "src":
        ks[-1] = 0                              # the last output batch row takes its keys and values from row 0
    val = lambda p: (p.hi.double() + p.lo.double()).cpu()  # noqa: E731
    qh = val(qp).reshape(B, N, HEADS, d).permute(0, 2, 1, 3)
    kh = val(kp)[ks.long()].reshape(B, L, HEADS, d).permute(0, 2, 1, 3)
    vh = val(vp)[ks.long()].reshape(B, L, HEADS, d).permute(0, 2, 1, 3)
    sc = qh @ kh.transpose(-1, -2) * scale
    ref = (torch.softmax(sc, -1) @ vh).permute(0, 2, 1, 3).reshape(B, N, C)
    src = ks.to(DEV) if kind == "src" else None
    return dict(qp=qp, kp=kp, vp=vp, src=src, scale=scale, ref=ref, lse2=torch.logsumexp(sc, -1) * LOG2E, sc2=sc * LOG2E)


def _run(c, **kw):
    return planes.attn_flash(c["qp"], c["kp"], c["vp"], HEADS, c["scale"], k_src=c["src"], v_src=c["src"], **kw)


def _err(got, ref):
    got = got.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite output"
    return ((got - ref).abs().max() / ref.abs().max()).item()


def _score_err(c):
    """what ROUNDINGS fp32 roundings do to the largest score (log2 units)"""
    return ROUNDINGS * 2.0 ** -24 * c["sc2"].abs().max().item()


def _out_tol(c, kind):
    return XTOL + (math.log(2.0) * _score_err(c) if kind == "low" else 0.0)


def _lse_tol(c):
    m = c["lse2"].abs().max().item()
    return LSETOL if m < 32.0 else LSETOL + 3 * 2.0 ** (math.floor(math.log2(m)) - 24) + _score_err(c)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_padding_attention_vs_fp64(shape, kind):
    N, L, d, S, want_lse = SHAPES[shape]
    c = _case(shape, kind)
    if kind == "low":
        print(f"    scores of the far-below-zero rows (log2 units): {c['sc2'].min().item():.1f} .. {c['sc2'].max().item():.1f}")
        assert c["sc2"].max().item() < -200.0
    lse = torch.full((B, HEADS, N), float("nan"), device=DEV) if want_lse else None
    hip.profile_begin()
    out = _run(c, out_planes=False, lse=lse)
    names = [r[0] for r in hip.profile_end()]
    assert names == [f"attn_flash_x3p_kernel<{d}>"], names
    again = _run(c, out_planes=False)
    op = _run(c)
    e = _err(out, c["ref"])
    print(f"padding attention {shape} N={N} L={L} d={d} {kind}: {e:.2e} of max |ref| (bound {_out_tol(c, kind):.2e})")
    assert e <= _out_tol(c, kind)
    assert torch.equal(out, again), "two launches on equal inputs must give the same bits"
    hi, lo = ref_split(out.float().cpu())
    assert torch.equal(op.hi.cpu(), hi), "hi plane differs from fp16(out)"
    assert torch.equal(op.lo.cpu(), lo), "lo plane differs from fp16(out - hi)"
    if want_lse:
        assert torch.isfinite(lse).all(), "lse not written"
        e_lse = (lse.double().cpu() - c["lse2"]).abs().max().item()
        print(f"    lse: {e_lse:.2e} (|lse| <= {c['lse2'].abs().max().item():.1f}, bound {_lse_tol(c):.2e})")
        assert e_lse <= _lse_tol(c)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("shape", [s for s in SHAPES if SHAPES[s][3] > 1])
def test_padding_attention_key_split(shape, kind):
    """the split's (O, m, l) partials, l read off the ones row, through the workspace and the combine"""
    N, L, d, S, want_lse = SHAPES[shape]
    c = _case(shape, kind)
    assert planes.attn_key_splits(B, HEADS, N, L, d, setting=S) == S
    lse = torch.full((B, HEADS, N), float("nan"), device=DEV)
    hip.profile_begin()
    out = _run(c, out_planes=False, lse=lse, key_splits=S)
    names = [r[0] for r in hip.profile_end()]
    assert len(names) == 1 and f"split {S}>" in names[0], names
    again = _run(c, out_planes=False, key_splits=S)
    op = _run(c, key_splits=S)
    one = _run(c, out_planes=False)
    e = _err(out, c["ref"])
    diff = (out.double() - one.double()).abs().max().item() / c["ref"].abs().max().item()
    assert torch.isfinite(lse).all(), "the combine returned without writing lse"
    e_lse = (lse.double().cpu() - c["lse2"]).abs().max().item()
    print(f"padding attention {shape} {kind}, {S} key splits: {e:.2e} of max |ref|, vs single launch {diff:.2e}, lse {e_lse:.2e} (bound {_lse_tol(c):.2e})")
    assert e <= _out_tol(c, kind)
    assert diff <= 2 * XTOL
    assert e_lse <= _lse_tol(c)
    assert torch.equal(out, again), "fixed combine order: two launches must give the same bits"
    hi, lo = ref_split(out.float().cpu())
    assert torch.equal(op.hi.cpu(), hi) and torch.equal(op.lo.cpu(), lo), "planes out differ from the split of the fp32 out"
