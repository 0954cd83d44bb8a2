"""The kernels of the fp16-storage reverse pass (`precision="f16"`, the default), one by one, against fp64 at the shapes and call
forms at which they take another path, on a real MI355X: csrc/attention_bwd.hip, csrc/backward.hip, csrc/map_loss.hip as
`ief_amd/grad.py` drives them and `ief_amd/hip.py` shapes their launches.

tests/test_gpu_grad.py holds each of them to fp32 autograd at a handful of friendly shapes; this file adds
  1. attention backward: sizes below / one past a tile, B = 3, every head dim; the query-split dK / dV path (uneven splits, an
     EMPTY trailing split, the reducer past its 2048-workgroup cap, two runs bit-identical); dQ only / dK, dV only with the
     other destinations untouched; q | k | v and dq | dk | dv as column slices (grad.py's self- and cross-attention forms); dO
     over three magnitudes; explicit `ds_mul`; peaked softmax rows; N = L = 4096; `ief_attn_bwd_delta_f32` past its grid cap
     with ldo != lddo; the refusals of `ief_attn_bwd_f16`
  2. GroupNorm backward: the two-launch form (ragged HW, empty trailing pixel splits, C8 > 256, 64 groups) and the
     one-workgroup form (HW = 1, 2 channels per group, a group straddling the concat, the 4096-pixel slab, inputs offset by 30,
     the fall-back when `stats` is given but C1 % 8 != 0), each with SiLU on / off and `add` given / None; refusals; saturation
  3. LayerNorm backward: one row, C = 8 (one live lane), C = 2048 (the limit), rows % 4 != 0, `add=None`, rows offset up to +-20
  4. GEGLU (interleaved) forward and backward: past the 4096-workgroup cap with a ragged tail, one chunk, |gate| to 12, overflow
  5. `zero_insert2x`, `pool2x2_sum`, `conv_out_bwd` at one element, odd non-square sizes and past the cap; the 3x3 data gradients
     (plain, stride 2, nearest-2x) on an 8 x 12 image
  6. the Pix2Pix-zero map objective: N*G below one workgroup, L = 1 and 96, every head dim, strided q / k / dq, `loss=None`
  7. `nti_loss_grad` below one stride of its workgroup, at 16384 elements and at zero residual; `nti_adam` at n = 1 and 257

Every reference is torch (autograd or plain arithmetic) in fp64 on the CPU, computed inside the test on exactly the fp16-rounded
inputs the kernel receives; no kernel of this library serves as a reference.  Tolerances are the project's own (head of
tests/test_gpu_grad.py), relative to max |reference| unless said otherwise; every test prints what it measured:
    single adjoint kernels (GroupNorm, LayerNorm, map objective dq)        <= 1e-2   (fp16 storage of gradients)
    attention backward                                                     <= 2e-2;  lse <= 2e-2 absolute (log2 units)
    GEGLU forward and backward, conv_out backward                          <= 2e-3
    3x3 data gradients                                                     <= 5e-3   (test_conv_data_gradient_vs_autograd)
    `ief_attn_bwd_delta_f32` (fp16 inputs, fp32 sum of d <= 160 terms)      <= 1e-3
    `pool2x2_sum`: the fp64 sum rounded once to fp16, +- one fp16 ulp (the fp32 sum of four fp16 numbers is not always exact:
        a second rounding can move the result by one ulp); `zero_insert2x`: bit-equal
    map objective value: <= 4 x the error of the objective evaluated by torch in fp32 on the CPU, floored at 1e-3 relative
    NTI objective and gradient <= 1e-5, Adam <= 1e-6 absolute on the parameters (test_nti_loss_grad_and_adam_vs_torch)
    saturation: where |reference| > 1.01 * 65504 the output is exactly +-65504, everything is finite; elements within 1 % of
        65504 are exempt and number < 1 % of the saturating ones; the others are within the kernel's tolerance of 65504
    gradients not requested / columns between slices: still the sentinel (or zero) they were filled with

Where the launch policy does not select the path a case was listed for (the case is kept, the nearest shape that does is added):
    GroupNorm (1, 1024, 512, 0, 64) with `stats`: 8 channels per group make a 16 KiB slab, below the 48 KiB threshold of the
        two-launch form, so it runs the one-workgroup form with 64 groups; (1, 4096, 512, 0, 64) is the two-launch form with 64 groups.
    `PYs` limited by GNB_PART_FLOATS / C cannot happen: 256 / C8 = 2048 / C is never above 4096 / C.
    Attention (160, 3, 1, 256, 5376): `hip.attn_bwd`'s formula does select 2 splits there (126 blocks < 128, 4 tiles), as listed.
With ONE key (L = 1) the softmax is the constant 1: the references of dQ, dK and of the map objective are identically zero, so
"relative to max |reference|" is undefined there; those are measured against the terms that cancel (`_grad_errs`, `denom`; measured <= 7.3e-7 / exactly 0).
The forward `geglu_il` does not saturate: an overflowing activation is +-inf, as in torch's fp16 (only gradients go through
`sat16`); the overflow case asserts exactly that for the forward and exact +-65504 for the backward.

Measured on the MI355X (largest of each group; 171 cases in 7 s; NO kernel had to change for these):
    attention backward   ragged sizes x every head dim 9.6e-4; split path 7.7e-4, second run bit-identical; dQ only / dK, dV only
                         1.1e-3, sentinels intact; sliced forms 6.5e-4, bit-equal to the contiguous call; ds_mul 1 / 1024 5.9e-4;
                         dO x 1 / 0.05 / 1e-3: 6.1e-4 / 5.9e-4 / 8.2e-4 (the reference rounded to fp16 alone: 2.8 .. 3.4e-4, so
                         1e-3 did not have to be raised); N = L = 4096 7.0e-4; lse <= 1.3e-3 absolute
                         peaked rows (one row's lse 89 log2 units above the median): dq 1.5e-3 dk 1.9e-3 dv 3.9e-3, lse 8.0e-3 --
                         inside 2e-2; fp64 with ONLY q * scale * log2e rounded to fp16 gives 7.6e-4 / 6.7e-4 / 2.9e-4, so that
                         rounding is a part of it and the kernel keeps its pre-scaled fp16 operand
                         dV past 65504 exactly +-65504 from the kernel's store and from the reducer, the others 6.7e-3 of 65504
                         `ief_attn_bwd_delta_f32` 1.1e-7
    GroupNorm backward   two-launch 4.0e-4, one-workgroup 4.2e-4 (inputs offset by 30: 3.3e-4); saturation exact in both forms
    LayerNorm backward   4.0e-4; rows offset by -20 .. +20 3.2e-4
    GEGLU                forward 2.9e-4, backward 3.2e-4 (|gate| to 15.0); overflow: backward exactly +-65504, forward +-inf
    pool2x2_sum          1 of 8,650,752 elements one ulp off the once-rounded fp64 sum, every other element bit-equal
    conv_out backward 4.4e-4; 3x3 data gradients at 8 x 12 5.3e-4; zero_insert2x bit-equal
    map objective        dq 2.9e-4; objective value 2.0e-9 .. 4.6e-8 (torch fp32 on the CPU 1.1e-8 .. 9.2e-8), exactly 0 at L = 1
    nti_loss_grad        objective 9.6e-7, gradient 1.5e-6; zero residual: d_eps and stats exactly zero; nti_adam 2.7e-7 absolute
"""
import math
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ief_amd import hip  # noqa: E402
from ief_amd.grad import UNetAdjoint  # noqa: E402

DEV = torch.device("cuda:0")
ADJ_TOL = 1e-2
ATTN_TOL = 2e-2
LSE_TOL = 2e-2
GEGLU_TOL = 2e-3
CONV_OUT_TOL = 2e-3
CONV3_TOL = 5e-3
DELTA_TOL = 1e-3
SENTINEL = 7.0
F16_MAX = 65504.0
LOG2E = 1.4426950408889634
IEF_EINVAL, IEF_ESHAPE, IEF_EALIGN = -1, -2, -3


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def h16(*shape, seed=0, scale=1.0, shift=0.0):
    """fp16 on the CPU: a seeded fp32 gaussian, scaled and shifted, rounded once"""
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).half()


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return None if t is None else t.to(DEV)


def check_saturating(got, ref, tol, label):
    """`got` (fp16, through sat16 / sat_half) against an fp64 reference that leaves the fp16 range"""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert torch.isfinite(got).all() and got.abs().max().item() <= F16_MAX
    a = ref.abs()
    sat = a > F16_MAX
    band = (a >= (1 - 1e-2) * F16_MAX) & (a <= (1 + 1e-2) * F16_MAX)
    hard = sat & ~band
    nsat, nband = int(sat.sum()), int(band.sum())
    assert nsat >= 100 and nband < 0.01 * nsat, (nsat, nband)
    exact = torch.equal(got[hard], torch.sign(ref[hard]) * F16_MAX)
    rest = ~sat & ~band
    e = ((got - ref)[rest].abs().max() / F16_MAX).item()
    print(f"{label}: {nsat} of {ref.numel()} elements past 65504 ({nband} within 1 % of it, exempt), exactly +-65504 there: {exact}; "
          f"the others {e:.2e} of 65504")
    assert exact and e < tol


# ------------------------------------------------------------------------------------------------ 1. attention backward
class AttnCase:
    """fp16 operands (CPU) of one attention layer and its fp64 graph; gradients for any dO by `grads`"""

    def __init__(self, d, heads, B, N, L, q=None, k=None, v=None, scale=None):
        C = heads * d
        self.d, self.heads, self.B, self.N, self.L, self.C = d, heads, B, N, L, C
        self.q = h16(B, N, C, seed=1) if q is None else q
        self.k = h16(B, L, C, seed=2) if k is None else k
        self.v = h16(B, L, C, seed=3) if v is None else v
        self.scale = d ** -0.5 if scale is None else scale
        self.qf, self.kf, self.vf = (t.double().requires_grad_(True) for t in (self.q, self.k, self.v))
        sc = self.heads_of(self.qf, N) @ self.heads_of(self.kf, L).transpose(-1, -2) * self.scale
        self.out = (torch.softmax(sc, -1) @ self.heads_of(self.vf, L)).transpose(1, 2).reshape(B, N, C)
        self.lse2 = torch.logsumexp(sc.detach(), -1) * LOG2E                      # [B, heads, N], log2 units

    def heads_of(self, t, n):
        return t.reshape(self.B, n, self.heads, self.d).transpose(1, 2)

    def do(self, mul=0.05):
        return h16(self.B, self.N, self.C, seed=4, scale=mul)

    def grads(self, do16):
        return torch.autograd.grad(self.out, (self.qf, self.kf, self.vf), do16.double(), retain_graph=True)


def _forward(case, q, k, v):
    """`o` and `lse` as the real run has them: from `hip.attn_flash(..., lse=...)`; lse held to fp64"""
    lse = torch.full((case.B, case.heads, case.N), float("nan"), dtype=torch.float32, device=DEV)
    o = hip.attn_flash(q, k, v, case.heads, case.scale, lse=lse)
    e_lse = (lse.double().cpu() - case.lse2).abs().max().item()
    assert e_lse < LSE_TOL, f"lse off by {e_lse:.2e}"
    return o, lse, e_lse


def _bwd(case, do16, fwd=None, with_dv=True, **kw):
    q, k, v = dev(case.q), dev(case.k), dev(case.v)
    o, lse, e_lse = fwd if fwd is not None else _forward(case, q, k, v)
    got = hip.attn_bwd(q, k, v, o, dev(do16), lse, case.heads, case.scale, **kw)
    return _grad_errs(case, do16, got, with_dv), got, e_lse


def _grad_errs(case, do16, got, with_dv=True):
    """error of (dq, dk, dv) relative to max |reference|.  With ONE key the softmax is the constant 1: dS = P (dP - delta)
    cancels exactly and the references of dQ and dK are identically zero, so there the error is taken relative to the terms
    that cancel, scale max |dP| max |K| for dQ and scale max |dP| max |Q| for dK (dP = dO V^T), not to zero"""
    refs = case.grads(do16)
    if case.L > 1:
        return [rel_err(g, r) for g, r in zip(got, refs)]
    assert refs[0].abs().max() == 0 and refs[1].abs().max() == 0
    dp = (case.heads_of(do16.double(), case.N) @ case.heads_of(case.v.double(), 1).transpose(-1, -2)).abs().max().item()
    errs = []
    for g, other in zip(got[:2], (case.k, case.q)):
        assert torch.isfinite(g).all()
        errs.append(g.double().abs().max().item() / (case.scale * dp * other.double().abs().max().item()))
    return errs + ([rel_err(got[2], refs[2])] if with_dv else [])


def _kv_splits(B, heads, N, L):
    """the query-split policy of `hip.attn_bwd`, restated: (splits, 64-row tiles, tiles per split)"""
    blocks, tiles = ((L + 127) // 128) * heads * B, (N + 63) // 64
    splits = max(1, min(tiles // 2, 256 // blocks)) if blocks < 128 and tiles >= 4 else 1
    return splits, tiles, (tiles + splits - 1) // splits


@pytest.mark.parametrize("B,heads,N,L", [(1, 1, 1, 1), (3, 2, 63, 65), (1, 2, 65, 129), (2, 1, 129, 1), (1, 3, 200, 77)])
@pytest.mark.parametrize("d", [32, 40, 64, 80, 160])
def test_attn_bwd_f16_ragged(d, B, heads, N, L):
    """one query / one key, one short of and one past a 64-row tile and a 128-column block, three images, every head dim"""
    case = AttnCase(d, heads, B, N, L)
    errs, _, e_lse = _bwd(case, case.do())
    print(f"attn_bwd fp16 ragged d={d} B={B} h={heads} N={N} L={L}: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e} lse {e_lse:.2e}")
    assert max(errs) < ATTN_TOL


@pytest.mark.parametrize("d,heads,B,N,L,empty_tail,past_reduce_cap", [
    (40, 2, 1, 576, 77, True, False),        # the 24 x 24 cross-attention: nine tiles in four splits of three, the last one empty
    (80, 1, 1, 320, 96, False, False),       # five tiles in two splits: three and two
    (160, 3, 1, 256, 5376, False, True)])    # 645,120 float4 for the reducer: past 2048 workgroups of 256
def test_attn_bwd_f16_split_path(d, heads, B, N, L, empty_tail, past_reduce_cap):
    """the query-split dK / dV path with `attn_bwd_reduce_kernel`; run twice: bit-identical (fixed summation order, no atomics)"""
    splits, tiles, tps = _kv_splits(B, heads, N, L)
    assert splits > 1, "the launch policy no longer splits this shape"
    assert ((splits - 1) * tps >= tiles) == empty_tail          # the last split starts past the last tile
    assert (B * L * heads * d // 4 > 2048 * 256) == past_reduce_cap
    case = AttnCase(d, heads, B, N, L)
    do16 = case.do()
    q, k, v = dev(case.q), dev(case.k), dev(case.v)
    fwd = _forward(case, q, k, v)
    errs, got, e_lse = _bwd(case, do16, fwd)
    _, again, _ = _bwd(case, do16, fwd)
    same = all(torch.equal(a, b) for a, b in zip(got, again))
    print(f"attn_bwd fp16 split d={d} h={heads} B={B} N={N} L={L} ({splits} splits of {tps} tiles over {tiles}): dq {errs[0]:.2e} "
          f"dk {errs[1]:.2e} dv {errs[2]:.2e} lse {e_lse:.2e}; second run bit-identical: {same}")
    assert max(errs) < ATTN_TOL and same


@pytest.mark.parametrize("d,heads,B,N,L", [(40, 2, 1, 576, 77), (64, 2, 3, 130, 130)])
def test_attn_bwd_f16_unrequested_outputs_untouched(d, heads, B, N, L):
    """`want_dq=False` (grad.py's stop at the frozen context) and `want_dkv=False` (Pix2Pix-zero): what is asked for is right, the
    other destinations and the columns between the slices keep their sentinel; the split and the single-launch dK / dV path"""
    case = AttnCase(d, heads, B, N, L)
    C = case.C
    do16 = case.do()
    refs = case.grads(do16)
    q, k, v = dev(case.q), dev(case.k), dev(case.v)
    o, lse, _ = _forward(case, q, k, v)
    for want_dq, want_dkv in ((True, True), (False, True), (True, False)):
        gq = torch.full((B, N, 2 * C), SENTINEL, dtype=torch.float16, device=DEV)
        gkv = torch.full((B, L, 3 * C), SENTINEL, dtype=torch.float16, device=DEV)
        dq, dk, dv = gq[..., C:], gkv[..., :C], gkv[..., 2 * C:]
        hip.attn_bwd(q, k, v, o, dev(do16), lse, heads, case.scale, dq=dq, dk=dk, dv=dv, want_dq=want_dq, want_dkv=want_dkv)
        errs = {}
        if want_dq:
            errs["dq"] = rel_err(dq, refs[0])
        else:
            assert (dq == SENTINEL).all(), "dQ was written although it was not requested"
        if want_dkv:
            errs["dk"], errs["dv"] = rel_err(dk, refs[1]), rel_err(dv, refs[2])
        else:
            assert (dk == SENTINEL).all() and (dv == SENTINEL).all(), "dK / dV were written although they were not requested"
        assert (gq[..., :C] == SENTINEL).all() and (gkv[..., C:2 * C] == SENTINEL).all()
        print(f"attn_bwd fp16 d={d} h={heads} B={B} N={N} L={L} want_dq={want_dq} want_dkv={want_dkv}: "
              + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
        assert max(errs.values()) < ATTN_TOL


def test_attn_bwd_f16_fused_qkv_slices():
    """the self-attention form of grad.py: q | k | v are column slices of one [B, N, 3C] projection and dq | dk | dv slices of one
    `dqkv` -- bit-equal to the contiguous call, and right"""
    d, heads, B, N = 40, 2, 2, 200
    case = AttnCase(d, heads, B, N, N)
    C = case.C
    do16 = case.do()
    qkv = dev(torch.cat([case.q, case.k, case.v], -1))
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    o, lse, _ = _forward(case, q, k, v)
    dqkv = torch.full((B, N, 3 * C), SENTINEL, dtype=torch.float16, device=DEV)
    hip.attn_bwd(q, k, v, o, dev(do16), lse, heads, case.scale, dq=dqkv[..., :C], dk=dqkv[..., C:2 * C], dv=dqkv[..., 2 * C:])
    plain = hip.attn_bwd(q.contiguous(), k.contiguous(), v.contiguous(), o, dev(do16), lse, heads, case.scale)
    sliced = (dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:])
    errs = [rel_err(g, r) for g, r in zip(sliced, case.grads(do16))]
    same = all(torch.equal(a, b) for a, b in zip(sliced, plain))
    print(f"attn_bwd fp16 fused-QKV slices: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}; bit-equal to contiguous: {same}")
    assert same and max(errs) < ATTN_TOL


def test_attn_bwd_f16_cross_slices():
    """the cross-attention form: k | v are slices of the [B, L, 4C] projection of every layer's context, dk | dv go into a
    zero-filled buffer of that width, dq into a slice of a sentinel-filled one; the split path (576 queries, 77 keys)"""
    d, heads, B, N, L = 40, 2, 1, 576, 77
    assert _kv_splits(B, heads, N, L)[0] > 1
    case = AttnCase(d, heads, B, N, L)
    C = case.C
    do16 = case.do()
    kv = dev(torch.cat([h16(B, L, C, seed=8), case.k, h16(B, L, C, seed=9), case.v], -1))
    q, k, v = dev(case.q), kv[..., C:2 * C], kv[..., 3 * C:]
    o, lse, _ = _forward(case, q, k, v)
    wide = torch.zeros(B, L, 4 * C, dtype=torch.float16, device=DEV)
    gq = torch.full((B, N, 2 * C), SENTINEL, dtype=torch.float16, device=DEV)
    hip.attn_bwd(q, k, v, o, dev(do16), lse, heads, case.scale, dq=gq[..., C:], dk=wide[..., C:2 * C], dv=wide[..., 3 * C:])
    plain = hip.attn_bwd(q, k.contiguous(), v.contiguous(), o, dev(do16), lse, heads, case.scale)
    sliced = (gq[..., C:], wide[..., C:2 * C], wide[..., 3 * C:])
    errs = [rel_err(g, r) for g, r in zip(sliced, case.grads(do16))]
    same = all(torch.equal(a, b) for a, b in zip(sliced, plain))
    print(f"attn_bwd fp16 cross slices: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}; bit-equal to contiguous: {same}")
    assert same and max(errs) < ATTN_TOL
    assert wide[..., :C].abs().max() == 0 and wide[..., 2 * C:3 * C].abs().max() == 0 and (gq[..., :C] == SENTINEL).all()


def test_attn_bwd_f16_do_magnitudes():
    """dO at 1, 0.05 and 1e-3 of unit scale.  A magnitude counts only if fp16 itself can hold the gradients: the fp64 reference
    rounded once to fp16 must be within a quarter of the tolerance of the unrounded one (asserted on the CPU); the smallest
    magnitude is raised until that holds and the value used is printed"""
    d, heads, B, N, L = 40, 2, 2, 320, 320
    case = AttnCase(d, heads, B, N, L)
    q, k, v = dev(case.q), dev(case.k), dev(case.v)
    fwd = _forward(case, q, k, v)
    representable = lambda mul: max(rel_err(r.half(), r) for r in case.grads(case.do(mul)))
    smallest = next(m for m in (1e-3, 2e-3, 5e-3, 1e-2) if representable(m) < ATTN_TOL / 4)
    for mul in (1.0, 0.05, smallest):
        floor16 = representable(mul)
        assert floor16 < ATTN_TOL / 4
        errs, _, _ = _bwd(case, case.do(mul), fwd)
        print(f"attn_bwd fp16 dO x {mul:g}: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e} (fp16 rounding of the reference alone: "
              f"{floor16:.2e})")
        assert max(errs) < ATTN_TOL


@pytest.mark.parametrize("ds_mul", [1.0, 1024.0])
def test_attn_bwd_f16_explicit_ds_mul(ds_mul):
    """dS * ds_mul is what gets packed into fp16 (the default is min(L, 1024)): both ends stay within tolerance"""
    d, heads, B, N, L = 40, 2, 2, 320, 320
    case = AttnCase(d, heads, B, N, L)
    errs, _, _ = _bwd(case, case.do(), ds_mul=ds_mul)
    print(f"attn_bwd fp16 ds_mul={ds_mul:g}: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}")
    assert max(errs) < ATTN_TOL


def test_attn_bwd_f16_peaked_rows():
    """the inputs of `test_attn_flash_peaky_rows`: one key per 64-key tile dominates query 5, rising tile by tile to ~100 log2
    units.  The kernel rounds q * scale * log2e to fp16 before the MFMA; an fp64 evaluation that applies ONLY that rounding is
    printed next to the kernel's error"""
    B, heads, N, d, L = 1, 2, 128, 64, 512
    C = heads * d
    q, k, v = h16(B, N, C, seed=1), h16(B, L, C, seed=2), h16(B, L, C, seed=3)
    for t in range(L // 64):
        k[0, 64 * t + 7, :] = q[0, 5, :] * (0.5 + 0.25 * t)
    case = AttnCase(d, heads, B, N, L, q, k, v, scale=d ** -0.5 * 4.0)
    do16 = case.do()
    refs = case.grads(do16)
    lead = (case.lse2.max() - case.lse2.median()).item()
    assert lead > 20.0                                                    # tens of log2 units between the peaked row and the rest
    errs, _, e_lse = _bwd(case, do16)
    # fp64 with q * scale * log2e rounded to fp16 (the factor formed in fp32, as the kernel forms it), nothing else rounded
    with torch.no_grad():
        sc32 = (torch.tensor(case.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
        q1 = (q.float() * sc32).half().double()
        qd, kd, vd, dod = q.double(), k.double(), v.double(), do16.double()
        s2 = case.heads_of(q1, N) @ case.heads_of(kd, L).transpose(-1, -2)
        P = torch.softmax(s2 * math.log(2.0), -1)
        dP = case.heads_of(dod, N) @ case.heads_of(vd, L).transpose(-1, -2)
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
        back = lambda t, n: t.transpose(1, 2).reshape(B, n, C)
        emul = (back(dS @ case.heads_of(kd, L), N) * case.scale, back(dS.transpose(-1, -2) @ case.heads_of(qd, N), L) * case.scale,
                back(P.transpose(-1, -2) @ case.heads_of(dod, N), L))
        e_emul = [rel_err(a, r) for a, r in zip(emul, refs)]
    print(f"attn_bwd fp16 peaked rows (largest row lse leads the median by {lead:.0f} log2 units): dq {errs[0]:.2e} dk {errs[1]:.2e} "
          f"dv {errs[2]:.2e} lse {e_lse:.2e}; fp64 with only q*scale*log2e rounded to fp16: dq {e_emul[0]:.2e} dk {e_emul[1]:.2e} "
          f"dv {e_emul[2]:.2e}")
    assert max(errs) < ATTN_TOL


def test_attn_bwd_f16_full_size():
    """N = L = 4096, the 64 x 64 level of SD-1.5, one head of 40: dQ, dK, dV against the fp64 gradients of one 4096^2 map"""
    case = AttnCase(40, 1, 1, 4096, 4096)
    errs, _, e_lse = _bwd(case, case.do())
    print(f"attn_bwd fp16 full size d=40 N=L=4096: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e} lse {e_lse:.2e}")
    assert max(errs) < ATTN_TOL


@pytest.mark.parametrize("N,split", [(129, False), (256, True)])
def test_attn_bwd_f16_dv_saturates(N, split):
    """`sat_half` in the kernel's own store and in `attn_bwd_reduce_kernel`: with one key dV = sum_n dO[n]; dO ~ 3e4 over 129 / 256
    queries puts most of it past 65504 -- exactly +-65504 there, finite everywhere (dQ, dK: identically zero references)"""
    d, heads, B, L = 40, 8, 3, 1
    assert (_kv_splits(B, heads, N, L)[0] > 1) == split
    case = AttnCase(d, heads, B, N, L)
    do16 = (f32(B, N, case.C, seed=4) * 3e4).clamp(-6e4, 6e4).half()
    errs, got, _ = _bwd(case, do16, with_dv=False)
    check_saturating(got[2], case.grads(do16)[2], ATTN_TOL, f"attn_bwd fp16 dV saturation N={N} ({'reducer' if split else 'single launch'})")
    print(f"    dq {errs[0]:.2e} dk {errs[1]:.2e} of the terms that cancel")
    assert max(errs) < ATTN_TOL


def test_attn_bwd_delta_f16_past_grid_cap_strided():
    """`ief_attn_bwd_delta_f32`: 532,870 rows (past 2048 workgroups of 256: the stride loop runs), O and dO column slices of
    buffers of DIFFERENT widths, both wider than heads * d"""
    B, heads, N, d = 1, 130, 4099, 8
    C = heads * d
    assert B * heads * N > 2048 * 256
    wo, wdo = h16(B, N, C + 8, seed=1), h16(B, N, C + 24, seed=2)
    od, dod = dev(wo)[..., 8:], dev(wdo)[..., 16:16 + C]
    assert od.stride(1) != dod.stride(1) and min(od.stride(1), dod.stride(1)) > C
    delta = torch.full((B, heads, N), float("nan"), dtype=torch.float32, device=DEV)
    rc = hip.load().ief_attn_bwd_delta_f32(od.data_ptr(), dod.data_ptr(), delta.data_ptr(), B, heads, N, d, od.stride(1),
                                           dod.stride(1), hip._stream())
    assert rc == 0
    ref = (wo[..., 8:].double() * wdo[..., 16:16 + C].double()).reshape(B, N, heads, d).sum(-1).transpose(1, 2)
    e = rel_err(delta, ref)
    print(f"attn_bwd_delta fp16 B={B} h={heads} N={N} d={d} ldo={od.stride(1)} lddo={dod.stride(1)}: {e:.2e}")
    assert e < DELTA_TOL


def test_attn_bwd_f16_refusals():
    """`ief_attn_bwd_f16` by its return code (argument checks only: nothing is launched, the destinations keep their sentinel)"""
    B, heads, N, L, d = 1, 2, 64, 64, 40
    C = heads * d
    W = C + 8
    bufs = [torch.zeros(B, n, W, dtype=torch.float16, device=DEV) for n in (N, L, L, N)]
    dst = [torch.full((B, n, W), SENTINEL, dtype=torch.float16, device=DEV) for n in (N, L, L)]
    lse, delta = (torch.zeros(B, heads, N, dtype=torch.float32, device=DEV) for _ in range(2))

    def call(what=3, **over):
        p = hip.IefAttnBwdParams()
        p.Q, p.K, p.V, p.dO = (t.data_ptr() for t in bufs)
        p.dQ, p.dK, p.dV = (t.data_ptr() for t in dst)
        p.lse, p.delta = lse.data_ptr(), delta.data_ptr()
        p.B, p.heads, p.N, p.L, p.d = B, heads, N, L, d
        p.ldq = p.ldk = p.ldv = p.ldo = p.lddq = p.lddk = p.lddv = W
        p.scale, p.ds_mul, p.kv_splits = d ** -0.5, 64.0, 0
        for name, val in over.items():
            setattr(p, name, val)
        return hip.load().ief_attn_bwd_f16(byref(p), what, hip._stream())

    assert call(ldq=C + 4) == IEF_EALIGN              # ldq % 8 != 0
    assert call(lddq=C + 2) == IEF_EALIGN             # lddq % 4 != 0
    assert call(heads=1, d=48) == IEF_ESHAPE          # no kernel for this head dim
    assert call(what=0) == IEF_ESHAPE
    assert call(ds_mul=0.0) == IEF_ESHAPE
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in dst)
    q = torch.zeros(B, N, C, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.attn_bwd(q, q, q, q, q, lse, heads, d ** -0.5, ds_mul=0.0)


# ------------------------------------------------------------------------------------------------ 2. GroupNorm backward
def _gn_two_launch(HW, C1, C2, G, stats):
    """the branch condition of `ief_groupnorm_bwd_f16`, restated: a change of it must not quietly move a case to the other form"""
    C = C1 + C2
    return stats and HW * (C // G) * 2 > 48 * 1024 and C1 % 8 == 0 and C2 % 8 == 0 and C <= 4096


def _gn_inputs(B, HW, C1, C2, G, shift=0.0, x_scale=1.0, dy_scale=0.1):
    C = C1 + C2
    x = h16(B, HW, C1, seed=1, scale=x_scale, shift=shift)
    x2 = h16(B, HW, C2, seed=2, scale=x_scale, shift=shift) if C2 else None
    dy = (f32(B, HW, C, seed=3) * dy_scale).clamp(-6e4, 6e4).half()
    add = h16(B, HW, C, seed=4, scale=0.1)
    gamma, beta = 1 + f32(C, seed=5, scale=0.1), f32(C, seed=6, scale=0.1)
    return x, x2, dy, add, gamma, beta


def _gn_ref(x, x2, dy, add, gamma, beta, G, silu):
    xin = (torch.cat([x, x2], -1) if x2 is not None else x).double().requires_grad_(True)
    y = F.group_norm(xin.transpose(1, 2), G, gamma.double(), beta.double(), 1e-5).transpose(1, 2)
    (F.silu(y) if silu else y).backward(dy.double())
    return xin.grad + (add.double() if add is not None else 0.0)


def _gn_stats(kind, x, x2, gamma, beta, G, silu):
    """`stats` [B, groups, 2] = (mean, rstd): the forward's own, or -- where the fp16 forward refuses the shape (C1 % 8 != 0) --
    torch's in fp64, rounded to fp32"""
    if kind is None:
        return None
    if kind == "fwd":
        return hip.groupnorm(dev(x), dev(gamma), dev(beta), G, 1e-5, silu=silu, x2=dev(x2), return_stats=True)[1]
    xin = (torch.cat([x, x2], -1) if x2 is not None else x).double()
    B, HW, C = xin.shape
    xg = xin.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    return dev(torch.stack([xg.mean(-1), (xg.var(-1, unbiased=False) + 1e-5).rsqrt()], -1).float().contiguous())


# (B, HW, C1, C2, groups, stats: "fwd" | "torch" | None, two-launch form expected, shift of the inputs)
GN_CASES = [
    (1, 413, 1280, 640, 32, "fwd", True, 0.0),       # ragged HW, 60 channels per group: chunks straddle groups; C8 = 240, PYs = 1
    (1, 333, 1280, 1280, 32, "fwd", True, 0.0),      # C8 = 320 > 256: 256 / C8 is zero before the clamp
    (2, 1000, 64, 0, 2, "fwd", True, 0.0),           # 62 splits of 17 pixels: splits 59 to 61 start past the end
    (1, 1024, 512, 0, 64, "fwd", False, 0.0),        # 64 groups; a 16 KiB slab: below the two-launch threshold (see the module docstring)
    (1, 4096, 512, 0, 64, "fwd", True, 0.0),         # 64 groups in the two-launch form: every lane of the first wave folds a group
    (1, 4096, 320, 0, 32, "fwd", True, 0.0),
    (3, 1, 64, 0, 32, None, False, 0.0),             # one pixel: HW < PY
    (2, 35, 36, 28, 32, None, False, 0.0),           # 2 channels per group, C1 % 8 != 0
    (2, 35, 36, 28, 32, "torch", False, 0.0),        # the same with stats given: must fall back
    (2, 16, 40, 24, 4, None, False, 0.0),            # group 2 (channels 32..47) straddles the two sources
    (1, 4096, 320, 0, 32, None, False, 0.0),         # the large slab streamed by one workgroup per (image, group)
    (2, 64, 320, 0, 32, None, False, 30.0),          # one-pass variance E[x^2] - mean^2 in fp32, 30 sigma from zero
]


@pytest.mark.parametrize("with_add", [True, False])
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("B,HW,C1,C2,G,stats_kind,two_launch,shift", GN_CASES)
def test_groupnorm_bwd_f16_forms(B, HW, C1, C2, G, stats_kind, two_launch, shift, silu, with_add):
    assert bool(_gn_two_launch(HW, C1, C2, G, stats_kind is not None)) == two_launch
    if two_launch:
        splits = hip.load().ief_gn_splits(HW)
        per = (HW + splits - 1) // splits
        empty = sum(1 for s in range(splits) if s * per >= HW)
        assert splits <= 64 and (empty == 3 if HW == 1000 else True), (splits, per, empty)
    x, x2, dy, add, gamma, beta = _gn_inputs(B, HW, C1, C2, G, shift=shift)
    add = add if with_add else None
    ref = _gn_ref(x, x2, dy, add, gamma, beta, G, silu)
    stats = _gn_stats(stats_kind, x, x2, gamma, beta, G, silu)
    got = hip.groupnorm_bwd(dev(x), dev(dy), dev(gamma), dev(beta), G, 1e-5, silu=silu, x2=dev(x2), add=dev(add), stats=stats)
    e = max(rel_err(got[0], ref[..., :C1]), rel_err(got[1], ref[..., C1:])) if C2 else rel_err(got, ref)
    print(f"groupnorm_bwd fp16 [{'two-launch' if two_launch else 'one-workgroup'}] B={B} HW={HW} C={C1}+{C2} G={G} stats={stats_kind} "
          f"shift={shift:g} silu={silu} add={with_add}: {e:.2e}")
    assert e < ADJ_TOL


def test_groupnorm_bwd_f16_refusals():
    def call(HW, C1, C2, G):
        x, x2, dy, _, gamma, beta = _gn_inputs(1, HW, C1, C2, 1)
        return hip.groupnorm_bwd(dev(x), dev(dy), dev(gamma), dev(beta), G, 1e-5, x2=dev(x2))

    for HW, C1, C2, G in ((16, 96, 0, 32),          # 3 channels per group
                          (16, 33, 31, 32),         # odd C1
                          (16, 130, 0, 65),         # 65 groups
                          (16, 100, 0, 32)):        # C % groups != 0
        with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
            call(HW, C1, C2, G)


@pytest.mark.parametrize("B,HW,C,G,stats_kind", [(2, 64, 320, 32, None), (1, 4096, 320, 32, "fwd")])
def test_groupnorm_bwd_f16_saturates(B, HW, C, G, stats_kind):
    """x at 0.03 sigma (rstd ~ 33) and dy ~ 2e4: |reference| ~ 6e5 -- both forms clamp to +-65504 exactly and stay finite"""
    x, _, dy, add, gamma, beta = _gn_inputs(B, HW, C, 0, G, x_scale=0.03, dy_scale=2e4)
    ref = _gn_ref(x, None, dy, add, gamma, beta, G, True)
    stats = _gn_stats(stats_kind, x, None, gamma, beta, G, True)
    assert bool(_gn_two_launch(HW, C, 0, G, stats is not None)) == (stats_kind is not None)
    got = hip.groupnorm_bwd(dev(x), dev(dy), dev(gamma), dev(beta), G, 1e-5, silu=True, add=dev(add), stats=stats)
    check_saturating(got, ref, ADJ_TOL, f"groupnorm_bwd fp16 saturation B={B} HW={HW} C={C} stats={stats_kind}")


# ------------------------------------------------------------------------------------------------ 3. LayerNorm backward
def _ln_ref(x, dy, add, gamma):
    xin = x.double().requires_grad_(True)
    C = x.shape[-1]
    F.layer_norm(xin, (C,), gamma.double(), torch.zeros(C, dtype=torch.float64), 1e-5).backward(dy.double())
    return xin.grad + (add.double() if add is not None else 0.0)


@pytest.mark.parametrize("with_add", [True, False])
@pytest.mark.parametrize("rows,C", [(1, 8), (5, 64), (301, 1280), (4099, 320), (7, 2048)])
def test_layernorm_bwd_f16_shapes(rows, C, with_add):
    """one wave per row, four rows per workgroup with an early return: a single row, rows % 4 != 0, C = 8 (one live lane), C = 2048
    (all four chunks of all 64 lanes), with and without `add`"""
    x, dy = h16(rows, C, seed=1, scale=3.0, shift=1.0), h16(rows, C, seed=2, scale=0.1)
    add = h16(rows, C, seed=3, scale=0.1) if with_add else None
    gamma = 1 + f32(C, seed=5, scale=0.1)
    e = rel_err(hip.layernorm_bwd(dev(x), dev(dy), dev(gamma), 1e-5, add=dev(add)), _ln_ref(x, dy, add, gamma))
    print(f"layernorm_bwd fp16 rows={rows} C={C} add={with_add}: {e:.2e}")
    assert e < ADJ_TOL


def test_layernorm_bwd_f16_offset_rows():
    """every row offset by its own constant between -20 and +20 (spacing of fp16 there: 2^-6)"""
    rows, C = 301, 1280
    x = (f32(rows, C, seed=1) + torch.linspace(-20.0, 20.0, rows)[:, None]).half()
    dy, add = h16(rows, C, seed=2, scale=0.1), h16(rows, C, seed=3, scale=0.1)
    gamma = 1 + f32(C, seed=5, scale=0.1)
    e = rel_err(hip.layernorm_bwd(dev(x), dev(dy), dev(gamma), 1e-5, add=dev(add)), _ln_ref(x, dy, add, gamma))
    print(f"layernorm_bwd fp16 rows={rows} C={C}, rows offset by -20 .. +20: {e:.2e}")
    assert e < ADJ_TOL


@pytest.mark.parametrize("C", [100, 2056])
def test_layernorm_bwd_f16_refusals(C):
    x = torch.zeros(4, C, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.layernorm_bwd(x, x, torch.ones(C, device=DEV))


# ------------------------------------------------------------------------------------------------ 4. GEGLU (interleaved)
def _geglu_ref(pre, dy, rows, Ch):
    p = pre.double().reshape(rows, Ch // 8, 2, 8).requires_grad_(True)
    out = (p[:, :, 0] * F.gelu(p[:, :, 1])).reshape(rows, Ch)
    out.backward(dy.double())
    return out.detach(), p.grad.reshape(rows, 2 * Ch)


@pytest.mark.parametrize("rows,Ch,gate_mul", [(8195, 1280, 1.0),      # 1,311,200 chunks: past 4096 workgroups of 256, ragged tail
                                              (1, 8, 1.0), (300, 640, 1.0),
                                              (300, 640, 3.0)])       # |gate| to ~12: erf saturated, exp(-g^2 / 2) underflows
def test_geglu_il_f16_fwd_bwd(rows, Ch, gate_mul):
    pre = f32(rows, 2 * Ch, seed=1).reshape(rows, Ch // 8, 2, 8)
    pre[:, :, 1] *= gate_mul
    gmax = pre[:, :, 1].abs().max().item()
    assert gate_mul == 1.0 or gmax > 11.5
    pre, dy = pre.reshape(rows, 2 * Ch).half(), h16(rows, Ch, seed=2, scale=0.1)
    ref_out, ref_dpre = _geglu_ref(pre, dy, rows, Ch)
    e_f, e_b = rel_err(hip.geglu_il(dev(pre)), ref_out), rel_err(hip.geglu_il_bwd(dev(pre), dev(dy)), ref_dpre)
    print(f"geglu_il fp16 rows={rows} Ch={Ch} (max |gate| {gmax:.1f}): forward {e_f:.2e} backward {e_b:.2e}")
    assert e_f < GEGLU_TOL and e_b < GEGLU_TOL


def test_geglu_il_f16_overflow():
    """hidden ~ 2000, gate ~ 10, dy ~ 1e4.  The backward goes through sat16: exactly +-65504 where the gradient leaves fp16.  The
    forward is an activation and does not saturate: past the range it is +-inf with the reference's sign, as torch's fp16"""
    rows, Ch = 300, 640
    pre = f32(rows, 2 * Ch, seed=1).reshape(rows, Ch // 8, 2, 8)
    pre[:, :, 0] *= 2000.0
    pre[:, :, 1] *= 10.0
    pre = pre.reshape(rows, 2 * Ch).half()
    dy = (f32(rows, Ch, seed=2) * 1e4).clamp(-6e4, 6e4).half()
    ref_out, ref_dpre = _geglu_ref(pre, dy, rows, Ch)
    check_saturating(hip.geglu_il_bwd(dev(pre), dev(dy)), ref_dpre, GEGLU_TOL, "geglu_il_bwd fp16 saturation")
    out = hip.geglu_il(dev(pre)).double().cpu()
    over, under = ref_out.abs() > 1.01 * F16_MAX, ref_out.abs() < 0.99 * F16_MAX
    assert over.sum() >= 100 and not torch.isnan(out).any()
    inf_ok = torch.equal(out[over], torch.sign(ref_out[over]) * float("inf"))
    e = ((out - ref_out)[under].abs().max() / F16_MAX).item()
    print(f"geglu_il fp16 overflow: {int(over.sum())} elements past 65504 are +-inf of the right sign: {inf_ok}; the others {e:.2e} of 65504")
    assert inf_ok and e < GEGLU_TOL


# ------------------------------------------------------------------------------------------------ 5. resampling, conv_out, 3x3
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (3, 5, 7, 24), (2, 64, 64, 320)])
def test_zero_insert2x_f16_bit_equal(B, H, W, C):
    """the last size is 5120 workgroups' worth of 16-byte chunks: past the 4096-workgroup cap, the grid-stride term runs"""
    x = h16(B, H, W, C, seed=1)
    want = torch.zeros(B, 2 * H, 2 * W, C, dtype=torch.float16)
    want[:, ::2, ::2] = x
    got = hip.zero_insert2x(dev(x)).cpu()
    print(f"zero_insert2x fp16 {B}x{H}x{W}x{C}: bit-equal {torch.equal(got, want)}")
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (3, 5, 7, 24), (2, 128, 132, 256)])
def test_pool2x2_sum_f16(B, H, W, C):
    """output sizes; the last one is 4224 workgroups' worth of chunks.  Against the fp64 sum rounded once to fp16, +- one ulp"""
    x = h16(B, 2 * H, 2 * W, C, seed=1)
    xd = x.double()
    ref16 = (xd[:, ::2, ::2] + xd[:, ::2, 1::2] + xd[:, 1::2, ::2] + xd[:, 1::2, 1::2]).half().double()
    got = hip.pool2x2_sum(dev(x)).double().cpu()
    ulp = torch.pow(2.0, torch.floor(torch.log2(ref16.abs().clamp_min(2.0 ** -14))) - 10)
    off = (got - ref16).abs()
    print(f"pool2x2_sum fp16 -> {B}x{H}x{W}x{C}: {int((off > 0).sum())} of {ref16.numel()} elements differ from the once-rounded sum, "
          f"the largest by {(off / ulp).max().item():.1f} ulp")
    assert torch.isfinite(got).all() and (off <= ulp).all()


@pytest.mark.parametrize("B,C,H,W,Cout", [(3, 320, 8, 12, 4), (1, 8, 1, 7, 16), (1, 8, 5, 1, 3), (2, 320, 128, 128, 4)])
def test_conv_out_bwd_f16_nonsquare(B, C, H, W, Cout):
    """H != W, one row, one column, the most output channels; the last size is 5120 workgroups' worth of chunks"""
    w = h16(Cout, C, 3, 3, seed=2, scale=(9 * C) ** -0.5)
    x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    de = f32(B, Cout, H, W, seed=3)
    F.conv2d(x, w.double(), padding=1).backward(de.double())
    got = hip.conv_out_bwd(dev(de), dev(w.permute(0, 2, 3, 1).contiguous()))
    e = rel_err(got.permute(0, 3, 1, 2), x.grad)
    print(f"conv_out_bwd fp16 B={B} C={C} {H}x{W} Cout={Cout}: {e:.2e}")
    assert e < CONV_OUT_TOL


def test_conv_out_bwd_f16_refuses_17_channels():
    de = torch.zeros(1, 17, 4, 4, device=DEV)
    w = torch.zeros(17, 3, 3, 8, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.conv_out_bwd(de, w)


@pytest.mark.parametrize("mode", ["plain", "stride2", "upsample"])
def test_conv3x3_data_gradient_f16_nonsquare(mode):
    """the 3x3 data gradients as grad.py forms them (`UNetAdjoint.wt_conv`) on an 8 x 12 image: a swap of H and W cannot hide"""
    B, Cin, Cout, H, W = 3, 128, 64, 8, 12
    x, w = h16(B, Cin, H, W, seed=1), h16(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    xi = x.double().requires_grad_(True)
    if mode == "plain":
        y = F.conv2d(xi, w.double(), padding=1)
    elif mode == "stride2":
        y = F.conv2d(xi, w.double(), padding=1, stride=2)
    else:
        y = F.conv2d(F.interpolate(xi, scale_factor=2.0, mode="nearest"), w.double(), padding=1)
    dy = h16(*y.shape, seed=3, scale=0.1)
    y.backward(dy.double())
    adj = UNetAdjoint.__new__(UNetAdjoint)
    adj._wt = {}
    wt = adj.wt_conv(dev(nhwc(w)))
    dd = dev(nhwc(dy))
    got = hip.conv3x3(dd, wt) if mode == "plain" else hip.conv3x3(hip.zero_insert2x(dd), wt) if mode == "stride2" \
        else hip.pool2x2_sum(hip.conv3x3(dd, wt))
    e = rel_err(got.permute(0, 3, 1, 2), xi.grad)
    print(f"conv data gradient fp16 [{mode}] {H}x{W}: {e:.2e}")
    assert e < CONV3_TOL


# ------------------------------------------------------------------------------------------------ 6. Pix2Pix-zero map objective
def _map_objective(q, k, ref, B, heads, N, L, d, scale, dt):
    qf = q.to(dt).requires_grad_(True)
    sp = lambda t, n: t.reshape(B, n, heads, d).transpose(1, 2).reshape(B * heads, n, d)
    P = torch.softmax(sp(qf, N) @ sp(k.to(dt), L).transpose(1, 2) * scale, -1)
    loss = ((P - ref.to(dt)) ** 2).sum((1, 2)).mean(0)
    loss.backward()
    return loss.detach(), qf.grad


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("with_loss", [True, False])
@pytest.mark.parametrize("acc", [True, False])
@pytest.mark.parametrize("B,heads,N,L,d", [(1, 1, 1, 77, 40),        # one query: 255 dead lanes shadow it
                                           (2, 3, 65, 1, 32),        # one key
                                           (1, 2, 300, 96, 80),      # L at the limit, two lanes per query, three workgroups
                                           (2, 1, 63, 77, 160),      # four lanes per query, N*G = 252 < 256
                                           (1, 2, 130, 40, 64)])     # 32-wide chunks, N*G = 260: a second workgroup of four lanes
def test_map_loss_f16_vs_fp64(B, heads, N, L, d, acc, with_loss, strided):
    """`hip.attn_map_loss_bwd` on fp16 q / k / dq and fp16 reference maps: dq and the summed objective against fp64 autograd; q and
    dq as column slices of wider buffers and k as a slice of a [B, L, 4C] projection when `strided`"""
    C = heads * d
    q, k = h16(B, N, C, seed=1), h16(B, L, C, seed=2)
    ref = torch.softmax(f32(B * heads, N, L, seed=3, scale=2.0), -1).half()
    dq0 = h16(B, N, C, seed=4, scale=0.01)
    scale, gs = d ** -0.5, 64.0
    loss64, grad64 = _map_objective(q, k, ref, B, heads, N, L, d, scale, torch.float64)
    want = grad64 * gs + (dq0.double() if acc else 0.0)
    nblk = hip.map_loss_blocks(N, d)
    assert nblk == (N * (d // (40 if d % 40 == 0 else 32)) + 255) // 256
    parts = torch.full((B * heads * nblk + 3,), SENTINEL, device=DEV) if with_loss else None
    if strided:
        qw = torch.full((B, N, 2 * C), SENTINEL, dtype=torch.float16, device=DEV)
        kw = torch.full((B, L, 4 * C), SENTINEL, dtype=torch.float16, device=DEV)
        dqw = torch.full((B, N, 3 * C), SENTINEL, dtype=torch.float16, device=DEV)
        qd, kd, dq = qw[..., C:], kw[..., C:2 * C], dqw[..., C:2 * C]
        qd.copy_(q), kd.copy_(k), dq.copy_(dq0)
    else:
        qd, kd, dq = dev(q), dev(k), dev(dq0.clone())
    hip.attn_map_loss_bwd(qd, kd, dev(ref), dq, heads, scale, gcoef=2.0 * gs / (B * heads), accumulate=acc, loss=parts,
                          loss_coef=1.0 / (B * heads))
    e = rel_err(dq, want)
    if strided:
        assert (dqw[..., :C] == SENTINEL).all() and (dqw[..., 2 * C:] == SENTINEL).all()
    label = f"map objective fp16 B={B} h={heads} N={N} L={L} d={d} acc={acc} strided={strided}"
    if not with_loss:
        print(f"{label} loss=None: dq {e:.2e}")
        assert e < ADJ_TOL
        return
    assert (parts[B * heads * nblk:] == SENTINEL).all()                  # nothing written past the last partial
    loss32, _ = _map_objective(q, k, ref, B, heads, N, L, d, scale, torch.float32)
    # one key: P = ref = 1 and the objective is exactly zero -- measured against the N unit terms per map that cancel instead
    denom = loss64.item() if L > 1 else float(N)
    assert denom > 0 and (L > 1 or loss64.item() == 0)
    floor32 = abs(loss32.item() - loss64.item()) / denom
    el = abs(parts[:B * heads * nblk].double().sum().item() - loss64.item()) / denom
    bound = max(4.0 * floor32, 1e-3)
    print(f"{label}: dq {e:.2e}, objective {el:.2e} (torch fp32 on the CPU: {floor32:.2e}, bound {bound:.2e})")
    assert e < ADJ_TOL and el <= bound


def test_map_loss_f16_refusals():
    B, heads, N, d = 1, 2, 16, 40
    C = heads * d
    q = torch.zeros(B, N, C, dtype=torch.float16, device=DEV)
    k97 = torch.zeros(B, 97, C, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.attn_map_loss_bwd(q, k97, torch.zeros(B * heads, N, 97, dtype=torch.float16, device=DEV), q.clone(), heads, d ** -0.5, 1.0)
    k = torch.zeros(B, 77, C, dtype=torch.float16, device=DEV)
    ref = torch.zeros(B * heads, N, 77, dtype=torch.float16, device=DEV)
    q_odd = torch.zeros(B, N, C + 4, dtype=torch.float16, device=DEV)[..., :C]          # ldq = C + 4: no multiple of 8
    with pytest.raises(RuntimeError, match="IEF_EALIGN"):
        hip.attn_map_loss_bwd(q_odd, k, ref, q.clone(), heads, d ** -0.5, 1.0)


# ------------------------------------------------------------------------------------------------ 7. NTI objective, Adam
def _nti_inputs(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for _ in range(4)]


@pytest.mark.parametrize("n", [100, 16384])
def test_nti_loss_grad_vs_fp64(n):
    """fewer elements than the workgroup's 1024-thread stride, and sixteen strides; tolerances of
    `test_nti_loss_grad_and_adam_vs_torch`"""
    eu, ec, x, tgt = _nti_inputs(n)
    a_f, a_t, gs, grad_scale = 0.31, 0.42, 7.5, 4.0
    coef = torch.tensor([a_f, a_t, gs, 0.0])
    d_eps, stats = torch.full((n,), float("nan"), device=DEV), torch.zeros(2, device=DEV)
    hip.nti_loss_grad(dev(eu), dev(ec), dev(x), dev(tgt), dev(coef), d_eps, stats, grad_scale)
    c = coef.double()
    eur = eu.double().requires_grad_(True)
    e = eur + c[2] * (ec.double() - eur)
    rec = c[1].sqrt() * (x.double() - (1 - c[0]).sqrt() * e) / c[0].sqrt() + (1 - c[1]).sqrt() * e
    loss = F.mse_loss(rec, tgt.double())
    loss.backward()
    e_loss = abs(stats[0].item() - loss.item()) / loss.item()
    e_max = abs(d_eps.abs().max().item() - grad_scale) / grad_scale
    e_grad = rel_err(d_eps.double() * stats[1].double(), eur.grad)
    print(f"nti_loss_grad n={n}: objective {e_loss:.2e}, max |d_eps| off {e_max:.2e}, gradient {e_grad:.2e}")
    assert e_loss <= 1e-5 and e_max < 1e-5 and e_grad < 1e-5


@pytest.mark.parametrize("n", [100, 16384])
def test_nti_loss_grad_zero_residual(n):
    """`target` equal to the reconstruction: a_from = a_to = 0.25 and eps = 0 make the kernel's own reconstruction exactly x
    (0.5 (x / 0.5) + sqrt(0.75) 0), so the residual is exactly zero -- d_eps all zero, stats = (0, 0), nothing NaN"""
    _, _, x, _ = _nti_inputs(n)
    zero = torch.zeros(n, device=DEV)
    coef = torch.tensor([0.25, 0.25, 7.5, 0.0], device=DEV)
    d_eps, stats = torch.full((n,), float("nan"), device=DEV), torch.full((2,), float("nan"), device=DEV)
    hip.nti_loss_grad(zero, zero.clone(), dev(x), dev(x).clone(), coef, d_eps, stats, 4.0)
    print(f"nti_loss_grad n={n} zero residual: stats {stats.tolist()}, max |d_eps| {d_eps.abs().max().item()}")
    assert torch.equal(d_eps, torch.zeros_like(d_eps)) and stats[0].item() == 0.0 and stats[1].item() == 0.0


@pytest.mark.parametrize("n", [1, 257])
def test_nti_adam_f16_small(n):
    """one element, and one past a workgroup: five steps against torch.optim.Adam in fp64 fed the same fp16-stored gradients"""
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    p_ref = p0.double().requires_grad_(True)
    lr, factor = 7e-3, 3e-4
    opt = torch.optim.Adam([p_ref], lr=lr)
    param, m, v = dev(p0.clone()), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p16 = torch.empty(n, dtype=torch.float16, device=DEV)
    hyper = torch.tensor([lr, 0.9, 0.999, 1e-8], device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = torch.tensor([0.0, factor], device=DEV)
    for _ in range(5):
        g16 = (torch.randn(n, generator=g) * 2.0).half()
        hip.nti_adam(param, m, v, dev(g16), st, hyper, step, p16)
        p_ref.grad = g16.double() * float(st[1].item())
        opt.step()
    e = (param.double().cpu() - p_ref.detach()).abs().max().item()
    print(f"nti_adam n={n}: {e:.2e} absolute after five steps")
    assert step.item() == 5 and e < 1e-6 and torch.equal(p16, param.half())
