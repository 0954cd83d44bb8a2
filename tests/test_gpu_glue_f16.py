"""The forward glue kernels of the fp16-storage mode (`precision="f16"`), one by one, against fp64 at every branch of their dispatch
code on a real MI355X: GroupNorm in its four launch forms (one workgroup per (batch, group), the three launches, and the one-launch
and fold + apply forms on producer statistics), LayerNorm, GEGLU, `conv_in` / `conv_out`, add / SiLU / casts / row gather / row
softmax / transpose / step-table select past their grid caps, `pointwise_f32` and the timestep embedding.

tests/test_gpu_ops.py and tests/test_gpu_vae.py touch each of them at one or two friendly shapes against fp32 with bounds of about
1e-2 on a normalised output; this file holds every fp16 output to one fp16 ulp PER ELEMENT and adds the shapes at which the kernels
take another path.  None of these entry points reports the kernel it launched, so each case restates the branch condition of
`csrc/norm.hip` / `csrc/conv_io.hip` / `csrc/elementwise.hip`, asserts that the case takes the path it is listed for and names it.

Every reference is torch on the CPU in fp64, or exact bit / integer arithmetic, computed inside the test from exactly the
fp16-rounded (or fp32) inputs the kernel receives; no kernel of this library serves as a reference.  Bounds (every test prints what
it measured):
    fp16 outputs of near-centred inputs (GroupNorm, LayerNorm, GEGLU, SiLU, add, conv_in, softmax), per element:
        |got - ref64| <= ulp16(ref64) + F,   ulp16(r) = 2^(floor(log2 |r|) - 10), never below 2^-24 (the correctly rounded value or
        one neighbour),   F = max(4 x max |torch fp32 on the CPU - ref64|, 2^-24), measured in the test (4 covers another summation
        order and the hardware rsqrt / exp).  The number of elements that are not bit-equal to `ref64.half()` is printed, not asserted.
    GroupNorm on inputs far from zero (|mean| / std = 40 and 75, 0.2 < std < 1.5, |offset| <= 45, outputs of size ~3): the fp16 mode
        takes the variance as E[x^2] - mean^2 by design, so the ulp bound does not apply; the bounds of
        `test_groupnorm_from_producer_statistics_offset_activations` do: own statistics < 8e-3, producer statistics < 1.5e-2 absolute.
        LayerNorm is two-pass and keeps the ulp bound on rows offset by -20 .. +20 of their spreads.
    (mean, rstd) of `return_stats=True`: <= 1e-5 of the largest, near-centred inputs (the bound of `test_producer_column_statistics`)
    conv_out (fp32 out, fp16-pair dot products): <= 1e-4 max |ref| + 1e-5 (the bound of `test_conv_in_out`)
    pointwise_f32 (fp32; a term passes through at most Cin + 1 roundings, its product and the additions after it):
        <= (Cin + 1) 2^-24 (|bias| + sum |w| |x|) per element
    timestep embedding: <= 2e-3 absolute; the row of t = 0 exactly [1 .. 1 | 0 .. 0]
    casts, gather, transpose, select_step, every sentinel row behind an output, destinations of refused calls: bit-equal
    every GroupNorm form run twice: bit-identical

Where a case of the issue is run differently from how it is worded:
    conv_in's LDS refusal cannot be reached any more: with the slice search continued past the first divisor (see below) the
        smallest slice (8 channels, Cin = 8) needs 11.25 KiB; the shapes refused before, (1, 8, 4, 4, 256) and (1, 8, 4, 4, 512),
        are positive cases, and Cin = 9 / Cout = 12 are the refusals that remain.
    conv_out has no switch between its LDS kernels and the wide kernel for one shape; the two are compared on the same input by
        running Cout = 8 in one call (C = 344 and 384: 48.4 / 54 KiB of weights, the wide kernel) and as two calls of Cout = 4 on
        the halves of the same weights (`conv_out_kernel<3>`).
    the one-workgroup GroupNorm reads gamma / beta one float at a time, so a gamma 4 bytes off 16-byte alignment is legal there;
        that refusal is asserted on the forms that read 4 floats at a time.

Measured on the MI355X (largest of each group; F is the fp32 floor of the bound, `!=` the share of elements not bit-equal to
`ref64.half()`):
    every case inside its bound: no element of any fp16 output outside ulp16 + F.  Largest |err| - ulp16 (what F has to cover):
    GroupNorm, own statistics     one-workgroup +6.5e-8, three-launch +1.3e-7 (F 1.1e-6 .. 4.3e-6); != at most 0.09 %
    GroupNorm, producer statistics one-launch +7.2e-8, fold + apply +1.7e-7, own statistics on the same inputs +1.7e-7 (F 1.4e-6 ..
                                  4.3e-6); != at most 0.06 %; on conv3x3's own statistics (tile height 128, one-launch) -2.1e-8, F 3.2e-6
    GroupNorm far from zero       own statistics 1.9e-3 / 3.6e-3 (one-workgroup, mean / std 40 / 75) and 2.7e-3 / 5.6e-3 (three-launch)
                                  against 8e-3; producer statistics 2.0e-3 / 3.6e-3 (one-launch), 2.5e-3 / 4.4e-3 (fold + apply)
                                  against 1.5e-2
    returned (mean, rstd)         1.2e-7 / 1.1e-7 (one-workgroup), 7.3e-8 / 9.3e-8 (three-launch) against 1e-5
    every GroupNorm form twice    bit-identical, sentinel rows kept (all 56 pairs of runs)
    LayerNorm                     at most -2.6e-9 at the nine widths (F 3.5e-7 .. 3.8e-6, != at most 0.04 %); rows offset by
                                  -20 .. +20 spreads +8.0e-7 against F = 1.0e-5 (!= 0.22 %)
    GEGLU                         +5.9e-7 against F = 1.8e-5 past the grid cap (outputs up to 100; != 4.3 %: the fp32 erf cancels
                                  for gates below -3, where the products are tiny); one chunk: bit-equal; overflow: +-inf exactly
    SiLU -3.0e-8 (F 3.9e-6, != 0.01 %), add: bit-equal to the rounded fp64 sum at both sizes, softmax -3.0e-8 (F <= 6.4e-7, != at
    most 0.03 %; row sums of the fp16 result 0.99988 .. 1.00021)
    conv_in                       +2.5e-8 (F 1.3e-7 .. 6.7e-6, != at most 0.08 %), the two shapes refused before included
    conv_out                      1.1e-6 absolute at most against bounds of 2.4e-5 .. 3.4e-4; wide kernel against conv_out_kernel<3>
                                  on the same input 1.0e-6
    pointwise_f32 0.30 of its bound; timestep embedding 2.8e-4 absolute, the row of t = 0 exact
    casts (values past 65504 included), gather, transpose, select_step, sentinels, destinations of refused calls: bit-equal
    the whole file                3.9 s (135 tests), library load included
No kernel had to change for these.  Two host-side changes came with this file.  `ief_conv_in_f32` stopped its slice search at the
first divisor of Cout and then refused (1, 8, 4, 4, 256) and (1, 8, 4, 4, 512) for 81 KiB of LDS; it now goes on to the first slicing
that fits 64 KiB (two and four slices of 128).  The alignment guards of section 8 are new: before, `ief_groupnorm_silu_f16`,
`ief_groupnorm_cstat_f16`, `ief_layernorm_f16`, `ief_geglu_f16`, `ief_softmax_rows_f16`, `ief_conv_in_f32` and `ief_conv_out_f32`
launched on a misaligned operand.  No caller in the library trips a guard: the whole suite passes with them in.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ief_amd import hip  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = 7.0
TINY = 2.0 ** -24


def randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def h16(*shape, seed=0, scale=1.0, shift=0.0):
    return (randn(*shape, seed=seed, scale=scale) + shift).half()


def dev(t):
    return None if t is None else t.to(DEV)


def bits(t):
    return t.cpu().contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def ulp16(r):
    """spacing of fp16 at |r| (fp64 tensor): 2^(floor(log2 |r|) - 10), 2^-24 in the subnormal range"""
    _, e = torch.frexp(r.abs().clamp_min(2.0 ** -14))          # |r| = m 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(r), e - 11)


def check_ulp(what, got, ref64, ref32):
    """the per-element bound of the module docstring; returns (worst excess over ulp16, F, elements not bit-equal)"""
    g = got.double().cpu()
    assert g.shape == ref64.shape, (g.shape, ref64.shape)
    floor32 = max(4.0 * (ref32.double() - ref64).abs().max().item(), TINY)
    err = (g - ref64).abs()
    over = err - ulp16(ref64)                                   # what the fp32 floor F has to cover
    nbad = int((over > floor32).sum())
    nneq = int((bits(got.cpu()) != bits(ref64.half())).sum())
    print(f"{what}: max |err| {err.max().item():.2e}, max (|err| - ulp16) {over.max().item():+.2e} against F = {floor32:.2e}, "
          f"{nbad} of {g.numel()} outside, {nneq} ({100.0 * nneq / g.numel():.2f} %) not bit-equal to ref64.half()")
    assert torch.isfinite(g).all(), what
    assert nbad == 0, f"{what}: {nbad} elements outside ulp16 + F, worst excess {over.max().item():.3e} (F = {floor32:.3e})"
    return over.max().item(), floor32, nneq


def with_sentinel_row(rows, cols, dtype=torch.float16):
    """(buffer [rows + 1, cols] filled with the sentinel, its first `rows` rows)"""
    buf = torch.full((rows + 1, cols), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:rows]


def sentinel_kept(buf):
    return bool((buf[-1] == SENTINEL).all())


def off_alignment(t, nelem=1):
    """the values of t as a contiguous device view that starts `nelem` elements (2 bytes fp16, 4 bytes fp32) past 16-byte alignment"""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[nelem:nelem + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == nelem * t.element_size() and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------------ 1. GroupNorm, own statistics
def gn_form(B, HW, C1, C2, G):
    """the dispatch of ief_groupnorm_silu_f16, restated -> (form, detail)"""
    C = C1 + C2
    cpg = C // G
    if cpg % 2 == 0 and C1 % 2 == 0 and cpg // 2 <= 256 and HW * cpg * 2 <= 48 * 1024:
        cp2 = cpg // 2
        PY = min(512 // cp2, HW)
        threads = (cp2 * PY + 63) // 64 * 64
        if threads > 512:
            PY -= 1
            threads = (cp2 * PY + 63) // 64 * 64
        rounds = (HW + PY * 8 - 1) // (PY * 8)
        KS = 1
        while KS * 2 <= rounds and KS * 2 <= 2 and B * G * KS < 512:
            KS *= 2
        return "one-workgroup", dict(PY=PY, live=cp2 * PY, threads=threads, rounds=rounds, KS=KS, interleaved=G % 32 == 0)
    splits = min(max(HW // 16, 1), 64)
    per = (HW + splits - 1) // splits
    C8 = C // 8
    PYs = max(min(256 // C8, per, 4096 // C if C <= 4096 else 0), 1)
    return "three-launch", dict(splits=splits, empty=sum(1 for s in range(splits) if s * per >= HW), PYs=PYs, live=C8 * PYs,
                                threads=max(C8 * PYs, 64), lds_floats=PYs * C)


# (B, HW, C1, C2, groups), the form the dispatch takes, and what the case exercises (checked against gn_form below)
GN_CASES = [
    ((1, 1, 64, 0, 32), "one-workgroup", dict(PY=1, threads=64)),                       # HW = 1: one live lane of 64
    ((2, 37, 64, 0, 32), "one-workgroup", dict(PY=37, threads=64)),                     # HW < PY
    ((1, 1024, 64, 0, 32), "one-workgroup", dict(PY=512, rounds=1, KS=1)),              # one round, 512 pixel lanes, 2 channels per group
    ((2, 256, 320, 0, 32), "one-workgroup", dict(live=510, threads=512)),               # two dead lanes
    ((2, 1024, 640, 0, 32), "one-workgroup", dict(rounds=3, KS=2)),                     # KS = 2, ragged last round (pixels 816 .. 1023 of 408)
    ((16, 1024, 320, 0, 32), "one-workgroup", dict(rounds=2, KS=1)),                    # B * groups = 512 keeps KS = 1 with two rounds
    ((1, 1024, 768, 0, 32), "one-workgroup", dict(rounds=4, KS=2)),                     # slab exactly 48 KiB
    ((2, 100, 328, 312, 32), "one-workgroup", dict(interleaved=True)),                  # group 16 = channels 320 .. 339 straddles the concat at 328
    ((2, 64, 24, 40, 4), "one-workgroup", dict(interleaved=False)),                     # group 1 = channels 16 .. 31 straddles at 24; linear map
    ((1, 64, 512, 0, 64), "one-workgroup", dict(interleaved=True)),                     # 64 groups: two interleaved chunks of 32
    ((2, 50, 64, 0, 1), "one-workgroup", dict(interleaved=False, threads=512)),         # one group
    ((1, 1025, 768, 0, 32), "three-launch", dict(splits=64, empty=3)),                  # one pixel past 48 KiB; splits 61 .. 63 own no pixel
    ((2, 50, 96, 0, 32), "three-launch", dict(live=204)),                               # 3 channels per group
    ((1, 5, 24, 0, 8), "three-launch", dict(live=15, threads=64)),                      # C8 * PY = 15: 64 threads, 49 of them padding
    ((1, 200, 4096, 0, 32), "three-launch", dict(PYs=1, live=512, lds_floats=4096)),    # C8 = 512 > 256: PYs 0 -> 1; LDS partials exactly full
    ((2, 1024, 640, 320, 32), "three-launch", dict(splits=64, empty=0)),                # 60 KiB slab, group 21 = 630 .. 659 straddles at 640
]

_GN_INPUTS = {}


def gn_inputs(case, kind="centred"):
    """x, x2 (fp16), gamma, beta (fp32) and the fp64 / fp32 CPU GroupNorm of the concat, computed once per case"""
    key = (case, kind)
    if key not in _GN_INPUTS:
        B, HW, C1, C2, G = case
        C = C1 + C2
        if kind == "centred":
            x, x2 = h16(B, HW, C1, seed=1, scale=2.0, shift=0.5), (h16(B, HW, C2, seed=2, shift=-1.0) if C2 else None)
        else:                                       # kind = (offset, std): far from zero
            x, x2 = h16(B, HW, C1, seed=1, scale=kind[1], shift=kind[0]), (h16(B, HW, C2, seed=2, scale=kind[1], shift=kind[0]) if C2 else None)
        gamma, beta = 1 + randn(C, seed=3, scale=0.1), randn(C, seed=4, scale=0.1)
        xin = x if x2 is None else torch.cat([x, x2], -1)
        n64 = F.group_norm(xin.double().permute(0, 2, 1), G, gamma.double(), beta.double(), 1e-5).permute(0, 2, 1).contiguous()
        n32 = F.group_norm(xin.float().permute(0, 2, 1), G, gamma, beta, 1e-5).permute(0, 2, 1).contiguous()
        _GN_INPUTS[key] = (x, x2, gamma, beta, xin, n64, n32)
    return _GN_INPUTS[key]


def gn_run(case, x, x2, gamma, beta, silu, **kw):
    """hip.groupnorm into a buffer with a sentinel row behind it, twice: (output, second output bit-identical, sentinel kept)"""
    B, HW, C1, C2, G = case
    buf, out = with_sentinel_row(B * HW, C1 + C2)
    out = out.view(B, HW, C1 + C2)
    got = hip.groupnorm(x, gamma, beta, G, 1e-5, silu=silu, x2=x2, out=out, **kw)
    got = got[0] if isinstance(got, tuple) else got
    assert got.data_ptr() == buf.data_ptr()
    first = got.clone()
    hip.groupnorm(x, gamma, beta, G, 1e-5, silu=silu, x2=x2, out=out, **kw)
    return first, torch.equal(bits(first), bits(out)), sentinel_kept(buf)


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("case,form,detail", GN_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}+{c[3]}g{c[4]}" for c, _, _ in GN_CASES])
def test_groupnorm_own_statistics(case, form, detail, silu):
    took, d = gn_form(*case)
    assert took == form and all(d[k] == v for k, v in detail.items()), (took, d)
    x, x2, gamma, beta, _, n64, n32 = gn_inputs(case)
    ref64, ref32 = (F.silu(n64), F.silu(n32)) if silu else (n64, n32)
    got, same, kept = gn_run(case, dev(x), dev(x2), dev(gamma), dev(beta), silu)
    check_ulp(f"groupnorm {case} silu={silu} [{took} {d}]", got, ref64, ref32)
    print(f"    second run bit-identical {same}, sentinel row kept {kept}")
    assert same and kept


def test_groupnorm_too_many_channels_for_the_three_launches_is_refused():
    """(1, 200, 4104, 0, 27): 152 channels per group, a 59 KiB slab -> the three-launch form, whose LDS partials hold 4096 channels"""
    case = (1, 200, 4104, 0, 27)
    assert gn_form(*case)[0] == "three-launch"
    buf, out = with_sentinel_row(200, 4104)
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.groupnorm(dev(h16(1, 200, 4104, seed=1)), dev(torch.ones(4104)), dev(torch.zeros(4104)), 27, 1e-5, out=out.view(1, 200, 4104))
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), "a refused call wrote to its destination"
    print("groupnorm C = 4104, groups = 27: IEF_ESHAPE, nothing written")


@pytest.mark.parametrize("case", [(2, 256, 320, 0, 32), (2, 50, 96, 0, 32)], ids=["one-workgroup", "three-launch"])
def test_groupnorm_returned_statistics(case):
    """`return_stats=True`: (mean, rstd) per (batch, group) against fp64, relative to the largest of each"""
    B, HW, C1, C2, G = case
    x, x2, gamma, beta, xin, _, _ = gn_inputs(case)
    out, st = hip.groupnorm(dev(x), dev(gamma), dev(beta), G, 1e-5, silu=True, return_stats=True)
    xg = xin.double().view(B, HW, G, -1).permute(0, 2, 1, 3).reshape(B, G, -1)
    mean, rstd = xg.mean(-1), (xg.var(-1, unbiased=False) + 1e-5).rsqrt()
    st = st.double().cpu()
    em = ((st[..., 0] - mean).abs().max() / mean.abs().max()).item()
    er = ((st[..., 1] - rstd).abs().max() / rstd.abs().max()).item()
    print(f"groupnorm {case} [{gn_form(*case)[0]}] returned statistics: mean {em:.2e}, rstd {er:.2e} (relative to the largest)")
    assert st.shape == (B, G, 2) and em <= 1e-5 and er <= 1e-5


@pytest.mark.parametrize("offset,std", [(30.0, 0.75), (-45.0, 0.6)])
@pytest.mark.parametrize("case", [(2, 256, 320, 0, 32), (2, 1024, 640, 320, 32)], ids=["one-workgroup", "three-launch"])
def test_groupnorm_own_statistics_offset_inputs(case, offset, std):
    """|mean| / std = 40 and 75: E[x^2] - mean^2 in fp32 by design; the project's own bound for it, 8e-3 absolute"""
    x, x2, gamma, beta, xin, n64, _ = gn_inputs(case, (offset, std))
    s = xin.float().std().item()
    assert 0.2 < s < 1.5 and abs(xin.float().mean().item() - offset) < 1.0
    got, same, kept = gn_run(case, dev(x), dev(x2), dev(gamma), dev(beta), True)
    e = (got.double().cpu() - F.silu(n64)).abs().max().item()
    print(f"groupnorm {case} [{gn_form(*case)[0]}] inputs {offset:+.0f} +- {s:.2f} (mean / std {abs(offset) / s:.0f}): max |err| {e:.2e} "
          f"(bound 8e-3), second run bit-identical {same}, sentinel kept {kept}")
    assert e < 8e-3 and same and kept


# ------------------------------------------------------------------------------------------------ 2. GroupNorm on producer statistics
def cstat_form(HW, C1, C2, G, bm1, bm2):
    """the dispatch of ief_groupnorm_cstat_f16, restated -> (form, slice widths, bytes of one workgroup's fold)"""
    C = C1 + C2
    cpg = C // G
    unit = cpg * 8 // math.gcd(cpg, 8)
    nt = max(HW // bm1, HW // bm2 if C2 else 0)
    CW = min(unit * ((192 + unit - 1) // unit), C)
    fused = unit <= 256 and CW <= 512 and CW // 8 <= 256 and nt * CW * 8 <= 16 * 1024
    return ("one-launch" if fused else "fold + apply"), [min(CW, C - c) for c in range(0, C, CW)], nt * CW * 8


def col_stats(x, bm, HW):
    """what a producer leaves for its fp16 output x [B, HW, C]: per tile of bm rows and channel (sum, sum of squares), here the
    fp64 sums rounded to fp32 -> hip.ColStats that describes the device copy of x"""
    B, _, C = x.shape
    xd = dev(x)
    if HW % bm == 0:
        t = x.double().view(B * HW // bm, bm, C)
        buf = torch.stack([t.sum(1), (t * t).sum(1)], -1).float()
    else:
        buf = torch.zeros((B * HW + bm - 1) // bm, C, 2)
    return xd, hip.ColStats(dev(buf.contiguous()), bm, HW, xd)


# (HW, C1, C2, groups, bm1, bm2), form, slices of the one-launch form
CSTAT_CASES = [
    ((256, 320, 0, 32, 128, 0), "one-launch", [200, 120]),                  # slices of 200 + 120 channels
    ((256, 320, 320, 32, 128, 64), "one-launch", [200, 200, 200, 40]),      # 2 tiles on x, 4 on x2; slice 2 takes channels of both
    ((128, 328, 312, 32, 64, 64), "one-launch", [200, 200, 200, 40]),       # concat at 328 inside slice 2, which also holds group 16 (320 .. 339)
    ((128, 32, 0, 32, 64, 0), "one-launch", [32]),                          # one channel per group
    ((1024, 320, 0, 32, 128, 0), "one-launch", [200, 120]),                 # 8 tiles: a 12.5 KiB fold, under the 16 KiB threshold
    ((2048, 320, 0, 32, 128, 0), "fold + apply", None),                     # 16 tiles: 25 KiB
    ((64, 2880, 0, 32, 64, 0), "fold + apply", None),                       # lcm(90, 8) = 360 > 256: no slice of whole groups and chunks
    ((2048, 320, 320, 32, 128, 64), "fold + apply", None),                  # two sources, 16 and 32 tiles
]


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("case,form,slices", CSTAT_CASES, ids=[f"{c[0]}x{c[1]}+{c[2]}g{c[3]}bm{c[4]}-{c[5]}" for c, _, _ in CSTAT_CASES])
def test_groupnorm_on_producer_statistics_consumer_alone(case, form, slices, silu):
    """the fold and the apply, independent of any producer: statistics built here from the fp16 tensors; against fp64 under the ulp
    bound, as is the own-statistics call on the same input"""
    HW, C1, C2, G, bm1, bm2 = case
    took, widths, fold = cstat_form(*case)
    assert took == form and (slices is None or widths == slices), (took, widths)
    if case[:2] == (1024, 320):
        assert fold == 12800
    B = 2
    gcase = (B, HW, C1, C2, G)
    x, x2, gamma, beta, _, n64, n32 = gn_inputs(gcase)
    ref64, ref32 = (F.silu(n64), F.silu(n32)) if silu else (n64, n32)
    xd, cs = col_stats(x, bm1, HW)
    x2d, cs2 = col_stats(x2, bm2, HW) if C2 else (None, None)
    got, same, kept = gn_run(gcase, xd, x2d, dev(gamma), dev(beta), silu, cstat=cs, cstat2=cs2)
    check_ulp(f"groupnorm on producer statistics {case} silu={silu} [{took}, slices {widths if slices else '-'}, fold {fold} B]", got, ref64, ref32)
    own, _, _ = gn_run(gcase, xd, x2d, dev(gamma), dev(beta), silu)
    check_ulp(f"    own statistics on the same input [{gn_form(*gcase)[0]}]", own, ref64, ref32)
    print(f"    second run bit-identical {same}, sentinel row kept {kept}")
    assert same and kept


@pytest.mark.parametrize("case", [(256, 320, 0, 32, 128, 0), (2048, 320, 320, 32, 128, 64)], ids=["one-launch", "fold+apply"])
@pytest.mark.parametrize("offset,std", [(30.0, 0.75), (-45.0, 0.6)])
def test_groupnorm_on_producer_statistics_offset_inputs(case, offset, std):
    HW, C1, C2, G, bm1, bm2 = case
    gcase = (2, HW, C1, C2, G)
    x, x2, gamma, beta, xin, n64, _ = gn_inputs(gcase, (offset, std))
    assert 0.2 < xin.float().std().item() < 1.5
    xd, cs = col_stats(x, bm1, HW)
    x2d, cs2 = col_stats(x2, bm2, HW) if C2 else (None, None)
    got, same, kept = gn_run(gcase, xd, x2d, dev(gamma), dev(beta), True, cstat=cs, cstat2=cs2)
    e = (got.double().cpu() - F.silu(n64)).abs().max().item()
    print(f"groupnorm on producer statistics {case} [{cstat_form(*case)[0]}] inputs {offset:+.0f} +- {std} : max |err| {e:.2e} (bound 1.5e-2), "
          f"second run bit-identical {same}, sentinel kept {kept}")
    assert e < 1.5e-2 and same and kept


def test_groupnorm_on_producer_statistics_refusals():
    """a tile height that does not divide HW: IEF_ESHAPE; statistics that describe another tensor: ValueError; nothing written"""
    B, HW, C, G = 2, 256, 320, 32
    x, _, gamma, beta, _, _, _ = gn_inputs((B, HW, C, 0, G))
    buf, out = with_sentinel_row(B * HW, C)
    xd, cs = col_stats(x, 96, HW)
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.groupnorm(xd, dev(gamma), dev(beta), G, 1e-5, silu=True, cstat=cs, out=out.view(B, HW, C))
    xd, cs = col_stats(x, 128, HW)
    with pytest.raises(ValueError):
        hip.groupnorm(torch.empty_like(xd), dev(gamma), dev(beta), G, 1e-5, silu=True, cstat=cs, out=out.view(B, HW, C))
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    print("groupnorm on producer statistics: HW % bm != 0 IEF_ESHAPE, statistics of another tensor ValueError, nothing written")


def test_groupnorm_on_a_real_producers_statistics():
    """hip.conv3x3(col_stats=True) into groupnorm(cstat=...), groups = 32: the reference is the fp64 GroupNorm of the fp16 tensor the
    convolution wrote"""
    B, hw, C = 2, 32, 320
    x, cs = hip.conv3x3(dev(h16(B, hw, hw, 64, seed=1)), dev(h16(C, 3, 3, 64, seed=2, scale=1 / 24.0)), dev(randn(C, seed=3, scale=0.3)),
                        col_stats=True)
    assert cs is not None and cs.describes(x)
    gamma, beta = 1 + randn(C, seed=9, scale=0.1), randn(C, seed=10, scale=0.1)
    xin = x.cpu().view(B, hw * hw, C)
    ref64 = F.silu(F.group_norm(xin.double().permute(0, 2, 1), 32, gamma.double(), beta.double(), 1e-5)).permute(0, 2, 1)
    ref32 = F.silu(F.group_norm(xin.float().permute(0, 2, 1), 32, gamma, beta, 1e-5)).permute(0, 2, 1)
    buf, out = with_sentinel_row(B * hw * hw, C)
    got = hip.groupnorm(x, dev(gamma), dev(beta), 32, 1e-5, silu=True, cstat=cs, out=out.view(B, hw, hw, C))
    form = cstat_form(hw * hw, C, 0, 32, cs.bm, 0)[0]
    check_ulp(f"groupnorm on conv3x3's statistics B={B} {hw}x{hw} C={C} tile height {cs.bm} [{form}]", got.view(B, hw * hw, C), ref64, ref32)
    assert sentinel_kept(buf)


# ------------------------------------------------------------------------------------------------ 3. LayerNorm
# layernorm_kernel keeps a row in LN_MAXCH = 4 register pieces of 8 halves per lane: C8 = C / 8 chunks over 64 lanes
LN_CASES = [
    (1, 8),         # one live lane; three idle waves in the workgroup
    (5, 512),       # piece 0 exactly full; the second workgroup has one live wave
    (7, 520),       # one chunk in piece 1
    (3, 1024), (3, 1032), (2, 1536), (2, 1544),     # the edges of pieces 1 / 2 / 3
    (6, 2048),      # all four pieces full: the widest row
    (4099, 320),    # 1025 workgroups of four rows, the last with three live waves
]


def _layernorm_case(x, what):
    rows, C = x.shape
    gamma, beta = 1 + randn(C, seed=2, scale=0.1), randn(C, seed=3, scale=0.1)
    ref64 = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    ref32 = F.layer_norm(x.float(), (C,), gamma, beta, 1e-5)
    buf, out = with_sentinel_row(rows, C)
    got = hip.layernorm(dev(x), dev(gamma), dev(beta), 1e-5, out=out)
    assert got.data_ptr() == buf.data_ptr()
    r = check_ulp(what, got, ref64, ref32)
    assert sentinel_kept(buf), "the row behind the last one was written"
    return r


@pytest.mark.parametrize("rows,C", LN_CASES)
def test_layernorm_register_row_edges(rows, C):
    assert C % 8 == 0 and C <= 2048
    _layernorm_case(h16(rows, C, seed=1, scale=3.0, shift=1.0), f"layernorm rows={rows} C={C} [{(C // 8 + 63) // 64} register pieces]")


def test_layernorm_offset_rows():
    """two-pass statistics: rows offset by -20 .. +20 of their spreads keep the ulp bound"""
    rows, C = 301, 1280
    x = randn(rows, C, seed=1)
    x = (x + (torch.linspace(-20.0, 20.0, rows) * x.std(1))[:, None]).half()
    _layernorm_case(x, f"layernorm rows={rows} C={C} rows offset by -20 .. +20 spreads")


@pytest.mark.parametrize("C", [2056, 12])
def test_layernorm_refused_widths(C):
    buf, out = with_sentinel_row(3, C)
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.layernorm(dev(h16(3, C, seed=1)), dev(torch.ones(C)), dev(torch.zeros(C)), 1e-5, out=out)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    print(f"layernorm C={C}: IEF_ESHAPE, nothing written")


# ------------------------------------------------------------------------------------------------ 4. GEGLU
def _geglu_case(x, what):
    rows, Ch = x.shape[0], x.shape[1] // 2
    hdn, gate = x.double().chunk(2, -1)
    ref64 = hdn * F.gelu(gate)
    hdn32, gate32 = x.float().chunk(2, -1)
    ref32 = hdn32 * F.gelu(gate32)
    buf, out = with_sentinel_row(rows, Ch)
    got = hip.geglu(dev(x), out=out)
    assert got.data_ptr() == buf.data_ptr()
    r = check_ulp(what, got, ref64, ref32)
    assert sentinel_kept(buf)
    return r


def test_geglu_past_the_grid_cap():
    """geglu_kernel caps its grid at 4096 workgroups x 256 lanes = 1048576 chunks of 8: 1027 rows x 1024 chunks are 1051648, the
    last 3072 of them a second trip of 12 workgroups; gates out to +-12"""
    rows, Ch = 1027, 8192
    assert rows * (Ch // 8) > 4096 * 256
    x = torch.cat([randn(rows, Ch, seed=1, scale=2.0), randn(rows, Ch, seed=2, scale=3.0).clamp(-12, 12)], -1)
    x[:, Ch:Ch + 49] = torch.linspace(-12.0, 12.0, 49)              # the gate's whole range in every row, the last ones included
    _geglu_case(x.half(), f"geglu rows={rows} Ch={Ch} (second trip of the grid-stride loop)")


def test_geglu_one_chunk():
    x = torch.cat([randn(1, 8, seed=1, scale=2.0), torch.tensor([[-12.0, -3.0, -0.5, 0.0, 0.5, 3.0, 6.0, 12.0]])], -1).half()
    _geglu_case(x, "geglu rows=1 Ch=8 (one chunk)")


def test_geglu_overflow_gives_inf_as_torch_fp16():
    """hidden * gelu(gate) beyond 65504: +-inf, like the fp16 rounding of the exact product"""
    hdn = torch.tensor([[60000.0, -60000.0, 60000.0, 30000.0, -30000.0, 65504.0, 1.0, -2.0]])
    gate = torch.tensor([[2.0, 2.0, -2.0, 3.0, 3.0, 1.5, 12.0, 12.0]])
    x = torch.cat([hdn, gate], -1).half()
    ref = (x.double()[:, :8] * F.gelu(x.double()[:, 8:])).half()
    got = hip.geglu(dev(x)).cpu()
    print(f"geglu overflow: got {got.tolist()}, fp16 of the fp64 product {ref.tolist()}")
    assert torch.isinf(ref[0, :2]).all() and torch.isinf(ref[0, 3:6]).all() and not torch.isinf(ref[0, 2]) and not torch.isinf(ref[0, 6:]).any()
    assert torch.equal(torch.isinf(got), torch.isinf(ref)) and torch.equal(torch.sign(got), torch.sign(ref))
    assert torch.equal(bits(got[torch.isinf(ref)]), bits(ref[torch.isinf(ref)]))
    fin = ~torch.isinf(ref)
    assert ((got[fin].double() - ref[fin].double()).abs() <= ulp16(ref[fin].double())).all()


# ------------------------------------------------------------------------------------------------ 5. elementwise
BIG = 524288 + 1027          # silu_kernel / the cast kernels cap at 2048 workgroups x 256 = 524288 elements: 1027 make a second trip


@pytest.mark.parametrize("n", [1, BIG])
def test_silu_f16_past_the_grid_cap(n):
    x = h16(n, seed=1, scale=3.0)
    got = hip.silu(dev(x))
    check_ulp(f"silu fp16 n={n}", got, F.silu(x.double()), F.silu(x.float()))


@pytest.mark.parametrize("n", [1, BIG])
def test_casts_bit_equal(n):
    """fp32 -> fp16 and back, past the grid cap: +-0, fp16 subnormals and what rounds to them, 65504, values that round to it or to
    inf, large finite values, inf; planted at the front and in the tail of the second trip"""
    sp32 = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 1.0001 * 2.0 ** -25, 3.0 * 2.0 ** -25, 1e-7, -1e-7, 6.0e-5, 2.0 ** -14,
                         1023.0 * 2.0 ** -24, 65504.0, -65504.0, 65519.996, 65520.0, -65520.0, 65536.0, 1.0e5, -7.0e4, 3.0e38, -3.0e38,
                         float("inf"), float("-inf"), 1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11, 0.1, -1.0 / 3.0])
    xf = randn(n, seed=2, scale=100.0)
    if n > 1:
        xf[:sp32.numel()] = sp32
        xf[-sp32.numel():] = sp32
    else:
        xf[0] = 1.0e5
    buf = torch.full((n + 8,), SENTINEL, dtype=torch.float16, device=DEV)
    got = hip.to_f16(dev(xf), out=buf[:n])
    want = xf.half()
    same16 = torch.equal(bits(got), bits(want))
    past = xf.abs() > 65504.0
    same_past = torch.equal(bits(got.cpu()[past]), bits(want[past]))
    kept16 = bool((buf[n:] == SENTINEL).all())
    sp16 = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 1023.0 * 2.0 ** -24, 2.0 ** -14, 65504.0, -65504.0, float("inf"), float("-inf"), 1.0 / 3.0])
    xh = h16(n, seed=3, scale=50.0)
    if n > 1:
        xh[:sp16.numel()] = sp16.half()
        xh[-sp16.numel():] = sp16.half()
    else:
        xh[0] = 2.0 ** -24
    buf32 = torch.full((n + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    got32 = hip.to_f32(dev(xh), out=buf32[:n])
    same32 = torch.equal(bits(got32), bits(xh.float()))
    kept32 = bool((buf32[n:] == SENTINEL).all())
    print(f"casts n={n}: fp32 -> fp16 bit-equal {same16} ({int(past.sum())} values past 65504 bit-equal {same_past}), fp16 -> fp32 bit-equal "
          f"{same32}, sentinels kept {kept16} {kept32}")
    assert same16 and same_past and same32 and kept16 and kept32


@pytest.mark.parametrize("n", [7, 8 * (524288 + 300) + 5])
def test_add_f16_tail_and_grid_cap(n):
    """add_f16_kernel: chunks of 8 over at most 2048 x 256 lanes = 524288 chunks (300 more take the second trip), then the n % 8
    elements of the scalar tail in workgroup 0; n = 7 is the tail alone"""
    a, b = h16(n, seed=1, scale=3.0, shift=1.0), h16(n, seed=2)
    buf = torch.full((n + 8,), SENTINEL, dtype=torch.float16, device=DEV)
    got = hip.add(dev(a), dev(b), out=buf[:n])
    check_ulp(f"add fp16 n={n} (n / 8 = {n // 8} chunks, tail {n % 8})", got, a.double() + b.double(), a.float() + b.float())
    assert bool((buf[n:] == SENTINEL).all())


def test_add_and_gather_refuse_misaligned_operands():
    """the guards these two entry points had before this file"""
    a, b = h16(64, seed=1), h16(64, seed=2)
    out = torch.full((64,), SENTINEL, dtype=torch.float16, device=DEV)
    for args in ((off_alignment(a), dev(b)), (dev(a), off_alignment(b))):
        with pytest.raises(RuntimeError, match="IEF_EALIGN"):
            hip.add(*args, out=out)
    with pytest.raises(RuntimeError, match="IEF_EALIGN"):
        hip.gather_rows(off_alignment(a.view(4, 16)), dev(torch.tensor([1, 0, 3, 2], dtype=torch.int32)))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    print("add (a, b) and gather_rows (x) two bytes off alignment: IEF_EALIGN, nothing written")


def test_gather_rows_f16_past_the_grid_cap():
    """gather_rows_kernel caps at 2048 x 256 = 524288 chunks of 8; 3 rows of 174771 chunks are 524313"""
    row = 8 * 174771
    assert 3 * (row // 8) > 2048 * 256
    x = h16(3, row, seed=1)
    src = torch.tensor([2, 0, 2], dtype=torch.int32)
    got = hip.gather_rows(dev(x), dev(src))
    same = torch.equal(bits(got), bits(x[src.long()]))
    print(f"gather_rows fp16 3 x {row} src [2, 0, 2]: bit-equal {same}")
    assert same


def _softmax_rows(kind, L):
    s = randn(3, L, seed=L, scale=4.0)
    if kind == "peak80":
        idx = (torch.arange(3) * 7919 + 5) % L
        s[torch.arange(3), idx] = s.max(1).values + 80.0
    elif kind == "shift6e4":
        s = s + 6.0e4
    elif kind == "constant":
        s = torch.tensor([[-3.0], [0.0], [1000.0]]).expand(3, L).contiguous()
    return s.half()


@pytest.mark.parametrize("kind", ["gauss4", "peak80", "shift6e4", "constant"])
@pytest.mark.parametrize("L", [8, 2048, 2056, 16384])
def test_softmax_rows_f16(L, kind):
    """softmax_rows_kernel keeps a row in SM_MAXCH = 8 register pieces of 8 halves per lane over 256 lanes: L = 8 one live lane,
    2048 piece 0 exactly full, 2056 one chunk in piece 1, 16384 all eight full"""
    s = _softmax_rows(kind, L)
    ref64, ref32 = torch.softmax(s.double(), -1), torch.softmax(s.float(), -1)
    buf, view = with_sentinel_row(3, L)
    view.copy_(s)
    out = hip.softmax_rows_(view)
    assert out.data_ptr() == buf.data_ptr()
    check_ulp(f"softmax_rows fp16 L={L} {kind} [{(L // 8 + 255) // 256} register pieces]", out, ref64, ref32)
    sums = out.double().sum(-1).cpu()
    print(f"    row sums of the fp16 result {[f'{v:.5f}' for v in sums.tolist()]}, sentinel row kept {sentinel_kept(buf)}")
    assert sentinel_kept(buf)


@pytest.mark.parametrize("L", [16392, 12])
def test_softmax_rows_f16_refused_widths(L):
    x = dev(h16(3, L, seed=1))
    keep = x.clone()
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.softmax_rows_(x)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    print(f"softmax_rows fp16 L={L}: IEF_ESHAPE, rows untouched")


@pytest.mark.parametrize("R,C", [(1, 1), (32, 32), (33, 31), (100, 257)])
def test_transpose_bit_equal(R, C):
    """transpose_kernel, 32 x 32 tiles: one element, one full tile, a partial second tile in both directions, 4 x 9 tiles"""
    x = h16(R, C, seed=R)
    got = hip.transpose(dev(x))
    same = torch.equal(bits(got), bits(x.t().contiguous()))
    print(f"transpose {R} x {C}: bit-equal {same}")
    assert got.shape == (C, R) and same


def test_select_step_past_the_grid_cap():
    """select_step_kernel caps at 1024 x 256 = 262144 words; rows of 262144 + 77 words.  A step below 0 reads the first row, one
    past the table the last"""
    words, rows = 262144 + 77, 3
    table = randn(rows, words, seed=1)
    td = dev(table)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    buf, out = with_sentinel_row(1, words, dtype=torch.float32)
    for s, row in ((-3, 0), (0, 0), (rows - 1, rows - 1), (1 << 20, rows - 1), (1, 1)):
        step.fill_(s)
        hip.select_step(td, out[0], step)
        same = torch.equal(bits(out[0]), bits(table[row]))
        print(f"select_step {4 * words} bytes per row, step {s}: row {row} bit-equal {same}, sentinel kept {sentinel_kept(buf)}")
        assert same and sentinel_kept(buf)
    with pytest.raises(RuntimeError, match="IEF_EALIGN"):                   # 14 bytes per row
        hip.select_step(dev(h16(3, 7, seed=1)), torch.empty(7, dtype=torch.float16, device=DEV), step)


def test_pointwise_f32():
    """pointwise_f32_kernel, one lane per pixel: 3 x 431 = 1293 pixels, the sixth workgroup ragged.  fp32 throughout: bias, then
    Cin products added one by one = Cin + 1 rounded operations per output"""
    B, Cin, Cout, HW = 3, 8, 8, 431
    x, w, bias = randn(B, Cin, HW, 1, seed=1), randn(Cout, Cin, seed=2, scale=0.5), randn(Cout, seed=3, scale=0.1)
    got = hip.pointwise_f32(dev(x), dev(w), dev(bias)).double().cpu()
    xd, wd = x.double()[..., 0], w.double()
    ref = torch.einsum("oc,bcp->bop", wd, xd) + bias.double()[None, :, None]
    mag = torch.einsum("oc,bcp->bop", wd.abs(), xd.abs()) + bias.double().abs()[None, :, None]
    ratio = ((got[..., 0] - ref).abs() / ((Cin + 1) * TINY * mag)).max().item()
    print(f"pointwise_f32 {Cin} -> {Cout}, {B} x {HW} pixels: max |err| {(got[..., 0] - ref).abs().max().item():.2e}, {ratio:.3f} of the bound")
    assert got.shape == (B, Cout, HW, 1) and ratio <= 1.0
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.pointwise_f32(dev(randn(1, 9, 4, 1, seed=1)), dev(randn(8, 9, seed=2)))


@pytest.mark.parametrize("dim", [2, 320, 1280])
def test_timestep_embedding_f16(dim):
    t = torch.tensor([981.0, 1.0, 0.0])
    emb = hip.timestep_embedding(dev(t), dim).cpu()
    half = dim // 2
    ang = t.double()[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)[None]
    ref = torch.cat([torch.cos(ang), torch.sin(ang)], -1)
    e = (emb.double() - ref).abs().max().item()
    row0 = torch.cat([torch.ones(half), torch.zeros(half)]).half()
    exact = torch.equal(bits(emb[2]), bits(row0))
    print(f"timestep_embedding fp16 dim={dim}: max abs err {e:.2e}, row of t = 0 exact {exact}")
    assert emb.shape == (3, dim) and emb.dtype == torch.float16 and e <= 2e-3 and exact


# ------------------------------------------------------------------------------------------------ 6. conv_in
def conv_in_slices(Cin, Cout):
    """the slice search of ief_conv_in_f32, restated -> (slices, channels per slice, LDS bytes)"""
    nsl = (Cout + 255) // 256
    while True:
        assert nsl <= Cout // 8
        if Cout % nsl == 0 and (Cout // nsl) % 8 == 0:
            lds = (9 * Cin * (Cout // nsl) + 32 * 9 * Cin) * 4
            if lds <= 64 * 1024:
                return nsl, Cout // nsl, lds
        nsl += 1


# (B, Cin, H, W, Cout), bias, (slices, channels per slice, LDS bytes)
CONV_IN_CASES = [
    ((1, 4, 1, 1, 8), True, (1, 8, 5760)),              # one pixel, one chunk: 31 of 32 pixel slots idle
    ((2, 4, 5, 7, 320), True, (2, 160, 27648)),         # two slices of 160; 70 pixels: the third workgroup has 6
    ((1, 4, 3, 3, 264), True, (3, 88, 17280)),          # 264 / 2 = 132 is no multiple of 8: three slices of 88
    ((1, 4, 3, 3, 264), False, (3, 88, 17280)),         # bias = None
    ((1, 8, 4, 4, 320), True, (2, 160, 55296)),         # 54 KiB of LDS
    ((1, 8, 4, 4, 256), True, (2, 128, 46080)),         # one slice of 256 needs 81 KiB: refused before the search went on
    ((1, 8, 4, 4, 512), True, (4, 128, 46080)),         # two slices of 256 likewise; three do not divide; four of 128
]


@pytest.mark.parametrize("case,with_bias,slices", CONV_IN_CASES, ids=[f"{c}{'' if b else '-nobias'}" for c, b, _ in CONV_IN_CASES])
def test_conv_in_f16_slices(case, with_bias, slices):
    B, Cin, H, W, Cout = case
    assert conv_in_slices(Cin, Cout) == slices
    x = randn(B, Cin, H, W, seed=1)
    w = h16(3, 3, Cin, Cout, seed=2, scale=(9 * Cin) ** -0.5)
    bias = randn(Cout, seed=3, scale=0.1) if with_bias else None
    wt = w.permute(3, 2, 0, 1)
    ref64 = F.conv2d(x.double(), wt.double(), None if bias is None else bias.double(), padding=1).permute(0, 2, 3, 1)
    ref32 = F.conv2d(x, wt.float(), bias, padding=1).permute(0, 2, 3, 1)
    buf, out = with_sentinel_row(B * H * W, Cout)
    got = hip.conv_in(dev(x), dev(w), dev(bias), out=out.view(B, H, W, Cout))
    assert got.data_ptr() == buf.data_ptr()
    check_ulp(f"conv_in fp16 {case} bias={with_bias} [{slices[0]} slices of {slices[1]}, {slices[2]} B of LDS]", got, ref64, ref32)
    assert sentinel_kept(buf)


@pytest.mark.parametrize("Cin,Cout", [(9, 320), (4, 12)])
def test_conv_in_f16_refused_shapes(Cin, Cout):
    buf, out = with_sentinel_row(9, Cout)
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.conv_in(dev(randn(1, Cin, 3, 3, seed=1)), dev(h16(3, 3, Cin, Cout, seed=2)), None, out=out.view(1, 3, 3, Cout))
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    print(f"conv_in fp16 Cin={Cin} Cout={Cout}: IEF_ESHAPE, nothing written")


# ------------------------------------------------------------------------------------------------ 7. conv_out
def conv_out_kernel(C, Cout):
    """the dispatch of ief_conv_out_f32, restated"""
    lds = Cout * 9 * C * 2
    for ch, cmax in ((1, 128), (2, 256), (3, 384)):
        if C <= cmax and lds <= 48 * 1024:
            return f"conv_out_kernel<{ch}>", lds
    return "conv_out_wide_kernel", lds


def _conv_out_ref(x, w, bias):
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None if bias is None else bias.double(), padding=1)


def _conv_out_run(x, w, bias):
    B, H, W, _ = x.shape
    Cout = w.shape[0]
    buf = torch.full((B * Cout * H * W + H * W,), SENTINEL, device=DEV)
    out = buf[:B * Cout * H * W].view(B, Cout, H, W)
    got = hip.conv_out(dev(x), dev(w), dev(bias), out=out)
    assert got.data_ptr() == buf.data_ptr() and got.dtype == torch.float32
    return got.double().cpu(), bool((buf[B * Cout * H * W:] == SENTINEL).all())


# (B, C, H, W, Cout), kernel, bytes of weights
CONV_OUT_CASES = [
    ((1, 8, 1, 1, 1), "conv_out_kernel<1>", 144),                   # one pixel, one chunk, one output: 15 of 16 lanes hold zeros
    ((2, 128, 5, 7, 3), "conv_out_kernel<1>", 6912),                # <1> at its upper edge; 70 pixels: the fifth workgroup has 6
    ((2, 136, 5, 7, 4), "conv_out_kernel<2>", 9792),                # one chunk past <1>
    ((2, 256, 5, 7, 4), "conv_out_kernel<2>", 18432),
    ((2, 264, 5, 7, 4), "conv_out_kernel<3>", 19008),               # one chunk past <2>
    ((2, 384, 5, 7, 4), "conv_out_kernel<3>", 27648),
    ((2, 336, 5, 7, 8), "conv_out_kernel<3>", 48384),               # the largest weight set under 48 KiB
    ((2, 344, 5, 7, 8), "conv_out_wide_kernel", 49536),             # C <= 384, weights past 48 KiB
    ((2, 392, 5, 7, 4), "conv_out_wide_kernel", 28224),             # one chunk past <3>
    ((2, 512, 5, 7, 4), "conv_out_wide_kernel", 36864),
]


@pytest.mark.parametrize("case,kernel,wbytes", CONV_OUT_CASES, ids=[str(c) for c, _, _ in CONV_OUT_CASES])
def test_conv_out_f16_every_kernel(case, kernel, wbytes):
    B, C, H, W, Cout = case
    assert conv_out_kernel(C, Cout) == (kernel, wbytes)
    x = h16(B, H, W, C, seed=1)
    w, bias = h16(Cout, 3, 3, C, seed=2, scale=(9 * C) ** -0.5), randn(Cout, seed=3, scale=0.1)
    ref = _conv_out_ref(x, w, bias)
    got, kept = _conv_out_run(x, w, bias)
    e, bound = (got - ref).abs().max().item(), 1e-4 * ref.abs().max().item() + 1e-5
    print(f"conv_out fp16 {case} [{kernel}, {wbytes} B of weights]: max |err| {e:.2e} (bound {bound:.2e}), sentinel kept {kept}")
    assert got.shape == (B, Cout, H, W) and torch.isfinite(got).all() and e <= bound and kept


@pytest.mark.parametrize("C", [344, 384])
def test_conv_out_f16_wide_kernel_against_the_lds_kernel(C):
    """Cout = 8 in one call takes the wide kernel at these widths (48.4 / 54 KiB of weights); the two halves of the same weights
    as Cout = 4 take `conv_out_kernel<3>`: both against fp64 and against each other, same bound; bias = None on this case"""
    B, H, W = 2, 5, 7
    assert conv_out_kernel(C, 8)[0] == "conv_out_wide_kernel" and conv_out_kernel(C, 4)[0] == "conv_out_kernel<3>"
    x, w = h16(B, H, W, C, seed=1), h16(8, 3, 3, C, seed=2, scale=(9 * C) ** -0.5)
    ref = _conv_out_ref(x, w, None)
    wide, kept = _conv_out_run(x, w, None)
    lds = torch.cat([_conv_out_run(x, w[:4].contiguous(), None)[0], _conv_out_run(x, w[4:].contiguous(), None)[0]], 1)
    bound = 1e-4 * ref.abs().max().item() + 1e-5
    ew, el, ewl = (wide - ref).abs().max().item(), (lds - ref).abs().max().item(), (wide - lds).abs().max().item()
    print(f"conv_out fp16 C={C} Cout=8: wide kernel {ew:.2e}, conv_out_kernel<3> on the halves {el:.2e}, one against the other {ewl:.2e} "
          f"(bound {bound:.2e})")
    assert ew <= bound and el <= bound and ewl <= bound and kept


@pytest.mark.parametrize("C,Cout", [(64, 9), (12, 4)])
def test_conv_out_f16_refused_shapes(C, Cout):
    out = torch.full((1, Cout, 3, 3), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.conv_out(dev(h16(1, 3, 3, C, seed=1)), dev(h16(Cout, 3, 3, C, seed=2)), None, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    print(f"conv_out fp16 C={C} Cout={Cout}: IEF_ESHAPE, nothing written")


# ------------------------------------------------------------------------------------------------ 8. alignment guards
def _refused(call, *dests):
    with pytest.raises(RuntimeError, match="IEF_EALIGN"):
        call()
    torch.cuda.synchronize()
    for d in dests:
        assert bool((d == SENTINEL).all()), "a refused call wrote to its destination"


def test_misaligned_operands_are_refused():
    """an fp16 operand that starts 2 bytes, or an fp32 gamma / beta that starts 4 bytes, past 16-byte alignment: IEF_EALIGN from the
    checks in front of the launch (csrc/norm.hip, csrc/conv_io.hip, ief_softmax_rows_f16), and the destination keeps its sentinel.
    Each entry point below has that guard on the lines before its launch, and the shapes restate which form would have run; no
    other entry point is handed such a pointer here"""
    def obuf(*shape):
        n = math.prod(shape)
        b = torch.full((n + 8,), SENTINEL, dtype=torch.float16, device=DEV)
        al, off = b[:n].view(shape), b[1:1 + n].view(shape)
        assert al.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 2
        return b, al, off

    # ief_groupnorm_silu_f16, one workgroup per (batch, group) (channel pairs: 4 bytes): x, x2, out
    case = (2, 37, 64, 64, 32)
    assert gn_form(*case)[0] == "one-workgroup"
    x, x2 = h16(2, 37, 64, seed=1), h16(2, 37, 64, seed=2)
    ga, be = dev(torch.ones(128)), dev(torch.zeros(128))
    b, oal, ooff = obuf(2, 37, 128)
    _refused(lambda: hip.groupnorm(off_alignment(x), ga, be, 32, 1e-5, x2=dev(x2), out=oal), b)
    _refused(lambda: hip.groupnorm(dev(x), ga, be, 32, 1e-5, x2=off_alignment(x2), out=oal), b)
    _refused(lambda: hip.groupnorm(dev(x), ga, be, 32, 1e-5, x2=dev(x2), out=ooff), b)
    # ... the three launches (8 halves / 4 floats): x, x2, out, gamma, beta
    case = (2, 50, 96, 96, 64)
    assert gn_form(*case)[0] == "three-launch"
    x, x2 = h16(2, 50, 96, seed=1), h16(2, 50, 96, seed=2)
    g1, b1 = torch.ones(192), torch.zeros(192)
    b, oal, ooff = obuf(2, 50, 192)
    _refused(lambda: hip.groupnorm(off_alignment(x), dev(g1), dev(b1), 64, 1e-5, x2=dev(x2), out=oal), b)
    _refused(lambda: hip.groupnorm(dev(x), dev(g1), dev(b1), 64, 1e-5, x2=off_alignment(x2), out=oal), b)
    _refused(lambda: hip.groupnorm(dev(x), dev(g1), dev(b1), 64, 1e-5, x2=dev(x2), out=ooff), b)
    _refused(lambda: hip.groupnorm(dev(x), off_alignment(g1), dev(b1), 64, 1e-5, x2=dev(x2), out=oal), b)
    _refused(lambda: hip.groupnorm(dev(x), dev(g1), off_alignment(b1), 64, 1e-5, x2=dev(x2), out=oal), b)
    # ief_groupnorm_cstat_f16, both forms: x, out, gamma, beta
    for HW in (256, 2048):
        xc = h16(1, HW, 320, seed=1)
        g1, b1 = torch.ones(320), torch.zeros(320)
        b, oal, ooff = obuf(1, HW, 320)
        xoff = off_alignment(xc)
        stats = col_stats(xc, 128, HW)[1].buf
        _refused(lambda: hip.groupnorm(xoff, dev(g1), dev(b1), 32, 1e-5, cstat=hip.ColStats(stats, 128, HW, xoff), out=oal), b)
        xd, cs = col_stats(xc, 128, HW)
        _refused(lambda: hip.groupnorm(xd, dev(g1), dev(b1), 32, 1e-5, cstat=cs, out=ooff), b)
        _refused(lambda: hip.groupnorm(xd, off_alignment(g1), dev(b1), 32, 1e-5, cstat=cs, out=oal), b)
        _refused(lambda: hip.groupnorm(xd, dev(g1), off_alignment(b1), 32, 1e-5, cstat=cs, out=oal), b)
    # ief_layernorm_f16: x, out, gamma, beta
    xl, g1, b1 = h16(9, 640, seed=1), torch.ones(640), torch.zeros(640)
    b, oal, ooff = obuf(9, 640)
    _refused(lambda: hip.layernorm(off_alignment(xl), dev(g1), dev(b1), out=oal), b)
    _refused(lambda: hip.layernorm(dev(xl), dev(g1), dev(b1), out=ooff), b)
    _refused(lambda: hip.layernorm(dev(xl), off_alignment(g1), dev(b1), out=oal), b)
    _refused(lambda: hip.layernorm(dev(xl), dev(g1), off_alignment(b1), out=oal), b)
    # ief_geglu_f16: in, out
    xg = h16(5, 128, seed=1)
    b, oal, ooff = obuf(5, 64)
    _refused(lambda: hip.geglu(off_alignment(xg), out=oal), b)
    _refused(lambda: hip.geglu(dev(xg), out=ooff), b)
    # ief_softmax_rows_f16: x (in place: the rows keep their values)
    xs = off_alignment(h16(3, 64, seed=1))
    keep = xs.clone()
    _refused(lambda: hip.softmax_rows_(xs))
    assert torch.equal(xs, keep)
    # ief_conv_in_f32: w, out
    xi, wi = randn(1, 4, 5, 6, seed=5), h16(3, 3, 4, 16, seed=6)
    b, oal, ooff = obuf(1, 5, 6, 16)
    _refused(lambda: hip.conv_in(dev(xi), off_alignment(wi), None, out=oal), b)
    _refused(lambda: hip.conv_in(dev(xi), dev(wi), None, out=ooff), b)
    # ief_conv_out_f32: x, w; the LDS kernel and the wide kernel read the same 16-byte pieces
    for C, Co in ((64, 4), (392, 4)):
        xo, wo = h16(1, 4, 4, C, seed=1), h16(Co, 3, 3, C, seed=2)
        out = torch.full((1, Co, 4, 4), SENTINEL, device=DEV)
        _refused(lambda: hip.conv_out(off_alignment(xo), dev(wo), None, out=out), out)
        _refused(lambda: hip.conv_out(dev(xo), off_alignment(wo), None, out=out), out)
    print("misaligned operands: groupnorm one-workgroup (x, x2, out), three-launch (x, x2, out, gamma, beta), on producer statistics in both "
          "forms (x, out, gamma, beta), layernorm (x, out, gamma, beta), geglu (in, out), softmax_rows (x), conv_in (w, out), conv_out (x, w; "
          "both kernels) all IEF_EALIGN, destinations untouched")
