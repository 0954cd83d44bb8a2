"""The AutoencoderKL's blocks against fp64, block by block, in all three precisions (`vae.py`, `precision=` "f16", "f32", "f16x3").

`tests/test_gpu_vae.py` runs the fp16-storage VAE end to end; the fp32-storage VAEs are reached only behind whole edits.  Here
every block of the `SD_VAE` widths gets a known input and is compared with `oracle/vae_ref.py` run in fp64 on the same input
(NHWC on the device, NCHW in the oracle), so an error cannot cancel across blocks: the resnets without and with the fused 1x1
shortcut, GroupNorm on its own and on the column statistics of its producers (plain, stride-2 `pad_hi_only` and `upsample=True`
convolutions), the single-head d = 512 attention done by GEMM, and `encode` / `decode` whole.

Error measure: max |got - ref64| / max |ref64|.  Bounds come from the reference side only:
    f32, f16x3   max(4 floor32, 1e-6), floor32 = the error of the same oracle function in torch fp32 on the CPU (the rule of
                 tests/test_gpu_cross_map_grad.py); a single launch (one convolution, one GEMM): XTOL = 4e-6 (tests/test_gpu_x3.py)
    f16          4 floor16, floor16 = the error of the oracle function in fp64 rounded to fp16 wherever the device stores an fp16
                 tensor (`_resnet_r`, `_attn_rows`); input and weights are the fp16-rounded ones on both sides.
                 Whole model: 1e-2 and uint8 <= 2 levels on > 99.9 %, as tests/test_gpu_vae.py.
Every test prints what it measured and its share of the bound.

Column statistics exist on the fp16 path only, from HW = 256 up (`hip._CSTAT_MIN_HW`) and not on every launch form: at 8x12
a resnet hands over None.  So the 512 -> 512 resnet runs on its predecessor's hand-over at 8x12, as the model chains them, and
the 128 -> 256 resnet at 16x24 on the stride-2 convolution's, which are real (asserted).

Measured on an MI355X (error as a share of the bound; worst case of each group):
    group                                               f16              f32     f16x3
    resnets, own statistics (4 shapes)                  0.29             0.44    0.26
    resnets on the producer's hand-over (2)             0.32             0.08    0.05
    resampling convolutions, one launch (4)             0.25             0.11    0.08
    GroupNorm + SiLU on what they hand over (4)         0.36             0.32    0.35
    GroupNorm alone (9 inputs, SiLU off and on)         0.25             0.33    0.33
    mid attention, N = 96 and 1024                      0.25             0.12    0.12    (before `a_map`, f16x3 at 1024: 0.58)
    mid attention, max |k| = 1000                       0.25             0.19    0.22    (f16x3 before `w_act`: NaN)
    mid attention, 4096 flat keys                       0.25             0.07    0.06    (before `a_map`, f16x3: 1.21)
    P.V alone, 4096 flat keys                           0.25             0.11    0.09    (before `a_map`, f16x3: 25.6)
    encode, decode at 64x96                             1.1e-3, 1.8e-3   0.38    0.36    uint8: at most 1 level off in all three
    encode, decode at 40x72                             refused          0.37    0.30
The fp16 path sits at a quarter of its bound nearly everywhere: a single launch rounds fp64-accurate values to fp16, as floor16 does.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ief_amd import hip  # noqa: E402
from ief_amd.vae import AutoencoderKL, SD_VAE, synthetic_vae_state_dict  # noqa: E402
from oracle import vae_ref  # noqa: E402
from oracle.p2p_ref import latent_to_uint8  # noqa: E402

PRECISIONS = ("f16", "f32", "f16x3")
G, EPS = SD_VAE.norm_num_groups, SD_VAE.eps
XTOL = 4e-6          # tests/test_gpu_x3.py / KTOL of tests/test_gpu_exact.py: one contraction against fp64
ATT = "decoder.mid_block.attentions.0"


# ----------------------------------------------------------------------------------------------- shared state
@functools.lru_cache(maxsize=None)
def _sd():
    return synthetic_vae_state_dict(SD_VAE, 2)


@functools.lru_cache(maxsize=None)
def _vae(prec):
    return AutoencoderKL(SD_VAE, _sd(), precision=prec)


def _sub(prefixes, conv):
    """the tensors of the state dict under `prefixes`, converted"""
    prefixes = (prefixes,) if isinstance(prefixes, str) else tuple(prefixes)
    return {k: conv(v) for k, v in _sd().items() if k.startswith(prefixes)}


def r16(t):
    return t.half().to(t.dtype)


def ident(t):
    return t


def _weights(prefixes, half, sd=None):
    """(fp64 weights, fp32 weights) the reference runs on: of the fp16-rounded tensors for the fp16-storage mode"""
    src = _sub(prefixes, ident) if sd is None else sd
    if half:
        return {k: v.half().double() for k, v in src.items()}, None
    return {k: v.double() for k, v in src.items()}, {k: v.float() for k, v in src.items()}


def randn(*shape, seed, scale=1.0, offset=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + offset


def rel_err(got, ref):
    got = got.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite values"
    return ((got - ref).abs().max() / ref.abs().max()).item()


def to_dev(x_nchw, prec):
    return x_nchw.permute(0, 2, 3, 1).contiguous().to("cuda", torch.float16 if prec == "f16" else torch.float32)


def to_host(y_nhwc):
    return y_nhwc.double().cpu().permute(0, 3, 1, 2)


def bound_of(prec, floor, single=False):
    if prec == "f16":
        return 4.0 * floor
    return XTOL if single else max(4.0 * floor, 1e-6)


def check(what, prec, got, ref, floor, single=False):
    assert floor > 0.0, f"{what}: the reference-side floor is zero"
    bound = bound_of(prec, floor, single)
    e = rel_err(got, ref)
    print(f"{what} [{prec}]: err {e:.3e}, floor{'16' if prec == 'f16' else '32'} {floor:.3e}, bound {bound:.3e}, "
          f"share {e / bound:.2f}")
    assert e <= bound, f"{what} [{prec}]: {e:.3e} > {bound:.3e}"
    return e


# ----------------------------------------------------------------------------------------------- reference side
def _gn(x, w, b, silu):
    y = F.group_norm(x, G, w, b, EPS)
    return F.silu(y) if silu else y


def _resnet_r(sd, p, x, r):
    """`vae_ref._resnet` rounded with r wherever `vae._Resnet` stores a tensor"""
    h = r(_gn(x, sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], True))
    h = r(F.conv2d(h, sd[p + ".conv1.weight"], sd[p + ".conv1.bias"], padding=1))
    h = r(_gn(h, sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], True))
    h = F.conv2d(h, sd[p + ".conv2.weight"], sd[p + ".conv2.bias"], padding=1)
    if (p + ".conv_shortcut.weight") in sd:                 # one launch on the device: conv2 + shortcut + both biases
        x = F.conv2d(x, sd[p + ".conv_shortcut.weight"], sd[p + ".conv_shortcut.bias"])
    return r(x + h)


def _attn_rows(sd, p, x, rows=None, r=ident):
    """`vae_ref._attn` for the query rows `rows` (None: all), rounded with r wherever `vae._MidAttention` stores a tensor
    -> (out [B, rows, C] tokens-major, k [B, N, C], probabilities [B, rows, N])"""
    B, C, H, W = x.shape
    h = r(_gn(x, sd[p + ".group_norm.weight"], sd[p + ".group_norm.bias"], False)).reshape(B, C, H * W).transpose(1, 2)
    xt = x.reshape(B, C, H * W).transpose(1, 2)
    hq = h
    if rows is not None:
        hq, xt = h[:, rows], xt[:, rows]
    q = r(F.linear(hq, sd[p + ".to_q.weight"], sd[p + ".to_q.bias"]))
    k = r(F.linear(h, sd[p + ".to_k.weight"], sd[p + ".to_k.bias"]))
    v = r(F.linear(h, sd[p + ".to_v.weight"], sd[p + ".to_v.bias"]))
    s = r(q @ k.transpose(1, 2) * C ** -0.5)
    pr = r(torch.softmax(s, -1))
    a = r(pr @ v)
    return r(xt + F.linear(a, sd[p + ".to_out.0.weight"], sd[p + ".to_out.0.bias"])), k, pr


def _tokens(y_nchw):
    B, C, H, W = y_nchw.shape
    return y_nchw.reshape(B, C, H * W).transpose(1, 2)


def _down(sd, p, x):
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), sd[p + ".weight"], sd[p + ".bias"], stride=2)


def _up(sd, p, x):
    return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), sd[p + ".weight"], sd[p + ".bias"], padding=1)


def _refs(fn, fn_r, prefixes, x, half, sd=None):
    """fn(sd, x) -> tensor or tuple of tensors (the oracle's function); fn_r(sd, x, r): its rounded form.
    -> (the input both sides get, fp64 references, floors: floor16 if half else floor32)"""
    w64, w32 = _weights(prefixes, half, sd)
    tup = lambda t: t if isinstance(t, tuple) else (t,)
    with torch.no_grad():
        if half:
            x = x.half().float()
            ref = tup(fn(w64, x.double()))
            low = tup(fn_r(w64, x.double(), r16))
        else:
            ref = tup(fn(w64, x.double()))
            low = tup(fn(w32, x))
    for t in ref + low:
        assert torch.isfinite(t).all()
    return x, ref, tuple(rel_err(l, t) for l, t in zip(low, ref))


# ----------------------------------------------------------------------------------------------- resnets
RESNETS = {   # name: (oracle prefix, device block, Cin, H, W)
    "512-512@8x12": ("decoder.mid_block.resnets.0", lambda v: v.d_mid[0], 512, 8, 12),
    "128-256@16x24": ("encoder.down_blocks.1.resnets.0", lambda v: v.e_down[1][0][0], 128, 16, 24),
    "512-256@16x24": ("decoder.up_blocks.2.resnets.0", lambda v: v.d_up[2][0][0], 512, 16, 24),
    "256-128@32x48": ("decoder.up_blocks.3.resnets.0", lambda v: v.d_up[3][0][0], 256, 32, 48),
}


def _resnet_refs(p, x, half):
    return _refs(lambda sd, t: vae_ref._resnet(sd, p, t, G, EPS), lambda sd, t, r: _resnet_r(sd, p, t, r), p, x, half)


@functools.lru_cache(maxsize=None)
def _resnet_case(name, half):
    p, _, cin, H, W = RESNETS[name]
    return _resnet_refs(p, randn(2, cin, H, W, seed=11), half)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", list(RESNETS))
def test_resnet_block(name, prec):
    """one `_Resnet` from a known input, statistics of its input its own (cstat=None); the three fused-shortcut directions
    take `hip.conv3x3_shortcut` at 256 / 256 / 128 output columns"""
    p, block, cin, H, W = RESNETS[name]
    x, (ref,), (floor,) = _resnet_case(name, prec == "f16")
    vae = _vae(prec)
    assert block(vae).short == (name != "512-512@8x12")
    with hip.f32_contraction(vae.contract):
        out, _ = block(vae)(to_dev(x, prec), None)
    check(f"resnet {name}", prec, to_host(out), ref, floor)


def _after_resnet(vae, prec):
    return vae.d_mid[2](to_dev(randn(2, 512, 8, 12, seed=12), prec), None)


def _after_downsample(vae, prec):
    w, b = vae.e_down[0][1]
    return hip.conv3x3(to_dev(randn(2, 128, 32, 48, seed=12), prec), w, b, stride=2, pad_hi_only=True, col_stats=True)


PRODUCED = {   # name: (oracle prefix of the block under test, device block, producer of its (input, statistics), statistics exist in f16)
    "512-512@8x12 after a resnet": ("decoder.mid_block.resnets.0", lambda v: v.d_mid[0], _after_resnet, False),
    "128-256@16x24 after the downsample": ("encoder.down_blocks.1.resnets.0", lambda v: v.e_down[1][0][0], _after_downsample, True),
}


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", list(PRODUCED))
def test_resnet_block_on_producer_statistics(name, prec):
    """a resnet on the (output, statistics) pair of the launch before it in the same mode, as `_encode` / `_decode` chain them,
    against fp64 on that very output: the same bound as with its own statistics.  The mid-block form at 8x12 gets what a
    preceding resnet hands over (HW = 96 < 256: no statistics on any path); the fused-shortcut form at 16x24 gets the stride-2
    convolution's, which are real in fp16: its first GroupNorm runs `ief_groupnorm_cstat_f16`"""
    p, block, producer, has_stats = PRODUCED[name]
    vae = _vae(prec)
    with hip.f32_contraction(vae.contract):
        y0, cs = producer(vae, prec)
        if prec == "f16" and has_stats:
            assert cs is not None and cs.describes(y0), "the producer returned no column statistics"
        else:
            assert cs is None
        before = y0.clone()
        out, _ = block(vae)(y0, cs)
    assert torch.equal(y0, before)
    x, (ref,), (floor,) = _resnet_refs(p, to_host(y0).float(), prec == "f16")
    assert torch.equal(x.double(), to_host(y0))               # the reference read exactly what the device block read
    check(f"resnet {name}", prec, to_host(out), ref, floor)


# ----------------------------------------------------------------------------------------------- resampling convolutions
SAMPLERS = {   # name: (kind, conv prefix, consumer's norm prefix, device (w, b), device consumer block, C, H, W)
    "down128@32x48": ("down", "encoder.down_blocks.0.downsamplers.0.conv", "encoder.down_blocks.1.resnets.0.norm1",
                      lambda v: v.e_down[0][1], lambda v: v.e_down[1][0][0], 128, 32, 48),
    "down128@10x18": ("down", "encoder.down_blocks.0.downsamplers.0.conv", "encoder.down_blocks.1.resnets.0.norm1",
                      lambda v: v.e_down[0][1], lambda v: v.e_down[1][0][0], 128, 10, 18),
    "up512@8x12": ("up", "decoder.up_blocks.0.upsamplers.0.conv", "decoder.up_blocks.1.resnets.0.norm1",
                   lambda v: v.d_up[0][1], lambda v: v.d_up[1][0][0], 512, 8, 12),
    "up256@16x24": ("up", "decoder.up_blocks.2.upsamplers.0.conv", "decoder.up_blocks.3.resnets.0.norm1",
                    lambda v: v.d_up[2][1], lambda v: v.d_up[3][0][0], 256, 16, 24),
}


@functools.lru_cache(maxsize=None)
def _sampler_case(name, half):
    kind, pc, pn, _, _, C, H, W = SAMPLERS[name]
    conv = _down if kind == "down" else _up

    def fn_r(sd, x, r):
        h = r(conv(sd, pc, x))
        return h, r(_gn(h, sd[pn + ".weight"], sd[pn + ".bias"], True))

    return _refs(lambda sd, x: fn_r(sd, x, ident), fn_r, (pc, pn), randn(2, C, H, W, seed=13), half)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_resampling_conv_and_consuming_groupnorm(name, prec):
    """the stride-2 `pad_hi_only` and the `upsample=True` convolution with `col_stats=True` (one launch: XTOL in the fp32
    modes), and the next block's GroupNorm + SiLU on what they hand over"""
    kind, _, _, wb, consumer, C, H, W = SAMPLERS[name]
    x, (ref_h, ref_g), (floor_h, floor_g) = _sampler_case(name, prec == "f16")
    vae = _vae(prec)
    w, b = wb(vae)
    n1 = consumer(vae).n1
    kw = dict(stride=2, pad_hi_only=True) if kind == "down" else dict(upsample=True)
    with hip.f32_contraction(vae.contract):
        h, hs = hip.conv3x3(to_dev(x, prec), w, b, col_stats=True, **kw)
        g = hip.groupnorm(h, n1[0], n1[1], G, EPS, silu=True, cstat=hs)
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if kind == "down" else (2 * H, 2 * W)
    assert tuple(h.shape) == (2, Ho, Wo, C)
    if prec == "f16" and name == "down128@32x48":             # HW = 384: real statistics (the other launches may run split-K
        assert hs is not None and hs.describes(h), "the convolution returned no column statistics"      # forms that emit none)
    print(f"{name} [{prec}]: column statistics {'handed over' if hs is not None else 'none'}")
    check(f"{name} convolution", prec, to_host(h), ref_h, floor_h, single=True)
    check(f"{name} consuming GroupNorm", prec, to_host(g), ref_g, floor_g)


# ----------------------------------------------------------------------------------------------- GroupNorm alone
GN_CASES = [(C, HW, 0.0) for C in (64, 128, 256, 512) for HW in ((8, 12), (32, 48))] + [(128, (32, 48), 30.0)]


@functools.lru_cache(maxsize=None)
def _gn_case(C, HW, offset, half):
    x = randn(2, C, *HW, seed=14, offset=offset)
    gamma, beta = 1 + randn(C, seed=15, scale=0.1), randn(C, seed=16, scale=0.1)
    if offset:
        xg = x.reshape(2, G, -1)
        assert (xg.mean(-1).abs() > 20 * xg.std(-1)).all()           # |mean| >> std in every group
    if half:
        x = x.half().float()
    out = []
    for silu in (False, True):
        ref = _gn(x.double(), gamma.double(), beta.double(), silu)
        low = r16(ref) if half else _gn(x, gamma, beta, silu)
        out.append((ref, rel_err(low, ref)))
    return x, gamma, beta, out


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("C,HW,offset", GN_CASES)
def test_groupnorm_vae_channels_per_group(C, HW, offset, prec):
    """32 groups over 64 / 128 / 256 / 512 channels (2, 4, 8, 16 per group), eps = 1e-6, SiLU off and on, HW = 96 and 1536;
    one input with mean 30 and unit deviation"""
    x, gamma, beta, refs = _gn_case(C, HW, offset, prec == "f16")
    xd = to_dev(x, prec)
    for silu, (ref, floor) in zip((False, True), refs):
        got = hip.groupnorm(xd, gamma.cuda(), beta.cuda(), G, EPS, silu=silu)
        check(f"GroupNorm C={C} HW={HW[0] * HW[1]} offset={offset:g} silu={silu}", prec, to_host(got), ref, floor)


# ----------------------------------------------------------------------------------------------- mid-block attention
def _attn_refs(x, half, sd=None, rows=None, oracle=True):
    """(input, out64 [B, rows, C], floor, k64, probabilities64).  oracle: the fp64 reference and floor32 come from
    `vae_ref._attn` itself (all rows); otherwise from its row-restricted restatement"""
    w64, w32 = _weights(ATT, half, sd)
    with torch.no_grad():
        if half:
            x = x.half().float()
        ref, k, pr = _attn_rows(w64, ATT, x.double(), rows)
        if oracle:
            assert rows is None
            ref_o = _tokens(vae_ref._attn(w64, ATT, x.double(), G, EPS))
            assert torch.equal(ref_o, ref) or rel_err(ref, ref_o) < 1e-14      # the restatement IS the oracle's function
            ref = ref_o
        if half:
            low = _attn_rows(w64, ATT, x.double(), rows, r16)[0]
        elif oracle:
            low = _tokens(vae_ref._attn(w32, ATT, x, G, EPS))
        else:
            low = _attn_rows(w32, ATT, x, rows)[0]
    assert torch.isfinite(ref).all() and torch.isfinite(low).all()
    return x, ref, rel_err(low, ref), k, pr


@functools.lru_cache(maxsize=None)
def _attn_case(H, W, half):
    return _attn_refs(randn(2, 512, H, W, seed=17), half)[:3]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("H,W", [(8, 12), (32, 32)])
def test_mid_attention(H, W, prec):
    """`_MidAttention` (C = d = 512) at N = 96 and N = 1024: scores by `hip.gemm` on column views of q|k|v, `softmax_rows_`,
    `hip.gemm_nt` on a strided v"""
    x, ref, floor = _attn_case(H, W, prec == "f16")
    vae = _vae(prec)
    with hip.f32_contraction(vae.contract):
        out, _ = vae.d_mid[1](to_dev(x, prec), None)
    check(f"mid attention N={H * W}", prec, out.reshape(2, H * W, 512), ref, floor)


def _scaled_attention(att, q_scale, k_scale):
    """(a copy of the device block `att`, the state dict it was packed from) with to_q / to_k (weight and bias) scaled"""
    sd = {k: v.clone() for k, v in _sub(ATT, ident).items()}
    for n, s in (("to_q", q_scale), ("to_k", k_scale)):
        sd[f"{ATT}.{n}.weight"] *= s
        sd[f"{ATT}.{n}.bias"] *= s
    blk = copy.copy(att)
    blk.wqkv = torch.cat([sd[f"{ATT}.to_{n}.weight"] for n in "qkv"], 0).to(att.wqkv.device, att.wqkv.dtype).contiguous()
    blk.bqkv = torch.cat([sd[f"{ATT}.to_{n}.bias"] for n in "qkv"], 0).to(att.bqkv.device, torch.float32).contiguous()
    return blk, sd


@functools.lru_cache(maxsize=None)
def _large_key_scale():
    x = randn(2, 512, 8, 12, seed=18)
    k = _attn_rows(_weights(ATT, False)[0], ATT, x.double())[1]
    return x, 1000.0 / k.abs().max().item()


@pytest.mark.parametrize("prec", PRECISIONS)
def test_mid_attention_large_keys(prec):
    """max |k| ~ 1000 (to_k scaled up, to_q scaled down by the same factor: the logits are the plain case's).  Activations own
    the whole fp16 range in every mode (`hip.py`, X3_SCALE_*), and k is an activation although it is the score GEMM's B
    operand.  Measured (MI355X), f16x3: with k split at the weights' scale 2^8 |k| >= 256 overflowed the fp16 hi half and the
    output was NaN; split at the activations' scale 1 it was finite but 1.054e-6 of 1e-6, a miss: the case makes q uniformly
    ~2^-8, whose lo halves are fp16 subnormals at scale 1 (2^-25 absolute resolution, 6e-6 of a typical element), against
    keys of 220 rms.  Neither operand of this product has a static range, so `hip.gemm(..., w_act=True)` runs it on the
    fp32-input MFMA in both fp32-storage modes: 2.2e-7.  f32 1.9e-7, f16 3.8e-4 of 1.5e-3"""
    x, f = _large_key_scale()
    vae = _vae(prec)
    blk, sd = _scaled_attention(vae.d_mid[1], 1.0 / f, f)
    x, ref, floor, k, _ = _attn_refs(x, prec == "f16", sd=sd)
    _attn_refs(x, False, sd=sd)                                        # the fp32 CPU run is finite (checked inside)
    kmax = k.abs().max().item()
    print(f"large keys: factor {f:.1f}, max |k| {kmax:.1f}")
    assert 256.0 < kmax < 65504.0
    with hip.f32_contraction(vae.contract):
        out, _ = blk(to_dev(x, prec), None)
    assert torch.isfinite(out).all(), f"[{prec}] non-finite output for keys inside the fp16 range"
    check("mid attention, max |k| ~ 1000", prec, out.reshape(2, 96, 512), ref, floor)


FLAT_ROWS = torch.arange(256) * 16 + torch.arange(256) % 16          # 256 of the 4096 query rows, every residue mod 16


@functools.lru_cache(maxsize=None)
def _flat_case(half):
    x = randn(1, 512, 64, 64, seed=19)
    sd = {k: v.clone() for k, v in _sub(ATT, ident).items()}
    sd[ATT + ".to_q.weight"] *= 0.05
    sd[ATT + ".to_q.bias"] *= 0.05
    x, ref, floor, _, pr = _attn_refs(x, half, sd=sd, rows=FLAT_ROWS, oracle=False)
    N = 4096
    assert pr.max().item() < 2.0 / N and pr.min().item() > 0.5 / N          # flat: every probability near 2^-12 ...
    assert (pr.max(-1).values > pr.min(-1).values * 1.01).all()             # ... and no row exactly uniform
    return x, ref, floor


@pytest.mark.parametrize("prec", PRECISIONS)
def test_mid_attention_flat_rows_4096_keys(prec):
    """N = 4096 (the 512-pixel image's mid block; the last width of the <64> register softmax), queries scaled by 0.05: every
    probability is about 2^-12, where the lo half of an fp32 probability split at scale 1 is an fp16 subnormal.
    Measured (MI355X), f16x3: 1.214e-6 of 1e-6 before (a miss), 5.9e-8 with `hip.gemm_nt(..., a_map=True)`, which
    splits the probabilities at X3_SCALE_PROB as the fused attention kernels do; f32 6.5e-8, f16 3.5e-4 of 1.4e-3"""
    x, ref, floor = _flat_case(prec == "f16")
    vae = _vae(prec)
    blk, _ = _scaled_attention(vae.d_mid[1], 0.05, 1.0)
    with hip.f32_contraction(vae.contract):
        out, _ = blk(to_dev(x, prec), None)
    check("mid attention, flat rows N=4096", prec, out.reshape(1, 4096, 512)[:, FLAT_ROWS.cuda()], ref, floor)


@functools.lru_cache(maxsize=None)
def _pv_case(half):
    N = 4096
    pr = torch.softmax(randn(256, N, seed=20, scale=0.05).double(), -1).float()
    v = randn(N, 512, seed=21)
    assert pr.max().item() < 2.0 / N and pr.min().item() > 0.5 / N
    if half:
        pr, v = pr.half().float(), v.half().float()
    ref = pr.double() @ v.double()
    floor = rel_err(r16(ref), ref) if half else rel_err(pr @ v, ref)
    return pr, v, ref, floor


@pytest.mark.parametrize("prec", PRECISIONS)
def test_probabilities_times_values_flat_rows(prec):
    """the P.V product of the case above on its own, called as `_MidAttention` calls it: one launch, so XTOL in the fp32
    modes.  Inside the block the residual (|x| ~ 4 against |P.V| ~ 0.05) hides most of this product's error from the block
    bound.  Measured (MI355X), f16x3: 1.02e-4 before (probabilities split at scale 1: 25 x XTOL), 3.8e-7 with
    `a_map=True`; f32 4.6e-7; f16 3.2e-4 of 1.3e-3"""
    pr, v, ref, floor = _pv_case(prec == "f16")
    dt = torch.float16 if prec == "f16" else torch.float32
    qkv = torch.zeros(4096, 3 * 512, dtype=dt, device="cuda")
    qkv[:, 1024:] = v.to("cuda", dt)                                   # v as the block sees it: a column view, row stride 3 C
    with hip.f32_contraction(_vae(prec).contract):
        out = _pv(pr.to("cuda", dt), qkv[:, 1024:])
    check("P.V, flat rows N=4096", prec, out, ref, floor, single=True)


def _pv(probs, v):
    return hip.gemm_nt(probs, v, a_map=True)


# ----------------------------------------------------------------------------------------------- whole model
@functools.lru_cache(maxsize=None)
def _model_case(H, W):
    img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(22)) * 2 - 1
    z = randn(2, 4, H // 8, W // 8, seed=23)
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in _sd().items()}
        enc, dec = vae_ref.encode_mean(sd64, SD_VAE, img.double()), vae_ref.decode(sd64, SD_VAE, z.double())
        del sd64
        enc32, dec32 = vae_ref.encode_mean(_sd(), SD_VAE, img), vae_ref.decode(_sd(), SD_VAE, z)
    return img, z, enc, dec, rel_err(enc32, enc), rel_err(dec32, dec)


def _whole_model(H, W, prec):
    img, z, enc, dec, f_enc, f_dec = _model_case(H, W)
    vae = _vae(prec)
    lat = vae.encode(img.cuda())["latent_dist"].mean
    out = vae.decode(z.cuda())["sample"]
    assert lat.dtype == torch.float32 and out.dtype == torch.float32
    diff = abs(latent_to_uint8(out.cpu()).astype(int) - latent_to_uint8(dec).astype(int))
    e_enc, e_dec = rel_err(lat, enc), rel_err(out, dec)
    if prec == "f16":
        print(f"SD_VAE {H}x{W} [f16]: encode {e_enc:.3e}, decode {e_dec:.3e} (bound 1e-2), uint8 max {diff.max()}, "
              f"<= 2 on {(diff <= 2).mean():.5f}")
        assert e_enc < 1e-2 and e_dec < 1e-2
        assert (diff <= 2).mean() > 0.999
    else:
        check(f"SD_VAE {H}x{W} encode", prec, lat, enc, f_enc)
        check(f"SD_VAE {H}x{W} decode", prec, out, dec, f_dec)
        print(f"SD_VAE {H}x{W} [{prec}]: uint8 max difference {diff.max()}")
        assert diff.max() <= 1


@pytest.mark.parametrize("prec", PRECISIONS)
def test_encode_decode_64x96(prec):
    """`encode` and `decode` of the SD_VAE at 64x96 pixels (latent 8x12, N = 96 in the mid blocks), B = 2, against fp64"""
    _whole_model(64, 96, prec)


@pytest.mark.parametrize("prec", ("f32", "f16x3"))
def test_encode_decode_40x72_key_count_not_a_multiple_of_8(prec):
    """latent 5x9: N = 45 keys in the mid blocks, odd images at every level.  The fp32 softmax takes any row length"""
    _whole_model(40, 72, prec)


def test_f16_refuses_key_count_not_a_multiple_of_8():
    """the fp16-storage attention maps need rows of whole 16-byte pieces (N % 8 == 0): N = 45 is refused by the library's
    argument check before anything is launched for the maps; nothing is returned, and the device stays usable"""
    img, z = _model_case(40, 72)[:2]
    vae = _vae("f16")
    lat = out = None
    with pytest.raises(RuntimeError, match="IEF_EALIGN|IEF_ESHAPE"):
        lat = vae.encode(img.cuda())
    with pytest.raises(RuntimeError, match="IEF_EALIGN|IEF_ESHAPE"):
        out = vae.decode(z.cuda())
    assert lat is None and out is None
    torch.cuda.synchronize()
    _whole_model(64, 96, "f16")                                        # and the same model still computes
