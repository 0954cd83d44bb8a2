"""Key-split form of the planes attention (`attn_flash_x3p_kernel<.., SPLIT>` + `attn_flash_x3p_combine_kernel`,
`csrc/split_x3.hip`) on a real MI355X: the keys of every (b, head, query block) go over S workgroups that leave unnormalised
partials (O, lazy maximum, row sum) in a workspace, one combine launch merges them in a fixed order.

Stated tolerances (every test prints what it measured):
    split + combine vs fp64 on the host        <= 4e-6 of max |reference|  (one contraction: the bound of tests/test_gpu_x3p.py)
    planes written by the combine               == split of its fp32 output, bit for bit
    lse vs fp64 logsumexp (log2 units)          <= 1e-5 absolute            (the bound of tests/test_gpu_grad_f32.py)
    split vs unsplit                            <= 2 * 4e-6                 (each within 4e-6 of the same reference)
    one UNet forward vs the fp32 oracle         <= 1e-4                     (the bound of test_unet_forward_x3_vs_oracle)
"""
from ctypes import byref

import pytest
import torch

pytestmark = pytest.mark.gpu

from ief_amd import denoise, hip, planes  # noqa: E402
from ief_amd.pipeline import StableDiffusionPipeline  # noqa: E402
from ief_amd.p2p.inversion.ddim import ddim_inversion  # noqa: E402
from oracle import unet_ref  # noqa: E402

DEV = torch.device("cuda:0")
XTOL = 4e-6
LOG2E = 1.4426950408889634
PROMPT = ["a photo of a house on a mountain"]


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return None if t is None else t.cuda()


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max()).item()


def ref_split(x):
    """the definition of the planes: two round-to-nearest conversions"""
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


def _case(B, heads, N, L, d):
    """the construction of tests/test_gpu_x3p.py::test_attention_planes_in: column slices of one q|k|v planes tensor when N == L,
    the last batch row's keys / values taken from row 0, an fp64 reference (out, lse in log2 units) on the first <= 512 queries"""
    C = heads * d
    q, k, v = f32(B, N, C, seed=1), f32(B, L, C, seed=2, scale=1.5), f32(B, L, C, seed=3)
    if N == L:
        qkv = planes.split(dev(torch.cat([q, k, v], -1)))
        qp, kp, vp = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    else:
        qp, kp, vp = planes.split(dev(q)), planes.split(dev(k)), planes.split(dev(v))
    ks = torch.arange(B, dtype=torch.int32)
    ks[-1] = 0
    sub = slice(0, min(N, 512))
    qh = q.double()[:, sub].reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    kh = k.double()[ks.long()].reshape(B, L, heads, d).permute(0, 2, 1, 3)
    vh = v.double()[ks.long()].reshape(B, L, heads, d).permute(0, 2, 1, 3)
    sc = qh @ kh.transpose(-1, -2) * d ** -0.5
    ref = (torch.softmax(sc, -1) @ vh).permute(0, 2, 1, 3).reshape(B, -1, C)
    return dict(qp=qp, kp=kp, vp=vp, ks=dev(ks), sub=sub, ref=ref, lse2=torch.logsumexp(sc, -1) * LOG2E, scale=d ** -0.5)


def _names():
    return [r[0] for r in hip.profile_end()]


# ----------------------------------------------------------------------------------------------- 1. against fp64
@pytest.mark.parametrize("B,heads,N,L,d,S", [(1, 8, 512, 1024, 40, 4),      # even split
                                             (1, 3, 77, 333, 40, 3),        # 6 tiles of 64, the last one masked, N below one workgroup
                                             (2, 2, 200, 144, 64, 2),       # 5 tiles of 32 -> 3 + 2, swizzled rows, indirection
                                             (1, 1, 130, 64, 80, 8),        # 2 tiles: S clamps to 2
                                             (1, 4, 256, 256, 80, 3),       # 8 tiles -> 3 + 3 + 2
                                             (1, 8, 4096, 4096, 40, 4)])    # the one real shape
def test_key_split_attention_vs_fp64(B, heads, N, L, d, S):
    c = _case(B, heads, N, L, d)
    want_lse = N == L and d in (40, 64)
    lse = torch.full((B, heads, N), float("nan"), device=DEV) if want_lse else None
    hip.profile_begin()
    out = planes.attn_flash(c["qp"], c["kp"], c["vp"], heads, c["scale"], k_src=c["ks"], v_src=c["ks"], out_planes=False, lse=lse,
                            key_splits=S)
    names = _names()
    S_eff = planes.attn_key_splits(B, heads, N, L, d, setting=S)
    assert len(names) == 1 and f"split {S_eff}>" in names[0] and "attn_flash_x3p_combine_kernel" in names[0], names
    op = planes.attn_flash(c["qp"], c["kp"], c["vp"], heads, c["scale"], k_src=c["ks"], v_src=c["ks"], key_splits=S)
    e = rel_err(out[:, c["sub"]], c["ref"])
    print(f"key-split attention B={B} h={heads} N={N} L={L} d={d} S={S} (runs {S_eff}): {e:.2e}")
    assert e < XTOL
    assert_planes_equal_split(op, out)
    if want_lse:
        assert torch.isfinite(lse).all(), "the combine returned without writing lse"
        e_lse = (lse.double().cpu()[:, :, c["sub"]] - c["lse2"]).abs().max().item()
        print(f"    lse: {e_lse:.2e}")
        assert e_lse < 1e-5


def test_key_split_leaves_rows_past_N_alone():
    """a strided fp32 destination with sentinel rows behind the N queries: neither the partials nor the combine write past N"""
    B, heads, N, L, d = 1, 2, 77, 333, 40
    c = _case(B, heads, N, L, d)
    buf = torch.full((B, N + 51, heads * d), -7.0, device=DEV)
    planes.attn_flash(c["qp"], c["kp"], c["vp"], heads, c["scale"], out=buf[:, :N], out_planes=False, key_splits=3)
    assert rel_err(buf[:, :N], c["ref"]) < XTOL
    assert (buf[:, N:] == -7.0).all()


# ----------------------------------------------------------------------------------------------- 2. key_splits = 1
def test_key_splits_1_is_the_single_launch():
    B, heads, N, L, d = 1, 8, 512, 1024, 40
    c = _case(B, heads, N, L, d)
    base = planes.attn_flash(c["qp"], c["kp"], c["vp"], heads, c["scale"], out_planes=False)
    hip.profile_begin()
    one = planes.attn_flash(c["qp"], c["kp"], c["vp"], heads, c["scale"], out_planes=False, key_splits=1)
    names = _names()
    assert names == [f"attn_flash_x3p_kernel<{d}>"], f"key_splits=1 must take the single launch and no combine: {names}"
    assert torch.equal(one, base)
    # a count that clamps to 1 (one key tile) is the single launch too
    c1 = _case(1, 2, 64, 64, 40)
    hip.profile_begin()
    a = planes.attn_flash(c1["qp"], c1["kp"], c1["vp"], 2, c1["scale"], out_planes=False, key_splits=4)
    assert _names() == ["attn_flash_x3p_kernel<40>"]
    assert torch.equal(a, planes.attn_flash(c1["qp"], c1["kp"], c1["vp"], 2, c1["scale"], out_planes=False))


# ----------------------------------------------------------------------------------------------- 3. determinism
def test_key_split_is_deterministic_and_close_to_the_single_launch():
    B, heads, N, L, d = 1, 8, 512, 1024, 40
    c = _case(B, heads, N, L, d)
    run = lambda S: planes.attn_flash(c["qp"], c["kp"], c["vp"], heads, c["scale"], out_planes=False, key_splits=S)  # noqa: E731
    a, b, one = run(4), run(4), run(1)
    assert torch.equal(a, b), "fixed combine order: two launches must give the same bits"
    diff = (a.double() - one.double()).abs().max().item() / c["ref"].abs().max().item()
    print(f"split vs unsplit: {diff:.2e} of max |ref|")
    assert diff <= 2 * XTOL


# ----------------------------------------------------------------------------------------------- 4. maximum in a late split
def test_key_split_maximum_in_a_late_split():
    """the inputs of tests/test_gpu_x3.py::test_attention_x3_peaky_rows_force_the_rescale: planted keys growing with the tile
    index, so the row maximum of query 5 lives in the LAST split and the combine scales the early partials down by 2^(m_s - M).
    Yardstick: the unsplit planes launch (the parent's kernel) on the same inputs."""
    B, heads, N, L, d = 1, 2, 160, 512, 64
    q, k, v = f32(B, N, heads * d, seed=1), f32(B, L, heads * d, seed=2), f32(B, L, heads * d, seed=3)
    for t in range(L // 32):
        k[0, 32 * t + 7, :] = q[0, 5, :] * (0.5 + 0.25 * t)
    scale = d ** -0.5 * 4.0
    qh, kh, vh = (x.double().reshape(B, -1, heads, d).permute(0, 2, 1, 3) for x in (q, k, v))
    ref = (torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).permute(0, 2, 1, 3).reshape(B, N, heads * d)
    qp, kp, vp = planes.split(dev(q)), planes.split(dev(k)), planes.split(dev(v))
    one = planes.attn_flash(qp, kp, vp, heads, scale, out_planes=False)
    got = planes.attn_flash(qp, kp, vp, heads, scale, out_planes=False, key_splits=4)
    assert torch.isfinite(got).all()
    e1, e4 = rel_err(one, ref), rel_err(got, ref)
    print(f"peaky rows on planes: unsplit {e1:.2e}, 4 key splits {e4:.2e}")
    assert e4 <= max(XTOL, 2 * e1)


# ----------------------------------------------------------------------------------------------- 5. rejected arguments
def test_key_split_rejected_arguments():
    B, heads, N, L, d = 1, 2, 128, 256, 40
    q, k, v = dev(f32(B, N, heads * d, seed=1)), dev(f32(B, L, heads * d, seed=2)), dev(f32(B, L, heads * d, seed=3))
    with pytest.raises(RuntimeError, match="IEF_EINVAL"):
        hip.attn_flash(q, k, v, heads, d ** -0.5, key_splits=2)           # fp32 inputs: no operand planes, nothing to split over
    # the C entry point itself, operand planes in: a workspace one float short, a null one, a misaligned one
    lib = hip.load()
    qp, kp, vp = planes.split(q), planes.split(k), planes.split(v)
    out = torch.full((B, N, heads * d), float("nan"), device=DEV)
    p = hip.IefAttnF32Params()
    for t, nm in ((qp, "Q"), (kp, "K"), (vp, "V")):
        setattr(p, nm + "p", t.hi.data_ptr())
        setattr(p, "plane" + nm, t.plane)
    p.ldq, p.ldk, p.ldv, p.sQb, p.sKb, p.sVb = heads * d, heads * d, heads * d, N * heads * d, L * heads * d, L * heads * d
    p.B, p.heads, p.N, p.L, p.d, p.scale = B, heads, N, L, d, d ** -0.5
    p.x3, p.zeros = 1, planes._zeros(q.device)
    p.Out, p.sOb, p.ldo = out.data_ptr(), N * heads * d, heads * d
    nws = lib.ief_attn_flash_ws_floats(B, heads, N, L, d, 2)
    assert nws == 2 * B * heads * N * (d + 2)
    ws = torch.empty(nws + 4, dtype=torch.float32, device=DEV)
    p.key_splits, p.ws, p.ws_floats = 2, ws.data_ptr(), nws - 1
    assert lib.ief_attn_flash_f32(byref(p), hip._stream()) == -1, "a workspace one float short must be IEF_EINVAL"
    p.ws, p.ws_floats = None, nws
    assert lib.ief_attn_flash_f32(byref(p), hip._stream()) == -1, "a null workspace must be IEF_EINVAL"
    p.ws, p.ws_floats = ws.data_ptr() + 4, nws
    assert lib.ief_attn_flash_f32(byref(p), hip._stream()) == -3, "a workspace off the 16-byte grid must be IEF_EALIGN"
    p.x3 = 0
    p.ws = ws.data_ptr()
    assert lib.ief_attn_flash_f32(byref(p), hip._stream()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call must not launch"
    p.x3 = 1
    assert lib.ief_attn_flash_f32(byref(p), hip._stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ----------------------------------------------------------------------------------------------- 6. whole net
@pytest.fixture(scope="module")
def small_ks2():
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:small", precision="f16x3", attn_key_splits=2, keep_state_dict=True)
    yield pipe
    denoise.drop_pool()


def test_unet_forward_with_key_splits_vs_oracle(small_ks2):
    pipe = small_ks2
    assert pipe.unet.attn_key_splits == 2 and all(m.attn_key_splits == 2 for m in pipe.unet.attention_modules())
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 4, pipe.cfg.sample_size, pipe.cfg.sample_size, generator=g)
    ctx = torch.randn(1, 77, pipe.cfg.cross_attention_dim, generator=g)
    for t in (981, 1):
        hip.profile_begin()
        eps = pipe.unet(x.to(DEV), t, encoder_hidden_states=ctx.to(DEV))["sample"]
        names = set(_names())
        split = [n for n in names if n.startswith("attn_flash_x3p_kernel") and "split 2>" in n and "attn_flash_x3p_combine_kernel" in n]
        assert split, f"the self-attention must run split + combine: {sorted(names)}"
        assert not any(n.startswith("attn_flash_x3p_kernel") and n not in split for n in names), sorted(names)
        e = rel_err(eps, unet_ref.unet_forward(pipe._state_dict, pipe.cfg, x, torch.tensor(t), ctx))
        print(f"x3 small B=1 t={t} attn_key_splits=2: rel err {e:.3e}")
        assert e < 1e-4


def test_inversion_graph_with_key_splits(small_ks2):
    """the captured loop and its pooled reuse give the same latents; another setting never takes that graph from the pool"""
    pipe = small_ks2
    denoise.drop_pool()
    pipe.scheduler.set_timesteps(3)
    lat0 = torch.randn(1, 4, pipe.cfg.sample_size, pipe.cfg.sample_size, generator=torch.Generator().manual_seed(1)) * 0.8
    inv = ddim_inversion()
    a = inv.ddim_inversion_loop(pipe, lat0.to(DEV), PROMPT)[0][-1].clone()
    b = inv.ddim_inversion_loop(pipe, lat0.to(DEV), PROMPT)[0][-1].clone()
    assert torch.equal(a, b)
    keys = set(denoise._POOL)
    assert keys and all(k[-1] == 2 for k in keys), "the pool key must carry the setting"
    try:
        pipe.unet.attn_key_splits = 1
        one = inv.ddim_inversion_loop(pipe, lat0.to(DEV), PROMPT)[0][-1].clone()
        assert set(denoise._POOL) - keys, "a graph captured under another setting must not be re-pointed"
    finally:
        pipe.unet.attn_key_splits = 2
    e = rel_err(a, one)
    print(f"3-step inversion, attn_key_splits 2 vs 1: {e:.2e}")
    assert e < 1e-5
