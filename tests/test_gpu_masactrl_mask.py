"""Mask-guided MasaCtrl on a real MI355X: the gathered-rows instantiation of the planes attention (`attn_flash_x3p_kernel<.., IDX>`,
csrc/split_x3.hip) and the fused plan kind 'masactrl_mask' end to end.

Stated tolerances (every test prints what it measured):
    a gathered launch vs fp64 attention over the gathered rows   <= 4e-6 of max |reference| -- the bound tests/test_gpu_x3p.py
                                                                    holds the plain planes attention to at every head dim
    rows outside q_idx, and everything while the gate holds 0    bit-unchanged
    fused plan vs the same editor on the generic path (latents after 4 steps, `small` family, f16x3)
                                                                 <= 2 x the same distance for plain MutualSelfAttentionControl,
                                                                    measured in the same test (the masked rows sum over fewer
                                                                    keys: less averaging of the rounding)
    captured step graph vs eager stepping of the fused plan      bit for bit
"""
from ctypes import byref

import pytest
import torch

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip, planes  # noqa: E402

XTOL = 4e-6          # tests/test_gpu_x3p.py: planes attention vs fp64
DEV = torch.device("cuda:0")
SENTINEL = -7.25     # exactly representable in fp16: hi = -7.25, lo = 0


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return None if t is None else t.cuda()


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(autouse=True)
def _x3():
    with hip.f32_contraction("x3"):
        yield


def _operands(B, heads, N, d):
    """Gaussian q / k / v at the scales of test_gpu_x3p.py's attention test, as column slices of one q|k|v planes tensor"""
    C = heads * d
    q, k, v = f32(B, N, C, seed=1), f32(B, N, C, seed=2, scale=1.5), f32(B, N, C, seed=3)
    qkv = planes.split(dev(torch.cat([q, k, v], -1)))
    return (q, k, v), (qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:])


def _ref64(q, k, v, heads, d, q_idx, k_idx, ks=None):
    """fp64 attention of the listed query rows over the listed key rows (batch rows of k / v taken from ks)"""
    B, C = q.shape[0], heads * d
    ks = torch.arange(B) if ks is None else ks.long()
    qi, ki = q_idx.long(), k_idx.long()
    qh = q.double()[:, qi].reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    kh = k.double()[ks][:, ki].reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    vh = v.double()[ks][:, ki].reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    return (torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, -1) @ vh).permute(0, 2, 1, 3).reshape(B, -1, C)


def _split_lists(N, n_first, seed, scramble=False):
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
    a, b = perm[:n_first], perm[n_first:]
    if not scramble:
        a, b = a.sort().values, b.sort().values
    return a.to(torch.int32), b.to(torch.int32)


@pytest.mark.parametrize("B,heads,N,d,nfk,nfq,scramble", [
    (4, 2, 256, 40, 150, 70, False),      # 150 / 106 keys: no multiple of the 64-key tile; 70 / 186 queries: no multiple of 32
    (1, 2, 1024, 80, 5, 300, False),      # 5 fg keys: less than one tile; 1019 bg keys
    (2, 2, 256, 64, 100, 90, True),       # lists in scrambled order, K / V from the OTHER batch row
])
def test_gathered_launch_vs_fp64(B, heads, N, d, nfk, nfq, scramble):
    (q, k, v), (qp, kp, vp) = _operands(B, heads, N, d)
    C = heads * d
    fk, bk = _split_lists(N, nfk, 5, scramble)
    fq, bq = _split_lists(N, nfq, 6, scramble)
    ks = torch.arange(B, dtype=torch.int32).flip(0) if scramble else None
    out = torch.full((B, N, C), SENTINEL, device=DEV)
    op = planes.split(out)
    worst = 0.0
    for n, (qi, ki) in enumerate(((fq, fk), (bq, bk))):
        r = planes.attn_flash(qp, kp, vp, heads, d ** -0.5, k_src=dev(ks), v_src=dev(ks), out=out, out_planes=op,
                              q_idx=dev(qi), k_idx=dev(ki))
        assert r is op
        ref = _ref64(q, k, v, heads, d, qi, ki, ks)
        e = rel_err(out[:, qi.long()], ref)
        worst = max(worst, e)
        print(f"gathered d={d} N={N}: {qi.numel()} queries x {ki.numel()} keys: {e:.2e}")
        if n == 0:      # after the first launch the other class's rows still hold the sentinel, bit for bit
            assert torch.equal(out[:, bq.long()].cpu(), torch.full((B, bq.numel(), C), SENTINEL))
            assert torch.equal(op.hi[:, bq.long()].cpu(), torch.full((B, bq.numel(), C), SENTINEL).half())
            assert op.lo[:, bq.long()].abs().max().item() == 0
    assert worst < XTOL
    hi = out.half()
    assert torch.equal(op.hi, hi) and torch.equal(op.lo, (out - hi.float()).half()), "planes written == split of the fp32 output"


@pytest.mark.parametrize("d", [40, 64, 80])
def test_identity_lists_vs_plain_launch(d):
    B, heads, N = 2, 2, 200
    (q, k, v), (qp, kp, vp) = _operands(B, heads, N, d)
    ident = torch.arange(N, dtype=torch.int32, device=DEV)
    plain = planes.attn_flash(qp, kp, vp, heads, d ** -0.5, out_planes=False)
    out = torch.full_like(plain, SENTINEL)
    planes.attn_flash(qp, kp, vp, heads, d ** -0.5, out=out, q_idx=ident, k_idx=ident)
    ref = _ref64(q, k, v, heads, d, ident.cpu(), ident.cpu())
    e, e_plain = rel_err(out, ref), rel_err(plain, ref)
    print(f"identity lists d={d}: gathered {e:.2e}, plain {e_plain:.2e}, bit-equal: {torch.equal(out, plain)}")
    assert e < XTOL and e_plain < XTOL


def test_gate_and_untouched_rows():
    B, heads, N, d = 2, 2, 256, 40
    C = heads * d
    _, (qp, kp, vp) = _operands(B, heads, N, d)
    qi, rest = _split_lists(N, 70, 7)
    ki, _ = _split_lists(N, 150, 8)
    out = torch.full((B, N, C), SENTINEL, device=DEV)
    op = planes.split(out)
    out0, op0 = out.clone(), op.t.clone()
    gate = torch.zeros(1, dtype=torch.int32, device=DEV)
    planes.attn_flash(qp, kp, vp, heads, d ** -0.5, out=out, out_planes=op, q_idx=dev(qi), k_idx=dev(ki), gate=gate)
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(op.t, op0), "gate = 0: nothing may be written"
    gate.fill_(1)
    planes.attn_flash(qp, kp, vp, heads, d ** -0.5, out=out, out_planes=op, q_idx=dev(qi), k_idx=dev(ki), gate=gate)
    torch.cuda.synchronize()
    assert torch.equal(out[:, rest.long()], out0[:, rest.long()]) and torch.equal(op.t[:, :, rest.long()], op0[:, :, rest.long()])
    assert (out[:, qi.long()] != SENTINEL).all()


def test_binding_refuses_a_gathered_launch_without_a_destination():
    _, (qp, kp, vp) = _operands(1, 2, 64, 40)
    idx = torch.arange(64, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="destination"):
        planes.attn_flash(qp, kp, vp, 2, 40 ** -0.5, q_idx=idx, k_idx=idx)
    with pytest.raises(ValueError, match="go together"):
        planes.attn_flash(qp, kp, vp, 2, 40 ** -0.5, q_idx=idx, out=torch.zeros(1, 64, 80, device=DEV))
    out = torch.full((1, 64, 80), SENTINEL, device=DEV)
    with pytest.raises(ValueError, match="no lse"):
        planes.attn_flash(qp, kp, vp, 2, 40 ** -0.5, q_idx=idx, k_idx=idx, out=out, lse=torch.zeros(1, 2, 64, device=DEV))
    with pytest.raises(ValueError, match="does not split"):
        planes.attn_flash(qp, kp, vp, 2, 40 ** -0.5, q_idx=idx, k_idx=idx, out=out, key_splits=2)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


def test_library_refusals_launch_nothing():
    lib = hip.load()
    B, heads, N, d = 1, 2, 128, 40
    C = heads * d
    (q, k, v), (qp, kp, vp) = _operands(B, heads, N, d)
    out = torch.full((B, N, C), float("nan"), device=DEV)
    idx = torch.arange(N + 1, dtype=torch.int32, device=DEV)[:N]
    lse = torch.zeros(B, heads, N, device=DEV)

    def params(planes_in=True):
        p = hip.IefAttnF32Params()
        if planes_in:
            for t, nm in ((qp, "Q"), (kp, "K"), (vp, "V")):
                setattr(p, nm + "p", t.hi.data_ptr())
                setattr(p, "plane" + nm, t.plane)
            p.ldq = p.ldk = p.ldv = 3 * C
            p.sQb = p.sKb = p.sVb = N * 3 * C
        else:
            qd, kd, vd = dev(q), dev(k), dev(v)
            keep.extend((qd, kd, vd))
            p.Q, p.K, p.V = qd.data_ptr(), kd.data_ptr(), vd.data_ptr()
            p.ldq = p.ldk = p.ldv = C
            p.sQb = p.sKb = p.sVb = N * C
        p.B, p.heads, p.N, p.L, p.d, p.scale = B, heads, N, N, d, d ** -0.5
        p.x3, p.zeros = 1, planes._zeros(DEV)
        p.Out, p.sOb, p.ldo = out.data_ptr(), N * C, C
        p.q_idx, p.k_idx = idx.data_ptr(), idx.data_ptr()
        return p

    keep = []
    call = lambda p: lib.ief_attn_flash_f32(byref(p), hip._stream())
    p = params()
    p.lse = lse.data_ptr()
    assert call(p) == -1, "lse with lists: IEF_EINVAL"
    p = params()
    ws = torch.empty(lib.ief_attn_flash_ws_floats(B, heads, N, N, d, 2) + 4, device=DEV)
    p.key_splits, p.ws, p.ws_floats = 2, ws.data_ptr(), ws.numel()
    assert call(p) == -1, "key_splits = 2 with lists: IEF_EINVAL"
    assert call(params(planes_in=False)) == -1, "lists on a non-planes call: IEF_EINVAL"
    p = params()
    p.k_idx = None
    assert call(p) == -1, "one list without the other: IEF_EINVAL"
    p = params()
    p.q_idx = idx.data_ptr() + 2
    assert call(p) == -3, "a list pointer off the 4-byte grid: IEF_EALIGN"
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call must not launch"
    assert call(params()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------------- whole sampler
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]


@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.pipeline import StableDiffusionPipeline
    return StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")


def test_fused_plan_vs_generic_path_and_graph_vs_eager(small_x3):
    from ief_amd.denoise import FusedDenoiser
    from ief_amd.masactrl.model.attention_control import MutualSelfAttentionControl, MutualSelfAttentionControlMask
    from ief_amd.masactrl.model.register import regiter_attention_editor_diffusers, unregister_attention_control as unreg
    from ief_amd.masactrl.model.sd_utils import MasaCtrl

    class PlainOnTheGenericPath(MutualSelfAttentionControl):       # lowering goes by class name: a subclass is an unknown editor
        pass

    class MaskOnTheGenericPath(MutualSelfAttentionControlMask):
        pass

    pipe = small_x3
    cfg = pipe.cfg
    steps, layers = 4, list(range(2, 11))       # `small`: 11 transformer layers, head dims 40 (32 x 32 tokens) and 80 (16 x 16)
    size = cfg.sample_size * 8
    ms, mt = torch.zeros(32, 32), torch.zeros(32, 32)
    ms[8:24, 4:16] = 1
    mt[4:16, 8:28] = 1
    g = torch.Generator().manual_seed(8888)
    x_T = torch.cat([torch.randn(1, 4, cfg.sample_size, cfg.sample_size, generator=g) for _ in range(2)]).to(DEV)
    editor = MasaCtrl(pipe, steps)

    def run(c, kind):
        regiter_attention_editor_diffusers(pipe, c)
        assert (pipe.unet._plan.kind if pipe.unet._plan is not None else None) == kind
        try:
            lat, _ = editor(prompt=PROMPTS, latents=x_T.clone(), guidance_scale=7.5, num_inference_steps=steps, height=size,
                            width=size, return_latents=True)
        finally:
            unreg(pipe, c)
        assert c.cur_step == steps
        return lat.float().cpu()

    kw = dict(layer_idx=layers, total_steps=steps)
    plain_f = run(MutualSelfAttentionControl(1, 2, **kw), "masactrl")
    plain_g = run(PlainOnTheGenericPath(1, 2, **kw), None)
    mask_f = run(MutualSelfAttentionControlMask(1, 2, mask_s=ms, mask_t=mt, **kw), "masactrl_mask")
    mask_g = run(MaskOnTheGenericPath(1, 2, mask_s=ms, mask_t=mt, **kw), None)
    yard, e = rel_err(plain_f, plain_g), rel_err(mask_f, mask_g)
    effect = rel_err(mask_f[1:], plain_f[1:])
    print(f"fused vs generic after {steps} steps: plain mutual attention {yard:.3e} (yardstick), mask-guided {e:.3e}; "
          f"the masks move the target latents by {effect:.3e}")
    assert rel_err(mask_f[:1], plain_f[:1]) <= 2 * yard, "the source row attends to itself either way"
    assert e <= 2 * yard
    assert effect > 100 * 2 * yard

    # the captured step graph against eager stepping of the same fused plan: bit for bit
    context = torch.cat([pipe.text_encoder(pipe.tokenizer([""] * 2, padding="max_length", max_length=pipe.tokenizer.model_max_length,
                                                          return_tensors="pt").input_ids.to(DEV))[0],
                         pipe.text_encoder(pipe.tokenizer(PROMPTS, padding="max_length", max_length=pipe.tokenizer.model_max_length,
                                                          return_tensors="pt").input_ids.to(DEV))[0]])
    lats = {}
    for use_graph in (True, False):
        c = MutualSelfAttentionControlMask(1, 2, mask_s=ms, mask_t=mt, **kw)
        regiter_attention_editor_diffusers(pipe, c)
        pipe.scheduler.set_timesteps(steps)
        loop = FusedDenoiser(pipe, context, 2, (cfg.sample_size, cfg.sample_size), 7.5, use_graph=use_graph)
        try:
            lats[use_graph] = loop.run(x_T.clone()).float().cpu()
        finally:
            loop.release()
            unreg(pipe, c)
        assert c.cur_step == steps
    assert torch.equal(lats[True], lats[False]), "captured-graph replay must equal eager stepping bit for bit"
    assert torch.equal(lats[True], mask_f)
