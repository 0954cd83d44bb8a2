"""MasaCtrl Union on a real MI355X: the two-segment instantiation of the planes attention (`attn_flash_x3p_kernel<.., UNI>`,
csrc/split_x3.hip) and the fused plan kind 'masactrl_union' end to end.

The launch under test: B = 4 rows [u_src, u_tgt, c_src, c_tgt], k_src = v_src = [0, 0, 2, 2], k2_src = v2_src = [-1, 1, -1, 3] -- a
target row runs ONE softmax over its half's source keys followed by its own, a source row over its own keys only.

Stated tolerances (every test prints what it measured):
    two-segment launch vs fp64 attention over the concatenated keys     <= 4e-6 of max |reference| -- the bound tests/test_gpu_x3p.py
                                                                           holds the plain planes attention to at every head dim
    target rows vs the plain launch on physically concatenated K / V    bit for bit (L a multiple of the key tile: same tiles, same
                                                                           order, same arithmetic)
    rows without a second segment vs the plain k_src launch             bit for bit
    a refused call                                                      its error code, the sentinel-filled output unchanged
    fused plan vs the same editor on the generic path (latents after 4 steps, `small` family, f16x3)
                                                                        <= 2 x the same distance for plain MutualSelfAttentionControl,
                                                                           measured in the same test
    source-row latents, Union vs plain mutual editor                    bit for bit (the source rows never see either control)
    captured step graph vs eager stepping; a re-pointed pooled loop vs that editor's fresh run      bit for bit

The inputs are conditioned so that a kernel ignoring a segment cannot pass: on the fp64 reference every target query has between 0.2
and 0.8 of its softmax mass in the second segment (unit Gaussians from `torch.Generator().manual_seed(1234 + d + L)`; on the
host these shapes gave 0.30 .. 0.73, mean 0.50).
"""
import functools
from ctypes import byref

import pytest
import torch

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip, planes  # noqa: E402

XTOL = 4e-6          # tests/test_gpu_x3p.py: planes attention vs fp64
DEV = torch.device("cuda:0")
SENTINEL = -7.25     # exactly representable in fp16
B, HEADS = 4, 2
K1, K2 = [0, 0, 2, 2], [-1, 1, -1, 3]


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(autouse=True)
def _x3():
    with hip.f32_contraction("x3"):
        yield


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(d, L):
    """seeded unit Gaussian q, k, v [4, L, heads * d] (host fp32) and the fp64 reference of the launch under test, with the share
    of every target query's softmax mass that lies in the second segment; made once per shape and not modified"""
    C = HEADS * d
    g = torch.Generator().manual_seed(1234 + d + L)
    q, k, v = (torch.randn(B, L, C, generator=g) for _ in range(3))
    heads = lambda t: t.double().reshape(-1, HEADS, d).permute(1, 0, 2)       # [rows, C] -> [h, rows, d]
    ref, mass = torch.empty(B, L, C, dtype=torch.float64), []
    for b in range(B):
        rows = [K1[b]] + ([K2[b]] if K2[b] >= 0 else [])
        kk, vv = torch.cat([heads(k[r]) for r in rows], 1), torch.cat([heads(v[r]) for r in rows], 1)
        p = torch.softmax(heads(q[b]) @ kk.transpose(1, 2) * d ** -0.5, -1)
        ref[b] = (p @ vv).permute(1, 0, 2).reshape(L, C)
        if K2[b] >= 0:
            mass.append(p[..., L:].sum(-1))
    mass = torch.stack(mass)
    return (q, k, v), ref, (mass.min().item(), mass.max().item())


def _planes(q, k, v):
    C = q.shape[-1]
    qkv = planes.split(torch.cat([q, k, v], -1).to(DEV))
    return qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]


def _union(qp, kp, vp, d, k2=K2):
    return planes.attn_flash(qp, kp, vp, HEADS, d ** -0.5, k_src=_i32(K1), v_src=_i32(K1), k2_src=_i32(k2), v2_src=_i32(k2),
                             out_planes=False)


# d = 40: 64-key tiles, 256 queries per workgroup -- one tile per segment (the prologue's tile is followed at once by a second-segment
# tile), an even and an odd tile count (the double buffer's parity at the switch), a tail of 36 keys INSIDE the walk, two query
# blocks with the second partial.  d = 64 / 80: 32-key tiles -- one tile, odd, even, a tail of 4 keys
SHAPES = [(40, 64), (40, 128), (40, 192), (40, 100), (40, 320)] + [(d, L) for d in (64, 80) for L in (32, 96, 128, 100)]


@pytest.mark.parametrize("d,L", SHAPES)
def test_two_segment_launch_vs_fp64(d, L):
    (q, k, v), ref, (lo, hi) = _case(d, L)
    print(f"d={d} L={L}: second segment holds {lo:.2f} .. {hi:.2f} of a target query's softmax mass")
    assert 0.2 <= lo and hi <= 0.8, "the inputs must make both segments matter to every target query"
    out = _union(*_planes(q, k, v), d)
    e_src, e_tgt = rel_err(out[0::2], ref[0::2]), rel_err(out[1::2], ref[1::2])
    print(f"d={d} L={L}: two-segment launch vs fp64: source rows {e_src:.2e}, target rows {e_tgt:.2e}")
    assert max(e_src, e_tgt) <= XTOL


@pytest.mark.parametrize("d,L", [(40, 64), (40, 128), (40, 192), (64, 32), (64, 96), (80, 96), (80, 128)])
def test_target_rows_equal_plain_launch_on_concatenated_keys(d, L):
    (q, k, v), _, _ = _case(d, L)
    out = _union(*_planes(q, k, v), d)
    for src, tgt in ((0, 1), (2, 3)):
        qp, kp, vp = (planes.split(t.to(DEV)) for t in (q[tgt:tgt + 1].contiguous(), torch.cat([k[src], k[tgt]])[None].contiguous(),
                                                        torch.cat([v[src], v[tgt]])[None].contiguous()))
        cat = planes.attn_flash(qp, kp, vp, HEADS, d ** -0.5, out_planes=False)
        assert cat.shape == (1, L, HEADS * d)
        assert torch.equal(out[tgt], cat[0]), f"row {tgt}: the same tiles in the same order must give the same bits"


@pytest.mark.parametrize("d,L", [(40, 100), (40, 320), (64, 100), (80, 96)])
def test_rows_without_second_segment_equal_plain_launch(d, L):
    (q, k, v), _, _ = _case(d, L)
    qp, kp, vp = _planes(q, k, v)
    plain = planes.attn_flash(qp, kp, vp, HEADS, d ** -0.5, k_src=_i32(K1), v_src=_i32(K1), out_planes=False)
    out = _union(qp, kp, vp, d)
    assert torch.equal(out[0::2], plain[0::2]), "rows 0 and 2 walk the first segment only"
    assert not torch.equal(out[1::2], plain[1::2])
    none = _union(qp, kp, vp, d, k2=[-1, -1, -1, -1])
    assert torch.equal(none, plain), "k2_src all -1: the plain k_src launch on all rows"
    # the planes output of the two-segment launch is the split of its fp32 output
    op = planes.attn_flash(qp, kp, vp, HEADS, d ** -0.5, k_src=_i32(K1), v_src=_i32(K1), k2_src=_i32(K2), v2_src=_i32(K2))
    hi = out.half()
    assert torch.equal(op.hi, hi) and torch.equal(op.lo, (out - hi.float()).half())


def test_binding_refusals():
    (q, k, v), _, _ = _case(40, 64)
    qp, kp, vp = _planes(q, k, v)
    k2, sc = _i32(K2), 40 ** -0.5
    idx = torch.arange(64, dtype=torch.int32, device=DEV)
    words = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.full((B, 64, 80), SENTINEL, device=DEV)
    with pytest.raises(ValueError, match="go together"):
        planes.attn_flash(qp, kp, vp, HEADS, sc, k2_src=k2, out=out, out_planes=False)
    with pytest.raises(ValueError, match="go together"):
        planes.attn_flash(qp, kp, vp, HEADS, sc, v2_src=k2, out=out, out_planes=False)
    for kw in (dict(lse=torch.zeros(B, HEADS, 64, device=DEV)), dict(key_splits=2), dict(q_idx=idx, k_idx=idx),
               dict(q_cls=words, k_cls=words)):
        with pytest.raises(ValueError, match="two-segment"):
            planes.attn_flash(qp, kp, vp, HEADS, sc, k2_src=k2, v2_src=k2, out=out, out_planes=False, **kw)
    with pytest.raises(ValueError, match="one entry per batch row"):
        planes.attn_flash(qp, kp, vp, HEADS, sc, k2_src=k2[:2].contiguous(), v2_src=k2, out=out, out_planes=False)
    with pytest.raises(TypeError):
        planes.attn_flash(qp, kp, vp, HEADS, sc, k2_src=k2.long(), v2_src=k2, out=out, out_planes=False)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


def test_library_refusals_launch_nothing():
    lib = hip.load()
    d, L = 40, 64
    C = HEADS * d
    (q, k, v), _, _ = _case(d, L)
    qp, kp, vp = _planes(q, k, v)
    out = torch.full((B, L, C), SENTINEL, device=DEV)
    k1, k2 = _i32(K1), torch.tensor(K2 + [0], dtype=torch.int32, device=DEV)[:B]
    idx = torch.arange(L, dtype=torch.int32, device=DEV)
    words = torch.zeros(L // 32, dtype=torch.int32, device=DEV)
    lse = torch.zeros(B, HEADS, L, device=DEV)
    ws = torch.empty(lib.ief_attn_flash_ws_floats(B, HEADS, L, L, d, 2) + 4, device=DEV)
    keep = []

    def params(planes_in=True):
        p = hip.IefAttnF32Params()
        if planes_in:
            for t, nm in ((qp, "Q"), (kp, "K"), (vp, "V")):
                setattr(p, nm + "p", t.hi.data_ptr())
                setattr(p, "plane" + nm, t.plane)
            p.ldq = p.ldk = p.ldv = 3 * C
            p.sQb = p.sKb = p.sVb = L * 3 * C
        else:
            qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
            keep.extend((qd, kd, vd))
            p.Q, p.K, p.V = qd.data_ptr(), kd.data_ptr(), vd.data_ptr()
            p.ldq = p.ldk = p.ldv = C
            p.sQb = p.sKb = p.sVb = L * C
        p.B, p.heads, p.N, p.L, p.d, p.scale = B, HEADS, L, L, d, d ** -0.5
        p.x3, p.zeros = 1, planes._zeros(DEV)
        p.Out, p.sOb, p.ldo = out.data_ptr(), L * C, C
        p.k_src, p.v_src, p.k2_src, p.v2_src = k1.data_ptr(), k1.data_ptr(), k2.data_ptr(), k2.data_ptr()
        return p

    call = lambda p: lib.ief_attn_flash_f32(byref(p), hip._stream())
    EINVAL, ESHAPE, EALIGN = -1, -2, -3
    p = params()
    p.v2_src = None
    assert call(p) == EINVAL, "k2_src without v2_src"
    p = params()
    p.k2_src = None
    assert call(p) == EINVAL, "v2_src without k2_src"
    p = params()
    p.lse = lse.data_ptr()
    assert call(p) == EINVAL, "with lse"
    p = params()
    p.key_splits, p.ws, p.ws_floats = 2, ws.data_ptr(), ws.numel()
    assert call(p) == EINVAL, "with key_splits = 2"
    p = params()
    p.q_idx, p.k_idx = idx.data_ptr(), idx.data_ptr()
    assert call(p) == EINVAL, "with lists"
    p = params()
    p.q_cls, p.k_cls = words.data_ptr(), words.data_ptr()
    assert call(p) == EINVAL, "with class words"
    assert call(params(planes_in=False)) == EINVAL, "without Qp"
    p = params()
    p.x3 = 0
    assert call(p) == EINVAL, "with x3 == 0"
    for nm in ("k2_src", "v2_src"):
        p = params()
        setattr(p, nm, k2.data_ptr() + 2)
        assert call(p) == EALIGN, f"{nm} off the 4-byte grid"
    p = params()
    p.d, p.heads = 32, 2
    assert call(p) == ESHAPE, "head dim 32 has no planes instantiation"
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call must not launch"
    assert call(params()) == 0
    torch.cuda.synchronize()
    assert (out != SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------- whole sampler
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]


@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.pipeline import StableDiffusionPipeline
    return StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")


def test_fused_plan_vs_generic_path_graph_and_pool(small_x3, capsys):
    from ief_amd import denoise
    from ief_amd.denoise import FusedDenoiser
    from ief_amd.masactrl.model.attention_control import MutualSelfAttentionControl, MutualSelfAttentionControlUnion
    from ief_amd.masactrl.model.register import regiter_attention_editor_diffusers, unregister_attention_control as unreg
    from ief_amd.masactrl.model.sd_utils import MasaCtrl

    class PlainOnTheGenericPath(MutualSelfAttentionControl):       # lowering goes by class name: a subclass is an unknown editor
        pass

    class UnionOnTheGenericPath(MutualSelfAttentionControlUnion):
        pass

    pipe = small_x3
    cfg = pipe.cfg
    steps, layers = 4, list(range(2, 11))       # `small`: 11 transformer layers, head dims 40 (32 x 32 tokens) and 80 (16 x 16)
    size = cfg.sample_size * 8
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
    capsys.readouterr()
    union_f = run(MutualSelfAttentionControlUnion(1, 2, **kw), "masactrl_union")
    assert "takes the generic path" not in capsys.readouterr().out
    union_g = run(UnionOnTheGenericPath(1, 2, **kw), None)
    yard, e = rel_err(plain_f, plain_g), rel_err(union_f, union_g)
    effect = rel_err(union_f[1:], plain_f[1:])
    print(f"fused vs generic after {steps} steps: plain mutual attention {yard:.3e} (yardstick), Union {e:.3e}; "
          f"the target's own keys move the target latents by {effect:.3e}")
    assert e <= 2 * yard
    assert effect > 100 * 2 * yard, "a plan that ignored the second segment would be plain mutual attention"
    assert torch.equal(union_f[:1], plain_f[:1]), "the source rows never see the control in either editor"

    # the captured step graph against eager stepping of the same fused plan: bit for bit
    context = torch.cat([pipe.text_encoder(pipe.tokenizer([""] * 2, padding="max_length", max_length=pipe.tokenizer.model_max_length,
                                                          return_tensors="pt").input_ids.to(DEV))[0],
                         pipe.text_encoder(pipe.tokenizer(PROMPTS, padding="max_length", max_length=pipe.tokenizer.model_max_length,
                                                          return_tensors="pt").input_ids.to(DEV))[0]])

    def fused_loop(c, use_graph, pooled=False):
        regiter_attention_editor_diffusers(pipe, c)
        pipe.scheduler.set_timesteps(steps)
        assert pipe.unet._plan.kind == "masactrl_union"
        hw = (cfg.sample_size, cfg.sample_size)
        loop = denoise.acquire(pipe, context, 2, hw, 7.5, use_graph=True) if pooled else FusedDenoiser(pipe, context, 2, hw, 7.5, use_graph=use_graph)
        try:
            lat = loop.run(x_T.clone()).float().cpu()
        finally:
            loop.release()
            unreg(pipe, c)
        assert c.cur_step == steps
        return lat, loop

    eager, _ = fused_loop(MutualSelfAttentionControlUnion(1, 2, **kw), False)
    denoise.drop_pool()
    graph, loop1 = fused_loop(MutualSelfAttentionControlUnion(1, 2, **kw), True, pooled=True)
    assert torch.equal(graph, eager), "captured-graph replay must equal eager stepping bit for bit"
    assert torch.equal(graph, union_f)
    # the pooled loop re-pointed at an editor with another step_idx of equal table length gives that editor's eager result
    kw2 = dict(layer_idx=layers, step_idx=[0, 3], total_steps=steps)
    eager2, _ = fused_loop(MutualSelfAttentionControlUnion(1, 2, **kw2), False)
    pooled2, loop2 = fused_loop(MutualSelfAttentionControlUnion(1, 2, **kw2), True, pooled=True)
    assert loop2 is loop1 and loop2.graph is not None, "equal signatures: the captured loop is taken from the pool, not rebuilt"
    print(f"second editor moves the latents by {rel_err(eager2[1:], eager[1:]):.3e} against the first")
    assert not torch.equal(eager2, eager), "the second editor must be a different edit"
    assert torch.equal(pooled2, eager2), "a re-pointed pooled loop must give the new editor's result"
    denoise.drop_pool()
