"""MasaCtrl with masks from cross-attention on a real MI355X: the token-mass kernel (`ief_cross_token_mass_f32`), the class kernel
(`ief_masa_auto_classes`), the class-masked instantiation of the planes attention (`attn_flash_x3p_kernel<.., CLS>`) and the fused
plan kind 'masactrl_mask_auto' end to end.

Stated tolerances (every test prints what it measured):
    token mass vs fp64                      <= 4 x the distance of the same quantity computed by torch in fp32 on the CPU from the
                                               same inputs (the yardstick; the summation orders differ).  Distances are max |x - ref|
                                               / max |ref|.  Measured on an MI355X: see the docstring of test_token_mass_vs_fp64
    class bits vs the fp64 restatement      equal, with an empty set of pixels whose normalised value lies within 1e-5 of thres (the
                                               test computes that set first and FAILS if it is not empty)
    class-masked launch vs fp64 attention of each target query over the source keys of its class
                                            <= 4e-6 of max |reference| -- the bound tests/test_gpu_x3p.py holds the plain planes
                                               attention to at every head dim
    batch rows that are not targets, and everything while the gate holds 0: bit-unchanged
    fused plan vs the same editor on the generic path (latents after 4 steps, `small` family, f16x3)
                                            <= 2 x the same distance for plain MutualSelfAttentionControl, measured in the same
                                               test (tests/test_gpu_masactrl_mask.py); class bits equal at every (step, layer)
    captured step graph vs eager stepping, and a pooled loop re-pointed at another editor vs that editor's eager run: bit for bit
"""
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip, planes  # noqa: E402

XTOL = 4e-6          # tests/test_gpu_x3p.py: planes attention vs fp64
DEV = torch.device("cuda:0")
SENTINEL = -7.25     # exactly representable in fp16: hi = -7.25, lo = 0
L = 77


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(autouse=True)
def _x3():
    with hip.f32_contraction("x3"):
        yield


def _weights(ref, cur):
    w = torch.zeros(2, L)
    for r, idx in enumerate((ref, cur)):
        for i in idx:
            w[r, i] += 1
    return w


# ------------------------------------------------------------------------------------------------------------- kernel (2)
def _mass(q, k, heads, w, rows, dtype):
    """out[r][n] = (1 / heads) sum_h sum_l w[r][l] softmax_l(scale q_h[rows[r]][n] . k_h[rows[r]][l]) by torch, in `dtype`"""
    B, N, C = q.shape
    d = C // heads
    out = []
    for r, row in enumerate(rows):
        qh = q[row].to(dtype).reshape(N, heads, d).permute(1, 0, 2)
        kh = k[row].to(dtype).reshape(-1, heads, d).permute(1, 0, 2)
        p = (qh @ kh.transpose(1, 2) * d ** -0.5).softmax(-1)            # [heads, N, L]
        out.append((p * w[r].to(dtype)).sum(-1).mean(0))
    return torch.stack(out)


@pytest.mark.parametrize("heads,d,ref,cur", [
    (8, 80, [1, 2, 2], [3]),                  # `small`'s 16 x 16 level; a token listed twice
    (8, 160, [1], [4, 5, 6, 9, 12]),          # SD1.5's 16 x 16 level; several tokens
    (2, 80, [76, 0], [5, 5, 5]),              # two heads; the first and the last token
])
def test_token_mass_vs_fp64(heads, d, ref, cur):
    """measured on an MI355X, max |x - fp64| / max |fp64| (kernel / torch fp32 on the CPU):
        heads 8, d 80:  2.588e-07 / 2.338e-07        heads 8, d 160:  2.955e-07 / 2.955e-07        heads 2, d 80:  5.382e-07 / 5.382e-07"""
    B, N, C = 4, 256, heads * d
    q, kv = f32(B, N, C, seed=1), f32(B, L, 2 * C, seed=2)
    k = kv[..., :C]
    w = _weights(ref, cur)
    rows = (2, 3)
    want = _mass(q, k, heads, w, rows, torch.float64)
    yard = rel_err(_mass(q, k, heads, w, rows, torch.float32), want)
    kvd = kv.to(DEV)
    buf = torch.full((3, 2, N), SENTINEL, device=DEV)
    hip.cross_token_mass(q.to(DEV), kvd[..., :C], heads, d ** -0.5, rows, w.to(DEV), buf[1])
    torch.cuda.synchronize()
    e = rel_err(buf[1], want)
    print(f"token mass heads={heads} d={d}: kernel {e:.3e}, torch fp32 on the CPU {yard:.3e} (bound 4 x), max |ref| {want.abs().max():.3e}")
    assert (buf[0] == SENTINEL).all() and (buf[2] == SENTINEL).all(), "one slot is written, its neighbours are not"
    assert e <= 4 * yard


def test_token_mass_refusals_launch_nothing():
    lib = hip.load()
    heads, d, N = 2, 80, 256
    C = heads * d
    q, k, w = f32(4, N, C, seed=1).to(DEV), f32(4, L, C, seed=2).to(DEV), _weights([1], [1]).to(DEV)
    out = torch.full((2, N), SENTINEL, device=DEV)

    def call(qp=None, kp=None, wp=None, op=None, dd=d, ll=L, ldq=C):
        return lib.ief_cross_token_mass_f32(q.data_ptr() if qp is None else qp, k.data_ptr() if kp is None else kp,
                                            w.data_ptr() if wp is None else wp, out.data_ptr() if op is None else op, 2, 3, heads, N,
                                            ll, dd, ldq, C, N * C, L * C, d ** -0.5, hip._stream())

    assert call(qp=q.data_ptr() + 4) == -3, "q off the 16-byte grid: IEF_EALIGN"
    assert call(kp=k.data_ptr() + 8) == -3
    assert call(op=out.data_ptr() + 2) == -3
    assert call(ldq=C + 2) == -3
    assert call(dd=84) == -2, "head dim no multiple of 8: IEF_ESHAPE"
    assert call(ll=129) == -2
    assert lib.ief_cross_token_mass_f32(None, k.data_ptr(), w.data_ptr(), out.data_ptr(), 2, 3, heads, N, L, d, C, C, N * C, L * C,
                                        d ** -0.5, hip._stream()) == -1
    with pytest.raises(TypeError):            # a host tensor never reaches the library
        hip.cross_token_mass(q.cpu(), k, heads, d ** -0.5, (2, 3), w, out)
    with pytest.raises(TypeError):
        hip.cross_token_mass(q, k, heads, d ** -0.5, (2, 3), w.cpu(), out)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call must not launch"
    assert call() == 0
    torch.cuda.synchronize()
    assert (out != SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------- kernel (3)
@pytest.fixture(scope="module")
def six_slots():
    """six slots [6, 2, 256] of token mass from Gaussian q / k (8 heads, d = 80, seeds 0-5), computed in fp64 and rounded to fp32
    once: the kernel and the restatement start from the same fp32 numbers"""
    heads, d = 8, 80
    w = _weights([1, 2, 2], [3])
    slots = [_mass(f32(4, 256, heads * d, seed=s), f32(4, L, heads * d, seed=100 + s), heads, w, (2, 3), torch.float64) for s in range(6)]
    return torch.stack(slots).float()


def _classes64(slots, c, thres, res):
    """the rule in fp64 from fp32 slots -> (key bits, query bits [res*res] bool, smallest |normalised - thres|, fg pixel counts)"""
    img = slots[:c].double().sum(0) / c                                   # [2, 256]
    lo, hi = img.amin(1, keepdim=True), img.amax(1, keepdim=True)
    img = ((img - lo) / (hi - lo)).reshape(2, 16, 16)
    gap = (img - thres).abs().min().item()
    near = int(((img - thres).abs() <= 1e-5).sum())
    bits = F.interpolate(img[None], (res, res))[0] >= thres
    return bits[0].flatten(), bits[1].flatten(), gap, near, (img >= thres).sum((1, 2)).tolist()


@pytest.mark.parametrize("res", [16, 32, 64])
@pytest.mark.parametrize("c", [1, 3, 6])
def test_class_bits_vs_fp64_restatement(six_slots, c, res):
    slots = six_slots.clone()
    slots[c:] = float("nan")                  # the slots beyond c hold garbage and must be ignored
    sd = slots.to(DEV)
    n = res * res
    for thres in (0.1, 0.3, 0.5):
        kb, qb, gap, near, fg = _classes64(six_slots, c, thres, res)
        assert near == 0, f"test inputs: {near} pixels lie within 1e-5 of thres {thres} (smallest gap {gap:.1e})"
        kc = torch.full((n // 32,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        qc = kc.clone()
        hip.masa_auto_classes(sd, c, torch.tensor([thres], device=DEV), res, kc, qc)
        torch.cuda.synchronize()
        gk, gq = hip.unpack_class_bits(kc, n), hip.unpack_class_bits(qc, n)
        print(f"classes c={c} res={res} thres={thres}: fg pixels key {fg[0]} / query {fg[1]} of 256, smallest gap {gap:.1e}, "
              f"mismatched bits {int((gk != kb).sum())} + {int((gq != qb).sum())}")
        assert torch.equal(gk, kb) and torch.equal(gq, qb)


def test_class_kernel_gate_degenerate_row_and_refusals(six_slots):
    lib = hip.load()
    sd = six_slots.to(DEV)
    thres = torch.tensor([0.3], device=DEV)
    kc = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    qc = kc.clone()
    gate = torch.zeros(1, dtype=torch.int32, device=DEV)
    hip.masa_auto_classes(sd, 3, thres, 16, kc, qc, gate=gate)
    torch.cuda.synchronize()
    assert (kc == 0x5A5A5A5A).all() and (qc == 0x5A5A5A5A).all(), "gate = 0: nothing may be written"
    flat = sd.clone()
    flat[:, 0] = 0.25                         # a key row that is constant over the image: max == min
    hip.masa_auto_classes(flat, 3, thres, 16, kc, qc)
    torch.cuda.synchronize()
    assert (kc == 0).all() and (qc == 0).all(), "a degenerate row makes every token of both rows background"
    for rc, args in ((-2, (sd.data_ptr(), 0, thres.data_ptr(), 16)), (-2, (sd.data_ptr(), 3, thres.data_ptr(), 12)),
                     (-1, (None, 3, thres.data_ptr(), 16)), (-3, (sd.data_ptr() + 2, 3, thres.data_ptr(), 16))):
        kc.fill_(7)
        assert lib.ief_masa_auto_classes(*args, kc.data_ptr(), qc.data_ptr(), None, hip._stream()) == rc
        torch.cuda.synchronize()
        assert (kc == 7).all(), "a refused call must not launch"


# ------------------------------------------------------------------------------------------------------------- kernel (4)
def _operands(B, heads, N, d):
    """Gaussian q / k / v at the scales of test_gpu_x3p.py's attention test, as column slices of one q|k|v planes tensor"""
    C = heads * d
    q, k, v = f32(B, N, C, seed=1), f32(B, N, C, seed=2, scale=1.5), f32(B, N, C, seed=3)
    qkv = planes.split(torch.cat([q, k, v], -1).to(DEV))
    return (q, k, v), (qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:])


def _ref64_classes(q, k, v, heads, d, qbits, kbits, tgt, src):
    """fp64 attention of every query of batch rows `tgt` over the keys of ITS class in batch rows `src` -> [len(tgt), N, C]"""
    N, C = q.shape[1], heads * d
    out = torch.empty(len(tgt), N, C, dtype=torch.float64)
    for i, (bt, bs) in enumerate(zip(tgt, src)):
        qh = q[bt].double().reshape(N, heads, d).permute(1, 0, 2)
        kh = k[bs].double().reshape(N, heads, d).permute(1, 0, 2)
        vh = v[bs].double().reshape(N, heads, d).permute(1, 0, 2)
        s = qh @ kh.transpose(1, 2) * d ** -0.5
        s = s.masked_fill(qbits[:, None] != kbits[None, :], float("-inf"))
        out[i] = (s.softmax(-1) @ vh).permute(1, 0, 2).reshape(N, C)
    return out


def _bits(n, frac, seed):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed)) < frac


def _case(name, N):
    kb, qb = torch.zeros(N, dtype=torch.bool), _bits(N, 0.3, 12)
    if name == "random":
        kb = _bits(N, 0.3, 11)
    elif name == "last40":            # every earlier key tile is fully masked for the fg queries, the first one included
        kb[-40:] = True
    elif name == "tile":              # one whole tile is fg; a whole tile masked in the middle for the bg queries
        kb[64:128] = True
    elif name == "single":
        kb[100] = True
    else:                             # no query is fg: the fg keys are dropped by everybody
        kb, qb = _bits(N, 0.3, 11), torch.zeros(N, dtype=torch.bool)
    return kb, qb


TGT, SRC = [1, 3], [0, 2]


def _cls_launch(ops, heads, d, qb, kb, out, op, gate=None):
    qp, kp, vp = ops
    i32 = lambda l: torch.tensor(l, dtype=torch.int32, device=DEV)
    return planes.attn_flash(qp, kp, vp, heads, d ** -0.5, q_src=i32(TGT), k_src=i32(SRC), v_src=i32(SRC), out=out[1::2],
                             out_planes=op[1::2], q_cls=hip.pack_class_bits(qb, DEV), k_cls=hip.pack_class_bits(kb, DEV), gate=gate)


@pytest.mark.parametrize("name,N,d", [("random", 256, 40), ("last40", 1024, 80), ("tile", 256, 64), ("single", 256, 40),
                                      ("no_fg_query", 256, 80)])
def test_class_masked_launch_vs_fp64(name, N, d):
    B, heads = 4, 2
    C = heads * d
    (q, k, v), ops = _operands(B, heads, N, d)
    kb, qb = _case(name, N)
    out = torch.full((B, N, C), SENTINEL, device=DEV)
    op = planes.split(out)
    out0, op0 = out.clone(), op.t.clone()
    gate = torch.zeros(1, dtype=torch.int32, device=DEV)
    _cls_launch(ops, heads, d, qb, kb, out, op, gate=gate)
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(op.t, op0), "gate = 0: nothing may be written"
    gate.fill_(1)
    _cls_launch(ops, heads, d, qb, kb, out, op, gate=gate)
    torch.cuda.synchronize()
    ref = _ref64_classes(q, k, v, heads, d, qb, kb, TGT, SRC)
    e = rel_err(out[1::2], ref)
    print(f"class-masked {name} d={d} N={N}: fg keys {int(kb.sum())}, fg queries {int(qb.sum())}: {e:.2e}")
    assert e < XTOL
    assert torch.equal(out[0::2], out0[0::2]) and torch.equal(op.t[:, 0::2], op0[:, 0::2]), "rows that are no targets stay as they were"
    hi = out[1::2].half()
    assert torch.equal(op.hi[1::2], hi) and torch.equal(op.lo[1::2], (out[1::2] - hi.float()).half()), "planes written == split of the fp32 output"


@pytest.mark.parametrize("d", [40, 64, 80])
def test_all_background_classes_vs_plain_source_launch(d):
    B, heads, N = 4, 2, 256
    C = heads * d
    (q, k, v), ops = _operands(B, heads, N, d)
    none = torch.zeros(N, dtype=torch.bool)
    out = torch.full((B, N, C), SENTINEL, device=DEV)
    _cls_launch(ops, heads, d, none, none, out, planes.split(out))
    src = torch.tensor([0, 0, 2, 2], dtype=torch.int32, device=DEV)
    plain = planes.attn_flash(*ops, heads, d ** -0.5, k_src=src, v_src=src, out_planes=False)
    ref = _ref64_classes(q, k, v, heads, d, none, none, TGT, SRC)
    e, e_plain = rel_err(out[1::2], ref), rel_err(plain[1::2], ref)
    print(f"all-background classes d={d}: class-masked {e:.2e}, plain k_src launch {e_plain:.2e}, bit-equal: "
          f"{torch.equal(out[1::2], plain[1::2])}")
    assert e < XTOL and e_plain < XTOL


def test_class_masked_refusals_launch_nothing():
    lib = hip.load()
    B, heads, N, d = 2, 2, 128, 40
    C = heads * d
    _, (qp, kp, vp) = _operands(B, heads, N, d)
    out = torch.full((B, N, C), SENTINEL, device=DEV)
    words = torch.zeros(N // 32 + 1, dtype=torch.int32, device=DEV)
    idx = torch.arange(N, dtype=torch.int32, device=DEV)
    lse = torch.zeros(B, heads, N, device=DEV)

    def params(n=N):
        p = hip.IefAttnF32Params()
        for t, nm in ((qp, "Q"), (kp, "K"), (vp, "V")):
            setattr(p, nm + "p", t.hi.data_ptr())
            setattr(p, "plane" + nm, t.plane)
        p.ldq = p.ldk = p.ldv = 3 * C
        p.sQb = p.sKb = p.sVb = N * 3 * C
        p.B, p.heads, p.N, p.L, p.d, p.scale = B, heads, n, N, d, d ** -0.5
        p.x3, p.zeros = 1, planes._zeros(DEV)
        p.Out, p.sOb, p.ldo = out.data_ptr(), N * C, C
        p.q_cls, p.k_cls = words.data_ptr(), words.data_ptr()
        return p

    call = lambda p: lib.ief_attn_flash_f32(byref(p), hip._stream())
    assert call(params(n=N - 8)) == -1, "N no multiple of 32: IEF_EINVAL"
    p = params()
    p.k_cls = None
    assert call(p) == -1, "a missing class pointer: IEF_EINVAL"
    p = params()
    p.q_cls = None
    assert call(p) == -1
    p = params()
    p.lse = lse.data_ptr()
    assert call(p) == -1, "lse with classes: IEF_EINVAL"
    p = params()
    ws = torch.empty(lib.ief_attn_flash_ws_floats(B, heads, N, N, d, 2) + 4, device=DEV)
    p.key_splits, p.ws, p.ws_floats = 2, ws.data_ptr(), ws.numel()
    assert call(p) == -1, "key_splits = 2 with classes: IEF_EINVAL"
    p = params()
    p.q_idx, p.k_idx = idx.data_ptr(), idx.data_ptr()
    assert call(p) == -1, "index lists with classes: IEF_EINVAL"
    p = params()
    p.q_cls = words.data_ptr() + 2
    assert call(p) == -3, "a class pointer off the 4-byte grid: IEF_EALIGN"
    with pytest.raises(ValueError, match="go together"):
        planes.attn_flash(qp, kp, vp, heads, d ** -0.5, out=out, q_cls=words[:4])
    with pytest.raises(ValueError, match="no lists"):
        planes.attn_flash(qp, kp, vp, heads, d ** -0.5, out=out, q_cls=words[:4], k_cls=words[:4], lse=lse)
    with pytest.raises(ValueError, match="destination"):
        planes.attn_flash(qp, kp, vp, heads, d ** -0.5, q_cls=words[:4], k_cls=words[:4])
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call must not launch"
    assert call(params()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and (out != SENTINEL).any()


# ------------------------------------------------------------------------------------------------------------- whole sampler
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]


@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.pipeline import StableDiffusionPipeline
    return StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")


def test_fused_plan_vs_generic_path_graph_vs_eager_and_pooled_loop(small_x3):
    from ief_amd import denoise
    from ief_amd.denoise import FusedDenoiser
    from ief_amd.masactrl.model.attention_control import MutualSelfAttentionControl, MutualSelfAttentionControlMaskAuto
    from ief_amd.masactrl.model.register import regiter_attention_editor_diffusers, unregister_attention_control as unreg
    from ief_amd.masactrl.model.sd_utils import MasaCtrl

    class PlainOnTheGenericPath(MutualSelfAttentionControl):       # lowering goes by class name: a subclass is an unknown editor
        pass

    class AutoOnTheGenericPath(MutualSelfAttentionControlMaskAuto):
        """records (soft key mask, soft query mask) of every controlled call that had maps"""
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.seen, self._soft = {}, []

        def _layer_mask(self, img, res, name):
            self._soft.append(F.interpolate(img[None, None], (res, res))[0, 0].flatten().double().cpu())
            return super()._layer_mask(img, res, name)

        def forward(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs):
            self._soft = []
            out = super().forward(q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs)
            if self._soft:
                self.seen[(self.cur_step, self.cur_att_layer // 2)] = (tuple(self._soft), len(self.cross_attns))
            return out

    pipe = small_x3
    cfg = pipe.cfg
    steps, layers = 4, list(range(5, 11))       # `small`: 11 transformer layers; layers 5-10 see c = 3, 4, 5, 6, 6, 6 maps
    size = cfg.sample_size * 8
    g = torch.Generator().manual_seed(8888)
    x_T = torch.cat([torch.randn(1, 4, cfg.sample_size, cfg.sample_size, generator=g) for _ in range(2)]).to(DEV)
    editor = MasaCtrl(pipe, steps)
    kw = dict(layer_idx=layers, total_steps=steps)
    auto = dict(thres=0.3, ref_token_idx=[1, 2, 2], cur_token_idx=[3, 4])
    auto2 = dict(thres=0.5, ref_token_idx=[5], cur_token_idx=[1, 6, 6])

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

    plain_f = run(MutualSelfAttentionControl(1, 5, **kw), "masactrl")
    plain_g = run(PlainOnTheGenericPath(1, 5, **kw), None)
    auto_f = run(MutualSelfAttentionControlMaskAuto(1, 5, **kw, **auto), "masactrl_mask_auto")
    gen = AutoOnTheGenericPath(1, 5, **kw, **auto)
    auto_g = run(gen, None)
    assert sorted(gen.seen) == [(s, l) for s in (1, 2, 3) for l in layers]
    assert [gen.seen[(1, l)][1] for l in layers] == [3, 4, 5, 6, 6, 6], "maps collected in front of layers 5-10"

    # eager stepping of the fused plan, reading the class bits back after every controlled layer
    context = torch.cat([pipe.text_encoder(pipe.tokenizer([""] * 2, padding="max_length", max_length=pipe.tokenizer.model_max_length,
                                                          return_tensors="pt").input_ids.to(DEV))[0],
                         pipe.text_encoder(pipe.tokenizer(PROMPTS, padding="max_length", max_length=pipe.tokenizer.model_max_length,
                                                          return_tensors="pt").input_ids.to(DEV))[0]])

    def fused_loop(c, use_graph, spy=None, pooled=False):
        regiter_attention_editor_diffusers(pipe, c)
        pipe.scheduler.set_timesteps(steps)
        plan = pipe.unet._plan
        assert plan.kind == "masactrl_mask_auto"
        if spy is not None:
            inner = plan.auto_launch

            def auto_launch(B, N, attn):
                r = inner(B, N, attn)
                if r is not None and c.cur_step in plan.masa_steps:
                    torch.cuda.synchronize()
                    spy[(c.cur_step, attn._exec_index // 2)] = plan.class_bits(attn._exec_index // 2, N)
                return r
            plan.auto_launch = auto_launch
        hw = (cfg.sample_size, cfg.sample_size)
        loop = denoise.acquire(pipe, context, 2, hw, 7.5, use_graph=True) if pooled else FusedDenoiser(pipe, context, 2, hw, 7.5, use_graph=use_graph)
        try:
            lat = loop.run(x_T.clone()).float().cpu()
        finally:
            loop.release()
            unreg(pipe, c)
        assert c.cur_step == steps
        return lat, loop

    bits = {}
    eager, _ = fused_loop(MutualSelfAttentionControlMaskAuto(1, 5, **kw, **auto), False, spy=bits)
    assert sorted(bits) == sorted(gen.seen)
    for key in sorted(bits):
        (soft_k, soft_q), _ = gen.seen[key]
        for nm, got, soft in (("key", bits[key][0], soft_k), ("query", bits[key][1], soft_q)):
            want = soft >= auto["thres"]
            bad = torch.nonzero(got != want).flatten()
            assert bad.numel() == 0, (f"step {key[0]} layer {key[1]}: {nm} bit of pixel {int(bad[0])} differs; the generic path's "
                                      f"normalised value there lies {abs(float(soft[bad[0]]) - auto['thres']):.2e} from thres")
    fg = [int(bits[k][0].sum()) for k in sorted(bits)]
    print(f"class bits equal at {len(bits)} (step, layer) pairs; fg keys per pair {fg}")

    yard, e = rel_err(plain_f, plain_g), rel_err(auto_f, auto_g)
    effect = rel_err(auto_f[1:], plain_f[1:])
    print(f"fused vs generic after {steps} steps: plain mutual attention {yard:.3e} (yardstick), auto masks {e:.3e}; "
          f"the masks move the target latents by {effect:.3e}")
    assert e <= 2 * yard
    assert effect > 100 * yard

    # captured graph vs eager stepping of the same fused plan: bit for bit; the sampler's own run is the captured one
    denoise.drop_pool()
    graph, loop1 = fused_loop(MutualSelfAttentionControlMaskAuto(1, 5, **kw, **auto), True, pooled=True)
    assert torch.equal(graph, eager), "captured-graph replay must equal eager stepping bit for bit"
    assert torch.equal(graph, auto_f)
    # the pooled loop re-pointed at an editor with another thres and other token lists gives that editor's eager result
    eager2, _ = fused_loop(MutualSelfAttentionControlMaskAuto(1, 5, **kw, **auto2), False)
    pooled2, loop2 = fused_loop(MutualSelfAttentionControlMaskAuto(1, 5, **kw, **auto2), True, pooled=True)
    assert loop2 is loop1 and loop2.graph is not None, "equal signatures: the captured loop is taken from the pool, not rebuilt"
    print(f"second editor moves the latents by {rel_err(eager2[1:], eager[1:]):.3e} against the first")
    assert not torch.equal(eager2, eager), "the second editor must be a different edit"
    assert torch.equal(pooled2, eager2), "a re-pointed pooled loop must give the new editor's result"
    denoise.drop_pool()
