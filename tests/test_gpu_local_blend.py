"""Prompt-to-Prompt LocalBlend on a real MI355X: the blend-mass kernel (`ief_cross_blend_mass_f32`), the blend kernel
(`ief_local_blend_f32`) and an edit controller with a `LocalBlend` lowered to the fused 'p2p' plan, end to end.

Stated tolerances (every test prints what it measured):
    blend mass vs fp64                      <= 4 x the distance of the same formula computed by torch in fp32 on the CPU from the same
                                               inputs (the yardstick and factor of tests/test_gpu_masactrl_auto.py's token mass).
                                               Distances are max |x - ref| / max |ref|; two calls into one accumulator == the fp32 sum
                                               of the two single calls; rows outside the launch bit-unchanged
    mask bits vs the fp64 restatement       equal at every pixel; the test first asserts ON ITS OWN REFERENCE that the masks cover
                                               between 0.1 and 0.9 of the pixels and that no normalised value lies within 1e-3 of
                                               the threshold
    blended latents                         bit-equal to torch's x[:1] + mask * (x - x[:1]) in fp32
    fused plan vs the same controller on the generic path (latents after 4 steps, `small` family, f16x3)
                                            mask bits equal at every step (no generic-path value within 1e-4 of the threshold: a
                                            fixed-order fp32 sum of at most 5 modules x 4 steps x 8 heads of softmax terms is good to
                                            about 1e-5), latents <= 2 x the distance the two paths show for the same controller
                                            without a blend, measured in the same test
    captured step graph vs eager stepping, a pooled loop re-pointed at another blend, the same loop run twice, edit_many vs one
    call per job: bit for bit
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip  # noqa: E402
from ief_amd.control import XL  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = -7.25
L, N = 77, 256
THRES = 0.3


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max()).item()


# ------------------------------------------------------------------------------------------------------------- the two kernels
def structured_calls(heads, d, Bp, calls, seed=0):
    """[(q [2 Bp, 256, heads*d], k [2 Bp, 77, heads*d], w [Bp, 2, 96])] per call, Gaussian q / k with structure: for prompt row i
    the queries inside a disc of radius 3 + i centred at (4 + 3 i, 5 + 2 i) get 1.5 k[token 3 + i] added, per head; v_i is non-zero
    only at token 3 + i, u_i (i >= 1) only at token 3.  The prompt rows are the conditional half: batch rows Bp .. 2 Bp - 1"""
    C = heads * d
    yy, xx = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
    out = []
    for c in range(calls):
        g = torch.Generator().manual_seed(1000 * seed + c)
        q, k = torch.randn(2 * Bp, N, C, generator=g), torch.randn(2 * Bp, L, C, generator=g)
        w = torch.zeros(Bp, 2, XL)
        for i in range(Bp):
            inside = ((yy - (4 + 3 * i)) ** 2 + (xx - (5 + 2 * i)) ** 2 <= (3 + i) ** 2).flatten()
            q[Bp + i, inside] += 1.5 * k[Bp + i, 3 + i]
            w[i, 1, 3 + i] = 1.0 + 0.5 * (c % 3)
            if i >= 1:
                w[i, 0, 3] = 0.25 * (1 + c % 2)
        out.append((q, k, w))
    return out


def blend_mass(q, k, w, heads, dtype):
    """(1 / heads) sum_h (sum_l v_i[l] softmax_l(scale q_h[Bp+i] . k_h[Bp+i][l]) + sum_l u_i[l] softmax_l(scale q_h[Bp] . k_h[Bp][l]))
    by torch, in `dtype` -> [Bp, 256]"""
    Bp, d = w.shape[0], q.shape[2] // heads

    def probs(row):
        qh = q[row].to(dtype).reshape(N, heads, d).permute(1, 0, 2)
        kh = k[row].to(dtype).reshape(L, heads, d).permute(1, 0, 2)
        return (qh @ kh.transpose(1, 2) * d ** -0.5).softmax(-1)

    src = probs(Bp)
    return torch.stack([((probs(Bp + i) * w[i, 1, :L].to(dtype)).sum(-1) + (src * w[i, 0, :L].to(dtype)).sum(-1)).mean(0)
                        for i in range(Bp)])


def blend_masks(acc, thres, hw):
    """LocalBlend.__call__'s last lines restated in fp64 -> (mask bool [Bp, 1, H, W] with mask_i = mask_0 | mask_i, the normalised
    values [Bp, 256])"""
    img = acc.double().reshape(-1, 1, 16, 16)
    pooled = F.max_pool2d(img, (3, 3), (1, 1), padding=(1, 1))
    big = F.interpolate(pooled, size=hw)
    norm = big / big.max(2, keepdim=True)[0].max(3, keepdim=True)[0]
    mask = norm.gt(thres)
    small = pooled / pooled.max(2, keepdim=True)[0].max(3, keepdim=True)[0]
    return mask[:1] | mask, small.reshape(-1, 256)


SHAPES = [(8, 80, 2, 3 * 2), (8, 40, 3, 2 * 5), (2, 160, 2, 2 * 1)]      # heads, d, Bp, steps x modules; d = 160: SD1.5's 16 x 16 level
_cases = {}


def case(heads, d, Bp, calls):
    """inputs, the fp64 accumulator, the torch-fp32 yardstick and the kernel's accumulator of one shape, computed once"""
    key = (heads, d, Bp, calls)
    if key not in _cases:
        ins = structured_calls(heads, d, Bp, calls)
        ref = sum(blend_mass(q, k, w, heads, torch.float64) for q, k, w in ins)
        f32 = torch.zeros(Bp, N)
        for q, k, w in ins:
            f32 += blend_mass(q, k, w, heads, torch.float32)
        masks, norm = blend_masks(ref, THRES, (16, 16))
        cover = [float(m.double().mean()) for m in masks]
        margin = float((norm - THRES).abs().min())
        assert all(0.1 <= c <= 0.9 for c in cover), f"the reference masks cover {cover} of the pixels"
        assert margin > 1e-3, f"a reference value lies {margin:.2e} from the threshold"
        buf = torch.full((Bp + 2, N), SENTINEL, device=DEV)
        buf[1:-1] = 0
        dev = [(q.to(DEV), k.to(DEV), w.to(DEV)) for q, k, w in ins]
        for q, k, w in dev:
            hip.cross_blend_mass(q, k, heads, d ** -0.5, Bp, w, buf[1:-1])
        torch.cuda.synchronize()
        _cases[key] = dict(ins=dev, ref=ref, f32=f32, buf=buf.cpu(), cover=cover, margin=margin)
    return _cases[key]


@pytest.mark.parametrize("heads,d,Bp,calls", SHAPES)
def test_blend_mass_vs_fp64(heads, d, Bp, calls):
    """measured on an MI355X, max |x - fp64| / max |fp64| (kernel / torch fp32 on the CPU):
        heads 8, d 80, Bp 2, 6 calls:  1.097e-07 / 1.097e-07      heads 8, d 40, Bp 3, 10 calls:  1.206e-07 / 1.371e-07
        heads 2, d 160, Bp 2, 2 calls:  1.319e-07 / 1.319e-07
    the reference masks cover 0.238 / 0.430 (/ 0.652) of the pixels; nearest normalised value to the threshold 8.8e-2 / 7.6e-2 / 4.4e-2"""
    c = case(heads, d, Bp, calls)
    yard, e = rel_err(c["f32"], c["ref"]), rel_err(c["buf"][1:-1], c["ref"])
    print(f"blend mass heads={heads} d={d} Bp={Bp} calls={calls}: kernel {e:.3e}, torch fp32 on the CPU {yard:.3e} (bound 4 x); "
          f"reference masks cover {[round(x, 3) for x in c['cover']]}, nearest value to the threshold {c['margin']:.2e}")
    assert (c["buf"][0] == SENTINEL).all() and (c["buf"][-1] == SENTINEL).all(), "rows outside the launch stay as they were"
    assert e <= 4 * yard
    # two calls into one accumulator == the sum of the two calls, each into an empty one
    (q0, k0, w0), (q1, k1, w1) = c["ins"][0], c["ins"][1]
    a, b, ab = (torch.zeros(Bp, N, device=DEV) for _ in range(3))
    scale = d ** -0.5
    hip.cross_blend_mass(q0, k0, heads, scale, Bp, w0, a)
    hip.cross_blend_mass(q1, k1, heads, scale, Bp, w1, b)
    hip.cross_blend_mass(q0, k0, heads, scale, Bp, w0, ab)
    hip.cross_blend_mass(q1, k1, heads, scale, Bp, w1, ab)
    torch.cuda.synchronize()
    assert torch.equal(ab, a + b) and not torch.equal(a, b)
    # a launch over the first prompt rows only leaves the other rows of the accumulator alone; column slices of q | k | v tensors
    part = torch.full((Bp, N), SENTINEL, device=DEV)
    part[0] = 0
    C = heads * d
    qkv = torch.cat([q0, torch.zeros_like(q0)], -1)
    kv = torch.cat([k0, torch.ones_like(k0)], -1)
    hip.cross_blend_mass(qkv[..., :C], kv[..., :C], heads, scale, Bp, w0[:1].contiguous(), part[:1])
    torch.cuda.synchronize()
    assert torch.equal(part[0], a[0]) and (part[1:] == SENTINEL).all()


@pytest.mark.parametrize("hw", [(32, 32), (64, 64), (32, 48)])
@pytest.mark.parametrize("heads,d,Bp,calls", SHAPES)
def test_blend_kernel_masks_and_latents(heads, d, Bp, calls, hw):
    c = case(heads, d, Bp, calls)
    acc = c["buf"][1:-1].to(DEV)
    thres = torch.tensor([THRES], device=DEV)
    want, _ = blend_masks(c["ref"], THRES, hw)                     # [Bp, 1, H, W], from the fp64 accumulator
    # the kernel's own mask bits: latents 0 in the source row and 1 in the others come back as the mask
    ind = torch.zeros(Bp, 1, *hw, device=DEV)
    ind[1:] = 1
    hip.local_blend(acc, thres, ind)
    x = torch.randn(Bp + 1, 4, *hw, generator=torch.Generator().manual_seed(5))
    x[-1] = SENTINEL                                                # a row past the launch
    got = x.to(DEV)
    hip.local_blend(acc, thres, got[:Bp])
    torch.cuda.synchronize()
    bits = ind.cpu() != 0
    assert torch.equal(bits[1:], want[1:]), f"{int((bits[1:] != want[1:]).sum())} mask bits differ from the fp64 restatement"
    m = want.to(torch.float32)
    assert torch.equal(got[:Bp].cpu(), x[:1] + m * (x[:Bp] - x[:1])), "x[:1] + mask * (x - x[:1]) in fp32, bit for bit"
    assert torch.equal(got[0].cpu(), x[0]) and (got[-1] == SENTINEL).all()
    # a row whose accumulator is all zero (no blend word found): 0 / 0 is not greater than the threshold, so it takes the source
    # row wherever the source's own mask is false
    acc0 = acc.clone()
    acc0[-1] = 0
    got = x[:Bp].to(DEV)
    hip.local_blend(acc0, thres, got)
    torch.cuda.synchronize()
    m0 = want[0].expand(4, *hw)
    last = got[-1].cpu()
    assert torch.equal(last[~m0], x[0][~m0]) and torch.equal(last[m0], (x[0] + (x[Bp - 1] - x[0]))[m0])
    print(f"blend heads={heads} d={d} Bp={Bp} latents {hw}: {int(want[1:].sum())} of {want[1:].numel()} mask bits set, all equal")


def test_refused_arguments_launch_nothing():
    lib = hip.load()
    heads, d, Bp = 2, 80, 2
    C = heads * d
    g = torch.Generator().manual_seed(1)
    q, k = torch.randn(4, N, C, generator=g).to(DEV), torch.randn(4, L, C, generator=g).to(DEV)
    w = torch.ones(Bp, 2, XL, device=DEV)
    acc = torch.full((Bp, N), SENTINEL, device=DEV)

    def mass(qp=None, kp=None, wp=None, ap=None, dd=d, ll=L, ldq=C, bp=Bp, hh=heads, ldw=XL):
        return lib.ief_cross_blend_mass_f32(q.data_ptr() if qp is None else qp, k.data_ptr() if kp is None else kp,
                                            w.data_ptr() if wp is None else wp, acc.data_ptr() if ap is None else ap, 2, bp, hh, N,
                                            ll, ldw, dd, ldq, C, N * C, L * C, d ** -0.5, hip._stream())

    assert mass(qp=q.data_ptr() + 4) == -3, "q off the 16-byte grid: IEF_EALIGN"
    assert mass(kp=k.data_ptr() + 8) == -3
    assert mass(ap=acc.data_ptr() + 2) == -3
    assert mass(wp=w.data_ptr() + 1) == -3
    assert mass(ldq=C + 2) == -3
    assert mass(dd=84) == -2, "head dim no multiple of 8: IEF_ESHAPE"
    assert mass(ll=129) == -2
    assert mass(ldw=L - 1) == -2
    assert mass(bp=0) == -2 and mass(bp=9) == -2
    assert mass(hh=65) == -2 and mass(hh=0) == -2
    assert lib.ief_cross_blend_mass_f32(None, k.data_ptr(), w.data_ptr(), acc.data_ptr(), 2, Bp, heads, N, L, XL, d, C, C, N * C, L * C,
                                        d ** -0.5, hip._stream()) == -1
    assert lib.ief_cross_blend_mass_f32(q.data_ptr(), k.data_ptr(), w.data_ptr(), None, 2, Bp, heads, N, L, XL, d, C, C, N * C, L * C,
                                        d ** -0.5, hip._stream()) == -1
    with pytest.raises(TypeError):            # a host tensor never reaches the library
        hip.cross_blend_mass(q.cpu(), k, heads, d ** -0.5, 2, w, acc)
    with pytest.raises(ValueError, match="outside the batch"):
        hip.cross_blend_mass(q, k, heads, d ** -0.5, 3, w, acc)
    with pytest.raises(ValueError, match="acc"):
        hip.cross_blend_mass(q, k, heads, d ** -0.5, 2, w, acc[:1])
    torch.cuda.synchronize()
    assert (acc == SENTINEL).all(), "a refused call must not launch"

    x = torch.full((Bp, 4, 32, 32), SENTINEL, device=DEV)
    x[0] = 1.0
    ones = torch.ones(Bp, N, device=DEV)
    thres = torch.tensor([THRES], device=DEV)

    def blend(ap=None, tp=None, xp=None, bp=Bp, cc=4, hh=32, ww=32):
        return lib.ief_local_blend_f32(ones.data_ptr() if ap is None else ap, thres.data_ptr() if tp is None else tp,
                                       x.data_ptr() if xp is None else xp, bp, cc, hh, ww, hip._stream())

    assert blend(ap=0) == -1 and blend(tp=0) == -1 and blend(xp=0) == -1, "a null pointer: IEF_EINVAL"
    assert blend(hh=24) == -2 and blend(ww=40) == -2 and blend(hh=0) == -2, "H, W multiples of 16: IEF_ESHAPE"
    assert blend(bp=1) == -2 and blend(cc=0) == -2
    assert blend(xp=x.data_ptr() + 2) == -3 and blend(ap=ones.data_ptr() + 1) == -3, "off the 4-byte grid: IEF_EALIGN"
    with pytest.raises(TypeError):
        hip.local_blend(ones.cpu(), thres, x)
    with pytest.raises(ValueError):
        hip.local_blend(ones[:1], thres, x)
    torch.cuda.synchronize()
    assert (x[1] == SENTINEL).all(), "a refused call must not launch"
    assert mass() == 0 and blend() == 0
    torch.cuda.synchronize()
    assert (acc != SENTINEL).all()
    assert (x[1] == SENTINEL).all() and (x[0] == 1).all(), "an all-ones accumulator masks every pixel in: the row keeps its own values"


# ------------------------------------------------------------------------------------------------------------- whole sampler
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]
STEPS = 4
# Chosen on the generic path.  The synthetic weights give nearly flat maps: the normalised values of all four steps lie in [0.95, 1],
# so the threshold has to sit there.  A scan of 0.965 .. 0.995 in steps of 0.00025 found 0.9905 with the widest clearance for these
# words: the target mask covers 0.188 / 0.207 / 0.172 / 0.129 of the pixels after steps 0-3 and the nearest normalised value lies
# 9.6e-4 / 7.6e-4 / 9.0e-4 / 1.1e-3 from the threshold (the test asserts 0.1 .. 0.9 and > 1e-4, and prints what it finds)
WORDS, E2E_THRES = [["house"], ["fall"]], 0.9905
WORDS2, E2E_THRES2 = [["mountain"], ["mountain", "fall"]], 0.98725       # the second blend of the pooled-loop check


@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.pipeline import StableDiffusionPipeline
    return StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")


def _recording_blend(pipe, words, thres):
    from ief_amd.p2p.model.ptp_utils import LocalBlend

    class Recording(LocalBlend):
        """keeps the normalised 16 x 16 values [Bp, 256] (fp64, host) `__call__` compares with the threshold, per step"""
        seen = None

        def __call__(self, x_t, attention_store):
            maps = attention_store["down_cross"][2:4] + attention_store["up_cross"][:3]
            maps = torch.cat([m.reshape(self.alpha_layers.shape[0], -1, 1, 16, 16, self.MAX_NUM_WORDS) for m in maps], dim=1)
            maps = (maps * self.alpha_layers.to(maps.dtype)).sum(-1).mean(1)
            pooled = F.max_pool2d(maps, (3, 3), (1, 1), padding=(1, 1))
            norm = pooled / pooled.max(2, keepdims=True)[0].max(3, keepdims=True)[0]
            self.seen.append(norm.reshape(-1, 256).double().cpu())
            return super().__call__(x_t, attention_store)

    lb = Recording(pipe.tokenizer, PROMPTS, words, threshold=thres, device=DEV)
    lb.seen = []
    return lb


def generic_blend_run(pipe, words, thres, x_T):
    """the blend on the generic path -> (latents after STEPS steps, the normalised values of every step)"""
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.register import unregister_attention_control
    from ief_amd.p2p.model.sd_utils import P2P

    class RefineOnTheGenericPath(AttentionRefine):       # lowering goes by class name: a subclass is an unknown controller
        pass

    lb = _recording_blend(pipe, words, thres)
    c = RefineOnTheGenericPath(PROMPTS, pipe.tokenizer, STEPS, 0.8, 0.4, local_blend=lb, device=DEV)
    lat, _ = P2P(pipe, STEPS).text2image_ldm_stable(pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=7.5,
                                                     latent=x_T.clone(), return_latents=True)
    assert pipe.unet._plan is None and c.cur_step == STEPS and len(lb.seen) == STEPS
    unregister_attention_control(pipe, c)
    return lat.float().cpu(), lb.seen


def _x_T(pipe):
    s = pipe.cfg.sample_size
    return torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(8888)).to(DEV)


def test_fused_blend_vs_generic_path_graph_vs_eager_pooled_and_edit_many(small_x3):
    """measured on an MI355X (the test prints every figure it asserts on): on the generic path the target mask covers 0.188 / 0.207 /
    0.172 / 0.129 of the pixels after steps 0-3, nearest normalised value to the threshold 9.62e-4 / 7.58e-4 / 9.05e-4 / 1.12e-3; mask
    bits equal at all four steps; latents fused vs generic 3.537e-6 with the blend, 3.535e-6 without (the yardstick; bound 2 x); the
    blend moves the target latents by 1.293e-2, the second blend by 1.189e-2 against the first"""
    from ief_amd import denoise
    from ief_amd.denoise import FusedDenoiser
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.ptp_utils import LocalBlend
    from ief_amd.p2p.model.register import register_attention_control, unregister_attention_control as unreg
    from ief_amd.p2p.model.sd_utils import P2P, _encode_prompts

    pipe = small_x3
    x_T = _x_T(pipe)
    hw = (pipe.cfg.sample_size, pipe.cfg.sample_size)
    editor = P2P(pipe, STEPS)

    class RefineOnTheGenericPath(AttentionRefine):
        pass

    def make(cls=AttentionRefine, words=WORDS, thres=E2E_THRES):
        lb = None if words is None else LocalBlend(pipe.tokenizer, PROMPTS, words, threshold=thres, device=DEV)
        return cls(PROMPTS, pipe.tokenizer, STEPS, 0.8, 0.4, local_blend=lb, device=DEV)

    def sampler(c, blend):
        lat, _ = editor.text2image_ldm_stable(pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=7.5, latent=x_T.clone(),
                                              return_latents=True)
        plan = pipe.unet._plan
        assert (plan is not None) == (type(c) is AttentionRefine) and c.cur_step == STEPS
        assert plan is None or (plan.kind == "p2p" and (plan.blend_w is not None) == blend)
        unreg(pipe, c)
        return lat.float().cpu()

    # the yardstick: the same controller without a blend, fused vs generic
    plain_f, plain_g = sampler(make(words=None), False), sampler(make(RefineOnTheGenericPath, words=None), False)
    yard = rel_err(plain_f, plain_g)

    # the inputs: on the generic path the target mask covers between 0.1 and 0.9 of the pixels at every step and no normalised
    # value lies within 1e-4 of the threshold
    blend_g, seen = generic_blend_run(pipe, WORDS, E2E_THRES, x_T)
    want = []
    for s, norm in enumerate(seen):
        bits = norm > E2E_THRES
        cover, margin = float((bits[0] | bits[1]).double().mean()), float((norm - E2E_THRES).abs().min())
        print(f"generic path step {s}: the target mask covers {cover:.3f} of the pixels (source alone {float(bits[0].double().mean()):.3f}), "
              f"nearest normalised value to the threshold {margin:.2e}")
        assert 0.1 <= cover <= 0.9 and margin > 1e-4
        want.append((bits[0], bits[0] | bits[1]))

    # eager stepping of the fused plan, reading the kernel's own mask bits after every step: indicator latents (0 in the source
    # row, 1 in the target's) come back as the mask; with the target's accumulator row emptied, as the source's mask alone
    with torch.no_grad():
        u, cnd = _encode_prompts(pipe, PROMPTS)
    context = torch.cat([u, cnd])

    def fused_loop(c, use_graph, spy=None, pooled=False):
        register_attention_control(pipe, c, fused=True)           # raises ValueError where the blend cannot be lowered
        pipe.scheduler.set_timesteps(STEPS)
        plan = pipe.unet._plan
        assert plan.kind == "p2p" and plan.blend_w is not None and c._device_blend is plan
        if spy is not None:
            inner = plan.blend_latents

            def blend_latents(x):
                out = inner(x)
                if not plan.muted:
                    ind = torch.zeros(2, 1, 16, 16, device=DEV)
                    ind[1] = 1
                    src = ind.clone()
                    acc0 = plan.blend_acc.clone()
                    acc0[1] = 0
                    hip.local_blend(plan.blend_acc, plan.blend_thres, ind)
                    hip.local_blend(acc0, plan.blend_thres, src)
                    torch.cuda.synchronize()
                    spy.append((src[1].flatten().cpu() != 0, ind[1].flatten().cpu() != 0))
                return out
            plan.blend_latents = blend_latents
        loop = (denoise.acquire(pipe, context, 2, hw, 7.5, use_graph=True) if pooled
                else FusedDenoiser(pipe, context, 2, hw, 7.5, use_graph=use_graph))
        try:
            lat = loop.run(x_T.clone()).float().cpu()
        finally:
            loop.release()
            unreg(pipe, c)
        assert c.cur_step == STEPS
        return lat, loop

    bits = []
    eager, _ = fused_loop(make(), False, spy=bits)
    assert len(bits) == STEPS
    for s, ((src, both), (want_src, want_both)) in enumerate(zip(bits, want)):
        assert torch.equal(src, want_src) and torch.equal(both, want_both), \
            f"step {s}: {int((src != want_src).sum())} source and {int((both != want_both).sum())} target mask bits differ"
    e = rel_err(eager, blend_g)
    effect = rel_err(eager[1:], plain_f[1:])
    print(f"fused vs generic after {STEPS} steps: without a blend {yard:.3e} (yardstick), with the blend {e:.3e} (bound 2 x); the blend "
          f"moves the target latents by {effect:.3e}; mask bits equal at all {STEPS} steps")
    assert torch.equal(eager[0], plain_f[0]), "the source row never sees the blend"
    assert e <= 2 * yard
    assert effect > 100 * (2 * yard)

    # captured graph == eager stepping, bit for bit; the sampler's own run is the captured one
    denoise.drop_pool()
    graph, loop1 = fused_loop(make(), True, pooled=True)
    assert torch.equal(graph, eager), "captured-graph replay must equal eager stepping bit for bit"
    assert torch.equal(sampler(make(), True), eager)
    # the same loop run twice: the accumulators start empty again
    again, loop1b = fused_loop(make(), True, pooled=True)
    assert loop1b is loop1 and torch.equal(again, graph), "a second run of the same loop must find empty accumulators"
    # a pooled loop re-pointed at a controller with other blend words and another threshold == that controller's fresh run
    eager2, _ = fused_loop(make(words=WORDS2, thres=E2E_THRES2), False)
    pooled2, loop2 = fused_loop(make(words=WORDS2, thres=E2E_THRES2), True, pooled=True)
    assert loop2 is loop1 and loop2.graph is not None, "equal signatures: the captured loop is taken from the pool, not rebuilt"
    print(f"the second blend moves the target latents by {rel_err(eager2[1:], eager[1:]):.3e} against the first")
    assert not torch.equal(eager2, eager), "the second controller must be a different edit"
    assert torch.equal(pooled2, eager2), "a re-pointed pooled loop must give the new controller's result"
    # a loop without a blend is another signature: it never takes a blend loop from the pool
    plain_again = sampler(make(words=None), False)
    assert torch.equal(plain_again, plain_f)
    denoise.drop_pool()

    # edit_many with two blend jobs == one call per job
    jobs = [(PROMPTS, make(), x_T.clone()), (PROMPTS, make(words=WORDS2, thres=E2E_THRES2), x_T.clone())]
    many = editor.edit_many(pipe, jobs, num_inference_steps=STEPS, guidance_scale=7.5)
    for (img, _), (words, thres) in zip(many, ((WORDS, E2E_THRES), (WORDS2, E2E_THRES2))):
        c = make(words=words, thres=thres)
        one, _ = editor.text2image_ldm_stable(pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=7.5, latent=x_T.clone())
        unreg(pipe, c)
        assert (img == one).all(), "edit_many must give what one call per job gives"
    denoise.drop_pool()


def test_step_callback_under_a_lowered_plan_blends_on_the_device(small_x3):
    """`P2P.diffusion_step` (the eager step of the sampler) calls `controller.step_callback`: under a lowered plan that is the
    device blend from the plan's accumulator, and the (empty) store is never read.  Bound: the eager step and the fused loop
    may differ by what they differ by for the same controller WITHOUT a blend, measured here, times 2 (a blended latent is a
    select between two latents that each sit within that distance)"""
    from ief_amd.denoise import FusedDenoiser
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.ptp_utils import LocalBlend
    from ief_amd.p2p.model.register import register_attention_control, unregister_attention_control as unreg
    from ief_amd.p2p.model.sd_utils import P2P, _encode_prompts

    pipe = small_x3
    x_T = _x_T(pipe)
    editor = P2P(pipe, STEPS)
    with torch.no_grad():
        u, cnd = _encode_prompts(pipe, PROMPTS)
    context = torch.cat([u, cnd])

    def both(blend):
        def make():
            lb = LocalBlend(pipe.tokenizer, PROMPTS, WORDS, threshold=E2E_THRES, device=DEV) if blend else None
            return AttentionRefine(PROMPTS, pipe.tokenizer, STEPS, 0.8, 0.4, local_blend=lb, device=DEV)
        c = make()
        register_attention_control(pipe, c, fused=True)
        pipe.scheduler.set_timesteps(STEPS)
        loop = FusedDenoiser(pipe, context, 2, (pipe.cfg.sample_size,) * 2, 7.5, use_graph=False)
        looped = loop.run(x_T.clone()).float().cpu()
        loop.release()
        unreg(pipe, c)
        c = make()
        register_attention_control(pipe, c, fused=True)
        pipe.scheduler.set_timesteps(STEPS)
        lat = x_T.expand(2, -1, -1, -1).contiguous()
        with torch.no_grad():
            for t in pipe.scheduler.timesteps:
                lat = editor.diffusion_step(pipe, c, lat, context, t, 7.5)
        unreg(pipe, c)
        assert c.cur_step == STEPS
        if blend:
            assert all(len(v) == 0 for v in c.attention_store.values()), "no map exists under a lowered plan"
        return looped, lat.float().cpu()

    yard = rel_err(*both(False))
    looped, stepped = both(True)
    e = rel_err(stepped, looped)
    print(f"eager diffusion_step vs the fused loop: without a blend {yard:.3e} (yardstick), with the device blend {e:.3e} (bound 2 x)")
    assert e <= 2 * yard


@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_generic_path_serves_the_other_modes(precision, capsys):
    """outside f16x3 the blend takes the generic path, says why once per registration, and runs end to end: the working store
    exists.  The source row never sees the blend, so it equals the source row of the same edit without one, bit for bit"""
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.ptp_utils import LocalBlend
    from ief_amd.p2p.model.register import register_attention_control, unregister_attention_control as unreg
    from ief_amd.p2p.model.sd_utils import P2P
    from ief_amd.pipeline import StableDiffusionPipeline

    class RefineOnTheGenericPath(AttentionRefine):
        pass

    pipe = StableDiffusionPipeline.from_pretrained("synthetic:small", precision=precision)
    x_T = _x_T(pipe)
    steps = 2
    editor = P2P(pipe, steps)
    lats = {}
    for blend in (True, False):
        lb = LocalBlend(pipe.tokenizer, PROMPTS, WORDS, threshold=E2E_THRES, device=DEV) if blend else None
        c = (AttentionRefine if blend else RefineOnTheGenericPath)(PROMPTS, pipe.tokenizer, steps, 0.8, 0.4, local_blend=lb, device=DEV)
        capsys.readouterr()
        if blend:
            with pytest.raises(ValueError, match="cannot be lowered"):
                register_attention_control(pipe, c, fused=True)
            assert capsys.readouterr().out.count("LocalBlend takes the generic path") == 1
        lat, _ = editor.text2image_ldm_stable(pipe, PROMPTS, c, num_inference_steps=steps, guidance_scale=7.5, latent=x_T.clone(),
                                              return_latents=True)
        assert pipe.unet._plan is None and c.cur_step == steps and c._device_blend is None
        if blend:
            assert capsys.readouterr().out.count("LocalBlend takes the generic path") == 1
            assert [len(c.attention_store[k]) for k in ("down_cross", "mid_cross", "up_cross")] == [4, 1, 6]
        unreg(pipe, c)
        lats[blend] = lat.float().cpu()
    assert torch.isfinite(lats[True]).all()
    print(f"{precision}: the blend moves the target row by {rel_err(lats[True][1], lats[False][1]):.3e}")
    assert torch.equal(lats[True][0], lats[False][0]), "the source row never sees the blend"
    assert not torch.equal(lats[True][1], lats[False][1])
