"""`hip.cross_map_grad` (`ief_attn_cross_map_grad_f32`, csrc/cross_map_grad_f32.hip) on a real MI355X: the gradient of one
cross-attention module's value path AND of Pix2Pix-zero's map objective w.r.t. its queries in one launch, and the reverse pass
(`grad.UNetAdjoint(mode="input")`) that calls it in the fp32-storage modes.

Every reference is torch autograd in fp64 on the CPU, computed once per shape and shared.  Stated tolerances:
    dQ (both paths, the value path alone, the objective alone)   <= 2e-5 of max |reference|   (KTOL, the bound of the materialised
                                                                   fp32 path, tests/test_gpu_adjoints_f32.py)
    objective value                                              <= max(4 x the error of torch fp32 on the CPU, 1e-6), relative
    reverse pass, fused against materialised                     input gradient <= 2 x KTOL of its maximum (each path is within
                                                                   KTOL of fp64), objective value <= 1e-6 relative
    two calls                                                    bit-equal
    sentinels around the dQ slice and past the last loss partial untouched
Each test prints what it measured, the materialised path's own errors on the same inputs next to it.

Measured on the MI355X: dQ 2.7e-7 .. 6.4e-7 (materialised path, same inputs: 3.4e-7 .. 8.9e-7), objective value 1.5e-8 .. 6.5e-8
(torch fp32 on the CPU 1.8e-8 .. 6.9e-8); value path alone 2.3e-7 .. 6.1e-7, objective alone 3.1e-7 .. 6.8e-7; reverse pass of the
tiny family, fused against materialised: input gradient 2.3e-6 (f16x3) / 7.7e-7 (f32), objective 4.2e-9 / 7.7e-9.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from ief_amd import hip  # noqa: E402
from ief_amd.grad import UNetAdjoint  # noqa: E402
from ief_amd.pipeline import StableDiffusionPipeline  # noqa: E402

DEV = torch.device("cuda:0")
KTOL = 2e-5
SENTINEL = 7.0
GS = 64.0
MAX_L = hip.CROSS_MAP_GRAD_MAX_L


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _objective_and_value(q, k, v, do, ref, B, heads, N, L, d, scale, dt):
    """(objective, d objective / dq, d (out . dO) / dq) in dtype dt: `_map_objective` of tests/test_gpu_adjoints_f32.py plus the
    value path out = softmax(scale q k^T) v"""
    qf = q.to(dt).requires_grad_(True)
    sp = lambda t, n: t.reshape(B, n, heads, d).transpose(1, 2).reshape(B * heads, n, d)
    P = torch.softmax(sp(qf, N) @ sp(k.to(dt), L).transpose(1, 2) * scale, -1)
    loss = ((P - ref.to(dt)) ** 2).sum((1, 2)).mean(0)
    g_obj, = torch.autograd.grad(loss, qf, retain_graph=True)
    out = (P @ sp(v.to(dt), L)).reshape(B, heads, N, d).transpose(1, 2).reshape(B, N, heads * d)
    g_val, = torch.autograd.grad((out * do.to(dt)).sum(), qf)
    return loss.detach(), g_obj, g_val


@functools.lru_cache(maxsize=None)
def _case(B, heads, N, L, d):
    C = heads * d
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, n, C, generator=g) for n in (N, L, L))
    do = torch.randn(B, N, C, generator=g) * 0.01
    ref = torch.softmax(torch.randn(B * heads, N, L, generator=g) * 2.0, -1)
    scale = d ** -0.5
    loss64, g_obj, g_val = _objective_and_value(q, k, v, do, ref, B, heads, N, L, d, scale, torch.float64)
    loss32 = _objective_and_value(q, k, v, do, ref, B, heads, N, L, d, scale, torch.float32)[0]
    return dict(q=q, k=k, v=v, do=do, ref=ref, scale=scale, loss64=loss64.item(),
                floor32=abs(loss32.item() - loss64.item()) / loss64.item(), g_obj=g_obj * GS, g_val=g_val)


class _Device:
    """the operands as the reverse pass hands them over: K and V column slices of one wider buffer at a non-zero column offset
    (`kv_all`), dQ a column slice of a buffer pre-filled with a sentinel"""

    def __init__(self, case, B, heads, N, L, d, zero_do=False):
        C = heads * d
        self.C = C
        self.q, self.ref = case["q"].to(DEV), case["ref"].to(DEV)
        self.do = torch.zeros(B, N, C, device=DEV) if zero_do else case["do"].to(DEV)
        self.wide = torch.full((B, L, 4 * C), SENTINEL, device=DEV)
        self.k, self.v = self.wide[..., C:2 * C], self.wide[..., 3 * C:]
        self.k.copy_(case["k"])
        self.v.copy_(case["v"])
        assert self.k.storage_offset() != 0 and self.k.stride(1) > C
        self.gq = torch.full((B, N, 3 * C), SENTINEL, device=DEV)
        self.dq = self.gq[..., C:2 * C]

    def sentinels_intact(self):
        C = self.C
        return bool((self.gq[..., :C] == SENTINEL).all() and (self.gq[..., 2 * C:] == SENTINEL).all()
                    and (self.wide[..., :C] == SENTINEL).all() and (self.wide[..., 2 * C:3 * C] == SENTINEL).all())


def _materialised(dv, case, B, heads, N, L, d, gcoef):
    """the two chains the fused launch replaces, on the same device operands: (dq, objective value)"""
    with hip.f32_contraction("x3"):
        dq, _, _ = hip.attn_bwd(dv.q, dv.k, dv.v, None, dv.do, None, heads, case["scale"], want_dkv=False)
        parts = torch.zeros(hip.map_loss_blocks_f32(B * heads * N), device=DEV)
        hip.attn_map_loss_bwd(dv.q, dv.k, dv.ref, dq, heads, case["scale"], gcoef=gcoef, accumulate=True, loss=parts,
                              loss_coef=1.0 / (B * heads))
    return dq, parts.double().sum().item()


CASES = [(2, 2, 300, 77, 40), (1, 2, 64, 77, 160), (2, 1, 256, 77, 64), (2, 3, 1030, 77, 32), (1, 1, 100, 20, 80),
         (3, 2, 65, 77, 40),                # a ragged last block, B = 3
         (1, 2, 70, MAX_L, 160)]            # the largest L the kernel accepts, at the head dim that sets the limit


@pytest.mark.parametrize("B,heads,N,L,d", CASES)
def test_cross_map_grad_vs_fp64_autograd(B, heads, N, L, d):
    """dQ of gs * objective + (out . dO).sum() and the objective value against fp64 autograd; strided K / V / dQ; sentinels; loss
    partials past the last block; loss=None; two calls bit-equal"""
    assert hip.cross_map_grad_ok(d, L)
    case = _case(B, heads, N, L, d)
    dv = _Device(case, B, heads, N, L, d)
    gcoef, loss_coef = 2.0 * GS / (B * heads), 1.0 / (B * heads)
    nblk = hip.cross_map_grad_blocks(N, d)
    lanes = d // (20 if d % 20 == 0 else 16)
    assert nblk == -(-N * lanes // 256)
    parts = torch.full((B * heads * nblk + 3,), SENTINEL, device=DEV)
    got = hip.cross_map_grad(dv.q, dv.k, dv.v, dv.do, dv.ref, heads, case["scale"], gcoef, dq=dv.dq, loss=parts, loss_coef=loss_coef)
    assert got.data_ptr() == dv.dq.data_ptr()
    want = case["g_obj"] + case["g_val"]
    e = rel_err(dv.dq, want)
    el = abs(parts[:B * heads * nblk].double().sum().item() - case["loss64"]) / case["loss64"]
    bound = max(4.0 * case["floor32"], 1e-6)
    dq_m, loss_m = _materialised(dv, case, B, heads, N, L, d, gcoef)
    print(f"cross_map_grad B={B} h={heads} N={N} L={L} d={d}: dq {e:.2e}, objective {el:.2e} (torch fp32 on the CPU: "
          f"{case['floor32']:.2e}, bound {bound:.2e}) | materialised path: dq {rel_err(dq_m, want):.2e}, objective "
          f"{abs(loss_m - case['loss64']) / case['loss64']:.2e}")
    assert e < KTOL and el <= bound
    assert dv.sentinels_intact()
    assert (parts[B * heads * nblk:] == SENTINEL).all()              # nothing written past the last block's partial
    # loss=None, a freshly allocated dq, a second call with partials: the same bits
    again = hip.cross_map_grad(dv.q, dv.k, dv.v, dv.do, dv.ref, heads, case["scale"], gcoef)
    assert again.is_contiguous() and torch.equal(again, dv.dq)
    parts2 = torch.full_like(parts, SENTINEL)
    first = dv.dq.clone()
    hip.cross_map_grad(dv.q, dv.k, dv.v, dv.do, dv.ref, heads, case["scale"], gcoef, dq=dv.dq, loss=parts2, loss_coef=loss_coef)
    assert torch.equal(first, dv.dq) and torch.equal(parts, parts2)


@pytest.mark.parametrize("B,heads,N,L,d", [(2, 2, 300, 77, 40), (1, 2, 64, 77, 160), (1, 1, 100, 20, 80)])
def test_cross_map_grad_halves(B, heads, N, L, d):
    """gcoef = 0: the fp64 dq of plain attention; dO = 0: the fp64 gradient of the objective -- a sign or scale error of one half
    cannot hide in the sum"""
    case = _case(B, heads, N, L, d)
    dv = _Device(case, B, heads, N, L, d)
    hip.cross_map_grad(dv.q, dv.k, dv.v, dv.do, dv.ref, heads, case["scale"], 0.0, dq=dv.dq)
    e_val = rel_err(dv.dq, case["g_val"])
    dz = _Device(case, B, heads, N, L, d, zero_do=True)
    hip.cross_map_grad(dz.q, dz.k, dz.v, dz.do, dz.ref, heads, case["scale"], 2.0 * GS / (B * heads), dq=dz.dq)
    e_obj = rel_err(dz.dq, case["g_obj"])
    print(f"cross_map_grad halves B={B} h={heads} N={N} L={L} d={d}: value path alone {e_val:.2e}, objective alone {e_obj:.2e}")
    assert e_val < KTOL and e_obj < KTOL
    assert dv.sentinels_intact() and dz.sentinels_intact()


def _raw_call(q, k, v, do, ref, dq, B, heads, N, L, d, ptr_shift=0):
    f = lambda t: None if t is None else t.data_ptr()
    return hip.load().ief_attn_cross_map_grad_f32(f(q) + ptr_shift if q is not None else None, f(k), f(v), f(do), f(ref), f(dq), None,
                                                  B, heads, N, L, d, heads * d, heads * d, heads * d, heads * d, heads * d,
                                                  ctypes.c_float(d ** -0.5), ctypes.c_float(1.0), ctypes.c_float(1.0), hip._stream())


def test_cross_map_grad_refusals():
    """a head dim of 48, L past the limit, a misaligned pointer, a null pointer: the documented codes and nothing launched; the
    predicate refuses the same shapes and `hip.attn_map_loss_bwd` still serves them"""
    B, heads, N = 1, 2, 64
    mk = lambda n, c: torch.randn(B, n, c, generator=torch.Generator().manual_seed(n + c)).to(DEV)
    for L, d, shift, null_q, code in ((77, 48, 0, False, -2), (MAX_L + 1, 40, 0, False, -2), (77, 40, 4, False, -3),
                                      (77, 40, 0, True, -1)):
        C = heads * d
        q = torch.zeros(B * N * C + 4, device=DEV)[:B * N * C].view(B, N, C)       # room for the shifted pointer
        q.copy_(mk(N, C))
        k, v, do = mk(L, C), mk(L, C), mk(N, C)
        ref = torch.softmax(mk(N * heads, L).reshape(B * heads, N, L), -1)
        dq = torch.full((B, N, C), SENTINEL, device=DEV)
        assert _raw_call(None if null_q else q, k, v, do, ref, dq, B, heads, N, L, d, shift) == code
        torch.cuda.synchronize()
        assert (dq == SENTINEL).all(), "a refused call launched"
        if shift or null_q:
            continue
        assert not hip.cross_map_grad_ok(d, L) and hip.cross_map_grad_ok(40, 77)
        with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
            hip.cross_map_grad(q, k, v, do, ref, heads, d ** -0.5, 1.0)
        # the materialised path takes the shape
        want = _objective_and_value(q.cpu(), k.cpu(), v.cpu(), do.cpu(), ref.cpu(), B, heads, N, L, d, d ** -0.5, torch.float64)[1] * GS
        with hip.f32_contraction("x3"):
            got = hip.attn_map_loss_bwd(q, k, ref, torch.zeros(B, N, C, device=DEV), heads, d ** -0.5,
                                        gcoef=2.0 * GS / (B * heads), accumulate=False)
        e = rel_err(got, want)
        print(f"refused by cross_map_grad (L={L}, d={d}), served by attn_map_loss_bwd: dq {e:.2e}")
        assert e < KTOL
    assert not hip.cross_map_grad_ok(40, 77, torch.float16) and not hip.cross_map_grad_ok(40, 0)
    assert hip.cross_map_grad_blocks(64, 48) == 0
    with pytest.raises(RuntimeError, match="IEF_EALIGN"):
        buf = torch.zeros(B * N * 80 + 4, device=DEV)
        hip.cross_map_grad(buf[1:1 + B * N * 80].view(B, N, 80), mk(77, 80), mk(77, 80), mk(N, 80),
                           torch.softmax(mk(N * heads, 77).reshape(B * heads, N, 77), -1), heads, 40 ** -0.5, 1.0)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_reverse_pass_fused_vs_materialised(precision, monkeypatch):
    """`UNetAdjoint(mode="input")` on the tiny family: one cross-gradient launch per cross-attention module and no scores, softmax
    backward or map-objective launch over 77 keys; the same input gradient and objective as with the predicate patched off"""
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", keep_state_dict=True, precision=precision)
    cfg, unet, B, gs = pipe.cfg, pipe.unet, 2, 1024.0
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 4, cfg.sample_size, cfg.sample_size, generator=g).to(DEV)
    ctx = (torch.randn(B, 77, cfg.cross_attention_dim, generator=g) * 0.1).to(DEV)
    unet(x, 500, encoder_hidden_states=ctx)                                      # sets last_tokens of every module
    cross = [m for m in unet.attention_modules() if m.is_cross]
    refs = [torch.softmax(torch.randn(B * m.heads, m.last_tokens, 77, generator=g) * 1.5, -1).to(DEV) for m in cross]
    temb = unet.time_rows(torch.tensor([500.0], device=DEV))
    over77 = {"scores": 0, "softmax_bwd": 0, "map_loss": 0}

    def counting(name, key, is77):
        orig = getattr(hip, name)

        def wrapped(*a, **kw):
            over77[key] += bool(is77(a))
            return orig(*a, **kw)
        monkeypatch.setattr(hip, name, wrapped)
    counting("_attn_scores_f32", "scores", lambda a: a[1].shape[1] == 77)
    counting("_softmax_bwd_f32_", "softmax_bwd", lambda a: a[0].shape[-1] == 77)
    counting("_attn_map_loss_bwd_f32", "map_loss", lambda a: True)

    def run():
        adj = UNetAdjoint(unet, gs, mode="input")
        adj.set_reference_maps(refs)
        adj.forward(x, temb, ctx)
        for key in over77:
            over77[key] = 0
        hip.profile_begin()
        try:
            d_x = adj.backward(torch.zeros_like(x))
        finally:
            names = [r[0] for r in hip.profile_end()]
        return d_x.clone(), adj.loss_parts.double().sum().item(), names, dict(over77), list(adj._cross_fused)

    d_f, loss_f, names_f, n77_f, fused_f = run()
    n_fused = sum(n.startswith("cross_map_grad_f32_kernel") for n in names_f)
    assert all(fused_f) and n_fused == len(cross), (fused_f, n_fused, len(cross))
    assert n77_f == {"scores": 0, "softmax_bwd": 0, "map_loss": 0}, n77_f
    monkeypatch.setattr(hip, "cross_map_grad_ok", lambda *a, **kw: False)
    d_m, loss_m, names_m, n77_m, fused_m = run()
    assert not any(fused_m) and not any(n.startswith("cross_map_grad_f32_kernel") for n in names_m)
    assert n77_m == {"scores": 3 * len(cross), "softmax_bwd": 2 * len(cross), "map_loss": len(cross)}, n77_m
    e, el = rel_err(d_f, d_m), abs(loss_f - loss_m) / loss_m
    print(f"UNetAdjoint(mode='input') [{precision}] tiny, {len(cross)} cross modules: {len(names_f)} timed launches fused, "
          f"{len(names_m)} materialised; input gradient fused vs materialised {e:.2e}, objective {el:.2e}")
    assert e <= 2 * KTOL and el <= 1e-6
