"""`hip.cross_bwd` (`ief_attn_cross_bwd_f32`, csrc/cross_bwd_f32.hip) on a real MI355X: dQ, dK and dV of a short-key cross-attention
without a map in HBM, and the null-text reverse pass (`grad.UNetAdjoint(mode="context")`, `nti.NullTextOptimizer`,
`nti.BatchedNullTextOptimizer`) that reaches it through `hip.attn_bwd` in the fp32-storage modes.

Every reference is torch autograd in fp64 on the CPU, computed once per shape and shared.  Stated tolerances (max |x - ref| / max |ref|):
    dQ, dK, dV                                     <= 2e-5 (KTOL of tests/test_gpu_grad_f32.py, the bound of the materialised path), and
                                                   <= 2 x the materialised path's own error on the same device operands wherever
                                                   that is above 1e-7 (the margin a fused form gets over its yardstick)
    one query removed                              dK / dV change by that query's fp64 contribution, <= 2e-5 of max |dK|, |dV|
    d loss / d context, whole UNet                 <= 1e-4 of its maximum against the autograd oracle, fused AND materialised
                                                   (the bound of test_unet_context_gradient_fp32_modes)
    two calls; B = 3 against three B = 1 calls; want_dq False against True; graph against eager; batched K = 2 against per image
                                                   bit-equal
    sentinels around dQ / dK / dV, between K and V, past the end of the scratch        untouched
Each test prints what it measured.

Measured on the MI355X: dQ 2.3e-7 .. 6.1e-7 (materialised path in split-operand mode, same device operands: 1.3e-6 .. 2.3e-6), dK 2.2e-7 ..
4.9e-7 (1.4e-6 .. 2.7e-6), dV 1.0e-7 .. 5.8e-7 (1.3e-6 .. 2.3e-6); one query removed: dK 1.9e-7, dV 2.3e-7; d loss / d context of the tiny
family at B = 2: fused 1.90e-5 / materialised 1.81e-5 / mutual 1.7e-5 (f16x3), 3.2e-6 / 3.5e-6 / 1.3e-6 (f32).
`hip.cross_bwd_ok` leaves d = 160 to the materialised path (slower fused at the levels that head dim belongs to):
the d = 160 shapes below call the kernel directly.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from ief_amd import hip  # noqa: E402
from ief_amd.grad import UNetAdjoint  # noqa: E402
from ief_amd.nti import BatchedNullTextOptimizer, NullTextOptimizer  # noqa: E402
from ief_amd.pipeline import StableDiffusionPipeline  # noqa: E402
from oracle import p2p_ref, unet_ref  # noqa: E402

DEV = torch.device("cuda:0")
KTOL = 2e-5
SENTINEL = 7.0
MAX_L = hip.CROSS_BWD_MAX_L


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _autograd64(q, k, v, do, heads, scale):
    """(dQ, dK, dV) of (softmax(scale q k^T) v . dO).sum() in fp64"""
    B, N, C = q.shape
    L, d = k.shape[1], C // heads
    qf, kf, vf = (t.double().requires_grad_(True) for t in (q, k, v))
    sp = lambda t, n: t.reshape(B, n, heads, d).transpose(1, 2)
    P = torch.softmax(sp(qf, N) @ sp(kf, L).transpose(2, 3) * scale, -1)
    out = (P @ sp(vf, L)).transpose(1, 2).reshape(B, N, C)
    return torch.autograd.grad((out * do.double()).sum(), (qf, kf, vf))


@functools.lru_cache(maxsize=None)
def _case(B, heads, N, L, d):
    C = heads * d
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, n, C, generator=g) for n in (N, L, L))
    do = torch.randn(B, N, C, generator=g) * 0.01
    scale = d ** -0.5
    dq, dk, dv = _autograd64(q, k, v, do, heads, scale)
    return dict(q=q, k=k, v=v, do=do, scale=scale, dq=dq, dk=dk, dv=dv)


class _Device:
    """the operands as the reverse pass hands them over: K and V column slices of one wide buffer at a non-zero column offset
    (`kv_all`), dK and dV slices of another (`dkv_all`), dQ a slice of a third; everything else in them a sentinel"""

    def __init__(self, case, B, heads, N, L, d, fill=SENTINEL):
        C = self.C = heads * d
        self.q, self.do = case["q"].to(DEV), case["do"].to(DEV)
        self.wide = torch.full((B, L, 4 * C), SENTINEL, device=DEV)
        self.k, self.v = self.wide[..., C:2 * C], self.wide[..., 3 * C:]
        self.k.copy_(case["k"])
        self.v.copy_(case["v"])
        assert self.k.storage_offset() != 0 and self.k.stride(1) > C
        self.gwide = torch.full((B, L, 4 * C), fill, device=DEV)
        self.dk, self.dv = self.gwide[..., C:2 * C], self.gwide[..., 3 * C:]
        self.gq = torch.full((B, N, 3 * C), fill, device=DEV)
        self.dq = self.gq[..., C:2 * C]

    def sentinels_intact(self, fill=SENTINEL, dq_too=False):
        C = self.C
        ok = ((self.gq[..., :C] == fill).all() and (self.gq[..., 2 * C:] == fill).all()
              and (self.gwide[..., :C] == fill).all() and (self.gwide[..., 2 * C:3 * C] == fill).all()
              and (self.wide[..., :C] == SENTINEL).all() and (self.wide[..., 2 * C:3 * C] == SENTINEL).all())
        return bool(ok and (not dq_too or (self.dq == fill).all()))


def _materialised(dv, heads, scale, monkeypatch):
    """what `cross_bwd` replaces, on the same device operands: `hip.attn_bwd` with the predicate forced off, split-operand mode"""
    with monkeypatch.context() as mp, hip.f32_contraction("x3"):
        mp.setattr(hip, "cross_bwd_ok", lambda *a, **kw: False)
        return hip.attn_bwd(dv.q, dv.k, dv.v, None, dv.do, None, heads, scale)


CASES = [(2, 2, 300, 77, 40),               # three query blocks, ragged last
         (3, 2, 65, 77, 40),                # one block, half dead lanes
         (1, 2, 70, 77, 160),               # QB = 32, three blocks
         (2, 1, 256, 77, 64),               # exact blocks
         (2, 3, 1030, 77, 32),              # nine blocks, ragged last
         (1, 1, 100, 20, 80),               # short L
         (1, 2, 33, 5, 40),                 # L not a multiple of the 4-key inner block
         (1, 1, 17, 1, 64),                 # a single key: P = 1, dQ = 0 exactly
         (1, 2, 70, MAX_L, 160)]            # the largest L accepted, at the head dim that sets the limit


@pytest.mark.parametrize("B,heads,N,L,d", CASES)
def test_cross_bwd_vs_fp64_autograd(B, heads, N, L, d, monkeypatch):
    assert hip.cross_bwd_ok(d, L) == (d != 160)       # the kernel takes d = 160, the reverse pass does not send it there (timing)
    lanes = d // (20 if d % 20 == 0 else 16)
    assert hip.cross_bwd_blocks(N, d) == -(-N * lanes // 256)
    case = _case(B, heads, N, L, d)
    dv = _Device(case, B, heads, N, L, d)
    got = hip.cross_bwd(dv.q, dv.k, dv.v, dv.do, heads, case["scale"], dq=dv.dq, dk=dv.dk, dv=dv.dv)
    assert [t.data_ptr() for t in got] == [dv.dq.data_ptr(), dv.dk.data_ptr(), dv.dv.data_ptr()]
    mat = _materialised(dv, heads, case["scale"], monkeypatch)
    errs = [(nm, rel_err(g, case[nm]), rel_err(m, case[nm])) for nm, g, m in zip(("dq", "dk", "dv"), got, mat)]
    print(f"cross_bwd B={B} h={heads} N={N} L={L} d={d}: " +
          ", ".join(f"{nm} {e:.2e} (materialised {em:.2e})" for nm, e, em in errs))
    assert dv.sentinels_intact()
    for nm, e, em in errs:
        assert e < KTOL, nm
        if em > 1e-7:
            assert e <= 2.0 * em, nm
    if L == 1:
        assert dv.dq.abs().max().item() == 0.0 and dv.dk.abs().max().item() == 0.0
    # through `hip.attn_bwd`, the way the reverse pass calls it, in both contraction modes: the same bits
    for mode in ("x3", "f32") if hip.cross_bwd_ok(d, L) else ():
        with hip.f32_contraction(mode):
            via = hip.attn_bwd(dv.q, dv.k, dv.v, None, dv.do, None, heads, case["scale"])
        assert all(torch.equal(a, b) for a, b in zip(via, got)), mode


def test_write_discipline_and_determinism():
    B, heads, N, L, d = 3, 2, 65, 77, 40
    case = _case(B, heads, N, L, d)
    GARBAGE = -3.0e4
    dv = _Device(case, B, heads, N, L, d, fill=GARBAGE)                      # dK / dV / dQ start as garbage: overwritten, not added to
    dq, dk, dvv = hip.cross_bwd(dv.q, dv.k, dv.v, dv.do, heads, case["scale"], dq=dv.dq, dk=dv.dk, dv=dv.dv)
    assert dv.sentinels_intact(GARBAGE)
    assert max(rel_err(dq, case["dq"]), rel_err(dk, case["dk"]), rel_err(dvv, case["dv"])) < KTOL
    first = [t.clone() for t in (dq, dk, dvv)]
    # want_dq=False: dq untouched, dK / dV the same bits
    nq = _Device(case, B, heads, N, L, d)
    r = hip.cross_bwd(nq.q, nq.k, nq.v, nq.do, heads, case["scale"], dq=nq.dq, dk=nq.dk, dv=nq.dv, want_dq=False)
    assert r[0] is None and nq.sentinels_intact(dq_too=True)
    assert torch.equal(nq.dk, first[1]) and torch.equal(nq.dv, first[2])
    # a second call, freshly allocated outputs
    again = hip.cross_bwd(dv.q, dv.k, dv.v, dv.do, heads, case["scale"])
    assert all(a.is_contiguous() and torch.equal(a, b) for a, b in zip(again, first))
    # row b of a B = 3 launch == a B = 1 launch on row b
    for b in range(B):
        one = hip.cross_bwd(dv.q[b:b + 1], dv.k[b:b + 1], dv.v[b:b + 1], dv.do[b:b + 1], heads, case["scale"])
        assert all(torch.equal(o[0], f[b]) for o, f in zip(one, first)), b
    # the scratch ends where ief_cross_bwd_scratch_floats says
    lib = hip.load()
    n_scr = lib.ief_cross_bwd_scratch_floats(B, heads, N, L, d)
    assert n_scr == B * heads * hip.cross_bwd_blocks(N, d) * 2 * L * d
    scratch = torch.full((n_scr + 1,), SENTINEL, device=DEV)
    raw = _Device(case, B, heads, N, L, d)
    C = heads * d
    assert lib.ief_attn_cross_bwd_f32(raw.q.data_ptr(), raw.k.data_ptr(), raw.v.data_ptr(), raw.do.data_ptr(), raw.dq.data_ptr(),
                                      raw.dk.data_ptr(), raw.dv.data_ptr(), scratch.data_ptr(), B, heads, N, L, d, C, 4 * C, 4 * C, C,
                                      3 * C, 4 * C, 4 * C, case["scale"], hip._stream()) == 0
    assert scratch[-1].item() == SENTINEL and not (scratch[:-1] == SENTINEL).any()
    assert all(torch.equal(a, b) for a, b in zip((raw.dq, raw.dk, raw.dv), first))


def test_ragged_block_counts_the_last_query_once():
    """N = 65 at d = 40: query 64 alone in the second half of a 128-query block, 63 dead lanes shadowing it.  Against the same
    data without it (N = 64) dK and dV move by exactly that query's fp64 contribution"""
    B, heads, N, L, d = 3, 2, 65, 77, 40
    case = _case(B, heads, N, L, d)
    dv = _Device(case, B, heads, N, L, d)
    _, dk65, dv65 = hip.cross_bwd(dv.q, dv.k, dv.v, dv.do, heads, case["scale"])
    q64, do64 = case["q"][:, :64].contiguous(), case["do"][:, :64].contiguous()
    _, dk64, dv64 = hip.cross_bwd(q64.to(DEV), dv.k, dv.v, do64.to(DEV), heads, case["scale"])
    _, rk, rv = _autograd64(case["q"][:, 64:], case["k"], case["v"], case["do"][:, 64:], heads, case["scale"])
    ek = ((dk65 - dk64).double().cpu() - rk).abs().max().item() / case["dk"].abs().max().item()
    ev = ((dv65 - dv64).double().cpu() - rv).abs().max().item() / case["dv"].abs().max().item()
    print(f"ragged block: query 64 moves dK by {rk.abs().max().item() / case['dk'].abs().max().item():.2e} and dV by "
          f"{rv.abs().max().item() / case['dv'].abs().max().item():.2e} of their maxima; error of the difference dK {ek:.2e}, dV {ev:.2e}")
    assert rk.abs().max().item() > 100 * KTOL * case["dk"].abs().max().item()          # a second count could not hide in the bound
    assert rv.abs().max().item() > 100 * KTOL * case["dv"].abs().max().item()
    assert ek < KTOL and ev < KTOL


def test_refusals():
    """the documented codes, nothing launched, outputs untouched"""
    B, heads, N = 1, 2, 64
    lib = hip.load()

    def call(L=77, d=40, null=None, shift=None, ld=None):
        C = heads * d
        t = {nm: torch.zeros(B * n * C + 4, device=DEV) for nm, n in (("Q", N), ("K", L), ("V", L), ("dO", N))}
        out = {nm: torch.full((B * n * C + 4,), SENTINEL, device=DEV) for nm, n in (("dQ", N), ("dK", max(L, 1)), ("dV", max(L, 1)))}
        scratch = torch.full((max(1, B * heads * 2 * 2 * max(L, 1) * d) + 4,), SENTINEL, device=DEV)
        ptr = {nm: x.data_ptr() for nm, x in list(t.items()) + list(out.items()) + [("scratch", scratch)]}
        if shift:
            ptr[shift] += 4
        if null:
            ptr[null] = None
        lds = {nm: C for nm in ("ldq", "ldk", "ldv", "ldo", "lddq", "lddk", "lddv")}
        lds.update(ld or {})
        rc = lib.ief_attn_cross_bwd_f32(ptr["Q"], ptr["K"], ptr["V"], ptr["dO"], ptr["dQ"], ptr["dK"], ptr["dV"], ptr["scratch"],
                                        B, heads, N, L, d, lds["ldq"], lds["ldk"], lds["ldv"], lds["ldo"], lds["lddq"], lds["lddk"],
                                        lds["lddv"], ctypes.c_float(d ** -0.5), hip._stream())
        torch.cuda.synchronize()
        untouched = all(bool((x == SENTINEL).all()) for x in list(out.values()) + [scratch])
        return rc, untouched, out

    for nm in ("Q", "K", "V", "dO", "dK", "dV", "scratch"):
        assert call(null=nm)[:2] == (-1, True), nm
    rc, _, out = call(null="dQ")                                            # dQ == NULL is the want_dq=False form
    assert rc == 0 and bool((out["dQ"] == SENTINEL).all()) and not bool((out["dK"][:-4] == SENTINEL).any())
    assert call(d=48)[:2] == (-2, True)
    assert call(L=0)[:2] == (-2, True)
    assert call(L=MAX_L + 1)[:2] == (-2, True)
    for nm in ("ldq", "ldk", "ldv", "ldo", "lddq", "lddk", "lddv"):
        assert call(ld={nm: heads * 40 - 4})[:2] == (-2, True), nm
        assert call(ld={nm: heads * 40 + 2})[:2] == (-3, True), nm
    for nm in ("Q", "K", "V", "dO", "dQ", "dK", "dV", "scratch"):
        assert call(shift=nm)[:2] == (-3, True), nm
    assert not hip.cross_bwd_ok(40, 77, torch.float16) and not hip.cross_bwd_ok(48, 77) and hip.cross_bwd_ok(40, 77)
    assert not hip.cross_bwd_ok(40, 0) and not hip.cross_bwd_ok(40, MAX_L + 1) and hip.cross_bwd_ok(80, MAX_L)
    assert not hip.cross_bwd_ok(160, 77)              # accepted by the kernel, slower than the materialised chain at its levels
    assert hip.cross_bwd_blocks(64, 48) == 0 and lib.ief_cross_bwd_scratch_floats(1, 2, 64, 77, 48) == 0
    assert MAX_L >= 77
    mk = lambda n, c: torch.randn(B, n, c, generator=torch.Generator().manual_seed(n + c)).to(DEV)
    with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
        hip.cross_bwd(mk(N, 96), mk(77, 96), mk(77, 96), mk(N, 96), heads, 48 ** -0.5)


# ------------------------------------------------------------------------------------------------ the reverse pass
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_context_pass_routing(precision, monkeypatch):
    """`UNetAdjoint(mode="context")` on the tiny family: one `cross_bwd` per cross-attention module (the `stop` block's without
    dQ), no scores launch over 77 keys, `ief_attn_bwd_x3` where it was; d loss / d context of the fused and of the materialised
    pass both within the bound of test_unet_context_gradient_fp32_modes of the autograd oracle"""
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", keep_state_dict=True, precision=precision)
    cfg, unet, B, t = pipe.cfg, pipe.unet, 2, 601
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 4, cfg.sample_size, cfg.sample_size, generator=g)
    ctx = torch.randn(B, 77, cfg.cross_attention_dim, generator=g) * 0.1
    de = torch.randn(B, 4, cfg.sample_size, cfg.sample_size, generator=g)
    de = de / de.abs().max()
    ctx_ref = ctx.clone().requires_grad_(True)
    (unet_ref.unet_forward(pipe._state_dict, cfg, x, t, ctx_ref) * de).sum().backward()
    n_cross = sum(m.is_cross for m in unet.attention_modules())
    temb = unet.time_rows(torch.tensor([float(t)], device=DEV))
    seen = {"cross_bwd": [], "scores77": 0, "bwd_x3": 0}

    def counting(name, note):
        orig = getattr(hip, name)

        def wrapped(*a, **kw):
            note(a, kw)
            return orig(*a, **kw)
        monkeypatch.setattr(hip, name, wrapped)
    counting("cross_bwd", lambda a, kw: seen["cross_bwd"].append((a[1].shape[1], kw.get("want_dq", True), kw.get("dk"))))
    counting("_attn_scores_f32", lambda a, kw: seen.__setitem__("scores77", seen["scores77"] + (a[1].shape[1] == 77)))
    counting("_attn_bwd_x3", lambda a, kw: seen.__setitem__("bwd_x3", seen["bwd_x3"] + 1))

    def run():
        adj = UNetAdjoint(unet)
        adj.forward(x.to(DEV), temb, ctx.to(DEV))
        seen.update(cross_bwd=[], scores77=0, bwd_x3=0)
        hip.profile_begin()
        try:
            got = adj.backward(de.to(DEV).contiguous())
        finally:
            names = [r[0] for r in hip.profile_end()]
        return got.clone(), names, dict(seen)

    g_f, names_f, n_f = run()
    # the tiny family's self-attention levels have at most 64 keys: the shape rule takes them too; the cross modules are the 77-key calls
    cross_calls = [c for c in n_f["cross_bwd"] if c[0] == 77]
    assert len(cross_calls) == n_cross and n_f["scores77"] == 0, (len(cross_calls), n_cross, n_f["scores77"])
    assert all(L <= MAX_L for L, _, _ in n_f["cross_bwd"])
    assert [w for _, w, _ in cross_calls].count(False) == 1                    # the `stop` block: dQ == NULL at the kernel
    for _, _, dk in cross_calls:                                               # `dkv_all`'s column slices went straight through
        assert dk is not None and dk.stride(1) > dk.shape[2]
    assert any(dk.storage_offset() != 0 for _, _, dk in cross_calls)
    assert sum(n.startswith("cross_bwd_f32_kernel") for n in names_f) == len(n_f["cross_bwd"])
    monkeypatch.setattr(hip, "cross_bwd_ok", lambda *a, **kw: False)
    g_m, names_m, n_m = run()
    assert n_m["cross_bwd"] == [] and n_m["scores77"] == 2 * n_cross, n_m
    assert n_m["bwd_x3"] == n_f["bwd_x3"]
    assert sum(n.startswith("attn_bwd_x3") for n in names_m) == sum(n.startswith("attn_bwd_x3") for n in names_f)
    e_f, e_m, mutual = rel_err(g_f, ctx_ref.grad), rel_err(g_m, ctx_ref.grad), rel_err(g_f, g_m)
    print(f"UNetAdjoint(mode='context') [{precision}] tiny, {n_cross} cross modules, {n_f['bwd_x3']} attn_bwd_x3 calls: {len(names_f)} "
          f"timed launches fused, {len(names_m)} materialised; d/d ctx vs the oracle: fused {e_f:.2e}, materialised {e_m:.2e}; "
          f"fused vs materialised {mutual:.2e}")
    assert e_f < 1e-4 and e_m < 1e-4


def test_one_null_text_timestep():
    """tiny family, f16x3, one timestep of 3 inner iterations: the captured graph equals eager launches bit for bit, and
    `BatchedNullTextOptimizer` with K = 2 equals the per-image optimiser on each image bit for bit"""
    steps, inner, gs = 2, 3, 7.5
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", keep_state_dict=True, precision="f16x3")
    pipe.scheduler.set_timesteps(steps)
    cfg, sched = pipe.cfg, p2p_ref.DDIMRef(num_inference_steps=steps)
    images = []
    for seed in (0, 1):
        g = torch.Generator().manual_seed(seed)
        ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g) * 0.1
        x0 = torch.randn(1, 4, cfg.sample_size, cfg.sample_size, generator=g)
        images.append((ctx, p2p_ref.ddim_inversion_loop(pipe._state_dict, cfg, ctx[1:], x0, sched)))
    hw = tuple(images[0][1][-1].shape[-2:])
    calls = []
    orig = hip.cross_bwd
    hip.cross_bwd = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    try:
        single = {}
        for use_graph in (True, False):
            for k, (ctx, lat) in enumerate(images):
                opt = NullTextOptimizer(pipe, ctx[1:], gs, hw, use_graph=use_graph)
                opt.begin(lat, ctx[:1])
                opt.outer_begin(0)
                for _ in range(inner):
                    opt.inner_step()
                    opt.inner_loss()
                opt.outer_end()
                single[use_graph, k] = (opt.out[-1].clone(), opt.lat.clone())
                opt.release()
        bat = BatchedNullTextOptimizer(pipe, torch.cat([c[1:] for c, _ in images]), gs, hw, 2)
        bat.begin([l for _, l in images], [c[:1] for c, _ in images], torch.cat([c[1:] for c, _ in images]))
        bat.outer_begin(0)
        for _ in range(inner):
            bat.inner_step()
            bat.inner_losses()
        bat.outer_end()
        out_b, lat_b = [bat.out[k][-1].clone() for k in range(2)], bat.lat.clone()
        bat.release()
    finally:
        hip.cross_bwd = orig
    assert calls, "the null-text pass never reached cross_bwd"
    for k in range(2):
        assert torch.equal(single[True, k][0], single[False, k][0]) and torch.equal(single[True, k][1], single[False, k][1]), k
        assert not torch.equal(single[True, k][0].cpu(), images[k][0][:1])                  # the embedding moved
        assert torch.equal(out_b[k].reshape(-1), single[True, k][0].reshape(-1)), k
        assert torch.equal(lat_b[k].reshape(-1), single[True, k][1].reshape(-1)), k
