"""The adjoint kernels of the fp32-storage reverse pass, one by one, against fp64 at the shapes and call forms the UNet of
`ief_amd/grad.py` runs them in (null-text inversion, Pix2Pix-zero) on a real MI355X.

tests/test_gpu_grad_f32.py holds each adjoint to fp64 at one to five friendly shapes; this file adds the shapes at which the
kernels take another path: the second and third channel-block pass of the row-streaming GroupNorm backward (C = 1280, 1920,
2560), its one-workgroup fallback, offset inputs, LayerNorm rows past a workgroup, the fp32 map objective of Pix2Pix-zero,
`hip.attn_bwd` asked for dQ only / dK, dV only, `ief_attn_bwd_x3` at its thresholds, at N = L = 4096 and over three dO
magnitudes, grid-stride loops past their 8192-workgroup cap, non-square images, and `lse` from the planes-in attention.

Every reference is torch (autograd or plain arithmetic) in fp64 on the CPU, computed inside the test; no kernel of this library
serves as a reference.  Stated tolerances (relative to max |reference| unless said otherwise; every test prints what it measured):
    single adjoint kernels (GroupNorm, LayerNorm, softmax backward, map objective dq, materialised attention
        gradients, conv_out / 3x3 data gradients, GEGLU)                                  <= 2e-5   (KTOL)
    the same on inputs offset by 20 sigma: <= 4 x the error of torch autograd in fp32 on the CPU for the same expression
        (fp32 statistics lose accuracy there by construction; 4 covers a different summation order), KTOL as the floor
    map objective value: <= 4 x the error of the objective evaluated by torch in fp32 on the CPU, floored at 1e-6
    `ief_attn_bwd_x3` (fused, recomputing), dQ / dK / dV                                   <= 1e-5
        with dO ~ 1e-3 (its lo halves are fp16 subnormals: the small-operand floor of the mode)   <= 2e-4
    `ief_attn_bwd_delta_f32in` (a 40-term fp32 dot product)                                <= 2e-6
    row log-sum-exp of the planes-in attention (log2 units)                                <= 1e-5 absolute
    `pool2x2_sum` (one rounding of a four-term sum)                                        <= 2e-7
    `zero_insert2x`, `_transpose_maps_f32`                                                 bit-equal
    gradients not requested: their destination still holds the sentinel it was filled with

Measured on the MI355X (largest of each group; no kernel had to change for these):
    GroupNorm backward   row-streaming 1.5e-7, one-workgroup 1.3e-7; offset 20: 3.4e-7 / 1.9e-7 (torch fp32 3.3e-7 / 2.6e-7)
    LayerNorm backward   1.9e-7; rows offset by 20 spreads 9.9e-8 (torch fp32 2.1e-7)
    map objective        dq 5.1e-7 (x3) / 1.2e-6 (f32); objective value 1.1e-8 .. 4.0e-8 (torch fp32 1.0e-8 .. 9.0e-8)
    softmax backward 2.7e-7; attention gradients on materialised maps 6.1e-7 (x3) / 5.4e-7 (f32), every call form
    ief_attn_bwd_x3      thresholds 1.4e-6, call forms 1.1e-6, N = L = 4096 1.9e-6 (d = 64) / 1.7e-6 (d = 40), peaked rows 3.6e-6,
                         dO x 1 / 0.05 / 1e-3: 7.2e-7 / 1.1e-6 / 1.9e-5;  delta 9.0e-8
    pool2x2_sum 8.4e-8; conv_out backward 2.9e-7; 3x3 data gradients at 8 x 12 3.0e-7; GEGLU backward 4.8e-8 (|gate| to 20.8)
    planes-in attention  lse 2.8e-6 absolute, gradients through ief_attn_bwd_x3 1.3e-6
"""
import functools
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ief_amd import hip, planes  # noqa: E402
from ief_amd.grad import UNetAdjoint  # noqa: E402

DEV = torch.device("cuda:0")
KTOL = 2e-5
XTOL_BWD = 1e-5            # ief_attn_bwd_x3 (tests/test_gpu_grad_f32.py::test_attn_bwd_x3_fused_recomputing_vs_autograd)
SMALL_OPERAND_TOL = 2e-4   # tests/test_gpu_x3.py::test_gemm_x3_operand_magnitudes
SENTINEL = 7.0
LOG2E = 1.4426950408889634


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return None if t is None else t.to(DEV)


@pytest.fixture(params=["x3", "f32"])
def contraction(request):
    with hip.f32_contraction(request.param):
        yield request.param


def launched(fn):
    """(result of fn(), names of the timed launches it made)"""
    hip.profile_begin()
    try:
        out = fn()
    finally:
        names = [r[0] for r in hip.profile_end()]
    return out, names


def offset_bound(floor32):
    """inputs far from zero: 4 x what torch's own fp32 evaluation of the expression loses, never below KTOL"""
    return max(4.0 * floor32, KTOL)


# ------------------------------------------------------------------------------------------------ 1. GroupNorm backward
def _gn_ref(x, x2, dy, add, gamma, beta, G, silu, dt):
    xin = (torch.cat([x, x2], -1) if x2 is not None else x).to(dt).requires_grad_(True)
    y = F.group_norm(xin.transpose(1, 2), G, gamma.to(dt), beta.to(dt), 1e-5).transpose(1, 2)
    (F.silu(y) if silu else y).backward(dy.to(dt))
    return xin.grad + add.to(dt)


# (B, HW, C1, C2, groups, x one float off 16-byte alignment, row-streaming form expected)
GN_CASES = [
    (2, 64, 1280, 0, 32, False, True),        # CQ = 320: a second channel-block pass, partial
    (2, 64, 1280, 640, 32, False, True),      # CQ = 480, 60 channels per group, one group straddles the two sources
    (1, 64, 1280, 1280, 32, False, True),     # CQ = 640: three passes, the last partial
    (1, 4096, 320, 0, 32, False, True),       # the batch-1 null-text shape: many runs, quads straddling groups
    (3, 35, 64, 0, 32, False, True),          # ragged HW, 2 channels per group
    (2, 35, 66, 30, 32, False, False),        # C1 % 4 != 0                       -> one workgroup per (image, group)
    (1, 16, 1024, 0, 2, False, False),        # 512 channels per group            -> one workgroup per (image, group)
    (2, 256, 320, 0, 32, True, False),        # x starts 4 bytes past 16-byte alignment -> one workgroup per (image, group)
]


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("B,HW,C1,C2,G,misalign,ws_form", GN_CASES)
def test_groupnorm_bwd_f32_forms_and_offsets(B, HW, C1, C2, G, misalign, ws_form, silu, offset):
    """`hip.groupnorm_bwd` on fp32 input: `ief_groupnorm_bwd_f32_ws` (five launches, `gn3_bwd_kernel` past 256 channel quads) and
    `ief_groupnorm_bwd_f32` (one workgroup per (image, group)), each case asserting the form it ran on; with `add`, SiLU on and
    off; and the same on inputs 20 sigma from zero, held to 4 x torch's own fp32 error"""
    C = C1 + C2
    x, x2 = f32(B, HW, C1, seed=1) * 2 + 0.5, (f32(B, HW, C2, seed=2) if C2 else None)
    if offset:
        x, x2 = x + 20.0, (x2 * 3 - 20 if C2 else None)
    dy, add = f32(B, HW, C, seed=3, scale=0.1), f32(B, HW, C, seed=4, scale=0.1)
    gamma, beta = 1 + f32(C, seed=5, scale=0.1), f32(C, seed=6, scale=0.1)
    ref = _gn_ref(x, x2, dy, add, gamma, beta, G, silu, torch.float64)
    parts = lambda t: [t[..., :C1], t[..., C1:]] if C2 else [t]
    if misalign:                  # scalar loads only in this form: a view one float into a larger buffer is safe HERE only
        buf = torch.zeros(x.numel() + 4, device=DEV)
        xd = buf[1:1 + x.numel()].view(B, HW, C1)
        xd.copy_(x)
        assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    else:
        xd = dev(x)
    x2d, dyd, addd, gd, bd = dev(x2), dev(dy), dev(add), dev(gamma), dev(beta)
    # the branch condition of hip.groupnorm_bwd, restated: a change of the dispatch must not quietly move a case to the other kernel
    al16 = all(t is None or t.data_ptr() % 16 == 0 for t in (xd, x2d, dyd, addd, gd, bd))
    takes_ws = hip.GN3_F32 and al16 and C1 % 4 == 0 and C2 % 4 == 0 and C // G <= 256
    assert hip.GN3_F32 and takes_ws == ws_form
    got, names = launched(lambda: hip.groupnorm_bwd(xd, dyd, gd, bd, G, 1e-5, silu=silu, x2=x2d, add=addd))
    assert names == (["gn3_bwd_f32 (5 launches)"] if ws_form else ["gn_bwd_f32_kernel"]), names
    got = list(got) if C2 else [got]
    e = max(rel_err(g, r) for g, r in zip(got, parts(ref)))
    form = "row-streaming" if ws_form else "one-workgroup"
    if not offset:
        print(f"groupnorm_bwd fp32 [{form}] B={B} HW={HW} C={C1}+{C2} G={G} silu={silu}: {e:.2e}")
        assert e < KTOL
        return
    ref32 = _gn_ref(x, x2, dy, add, gamma, beta, G, silu, torch.float32)
    floor32 = max(rel_err(g, r) for g, r in zip(parts(ref32), parts(ref)))
    print(f"groupnorm_bwd fp32 [{form}] B={B} HW={HW} C={C1}+{C2} G={G} silu={silu} offset 20: {e:.2e} (torch fp32 on the CPU: "
          f"{floor32:.2e}, bound {offset_bound(floor32):.2e})")
    assert e <= offset_bound(floor32)


# ------------------------------------------------------------------------------------------------ 2. LayerNorm backward
def _ln_ref(x, dy, add, gamma, dt):
    xin = x.to(dt).requires_grad_(True)
    C = x.shape[-1]
    F.layer_norm(xin, (C,), gamma.to(dt), torch.zeros(C, dtype=dt), 1e-5).backward(dy.to(dt))
    return xin.grad + (add.to(dt) if add is not None else 0.0)


@pytest.mark.parametrize("variant", ["add", "noadd", "offset"])
@pytest.mark.parametrize("rows,C", [(1, 64), (5, 640), (301, 1280), (4099, 320), (7, 100)])
def test_layernorm_bwd_f32_shapes(rows, C, variant):
    """`ief_layernorm_bwd_f32`: one wave per row striding C by 64, four rows per workgroup with an early return -- a single row,
    row counts that are no multiple of four, C = 640 / 1280 (the product's), C that is no multiple of 64; rows offset by 20
    spreads held to 4 x torch's own fp32 error"""
    x, dy = f32(rows, C, seed=1) * 3 + 1, f32(rows, C, seed=2, scale=0.1)
    add = None if variant == "noadd" else f32(rows, C, seed=3, scale=0.1)
    gamma = 1 + f32(C, seed=5, scale=0.1)
    if variant == "offset":
        sign = 1.0 - 2.0 * (torch.arange(rows) % 2).float()
        x = x + (20.0 * x.std(1) * sign)[:, None]
    ref = _ln_ref(x, dy, add, gamma, torch.float64)
    e = rel_err(hip.layernorm_bwd(dev(x), dev(dy), dev(gamma), 1e-5, add=dev(add)), ref)
    if variant != "offset":
        print(f"layernorm_bwd fp32 rows={rows} C={C} {variant}: {e:.2e}")
        assert e < KTOL
        return
    floor32 = rel_err(_ln_ref(x, dy, add, gamma, torch.float32), ref)
    print(f"layernorm_bwd fp32 rows={rows} C={C} rows offset by 20 spreads: {e:.2e} (torch fp32 on the CPU: {floor32:.2e}, "
          f"bound {offset_bound(floor32):.2e})")
    assert e <= offset_bound(floor32)


# ------------------------------------------------------------------------------------------------ 3. map objective, fp32
def _map_objective(q, k, ref, B, heads, N, L, d, scale, dt):
    qf = q.to(dt).requires_grad_(True)
    sp = lambda t, n: t.reshape(B, n, heads, d).transpose(1, 2).reshape(B * heads, n, d)
    P = torch.softmax(sp(qf, N) @ sp(k.to(dt), L).transpose(1, 2) * scale, -1)
    loss = ((P - ref.to(dt)) ** 2).sum((1, 2)).mean(0)
    loss.backward()
    return loss.detach(), qf.grad


@pytest.mark.parametrize("B,heads,N,L,d,acc,with_loss", [
    (2, 2, 300, 77, 40, True, True), (1, 2, 64, 77, 160, False, True), (2, 1, 256, 77, 64, True, True),
    (2, 3, 1030, 77, 32, False, True), (1, 1, 100, 20, 80, True, True),       # the list of test_map_loss_kernel_vs_autograd
    (1, 1, 100, 20, 80, True, False),                                          # loss = None
    (3, 2, 65, 77, 40, False, True)])                                          # 390 map rows: a ragged last block of 64
def test_map_loss_f32_vs_autograd(B, heads, N, L, d, acc, with_loss, contraction):
    """`hip.attn_map_loss_bwd` on fp32 q / k / dq and fp32 reference maps (`ief_map_loss_rows_f32`, `ief_softmax_bwd_rows_f32`,
    `_attn_map_loss_bwd_f32`): dq and the objective value against fp64 autograd"""
    C = heads * d
    g = torch.Generator().manual_seed(0)
    q, k = torch.randn(B, N, C, generator=g), torch.randn(B, L, C, generator=g)
    ref = torch.softmax(torch.randn(B * heads, N, L, generator=g) * 2.0, -1)
    dq0 = torch.randn(B, N, C, generator=g) * 0.01
    scale, gs = d ** -0.5, 64.0
    loss64, grad64 = _map_objective(q, k, ref, B, heads, N, L, d, scale, torch.float64)
    want = grad64 * gs + (dq0.double() if acc else 0.0)
    rows = B * heads * N
    nblk = hip.map_loss_blocks_f32(rows)
    assert nblk == (rows + 63) // 64
    parts = torch.full((nblk + 3,), SENTINEL, device=DEV) if with_loss else None
    dq = dev(dq0.clone())
    hip.attn_map_loss_bwd(dev(q), dev(k), dev(ref), dq, heads, scale, gcoef=2.0 * gs / (B * heads), accumulate=acc,
                          loss=parts, loss_coef=1.0 / (B * heads))
    e = rel_err(dq, want)
    if not with_loss:
        print(f"map objective fp32 [{contraction}] B={B} h={heads} N={N} L={L} d={d} acc={acc} loss=None: dq {e:.2e}")
        assert e < KTOL
        return
    assert (parts[nblk:] == SENTINEL).all()                  # nothing written past the last block's partial
    loss32, _ = _map_objective(q, k, ref, B, heads, N, L, d, scale, torch.float32)
    floor32 = abs(loss32.item() - loss64.item()) / loss64.item()
    el = abs(parts[:nblk].double().sum().item() - loss64.item()) / loss64.item()
    bound = max(4.0 * floor32, 1e-6)
    print(f"map objective fp32 [{contraction}] B={B} h={heads} N={N} L={L} d={d} acc={acc}: dq {e:.2e}, objective {el:.2e} "
          f"(torch fp32 on the CPU: {floor32:.2e}, bound {bound:.2e})")
    assert e < KTOL and el <= bound


@pytest.mark.parametrize("L", [20, 77, 64, 333])
@pytest.mark.parametrize("rows", [1, 5, 4097])
def test_softmax_bwd_rows_f32(rows, L):
    """`ief_softmax_bwd_rows_f32` alone: dS = scale P o (dP - sum dP o P), in place on dP, one wave per row"""
    P = torch.softmax(f32(rows, L, seed=1, scale=2.0), -1)
    dP = f32(rows, L, seed=2)
    scale = 0.158
    ref = scale * P.double() * (dP.double() - (dP.double() * P.double()).sum(-1, keepdim=True))
    Pd, dPd = dev(P), dev(dP)
    out = hip._softmax_bwd_f32_(Pd, dPd, scale)
    e = rel_err(out, ref)
    print(f"softmax_bwd_rows fp32 rows={rows} L={L}: {e:.2e}")
    assert out.data_ptr() == dPd.data_ptr() and torch.equal(Pd.cpu(), P) and e < KTOL


@pytest.mark.parametrize("R,N,L", [(1, 1, 1), (3, 33, 31), (2, 130, 77), (5, 64, 64)])
def test_transpose_maps_f32_bit_equal(R, N, L):
    x = f32(R, N, L, seed=1)
    got = hip._transpose_maps_f32(dev(x))
    print(f"transpose_maps fp32 R={R} N={N} L={L}: bit-equal {torch.equal(got.cpu(), x.transpose(1, 2).contiguous())}")
    assert got.is_contiguous() and torch.equal(got.cpu(), x.transpose(1, 2).contiguous())


# ------------------------------------------------------------------------------------------------ attention references
@functools.lru_cache(maxsize=None)
def _attn_case(d, heads, B, N, L, qmul=1.0):
    """operands (fp32, CPU) of one attention layer and the fp64 gradients for the UNIT-scale dO (the gradients are linear in dO):
    q | k | v are column slices of one packed tensor where N == L, q alone and k | v packed otherwise"""
    C = heads * d
    qkv = torch.cat([f32(B, N, C, seed=1) * qmul, f32(B, N, C, seed=2), f32(B, N, C, seed=3)], -1)
    kv = None if L == N else torch.cat([f32(B, L, C, seed=2), f32(B, L, C, seed=3)], -1)
    do = f32(B, N, C, seed=4)
    q = qkv[..., :C]
    k, v = (qkv[..., C:2 * C], qkv[..., 2 * C:]) if L == N else (kv[..., :C], kv[..., C:])
    scale = d ** -0.5
    qf, kf, vf = (t.double().requires_grad_(True) for t in (q, k, v))
    sp = lambda t, n: t.reshape(B, n, heads, d).transpose(1, 2)
    sc = sp(qf, N) @ sp(kf, L).transpose(-1, -2) * scale
    P = torch.softmax(sc, -1)
    out = (P @ sp(vf, L)).transpose(1, 2).reshape(B, N, C)
    out.backward(do.double())
    with torch.no_grad():
        lse2 = torch.logsumexp(sc, -1) * LOG2E                                           # [B, heads, N], log2 units
        dP = sp(do.double(), N) @ sp(vf, L).transpose(-1, -2)
        ds_max = (P * (dP - (P * dP).sum(-1, keepdim=True))).abs().max().item()          # unit dO, without the score scale
        peaked = (P.max(-1).values > 0.9).double().mean().item()                         # share of rows close to one-hot
    return dict(qkv=qkv, kv=kv, do=do, out=out.detach(), lse2=lse2, ds_max=ds_max, peaked=peaked,
                grads=(qf.grad, kf.grad, vf.grad), C=C, scale=scale)


def _attn_device(case, N, L):
    C = case["C"]
    pk = dev(case["qkv"])
    q = pk[..., :C]
    if L == N:
        return q, pk[..., C:2 * C], pk[..., 2 * C:]
    kvd = dev(case["kv"])
    return q, kvd[..., :C], kvd[..., C:]


class _Dest:
    """gradient destinations as column slices of wider buffers filled with a sentinel"""

    def __init__(self, B, N, L, C):
        self.gq, self.gkv = torch.full((B, N, 2 * C), SENTINEL, device=DEV), torch.full((B, L, 3 * C), SENTINEL, device=DEV)
        self.dq, self.dk, self.dv = self.gq[..., C:], self.gkv[..., :C], self.gkv[..., 2 * C:]
        self.pad = (self.gq[..., :C], self.gkv[..., C:2 * C])

    def untouched(self, *ts):
        return all(bool((t == SENTINEL).all()) for t in ts + self.pad)


def _three_call_forms(case, B, N, L, heads, o, lse, do_mul, tol, label, kernel_prefix):
    q, k, v = _attn_device(case, N, L)
    do = dev(case["do"] * do_mul)
    refs = [g * do_mul for g in case["grads"]]
    worst = 0.0
    for want_dq, want_dkv in ((True, True), (True, False), (False, True)):
        dst = _Dest(B, N, L, case["C"])
        assert dst.untouched(dst.dq, dst.dk, dst.dv)                    # before the call: every destination holds the sentinel
        _, names = launched(lambda: hip.attn_bwd(q, k, v, o, do, lse, heads, case["scale"], dq=dst.dq, dk=dst.dk, dv=dst.dv,
                                                 want_dq=want_dq, want_dkv=want_dkv))
        fused = [n for n in names if n.startswith("attn_bwd_x3_kernel")]
        assert (len(fused) == 1 and len(names) == 1) if kernel_prefix == "fused" else not fused, names
        errs = {}
        if want_dq:
            errs["dq"] = rel_err(dst.dq, refs[0])
        else:
            assert dst.untouched(dst.dq), f"{label}: dQ was written although it was not requested"
        if want_dkv:
            errs["dk"], errs["dv"] = rel_err(dst.dk, refs[1]), rel_err(dst.dv, refs[2])
        else:
            assert dst.untouched(dst.dk, dst.dv), f"{label}: dK / dV were written although they were not requested"
        assert dst.untouched()                                           # the columns between the slices
        print(f"{label} want_dq={want_dq} want_dkv={want_dkv}: " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
        assert max(errs.values()) < tol
        worst = max(worst, *errs.values())
    return worst


# ------------------------------------------------------------------------------------------------ 4. materialised maps
@pytest.mark.parametrize("d,heads,B,N,L", [(40, 2, 1, 200, 77), (64, 3, 3, 130, 64), (80, 1, 2, 64, 36)])
def test_attn_bwd_materialised_call_forms(d, heads, B, N, L, contraction):
    """`hip.attn_bwd` without `lse` (materialised fp32 maps): all gradients, dQ only (`want_dkv=False`, grad.py's stop at the
    frozen context), dK / dV only (`want_dq=False`) -- both sides of the `% 4` switch between the in-place transposed product and
    the transposing path, batch 1 and batch 3 with 3 heads; what was not requested keeps its sentinel"""
    case = _attn_case(d, heads, B, N, L)
    _three_call_forms(case, B, N, L, heads, None, None, 0.05, KTOL, f"attn_bwd materialised [{contraction}] d={d} h={heads} B={B} "
                      f"N={N} L={L}", "materialised")


# ------------------------------------------------------------------------------------------------ 5. ief_attn_bwd_x3
def _fused_forward(case, N, L, heads):
    q, k, v = _attn_device(case, N, L)
    B = q.shape[0]
    lse = torch.full((B, heads, N), float("nan"), device=DEV)
    o = hip.attn_flash(q, k, v, heads, case["scale"], lse=lse)
    e_lse = (lse.double().cpu() - case["lse2"]).abs().max().item()
    assert rel_err(o, case["out"]) < 4e-6 and e_lse < 1e-5, (rel_err(o, case["out"]), e_lse)
    return q, k, v, o, lse


def _fused_grads(case, B, N, L, heads, do_mul, fwd=None):
    q, k, v, o, lse = fwd if fwd is not None else _fused_forward(case, N, L, heads)
    dst = _Dest(B, N, L, case["C"])
    _, names = launched(lambda: hip.attn_bwd(q, k, v, o, dev(case["do"] * do_mul), lse, heads, case["scale"], dq=dst.dq, dk=dst.dk,
                                             dv=dst.dv))
    assert len(names) == 1 and names[0].startswith("attn_bwd_x3_kernel"), names
    assert dst.untouched()
    return [rel_err(g, r * do_mul) for g, r in zip((dst.dq, dst.dk, dst.dv), case["grads"])]


@pytest.mark.parametrize("d,heads,B,N,L", [
    (40, 1, 1, 1, 128),          # one query; L = 128 exactly: the x3_fused_bwd_ok threshold
    (64, 1, 1, 128, 128),        # exactly one 128-column block and two 64-row tiles
    (40, 5, 3, 129, 257),        # one column past a block, one row past a tile; 30 and 45 workgroups: no multiple of 8 (xcd_remap)
    (64, 2, 1, 65, 193)])
def test_attn_bwd_x3_fused_edges(d, heads, B, N, L):
    with hip.f32_contraction("x3"):
        assert hip.x3_fused_bwd_ok(d, L) and not hip.x3_fused_bwd_ok(d, 127)
        errs = _fused_grads(_attn_case(d, heads, B, N, L), B, N, L, heads, 0.05)
    print(f"attn_bwd_x3 edges d={d} h={heads} B={B} N={N} L={L}: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}")
    assert max(errs) < XTOL_BWD


def test_attn_bwd_x3_fused_call_forms():
    """`ief_attn_bwd_x3` with what = 1 (dQ half only), what = 2 (dK / dV half only) and both: the half that is not launched writes
    nothing, the other is still right"""
    d, heads, B, N, L = 40, 2, 2, 320, 320
    case = _attn_case(d, heads, B, N, L)
    with hip.f32_contraction("x3"):
        q, k, v, o, lse = _fused_forward(case, N, L, heads)
        _three_call_forms(case, B, N, L, heads, o, lse, 0.05, XTOL_BWD, f"attn_bwd_x3 d={d} h={heads} B={B} N={N} L={L}", "fused")


@pytest.mark.parametrize("d", [40, 64])
def test_attn_bwd_x3_fused_full_size(d):
    """N = L = 4096, the 64 x 64 level of SD1.5, one head: all of dQ, dK, dV against the fp64 gradients of one 4096^2 map"""
    heads, B, N, L = 1, 1, 4096, 4096
    with hip.f32_contraction("x3"):
        errs = _fused_grads(_attn_case(d, heads, B, N, L), B, N, L, heads, 0.05)
    print(f"attn_bwd_x3 full size d={d} N=L=4096: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}")
    assert max(errs) < XTOL_BWD


def test_attn_bwd_x3_fused_do_magnitudes():
    """dO at 1.0, 0.05 and 1e-3 of unit scale.  dO is split with scale 1: at 1e-3 its lo halves (~1e-3 2^-11) are fp16 subnormals,
    the documented small-operand floor of the mode (2e-4, as `test_gemm_x3_operand_magnitudes`); dS is split with the fixed 2^14"""
    d, heads, B, N, L = 40, 2, 2, 320, 320
    case = _attn_case(d, heads, B, N, L)
    got = {}
    with hip.f32_contraction("x3"):
        fwd = _fused_forward(case, N, L, heads)
        for mul in (1.0, 0.05, 1e-3):
            assert case["ds_max"] * mul * hip.X3_SCALE_PROB < 65504.0        # the split of dS stays inside fp16
            got[mul] = _fused_grads(case, B, N, L, heads, mul, fwd)
            print(f"attn_bwd_x3 dO x {mul:g} (max |dS| {case['ds_max'] * mul:.2e}): dq {got[mul][0]:.2e} dk {got[mul][1]:.2e} "
                  f"dv {got[mul][2]:.2e}")
    assert max(got[1.0]) < XTOL_BWD and max(got[0.05]) < XTOL_BWD
    assert max(got[1e-3]) < SMALL_OPERAND_TOL


def test_attn_bwd_x3_fused_peaked_rows():
    """q x 4: many softmax rows close to one-hot (P spans its whole range inside one tile); max |dS| < 1 on the fp64 reference, so
    the fixed 2^14 split scale of dS is not what is being tested and nothing overflows"""
    d, heads, B, N, L = 40, 2, 2, 320, 320
    case = _attn_case(d, heads, B, N, L, 4.0)
    peaked = case["peaked"]
    assert case["ds_max"] * 0.05 < 1.0 and peaked > 0.05
    with hip.f32_contraction("x3"):
        errs = _fused_grads(case, B, N, L, heads, 0.05)
    print(f"attn_bwd_x3 peaked rows ({100 * peaked:.0f} % of the rows with max P > 0.9, max |dS| {case['ds_max'] * 0.05:.2e}): "
          f"dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}")
    assert max(errs) < XTOL_BWD


def test_attn_bwd_delta_f32in_strided():
    """`ief_attn_bwd_delta_f32in`: delta[b][h][n] = sum_d dO O with O and dO as column slices of wider buffers"""
    B, heads, N, d = 3, 5, 130, 40
    C = heads * d
    wo, wdo = f32(B, N, 3 * C, seed=1), f32(B, N, 2 * C, seed=2)
    od, dod = dev(wo)[..., C:2 * C], dev(wdo)[..., C:]
    delta = torch.full((B, heads, N), float("nan"), device=DEV)
    hip._check(hip.load().ief_attn_bwd_delta_f32in(od.data_ptr(), dod.data_ptr(), delta.data_ptr(), B, heads, N, d, od.stride(1),
                                                   dod.stride(1), hip._stream()), "ief_attn_bwd_delta_f32in")
    ref = (wo[..., C:2 * C].double() * wdo[..., C:].double()).reshape(B, N, heads, d).sum(-1).transpose(1, 2)
    e = rel_err(delta, ref)
    print(f"attn_bwd_delta_f32in B={B} h={heads} N={N} d={d}, strided: {e:.2e}")
    assert e < 2e-6


# ------------------------------------------------------------------------------------------------ 6. conv helpers, GEGLU
SIZES_BHWC = [(3, 5, 7, 4), (1, 8, 12, 1284), (2, 64, 64, 320)]


@pytest.mark.parametrize("B,H,W,C", SIZES_BHWC)
def test_zero_insert2x_f32_bit_equal(B, H, W, C):
    """the last size is 10240 workgroups' worth of float4: past the 8192-workgroup cap, the grid-stride term runs"""
    x = f32(B, H, W, C, seed=1)
    want = torch.zeros(B, 2 * H, 2 * W, C)
    want[:, ::2, ::2] = x
    got = hip.zero_insert2x(dev(x)).cpu()
    print(f"zero_insert2x fp32 {B}x{H}x{W}x{C}: bit-equal {torch.equal(got, want)}")
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,H,W,C", SIZES_BHWC + [(2, 128, 132, 256)])
def test_pool2x2_sum_f32(B, H, W, C):
    """output sizes; the added last one is 8448 workgroups' worth of float4 (the issue's three stay below the cap)"""
    x = f32(B, 2 * H, 2 * W, C, seed=1)
    xd = x.double()
    ref = xd[:, ::2, ::2] + xd[:, ::2, 1::2] + xd[:, 1::2, ::2] + xd[:, 1::2, 1::2]
    e = rel_err(hip.pool2x2_sum(dev(x)), ref)
    print(f"pool2x2_sum fp32 -> {B}x{H}x{W}x{C}: {e:.2e}")
    assert e < 2e-7


@pytest.mark.parametrize("B,C,H,W,Cout", [(3, 320, 8, 12, 4), (1, 4, 5, 7, 16), (2, 320, 64, 64, 4), (1, 320, 168, 160, 4)])
def test_conv_out_bwd_f32w_nonsquare(B, C, H, W, Cout):
    """H != W; the added last size is 8400 workgroups' worth of float4 (the issue's three stay below the cap)"""
    w = f32(Cout, C, 3, 3, seed=2, scale=(9 * C) ** -0.5)
    x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    de = f32(B, Cout, H, W, seed=3)
    F.conv2d(x, w.double(), padding=1).backward(de.double())
    got = hip.conv_out_bwd(dev(de), dev(w.permute(0, 2, 3, 1).contiguous()))
    e = rel_err(got.permute(0, 3, 1, 2), x.grad)
    print(f"conv_out_bwd fp32 weights B={B} C={C} {H}x{W} Cout={Cout}: {e:.2e}")
    assert e < KTOL


def test_conv3x3_data_gradients_nonsquare(contraction):
    """the 3x3 data gradients as grad.py forms them (`UNetAdjoint.wt_conv`; plain, stride 2 through the zero-inserted gradient,
    nearest-2x through the 2x2 block sum) on an 8 x 12 image: a swap of H and W cannot hide"""
    B, Cin, Cout, H, W = 3, 64, 160, 8, 12
    xc, w = f32(B, Cin, H, W, seed=1), f32(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    adj = UNetAdjoint.__new__(UNetAdjoint)
    adj._wt = {}
    wt = adj.wt_conv(dev(nhwc(w)))
    for mode in ("plain", "stride2", "upsample"):
        xi = xc.double().requires_grad_(True)
        if mode == "plain":
            y = F.conv2d(xi, w.double(), padding=1)
        elif mode == "stride2":
            y = F.conv2d(xi, w.double(), padding=1, stride=2)
        else:
            y = F.conv2d(F.interpolate(xi, scale_factor=2.0, mode="nearest"), w.double(), padding=1)
        dyc = f32(*y.shape, seed=3, scale=0.1)
        y.backward(dyc.double())
        dd = dev(nhwc(dyc))
        got = hip.conv3x3(dd, wt) if mode == "plain" else hip.conv3x3(hip.zero_insert2x(dd), wt) if mode == "stride2" \
            else hip.pool2x2_sum(hip.conv3x3(dd, wt))
        e = rel_err(got.permute(0, 3, 1, 2), xi.grad)
        print(f"conv data gradient fp32 [{contraction}, {mode}] {H}x{W}: {e:.2e}")
        assert e < KTOL


@pytest.mark.parametrize("rows,Ch", [(1, 8), (300, 640), (4100, 1280)])
def test_geglu_il_bwd_f32_tails(rows, Ch):
    """gates drawn at scale 4: |g| reaches the erf and exp tails; the last size is past the 8192-workgroup cap"""
    pre = f32(rows, 2 * Ch, seed=1).reshape(rows, Ch // 8, 2, 8)
    pre[:, :, 1] *= 4.0
    dy = f32(rows, Ch, seed=2, scale=0.1)
    p = pre.double().requires_grad_(True)
    (p[:, :, 0] * F.gelu(p[:, :, 1])).reshape(rows, Ch).backward(dy.double())
    e = rel_err(hip.geglu_il_bwd(dev(pre.reshape(rows, 2 * Ch)), dev(dy)), p.grad.reshape(rows, 2 * Ch))
    print(f"geglu_il_bwd fp32 rows={rows} Ch={Ch} (max |gate| {pre[:, :, 1].abs().max():.1f}): {e:.2e}")
    assert e < KTOL


# ------------------------------------------------------------------------------------------------ 7. lse of the planes-in attention
@pytest.mark.parametrize("B,heads,N,L,d", [(2, 2, 200, 144, 64), (1, 3, 130, 257, 40)])
def test_attention_planes_in_writes_lse(B, heads, N, L, d):
    """`attn_flash_x3p_kernel` with `lse`: a buffer pre-filled with NaN comes back as logsumexp(scores) log2(e) (the units of
    `attn_flash_x3_kernel`), and `ief_attn_bwd_x3` fed with it gives the gradients -- never IEF_OK with the buffer untouched"""
    case = _attn_case(d, heads, B, N, L)
    with hip.f32_contraction("x3"):
        q, k, v = _attn_device(case, N, L)
        qp, kp, vp = planes.split(q.contiguous()), planes.split(k.contiguous()), planes.split(v.contiguous())
        lse = torch.full((B, heads, N), float("nan"), device=DEV)
        o = planes.attn_flash(qp, kp, vp, heads, case["scale"], out_planes=False, lse=lse)
        assert torch.isfinite(lse).all(), "planes-in attention returned without writing lse"
        e_o, e_lse = rel_err(o, case["out"]), (lse.double().cpu() - case["lse2"]).abs().max().item()
        errs = _fused_grads(case, B, N, L, heads, 0.05, (q, k, v, o, lse))
    print(f"attention planes-in lse B={B} h={heads} N={N} L={L} d={d}: out {e_o:.2e} lse {e_lse:.2e} | dq {errs[0]:.2e} "
          f"dk {errs[1]:.2e} dv {errs[2]:.2e}")
    assert e_o < 4e-6 and e_lse < 1e-5 and max(errs) < XTOL_BWD


def test_attn_flash_f32_refuses_lse_it_would_not_write():
    """the fp32-MFMA attention kernel has no lse output: `ief_attn_flash_f32` with x3 == 0 and a non-null lse is IEF_EINVAL, not
    IEF_OK with the buffer untouched (argument check only: nothing is launched)"""
    B, heads, N, L, d = 1, 1, 64, 128, 40
    q, k, v, out = (torch.zeros(B, n, d, device=DEV) for n in (N, L, L, N))
    lse = torch.full((B, heads, N), float("nan"), device=DEV)
    p = hip.IefAttnF32Params()
    p.Q, p.K, p.V, p.Out, p.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr()
    p.B, p.heads, p.N, p.L, p.d, p.scale = B, heads, N, L, d, d ** -0.5
    p.sQb, p.ldq, p.sKb, p.ldk, p.sVb, p.ldv, p.sOb, p.ldo = N * d, d, L * d, d, L * d, d, N * d, d
    p.x3 = 0
    assert hip.load().ief_attn_flash_f32(byref(p), hip._stream()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(lse).all()
