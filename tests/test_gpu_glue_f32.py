"""The forward glue kernels of the two fp32-storage modes (`f32`, `f16x3`), one by one, against fp64 at the shapes and branches they
run in on a real MI355X: LayerNorm (fp32 out and operand planes out), row softmax, the Prompt-to-Prompt edit on materialised maps,
add / SiLU / row gather / GEGLU / the CFG + DDIM update past their grid caps, the timestep embedding, the boundary convolutions,
the uint8 image epilogue and the weight split into fp16 hi / lo planes.

tests/test_gpu_exact.py checks each of them at one friendly shape (`test_norms_and_elementwise_f32`,
`test_boundary_convs_and_image_epilogue_f32`); this file adds the shapes at which the kernels take another path: every register-row
form of the LayerNorm and its scalar fallback, all four softmax kernels at both sides of their thresholds, odd key counts and ragged
row blocks of the map edit, the second trip of every capped grid-stride loop, the scalar GEGLU, the generic `conv_in`, the `<2>` and
the non-LDS `conv_out`, and operands that are not 16-byte aligned (an error code, never a launch).  None of these entry points is
timed by `hip.profile_begin()`, so no launch name can be asserted: the comment beside each case names the kernel that the dispatch
code of `csrc/exact_f32.hip` / `csrc/split_x3.hip` / `csrc/elementwise.hip` selects for it.

Every reference is torch on the CPU in fp64, or exact integer / bit arithmetic, computed inside the test from the fp32 inputs; no
kernel of this library serves as a reference.  Stated tolerances (relative to max |reference| unless said otherwise; every test
prints what it measured):
    single fp32 kernels (LayerNorm, map edit, conv_in, conv_out)                          <= 2e-5   (KTOL)
    LayerNorm on rows offset by 20 of their spreads: <= 4 x the error of torch's own fp32 evaluation on the CPU, KTOL as the floor
        (fp32 statistics lose accuracy there by construction; 4 covers a different summation order)
    softmax maps <= 1e-6 absolute, row sums within 1e-6 of 1
    add <= 1e-7, SiLU <= 1e-6, GEGLU <= 1e-6                (the bounds of `test_norms_and_elementwise_f32`)
    CFG + DDIM update <= 2e-6 max |ref| + 1e-6              (the bound of `test_cfg_ddim_step_matches_eager_formula`)
    timestep embedding <= 2e-4 absolute against the fp32 torch expression; the row of t = 0 exactly [1 .. 1 | 0 .. 0]
    operand planes, weight planes, gathered rows, uint8 images, rows that are not edited, everything behind the last row: bit-equal

One case of the issue is run differently from how it is worded: C = 100 is a multiple of 4, so `ief_layernorm_f32` takes
`layernorm_f32_vec_kernel<2>` with 25 quads for it (not the scalar kernel) and `ief_layernorm_x3p` accepts it.  It stays in the
list and is checked in both forms; C = 102 is added as the width the scalar kernel really takes and the planes entry refuses.

Measured on the MI355X (largest of each group):
    LayerNorm fp32       1.6e-7 (vector forms), 1.1e-7 (scalar kernel); rows offset by 20 spreads 6.7e-7 / 6.8e-7 (torch fp32 on the
                         CPU 3.3e-7 .. 8.3e-7, so the bound is its floor, KTOL); planes bit-equal at every shape, sentinels kept
    row softmax          1.8e-7 absolute (L = 65), row sums off by at most 2.1e-7; shifted rows and one-hot rows no worse
    map edit             8.5e-8; rows that are not edited bit-equal
    add 5.4e-8, SiLU 7.0e-8, GEGLU 8.0e-8 (vector form) / 5.1e-8 (scalar, bit-equal to the vector form), gather bit-equal
    CFG + DDIM update    t = 981: 9.5e-6 absolute against a bound of 1.7e-5 (x0: 9.8e-5 against 1.2e-3); t = 1: 6.8e-7 against 1.1e-5
    timestep embedding   6.1e-5 absolute; the row of t = 0 exact
    conv_in 2.5e-7, conv_out 3.2e-7, uint8 image: no byte differs, weight planes bit-equal (6.4 M fp16-subnormal lo halves)
    the whole file       3.1 s (84 tests), library load excluded
No kernel had to change for these.  The alignment guards of section 8 were added with this file: before it, `ief_conv_out_f32act`,
`ief_conv_in_f32act`, `ief_x3_split_weights`, `ief_gemm_f32` and `ief_attn_flash_f32` (x3 == 0) launched on a misaligned operand,
and the one-launch `ief_groupnorm_silu_f32` read channel pairs from a source that was not 8-byte aligned.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ief_amd import hip, planes  # noqa: E402
from ief_amd.scheduler import DDIMScheduler  # noqa: E402
from oracle import unet_ref  # noqa: E402

DEV = torch.device("cuda:0")
KTOL = 2e-5
SENTINEL = 7.0


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return None if t is None else t.to(DEV)


def offset_bound(floor32):
    """inputs far from zero: 4 x what torch's own fp32 evaluation of the expression loses, never below KTOL"""
    return max(4.0 * floor32, KTOL)


def one_float_off(t):
    """the values of t as a contiguous device view that starts 4 bytes past 16-byte alignment"""
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ------------------------------------------------------------------------------------------------ 1. LayerNorm
# (rows, C, x one float off alignment, planes form exists)            kernel of ief_layernorm_f32 | ief_layernorm_x3p
LN_CASES = [
    (1, 64, False, True),        # layernorm_f32_vec_kernel<2>, 16 quads: 48 idle lanes; one row: three idle waves
    (5, 512, False, True),       # <2> at its upper edge (two full pieces per lane); the second workgroup has one live wave
    (7, 516, False, True),       # <5>, one quad past <2>
    (301, 1280, False, True),    # <5> at its upper edge
    (3, 1284, False, True),      # <10>, one quad past <5>
    (4099, 320, False, True),    # <2>; 1025 workgroups, the last with three idle waves
    (2, 2560, False, True),      # <10> at its upper edge
    (7, 100, False, True),       # <2> with 25 quads (100 % 4 == 0: see the module docstring)
    (7, 102, False, False),      # C % 4 != 0   -> layernorm_f32_kernel (scalar)       | IEF_ESHAPE
    (3, 2564, False, False),     # C > 2560     -> layernorm_f32_kernel (scalar)       | IEF_ESHAPE
    (9, 640, True, False),       # x misaligned -> layernorm_f32_kernel (scalar)       | (IEF_EALIGN: test_misaligned_operands_are_refused)
]


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("rows,C,misalign,has_planes", LN_CASES)
def test_layernorm_f32_and_planes_forms(rows, C, misalign, has_planes, offset):
    """`hip.layernorm` (fp32) against fp64 and `planes.layernorm` bit for bit against the split definition of that fp32 output, on
    unit gaussian rows and on rows offset by 20 of their spreads; rows behind the last one keep their sentinel"""
    x = f32(rows, C, seed=1)
    if offset:
        sign = 1.0 - 2.0 * (torch.arange(rows) % 2).float()
        x = x + (20.0 * x.std(1) * sign)[:, None]
    gamma, beta = 1 + f32(C, seed=2, scale=0.1), f32(C, seed=3, scale=0.1)
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    xd, gd, bd = (one_float_off(x) if misalign else dev(x)), dev(gamma), dev(beta)
    # the branch condition of ief_layernorm_f32, restated: a case must not quietly move to another kernel
    vec = C % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (xd, gd, bd))
    assert vec == (C % 4 == 0 and not misalign) and has_planes == (vec and C <= 2560)
    buf = torch.full((rows + 3, C), SENTINEL, device=DEV)
    y = hip.layernorm(xd, gd, bd, out=buf[:rows])
    assert y.data_ptr() == buf.data_ptr() and bool((buf[rows:] == SENTINEL).all()), "rows past `rows` were written"
    e = rel_err(y, ref)
    what = f"layernorm fp32 rows={rows} C={C}{' x one float off alignment' if misalign else ''}"
    if offset:
        floor32 = rel_err(F.layer_norm(x, (C,), gamma, beta, 1e-5), ref)
        print(f"{what} rows offset by 20 spreads: {e:.2e} (torch fp32 on the CPU: {floor32:.2e}, bound {offset_bound(floor32):.2e})")
        assert e <= offset_bound(floor32)
    else:
        print(f"{what}: {e:.2e}")
        assert e < KTOL
    if not has_planes:
        if not misalign:
            with pytest.raises(RuntimeError, match="IEF_ESHAPE"):
                planes.layernorm(xd, gd, bd)
        return
    yc = y.cpu()
    hi = yc.half()
    lo = (yc - hi.float()).half()
    p = planes.layernorm(xd, gd, bd)
    same_hi, same_lo = torch.equal(bits(p.hi), bits(hi)), torch.equal(bits(p.lo), bits(lo))
    # the entry point itself, into planes with sentinel rows behind them
    pb = torch.full((2, rows + 3, C), SENTINEL, dtype=torch.float16, device=DEV)
    hip._check(hip.load().ief_layernorm_x3p(xd.data_ptr(), pb.data_ptr(), pb.stride(0), gd.data_ptr(), bd.data_ptr(), rows, C, 1e-5,
                                            hip._stream()), "ief_layernorm_x3p")
    tail_ok = bool((pb[:, rows:] == SENTINEL).all())
    same_raw = torch.equal(bits(pb[0, :rows]), bits(hi)) and torch.equal(bits(pb[1, :rows]), bits(lo))
    print(f"layernorm planes rows={rows} C={C} offset={offset}: hi bit-equal {same_hi}, lo bit-equal {same_lo}, with sentinel rows "
          f"behind {same_raw}, sentinel kept {tail_ok}")
    assert same_hi and same_lo and same_raw and tail_ok


# ------------------------------------------------------------------------------------------------ 2. row softmax
# L -> kernel of ief_softmax_rows_f32: 1, 64, 65, 128 softmax_rows_f32_reg_kernel<2>; 129, 1024 <16>; 1025, 4096 <64> (64 floats per
# lane in registers); 4097, 9216 softmax_rows_f32_kernel (the loop); 5 rows: the second workgroup has one live wave
@pytest.mark.parametrize("kind", ["gauss4", "shift1e4", "peak80"])
@pytest.mark.parametrize("L", [1, 64, 65, 128, 129, 1024, 1025, 4096, 4097, 9216])
def test_softmax_rows_f32_every_kernel(L, kind):
    rows = 5
    s = f32(rows, L, seed=L) * 4
    if kind == "shift1e4":
        s = s + (1e4 * (1.0 - 2.0 * (torch.arange(rows) % 2).float()))[:, None]
    elif kind == "peak80":
        idx = (torch.arange(rows) * 7919) % L
        s[torch.arange(rows), idx] = 0.0
        s[torch.arange(rows), idx] = s.max(1).values + 80.0
    ref = torch.softmax(s.double(), -1)
    buf = torch.full((rows * L + 67,), SENTINEL, device=DEV)
    view = buf[:rows * L].view(rows, L)
    view.copy_(s)
    out = hip.softmax_rows_(view)
    got = out.double().cpu()
    e, es = (got - ref).abs().max().item(), (got.sum(-1) - 1.0).abs().max().item()
    tail_ok = bool((buf[rows * L:] == SENTINEL).all())
    print(f"softmax_rows fp32 L={L} {kind}: max abs err {e:.2e}, row sums off by {es:.2e}, sentinel kept {tail_ok}")
    assert out.data_ptr() == buf.data_ptr() and torch.isfinite(got).all() and tail_ok
    assert e < 1e-6 and es < 1e-6


# ------------------------------------------------------------------------------------------------ 3. P2P edit on materialised maps
# p2p_cross_edit_f32_kernel: (1, 1, 77) one row (31 duplicate lanes), odd L: ksteps = 39, the last step half padding;
# (3, 129, 33) a second workgroup with one live row, L one past a 32-column tile; (2, 300, 96) all three column tiles, 300 % 128 = 44;
# (2, 31, 1) N < 32, one key; (8, 256, 40) the SD shape of heads and rows with 40 keys
@pytest.mark.parametrize("heads,N,L", [(1, 1, 77), (3, 129, 33), (2, 300, 96), (2, 31, 1), (8, 256, 40)])
def test_p2p_cross_edit_f32_shapes(heads, N, L):
    B = 4
    g = torch.Generator().manual_seed(0)
    mt, coef = torch.zeros(2, 96, 96), torch.zeros(2, 2, 96)
    Ms, cs = [], []
    for s in range(2):              # the tables of test_cross_attention_p2p_edit_fused_x3
        mapper = torch.randint(-1, L, (L,), generator=g)
        mapper[L // 2] = -1 if (L > 1 or s == 0) else 0
        a = (mapper != -1).float()
        M = torch.zeros(L, L)
        M[mapper % L, torch.arange(L)] = 1.0
        if L > 6:
            M[5, 5], M[5, 6] = 1.0 / 3.0, 2.0 / 3.0         # not fp16 numbers
        gate = (torch.rand(L, generator=g) > 0.3).float() * (0.25 + 0.75 * torch.rand(L, generator=g))
        c1, c2 = gate * a, 1 - gate * a
        mt[s, :L, :L] = M.t()
        coef[s, 0, :L], coef[s, 1, :L] = c1, c2
        Ms.append(M.double()), cs.append((c1.double(), c2.double()))
    es, sl = torch.tensor([-1, 0, -1, 2], dtype=torch.int32), torch.tensor([0, 1, 0, 0], dtype=torch.int32)
    P = torch.softmax(f32(B * heads, N, L, seed=1, scale=2.0), -1)
    P4 = P.double().view(B, heads, N, L)
    buf = torch.full((P.numel() + 61,), SENTINEL, device=DEV)
    maps = buf[:P.numel()].view(B * heads, N, L)
    maps.copy_(P)
    out = hip.p2p_cross_edit_(maps, B, heads, dev(es), dev(sl), dev(mt), dev(coef))
    got = out.cpu().view(B, heads, N, L)
    assert out.data_ptr() == buf.data_ptr() and bool((buf[P.numel():] == SENTINEL).all())
    worst = 0.0
    for b in range(B):
        if es[b] < 0:
            assert torch.equal(bits(got[b]), bits(P.view(B, heads, N, L)[b])), f"batch row {b} is not edited and changed"
            continue
        c1, c2 = cs[sl[b]]
        worst = max(worst, rel_err(got[b], c1 * (P4[es[b]] @ Ms[sl[b]]) + c2 * P4[b]))
    print(f"p2p_cross_edit fp32 heads={heads} N={N} L={L}: edited rows {worst:.2e}, other rows bit-equal")
    assert worst < KTOL


# ------------------------------------------------------------------------------------------------ 4. past the grid caps
@pytest.mark.parametrize("n", [3, 4096 * 256 + 1027])
def test_add_silu_f32_past_the_grid_cap(n):
    """`ew_f32_kernel` (which = 0, 1) caps its grid at 4096 workgroups: the larger n takes the second trip of the loop, with 1027
    elements in it; n = 3: one partial workgroup"""
    a, b = f32(n, seed=1) * 3 + 1, f32(n, seed=2)
    ea = rel_err(hip.add(dev(a), dev(b)), a.double() + b.double())
    es = rel_err(hip.silu(dev(a)), F.silu(a.double()))
    print(f"add / silu fp32 n={n}: add {ea:.2e}, silu {es:.2e}")
    assert ea < 1e-7 and es < 1e-6


def test_gather_rows_f32_past_the_grid_cap():
    """`gather_rows_f32_kernel` caps at 2048 workgroups = 524288 quads; 3 rows of 175000 quads are 525000"""
    x = f32(3, 4 * 175000, seed=1)
    src = torch.tensor([2, 0, 2], dtype=torch.int32)
    got = hip.gather_rows(dev(x), dev(src))
    same = torch.equal(bits(got), bits(x[src.long()]))
    print(f"gather_rows fp32 3 x {4 * 175000}: bit-equal {same}")
    assert same


def _geglu_ref(pre, Ch):
    grp = pre.double().reshape(-1, Ch // 8, 2, 8)
    return (grp[:, :, 0] * F.gelu(grp[:, :, 1])).reshape(-1, Ch)


def test_geglu_il_f32_vector_form_past_the_grid_cap():
    """`geglu_il_f32_vec_kernel` caps at 16384 workgroups = 4194304 output quads; 3300 rows of 1280 quads are 4224000.  The first 8
    rows, the last 8 (second trip) and the 16 around output quad 4194304 (row 3276) against fp64"""
    rows, Ch = 3300, 5120
    pre = f32(rows, 2 * Ch, seed=1)
    mid = 4194304 // (Ch // 4)
    assert rows * (Ch // 4) > 4194304 and 8 <= mid - 8 and mid + 8 <= rows - 8
    sel = torch.cat([torch.arange(0, 8), torch.arange(mid - 8, mid + 8), torch.arange(rows - 8, rows)])
    got = hip.geglu_il(dev(pre))
    assert got.shape == (rows, Ch)
    e = rel_err(got[dev(sel)], _geglu_ref(pre[sel], Ch))
    print(f"geglu_il fp32 vector form rows={rows} Ch={Ch} (rows 0-7, {mid - 8}-{mid + 7}, {rows - 8}-{rows - 1}): {e:.2e}")
    assert e < 1e-6


def test_geglu_il_f32_scalar_fallback():
    """a base pointer that is not 16-byte aligned: `ew_f32_kernel` with which = 2, same bits as the vector form"""
    rows, Ch = 50, 64
    pre = f32(rows, 2 * Ch, seed=8)
    got = hip.geglu_il(one_float_off(pre))
    vec = hip.geglu_il(dev(pre))
    e, same = rel_err(got, _geglu_ref(pre, Ch)), torch.equal(bits(got), bits(vec))
    print(f"geglu_il fp32 scalar fallback rows={rows} Ch={Ch}: {e:.2e}, bit-equal to the vector form {same}")
    assert e < 1e-6 and same


@pytest.mark.parametrize("with_x0", [False, True])
@pytest.mark.parametrize("t", [981, 1])
def test_cfg_ddim_step_past_the_grid_cap(t, with_x0):
    """`cfg_ddim_kernel` caps at 2048 workgroups = 524288 elements: 515 more take the second trip; the fp64 formula of
    `test_cfg_ddim_step_matches_eager_formula` evaluated on the fp32 coefficients the kernel reads"""
    n = 2048 * 256 + 515
    s = DDIMScheduler()
    s.set_timesteps(50)
    coef = torch.tensor([*s.step_coeffs(t), 7.5])
    eu, ec, x = f32(n, seed=1), f32(n, seed=2), f32(n, seed=3)
    a_f, a_t, g = coef.double().tolist()
    e = eu.double() + g * (ec.double() - eu.double())
    x0 = (x.double() - math.sqrt(1 - a_f) * e) / math.sqrt(a_f)
    ref = math.sqrt(a_t) * x0 + math.sqrt(1 - a_t) * e
    x0d = torch.full((n + 5,), SENTINEL, device=DEV) if with_x0 else None
    out = hip.cfg_ddim_step(dev(eu), dev(ec), dev(x), dev(coef), x0_out=None if x0d is None else x0d[:n])
    err = (out.double().cpu() - ref).abs().max().item()
    bound = 2e-6 * ref.abs().max().item() + 1e-6
    print(f"cfg_ddim_step n={n} t={t} x0_out={with_x0}: max abs err {err:.2e} (bound {bound:.2e})")
    assert torch.isfinite(out).all() and err <= bound
    if with_x0:
        err0 = (x0d[:n].double().cpu() - x0).abs().max().item()
        bound0 = 2e-6 * x0.abs().max().item() + 1e-6
        print(f"cfg_ddim_step n={n} t={t} x0: max abs err {err0:.2e} (bound {bound0:.2e})")
        assert err0 <= bound0 and bool((x0d[n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 5. timestep embedding
@pytest.mark.parametrize("dim", [320, 1280, 256])
def test_timestep_embedding_f32(dim):
    """SD's 320, 1280 and SDXL's `add_time_proj` (256); t = 0 must give cos = 1, sin = 0 exactly"""
    t = torch.tensor([0.0, 1.0, 500.0, 981.0, 999.0])
    emb = hip.timestep_embedding(dev(t), dim, dtype=torch.float32).cpu()
    ref = unet_ref.timestep_embedding(t, dim)
    e = (emb - ref).abs().max().item()
    row0 = torch.cat([torch.ones(dim // 2), torch.zeros(dim // 2)])
    print(f"timestep_embedding fp32 dim={dim}: max abs err {e:.2e}, row of t = 0 exact {torch.equal(emb[0], row0)}")
    assert emb.shape == (5, dim) and e < 2e-4 and torch.equal(emb[0], row0)


# ------------------------------------------------------------------------------------------------ 6. boundary convolutions, image
# ief_conv_in_f32act: Cin = 3 (the VAE encoder's 3 -> 128) and Cin = 8 take conv_in_f32_kernel<0>, Cin = 4 conv_in_f32_kernel<4>;
# the last case is 2129920 work items against the cap of 8192 x 256 = 2097152: the last rows of the second image are the second trip
@pytest.mark.parametrize("B,Cin,H,W,Cout,edge_rows_only", [(1, 3, 9, 7, 128, False), (2, 8, 5, 6, 64, False),
                                                          (2, 4, 128, 104, 320, True)])
def test_conv_in_f32_generic_kernel_and_grid_cap(B, Cin, H, W, Cout, edge_rows_only):
    x = f32(B, Cin, H, W, seed=1)
    w, bias = f32(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5), f32(Cout, seed=3, scale=0.1)
    got = hip.conv_in(dev(x), dev(w.permute(2, 3, 1, 0).contiguous()), dev(bias))
    assert got.shape == (B, H, W, Cout) and got.dtype == torch.float32
    if edge_rows_only:      # the first and the last pixel row of every image, from the two input rows each of them sees
        assert B * H * W * (Cout // 4) > 8192 * 256
        top = F.conv2d(F.pad(x[:, :, :2].double(), (1, 1, 1, 0)), w.double(), bias.double())
        bot = F.conv2d(F.pad(x[:, :, -2:].double(), (1, 1, 0, 1)), w.double(), bias.double())
        ref = torch.cat([top, bot], 2).permute(0, 2, 3, 1)
        got = got[:, [0, H - 1]]
    else:
        ref = F.conv2d(x.double(), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    e = rel_err(got, ref)
    print(f"conv_in fp32 B={B} {Cin} -> {Cout} {H}x{W}{' (first and last image rows)' if edge_rows_only else ''}: {e:.2e}")
    assert e < KTOL


# ief_conv_out_f32act: (1, 128, 9, 7, 3) conv_out_f32_lds_kernel<2> (the VAE decoder's 128 -> 3), 63 pixels: the last workgroup has one
# idle pixel slot; (2, 4, 3, 5, 4) <2> with ONE channel quad, 30 pixels; (1, 320, 16, 16, 4) <5>, the anchor;
# (1, 320, 8, 8, 8) Cout > 4 and (1, 512, 5, 5, 4) 72 KiB of weights: conv_out_f32_kernel (no LDS)
@pytest.mark.parametrize("B,C,H,W,Cout", [(1, 128, 9, 7, 3), (2, 4, 3, 5, 4), (1, 320, 16, 16, 4), (1, 320, 8, 8, 8), (1, 512, 5, 5, 4)])
def test_conv_out_f32_every_form(B, C, H, W, Cout):
    lds_form = Cout * 9 * C * 4 <= 48 * 1024 and C <= 320 and Cout <= 4       # the dispatch of ief_conv_out_f32act, restated
    assert lds_form == ((C, Cout) in ((128, 3), (4, 4), (320, 4)))
    x = f32(B, H, W, C, seed=1)
    w, bias = f32(Cout, C, 3, 3, seed=2, scale=(9 * C) ** -0.5), f32(Cout, seed=3, scale=0.1)
    got = hip.conv_out(dev(x), dev(w.permute(0, 2, 3, 1).contiguous()), dev(bias))
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), bias.double(), padding=1)
    e = rel_err(got, ref)
    print(f"conv_out fp32 B={B} {C} -> {Cout} {H}x{W} [{'LDS' if lds_form else 'no LDS'}]: {e:.2e}")
    assert got.shape == (B, Cout, H, W) and e < KTOL


@pytest.mark.parametrize("B,C,H,W", [(2, 3, 420, 420), (2, 1, 37, 41)])
def test_image_u8_edges_and_grid_cap(B, C, H, W):
    """`image_u8_kernel` caps at 4096 workgroups = 1048576 elements; 2 x 3 x 420 x 420 are 1058400.  Planted over the whole tensor,
    its last elements included: the clamp's ends, values beyond them, large finite values, and the fp32 pre-images of k / 255
    with their neighbours one ulp below and above (where truncation decides the level)"""
    img = f32(B, C, H, W, seed=6) * 0.8
    ks = torch.tensor([0, 1, 127, 128, 254, 255], dtype=torch.float64)
    pre = (2.0 * ks / 255.0 - 1.0).float()
    inf = torch.tensor(float("inf"))
    special = torch.cat([torch.tensor([-1.0, 1.0, 1.5, -1.5, 3.0e38, -3.0e38, 1e-30, -1e-30, 0.0]), pre, torch.nextafter(pre, -inf),
                         torch.nextafter(pre, inf)])
    flat = img.view(-1)
    pos = torch.linspace(0, flat.numel() - 1, 4 * special.numel()).long()
    flat[pos] = special.repeat(4)
    flat[-special.numel():] = special                       # the tail of the second trip
    got = hip.image_u8(dev(img)).cpu().numpy()
    want = ((img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy() * 255).astype("uint8")     # sd_utils.py:85-88
    ndiff = int((got != want).sum())
    print(f"image_u8 {B}x{C}x{H}x{W}: {ndiff} bytes differ from the fp32 expression, levels present {len(set(want.reshape(-1).tolist()))}")
    assert got.shape == (B, H, W, C) and ndiff == 0


# ------------------------------------------------------------------------------------------------ 7. weight split
@pytest.mark.parametrize("shape", [(1, 4), (2560, 320), (8, 2097153)])
def test_x3_weight_planes_bit_equal(shape):
    """`x3_split_weights_kernel` caps at 16384 workgroups = 4194304 quads; 8 x 2097153 floats are 4194306.  |w| from 1e-6 to 200 at the
    weight scale 2^8: hi = fp16(256 w), lo = fp16(256 w - hi), the lo halves of the small ones fp16 subnormals"""
    n = shape[0] * shape[1]
    assert n % 4 == 0
    g = torch.Generator().manual_seed(n)
    mag = torch.exp(torch.rand(n, generator=g) * (math.log(200.0) - math.log(1e-6)) + math.log(1e-6))
    w = (mag * (1.0 - 2.0 * (torch.rand(n, generator=g) > 0.5).float())).view(shape)
    w.view(-1)[:4] = torch.tensor([200.0, -200.0, 1e-6, -1e-6])
    w.view(-1)[-2:] = torch.tensor([200.0, 1e-6])
    wd = dev(w)
    p = hip.x3_weight_planes(wd)
    sw = w * 256.0
    hi = sw.half()
    lo = (sw - hi.float()).half()
    same_hi, same_lo = torch.equal(bits(p[0]), bits(hi)), torch.equal(bits(p[1]), bits(lo))
    print(f"x3_weight_planes {shape[0]} x {shape[1]}: hi bit-equal {same_hi}, lo bit-equal {same_lo} "
          f"(fp16 subnormal lo halves: {int(((lo != 0) & (lo.float().abs() < 2.0 ** -14)).sum())})")
    assert p.shape == (2, *shape) and p.dtype == torch.float16 and torch.isfinite(hi).all() and same_hi and same_lo


# ------------------------------------------------------------------------------------------------ 8. alignment guards
def _refused(call, *dests):
    with pytest.raises(RuntimeError, match="IEF_EALIGN"):
        call()
    torch.cuda.synchronize()
    for d in dests:
        assert bool((d == SENTINEL).all()), "a refused call wrote to its destination"


def test_misaligned_operands_are_refused():
    """an operand that a kernel accesses in 16-byte pieces (8-byte for the fp16 planes) and that starts one element past that
    alignment: IEF_EALIGN from the checks in front of the launch, and the destination keeps its sentinel.  Each entry point below
    has that guard on the lines before its launch (csrc/exact_f32.hip, csrc/split_x3.hip); no other entry point is handed such a
    pointer here"""
    lib = hip.load()
    # ief_conv_out_f32act: x and w
    B, C, H, W, Cout = 1, 64, 4, 4, 4
    x, w, bias = f32(B, H, W, C, seed=1), f32(Cout, 3, 3, C, seed=2), f32(Cout, seed=3)
    out = torch.full((B, Cout, H, W), SENTINEL, device=DEV)
    _refused(lambda: hip.conv_out(one_float_off(x), dev(w), dev(bias), out=out), out)
    _refused(lambda: hip.conv_out(dev(x), one_float_off(w), dev(bias), out=out), out)
    for Co in (8,):         # the kernel without LDS reads the same 16-byte pieces
        w8 = f32(Co, 3, 3, C, seed=4)
        out8 = torch.full((B, Co, H, W), SENTINEL, device=DEV)
        _refused(lambda: hip.conv_out(one_float_off(x), dev(w8), None, out=out8), out8)
        _refused(lambda: hip.conv_out(dev(x), one_float_off(w8), None, out=out8), out8)
    # ief_conv_in_f32act: w and out, both kernels
    for Cin in (4, 3):
        xi, wi = f32(1, Cin, 5, 6, seed=5), f32(3, 3, Cin, 16, seed=6)
        obuf = torch.full((1 * 5 * 6 * 16 + 4,), SENTINEL, device=DEV)
        oal, ooff = obuf[:480].view(1, 5, 6, 16), obuf[1:481].view(1, 5, 6, 16)
        assert ooff.data_ptr() % 16 == 4
        _refused(lambda: hip.conv_in(dev(xi), one_float_off(wi), None, out=oal), obuf)
        _refused(lambda: hip.conv_in(dev(xi), dev(wi), None, out=ooff), obuf)
    # ief_x3_split_weights: w (16 bytes), planes (8 bytes)
    ww = f32(8, 16, seed=7)
    _refused(lambda: hip.x3_weight_planes(one_float_off(ww)))
    wd = dev(ww)
    pbuf = torch.full((2 * 128 + 4,), SENTINEL, dtype=torch.float16, device=DEV)
    woff = one_float_off(ww)
    _refused(lambda: hip._check(lib.ief_x3_split_weights(woff.data_ptr(), pbuf.data_ptr(), 128, 256.0, hip._stream()),
                                "ief_x3_split_weights"), pbuf)
    for halves in (1, 2):   # planes 2 and 4 bytes past 8-byte alignment
        _refused(lambda: hip._check(lib.ief_x3_split_weights(wd.data_ptr(), pbuf[halves:].data_ptr(), 128, 256.0, hip._stream()),
                                    "ief_x3_split_weights"), pbuf)
    # ief_layernorm_x3p: x (ief_layernorm_f32 falls back to its scalar kernel instead: test_layernorm_f32_and_planes_forms)
    xl, gl, bl = f32(9, 640, seed=1), dev(torch.ones(640)), dev(torch.zeros(640))
    _refused(lambda: planes.layernorm(one_float_off(xl), gl, bl))
    # ief_gemm_f32 on the fp32-input MFMA: A and W (16-byte row chunks)
    a, wg = f32(8, 32, seed=8), f32(16, 32, seed=9)
    og = torch.full((8, 16), SENTINEL, device=DEV)
    with hip.f32_contraction("f32"):
        _refused(lambda: hip.gemm(one_float_off(a), dev(wg), out=og), og)
        _refused(lambda: hip.gemm(dev(a), one_float_off(wg), out=og), og)
    # ief_attn_flash_f32 with x3 == 0: q, k, v
    from ctypes import byref
    Bq, heads, N, L, d = 1, 1, 64, 128, 40
    q, k, v = (f32(Bq, n, d, seed=10 + i) for i, n in enumerate((N, L, L)))
    oa = torch.full((Bq, N, d), SENTINEL, device=DEV)
    for which in range(3):
        ts = [one_float_off(t) if i == which else dev(t) for i, t in enumerate((q, k, v))]
        p = hip.IefAttnF32Params()
        p.Q, p.K, p.V, p.Out = ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), oa.data_ptr()
        p.B, p.heads, p.N, p.L, p.d, p.scale = Bq, heads, N, L, d, d ** -0.5
        p.sQb, p.ldq, p.sKb, p.ldk, p.sVb, p.ldv, p.sOb, p.ldo = N * d, d, L * d, d, L * d, d, N * d, d
        p.x3 = 0
        _refused(lambda: hip._check(lib.ief_attn_flash_f32(byref(p), hip._stream()), "ief_attn_flash_f32"), oa)
    print("misaligned operands: conv_out (x, w; both kernels), conv_in (w, out; both kernels), x3_split_weights (w, planes), gemm_f32 "
          "(A, W), attn_flash_f32 (q, k, v) all IEF_EALIGN, destinations untouched")


def test_groupnorm_f32_one_launch_form_falls_back_on_a_misaligned_source():
    """`ief_groupnorm_silu_f32` (the one-launch form: C1 % 4 != 0 keeps it off the row-streaming launches) reads channel PAIRS with
    8-byte accesses; a source 4 bytes past that alignment takes `groupnorm_f32_scalar_kernel` instead: same operator, fp64 bound"""
    B, HW, C, G = 2, 35, 66, 3
    x = f32(B, HW, C, seed=1) * 2 + 0.5
    gamma, beta = 1 + f32(C, seed=2, scale=0.1), f32(C, seed=3, scale=0.1)
    ref = F.silu(F.group_norm(x.double().permute(0, 2, 1), G, gamma.double(), beta.double(), 1e-5)).permute(0, 2, 1)
    e_al = rel_err(hip.groupnorm(dev(x), dev(gamma), dev(beta), G, 1e-5, silu=True), ref)
    e_off = rel_err(hip.groupnorm(one_float_off(x), dev(gamma), dev(beta), G, 1e-5, silu=True), ref)
    print(f"groupnorm fp32 one-launch form C={C}: aligned {e_al:.2e}, source one float off alignment {e_off:.2e}")
    assert e_al < KTOL and e_off < KTOL
