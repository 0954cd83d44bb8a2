"""Q batch-row indirection of the fused split-operand cross-attention (`attn_cross_p2p_x3_kernel<D, true>`, csrc/cross_p2p_x3.hip)
on a real MI355X: a launch over B batch rows of K / V whose queries come from FEWER batch rows of Q -- the CFG step whose two
halves share one query projection.

Stated tolerances (every test prints what it measured):
    q_src = [0, 1, 0, 1] over a 2-row Q vs the same launch fed the repeated 4-row Q      bit for bit (the same arithmetic on the same
                                                                                         numbers: only the address of a Q row differs)
    either vs fp64 on the host                                                           <= 4e-6 of max |reference| -- the bound
                                                                                         tests/test_gpu_x3p_keysplit.py holds the planes
                                                                                         kernels to
Shapes: B = 4, 2 heads, 160 queries (one whole and one partial 128-query block), 77 keys, every head dim the kernel has; the edit off
and on (row 3 edited from row 2, so the SOURCE row's maps go through q_src too).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip  # noqa: E402

XTOL = 4e-6
DEV = torch.device("cuda:0")
B, HEADS, N, L = 4, 2, 160, 77


def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(autouse=True)
def _x3():
    with hip.f32_contraction("x3"):
        yield


def _case(d):
    """operands, the edit tables of tests/test_gpu_x3.py::test_cross_attention_p2p_edit_fused_x3 (one slot), fp64 results with the
    edit off and on -- computed once per head dim"""
    C = HEADS * d
    q2, k, v = f32(2, N, C, seed=1), f32(B, L, C, seed=2, scale=1.5), f32(B, L, C, seed=3)
    q4 = torch.cat([q2, q2])
    g = torch.Generator().manual_seed(0)
    mapper = torch.randint(-1, L, (L,), generator=g)
    a = (mapper != -1).float()
    M = torch.zeros(L, L)
    M[mapper % L, torch.arange(L)] = 1.0
    M[5, 5], M[5, 6] = 1.0 / 3.0, 2.0 / 3.0
    gate = (torch.rand(L, generator=g) > 0.3).float() * (0.25 + 0.75 * torch.rand(L, generator=g))
    c1, c2 = gate * a, 1 - gate * a
    mt, coef = torch.zeros(1, 96, 96), torch.zeros(1, 2, 96)
    mt[0, :L, :L] = M.t()
    coef[0, 0, :L], coef[0, 1, :L] = c1, c2
    es, sl = torch.tensor([-1, -1, -1, 2], dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    qh = q4.double().reshape(B, N, HEADS, d).permute(0, 2, 1, 3)
    kh = k.double().reshape(B, L, HEADS, d).permute(0, 2, 1, 3)
    vh = v.double().reshape(B, L, HEADS, d).permute(0, 2, 1, 3)
    P = torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, -1)
    Pe = P.clone()
    Pe[3] = c1.double() * (P[2] @ M.double()) + c2.double() * P[3]
    back = lambda X: (X @ vh).permute(0, 2, 1, 3).reshape(B, N, C)
    return dict(q2=q2.cuda(), q4=q4.cuda(), k=k.cuda(), v=v.cuda(), edit=(es.cuda(), sl.cuda(), mt.cuda(), coef.cuda()),
                ref_off=back(P), ref_on=back(Pe))


_cases = {}


@pytest.mark.parametrize("edit", [False, True])
@pytest.mark.parametrize("d", [40, 64, 80, 160])
def test_q_src_is_the_repeated_q_and_within_fp64_bound(d, edit):
    c = _cases.get(d) or _cases.setdefault(d, _case(d))
    rows = hip.BatchRows([0, 1, 0, 1], 2, DEV)
    args = c["edit"] if edit else (None, None, None, None)
    ref = c["ref_on"] if edit else c["ref_off"]
    # the kernel itself, edited or not (hip.attn_cross_p2p hands the unedited layer to the flash kernel)
    hip.profile_begin()
    got = hip._attn_cross_p2p_x3(c["q2"], c["k"], c["v"], HEADS, d ** -0.5, *args, q_src=rows)
    rep = hip._attn_cross_p2p_x3(c["q4"], c["k"], c["v"], HEADS, d ** -0.5, *args)
    names = [n for n, _, _ in hip.profile_end()]
    assert names == [f"attn_cross_p2p_x3_kernel<{d}>"] * 2, names
    e, er = rel_err(got, ref), rel_err(rep, ref)
    print(f"cross q_src d={d} edit={'on' if edit else 'off'}: {e:.2e} vs fp64 (repeated Q {er:.2e}); bit-equal: {torch.equal(got, rep)}")
    assert got.shape == (B, N, HEADS * d)
    assert torch.equal(got, rep), "q_src over the 2-row Q must equal the launch fed the repeated 4-row Q bit for bit"
    assert e <= XTOL and er <= XTOL
    # operand planes out: the split of the same fp32 numbers
    gp = hip._attn_cross_p2p_x3(c["q2"], c["k"], c["v"], HEADS, d ** -0.5, *args, q_src=rows, out_planes=True)
    assert torch.equal(gp.hi, got.half()) and torch.equal(gp.lo, (got - got.half().float()).half())
    # the public entry: same numbers edited; unedited it is the flash kernel with its own q_src, within the same bound
    pub = hip.attn_cross_p2p(c["q2"], c["k"], c["v"], HEADS, d ** -0.5, *args, q_src=rows)
    assert rel_err(pub, ref) <= XTOL and (not edit or torch.equal(pub, got))


def test_q_src_is_checked_on_the_host():
    c = _cases.get(40) or _cases.setdefault(40, _case(40))
    with pytest.raises(ValueError, match="every entry must be a row"):
        hip.BatchRows([0, 1, 2, 1], 2, DEV)
    with pytest.raises(ValueError, match="every entry must be a row"):
        hip.BatchRows([0, -1, 0, 1], 2, DEV)
    with pytest.raises(ValueError, match="BatchRows"):          # a bare device list is not accepted: nobody checked it
        hip.attn_cross_p2p(c["q2"], c["k"], c["v"], HEADS, 40 ** -0.5, q_src=torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="BatchRows"):          # checked against 3 rows, used with a 2-row Q
        hip.attn_cross_p2p(c["q2"], c["k"], c["v"], HEADS, 40 ** -0.5, q_src=hip.BatchRows([0, 1, 2, 1], 3, DEV))
    with pytest.raises(ValueError, match="BatchRows"):          # one entry per batch row of k / v
        hip.attn_cross_p2p(c["q2"], c["k"], c["v"], HEADS, 40 ** -0.5, q_src=hip.BatchRows([0, 1], 2, DEV))
