"""Every attention entry point refuses a `v` (the backward: a `do`) that is one row short, and a `k` of other channels, BEFORE
anything is launched: the library only sees pointers and leading dimensions, so on the device such an operand would be an
out-of-bounds read instead of an error (`hip.attn_geometry`).  Nothing here reaches a kernel: every case ends on the host, and the
caller's buffers still hold their sentinel afterwards."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ief_amd import hip, planes  # noqa: E402

SENTINEL = -7.0
B, HEADS, N, L, D = 1, 2, 32, 32, 40
C = HEADS * D
LX = 8                                  # keys of the cross_bwd / cross_map_grad cases
SCALE = D ** -0.5


def _t(rows, c=C, dtype=torch.float32, seed=0):
    return torch.randn(B, rows, c, generator=torch.Generator().manual_seed(seed + rows + c)).to("cuda", dtype)


def _buf(rows, c=C, dtype=torch.float32):
    return torch.full((B, rows, c), SENTINEL, dtype=dtype, device="cuda")


def _refused(call, *bufs):
    with pytest.raises(ValueError):
        call()
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == SENTINEL).all()), "a refused call wrote its output"


def _bad_kv(dtype, rows=L):
    """(k, v) pairs of a forward: v one row short, k with C + 8 channels"""
    return (_t(rows, dtype=dtype, seed=1), _t(rows - 1, dtype=dtype, seed=2)), (_t(rows, C + 8, dtype, seed=1), _t(rows, dtype=dtype, seed=2))


@pytest.mark.parametrize("mode", ["f16", "f32", "x3"])
def test_attn_flash(mode):
    dtype = torch.float16 if mode == "f16" else torch.float32
    out = _buf(N, dtype=dtype)
    with hip.f32_contraction("x3" if mode == "x3" else "f32"):
        for k, v in _bad_kv(dtype):
            _refused(lambda: hip.attn_flash(_t(N, dtype=dtype), k, v, HEADS, SCALE, out=out), out)


def test_planes_attn_flash():
    out = _buf(N)
    with hip.f32_contraction("x3"):
        q = planes.split(_t(N))
        for k, v in _bad_kv(torch.float32):
            kp, vp = planes.split(k), planes.split(v)
            _refused(lambda: planes.attn_flash(q, kp, vp, HEADS, SCALE, out=out, out_planes=False), out)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_attn_cross_p2p(dtype):
    out = _buf(N, dtype=dtype)
    for k, v in _bad_kv(dtype):
        _refused(lambda: hip.attn_cross_p2p(_t(N, dtype=dtype), k, v, HEADS, SCALE, out=out), out)


def test_attn_apply():
    probs = torch.softmax(torch.randn(B * HEADS, N, L, generator=torch.Generator().manual_seed(3)), -1).to("cuda", torch.float16)
    out = _buf(N, dtype=torch.float16)
    _refused(lambda: hip.attn_apply(probs, _t(L - 1, dtype=torch.float16), HEADS, out=out), out)
    _refused(lambda: hip.attn_apply(probs, _t(L, C + 8, torch.float16), HEADS, out=out), out)       # v is all there is: its channels


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("want_dkv", [True, False])
def test_attn_bwd(dtype, want_dkv):
    """fp32, want_dkv: the `cross_bwd` route; fp32 without: the materialised maps"""
    q, k, v, o = (_t(r, dtype=dtype, seed=s) for r, s in ((N, 0), (L, 1), (L, 2), (N, 3)))
    lse = torch.zeros(B, HEADS, N, device="cuda")
    dq, dk, dv = _buf(N, dtype=dtype), _buf(L, dtype=dtype), _buf(L, dtype=dtype)
    _refused(lambda: hip.attn_bwd(q, k, v, o, _t(N - 1, dtype=dtype, seed=4), lse, HEADS, SCALE, dq=dq, dk=dk, dv=dv,
                                  want_dkv=want_dkv), dq, dk, dv)


def test_cross_bwd():
    q, k, v = _t(N), _t(LX, seed=1), _t(LX, seed=2)
    dq, dk, dv = _buf(N), _buf(LX), _buf(LX)
    _refused(lambda: hip.cross_bwd(q, k, v, _t(N - 1, seed=4), HEADS, SCALE, dq=dq, dk=dk, dv=dv), dq, dk, dv)


def test_cross_map_grad():
    q, k, v = _t(N), _t(LX, seed=1), _t(LX, seed=2)
    ref = torch.softmax(torch.randn(B * HEADS, N, LX, generator=torch.Generator().manual_seed(5)), -1).cuda()
    dq = _buf(N)
    _refused(lambda: hip.cross_map_grad(q, k, v, _t(N - 1, seed=4), ref, HEADS, SCALE, 1.0, dq=dq), dq)
