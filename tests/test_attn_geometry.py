"""CPU tests of `hip.attn_geometry`, the one description of an attention launch that every attention wrapper shares (`hip.attn_flash`,
`attn_cross_p2p`, `attn_probs`, `attn_apply`, `attn_bwd`, `cross_bwd`, `cross_map_grad`, `planes.attn_flash`), and of the host
predicates that say which kernel takes a layer.  Shapes and flags only, so nothing here needs a device.  Every expected value
below is written out by hand from the definitions:

    q [Bq, N, C], k [Bk, L, C], v [Bv, L, C], C = heads d
    B   = `batch` if given, else Bq                                     (the launch's batch rows)
    an operand without a batch-row list has exactly B batch rows; one with a list may have any number
    out [B, N, C], lse [B, heads, N]                                    (counted in the launch's rows)
    do, o [Bq, N, C]                                                    (q's shape)

    cross_p2p_x3_ok(d, L)      = d in {40, 64, 80, 160} and L <= 96
    x3_fused_bwd_ok(d, L)      = the f16x3 contraction, IEF_X3_FUSED_BWD and IEF_FLASH_F32 on, d in {40, 64}, L >= 128
    cross_map_grad_ok(d, L, t) = t is fp32, d in {32, 40, 64, 80, 160}, 1 <= L <= IEF_CROSS_MAP_GRAD_MAX_L (106)
    cross_bwd_ok(d, L, t)      = t is fp32, d in {32, 40, 64, 80},      1 <= L <= IEF_CROSS_BWD_MAX_L (80)
"""
import pytest
import torch

from ief_amd import hip


def test_self_attention():
    g = hip.attn_geometry((2, 64, 80), (2, 64, 80), (2, 64, 80), 2)
    assert (g.B, g.N, g.L, g.C, g.d) == (2, 64, 64, 80, 40)
    assert tuple(g) == (2, 64, 64, 80, 40)


def test_cross_attention_77_keys_with_every_optional_operand():
    s = (2, 4096, 320)
    g = hip.attn_geometry(s, (2, 77, 320), (2, 77, 320), 8, out=s, do=s, o=s, lse=(2, 8, 4096))
    assert (g.B, g.N, g.L, g.C, g.d) == (2, 4096, 77, 320, 40)


def test_q_of_half_the_batch_under_q_src():
    """the shared prefix of a CFG step: q projected once at Bp = 2 rows, the launch and k / v at 2 Bp = 4"""
    g = hip.attn_geometry((2, 256, 640), (4, 77, 640), (4, 77, 640), 8, out=(4, 256, 640), q_src=True, batch=4)
    assert (g.B, g.N, g.L, g.C, g.d) == (4, 256, 77, 640, 80)
    with pytest.raises(ValueError):                             # the same launch without the list
        hip.attn_geometry((2, 256, 640), (4, 77, 640), (4, 77, 640), 8, batch=4)
    with pytest.raises(ValueError):                             # the list does not excuse k
        hip.attn_geometry((2, 256, 640), (2, 77, 640), (4, 77, 640), 8, q_src=True, batch=4)


def test_destination_of_other_batch_rows_under_all_three_lists():
    """a mask-guided MasaCtrl launch: a destination of Bo = 2 rows (the targets) over operands of 4"""
    s = (4, 1024, 80)
    g = hip.attn_geometry(s, s, s, 2, out=(2, 1024, 80), q_src=True, k_src=True, v_src=True, batch=2)
    assert (g.B, g.N, g.L, g.C, g.d) == (2, 1024, 1024, 80, 40)
    for missing in ("q_src", "k_src", "v_src"):
        flags = dict(q_src=True, k_src=True, v_src=True)
        flags[missing] = False
        with pytest.raises(ValueError, match=missing):
            hip.attn_geometry(s, s, s, 2, out=(2, 1024, 80), batch=2, **flags)


Q = (1, 32, 80)


@pytest.mark.parametrize("k, v, heads, kw", [
    (Q, (1, 31, 80), 2, {}),                                    # v one row short
    ((1, 32, 88), Q, 2, {}),                                    # k with another C
    (Q, (1, 32, 88), 2, {}),                                    # v with another C
    (Q, Q, 3, {}),                                              # C = 80 is not a multiple of 3 heads
    (Q, Q, 0, {}),                                              # no heads
    ((32, 80), Q, 2, {}),                                       # a 2-D operand
    (Q, (1, 1, 32, 80), 2, {}),                                 # a 4-D operand
    (Q, Q, 2, dict(out=(1, 31, 80))),                           # out of another N
    (Q, Q, 2, dict(out=(1, 32, 40))),                           # ... another C
    (Q, Q, 2, dict(out=(2, 32, 80))),                           # ... another batch
    (Q, Q, 2, dict(out=(32, 80))),                              # ... 2-D
    (Q, Q, 2, dict(do=(1, 31, 80))),                            # do one row short
    (Q, Q, 2, dict(o=(1, 32, 88))),                             # o with another C
    (Q, Q, 2, dict(lse=(1, 32, 2))),                            # lse [B, N, heads]
    (Q, Q, 2, dict(lse=(2, 32))),                               # lse 2-D
    (Q, Q, 2, dict(lse=(2, 2, 32))),                            # lse of another batch
    ((2, 32, 80), (2, 32, 80), 2, {}),                          # batch mismatch without a list
    (Q, (2, 32, 80), 2, {}),                                    # ... of v alone
    ((1, 0, 80), (1, 0, 80), 2, {}),                            # no keys
])
def test_mismatch_raises(k, v, heads, kw):
    with pytest.raises(ValueError):
        hip.attn_geometry(Q, k, v, heads, **kw)


def test_no_queries_raises():
    with pytest.raises(ValueError):
        hip.attn_geometry((1, 0, 80), Q, Q, 2)


def test_head_dims_without_a_kernel_are_not_this_functions_business():
    """d = 48 has no kernel anywhere: the predicates say so and the library answers IEF_ESHAPE; the geometry is still one"""
    g = hip.attn_geometry((1, 64, 96), (1, 77, 96), (1, 77, 96), 2)
    assert g.d == 48


def test_message_prefix_is_the_callers():
    with pytest.raises(ValueError, match=r"^planes\.attn_flash: v "):
        hip.attn_geometry(Q, Q, (1, 31, 80), 2, who="planes.attn_flash")
    with pytest.raises(ValueError, match=r"^attn_flash: v "):
        hip.attn_geometry(Q, Q, (1, 31, 80), 2)


def test_cross_p2p_x3_ok_edges():
    for d in (40, 64, 80, 160):
        assert hip.cross_p2p_x3_ok(d, 96) is True and hip.cross_p2p_x3_ok(d, 77) is True
        assert hip.cross_p2p_x3_ok(d, 97) is False
    for d in (32, 48, 96, 128, 320):
        assert hip.cross_p2p_x3_ok(d, 77) is False


def test_x3_fused_bwd_ok_edges(monkeypatch):
    monkeypatch.setattr(hip, "X3_FUSED_BWD", True)
    monkeypatch.setattr(hip, "FLASH_F32", True)
    assert not hip.x3_fused_bwd_ok(40, 4096)                    # the f32 contraction is the default
    with hip.f32_contraction("x3"):
        assert hip.x3_fused_bwd_ok(40, 128) and hip.x3_fused_bwd_ok(64, 128) and hip.x3_fused_bwd_ok(40, 4096)
        assert not hip.x3_fused_bwd_ok(40, 127) and not hip.x3_fused_bwd_ok(64, 77)
        assert not hip.x3_fused_bwd_ok(32, 128) and not hip.x3_fused_bwd_ok(80, 128) and not hip.x3_fused_bwd_ok(160, 128)
        monkeypatch.setattr(hip, "FLASH_F32", False)
        assert not hip.x3_fused_bwd_ok(40, 128)
        monkeypatch.setattr(hip, "FLASH_F32", True)
        monkeypatch.setattr(hip, "X3_FUSED_BWD", False)
        assert not hip.x3_fused_bwd_ok(40, 128)
    with hip.f32_contraction("f32"):
        monkeypatch.setattr(hip, "X3_FUSED_BWD", True)
        assert not hip.x3_fused_bwd_ok(40, 128)


def test_cross_map_grad_ok_edges():
    assert hip.CROSS_MAP_GRAD_MAX_L == 106
    for d in (32, 40, 64, 80, 160):
        assert hip.cross_map_grad_ok(d, 1) and hip.cross_map_grad_ok(d, 77) and hip.cross_map_grad_ok(d, 106)
        assert not hip.cross_map_grad_ok(d, 0) and not hip.cross_map_grad_ok(d, 107)
        assert not hip.cross_map_grad_ok(d, 77, torch.float16)
    for d in (16, 48, 96, 128, 320):
        assert not hip.cross_map_grad_ok(d, 77)


def test_cross_bwd_ok_edges():
    assert hip.CROSS_BWD_MAX_L == 80
    for d in (32, 40, 64, 80):
        assert hip.cross_bwd_ok(d, 1) and hip.cross_bwd_ok(d, 77) and hip.cross_bwd_ok(d, 80)
        assert not hip.cross_bwd_ok(d, 0) and not hip.cross_bwd_ok(d, 81)
        assert not hip.cross_bwd_ok(d, 77, torch.float16)
    for d in (16, 48, 96, 160, 320):                            # 160: the kernel takes it, the route does not
        assert not hip.cross_bwd_ok(d, 77)
