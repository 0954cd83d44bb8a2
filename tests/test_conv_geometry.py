"""CPU tests of `hip.conv_geometry`: the one description of a 3x3 convolution's geometry that `hip.conv3x3` (fp16 and fp32
storage) and `planes.conv3x3` share.  It takes shapes and flags only, so nothing here needs a device.  Every expected value
below is written out by hand from the definitions:

    (H, Wd)  = (2 Hp, 2 Wp) under `upsample`, else (Hp, Wp)
    Ho, Wo   = (H + pad - 3) // stride + 1, (Wd + pad - 3) // stride + 1      with pad = 1 under `pad_hi_only`, else 2
    M, K     = B Ho Wo, 9 (C1 + C2) + CE1 + CE2
    rows_per_batch = Ho Wo for a rowvec [B, Cout] with B > 1, else B Ho Wo
    halo_geom  = stride 1, no pad_hi_only, no extra, Hp >= 2, and 2 <= Wd <= 64 (plain) or
                 Wd <= 128, H Wd a multiple of 256, Wd a divisor of 256 (upsample)
    phase_geom = upsample, stride 1, no pad_hi_only, no extra, Hp >= 2, 2 <= Wp <= 64
"""
import pytest

from ief_amd import hip

W320 = (320, 3, 3, 320)


def test_plain_3x3():
    g = hip.conv_geometry((4, 64, 64, 320), W320)
    assert (g.B, g.Hp, g.Wp, g.C1, g.C2, g.CE1, g.CE2, g.Cout) == (4, 64, 64, 320, 0, 0, 0, 320)
    assert (g.H, g.Wd, g.Ho, g.Wo) == (64, 64, 64, 64)
    assert (g.M, g.K) == (16384, 2880)
    assert g.rows_per_batch == 0
    assert g.halo_geom is True and g.phase_geom is False


def test_stride_2():
    g = hip.conv_geometry((4, 64, 64, 320), W320, stride=2)
    assert (g.Ho, g.Wo, g.M) == (32, 32, 4096)              # (64 + 2 - 3) // 2 + 1
    assert g.halo_geom is False and g.phase_geom is False


def test_stride_2_pad_hi_only():
    g = hip.conv_geometry((4, 64, 64, 320), W320, stride=2, pad_hi_only=True)
    assert (g.Ho, g.Wo, g.M) == (32, 32, 4096)              # (64 + 1 - 3) // 2 + 1
    assert g.halo_geom is False and g.phase_geom is False
    g = hip.conv_geometry((1, 9, 7, 320), W320, stride=2, pad_hi_only=True)
    assert (g.Ho, g.Wo) == (4, 3)                           # (9 + 1 - 3) // 2 + 1, (7 + 1 - 3) // 2 + 1


def test_upsample():
    g = hip.conv_geometry((2, 32, 32, 320), W320, upsample=True)
    assert (g.Hp, g.Wp, g.H, g.Wd, g.Ho, g.Wo) == (32, 32, 64, 64, 64, 64)
    assert (g.M, g.K) == (8192, 2880)
    assert g.halo_geom is True and g.phase_geom is True


def test_upsample_rows_too_wide():
    g = hip.conv_geometry((1, 2, 65, 320), W320, upsample=True)
    assert (g.H, g.Wd, g.Ho, g.Wo, g.M) == (4, 130, 4, 130, 520)
    assert g.halo_geom is False and g.phase_geom is False


def test_upsample_rows_that_do_not_tile_256_pixels():
    g = hip.conv_geometry((1, 6, 6, 320), W320, upsample=True)              # 12 x 12 output: 144 % 256 != 0, 256 % 12 != 0
    assert (g.Ho, g.Wo) == (12, 12)
    assert g.halo_geom is False and g.phase_geom is True                    # the phase form's limits are those of the 6-pixel source rows
    g = hip.conv_geometry((1, 64, 64, 320), W320, upsample=True)            # rows of 128: 128 * 128 % 256 == 0, 256 % 128 == 0
    assert g.Wd == 128 and g.halo_geom is True and g.phase_geom is True
    g = hip.conv_geometry((1, 96, 96, 320), W320, upsample=True)            # rows of 192 > 128, source rows of 96 > 64
    assert g.halo_geom is False and g.phase_geom is False


def test_plain_width_limits():
    assert hip.conv_geometry((1, 8, 128, 320), W320).halo_geom is False
    assert hip.conv_geometry((1, 8, 65, 320), W320).halo_geom is False
    assert hip.conv_geometry((1, 8, 64, 320), W320).halo_geom is True
    assert hip.conv_geometry((1, 8, 2, 320), W320).halo_geom is True
    assert hip.conv_geometry((1, 8, 1, 320), W320).halo_geom is False


def test_plain_one_row():
    g = hip.conv_geometry((2, 1, 16, 320), W320)
    assert (g.Ho, g.Wo, g.M) == (1, 16, 32)
    assert g.halo_geom is False


def test_concat():
    g = hip.conv_geometry((2, 32, 32, 640), (640, 3, 3, 960), x2=(2, 32, 32, 320))
    assert (g.C1, g.C2, g.Cout) == (640, 320, 640)
    assert (g.M, g.K) == (2048, 8640)                       # 9 * (640 + 320)
    assert g.halo_geom is True


def test_fused_shortcut():
    g = hip.conv_geometry((2, 16, 16, 640), (640, 5760 + 320 + 640), extra=((2, 16, 16, 320), (2, 16, 16, 640)))
    assert (g.CE1, g.CE2, g.K) == (320, 640, 6720)          # 9 * 640 + 320 + 640
    assert g.halo_geom is False and g.phase_geom is False
    g = hip.conv_geometry((2, 16, 16, 640), (640, 8640 + 64), x2=(2, 16, 16, 320), extra=((2, 16, 16, 64), None))
    assert (g.C2, g.CE1, g.CE2, g.K) == (320, 64, 0, 8704)  # 9 * (640 + 320) + 64


def test_rowvec_rows_per_batch():
    x = (4, 64, 64, 320)
    assert hip.conv_geometry(x, W320, rowvec=(4, 320)).rows_per_batch == 4096               # Ho Wo
    assert hip.conv_geometry(x, W320, rowvec=(1, 320)).rows_per_batch == 16384              # B Ho Wo
    assert hip.conv_geometry((1, 64, 64, 320), W320, rowvec=(1, 320)).rows_per_batch == 4096
    assert hip.conv_geometry(x, W320, rowvec=(4, 320), stride=2).rows_per_batch == 1024     # of the OUTPUT: 32 * 32


def test_residual_at_the_output_resolution():
    g = hip.conv_geometry((4, 64, 64, 320), W320, stride=2, residual=(4, 32, 32, 320))
    assert (g.Ho, g.Wo) == (32, 32)


@pytest.mark.parametrize("kw", [
    dict(x2=(1, 4, 5, 32)),                                                 # x2 with another W
    dict(x2=(1, 5, 4, 32)),                                                 # ... another H
    dict(x2=(2, 4, 4, 32)),                                                 # ... another batch
])
def test_x2_mismatch_raises(kw):
    with pytest.raises(ValueError):
        hip.conv_geometry((1, 4, 4, 32), (64, 3, 3, 64), **kw)


@pytest.mark.parametrize("extra", [((1, 4, 5, 64), None), ((1, 5, 4, 64), None), ((1, 4, 4, 64), (1, 4, 5, 64)),
                                   ((1, 4, 4, 64), (1, 3, 4, 64))])
def test_extra_mismatch_raises(extra):
    K = 9 * 32 + 64 + (64 if extra[1] is not None else 0)
    with pytest.raises(ValueError):
        hip.conv_geometry((1, 4, 4, 32), (64, K), extra=extra)


def test_rowvec_mismatch_raises():
    with pytest.raises(ValueError):
        hip.conv_geometry((4, 8, 8, 320), W320, rowvec=(2, 320))
    with pytest.raises(ValueError):
        hip.conv_geometry((4, 8, 8, 320), W320, rowvec=(4, 160))
    with pytest.raises(ValueError):
        hip.conv_geometry((4, 8, 8, 320), W320, rowvec=(320,))


@pytest.mark.parametrize("residual", [(4, 8, 8, 160), (4, 8, 9, 320), (2, 8, 8, 320), (256, 320)])
def test_residual_mismatch_raises(residual):
    with pytest.raises(ValueError):
        hip.conv_geometry((4, 8, 8, 320), W320, residual=residual)


def test_residual_of_the_input_resolution_raises_under_stride_2():
    with pytest.raises(ValueError):
        hip.conv_geometry((4, 8, 8, 320), W320, stride=2, residual=(4, 8, 8, 320))


def test_weight_mismatch_raises():
    with pytest.raises(ValueError):
        hip.conv_geometry((1, 4, 4, 32), (64, 3, 3, 64), x2=(1, 4, 4, 64))      # last dim 64 != C1 + C2 = 96
    with pytest.raises(ValueError):
        hip.conv_geometry((1, 4, 4, 32), (64, 3, 3, 64))                        # last dim 64 != C1 = 32
    with pytest.raises(ValueError):
        hip.conv_geometry((1, 4, 4, 32), (64, 288))                             # a fused 2-D weight without extra sources
    with pytest.raises(ValueError):
        hip.conv_geometry((1, 4, 4, 32), (64, 3, 3, 32), extra=((1, 4, 4, 64), None))   # extra sources need the fused [Cout, K]
    with pytest.raises(ValueError):
        hip.conv_geometry((1, 4, 4, 32), (64, 288), extra=((1, 4, 4, 64), None))        # K = 288 + 64


def test_message_prefix_is_the_callers():
    with pytest.raises(ValueError, match=r"^planes\.conv3x3: x2 "):
        hip.conv_geometry((1, 4, 4, 32), (64, 3, 3, 64), x2=(1, 4, 5, 32), who="planes.conv3x3")
    with pytest.raises(ValueError, match=r"^conv3x3: x2 "):
        hip.conv_geometry((1, 4, 4, 32), (64, 3, 3, 64), x2=(1, 4, 5, 32))
