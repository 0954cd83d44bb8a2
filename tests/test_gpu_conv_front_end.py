"""The three convolution entry points refuse a skip tensor of another spatial shape BEFORE anything is launched: the library only
sees pointers, so on the device a mis-shaped `x2` would be an out-of-bounds read instead of an error (`hip.conv_geometry`)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ief_amd import hip, planes  # noqa: E402

SENTINEL = -7.0


def test_conv3x3_refuses_a_misshaped_x2_in_every_mode():
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(1, 4, 4, 32, generator=gen).cuda()
    x2 = torch.randn(1, 4, 5, 32, generator=gen).cuda()
    w = (torch.randn(64, 3, 3, 64, generator=gen) / 24).cuda()                  # K = 9 * (32 + 32)
    for dtype in (torch.float16, torch.float32):
        out = torch.full((1, 4, 4, 64), SENTINEL, dtype=dtype, device="cuda")
        with pytest.raises(ValueError):
            hip.conv3x3(x.to(dtype), w.to(dtype), x2=x2.to(dtype), out=out)
        torch.cuda.synchronize()
        assert (out == SENTINEL).all(), f"hip.conv3x3 ({dtype}) wrote its output"
    out = torch.full((1, 4, 4, 64), SENTINEL, dtype=torch.float32, device="cuda")
    op = planes.Planes(torch.full((2, 1, 4, 4, 64), SENTINEL, dtype=torch.float16, device="cuda"))
    with hip.f32_contraction("x3"):
        xp, x2p = planes.split(x), planes.split(x2)
        with pytest.raises(ValueError):
            planes.conv3x3(xp, w, x2=x2p, out=out, out_planes=op)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (op.t == SENTINEL).all(), "planes.conv3x3 wrote its output"
