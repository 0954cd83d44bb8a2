"""The batch-repeat launch (`ief_repeat_batch`, csrc/elementwise.hip) and `conv_in` writing its own operand planes
(`ief_conv_in_f32act_planes`, csrc/exact_f32.hip) on a real MI355X -- the two glue launches of the CFG step's shared prefix.
Everything here is bit for bit: a copy, and a split defined as two round-to-nearest conversions."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip, planes  # noqa: E402

DEV = torch.device("cuda:0")


def f32(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_four_jobs_of_unequal_sizes_in_one_launch():
    """sizes: one 16-byte chunk per row block; a block that is no multiple of the 256-thread workgroup; operand planes (two
    blocks per job, the destination's plane stride twice the source's); a job larger than one pass of the capped grid
    (2048 workgroups x 256 threads x 16 bytes = 8 MiB)"""
    a = f32(2, 4, seed=1).cuda()                                  # 32 bytes: one chunk per batch row... two per block
    b = f32(2, 33, 20, seed=2).cuda().half()                      # fp16, 2640 bytes: 165 chunks
    c = planes.split(f32(2, 7, 5, 8, seed=3).cuda())              # Planes [2][2, 7, 5, 8]
    d = f32(3, 1024, 1030, seed=4).cuda()                         # 12.07 MiB: second trip of the grid-stride loop; Bp = 3
    hip.profile_begin()
    ra, rb, rc, rd = hip.repeat_batch(a, b, c, d)
    names = [n for n, _, _ in hip.profile_end()]
    assert names == ["repeat_batch_kernel"], names
    assert torch.equal(ra, torch.cat([a, a])) and torch.equal(rb, torch.cat([b, b])) and torch.equal(rd, torch.cat([d, d]))
    assert isinstance(rc, planes.Planes) and tuple(rc.shape) == (4, 7, 5, 8)
    assert torch.equal(rc.hi, torch.cat([c.hi, c.hi])) and torch.equal(rc.lo, torch.cat([c.lo, c.lo]))
    one = hip.repeat_batch(b)
    assert torch.equal(one, rb)
    with pytest.raises(ValueError):
        hip.repeat_batch(a, a, a, a, a)


def test_misaligned_operands_are_refused_without_a_launch():
    lib = hip.load()
    src = f32(64, seed=5).cuda()
    dst = torch.full((129,), float("nan"), device=DEV)

    def call(s, d, nbytes, blocks=1, n=1):
        jobs = (hip.IefRepeatJob * 1)()
        jobs[0].src, jobs[0].dst, jobs[0].bytes, jobs[0].blocks = s, d, nbytes, blocks
        return lib.ief_repeat_batch(jobs, n, hip._stream())

    assert call(src.data_ptr() + 4, dst.data_ptr(), 64) == -3, "source off the 16-byte grid: IEF_EALIGN"
    assert call(src.data_ptr(), dst.data_ptr() + 4, 64) == -3, "destination off the 16-byte grid: IEF_EALIGN"
    assert call(src.data_ptr(), dst.data_ptr(), 72) == -3, "a block that is no multiple of 16 bytes: IEF_EALIGN"
    assert call(None, dst.data_ptr(), 64) == -1 and call(src.data_ptr(), dst.data_ptr(), 64, n=5) == -2 and call(src.data_ptr(), dst.data_ptr(), 0) == -2
    with pytest.raises(RuntimeError, match="IEF_EALIGN"):
        hip.repeat_batch(f32(2, 3, seed=6).cuda())                # 12-byte row blocks
    torch.cuda.synchronize()
    assert torch.isnan(dst).all(), "a refused call must not launch"
    assert call(src.data_ptr(), dst.data_ptr(), 256) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst[:128], torch.cat([src, src])) and torch.isnan(dst[128])


@pytest.mark.parametrize("B,Cin,H,W,Cout", [(1, 4, 8, 8, 320), (2, 4, 16, 16, 320), (1, 3, 8, 8, 64)])
def test_conv_in_writes_its_planes(B, Cin, H, W, Cout):
    """fp32 output: the bits of the entry point without planes (same kernel body, same accumulation order); planes: the split of it,
    bit for bit what the standalone splitter makes.  Cin = 4 takes conv_in_f32_kernel<4>, Cin = 3 the generic kernel."""
    x = f32(B, Cin, H, W, seed=7).cuda()
    w = (f32(3, 3, Cin, Cout, seed=8) * 0.2).cuda()
    bias = f32(Cout, seed=9).cuda()
    with hip.f32_contraction("x3"):
        plain = hip.conv_in(x, w, bias)
        hip.profile_begin()
        out, op = hip.conv_in(x, w, bias, out_planes=True)
        names = [n for n, _, _ in hip.profile_end()]
        ref = planes.split(plain)
    assert names == ["conv_in_f32_kernel<planes>"], names
    assert torch.equal(out, plain), "the fp32 result must keep its bits"
    assert torch.equal(op.t, ref.t), "planes == planes.split of the fp32 result"
    assert torch.equal(op.hi, plain.half()) and torch.equal(op.lo, (plain - plain.half().float()).half())
    lib = hip.load()
    bad = lib.ief_conv_in_f32act_planes(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), op.t.data_ptr() + 2, op.plane,
                                        B, Cin, H, W, Cout, hip._stream())
    assert bad == -3, "planes off the 8-byte grid: IEF_EALIGN"
