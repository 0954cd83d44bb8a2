"""Mask-guided MasaCtrl (`MutualSelfAttentionControlMask`) on the host: the editor's Python against an fp64 restatement of
`/root/reference/masactrl/model/attention_control.py:134-189`, the plan's row lists, the lowering's refusals and the
parameter block's size.  No GPU.

Stated tolerance: the fp32 editor vs the fp64 restatement <= 1e-5 absolute (outputs are convex combinations of unit-scale
Gaussian values; fp32 rounding of 64-term softmaxes and sums is some 1e-7 per term) -- the test prints what it measured.
"""
import types

import pytest
import torch
import torch.nn.functional as F

import ief_amd  # noqa: F401
from ief_amd import hip
from ief_amd.control import ControlPlan
from ief_amd.masactrl.model.attention_base import AttentionBase
from ief_amd.masactrl.model.attention_control import MutualSelfAttentionControlMask
from ief_amd.masactrl.model.register import lower_editor


def _masks(h=16, seed=0):
    """two different binary [h, h] masks with both classes present at every resolution down to 8 x 8"""
    ms, mt = torch.zeros(h, h), torch.zeros(h, h)
    ms[h // 4: 3 * h // 4, h // 8: h // 2] = 1
    mt[h // 8: h // 2, h // 4: 7 * h // 8] = 1
    return ms, mt


def _ref64(q, k, v, heads, scale, ms, mt):
    """reference lines 134-189 in fp64: additive finfo.min on the scores, two softmaxes, blend by mask_t"""
    q, k, v = q.double(), k.double(), v.double()
    n, d = q.shape[1], q.shape[2]
    H = int(n ** 0.5)
    m_s = F.interpolate(ms[None, None].double(), (H, H)).flatten()
    m_t = F.interpolate(mt[None, None].double(), (H, H)).reshape(-1, 1)
    lowest = torch.finfo(torch.float64).min

    def batch(qq, kk, vv, masked):
        s = torch.einsum("hid,hjd->hij", qq, kk) * scale                 # one sample: [heads, n, n]
        if masked:
            s = torch.cat([s + m_s.masked_fill(m_s == 0, lowest), s + m_s.masked_fill(m_s == 1, lowest)])
            vv = torch.cat([vv, vv])
        o = torch.einsum("hij,hjd->hid", s.softmax(-1), vv)              # (h1 heads) n d
        return o.reshape(-1, heads, n, d).permute(0, 2, 1, 3).reshape(-1, n, heads * d)

    qu, qc = q.chunk(2)
    ku, kc = k.chunk(2)
    vu, vc = v.chunk(2)
    outs = []
    for qq, kk, vv in ((qu, ku, vu), (qc, kc, vc)):
        outs.append(batch(qq[:heads], kk[:heads], vv[:heads], False))
        fg, bg = batch(qq[-heads:], kk[:heads], vv[:heads], True).chunk(2)
        outs.append(fg * m_t + bg * (1 - m_t))
    return torch.cat(outs)


def _qkv(B=4, heads=2, n=64, d=8):
    g = torch.Generator().manual_seed(3)
    return [torch.randn(B * heads, n, d, generator=g) for _ in range(3)]


def test_editor_matches_fp64_restatement_of_the_reference():
    heads, d = 2, 8
    q, k, v = _qkv()
    ms, mt = _masks()
    c = MutualSelfAttentionControlMask(0, 0, total_steps=5, mask_s=ms, mask_t=mt)
    c.num_att_layers = 32
    out = c(q, k, v, None, None, False, "down", heads, scale=d ** -0.5)
    ref = _ref64(q, k, v, heads, d ** -0.5, ms, mt)
    assert out.shape == (4, 64, heads * d) and out.dtype == torch.float32
    e = (out.double() - ref).abs().max().item()
    print(f"mask-guided editor vs fp64 restatement: max abs {e:.2e}")
    assert e <= 1e-5
    # the masks act: the target rows differ from plain mutual attention, the source rows are plain self-attention
    plain = AttentionBase.forward(c, q, k, v, None, (torch.bmm(q, k.transpose(1, 2)) * d ** -0.5).softmax(-1), False, "down", heads)
    assert (out[0] - plain[0]).abs().max() < 1e-5 and (out[2] - plain[2]).abs().max() < 1e-5
    assert (out[1] - plain[1]).abs().max() > 1e-2 and (out[3] - plain[3]).abs().max() > 1e-2


@pytest.mark.parametrize("why", ["step", "layer", "cross"])
def test_uncontrolled_calls_fall_through_to_attention_base(why):
    heads, d = 2, 8
    q, k, v = _qkv()
    ms, mt = _masks()
    c = MutualSelfAttentionControlMask(2, 3, total_steps=5, mask_s=ms, mask_t=mt)
    c.num_att_layers = 32
    c.cur_step, c.cur_att_layer = (1, 6) if why == "step" else (2, 4) if why == "layer" else (2, 6)
    attn = (torch.bmm(q, k.transpose(1, 2)) * d ** -0.5).softmax(-1)
    out = c(q, k, v, None, attn, why == "cross", "mid", heads, scale=d ** -0.5)
    assert torch.equal(out, AttentionBase.forward(c, q, k, v, None, attn, False, "mid", heads))


@pytest.mark.parametrize("N", [64, 256, 1024])
def test_plan_lists_are_nonzero_of_torchs_resized_masks(N):
    ms, mt = _masks(64)
    plan = ControlPlan(None, "masactrl_mask", "cpu", masa_steps=[1, 2], masa_layers=[0], mask_s=ms, mask_t=mt, mask_tokens=[N])
    H = int(N ** 0.5)
    rs = F.interpolate(ms[None, None], (H, H)).flatten()
    rt = F.interpolate(mt[None, None], (H, H)).flatten()
    fk, bk, fq, bq = plan.mask_lists(N)
    for got, want in ((fk, rs == 1), (bk, rs == 0), (fq, rt == 1), (bq, rt == 0)):
        assert got.dtype == torch.int32 and torch.equal(got.long(), torch.nonzero(want).flatten())
    assert fk.numel() + bk.numel() == N and fq.numel() + bq.numel() == N
    sig = plan.signature(None)
    assert sig[0] == "masactrl_mask" and sig[-1] == ((N, (fk.numel(), bk.numel(), fq.numel(), bq.numel())),)


def _fake_unet(head_dims=(40, 80), sample=32, precision="f16x3"):
    """the attributes the lowering reads: two levels, one transformer layer (self, cross) per block"""
    class Attention:
        def __init__(self, i, d, cross):
            self._exec_index, self.dim_head, self.is_cross = i, d, cross

    attn = Attention

    def block(i0, d, sampler):
        mods = [attn(i0, d, False), attn(i0 + 1, d, True)]
        return types.SimpleNamespace(modules=lambda: mods, downsamplers=sampler, upsamplers=sampler)

    return types.SimpleNamespace(precision=precision, x3p=True, cfg=types.SimpleNamespace(sample_size=sample),
                                 down_blocks=[block(0, head_dims[0], [1]), block(2, head_dims[1], None)],
                                 mid_block=block(4, head_dims[1], None),
                                 up_blocks=[block(6, head_dims[1], [1]), block(8, head_dims[0], None)])


def _editor(ms, mt, layers=(0, 1, 2, 3, 4)):
    return MutualSelfAttentionControlMask(1, 0, layer_idx=list(layers), total_steps=4, mask_s=ms, mask_t=mt)


def test_lowering_gives_the_fused_plan_for_binary_masks(capsys):
    ms, mt = _masks()
    plan = lower_editor(_editor(ms, mt), "cpu", _fake_unet())
    assert plan is not None and plan.kind == "masactrl_mask" and plan.mask_tokens == (256, 1024)
    assert plan.masa_layers == {0, 1, 2, 3, 4} and plan.masa_steps == {1, 2, 3}
    assert lower_editor(_editor(ms, mt), "cpu", _fake_unet(precision="f16")) is None
    assert "generic path" in capsys.readouterr().out


@pytest.mark.parametrize("case", ["non_binary", "all_zero_mask_s", "missing_mask_t", "d160_layer"])
def test_lowering_refuses_what_the_fused_rule_does_not_cover(case, capsys):
    ms, mt = _masks()
    unet = _fake_unet()
    if case == "non_binary":
        ms = ms * 0.5
    elif case == "all_zero_mask_s":
        ms = torch.zeros_like(ms)
    elif case == "missing_mask_t":
        mt = None
    else:
        unet = _fake_unet(head_dims=(40, 160))
    assert lower_editor(_editor(ms, mt), "cpu", unet) is None
    said = capsys.readouterr().out
    assert said.count("mask-guided MasaCtrl takes the generic path") == 1


def test_params_block_size_and_zeroed_new_fields():
    lib = hip.load()
    assert hip.ctypes.sizeof(hip.IefAttnF32Params) == lib.ief_struct_size(6)
    names = [f[0] for f in hip.IefAttnF32Params._fields_]
    assert names[-3:] == ["q_idx", "k_idx", "gate"], "new fields go at the END of the block"
    p = hip.IefAttnF32Params()
    assert not p.q_idx and not p.k_idx and not p.gate
    assert lib.ief_attn_flash_f32(hip.ctypes.byref(p), None) == -1      # all-zero block: IEF_EINVAL from the argument checks, as before


def test_mask_pngs_are_written_without_torchvision(tmp_path):
    from PIL import Image
    import numpy as np
    from ief_amd.masactrl.model.attention_control import load_mask_png
    ms, mt = _masks()
    MutualSelfAttentionControlMask(1, 0, total_steps=4, mask_s=ms, mask_t=mt, mask_save_dir=str(tmp_path / "m"))
    for nm, m in (("mask_s.png", ms), ("mask_t.png", mt)):
        img = np.asarray(Image.open(tmp_path / "m" / nm))
        assert img.shape == (16, 16, 3) and np.array_equal(img[..., 0], (m.numpy() * 255).astype(np.uint8))
        assert torch.equal(load_mask_png(str(tmp_path / "m" / nm)), m)
