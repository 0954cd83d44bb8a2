"""MasaCtrl with masks from cross-attention (`MutualSelfAttentionControlMaskAuto`) on the host: the editor's Python against an fp64
restatement of the rule, its counters and per-step state, the host part of the lowering decision and the CLI flags.  No GPU.

The rule (UNet batch [u_src, u_tgt, c_src, c_tgt]): every cross-attention call with 256 queries appends the head-mean of its map to a
per-step list; a controlled self-attention layer with c >= 1 collected maps takes A = their mean as [B, 16, 16, 77], img_T =
A[..., T].sum(-1), normalises each batch row to (img - min) / (max - min), takes row c_src of img_ref as KEY mask and row c_tgt of
img_cur as QUERY mask, resizes both (nearest) to the layer and binarises with >= thres; both target rows attend to their half's source
K / V once with the non-foreground keys at finfo.min (+ 1 on the others) and once with the foreground keys at finfo.min, blended
by the query mask.  c == 0: plain mutual attention.

Stated tolerance: the fp32 editor vs the fp64 restatement <= 1e-5 absolute (outputs are convex combinations of unit-scale Gaussian
values; fp32 rounding of <= 1024-term softmaxes is some 1e-7 per term) with IDENTICAL masks: the test first checks that no normalised
pixel lies within 1e-5 of thres, so fp32 and fp64 binarise alike.  Every test prints what it measured.
"""
import importlib.util
import os
import types

import pytest
import torch
import torch.nn.functional as F

import ief_amd  # noqa: F401
from ief_amd.masactrl.model.attention_base import AttentionBase
from ief_amd.masactrl.model.attention_control import MutualSelfAttentionControl, MutualSelfAttentionControlMaskAuto
from ief_amd.masactrl.model.register import auto_mask_refusal, lower_editor

HEADS, D, L = 2, 8, 77
REF, CUR = [2, 5, 5], [3]          # a token listed twice counts twice


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _cross_maps(n, seed, tokens=256):
    """n softmax maps [(4 heads), tokens, 77] with some spatial structure"""
    return [(_rand(4 * HEADS, tokens, L, seed=seed + i) * 2).softmax(-1) for i in range(n)]


def _qkv(n, seed=3):
    return [_rand(4 * HEADS, n, D, seed=seed + i) for i in range(3)]


def _masks64(maps, res, thres):
    """the rule's masks in fp64 from the raw maps -> (key mask, query mask, smallest |normalised - thres|)"""
    A = torch.stack([m.double().reshape(4, HEADS, 256, L).mean(1) for m in maps]).mean(0).reshape(4, 16, 16, L)
    out, gap = [], float("inf")
    for idx, row in ((REF, 2), (CUR, 3)):
        img = A[..., idx].sum(-1)
        lo, hi = img.amin(dim=(1, 2), keepdim=True), img.amax(dim=(1, 2), keepdim=True)
        img = ((img - lo) / (hi - lo))[row]
        gap = min(gap, (img - thres).abs().min().item())
        out.append((F.interpolate(img[None, None], (res, res))[0, 0] >= thres).double())
    return out[0], out[1], gap


def _ref64(q, k, v, scale, key_mask, query_mask):
    q, k, v = q.double(), k.double(), v.double()
    n = q.shape[1]
    lowest = torch.finfo(torch.float64).min

    def attend(qq, kk, vv, bias=None):
        s = torch.einsum("hid,hjd->hij", qq, kk) * scale
        if bias is not None:
            s = s + bias
        return torch.einsum("hij,hjd->hid", s.softmax(-1), vv).permute(1, 0, 2).reshape(1, n, -1)

    outs = []
    for half in (0, 2):
        src, tgt = slice(half * HEADS, (half + 1) * HEADS), slice((half + 1) * HEADS, (half + 2) * HEADS)
        outs.append(attend(q[src], k[src], v[src]))
        if key_mask is None:
            outs.append(attend(q[tgt], k[src], v[src]))
            continue
        km, qm = key_mask.flatten(), query_mask.reshape(-1, 1)
        fg = attend(q[tgt], k[src], v[src], km.masked_fill(km == 0, lowest))
        bg = attend(q[tgt], k[src], v[src], km.masked_fill(km == 1, lowest))
        outs.append(fg * qm + bg * (1 - qm))
    return torch.cat(outs)


def _editor(thres=0.3, **kw):
    c = MutualSelfAttentionControlMaskAuto(1, 0, total_steps=4, thres=thres, ref_token_idx=REF, cur_token_idx=CUR, **kw)
    c.num_att_layers = 8
    return c


@pytest.mark.parametrize("res", [16, 32])
def test_editor_matches_fp64_restatement_of_the_rule(res):
    thres, scale = 0.3, D ** -0.5
    c = _editor(thres)
    c.cur_step = 1
    maps = _cross_maps(3, seed=10)
    q, k, v = _qkv(res * res)
    qx, kx, vx = _rand(4 * HEADS, 256, D, seed=7), _rand(4 * HEADS, L, D, seed=8), _rand(4 * HEADS, L, D, seed=9)
    for m in maps:                  # three cross-attention calls at the 16 x 16 level: plain attention, maps collected
        out = c(qx, kx, vx, None, m, True, "down", HEADS, scale=scale)
        assert torch.equal(out, AttentionBase.forward(c, qx, kx, vx, None, m, True, "down", HEADS))
    assert len(c.cross_attns) == 3 and c.cross_attns[0].shape == (4, 256, L)
    c(qx[:, :64], kx, vx, None, _cross_maps(1, 50, tokens=64)[0], True, "down", HEADS, scale=scale)
    assert len(c.cross_attns) == 3, "a map with 64 queries is not collected"
    assert (c.cur_step, c.cur_att_layer) == (1, 4)
    out = c(q, k, v, None, None, False, "up", HEADS, scale=scale)
    key_mask, query_mask, gap = _masks64(maps, res, thres)
    assert gap > 1e-5, f"test inputs: a normalised pixel lies {gap:.1e} from thres"
    assert torch.equal(c.mask_s.double(), key_mask) and torch.equal(c.mask_t.double(), query_mask)
    ref = _ref64(q, k, v, scale, key_mask, query_mask)
    e = (out.double() - ref).abs().max().item()
    plain = _ref64(q, k, v, scale, None, None)
    moved = (ref[1] - plain[1]).abs().max().item()
    print(f"res {res}: editor vs fp64 restatement {e:.2e}; fg keys {int(key_mask.sum())}/{res * res}, fg queries "
          f"{int(query_mask.sum())}/{res * res}, gap to thres {gap:.1e}; the masks move the target rows by {moved:.2e}")
    assert out.shape == (4, res * res, HEADS * D) and out.dtype == torch.float32
    assert e <= 1e-5
    assert 0 < key_mask.sum() < res * res and moved > 1e-2
    assert (out[0].double() - plain[0]).abs().max() <= 1e-5 and (out[2].double() - plain[2]).abs().max() <= 1e-5


def test_no_maps_yet_is_plain_mutual_attention_and_after_step_clears():
    scale = D ** -0.5
    c = _editor()
    c.cur_step = 1
    q, k, v = _qkv(256)
    out = c(q, k, v, None, None, False, "down", HEADS, scale=scale)          # c == 0
    plain = MutualSelfAttentionControl(1, 0, total_steps=4)
    plain.num_att_layers, plain.cur_step = 8, 1
    assert torch.equal(out, plain(q, k, v, None, None, False, "down", HEADS, scale=scale))
    assert c.mask_s is None and c.mask_t is None
    m = _cross_maps(1, seed=20)[0]
    for _ in range(7):              # the step's remaining seven calls: the counter wraps, after_step clears the list
        c(q, _rand(4 * HEADS, L, D, seed=1), _rand(4 * HEADS, L, D, seed=2), None, m, True, "up", HEADS, scale=scale)
    assert (c.cur_step, c.cur_att_layer) == (2, 0) and c.cross_attns == []


@pytest.mark.parametrize("why", ["step", "layer"])
def test_outside_the_schedule_is_attention_base(why):
    scale = D ** -0.5
    c = MutualSelfAttentionControlMaskAuto(2, 3, total_steps=5, ref_token_idx=REF, cur_token_idx=CUR)
    c.num_att_layers = 32
    c.cur_step, c.cur_att_layer = (1, 6) if why == "step" else (2, 4)
    c.cross_attns = [t.reshape(4, HEADS, 256, L).mean(1) for t in _cross_maps(1, seed=30)]
    q, k, v = _qkv(64)
    attn = (torch.bmm(q, k.transpose(1, 2)) * scale).softmax(-1)
    out = c(q, k, v, None, attn, False, "mid", HEADS, scale=scale)
    assert torch.equal(out, AttentionBase.forward(c, q, k, v, None, attn, False, "mid", HEADS))


def test_mask_save_dir_writes_both_masks(tmp_path):
    c = _editor(0.3, mask_save_dir=str(tmp_path / "m"))
    c.cur_step = 1
    c.cross_attns = [t.reshape(4, HEADS, 256, L).mean(1) for t in _cross_maps(2, seed=40)]
    q, k, v = _qkv(256)
    c(q, k, v, None, None, False, "up", HEADS, scale=D ** -0.5)
    assert sorted(os.listdir(tmp_path / "m")) == ["mask_s_1_0.png", "mask_t_1_0.png"]


# ------------------------------------------------------------------------------------------------------------- lowering
def _ok_editor(**kw):
    args = dict(thres=0.3, ref_token_idx=[1, 2, 2], cur_token_idx=[1])
    args.update(kw)
    return MutualSelfAttentionControlMaskAuto(1, 0, layer_idx=[1, 2, 3], total_steps=4, **args)


SHAPES = [(40, 1024), (80, 256)]


def test_lowering_accepts_what_the_fused_rule_covers():
    assert auto_mask_refusal(_ok_editor(), "f16x3", True, True, SHAPES) is None
    assert auto_mask_refusal(_ok_editor(thres=1.0), "f16x3", True, True, SHAPES) is None


@pytest.mark.parametrize("case,word", [
    ("precision", "f16x3"), ("no_planes", "f16x3"), ("save_dir", "mask_save_dir"), ("thres0", "thres"), ("thres_big", "thres"),
    ("token_out", "ref_token_idx"), ("token_neg", "cur_token_idx"), ("batch", "batch"), ("d160", "head dim"),
    ("few_tokens", "fewer"), ("odd_tokens", "multiple"),
])
def test_lowering_refusals_each_give_a_reason(case, word, tmp_path):
    ed, prec, fp, shapes, batch = _ok_editor(), "f16x3", True, SHAPES, 4
    if case == "precision":
        prec = "f16"
    elif case == "no_planes":
        fp = False
    elif case == "save_dir":
        ed = _ok_editor(mask_save_dir=str(tmp_path / "m"))
    elif case == "thres0":
        ed = _ok_editor(thres=0.0)
    elif case == "thres_big":
        ed = _ok_editor(thres=1.5)
    elif case == "token_out":
        ed = _ok_editor(ref_token_idx=[1, 77])
    elif case == "token_neg":
        ed = _ok_editor(cur_token_idx=[-1])
    elif case == "batch":
        batch = 2
    elif case == "d160":
        shapes = [(40, 1024), (160, 256)]
    elif case == "few_tokens":
        shapes = [(80, 64)]
    else:
        shapes = [(80, 24 * 24 * 4 + 16)]
    why = auto_mask_refusal(ed, prec, True, fp, shapes, batch)
    print(f"{case}: {why}")
    assert why is not None and word in why


def _fake_unet(precision="f16x3"):
    """two levels (32 x 32 with head dim 40, 16 x 16 with head dim 80), one transformer layer (self, cross) per block"""
    class Attention:
        def __init__(self, i, d, cross):
            self._exec_index, self.dim_head, self.is_cross = i, d, cross

    def block(i0, d, sampler):
        mods = [Attention(i0, d, False), Attention(i0 + 1, d, True)]
        return types.SimpleNamespace(modules=lambda: mods, downsamplers=sampler, upsamplers=sampler)

    return types.SimpleNamespace(precision=precision, x3p=True, cfg=types.SimpleNamespace(sample_size=32),
                                 down_blocks=[block(0, 40, [1]), block(2, 80, None)], mid_block=block(4, 80, None),
                                 up_blocks=[block(6, 80, [1]), block(8, 40, None)])


def test_lowering_counts_slots_in_execution_order(capsys):
    plan = lower_editor(_ok_editor(), "cpu", _fake_unet())
    assert plan is not None and plan.kind == "masactrl_mask_auto"
    assert plan.auto_slots == {3: 0, 5: 1, 7: 2}, "the 256-token cross-attention modules, in execution order"
    assert plan.auto_layers == {2: (0, 256), 4: (1, 256), 6: (2, 256)}, "layer -> (maps collected before it, tokens)"
    assert torch.equal(plan.auto_weights()[0, :3], torch.tensor([0., 1., 2.])) and plan.auto_weights()[1].sum() == 1
    sig = plan.signature(None)
    other = lower_editor(_ok_editor(thres=0.7, cur_token_idx=[4, 5]), "cpu", _fake_unet())
    assert other.signature(None) == sig, "thres and the token lists are table contents, not signature"
    assert plan.controls_first_self(types.SimpleNamespace(down_blocks=[types.SimpleNamespace(attentions=[types.SimpleNamespace(
        transformer_blocks=[types.SimpleNamespace(attn1=types.SimpleNamespace(_exec_index=2))])])]), 1024)
    assert lower_editor(_ok_editor(), "cpu", _fake_unet("f16")) is None
    assert capsys.readouterr().out.count("auto-mask MasaCtrl takes the generic path") == 1


# ------------------------------------------------------------------------------------------------------------- CLI
def _cli(name):
    path = os.path.join(os.path.dirname(os.path.abspath(ief_amd.__file__)), "masactrl", name)
    spec = importlib.util.spec_from_file_location("masactrl_cli_" + name[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["edit_syn.py", "edit_real.py"])
def test_cli_flags(name):
    mod = _cli(name)
    a = mod.parser.parse_args([])
    assert (a.mask_auto, a.thres, a.ref_token_idx, a.cur_token_idx, a.mask_save_dir) == (False, 0.1, [1], [1], None)
    a = mod.parser.parse_args(["--mask_auto", "--thres", "0.3", "--ref_token_idx", "2", "5", "5", "--cur_token_idx", "3",
                               "--mask_save_dir", "m"])
    assert (a.mask_auto, a.thres, a.ref_token_idx, a.cur_token_idx, a.mask_save_dir) == (True, 0.3, [2, 5, 5], [3], "m")
    with pytest.raises(SystemExit):
        mod.main(["--mask_auto", "--mask_s", "a.png", "--mask_t", "b.png"])
