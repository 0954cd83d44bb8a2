"""MasaCtrl with united source and target keys (`MutualSelfAttentionControlUnion`) on the host: the editor's Python against an fp64
restatement of the rule, the generalised `attn_batch`, the plan's step tables, the parameter block, the host part of the lowering
decision and the CLI flag.  No GPU.

The rule (UNet batch [u_src, u_tgt, c_src, c_tgt], a self-attention call at a controlled (step, layer)): row u_tgt attends with its
own queries over [K_u_src ; K_u_tgt] with values [V_u_src ; V_u_tgt] -- ONE softmax over 2 N keys, source keys first -- and row c_tgt
likewise over its half; rows u_src and c_src are plain self-attention on their own K, V.  Everything else is `AttentionBase.forward`.

Stated tolerance: the fp32 editor's target rows vs the fp64 restatement <= 1e-6 of max |reference| (a softmax over 48 keys and
a 48-term convex combination of unit-scale values in fp32: some 1e-7 per operation).  The source rows and the uncontrolled calls
are held to bit equality.  Every test prints what it measured.
"""
import importlib.util
import os
import types

import pytest
import torch

import ief_amd  # noqa: F401
from ief_amd import hip
from ief_amd.control import ControlPlan
from ief_amd.masactrl.model.attention_base import AttentionBase
from ief_amd.masactrl.model.attention_control import MutualSelfAttentionControl, MutualSelfAttentionControlUnion
from ief_amd.masactrl.model.register import lower_editor

HEADS, N, D = 2, 24, 8
SCALE = D ** -0.5


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _qkv(batch=4):
    q, k, v = (_rand(batch * HEADS, N, D, seed=11 + i) for i in range(3))
    sim = torch.bmm(q, k.transpose(1, 2)) * SCALE
    return q, k, v, sim, sim.softmax(-1)


def _editor():
    """controlled at steps 1.. and layers 2..; `num_att_layers` as a registration would set it"""
    ed = MutualSelfAttentionControlUnion(start_step=1, start_layer=2, total_steps=4)
    ed.num_att_layers = 32
    return ed


def _at(ed, step, layer):
    ed.cur_step, ed.cur_att_layer = step, 2 * layer
    return ed


def _base(q, k, v, sim, attn, rows=slice(None)):
    return AttentionBase.forward(AttentionBase(), q[rows], k[rows], v[rows], None, attn[rows], False, "up", HEADS, scale=SCALE)


def _target64(q, k, v, src, tgt):
    """fp64: softmax(scale q_tgt [K_src ; K_tgt]^T) [V_src ; V_tgt] per head -> [N, heads * d]"""
    q, k, v = q.double(), k.double(), v.double()
    rows = lambda t, b: t[b * HEADS:(b + 1) * HEADS]
    K, V = torch.cat([rows(k, src), rows(k, tgt)], 1), torch.cat([rows(v, src), rows(v, tgt)], 1)       # [h, 2N, d]
    out = torch.softmax(rows(q, tgt) @ K.transpose(1, 2) * SCALE, -1) @ V                                # [h, N, d]
    return out.permute(1, 0, 2).reshape(N, HEADS * D)


def test_controlled_call_targets_vs_fp64_sources_bit_equal():
    q, k, v, sim, attn = _qkv()
    out = _at(_editor(), 1, 2).forward(q, k, v, sim, attn, False, "up", HEADS, scale=SCALE)
    assert out.shape == (4, N, HEADS * D)
    for src, tgt in ((0, 1), (2, 3)):
        ref = _target64(q, k, v, src, tgt)
        e = ((out[tgt].double() - ref).abs().max() / ref.abs().max()).item()
        mutual = _target64(q, k, v, src, src)      # what ignoring the target's own keys would give (queries still the target's)
        print(f"row {tgt}: |editor - fp64| / max|fp64| = {e:.2e}")
        assert e <= 1e-6
        rows = slice(src * HEADS, (src + 1) * HEADS)
        assert torch.equal(out[src], _base(q, k, v, sim, attn, rows)[0]), "a source row is plain self-attention, bit for bit"
        assert not torch.allclose(out[tgt].double(), mutual, atol=1e-3)


def test_uncontrolled_calls_are_attention_base_bit_for_bit():
    q, k, v, sim, attn = _qkv()
    want = _base(q, k, v, sim, attn)
    ed = _editor()
    for step, layer, cross, what in ((0, 2, False, "uncontrolled step"), (1, 1, False, "uncontrolled layer"), (1, 2, True, "cross")):
        got = _at(ed, step, layer).forward(q, k, v, sim, attn, cross, "up", HEADS, scale=SCALE)
        assert torch.equal(got, want), what


def test_another_batch_than_four_raises():
    q, k, v, sim, attn = _qkv(batch=2)
    with pytest.raises(RuntimeError, match="u_src, u_tgt, c_src, c_tgt"):
        _at(_editor(), 1, 2).forward(q, k, v, sim, attn, False, "up", HEADS, scale=SCALE)
    # uncontrolled calls never look at the batch
    assert _at(_editor(), 0, 2).forward(q, k, v, sim, attn, False, "up", HEADS, scale=SCALE).shape == (2, N, HEADS * D)


def test_attn_batch_with_one_key_sample_is_unchanged():
    """the expression `attn_batch` had before it took the keys of several samples, inline"""
    q, k, v, _, _ = _qkv()
    ed = MutualSelfAttentionControl(start_step=1, start_layer=2, total_steps=4)
    for qs in (q, q[:2 * HEADS], q[HEADS:2 * HEADS]):
        k1, v1 = k[:HEADS], v[:HEADS]
        bh, n, d = qs.shape
        b = bh // HEADS
        qh = qs.reshape(b, HEADS, n, d).permute(1, 0, 2, 3).reshape(HEADS, b * n, d)
        s = torch.bmm(qh, k1.transpose(1, 2)) * SCALE
        want = torch.bmm(s.softmax(-1), v1).reshape(HEADS, b, n, d).permute(1, 2, 0, 3).reshape(b, n, HEADS * d)
        got = ed.attn_batch(qs, k1, v1, None, None, False, "up", HEADS, scale=SCALE)
        assert torch.equal(got, want)
    # two key samples: keys concatenated per head, in sample order
    got = ed.attn_batch(q[HEADS:2 * HEADS], k[:2 * HEADS], v[:2 * HEADS], None, None, False, "up", HEADS, scale=SCALE)
    ref = _target64(q, k, v, 0, 1)
    assert ((got[0].double() - ref).abs().max() / ref.abs().max()).item() <= 1e-6


def test_plan_step_tables():
    tab, k2 = ControlPlan.union_tables([1, 3])
    assert tab.dtype == torch.int32 and k2.dtype == torch.int32 and tab.device.type == "cpu" and k2.device.type == "cpu"
    ident, none = [0, 1, 2, 3], [-1, -1, -1, -1]
    assert tab.tolist() == [ident, [0, 0, 2, 2], ident, [0, 0, 2, 2], ident], "first-segment rows; identity row past the end"
    assert k2.tolist() == [none, [-1, 1, -1, 3], none, [-1, 1, -1, 3], none], "second-segment rows; -1 row past the end"
    assert torch.equal(tab, ControlPlan.masa_table([1, 3], 4))
    t0, k0 = ControlPlan.union_tables([])
    assert t0.tolist() == [ident] and k0.tolist() == [none]


def test_plan_kind_signature_and_batch():
    assert "masactrl_union" in ControlPlan.MASA_KINDS and "masactrl_union" not in ControlPlan.GATED_KINDS
    ed = _editor()
    plan = lower_editor(ed, "cpu", _fake_unet())
    assert plan is not None and plan.kind == "masactrl_union" and plan.controller is ed
    assert plan.masa_steps == {1, 2, 3} and plan.masa_layers == set(range(2, 16))
    assert plan.signature(None) == ("masactrl_union", tuple(range(2, 16)), 5)
    other = MutualSelfAttentionControlUnion(start_step=1, start_layer=2, step_idx=[2, 3], total_steps=4)
    assert lower_editor(other, "cpu", _fake_unet()).signature(None) == plan.signature(None), "step_idx is table contents"
    with pytest.raises(RuntimeError, match="u_src, u_tgt, c_src, c_tgt"):
        plan.prepare(2)
    first = lambda i: types.SimpleNamespace(down_blocks=[types.SimpleNamespace(attentions=[types.SimpleNamespace(
        transformer_blocks=[types.SimpleNamespace(attn1=types.SimpleNamespace(_exec_index=i))])])])
    assert plan.controls_first_self(first(4), 1024) and not plan.controls_first_self(first(0), 1024)


def test_params_block():
    lib = hip.load()
    names = [f[0] for f in hip.IefAttnF32Params._fields_]
    assert "k2_src" in names and "v2_src" in names
    assert names[-3:] == ["q_idx", "k_idx", "gate"]
    assert names.index("k_cls") == names.index("v2_src") + 1 == names.index("k2_src") + 2, "the pair sits directly in front of k_cls"
    assert hip.ctypes.sizeof(hip.IefAttnF32Params) == lib.ief_struct_size(6)
    assert hip.ABI_VERSION == 4 and lib.ief_abi_version() == 4
    p = hip.IefAttnF32Params()
    assert not p.k2_src and not p.v2_src


def _fake_unet(precision="f16x3", d_low=80):
    """two levels (32 x 32 with head dim 40, 16 x 16 with head dim d_low), one transformer layer (self, cross) per block"""
    class Attention:
        def __init__(self, i, d, cross):
            self._exec_index, self.dim_head, self.is_cross = i, d, cross

    def block(i0, d, sampler):
        mods = [Attention(i0, d, False), Attention(i0 + 1, d, True)]
        return types.SimpleNamespace(modules=lambda: mods, downsamplers=sampler, upsamplers=sampler)

    return types.SimpleNamespace(precision=precision, x3p=True, cfg=types.SimpleNamespace(sample_size=32),
                                 down_blocks=[block(0, 40, [1]), block(2, d_low, None)], mid_block=block(4, d_low, None),
                                 up_blocks=[block(6, d_low, [1]), block(8, 40, None)])


@pytest.mark.parametrize("unet", [_fake_unet("f32"), _fake_unet("f16"), _fake_unet(d_low=160), None])
def test_lowering_refusals_print_one_line(unet, capsys):
    ed = _editor()
    capsys.readouterr()
    assert lower_editor(ed, "cpu", unet) is None
    said = capsys.readouterr().out
    print(said)
    assert said.count("\n") == 1 and said.count("MasaCtrl Union takes the generic path: ") == 1


# ------------------------------------------------------------------------------------------------------------- CLI
def _cli(name):
    path = os.path.join(os.path.dirname(os.path.abspath(ief_amd.__file__)), "masactrl", name)
    spec = importlib.util.spec_from_file_location("masactrl_union_cli_" + name[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["edit_syn.py", "edit_real.py"])
def test_cli_flag_and_conflicts(name, capsys):
    mod = _cli(name)
    assert mod.parser.parse_args([]).union is False
    assert mod.parser.parse_args(["--union"]).union is True
    for extra in (["--mask_s", "a.png", "--mask_t", "b.png"], ["--mask_auto"]):
        with pytest.raises(SystemExit) as e:
            mod.main(["--union"] + extra)
        assert e.value.code == 2 and "--union" in capsys.readouterr().err
