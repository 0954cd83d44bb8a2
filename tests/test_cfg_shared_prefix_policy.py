"""Host-only: when does a CFG denoising step run the prefix its two halves share once (`denoise.cfg_shared_prefix_reason`), and what
does a control plan say about the first self-attention (`ControlPlan.controls_first_self`)?"""
from types import SimpleNamespace

import pytest
import torch

import ief_amd  # noqa: F401
from ief_amd.control import ControlPlan
from ief_amd.denoise import cfg_shared_prefix_reason

OK = dict(mode="denoise", cfg=True, x3p=True, aug=False, first_block_cross=True, native=True, fused_cross=True, ln_folded=False,
          plan_on_first_self=False, taps=False, enabled=True)


def test_the_flagship_step_is_eligible():
    assert cfg_shared_prefix_reason(**OK) is None


@pytest.mark.parametrize("change,word", [
    (dict(aug=True), "additional"),                        # SDXL: a time-embedding row per batch row
    (dict(first_block_cross=False), "no cross-attention"),  # SDXL's down_blocks[0]
    (dict(native=False), "generic"),                       # a Python controller hooked an attention module of down_blocks[0]
    (dict(taps=True), "tapped"),
    (dict(plan_on_first_self=True), "control plan"),       # MasaCtrl from layer 0, P2P self-replace on <= 16 x 16 latents, PnP there
    (dict(cfg=False), "classifier-free"),                  # no guidance: no second half
    (dict(mode="invert"), "classifier-free"),              # DDIM inversion
    (dict(x3p=False), "operand planes"),                   # the f16 and f32 modes (and f16x3 channel counts without the planes trunk)
    (dict(fused_cross=False), "fused"),
    (dict(ln_folded=True), "folded"),
    (dict(enabled=False), "IEF_CFG_SHARED_PREFIX"),
])
def test_one_fact_off_means_the_whole_batch(change, word):
    reason = cfg_shared_prefix_reason(**{**OK, **change})
    assert isinstance(reason, str) and word in reason, reason


def test_every_fact_is_required_by_name():
    with pytest.raises(TypeError):
        cfg_shared_prefix_reason(mode="denoise", cfg=True)
    with pytest.raises(TypeError):
        cfg_shared_prefix_reason("denoise", True, True)


def _unet(first_index=0):
    first = SimpleNamespace(_exec_index=first_index)
    tr = SimpleNamespace(transformer_blocks=[SimpleNamespace(attn1=first)])
    return SimpleNamespace(down_blocks=[SimpleNamespace(attentions=[tr])]), first


def test_plans_and_the_first_self_attention():
    unet, first = _unet()
    masa = lambda layers: ControlPlan(None, "masactrl", "cpu", masa_steps=[1, 2], masa_layers=layers)
    assert masa([0, 1, 2]).controls_first_self(unet, 1024)
    assert not masa([2, 3]).controls_first_self(unet, 1024)
    # decided from the layers alone: an EMPTY step list today may be another one after the loop is re-pointed
    assert ControlPlan(None, "masactrl", "cpu", masa_steps=[], masa_layers=[0]).controls_first_self(unet, 1024)
    mask = ControlPlan(None, "masactrl_mask", "cpu", masa_steps=[1], masa_layers=[0], mask_s=torch.ones(4, 4), mask_t=torch.ones(4, 4))
    assert mask.controls_first_self(unet, 1024)
    p2p = ControlPlan(None, "p2p", "cpu", num_prompts=2, num_steps=3, mt=torch.zeros(1, 96, 96), coef_table=torch.zeros(4, 1, 2, 96),
                      self_window=(0, 2), self_max_tokens=256)
    assert p2p.controls_first_self(unet, 256) and not p2p.controls_first_self(unet, 257) and not p2p.controls_first_self(unet, 4096)
    assert ControlPlan(None, "pnp", "cpu", pnp_layers=[id(first)]).controls_first_self(unet, 4096)
    assert not ControlPlan(None, "pnp", "cpu", pnp_layers=[id(unet)]).controls_first_self(unet, 4096)
    assert not ControlPlan(None, "empty", "cpu").controls_first_self(unet, 16)
    no_attn = SimpleNamespace(down_blocks=[SimpleNamespace(attentions=[])])
    assert not masa([0]).controls_first_self(no_attn, 1024)
