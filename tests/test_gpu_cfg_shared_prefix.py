"""The CFG step with a shared prefix (`denoise.cfg_shared_prefix_reason`, `UNet2DConditionModel.forward(cfg_pair=True)`) on a real
MI355X: `small` family (32 x 32 latents, 1024 tokens in the first transformer), f16x3, a 3-step AttentionRefine edit.

Stated bounds (every test prints what it measured):
    captured step graph vs eager stepping, shared form        bit for bit
    shared form vs the form that runs the whole CFG batch     <= the distance of the whole-batch form from the fp32 oracle
                                                                 (`oracle/p2p_ref.py`), measured in the same test: the Bp-row prefix
                                                                 launches may take other tile / split-K plans than the 2 Bp-row ones,
                                                                 which moves last bits -- equally in both halves -- and nothing else
    a plan that controls the first self-attention             the whole-batch form, said once in the log
    one eager step's launches                                  conv_in writes its planes (no splitter launch), the loop hands the
                                                                 UNet its Bp latents (no CFG batch buffer, hence no copy into one), ONE
                                                                 repeat launch, every GEMM / convolution in front of it at Bp rows
"""
import logging
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import denoise, hip  # noqa: E402
from ief_amd.denoise import FusedDenoiser  # noqa: E402
from ief_amd.p2p.model.attention_control import AttentionRefine  # noqa: E402
from ief_amd.p2p.model.register import register_attention_control, unregister_attention_control  # noqa: E402
from ief_amd.p2p.model.sd_utils import _encode_prompts  # noqa: E402
from oracle import p2p_ref  # noqa: E402

DEV = torch.device("cuda:0")
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]
STEPS = 3


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.pipeline import StableDiffusionPipeline
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")
    with torch.no_grad():
        u, c = _encode_prompts(pipe, PROMPTS)
    hw = pipe.cfg.sample_size
    x_T = torch.randn(1, 4, hw, hw, generator=torch.Generator().manual_seed(8888))
    return pipe, torch.cat([u, c]), x_T


def _edit(small, shared, use_graph, monkeypatch, steps=STEPS):
    pipe, ctx, x_T = small
    monkeypatch.setattr(denoise, "CFG_SHARED_PREFIX", shared)
    c = AttentionRefine(PROMPTS, pipe.tokenizer, steps, 0.8, 0.4, device=DEV)
    register_attention_control(pipe, c)
    pipe.scheduler.set_timesteps(steps)
    hw = pipe.cfg.sample_size
    loop = FusedDenoiser(pipe, ctx, 2, (hw, hw), 7.5, use_graph=use_graph)
    try:
        assert loop.shared == shared, loop.shared_reason
        lat = loop.run(x_T.to(DEV)).float().cpu()
    finally:
        loop.release()
        unregister_attention_control(pipe, c)
    assert c.cur_step == steps
    return lat


@pytest.fixture(scope="module")
def results():
    return {}


def test_graph_equals_eager_in_the_shared_form(small_x3, results, monkeypatch):
    results["graph"] = _edit(small_x3, True, True, monkeypatch)
    results["eager"] = _edit(small_x3, True, False, monkeypatch)
    assert torch.equal(results["graph"], results["eager"]), "captured-graph replay must equal eager stepping bit for bit"


def test_shared_form_vs_whole_batch_form_within_the_oracle_distance(small_x3, results, monkeypatch):
    pipe, ctx, x_T = small_x3
    shared = results.get("graph")
    if shared is None:
        shared = _edit(small_x3, True, True, monkeypatch)
    whole = _edit(small_x3, False, True, monkeypatch)
    c = AttentionRefine(PROMPTS, pipe.tokenizer, STEPS, 0.8, 0.4, device=DEV)
    rc = p2p_ref.P2PControlRef(mode="refine", num_prompts=2, cross_alpha=c.cross_replace_alpha.float().cpu(),
                               num_self_replace=c.num_self_replace, mapper=c.mapper.cpu(), alphas=c.alphas.float().cpu())
    ref = p2p_ref.edit_loop(pipe._state_dict, pipe.cfg, ctx.float().cpu(), x_T, rc, p2p_ref.DDIMRef(STEPS), 7.5)
    d_forms, d_oracle, d_shared = rel_err(shared, whole), rel_err(whole, ref), rel_err(shared, ref)
    print(f"{STEPS}-step AttentionRefine edit, small / f16x3: shared vs whole-batch form {d_forms:.3e}; whole-batch form vs fp32 oracle "
          f"{d_oracle:.3e}; shared form vs fp32 oracle {d_shared:.3e}")
    assert d_forms <= d_oracle


def test_a_plan_on_the_first_self_attention_keeps_the_whole_batch(small_x3, monkeypatch, caplog):
    from ief_amd.masactrl.model.attention_control import MutualSelfAttentionControl
    from ief_amd.masactrl.model.register import regiter_attention_editor_diffusers, unregister_attention_control as unreg
    pipe, ctx, x_T = small_x3
    monkeypatch.setattr(denoise, "CFG_SHARED_PREFIX", True)
    monkeypatch.setattr(denoise, "_said", set())
    hw = pipe.cfg.sample_size
    lats = []
    with caplog.at_level(logging.WARNING, logger="ief_amd.denoise"):
        for layers in (list(range(0, 11)), list(range(0, 11)), list(range(2, 11))):
            c = MutualSelfAttentionControl(1, 2, layer_idx=layers, total_steps=STEPS)
            regiter_attention_editor_diffusers(pipe, c)
            assert pipe.unet._plan is not None and pipe.unet._plan.kind == "masactrl"
            pipe.scheduler.set_timesteps(STEPS)
            loop = FusedDenoiser(pipe, ctx, 2, (hw, hw), 7.5, use_graph=False)
            try:
                assert loop.shared == (layers[0] != 0), loop.shared_reason
                if not loop.shared:
                    assert "first transformer" in loop.shared_reason and loop.lat_in is not loop.lat
                lats.append(loop.run(x_T.to(DEV).expand(2, -1, -1, -1), num_steps=2).float().cpu())
            finally:
                loop.release()
                unreg(pipe, c)
    said = [r for r in caplog.records if "shared prefix" in r.getMessage()]
    assert len(said) == 1 and "first transformer" in said[0].getMessage(), [r.getMessage() for r in caplog.records]
    assert torch.equal(lats[0], lats[1])


def test_launches_of_one_eager_step(small_x3, monkeypatch):
    pipe, ctx, x_T = small_x3
    monkeypatch.setattr(denoise, "CFG_SHARED_PREFIX", True)
    monkeypatch.setattr(hip, "PROF_SHAPES", True)
    c = AttentionRefine(PROMPTS, pipe.tokenizer, STEPS, 0.8, 0.4, device=DEV)
    register_attention_control(pipe, c)
    pipe.scheduler.set_timesteps(STEPS)
    hw = pipe.cfg.sample_size
    loop = FusedDenoiser(pipe, ctx, 2, (hw, hw), 7.5, use_graph=False)
    try:
        assert loop.shared and loop.lat_in is loop.lat, "the loop keeps no CFG batch buffer: nothing to copy the latents into"
        loop.start(x_T.to(DEV))
        loop.step_once()
        hip.profile_begin()
        loop.step_once()
        names = [r[0] for r in hip.profile_end()]
    finally:
        loop.release()
        unregister_attention_control(pipe, c)
    assert names[0] == "conv_in_f32_kernel<planes>", names[:3]
    assert not [n for n in names if "x3_split_act" in n], "conv_in writes its planes: no splitter launch in the step"
    assert names.count("repeat_batch_kernel") == 1
    cut = names.index("repeat_batch_kernel")
    cross = next(i for i, n in enumerate(names) if n.startswith("attn_cross_p2p_x3_kernel"))
    shaped = lambda ns: [n for n in ns if re.search(r" \d+x\d+x\d+ s\d+", n)]
    rows = lambda n: int(re.search(r" (\d+)x\d+x\d+ s\d+", n).group(1))
    print("prefix launches:", names[:cross + 2])
    # conv1, conv2 of resnets[0]; proj_in, q|k|v, to_out, to_q: all at Bp * 32 * 32 rows, the repeat launch among them (its
    # outputs are first read by the cross-attention's to_out)
    pre = shaped(names[:cross])
    assert cut < cross and len(pre) == 6 and all(rows(n) == 2 * hw * hw for n in pre), pre
    assert sum("attn_flash_x3p_kernel<40>" in n for n in names[:cross]) == 1, "the 32 x 32 self-attention runs once, at Bp rows"
    assert names[cross].startswith("attn_cross_p2p_x3_kernel<40>") and rows(shaped(names[cross:])[0]) == 4 * hw * hw
