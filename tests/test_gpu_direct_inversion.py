"""Direct Inversion on a real MI355X: the rectifying CFG + DDIM step (`ief_cfg_ddim_step_rect_f32`), the captured edit loop that
moves its source row back onto the stored DDIM inversion trajectory after every step, the samplers and the CLIs.

The rule (`p2p/inversion/direct.py`): after edit step i, row 0 is x'' = x' + (z - x') with z = z*_{S-1-i}, both operations rounded
in fp32; every other row is x'.  Stated checks (every test prints what it measured):
    rows >= 1 and x0_out                     bit-equal to `ief_cfg_ddim_step_f32` on the same inputs
    row 0                                    bit-equal to torch's xp[0] + (traj[r] - xp[0]) (fp32, on the device) with xp the plain
                                             entry point's output, and within 2^-23 (|z| + |xp|) of traj[r] elementwise -- the bound
                                             that follows from two correctly rounded operations:
                                             d = fl(z - xp) has |d - (z - xp)| <= 2^-24 |z - xp| <= 2^-24 (|z| + |xp|), and
                                             fl(xp + d) adds at most 2^-24 |xp + d| <= 2^-24 (|z| + 2^-24 (|z| + |xp|))
    captured loop / eager stepping / the rule written out with torch on a loop WITHOUT a trajectory: bit for bit
    the source row of an edit without a trajectory is at least 100 x farther from z*_0 than the rectified one
    a re-pointed pooled loop, edit_many, --invert_batch / --in_flight: bit for bit / the same pixels
Measured on an MI355X: kernel rows at most 0.998 of the bound; `small`, f16x3, 4 steps, guidance 7.5: the rectified source row ends
exactly on z*_0 (P2P and MasaCtrl), the plain edit's 4.6 away = 5.2e6 bounds; per-step rows with a lowered LocalBlend at most 0.884
of the bound, on the eager sampler path 0.895; decoded source image 0 grey levels from latent2image(z*_0).
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip  # noqa: E402
from _procs import run_parallel  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "image-editing-framework_amd")
EPS = 2.0 ** -23
IEF_EINVAL, IEF_ESHAPE = -1, -2          # csrc/ief_common.h
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]
STEPS, GUIDANCE = 4, 7.5


def within_bound(got, z, xp):
    """max over the elements of |got - z| / (2^-23 (|z| + |xp|)): <= 1 is the stated bound"""
    got, z, xp = got.double().cpu(), z.double().cpu(), xp.double().cpu()
    bound = EPS * (z.abs() + xp.abs())
    assert ((got - z).abs() <= bound).all(), f"worst |x'' - z| / bound = {((got - z).abs() / bound.clamp_min(1e-300)).max().item():.3f}"
    return ((got - z).abs() / bound.clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------------------------------------------------- the kernel
def kernel_inputs(Bp, row_elems, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    eu, ec, x = r(Bp, row_elems), r(Bp, row_elems), r(Bp, row_elems)
    traj = torch.stack([r(row_elems), 1e-3 * r(row_elems), 50 * r(row_elems)])          # three rows, three scales
    coef = torch.tensor([0.55, 0.71, GUIDANCE, 0.0])
    return [t.to(DEV) for t in (eu, ec, x, traj, coef)]


@pytest.mark.parametrize("Bp", [2, 3])
@pytest.mark.parametrize("row_elems", [256, 252, 16384])
def test_rect_step_kernel(Bp, row_elems):
    eu, ec, x, traj, coef = kernel_inputs(Bp, row_elems, 17 * Bp + row_elems)
    worst = 0.0
    for cfg in (True, False):
        u = eu if cfg else None
        x0p = torch.empty_like(x)
        xp = hip.cfg_ddim_step(u, ec, x, coef, x0_out=x0p)
        for s, r in ((0, 0), (1, 1), (2, 2), (7, 2), (-1, 0)):
            step = torch.tensor([s], dtype=torch.int32, device=DEV)
            x0r = torch.full_like(x, float("nan"))
            out = hip.cfg_ddim_step(u, ec, x, coef, out=torch.full_like(x, float("nan")), x0_out=x0r, rect=(traj, step))
            torch.cuda.synchronize()
            assert torch.equal(out[1:], xp[1:]), f"rows >= 1 must be the plain step's (cfg={cfg}, step={s})"
            assert torch.equal(x0r, x0p), "x0_out is the un-rectified x0 prediction of the plain step"
            want = xp[0] + (traj[r] - xp[0])
            assert torch.equal(out[0], want), f"row 0 must be xp + (z - xp), row {r} of the trajectory (cfg={cfg}, step={s})"
            worst = max(worst, within_bound(out[0], traj[r], xp[0]))
            xc = x.clone()
            assert hip.cfg_ddim_step(u, ec, xc, coef, out=xc, rect=(traj, step)) is xc
            assert torch.equal(xc, out), "in place == out of place"
            assert int(step.item()) == s, "the kernel only reads the step"
            no_x0 = hip.cfg_ddim_step(u, ec, x, coef, rect=(traj, step))
            assert torch.equal(no_x0, out)
    print(f"rect step Bp={Bp} row_elems={row_elems}: worst |x'' - z| / (2^-23 (|z| + |xp|)) = {worst:.3f} (bound 1)")


def test_rect_step_refusals_launch_nothing():
    lib = hip.load()
    eu, ec, x, traj, coef = kernel_inputs(2, 256, 5)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, x0 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    p = lambda t: t.data_ptr()
    good = dict(eps_u=p(eu), eps_c=p(ec), x=p(x), x_out=p(out), x0_out=p(x0), coef=p(coef), n=x.numel(), row_elems=256,
                traj=p(traj), traj_rows=3, step=p(step))

    def call(**kw):
        a = dict(good, **kw)
        return lib.ief_cfg_ddim_step_rect_f32(a["eps_u"], a["eps_c"], a["x"], a["x_out"], a["x0_out"], a["coef"], a["n"], a["row_elems"],
                                              a["traj"], a["traj_rows"], a["step"], torch.cuda.current_stream().cuda_stream)

    for name in ("eps_c", "x", "x_out", "coef", "traj", "step"):
        assert call(**{name: None}) == IEF_EINVAL, name
    for kw in (dict(n=0), dict(n=-512), dict(row_elems=0), dict(row_elems=-256), dict(row_elems=200), dict(traj_rows=0),
               dict(traj_rows=-1)):
        assert call(**kw) == IEF_ESHAPE, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(x0).all(), "a refused call must not launch"
    # the binding's own checks, in front of the library
    with pytest.raises(ValueError):
        hip.cfg_ddim_step(eu, ec, x, coef, rect=(traj[:, :128].contiguous(), step))
    with pytest.raises(TypeError):
        hip.cfg_ddim_step(eu, ec, x, coef, rect=(traj, step.long()))
    with pytest.raises(TypeError):
        hip.cfg_ddim_step(eu, ec, x, coef, rect=(traj.double(), step))
    assert call() == 0 and call(eps_u=None, x0_out=None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------------- the P2P sampler
def invert(pipe, seed, prompt=PROMPTS[0], steps=STEPS):
    """the `steps`-step DDIM inversion of a seeded latent -> (z*_0 [1,4,s,s], x_T, trajectory [steps,4,s,s])"""
    from ief_amd.p2p.inversion.direct import DirectInversion
    s = pipe.cfg.sample_size
    z0 = torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(seed)).to(DEV)
    pipe.scheduler.set_timesteps(steps)
    inv = DirectInversion()
    latents, _ = inv.ddim_inversion_loop(pipe, z0, [prompt])
    assert len(latents) == steps + 1 and torch.equal(latents[0], z0)
    traj = inv.trajectory(latents)
    assert traj.shape == (steps, 4, s, s) and torch.equal(traj[-1], z0[0]) and torch.equal(traj[0], latents[-2][0])
    return z0, latents[-1].clone(), traj


def p2p_context(pipe):
    from ief_amd.p2p.model.sd_utils import _encode_prompts
    with torch.no_grad():
        u, c = _encode_prompts(pipe, PROMPTS)
    return torch.cat([u, c])


class P2PRuns:
    """the three ways to run one Prompt-to-Prompt edit with a rectified source row"""

    def __init__(self, pipe, blend=None, guidance=GUIDANCE):
        from ief_amd.p2p.model.sd_utils import P2P
        self.pipe, self.blend, self.guidance = pipe, blend, guidance
        self.editor = P2P(pipe, STEPS)
        self.context = p2p_context(pipe)
        self.hw = (pipe.cfg.sample_size,) * 2

    def controller(self):
        from ief_amd.p2p.model.attention_control import AttentionRefine
        from ief_amd.p2p.model.ptp_utils import LocalBlend
        lb = None if self.blend is None else LocalBlend(self.pipe.tokenizer, PROMPTS, self.blend[0], threshold=self.blend[1], device=DEV)
        return AttentionRefine(PROMPTS, self.pipe.tokenizer, STEPS, 0.8, 0.4, local_blend=lb, device=DEV)

    def sampler(self, x_T, traj):
        """`P2P.text2image_ldm_stable`: the captured loop"""
        from ief_amd.p2p.model.register import unregister_attention_control as unreg
        c = self.controller()
        lat, _ = self.editor.text2image_ldm_stable(self.pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=self.guidance,
                                                   latent=x_T.clone(), return_latents=True, source_trajectory=traj)
        plan = self.pipe.unet._plan
        assert plan is not None and plan.kind == "p2p" and c.cur_step == STEPS and (plan.blend_w is not None) == (self.blend is not None)
        unreg(self.pipe, c)
        return lat.float().cpu()

    def loop(self, x_T, traj, use_graph, pooled=False, manual=None, after_step=None):
        """a `FusedDenoiser` under the lowered plan.  manual: the trajectory applied BY THE TEST with torch after every `step_once()`
        of a loop that has none -- the rule without the new kernel (the un-rectified x'[0] of every step is kept as `loop.seen`);
        after_step(i, loop) is called after step i"""
        from ief_amd import denoise
        from ief_amd.p2p.model.register import register_attention_control, unregister_attention_control as unreg
        c = self.controller()
        register_attention_control(self.pipe, c, fused=True)
        self.pipe.scheduler.set_timesteps(STEPS)
        if pooled:
            loop = denoise.acquire(self.pipe, self.context, 2, self.hw, self.guidance, use_graph=True, source_trajectory=traj)
        else:
            loop = denoise.FusedDenoiser(self.pipe, self.context, 2, self.hw, self.guidance, use_graph=use_graph, source_trajectory=traj)
        loop.seen = []
        try:
            loop.start(x_T.clone())
            for i in range(STEPS):
                loop.step_once()
                if manual is not None:
                    xp = loop.lat[0].clone()
                    loop.seen.append(xp)
                    loop.lat[0] = xp + (manual[i] - xp)
                if after_step is not None:
                    after_step(i, loop)
            lat = loop.result().float().cpu()
        finally:
            loop.release()
            unreg(self.pipe, c)
        assert c.cur_step == STEPS
        return lat, loop


@pytest.fixture(scope="module")
def small_x3():
    from ief_amd.pipeline import StableDiffusionPipeline
    return StableDiffusionPipeline.from_pretrained("synthetic:small", keep_state_dict=True, precision="f16x3")


@pytest.fixture(scope="module")
def small_inversions(small_x3):
    """two images' inversions, computed once and left unchanged"""
    return invert(small_x3, 8888), invert(small_x3, 4242)


def farther_factor(plain0, rect0, z0, xp0):
    """how many times farther from z*_0 the un-rectified source row is; a rectified row that hits z*_0 exactly counts as being
    the bound away"""
    e_plain = (plain0.double() - z0.double().cpu()).abs().max().item()
    floor = (EPS * (z0.double().abs() + xp0.double().abs())).max().item()
    e_rect = (rect0.double() - z0.double().cpu()).abs().max().item()
    return e_plain / max(e_rect, floor), e_plain, e_rect


def test_p2p_sampler_graph_eager_rule_bound_and_distance(small_x3, small_inversions):
    from ief_amd import denoise
    pipe = small_x3
    (z0, x_T, traj), _ = small_inversions
    runs = P2PRuns(pipe)
    denoise.drop_pool()
    graph = runs.sampler(x_T, traj)
    eager, _ = runs.loop(x_T, traj, use_graph=False)
    rule, rule_loop = runs.loop(x_T, None, use_graph=False, manual=traj)
    seen = rule_loop.seen                       # x'[0] of every step, before the test's own rectification
    assert torch.equal(graph, eager), "the captured loop must equal eager stepping bit for bit"
    assert torch.equal(graph, rule), "both must equal step_once() + torch's x' + (z - x') on a loop without a trajectory"
    plain = runs.sampler(x_T, None)

    worst = within_bound(graph[0], z0[0], seen[-1])
    factor, e_plain, e_rect = farther_factor(plain[0], graph[0], z0[0], seen[-1])
    moved = ((graph[1] - plain[1]).abs().max() / plain[1].abs().max()).item()
    print(f"P2P small f16x3, {STEPS} steps, guidance {GUIDANCE}: source row vs z*_0: |x'' - z| / bound {worst:.3f} (bound 1); max |.| "
          f"{e_rect:.3e} rectified, {e_plain:.3e} without a trajectory: {factor:.3e} x farther (floor 100); the target row moves by "
          f"{moved:.3e} of its size")
    assert factor >= 100
    assert not torch.equal(graph[1], plain[1]), "the target row reads the rectified source row's maps"

    # the decoded source image is the decoded z*_0 within one grey level
    img = runs.editor.latent2image(pipe.vae, graph[:1].to(DEV)).astype(int)
    ref = runs.editor.latent2image(pipe.vae, z0).astype(int)
    print(f"decoded source image vs latent2image(z*_0): max {np.abs(img - ref).max()} grey levels (bound 1)")
    assert img.shape == ref.shape and np.abs(img - ref).max() <= 1
    denoise.drop_pool()


def test_p2p_pooled_loop_repointed_and_edit_many(small_x3, small_inversions):
    from ief_amd import denoise
    from ief_amd.p2p.model.register import unregister_attention_control as unreg
    pipe = small_x3
    (z0a, x_Ta, traja), (z0b, x_Tb, trajb) = small_inversions
    runs = P2PRuns(pipe)
    denoise.drop_pool()
    fresh_b, _ = runs.loop(x_Tb, trajb, use_graph=True)                 # never pooled: its own capture
    first, loop1 = runs.loop(x_Ta, traja, use_graph=True, pooled=True)
    second, loop2 = runs.loop(x_Tb, trajb, use_graph=True, pooled=True)
    assert loop2 is loop1 and loop2.graph is not None, "equal signatures: the captured loop is taken from the pool, not rebuilt"
    assert not torch.equal(first, second)
    assert torch.equal(second, fresh_b), "a pooled loop re-pointed at the second image's trajectory must give that image's fresh run"
    assert not torch.equal(traja, trajb) and torch.equal(loop2.traj.cpu(), trajb.cpu()) and loop2.traj.data_ptr() == loop1.traj.data_ptr()
    # a loop without a trajectory is another pool entry, and the reverse
    none, loop3 = runs.loop(x_Ta, None, use_graph=True, pooled=True)
    assert loop3 is not loop1 and loop3.traj is None
    with pytest.raises(ValueError):
        loop3.rebind(runs.context, GUIDANCE, None, None, traja)
    again, loop4 = runs.loop(x_Ta, traja, use_graph=True, pooled=True)
    assert loop4 is loop1 and torch.equal(again, first)
    denoise.drop_pool()

    # edit_many with two jobs == one call per job
    jobs = [(PROMPTS, runs.controller(), x_Ta.clone(), None, traja), (PROMPTS, runs.controller(), x_Tb.clone(), None, trajb)]
    many = runs.editor.edit_many(pipe, jobs, num_inference_steps=STEPS, guidance_scale=GUIDANCE)
    for (img, _), (x_T, traj) in zip(many, ((x_Ta, traja), (x_Tb, trajb))):
        c = runs.controller()
        one, _ = runs.editor.text2image_ldm_stable(pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=GUIDANCE,
                                                   latent=x_T.clone(), source_trajectory=traj)
        unreg(pipe, c)
        assert (img == one).all(), "edit_many must give what one call per job gives"
    with pytest.raises(ValueError):
        runs.editor.edit_many(pipe, [(PROMPTS, runs.controller(), x_Ta.clone(), [torch.zeros(1, 77, 8)] * STEPS, traja)],
                              num_inference_steps=STEPS, guidance_scale=GUIDANCE)
    unreg(pipe, None)
    denoise.drop_pool()


@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_p2p_graph_eager_and_rule_on_tiny(precision):
    from ief_amd import denoise
    from ief_amd.pipeline import StableDiffusionPipeline
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", precision=precision)
    z0, x_T, traj = invert(pipe, 8888)
    runs = P2PRuns(pipe)
    denoise.drop_pool()
    graph = runs.sampler(x_T, traj)
    eager, _ = runs.loop(x_T, traj, use_graph=False)
    rule, _ = runs.loop(x_T, None, use_graph=False, manual=traj)
    assert torch.equal(graph, eager), "the captured loop must equal eager stepping bit for bit"
    assert torch.equal(graph, rule), "both must equal step_once() + torch's x' + (z - x') on a loop without a trajectory"
    assert not torch.equal(graph, runs.sampler(x_T, None))
    denoise.drop_pool()


def test_eager_sampler_path_applies_the_same_kernel(small_x3, small_inversions, monkeypatch):
    """a controller on the generic path (lowering goes by class name) steps eagerly through `P2P.diffusion_step`: the source row is
    rectified there too, by the same kernel with a host step index.  The test wraps `hip.cfg_ddim_step` to see every call: it
    computes the plain step of the same inputs next to it, which is the x' of the bound"""
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.register import unregister_attention_control as unreg
    from ief_amd.p2p.model.sd_utils import P2P

    class RefineOnTheGenericPath(AttentionRefine):
        pass

    pipe = small_x3
    (z0, x_T, traj), _ = small_inversions
    editor = P2P(pipe, STEPS)
    real, calls = hip.cfg_ddim_step, []

    def spy(eps_u, eps_c, x, coef, out=None, x0_out=None, rect=None):
        got = real(eps_u, eps_c, x, coef, out=out, x0_out=x0_out, rect=rect)
        if rect is not None:
            assert out is None
            calls.append((int(rect[1].item()), real(eps_u, eps_c, x, coef), got.clone()))
        return got

    monkeypatch.setattr(hip, "cfg_ddim_step", spy)
    out = {}
    for t in (traj, None):
        c = RefineOnTheGenericPath(PROMPTS, pipe.tokenizer, STEPS, 0.8, 0.4, device=DEV)
        lat, _ = editor.text2image_ldm_stable(pipe, PROMPTS, c, num_inference_steps=STEPS, guidance_scale=GUIDANCE,
                                              latent=x_T.clone(), return_latents=True, source_trajectory=t)
        assert pipe.unet._plan is None and c.cur_step == STEPS
        unreg(pipe, c)
        out[t is None] = lat.float().cpu()
    assert [s for s, _, _ in calls] == list(range(STEPS)), "one rectifying launch per step, with the host's step index"
    worst = 0.0
    for s, xp, got in calls:
        assert torch.equal(got[1:], xp[1:]) and torch.equal(got[0], xp[0] + (traj[s] - xp[0]))
        worst = max(worst, within_bound(got[0], traj[s], xp[0]))
    assert torch.equal(out[False], calls[-1][2].float().cpu())
    factor, e_plain, e_rect = farther_factor(out[True][0], out[False][0], z0[0], calls[-1][1][0])
    print(f"eager sampler, generic controller: row 0 vs the trajectory after every step, worst |x'' - z| / bound {worst:.3f} (bound 1); "
          f"final source row vs z*_0 max |.| {e_rect:.3e} rectified, {e_plain:.3e} without: {factor:.3e} x farther (floor 100)")
    assert factor >= 100


# ------------------------------------------------------------------------------------------------------------- with a LocalBlend
WORDS, THRES = [["house"], ["fall"]], 0.9905          # tests/test_gpu_local_blend.py: the threshold at which `small`'s flat maps split


def test_lowered_local_blend_runs_after_the_rectification(small_x3, small_inversions):
    pipe = small_x3
    (z0, x_T, traj), _ = small_inversions
    runs = P2PRuns(pipe, blend=(WORDS, THRES))
    plain = P2PRuns(pipe)
    # row 0 never reads another row and the blend leaves it alone: the un-rectified x'[0] of every step is that of the edit
    # without a blend, taken from the rule loop
    from ief_amd import denoise
    rule, rule_loop = plain.loop(x_T, None, use_graph=False, manual=traj)
    xps = rule_loop.seen

    worst = []

    def check(i, loop):
        worst.append(within_bound(loop.lat[0], traj[i], xps[i]))

    eager, _ = runs.loop(x_T, traj, use_graph=False, after_step=check)
    assert len(worst) == STEPS
    denoise.drop_pool()
    graph, _ = runs.loop(x_T, traj, use_graph=True, after_step=check)
    assert len(worst) == 2 * STEPS
    assert torch.equal(graph, eager), "captured-graph replay must equal eager stepping bit for bit"
    assert torch.equal(graph, runs.sampler(x_T, traj))
    assert torch.equal(graph[0], rule[0]), "the blend leaves the rectified source row alone"
    moved = ((graph[1] - rule[1]).abs().max() / rule[1].abs().max()).item()
    print(f"with a lowered LocalBlend: row 0 vs the trajectory after every step, worst |x'' - z| / bound {max(worst):.3f} (bound 1); "
          f"the blend moves the target row by {moved:.3e} of its size")
    assert not torch.equal(graph[1], rule[1]), "the blend must act on the target row"
    denoise.drop_pool()


# ------------------------------------------------------------------------------------------------------------- MasaCtrl
def test_masactrl_sampler_graph_eager_rule_bound_and_distance(small_x3, small_inversions):
    from ief_amd import denoise
    from ief_amd.masactrl.model.attention_control import MutualSelfAttentionControl
    from ief_amd.masactrl.model.register import regiter_attention_editor_diffusers, unregister_attention_control as unreg
    from ief_amd.masactrl.model.sd_utils import MasaCtrl
    pipe = small_x3
    (z0, x_T, traj), _ = small_inversions
    cfg = pipe.cfg
    size, hw = cfg.sample_size * 8, (cfg.sample_size,) * 2
    start = torch.cat([x_T, x_T])
    editor = MasaCtrl(pipe, STEPS)
    make = lambda: MutualSelfAttentionControl(1, 2, layer_idx=list(range(2, 11)), total_steps=STEPS)

    def sampler(t):
        c = make()
        regiter_attention_editor_diffusers(pipe, c)
        assert pipe.unet._plan is not None and pipe.unet._plan.kind == "masactrl"
        try:
            lat, _ = editor(prompt=PROMPTS, latents=start.clone(), guidance_scale=GUIDANCE, num_inference_steps=STEPS, height=size,
                            width=size, return_latents=True, source_trajectory=t)
        finally:
            unreg(pipe, c)
        assert c.cur_step == STEPS
        return lat.float().cpu()

    tok = pipe.tokenizer
    enc = lambda p: pipe.text_encoder(tok(p, padding="max_length", max_length=tok.model_max_length, return_tensors="pt").input_ids.to(DEV))[0]
    with torch.no_grad():
        context = torch.cat([enc([""] * 2), enc(PROMPTS)])

    def loop(t, manual=None):
        c = make()
        regiter_attention_editor_diffusers(pipe, c)
        pipe.scheduler.set_timesteps(STEPS)
        lp = denoise.FusedDenoiser(pipe, context, 2, hw, GUIDANCE, use_graph=False, source_trajectory=t)
        seen = []
        try:
            lp.start(start.clone())
            for i in range(STEPS):
                lp.step_once()
                if manual is not None:
                    xp = lp.lat[0].clone()
                    seen.append(xp)
                    lp.lat[0] = xp + (manual[i] - xp)
            lat = lp.result().float().cpu()
        finally:
            lp.release()
            unreg(pipe, c)
        return lat, seen

    denoise.drop_pool()
    graph = sampler(traj)
    eager, _ = loop(traj)
    rule, seen = loop(None, manual=traj)
    assert torch.equal(graph, eager), "the captured loop must equal eager stepping bit for bit"
    assert torch.equal(graph, rule), "both must equal step_once() + torch's x' + (z - x') on a loop without a trajectory"
    plain = sampler(None)
    worst = within_bound(graph[0], z0[0], seen[-1])
    factor, e_plain, e_rect = farther_factor(plain[0], graph[0], z0[0], seen[-1])
    print(f"MasaCtrl small f16x3, {STEPS} steps, guidance {GUIDANCE}: source row vs z*_0: |x'' - z| / bound {worst:.3f} (bound 1); max |.| "
          f"{e_rect:.3e} rectified, {e_plain:.3e} without a trajectory: {factor:.3e} x farther (floor 100)")
    assert factor >= 100
    with pytest.raises(ValueError):
        editor(prompt=PROMPTS, latents=start.clone(), guidance_scale=GUIDANCE, num_inference_steps=STEPS, height=size, width=size,
               source_trajectory=traj, uncond_embeddings_list=[context[:1]] * STEPS)
    denoise.drop_pool()


# ------------------------------------------------------------------------------------------------------------- the CLIs
def _jpg(path):
    rng = np.random.RandomState(0)
    Image.fromarray(np.kron(rng.randint(0, 255, (8, 8, 3)), np.ones((16, 16, 1))).astype(np.uint8)).save(path)


@pytest.mark.parametrize("folder", ["p2p", "masactrl"])
def test_edit_real_cli_direct(tmp_path, folder):
    _jpg(tmp_path / "test.jpg")
    run_parallel([([os.path.join(PKG, folder, "edit_real.py"), "--sd_version", "tiny", "--inversion_type", "direct", "--source_image",
                    str(tmp_path / "test.jpg")], tmp_path)])
    pngs = {n: np.array(Image.open(tmp_path / "exp" / n)).astype(int) for n in ("source.png", "inversion.png", "edit.png")}
    assert pngs["source.png"].shape == pngs["inversion.png"].shape == pngs["edit.png"].shape
    assert np.abs(pngs["inversion.png"] - pngs["edit.png"]).max() > 0


def test_pie_driver_direct_batched_in_flight_matches_per_image(tmp_path):
    script = os.path.join(PKG, "p2p", "test.py")
    base = ["--sd_version", "tiny", "--synthetic", "2", "--inversion_type", "direct"]
    a, b = tmp_path / "a", tmp_path / "b"
    one, many = run_parallel([([script] + base + ["--exp_path", str(a)], tmp_path / "cwd_a"),
                              ([script] + base + ["--invert_batch", "2", "--in_flight", "2", "--exp_path", str(b)], tmp_path / "cwd_b")])
    assert one.last_json()["images"] == 2 and many.last_json()["images"] == 2
    dirs = sorted(x for x in os.listdir(a) if x.startswith("syn_"))
    assert len(dirs) == 2 and sorted(x for x in os.listdir(b) if x.startswith("syn_")) == dirs
    for d in dirs:
        for name in ("inversion.png", "edit.png"):
            pa, pb = np.array(Image.open(a / d / name)).astype(int), np.array(Image.open(b / d / name)).astype(int)
            assert pa.shape == pb.shape and np.abs(pa - pb).max() == 0, (d, name, np.abs(pa - pb).max())


def test_edit_real_cli_direct_smallxl(tmp_path):
    _jpg(tmp_path / "test.jpg")
    run_parallel([([os.path.join(PKG, "p2p", "edit_real.py"), "--sd_version", "smallxl", "--inversion_type", "direct", "--source_image",
                    str(tmp_path / "test.jpg")], tmp_path)])
    for n in ("source.png", "inversion.png", "edit.png"):
        assert (tmp_path / "exp" / n).exists()
