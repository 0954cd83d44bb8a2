"""The denoising / inversion hot loop as ONE captured hipGraph replayed once per step.

One step of the reference's loop (`/root/reference/p2p/model/sd_utils.py:67-79`) is
    cat([latents]*2) -> UNet -> chunk -> CFG -> scheduler.step -> controller.step_callback
and one inversion step (`/root/reference/p2p/inversion/ddim.py:27-31`) is UNet (cond only) ->
`ddim_reverse`.  Eagerly that is ~430 kernel launches per step driven from Python; the launch
overhead would exceed the GPU time.  Here the whole step is captured once:

    select_step(time-embedding row)  select_step(DDIM coefficients)     <- read a DEVICE step counter
    [P2P plan: select_step(gate coefficients), select_step(self-replace sources)]
    latents -> CFG batch copy -> UNet (fused attention control) -> fused CFG + DDIM update (in place)
    [Direct Inversion: the same launch moves the source row (row 0) back onto the stored inversion trajectory]
    [edit-friendly DDPM inversion: CFG with a scale per batch row + the eta = 1 update with the stored noise map of this step instead]
    [DiffEdit: the same launch puts every row back onto the stored inversion trajectory outside that row's edit mask]
    [LEDITS++: the batch is [uncond | concept_1 .. concept_E] on ONE latent; after the UNet the implicit masks (two one-workgroup
     launches) and the masked multi-concept guidance + eta = 1 update with this step's stored noise map]
    [proximal guidance on a negative-prompt-inversion edit: the per-row quantile of |eps_c - eps_u| (one workgroup per row), then the
     thresholded guidance, the update and the pull of x0 towards the encoded source outside the dilated edit mask in one launch]
    [P2P plan with a LocalBlend: the word-masked blend of the updated latents, in place]
    advance_step
(on the f16x3 planes trunk the UNet takes the latents themselves and runs what both halves of the CFG batch share once: no copy;
`cfg_shared_prefix_reason`)

so a 50-step edit is 50 graph replays with no host work in between; everything that varies
with the step is a per-step table row selected on the device.  Static buffers: latents (fp32
NCHW), the CFG batch, the fp16 context (per-step rows when null-text embeddings are supplied).
"""
import logging
import os
from typing import Dict, List, Optional

import torch

from . import hip

# Captured step graphs are kept and RE-USED for the next image of the same shape (`acquire` / `release`): capturing
# costs an eager warm-up step plus the capture pass (tens of ms, ~10 % of a 50-step edit) and, with several images
# in flight, is the serial part of the schedule.  IEF_REUSE_GRAPHS=0 captures afresh for every loop.
REUSE_GRAPHS = os.environ.get("IEF_REUSE_GRAPHS", "1") == "1"
_POOL: Dict[tuple, list] = {}
_POOL_CAP = 8

# A CFG step feeds the UNet cat([latents] * 2) (`/root/reference/p2p/model/sd_utils.py:72`) and ONE time-embedding row: rows b and
# b + Bp are bit-identical until the first launch that reads the context, the cross-attention of down_blocks[0].attentions[0].
# Where nothing else tells the halves apart (`cfg_shared_prefix_reason`) that prefix -- conv_in, the first resnet, the first
# transformer's GroupNorm, proj_in, LayerNorm 1, q|k|v, the 64 x 64 self-attention, to_out, LayerNorm 2, the cross-attention's
# to_q -- runs once, at Bp rows.  IEF_CFG_SHARED_PREFIX=0: every loop builds the CFG batch and runs it whole (A/B runs).
CFG_SHARED_PREFIX = os.environ.get("IEF_CFG_SHARED_PREFIX", "1") == "1"
_log = logging.getLogger("ief_amd.denoise")
_said = set()


def cfg_shared_prefix_reason(*, mode, cfg, x3p, aug, first_block_cross, native, fused_cross, ln_folded, plan_on_first_self,
                             taps=False, enabled=True, ledits=False):
    """None where a CFG denoising step may run the prefix its two halves share once (at Bp rows), else the reason why not -- a pure
    function of host-side facts (`UNet2DConditionModel.cfg_shared_facts` collects the model's):
      mode / cfg          the loop is `denoise` with classifier-free guidance (inversion and the no-CFG loops have no second half)
      x3p                 the trunk runs on f16x3 operand planes (the only trunk with the seam)
      aug                 SDXL's additional embedding gives every batch row its own time-embedding row: the halves differ from conv_in on
      first_block_cross   down_blocks[0] has transformers (SDXL's does not: nothing to share before the first context read)
      native              no hook owns an attention module of down_blocks[0] (a Python controller sees, and may edit, every row)
      fused_cross         the first cross-attention takes the fused split-operand kernel, the one launch with Q batch-row indirection
      ln_folded           IEF_X3P_FOLD_LN=1 (an A/B form of the transformer blocks that has no seam)
      plan_on_first_self  the control plan redirects rows of the first self-attention in some step (`ControlPlan.controls_first_self`)
      taps                a debugging forward that records intermediate tensors at full batch
      enabled             IEF_CFG_SHARED_PREFIX
      ledits              a LEDITS++ loop: 1 + E rows on one latent, not two halves (widening the prefix to them is out of scope)"""
    if ledits:
        return "the LEDITS++ batch is [uncond | concepts] on one latent, not two halves"
    if not enabled:
        return "switched off (IEF_CFG_SHARED_PREFIX=0)"
    if mode != "denoise" or not cfg:
        return "not a classifier-free-guidance denoising loop"
    if not x3p:
        return "the trunk does not run on f16x3 operand planes"
    if aug:
        return "the additional (text-time) embedding differs between the halves of the batch"
    if not first_block_cross:
        return "down_blocks[0] has no cross-attention"
    if not native:
        return "an attention module of down_blocks[0] is on the generic (hooked) path"
    if not fused_cross:
        return "the first cross-attention does not take the fused split-operand kernel"
    if ln_folded:
        return "the transformer LayerNorms are folded (IEF_X3P_FOLD_LN=1)"
    if taps:
        return "intermediate tensors are tapped"
    if plan_on_first_self:
        return "the control plan acts on the self-attention of the first transformer"
    return None


def _check_finite(lat, unet):
    """one host sync per finished loop: the fp16-operand modes ("f16", "f16x3") represent operand elements up to 65504; an
    activation beyond that becomes inf in its hi half and the output NaN -- say so instead of handing NaN images on"""
    if not bool(torch.isfinite(lat).all()):
        mode = getattr(unet, "precision", "f16")
        hint = ("an operand left the fp16 range (|x| > 65504): run this model with precision=\"f32\" (IEF_PRECISION=f32 / --precision f32), "
                "the fp32-input MFMA has the fp32 range" if mode != "f32" else "check the inputs / weights")
        raise FloatingPointError(f"non-finite latents after the denoising loop (precision={mode}): {hint}")


def check_source_trajectory(traj, *, mode, cfg, uncond_list, row_shape, num_steps):
    """the argument checks of a Direct Inversion loop (host-side facts only; raises ValueError): `traj` is fp32 [S, C, h, w] with
    row i = z*_{S-1-i}, the latent the SOURCE row must hold after edit step i"""
    if mode != "denoise":
        raise ValueError(f"source_trajectory: only a denoising loop rectifies its source row (mode={mode!r})")
    if not cfg:
        raise ValueError("source_trajectory: Direct Inversion rectifies the source row of a classifier-free-guidance edit; "
                         "without guidance the cond-only inversion is already reproduced")
    if uncond_list is not None:
        raise ValueError("source_trajectory together with uncond_list: choose Direct Inversion or null-text embeddings, not both")
    if not isinstance(traj, torch.Tensor) or traj.dtype != torch.float32:
        raise ValueError("source_trajectory: expected one fp32 tensor [steps, C, h, w]")
    if tuple(traj.shape[1:]) != tuple(row_shape) or traj.dim() != 1 + len(row_shape):
        raise ValueError(f"source_trajectory: rows of shape {tuple(traj.shape[1:])} for latents of shape {tuple(row_shape)}")
    if traj.shape[0] != num_steps:
        raise ValueError(f"source_trajectory: {traj.shape[0]} rows for a schedule of {num_steps} steps")


def guidance_rows(guidance_scale, num_latents):
    """one guidance scale per batch row: a number serves every row, a sequence brings one each (ValueError otherwise)"""
    if isinstance(guidance_scale, (int, float)):
        return [float(guidance_scale)] * num_latents
    try:
        rows = [float(g) for g in guidance_scale]
    except TypeError:
        raise ValueError("noise_maps: guidance_scale is one number or a sequence of one number per prompt") from None
    if len(rows) != num_latents:
        raise ValueError(f"noise_maps: {len(rows)} guidance scales for {num_latents} batch rows")
    return rows


def check_noise_maps(maps, *, mode, cfg, uncond_list, source_trajectory, row_shape, num_steps, skip, guidance_scale=None,
                     num_latents=None):
    """the argument checks of an edit-friendly DDPM inversion loop (host-side facts only; raises ValueError): `maps` is fp32
    [S - skip, C, h, w], row i = the noise map z of edit step i, which runs timestep `timesteps[skip + i]` of the S-step schedule"""
    if mode != "denoise":
        raise ValueError(f"noise_maps: only a denoising loop adds stored noise (mode={mode!r})")
    if not cfg:
        raise ValueError("noise_maps: the maps were extracted under classifier-free guidance and the edit needs a guidance scale per "
                         "row; a loop without guidance has none")
    if uncond_list is not None:
        raise ValueError("noise_maps together with uncond_list: choose DDPM inversion or null-text embeddings, not both")
    if source_trajectory is not None:
        raise ValueError("noise_maps together with source_trajectory: choose DDPM inversion or Direct Inversion, not both")
    if not isinstance(skip, int) or isinstance(skip, bool) or not 0 <= skip < num_steps:
        raise ValueError(f"noise_maps: skip must be an integer in [0, {num_steps}), got {skip!r}")
    if not isinstance(maps, torch.Tensor) or maps.dtype != torch.float32:
        raise ValueError("noise_maps: expected one fp32 tensor [steps - skip, C, h, w]")
    if tuple(maps.shape[1:]) != tuple(row_shape) or maps.dim() != 1 + len(row_shape):
        raise ValueError(f"noise_maps: rows of shape {tuple(maps.shape[1:])} for latents of shape {tuple(row_shape)}")
    if maps.shape[0] != num_steps - skip:
        raise ValueError(f"noise_maps: {maps.shape[0]} rows for a schedule of {num_steps} steps with skip {skip} "
                         f"({num_steps - skip} edit steps)")
    if num_latents is not None:
        guidance_rows(guidance_scale, num_latents)


def check_solver_order(solver_order, noise_maps):
    """the solver order of a loop (raises ValueError): 1, or 2 for the second-order multistep SDE-DPM-Solver++, which steps on the
    noise maps of an edit-friendly DDPM inversion extracted at that order and exists only with them"""
    if isinstance(solver_order, bool) or solver_order not in (1, 2):
        raise ValueError(f"solver_order must be 1 or 2, got {solver_order!r}")
    if solver_order == 2 and noise_maps is None:
        raise ValueError("solver_order=2: the second-order solver steps on the noise maps of an edit-friendly DDPM inversion "
                         "(noise_maps=); every other loop is a DDIM loop")


def check_edit_mask(mask, *, mode, cfg, uncond_list, noise_maps, source_trajectory, row_shape, num_steps, skip, num_latents):
    """the argument checks of a DiffEdit loop (host-side facts only; raises ValueError): `mask` is fp32 or bool [Bp, h, w] (or
    [h, w], shared by every row), nonzero = edited; `source_trajectory` is fp32 [S - skip, C, h, w] with row i = z*_{S-skip-1-i}, the
    latent every row must hold OUTSIDE its mask after edit step i, which runs timestep `timesteps[skip + i]`"""
    if mode != "denoise":
        raise ValueError(f"edit_mask: only a denoising loop keeps its background on the inversion trajectory (mode={mode!r})")
    if not cfg:
        raise ValueError("edit_mask: DiffEdit decodes under classifier-free guidance; a loop without guidance has no masked step")
    if uncond_list is not None:
        raise ValueError("edit_mask together with uncond_list: choose DiffEdit or null-text embeddings, not both")
    if noise_maps is not None:
        raise ValueError("edit_mask together with noise_maps: choose DiffEdit or DDPM inversion, not both")
    if not isinstance(skip, int) or isinstance(skip, bool) or not 0 <= skip < num_steps:
        raise ValueError(f"edit_mask: skip must be an integer in [0, {num_steps}), got {skip!r}")
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.float32, torch.bool):
        raise ValueError("edit_mask: expected one fp32 or bool tensor [Bp, h, w] (or [h, w] for every row)")
    hw = tuple(row_shape[-2:])
    if tuple(mask.shape) not in (hw, (num_latents, *hw)):
        raise ValueError(f"edit_mask: shape {tuple(mask.shape)} for {num_latents} latents of {hw[0]} x {hw[1]}")
    if source_trajectory is None:
        raise ValueError("edit_mask: needs the source_trajectory the background is put back onto")
    if not isinstance(source_trajectory, torch.Tensor) or source_trajectory.dtype != torch.float32:
        raise ValueError("edit_mask: source_trajectory is one fp32 tensor [steps - skip, C, h, w]")
    if tuple(source_trajectory.shape[1:]) != tuple(row_shape) or source_trajectory.dim() != 1 + len(row_shape):
        raise ValueError(f"edit_mask: trajectory rows of shape {tuple(source_trajectory.shape[1:])} for latents of shape "
                         f"{tuple(row_shape)}")
    if source_trajectory.shape[0] != num_steps - skip:
        raise ValueError(f"edit_mask: {source_trajectory.shape[0]} trajectory rows for a schedule of {num_steps} steps with skip {skip} "
                         f"({num_steps - skip} edit steps)")


def check_ledits_loop(plan, *, unet_plan, mode, guidance_scale, uncond_list, source_trajectory, edit_mask, noise_maps, skip,
                      row_shape, num_steps, num_latents, context_rows, added_cond_kwargs=None):
    """the argument checks of a LEDITS++ loop (host-side facts only; raises ValueError): `plan` is the 'ledits' control plan
    registered on the UNet; the loop runs ONE latent at UNet batch 1 + E = [uncond | concepts] on the noise maps of an edit-friendly
    DDPM inversion, and the scales travel in the plan (`guidance_scale` stays None)"""
    from .control import check_ledits
    if getattr(plan, "kind", None) != "ledits":
        raise ValueError("ledits: expected the 'ledits' ControlPlan registered on the UNet")
    check_ledits(plan.led["E"], sdxl=added_cond_kwargs is not None, uncond_list=uncond_list, source_trajectory=source_trajectory,
                 edit_mask=edit_mask, controller=unet_plan is not plan)
    if guidance_scale is not None:
        raise ValueError("ledits: the guidance scales of the concepts travel in the plan; guidance_scale stays None")
    if noise_maps is None:
        raise ValueError("ledits: the edit runs on the noise maps of an edit-friendly DDPM inversion (noise_maps=)")
    check_noise_maps(noise_maps, mode=mode, cfg=True, uncond_list=None, source_trajectory=None, row_shape=row_shape,
                     num_steps=num_steps, skip=skip)
    if num_latents != 1:
        raise ValueError(f"ledits: ONE latent per loop, got {num_latents}")
    if context_rows != 1 + plan.led["E"]:
        raise ValueError(f"ledits: the context holds [uncond | {plan.led['E']} concepts] = {1 + plan.led['E']} rows, got {context_rows}")
    if plan.num_steps != num_steps - skip:
        raise ValueError(f"ledits: the plan's scale table covers {plan.num_steps} edit steps, the loop runs {num_steps - skip}")
    if tuple(row_shape[-2:]) != plan.led["hw"]:
        raise ValueError(f"ledits: the plan was lowered for latents of {plan.led['hw']}, the loop runs {tuple(row_shape[-2:])}")


class ProxGuidance:
    """The plan of proximal guidance on a negative-prompt-inversion edit (Han et al., "Improving Tuning-Free Real Image Editing with
    Proximal Guidance"): what a loop's two extra launches (`hip.prox_threshold`, `hip.cfg_ddim_step(prox=)`) need.
      mode      "l0" (hard) or "l1" (soft) thresholding of eps_c - eps_u at the row's quantile
      quantile  q in [0, 1]: the per-row quantile of |eps_c - eps_u|
      radius    0 .. 3: the Chebyshev dilation of the edit mask the inversion guidance spares
      prox_on   one 0 / 1 per edit step: threshold in this step
      eta       one number per edit step: the pull of the x0 prediction towards the encoded source outside the mask (0 = none)
    mode and radius are launch arguments, so they are part of a pooled loop's key; quantile and the two rows are table contents."""

    def __init__(self, mode, quantile, radius, prox_on, eta):
        if mode not in hip.PROX_MODES:
            raise ValueError(f"prox: mode is one of {sorted(hip.PROX_MODES)}, got {mode!r}")
        quantile = float(quantile)
        if not 0.0 <= quantile <= 1.0:
            raise ValueError(f"prox: the quantile lies in [0, 1], got {quantile!r}")
        if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= 3:
            raise ValueError(f"prox: the dilation radius is an integer in [0, 3], got {radius!r}")
        self.mode, self.quantile, self.radius = mode, quantile, radius
        self.prox_on = [1.0 if p else 0.0 for p in prox_on]
        self.eta = [float(e) for e in eta]
        if len(self.prox_on) != len(self.eta) or not self.eta:
            raise ValueError(f"prox: {len(self.prox_on)} prox_on entries and {len(self.eta)} eta entries (one each per edit step)")

    @classmethod
    def from_schedule(cls, timesteps, mode="l0", quantile=0.7, radius=1, prox_steps=None, recon_lr=1.0, recon_t=400):
        """the plan the command lines build: prox_on in the edit steps [A, B) of `prox_steps` (None: all), eta = recon_lr at the
        timesteps below recon_t and 0 elsewhere"""
        ts = [int(t) for t in timesteps]
        a, b = (0, len(ts)) if prox_steps is None else (int(prox_steps[0]), int(prox_steps[1]))
        if not 0 <= a <= b <= len(ts):
            raise ValueError(f"prox: prox_steps {a} {b} outside the {len(ts)} edit steps")
        return cls(mode, quantile, radius, [a <= i < b for i in range(len(ts))], [float(recon_lr) if t < recon_t else 0.0 for t in ts])

    def rank(self, row_elems):
        """fp32 [2] = [lo, frac] of the quantile over a row of row_elems values (`control.ledits_rank`, the pinned host rule)"""
        from .control import ledits_rank
        return torch.tensor(list(ledits_rank(self.quantile, row_elems)), dtype=torch.float32)


def check_prox(plan, *, mode, cfg, uncond_list, source_trajectory, noise_maps, edit_mask, ledits, added_cond_kwargs, local_blend,
               source_latent, row_shape, num_steps):
    """the argument checks of a loop under proximal guidance (host-side facts only; raises ValueError): `plan` is a `ProxGuidance`,
    `source_latent` the encoded source image, fp32 [C, h, w] (or [1, C, h, w])"""
    if not isinstance(plan, ProxGuidance):
        raise ValueError("prox: expected a ProxGuidance plan")
    for other, name, what in ((uncond_list, "uncond_list", "null-text embeddings"),
                              (source_trajectory, "source_trajectory", "Direct Inversion"),
                              (noise_maps, "noise_maps", "DDPM inversion"), (edit_mask, "edit_mask", "DiffEdit"),
                              (ledits, "ledits", "LEDITS++"), (added_cond_kwargs, "added_cond_kwargs", "SDXL"),
                              (local_blend, "LocalBlend", "a LocalBlend on the controller")):
        if other is not None and other is not False:
            raise ValueError(f"prox together with {name}: proximal guidance runs on a negative-prompt-inversion edit, not with {what}")
    if mode != "denoise" or not cfg:
        raise ValueError("prox together with a loop without guidance: proximal guidance thresholds eps_c - eps_u, which only a "
                         "classifier-free-guidance denoising loop forms")
    if not isinstance(source_latent, torch.Tensor) or source_latent.dtype != torch.float32:
        raise ValueError("prox: needs source_latent, the encoded source image as one fp32 tensor [C, h, w]")
    if tuple(source_latent.shape[-3:]) != tuple(row_shape) or source_latent.numel() != row_shape[0] * row_shape[1] * row_shape[2]:
        raise ValueError(f"prox: source_latent of shape {tuple(source_latent.shape)} for latents of shape {tuple(row_shape)}")
    if row_shape[0] * row_shape[1] * row_shape[2] > hip.PROX_MAX_ROW:
        raise ValueError(f"prox: a latent row of {row_shape[0] * row_shape[1] * row_shape[2]} elements, the threshold serves at most "
                         f"{hip.PROX_MAX_ROW}")
    if len(plan.eta) != num_steps:
        raise ValueError(f"prox: the plan's rows cover {len(plan.eta)} edit steps, the loop runs {num_steps}")


def _mask_rows(mask, num_latents, device):
    """the device buffer of an edit mask: fp32 [Bp, h, w], one mask per batch row"""
    m = mask.to(device).float()
    return (m[None].expand(num_latents, -1, -1) if m.dim() == 2 else m).contiguous().clone()


class FusedDenoiser:
    def __init__(self, model, context: torch.Tensor, num_latents: int, latent_hw, guidance_scale: Optional[float],
                 mode: str = "denoise", uncond_list: Optional[List[torch.Tensor]] = None, use_graph: bool = True,
                 added_cond_kwargs=None, source_trajectory: Optional[torch.Tensor] = None,
                 noise_maps: Optional[torch.Tensor] = None, skip: int = 0, edit_mask: Optional[torch.Tensor] = None,
                 ledits=None, solver_order: int = 1, prox=None, source_latent: Optional[torch.Tensor] = None):
        """context: [2*Bp,77,C] (uncond, cond) for mode 'denoise' with CFG, [Bp,77,C] for 'invert' / no-CFG.
        added_cond_kwargs: SDXL's {"text_embeds" [B, 1280], "time_ids" [B, 6]} (one row per UNet batch row); they are
        constant over the steps, so they fold into the per-step time-embedding rows (then one row PER BATCH ROW).
        source_trajectory: Direct Inversion -- fp32 [S, C, h, w], row i = z*_{S-1-i} of the DDIM inversion; after step i batch row 0
        (the source branch) is x' + (z - x') in the launch of the CFG + DDIM update, every other row is x'.
        noise_maps, skip: edit-friendly DDPM inversion -- fp32 [S - skip, C, h, w], the maps of `p2p.inversion.ddpm.DDPMInversion`; the
        loop runs the S - skip timesteps `timesteps[skip:]` from y_skip, step i is the eta = 1 update with map i (every batch row
        reads the same map), and `guidance_scale` may be a sequence of one scale per latent (the source row takes the scale its
        maps were extracted with).
        edit_mask, source_trajectory, skip: DiffEdit -- fp32 or bool [Bp, h, w] (or [h, w]), nonzero = edited, with the trajectory of
        a PARTIAL inversion, fp32 [S - skip, C, h, w], row i = z*_{S-skip-1-i}; the loop runs `timesteps[skip:]` from z*_{S-skip} and
        after step i every row is x' inside its mask and the trajectory row outside it (a select, in the launch of the update).
        ledits, noise_maps, skip: LEDITS++ -- the 'ledits' `control.ControlPlan` registered on the UNet (E concepts); num_latents is
        1, context [1 + E, 77, C] = [uncond | concept_1 .. concept_E], guidance_scale None (the per-step scales are the plan's);
        every row of the UNet batch is the one latent, and the step ends with the plan's masks and `ief_ledits_ddpm_step_f32`.
        solver_order (with noise_maps): 1 = the eta = 1 update; 2 = the second-order multistep SDE-DPM-Solver++ on maps extracted
        at order 2 with the same skip (`DDPMInversion.noise_maps(solver_order=2)`): the loop owns the x0 prediction of the previous
        step and a five-column coefficient table {a, p, sigma, dir, c2} (`DDIMScheduler.dpmpp_table`), and its step ends with
        `ief_cfg_dpmpp_step_f32` / `ief_ledits_dpmpp_step_f32` inside the captured graph.
        prox, source_latent: proximal guidance on a negative-prompt-inversion edit -- a `ProxGuidance` plan and the encoded source
        image, fp32 [C, h, w]; the context's unconditional rows are the caller's (NPI: the source prompt's embedding).  The step
        ends with `hip.prox_threshold` and `hip.cfg_ddim_step(prox=)` in place of the plain update, the coefficient rows are
        {a_from, a_to, g, prox_on, eta}, and nothing syncs."""
        check_solver_order(solver_order, noise_maps)
        self.solver_order = solver_order
        self.model, self.unet, self.sched = model, model.unet, model.scheduler
        dev = self.unet.device
        self.mode = mode
        self.cfg = guidance_scale is not None
        self.ledits = ledits
        self.prox = prox
        if prox is not None:
            check_prox(prox, mode=mode, cfg=self.cfg, uncond_list=uncond_list, source_trajectory=source_trajectory,
                       noise_maps=noise_maps, edit_mask=edit_mask, ledits=ledits, added_cond_kwargs=added_cond_kwargs,
                       local_blend=getattr(self.unet._plan, "blend_w", None), source_latent=source_latent,
                       row_shape=(self.unet.config.in_channels, *latent_hw), num_steps=len(self.sched.timesteps))
        elif source_latent is not None:
            raise ValueError("source_latent: only a loop under proximal guidance (prox=) reads the encoded source image")
        if ledits is not None:
            check_ledits_loop(ledits, unet_plan=self.unet._plan, mode=mode, guidance_scale=guidance_scale, uncond_list=uncond_list,
                              source_trajectory=source_trajectory, edit_mask=edit_mask, noise_maps=noise_maps, skip=skip,
                              row_shape=(self.unet.config.in_channels, *latent_hw), num_steps=len(self.sched.timesteps),
                              num_latents=num_latents, context_rows=context.shape[0], added_cond_kwargs=added_cond_kwargs)
        elif getattr(self.unet._plan, "kind", None) == "ledits":
            raise ValueError("a 'ledits' control plan is registered on the UNet: its loop is built with ledits=plan")
        if ledits is None and edit_mask is not None:
            check_edit_mask(edit_mask, mode=mode, cfg=self.cfg, uncond_list=uncond_list, noise_maps=noise_maps,
                            source_trajectory=source_trajectory, row_shape=(self.unet.config.in_channels, *latent_hw),
                            num_steps=len(self.sched.timesteps), skip=skip, num_latents=num_latents)
            if added_cond_kwargs is not None:
                raise ValueError("edit_mask: DiffEdit is built for the SD1.x / SD2.x pipelines (no added_cond_kwargs)")
        elif ledits is None and source_trajectory is not None:
            check_source_trajectory(source_trajectory, mode=mode, cfg=self.cfg, uncond_list=uncond_list,
                                    row_shape=(self.unet.config.in_channels, *latent_hw), num_steps=len(self.sched.timesteps))
        if ledits is not None:
            pass                              # check_ledits_loop has checked the maps and the skip
        elif noise_maps is not None:
            check_noise_maps(noise_maps, mode=mode, cfg=self.cfg, uncond_list=uncond_list, source_trajectory=source_trajectory,
                             row_shape=(self.unet.config.in_channels, *latent_hw), num_steps=len(self.sched.timesteps), skip=skip,
                             guidance_scale=guidance_scale, num_latents=num_latents)
            if added_cond_kwargs is not None:
                raise ValueError("noise_maps: DDPM inversion is built for the SD1.x / SD2.x pipelines (no added_cond_kwargs)")
        elif skip and edit_mask is None:
            raise ValueError("skip: only a loop with noise maps starts inside the schedule")
        self.skip = skip if (noise_maps is not None or edit_mask is not None) else 0
        self.Bp = num_latents
        self.B = 2 * num_latents if self.cfg else num_latents
        if ledits is not None:
            self.B = 1 + ledits.led["E"]
        if context.shape[0] != self.B:
            raise ValueError(f"context batch {context.shape[0]} != UNet batch {self.B}")
        h, w = latent_hw
        C = self.unet.config.in_channels
        self.lat = torch.zeros(self.Bp, C, h, w, dtype=torch.float32, device=dev)
        # decided once, here, from the model and the plan registered NOW: the launches of a captured step follow from it, so it is
        # part of `_key` (every fact it rests on is in the plan's signature, the model or the shapes)
        self.shared_reason = self._shared_reason(context.shape[1])
        self.shared = self.shared_reason is None
        if (self.cfg and not self.shared and mode == "denoise" and CFG_SHARED_PREFIX and getattr(self.unet, "x3p", False)
                and self.shared_reason not in _said):
            _said.add(self.shared_reason)       # a planes model that could share and does not: said once per reason
            _log.warning("CFG step without the shared prefix: %s", self.shared_reason)
        self.lat_in = self.lat if (self.shared or not self.cfg) else torch.zeros(self.B, C, h, w, dtype=torch.float32, device=dev)
        if ledits is not None:              # every row of [uncond | concepts] is the one latent
            self.lat_in = torch.zeros(self.B, C, h, w, dtype=torch.float32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.coef_cur = torch.zeros(5 if (solver_order == 2 or prox is not None) else 4, dtype=torch.float32, device=dev)
        # order 2: the x0 prediction the previous step wrote.  Never zeroed: the first step of a run is order 1 and does not read it
        self.x0_prev = None
        if solver_order == 2:
            self.x0_prev = torch.zeros((C, h, w) if ledits is not None else (self.Bp, C, h, w), dtype=torch.float32, device=dev)
        self.coef_table = self.temb_table = self.temb_cur = self.ctx = self.ctx_table = None
        # the graph READS this buffer (row = the device step counter): `rebind` copies the next image's rows into it
        self.traj = None if source_trajectory is None else source_trajectory.to(dev).contiguous().clone()
        # likewise the noise maps and the per-row guidance scales of a DDPM inversion edit
        self.maps = None if noise_maps is None else noise_maps.to(dev).contiguous().clone()
        self.g_rows = None
        # and the edit masks of a DiffEdit loop, one per batch row
        self.mask = None if edit_mask is None else _mask_rows(edit_mask, num_latents, dev)
        # and the encoded source, the quantile's rank and the per-row thresholds of a loop under proximal guidance
        self.z0 = self.prox_rank = self.prox_thres = None
        if prox is not None:
            self.z0 = source_latent.to(dev).reshape(C, h, w).contiguous().clone()
            self.prox_rank = prox.rank(C * h * w).to(dev)
            self.prox_thres = torch.zeros(self.Bp, dtype=torch.float32, device=dev)
        self._fill(context, guidance_scale, uncond_list, added_cond_kwargs)
        self.use_graph = use_graph
        self.graph = None
        self.plan = self.unet._plan
        self._keep, self._pooled_started, self._pool_key = None, False, None
        self._done = 0          # steps taken since the last rewind (host mirror of the device step counter)

    def _fill(self, context, guidance_scale, uncond_list, added_cond_kwargs=None):
        """(re)compute every table the step graph reads, IN PLACE once the buffers exist (re-use of a captured loop)"""
        dev = self.unet.device
        ts = self.sched.timesteps.tolist()
        if self.mode == "invert":
            ts = ts[::-1]
            coef = [self.sched.reverse_coeffs(t) for t in ts]
        elif self.maps is not None:
            ts = ts[self.skip:]
            if self.solver_order == 2:      # rows {a, p, sigma, dir, c2}: order 1 on the first and the last step of the run
                coef = self.sched.dpmpp_table(self.skip, 2)
            else:
                coef = [self.sched.ddpm_coeffs(t) for t in ts]
        else:
            if self.mask is not None:       # DiffEdit decodes the tail of the schedule
                ts = ts[self.skip:]
            coef = [self.sched.step_coeffs(t) for t in ts]
        g = float(guidance_scale) if self.cfg and self.maps is None else 1.0
        self.num_steps = len(ts)

        def put(name, value):
            cur = getattr(self, name)
            if cur is None:
                setattr(self, name, value)
            else:
                cur.copy_(value)

        if self.maps is not None:         # rows {a, p, sigma, dir} (order 2: and c2); the guidance scales travel per batch row
            put("coef_table", torch.tensor(coef, dtype=torch.float32, device=dev))
            if self.ledits is None:
                put("g_rows", torch.tensor(guidance_rows(guidance_scale, self.Bp), dtype=torch.float32, device=dev))
        elif getattr(self, "prox", None) is not None:   # rows {a_from, a_to, g, prox_on, eta}
            put("coef_table", torch.tensor([[a, b, g, on, eta] for (a, b), on, eta in zip(coef, self.prox.prox_on, self.prox.eta)],
                                           dtype=torch.float32, device=dev))
        else:
            put("coef_table", torch.tensor([[a, b, g, 0.0] for a, b in coef], dtype=torch.float32, device=dev))
        aug = self.unet.aug_embedding(added_cond_kwargs)          # None unless the UNet has SDXL's additional embedding
        if aug is not None and aug.shape[0] != self.B:
            raise ValueError(f"added_cond_kwargs batch {aug.shape[0]} != UNet batch {self.B}")
        rows = self.unet.time_rows(torch.tensor(ts, dtype=torch.float32, device=dev), aug)
        nb = 1 if aug is None else self.B
        put("temb_table", rows.reshape(len(ts), nb, -1).contiguous())
        if self.temb_cur is None:
            self.temb_cur = torch.zeros(nb, self.temb_table.shape[2], dtype=torch.float32, device=dev)
        ctx16 = self.unet._act(context.to(dev))               # the model's activation dtype (fp16; fp32 in the exact mode)
        if uncond_list is not None:  # null-text embeddings: the uncond half changes every step
            rows = []
            for u in uncond_list:
                u16 = self.unet._act(u.to(dev)).expand(self.Bp, *ctx16.shape[1:])
                rows.append(torch.cat([u16, ctx16[self.Bp:]], 0))
            put("ctx_table", torch.stack(rows).contiguous())
            if self.ctx is None:
                self.ctx = torch.zeros_like(ctx16)
        else:
            # a COPY: in the fp32-storage modes `_act` hands back the caller's own tensor, and a pooled loop re-pointed at the
            # next image writes into this buffer -- the previous image's context (still held by the caller for its null-text
            # optimisation / edit) must not change under it
            put("ctx", ctx16.clone())

    def _shared_reason(self, ctx_len):
        """None where this loop's steps run the shared prefix (`cfg_shared_prefix_reason`), else why not"""
        facts = getattr(self.unet, "cfg_shared_facts", None)
        if facts is None:
            return "the UNet has no shared-prefix form"
        return cfg_shared_prefix_reason(mode=self.mode, cfg=self.cfg, enabled=CFG_SHARED_PREFIX and type(self)._step_body is FusedDenoiser._step_body,
                                        ledits=getattr(self, "ledits", None) is not None,
                                        **facts(tuple(self.lat.shape[-2:]), ctx_len))

    def _key(self, context, uncond_list, source_trajectory=None, noise_maps=None, skip=0, edit_mask=None, ledits=None,
             solver_order=1, prox=None):
        plan = self.unet._plan
        key = (id(self.unet), self.mode, self.Bp, tuple(self.lat.shape[-2:]), self.cfg, tuple(context.shape),
               None if uncond_list is None else len(uncond_list), len(self.sched.timesteps),
               None if plan is None else plan.signature(self.unet), self._shared_reason(context.shape[1]) is None,
               edit_mask is not None, source_trajectory is not None, noise_maps is not None,
               skip if (noise_maps is not None or edit_mask is not None) else 0, getattr(self.unet, "attn_key_splits", 1))
        # a LEDITS++ loop says so itself (its plan's signature, above, carries E, the mask mode and the module indices)
        key = key if ledits is None else key + ("ledits",)
        # an order-1 loop keeps the key it always had; an order-2 loop (other launches, a wider table) names its solver
        key = key if solver_order == 1 else key + (("solver_order", solver_order),)
        # proximal guidance: other launches, and mode and radius are launch arguments (the quantile and the rows are contents)
        return key if prox is None else key + (("prox", prox.mode, prox.radius),)

    def rebind(self, context, guidance_scale, uncond_list, added_cond_kwargs=None, source_trajectory=None, noise_maps=None,
               skip=0, edit_mask=None, ledits=None, solver_order=1, prox=None, source_latent=None):
        """point a captured loop at the next image: new tables, new cross-attention K/V, the new controller's plan, the next
        image's inversion trajectory or noise maps and guidance scales, or its edit masks; a LEDITS++ loop takes the next
        image's concepts, scales and thresholds from the freshly registered plan"""
        check_solver_order(solver_order, noise_maps)
        if solver_order != self.solver_order:
            raise ValueError(f"rebind: a loop captured at solver order {self.solver_order} serves only jobs of that order")
        if (ledits is None) != (self.ledits is None):
            raise ValueError("rebind: a LEDITS++ loop serves only LEDITS++ jobs, and the reverse")
        if (prox is None) != (self.prox is None) or (prox is not None and (prox.mode, prox.radius) != (self.prox.mode, self.prox.radius)):
            raise ValueError("rebind: a loop captured under proximal guidance serves only jobs of the same mode and radius, and the "
                             "reverse")
        if prox is not None:
            check_prox(prox, mode=self.mode, cfg=self.cfg, uncond_list=uncond_list, source_trajectory=source_trajectory,
                       noise_maps=noise_maps, edit_mask=edit_mask, ledits=ledits, added_cond_kwargs=added_cond_kwargs,
                       local_blend=getattr(self.unet._plan, "blend_w", None), source_latent=source_latent,
                       row_shape=tuple(self.lat.shape[1:]), num_steps=len(self.sched.timesteps))
            self.prox = prox            # `_fill` writes its rows into the coefficient table
            self.z0.copy_(source_latent.to(self.z0.device).reshape(self.z0.shape))
            self.prox_rank.copy_(prox.rank(self.z0.numel()))
        elif source_latent is not None:
            raise ValueError("source_latent: only a loop under proximal guidance (prox=) reads the encoded source image")
        if ledits is not None:
            check_ledits_loop(ledits, unet_plan=self.unet._plan, mode=self.mode, guidance_scale=guidance_scale, uncond_list=uncond_list,
                              source_trajectory=source_trajectory, edit_mask=edit_mask, noise_maps=noise_maps, skip=skip,
                              row_shape=tuple(self.lat.shape[1:]), num_steps=len(self.sched.timesteps), num_latents=self.Bp,
                              context_rows=context.shape[0], added_cond_kwargs=added_cond_kwargs)
            if skip != self.skip or ledits.signature(self.unet) != self.plan.signature(self.unet):
                raise ValueError("rebind: a LEDITS++ loop serves only jobs of the same skip and plan signature")
        if (edit_mask is None) != (self.mask is None) or (edit_mask is not None and skip != self.skip):
            raise ValueError("rebind: a loop captured with an edit mask serves only jobs that bring a mask and the same skip, and the "
                             "reverse")
        if edit_mask is not None:
            check_edit_mask(edit_mask, mode=self.mode, cfg=self.cfg, uncond_list=uncond_list, noise_maps=noise_maps,
                            source_trajectory=source_trajectory, row_shape=tuple(self.lat.shape[1:]),
                            num_steps=len(self.sched.timesteps), skip=skip, num_latents=self.Bp)
            self.mask.copy_(_mask_rows(edit_mask, self.Bp, self.mask.device))
        if (noise_maps is None) != (self.maps is None) or (noise_maps is not None and skip != self.skip):
            raise ValueError("rebind: a loop captured with noise maps serves only jobs that bring maps of the same skip, and the reverse")
        if noise_maps is not None:
            if ledits is None:              # check_ledits_loop has checked a LEDITS++ job's maps
                check_noise_maps(noise_maps, mode=self.mode, cfg=self.cfg, uncond_list=uncond_list, source_trajectory=source_trajectory,
                                 row_shape=tuple(self.lat.shape[1:]), num_steps=len(self.sched.timesteps), skip=skip,
                                 guidance_scale=guidance_scale, num_latents=self.Bp)
            self.maps.copy_(noise_maps)
        if (source_trajectory is None) != (self.traj is None):
            raise ValueError("rebind: a loop captured with a source trajectory serves only jobs that bring one, and the reverse")
        if source_trajectory is not None:
            if edit_mask is None:
                check_source_trajectory(source_trajectory, mode=self.mode, cfg=self.cfg, uncond_list=uncond_list,
                                        row_shape=tuple(self.lat.shape[1:]), num_steps=len(self.sched.timesteps))
            self.traj.copy_(source_trajectory)
        self._fill(context, guidance_scale, uncond_list, added_cond_kwargs)
        if self.ctx_table is None:          # K/V of the fixed context live in tensors the graph reads: refresh in place, by the
            # same kernels the forward used (the model's contraction mode: "x3" and "f32" differ in the last bits, and an
            # image must not depend on whether its loop was captured for it or re-pointed at it)
            with hip.f32_contraction(getattr(self.unet, "contract", "f32")):
                for m, kv in self._keep:
                    hip.gemm(self.ctx, m.w_kv, out=kv)
        fresh = self.unet._plan
        if self.plan is not None:
            self.plan.load_from(fresh, self.B)
            self.plan.sync_step()
        self.step.zero_()
        self._done = 0

    # ------------------------------------------------------------------ one step, stream-ordered
    def _step_body(self):
        hip.select_step(self.temb_table, self.temb_cur, self.step)
        hip.select_step(self.coef_table, self.coef_cur, self.step)
        if self.ctx_table is not None:
            hip.select_step(self.ctx_table, self.ctx, self.step)
        if self.ledits is not None:
            # [uncond | concept_1 .. concept_E], all rows on the same latent and time embedding; then the implicit masks and the
            # masked multi-concept guidance with the eta = 1 update (`ControlPlan.ledits_step`)
            self.lat_in.copy_(self.lat.expand_as(self.lat_in))
            eps = self.unet(self.lat_in, encoder_hidden_states=self.ctx, temb_row=self.temb_cur)["sample"]
            if self.x0_prev is None:
                self.plan.ledits_step(eps, self.lat, self.coef_cur, self.maps, self.step)
            else:
                self.plan.ledits_step(eps, self.lat, self.coef_cur, self.maps, self.step, x0_prev=self.x0_prev)
            hip.advance_step(self.step)
            return
        if self.cfg and self.shared:
            # the UNet takes the Bp latents themselves: no CFG batch copy, and what both halves share is computed once
            eps = self.unet(self.lat, encoder_hidden_states=self.ctx, temb_row=self.temb_cur, cfg_pair=True)["sample"]
        else:
            if self.cfg:
                self.lat_in[: self.Bp].copy_(self.lat)
                self.lat_in[self.Bp:].copy_(self.lat)
            eps = self.unet(self.lat_in, encoder_hidden_states=self.ctx, temb_row=self.temb_cur)["sample"]
        if self.maps is not None and self.solver_order == 2:
            hip.cfg_dpmpp_step(eps[: self.Bp], eps[self.Bp:], self.lat, self.coef_cur, self.g_rows, self.maps, self.step, self.x0_prev,
                               out=self.lat)
        elif self.maps is not None:
            hip.cfg_ddpm_step(eps[: self.Bp], eps[self.Bp:], self.lat, self.coef_cur, self.g_rows, self.maps, self.step, out=self.lat)
        elif self.mask is not None:
            hip.cfg_ddim_step(eps[: self.Bp], eps[self.Bp:], self.lat, self.coef_cur, out=self.lat,
                              masked=(self.traj, self.step, self.mask))
        elif self.prox is not None:
            # the per-row quantile of |eps_c - eps_u| (one workgroup per row), then the thresholded guidance, the update and the
            # pull towards the encoded source in one launch; this step's prox_on and eta came with the coefficient row
            hip.prox_threshold(eps[: self.Bp], eps[self.Bp:], self.prox_rank, out=self.prox_thres)
            hip.cfg_ddim_step(eps[: self.Bp], eps[self.Bp:], self.lat, self.coef_cur, out=self.lat,
                              prox=(self.prox_thres, self.z0, self.prox.mode, self.prox.radius))
        elif self.cfg:
            hip.cfg_ddim_step(eps[: self.Bp], eps[self.Bp:], self.lat, self.coef_cur, out=self.lat,
                              rect=None if self.traj is None else (self.traj, self.step))
        else:
            hip.cfg_ddim_step(None, eps, self.lat, self.coef_cur, out=self.lat)
        if self.plan is not None and self.cfg:
            # the reference's `controller.step_callback` (p2p/model/sd_utils.py, diffusion_step): a lowered LocalBlend blends the
            # updated latents in place from the maps this and the earlier steps accumulated; nothing for any other plan
            self.plan.blend_latents(self.lat)
        hip.advance_step(self.step)

    def _set_kv_cache(self, on: bool):
        for m in self.unet.attention_modules():
            m.cache_kv = on

    def _capture(self):
        plan = self.plan
        # the context K/V are step-invariant unless null-text rows are swapped in per step
        self._set_kv_cache(self.ctx_table is None)
        # warm-up outside the graph with the control plan muted (fills the K/V cache and the
        # allocator pools without moving any counter), on a side stream as capture requires
        saved = self.lat.clone()
        if plan is not None:
            plan.prepare(self.B)
            plan.muted = True
        used0 = hip.counters_used()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step_body()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if plan is not None:
            plan.muted = False
        self.lat.copy_(saved)
        self.step.zero_()
        if plan is not None:
            plan.sync_step()
            plan.captured = True
        # the split-K launches of this graph combine their slabs inside the launch and need arrival counters nobody else
        # touches while the graph may run: an arena of the size the warm-up pass used, owned by this loop
        self._arena = hip.counter_arena(hip.counters_used() - used0, self.lat.device)
        self.graph = torch.cuda.CUDAGraph()
        with self._arena, torch.cuda.graph(self.graph):
            self._step_body()
        self.lat.copy_(saved)
        self.step.zero_()
        if plan is not None:
            plan.sync_step()

    # ------------------------------------------------------------------ public
    def start(self, latents: torch.Tensor):
        """load the initial latents [Bp,C,h,w] (or [1,...] broadcast), rewind, capture the step graph if needed.
        Must run while this loop's controller (if any) is registered on the UNet; stepping afterwards does not
        need the registration, so several started loops can be stepped in turn (`run_interleaved`)."""
        self.lat.copy_(latents.to(self.lat.device).float().expand_as(self.lat))
        self.step.zero_()
        self._done = 0
        if self.use_graph and self.graph is None:
            self._capture()
        elif not self.use_graph:
            self._set_kv_cache(self.ctx_table is None)
        # tensors the graph READS but does not own (cross-attention K/V projected during the warm-up): keep them
        # alive for as long as this loop may be replayed, whatever another loop's warm-up caches afterwards
        if getattr(self, "_keep", None) is None or not self._pooled_started:
            self._keep = [(m, m._kv) for m in self.unet.attention_modules() if m.is_cross and m._kv is not None]
            self._pooled_started = True
        if self.plan is not None and self.graph is not None:
            self.plan.sync_step()

    def rewind(self, latents: Optional[torch.Tensor] = None):
        """back to step 0 of the schedule (device and host counters, the plan's counter from its controller)"""
        if latents is not None:
            self.lat.copy_(latents.to(self.lat.device).float().expand_as(self.lat))
        self.step.zero_()
        self._done = 0
        if self.plan is not None:
            self.plan.sync_step()

    def step_once(self):
        # the per-step tables have num_steps rows: a replay past them would re-read the last row (the kernel clamps the row
        # index) and silently apply the final timestep again
        if self._done >= self.num_steps:
            raise IndexError(f"step {self._done} is past the {self.num_steps}-step schedule this loop was built for; "
                             "rewind() or start() it first")
        self._done += 1
        if self.graph is not None:
            self.graph.replay()
            if self.plan is not None:
                self.plan.replay_done()
        else:
            self._step_body()

    def result(self) -> torch.Tensor:
        return self.lat.clone()

    def run(self, latents: torch.Tensor, num_steps: Optional[int] = None, keep_all: bool = False):
        """latents [Bp,C,h,w] (or [1,...] broadcast) -> final latents (and the trajectory if keep_all)."""
        self.start(latents)
        n = self.num_steps if num_steps is None else num_steps
        traj = [self.lat.clone()] if keep_all else None
        for _ in range(n):
            self.step_once()
            if keep_all:
                traj.append(self.lat.clone())
        out = self.lat.clone()
        _check_finite(out, self.unet)
        return (out, traj) if keep_all else out

    def release(self):
        key = getattr(self, "_pool_key", None)
        if REUSE_GRAPHS and key is not None and self.graph is not None and len(_POOL.setdefault(key, [])) < _POOL_CAP:
            _POOL[key].append(self)          # keep the captured graph for the next image of this shape
            return
        if self.plan is not None:
            self.plan.captured = False
        self.graph = None


def cfg_split_rows(context: torch.Tensor, num_latents: int, half: int) -> torch.Tensor:
    """rows of the CFG context [uncond..., cond...] that rank `half` of a 2-GPU CFG split runs (0: unconditional)"""
    if context.shape[0] != 2 * num_latents or half not in (0, 1):
        raise ValueError("cfg_split_rows: context must be [2 * num_latents, ...] and half 0 or 1")
    return context[:num_latents] if half == 0 else context[num_latents:]


def exchange_eps(eps_all: torch.Tensor, mine: torch.Tensor, group=None):
    """the ONE exchange of a CFG-split step: every rank contributes its half of eps ([Bp,4,h,w] fp32, 64 KiB per latent at
    64x64) and receives both, rank order = [unconditional, conditional] (`/root/reference/p2p/model/sd_utils.py:74`: the
    chunk(2) the CFG combine reads).  RCCL all-gather on device buffers; on a gloo group (CPU tests, two ranks sharing one
    GPU) the halves are staged through host memory."""
    import torch.distributed as dist
    if dist.get_backend(group) == "gloo":
        parts = [torch.empty(mine.shape, dtype=mine.dtype) for _ in range(dist.get_world_size(group))]
        dist.all_gather(parts, mine.detach().cpu().contiguous(), group=group)
        eps_all.copy_(torch.cat(parts).to(eps_all.device))
    else:
        dist.all_gather_into_tensor(eps_all, mine.contiguous(), group=group)
    return eps_all


class CfgSplitDenoiser(FusedDenoiser):
    """ONE edit on TWO GPUs: the CFG batch [uncond_src, uncond_tgt | cond_src, cond_tgt] has no data
    dependence between its halves inside the UNet — controllers act on the conditional rows only
    (`/root/reference/p2p/model/attention_base.py:20-22`) — so rank 0 of the pair runs the unconditional rows, rank 1
    the conditional rows with the controller's plan, and each step needs one exchange: the two eps halves (128 KiB at
    64x64 latents) are all-gathered before the CFG combine (`sd_utils.py:74-75`).  Both ranks then apply the same fused
    CFG + DDIM update to their own copy of the latents, which therefore stay identical without a second exchange.

    Per step: captured graph A {row selects, UNet on this rank's rows} -> all-gather -> captured graph B {CFG + DDIM
    update, advance}.  The controller must be registered with `rows="uncond"` / `rows="cond"` on the two ranks
    (`p2p.model.register.register_attention_control`); its counters advance on both."""

    def __init__(self, model, context, num_latents, latent_hw, guidance_scale: float, group=None, uncond_list=None,
                 use_graph: bool = True, source_trajectory=None, noise_maps=None, skip=0, edit_mask=None, solver_order=1):
        if solver_order != 1:
            raise ValueError("CFG split: the second-order solver steps on DDPM noise maps, which are not built for the two-GPU "
                             "split; run the edit on one GPU")
        if getattr(model.unet._plan, "kind", None) == "ledits":
            raise ValueError("CFG split: LEDITS++ runs [uncond | concepts] on one latent, not two halves; run the edit on one GPU")
        if edit_mask is not None:
            raise ValueError("CFG split: DiffEdit (edit_mask) is not built for the two-GPU split; run the edit on one GPU")
        if noise_maps is not None or skip:
            raise ValueError("CFG split: edit-friendly DDPM inversion (noise_maps) is not built for the two-GPU split; run the edit "
                             "on one GPU")
        if source_trajectory is not None:
            raise ValueError("CFG split: Direct Inversion (source_trajectory) is not built for the two-GPU split; run the edit "
                             "on one GPU")
        import torch.distributed as dist
        if dist.get_world_size(group) != 2:
            raise ValueError("a CFG split runs on a group of exactly two ranks")
        self.group = group
        self.half = dist.get_rank(group)
        self._guidance = float(guidance_scale)
        plan = model.unet._plan
        want = num_latents
        if plan is not None and plan.kind == "p2p" and (not plan.cond_only or self.half != 1 or plan.batch != want):
            raise ValueError('CFG split: register the controller with rows="cond" on rank 1 and rows="uncond" on rank 0')
        # every other plan kind (MasaCtrl, Plug-and-Play) and every Python hook was built for the FULL [uncond..., cond...]
        # batch: on a half batch its row indirections would point at the wrong or at missing rows without any error
        if plan is not None and plan.kind not in ("p2p", "empty"):
            raise ValueError(f"CFG split: a '{plan.kind}' control plan addresses the full CFG batch; only Prompt-to-Prompt "
                             'controllers registered with rows="cond" / "uncond" (or no controller) can be split')
        if plan is None and not all(m.is_native() for m in model.unet.attention_modules()):
            raise ValueError("CFG split: an attention hook is installed that was written for the full CFG batch")
        super().__init__(model, cfg_split_rows(context, num_latents, self.half), num_latents, latent_hw, None, mode="denoise",
                         uncond_list=uncond_list if self.half == 0 else None, use_graph=use_graph)
        C = self.unet.config.in_channels
        h, w = latent_hw
        self.eps_all = torch.zeros(2 * self.Bp, C, h, w, dtype=torch.float32, device=self.lat.device)
        self.eps_mine = torch.zeros(self.Bp, C, h, w, dtype=torch.float32, device=self.lat.device)
        self.graph_b = None

    def _fill(self, context, guidance_scale, uncond_list, added_cond_kwargs=None):
        super()._fill(context, None, uncond_list, added_cond_kwargs)
        self.coef_table[:, 2] = self._guidance          # the parent wrote 1.0 (no CFG inside ITS step)

    # ---- the two captured halves of a step
    def _forward_part(self):
        hip.select_step(self.temb_table, self.temb_cur, self.step)
        hip.select_step(self.coef_table, self.coef_cur, self.step)
        if self.ctx_table is not None:
            hip.select_step(self.ctx_table, self.ctx, self.step)
        eps = self.unet(self.lat, encoder_hidden_states=self.ctx, temb_row=self.temb_cur)["sample"]
        self.eps_mine.copy_(eps)

    def _update_part(self):
        hip.cfg_ddim_step(self.eps_all[: self.Bp], self.eps_all[self.Bp:], self.lat, self.coef_cur, out=self.lat)
        hip.advance_step(self.step)

    def _step_body(self):
        self._forward_part()
        exchange_eps(self.eps_all, self.eps_mine, self.group)
        self._update_part()

    def _capture(self):
        plan = self.plan
        self._set_kv_cache(self.ctx_table is None)
        saved = self.lat.clone()
        if plan is not None:
            plan.prepare(self.B)
            plan.muted = True
        used0 = hip.counters_used()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._forward_part()            # warm-up of the forward half only: no collective on a side stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if plan is not None:
            plan.muted = False
        self.step.zero_()
        if plan is not None:
            plan.sync_step()
            plan.captured = True
        self._arena = hip.counter_arena(hip.counters_used() - used0, self.lat.device)
        self.graph = torch.cuda.CUDAGraph()
        with self._arena, torch.cuda.graph(self.graph):
            self._forward_part()
        self.graph_b = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_b):
            self._update_part()
        self.lat.copy_(saved)
        self.step.zero_()
        if plan is not None:
            plan.sync_step()

    def step_once(self):
        if self._done >= self.num_steps:
            raise IndexError(f"step {self._done} is past the {self.num_steps}-step schedule this loop was built for")
        self._done += 1
        if self.graph is not None:
            self.graph.replay()
            exchange_eps(self.eps_all, self.eps_mine, self.group)
            self.graph_b.replay()
            if self.plan is not None:
                self.plan.replay_done()
        else:
            self._step_body()

    def release(self):
        if self.plan is not None:
            self.plan.captured = False
        self.graph = self.graph_b = None


def acquire(model, context, num_latents, latent_hw, guidance_scale, mode="denoise", uncond_list=None,
            use_graph=True, added_cond_kwargs=None, source_trajectory=None, noise_maps=None, skip=0,
            edit_mask=None, ledits=None, solver_order=1, prox=None, source_latent=None) -> FusedDenoiser:
    """a FusedDenoiser for this job: a pooled one with a captured graph of the same shape / plan signature, re-pointed
    at the new context, tables and controller — or a new one.  source_trajectory: Direct Inversion (`FusedDenoiser`); loops
    with and without one never share a pool entry.  noise_maps, skip: edit-friendly DDPM inversion (`FusedDenoiser`;
    guidance_scale may then be one scale per latent); presence of maps and skip are part of the pool key.  edit_mask (with
    source_trajectory and skip): DiffEdit (`FusedDenoiser`); loops with and without a mask never share a pool entry.  ledits (with
    noise_maps and skip; guidance_scale None): LEDITS++ (`FusedDenoiser`), the 'ledits' plan registered on the UNet -- its signature
    (E, the mask mode, the module indices) is part of the pool key, so pooled loops of different kinds never mix.  solver_order
    (with noise_maps): 2 = the second-order SDE-DPM-Solver++ step (`FusedDenoiser`); part of the pool key, order-1 keys unchanged.
    prox (with source_latent): proximal guidance on a negative-prompt-inversion edit (`ProxGuidance`, `FusedDenoiser`); its mode and
    radius are part of the pool key, its quantile and per-step rows are contents a pooled loop is re-pointed at"""
    check_solver_order(solver_order, noise_maps)
    if REUSE_GRAPHS and use_graph:
        probe = FusedDenoiser.__new__(FusedDenoiser)
        probe.unet, probe.sched, probe.mode = model.unet, model.scheduler, mode
        probe.cfg, probe.Bp, probe.ledits = guidance_scale is not None, num_latents, ledits
        probe.lat = torch.empty(0, 0, *latent_hw)
        key = probe._key(context, uncond_list, source_trajectory, noise_maps, skip, edit_mask, ledits, solver_order, prox)
        free = _POOL.get(key)
        if free:
            loop = free.pop()
            loop.rebind(context, guidance_scale, uncond_list, added_cond_kwargs, source_trajectory, noise_maps, skip, edit_mask, ledits,
                        solver_order, prox, source_latent)
            return loop
        loop = FusedDenoiser(model, context, num_latents, latent_hw, guidance_scale, mode, uncond_list, use_graph,
                             added_cond_kwargs, source_trajectory, noise_maps, skip, edit_mask, ledits, solver_order, prox, source_latent)
        loop._pool_key = key
        return loop
    return FusedDenoiser(model, context, num_latents, latent_hw, guidance_scale, mode, uncond_list, use_graph,
                         added_cond_kwargs, source_trajectory, noise_maps, skip, edit_mask, ledits, solver_order, prox, source_latent)


def drop_pool():
    """free every pooled graph (tests; before changing weights)"""
    for loops in _POOL.values():
        for l in loops:
            l.graph = None
    _POOL.clear()


def run_interleaved(loops: List[FusedDenoiser], num_steps: Optional[int] = None):
    """Step several STARTED loops (independent images) in turn, each on its own stream.

    One edit step is ~380 dependent launches of which each pays ~4 us of dispatch latency, so a single chain leaves
    the GPU idle a fifth of the time; with E chains in flight those gaps are filled by the other chains' kernels
    (measured on SD1.5 shapes, UNet batch 4: 7.7 ms per step alone, 6.4 / 5.8 / 5.6 ms per step with 2 / 3 / 4 in
    flight).  Results are those of running the loops one after the other."""
    if not loops:
        return
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in loops]
    for s in streams:
        s.wait_stream(cur)
    n = min(l.num_steps for l in loops) if num_steps is None else num_steps
    for _ in range(n):
        for loop, s in zip(loops, streams):
            with torch.cuda.stream(s):
                loop.step_once()
    for s in streams:
        cur.wait_stream(s)
