"""LEDITS++ (Brack, Friedrich, Kornmeier, Tsaban, Schramowski, Kersting, Passos, "LEDITS++: Limitless Image Editing using
Text-to-Image Models", CVPR 2024): the sixth method folder.  No target prompt, no source branch, any number of edit concepts, each
acting only inside an implicit mask.

    editor = LEDITS(pipe, num_steps)
    images, latents, masks = editor(pipe, x0, ["glasses", "hat"], edit_guidance_scale=[5, 7], reverse=[1])

1. Inversion.  The edit-friendly DDPM inversion of `p2p.inversion.ddpm.DDPMInversion` under the source prompt -- by default the
   EMPTY prompt, for which only the unconditional row runs (batch K instead of 2 K).  y_skip and the maps z_skip .. z_{S-1}.
2. Edit step i (timestep `timesteps[skip + i]`), ONE latent x at UNet batch 1 + E = [uncond | concept_1 .. concept_E]:
       M1_e = [smooth(A_e) >= quantile_q(smooth(A_e))]     A_e the 16 x 16 cross-attention mass of concept e's own tokens in THIS step
                                                           (five modules, head-mean), 3 x 3 Gaussian sigma 0.5, reflect padding
       s_e[p] = sum_c |eps_e - eps_u|[c, p] M1_e[cell(p)]; M_e = [s_e >= quantile_q(s_e)] and M1_e
       eps' = eps_u + sum_e scale_e[i] M_e (eps_e - eps_u);  x' = mu(x, eps') + sigma_i z_i
   scale_e[i] is -scale for a removed concept and 0 before its warm-up / from its cool-down step on.  Both quantiles are
   torch.quantile's linear rule with exact order statistics (`ief_ledits_attn_mask_f32`, `ief_ledits_guidance_mask_f32`,
   `ief_ledits_ddpm_step_f32`), all inside the captured step graph of `denoise.FusedDenoiser(ledits=...)`.
   `cross_attn_mask=False` drops M1 (m = 1), `intersect_mask=False` drops the guidance threshold (M_e = M1_e); without both the
   guidance is unmasked.

The cross-attention mask stands where LocalBlend's fused form stands (f16x3, the planes path, SD1.x shape families, 256-query modules
at the configured sample size); anywhere else asking for it is a ValueError.  Without it the method runs in all three precision modes.

Out of scope: SEGA's per-channel quantile, momentum, SDXL pipelines, several images in flight, the masks on top of attention
controllers, the two-GPU CFG split.
"""
import torch

from ...control import ControlPlan, StepCounter, _per_concept, check_ledits, ledits_cross_mask_refusal, ledits_scale_table
from ...denoise import acquire
from ...p2p.inversion.ddim import ddim_inversion
from ...p2p.inversion.ddpm import DDPMInversion
from ...p2p.model.register import _attention_modules, blend_modules
from ...p2p.model.sd_utils import P2P, _encode_prompts


def concept_token_counts(tokenizer, prompts):
    """tokens of each concept between BOS and EOS (the window v_e covers), after the tokenizer's truncation"""
    ids = tokenizer(list(prompts), padding="max_length", max_length=tokenizer.model_max_length, truncation=True,
                    return_tensors="pt").input_ids
    eos = getattr(tokenizer, "eos_token_id", 49407)
    counts = []
    for e, row in enumerate(ids.tolist()):
        n = next((i for i, t in enumerate(row[1:]) if t == eos), len(row) - 2)
        if n < 1:
            raise ValueError(f"LEDITS++: edit concept {e} ({prompts[e]!r}) has no tokens")
        counts.append(n)
    return counts


def lower_ledits(unet, num_steps, token_counts, scales, reverse=(), thresholds=0.9, warmup=0, cooldown=None, cross_attn_mask=True,
                 intersect_mask=True, latent_hw=None):
    """the 'ledits' ControlPlan of an edit of `num_steps` steps (host checks, then device tables); ValueError where the
    cross-attention mask is asked for and cannot be served"""
    E = len(token_counts)
    ths = _per_concept(thresholds, E, "edit_threshold")
    check_ledits(E, ths, sdxl=bool(getattr(getattr(unet, "cfg", None), "addition_embed", False)))
    scs = _per_concept(scales, E, "edit_guidance_scale")
    if latent_hw is None:
        latent_hw = (int(unet.cfg.sample_size),) * 2
    mods = ()
    if cross_attn_mask:
        named = blend_modules(unet)
        why = ledits_cross_mask_refusal(getattr(unet, "precision", None), getattr(unet, "x3p", False),
                                        [(m.heads, m.dim_head, N) for m, N in named], latent_hw)
        if why is not None:
            raise ValueError(f"LEDITS++: {why}")
        mods = tuple(m._exec_index for m, _ in named)
    table = ledits_scale_table(num_steps, scs, reverse, warmup, cooldown)
    return ControlPlan(StepCounter(), "ledits", unet.device, num_steps=num_steps,
                       ledits=dict(scale=table, thresholds=ths, token_counts=list(token_counts), cross_mask=bool(cross_attn_mask),
                                   intersect_mask=bool(intersect_mask), modules=mods, latent_hw=tuple(int(v) for v in latent_hw),
                                   channels=int(unet.config.in_channels)))


def register_ledits(pipe, plan):
    """install the plan on every attention module; ValueError while anything else owns one"""
    unet = pipe.unet
    check_ledits(plan.led["E"], controller=not (all(m.is_native() for m in unet.attention_modules())
                                                and getattr(unet, "_plan", None) is None))
    for _, m in _attention_modules(unet):
        m._plan = plan
    unet._plan = plan
    return plan


def unregister_ledits(pipe):
    for _, m in _attention_modules(pipe.unet):
        m._plan = None
    pipe.unet._plan = None


class LEDITS:
    latent2image = P2P.latent2image             # (vae, latents) -> uint8 [B, H, W, 3]
    image2latent = ddim_inversion.image2latent

    def __init__(self, pipe, num_steps, solver_order=1) -> None:
        """solver_order 2: inversion and edit on the second-order multistep SDE-DPM-Solver++ (the paper's solver, meant for about
        20 steps); 1 (default): the eta = 1 DDPM update"""
        if isinstance(solver_order, bool) or solver_order not in (1, 2):
            raise ValueError(f"LEDITS++: solver_order must be 1 or 2, got {solver_order!r}")
        self.model = pipe
        self.solver_order = solver_order
        pipe.scheduler.set_timesteps(num_steps)

    @torch.no_grad()
    def invert(self, pipe, x0, source_prompt="", source_guidance_scale=3.5, skip=7, rows_per_launch=4, generator=None):
        """-> (y_skip [1, C, h, w], maps fp32 [S - skip, C, h, w]); an empty source prompt runs the unconditional-only extraction"""
        y, maps, _ = DDPMInversion().noise_maps(pipe, x0, [source_prompt], guidance_scale=source_guidance_scale, skip=skip,
                                                rows_per_launch=rows_per_launch, generator=generator,
                                                solver_order=self.solver_order)
        return y, maps

    @torch.no_grad()
    def edit(self, pipe, y_skip, maps, skip, edit_prompts, edit_guidance_scale=5.0, reverse=(), edit_threshold=0.9,
             edit_warmup_steps=0, edit_cooldown_steps=None, cross_attn_mask=True, intersect_mask=True, keep_masks=False,
             use_graph=True):
        """the edit from y_skip on the stored maps -> (final latent [1, C, h, w], per-step masks fp32 [S - skip, E, h, w] or None)"""
        prompts = [edit_prompts] if isinstance(edit_prompts, str) else list(edit_prompts)
        S = len(pipe.scheduler.timesteps)
        hw = tuple(y_skip.shape[-2:])
        plan = lower_ledits(pipe.unet, S - skip, concept_token_counts(pipe.tokenizer, prompts) if prompts else [],
                            edit_guidance_scale, reverse, edit_threshold, edit_warmup_steps, edit_cooldown_steps, cross_attn_mask,
                            intersect_mask, hw)
        uncond, cond = _encode_prompts(pipe, prompts)
        register_ledits(pipe, plan)
        try:
            loop = acquire(pipe, torch.cat([uncond[:1], cond]), 1, hw, None, noise_maps=maps, skip=skip, ledits=plan,
                           use_graph=use_graph, solver_order=self.solver_order)
            try:
                if not keep_masks or not (cross_attn_mask or intersect_mask):
                    return loop.run(y_skip), None
                loop.start(y_skip)
                masks = []
                for _ in range(loop.num_steps):
                    loop.step_once()
                    masks.append(loop.plan.led["mask"].clone())
                return loop.result(), torch.stack(masks)
            finally:
                loop.release()
        finally:
            unregister_ledits(pipe)

    @torch.no_grad()
    def __call__(self, pipe, x0, edit_prompts, edit_guidance_scale=5.0, reverse=(), edit_threshold=0.9, edit_warmup_steps=0,
                 edit_cooldown_steps=None, source_prompt="", source_guidance_scale=3.5, skip=7, cross_attn_mask=True,
                 intersect_mask=True, rows_per_launch=4, generator=None, keep_masks=False, cfg_split_group=None,
                 uncond_embeddings_list=None, source_trajectory=None, edit_mask=None, controller=None):
        """x0 fp32 [1, C, h, w], the encoded image -> (uint8 image [1, H, W, 3], final latent fp32 [1, C, h, w], per-step masks or
        None).  The last five arguments exist to be refused by name: none of them combines with this method."""
        prompts = [edit_prompts] if isinstance(edit_prompts, str) else list(edit_prompts)
        unet = pipe.unet
        check_ledits(len(prompts), _per_concept(edit_threshold, max(len(prompts), 1), "edit_threshold"),
                     sdxl=bool(getattr(getattr(unet, "cfg", None), "addition_embed", False)), cfg_split=cfg_split_group is not None,
                     uncond_list=uncond_embeddings_list, source_trajectory=source_trajectory, edit_mask=edit_mask,
                     controller=controller is not None or getattr(unet, "_plan", None) is not None
                     or not all(m.is_native() for m in unet.attention_modules()))
        if x0.dim() != 4 or x0.shape[0] != 1:
            raise ValueError("LEDITS++: x0 is one encoded image [1, C, h, w]")
        y, maps = self.invert(pipe, x0, source_prompt, source_guidance_scale, skip, rows_per_launch, generator)
        latents, masks = self.edit(pipe, y, maps, skip, prompts, edit_guidance_scale, reverse, edit_threshold, edit_warmup_steps,
                                   edit_cooldown_steps, cross_attn_mask, intersect_mask, keep_masks)
        return self.latent2image(pipe.vae, latents), latents, masks
