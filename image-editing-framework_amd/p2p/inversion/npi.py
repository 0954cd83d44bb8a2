"""Negative-prompt inversion (Miyake, Iohara, Saito, Tanaka, "Negative-prompt Inversion: Fast Image Inversion for Editing with
Text-guided Diffusion Models"): the fifth inversion type.

The DDIM inversion is kept as it is (`ddim_inversion.ddim_inversion_loop`: cond-only on the source prompt, no guidance).  What changes
is the EDIT's context: every UNCONDITIONAL row reads the source prompt's embedding instead of the empty prompt's, so on the source
row eps_u == eps_c, guidance does not act, and the row follows the inversion back -- what null-text inversion optimises for, at the
cost of `--inversion_type ddim`.  The samplers take the embedding as `negative_prompt_embeds=` (`P2P.text2image_ldm_stable`,
`MasaCtrl.__call__`).

Proximal guidance (Han et al., "Improving Tuning-Free Real Image Editing with Proximal Guidance") is built on top: `prox_plan` makes
the `denoise.ProxGuidance` plan of an edit and `source_latent` the encoded image its inversion guidance pulls towards.
"""
import torch

from ...denoise import ProxGuidance
from .ddim import ddim_inversion


def negative_context(context):
    """context: the [2, 77, C] = (uncond, cond) of `ddim_inversion_loop` on the SOURCE prompt -> [1, 77, C], the source embedding"""
    if context.dim() != 3 or context.shape[0] != 2:
        raise ValueError(f"negative_context: expected the inversion's [2, tokens, C] context, got {tuple(context.shape)}")
    return context[1:2].clone()


class NPI(ddim_inversion):
    """`ddim_inversion` plus the source embedding as the edit's negative context: `ddim_inversion_loop` is inherited untouched"""

    def negative_prompt_embeds(self, context):
        return negative_context(context)

    def source_latent(self, latents):
        """the encoded source image z*_0 of `ddim_inversion_loop`'s latents: fp32 [C, h, w]"""
        return latents[0][0].float().contiguous()

    def prox_plan(self, model, mode="l0", quantile=0.7, radius=1, prox_steps=None, recon_lr=1.0, recon_t=400):
        """the `ProxGuidance` plan over the scheduler's current timesteps (None for mode "none")"""
        if mode in (None, "none"):
            return None
        return ProxGuidance.from_schedule(model.scheduler.timesteps.tolist(), mode, quantile, radius, prox_steps, recon_lr, recon_t)
