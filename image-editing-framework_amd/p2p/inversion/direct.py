"""Direct Inversion (Ju et al., "Direct Inversion: Boosting Diffusion-based Editing with 3 Lines of Code"): the third inversion type.

The DDIM inversion is kept as it is (`ddim_inversion.ddim_inversion_loop`: cond-only on the source prompt, S + 1 latents
z*_0 = the encoded image ... z*_S = x_T).  What changes is the EDIT: after edit step i the source row of the batch is moved back onto
the stored trajectory,

    row 0:      x'' = x' + (z*_{S-1-i} - x')        fp32, both operations rounded
    rows >= 1:  x'' = x'

inside the launch of the CFG + DDIM update (`ief_cfg_ddim_step_rect_f32`).  No optimisation and no extra UNet pass: the cost of
`--inversion_type ddim`, the source reconstruction of `null-text`.  The samplers take the rows as `source_trajectory=`
(`P2P.text2image_ldm_stable`, `P2P.edit_many`, `MasaCtrl.__call__`); `trajectory()` puts them in the order the edit loop reads.
"""
import torch

from .ddim import ddim_inversion, ddim_inversion_xl


def _trajectory(latents):
    """latents: the S + 1 tensors [B, C, h, w] of `ddim_inversion_loop` -> fp32 [S, C, h, w] (B == 1) or [B, S, C, h, w], row i =
    z*_{S-1-i}: what the source row must hold after edit step i (z*_S = x_T is where the edit starts and is not a row)"""
    if len(latents) < 2:
        raise ValueError("trajectory: needs the latents of at least one inversion step (z*_0 and z*_1)")
    rows = torch.stack([t.float() for t in reversed(latents[:-1])], dim=1)       # [B, S, C, h, w]
    return rows[0].contiguous() if rows.shape[0] == 1 else rows.contiguous()


class DirectInversion(ddim_inversion):
    """`ddim_inversion` whose trajectory the edit re-reads: `ddim_inversion_loop` is inherited untouched"""

    def trajectory(self, latents):
        return _trajectory(latents)


class DirectInversion_XL(ddim_inversion_xl):
    """the same on an SDXL-family pipeline (`ddim_inversion_xl`)"""

    def trajectory(self, latents):
        return _trajectory(latents)
