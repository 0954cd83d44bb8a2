"""DiffEdit (Couairon, Verbeek, Schwenk, Cord, "DiffEdit: Diffusion-based semantic image editing with mask guidance", ICLR 2023): the
fifth method folder.  No attention hooks, no optimisation, no second branch -- and pixels outside the edited object stay the source's
by construction.

    editor = DiffEdit(pipe, num_steps)
    images, latents, masks = editor(pipe, x0, source_prompt, target_prompts)       # uint8 [T, H, W, 3], fp32 [T, C, h, w], [T, h, w]

With S = len(scheduler.timesteps), edit order t_0 > ... > t_{S-1}, (a_i, p_i) = `step_coeffs(t_i)`, x0 the encoded image and
z*_0 = x0, ..., z*_S the latents of the DDIM inversion (cond-only on the source prompt, as everywhere in this repository):

1. Mask (`infer_mask`).  i_m = S - int(S strength_mask), t_m = timesteps[i_m]; n noises n_j, ONE draw [n, C, h, w] from a CPU
   generator; y_j = sqrt(a_m) x0 + sqrt(1 - a_m) n_j; for target prompt k
       d_k[p] = 1 / (n C) sum_j sum_c |eps_c(y_j, t_m, target_k)[c, p] - eps_c(y_j, t_m, source)[c, p]|
       v_k[p] = min(max(d_k[p], 0), ratio mean_p d_k) / (ratio mean_p d_k);        M_k[p] = 1 if v_k[p] > threshold else 0
   Only the CONDITIONAL noise estimates are evaluated.  Published implementations form both estimates under classifier-free guidance
   with the same negative prompt; their difference is then g (eps_c_target - eps_c_source), and g > 0 cancels in v.  So the
   unconditional rows are never run: half the UNet work of the mask pass.  K noisy rows go through the UNet per launch at batch
   (1 + T) K = [K source | K target_1 | ...] with one time-embedding row, followed by T `ief_diffedit_map_accum_f32` launches; T
   `ief_diffedit_mask_f32` launches end the pass.  Identical prompts give mean d = 0, v = NaN, which compares false: a zero mask.
2. Inversion.  skip = S - int(S strength); only the first S - skip inversion steps run.  The edit starts from z*_{S-skip} and runs
   `timesteps[skip:]`; trajectory row i = z*_{S-skip-1-i} (`trajectory`, the convention of Direct Inversion), the last row x0 itself.
3. Edit step i, batch row b = target prompt b:  x_out = M_b[p] != 0 ? x' : z_i[c, p]  with x' the CFG + DDIM update, inside the launch of
   that update (`ief_cfg_ddim_step_masked_f32`, captured in the step graph of `denoise.FusedDenoiser(edit_mask=...)`).  A select: with
   a binary mask it is what M x' + (1 - M) z gives in IEEE arithmetic.  After the last step every background element equals x0 bit
   for bit.

A user-supplied mask (`mask=`, `mask_from_image`) skips part 1 and is shared by every row.

Out of scope: SDXL pipelines, the two-GPU CFG split, several images in flight, controllers or null-text embeddings on top of the mask,
soft masks and mask dilation / blur, inversion under classifier-free guidance.
"""
import numpy as np
import torch
from PIL import Image

from ... import hip
from ...denoise import acquire
from ...p2p.inversion.ddim import ddim_inversion
from ...p2p.inversion.direct import _trajectory
from ...p2p.model.sd_utils import P2P, _encode_prompts


def strength_index(num_steps: int, strength: float) -> int:
    """S - int(S strength): the index into `scheduler.timesteps` a strength in (0, 1] stands for -- the mask's timestep for
    `strength_mask`, the edit's first step (`skip`) for `strength`.  ValueError where no step is left (the index would be S)."""
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength must lie in (0, 1], got {strength!r}")
    i = num_steps - int(num_steps * strength)
    if not 0 <= i < num_steps:
        raise ValueError(f"strength {strength} leaves no step of a {num_steps}-step schedule")
    return i


def trajectory(latents):
    """the S - skip + 1 latents z*_0 ... z*_{S-skip} of a partial inversion [1, C, h, w] -> fp32 [S - skip, C, h, w], row i =
    z*_{S-skip-1-i}: what the background holds after edit step i (z*_{S-skip} is where the edit starts and is not a row)"""
    rows = _trajectory(latents)
    if rows.dim() != 4:
        raise ValueError("trajectory: one image per inversion")
    return rows


def mask_from_image(image, latent_hw):
    """a mask image (path or PIL image; white = edit) -> fp32 [h, w] of 0 / 1: resized to the latent size with nearest, thresholded
    at >= 0.5"""
    if not isinstance(image, Image.Image):
        image = Image.open(image)
    h, w = latent_hw
    arr = np.asarray(image.convert("L").resize((w, h), Image.NEAREST), dtype=np.float32) / 255.0
    return torch.from_numpy((arr >= 0.5).astype(np.float32))


class DiffEdit:
    latent2image = P2P.latent2image             # (vae, latents) -> uint8 [B, H, W, 3]
    image2latent = ddim_inversion.image2latent

    def __init__(self, pipe, num_steps) -> None:
        self.model = pipe
        pipe.scheduler.set_timesteps(num_steps)

    @staticmethod
    def _refuse(pipe, what):
        unet = pipe.unet
        if not (all(m.is_native() for m in unet.attention_modules()) and getattr(unet, "_plan", None) is None):
            raise RuntimeError(f"{what}: an attention hook or control plan is installed; DiffEdit runs the plain UNet")
        if getattr(getattr(unet, "cfg", None), "addition_embed", False):
            raise ValueError(f"{what}: built for the SD1.x / SD2.x pipelines, not for an SDXL UNet")

    @staticmethod
    def _prompts(source_prompt, target_prompts):
        if not isinstance(source_prompt, str):
            if len(source_prompt) != 1:
                raise ValueError("DiffEdit: one image and one source prompt per call")
            source_prompt = source_prompt[0]
        targets = [target_prompts] if isinstance(target_prompts, str) else list(target_prompts)
        if not targets:
            raise ValueError("DiffEdit: at least one target prompt")
        return source_prompt, targets

    @torch.no_grad()
    def infer_mask(self, pipe, x0, source_prompt, target_prompts, num_maps=10, rows_per_launch=10, strength_mask=0.5, ratio=3.0,
                   threshold=0.5, generator=None):
        """x0 [1, C, h, w] (or [C, h, w]) -> (masks fp32 0 / 1 [T, h, w], maps d fp32 [T, h, w]) on the UNet's device.  The noises
        are one draw [num_maps, C, h, w] from a CPU generator (default: seed 0), so a run does not depend on the device."""
        self._refuse(pipe, "DiffEdit.infer_mask")
        unet, sched = pipe.unet, pipe.scheduler
        source_prompt, targets = self._prompts(source_prompt, target_prompts)
        n, K, T = int(num_maps), int(rows_per_launch), len(targets)
        if n < 1 or K < 1:
            raise ValueError("infer_mask: num_maps and rows_per_launch must be >= 1")
        ts = sched.timesteps.tolist()
        t_m = ts[strength_index(len(ts), strength_mask)]
        if generator is None:
            generator = torch.Generator().manual_seed(0)
        if generator.device.type != "cpu":
            raise ValueError("infer_mask: the noise is drawn from a CPU torch.Generator (device-independent runs)")
        dev = unet.device
        x0c = x0.float().reshape(-1, *x0.shape[-2:]).cpu()
        C, h, w = x0c.shape
        noise = torch.randn((n, C, h, w), generator=generator, dtype=torch.float32)
        a = torch.tensor(sched.step_coeffs(t_m)[0], dtype=torch.float32)
        y = (torch.sqrt(a) * x0c[None] + torch.sqrt(1.0 - a) * noise).to(dev).contiguous()
        _, cond = _encode_prompts(pipe, [source_prompt] + targets)               # [1 + T, 77, width]
        temb = unet.time_rows(torch.tensor([t_m], dtype=torch.float32, device=dev))          # one row for the whole batch
        acc = torch.zeros(T, h, w, dtype=torch.float32, device=dev)
        ctxs = {}         # one context tensor per chunk size: the cross-attention K/V cache is keyed on the tensor
        for r0 in range(0, n, K):
            rows = y[r0:r0 + K]
            k = rows.shape[0]
            if k not in ctxs:
                ctxs[k] = unet._act(cond.to(dev).repeat_interleave(k, dim=0).contiguous())
            # fp16 storage: every row is planned as a batch-1 launch plans it, so its eps -- and the map -- does not depend on K
            # (`hip.plans_per_row`; the fp32-storage modes keep K in their last bits, as the batched DDIM inversion does)
            with hip.plans_per_row((1 + T) * k):
                eps = unet(rows.repeat(1 + T, 1, 1, 1), encoder_hidden_states=ctxs[k], temb_row=temb)["sample"]
            for j in range(T):
                hip.diffedit_map_accum(eps[(1 + j) * k:(2 + j) * k], eps[:k], acc[j])
        masks = torch.empty_like(acc)
        for j in range(T):
            hip.diffedit_mask(acc[j], n * C, ratio, threshold, out=masks[j])
        return masks, acc / float(n * C)

    @torch.no_grad()
    def invert(self, pipe, x0, source_prompt, skip):
        """the first S - skip steps of the DDIM inversion of x0 [1, C, h, w] under the source prompt (cond-only) ->
        (z*_{S-skip} [1, C, h, w], trajectory fp32 [S - skip, C, h, w])"""
        self._refuse(pipe, "DiffEdit.invert")
        S = len(pipe.scheduler.timesteps)
        _, cond = _encode_prompts(pipe, [source_prompt])
        loop = acquire(pipe, cond, 1, tuple(x0.shape[-2:]), None, mode="invert")
        try:
            _, latents = loop.run(x0, num_steps=S - skip, keep_all=True)
        finally:
            loop.release()
        return latents[-1], trajectory(latents)

    @torch.no_grad()
    def __call__(self, pipe, x0, source_prompt, target_prompts, mask=None, strength=0.8, guidance_scale=7.5, num_maps=10,
                 rows_per_launch=10, strength_mask=0.5, ratio=3.0, threshold=0.5, generator=None):
        """x0 fp32 [1, C, h, w], the encoded image -> (uint8 images [T, H, W, 3], final latents fp32 [T, C, h, w], masks fp32
        [T, h, w]).  mask: fp32 / bool [h, w] (`mask_from_image`) shared by every target; None infers one per target prompt."""
        self._refuse(pipe, "DiffEdit")
        source_prompt, targets = self._prompts(source_prompt, target_prompts)
        if x0.dim() != 4 or x0.shape[0] != 1:
            raise ValueError("DiffEdit: x0 is one encoded image [1, C, h, w]")
        T, hw = len(targets), tuple(x0.shape[-2:])
        skip = strength_index(len(pipe.scheduler.timesteps), strength)
        dev = pipe.unet.device
        if mask is None:
            masks, _ = self.infer_mask(pipe, x0, source_prompt, targets, num_maps, rows_per_launch, strength_mask, ratio, threshold,
                                       generator)
        else:
            if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != hw:
                raise ValueError(f"DiffEdit: a supplied mask is one tensor [{hw[0]}, {hw[1]}]")
            masks = mask.to(dev).float()[None].expand(T, -1, -1).contiguous()
        start, traj = self.invert(pipe, x0.to(dev).float(), source_prompt, skip)
        uncond, cond = _encode_prompts(pipe, targets)
        loop = acquire(pipe, torch.cat([uncond, cond]), T, hw, float(guidance_scale), source_trajectory=traj,
                       edit_mask=masks, skip=skip)
        try:
            latents = loop.run(start)
        finally:
            loop.release()
        return self.latent2image(pipe.vae, latents), latents, masks
