"""Edit-friendly DDPM inversion (Huberman-Spiegelglas, Kulikov, Michaeli, "An Edit Friendly DDPM Noise Space", CVPR 2024): the
fourth inversion type.

Unlike the DDIM inversion there is NO chain.  With `scheduler.timesteps` in edit order t_0 > ... > t_{S-1}, (a_i, p_i) =
`step_coeffs(t_i)` and the eta = 1 quantities of `DDIMScheduler.ddpm_coeffs` (sigma_i, dir_i), the stored latents are drawn
independently from the encoded image x0,

    y_S = x0,      y_i = sqrt(a_i) x0 + sqrt(1 - a_i) n_i     (n_i: seeded CPU generator, fp32)

and the noise maps follow from one UNet evaluation each, independent of each other:

    eps_i = eps_u + g_src (eps_c - eps_u)                     UNet at (y_i, t_i), source prompt
    mu_i  = sqrt(p_i) (y_i - sqrt(1 - a_i) eps_i) / sqrt(a_i) + dir_i eps_i
    z_i   = (y_{i+1} - mu_i) / sigma_i                        i = skip ... S - 1

So one image gives S - skip rows that run through the UNet K at a time, at CFG batch 2 K with ONE TIMESTEP PER ROW (`temb_row`
with one row per batch row), followed by one `ief_ddpm_noise_maps_f32` launch per chunk: no other inversion here fills the chip
from a single image.  The edit starts from y_skip and runs `timesteps[skip:]`; step i of it is x' = mu_i(x, eps) + sigma_i z_i on
every batch row (`ief_cfg_ddpm_step_f32`), with a guidance scale per row: the source row takes g_src and so reproduces y_{i+1}, ...,
y_S = x0 up to rounding, the target rows take a stronger scale.

The published code zeroes the last map (its final step is deterministic).  Here EVERY map is kept: with z_{S-1} the source row ends
on x0 itself, not on the mean of the last step, which is what "the source row reproduces the image" asks for.

`solver_order=2` extracts the maps of the second-order multistep SDE-DPM-Solver++ instead (the solver LEDITS++ is published with, for
about 20 steps).  Its first-order coefficients ARE sigma_i and dir_i, so only the mean changes, by one term on the x0 predictions of
two consecutive rows:

    x0_i = (y_i - sqrt(1 - a_i) eps_i) / sqrt(a_i);   mu_i = sqrt(p_i) x0_i + dir_i eps_i + c2_i (x0_i - x0_{i-1})

with c2_i from `DDIMScheduler.dpmpp_coeffs` and c2 = 0 on row `skip` and on row S - 1 (`dpmpp_orders`).  x0_{i-1} comes from the UNet
output at row i - 1, not from a stepped latent: still no chain, and one carry buffer hands it from chunk to chunk
(`ief_dpmpp_noise_maps_f32`).  The edit must run the same `skip` at order 2 (`ief_cfg_dpmpp_step_f32`).

Out of scope: SDXL pipelines, eta != 1, chunks that mix rows of several images, solver orders above 2.
"""
import torch

from ... import hip
from .ddim import ddim_inversion


class DDPMInversion(ddim_inversion):
    """`ddim_inversion` (for `image2latent` / `get_context`) plus the noise-map extraction; `ddim_inversion_loop` is inherited
    untouched and not used by it"""

    def sample_xts(self, model, x0, generator=None):
        """x0 [1, C, h, w] (or [C, h, w]) -> fp32 [S + 1, C, h, w] on x0's device: row i < S = sqrt(a_i) x0 + sqrt(1 - a_i) n_i at
        `timesteps[i]`, row S = x0.  The n_i are ONE draw of [S, C, h, w] from a CPU generator (default: seed 0), so a run does not
        depend on the device."""
        x0 = x0.float().reshape(-1, *x0.shape[-2:])
        ts = model.scheduler.timesteps.tolist()
        if generator is None:
            generator = torch.Generator().manual_seed(0)
        if generator.device.type != "cpu":
            raise ValueError("sample_xts: the noise is drawn from a CPU torch.Generator (device-independent runs)")
        noise = torch.randn((len(ts), *x0.shape), generator=generator, dtype=torch.float32)
        a = torch.tensor([model.scheduler.step_coeffs(t)[0] for t in ts], dtype=torch.float32).reshape(-1, 1, 1, 1)
        x0c = x0.cpu()
        xts = torch.sqrt(a) * x0c[None] + torch.sqrt(1.0 - a) * noise
        return torch.cat([xts, x0c[None]]).to(x0.device).contiguous()

    @torch.no_grad()
    def noise_maps(self, model, x0, prompt, guidance_scale=3.5, skip=0, rows_per_launch=4, generator=None, uncond_only=None,
                   solver_order=1):
        """-> (y_skip [1, C, h, w], maps fp32 [S - skip, C, h, w], xts [S + 1, C, h, w]).  guidance_scale 3.5 and skip 0 are the
        paper's extraction defaults (its edits then skip 36 % of the steps).  Rows skip ... S - 1 go through the UNet
        `rows_per_launch` at a time: one forward at batch 2 K = [K unconditional | K conditional] rows with the chunk's K
        time-embedding rows repeated for both halves, then one extraction launch.  The last chunk is simply shorter (eager
        launches: nothing is captured, so nothing needs padding).  uncond_only: None = the unconditional-only form (batch K, one
        half) exactly when the source prompt is empty; False forces both halves (what an empty prompt ran before that form existed);
        True with a non-empty prompt is a ValueError.  solver_order 2: the maps of the second-order multistep SDE-DPM-Solver++
        (`DDIMScheduler.dpmpp_coeffs`; rows skip and S - 1 are order 1, `dpmpp_orders`), for an edit that runs the same skip at
        order 2: the mean of row i takes c2_i (x0_i - x0_{i-1}) with both x0 predictions from the rows' own UNet outputs -- still
        no chain -- and one carry buffer hands x0 from a chunk's last row to the next chunk (`ief_dpmpp_noise_maps_f32`)."""
        unet, sched = model.unet, model.scheduler
        if not (all(m.is_native() for m in unet.attention_modules()) and getattr(unet, "_plan", None) is None):
            raise RuntimeError("DDPMInversion: an attention hook is installed; invert before registering controllers")
        if getattr(getattr(unet, "cfg", None), "addition_embed", False):
            raise ValueError("DDPMInversion: built for the SD1.x / SD2.x pipelines, not for an SDXL UNet")
        ts = sched.timesteps.tolist()
        S = len(ts)
        if not isinstance(skip, int) or not 0 <= skip < S:
            raise ValueError(f"noise_maps: skip must be an integer in [0, {S}), got {skip!r}")
        K = int(rows_per_launch)
        if K < 1:
            raise ValueError("noise_maps: rows_per_launch must be >= 1")
        if isinstance(prompt, str):
            prompt = [prompt]
        if len(prompt) != 1:
            raise ValueError("noise_maps: one image and one source prompt per call")
        dev = unet.device
        xts = self.sample_xts(model, x0.to(dev), generator)
        uncond, cond = self.get_context(model, prompt).chunk(2)
        g = float(guidance_scale)
        if solver_order not in (1, 2):
            raise ValueError(f"noise_maps: solver_order must be 1 or 2, got {solver_order!r}")
        carry = None
        if solver_order == 2:           # rows {a, p, sigma, dir, g, c2}; rows before `skip` are not extracted (placeholders)
            rows = [(0.0,) * 5] * skip + sched.dpmpp_table(skip, 2)
            coef = torch.tensor([[*r[:4], g, r[4]] for r in rows], dtype=torch.float32, device=dev)
            carry = torch.empty(xts.shape[1:], dtype=torch.float32, device=dev)       # first read after row `skip` wrote it
        else:
            coef = torch.tensor([[*sched.ddpm_coeffs(t), g] for t in ts], dtype=torch.float32, device=dev)
        temb = unet.time_rows(torch.tensor(ts, dtype=torch.float32, device=dev))          # [S, width]
        maps = torch.empty(S - skip, *xts.shape[1:], dtype=torch.float32, device=dev)
        # an EMPTY source prompt (LEDITS++'s default) makes the conditional row the unconditional one: eps_u + g (eps_c - eps_u) is
        # eps_u whatever g, so only that row runs -- chunks at batch K instead of 2 K, and the extraction takes eps_u = None
        if uncond_only is None:
            uncond_only = prompt[0] == ""
        elif uncond_only and prompt[0] != "":
            raise ValueError("noise_maps: the unconditional-only form stands for an EMPTY source prompt")

        def extract(eu, ec, y, y_next, rows, out):
            if carry is None:
                hip.ddpm_noise_maps(eu, ec, y, y_next, rows, out=out)
            else:
                hip.dpmpp_noise_maps(eu, ec, y, y_next, rows, carry, out=out)

        ctxs = {}       # one context tensor per chunk size: the cross-attention K/V cache is keyed on the tensor, so the full
        for r0 in range(skip, S, K):      # chunks project their K/V once
            r1 = min(r0 + K, S)
            k = r1 - r0
            y = xts[r0:r1]
            if k not in ctxs:
                halves = [uncond.expand(k, -1, -1)] if uncond_only else [uncond.expand(k, -1, -1), cond.expand(k, -1, -1)]
                ctxs[k] = unet._act(torch.cat(halves).to(dev).contiguous())
            ctx = ctxs[k]
            rows = temb[r0:r1]
            if uncond_only:
                eps = unet(y.contiguous(), encoder_hidden_states=ctx, temb_row=rows.contiguous())["sample"]
                extract(None, eps, y, xts[r0 + 1:r1 + 1], coef[r0:r1], out=maps[r0 - skip:r1 - skip])
                continue
            eps = unet(torch.cat([y, y]), encoder_hidden_states=ctx, temb_row=torch.cat([rows, rows]).contiguous())["sample"]
            extract(eps[:k], eps[k:], y, xts[r0 + 1:r1 + 1], coef[r0:r1], out=maps[r0 - skip:r1 - skip])
        return xts[skip:skip + 1].clone(), maps, xts
