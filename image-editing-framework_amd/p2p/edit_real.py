"""Invert a real image, then edit it with Prompt-to-Prompt — CLI of `/root/reference/p2p/edit_real.py`.

Same flags and defaults (`--inversion_type` defaults to "null-text" as in the reference, :26), same outputs:
`./exp/source.png`, `./exp/inversion.png`, `./exp/edit.png`; plus `--blend_source_words` / `--blend_target_words` /
`--blend_threshold` for `LocalBlend`, and `--inversion_type direct` (not a reference value): Direct Inversion, the DDIM inversion
whose trajectory the edit's source row is moved back onto after every step (`ief_amd.p2p.inversion.direct`), and
`--inversion_type ddpm` (not a reference value): edit-friendly DDPM inversion (`ief_amd.p2p.inversion.ddpm`) -- noise maps extracted
`--invert_batch` rows per UNet launch under `--ddpm_guidance_src`, the edit from step `--skip` on with `--ddpm_guidance_tar` on the
target row; `--seed` also seeds the maps' noise.  Not for SDXL pipelines.  `--num_steps N --solver_order 2` (ddpm only) runs inversion
and edit on N steps of the second-order multistep SDE-DPM-Solver++ (LEDITS++'s solver, meant for about 20 steps) instead of 50 eta = 1
DDPM steps; `--skip` then defaults to 36 % of N.  That 20 second-order steps edit as well as 50 first-order ones is the paper's claim:
the synthetic weights here cannot show it, so 50 / order 1 stay the defaults.
`--inversion_type npi` (not a reference value): negative-prompt inversion (`ief_amd.p2p.inversion.npi`) -- the DDIM inversion, and the
edit's unconditional rows read the source prompt's embedding.  `--prox l0|l1` adds proximal guidance inside the fused step (default
none here): `--prox_quantile 0.7`, `--prox_steps A B` (default all), `--recon_lr 1.0` below timestep `--recon_t 400`, `--dilate_mask 1`.
Not for SDXL pipelines, not with blend words.
"""
import argparse
import os

import torch
from PIL import Image

from _bootstrap import load_pipe, seed_everything

from ief_amd.p2p.inversion.ddim import ddim_inversion, ddim_inversion_xl
from ief_amd.p2p.inversion.ddpm import DDPMInversion
from ief_amd.p2p.inversion.direct import DirectInversion, DirectInversion_XL
from ief_amd.p2p.inversion.npi import NPI
from ief_amd.p2p.inversion.nti import NTI, NTI_XL
from ief_amd.p2p.model.attention_control import AttentionRefine, AttentionReplace
from ief_amd.p2p.model.ptp_utils import local_blend_from_words
from ief_amd.p2p.model.register import unregister_attention_control
from ief_amd.p2p.model.sd_utils import P2P, P2P_NTI, P2P_XL, P2P_XL_NTI
from ief_amd.p2p.utils.save_image import save_img
from ief_amd.prox_args import add_prox_arguments, check_prox_arguments
from ief_amd.solver_args import NUM_STEPS, StoreGiven, add_solver_arguments, check_solver_arguments, resolve_skip

XL_VERSIONS = ("xl-base", "smallxl")       # the `StableDiffusionXLPipeline` branch of `_bootstrap._build_pipe`


def add_ddpm_arguments(ap):
    """the flags of `--inversion_type ddpm` (shared with test.py); defaults: the paper's"""
    add_solver_arguments(ap)
    ap.add_argument("--ddpm_guidance_src", type=float, default=3.5, help="ddpm: guidance scale of the extraction and of the source row")
    ap.add_argument("--ddpm_guidance_tar", type=float, default=15.0, help="ddpm: guidance scale of the target row")
    ap.add_argument("--skip", type=int, default=18, action=StoreGiven,
                    help="ddpm: the edit starts at this step of the --num_steps (default 18 = 36 %% of 50 steps, the paper's setting, "
                         "int(0.36 N) at another N); 0 = from pure noise")


def check_ddpm_arguments(ap, args, nti_batch=1):
    """argparse errors of `--inversion_type ddpm`; -> the keyword arguments `edit_one` takes as `ddpm=`, or None"""
    if args.inversion_type != "ddpm":
        if args.num_steps != NUM_STEPS or args.solver_order != 1:
            ap.error(f"--num_steps / --solver_order belong to --inversion_type ddpm; --inversion_type {args.inversion_type} runs its "
                     f"{NUM_STEPS} DDIM steps")
        return None
    check_solver_arguments(ap, args)
    args.skip = resolve_skip(args, 0.36)
    if nti_batch > 1:
        ap.error("--nti_batch groups null-text optimisations; --inversion_type ddpm runs none (use --invert_batch / --in_flight)")
    if args.sd_version in XL_VERSIONS:
        ap.error("--inversion_type ddpm is built for the SD1.x / SD2.x pipelines, not for --sd_version " + args.sd_version)
    if not 0 <= args.skip < args.num_steps:
        ap.error(f"--skip must lie in [0, {args.num_steps}): the edit runs the steps from --skip on")
    if args.invert_batch < 1:
        ap.error("--invert_batch must be >= 1")
    ddpm = dict(guidance_src=args.ddpm_guidance_src, guidance_tar=args.ddpm_guidance_tar, skip=args.skip,
                rows_per_launch=args.invert_batch, seed=args.seed)
    if args.num_steps != NUM_STEPS:     # the defaults stay out: the dict of a default run is what it always was
        ddpm["num_steps"] = args.num_steps
    if args.solver_order != 1:
        ddpm["solver_order"] = args.solver_order
    return ddpm


parser = argparse.ArgumentParser("General config")
parser.add_argument("--sd_version", type=str, default="1.5")
parser.add_argument("--device", type=int, default=0)
parser.add_argument("--seed", type=int, default=42)
parser.add_argument("--source_prompt", type=str, default="a gray horse in the field")
parser.add_argument("--target_prompt", type=str, default="a whie horse in the field")
parser.add_argument("--source_image", type=str, default="./test.jpg")
parser.add_argument("--inversion_type", type=str, default="null-text")
# not a reference flag; default = the mode that meets the reference's fp32 results to 1e-3 (see edit_syn.py); every inversion
# type runs in every mode (the null-text reverse pass in fp32 for "f16x3" / "f32")
parser.add_argument("--precision", type=str, default=os.environ.get("IEF_PRECISION", "f16x3"), choices=["f16", "f32", "f16x3"])
# not a reference flag; "f16x3": keys of the planes self-attention over several workgroups (the batch-1 inversion steps leave
# most of the chip idle); unset = the IEF_X3P_KEY_SPLITS environment variable, else 1
parser.add_argument("--attn_key_splits", type=str, default=None, choices=["1", "2", "4", "8", "auto"])
# not reference flags (its CLIs pass local_blend=None): word-masked latent blending.  Both word lists or neither: the words of the
# source / the target prompt whose cross-attention marks the region the edit may change; outside it the edited latents are the
# source's after every step (`ptp_utils.LocalBlend`)
parser.add_argument("--blend_source_words", type=str, nargs="+", default=None)
parser.add_argument("--blend_target_words", type=str, nargs="+", default=None)
parser.add_argument("--blend_threshold", type=float, default=0.3)
add_ddpm_arguments(parser)
add_prox_arguments(parser, default="none")
parser.add_argument("--invert_batch", type=int, default=4, help="--inversion_type ddpm: rows (timesteps) per UNet launch, at CFG batch 2 K (8 measured fastest on SD1.5)")


def edit_latent(pipe, editor, x_T, source_prompt, target_prompt, edit_type, device, extra=None, num_inference_steps=50,
                guidance_scale=7.5, cross_replace_steps=0.8, self_replace_steps=0.6, local_blend=None, controller_steps=None):
    """Prompt-to-Prompt edit from an inverted latent x_T [1,4,h,w] -> uint8 images [2,H,W,3] (reconstruction, edit).
    controller_steps: the steps the controller counts when the edit runs only a part of the schedule (ddpm with --skip)"""
    kw = dict(prompts=source_prompt + target_prompt, tokenizer=pipe.tokenizer, num_steps=controller_steps or num_inference_steps,
              cross_replace_steps=cross_replace_steps, self_replace_steps=self_replace_steps, device=device,
              local_blend=local_blend)
    if edit_type == "replace":
        controller = AttentionReplace(**kw)
    elif edit_type == "refine":
        controller = AttentionRefine(**kw)
    else:
        raise ValueError("Please choose right eidt type")
    images, _ = editor.text2image_ldm_stable(pipe, source_prompt + target_prompt, controller, latent=x_T,
                                             num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                             low_resource=False, **(extra or {}))
    controller.reset()
    unregister_attention_control(pipe, controller)
    return images


def npi_extra(pipe, invertor, latents, context, prox, num_inference_steps=50):
    """the sampler arguments of a negative-prompt-inversion edit from the DDIM inversion's (latents, context): the source embedding
    as negative context, and with `prox` (`check_prox_arguments`' dict) the proximal plan and the encoded source"""
    extra = {"negative_prompt_embeds": invertor.negative_prompt_embeds(context)}
    if prox is not None:
        pipe.scheduler.set_timesteps(num_inference_steps)
        extra["prox"] = invertor.prox_plan(pipe, **prox)
        extra["source_latent"] = invertor.source_latent(latents)
    return extra


def ddpm_invert(pipe, invertor, latent, source_prompt, num_inference_steps, ddpm):
    """the noise maps of one encoded image -> (y_skip [1,4,h,w], maps [S - skip,4,h,w])"""
    pipe.scheduler.set_timesteps(num_inference_steps)
    y_skip, maps, _ = invertor.noise_maps(pipe, latent, source_prompt, guidance_scale=ddpm["guidance_src"], skip=ddpm["skip"],
                                          rows_per_launch=ddpm["rows_per_launch"],
                                          generator=torch.Generator().manual_seed(ddpm["seed"]),
                                          solver_order=ddpm.get("solver_order", 1))
    return y_skip, maps


def edit_one(pipe, editor, invertor, image, source_prompt, target_prompt, inversion_type, edit_type, device,
             num_inference_steps=50, guidance_scale=7.5, cross_replace_steps=0.8, self_replace_steps=0.6,
             num_inner_steps=10, early_stop_epsilon=1e-5, local_blend=None, ddpm=None, prox=None):
    """invert + edit one PIL image -> uint8 images [2,H,W,3] (inversion reconstruction, edit).  ddpm: `check_ddpm_arguments`' dict
    for inversion_type "ddpm" (its `seed` seeds this image's noise); prox: `check_prox_arguments`' dict for inversion_type "npi"
    (None: plain negative-prompt inversion)"""
    latent = invertor.image2latent(model=pipe, image=image, device=device, dtype=torch.float32)
    if inversion_type == "ddpm":
        num_inference_steps = ddpm.get("num_steps", num_inference_steps)
        y_skip, maps = ddpm_invert(pipe, invertor, latent, source_prompt, num_inference_steps, ddpm)
        return edit_latent(pipe, editor, y_skip, source_prompt, target_prompt, edit_type, device,
                           dict(noise_maps=maps, skip=ddpm["skip"], solver_order=ddpm.get("solver_order", 1)),
                           num_inference_steps, (ddpm["guidance_src"], ddpm["guidance_tar"]), cross_replace_steps, self_replace_steps,
                           local_blend, controller_steps=num_inference_steps - ddpm["skip"])
    latents, context = invertor.ddim_inversion_loop(pipe, latent, source_prompt)
    extra = {}
    if inversion_type == "null-text":
        extra["uncond_embeddings_list"] = invertor.null_optimization(pipe, latents, context, num_inner_steps,
                                                                     early_stop_epsilon, guidance_scale)
    elif inversion_type == "direct":
        extra["source_trajectory"] = invertor.trajectory(latents)
    elif inversion_type == "npi":
        extra.update(npi_extra(pipe, invertor, latents, context, prox, num_inference_steps))
    elif inversion_type != "ddim":
        raise ValueError("Please choose right inversion type")
    return edit_latent(pipe, editor, latents[-1], source_prompt, target_prompt, edit_type, device, extra,
                       num_inference_steps, guidance_scale, cross_replace_steps, self_replace_steps, local_blend)


def main(argv=None):
    args = parser.parse_args(argv)
    ddpm = check_ddpm_arguments(parser, args)
    prox = check_prox_arguments(parser, args, blend=args.blend_source_words is not None or args.blend_target_words is not None)
    if (args.blend_source_words is None) != (args.blend_target_words is None):
        parser.error("--blend_source_words and --blend_target_words go together")
    device = torch.device("cuda:{}".format(args.device))
    seed_everything(args.seed)
    out_path = "./exp"
    edit_type = "refine"  # ["refine", "replace"]
    pipe = load_pipe(args.sd_version, device, precision=args.precision, attn_key_splits=args.attn_key_splits)
    xl = pipe.__class__.__name__ == "StableDiffusionXLPipeline"          # dispatch of edit_real.py:97-115
    if args.inversion_type == "ddim":
        editor = (P2P_XL if xl else P2P)(model=pipe, num_inference_steps=50)
        invertor = ddim_inversion_xl() if xl else ddim_inversion()
    elif args.inversion_type == "null-text":
        editor = (P2P_XL_NTI if xl else P2P_NTI)(model=pipe, num_inference_steps=50)
        invertor = NTI_XL() if xl else NTI()
    elif args.inversion_type == "direct":
        editor = (P2P_XL if xl else P2P)(model=pipe, num_inference_steps=50)
        invertor = DirectInversion_XL() if xl else DirectInversion()
    elif args.inversion_type == "ddpm":
        editor = P2P(model=pipe, num_inference_steps=args.num_steps)
        invertor = DDPMInversion()
    elif args.inversion_type == "npi":
        editor = P2P(model=pipe, num_inference_steps=50)
        invertor = NPI()
    else:
        raise ValueError("Please choose right inversion type")
    size = pipe.unet.config.sample_size * pipe.vae_scale_factor
    image = Image.open(args.source_image).convert("RGB").resize((size, size))
    os.makedirs(out_path, exist_ok=True)
    image.save(os.path.join(out_path, "source.png"))
    images = edit_one(pipe, editor, invertor, image, [args.source_prompt], [args.target_prompt], args.inversion_type,
                      edit_type, device,
                      local_blend=local_blend_from_words(pipe.tokenizer, [args.source_prompt, args.target_prompt],
                                                         args.blend_source_words, args.blend_target_words, args.blend_threshold,
                                                         device), ddpm=ddpm, prox=prox)
    save_img(images[0], os.path.join(out_path, "inversion.png"))
    save_img(images[1], os.path.join(out_path, "edit.png"))


if __name__ == "__main__":
    main()
