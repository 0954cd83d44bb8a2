"""Invert a real image, then edit it with MasaCtrl — CLI of `/root/reference/masactrl/edit_real.py` (same flags and
defaults: `--inversion_type` "null-text" (:27), `STEP = 4`, `LAYPER = 10`; outputs `./exp/source.png`,
`./exp/inversion.png`, `./exp/edit.png`).  `--inversion_type direct` (not a reference value): Direct Inversion, the DDIM inversion
whose trajectory the edit's source row is moved back onto after every step (`ief_amd.p2p.inversion.direct`).
`--inversion_type npi` (not a reference value): negative-prompt inversion (`ief_amd.masactrl.inversion.npi`) with proximal guidance
inside the fused step, `--prox l0` by default here (`none`: plain NPI; `l1`: soft thresholding), `--prox_quantile 0.7`,
`--prox_steps A B` (default all), `--recon_lr 1.0` below timestep `--recon_t 400`, `--dilate_mask 1`.  Not for SDXL pipelines."""
import argparse
import os
import sys

import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "p2p"))
from _bootstrap import load_pipe, seed_everything  # noqa: E402

from ief_amd.masactrl.model.attention_control import (MutualSelfAttentionControl, MutualSelfAttentionControlMask,  # noqa: E402
                                                      MutualSelfAttentionControlMaskAuto, MutualSelfAttentionControlUnion,
                                                      load_mask_png)
from ief_amd.masactrl.model.register import regiter_attention_editor_diffusers, unregister_attention_control  # noqa: E402
from ief_amd.masactrl.inversion.npi import NPI  # noqa: E402
from ief_amd.masactrl.model.sd_utils import MasaCtrl, MasaCtrl_NTI, MasaCtrl_XL, MasaCtrl_XL_NTI  # noqa: E402
from ief_amd.p2p.inversion.ddim import ddim_inversion, ddim_inversion_xl  # noqa: E402
from ief_amd.p2p.inversion.direct import DirectInversion, DirectInversion_XL  # noqa: E402
from ief_amd.p2p.inversion.nti import NTI, NTI_XL_5e2 as NTI_XL  # noqa: E402  (this folder's copy: lr 5e-2)
from ief_amd.p2p.utils.save_image import save_img  # noqa: E402
from ief_amd.prox_args import add_prox_arguments, check_prox_arguments  # noqa: E402

parser = argparse.ArgumentParser("General config")
parser.add_argument("--sd_version", type=str, default="1.5")
parser.add_argument("--device", type=int, default=0)
parser.add_argument("--seed", type=int, default=42)
parser.add_argument("--source_prompt", type=str, default="a gray horse in the field")
parser.add_argument("--target_prompt", type=str, default="a whie horse in the field")
parser.add_argument("--source_image", type=str, default="./test.jpg")
parser.add_argument("--inversion_type", type=str, default="null-text")
# optional, both or neither: foreground masks of the source / target image (PNG, thresholded at 0.5) -> mask-guided MasaCtrl
parser.add_argument("--mask_s", type=str, default=None)
parser.add_argument("--mask_t", type=str, default=None)
# --mask_auto: the masks come from the step's own cross-attention maps of the prompt tokens --ref_token_idx (source prompt) and
# --cur_token_idx (target prompt), thresholded at --thres (MutualSelfAttentionControlMaskAuto); not together with --mask_s / --mask_t
parser.add_argument("--mask_auto", action="store_true")
parser.add_argument("--thres", type=float, default=0.1)
parser.add_argument("--ref_token_idx", type=int, nargs="+", default=[1])
parser.add_argument("--cur_token_idx", type=int, nargs="+", default=[1])
parser.add_argument("--mask_save_dir", type=str, default=None)
# --union: the target image attends over the source keys AND its own under one softmax (MutualSelfAttentionControlUnion); start
# step and layer as the plain editor's; not together with --mask_s / --mask_t or --mask_auto
parser.add_argument("--union", action="store_true")
add_prox_arguments(parser, default="l0")

STEP, LAYPER = 4, 10
NUM_INNER_STEPS, EARLY_STOP_EPSILON = 10, 1e-5


def edit_one(pipe, editor, invertor, image, source_prompt, target_prompt, inversion_type, device, size,
             num_inference_steps=50, guidance_scale=7.5, masks=None, auto=None, union=False, prox=None):
    """invert + MasaCtrl-edit one PIL image -> uint8 images [2,H,W,3] (reconstruction, edit); :128-153 of the reference.
    masks: optional (mask_s, mask_t) fp32 [h, w] in {0, 1} -> the mask-guided editor; auto: optional dict(thres=, ref_token_idx=,
    cur_token_idx=, mask_save_dir=) -> the editor that makes its masks from cross-attention; union: the editor with united
    source and target keys; prox: `check_prox_arguments`' dict for inversion_type "npi" (None: plain negative-prompt inversion)"""
    latent = invertor.image2latent(model=pipe, image=image, device=device, dtype=torch.float32)
    latents, context = invertor.ddim_inversion_loop(pipe, latent, source_prompt)
    extra = {}
    if inversion_type == "null-text":
        # before the editor is registered, as in the reference (:143-147)
        extra["uncond_embeddings_list"] = invertor.null_optimization(pipe, latents, context, NUM_INNER_STEPS,
                                                                     EARLY_STOP_EPSILON, guidance_scale)
    elif inversion_type == "direct":
        extra["source_trajectory"] = invertor.trajectory(latents)
    elif inversion_type == "npi":
        extra["negative_prompt_embeds"] = invertor.negative_prompt_embeds(context)
        if prox is not None:
            pipe.scheduler.set_timesteps(num_inference_steps)
            extra["prox"] = invertor.prox_plan(pipe, **prox)
            extra["source_latent"] = invertor.source_latent(latents)
    elif inversion_type != "ddim":
        raise ValueError("Please choose right inversion type")
    init_latent = torch.cat([latents[-1], latents[-1]])
    xl = pipe.__class__.__name__ == "StableDiffusionXLPipeline"          # model_type / LAYPER switch of edit_real.py:96-115
    if auto is not None:
        controller = MutualSelfAttentionControlMaskAuto(STEP, 54 if xl else LAYPER, model_type="SDXL" if xl else "SD", **auto)
    elif masks is not None:
        controller = MutualSelfAttentionControlMask(STEP, 54 if xl else LAYPER, mask_s=masks[0], mask_t=masks[1],
                                                    model_type="SDXL" if xl else "SD")
    elif union:
        controller = MutualSelfAttentionControlUnion(STEP, 54 if xl else LAYPER, model_type="SDXL" if xl else "SD")
    else:
        controller = MutualSelfAttentionControl(STEP, 54 if xl else LAYPER, model_type="SDXL" if xl else "SD")
    regiter_attention_editor_diffusers(editor.model, controller)
    images, _ = editor(prompt=source_prompt + target_prompt, latents=init_latent, guidance_scale=guidance_scale,
                       num_inference_steps=num_inference_steps, height=size, width=size, **extra)
    # the reference leaves the editor hooked; past its last step it is the identity (attention_control.py:56), so
    # dropping it here changes nothing and lets the next image's inversion take the captured-graph path
    unregister_attention_control(editor.model, controller)
    return images


def pick(pipe, inversion_type, num_inference_steps=50):
    """(invertor, editor) for a pipeline class and inversion type — the dispatch of edit_real.py:96-115 / test.py"""
    xl = pipe.__class__.__name__ == "StableDiffusionXLPipeline"
    if inversion_type == "ddim":
        return (ddim_inversion_xl() if xl else ddim_inversion()), (MasaCtrl_XL if xl else MasaCtrl)(pipe, num_inference_steps)
    if inversion_type == "null-text":
        return (NTI_XL() if xl else NTI()), (MasaCtrl_XL_NTI if xl else MasaCtrl_NTI)(pipe, num_inference_steps)
    if inversion_type == "direct":
        return (DirectInversion_XL() if xl else DirectInversion()), (MasaCtrl_XL if xl else MasaCtrl)(pipe, num_inference_steps)
    if inversion_type == "npi" and not xl:
        return NPI(), MasaCtrl(pipe, num_inference_steps)
    raise ValueError("Please choose right inversion type")


def main(argv=None):
    args = parser.parse_args(argv)
    if (args.mask_s is None) != (args.mask_t is None):
        parser.error("--mask_s and --mask_t go together")
    if args.mask_auto and args.mask_s is not None:
        parser.error("--mask_auto makes its own masks: not together with --mask_s / --mask_t")
    if args.union and (args.mask_auto or args.mask_s is not None):
        parser.error("--union takes no masks: not together with --mask_s / --mask_t or --mask_auto")
    prox = check_prox_arguments(parser, args)
    device = torch.device("cuda:{}".format(args.device))
    seed_everything(args.seed)
    num_inference_steps = 50
    out_path = "./exp"
    pipe = load_pipe(args.sd_version, device)
    size = pipe.unet.config.sample_size * pipe.vae_scale_factor
    invertor, editor = pick(pipe, args.inversion_type, num_inference_steps)
    os.makedirs(out_path, exist_ok=True)
    original_image = Image.open(args.source_image).convert("RGB").resize((size, size))
    original_image.save(os.path.join(out_path, "source.png"))
    masks = None if args.mask_s is None else (load_mask_png(args.mask_s, device), load_mask_png(args.mask_t, device))
    images = edit_one(pipe, editor, invertor, original_image, [args.source_prompt], [args.target_prompt],
                      args.inversion_type, device, size, num_inference_steps, masks=masks,
                      auto=dict(thres=args.thres, ref_token_idx=args.ref_token_idx, cur_token_idx=args.cur_token_idx,
                                mask_save_dir=args.mask_save_dir) if args.mask_auto else None, union=args.union, prox=prox)
    save_img(images[0], os.path.join(out_path, "inversion.png"))
    save_img(images[1], os.path.join(out_path, "edit.png"))


if __name__ == "__main__":
    main()
