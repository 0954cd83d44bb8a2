"""Edit a real image with LEDITS++: the edit-friendly DDPM inversion under `--source_prompt` (empty by default: only the unconditional
row runs), then the edit from step `--skip` on, every `--edit_prompt` concept pushing the noise estimate inside its own implicit mask
(`ief_amd.ledits.model.sd_utils`).  `--remove IDX ...` reverses the direction of those concepts.  Outputs `./exp/source.png`,
`./exp/inversion.png` (the decode of the encoded image) and `./exp/edit.png`; with `--mask_save_dir D` the masks of every step and
concept as `D/step_XX_concept_Y.png`.  Not for SDXL pipelines.  `--num_steps N --solver_order 2` runs inversion and edit on N steps of the
second-order multistep SDE-DPM-Solver++, the solver the method is published with (about 20 steps), instead of 50 eta = 1 DDPM steps;
`--skip` then defaults to 15 % of N.  That 20 second-order steps edit as well as 50 first-order ones is the paper's claim: the synthetic
weights here cannot show it, so 50 / order 1 stay the defaults."""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "p2p"))
from _bootstrap import load_pipe, seed_everything  # noqa: E402

from ief_amd.control import LEDITS_MAX_CONCEPTS  # noqa: E402
from ief_amd.ledits.model.sd_utils import LEDITS  # noqa: E402
from ief_amd.p2p.utils.save_image import save_img  # noqa: E402
from ief_amd.solver_args import NUM_STEPS, StoreGiven, add_solver_arguments, check_solver_arguments, resolve_skip  # noqa: E402

XL_VERSIONS = ("xl-base", "smallxl")       # the `StableDiffusionXLPipeline` branch of `_bootstrap._build_pipe`


def add_ledits_arguments(ap):
    """the flags both CLIs of this folder share; defaults: the paper's"""
    ap.add_argument("--edit_guidance_scale", type=float, nargs="+", default=[5.0], help="one value, or one per concept")
    ap.add_argument("--remove", type=int, nargs="*", default=[], metavar="IDX", help="concepts (by index) whose direction is reversed")
    ap.add_argument("--edit_threshold", type=float, nargs="+", default=[0.9], help="the masks' quantile; one value, or one per concept")
    ap.add_argument("--edit_warmup_steps", type=int, nargs="+", default=[0], help="edit steps before a concept acts")
    ap.add_argument("--edit_cooldown_steps", type=int, nargs="+", default=None, help="edit step from which a concept no longer acts")
    ap.add_argument("--source_guidance_scale", type=float, default=3.5, help="guidance of the inversion (unused with an empty prompt)")
    ap.add_argument("--skip", type=int, default=7, action=StoreGiven,
                    help="the edit runs the steps from --skip on (default 7 = 15 %% of 50, the paper's setting, int(0.15 N) at another N)")
    add_solver_arguments(ap)
    ap.add_argument("--no_cross_attn_mask", action="store_true", help="no mask from the concept's cross-attention")
    ap.add_argument("--no_intersect_mask", action="store_true", help="no threshold on the concept's own guidance")
    ap.add_argument("--invert_batch", type=int, default=4, help="rows (timesteps) per UNet launch of the inversion")
    ap.add_argument("--precision", type=str, default=os.environ.get("IEF_PRECISION", "f16x3"), choices=["f16", "f32", "f16x3"])


def check_ledits_arguments(ap, args, num_concepts):
    """argparse errors of both CLIs; -> the keyword arguments `LEDITS.__call__` takes"""
    E = num_concepts
    if args.sd_version in XL_VERSIONS:
        ap.error("LEDITS++ is built for the SD1.x / SD2.x pipelines, not for --sd_version " + args.sd_version)
    if not 1 <= E <= LEDITS_MAX_CONCEPTS:
        ap.error(f"--edit_prompt takes 1 .. {LEDITS_MAX_CONCEPTS} concepts")
    for name in ("edit_guidance_scale", "edit_threshold", "edit_warmup_steps", "edit_cooldown_steps"):
        v = getattr(args, name)
        if v is not None and len(v) not in (1, E):
            ap.error(f"--{name} takes one value, or one per concept ({E})")
    if any(not 0.0 <= q <= 1.0 for q in args.edit_threshold):
        ap.error("--edit_threshold is a quantile in [0, 1]")
    if any(n < 0 for n in args.edit_warmup_steps) or any(n < 0 for n in (args.edit_cooldown_steps or [])):
        ap.error("--edit_warmup_steps / --edit_cooldown_steps must be >= 0")
    if any(not 0 <= r < E for r in args.remove):
        ap.error(f"--remove takes concept indices in [0, {E})")
    check_solver_arguments(ap, args)
    args.skip = resolve_skip(args, 0.15)
    if not 0 <= args.skip < args.num_steps:
        ap.error(f"--skip must lie in [0, {args.num_steps}): the edit runs the steps from --skip on")
    if args.invert_batch < 1:
        ap.error("--invert_batch must be >= 1")
    return dict(edit_guidance_scale=list(args.edit_guidance_scale), reverse=list(args.remove), edit_threshold=list(args.edit_threshold),
                edit_warmup_steps=list(args.edit_warmup_steps),
                edit_cooldown_steps=None if args.edit_cooldown_steps is None else list(args.edit_cooldown_steps),
                source_guidance_scale=args.source_guidance_scale, skip=args.skip, cross_attn_mask=not args.no_cross_attn_mask,
                intersect_mask=not args.no_intersect_mask, rows_per_launch=args.invert_batch)


def mask_image(mask, size):
    """mask [h, w] of 0 / 1 -> uint8 [size, size, 3], white = edited (nearest)"""
    m = (mask.detach().cpu().numpy() > 0).astype(np.uint8) * 255
    return np.repeat(np.asarray(Image.fromarray(m).resize((size, size), Image.NEAREST))[:, :, None], 3, axis=2)


def edit_one(pipe, editor, image, source_prompt, edit_prompts, device, kw, seed, keep_masks=False):
    """one PIL image -> (uint8 inversion [H, W, 3], uint8 edit [H, W, 3], per-step masks fp32 [steps, E, h, w] or None)"""
    x0 = editor.image2latent(model=pipe, image=image, device=device, dtype=torch.float32)
    images, _, masks = editor(pipe, x0, edit_prompts, source_prompt=source_prompt, generator=torch.Generator().manual_seed(seed),
                              keep_masks=keep_masks, **kw)
    return editor.latent2image(pipe.vae, x0)[0], images[0], masks


parser = argparse.ArgumentParser("General config")
parser.add_argument("--sd_version", type=str, default="1.5")
parser.add_argument("--device", type=int, default=0)
parser.add_argument("--seed", type=int, default=42)
parser.add_argument("--source_prompt", type=str, default="")
parser.add_argument("--edit_prompt", type=str, nargs="+", default=["glasses"])
parser.add_argument("--source_image", type=str, default="./test.jpg")
parser.add_argument("--mask_save_dir", type=str, default=None, help="write the masks of every step and concept here")
add_ledits_arguments(parser)


def main(argv=None):
    args = parser.parse_args(argv)
    kw = check_ledits_arguments(parser, args, len(args.edit_prompt))
    device = torch.device("cuda:{}".format(args.device))
    seed_everything(args.seed)
    out_path = "./exp"
    pipe = load_pipe(args.sd_version, device, precision=args.precision)
    size = pipe.unet.config.sample_size * pipe.vae_scale_factor
    editor = LEDITS(pipe, args.num_steps, args.solver_order)
    os.makedirs(out_path, exist_ok=True)
    original_image = Image.open(args.source_image).convert("RGB").resize((size, size))
    original_image.save(os.path.join(out_path, "source.png"))
    inversion, edit, masks = edit_one(pipe, editor, original_image, args.source_prompt, args.edit_prompt, device, kw, args.seed,
                                      keep_masks=args.mask_save_dir is not None)
    save_img(inversion, os.path.join(out_path, "inversion.png"))
    save_img(edit, os.path.join(out_path, "edit.png"))
    if masks is not None:
        os.makedirs(args.mask_save_dir, exist_ok=True)
        for i in range(masks.shape[0]):
            for e in range(masks.shape[1]):
                save_img(mask_image(masks[i, e], size), os.path.join(args.mask_save_dir, f"step_{i:02d}_concept_{e}.png"))


if __name__ == "__main__":
    main()
