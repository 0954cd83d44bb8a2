"""Edit a synthesized image with Prompt-to-Prompt — CLI of `/root/reference/p2p/edit_syn.py`.

Same flags, defaults, hyper-parameters and outputs (`./exp/source.png`, `./exp/edit.png`), plus `--blend_source_words` /
`--blend_target_words` / `--blend_threshold` for `LocalBlend`;
`--device` is the HIP device index.  Phase 1 synthesizes the source image with `EmptyControl`;
phase 2 re-runs with both prompts from the SAME x_T under `AttentionRefine` / `AttentionReplace`.
"""
import argparse
import os

import torch

from _bootstrap import load_pipe, seed_everything

from ief_amd.p2p.model.attention_base import EmptyControl
from ief_amd.p2p.model.attention_control import AttentionRefine, AttentionReplace
from ief_amd.p2p.model.ptp_utils import local_blend_from_words
from ief_amd.p2p.model.sd_utils import P2P, P2P_XL
from ief_amd.p2p.utils.save_image import save_img

parser = argparse.ArgumentParser("General config")
parser.add_argument("--sd_version", type=str, default="1.5")
parser.add_argument("--device", type=int, default=0)
parser.add_argument("--seed", type=int, default=8888)
parser.add_argument("--source_prompt", type=str, default="a photo of a house on a mountain")
parser.add_argument("--target_prompt", type=str, default="a photo of a house on a mountain at fall")
# not a reference flag.  The reference loads the pipeline in fp32 (edit_syn.py:38); the default here is the mode that reproduces
# its images to 4e-6 (bound 1e-3): "f16x3" = fp32 storage, every contraction on split fp16 operands.  "f32" = the same on the
# fp32-input MFMA (2.7x slower); "f16" = fp16 storage with fp32 accumulation (2.5x faster, images within 2 grey levels)
parser.add_argument("--precision", type=str, default=os.environ.get("IEF_PRECISION", "f16x3"), choices=["f16", "f32", "f16x3"])
# not reference flags (its CLIs pass local_blend=None): word-masked latent blending.  Both word lists or neither: the words of the
# source / the target prompt whose cross-attention marks the region the edit may change; outside it the edited latents are the
# source's after every step (`ptp_utils.LocalBlend`)
parser.add_argument("--blend_source_words", type=str, nargs="+", default=None)
parser.add_argument("--blend_target_words", type=str, nargs="+", default=None)
parser.add_argument("--blend_threshold", type=float, default=0.3)


def main(argv=None):
    args = parser.parse_args(argv)
    if (args.blend_source_words is None) != (args.blend_target_words is None):
        parser.error("--blend_source_words and --blend_target_words go together")
    device = torch.device("cuda:{}".format(args.device))
    seed_everything(args.seed)
    source_prompt, target_prompt = [args.source_prompt], [args.target_prompt]
    num_inference_steps, GUIDANCE_SCALE, LOW_RESOURCE = 50, 7.5, False
    out_path = "./exp"
    cross_replace_steps, self_replace_steps = 0.8, 0.4
    edit_type = "refine"  # ["refine", "replace"]

    pipe = load_pipe(args.sd_version, device, precision=args.precision)
    if pipe.__class__.__name__ == "StableDiffusionPipeline":            # dispatch of edit_syn.py:90-93
        editor = P2P(model=pipe, num_inference_steps=num_inference_steps)
    elif pipe.__class__.__name__ == "StableDiffusionXLPipeline":
        editor = P2P_XL(model=pipe, num_inference_steps=num_inference_steps)
    else:
        raise ValueError("please use the right sd_version")

    os.makedirs(out_path, exist_ok=True)
    controller = EmptyControl(LOW_RESOURCE=LOW_RESOURCE)
    image, latent = editor.text2image_ldm_stable(pipe, source_prompt, controller, latent=None,
                                                 num_inference_steps=num_inference_steps,
                                                 guidance_scale=GUIDANCE_SCALE, low_resource=LOW_RESOURCE)
    save_img(image, os.path.join(out_path, "source.png"))

    kw = dict(prompts=source_prompt + target_prompt, tokenizer=pipe.tokenizer, num_steps=num_inference_steps,
              cross_replace_steps=cross_replace_steps, self_replace_steps=self_replace_steps, device=device,
              local_blend=local_blend_from_words(pipe.tokenizer, source_prompt + target_prompt, args.blend_source_words,
                                                 args.blend_target_words, args.blend_threshold, device))
    if edit_type == "replace":
        controller = AttentionReplace(**kw)
    elif edit_type == "refine":
        controller = AttentionRefine(**kw)
    else:
        raise ValueError("Please choose right eidt type")
    image, latent = editor.text2image_ldm_stable(pipe, source_prompt + target_prompt, controller, latent=latent,
                                                 num_inference_steps=num_inference_steps,
                                                 guidance_scale=GUIDANCE_SCALE, low_resource=LOW_RESOURCE)
    save_img(image[1], os.path.join(out_path, "edit.png"))


if __name__ == "__main__":
    main()
