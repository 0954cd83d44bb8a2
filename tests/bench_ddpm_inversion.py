"""Edit-friendly DDPM inversion on SD1.5 shapes (64 x 64 latents, f16x3, 50 steps): what the chain-free extraction, the edit step with
noise maps and the whole PIE loop cost next to the existing inversion types.

    python tests/bench_ddpm_inversion.py [--samples 5] [--images 8] [--nti_samples 2] [--skip_e2e]
extraction   wall ms per image of `DDPMInversion.noise_maps` (skip 0: 50 rows) at K = 1, 2, 4, 8 rows per launch (CFG batch 2 K,
             eager launches) against the 50-step batch-1 DDIM inversion (`ddim_inversion_loop`, its pooled captured graph)
edit_step    ms per captured step of the two-prompt P2P edit (UNet batch 4) with noise maps against without
end_to_end   images/s of `p2p/test.py`'s `run_items` over `--images` synthetic images (--invert_batch 4 --in_flight 4, nothing saved):
             ddim, direct, ddpm at skip 18 and skip 0, null-text with --nti_batch 4 (`--nti_samples` samples: one costs a minute)
The variants of a group take turns within this one process, `samples` times after one untimed turn; medians with the spread
(max - min) of their samples.  One JSON line.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P2P_DIR = os.path.join(ROOT, "image-editing-framework_amd", "p2p")
sys.path.insert(0, P2P_DIR)
import torch  # noqa: E402

import ief_amd  # noqa: E402,F401

DEV = torch.device("cuda:0")
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]
S = 50


def summary(v, digits=3):
    return {"median": round(statistics.median(v), digits), "spread": round(max(v) - min(v), digits), "samples": len(v)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def take_turns(variants, samples):
    for f in variants.values():          # one untimed turn: captures, pools, allocator
        f()
    out = {name: [] for name in variants}
    for _ in range(samples):
        for name, f in variants.items():
            out[name].append(wall(f))
    return out


def extraction(pipe, samples):
    from ief_amd.p2p.inversion.ddim import ddim_inversion
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    s = pipe.unet.config.sample_size
    x0 = torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(1)).to(DEV)
    pipe.scheduler.set_timesteps(S)
    inv, ddim = DDPMInversion(), ddim_inversion()
    variants = {"ddim_inversion_batch_1": lambda: ddim.ddim_inversion_loop(pipe, x0, [PROMPTS[0]])}
    for K in (1, 2, 4, 8):
        variants[f"ddpm_K={K}"] = (lambda K=K: inv.noise_maps(pipe, x0, [PROMPTS[0]], rows_per_launch=K,
                                                               generator=torch.Generator().manual_seed(2)))
    ms = {k: [1e3 * x for x in v] for k, v in take_turns(variants, samples).items()}
    res = {k: summary(v, 2) for k, v in ms.items()}
    base = statistics.median(ms["ddim_inversion_batch_1"])
    for K in (1, 2, 4, 8):
        med = statistics.median(ms[f"ddpm_K={K}"])
        # a K-row CFG launch against 2 K batch-1 steps of the DDIM inversion
        res[f"ddpm_K={K}"]["launch_vs_2K_batch_1_steps"] = round((med / -(-S // K)) / (2 * K * base / S), 3)
        res[f"ddpm_K={K}"]["vs_ddim_inversion"] = round(med / base, 3)
    res["unit"] = "ms per image (50 rows / 50 steps)"
    return res


def edit_step(pipe, samples):
    from ief_amd import denoise
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.register import register_attention_control, unregister_attention_control
    from ief_amd.p2p.model.sd_utils import _encode_prompts
    s = pipe.unet.config.sample_size
    pipe.scheduler.set_timesteps(S)
    with torch.no_grad():
        u, c = _encode_prompts(pipe, PROMPTS)
    ctx = torch.cat([u, c])
    x = torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(3)).to(DEV)
    maps = torch.randn(S, 4, s, s, generator=torch.Generator().manual_seed(4)).to(DEV)
    loops = {}
    for name, kw, g in (("without_maps", {}, 7.5), ("with_maps", dict(noise_maps=maps, skip=0), (3.5, 15.0))):
        ctrl = AttentionRefine(PROMPTS, pipe.tokenizer, S, 0.8, 0.4, device=DEV)
        register_attention_control(pipe, ctrl)
        lp = denoise.FusedDenoiser(pipe, ctx, 2, (s, s), g, **kw)
        lp.start(x)
        unregister_attention_control(pipe, None)
        loops[name] = (lp, ctrl)

    def run(name):
        lp, ctrl = loops[name]

        def f():
            ctrl.reset()
            lp.rewind(x)
            for _ in range(S):
                lp.step_once()
        return f

    ms = take_turns({name: run(name) for name in loops}, samples)
    for lp, _ in loops.values():
        lp.release()
    denoise.drop_pool()
    res = {k: summary([1e3 * x / S for x in v]) for k, v in ms.items()}
    res["unit"] = "ms per captured step (UNet batch 4), 50-step replays"
    return res


def end_to_end(pipe, images, samples, nti_samples):
    spec = importlib.util.spec_from_file_location("ief_p2p_pie_driver_ddpm_bench", os.path.join(P2P_DIR, "test.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    from ief_amd.p2p.dataset.pie import SyntheticPIE
    from ief_amd.p2p.inversion.ddim import ddim_inversion
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    from ief_amd.p2p.inversion.direct import DirectInversion
    from ief_amd.p2p.inversion.nti import NTI
    from ief_amd.p2p.model.sd_utils import P2P, P2P_NTI
    size = pipe.unet.config.sample_size * pipe.vae_scale_factor
    items = list(SyntheticPIE(tempfile.mkdtemp(prefix="ief_bench_ddpm_"), images, size=size).items)
    ddpm = lambda skip: dict(guidance_src=3.5, guidance_tar=15.0, skip=skip, rows_per_launch=4, seed=42)
    kw = dict(invert_batch=4, in_flight=4)

    def variant(editor_cls, invertor, typ, **extra):
        editor = editor_cls(model=pipe, num_inference_steps=S)
        return lambda: drv.run_items(pipe, editor, invertor, items, size, DEV, typ, **kw, **extra)

    fast = {"ddim": variant(P2P, ddim_inversion(), "ddim"), "direct": variant(P2P, DirectInversion(), "direct"),
            "ddpm_skip_18": variant(P2P, DDPMInversion(), "ddpm", ddpm=ddpm(18)),
            "ddpm_skip_0": variant(P2P, DDPMInversion(), "ddpm", ddpm=ddpm(0))}
    res = {k: summary([images / x for x in v], 4) for k, v in take_turns(fast, samples).items()}
    if nti_samples > 0:
        nti = take_turns({"null_text_nti_batch_4": variant(P2P_NTI, NTI(), "null-text", nti_batch=4)}, nti_samples)
        res.update({k: summary([images / x for x in v], 4) for k, v in nti.items()})
    res["unit"] = f"images/s over {images} synthetic {size}x{size} images, --invert_batch 4 --in_flight 4"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--nti_samples", type=int, default=2)
    ap.add_argument("--skip_e2e", action="store_true")
    a = ap.parse_args()
    if a.samples < 5:
        ap.error("at least 5 samples")
    from _bootstrap import load_pipe, seed_everything
    seed_everything(42)
    pipe = load_pipe("1.5", DEV, precision="f16x3", attn_key_splits=None)
    res = {"workload": "edit-friendly DDPM inversion, SD1.5 shapes, 64x64 latents, f16x3, 50 steps"}
    res["extraction"] = extraction(pipe, a.samples)
    print(json.dumps({"extraction": res["extraction"]}), flush=True)
    res["edit_step"] = edit_step(pipe, a.samples)
    print(json.dumps({"edit_step": res["edit_step"]}), flush=True)
    if not a.skip_e2e:
        res["end_to_end"] = end_to_end(pipe, a.images, a.samples, a.nti_samples)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
