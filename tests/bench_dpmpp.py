"""Second-order SDE-DPM-Solver++ steps on the DDPM noise space, SD1.5 shapes (64 x 64 latents, f16x3): what the order-2 step costs
next to the order-1 step it extends, and what 20 second-order steps cost next to 50 first-order ones.

    python tests/bench_dpmpp.py [--samples 5] [--images 8] [--e2e_samples 2] [--skip_e2e]
captured_step    device ms per captured step, order 1 against order 2: the `p2p` DDPM loop at UNet batch 4 (two prompts under
                 classifier-free guidance) and the LEDITS++ loop at E = 1 and 3 (both masks on), 50 steps, the methods' own skips
extraction       device ms of `DDPMInversion.noise_maps` per image: 50 rows at order 1 against 20 rows at order 2, at 4 and 8 rows
                 per launch (CFG batch 2 K, skip 0)
end_to_end       images/s of `ledits/test.py` and `p2p/test.py --inversion_type ddpm` over `--images` synthetic images, 50 steps at
                 order 1 (the defaults) against `--num_steps 20 --solver_order 2`, each as a child process that saves nothing
The variants of a group take turns within this one process, `samples` times after one untimed turn; device events around each
turn; medians with the spread (max - min) of their samples.  One JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "image-editing-framework_amd")
sys.path.insert(0, os.path.join(PKG, "p2p"))
import torch  # noqa: E402

import ief_amd  # noqa: E402,F401

DEV = torch.device("cuda:0")
CONCEPTS = ["glasses", "a red hat", "snow"]
PROMPTS = ["a photo of a house on a mountain", "a photo of a house on a mountain at fall"]
S = 50


def summary(v, digits=3):
    return {"median": round(statistics.median(v), digits), "spread": round(max(v) - min(v), digits), "samples": len(v)}


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def take_turns(variants, samples):
    for f in variants.values():          # one untimed turn: captures, pools, allocator
        f()
    out = {name: [] for name in variants}
    for _ in range(samples):
        for name, f in variants.items():
            out[name].append(device_ms(f))
    return out


def captured_step(pipe, samples):
    from ief_amd import denoise
    from ief_amd.ledits.model.sd_utils import concept_token_counts, lower_ledits, register_ledits, unregister_ledits
    from ief_amd.p2p.model.sd_utils import _encode_prompts
    s = pipe.unet.config.sample_size
    pipe.scheduler.set_timesteps(S)
    x = torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(3)).to(DEV)
    loops = {}
    with torch.no_grad():
        for order in (1, 2):
            skip = 18
            maps = torch.randn(S - skip, 4, s, s, generator=torch.Generator().manual_seed(4)).to(DEV)
            u, c = _encode_prompts(pipe, PROMPTS)
            lp = denoise.FusedDenoiser(pipe, torch.cat([u, c]), 2, (s, s), [3.5, 15.0], noise_maps=maps, skip=skip, solver_order=order)
            lp.start(x)
            loops[f"p2p_batch_4_order_{order}"] = lp
            skip = 7
            maps = torch.randn(S - skip, 4, s, s, generator=torch.Generator().manual_seed(4)).to(DEV)
            for E in (1, 3):
                u, c = _encode_prompts(pipe, CONCEPTS[:E])
                plan = lower_ledits(pipe.unet, S - skip, concept_token_counts(pipe.tokenizer, CONCEPTS[:E]), 5.0, latent_hw=(s, s))
                register_ledits(pipe, plan)
                lp = denoise.FusedDenoiser(pipe, torch.cat([u[:1], c]), 1, (s, s), None, noise_maps=maps, skip=skip, ledits=plan,
                                           solver_order=order)
                lp.start(x)              # captured while its plan is registered; stepping afterwards does not need the registration
                unregister_ledits(pipe)
                loops[f"ledits_E={E}_order_{order}"] = lp

    def run(lp):
        def f():
            lp.rewind(x)
            for _ in range(lp.num_steps):
                lp.step_once()
        return f

    ms = take_turns({name: run(lp) for name, lp in loops.items()}, samples)
    res = {k: summary([t / loops[k].num_steps for t in v]) for k, v in ms.items()}
    for lp in loops.values():
        lp.release()
    denoise.drop_pool()
    for name in ("p2p_batch_4", "ledits_E=1", "ledits_E=3"):
        res[f"{name}_order_2_minus_order_1"] = round(res[f"{name}_order_2"]["median"] - res[f"{name}_order_1"]["median"], 3)
    res["unit"] = "device ms per captured step, whole-loop replays (32 steps p2p, 43 steps ledits)"
    return res


def extraction(pipe, samples):
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    s = pipe.unet.config.sample_size
    x0 = torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(1)).to(DEV)
    inv = DDPMInversion()

    def variant(steps, order, K):
        def f():
            pipe.scheduler.set_timesteps(steps)
            inv.noise_maps(pipe, x0, [PROMPTS[0]], skip=0, rows_per_launch=K, generator=torch.Generator().manual_seed(2), solver_order=order)
        return f

    variants = {f"S={steps}_order_{order}_K={K}": variant(steps, order, K) for K in (4, 8) for steps, order in ((50, 1), (20, 2))}
    res = {k: summary(v, 2) for k, v in take_turns(variants, samples).items()}
    res["unit"] = "device ms per image (all S rows, CFG batch 2 K, eager launches)"
    return res


def end_to_end(images, samples):
    """each driver as the child process a user starts; its own JSON line carries the images/s of its timed loop"""
    fast = ["--num_steps", "20", "--solver_order", "2"]
    ledits, p2p = [os.path.join(PKG, "ledits", "test.py")], [os.path.join(PKG, "p2p", "test.py"), "--inversion_type", "ddpm"]
    jobs = {"ledits_50_order_1": ledits, "ledits_20_order_2": ledits + fast, "p2p_ddpm_50_order_1": p2p, "p2p_ddpm_20_order_2": p2p + fast}
    rates = {k: [] for k in jobs}
    for _ in range(samples):
        for name, argv in jobs.items():
            with tempfile.TemporaryDirectory(prefix="ief_bench_dpmpp_") as d:
                p = subprocess.run([sys.executable] + argv + ["--sd_version", "1.5", "--synthetic", str(images), "--no_save", "--exp_path", d],
                                   cwd=d, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise RuntimeError(f"{name}: {p.stderr[-2000:]}")
            rates[name].append(json.loads(p.stdout.strip().splitlines()[-1])["images_per_sec"])
    out = {k: summary(v, 4) for k, v in rates.items()}
    out["unit"] = f"images/s over {images} synthetic 512x512 images, one child process per sample (captures included)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--e2e_samples", type=int, default=2)
    ap.add_argument("--skip_e2e", action="store_true")
    a = ap.parse_args()
    if a.samples < 5:
        ap.error("at least 5 samples")
    from _bootstrap import load_pipe, seed_everything
    seed_everything(42)
    pipe = load_pipe("1.5", DEV, precision="f16x3", attn_key_splits=None)
    res = {"workload": "SDE-DPM-Solver++ order 2 on the DDPM noise space, SD1.5 shapes, 64x64 latents, f16x3"}
    res["captured_step"] = captured_step(pipe, a.samples)
    print(json.dumps({"captured_step": res["captured_step"]}), flush=True)
    res["extraction"] = extraction(pipe, a.samples)
    print(json.dumps({"extraction": res["extraction"]}), flush=True)
    del pipe
    torch.cuda.empty_cache()
    if not a.skip_e2e:
        res["end_to_end"] = end_to_end(a.images, a.e2e_samples)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
