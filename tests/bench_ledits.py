"""LEDITS++ on SD1.5 shapes (64 x 64 latents, f16x3, 50 steps): what the masked multi-concept step, its three small launches, the
unconditional-only extraction and the whole PIE loop cost next to what the repository already had.

    python tests/bench_ledits.py [--samples 5] [--images 8] [--e2e_samples 2] [--skip_e2e]
captured_step    device ms per captured step of the LEDITS++ loop at E = 1, 2, 3 concepts (UNet batch 1 + E, both masks on; E = 1 also
                 without the cross-attention mask, i.e. without the five mass launches) against the captured edit-friendly DDPM step
                 of `p2p` at UNet batch 2 and 4 (one and two prompts under classifier-free guidance; a batch of 3 has no such loop)
mask_and_step    device us of the three launches a + b + c together (E = 1, 2, 3) against the same rule written with torch operations
                 on the device (`torch.quantile`, conv2d with reflect padding), 200 repetitions per sample
extraction       device ms of `DDPMInversion.noise_maps` under the empty prompt at 4 rows per launch: the unconditional-only form
                 (batch K) against both halves (batch 2 K)
end_to_end       images/s of `ledits/test.py`, `diffedit/test.py` and `p2p/test.py --inversion_type ddpm` over `--images` synthetic
                 images, each as a child process that saves nothing
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
S, SKIP, REPS = 50, 7, 200


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
    n = S - SKIP
    x = torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(3)).to(DEV)
    maps = torch.randn(n, 4, s, s, generator=torch.Generator().manual_seed(4)).to(DEV)
    loops = {}
    with torch.no_grad():
        for Bp in (1, 2):
            u, c = _encode_prompts(pipe, PROMPTS[:Bp])
            lp = denoise.FusedDenoiser(pipe, torch.cat([u, c]), Bp, (s, s), [3.5, 15.0][:Bp], noise_maps=maps, skip=SKIP)
            lp.start(x)
            loops[f"p2p_ddpm_batch_{2 * Bp}"] = lp
        for E, cross in ((1, True), (1, False), (2, True), (3, True)):
            u, c = _encode_prompts(pipe, CONCEPTS[:E])
            plan = lower_ledits(pipe.unet, n, concept_token_counts(pipe.tokenizer, CONCEPTS[:E]), 5.0, cross_attn_mask=cross, latent_hw=(s, s))
            register_ledits(pipe, plan)
            lp = denoise.FusedDenoiser(pipe, torch.cat([u[:1], c]), 1, (s, s), None, noise_maps=maps, skip=SKIP, ledits=plan)
            lp.start(x)              # captured while its plan is registered; stepping afterwards does not need the registration
            unregister_ledits(pipe)
            loops[f"ledits_E={E}" + ("" if cross else "_no_cross_mask")] = lp

    def run(lp):
        def f():
            lp.rewind(x)
            for _ in range(n):
                lp.step_once()
        return f

    ms = take_turns({name: run(lp) for name, lp in loops.items()}, samples)
    for lp in loops.values():
        lp.release()
    denoise.drop_pool()
    res = {k: summary([t / n for t in v]) for k, v in ms.items()}
    res["E=1_minus_p2p_batch_2"] = round(res["ledits_E=1"]["median"] - res["p2p_ddpm_batch_2"]["median"], 3)
    res["E=1_mass_launches"] = round(res["ledits_E=1"]["median"] - res["ledits_E=1_no_cross_mask"]["median"], 3)
    res["E=3_minus_p2p_batch_4"] = round(res["ledits_E=3"]["median"] - res["p2p_ddpm_batch_4"]["median"], 3)
    res["unit"] = f"device ms per captured step, {n}-step replays"
    return res


def torch_rule(acc, taps, eps, q, scale, x, coef, z):
    """rules a-c with torch operations on the device: what the three launches replace"""
    E, C, H, W = eps.shape[0] - 1, eps.shape[1], eps.shape[2], eps.shape[3]
    img = torch.nn.functional.pad(acc.reshape(E, 1, 16, 16), (1, 1, 1, 1), mode="reflect")
    sm = torch.nn.functional.conv2d(img, taps.reshape(1, 1, 3, 3)).reshape(E, 256)
    m1 = (sm >= torch.quantile(sm, q, dim=1, keepdim=True)).float()
    m = torch.nn.functional.interpolate(m1.reshape(E, 1, 16, 16), (H, W))[:, 0]
    d = eps[1:] - eps[:1]
    s = d.abs().sum(1) * m
    mask = ((s >= torch.quantile(s.reshape(E, -1), q, dim=1).reshape(E, 1, 1)) & (m != 0)).float()
    e = eps[0] + (scale.reshape(E, 1, 1, 1) * mask[:, None] * d).sum(0)
    x0 = (x - torch.sqrt(1 - coef[0]) * e) / torch.sqrt(coef[0])
    return torch.sqrt(coef[1]) * x0 + coef[3] * e + coef[2] * z


def mask_and_step(samples):
    from ief_amd import hip
    from ief_amd.control import ledits_rank_table, ledits_taps
    g = torch.Generator().manual_seed(7)
    variants = {}
    for E in (1, 2, 3):
        eps = torch.randn(1 + E, 4, 64, 64, generator=g).to(DEV)
        acc = (torch.rand(E, 256, generator=g) + 0.5).to(DEV)
        x, noise = torch.randn(1, 4, 64, 64, generator=g).to(DEV), torch.randn(2, 4, 64, 64, generator=g).to(DEV)
        taps = ledits_taps().to(DEV)
        r1, r2 = ledits_rank_table([0.9] * E, 256).to(DEV), ledits_rank_table([0.9] * E, 4096).to(DEV)
        scale, coef = torch.full((E,), 5.0, device=DEV), torch.tensor([0.55, 0.71, 0.3, 0.4], device=DEV)
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        m1, mask, th, out = torch.empty(E, 256, device=DEV), torch.empty(E, 64, 64, device=DEV), torch.empty(E, device=DEV), torch.empty_like(x)

        def kernels(eps=eps, acc=acc, taps=taps, r1=r1, r2=r2, scale=scale, x=x, coef=coef, noise=noise, step=step, m1=m1, mask=mask, th=th, out=out):
            for _ in range(REPS):
                hip.ledits_attn_mask(acc, taps, r1, out=m1)
                hip.ledits_guidance_mask(eps, m1, r2, out=mask, thres_out=th)
                hip.ledits_ddpm_step(eps, mask, scale, x, coef, noise, step, out=out)

        def rule(eps=eps, acc=acc, taps=taps, scale=scale, x=x, coef=coef, noise=noise):
            for _ in range(REPS):
                torch_rule(acc, taps, eps, 0.9, scale, x[0], coef, noise[0])

        variants[f"kernels_E={E}"] = kernels
        variants[f"torch_E={E}"] = rule
    ms = take_turns(variants, samples)
    res = {k: summary([1000.0 * t / REPS for t in v], 2) for k, v in ms.items()}
    res["unit"] = f"device us per (a + b + c), 64 x 64 latents, {REPS} repetitions per sample, launched from Python (no graph)"
    return res


def extraction(pipe, samples):
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    s = pipe.unet.config.sample_size
    pipe.scheduler.set_timesteps(S)
    x0 = torch.randn(1, 4, s, s, generator=torch.Generator().manual_seed(1)).to(DEV)
    inv = DDPMInversion()
    variants = {name: (lambda uo=uo: inv.noise_maps(pipe, x0, [""], skip=0, rows_per_launch=4, generator=torch.Generator().manual_seed(2),
                                                    uncond_only=uo))
                for name, uo in (("unconditional_only_K=4", None), ("both_halves_K=4", False))}
    res = {k: summary(v, 2) for k, v in take_turns(variants, samples).items()}
    res["unit"] = "device ms per image (50 rows, eager launches)"
    return res


def end_to_end(images, samples):
    """each driver as the child process a user starts; its own JSON line carries the images/s of its timed loop"""
    jobs = {"ledits": [os.path.join(PKG, "ledits", "test.py")],
            "diffedit": [os.path.join(PKG, "diffedit", "test.py")],
            "p2p_ddpm": [os.path.join(PKG, "p2p", "test.py"), "--inversion_type", "ddpm"]}
    rates = {k: [] for k in jobs}
    for _ in range(samples):
        for name, argv in jobs.items():
            with tempfile.TemporaryDirectory(prefix="ief_bench_ledits_") as d:
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
    res = {"workload": "LEDITS++, SD1.5 shapes, 64x64 latents, f16x3, 50 steps, skip 7"}
    res["mask_and_step"] = mask_and_step(a.samples)
    print(json.dumps({"mask_and_step": res["mask_and_step"]}), flush=True)
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
