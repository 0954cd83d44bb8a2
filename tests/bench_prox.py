"""What proximal guidance costs: the two launches against the same rule in torch operations, and the captured edit step with and
without them.

    python tests/bench_prox.py [--out FILE.json] [--no-step]

Device events around graph replays, the variants alternating in one process, medians of 5 laps with the spread (min .. max).
  launches   `hip.prox_threshold` + `hip.cfg_ddim_step(prox=)` (l0, q 0.7, radius 1, eta 1) at Bp = 2 and row_elems 16384 / 36864 /
             65536, each also alone, against the rule written with `torch.quantile`, `torch.where` and `max_pool2d`
  step       the captured SD1.5 64 x 64 f16x3 Prompt-to-Prompt step at UNet batch 4 on the NPI context, with and without the plan
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ief_amd  # noqa: E402,F401
from ief_amd import denoise, hip  # noqa: E402
from ief_amd.control import ledits_rank  # noqa: E402

LAPS, REPEATS = 5, 50
DEV = torch.device("cuda:0")


def laps_of(variants, repeats=REPEATS):
    """variants: {name: callable}; every callable is captured `repeats` times in one graph (eagerly timed where capture fails), then
    the graphs are replayed in turn LAPS times -> {name: {"us": median, "min": .., "max": .., "captured": bool}} per call"""
    runs = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        try:
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(st):
                with torch.cuda.graph(g, stream=st):
                    for _ in range(repeats):
                        fn()
            torch.cuda.current_stream().wait_stream(st)
            runs[name] = (g.replay, True)
        except Exception:                      # an operation that syncs cannot be captured: time the launches from Python
            torch.cuda.synchronize()
            runs[name] = ((lambda f=fn: [f() for _ in range(repeats)]), False)
        runs[name][0]()
        torch.cuda.synchronize()
    times = {n: [] for n in runs}
    for _ in range(LAPS):
        for name, (run, _) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / repeats * 1e3)
    return {n: {"us": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2), "captured": runs[n][1]}
            for n, t in times.items()}


def launches(C, h, w, Bp=2, q=0.7, radius=1):
    g = torch.Generator().manual_seed(C * h * w)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    eu, ec, x, z0 = r(Bp, C, h, w), r(Bp, C, h, w), r(Bp, C, h, w), r(C, h, w)
    out, thr = torch.empty_like(x), torch.empty(Bp, device=DEV)
    coef = torch.tensor([0.55, 0.71, 7.5, 1.0, 1.0], device=DEV)
    rank = torch.tensor(list(ledits_rank(q, C * h * w)), dtype=torch.float32, device=DEV)
    sb_f, sa_f, sa_t, sb_t = (1 - coef[0]).sqrt(), coef[0].sqrt(), coef[1].sqrt(), (1 - coef[1]).sqrt()
    first = torch.zeros(Bp, 1, 1, 1, dtype=torch.bool, device=DEV)
    first[0] = True

    def fused():
        hip.prox_threshold(eu, ec, rank, out=thr)
        hip.cfg_ddim_step(eu, ec, x, coef, out=out, prox=(thr, z0, "l0", radius))

    def in_torch():
        d = ec - eu
        a = d.abs()
        lam = torch.quantile(a.flatten(1), q, dim=1).view(-1, 1, 1, 1)
        keep = a > lam
        eps = eu + coef[2] * torch.where(keep | first, d, torch.zeros_like(d))
        x0 = (x - sb_f * eps) / sa_f
        m = F.max_pool2d(keep.float(), 2 * radius + 1, stride=1, padding=radius) > 0
        x0 = torch.where(m | first, x0, x0 - coef[4] * (x0 - z0))
        out.copy_(sa_t * x0 + sb_t * eps)

    res = laps_of({"fused_pair": fused, "torch_rule": in_torch,
                   "threshold_alone": lambda: hip.prox_threshold(eu, ec, rank, out=thr),
                   "prox_step_alone": lambda: hip.cfg_ddim_step(eu, ec, x, coef, out=out, prox=(thr, z0, "l0", radius)),
                   "plain_step": lambda: hip.cfg_ddim_step(eu, ec, x, coef[:3], out=out)})
    return {"row_elems": C * h * w, "Bp": Bp, **res}


def step_times():
    import bench
    from ief_amd.p2p.model.attention_control import AttentionRefine
    from ief_amd.p2p.model.register import register_attention_control
    from ief_amd.p2p.model.sd_utils import _encode_prompts
    pipe, _ = bench.build_pipe("sd15", DEV, 0, 1, precision="f16x3")
    pipe.scheduler.set_timesteps(50)
    x_T = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(8888)).to(DEV)
    z0 = torch.randn(4, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        _, c = _encode_prompts(pipe, bench.PROMPTS)
    ctx = torch.cat([c[:1].expand_as(c), c])
    plan = denoise.ProxGuidance.from_schedule(pipe.scheduler.timesteps.tolist(), "l0", 0.7, 1, None, 1.0, 1000)     # eta on in every step
    loops = {}
    for name, kw in (("npi", {}), ("npi_prox", dict(prox=plan, source_latent=z0))):
        ctrl = AttentionRefine(bench.PROMPTS, pipe.tokenizer, 50, 0.8, 0.4, device=DEV)
        register_attention_control(pipe, ctrl)
        loop = denoise.FusedDenoiser(pipe, ctx, 2, (64, 64), 7.5, use_graph=True, **kw)
        loop.start(x_T)
        for _ in range(5):
            loop.step_once()
        loops[name] = loop
    torch.cuda.synchronize()
    times = {n: [] for n in loops}
    n_steps = 20
    for _ in range(LAPS):
        for name, loop in loops.items():
            loop.rewind(x_T)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_steps):
                loop.step_once()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / n_steps * 1e3)
    return {n: {"us": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)} for n, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    res = {"launches": [launches(*s) for s in ((4, 64, 64), (4, 96, 96), (4, 128, 128))]}
    for row in res["launches"]:
        print(json.dumps(row), flush=True)
    if not args.no_step:
        res["step_sd15_64_f16x3_batch4"] = step_times()
        print(json.dumps(res["step_sd15_64_f16x3_batch4"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
