"""Null-text optimisation: wall time per IMAGE and inner iteration of the four schedules, at SD1.5 scale.

    python tests/bench_nti_batched.py [--config sd15] [--latent 64] [--precision f16x3] [--iters 30] [--samples 5]
(a) `NullTextOptimizer.run`, one image          (b) `run_many`, 4 images in flight on 4 streams
(c) `BatchedNullTextOptimizer`, K = 2           (d) `BatchedNullTextOptimizer`, K = 4
An inner iteration is what the loops do between two looks at the stop rule: the graph replay(s) and the host read of the
loss(es), which is the device synchronise; the stop itself is disabled, so every sample is `iters` full iterations.  Every
graph is captured and warmed first; the variants take turns within one process, `samples` times; the figure is the median,
and for (b) the spread of its samples is printed too: (d) is faster than (b) only if it is below it by more than that.
Before timing, the batched rows are compared with `run` at this size: 1 timestep x 3 Adam steps, every element whose gradient
is resolved (>= 1e-3 of the largest at each of the steps, the gradients recovered from Adam's first moment of the per-image
run) within 1e-2 of the timestep's movement.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ief_amd  # noqa: E402,F401
from ief_amd.nti import BatchedNullTextOptimizer, NullTextOptimizer  # noqa: E402
from ief_amd.pipeline import StableDiffusionPipeline  # noqa: E402

NOISE, INNER = 1e-3, 3


def single_with_gradients(opt, lats, unc):
    """1 timestep x INNER steps of `run`, plus the mask of the elements with an unresolved gradient at one of the steps"""
    opt.begin(lats, unc)
    opt.outer_begin(0)
    m_prev, unresolved = torch.zeros_like(opt.m), torch.zeros_like(opt.m, dtype=torch.bool)
    for _ in range(INNER):
        opt.inner_step()
        opt.inner_loss()
        g = (opt.m - 0.9 * m_prev) / 0.1            # m_j = beta1 m_(j-1) + (1 - beta1) g_j
        unresolved |= g.abs() < NOISE * g.abs().max()
        m_prev = opt.m.clone()
    opt.outer_end()
    return opt.out[0].clone(), unresolved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15")
    ap.add_argument("--latent", type=int, default=0)
    ap.add_argument("--precision", default="f16x3", choices=["f16", "f16x3", "f32"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--samples", type=int, default=5)
    a = ap.parse_args()
    if a.iters < 30 or a.samples < 5:
        ap.error("at least 30 iterations per sample and 5 samples")
    pipe = StableDiffusionPipeline.from_pretrained(f"synthetic:{a.config}", precision=a.precision)
    cfg = pipe.cfg
    hw = a.latent or cfg.sample_size
    pipe.scheduler.set_timesteps(50)
    g = torch.Generator().manual_seed(0)
    E = 4
    ctxs = [torch.randn(2, 77, cfg.cross_attention_dim, generator=g) * 0.1 for _ in range(E)]
    lats = [[torch.randn(1, 4, hw, hw, generator=g) for _ in range(51)] for _ in range(E)]
    uncs, conds = [c[:1] for c in ctxs], [c[1:] for c in ctxs]
    singles = [NullTextOptimizer(pipe, conds[k], 7.5, (hw, hw)) for k in range(E)]
    batched = {K: BatchedNullTextOptimizer(pipe, conds[0], 7.5, (hw, hw), K) for K in (2, 4)}

    # ---- agreement at this size (also captures and warms every graph)
    refs = [single_with_gradients(singles[k], lats[k], uncs[k]) for k in range(E)]
    worst = {}
    for K, opt in batched.items():
        out = opt.run(lats[:K], uncs[:K], INNER, -1.0, num_outer=1, cond=conds[:K])
        worst[K] = 0.0
        for k in range(K):
            ref, unresolved = refs[k]
            moved = (ref - uncs[k].to(ref.device)).abs().max().item()
            worst[K] = max(worst[K], (out[k][0] - ref).abs()[~unresolved].max().item() / moved)
            assert int(unresolved.sum()) <= 0.05 * unresolved.numel(), "too many unresolved elements for the check to mean much"
        assert worst[K] <= 1e-2, f"K={K}: batched rows differ from run by {worst[K]:.2e} of the movement"

    # ---- timing: every variant is inside timestep 0 with fresh Adam state; the stop rule is not applied
    streams = [torch.cuda.Stream() for _ in range(E)]
    for o in singles:
        o.outer_begin(0)
    for K, opt in batched.items():
        opt.begin(lats[:K], uncs[:K], conds[:K])
        opt.outer_begin(0)
    torch.cuda.synchronize()

    def one(n):
        for _ in range(n):
            singles[0].inner_step()
            singles[0].inner_loss()
        return 1

    def in_flight(n):
        # the interleaving of `nti.run_many` (its loop over inner steps: every image's replay on its own stream, then one loss
        # read per image) with the stop rule left out; `run_many` itself cannot be timed per iteration from outside
        cur = torch.cuda.current_stream()
        for s in streams:
            s.wait_stream(cur)
        for _ in range(n):
            for o, s in zip(singles, streams):
                with torch.cuda.stream(s):
                    o.inner_step()
            for o, s in zip(singles, streams):
                with torch.cuda.stream(s):
                    o.inner_loss()
        for s in streams:
            cur.wait_stream(s)
        return E

    def batch(K):
        def f(n):
            for _ in range(n):
                batched[K].inner_step()
                batched[K].inner_losses()
            return K
        return f

    variants = {"run": one, "run_many_4": in_flight, "batched_2": batch(2), "batched_4": batch(4)}
    for f in variants.values():          # warm every graph on the path that is timed
        f(3)
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(a.samples):
        for name, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            images = f(a.iters)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.iters / images)
    med = {name: statistics.median(v) for name, v in ms.items()}
    b = ms["run_many_4"]
    for o in singles + list(batched.values()):
        o.release()
    print(json.dumps({
        "workload": f"NTI inner iteration, {a.config} latent {hw}x{hw}, {a.precision}, {a.samples} samples x {a.iters} iterations",
        "ms_per_image_iteration": {k: round(v, 3) for k, v in med.items()},
        "run_many_4_spread_ms": round(max(b) - min(b), 3), "run_many_4_samples_ms": [round(v, 3) for v in b],
        "batched_4_samples_ms": [round(v, 3) for v in ms["batched_4"]],
        "batched_4_faster_than_run_many_4": bool(med["run_many_4"] - med["batched_4"] > max(b) - min(b)),
        "batched_vs_run_worst_of_movement": {f"K={K}": float(f"{v:.2e}") for K, v in worst.items()}}))


if __name__ == "__main__":
    main()
