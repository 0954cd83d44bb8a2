"""Pix2Pix-zero in f16x3: what the fused cross-attention guidance gradient (`hip.cross_map_grad`) is worth.

    python tests/bench_p2pzero_cross_grad.py [--config sd15] [--samples 7] [--iters 20] [--skip_step]
(a) per level: the one fused launch against the launches it replaces -- `hip.attn_bwd(want_dkv=False)` + `hip.attn_map_loss_bwd`
    on materialised maps, what the reverse pass runs with `hip.cross_map_grad_ok` false -- at the four SD1.5 cross-attention
    shapes at B = 2, 8 heads, 77 keys; K / V are column slices of a wide buffer as `grad.UNetAdjoint` hands them over.
(b) whole step: the captured `P2P_Zero` edit step (forward, reverse, SGD step, forward, CFG + DDIM) at the model's own latent
    size, fused against not fused (the predicate patched off while that engine is built; nothing else differs).
Every variant is a captured graph (as the product runs it; `iters` repetitions per graph in (a)), timed with device events on
the replaying stream; the variants take turns within one process, `samples` times; the figures are medians with the spread
(max - min) of their samples.  The recorder's launch counts of one eager edit step are printed for both forms.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ief_amd  # noqa: E402,F401
from ief_amd import hip  # noqa: E402
from ief_amd.pipeline import StableDiffusionPipeline  # noqa: E402
from ief_amd.pix2pix_zero.model.sd_utils import P2P_Zero  # noqa: E402

DEV = torch.device("cuda:0")
LEVELS = [(4096, 40, 8), (1024, 80, 8), (256, 160, 8), (64, 160, 8)]       # (N, d, heads) of SD1.5 at 512^2
PROMPTS = ["a photo of a cat on the grass", "a photo of a dog on the grass"]


def capture(body):
    """warm `body` on a side stream, then capture it (the order of `pix2pix_zero.model.sd_utils._Engine._capture`)"""
    used0 = hip.counters_used()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    arena = hip.counter_arena(hip.counters_used() - used0, DEV)
    g = torch.cuda.CUDAGraph()
    with arena, torch.cuda.graph(g):
        body()
    return g, arena


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def take_turns(variants, samples, per_call):
    """{name: [ms per unit, one entry per sample]}: every variant once per round, `samples` rounds"""
    for f in variants.values():
        f()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(samples):
        for name, f in variants.items():
            ms[name].append(timed_ms(f) / per_call)
    return ms


def summary(v, digits=4):
    return {"median": round(statistics.median(v), digits), "spread": round(max(v) - min(v), digits)}


def level(N, d, heads, samples, iters):
    B, L, C = 2, 77, heads * d
    g = torch.Generator().manual_seed(N + d)
    q, do = torch.randn(B, N, C, generator=g).to(DEV), (torch.randn(B, N, C, generator=g) * 0.01).to(DEV)
    wide = torch.randn(B, L, 4 * C, generator=g).to(DEV)
    k, v = wide[..., C:2 * C], wide[..., 3 * C:]
    ref = torch.softmax(torch.randn(B * heads, N, L, generator=g) * 2.0, -1).to(DEV)
    scale, gcoef, lc = d ** -0.5, 2.0 * 1024.0 / (B * heads), 1.0 / (B * heads)
    dq = torch.empty(B, N, C, device=DEV)
    parts_f = torch.zeros(B * heads * hip.cross_map_grad_blocks(N, d), device=DEV)
    parts_m = torch.zeros(hip.map_loss_blocks_f32(B * heads * N), device=DEV)

    def fused():
        for _ in range(iters):
            hip.cross_map_grad(q, k, v, do, ref, heads, scale, gcoef, dq=dq, loss=parts_f, loss_coef=lc)

    def replaced():
        for _ in range(iters):
            g2, _, _ = hip.attn_bwd(q, k, v, None, do, None, heads, scale, want_dkv=False)
            hip.attn_map_loss_bwd(q, k, ref, g2, heads, scale, gcoef=gcoef, accumulate=True, loss=parts_m, loss_coef=lc)

    with hip.f32_contraction("x3"):
        graphs = {"fused": capture(fused), "replaced": capture(replaced)}
    ms = take_turns({name: gr[0].replay for name, gr in graphs.items()}, samples, iters)
    out = {name: summary([1e3 * x for x in v], 2) for name, v in ms.items()}                 # microseconds
    out["fused_no_slower"] = bool(statistics.median(ms["fused"]) <= statistics.median(ms["replaced"]))
    return out


def edit_engine(pipe, steps, fused):
    """the `_Engine` of a short `P2P_Zero` run with its captured edit graph, and the timed-launch names of one eager edit body"""
    ok = hip.cross_map_grad_ok
    if not fused:
        hip.cross_map_grad_ok = lambda *a, **kw: False          # measurement only: the product has no switch
    try:
        editor = P2P_Zero(pipe, steps)
        x_T = torch.randn(1, 4, pipe.cfg.sample_size, pipe.cfg.sample_size, generator=torch.Generator().manual_seed(5))
        editor(prompt=PROMPTS, num_inference_steps=steps, guidance_scale=7.5, guidance_amount=0.1, latents=x_T, return_latents=True,
               num_steps=2)
        E = next(iter(editor._engines.values()))
        assert all(E.adj._cross_fused) == fused and any(E.adj._cross_fused) == fused
        lat0 = E.lat.clone()
        hip.profile_begin()
        try:
            with torch.no_grad():
                E._edit_body()
        finally:
            names = [r[0] for r in hip.profile_end()]
        E.lat.copy_(lat0)
    finally:
        hip.cross_map_grad_ok = ok
    return editor, E, lat0, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15")
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip_step", action="store_true", help="per-level figures only")
    a = ap.parse_args()
    if a.samples < 5:
        ap.error("at least 5 samples")
    res = {"workload": f"Pix2Pix-zero cross-attention guidance gradient, f16x3, {a.samples} samples"}
    res["per_level_us"] = {f"N={N} d={d} h={h}": level(N, d, h, a.samples, a.iters) for N, d, h in LEVELS}
    if not a.skip_step:
        pipe = StableDiffusionPipeline.from_pretrained(f"synthetic:{a.config}", precision="f16x3")
        ed_f, E_f, lat_f, names_f = edit_engine(pipe, 50, True)
        ed_m, E_m, lat_m, names_m = edit_engine(pipe, 50, False)

        def step(E, lat0):
            def f():
                E.lat.copy_(lat0)
                for _ in range(3):
                    E.edit_step()
            return f
        ms = take_turns({"fused": step(E_f, lat_f), "materialised": step(E_m, lat_m)}, a.samples, 3)
        res["edit_step_ms"] = {name: summary(v, 3) for name, v in ms.items()}
        gain = statistics.median(ms["materialised"]) - statistics.median(ms["fused"])
        res["edit_step_gain_ms"] = round(gain, 3)
        res["edit_step_faster_by_more_than_spread"] = bool(gain > max(max(v) - min(v) for v in ms.values()))
        cross = len(E_f.cross)
        res["timed_launches_per_edit_step"] = {"fused": len(names_f), "materialised": len(names_m), "cross_modules": cross,
                                               "cross_map_grad": sum(n.startswith("cross_map_grad") for n in names_f)}
        ed_f.release(), ed_m.release()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
