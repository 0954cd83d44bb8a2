"""Null-text reverse pass in f16x3: what the fused cross-attention backward (`hip.cross_bwd`: main kernel + reducer) is worth.

    python tests/bench_cross_bwd.py [--samples 7] [--iters 20]
Per level and batch, operands as `grad.UNetAdjoint(mode="context")` hands them over -- K / V column slices of a wide buffer,
dK / dV column slices of another -- at the four SD1.5 cross-attention shapes, 8 heads, 77 keys, B = 1 and B = 4: `hip.cross_bwd`
called directly against what it replaces, `hip.attn_bwd(want_dkv=True)` on the materialised maps of `hip._attn_bwd_f32` (reached
by patching `hip.cross_bwd_ok` off while the graphs are captured: measurement only, the product has no switch).  The figures are
what `hip.cross_bwd_ok` was written from: it routes the levels where fused is no slower.
Every variant is a captured graph of `iters` repetitions, timed with device events on the replaying stream; the two take turns
within one process, `samples` times; the figures are microseconds per module, medians with the spread (max - min) of their
samples.  The recorder's timed launches of one eager call are counted for both forms (the materialised form's transposes, softmax
backward and torch copies are launches the recorder does not see; they are counted from the code in DESIGN.md).  One JSON line.
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

DEV = torch.device("cuda:0")
LEVELS = [(4096, 40, 8), (1024, 80, 8), (256, 160, 8), (64, 160, 8)]       # (N, d, heads) of SD1.5 at 512^2
BATCHES = [1, 4]


def capture(body):
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
    for f in variants.values():
        f()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(samples):
        for name, f in variants.items():
            ms[name].append(timed_ms(f) / per_call)
    return ms


def summary(v, digits=2):
    return {"median": round(statistics.median(v), digits), "spread": round(max(v) - min(v), digits)}


def level(B, N, d, heads, samples, iters):
    L, C = 77, heads * d
    g = torch.Generator().manual_seed(N + d)
    q, do = torch.randn(B, N, C, generator=g).to(DEV), (torch.randn(B, N, C, generator=g) * 0.01).to(DEV)
    wide = torch.randn(B, L, 4 * C, generator=g).to(DEV)
    k, v = wide[..., C:2 * C], wide[..., 3 * C:]
    gwide = torch.empty(B, L, 4 * C, device=DEV)
    dk, dv = gwide[..., C:2 * C], gwide[..., 3 * C:]
    scale = d ** -0.5

    def body(form, n):
        def f():
            for _ in range(n):
                if form == "fused":           # called directly: the figures decide which levels `cross_bwd_ok` routes here
                    hip.cross_bwd(q, k, v, do, heads, scale, dk=dk, dv=dv)
                else:
                    hip.attn_bwd(q, k, v, None, do, None, heads, scale, dk=dk, dv=dv)
        return f

    ok = hip.cross_bwd_ok
    graphs, names = {}, {}
    with hip.f32_contraction("x3"):
        hip.cross_bwd_ok = lambda *a, **kw: False
        try:
            for form in ("fused", "replaced"):
                graphs[form] = capture(body(form, iters))
                hip.profile_begin()
                try:
                    body(form, 1)()
                finally:
                    names[form] = [r[0] for r in hip.profile_end()]
        finally:
            hip.cross_bwd_ok = ok
    assert any(n.startswith("cross_bwd_f32_kernel") for n in names["fused"]) and \
        not any(n.startswith("cross_bwd_f32_kernel") for n in names["replaced"])
    ms = take_turns({name: gr[0].replay for name, gr in graphs.items()}, samples, iters)
    out = {name: summary([1e3 * x for x in v]) for name, v in ms.items()}                    # microseconds
    out["timed_launches"] = {form: len(n) for form, n in names.items()}
    out["fused_no_slower"] = bool(statistics.median(ms["fused"]) <= statistics.median(ms["replaced"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.samples < 5:
        ap.error("at least 5 samples")
    res = {"workload": f"cross-attention backward (dQ, dK, dV), f16x3, 77 keys, {a.samples} samples, us per module"}
    for B in BATCHES:
        res[f"B={B}"] = {f"N={N} d={d} h={h}": level(B, N, d, h, a.samples, a.iters) for N, d, h in LEVELS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
