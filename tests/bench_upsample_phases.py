"""Per-call timing of Upsample2D's convolution in the f16x3 mode: today's plan entry against the phase form (tile 13).

    python tests/bench_upsample_phases.py [--out FILE.json] [--only sd15]

For every `|u` shape of the UNets (SD1.5 at 512 px with batch 4 and 2, at 1024 px, SDXL) the launch is timed as the tuner times
plans: cache-cold weight copies (`hip._cold_copies`, every launch streams its weights from HBM as inside a step), 20 warm-up
launches, then HIP events around 100 launches (replayed from one hipGraph, so the host's launch cost is not in the number),
the median of 3 laps.  A `conv|...|u` entry of tuned_plans_x3.json moves to tile 13 only where this table shows it faster.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ief_amd import hip, planes  # noqa: E402

# (group, B, Hi, Wi, C): source image -> output [B, 2Hi, 2Wi, C]
SHAPES = [("sd15", 4, 8, 8, 1280), ("sd15", 4, 16, 16, 1280), ("sd15", 4, 32, 32, 640),
          ("sd15", 2, 8, 8, 1280), ("sd15", 2, 16, 16, 1280), ("sd15", 2, 32, 32, 640),
          ("1024", 4, 16, 16, 1280), ("1024", 4, 32, 32, 1280), ("1024", 4, 64, 64, 640),
          ("1024", 2, 16, 16, 1280), ("1024", 2, 32, 32, 1280), ("1024", 2, 64, 64, 640),
          ("sdxl", 2, 32, 32, 1280), ("sdxl", 2, 64, 64, 640), ("sdxl", 4, 32, 32, 1280), ("sdxl", 4, 64, 64, 640)]
WARMUP, LAUNCHES, LAPS = 20, 100, 3


def time_plan(xp, wc, bias, tile, splits):
    """median over LAPS of the mean us per launch of LAUNCHES graph-replayed launches"""
    def run(i):
        return planes.conv3x3(xp, wc[i % len(wc)], bias, upsample=True, out=True, out_planes=True, tile=tile, splits=splits)
    for i in range(WARMUP):
        run(i)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            for i in range(LAUNCHES):
                run(i)
    torch.cuda.current_stream().wait_stream(st)
    g.replay()
    torch.cuda.synchronize()
    laps = []
    for _ in range(LAPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        laps.append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    return statistics.median(laps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one group: sd15, 1024 or sdxl")
    args = ap.parse_args()
    rows, seen = [], set()
    gen = torch.Generator().manual_seed(0)
    with hip.f32_contraction("x3"):
        for group, B, Hi, Wi, C in SHAPES:
            M, K = B * 4 * Hi * Wi, 9 * C
            key = f"conv|{M}|{C}|{K}|u"
            if (args.only and group != args.only) or key in seen:
                continue
            seen.add(key)
            x = (torch.randn(B, Hi, Wi, C, generator=gen)).cuda()
            w = (torch.randn(C, 3, 3, C, generator=gen) * K ** -0.5).cuda()
            bias = torch.zeros(C, device="cuda")
            xp = planes.split(x)
            wc = hip._cold_copies(w, iters=LAUNCHES)
            cur = planes._plan_table().get(key)
            if cur is None or cur[0] == 13:
                cur = None
            ncb = C // 32
            cands = [(13, sp) for t, sp in planes.candidate_plans(M, C, K, conv=True, ncb=ncb, phase_ok=True) if t == 13]
            if cur is not None:
                for x_ in wc:
                    planes.weight_planes(x_)
                t_cur = time_plan(xp, wc, bias, cur[0], cur[1])
                for x_ in wc:
                    hip._x3_planes.pop((x_.data_ptr(), tuple(x_.shape), float(planes.W_SCALE)), None)
            else:
                t_cur = float("nan")
            for x_ in wc:
                hip.x3_upsample_phase_planes(x_, planes.W_SCALE)
            best = None
            for t, sp in cands:
                us = time_plan(xp, wc, bias, t, sp)
                if best is None or us < best[0]:
                    best = (us, sp)
            row = {"group": group, "key": key, "B": B, "Hi": Hi, "Wi": Wi, "C": C, "current": cur, "current_us": round(t_cur, 1),
                   "phase_splits": best[1], "phase_us": round(best[0], 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del wc, w, x, xp
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
