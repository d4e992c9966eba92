#!/usr/bin/env python3
"""What constant cameras and points cost in both bundle-adjustment forms (toa_ba_run_constant / toa_ba_lists_run_constant, DESIGN
section 17), at the two shapes of bench.py: `ba` (1024 scenes x 8 cameras x 256 points, fp64, the one-workgroup kernel) and `balists`
(4 scenes x 64 cameras x 5 000 points x 6 observations per point, fp64, the bl_* pipeline); benchmark options, bench.py's generators
and seeds.

Arms, alternated in one process after a warm-up of each:
  plain      the plain entry (toa_ba_run / toa_ba_lists_run): the yardstick, and the figure to hold against bench.py of the parent
  no_flags   the new entry with flags of all zeros: the second instantiations of the kernels on the plain entry's trajectories
  cam0       camera 0 of every scene constant (gauge fixing)
  all_points every point constant (localisation against a known map): the cameras decouple

One JSON line per arm and alternation (ms per solve by events, LM iterations per scene), then a summary line per shape: medians of
the alternations, the spread ((max - min) / median), ms per LM iteration, the ratios to plain.

usage: python tools/ba_constant_probe.py [--alternations 5] [--out profiles/r16_ba_constant_probe.jsonl] [--scale 1.0]   (--scale shrinks the batch)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_solve(ta, x0, model, opts, out=None):
    """One solve from x0, timed by events as bench.py times its steps: the caller's Output is reused (none: a fresh one, the warm-up)."""
    x = x0.clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ta.Optimize(x, model, opts, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def shapes(ta, scale):
    from tinyopt_amd import synth
    P, C, N = max(8, int(1024 * scale)), 8, 256
    data, x0, _ = synth.synth_ba(P, C, N, np.float64, seed=0x71940917)
    yield "ba", ta.BundleAdjustment(torch.from_numpy(data).cuda(), C, N), torch.from_numpy(x0).cuda(), P, C, N
    P, C, N, K = 4, 64, max(256, int(5000 * scale)), 6
    intr, oc, op, ouv, x0, _ = synth.synth_ba_lists(P, C, N, K, np.float64, seed=0x71940917)
    model = ta.BundleAdjustmentLists(torch.from_numpy(intr).cuda(), torch.from_numpy(oc).cuda(), torch.from_numpy(op).cuda(), torch.from_numpy(ouv).cuda(), C, N)
    yield "balists", model, torch.from_numpy(x0).cuda(), P, C, N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_ba_constant_probe.jsonl"))
    a = ap.parse_args()
    import tinyopt_amd as ta
    opts = ta.Options.benchmark()
    lines = []
    for shape, plain, x0, P, C, N in shapes(ta, a.scale):
        cam0 = torch.zeros(C, dtype=torch.bool)
        cam0[0] = True
        models = {"plain": plain, "no_flags": plain.with_constant(cameras=torch.zeros(C, dtype=torch.bool), points=torch.zeros(N, dtype=torch.bool)),
                  "cam0": plain.with_constant(cameras=cam0), "all_points": plain.with_constant(points=torch.ones(N, dtype=torch.bool))}
        outs = {k: timed_solve(ta, x0, m, opts)[1] for k, m in models.items()}   # warm-up: workspaces, code objects; each arm's Output
        for k, m in models.items():
            timed_solve(ta, x0, m, opts, outs[k])
        ms, iters = {k: [] for k in models}, {}
        for alt in range(a.alternations):
            for name, m in models.items():
                t, out = timed_solve(ta, x0, m, opts, outs[name])
                ms[name].append(t)
                iters[name] = float(out.num_iters.sum().item()) / P
                line = dict(probe="ba_constant_probe", shape=shape, arm=name, alternation=alt, scenes=P, cameras=C, points=N, dtype="f64",
                            ms_per_solve=round(t, 4), iterations_per_scene=round(iters[name], 3), stops=sorted(set(out.stop_reason.tolist())))
                lines.append(line)
                print(json.dumps(line), flush=True)
        med = {k: statistics.median(v) for k, v in ms.items()}
        summary = dict(probe="ba_constant_probe", shape=shape, arm="summary", alternations=a.alternations, scenes=P, cameras=C, points=N,
                       median_ms_per_solve={k: round(v, 4) for k, v in med.items()},
                       spread={k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
                       iterations_per_scene={k: round(v, 3) for k, v in iters.items()},
                       median_ms_per_iteration={k: round(med[k] / iters[k], 5) for k in med},
                       over_plain_ms_per_solve={k: round(med[k] / med["plain"], 4) for k in med})
        lines.append(summary)
        print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        for line in lines:
            fo.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
