#!/usr/bin/env python3
"""What a run-time model on the large-n pipeline costs (JitResidual(..., large_n=True); csrc/large_model_rows.hpp): the DenseRow
residual as text — with its own Jacobian rows, and differentiated on Jets — against DenseRowNatural, the compiled-in family, on the
same rows.  Benchmark options.

Shapes:
  large256   fp32, 128 problems x n = 256 x m = 8 192
  large128   fp32, 512 x n = 128 x m = 4 096   (the natural route is the one-kernel persistent form here: a larger gap is expected)
  f64_128    fp64, 128 x n = 128 x m = 4 096   (the fp64 Gram of the run-time route, large_model_gram_kernel)

Per shape the arms (natural, manual, ad) are alternated in one process after a warm-up of each.  The figure is MILLISECONDS PER LM
ITERATION: the solve's time over its mean passes per problem, from the counters (Builds + cost-only Evaluates + Builds served from
the memo).  One JSON line per arm and alternation, then a summary line per shape: medians, the spread (max - min over the
alternations, relative to the median), the ratio of the run-time arms to natural, and stats() of the two run-time models.

usage: python tools/large_model_probe.py [--alternations 5] [--scale 1.0] [--shapes large256,large128,f64_128]
                                         [--out profiles/r14_large_model_probe.jsonl]        (--scale shrinks P)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"large256": (torch.float32, 128, 256, 8192), "large128": (torch.float32, 512, 128, 4096), "f64_128": (torch.float64, 128, 128, 4096)}


def manual_body(n):
    return (f"T t = x[0] * p[0];\nfor (int j = 1; j < {n}; ++j) t += x[j] * p[j];\nT sn, cs; sincos_t(t, &sn, &cs);\nr[0] = t + T(0.1) * sn - p[{n}];\n"
            f"if (want_grad) {{\n  const T sc = T(1) + T(0.1) * cs;\n  for (int j = 0; j < {n}; ++j) J[0][j] = sc * p[j];\n}}")


def ad_body(n):
    return f"S t = x[0] * p[0];\nfor (int j = 1; j < {n}; ++j) t = t + x[j] * p[j];\nr[0] = t + T(0.1) * sin(t) - p[{n}];"


def timed_solve(ta, x0, model, opts):
    x = x0.clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ta.Optimize(x, model, opts)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shapes", default="large256,large128,f64_128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_large_model_probe.jsonl"))
    a = ap.parse_args()
    import tinyopt_amd as ta
    opts = ta.Options.benchmark()
    lines = []
    for shape in a.shapes.split(","):
        dtype, P0, n, m = SHAPES[shape]
        P = max(4, int(P0 * a.scale))
        g = torch.Generator(device="cuda").manual_seed(14)
        xs = torch.rand(P, n, device="cuda", dtype=dtype, generator=g) * 2 - 1
        x0 = xs + 0.1 * (torch.rand(P, n, device="cuda", dtype=dtype, generator=g) * 2 - 1)
        A = (torch.rand(P, m, n, device="cuda", dtype=dtype, generator=g) * 2 - 1) / n ** 0.5
        t = (A * xs[:, None, :]).sum(2)
        b = t + 0.1 * torch.sin(t) + 0.01 * (torch.rand(P, m, device="cuda", dtype=dtype, generator=g) * 2 - 1)
        items = torch.cat([A, b[..., None]], -1).contiguous()
        res = {k: ta.JitResidual(body, n=n, item_scalars=n + 1, dtype=dtype, kind=kind, large_n=True)
               for k, body, kind in (("manual", manual_body(n), "accumulate"), ("ad", ad_body(n), "residual"))}
        models = {"natural": ta.DenseRowNatural(A, b), "manual": res["manual"].bind(items), "ad": res["ad"].bind(items)}
        del A, b, t

        def arm(name):
            sec, out = timed_solve(ta, x0, models[name], opts)
            c = out.counters
            passes = float((c[0] + c[1] + c[4]).item())
            return sec, passes / P

        for name in models:   # warm-up: builds, workspaces, caches
            arm(name)
        per_iter, times = {k: [] for k in models}, {k: [] for k in models}
        for alt in range(a.alternations):
            for name in models:
                sec, iters = arm(name)
                times[name].append(sec)
                per_iter[name].append(sec / iters)
                line = dict(probe="large_model_probe", shape=shape, arm=name, alternation=alt, P=P, n=n, m=m, dtype="f32" if dtype == torch.float32 else "f64",
                            ms_per_solve=round(sec * 1e3, 4), iterations_per_problem=round(iters, 4), ms_per_iteration=round(sec * 1e3 / iters, 5))
                lines.append(line)
                print(json.dumps(line), flush=True)
        med = {k: statistics.median(v) for k, v in per_iter.items()}
        summary = dict(probe="large_model_probe", shape=shape, arm="summary", alternations=a.alternations, P=P, n=n, m=m,
                       median_ms_per_iteration={k: round(v * 1e3, 5) for k, v in med.items()},
                       median_ms_per_solve={k: round(statistics.median(v) * 1e3, 4) for k, v in times.items()},
                       spread={k: round((max(v) - min(v)) / med[k], 4) for k, v in per_iter.items()},
                       manual_over_natural=round(med["manual"] / med["natural"], 4), ad_over_natural=round(med["ad"] / med["natural"], 4),
                       stats_manual=res["manual"].stats(), stats_ad=res["ad"].stats())
        lines.append(summary)
        print(json.dumps(summary), flush=True)
        del models, items
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        for line in lines:
            fo.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
