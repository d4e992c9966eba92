#!/usr/bin/env python3
"""What box bounds cost (toa_jit_lm_run_bounds; csrc/bounds.hpp): the C4 shape as text with its own Jacobian (12 500 problems x n = 50
x 2 000 items, fp32), benchmark options.

Arms, alternated in one process after a warm-up of each:
  plain      toa_jit_lm_run: the kernel without bounds — the yardstick
  unbounded  with_bounds(-inf, +inf): the same trajectories, hence the same pass counts: MILLISECONDS PER SOLVE compare directly
  binding    bounds that bind for about a tenth of the parameters (an interval that ends 0.05 short of the planted solution): another
             problem with other iteration counts, so the figure is MILLISECONDS PER LM ITERATION — the solve's time over its mean passes
             per problem, from the counters (Builds + cost-only Evaluates + Builds served from the memo)

One JSON line per arm and alternation, then a summary line: medians, the spread (max - min over the alternations, relative to the
median), the ratios to plain, and the registers / scratch / occupancy of the bounds kernels of the circle fit, n = 20 fp64 and this
shape (toa_jit_model_stats_bounds), and of this shape's prior and prior + bounds kernels.

usage: python tools/bounds_probe.py [--alternations 5] [--scale 1.0] [--out profiles/r15_bounds_probe.jsonl]   (--scale shrinks P)
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

N, M = 50, 2000
CIRCLE = "const S dx = p[0] - x[0];\nconst S dy = p[1] - x[1];\nr[0] = dx * dx + dy * dy - x[2] * x[2];"


def body(n):
    """a.x + 0.1 sin(a.x) - b with its own Jacobian row."""
    return (f"T t = x[0] * p[0];\nfor (int j = 1; j < {n}; ++j) t += x[j] * p[j];\nT sn, cs; sincos_t(t, &sn, &cs);\nr[0] = t + T(0.1) * sn - p[{n}];\n"
            f"if (want_grad) {{\n  const T sc = T(1) + T(0.1) * cs;\n#pragma unroll\n  for (int j = 0; j < {n}; ++j) J[0][j] = sc * p[j];\n}}")


def timed_solve(ta, x0, model, opts):
    """One solve from x0, timed by events: (seconds, its Output, x)."""
    x = x0.clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ta.Optimize(x, model, opts)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_bounds_probe.jsonl"))
    a = ap.parse_args()
    import tinyopt_amd as ta
    dtype = torch.float32
    P = max(64, int(12500 * a.scale))
    g = torch.Generator(device="cuda").manual_seed(15)
    xs = torch.rand(P, N, device="cuda", dtype=dtype, generator=g) * 2 - 1
    x0 = xs + 0.1 * (torch.rand(P, N, device="cuda", dtype=dtype, generator=g) * 2 - 1)
    data = torch.empty(P, M, N + 1, device="cuda", dtype=dtype)
    for lo in range(0, P, 500):   # (in slices: the temporaries of 12 500 x 2 000 rows at once are several GB)
        hi = min(P, lo + 500)
        A = torch.rand(hi - lo, M, N, device="cuda", dtype=dtype, generator=g) * 2 - 1
        t = (A * xs[lo:hi, None, :]).sum(2)
        data[lo:hi, :, :N] = A
        data[lo:hi, :, N] = t + 0.1 * torch.sin(t) + 0.01 * (torch.rand(hi - lo, M, device="cuda", dtype=dtype, generator=g) * 2 - 1)
    # binding: every tenth parameter (shifted per problem) may not come closer than 0.05 to its planted value from below
    inf = float("inf")
    hi_b = torch.full((P, N), inf, device="cuda", dtype=dtype)
    pick = ((torch.arange(N, device="cuda")[None] + torch.arange(P, device="cuda")[:, None]) % 10) == 0
    hi_b[pick] = (xs - 0.05)[pick]
    res = ta.JitResidual(body(N), n=N, item_scalars=N + 1, dtype=dtype, kind="accumulate")
    plain = res.bind(data)
    models = {"plain": plain, "unbounded": plain.with_bounds(None, None), "binding": plain.with_bounds(None, hi_b)}
    opts = ta.Options.benchmark()
    on_bound = {}

    def arm(name):
        t, out, x = timed_solve(ta, x0, models[name], opts)
        c = out.counters
        passes = float((c[0] + c[1] + c[4]).item())
        if name == "binding":
            on_bound[name] = float((x == hi_b).float().mean().item())
        return t, passes / P, float(out.num_iters.sum().item()) / P, float(c[4].item()) / P

    for name in models:   # warm-up: builds, workspaces, caches
        arm(name)
    lines, per_iter, times, passes = [], {k: [] for k in models}, {k: [] for k in models}, {}
    for alt in range(a.alternations):
        for name in models:
            t, iters, num_iters, reused = arm(name)
            times[name].append(t)
            per_iter[name].append(t / iters)
            passes[name] = iters
            line = dict(probe="bounds_probe", arm=name, alternation=alt, P=P, n=N, m=M, dtype="f32", ms_per_solve=round(t * 1e3, 4),
                        iterations_per_problem=round(iters, 4), num_iters_per_problem=round(num_iters, 4), memo_builds_per_problem=round(reused, 4),
                        ms_per_iteration=round(t * 1e3 / iters, 5))
            lines.append(line)
            print(json.dumps(line), flush=True)
    med = {k: statistics.median(v) for k, v in per_iter.items()}
    med_t = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med_t[k] for k, v in times.items()}
    circle = ta.JitResidual(CIRCLE, n=3, item_scalars=2, dtype=torch.float64)
    row20 = ta.JitResidual(body(20), n=20, item_scalars=21, dtype=torch.float64, kind="accumulate")
    summary = dict(probe="bounds_probe", arm="summary", alternations=a.alternations, P=P, n=N, m=M,
                   median_ms_per_solve={k: round(v * 1e3, 4) for k, v in med_t.items()},
                   median_ms_per_iteration={k: round(v * 1e3, 5) for k, v in med.items()},
                   passes_per_problem={k: round(v, 4) for k, v in passes.items()},
                   spread_ms_per_solve={k: round(v, 4) for k, v in spread.items()},
                   unbounded_over_plain_ms_per_solve=med_t["unbounded"] / med_t["plain"],
                   binding_over_plain_ms_per_iteration=med["binding"] / med["plain"],
                   fraction_of_parameters_on_their_bound=on_bound.get("binding"),
                   stats_plain=res.stats(), stats_bounds=res.stats_bounds(), stats_prior=res.stats_prior(), stats_bounds_prior=res.stats_bounds(with_prior=True),
                   stats_bounds_circle_f64=circle.stats_bounds(),
                   stats_bounds_n20_f64=row20.stats_bounds(), stats_plain_circle_f64=circle.stats(), stats_plain_n20_f64=row20.stats())
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        for line in lines:
            fo.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
