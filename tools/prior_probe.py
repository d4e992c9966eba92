#!/usr/bin/env python3
"""What a Gaussian prior beside the items costs (toa_jit_lm_run_prior; csrc/prior.hpp): the C4 shape as text with its own Jacobian
(12 500 problems x n = 50 x 2 000 items, fp32), benchmark options.

Arms, alternated in one process after a warm-up of each:
  no_prior   toa_jit_lm_run: the kernel without the prior — the yardstick
  diagonal   with_prior(mu, W [P, n]): k = n residuals, nothing off the diagonal
  full       with_prior(mu, W [P, 50, n]): k = 50 rows, W^T W added to every image of H

The prior changes the problem and so the iteration counts: the figure to compare is MILLISECONDS PER LM ITERATION — the solve's time
over its mean iterations per problem, from the pass counters (Builds + cost-only Evaluates + Builds served from the memo).  One JSON
line per arm and alternation, then a summary line: medians, the spread (max - min over the alternations, relative to the median) and
the ratio of every prior arm to no_prior, with the registers / scratch of the three kernels.

usage: python tools/prior_probe.py [--alternations 5] [--scale 1.0] [--out profiles/r13_prior_probe.jsonl]   (--scale shrinks P)
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

N, M, K = 50, 2000, 50


def body(n):
    """a.x + 0.1 sin(a.x) - b with its own Jacobian row."""
    return (f"T t = x[0] * p[0];\nfor (int j = 1; j < {n}; ++j) t += x[j] * p[j];\nT sn, cs; sincos_t(t, &sn, &cs);\nr[0] = t + T(0.1) * sn - p[{n}];\n"
            f"if (want_grad) {{\n  const T sc = T(1) + T(0.1) * cs;\n#pragma unroll\n  for (int j = 0; j < {n}; ++j) J[0][j] = sc * p[j];\n}}")


def timed_solve(ta, x0, model, opts):
    """One solve from x0, timed by events: (seconds, its Output)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_prior_probe.jsonl"))
    a = ap.parse_args()
    import tinyopt_amd as ta
    dtype = torch.float32
    P = max(64, int(12500 * a.scale))
    g = torch.Generator(device="cuda").manual_seed(13)
    xs = torch.rand(P, N, device="cuda", dtype=dtype, generator=g) * 2 - 1
    x0 = xs + 0.1 * (torch.rand(P, N, device="cuda", dtype=dtype, generator=g) * 2 - 1)
    data = torch.empty(P, M, N + 1, device="cuda", dtype=dtype)
    for lo in range(0, P, 500):   # (in slices: the temporaries of 12 500 x 2 000 rows at once are several GB)
        hi = min(P, lo + 500)
        A = torch.rand(hi - lo, M, N, device="cuda", dtype=dtype, generator=g) * 2 - 1
        t = (A * xs[lo:hi, None, :]).sum(2)
        data[lo:hi, :, :N] = A
        data[lo:hi, :, N] = t + 0.1 * torch.sin(t) + 0.01 * (torch.rand(hi - lo, M, device="cuda", dtype=dtype, generator=g) * 2 - 1)
    # a prior of moderate weight about a point near the planted solution: sigma = 0.5 per parameter; the full form is a random
    # well-conditioned 50 x 50 factor of the same scale
    mu = xs + 0.05 * (torch.rand(P, N, device="cuda", dtype=dtype, generator=g) * 2 - 1)
    Wd = torch.full((P, N), 2.0, device="cuda", dtype=dtype)
    Wf = 2.0 * torch.eye(N, device="cuda", dtype=dtype)[None] + 0.2 * (torch.rand(P, K, N, device="cuda", dtype=dtype, generator=g) * 2 - 1)
    res = ta.JitResidual(body(N), n=N, item_scalars=N + 1, dtype=dtype, kind="accumulate")
    plain = res.bind(data)
    models = {"no_prior": plain, "diagonal": plain.with_prior(mu, Wd), "full": plain.with_prior(mu, Wf.contiguous())}
    opts = ta.Options.benchmark()

    def arm(name):
        t, out = timed_solve(ta, x0, models[name], opts)
        c = out.counters
        passes = float((c[0] + c[1] + c[4]).item())
        return t, passes / P, float(out.num_iters.sum().item()) / P, float(c[4].item()) / P

    for name in models:   # warm-up: builds, workspaces, caches
        arm(name)
    lines, per_iter, times = [], {k: [] for k in models}, {k: [] for k in models}
    for alt in range(a.alternations):
        for name in models:
            t, iters, num_iters, reused = arm(name)
            times[name].append(t)
            per_iter[name].append(t / iters)
            line = dict(probe="prior_probe", arm=name, alternation=alt, P=P, n=N, m=M, k=0 if name == "no_prior" else (N if name == "diagonal" else K),
                        dtype="f32", ms_per_solve=round(t * 1e3, 4), iterations_per_problem=round(iters, 4), num_iters_per_problem=round(num_iters, 4),
                        memo_builds_per_problem=round(reused, 4), ms_per_iteration=round(t * 1e3 / iters, 5))
            lines.append(line)
            print(json.dumps(line), flush=True)
    med = {k: statistics.median(v) for k, v in per_iter.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in per_iter.items()}
    summary = dict(probe="prior_probe", arm="summary", alternations=a.alternations, P=P, n=N, m=M, k_full=K,
                   median_ms_per_iteration={k: round(v * 1e3, 5) for k, v in med.items()},
                   median_ms_per_solve={k: round(statistics.median(v) * 1e3, 4) for k, v in times.items()},
                   spread={k: round(v, 4) for k, v in spread.items()},
                   diagonal_over_no_prior=med["diagonal"] / med["no_prior"], full_over_no_prior=med["full"] / med["no_prior"],
                   bytes_ratio_full=(K * N + N) / (M * (N + 1)),
                   stats_no_prior=res.stats(), stats_prior=res.stats_prior())
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        for line in lines:
            fo.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
