#!/usr/bin/env python3
"""Throughput of a ragged batch (toa_jit_lm_run_ragged; csrc/ragged.hpp) beside the uniform path on the same body: the C4 shape as text
with its own Jacobian (n = 50, fp32), 12 500 problems whose item counts are drawn uniformly from 200..3 800 (seeded; mean 2 000).

Arms, alternated in one process after a warm-up of each:
  longest_first   the ragged run, problems handed out longest first (the default)
  keep_order      the ragged run, problems handed out in index order (TOA_RAGGED_KEEP_ORDER)
  uniform         12 500 x 2 000 items through toa_jit_lm_run: existing code streaming the same number of bytes — the yardstick
  per_count       a seeded 64-problem subset of the ragged data solved the only way there was before: one uniform call per distinct
                  count (beside the same 64 problems as one ragged call)

One JSON line per arm and alternation (ms per solve, item-passes/s from the pass counters), then a summary line: medians, the
ragged-to-uniform ratio and the spread (max - min over the alternations, relative to the median) of every arm.

usage: python tools/ragged_probe.py [--alternations 5] [--scale 1.0] [--out profiles/r12_ragged_probe.jsonl]   (--scale shrinks P)
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

N, LO, HI, MEAN = 50, 200, 3800, 2000


def body(n):
    """a.x + 0.1 sin(a.x) - b with its own Jacobian row."""
    return (f"T t = x[0] * p[0];\nfor (int j = 1; j < {n}; ++j) t += x[j] * p[j];\nT sn, cs; sincos_t(t, &sn, &cs);\nr[0] = t + T(0.1) * sn - p[{n}];\n"
            f"if (want_grad) {{\n  const T sc = T(1) + T(0.1) * cs;\n#pragma unroll\n  for (int j = 0; j < {n}; ++j) J[0][j] = sc * p[j];\n}}")


def timed_solve(ta, x0, model, opts, **kw):
    """One solve from x0, timed by events: (seconds, its Output)."""
    x = x0.clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ta.Optimize(x, model, opts, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_ragged_probe.jsonl"))
    a = ap.parse_args()
    import tinyopt_amd as ta
    dtype = torch.float32
    P = max(64, int(12500 * a.scale))
    rng = np.random.default_rng(12)
    counts = rng.integers(LO, HI + 1, P)
    total = int(counts.sum())
    g = torch.Generator(device="cuda").manual_seed(12)
    # items: rows a in [-1, 1]^n, b = the residual-free value at a planted x* plus noise (a DenseRow problem per count)
    xs = torch.rand(P, N, device="cuda", dtype=dtype, generator=g) * 2 - 1
    x0 = xs + 0.1 * (torch.rand(P, N, device="cuda", dtype=dtype, generator=g) * 2 - 1)

    def make_items(xstar_rows, rows):
        A = torch.rand(rows, N, device="cuda", dtype=dtype, generator=g) * 2 - 1
        t = (A * xstar_rows).sum(1)
        b = t + 0.1 * torch.sin(t) + 0.01 * (torch.rand(rows, device="cuda", dtype=dtype, generator=g) * 2 - 1)
        return torch.cat([A, b[:, None]], 1)

    owner = torch.repeat_interleave(torch.arange(P, device="cuda"), torch.from_numpy(counts).cuda())
    data_r = make_items(xs[owner], total)
    data_u = make_items(xs.repeat_interleave(MEAN, 0), P * MEAN).reshape(P, MEAN, N + 1)
    res = ta.JitResidual(body(N), n=N, item_scalars=N + 1, dtype=dtype, kind="accumulate")
    ragged = res.bind_ragged(data_r, counts=counts)
    uniform = res.bind(data_u)
    opts = ta.Options.benchmark()
    # the 64-problem subset: one uniform call per distinct count, beside the same problems as one ragged call
    sub = np.sort(np.random.default_rng(64).choice(P, 64, replace=False))
    off = ragged.offsets_host.numpy()
    sub_items = [data_r[off[p]:off[p + 1]] for p in sub]
    sub_ragged = res.bind_ragged(torch.cat(sub_items, 0), counts=counts[sub])
    groups = {}
    for k, p in enumerate(sub):
        groups.setdefault(int(counts[p]), []).append(k)
    sub_models = [(ks, res.bind(torch.stack([sub_items[k] for k in ks], 0))) for ks in groups.values()]
    x0_sub = x0[torch.from_numpy(sub).cuda()]

    def arm_ragged(keep):
        t, out = timed_solve(ta, x0, ragged, opts, keep_order=keep)
        # (benchmark options: no cost threshold, ten iterations — the passes per problem hardly vary, so mean passes x items it is)
        return t, float((out.counters[0] + out.counters[1]).item()) / P * total

    def arm_uniform():
        t, out = timed_solve(ta, x0, uniform, opts)
        return t, float((out.counters[0] + out.counters[1]).item()) * MEAN

    def arm_sub_ragged():
        t, _ = timed_solve(ta, x0_sub, sub_ragged, opts)
        return t, 0.0

    def arm_per_count():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        xs_ = [x0_sub[torch.tensor(ks, device="cuda")].clone() for ks, _ in sub_models]
        e0.record()
        for xk, (_, m) in zip(xs_, sub_models):
            ta.Optimize(xk, m, opts)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3, 0.0

    arms = {"longest_first": lambda: arm_ragged(False), "keep_order": lambda: arm_ragged(True), "uniform": arm_uniform,
            "subset64_ragged": arm_sub_ragged, "subset64_per_count": arm_per_count}
    for f in arms.values():   # warm-up: builds, workspaces, caches
        f()
    lines, times = [], {k: [] for k in arms}
    for alt in range(a.alternations):
        for name, f in arms.items():
            t, passes = f()
            times[name].append(t)
            line = dict(probe="ragged_probe", arm=name, alternation=alt, P=P if not name.startswith("subset64") else 64, n=N, dtype="f32",
                        total_items=int(counts[sub].sum()) if name.startswith("subset64") else (total if name != "uniform" else P * MEAN), ms_per_solve=round(t * 1e3, 4))
            if passes:
                line["item_passes_per_s"] = passes / t
            if name == "subset64_per_count":
                line["uniform_calls"] = len(sub_models)
            lines.append(line)
            print(json.dumps(line), flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    summary = dict(probe="ragged_probe", arm="summary", alternations=a.alternations, P=P, count_range=[LO, HI], total_items=total,
                   uniform_items=P * MEAN, median_ms={k: round(v * 1e3, 4) for k, v in med.items()}, spread={k: round(v, 4) for k, v in spread.items()},
                   # per item streamed: the ragged batch holds total_items, the uniform one P x 2 000
                   ragged_over_uniform_per_item=(med["longest_first"] / total) / (med["uniform"] / (P * MEAN)),
                   keep_order_over_longest_first=med["keep_order"] / med["longest_first"],
                   per_count_over_ragged_subset64=med["subset64_per_count"] / med["subset64_ragged"],
                   stats_ragged=res.stats_ragged(), stats_uniform=res.stats())
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        for line in lines:
            fo.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
