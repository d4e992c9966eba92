#!/usr/bin/env python3
"""Shared item tables (JitResidual(..., shared_scalars=n)) beside the replicated form they replace: batched logistic
regression as kind="cost_ggn" under Levenberg-Marquardt on ONE design matrix X [items, n] and per-problem labels,

  * replicated  item = (y, the row of X): item_scalars = n + 1, X copied into every problem's items — what a caller had to do before;
  * shared      item = (y), shared_scalars = n: X handed over once per call, staged beside the private items (expected to be served by the L2);

both arms in one process on the same numbers, alternated after a warm-up of each, at

  * 12 500 problems x n = 50 x 2 000 items, fp32 and fp64;
  * 16 384 problems x n = 12 x 2 000 items, fp32.

Per shape, precision and arm one JSON line: ms per solve as the median of the alternations with their min-max, passes per problem (a
pass = one read of a problem's items), ms per pass, the bytes the arm must fetch from HBM by its shapes (the table counted once per
solve: 400 KB are expected to stay in a 4 MiB L2; computed, not read from counters), the fraction of the 8 TB/s HBM peak by those bytes, the mean
final cost, the StopReasons and stats() (registers / scratch / workgroups per CU).  The yardstick of the shared arm is the replicated
arm of the same run.  Recorded, not gated.

usage: python tools/shared_probe.py [--items 2000] [--alternations 5] [--scale 1.0] [--out profiles/r20_shared_probe.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def body(n, table):
    """table: an accessor of the item's features — s[j] (shared) or p[1 + j] (replicated); the label is p[0] in both"""
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += {table('j')} * x[j];\n"
            "const T y = p[0], e = exp(-y * z), sg = T(1) / (T(1) + e);\n"
            "c = log(T(1) + e);\n"
            f"if (want_grad) {{ gs = -y * (T(1) - sg); hs = sg * (T(1) - sg); for (int a = 0; a < {n}; ++a) J[a] = {table('a')}; }}\n")


def timed(ta, x, x0, model, o, out):
    x.copy_(x0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ta.Optimize(x, model, o, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def run_shape(ta, P, n, items, dtype, alternations, sink):
    g = torch.Generator(device="cuda").manual_seed(4321 + n)
    X = (torch.randn(items, n, device="cuda", dtype=dtype, generator=g) / n ** 0.5).contiguous()
    w = torch.randn(P, n, device="cuda", dtype=dtype, generator=g)
    y = torch.where(w @ X.T + 0.5 * torch.randn(P, items, device="cuda", dtype=dtype, generator=g) > 0, 1.0, -1.0).to(dtype)
    del w
    esz = X.element_size()
    run = {}
    rep = ta.JitResidual(body(n, lambda j: f"p[1 + {j}]"), n=n, item_scalars=n + 1, dtype=dtype, kind="cost_ggn")
    data = torch.cat([y[:, :, None], X[None].expand(P, items, n)], dim=2).contiguous()
    run["replicated"] = dict(res=rep, model=rep.bind(data), bytes_per_pass=items * (n + 1) * esz, table_bytes=0)
    del data
    sh = ta.JitResidual(body(n, lambda j: f"s[{j}]"), n=n, item_scalars=1, shared_scalars=n, dtype=dtype, kind="cost_ggn")
    run["shared"] = dict(res=sh, model=sh.bind(y[:, :, None].contiguous(), shared=X), bytes_per_pass=items * esz, table_bytes=items * n * esz)
    o = ta.Options()
    x0 = torch.zeros(P, n, device="cuda", dtype=dtype)
    x = x0.clone()
    for arm in run.values():                            # a warm-up of each
        arm["times"] = []
        _, arm["out"] = timed(ta, x, x0, arm["model"], o, None)
        arm["x"] = x.clone()
    for _ in range(alternations):                       # ... then alternated
        for arm in run.values():
            t, arm["out"] = timed(ta, x, x0, arm["model"], o, arm["out"])
            arm["times"].append(t)
    dx = float((run["shared"]["x"] - run["replicated"]["x"]).abs().max().item())
    for name, arm in run.items():
        out = arm["out"]
        passes = int(out.counters[0].item()) + int(out.counters[1].item())   # Builds + cost-only evaluations
        ts = sorted(arm["times"])
        t = ts[len(ts) // 2]
        hbm_bytes = passes * arm["bytes_per_pass"] + arm["table_bytes"]
        stops = torch.bincount(out.stop_reason.to(torch.int64) + 4, minlength=14).tolist()
        line = dict(probe="shared_probe", arm=name, dtype="f32" if dtype == torch.float32 else "f64", P=P, n=n, items=items,
                    passes=passes, passes_per_problem=passes / P, iterations_per_problem=float(out.num_iters.sum().item()) / P,
                    ms_per_solve=round(t * 1e3, 4), ms_per_pass=round(t * 1e3 * P / max(passes, 1), 6),
                    spread_ms_per_solve=[round(ts[0] * 1e3, 4), round(ts[-1] * 1e3, 4)],
                    resident_bytes=int(P * arm["bytes_per_pass"] + arm["table_bytes"]), hbm_bytes_per_solve=int(hbm_bytes),
                    GB_per_s=hbm_bytes / t / 1e9, hbm_fraction_of_8TBps=hbm_bytes / t / HBM_PEAK,
                    mean_final_cost=float(out.final_cost.mean().item()), stop_reasons={str(i - 4): c for i, c in enumerate(stops) if c},
                    max_abs_x_difference_between_the_arms=dx, stats=arm["res"].stats(), alternations_ms=[round(v * 1e3, 4) for v in arm["times"]])
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()
    for arm in run.values():
        arm["res"].close()
    del run, x, x0, X, y
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the problem counts (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_shared_probe.jsonl"), help='"" = print only')
    a = ap.parse_args()
    import tinyopt_amd as ta
    sink = open(a.out, "w") if a.out else None
    for P, n, dt in ((12500, 50, torch.float32), (12500, 50, torch.float64), (16384, 12, torch.float32)):
        run_shape(ta, max(1, int(P * a.scale)), n, a.items, dt, a.alternations, sink)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
