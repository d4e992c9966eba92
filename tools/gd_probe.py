#!/usr/bin/env python3
"""Throughput of the first-order path (toa_jit_gd_run): batched logistic regression c_i = log(1 + exp(-y_i a_i . x)).

Every stop threshold is zeroed, so each problem runs max_iters + 1 Builds (one pass over its items each).  One JSON line
per case: iterations/s, ms per batched solve, and the HBM fraction — bytes streamed per pass P * items * (n + 1) * sizeof(T),
times the passes the kernel counted, over the kernel time (torch events), over 8 TB/s — plus the build's stats()
(registers, scratch, workgroups per CU).

usage: python tools/gd_probe.py [--P 16384] [--items 2000] [--iters 20] [--reps 5] [--cases default|quick]
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


def body(n, kind):
    if kind == "cost":
        return f"S z = S(0); for (int j = 0; j < {n}; ++j) z += p[j] * x[j]; c = log(S(1) + exp(-p[{n}] * z));"
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j]; const T yy = p[{n}]; const T e = exp(-yy * z);\n"
            f"c = log(T(1) + e);\n"
            f"if (want_grad) {{ const T s = -yy * e / (T(1) + e); for (int j = 0; j < {n}; ++j) G[j] += s * p[j]; }}")


def run_case(ta, P, n, items, dtype, kind, iters, reps):
    g = torch.Generator(device="cuda").manual_seed(1234 + n)
    A = torch.randn(P, items, n, device="cuda", dtype=dtype, generator=g) / n ** 0.5
    w = torch.randn(P, n, 1, device="cuda", dtype=dtype, generator=g)
    y = torch.where(torch.bmm(A, w).squeeze(2) + 0.5 * torch.randn(P, items, device="cuda", dtype=dtype, generator=g) > 0, 1.0, -1.0).to(dtype)
    data = torch.cat([A, y[:, :, None]], dim=2).contiguous()
    del A
    res = ta.JitResidual(body(n, kind), n=n, item_scalars=n + 1, dtype=dtype, kind=kind)
    model = res.bind(data)
    o = ta.Options()
    o.solver_type = ta.Options.GradientDescent
    o.max_iters = iters
    o.min_error = o.min_rerr_dec = o.min_step_norm2 = o.min_grad_norm2 = 0.0
    o.max_consec_failures = 0
    o.max_total_failures = 0
    o.gd.lr = 1.0 / items
    x0 = torch.zeros(P, n, device="cuda", dtype=dtype)
    x = x0.clone()
    out = ta.Optimize(x, model, o)          # warm-up (and the first launch of the code object)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        x.copy_(x0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ta.Optimize(x, model, o, out=out)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    t = sorted(times)[len(times) // 2]
    passes = int(out.counters[0].item())
    its = int(out.num_iters.sum().item())
    stops = torch.bincount(out.stop_reason.to(torch.int64) + 4, minlength=14).tolist()
    esz = data.element_size()
    bytes_streamed = passes * items * (n + 1) * esz
    line = dict(probe="gd_probe", form=kind, dtype="f32" if dtype == torch.float32 else "f64", P=P, n=n, items=items,
                max_iters=iters, passes=passes, iterations=its, ms_per_solve=round(t * 1e3, 4), iterations_per_s=its / t,
                passes_per_s=passes / t, GB_per_s=bytes_streamed / t / 1e9, hbm_fraction_of_8TBps=bytes_streamed / t / HBM_PEAK,
                all_max_iters=stops[5 + 4] == P, stats=res.stats(), reps_s=[round(v * 1e3, 4) for v in times])
    print(json.dumps(line), flush=True)
    res.close()
    del data, model, x, x0, out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=16384)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="default", choices=["default", "quick"])
    a = ap.parse_args()
    import tinyopt_amd as ta
    cases = [(12, torch.float32, "cost_grad"), (12, torch.float32, "cost")]
    if a.cases == "default":
        cases += [(50, torch.float32, "cost_grad"), (50, torch.float32, "cost"), (12, torch.float64, "cost_grad"), (12, torch.float64, "cost")]
    for n, dt, kind in cases:
        run_case(ta, a.P, n, a.items, dt, kind, a.iters, a.reps)


if __name__ == "__main__":
    main()
