#!/usr/bin/env python3
"""Batched logistic regression, second order beside first order: the kind="cost_hess" body under Levenberg-Marquardt (toa_jit_lm_run
over HessCostModel) and the kind="cost_grad" body under gradient descent (toa_jit_gd_run, tools/gd_probe.py), at
the shape of gd_probe — 16 384 problems x n = 12 x 2 000 items, fp32 and fp64 — alternated in one process after a warm-up of each.

Per precision and arm one JSON line: ms per pass (a pass = one read of a problem's items: a Build, or a cost-only evaluation) as the
median of the alternations with their spread, passes per problem until the solve stops (LM: Options() with min_grad_norm2 as the
stop that a converged Newton solve meets; GD: 21 passes, its max_iters + 1, nowhere near a minimum), the fraction of the 8 TB/s HBM
peak by the bytes streamed, the final cost per problem and stats().  Recorded, not gated.

usage: python tools/newton_probe.py [--P 16384] [--items 2000] [--alternations 5] [--out profiles/r17_newton_probe.jsonl]
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
N = 12
HESS_BODY = f"""
T z = 0; for (int j = 0; j < {N}; ++j) z += p[j] * x[j];
const T y = p[{N}], e = exp(-y * z), s = T(1) / (T(1) + e);        // sigma(y z)
c = log(T(1) + e);
if (want_grad) {{
  const T gz = -y * (T(1) - s), hz = s * (T(1) - s);
  for (int a = 0; a < {N}; ++a) {{ G[a] += gz * p[a]; for (int b = a; b < {N}; ++b) H(a, b) += hz * p[a] * p[b]; }}
}}
"""
GRAD_BODY = (f"T z = 0; for (int j = 0; j < {N}; ++j) z += p[j] * x[j]; const T yy = p[{N}]; const T e = exp(-yy * z);\n"
             "c = log(T(1) + e);\n"
             f"if (want_grad) {{ const T s = -yy * e / (T(1) + e); for (int j = 0; j < {N}; ++j) G[j] += s * p[j]; }}")


def timed(ta, x, x0, model, o, out):
    x.copy_(x0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ta.Optimize(x, model, o, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def run_dtype(ta, P, items, dtype, alternations, sink):
    g = torch.Generator(device="cuda").manual_seed(1234 + N)
    A = torch.randn(P, items, N, device="cuda", dtype=dtype, generator=g) / N ** 0.5
    w = torch.randn(P, N, 1, device="cuda", dtype=dtype, generator=g)
    y = torch.where(torch.bmm(A, w).squeeze(2) + 0.5 * torch.randn(P, items, device="cuda", dtype=dtype, generator=g) > 0, 1.0, -1.0).to(dtype)
    data = torch.cat([A, y[:, :, None]], dim=2).contiguous()
    del A
    arms = {}
    lm = ta.Options()                                   # Newton with Marquardt's damping: the reference's defaults
    gd = ta.Options()                                   # tools/gd_probe.py's run: 21 passes at lr = 1 / items
    gd.solver_type, gd.max_iters = ta.Options.GradientDescent, 20
    gd.min_error = gd.min_rerr_dec = gd.min_step_norm2 = gd.min_grad_norm2 = 0.0
    gd.max_consec_failures = gd.max_total_failures = 0
    gd.gd.lr = 1.0 / items
    for name, body, kind, o in (("cost_hess under LM", HESS_BODY, "cost_hess", lm), ("cost_grad under GD", GRAD_BODY, "cost_grad", gd)):
        res = ta.JitResidual(body, n=N, item_scalars=N + 1, dtype=dtype, kind=kind)
        arms[name] = dict(res=res, model=res.bind(data), o=o, times=[], out=None)
    x0 = torch.zeros(P, N, device="cuda", dtype=dtype)
    x = x0.clone()
    for arm in arms.values():                           # a warm-up of each
        _, arm["out"] = timed(ta, x, x0, arm["model"], arm["o"], None)
    for _ in range(alternations):                       # ... then alternated
        for arm in arms.values():
            t, arm["out"] = timed(ta, x, x0, arm["model"], arm["o"], arm["out"])
            arm["times"].append(t)
    esz = data.element_size()
    for name, arm in arms.items():
        out = arm["out"]
        passes = int(out.counters[0].item()) + int(out.counters[1].item())   # Builds + cost-only evaluations
        ts = sorted(arm["times"])
        t = ts[len(ts) // 2]
        bytes_streamed = passes * items * (N + 1) * esz
        stops = torch.bincount(out.stop_reason.to(torch.int64) + 4, minlength=14).tolist()
        line = dict(probe="newton_probe", arm=name, dtype="f32" if dtype == torch.float32 else "f64", P=P, n=N, items=items,
                    passes=passes, passes_per_problem=passes / P, iterations_per_problem=float(out.num_iters.sum().item()) / P,
                    ms_per_solve=round(t * 1e3, 4), ms_per_pass=round(t * 1e3 * P / passes, 6),
                    spread_ms_per_solve=[round(ts[0] * 1e3, 4), round(ts[-1] * 1e3, 4)],
                    GB_per_s=bytes_streamed / t / 1e9, hbm_fraction_of_8TBps=bytes_streamed / t / HBM_PEAK,
                    mean_final_cost=float(out.final_cost.mean().item()), stop_reasons={str(i - 4): c for i, c in enumerate(stops) if c},
                    stats=arm["res"].stats(), alternations_ms=[round(v * 1e3, 4) for v in arm["times"]])
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()
    for arm in arms.values():
        arm["res"].close()
    del data, arms, x, x0
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=16384)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import tinyopt_amd as ta
    sink = open(a.out, "w") if a.out else None
    for dt in (torch.float32, torch.float64):
        run_dtype(ta, a.P, a.items, dt, a.alternations, sink)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
