#!/usr/bin/env python3
"""Batched logistic regression as a rank-one second-order cost: the kind="cost_ggn" body under Levenberg-Marquardt (toa_jit_lm_run over
RowModel<GgnRowFunctor>) beside the solvers a scalar cost had before it, alternated in one process after a warm-up
of each arm:

  * 12 500 problems x n = 50 x 2 000 items, fp32 and fp64, beside kind="cost_grad" under L-BFGS (Options.LBFGS) on the same data;
  * 16 384 problems x n = 12 x 2 000 items, fp32 and fp64, beside kind="cost_hess" under LM.

Per shape, precision and arm one JSON line: ms per solve as the median of the alternations with their spread, passes per problem (a
pass = one read of a problem's items: a Build, or a cost-only evaluation), ms per pass, the fraction of the 8 TB/s HBM peak by the
bytes streamed, the mean final cost, the StopReasons and stats() (registers / scratch / workgroups per CU).  Recorded, not gated.

usage: python tools/ggn_probe.py [--items 2000] [--alternations 5] [--scale 1.0] [--out profiles/r19_ggn_probe.jsonl]
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


def ggn_body(n):
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j];\n"
            f"const T y = p[{n}], e = exp(-y * z), s = T(1) / (T(1) + e);\n"
            "c = log(T(1) + e);\n"
            f"if (want_grad) {{ gs = -y * (T(1) - s); hs = s * (T(1) - s); for (int a = 0; a < {n}; ++a) J[a] = p[a]; }}\n")


def hess_body(n):
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j];\n"
            f"const T y = p[{n}], e = exp(-y * z), s = T(1) / (T(1) + e);\n"
            "c = log(T(1) + e);\n"
            "if (want_grad) {\n  const T gz = -y * (T(1) - s), hz = s * (T(1) - s);\n"
            f"  for (int a = 0; a < {n}; ++a) {{ G[a] += gz * p[a]; for (int b = a; b < {n}; ++b) H(a, b) += hz * p[a] * p[b]; }}\n}}\n")


def grad_body(n):
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j]; const T yy = p[{n}]; const T e = exp(-yy * z);\n"
            "c = log(T(1) + e);\n"
            f"if (want_grad) {{ const T s = -yy * e / (T(1) + e); for (int j = 0; j < {n}; ++j) G[j] += s * p[j]; }}")


def timed(ta, x, x0, model, o, out):
    x.copy_(x0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ta.Optimize(x, model, o, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def run_shape(ta, P, n, items, dtype, other, alternations, sink):
    g = torch.Generator(device="cuda").manual_seed(1234 + n)
    A = torch.randn(P, items, n, device="cuda", dtype=dtype, generator=g) / n ** 0.5
    w = torch.randn(P, n, 1, device="cuda", dtype=dtype, generator=g)
    y = torch.where(torch.bmm(A, w).squeeze(2) + 0.5 * torch.randn(P, items, device="cuda", dtype=dtype, generator=g) > 0, 1.0, -1.0).to(dtype)
    data = torch.cat([A, y[:, :, None]], dim=2).contiguous()
    del A
    lm = ta.Options()
    arms = {"cost_ggn under LM": (ggn_body(n), "cost_ggn", lm)}
    if other == "lbfgs":
        lb = ta.Options()
        lb.solver_type = ta.Options.LBFGS
        arms["cost_grad under L-BFGS"] = (grad_body(n), "cost_grad", lb)
    else:
        arms["cost_hess under LM"] = (hess_body(n), "cost_hess", ta.Options())
    run = {}
    for name, (body, kind, o) in arms.items():
        res = ta.JitResidual(body, n=n, item_scalars=n + 1, dtype=dtype, kind=kind)
        run[name] = dict(res=res, model=res.bind(data), o=o, times=[], out=None)
    x0 = torch.zeros(P, n, device="cuda", dtype=dtype)
    x = x0.clone()
    for arm in run.values():                            # a warm-up of each
        _, arm["out"] = timed(ta, x, x0, arm["model"], arm["o"], None)
    for _ in range(alternations):                       # ... then alternated
        for arm in run.values():
            t, arm["out"] = timed(ta, x, x0, arm["model"], arm["o"], arm["out"])
            arm["times"].append(t)
    esz = data.element_size()
    for name, arm in run.items():
        out = arm["out"]
        passes = int(out.counters[0].item()) + int(out.counters[1].item())   # Builds + cost-only evaluations
        ts = sorted(arm["times"])
        t = ts[len(ts) // 2]
        bytes_streamed = passes * items * (n + 1) * esz
        stops = torch.bincount(out.stop_reason.to(torch.int64) + 4, minlength=14).tolist()
        lbfgs = name.endswith("L-BFGS")
        line = dict(probe="ggn_probe", arm=name, dtype="f32" if dtype == torch.float32 else "f64", P=P, n=n, items=items,
                    passes=passes, passes_per_problem=passes / P, iterations_per_problem=float(out.num_iters.sum().item()) / P,
                    ms_per_solve=round(t * 1e3, 4), ms_per_pass=round(t * 1e3 * P / max(passes, 1), 6),
                    spread_ms_per_solve=[round(ts[0] * 1e3, 4), round(ts[-1] * 1e3, 4)],
                    GB_per_s=bytes_streamed / t / 1e9, hbm_fraction_of_8TBps=bytes_streamed / t / HBM_PEAK,
                    mean_final_cost=float(out.final_cost.mean().item()), stop_reasons={str(i - 4): c for i, c in enumerate(stops) if c},
                    stats=arm["res"].stats_lbfgs() if lbfgs else arm["res"].stats(), alternations_ms=[round(v * 1e3, 4) for v in arm["times"]])
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()
    for arm in run.values():
        arm["res"].close()
    del data, run, x, x0
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scales both problem counts (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_ggn_probe.jsonl"), help='"" = print only')
    a = ap.parse_args()
    import tinyopt_amd as ta
    sink = open(a.out, "w") if a.out else None
    for P, n, other in ((12500, 50, "lbfgs"), (16384, 12, "hess")):
        for dt in (torch.float32, torch.float64):
            run_shape(ta, max(1, int(P * a.scale)), n, a.items, dt, other, a.alternations, sink)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
