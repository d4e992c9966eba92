#!/usr/bin/env python3
"""L-BFGS beside gradient descent on the same scalar cost model (toa_jit_lbfgs_run / toa_jit_gd_run): batched logistic regression
c_i = log(1 + exp(-y_i a_i . x)), the workload of tools/gd_probe.py, as a cost_grad body.

Arm (a), "pass": every stop threshold zeroed, so both solvers run max_iters + 1 passes per problem; ms per pass of the batch of the
L-BFGS kernel against the GD kernel, alternated in one process after a warm-up of each, medians of `reps` alternations.  The ratio
says what the per-wave state machine (the two-loop recursion, the line search) costs beside a pass over the items.
Arm (b), "solve": default thresholds (fp32: the defaults too), until each solver stops: passes per problem, ms per batched solve,
mean final cost, stop reasons.  GD runs at lr = 1 / items as in tools/gd_probe.py.

One JSON line per case and arm.  usage: python tools/lbfgs_probe.py [--P 16384] [--items 2000] [--iters 20] [--reps 5] [--cases default|quick]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.gd_probe import HBM_PEAK, body  # noqa: E402


def _options(ta, solver, items, iters=None):
    o = ta.Options()
    o.solver_type = solver
    o.hessian.save_last = False
    o.gd.lr = 1.0 / items
    if iters is not None:   # arm (a): nothing stops a problem but the iteration count
        o.max_iters = iters
        o.min_error = o.min_rerr_dec = o.min_step_norm2 = o.min_grad_norm2 = 0.0
        o.max_consec_failures = 0
        o.max_total_failures = 0
    return o


def _timed(ta, x, x0, model, o, out):
    x.copy_(x0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ta.Optimize(x, model, o, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def run_case(ta, P, n, items, dtype, iters, reps):
    g = torch.Generator(device="cuda").manual_seed(1234 + n)
    A = torch.randn(P, items, n, device="cuda", dtype=dtype, generator=g) / n ** 0.5
    w = torch.randn(P, n, 1, device="cuda", dtype=dtype, generator=g)
    y = torch.where(torch.bmm(A, w).squeeze(2) + 0.5 * torch.randn(P, items, device="cuda", dtype=dtype, generator=g) > 0, 1.0, -1.0).to(dtype)
    data = torch.cat([A, y[:, :, None]], dim=2).contiguous()
    del A
    res = ta.JitResidual(body(n, "cost_grad"), n=n, item_scalars=n + 1, dtype=dtype, kind="cost_grad")
    model = res.bind(data)
    x0 = torch.zeros(P, n, device="cuda", dtype=dtype)
    x = x0.clone()
    solvers = {"lbfgs": ta.Options.LBFGS, "gd": ta.Options.GradientDescent}
    common = dict(probe="lbfgs_probe", dtype="f32" if dtype == torch.float32 else "f64", P=P, n=n, items=items)
    stats = {"lbfgs": res.stats_lbfgs(), "gd": res.stats()}
    esz = data.element_size()
    for arm, it in (("pass", iters), ("solve", None)):
        opts = {k: _options(ta, s, items, it) for k, s in solvers.items()}
        outs, times = {}, {k: [] for k in solvers}
        for k in solvers:                      # warm-up of each (and the first launch of its code object)
            _, outs[k] = _timed(ta, x, x0, model, opts[k], None)
        for _ in range(reps):                  # alternated
            for k in solvers:
                t, outs[k] = _timed(ta, x, x0, model, opts[k], outs[k])
                times[k].append(t)
        lines = {}
        for k in solvers:
            t = sorted(times[k])[len(times[k]) // 2]
            passes = int(outs[k].counters[0].item())
            stops = torch.bincount(outs[k].stop_reason.to(torch.int64) + 4, minlength=14).tolist()
            lines[k] = dict(common, arm=arm, solver=k, max_iters=opts[k].max_iters, passes=passes, passes_per_problem=passes / P,
                            ms_per_solve=round(t * 1e3, 4), ms_per_pass_of_the_batch=t * 1e3 / (passes / P),
                            hbm_fraction_of_8TBps=passes * items * (n + 1) * esz / t / HBM_PEAK,
                            mean_final_cost=float(outs[k].final_cost.mean().item()),
                            stop_reasons={str(i - 4): c for i, c in enumerate(stops) if c}, stats=stats[k],
                            reps_ms=[round(v * 1e3, 4) for v in times[k]])
        lines["lbfgs"]["ms_per_pass_ratio_to_gd"] = lines["lbfgs"]["ms_per_pass_of_the_batch"] / lines["gd"]["ms_per_pass_of_the_batch"]
        for k in solvers:
            print(json.dumps(lines[k]), flush=True)
    res.close()
    del data, model, x, x0, outs
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
    cases = [(12, torch.float32)]
    if a.cases == "default":
        cases += [(12, torch.float64), (50, torch.float32), (50, torch.float64)]
    for n, dt in cases:
        run_case(ta, a.P, n, a.items, dt, a.iters, a.reps)


if __name__ == "__main__":
    main()
