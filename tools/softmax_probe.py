#!/usr/bin/env python3
"""Batched softmax regression as a multi-output second-order cost: the kind="cost_ggn_multi" body under Levenberg-Marquardt
(toa_jit_lm_run over RowModel<GgnMultiRowFunctor>) beside the doors the same cost had before it, alternated in one
process after a warm-up of each arm, fp32 and fp64:

  * 3 classes with a reference class (K = 2, d = 25, n = 50), 12 500 problems x 2 000 items on ONE design matrix: the kind under LM;
    the same cost as kind="cost_grad" under L-BFGS; the kind with a diagonal ridge (with_prior); the kind with the design matrix as a
    shared table (bind(..., shared=)) beside the replicated form;
  * K = 2, d = 6, n = 12, 16 384 problems: the kind beside the same cost as a kind="cost_hess" body under LM;
  * K = 1 (logistic regression, n = 50, 12 500 problems): the kind beside kind="cost_ggn" on the same numbers.

Per arm one JSON line: ms per solve as the median of the alternations with their spread, passes per problem (a pass = one read of a
problem's items: a Build, or a cost-only evaluation), ms per pass, the fraction of the 8 TB/s HBM peak by the shapes (the bytes of the
problem's own items per pass; the shared table is not counted), the mean final cost, the StopReasons and stats() (registers / scratch /
workgroups per CU).  Recorded, not gated.

usage: python tools/softmax_probe.py [--items 2000] [--alternations 5] [--scale 1.0] [--out profiles/r21_softmax_probe.jsonl]
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


def _head(K, d, feat, label):
    """u, the stable log-sum-exp and the label's logit: shared by the three bodies; feat: where the features are read from"""
    return "\n".join([
        f"T u[{K}];",
        f"for (int k = 0; k < {K}; ++k) {{ u[k] = T(0); for (int j = 0; j < {d}; ++j) u[k] += {feat}[j] * x[k * {d} + j]; }}",
        f"T mx = T(0); for (int k = 0; k < {K}; ++k) mx = fmax(mx, u[k]);",
        f"T e[{K}]; T z = exp(-mx); for (int k = 0; k < {K}; ++k) {{ e[k] = exp(u[k] - mx); z += e[k]; }}",
        f"const T y = {label}; T uy = T(0); for (int k = 0; k < {K}; ++k) uy = (y == T(k + 1)) ? u[k] : uy;",
        "c = log(z) + mx - uy;"])


def multi_body(K, d, shared=False):
    feat, label, n = ("s", "p[0]", K * d) if shared else ("p", f"p[{d}]", K * d)
    return "\n".join([
        _head(K, d, feat, label),
        "if (want_grad) {",
        f"  T q[{K}]; for (int k = 0; k < {K}; ++k) q[k] = e[k] / z;",
        f"  for (int k = 0; k < {K}; ++k) {{ gs[k] = q[k] - ((y == T(k + 1)) ? T(1) : T(0));",
        "    for (int l = 0; l <= k; ++l) Hs[k][l] = (k == l) ? q[k] * (T(1) - q[k]) : -q[k] * q[l]; }",
        f"  for (int k = 0; k < {K}; ++k) {{ for (int a = 0; a < {n}; ++a) J[k][a] = T(0); for (int j = 0; j < {d}; ++j) J[k][k * {d} + j] = {feat}[j]; }}",
        "}"]) + "\n"


def grad_body(K, d):
    return "\n".join([
        _head(K, d, "p", f"p[{d}]"),
        "if (want_grad) {",
        f"  for (int k = 0; k < {K}; ++k) {{ const T gk = e[k] / z - ((y == T(k + 1)) ? T(1) : T(0)); for (int j = 0; j < {d}; ++j) G[k * {d} + j] += gk * p[j]; }}",
        "}"]) + "\n"


def hess_body(K, d):
    return "\n".join([
        _head(K, d, "p", f"p[{d}]"),
        "if (want_grad) {",
        f"  T q[{K}]; for (int k = 0; k < {K}; ++k) q[k] = e[k] / z;",
        f"  for (int k = 0; k < {K}; ++k) {{ const T gk = q[k] - ((y == T(k + 1)) ? T(1) : T(0));",
        f"    for (int i = 0; i < {d}; ++i) {{ G[k * {d} + i] += gk * p[i];",
        f"      for (int l = k; l < {K}; ++l) {{ const T w = (k == l) ? q[k] * (T(1) - q[k]) : -q[k] * q[l];",
        f"        for (int j = 0; j < {d}; ++j) if (l > k || j >= i) H(k * {d} + i, l * {d} + j) += w * p[i] * p[j]; }} }} }}",
        "}"]) + "\n"


def logistic_body(n, multi):
    gs, hs, J = ("gs[0]", "Hs[0][0]", "J[0][a]") if multi else ("gs", "hs", "J[a]")
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j];\n"
            f"const T y = p[{n}], e = exp(-y * z), s = T(1) / (T(1) + e);\n"
            "c = log(T(1) + e);\n"
            f"if (want_grad) {{ {gs} = -y * (T(1) - s); {hs} = s * (T(1) - s); for (int a = 0; a < {n}; ++a) {J} = p[a]; }}\n")


def timed(ta, x, x0, model, o, out):
    x.copy_(x0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ta.Optimize(x, model, o, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def alternate(ta, shape, arms, P, n, items, dtype, alternations, sink):
    """arms: name -> (res, model, options, bytes of a problem's own items per pass)"""
    run = {name: dict(res=r, model=m, o=o, bytes=b, times=[], out=None) for name, (r, m, o, b) in arms.items()}
    x0 = torch.zeros(P, n, device="cuda", dtype=dtype)
    x = x0.clone()
    for arm in run.values():                            # a warm-up of each
        _, arm["out"] = timed(ta, x, x0, arm["model"], arm["o"], None)
    for _ in range(alternations):                       # ... then alternated
        for arm in run.values():
            t, arm["out"] = timed(ta, x, x0, arm["model"], arm["o"], arm["out"])
            arm["times"].append(t)
    for name, arm in run.items():
        out = arm["out"]
        passes = int(out.counters[0].item()) + int(out.counters[1].item())   # Builds + cost-only evaluations
        ts = sorted(arm["times"])
        t = ts[len(ts) // 2]
        streamed = passes * arm["bytes"]
        stops = torch.bincount(out.stop_reason.to(torch.int64) + 4, minlength=14).tolist()
        lbfgs = name.endswith("L-BFGS")
        st = arm["res"].stats_lbfgs() if lbfgs else (arm["res"].stats_prior() if "ridge" in name else arm["res"].stats())
        line = dict(probe="softmax_probe", shape=shape, arm=name, dtype="f32" if dtype == torch.float32 else "f64", P=P, n=n, items=items,
                    passes=passes, passes_per_problem=passes / P, iterations_per_problem=float(out.num_iters.sum().item()) / P,
                    ms_per_solve=round(t * 1e3, 4), ms_per_pass=round(t * 1e3 * P / max(passes, 1), 6),
                    spread_ms_per_solve=[round(ts[0] * 1e3, 4), round(ts[-1] * 1e3, 4)],
                    GB_per_s=streamed / t / 1e9, hbm_fraction_of_8TBps=streamed / t / HBM_PEAK,
                    mean_final_cost=float(out.final_cost.mean().item()), stop_reasons={str(i - 4): c for i, c in enumerate(stops) if c},
                    stats=st, alternations_ms=[round(v * 1e3, 4) for v in arm["times"]])
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()
    for arm in run.values():
        arm["res"].close()


def softmax_data(P, K, d, items, dtype, seed):
    """ONE design matrix X [items, d] for the batch; per problem a weight matrix and classes drawn from its softmax (noisy labels)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(items, d, device="cuda", dtype=dtype, generator=g) / d ** 0.5
    W = 2.0 * torch.randn(P, d, K, device="cuda", dtype=dtype, generator=g)
    u = torch.cat([torch.zeros(P, items, 1, device="cuda", dtype=dtype), torch.matmul(X, W)], dim=2)
    gum = -torch.log(-torch.log(torch.rand(P, items, K + 1, device="cuda", dtype=dtype, generator=g).clamp_min(1e-12)))
    y = (u + gum).argmax(dim=2).to(dtype)               # (the Gumbel trick: a draw from the softmax of u)
    return X, y


def run_softmax(ta, shape, P, K, d, items, dtype, wide, alternations, sink):
    n, esz = K * d, torch.empty(0, dtype=dtype).element_size()
    X, y = softmax_data(P, K, d, items, dtype, 4321 + n)
    data = torch.cat([X.expand(P, items, d), y[:, :, None]], dim=2).contiguous()
    own = items * (d + 1) * esz
    multi = lambda: ta.JitResidual(multi_body(K, d), n=n, item_scalars=d + 1, residuals_per_item=K, dtype=dtype, kind="cost_ggn_multi")   # noqa: E731
    r = multi()
    arms = {"cost_ggn_multi under LM": (r, r.bind(data), ta.Options(), own)}
    if wide:
        lb = ta.Options()
        lb.solver_type = ta.Options.LBFGS
        rg = ta.JitResidual(grad_body(K, d), n=n, item_scalars=d + 1, dtype=dtype, kind="cost_grad")
        arms["cost_grad under L-BFGS"] = (rg, rg.bind(data), lb, own)
        rr = multi()
        lam = torch.full((P, n), 0.3, device="cuda", dtype=dtype)
        arms["cost_ggn_multi + diagonal ridge under LM"] = (rr, rr.bind(data).with_prior(torch.zeros(P, n, device="cuda", dtype=dtype), lam), ta.Options(), own)
        rs = ta.JitResidual(multi_body(K, d, shared=True), n=n, item_scalars=1, residuals_per_item=K, dtype=dtype, kind="cost_ggn_multi", shared_scalars=d)
        arms["cost_ggn_multi, shared design matrix, under LM"] = (rs, rs.bind(y[:, :, None].contiguous(), shared=X.contiguous()), ta.Options(), items * esz)
    else:
        rh = ta.JitResidual(hess_body(K, d), n=n, item_scalars=d + 1, dtype=dtype, kind="cost_hess")
        arms["cost_hess under LM"] = (rh, rh.bind(data), ta.Options(), own)
    alternate(ta, shape, arms, P, n, items, dtype, alternations, sink)
    del data, arms, X, y
    torch.cuda.empty_cache()


def run_logistic(ta, shape, P, n, items, dtype, alternations, sink):
    g = torch.Generator(device="cuda").manual_seed(1234 + n)
    A = torch.randn(P, items, n, device="cuda", dtype=dtype, generator=g) / n ** 0.5
    w = torch.randn(P, n, 1, device="cuda", dtype=dtype, generator=g)
    y = torch.where(torch.bmm(A, w).squeeze(2) + 0.5 * torch.randn(P, items, device="cuda", dtype=dtype, generator=g) > 0, 1.0, -1.0).to(dtype)
    data = torch.cat([A, y[:, :, None]], dim=2).contiguous()
    del A
    own = items * (n + 1) * data.element_size()
    r6 = ta.JitResidual(logistic_body(n, True), n=n, item_scalars=n + 1, residuals_per_item=1, dtype=dtype, kind="cost_ggn_multi")
    r5 = ta.JitResidual(logistic_body(n, False), n=n, item_scalars=n + 1, dtype=dtype, kind="cost_ggn")
    arms = {"cost_ggn_multi, K = 1, under LM": (r6, r6.bind(data), ta.Options(), own), "cost_ggn under LM": (r5, r5.bind(data), ta.Options(), own)}
    alternate(ta, shape, arms, P, n, items, dtype, alternations, sink)
    del data, arms
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the problem counts (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_softmax_probe.jsonl"), help='"" = print only')
    a = ap.parse_args()
    import tinyopt_amd as ta
    sink = open(a.out, "w") if a.out else None
    sc = lambda P: max(1, int(P * a.scale))   # noqa: E731
    for dt in (torch.float32, torch.float64):
        run_softmax(ta, "softmax K=2 d=25 n=50", sc(12500), 2, 25, a.items, dt, True, a.alternations, sink)
        run_softmax(ta, "softmax K=2 d=6 n=12", sc(16384), 2, 6, a.items, dt, False, a.alternations, sink)
        run_logistic(ta, "logistic K=1 n=50", sc(12500), 50, a.items, dt, a.alternations, sink)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
