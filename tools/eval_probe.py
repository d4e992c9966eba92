#!/usr/bin/env python3
"""Throughput of Eval (toa_jit_eval; csrc/eval_rows.hpp): the DenseRow residual a.x + 0.1 sin(a.x) - b with its own Jacobian and
as AD text at the C4 shape (12 500 x n = 50 x m = 2 000, fp32), and with its own Jacobian at 131 072 x n = 6 x m = 1 000 and at
32 768 x n = 32 x m = 1 000 (the width at which the row writes of the dense LDS image conflict worst).

One JSON line per case, timed by events over `--reps` warm calls: ms per call, the bytes read plus written per call (items + x in,
res + J out), the fraction of 8 TB/s — and two yardsticks on the same model, data and process: toa_jit_accumulate(want_grad = 1),
and a torch device-to-device copy_ of a buffer of (bytes read + bytes written) / 2 bytes, which moves the same traffic with no
arithmetic.

usage: python tools/eval_probe.py [--reps 20] [--scale 1.0]     (--scale shrinks P: a quick look)
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


def dense_row_body(n, kind):
    """a.x + 0.1 sin(a.x) - b as AD text, or with its own Jacobian row."""
    if kind == "residual":
        return f"S t = x[0] * p[0];\n#pragma unroll 2\nfor (int j = 1; j < {n}; ++j) t = t + x[j] * p[j];\nr[0] = t + T(0.1) * sin(t) - p[{n}];"
    return (f"T t = x[0] * p[0];\nfor (int j = 1; j < {n}; ++j) t += x[j] * p[j];\nr[0] = t + T(0.1) * sin(t) - p[{n}];\n"
            f"if (want_grad) {{ const T sc = T(1) + T(0.1) * cos(t); for (int j = 0; j < {n}; ++j) J[0][j] = sc * p[j]; }}")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def run_case(ta, P, n, items, kind, reps):
    dtype = torch.float32
    g = torch.Generator(device="cuda").manual_seed(77 + n)
    data = torch.rand(P, items, n + 1, device="cuda", dtype=dtype, generator=g) * 2 - 1
    x = torch.rand(P, n, device="cuda", dtype=dtype, generator=g) * 2 - 1
    res = ta.JitResidual(dense_row_body(n, kind), n=n, item_scalars=n + 1, dtype=dtype, kind=kind)
    model = res.bind(data)
    r = torch.empty(P, items, device="cuda", dtype=dtype)
    J = torch.empty(P, items, n, device="cuda", dtype=dtype)
    t_eval = timed(lambda: ta.Eval(model, x, res_out=r, J_out=J), reps)
    t_jac = timed(lambda: ta.CalculateJac(model, x, J_out=J), reps)
    t_res = timed(lambda: ta.Eval(model, x, jac=False, res_out=r), reps)
    ctx = ta.api.default_context()
    gg = torch.empty(P, n, device="cuda", dtype=dtype)
    H = torch.empty(P, n, n, device="cuda", dtype=dtype)
    c = torch.empty(P, device="cuda", dtype=torch.float64)
    t_acc = timed(lambda: ta.api.check(ctx.lib.toa_jit_accumulate(ctx.h, res._h, items, P, model.packed.data_ptr(), x.data_ptr(), 1, gg.data_ptr(),
                                                                  H.data_ptr(), c.data_ptr(), None)), reps)
    esz = data.element_size()
    b_in, b_out = (data.numel() + x.numel()) * esz, (r.numel() + J.numel()) * esz
    half = (b_in + b_out) // 2
    src = torch.empty(half, device="cuda", dtype=torch.uint8)
    dst = torch.empty(half, device="cuda", dtype=torch.uint8)
    t_copy = timed(lambda: dst.copy_(src), reps)
    line = dict(probe="eval_probe", form=kind, dtype="f32", P=P, n=n, items=items, reps=reps, ms_eval=round(t_eval * 1e3, 4),
                bytes_read=b_in, bytes_written=b_out, GB_per_s=(b_in + b_out) / t_eval / 1e9, hbm_fraction_of_8TBps=(b_in + b_out) / t_eval / HBM_PEAK,
                ms_calculate_jac=round(t_jac * 1e3, 4), ms_eval_residuals_only=round(t_res * 1e3, 4),
                ms_accumulate_want_grad=round(t_acc * 1e3, 4), ms_torch_copy_same_traffic=round(t_copy * 1e3, 4), copy_bytes=half,
                eval_over_copy=t_eval / t_copy)
    print(json.dumps(line), flush=True)
    res.close()
    del data, model, r, J, src, dst, H
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    import tinyopt_amd as ta
    for P, n, items, kind in ((12500, 50, 2000, "accumulate"), (12500, 50, 2000, "residual"), (131072, 6, 1000, "accumulate"),
                               (32768, 32, 1000, "accumulate")):   # n = 32: the dense image's worst width (32-way conflicts of the row writes)
        run_case(ta, max(1, int(P * a.scale)), n, items, kind, a.reps)


if __name__ == "__main__":
    main()
