"""A numpy restatement of gradient descent as the reference runs it: Optimizer_::OptimizeAcc / Step
(include/tinyopt/optimizers/optimizer.h:242-539) with SolverGD (include/tinyopt/solvers/gd.h), written from the reference, not
from the device code.  Arithmetic in the problem's dtype (fp32 or fp64) wherever the reference computes in `Scalar`; costs,
norms and relative decreases in double as the reference does.

`gd_optimize(x0, f, pod, lr, dtype)` runs a batch: f(p, x) -> (cost, grad) of problem p at x, both in `dtype`; pod is the
toa_options POD (tinyopt_amd._capi.ToaOptions), lr the float Options::gd.lr.  Returns the dict
tests/parity.py::check_trajectories expects.
"""
from __future__ import annotations

import numpy as np

DBL_MAX = np.finfo(np.float64).max
STOP_NAN_OR_INF, STOP_NONE, STOP_MIN_ERROR, STOP_MIN_REL_ERROR, STOP_MIN_DELTA_NORM, STOP_MIN_GRAD_NORM = -2, 0, 1, 2, 3, 4
STOP_MAX_ITERS, STOP_MAX_NO_DECR, STOP_MAX_CONSEC_NO_DECR, STOP_SOLVER_FAILED = 5, 6, 7, -3


def float_epsilon(T) -> float:   # math.h:297-301
    return float(np.float32(1e-4)) if T == np.float32 else float(np.float32(1e-7))


def normalize_cost(c: float, pod) -> float:   # base.h:41-45 on Cost(Scalar): num_residuals = 1
    if not pod.use_squared_norm:
        with np.errstate(invalid="ignore"):
            c = float(np.sqrt(c))
    if pod.downscale_by_2:
        c *= 0.5
    if pod.normalize:
        c /= 1
    return c


def gd_build_solve(x, f, pod, lr, T):
    """SolverGD::Build (clear, accumulate, Clamp) + Solve.  Returns (normalised cost, g, dx or None)."""
    c, g = f(x)
    g = np.asarray(g, T).copy()
    if pod.grad_clipping != 0:   # base.h:29-38
        m = T(pod.grad_clipping)
        g = np.minimum(np.maximum(g, -m), m)
    cost = normalize_cost(float(c), pod)
    if cost == DBL_MAX:          # Solve: !cost().isValid()
        return cost, g, None
    return cost, g, T(-np.float32(lr)) * g   # -options_.gd.lr * grad_ (a float promoted to Scalar)


def gd_solve_one(x0, f, pod, lr, T, hs):
    """OptimizeAcc for one problem.  Returns (x, stop, iters, fails, consec, final_cost, final_rerr, errs, deltas2, succ)."""
    T = np.dtype(T).type
    x = np.asarray(x0, T).copy()
    max_iters = pod.max_iters + 1 + (1 if pod.check_final_cost else 0)   # :248-250
    mcf, mtf = int(pod.max_consec_failures), int(pod.max_total_failures)
    max_tries = max(1, mcf) if mcf > 0 else 255
    tmax = float(np.finfo(T).max)
    st = dict(final_cost=DBL_MAX, final_rerr=DBL_MAX, stop=STOP_NONE, iters=0, fails=0, consec=0)
    errs, d2s, succ = np.zeros(hs), np.zeros(hs), np.zeros(hs, np.uint8)

    def step(it):   # :331-539 -> (good, dx or None)
        dx, g, cost, failed = None, None, None, True
        while st["consec"] <= max_tries:
            cost, g, dx = gd_build_solve(x, f, pod, lr, T)
            if dx is not None:
                failed = False
                break
            st["consec"] = (st["consec"] + 1) & 0xFF
            st["fails"] = (st["fails"] + 1) & 0xFF
            if np.isnan(cost) or np.isinf(cost):
                st["stop"] = STOP_NAN_OR_INF
                return False, None
            if mcf > 0 and st["consec"] >= mcf:
                if st["final_cost"] < tmax:
                    st["stop"] = STOP_MAX_CONSEC_NO_DECR
                break
        if failed:
            st["stop"] = STOP_SOLVER_FAILED
            return False, None
        err = cost
        if np.isnan(err) or np.isinf(err):
            st["stop"] = STOP_NAN_OR_INF
            return False, None
        with np.errstate(over="ignore", invalid="ignore"):
            dx_norm2 = float(np.sum(dx * dx, dtype=T))
            grad_norm2 = float(np.sum(g * g, dtype=T)) if pod.min_grad_norm2 > 0 else 0.0
        if np.isnan(dx_norm2) or np.isinf(dx_norm2):
            st["stop"] = STOP_NAN_OR_INF
            return False, None
        fc = st["final_cost"]
        derr = err - fc
        good = derr < 0.0
        rel = (fc - err) / fc if (fc > float_epsilon(T) and fc < tmax) else 0.0
        if st["iters"] < hs:
            errs[st["iters"]], d2s[st["iters"]], succ[st["iters"]] = err, dx_norm2, 1 if good else 0
        if good or it == 0:
            st["consec"] = 0
            st["final_cost"], st["final_rerr"] = err, rel
        else:
            st["fails"] = (st["fails"] + 1) & 0xFF
            st["consec"] = (st["consec"] + 1) & 0xFF
            if mcf > 0 and st["consec"] >= mcf:
                st["stop"] = STOP_MAX_CONSEC_NO_DECR
                return False, None
            if mtf > 0 and st["fails"] >= mtf:
                st["stop"] = STOP_MAX_NO_DECR
                return False, None
        if pod.min_error > 0 and err < pod.min_error:
            st["stop"] = STOP_MIN_ERROR
        elif pod.min_rerr_dec > 0 and 0.0 < rel < pod.min_rerr_dec:
            st["stop"] = STOP_MIN_REL_ERROR
        elif pod.min_step_norm2 > 0 and dx_norm2 < pod.min_step_norm2:
            st["stop"] = STOP_MIN_DELTA_NORM
        elif pod.min_grad_norm2 > 0 and grad_norm2 < pod.min_grad_norm2:
            st["stop"] = STOP_MIN_GRAD_NORM
        return good, dx

    last_dx = None
    with np.errstate(over="ignore", invalid="ignore"):
        for it in range(max_iters):   # :266-310
            good, dx = step(it)
            if good:
                x = x + dx
                last_dx = dx
            elif last_dx is not None:   # roll back
                x = x + (-last_dx)
                last_dx = None
            elif dx is not None:
                x = x + dx
                last_dx = dx
            st["iters"] += 1
            if st["stop"] != STOP_NONE:
                break
    if st["stop"] == STOP_NONE and st["iters"] >= max_iters:
        st["stop"] = STOP_MAX_ITERS
    return x, st, errs, d2s, succ


def gd_optimize(x0, f, pod, lr, dtype):
    """x0: [P, n]; f(p, x) -> (cost, grad) of problem p.  Returns the dict of tests/parity.py::check_trajectories
    (errs / succ / deltas2 [P, max_iters + 2], iters, stop, x, cost, fails, consec, rerr)."""
    T = np.dtype(dtype).type
    P, n = np.asarray(x0).shape
    hs = pod.max_iters + 2
    out = dict(errs=np.zeros((P, hs)), succ=np.zeros((P, hs), np.uint8), deltas2=np.zeros((P, hs)), iters=np.zeros(P, np.int64),
               stop=np.zeros(P, np.int64), x=np.zeros((P, n), T), cost=np.zeros(P), fails=np.zeros(P, np.int64),
               consec=np.zeros(P, np.int64), rerr=np.zeros(P))
    for p in range(P):
        x, st, errs, d2s, succ = gd_solve_one(x0[p], lambda xx, p=p: f(p, xx), pod, lr, T, hs)
        out["x"][p] = x
        out["errs"][p], out["deltas2"][p], out["succ"][p] = errs, d2s, succ
        out["iters"][p], out["stop"][p], out["fails"][p], out["consec"][p] = st["iters"], st["stop"], st["fails"], st["consec"]
        out["cost"][p], out["rerr"][p] = st["final_cost"], st["final_rerr"]
    return out


# ---- the cost functions of the tests, in the problem's dtype ------------------------------------------------------------
def quartic(x, T):
    """tests/unconstrained.cpp:19-42: 3 y^2 + y^4 - 2, y = x - 42, and its gradient (the same association as the device bodies)."""
    T = np.dtype(T).type
    y = T(x[0]) - T(42)
    c = (T(3) * y * y + y * y * y * y) - T(2)
    g = T(2) * T(3) * y + T(4) * (y * y * y)
    return c, np.array([g], T)


def logistic(A, yl, x, T):
    """sum_i log(1 + exp(-y_i a_i . x)) and its gradient; A [items, n], yl [items]."""
    T = np.dtype(T).type
    A = np.asarray(A, T)
    z = np.zeros(A.shape[0], T)
    for j in range(A.shape[1]):   # the bodies' own order: z += p[j] * x[j]
        z = z + A[:, j] * T(x[j])
    with np.errstate(over="ignore"):
        e = np.exp(-yl.astype(T) * z)
    c = np.sum(np.log(T(1) + e), dtype=T)
    s = -yl.astype(T) * e / (T(1) + e)
    return T(c), (A * s[:, None]).sum(axis=0, dtype=T)
