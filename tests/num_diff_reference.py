"""A numpy restatement of the reference's numerical differentiation and gradient checkers, written from the reference
(include/tinyopt/diff/num_diff.h:56-126 NumEval, :197-309 CreateNumDiffFunc1 / 2; include/tinyopt/diff/gradient_check.h), not
from the device code.  Arithmetic in the test dtype T wherever the reference computes in `Scalar`.

The checkers are the batched library's definition (include/tinyopt_amd.h toa_jit_check_gradient): a residual function with a
hand-written Jacobian J is compared through g = J^T r and H = J^T J against the same products of the numeric Jacobian, a scalar
cost with a hand-written gradient through g; step eps / 10, pass when every distance is < eps.
"""
from __future__ import annotations

import numpy as np

FORWARD, CENTRAL, FAST_CENTRAL = "forward", "central", "fast_central"   # diff::Method (num_diff.h:20-52)


def float_epsilon(T):   # math.h:297-301: static_cast<Scalar>(is_float ? 1e-4f : 1e-7f)
    T = np.dtype(T).type
    return T(np.float32(1e-4)) if T == np.float32 else T(np.float32(1e-7))


def default_eps(T) -> float:   # gradient_check.h:53
    return 1e-2 if np.dtype(T).type == np.float32 else 1e-5


def num_eval(f, x, method=CENTRAL, h=None, T=np.float64):
    """NumEval: f(x) -> residuals [R] (or a scalar) in T.  Returns (res, J [R, n])."""
    T = np.dtype(T).type
    x = np.asarray(x, T)
    h = float_epsilon(T) if h is None else T(h)
    res = np.atleast_1d(np.asarray(f(x), T))
    n = x.shape[0]
    J = np.zeros((res.shape[0], n), T)
    for r in range(n):
        y = x.copy()
        y[r] = T(y[r] + h)                                   # dx[r] = h; PlusEq(y, dx)
        res_plus = np.atleast_1d(np.asarray(f(y), T))
        if method == CENTRAL:
            y = x.copy()                                     # copy again
            y[r] = T(y[r] + (-h))
            res_minus = np.atleast_1d(np.asarray(f(y), T))
            J[:, r] = (res_plus - res_minus) / (T(2) * h)
        elif method == FAST_CENTRAL:
            y[r] = T(y[r] + T(-2) * h)                       # formed from y = x + h
            res_minus = np.atleast_1d(np.asarray(f(y), T))
            J[:, r] = (res_plus - res_minus) / (T(2) * h)
        elif method == FORWARD:
            J[:, r] = (res_plus - res) / h
        else:
            raise ValueError(method)
    return res, J


def estimate_num_jac(f, x, method=CENTRAL, h=None, T=np.float64):
    return num_eval(f, x, method, h, T)[1]


def num_diff_func(f, method=CENTRAL, h=None, T=np.float64):
    """CreateNumDiffFunc2 (CreateNumDiffFunc1 without H): x -> (res, g = J^T res, H = J^T J)."""
    def acc(x):
        res, J = num_eval(f, x, method, h, T)
        return res, J.T @ res, J.T @ J
    return acc


def check_residuals_gradient(f_with_jac, x, eps=None, method=CENTRAL, check_H=True, T=np.float64):
    """f_with_jac(x) -> (residuals [R], J [R, n]) — the hand-written derivatives; its residuals alone are differenced.
    Returns (ok, max |g - g_num|, max |H - H_num|)."""
    T = np.dtype(T).type
    eps = default_eps(T) if eps is None or eps <= 0 else float(eps)
    res, J = f_with_jac(np.asarray(x, T))
    res, J = np.atleast_1d(np.asarray(res, T)), np.atleast_2d(np.asarray(J, T))
    _, Jn = num_eval(lambda xx: f_with_jac(xx)[0], x, method, T(eps / 10.0), T)
    dg = float(np.abs(J.T @ res - Jn.T @ res).max())
    dH = float(np.abs(J.T @ J - Jn.T @ Jn).max()) if check_H else 0.0
    return (dg < eps) and (not check_H or dH < eps), dg, dH


def check_gradient(f_with_grad, x, eps=None, method=CENTRAL, T=np.float64):
    """f_with_grad(x) -> (cost, grad [n]).  Returns (ok, max |g - g_num|)."""
    T = np.dtype(T).type
    eps = default_eps(T) if eps is None or eps <= 0 else float(eps)
    _, g = f_with_grad(np.asarray(x, T))
    _, Jn = num_eval(lambda xx: f_with_grad(xx)[0], x, method, T(eps / 10.0), T)
    dg = float(np.abs(np.asarray(g, T) - Jn[0]).max())
    return dg < eps, dg
