"""CPU pins of the gradient-descent restatement (tests/gd_reference.py) against the reference's own expectations for
gd::Optimizer (tests/unconstrained.cpp, tests/solvers.cpp) and a hand-derived roll-back trajectory.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gd_reference as gr  # noqa: E402


def _pod(**kw):
    from tinyopt_amd._capi import ToaOptions
    from tinyopt_amd.api import Options
    o = Options()
    o.solver_type = Options.GradientDescent
    for k, v in kw.items():
        setattr(o, k, v)
    return o.to_pod()


def test_quartic_converges_like_unconstrained_cpp():
    """tests/unconstrained.cpp:19-42: x0 = 40.1, lr = 0.01, 1000 iterations, min_error = min_rerr_dec = 0 ->
    Succeeded, Converged, x = 42 +- 1e-5."""
    pod = _pod(max_iters=1000, min_error=0.0, min_rerr_dec=0.0)
    out = gr.gd_optimize(np.array([[40.1]]), lambda p, x: gr.quartic(x, np.float64), pod, 0.01, np.float64)
    stop = int(out["stop"][0])
    assert stop >= 0                       # Succeeded (output.h:30)
    assert 1 <= stop < 5                   # Converged (output.h:33-35)
    assert abs(out["x"][0, 0] - 42.0) < 1e-5
    assert out["cost"][0] == pytest.approx(-2.0, abs=1e-9)   # costs go negative: the minimum is -2


def test_one_build_and_solve_like_solvers_cpp():
    """tests/solvers.cpp:47-70: r = x - y at x = 0, lr = 0.1, one Build + Solve -> dx = lr * y +- 1e-2."""
    y = np.array([4.0, 5.0])
    pod = _pod()

    def f(x):   # the cost 0.5 |x - y|^2: g = J^T r = x - y
        r = x - y
        return 0.5 * float(r @ r), r

    cost, g, dx = gr.gd_build_solve(np.zeros(2), f, pod, 0.1, np.float64)
    assert dx is not None
    assert np.allclose(dx, 0.1 * y, atol=1e-2)
    assert np.allclose(g, -y)


def test_too_large_lr_rolls_back_and_stops_on_consecutive_failures():
    """c = x^2, lr = 1.5, x0 = 1: every step lands on -2x (cost 4x^2).  By hand (optimizer.h:266-310, 428-460):
    it 0  x = 1   err 1  accepted (first iteration)   -> x = -2
    it 1  x = -2  err 4  rejected (consec 1)          -> roll back to 1
    it 2  x = 1   err 1  rejected (no decrease, 2)    -> no last step: x + dx = -2
    it 3  x = -2  err 4  rejected (3)                 -> roll back to 1
    it 4  x = 1   err 1  rejected (4)                 -> x = -2
    it 5  x = -2  err 4  rejected (5 = max_consec_failures): kMaxConsecNoDecr -> roll back to 1"""
    pod = _pod()

    def f(p, x):
        return x[0] * x[0], np.array([2 * x[0]])

    for dt in (np.float64, np.float32):
        out = gr.gd_optimize(np.array([[1.0]], dt), f, pod, 1.5, dt)
        assert int(out["stop"][0]) == gr.STOP_MAX_CONSEC_NO_DECR
        assert int(out["iters"][0]) == 6
        assert out["x"][0, 0] == 1.0
        assert list(out["errs"][0, :6]) == [1, 4, 1, 4, 1, 4]
        assert list(out["succ"][0, :6]) == [1, 0, 0, 0, 0, 0]
        assert list(out["deltas2"][0, :6]) == [9, 36, 9, 36, 9, 36]
        assert int(out["fails"][0]) == 5 and out["cost"][0] == 1.0


def test_max_total_failures_and_nan():
    """kMaxNoDecr after max_total_failures rejected steps; a cost that turns NaN ends in kSystemHasNaNOrInf, x rolled back."""
    pod = _pod(max_total_failures=2)
    out = gr.gd_optimize(np.array([[1.0]]), lambda p, x: (x[0] * x[0], np.array([2 * x[0]])), pod, 1.5, np.float64)
    assert int(out["stop"][0]) == gr.STOP_MAX_NO_DECR and int(out["iters"][0]) == 3

    def f(p, x):   # sqrt(x): lr = 4 jumps from 1 to -1
        with np.errstate(invalid="ignore"):
            return np.sqrt(x[0]), np.array([0.5 / np.sqrt(x[0])])

    out = gr.gd_optimize(np.array([[1.0]]), f, _pod(), 4.0, np.float64)
    assert int(out["stop"][0]) == gr.STOP_NAN_OR_INF and int(out["iters"][0]) == 2 and out["x"][0, 0] == 1.0


def test_gd_options_defaults_agree(built):
    """options.h:147-154: Options::GD::lr = 1e-3f, in the C-ABI default and the Python mirror."""
    from tinyopt_amd import _capi
    from tinyopt_amd.api import Options
    lib = _capi.load()
    g = _capi.ToaGdOptions()
    g.lr = 5.0
    lib.toa_gd_options_default(C.byref(g))
    assert g.lr == pytest.approx(1e-3) and np.float32(g.lr) == np.float32(Options().gd.lr)
    assert list(g.reserved) == [0] * 7
    assert Options.GradientDescent == 2 and _capi.ABI_VERSION == lib.toa_abi_version() == 7
