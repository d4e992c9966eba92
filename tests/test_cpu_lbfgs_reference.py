"""CPU pins of the L-BFGS restatement (tests/lbfgs_reference.py; the state machine of DESIGN section 19): hand-derived trajectories
that are exact in binary, known minimisers, scipy's L-BFGS-B on logistic data with a DERIVED bound, the mechanics of the ring and
the refusals of tinyopt_amd.api.Optimize for Options.LBFGS (over a recording stand-in of the library).  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gd_reference as gr  # noqa: E402
import lbfgs_reference as lr  # noqa: E402


def _pod(**kw):
    from tinyopt_amd.api import Options
    o = Options()
    o.solver_type = Options.LBFGS
    for k, v in kw.items():
        setattr(o, k, v)
    return o.to_pod()


def _square(p, x):
    return x[0] * x[0], np.array([2.0 * x[0]])


def _logit_data(P, n, items, dtype, seed=0):
    """tests/test_gpu_gd.py::_logit_data's generator (that module needs a GPU to import)."""
    rng = np.random.default_rng(seed + 1000 * n + items)
    A = (rng.standard_normal((P, items, n)) / np.sqrt(n)).astype(dtype)
    w = rng.standard_normal((P, n))
    z = np.einsum("pin,pn->pi", A.astype(np.float64), w)
    yl = np.where(z + 0.5 * rng.standard_normal(z.shape) > 0, 1.0, -1.0).astype(dtype)
    return A, yl


# ---------------------------------------------------------------------------------------------------- 1. trajectories by hand
def test_square_from_4_by_hand():
    """c = x^2, x0 = 4.  pass 1 at 4: c 16, g 8, accepted (first); no pair: d = -8 / max(1, 8) = -1, trial 3.
    pass 2 at 3: c 9 <= 16 + 1e-4 * 1 * (8 * -1), accepted; s = -1, y = 6 - 8 = -2, s.y = 2, rho = 1/2, gamma = 2/4;
    two-loop: a = 1/2 * (-1 * 6) = -3, q = 6 - (-3)(-2) = 0, r = 0, b = 0, r = 0 + (-1)(-3 - 0) = 3, d = -3, trial 0.
    pass 3 at 0: c 0 accepted, 0 < min_error: kMinError.  Three iterations, no failure."""
    out = lr.lbfgs_optimize(np.array([[4.0]]), _square, _pod(), np.float64)
    assert out["stop"][0] == gr.STOP_MIN_ERROR and out["iters"][0] == 3 and out["fails"][0] == 0 and out["passes"][0] == 3
    assert (out["accepted_x"][0][:, 0] == [4.0, 3.0, 0.0]).all()
    assert (out["errs"][0][:3] == [16.0, 9.0, 0.0]).all() and (out["succ"][0][:3] == 1).all()
    assert (out["deltas2"][0][:3] == [0.0, 1.0, 9.0]).all()
    assert out["x"][0, 0] == 0.0 and out["cost"][0] == 0.0


def test_square_from_quarter_rejects_the_mirror_point():
    """x0 = 1/4: g = 1/2 (|g| < 1: d = -1/2), trial -1/4 has the SAME cost: 1/16 <= 1/16 - 1e-4 * 1/4 fails, rejected (min_rerr_dec = 0
    keeps the floor rule silent), alpha 1/2, trial 0 accepted: kMinError."""
    out = lr.lbfgs_optimize(np.array([[0.25]]), _square, _pod(min_rerr_dec=0.0), np.float64)
    assert out["stop"][0] == gr.STOP_MIN_ERROR and out["iters"][0] == 3 and out["fails"][0] == 1 and out["consec"][0] == 0
    assert (out["succ"][0][:3] == [1, 0, 1]).all() and (out["errs"][0][:3] == [0.0625, 0.0625, 0.0]).all()
    assert (out["deltas2"][0][:3] == [0.0, 0.25, 0.0625]).all()
    assert out["x"][0, 0] == 0.0
    # with the floor rule awake the equal cost is the round-off floor: kMinRelError at the accepted point
    out = lr.lbfgs_optimize(np.array([[0.25]]), _square, _pod(), np.float64)
    assert out["stop"][0] == gr.STOP_MIN_REL_ERROR and out["x"][0, 0] == 0.25 and out["fails"][0] == 1


def test_square_consecutive_failure_limit():
    out = lr.lbfgs_optimize(np.array([[0.25]]), _square, _pod(min_rerr_dec=0.0, max_consec_failures=1), np.float64)
    assert out["stop"][0] == gr.STOP_MAX_CONSEC_NO_DECR and out["x"][0, 0] == 0.25 and out["iters"][0] == 2
    assert out["fails"][0] == 1 and out["consec"][0] == 1 and out["cost"][0] == 0.0625
    out = lr.lbfgs_optimize(np.array([[0.25]]), _square, _pod(min_rerr_dec=0.0, max_consec_failures=0, max_total_failures=1), np.float64)
    assert out["stop"][0] == gr.STOP_MAX_NO_DECR and out["x"][0, 0] == 0.25


def test_nan_at_the_first_trial_keeps_x0():
    """c = sqrt(x) from 1/4: g = 1, d = -1, the trial -3/4 is NaN: kSystemHasNaNOrInf, x = x0, one iteration counted."""
    def f(p, x):
        with np.errstate(invalid="ignore"):
            return np.sqrt(x[0]), np.array([0.5 / np.sqrt(x[0])])
    out = lr.lbfgs_optimize(np.array([[0.25]]), f, _pod(), np.float64)
    assert out["stop"][0] == gr.STOP_NAN_OR_INF and out["x"][0, 0] == 0.25 and out["iters"][0] == 1 and out["passes"][0] == 2


# ---------------------------------------------------------------------------------------------------- 2. minimisers
def test_rosenbrock_quartic_powell():
    out = lr.lbfgs_optimize(np.array([[-1.2, 1.0]]), lambda p, x: lr.rosenbrock(x, np.float64), _pod(max_iters=200), np.float64)
    assert out["stop"][0] >= 1 and np.abs(out["x"][0] - 1.0).max() < 1e-5, (out["stop"], out["x"])
    # (the quartic's minimum is -2: min_error = 0, as tests/unconstrained.cpp sets it, or a negative cost is "below min_error")
    out = lr.lbfgs_optimize(np.array([[38.0]]), lambda p, x: gr.quartic(x, np.float64), _pod(max_iters=200, min_error=0.0), np.float64)
    assert out["stop"][0] >= 1 and abs(out["x"][0, 0] - 42.0) < 1e-5 and out["cost"][0] == pytest.approx(-2.0, abs=1e-9)
    pod = _pod(max_iters=300)
    out = lr.lbfgs_optimize(np.array([[3.0, -1.0, 0.0, 1.0]]), lambda p, x: lr.powell(x, np.float64), pod, np.float64)
    assert out["stop"][0] == gr.STOP_MIN_ERROR and out["cost"][0] < pod.min_error, (out["stop"], out["cost"])


@pytest.mark.parametrize("n,items", [(3, 64), (12, 300), (63, 1000)])
def test_logistic_against_scipy(n, items):
    """f - f* <= |g|^2 / (2 mu) for a mu-strongly convex f: mu = the smallest eigenvalue of the closed-form Hessian A^T D A
    (D = sigma (1 - sigma)) at scipy's solution, less the 10 % by which the Hessian can shrink between two points this close; g the
    restatement's fp64 gradient at its final x.  scipy's end lies above f* too, by at most its own bound: the larger of the two bounds
    the difference."""
    from scipy.optimize import minimize
    A, yl = _logit_data(4, n, items, np.float64)
    pod = _pod(max_iters=200, min_rerr_dec=0.0)   # (run to the gradient's floor: the bound is in terms of |g|)
    pod.min_step_norm2 = 0.0
    for p in range(4):
        f = lambda x, p=p: gr.logistic(A[p], yl[p], x, np.float64)   # noqa: E731
        x, st, *_ = lr.lbfgs_solve_one(np.zeros(n), f, pod, np.float64, pod.max_iters + 2)
        sp = minimize(lambda x: float(f(x)[0]), np.zeros(n), jac=lambda x: f(x)[1], method="L-BFGS-B", options=dict(gtol=1e-10, ftol=0, maxiter=2000))
        z = A[p] @ sp.x
        sig = 1.0 / (1.0 + np.exp(-z))
        # (mu must lie below the Hessian on the way to the minimiser: sigma (1 - sigma) changes by at most exp(-|dz|) over a change dz
        #  of an item's z, |dz| <= |a_i| |dx|; the factor is computed — three times the distance of the two ends — and must stay above 0.9)
        assert np.exp(-3 * np.linalg.norm(A[p], axis=1).max() * np.linalg.norm(x - sp.x)) >= 0.9
        mu = 0.9 * np.linalg.eigvalsh(A[p].T @ (A[p] * (sig * (1 - sig))[:, None])).min()
        assert mu > 0
        g_mine, g_sp = f(x)[1], f(sp.x)[1]
        # (both ends lie above f*, each by at most its own bound: they differ by at most the larger; plus the round-off of f in fp64)
        bound = max(g_mine @ g_mine, g_sp @ g_sp) / (2 * mu) + 8 * items * np.finfo(np.float64).eps * abs(sp.fun)
        print(f"n={n} items={items} p={p}: f {float(f(x)[0]):.12g} scipy {sp.fun:.12g} bound {bound:.3g} iters {st['iters']}")
        assert abs(float(f(x)[0]) - sp.fun) <= bound, (p, float(f(x)[0]), sp.fun, bound)


# ---------------------------------------------------------------------------------------------------- 3. mechanics
def _logit_batch(n, items, dtype, P=6, **kw):
    A, yl = _logit_data(P, n, items, dtype)
    pod = _pod(**kw)
    return A, yl, pod, lambda p, x: gr.logistic(A[p], yl[p], x, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_accepted_costs_never_increase_and_x_is_accepted(dtype):
    A, yl, pod, f = _logit_batch(12, 65, dtype, max_iters=40)
    out = lr.lbfgs_optimize(np.zeros((6, 12), dtype), f, pod, dtype)
    for p in range(6):
        k = out["iters"][p]
        acc = out["errs"][p][:k][out["succ"][p][:k] == 1]
        assert (np.diff(acc) <= 0).all(), (p, acc)
        assert (out["x"][p] == out["accepted_x"][p][-1]).all()
        assert out["cost"][p] == acc[-1]


def test_x_out_is_an_accepted_point_in_every_stop_branch():
    stops = set()
    cases = [dict(), dict(max_iters=3), dict(min_rerr_dec=0.0, max_iters=60), dict(min_grad_norm2=1e-2), dict(min_step_norm2=1e-2),
             dict(min_error=100.0), dict(min_rerr_dec=0.0, min_step_norm2=0.0, max_consec_failures=2, max_iters=200),
             dict(min_rerr_dec=0.0, min_step_norm2=0.0, max_consec_failures=0, max_total_failures=3, max_iters=200)]
    for kw in cases:
        A, yl, pod, f = _logit_batch(3, 64, np.float32, **kw)
        out = lr.lbfgs_optimize(np.zeros((6, 3), np.float32), f, pod, np.float32)
        for p in range(6):
            stops.add(int(out["stop"][p]))
            assert any((out["x"][p] == a).all() for a in out["accepted_x"][p]), (kw, p)
            assert (out["x"][p] == out["accepted_x"][p][-1]).all()
    # kSystemHasNaNOrInf: sqrt(x) from 1, 1/4 and 4 — the first trial x0 - g / max(1, |g|) is negative for the first two only
    def root(p, x):
        with np.errstate(invalid="ignore"):
            return np.float32(np.sqrt(x[0])), np.array([0.5 / np.sqrt(x[0])], np.float32)
    out = lr.lbfgs_optimize(np.array([[0.25], [0.125]], np.float32), root, _pod(), np.float32)
    for p in range(2):
        stops.add(int(out["stop"][p]))
        assert out["x"][p, 0] == [0.25, 0.125][p] and (out["x"][p] == out["accepted_x"][p][-1]).all()
    every = {gr.STOP_NAN_OR_INF, gr.STOP_MIN_ERROR, gr.STOP_MIN_REL_ERROR, gr.STOP_MIN_DELTA_NORM, gr.STOP_MIN_GRAD_NORM, gr.STOP_MAX_ITERS,
             gr.STOP_MAX_NO_DECR, gr.STOP_MAX_CONSEC_NO_DECR}
    assert stops == every, (stops, every)   # every StopReason the state machine can set (kSkipped is the kernel's, for a problem without items)


def test_ring_wraps_and_history_beyond_the_accepted_steps_changes_nothing():
    A, yl, pod, f = _logit_batch(63, 1000, np.float64, P=2, max_iters=100, min_rerr_dec=1e-14)
    x0 = np.zeros((2, 63))
    ref = lr.lbfgs_optimize(x0, f, pod, np.float64, history=16)
    for h in (1, 3):
        out = lr.lbfgs_optimize(x0, f, pod, np.float64, history=h)
        assert (out["succ"].sum(axis=1) > 10).all(), (h, out["succ"].sum(axis=1))          # the ring has wrapped
        assert (out["stop"] >= 1).all() and (out["stop"] < 5).all(), (h, out["stop"])      # Converged
        assert np.allclose(out["cost"], ref["cost"], rtol=1e-8), (h, out["cost"], ref["cost"])
    A, yl, pod, f = _logit_batch(12, 300, np.float64, P=2)
    a = lr.lbfgs_optimize(np.zeros((2, 12)), f, pod, np.float64, history=16)
    b = lr.lbfgs_optimize(np.zeros((2, 12)), f, pod, np.float64, history=63, ring_limit=False)
    assert (a["succ"].sum(axis=1) < 16).all()
    for k in ("x", "errs", "succ", "deltas2", "iters", "stop", "cost"):
        assert (a[k] == b[k]).all(), k


# ---------------------------------------------------------------------------------------------------- 4. refusals (no GPU: a recording library)
class _RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        from tinyopt_amd import _capi
        if name not in _capi.PROTOTYPES:
            raise AttributeError(name)

        def entry(*args):
            assert len(args) == len(_capi.PROTOTYPES[name][1]), name
            self.calls.append((name, args))
            return 0
        return entry


class _Ctx:
    device = 0

    def __init__(self):
        self.lib, self.h = _RecordingLib(), C.c_void_p(0x1000)


class _CudaLike:
    is_cuda = True

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return getattr(self._t, name)


_KEEP = []


def _cost_model(kind="cost_grad", ragged=False, n=3):
    from tinyopt_amd import api
    r = object.__new__(api.JitResidual)
    r.__dict__.update(ctx=_Ctx(), n=n, kR=1, kD=2, kH=0, dtype=torch.float64, manifold="euclid", kind=kind, diff="ad", diff_h=0.0, large_n=False,
                      xdim=n, _h=C.c_void_p(0x2000))
    _KEEP.append(r)
    if ragged:
        m = object.__new__(api.RaggedJitModel)
        off = torch.tensor([0, 2, 2, 7])
        m.__dict__.update(res=r, P=3, n=n, xdim=n, dtype=torch.float64, total_items=7, max_items=5, offsets_host=off, offsets=off,
                          data=torch.ones(7, 2, dtype=torch.float64), header=None)
    else:
        m = object.__new__(api.JitModel)
        m.__dict__.update(res=r, P=3, items=4, n=n, dtype=torch.float64, xdim=n, m=4, packed=torch.ones(3, 8, dtype=torch.float64))
    return m


def _optimize(model, **kw):
    from tinyopt_amd import api
    o = api.Options()
    o.solver_type = api.Options.LBFGS
    for k, v in kw.pop("lbfgs", {}).items():
        setattr(o.lbfgs, k, v)
    call_kw = {k: kw.pop(k) for k in ("splits",) if k in kw}
    for k, v in kw.items():
        setattr(o, k, v)
    ctx = _Ctx()
    x = _CudaLike(torch.zeros(3, model.n, dtype=torch.float64))
    out = api.Optimize(x, model, o, ctx=ctx, **call_kw)
    return out, ctx.lib.calls


@pytest.mark.parametrize("ragged", [False, True])
def test_optimize_routes_lbfgs_to_its_entry(ragged):
    from tinyopt_amd import _capi
    out, calls = _optimize(_cost_model(ragged=ragged), lbfgs=dict(history=5, c1=0.01, shrink=0.25))
    names = [c[0] for c in calls]
    assert names == ["toa_set_loss", "toa_lbfgs_options_default", "toa_jit_lbfgs_run_ragged" if ragged else "toa_jit_lbfgs_run"], names
    args = calls[-1][1]
    pods = [a._obj for a in args if hasattr(a, "_obj")]
    lb = [p for p in pods if isinstance(p, _capi.ToaLbfgsOptions)][0]
    assert (lb.history, lb.c1, lb.shrink) == (5, pytest.approx(0.01), 0.25)
    opt = [p for p in pods if isinstance(p, _capi.ToaOptions)][0]
    assert opt.solver_type == 3
    res = [p for p in pods if isinstance(p, _capi.ToaResults)][0]
    assert not res.final_hessian and out.final_hessian is None
    assert not hasattr(_capi.ToaOptions, "history")   # (toa_options is untouched: the block travels beside it)


@pytest.mark.parametrize("kw,text", [
    (dict(lbfgs=dict(history=0)), "history"), (dict(lbfgs=dict(history=17)), "history"),
    (dict(lbfgs=dict(c1=0.0)), "c1"), (dict(lbfgs=dict(c1=1.0)), "c1"), (dict(lbfgs=dict(shrink=0.0)), "shrink"), (dict(lbfgs=dict(shrink=1.0)), "shrink"),
    (dict(grad_clipping=0.5), "grad_clipping"), (dict(splits=4), "splits"), (dict(max_duration_ms=5.0), "max_duration_ms"),
    (dict(stop_callback=lambda e, d, g: False), "stop callbacks")])
def test_optimize_refuses_before_any_library_call(kw, text):
    with pytest.raises(ValueError, match=text):
        _optimize(_cost_model(), **kw)


def test_optimize_refuses_models_that_are_no_first_order_cost():
    from tinyopt_amd import api
    for kind in ("residual", "accumulate", "cost_hess"):
        with pytest.raises(ValueError, match="L-BFGS"):
            _optimize(_cost_model(kind=kind))
    dense = object.__new__(api.DenseRow)
    dense.__dict__.update(packed=torch.ones(64, dtype=torch.float64), n=3, m=5, P=3, dtype=torch.float64)
    with pytest.raises(ValueError, match="scalar cost model"):
        _optimize(dense)
    m = _cost_model(kind="residual")
    m = m.with_prior(torch.zeros(3, 3, dtype=torch.float64), torch.ones(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="no L-BFGS"):
        _optimize(m)
    o = api.Options()
    o.solver_type = api.Options.LBFGS
    with pytest.raises(ValueError, match="no stepping form"):
        api.Optimizer(_CudaLike(torch.zeros(3, 3, dtype=torch.float64)), _cost_model(), o, ctx=_Ctx())


def test_restatement_refuses_the_same_ranges():
    pod = _pod()
    for kw in (dict(history=0), dict(history=17), dict(c1=0.0), dict(c1=1.0), dict(shrink=0.0), dict(shrink=1.0)):
        with pytest.raises(ValueError):
            lr.lbfgs_optimize(np.zeros((1, 1)), _square, pod, np.float64, **kw)
    with pytest.raises(ValueError):
        lr.lbfgs_optimize(np.zeros((1, 1)), _square, _pod(grad_clipping=1.0), np.float64)


# ---------------------------------------------------------------------------------------------------- the comparison the GPU tests use
def _case(n, items, dtype, P=97, **kw):
    A, yl, _ = lr.logit_data(P, n, items, dtype)
    kw = dict(dict(max_iters=40), **kw)
    if dtype == np.float32:
        kw = dict(dict(min_error=1e-3, min_rerr_dec=1e-3), **kw)   # (thresholds of fp32's own precision: tests/test_gpu_lbfgs.py)
    pod = _pod(**kw)
    eps = float(np.finfo(dtype).eps)
    noise = lambda p, c: eps * ((items + 4) * abs(c) + items)   # noqa: E731
    f = lambda p, x: gr.logistic(A[p], yl[p], x, dtype)   # noqa: E731
    fast = lambda p, x: lr.logistic_fast(A[p], yl[p], x, dtype)   # noqa: E731
    x0 = np.zeros((P, n), dtype)
    ref = lr.lbfgs_optimize(x0, f, pod, dtype)
    twins = [lr.lbfgs_optimize(x0, lr.perturbed(fast, 4 * eps, s), pod, dtype) for s in (1, 2, 3, 4)]
    return x0, f, pod, noise, ref, twins


@pytest.mark.parametrize("n,items,dtype", [(12, 64, np.float32), (13, 1000, np.float32), (1, 1, np.float64), (63, 64, np.float64)])
def test_a_fourth_twin_passes_the_comparison_within_the_cap(n, items, dtype):
    """Four of the GPU test's forty cases (seed 0, P = 97), among them the two most sensitive (one item and one parameter; separable
    at n = 63): the ill-determined problems found by three twins, a FOURTH twin as the run — full or parted inside the 5 % cap."""
    x0, f, pod, noise, ref, twins = _case(n, items, dtype)
    ill = lr.ill_determined(ref, twins[:3], dtype, noise)
    st = lr.compare_trajectories(twins[3], ref, dtype, noise, ill=ill)
    print(n, items, dtype.__name__, st)
    assert st["parted"] <= 0.05 * 97 and st["max_cost_dev"] <= lr.K_COST, st


def test_comparison_refuses_a_different_solver_and_a_wrong_cost():
    """A run with one pair of history is no rounding of the run with eight, and a cost that is off by 1e-9 in fp64 is no round-off."""
    x0, f, pod, noise, ref, twins = _case(12, 300, np.float64, P=8)
    ill = lr.ill_determined(ref, twins[:3], np.float64, noise)
    assert not ill.any()
    st = lr.compare_trajectories(twins[3], ref, np.float64, noise, ill=ill)
    assert st["full"] + st["parted"] == 8 and st["parted"] <= 1
    other = lr.lbfgs_optimize(x0, f, pod, np.float64, history=1)
    with pytest.raises(AssertionError):
        lr.compare_trajectories(other, ref, np.float64, noise, ill=ill)
    wrong = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
    wrong["errs"][3, 2] *= 1 + 1e-9
    with pytest.raises(AssertionError, match="well-determined"):
        lr.compare_trajectories(wrong, ref, np.float64, noise, ill=ill)
    wrong = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
    wrong["x"][5] += 1e-6
    with pytest.raises(AssertionError, match="well-determined"):
        lr.compare_trajectories(wrong, ref, np.float64, noise, ill=ill)


def test_a_cost_model_never_carries_a_prior_or_bounds():
    """with_prior / with_bounds refuse a cost model when they are attached, so the ("prior" | "bounds", "lbfgs") refusals of Optimize
    can only ever speak for a residual model."""
    m = _cost_model()
    with pytest.raises(ValueError, match="scalar cost model"):
        m.with_prior(torch.zeros(3, 3, dtype=torch.float64), torch.ones(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="scalar cost model"):
        m.with_bounds(torch.zeros(3, 3, dtype=torch.float64) - 1, None)
