"""The yardstick of the second-order scalar costs (tests/hess_reference.py) held to itself and to the committed traces, and the Python
routes of kind="cost_hess" with the recording library of tests/test_cpu_api_routes.py.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hess_reference as hr  # noqa: E402
from parity import check_against_trace  # noqa: E402
from test_cpu_api_routes import F64, P, CudaLike, StubContext, _jit, _name_pointers  # noqa: E402
from tinyopt_amd import api  # noqa: E402

EPS = 2.0 ** -52
LOGISTIC_ITEMS, LOGISTIC_X0 = hr.logistic_case(3, 4, 5)
SPOT_ITEMS, SPOT_X0 = hr.spot_case(4)
RNG = np.random.default_rng(5)
CALLBACKS = {   # name: (term, items, points)
    "rosenbrock": (hr.rosenbrock_term, [[0.0]], [[-1.2, 1.0], [0.3, 0.7], [1.0, 1.0]]),
    "plateau": (hr.plateau_term, [[0.0]], [[3.0, 3.0], [2.6, 2.6], [3.3, 2.9]]),
    "powell": (hr.powell_term, [[0.0]], [[3.0, -1.0, 0.0, 1.0], [0.5, 0.2, -0.3, 0.4]]),
    "quadratic": (hr.quadratic_term, RNG.integers(-4, 5, (7, 4)) / 4.0, [[0.25, -0.5, 1.0], [0.0, 0.0, 0.0]]),
    "logistic": (hr.logistic_term, LOGISTIC_ITEMS, [list(LOGISTIC_X0), [0.0] * 4, [1.5, -2.0, 0.5, 1.0]]),
    "spot": (hr.spot_term, SPOT_ITEMS[::6], [list(SPOT_X0), [80.0, 3.0, 3.0, 5.0]]),
    "saddle": (hr.saddle_term, [[0.0]], [[0.0, 0.5], [0.3, -0.4], [-0.9, 0.2]]),
}


def central(f, x, a, h):
    xp, xm = list(x), list(x)
    xp[a] += h
    xm[a] -= h
    return (np.asarray(f(xp)) - np.asarray(f(xm))) / (xp[a] - xm[a])


def third_derivative(f, x, a, d=1e-2):
    """|d^3 f / dx_a^3| near x from the five-point stencil with a coarse step: what the truncation bound below is scaled by."""
    def at(k):
        y = list(x)
        y[a] += k * d
        return np.asarray(f(y))
    return np.abs(at(2) - 2.0 * at(1) + 2.0 * at(-1) - at(-2)) / (2.0 * d ** 3)


@pytest.mark.parametrize("name", list(CALLBACKS))
def test_callbacks_are_their_own_derivatives(name):
    """g against central differences of c, and H against central differences of g, with step h = 1e-5 max(1, |x_a|).  The textbook bound
    of a central difference of f: truncation h^2 / 6 |f'''| plus rounding eps |f| / h (two values of f, each rounded to eps |f| / 2 by
    a sum that is itself accurate to a few eps: a factor 8 covers the items' sums).  |f'''| is taken from a coarse five-point stencil
    and doubled.
    The plateau is the reference's callback AS WRITTEN (tests/optimize_easy.cpp:88-144, what the oracle and the committed traces run):
    its H(0, 1) has the opposite sign of d^2 f / dx dy = -ex (sx + 2 dx cx) (sy + 2 dy cy).  The test states that and holds the entry
    to the derivative's magnitude."""
    term, items, points = CALLBACKS[name]
    fn = hr.item_sum(term, items)
    for x in points:
        c, g, H, nres = fn(list(x), True)
        assert nres == 1 and fn(list(x), False)[0] == c
        n = len(x)
        assert all(H[a][b] == H[b][a] for a in range(n) for b in range(n))
        cost = lambda y: fn(y, True)[0]   # noqa: E731
        grad = lambda y: fn(y, True)[1]   # noqa: E731
        for a in range(n):
            h = 1e-5 * max(1.0, abs(x[a]))
            bound_c = h * h / 6.0 * 2.0 * third_derivative(cost, x, a) + 8.0 * EPS * max(abs(c), 1.0) / h
            assert abs(central(cost, x, a, h) - g[a]) <= bound_c, (name, x, a, "g", central(cost, x, a, h), g[a], bound_c)
            gscale = max(1.0, max(abs(v) for v in g))
            bound_g = h * h / 6.0 * 2.0 * third_derivative(grad, x, a) + 8.0 * EPS * gscale / h
            col = central(grad, x, a, h)
            want = np.array([H[b][a] * (-1.0 if (name == "plateau" and a != b) else 1.0) for b in range(n)])
            assert (np.abs(col - want) <= bound_g).all(), (name, x, a, "H", col, H, bound_g)


def test_reference_functions_reproduce_the_committed_traces():
    """Rosenbrock, plateau and Powell as item sums of ONE item run the committed second reading to its committed traces."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_traces.json")) as f:
        cases = json.load(f)["cases"]
    terms = {"rosenbrock": hr.rosenbrock_term, "plateau": hr.plateau_term, "powell": hr.powell_term}
    seen = {k: 0 for k in terms}
    for c in cases:
        if c["function"] not in terms or c.get("dtype", "float64") != "float64":
            continue
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in c["options"].items()}
        opt = hr.ref.Options()
        for k, v in kw.items():   # (the stored values are the promoted floats already)
            setattr(opt, k, v)
        r = hr.optimize(terms[c["function"]], [[0.0]], c["x0"], opt)
        got = dict(errs=r["errs"], deltas2=r["deltas2"], succ=[int(s) for s in r["successes"]], stop=r["stop"], iters=r["num_iters"],
                   fails=r["num_failures"], x=r["x"], cost=r["final_cost"])
        assert check_against_trace(c, got, label=f'{c["function"]} {c["x0"]} {c["comment"]}') in ("full", "tie")
        seen[c["function"]] += 1
    assert all(v >= 5 for v in seen.values()), seen


# ---- the Python routes ---------------------------------------------------------------------------------------------------------------
def _hess():
    return _jit(kind="cost_hess")


def _call(fn):
    """(exception or None, the library calls made) of fn(cost, x, ctx)."""
    cost, ctx = _hess(), StubContext()
    x = CudaLike(torch.ones(P, cost.n, dtype=F64))
    _name_pointers(ctx, cost, x)
    try:
        fn(cost, x, ctx)
        return None, ctx.lib.calls
    except Exception as e:  # noqa: BLE001
        return e, ctx.lib.calls


@pytest.mark.parametrize("solver", [api.Options.LevenbergMarquardt, api.Options.GaussNewton])
def test_cost_hess_reaches_toa_jit_lm_run(solver):
    o = api.Options()
    o.solver_type = solver
    err, calls = _call(lambda cost, x, ctx: api.Optimize(x, cost, o, ctx=ctx))
    assert err is None
    run = [c for c in calls if c[0].startswith("toa_jit_")]
    assert [c[0] for c in run] == ["toa_jit_lm_run"] and run[0][2:5] == ["handle", "model", 4]
    pod = next(a for a in run[0] if isinstance(a, dict) and a.get("pod") == "ToaOptions")
    assert pod["solver_type"] == solver and pod["save_last"] == 1
    # the seam: g, the full H, the cost
    err, calls = _call(lambda cost, x, ctx: api.accumulate(cost, x, ctx=ctx))
    acc = [c for c in calls if c[0] == "toa_jit_accumulate"]
    assert err is None and len(acc) == 1 and "NULL" not in acc[0][9:12]   # want_grad = 1: g, H and the cost are all handed over
    assert acc[0][8] == 1


PREFIX = 'a second-order scalar cost (kind="cost_hess") runs in the uniform one-launch form through Optimize (LM / GN), accumulate and CheckGradient only: '


def _options(**kw):
    o = api.Options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


REFUSED_CALLS = {
    "GradientDescent": (lambda cost, x, ctx: api.Optimize(x, cost, _options(solver_type=api.Options.GradientDescent), ctx=ctx),
                        "no GradientDescent: the reference throws for f(x, grad, H) under GradientDescent too (optimize.h:59-75)"),
    "splits": (lambda cost, x, ctx: api.Optimize(x, cost, api.Options(), ctx=ctx, splits=2), "no row-split form (splits): its Hessian is no Gram of rows to split"),
    "max_duration_ms": (lambda cost, x, ctx: api.Optimize(x, cost, _options(max_duration_ms=5.0), ctx=ctx),
                        "no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)"),
    "stop_callback": (lambda cost, x, ctx: api.Optimize(x, cost, _options(stop_callback=lambda e, d, g: False), ctx=ctx),
                      "no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)"),
    "Optimizer": (lambda cost, x, ctx: api.Optimizer(x, cost, api.Options(), ctx=ctx), "no stepping form (Optimizer)"),
    "Eval": (lambda cost, x, ctx: api.Eval(cost, x, ctx=ctx), "no Eval (it has no residual rows: accumulate returns its value, its gradient and its Hessian)"),
    "CalculateJac": (lambda cost, x, ctx: api.CalculateJac(cost, x, ctx=ctx),
                     "no CalculateJac (it has no residual rows: accumulate returns its value, its gradient and its Hessian)"),
    "with_loss": (lambda cost, x, ctx: cost.with_loss("huber", 1.0), "no M-estimator (with_loss): a scalar cost has no residuals to robustify"),
    "with_prior": (lambda cost, x, ctx: cost.with_prior(torch.zeros(P, cost.n, dtype=F64), torch.ones(P, cost.n, dtype=F64)),
                   "no Gaussian prior (with_prior): a prior is a block of residuals, and it has none"),
    "with_bounds": (lambda cost, x, ctx: cost.with_bounds(torch.zeros(P, cost.n, dtype=F64), None),
                    "no box bounds (with_bounds): they project the Gauss-Newton system of a residual model"),
    "bind_ragged": (lambda cost, x, ctx: cost.res.bind_ragged(torch.ones(7, 2, dtype=F64), counts=[2, 0, 5]), "no ragged batches (bind_ragged)"),
}


@pytest.mark.parametrize("what", list(REFUSED_CALLS))
def test_refusals_before_any_call(what):
    fn, text = REFUSED_CALLS[what]
    err, calls = _call(fn)
    assert isinstance(err, ValueError) and str(err) == PREFIX + text, (what, err)
    assert calls == []


@pytest.mark.parametrize("kw,text", [
    (dict(manifold="se3"), "Euclidean parameters only, not manifold='se3'"),
    (dict(diff="central"), 'the body brings its own derivatives, nothing is differentiated: diff="ad" only, not diff=\'central\''),
    (dict(large_n=True), "no large_n (the launch-per-phase pipeline is for residual models)"),
    (dict(residuals_per_item=2), "an item has one cost term: residuals_per_item = 1, not 2"),
    (dict(n=13), "1 <= n <= 12 in float32 and float64 (the Hessian's triangle, n (n + 1) / 2 <= 78 accumulators, is kept in registers), not n = 13 (91 accumulators)"),
    (dict(n=0), "1 <= n <= 12 in float32 and float64 (the Hessian's triangle, n (n + 1) / 2 <= 78 accumulators, is kept in registers), not n = 0 (0 accumulators)"),
])
def test_construction_refusals_before_any_call(kw, text):
    ctx = StubContext()
    args = dict(n=2, item_scalars=1, kind="cost_hess", dtype=F64, ctx=ctx)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        api.JitResidual("c = x[0];", **args)
    assert str(e.value) == PREFIX + text and ctx.lib.calls == []
