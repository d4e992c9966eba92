"""Box bounds on the CPU: the rules of tests/bounds_reference.py around the second reading's LM loop — that
bounds which never bind change nothing, that a fixed parameter is the reduced problem, and that the active-set rule finds the
constrained optimum of bounded linear least squares (against enumeration)."""
import numpy as np
import pytest

import bounds_reference as br

ref = br.ref
INF = br.INF


def _decisions(out):
    return (tuple(out["successes"]), out["stop"], out["num_iters"], out["num_failures"], tuple(t["rebuilt"] for t in out["trace"]))


@pytest.mark.parametrize("name,x0,kw", [
    ("beale", [1.0, 1.0], dict(max_iters=200, max_consec_failures=0, min_error=1e-30, damping_init=1e-3)),
    ("beale", [0.5, 1.5], dict(max_iters=200, max_consec_failures=5, min_error=1e-30, damping_init=1e-3)),
    ("himmelblau", [3.5, 2.5], dict(max_iters=200, max_consec_failures=0, min_error=1e-30)),
    ("himmelblau", [0.0, 0.0], dict(max_iters=200, max_consec_failures=0, min_error=1e-30, damping_init=1e-2)),
])
def test_infinite_bounds_reproduce_optimize(name, x0, kw):
    """(a) with -inf / +inf the wrapper is the identity: the same decisions, every x of the trace bit for bit"""
    opt = ref.Options(**kw)
    plain = ref.optimize(name, x0, opt)
    out = br.optimize_bounded(ref.FUNCS[name], x0, opt, [-INF] * 2, [INF] * 2)
    assert _decisions(out) == _decisions(plain)
    assert out["x"] == plain["x"] and out["errs"] == plain["errs"] and out["deltas2"] == plain["deltas2"]
    assert [t["x"] for t in out["trace"]] == [t["x"] for t in plain["trace"]]
    assert out["final_hessian"] == plain["final_hessian"]


@pytest.mark.parametrize("name,x0,fixed,kw", [
    ("beale", [1.0, 1.0], 1, dict(max_iters=200, max_consec_failures=0, min_error=1e-30, damping_init=1e-3)),
    ("beale", [1.0, 0.3], 0, dict(max_iters=200, max_consec_failures=0, min_error=1e-30, damping_init=1e-3)),
    ("himmelblau", [3.5, 2.5], 1, dict(max_iters=200, max_consec_failures=0, min_error=1e-30)),
    ("himmelblau", [3.5, 2.5], 0, dict(max_iters=200, max_consec_failures=0, min_error=1e-30)),
])
def test_fixed_parameter_is_the_reduced_problem(name, x0, fixed, kw):
    """(b) lo == hi on one parameter: `optimize` on the function of the other parameter alone — costs, decisions, the free x"""
    opt = ref.Options(**kw)
    fn = ref.FUNCS[name]
    free = 1 - fixed

    def reduced(v, want):
        full = [0.0, 0.0]
        full[free], full[fixed] = v[0], x0[fixed]
        c, g, H, nres = fn(full, want)
        return (c, [g[free]], [[H[free][free]]], nres) if want else (c, None, None, nres)

    want = br.optimize_plain(reduced, [x0[free]], opt)
    lo, hi = [-INF, -INF], [INF, INF]
    lo[fixed] = hi[fixed] = x0[fixed]
    out = br.optimize_bounded(fn, x0, opt, lo, hi)
    assert _decisions(out) == _decisions(want)
    assert out["x"][fixed] == x0[fixed]
    np.testing.assert_allclose(out["errs"], want["errs"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(out["x"][free], want["x"][0], rtol=1e-12, atol=0)
    for t, tw in zip(out["trace"], want["trace"]):
        assert t["x"][fixed] == x0[fixed]
        np.testing.assert_allclose(t["x"][free], tw["x"][0], rtol=1e-12, atol=0)


def test_bounded_dense_problems_reach_the_brute_force_optimum():
    """(c) 200 seeded dense problems (n = 4, m = 9), max_consec_failures = 30: x is inside the box exactly and the final cost is within
    1e-10 relative of the bounded optimum found by enumerating the 3^4 patterns free / at lo / at hi.  The tolerance is the issue's; the
    stop tests are switched off except the step norm (1e-30) so that a solve ends on its optimum, not on a relative-decrease test."""
    opt = ref.Options(max_iters=300, max_consec_failures=30, min_error=0.0, min_rerr_dec=0.0, min_step_norm2=1e-30, min_grad_norm2=1e-30)
    worst, ends_on_bound, nfixed = 0.0, 0, 0
    for seed in range(200):
        A, b, x0, lo, hi = br.dense_case(seed)
        out = br.optimize_bounded(br.dense_fn(A, b), list(x0), opt, list(lo), list(hi))
        x = np.array(out["x"])
        assert np.all(x >= lo) and np.all(x <= hi), (seed, x, lo, hi)
        for t in out["trace"]:
            assert all(a <= v <= c for v, a, c in zip(t["x"], lo, hi)), seed
        best = br.brute_force_optimum(A, b, lo, hi)
        r = A @ x - b
        excess = (float(r @ r) - best) / best
        worst = max(worst, excess)
        assert excess <= 1e-10, (seed, excess, out["stop"], out["num_iters"])
        ends_on_bound += int(np.any((x == lo) | (x == hi)))
        nfixed += int(np.any(lo == hi))
    print(f"worst relative excess over the brute-force optimum: {worst:.3g}; {ends_on_bound} of 200 end on a bound, {nfixed} with a fixed parameter")
    assert ends_on_bound >= 100 and nfixed == 40
