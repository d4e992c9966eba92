"""The yardstick of the constant-camera / constant-point tests: the projection of that section around the
committed second reading of a bundle adjustment (tests/golden/make_reference_traces_ba.py, imported as a module: it is side-effect
free, and through it part 1's loop, make_reference_traces.optimize).  Nothing here reads the loop again — `optimize` runs it; this
file only wraps the cost callback fn(x, want) -> (cost, g, H, nres) of `make_cost`: on every Build, for every tangent index of a
constant block (cameras first, six each, then three per point), g_i = 0, row and column i of the full (6C + 3N)^2 Hessian = 0 and
H_ii = 1.  The loop then applies grad_clipping, check_min_H_diag and the damping to that system, as it does to any other.  A
cost-only call is untouched.  Needs numpy only.
"""
import importlib.util
import itertools
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load():
    name = "toa_make_reference_traces_ba"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, "golden", "make_reference_traces_ba.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


gen = _load()          # make_cost, make_plus, scene
base = gen.base        # Options, optimize, decisions, the StopReason integers


def constant_indices(C, N, cams=(), pts=()):
    """Tangent indices of the constant blocks: 6 c .. 6 c + 5 for camera c, 6 C + 3 j .. + 2 for point j."""
    idx = [6 * c + k for c in sorted(cams) for k in range(6)] + [6 * C + 3 * j + k for j in sorted(pts) for k in range(3)]
    assert all(0 <= c < C for c in cams) and all(0 <= j < N for j in pts)
    return idx


def project(g, H, idx):
    """g_i = 0, row and column i of H = 0, H_ii = 1 for every i of idx.  Returns new (g, H)."""
    fixed = set(idx)
    n = len(g)
    g = [0.0 if i in fixed else g[i] for i in range(n)]
    H = [[(1.0 if i == j else 0.0) if (i in fixed or j in fixed) else H[i][j] for j in range(n)] for i in range(n)]
    return g, H


def constant(fn, idx):
    """fn with the projection on every Build; a cost-only call is untouched."""
    def wrapped(x, want):
        c, g, H, nres = fn(x, want)
        if want:
            g, H = project(g, H, idx)
        return c, g, H, nres
    return wrapped


def options_from_pod(pod):
    """The second reading's Options from a ToaOptions pod (its floats are the reference's floats already)."""
    return base.Options(solver="lm" if pod.solver_type == 0 else "gn", check_final_cost=bool(pod.check_final_cost),
                        use_step_quality_approx=bool(pod.use_step_quality_approx), grad_clipping=pod.grad_clipping, use_ldlt=bool(pod.use_ldlt),
                        check_min_H_diag=pod.check_min_H_diag, use_squared_norm=bool(pod.use_squared_norm), downscale_by_2=bool(pod.downscale_by_2),
                        normalize=bool(pod.normalize), max_iters=pod.max_iters, min_error=pod.min_error, min_rerr_dec=pod.min_rerr_dec,
                        min_step_norm2=pod.min_step_norm2, min_grad_norm2=pod.min_grad_norm2, max_total_failures=pod.max_total_failures,
                        max_consec_failures=pod.max_consec_failures, damping_init=pod.damping_init,
                        damping_range=(pod.damping_min, pod.damping_max), good_factor=pod.good_factor, bad_factor=pod.bad_factor)


_counter = itertools.count()


def optimize_constant(C, N, f, cx, cy, uv, vis, x0, opt, cams=(), pts=(), kind=None, th2=0.0, perturb=None):
    """`optimize` of the second reading on the scene with the given cameras / points constant: its output dict, plus "evals" (the
    (inliers, residuals) of every cost call)."""
    tally = []
    fn = constant(gen.make_cost(C, N, f, cx, cy, uv, vis, kind, th2, tally), constant_indices(C, N, cams, pts))
    name = f"_ba_constant_{next(_counter)}"
    base.FUNCS[name] = fn
    try:
        kw = {} if perturb is None else dict(perturb=perturb)
        out = base.optimize(name, list(x0), opt, plus=gen.make_plus(C, N), ndim=6 * C + 3 * N, **kw)
    finally:
        del base.FUNCS[name]
    out["evals"] = tally
    return out


def robust_ok(C, N, f, cx, cy, uv, vis, x0, opt, out, **kw):
    """The generator's own rule for a usable case: no accept / reject decision closer than 1e-9 to flipping, and the same decisions
    with every cost perturbed by +-1e-13 (alternating signs)."""
    if not out["min_margin"] >= 1e-9:
        return False
    for eps in (1e-13, -1e-13):
        ctr = [0]

        def perturb(c_, eps=eps, ctr=ctr):
            ctr[0] += 1
            return c_ * (1.0 + eps * (1 if ctr[0] % 2 else -1))
        if base.decisions(optimize_constant(C, N, f, cx, cy, uv, vis, x0, opt, perturb=perturb, **kw)) != base.decisions(out):
            return False
    return True
