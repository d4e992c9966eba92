"""The yardstick of the box-bounds tests: the rules of csrc/bounds.hpp around the committed second reading of the
LM loop (tests/golden/make_reference_traces.py, imported as a module: it is side-effect free and has the hooks).  Nothing here reads
the loop again — `optimize` runs it; this file only

  * wraps a cost callback fn(x, want) -> (cost, g, H, nres) with rule 2 (the active set, applied to the g and H a Build returns), and
  * hands `optimize(..., plus=...)` a closure for rules 1 and 3 (the clipped step; the step TAKEN is remembered and undone on sign = -1).

Rule 1 (the start is clipped into the box) is applied to x0 before the loop starts.  Needs numpy only.
"""
import importlib.util
import itertools
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load():
    spec = importlib.util.spec_from_file_location("toa_make_reference_traces", os.path.join(_HERE, "golden", "make_reference_traces.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load()
INF = float("inf")


def clip(v, lo, hi):
    """comparisons, as the kernel: a NaN stays a NaN"""
    return lo if v < lo else (hi if v > hi else v)


def active_set(x, g, lo, hi):
    """rule 2: fixed, or on a bound with the gradient (the one the solver negates) pointing outward"""
    return [lo[j] == hi[j] or (x[j] <= lo[j] and g[j] > 0.0) or (x[j] >= hi[j] and g[j] < 0.0) for j in range(len(g))]


def project(x, g, H, lo, hi):
    """g_j = 0, row and column j of H = 0, H_jj = 1 for every active j.  Returns (g, H, active)."""
    n = len(g)
    act = active_set(x, g, lo, hi)
    g = [0.0 if act[j] else g[j] for j in range(n)]
    H = [[(1.0 if i == j else 0.0) if (act[i] or act[j]) else H[i][j] for j in range(n)] for i in range(n)]
    return g, H, act


def bounded(fn, lo, hi, log=None):
    """fn with rule 2 on every Build; a cost-only call is untouched.  log: a list that receives the active set of every Build."""
    def wrapped(x, want):
        c, g, H, nres = fn(x, want)
        if want:
            g, H, act = project(x, g, H, lo, hi)
            if log is not None:
                log.append(act)
        return c, g, H, nres
    return wrapped


def make_plus(lo, hi):
    """rules 1 and 3 for optimize(plus=...): x_j <- clip(x_j + dx_j); where the clip moved a component the step taken is x_new - x_old,
    elsewhere dx_j as it is; sign = -1 undoes the step TAKEN (and clips, which only repairs rounding)."""
    taken = [None]

    def plus(x, dx, sign):
        if sign > 0:
            out, tk = [], []
            for j in range(len(x)):
                x1 = x[j] + dx[j]
                xc = clip(x1, lo[j], hi[j])
                tk.append(dx[j] if (xc == x1 or xc != xc) else xc - x[j])
                out.append(xc)
            taken[0] = tk
            return out
        return [clip(x[j] - taken[0][j], lo[j], hi[j]) for j in range(len(x))]
    return plus


_counter = itertools.count()


def optimize_bounded(fn, x0, opt, lo, hi, log=None):
    """`optimize` of the second reading on fn inside the box: the output dict of make_reference_traces.optimize."""
    name = f"_bounded_{next(_counter)}"
    ref.FUNCS[name] = bounded(fn, lo, hi, log)
    try:
        return ref.optimize(name, [clip(v, a, b) for v, a, b in zip(x0, lo, hi)], opt, plus=make_plus(lo, hi))
    finally:
        del ref.FUNCS[name]


def optimize_plain(fn, x0, opt):
    name = f"_plain_{next(_counter)}"
    ref.FUNCS[name] = fn
    try:
        return ref.optimize(name, list(x0), opt)
    finally:
        del ref.FUNCS[name]


def dense_fn(A, b):
    """r = A x - b as a residual problem (through _from_residuals: grad = J^T r, H = J^T J, cost = |r|^2 over m residuals)"""
    A = [[float(v) for v in row] for row in A]
    b = [float(v) for v in b]

    def fn(x, want):
        r = []
        for i, row in enumerate(A):
            s = -b[i]
            for j, a in enumerate(row):
                s += a * x[j]
            r.append(s)
        return ref._from_residuals(r, A, want)
    return fn


def rosenbrock_res(x, want):
    """Rosenbrock as two residuals: r = (1 - x, 10 (y - x^2))"""
    r = [1.0 - x[0], 10.0 * (x[1] - x[0] * x[0])]
    J = [[-1.0, 0.0], [-20.0 * x[0], 10.0]]
    return ref._from_residuals(r, J, want)


def ext_rosenbrock_res(x, want):
    """extended Rosenbrock, n = 4: the pairs (0, 1) and (2, 3), two residuals each, in item order"""
    r, J = [], []
    for k in (0, 2):
        r += [1.0 - x[k], 10.0 * (x[k + 1] - x[k] * x[k])]
        a, c = [0.0] * 4, [0.0] * 4
        a[k] = -1.0
        c[k], c[k + 1] = -20.0 * x[k], 10.0
        J += [a, c]
    return ref._from_residuals(r, J, want)


def dense_case(seed, n=4, m=9):
    """A seeded dense bounded problem: intervals up to 0.6 wide around a noisy truth; every fifth seed fixes a parameter, every seventh
    leaves one side of one parameter open.  Returns A [m, n], b [m], x0, lo, hi (float64 arrays)."""
    rng = np.random.default_rng(7000 + seed)
    A = rng.normal(size=(m, n))
    xt = rng.normal(size=n)
    b = A @ xt + 0.1 * rng.normal(size=m)
    centre = xt + 0.3 * rng.normal(size=n)
    w = rng.uniform(0.0, 0.6, size=n)
    lo, hi = centre - 0.5 * w, centre + 0.5 * w
    x0 = xt + rng.normal(size=n)
    fixed = -1
    if seed % 5 == 0:
        fixed = int(rng.integers(n))
        hi[fixed] = lo[fixed]
    if seed % 7 == 0:
        k = int(rng.integers(n))
        if k == fixed:   # (the open side goes to another parameter than the fixed one)
            k = (k + 1) % n
        if rng.integers(2):
            hi[k] = INF
        else:
            lo[k] = -INF
    return A, b, x0, lo, hi


def brute_force_optimum(A, b, lo, hi):
    """min |A x - b|^2 inside the box by enumeration: every parameter free, at lo or at hi (3^n patterns), the free ones by least
    squares; the smallest cost among the patterns whose free parameters land inside their intervals."""
    m, n = A.shape
    best = INF
    for pat in itertools.product((0, 1, 2), repeat=n):
        if any((s == 1 and not np.isfinite(lo[j])) or (s == 2 and not np.isfinite(hi[j])) for j, s in enumerate(pat)):
            continue
        x = np.zeros(n)
        free = [j for j, s in enumerate(pat) if s == 0]
        for j, s in enumerate(pat):
            if s == 1:
                x[j] = lo[j]
            elif s == 2:
                x[j] = hi[j]
        if free:
            rhs = b - A @ x
            x[free] = np.linalg.lstsq(A[:, free], rhs, rcond=None)[0]
        if np.all(x >= lo) and np.all(x <= hi):
            r = A @ x - b
            best = min(best, float(r @ r))
    return best
