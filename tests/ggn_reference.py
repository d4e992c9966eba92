"""The yardstick of the rank-one second-order scalar costs (kind="cost_ggn"): the kind's callbacks in numpy —
per item a cost term c, a scalar gs = dc/du, a curvature weight hs and a direction J = grad u; the problem's gradient is sum gs J and
its Hessian sum w J J^T with w = hs clamped from below at wmin (a NaN stays), in the problem's dtype — handed to the committed second
reading of the LM loop through bounds_reference.optimize_plain, the way hess_reference.py does it.  Nothing here reads the loop again.
Beside every callback stands the device body that states the same function as text.  Needs numpy only.
"""
import math

import numpy as np

import bounds_reference as br
import hess_reference as hr

ref = br.ref
WMIN = {np.dtype(np.float32): 2.0 ** -60, np.dtype(np.float64): 2.0 ** -200}


def weight(hs, dtype, wmin_of=None):
    """w = hs where hs > wmin, wmin where hs <= wmin, NaN where hs is NaN; wmin_of: the dtype whose wmin applies (default: dtype's own)"""
    wmin = np.dtype(dtype).type(WMIN[np.dtype(wmin_of or dtype)])
    return np.where(hs <= wmin, wmin, hs).astype(dtype)


# ---- the items' parts at x: parts(x, data, want) -> (c [items], gs [items], hs [items], J [items, n]); gs, hs, J None unless want ------
def logistic_parts(x, data, want):
    """c = log(1 + exp(-y z)), u = z = a . x; item = features (n), label y = +-1"""
    n = len(x)
    a, y = data[:, :n], data[:, n]
    z = a @ x
    e = np.exp(-y * z)
    s = 1.0 / (1.0 + e)
    if not want:
        return np.log(1.0 + e), None, None, None
    return np.log(1.0 + e), -y * (1.0 - s), s * (1.0 - s), a


def poisson_parts(x, data, want):
    """Poisson regression with the log link: c = exp(z) - k z, u = z = a . x; item = features (n), count k"""
    n = len(x)
    a, k = data[:, :n], data[:, n]
    mu = np.exp(a @ x)
    c = mu - k * (a @ x)
    if not want:
        return c, None, None, None
    return c, mu - k, mu, a


def spot_parts(x, data, want):
    """The Poisson deviance of a Gaussian spot (hess_reference.spot_term): u = mu(x) = b + A exp(-((u - x0)^2 + (v - y0)^2) / (2 sigma^2)),
    c = mu - k + k log(k / mu), gs = 1 - k / mu, hs = k / mu^2, J = grad mu.  u is NOT linear in x: the (1 - k / mu) Hess(mu) term of
    the full Hessian is dropped (hess_reference keeps it)."""
    A, x0, y0, b = x
    u, v, k = data[:, 0], data[:, 1], data[:, 2]
    is2 = x.dtype.type(1.0) / (x.dtype.type(hr.SPOT_SIGMA) * x.dtype.type(hr.SPOT_SIGMA))
    du, dv = u - x0, v - y0
    E = np.exp(x.dtype.type(-0.5) * (du * du + dv * dv) * is2)
    mu = b + A * E
    kk = np.where(k > 0, k, 1.0).astype(x.dtype)
    c = (mu - k) + np.where(k > 0, k * np.log(kk / mu), 0.0).astype(x.dtype)
    if not want:
        return c, None, None, None
    J = np.stack([E, A * E * du * is2, A * E * dv * is2, np.ones_like(E)], axis=1)
    return c, 1.0 - k / mu, k / (mu * mu), J


def quadratic_parts(x, data, want):
    """c = hs (a . x - b)^2 / 2, u = a . x - b; item = a (n), b, hs"""
    n = len(x)
    a, b, hs = data[:, :n], data[:, n], data[:, n + 1]
    r = a @ x - b
    c = 0.5 * hs * r * r
    if not want:
        return c, None, None, None
    return c, hs * r, hs, a


def table_parts(x, data, want):
    """The exact-sum body: nothing depends on x — item = (J (n), c, gs, hs)"""
    n = len(x)
    if not want:
        return data[:, n], None, None, None
    return data[:, n], data[:, n + 1], data[:, n + 2], data[:, :n]


def sums(parts, x, data, dtype, want=True, wmin_of=None):
    """(cost, g [n], H [n, n]) of one problem in `dtype`: sum c, sum gs J, sum w J J^T (numpy's own summation order)."""
    x, data = np.asarray(x, dtype), np.asarray(data, dtype)
    c, gs, hs, J = parts(x, data, want)
    cost = c.astype(dtype).sum(dtype=dtype)
    if not want:
        return cost, None, None
    w = weight(hs.astype(dtype), dtype, wmin_of)
    g = (gs.astype(dtype)[:, None] * J).sum(axis=0, dtype=dtype)
    H = np.einsum("i,ia,ib->ab", w, J.astype(dtype), J.astype(dtype)).astype(dtype)
    H = np.triu(H) + np.triu(H, 1).T   # (the upper triangle, mirrored: bit-symmetric like the device's Gram)
    return cost, g, H


def item_sum(parts, data, dtype=np.float64):
    """The callback fn(x, want) -> (cost, g, H, nres) of the loop, as ONE residual (Cost(Scalar), cost.h:22)."""
    data = np.asarray(data, dtype)

    def fn(x, want):
        c, g, H = sums(parts, x, data, dtype, want)
        return float(c), (g.astype(np.float64).tolist() if want else None), (H.astype(np.float64).tolist() if want else None), 1
    return fn


def optimize(parts, data, x0, opt, dtype=np.float64):
    return br.optimize_plain(item_sum(parts, data, dtype), [float(v) for v in x0], opt)


# ---- the same functions as device text (kind="cost_ggn"): c, and inside `if (want_grad)`: gs, hs, J[a] = for every a < n --------------
def logistic_body(n, flip=False):
    """The issue's logistic body for n parameters; flip: gs has the wrong sign (CheckGradient)."""
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j];\n"
            f"const T y = p[{n}], e = exp(-y * z), s = T(1) / (T(1) + e);\n"
            "c = log(T(1) + e);\n"
            f"if (want_grad) {{ gs = {'y' if flip else '-y'} * (T(1) - s); hs = s * (T(1) - s); for (int a = 0; a < {n}; ++a) J[a] = p[a]; }}\n")


def poisson_body(n):
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j];\n"
            f"const T k = p[{n}], mu = exp(z);\n"
            "c = mu - k * z;\n"
            f"if (want_grad) {{ gs = mu - k; hs = mu; for (int a = 0; a < {n}; ++a) J[a] = p[a]; }}\n")


SPOT_BODY = """
const T A = x[0], b = x[3], is2 = T(1.0) / (T(1.5) * T(1.5));
const T du = p[0] - x[1], dv = p[1] - x[2], k = p[2];
const T E = exp(T(-0.5) * (du * du + dv * dv) * is2);
const T mu = b + A * E;
c = (mu - k) + (k > T(0) ? k * log(k / mu) : T(0));
if (want_grad) {
  gs = T(1.0) - k / mu;
  hs = k / (mu * mu);
  J[0] = E; J[1] = A * E * du * is2; J[2] = A * E * dv * is2; J[3] = T(1.0);
}
"""


def quadratic_body(n):
    return (f"T r = -p[{n}]; for (int j = 0; j < {n}; ++j) r += p[j] * x[j];\n"
            f"c = T(0.5) * p[{n + 1}] * r * r;\n"
            f"if (want_grad) {{ gs = p[{n + 1}] * r; hs = p[{n + 1}]; for (int a = 0; a < {n}; ++a) J[a] = p[a]; }}\n")


def table_body(n):
    return (f"c = p[{n}];\n"
            f"if (want_grad) {{ gs = p[{n + 1}]; hs = p[{n + 2}]; for (int a = 0; a < {n}; ++a) J[a] = p[a]; }}\n")


# ---- seeded problems -----------------------------------------------------------------------------------------------------------------
logistic_case = hr.logistic_case
spot_case = hr.spot_case


def poisson_case(seed, n, items):
    rng = np.random.default_rng(9500 + seed)
    X = rng.normal(size=(items, n)) / math.sqrt(n)
    w = rng.normal(size=n)
    k = rng.poisson(np.exp(X @ w + 1.0)).astype(np.float64)
    return np.concatenate([X, k[:, None]], axis=1), rng.normal(size=n) * 0.3


def exact_case(n, items, P, seed=0):
    """Items (J (n), c, gs, hs) whose sums are exact in float32 in ANY order: J in {-2 .. 2} / 2, gs in {-8 .. 8} / 4, c in {-64 .. 64} / 8 and,
    per PROBLEM, one of three curvature regimes — hs a power of four in {1/16, 1/4, 1, 4} (problems 0, 3, 6, ...), hs = 0 (1, 4, ...) and
    hs in {-1, -4} (2, 5, ...): the last two contribute wmin J J^T to H, a power of two times multiples of 1/4, exact as well.  With at
    most 8192 items: |sum c| <= 2^16 in steps of 2^-3 (19 bits), |sum gs J| <= 2^14 in steps of 2^-3 (17 bits), |sum w J J^T| <= 2^15 in
    steps of 2^-6 (21 bits) — all below float32's 24."""
    assert items <= 8192
    rng = np.random.default_rng(1000 * n + items + seed)
    d = np.zeros((P, items, n + 3))
    d[:, :, :n] = rng.integers(-2, 3, (P, items, n)) / 2.0
    d[:, :, n] = rng.integers(-64, 65, (P, items)) / 8.0
    d[:, :, n + 1] = rng.integers(-8, 9, (P, items)) / 4.0
    for p in range(P):
        if p % 3 == 0:
            d[p, :, n + 2] = 4.0 ** rng.integers(-2, 2, items)
        elif p % 3 == 2:
            d[p, :, n + 2] = -(4.0 ** rng.integers(0, 2, items))
    return d


def exact_sums(d, dtype, wmin_of=None):
    """(cost [P], g [P, n], H [P, n, n]) of exact_case's data summed in `dtype`, with the wmin of `wmin_of` (default: dtype's own)"""
    P, n = d.shape[0], d.shape[2] - 3
    out = [sums(table_parts, np.zeros(n), d[p], dtype, True, wmin_of) for p in range(P)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


# ---- geometry: items per super-step of the model's passes (csrc/row_model.hpp RowStageGeom::make, restated) -----------------------------
def _stride16(elems, sz):
    q = (elems * sz + 15) // 16
    if not q & 1:
        q += 1
    return q * 16 // sz


def row_stage_items(n, item_scalars, dtype):
    """(items per super-step of the accumulate pass, ... of the cost-only pass) of a kind="cost_ggn" model: one residual per item, two
    ring regions, two workgroups per compute unit, one region for the accumulate pass."""
    sz = np.dtype(dtype).itemsize
    rem = n & 15
    thin = n >= 16 and rem + 1 <= 4
    nbm = (n >> 4) if thin else (n + 16) // 16
    rs = 16 * nbm + rem + 1 if thin else nbm * ((n + nbm) // nbm)
    rsp, ps = _stride16(rs, sz), (_stride16(item_scalars, sz) if item_scalars > 0 else 0)
    bud = 160 * 1024 // 8 - 320 * sz - 512

    def region(it):
        return max(it * ps * sz, ((it + 3) & ~3) * rsp * sz)

    def fit(nbuf):
        it = 64
        while it > 1 and nbuf * region(it) > bud:
            it = it - 4 if it > 4 else it >> 1
        return it
    return fit(1), fit(2)


options_pair = hr.options_pair
