"""The yardstick of the second-order scalar costs (kind="cost_hess"): the cost callbacks f(x, grad, H) in plain
Python floats, summed over items in item order, handed to the committed second reading of the LM loop through
bounds_reference.optimize_plain.  Nothing here reads the loop again.  Beside every callback stands the device body that states the
same function as text, so that a test compares two statements of one formula.  Needs numpy only.
"""
import math

import numpy as np

import bounds_reference as br

ref = br.ref


# ---- one item's term: fn(x, p, want) -> (c, g, H) with g, H None unless want; H is the full symmetric matrix -------------------
def rosenbrock_term(x, p, want):          # tests/optimize_easy.cpp:35-79
    t1, t2 = 1.0 - x[0], x[1] - x[0] * x[0]
    g = H = None
    if want:
        g = [-2.0 * t1 - 400.0 * x[0] * t2, 200.0 * t2]
        h01 = -400.0 * x[0]
        H = [[2.0 - 400.0 * x[1] + 1200.0 * x[0] * x[0], h01], [h01, 200.0]]
    return t1 * t1 + 100.0 * t2 * t2, g, H


def plateau_term(x, p, want):             # tests/optimize_easy.cpp:88-144
    PI = math.acos(-1.0)
    dx, dy = x[0] - PI, x[1] - PI
    ex = math.exp(-(dx * dx + dy * dy))
    cx, cy, sx, sy = math.cos(x[0]), math.cos(x[1]), math.sin(x[0]), math.sin(x[1])
    g = H = None
    if want:
        g = [cy * ex * (sx + 2.0 * dx * cx), cx * ex * (sy + 2.0 * dy * cy)]
        h01 = ex * (sx + 2.0 * dx * cx) * (sy + 2.0 * dy * cy)
        H = [[cy * ex * (cx - 4.0 * dx * sx + (2.0 - 4.0 * dx * dx) * cx), h01],
             [h01, cx * ex * (cy - 4.0 * dy * sy + (2.0 - 4.0 * dy * dy) * cy)]]
    return 1.0 - (cx * cy * ex), g, H


def powell_term(x, p, want):              # tests/optimize_easy.cpp:153-221
    t1, t2, t3, t4 = x[0] + 10.0 * x[1], x[2] - x[3], x[1] - 2.0 * x[2], x[0] - x[3]
    g = H = None
    if want:
        c3, c4 = t3 * t3 * t3, t4 * t4 * t4
        g = [2.0 * t1 + 40.0 * c4, 20.0 * t1 + 4.0 * c3, 10.0 * t2 - 8.0 * c3, -10.0 * t2 - 40.0 * c4]
        d3, d4 = 12.0 * t3 * t3, 120.0 * t4 * t4
        H = [[2.0 + d4, 20.0, 0.0, -d4], [20.0, 200.0 + d3, -2.0 * d3, 0.0], [0.0, -2.0 * d3, 10.0 + 4.0 * d3, -10.0], [-d4, 0.0, -10.0, 10.0 + d4]]
    return t1 * t1 + 5.0 * t2 * t2 + (t3 * t3) * (t3 * t3) + (t4 * t4) * (t4 * t4) * 10.0, g, H


def quadratic_term(x, p, want):           # c = (a . x - b)^2 / 2, item = a (n), b
    n = len(x)
    r = -p[n]
    for j in range(n):
        r += p[j] * x[j]
    g = H = None
    if want:
        g = [r * p[a] for a in range(n)]
        H = [[p[a] * p[b] for b in range(n)] for a in range(n)]
    return 0.5 * r * r, g, H


def logistic_term(x, p, want):            # c = log(1 + exp(-y z)), z = w . x, item = features (n), label y = +-1
    n = len(x)
    z = 0.0
    for j in range(n):
        z += p[j] * x[j]
    y = p[n]
    e = math.exp(-y * z)
    s = 1.0 / (1.0 + e)
    g = H = None
    if want:
        gz, hz = -y * (1.0 - s), s * (1.0 - s)
        g = [gz * p[a] for a in range(n)]
        H = [[hz * p[a] * p[b] for b in range(n)] for a in range(n)]
    return math.log(1.0 + e), g, H


SPOT_SIGMA = 1.5


def spot_term(x, p, want):
    """Poisson likelihood of a Gaussian spot: mu = b + A exp(-((u - x0)^2 + (v - y0)^2) / (2 sigma^2)), c = mu - k + k log(k / mu) —
    the negative log-likelihood less its value at mu = k, so that every term is >= 0 and min_error sees a cost, not a sign;
    x = (A, x0, y0, b), item = (u, v, k).  H = (1 - k / mu) Hess(mu) + (k / mu^2) grad(mu) grad(mu)^T: not a Gram, and indefinite
    away from the optimum."""
    A, x0, y0, b = x
    u, v, k = p
    is2 = 1.0 / (SPOT_SIGMA * SPOT_SIGMA)
    du, dv = u - x0, v - y0
    E = math.exp(-0.5 * (du * du + dv * dv) * is2)
    mu = b + A * E
    g = H = None
    if want:
        m = [E, A * E * du * is2, A * E * dv * is2, 1.0]
        w1, w2 = 1.0 - k / mu, k / (mu * mu)
        M = [[0.0] * 4 for _ in range(4)]
        M[0][1] = E * du * is2
        M[0][2] = E * dv * is2
        M[1][1] = A * E * (du * du * is2 * is2 - is2)
        M[1][2] = A * E * du * dv * is2 * is2
        M[2][2] = A * E * (dv * dv * is2 * is2 - is2)
        g = [w1 * m[a] for a in range(4)]
        H = [[w1 * M[min(a, c)][max(a, c)] + w2 * m[a] * m[c] for c in range(4)] for a in range(4)]
    return (mu - k) + (k * math.log(k / mu) if k > 0.0 else 0.0), g, H


def saddle_term(x, p, want):              # c = x^4 / 4 - x^2 / 2 + y^2 + 1: a saddle at the origin, minima (3 / 4) at (+-1, 0)
    g = H = None
    if want:
        g = [x[0] * x[0] * x[0] - x[0], 2.0 * x[1]]
        H = [[3.0 * x[0] * x[0] - 1.0, 0.0], [0.0, 2.0]]
    return 0.25 * (x[0] * x[0]) * (x[0] * x[0]) - 0.5 * x[0] * x[0] + x[1] * x[1] + 1.0, g, H


def item_sum(term, items):
    """The callback fn(x, want) -> (cost, g, H, nres) of the loop: the terms of `items` ([items][scalars]) summed in item order, as ONE
    residual (Cost(Scalar), cost.h:22)."""
    items = [[float(v) for v in p] for p in items]

    def fn(x, want):
        n = len(x)
        c = 0.0
        g = [0.0] * n if want else None
        H = [[0.0] * n for _ in range(n)] if want else None
        for p in items:
            ci, gi, Hi = term(x, p, want)
            c += ci
            if want:
                for a in range(n):
                    g[a] += gi[a]
                    for b in range(a, n):   # (the upper triangle, as the device sums it; mirrored below)
                        H[a][b] += Hi[a][b]
        if want:
            for a in range(n):
                for b in range(a):
                    H[a][b] = H[b][a]
        return c, g, H, 1
    return fn


def optimize(term, items, x0, opt):
    return br.optimize_plain(item_sum(term, items), [float(v) for v in x0], opt)


# ---- the same functions as device text (kind="cost_hess"): c, G[a] +=, H(a, b) += for a <= b ---------------------------------------
# (The reference's three test functions are held to the C oracle at 1e-9 down to costs of 1e-14, where t2 = y - x^2 is all cancellation:
#  their text switches floating-point contraction off, so that it rounds as the oracle's CPU build does — a fused y - x * x differs in
#  the eighth digit there.  What a user who wants a CPU run's digits writes too.)
ROSENBROCK_BODY = """
{
#pragma clang fp contract(off)
const T t1 = T(1.0) - x[0], t2 = x[1] - x[0] * x[0];
c = t1 * t1 + T(100.0) * t2 * t2;
if (want_grad) {
  G[0] += T(-2.0) * t1 - T(400.0) * x[0] * t2;
  G[1] += T(200.0) * t2;
  H(0, 0) += T(2.0) - T(400.0) * x[1] + T(1200.0) * x[0] * x[0];
  H(0, 1) += T(-400.0) * x[0];
  H(1, 1) += T(200.0);
}
}
"""
PLATEAU_BODY = """
{
#pragma clang fp contract(off)
const T PI = T(3.14159265358979323846);
const T dx = x[0] - PI, dy = x[1] - PI;
const T ex = exp(-(dx * dx + dy * dy));
const T cx = cos(x[0]), cy = cos(x[1]), sx = sin(x[0]), sy = sin(x[1]);
c = T(1.0) - (cx * cy * ex);
if (want_grad) {
  G[0] += cy * ex * (sx + T(2.0) * dx * cx);
  G[1] += cx * ex * (sy + T(2.0) * dy * cy);
  H(0, 0) += cy * ex * (cx - T(4.0) * dx * sx + (T(2.0) - T(4.0) * dx * dx) * cx);
  H(1, 1) += cx * ex * (cy - T(4.0) * dy * sy + (T(2.0) - T(4.0) * dy * dy) * cy);
  const T h01 = ex * (sx + T(2.0) * dx * cx) * (sy + T(2.0) * dy * cy);
  H(0, 1) += h01;
  H(1, 0) += h01;   // (the lower triangle is discarded: a body may fill the full matrix)
}
}
"""
POWELL_BODY = """
{
#pragma clang fp contract(off)
const T t1 = x[0] + T(10.0) * x[1], t2 = x[2] - x[3], t3 = x[1] - T(2.0) * x[2], t4 = x[0] - x[3];
c = t1 * t1 + T(5.0) * t2 * t2 + (t3 * t3) * (t3 * t3) + (t4 * t4) * (t4 * t4) * T(10.0);
if (want_grad) {
  const T c3 = t3 * t3 * t3, c4 = t4 * t4 * t4;
  G[0] += T(2.0) * t1 + T(40.0) * c4;
  G[1] += T(20.0) * t1 + T(4.0) * c3;
  G[2] += T(10.0) * t2 - T(8.0) * c3;
  G[3] += T(-10.0) * t2 - T(40.0) * c4;
  const T d3 = T(12.0) * t3 * t3, d4 = T(120.0) * t4 * t4;
  H(0, 0) += T(2.0) + d4;  H(0, 1) += T(20.0);         H(0, 3) += -d4;
  H(1, 1) += T(200.0) + d3; H(1, 2) += T(-2.0) * d3;
  H(2, 2) += T(10.0) + T(4.0) * d3; H(2, 3) += T(-10.0);
  H(3, 3) += T(10.0) + d4;
}
}
"""
SADDLE_BODY = """
c = T(0.25) * (x[0] * x[0]) * (x[0] * x[0]) - T(0.5) * x[0] * x[0] + x[1] * x[1] + T(1.0);
if (want_grad) {
  G[0] += x[0] * x[0] * x[0] - x[0];
  G[1] += T(2.0) * x[1];
  H(0, 0) += T(3.0) * x[0] * x[0] - T(1.0);
  H(1, 1) += T(2.0);
}
"""
SPOT_BODY = """
const T A = x[0], b = x[3], is2 = T(1.0) / (T(1.5) * T(1.5));
const T du = p[0] - x[1], dv = p[1] - x[2], k = p[2];
const T E = exp(T(-0.5) * (du * du + dv * dv) * is2);
const T mu = b + A * E;
c = (mu - k) + (k > T(0) ? k * log(k / mu) : T(0));
if (want_grad) {
  const T m[4] = {E, A * E * du * is2, A * E * dv * is2, T(1.0)};
  const T w1 = T(1.0) - k / mu, w2 = k / (mu * mu);
  T M[4][4] = {};
  M[0][1] = E * du * is2;
  M[0][2] = E * dv * is2;
  M[1][1] = A * E * (du * du * is2 * is2 - is2);
  M[1][2] = A * E * du * dv * is2 * is2;
  M[2][2] = A * E * (dv * dv * is2 * is2 - is2);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    G[a] += w1 * m[a];
#pragma unroll
    for (int q = a; q < 4; ++q) H(a, q) += w1 * M[a][q] + w2 * m[a] * m[q];
  }
}
"""


def quadratic_body(n):
    return (f"T r = -p[{n}]; for (int j = 0; j < {n}; ++j) r += p[j] * x[j];\n"
            "c = T(0.5) * r * r;\n"
            "if (want_grad) {\n"
            f"  for (int a = 0; a < {n}; ++a) {{ G[a] += r * p[a]; for (int q = a; q < {n}; ++q) H(a, q) += p[a] * p[q]; }}\n"
            "}\n")


def logistic_body(n, flip=None):
    """DESIGN section 18's logistic body for n parameters; flip = (a, b): the sign of that one Hessian entry is wrong (CheckGradient)."""
    s = (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j];\n"
         f"const T y = p[{n}], e = exp(-y * z), s = T(1) / (T(1) + e);\n"
         "c = log(T(1) + e);\n"
         "if (want_grad) {\n"
         "  const T gz = -y * (T(1) - s), hz = s * (T(1) - s);\n"
         f"  for (int a = 0; a < {n}; ++a) {{ G[a] += gz * p[a]; for (int q = a; q < {n}; ++q) H(a, q) += hz * p[a] * p[q]; }}\n")
    if flip is not None:
        s += f"  H({flip[0]}, {flip[1]}) -= T(2) * hz * p[{flip[0]}] * p[{flip[1]}];\n"
    return s + "}\n"


# ---- seeded problems -----------------------------------------------------------------------------------------------------------------
def logistic_case(seed, n, items):
    """Noisy, non-separable labels from a planted weight vector: (data [items, n + 1], x0 [n])."""
    rng = np.random.default_rng(9100 + seed)
    X = rng.normal(size=(items, n)) / math.sqrt(n)
    w = rng.normal(size=n) * 2.0
    y = np.where(rng.uniform(size=items) < 1.0 / (1.0 + np.exp(-(X @ w))), 1.0, -1.0)
    return np.concatenate([X, y[:, None]], axis=1), rng.normal(size=n) * 0.3


def spot_case(seed, side=7):
    """A side x side window of Poisson counts around a spot: (data [side^2, 3], x0 [4])."""
    rng = np.random.default_rng(9300 + seed)
    A, x0, y0, b = rng.uniform(60.0, 120.0), rng.uniform(2.4, 3.6), rng.uniform(2.4, 3.6), rng.uniform(3.0, 8.0)
    u, v = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64), indexing="ij")
    mu = b + A * np.exp(-0.5 * ((u - x0) ** 2 + (v - y0) ** 2) / SPOT_SIGMA ** 2)
    k = rng.poisson(mu).astype(np.float64)
    data = np.stack([u.ravel(), v.ravel(), k.ravel()], axis=1)
    start = np.array([A * rng.uniform(0.7, 1.3), x0 + rng.uniform(-0.5, 0.5), y0 + rng.uniform(-0.5, 0.5), b * rng.uniform(0.6, 1.4)])
    return data, start


def options_pair(ta_options_cls=None, base=None, **kw):
    """The same options for the device (tinyopt_amd.Options; None where only the second reading's half is wanted) and for the second
    reading: `solver` "lm" / "gn", `damping_init`, `use_ldlt` and the flat fields by the second reading's names.
    base = "benchmark": Options.benchmark() (benchmarks/options.h:10-27)."""
    rkw = dict(max_iters=10, min_error=0.0, min_rerr_dec=1e-12, min_step_norm2=1e-16, max_consec_failures=3) if base == "benchmark" else {}
    rkw.update(kw)
    ropt = ref.Options(**rkw)
    if ta_options_cls is None:
        return None, ropt
    o = ta_options_cls.benchmark() if base == "benchmark" else ta_options_cls()
    for k, v in kw.items():
        if k == "solver":
            o.solver_type = {"lm": 0, "gn": 1}[v]
        elif k == "damping_init":
            o.lm.damping_init = v
        elif k == "use_ldlt":
            o.hessian.use_ldlt = v
        else:
            assert hasattr(o, k), k
            setattr(o, k, v)
    return o, ropt
