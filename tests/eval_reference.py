"""What tests/test_gpu_eval.py compares Eval / CalculateJac with: a generator of dyadic problems whose rows are exact in fp32, the
numpy row functions of the bodies used there, and the texts of those bodies."""
from fractions import Fraction

import numpy as np

import num_diff_reference as nd

H6 = 2.0 ** -6   # the dyadic step of the exact numeric cases

# (n, kR, items) of the exact cases, and what each can get wrong
SHAPES = [
    (1, 1, 1),      # the smallest
    (3, 1, 7),      # fp32 problem stride 84 B: problems 1 and 2 start 4 and 8 bytes off a 16-byte boundary
    (3, 3, 70),     # several rows per item, a partial last super-step
    (13, 1, 70),    # two Jet chunks
    (16, 1, 65),    # a tail of one item
    (50, 1, 130),   # the C4 width, three super-steps
    (63, 8, 9),     # the widest row, eight rows per item
]
# mode -> (JitResidual keywords, the + x[0]^2 variant?)
MODES = {
    "accumulate": (dict(kind="accumulate"), False),
    "residual": (dict(kind="residual"), False),
    "central": (dict(kind="residual", diff="central", diff_h=H6), False),
    "fast_central": (dict(kind="residual", diff="fast_central", diff_h=H6), False),
    "forward": (dict(kind="residual", diff="forward", diff_h=H6), True),
    "residual_sq": (dict(kind="residual"), True),
    # n = 3 only: Euclidean parameters written as the user's container, x (+) d = x + d — AD through the table of Jets of x (+) d
    "user_manifold": (dict(kind="residual", manifold="user", plus_body="for (int i = 0; i < 3; ++i) xp[i] = x[i] + d[i];", x_scalars=3), False),
}


def linear_body(n, kR, kind, squared=False):
    """r_q = sum_j p[q (n + 1) + j] x[j] - p[q (n + 1) + n]  (+ x[0]^2), as residual text or with its own Jacobian rows."""
    s = f"for (int q = 0; q < {kR}; ++q) {{ S z = S(0); for (int j = 0; j < {n}; ++j) z += p[q * {n + 1} + j] * x[j]; r[q] = z - p[q * {n + 1} + {n}]"
    s += " + x[0] * x[0]; }" if squared else "; }"
    if kind == "accumulate":
        s += f"\nif (want_grad) {{ for (int q = 0; q < {kR}; ++q) {{ for (int j = 0; j < {n}; ++j) J[q][j] = p[q * {n + 1} + j]; "
        s += "J[q][0] += T(2) * x[0]; } }" if squared else "} }"
    return s


def dyadic_case(n, kR, items, P=3, seed=None):
    """data [P, items, kR (n + 1)] in [-2, 2] and x [P, n] in [-1, 1] (beyond 16 parameters [-1/2, 1/2]), all multiples of 1/8."""
    rng = np.random.default_rng(1000 * n + 10 * kR + items if seed is None else seed)
    xm = 8 if n <= 16 else 4
    data = rng.integers(-16, 17, (P, items, kR * (n + 1))) / 8.0
    x = rng.integers(-xm, xm + 1, (P, n)) / 8.0
    return data, x


def linear_rows(data, x, n, dtype=np.float64, squared=False, forward_h=None):
    """(r [P, m], J [P, m, n]) of the linear body, every operation in `dtype`, the sums in index order.  forward_h: the Jacobian
    that forward differences with that step read off the squared variant (column 0: 2 x0 + h)."""
    P = data.shape[0]
    d = data.reshape(P, -1, n + 1).astype(dtype)
    xx = x.astype(dtype)
    r = np.zeros(d.shape[:2], dtype)
    for j in range(n):
        r = r + d[:, :, j] * xx[:, j, None]
    r = r - d[:, :, n]
    J = d[:, :, :n].copy()
    if squared:
        r = r + (xx[:, 0] * xx[:, 0])[:, None]
        J[:, :, 0] = J[:, :, 0] + (dtype(2) * xx[:, 0])[:, None]
        if forward_h is not None:
            J[:, :, 0] = J[:, :, 0] + dtype(forward_h)
    return r, J


def linear_rows_exact(data, x, n, squared=False, forward_h=None):
    """The same in exact rational arithmetic (object arrays of Fractions) and the largest partial-sum magnitude met, in units of the
    finest grain that occurs (2^-12: h^2 of the forward differences)."""
    P = data.shape[0]
    F = np.vectorize(lambda v: Fraction(v), otypes=[object])
    d, xx = F(data.reshape(P, -1, n + 1)), F(x)
    r = np.full(d.shape[:2], Fraction(0), dtype=object)
    big = Fraction(0)
    for j in range(n):
        r = r + d[:, :, j] * xx[:, j, None]
        big = max(big, np.abs(r).max())
    r = r - d[:, :, n]
    J = d[:, :, :n].copy()
    if squared:
        r = r + (xx[:, 0] * xx[:, 0])[:, None]
        J[:, :, 0] = J[:, :, 0] + (2 * xx[:, 0])[:, None]
        if forward_h is not None:
            J[:, :, 0] = J[:, :, 0] + Fraction(forward_h)
    big = max(big, np.abs(r).max(), np.abs(J).max())
    # a perturbed evaluation adds at most h |p_j| <= 2 h (and, squared, 2 |x0| h + h^2) to a partial sum
    return r, J, float(big + 1) * 4096


def numeric_rows(data, x, n, dtype, method, squared):
    """NumEval (num_diff_reference.num_eval) of the linear body in `dtype`, problem by problem."""
    P = data.shape[0]
    rs, Js = [], []
    for p in range(P):
        d = data[p].reshape(-1, n + 1).astype(dtype)

        def f(v, d=d):
            r = np.zeros(d.shape[0], dtype)
            for j in range(n):
                r = r + d[:, j] * v[j]
            r = r - d[:, n]
            return r + v[0] * v[0] if squared else r
        r, J = nd.num_eval(f, x[p].astype(dtype), method, dtype(H6), dtype)
        rs.append(r)
        Js.append(J)
    return np.stack(rs), np.stack(Js)


def as_dtype(a, dtype):
    return np.array(a, dtype=object).astype(np.float64).astype(dtype)


# ---- the DenseRow residual a.x + 0.1 sin(a.x) - b ---------------------------------------------------------------------------------
def dense_row_body(n, kind):
    if kind == "residual":
        return f"S t = x[0] * p[0];\n#pragma unroll 2\nfor (int j = 1; j < {n}; ++j) t = t + x[j] * p[j];\nr[0] = t + T(0.1) * sin(t) - p[{n}];"
    return (f"T t = x[0] * p[0];\nfor (int j = 1; j < {n}; ++j) t += x[j] * p[j];\nr[0] = t + T(0.1) * sin(t) - p[{n}];\n"
            f"if (want_grad) {{ const T sc = T(1) + T(0.1) * cos(t); for (int j = 0; j < {n}; ++j) J[0][j] = sc * p[j]; }}")


def dense_row_rows(data, x):
    """float64 (r [P, m], J [P, m, n]) for data [P, m, n + 1] = [a | b]."""
    a, b = data[:, :, :-1].astype(np.float64), data[:, :, -1].astype(np.float64)
    t = np.einsum("pmj,pj->pm", a, x.astype(np.float64))
    return t + 0.1 * np.sin(t) - b, (1.0 + 0.1 * np.cos(t))[:, :, None] * a
