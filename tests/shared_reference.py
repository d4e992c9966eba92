"""Yardsticks of shared item tables (JitResidual(..., shared_scalars=kS)), shared by tests/test_cpu_shared.py and
tests/test_gpu_shared.py.  Needs numpy only.

  * the numpy restatement of RowStageGeom::make (csrc/row_stage_geom.hpp) with kS — ggn_reference.row_stage_items, extended;
  * device bodies that read `s[k]`, and `replicate`, which rewrites such a text into its REPLICATED twin: s[k] -> p[kD + k], to be
    bound to data in which the table is copied behind every problem's own item scalars (a path the library had before tables);
  * the exact-sum case: dyadic private scalars and table rows, every table row different from every other, and the sums in numpy.
"""
import re

import numpy as np

import ggn_reference as gr


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def _stride16(elems, sz):
    q = (elems * sz + 15) // 16
    if not q & 1:
        q += 1
    return q * 16 // sz


def row_stage_geom(sz, n, kR, kD, kS=0, compute_bound=True, nbuf=2, waves=2, extra=0):
    """RowStageGeom::make, field by field: a region holds the private raw image (it * ps), behind it the shared one (it * pss), and the
    [J | r] image over both; region() is the larger of the raw total and the image."""
    rem = n & 15
    thin = n >= 16 and rem + 1 <= 4
    nbm = (n >> 4) if thin else (n + 16) // 16
    rs = 16 * nbm + rem + 1 if thin else nbm * ((n + nbm) // nbm)
    rsp = _stride16(rs, sz)
    ps = _stride16(kD, sz) if kD > 0 else 0
    pss = _stride16(kS, sz) if kS > 0 else 0
    bud = 160 * 1024 // (4 * waves) - 320 * sz - 512 - extra

    def region(it):
        return max(it * (ps + pss) * sz, ((it * kR + 3) & ~3) * rsp * sz)

    def fit(regions):
        it = 64 // kR
        if it >= 4:
            it &= ~3
        while it > 1 and regions * region(it) > bud:
            it = it - 4 if it > 4 else it >> 1
        return it
    items2 = fit(nbuf)
    nbytes = nbuf * region(items2)
    items1 = 0
    if compute_bound:
        items1 = fit(1)
        nbytes = max(nbytes, region(items1))
    nbytes = (nbytes + 15) & ~15
    return dict(items2=items2, nbuf=nbuf, items1=items1, ps=ps, pss=pss, rsp=rsp, bytes=nbytes + ((extra + 15) & ~15), table_off=nbytes)


def row_stage_items(n, kD, kS, dtype, kR=1):
    """(items per super-step of the accumulate pass, ... of the cost-only pass) of a run-time row model: one region for the accumulate
    pass (every functor, the library's default), two ring regions for the cost-only pass, two workgroups per compute unit."""
    g = row_stage_geom(np.dtype(dtype).itemsize, n, kR, kD, kS, True)
    return g["items1"], g["items2"]


def edge_counts(n, kD, kS, dtype, kR=1):
    """Item counts at the geometry's edges: {1, 63, 64, 65} and IT - 1, IT, IT + 1, 3 IT + 5 of both passes."""
    its = row_stage_items(n, kD, kS, dtype, kR)
    return sorted({1, 63, 64, 65} | {c for it in its for c in (it - 1, it, it + 1, 3 * it + 5) if c >= 1})


# ---- a shared body and its replicated twin --------------------------------------------------------------------------------------------
def replicate(body, kD):
    """The same text with every s[<index>] rewritten to p[kD + (<index>)]: the table's columns behind the item's own kD scalars."""
    return re.sub(r"\bs\[([^\]]+)\]", lambda m: f"p[{kD} + ({m.group(1)})]", body)


def replicated_data(data, table):
    """[P, items, kD + kS]: the table copied behind every problem's own item scalars."""
    P = data.shape[0]
    return np.concatenate([data, np.broadcast_to(table[None], (P,) + table.shape)], axis=2)


# ---- the exact-sum case ---------------------------------------------------------------------------------------------------------------
def _hash(a, b, c, salt):
    """A fixed pseudo-random value in {-2, -1, 0, 1, 2} / 2 for integer arrays a, b, c (broadcast)."""
    v = (a.astype(np.uint64) * np.uint64(2654435761) + b.astype(np.uint64) * np.uint64(40503) + c.astype(np.uint64) * np.uint64(2246822519) +
         np.uint64(salt) * np.uint64(3266489917))
    v ^= v >> np.uint64(15)
    v *= np.uint64(2246822519)
    v ^= v >> np.uint64(13)
    return ((v % np.uint64(5)).astype(np.int64) - 2) / 2.0


def exact_case(kD, kS, items, P):
    """(data [P, items, kD], table [items, kS]): dyadic, pseudo-random in (problem, item, column)."""
    p_, i_, j_ = np.meshgrid(np.arange(P), np.arange(items), np.arange(max(kD, 1)), indexing="ij")
    data = _hash(p_, i_, j_, 1)[:, :, :kD]
    i2, k2 = np.meshgrid(np.arange(items), np.arange(kS), indexing="ij")
    table = _hash(np.zeros_like(i2), i2, k2, 2)
    # the row's first column counts the item, in eighths: (i mod 61 - 30) / 8 — two rows less than 61 items apart differ whatever the
    # other columns hold, and a row read from the private image (halves) or from padding (zeros) is not the row that belongs there
    table[:, 0] = ((np.arange(items) % 61) - 30) / 8.0
    return data, table


def _columns(n, width):
    """For each parameter a: the columns of a `width`-wide row that its J entry sums — all of them are used when width >= n, column
    a mod width otherwise; none for width = 0."""
    if width == 0:
        return [[] for _ in range(n)]
    if width >= n:
        return [[k for k in range(width) if k % n == a] for a in range(n)]
    return [[a % width] for a in range(n)]


def exact_body(kind, n, kR, kD, kS):
    """kind "accumulate": J[0][a] = the sum of the table columns and private scalars that _columns deals to a, J[1][a] = -J[0][a],
    r[q] = u + q with u = p[0] (kD > 0) or s[0].  kind "cost_ggn": c = u, gs = s[kS - 1], hs = 1/4, J[a] the same sums.  Nothing
    depends on x: the sums are those of the data alone."""
    ks, kd = _columns(n, kS), _columns(n, kD)
    u = "p[0]" if kD > 0 else "s[0]"

    def jsum(a):
        return " + ".join([f"s[{k}]" for k in ks[a]] + [f"p[{j}]" for j in kd[a]])
    if kind == "cost_ggn":
        rows = " ".join(f"J[{a}] = {jsum(a)};" for a in range(n))
        return f"c = {u};\nif (want_grad) {{ gs = s[{kS - 1}]; hs = T(0.25); {rows} }}\n"
    rows = " ".join(f"J[0][{a}] = {jsum(a)};" for a in range(n))
    if kR == 2:
        rows += " " + " ".join(f"J[1][{a}] = -({jsum(a)});" for a in range(n))
    res = " ".join(f"r[{q}] = {u} + T({q});" for q in range(kR))
    return f"{res}\nif (want_grad) {{ {rows} }}\n"


def exact_sums(kind, n, kR, data, table, dtype, wmin_of=None):
    """(cost [P], g [P, n], H [P, n, n], sum of the magnitudes of the terms of the largest entry) of exact_body on (data, table), every
    product and sum taken in `dtype`."""
    P, items, kD = data.shape
    kS = table.shape[1]
    d, t = data.astype(dtype), table.astype(dtype)
    ks, kd = _columns(n, kS), _columns(n, kD)
    J0 = np.zeros((P, items, n), dtype)
    for a in range(n):
        for k in ks[a]:
            J0[:, :, a] += t[None, :, k]
        for j in kd[a]:
            J0[:, :, a] += d[:, :, j]
    u = d[:, :, 0] if kD > 0 else np.broadcast_to(t[None, :, 0], (P, items))
    if kind == "cost_ggn":
        gs = np.broadcast_to(t[None, :, kS - 1], (P, items)).astype(dtype)
        w = gr.weight(np.full((P, items), 0.25, dtype), dtype, wmin_of)
        cost = u.sum(axis=1, dtype=dtype)
        g = (gs[:, :, None] * J0).sum(axis=1, dtype=dtype)
        H = np.einsum("pi,pia,pib->pab", w, J0, J0).astype(dtype)
        # (every value is a multiple of 1/8: c in units of 1/8, gs J of 1/64, w J J^T of 1/256)
        big = max(np.abs(u).sum(axis=1).max() * 8, (np.abs(gs)[:, :, None] * np.abs(J0)).sum(axis=1).max() * 64, (0.25 * J0 * J0).sum(axis=1).max() * 256)
        return cost, g, H, float(big)
    J = np.stack([J0] + ([-J0] if kR == 2 else []), axis=2).reshape(P, items * kR, n)
    r = np.stack([u + dtype(q) for q in range(kR)], axis=2).reshape(P, items * kR).astype(dtype)
    cost = (r * r).sum(axis=1, dtype=dtype)
    g = (J * r[:, :, None]).sum(axis=1, dtype=dtype)
    H = np.einsum("pma,pmb->pab", J, J).astype(dtype)
    # (every value is a multiple of 1/8 — r of 1/8, J of 1/2 —, so every term is a multiple of 1/64)
    big = max((r * r).sum(axis=1).max(), (np.abs(J) * np.abs(r)[:, :, None]).sum(axis=1).max(), (J * J).sum(axis=1).max()) * 64
    return cost, g, H, float(big)


# ---- generalised linear models on a shared design matrix: the item's own scalar is p[0] (the label / the count), its features s[j] -----------
def logistic_body(n):
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += s[j] * x[j];\n"
            "const T y = p[0], e = exp(-y * z), sg = T(1) / (T(1) + e);\n"
            "c = log(T(1) + e);\n"
            f"if (want_grad) {{ gs = -y * (T(1) - sg); hs = sg * (T(1) - sg); for (int a = 0; a < {n}; ++a) J[a] = s[a]; }}\n")


def poisson_body(n):
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += s[j] * x[j];\n"
            "const T k = p[0], mu = exp(z);\n"
            "c = mu - k * z;\n"
            f"if (want_grad) {{ gs = mu - k; hs = mu; for (int a = 0; a < {n}; ++a) J[a] = s[a]; }}\n")


def linear_body(n, kind="residual"):
    """r = s . x - p[0]: kind "residual" over the scalar type S (Jets, or finite differences), "accumulate" with its own row."""
    if kind == "accumulate":
        return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += s[j] * x[j];\nr[0] = z - p[0];\n"
                f"if (want_grad) {{ for (int a = 0; a < {n}; ++a) J[0][a] = s[a]; }}\n")
    return f"S z = S(0); for (int j = 0; j < {n}; ++j) z += s[j] * x[j];\nr[0] = z - p[0];\n"


DECAY_ACC_BODY = ("const T E = exp(-x[1] * s[0]);\nr[0] = x[0] * E + x[2] - p[0];\n"
                  "if (want_grad) { J[0][0] = E; J[0][1] = -x[0] * s[0] * E; J[0][2] = T(1); }\n")   # ... with its own Jacobian row
DECAY_BODY = "r[0] = x[0] * exp(-x[1] * s[0]) + x[2] - p[0];\n"   # a curve fit per pixel over ONE time axis: s[0] = t_i, p[0] = the sample


def glm_batch(case, n, items, P):
    """`case` = ggn_reference.logistic_case / poisson_case: ONE design matrix (problem 0's) for all, the per-problem targets drawn by
    each seed's own generator on its own X (a label / count vector is as good against another X), and per-problem starts.
    Returns (X [items, n], y [P, items], x0 [P, n])."""
    cases = [case(seed, n, items) for seed in range(P)]
    return cases[0][0][:, :n].copy(), np.array([c[0][:, n] for c in cases]), np.array([c[1] for c in cases])


def glm_data(X, y):
    """ggn_reference's per-problem layout [features | target] of problem data sharing X: [P, items, n + 1]."""
    return np.concatenate([np.broadcast_to(X[None], (y.shape[0],) + X.shape), y[:, :, None]], axis=2)
