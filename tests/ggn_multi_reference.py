"""The yardstick of the multi-output second-order scalar costs (kind="cost_ggn_multi"): the kind's callbacks in
numpy — per item a cost term c, gs [K] = dc/du, the K x K curvature Hs (its LOWER triangle is read) and J [K, n] = du/dx — and the
row transform of csrc/ggn_multi_cost.hpp restated operation for operation in the problem's dtype: an unpivoted L D L^T of Hs with the
pivots clamped from below at wmin, y = L^-1 gs, row j of the [J | r] image = [sqrt(w_j) (J_j + sum_{i>j} L_ij J_i) | y_j / sqrt(w_j)].
The problem's gradient and Hessian are what the Gram of those rows holds, g = sum y_j C_j and H = sum w_j C_j C_j^T (C_j the combination).
All of it is handed to the committed second reading of the LM loop through bounds_reference.optimize_plain; nothing here reads the
loop again.  Beside every callback stands the device body that states the same function as text.  Needs numpy only.
"""
import numpy as np

import bounds_reference as br
import ggn_reference as gr
import hess_reference as hr

WMIN = gr.WMIN
options_pair = hr.options_pair


# ---- the rule (csrc/ggn_multi_cost.hpp), every operation rounded on its own in `dtype`, vectorised over the items ---------------------
def transform(gs, Hs, J, dtype, wmin_of=None, full=False):
    """gs [items, K], Hs [items, K, K] (lower triangle), J [items, K, n] -> (rows [items, K, n], r [items, K], w [items, K]);
    full: and the unscaled combinations J_j + sum_{i>j} L_ij J_i [items, K, n] and y = L^-1 gs [items, K]."""
    dtype = np.dtype(dtype).type
    gs, Hs, J = np.array(gs, dtype), np.array(Hs, dtype), np.array(J, dtype)
    items, K = gs.shape
    wmin = dtype(WMIN[np.dtype(wmin_of or dtype)])
    L = Hs.copy()
    e, sq, w = np.zeros((items, K), dtype), np.zeros((items, K), dtype), np.zeros((items, K), dtype)
    with np.errstate(all="ignore"):
        for j in range(K):
            d = L[:, j, j].copy()
            for q in range(j):
                d = d - L[:, j, q] * (L[:, j, q] * e[:, q])
            clamped = d <= wmin                      # (a NaN compares false: it stays)
            w[:, j] = np.where(clamped, wmin, d)
            e[:, j] = np.where(clamped, dtype(0), d)
            sq[:, j] = np.sqrt(w[:, j])
            for i in range(j + 1, K):
                t = L[:, i, j].copy()
                for q in range(j):
                    t = t - L[:, i, q] * (L[:, j, q] * e[:, q])
                L[:, i, j] = np.where(clamped, dtype(0), t / d)
        y, r = gs.copy(), np.zeros((items, K), dtype)
        for j in range(K):
            t = gs[:, j].copy()
            for q in range(j):
                t = t - L[:, j, q] * y[:, q]
            y[:, j] = t
            r[:, j] = t / sq[:, j]
        rows, comb = np.zeros_like(J), np.zeros_like(J)
        for j in range(K):
            t = J[:, j, :].copy()
            for i in range(j + 1, K):
                t = t + L[:, i, j][:, None] * J[:, i, :]
            comb[:, j, :] = t
            rows[:, j, :] = t * sq[:, j][:, None]
    if full:
        return rows, r, w, comb, y
    return rows, r, w


def sums(parts, x, data, dtype, want=True, wmin_of=None):
    """(cost, g [n], H [n, n]) of one problem in `dtype`: sum c, g = sum y_j C_j and H = sum w_j C_j C_j^T over the combinations
    C_j = J_j + sum_{i>j} L_ij J_i of the rule — what the Gram of the rows [sqrt(w_j) C_j | y_j / sqrt(w_j)] holds, written as
    ggn_reference.sums writes its K = 1 case (numpy's own summation order), so that K = 1 IS that function to the bit."""
    x, data = np.asarray(x, dtype), np.asarray(data, dtype)
    c, gs, Hs, J = parts(x, data, want)
    cost = c.astype(dtype).sum(dtype=dtype)
    if not want:
        return cost, None, None
    _, _, w, comb, y = transform(gs, Hs, J, dtype, wmin_of, full=True)
    n = comb.shape[2]
    with np.errstate(all="ignore"):
        g = (y.reshape(-1)[:, None] * comb.reshape(-1, n)).sum(axis=0, dtype=dtype)
        H = np.einsum("i,ia,ib->ab", w.reshape(-1), comb.reshape(-1, n), comb.reshape(-1, n)).astype(dtype)
    H = np.triu(H) + np.triu(H, 1).T   # (the upper triangle, mirrored: bit-symmetric like the device's Gram)
    return cost, g, H


def direct_sums(parts, x, data):
    """The same sums stated directly in float64: g = sum_k gs_k J_k, H = sum J^T Hs J with the symmetric Hs (no factorisation)."""
    x, data = np.asarray(x, np.float64), np.asarray(data, np.float64)
    c, gs, Hs, J = parts(x, data, True)
    S = np.tril(Hs) + np.transpose(np.tril(Hs, -1), (0, 2, 1))
    return c.sum(), np.einsum("ik,ika->a", gs, J), np.einsum("ika,ikl,ilb->ab", J, S, J)


def ridge(x, mu, W, dtype=np.float64):
    """The prior of the kind: (1/2 |W (x - mu)|^2, W^T r, W^T W); W [n] is the diagonal form, [k, n] the full one."""
    x, mu, W = np.asarray(x, dtype), np.asarray(mu, dtype), np.asarray(W, dtype)
    if W.ndim == 1:
        r = W * (x - mu)
        return 0.5 * (r * r).sum(), W * r, np.diag(W * W)
    r = W @ (x - mu)
    return 0.5 * (r * r).sum(), W.T @ r, W.T @ W


def item_sum(parts, data, dtype=np.float64, prior=None):
    """The callback fn(x, want) -> (cost, g, H, nres) of the loop, as ONE residual; prior = (mu, W) adds the ridge term."""
    data = np.asarray(data, dtype)

    def fn(x, want):
        c, g, H = sums(parts, x, data, dtype, want)
        c = float(c)
        if prior is not None:
            pc, pg, pH = ridge(x, prior[0], prior[1], dtype)
            c += float(pc)
            if want:
                g, H = g + pg, H + pH
        return c, (np.asarray(g, np.float64).tolist() if want else None), (np.asarray(H, np.float64).tolist() if want else None), 1
    return fn


def optimize(parts, data, x0, opt, dtype=np.float64, prior=None):
    return br.optimize_plain(item_sum(parts, data, dtype, prior), [float(v) for v in x0], opt)


# ---- the items' parts at x: parts(x, data, want) -> (c [items], gs [items, K], Hs [items, K, K], J [items, K, n]) ----------------------
def softmax_parts(K, d):
    """(K + 1)-class softmax regression with class 0 the reference class: u_k = a . x[k d : (k + 1) d] for the K free logits, the
    reference logit is 0; item = features a (d), the class y in 0 .. K.  c = log(1 + sum exp u_k) - u_y (u_0 = 0), computed stably."""
    def parts(x, data, want):
        a, y = data[:, :d], data[:, d]
        u = a @ x.reshape(K, d).T                                  # [items, K]
        mx = np.maximum(u.max(axis=1), 0.0)
        e = np.exp(u - mx[:, None])
        z = np.exp(-mx) + e.sum(axis=1)
        hit = (y[:, None] == np.arange(1, K + 1)[None, :]).astype(x.dtype)
        c = np.log(z) + mx - (hit * u).sum(axis=1)
        if not want:
            return c, None, None, None
        q = e / z[:, None]
        Hs = -q[:, :, None] * q[:, None, :]
        Hs[:, np.arange(K), np.arange(K)] = q * (1.0 - q)
        J = np.zeros((len(a), K, K * d), x.dtype)
        for k in range(K):
            J[:, k, k * d:(k + 1) * d] = a
        return c, q - hit, Hs, J
    return parts


def softmax_body(K, d, flip=False):
    """softmax_parts as text; flip: gs has the wrong sign (CheckGradient)."""
    n = K * d
    sign = "-" if flip else ""
    return "\n".join([
        f"T u[{K}];",
        f"for (int k = 0; k < {K}; ++k) {{ u[k] = T(0); for (int j = 0; j < {d}; ++j) u[k] += p[j] * x[k * {d} + j]; }}",
        f"T mx = T(0); for (int k = 0; k < {K}; ++k) mx = fmax(mx, u[k]);",
        f"T e[{K}]; T z = exp(-mx); for (int k = 0; k < {K}; ++k) {{ e[k] = exp(u[k] - mx); z += e[k]; }}",
        f"const T y = p[{d}]; T uy = T(0); for (int k = 0; k < {K}; ++k) uy = (y == T(k + 1)) ? u[k] : uy;",
        "c = log(z) + mx - uy;",
        "if (want_grad) {",
        f"  T q[{K}]; for (int k = 0; k < {K}; ++k) q[k] = e[k] / z;",
        f"  for (int k = 0; k < {K}; ++k) {{ gs[k] = {sign}(q[k] - ((y == T(k + 1)) ? T(1) : T(0)));",
        "    for (int l = 0; l <= k; ++l) Hs[k][l] = (k == l) ? q[k] * (T(1) - q[k]) : -q[k] * q[l]; }",
        f"  for (int k = 0; k < {K}; ++k) {{ for (int a = 0; a < {n}; ++a) J[k][a] = T(0); for (int j = 0; j < {d}; ++j) J[k][k * {d} + j] = p[j]; }}",
        "}"]) + "\n"


def softmax_full_hessian(K, d, x, data):
    """The full Hessian of the same cost stated on its own (u is linear in x, so the Gauss-Newton Hessian is exact):
    H[(k, i), (l, j)] = sum_items a_i a_j (q_k [k == l] - q_k q_l), and g[(k, i)] = sum_items a_i (q_k - [y == k + 1])."""
    a, y = data[:, :d], data[:, d]
    u = a @ np.asarray(x, np.float64).reshape(K, d).T
    q = np.exp(u) / (1.0 + np.exp(u).sum(axis=1))[:, None]
    g = np.zeros(K * d)
    H = np.zeros((K * d, K * d))
    for k in range(K):
        g[k * d:(k + 1) * d] = a.T @ (q[:, k] - (y == k + 1))
        for l in range(K):
            wkl = q[:, k] * ((k == l) - q[:, l])
            H[k * d:(k + 1) * d, l * d:(l + 1) * d] = (a * wkl[:, None]).T @ a
    return g, H


def softmax_case(seed, K, d, items, separable=False):
    """Features N(0, 1) / sqrt(d), classes drawn from the softmax of a random weight matrix (noisy labels: a finite minimiser where
    items exceed the parameters), x0 far from it; separable: the most likely class instead, which no finite x minimises."""
    rng = np.random.default_rng(7700 + 131 * K + 17 * d + seed)
    a = rng.normal(size=(items, d)) / np.sqrt(d)
    Wt = rng.normal(size=(K, d)) * 2.0
    u = np.concatenate([np.zeros((items, 1)), a @ Wt.T], axis=1)
    pr = np.exp(u - u.max(axis=1, keepdims=True))
    pr /= pr.sum(axis=1, keepdims=True)
    y = pr.argmax(axis=1) if separable else np.array([rng.choice(K + 1, p=row) for row in pr])
    return np.concatenate([a, y[:, None].astype(np.float64)], axis=1), rng.normal(size=K * d) * 0.5


def gauss_parts(x, data, want):
    """A heteroscedastic Gaussian likelihood, two predictors per item (K = 2, n = 4): mean m = a0 x0 + a1 x1 and log-variance
    s = a0 x2 + a1 x3; item = (a0, a1, y).  c = (s + (y - m)^2 exp(-s)) / 2.  Hs is the FISHER information of (m, s), diag(exp(-s), 1/2)
    (the observed curvature of this likelihood is indefinite wherever y != m; the kind is a Gauss-Newton door)."""
    a, y = data[:, :2], data[:, 2]
    m, s = a @ x[:2], a @ x[2:]
    ies, rr = np.exp(-s), y - (a @ x[:2])
    c = 0.5 * (s + rr * rr * ies)
    if not want:
        return c, None, None, None
    gs = np.stack([-rr * ies, 0.5 * (1.0 - rr * rr * ies)], axis=1)
    Hs = np.zeros((len(y), 2, 2), x.dtype)
    Hs[:, 0, 0], Hs[:, 1, 1] = ies, 0.5
    J = np.zeros((len(y), 2, 4), x.dtype)
    J[:, 0, :2], J[:, 1, 2:] = a, a
    return c, gs, Hs, J


GAUSS_BODY = """
const T m = p[0] * x[0] + p[1] * x[1], s = p[0] * x[2] + p[1] * x[3];
const T ies = exp(-s), rr = p[2] - m;
c = T(0.5) * (s + rr * rr * ies);
if (want_grad) {
  gs[0] = -rr * ies; gs[1] = T(0.5) * (T(1) - rr * rr * ies);
  Hs[0][0] = ies; Hs[1][0] = T(0); Hs[1][1] = T(0.5);
  J[0][0] = p[0]; J[0][1] = p[1]; J[0][2] = T(0); J[0][3] = T(0);
  J[1][0] = T(0); J[1][1] = T(0); J[1][2] = p[0]; J[1][3] = p[1];
}
"""


def gauss_case(seed, items=60):
    rng = np.random.default_rng(8800 + seed)
    a = np.stack([np.ones(items), rng.uniform(-1, 1, items)], axis=1)
    xt = np.array([0.5, 1.5, -0.5, 1.0])
    y = a @ xt[:2] + np.exp(0.5 * (a @ xt[2:])) * rng.normal(size=items)
    return np.concatenate([a, y[:, None]], axis=1), xt + rng.normal(size=4) * 0.8


def quadratic_parts(K, n):
    """c = (u - b)^T A (u - b) / 2 with u = V x (K outputs): item = V (K n), b (K), the lower triangle of A (K (K + 1) / 2, row by row)."""
    def parts(x, data, want):
        V = data[:, :K * n].reshape(-1, K, n)
        b = data[:, K * n:K * n + K]
        A = np.zeros((len(data), K, K), x.dtype)
        A[:, np.tril_indices(K)[0], np.tril_indices(K)[1]] = data[:, K * n + K:]
        S = np.tril(A) + np.transpose(np.tril(A, -1), (0, 2, 1))
        r = V @ x - b
        c = 0.5 * np.einsum("ik,ikl,il->i", r, S, r)
        if not want:
            return c, None, None, None
        return c, np.einsum("ikl,il->ik", S, r), A, V
    return parts


def quadratic_body(K, n):
    o_b, o_A = K * n, K * n + K
    tri = [(k, l) for k in range(K) for l in range(k + 1)]
    sym = lambda k, l: o_A + tri.index((max(k, l), min(k, l)))   # noqa: E731
    lines = [f"T r[{K}];", f"for (int k = 0; k < {K}; ++k) {{ r[k] = -p[{o_b} + k]; for (int j = 0; j < {n}; ++j) r[k] += p[k * {n} + j] * x[j]; }}"]
    for k in range(K):
        lines.append(f"const T t{k} = " + " + ".join(f"p[{sym(k, l)}] * r[{l}]" for l in range(K)) + ";")
    lines.append("c = T(0.5) * (" + " + ".join(f"r[{k}] * t{k}" for k in range(K)) + ");")
    lines.append("if (want_grad) {")
    lines += [f"  gs[{k}] = t{k};" for k in range(K)]
    lines += [f"  Hs[{k}][{l}] = p[{o_A + i}];" for i, (k, l) in enumerate(tri)]
    lines.append(f"  for (int k = 0; k < {K}; ++k) for (int a = 0; a < {n}; ++a) J[k][a] = p[k * {n} + a];")
    lines.append("}")
    return "\n".join(lines) + "\n"


def table_parts(K, n):
    """The exact-sum body: nothing depends on x — item = J (K n), c, gs (K), the lower triangle of Hs (row by row)."""
    def parts(x, data, want):
        c = data[:, K * n]
        if not want:
            return c, None, None, None
        Hs = np.zeros((len(data), K, K), data.dtype)
        Hs[:, np.tril_indices(K)[0], np.tril_indices(K)[1]] = data[:, K * n + 1 + K:]
        return c, data[:, K * n + 1:K * n + 1 + K], Hs, data[:, :K * n].reshape(-1, K, n)
    return parts


def table_scalars(K, n):
    return K * n + 1 + K + K * (K + 1) // 2


def table_body(K, n, shared=False):
    """shared: J comes from the shared table s[] (K n scalars per row), the rest stays in the item."""
    o = 0 if shared else K * n
    src = "s" if shared else "p"
    tri = [(k, l) for k in range(K) for l in range(k + 1)]
    lines = [f"c = p[{o}];", "if (want_grad) {", f"  for (int k = 0; k < {K}; ++k) gs[k] = p[{o + 1} + k];"]
    lines += [f"  Hs[{k}][{l}] = p[{o + 1 + K + i}];" for i, (k, l) in enumerate(tri)]
    lines.append(f"  for (int k = 0; k < {K}; ++k) for (int a = 0; a < {n}; ++a) J[k][a] = {src}[k * {n} + a];")
    lines.append("}")
    return "\n".join(lines) + "\n"


def exact_case(K, n, items, P, seed=0):
    """Items whose sums are exact in float32 in ANY order.  J in {-2 .. 2} / 2, gs integers in -2 .. 2, c in {-64 .. 64} / 8 and
    Hs = L D L^T with L unit lower triangular, its entries below the diagonal in {0, +-1/2, +-1}, and per PROBLEM one of three
    regimes for D: powers of four in {1, 4} (problems 0, 3, 6, ...), D = 0 (1, 4, ...: Hs = 0) and D in {-1, -4} (2, 5, ...).  The
    factorisation finds L and D again exactly (every quotient divides by a power of four).  Positive regime, K <= 4, at most 256 items
    (1024 rows): a row sqrt(d_j) (J_j + sum L_ij J_i) is a multiple of 1/4 of magnitude <= 8, y = L^-1 gs a multiple of 1/8 of magnitude
    <= 16, r = y / sqrt(d) a multiple of 1/16 <= 16; a term of g is a multiple of 2^-6 <= 2^7 and the sum of 2^10 of them needs 23
    bits, a term of H a multiple of 2^-4 <= 2^6, 20 bits; the cost 2^3 x 2^8 in steps of 2^-3, 14 bits — all within float32's 24.  The
    other two regimes clamp every pivot (a negative semi-definite Hs has no positive pivot once the earlier ones count as 0): the rows
    are sqrt(wmin) J_j, a power of two times multiples of 1/2, r = gs / sqrt(wmin), and H = wmin sum J_j J_j^T exactly."""
    assert K <= 4 and items <= 256
    rng = np.random.default_rng(100000 * K + 1000 * n + items + seed)
    d = np.zeros((P, items, table_scalars(K, n)))
    d[:, :, :K * n] = rng.integers(-2, 3, (P, items, K * n)) / 2.0
    d[:, :, K * n] = rng.integers(-64, 65, (P, items)) / 8.0
    d[:, :, K * n + 1:K * n + 1 + K] = rng.integers(-2, 3, (P, items, K))
    il = np.tril_indices(K)
    for p in range(P):
        L = np.tril(rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], (items, K, K)), -1) + np.eye(K)
        if p % 3 == 0:
            D = 4.0 ** rng.integers(0, 2, (items, K))
        elif p % 3 == 1:
            D = np.zeros((items, K))
        else:
            D = -(4.0 ** rng.integers(0, 2, (items, K)))
        Hs = np.einsum("iab,ib,icb->iac", L, D, L)
        d[p, :, K * n + 1 + K:] = Hs[:, il[0], il[1]]
    return d


def exact_sums(K, n, d, dtype, wmin_of=None):
    parts = table_parts(K, n)
    out = [sums(parts, np.zeros(n), d[p], dtype, True, wmin_of) for p in range(d.shape[0])]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


# ---- geometry: items per super-step of the model's passes (csrc/row_stage_geom.hpp RowStageGeom::make, restated for K rows per item) ---
def row_stage_items(K, n, item_scalars, dtype, shared_scalars=0):
    """Items per super-step of the ring of two regions (the accumulate pass and the cost-only pass of this kind both use it)."""
    sz = np.dtype(dtype).itemsize
    rem = n & 15
    thin = n >= 16 and rem + 1 <= 4
    nbm = (n >> 4) if thin else (n + 16) // 16
    rs = 16 * nbm + rem + 1 if thin else nbm * ((n + nbm) // nbm)
    st = gr._stride16
    rsp, ps, pss = st(rs, sz), (st(item_scalars, sz) if item_scalars > 0 else 0), (st(shared_scalars, sz) if shared_scalars > 0 else 0)
    bud = 160 * 1024 // 8 - 320 * sz - 512
    it = 64 // K
    if it >= 4:
        it &= ~3
    while it > 1 and 2 * max(it * (ps + pss) * sz, ((it * K + 3) & ~3) * rsp * sz) > bud:
        it = it - 4 if it > 4 else it >> 1
    return it


def optimize_full_hessian(K, d, data, x0, opt):
    """The sibling's yardstick: the same softmax cost with its FULL Hessian stated on its own (softmax_full_hessian: what a
    kind="cost_hess" body adds up), inside the same second reading of the loop."""
    data = np.asarray(data, np.float64)
    parts = softmax_parts(K, d)

    def fn(x, want):
        x = np.asarray(x, np.float64)
        c = float(parts(x, data, False)[0].sum())
        if not want:
            return c, None, None, 1
        g, H = softmax_full_hessian(K, d, x, data)
        return c, g.tolist(), H.tolist(), 1
    return br.optimize_plain(fn, [float(v) for v in x0], opt)
