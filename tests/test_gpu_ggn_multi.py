"""Multi-output second-order scalar costs on the device (kind="cost_ggn_multi"): run-time bodies that assign c,
gs[k], Hs[k][l] and J[k][a]; the lane factors Hs and writes K scaled rows per item into the row models' image, so that the matrix-core
Gram holds g = sum gs_k J_k and H = sum J^T Hs J; LM / GN through lm_fused_kernel<RowModel<GgnMultiRowFunctor>>, with a Gaussian prior
as the ridge term and with a shared item table.  Yardstick: tests/ggn_multi_reference.py.  Every test here needs the kind, so every one
of them fails on a library that does not know it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ggn_multi_reference as gm  # noqa: E402
import ggn_reference as gr  # noqa: E402
import hess_reference as hr  # noqa: E402
from ggn_multi_cells import CELLS, PRIOR_CELLS, SEEDS, body_of, parts_of, prior_of, trajectory_cases  # noqa: E402
from parity import gpu_dict  # noqa: E402
from test_gpu_ggn import _check_problem, ref_dict  # noqa: E402

pytestmark = pytest.mark.gpu
TDT = {np.float32: torch.float32, np.float64: torch.float64}
EPS = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}   # the unit round-off
P = 97
_MODELS = {}


def model_of(ta, key, body, n, kD, K, dtype, kind="cost_ggn_multi", kS=0):
    """One compiled model per (key, dtype) for the whole module."""
    k = (key, dtype)
    if k not in _MODELS:
        _MODELS[k] = ta.JitResidual(body, n=n, item_scalars=kD, residuals_per_item=K, kind=kind, dtype=TDT[dtype], shared_scalars=kS)
    return _MODELS[k]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the sum, exactly -----------------------------------------------------------------------------------------------------------
LAYOUT_EDGES = [1, 2, 12, 13, 15, 16, 19, 20, 31, 32, 35, 36, 47, 48, 50, 51, 52, 63]   # every edge of DenseRowLayout::make, and 50
EXACT_CELLS = [(K, n) for K in (1, 2, 3, 4) for n in LAYOUT_EDGES]
KIND5_TOO = (1, 13, 19, 50, 63)   # where the K = 1 cell also runs kind 5's table body on the same numbers


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K,n", EXACT_CELLS)
def test_the_sum_exactly(ta, K, n, dtype):
    """ggn_multi_reference.exact_case (its docstring states the bit budget): Hs = L D L^T from L in {0, +-1/2, +-1} and D a power of
    four, or zero, or negative, per problem.  accumulate's cost, g and H EQUAL numpy's at every edge of the super-step (IT items, from
    the geometry); the clamped problems give wmin sum_k J_k J_k^T exactly; with K = 1 kind 5 gives the same bits on the same numbers."""
    kD = gm.table_scalars(K, n)
    res = model_of(ta, f"table{K}x{n}", gm.table_body(K, n), n, kD, K, dtype)
    it = gm.row_stage_items(K, n, kD, dtype)
    counts = sorted({c for c in (1, 64 // K - 1, 64 // K, 64 // K + 1, it - 1, it, it + 1, 3 * it + 5) if c >= 1})
    x = cuda(np.zeros((P, n), dtype))
    for items in counts:
        d = gm.exact_case(K, n, items, P)
        c32, g32, H32 = gm.exact_sums(K, n, d, np.float32)
        c64, g64, H64 = gm.exact_sums(K, n, d, np.float64, np.float32)
        assert (c32 == c64).all() and (g32 == g64).all() and (H32 == H64).all(), "the case is not exact in float32"
        c64, g64, H64 = gm.exact_sums(K, n, d, np.float64, dtype)   # (the clamped problems' H with the dtype's own wmin)
        dd = cuda(d.astype(dtype))
        model = res.bind(dd)
        g, H, c, nres = ta.accumulate(model, x)
        assert (c.cpu().numpy() == c64).all(), (K, n, items, "cost")
        assert (g.cpu().numpy() == g64.astype(dtype)).all(), (K, n, items, "g")
        assert (H.cpu().numpy() == H64.astype(dtype)).all(), (K, n, items, "H")
        assert (nres.cpu().numpy() == 1).all()
        g0, H0, c0, _ = ta.accumulate(model, x, want_grad=False)
        assert g0 is None and H0 is None and (c0.cpu().numpy() == c64).all(), (K, n, items, "cost only")
        J = d[1::3, :, :K * n].reshape(-1, items * K, n)
        wmin = gm.WMIN[np.dtype(dtype)]
        assert (H.cpu().numpy()[1::3] == (wmin * np.einsum("pia,pib->pab", J, J)).astype(dtype)).all() and np.abs(g64[1::3]).max() > 0
        if K == 1 and n in KIND5_TOO:   # the same item layout as kind 5's table body: (J (n), c, gs, hs)
            r5 = model_of(ta, f"table5x{n}", gr.table_body(n), n, kD, 1, dtype, kind="cost_ggn")
            g5, H5, c5, _ = ta.accumulate(r5.bind(dd), x)
            assert torch.equal(g5, g) and torch.equal(H5, H) and torch.equal(c5, c), (n, items, "kind 5")


def test_K1_solves_as_kind_5_bit_for_bit(ta):
    """The logistic body as kind 5 and as kind 6 with K = 1 on the same 97 problems: the same x, costs, iterations to the bit."""
    n, items = 13, 200
    cases = [gr.logistic_case(seed, n, items) for seed in range(P)]
    data, x0 = cuda(np.array([c[0] for c in cases])), np.array([c[1] for c in cases])
    b6 = (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j];\nconst T y = p[{n}], e = exp(-y * z), s = T(1) / (T(1) + e);\nc = log(T(1) + e);\n"
          f"if (want_grad) {{ gs[0] = -y * (T(1) - s); Hs[0][0] = s * (T(1) - s); for (int a = 0; a < {n}; ++a) J[0][a] = p[a]; }}\n")
    for dtype in (np.float32, np.float64):
        r5 = model_of(ta, "logistic13 kind 5", gr.logistic_body(n), n, n + 1, 1, dtype, kind="cost_ggn")
        r6 = model_of(ta, "logistic13 K1", b6, n, n + 1, 1, dtype)
        x5, x6 = cuda(x0.astype(dtype)), cuda(x0.astype(dtype))
        dd = data.to(TDT[dtype])
        o5, o6 = ta.Optimize(x5, r5.bind(dd), ta.Options(), history=True), ta.Optimize(x6, r6.bind(dd), ta.Options(), history=True)
        torch.cuda.synchronize()
        assert torch.equal(x5, x6) and torch.equal(o5.final_cost, o6.final_cost) and torch.equal(o5.num_iters, o6.num_iters)
        assert torch.equal(o5.errs, o6.errs) and torch.equal(o5.stop_reason, o6.stop_reason)


# ---- 2. the sum, rounded -----------------------------------------------------------------------------------------------------------
def _abs_terms(gs_abs, Hs, J, dtype):
    """Per problem sum_items of the terms' magnitudes with the absolute values carried through the rule: |L|_ij = (|Hs_ij| +
    sum |L|_iq |L|_jq e_q) / d_j, |w|_j = |Hs_jj| + sum |L|_jq^2 e_q, |y|_j = |gs|_j + sum |L|_jq |y|_q, |C|_j = |J_j| + sum |L|_ij |J_i|;
    T_g = sum_j |y|_j |C|_j, T_H = sum_j |w|_j |C|_j |C|_j^T.  e, d: the pivots the fp64 rule finds (positive definite blocks: none clamped)."""
    items, K = gs_abs.shape
    _, _, w, _, _ = gm.transform(gs_abs, Hs, J, np.float64, dtype, full=True)
    La, wa = np.zeros((items, K, K)), np.zeros((items, K))
    for j in range(K):
        wa[:, j] = np.abs(Hs[:, j, j]) + sum(La[:, j, q] ** 2 * w[:, q] for q in range(j))
        for i in range(j + 1, K):
            La[:, i, j] = (np.abs(Hs[:, i, j]) + sum(La[:, i, q] * La[:, j, q] * w[:, q] for q in range(j))) / w[:, j]
    ya = np.zeros((items, K))
    for j in range(K):
        ya[:, j] = gs_abs[:, j] + sum(La[:, j, q] * ya[:, q] for q in range(j))
    Ca = np.abs(J).copy()
    for j in range(K):
        for i in range(j + 1, K):
            Ca[:, j, :] += La[:, i, j][:, None] * np.abs(J[:, i, :])
    return np.einsum("ik,ika->a", ya, Ca), np.einsum("ik,ika,ikb->ab", wa, Ca, Ca)


ROUNDED = [("softmax", 2, 6), ("softmax", 3, 5), ("softmax", 2, 25), ("softmax", 3, 21), ("softmax", 8, 2), ("gauss", 2, 2)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name,K,d", ROUNDED)
def test_the_sum_rounded(ta, name, K, d, dtype):
    """Softmax and the Gaussian likelihood on random data against the fp64 restatement, entry by entry: a device value lies within
    2 B of it, B = eps (items + c) sum_items |term|, the terms' magnitudes with the absolute values carried through L, y and the row
    combination (_abs_terms).  The derivation of c, in units of eps relative to those magnitudes (first order): a pivot d_j is Hs_jj
    minus j products of two factors each, 3 j roundings, and its root one more; an L_ij the same plus the division, 3 j + 1; the
    combination C_j adds K - 1 - j products, 2 (K - 1 - j) roundings plus those of the L it reads; a row is C_j times the root, 1; y_j
    has 2 j roundings plus those of its L, r = y / root 1.  A term of H is a product of two rows, a term of g a row times r; over
    j <= K - 1 every count is below 2 (3 K + 1) + 2 (K - 1) + 3 <= 8 K + 3, and the matrix core's product and the accumulation in any
    order are the `items K` rows' own — so c = 8 K + 3 per row, times K rows per item: B = eps K (items + 8 K + 3) sum |term|.  What
    feeds the rule is rounded too: the logits are dot products of d terms, |delta u| <= d eps sum |a_j x_j| =: d eps U, which moves every
    q_k, and with them gs and Hs, by a relative (K + 1) d eps U at the most (softmax's derivative in u is bounded by q (1 - q)); the
    library exp / log are the factor 2, as in test_gpu_ggn.py.  So B = eps (K (items + 8 K + 3) + (K + 1) d (1 + U)) sum |term|, U the
    problem's largest sum_j |a_j| |x_j|.  gs's magnitude is q + [y = k] (its two terms).  The cost: within items 2 eps sum |c_i| plus
    the logits' d eps U per item."""
    items = 200 if name == "softmax" else 60
    cases = [gm.softmax_case(seed, K, d, items) if name == "softmax" else gm.gauss_case(seed, items) for seed in range(P)]
    parts = gm.softmax_parts(K, d) if name == "softmax" else gm.gauss_parts
    body = gm.softmax_body(K, d) if name == "softmax" else gm.GAUSS_BODY
    n = K * d
    data = np.array([c[0] for c in cases]).astype(dtype)
    x0 = np.array([c[1] for c in cases]).astype(dtype)
    res = model_of(ta, f"{name}{K}x{d}", body, n, data.shape[2], K, dtype)
    g, H, c, nres = ta.accumulate(res.bind(cuda(data)), cuda(x0))
    g, H, c = g.cpu().numpy().astype(np.float64), H.cpu().numpy().astype(np.float64), c.cpu().numpy()
    eps, worst = EPS[dtype], dict(g=0.0, H=0.0, c=0.0)
    for p in range(P):
        xp, dp = x0[p].astype(np.float64), data[p].astype(np.float64)
        ci, gs, Hs, J = parts(xp, dp, True)
        _, gd, Hd = gm.direct_sums(parts, xp, dp)
        if name == "softmax":
            hit = (dp[:, d][:, None] == np.arange(1, K + 1)[None, :])
            gs_abs = np.abs(gs + hit) + hit
            U = (np.abs(dp[:, :d]) @ np.abs(xp.reshape(K, d)).T).max()
        else:
            rr2 = (dp[:, 2] - dp[:, :2] @ xp[:2]) ** 2 * np.exp(-(dp[:, :2] @ xp[2:]))
            gs_abs = np.stack([np.abs(gs[:, 0]), 0.5 * (1.0 + rr2)], axis=1)
            U = (np.abs(dp[:, :2]) @ np.abs(xp.reshape(2, 2)).T).max() * (1.0 + rr2.max())   # (rr^2 exp(-s) moves with both predictors)
        Tg, TH = _abs_terms(gs_abs, Hs, J, dtype)
        f = eps * (K * (items + 8 * K + 3) + (K + 1) * d * (1.0 + U))
        Bc = items * 2.0 * eps * np.abs(ci).sum() + items * d * eps * U
        worst["g"] = max(worst["g"], float((np.abs(g[p] - gd)[Tg > 0] / (f * Tg[Tg > 0])).max()))
        worst["H"] = max(worst["H"], float((np.abs(H[p] - Hd)[TH > 0] / (f * TH[TH > 0])).max()))
        assert (g[p][Tg == 0] == 0).all() and (H[p][TH == 0] == 0).all()
        worst["c"] = max(worst["c"], float(abs(c[p] - ci.sum()) / Bc))
    print(name, K, d, np.dtype(dtype).name, "worst ratio to B: g %.3f H %.3f, cost to its bound %.4f" % (worst["g"], worst["H"], worst["c"]))
    assert worst["g"] <= 2.0 and worst["H"] <= 2.0 and worst["c"] <= 1.0, worst
    assert (nres.cpu().numpy() == 1).all()


# ---- 3. trajectories ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,optname", CELLS)
def test_trajectories(ta, problem, optname):
    """fp64 against the second reading under parity.check_trajectories; seeds: ggn_multi_cells.py (section 20's margin rule).  The only
    permitted parting is a proven roll-back tie (test_gpu_ggn._check_problem)."""
    cases, refs, o_kw = trajectory_cases(problem, optname)
    o, _ = gm.options_pair(ta.Options, **o_kw)
    n = len(cases[0][1])
    K = 2 if problem == "gauss" else gm_K(problem)
    res = model_of(ta, problem, body_of(problem), n, cases[0][0].shape[1], K, np.float64)
    x = cuda(np.array([c[1] for c in cases]))
    out = ta.Optimize(x, res.bind(cuda(np.array([c[0] for c in cases]))), o, history=True)
    torch.cuda.synchronize()
    got, ref = gpu_dict(out, x), ref_dict(refs, out.errs.shape[1])
    verdicts = [_check_problem(got, ref, p, o.to_pod(), f"{problem} {optname}") for p in range(len(cases))]
    print(problem, optname, {v: verdicts.count(v) for v in sorted(set(verdicts))}, "stops", [r["stop"] for r in refs], "device", got["stop"].tolist(),
          "iterations", [r["num_iters"] for r in refs], "failures", [r["num_failures"] for r in refs])
    assert set(verdicts) <= {"full", "tie", "roll-back tie"}
    assert all(v != "roll-back tie" for v, r in zip(verdicts, refs) if all(r["successes"]))
    assert sum(1 for r in refs if not all(r["successes"])) >= 2, "the cell's coverage of rejected steps"
    assert (out.final_num_residuals.cpu().numpy() == 1).all() and (out.final_inlier_ratio.cpu().numpy() == 1).all()


def gm_K(problem):
    from ggn_multi_cells import PROBLEMS
    return PROBLEMS[problem][0]


@pytest.mark.parametrize("K,d", [(2, 6), (2, 25)])
def test_fp32_trajectories_end_at_the_minimum(ta, K, d):
    """fp32 under Options(): a success, and the final cost — recomputed in fp64 numpy at the device's final x — within
    items * 2^-23 * sum |c_i| of the fp64 yardstick's final cost: the worst-case rounding of the sum (test_gpu_hess.py's rule)."""
    parts, items = gm.softmax_parts(K, d), 200
    o, ropt = gm.options_pair(ta.Options)
    cases = [gm.softmax_case(seed, K, d, items) for seed in range(6)]
    cases = [(dd.astype(np.float32).astype(np.float64), x0.astype(np.float32).astype(np.float64)) for dd, x0 in cases]
    refs = [gm.optimize(parts, dd, x0, ropt) for dd, x0 in cases]
    res = model_of(ta, f"softmax{K}x{d}", gm.softmax_body(K, d), K * d, d + 1, K, np.float32)
    x = cuda(np.array([c[1] for c in cases], np.float32))
    out = ta.Optimize(x, res.bind(cuda(np.array([c[0] for c in cases], np.float32))), o)
    torch.cuda.synchronize()
    xs, stop = x.cpu().numpy().astype(np.float64), out.stop_reason.cpu().numpy()
    for p, ((dd, _), r) in enumerate(zip(cases, refs)):
        ci = parts(xs[p], dd, False)[0]
        bound = len(dd) * 2.0 ** -23 * np.abs(ci).sum()
        print("softmax", K, d, p, "stop", stop[p], "cost at the device's x", ci.sum(), "yardstick", r["final_cost"], "bound", bound)
        assert stop[p] >= 0 and abs(ci.sum() - r["final_cost"]) <= bound, (p, stop[p], ci.sum(), r["final_cost"], bound)


# ---- 4. ridge ----------------------------------------------------------------------------------------------------------------------
def _priors(n, dtype, full):
    rng = np.random.default_rng(77 + n + int(full))
    mu = rng.normal(size=(P, n)) * 0.1
    W = rng.uniform(0.5, 1.5, (P, 5 if full else 1, n)) * (rng.random((P, 5 if full else 1, n)) < (0.6 if full else 1.1))
    return mu.astype(dtype), (W if full else W[:, 0, :]).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("K,d", [(2, 6), (2, 25)])
def test_ridge_accumulate(ta, K, d, full, dtype):
    """accumulate with a prior = the items' sums (the device's own, without the prior) + the yardstick's ridge term to the prior's own
    rounding, eps (k + 2) sum |term| per entry (k rows of W, a product and a difference each); nres stays 1; and the reported cost's
    central difference matches g (this fails if the 1/2 is missing: the ridge's share of g would be half of the difference's)."""
    n, items = K * d, 200
    cases = [gm.softmax_case(seed, K, d, items) for seed in range(P)]
    data, x0 = np.array([c[0] for c in cases]).astype(dtype), np.array([c[1] for c in cases]).astype(dtype)
    mu, W = _priors(n, dtype, full)
    res = model_of(ta, f"softmax{K}x{d}", gm.softmax_body(K, d), n, d + 1, K, dtype)
    plain = res.bind(cuda(data))
    model = plain.with_prior(cuda(mu), cuda(W))
    x = cuda(x0)
    g0, H0, c0, _ = ta.accumulate(plain, x)
    g, H, c, nres = ta.accumulate(model, x)
    assert (nres.cpu().numpy() == 1).all()
    eps, k = EPS[dtype], (5 if full else 1)
    for p in range(P):
        pc, pg, pH = gm.ridge(x0[p].astype(np.float64), mu[p].astype(np.float64), W[p].astype(np.float64))
        Wa, ra = np.abs(W[p].astype(np.float64)), None
        dxa = np.abs(x0[p].astype(np.float64)) + np.abs(mu[p].astype(np.float64))
        ra = Wa * dxa if not full else Wa @ dxa
        Bg = eps * (k + 3) * ((Wa * ra) if not full else Wa.T @ ra) + eps * np.abs(g0[p].cpu().numpy().astype(np.float64))
        BH = eps * (k + 3) * (np.diag(Wa * Wa) if not full else Wa.T @ Wa) + eps * np.abs(H0[p].cpu().numpy().astype(np.float64))
        assert (np.abs(g[p].cpu().numpy() - (g0[p].cpu().numpy().astype(np.float64) + pg)) <= 2 * Bg + 1e-300).all(), p
        assert (np.abs(H[p].cpu().numpy() - (H0[p].cpu().numpy().astype(np.float64) + pH)) <= 2 * BH + 1e-300).all(), p
        assert abs(float(c[p]) - (float(c0[p]) + pc)) <= 2 * eps * (k + 3) * (0.5 * (ra * ra).sum()) + 2 * eps * abs(float(c0[p])), p
    if dtype == np.float64:   # the reported cost's central difference against g: truncation h^2 |c'''| / 6 and round-off 2 eps cost / h
        h = 1e-5
        for a in (0, n - 1):
            xp, xm = x.clone(), x.clone()
            xp[:, a] += h
            xm[:, a] -= h
            cp, cm = ta.accumulate(model, xp, want_grad=False)[2], ta.accumulate(model, xm, want_grad=False)[2]
            num = ((cp - cm) / (xp[:, a] - xm[:, a])).cpu().numpy()
            tol = 1e-4 * np.abs(g[:, a].cpu().numpy()) + 8 * 2.0 ** -53 * np.abs(c.cpu().numpy()) / h + 1e-6
            assert (np.abs(num - g[:, a].cpu().numpy()) <= tol).all(), (a, np.abs(num - g[:, a].cpu().numpy()).max())
            ridge_share = np.array([gm.ridge(x0[p], mu[p], W[p])[1][a] for p in range(P)])
            assert (np.abs(ridge_share) > 4 * tol).sum() > P // 2, "the ridge's share of g is visible in most problems"


@pytest.mark.parametrize("problem,form", PRIOR_CELLS)
def test_ridge_trajectories(ta, problem, form):
    """fp64 softmax at n = 12 and n = 50 with a diagonal and a full prior under Options(), iteration by iteration against the yardstick
    with the ridge term (ggn_multi_cells.PRIOR_CELLS: seeds by the margin rule, at least two problems per cell reject a step, so the
    roll-back and the cost-only passes run with the prior too).  The only permitted parting is a proven roll-back tie."""
    cases, refs, o_kw = trajectory_cases(problem, form)
    o, _ = gm.options_pair(ta.Options, **o_kw)
    n, K = len(cases[0][1]), gm_K(problem)
    pri = [prior_of(problem, form, seed) for seed in SEEDS[(problem, form)]]
    res = model_of(ta, problem, body_of(problem), n, cases[0][0].shape[1], K, np.float64)
    x = cuda(np.array([c[1] for c in cases]))
    model = res.bind(cuda(np.array([c[0] for c in cases]))).with_prior(cuda(np.array([q[0] for q in pri])), cuda(np.array([q[1] for q in pri])))
    out = ta.Optimize(x, model, o, history=True)
    torch.cuda.synchronize()
    got, ref = gpu_dict(out, x), ref_dict(refs, out.errs.shape[1])
    verdicts = [_check_problem(got, ref, p, o.to_pod(), f"{problem} {form}") for p in range(len(cases))]
    print(problem, form, {v: verdicts.count(v) for v in sorted(set(verdicts))}, "stops", [r["stop"] for r in refs], "device", got["stop"].tolist(),
          "iterations", [r["num_iters"] for r in refs], "failures", [r["num_failures"] for r in refs])
    assert set(verdicts) <= {"full", "tie", "roll-back tie"}
    assert all(v != "roll-back tie" for v, r in zip(verdicts, refs) if all(r["successes"]))
    assert sum(1 for r in refs if not all(r["successes"])) >= 2, "the cell's coverage of rejected steps"
    assert (out.final_num_residuals.cpu().numpy() == 1).all() and (out.final_inlier_ratio.cpu().numpy() == 1).all()
    if set(verdicts) == {"full"}:   # final_hessian: the items' Gram + W^T W at the last Build
        Hr = np.array([r["final_hessian"] for r in refs])
        assert np.allclose(out.final_hessian.cpu().numpy(), Hr, rtol=1e-6, atol=1e-9 * np.abs(Hr).max())


def test_ridge_makes_a_separable_problem_finite(ta):
    """Separable labels: no finite minimiser without the ridge; with a diagonal ridge the solve ends with a success at a finite x."""
    K, d, items = 2, 6, 60
    n = K * d
    cases = [gm.softmax_case(seed, K, d, items, separable=True) for seed in range(P)]
    res = model_of(ta, f"softmax{K}x{d}", gm.softmax_body(K, d), n, d + 1, K, np.float64)
    x = cuda(np.zeros((P, n)))
    lam = cuda(np.full((P, n), 0.3))
    o = ta.Options()
    o.max_iters = 100
    out = ta.Optimize(x, res.bind(cuda(np.array([c[0] for c in cases]))).with_prior(cuda(np.zeros((P, n))), lam), o)
    torch.cuda.synchronize()
    assert (out.stop_reason.cpu().numpy() >= 0).all() and bool(torch.isfinite(x).all()) and float(x.abs().max()) < 1e3
    assert (out.final_cost.cpu().numpy() < items * np.log(3.0)).all()


# ---- 5. against the sibling --------------------------------------------------------------------------------------------------------
def softmax_hess_body(K, d):
    """The same cost as a kind="cost_hess" body: the full Hessian added to the register triangle."""
    n = K * d
    return "\n".join([
        f"T u[{K}];",
        f"for (int k = 0; k < {K}; ++k) {{ u[k] = T(0); for (int j = 0; j < {d}; ++j) u[k] += p[j] * x[k * {d} + j]; }}",
        f"T mx = T(0); for (int k = 0; k < {K}; ++k) mx = fmax(mx, u[k]);",
        f"T e[{K}]; T z = exp(-mx); for (int k = 0; k < {K}; ++k) {{ e[k] = exp(u[k] - mx); z += e[k]; }}",
        f"const T y = p[{d}]; T uy = T(0); for (int k = 0; k < {K}; ++k) uy = (y == T(k + 1)) ? u[k] : uy;",
        "c = log(z) + mx - uy;",
        "if (want_grad) {",
        f"  T q[{K}]; for (int k = 0; k < {K}; ++k) q[k] = e[k] / z;",
        f"  for (int k = 0; k < {K}; ++k) {{ const T gk = q[k] - ((y == T(k + 1)) ? T(1) : T(0));",
        f"    for (int i = 0; i < {d}; ++i) {{ G[k * {d} + i] += gk * p[i];",
        f"      for (int l = k; l < {K}; ++l) {{ const T w = (k == l) ? q[k] * (T(1) - q[k]) : -q[k] * q[l];",
        f"        for (int j = 0; j < {d}; ++j) if (l > k || j >= i) H(k * {d} + i, l * {d} + j) += w * p[i] * p[j]; }} }} }}",
        "}"]) + f"\n// n = {n}\n"


def test_against_cost_hess(ta):
    """n = 12 (K = 2, d = 6): the same 97 softmax problems through kind="cost_hess" (the full Hessian of the same cost; u is linear, so
    it IS J^T Hs J) and through the new kind, min_rerr_dec = 1e-6: the same StopReason, iteration count and accept flags; at most 5 %
    may part."""
    K, d, items = 2, 6, 200
    n = K * d
    cases = [gm.softmax_case(seed, K, d, items) for seed in range(P)]
    data, x0 = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    o, _ = gm.options_pair(ta.Options, min_rerr_dec=1e-6)
    rh = model_of(ta, "softmax hess", softmax_hess_body(K, d), n, d + 1, 1, np.float64, kind="cost_hess")
    rg = model_of(ta, f"softmax{K}x{d}", gm.softmax_body(K, d), n, d + 1, K, np.float64)
    xh, xg = cuda(x0.copy()), cuda(x0.copy())
    oh, og = ta.Optimize(xh, rh.bind(cuda(data)), o, history=True), ta.Optimize(xg, rg.bind(cuda(data)), o, history=True)
    torch.cuda.synchronize()
    parted = sum(1 for p in range(P) if not (int(oh.stop_reason[p]) == int(og.stop_reason[p]) and int(oh.num_iters[p]) == int(og.num_iters[p]) and
                                             torch.equal(oh.successes[p], og.successes[p])))
    print("against cost_hess: parted", parted, "of", P)
    assert parted <= 0.05 * P
    assert np.allclose(xh.cpu().numpy(), xg.cpu().numpy(), rtol=1e-4, atol=1e-5)


# ---- 6. shared table ---------------------------------------------------------------------------------------------------------------
def softmax_shared_body(K, d):
    return gm.softmax_body(K, d).replace("p[j]", "s[j]").replace(f"p[{d}]", "p[0]")


@pytest.mark.parametrize("K,d", [(2, 6), (2, 25)])
def test_shared_table_equals_the_replicated_twin(ta, K, d):
    """One design matrix for 97 softmax problems (the labels stay private): accumulate and whole solves equal the replicated twin bit
    for bit, with and without a ridge."""
    n, items = K * d, 200
    rng = np.random.default_rng(31 + d)
    X = rng.normal(size=(items, d)) / np.sqrt(d)
    y = rng.integers(0, K + 1, (P, items)).astype(np.float64)
    x0 = rng.normal(size=(P, n)) * 0.5
    mu, W = _priors(n, np.float32, False)
    for dtype in (np.float32, np.float64):
        twin = model_of(ta, f"softmax{K}x{d}", gm.softmax_body(K, d), n, d + 1, K, dtype)
        sh = model_of(ta, f"softmax shared {K}x{d}", softmax_shared_body(K, d), n, 1, K, dtype, kS=d)
        rep = cuda(np.concatenate([np.broadcast_to(X, (P, items, d)), y[:, :, None]], axis=2).astype(dtype))
        mt, ms = twin.bind(rep), sh.bind(cuda(y[:, :, None].astype(dtype)), shared=cuda(X.astype(dtype)))
        for with_ridge in (False, True):
            if with_ridge:
                mt, ms = mt.with_prior(cuda(mu.astype(dtype)), cuda(W.astype(dtype))), ms.with_prior(cuda(mu.astype(dtype)), cuda(W.astype(dtype)))
            xa = cuda(x0.astype(dtype))
            for a, b in zip(ta.accumulate(mt, xa), ta.accumulate(ms, xa)):
                assert torch.equal(a, b), (K, d, dtype, with_ridge)
            xt, xs = cuda(x0.astype(dtype)), cuda(x0.astype(dtype))
            ot, os_ = ta.Optimize(xt, mt, ta.Options()), ta.Optimize(xs, ms, ta.Options())
            torch.cuda.synchronize()
            assert torch.equal(xt, xs) and torch.equal(ot.final_cost, os_.final_cost) and torch.equal(ot.stop_reason, os_.stop_reason)
            assert (ot.stop_reason.cpu().numpy() >= 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K,n", [(2, 12), (3, 50)])
def test_shared_exact_cell_equals_the_replicated_twin(ta, K, n, dtype):
    """The exact-sum cell with J in the shared table (one [items, K n] table for all 97 problems; c, gs and Hs stay private): cost, g
    and H EQUAL numpy's and the replicated twin's, bit for bit, at the edges of the super-step."""
    kD = gm.table_scalars(K, n)
    twin = model_of(ta, f"table{K}x{n}", gm.table_body(K, n), n, kD, K, dtype)
    sh = model_of(ta, f"table shared {K}x{n}", gm.table_body(K, n, shared=True), n, kD - K * n, K, dtype, kS=K * n)
    it = gm.row_stage_items(K, n, kD - K * n, dtype, K * n)
    x = cuda(np.zeros((P, n), dtype))
    for items in sorted({1, it - 1, it, it + 1, 3 * it + 5} - {0}):
        d = gm.exact_case(K, n, items, P)
        d[:, :, :K * n] = d[0, :, :K * n]   # one J for the whole batch
        c64, g64, H64 = gm.exact_sums(K, n, d, np.float64, dtype)
        gt, Ht, ct, _ = ta.accumulate(twin.bind(cuda(d.astype(dtype))), x)
        gs_, Hs_, cs_, nres = ta.accumulate(sh.bind(cuda(d[:, :, K * n:].astype(dtype)), shared=cuda(d[0, :, :K * n].astype(dtype))), x)
        assert torch.equal(gt, gs_) and torch.equal(Ht, Hs_) and torch.equal(ct, cs_) and (nres.cpu().numpy() == 1).all(), (K, n, items)
        assert (cs_.cpu().numpy() == c64).all() and (gs_.cpu().numpy() == g64.astype(dtype)).all() and (Hs_.cpu().numpy() == H64.astype(dtype)).all()


# ---- 7. further --------------------------------------------------------------------------------------------------------------------
def test_more_problems_than_waves_permuted_and_repeated(ta):
    K, d = 2, 6
    res = model_of(ta, f"softmax{K}x{d}", gm.softmax_body(K, d), K * d, d + 1, K, np.float32)
    waves = 4 * torch.cuda.get_device_properties(0).multi_processor_count * res.stats()["wg_per_cu"]
    Pbig = waves + 501
    base = [gm.softmax_case(seed, K, d, 40) for seed in range(64)]
    pick = np.arange(Pbig) % 64
    data = np.array([base[i][0] for i in pick], np.float32)
    x0 = np.array([base[i][1] for i in pick], np.float32)
    o = ta.Options()
    x = cuda(x0.copy())
    out = ta.Optimize(x, res.bind(cuda(data)), o)
    assert int(out.counters[3]) == Pbig
    x2 = cuda(x0.copy())
    out2 = ta.Optimize(x2, res.bind(cuda(data)), o)
    assert torch.equal(x, x2) and torch.equal(out.final_cost, out2.final_cost)
    perm = np.random.default_rng(5).permutation(Pbig)
    xp = cuda(x0[perm].copy())
    outp = ta.Optimize(xp, res.bind(cuda(data[perm])), o)
    torch.cuda.synchronize()
    pt = torch.from_numpy(perm).cuda()
    assert torch.equal(xp, x[pt]) and torch.equal(outp.final_cost, out.final_cost[pt]) and torch.equal(outp.num_iters, out.num_iters[pt])
    assert torch.equal(x[:64], x[64:128])


@pytest.mark.parametrize("what", ["c", "gs", "Hs", "J"])
def test_a_non_finite_item_ends_its_problem_alone(ta, what):
    K, n, items = 2, 5, 70
    d = gm.exact_case(K, n, items, 3)
    d[:, :, K * n + 1 + K:] = np.array([1.0, 0.5, 4.0])   # Hs = [[1, .], [.5, 4]]: positive definite everywhere
    bad = d.copy()
    col = {"c": K * n, "gs": K * n + 2, "Hs": K * n + 1 + K + 1, "J": n + 2}[what]
    bad[1, 66, col] = float("nan")
    o_b = K * n
    body = (f"T u[2]; for (int k = 0; k < 2; ++k) {{ u[k] = T(0); for (int j = 0; j < {n}; ++j) u[k] += p[k * {n} + j] * x[j]; }}\n"
            f"const T t0 = p[{o_b + 3}] * u[0] + p[{o_b + 4}] * u[1], t1 = p[{o_b + 4}] * u[0] + p[{o_b + 5}] * u[1];\n"
            f"c = p[{o_b}] + T(0.5) * (u[0] * t0 + u[1] * t1) + p[{o_b + 1}] * u[0] + p[{o_b + 2}] * u[1];\n"
            f"if (want_grad) {{ gs[0] = p[{o_b + 1}] + t0; gs[1] = p[{o_b + 2}] + t1; Hs[0][0] = p[{o_b + 3}]; Hs[1][0] = p[{o_b + 4}]; Hs[1][1] = p[{o_b + 5}];\n"
            f"  for (int k = 0; k < 2; ++k) for (int a = 0; a < {n}; ++a) J[k][a] = p[k * {n} + a]; }}\n")
    res = model_of(ta, "quadlike", body, n, gm.table_scalars(K, n), K, np.float64)
    x0 = np.full((3, n), 0.25)
    xa, xb = cuda(x0.copy()), cuda(x0.copy())
    oa = ta.Optimize(xa, res.bind(cuda(d)), ta.Options())
    ob = ta.Optimize(xb, res.bind(cuda(bad)), ta.Options())
    torch.cuda.synchronize()
    assert int(ob.stop_reason[1]) == int(ta.StopReason.kSystemHasNaNOrInf) and torch.equal(xb[1], cuda(x0[1]))
    for p in (0, 2):
        assert torch.equal(xa[p], xb[p]) and int(oa.stop_reason[p]) == int(ob.stop_reason[p]) and int(oa.stop_reason[p]) >= 0


def test_an_indefinite_Hs_still_steps_downhill(ta):
    """Hs = [[1, 2], [2, 1]] (eigenvalues 3 and -1) at every item of problem 0: the second pivot, 1 - 4 = -3, is clamped — H is positive
    semi-definite, g is the true gradient, and one damped step goes downhill."""
    K, n, items = 2, 3, 30
    rng = np.random.default_rng(3)
    d = np.zeros((2, items, K * n + K + 3))   # quadratic_parts' item: V (K n), b (K), the lower triangle of A
    d[:, :, :K * n + K] = rng.normal(size=(2, items, K * n + K))
    d[0, :, K * n + K:] = np.array([1.0, 2.0, 1.0])
    d[1, :, K * n + K:] = np.array([2.0, 1.0, 2.0])
    res = model_of(ta, "quadratic2x3", gm.quadratic_body(K, n), n, K * n + K + 3, K, np.float64)
    x0 = np.full((2, n), 0.1)
    model = res.bind(cuda(d))
    g, H, c0, _ = ta.accumulate(model, cuda(x0.copy()))
    assert np.linalg.eigvalsh(H[0].cpu().numpy()).min() >= -1e-12 * float(H[0].abs().max())
    _, gd, _ = gm.direct_sums(gm.quadratic_parts(K, n), x0[0], d[0])
    assert np.allclose(g[0].cpu().numpy(), gd, rtol=1e-12, atol=1e-12)   # the gradient, whatever was clamped
    o = ta.Options()
    o.max_iters = 1
    x = cuda(x0.copy())
    out = ta.Optimize(x, model, o)
    torch.cuda.synchronize()
    c1 = ta.accumulate(model, x, want_grad=False)[2]
    assert int(out.stop_reason[0]) >= 0 and float(c1[0]) < float(c0[0]) and float(c1[1]) < float(c0[1])


def test_outputs_save_last_and_covariance(ta):
    K, d, items = 3, 5, 200
    n = K * d
    cases = [gm.softmax_case(seed, K, d, items) for seed in range(6)]
    data, x0 = cuda(np.array([c[0] for c in cases])), np.array([c[1] for c in cases])
    res = model_of(ta, f"softmax{K}x{d}", gm.softmax_body(K, d), n, d + 1, K, np.float64)
    og = ta.Options()
    og.solver_type, og.max_iters = ta.Options.GaussNewton, 0
    xg = cuda(x0.copy())
    outg = ta.Optimize(xg, res.bind(data), og)
    H0 = ta.accumulate(res.bind(data), cuda(x0.copy()))[1]
    assert torch.equal(outg.final_hessian, H0.to(torch.float64))
    assert (outg.final_num_residuals.cpu().numpy() == 1).all() and (outg.final_inlier_ratio.cpu().numpy() == 1).all()
    x = cuda(x0.copy())
    out = ta.Optimize(x, res.bind(data), ta.Options())
    cov = out.Covariance()
    Hf = out.final_hessian.cpu().numpy()
    cov = (cov[0] if isinstance(cov, tuple) else cov).cpu().numpy()
    for p in range(6):   # the inverse Fisher information of the fit
        assert np.allclose(cov[p] @ Hf[p], np.eye(n), atol=1e-6), p


def test_check_gradient(ta):
    K, d = 2, 6
    n = K * d
    cases = [gm.softmax_case(seed, K, d, 200) for seed in range(3)]
    data, x = cuda(np.array([c[0] for c in cases])), cuda(np.array([c[1] for c in cases]))
    res = model_of(ta, f"softmax{K}x{d}", gm.softmax_body(K, d), n, d + 1, K, np.float64)
    good = ta.CheckGradient(res.bind(data), x, check_H=True)   # (u is linear in x: H agrees with the differences too)
    print("CheckGradient: g", good.max_dist_g.tolist(), "H", good.max_dist_H.tolist(), "eps", good.eps)
    assert good.all() and float(good.max_dist_H.max()) < good.eps and float(good.max_dist_g.max()) < good.eps
    assert ta.CheckGradient(res.bind(data), x, check_H=False).all()
    flipped = model_of(ta, "softmax flipped", gm.softmax_body(K, d, flip=True), n, d + 1, K, np.float64)
    bad = ta.CheckGradient(flipped.bind(data), x, check_H=False)
    assert not bad.ok.any() and float(bad.max_dist_g.min()) > bad.eps


# (K, d) of the fp32 cells of DESIGN section 22's register table whose kept static build shows no scratch: all six
@pytest.mark.parametrize("K,d", [(1, 50), (2, 6), (2, 25), (3, 21), (4, 3), (8, 2)])
def test_no_scratch(ta, K, d):
    st = model_of(ta, f"softmax{K}x{d}", gm.softmax_body(K, d), K * d, d + 1, K, np.float32).stats()
    print(f"softmax K = {K} n = {K * d} fp32 stats", st)
    assert st["scratch_bytes"] == 0 and st["num_regs"] > 0 and st["wg_per_cu"] >= 1 and st["lds_bytes_per_wg"] > 0


def test_refusals_through_the_c_abi(ta):
    K, d = 2, 1
    body, n = gm.softmax_body(K, d), 2
    res = model_of(ta, "softmax2x1", body, n, 2, K, np.float64)
    Pn = 3
    data = torch.zeros(Pn, 1, 2, dtype=torch.float64, device="cuda")
    model, xx = res.bind(data), cuda(np.tile([-1.2, 1.0], (Pn, 1)))
    ctx, lib, check = ta.api.default_context(), ta.api.default_context().lib, ta.api.check
    from tinyopt_amd import _capi
    C = ta.api.C
    h = C.c_void_p()
    KIND = "TOA_JIT_COST_GGN_MULTI"
    for field, val, text in (("num_params", 64, "1 <= num_params <= 63 .* not 64"), ("residuals_per_item", 9, "1 <= K <= 8 .* not 9"),
                             ("residuals_per_item", 0, "1 <= K <= 8"), ("manifold", 1, "Euclidean parameters only"),
                             ("diff", 2, "diff must be TOA_DIFF_DEFAULT"), ("large_n", 1, "large_n is for residual models")):
        spec = _capi.ToaJitSpec()
        spec.dtype, spec.num_params, spec.residuals_per_item, spec.scalars_per_item, spec.kind = 1, 2, 2, 2, 6
        setattr(spec, field, val)
        with pytest.raises(ta.ToaError, match=KIND + ".*" + text):
            check(lib.toa_model_compile_ex(ctx.h, C.byref(spec), body.encode(), C.byref(h), None, 0))
    spec = _capi.ToaJitSpec()
    spec.dtype, spec.num_params, spec.residuals_per_item, spec.scalars_per_item, spec.kind = 1, 2, 2, 2, 7
    with pytest.raises(ta.ToaError, match="kind must be .*TOA_JIT_COST_GGN or TOA_JIT_COST_GGN_MULTI"):
        check(lib.toa_model_compile_ex(ctx.h, C.byref(spec), body.encode(), C.byref(h), None, 0))
    out = ta.api._alloc_output(Pn, 2, ta.Options(), False, xx.device)
    rp = ta.api._results_pod(out)
    pod = ta.Options().to_pod()
    head = (ctx.h, res._h, 1, Pn, model.packed.data_ptr())
    x1 = xx.clone()
    g, H, c = (torch.zeros(Pn, 2, dtype=torch.float64, device="cuda"), torch.zeros(Pn, 2, 2, dtype=torch.float64, device="cuda"),
               torch.zeros(Pn, dtype=torch.float64, device="cuda"))
    check(lib.toa_set_loss(ctx.h, 1, 1.0))   # a handle with a loss set
    try:
        with pytest.raises(ta.ToaError, match=KIND + ".*no residuals to robustify"):
            check(lib.toa_jit_lm_run(*head, x1.data_ptr(), C.byref(pod), C.byref(rp), None))
        with pytest.raises(ta.ToaError, match=KIND + ".*no residuals to robustify"):
            check(lib.toa_jit_accumulate(*head, x1.data_ptr(), 1, g.data_ptr(), H.data_ptr(), c.data_ptr(), None))
    finally:
        check(lib.toa_set_loss(ctx.h, 0, 0.0))
    gdo = _capi.ToaGdOptions()
    lib.toa_gd_options_default(C.byref(gdo))
    pod_gd = ta.Options().to_pod()
    pod_gd.solver_type = 2
    with pytest.raises(ta.ToaError, match=KIND + ".*GradientDescent"):
        check(lib.toa_jit_gd_run(*head, x1.data_ptr(), C.byref(pod_gd), C.byref(gdo), C.byref(rp), None))
    with pytest.raises(ta.ToaError, match=KIND + ".*GradientDescent"):
        check(lib.toa_jit_lm_run(*head, x1.data_ptr(), C.byref(pod_gd), C.byref(rp), None))
    lbo = _capi.ToaLbfgsOptions()
    lib.toa_lbfgs_options_default(C.byref(lbo))
    pod_lb = ta.Options().to_pod()
    pod_lb.solver_type = 3
    with pytest.raises(ta.ToaError, match=KIND + ".*L-BFGS"):
        check(lib.toa_jit_lbfgs_run(*head, x1.data_ptr(), C.byref(pod_lb), C.byref(lbo), C.byref(rp), None))
    with pytest.raises(ta.ToaError, match=KIND + ".*L-BFGS"):
        check(lib.toa_jit_lm_run(*head, x1.data_ptr(), C.byref(pod_lb), C.byref(rp), None))
    with pytest.raises(ta.ToaError, match=KIND + ".*row-split"):
        check(lib.toa_jit_lm_run_split(*head, x1.data_ptr(), C.byref(pod), C.byref(rp), None, 2))
    state = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(ta.ToaError, match=KIND + ".*stepping form"):
        check(lib.toa_jit_lm_begin(*head, x1.data_ptr(), C.byref(pod), C.byref(rp), state.data_ptr()))
    with pytest.raises(ta.ToaError, match=KIND + ".*no residual rows"):
        check(lib.toa_jit_eval(*head, x1.data_ptr(), g.data_ptr(), None))
    bounds = _capi.ToaBounds()
    bounds.lo_dev, bounds.hi_dev = g.data_ptr(), g.data_ptr()
    with pytest.raises(ta.ToaError, match=KIND + ".*box bounds"):
        check(lib.toa_jit_lm_run_bounds(*head, x1.data_ptr(), C.byref(bounds), None, C.byref(pod), C.byref(rp), None))
    off = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device="cuda")
    with pytest.raises(ta.ToaError, match=KIND + ".*ragged batches"):
        check(lib.toa_jit_lm_run_ragged(ctx.h, res._h, off.data_ptr(), None, 1, 3, Pn, data.data_ptr(), x1.data_ptr(), C.byref(pod), C.byref(rp), None, 0))
    v = [C.c_int(0) for _ in range(3)]
    with pytest.raises(ta.ToaError, match=KIND + ".*ragged batches"):
        check(lib.toa_jit_model_stats_ragged(ctx.h, res._h, *[C.byref(t) for t in v]))
    with pytest.raises(ta.ToaError, match=KIND + ".*box bounds"):
        check(lib.toa_jit_model_stats_bounds(ctx.h, res._h, 0, 0, *[C.byref(t) for t in v]))
    sh = model_of(ta, "softmax shared 2x1", softmax_shared_body(K, d), n, 1, K, np.float64, kS=1)
    with pytest.raises(ta.ToaError, match="shared item table.*CheckGradient"):
        check(lib.toa_jit_check_gradient(ctx.h, sh._h, 1, Pn, data.data_ptr(), x1.data_ptr(), 0.0, 2, 0, c.data_ptr(), None))
    assert torch.equal(x1, xx)   # nothing ran
    check(lib.toa_jit_model_stats_prior(ctx.h, res._h, 0, *[C.byref(t) for t in v]))   # the prior form is served
    assert v[1].value > 0
    # H_dev may be NULL: g and the cost alone
    check(lib.toa_jit_accumulate(*head, x1.data_ptr(), 1, g.data_ptr(), None, c.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(g, ta.accumulate(model, xx)[0])
    with pytest.raises(ValueError, match="cost_ggn_multi.*no ragged batches"):
        res.bind_ragged(data.reshape(-1, 2), counts=[1, 1, 1])
    with pytest.raises(ValueError, match="cost_ggn_multi.*no box bounds"):
        model.with_bounds(None, None)
    with pytest.raises(ValueError, match="cost_ggn_multi.*no M-estimator"):
        model.with_loss("huber", 1.0)
