"""Shared item tables on the device (JitResidual(..., shared_scalars=kS)): a body reads row i of ONE table
[items, kS] as s[k] beside item i's own scalars, for every problem of the batch; RowModel::pass stages the rows by LDS-DMA next to the
private items.  Yardsticks, never the code under test: numpy in fp64 (tests/shared_reference.py, ggn_reference.py, the second reading
of the loop through bounds_reference.optimize_plain) and the REPLICATED twin — the same body text with s[k] rewritten to p[kD + k],
bound to data in which the table is copied into every problem, a path the library had before tables.  Every test here compiles a body
that names `s`, so every one of them fails on a library that does not know the spec field."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_reference as br  # noqa: E402
import ggn_reference as gr  # noqa: E402
import shared_reference as sr  # noqa: E402
from parity import check_trajectories, gpu_dict  # noqa: E402
from shared_cells import CELLS, trajectory_cases  # noqa: E402
from test_gpu_ggn import _check_problem, ref_dict  # noqa: E402

pytestmark = pytest.mark.gpu
TDT = {np.float32: torch.float32, np.float64: torch.float64}
EPS = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}   # the unit round-off
P = 97
H6 = 2.0 ** -6
_MODELS = {}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pair_of(ta, body, n, kD, kS, dtype, kind, kR=1, **kw):
    """(the shared model, its replicated twin): one compile each per text for the whole module."""
    key = (body, n, kD, kS, dtype, kind, kR, tuple(sorted(kw.items())))
    if key not in _MODELS:
        args = dict(n=n, residuals_per_item=kR, kind=kind, dtype=TDT[dtype], **kw)
        _MODELS[key] = (ta.JitResidual(body, item_scalars=kD, shared_scalars=kS, **args),
                        ta.JitResidual(sr.replicate(body, kD), item_scalars=kD + kS, **args))
    return _MODELS[key]


def bind_pair(pair, data, table, dtype):
    """Both forms bound to the same problem: the shared model to (data, table), the twin to the table copied behind every item."""
    shared, twin = pair
    return (shared.bind(cuda(data.astype(dtype)), shared=cuda(table.astype(dtype))), twin.bind(cuda(sr.replicated_data(data, table).astype(dtype))))


# ---- 1. the sum, exactly -----------------------------------------------------------------------------------------------------------
# (kind, dtype, n, kR, kD, kS): every n of {1, 4, 13, 16, 50, 63}, every (kD, kS) of {(0, 3), (1, 1), (1, 5), (2, 4), (1, 51), (3, 130)}, both kinds
# in both dtypes.  kS * sizeof(T) no multiple of 16: (0, 3), (1, 1), (1, 5) in fp32, (1, 1), (1, 5), (1, 51) in fp64; a shared image of
# several 1 KiB pieces: every cell but kS * sizeof(T) <= 16 at 64 items; a last piece that is partial: kR = 2 with (1, 5) fp32 (32 rows
# of 48 bytes) and the cells where the table leaves fewer than 64 items — (1, 51) fp64, (3, 130); kD = 0; kR = 2 for "accumulate".
EXACT_CELLS = [
    ("accumulate", np.float32, 1, 1, 0, 3), ("accumulate", np.float32, 4, 2, 1, 5), ("accumulate", np.float64, 13, 1, 1, 1),
    ("accumulate", np.float32, 16, 2, 2, 4), ("accumulate", np.float64, 50, 1, 1, 51), ("accumulate", np.float32, 63, 1, 3, 130),
    ("accumulate", np.float64, 4, 2, 3, 130),
    ("cost_ggn", np.float32, 50, 1, 1, 51), ("cost_ggn", np.float64, 1, 1, 1, 1), ("cost_ggn", np.float32, 13, 1, 0, 3),
    ("cost_ggn", np.float64, 16, 1, 1, 5), ("cost_ggn", np.float32, 4, 1, 3, 130), ("cost_ggn", np.float64, 63, 1, 2, 4),
]


@pytest.mark.parametrize("kind,dtype,n,kR,kD,kS", EXACT_CELLS)
def test_the_sum_exactly(ta, kind, dtype, n, kR, kD, kS):
    """Dyadic private scalars and table rows (the row's first column counts the item: a row from the wrong item, from padding or from
    the private image changes the sum), magnitudes at which every product and every partial sum is exact in float32: accumulate's
    cost, g and H EQUAL numpy's and the replicated twin's, bit for bit, with and without the gradient, at every edge of the super-step
    of both passes (IT from the restated geometry WITH the shared image)."""
    pair = pair_of(ta, sr.exact_body(kind, n, kR, kD, kS), n, kD, kS, dtype, kind, kR)
    x = cuda(np.zeros((P, n), dtype))
    for items in sr.edge_counts(n, kD, kS, dtype, kR):
        data, table = sr.exact_case(kD, kS, items, P)
        c32, g32, H32, big = sr.exact_sums(kind, n, kR, data, table, np.float32)
        c64, g64, H64, _ = sr.exact_sums(kind, n, kR, data, table, np.float64, np.float32)
        assert big < 2 ** 24 and (c32 == c64).all() and (g32 == g64).all() and (H32 == H64).all(), "the case is not exact in float32"
        shared, twin = bind_pair(pair, data, table, dtype)
        g, H, c, nres = [t.cpu().numpy() for t in ta.accumulate(shared, x)]
        assert (c == c64).all(), (items, "cost")
        assert (g == g64.astype(dtype)).all(), (items, "g")
        assert (H == H64.astype(dtype)).all(), (items, "H")
        assert (nres == (1 if kind == "cost_ggn" else items * kR)).all()
        gt, Ht, ct, nt = [t.cpu().numpy() for t in ta.accumulate(twin, x)]
        assert np.array_equal(g, gt) and np.array_equal(H, Ht) and np.array_equal(c, ct) and np.array_equal(nres, nt), (items, "twin")
        g0, H0, c0, _ = ta.accumulate(shared, x, want_grad=False)
        assert g0 is None and H0 is None and (c0.cpu().numpy() == c64).all(), (items, "cost only")
        assert torch.equal(ta.accumulate(twin, x, want_grad=False)[2], c0)


# ---- 2. the sum, rounded -----------------------------------------------------------------------------------------------------------
GLMS = {   # name: (parts, shared body, n, items, ggn_reference's case generator)
    "logistic12": (gr.logistic_parts, sr.logistic_body(12), 12, 200, gr.logistic_case),
    "logistic50": (gr.logistic_parts, sr.logistic_body(50), 50, 200, gr.logistic_case),
    "poisson13": (gr.poisson_parts, sr.poisson_body(13), 13, 157, gr.poisson_case),
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(GLMS))
def test_the_sum_rounded_glm(ta, name, dtype):
    """Logistic and Poisson regression as kind="cost_ggn" on ONE design matrix (problem 0's X for all, per-problem targets and starts)
    against the fp64 restatement, entry by entry, by test_gpu_ggn.py's rule: a device value lies within 2 B of numpy's,
    B = eps (items + 6) sum_i |term_i|; the cost within items 2 eps sum |c_i|."""
    parts, body, n, items, case = GLMS[name]
    X, y, x0 = sr.glm_batch(case, n, items, P)
    X, y, x0 = X.astype(dtype), y.astype(dtype), x0.astype(dtype)
    res, _ = pair_of(ta, body, n, 1, n, dtype, "cost_ggn")
    g, H, c, nres = ta.accumulate(res.bind(cuda(y[:, :, None]), shared=cuda(X)), cuda(x0))
    g, H, c = g.cpu().numpy().astype(np.float64), H.cpu().numpy().astype(np.float64), c.cpu().numpy()
    data = sr.glm_data(X.astype(np.float64), y.astype(np.float64))
    eps, worst = EPS[dtype], dict(g=0.0, H=0.0, c=0.0)
    for p in range(P):
        ci, gs, hs, J = parts(x0[p].astype(np.float64), data[p], True)
        w = np.where(hs <= gr.WMIN[np.dtype(dtype)], gr.WMIN[np.dtype(dtype)], hs)
        tg, tH = gs[:, None] * J, w[:, None, None] * J[:, :, None] * J[:, None, :]
        Bg, BH = eps * (items + 6) * np.abs(tg).sum(axis=0), eps * (items + 6) * np.abs(tH).sum(axis=0)
        Bc = items * 2.0 * eps * np.abs(ci).sum()
        worst["g"] = max(worst["g"], float((np.abs(g[p] - tg.sum(axis=0)) / Bg).max()))
        worst["H"] = max(worst["H"], float((np.abs(H[p] - tH.sum(axis=0)) / BH).max()))
        worst["c"] = max(worst["c"], float(abs(c[p] - ci.sum()) / Bc))
    print(name, np.dtype(dtype).name, "shared X: worst ratio to B: g %.3f H %.3f, cost to its bound %.4f" % (worst["g"], worst["H"], worst["c"]))
    assert worst["g"] <= 2.0 and worst["H"] <= 2.0 and worst["c"] <= 1.0, worst
    assert (nres.cpu().numpy() == 1).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_sum_rounded_linear_residual(ta, dtype):
    """r_i = s_i . x - p_i on a shared design, differentiated on the device (Jets), n = 12, 200 items, against fp64 numpy by the same
    rule as the GLMs: a device value of g and H lies within 2 B, B = eps (items + 6) sum_i |term_i| with the terms J_ia r_i and
    J_ia J_ib, and the cost within items 2 eps sum_i r_i^2.  Printed beside them, not asserted: the ratio of g to the bound that
    follows the residual's own rounding (r_i is a rounded sum of n + 1 terms, |delta r_i| <= (n + 1) eps R_i, R_i = sum_j |s_ij x_j| +
    |p_i|):  eps (items + n + 7) sum_i |J_ia| R_i."""
    n, items = 12, 200
    rng = np.random.default_rng(77)
    X = (rng.normal(size=(items, n)) / np.sqrt(n)).astype(dtype)
    y = rng.normal(size=(P, items)).astype(dtype)
    x0 = rng.normal(size=(P, n)).astype(dtype)
    res, twin = pair_of(ta, sr.linear_body(n), n, 1, n, dtype, "residual")
    g, H, c, nres = [t.cpu().numpy().astype(np.float64) for t in ta.accumulate(res.bind(cuda(y[:, :, None]), shared=cuda(X)), cuda(x0))]
    X64, eps, worst = X.astype(np.float64), EPS[dtype], dict(g=0.0, H=0.0, c=0.0, g_refined=0.0)
    BH = eps * (items + 6) * np.einsum("ia,ib->ab", np.abs(X64), np.abs(X64))
    for p in range(P):
        xp, yp = x0[p].astype(np.float64), y[p].astype(np.float64)
        r = X64 @ xp - yp
        R = np.abs(X64) @ np.abs(xp) + np.abs(yp)
        Bg = eps * (items + 6) * (np.abs(X64) * np.abs(r)[:, None]).sum(axis=0)
        Bc = items * 2.0 * eps * (r * r).sum()
        worst["g"] = max(worst["g"], float((np.abs(g[p] - X64.T @ r) / Bg).max()))
        worst["H"] = max(worst["H"], float((np.abs(H[p] - X64.T @ X64) / BH).max()))
        worst["c"] = max(worst["c"], float(abs(c[p] - (r * r).sum()) / Bc))
        worst["g_refined"] = max(worst["g_refined"], float((np.abs(g[p] - X64.T @ r) / (eps * (items + n + 7) * (np.abs(X64) * R[:, None]).sum(axis=0))).max()))
    print("linear residual (AD)", np.dtype(dtype).name, "shared X: worst ratio to B: g %.3f H %.3f, cost to its bound %.4f; g to the refined bound %.3f" %
          (worst["g"], worst["H"], worst["c"], worst["g_refined"]))
    assert worst["g"] <= 2.0 and worst["H"] <= 2.0 and worst["c"] <= 1.0, worst
    assert (nres == items).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [3, 20])
def test_numeric_differences_exactly(ta, n, dtype):
    """diff="forward", "central" and "fast_central" with h = 2^-6 on the shared-design linear residual, every scalar a multiple of 1/8
    (a linear residual: forward differences are exact too): the bound of
    tests/test_gpu_num_diff.py's exact case — the numeric model's (g, H, cost, nres) are BIT-identical to those of the body with the
    hand-written row, to the Jets', to the replicated twin's, and to numpy's."""
    items = 70
    rng = np.random.default_rng(100 * n)
    X = rng.integers(-16, 17, (items, n)) / 8.0
    y = rng.integers(-16, 17, (3, items)) / 8.0
    x = rng.integers(-4, 5, (3, n)) / 8.0
    r = x @ X.T - y
    want = (np.einsum("pi,ia->pa", r, X), np.broadcast_to(X.T @ X, (3, n, n)), (r * r).sum(axis=1))
    assert max(np.abs(want[0]).max(), np.abs(want[1]).max(), want[2].max()) * 4096 < 2 ** 24   # (units of 2^-12: exact in float32 in any order)
    got = {}
    for label, body, kind, kw in (("forward", sr.linear_body(n), "residual", dict(diff="forward", diff_h=H6)),
                                  ("central", sr.linear_body(n), "residual", dict(diff="central", diff_h=H6)),
                                  ("fast_central", sr.linear_body(n), "residual", dict(diff="fast_central", diff_h=H6)),
                                  ("jets", sr.linear_body(n), "residual", {}), ("own row", sr.linear_body(n, "accumulate"), "accumulate", {})):
        for form, model in zip(("shared", "twin"), bind_pair(pair_of(ta, body, n, 1, n, dtype, kind, **kw), y[:, :, None], X, dtype)):
            got[(label, form)] = [t.cpu().numpy() for t in ta.accumulate(model, cuda(x.astype(dtype)))]
    for key, (g, H, c, nres) in got.items():
        assert np.array_equal(g, want[0].astype(dtype)) and np.array_equal(H, want[1].astype(dtype)) and np.array_equal(c, want[2]), key
        assert (nres == items).all()


# ---- 3. trajectories, fp64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,optname", CELLS)
def test_trajectories(ta, problem, optname):
    """fp64 solves from far starts against the second reading of the loop under parity.check_trajectories, six problems per cell that
    share one table (shared_cells.py: seeds chosen on the CPU so that no accept / reject decision of the yardstick is closer than 1e-9
    to flipping; at least two problems per cell reject a step).  The only admitted parting is a proven roll-back tie."""
    cell = trajectory_cases(problem, optname)
    o, _ = gr.options_pair(ta.Options, **cell["options"])
    res, _ = pair_of(ta, cell["body"], cell["n"], 1, cell["kS"], np.float64, cell["kind"])
    x = cuda(cell["x0"].copy())
    out = ta.Optimize(x, res.bind(cuda(cell["data"]), shared=cuda(cell["table"])), o, history=True)
    torch.cuda.synchronize()
    refs = cell["refs"]
    got, ref = gpu_dict(out, x), ref_dict(refs, out.errs.shape[1])
    verdicts = [_check_problem(got, ref, p, o.to_pod(), f"{problem} {optname}") for p in range(len(refs))]
    print(problem, optname, {v: verdicts.count(v) for v in sorted(set(verdicts))}, "stops", [r["stop"] for r in refs], "device", got["stop"].tolist(),
          "iterations", [r["num_iters"] for r in refs], "failures", [r["num_failures"] for r in refs])
    assert set(verdicts) <= {"full", "tie", "roll-back tie"}
    assert all(v != "roll-back tie" for v, r in zip(verdicts, refs) if all(r["successes"]))
    if cell["rejects"]:   # (a linear least-squares problem rejects no step)
        assert sum(1 for r in refs if not all(r["successes"])) >= 2, "the cell's coverage of rejected steps"
    want_nres = 1 if cell["kind"] == "cost_ggn" else cell["data"].shape[1]
    assert (out.final_num_residuals.cpu().numpy() == want_nres).all()


# ---- 4. against the replicated twin, whole solves ------------------------------------------------------------------------------------
def _same_fate(a, b, p):
    return (int(a.stop_reason[p]) == int(b.stop_reason[p]) and int(a.num_iters[p]) == int(b.num_iters[p]) and torch.equal(a.successes[p], b.successes[p]))


def test_whole_solves_against_the_twin_logistic(ta):
    """The 97 logistic problems at n = 12 on one design matrix (min_rerr_dec = 1e-6, as test_gpu_ggn.py's sibling test) through both
    forms: per problem the same StopReason, iteration count and accept flags, final costs within the cost bound of the rounded sums.
    A problem may part only at a decision the restatement took within 2 B of flipping; cap: 5 % of the 97."""
    n, items = 12, 200
    X, y, x0 = sr.glm_batch(gr.logistic_case, n, items, P)
    data = sr.glm_data(X, y)
    o, ropt = gr.options_pair(ta.Options, min_rerr_dec=1e-6)
    shared, twin = bind_pair(pair_of(ta, sr.logistic_body(n), n, 1, n, np.float64, "cost_ggn"), y[:, :, None], X, np.float64)
    xs, xt = cuda(x0.copy()), cuda(x0.copy())
    a, b = ta.Optimize(xs, shared, o, history=True), ta.Optimize(xt, twin, o, history=True)
    torch.cuda.synchronize()
    parted = 0
    for p in range(P):
        if _same_fate(a, b, p):
            ci = gr.logistic_parts(xs[p].cpu().numpy(), data[p], False)[0]
            assert abs(float(a.final_cost[p]) - float(b.final_cost[p])) <= 2 * items * 2.0 ** -52 * np.abs(ci).sum(), p
            continue
        r = gr.optimize(gr.logistic_parts, data[p], x0[p], ropt)
        B = 2.0 ** -53 * (items + 6) * np.abs(gr.logistic_parts(np.array(r["x"]), data[p], False)[0]).sum() / max(r["final_cost"], 1e-300)
        assert r["min_margin"] <= 2 * B, (p, "parted away from a tie", r["min_margin"], B)
        parted += 1
    print("shared against replicated, logistic n = 12: parted", parted, "of", P)
    assert parted <= 0.05 * P and (a.stop_reason >= 0).all()


def test_whole_solves_against_the_twin_linear(ta):
    """The shared-design linear residual (Jets, n = 50, 130 items, fp64) through both forms: same StopReason, iteration count and accept
    flags, and the same x to 1e-9 of its scale; cap on problems whose fates part: 5 %."""
    n, items = 50, 130
    rng = np.random.default_rng(78)
    X, y, x0 = rng.normal(size=(items, n)) / np.sqrt(n), rng.normal(size=(P, items)), rng.normal(size=(P, n)) * 3.0
    shared, twin = bind_pair(pair_of(ta, sr.linear_body(n), n, 1, n, np.float64, "residual"), y[:, :, None], X, np.float64)
    xs, xt = cuda(x0.copy()), cuda(x0.copy())
    a, b = ta.Optimize(xs, shared, ta.Options(), history=True), ta.Optimize(xt, twin, ta.Options(), history=True)
    torch.cuda.synchronize()
    parted = sum(0 if _same_fate(a, b, p) else 1 for p in range(P))
    xbest = np.linalg.lstsq(X, y.T, rcond=None)[0].T
    print("shared against replicated, linear n = 50: parted", parted, "of", P, "max |x - lstsq|", float(np.abs(xs.cpu().numpy() - xbest).max()))
    assert parted <= 0.05 * P and (a.stop_reason >= 0).all()
    assert np.allclose(xs.cpu().numpy(), xt.cpu().numpy(), rtol=0, atol=1e-9 * np.abs(xbest).max())
    assert np.allclose(xs.cpu().numpy(), xbest, rtol=0, atol=1e-7 * np.abs(xbest).max())


# ---- 5. composition and edges ---------------------------------------------------------------------------------------------------------
def _decay_batch(Pn=P, items=45, seed=5):
    """A curve fit per pixel over ONE time axis: y = A exp(-k t) + b + noise; starts off the truth."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 4.0, items)
    truth = np.stack([rng.uniform(1.0, 3.0, Pn), rng.uniform(0.4, 1.5, Pn), rng.uniform(-0.5, 0.5, Pn)], axis=1)
    y = truth[:, 0:1] * np.exp(-truth[:, 1:2] * t[None]) + truth[:, 2:3] + 0.01 * rng.normal(size=(Pn, items))
    return t[:, None].copy(), y, truth * rng.uniform(0.8, 1.25, truth.shape), truth


@pytest.mark.parametrize("what", ["huber", "prior_diag", "prior_full", "bounds", "prior+bounds"])
def test_composition_against_the_twin(ta, what):
    """with_loss / with_prior / with_bounds carry the table along: the decay fit (a `residual` model, n = 3, fp64) under each against
    its replicated twin — the same arithmetic on the same numbers, so the same StopReason and iteration count and the same x to 1e-9
    (the two forms differ at most in the order of the Gram's sums).  With bounds that bind every x is inside the box exactly."""
    t, y, x0, truth = _decay_batch()
    shared, twin = bind_pair(pair_of(ta, sr.DECAY_BODY, 3, 1, 1, np.float64, "residual"), y[:, :, None], t, np.float64)
    rng = np.random.default_rng(9)
    mu, Wd = cuda(truth + 0.05), cuda(np.full((P, 3), 2.0))
    Wf = cuda(rng.normal(size=(P, 2, 3)))
    lo, hi = truth - 1.0, truth + 1.0
    lo[:, 1] = truth[:, 1] + 0.05          # the rate's bound binds: the optimum lies below it
    hi[::2, 0] = truth[::2, 0] - 0.1       # ... and every other amplitude's
    lo[1::3, 2] = hi[1::3, 2] = 0.0        # ... and every third offset is fixed
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    o = ta.Options()
    o.max_consec_failures = 30

    def dress(m):
        if what == "huber":
            return m.with_loss("huber", 0.02)
        if what == "prior_diag":
            return m.with_prior(mu, Wd)
        if what == "prior_full":
            return m.with_prior(mu, Wf)
        if what == "bounds":
            return m.with_bounds(cuda(lo), cuda(hi))
        return m.with_prior(mu, Wd).with_bounds(cuda(lo), cuda(hi))
    xs, xt = cuda(x0.copy()), cuda(x0.copy())
    a, b = ta.Optimize(xs, dress(shared), o), ta.Optimize(xt, dress(twin), o)
    torch.cuda.synchronize()
    same = (a.stop_reason == b.stop_reason) & (a.num_iters == b.num_iters)
    print(what, "same fate", int(same.sum()), "of", P, "stops", sorted(set(a.stop_reason.tolist())), "max |dx|", float((xs - xt).abs().max()))
    # (inside a box that binds, clip-and-reject can stall at different points of a flat valley when a last bit differs — DESIGN section
    #  16 —, and the two forms are two compilations of the body: the fates may part, in at most 5 % of the problems)
    assert int(same.sum()) >= 0.95 * P and (a.stop_reason >= 0).all() and (b.stop_reason >= 0).all()
    assert "bounds" in what or bool(same.all())
    assert torch.allclose(xs[same], xt[same], rtol=0, atol=1e-9 * 3.0)
    assert torch.allclose(a.final_cost[same], b.final_cost[same], rtol=1e-9, atol=1e-15)
    assert torch.equal(a.final_num_residuals, b.final_num_residuals)
    if "bounds" in what:
        for xn in (xs.cpu().numpy(), xt.cpu().numpy()):
            assert (xn >= lo).all() and (xn <= hi).all() and (xn[1::3, 2] == 0.0).all() and (xn[:, 1] == lo[:, 1]).mean() > 0.5
    if what == "huber":
        assert torch.equal(a.final_inlier_ratio, b.final_inlier_ratio) and float(a.final_inlier_ratio.min()) < 1.0
    # the seam carries the table too: accumulate of both dressed forms at the solution
    ga, gb = ta.accumulate(dress(shared), xs), ta.accumulate(dress(twin), xs)
    for u, v in zip(ga, gb):
        assert torch.allclose(u.to(torch.float64), v.to(torch.float64), rtol=1e-9, atol=1e-9)


def test_more_problems_than_waves_permuted_and_repeated(ta):
    n, items = 12, 40
    res, _ = pair_of(ta, sr.logistic_body(n), n, 1, n, np.float32, "cost_ggn")
    waves = 4 * torch.cuda.get_device_properties(0).multi_processor_count * res.stats()["wg_per_cu"]
    Pbig = waves + 501
    X, y, x0 = sr.glm_batch(gr.logistic_case, n, items, 64)
    pick = np.arange(Pbig) % 64
    data, x0 = y[pick][:, :, None].astype(np.float32), x0[pick].astype(np.float32)
    table = cuda(X.astype(np.float32))
    o = ta.Options()
    x = cuda(x0.copy())
    out = ta.Optimize(x, res.bind(cuda(data), shared=table), o)
    assert int(out.counters[3]) == Pbig
    x2 = cuda(x0.copy())
    out2 = ta.Optimize(x2, res.bind(cuda(data), shared=table), o)
    assert torch.equal(x, x2) and torch.equal(out.final_cost, out2.final_cost)   # repeated
    perm = np.random.default_rng(5).permutation(Pbig)
    xp = cuda(x0[perm].copy())
    outp = ta.Optimize(xp, res.bind(cuda(data[perm]), shared=table), o)
    torch.cuda.synchronize()
    pt = torch.from_numpy(perm).cuda()
    assert torch.equal(xp, x[pt]) and torch.equal(outp.final_cost, out.final_cost[pt]) and torch.equal(outp.num_iters, out.num_iters[pt])
    assert torch.equal(outp.stop_reason, out.stop_reason[pt]) and torch.equal(x[:64], x[64:128]) and (out.stop_reason >= 0).all()


def test_a_nan_in_a_table_row_ends_every_problem(ta):
    t, y, x0, _ = _decay_batch(Pn=9)
    t[41, 0] = float("nan")
    res, _ = pair_of(ta, sr.DECAY_BODY, 3, 1, 1, np.float64, "residual")
    x = cuda(x0.copy())
    out = ta.Optimize(x, res.bind(cuda(y[:, :, None]), shared=cuda(t)), ta.Options())
    torch.cuda.synchronize()
    assert (out.stop_reason == int(ta.StopReason.kSystemHasNaNOrInf)).all() and torch.equal(x, cuda(x0))


def test_final_hessian_save_last_and_covariance(ta):
    t, y, x0, _ = _decay_batch(Pn=7)
    res, _ = pair_of(ta, sr.DECAY_BODY, 3, 1, 1, np.float64, "residual")
    model = res.bind(cuda(y[:, :, None]), shared=cuda(t))
    og = ta.Options()
    og.solver_type, og.max_iters = ta.Options.GaussNewton, 0   # one pass that builds at x0 and nowhere else
    xg = cuda(x0.copy())
    outg = ta.Optimize(xg, model, og)
    assert torch.equal(outg.final_hessian, ta.accumulate(model, cuda(x0.copy()))[1])
    x = cuda(x0.copy())
    out = ta.Optimize(x, model, ta.Options())
    H = ta.accumulate(model, x)[1]
    cov, ok = out.Covariance()
    torch.cuda.synchronize()
    assert bool((ok != 0).all())
    assert torch.allclose(out.final_hessian, H, rtol=1e-6, atol=0) and torch.allclose(cov @ out.final_hessian, torch.eye(3, dtype=torch.float64, device="cuda").expand(7, 3, 3), atol=1e-8)
    ob = ta.Options.benchmark()                                # save_last off: no Hessian comes back
    assert ta.Optimize(cuda(x0.copy()), model, ob).final_hessian is None
    x1 = cuda(x0[2:3].copy())                                   # a problem solved alone equals its row in the batch, bit for bit
    out1 = ta.Optimize(x1, res.bind(cuda(y[2:3, :, None]), shared=cuda(t)), ta.Options())
    assert torch.equal(x1[0], x[2]) and out1.final_cost[0] == out.final_cost[2] and torch.equal(out1.final_hessian[0], out.final_hessian[2])


def test_no_scratch_with_the_table(ta):
    for n in (12, 50):
        st = pair_of(ta, sr.logistic_body(n), n, 1, n, np.float32, "cost_ggn")[0].stats()
        print(f"logistic n = {n} fp32, shared X: stats", st)
        assert st["scratch_bytes"] == 0 and st["num_regs"] > 0 and st["wg_per_cu"] >= 1 and st["lds_bytes_per_wg"] > 0


def test_refusals_through_the_c_abi(ta):
    from tinyopt_amd import _capi
    C = ta.api.C
    ctx, check = ta.api.default_context(), ta.api.check
    lib = ctx.lib
    t, y, x0, _ = _decay_batch(Pn=3, items=8)
    res, twin = pair_of(ta, sr.DECAY_BODY, 3, 1, 1, np.float64, "residual")
    table, data, xx = cuda(t), cuda(y[:, :, None]), cuda(x0.copy())
    x1 = xx.clone()
    out = ta.api._alloc_output(3, 3, ta.Options(), False, xx.device)
    rp, pod = ta.api._results_pod(out), ta.Options().to_pod()
    g, H, c = (torch.zeros(3, 3, dtype=torch.float64, device="cuda"), torch.zeros(3, 3, 3, dtype=torch.float64, device="cuda"),
               torch.zeros(3, dtype=torch.float64, device="cuda"))
    sh = _capi.ToaShared()
    sh.table_dev, sh.rows = table.data_ptr(), 8
    head = (ctx.h, res._h, 8, 3, data.data_ptr())
    run = (x1.data_ptr(), None, None, C.byref(pod), C.byref(rp), None)
    acc = (x1.data_ptr(), None, None, 1, g.data_ptr(), H.data_ptr(), c.data_ptr(), None)
    # the table itself
    for rows in (7, 9, 0):
        bad = _capi.ToaShared()
        bad.table_dev, bad.rows = table.data_ptr(), rows
        with pytest.raises(ta.ToaError, match=f"tinyopt_amd error -1: toa_jit_lm_run_shared: the shared table has one row per item: rows must be num_items = 8, not {rows}"):
            check(lib.toa_jit_lm_run_shared(*head, C.byref(bad), *run))
        with pytest.raises(ta.ToaError, match="toa_jit_accumulate_shared: the shared table has one row per item"):
            check(lib.toa_jit_accumulate_shared(*head, C.byref(bad), *acc))
    null = _capi.ToaShared()
    null.rows = 8
    with pytest.raises(ta.ToaError, match="error -1: toa_jit_lm_run_shared: null shared table_dev"):
        check(lib.toa_jit_lm_run_shared(*head, C.byref(null), *run))
    with pytest.raises(ta.ToaError, match="error -1: toa_jit_accumulate_shared: null shared$"):
        check(lib.toa_jit_accumulate_shared(*head, None, *acc))
    # a shared model at each old entry
    only = "a model with a shared item table .* toa_jit_lm_run_shared and toa_jit_accumulate_shared only"
    old = x1.data_ptr()
    prior, bounds = _capi.ToaPrior(), _capi.ToaBounds()
    prior.mu_dev, prior.W_dev, bounds.lo_dev, bounds.hi_dev = g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr()
    off = torch.tensor([0, 2, 5, 8], dtype=torch.int64, device="cuda")
    rag = (ctx.h, res._h, off.data_ptr(), None, 3, 8, 3, data.data_ptr())
    gdo, lbo = _capi.ToaGdOptions(), _capi.ToaLbfgsOptions()
    lib.toa_gd_options_default(C.byref(gdo))
    lib.toa_lbfgs_options_default(C.byref(lbo))
    state = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    v = [C.c_int(0) for _ in range(3)]
    calls = {
        "toa_jit_lm_run": lambda: lib.toa_jit_lm_run(*head, old, C.byref(pod), C.byref(rp), None),
        "toa_jit_lm_run_prior": lambda: lib.toa_jit_lm_run_prior(*head, old, C.byref(prior), C.byref(pod), C.byref(rp), None),
        "toa_jit_lm_run_bounds": lambda: lib.toa_jit_lm_run_bounds(*head, old, C.byref(bounds), None, C.byref(pod), C.byref(rp), None),
        "toa_jit_lm_run_ragged": lambda: lib.toa_jit_lm_run_ragged(*rag, old, C.byref(pod), C.byref(rp), None, 0),
        "toa_jit_lm_run_ragged_prior": lambda: lib.toa_jit_lm_run_ragged_prior(*rag, old, C.byref(prior), C.byref(pod), C.byref(rp), None, 0),
        "toa_jit_lm_run_ragged_bounds": lambda: lib.toa_jit_lm_run_ragged_bounds(*rag, old, C.byref(bounds), None, C.byref(pod), C.byref(rp), None, 0),
        "toa_jit_lm_run_split": lambda: lib.toa_jit_lm_run_split(*head, old, C.byref(pod), C.byref(rp), None, 2),
        "toa_jit_lm_begin": lambda: lib.toa_jit_lm_begin(*head, old, C.byref(pod), C.byref(rp), state.data_ptr()),
        "toa_jit_lm_step": lambda: lib.toa_jit_lm_step(*head, old, C.byref(pod), C.byref(rp), None, state.data_ptr(), None),
        "toa_jit_lm_stop": lambda: lib.toa_jit_lm_stop(*head, old, C.byref(pod), C.byref(rp), None, state.data_ptr(), state.data_ptr()),
        "toa_jit_gd_run": lambda: lib.toa_jit_gd_run(*head, old, C.byref(pod), C.byref(gdo), C.byref(rp), None),
        "toa_jit_gd_run_ragged": lambda: lib.toa_jit_gd_run_ragged(*rag, old, C.byref(pod), C.byref(gdo), C.byref(rp), None, 0),
        "toa_jit_lbfgs_run": lambda: lib.toa_jit_lbfgs_run(*head, old, C.byref(pod), C.byref(lbo), C.byref(rp), None),
        "toa_jit_lbfgs_run_ragged": lambda: lib.toa_jit_lbfgs_run_ragged(*rag, old, C.byref(pod), C.byref(lbo), C.byref(rp), None, 0),
        "toa_jit_accumulate": lambda: lib.toa_jit_accumulate(*head, old, 1, g.data_ptr(), H.data_ptr(), c.data_ptr(), None),
        "toa_jit_accumulate_prior": lambda: lib.toa_jit_accumulate_prior(*head, old, C.byref(prior), 1, g.data_ptr(), H.data_ptr(), c.data_ptr(), None),
        "toa_jit_accumulate_bounds": lambda: lib.toa_jit_accumulate_bounds(*head, old, C.byref(bounds), None, 1, g.data_ptr(), H.data_ptr(), c.data_ptr(), None),
        "toa_jit_accumulate_ragged": lambda: lib.toa_jit_accumulate_ragged(*rag, old, 1, g.data_ptr(), H.data_ptr(), c.data_ptr(), None),
        "toa_jit_accumulate_ragged_prior": lambda: lib.toa_jit_accumulate_ragged_prior(*rag, old, C.byref(prior), 1, g.data_ptr(), H.data_ptr(), c.data_ptr(), None),
        "toa_jit_accumulate_ragged_bounds": lambda: lib.toa_jit_accumulate_ragged_bounds(*rag, old, C.byref(bounds), None, 1, g.data_ptr(), H.data_ptr(), c.data_ptr(), None),
        "toa_jit_eval": lambda: lib.toa_jit_eval(*head, old, c.data_ptr(), None),
        "toa_jit_eval_ragged": lambda: lib.toa_jit_eval_ragged(*rag, old, c.data_ptr(), None),
        "toa_jit_check_gradient": lambda: lib.toa_jit_check_gradient(*head, old, 0.0, 2, 1, c.data_ptr(), None),
        "toa_jit_model_stats_ragged": lambda: lib.toa_jit_model_stats_ragged(ctx.h, res._h, *[C.byref(t_) for t_ in v]),
    }
    for name, call in calls.items():
        who = "toa_jit_lm_begin / step / stop" if name in ("toa_jit_lm_begin", "toa_jit_lm_step", "toa_jit_lm_stop") else name
        with pytest.raises(ta.ToaError, match=f"tinyopt_amd error -4: {who}: {only}: "):
            check(call())
    # a plain model at the new entries
    headt = (ctx.h, twin._h, 8, 3, data.data_ptr())
    for call in (lambda: lib.toa_jit_lm_run_shared(*headt, C.byref(sh), *run), lambda: lib.toa_jit_accumulate_shared(*headt, C.byref(sh), *acc)):
        with pytest.raises(ta.ToaError, match=r"error -4: toa_jit_\w+_shared: the model has no shared item table \(toa_jit_spec::shared_scalars = 0\)"):
            check(call())
    # at compile time
    h = C.c_void_p()
    for field, val, text, code in (("kind", 2, "TOA_JIT_COST / TOA_JIT_COST_GRAD / TOA_JIT_COST_HESS do not", -4), ("kind", 3, "do not", -4),
                                   ("manifold", 1, "takes Euclidean parameters only", -4), ("large_n", 1, "not built for large_n models", -4),
                                   ("shared_scalars", 513, r"shared_scalars in \[0, 512\]", -1), ("shared_scalars", -1, r"shared_scalars in \[0, 512\]", -1)):
        spec = _capi.ToaJitSpec()
        spec.dtype, spec.num_params, spec.residuals_per_item, spec.scalars_per_item, spec.kind, spec.shared_scalars = 1, 6, 1, 1, 0, 2
        setattr(spec, field, val)
        with pytest.raises(ta.ToaError, match=f"error {code}: toa_model_compile: .*" + text):
            check(lib.toa_model_compile_ex(ctx.h, C.byref(spec), b"r[0] = s[0];", C.byref(h), None, 0))
    assert torch.equal(x1, xx)   # nothing ran
    # ... and the stats entries describe the builds as for any model; an empty batch is no error
    assert res.stats_prior()["num_regs"] > 0 and res.stats_bounds(with_prior=True)["num_regs"] > 0
    check(lib.toa_jit_lm_run_shared(ctx.h, res._h, 8, 0, None, C.byref(sh), None, None, None, C.byref(pod), C.byref(rp), None))
    check(lib.toa_jit_accumulate_shared(*head, C.byref(sh), *acc))
    torch.cuda.synchronize()
    assert torch.equal(g, ta.accumulate(res.bind(data, shared=table), xx)[0])


def test_items_without_private_scalars(ta):
    """item_scalars = 0 beside a table is legal: every problem evaluates the table alone (with its header)."""
    n, items, Pn = 4, 67, 5
    rng = np.random.default_rng(3)
    X = rng.integers(-8, 9, (items, n + 1)) / 4.0
    body = f"T z = -s[{n}] * h[0]; for (int j = 0; j < {n}; ++j) z += s[j] * x[j];\nr[0] = z;\nif (want_grad) {{ for (int a = 0; a < {n}; ++a) J[0][a] = s[a]; }}\n"
    res = ta.JitResidual(body, n=n, item_scalars=0, header_scalars=1, shared_scalars=n + 1, kind="accumulate", dtype=torch.float64)
    hdr = np.arange(1, Pn + 1, dtype=np.float64)[:, None]
    x = cuda(np.zeros((Pn, n)))
    model = res.bind(None, header=cuda(hdr), items=items, shared=cuda(X))
    g, H, c, nres = ta.accumulate(model, x)
    r = -X[None, :, n] * hdr
    assert np.array_equal(c.cpu().numpy(), (r * r).sum(axis=1)) and np.array_equal(g.cpu().numpy(), np.einsum("pi,ia->pa", r, X[:, :n]))
    assert np.array_equal(H.cpu().numpy(), np.broadcast_to(X[:, :n].T @ X[:, :n], (Pn, n, n))) and (nres.cpu().numpy() == items).all()
    out = ta.Optimize(x, model, ta.Options())
    torch.cuda.synchronize()
    want = np.linalg.lstsq(X[:, :n], X[:, n], rcond=None)[0][None] * hdr
    assert (out.stop_reason >= 0).all() and np.allclose(x.cpu().numpy(), want, atol=1e-9)
