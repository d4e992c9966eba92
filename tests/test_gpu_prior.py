"""Gaussian priors beside run-time models (JitModel.with_prior / RaggedJitModel.with_prior; toa_jit_*_prior, csrc/prior.hpp): per problem
r = W (x - mu) appended after the item pass.  Yardsticks: the seam of the same model without the prior plus the prior's W^T W, W^T r and
|r|^2 in numpy float64; the oracle's GaussianPrior / MahaPrior for batches without items; a tagged-item text model run by the plain
Optimize for data + prior; the uniform prior'd call for every problem of a ragged prior'd batch (bit for bit)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from parity import check_trajectories, gpu_dict  # noqa: E402
from test_gpu_jit import CIRCLE, SE3_PRIOR, SO2_PLUS, SO2_RESIDUAL  # noqa: E402
from test_gpu_ragged import OUT_FIELDS, SKIPPED, TDT, Case, _res, circle_case, circle_options  # noqa: E402
from test_gpu_row_models import ad_body, manual_body  # noqa: E402

pytestmark = pytest.mark.gpu

SEAM_TOL = {np.float64: 1e-10, np.float32: 1e-4}   # the project's seam tolerance, relative to max |H|, max |g| and the cost
ROW_N = 20


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def prior_np(mu, W, x):
    """The prior's contribution in float64: (W^T W [P, n, n], W^T r [P, n], |r|^2 [P], k)."""
    mu, W, x = (np.asarray(a, np.float64) for a in (mu, W, x))
    if W.ndim == 2:
        r = W * (x - mu)
        H = np.zeros(W.shape + (W.shape[1],))
        idx = np.arange(W.shape[1])
        H[:, idx, idx] = W * W
        return H, W * r, (r * r).sum(-1), W.shape[1]
    r = np.einsum("pkj,pj->pk", W, x - mu)
    return np.einsum("pki,pkj->pij", W, W), np.einsum("pkj,pk->pj", W, r), (r * r).sum(-1), W.shape[1]


def make_prior(rng, P, n, form, dtype, x, spread=0.3, scale=1.0):
    """form: "diag", or the number of rows of a full W.  mu = x + noise, so the residuals are neither zero nor huge."""
    mu = (np.asarray(x, np.float64) + spread * rng.uniform(-1, 1, (P, n))).astype(dtype)
    if form == "diag":
        W = (scale * rng.uniform(0.5, 2.0, (P, n))).astype(dtype)
    else:
        W = (scale * rng.uniform(-1, 1, (P, int(form), n))).astype(dtype)
    return mu, W


def assert_seam(ta, model, x, mu, W, dtype, items, kR=1, loss=None):
    """accumulate(model.with_prior) against accumulate(model) + the numpy prior, to the seam tolerance; nres exactly items kR + k."""
    base = model.with_loss(*loss) if loss else model
    pm = base.with_prior(cuda(mu), cuda(W))
    g0, H0, c0, n0 = ta.accumulate(base, x)
    g1, H1, c1, n1 = ta.accumulate(pm, x)
    _, _, c2, n2 = ta.accumulate(pm, x, want_grad=False)
    torch.cuda.synchronize()
    Hp, gp, cp, k = prior_np(mu, W, x.cpu().numpy())
    tol = SEAM_TOL[dtype]
    H1n, g1n, c1n = H1.cpu().numpy().astype(np.float64), g1.cpu().numpy().astype(np.float64), c1.cpu().numpy()
    eH = np.abs(H1n - (H0.cpu().numpy().astype(np.float64) + Hp)).max() / np.abs(H1n).max()
    eg = np.abs(g1n - (g0.cpu().numpy().astype(np.float64) + gp)).max() / np.abs(g1n).max()
    ec = (np.abs(c1n - (c0.cpu().numpy() + cp)) / np.abs(c1n)).max()
    ec2 = (np.abs(c2.cpu().numpy() - (c0.cpu().numpy() + cp)) / np.abs(c1n)).max()
    print(f"seam: H {eH:.2e} g {eg:.2e} cost {ec:.2e} cost-only {ec2:.2e} (tolerance {tol:g})")
    assert eH <= tol and eg <= tol and ec <= tol and ec2 <= tol
    assert np.array_equal(H1n, np.swapaxes(H1n, 1, 2)), "H is not symmetric bit for bit"
    want = items * kR + k
    assert bool((n0 == items * kR).all()) and bool((n1 == want).all()) and bool((n2 == want).all()), (n0, n1, n2, want)


# ---- 1. the seam: exact bookkeeping ------------------------------------------------------------------------------------------------
def circle_uniform(dtype, P=4, items=10):
    rng = np.random.default_rng(3)
    ang = np.linspace(0, 2 * np.pi, items, endpoint=False)[None] + rng.uniform(0, 1, (P, 1))
    pts = (np.stack([2 + 2 * np.cos(ang), 7 + 2 * np.sin(ang)], -1) + 1e-3 * rng.uniform(-1, 1, (P, items, 2))).astype(dtype)
    x = (np.array([2.0, 7.0, 2.0]) + 0.2 * rng.uniform(-1, 1, (P, 3))).astype(dtype)
    return pts, x


def forms_of(n):
    return ["diag", 1, n]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_seam_circle(ta, dtype):
    """JetModel: n = 3, 10 items."""
    pts, x = circle_uniform(dtype)
    model = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype]).bind(cuda(pts))
    rng = np.random.default_rng(21)
    for form in forms_of(3):
        mu, W = make_prior(rng, len(x), 3, form, dtype, x, scale=3.0)
        assert_seam(ta, model, cuda(x), mu, W, dtype, items=10)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["residual", "accumulate"])
def test_seam_dense_row_n20(ta, oracle, kind, dtype):
    """RowModel: the DenseRow residual as text, n = 20, both kinds, 65 items (one more than a super-step of 64 rows)."""
    P, m = 3, 65
    A, b, x0, _ = oracle.synth_dense_row(P, ROW_N, m, dtype, seed=77)
    body = manual_body(ROW_N) if kind == "accumulate" else ad_body(ROW_N)
    model = _res(ta, body, n=ROW_N, item_scalars=ROW_N + 1, dtype=TDT[dtype], kind=kind).bind(cuda(np.concatenate([A, b[..., None]], -1)))
    rng = np.random.default_rng(22)
    for form in forms_of(ROW_N):
        mu, W = make_prior(rng, P, ROW_N, form, dtype, x0, scale=2.0)
        assert_seam(ta, model, cuda(x0), mu, W, dtype, items=m)


def test_seam_last_lane_n63(ta, oracle):
    """n = 63 with k = 63 and 70 items, fp64: the last lane of the wave, the widest W."""
    P, n, m, dtype = 2, 63, 70, np.float64
    A, b, x0, _ = oracle.synth_dense_row(P, n, m, dtype, seed=78)
    model = _res(ta, manual_body(n), n=n, item_scalars=n + 1, dtype=TDT[dtype], kind="accumulate").bind(cuda(np.concatenate([A, b[..., None]], -1)))
    rng = np.random.default_rng(23)
    for form in forms_of(n):
        mu, W = make_prior(rng, P, n, form, dtype, x0, scale=2.0)
        assert_seam(ta, model, cuda(x0), mu, W, dtype, items=m)


# ---- 2. the prior is not robustified ----------------------------------------------------------------------------------------------
def test_prior_is_not_robustified(ta, oracle):
    """n = 20 with a Huber loss and gross outliers: (prior + loss) - (loss) is the plain prior, and the k prior residuals are inliers."""
    P, m, dtype, th = 3, 65, np.float64, 1.0
    A, _, _, _ = oracle.synth_dense_row(P, ROW_N, m, dtype, seed=79)
    rng = np.random.default_rng(79)
    xs = rng.uniform(-1, 1, (P, ROW_N))                 # planted: the clean rows fit to 1e-3, far inside the threshold
    t = np.einsum("pmj,pj->pm", A.astype(np.float64), xs)
    b = t + 0.1 * np.sin(t) + 1e-3 * rng.uniform(-1, 1, (P, m))
    x0 = xs + 0.05 * rng.uniform(-1, 1, (P, ROW_N))
    bad = np.zeros((P, m), bool)
    bad[:, ::22] = True
    b[bad] += 50.0                      # gross outliers, far outside it: three rows of 65
    model = _res(ta, manual_body(ROW_N), n=ROW_N, item_scalars=ROW_N + 1, dtype=TDT[dtype], kind="accumulate").bind(
        cuda(np.concatenate([A, b[..., None]], -1)))
    rng = np.random.default_rng(24)
    for form in forms_of(ROW_N):
        mu, W = make_prior(rng, P, ROW_N, form, dtype, x0, scale=2.0)
        assert_seam(ta, model, cuda(x0), mu, W, dtype, items=m, loss=("huber", th))
    # the inlier ratio of a solve: the items' inliers at the final x plus all k prior residuals, over items + k
    # (a full-rank prior about the planted point keeps the Huber pull of the outliers from biasing the fit: in a float64 IRLS of
    #  these inputs the clean rows end at r^2 <= 0.09 and start at <= 0.05, the outliers stay above 2 400 — nothing near th^2 = 1)
    k = ROW_N
    mu = xs + 1e-3 * rng.uniform(-1, 1, (P, ROW_N))
    W = 3.0 * np.eye(ROW_N)[None] + 0.3 * rng.uniform(-1, 1, (P, k, ROW_N))
    x = cuda(x0)
    out = ta.Optimize(x, model.with_loss("huber", th).with_prior(cuda(mu), cuda(W)), ta.Options())
    torch.cuda.synchronize()
    t = np.einsum("pmj,pj->pm", A, x.cpu().numpy())
    r2 = (t + 0.1 * np.sin(t) - b) ** 2
    assert not ((r2 > 0.5 * th * th) & (r2 < 2.0 * th * th)).any(), "an item sits on the threshold: the count would depend on the iterate"
    inl = (r2 <= th * th).sum(-1)
    assert bool((out.stop_reason >= 0).all()) and (inl == m - 3).all()
    assert np.array_equal(out.final_num_residuals.cpu().numpy(), np.full(P, m + k))
    assert np.array_equal(out.final_inlier_ratio.cpu().numpy(), ((inl + k).astype(np.float32) / np.float32(m + k)).astype(np.float32))


# ---- 3. a batch without items: the pure prior against the oracle ----------------------------------------------------------------------
def empty_ragged(ta, n, dtype, P):
    if n == 3:
        res = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype])
    else:   # (the DenseRow text with its own Jacobian: the model of the other tests of this n, whatever it is — it has no items here)
        res = _res(ta, manual_body(n), n=n, item_scalars=n + 1, dtype=TDT[dtype], kind="accumulate")
    return res.bind_ragged(torch.zeros(0, res.kD, dtype=TDT[dtype], device="cuda"), counts=[0] * P)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [3, 12, 50])
def test_pure_diagonal_prior_matches_oracle(ta, oracle, n, dtype):
    """Every problem has count 0; W = 1 / sigma: the oracle's GaussianPrior, whole trajectories at tests/parity.py's tolerances.  As in
    tests/test_gpu_models.py::test_gaussian_prior_matches_oracle this solve converges in one step, after which every cost is a sum of
    round-off residues: costs below eps x (first cost) are clamped onto one floor value on BOTH sides before the comparison.  The
    covariance (tests/cov.cpp:20-47, margin 1e-5) is checked in float64, the reference test's type."""
    P = 8
    y, sigma, x0 = oracle.synth_gaussian_prior(P, n, dtype, seed=5)
    o = ta.Options.benchmark()
    o.hessian.save_last = True
    ref = oracle.gaussian_prior_lm(y, sigma, x0, o.to_pod(), history=True)
    model = empty_ragged(ta, n, dtype, P).with_prior(cuda(y), cuda((1.0 / sigma).astype(dtype)))
    x = cuda(x0.copy())
    out = ta.Optimize(x, model, o, history=True)
    torch.cuda.synchronize()
    assert not bool((out.stop_reason == SKIPPED).any()) and bool((out.stop_reason >= 0).all())
    assert np.array_equal(out.final_num_residuals.cpu().numpy(), np.full(P, n))
    refd = dict(errs=ref["errs"].copy(), succ=ref["succ"], iters=ref["iters"], stop=ref["stop"], x=ref["x"],
                cost=ref["cost"].copy(), fails=ref["fails"], deltas2=ref["deltas2"])
    g = gpu_dict(out, x)
    scale = np.maximum(ref["errs"][:, :1], 1e-300)
    eps = 1e-15 if dtype == np.float64 else 1e-6
    for d in (g, refd):
        d["errs"] = np.where(d["errs"] / scale < eps, 0.0, d["errs"]) + eps * scale
        d["cost"] = np.where(d["cost"] / scale[:, 0] < eps, 0.0, d["cost"]) + eps * scale[:, 0]
    st = check_trajectories(g, refd, dtype, o.to_pod(), label=f"pure diagonal prior n={n}")
    assert st["full"] + st["ties"] == P, st
    if dtype == np.float64:
        C, ok = out.Covariance()
        Cn = C.cpu().numpy()
        want = np.zeros_like(Cn)
        idx = np.arange(n)
        want[:, idx, idx] = sigma.astype(np.float64) ** 2
        assert ok.cpu().numpy().all() and np.abs(Cn - want).max() < 1e-5


@pytest.mark.parametrize("n", [2, 6])
def test_pure_full_prior_matches_oracle(ta, oracle, n):
    """Every problem has count 0; W = U, the upper Cholesky factor of cov^-1 (tests/cov.cpp:96): the oracle's MahaPrior."""
    P, dtype = 6, np.float64
    rng = np.random.default_rng(8)
    A = rng.uniform(-1, 1, (P, n + 3, n))
    cov = np.einsum("pij,pik->pjk", A, A) + 0.5 * np.eye(n)
    y = rng.uniform(-2, 2, (P, n)).astype(dtype)
    data = oracle.maha_prior_data(y, cov)
    U = data[:, n:].reshape(P, n, n)
    x0 = np.zeros((P, n), dtype)
    o = ta.Options()
    ref = oracle.maha_prior_lm(data, x0, o.to_pod())
    model = empty_ragged(ta, n, dtype, P).with_prior(cuda(y), cuda(U))
    x = cuda(x0.copy())
    out = ta.Optimize(x, model, o)
    torch.cuda.synchronize()
    assert not bool((out.stop_reason == SKIPPED).any())
    assert np.abs(x.cpu().numpy() - ref["x"]).max() < 1e-8
    assert np.array_equal(out.stop_reason.cpu().numpy(), ref["stop"]) and np.array_equal(out.num_iters.cpu().numpy(), ref["iters"])
    assert np.allclose(out.final_hessian.cpu().numpy(), ref["H"], rtol=1e-9, atol=1e-12 * np.abs(ref["H"]).max())
    assert np.array_equal(out.final_num_residuals.cpu().numpy(), np.full(P, n))
    C, ok = out.Covariance()
    assert ok.cpu().numpy().all() and np.abs(C.cpu().numpy() - cov).max() < 1e-5    # the posterior covariance (tests/cov.cpp:96-110)


# ---- 4. data + prior against a tagged-item model run by the plain Optimize ---------------------------------------------------------
TAGGED = """
if (p[0] == T(0)) {
  const S dx = p[1] - x[0];
  const S dy = p[2] - x[1];
  r[0] = dx * dx + dy * dy - x[2] * x[2];
} else {
  r[0] = p[1] * (x[0] - p[4]) + p[2] * (x[1] - p[5]) + p[3] * (x[2] - p[6]);
}
"""


def test_data_and_prior_match_tagged_items(ta):
    """The circle batch of tests/test_gpu_ragged.py (its non-empty problems) with a full k = 3 prior of moderate weight, against the
    same rows smuggled into the item list behind a tag (item = [tag, 2 n scalars]): the two differ only in summation order."""
    dtype, n = np.float64, 3
    base = circle_case(dtype)
    keep = [p for p, c in enumerate(base.counts) if c > 0]
    items = [base.items[p] for p in keep]
    P = len(items)
    rng = np.random.default_rng(31)
    mu = (np.array([2.0, 7.0, 2.0]) + rng.uniform(0.2, 0.5, (P, n)) * rng.choice([-1.0, 1.0], (P, n))).astype(dtype)   # away from the data's optimum
    W = rng.uniform(-3, 3, (P, n, n)).astype(dtype)
    x0 = np.tile(np.array([0, 0, 1], dtype), (P, 1))
    tagged = []
    for p in range(P):
        pts = np.concatenate([np.zeros((len(items[p]), 1)), items[p], np.zeros((len(items[p]), 4))], -1)
        rows = np.concatenate([np.ones((n, 1)), W[p], np.tile(mu[p], (n, 1))], -1)
        tagged.append(np.concatenate([pts, rows], 0).astype(dtype))
    opts = circle_options(ta)
    ct = Case(tagged, x0)
    xt = ct.x()
    ot = ta.Optimize(xt, ct.ragged(_res(ta, TAGGED, n=n, item_scalars=1 + 2 * n, dtype=TDT[dtype])), opts, history=True)
    cp = Case(items, x0)
    xp = cp.x()
    op = ta.Optimize(xp, cp.ragged(_res(ta, CIRCLE, n=n, item_scalars=2, dtype=TDT[dtype])).with_prior(cuda(mu), cuda(W)), opts, history=True)
    torch.cuda.synchronize()
    gp, gt = gpu_dict(op, xp), gpu_dict(ot, xt)
    st = check_trajectories(gp, gt, dtype, opts.to_pod(), tol=dict(err_rtol=1e-9, cost_rtol=1e-9, x_tol=1e-8), label="prior vs tagged items")
    print("prior vs tagged items:", st, "iterations", gp["iters"].tolist())
    assert st["full"] == P and st["ties"] == 0, st                      # no problem is excused
    assert np.array_equal(gp["stop"], gt["stop"]) and np.array_equal(gp["iters"], gt["iters"])
    hs = gp["succ"].shape[1]
    live = np.arange(hs)[None] < gp["iters"][:, None]
    assert np.array_equal(gp["succ"] * live, gt["succ"] * live)         # the same accept / reject sequence
    assert np.abs(gp["x"] - gt["x"]).max() < 1e-8
    assert np.array_equal(op.final_num_residuals.cpu().numpy(), ot.final_num_residuals.cpu().numpy())
    assert (gp["cost"] > 1e-6).all(), "a cost reached the cancellation floor: move mu"


# ---- 5. uniform = ragged, bit for bit -----------------------------------------------------------------------------------------------
PRIOR_ROW_COUNTS = [1, 15, 16, 17, 63, 64, 65, 129]


def prior_row_case(oracle, dtype):
    items, x0 = [], []
    for p, cnt in enumerate(PRIOR_ROW_COUNTS):
        A, b, x, _ = oracle.synth_dense_row(1, ROW_N, cnt, dtype, seed=900 + p)
        items.append(np.concatenate([A[0], b[0][:, None]], -1))
        x0.append(x[0])
    return Case(items, np.stack(x0))


def assert_bit_equal_to_uniform_prior(ta, case, res, opts, x, out, mu, W, skip=()):
    for p, cnt in enumerate(case.counts):
        if cnt == 0 or p in skip:
            continue
        m1 = case.alone(res, p).with_prior(cuda(mu[p:p + 1]), cuda(W[p:p + 1]))
        x1 = case.x(p)
        o1 = ta.Optimize(x1, m1, opts, history=True)
        torch.cuda.synchronize()
        assert torch.equal(x[p], x1[0]), f"problem {p} ({cnt} items): x differs by {float((x[p] - x1[0]).abs().max())}"
        for f in OUT_FIELDS:
            a, b = getattr(out, f), getattr(o1, f)
            if a is None and b is None:
                continue
            assert torch.equal(a[p], b[0]), f"problem {p} ({cnt} items): {f} differs: {a[p]} vs {b[0]}"


def test_ragged_prior_is_bit_equal_to_uniform_prior(ta, oracle):
    """n = 20 rows at counts around every super-step size with a full k = 20 prior: every problem of the ragged run is the uniform
    prior'd run of that problem alone, bit for bit; the queue order changes nothing; the under-determined problems (count <= n),
    which the prior makes well posed, converge."""
    dtype = np.float64
    case = prior_row_case(oracle, dtype)
    res = _res(ta, manual_body(ROW_N), n=ROW_N, item_scalars=ROW_N + 1, dtype=TDT[dtype], kind="accumulate")
    rng = np.random.default_rng(41)
    mu, W = make_prior(rng, case.P, ROW_N, ROW_N, dtype, case.x0, spread=0.1, scale=1.0)
    W = (W + 2.0 * np.eye(ROW_N)[None]).astype(dtype)     # full rank: W^T W is positive definite
    opts = ta.Options()
    opts.hessian.save_last = True
    model = case.ragged(res).with_prior(cuda(mu), cuda(W))
    x = case.x()
    out = ta.Optimize(x, model, opts, history=True)
    xk = case.x()
    outk = ta.Optimize(xk, model, opts, history=True, keep_order=True)
    torch.cuda.synchronize()
    assert bool(out.Succeeded().all()), out.stop_reason
    assert np.array_equal(out.final_num_residuals.cpu().numpy(), np.array(PRIOR_ROW_COUNTS) + ROW_N)
    assert torch.equal(x, xk)
    for f in OUT_FIELDS:
        a, b = getattr(out, f), getattr(outk, f)
        assert (a is None and b is None) or torch.equal(a, b), f"keep_order=True: {f}"
    assert_bit_equal_to_uniform_prior(ta, case, res, opts, x, out, mu, W)


# ---- 6. an empty problem inside a mixed ragged batch ------------------------------------------------------------------------------
def test_empty_problem_in_a_mixed_batch(ta):
    dtype, n = np.float64, 3
    pts, xu = circle_uniform(dtype, P=2, items=65)
    case = Case([pts[0][:10], np.zeros((0, 2), dtype), pts[1]], np.stack([xu[0], np.array([0.0, 0.0, 1.0]), xu[1]]).astype(dtype))
    res = _res(ta, CIRCLE, n=n, item_scalars=2, dtype=TDT[dtype])
    rng = np.random.default_rng(51)
    mu, W = make_prior(rng, case.P, n, "diag", dtype, np.tile(np.array([2.0, 7.0, 2.0]), (3, 1)), spread=0.2, scale=1.0)
    opts = ta.Options()
    opts.solver_type = ta.Options.GaussNewton
    x = case.x()
    out = ta.Optimize(x, case.ragged(res).with_prior(cuda(mu), cuda(W)), opts, history=True)
    torch.cuda.synchronize()
    assert int(out.stop_reason[1]) >= 0 and int(out.stop_reason[1]) != SKIPPED
    assert float((x[1].cpu() - torch.from_numpy(mu[1])).abs().max()) < 1e-12      # one Gauss-Newton step lands on mu
    assert int(out.final_num_residuals[1]) == n and float(out.final_inlier_ratio[1]) == 1.0
    assert_bit_equal_to_uniform_prior(ta, case, res, opts, x, out, mu, W)          # its neighbours: their solo runs


# ---- 7. a numeric model -------------------------------------------------------------------------------------------------------------
def test_numeric_model_with_prior(ta):
    """diff="central" wraps the same templates: the circle fit with a full prior, beside its AD twin.  Bound as in
    tests/test_gpu_num_diff.py::test_solve_with_central_differences: every problem succeeds and the two land within 5e-3."""
    dtype, n = np.float64, 3
    pts, x0 = circle_uniform(dtype, P=5, items=40)
    rng = np.random.default_rng(61)
    mu, W = make_prior(rng, 5, n, n, dtype, np.tile(np.array([2.0, 7.0, 2.0]), (5, 1)), spread=0.2, scale=2.0)
    xs, iters = {}, {}
    for diff in ("central", "ad"):
        model = _res(ta, CIRCLE, n=n, item_scalars=2, dtype=TDT[dtype], diff=diff).bind(cuda(pts)).with_prior(cuda(mu), cuda(W))
        x = cuda(x0.copy())
        out = ta.Optimize(x, model, circle_options(ta))
        torch.cuda.synchronize()
        assert bool((out.stop_reason >= 0).all()) and bool((out.final_num_residuals == 40 + n).all())
        xs[diff], iters[diff] = x.cpu().numpy(), out.num_iters.cpu().numpy().tolist()
    err = np.abs(xs["central"] - xs["ad"]).max()
    print(f"numeric vs AD with a prior: iterations {iters}, max |x_num - x_ad| {err:.3e}")
    assert err < 5e-3


# ---- 8. what a prior'd model does not do --------------------------------------------------------------------------------------------
def test_refusals(ta):
    dtype = np.float64
    pts, x0 = circle_uniform(dtype)
    P = len(x0)
    res = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype])
    mu, W = cuda(x0), torch.ones(P, 3, dtype=torch.float64, device="cuda")
    model = res.bind(cuda(pts)).with_prior(mu, W)
    ragged = res.bind_ragged(cuda(pts.reshape(-1, 2)), counts=[10] * P).with_prior(mu, W)
    x = cuda(x0)
    before = x.clone()
    for m in (model, ragged):
        with pytest.raises(ValueError, match="splits"):
            ta.Optimize(x, m, circle_options(ta), splits=2)
        o = circle_options(ta)
        o.stop_callback = lambda err, dx2, g2: False
        with pytest.raises(ValueError, match="host controls"):
            ta.Optimize(x, m, o)
        with pytest.raises(ValueError, match="stepping"):
            ta.Optimizer(x, m, circle_options(ta))
        with pytest.raises(ValueError, match="CheckGradient"):
            ta.CheckGradient(m, x)
        with pytest.raises(ValueError, match="Eval"):
            ta.Eval(m, x)
        with pytest.raises(ValueError, match="CalculateJac"):
            ta.CalculateJac(m, x)
        g = circle_options(ta)
        g.solver_type = ta.Options.GradientDescent
        with pytest.raises(ValueError, match="GradientDescent"):
            ta.Optimize(x, m, g)
    with pytest.raises(ValueError, match="1 <= k <= n"):                         # rows > n
        res.bind(cuda(pts)).with_prior(mu, torch.ones(P, 4, 3, dtype=torch.float64, device="cuda"))
    # the library itself refuses rows > n (TOA_E_ARG) before anything is launched
    from tinyopt_amd import _capi
    pr = _capi.ToaPrior()
    pr.mu_dev, pr.W_dev, pr.rows = mu.data_ptr(), W.data_ptr(), 4
    c = torch.zeros(P, dtype=torch.float64, device="cuda")
    ctx = res.ctx
    rc = ctx.lib.toa_jit_accumulate_prior(ctx.h, res._h, 10, P, model.packed.data_ptr(), x.data_ptr(), _capi.C.byref(pr), 0, None, None, c.data_ptr(), None)
    assert rc == -1 and b"rows" in ctx.lib.toa_last_error()
    # manifolds and cost kinds: refused where the prior is attached
    se3 = types_of(ta, "se3")
    with pytest.raises(ValueError, match="manifold='se3'"):
        se3.with_prior(torch.zeros(1, 6, dtype=torch.float64, device="cuda"), torch.ones(1, 6, dtype=torch.float64, device="cuda"))
    user = types_of(ta, "user")
    with pytest.raises(ValueError, match="manifold='user'"):
        user.with_prior(torch.zeros(1, 1, dtype=torch.float64, device="cuda"), torch.ones(1, 1, dtype=torch.float64, device="cuda"))
    for kind in ("cost", "cost_grad"):
        with pytest.raises(ValueError, match="scalar cost"):
            types_of(ta, kind).with_prior(torch.zeros(1, 2, dtype=torch.float64, device="cuda"), torch.ones(1, 2, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(x, before) and float(c.abs().max()) == 0, "a refused call launched something"


def types_of(ta, what):
    """Small bound models of the kinds a prior is refused for."""
    f64 = dict(dtype=torch.float64, device="cuda")
    if what == "se3":
        res = _res(ta, SE3_PRIOR, n=6, item_scalars=0, residuals_per_item=6, header_scalars=12, manifold="se3", dtype=torch.float64)
        return res.bind(None, header=torch.zeros(1, 12, **f64))
    if what == "user":
        res = _res(ta, SO2_RESIDUAL, n=1, item_scalars=4, residuals_per_item=2, dtype=torch.float64, manifold="user", plus_body=SO2_PLUS, x_scalars=2)
        return res.bind(torch.zeros(1, 1, 4, **f64))
    body = "c = (x[0] - p[0]) * (x[0] - p[0]) + x[1] * x[1];" + (" if (want_grad) { G[0] += T(2) * (x[0] - p[0]); G[1] += T(2) * x[1]; }" if what == "cost_grad" else "")
    return _res(ta, body, n=2, item_scalars=1, dtype=torch.float64, kind=what).bind(torch.zeros(1, 1, 1, **f64))


# ---- 9. no scratch ------------------------------------------------------------------------------------------------------------------
def test_prior_kernels_do_not_spill(ta):
    circle = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=torch.float64)
    row = _res(ta, manual_body(ROW_N), n=ROW_N, item_scalars=ROW_N + 1, dtype=torch.float64, kind="accumulate")
    for res in (circle, row):
        for ragged in (False, True):
            s = res.stats_prior(ragged=ragged)
            print("stats_prior", res.n, "ragged" if ragged else "uniform", s)
            assert s["scratch_bytes"] == 0 and s["num_regs"] > 0 and s["wg_per_cu"] >= 1
