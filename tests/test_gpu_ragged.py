"""Ragged batches of run-time models (JitResidual.bind_ragged; toa_jit_*_ragged, csrc/ragged.hpp): every problem has its own item
count.  The yardstick is the uniform path itself: problem p of a ragged batch must be BIT-equal (x, the errs history, iterations,
StopReason, final cost) to the same problem run alone through the uniform call with items = its count — every problem here has
fewer than 512 residual rows, so that call stays on the one-wavefront route.  Where the project has an oracle it is compared too,
at the tolerances the uniform tests of that model use."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gd_reference as gr  # noqa: E402
from parity import check_trajectories, gpu_dict  # noqa: E402
from test_gpu_eval import Guarded  # noqa: E402
from test_gpu_gd import logit_body  # noqa: E402
from test_gpu_jit import CIRCLE  # noqa: E402
from test_gpu_row_models import ad_body, manual_body  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {np.float32: torch.float32, np.float64: torch.float64}
SKIPPED = -1
CIRCLE_COUNTS = [3, 4, 10, 63, 64, 65, 130, 0, 200]
ROW_COUNTS = [1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 129, 300]   # around every possible super-step size
ROW_N = 20
HDR_COUNTS = [5, 64, 160]
GD_COUNTS = [1, 63, 64, 65, 200, 0]
GD_N = 12
HDR_BODY = """
const S a = x[0], k = x[1], f = x[2], c = x[3];
const S e = exp(-k * p[0]);
r[0] = a * e * sin(f * p[0] + h[1]) + c - p[1];
r[1] = h[0] * (atan2(a * e * cos(f * p[0] + h[1]), S(1.0) + pow(c, 2)) - p[2]);
"""
_RES = {}


def _res(ta, body, **kw):
    key = (body, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _RES:
        _RES[key] = ta.JitResidual(body, **kw)
    return _RES[key]


class Case:
    """A ragged batch: per-problem item arrays (numpy, [count, kD]), optional headers [P, kH], x0 [P, n]."""

    def __init__(self, items, x0, header=None):
        self.items, self.x0, self.header = items, x0, header
        self.counts = [a.shape[0] for a in items]
        self.P = len(items)

    def ragged(self, res):
        data = torch.from_numpy(np.concatenate(self.items, axis=0)).cuda()
        hdr = torch.from_numpy(self.header).cuda() if self.header is not None else None
        return res.bind_ragged(data, counts=self.counts, header=hdr)

    def alone(self, res, p):
        """Problem p as a uniform batch of one."""
        hdr = torch.from_numpy(self.header[p:p + 1]).cuda() if self.header is not None else None
        return res.bind(torch.from_numpy(self.items[p][None]).cuda(), hdr)

    def x(self, p=None):
        return torch.from_numpy((self.x0 if p is None else self.x0[p:p + 1]).copy()).cuda()


_CASES = {}


def circle_case(dtype):
    """tests/circle.cpp:20-30 per problem: points on the circle of radius 2 about (2, 7) + 1e-5 noise, x0 = (0, 0, 1)."""
    if ("circle", dtype) not in _CASES:
        rng = np.random.default_rng(11)
        items = []
        for cnt in CIRCLE_COUNTS:
            ang = np.linspace(0, 2 * np.pi, cnt, endpoint=False) + rng.uniform(0, 1)
            items.append((np.stack([2 + 2 * np.cos(ang), 7 + 2 * np.sin(ang)], -1) + 1e-5 * rng.uniform(-1, 1, (cnt, 2))).astype(dtype))
        _CASES[("circle", dtype)] = Case(items, np.tile(np.array([0, 0, 1], dtype), (len(items), 1)))
    return _CASES[("circle", dtype)]


def circle_options(ta):
    o = ta.Options()
    o.lm.damping_init = 1e1
    return o


def row_case(oracle, dtype):
    """The DenseRow residual, n = 20: the oracle's synthetic problems, one per count."""
    if ("row", dtype) not in _CASES:
        items, x0, AB = [], [], []
        for p, cnt in enumerate(ROW_COUNTS):
            A, b, x, _ = oracle.synth_dense_row(1, ROW_N, cnt, dtype, seed=500 + p)
            items.append(np.concatenate([A[0], b[0][:, None]], -1))
            x0.append(x[0])
            AB.append((A, b))
        c = Case(items, np.stack(x0))
        c.AB = AB
        _CASES[("row", dtype)] = c
    return _CASES[("row", dtype)]


def row_res(ta, dtype, kind):
    if kind == "accumulate":
        return _res(ta, manual_body(ROW_N), n=ROW_N, item_scalars=ROW_N + 1, dtype=TDT[dtype], kind="accumulate")
    return _res(ta, ad_body(ROW_N), n=ROW_N, item_scalars=ROW_N + 1, dtype=TDT[dtype])


def header_case():
    if "hdr" not in _CASES:
        rng = np.random.default_rng(5)
        P = len(HDR_COUNTS)
        xs = np.stack([rng.uniform(1.5, 2.5, P), rng.uniform(0.2, 0.6, P), rng.uniform(2.0, 3.0, P), rng.uniform(-0.5, 0.5, P)], axis=1)
        hdr = np.stack([rng.uniform(0.5, 1.5, P), rng.uniform(-1, 1, P)], axis=1)
        items = []
        for p, cnt in enumerate(HDR_COUNTS):
            t = np.linspace(0.0, 3.0, cnt)
            a, k, f, c = xs[p]
            e = np.exp(-k * t)
            y0 = a * e * np.sin(f * t + hdr[p, 1]) + c + 1e-3 * rng.uniform(-1, 1, cnt)
            y1 = np.arctan2(a * e * np.cos(f * t + hdr[p, 1]), 1.0 + c ** 2) + 1e-3 * rng.uniform(-1, 1, cnt)
            items.append(np.stack([t, y0, y1], axis=1))
        _CASES["hdr"] = Case(items, xs + 0.05 * rng.uniform(-1, 1, xs.shape), hdr)
    return _CASES["hdr"]


def logit_case(dtype):
    if ("logit", dtype) not in _CASES:
        rng = np.random.default_rng(77)
        items = []
        for cnt in GD_COUNTS:
            A = (rng.standard_normal((cnt, GD_N)) / np.sqrt(GD_N)).astype(dtype)
            w = rng.standard_normal(GD_N)
            yl = np.where(A.astype(np.float64) @ w + 0.5 * rng.standard_normal(cnt) > 0, 1.0, -1.0).astype(dtype)
            items.append(np.concatenate([A, yl[:, None]], axis=1))
        _CASES[("logit", dtype)] = Case(items, np.zeros((len(items), GD_N), dtype))
    return _CASES[("logit", dtype)]


OUT_FIELDS = ("stop_reason", "num_iters", "num_failures", "num_consec_failures", "final_cost", "final_num_residuals", "final_rerr_dec",
              "final_inlier_ratio", "errs", "deltas2", "successes", "final_hessian")


def solve_ragged(ta, case, model, opts, **kw):
    x = case.x()
    out = ta.Optimize(x, model, opts, history=True, **kw)
    torch.cuda.synchronize()
    return x, out


def assert_bit_equal_to_uniform(ta, case, res, opts, x, out, loss=None):
    """Every problem with items against its own uniform solve; a problem without items: kSkipped, x untouched, no residuals."""
    for p, cnt in enumerate(case.counts):
        if cnt == 0:
            assert int(out.stop_reason[p]) == SKIPPED, f"problem {p} (no items): StopReason {int(out.stop_reason[p])}"
            assert torch.equal(x[p].cpu(), torch.from_numpy(case.x0[p])), f"problem {p} (no items): x was changed"
            assert int(out.final_num_residuals[p]) == 0
            continue
        m1 = case.alone(res, p)
        if loss:
            m1 = m1.with_loss(*loss)
        x1 = case.x(p)
        o1 = ta.Optimize(x1, m1, opts, history=True)
        torch.cuda.synchronize()
        assert torch.equal(x[p], x1[0]), f"problem {p} ({cnt} items): x differs by {float((x[p] - x1[0]).abs().max())}"
        for f in OUT_FIELDS:
            a, b = getattr(out, f), getattr(o1, f)
            if a is None and b is None:
                continue
            assert torch.equal(a[p], b[0]), f"problem {p} ({cnt} items): {f} differs: {a[p]} vs {b[0]}"


# ---- 1. the circle fit as text (JetModel) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_circle_fit_ragged(ta, oracle, dtype):
    case, opts = circle_case(dtype), circle_options(ta)
    res = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype])
    model = case.ragged(res)
    assert model.P == len(CIRCLE_COUNTS) and model.max_items == 200 and model.offsets.dtype == torch.int64
    x, out = solve_ragged(ta, case, model, opts)
    assert_bit_equal_to_uniform(ta, case, res, opts, x, out)
    assert res.stats_ragged()["scratch_bytes"] == 0
    if dtype == np.float64:   # as tests/test_gpu_jit.py
        for p, cnt in enumerate(case.counts):
            if cnt == 0:
                continue
            ref = oracle.circle_fit_lm(case.items[p][None], case.x0[p:p + 1], opts.to_pod())
            assert np.abs(x[p].cpu().numpy() - ref["x"][0]).max() < 1e-8, f"problem {p} ({cnt} items)"
            assert int(out.stop_reason[p]) == int(ref["stop"][0]) and int(out.num_iters[p]) == int(ref["iters"][0]), f"problem {p} ({cnt} items)"
            assert np.allclose(float(out.final_cost[p]), ref["cost"][0], rtol=1e-6, atol=1e-18), f"problem {p} ({cnt} items)"


# ---- 2. the DenseRow residual as text, n = 20 (row model) --------------------------------------------------------------------------
def cost_abs_allowance(A, b, x0, ref):
    """How far two correct float64 evaluations of ONE recorded cost may differ through cancellation, in the units of ref["errs"], per
    entry of the history.  cost = sum_i r_i^2, r_i = t_i + 0.1 sin(t_i) - b_i, t_i = a_i . x.  With u = 2^-53, the n-term dot product,
    the sine and the subtraction give |fl(r_i) - r_i| <= eps = (n + 2) u max_i(sum_j |a_ij x_j| + |b_i| + 0.1); then
    |fl(C) - C| <= 2 sum_i |r_i| eps <= 2 sqrt(m C) eps (Cauchy-Schwarz) for each of the two sides: 4 sqrt(m C) eps.  While the
    residuals are of the size of their terms this is far below 1e-9 C (1e-13 at the first entries here) and changes nothing; it
    matters only where an exactly fitted problem has driven its r_i to ~1e-8 and the cost to ~1e-15.  Everything comes from the
    reference's run: its data, its x, its recorded costs (scaled back to sum r^2 by the ratio at x0, where nothing cancels)."""
    A, b, x0 = np.asarray(A[0], np.float64), np.asarray(b[0], np.float64), np.asarray(x0, np.float64)
    m, n = A.shape
    t0 = A @ x0
    scale = float(ref["errs"][0][0]) / float(((t0 + 0.1 * np.sin(t0) - b) ** 2).sum())
    xmax = np.maximum(np.abs(x0), np.abs(np.asarray(ref["x"][0], np.float64)))
    eps = (n + 2) * 2.0 ** -53 * float((np.abs(A) @ xmax + np.abs(b) + 0.1).max())
    C = np.abs(np.asarray(ref["errs"][0], np.float64)) / scale
    return scale * 4.0 * np.sqrt(m * C) * eps, lambda c: scale * 4.0 * np.sqrt(m * abs(c) / scale) * eps


def assert_same_trajectory(g, ref, allow, allow_of, label):
    """One problem, entry by entry, no ties: the same StopReason, iteration and failure counts and accept / reject flags; every recorded
    cost and the final cost to tests/parity.py's 1e-9 relative plus the cancellation allowance of THAT cost; x to parity's 1e-8."""
    k = int(ref["iters"][0])
    assert int(g["stop"][0]) == int(ref["stop"][0]) and int(g["iters"][0]) == k, (label, g["stop"][0], ref["stop"][0], g["iters"][0], k)
    assert np.array_equal(np.asarray(g["succ"][0][:k], bool), np.asarray(ref["succ"][0][:k], bool)), label
    if ref.get("fails") is not None:
        assert int(g["fails"][0]) == int(ref["fails"][0]), (label, "fails")
    for i in range(k):
        ge, re_ = float(g["errs"][0][i]), float(ref["errs"][0][i])
        print(f"{label}: entry {i}: device {ge:.17g} reference {re_:.17g} |diff| {abs(ge - re_):.3g} allowed {1e-9 * abs(re_) + allow[i]:.3g}")
        assert abs(ge - re_) <= 1e-9 * abs(re_) + allow[i], (label, i, ge, re_, allow[i])
    gc, rc = float(g["cost"][0]), float(ref["cost"][0])
    assert abs(gc - rc) <= 1e-9 * abs(rc) + allow_of(rc), (label, "final cost", gc, rc)
    xr = np.asarray(ref["x"][0], np.float64)
    assert np.abs(np.asarray(g["x"][0], np.float64) - xr).max() < 1e-8 * max(1.0, float(np.abs(xr).max())), (label, "x")


@pytest.mark.parametrize("dtype,kind", [(np.float64, "residual"), (np.float32, "accumulate")])
def test_dense_row_ragged(ta, oracle, dtype, kind):
    """Default options, not the benchmark's: with min_error = 0 an exactly fitted problem (count <= n) would iterate on round-off.
    fp64 against the oracle: a problem with more items than parameters through tests/parity.py::check_trajectories as it is
    (1e-9).  A problem with no more items than parameters (counts 1, 15, 16, 17) is fitted exactly and its last one or two recorded
    costs are cancellation residue (1e-13 .. 1e-16, measured 2e-8 relative apart at 1.8e-15), which check_trajectories' purely
    relative comparison cannot take: those go entry by entry through assert_same_trajectory — 1e-9 relative on every entry plus the
    absolute cancellation allowance of that entry (cost_abs_allowance), no ties accepted."""
    case, opts = row_case(oracle, dtype), ta.Options()
    res = row_res(ta, dtype, kind)
    x, out = solve_ragged(ta, case, case.ragged(res), opts)
    assert_bit_equal_to_uniform(ta, case, res, opts, x, out)
    assert res.stats_ragged()["scratch_bytes"] == 0
    if dtype == np.float64:
        g = gpu_dict(out, x)
        for p, cnt in enumerate(case.counts):
            A, b = case.AB[p]
            ref = oracle.dense_row_lm(A, b, case.x0[p:p + 1], opts.to_pod(), history=True)
            gp = {k: v[p:p + 1] for k, v in g.items()}
            label = f"ragged n = {ROW_N}, {cnt} items"
            if cnt > ROW_N:
                st = check_trajectories(gp, ref, dtype, opts.to_pod(), label=label)
                assert st["full"] + st["ties"] == 1
            else:
                allow, allow_of = cost_abs_allowance(A, b, case.x0[p], ref)
                assert_same_trajectory(gp, ref, allow, allow_of, label)


# ---- 3. a separate header array, two residuals per item ----------------------------------------------------------------------------
def test_header_and_two_residuals_ragged(ta):
    case, opts = header_case(), ta.Options()
    res = _res(ta, HDR_BODY, n=4, item_scalars=3, residuals_per_item=2, header_scalars=2, dtype=torch.float64)
    model = case.ragged(res)
    x, out = solve_ragged(ta, case, model, opts)
    assert_bit_equal_to_uniform(ta, case, res, opts, x, out)
    assert bool((out.stop_reason >= 0).all())
    assert_accumulate_bit_equal(ta, case, res, model, kR=2)


# ---- 4. the Accumulate seam ----------------------------------------------------------------------------------------------------------
def assert_accumulate_bit_equal(ta, case, res, model, kR=1, is_cost=False):
    x = case.x()
    g, H, c, nres = ta.accumulate(model, x)
    c0 = ta.accumulate(model, x, want_grad=False)[2]
    torch.cuda.synchronize()
    for p, cnt in enumerate(case.counts):
        if cnt == 0:
            assert float(g[p].abs().max()) == 0 and float(c[p]) == 0 and float(c0[p]) == 0 and int(nres[p]) == 0
            assert H is None or float(H[p].abs().max()) == 0
            continue
        g1, H1, c1, n1 = ta.accumulate(case.alone(res, p), case.x(p))
        c01 = ta.accumulate(case.alone(res, p), case.x(p), want_grad=False)[2]
        torch.cuda.synchronize()
        assert torch.equal(g[p], g1[0]) and torch.equal(c[p], c1[0]) and torch.equal(c0[p], c01[0]), f"problem {p} ({cnt} items)"
        assert is_cost or torch.equal(H[p], H1[0]), f"problem {p} ({cnt} items): H"
        assert int(nres[p]) == int(n1[0]) == (1 if is_cost else cnt * kR)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_accumulate_ragged_circle(ta, dtype):
    case = circle_case(dtype)
    res = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype])
    assert_accumulate_bit_equal(ta, case, res, case.ragged(res))


@pytest.mark.parametrize("dtype,kind", [(np.float64, "residual"), (np.float32, "accumulate")])
def test_accumulate_ragged_dense_row(ta, oracle, dtype, kind):
    case = row_case(oracle, dtype)
    res = row_res(ta, dtype, kind)
    assert_accumulate_bit_equal(ta, case, res, case.ragged(res))


# ---- 5. Eval / CalculateJac ----------------------------------------------------------------------------------------------------------
def assert_eval_bit_equal(ta, case, res, kR=1):
    model, x, n = case.ragged(res), case.x(), res.n
    rows = sum(case.counts) * kR
    assert model.rows == rows
    gr_, gj = Guarded((rows,), x.dtype), Guarded((rows, n), x.dtype)
    ta.Eval(model, x, res_out=gr_.view, J_out=gj.view)
    gr0 = Guarded((rows,), x.dtype)
    r0, J0 = ta.Eval(model, x, jac=False, res_out=gr0.view)
    gj1 = Guarded((rows, n), x.dtype)
    ta.CalculateJac(model, x, J_out=gj1.view)
    torch.cuda.synchronize()
    assert J0 is None
    assert gr_.intact() and gj.intact() and gr0.intact() and gj1.intact(), "a sentinel behind res / J was overwritten"
    row = 0
    for p, cnt in enumerate(case.counts):
        if cnt == 0:
            continue
        r1, J1 = ta.Eval(case.alone(res, p), case.x(p))
        r2, _ = ta.Eval(case.alone(res, p), case.x(p), jac=False)
        torch.cuda.synchronize()
        sl = slice(row, row + cnt * kR)
        assert torch.equal(gr_.view[sl], r1[0]) and torch.equal(gj.view[sl], J1[0]), f"problem {p} ({cnt} items)"
        assert torch.equal(gr0.view[sl], r2[0]) and torch.equal(gj1.view[sl], J1[0]), f"problem {p} ({cnt} items)"
        row += cnt * kR
    assert row == rows


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_eval_ragged_circle(ta, dtype):
    assert_eval_bit_equal(ta, circle_case(dtype), _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype]))


@pytest.mark.parametrize("dtype,kind", [(np.float64, "residual"), (np.float32, "accumulate")])
def test_eval_ragged_dense_row(ta, oracle, dtype, kind):
    assert_eval_bit_equal(ta, row_case(oracle, dtype), row_res(ta, dtype, kind))


# ---- 6. the queue order ----------------------------------------------------------------------------------------------------------------
def test_queue_order_does_not_change_results(ta, oracle):
    dtype = np.float64
    case, opts = row_case(oracle, dtype), ta.Options.benchmark()
    model = case.ragged(row_res(ta, dtype, "residual"))
    xa, oa = solve_ragged(ta, case, model, opts)
    xb, ob = solve_ragged(ta, case, model, opts)
    xk, ok = solve_ragged(ta, case, model, opts, keep_order=True)
    for x2, o2, what in ((xb, ob, "a second default run"), (xk, ok, "keep_order=True")):
        assert torch.equal(xa, x2), what
        for f in OUT_FIELDS + ("counters",):
            a, b = getattr(oa, f), getattr(o2, f)
            assert (a is None and b is None) or torch.equal(a, b), f"{what}: {f}"
    assert int(oa.counters[3]) == case.P


# ---- 7. a loss -------------------------------------------------------------------------------------------------------------------------
def test_huber_loss_ragged(ta):
    dtype = np.float64
    case, opts = circle_case(dtype), circle_options(ta)
    res = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype])
    x, out = solve_ragged(ta, case, case.ragged(res).with_loss("huber", 0.05), opts)
    assert_bit_equal_to_uniform(ta, case, res, opts, x, out, loss=("huber", 0.05))


# ---- 8. gradient descent ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["cost", "cost_grad"])
def test_gradient_descent_ragged(ta, kind, dtype):
    case = logit_case(dtype)
    res = _res(ta, logit_body(GD_N, kind), n=GD_N, item_scalars=GD_N + 1, dtype=TDT[dtype], kind=kind)
    o = ta.Options()
    o.solver_type = ta.Options.GradientDescent
    o.hessian.save_last = False
    o.max_iters = 25
    o.gd.lr = float(np.float32(1.0 / 64))
    model = case.ragged(res)
    x, out = solve_ragged(ta, case, model, o)
    assert out.final_hessian is None
    assert_bit_equal_to_uniform(ta, case, res, o, x, out)
    assert_accumulate_bit_equal(ta, case, res, model, is_cost=True)
    if dtype == np.float64:
        g = gpu_dict(out, x)
        for p, cnt in enumerate(case.counts):
            if cnt == 0:
                continue
            A, yl = case.items[p][:, :GD_N], case.items[p][:, GD_N]
            ref = gr.gd_optimize(case.x0[p:p + 1], lambda _, xx: gr.logistic(A, yl, xx, dtype), o.to_pod(), o.gd.lr, dtype)
            st = check_trajectories({k: v[p:p + 1] for k, v in g.items()}, ref, dtype, o.to_pod(), label=f"ragged logit {kind}, {cnt} items")
            assert st["full"] + st["ties"] == 1


# ---- 9. a numeric model ----------------------------------------------------------------------------------------------------------------
def test_numeric_model_ragged(ta):
    dtype = np.float64
    case, opts = circle_case(dtype), circle_options(ta)
    res = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype], diff="central")
    x, out = solve_ragged(ta, case, case.ragged(res), opts)
    assert_bit_equal_to_uniform(ta, case, res, opts, x, out)


# ---- 10. what a ragged batch does not do -----------------------------------------------------------------------------------------------
def test_refusals_ragged(ta):
    dtype = np.float64
    case = circle_case(dtype)
    res = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype])
    model = case.ragged(res)
    with pytest.raises(ValueError, match="splits"):
        ta.Optimize(case.x(), model, circle_options(ta), splits=2)
    o = circle_options(ta)
    o.stop_callback = lambda err, dx2, g2: False
    with pytest.raises(ValueError, match="host controls"):
        ta.Optimize(case.x(), model, o)
    with pytest.raises(ValueError, match="stepping"):
        ta.Optimizer(case.x(), model, circle_options(ta))
    with pytest.raises(ValueError, match="CheckGradient"):
        ta.CheckGradient(model, case.x())
    with pytest.raises(ValueError, match="total_items"):
        res.bind_ragged(torch.zeros(10, 2, dtype=torch.float64, device="cuda"), counts=[3, 3])
    # a cost model on LM is refused by the library, as for a uniform batch
    lc = logit_case(dtype)
    cost = _res(ta, logit_body(GD_N, "cost"), n=GD_N, item_scalars=GD_N + 1, dtype=TDT[dtype], kind="cost")
    with pytest.raises(ta.ToaError):
        ta.Optimize(lc.x(), lc.ragged(cost), ta.Options())


# ---- 11. a batch whose problems are all empty ------------------------------------------------------------------------------------------
def test_all_problems_empty(ta):
    """total_items = 0 is legal: every problem ends with kSkipped and x untouched, the seam gives zeros, Eval returns empty rows."""
    res = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=torch.float64)
    model = res.bind_ragged(torch.zeros(0, 2, dtype=torch.float64, device="cuda"), counts=[0, 0, 0])
    assert model.P == 3 and model.max_items == 0 and model.total_items == 0
    x0 = torch.tensor([[0.0, 0.0, 1.0]] * 3, dtype=torch.float64, device="cuda")
    x = x0.clone()
    out = ta.Optimize(x, model, circle_options(ta))
    g, H, c, nres = ta.accumulate(model, x)
    r, J = ta.Eval(model, x)
    torch.cuda.synchronize()
    assert bool((out.stop_reason == SKIPPED).all()) and torch.equal(x, x0) and bool((out.final_num_residuals == 0).all())
    assert float(g.abs().max()) == 0 and float(H.abs().max()) == 0 and float(c.abs().max()) == 0 and bool((nres == 0).all())
    assert tuple(r.shape) == (0,) and tuple(J.shape) == (0, 3)
