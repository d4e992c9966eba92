"""The yardstick of the rank-one second-order scalar costs (tests/ggn_reference.py) pinned on the CPU: its callbacks
against their own central differences, against hess_reference's logistic callbacks at n = 12, a trajectory derived by hand that is
exact in binary, the exact-sum data of the GPU test, the seeds of the GPU trajectories; and the Python routes of kind="cost_ggn" —
every refusal text, and the calls Optimize / accumulate / CheckGradient make — over a recording library (the route tests fail on a
tree whose api.py does not know the kind)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ggn_cells as cells  # noqa: E402
import ggn_reference as gr  # noqa: E402
import hess_reference as hr  # noqa: E402

from tinyopt_amd import _capi, api  # noqa: E402


# ---- the callbacks -------------------------------------------------------------------------------------------------------------------
CASES = {
    "logistic": (gr.logistic_parts, lambda: gr.logistic_case(3, 7, 40), True),
    "poisson": (gr.poisson_parts, lambda: gr.poisson_case(3, 6, 40), True),
    "spot": (gr.spot_parts, lambda: gr.spot_case(5), False),          # u = mu(x) is not linear in x: only the gradient is exact
    "quadratic": (gr.quadratic_parts, lambda: (np.random.default_rng(2).normal(size=(30, 7)) ** 2 + 0.1, np.full(5, 0.3)), True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_callbacks_against_their_own_central_differences(name):
    """g = sum gs J against central differences of the cost (h = 1e-6: truncation h^2 |c'''| / 6 ~ 1e-12, round-off eps |c| / h ~ 1e-8
    relative to the cost, so 1e-6 of the gradient's scale holds both); H = sum w J J^T against central differences of g where u is
    linear in x (the dropped phi' hess u term is zero there)."""
    parts, case, linear = CASES[name]
    data, x0 = case()
    x0 = np.asarray(x0, np.float64)
    c, g, H = gr.sums(parts, x0, data, np.float64)
    h = 1e-6
    for a in range(len(x0)):
        e = np.zeros_like(x0)
        e[a] = h
        cp, gp, _ = gr.sums(parts, x0 + e, data, np.float64)
        cm, gm, _ = gr.sums(parts, x0 - e, data, np.float64)
        assert abs((cp - cm) / (2 * h) - g[a]) <= 1e-6 * max(1.0, np.abs(g).max()), (name, a)
        if linear:
            assert np.abs((gp - gm) / (2 * h) - H[:, a]).max() <= 1e-5 * max(1.0, np.abs(H).max()), (name, a)
    assert (H == H.T).all() and np.linalg.eigvalsh(H).min() >= -1e-12 * np.abs(H).max()
    assert gr.sums(parts, x0, data, np.float64, want=False)[0] == c


def test_logistic_equals_hess_reference_at_n_12():
    """The same derivation, another summation form: hess_reference sums hz p_a p_b item by item in Python floats, this file forms
    einsum(w, J, J).  Every term is the same three-factor product up to one rounding of association, and a sum of `items` terms in any
    order differs from another by at most (items + 2) eps sum |term|: that bound, per entry."""
    n, items = 12, 200
    data, x0 = gr.logistic_case(1, n, items)
    ch, gh, Hh, _ = hr.item_sum(hr.logistic_term, data)([float(v) for v in x0], True)
    c, g, H = gr.sums(gr.logistic_parts, x0, data, np.float64)
    _, gs, hs, J = gr.logistic_parts(x0, data, True)
    eps = 2.0 ** -53
    Bg = (items + 2) * eps * np.abs(gs[:, None] * J).sum(axis=0)
    BH = (items + 2) * eps * np.einsum("i,ia,ib->ab", np.abs(hs), np.abs(J), np.abs(J))
    assert (np.abs(g - np.array(gh)) <= Bg).all() and (np.abs(H - np.array(Hh)) <= BH).all()
    assert abs(c - ch) <= (items + 2) * eps * c


def test_weight_rule():
    for dt in (np.float32, np.float64):
        wmin = gr.WMIN[np.dtype(dt)]
        hs = np.array([4.0, wmin * 2, wmin, 0.0, -1.0, np.nan, np.inf], dt)
        w = gr.weight(hs, dt)
        assert (w[:5] == np.array([4.0, wmin * 2, wmin, wmin, wmin], dt)).all() and np.isnan(w[5]) and np.isinf(w[6])
        assert np.sqrt(dt(wmin)) ** 2 == dt(wmin) and wmin > 0   # a power of four: its root is exact


def test_a_quadratic_reaches_its_minimum_in_one_newton_step():
    """c = hs (a . x - b)^2 / 2 over three items with dyadic data, derived by hand: a = (1, 0), (0, 1), (1, 1); b = 1, 2, 1; hs = 4, 1, 1
    from x = (0, 0).  g = sum hs (a . x - b) a = (-4 - 1, -2 - 1) = (-5, -3); H = sum hs a a^T = [[5, 1], [1, 2]], det 9;
    dx = -H^-1 g = ((2 * 5 - 1 * 3) / 9, (5 * 3 - 1 * 5) / 9) = (7 / 9, 10 / 9).  Not dyadic — so the data is scaled to make it so: with
    a third item a = (1, 1) replaced by a = (2, 0), b = 2, hs = 1 the system decouples: H = diag(4 + 4, 1) = diag(8, 1),
    g = (-4 - 4, -2) = (-8, -2), dx = (1, 2): exact in binary.  At (1, 2) every residual is zero, so the cost is 0 exactly."""
    data = np.array([[1.0, 0.0, 1.0, 4.0], [0.0, 1.0, 2.0, 1.0], [2.0, 0.0, 2.0, 1.0]])
    c, g, H = gr.sums(gr.quadratic_parts, np.zeros(2), data, np.float64)
    assert c == 0.5 * (4 + 4 + 4) and (g == [-8.0, -2.0]).all() and (H == [[8.0, 0.0], [0.0, 1.0]]).all()
    _, ropt = gr.options_pair(None, solver="gn")
    r = gr.optimize(gr.quadratic_parts, data, [0.0, 0.0], ropt)
    assert r["errs"][0] == 6.0 and r["errs"][1] == 0.0 and r["successes"][:2] == [True, True]
    assert r["x"] == [1.0, 2.0] and r["final_cost"] == 0.0
    for dt in (np.float32, np.float64):   # the same sums in the problem's dtype
        c32, g32, H32 = gr.sums(gr.quadratic_parts, np.zeros(2), data, dt)
        assert c32 == c and (g32 == g).all() and (H32 == H).all() and g32.dtype == dt


@pytest.mark.parametrize("n", [1, 13, 50, 63])
def test_exact_case_is_exact_in_float32(n):
    for items in (1, 65, 197):
        d = gr.exact_case(n, items, 6)
        a, b = gr.exact_sums(d, np.float32), gr.exact_sums(d, np.float64, np.float32)
        assert all((u == v).all() for u, v in zip(a, b)), (n, items)
        assert (d.astype(np.float32) == d).all()
    # ... and at the magnitudes' proven limit, 8192 items
    d = gr.exact_case(n, 8192, 3)
    a, b = gr.exact_sums(d, np.float32), gr.exact_sums(d, np.float64, np.float32)
    assert all((u == v).all() for u, v in zip(a, b))


def test_geometry_restated():
    """RowStageGeom::make for this kind, spot values worked out by hand: n = 50 fp32, items of 51 scalars — rows of 3 x 17 = 51 scalars
    and items of 51 scalars both take 13 x 16 bytes = 208 B; the budget is 20480 - 1280 - 512 = 18688 B: one region holds 64 x 208 =
    13312 B (IT = 64), a ring of two 44 x 208 x 2 = 18304 B (IT = 44)."""
    assert gr.row_stage_items(50, 51, np.float32) == (64, 44)
    for n in (1, 12, 13, 63):
        for dt in (np.float32, np.float64):
            it1, it2 = gr.row_stage_items(n, n + 3, dt)
            assert 1 <= it2 <= it1 <= 64


@pytest.mark.parametrize("problem,optname", cells.CELLS)
def test_trajectory_seeds_are_usable(problem, optname):
    """The seeds of the GPU trajectories (ggn_cells.py): no accept / reject decision of the yardstick closer than 1e-9 to flipping, and at
    least two problems per cell that take rejected steps."""
    cases, refs, _ = cells.trajectory_cases(problem, optname)
    assert len(cases) == cells.P_TRAJ and all(cells.decision_margin(r) >= cells.NEED_MARGIN and r["stop"] >= 0 for r in refs)
    assert sum(1 for r in refs if not all(r["successes"])) >= 2


def test_left_out_cells_are_few():
    assert len(cells.LEFT_OUT) * 10 <= len(cells.CELLS) + len(cells.LEFT_OUT)


def test_sibling_batch_stays_within_its_cap():
    """The batch of test_gpu_ggn.test_against_cost_hess: how many of the 97 problems the restatement ALONE decides within 2 B of a tie
    (B = eps (items + 6) sum |c_i| / cost) — the cap of 5 % holds for the chosen data and options (min_rerr_dec = 1e-6: a solve
    under the default 1e-10 runs into its round-off floor and takes its last decision there, 27 of these 97 do)."""
    n, items, near = 12, 200, 0
    _, ropt = gr.options_pair(None, min_rerr_dec=1e-6)
    for seed in range(97):
        data, x0 = gr.logistic_case(seed, n, items)
        r = gr.optimize(gr.logistic_parts, data, x0, ropt)
        B = 2.0 ** -53 * (items + 6) * np.abs(gr.logistic_parts(np.array(r["x"]), data, False)[0]).sum() / max(r["final_cost"], 1e-300)
        near += r["min_margin"] <= 2 * B
    assert near <= 0.05 * 97, near


# ---- the Python routes: a recording library, as test_cpu_api_routes.py builds one -------------------------------------------------------
F64, P = torch.float64, 3


class RecordingLib:
    """Every attribute is a library entry that records (name, the arguments it was called with) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in _capi.PROTOTYPES:
            raise AttributeError(name)
        argtypes = _capi.PROTOTYPES[name][1]

        def entry(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for a prototype of {len(argtypes)}"
            self.calls.append((name, args))
            return 0
        return entry


class StubContext:
    device = 0

    def __init__(self):
        self.lib, self.h = RecordingLib(), C.c_void_p(0x1000)


class CudaLike:
    is_cuda = True

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return getattr(self._t, name)


_KEEP = []


def _ggn(n=3):
    r = object.__new__(api.JitResidual)
    r.__dict__.update(ctx=StubContext(), n=n, kR=1, kD=2, kH=0, dtype=F64, manifold="euclid", kind="cost_ggn", diff="ad", diff_h=0.0,
                      large_n=False, xdim=n, _h=C.c_void_p(0x2000))
    _KEEP.append(r)
    m = object.__new__(api.JitModel)
    m.__dict__.update(res=r, P=P, items=4, n=n, dtype=F64, xdim=n, m=4, packed=torch.ones(P, 8, dtype=F64))
    return m


def _call(fn):
    cost, ctx = _ggn(), StubContext()
    x = CudaLike(torch.ones(P, cost.n, dtype=F64))
    try:
        fn(cost, x, ctx)
        return None, ctx.lib.calls, cost, x
    except Exception as e:  # noqa: BLE001
        return e, ctx.lib.calls, cost, x


def _value(a):
    return a.value if isinstance(a, C.c_void_p) else a


def test_the_kind_is_known():
    assert api.JitResidual.KINDS["cost_ggn"] == 5 and "cost_ggn" not in api.JitResidual.COST_KINDS and api.JitResidual.COST_GGN_MAX_N == 63


@pytest.mark.parametrize("solver", [api.Options.LevenbergMarquardt, api.Options.GaussNewton])
def test_cost_ggn_reaches_toa_jit_lm_run(solver):
    o = api.Options()
    o.solver_type = solver
    err, calls, cost, x = _call(lambda cost, x, ctx: api.Optimize(x, cost, o, ctx=ctx))
    assert err is None
    run = [c for c in calls if c[0].startswith("toa_jit_")]
    assert [c[0] for c in run] == ["toa_jit_lm_run"]
    args = run[0][1]
    assert _value(args[0]) == 0x1000 and _value(args[1]) == 0x2000 and args[2] == 4 and args[3] == P
    assert args[4] == cost.packed.data_ptr() and args[5] == x.data_ptr()
    pod = args[6]._obj
    assert pod.solver_type == solver and pod.save_last == 1


def test_accumulate_hands_over_g_H_and_the_cost():
    err, calls, cost, x = _call(lambda cost, x, ctx: api.accumulate(cost, x, ctx=ctx))
    acc = [c for c in calls if c[0] == "toa_jit_accumulate"]
    assert err is None and len(acc) == 1
    args = acc[0][1]
    assert args[6] == 1 and all(a is not None and a != 0 for a in args[7:10])   # want_grad = 1: g, the full H and the cost
    err, calls, cost, x = _call(lambda cost, x, ctx: api.accumulate(cost, x, want_grad=False, ctx=ctx))
    args = [c for c in calls if c[0] == "toa_jit_accumulate"][0][1]
    assert err is None and args[6] == 0 and args[7] is None and args[8] is None and args[9]


@pytest.mark.parametrize("check_H", [False, True])
def test_check_gradient_calls(check_H):
    """CheckGradient: one toa_jit_check_gradient (g); with check_H, 1 + 2 n accumulate calls on shifted copies of x (host side, as for
    kind="cost_hess")."""
    err, calls, cost, x = _call(lambda cost, x, ctx: api.CheckGradient(cost, x, check_H=check_H, ctx=ctx))
    assert err is None, err
    names = [c[0] for c in calls if c[0].startswith("toa_jit_")]
    assert names.count("toa_jit_check_gradient") == 1 and names.count("toa_jit_accumulate") == ((1 + 2 * cost.n) if check_H else 0)


PREFIX = ('a rank-one second-order scalar cost (kind="cost_ggn") runs in the uniform one-launch form through Optimize (LM / GN), accumulate and '
          "CheckGradient only: ")


def _options(**kw):
    o = api.Options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


NO_HOST = "no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)"
REFUSED_CALLS = {
    "GradientDescent": (lambda cost, x, ctx: api.Optimize(x, cost, _options(solver_type=api.Options.GradientDescent), ctx=ctx),
                        'no GradientDescent: run the same cost as kind="cost_grad"'),
    "LBFGS": (lambda cost, x, ctx: api.Optimize(x, cost, _options(solver_type=api.Options.LBFGS), ctx=ctx), 'no L-BFGS: run the same cost as kind="cost_grad"'),
    "splits": (lambda cost, x, ctx: api.Optimize(x, cost, api.Options(), ctx=ctx, splits=2), "no row-split form (splits)"),
    "max_duration_ms": (lambda cost, x, ctx: api.Optimize(x, cost, _options(max_duration_ms=5.0), ctx=ctx), NO_HOST),
    "stop_callback": (lambda cost, x, ctx: api.Optimize(x, cost, _options(stop_callback=lambda e, d, g: False), ctx=ctx), NO_HOST),
    "Optimizer": (lambda cost, x, ctx: api.Optimizer(x, cost, api.Options(), ctx=ctx), "no stepping form (Optimizer)"),
    "Eval": (lambda cost, x, ctx: api.Eval(cost, x, ctx=ctx), "no Eval (it has no residual rows: accumulate returns its value, its gradient and its Hessian)"),
    "CalculateJac": (lambda cost, x, ctx: api.CalculateJac(cost, x, ctx=ctx),
                     "no CalculateJac (it has no residual rows: accumulate returns its value, its gradient and its Hessian)"),
    "with_loss": (lambda cost, x, ctx: cost.with_loss("huber", 1.0), "no M-estimator (with_loss): a scalar cost has no residuals to robustify"),
    "with_prior": (lambda cost, x, ctx: cost.with_prior(torch.zeros(P, cost.n, dtype=F64), torch.ones(P, cost.n, dtype=F64)),
                   "no Gaussian prior (with_prior): hand a ridge term over as extra items whose J is a unit vector"),
    "with_bounds": (lambda cost, x, ctx: cost.with_bounds(torch.zeros(P, cost.n, dtype=F64), None), "no box bounds (with_bounds)"),
    "bind_ragged": (lambda cost, x, ctx: cost.res.bind_ragged(torch.ones(7, 2, dtype=F64), counts=[2, 0, 5]), "no ragged batches (bind_ragged)"),
}


@pytest.mark.parametrize("what", list(REFUSED_CALLS))
def test_refusals_before_any_call(what):
    fn, text = REFUSED_CALLS[what]
    err, calls, _, _ = _call(fn)
    assert isinstance(err, ValueError) and str(err) == PREFIX + text, (what, err)
    assert calls == []


@pytest.mark.parametrize("kw,text", [
    (dict(manifold="se3"), "Euclidean parameters only, not manifold='se3'"),
    (dict(diff="central"), 'the body brings its own derivatives, nothing is differentiated: diff="ad" only, not diff=\'central\''),
    (dict(large_n=True), "no large_n (the launch-per-phase pipeline is for residual models)"),
    (dict(residuals_per_item=2), "an item has one cost term: residuals_per_item = 1, not 2"),
    (dict(n=64), "1 <= n <= 63 in float32 and float64 (one wavefront per problem), not n = 64"),
    (dict(n=0), "1 <= n <= 63 in float32 and float64 (one wavefront per problem), not n = 0"),
])
def test_construction_refusals_before_any_call(kw, text):
    ctx = StubContext()
    args = dict(n=2, item_scalars=1, kind="cost_ggn", dtype=F64, ctx=ctx)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        api.JitResidual("c = x[0];", **args)
    assert str(e.value) == PREFIX + text and ctx.lib.calls == []
