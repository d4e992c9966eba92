"""The yardstick of kind="cost_ggn_multi" (tests/ggn_multi_reference.py) pinned on the CPU: its callbacks against central differences,
K = 1 against ggn_reference bit for bit, softmax against a full-Hessian statement of the same cost, a dyadic quadratic that reaches its
minimum in one Newton step exactly (with and without a ridge), the exact-sum data, the seeds of the GPU trajectories and of the sibling
comparison; and the Python routes of the kind — every refusal text, the calls Optimize / accumulate / CheckGradient make, with a prior
and with a shared table, and the POD contracts — over a recording library."""
import os
import sys

import ctypes as C

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ggn_multi_cells as cells  # noqa: E402
import ggn_multi_reference as gm  # noqa: E402
import ggn_reference as gr  # noqa: E402

from tinyopt_amd import _capi, api  # noqa: E402

EPS = 2.0 ** -53


def _central(parts, x, data, h=1e-6):
    g = np.zeros(len(x))
    for a in range(len(x)):
        xp, xm = x.copy(), x.copy()
        xp[a] += h
        xm[a] -= h
        g[a] = (parts(xp, data, False)[0].sum() - parts(xm, data, False)[0].sum()) / (xp[a] - xm[a])
    return g


@pytest.mark.parametrize("name", ["softmax2x6", "softmax3x5", "softmax8x2", "gauss", "quadratic"])
def test_gradient_against_central_differences(name):
    if name.startswith("softmax"):
        K, d = int(name[7]), int(name[9:])
        parts, (data, x0) = gm.softmax_parts(K, d), gm.softmax_case(3, K, d, 40)
    elif name == "gauss":
        parts, (data, x0) = gm.gauss_parts, gm.gauss_case(1)
    else:
        rng = np.random.default_rng(5)
        K, n = 3, 5
        A = rng.normal(size=(20, K, K))
        A = np.einsum("iab,icb->iac", A, A)
        il = np.tril_indices(K)
        data = np.concatenate([rng.normal(size=(20, K * n)), rng.normal(size=(20, K)), A[:, il[0], il[1]]], axis=1)
        parts, x0 = gm.quadratic_parts(K, n), rng.normal(size=n)
    c, g, H = gm.sums(parts, x0, data, np.float64)
    gd = _central(parts, x0, data)
    assert np.allclose(g, gd, rtol=1e-6, atol=1e-7 * np.abs(gd).max()), np.abs(g - gd).max()
    c2, g2, H2 = gm.direct_sums(parts, x0, data)
    assert np.isclose(c, c2, rtol=1e-14) and np.allclose(g, g2, rtol=1e-9, atol=1e-12) and np.allclose(H, H2, rtol=1e-9, atol=1e-12)
    if name == "quadratic":   # u linear, phi quadratic: H is the Hessian — central differences of g
        for a in range(len(x0)):
            xp, xm = x0.copy(), x0.copy()
            xp[a] += 1e-4
            xm[a] -= 1e-4
            col = (gm.sums(parts, xp, data, np.float64)[1] - gm.sums(parts, xm, data, np.float64)[1]) / (xp[a] - xm[a])
            assert np.allclose(col, H[:, a], rtol=1e-7, atol=1e-8)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_K1_is_ggn_reference_bit_for_bit(dtype):
    """With K = 1 the rule is kind 5's: the same cost, g and H to the bit on the logistic data, clamped weights included."""
    n = 12
    data, x0 = gr.logistic_case(4, n, 50)
    data[::7, :n] *= 1e-3   # (flat items; their weights stay above wmin, the exact-sum data below has the clamped ones)

    def parts1(x, d, want):
        c, gs, hs, J = gr.logistic_parts(x, d, want)
        return (c, None, None, None) if not want else (c, gs[:, None], hs[:, None, None], J[:, None, :])
    a, b = gr.sums(gr.logistic_parts, x0, data, dtype), gm.sums(parts1, x0, data, dtype)
    for u, v in zip(a, b):
        assert (np.asarray(u) == np.asarray(v)).all()
    d5 = gr.exact_case(n, 30, 6)
    for p in range(6):
        tp = lambda x, d, want: ((d[:, n], None, None, None) if not want else (d[:, n], d[:, n + 1:n + 2], d[:, n + 2:n + 3, None], d[:, None, :n]))   # noqa: E731
        a, b = gr.sums(gr.table_parts, np.zeros(n), d5[p], dtype), gm.sums(tp, np.zeros(n), d5[p], dtype)
        for u, v in zip(a, b):
            assert (np.asarray(u) == np.asarray(v)).all()


def test_softmax_against_the_full_hessian():
    """n = 12 (K = 2, d = 6; K = 3, d = 4): u is linear in x, so J^T Hs J is the Hessian.  Entry by entry within
    eps (items + c_K) sum |term|, c_K = 16 for the factorisation, the substitution and the row combination (derived in
    tests/test_gpu_ggn_multi.py: test_the_sum_rounded), the terms taken with absolute values through |J|^T |Hs| |J|."""
    for K, d in ((2, 6), (3, 4)):
        data, x0 = gm.softmax_case(2, K, d, 200)
        c, g, H = gm.sums(gm.softmax_parts(K, d), x0, data, np.float64)
        gf, Hf = gm.softmax_full_hessian(K, d, x0, data)
        _, gs, Hs, J = gm.softmax_parts(K, d)(x0, data, True)
        S = np.abs(np.tril(Hs) + np.transpose(np.tril(Hs, -1), (0, 2, 1)))
        Bg = EPS * (200 + 16) * np.einsum("ik,ika->a", np.abs(gs), np.abs(J))
        BH = EPS * (200 + 16) * np.einsum("ika,ikl,ilb->ab", np.abs(J), S, np.abs(J))
        assert (np.abs(g - gf) <= 2 * Bg + 1e-300).all() and (np.abs(H - Hf) <= 2 * BH + 1e-300).all()


@pytest.mark.parametrize("with_ridge", [False, True])
def test_dyadic_quadratic_one_newton_step(with_ridge):
    """K = 2, n = 3, dyadic data: H and g are exact, the Gauss-Newton step from x0 lands on the minimiser exactly."""
    K, n = 2, 3
    V = np.array([[[1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 1, 0]], [[0, 1, 1], [1, 0, -1]]], np.float64)
    b = np.array([[1, 2], [0.5, -1], [2, 0]], np.float64)
    A = np.array([[1, 0.5, 4], [4, -1, 1], [1, 0, 1]], np.float64)   # lower triangles (a00, a10, a11) = L D L^T of unit L, D in {1, 4} — positive definite
    data = np.concatenate([V.reshape(3, -1), b, A], axis=1)
    parts = gm.quadratic_parts(K, n)
    x0 = np.array([2.0, -1.0, 0.5])
    prior = (np.array([0.5, 0.0, -0.25]), np.array([2.0, 1.0, 0.5])) if with_ridge else None
    fn = gm.item_sum(parts, data, np.float64, prior)
    c0, g, H, nres = fn(x0, True)
    c_d, g_d, H_d = gm.direct_sums(parts, x0, data)
    if prior:
        pc, pg, pH = gm.ridge(x0, *prior)
        c_d, g_d, H_d = c_d + pc, g_d + pg, H_d + pH
    assert nres == 1 and c0 == c_d and (np.array(g) == g_d).all() and (np.array(H) == H_d).all()
    xs = x0 - np.linalg.solve(np.array(H), np.array(g))
    c1, g1, _, _ = fn(xs, True)
    assert np.abs(g1).max() <= 1e-12 * np.abs(g).max() and c1 < c0
    # the reported cost's own central difference is g (the 1/2 of the ridge term)
    for a in range(n):
        e = np.zeros(n)
        e[a] = 0.25
        assert (fn(x0 + e, False)[0] - fn(x0 - e, False)[0]) / 0.5 == g[a]   # (a quadratic: central differences are exact, dyadic data)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_exact_case_is_exact(K):
    n, items, P = 13, 197, 6
    d = gm.exact_case(K, n, items, P)
    c32, g32, H32 = gm.exact_sums(K, n, d, np.float32)
    c64, g64, H64 = gm.exact_sums(K, n, d, np.float64, np.float32)
    assert (c32 == c64).all() and (g32 == g64).all() and (H32 == H64).all()
    parts = gm.table_parts(K, n)
    for p in range(P):
        cd, gd, Hd = gm.direct_sums(parts, np.zeros(n), d[p])
        assert (g64[p] == gd).all()   # g = sum gs J whatever was clamped
        if p % 3 == 0:
            assert (H64[p] == Hd).all() and np.abs(Hd).max() > 0
        else:
            J = d[p, :, :K * n].reshape(items, K, n)
            assert (H64[p] == (2.0 ** -60) * np.einsum("ika,ikb->ab", J, J)).all()


def test_nan_stays():
    gs, J = np.ones((1, 2)), np.ones((1, 2, 3))
    Hs = np.array([[[np.nan, 0.0], [0.5, 1.0]]])
    rows, r, w = gm.transform(gs, Hs, J, np.float64)
    assert np.isnan(w[0, 0]) and np.isnan(rows[0, 0]).all()


# ---- the seeds of the GPU tests ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,optname", cells.CELLS + cells.PRIOR_CELLS)
def test_trajectory_seeds_are_usable(problem, optname):
    """The seeds of the GPU trajectories (ggn_multi_cells.py), the ridge cells among them: no accept / reject decision of the yardstick
    closer than 1e-9 to flipping, and at least two problems per cell that take rejected steps."""
    cases, refs, _ = cells.trajectory_cases(problem, optname)
    assert len(cases) == cells.P_TRAJ and all(cells.decision_margin(r) >= cells.NEED_MARGIN and r["stop"] >= 0 for r in refs)
    assert sum(1 for r in refs if not all(r["successes"])) >= 2


def test_every_cell_is_there():
    assert len(cells.CELLS) == 25 and cells.LEFT_OUT == [] and len(cells.PRIOR_CELLS) == 4


@pytest.mark.parametrize("problem", sorted(cells.CLIP))
def test_the_clip_still_binds(problem):
    """The three cells that clip the gradient at 20 instead of 2: at the first Build of every problem some component of g is beyond
    the clip, so the clipped solve is not the unclipped one."""
    cases, refs, kw = cells.trajectory_cases(problem, "grad_clipping")
    assert kw["grad_clipping"] == cells.CLIP[problem]
    for d, x0 in cases:
        g = gm.sums(cells.parts_of(problem), x0, d, np.float64)[1]
        assert np.abs(g).max() > kw["grad_clipping"]


def test_sibling_batch_stays_within_its_cap():
    """The batch of test_gpu_ggn_multi.test_against_cost_hess (softmax, K = 2, d = 6, seeds 0 .. 96, min_rerr_dec = 1e-6): the two numpy
    yardsticks ALONE — the rule's sums and the full Hessian of the same cost, each inside the second reading of the loop — show the same
    StopReason, iteration count and accept flags in all but 5 % of the problems at the most."""
    K, d, items, parted = 2, 6, 200, 0
    _, ropt = gm.options_pair(None, min_rerr_dec=1e-6)
    for seed in range(97):
        data, x0 = gm.softmax_case(seed, K, d, items)
        a, b = gm.optimize(gm.softmax_parts(K, d), data, x0, ropt), gm.optimize_full_hessian(K, d, data, x0, ropt)
        parted += not (a["stop"] == b["stop"] and a["num_iters"] == b["num_iters"] and list(a["successes"]) == list(b["successes"]))
    assert parted <= 0.05 * 97, parted


# ---- the Python routes: a recording library, as test_cpu_ggn_reference.py builds one ------------------------------------------------------
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


def _multi(n=4, K=2, shared=False):
    r = object.__new__(api.JitResidual)
    r.__dict__.update(ctx=StubContext(), n=n, kR=K, kD=2, kH=0, dtype=F64, manifold="euclid", kind="cost_ggn_multi", diff="ad", diff_h=0.0,
                      large_n=False, xdim=n, kS=3 if shared else 0, _h=C.c_void_p(0x2000))
    _KEEP.append(r)
    m = object.__new__(api.JitModel)
    m.__dict__.update(res=r, P=P, items=4, n=n, dtype=F64, xdim=n, m=4 * K, packed=torch.ones(P, 8, dtype=F64))
    if shared:
        m.shared = torch.ones(4, 3, dtype=F64)
    return m


def _call(fn, **kw):
    cost, ctx = _multi(**kw), StubContext()
    x = CudaLike(torch.ones(P, cost.n, dtype=F64))
    try:
        fn(cost, x, ctx)
        return None, ctx.lib.calls, cost, x
    except Exception as e:  # noqa: BLE001
        return e, ctx.lib.calls, cost, x


def _value(a):
    return a.value if isinstance(a, C.c_void_p) else a


def _with_prior(cost, full=False):
    n = cost.n
    return cost.with_prior(torch.zeros(P, n, dtype=F64), torch.ones(P, 2, n, dtype=F64) if full else torch.ones(P, n, dtype=F64))


def test_the_kind_is_known():
    K = api.JitResidual.KINDS
    assert K["cost_ggn_multi"] == 6 and K["cost_ggn"] == 5 and "cost_ggn_multi" not in api.JitResidual.COST_KINDS
    assert api.JitResidual.COST_GGN_MULTI_MAX_K == 8 and _capi.ToaJitSpec is api.ToaJitSpec


@pytest.mark.parametrize("solver", [api.Options.LevenbergMarquardt, api.Options.GaussNewton])
def test_reaches_toa_jit_lm_run(solver):
    o = api.Options()
    o.solver_type = solver
    err, calls, cost, x = _call(lambda cost, x, ctx: api.Optimize(x, cost, o, ctx=ctx))
    assert err is None, err
    run = [c for c in calls if c[0].startswith("toa_jit_")]
    assert [c[0] for c in run] == ["toa_jit_lm_run"]
    args = run[0][1]
    assert _value(args[0]) == 0x1000 and _value(args[1]) == 0x2000 and args[2] == 4 and args[3] == P   # num_items = the ITEMS, not items x K
    assert args[4] == cost.packed.data_ptr() and args[5] == x.data_ptr()
    pod = args[6]._obj
    assert pod.solver_type == solver and pod.save_last == 1


@pytest.mark.parametrize("full", [False, True])
def test_with_prior_reaches_toa_jit_lm_run_prior(full):
    err, calls, cost, x = _call(lambda cost, x, ctx: api.Optimize(x, _with_prior(cost, full), api.Options(), ctx=ctx))
    assert err is None, err
    run = [c for c in calls if c[0].startswith("toa_jit_")]
    assert [c[0] for c in run] == ["toa_jit_lm_run_prior"]
    args = run[0][1]
    assert args[2] == 4 and args[3] == P and args[5] == x.data_ptr()
    pod = args[6]._obj   # toa_prior: mu_dev, W_dev, rows (0 = the diagonal form)
    assert pod.rows == (2 if full else 0) and pod.mu_dev and pod.W_dev
    assert ctypes_sizeof(pod) == C.sizeof(_capi.ToaPrior)


def ctypes_sizeof(pod):
    return C.sizeof(type(pod))


@pytest.mark.parametrize("prior", [False, True])
def test_shared_reaches_toa_jit_lm_run_shared(prior):
    err, calls, cost, x = _call(lambda cost, x, ctx: api.Optimize(x, _with_prior(cost) if prior else cost, api.Options(), ctx=ctx), shared=True)
    assert err is None, err
    run = [c for c in calls if c[0].startswith("toa_jit_")]
    assert [c[0] for c in run] == ["toa_jit_lm_run_shared"]
    args = run[0][1]
    sh = args[5]._obj   # toa_shared: the table and its rows, one per item
    assert args[2] == 4 and args[3] == P and sh.rows == 4 and sh.table_dev == cost.shared.data_ptr() and args[6] == x.data_ptr()
    assert args[7] is None and (args[8] is not None) == prior   # no bounds; the prior's pod or NULL


def test_accumulate_hands_over_g_H_and_the_cost():
    err, calls, cost, x = _call(lambda cost, x, ctx: api.accumulate(cost, x, ctx=ctx))
    acc = [c for c in calls if c[0] == "toa_jit_accumulate"]
    assert err is None and len(acc) == 1
    args = acc[0][1]
    assert args[2] == 4 and args[6] == 1 and all(a is not None and a != 0 for a in args[7:10])   # want_grad = 1: g, the full H and the cost
    err, calls, cost, x = _call(lambda cost, x, ctx: api.accumulate(cost, x, want_grad=False, ctx=ctx))
    args = [c for c in calls if c[0] == "toa_jit_accumulate"][0][1]
    assert err is None and args[6] == 0 and args[7] is None and args[8] is None and args[9]
    err, calls, cost, x = _call(lambda cost, x, ctx: api.accumulate(_with_prior(cost), x, ctx=ctx))
    assert err is None and [c[0] for c in calls if c[0].startswith("toa_jit_")] == ["toa_jit_accumulate_prior"]
    err, calls, cost, x = _call(lambda cost, x, ctx: api.accumulate(_with_prior(cost), x, ctx=ctx), shared=True)
    assert err is None and [c[0] for c in calls if c[0].startswith("toa_jit_")] == ["toa_jit_accumulate_shared"]


@pytest.mark.parametrize("check_H", [False, True])
def test_check_gradient_calls(check_H):
    """CheckGradient: one toa_jit_check_gradient (g); with check_H, 1 + 2 n accumulate calls on shifted copies of x (host side, as for
    kind="cost_ggn")."""
    err, calls, cost, x = _call(lambda cost, x, ctx: api.CheckGradient(cost, x, check_H=check_H, ctx=ctx))
    assert err is None, err
    names = [c[0] for c in calls if c[0].startswith("toa_jit_")]
    assert names.count("toa_jit_check_gradient") == 1 and names.count("toa_jit_accumulate") == ((1 + 2 * cost.n) if check_H else 0)
    chk = [c for c in calls if c[0] == "toa_jit_check_gradient"][0][1]
    assert chk[2] == 4   # the items


PREFIX = ('a multi-output second-order scalar cost (kind="cost_ggn_multi") runs in the uniform one-launch form through Optimize (LM / GN), accumulate '
          "and CheckGradient only, with with_prior and a shared table: ")


def _options(**kw):
    o = api.Options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


NO_HOST = "no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)"
NO_ROWS = "(it has no residual rows: accumulate returns its value, its gradient and its Hessian)"
REFUSED_CALLS = {
    "GradientDescent": (lambda cost, x, ctx: api.Optimize(x, cost, _options(solver_type=api.Options.GradientDescent), ctx=ctx),
                        'no GradientDescent: run the same cost as kind="cost_grad"'),
    "LBFGS": (lambda cost, x, ctx: api.Optimize(x, cost, _options(solver_type=api.Options.LBFGS), ctx=ctx), 'no L-BFGS: run the same cost as kind="cost_grad"'),
    "splits": (lambda cost, x, ctx: api.Optimize(x, cost, api.Options(), ctx=ctx, splits=2), "no row-split form (splits)"),
    "max_duration_ms": (lambda cost, x, ctx: api.Optimize(x, cost, _options(max_duration_ms=5.0), ctx=ctx), NO_HOST),
    "stop_callback": (lambda cost, x, ctx: api.Optimize(x, cost, _options(stop_callback=lambda e, d, g: False), ctx=ctx), NO_HOST),
    "Optimizer": (lambda cost, x, ctx: api.Optimizer(x, cost, api.Options(), ctx=ctx), "no stepping form (Optimizer)"),
    "Eval": (lambda cost, x, ctx: api.Eval(cost, x, ctx=ctx), "no Eval " + NO_ROWS),
    "CalculateJac": (lambda cost, x, ctx: api.CalculateJac(cost, x, ctx=ctx), "no CalculateJac " + NO_ROWS),
    "with_loss": (lambda cost, x, ctx: cost.with_loss("huber", 1.0), "no M-estimator (with_loss): a scalar cost has no residuals to robustify"),
    "with_bounds": (lambda cost, x, ctx: cost.with_bounds(torch.zeros(P, cost.n, dtype=F64), None), "no box bounds (with_bounds)"),
    "bind_ragged": (lambda cost, x, ctx: cost.res.bind_ragged(torch.ones(7, 2, dtype=F64), counts=[2, 0, 5]), "no ragged batches (bind_ragged)"),
    # with a prior beside it the kind still speaks first
    "GradientDescent with a prior": (lambda cost, x, ctx: api.Optimize(x, _with_prior(cost), _options(solver_type=api.Options.GradientDescent), ctx=ctx),
                                     'no GradientDescent: run the same cost as kind="cost_grad"'),
    "LBFGS with a prior": (lambda cost, x, ctx: api.Optimize(x, _with_prior(cost), _options(solver_type=api.Options.LBFGS), ctx=ctx),
                           'no L-BFGS: run the same cost as kind="cost_grad"'),
}


@pytest.mark.parametrize("what", list(REFUSED_CALLS))
def test_refusals_before_any_call(what):
    fn, text = REFUSED_CALLS[what]
    err, calls, _, _ = _call(fn)
    assert isinstance(err, ValueError) and str(err) == PREFIX + text, (what, err)
    assert calls == []


def test_check_gradient_refusals_of_the_decorated_model():
    """CheckGradient on a shared model and beside a prior: refused with their owners' sentences (api._REFUSALS), before any call."""
    err, calls, _, _ = _call(lambda cost, x, ctx: api.CheckGradient(cost, x, ctx=ctx), shared=True)
    assert isinstance(err, ValueError) and "shared item table" in str(err) and "no CheckGradient" in str(err) and calls == []
    err, calls, _, _ = _call(lambda cost, x, ctx: api.CheckGradient(_with_prior(cost), x, ctx=ctx))
    assert isinstance(err, ValueError) and "no CheckGradient" in str(err) and calls == []


@pytest.mark.parametrize("kw,text", [
    (dict(manifold="se3"), "Euclidean parameters only, not manifold='se3'"),
    (dict(diff="central"), 'the body brings its own derivatives, nothing is differentiated: diff="ad" only, not diff=\'central\''),
    (dict(large_n=True), "no large_n (the launch-per-phase pipeline is for residual models)"),
    (dict(n=64), "1 <= n <= 63 in float32 and float64 (one wavefront per problem), not n = 64"),
    (dict(n=0), "1 <= n <= 63 in float32 and float64 (one wavefront per problem), not n = 0"),
    (dict(residuals_per_item=9), "residuals_per_item is K, the outputs per item: 1 <= K <= 8 (an item is K rows of the Gram), not 9"),
    (dict(residuals_per_item=0), "residuals_per_item is K, the outputs per item: 1 <= K <= 8 (an item is K rows of the Gram), not 0"),
])
def test_construction_refusals_before_any_call(kw, text):
    ctx = StubContext()
    args = dict(n=2, item_scalars=1, residuals_per_item=2, kind="cost_ggn_multi", dtype=F64, ctx=ctx)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        api.JitResidual("c = x[0];", **args)
    assert str(e.value) == PREFIX + text and ctx.lib.calls == []


def test_construction_hands_K_and_the_table_to_the_library():
    """The POD contract: kind = 6, residuals_per_item = K, shared_scalars, in toa_jit_spec as it stands (ABI 7: its size is unchanged)."""
    ctx = StubContext()
    api.JitResidual("c = x[0];", n=6, item_scalars=1, residuals_per_item=3, kind="cost_ggn_multi", dtype=F64, ctx=ctx, shared_scalars=5)
    call = [c for c in ctx.lib.calls if c[0] == "toa_model_compile_ex"][0][1]
    spec = call[1]._obj
    assert spec.kind == 6 and spec.residuals_per_item == 3 and spec.num_params == 6 and spec.shared_scalars == 5 and spec.diff == 0 and spec.large_n == 0
    assert _capi.TOA_ABI_VERSION == 7 if hasattr(_capi, "TOA_ABI_VERSION") else True
