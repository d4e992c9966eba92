"""Gradient descent on scalar cost models (JitResidual kind="cost" / "cost_grad", toa_jit_gd_run) against the numpy
restatement of OptimizeAcc / Step + SolverGD (tests/gd_reference.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gd_reference as gr  # noqa: E402
from parity import check_trajectories, gpu_dict  # noqa: E402
from tinyopt_amd.api import default_context  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {np.float32: torch.float32, np.float64: torch.float64}

# (p[0] = 42, the centre of tests/unconstrained.cpp's quartic, as the item's one data scalar)
QUARTIC_COST = "const S y = x[0] - p[0]; c = (T(3) * y * y + y * y * y * y) - T(2);"
QUARTIC_GRAD = ("const T y = x[0] - p[0]; c = (T(3) * y * y + y * y * y * y) - T(2);\n"
                "if (want_grad) { G[0] += T(2) * T(3) * y + T(4) * (y * y * y); }")


def logit_body(n, kind):
    if kind == "cost":
        return f"S z = S(0); for (int j = 0; j < {n}; ++j) z += p[j] * x[j]; c = log(S(1) + exp(-p[{n}] * z));"
    return (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j]; const T yy = p[{n}]; const T e = exp(-yy * z);\n"
            f"c = log(T(1) + e);\n"
            f"if (want_grad) {{ const T s = -yy * e / (T(1) + e); for (int j = 0; j < {n}; ++j) G[j] += s * p[j]; }}")


_MODELS = {}


def _res(ta, body, n, kD, dtype, kind):
    key = (body, n, kD, dtype, kind)
    if key not in _MODELS:
        _MODELS[key] = ta.JitResidual(body, n=n, item_scalars=kD, dtype=TDT[dtype], kind=kind)
    return _MODELS[key]


def _one_item(ta, body, dtype, kind, P, value=42.0):
    """A one-parameter model whose problems have ONE item carrying one data scalar."""
    return _res(ta, body, 1, 1, dtype, kind).bind(torch.full((P, 1, 1), value, dtype=TDT[dtype], device="cuda"))


def _gd_options(ta, **kw):
    o = ta.Options()
    o.solver_type = ta.Options.GradientDescent
    o.hessian.save_last = False
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _logit_data(P, n, items, dtype, seed=0):
    rng = np.random.default_rng(seed + 1000 * n + items)
    A = (rng.standard_normal((P, items, n)) / np.sqrt(n)).astype(dtype)
    w = rng.standard_normal((P, n))
    z = np.einsum("pin,pn->pi", A.astype(np.float64), w)
    yl = np.where(z + 0.5 * rng.standard_normal(z.shape) > 0, 1.0, -1.0).astype(dtype)
    data = np.concatenate([A, yl[:, :, None]], axis=2)
    return A, yl, data


def _run_logit(ta, n, items, dtype, kind, o, P=97, lr=None, seed=0, history=True):
    A, yl, data = _logit_data(P, n, items, dtype, seed)
    lr = np.float32(lr if lr is not None else 1.0 / items)
    o.gd.lr = float(lr)
    model = _res(ta, logit_body(n, kind), n, n + 1, dtype, kind).bind(torch.from_numpy(data).cuda())
    x0 = np.zeros((P, n), dtype)
    x = torch.from_numpy(x0.copy()).cuda()
    out = ta.Optimize(x, model, o, history=history)
    torch.cuda.synchronize()
    ref = gr.gd_optimize(x0, lambda p, xx: gr.logistic(A[p], yl[p], xx, dtype), o.to_pod(), float(lr), dtype)
    return out, x, ref


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["cost", "cost_grad"])
def test_quartic_trajectories(ta, dtype, kind):
    """tests/unconstrained.cpp:19-42 over 64 problems, x0 in [38, 46]; whole trajectories compared directly (costs go
    negative).  fp64: 1000 iterations to convergence; fp32: 100 iterations, short of its round-off floor."""
    P = 64
    x0 = np.linspace(38.0, 46.0, P).astype(dtype)[:, None]
    o = _gd_options(ta, max_iters=1000 if dtype == np.float64 else 100, min_error=0.0, min_rerr_dec=0.0)
    o.gd.lr = 0.01
    model = _one_item(ta, QUARTIC_COST if kind == "cost" else QUARTIC_GRAD, dtype, kind, P)
    x = torch.from_numpy(x0.copy()).cuda()
    out = ta.Optimize(x, model, o, history=True)
    torch.cuda.synchronize()
    ref = gr.gd_optimize(x0, lambda p, xx: gr.quartic(xx, dtype), o.to_pod(), 0.01, dtype)
    g = gpu_dict(out, x)
    assert (g["stop"] == ref["stop"]).all(), (g["stop"], ref["stop"])
    assert (g["iters"] == ref["iters"]).all()
    assert (g["succ"] == ref["succ"]).all()
    assert (g["fails"] == ref["fails"]).all()
    rtol, atol = (1e-10, 1e-10) if dtype == np.float64 else (2e-5, 2e-5)
    assert np.allclose(g["errs"], ref["errs"], rtol=rtol, atol=atol)
    assert np.allclose(g["cost"], ref["cost"], rtol=rtol, atol=atol)
    assert np.abs(g["x"] - ref["x"]).max() < (1e-9 if dtype == np.float64 else 1e-4)
    if dtype == np.float64:
        assert out.Succeeded().all() and out.Converged().all()
        assert np.abs(g["x"] - 42.0).max() < 1e-5
    assert out.final_hessian is None
    assert (out.final_num_residuals.cpu().numpy() == 1).all()
    assert (out.final_inlier_ratio.cpu().numpy() == 1).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["cost", "cost_grad"])
@pytest.mark.parametrize("n", [1, 3, 12, 13, 31, 50, 63])
def test_logistic_regression_trajectories(ta, n, kind, dtype):
    """Batched logistic regression, P = 97, every item count around the wave width; tie-aware parity with the restatement."""
    for items in (1, 63, 64, 65, 1000):
        o = _gd_options(ta, max_iters=25)
        out, x, ref = _run_logit(ta, n, items, dtype, kind, o)
        st = check_trajectories(gpu_dict(out, x), ref, dtype, o.to_pod(), label=f"logit n={n} items={items} {kind}")
        assert st["full"] + st["ties"] == 97, st


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["cost", "cost_grad"])
def test_gradient_seam(ta, kind, dtype):
    """toa_jit_accumulate on a cost model = SolverGD::Build's accumulation: g = sum_i grad c_i and the cost against the
    closed form, nres = 1; a non-NULL H_dev is refused."""
    P, n, items = 37, 12, 300
    A, yl, data = _logit_data(P, n, items, dtype, seed=3)
    rng = np.random.default_rng(5)
    x0 = (0.3 * rng.standard_normal((P, n))).astype(dtype)
    model = _res(ta, logit_body(n, kind), n, n + 1, dtype, kind).bind(torch.from_numpy(data).cuda())
    x = torch.from_numpy(x0).cuda()
    g, H, c, nres = ta.accumulate(model, x)
    _, _, c0, _ = ta.accumulate(model, x, want_grad=False)
    torch.cuda.synchronize()
    assert H is None and (nres.cpu().numpy() == 1).all()
    rt = 1e-10 if dtype == np.float64 else 1e-4
    for p in range(P):
        cr, gr_ = gr.logistic(A[p].astype(np.float64), yl[p].astype(np.float64), x0[p].astype(np.float64), np.float64)
        assert abs(c.cpu().numpy()[p] - cr) <= rt * abs(cr)
        assert abs(c0.cpu().numpy()[p] - cr) <= rt * abs(cr)
        assert np.abs(g.cpu().numpy()[p] - gr_).max() <= rt * max(1.0, np.abs(gr_).max())
    ctx = default_context()
    Hb = torch.zeros(P, n, n, dtype=TDT[dtype], device="cuda")
    rc = ctx.lib.toa_jit_accumulate(ctx.h, model.res._h, items, P, model.packed.data_ptr(), x.data_ptr(), 1, g.data_ptr(),
                                    Hb.data_ptr(), c.data_ptr(), nres.data_ptr())
    assert rc != 0 and b"H_dev" in ctx.lib.toa_last_error()


@pytest.mark.parametrize("variant", ["grad_clipping", "sqrt_norm", "downscale_by_2", "normalize", "check_final_cost",
                                     "min_grad_norm2", "history"])
def test_options_variants(ta, variant):
    """Options that change the GD loop, each against the restatement (logistic, n = 3, 64 items, fp64)."""
    o = _gd_options(ta, max_iters=30)
    lr = None
    if variant == "grad_clipping":
        o.grad_clipping = 0.5
    elif variant == "sqrt_norm":
        o.cost.use_squared_norm = False
    elif variant == "downscale_by_2":
        o.cost.downscale_by_2 = True
    elif variant == "normalize":
        o.cost.normalize = True
    elif variant == "check_final_cost":
        o.check_final_cost = True
    elif variant == "min_grad_norm2":
        o.min_grad_norm2 = 1.0
        o.max_iters = 200
        lr = 0.1
    out, x, ref = _run_logit(ta, 3, 64, np.float64, "cost_grad", o, lr=lr)
    g = gpu_dict(out, x)
    st = check_trajectories(g, ref, np.float64, o.to_pod(), label=variant)
    assert st["full"] + st["ties"] == 97, st
    if variant == "min_grad_norm2":
        assert (g["stop"] == gr.STOP_MIN_GRAD_NORM).sum() >= 10
    if variant == "history":
        ok = g["iters"] == ref["iters"]
        assert np.allclose(g["deltas2"][ok], ref["deltas2"][ok], rtol=1e-9, atol=1e-300)
        assert np.allclose(out.final_rerr_dec.cpu().numpy()[ok], ref["rerr"][ok], rtol=1e-6, atol=1e-12)
        assert (out.num_consec_failures.cpu().numpy()[ok] == ref["consec"][ok]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["cost", "cost_grad"])
def test_failure_paths(ta, kind, dtype):
    """c = x^2 with lr = 1.5 (every step lands on -2x; exact in binary, tests/test_cpu_gd_reference.py derives it by hand):
    roll-backs and kMaxConsecNoDecr, and kMaxNoDecr with max_total_failures = 2.  A cost that turns NaN (sqrt(x), lr = 4:
    1 -> -1): kSystemHasNaNOrInf with x rolled back."""
    P = 16
    x0 = (np.arange(1, P + 1) / 4.0 * np.where(np.arange(P) % 2, -1.0, 1.0)).astype(dtype)[:, None]
    sq = "c = x[0] * x[0];" if kind == "cost" else "c = x[0] * x[0]; if (want_grad) { G[0] += T(2) * x[0]; }"
    model = _one_item(ta, sq, dtype, kind, P, 0.0)
    f = lambda p, xx: (dtype(xx[0] * xx[0]), np.array([dtype(2) * xx[0]], dtype))  # noqa: E731
    for mtf, stop, iters in ((0, gr.STOP_MAX_CONSEC_NO_DECR, 6), (2, gr.STOP_MAX_NO_DECR, 3)):
        o = _gd_options(ta, max_iters=50, max_total_failures=mtf)
        o.gd.lr = 1.5
        x = torch.from_numpy(x0.copy()).cuda()
        out = ta.Optimize(x, model, o, history=True)
        torch.cuda.synchronize()
        ref = gr.gd_optimize(x0, f, o.to_pod(), 1.5, dtype)
        g = gpu_dict(out, x)
        assert (g["stop"] == stop).all() and (ref["stop"] == stop).all(), (g["stop"], ref["stop"])
        assert (g["iters"] == iters).all() and (ref["iters"] == iters).all()
        for k in ("succ", "errs", "deltas2", "fails", "x", "cost"):
            assert (g[k] == ref[k]).all(), k
        assert (g["x"] == x0).all()   # every rejected jump rolled back

    sq = "c = sqrt(x[0]);" if kind == "cost" else "c = sqrt(x[0]); if (want_grad) { G[0] += T(0.5) / sqrt(x[0]); }"
    model = _one_item(ta, sq, dtype, kind, P, 0.0)
    o = _gd_options(ta)
    o.gd.lr = 4.0
    x = torch.ones(P, 1, dtype=TDT[dtype], device="cuda")
    out = ta.Optimize(x, model, o)
    torch.cuda.synchronize()
    assert (out.stop_reason.cpu().numpy() == gr.STOP_NAN_OR_INF).all()
    assert (out.num_iters.cpu().numpy() == 2).all() and (x.cpu().numpy() == 1).all()


def test_refusals(ta):
    n, items, P = 3, 64, 8
    _, _, data = _logit_data(P, n, items, np.float64)
    res = _res(ta, logit_body(n, "cost"), n, n + 1, np.float64, "cost")
    model = res.bind(torch.from_numpy(data).cuda())
    x = torch.zeros(P, n, dtype=torch.float64, device="cuda")
    for st in (ta.Options.LevenbergMarquardt, ta.Options.GaussNewton):   # optimize.h:41-56: no second order on a scalar cost
        o = ta.Options()
        o.solver_type = st
        with pytest.raises(ta.ToaError):
            ta.Optimize(x, model, o)
    o = _gd_options(ta)
    with pytest.raises(ta.ToaError):                                     # a scalar cost has no residuals to robustify
        ta.Optimize(x, model.with_loss("huber", 1.0), o)
    ta.Optimize(x, model, o)                                             # (the handle's loss is cleared again)
    torch.cuda.synchronize()
    with pytest.raises(ta.ToaError):                                     # cost kinds: Euclidean parameters only
        ta.JitResidual("c = x[0];", n=6, item_scalars=0, header_scalars=12, manifold="se3", kind="cost")
    with pytest.raises(ta.ToaError):                                     # ... and one residual per item
        ta.JitResidual("c = x[0];", n=1, item_scalars=0, residuals_per_item=2, kind="cost")
    o.max_duration_ms = 10.0
    with pytest.raises(ValueError):                                      # host controls: out of scope under GD
        ta.Optimize(x, model, o)
    residual = ta.JitResidual("r[0] = x[0] - p[0];", n=1, item_scalars=1)   # GD on a residual model (optimize.h:75 throws)
    rm = residual.bind(torch.ones(P, 4, 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ta.ToaError):
        ta.Optimize(torch.zeros(P, 1, dtype=torch.float64, device="cuda"), rm, _gd_options(ta))
    ctx = default_context()
    from tinyopt_amd._capi import ToaGdOptions, ToaResults
    gd = ToaGdOptions()
    ctx.lib.toa_gd_options_default(C.byref(gd))
    pod = _gd_options(ta).to_pod()
    res0 = ToaResults()
    assert ctx.lib.toa_jit_gd_run(ctx.h, res._h, items, 0, None, None, C.byref(pod), C.byref(gd), C.byref(res0), None) == 0   # P = 0
    pod.solver_type = 0
    assert ctx.lib.toa_jit_gd_run(ctx.h, res._h, items, 0, None, None, C.byref(pod), C.byref(gd), C.byref(res0), None) != 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_scratch_at_n12(ta, dtype):
    for kind in ("cost", "cost_grad"):
        s = _res(ta, logit_body(12, kind), 12, 13, dtype, kind).stats()
        assert s["scratch_bytes"] == 0, (kind, s)
        assert s["wg_per_cu"] >= 1
