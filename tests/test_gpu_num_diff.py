"""Numerical differentiation of run-time models (JitResidual diff="forward" | "central" | "fast_central"; csrc/num_diff.hpp) and
CheckGradient (toa_jit_check_gradient), against the numpy restatement of the reference's diff/num_diff.h and
diff/gradient_check.h (tests/num_diff_reference.py)."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gd_reference as gr  # noqa: E402
import num_diff_reference as nd  # noqa: E402
from parity import gpu_dict  # noqa: E402
from tinyopt_amd.api import default_context  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {np.float32: torch.float32, np.float64: torch.float64}
E_ARG, E_UNSUPPORTED = -1, -4
H6 = 2.0 ** -6   # the dyadic step of the exact cases
_RES = {}


def _res(ta, body, **kw):
    key = (body, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _RES:
        _RES[key] = ta.JitResidual(body, **kw)
    return _RES[key]


# ---- exact cases: r_q = sum_j p[q (n + 1) + j] x[j] - p[q (n + 1) + n], every scalar a multiple of 1/8 -------------------------
def linear_body(n, kR, kind, squared=False, flip=None):
    """squared: + x[0]^2 in every residual (forward differences then read J + h in column 0).  flip: that column of the hand-written
    Jacobian with the wrong sign."""
    s = f"for (int q = 0; q < {kR}; ++q) {{ S z = S(0); for (int j = 0; j < {n}; ++j) z += p[q * {n + 1} + j] * x[j]; r[q] = z - p[q * {n + 1} + {n}]"
    s += " + x[0] * x[0]; }" if squared else "; }"
    if kind == "accumulate":
        s += f"\nif (want_grad) {{ for (int q = 0; q < {kR}; ++q) for (int j = 0; j < {n}; ++j) J[q][j] = p[q * {n + 1} + j]; "
        if flip is not None:
            s += f"for (int q = 0; q < {kR}; ++q) J[q][{flip}] = -J[q][{flip}]; "
        s += "}"
    return s


_EXACT = {}


def exact_case(n, kR):
    """Data, x (P = 3, 70 items) and the exact J, r, g, H, cost as Fractions, computed once per shape."""
    if (n, kR) in _EXACT:
        return _EXACT[(n, kR)]
    P, items = 3, 70
    rng = np.random.default_rng(100 * n + kR)
    xm = 8 if n <= 16 else 4           # x in [-1, 1] (beyond 16 parameters [-1/2, 1/2]): the sums stay inside 24 bits, see the premise
    data = rng.integers(-16, 17, (P, items, kR * (n + 1))) / 8.0
    x = rng.integers(-xm, xm + 1, (P, n)) / 8.0
    # exact rational arithmetic, carried as integers over a common power-of-two denominator and handed out as Fractions
    D, X = np.rint(data * 8).astype(np.int64).reshape(P, items * kR, n + 1), np.rint(x * 8).astype(np.int64)
    F = np.vectorize(lambda v, den: Fraction(int(v), den), otypes=[object])
    c = dict(P=P, items=items, data=data, x=x, cases={})
    for squared in (False, True):
        J = D[:, :, :n] * 8                                                  # units of 1/64
        r = np.einsum("pmj,pj->pm", D[:, :, :n], X) - D[:, :, n] * 8         # units of 1/64
        if squared:   # forward differences of x0^2: ((x0 + h)^2 - x0^2) / h = 2 x0 + h, h = 1/64
            r = r + (X[:, 0] * X[:, 0])[:, None]
            J = J.copy()
            J[:, :, 0] += (16 * X[:, 0] + 1)[:, None]
        g = np.einsum("pma,pm->pa", J, r)                                    # units of 2^-12, like H and the cost
        H = np.einsum("pma,pmb->pab", J, J)
        cost = np.einsum("pm,pm->p", r, r)
        # order independence: the sum of the magnitudes of the terms of every accumulated quantity, in units of 2^-12, is below 2^24
        big = max(np.einsum("pma,pm->pa", np.abs(J), np.abs(r)).max(), H.diagonal(axis1=1, axis2=2).max(), cost.max())
        c["cases"][squared] = dict(J=F(J, 64), r=F(r, 64), g=F(g, 4096), H=F(H, 4096), cost=F(cost, 4096), bits=float(big))
    _EXACT[(n, kR)] = c
    return c


def _f(a, dtype):
    return np.array(a, dtype=object).astype(np.float64).astype(dtype)


def _acc(ta, res, c, dtype):
    model = res.bind(torch.from_numpy(c["data"].astype(dtype)).cuda())
    g, H, cost, nres = ta.accumulate(model, torch.from_numpy(c["x"].astype(dtype)).cuda())
    torch.cuda.synchronize()
    return g.cpu().numpy(), H.cpu().numpy(), cost.cpu().numpy(), nres.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,kR", [(1, 1), (3, 3), (15, 1), (16, 1), (20, 1), (63, 1)])
def test_exact_dyadic_accumulate(ta, n, kR, dtype):
    """Dyadic data, x and h = 2^-6: every intermediate is exact in fp32, so the numeric model's (g, H, cost, nres) are BIT-identical to
    those of the kind="accumulate" model with the hand-written Jacobian and to exact rational arithmetic; fast central equals
    central; forward differences of the squared column give exactly J + h."""
    c = exact_case(n, kR)
    kw = dict(n=n, item_scalars=kR * (n + 1), residuals_per_item=kR, dtype=TDT[dtype])
    lin = c["cases"][False]
    # ---- the premise, on the CPU: the restatement in the test dtype equals exact rational arithmetic (and no sum leaves 24 bits)
    for squared, method in ((False, nd.CENTRAL), (False, nd.FAST_CENTRAL), (True, nd.FORWARD)):
        e = c["cases"][squared]
        assert e["bits"] < 2 ** 24
        for p in range(c["P"]):
            d = c["data"][p].reshape(-1, n + 1).astype(dtype)
            f = (lambda xx: d[:, :n] @ xx - d[:, n] + xx[0] * xx[0]) if squared else (lambda xx: d[:, :n] @ xx - d[:, n])
            rr, Jn = nd.num_eval(f, c["x"][p].astype(dtype), method, dtype(H6), dtype)
            assert Jn.dtype == dtype and (Jn == _f(e["J"][p], dtype)).all() and (rr == _f(e["r"][p], dtype)).all()
            assert (Jn.T @ rr == _f(e["g"][p], dtype)).all() and (Jn.T @ Jn == _f(e["H"][p], dtype)).all()
    # ---- the device
    ga, Ha, ca, na = _acc(ta, _res(ta, linear_body(n, kR, "accumulate"), kind="accumulate", **kw), c, dtype)
    gc, Hc, cc, nc = _acc(ta, _res(ta, linear_body(n, kR, "residual"), diff="central", diff_h=H6, **kw), c, dtype)
    assert (na == c["items"] * kR).all() and (nc == na).all()
    assert np.array_equal(gc, ga) and np.array_equal(Hc, Ha) and np.array_equal(cc, ca)
    assert np.array_equal(gc, _f(lin["g"], dtype)) and np.array_equal(Hc, _f(lin["H"], dtype))
    assert np.array_equal(cc, _f(lin["cost"], np.float64))
    gf, Hf, cf, nf = _acc(ta, _res(ta, linear_body(n, kR, "residual"), diff="fast_central", diff_h=H6, **kw), c, dtype)
    assert np.array_equal(gf, gc) and np.array_equal(Hf, Hc) and np.array_equal(cf, cc) and (nf == nc).all()
    sq = c["cases"][True]
    gw, Hw, cw, _ = _acc(ta, _res(ta, linear_body(n, kR, "residual", squared=True), diff="forward", diff_h=H6, **kw), c, dtype)
    assert np.array_equal(gw, _f(sq["g"], dtype)) and np.array_equal(Hw, _f(sq["H"], dtype))
    assert np.array_equal(cw, _f(sq["cost"], np.float64))


# ---- a solve: the planted problem and bound of tests/test_gpu_jit.py:53-110 -----------------------------------------------------
def test_solve_with_central_differences(ta):
    """n = 4, two residuals per item through exp / sin / cos / atan2 / pow, fp64, diff="central": every problem succeeds and lands
    within 5e-3 of the planted parameters, plain and with a Huber loss.  (Iteration counts beside the AD run: printed.)"""
    body = """
    const S a = x[0], k = x[1], f = x[2], c = x[3];
    const S e = exp(-k * p[0]);
    r[0] = a * e * sin(f * p[0] + h[1]) + c - p[1];
    r[1] = h[0] * (atan2(a * e * cos(f * p[0] + h[1]), S(1.0) + pow(c, 2)) - p[2]);
    """
    P, items = 11, 160
    rng = np.random.default_rng(5)
    xs = np.stack([rng.uniform(1.5, 2.5, P), rng.uniform(0.2, 0.6, P), rng.uniform(2.0, 3.0, P), rng.uniform(-0.5, 0.5, P)], axis=1)
    hdr = np.stack([rng.uniform(0.5, 1.5, P), rng.uniform(-1, 1, P)], axis=1)
    t = np.tile(np.linspace(0.0, 3.0, items), (P, 1))
    a, k, f, c = (xs[:, i:i + 1] for i in range(4))
    e = np.exp(-k * t)
    y0 = a * e * np.sin(f * t + hdr[:, 1:2]) + c
    y1 = np.arctan2(a * e * np.cos(f * t + hdr[:, 1:2]), 1.0 + c ** 2)
    y0 = y0 + 1e-3 * rng.uniform(-1, 1, y0.shape)
    y1 = y1 + 1e-3 * rng.uniform(-1, 1, y1.shape)
    data = torch.from_numpy(np.stack([t, y0, y1], axis=2)).cuda()
    x0 = xs + 0.05 * rng.uniform(-1, 1, xs.shape)
    kw = dict(n=4, item_scalars=3, residuals_per_item=2, header_scalars=2, dtype=torch.float64)
    iters = {}
    for diff in ("central", "ad"):
        model = _res(ta, body, diff=diff, **kw).bind(data, torch.from_numpy(hdr).cuda())
        for loss in (None, "huber"):
            x = torch.from_numpy(x0.copy()).cuda()
            out = ta.Optimize(x, model.with_loss("huber", 0.05) if loss else model, ta.Options())
            torch.cuda.synchronize()
            iters[(diff, loss)] = out.num_iters.cpu().numpy()
            err = np.abs(x.cpu().numpy() - xs).max()
            print(f"diff={diff} loss={loss}: iterations {iters[(diff, loss)].tolist()} max |x - x_planted| {err:.3e}")
            assert bool((out.stop_reason >= 0).all())
            assert err < 5e-3


# ---- gradient descent: the quartic of tests/test_gpu_gd.py as kind="cost", diff="central" ---------------------------------------
def test_gd_quartic_with_central_differences(ta):
    """tests/unconstrained.cpp:19-42 over 64 problems, fp64, 1000 iterations: the trajectory against tests/gd_reference.py driven by
    the restated numeric gradient (NumEval on the cost, kCentral, h = FloatEpsilon), with test_quartic_trajectories' fp64 tolerances."""
    dtype, P = np.float64, 64
    x0 = np.linspace(38.0, 46.0, P).astype(dtype)[:, None]
    o = ta.Options()
    o.solver_type = ta.Options.GradientDescent
    o.hessian.save_last = False
    o.max_iters, o.min_error, o.min_rerr_dec = 1000, 0.0, 0.0
    o.gd.lr = 0.01
    res = _res(ta, "const S y = x[0] - p[0]; c = (T(3) * y * y + y * y * y * y) - T(2);", n=1, item_scalars=1, dtype=torch.float64, kind="cost",
               diff="central")
    model = res.bind(torch.full((P, 1, 1), 42.0, dtype=torch.float64, device="cuda"))
    x = torch.from_numpy(x0.copy()).cuda()
    out = ta.Optimize(x, model, o, history=True)
    torch.cuda.synchronize()

    def f(p, xx):
        cost = lambda v: gr.quartic(v, dtype)[0]  # noqa: E731
        c, J = nd.num_eval(cost, xx, nd.CENTRAL, None, dtype)
        return c[0], J[0]
    ref = gr.gd_optimize(x0, f, o.to_pod(), 0.01, dtype)
    g = gpu_dict(out, x)
    print("max |x - x_ref|", np.abs(g["x"] - ref["x"]).max(), "iters equal", (g["iters"] == ref["iters"]).all(),
          "max |errs - ref|", np.abs(g["errs"] - ref["errs"]).max())
    assert (g["stop"] == ref["stop"]).all(), (g["stop"], ref["stop"])
    assert (g["iters"] == ref["iters"]).all()
    assert (g["succ"] == ref["succ"]).all()
    assert (g["fails"] == ref["fails"]).all()
    assert np.allclose(g["errs"], ref["errs"], rtol=1e-10, atol=1e-10)
    assert np.allclose(g["cost"], ref["cost"], rtol=1e-10, atol=1e-10)
    assert np.abs(g["x"] - ref["x"]).max() < 1e-9
    assert out.final_hessian is None


# ---- the checker ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_check_gradient_exact_and_flipped_sign(ta, dtype):
    """The exact dyadic case (n = 20, hand-written Jacobian; eps = 10 * 2^-6 so that the twin's step eps / 10 is dyadic): passes with
    both distances exactly 0.  Column 7 with the wrong sign: no problem passes, and the distances are exactly
    2 |sum_i J_i7 r_i| and 2 max_{k != 7} |H_7k|."""
    n, eps = 20, 10 * H6
    assert eps / 10.0 == H6
    c = exact_case(n, 1)
    e = c["cases"][False]
    kw = dict(n=n, item_scalars=n + 1, dtype=TDT[dtype], kind="accumulate")
    data, x = torch.from_numpy(c["data"].astype(dtype)).cuda(), torch.from_numpy(c["x"].astype(dtype)).cuda()
    for method in ("central", "forward", "fast_central"):   # (a linear residual: all three are exact)
        chk = ta.CheckGradient(_res(ta, linear_body(n, 1, "accumulate"), **kw).bind(data), x, eps=eps, method=method)
        torch.cuda.synchronize()
        assert chk.all() and bool((chk.max_dist_g == 0).all()) and bool((chk.max_dist_H == 0).all())
    chk = ta.CheckGradient(_res(ta, linear_body(n, 1, "accumulate", flip=7), **kw).bind(data), x, eps=eps)
    torch.cuda.synchronize()
    want_g = np.array([float(2 * abs(e["g"][p][7])) for p in range(c["P"])])
    want_H = np.array([float(2 * max(abs(e["H"][p][7][k]) for k in range(n) if k != 7)) for p in range(c["P"])])
    assert (np.maximum(want_g, want_H) >= eps).all()   # (the data make the error visible)
    assert not bool(chk.ok.any())
    assert np.array_equal(chk.max_dist_g.cpu().numpy(), want_g) and np.array_equal(chk.max_dist_H.cpu().numpy(), want_H)
    chk = ta.CheckGradient(_res(ta, linear_body(n, 1, "accumulate", flip=7), **kw).bind(data), x, eps=eps, check_H=False)
    torch.cuda.synchronize()
    assert bool((chk.max_dist_H == 0).all()) and np.array_equal(chk.ok.cpu().numpy(), want_g < eps)


def test_check_gradient_of_a_cost_with_its_own_gradient(ta):
    """kind="cost_grad": logistic regression (n = 12, the body of tools/gd_probe.py) passes at the default eps in fp64; with one
    term of the gradient dropped it does not."""
    n, P, items = 12, 5, 200
    rng = np.random.default_rng(11)
    A = rng.standard_normal((P, items, n)) / np.sqrt(n)
    yl = np.where(rng.standard_normal((P, items)) > 0, 1.0, -1.0)
    data = torch.from_numpy(np.concatenate([A, yl[:, :, None]], axis=2)).cuda()
    x = torch.from_numpy(0.3 * rng.standard_normal((P, n))).cuda()
    good = (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j]; const T yy = p[{n}]; const T e = exp(-yy * z);\n"
            f"c = log(T(1) + e);\n"
            f"if (want_grad) {{ const T s = -yy * e / (T(1) + e); for (int j = 0; j < {n}; ++j) G[j] += s * p[j]; }}")
    kw = dict(n=n, item_scalars=n + 1, dtype=torch.float64, kind="cost_grad")
    chk = ta.CheckGradient(_res(ta, good, **kw).bind(data), x)
    torch.cuda.synchronize()
    print("cost_grad max_dist_g", chk.max_dist_g.cpu().numpy())
    assert chk.all() and chk.eps == 1e-5 and bool((chk.max_dist_H == 0).all())
    dropped = good.replace(f"for (int j = 0; j < {n}; ++j) G[j]", f"for (int j = 0; j < {n - 1}; ++j) G[j]")
    assert dropped != good
    bad = ta.CheckGradient(_res(ta, dropped, **kw).bind(data), x)
    torch.cuda.synchronize()
    assert not bool(bad.ok.any())
    # the distance is the dropped term itself: |g_11| of the full gradient (to the accuracy of the differences)
    g_full = ta.accumulate(_res(ta, good, **kw).bind(data), x)[0].cpu().numpy()
    assert np.allclose(bad.max_dist_g.cpu().numpy(), np.abs(g_full[:, n - 1]), atol=1e-5)


@pytest.mark.parametrize("dtype,method", [(np.float32, "forward"), (np.float64, "fast_central")])
def test_check_gradient_of_a_wide_cost_forward_and_fast_central(ta, dtype, method):
    """NumCostFunctor beyond twelve parameters (n = 20: two chunks of ten columns), with forward and fast central differences and in
    fp32: the logistic cost_grad body passes; with the LAST gradient term (second chunk) dropped it fails by that term.
    eps: the default in fp64, 1e-1 in fp32 (step 1e-2).  That the good body must pass is worked out from the data, not observed:
      truncation  forward differences of c(z) = log(1 + exp(-y z)), |c''| <= 1/4: at most h / 8 * sum_i p_ij^2 in column j
                  (the central forms are O(h^2) and below that);
      rounding    one evaluation of c is off by at most u (n S + 8): the n-term dot product z (|dc/dz| < 1, S >= sum_j |p_j| (|x_j| + h))
                  and a few ulp of exp / log / the sum at c < 2; a quotient carries two of them over h, an item each;
                  the sums over the items, of the body's own gradient and of the quotients (terms below 1, a handful of
                  roundings each, partial sums below the item count): items u (16 + items) each."""
    n, P, items = 20, 3, 40
    rng = np.random.default_rng(23)
    A = rng.standard_normal((P, items, n)) / np.sqrt(n)
    yl = np.where(rng.standard_normal((P, items)) > 0, 1.0, -1.0)
    A[:, :, n - 1] = yl * (0.1 + np.abs(A[:, :, n - 1]))      # every item pulls the last gradient term the same way: it cannot cancel
    xs = 0.3 * rng.standard_normal((P, n))
    A, xs = A.astype(dtype).astype(np.float64), xs.astype(dtype).astype(np.float64)
    eps = 1e-1 if dtype == np.float32 else 1e-5
    h, u = eps / 10.0, float(np.finfo(dtype).eps)
    z = np.einsum("pij,pj->pi", A, xs)
    assert (np.log1p(np.exp(np.abs(z) + h)) < 2).all()
    S = (np.abs(A) * (np.abs(xs)[:, None, :] + h)).sum(axis=2).max()
    bound = h / 8 * (A * A).sum(axis=1).max() + items * 2 * u * (n * S + 8) / h + 2 * items * u * (16 + items)
    g_last = -(yl * A[:, :, n - 1] / (1.0 + np.exp(yl * z))).sum(axis=1)   # the full gradient's last term, in fp64 on the CPU
    print(f"{dtype.__name__} {method}: worked-out bound {bound:.3e} against eps {eps:g}; |g_last| {np.abs(g_last)}")
    assert bound < eps and (np.abs(g_last) > 2 * eps).all()
    data = torch.from_numpy(np.concatenate([A, yl[:, :, None]], axis=2).astype(dtype)).cuda()
    x = torch.from_numpy(xs.astype(dtype)).cuda()
    good = (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j]; const T yy = p[{n}]; const T e = exp(-yy * z);\n"
            f"c = log(T(1) + e);\n"
            f"if (want_grad) {{ const T s = -yy * e / (T(1) + e); for (int j = 0; j < {n}; ++j) G[j] += s * p[j]; }}")
    kw = dict(n=n, item_scalars=n + 1, dtype=TDT[dtype], kind="cost_grad")
    chk = ta.CheckGradient(_res(ta, good, **kw).bind(data), x, eps=eps, method=method)
    torch.cuda.synchronize()
    print("max_dist_g", chk.max_dist_g.cpu().numpy())
    assert chk.all() and bool((chk.max_dist_g < bound).all()) and bool((chk.max_dist_H == 0).all())
    dropped = good.replace(f"for (int j = 0; j < {n}; ++j) G[j]", f"for (int j = 0; j < {n - 1}; ++j) G[j]")
    assert dropped != good
    bad = ta.CheckGradient(_res(ta, dropped, **kw).bind(data), x, eps=eps, method=method)
    torch.cuda.synchronize()
    assert not bool(bad.ok.any())
    assert (np.abs(bad.max_dist_g.cpu().numpy() - np.abs(g_last)) < bound).all()


def test_check_gradient_of_an_ad_model_fp32_default_eps(ta):
    """A kind="residual" model (Jets) against its numeric twin, fp32, default eps = 1e-2 (step 1e-3): the circle fit of
    tests/circle.cpp:32-68 on a small circle, away from the solution."""
    P, items = 4, 6
    rng = np.random.default_rng(2)
    ang = np.linspace(0, 2 * np.pi, items, endpoint=False)[None, :] + rng.uniform(0, 1, (P, 1))
    obs = np.stack([0.25 + 0.5 * np.cos(ang), 0.5 + 0.5 * np.sin(ang)], -1).astype(np.float32)
    x = torch.tensor(np.tile(np.array([0.2, 0.4, 0.4], np.float32), (P, 1))).cuda()
    res = _res(ta, "const S dx = p[0] - x[0];\nconst S dy = p[1] - x[1];\nr[0] = dx * dx + dy * dy - x[2] * x[2];", n=3, item_scalars=2,
               dtype=torch.float32)
    chk = ta.CheckGradient(res.bind(torch.from_numpy(obs).cuda()), x)
    torch.cuda.synchronize()
    print("AD fp32 max_dist_g", chk.max_dist_g.cpu().numpy(), "max_dist_H", chk.max_dist_H.cpu().numpy())
    assert chk.eps == 1e-2 and chk.all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ta):
    def refused(code, text, *a, **kw):
        with pytest.raises(ta.ToaError) as e:
            ta.JitResidual(*a, **kw)
        assert f"error {code}:" in str(e.value) and text in str(e.value), str(e.value)
    own = "a TOA_JIT_ACCUMULATE / TOA_JIT_COST_GRAD body brings its own derivatives"
    refused(E_ARG, own, "r[0] = x[0]; if (want_grad) { J[0][0] = T(1); }", n=1, item_scalars=0, kind="accumulate", diff="central")
    refused(E_ARG, own, "c = x[0]; if (want_grad) { G[0] += T(1); }", n=1, item_scalars=0, kind="cost_grad", diff="forward")
    euclid = "is for Euclidean parameters (manifold = TOA_MANIFOLD_EUCLID)"
    refused(E_UNSUPPORTED, euclid, "r[0] = x[9];", n=6, item_scalars=0, header_scalars=12, manifold="se3", diff="central")
    refused(E_UNSUPPORTED, euclid, "r[0] = x[0];", n=1, item_scalars=0, manifold="user", plus_body="xp[0] = x[0] + d[0];", x_scalars=1,
            diff="fast_central")
    refused(E_ARG, "diff_h must be finite and >= 0", "r[0] = x[0];", n=1, item_scalars=0, diff="central", diff_h=-1.0)
    refused(E_ARG, "diff_h must be finite and >= 0", "r[0] = x[0];", n=1, item_scalars=0, diff="central", diff_h=float("inf"))
    with pytest.raises(ValueError, match="unknown diff 'backward'"):
        ta.JitResidual("r[0] = x[0];", n=1, item_scalars=0, diff="backward")

    # the row-split and the stepping forms
    res = _res(ta, "r[0] = x[0] - p[0];", n=1, item_scalars=1, dtype=torch.float64, diff="central")
    P, items = 2, 4
    model = res.bind(torch.ones(P, items, 1, dtype=torch.float64, device="cuda"))
    x = torch.zeros(P, 1, dtype=torch.float64, device="cuda")
    ctx = default_context()
    from tinyopt_amd.api import _alloc_output, _results_pod
    o = ta.Options()
    pod, out = o.to_pod(), _alloc_output(P, 1, o, False, x.device)
    r = _results_pod(out)
    text = b"a numerically differentiated model (toa_jit_spec::diff = TOA_DIFF_NUM_*) has no row-split and no stepping form"
    rc = ctx.lib.toa_jit_lm_run_split(ctx.h, res._h, items, P, model.packed.data_ptr(), x.data_ptr(), C.byref(pod), C.byref(r), None, 0)
    assert rc == E_UNSUPPORTED and text in ctx.lib.toa_last_error()
    state = torch.zeros(max(int(ctx.lib.toa_lm_state_bytes(1, 1, P)), 1), dtype=torch.uint8, device="cuda")
    rc = ctx.lib.toa_jit_lm_begin(ctx.h, res._h, items, P, model.packed.data_ptr(), x.data_ptr(), C.byref(pod), C.byref(r), state.data_ptr())
    assert rc == E_UNSUPPORTED and text in ctx.lib.toa_last_error()
    # Python: host controls and splits, before any launch
    one_launch = r"a numerically differentiated model \(diff=\.\.\.\) runs as one launch per solve"
    with pytest.raises(ValueError, match=one_launch):
        ta.Optimize(x, model, ta.Options(), splits=2)
    oc = ta.Options()
    oc.max_duration_ms = 10.0
    with pytest.raises(ValueError, match=one_launch):
        ta.Optimize(x, model, oc)
    oc = ta.Options()
    oc.stop_callback = lambda err, dx2, g2: False
    with pytest.raises(ValueError, match=one_launch):
        ta.Optimize(x, model, oc)
    with pytest.raises(ValueError, match=r"a numerically differentiated model \(diff=\.\.\.\) has no stepping form"):
        ta.Optimizer(x, model, ta.Options())
    # ... and the plain run is served (never by the automatic row-split route: two problems of 600 residuals)
    big = res.bind(torch.full((P, 600, 1), 3.0, dtype=torch.float64, device="cuda"))
    outb = ta.Optimize(x, big, ta.Options())
    torch.cuda.synchronize()
    assert bool((outb.stop_reason >= 0).all()) and np.abs(x.cpu().numpy() - 3.0).max() < 1e-6
    # the checker: method, manifold
    dist = torch.zeros(P, 2, dtype=torch.float64, device="cuda")
    rc = ctx.lib.toa_jit_check_gradient(ctx.h, res._h, items, P, model.packed.data_ptr(), x.data_ptr(), 0.0, 0, 1, dist.data_ptr(), None)
    assert rc == E_ARG and b"method must be" in ctx.lib.toa_last_error()


def test_checker_names_a_body_that_uses_x_as_a_pointer(ta):
    """A hand-written body is checkable when it reads the parameters only as x[j]: its twin sees x as an accessor.  One that takes x
    as a pointer runs, and the checker's refusal says why and carries the compiler's log."""
    res = ta.JitResidual("const T* xx = x; r[0] = xx[0] - p[0]; if (want_grad) { J[0][0] = T(1); }", n=1, item_scalars=1, dtype=torch.float64,
                         kind="accumulate")
    model = res.bind(torch.full((2, 3, 1), 2.0, dtype=torch.float64, device="cuda"))
    x = torch.ones(2, 1, dtype=torch.float64, device="cuda")
    g = ta.accumulate(model, x)[0]
    torch.cuda.synchronize()
    assert np.array_equal(g.cpu().numpy(), np.full((2, 1), -3.0))
    with pytest.raises(ta.ToaError) as e:
        ta.CheckGradient(model, x)
    msg = str(e.value)
    assert f"error {E_ARG}:" in msg and "numeric twin does not build" in msg and "only as x[j]" in msg
    assert "accumulate_body" in msg and "error:" in msg   # (hiprtc's log: the line of the body)


def test_checker_is_refused_under_capture_until_its_twin_exists(ta):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res = ta.JitResidual("r[0] = x[0] * x[0] - p[0];  // capture test of the checker: a text of its own", n=1, item_scalars=1, dtype=torch.float64)
        model = res.bind(torch.full((3, 2, 1), 2.0, dtype=torch.float64, device="cuda"))
        x = torch.ones(3, 1, dtype=torch.float64, device="cuda")
        ta.accumulate(model, x)   # (warms the context of this stream)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(Exception, match="its numeric twin is compiled the first time .* cannot happen while the stream is being captured"):
            with torch.cuda.graph(g, stream=s):
                ta.CheckGradient(model, x)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        chk = ta.CheckGradient(model, x)
        s.synchronize()
        assert chk.all()
