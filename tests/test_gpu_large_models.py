"""Run-time models beyond 63 parameters (JitResidual(..., large_n=True); csrc/large_model_rows.hpp on the launch-per-phase pipeline
of csrc/large_n.hip): the rows and the Accumulate seam bit for bit on dyadic problems, LM trajectories against the oracle and
against DenseRowNatural, the same text through both routes, items of several residuals with a header, lanes and data strides,
failure modes, and what such a model refuses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_reference as er  # noqa: E402
from parity import check_trajectories, gpu_dict  # noqa: E402
from test_gpu_eval import Guarded  # noqa: E402
from test_gpu_row_models import _two_rows_manual, ad_body, manual_body  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {np.float32: torch.float32, np.float64: torch.float64}
# (n, kR, items): n = 100, 129 are no multiple of the Jet chunk, n = 65, 129 none of the 16-byte vector; 33, 40, 24 items end inside a super-step
SHAPES = [(64, 1, 70), (65, 2, 33), (100, 1, 130), (128, 1, 200), (129, 3, 40), (144, 1, 96), (256, 1, 150), (512, 1, 24), (1024, 1, 40)]
_RES, _CASE = {}, {}


def _res(ta, body, **kw):
    key = (body, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _RES:
        _RES[key] = ta.JitResidual(body, **kw)
    return _RES[key]


def _cases():
    return [pytest.param(n, kR, items, dt, id=f"{n}-{kR}-{items}-{'f32' if dt == np.float32 else 'f64'}")
            for (n, kR, items) in SHAPES for dt in (np.float32, np.float64) if not (n == 1024 and dt == np.float64)]


def _dyadic(n, kR, items):
    """The dyadic problem of a shape and its exact rows (float64), computed once and shared."""
    key = (n, kR, items)
    if key not in _CASE:
        data, x = er.dyadic_case(n, kR, items, P=3)
        r, J = er.linear_rows(data, x, n, np.float64)
        _CASE[key] = (data, x, r, J)
    return _CASE[key]


def _linear_model(ta, n, kR, items, kind, dtype):
    data, x, r, J = _dyadic(n, kR, items)
    res = _res(ta, er.linear_body(n, kR, kind), n=n, item_scalars=kR * (n + 1), residuals_per_item=kR, dtype=TDT[dtype], kind=kind, large_n=True)
    model = res.bind(torch.from_numpy(data.astype(dtype)).cuda())
    return model, torch.from_numpy(x.astype(dtype)).cuda(), r, J


def _eval_guarded(ta, model, x, res=True, jac=True):
    P = x.shape[0]
    gr = Guarded((P, model.m), x.dtype) if res else None
    gj = Guarded((P, model.m, model.n), x.dtype) if jac else None
    if res:
        ta.Eval(model, x, jac=jac, res_out=gr.view, J_out=gj.view if jac else None)
    else:
        ta.CalculateJac(model, x, J_out=gj.view)
    torch.cuda.synchronize()
    assert gr is None or gr.intact(), "res: a sentinel was overwritten"
    assert gj is None or gj.intact(), "J: a sentinel was overwritten"
    return (gr.numpy() if res else None), (gj.numpy() if jac else None)


# ---- 1. rows, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["accumulate", "residual"])
@pytest.mark.parametrize("n,kR,items,dtype", _cases())
def test_rows_bit_for_bit(ta, n, kR, items, dtype, kind):
    """Eval (both, J alone, res alone) of the linear body over multiples of 1/8 equals exact arithmetic cast to the dtype — every
    partial sum is exact in fp32 in any order at these shapes — and no scalar outside the outputs is written."""
    model, x, r, J = _linear_model(ta, n, kR, items, kind, dtype)
    r, J = r.astype(dtype), J.astype(dtype)
    rg, Jg = _eval_guarded(ta, model, x)
    assert rg.dtype == dtype and Jg.dtype == dtype and rg.shape == r.shape and Jg.shape == J.shape
    assert np.array_equal(rg, r), f"res differs in {int((rg != r).sum())} places, max {np.abs(rg - r).max()}"
    assert np.array_equal(Jg, J), f"J differs in {int((Jg != J).sum())} places, max {np.abs(Jg - J).max()}"
    _, Jj = _eval_guarded(ta, model, x, res=False)
    rr, none = _eval_guarded(ta, model, x, jac=False)
    assert none is None and np.array_equal(Jj, J) and np.array_equal(rr, r)


# ---- 2. the seam, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["accumulate", "residual"])
@pytest.mark.parametrize("n,kR,items,dtype", _cases())
def test_seam_bit_for_bit(ta, n, kR, items, dtype, kind):
    """ta.accumulate on the same problems: g = J^T r and H = J^T J of the exact rows are exact in the dtype too (fp32: partial sums
    <= 4.8e5 and <= 2.2e4 units of their grain against 2^24), so the per-wave J^T r partials, the fp32 Gram over the padded J (odd n)
    and the fp64 Gram must reproduce numpy's bits; H symmetric bit for bit; nres = m; the cost-only pass gives the same cost."""
    model, x, r, J = _linear_model(ta, n, kR, items, kind, dtype)
    g, H, c, nres = ta.accumulate(model, x)
    c0 = ta.accumulate(model, x, want_grad=False)[2]
    torch.cuda.synchronize()
    g_ref = np.einsum("pmj,pm->pj", J, r).astype(dtype)
    H_ref = np.einsum("pmi,pmj->pij", J, J).astype(dtype)
    c_ref = (r * r).sum(1)
    gg, Hg, cg = g.cpu().numpy(), H.cpu().numpy(), c.cpu().numpy()
    assert np.array_equal(gg, g_ref), f"g differs in {int((gg != g_ref).sum())} places, max {np.abs(gg - g_ref).max()}"
    assert np.array_equal(Hg, H_ref), f"H differs in {int((Hg != H_ref).sum())} places, max {np.abs(Hg - H_ref).max()}"
    assert np.array_equal(Hg, np.swapaxes(Hg, 1, 2))
    assert (nres.cpu().numpy() == model.m).all()
    print("cost", cg, c_ref)
    if dtype == np.float64:
        assert np.array_equal(cg, c_ref)
    else:
        assert np.abs(cg - c_ref).max() <= 1e-6 * np.abs(c_ref).max()
    assert np.array_equal(c0.cpu().numpy(), cg)


# ---- 3. trajectories ----------------------------------------------------------------------------------------------------------------
def _items(A, b):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([A, b[..., None]], -1))).cuda()


TRAJ = [(np.float64, 64, 300, "accumulate"), (np.float32, 65, 259, "accumulate"), (np.float32, 96, 400, "accumulate"), (np.float64, 100, 333, "accumulate"),
        (np.float32, 128, 600, "accumulate"), (np.float64, 130, 400, "accumulate"), (np.float32, 144, 600, "accumulate"), (np.float32, 256, 700, "accumulate"),
        (np.float64, 100, 333, "residual"), (np.float32, 144, 600, "residual")]


@pytest.mark.parametrize("dtype,n,m,kind", TRAJ)
def test_trajectories_against_the_oracle_and_the_natural_family(ta, oracle, dtype, n, m, kind):
    """The DenseRow residual as text on the large-n route: the LM trajectory equals the oracle's under the benchmark options and the
    defaults, and the solve lands where DenseRowNatural — the compiled-in family on the same rows — lands."""
    P = 4
    A, b, x0, _ = oracle.synth_dense_row(P, n, m, dtype, seed=900 + n + m)
    body = manual_body(n) if kind == "accumulate" else ad_body(n)
    model = _res(ta, body, n=n, item_scalars=n + 1, dtype=TDT[dtype], kind=kind, large_n=True).bind(_items(A, b))
    xtol = 1e-8 if dtype == np.float64 else 2e-3
    for opts in (ta.Options.benchmark(), ta.Options()):
        ref = oracle.dense_row_lm(A, b, x0, opts.to_pod(), history=True)
        x = torch.from_numpy(x0.copy()).cuda()
        out = ta.Optimize(x, model, opts, history=True)
        torch.cuda.synchronize()
        st = check_trajectories(gpu_dict(out, x), ref, dtype, opts.to_pod(), label=f"large-n {kind} n = {n}")
        assert st["full"] + st["ties"] == P
        xb = torch.from_numpy(x0.copy()).cuda()
        outb = ta.Optimize(xb, ta.DenseRowNatural(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()), opts, history=True)
        torch.cuda.synchronize()
        assert float((x - xb).abs().max()) <= xtol * max(1.0, float(xb.abs().max()))
        if dtype == np.float64:
            assert torch.equal(out.num_iters, outb.num_iters) and torch.equal(out.stop_reason, outb.stop_reason)


# ---- 4. the same text, both routes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["accumulate", "residual"])
def test_same_text_through_both_routes(ta, oracle, kind):
    n, m, P = 50, 400, 6
    A, b, x0, _ = oracle.synth_dense_row(P, n, m, np.float64, seed=77)
    body = manual_body(n) if kind == "accumulate" else ad_body(n)
    kw = dict(n=n, item_scalars=n + 1, dtype=torch.float64, kind=kind)
    opts = ta.Options()
    xs, outs = [], []
    for large in (False, True):
        model = _res(ta, body, large_n=large, **kw).bind(_items(A, b))
        x = torch.from_numpy(x0.copy()).cuda()
        outs.append(ta.Optimize(x, model, opts, history=True))
        xs.append(x)
    torch.cuda.synchronize()
    assert float((xs[0] - xs[1]).abs().max()) <= 1e-9
    assert torch.equal(outs[0].num_iters, outs[1].num_iters) and torch.equal(outs[0].stop_reason, outs[1].stop_reason)
    Ha, Hb = outs[0].final_hessian, outs[1].final_hessian
    assert float((Ha - Hb).abs().max()) <= 1e-10 * float(Ha.abs().max())


# ---- 5. several residuals and a header ----------------------------------------------------------------------------------------------
def test_two_residuals_per_item_and_a_header(ta, oracle):
    n, items, P = 72, 150, 4
    m = 2 * items
    A, b, x0, _ = oracle.synth_dense_row(P, n, m, np.float64, seed=372)
    body = _two_rows_manual(n).replace("r[0] = t", "r[0] = h[0] * t").replace("r[1] = u", "r[1] = h[0] * u")
    body = body.replace("const T s0 = T(1)", "const T s0 = h[0] * T(1)").replace(", s1 = T(1)", ", s1 = h[0] * T(1)")
    fit = _res(ta, body, n=n, item_scalars=2 * n + 2, residuals_per_item=2, header_scalars=1, dtype=torch.float64, kind="accumulate", large_n=True)
    item = np.concatenate([A[:, 0::2], A[:, 1::2], b[:, 0::2, None], b[:, 1::2, None]], -1)
    model = fit.bind(torch.from_numpy(np.ascontiguousarray(item)).cuda(), header=torch.ones(P, 1, dtype=torch.float64, device="cuda"))
    opts = ta.Options.benchmark()
    ref = oracle.dense_row_lm(A, b, x0, opts.to_pod(), history=True)
    x = torch.from_numpy(x0.copy()).cuda()
    out = ta.Optimize(x, model, opts, history=True)
    torch.cuda.synchronize()
    st = check_trajectories(gpu_dict(out, x), ref, np.float64, opts.to_pod(), label="two rows per item and a header, n = 72")
    assert st["full"] + st["ties"] == P


# ---- 6. lanes and strides -----------------------------------------------------------------------------------------------------------
def test_lanes_and_strides(ta, oracle):
    """Twenty problems run as two lanes (the second one's data begins at ten data strides), every one against the oracle; twice, and
    with the memo of linearisations off: the same bits.
    With 80 rows for 64 parameters the final cost (~5e-6) is a sum of squares of residuals of ~2.5e-4, each a difference of O(1)
    fp32 numbers: the ORACLE's own fp32 cost at its own final x is off the float64 cost of that x by up to 7.3e-4 relative (median
    2.2e-4; computed on the CPU for this seed).  Two fp32 evaluations may therefore differ by 1.5e-3; the costs are compared to 3e-3
    (parity.py's fp32 default of 5e-4 is sized for m ~ 10^3 noise-dominated residuals)."""
    P, n, m = 20, 64, 80
    A, b, x0, _ = oracle.synth_dense_row(P, n, m, np.float32, seed=64)
    model = _res(ta, manual_body(n), n=n, item_scalars=n + 1, dtype=torch.float32, kind="accumulate", large_n=True).bind(_items(A, b))
    opts = ta.Options.benchmark()
    ref = oracle.dense_row_lm(A, b, x0, opts.to_pod(), history=True)
    x = torch.from_numpy(x0.copy()).cuda()
    out = ta.Optimize(x, model, opts, history=True)
    torch.cuda.synchronize()
    st = check_trajectories(gpu_dict(out, x), ref, np.float32, opts.to_pod(), tol=dict(err_rtol=3e-3, floor_rtol=3e-3, cost_rtol=3e-3), label="two lanes")
    assert st["full"] + st["ties"] == P
    x2 = torch.from_numpy(x0.copy()).cuda()
    out2 = ta.Optimize(x2, model, opts, history=True)
    x3 = torch.from_numpy(x0.copy()).cuda()
    with ta.api.default_context().tuning(memo_off=1):
        out3 = ta.Optimize(x3, model, opts, history=True)
    torch.cuda.synchronize()
    assert torch.equal(x2, x) and torch.equal(out2.errs, out.errs) and torch.equal(out2.num_iters, out.num_iters)
    assert torch.equal(x3, x) and torch.equal(out3.errs, out.errs) and torch.equal(out3.num_iters, out.num_iters)


# ---- 7. failure modes ---------------------------------------------------------------------------------------------------------------
def test_failure_modes(ta, oracle):
    P, n, m = 3, 70, 200
    A, b, x0, _ = oracle.synth_dense_row(P, n, m, np.float64)
    fit = _res(ta, manual_body(n), n=n, item_scalars=n + 1, dtype=torch.float64, kind="accumulate", large_n=True)
    A2 = A.copy()
    A2[1, 5, 3] = np.nan
    out = ta.Optimize(torch.from_numpy(x0.copy()).cuda(), fit.bind(_items(A2, b)), ta.Options())
    stop = out.stop_reason.cpu().numpy()
    assert stop[1] == int(ta.StopReason.kSystemHasNaNOrInf) and stop[0] >= 0 and stop[2] >= 0
    A3 = A.copy()
    A3[2, :, 7] = 0.0   # a zero column: J^T J singular; Gauss-Newton has no damping to repair it
    o = ta.Options()
    o.solver_type = ta.Options.GaussNewton
    out = ta.Optimize(torch.from_numpy(x0.copy()).cuda(), fit.bind(_items(A3, b)), o)
    stop = out.stop_reason.cpu().numpy()
    assert stop[2] == int(ta.StopReason.kSolverFailed) and stop[0] >= 0 and stop[1] >= 0


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_stats(ta):
    lin = er.linear_body(64, 1, "residual")
    kw = dict(n=64, item_scalars=65, dtype=torch.float32)
    with pytest.raises(ta.ToaError, match="large_n"):
        ta.JitResidual(lin, large_n=False, **kw)   # without the flag: refused as before
    with pytest.raises(ValueError, match="no scalar costs"):
        ta.JitResidual("c = x[0];", kind="cost", large_n=True, **kw)
    with pytest.raises(ValueError, match="Euclidean parameters only"):
        ta.JitResidual(lin, manifold="user", plus_body="for (int i = 0; i < 64; ++i) xp[i] = x[i] + d[i];", x_scalars=64, large_n=True, **kw)
    with pytest.raises(ValueError, match='diff="ad" only'):
        ta.JitResidual(lin, diff="central", large_n=True, **kw)
    with pytest.raises(ValueError, match="<= 512 in float64"):
        ta.JitResidual(lin, n=513, item_scalars=514, dtype=torch.float64, large_n=True)
    with pytest.raises(ValueError, match="1 <= n <= 1024"):
        ta.JitResidual(lin, n=1025, item_scalars=8, dtype=torch.float32, large_n=True)
    with pytest.raises(ValueError, match="item_scalars <= 2048"):
        ta.JitResidual(lin, n=64, item_scalars=2049, dtype=torch.float32, large_n=True)
    with pytest.raises(ta.ToaError, match="does not fit the rows kernel's LDS"):
        ta.JitResidual(lin, n=512, item_scalars=2048, residuals_per_item=8, dtype=torch.float64, large_n=True)
    res = _res(ta, lin, kind="residual", large_n=True, **kw)
    st = res.stats()
    assert st["num_regs"] > 0 and st["lds_bytes_per_wg"] > 0 and st["wg_per_cu"] >= 1 and st["scratch_bytes"] >= 0
    data, x = er.dyadic_case(64, 1, 70, P=3)
    dd, xx = torch.from_numpy(data.astype(np.float32)).cuda(), torch.from_numpy(x.astype(np.float32)).cuda()
    model = res.bind(dd)
    with pytest.raises(ValueError, match="no M-estimator"):
        model.with_loss("huber", 1.0)
    ctx = ta.api.default_context()
    ta.api.check(ctx.lib.toa_set_loss(ctx.h, 1, 1.0))   # a handle with a loss set, past the Python layer
    try:
        with pytest.raises(ta.ToaError, match="M-estimator"):
            g = torch.zeros(3, 64, device="cuda")
            H = torch.zeros(3, 64, 64, device="cuda")
            c = torch.zeros(3, dtype=torch.float64, device="cuda")
            ta.api.check(ctx.lib.toa_jit_accumulate(ctx.h, res._h, 70, 3, model.packed.data_ptr(), xx.data_ptr(), 1, g.data_ptr(), H.data_ptr(),
                                                    c.data_ptr(), None))
    finally:
        ta.api.check(ctx.lib.toa_set_loss(ctx.h, 0, 0.0))
    with pytest.raises(ValueError, match="no Gaussian prior"):
        model.with_prior(torch.zeros(3, 64, device="cuda"), torch.ones(3, 64, device="cuda"))
    with pytest.raises(ValueError, match="no ragged batches"):
        res.bind_ragged(dd.reshape(-1, 65), counts=[70, 70, 70])
    with pytest.raises(ValueError, match="no row-split form"):
        ta.Optimize(xx.clone(), model, ta.Options(), splits=2)
    with pytest.raises(ValueError, match="no stepping form \\(Optimizer\\)"):
        ta.Optimizer(xx.clone(), model, ta.Options())
    o = ta.Options()
    o.max_duration_ms = 5.0
    with pytest.raises(ValueError, match="no host controls"):
        ta.Optimize(xx.clone(), model, o)
    o = ta.Options()
    o.stop_callback = lambda err, dx2, g2: False
    with pytest.raises(ValueError, match="no host controls"):
        ta.Optimize(xx.clone(), model, o)
    o = ta.Options()
    o.solver_type = ta.Options.GradientDescent
    with pytest.raises(ValueError, match="no GradientDescent"):
        ta.Optimize(xx.clone(), model, o)
    with pytest.raises(ValueError, match="no CheckGradient"):
        ta.CheckGradient(model, xx)
    # stream capture of the solve: refused, nothing recorded (the pattern of tests/test_gpu_graph_capture.py)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xc = xx.clone()
        outc = ta.Optimize(xc, model, ta.Options.benchmark())   # eager: fine (and warms the context of this stream)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(Exception, match="no stream capture"):
            with torch.cuda.graph(graph, stream=s):
                ta.Optimize(xc, model, ta.Options.benchmark(), out=outc)
    torch.cuda.synchronize()
