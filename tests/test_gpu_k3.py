"""K3 (`toa_solve_damped`), the covariance seam (`toa_inv_cov`) and the solve inside the fused LM loop at every n, at the edges
of the 16-column panels and on the pivoted fall-back — against the derived backward-error bound n * gamma_{3n+8} and the
verdicts of the CPU oracle.  The matrices, the bound and its derivation are in tests/k3_cases.py; tests/test_cpu_k3_cases.py
shows that the oracle itself meets every condition asked here on every case used here.

What this file pins beyond test_solve_damped_spd / test_solve_damped_acceptance_rule / test_inv_cov_and_output_covariance:
  * the fast path at EVERY n <= 63 (register panel up to 16, blocked on the matrix cores beyond), also badly scaled;
  * a fast path that gives up at pivot k for k on both sides of every panel boundary, with n on both sides of every panel count:
    the image is re-created (`fill()` / `write_sym`), the pivoted routine reads the full matrix, its permutation is applied, its
    verdict is Eigen's — for an indefinite matrix (refused, dx = 0), exact zero rows (accepted, dx[k] = 0, the rest solved) and
    pivots above the fast path's upper gate (accepted);
  * a launch that mixes all fates gives every matrix the bits it gets alone;
  * the same inside the fused LM loop, whose refill is its own code (lm_device.hpp);
  * the workgroup LDL^T for 64 <= n <= 128 at its panel edges, including that it REFUSES a singular semi-definite matrix.

Measured on an MI355X, worst eta / bound (column residual / bound for the covariance):
  test_every_n                     fp32 0.041   fp64 0.091
  test_fall_back_at_every_panel    fp32 0.020   fp64 0.051
  test_inv_cov_families            fp32 0.031   fp64 0.046
  test_workgroup_ldlt_panel_edges  fp32 1.0e-4   fp64 1.2e-4
(the oracle: 0.03 / 0.06, 0.02 / 0.05, 0.03 / 0.05, 8e-5 / 1e-4).

Grid stride.  solve_damped_kernel runs four waves per workgroup on min(ceil(P / 4), 8 x CUs) workgroups, so a wave takes a
second matrix only beyond P = 32 x CUs = 8192 on an MI355X.  The mixed launches here have P <= 54: every wave solves ONE
matrix and none reaches the stride — the mixed-batch comparison shows independence of the LDS slices side by side, not
reuse of one slice in sequence (that would take > 32 000 matrices per launch).  The fused LM loop does reuse a wave's slice,
solve after solve, and test_fused_loop_takes_the_fall_back runs the fall-back in every one of its iterations."""
import numpy as np
import pytest
import torch

import k3_cases as K
from parity import TOL, check_trajectories, gpu_dict

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", K.DTYPES, ids=["f32", "f64"])


def _solve(ta, cases):
    """One launch of toa_solve_damped over cases that share n, dtype and damping factor."""
    scale = cases[0].scale
    assert all(c.scale == scale and c.n == cases[0].n and c.dtype == cases[0].dtype for c in cases)
    H, g = K.stack(cases)
    dx, ok = ta.solve_damped(torch.from_numpy(H).cuda(), torch.from_numpy(g).cuda(), scale)
    return dx.cpu().numpy(), ok.cpu().numpy()


def _oracle(oracle, cases):
    H, g = K.stack(cases)
    return oracle.solve_damped(H, g, cases[0].scale)


def _check(c, dx, ok, ok_ref, worst, want_ok=None):
    """One matrix: the verdict (Eigen's, the oracle's), exact zeros where they are promised, eta <= bound where it is solved."""
    want_ok = c.ok if want_ok is None else want_ok
    assert ok == want_ok, (c.name, c.n, "verdict", int(ok))
    if ok_ref is not None:
        assert ok == ok_ref, (c.name, c.n, "verdict differs from the oracle's", int(ok), int(ok_ref))
    assert np.isfinite(dx).all(), (c.name, c.n)
    if not want_ok:
        assert not dx.any(), (c.name, c.n, "dx of a refused solve")
        return
    assert not dx[list(c.zeros)].any(), (c.name, c.n, "dx on a zero row", dx[list(c.zeros)])
    if len(c.keep):
        r = K.eta(c, dx) / K.eta_bound(c)
        worst[0] = max(worst[0], r)
        assert r <= 1.0, (c.name, c.n, "eta / bound", r)


@DT
def test_every_n(ta, oracle, dtype):
    """n = 1 .. 63: gram at three damping factors and graded (condition 1e6 / 1e12, unfavourable order), P = 8 each."""
    worst = [0.0]
    for n in K.EVERY_N:
        for label, scale, cases in K.every_n_batches(n, dtype):
            dx, ok = _solve(ta, cases)
            _, ok_ref = _oracle(oracle, cases)
            for c, d, o, r in zip(cases, dx, ok, ok_ref):
                _check(c, d, o, r, worst)
    print(f"every n, {np.dtype(dtype).name}: worst eta / bound = {worst[0]:.3g}")


@DT
def test_fall_back_at_every_panel(ta, oracle, dtype):
    worst = [0.0]
    for n in K.PANEL_NS:
        cases = K.fall_back_cases(n, dtype)
        dx, ok = _solve(ta, cases)
        _, ok_ref = _oracle(oracle, cases)
        for c, d, o, r in zip(cases, dx, ok, ok_ref):
            _check(c, d, o, r, worst)
        # all of them and a gram matrix after each in ONE launch: every matrix gets the bits it gets alone
        mixed = K.mixed_batch(n, dtype)
        dxm, okm = _solve(ta, mixed)
        for i, c in enumerate(mixed):
            _check(c, dxm[i], okm[i], None, worst)
            d1, o1 = _solve(ta, [c])
            assert okm[i] == o1[0] and dxm[i].tobytes() == d1[0].tobytes(), (c.name, n, "mixed launch differs from the matrix alone")
    print(f"fall-back, {np.dtype(dtype).name}: worst eta / bound = {worst[0]:.3g}; "
          f"largest launch {2 * len(K.fall_back_cases(63, dtype))} matrices, grid stride {32 * ta.api.default_context().info()['num_cus']}")


def _inv_cov(ta, cases):
    C, ok = ta.inv_cov(torch.from_numpy(np.stack([c.H for c in cases])).cuda())
    return C.cpu().numpy(), ok.cpu().numpy()


@DT
def test_inv_cov_families(ta, dtype):
    """(The inverse of a `huge` matrix has subnormal off-diagonal entries in both types: its bound holds because the kernel's
    divisions and stores keep gradual underflow, as the oracle's host does.)"""
    worst = 0.0
    for n in K.INV_COV_NS:
        cases = K.inv_cov_cases(n, dtype)
        C, ok = _inv_cov(ta, cases)
        for c, Cp, o in zip(cases, C, ok):
            assert o == 1 and np.isfinite(Cp).all(), (c.name, n)
            z = list(c.zeros)
            assert not Cp[z].any() and not Cp[:, z].any(), (c.name, n, "row / column of a zero row")
            r = K.inv_cov_ratio(c, Cp)
            worst = max(worst, r)
            assert r <= 1.0, (c.name, n, "column residual / bound", r)
    for n, k in K.INV_COV_INDEFINITE:      # refused: the kernel defines the output
        good = K.gram(n, dtype)
        C, ok = _inv_cov(ta, [K.indefinite_at(n, dtype, k), good])
        assert list(ok) == [0, 1] and not C[0].any(), (n, k)
        assert K.inv_cov_ratio(good, C[1]) <= 1.0
    # n = 1 with a negative entry: the reference's unprotected branch (math.h:49-50), C = 1 / H and no verdict
    H = np.array([[[-4.0]], [[0.25]]], dtype)
    C, ok = ta.inv_cov(torch.from_numpy(H).cuda())
    assert list(ok.cpu().numpy()) == [1, 1] and np.array_equal(C.cpu().numpy(), (1 / H).astype(dtype))
    print(f"covariance, {np.dtype(dtype).name}: worst column residual / bound = {worst:.3g}")


def _ref_dict(ref):
    return dict(errs=ref["errs"], succ=ref["succ"], iters=ref["iters"], stop=ref["stop"], x=ref["x"], cost=ref["cost"],
                fails=ref["fails"], deltas2=ref["deltas2"])


def _run_lm(ta, A, b, x0):
    model = ta.DenseRow.from_arrays(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda())
    x = torch.from_numpy(x0.copy()).cuda()
    out = ta.Optimize(x, model, ta.Options(), history=True)
    torch.cuda.synchronize()
    return out, x


@DT
@pytest.mark.parametrize("n,m,k", K.FUSED_SHAPES)
def test_fused_loop_takes_the_fall_back(ta, oracle, dtype, n, m, k):
    """DenseRow with column k of A zero: H has an exact zero row in every iteration, so every solve of the fused kernel leaves
    the fast path at pivot k, re-creates its image (lm_device.hpp) and runs the pivoted routine."""
    A, b, x0 = K.fused_problem(oracle, n, m, k, dtype)
    pod = ta.Options().to_pod()
    ref = oracle.dense_row_lm(A, b, x0, pod, history=True)
    out, x = _run_lm(ta, A, b, x0)
    xg = x.cpu().numpy()
    assert xg[:, k].tobytes() == x0[:, k].tobytes(), "the parameter without data must keep the caller's bits"
    stop = out.stop_reason.cpu().numpy()
    if dtype == np.float64:
        st = check_trajectories(gpu_dict(out, x), _ref_dict(ref), dtype, pod, label=f"{n}x{m} zero column {k}")
        assert st["full"] + st["ties"] == K.FUSED_P
        assert (stop >= 1).all() and (out.num_failures.cpu().numpy() == 0).all()
    else:
        # as test_tiny_and_empty_batches: the same verdict class, and the same final cost where the stop reasons agree.  fp32 costs of
        # two correct runs agree to parity.TOL's cost_rtol (sequential float sum against the matrix cores' blocked order)
        assert np.array_equal(stop >= 0, ref["stop"] >= 0), (stop, ref["stop"])
        good = (stop >= 0) & (stop == ref["stop"])
        if good.any():
            assert np.allclose(out.final_cost.cpu().numpy()[good], ref["cost"][good], rtol=TOL["f32"]["cost_rtol"], atol=1e-12)
    # only problems 1 and 3 carry the zero column: problems 0 and 2 are solved as in a batch without any, bit for bit
    A13 = K.fused_problem(oracle, n, m, k, dtype, cols=(1, 3))[0]
    A_none = K.fused_problem(oracle, n, m, k, dtype, cols=())[0]
    o13, x13 = _run_lm(ta, A13, b, x0)
    o0, xn = _run_lm(ta, A_none, b, x0)
    for p in (0, 2):
        assert x13[p].cpu().numpy().tobytes() == xn[p].cpu().numpy().tobytes(), (p, "x")
        for f in ("final_cost", "num_iters", "stop_reason", "num_failures"):
            assert getattr(o13, f)[p].cpu().numpy().tobytes() == getattr(o0, f)[p].cpu().numpy().tobytes(), (p, f)
    for p in (1, 3):
        assert x13[p, k].cpu().numpy().tobytes() == x0[p, k].tobytes()
        assert int(o13.stop_reason[p]) >= 0


@DT
def test_workgroup_ldlt_panel_edges(ta, oracle, dtype):
    """64 <= n <= 128 (ldlt_wg.hpp): full and partial last panels of five to eight; a negative pivot in the first, second, fifth and
    last panel.  zero_rows is REFUSED here (ok = 0, dx = 0) where Eigen's rule and the one-wavefront path accept it: the workgroup
    LDL^T has no pivoted fall-back — the difference ldlt_wg.hpp and the C header document, pinned so that it cannot change silently."""
    worst = [0.0]
    for n in K.WG_NS:
        acc, refused = K.wg_cases(n, dtype)
        for fam in range(2):
            cases = acc[fam * K.WG_P:(fam + 1) * K.WG_P]
            dx, ok = _solve(ta, cases)
            _, ok_ref = _oracle(oracle, cases)
            for c, d, o, r in zip(cases, dx, ok, ok_ref):
                _check(c, d, o, r, worst)
        dx, ok = _solve(ta, refused + acc[:1])      # (a definite matrix in the same launch is still solved)
        for c, d, o in zip(refused, dx, ok):
            _check(c, d, o, None, worst, want_ok=0)
        _check(acc[0], dx[-1], ok[-1], None, worst)
    print(f"workgroup LDL^T, {np.dtype(dtype).name}: worst eta / bound = {worst[0]:.3g}")
