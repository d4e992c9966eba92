"""The yardstick of tests/test_gpu_k3.py checked on its own: on every matrix that file hands to the HIP kernels the CPU oracle
gives the expected verdict, meets the derived backward-error bound n * gamma_{3n+8} (tests/k3_cases.py) where it accepts,
returns dx == 0 where it rejects and dx[k] == 0 on a zero row — and numpy confirms that the inputs have the structure their
family promises (sign of the spectrum, which unpivoted pivot leaves the fast path).  A GPU failure then cannot be the inputs'
fault.  There is no list of cases left out: the families are constructed, not sampled, so every cell must pass.

The oracle's worst eta / bound over everything below: 0.03 in fp32 and 0.06 in fp64 (each test prints its own).  `huge` stays
finite in the oracle in fp64 as in fp32, also as a covariance, whose off-diagonal entries are subnormal numbers."""
import numpy as np
import pytest

import k3_cases as K

DT = pytest.mark.parametrize("dtype", K.DTYPES, ids=["f32", "f64"])


def _solve(oracle, cases):
    """oracle.solve_damped over a list of cases that share n and dtype (one call per damping factor)."""
    dx = [None] * len(cases)
    ok = [None] * len(cases)
    for s in sorted({c.scale for c in cases}):
        idx = [i for i, c in enumerate(cases) if c.scale == s]
        H, g = K.stack([cases[i] for i in idx])
        d, o = oracle.solve_damped(H, g, s)
        for j, i in enumerate(idx):
            dx[i], ok[i] = d[j], int(o[j])
    return dx, ok


def _check_solution(c, dx, ok, worst):
    """The oracle's answer on one case: verdict, exact zeros, eta <= bound."""
    assert ok == c.ok, (c.name, c.n, ok)
    assert np.isfinite(dx).all(), (c.name, c.n)
    if not c.ok:
        assert not dx.any(), (c.name, c.n)
        return
    assert not dx[list(c.zeros)].any(), (c.name, c.n)
    if len(c.keep):
        r = K.eta(c, dx) / K.eta_bound(c)
        worst[0] = max(worst[0], r)
        assert r <= 1.0, (c.name, c.n, r)


def _check_structure(c):
    """numpy's view of one input: the spectrum's sign structure and the pivot at which an unpivoted elimination stops."""
    n = c.n
    assert np.array_equal(c.H, c.H.T) and np.isfinite(c.H).all() and np.isfinite(c.g).all()
    Hs, _, _ = c.rescaled()                       # damped, reduced to the non-zero rows, rescaled: float64
    piv = K.unpivoted_pivots(K.damped(c.H, c.scale))
    fam = c.name.split("[")[0].split("(")[0]
    if fam in ("gram", "graded"):
        assert np.linalg.eigvalsh(Hs).min() > 0
        assert len(piv) == n and all(K.fast_path_gate(d, c.dtype) for d in piv), (c.name, n)     # the fast path runs to the end
    elif fam == "indefinite_at":
        k = int(c.name[len("indefinite_at("):-1])
        assert np.linalg.eigvalsh(Hs).min() < -1.0, (c.name, n)
        assert len(piv) == k + 1 and (piv[:k] > 0).all() and piv[k] < 0, (c.name, n, piv)
        assert all(K.fast_path_gate(d, c.dtype) for d in piv[:k])
    elif fam == "zero_rows":
        k0 = c.zeros[0]
        for k in c.zeros:
            assert not c.H[k].any() and not c.H[:, k].any()
        assert np.linalg.eigvalsh(Hs).min() > 0                                                   # the reduced system is definite
        assert len(piv) == k0 + 1 and (piv[:k0] > 0).all() and piv[k0] == 0, (c.name, n, piv)     # an EXACT zero pivot at step k0
    elif fam == "huge":
        assert np.linalg.eigvalsh(Hs).min() > 0 and np.linalg.cond(Hs) < 1e3
        assert not K.fast_path_gate(float(c.H[0, 0]) * 1.0, c.dtype)                              # refused at pivot 0
        lo = 125 if c.dtype == np.float32 else 1021
        d = np.diag(K.damped(c.H, c.scale))
        assert np.isfinite(d).all() and d.min() >= 2.0 ** lo and d.max() < 2.0 ** (lo + 2)
    else:
        assert fam in ("all_zero", "zero_diagonal_pair", "negative_definite", "diagonal_one_negative"), fam
        ev = np.linalg.eigvalsh(K.damped(c.H, c.scale))
        if fam == "all_zero":
            assert not c.H.any()
        elif fam == "negative_definite":
            assert ev.max() < 0
        else:
            assert ev.min() < -0.4 and ev.max() > 0.4                                             # indefinite, with a margin
        assert not K.fast_path_gate(piv[-1], c.dtype)


@DT
def test_every_n_cases(oracle, dtype):
    worst = [0.0]
    for n in K.EVERY_N:
        for label, scale, cases in K.every_n_batches(n, dtype):
            assert len(cases) == K.EVERY_N_P and all(c.scale == scale and c.n == n and c.dtype == dtype for c in cases)
            dx, ok = _solve(oracle, cases)
            for c, d, o in zip(cases, dx, ok):
                _check_structure(c)
                _check_solution(c, d, o, worst)
    print(f"oracle, every n, {np.dtype(dtype).name}: worst eta / bound = {worst[0]:.3g}")


@DT
def test_fall_back_cases(oracle, dtype):
    worst = [0.0]
    for n in K.PANEL_NS:
        cases = K.mixed_batch(n, dtype)
        names = [c.name for c in cases[0::2]]
        for want in ["huge[0]", "all_zero", "zero_diagonal_pair", "negative_definite", "diagonal_one_negative", f"zero_rows([0,{n - 1}])"] + \
                [f"indefinite_at({k})" for k in K.panel_ks(n)] + [f"zero_rows([{k}])" for k in K.panel_ks(n)]:
            assert want in names, (n, want)
        dx, ok = _solve(oracle, cases)
        for c, d, o in zip(cases, dx, ok):
            _check_structure(c)
            _check_solution(c, d, o, worst)
    print(f"oracle, fall-back cases, {np.dtype(dtype).name}: worst eta / bound = {worst[0]:.3g}")


def _oracle_inv_cov(oracle, c):
    """C = H^-1 column by column through the oracle's solve (H C[:, j] = e_j), as InvCov's `chol.solve(Identity)` does."""
    n = c.n
    H = np.broadcast_to(c.H, (n, n, n)).copy()
    C, ok = oracle.solve_damped(H, -np.eye(n, dtype=c.dtype), 1.0)
    return C.T, ok


@DT
def test_inv_cov_cases(oracle, dtype):
    worst = 0.0
    for n in K.INV_COV_NS:
        for c in K.inv_cov_cases(n, dtype):
            _check_structure(c)
            C, ok = _oracle_inv_cov(oracle, c)
            assert ok.all() and np.isfinite(C).all(), (c.name, n)
            z = list(c.zeros)
            assert not C[z].any() and not C[:, z].any(), (c.name, n)
            r = K.inv_cov_ratio(c, C)
            worst = max(worst, r)
            assert r <= 1.0, (c.name, n, r)
    for n, k in K.INV_COV_INDEFINITE:
        c = K.indefinite_at(n, dtype, k)
        _check_structure(c)
        C, ok = _oracle_inv_cov(oracle, c)
        assert not ok.any() and not C.any(), (n, k)
    print(f"oracle, covariance cases, {np.dtype(dtype).name}: worst column residual / bound = {worst:.3g}")


@DT
def test_workgroup_cases(oracle, dtype):
    """64 <= n <= 128.  The oracle ACCEPTS the zero_rows matrices (Eigen's rule); the workgroup LDL^T refuses them, which
    test_workgroup_ldlt_panel_edges pins — here they only have to be what they claim to be."""
    worst = [0.0]
    for n in K.WG_NS:
        acc, ref = K.wg_cases(n, dtype)
        assert len(acc) == 2 * K.WG_P and len(ref) == 2 * len(K.wg_ks(n))
        dx, ok = _solve(oracle, acc + ref)
        for c, d, o in zip(acc + ref, dx, ok):
            _check_structure(c)
            _check_solution(c, d, o, worst)
    print(f"oracle, workgroup cases, {np.dtype(dtype).name}: worst eta / bound = {worst[0]:.3g}")


@DT
def test_fused_loop_problems(oracle, dtype):
    """The DenseRow problems with a zero column: the oracle converges without a rejected solve and never moves x[:, k]."""
    from tinyopt_amd.api import Options
    for n, m, k in K.FUSED_SHAPES:
        A, b, x0 = K.fused_problem(oracle, n, m, k, dtype)
        assert not A[:, :, k].any()
        ref = oracle.dense_row_lm(A, b, x0, Options().to_pod(), history=True)
        assert (ref["stop"] >= 0).all(), (n, m, k, ref["stop"])
        if dtype == np.float64:   # (fp32 runs end in rejected steps on the round-off floor of the cost: only the verdict class is compared there)
            assert (ref["stop"] >= 1).all() and (ref["fails"] == 0).all(), (n, m, k, ref["stop"], ref["fails"])
            assert (ref["iters"] <= 8).all(), ref["iters"]
        assert np.array_equal(ref["x"][:, k], x0[:, k])
        some = K.fused_problem(oracle, n, m, k, dtype, cols=(1, 3))[0]
        assert not some[1, :, k].any() and not some[3, :, k].any() and some[0, :, k].any() and some[2, :, k].any()
