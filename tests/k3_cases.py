"""Matrix families and the backward-error bound for the K3 solve (`toa_solve_damped`) and the covariance seam (`toa_inv_cov`).

Plain numpy, no GPU, everything seeded: tests/test_cpu_k3_cases.py shows that the CPU oracle satisfies every condition on every
case listed here, tests/test_gpu_k3.py then asks the same of the HIP kernels.  Both iterate the SAME lists (every_n_batches,
fall_back_cases, inv_cov_cases, wg_cases, FUSED_SHAPES), so no GPU case exists that the CPU test has not accepted.

The bound.  For LDL^T / Cholesky of a positive-definite matrix in ANY symmetric pivot order (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., Thms 10.3-10.4) the computed solution solves (A + dA) x = b with |dA| <= gamma_{3n+1} |L||D||L^T|,
and || |L||D||L^T| ||_2 <= n ||A||_2.  Hence the normwise backward error of a damped system Hd dx = -g,

    eta = ||Hd dx + g||_2 / (||Hd||_2 ||dx||_2 + ||g||_2),

is at most n gamma_k with gamma_k = k u / (1 - k u), u the unit round-off of the element type.  k = 3n + 8: the eight extra
roundings cover the multiplication by a < 1 ulp reciprocal in place of a division, D folded into the matrix-core operand and the
damped diagonal rounded once.  About 7e-4 at n = 63 in fp32 and 1.4e-12 in fp64; any structural error (a wrong refill, a wrong
permutation, a tile that misses a row) gives eta of order 1.

LDL^T is invariant under a two-sided scaling by powers of two, so for the families that carry one (`graded`, `huge`) eta is
evaluated on the exactly rescaled system — there the bound applies; the unscaled eta is dominated by the largest block.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace

import numpy as np

DTYPES = (np.float32, np.float64)


def unit_roundoff(dtype) -> float:
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def bound(n: int, dtype) -> float:
    """n * gamma_{3n+8} (module docstring)."""
    ku = (3 * n + 8) * unit_roundoff(dtype)
    return n * ku / (1.0 - ku)


def damped(H, scale, dtype=None):
    """H with its diagonal multiplied by `scale` in double and rounded to the element type (lm.h:108-117); float64 out."""
    dtype = np.dtype(dtype or H.dtype)
    Hd = np.array(H, np.float64)
    i = np.arange(Hd.shape[-1])
    Hd[..., i, i] = (Hd[..., i, i] * float(scale)).astype(dtype).astype(np.float64)
    return Hd


@dataclass
class Case:
    name: str
    H: np.ndarray               # [n, n], element type, exactly symmetric
    g: np.ndarray               # [n], element type
    ok: int                     # the verdict Eigen's rule gives (math.h:236)
    scale: float = 1.0          # damping factor handed to the solve
    zeros: tuple = ()           # rows / columns that are exactly zero: dx there is exactly 0, eta is that of the reduced system
    row_exp: np.ndarray = field(default=None)   # H = S H' S with S = diag(2^row_exp): eta is evaluated on H'
    h_exp: int = 0              # H (and S H' S) carries a further factor 2^h_exp
    g_exp: int = 0              # g carries a factor 2^g_exp beyond S

    @property
    def n(self):
        return self.H.shape[0]

    @property
    def dtype(self):
        return self.H.dtype

    @property
    def keep(self):
        return np.array([i for i in range(self.n) if i not in self.zeros], int)

    def with_scale(self, scale):
        return replace(self, scale=float(scale))

    def rescaled(self):
        """(Hd', g', e): the reduced damped system after the exact power-of-two rescaling, float64; dx' = dx * 2^(e + h_exp - g_exp)."""
        kp = self.keep
        e = (self.row_exp if self.row_exp is not None else np.zeros(self.n, int))[kp]
        Hd = damped(self.H, self.scale)[np.ix_(kp, kp)]
        Hs = np.ldexp(Hd, -(e[:, None] + e[None, :]) - self.h_exp)
        gs = np.ldexp(np.asarray(self.g, np.float64)[kp], -e - self.g_exp)
        return Hs, gs, e


def eta(case: Case, dx) -> float:
    """Normwise backward error of dx for the case's (reduced, rescaled) damped system, in float64."""
    Hs, gs, e = case.rescaled()
    xs = np.ldexp(np.asarray(dx, np.float64)[case.keep], e + case.h_exp - case.g_exp)
    r = Hs @ xs + gs
    return float(np.linalg.norm(r) / (np.linalg.norm(Hs, 2) * np.linalg.norm(xs) + np.linalg.norm(gs)))


def eta_bound(case: Case) -> float:
    return bound(len(case.keep), case.dtype)


def inv_cov_ratio(case: Case, C) -> float:
    """max over the columns j of ||H C[:, j] - e_j||_2 / (bound (||H||_2 ||C[:, j]||_2 + 1)) on the reduced, rescaled system
    (case.scale must be 1: the covariance seam does not damp)."""
    assert case.scale == 1.0
    Hs, _, e = case.rescaled()
    kp = case.keep
    Cs = np.ldexp(np.asarray(C, np.float64)[np.ix_(kp, kp)], e[:, None] + e[None, :] + case.h_exp)
    R = Hs @ Cs - np.eye(len(kp))
    hn = np.linalg.norm(Hs, 2)
    return float((np.linalg.norm(R, axis=0) / (eta_bound(case) * (hn * np.linalg.norm(Cs, axis=0) + 1.0))).max())


def unpivoted_pivots(Hd):
    """The pivots of an unpivoted elimination of Hd (float64), up to and including the first that is not positive."""
    S = np.array(Hd, np.float64)
    out = []
    for k in range(S.shape[0]):
        d = S[k, k]
        out.append(d)
        if not d > 0:
            break
        S[k + 1:, k + 1:] -= np.outer(S[k + 1:, k] / d, S[k, k + 1:])
    return np.array(out)


def fast_path_gate(d, dtype) -> bool:
    """pivot_in_range of ldlt_regs.hpp: positive, above the smallest normal number, below 2^125 (fp32) / 2^1021 (fp64)."""
    f32 = np.dtype(dtype) == np.float32
    lo, hi = (2.0 ** -126, 2.0 ** 125) if f32 else (2.0 ** -1022, 2.0 ** 1021)
    return bool(lo < d < hi)


# ---- the families: functions of (n, dtype, seed) --------------------------------------------------------------------------------
def _rng(tag, n, seed):
    return np.random.default_rng([tag, n, seed])


def _gram64(rng, n):
    J = rng.uniform(-1, 1, (3 * n + 2, n))
    H = J.T @ J
    return np.triu(H) + np.triu(H, 1).T     # exactly symmetric


def _rhs(rng, n):
    return rng.uniform(-1, 1, n)


def gram(n, dtype, seed=0) -> Case:
    """(a) J^T J with J uniform in [-1, 1], (3n + 2) x n."""
    rng = _rng(1, n, seed)
    return Case(f"gram[{seed}]", _gram64(rng, n).astype(dtype), _rhs(rng, n).astype(dtype), 1)


GRADED_MAX_EXP = {np.dtype(np.float32): 10, np.dtype(np.float64): 20}


def graded(n, dtype, seed=0) -> Case:
    """(b) S (gram) S, S = diag(2^e) with the integer exponents spread over 0 .. 10 (fp32) / 0 .. 20 (fp64) in shuffled order:
    condition number about 1e6 / 1e12, and the unpivoted order is not the favourable one.  g = S g0, so that the rescaled system
    is the balanced one."""
    rng = _rng(2, n, seed)
    H0 = _gram64(rng, n).astype(dtype)
    g0 = _rhs(rng, n).astype(dtype)
    e = np.rint(np.linspace(0, GRADED_MAX_EXP[np.dtype(dtype)], n)).astype(int)
    rng.shuffle(e)
    H = np.ldexp(H0, e[:, None] + e[None, :]).astype(dtype)     # exact
    return Case(f"graded[{seed}]", H, np.ldexp(g0, e).astype(dtype), 1, row_exp=e)


def indefinite_at(n, dtype, k, seed=0) -> Case:
    """(c) gram with entry (k, k) lowered by twice its Schur complement against the leading k x k block: the first k pivots of an
    unpivoted elimination are positive, pivot k is negative.  Expected: ok = 0, dx = 0 exactly."""
    rng = _rng(3, n, seed)
    H = _gram64(rng, n)
    g = _rhs(rng, n)
    s = H[k, k] - (H[k, :k] @ np.linalg.solve(H[:k, :k], H[:k, k]) if k else 0.0)
    H[k, k] -= 2.0 * s
    return Case(f"indefinite_at({k})", H.astype(dtype), g.astype(dtype), 0)


def zero_rows(n, dtype, ks, seed=0) -> Case:
    """(d) gram with row and column k set to zero for every k in ks: singular, positive semi-definite with EXACT zero pivots.
    Eigen's rule accepts it; dx[k] = 0 exactly (also where g[k] != 0), the rest solves the reduced system."""
    rng = _rng(4, n, seed)
    H = _gram64(rng, n)
    g = _rhs(rng, n)
    ks = tuple(sorted(set(int(k) for k in ks)))
    for k in ks:
        H[k, :] = 0.0
        H[:, k] = 0.0
    label = ",".join(map(str, ks)) if len(ks) <= 3 else f"{ks[0]},{ks[1]},..,{ks[-1]}"
    return Case(f"zero_rows([{label}])", H.astype(dtype), g.astype(dtype), 1, zeros=ks)


HUGE_EXP = {np.dtype(np.float32): (125, 100), np.dtype(np.float64): (1021, 900)}


def huge(n, dtype, seed=0) -> Case:
    """(e) gram scaled by an exact power of two so that every diagonal entry is >= 2^125 (fp32) / 2^1021 (fp64) and the largest is
    below 2^127 / 2^1023; g scaled by 2^100 / 2^900.  Every pivot is above the upper gate of the fast path, which refuses at
    pivot 0; the pivoted routine must solve a perfectly conditioned system."""
    rng = _rng(5, n, seed)
    H0 = _gram64(rng, n).astype(dtype)
    g0 = _rhs(rng, n).astype(dtype)
    top, ge = HUGE_EXP[np.dtype(dtype)]
    a = top - int(np.floor(np.log2(float(np.diag(H0).min()))))
    H = np.ldexp(H0, a).astype(dtype)
    d = np.diag(H).astype(np.float64)
    assert np.isfinite(H).all() and d.min() >= 2.0 ** top and d.max() < 2.0 ** (top + 2), (n, dtype, seed)
    return Case(f"huge[{seed}]", H, np.ldexp(g0, ge).astype(dtype), 1, h_exp=a, g_exp=ge)


def verdict_cases(n, dtype, seed=0):
    """(f) the hand-made verdict matrices of test_solve_damped_acceptance_rule grown to size n (n >= 3)."""
    rng = _rng(6, n, seed)
    G = _gram64(rng, n)
    g = _rhs(rng, n).astype(dtype)
    pair = np.zeros((n, n))
    pair[n // 3, n - 1] = pair[n - 1, n // 3] = 1.0
    dneg = rng.uniform(0.5, 2.0, n)
    dneg[n // 2] = -dneg[n // 2]
    return [Case("all_zero", np.zeros((n, n), dtype), g, 1, zeros=tuple(range(n))),
            Case("zero_diagonal_pair", pair.astype(dtype), g, 0),
            Case("negative_definite", (-G).astype(dtype), g, 0),
            Case("diagonal_one_negative", np.diag(dneg).astype(dtype), g, 0)]


def stack(cases):
    return np.stack([c.H for c in cases]), np.stack([c.g for c in cases])


# ---- the case lists the CPU and the GPU test share ------------------------------------------------------------------------------
EVERY_N = tuple(range(1, 64))
EVERY_N_SCALES = (1.0, 1.0001, 3.0)
EVERY_N_P = 8


def every_n_batches(n, dtype):
    """[(label, scale, [P cases])] of test_every_n at one n: gram at three damping factors, graded at one."""
    out = [(f"gram x{s}", s, [gram(n, dtype, seed).with_scale(s) for seed in range(EVERY_N_P)]) for s in EVERY_N_SCALES]
    out.append(("graded x1.0001", 1.0001, [graded(n, dtype, seed).with_scale(1.0001) for seed in range(EVERY_N_P)]))
    return out


# the register form, and one, two, three and four 16-column panels with full and partial last panels
PANEL_NS = (3, 12, 16, 17, 20, 31, 32, 33, 40, 47, 48, 49, 50, 63)
FALL_BACK_SCALE = 1.0001


def panel_ks(n):
    return sorted(k for k in {0, 1, 15, 16, 17, 31, 32, 47, 48, n - 1} if 0 <= k < n)


def fall_back_cases(n, dtype):
    """Every matrix of test_fall_back_at_every_panel at one n (all at the same damping factor: one launch can mix them)."""
    cs = [indefinite_at(n, dtype, k) for k in panel_ks(n)]
    cs += [zero_rows(n, dtype, [k]) for k in panel_ks(n)]
    cs += [zero_rows(n, dtype, [0, n - 1]), zero_rows(n, dtype, range(0, n, 2)), huge(n, dtype)]
    cs += verdict_cases(n, dtype)
    return [c.with_scale(FALL_BACK_SCALE) for c in cs]


def mixed_batch(n, dtype):
    """fall_back_cases(n) with a gram matrix after every one of them: the order of the launch that mixes fates."""
    out = []
    for i, c in enumerate(fall_back_cases(n, dtype)):
        out += [c, gram(n, dtype, 100 + i).with_scale(FALL_BACK_SCALE)]
    return out


INV_COV_NS = (1, 2, 7, 16, 17, 32, 33, 48, 49, 63)
INV_COV_P = 3


def inv_cov_cases(n, dtype):
    """Every matrix of test_inv_cov_families at one n (the covariance seam does not damp: scale 1)."""
    cs = [gram(n, dtype, seed) for seed in range(INV_COV_P)] + [graded(n, dtype, seed) for seed in range(INV_COV_P)]
    if n >= 2:
        cs += [zero_rows(n, dtype, [k]) for k in sorted({0, n // 2, n - 1})]
    cs.append(huge(n, dtype))
    return cs


INV_COV_INDEFINITE = tuple((n, k) for n in (20, 40, 63) for k in (0, 16, n - 1))

WG_NS = (64, 65, 79, 80, 81, 96, 111, 112, 113, 127, 128)
WG_P = 3
WG_SCALE = 1.0001


def wg_ks(n):
    return sorted(k for k in {0, 15, 16, 63, 64, n - 1} if k < n)


def wg_cases(n, dtype):
    """(accepted, refused) of test_workgroup_ldlt_panel_edges at one n.  `refused` holds the indefinite matrices AND the
    zero_rows ones: the workgroup LDL^T has no pivoted fall-back, it refuses a singular semi-definite matrix where Eigen's rule
    (and Case.ok) accepts it — the documented difference (ldlt_wg.hpp, include/tinyopt_amd.h)."""
    acc = [f(n, dtype, seed).with_scale(WG_SCALE) for f in (gram, graded) for seed in range(WG_P)]
    ref = [indefinite_at(n, dtype, k).with_scale(WG_SCALE) for k in wg_ks(n)]
    ref += [zero_rows(n, dtype, [k]).with_scale(WG_SCALE) for k in wg_ks(n)]
    return acc, ref


# (n, m, k): DenseRow problems whose column k of A is zero, so that H has an exact zero row in every iteration of the fused loop
FUSED_SHAPES = ((12, 40, 5), (20, 60, 0), (20, 60, 16), (50, 150, 17), (50, 150, 49))
FUSED_P = 4


def fused_problem(oracle, n, m, k, dtype, cols=None):
    """(A, b, x0) of oracle.synth_dense_row(4, n, m, dtype, seed = 10 n + k) with column k of A zeroed — in every problem, or in
    the problems listed in `cols` only."""
    A, b, x0, _ = oracle.synth_dense_row(FUSED_P, n, m, dtype, seed=10 * n + k)
    A = A.copy()
    for p in (range(FUSED_P) if cols is None else cols):
        A[p, :, k] = 0
    return A, b, x0
