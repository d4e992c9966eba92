"""A numpy restatement of the batched L-BFGS state machine of DESIGN section 19 (tinyopt_amd/csrc/lbfgs_device.hpp), written from
that definition and not from the device code: limited-memory BFGS (Nocedal & Wright, algorithm 7.4) with a backtracking Armijo
search, the reference's stop tests (optimizer.h:519-534) on the normalised cost.  Vector arithmetic and dot products in the
problem's dtype; the Armijo comparison, the normalised costs and the relative decrease in double.

`lbfgs_optimize(x0, f, pod, dtype, history, c1, shrink)` runs a batch: f(p, x) -> (cost, grad) of problem p at x, both in `dtype`;
pod is the toa_options POD (tinyopt_amd._capi.ToaOptions).  Returns the dict tests/parity.py::gpu_dict returns (plus consec / rerr and
`accepted_x`: every accepted point of the problem, for the tests of the restatement itself).
"""
from __future__ import annotations

import numpy as np

from gd_reference import (DBL_MAX, STOP_MAX_CONSEC_NO_DECR, STOP_MAX_ITERS, STOP_MAX_NO_DECR, STOP_MIN_DELTA_NORM, STOP_MIN_ERROR,  # noqa: F401
                          STOP_MIN_GRAD_NORM, STOP_MIN_REL_ERROR, STOP_NAN_OR_INF, STOP_NONE, float_epsilon, normalize_cost)

STOP_SKIPPED = -1


def check_lbfgs_options(history, c1, shrink, grad_clipping=0.0):
    """The ranges every layer refuses outside of (toa_jit_lbfgs_run, Optimize, the C++ adaptor)."""
    if not 1 <= int(history) <= 16:
        raise ValueError("L-BFGS: history must be in 1 .. 16")
    if not 0.0 < c1 < 1.0:
        raise ValueError("L-BFGS: c1 (the Armijo constant) must be in (0, 1)")
    if not 0.0 < shrink < 1.0:
        raise ValueError("L-BFGS: shrink (the backtracking factor) must be in (0, 1)")
    if grad_clipping != 0:
        raise ValueError("L-BFGS: grad_clipping must be 0")


def _dot(a, b, T):
    return T(np.sum(a * b, dtype=T))


def two_loop(g, pairs, gamma, T):
    """H g over the pairs [(s, y, rho)], oldest first, with H0 = gamma I."""
    q = g.copy()
    a = [None] * len(pairs)
    for i in range(len(pairs) - 1, -1, -1):
        s, y, rho = pairs[i]
        a[i] = T(rho * _dot(s, q, T))
        q = q - a[i] * y
    r = T(gamma) * q
    for i in range(len(pairs)):
        s, y, rho = pairs[i]
        b = T(rho * _dot(y, r, T))
        r = r + s * T(a[i] - b)
    return r


def lbfgs_solve_one(x0, f, pod, T, hs, history=8, c1=1e-4, shrink=0.5, ring_limit=True):
    """One problem.  ring_limit=False lifts the 1 .. 16 range of `history` (the restatement's own tests compare 16 with 63)."""
    T = np.dtype(T).type
    if ring_limit:
        check_lbfgs_options(history, c1, shrink, pod.grad_clipping)
    c1d, shr = float(np.float32(c1)), T(np.float32(shrink))
    tmax = float(np.finfo(T).max)
    mcf, mtf = int(pod.max_consec_failures), int(pod.max_total_failures)
    x_acc = np.asarray(x0, T).copy()
    trial = x_acc.copy()
    first, pairs, gamma = True, [], T(1)
    st = dict(final_cost=DBL_MAX, final_rerr=DBL_MAX, stop=STOP_NONE, iters=0, fails=0, consec=0, passes=0)
    errs, d2s, succ = np.zeros(hs), np.zeros(hs), np.zeros(hs, np.uint8)
    margins = np.full(hs, np.inf)   # per iteration: how far, in units of the cost, its closest cost decision was from flipping

    def margin(v):
        if st["iters"] - 1 < hs and np.isfinite(v):
            margins[st["iters"] - 1] = min(margins[st["iters"] - 1], abs(float(v)))
    f_acc = g_acc = d = None
    alpha, gd = T(1), T(0)
    accepted_x = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for _ in range(pod.max_iters + 1):
            c, g = f(trial)
            c, g = T(c), np.asarray(g, T).copy()
            st["passes"] += 1
            if not (np.isfinite(c) and np.isfinite(g).all()):
                st["stop"] = STOP_NAN_OR_INF
                break
            accepted = first or float(c) <= float(f_acc) + c1d * float(alpha) * float(gd)
            err = normalize_cost(float(c), pod)
            s = trial - x_acc
            if st["iters"] < hs:
                errs[st["iters"]], d2s[st["iters"]], succ[st["iters"]] = err, (0.0 if first else float(_dot(s, s, T))), 1 if accepted else 0
            st["iters"] += 1
            if not first:
                margin(float(c) - (float(f_acc) + c1d * float(alpha) * float(gd)))
            if accepted:
                if not first:
                    y = g - g_acc
                    sy = _dot(s, y, T)
                    rho = T(1) / sy
                    if sy > 0 and np.isfinite(rho):
                        pairs.append((s, y, rho))
                        if len(pairs) > history:
                            pairs.pop(0)
                        gamma = T(sy / _dot(y, y, T))
                prev = st["final_cost"]
                rel = (prev - err) / prev if (prev > float_epsilon(T) and prev < tmax) else 0.0
                x_acc, f_acc, g_acc = trial.copy(), c, g
                if pod.min_error > 0:
                    margin(err - pod.min_error)
                if not first and pod.min_rerr_dec > 0 and prev < tmax:
                    margin(prev - err)                              # rel > 0
                    margin((rel - pod.min_rerr_dec) * prev)         # rel < min_rerr_dec
                accepted_x.append(x_acc.copy())
                st["consec"], st["final_cost"], st["final_rerr"] = 0, err, rel
                if pod.min_error > 0 and err < pod.min_error:
                    st["stop"] = STOP_MIN_ERROR
                elif not first and pod.min_rerr_dec > 0 and 0.0 < rel < pod.min_rerr_dec:
                    st["stop"] = STOP_MIN_REL_ERROR
                elif pod.min_grad_norm2 > 0 and float(_dot(g, g, T)) < pod.min_grad_norm2:
                    st["stop"] = STOP_MIN_GRAD_NORM
                if st["stop"] != STOP_NONE:
                    break
                first = False
                d, gd = None, T(0)
                if pairs:
                    d = -two_loop(g_acc, pairs, gamma, T)
                    gd = _dot(g_acc, d, T)
                if not pairs or not (gd < 0) or not np.isfinite(gd):
                    pairs = []
                    d = -g_acc / max(T(1), T(np.sqrt(_dot(g_acc, g_acc, T))))
                    gd = _dot(g_acc, d, T)
                alpha = T(1)
            else:
                st["consec"] += 1
                st["fails"] += 1
                margin(abs(float(c) - float(f_acc)) - pod.min_rerr_dec * abs(float(f_acc)))
                if abs(float(c) - float(f_acc)) < pod.min_rerr_dec * abs(float(f_acc)):   # the round-off floor
                    st["stop"] = STOP_MIN_REL_ERROR
                    break
                if mcf > 0 and st["consec"] >= mcf:
                    st["stop"] = STOP_MAX_CONSEC_NO_DECR
                    break
                if mtf > 0 and st["fails"] >= mtf:
                    st["stop"] = STOP_MAX_NO_DECR
                    break
                alpha = T(alpha * shr)
            step = alpha * d
            if float(_dot(step, step, T)) < pod.min_step_norm2:
                st["stop"] = STOP_MIN_DELTA_NORM
                break
            trial = x_acc + step
    if st["stop"] == STOP_NONE:
        st["stop"] = STOP_MAX_ITERS
    st["margins"] = margins
    return x_acc, st, errs, d2s, succ, accepted_x


def lbfgs_optimize(x0, f, pod, dtype, history=8, c1=1e-4, shrink=0.5, ring_limit=True):
    """x0: [P, n]; f(p, x) -> (cost, grad) of problem p.  Returns errs / succ / deltas2 [P, max_iters + 2], iters, stop, x, cost, fails,
    consec, rerr, passes and accepted_x (a list of [k, n] arrays)."""
    T = np.dtype(dtype).type
    P, n = np.asarray(x0).shape
    hs = pod.max_iters + 2
    out = dict(errs=np.zeros((P, hs)), succ=np.zeros((P, hs), np.uint8), deltas2=np.zeros((P, hs)), iters=np.zeros(P, np.int64),
               stop=np.zeros(P, np.int64), x=np.zeros((P, n), T), cost=np.zeros(P), fails=np.zeros(P, np.int64),
               consec=np.zeros(P, np.int64), rerr=np.zeros(P), passes=np.zeros(P, np.int64), accepted_x=[], margins=np.full((P, hs), np.inf))
    for p in range(P):
        x, st, errs, d2s, succ, acc = lbfgs_solve_one(x0[p], lambda xx, p=p: f(p, xx), pod, T, hs, history, c1, shrink, ring_limit)
        out["x"][p] = x
        out["errs"][p], out["deltas2"][p], out["succ"][p] = errs, d2s, succ
        out["iters"][p], out["stop"][p], out["fails"][p], out["consec"][p] = st["iters"], st["stop"], st["fails"], st["consec"]
        out["cost"][p], out["rerr"][p], out["passes"][p] = st["final_cost"], st["final_rerr"], st["passes"]
        out["accepted_x"].append(np.array(acc, T).reshape(-1, n))
        out["margins"][p] = st["margins"]
    return out


# ---- the comparison of a run with the restatement ------------------------------------------------------------------------
# A cost at the same iteration may differ by K_COST x the round-off bound of ONE evaluation of the cost: the trial point carries the
# round-off of every pass before it, at most max_iters + 1 = 41 in the tests, each moving the next cost by about one bound where the
# problem is well conditioned — 64 covers that linear accumulation.  What grows faster is amplification, and the problem counts as
# ill-determined (ill_determined, found at K_ILL: a quarter of K_COST, because the twins that find it are a sample).
K_COST, K_ILL = 64.0, 16.0
X_TOL = {np.float64: 1e-8, np.float32: 2e-3}   # the final x, relative to max(1, |x|): tests/parity.py's


def perturbed(f, rel, seed=1):
    """f with every cost and every gradient component multiplied by 1 + rel u, u uniform in [-1, 1]: another rounding of the same
    function (rel: a few units in the last place, what another order of evaluation does)."""
    rng = np.random.default_rng(seed)

    def fp(p, x):
        c, g = f(p, x)
        g = np.asarray(g)
        T = g.dtype.type
        return T(c * T(1 + rel * rng.uniform(-1, 1))), (g * (1 + rel * rng.uniform(-1, 1, g.shape))).astype(T)
    return fp


def logistic_fast(A, yl, x, T):
    """gd_reference.logistic with z as one matrix product: another rounding of the same function, for the twins of ill_determined."""
    T = np.dtype(T).type
    A, yl = np.asarray(A, T), np.asarray(yl, T)
    with np.errstate(over="ignore"):
        e = np.exp(-yl * (A @ np.asarray(x, T)))
    return T(np.sum(np.log(T(1) + e), dtype=T)), ((-yl * e / (T(1) + e)) @ A).astype(T)


def _departs(got, ref, p, dtype, noise, k_cost=K_COST):
    """The first iteration at which run `got` of problem p leaves `ref` — (i, "flag" | "cost" | "stop") — or None: another accept /
    reject flag, a cost beyond K_COST x the round-off bound, another length or stop reason after the last common iteration."""
    gk, rk = int(got["iters"][p]), int(ref["iters"][p])
    for i in range(min(gk, rk)):
        if bool(got["succ"][p][i]) != bool(ref["succ"][p][i]):
            return i, "flag"
        if abs(got["errs"][p][i] - ref["errs"][p][i]) > k_cost * noise(p, ref["errs"][p][i]):
            return i, "cost"
    if gk != rk or got["stop"][p] != ref["stop"][p]:
        return min(gk, rk) - 1, "stop"
    xg, xr = np.asarray(got["x"][p], np.float64), np.asarray(ref["x"][p], np.float64)
    if np.abs(xg - xr).max() > (k_cost / K_COST) * X_TOL[np.dtype(dtype).type] * max(1.0, np.abs(xr).max()):   # (twins: a quarter)
        return rk - 1, "x"
    return None


def ill_determined(ref, twins, dtype, noise):
    """The problems whose trajectory the restatement itself does not determine to K_ILL x the round-off bound: a twin — the
    restatement over another rounding of the same costs and gradients (perturbed, a few units in the last place) — leaves `ref` in a
    cost or in x without a decision having flipped.  L-BFGS amplifies last places where the minimiser lies at infinity (separable
    data: fewer items than parameters) — y = g - g_acc cancels.  Returns a bool array [P]."""
    P = len(ref["iters"])
    ill = np.zeros(P, bool)
    for tw in twins:
        for p in range(P):
            d = _departs(tw, ref, p, dtype, noise, K_ILL)
            if d is not None and d[1] in ("cost", "x"):
                ill[p] = True
    return ill


def compare_trajectories(got, ref, dtype, noise, label="", ill=None):
    """got: the dict of parity.gpu_dict; ref: lbfgs_optimize's; noise(p, cost): the round-off bound of problem p's cost at a point
    where it is `cost`, in units of the cost; ill: ill_determined's array.  Per problem, iteration by iteration: the same accept /
    reject flag and the same cost to K_COST x noise; then the same StopReason, iteration and failure counts, the final x to X_TOL and
    the final cost to K_COST x noise ("full").  A problem may leave the restatement in two ways only, both counted in "parted":
      * at a decision — another flag at iteration j, or another ending after iteration j — that the restatement took within the
        round-off: its closest cost decision of that iteration (Armijo, min_error, min_rerr_dec, the round-off floor) was within
        2 x noise of flipping (two costs enter each decision, the trial's and the accepted one's, each with its own round-off);
      * as a problem the restatement itself does not determine (`ill`): its flags are still compared as far as both runs go, and
        nothing else is asked of it but the final-cost rule below — which is why it COUNTS as parted whatever the run did.
    Both runs hold accepted points of a descent, so a parted problem's final cost must not exceed the last cost both accepted by
    more than K_COST x noise.  Anything else raises.  Returns {"full", "parted", "ill", "parted_at", "max_cost_dev"}: max_cost_dev is
    the largest |cost - ref| / noise over the compared iterations of the full problems (<= K_COST)."""
    P = len(ref["iters"])
    full, parted, at, dev = 0, 0, [], 0.0
    n_ill = 0
    for p in range(P):
        if ref["stop"][p] == STOP_SKIPPED or got["stop"][p] == STOP_SKIPPED:
            assert got["stop"][p] == ref["stop"][p], (label, p, "skipped")
            full += 1
            continue
        re_, rs, gs = ref["errs"][p], ref["succ"][p], got["succ"][p]
        d = _departs(got, ref, p, dtype, noise)
        is_ill = ill is not None and bool(ill[p])
        if d is None and not is_ill:
            full += 1
            assert got["fails"][p] == ref["fails"][p], (label, p, "fails", got["fails"][p], ref["fails"][p])
            assert abs(got["cost"][p] - ref["cost"][p]) <= K_COST * noise(p, ref["cost"][p]), (label, p, "cost", got["cost"][p], ref["cost"][p])
            k = int(ref["iters"][p])
            dev = max(dev, max(abs(got["errs"][p][i] - re_[i]) / noise(p, re_[i]) for i in range(k)))
            continue
        j = d[0] if d is not None else int(ref["iters"][p]) - 1
        if not is_ill:
            assert d[1] in ("flag", "stop"), (label, p, d, "a well-determined problem leaves the restatement in its " + d[1], got["errs"][p][j], re_[j])
            assert j >= 0, (label, p, "no common iteration")
            assert ref["margins"][p][j] <= 2 * noise(p, re_[j]), (label, p, f"runs part at iteration {j} away from the round-off of the cost",
                                                                   ref["margins"][p][j], noise(p, re_[j]), int(got["stop"][p]), int(ref["stop"][p]))
        else:
            n_ill += 1
        acc = [i for i in range(max(j, 0) + 1) if rs[i] and gs[i]]
        last_common = re_[acc[-1]] if acc else re_[0]
        for name, c in (("got", got["cost"][p]), ("ref", ref["cost"][p])):
            assert c <= last_common + K_COST * noise(p, last_common), (label, p, name, "final cost above the last common accepted cost", c, last_common)
        parted += 1
        at.append(j)
    return {"full": full, "parted": parted, "ill": n_ill, "parted_at": at, "max_cost_dev": dev}


def logit_data(P, n, items, dtype, seed=0, signal=0.3):
    """Logistic problems with noisy labels: A [P, items, n] of magnitude U(0.5, 1.5) / sqrt(n) and random sign, labels sign(signal * a.w + N(0, 1)) for a planted w ~ N(0, I).
    Returns (A, labels, data [P, items, n + 1])."""
    rng = np.random.default_rng(seed + 1000 * n + items)
    # (magnitudes in [0.5, 1.5]: no feature near 0 — with ONE item and ONE parameter the first pair's y = g - g_acc would cancel)
    A = (rng.uniform(0.5, 1.5, (P, items, n)) * rng.choice([-1.0, 1.0], (P, items, n)) / np.sqrt(n)).astype(dtype)
    w = rng.standard_normal((P, n))
    z = np.einsum("pin,pn->pi", A.astype(np.float64), w)
    yl = np.where(signal * z + rng.standard_normal(z.shape) > 0, 1.0, -1.0).astype(dtype)
    return A, yl, np.concatenate([A, yl[:, :, None]], axis=2)


# ---- the known-answer costs of the tests, in the problem's dtype ---------------------------------------------------------
def rosenbrock(x, T):
    T = np.dtype(T).type
    a, b = T(x[0]), T(x[1])
    u, v = b - a * a, T(1) - a
    return T(100) * u * u + v * v, np.array([T(-400) * a * u - T(2) * v, T(200) * u], T)


def powell(x, T):
    """Powell's singular function: (x0 + 10 x1)^2 + 5 (x2 - x3)^2 + (x1 - 2 x2)^4 + 10 (x0 - x3)^4."""
    T = np.dtype(T).type
    x = np.asarray(x, T)
    a, b, c, d = x[0] + T(10) * x[1], x[2] - x[3], x[1] - T(2) * x[2], x[0] - x[3]
    cost = a * a + T(5) * b * b + c * c * c * c + T(10) * d * d * d * d
    g = np.array([T(2) * a + T(40) * d * d * d, T(20) * a + T(4) * c * c * c, T(10) * b - T(8) * c * c * c, T(-10) * b - T(40) * d * d * d], T)
    return cost, g
