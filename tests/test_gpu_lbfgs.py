"""Batched L-BFGS on scalar cost models (Options.LBFGS, toa_jit_lbfgs_run) against the numpy restatement of its
state machine (tests/lbfgs_reference.py), known minimisers, the second-order door, and itself (queue, ragged, repeated runs).

How a run is compared with the restatement (lbfgs_reference.compare_trajectories): iteration by iteration the same accept / reject
flag and the same cost to K_COST = 64 x the round-off bound of one evaluation of the cost (41 passes accumulate), then the same ending, the final x to tests/parity.py's
tolerance.  A problem may leave the restatement only at a cost decision (Armijo, min_error, min_rerr_dec, the round-off floor) that
the restatement took within 2 x that bound (two costs enter a decision), or as a problem that the restatement itself does not
determine to K_ILL = 16 x the bound (one of three twins over a 4-ulp perturbation of costs and gradients leaves it: ill_determined;
decided on the CPU, before the device is looked at).  Both kinds count against the cap of 5 % of a case's problems.
The round-off bound of a logistic cost c = sum_i log(1 + exp(-y_i z_i)) over `items` terms in a format of precision eps:
    eps * ((items + 4) * sum |c_i|  +  items)
— items * eps * sum |c_i| for the order of the sum, 4 ulp for what exp and log of the two sides differ by, and eps per term because
1 + e is rounded before the logarithm (an absolute error: it is all that is left of a term once e < eps).
Data: labels sign(0.3 a.w + N(0, 1)) — noisy enough that every problem with more items than parameters has a finite, well-conditioned
minimiser.  With the cleaner labels of tests/test_gpu_gd.py (0.5 noise on a.w of unit variance) 63 - 65 items in 12 or 13 dimensions are
nearly separable, the minimiser lies far out, and L-BFGS amplifies last places by 1e2 - 1e4 x the bound in a fifth of the problems: no run
can be held to the bound there, the restatement's own twin included.  Separable problems remain where the issue asks for them (fewer
items than parameters); they are what the ill-determined class is for.
fp32 runs stop at thresholds of their own precision (min_error = min_rerr_dec = 1e-3: an order above the round-off of the sum of
1 000 terms, 1.2e-4, below which a decrease cannot be told from none) — with the fp64 defaults EVERY fp32 problem ends on a last-bit decision;
test_fp32_under_the_defaults compares the end state there.
The largest cost tolerance applied in any case is K_COST = 64 x the bound.  What the device needed of it on an MI355X: below 1 x the
bound wherever a problem has more items than parameters, up to 3.6 x (fp32) and 10.8 x (fp64, n = 63 with 64 items) in the separable
cases; parted problems per case: 0 - 2, and 4 of 97 in two fp32 cases at n = 1 (Armijo ties on the fp32 floor after a superlinear
step); ill-determined: 0 or 1 per trajectory case, 8 at history 1.
Seed 0 of the generator; checked on the CPU over all forty (dtype, n, items) cases: the ill-determined problems and the problems at
which the twin parts stay inside the cap in every case (tests/test_cpu_lbfgs_reference.py repeats two of them)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gd_reference as gr  # noqa: E402
import hess_reference as hr  # noqa: E402
import lbfgs_reference as lr  # noqa: E402
from parity import gpu_dict  # noqa: E402
from test_gpu_gd import QUARTIC_COST, QUARTIC_GRAD, logit_body  # noqa: E402
from tinyopt_amd.api import default_context  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {np.float32: torch.float32, np.float64: torch.float64}
P = 97
CAP = 0.05
_MODELS, _REFS = {}, {}


def _logit_data(P, n, items, dtype, seed=0):
    return lr.logit_data(P, n, items, dtype, seed)


def _res(ta, body, n, kD, dtype, kind):
    key = (body, n, kD, dtype, kind)
    if key not in _MODELS:
        _MODELS[key] = ta.JitResidual(body, n=n, item_scalars=kD, dtype=TDT[dtype], kind=kind)
    return _MODELS[key]


def _options(ta, dtype=np.float64, **kw):
    o = ta.Options()
    o.solver_type = ta.Options.LBFGS
    o.hessian.save_last = False
    o.max_iters = 40
    if dtype == np.float32:   # (thresholds of the format's own precision: the module docstring)
        o.min_error, o.min_rerr_dec = 1e-3, 1e-3
    for k, v in kw.items():
        if k in ("history", "c1", "shrink"):
            setattr(o.lbfgs, k, v)
        elif k in ("use_squared_norm", "downscale_by_2", "normalize"):
            setattr(o.cost, k, v)
        else:
            setattr(o, k, v)
    return o


def _noise(items, dtype):
    eps = float(np.finfo(dtype).eps)
    return lambda p, c: eps * ((items + 4) * abs(c) + items)


def _reference(n, items, dtype, o, key=(), noise=None):
    """(ref, ill) of the logistic case, computed once per (n, items, dtype, options) and shared by every test that needs it."""
    k = (n, items, dtype, o.lbfgs.history, key)
    if k not in _REFS:
        A, yl, _ = _logit_data(P, n, items, dtype)
        f = lambda p, xx: gr.logistic(A[p], yl[p], xx, dtype)   # noqa: E731
        x0 = np.zeros((P, n), dtype)
        pod = o.to_pod()
        ref = lr.lbfgs_optimize(x0, f, pod, dtype, o.lbfgs.history, o.lbfgs.c1, o.lbfgs.shrink)
        fast = lambda p, xx: lr.logistic_fast(A[p], yl[p], xx, dtype)   # noqa: E731
        rel = 4 * float(np.finfo(dtype).eps)
        twins = [lr.lbfgs_optimize(x0, lr.perturbed(fast, rel, seed), pod, dtype, o.lbfgs.history, o.lbfgs.c1, o.lbfgs.shrink) for seed in (1, 2, 3)]
        _REFS[k] = (ref, lr.ill_determined(ref, twins, dtype, noise or _noise(items, dtype)))
    return _REFS[k]


def _run(ta, n, items, dtype, kind, o, history=True, out=None):
    _, _, data = _logit_data(P, n, items, dtype)
    model = _res(ta, logit_body(n, kind), n, n + 1, dtype, kind).bind(torch.from_numpy(data).cuda())
    x = torch.zeros(P, n, dtype=TDT[dtype], device="cuda")
    out = ta.Optimize(x, model, o, history=history, out=out)
    torch.cuda.synchronize()
    return out, x


def _check_case(ta, n, items, dtype, kind, o, key=(), noise=None, cap_ill=True):
    out, x = _run(ta, n, items, dtype, kind, o)
    noise = noise or _noise(items, dtype)
    ref, ill = _reference(n, items, dtype, o, key, noise)
    label = f"logit n={n} items={items} {kind} {np.dtype(dtype).name} {key}"
    st = lr.compare_trajectories(gpu_dict(out, x), ref, dtype, noise, label, ill=ill)
    print(label, st)   # (the largest cost tolerance applied is K_COST x the bound; max_cost_dev is what the run needed of it)
    assert st["parted"] - (0 if cap_ill else st["ill"]) <= CAP * P, (label, st)
    return out, x, ref


# ---------------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,kind", [(1, "cost_grad"), (12, "cost_grad"), (13, "cost_grad"), (63, "cost_grad"), (12, "cost"), (13, "cost")])
def test_logistic_trajectories(ta, n, kind, dtype):
    """P = 97, every item count around the wave width, max_iters = 40; 12 | 13 is the register-x / LDS-x border of CostModel::pass."""
    for items in (1, 63, 64, 65, 1000):
        _check_case(ta, n, items, dtype, kind, _options(ta, dtype))


@pytest.mark.parametrize("history", [1, 3, 8, 16])
def test_history_sizes(ta, history):
    """n = 63 with 65 items is separable: the minimiser lies at infinity, and with ONE pair of history the solve crawls there for all
    41 passes, amplifying last places on the way — the restatement does not determine 8 (fp64) to 13 (fp32) of the 97 problems at
    history 1 (0 - 2 at history 3, 8 and 16; found on the CPU).  The cap of 5 % here is on the problems that part at a decision; the
    ill-determined ones are printed, their flags and their final cost are still checked."""
    for dtype in (np.float32, np.float64):
        _check_case(ta, 63, 65, dtype, "cost_grad", _options(ta, dtype, history=history), cap_ill=False)


def test_fp32_under_the_defaults(ta):
    """The options users and the probe run, in fp32: every problem ends on its round-off floor, so trajectories are not comparable, the
    end state is.  n = 12, 1 000 items (a finite, well-conditioned minimiser): the cost at the device's final x, evaluated in fp64,
    is within the fp32 round-off bound of the minimum f* (the fp64 restatement run to its floor), as the fp32 restatement's
    is; x is within sqrt(2 (f - f*) / mu) of the minimiser, mu the smallest eigenvalue of the Hessian there; the endings are
    successes and those of the floor (kMinRelError, kMinDeltaNorm, kMaxConsecNoDecr) and agree with the restatement's in kind."""
    n, items = 12, 1000
    A, yl, data = _logit_data(P, n, items, np.float32)
    o = _options(ta, max_iters=50)            # (fp64 thresholds: the defaults)
    x = torch.zeros(P, n, dtype=torch.float32, device="cuda")
    out = ta.Optimize(x, _res(ta, logit_body(n, "cost_grad"), n, n + 1, np.float32, "cost_grad").bind(torch.from_numpy(data).cuda()), o, history=True)
    torch.cuda.synchronize()
    A64, y64 = A.astype(np.float64), yl.astype(np.float64)
    pod = o.to_pod()
    r32 = lr.lbfgs_optimize(np.zeros((P, n), np.float32), lambda p, xx: gr.logistic(A[p], yl[p], xx, np.float32), pod, np.float32)
    r64 = lr.lbfgs_optimize(np.zeros((P, n)), lambda p, xx: gr.logistic(A64[p], y64[p], xx, np.float64), _options(ta, max_iters=100, min_rerr_dec=1e-14).to_pod(), np.float64)
    xg, stops = x.cpu().numpy().astype(np.float64), out.stop_reason.cpu().numpy()
    floor = {gr.STOP_MIN_REL_ERROR, gr.STOP_MIN_DELTA_NORM, gr.STOP_MAX_CONSEC_NO_DECR}
    assert set(stops.tolist()) <= floor and set(r32["stop"].tolist()) <= floor, (set(stops.tolist()), set(r32["stop"].tolist()))
    noise = _noise(items, np.float32)
    for p in range(P):
        fstar = float(gr.logistic(A64[p], y64[p], r64["x"][p], np.float64)[0])
        sig = 1.0 / (1.0 + np.exp(-(A64[p] @ r64["x"][p])))
        mu = np.linalg.eigvalsh(A64[p].T @ (A64[p] * (sig * (1 - sig))[:, None])).min()
        for name, xe in (("device", xg[p]), ("restatement", r32["x"][p].astype(np.float64))):
            gap = float(gr.logistic(A64[p], y64[p], xe, np.float64)[0]) - fstar
            assert -noise(p, fstar) <= gap <= noise(p, fstar), (name, p, gap, noise(p, fstar))
            assert np.abs(xe - r64["x"][p]).max() <= np.sqrt(2 * noise(p, fstar) / (0.9 * mu)), (name, p)
    assert abs(int((stops == gr.STOP_MAX_CONSEC_NO_DECR).sum()) - int((r32["stop"] == gr.STOP_MAX_CONSEC_NO_DECR).sum())) <= 0.25 * P
    assert (out.num_iters.cpu().numpy() <= o.max_iters + 1).all() and (out.final_cost.cpu().numpy() > 0).all()


# ---------------------------------------------------------------------------------------------------- known answers
ROSENBROCK = ("const T u = x[1] - x[0] * x[0], v = T(1) - x[0]; c = T(100) * u * u + v * v;\n"
              "if (want_grad) { G[0] += T(-400) * x[0] * u - T(2) * v; G[1] += T(200) * u; }")
POWELL = ("const T a = x[0] + T(10) * x[1], b = x[2] - x[3], q = x[1] - T(2) * x[2], d = x[0] - x[3];\n"
          "c = a * a + T(5) * b * b + q * q * q * q + T(10) * d * d * d * d;\n"
          "if (want_grad) { G[0] += T(2) * a + T(40) * d * d * d; G[1] += T(20) * a + T(4) * q * q * q;\n"
          "  G[2] += T(10) * b - T(8) * q * q * q; G[3] += T(-10) * b - T(40) * d * d * d; }")


def _solve_one_item(ta, body, kind, x0, o, value=0.0):
    n = x0.shape[1]
    model = _res(ta, body, n, 1, np.float64, kind).bind(torch.full((x0.shape[0], 1, 1), value, dtype=torch.float64, device="cuda"))
    x = torch.from_numpy(x0.copy()).cuda()
    out = ta.Optimize(x, model, o, history=True)
    torch.cuda.synchronize()
    return out, x


def test_known_minimisers(ta):
    """Rosenbrock from around (-1.2, 1) (the start itself takes 55 passes in the restatement), the reference's quartic from [36, 40], Powell's singular function from around (3, -1, 0, 1):
    64 start points each, fp64, as one-item models."""
    rng = np.random.default_rng(11)
    # (max_consec_failures = 0: in the curved valley a line search may need more than five halvings of a unit step)
    x0 = np.array([-1.2, 1.0]) + 0.02 * rng.uniform(-1, 1, (64, 2))
    out, x = _solve_one_item(ta, ROSENBROCK, "cost_grad", x0, _options(ta, max_iters=500, max_consec_failures=0))
    assert out.Converged().all() and np.abs(x.cpu().numpy() - 1.0).max() < 1e-5, (out.stop_reason, x)
    for body, kind in ((QUARTIC_GRAD, "cost_grad"), (QUARTIC_COST, "cost")):
        x0 = np.linspace(36.0, 40.0, 64)[:, None]
        out, x = _solve_one_item(ta, body, kind, x0, _options(ta, max_iters=200, min_error=0.0), 42.0)
        assert out.Converged().all() and np.abs(x.cpu().numpy() - 42.0).max() < 1e-5
        assert np.abs(out.final_cost.cpu().numpy() + 2.0).max() < 1e-9
        ref = lr.lbfgs_optimize(x0, lambda p, xx: gr.quartic(xx, np.float64), _options(ta, max_iters=200, min_error=0.0).to_pod(), np.float64)
        assert (out.num_iters.cpu().numpy() <= ref["iters"] + 3).all()   # (and nowhere near gradient descent's 1 000 passes)
    x0 = np.array([3.0, -1.0, 0.0, 1.0]) * (1.0 + 0.2 * rng.uniform(-1, 1, (64, 4))) + np.array([0, 0, 0.1, 0]) * rng.uniform(-1, 1, (64, 1))
    o = _options(ta, max_iters=400, max_consec_failures=0)
    out, x = _solve_one_item(ta, POWELL, "cost_grad", x0, o)
    cost = out.final_cost.cpu().numpy()
    assert (out.stop_reason.cpu().numpy() >= 1).all()
    assert (cost < 1e-8).all(), cost.max()            # the minimum 0 at the origin is degenerate (a singular Hessian): approached, slowly
    assert (cost < o.min_error).sum() >= 32, (cost < o.min_error).sum()


def test_against_the_newton_solve(ta):
    """Logistic, n = 12, fp64: L-BFGS and the cost_hess Newton solve end at the same minimum.  f - f* <= |g|^2 / (2 mu) at each end,
    mu = 0.9 x the smallest eigenvalue of A^T D A at the Newton solution (the margin of tests/test_cpu_lbfgs_reference.py)."""
    n, items, Pn = 12, 300, 16
    cases = [hr.logistic_case(s, n, items) for s in range(Pn)]
    data = np.stack([c[0] for c in cases])
    x0 = np.stack([c[1] for c in cases])
    dev = torch.from_numpy(data).cuda()
    newton = _res(ta, hr.logistic_body(n), n, n + 1, np.float64, "cost_hess").bind(dev)
    xn = torch.from_numpy(x0.copy()).cuda()
    on = ta.Options()
    on.hessian.save_last = False
    outn = ta.Optimize(xn, newton, on)
    lb = _res(ta, logit_body(n, "cost_grad"), n, n + 1, np.float64, "cost_grad").bind(dev)
    xl = torch.from_numpy(x0.copy()).cuda()
    outl = ta.Optimize(xl, lb, _options(ta, max_iters=100, min_rerr_dec=1e-14))
    torch.cuda.synchronize()
    assert outn.Converged().all() and (outl.stop_reason.cpu().numpy() >= 1).all()
    fn, fl = outn.final_cost.cpu().numpy(), outl.final_cost.cpu().numpy()
    for p in range(Pn):
        A, y = data[p, :, :n], data[p, :, n]
        sig = 1.0 / (1.0 + np.exp(-(A @ xn.cpu().numpy()[p])))
        # f - f* <= |g|^2 / (2 mu) needs mu below the Hessian on the way to the minimiser: sigma (1 - sigma) changes by at most
        # exp(-|dz|) over a change dz of an item's z, and |dz| <= |a_i| |dx| — the factor is computed and must stay above the 0.9 used
        dx = np.abs(xl.cpu().numpy()[p] - xn.cpu().numpy()[p]).max() * np.sqrt(n)
        assert np.exp(-3 * np.linalg.norm(A, axis=1).max() * dx) >= 0.9, (p, dx)
        mu = 0.9 * np.linalg.eigvalsh(A.T @ (A * (sig * (1 - sig))[:, None])).min()
        gl = gr.logistic(A, y, xl.cpu().numpy()[p], np.float64)[1]
        gn = gr.logistic(A, y, xn.cpu().numpy()[p], np.float64)[1]
        # (both ends lie above f*, each by at most its own bound: their difference by at most the larger; plus the round-off of f)
        bound = max(gl @ gl, gn @ gn) / (2 * mu) + _noise(items, np.float64)(p, fn[p])
        print(p, fl[p], fn[p], bound)
        assert abs(fl[p] - fn[p]) <= bound, (p, fl[p], fn[p], bound)


# ---------------------------------------------------------------------------------------------------- queue, reset, ragged
def _bits(out, x):
    return [t.cpu().numpy().copy() for t in (x, out.stop_reason, out.num_iters, out.num_failures, out.final_cost, out.errs, out.successes)]


def test_queue_and_ring_reset(ta):
    """More problems than the launch has waves: the later ones are popped from the queue by a wave that has solved one before.  Every
    problem is bit-equal to itself in a batch of 97 (a ring or a line search left over from the wave's last problem would show), a
    permuted batch gives the permuted bits, two runs the same bits."""
    n, items = 3, 64
    A, yl, data = _logit_data(P, n, items, np.float64)
    rng = np.random.default_rng(5)
    x0 = 0.5 * rng.standard_normal((P, n))
    res = _res(ta, logit_body(n, "cost_grad"), n, n + 1, np.float64, "cost_grad")
    waves = default_context().info()["num_cus"] * res.stats_lbfgs()["wg_per_cu"] * 4
    big = waves + 4 * P + 13
    o = _options(ta)

    def solve(idx):
        model = res.bind(torch.from_numpy(data[idx]).cuda())
        x = torch.from_numpy(x0[idx].copy()).cuda()
        out = ta.Optimize(x, model, o, history=True)
        torch.cuda.synchronize()
        return _bits(out, x)

    base = solve(np.arange(P))
    assert len(set(base[2].tolist())) > 3          # (problems of different lengths: the queue hands them out unevenly)
    idx = np.arange(big) % P
    one, two = solve(idx), solve(idx)
    perm = rng.permutation(big)
    three = solve(idx[perm])
    for a, b, c, d in zip(base, one, two, three):
        assert (b == a[idx]).all() and (c == b).all() and (d == a[idx[perm]]).all()


def test_ragged_is_bit_equal_to_uniform(ta):
    n, dtype = 12, np.float64
    counts = np.array([0, 1, 63, 64, 65, 2, 64, 0, 65, 63, 1, 128, 64, 0, 130, 65, 63, 1, 64, 3])
    Pr = len(counts)
    A, yl, data = _logit_data(Pr, n, int(counts.max()), dtype)
    rng = np.random.default_rng(3)
    x0 = 0.3 * rng.standard_normal((Pr, n))
    res = _res(ta, logit_body(n, "cost_grad"), n, n + 1, dtype, "cost_grad")
    flat = np.concatenate([data[p, :counts[p]] for p in range(Pr)])
    o = _options(ta)
    for keep in (False, True):
        x = torch.from_numpy(x0.copy()).cuda()
        out = ta.Optimize(x, res.bind_ragged(torch.from_numpy(flat).cuda(), counts=counts), o, history=True, keep_order=keep)
        torch.cuda.synchronize()
        got = _bits(out, x)
        for cnt in sorted(set(counts.tolist())):
            idx = np.flatnonzero(counts == cnt)
            if cnt == 0:
                assert (got[1][idx] == lr.STOP_SKIPPED).all() and (got[0][idx] == x0[idx]).all() and (got[2][idx] == 0).all()
                continue
            xu = torch.from_numpy(x0[idx].copy()).cuda()
            outu = ta.Optimize(xu, res.bind(torch.from_numpy(np.ascontiguousarray(data[idx, :cnt])).cuda()), o, history=True)
            torch.cuda.synchronize()
            for a, b in zip(got, _bits(outu, xu)):
                assert (a[idx] == b).all(), (cnt, keep)
    assert res.stats_lbfgs(ragged=True)["scratch_bytes"] == 0


# ---------------------------------------------------------------------------------------------------- options, outputs
@pytest.mark.parametrize("variant", ["sqrt_norm", "downscale_by_2", "normalize", "min_grad_norm2", "max_total_failures", "check_final_cost",
                                     "c1_shrink"])
def test_options_variants(ta, variant):
    """Options that change the loop or the reported costs, each against the restatement (logistic, n = 3, 64 items, fp64)."""
    kw = {"sqrt_norm": dict(use_squared_norm=False), "downscale_by_2": dict(downscale_by_2=True), "normalize": dict(normalize=True),
          "min_grad_norm2": dict(min_grad_norm2=1e-2), "max_total_failures": dict(max_total_failures=1, max_consec_failures=0, c1=0.3),
          "check_final_cost": dict(check_final_cost=True), "c1_shrink": dict(c1=0.3, shrink=0.25)}[variant]
    o = _options(ta, **kw)
    raw = _noise(64, np.float64)
    # (the noise in the units of the REPORTED cost: sqrt(c) moves by noise / (2 sqrt(c)), c / 2 by half of it)
    noise = {"sqrt_norm": lambda p, e: raw(p, e * e) / (2 * max(abs(e), 1e-300)), "downscale_by_2": lambda p, e: raw(p, 2 * e) / 2}.get(variant, raw)
    out, x, ref = _check_case(ta, 3, 64, np.float64, "cost_grad", o, key=variant, noise=noise)
    stops = out.stop_reason.cpu().numpy()
    if variant == "min_grad_norm2":
        assert (stops == gr.STOP_MIN_GRAD_NORM).sum() >= 10
    if variant == "max_total_failures":
        assert (stops == gr.STOP_MAX_NO_DECR).sum() >= 10 and (out.num_failures.cpu().numpy()[stops == gr.STOP_MAX_NO_DECR] == 1).all()
    if variant == "check_final_cost":   # accepted and ignored: the bits of the run without it
        o2, x2 = _run(ta, 3, 64, np.float64, "cost_grad", _options(ta))
        assert torch.equal(x, x2) and torch.equal(out.num_iters, o2.num_iters) and torch.equal(out.final_cost, o2.final_cost)


def test_outputs_history_and_callers_out(ta):
    o = _options(ta)
    out, x = _run(ta, 12, 65, np.float64, "cost_grad", o)
    assert out.final_hessian is None
    assert (out.final_num_residuals.cpu().numpy() == 1).all() and (out.final_inlier_ratio.cpu().numpy() == 1).all()
    iters = out.num_iters.cpu().numpy()
    cnt = out.counters.cpu().numpy()
    assert cnt[0] == iters.sum() and cnt[3] == P and cnt[1] == 0
    ref, _ = _reference(12, 65, np.float64, o)
    same = iters == ref["iters"]
    assert same.sum() >= (1 - CAP) * P
    # (|trial - x_acc|^2, 0 at the first pass; the first rows, before L-BFGS has amplified the last places of the steps)
    assert (out.deltas2.cpu().numpy()[:, 0] == 0).all()
    assert np.allclose(out.deltas2.cpu().numpy()[same, :4], ref["deltas2"][same, :4], rtol=1e-8, atol=1e-300)
    assert (out.num_consec_failures.cpu().numpy()[same] == ref["consec"][same]).all()
    assert np.allclose(out.final_rerr_dec.cpu().numpy()[same], ref["rerr"][same], rtol=1e-5, atol=1e-11)
    plain, xp = _run(ta, 12, 65, np.float64, "cost_grad", o, history=False)
    assert plain.errs is None and torch.equal(xp, x) and torch.equal(plain.num_iters, out.num_iters) and torch.equal(plain.final_cost, out.final_cost)
    o.hessian.save_last = True          # (no final Hessian whatever save_last says)
    mine = ta.api._alloc_output(P, 12, o, True, "cuda", final_hessian=False)
    got, xg = _run(ta, 12, 65, np.float64, "cost_grad", o, out=mine)
    assert got is mine and got.final_hessian is None and torch.equal(xg, x) and torch.equal(got.errs, out.errs)
    fresh, _ = _run(ta, 12, 65, np.float64, "cost_grad", o)
    assert fresh.final_hessian is None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_scratch_at_n12(ta, dtype):
    for kind in ("cost", "cost_grad"):
        s = _res(ta, logit_body(12, kind), 12, 13, dtype, kind).stats_lbfgs()
        assert s["scratch_bytes"] == 0, (kind, s)
        assert s["wg_per_cu"] >= 1 and s["num_regs"] > 0


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(ta):
    n, items, Pq = 3, 64, 8
    _, _, data = _logit_data(Pq, n, items, np.float64)
    dev = torch.from_numpy(data).cuda()
    res = _res(ta, logit_body(n, "cost_grad"), n, n + 1, np.float64, "cost_grad")
    model = res.bind(dev)
    x = torch.zeros(Pq, n, dtype=torch.float64, device="cuda")
    gdo = ta.Options()
    gdo.solver_type = ta.Options.GradientDescent
    gdo.hessian.save_last = False
    xg = x.clone()
    before = ta.Optimize(xg, model, gdo)
    torch.cuda.synchronize()
    o = _options(ta)
    # models that are no first-order scalar cost
    residual = ta.JitResidual("r[0] = x[0] - p[0];", n=1, item_scalars=1)
    rm = residual.bind(torch.ones(Pq, 4, 1, dtype=torch.float64, device="cuda"))
    x1 = torch.zeros(Pq, 1, dtype=torch.float64, device="cuda")
    acc = ta.JitResidual("r[0] = x[0] - p[0]; if (want_grad) { J[0][0] = T(1); }", n=1, item_scalars=1, kind="accumulate")
    am = acc.bind(torch.ones(Pq, 4, 1, dtype=torch.float64, device="cuda"))
    hess = _res(ta, hr.logistic_body(n), n, n + 1, np.float64, "cost_hess").bind(dev)
    big = ta.JitResidual("r[0] = x[0] - p[0];", n=70, item_scalars=1, large_n=True)
    bm = big.bind(torch.ones(Pq, 80, 1, dtype=torch.float64, device="cuda"))
    for m, xx in ((rm, x1), (am, x1), (hess, x), (bm, torch.zeros(Pq, 70, dtype=torch.float64, device="cuda")),
                  (rm.with_prior(torch.zeros(Pq, 1, dtype=torch.float64, device="cuda"), torch.ones(Pq, 1, dtype=torch.float64, device="cuda")), x1),
                  (rm.with_bounds(torch.zeros(Pq, 1, dtype=torch.float64, device="cuda") - 1, None), x1)):
        with pytest.raises(ValueError, match="L-BFGS"):
            ta.Optimize(xx, m, o)
    for attach in (lambda m: m.with_prior(torch.zeros(Pq, n, dtype=torch.float64, device="cuda"), torch.ones(Pq, n, dtype=torch.float64, device="cuda")),
                   lambda m: m.with_bounds(torch.zeros(Pq, n, dtype=torch.float64, device="cuda") - 1, None)):
        with pytest.raises(ValueError, match="scalar cost model"):      # a cost model never carries a prior or bounds: refused when attached,
            attach(model)                                                # so ("prior" | "bounds", "lbfgs") speak for residual models only
    with pytest.raises(ta.ToaError, match="loss"):                       # a scalar cost has no residuals to robustify
        ta.Optimize(x, model.with_loss("huber", 1.0), o)
    ta.Optimize(x.clone(), model, o)                                      # (the handle's loss is cleared again)
    torch.cuda.synchronize()
    for kw in (dict(grad_clipping=0.5), dict(history=0), dict(history=17), dict(c1=0.0), dict(c1=1.0), dict(shrink=0.0), dict(shrink=1.0),
               dict(max_duration_ms=5.0), dict(stop_callback=lambda e, d, g: False)):
        with pytest.raises(ValueError, match="L-BFGS"):
            ta.Optimize(x, model, _options(ta, **kw))
    with pytest.raises(ValueError, match="splits"):
        ta.Optimize(x, model, o, splits=4)
    with pytest.raises(ValueError, match="no stepping form"):
        ta.Optimizer(x, model, o)
    # the raw C entry
    ctx = default_context()
    from tinyopt_amd._capi import ToaLbfgsOptions, ToaResults
    lb = ToaLbfgsOptions()
    ctx.lib.toa_lbfgs_options_default(C.byref(lb))
    assert (lb.history, lb.c1, lb.shrink) == (8, pytest.approx(1e-4), 0.5)
    pod = o.to_pod()
    res0 = ToaResults()
    run = lambda h, p, l: ctx.lib.toa_jit_lbfgs_run(ctx.h, h, items, 0, None, None, C.byref(p), C.byref(l), C.byref(res0), None)   # noqa: E731
    assert run(res._h, pod, lb) == 0                                      # P = 0
    for st in (0, 1, 2):
        pod.solver_type = st
        assert run(res._h, pod, lb) != 0 and b"solver_type must be 3" in ctx.lib.toa_last_error()
    pod.solver_type = 3
    for field, bad in (("history", 0), ("history", 17), ("c1", 0.0), ("c1", 1.0), ("shrink", 0.0), ("shrink", 1.0)):
        lb2 = ToaLbfgsOptions()
        ctx.lib.toa_lbfgs_options_default(C.byref(lb2))
        setattr(lb2, field, bad)
        assert run(res._h, pod, lb2) != 0 and field.encode() in ctx.lib.toa_last_error()
    pod.grad_clipping = 0.5
    assert run(res._h, pod, lb) != 0 and b"grad_clipping" in ctx.lib.toa_last_error()
    pod.grad_clipping = 0.0
    for other in (residual, acc, _res(ta, hr.logistic_body(n), n, n + 1, np.float64, "cost_hess"), big):
        assert run(other._h, pod, lb) != 0
        v = [C.c_int(0) for _ in range(3)]
        assert ctx.lib.toa_jit_model_stats_lbfgs(ctx.h, other._h, 0, *[C.byref(t) for t in v]) != 0
    # a GD run on the same handle afterwards: the bits it gave before
    xg2 = x.clone()
    after = ta.Optimize(xg2, model, gdo)
    torch.cuda.synchronize()
    assert torch.equal(xg, xg2) and torch.equal(before.num_iters, after.num_iters) and torch.equal(before.final_cost, after.final_cost)


def test_first_use_under_capture_is_refused(ta):
    """The L-BFGS code object is built lazily: its first use cannot happen inside a stream capture; afterwards the model runs."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        n, items, Pq = 2, 8, 8
        _, _, data = _logit_data(Pq, n, items, np.float64)
        fresh = ta.JitResidual(logit_body(n, "cost_grad"), n=n, item_scalars=n + 1, dtype=torch.float64, kind="cost_grad")
        model = fresh.bind(torch.from_numpy(data).cuda())
        x = torch.zeros(Pq, n, dtype=torch.float64, device="cuda")
        gdo = ta.Options()
        gdo.solver_type = ta.Options.GradientDescent
        gdo.hessian.save_last = False
        ta.Optimize(x.clone(), model, gdo)           # (the handle's workspaces exist)
        o = _options(ta)
        out = ta.api._alloc_output(Pq, n, o, False, x.device, final_hessian=False)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(Exception, match="cannot happen while the stream is being captured"):
            with torch.cuda.graph(g, stream=s):
                ta.Optimize(x, model, o, out=out)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        o2 = ta.Optimize(x, model, _options(ta))
        s.synchronize()
        assert bool((o2.stop_reason > 0).all())
