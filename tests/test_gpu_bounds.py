"""Box bounds and fixed parameters of run-time models (JitModel.with_bounds / RaggedJitModel.with_bounds; toa_jit_*_bounds,
csrc/bounds.hpp).  Yardsticks: the seam of the same model without bounds plus rule 2 in numpy, bit for bit; the
plain Optimize for bounds that never bind, bit for bit; the oracle's DenseRow on the reduced problem for fixed parameters; the
second reading's LM loop inside the rules of tests/bounds_reference.py for binding bounds, whole trajectories; the uniform bounded
solve for every problem of a ragged bounded batch, bit for bit.  Every solve here also asserts lo <= x <= hi exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_reference as br  # noqa: E402
from parity import check_trajectories, gpu_dict  # noqa: E402
from test_gpu_jit import CIRCLE  # noqa: E402
from test_gpu_prior import circle_uniform, cuda, make_prior, types_of  # noqa: E402
from test_gpu_ragged import OUT_FIELDS, SKIPPED, TDT, Case, _res, circle_options  # noqa: E402
from test_gpu_row_models import ad_body, manual_body  # noqa: E402

pytestmark = pytest.mark.gpu

ref = br.ref
INF = np.inf
ROW_N = 20
SOLVER_FAILED = -3


def assert_inside(x, lo, hi, label=""):
    """invariant 5: comparisons, not tolerances"""
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert np.all(x >= lo) and np.all(x <= hi), (label, "x left the box", x, lo, hi)


def bounded(model, lo, hi):
    return model.with_bounds(cuda(lo), cuda(hi))


# ---- 1. the seam: rule 2 on g and H, bit for bit ---------------------------------------------------------------------------------------
def rule2_np(x, g, H, lo, hi):
    act = (lo == hi) | ((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0))
    g, H = g.copy(), H.copy()
    g[act] = 0
    for p in range(len(x)):
        H[p][act[p], :] = 0
        H[p][:, act[p]] = 0
        idx = np.nonzero(act[p])[0]
        H[p][idx, idx] = 1
    return g, H, act


def seam_box(x, g):
    """Bounds around a given x, parameter (p, j) by (p + j) % 6: 0 on a bound with the gradient pointing outward (active: the lower
    bound when g > 0, the upper when g < 0), 1 on a bound with the gradient pointing inward (free), 2 strictly inside a finite interval,
    3 lo == hi, 4 no bound, 5 outside the box on the side the gradient pushes to (x is taken as given: active).  Both gradient signs occur on
    both sides because the signs of g are the model's."""
    P, n = x.shape
    lo, hi = np.full((P, n), -INF, x.dtype), np.full((P, n), INF, x.dtype)
    cat = (np.arange(P)[:, None] + np.arange(n)[None]) % 6
    pos = g > 0
    lo[(cat == 0) & pos] = x[(cat == 0) & pos]
    hi[(cat == 0) & ~pos] = x[(cat == 0) & ~pos]
    hi[(cat == 1) & pos] = x[(cat == 1) & pos]
    lo[(cat == 1) & ~pos] = x[(cat == 1) & ~pos]
    lo[cat == 2] = x[cat == 2] - 0.25
    hi[cat == 2] = x[cat == 2] + 0.5
    lo[cat == 3] = x[cat == 3]
    hi[cat == 3] = x[cat == 3]
    lo[(cat == 5) & pos] = x[(cat == 5) & pos] + 0.125
    hi[(cat == 5) & ~pos] = x[(cat == 5) & ~pos] - 0.125
    want_active = ((cat == 0) | (cat == 3) | (cat == 5)) & ((g != 0) | (cat == 3))
    return lo, hi, want_active


def assert_seam(ta, base, x):
    """accumulate(base.with_bounds) is accumulate(base) with rule 2 applied in numpy: g, H, cost, nres bit for bit; H symmetric bit for
    bit; the cost-only call untouched."""
    g0, H0, c0, n0 = ta.accumulate(base, x)
    _, _, c0e, n0e = ta.accumulate(base, x, want_grad=False)
    torch.cuda.synchronize()
    xn, g0n, H0n = x.cpu().numpy(), g0.cpu().numpy(), H0.cpu().numpy()
    lo, hi, want_active = seam_box(xn, g0n)
    bm = bounded(base, lo, hi)
    g1, H1, c1, n1 = ta.accumulate(bm, x)
    _, _, c1e, n1e = ta.accumulate(bm, x, want_grad=False)
    torch.cuda.synchronize()
    gw, Hw, act = rule2_np(xn, g0n, H0n, lo, hi)
    assert np.array_equal(act, want_active)
    on_lo, on_hi, free = (xn == lo) & (lo != hi), (xn == hi) & (lo != hi), lo != hi
    four = [(act & on_lo).sum(), (~act & on_lo).sum(), (act & on_hi).sum(), (~act & on_hi).sum()]
    print("on lo active / free, on hi active / free:", four, "outside:", (act & free & ~on_lo & ~on_hi).sum(), "fixed:", (~free).sum())
    assert four[0] + four[2] > 0 and four[1] + four[3] > 0 and (~free).any() and (act & free & ~on_lo & ~on_hi).any()
    if xn.size >= 60:   # (which side a parameter sits on follows the sign of the model's gradient: both occur where there are enough of them)
        assert min(four) > 0, four
    H1n = H1.cpu().numpy()
    assert np.array_equal(g1.cpu().numpy(), gw), "g differs from rule 2 on the plain seam"
    assert np.array_equal(H1n, Hw), f"H differs from rule 2 on the plain seam: {np.abs(H1n - Hw).max()}"
    assert np.array_equal(H1n, np.swapaxes(H1n, 1, 2)), "H is not symmetric bit for bit"
    assert torch.equal(c1, c0) and torch.equal(n1, n0) and torch.equal(c1e, c0e) and torch.equal(n1e, n0e)


def seam_variants(model, x, dtype, n, seed):
    """the model as it is, with a Huber loss, and with a full prior (k = n rows)"""
    rng = np.random.default_rng(seed)
    mu, W = make_prior(rng, len(x), n, n, dtype, x, scale=2.0)
    return [model, model.with_loss("huber", 0.5), model.with_prior(cuda(mu), cuda(W))]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_seam_circle(ta, dtype):
    """JetModel: n = 3, 10 items."""
    pts, x = circle_uniform(dtype, P=8)
    model = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype]).bind(cuda(pts))
    for base in seam_variants(model, x, dtype, 3, 31):
        assert_seam(ta, base, cuda(x))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["residual", "accumulate"])
def test_seam_dense_row_n20(ta, oracle, kind, dtype):
    """RowModel: the DenseRow residual as text, n = 20, both kinds, 65 items (one row past a super-step of 64 rows)."""
    P, m = 3, 65
    A, b, x0, _ = oracle.synth_dense_row(P, ROW_N, m, dtype, seed=77)
    body = manual_body(ROW_N) if kind == "accumulate" else ad_body(ROW_N)
    model = _res(ta, body, n=ROW_N, item_scalars=ROW_N + 1, dtype=TDT[dtype], kind=kind).bind(cuda(np.concatenate([A, b[..., None]], -1)))
    for base in seam_variants(model, x0, dtype, ROW_N, 32):
        assert_seam(ta, base, cuda(x0))


def test_seam_last_lane_n63(ta, oracle):
    """n = 63 and 70 items, fp64: the last lane of the wave owns a parameter."""
    P, n, m, dtype = 2, 63, 70, np.float64
    A, b, x0, _ = oracle.synth_dense_row(P, n, m, dtype, seed=78)
    model = _res(ta, manual_body(n), n=n, item_scalars=n + 1, dtype=TDT[dtype], kind="accumulate").bind(cuda(np.concatenate([A, b[..., None]], -1)))
    for base in seam_variants(model, x0, dtype, n, 33):
        assert_seam(ta, base, cuda(x0))


# ---- 2. bounds that never bind: the plain solve, bit for bit ---------------------------------------------------------------------------
def assert_same_solve(ta, plain, model_of, x0, opts, P, n, dtype):
    """model_of(lo, hi) with -inf / +inf and with finite-but-far bounds against `plain`: x, every output field, the history."""
    x_ref = cuda(x0.copy())
    o_ref = ta.Optimize(x_ref, plain, opts, history=True)
    torch.cuda.synchronize()
    for lo_v, hi_v in ((-INF, INF), (-1e6, 1e6)):
        lo, hi = np.full((P, n), lo_v, dtype), np.full((P, n), hi_v, dtype)
        x = cuda(x0.copy())
        out = ta.Optimize(x, model_of(lo, hi), opts, history=True)
        torch.cuda.synchronize()
        assert torch.equal(x, x_ref), f"x differs by {float((x - x_ref).abs().max())} with bounds {lo_v} .. {hi_v}"
        for f in OUT_FIELDS:
            a, b = getattr(out, f), getattr(o_ref, f)
            if a is None and b is None:
                continue
            assert torch.equal(a, b), f"{f} differs with bounds {lo_v} .. {hi_v}"
        assert_inside(x, lo, hi)
    # (None for a side is the same model)
    x = cuda(x0.copy())
    ta.Optimize(x, model_of(None, None), opts)
    torch.cuda.synchronize()
    assert torch.equal(x, x_ref)


def test_never_binding_circle_and_loss(ta):
    dtype = np.float64
    pts, x0 = circle_uniform(dtype, P=6)
    x0 = np.tile(np.array([0.0, 0.0, 1.0]), (6, 1))       # (tests/circle.cpp's start: a longer route, with rejected steps)
    model = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype]).bind(cuda(pts))
    for plain in (model, model.with_loss("huber", 0.5)):
        assert_same_solve(ta, plain, lambda lo, hi, m=plain: m.with_bounds(None if lo is None else cuda(lo), None if hi is None else cuda(hi)),
                          x0, circle_options(ta), 6, 3, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_never_binding_dense_row_n20(ta, oracle, dtype):
    P, m = 4, 65
    A, b, x0, _ = oracle.synth_dense_row(P, ROW_N, m, dtype, seed=81)
    model = _res(ta, manual_body(ROW_N), n=ROW_N, item_scalars=ROW_N + 1, dtype=TDT[dtype], kind="accumulate").bind(
        cuda(np.concatenate([A, b[..., None]], -1)))
    assert_same_solve(ta, model, lambda lo, hi: model.with_bounds(None if lo is None else cuda(lo), None if hi is None else cuda(hi)),
                      x0, ta.Options(), P, ROW_N, dtype)


def ragged_circle(dtype, counts, seed=41):
    rng = np.random.default_rng(seed)
    items = []
    for cnt in counts:
        ang = np.linspace(0, 2 * np.pi, cnt, endpoint=False) + rng.uniform(0, 1)
        items.append((np.stack([2 + 2 * np.cos(ang), 7 + 2 * np.sin(ang)], -1) + 1e-3 * rng.uniform(-1, 1, (cnt, 2))).astype(dtype))
    x0 = (np.array([1.6, 6.7, 1.7]) + 0.2 * rng.uniform(-1, 1, (len(counts), 3))).astype(dtype)
    return Case(items, x0)


def test_never_binding_ragged(ta):
    dtype = np.float64
    case = ragged_circle(dtype, [0, 3, 70, 9])
    res = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype])
    plain = case.ragged(res)
    assert_same_solve(ta, plain, lambda lo, hi: plain.with_bounds(None if lo is None else cuda(lo), None if hi is None else cuda(hi)),
                      case.x0, circle_options(ta), case.P, 3, dtype)


# ---- 3. fixed parameters: the oracle on the reduced problem ----------------------------------------------------------------------------
def test_fixed_parameters_match_the_reduced_problem(ta, oracle):
    """n = 20, m = 65, P = 4, a mask per problem: none fixed, three fixed, the last lane's parameter fixed, all fixed.  The oracle's
    DenseRow residual is r = t + 0.1 sin t - b with t = a . x, so `columns removed, b - A_fix c` IS the problem with x_fix = c only for
    c = 0 (then A_fix c = 0 and t is the free columns' sum exactly): the fixed parameters are held at 0.  (Fixed parameters at other
    values: the seeded dense cases of test_binding_bounds_dense.)  The all-fixed problem is held at its start, whatever that is."""
    P, n, m, dtype = 4, ROW_N, 65, np.float64
    A, b, x0, _ = oracle.synth_dense_row(P, n, m, dtype, seed=83)
    masks = [[], [2, 7, 11], [n - 1], list(range(n))]
    lo, hi = np.full((P, n), -INF), np.full((P, n), INF)
    for p, fx in enumerate(masks):
        if p < 3:
            x0[p, fx] = 0.0
        lo[p, fx] = x0[p, fx]
        hi[p, fx] = x0[p, fx]
    model = _res(ta, manual_body(n), n=n, item_scalars=n + 1, dtype=TDT[dtype], kind="accumulate").bind(cuda(np.concatenate([A, b[..., None]], -1)))
    opts = ta.Options()
    x = cuda(x0.copy())
    out = ta.Optimize(x, bounded(model, lo, hi), opts, history=True)
    torch.cuda.synchronize()
    assert_inside(x, lo, hi)
    g = gpu_dict(out, x)
    for p, fx in enumerate(masks):
        assert np.array_equal(g["x"][p, fx], x0[p, fx]), f"problem {p}: a fixed parameter moved"
        if p == 3:
            assert int(g["stop"][p]) != SOLVER_FAILED and int(g["stop"][p]) >= 0, g["stop"][p]
            continue
        free = [j for j in range(n) if j not in fx]
        r = oracle.dense_row_lm(np.ascontiguousarray(A[p:p + 1][:, :, free]), np.ascontiguousarray(b[p:p + 1]), np.ascontiguousarray(x0[p:p + 1][:, free]),
                                opts.to_pod(), history=True)
        refd = dict(errs=r["errs"], succ=r["succ"], iters=r["iters"], stop=r["stop"], x=r["x"], cost=r["cost"], fails=r["fails"], deltas2=r["deltas2"])
        gp = {k: v[p:p + 1] for k, v in g.items()}
        gp["x"] = g["x"][p:p + 1][:, free]
        st = check_trajectories(gp, refd, dtype, opts.to_pod(), label=f"fixed {fx}")
        assert st["full"] + st["ties"] == 1, st


# ---- 4. binding bounds: whole trajectories against the second reading inside the rules -------------------------------------------------
ROSENBROCK = "r[0] = S(1) - x[0];\nr[1] = p[0] * (x[1] - x[0] * x[0]);"                       # item = [10]
HIMMELBLAU = "r[0] = x[0] * x[0] + x[1] - p[0];\nr[1] = x[0] + x[1] * x[1] - p[1];"           # item = [11, 7]
BEALE = ("r[0] = p[0] - x[0] + x[0] * x[1];\nr[1] = p[1] - x[0] + x[0] * x[1] * x[1];\n"
         "r[2] = p[2] - x[0] + x[0] * x[1] * x[1] * x[1];")                                    # item = [1.5, 2.25, 2.625]


def ext_rosenbrock_body(n):
    """One residual per item; the item's scalars select the pair (one-hot, statically indexed) and which of its two residuals."""
    h = n // 2
    return (f"S a = p[0] * x[0], b = p[0] * x[1];\n#pragma unroll\nfor (int k = 1; k < {h}; ++k) {{ a = a + p[k] * x[2 * k]; b = b + p[k] * x[2 * k + 1]; }}\n"
            f"r[0] = p[{h}] * (S(1) - a) + (T(1) - p[{h}]) * T(10) * (b - a * a);")


def ext_rosenbrock_items(n, dtype):
    h = n // 2
    items = np.zeros((2 * h, h + 1), dtype)
    for k in range(h):
        items[2 * k, k] = items[2 * k + 1, k] = 1
        items[2 * k, h] = 1
    return items


def ext_rosenbrock_fn(n):
    def fn(x, want):
        r, J = [], []
        for k in range(0, n, 2):
            r += [1.0 - x[k], 10.0 * (x[k + 1] - x[k] * x[k])]
            a, c = [0.0] * n, [0.0] * n
            a[k] = -1.0
            c[k], c[k + 1] = -20.0 * x[k], 10.0
            J += [a, c]
        return ref._from_residuals(r, J, want)
    return fn


def both_options(ta, **kw):
    """The same options for the device and for the second reading."""
    o = ta.Options()
    for k, v in kw.items():
        if k == "damping_init":
            o.lm.damping_init = v
        else:
            assert hasattr(o, k), k
            setattr(o, k, v)
    return o, ref.Options(**kw)


# What one problem's device run is held to against its reference trace, by scalar type: costs, |dx|^2, x (relative to max(1, |x|)),
# and how close to the last accepted cost a roll-back's re-evaluation must be on both sides to count as the same point.  fp64 and
# the first three of fp32 are parity.check_against_trace's (the second reading's traces against a device run; fp32: the convention of
# F32_CASES).  The fp32 floor: a roll-back that misses x by one ulp (6e-8 relative) moves the cost by |g| |x| 6e-8, and |g| |x| / cost
# stays below ~300 on these functions' routes: 2e-5.
TRACE_TOL = {np.float64: dict(cost=1e-8, dx2=1e-6, x=1e-8, floor=1e-12), np.float32: dict(cost=2e-3, dx2=2e-2, x=5e-3, floor=2e-5)}


def check_trace(g, r, p, dtype, label):
    """Problem p of a device run (gpu_dict) against its reference output: the rule of parity.check_against_trace.  Pass by pass the same
    accept / reject flag, cost and |dx|^2; no difference to the end => the same StopReason, iteration and failure counts, x and final cost
    ("full").  The one difference that is allowed is the roll-back tie: after a rejected step the loop rolls x back and accumulates again
    at that point, so `err < final_cost` compares two numbers that are equal in exact arithmetic — 0 exactly when (x + dx) - dx restored x
    bit for bit, a last-bit coin toss otherwise, and which of the two depends on the last bits of dx.  It must be PROVEN: the pass before
    was rejected on both sides, both evaluated the same point, and its cost is the last accepted cost to the floor on both sides; the
    comparison of everything before it stands, the routes after it are not comparable ("tie").  (parity.check_trajectories, which the
    dense cases below use, takes a tie for the end of a converged solve and requires every later cost to stay on that floor: these
    functions meet roll-backs in the middle of their routes.)"""
    t = TRACE_TOL[dtype]
    ge, gs, gd = g["errs"][p], g["succ"][p].astype(np.int64), g["deltas2"][p]
    e, fs, d2 = np.asarray(r["errs"]), np.asarray([int(v) for v in r["successes"]], np.int64), np.asarray(r["deltas2"])
    k, kg = len(e), int(g["iters"][p])
    assert (g["stop"][p] < 0) == (r["stop"] < 0), (label, p, "verdict", g["stop"][p], r["stop"])
    scale = np.abs(e).max() if k else 1.0
    kk = min(k, kg, len(ge))
    div = next((i for i in range(kk) if gs[i] != fs[i]), None)
    upto = kk if div is None else div + 1
    assert np.allclose(ge[:upto], e[:upto], rtol=t["cost"], atol=1e-300), (label, p, "cost history", div, ge[:upto], e[:upto])
    assert np.allclose(gd[:upto - (div is not None)], d2[:upto - (div is not None)], rtol=t["dx2"], atol=1e-12 * max(d2.max(), 1e-300) if k else 0), \
        (label, p, "|dx|^2 history", gd[:upto], d2[:upto])
    if div is not None:
        assert div >= 2 and not fs[div - 1] and not gs[div - 1], (label, p, "the runs part where no step was rolled back", div)
        acc = [i for i in range(div) if fs[i] or i == 0][-1]
        assert abs(e[div] - e[acc]) <= t["floor"] * abs(e[acc]) and abs(ge[div] - ge[acc]) <= t["floor"] * abs(ge[acc]), \
            (label, p, "accept / reject flags differ away from a roll-back tie", div, e[div], ge[div], e[acc], ge[acc])
        return "tie"
    assert int(g["stop"][p]) == r["stop"] and kg == r["num_iters"] and int(g["fails"][p]) == r["num_failures"], \
        (label, p, "stop / iters / fails", int(g["stop"][p]), r["stop"], kg, r["num_iters"], int(g["fails"][p]), r["num_failures"])
    xs = np.asarray(r["x"])
    assert np.abs(g["x"][p] - xs).max() <= t["x"] * max(1.0, np.abs(xs).max()), (label, p, "x", g["x"][p], xs)
    assert abs(float(g["cost"][p]) - r["final_cost"]) <= t["cost"] * abs(r["final_cost"]), (label, p, "final cost")
    return "full"


def run_cases(ta, model_of, cases, opts, ropt, dtype, n, need_margin, label, traces=False):
    """cases: [(fn, x0, lo, hi)], one problem each, solved in ONE bounded batch; every reference trace must keep its decisions
    `need_margin` from flipping.  Returns the reference outputs and the active-set logs."""
    P = len(cases)
    x0 = np.array([c[1] for c in cases], dtype)
    lo = np.array([c[2] for c in cases], dtype)
    hi = np.array([c[3] for c in cases], dtype)
    refs, logs = [], []
    for p, (fn, _, _, _) in enumerate(cases):   # (the reference starts from the values the device gets: rounded to its scalar type)
        log = []
        r = br.optimize_bounded(fn, [float(v) for v in x0[p]], ropt, [float(v) for v in lo[p]], [float(v) for v in hi[p]], log)
        assert r["min_margin"] >= need_margin, (label, p, "the reference trace sits too close to a tie", r["min_margin"])
        refs.append(r)
        logs.append(log)
    x = cuda(x0.copy())
    out = ta.Optimize(x, model_of(P).with_bounds(cuda(lo), cuda(hi)), opts, history=True)
    torch.cuda.synchronize()
    assert_inside(x, lo, hi, label)
    hs = out.errs.shape[1]

    def pad(v, fill=0.0):
        a = np.full(hs, fill)
        a[:min(len(v), hs)] = v[:hs]
        return a
    refd = dict(errs=np.array([pad(r["errs"]) for r in refs]), succ=np.array([pad([int(s) for s in r["successes"]]) for r in refs]),
                iters=np.array([r["num_iters"] for r in refs]), stop=np.array([r["stop"] for r in refs]), x=np.array([r["x"] for r in refs]),
                cost=np.array([r["final_cost"] for r in refs]), fails=np.array([r["num_failures"] for r in refs]),
                deltas2=np.array([pad(r["deltas2"]) for r in refs]))
    if traces:
        g = gpu_dict(out, x)
        verdicts = [check_trace(g, refs[p], p, dtype, label) for p in range(P)]
        print(label, verdicts, "stops", refd["stop"].tolist(), "iterations", refd["iters"].tolist(), "device iterations", g["iters"].tolist())
    else:
        st = check_trajectories(gpu_dict(out, x), refd, dtype, opts.to_pod(), label=label)
        print(label, st, "stops", refd["stop"].tolist(), "iterations", refd["iters"].tolist())
        assert st["full"] + st["ties"] == P, st
    return refs, logs, x.cpu().numpy(), lo, hi


def coverage(refs, logs, x0s, los, his):
    rejected = any(not s for r in refs for s in r["successes"][1:])
    # a parameter that is active (not fixed) at one Build and free at a later one
    leaves = any(any(a[j] and not b[j] for a, b in zip(log, log[1:]) for j in range(len(a)) if lo[j] != hi[j])
                 for log, lo, hi in zip(logs, los, his))
    outside = any(any(v < a or v > b for v, a, b in zip(x0, lo, hi)) for x0, lo, hi in zip(x0s, los, his))
    return rejected, leaves, outside


def test_binding_bounds_test_functions(ta):
    """Rosenbrock (as residuals) with hi_x = 0.8 and inside [-2, 0.5] x [-2, 0.2], Himmelblau with hi_x = 2.5, Beale with x in [3.2, 5]:
    fp64, one batch per function and iteration budget.  The starts are those of a seeded scan whose reference traces keep every
    decision 1e-6 from flipping (run_cases asserts it): a roll-back that misses x by a last bit puts the next decision on a tie, which
    most long traces of these functions meet near their end, hence the budgets of 15 and 8 iterations beside the full ones.  Over the
    set: rejected steps, parameters that leave their bound, starts outside the box."""
    dtype = np.float64
    RB = dict(min_rerr_dec=0.0, max_consec_failures=30)
    HB = dict(max_consec_failures=30, min_error=1e-30)
    BL = dict(max_consec_failures=30, min_error=1e-30, damping_init=1e-3)
    sets = [
        ("rosenbrock hi_x = 0.8", ROSENBROCK, 2, [10.0], br.rosenbrock_res, RB, [-INF, -INF], [0.8, INF],
         [(200, [[0.3, 1.16], [-0.81, -1.31], [0.2, 0.91], [-0.72, -0.55]])]),
        ("rosenbrock box", ROSENBROCK, 2, [10.0], br.rosenbrock_res, RB, [-2.0, -2.0], [0.5, 0.2],
         [(15, [[-0.13, -0.42]]), (8, [[-2.08, 1.19], [-1.38, 0.18], [-1.95, 1.27]])]),
        ("himmelblau hi_x = 2.5", HIMMELBLAU, 2, [11.0, 7.0], ref.himmelblau, HB, [-INF, -INF], [2.5, INF],
         [(15, [[0.15, 3.16], [0.75, 0.61], [0.36, 2.55]]), (8, [[3.06, 0.69], [3.77, 0.73]])]),
        ("beale x in [3.2, 5]", BEALE, 3, [1.5, 2.25, 2.625], ref.beale, BL, [3.2, -INF], [5.0, INF],
         [(15, [[5.81, 1.14], [4.89, 1.14], [3.29, -0.04]])]),
    ]
    all_refs, all_logs, x0s, los, his = [], [], [], [], []
    for name, body, kR, item, fn, kw, lo, hi, groups in sets:
        res = _res(ta, body, n=2, item_scalars=len(item), residuals_per_item=kR, dtype=TDT[dtype])
        for max_iters, starts in groups:
            opts, ropt = both_options(ta, max_iters=max_iters, **kw)
            cases = [(fn, x0, lo, hi) for x0 in starts]
            refs, logs, _, _, _ = run_cases(ta, lambda P, res=res, item=item: res.bind(cuda(np.tile(np.array(item, dtype), (P, 1, 1)))), cases, opts, ropt,
                                            dtype, 2, 1e-6, f"{name}, {max_iters} iterations", traces=True)
            all_refs += refs
            all_logs += logs
            x0s += starts
            los += [lo] * len(starts)
            his += [hi] * len(starts)
    rejected, leaves, outside = coverage(all_refs, all_logs, x0s, los, his)
    assert rejected and leaves and outside, (rejected, leaves, outside)


@pytest.mark.parametrize("n", [4, 12])
def test_binding_bounds_extended_rosenbrock_fp32(ta, n):
    """Extended Rosenbrock in fp32, one residual per item, one-hot item scalars selecting the pair (statically indexed): n = 4 is a
    JetModel (a run-time model of four fp32 parameters is never a RowModel: the staged rows start at eleven), n = 12 a RowModel —
    staged rows, rejected steps, the memo.  Short traces whose decisions stay 1e-3 from flipping: the convention of F32_CASES."""
    dtype = np.float32
    opts, ropt = both_options(ta, max_iters=8, min_rerr_dec=0.0, max_consec_failures=20)
    res = _res(ta, ext_rosenbrock_body(n), n=n, item_scalars=n // 2 + 1, dtype=TDT[dtype])
    fn = ext_rosenbrock_fn(n)
    h = n // 2
    cases = [(fn, [-1.2, 1.0] * h, [-INF] * n, [0.8, INF] * h),
             (fn, [-1.2, 1.0] * h, [-2.0] * n, [0.5, 0.2] * h),
             (fn, [-0.9, 1.3] * h, [-INF] * n, ([0.8, INF] + [INF, INF]) * (h // 2)),
             (fn, [-2.08, 1.19] * h, [-2.0] * n, [0.5, 0.2] * h)]
    items = ext_rosenbrock_items(n, dtype)
    refs, logs, _, _, _ = run_cases(ta, lambda P: res.bind(cuda(np.tile(items, (P, 1, 1)))), cases, opts, ropt, dtype, n, 1e-3, f"ext rosenbrock n={n}",
                                    traces=True)
    assert any(not s for r in refs for s in r["successes"][1:]), "no rejected step in the set"


def linear_body(n):
    return f"S t = x[0] * p[0];\n#pragma unroll\nfor (int j = 1; j < {n}; ++j) t = t + x[j] * p[j];\nr[0] = t - p[{n}];"


@pytest.mark.parametrize("n,m", [(4, 9), (8, 12)])
def test_binding_bounds_dense(ta, n, m):
    """Seeded dense linear problems in fp64 (n = 4: JetModel; n = 8: RowModel), the first 8 seeds whose reference trace keeps every
    decision 1e-6 from flipping, one batch: trajectories against the reference, and every one ends on a bound."""
    dtype = np.float64
    opts, ropt = both_options(ta, max_iters=100, max_consec_failures=30)
    picked = []
    for seed in range(200):
        A, b, x0, lo, hi = br.dense_case(seed, n, m)
        out = br.optimize_bounded(br.dense_fn(A, b), list(x0), ropt, list(lo), list(hi))
        if out["min_margin"] >= 1e-6 and out["stop"] >= 0:
            picked.append((A, b, x0, lo, hi))
        if len(picked) == 8:
            break
    assert len(picked) == 8, len(picked)
    res = _res(ta, linear_body(n), n=n, item_scalars=n + 1, dtype=TDT[dtype])
    data = np.stack([np.concatenate([A, b[:, None]], -1) for A, b, _, _, _ in picked])
    cases = [(br.dense_fn(A, b), list(x0), list(lo), list(hi)) for A, b, x0, lo, hi in picked]
    refs, _, x, lo, hi = run_cases(ta, lambda P: res.bind(cuda(data)), cases, opts, ropt, dtype, n, 1e-6, f"dense n={n} m={m}")
    assert all(np.any((x[p] == lo[p]) | (x[p] == hi[p])) for p in range(8))


# ---- 6. ragged -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prior", [False, True])
def test_ragged_is_bit_equal_to_uniform(ta, with_prior):
    """Counts [0, 3, 70, 9] with bounds that bind (the radius below 1.8, a centre coordinate fixed, a start outside the box): every
    problem is its uniform bounded solve bit for bit; the empty problem is kSkipped (its x the clipped start) without a prior and an
    ordinary problem with one."""
    dtype, n = np.float64, 3
    case = ragged_circle(dtype, [0, 3, 70, 9])
    res = _res(ta, CIRCLE, n=n, item_scalars=2, dtype=TDT[dtype])
    lo, hi = np.full((case.P, n), -INF), np.full((case.P, n), INF)
    hi[:, 2] = 1.8
    lo[2, 0] = hi[2, 0] = case.x0[2, 0]
    lo[0, 1] = 7.5          # (the empty problem starts below it)
    lo[3, 0] = 2.2
    rng = np.random.default_rng(43)
    mu, W = make_prior(rng, case.P, n, "diag", dtype, np.tile(np.array([2.0, 7.0, 2.0]), (case.P, 1)), spread=0.2, scale=1.0)
    opts = circle_options(ta)
    opts.max_consec_failures = 30

    def dress(model, sl):
        if with_prior:
            model = model.with_prior(cuda(mu[sl]), cuda(W[sl]))
        return model.with_bounds(cuda(lo[sl]), cuda(hi[sl]))
    x = case.x()
    out = ta.Optimize(x, dress(case.ragged(res), slice(None)), opts, history=True)
    torch.cuda.synchronize()
    assert_inside(x, lo, hi)
    x0c = np.minimum(np.maximum(case.x0, lo), hi)
    for p, cnt in enumerate(case.counts):
        if cnt == 0 and not with_prior:
            assert int(out.stop_reason[p]) == SKIPPED and int(out.final_num_residuals[p]) == 0
            assert np.array_equal(x[p].cpu().numpy(), x0c[p]), "the empty problem's x is not its clipped start"
            continue
        if cnt == 0:   # an ordinary problem of n residuals: its uniform twin has no items to bind, so it is checked by itself
            assert int(out.stop_reason[p]) >= 0 and int(out.stop_reason[p]) != SKIPPED and int(out.final_num_residuals[p]) == n
            continue
        x1 = case.x(p)
        o1 = ta.Optimize(x1, dress(case.alone(res, p), slice(p, p + 1)), opts, history=True)
        torch.cuda.synchronize()
        assert torch.equal(x[p], x1[0]), f"problem {p} ({cnt} items): x differs by {float((x[p] - x1[0]).abs().max())}"
        for f in OUT_FIELDS:
            a, b = getattr(out, f), getattr(o1, f)
            if a is None and b is None:
                continue
            assert torch.equal(a[p], b[0]), f"problem {p} ({cnt} items): {f} differs: {a[p]} vs {b[0]}"
    assert float(x[2, 0]) == case.x0[2, 0] and bool((x[1:, 2] <= 1.8).all())


def test_covariance_of_a_bounded_solve(ta):
    """final_hessian is the projected matrix of the last Build: Covariance() is the inverse of the free block and 1 on the active diagonal."""
    dtype, n = np.float64, 3
    pts, x0 = circle_uniform(dtype, P=2)
    lo, hi = np.full((2, n), -INF), np.full((2, n), INF)
    lo[0, 2] = hi[0, 2] = 1.5
    model = _res(ta, CIRCLE, n=n, item_scalars=2, dtype=TDT[dtype]).bind(cuda(pts))
    x = cuda(x0.copy())
    out = ta.Optimize(x, bounded(model, lo, hi), circle_options(ta))
    torch.cuda.synchronize()
    H = out.final_hessian.cpu().numpy().reshape(2, n, n)
    assert np.array_equal(H[0][2], [0, 0, 1]) and np.array_equal(H[0][:, 2], [0, 0, 1])
    C, ok = out.Covariance()
    Cn = C.cpu().numpy().reshape(2, n, n)
    assert bool(ok.all()) and abs(Cn[0][2, 2] - 1.0) < 1e-15 and np.abs(Cn[0][:2, 2]).max() == 0
    assert np.allclose(Cn[0][:2, :2], np.linalg.inv(H[0][:2, :2]), rtol=1e-9)
    assert np.allclose(Cn[1], np.linalg.inv(H[1]), rtol=1e-9)


def test_numeric_model_with_bounds(ta):
    """diff="central" wraps the same templates, so a numerically differentiated model inherits the wrapper as it inherits the prior's:
    the circle fit with the radius held below 1.8 and a centre coordinate fixed, beside its AD twin.  Bound as in
    tests/test_gpu_num_diff.py::test_solve_with_central_differences: every problem ends regularly and the two land within 5e-3."""
    dtype, n = np.float64, 3
    pts, x0 = circle_uniform(dtype, P=5, items=40)
    lo, hi = np.full((5, n), -INF), np.full((5, n), INF)
    hi[:, 2] = 1.8
    lo[1, 0] = hi[1, 0] = x0[1, 0]
    opts = circle_options(ta)
    opts.max_consec_failures = 30
    xs = {}
    for diff in ("central", "ad"):
        model = bounded(_res(ta, CIRCLE, n=n, item_scalars=2, dtype=TDT[dtype], diff=diff).bind(cuda(pts)), lo, hi)
        x = cuda(x0.copy())
        out = ta.Optimize(x, model, opts)
        torch.cuda.synchronize()
        assert bool((out.stop_reason >= 0).all()), out.stop_reason
        assert_inside(x, lo, hi, diff)
        xs[diff] = x.cpu().numpy()
        assert np.array_equal(xs[diff][:, 2], np.full(5, 1.8)) and xs[diff][1, 0] == x0[1, 0]
    err = np.abs(xs["central"] - xs["ad"]).max()
    print(f"numeric vs AD inside a box: max |x_num - x_ad| {err:.3e}")
    assert err < 5e-3


# ---- 7. what a bounded model does not do -----------------------------------------------------------------------------------------------
def test_refusals(ta):
    dtype = np.float64
    pts, x0 = circle_uniform(dtype)
    P = len(x0)
    res = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=TDT[dtype])
    plain = res.bind(cuda(pts))
    model = plain.with_bounds(None, None)
    ragged = res.bind_ragged(cuda(pts.reshape(-1, 2)), counts=[10] * P).with_bounds(None, None)
    x = cuda(x0)
    before = x.clone()
    for m in (model, ragged):
        with pytest.raises(ValueError, match="splits"):
            ta.Optimize(x, m, circle_options(ta), splits=2)
        o = circle_options(ta)
        o.stop_callback = lambda err, dx2, g2: False
        with pytest.raises(ValueError, match="host controls"):
            ta.Optimize(x, m, o)
        with pytest.raises(ValueError, match="stepping"):
            ta.Optimizer(x, m, circle_options(ta))
        with pytest.raises(ValueError, match="with_bounds.*CheckGradient"):
            ta.CheckGradient(m, x)
        with pytest.raises(ValueError, match="with_bounds.*Eval"):
            ta.Eval(m, x)
        with pytest.raises(ValueError, match="with_bounds.*CalculateJac"):
            ta.CalculateJac(m, x)
        g = circle_options(ta)
        g.solver_type = ta.Options.GradientDescent
        with pytest.raises(ValueError, match="GradientDescent"):
            ta.Optimize(x, m, g)
    # shape, dtype, device, order
    f64 = dict(dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match=r"lo must be \[P, n\]"):
        plain.with_bounds(torch.zeros(P, 2, **f64), None)
    with pytest.raises(ValueError, match="dtype"):
        plain.with_bounds(None, torch.zeros(P, 3, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="device"):
        plain.with_bounds(torch.zeros(P, 3, dtype=torch.float64), None)
    with pytest.raises(ValueError, match="lo <= hi"):
        plain.with_bounds(torch.ones(P, 3, **f64), torch.zeros(P, 3, **f64))
    with pytest.raises(ValueError, match="lo <= hi"):
        plain.with_bounds(torch.full((P, 3), float("nan"), **f64), None)
    # manifolds, cost kinds and large-n models: refused where the bounds are attached
    with pytest.raises(ValueError, match="manifold='se3'"):
        types_of(ta, "se3").with_bounds(None, None)
    with pytest.raises(ValueError, match="manifold='user'"):
        types_of(ta, "user").with_bounds(None, None)
    for kind in ("cost", "cost_grad"):
        with pytest.raises(ValueError, match="scalar cost"):
            types_of(ta, kind).with_bounds(None, None)
    large = _res(ta, "r[0] = x[0] - p[0];", n=1, item_scalars=1, dtype=torch.float64, large_n=True).bind(torch.zeros(1, 2, 1, **f64))
    with pytest.raises(ValueError, match="large_n"):
        large.with_bounds(None, None)
    # the library itself, with code and text, before anything is built or launched
    from tinyopt_amd import _capi
    C = _capi.C
    ctx = res.ctx
    lib = ctx.lib
    lo_t, hi_t = torch.full((P, 3), -INF, **f64), torch.full((P, 3), INF, **f64)
    c = torch.zeros(P, dtype=torch.float64, device="cuda")

    def acc(handle, bd, items=10, data=plain.packed):
        return lib.toa_jit_accumulate_bounds(ctx.h, handle, items, P, data.data_ptr(), x.data_ptr(), bd, None, 0, None, None, c.data_ptr(), None)
    bd = _capi.ToaBounds()
    bd.lo_dev, bd.hi_dev = lo_t.data_ptr(), hi_t.data_ptr()
    assert acc(res._h, None) == -1 and b"null bounds" in lib.toa_last_error()
    half = _capi.ToaBounds()
    half.lo_dev = lo_t.data_ptr()
    assert acc(res._h, C.byref(half)) == -1 and b"null bounds lo_dev / hi_dev" in lib.toa_last_error()
    pod, rs = circle_options(ta).to_pod(), _capi.ToaResults()
    assert lib.toa_jit_lm_run_bounds(ctx.h, res._h, 10, P, plain.packed.data_ptr(), x.data_ptr(), None, None, C.byref(pod), C.byref(rs), None) == -1
    assert b"toa_jit_lm_run_bounds: null bounds" in lib.toa_last_error()
    for what, text in (("se3", b"box on the tangent"), ("user", b"box on the tangent"), ("cost", b"scalar cost model"), ("cost_grad", b"scalar cost model")):
        m = types_of(ta, what)
        assert acc(m.res._h, C.byref(bd), items=m.items, data=m.packed) == -4 and text in lib.toa_last_error(), (what, lib.toa_last_error())
    assert acc(large.res._h, C.byref(bd), items=2, data=large.packed) == -4 and b"box bounds (toa_jit_*_bounds) are not built for it" in lib.toa_last_error()
    v = [C.c_int(0) for _ in range(3)]
    assert lib.toa_jit_model_stats_bounds(ctx.h, large.res._h, 0, 0, *[C.byref(t) for t in v]) == -4
    torch.cuda.synchronize()
    assert torch.equal(x, before) and float(c.abs().max()) == 0, "a refused call launched something"


def test_first_use_is_refused_under_capture(ta):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res = ta.JitResidual("r[0] = x[0] * x[0] - p[0];  // capture test of the bounds kernels: a text of its own", n=1, item_scalars=1, dtype=torch.float64)
        model = res.bind(torch.full((3, 2, 1), 2.0, dtype=torch.float64, device="cuda"))
        bm = model.with_bounds(None, torch.full((3, 1), 1.25, dtype=torch.float64, device="cuda"))
        x = torch.full((3, 1), 1.5, dtype=torch.float64, device="cuda")
        ta.accumulate(model, x)   # (warms the context of this stream)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(Exception, match="bounds kernels of this model are compiled on their first use .* cannot happen while the stream is being captured"):
            with torch.cuda.graph(g, stream=s):
                ta.Optimize(x, bm, ta.Options())
    torch.cuda.synchronize()
    assert bool((x == 1.5).all())   # nothing was recorded, nothing ran
    with torch.cuda.stream(s):
        ta.Optimize(x, bm, ta.Options())
        s.synchronize()
        assert bool((x == 1.25).all())   # sqrt(2) is outside: the solve ends on the bound


def test_bounds_kernels_report_their_registers(ta):
    circle = _res(ta, CIRCLE, n=3, item_scalars=2, dtype=torch.float64)
    row = _res(ta, manual_body(ROW_N), n=ROW_N, item_scalars=ROW_N + 1, dtype=torch.float64, kind="accumulate")
    for res in (circle, row):
        for ragged, prior in ((False, False), (True, True)):
            s = res.stats_bounds(ragged=ragged, with_prior=prior)
            print("stats_bounds", res.n, "ragged" if ragged else "uniform", "prior" if prior else "no prior", s)
            assert s["num_regs"] > 0 and s["wg_per_cu"] >= 1
