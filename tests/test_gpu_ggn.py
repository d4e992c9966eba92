"""Rank-one second-order scalar costs on the device (kind="cost_ggn"): run-time bodies that assign c, gs, hs and J,
summed as g = sum gs J and H = sum w J J^T on the matrix-core Gram of the row models and run by LM / GN through
lm_fused_kernel<RowModel<GgnRowFunctor>>.  Yardstick: tests/ggn_reference.py — the kind's callbacks in numpy inside the committed
second reading of the loop.  Every test here needs the kind, so every one of them fails on a library that does not know it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ggn_reference as gr  # noqa: E402
import hess_reference as hr  # noqa: E402
from ggn_cells import CELLS, P_TRAJ, trajectory_cases  # noqa: E402
from parity import check_trajectories, first_divergence, gpu_dict  # noqa: E402

pytestmark = pytest.mark.gpu
TDT = {np.float32: torch.float32, np.float64: torch.float64}
EPS = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}   # the unit round-off
P = 97
_MODELS = {}


def model_of(ta, key, body, n, kD, dtype, kind="cost_ggn"):
    """One compiled model per (key, dtype) for the whole module."""
    k = (key, dtype)
    if k not in _MODELS:
        _MODELS[k] = ta.JitResidual(body, n=n, item_scalars=kD, kind=kind, dtype=TDT[dtype])
    return _MODELS[k]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ref_dict(refs, hs):
    def pad(v):
        a = np.zeros(hs)
        a[:min(len(v), hs)] = v[:hs]
        return a
    return dict(errs=np.array([pad(r["errs"]) for r in refs]), succ=np.array([pad([int(s) for s in r["successes"]]) for r in refs]),
                iters=np.array([r["num_iters"] for r in refs]), stop=np.array([r["stop"] for r in refs]), x=np.array([r["x"] for r in refs]),
                cost=np.array([r["final_cost"] for r in refs]), fails=np.array([r["num_failures"] for r in refs]),
                deltas2=np.array([pad(r["deltas2"]) for r in refs]))


# ---- 1. the sum, exactly -----------------------------------------------------------------------------------------------------------
LAYOUT_EDGES = [1, 2, 12, 13, 15, 16, 19, 20, 31, 32, 35, 36, 47, 48, 50, 51, 52, 63]   # every edge of DenseRowLayout::make, and 50


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", LAYOUT_EDGES)
def test_the_sum_exactly(ta, n, dtype):
    """Dyadic gs and J, hs a power of four (or zero, or negative: then H gets wmin J J^T alone), magnitudes at which every product and
    every partial sum is exact in float32 (ggn_reference.exact_case): accumulate's cost, g and H EQUAL numpy's, at every layout edge of
    n and at every edge of the super-step (IT of the accumulate pass and of the cost-only pass, from the geometry)."""
    res = model_of(ta, f"table{n}", gr.table_body(n), n, n + 3, dtype)
    its = gr.row_stage_items(n, n + 3, dtype)
    counts = sorted({1, 63, 64, 65} | {c for it in its for c in (it - 1, it, it + 1, 3 * it + 5) if c >= 1})
    x = cuda(np.zeros((P, n), dtype))
    for items in counts:
        d = gr.exact_case(n, items, P)
        c32, g32, H32 = gr.exact_sums(d, np.float32)
        c64, g64, H64 = gr.exact_sums(d, np.float64, np.float32)
        assert (c32 == c64).all() and (g32 == g64).all() and (H32 == H64).all(), "the case is not exact in float32"
        c64, g64, H64 = gr.exact_sums(d, np.float64, dtype)   # (the clamped problems' H is wmin J J^T with the dtype's own wmin)
        model = res.bind(cuda(d.astype(dtype)))
        g, H, c, nres = ta.accumulate(model, x)
        assert (c.cpu().numpy() == c64).all(), (n, items, "cost")
        assert (g.cpu().numpy() == g64.astype(dtype)).all(), (n, items, "g")
        assert (H.cpu().numpy() == H64.astype(dtype)).all(), (n, items, "H")
        assert (nres.cpu().numpy() == 1).all()
        g0, H0, c0, _ = ta.accumulate(model, x, want_grad=False)
        assert g0 is None and H0 is None and (c0.cpu().numpy() == c64).all(), (n, items, "cost only")
        # (problems 1, 4, ... have hs = 0 and 2, 5, ... hs < 0: their gradient is there, their H is wmin J J^T)
        wmin = gr.WMIN[np.dtype(dtype)]
        JJ = np.einsum("pia,pib->pab", d[1::3, :, :n], d[1::3, :, :n])
        assert (H.cpu().numpy()[1::3] == (wmin * JJ).astype(dtype)).all() and np.abs(g64[1::3]).max() > 0


# ---- 2. the sum, rounded -----------------------------------------------------------------------------------------------------------
ROUNDED = {   # name: (parts, body, n, items, case(seed))
    "logistic12": (gr.logistic_parts, gr.logistic_body(12), 12, 200, lambda s: gr.logistic_case(s, 12, 200)),
    "logistic50": (gr.logistic_parts, gr.logistic_body(50), 50, 200, lambda s: gr.logistic_case(s, 50, 200)),
    "poisson13": (gr.poisson_parts, gr.poisson_body(13), 13, 157, lambda s: gr.poisson_case(s, 13, 157)),
    "spot": (gr.spot_parts, gr.SPOT_BODY, 4, 49, gr.spot_case),
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(ROUNDED))
def test_the_sum_rounded(ta, name, dtype):
    """Logistic and Poisson bodies on random data against the fp64 restatement, entry by entry: with B = eps (items + 6) sum_i |term_i|
    (eps the unit round-off: one rounding each for the root, the two scalings and the product, plus the accumulation in any order) a
    device value lies within 2 B (the factor 2: the library exp / log that feed gs and hs).  The cost: within items eps_machine
    sum |c_i|, the rule of test_gpu_hess.py's fp32 sums."""
    parts, body, n, items, case = ROUNDED[name]
    cases = [case(seed) for seed in range(P)]
    data = np.array([c[0] for c in cases]).astype(dtype)
    x0 = np.array([c[1] for c in cases]).astype(dtype)
    res = model_of(ta, name, body, n, data.shape[2], dtype)
    g, H, c, nres = ta.accumulate(res.bind(cuda(data)), cuda(x0))
    g, H, c = g.cpu().numpy().astype(np.float64), H.cpu().numpy().astype(np.float64), c.cpu().numpy()
    eps, worst = EPS[dtype], dict(g=0.0, H=0.0, c=0.0)
    for p in range(P):
        ci, gs, hs, J = parts(x0[p].astype(np.float64), data[p].astype(np.float64), True)
        w = np.where(hs <= gr.WMIN[np.dtype(dtype)], gr.WMIN[np.dtype(dtype)], hs)
        tg, tH = gs[:, None] * J, w[:, None, None] * J[:, :, None] * J[:, None, :]
        Bg, BH = eps * (items + 6) * np.abs(tg).sum(axis=0), eps * (items + 6) * np.abs(tH).sum(axis=0)
        Bc = items * 2.0 * eps * np.abs(ci).sum()
        worst["g"] = max(worst["g"], float((np.abs(g[p] - tg.sum(axis=0)) / Bg).max()))
        worst["H"] = max(worst["H"], float((np.abs(H[p] - tH.sum(axis=0)) / BH).max()))
        worst["c"] = max(worst["c"], float(abs(c[p] - ci.sum()) / Bc))
    print(name, np.dtype(dtype).name, "worst ratio to B: g %.3f H %.3f, cost to its bound %.4f" % (worst["g"], worst["H"], worst["c"]))
    assert worst["g"] <= 2.0 and worst["H"] <= 2.0 and worst["c"] <= 1.0, worst
    assert (nres.cpu().numpy() == 1).all()


# ---- 3. trajectories ---------------------------------------------------------------------------------------------------------------
BODIES = {"logistic12": gr.logistic_body(12), "logistic13": gr.logistic_body(13), "logistic50": gr.logistic_body(50),
          "logistic63": gr.logistic_body(63), "spot": gr.SPOT_BODY}


def _check_problem(got, ref, p, pod, label):
    """Problem p through parity.check_trajectories: "full", or "tie" (parted at the round-off floor of a converged solve).  A run that
    rejects a step meets one more coin toss, in the MIDDLE of its route: the loop rolls x back by x + dx - dx, evaluates there again,
    and `err < final_cost` compares two numbers that are equal in exact arithmetic; the routes after that are not comparable —
    check_trajectories, written for the end of a solve, reports such a run as having left the floor.  Then the rule of
    test_gpu_hess.py applies ("roll-back tie"): everything before the parting agrees, the pass before it was rejected on both sides,
    both evaluated the same point, and its cost is the last accepted cost to 1e-9; and both runs still end without a failure."""
    one = lambda d: {k: v[p:p + 1] for k, v in d.items() if v is not None}   # noqa: E731
    try:
        st = check_trajectories(one(got), one(ref), np.float64, pod, label=label)
        return "tie" if st["ties"] else "full"
    except AssertionError as e:
        why = e
    ge, gs, re_, rs = got["errs"][p], got["succ"][p], ref["errs"][p], ref["succ"][p]
    gk, rk = int(got["iters"][p]), int(ref["iters"][p])
    k = first_divergence(ge, gs, gk, re_, rs, rk, rtol=1e-9, atol=0.0)
    if k is None or k < 2 or gs[k - 1] or rs[k - 1] or k >= min(gk, rk):
        raise why   # the runs do not part right after a rolled-back step: check_trajectories' verdict stands
    acc = [i for i in range(k) if gs[i] or i == 0][-1]
    assert np.isclose(ge[k], re_[k], rtol=1e-9, atol=0.0), (label, p, k, "different point", ge[k], re_[k])
    assert abs(ge[k] - ge[acc]) <= 1e-9 * abs(ge[acc]) and abs(re_[k] - re_[acc]) <= 1e-9 * abs(re_[acc]), (label, p, k, ge[k], re_[k], ge[acc])
    assert got["stop"][p] >= 0 and ref["stop"][p] >= 0, (label, p, got["stop"][p], ref["stop"][p])
    return "roll-back tie"


@pytest.mark.parametrize("problem,optname", CELLS)
def test_trajectories(ta, problem, optname):
    """Logistic regression at n = 12, 13, 50, 63 (200 items) and the Poisson spot fit (n = 4, the deviance as the cost) in fp64 against
    the second reading under parity.check_trajectories; the seeds are ggn_cells.py's (no decision of the yardstick closer than 1e-9 to
    flipping, the re-evaluation of a rolled-back point exempt; at least two problems per cell take rejected steps — the roll-back's
    coverage, and the re-accumulation's, since this model keeps no memo).  Left out: ggn_cells.LEFT_OUT, two cells of twenty-five."""
    cases, refs, o_kw = trajectory_cases(problem, optname)
    o, _ = gr.options_pair(ta.Options, **o_kw)
    n = len(cases[0][1])
    res = model_of(ta, problem, BODIES[problem], n, cases[0][0].shape[1], np.float64)
    x = cuda(np.array([c[1] for c in cases]))
    out = ta.Optimize(x, res.bind(cuda(np.array([c[0] for c in cases]))), o, history=True)
    torch.cuda.synchronize()
    got, ref = gpu_dict(out, x), ref_dict(refs, out.errs.shape[1])
    verdicts = [_check_problem(got, ref, p, o.to_pod(), f"{problem} {optname}") for p in range(len(cases))]
    print(problem, optname, {v: verdicts.count(v) for v in sorted(set(verdicts))}, "stops", [r["stop"] for r in refs], "device", got["stop"].tolist(),
          "iterations", [r["num_iters"] for r in refs], "failures", [r["num_failures"] for r in refs])
    # every problem is identical to the end or parted at a PROVEN tie (_check_problem raises otherwise); a run without a rejected step
    # has no roll-back to part at
    assert set(verdicts) <= {"full", "tie", "roll-back tie"}
    assert all(v != "roll-back tie" for v, r in zip(verdicts, refs) if all(r["successes"]))
    assert sum(1 for r in refs if not all(r["successes"])) >= 2, "the cell's coverage of rejected steps"
    assert (out.final_num_residuals.cpu().numpy() == 1).all() and (out.final_inlier_ratio.cpu().numpy() == 1).all()
    if set(verdicts) == {"full"} and out.final_hessian is not None:   # (Options.benchmark() exports none)
        Hr = np.array([r["final_hessian"] for r in refs])
        assert np.allclose(out.final_hessian.cpu().numpy(), Hr, rtol=1e-6, atol=1e-9 * np.abs(Hr).max())


@pytest.mark.parametrize("problem", ["logistic12", "logistic50", "spot"])
def test_fp32_trajectories_end_at_the_minimum(ta, problem):
    """fp32 under Options(): a success, and the final cost — recomputed in fp64 numpy at the device's final x — within
    items * 2^-23 * sum |c_i| of the fp64 yardstick's final cost: the worst-case rounding of the sum (test_gpu_hess.py's rule)."""
    parts = gr.spot_parts if problem == "spot" else gr.logistic_parts
    case = gr.spot_case if problem == "spot" else (lambda s: gr.logistic_case(s, int(problem[8:]), 200))
    o, ropt = gr.options_pair(ta.Options)
    cases = [case(seed) for seed in range(P_TRAJ)]
    cases = [(d.astype(np.float32).astype(np.float64), x0.astype(np.float32).astype(np.float64)) for d, x0 in cases]
    refs = [gr.optimize(parts, d, x0, ropt) for d, x0 in cases]
    res = model_of(ta, problem, BODIES[problem], len(cases[0][1]), cases[0][0].shape[1], np.float32)
    x = cuda(np.array([c[1] for c in cases], np.float32))
    out = ta.Optimize(x, res.bind(cuda(np.array([c[0] for c in cases], np.float32))), o)
    torch.cuda.synchronize()
    xs, stop = x.cpu().numpy().astype(np.float64), out.stop_reason.cpu().numpy()
    for p, ((d, _), r) in enumerate(zip(cases, refs)):
        ci = parts(xs[p], d, False)[0]
        bound = len(d) * 2.0 ** -23 * np.abs(ci).sum()
        print(problem, p, "stop", stop[p], "cost at the device's x", ci.sum(), "yardstick", r["final_cost"], "bound", bound)
        assert stop[p] >= 0, (problem, p, stop[p])
        assert abs(ci.sum() - r["final_cost"]) <= bound, (problem, p, ci.sum(), r["final_cost"], bound)


# ---- 4. against the sibling --------------------------------------------------------------------------------------------------------
def test_against_cost_hess(ta):
    """At n = 12 the same logistic batch through kind="cost_hess" (hess_reference.logistic_body: the full outer product in a register
    triangle) and through kind="cost_ggn": per problem the same StopReason, iteration count and accept flags, and final costs within
    the cost bound of test_the_sum_rounded.  A problem may part only at a decision the restatement took within 2 B of flipping; such
    partings are counted against a cap of 5 % of the 97 (checked for the restatement alone in test_cpu_ggn_reference.py)."""
    n, items = 12, 200
    cases = [gr.logistic_case(seed, n, items) for seed in range(P)]
    data, x0 = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    o, ropt = gr.options_pair(ta.Options, min_rerr_dec=1e-6)   # (under the default 1e-10 a solve takes its last decision on the round-off floor)
    outs = {}
    for kind, body in (("cost_hess", hr.logistic_body(n)), ("cost_ggn", gr.logistic_body(n))):
        res = model_of(ta, "sibling " + kind, body, n, n + 1, np.float64, kind=kind)
        x = cuda(x0.copy())
        outs[kind] = (ta.Optimize(x, res.bind(cuda(data)), o, history=True), x)
    torch.cuda.synchronize()
    (oh, xh), (og, xg) = outs["cost_hess"], outs["cost_ggn"]
    parted = 0
    for p in range(P):
        same = (int(oh.stop_reason[p]) == int(og.stop_reason[p]) and int(oh.num_iters[p]) == int(og.num_iters[p]) and
                torch.equal(oh.successes[p], og.successes[p]))
        if same:
            ci = gr.logistic_parts(xg[p].cpu().numpy(), data[p], False)[0]
            assert abs(float(oh.final_cost[p]) - float(og.final_cost[p])) <= 2 * items * 2.0 ** -52 * np.abs(ci).sum(), p
            continue
        r = gr.optimize(gr.logistic_parts, data[p], x0[p], ropt)
        B = 2.0 ** -53 * (items + 6) * np.abs(gr.logistic_parts(np.array(r["x"]), data[p], False)[0]).sum() / max(r["final_cost"], 1e-300)
        assert r["min_margin"] <= 2 * B, (p, "parted away from a tie", r["min_margin"], B)
        parted += 1
    print("against cost_hess: parted", parted, "of", P)
    assert parted <= 0.05 * P


# ---- 5. further --------------------------------------------------------------------------------------------------------------------
def test_more_problems_than_waves_permuted_and_repeated(ta):
    res = model_of(ta, "logistic12", gr.logistic_body(12), 12, 13, np.float32)
    waves = 4 * torch.cuda.get_device_properties(0).multi_processor_count * res.stats()["wg_per_cu"]
    Pbig = waves + 501
    base = [gr.logistic_case(seed, 12, 40) for seed in range(64)]
    pick = np.arange(Pbig) % 64
    data = np.array([base[i][0] for i in pick], np.float32)
    x0 = np.array([base[i][1] for i in pick], np.float32)
    o = ta.Options()
    x = cuda(x0.copy())
    out = ta.Optimize(x, res.bind(cuda(data)), o)
    assert int(out.counters[3]) == Pbig
    x2 = cuda(x0.copy())
    out2 = ta.Optimize(x2, res.bind(cuda(data)), o)
    assert torch.equal(x, x2) and torch.equal(out.final_cost, out2.final_cost)   # repeated
    perm = np.random.default_rng(5).permutation(Pbig)
    xp = cuda(x0[perm].copy())
    outp = ta.Optimize(xp, res.bind(cuda(data[perm])), o)
    torch.cuda.synchronize()
    pt = torch.from_numpy(perm).cuda()
    assert torch.equal(xp, x[pt]) and torch.equal(outp.final_cost, out.final_cost[pt]) and torch.equal(outp.num_iters, out.num_iters[pt])
    assert torch.equal(outp.stop_reason, out.stop_reason[pt])
    assert torch.equal(x[:64], x[64:128])   # (the same problem in another wave)


@pytest.mark.parametrize("what", ["c", "gs", "hs", "J"])
def test_a_non_finite_item_ends_its_problem_alone(ta, what):
    n, items = 5, 70
    d = gr.exact_case(n, items, 3)[:, :, :]
    d[:, :, n + 2] = 1.0
    bad = d.copy()
    col = {"c": n, "gs": n + 1, "hs": n + 2, "J": 2}[what]
    bad[1, 66, col] = float("nan")
    res = model_of(ta, f"quadlike{n}", (f"T z = 0; for (int j = 0; j < {n}; ++j) z += p[j] * x[j];\n"
                                        f"c = p[{n}] + T(0.5) * p[{n + 2}] * z * z + p[{n + 1}] * z;\n"
                                        f"if (want_grad) {{ gs = p[{n + 1}] + p[{n + 2}] * z; hs = p[{n + 2}]; for (int a = 0; a < {n}; ++a) J[a] = p[a]; }}\n"),
                   n, n + 3, np.float64)
    x0 = np.full((3, n), 0.25)
    xa, xb = cuda(x0.copy()), cuda(x0.copy())
    oa = ta.Optimize(xa, res.bind(cuda(d)), ta.Options())
    ob = ta.Optimize(xb, res.bind(cuda(bad)), ta.Options())
    torch.cuda.synchronize()
    assert int(ob.stop_reason[1]) == int(ta.StopReason.kSystemHasNaNOrInf) and torch.equal(xb[1], cuda(x0[1]))
    for p in (0, 2):
        assert torch.equal(xa[p], xb[p]) and int(oa.stop_reason[p]) == int(ob.stop_reason[p]) and int(oa.stop_reason[p]) >= 0


def test_a_problem_of_negative_curvature_still_descends(ta):
    """hs < 0 at every item of problem 0: H is wmin J J^T, Marquardt's damping scales its diagonal, and the steps along -g are short but
    downhill — the cost decreases and no step is taken uphill; problem 1 (hs > 0) converges as usual."""
    n, items = 3, 30
    rng = np.random.default_rng(3)
    d = np.zeros((2, items, n + 2))
    d[:, :, :n] = rng.normal(size=(2, items, n))
    d[:, :, n] = rng.normal(size=(2, items))
    d[0, :, n + 1], d[1, :, n + 1] = -1.0, 1.0
    res = model_of(ta, f"quadratic{n}", gr.quadratic_body(n), n, n + 2, np.float64)
    x0 = np.full((2, n), 0.1)
    x = cuda(x0.copy())
    model = res.bind(cuda(d))
    c0 = ta.accumulate(model, cuda(x0.copy()), want_grad=False)[2].cpu().numpy()
    o = ta.Options()
    o.max_iters = 1   # (the concave quadratic is unbounded below: one step, a long one along -g since H is tiny, and it must be downhill)
    out = ta.Optimize(x, model, o, history=True)
    torch.cuda.synchronize()
    c1 = ta.accumulate(model, x, want_grad=False)[2].cpu().numpy()
    print("negative curvature: cost", c0[0], "->", c1[0], "stop", int(out.stop_reason[0]), "iterations", int(out.num_iters[0]))
    assert int(out.stop_reason[0]) >= 0 and np.isfinite(c1[0]) and c1[0] < c0[0]
    assert c1[1] < c0[1]
    H = ta.accumulate(model, cuda(x0.copy()))[1].cpu().numpy()
    assert np.linalg.eigvalsh(H[0]).min() >= -1e-300 and np.abs(H[0]).max() < 1e-50   # positive semi-definite, and tiny


def test_outputs_and_save_last(ta):
    n, items = 13, 200
    cases = [gr.logistic_case(seed, n, items) for seed in range(P_TRAJ)]
    data, x0 = cuda(np.array([c[0] for c in cases])), np.array([c[1] for c in cases])
    res = model_of(ta, "logistic13", gr.logistic_body(n), n, n + 1, np.float64)
    # one Gauss-Newton pass builds at x0 and nowhere else: final_hessian is the seam's H at x0, exactly (save_last, the default)
    og = ta.Options()
    og.solver_type, og.max_iters = ta.Options.GaussNewton, 0
    xg = cuda(x0.copy())
    outg = ta.Optimize(xg, res.bind(data), og)
    H0 = ta.accumulate(res.bind(data), cuda(x0.copy()))[1]
    assert torch.equal(outg.final_hessian, H0.to(torch.float64))
    assert (outg.final_num_residuals.cpu().numpy() == 1).all() and (outg.final_inlier_ratio.cpu().numpy() == 1).all()
    # a problem solved alone equals its row in the batch, bit for bit
    o = ta.Options()
    x = cuda(x0.copy())
    out = ta.Optimize(x, res.bind(data), o)
    x1 = cuda(x0[2:3].copy())
    out1 = ta.Optimize(x1, res.bind(data[2:3].contiguous()), o)
    assert torch.equal(x1[0], x[2]) and out1.final_cost[0] == out.final_cost[2] and torch.equal(out1.final_hessian[0], out.final_hessian[2])


def test_check_gradient(ta):
    n = 12
    cases = [gr.logistic_case(seed, n, 200) for seed in range(3)]
    data, x = cuda(np.array([c[0] for c in cases])), cuda(np.array([c[1] for c in cases]))
    res = model_of(ta, "logistic12", gr.logistic_body(n), n, n + 1, np.float64)
    good = ta.CheckGradient(res.bind(data), x, check_H=True)   # (u is linear in x: H agrees with the differences too)
    print("CheckGradient: g", good.max_dist_g.tolist(), "H", good.max_dist_H.tolist(), "eps", good.eps)
    assert good.all() and float(good.max_dist_H.max()) < good.eps and float(good.max_dist_g.max()) < good.eps
    assert ta.CheckGradient(res.bind(data), x, check_H=False).all()
    flipped = model_of(ta, "logistic12 flipped", gr.logistic_body(n, flip=True), n, n + 1, np.float64)
    bad = ta.CheckGradient(flipped.bind(data), x, check_H=False)
    assert not bad.ok.any() and float(bad.max_dist_g.min()) > bad.eps


def test_no_scratch(ta):
    for n in (12, 50):
        st = model_of(ta, f"logistic{n}", gr.logistic_body(n), n, n + 1, np.float32).stats()
        print(f"logistic n = {n} fp32 stats", st)
        assert st["scratch_bytes"] == 0 and st["num_regs"] > 0 and st["wg_per_cu"] >= 1 and st["lds_bytes_per_wg"] > 0


def test_refusals_through_the_c_abi(ta):
    body, n = gr.logistic_body(2), 2
    res = model_of(ta, "logistic2", body, n, 3, np.float64)
    Pn = 3
    data = torch.zeros(Pn, 1, 3, dtype=torch.float64, device="cuda")
    model, xx = res.bind(data), cuda(np.tile([-1.2, 1.0], (Pn, 1)))
    ctx, lib, check = ta.api.default_context(), ta.api.default_context().lib, ta.api.check
    from tinyopt_amd import _capi
    C = ta.api.C
    h = C.c_void_p()
    spec = _capi.ToaJitSpec()
    spec.dtype, spec.num_params, spec.residuals_per_item, spec.scalars_per_item, spec.kind = 1, 64, 1, 1, 5
    with pytest.raises(ta.ToaError, match=r"TOA_JIT_COST_GGN.*1 <= num_params <= 63 .* not 64"):
        check(lib.toa_model_compile_ex(ctx.h, C.byref(spec), body.encode(), C.byref(h), None, 0))
    for field, val, text in (("residuals_per_item", 2, "residuals_per_item must be 1"), ("manifold", 1, "Euclidean parameters only"),
                             ("diff", 2, "diff must be TOA_DIFF_DEFAULT"), ("large_n", 1, "large_n is for residual models")):
        spec = _capi.ToaJitSpec()
        spec.dtype, spec.num_params, spec.residuals_per_item, spec.scalars_per_item, spec.kind = 1, 2, 1, 3, 5
        setattr(spec, field, val)
        with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*" + text):
            check(lib.toa_model_compile_ex(ctx.h, C.byref(spec), body.encode(), C.byref(h), None, 0))
    out = ta.api._alloc_output(Pn, 2, ta.Options(), False, xx.device)
    rp = ta.api._results_pod(out)
    pod = ta.Options().to_pod()
    head = (ctx.h, res._h, 1, Pn, model.packed.data_ptr())
    x1 = xx.clone()
    g, H, c = (torch.zeros(Pn, 2, dtype=torch.float64, device="cuda"), torch.zeros(Pn, 2, 2, dtype=torch.float64, device="cuda"),
               torch.zeros(Pn, dtype=torch.float64, device="cuda"))
    check(lib.toa_set_loss(ctx.h, 1, 1.0))   # a handle with a loss set
    try:
        with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*no residuals to robustify"):
            check(lib.toa_jit_lm_run(*head, x1.data_ptr(), C.byref(pod), C.byref(rp), None))
        with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*no residuals to robustify"):
            check(lib.toa_jit_accumulate(*head, x1.data_ptr(), 1, g.data_ptr(), H.data_ptr(), c.data_ptr(), None))
    finally:
        check(lib.toa_set_loss(ctx.h, 0, 0.0))
    gdo = _capi.ToaGdOptions()
    lib.toa_gd_options_default(C.byref(gdo))
    pod_gd = ta.Options().to_pod()
    pod_gd.solver_type = 2
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*GradientDescent"):
        check(lib.toa_jit_gd_run(*head, x1.data_ptr(), C.byref(pod_gd), C.byref(gdo), C.byref(rp), None))
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*GradientDescent"):
        check(lib.toa_jit_lm_run(*head, x1.data_ptr(), C.byref(pod_gd), C.byref(rp), None))
    lbo = _capi.ToaLbfgsOptions()
    lib.toa_lbfgs_options_default(C.byref(lbo))
    pod_lb = ta.Options().to_pod()
    pod_lb.solver_type = 3
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*L-BFGS"):
        check(lib.toa_jit_lbfgs_run(*head, x1.data_ptr(), C.byref(pod_lb), C.byref(lbo), C.byref(rp), None))
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*L-BFGS"):
        check(lib.toa_jit_lm_run(*head, x1.data_ptr(), C.byref(pod_lb), C.byref(rp), None))
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*row-split"):
        check(lib.toa_jit_lm_run_split(*head, x1.data_ptr(), C.byref(pod), C.byref(rp), None, 2))
    state = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*stepping form"):
        check(lib.toa_jit_lm_begin(*head, x1.data_ptr(), C.byref(pod), C.byref(rp), state.data_ptr()))
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*no residual rows"):
        check(lib.toa_jit_eval(*head, x1.data_ptr(), g.data_ptr(), None))
    prior = _capi.ToaPrior()
    prior.mu_dev, prior.W_dev, prior.rows = g.data_ptr(), g.data_ptr(), 0
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*Gaussian prior"):
        check(lib.toa_jit_lm_run_prior(*head, x1.data_ptr(), C.byref(prior), C.byref(pod), C.byref(rp), None))
    bounds = _capi.ToaBounds()
    bounds.lo_dev, bounds.hi_dev = g.data_ptr(), g.data_ptr()
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*box bounds"):
        check(lib.toa_jit_lm_run_bounds(*head, x1.data_ptr(), C.byref(bounds), None, C.byref(pod), C.byref(rp), None))
    off = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device="cuda")
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*ragged batches"):
        check(lib.toa_jit_lm_run_ragged(ctx.h, res._h, off.data_ptr(), None, 1, 3, Pn, data.data_ptr(), x1.data_ptr(), C.byref(pod), C.byref(rp), None, 0))
    v = [C.c_int(0) for _ in range(3)]
    with pytest.raises(ta.ToaError, match="TOA_JIT_COST_GGN.*no ragged, prior or bounds form"):
        check(lib.toa_jit_model_stats_ragged(ctx.h, res._h, *[C.byref(t) for t in v]))
    assert torch.equal(x1, xx)   # nothing ran
    # H_dev may be NULL: g and the cost alone
    check(lib.toa_jit_accumulate(*head, x1.data_ptr(), 1, g.data_ptr(), None, c.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(g, ta.accumulate(model, xx)[0])
