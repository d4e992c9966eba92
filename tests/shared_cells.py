"""The trajectory cells of shared item tables, used by tests/test_gpu_shared.py: five problems x three option sets,
six seeded problems each that SHARE one table, and their yardstick outputs (computed once per process).

  logistic12 / logistic50   kind="cost_ggn": logistic regression on ONE design matrix (ggn_reference.logistic_case(0)'s X): per seed
                            noisy labels from a planted weight vector and a start times 8 (far, so that steps overshoot)
  decay                     kind="residual" (Jets): y = A exp(-k t) + b over ONE time axis, n = 3, 45 samples, starts off the truth
  decay_acc                 kind="accumulate": the same fit with its hand-written Jacobian rows (the same yardstick, the same seeds): the
                            accumulate kind's cells with rejected steps
  linear50                  kind="accumulate": r = s . x - p[0] on ONE design matrix, n = 50, 130 items

The seed rule is ggn_cells.py's: a seed is usable when the yardstick alone takes no accept / reject decision closer than 1e-9
(relative) to flipping (ggn_cells.decision_margin; the re-evaluation of a rolled-back point exempt), found by `find_seeds` over
0, 1, 2, ... on the CPU: per cell the first six usable seeds, at least two of which reject a step.
linear50 is a linear least-squares problem: no step of it is ever rejected, so its cells carry no such coverage (REJECTS).
No cell is left out."""
import numpy as np

import bounds_reference as br
import ggn_cells as gc
import ggn_reference as gr
import shared_reference as sr

ref = br.ref
P_TRAJ = 6
OPTION_SETS = {"default": dict(), "benchmark": dict(base="benchmark"), "gauss_newton": dict(solver="gn")}
PROBLEMS = ("logistic12", "logistic50", "decay", "decay_acc", "linear50")
REJECTS = {"logistic12": True, "logistic50": True, "decay": True, "decay_acc": True, "linear50": False}
# The margin rule is section 20's, for kind="cost_ggn" (the decay fit meets it too).  A linear least-squares solve ends ON the round-off
# floor — its second step changes the cost by ulps, whatever the seed —, which parity.check_trajectories proves a tie.
MARGIN = {"logistic12": True, "logistic50": True, "decay": True, "decay_acc": True, "linear50": False}
SEEDS = {
    ("logistic12", "default"): [0, 1, 2, 3, 4, 6], ("logistic12", "benchmark"): [0, 1, 2, 3, 4, 6], ("logistic12", "gauss_newton"): [0, 1, 2, 3, 4, 6],
    ("logistic50", "default"): [0, 1, 2, 3, 4, 5], ("logistic50", "benchmark"): [0, 1, 2, 3, 4, 5], ("logistic50", "gauss_newton"): [0, 1, 2, 3, 4, 5],
    ("decay", "default"): [0, 1, 2, 3, 5, 6], ("decay", "benchmark"): [0, 1, 2, 3, 5, 6], ("decay", "gauss_newton"): [0, 1, 2, 3, 5, 6],
    ("decay_acc", "default"): [0, 1, 2, 3, 5, 6], ("decay_acc", "benchmark"): [0, 1, 2, 3, 5, 6], ("decay_acc", "gauss_newton"): [0, 1, 2, 3, 5, 6],
    ("linear50", "default"): [0, 1, 2, 3, 4, 5], ("linear50", "benchmark"): [0, 1, 2, 3, 4, 5], ("linear50", "gauss_newton"): [0, 1, 2, 3, 4, 5],
}
LEFT_OUT = []
CELLS = [(p, o) for p in PROBLEMS for o in OPTION_SETS if (p, o) not in LEFT_OUT]

DECAY_T = np.linspace(0.0, 4.0, 45)


def _residual_fn(rows):
    """rows(x) -> (r [m], J [m, n]) as the loop's callback (grad = J^T r, H = J^T J, cost = |r|^2 over m residuals)"""
    def fn(x, want):
        r, J = rows(np.asarray(x, np.float64))
        return ref._from_residuals(r.tolist(), J.tolist(), want)
    return fn


def table_of(problem):
    if problem.startswith("logistic"):
        n = int(problem[len("logistic"):])
        return gr.logistic_case(0, n, 200)[0][:, :n].copy()
    if problem in ("decay", "decay_acc"):
        return DECAY_T[:, None].copy()
    return np.random.default_rng(4100).normal(size=(130, 50)) / np.sqrt(50.0)


def case_of(problem, seed):
    """(the problem's private item scalars [items, 1], x0 [n], the yardstick's callback) on the problem's one table"""
    T = table_of(problem)
    rng = np.random.default_rng(4200 + seed)
    if problem.startswith("logistic"):   # (hess_reference.logistic_case's recipe on the ONE design: noisy labels from a planted weight vector)
        n = T.shape[1]
        w = rng.normal(size=n) * 2.0
        y = np.where(rng.uniform(size=T.shape[0]) < 1.0 / (1.0 + np.exp(-(T @ w))), 1.0, -1.0)
        x0 = rng.normal(size=n) * 0.3 * gc.X0_SCALE
        return y[:, None], x0, gr.item_sum(gr.logistic_parts, np.concatenate([T, y[:, None]], axis=1))
    if problem in ("decay", "decay_acc"):
        t = T[:, 0]
        A, k, b = rng.uniform(1.0, 3.0), rng.uniform(0.4, 1.5), rng.uniform(-0.5, 0.5)
        y = A * np.exp(-k * t) + b + 0.01 * rng.normal(size=len(t))
        x0 = np.array([A * rng.uniform(2.0, 4.0), k * rng.uniform(3.0, 6.0), b + rng.uniform(-2.0, 2.0)])

        def rows(x):
            E = np.exp(-x[1] * t)
            return x[0] * E + x[2] - y, np.stack([E, -x[0] * t * E, np.ones_like(E)], axis=1)
        return y[:, None], x0, _residual_fn(rows)
    y = rng.normal(size=T.shape[0])
    return y[:, None], rng.normal(size=T.shape[1]) * 3.0, _residual_fn(lambda x: (T @ x - y, T))


def model_of(problem):
    """(kind, body, n, shared_scalars) of the problem's device model; item_scalars = 1"""
    if problem.startswith("logistic"):
        n = int(problem[len("logistic"):])
        return "cost_ggn", sr.logistic_body(n), n, n
    if problem == "decay":
        return "residual", sr.DECAY_BODY, 3, 1
    if problem == "decay_acc":
        return "accumulate", sr.DECAY_ACC_BODY, 3, 1
    return "accumulate", sr.linear_body(50, "accumulate"), 50, 50


def run_yardstick(problem, optname, seed):
    _, ropt = gr.options_pair(None, **OPTION_SETS[optname])
    _, x0, fn = case_of(problem, seed)
    with np.errstate(over="ignore", invalid="ignore"):   # (a far start saturates exp: as on the device)
        return br.optimize_plain(fn, [float(v) for v in x0], ropt)


def find_seeds(problem, optname, limit=1800):
    """How SEEDS was made: the first six usable seeds, among them at least two (where the problem can reject at all) whose run rejects
    a step — a later rejecting seed replaces the last non-rejecting one until there are two."""
    usable, rejecting = [], set()
    need = 2 if REJECTS[problem] else 0
    for seed in range(limit):
        r = run_yardstick(problem, optname, seed)
        if r["stop"] < 0 or (MARGIN[problem] and gc.decision_margin(r) < gc.NEED_MARGIN):
            continue
        rej = not all(r["successes"])
        if len(usable) < P_TRAJ:
            usable.append(seed)
        elif rej and len(rejecting) < need:
            plain = [s for s in usable if s not in rejecting]
            usable[usable.index(plain[-1])] = seed
        else:
            continue
        if rej:
            rejecting.add(seed)
        if len(usable) == P_TRAJ and len(rejecting & set(usable)) >= need:
            return usable
    return None


_CACHE = {}


def trajectory_cases(problem, optname):
    """The cell: data [6, items, 1], table, x0 [6, n], the yardstick outputs, the model and the option keywords; computed once, not changed."""
    key = (problem, optname)
    if key not in _CACHE:
        kind, body, n, kS = model_of(problem)
        cases = [case_of(problem, seed) for seed in SEEDS[key]]
        refs = [run_yardstick(problem, optname, seed) for seed in SEEDS[key]]
        for seed, r in zip(SEEDS[key], refs):
            assert r["stop"] >= 0 and (not MARGIN[problem] or gc.decision_margin(r) >= gc.NEED_MARGIN), (problem, optname, seed, "the yardstick sits on a tie",
                                                                                                         gc.decision_margin(r))
        _CACHE[key] = dict(data=np.array([c[0] for c in cases]), table=table_of(problem), x0=np.array([c[1] for c in cases]), refs=refs,
                           kind=kind, body=body, n=n, kS=kS, options=dict(OPTION_SETS[optname]), rejects=REJECTS[problem])
    return _CACHE[key]
