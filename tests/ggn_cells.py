"""The trajectory cells of kind="cost_ggn" (DESIGN section 20), shared by tests/test_gpu_ggn.py and tests/test_cpu_ggn_reference.py:
five problems x five option sets, six seeded problems each, and their yardstick outputs (computed once per process).

A seed is usable when the yardstick ALONE — ggn_reference.py inside the second reading of the loop — takes no accept / reject decision
closer than 1e-9 (relative) to flipping (decision_margin below).  ONE kind of decision is exempt, because no seed with a rejected step
is free of it: after a rejected step the loop rolls x back by x + dx - dx, which returns x to an ulp, evaluates there again and
compares that cost with the accepted one — two numbers equal in exact arithmetic.  Whether that pass counts as accepted is round-off's
choice on either side; parity.check_trajectories proves such a parting a tie (same point, cost on the floor of the accepted cost, same
end) and refuses every other.  The seeds were found by running the yardstick over 0, 1, 2, ... on the CPU:
per cell the first three usable seeds whose run REJECTS at least one step (the roll-back's coverage), then the first usable seeds
without one.  Starts are far from the optimum so that steps overshoot: the logistic starts of hess_reference.logistic_case times 8,
the spot's amplitude times 1.7 and its background halved.  Two cells are left out: LEFT_OUT."""
import numpy as np

import ggn_reference as gr

NEED_MARGIN = 1e-9
P_TRAJ = 6
X0_SCALE = 8.0
OPTION_SETS = {
    "default": dict(),
    "benchmark": dict(base="benchmark"),
    "gauss_newton": dict(solver="gn"),
    "grad_clipping": dict(grad_clipping=2.0),   # (the spot's gradients are counts: clipped at 50, see options_of)
    "no_ldlt": dict(use_ldlt=False),
}
PROBLEMS = ("logistic12", "logistic13", "logistic50", "logistic63", "spot")
SEEDS = {
    ("logistic12", "default"): [1, 2, 3, 103, 172, 253], ("logistic12", "benchmark"): [1, 2, 3, 5, 6, 7],
    ("logistic12", "gauss_newton"): [1, 2, 3, 103, 172, 253], ("logistic12", "no_ldlt"): [1, 2, 3, 103, 172, 253],
    ("logistic13", "default"): [0, 1, 2, 218, 286, 367], ("logistic13", "benchmark"): [0, 1, 2, 4, 5, 6],
    ("logistic13", "gauss_newton"): [0, 1, 2, 218, 286, 367], ("logistic13", "no_ldlt"): [0, 1, 2, 218, 286, 367],
    ("logistic50", "default"): [0, 1, 2, 3, 4, 5], ("logistic50", "benchmark"): [0, 1, 2, 735, 3, 4],
    ("logistic50", "gauss_newton"): [0, 1, 2, 3, 4, 5], ("logistic50", "grad_clipping"): [0, 1, 2, 3, 4, 5],
    ("logistic50", "no_ldlt"): [0, 1, 2, 3, 4, 5],
    ("logistic63", "default"): [0, 1, 2, 172, 3, 4], ("logistic63", "benchmark"): [0, 1, 2, 172, 3, 4],
    ("logistic63", "gauss_newton"): [0, 1, 2, 172, 3, 4], ("logistic63", "grad_clipping"): [0, 1, 2, 172, 209, 3],
    ("logistic63", "no_ldlt"): [0, 1, 2, 172, 3, 4],
    ("spot", "default"): [0, 4, 6, 33, 117, 122], ("spot", "benchmark"): [0, 4, 6, 7, 12, 18],
    ("spot", "gauss_newton"): [0, 4, 6, 33, 117, 122], ("spot", "grad_clipping"): [0, 1, 3, 4, 29, 117],
    ("spot", "no_ldlt"): [0, 4, 6, 33, 117, 122],
}
# Left out, two cells of twenty-five: logistic regression at n = 12 and n = 13 with the gradient clipped at 2 — of their seeds 0 .. 1800
# none (n = 12) and one (n = 13) is usable AND rejects a step (a clipped gradient shortens every step: nothing overshoots).
LEFT_OUT = [("logistic12", "grad_clipping"), ("logistic13", "grad_clipping")]
CELLS = [(p, o) for p in PROBLEMS for o in OPTION_SETS if (p, o) not in LEFT_OUT]


def options_of(problem, optname):
    kw = dict(OPTION_SETS[optname])
    if problem == "spot" and optname == "grad_clipping":
        kw["grad_clipping"] = 50.0
    return kw


def case_of(problem, seed):
    """(data [items, item scalars], x0 [n]) of a cell's problem"""
    if problem == "spot":
        d, x0 = gr.spot_case(seed)
        x0 = x0.copy()
        x0[0] *= 1.7
        x0[3] *= 0.5
        return d, x0
    d, x0 = gr.logistic_case(seed, int(problem[len("logistic"):]), 200)
    return d, x0 * X0_SCALE


def decision_margin(r):
    """The smallest relative distance |err - accepted| / accepted over the accept / reject decisions of a yardstick run, the re-evaluation
    of a rolled-back point (the pass after a rejected one, within 1e-12 of the accepted cost) exempt."""
    acc, prev_ok, m = None, True, float("inf")
    for i, (e, s) in enumerate(zip(r["errs"], r["successes"])):
        if i == 0:
            acc = e
        else:
            rel = abs(e - acc) / max(abs(acc), 1e-300)
            if prev_ok or rel > 1e-12:
                m = min(m, rel)
            if s:
                acc = e
        prev_ok = bool(s)
    return m


_CACHE = {}


def trajectory_cases(problem, optname):
    """(the P_TRAJ problems of a cell, their yardstick outputs, the cell's option keywords); computed once, shared, not changed."""
    key = (problem, optname)
    if key not in _CACHE:
        parts = gr.spot_parts if problem == "spot" else gr.logistic_parts
        kw = options_of(problem, optname)
        _, ropt = gr.options_pair(None, **kw)
        cases = [case_of(problem, seed) for seed in SEEDS[key]]
        with np.errstate(over="ignore", invalid="ignore"):   # (a far start saturates exp(-y z): the item's cost is then -y z, as on the device)
            refs = [gr.optimize(parts, d, x0, ropt) for d, x0 in cases]
        for seed, r in zip(SEEDS[key], refs):
            assert decision_margin(r) >= NEED_MARGIN and r["stop"] >= 0, (problem, optname, seed, "the yardstick sits on a tie", decision_margin(r))
        _CACHE[key] = (cases, refs, kw)
    return _CACHE[key]
