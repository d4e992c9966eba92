"""What every run entry point refuses, pinned through the raw C ABI: the return code and the exact toa_last_error() text for a
missing final_cost, a history stride one short, max_iters = 70000, a solver_type the entry does not serve and null options — and
what an empty batch (P = 0) returns when the data pointers are null.

Entry points: toa_lm_run, toa_jit_lm_run, toa_jit_lm_run_split, toa_jit_lm_begin / _step / _stop, toa_jit_gd_run, toa_ba_run and
toa_ba_lists_run.  Shapes are tiny (n = 3, 8 items, P = 2) and one residual model and one cost model serve the whole file.

Two things the entries do NOT have in common, pinned as they are:
  * the stepping form of a run-time model (toa_jit_lm_begin / _step / _stop) has no max_iters bound — the host drives its loop —
    so max_iters = 70000 is accepted there (one begin, step, stop on two 8-row problems);
  * P = 0 returns TOA_OK whatever the data pointers are on the run-time-model entries only: toa_lm_run, toa_ba_run and
    toa_ba_lists_run test their pointers first ("<entry>: null pointer", "DenseRow: data pointer is null")."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

E_ARG = -1
N, ITEMS, P = 3, 8, 2
MAX_ITERS = 5
LM_SOLVER = "solver_type must be 0 (LM) or 1 (GN)"
# entry -> (the name its messages carry, its solver_type message, its null-options message)
ENTRIES = {
    "toa_lm_run": ("toa_lm_run", LM_SOLVER + " on this path", "toa_lm_run: null pointer"),
    "toa_jit_lm_run": ("toa_jit_lm_run", LM_SOLVER, "toa_jit_lm_run: null pointer"),
    "toa_jit_lm_run_split": ("toa_jit_lm_run_split", LM_SOLVER, "toa_jit_lm_run_split: null pointer"),
    "toa_jit_lm_begin": ("toa_jit_lm_step", LM_SOLVER, "toa_jit_lm_step: null pointer"),
    "toa_jit_lm_step": ("toa_jit_lm_step", LM_SOLVER, "toa_jit_lm_step: null pointer"),
    "toa_jit_lm_stop": ("toa_jit_lm_step", LM_SOLVER, "toa_jit_lm_step: null pointer"),
    "toa_jit_gd_run": ("toa_jit_gd_run", "solver_type must be 2 (GradientDescent)", "toa_jit_gd_run: null options"),
    "toa_ba_run": ("toa_ba_run", LM_SOLVER, "toa_ba_run: null pointer"),
    "toa_ba_lists_run": ("toa_ba_lists_run", LM_SOLVER, "toa_ba_lists_run: null pointer"),
}
STEPPING = ("toa_jit_lm_begin", "toa_jit_lm_step", "toa_jit_lm_stop")
JIT = ("toa_jit_lm_run", "toa_jit_lm_run_split", "toa_jit_gd_run") + STEPPING


class Env:
    def __init__(self, ta):
        from tinyopt_amd import _capi
        from tinyopt_amd.api import Context
        self.capi = _capi
        self.ctx = Context()
        self.lib = self.ctx.lib
        f64 = dict(dtype=torch.float64, device="cuda")
        self.residual = ta.JitResidual("r[0] = p[0] * x[0] + p[1] * x[1] + x[2] - p[2];", n=N, item_scalars=3, ctx=self.ctx)
        self.cost = ta.JitResidual("const S e = p[0] * x[0] + p[1] * x[1] + x[2] - p[2]; c = e * e;", n=N, item_scalars=3,
                                   kind="cost", ctx=self.ctx)
        gen = torch.Generator(device="cpu").manual_seed(7)
        self.data = torch.randn(P, ITEMS, 3, dtype=torch.float64, generator=gen).cuda()
        self.x = torch.zeros(P, 12, **f64)            # (wide enough for every entry's parameter block)
        self.ids = torch.zeros(64, dtype=torch.int32, device="cuda")   # observation lists of toa_ba_lists_run
        self.stop = torch.zeros(P, dtype=torch.int32, device="cuda")
        self.iters = torch.zeros(P, dtype=torch.int32, device="cuda")
        self.final = torch.zeros(P, **f64)
        self.errs = torch.zeros(P, MAX_ITERS + 2, **f64)
        self.counters = torch.zeros(8, dtype=torch.int64, device="cuda")
        self.active = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.stop_request = torch.zeros(P, dtype=torch.int32, device="cuda")
        self.state = torch.zeros(self.lib.toa_lm_state_bytes(_capi.F64, N, P), dtype=torch.uint8, device="cuda")
        self.gd = _capi.ToaGdOptions()
        self.lib.toa_gd_options_default(C.byref(self.gd))

    def options(self, entry):
        o = self.capi.ToaOptions()
        self.lib.toa_options_default(C.byref(o))
        o.solver_type = 2 if entry == "toa_jit_gd_run" else 0
        o.max_iters = MAX_ITERS
        return o

    def results(self):
        r = self.capi.ToaResults()
        r.stop_reason, r.num_iters, r.final_cost = self.stop.data_ptr(), self.iters.data_ptr(), self.final.data_ptr()
        return r

    def call(self, entry, o, r, batch=P, null_data=False):
        """`entry` on the file's buffers; o / r: the options / results blocks (None = a null pointer)."""
        lib, h = self.lib, self.ctx.h
        po = C.byref(o) if o is not None else None
        pr = C.byref(r) if r is not None else None
        d = None if null_data else self.data.data_ptr()
        x = None if null_data else self.x.data_ptr()
        ids = None if null_data else self.ids.data_ptr()
        cnt, st = self.counters.data_ptr(), (None if null_data else self.state.data_ptr())
        res, cost = self.residual._h, self.cost._h
        if entry == "toa_lm_run":
            return lib.toa_lm_run(h, self.capi.MODEL_DENSE_ROW, self.capi.F64, N, ITEMS, batch, d, x, po, pr, cnt)
        if entry == "toa_jit_lm_run":
            return lib.toa_jit_lm_run(h, res, ITEMS, batch, d, x, po, pr, cnt)
        if entry == "toa_jit_lm_run_split":
            return lib.toa_jit_lm_run_split(h, res, ITEMS, batch, d, x, po, pr, cnt, 0)
        if entry == "toa_jit_lm_begin":
            return lib.toa_jit_lm_begin(h, res, ITEMS, batch, d, x, po, pr, st)
        if entry == "toa_jit_lm_step":
            return lib.toa_jit_lm_step(h, res, ITEMS, batch, d, x, po, pr, cnt, st, self.active.data_ptr())
        if entry == "toa_jit_lm_stop":
            return lib.toa_jit_lm_stop(h, res, ITEMS, batch, d, x, po, pr, cnt, st, self.stop_request.data_ptr())
        if entry == "toa_jit_gd_run":
            return lib.toa_jit_gd_run(h, cost, ITEMS, batch, d, x, po, C.byref(self.gd), pr, cnt)
        if entry == "toa_ba_run":
            return lib.toa_ba_run(h, self.capi.F64, 1, ITEMS, batch, d, x, po, pr, cnt)
        if entry == "toa_ba_lists_run":
            return lib.toa_ba_lists_run(h, self.capi.F64, 1, 2, ITEMS, batch, d, ids, ids, d, x, po, pr, cnt, 0.0)
        raise KeyError(entry)

    def refused(self, entry, o, r, text, **kw):
        rc = self.call(entry, o, r, **kw)
        assert rc == E_ARG, (entry, rc, self.lib.toa_last_error())
        assert self.lib.toa_last_error().decode() == text, entry


@pytest.fixture(scope="module")
def env(ta):
    e = Env(ta)
    yield e
    torch.cuda.synchronize()
    e.residual.close()
    e.cost.close()
    e.ctx.close()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_missing_final_cost(env, entry):
    r = env.results()
    r.final_cost = None
    env.refused(entry, env.options(entry), r, f"{ENTRIES[entry][0]}: stop_reason, num_iters and final_cost outputs are required")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_history_stride_one_short(env, entry):
    r = env.results()
    r.errs, r.hist_stride = env.errs.data_ptr(), MAX_ITERS + 1
    env.refused(entry, env.options(entry), r, f"{ENTRIES[entry][0]}: hist_stride must be >= max_iters + 2")


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e not in STEPPING])
def test_max_iters_out_of_range(env, entry):
    o = env.options(entry)
    o.max_iters = 70000
    env.refused(entry, o, env.results(), "max_iters out of range")


def test_max_iters_unbounded_in_the_stepping_form(env):
    """(the host drives this loop: nothing in it is sized by max_iters)"""
    o = env.options("toa_jit_lm_begin")
    o.max_iters = 70000
    for entry in STEPPING:
        assert env.call(entry, o, env.results()) == 0, (entry, env.lib.toa_last_error())
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_solver_type_not_served(env, entry):
    o = env.options(entry)
    o.solver_type = 0 if entry == "toa_jit_gd_run" else 2
    env.refused(entry, o, env.results(), f"{ENTRIES[entry][0]}: {ENTRIES[entry][1]}")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_options(env, entry):
    env.refused(entry, None, env.results(), ENTRIES[entry][2])


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_empty_batch(env, entry):
    o, r = env.options(entry), env.results()
    assert env.call(entry, o, r, batch=0) == 0, (entry, env.lib.toa_last_error())
    if entry in JIT:
        assert env.call(entry, o, r, batch=0, null_data=True) == 0, (entry, env.lib.toa_last_error())
    else:
        text = "DenseRow: data pointer is null" if entry == "toa_lm_run" else f"{entry}: null pointer"
        env.refused(entry, o, r, text, batch=0, null_data=True)
