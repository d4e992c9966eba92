"""What every run entry point refuses, pinned through the raw C ABI: the return code and the exact toa_last_error() text for a
missing final_cost, a history stride one short, max_iters = 70000, a solver_type the entry does not serve and null options — and
what an empty batch (P = 0) returns when the data pointers are null.

Entry points: toa_lm_run, toa_jit_lm_run, toa_jit_lm_run_split, toa_jit_lm_begin / _step / _stop, toa_jit_gd_run, toa_ba_run and
toa_ba_lists_run.  Shapes are tiny (n = 3, 8 items, P = 2) and one residual model and one cost model serve the whole file.

Two things the entries do NOT have in common, pinned as they are:
  * the stepping form of a run-time model (toa_jit_lm_begin / _step / _stop) has no max_iters bound — the host drives its loop —
    so max_iters = 70000 is accepted there (one begin, step, stop on two 8-row problems);
  * P = 0 returns TOA_OK whatever the data pointers are on the run-time-model entries only: toa_lm_run, toa_ba_run and
    toa_ba_lists_run test their pointers first ("<entry>: null pointer", "DenseRow: data pointer is null").

The second half pins what the compiled-in entries refuse about the ROUTE of a call (csrc/small_route.hpp and the checks of
csrc/capi.hip in front of it): a row-split of a family that has none, the natural layout's missing forms, a parameter count
without an instance, a stepping call without its state or stop block, a dtype that is neither TOA_F32 nor TOA_F64."""
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


# ---- the routing refusals of the compiled-in entries (toa_lm_run / _run_split / _begin / _stop, toa_accumulate and the two
# ---- per-element helpers): code and exact text; every one is decided before anything is launched ----
E_UNSUPPORTED = -4
DTYPE_TEXT = "dtype must be TOA_F32 or TOA_F64"
ROW_SPLIT_TEXT = "row-split execution is available for DenseRow and SE3Reproj"


def compiled_in(env, entry, model, n, *, dtype=None, splits=None, state=True, stop_request=True):
    """`entry` of the compiled-in families on the file's buffers (m = ITEMS, P problems)."""
    lib, h, k = env.lib, env.ctx.h, env.capi
    dtype = k.F64 if dtype is None else dtype
    o, r = env.options("toa_lm_run"), env.results()
    head = (h, model, dtype, n, ITEMS, P, env.data.data_ptr(), env.x.data_ptr(), C.byref(o), C.byref(r))
    cnt, st = env.counters.data_ptr(), (env.state.data_ptr() if state else None)
    if entry == "toa_lm_run":
        return lib.toa_lm_run(*head, cnt)
    if entry == "toa_lm_run_split":
        return lib.toa_lm_run_split(*head, cnt, splits)
    if entry == "toa_lm_begin":
        return lib.toa_lm_begin(*head, st)
    if entry == "toa_lm_stop":
        return lib.toa_lm_stop(*head, cnt, st, env.stop_request.data_ptr() if stop_request else None)
    raise KeyError(entry)


def refused_with(env, rc, code, text):
    assert rc == code, (rc, env.lib.toa_last_error())
    assert env.lib.toa_last_error().decode() == text


@pytest.mark.parametrize("model,n", [("MODEL_CIRCLE_FIT", 3), ("MODEL_DENSE_ROW_AD", 12)])
@pytest.mark.parametrize("splits", [0, 1])
def test_row_split_of_a_family_without_one(env, model, n, splits):
    refused_with(env, compiled_in(env, "toa_lm_run_split", getattr(env.capi, model), n, splits=splits), E_UNSUPPORTED, ROW_SPLIT_TEXT)


def test_row_split_negative_splits(env):
    refused_with(env, compiled_in(env, "toa_lm_run_split", env.capi.MODEL_DENSE_ROW, N, splits=-1), E_ARG,
                 "toa_lm_run_split: splits must be >= 0 (0 = choose automatically)")


@pytest.mark.parametrize("splits", [0, 2])
def test_natural_layout_has_no_row_split_form(env, splits):
    refused_with(env, compiled_in(env, "toa_lm_run_split", env.capi.MODEL_DENSE_ROW_NATURAL, N, splits=splits), E_UNSUPPORTED,
                 "TOA_MODEL_DENSE_ROW_NATURAL: no row-split form")


def test_natural_layout_stepping_form_below_64(env):
    refused_with(env, compiled_in(env, "toa_lm_begin", env.capi.MODEL_DENSE_ROW_NATURAL, 6), E_UNSUPPORTED,
                 "TOA_MODEL_DENSE_ROW_NATURAL: the stepping form starts at n = 64 (use TOA_MODEL_DENSE_ROW below)")


def test_dense_row_ad_at_an_n_without_an_instance(env):
    refused_with(env, compiled_in(env, "toa_lm_run", env.capi.MODEL_DENSE_ROW_AD, 13), E_UNSUPPORTED,
                 "DenseRowAD: instantiated for n = 12 and n = 50 (a functor's parameter count is a compile-time constant)")


def test_begin_without_a_state_block(env):
    refused_with(env, compiled_in(env, "toa_lm_begin", env.capi.MODEL_DENSE_ROW, N, state=False), E_ARG,
                 "toa_lm_begin / toa_lm_step: state_dev is null")


def test_stop_without_a_stop_request(env):
    refused_with(env, compiled_in(env, "toa_lm_stop", env.capi.MODEL_DENSE_ROW, N, stop_request=False), E_ARG,
                 "toa_lm_stop: stop_request_dev is null")


@pytest.mark.parametrize("entry", ["toa_lm_run", "toa_accumulate", "toa_robust_norm", "toa_jet_eval"])
def test_bad_dtype(env, entry):
    lib, h, bad = env.lib, env.ctx.h, 7
    d, x, f = env.data.data_ptr(), env.x.data_ptr(), env.final.data_ptr()
    if entry == "toa_lm_run":
        rc = compiled_in(env, entry, env.capi.MODEL_DENSE_ROW, N, dtype=bad)
    elif entry == "toa_accumulate":
        rc = lib.toa_accumulate(h, env.capi.MODEL_DENSE_ROW, bad, N, ITEMS, P, d, x, 0, None, None, f, None)
    elif entry == "toa_robust_norm":
        rc = lib.toa_robust_norm(h, 1, bad, P, d, 1.0, x, f)
    else:
        rc = lib.toa_jet_eval(h, 0, bad, P, d, d, x)
    refused_with(env, rc, E_ARG, ("toa_robust_norm: " if entry == "toa_robust_norm" else "") + DTYPE_TEXT)
