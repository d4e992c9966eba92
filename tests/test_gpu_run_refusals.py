"""What every run entry point refuses, pinned through the raw C ABI: the return code and the exact toa_last_error() text for a
missing final_cost, a history stride one short, max_iters = 70000, a solver_type the entry does not serve and null options — and
what an empty batch (P = 0) returns when the data pointers are null.

Entry points: toa_lm_run, toa_jit_lm_run, toa_jit_lm_run_split, toa_jit_lm_begin / _step / _stop, toa_jit_gd_run, toa_ba_run and
toa_ba_lists_run, and the prior, ragged, seam and Eval entries of a run-time model.  Shapes are tiny (n = 3, 8 items, P = 2; the
ragged batch has counts [3, 5]; the prior is diagonal) and one residual model, one cost model and the residual compiled with
large_n serve the whole file.

Two things the entries do NOT have in common, pinned as they are:
  * the stepping form of a run-time model (toa_jit_lm_begin / _step / _stop) has no max_iters bound — the host drives its loop —
    so max_iters = 70000 is accepted there (one begin, step, stop on two 8-row problems);
  * P = 0 returns TOA_OK whatever the data pointers are on the run-time-model entries only: toa_lm_run, toa_ba_run and
    toa_ba_lists_run test their pointers first ("<entry>: null pointer", "DenseRow: data pointer is null").

The middle part pins what the prior, ragged, seam and Eval entries of a run-time model refuse (toa_jit_lm_run_prior / _ragged /
_ragged_prior, toa_jit_gd_run_ragged, toa_jit_accumulate and toa_jit_eval with their forms): code, exact text and, where two failing
conditions hold at once, which of the two is reported.  Every one is decided before anything is built or launched.

The last part pins what the compiled-in entries refuse about the ROUTE of a call (csrc/small_route.hpp and the checks of
csrc/capi.hip in front of it): a row-split of a family that has none, the natural layout's missing forms, a parameter count
without an instance, a stepping call without its state or stop block, a dtype that is neither TOA_F32 nor TOA_F64."""
import contextlib
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
    "toa_jit_lm_run_prior": ("toa_jit_lm_run_prior", LM_SOLVER, "toa_jit_lm_run_prior: null pointer"),
    "toa_jit_lm_run_ragged": ("toa_jit_lm_run_ragged", LM_SOLVER, "toa_jit_lm_run_ragged: null pointer"),
    "toa_jit_lm_run_ragged_prior": ("toa_jit_lm_run_ragged_prior", LM_SOLVER, "toa_jit_lm_run_ragged_prior: null pointer"),
    "toa_jit_gd_run_ragged": ("toa_jit_gd_run_ragged", "solver_type must be 2 (GradientDescent)", "toa_jit_gd_run_ragged: null options"),
    # the seams and Eval take no options: no solver_type or null-options message
    "toa_jit_accumulate": ("toa_jit_accumulate", None, None),
    "toa_jit_accumulate_prior": ("toa_jit_accumulate_prior", None, None),
    "toa_jit_accumulate_ragged": ("toa_jit_accumulate_ragged", None, None),
    "toa_jit_accumulate_ragged_prior": ("toa_jit_accumulate_ragged_prior", None, None),
    "toa_jit_eval": ("toa_jit_eval", None, None),
    "toa_jit_eval_ragged": ("toa_jit_eval_ragged", None, None),
}
RUN = [e for e in ENTRIES if ENTRIES[e][1] is not None]   # the entries that take options and results
STEPPING = ("toa_jit_lm_begin", "toa_jit_lm_step", "toa_jit_lm_stop")
GD = ("toa_jit_gd_run", "toa_jit_gd_run_ragged")
LM = ("toa_jit_lm_run", "toa_jit_lm_run_prior", "toa_jit_lm_run_ragged", "toa_jit_lm_run_ragged_prior")
SEAM = ("toa_jit_accumulate", "toa_jit_accumulate_prior", "toa_jit_accumulate_ragged", "toa_jit_accumulate_ragged_prior")
EVAL = ("toa_jit_eval", "toa_jit_eval_ragged")
PRIOR = tuple(e for e in ENTRIES if e.endswith("_prior"))
RAGGED = tuple(e for e in ENTRIES if "_ragged" in e)
FORMS = LM[1:] + GD[1:] + SEAM + EVAL   # the prior, ragged, seam and Eval entries
JIT = ("toa_jit_lm_run", "toa_jit_lm_run_split") + STEPPING + LM[1:] + GD
MAX_ITEMS = 5   # the ragged batch: counts [3, 5]


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
        self.large = ta.JitResidual("r[0] = p[0] * x[0] + p[1] * x[1] + x[2] - p[2];", n=N, item_scalars=3, large_n=True, ctx=self.ctx)
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
        self.offsets = torch.tensor([0, 3, ITEMS], dtype=torch.int64, device="cuda")   # (the ragged entries read data as [8][3])
        self.mu, self.W = torch.zeros(N, **f64), torch.ones(N, **f64)
        self.g, self.H, self.cost_out = torch.zeros(P, N, **f64), torch.zeros(P, N, N, **f64), torch.zeros(P, **f64)
        self.res_out, self.J_out = torch.zeros(P * ITEMS + 1, **f64), torch.zeros(P * ITEMS * N, **f64)

    def options(self, entry):
        o = self.capi.ToaOptions()
        self.lib.toa_options_default(C.byref(o))
        o.solver_type = 2 if entry in GD else 0
        o.max_iters = MAX_ITERS
        return o

    def results(self):
        r = self.capi.ToaResults()
        r.stop_reason, r.num_iters, r.final_cost = self.stop.data_ptr(), self.iters.data_ptr(), self.final.data_ptr()
        return r

    def prior(self, rows=0, mu=True):
        p = self.capi.ToaPrior()
        p.mu_dev, p.W_dev, p.rows = (self.mu.data_ptr() if mu else None), self.W.data_ptr(), rows
        return p

    def call(self, entry, o, r, batch=P, null_data=False, **kw):
        """`entry` on the file's buffers; o / r: the options / results blocks (None = a null pointer).  kw, for the entries of a
        run-time model: handle = False (a null handle); model = "residual" / "cost" / "large" / None (a null model); prior = a ToaPrior
        or None; items, max_items, total_items, flags; null = the data pointers to pass as null among "data", "x", "offsets";
        want_grad, g, H (the seams); res_dev, J_dev (Eval)."""
        a = dict(handle=True, model="cost" if entry in GD else "residual", prior=self.prior(), items=ITEMS, max_items=MAX_ITEMS,
                 total_items=ITEMS, flags=0, null=(), want_grad=0, g=None, H=None, res_dev=self.res_out.data_ptr(), J_dev=None)
        assert not set(kw) - set(a), kw
        a.update(kw)
        null = ("data", "x", "offsets") if null_data else a["null"]
        lib, h = self.lib, (self.ctx.h if a["handle"] else None)
        po = C.byref(o) if o is not None else None
        pr = C.byref(r) if r is not None else None
        d = None if "data" in null else self.data.data_ptr()
        x = None if "x" in null else self.x.data_ptr()
        ids = None if null_data else self.ids.data_ptr()
        cnt, st = self.counters.data_ptr(), (None if null_data else self.state.data_ptr())
        res, cost = self.residual._h, self.cost._h
        model = None if a["model"] is None else getattr(self, a["model"])._h
        pp = C.byref(a["prior"]) if a["prior"] is not None else None
        uni = (h, model, a["items"], batch, d, x)
        rag = (h, model, None if "offsets" in null else self.offsets.data_ptr(), None, a["max_items"], a["total_items"], batch, d, x)
        seam = (a["want_grad"], a["g"], a["H"], self.cost_out.data_ptr(), None)
        if entry == "toa_jit_lm_run_prior":
            return lib.toa_jit_lm_run_prior(*uni, pp, po, pr, cnt)
        if entry == "toa_jit_lm_run_ragged":
            return lib.toa_jit_lm_run_ragged(*rag, po, pr, cnt, a["flags"])
        if entry == "toa_jit_lm_run_ragged_prior":
            return lib.toa_jit_lm_run_ragged_prior(*rag, pp, po, pr, cnt, a["flags"])
        if entry == "toa_jit_gd_run_ragged":
            return lib.toa_jit_gd_run_ragged(*rag, po, C.byref(self.gd), pr, cnt, a["flags"])
        if entry == "toa_jit_accumulate":
            return lib.toa_jit_accumulate(*uni, *seam)
        if entry == "toa_jit_accumulate_prior":
            return lib.toa_jit_accumulate_prior(*uni, pp, *seam)
        if entry == "toa_jit_accumulate_ragged":
            return lib.toa_jit_accumulate_ragged(*rag, *seam)
        if entry == "toa_jit_accumulate_ragged_prior":
            return lib.toa_jit_accumulate_ragged_prior(*rag, pp, *seam)
        if entry == "toa_jit_eval":
            return lib.toa_jit_eval(*uni, a["res_dev"], a["J_dev"])
        if entry == "toa_jit_eval_ragged":
            return lib.toa_jit_eval_ragged(*rag, a["res_dev"], a["J_dev"])
        if entry == "toa_lm_run":
            return lib.toa_lm_run(h, self.capi.MODEL_DENSE_ROW, self.capi.F64, N, ITEMS, batch, d, x, po, pr, cnt)
        if entry == "toa_jit_lm_run":
            return lib.toa_jit_lm_run(*uni, po, pr, cnt)
        if entry == "toa_jit_lm_run_split":
            return lib.toa_jit_lm_run_split(h, res, ITEMS, batch, d, x, po, pr, cnt, 0)
        if entry == "toa_jit_lm_begin":
            return lib.toa_jit_lm_begin(h, res, ITEMS, batch, d, x, po, pr, st)
        if entry == "toa_jit_lm_step":
            return lib.toa_jit_lm_step(h, res, ITEMS, batch, d, x, po, pr, cnt, st, self.active.data_ptr())
        if entry == "toa_jit_lm_stop":
            return lib.toa_jit_lm_stop(h, res, ITEMS, batch, d, x, po, pr, cnt, st, self.stop_request.data_ptr())
        if entry == "toa_jit_gd_run":
            return lib.toa_jit_gd_run(*uni, po, C.byref(self.gd), pr, cnt)
        if entry == "toa_ba_run":
            return lib.toa_ba_run(h, self.capi.F64, 1, ITEMS, batch, d, x, po, pr, cnt)
        if entry == "toa_ba_lists_run":
            return lib.toa_ba_lists_run(h, self.capi.F64, 1, 2, ITEMS, batch, d, ids, ids, d, x, po, pr, cnt, 0.0)
        raise KeyError(entry)

    def refused(self, entry, o, r, text, code=E_ARG, **kw):
        rc = self.call(entry, o, r, **kw)
        assert rc == code, (entry, rc, self.lib.toa_last_error())
        assert self.lib.toa_last_error().decode() == text, entry

    def refuses(self, entry, text, code=E_ARG, **kw):
        """... with the entry's own well-formed options and results"""
        self.refused(entry, self.options(entry), self.results(), text, code=code, **kw)


@pytest.fixture(scope="module")
def env(ta):
    e = Env(ta)
    yield e
    torch.cuda.synchronize()
    e.residual.close()
    e.cost.close()
    e.large.close()
    e.ctx.close()


@pytest.mark.parametrize("entry", RUN)
def test_missing_final_cost(env, entry):
    r = env.results()
    r.final_cost = None
    env.refused(entry, env.options(entry), r, f"{ENTRIES[entry][0]}: stop_reason, num_iters and final_cost outputs are required")


@pytest.mark.parametrize("entry", RUN)
def test_history_stride_one_short(env, entry):
    r = env.results()
    r.errs, r.hist_stride = env.errs.data_ptr(), MAX_ITERS + 1
    env.refused(entry, env.options(entry), r, f"{ENTRIES[entry][0]}: hist_stride must be >= max_iters + 2")


@pytest.mark.parametrize("entry", [e for e in RUN if e not in STEPPING])
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


@pytest.mark.parametrize("entry", RUN)
def test_solver_type_not_served(env, entry):
    o = env.options(entry)
    o.solver_type = 0 if entry in GD else 2
    env.refused(entry, o, env.results(), f"{ENTRIES[entry][0]}: {ENTRIES[entry][1]}")


@pytest.mark.parametrize("entry", RUN)
def test_null_options(env, entry):
    env.refused(entry, None, env.results(), ENTRIES[entry][2])


@pytest.mark.parametrize("entry", RUN)
def test_empty_batch(env, entry):
    o, r = env.options(entry), env.results()
    assert env.call(entry, o, r, batch=0) == 0, (entry, env.lib.toa_last_error())
    if entry in JIT:
        assert env.call(entry, o, r, batch=0, null_data=True) == 0, (entry, env.lib.toa_last_error())
    else:
        text = "DenseRow: data pointer is null" if entry == "toa_lm_run" else f"{entry}: null pointer"
        env.refused(entry, o, r, text, batch=0, null_data=True)


# ---- the prior, ragged, seam and Eval entries of a run-time model: code and exact text, and which of two failing conditions is
# ---- reported when both hold; every one is decided before anything is built or launched ----
E_UNSUPPORTED = -4
LARGE_N = ("a model compiled with toa_jit_spec::large_n runs on the launch-per-phase pipeline through toa_jit_lm_run, toa_jit_accumulate "
           "and toa_jit_eval only: ")
LARGE_N_PRIOR = LARGE_N + "a Gaussian prior (toa_jit_*_prior) is not built for it"
LARGE_N_RAGGED = LARGE_N + "ragged batches (toa_jit_*_ragged) are not built for it"
COST_ON_LM = ("a scalar cost model (TOA_JIT_COST / TOA_JIT_COST_GRAD) has no residuals for LM / GN (optimize.h:41-56 throws): run it with "
              "solver_type = 2 through toa_jit_gd_run")
COST_WITH_PRIOR = ("a Gaussian prior is a block of residuals; a scalar cost model (TOA_JIT_COST / TOA_JIT_COST_GRAD, gradient descent) has "
                   "none to add it to")
RESIDUAL_ON_GD = ("GradientDescent needs a scalar cost model (TOA_JIT_COST / TOA_JIT_COST_GRAD; optimize.h:59-75 throws for a residual "
                  "function)")
FLAGS_TEXT = "unknown bits in flags (TOA_RAGGED_KEEP_ORDER is the only one)"
RAGGED_SHAPE = "bad shape (0 <= max_items <= total_items, 0 <= P < 2^31)"
COST_LOSS = "a scalar cost has no residuals to robustify: clear the handle's loss (toa_set_loss)"
COST_HESSIAN = "a scalar cost model forms no Hessian (SolverGD, gd.h): H_dev must be NULL"
EVAL_LOSS = "Eval is the plain function, its residuals and their Jacobian: clear the handle's loss (toa_set_loss)"
EVAL_NEITHER = "neither res_dev nor J_dev: at least one output must be non-NULL"
EVAL_ALIGN = "res_dev / J_dev must be aligned to the scalar type"
HUBER = 2   # TOA_LOSS_HUBER
WITH_FLAGS = ("toa_jit_lm_run_ragged", "toa_jit_lm_run_ragged_prior", "toa_jit_gd_run_ragged")


def rows_text(entry, rows):
    return f"{entry}: prior rows must be 0 (the diagonal form) or 1 .. num_params = {N}, not {rows}"


def eval_cost_text(entry):
    return (f"{entry}: a scalar cost model (TOA_JIT_COST / TOA_JIT_COST_GRAD) has no residual rows: {entry.replace('eval', 'accumulate')} "
            "already is Eval of a scalar function, its value and its gradient row (auto_diff.h:14-138)")


def null_pointer_text(entry):
    return f"{entry}: bad shape or null pointer" if entry in SEAM else f"{entry}: null pointer"


@contextlib.contextmanager
def handle_loss(env):
    """A loss on the handle for the length of a `with` block, cleared again whatever happens inside."""
    assert env.lib.toa_set_loss(env.ctx.h, HUBER, 1.0) == 0
    try:
        yield
    finally:
        assert env.lib.toa_set_loss(env.ctx.h, 0, 0.0) == 0


@pytest.mark.parametrize("what", ["handle", "model"])
@pytest.mark.parametrize("entry", FORMS)
def test_null_handle_or_model(env, entry, what):
    kw = dict(handle=False) if what == "handle" else dict(model=None)
    env.refuses(entry, f"{entry}: null handle / model", **kw)
    env.refuses(entry, f"{entry}: null handle / model", prior=None, items=0, max_items=9, **kw)   # (before the prior and the shape)


@pytest.mark.parametrize("entry", PRIOR)
def test_prior_refusals(env, entry):
    env.refuses(entry, f"{entry}: null prior", prior=None)
    env.refuses(entry, rows_text(entry, 4), prior=env.prior(rows=4))
    env.refuses(entry, rows_text(entry, -1), prior=env.prior(rows=-1))
    env.refuses(entry, f"{entry}: null prior mu_dev / W_dev", prior=env.prior(mu=False))
    env.refuses(entry, f"{entry}: {COST_WITH_PRIOR}", code=E_UNSUPPORTED, model="cost")


@pytest.mark.parametrize("entry", PRIOR)
def test_prior_refusals_which_comes_first(env, entry):
    env.refuses(entry, f"{entry}: null prior", prior=None, model="cost")
    env.refuses(entry, f"{entry}: {COST_WITH_PRIOR}", code=E_UNSUPPORTED, model="cost", prior=env.prior(rows=4))
    env.refuses(entry, rows_text(entry, 4), prior=env.prior(rows=4, mu=False))
    # the prior is judged before the large-n route, the flags and the shape
    env.refuses(entry, f"{entry}: null prior mu_dev / W_dev", prior=env.prior(mu=False), model="large")
    if entry in RAGGED:
        kw = dict(flags=2) if entry in WITH_FLAGS else {}
        env.refuses(entry, f"{entry}: null prior mu_dev / W_dev", prior=env.prior(mu=False), max_items=9, **kw)
    else:
        env.refuses(entry, f"{entry}: null prior mu_dev / W_dev", prior=env.prior(mu=False), items=0)


@pytest.mark.parametrize("entry", ["toa_jit_lm_run", "toa_jit_lm_run_ragged"])
def test_cost_model_on_an_lm_entry(env, entry):
    """(the prior entries refuse a cost model for its prior first: test_prior_refusals)"""
    env.refuses(entry, f"{entry}: {COST_ON_LM}", model="cost")
    if entry in RAGGED:
        env.refuses(entry, f"{entry}: {COST_ON_LM}", model="cost", flags=2)
        env.refuses(entry, f"{entry}: {COST_ON_LM}", model="cost", max_items=9)
    else:
        env.refuses(entry, f"{entry}: {COST_ON_LM}", model="cost", items=0)


@pytest.mark.parametrize("entry", GD)
def test_residual_model_on_a_gd_entry(env, entry):
    env.refuses(entry, f"{entry}: {RESIDUAL_ON_GD}", model="residual")
    if entry in RAGGED:
        env.refuses(entry, f"{entry}: {RESIDUAL_ON_GD}", model="residual", flags=2)
        env.refuses(entry, f"{entry}: {RESIDUAL_ON_GD}", model="large")   # (a large-n model is a residual model: said first)
    else:
        env.refuses(entry, f"{entry}: {RESIDUAL_ON_GD}", model="residual", items=0)
        env.refuses(entry, f"{entry}: {LARGE_N}gradient descent runs scalar cost models on the one-wavefront route", code=E_UNSUPPORTED,
                    model="large")


@pytest.mark.parametrize("entry", [e for e in RAGGED if e not in GD])
def test_large_n_model_on_a_ragged_entry(env, entry):
    """(on the ragged prior entries too: the prior itself is well-formed, and the ragged shape is judged before the run)"""
    env.refuses(entry, f"{entry}: {LARGE_N_RAGGED}", code=E_UNSUPPORTED, model="large")
    env.refuses(entry, f"{entry}: {LARGE_N_RAGGED}", code=E_UNSUPPORTED, model="large", max_items=9)
    env.refuses(entry, f"{entry}: {LARGE_N_RAGGED}", code=E_UNSUPPORTED, model="large", null=("x",))
    if entry in WITH_FLAGS:
        env.refuses(entry, f"{entry}: {FLAGS_TEXT}", model="large", flags=2)


@pytest.mark.parametrize("entry", ["toa_jit_lm_run_prior", "toa_jit_accumulate_prior"])
def test_large_n_model_on_a_prior_entry(env, entry):
    env.refuses(entry, f"{entry}: {LARGE_N_PRIOR}", code=E_UNSUPPORTED, model="large")
    env.refuses(entry, f"{entry}: {LARGE_N_PRIOR}", code=E_UNSUPPORTED, model="large", items=0)
    env.refuses(entry, f"{entry}: {LARGE_N_PRIOR}", code=E_UNSUPPORTED, model="large", null=("x",))


@pytest.mark.parametrize("entry", WITH_FLAGS)
def test_unknown_flag_bits(env, entry):
    env.refuses(entry, f"{entry}: {FLAGS_TEXT}", flags=2)
    env.refuses(entry, f"{entry}: {FLAGS_TEXT}", flags=3)   # (the known bit beside an unknown one)
    env.refuses(entry, f"{entry}: {FLAGS_TEXT}", flags=2, max_items=9)
    env.refused(entry, None, env.results(), f"{entry}: {FLAGS_TEXT}", flags=2)


@pytest.mark.parametrize("entry", RAGGED)
def test_max_items_beyond_total_items(env, entry):
    env.refuses(entry, f"{entry}: {RAGGED_SHAPE}", max_items=9)
    env.refuses(entry, f"{entry}: {RAGGED_SHAPE}", max_items=9, null=("x", "offsets"))
    if entry in RUN:
        env.refused(entry, None, env.results(), f"{entry}: {RAGGED_SHAPE}", max_items=9)
    if entry in EVAL:
        env.refuses(entry, f"{entry}: {RAGGED_SHAPE}", max_items=9, res_dev=None)


@pytest.mark.parametrize("entry", [e for e in FORMS if e not in RAGGED])
def test_no_items(env, entry):
    text = f"{entry}: bad shape or null pointer" if entry in SEAM else f"{entry}: bad shape"
    env.refuses(entry, text, items=0)
    env.refuses(entry, text, items=0, null=("x",))
    if entry in EVAL:
        env.refuses(entry, text, items=0, res_dev=None)
    if entry in RUN:
        env.refused(entry, None, None, text, items=0)


@pytest.mark.parametrize("entry", SEAM + EVAL)
def test_empty_batch_of_a_seam_or_eval(env, entry):
    """The seams judge their pointers before the empty batch returns; Eval returns first."""
    assert env.call(entry, None, None, batch=0) == 0, (entry, env.lib.toa_last_error())
    if entry in EVAL:
        assert env.call(entry, None, None, batch=0, null_data=True) == 0, (entry, env.lib.toa_last_error())
    else:
        env.refuses(entry, f"{entry}: bad shape or null pointer", batch=0, null_data=True)
    if entry == "toa_jit_eval":   # (the uniform Eval wants an output even for an empty batch; the ragged one returns before it asks)
        env.refuses(entry, f"{entry}: {EVAL_NEITHER}", batch=0, res_dev=None)
    if entry == "toa_jit_eval_ragged":
        assert env.call(entry, None, None, batch=0, res_dev=None) == 0, (entry, env.lib.toa_last_error())


@pytest.mark.parametrize("entry", FORMS)
def test_null_data_pointers(env, entry):
    env.refuses(entry, null_pointer_text(entry), null=("x",))
    if entry in RAGGED:
        env.refuses(entry, null_pointer_text(entry), null=("offsets",))
    if entry in RUN:
        env.refused(entry, env.options(entry), None, null_pointer_text(entry))


@pytest.mark.parametrize("entry", LM + GD)
def test_options_refusals_which_comes_first(env, entry):
    """Two failing conditions of the options / results at once.  The GD entries judge solver_type and max_iters before the
    empty-batch return and so before the outputs; the LM entries judge everything in check_run_args' order."""
    who = ENTRIES[entry][0]
    final_cost = f"{who}: stop_reason, num_iters and final_cost outputs are required"
    solver = f"{who}: {ENTRIES[entry][1]}"
    bad_solver = 0 if entry in GD else 2
    r = env.results()
    r.final_cost = None
    env.refused(entry, None, r, ENTRIES[entry][2])
    o = env.options(entry)
    o.solver_type = bad_solver
    env.refused(entry, o, r, solver if entry in GD else final_cost)
    o = env.options(entry)
    o.max_iters = 70000
    env.refused(entry, o, r, "max_iters out of range" if entry in GD else final_cost)
    r = env.results()
    r.errs, r.hist_stride = env.errs.data_ptr(), MAX_ITERS + 1
    o = env.options(entry)
    o.solver_type = bad_solver
    env.refused(entry, o, r, solver)
    o = env.options(entry)
    o.max_iters = 70000
    env.refused(entry, o, r, "max_iters out of range" if entry in GD else f"{who}: hist_stride must be >= max_iters + 2")
    # (the data pointers: before the LM entries' options, after the GD entries' max_iters)
    env.refused(entry, o, r, "max_iters out of range" if entry in GD else null_pointer_text(entry), null=("x",))


@pytest.mark.parametrize("entry", GD)
def test_loss_on_the_handle_gd(env, entry):
    with handle_loss(env):
        env.refuses(entry, f"{entry}: {COST_LOSS}")
        env.refuses(entry, f"{entry}: {COST_LOSS}", null=("x",))
        o = env.options(entry)
        o.max_iters = 70000
        env.refused(entry, o, env.results(), f"{entry}: {COST_LOSS}")
        o = env.options(entry)
        o.solver_type = 0
        env.refused(entry, o, env.results(), f"{entry}: {ENTRIES[entry][1]}")
        env.refused(entry, None, env.results(), ENTRIES[entry][2])


@pytest.mark.parametrize("entry", ["toa_jit_accumulate", "toa_jit_accumulate_ragged"])
def test_cost_model_on_a_seam(env, entry):
    H = env.H.data_ptr()
    env.refuses(entry, f"{entry}: {COST_HESSIAN}", model="cost", H=H)
    env.refuses(entry, f"{entry}: {COST_HESSIAN}", model="cost", H=H, null=("x",))
    env.refuses(entry, f"{entry}: bad shape or null pointer", model="cost", want_grad=1)
    shape = dict(max_items=9) if entry in RAGGED else dict(items=0)
    shape_text = f"{entry}: {RAGGED_SHAPE}" if entry in RAGGED else f"{entry}: bad shape or null pointer"
    env.refuses(entry, f"{entry}: {COST_HESSIAN}", model="cost", H=H, **shape)
    with handle_loss(env):
        env.refuses(entry, f"{entry}: {COST_LOSS}", model="cost")
        env.refuses(entry, f"{entry}: {COST_HESSIAN}", model="cost", H=H)
        env.refuses(entry, f"{entry}: {COST_LOSS}", model="cost", **shape)
    env.refuses(entry, shape_text, model="cost", **shape)


@pytest.mark.parametrize("entry", SEAM)
def test_want_grad_without_its_outputs(env, entry):
    g, H = env.g.data_ptr(), env.H.data_ptr()
    env.refuses(entry, f"{entry}: bad shape or null pointer", want_grad=1, H=H)
    env.refuses(entry, f"{entry}: bad shape or null pointer", want_grad=1, g=g)
    with handle_loss(env):   # (a residual model's seam takes the handle's loss: what is refused is still the pointer)
        env.refuses(entry, f"{entry}: bad shape or null pointer", want_grad=1, H=H)


@pytest.mark.parametrize("entry", EVAL)
def test_eval_refusals(env, entry):
    env.refuses(entry, eval_cost_text(entry), model="cost")
    env.refuses(entry, f"{entry}: {EVAL_NEITHER}", res_dev=None)
    env.refuses(entry, f"{entry}: {EVAL_NEITHER}", res_dev=None, null=("x",))
    env.refuses(entry, f"{entry}: {EVAL_ALIGN}", res_dev=env.res_out.data_ptr() + 1)
    env.refuses(entry, f"{entry}: {EVAL_ALIGN}", J_dev=env.J_out.data_ptr() + 1)
    env.refuses(entry, f"{entry}: null pointer", res_dev=env.res_out.data_ptr() + 1, null=("x",))
    shape = dict(max_items=9) if entry in RAGGED else dict(items=0)
    with handle_loss(env):
        env.refuses(entry, f"{entry}: {EVAL_LOSS}")
        env.refuses(entry, eval_cost_text(entry), model="cost")
        env.refuses(entry, f"{entry}: {EVAL_LOSS}", res_dev=None, **shape)


# ---- the routing refusals of the compiled-in entries (toa_lm_run / _run_split / _begin / _stop, toa_accumulate and the two
# ---- per-element helpers): code and exact text; every one is decided before anything is launched ----
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
