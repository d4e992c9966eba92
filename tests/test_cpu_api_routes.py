"""The route table of tinyopt_amd/api.py, pinned on the CPU: for every combination of model family, options, call arguments and entry
point, either the refusal (exception type and full text) or the library calls the entry makes — each with its entry name, argument
count, integer / float argument values, which pointer arguments are NULL, and the pods handed by reference, field by field.  A pointer
that is the handle, the compiled model, x or one of the model's own tensors is recorded by that name, so an argument order is pinned too.

Nothing here needs a GPU: the context's ``lib`` records every call and returns 0, x wraps a CPU tensor and reports ``is_cuda``, the models
are assembled from CPU tensors (the mixins' own ``with_loss`` / ``with_prior`` / ``with_bounds`` run as they are).

The expected table, tests/golden/api_routes.json, is recorded by this file from the commit BEFORE a change of api.py (the file names
it), never from the code under test:  API_ROUTES_RECORD=<path> python -m pytest tests/test_cpu_api_routes.py  in a tree that holds
that commit's tinyopt_amd/.  Distinct outcomes and distinct pods are stored once, one per line; a row of the table is (entry point,
family) -> the outcome indices of the inner walk, in the order of ``INNER[entry]``."""
import ctypes as C
import itertools
import json
import os

import torch

from tinyopt_amd import _capi, api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_routes.json")
RECORD = os.environ.get("API_ROUTES_RECORD")
P = 3


# ---------------------------------------------------------------------------------------------------------------- stand-ins
def _is_ptr_type(t) -> bool:
    return t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents")


def _ptr(v, names) -> str:
    return "NULL" if not v else names.get(v, "ptr")


def _pod(s: C.Structure, names) -> dict:
    d = {"pod": type(s).__name__}
    for name, typ in s._fields_:
        v = getattr(s, name)
        if name.startswith("_") or isinstance(v, C.Array):
            continue
        d[name] = _ptr(v, names) if _is_ptr_type(typ) else v
    return d


def _arg(v, typ, names):
    if _is_ptr_type(typ):
        if hasattr(v, "_obj"):                     # byref(pod)
            return _pod(v._obj, names) if isinstance(v._obj, C.Structure) else "ptr"
        return _ptr(v.value if isinstance(v, C.c_void_p) else v, names)
    if not isinstance(v, (int, float)) or isinstance(v, bool):   # (ctypes refuses it: ArgumentError)
        raise TypeError(f"{v!r} where the entry takes a number")
    return float(v) if typ in (C.c_float, C.c_double) else int(v)


class RecordingLib:
    """Every attribute is a library entry that records its call and returns 0.  ``names``: address -> the name it is recorded by."""

    def __init__(self):
        self.calls, self.names = [], {}

    def __getattr__(self, name):
        if name not in _capi.PROTOTYPES:
            raise AttributeError(name)
        argtypes = _capi.PROTOTYPES[name][1]

        def entry(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for a prototype of {len(argtypes)}"
            self.calls.append([name, len(args)] + [_arg(a, t, self.names) for a, t in zip(args, argtypes)])
            return 0
        return entry


class StubContext:
    device = 0

    def __init__(self):
        self.lib, self.h = RecordingLib(), C.c_void_p(0x1000)


class CudaLike:
    """A CPU tensor that says it is on the GPU; everything else is the tensor's."""
    is_cuda = True

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return getattr(self._t, name)


def _bare(cls, **attrs):
    o = object.__new__(cls)
    o.__dict__.update(attrs)
    return o


F64 = torch.float64
_KEEP = []   # (residuals are kept for the life of the module: their __del__ would call the recording library)


def _residual(kind="residual", n=3, diff="ad", large_n=False):
    r = _bare(api.JitResidual, ctx=StubContext(), n=n, kR=1, kD=2, kH=0, dtype=F64, manifold="euclid", kind=kind, diff=diff, diff_h=0.0,
              large_n=large_n, xdim=n, _h=C.c_void_p(0x2000))
    _KEEP.append(r)
    return r


def _jit(**kw):
    r = _residual(**kw)
    return _bare(api.JitModel, res=r, P=P, items=4, n=r.n, dtype=F64, xdim=r.n, m=4, packed=torch.ones(P, 8, dtype=F64))


def _ragged(**kw):
    r = _residual(**kw)
    off = torch.tensor([0, 2, 2, 7])
    return _bare(api.RaggedJitModel, res=r, P=P, n=r.n, xdim=r.n, dtype=F64, total_items=7, max_items=5, offsets_host=off, offsets=off,
                 data=torch.ones(7, 2, dtype=F64), header=None)


def _extras(make, which):
    m = make()
    mu, W = torch.zeros(P, m.n, dtype=F64), torch.ones(P, m.n, dtype=F64)
    if which in ("prior", "both"):
        m = m.with_prior(mu, W)
    if which in ("bounds", "both"):
        m = m.with_bounds(mu - 1, None)
    if which == "loss":
        m = m.with_loss("huber", 1.5)
    return m


def _ba():
    return _bare(api.BundleAdjustment, P=P, ncam=2, npts=4, dtype=F64, n=24, m=16, xdim=36, packed=torch.ones(P, 32, dtype=F64))


def _ba_lists():
    i32 = lambda: torch.ones(P, 5, dtype=torch.int32)  # noqa: E731
    return _bare(api.BundleAdjustmentLists, P=P, ncam=2, npts=4, nobs=5, dtype=F64, n=24, m=10, xdim=36, intr=torch.ones(P, 4, dtype=F64),
                 obs_cam=i32(), obs_pt=i32(), obs_uv=torch.ones(P, 5, 2, dtype=F64))


FAMILIES = {
    "DenseRow": lambda: _bare(api.DenseRow, packed=torch.ones(64, dtype=F64), n=3, m=5, P=P, dtype=F64),
    "DenseRow+loss": lambda: _bare(api.DenseRow, packed=torch.ones(64, dtype=F64), n=3, m=5, P=P, dtype=F64).with_loss("cauchy", 2.0),
    "DenseRowNatural": lambda: _bare(api.DenseRowNatural, packed=torch.ones(P, 70 * 80 + 80, dtype=F64), n=70, m=80, P=P, dtype=F64),
    "BundleAdjustment": _ba,
    "BundleAdjustmentLists": _ba_lists,
    "Jit residual": _jit,
    "Jit accumulate": lambda: _jit(kind="accumulate"),
    "Jit cost": lambda: _jit(kind="cost"),
    "Jit residual central": lambda: _jit(diff="central"),
    "Jit cost central": lambda: _jit(kind="cost", diff="central"),
    "Jit residual large_n": lambda: _jit(n=70, large_n=True),
    "Jit accumulate large_n": lambda: _jit(kind="accumulate", n=70, large_n=True),
    "Jit residual+prior": lambda: _extras(_jit, "prior"),
    "Jit residual+bounds": lambda: _extras(_jit, "bounds"),
    "Jit residual+prior+bounds": lambda: _extras(_jit, "both"),
    "Jit residual+loss": lambda: _extras(_jit, "loss"),
    "Ragged residual": _ragged,
    "Ragged residual+prior": lambda: _extras(_ragged, "prior"),
    "Ragged residual+bounds": lambda: _extras(_ragged, "bounds"),
    "Ragged residual+prior+bounds": lambda: _extras(_ragged, "both"),
    "Ragged cost": lambda: _ragged(kind="cost"),
}


def _options(name):
    o = api.Options()
    if name == "GradientDescent":
        o.solver_type = api.Options.GradientDescent
    elif name == "GradientDescent+stop_callback":
        o.solver_type = api.Options.GradientDescent
        o.stop_callback = lambda err, dx2, g2: False
    elif name == "stop_callback":
        o.stop_callback = lambda err, dx2, g2: False
    elif name == "max_duration_ms":
        o.max_duration_ms = 5.0
    elif name == "log.enable":
        o.log.enable = True
    return o


OPTIONS = ["default", "GradientDescent", "GradientDescent+stop_callback", "stop_callback", "max_duration_ms", "log.enable"]
METHODS = ["forward", "central", "fast_central", "no_such_method"]
# entry point -> the axes of its inner walk (each a list of labels), walked as itertools.product in this order
INNER = {
    "Optimize": [OPTIONS, ["splits=None", "splits=0", "splits=4"], ["out=None", "out=given"], ["keep_order=False", "keep_order=True"],
                 ["capturing=False", "capturing=True"]],
    "Optimizer": [OPTIONS],
    "accumulate": [["want_grad=True", "want_grad=False"]],
    "Eval": [["jac=True", "jac=False"]],
    "CalculateJac": [["-"]],
    "CheckGradient": [METHODS],
}


# ---------------------------------------------------------------------------------------------------------------- one cell
def _shape(t):
    return None if t is None else list(t.shape)


def _name_pointers(ctx, cost, x) -> None:
    """The addresses an argument list is expected to carry, by name (everything an entry allocates itself stays "ptr")."""
    names = ctx.lib.names
    names[ctx.h.value], names[x.data_ptr()] = "handle", "x"
    for attr in ("packed", "data", "offsets", "header", "intr", "obs_cam", "obs_pt", "obs_uv"):
        if isinstance(cost.__dict__.get(attr), torch.Tensor):
            names[getattr(cost, attr).data_ptr()] = attr
    if "res" in cost.__dict__:
        names[cost.res._h.value] = "model"
    for attr, parts in (("prior", ("mu", "W")), ("bounds", ("lo", "hi"))):
        for part, t in zip(parts, cost.__dict__.get(attr) or ()):
            names[t.data_ptr()] = part


def _run_cell(entry, cost, x, ctx, labels, monkeypatch):
    if entry == "Optimize":
        opt, splits, out, keep, cap = labels
        options = _options(opt)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: cap.endswith("True"))
        given = api._alloc_output(P, cost.n, options, False, "cpu") if out == "out=given" else None
        got = api.Optimize(x, cost, options, ctx=ctx, out=given, splits={"splits=None": None, "splits=0": 0, "splits=4": 4}[splits],
                           keep_order=keep.endswith("True"))
        if isinstance(got, str):
            return got
        return {"same_out": got is given, "final_hessian": _shape(got.final_hessian)}
    if entry == "Optimizer":
        opt = api.Optimizer(x, cost, _options(labels[0]), ctx=ctx)
        running = opt.Step()
        opt.stop(torch.zeros(P, dtype=torch.int32))
        return {"running": running, "final_hessian": _shape(opt.out.final_hessian)}
    if entry == "accumulate":
        return [_shape(t) for t in api.accumulate(cost, x, want_grad=labels[0].endswith("True"), ctx=ctx)]
    if entry == "Eval":
        return [_shape(t) for t in api.Eval(cost, x, jac=labels[0].endswith("True"), ctx=ctx)]
    if entry == "CalculateJac":
        return _shape(api.CalculateJac(cost, x, ctx=ctx))
    if entry == "CheckGradient":
        got = api.CheckGradient(cost, x, method=labels[0], ctx=ctx)
        return {"eps": got.eps}
    raise AssertionError(entry)


def _walk(monkeypatch):
    """{"entry | family": [outcome, ...]} over the whole cross product."""
    def stepping(x, cost, options, history, ctx):
        ctx.lib.calls.append(["-> the stepping form (_optimize_with_host_controls)", int(history)])
        return "stepping"
    monkeypatch.setattr(api, "_optimize_with_host_controls", stepping)
    table = {}
    for entry, axes in INNER.items():
        for fam, make in FAMILIES.items():
            cost = make()
            x = CudaLike(torch.ones(P, cost.xdim if hasattr(cost, "xdim") else cost.n, dtype=F64))
            row = table[f"{entry} | {fam}"] = []
            for labels in itertools.product(*axes):
                ctx = StubContext()
                _name_pointers(ctx, cost, x)
                try:
                    ret = _run_cell(entry, cost, x, ctx, labels, monkeypatch)
                    row.append({"calls": ctx.lib.calls, "returns": ret})
                except Exception as e:  # noqa: BLE001 — the refusal IS the outcome
                    row.append({"raises": type(e).__name__, "text": str(e), "calls_before": ctx.lib.calls})
    return table


def _canon(outcome) -> str:
    return json.dumps(outcome, sort_keys=True)


def _intern_pods(o, index):
    """The outcome with every pod replaced by {"pod#": its index in ``index``} (a dict canon -> position, filled here)."""
    if isinstance(o, dict):
        return {"pod#": index.setdefault(_canon(o), len(index))} if "pod" in o else {k: _intern_pods(v, index) for k, v in o.items()}
    return [_intern_pods(v, index) for v in o] if isinstance(o, list) else o


def _expand_pods(o, pods):
    if isinstance(o, dict):
        return pods[o["pod#"]] if "pod#" in o else {k: _expand_pods(v, pods) for k, v in o.items()}
    return [_expand_pods(v, pods) for v in o] if isinstance(o, list) else o


def test_route_table(monkeypatch):
    table = _walk(monkeypatch)
    axes = {k: v for k, v in INNER.items()}
    if RECORD:
        index, pods, rows = {}, {}, {}
        for key, row in table.items():
            rows[key] = [index.setdefault(_canon(_intern_pods(o, pods)), len(index)) for o in row]

        def lines(items):   # one JSON value per line: a re-recording diffs by outcome
            return "[\n" + ",\n".join(items) + "\n]"
        with open(RECORD, "w") as f:
            f.write('{"recorded_from": %s,\n"axes": %s,\n"pods": %s,\n"outcomes": %s,\n"rows": {\n%s\n}}\n' % (
                json.dumps(os.environ.get("API_ROUTES_COMMIT", "unknown")), json.dumps(axes), lines(pods), lines(index),
                ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in rows.items())))
        return
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["axes"] == axes, "the walk's axes are not the recorded ones: record the table again from the parent commit"
    assert set(table) == set(gold["rows"]), f"rows of the walk and of the table differ: {sorted(set(table) ^ set(gold['rows']))}"
    gold["outcomes"] = [_expand_pods(o, gold["pods"]) for o in gold["outcomes"]]
    bad = []
    for key, row in table.items():
        want = gold["rows"][key]
        labels = list(itertools.product(*INNER[key.split(" | ")[0]]))
        assert len(want) == len(row) == len(labels), f"{key}: {len(want)} recorded cells, {len(row)} walked"
        for lab, o, wi in zip(labels, row, want):
            if _canon(o) != _canon(gold["outcomes"][wi]):
                bad.append(f"{key} {lab}:\n    got  {_canon(o)}\n    want {_canon(gold['outcomes'][wi])}")
    assert not bad, f"{len(bad)} cells differ from the recorded table; the first:\n" + "\n".join(bad[:5])


def test_route_table_is_not_trivial():
    """(the table holds refusals and accepted calls of every entry family the walk can reach)"""
    with open(GOLDEN) as f:
        gold = json.load(f)
    names = {c[0] for o in gold["outcomes"] for c in o.get("calls", [])}
    assert len(json.dumps(gold["pods"])) < 20000 and all("pod" in p for p in gold["pods"])
    for want in ("toa_lm_run", "toa_lm_run_split", "toa_ba_run", "toa_ba_lists_run", "toa_jit_lm_run", "toa_jit_lm_run_split", "toa_jit_lm_run_prior",
                 "toa_jit_lm_run_bounds", "toa_jit_lm_run_ragged", "toa_jit_lm_run_ragged_prior", "toa_jit_lm_run_ragged_bounds", "toa_jit_gd_run",
                 "toa_jit_gd_run_ragged", "toa_accumulate", "toa_jit_accumulate", "toa_jit_accumulate_prior", "toa_jit_accumulate_bounds",
                 "toa_jit_accumulate_ragged", "toa_jit_accumulate_ragged_prior", "toa_jit_accumulate_ragged_bounds", "toa_jit_eval",
                 "toa_jit_eval_ragged", "toa_jit_check_gradient", "toa_lm_begin", "toa_lm_step", "toa_lm_stop", "toa_jit_lm_begin", "toa_jit_lm_step",
                 "toa_jit_lm_stop", "toa_set_loss", "toa_gd_options_default"):
        assert want in names, want
    assert sum(1 for o in gold["outcomes"] if "raises" in o) >= 30
