"""Shared item tables (JitResidual(..., shared_scalars=kS)) on the CPU: the stage geometry with a shared image — the
header's own RowStageGeom::make, printed by a plain host program, against the numpy restatement and, for kS = 0, against what the same
program printed from the header of the commit before (tests/golden/row_stage_geom_parent.json); the POD contracts; and the Python
routes over the recording library of tests/test_cpu_api_routes.py: the two new entries with their argument order, and every refusal's
full text."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shared_reference as sr  # noqa: E402
import test_cpu_api_routes as routes  # noqa: E402
from tinyopt_amd import _capi, api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_row_stage_geom.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_test_row_stage_geom")
COLUMNS = ["sz", "n", "kR", "kD", "kS", "compute_bound", "items2", "nbuf", "items1", "ps", "pss", "rsp", "bytes", "table_off"]


@pytest.fixture(scope="module")
def header_rows():
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120, check=True)
    rows = [[int(v) for v in line.replace(":", " ").split()] for line in r.stdout.splitlines()]
    assert len(rows) == 2 * 7 * 3 * 3 * 8 * 2 and all(len(row) == len(COLUMNS) for row in rows)
    return rows


def test_geometry_equals_the_restatement(header_rows):
    for row in header_rows:
        sz, n, kR, kD, kS, cb = row[:6]
        g = sr.row_stage_geom(sz, n, kR, kD, kS, bool(cb))
        assert [g[k] for k in COLUMNS[6:]] == row[6:], (row[:6], g, row[6:])
        # what the pass relies on: both strides 16 bytes x an odd number (or no image), the regions inside the stage
        for stride, width in ((g["ps"], kD), (g["pss"], kS)):
            assert (stride == 0) == (width == 0) and stride >= width and (stride * sz) % 16 == 0 and (width == 0 or (stride * sz // 16) & 1)
        for it, regions in ((g["items2"], g["nbuf"]), (g["items1"], 1)):
            if it:
                assert regions * max(it * (g["ps"] + g["pss"]) * sz, ((it * kR + 3) & ~3) * g["rsp"] * sz) <= g["bytes"] and 1 <= it <= 64 // kR


def test_geometry_without_a_table_is_the_parents(header_rows):
    with open(os.path.join(ROOT, "tests", "golden", "row_stage_geom_parent.json")) as f:
        gold = json.load(f)
    assert gold["columns"] == COLUMNS
    mine = [row for row in header_rows if row[4] == 0]
    assert len(mine) == len(gold["rows"]) == 2 * 7 * 3 * 3 * 2
    assert mine == gold["rows"]
    assert all(row[10] == 0 for row in mine)   # (no shared image)


def test_the_table_shrinks_the_super_step_where_it_must(header_rows):
    """The cells tests/test_gpu_shared.py relies on, read from the HEADER's own output (and, where the grid does not hold the cell, from
    the restatement that the test above ties to it): a 51-column fp64 table and a 130-column one leave fewer than 64 items per
    super-step; a 5-column fp32 one does not; the 1 KiB pieces of a 32-item image of 48-byte rows end in a partial piece."""
    hdr = {tuple(r[:6]): dict(zip(COLUMNS[6:], r[6:])) for r in header_rows}   # (sz, n, kR, kD, kS, compute_bound)
    assert hdr[(8, 50, 1, 1, 51, 1)]["items1"] == 36 and hdr[(8, 50, 1, 1, 51, 1)]["items2"] < 36
    assert hdr[(4, 63, 1, 1, 130, 1)]["items1"] < 64 and hdr[(8, 4, 2, 1, 130, 1)]["items1"] < 32
    g = hdr[(4, 4, 2, 1, 5, 1)]
    assert (g["items1"], g["items2"]) == (32, 32) and g["pss"] * 4 == 48 and (32 * 48) % 1024 != 0
    g = hdr[(4, 1, 1, 0, 3, 1)]
    assert (g["items1"], g["items2"], g["ps"]) == (64, 64, 0)
    assert sr.row_stage_items(50, 1, 51, np.float64)[0] == 36 and sr.row_stage_items(63, 3, 130, np.float32)[0] < 64
    assert sr.row_stage_items(4, 3, 130, np.float64, kR=2)[0] < 32
    # ggn_reference's restatement is the kS = 0, kR = 1 case of this one
    import ggn_reference as gr
    for n, kD, dt in ((12, 13, np.float32), (50, 51, np.float32), (50, 51, np.float64), (63, 64, np.float64), (1, 4, np.float32)):
        assert gr.row_stage_items(n, kD, dt) == sr.row_stage_items(n, kD, 0, dt)


def test_pod_contracts():
    S = _capi.ToaJitSpec
    assert C.sizeof(S) == 8 * 4 + C.sizeof(C.c_void_p) + 6 * 4
    assert S.x_scalars.offset == 28 and S.plus_body.offset == 32 and S.diff.offset == 40 and S.diff_h.offset == 44
    assert S.reserved.offset == 48 and S.reserved.size == 16
    tail = _capi._ToaJitSpecTail
    assert S._tail.offset + tail.large_n.offset == 48 and S._tail.offset + tail.shared_scalars.offset == 52
    spec = S()
    spec.shared_scalars = 7
    assert list(spec.reserved) == [0, 7, 0, 0] and spec.large_n == 0
    spec.large_n = 1
    assert list(spec.reserved) == [1, 7, 0, 0]
    assert C.sizeof(_capi.ToaShared) == 32 and _capi.ToaShared.table_dev.offset == 0 and _capi.ToaShared.rows.offset == 8
    assert _capi.ABI_VERSION == 7
    hdr = open(os.path.join(ROOT, "include", "tinyopt_amd.h")).read()
    assert re.search(r"#define TOA_ABI_VERSION 7\b", hdr) and "int32_t reserved[4];" in hdr and "int32_t shared_scalars;" in hdr
    assert "typedef struct toa_shared { const void* table_dev; int64_t rows; int32_t reserved[4]; } toa_shared;" in hdr
    for name in ("toa_jit_lm_run_shared", "toa_jit_accumulate_shared"):
        assert name in _capi.PROTOTYPES and name + "(" in hdr
    assert len(_capi.PROTOTYPES["toa_jit_lm_run_shared"][1]) == 12 and len(_capi.PROTOTYPES["toa_jit_accumulate_shared"][1]) == 14


# ---- the Python routes ----------------------------------------------------------------------------------------------------------------
P, F64 = routes.P, routes.F64


def _shared(kind="residual", diff="ad", which=None):
    m = routes._jit(kind=kind, diff=diff)
    m.res.kS = 2
    m.shared = torch.ones(4, 2, dtype=F64)
    return routes._extras(lambda: m, which) if which else m


def _cell(fn, cost):
    ctx = routes.StubContext()
    x = routes.CudaLike(torch.ones(P, cost.n, dtype=F64))
    routes._name_pointers(ctx, cost, x)
    ctx.lib.names[cost.shared.data_ptr()] = "table"
    ret = fn(x, ctx)
    return ctx.lib.calls, ret


SHARED_POD = {"pod": "ToaShared", "table_dev": "table", "rows": 4}


@pytest.mark.parametrize("which", [None, "loss", "prior", "bounds", "both"])
def test_optimize_and_accumulate_route_to_the_shared_entries(which):
    cost = _shared(which=which)
    calls, out = _cell(lambda x, ctx: api.Optimize(x, cost, api.Options(), ctx=ctx), cost)
    run = [c for c in calls if c[0] != "toa_set_loss"]
    assert len(run) == 1 and run[0][0] == "toa_jit_lm_run_shared" and run[0][1] == 12
    a = run[0][2:]
    assert a[:4] == ["handle", "model", 4, P] and a[4] == "packed" and a[5] == SHARED_POD and a[6] == "x"
    want_bounds, want_prior = which in ("bounds", "both"), which in ("prior", "both")
    assert (a[7] == "NULL") != want_bounds and (a[8] == "NULL") != want_prior
    if want_bounds:
        assert a[7]["pod"] == "ToaBounds" and a[7]["lo_dev"] == "lo" and a[7]["hi_dev"] == "hi"
    if want_prior:
        assert a[8]["pod"] == "ToaPrior" and a[8]["mu_dev"] == "mu" and a[8]["W_dev"] == "W" and a[8]["rows"] == 0
    assert a[9]["pod"] == "ToaOptions" and a[10]["pod"] == "ToaResults" and a[11] == "ptr"
    loss = [c for c in calls if c[0] == "toa_set_loss"]
    assert len(loss) == 1 and (loss[0][3] != 0) == (which == "loss")
    assert list(out.final_hessian.shape) == [P, cost.n, cost.n]
    for want_grad in (True, False):
        calls, got = _cell(lambda x, ctx: api.accumulate(cost, x, want_grad=want_grad, ctx=ctx), cost)
        run = [c for c in calls if c[0] != "toa_set_loss"]
        assert len(run) == 1 and run[0][0] == "toa_jit_accumulate_shared" and run[0][1] == 14
        a = run[0][2:]
        assert a[:4] == ["handle", "model", 4, P] and a[4] == "packed" and a[5] == SHARED_POD and a[6] == "x"
        assert (a[7] == "NULL") != want_bounds and (a[8] == "NULL") != want_prior and a[9] == int(want_grad)
        assert [v == "NULL" for v in a[10:]] == [not want_grad, not want_grad, False, False]


def test_gauss_newton_routes_the_same_way():
    cost = _shared(kind="accumulate")
    o = api.Options()
    o.solver_type = api.Options.GaussNewton
    calls, _ = _cell(lambda x, ctx: api.Optimize(x, cost, o, ctx=ctx), cost)
    assert [c[0] for c in calls if c[0] != "toa_set_loss"] == ["toa_jit_lm_run_shared"]
    assert [c for c in calls if c[0] == "toa_jit_lm_run_shared"][0][11]["solver_type"] == 1


PREFIX = ("a model with a shared item table (shared_scalars > 0) runs in the uniform one-launch form through Optimize (LM / GN) and "
          "accumulate only: ")
NO_ROWS = "no {} (its kernels read replicated items: bind the table copied into every problem's items)"


def _refused(fn, cost, text):
    with pytest.raises(ValueError) as e:
        _cell(fn, cost)
    assert str(e.value) == text, str(e.value)


def test_every_refusal_of_a_bound_shared_model():
    cost = _shared()
    opt = routes._options
    host = "no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)"
    for name in ("stop_callback", "max_duration_ms", "log.enable"):
        _refused(lambda x, ctx: api.Optimize(x, cost, opt(name), ctx=ctx), cost, PREFIX + host)
    _refused(lambda x, ctx: api.Optimize(x, cost, opt("GradientDescent"), ctx=ctx), cost, PREFIX + "no GradientDescent")
    _refused(lambda x, ctx: api.Optimize(x, cost, opt("GradientDescent+stop_callback"), ctx=ctx), cost, PREFIX + "no GradientDescent")
    lb = api.Options()
    lb.solver_type = api.Options.LBFGS
    _refused(lambda x, ctx: api.Optimize(x, cost, lb, ctx=ctx), cost, PREFIX + "no L-BFGS")
    for splits in (0, 4):
        _refused(lambda x, ctx: api.Optimize(x, cost, api.Options(), ctx=ctx, splits=splits), cost, PREFIX + "no row-split form (splits)")
    _refused(lambda x, ctx: api.Optimize(x, cost, api.Options(), ctx=ctx, keep_order=True), cost,
             "keep_order is the queue order of a ragged batch (JitResidual.bind_ragged)")
    _refused(lambda x, ctx: api.Optimizer(x, cost, api.Options(), ctx=ctx), cost, PREFIX + "no stepping form (Optimizer)")
    _refused(lambda x, ctx: api.Eval(cost, x, ctx=ctx), cost, PREFIX + NO_ROWS.format("Eval"))
    _refused(lambda x, ctx: api.CalculateJac(cost, x, ctx=ctx), cost, PREFIX + NO_ROWS.format("CalculateJac"))
    _refused(lambda x, ctx: api.CheckGradient(cost, x, ctx=ctx), cost,
             PREFIX + 'no CheckGradient (compare accumulate of a kind="accumulate" body with accumulate of its residuals under diff="central", '
                      'both with the table)')
    # nothing reached the library in any of them
    for fn in (lambda x, ctx: api.Eval(cost, x, ctx=ctx), lambda x, ctx: api.Optimizer(x, cost, api.Options(), ctx=ctx)):
        ctx = routes.StubContext()
        with pytest.raises(ValueError):
            fn(routes.CudaLike(torch.ones(P, cost.n, dtype=F64)), ctx)
        assert ctx.lib.calls == []


def test_bind_takes_the_table_where_it_belongs():
    res = routes._residual()
    res.kD, res.kS = 1, 2
    data = routes.CudaLike(torch.ones(P, 4, 1, dtype=F64))
    table = torch.ones(4, 2, dtype=F64)
    m = res.bind(data, shared=table)
    assert m.shared is not None and m.shared.data_ptr() == table.data_ptr() and (m.P, m.items, m.m) == (P, 4, 4)
    assert m.with_loss("huber", 1.0).shared is m.shared
    assert m.with_prior(torch.zeros(P, 3, dtype=F64), torch.ones(P, 3, dtype=F64)).with_bounds(None, torch.ones(P, 3, dtype=F64)).shared is m.shared
    with pytest.raises(ValueError, match=r"^bind: a model with shared_scalars = 2 needs shared=, the batch's \[items, 2\] table$"):
        res.bind(data)
    for bad, text in ((torch.ones(5, 2, dtype=F64), r"^bind: shared must be an \[items, shared_scalars\] = \[4, 2\] tensor, not \[5, 2\]$"),
                      (torch.ones(4, 3, dtype=F64), r"= \[4, 2\] tensor, not \[4, 3\]$"), ("table", r"tensor, not str$"),
                      (torch.ones(4, 2, dtype=torch.float32), r"^bind: shared must have the model's dtype torch.float64 on the data's device cpu, not torch.float32 on cpu$")):
        with pytest.raises(ValueError, match=text):
            res.bind(data, shared=bad)
    with pytest.raises(ValueError) as e:
        res.bind_ragged(torch.ones(7, 1, dtype=F64), counts=[2, 0, 5])
    assert str(e.value) == PREFIX + "no ragged batches (bind_ragged)"
    plain = routes._residual()
    with pytest.raises(ValueError, match=r"^bind: shared= is the table of a model with shared_scalars > 0; this model has none$"):
        plain.bind(routes.CudaLike(torch.ones(P, 4, 2, dtype=F64)), shared=table)


@pytest.mark.parametrize("kw,text", [
    (dict(kind="cost"), 'kind="residual", "accumulate" and "cost_ggn" take a table (the row models stage it), not kind=\'cost\''),
    (dict(kind="cost_grad"), 'kind="residual", "accumulate" and "cost_ggn" take a table (the row models stage it), not kind=\'cost_grad\''),
    (dict(kind="cost_hess"), 'kind="residual", "accumulate" and "cost_ggn" take a table (the row models stage it), not kind=\'cost_hess\''),
    (dict(manifold="se3", n=6), "Euclidean parameters only, not manifold='se3'"),
    (dict(manifold="user", x_scalars=4, plus_body=""), "Euclidean parameters only, not manifold='user'"),
    (dict(large_n=True), "no large_n"),
])
def test_the_constructor_refuses_before_it_compiles(kw, text):
    ctx = routes.StubContext()
    args = dict(n=3, item_scalars=1, shared_scalars=2, ctx=ctx)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        api.JitResidual("r[0] = s[0];", **args)
    assert str(e.value) == PREFIX + text and ctx.lib.calls == []
    for bad in (-1, 513):
        with pytest.raises(ValueError, match=r"^shared_scalars must be in 0 \.\. 512 \(0 = no shared item table\), not " + str(bad) + "$"):
            api.JitResidual("r[0] = s[0];", n=3, item_scalars=1, shared_scalars=bad, ctx=ctx)


def test_the_constructor_hands_the_field_to_the_library():
    seen = {}

    class Lib:   # (the recording library cannot name a log buffer: the three entries the constructor and the destructor call)
        def toa_model_compile_ex(self, h, spec, body, out, log, cap):
            seen["spec"], seen["body"] = bytes(spec._obj), body
            return 0

        def toa_jit_model_info(self, *a):
            return 0

        def toa_model_destroy(self, *a):
            return 0
    ctx = routes.StubContext()
    ctx.lib = Lib()
    res = api.JitResidual("r[0] = s[0] - p[0];", n=3, item_scalars=1, shared_scalars=5, ctx=ctx)
    assert res.kS == 5 and seen["body"] == b"r[0] = s[0] - p[0];"
    words = np.frombuffer(seen["spec"][48:], np.int32)
    assert list(words) == [0, 5, 0, 0] and np.frombuffer(seen["spec"][:20], np.int32).tolist() == [1, 3, 1, 1, 0]
    plain = api.JitResidual("r[0] = p[0];", n=3, item_scalars=1, ctx=ctx)
    assert plain.kS == 0 and seen["spec"][40:] == bytes(24)   # (as before: all zeros after the old fields)


def test_the_exact_case_is_exact_and_its_rows_differ():
    """The premise of tests/test_gpu_shared.py's exact sums, on the CPU: computed in float32 and in float64 the sums are equal, the
    magnitudes of every entry's terms stay below 2^24 units (so ANY order of summation is exact), and no two table rows are alike."""
    for kind, n, kR, kD, kS in (("accumulate", 1, 1, 0, 3), ("accumulate", 4, 2, 1, 5), ("accumulate", 63, 1, 3, 130), ("cost_ggn", 50, 1, 1, 51),
                                ("cost_ggn", 1, 1, 1, 1), ("cost_ggn", 4, 1, 3, 130)):
        items = 3 * 64 + 5
        data, table = sr.exact_case(kD, kS, items, 5)
        assert all(len({tuple(r) for r in table[i0:i0 + 61]}) == min(61, items - i0) for i0 in range(0, items, 7))   # (any two rows < 61 apart)
        assert kS < 5 or len({tuple(r) for r in table}) == items
        c32, g32, H32, big = sr.exact_sums(kind, n, kR, data, table, np.float32)
        c64, g64, H64, _ = sr.exact_sums(kind, n, kR, data, table, np.float64, np.float32)
        assert big < 2 ** 24 and (c32 == c64).all() and (g32 == g64).all() and (H32 == H64).all(), (kind, n, kD, kS, big)
        assert np.abs(g64).max() > 0 and np.abs(H64).max() > 0
    body = sr.exact_body("accumulate", 4, 2, 1, 5)
    assert "s[4]" in body and "p[0]" in body and sr.replicate(body, 1).count("s[") == 0 and "p[1 + (4)]" in sr.replicate(body, 1)
