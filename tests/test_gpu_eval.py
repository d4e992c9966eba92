"""Eval / CalculateJac of run-time models (toa_jit_eval; csrc/eval_rows.hpp): the residuals and the Jacobian rows of a batch,
against exact arithmetic where the problem is dyadic (tests/test_cpu_eval.py holds the premises), numpy in float64 otherwise, and
the Accumulate seam the solver uses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_reference as er  # noqa: E402
from test_gpu_jit import SE3_PRIOR, SO2_PLUS, SO2_RESIDUAL  # noqa: E402
from tinyopt_amd.api import default_context  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {np.float32: torch.float32, np.float64: torch.float64}
E_ARG, E_UNSUPPORTED = -1, -4
SENTINEL, PAD = -12345.5, 64
SEAM_TOL = {np.float32: 1e-4, np.float64: 1e-10}
_RES = {}


def _res(ta, body, **kw):
    key = (body, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _RES:
        _RES[key] = ta.JitResidual(body, **kw)
    return _RES[key]


class Guarded:
    """An output tensor with PAD sentinel scalars in front and behind."""

    def __init__(self, shape, tdt):
        self.numel = int(np.prod(shape))
        self.buf = torch.full((self.numel + 2 * PAD,), SENTINEL, dtype=tdt, device="cuda")
        self.view = self.buf[PAD:PAD + self.numel].view(*shape)

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.numel:] == SENTINEL).all())

    def numpy(self):
        return self.view.cpu().numpy()


def _eval_guarded(ta, model, x, res=True, jac=True):
    """Eval into guarded tensors -> (res or None, J or None), the sentinels checked."""
    P = x.shape[0]
    gr = Guarded((P, model.m), x.dtype) if res else None
    gj = Guarded((P, model.m, model.n), x.dtype) if jac else None
    if res:
        ta.Eval(model, x, jac=jac, res_out=gr.view, J_out=gj.view if jac else None)
    else:
        ta.CalculateJac(model, x, J_out=gj.view)
    torch.cuda.synchronize()
    assert gr is None or gr.intact(), "res: a sentinel was overwritten"
    assert gj is None or gj.intact(), "J: a sentinel was overwritten"
    return (gr.numpy() if res else None), (gj.numpy() if jac else None)


def _linear_model(ta, n, kR, items, mode, dtype, P=3):
    kw, squared = er.MODES[mode]
    data, x = er.dyadic_case(n, kR, items, P=P)
    res = _res(ta, er.linear_body(n, kR, kw["kind"], squared), n=n, item_scalars=kR * (n + 1), residuals_per_item=kR, dtype=TDT[dtype], **kw)
    model = res.bind(torch.from_numpy(data.astype(dtype)).cuda())
    fwd = er.H6 if mode == "forward" else None
    r, J = er.linear_rows(data, x, n, np.float64, squared, fwd)   # exact (tests/test_cpu_eval.py)
    return model, torch.from_numpy(x.astype(dtype)).cuda(), r.astype(dtype), J.astype(dtype)


# ---- 1. exact, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", ["accumulate", "residual", "central", "fast_central", "forward"])
@pytest.mark.parametrize("n,kR,items", er.SHAPES)
def test_exact_dyadic_rows(ta, n, kR, items, mode, dtype):
    """Linear bodies over multiples of 1/8 with h = 2^-6: res and J equal exact rational arithmetic cast to the dtype, whichever way
    the rows are differentiated (forward differences: the squared variant, column 0 reads 2 x0 + h); no byte outside the outputs
    is written.  fp64 (63, 8, 9) on Jets spills its 504 row values to scratch memory (expected: correct, slow)."""
    model, x, r, J = _linear_model(ta, n, kR, items, mode, dtype)
    rg, Jg = _eval_guarded(ta, model, x)
    assert rg.dtype == dtype and Jg.dtype == dtype and rg.shape == r.shape and Jg.shape == J.shape
    assert np.array_equal(rg, r), f"res differs in {int((rg != r).sum())} places, max {np.abs(rg - r).max()}"
    assert np.array_equal(Jg, J), f"J differs in {int((Jg != J).sum())} places, max {np.abs(Jg - J).max()}"


# ---- 2. J alone, res alone, both ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,kR,items,mode", [(3, 1, 7, "residual"), (3, 3, 70, "accumulate"), (3, 3, 70, "residual_sq"), (13, 1, 70, "central")])
def test_jacobian_alone_residuals_alone_and_both_give_the_same_bits(ta, n, kR, items, mode, dtype):
    model, x, r, J = _linear_model(ta, n, kR, items, mode, dtype)
    rb, Jb = _eval_guarded(ta, model, x)
    _, Jj = _eval_guarded(ta, model, x, res=False)
    rr, none = _eval_guarded(ta, model, x, jac=False)
    assert none is None
    assert np.array_equal(rb, r) and np.array_equal(Jb, J)
    assert np.array_equal(Jj, Jb) and np.array_equal(rr, rb)
    # the allocating forms
    r2, J2 = ta.Eval(model, x)
    r3, J3 = ta.Eval(model, x, jac=False)
    assert J3 is None and np.array_equal(r2.cpu().numpy(), r) and np.array_equal(J2.cpu().numpy(), J) and torch.equal(r3, r2)
    assert torch.equal(ta.CalculateJac(model, x), J2)


# ---- 3. many small problems, one huge problem -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,items,P,mode", [(3, 5, 5000, "accumulate"), (3, 5, 5000, "residual"), (6, 20000, 1, "accumulate"), (6, 20000, 1, "residual")])
def test_batch_scale_and_one_huge_problem(ta, n, items, P, mode):
    """Thousands of small problems (P = 5 000: one work unit per wavefront on a device of 256 compute units — the cases that give a
    wavefront a second unit are in test_waves_run_several_units_and_several_super_steps), and ONE problem of 20 000 items, which
    only a decomposition over super-steps spreads over the device: exact bodies, bit-identical rows, sentinels untouched."""
    model, x, r, J = _linear_model(ta, n, 1, items, mode, np.float32, P=P)
    rg, Jg = _eval_guarded(ta, model, x)
    assert np.array_equal(rg, r) and np.array_equal(Jg, J)
    _, Jj = _eval_guarded(ta, model, x, res=False)
    assert np.array_equal(Jj, J)


def _launch_plan(items, P, cus):
    """toa_jit_eval's decomposition (csrc/jit.hip), restated for 64 items per super-step (kR = 1, narrow rows): super-steps per unit,
    units, and the wave slots of the grid."""
    nss = (items + 63) // 64
    want = cus * 128
    spu = nss if P >= want else max(1, min(nss, nss * P // want))
    upp = (nss + spu - 1) // spu
    slots = 4 * max(1, min((P * upp + 3) // 4, cus * 16))
    return spu, P * upp, slots


@pytest.mark.parametrize("case", ["second_unit", "second_unit_manifold", "same_problem_second_unit", "range_of_steps", "whole_problem_steps",
                                  "whole_problem_steps_manifold"])
def test_waves_run_several_units_and_several_super_steps(ta, case):
    """The two loop-carried paths of eval_rows_kernel, sized from the device's compute-unit count: a wavefront that takes a SECOND
    work unit (grid-stride; x and, on a manifold, the table of Jets rebuilt when the problem changes, kept when it does not), and
    a unit of SEVERAL super-steps (the LDS region fetched into again after its image was copied out).  Exact dyadic bodies,
    bit-identical rows, sentinels untouched."""
    cus = default_context().info()["num_cus"]
    want, grid_slots = cus * 128, cus * 64
    n, items, P, mode, spu_min, same_problem = {
        # more problems of one super-step than the grid has waves: a second unit, of another problem
        "second_unit": (3, 5, grid_slots + 8 * cus + 3, "accumulate", 1, False),
        "second_unit_manifold": (3, 5, grid_slots + 8 * cus + 3, "user_manifold", 1, False),
        # ONE problem of more super-steps than the grid has waves: a second unit of the SAME problem
        "same_problem_second_unit": (3, 64 * (grid_slots + 8 * cus) + 3, 1, "residual", 1, True),
        # a quarter of the wanted units as problems of twelve super-steps: ranges of three super-steps, two units per wave
        "range_of_steps": (6, 64 * 12 - 7, want // 4 + 1, "residual", 3, False),
        # as many problems as wanted units: a unit is a whole problem of three super-steps, two units per wave
        "whole_problem_steps": (3, 130, want + 5, "accumulate", 3, False),
        "whole_problem_steps_manifold": (3, 130, want + 5, "user_manifold", 3, False),
    }[case]
    spu, units, slots = _launch_plan(items, P, cus)
    assert spu == spu_min and units > slots, "the case does not reach the path it is there for on this device"
    assert (P == 1) == same_problem
    model, x, r, J = _linear_model(ta, n, 1, items, mode, np.float32, P=P)
    rg, Jg = _eval_guarded(ta, model, x)
    assert np.array_equal(rg, r), f"res differs in {int((rg != r).sum())} places"
    assert np.array_equal(Jg, J), f"J differs in {int((Jg != J).sum())} places"
    rr, _ = _eval_guarded(ta, model, x, jac=False)
    assert np.array_equal(rr, r)


# ---- 4. a transcendental body -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["residual", "accumulate"])
@pytest.mark.parametrize("n", [6, 50])
def test_dense_row_residual_against_numpy(ta, n, kind, dtype):
    """a.x + 0.1 sin(a.x) - b, 100 items, P = 4, as AD text and with its own Jacobian, against numpy in float64; the seam tolerances
    (DESIGN section 7), per problem against max |J| and max |r|."""
    P, items = 4, 100
    rng = np.random.default_rng(n)
    data = rng.uniform(-1, 1, (P, items, n + 1)).astype(dtype)
    x = rng.uniform(-1, 1, (P, n)).astype(dtype)
    model = _res(ta, er.dense_row_body(n, kind), n=n, item_scalars=n + 1, dtype=TDT[dtype], kind=kind).bind(torch.from_numpy(data).cuda())
    rg, Jg = _eval_guarded(ta, model, torch.from_numpy(x).cuda())
    r, J = er.dense_row_rows(data, x)
    tol = SEAM_TOL[dtype]
    for p in range(P):
        er_, ej = np.abs(rg[p] - r[p]).max() / np.abs(r[p]).max(), np.abs(Jg[p] - J[p]).max() / np.abs(J[p]).max()
        print(f"n={n} {kind} {np.dtype(dtype).name} problem {p}: rel err r {er_:.3e} J {ej:.3e} (tolerance {tol:g})")
        assert er_ < tol and ej < tol


# ---- 5. consistency with the seam the solver uses ---------------------------------------------------------------------------------
def _seam_check(ta, model, x, dtype):
    r, J = ta.Eval(model, x)
    g, H, cost, nres = ta.accumulate(model, x)
    torch.cuda.synchronize()
    r, J = r.double().cpu().numpy(), J.double().cpu().numpy()
    assert J.shape == (x.shape[0], model.m, model.n) and (nres.cpu().numpy() == model.m).all()
    gh, Hh, ch = np.einsum("pma,pm->pa", J, r), np.einsum("pma,pmb->pab", J, J), np.einsum("pm,pm->p", r, r)
    tol = SEAM_TOL[dtype]
    for name, dev, host in (("g", g, gh), ("H", H, Hh), ("cost", cost, ch)):
        dev = dev.double().cpu().numpy()
        for p in range(x.shape[0]):
            err = np.abs(dev[p] - host[p]).max() / max(np.abs(host[p]).max(), 1e-300)
            print(f"{name} problem {p}: rel err {err:.3e} (tolerance {tol:g})")
            assert err < tol, name


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [12, 20])
def test_rows_agree_with_the_accumulate_seam_euclidean(ta, n, dtype):
    P, items = 4, 100
    rng = np.random.default_rng(50 + n)
    data = torch.from_numpy(rng.uniform(-1, 1, (P, items, n + 1)).astype(dtype)).cuda()
    x = torch.from_numpy(rng.uniform(-1, 1, (P, n)).astype(dtype)).cuda()
    _seam_check(ta, _res(ta, er.dense_row_body(n, "residual"), n=n, item_scalars=n + 1, dtype=TDT[dtype]).bind(data), x, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rows_agree_with_the_accumulate_seam_on_manifolds(ta, oracle, dtype):
    """The SE3 pose prior (x has 12 stored scalars, J six tangent columns; no item data) and the unit circle with x (+) d as text
    (tests/test_gpu_jit.py's bodies)."""
    rng = np.random.default_rng(9)
    P = 5
    ident = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (P, 1))
    hdr = torch.from_numpy(oracle.se3_plus(ident, 0.6 * rng.uniform(-1, 1, (P, 6))).astype(dtype)).cuda()
    pose = torch.from_numpy(oracle.se3_plus(ident, 0.3 * rng.uniform(-1, 1, (P, 6))).astype(dtype)).cuda()
    prior = _res(ta, SE3_PRIOR, n=6, item_scalars=0, residuals_per_item=6, header_scalars=12, dtype=TDT[dtype], manifold="se3").bind(None, hdr)
    r, J = ta.Eval(prior, pose)
    assert tuple(r.shape) == (P, 6) and tuple(J.shape) == (P, 6, 6) and pose.shape[1] == 12
    _seam_check(ta, prior, pose, dtype)
    items = 70
    th = rng.uniform(-1, 1, P)
    a = rng.uniform(-1, 1, (P, items, 2))
    b = rng.uniform(-1, 1, (P, items, 2))
    circle = _res(ta, SO2_RESIDUAL, n=1, item_scalars=4, residuals_per_item=2, dtype=TDT[dtype], manifold="user", plus_body=SO2_PLUS, x_scalars=2)
    model = circle.bind(torch.from_numpy(np.concatenate([a, b], -1).astype(dtype)).cuda())
    xc = torch.from_numpy(np.stack([np.cos(th), np.sin(th)], -1).astype(dtype)).cuda()
    assert tuple(ta.CalculateJac(model, xc).shape) == (P, 2 * items, 1)
    _seam_check(ta, model, xc, dtype)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(ta):
    ctx = default_context()
    lib = ctx.lib
    cost = _res(ta, "const S y = x[0] - p[0]; c = y * y;", n=1, item_scalars=1, dtype=torch.float64, kind="cost")
    data = torch.ones(2, 3, 1, dtype=torch.float64, device="cuda")
    x = torch.ones(2, 1, dtype=torch.float64, device="cuda")
    with pytest.raises(Exception, match="scalar cost.*toa_jit_accumulate already is"):
        ta.Eval(cost.bind(data), x)
    res = _res(ta, "r[0] = x[0] * x[0] - p[0];  // the refusals of Eval", n=1, item_scalars=1, dtype=torch.float64)
    model = res.bind(data)
    with pytest.raises(Exception, match="plain function.*loss"):
        ta.Eval(model.with_loss("huber", 1.0), x)
    ta.Eval(model, x)   # (and the plain model clears the handle's loss again)
    out = torch.zeros(2, 3, dtype=torch.float64, device="cuda")

    def call(m, items, P, d, xx, r, J):
        return lib.toa_jit_eval(ctx.h, m, items, P, d, xx, r, J)
    dp, xp, rp = data.data_ptr(), x.data_ptr(), out.data_ptr()
    assert call(res._h, 3, 2, dp, xp, None, None) == E_ARG and b"neither" in lib.toa_last_error()
    assert call(cost._h, 3, 2, dp, xp, rp, None) == E_ARG and b"scalar cost" in lib.toa_last_error()
    assert call(res._h, 0, 2, dp, xp, rp, None) == E_ARG and b"shape" in lib.toa_last_error()
    assert call(res._h, 3, -1, dp, xp, rp, None) == E_ARG and b"shape" in lib.toa_last_error()
    assert call(res._h, 3, 2, None, xp, rp, None) == E_ARG and b"null" in lib.toa_last_error()
    assert call(res._h, 3, 2, dp, None, rp, None) == E_ARG and b"null" in lib.toa_last_error()
    assert call(None, 3, 2, dp, xp, rp, None) == E_ARG
    assert call(res._h, 3, 0, None, None, rp, None) == 0          # an empty batch
    assert call(res._h, 1 << 30, 1, dp, xp, None, rp) == E_UNSUPPORTED and b"4 GiB" in lib.toa_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    for fn in (ta.Eval, ta.CalculateJac):
        with pytest.raises(TypeError, match="bound run-time model"):
            fn(ta.TestFn("rosenbrock", 2), torch.zeros(2, 2, dtype=torch.float64, device="cuda"))


# ---- 7. capture -------------------------------------------------------------------------------------------------------------------
def test_eval_is_refused_under_capture_until_its_kernels_exist(ta):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res = ta.JitResidual("r[0] = x[0] * x[0] - p[0];  // capture test of Eval: a text of its own", n=1, item_scalars=1, dtype=torch.float64)
        model = res.bind(torch.full((3, 2, 1), 2.0, dtype=torch.float64, device="cuda"))
        x = torch.full((3, 1), 1.5, dtype=torch.float64, device="cuda")
        r = torch.zeros(3, 2, dtype=torch.float64, device="cuda")
        J = torch.zeros(3, 2, 1, dtype=torch.float64, device="cuda")
        ta.accumulate(model, x)   # (warms the context of this stream)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(Exception, match="Eval kernels of this model are compiled on their first use .* cannot happen while the stream is being captured"):
            with torch.cuda.graph(g, stream=s):
                ta.Eval(model, x, res_out=r, J_out=J)
    torch.cuda.synchronize()
    assert bool((r == 0).all()) and bool((J == 0).all())   # nothing was recorded, nothing ran
    with torch.cuda.stream(s):
        r0, J0 = ta.Eval(model, x)
        s.synchronize()
        assert bool((r0 == 0.25).all()) and bool((J0 == 3.0).all())
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=s):
            ta.Eval(model, x, res_out=r, J_out=J)
        s.synchronize()
        x.fill_(2.0)          # the replay reads the captured tensors: r = 4 - 2, J = 4
        g2.replay()
        s.synchronize()
        r1, J1 = ta.Eval(model, x)
        s.synchronize()
        assert torch.equal(r, r1) and torch.equal(J, J1) and bool((r == 2.0).all()) and bool((J == 4.0).all())
