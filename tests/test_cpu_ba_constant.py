"""Constant cameras and points of the bundle-adjustment families, without a GPU: the projection of the
yardstick (tests/ba_constant_reference.py) on a hand-made case, what holding two cameras constant does to a Gauss-Newton solve of
the generator's (3, 9) scene, and which library entry the Python layer calls with and without flags (a recording library, as in
tests/test_cpu_api_routes.py)."""
import pytest
import torch

import ba_constant_reference as R
from test_cpu_api_routes import CudaLike, StubContext, _ba, _ba_lists
from tinyopt_amd import api

base = R.base


def test_projection_on_a_hand_made_two_camera_case():
    """2 cameras, 1 point: n = 15.  Camera 1 constant: indices 6..11; the point as well: 12..14."""
    n = 15
    g = [float(i + 1) for i in range(n)]
    H = [[float(10 * i + j + 1) for j in range(n)] for i in range(n)]
    idx = R.constant_indices(2, 1, cams=(1,))
    assert idx == [6, 7, 8, 9, 10, 11]
    g1, H1 = R.project(g, H, idx)
    for i in range(n):
        for j in range(n):
            want = (1.0 if i == j else 0.0) if (i in idx or j in idx) else H[i][j]
            assert H1[i][j] == want, (i, j)
        assert g1[i] == (0.0 if i in idx else g[i])
    assert g[6] == 7.0 and H[6][6] == 67.0                                     # the inputs are not written
    assert R.constant_indices(2, 1, cams=(1,), pts=(0,)) == [6, 7, 8, 9, 10, 11, 12, 13, 14]
    calls = []

    def fn(x, want):
        calls.append(want)
        return 3.5, (list(g) if want else None), ([r[:] for r in H] if want else None), 4
    w = R.constant(fn, idx)
    assert w(None, False) == (3.5, None, None, 4)                               # a cost-only call is untouched
    c, g2, H2, nres = w(None, True)
    assert (c, nres) == (3.5, 4) and g2 == g1 and H2 == H1


def test_two_constant_cameras_make_gauss_newton_usable():
    """The generator's (3, 9) scene — the one whose comment says "GaussNewton proper fails at once: the gauge makes H singular".
    Without flags a Gauss-Newton solve ends kSolverFailed; with cameras 0 and 1 constant it converges, and the two poses keep the
    caller's values in the yardstick too."""
    k = 2
    Cn, N, inv, outl, kind, th, pp, qp, _ = R.gen.CASES[k]
    assert (Cn, N) == (3, 9)
    f, cx, cy, uv, vis, x0, _ = R.gen.scene(9000 + k, Cn, N, inv, outl, pp, qp)
    opt = base.Options(solver="gn", min_rerr_dec=1e-6, max_iters=30)
    plain = R.optimize_constant(Cn, N, f, cx, cy, uv, vis, x0, opt)
    assert plain["stop"] == base.kSolverFailed, plain["stop"]
    held = R.optimize_constant(Cn, N, f, cx, cy, uv, vis, x0, opt, cams=(0, 1))
    assert held["stop"] > 0 and held["num_failures"] == 0 and all(held["successes"]), (held["stop"], held["successes"])
    assert held["num_iters"] >= 3 and held["final_cost"] < held["errs"][0], (held["num_iters"], held["errs"])   # (every step solved and accepted)
    assert held["x"][:24] == x0[:24] and held["x"][24:] != x0[24:]


def _recorded(model, x):
    ctx = StubContext()
    ctx.lib.names.update({ctx.h.value: "handle", x.data_ptr(): "x"})
    api.Optimize(CudaLike(x), model, api.Options(), ctx=ctx)
    return [c for c in ctx.lib.calls if c[0].startswith("toa_ba")]


@pytest.mark.parametrize("make,plain,twin", [(_ba, "toa_ba_run", "toa_ba_run_constant"), (_ba_lists, "toa_ba_lists_run", "toa_ba_lists_run_constant")])
def test_python_layer_routes(make, plain, twin, monkeypatch):
    """Without flags: the plain entry, as before.  With flags: the twin, the same leading arguments and a toa_ba_constant last —
    its members NULL where a kind was not given.  with_constant returns a copy, broadcasts [C] / [N] over the batch, composes with
    with_loss, and refuses other dtypes and shapes."""
    monkeypatch.setattr(api, "_apply_loss", lambda ctx, cost: None)
    m = make()
    if make is _ba_lists:
        m.obs_cam[:] = 0
    x = torch.zeros(m.P, m.xdim, dtype=torch.float64)
    calls = _recorded(m, x)
    assert [c[0] for c in calls] == [plain]
    cams = torch.tensor([True, False])
    held = m.with_constant(cameras=cams)
    assert held is not m and m.constant is None and held.constant[1] is None
    assert held.constant[0].dtype == torch.uint8 and held.constant[0].tolist() == [[1, 0]] * m.P
    calls2 = _recorded(held, x)
    assert [c[0] for c in calls2] == [twin]
    assert calls2[0][2:-1] == calls[0][2:] and calls2[0][1] == calls[0][1] + 1
    pod = calls2[0][-1]
    assert pod["pod"] == "ToaBaConstant" and pod["cam_dev"] == "ptr" and pod["pt_dev"] == "NULL"
    both = held.with_loss("huber", 2.0).with_constant(cameras=held.constant[0], points=torch.ones(m.P, m.npts, dtype=torch.uint8))
    assert both.loss == "huber" and both.constant[1].shape == (m.P, m.npts)
    pod = _recorded(both, x)[0][-1]
    assert pod["cam_dev"] == "ptr" and pod["pt_dev"] == "ptr"
    assert _recorded(held.with_constant(), x)[0][0] == plain                    # no flags again: the plain entry
    for bad in (torch.zeros(2), torch.zeros(3, dtype=torch.bool), torch.zeros(m.P + 1, 2, dtype=torch.bool)):
        with pytest.raises(ValueError, match="with_constant: cameras"):
            m.with_constant(cameras=bad)
    with pytest.raises(ValueError, match="with_constant: points"):
        m.with_constant(points=torch.zeros(m.npts + 1, dtype=torch.uint8))


def test_from_dense_carries_the_flags(monkeypatch):
    """from_dense(model) of a dense model made by its own constructor: the observation lists, the loss and the flags."""
    P, Cn, N = 2, 2, 3
    data = torch.zeros(P, 8 + 3 * Cn * N, dtype=torch.float64)
    data[:, :3] = torch.tensor([500.0, 320.0, 240.0])
    data[:, 8 + 2 * Cn * N:] = 1.0
    monkeypatch.setattr(torch.Tensor, "is_cuda", True)             # (the constructors assert a GPU tensor: none here)
    dense = api.BundleAdjustment(data, Cn, N)
    held = dense.with_constant(cameras=torch.tensor([1, 0], dtype=torch.uint8), points=torch.tensor([False, True, True])).with_loss("cauchy", 1.5)
    lists = api.BundleAdjustmentLists.from_dense(held)
    assert lists.nobs == Cn * N and lists.loss == "cauchy" and lists.th == 1.5
    assert lists.constant[0].tolist() == [[1, 0]] * P and lists.constant[1].tolist() == [[0, 1, 1]] * P
    plain = api.BundleAdjustmentLists.from_dense(dense)
    assert plain.constant is None and plain.loss is None and torch.equal(plain.obs_cam, lists.obs_cam)
