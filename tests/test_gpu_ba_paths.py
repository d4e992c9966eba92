"""Bundle adjustment, the paths the other three BA files do not enter (csrc/ba_schur.hip): `bl_schur_kernel` with its rows split
three ways plus `bl_schur_reduce_kernel` (C <= 128 and M / C >= 256), runs of a camera's observations that are empty or end inside
a 32-observation chunk, the second and third camera tile, the library Cholesky per scene (6 C > 512 in fp64, > 1024 in fp32, or
`large_library_solver`), the general LU at 6 C = 144, fp32 beyond 32 cameras, scenes of one batch that stop at different passes,
points no camera sees and a camera that sees nothing.  Everything is compared with the oracle (`oracle.ba_lm`: the reference's dense
(6 C + 3 N)^2 Hessian with pivoted LDL^T) — whole trajectories as tests/test_gpu_ba_lists.py does, and the first two steps against a
yardstick taken from the oracle alone (`test_first_steps_tightly`).  Section 7 pins the step bookkeeping both forms share
(lm_device.hpp) against the oracle, option branch by option branch.  Every oracle result is computed once per (scene, number
format, options) and shared (`_REF`)."""
import contextlib

import numpy as np
import pytest
import torch

from parity import check_trajectories, first_divergence, gpu_dict, last_accepted

pytestmark = pytest.mark.gpu

F64_TOL = dict(x_tol=1e-5, cost_rtol=1e-8)
F32_TOL = dict(x_tol=5e-2, cost_rtol=5e-3, err_rtol=2e-3, floor_rtol=2e-3)      # (those of test_lists_match_dense_oracle)

# name: cameras, points, scenes, seed, fraction of observations dropped, visibility pattern imposed on top (`_impose`)
SCENES = {
    # 1. split Schur rows: M / C >= 256
    "split4x260": dict(ncam=4, npts=260, P=3, seed=101),                           # runs of 96 / 96 / 68 observations
    "edge4x255": dict(ncam=4, npts=255, P=3, seed=101, gen_npts=260),              # the same scene without its last 5 points: split = 1
    "split5x330": dict(ncam=5, npts=330, P=2, seed=102, pattern="cam4_sees_40"),   # M = 1360: camera 4's runs are 32 / 8 / 0
    "split72x256": dict(ncam=72, npts=256, P=1, seed=103),                         # two camera tiles, 72 observers per point
    # 2. solver routes and camera tiles
    "lib86x40": dict(ncam=86, npts=40, P=2, seed=104),                             # 6 C = 516: the library Cholesky in fp64
    "lib172x24": dict(ncam=172, npts=24, P=1, seed=105),                           # 6 C = 1032: the same in fp32, third tile
    "mid24x30": dict(ncam=24, npts=30, P=2, seed=106, invisible=0.3),
    "full24x30": dict(ncam=24, npts=30, P=2, seed=107),
    "nine72x120": dict(ncam=72, npts=120, P=1, seed=77, pattern="nine"),           # test_lists_beyond_one_camera_tile_match_dense_oracle's
    # 3. mixed fates
    "fates16x48": dict(ncam=16, npts=48, P=3, seed=108, invisible=0.3),
    "fates24x30": dict(ncam=24, npts=30, P=3, seed=109, invisible=0.3),
    # 4. unseen points, a blind camera
    "unseen6x40": dict(ncam=6, npts=40, P=2, seed=110, invisible=0.3, pattern="unseen"),
    "unseen16x48": dict(ncam=16, npts=48, P=2, seed=111, invisible=0.3, pattern="unseen"),
    "unseen24x30": dict(ncam=24, npts=30, P=2, seed=112, invisible=0.3, pattern="unseen"),
    "blind6x40": dict(ncam=6, npts=40, P=2, seed=110, invisible=0.3, pattern="blind"),
    "blind16x48": dict(ncam=16, npts=48, P=2, seed=111, invisible=0.3, pattern="blind"),
    "blind24x30": dict(ncam=24, npts=30, P=2, seed=112, invisible=0.3, pattern="blind"),
    # 5. the dense-mask counts added to test_ba_matches_dense_oracle (its scenes: seed 7 + C, a pattern per scene)
    "dense4x60": dict(ncam=4, npts=60, P=3, seed=11, own_patterns=True),
    "dense6x45": dict(ncam=6, npts=45, P=3, seed=13, invisible=0.2, own_patterns=True),
    "dense9x35": dict(ncam=9, npts=35, P=3, seed=16, own_patterns=True),
}
_SCENE, _REF = {}, {}


def _unseen(npts):
    return [0, 17, 18, npts - 1]


def _impose(kind, vis, seed):
    ncam, npts = vis.shape
    rng = np.random.default_rng(seed + 1)
    if kind == "cam4_sees_40":
        vis[4] = 0.0
        vis[4, rng.choice(npts, 40, replace=False)] = 1.0
    elif kind == "nine":                      # (as _sparse_scene of tests/test_gpu_ba_lists.py)
        vis[:] = 0.0
        for j in range(npts):
            vis[rng.choice(ncam, 9, replace=False), j] = 1.0
    elif kind == "unseen":
        vis[:, _unseen(npts)] = 0.0
    elif kind == "blind":
        vis[ncam // 2] = 0.0
    else:
        assert kind is None, kind


def _take_points(data, x0, ncam, npts, keep):
    P = data.shape[0]
    uv = data[:, 8:8 + 2 * ncam * npts].reshape(P, ncam, npts, 2)[:, :, :keep].reshape(P, -1)
    vis = data[:, 8 + 2 * ncam * npts:].reshape(P, ncam, npts)[:, :, :keep].reshape(P, -1)
    return np.concatenate([data[:, :8], uv, vis], 1), np.ascontiguousarray(x0[:, :12 * ncam + 3 * keep])


def _scene(oracle, name):
    """(data, x0) in float64 — the fp32 runs take their casts, which is what `synth_ba` hands out for float32.  One visibility
    pattern (scene 0's, then `pattern`) in every scene of the batch: `from_dense` needs equal M."""
    if name not in _SCENE:
        s = SCENES[name]
        ncam, npts, gen = s["ncam"], s["npts"], s.get("gen_npts", s["npts"])
        data, x0, _ = oracle.synth_ba(s["P"], ncam, gen, np.float64, seed=s["seed"], invisible=s.get("invisible", 0.0))
        if gen != npts:
            data, x0 = _take_points(data, x0, ncam, gen, npts)
        if not s.get("own_patterns"):
            vis = data[0, 8 + 2 * ncam * npts:].reshape(ncam, npts).copy()
            _impose(s.get("pattern"), vis, s["seed"])
            data[:, 8 + 2 * ncam * npts:] = vis.ravel()[None, :]
        _SCENE[name] = (data, x0)
    return _SCENE[name]


def _opts(ta, key):
    o = ta.Options.benchmark() if key in ("benchmark", "lu") else ta.Options()
    if key == "lu":
        o.hessian.use_ldlt = False
    if key in ("first", "first_lu"):
        o.max_iters = 1
        o.hessian.use_ldlt = key == "first"
    return o


def _ref(ta, oracle, name, dtype, okey, x0=None, tag=""):
    """The oracle's solve of a scene, once per (scene, number format, options[, start])."""
    key = (name, np.dtype(dtype).name, okey, tag)
    if key not in _REF:
        data, x0s = _scene(oracle, name)
        s = SCENES[name]
        start = x0s if x0 is None else x0
        ref = oracle.ba_lm(data.astype(dtype), start.astype(dtype), s["ncam"], s["npts"], _opts(ta, okey).to_pod())
        assert (ref["stop"] >= 0).all(), (name, ref["stop"])
        _REF[key] = ref
    return _REF[key]


def _knob(ta, on):
    return ta.api.default_context().tuning(large_library_solver=1) if on else contextlib.nullcontext()


def _run(ta, form, data, x0, ncam, npts, opts, dtype, knob=False):
    dd = torch.from_numpy(data.astype(dtype)).cuda()
    model = ta.BundleAdjustment(dd, ncam, npts) if form == "dense" else ta.BundleAdjustmentLists.from_dense(dd, ncam, npts)
    if form == "lists":
        assert model.nobs == int(data[0, 8 + 2 * ncam * npts:].sum())
    x = torch.from_numpy(x0.astype(dtype)).cuda()
    with _knob(ta, knob):
        out = ta.Optimize(x, model, opts, history=True)
        torch.cuda.synchronize()
    return x, out


def _against_oracle(ta, oracle, name, dtype, okey, form="lists", knob=False, x0=None, tag=""):
    """One solve of the whole batch against the oracle's, the way test_lists_match_dense_oracle compares; returns (x, out, ref)."""
    s = SCENES[name]
    ncam, npts, P = s["ncam"], s["npts"], s["P"]
    data, x0s = _scene(oracle, name)
    start = x0s if x0 is None else x0
    ref = _ref(ta, oracle, name, dtype, okey, x0=x0, tag=tag)
    opts = _opts(ta, okey)
    x, out = _run(ta, form, data, start, ncam, npts, opts, dtype, knob=knob)
    f64 = dtype == np.float64
    assert (out.stop_reason.cpu().numpy() >= 0).all(), (name, out.stop_reason.cpu().numpy(), out.num_iters.cpu().numpy())
    assert np.array_equal(out.final_num_residuals.cpu().numpy(), ref["nres"])
    refd = {k: ref[k] for k in ("errs", "succ", "iters", "stop", "x", "cost", "fails", "deltas2")}
    st = check_trajectories(gpu_dict(out, x), refd, dtype, opts.to_pod(), tol=F64_TOL if f64 else F32_TOL, label=f"BA {form} {name} {okey}")
    assert st["full"] + st["ties"] == P
    if f64:
        k = int(min(out.num_iters.min().item(), ref["iters"].min()))
        assert np.allclose(out.deltas2.cpu().numpy()[:, :k], ref["deltas2"][:, :k], rtol=1e-6)      # the STEP equals the dense step
    return x, out, ref


def _same_bits_alone_and_again(ta, oracle, name, dtype, okey, x, out, row, x0=None, form="lists", knob=False):
    """Scene `row` solved alone gives the bits of its row in the batch; a second run of the batch gives the same bits."""
    s = SCENES[name]
    data, x0s = _scene(oracle, name)
    start = x0s if x0 is None else x0
    opts = _opts(ta, okey)
    x1, o1 = _run(ta, form, data[row:row + 1], start[row:row + 1], s["ncam"], s["npts"], opts, dtype, knob=knob)
    assert torch.equal(x1[0], x[row]), (name, row, float((x1[0] - x[row]).abs().max()))
    assert int(o1.num_iters[0]) == int(out.num_iters[row]) and float(o1.final_cost[0]) == float(out.final_cost[row])
    x2, o2 = _run(ta, form, data, start, s["ncam"], s["npts"], opts, dtype, knob=knob)
    assert torch.equal(x2, x) and torch.equal(o2.errs, out.errs) and torch.equal(o2.num_iters, out.num_iters)


# ---- 1. split Schur rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,okey", [
    ("split4x260", np.float64, "default"), ("split4x260", np.float64, "benchmark"), ("split4x260", np.float32, "default"),
    ("edge4x255", np.float64, "default"), ("split5x330", np.float64, "default"), ("split72x256", np.float64, "default")])
def test_split_schur_rows_match_dense_oracle(ta, oracle, name, dtype, okey):
    """`bl_schur_kernel` dealing a camera's observations to three workgroups and `bl_schur_reduce_kernel` summing their partial
    rows: a last run that ends 4 observations into a chunk (4 x 260), the other side of the M / C >= 256 border (4 x 255: one
    workgroup per camera), a camera whose runs are 32 / 8 / 0 (5 x 330), and split rows over two camera tiles with 72 observers
    per point, most of them read past the staged list (72 x 256)."""
    s = SCENES[name]
    data, _ = _scene(oracle, name)
    M = int(data[0, 8 + 2 * s["ncam"] * s["npts"]:].sum())
    assert (M // s["ncam"] >= 256) == (name != "edge4x255")                # the side of the border the case is meant for
    x, out, _ = _against_oracle(ta, oracle, name, dtype, okey)
    _same_bits_alone_and_again(ta, oracle, name, dtype, okey, x, out, s["P"] - 1)


# ---- 2. solver routes and camera tiles ----------------------------------------------------------------------------------------------
def test_library_cholesky_per_scene_fp64(ta, oracle):
    """86 cameras: 6 C = 516 > 512 — the library's Cholesky, ONE call per scene with the solve mask, and the second camera tile.
    Scene 1 alone gives the bits of row 1 of the batch (the promise in the comment at `toa_large_solve_each`)."""
    x, out, _ = _against_oracle(ta, oracle, "lib86x40", np.float64, "default")
    _same_bits_alone_and_again(ta, oracle, "lib86x40", np.float64, "default", x, out, 1)


def test_library_cholesky_fp32_third_camera_tile(ta, oracle):
    """172 cameras in fp32: 6 C = 1032 > 1024 — the library route in fp32; cameras 128..171 take the third tile."""
    _against_oracle(ta, oracle, "lib172x24", np.float32, "default")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_library_solver_knob_follows_the_oracle(ta, oracle, dtype):
    """`large_library_solver = 1` sends a 144-unknown reduced system down the library route: the oracle's trajectory in both
    number formats; in fp64 the counts and verdicts of the solve without the knob, and its x to 1e-9."""
    x, out, _ = _against_oracle(ta, oracle, "mid24x30", dtype, "default", knob=True)
    if dtype == np.float64:
        x0, o0, _ = _against_oracle(ta, oracle, "mid24x30", dtype, "default")
        assert torch.equal(out.num_iters, o0.num_iters) and torch.equal(out.stop_reason, o0.stop_reason)
        assert float((x - x0).abs().max()) < 1e-9


def test_use_ldlt_false_at_144_unknowns(ta, oracle):
    """The pattern of test_use_ldlt_false_in_both_ba_forms at 6 C = 144: the library's general LU on a system the lists form
    otherwise hands to the one-workgroup Cholesky."""
    _against_oracle(ta, oracle, "full24x30", np.float64, "lu")


def test_two_camera_tiles_fp32(ta, oracle):
    """The scene of test_lists_beyond_one_camera_tile_match_dense_oracle (72 cameras, nine observers per point) in fp32."""
    data, _ = _scene(oracle, "nine72x120")
    assert int(data[0, 8 + 2 * 72 * 120:].sum()) == 9 * 120
    _against_oracle(ta, oracle, "nine72x120", np.float32, "default")


# ---- 3. mixed fates in one batch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fates16x48", "fates24x30"])
def test_mixed_fates_in_one_batch(ta, oracle, name):
    """Three scenes of one batch stopping at different passes (flags [0] and the solve mask; at C = 24 the in-place Cholesky):
    scene 0 starts from the solution of an earlier solve of itself, scene 1 from x0, scene 2 from x0 with the pose perturbation
    doubled.  Each against its own oracle trajectory; each alone bit-equal to its row."""
    s = SCENES[name]
    data, x0 = _scene(oracle, name)
    first = _ref(ta, oracle, name, np.float64, "default")
    _, x0_far, _ = oracle.synth_ba(s["P"], s["ncam"], s["npts"], np.float64, seed=s["seed"], invisible=s["invisible"], pose_pert=0.04)
    start = x0.copy()
    start[0] = first["x"][0]
    start[2] = x0_far[2]
    assert not np.array_equal(x0_far[2, :12 * s["ncam"]], x0[2, :12 * s["ncam"]]) and np.array_equal(x0_far[2, 12 * s["ncam"]:], x0[2, 12 * s["ncam"]:])
    x, out, ref = _against_oracle(ta, oracle, name, np.float64, "default", x0=start, tag="fates")
    assert ref["iters"][0] <= 2, ref["iters"]
    assert len(set(int(k) for k in ref["iters"])) > 1, ref["iters"]                  # (on the oracle's counts: never vacuous)
    for row in range(s["P"]):
        _same_bits_alone_and_again(ta, oracle, name, np.float64, "default", x, out, row, x0=start)


# ---- 4. unseen points and a blind camera --------------------------------------------------------------------------------------------
_FORMS = [("6x40", "dense", np.float64, "default"), ("6x40", "dense", np.float64, "benchmark"), ("6x40", "dense", np.float32, "default"),
          ("6x40", "lists", np.float64, "default"), ("6x40", "lists", np.float64, "benchmark"),
          ("16x48", "lists", np.float64, "default"), ("16x48", "lists", np.float64, "benchmark"),
          ("24x30", "lists", np.float64, "default"), ("24x30", "lists", np.float64, "benchmark"), ("24x30", "lists", np.float32, "default")]


@pytest.mark.parametrize("size,form,dtype,okey", _FORMS)
def test_unseen_points_take_a_zero_step(ta, oracle, size, form, dtype, okey):
    """Points 0, 17, 18 and N - 1 are seen by no camera: V_j = 0, `empty` in the point solve, `bl_index_a_kernel`'s fill of
    pt_start for empty points at the head, in the middle (two in a row) and at the tail.  The oracle's pivoted LDL^T steps over
    their zero pivots; so must the device — the trajectory is the oracle's and the four points keep the bits of x0."""
    name = "unseen" + size
    s = SCENES[name]
    x, out, ref = _against_oracle(ta, oracle, name, dtype, okey, form=form)
    _, x0 = _scene(oracle, name)
    cols = [12 * s["ncam"] + 3 * j + a for j in _unseen(s["npts"]) for a in range(3)]
    assert np.array_equal(ref["x"][:, cols], x0.astype(dtype)[:, cols])
    assert np.array_equal(x.cpu().numpy()[:, cols], x0.astype(dtype)[:, cols])


@pytest.mark.parametrize("size,form,dtype,okey,knob", [f + (False,) for f in _FORMS] + [("24x30", "lists", np.float64, "default", True)])
def test_blind_camera_takes_a_zero_step(ta, oracle, size, form, dtype, okey, knob):
    """Camera C / 2 sees nothing: U_c = 0 and no W, a zero block row of S.  The oracle's pivoted LDL^T pushes the six zero pivots
    to the end and solves with the pseudo-inverse: the camera does not move.  The lists form factorises S without pivoting (before
    the rule below every solve failed: kSolverFailed after one iteration), so `bl_build_kernel` sets the blind camera's damped
    diagonal to one — the identity block in S; its right-hand side is zero, hence dc = 0.  The dense-mask kernel reaches the same
    step through its pivoted fallback."""
    name = "blind" + size
    s = SCENES[name]
    x, out, ref = _against_oracle(ta, oracle, name, dtype, okey, form=form, knob=knob)
    _, x0 = _scene(oracle, name)
    cols = list(range(12 * (s["ncam"] // 2), 12 * (s["ncam"] // 2) + 12))
    assert np.array_equal(ref["x"][:, cols], x0.astype(dtype)[:, cols])
    assert np.array_equal(x.cpu().numpy()[:, cols], x0.astype(dtype)[:, cols])


# ---- 6. the first steps, tightly ----------------------------------------------------------------------------------------------------
_FIRST = ([("split4x260", "lists", np.float64, False), ("split4x260", "lists", np.float32, False), ("edge4x255", "lists", np.float64, False),
           ("split5x330", "lists", np.float64, False), ("split72x256", "lists", np.float64, False),
           ("lib86x40", "lists", np.float64, False), ("lib172x24", "lists", np.float32, False),
           ("mid24x30", "lists", np.float64, True), ("mid24x30", "lists", np.float32, True), ("full24x30", "lists", np.float64, False),
           ("nine72x120", "lists", np.float32, False)]
          + [(kind + size, form, dtype, False) for kind in ("unseen", "blind") for size, form, dtype, okey in _FORMS if okey == "default"]
          + [(name, "dense", dtype, False) for name in ("dense4x60", "dense6x45", "dense9x35") for dtype in (np.float64, np.float32)])


@pytest.mark.parametrize("name,form,dtype,knob", _FIRST)
def test_first_steps_tightly(ta, oracle, name, form, dtype, knob):
    """Whole trajectories are compared with x_tol = 1e-5 (fp64) / 5e-2 (fp32) because the gauge drifts over a solve; the first
    steps do not.  With max_iters = 1 the oracle takes two steps and stops with kMaxIters; the device's x after such a run is
    compared with the fp64 oracle's.  The yardstick comes from the oracle alone:
        gap32 = max |x_oracle(fp32 inputs) - x_oracle(fp64 inputs)|
    fp32 device: max |x - x_oracle64| <= 4 gap32 (the margin for blocked against sequential sums); fp64 device: <= 64 * 2^-29 * gap32
    (2^-29: the ratio of the two unit round-offs; 64: Schur elimination and dense pivoted LDL^T round differently on one system).
    `full24x30` runs with use_ldlt = false, `mid24x30` under large_library_solver = 1, the rest with Options().

    max |x - x_oracle64| / bound  measured on the MI355X, per case (every bound holds as the issue states it, none was raised):
      fp64 lists   split4x260 0.015  edge4x255 0.024  split5x330 0.013  split72x256 0.031  lib86x40 0.009  mid24x30 0.015
                   full24x30 0.017  unseen6x40 0.026  unseen16x48 0.016  unseen24x30 0.011  blind6x40 0.019  blind16x48 0.039
                   blind24x30 0.018
      fp64 dense   unseen6x40 0.019  blind6x40 0.015  dense4x60 0.019  dense6x45 0.020  dense9x35 0.021
      fp32 lists   split4x260 0.074  lib172x24 0.260  mid24x30 0.130  nine72x120 0.158  unseen24x30 0.095  blind24x30 0.115
      fp32 dense   unseen6x40 0.114  blind6x40 0.115  dense4x60 0.083  dense6x45 0.269  dense9x35 0.230
    (gap32 is 1.4e-5 to 1.0e-4 on these scenes for steps of 5e-2 to 8e-2; the fp64 device sits 5e-14 to 2.3e-13 from the oracle.)"""
    s = SCENES[name]
    okey = "first_lu" if name == "full24x30" else "first"
    data, x0 = _scene(oracle, name)
    r64, r32 = _ref(ta, oracle, name, np.float64, okey), _ref(ta, oracle, name, np.float32, okey)
    kmax = int(ta.StopReason.kMaxIters)
    assert (r64["stop"] == kmax).all() and (r32["stop"] == kmax).all() and (r64["iters"] == 2).all(), (r64["stop"], r64["iters"])
    gap32 = float(np.abs(r32["x"].astype(np.float64) - r64["x"]).max())
    assert gap32 > 0
    x, out = _run(ta, form, data, x0, s["ncam"], s["npts"], _opts(ta, okey), dtype, knob=knob)
    assert (out.stop_reason.cpu().numpy() == kmax).all() and (out.num_iters.cpu().numpy() == 2).all(), (out.stop_reason, out.num_iters)
    err = float(np.abs(x.cpu().numpy().astype(np.float64) - r64["x"]).max())
    bound = 4.0 * gap32 if dtype == np.float32 else 64.0 * 2.0 ** -29 * gap32
    step = float(np.abs(r64["x"] - x0).max())
    print(f"FIRST {name} {form} {np.dtype(dtype).name}: step {step:.3e} gap32 {gap32:.3e} err {err:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (name, form, err, bound, gap32)


# ---- 7. every branch of the step bookkeeping, in both forms -------------------------------------------------------------------------
def _variant(ta, key):
    o = ta.Options()
    if key == "final_cost": o.check_final_cost = True; o.max_iters = 3                        # the final cost-only pass
    elif key == "one_iter": o.max_iters = 1                                                   # the iteration bound
    elif key == "damping10": o.lm.damping_init = 10.0                                         # a chain of GoodSteps
    elif key == "step_quality": o.use_step_quality_approx = True                              # the step-quality branch of GoodStep
    elif key == "clip5": o.grad_clipping = 0.5; o.max_iters = 5                               # rejected steps, roll-backs, eval-only iterations
    elif key == "clip_total2": o.grad_clipping = 0.5; o.max_iters = 8; o.max_total_failures = 2       # kMaxNoDecr
    elif key == "clip_consec2": o.grad_clipping = 0.5; o.max_iters = 8; o.max_consec_failures = 2     # kMaxConsecNoDecr
    elif key == "clip_total1": o.grad_clipping = 0.5; o.max_iters = 8; o.max_total_failures = 1       # the FIRST rejection: roll back, kMaxNoDecr
    elif key == "clip_consec1": o.grad_clipping = 0.5; o.max_iters = 8; o.max_consec_failures = 1     # ... roll back, kMaxConsecNoDecr
    elif key == "clip_final_cost": o.grad_clipping = 0.5; o.max_iters = 4; o.check_final_cost = True  # rejections under the final-cost pass
    elif key == "min_h_diag": o.hessian.check_min_H_diag = 1e9                                # Build fails, re-damps, retries to the consecutive limit
    elif key == "min_error": o.min_error = 1e9                                                # immediate kMinError
    else: raise KeyError(key)
    return o


# (Gauss-Newton is absent on purpose: a BA Hessian has seven free gauge directions, so without damping the verdict of the
#  factorisation is decided by rounding — not a property of the code under test.)
_VARIANTS = ["final_cost", "one_iter", "damping10", "step_quality", "clip5", "clip_total2", "clip_consec2", "clip_final_cost",
             "min_h_diag", "min_error", "clip_total1", "clip_consec1"]
# The four variants with grad_clipping reject steps, and a rejected step cannot be followed against the oracle to the end: the
# iteration after a roll-back evaluates the restored point, so `err < final_cost` (optimizer.h:428-429) compares two costs that
# are equal in exact arithmetic and is decided by the last bit of (x (+) dx) (+) -dx — SE3 poses never come back bit for bit.
# Measured on the MI355X before the bookkeeping moved: all twelve cases part from the oracle at such an iteration (cost equal
# to the accepted cost to 1e-16) and then walk away from it, e.g. dense 3 x 40 clip5: stop 2/2/2, iterations 3/6/3, failures
# 1/3/1 against the oracle's 5/2/2, 6/6/3, 4/3/1; the two device forms part from each other the same way.  These variants are
# pinned by test_rejected_steps_roll_back_and_count instead: the oracle up to the tie, the rules of the loop body after it.
# clip_total1 and clip_consec1 reject a step too, but their first rejection ends the solve — the step is rolled back, the StopReason
# and the counters are set, and the restored point is never evaluated again: no tie, so they follow the oracle to the end (the
# roll-back shows in the final x).
_CLIPPED = ["clip5", "clip_total2", "clip_consec2", "clip_final_cost"]
_FOLLOWED = [k for k in _VARIANTS if k not in _CLIPPED]
_VARIANT_SCENES = [("dense", 3, 40), ("lists", 3, 40), ("lists", 12, 30)]
_VREF = {}


def _variant_ref(ta, oracle, ncam, npts, key):
    """(data, x0, the oracle's solve) of the three scenes `synth_ba(3, C, N, float64, seed=9)` under one variant, once."""
    k = (ncam, npts, key)
    if k not in _VREF:
        data, x0, _ = oracle.synth_ba(3, ncam, npts, np.float64, seed=9)
        _VREF[k] = (data, x0, oracle.ba_lm(data, x0, ncam, npts, _variant(ta, key).to_pod()))
    return _VREF[k]


def _oracle_consec(ref):
    """num_consec_failures is not among the oracle's outputs, but its history fixes it: the counter is zeroed by iteration 0 and by
    every accepted step, and raised by every rejected step and every failed solve (optimizer.h:370-373, 441-453).  A stop below zero
    ends an iteration before it is recorded.  Failed solves (num_failures minus the rejections on record) can be placed only when
    there is no record at all, which is asserted."""
    out = []
    for p in range(len(ref["iters"])):
        nh = int(ref["iters"][p]) - (1 if ref["stop"][p] < 0 else 0)
        rejected = [i for i in range(1, nh) if not ref["succ"][p, i]]
        solve_fails = int(ref["fails"][p]) - len(rejected)
        assert solve_fails == 0 or nh == 0, (p, solve_fails, nh)
        reset = max([i for i in range(nh) if i == 0 or ref["succ"][p, i]], default=-1)
        out.append(len([i for i in rejected if i > reset]) + solve_fails)
    return np.array(out)


def _rolled_back(ref):
    """Scenes whose record holds a rejected step right after an applied one: x (+)= -last_dx (optimizer.h:283-287)."""
    return sum(1 for p in range(len(ref["iters"])) for i in range(1, int(ref["iters"][p]) if ref["stop"][p] >= 0 else 0)
               if not ref["succ"][p, i] and (i == 1 or ref["succ"][p, i - 1]))


def test_option_variants_reach_their_branches(ta, oracle):
    """The oracle's own results on the inputs of test_option_variants_match_dense_oracle: at least one roll-back, one kMaxNoDecr,
    one kMaxConsecNoDecr, one kSolverFailed after retries, scenes of one batch with different fates — so the pin cannot quietly
    stop reaching those branches."""
    SR = ta.StopReason
    for ncam, npts in sorted({(c, n) for _, c, n in _VARIANT_SCENES}):
        ref = {key: _variant_ref(ta, oracle, ncam, npts, key)[2] for key in _VARIANTS}
        assert _rolled_back(ref["clip5"]) >= 1 and (ref["clip5"]["fails"] >= 1).all(), (ref["clip5"]["succ"], ref["clip5"]["fails"])
        assert (ref["clip_total2"]["stop"] == int(SR.kMaxNoDecr)).any(), ref["clip_total2"]["stop"]
        assert (ref["clip_consec2"]["stop"] == int(SR.kMaxConsecNoDecr)).any(), ref["clip_consec2"]["stop"]
        assert (ref["clip_final_cost"]["fails"] >= 1).all(), ref["clip_final_cost"]["fails"]
        assert (ref["min_h_diag"]["stop"] == int(SR.kSolverFailed)).all() and (ref["min_h_diag"]["iters"] == 1).all()
        assert (ref["min_h_diag"]["fails"] == 5).all() and (_oracle_consec(ref["min_h_diag"]) == 5).all()
        assert (ref["min_error"]["stop"] == int(SR.kMinError)).all() and (ref["min_error"]["iters"] == 1).all()
        assert (ref["one_iter"]["stop"] == int(SR.kMaxIters)).all() and (ref["one_iter"]["iters"] == 2).all()
        assert (ref["damping10"]["iters"] > ref["step_quality"]["iters"]).all(), (ref["damping10"]["iters"], ref["step_quality"]["iters"])
        # the two variants that follow the oracle through a rejection: every scene rolls its only rejected step back and stops, and
        # that step is far larger than x_tol, so a step left standing (or applied again) cannot pass the comparison of x
        for key, stop in (("clip_total1", SR.kMaxNoDecr), ("clip_consec1", SR.kMaxConsecNoDecr)):
            r = ref[key]
            assert (r["stop"] == int(stop)).all() and (r["fails"] == 1).all() and (_oracle_consec(r) == 1).all(), (key, r["stop"], r["fails"])
            assert _rolled_back(r) == 3, (key, r["succ"])
            last = np.array([r["deltas2"][p, r["iters"][p] - 1] for p in range(3)])
            assert (np.sqrt(last / (6 * ncam + 3 * npts)) > 100 * F64_TOL["x_tol"] * np.abs(r["x"]).max()).all(), (key, last)
    r = _variant_ref(ta, oracle, 3, 40, "clip5")[2]
    assert len(set(zip(r["stop"].tolist(), r["iters"].tolist(), r["fails"].tolist()))) == 3, (r["stop"], r["iters"], r["fails"])


@pytest.mark.parametrize("key", _CLIPPED)
@pytest.mark.parametrize("form,ncam,npts", _VARIANT_SCENES)
def test_rejected_steps_roll_back_and_count(ta, oracle, form, ncam, npts, key):
    """Rejected steps on the BA kernels, checked by what does not hang on a last bit (see _CLIPPED):
      * up to the first iteration at which device and oracle part, the same costs (1e-9) and accept / reject flags; they part only
        at an iteration that follows a rejected step and whose cost is the last accepted cost to 1e-11 on both sides: a proven tie;
      * every rejected step that follows an applied one is rolled back: the next iteration's cost is the last accepted cost
        to 1e-9 (a step applied a second time, or not taken back, leaves it percents away);
      * the counters and the StopReason are those of optimizer.h:441-460 and :320-321 replayed on the device's OWN record: every
        rejection counts, an accepted step zeroes the consecutive count, kMaxConsecNoDecr / kMaxNoDecr end the loop exactly when
        their limit is reached, kMaxIters exactly at the iteration bound, and the final cost is the last accepted one."""
    SR = ta.StopReason
    data, x0, ref = _variant_ref(ta, oracle, ncam, npts, key)
    opts = _variant(ta, key)
    pod = opts.to_pod()
    x, out = _run(ta, form, data, x0, ncam, npts, opts, np.float64)
    got = gpu_dict(out, x)
    consec = out.num_consec_failures.cpu().numpy()
    print(f"REJECT {form} {ncam}x{npts} {key}: stop {got['stop']} / {ref['stop']}  iters {got['iters']} / {ref['iters']}  "
          f"fails {got['fails']} / {ref['fails']}  consec {consec} / {_oracle_consec(ref)}")
    bound = pod.max_iters + 1 + (1 if pod.check_final_cost else 0)
    rolled = 0
    for p in range(3):
        e, s, k = got["errs"][p], got["succ"][p], int(got["iters"][p])
        re_, rs, rk = ref["errs"][p], ref["succ"][p], int(ref["iters"][p])
        label = (form, ncam, npts, key, p)
        assert got["stop"][p] > 0 and 1 <= k <= bound, (label, got["stop"][p], k)
        d = first_divergence(e, s, k, re_, rs, rk, rtol=1e-9, atol=1e-300)
        if d is not None and d < min(k, rk):
            acc = last_accepted(e, s, d)
            assert d >= 2 and not s[d - 1] and not rs[d - 1], (label, "parted away from a roll-back", d)
            assert abs(e[d] - acc) <= 1e-11 * acc and abs(re_[d] - acc) <= 1e-11 * acc, (label, "parted away from a tie", d, e[d], re_[d], acc)
        fails = run = 0
        stop = None
        for i in range(k):
            assert stop is None, (label, "went on after a failure limit", i)
            if i == 0 or s[i]:
                run = 0
                continue
            fails += 1
            run += 1
            if pod.max_consec_failures > 0 and run >= pod.max_consec_failures: stop = int(SR.kMaxConsecNoDecr)
            elif pod.max_total_failures > 0 and fails >= pod.max_total_failures: stop = int(SR.kMaxNoDecr)
            if (i == 1 or s[i - 1]) and i + 1 < k:
                rolled += 1
                acc = last_accepted(e, s, i)
                assert abs(e[i + 1] - acc) <= 1e-9 * acc, (label, "not rolled back", i, e[i + 1], acc)
        assert fails == got["fails"][p] and run == consec[p], (label, fails, got["fails"][p], run, consec[p])
        if stop is not None:
            assert got["stop"][p] == stop, (label, got["stop"][p], stop)
        elif got["stop"][p] == int(SR.kMaxIters):
            assert k == bound, (label, k, bound)
        else:
            assert int(SR.kMinError) <= got["stop"][p] <= int(SR.kMinGradNorm), (label, got["stop"][p])
        assert got["cost"][p] == last_accepted(e, s, k), (label, got["cost"][p], last_accepted(e, s, k))
    assert rolled >= 1, (form, ncam, npts, key, "no roll-back on the device")


@pytest.mark.parametrize("key", _FOLLOWED)
@pytest.mark.parametrize("form,ncam,npts", _VARIANT_SCENES)
def test_option_variants_match_dense_oracle(ta, oracle, form, ncam, npts, key):
    """The "solve failed: count, stop or re-damp and retry" branch and the loop body of OptimizeAcc (accept, roll back or first
    step, eval-only iteration, rebuild, the counters) on the BA kernels, which state them outside one wavefront: `ba_schur_kernel`
    (dense form) and `bl_step_kernel` (lists form: 3 cameras, and 12 — the workgroup LDL^T behind bl_schur).  Whole trajectories
    against the oracle with the fp64 tolerances of test_ba_matches_dense_oracle, and the same StopReason, iteration, failure and
    consecutive-failure counts."""
    P = 3
    data, x0, ref = _variant_ref(ta, oracle, ncam, npts, key)
    opts = _variant(ta, key)
    x, out = _run(ta, form, data, x0, ncam, npts, opts, np.float64)
    got = gpu_dict(out, x)
    consec = out.num_consec_failures.cpu().numpy()
    print(f"VARIANT {form} {ncam}x{npts} {key}: stop {got['stop']} / {ref['stop']}  iters {got['iters']} / {ref['iters']}  "
          f"fails {got['fails']} / {ref['fails']}  consec {consec} / {_oracle_consec(ref)}")
    refd = {k: ref[k] for k in ("errs", "succ", "iters", "stop", "x", "cost", "fails", "deltas2")}
    st = check_trajectories(got, refd, np.float64, opts.to_pod(), tol=F64_TOL, label=f"BA {form} {ncam}x{npts} {key}")
    assert st["full"] + st["ties"] == P, st
    assert np.array_equal(got["stop"], ref["stop"]) and np.array_equal(got["iters"], ref["iters"])
    assert np.array_equal(got["fails"], ref["fails"]) and np.array_equal(consec, _oracle_consec(ref))
