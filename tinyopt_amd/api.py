"""Host-side mirror of tinyopt's Optimize / Options / Output for batched device models.

Names and meanings follow the reference:
  Options   include/tinyopt/optimizers/options.h:18-156 (nested groups hessian / cost / lm kept)
  Output    include/tinyopt/output.h:26-145 (one entry per problem of the batch)
  Optimize  include/tinyopt/optimize.h:16-77  ``Optimize(x, cost, options)``; x is updated in place
"""
from __future__ import annotations

import contextlib
import copy
import ctypes as C
import enum
import functools
import time

import numpy as np
from dataclasses import dataclass, field
from typing import Optional

import torch

from . import _capi
from ._capi import (F32, F64, MODEL_DENSE_ROW_AD, MODEL_DENSE_ROW_NATURAL, MODEL_TESTFN, MODEL_MAHA_PRIOR, MODEL_SE3_PRIOR, MODEL_CIRCLE_FIT, MODEL_DENSE_ROW, MODEL_DENSE_ROW_AD6, MODEL_GAUSSIAN_PRIOR, MODEL_SE3_REPROJ,
                    MODEL_SQRT2, ToaBaConstant, ToaBounds, ToaGdOptions, ToaJitSpec, ToaLbfgsOptions, ToaOptions, ToaPrior, ToaResults, ToaShared, check)


class StopReason(enum.IntEnum):  # include/tinyopt/stop_reasons.h:14-43
    kOutOfMemory = -4
    kSolverFailed = -3
    kSystemHasNaNOrInf = -2
    kSkipped = -1
    kNone = 0
    kMinError = 1
    kMinRelError = 2
    kMinDeltaNorm = 3
    kMinGradNorm = 4
    kMaxIters = 5
    kMaxNoDecr = 6
    kMaxConsecNoDecr = 7
    kTimedOut = 8
    kUserStopped = 9


@dataclass
class _Hessian:  # options.h:58-67
    use_ldlt: bool = True
    H_is_full: bool = True
    check_min_H_diag: float = 0.0
    save_last: bool = True


@dataclass
class _CostScaling:  # options.h:75-80
    use_squared_norm: bool = True
    downscale_by_2: bool = False
    normalize: bool = False


@dataclass
class _LM:  # options.h:127-141
    damping_init: float = 1e-4
    damping_range: tuple = (1e-9, 1e9)
    good_factor: float = 1.0 / 3.0
    bad_factor: float = 2.0


@dataclass
class _GD:  # options.h:147-154 — Options::GD
    lr: float = 1e-3   # learning rate (a float in the reference: promoted to the scalar type of x)


@dataclass
class _LBFGS:  # toa_lbfgs_options: the textbook values (Nocedal & Wright, chapters 3 and 7)
    history: int = 8       # pairs (s, y) kept, 1 .. 16
    c1: float = 1e-4       # the Armijo constant, in (0, 1)
    shrink: float = 0.5    # alpha *= shrink after a rejected trial, in (0, 1)


@dataclass
class _Log:  # options.h:113-125 — the per-iteration log line of Optimizer_::Step (optimizer.h:463-516)
    enable: bool = False           # (the reference logs by default; a batched solve does not: one line per problem and iteration)
    e: str = "\u03b5\u00b2"          # symbol of the error in the line
    print_emoji: bool = True
    print_x: bool = False
    print_dx: bool = False
    print_inliers: bool = False
    print_t: bool = True
    problems: Optional[object] = None   # which problems of the batch are logged: None = problem 0, an iterable of indices, or "all"
    sink: Optional[object] = None       # callable(str); None = print (the reference's TINYOPT_LOG writes to std::cout, log.h:23)


@dataclass
class Options:
    """tinyopt::Options (options.h:18-156).  ``max_duration_ms``, ``stop_callback`` and ``stop_callback2`` are
    host-side controls: when any of them is set, ``Optimize`` runs the loop through the stepping form and evaluates
    them between iterations (optimizer.h:302-305, 529-534) — per problem: ``stop_callback(err, dx_norm2, grad_norm2)``
    / ``stop_callback2(err, dx, g)`` with numpy vectors.  ``log.enable`` (off by default here) prints the reference's
    per-iteration line for the chosen problems through the same stepping form (``log.print_max_stdev`` / ``print_J_jet`` /
    ``print_failure`` are not mirrored)."""
    LevenbergMarquardt = 0
    GaussNewton = 1
    GradientDescent = 2   # scalar cost models only (JitResidual kind="cost" / "cost_grad"): optimize.h:59-72
    LBFGS = 3             # scalar cost models only: limited-memory BFGS with an Armijo line search (``lbfgs``)
    solver_type: int = 0
    check_final_cost: bool = False
    use_step_quality_approx: bool = False
    grad_clipping: float = 0.0
    hessian: _Hessian = field(default_factory=_Hessian)
    cost: _CostScaling = field(default_factory=_CostScaling)
    max_iters: int = 50
    min_error: float = 1e-12
    min_rerr_dec: float = 1e-10
    min_step_norm2: float = 1e-14
    min_grad_norm2: float = 1e-18
    max_total_failures: int = 0
    max_consec_failures: int = 5
    max_duration_ms: float = 0.0               # options.h:96; 0 = no limit
    stop_callback: Optional[object] = None     # options.h:97-101  bool(err, |dx|^2, |g|^2)
    stop_callback2: Optional[object] = None    # options.h:102-106 bool(err, dx, g)
    lm: _LM = field(default_factory=_LM)
    gd: _GD = field(default_factory=_GD)
    log: _Log = field(default_factory=_Log)
    lbfgs: _LBFGS = field(default_factory=_LBFGS)   # (not part of to_pod(): toa_lbfgs_options travels beside toa_options)

    def has_host_controls(self) -> bool:
        return self.max_duration_ms > 0 or self.stop_callback is not None or self.stop_callback2 is not None or self.log.enable

    @staticmethod
    def benchmark() -> "Options":
        """benchmarks/options.h:10-27 CreateOptions()."""
        o = Options()
        o.max_iters = 10
        o.min_error = 0.0
        o.min_rerr_dec = 1e-12
        o.min_step_norm2 = 1e-16
        o.max_consec_failures = 3
        o.hessian.save_last = False
        return o

    def to_pod(self) -> ToaOptions:
        p = ToaOptions()
        p.solver_type = int(self.solver_type)
        p.max_iters = int(self.max_iters)
        p.min_error = self.min_error
        p.min_rerr_dec = self.min_rerr_dec
        p.min_step_norm2 = self.min_step_norm2
        p.min_grad_norm2 = self.min_grad_norm2
        p.max_total_failures = int(self.max_total_failures)
        p.max_consec_failures = int(self.max_consec_failures)
        p.damping_init = self.lm.damping_init
        p.damping_min, p.damping_max = self.lm.damping_range
        p.good_factor = self.lm.good_factor
        p.bad_factor = self.lm.bad_factor
        p.grad_clipping = self.grad_clipping
        p.check_min_H_diag = self.hessian.check_min_H_diag
        p.check_final_cost = int(self.check_final_cost)
        p.use_step_quality_approx = int(self.use_step_quality_approx)
        p.use_ldlt = int(self.hessian.use_ldlt)
        p.H_is_full = int(self.hessian.H_is_full)
        p.save_last = int(self.hessian.save_last)
        p.use_squared_norm = int(self.cost.use_squared_norm)
        p.downscale_by_2 = int(self.cost.downscale_by_2)
        p.normalize = int(self.cost.normalize)
        return p


_GRADIENT_DESCENT = Options.GradientDescent
_LBFGS_SOLVER = Options.LBFGS


def _dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.float64:
        return F64
    raise ValueError("dtype must be torch.float32 or torch.float64")  # reference: Scalar is float/double


class Context:
    """Owns a C-ABI handle bound to one GPU and torch's current stream on it."""

    def __init__(self, device: Optional[int] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("tinyopt_amd needs a ROCm GPU (MI355X / gfx950); there is no CPU path")
        self.lib = _capi.load()
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.stream = torch.cuda.current_stream(self.device)
        h = C.c_void_p()
        check(self.lib.toa_create(C.byref(h), self.device, C.c_void_p(self.stream.cuda_stream)))
        self.h = h

    def info(self):
        cus, khz = C.c_int(), C.c_int()
        name = C.create_string_buffer(128)
        check(self.lib.toa_device_info(self.h, C.byref(cus), C.byref(khz), name, 128))
        return {"num_cus": cus.value, "clock_khz": khz.value, "name": name.value.decode()}

    def hbm_read_GBps(self, tensor, reps: int = 5) -> float:
        """Measured streaming-read rate over `tensor`'s bytes (the STREAM-like ceiling of SURVEY §8d)."""
        out = C.c_double()
        check(self.lib.toa_hbm_read_probe(self.h, C.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size(),
                                          int(reps), C.byref(out)))
        return out.value

    def llc_read_GBps(self, tensor, max_bytes: int = 192 << 20) -> float:
        """Measured re-read rate of a working set that fits the Infinity Cache (the first `max_bytes` of `tensor`)."""
        out = C.c_double()
        nbytes = min(tensor.numel() * tensor.element_size(), int(max_bytes))
        check(self.lib.toa_llc_read_probe(self.h, C.c_void_p(tensor.data_ptr()), nbytes, C.byref(out)))
        return out.value

    def set_tuning(self, **kw) -> None:
        """The A/B arms of the library (include/tinyopt_amd.h toa_tuning) as typed per-handle state: ``ctx.set_tuning(memo_off=1)``;
        no arguments = the library's own choices.  The product reads no environment variable."""
        t = _capi.ToaTuning()
        for k, v in kw.items():
            if k == "reserved" or not hasattr(t, k):
                raise ValueError(f"unknown tuning field {k!r}")
            setattr(t, k, int(v))
        check(self.lib.toa_set_tuning(self.h, C.byref(t) if kw else None))
        self._se3_l2 = int(kw.get("se3_reproj_header_l2", 0))   # (what _apply_loss last left in that field: it only calls when it changes)

    def get_tuning(self) -> dict:
        t = _capi.ToaTuning()
        check(self.lib.toa_get_tuning(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "reserved"}

    def tuning(self, **kw):
        """``with ctx.tuning(coop_off=1): ...`` — the fields set for the block, the previous state restored after it."""
        @contextlib.contextmanager
        def cm():
            old = self.get_tuning()
            self.set_tuning(**{**old, **kw})
            try:
                yield self
            finally:
                self.set_tuning(**old) if any(old.values()) else self.set_tuning()
        return cm()

    def debug_timeline(self, path: Optional[str]) -> None:
        check(self.lib.toa_debug_timeline(self.h, path.encode() if path else None))

    def close(self):
        if getattr(self, "h", None):
            self.lib.toa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device: Optional[int] = None) -> Context:
    dev = torch.cuda.current_device() if device is None else int(device)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    if key not in _default_ctx:
        _default_ctx[key] = Context(dev)
    return _default_ctx[key]


def dense_row_layout(dtype: torch.dtype, n: int, m: int):
    lib = _capi.load()
    nb, thin, rs, m4 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    nbytes = C.c_size_t()
    check(lib.toa_dense_row_layout(_dtype_code(dtype), n, m, C.byref(nb), C.byref(thin), C.byref(rs), C.byref(m4),
                                   C.byref(nbytes)))
    rsm = rs.value - thin.value
    nmr = 16 * nb.value if thin.value else n
    return {"nb": nb.value, "thin": thin.value, "row_stride": rs.value, "rows_padded": m4.value,
            "bytes_per_problem": nbytes.value,
            # physical positions inside a packed row (mirrors DenseRowLayout::pos_col / pos_b)
            "pos_cols": [j if j < nmr else rsm + (j - nmr) for j in range(n)],
            "pos_b": (rs.value - 1) if thin.value else (rsm - 1)}


class _Model:
    """What every device model is to the entry points.  ``route``: which family of library entries takes it ("builtin": the compiled-in
    ``model_id`` families, "ba", "ba_lists", "jit": a bound run-time model, see ``_JitBatch``)."""
    route = "builtin"
    model_id = None
    loss, th = None, 0.0
    prior = None        # (mu, W, rows): rows = 0 the diagonal form
    bounds = None       # (lo, hi)
    shared = None       # a bound run-time model with shared_scalars: the batch's one table [items, shared_scalars]
    ragged = large_n = header_l2 = False
    xdim = functools.cached_property(lambda self: self.n)   # scalars of x per problem, where a model does not say

    def _head(self, ctx: "Context", x: torch.Tensor) -> tuple:
        """What every library entry over a batch starts with: the handle, the batch, x."""
        return (ctx.h, self.model_id, _dtype_code(x.dtype), self.n, self.m, x.shape[0], self.packed.data_ptr(), x.data_ptr())


class _LossMixin(_Model):
    """Models whose residual items can be wrapped in one of the reference's M-estimators (losses/robust_norms.h:32-316):
    ``model.with_loss("huber", th)`` is the device counterpart of calling ``losses::Huber(n2, th*th, true)`` on each
    residual's squared norm inside the cost functor (docs/API.md:396-411).  cost += l, the item's J^T J and J^T r are
    scaled by s = dl/dn2, and Output.final_inlier_ratio reports the residuals with n2 <= th^2 (cost.h:84-95)."""

    def with_loss(self, loss: Optional[str], th: float = 0.0):
        if loss is not None and loss not in LOSS_KINDS:
            raise ValueError(f"unknown loss {loss!r}; one of {sorted(LOSS_KINDS)}")
        if loss not in (None, "l2") and self.large_n:
            _refuse_large_n("no M-estimator (with_loss): the pipeline's loss is per row, an item's is on its squared norm")
        if loss not in (None, "l2") and _is_cost_hess(self):
            _refuse_cost_hess("no M-estimator (with_loss): a scalar cost has no residuals to robustify")
        if loss not in (None, "l2") and _is_cost_ggn(self):
            _refuse_cost_ggn("no M-estimator (with_loss): a scalar cost has no residuals to robustify")
        if loss not in (None, "l2") and _is_cost_ggn_multi(self):
            _refuse_cost_ggn_multi("no M-estimator (with_loss): a scalar cost has no residuals to robustify")
        m = copy.copy(self)          # shares the device data
        m.loss, m.th = (loss if loss not in (None, "l2") else None), float(th)
        return m


class _ConstantMixin(_Model):
    """The two bundle-adjustment families: ``model.with_constant(cameras=..., points=...)`` holds cameras and points constant (DESIGN
    section 17; `toa_ba_run_constant` / `toa_ba_lists_run_constant`) — gauge fixing (the first camera, or two), localisation against a
    known map (every point), structure-only refinement (every camera), incremental mapping (the old key-frames and their points).
    ``cameras``: bool or uint8, [P, C], or [C] for every scene of the batch; ``points``: [P, N] or [N]; non-zero = constant; None =
    none of that kind.  A constant block's tangent entries leave the system on every Build (gradient 0, rows and columns of the
    Hessian 0, diagonal 1, before clipping, the diagonal check and the damping), its step is exactly 0 and its stored pose / point
    is never written: bit for bit the caller's after the solve.  Cost, residual count, inliers and the M-estimator are untouched.
    Returns a copy that shares the device data, as ``with_loss`` does, and composes with it; a model without flags makes the calls
    it always made."""
    constant = None     # (camera flags [P, C] uint8 or None, point flags [P, N] uint8 or None)

    def with_constant(self, cameras: Optional[torch.Tensor] = None, points: Optional[torch.Tensor] = None):
        dev = (self.packed if self.route == "ba" else self.intr).device

        def flags(t, count, what, letter):
            if t is None:
                return None
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"with_constant: {what} must be a bool or uint8 tensor")
            if t.dim() == 1:
                t = t.unsqueeze(0).expand(self.P, -1)
            if tuple(t.shape) != (self.P, count):
                raise ValueError(f"with_constant: {what} must be [P, {letter}] = [{self.P}, {count}] or [{letter}] = [{count}], not {list(t.shape)}")
            return t.to(device=dev, dtype=torch.uint8).contiguous()
        cam, pts = flags(cameras, self.ncam, "cameras", "C"), flags(points, self.npts, "points", "N")
        m = copy.copy(self)          # shares the device data
        m.constant = None if cam is None and pts is None else (cam, pts)
        return m

    def _constant_pod(self) -> ToaBaConstant:
        pod = ToaBaConstant()
        cam, pts = self.constant
        pod.cam_dev = cam.data_ptr() if cam is not None else None
        pod.pt_dev = pts.data_ptr() if pts is not None else None
        return pod


class _PriorMixin(_Model):
    """Bound run-time models that take a Gaussian prior beside their items: ``model.with_prior(mu, W)`` — per problem
    ``r = W (x - mu)`` appended to the items' residuals after every pass (cost += |r|^2, g += W^T r, H += W^T W, k more
    residuals), what a hand-written Accumulate callback of the reference adds at its end.  ``mu``: [P, n].  ``W``: [P, n] is the
    diagonal form (``W = 1 / sigma``: the reference's GaussianPrior, k = n), [P, k, n] with 1 <= k <= n the full form (``W = U``:
    MahaPrior, tests/cov.cpp:96).  The prior is never passed through ``with_loss``'s M-estimator and its residuals count as inliers;
    ``Output.Covariance()`` of a prior'd run is the posterior covariance.  Composes with ``with_loss``.  Euclidean residual models
    only; no ``splits`` (and never the automatic row-split), no host controls, no ``Optimizer``, no ``Eval`` / ``CalculateJac`` /
    ``CheckGradient`` (those are about the model's own rows)."""
    def with_prior(self, mu: torch.Tensor, W: torch.Tensor):
        res = self.res
        if self.large_n:
            _refuse_large_n("no Gaussian prior (with_prior)")
        if _is_cost_hess(self):
            _refuse_cost_hess("no Gaussian prior (with_prior): a prior is a block of residuals, and it has none")
        if _is_cost_ggn(self):
            _refuse_cost_ggn("no Gaussian prior (with_prior): hand a ridge term over as extra items whose J is a unit vector")
        if res.kind in JitResidual.COST_KINDS:
            _refuse_prior('a scalar cost model (kind="cost" / "cost_grad", GradientDescent) has no residuals to add a prior to')
        if res.manifold != "euclid":
            _refuse_prior(f'manifold={res.manifold!r}: x - mu is not the manifold\'s minus (Euclidean parameters only)')
        if not isinstance(mu, torch.Tensor) or not isinstance(W, torch.Tensor):
            raise ValueError("with_prior: mu and W must be tensors")
        P, n = self.P, self.n
        if tuple(mu.shape) != (P, n):
            raise ValueError(f"with_prior: mu must be [P, n] = [{P}, {n}], not {list(mu.shape)}")
        if W.dim() == 2:
            if tuple(W.shape) != (P, n):
                raise ValueError(f"with_prior: a diagonal W must be [P, n] = [{P}, {n}], not {list(W.shape)}")
            rows = 0
        elif W.dim() == 3:
            if W.shape[0] != P or W.shape[2] != n:
                raise ValueError(f"with_prior: a full W must be [P, k, n] = [{P}, k, {n}], not {list(W.shape)}")
            rows = int(W.shape[1])
            if rows < 1 or rows > n:
                raise ValueError(f"with_prior: a full W has 1 <= k <= n = {n} rows, not {rows}")
        else:
            raise ValueError(f"with_prior: W must be [P, n] (diagonal) or [P, k, n] (full), not {W.dim()}-dimensional")
        for name, t in (("mu", mu), ("W", W)):
            if t.dtype != self.dtype:
                raise ValueError(f"with_prior: {name} must have the model's dtype {self.dtype}, not {t.dtype}")
            if t.device != self._prior_device():
                raise ValueError(f"with_prior: {name} must be on the model's device {self._prior_device()}, not {t.device}")
        m = copy.copy(self)          # shares the device data
        m.prior = (mu.contiguous(), W.contiguous(), rows)
        return m

    def _prior_pod(self):
        pod = ToaPrior()
        pod.mu_dev, pod.W_dev, pod.rows = self.prior[0].data_ptr(), self.prior[1].data_ptr(), self.prior[2]
        return pod


class _BoundsMixin(_Model):
    """Bound run-time models that keep parameters inside a box: ``model.with_bounds(lo, hi)`` — per problem ``lo[p, j] <= x[p, j] <=
    hi[p, j]``, ``[P, n]`` tensors of the model's dtype and device; ``None`` for a side means no bound there (-inf / +inf), and
    ``lo[p, j] == hi[p, j]`` holds parameter j of problem p constant.  x0 is clipped into the box before the first Build; after every
    Build the parameters that sit on a bound with the gradient pointing outward (and the fixed ones) are taken out of the system
    (g_j = 0, row and column j of H zero, H_jj = 1), so their step is 0 and ``min_grad_norm2`` tests the projected gradient; every
    step is clipped, and a roll-back undoes the clipped step.  Every x the solve visits and returns is inside the box exactly.
    ``Output.final_hessian`` is the projected matrix of the last Build, so ``Output.Covariance()`` is the inverse of the free block
    for the free parameters and 1 on the diagonal of the active ones.  Clip-and-reject, not a trust-region reflection: with a small
    ``max_consec_failures`` a solve can stop with kMaxConsecNoDecr short of the constrained optimum — raise it (30) for hard boxes.
    Composes with ``with_loss`` and ``with_prior`` in any order.  Euclidean residual models only; no ``splits`` (and never the
    automatic row-split), no host controls, no ``Optimizer``, no ``Eval`` / ``CalculateJac`` / ``CheckGradient``."""
    def with_bounds(self, lo: Optional[torch.Tensor], hi: Optional[torch.Tensor]):
        res = self.res
        if self.large_n:
            _refuse_large_n("no box bounds (with_bounds)")
        if _is_cost_hess(self):
            _refuse_cost_hess("no box bounds (with_bounds): they project the Gauss-Newton system of a residual model")
        if _is_cost_ggn(self):
            _refuse_cost_ggn("no box bounds (with_bounds)")
        if _is_cost_ggn_multi(self):
            _refuse_cost_ggn_multi("no box bounds (with_bounds)")
        if res.kind in JitResidual.COST_KINDS:
            _refuse_bounds('a scalar cost model (kind="cost" / "cost_grad", GradientDescent) has no Gauss-Newton system to project')
        if res.manifold != "euclid":
            _refuse_bounds(f'manifold={res.manifold!r}: a box on the tangent is not a box on the parameter (Euclidean parameters only)')
        P, n = self.P, self.n
        dev = self._prior_device()
        sides = []
        for name, t, fill in (("lo", lo, float("-inf")), ("hi", hi, float("inf"))):
            if t is None:
                t = torch.full((P, n), fill, dtype=self.dtype, device=dev)
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"with_bounds: {name} must be a tensor or None")
            if tuple(t.shape) != (P, n):
                raise ValueError(f"with_bounds: {name} must be [P, n] = [{P}, {n}], not {list(t.shape)}")
            if t.dtype != self.dtype:
                raise ValueError(f"with_bounds: {name} must have the model's dtype {self.dtype}, not {t.dtype}")
            if t.device != dev:
                raise ValueError(f"with_bounds: {name} must be on the model's device {dev}, not {t.device}")
            sides.append(t.contiguous())
        # one device reduction, here and never per solve (a NaN fails the comparison)
        if P * n > 0 and not bool((sides[0] <= sides[1]).all()):
            raise ValueError("with_bounds: lo <= hi must hold for every parameter of every problem, without NaN")
        m = copy.copy(self)          # shares the device data
        m.bounds = (sides[0], sides[1])
        return m

    def _bounds_pod(self):
        pod = ToaBounds()
        pod.lo_dev, pod.hi_dev = self.bounds[0].data_ptr(), self.bounds[1].data_ptr()
        return pod


class _JitBatch(_LossMixin, _PriorMixin, _BoundsMixin):
    """A bound run-time model, uniform (``JitModel``) or ragged (``RaggedJitModel``), says here once what it hands the library — as
    jit.hip's JitBatch does on the other side: ``_head`` (the handle, the batch, x), ``_extras`` (what follows x) and, with ``ragged``,
    the key that picks the member of an entry family in ``_JIT_ENTRIES``.  A new per-model extra is one more branch of ``_extras`` and
    one more column of that table."""
    route, _plain = "jit", (False, None)
    large_n = functools.cached_property(lambda self: getattr(self.res, "large_n", False))   # (tests/test_cpu_prior.py binds a residual without one)

    def _extras(self):
        """(the key (ragged, extra) of _JIT_ENTRIES, the extra's arguments): the bounds pod and the prior's or NULL, or the prior pod, or
        nothing.  A byref holds its pod, so the tuple keeps them alive for the call."""
        if self.shared is not None:   # (uniform only) the table stands in _head, behind the data; bounds and prior follow x, each or NULL
            return (False, "shared"), (C.byref(self._bounds_pod()) if self.bounds is not None else None,
                                       C.byref(self._prior_pod()) if self.prior is not None else None)
        if self.bounds is not None:
            return (self.ragged, "bounds"), (C.byref(self._bounds_pod()), C.byref(self._prior_pod()) if self.prior is not None else None)
        if self.prior is not None:
            return (self.ragged, "prior"), (C.byref(self._prior_pod()),)
        return self._plain, ()


_JIT_ENTRIES = {   # entry family -> (ragged, extra) -> the library entry
    "lm_run": {(False, "shared"): "toa_jit_lm_run_shared", (False, "prior"): "toa_jit_lm_run_prior", (False, "bounds"): "toa_jit_lm_run_bounds",
               (True, None): "toa_jit_lm_run_ragged", (True, "prior"): "toa_jit_lm_run_ragged_prior", (True, "bounds"): "toa_jit_lm_run_ragged_bounds"},
    "gd_run": {(False, None): "toa_jit_gd_run", (True, None): "toa_jit_gd_run_ragged"},
    "lbfgs_run": {(False, None): "toa_jit_lbfgs_run", (True, None): "toa_jit_lbfgs_run_ragged"},
    "accumulate": {(False, None): "toa_jit_accumulate", (False, "shared"): "toa_jit_accumulate_shared", (False, "prior"): "toa_jit_accumulate_prior", (False, "bounds"): "toa_jit_accumulate_bounds",
                   (True, None): "toa_jit_accumulate_ragged", (True, "prior"): "toa_jit_accumulate_ragged_prior",
                   (True, "bounds"): "toa_jit_accumulate_ragged_bounds"},
    "eval": {(False, None): "toa_jit_eval", (True, None): "toa_jit_eval_ragged"},
}
_STEP_ENTRIES = {False: ("toa_lm_begin", "toa_lm_step", "toa_lm_stop"), True: ("toa_jit_lm_begin", "toa_jit_lm_step", "toa_jit_lm_stop")}   # by route == "jit"


def _refuse_bounds(what: str):
    raise ValueError(f"box bounds (with_bounds) stand on a Euclidean residual model in the one-launch form only: {what}")


def _refuse_large_n(what: str):
    raise ValueError(f"a model compiled with large_n=True runs on the launch-per-phase pipeline through Optimize (LM / GN), accumulate, Eval "
                     f"and CalculateJac only: {what}")


def _refuse_prior(what: str):
    raise ValueError(f"a Gaussian prior (with_prior) stands beside a Euclidean residual model in the one-launch form only: {what}")


def _refuse_cost_hess(what: str):
    raise ValueError(f'a second-order scalar cost (kind="cost_hess") runs in the uniform one-launch form through Optimize (LM / GN), accumulate '
                     f"and CheckGradient only: {what}")


def _is_cost_hess(cost) -> bool:
    return cost.route == "jit" and getattr(cost.res, "kind", None) == "cost_hess"


def _refuse_cost_ggn(what: str):
    raise ValueError(f'a rank-one second-order scalar cost (kind="cost_ggn") runs in the uniform one-launch form through Optimize (LM / GN), '
                     f"accumulate and CheckGradient only: {what}")


def _is_cost_ggn(cost) -> bool:
    return cost.route == "jit" and getattr(cost.res, "kind", None) == "cost_ggn"


def _refuse_cost_ggn_multi(what: str):
    raise ValueError(f'a multi-output second-order scalar cost (kind="cost_ggn_multi") runs in the uniform one-launch form through Optimize '
                     f"(LM / GN), accumulate and CheckGradient only, with with_prior and a shared table: {what}")


def _is_cost_ggn_multi(cost) -> bool:
    return cost.route == "jit" and getattr(cost.res, "kind", None) == "cost_ggn_multi"


def _refuse_shared(what: str):
    raise ValueError(f"a model with a shared item table (shared_scalars > 0) runs in the uniform one-launch form through Optimize (LM / GN) and "
                     f"accumulate only: {what}")


def _refuse_ragged(what: str):
    raise ValueError(f"a ragged batch (bind_ragged) runs in the one-launch form only: {what}")


def _refuse_plainly(what: str):
    raise ValueError(what)


# Every sentence a refusal of an entry point can end in, once: (what refuses, what is refused) -> the sentence.  What refuses is a name
# of _who(cost); the first four speak through their _refuse_* prefix.  Each entry point consults the pairs of its own *_REFUSES tuple
# in that tuple's order and raises the first that applies, before its first library call and before it allocates anything.  A new
# refusal is one line here and one pair in the order of each entry point that makes it.
_NO_SPLITS, _NO_HOST, _NO_GD, _NO_STEPPING = ("no row-split form (splits)", "no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)",
                                              "no GradientDescent", "no stepping form (Optimizer)")
_BA_ONE_LAUNCH = "BundleAdjustment runs as one launch per solve: no stop callbacks / splits"
_BA_LISTS_ONE_LAUNCH = "BundleAdjustmentLists: no stop callbacks / splits (max_duration_ms is honoured)"
_NUMERIC_ONE_LAUNCH = ("a numerically differentiated model (diff=...) runs as one launch per solve: no stop callbacks, max_duration_ms, "
                       "log line or splits (it has no stepping and no row-split form)")
_REFUSALS = {
    **{(who, what): text for who in ("ragged", "bounds", "prior", "large_n")
       for what, text in (("splits", _NO_SPLITS), ("host", _NO_HOST), ("gd", _NO_GD), ("Optimizer", _NO_STEPPING))},
    ("large_n", "splits"): _NO_SPLITS + ": the pipeline already spreads a problem's rows over the device",   # (says more than the four share)
    ("large_n", "capture"): "no stream capture of the solve (the host enqueues its passes)",
    ("large_n", "CheckGradient"): "no CheckGradient (its numeric twin is a one-wavefront model of at most 63 parameters)",
    ("ragged", "CheckGradient"): "no CheckGradient (check the model on a uniform batch: JitResidual.bind)",
    **{(who, "CheckGradient"): f"no CheckGradient (it checks the model's own rows: check the model without the {who})" for who in ("bounds", "prior")},
    **{(who, what): f"no {what} (it returns the model's own rows: evaluate the model without the {who})"
       for who in ("bounds", "prior") for what in ("Eval", "CalculateJac")},
    ("uniform", "keep_order"): "keep_order is the queue order of a ragged batch (JitResidual.bind_ragged)",
    ("ba", "host"): _BA_ONE_LAUNCH, ("ba", "splits"): _BA_ONE_LAUNCH,
    ("ba_lists", "callbacks"): _BA_LISTS_ONE_LAUNCH, ("ba_lists", "splits"): _BA_LISTS_ONE_LAUNCH,
    ("numeric", "host"): _NUMERIC_ONE_LAUNCH, ("numeric", "splits"): _NUMERIC_ONE_LAUNCH,
    ("numeric", "Optimizer"): "a numerically differentiated model (diff=...) has no stepping form",
    ("gd_cost", "host"): "GradientDescent runs as one launch per solve: stop callbacks, max_duration_ms and the log line are not "
                         "supported on this path (no stepping form for scalar costs)",
    ("gd_cost", "splits"): "GradientDescent: no row-split form (splits)",
    ("stepping", "out with host controls"): "stop callbacks / max_duration_ms run through the stepping form: splits / out are not taken",
    ("cost_hess", "gd"): _NO_GD + ": the reference throws for f(x, grad, H) under GradientDescent too (optimize.h:59-75)",
    ("cost_hess", "splits"): _NO_SPLITS + ": its Hessian is no Gram of rows to split", ("cost_hess", "host"): _NO_HOST,
    ("cost_hess", "Optimizer"): _NO_STEPPING,
    # L-BFGS (Options.LBFGS): who may not ask for it, and what a cost model may not ask for beside it
    ("not_cost", "lbfgs"): 'L-BFGS (Options.LBFGS) needs a scalar cost model (JitResidual kind="cost" / "cost_grad"): a residual model runs under LM / GN',
    ("cost_hess", "lbfgs"): "no L-BFGS: it builds its own curvature from gradients; f(x, grad, H) runs under LM / GN",
    **{(who, "lbfgs"): "no L-BFGS" for who in ("prior", "large_n")},
    ("bounds", "lbfgs"): "no L-BFGS (and L-BFGS has no box bounds: this is not L-BFGS-B)",
    ("lbfgs_cost", "host"): "L-BFGS runs as one launch per solve: stop callbacks, max_duration_ms and the log line are not supported on this "
                            "path (no stepping form for scalar costs)",
    ("lbfgs_cost", "splits"): "L-BFGS: no row-split form (splits)",
    ("lbfgs_cost", "grad_clipping"): "L-BFGS: grad_clipping must be 0 (a clipped gradient makes the pairs' y = g - g_acc meaningless)",
    ("lbfgs_cost", "lbfgs.history"): "L-BFGS: lbfgs.history must be in 1 .. 16",
    ("lbfgs_cost", "lbfgs.c1"): "L-BFGS: lbfgs.c1 (the Armijo constant) must be in (0, 1)",
    ("lbfgs_cost", "lbfgs.shrink"): "L-BFGS: lbfgs.shrink (the backtracking factor) must be in (0, 1)",
    ("lbfgs", "Optimizer"): "L-BFGS (Options.LBFGS) has no stepping form (Optimizer): run it through Optimize",
    **{("cost_hess", what): f"no {what} (it has no residual rows: accumulate returns its value, its gradient and its Hessian)" for what in ("Eval", "CalculateJac")},
    # a rank-one second-order scalar cost (kind="cost_ggn"): LM / GN in the uniform one-launch form
    ("cost_ggn", "gd"): _NO_GD + ': run the same cost as kind="cost_grad"',
    ("cost_ggn", "lbfgs"): 'no L-BFGS: run the same cost as kind="cost_grad"',
    ("cost_ggn", "splits"): _NO_SPLITS, ("cost_ggn", "host"): _NO_HOST, ("cost_ggn", "Optimizer"): _NO_STEPPING,
    **{("cost_ggn", what): f"no {what} (it has no residual rows: accumulate returns its value, its gradient and its Hessian)" for what in ("Eval", "CalculateJac")},
    # a multi-output second-order scalar cost (kind="cost_ggn_multi"): LM / GN in the uniform one-launch form, with its prior and a table
    ("cost_ggn_multi", "gd"): _NO_GD + ': run the same cost as kind="cost_grad"',
    ("cost_ggn_multi", "lbfgs"): 'no L-BFGS: run the same cost as kind="cost_grad"',
    ("cost_ggn_multi", "splits"): _NO_SPLITS, ("cost_ggn_multi", "host"): _NO_HOST, ("cost_ggn_multi", "Optimizer"): _NO_STEPPING,
    **{("cost_ggn_multi", what): f"no {what} (it has no residual rows: accumulate returns its value, its gradient and its Hessian)" for what in ("Eval", "CalculateJac")},
    # a model with a shared item table (shared_scalars > 0): LM / GN and accumulate in the uniform one-launch form
    ("shared", "splits"): _NO_SPLITS, ("shared", "host"): _NO_HOST, ("shared", "gd"): _NO_GD, ("shared", "lbfgs"): "no L-BFGS",
    ("shared", "Optimizer"): _NO_STEPPING,
    ("shared", "CheckGradient"): 'no CheckGradient (compare accumulate of a kind="accumulate" body with accumulate of its residuals under '
                                 'diff="central", both with the table)',
    **{("shared", what): f"no {what} (its kernels read replicated items: bind the table copied into every problem's items)" for what in ("Eval", "CalculateJac")},
}
_REFUSE_AS = {"ragged": _refuse_ragged, "bounds": _refuse_bounds, "prior": _refuse_prior, "large_n": _refuse_large_n, "cost_hess": _refuse_cost_hess,
              "cost_ggn": _refuse_cost_ggn, "cost_ggn_multi": _refuse_cost_ggn_multi, "shared": _refuse_shared}
_OPTIMIZE_REFUSES = (("shared", "lbfgs"), ("shared", "gd"), ("shared", "splits"), ("shared", "host"),
                     ("cost_ggn", "lbfgs"), ("cost_ggn", "gd"), ("cost_ggn", "splits"), ("cost_ggn", "host"),
                     ("cost_ggn_multi", "lbfgs"), ("cost_ggn_multi", "gd"), ("cost_ggn_multi", "splits"), ("cost_ggn_multi", "host"),
                     ("cost_hess", "lbfgs"), ("bounds", "lbfgs"), ("prior", "lbfgs"), ("large_n", "lbfgs"), ("not_cost", "lbfgs"),
                     ("lbfgs_cost", "host"), ("lbfgs_cost", "splits"), ("lbfgs_cost", "grad_clipping"), ("lbfgs_cost", "lbfgs.history"),
                     ("lbfgs_cost", "lbfgs.c1"), ("lbfgs_cost", "lbfgs.shrink"),
                     ("cost_hess", "gd"), ("cost_hess", "splits"), ("cost_hess", "host"), ("ragged", "splits"), ("ragged", "host"), ("uniform", "keep_order"), ("ba", "host"), ("ba", "splits"),
                     ("ba_lists", "callbacks"), ("ba_lists", "splits"),
                     ("bounds", "splits"), ("bounds", "host"), ("bounds", "gd"), ("prior", "splits"), ("prior", "host"), ("prior", "gd"),
                     ("large_n", "splits"), ("large_n", "host"), ("large_n", "gd"), ("large_n", "capture"), ("numeric", "host"), ("numeric", "splits"),
                     ("gd_cost", "host"), ("gd_cost", "splits"), ("stepping", "out with host controls"))
_OPTIMIZER_REFUSES = tuple((who, "Optimizer") for who in ("shared", "lbfgs", "cost_hess", "cost_ggn", "cost_ggn_multi", "ragged", "bounds", "prior", "numeric", "large_n"))
_CHECK_GRADIENT_REFUSES = tuple((who, "CheckGradient") for who in ("shared", "bounds", "prior", "ragged", "large_n"))
_ROWS_REFUSES = {what: (("shared", what), ("cost_hess", what), ("cost_ggn", what), ("cost_ggn_multi", what), ("bounds", what), ("prior", what)) for what in ("Eval", "CalculateJac")}


def _who(cost, gd: bool = False, lbfgs: bool = False) -> set:
    """The names under which ``cost`` can refuse something (the first column of _REFUSALS); ``gd`` / ``lbfgs``: the options ask for
    GradientDescent / L-BFGS."""
    who = {cost.route, "ragged" if cost.ragged else "uniform"}
    if cost.bounds is not None:
        who.add("bounds")
    if cost.prior is not None:
        who.add("prior")
    if cost.large_n:
        who.add("large_n")
    if cost.shared is not None:
        who.add("shared")
    if cost.route == "jit" and cost.res.diff != "ad":
        who.add("numeric")
    if gd and cost.route == "jit" and cost.res.kind in JitResidual.COST_KINDS:
        who.add("gd_cost")
    if lbfgs:   # a first-order cost model, or anything else
        who.add("lbfgs_cost" if cost.route == "jit" and cost.res.kind in JitResidual.COST_KINDS else "not_cost")
    if _is_cost_hess(cost):
        who.add("cost_hess")
    if _is_cost_ggn(cost):
        who.add("cost_ggn")
    if _is_cost_ggn_multi(cost):
        who.add("cost_ggn_multi")
    if cost.route != "ba_lists":   # (it honours max_duration_ms itself; every other family goes to the stepping form for host controls)
        who.add("stepping")
    return who


def _refuse(order, who, asked) -> None:
    """Raise the first refusal of ``order`` whose first half is in ``who`` and whose second is in ``asked``."""
    for key in order:
        if key[0] in who and key[1] in asked:
            _REFUSE_AS.get(key[0], _refuse_plainly)(_REFUSALS[key])


def _apply_loss(ctx: "Context", cost) -> None:
    """The handle carries the cost functor's M-estimator (toa_set_loss): set it from the model before every launch."""
    # SE3Reproj carries its loss in the data header: a model without one runs the kernels without the M-estimator branch (toa_tuning::
    # se3_reproj_header_l2; fp64: 308 -> 216 registers) — the field follows the model, a host call only when it changes
    want = 1 if cost.header_l2 else 0
    if getattr(ctx, "_se3_l2", 0) != want:
        ctx.set_tuning(**{**ctx.get_tuning(), "se3_reproj_header_l2": want})
    kind = cost.loss
    if kind is None:
        check(ctx.lib.toa_set_loss(ctx.h, 0, 0.0))
    else:
        check(ctx.lib.toa_set_loss(ctx.h, LOSS_KINDS[kind], float(cost.th) * float(cost.th)))


class DenseRow(_LossMixin):
    """Device residual model  r_i(x) = a_i.x + 0.1 sin(a_i.x) - b_i  for a batch of P problems.

    Plays the role of the user's cost functor in ``Optimize(x, cost)`` (a Jet-invocable residual
    functor in the reference, e.g. benchmarks/dense.cpp:56,71-74) — here a tag object that selects
    the pre-instantiated device functor and owns the problem data in HBM (packed layout).
    """
    model_id = MODEL_DENSE_ROW

    def __init__(self, packed: torch.Tensor, n: int, m: int, P: int):
        self.packed, self.n, self.m, self.P = packed, int(n), int(m), int(P)
        self.dtype = packed.dtype

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        """bytes one Accumulate/Evaluate pass must read per problem = m(n+1)sizeof(T)."""
        return self.m * (self.n + 1) * self.packed.element_size()

    @staticmethod
    def from_arrays(A: torch.Tensor, b: torch.Tensor, ctx: Optional[Context] = None) -> "DenseRow":
        """A: [P, m, n], b: [P, m] on the GPU (natural layout) -> packed layout."""
        ctx = ctx or default_context(A.device.index)
        P, m, n = A.shape
        assert b.shape == (P, m) and A.dtype == b.dtype and A.is_cuda and b.is_cuda
        A, b = A.contiguous(), b.contiguous()
        lay = dense_row_layout(A.dtype, n, m)
        packed = torch.empty(P * lay["rows_padded"] * lay["row_stride"], dtype=A.dtype, device=A.device)
        check(ctx.lib.toa_dense_row_pack(ctx.h, _dtype_code(A.dtype), n, m, P, A.data_ptr(), b.data_ptr(), packed.data_ptr()))
        return DenseRow(packed, n, m, P)

    @staticmethod
    def synthetic(P: int, n: int, m: int, dtype: torch.dtype, seed: int = 0x71940917, problem0: int = 0,
                  ctx: Optional[Context] = None):
        """Generate the SURVEY §8(d) batch directly in HBM.  Returns (model, x0, xstar)."""
        ctx = ctx or default_context()
        dev = torch.device("cuda", ctx.device)
        lay = dense_row_layout(dtype, n, m)
        packed = torch.empty(P * lay["rows_padded"] * lay["row_stride"], dtype=dtype, device=dev)
        x0 = torch.empty(P, n, dtype=dtype, device=dev)
        xstar = torch.empty(P, n, dtype=dtype, device=dev)
        check(ctx.lib.toa_dense_row_synth(ctx.h, _dtype_code(dtype), n, m, P, seed, problem0, packed.data_ptr(),
                                          x0.data_ptr(), xstar.data_ptr()))
        return DenseRow(packed, n, m, P), x0, xstar


class GaussianPrior(_Model):
    """Device residual model  r = (x - y) / sigma  (m = n) — the residual of the reference's published dense
    benchmark with the semantics of its manual Accumulate callback (benchmarks/dense.cpp:57-66):
    grad = J*res, H.diagonal() = sigma^-2, cost = res.squaredNorm() returned as a scalar (1 residual)."""
    model_id = MODEL_GAUSSIAN_PRIOR

    def __init__(self, y: torch.Tensor, sigma: torch.Tensor):
        assert y.shape == sigma.shape and y.dim() == 2 and y.is_cuda and y.dtype == sigma.dtype
        self.P, self.n = y.shape
        self.m = self.n
        self.dtype = y.dtype
        self.packed = torch.stack([y, sigma], dim=1).contiguous()  # [P][2][n]

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return 2 * self.n * self.packed.element_size()


class Sqrt2(_Model):
    """Device residual model  r = x*x - 2  (n = m = 1), tests/sqrt2.cpp:30-70."""
    model_id = MODEL_SQRT2

    def __init__(self, P: int, dtype: torch.dtype, device=None):
        self.P, self.n, self.m, self.dtype = int(P), 1, 1, dtype
        self.packed = torch.zeros(1, dtype=dtype, device=device or "cuda")  # no problem data

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return 0


class SE3Reproj(_Model):
    """Device residual model: pinhole reprojection of 3-D points under an SE3 pose.
    x is [P, 12] (rotation matrix row-major + translation); the tangent has n = 6 (upsilon, omega) and the update
    is the right-multiplicative  pose <- pose * exp(delta)  of include/tinyopt/3rdparty/traits/sophus.h:24-26.
    data: [P, 8 + 5*npts] = [f, cx, cy, loss, th2, 0,0,0 | x, y, z, u, v per point].

    loss / th: optional M-estimator on each point's squared reprojection error (the reference's
    losses/robust_norms.h:32-316): ``loss`` in LOSS_KINDS ("huber", "cauchy", ...), ``th`` the threshold in pixels
    (th2 = th*th is what the reference's functions take).  The inlier ratio lands in Output.final_inlier_ratio."""
    model_id = MODEL_SE3_REPROJ
    xdim = 12

    def __init__(self, data: torch.Tensor, npts: int, loss: Optional[str] = None, th: float = 0.0):
        assert data.dim() == 2 and data.shape[1] == 8 + 5 * npts and data.is_cuda
        self.P, self.n, self.m, self.dtype = data.shape[0], 6, 2 * int(npts), data.dtype
        self.packed = data.contiguous()
        if loss is not None:
            if self.packed.data_ptr() == data.data_ptr():
                self.packed = self.packed.clone()
            self.packed[:, 3] = float(LOSS_KINDS[loss])
            self.packed[:, 4] = float(th) * float(th)
        # (one read-back at construction: a header the caller filled in by hand may name a loss too)
        self.header_l2 = loss is None and not bool((self.packed[:, 3] != 0).any())

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return (self.m // 2) * 5 * self.packed.element_size()


class CircleFit(_LossMixin):
    """tests/circle.cpp:32-68 on the device, differentiated by forward-mode dual numbers (csrc/jet.hpp):
    x = (cx, cy, radius), one residual ||p - c||^2 - radius^2 per observed point.  obs: [P, m, 2]."""
    model_id = MODEL_CIRCLE_FIT

    def __init__(self, obs: torch.Tensor):
        assert obs.dim() == 3 and obs.shape[2] == 2 and obs.is_cuda
        self.P, self.m, self.n, self.dtype = obs.shape[0], obs.shape[1], 3, obs.dtype
        self.packed = obs.contiguous()

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return self.m * 2 * self.packed.element_size()


class BundleAdjustmentLists(_LossMixin, _ConstantMixin):
    """Bundle adjustment with VISIBILITY LISTS (`toa_ba_lists_run`): tens to hundreds of SE3 cameras, each point observed by a
    few of them — what the reference would hand to Eigen's SimplicialLDLT (math.h:266-277; README.md:30,165-167).  Same x as
    ``BundleAdjustment`` ([P, 12 C + 3 N]); the observations are a list sorted by (point, camera):
    intr [P, 4] = (f, cx, cy, 0), obs_cam / obs_pt [P, M] int32, obs_uv [P, M, 2].  ``Options.max_duration_ms`` is honoured.
    ``.with_loss("huber", th)`` puts every observation's squared reprojection error through an M-estimator (round 4);
    ``.with_constant(cameras=, points=)`` holds cameras and points constant (``_ConstantMixin``)."""
    route = "ba_lists"

    def __init__(self, intr: torch.Tensor, obs_cam: torch.Tensor, obs_pt: torch.Tensor, obs_uv: torch.Tensor, ncam: int, npts: int):
        assert intr.dim() == 2 and intr.shape[1] == 4 and intr.is_cuda
        P, M = obs_cam.shape
        assert obs_pt.shape == (P, M) and obs_uv.shape == (P, M, 2) and intr.shape[0] == P
        assert obs_cam.dtype == torch.int32 and obs_pt.dtype == torch.int32 and obs_uv.dtype == intr.dtype
        self.P, self.ncam, self.npts, self.nobs, self.dtype = P, int(ncam), int(npts), M, intr.dtype
        self.n, self.m, self.xdim = 6 * self.ncam + 3 * self.npts, 2 * M, 12 * self.ncam + 3 * self.npts
        self.intr, self.obs_cam, self.obs_pt, self.obs_uv = intr.contiguous(), obs_cam.contiguous(), obs_pt.contiguous(), obs_uv.contiguous()

    @staticmethod
    def from_dense(data, ncam: Optional[int] = None, npts: Optional[int] = None) -> "BundleAdjustmentLists":
        """From ``BundleAdjustment``'s dense layout [P, 8 + 3 C N] = [f cx cy 0.. | uv (C, N, 2) | vis (C, N)]; every scene must
        have the same number of visible observations.  ``data`` may be the ``BundleAdjustment`` model itself: its loss and its
        constant cameras / points (``with_constant``) are carried over."""
        if isinstance(data, BundleAdjustment):
            lists = BundleAdjustmentLists.from_dense(data.packed, data.ncam, data.npts)
            lists.loss, lists.th, lists.constant = data.loss, data.th, data.constant
            return lists
        P = data.shape[0]
        uv = data[:, 8:8 + 2 * ncam * npts].reshape(P, ncam, npts, 2)
        vis = data[:, 8 + 2 * ncam * npts:].reshape(P, ncam, npts) != 0
        cams, pts, uvs = [], [], []
        for p in range(P):
            v = vis[p].t().contiguous()                    # [N, C]: point-major => sorted by (point, camera)
            idx = v.nonzero(as_tuple=False)
            pts.append(idx[:, 0].to(torch.int32))
            cams.append(idx[:, 1].to(torch.int32))
            uvs.append(uv[p].permute(1, 0, 2)[v])
        if len({int(t.shape[0]) for t in pts}) != 1:
            raise ValueError("every scene must have the same number of observations")
        intr = torch.zeros(P, 4, dtype=data.dtype, device=data.device)
        intr[:, :3] = data[:, :3]
        return BundleAdjustmentLists(intr, torch.stack(cams), torch.stack(pts), torch.stack(uvs), ncam, npts)

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return self.nobs * (2 * self.obs_uv.element_size() + 8) + self.xdim * self.obs_uv.element_size()


class JitResidual:
    """A residual the library has never seen, compiled at run time: the device-side form of tinyopt's "pass any callable"
    (``Optimize(x, [](const auto& x) { return r(x); })``, optimize.h:16-33, optimizer.h:145-160, docs/API.md:21-35).

    ``body`` is the BODY of the residual as C++ source text, written like the reference's lambda and generic in its scalar
    type ``S`` (instantiated on Jet<T, n> for Accumulate — forward-mode AD, optimize_autodiff.h:91-166 — and on plain T for
    the cost-only form): ``x[j]`` parameter j (an S), ``p[k]`` the item's data scalars, ``h[k]`` the problem's header
    scalars, ``r[q]`` the item's residuals; every ceres::Jet function (sin, exp, pow, atan2, ...) is in scope.  Example, the
    circle fit of tests/circle.cpp:32-68::

        fit = ta.JitResidual("const S dx = p[0] - x[0]; const S dy = p[1] - x[1]; r[0] = dx*dx + dy*dy - x[2]*x[2];",
                             n=3, item_scalars=2, dtype=torch.float64)
        out = ta.Optimize(x, fit.bind(points), options)        # points: [P, items, 2] on the GPU

    hiprtc builds lm_fused_kernel / accumulate_kernel for JetModel<T, that functor> (2-3 s the first time; the code object is
    cached on disk — ``JitResidual.set_cache_dir`` — so a second construction of the same residual, in this or another process,
    takes milliseconds: ``from_cache``) and the code object is loaded into the process: no rebuild of libtinyopt_amd.so, and no
    source tree next to it (the kernel headers are embedded in the library).

    Round 4:
      * ``n`` up to 63 — beyond 12 parameters the functor is evaluated on chunked Jets in matrix-core operand order (the path
        of ``DenseRowAD``): one residual per item, Euclidean, no loss;
      * ``manifold="se3"`` — x is ONE pose [P, 12] (rotation matrix row-major + translation), n = 6; the body reads the pose
        through ``x[0..11]`` (Jets over the right perturbation, optimize_autodiff.h:48-77 + sophus.h:13-27) and may call
        ``se3_log<S, T>(R, t, xi)``; the update is pose <- pose * exp(delta).  tests/sophus.cpp:26-44 as a string::

            prior = ta.JitResidual(SE3_PRIOR_BODY, n=6, item_scalars=0, residuals_per_item=6, header_scalars=12, manifold="se3")

      * ``kind="accumulate"`` — a manual Accumulate callback (docs/API.md:37-57): the body fills ``r[q]`` and, inside
        ``if (want_grad) { ... }``, its own Jacobian rows ``J[q][a]`` (plain T, no AD).

    Scalar costs (the first-order half of the reference's ``Optimize``, optimize.h:59-72, solvers/gd.h) — run with
    ``options.solver_type = Options.GradientDescent`` (``options.gd.lr``); Euclidean parameters, one "residual" per item:
      * ``kind="cost"`` — ``f(x) -> scalar``: the body assigns ``c``, the item's cost term, over the scalar type ``S``
        (differentiated on Jets); the problem's cost is the sum over its items.  Logistic regression::

            logit = ta.JitResidual("S z = S(0); for (int j = 0; j < 12; ++j) z += p[j] * x[j]; "
                                   "c = log(S(1) + exp(-p[12] * z));", n=12, item_scalars=13, kind="cost", dtype=torch.float32)

      * ``kind="cost_grad"`` — ``f(x, grad) -> scalar`` (tests/unconstrained.cpp:19-42): ``c`` on plain T and, inside
        ``if (want_grad) { ... }``, the item's own gradient added to ``G[a]``.

    The same two kinds run under ``options.solver_type = Options.LBFGS``: limited-memory BFGS with a backtracking
    Armijo search — ``options.lbfgs.history`` pairs (1 .. 16, default 8) kept in the wave's LDS, ``lbfgs.c1`` (1e-4), ``lbfgs.shrink``
    (0.5) — for any n up to 63, uniform and ragged batches, no ``lr`` to tune and no Hessian to write down; x is always an accepted
    point, no final Hessian.  Refused with a sentence: every other model kind, ``with_loss``, ``with_prior``, ``with_bounds`` (no
    L-BFGS-B), ``splits``, the stepping ``Optimizer``, host controls, ``large_n``, ``grad_clipping != 0``, option values out of range.
    ``stats_lbfgs()`` describes its kernel.

    Second-order scalar costs (the reference's ``f(x, grad, H) -> cost``, optimize.h:26-57; tests/optimize_easy.cpp is written in this
    form) — ``kind="cost_hess"``, run by LM or GN over the body's OWN gradient and Hessian, which need not be a Gram: batched Newton
    for logistic and Poisson regression, maximum-likelihood fits, any GLM.  The body sees ``x[j]``, ``h[k]``, ``p[k]`` on plain T as a
    ``cost_grad`` body does; it assigns ``c``, the item's cost term, and inside ``if (want_grad) { ... }`` ADDS the item's gradient to
    ``G[a]`` and the item's Hessian to ``H(a, b)`` for ``a <= b`` (the upper triangle with the diagonal; a write with ``a > b`` is
    discarded, so a body that fills the full symmetric matrix gives the same system).  The problem's cost is the sum of its items'
    terms as ONE residual, its gradient and Hessian their sums.  ``Options.GaussNewton``, or ``lm.damping_init = 0``, is Newton's
    method; an indefinite Hessian fails the factorisation and the iteration goes through BadStep; ``hessian.save_last`` returns the
    undamped Hessian of the last Build.  Loops over ``a``, ``b`` need COMPILE-TIME bounds: ``H`` is a triangle of n (n + 1) / 2
    registers per lane, and a triangle indexed by a loop the compiler does not unroll lands in scratch memory
    (``stats()["scratch_bytes"]`` shows it).  Euclidean parameters, one cost term per item, ``diff="ad"``, 1 <= n <= 12 in float32 and
    float64.  ``Optimize`` (LM / GN), ``accumulate`` (g, the full symmetric H, cost) and ``CheckGradient`` take such a model
    (``check_H=True`` compares the body's H with central differences of the body's own gradient); GradientDescent (the reference
    throws for this signature too), ``with_loss``, ``with_prior``, ``with_bounds``, ``bind_ragged``, ``splits``, the stepping
    ``Optimizer``, host controls, ``Eval`` / ``CalculateJac``, manifolds, numeric ``diff`` and ``large_n`` are refused with a
    sentence.  Logistic regression (n = 12, an item = 12 features + the label +-1)::

        newton = ta.JitResidual('''
            T z = 0; for (int j = 0; j < 12; ++j) z += p[j] * x[j];
            const T y = p[12], e = exp(-y * z), s = T(1) / (T(1) + e);        // sigma(y z)
            c = log(T(1) + e);
            if (want_grad) {
              const T gz = -y * (T(1) - s), hz = s * (T(1) - s);
              for (int a = 0; a < 12; ++a) { G[a] += gz * p[a]; for (int b = a; b < 12; ++b) H(a, b) += hz * p[a] * p[b]; }
            }''', n=12, item_scalars=13, kind="cost_hess", dtype=torch.float64)
        out = ta.Optimize(w, newton.bind(samples), ta.Options())        # samples: [P, items, 13] on the GPU

    Rank-one second-order scalar costs — ``kind="cost_ggn"``: a cost ``c_i = phi(u_i(x))`` with a SCALAR inner function (logistic
    and Poisson regression, any GLM, any likelihood of a scalar predictor), run by LM or GN on the matrix-core Gram of the row
    models, so that Newton's method reaches 63 parameters.  The body sees ``x[j]``, ``h[k]``, ``p[k]`` on plain T; it assigns ``c``
    and, inside ``if (want_grad) { ... }``, three things: ``gs`` = dc/du, ``hs`` = the curvature weight phi''(u), and ``J[a]`` =
    (grad u)[a] for EVERY a < n (assigned, not added).  The item contributes ``g += gs J`` and ``H += w J J^T`` with ``w = hs``
    where ``hs > wmin``, ``wmin`` where ``hs <= wmin`` (2^-60 in float32, 2^-200 in float64) and NaN where ``hs`` is NaN: the
    generalised Gauss-Newton Hessian (the phi'(u) hess u term is dropped; exact where u is linear in x).  A negative or zero
    curvature contributes its gradient and, up to wmin, nothing to H, which stays positive semi-definite: a Gauss-Newton door, not
    one for indefinite Hessians (``cost_hess`` remains that).  The problem's cost is the sum of the items' ``c`` as ONE residual.
    Loops over ``a`` need COMPILE-TIME bounds (``J`` is the lane's row in registers; ``stats()["scratch_bytes"]`` shows a
    violation).  Euclidean parameters, one cost term per item, ``diff="ad"``, 1 <= n <= 63 in float32 and float64.  ``Optimize``
    (LM / GN; ``Options.GaussNewton`` or ``lm.damping_init = 0`` is Newton's method), ``accumulate`` (g, the full symmetric H, cost)
    and ``CheckGradient`` take such a model (``check_H=True`` agrees only where u is linear in x or phi' vanishes);
    GradientDescent, L-BFGS, ``with_loss``, ``with_prior``, ``with_bounds``, ``bind_ragged``, ``splits``, the stepping ``Optimizer``,
    host controls, ``Eval`` / ``CalculateJac``, manifolds, numeric ``diff`` and ``large_n`` are refused with a sentence.  Logistic
    regression at n = 50 (an item = 50 features + the label +-1)::

        newton50 = ta.JitResidual('''
            T z = 0; for (int j = 0; j < 50; ++j) z += p[j] * x[j];
            const T y = p[50], e = exp(-y * z), s = T(1) / (T(1) + e);
            c = log(T(1) + e);
            if (want_grad) { gs = -y * (T(1) - s); hs = s * (T(1) - s); for (int a = 0; a < 50; ++a) J[a] = p[a]; }''',
            n=50, item_scalars=51, kind="cost_ggn", dtype=torch.float32)

    Multi-output second-order scalar costs — ``kind="cost_ggn_multi"``: a cost ``c_i = phi(u_i(x))`` with a VECTOR
    inner function of ``K = residuals_per_item`` outputs, 1 <= K <= 8: multinomial / softmax regression, a Gaussian likelihood with
    mean and log-variance predictors, any multi-output GLM.  The body assigns ``c`` and, inside ``if (want_grad) { ... }``,
    ``gs[k]`` = dc/du_k, ``Hs[k][l]`` for l <= k (the LOWER triangle of the K x K curvature; the upper one is never read) and
    ``J[k][a]`` = du_k/dx_a for every k < K, a < n (assigned, not added).  The item contributes ``g += sum_k gs_k J_k`` and
    ``H += J^T Hs J`` through an unpivoted L D L^T of ``Hs`` per item whose pivots are clamped from below at wmin (2^-60 / 2^-200), so H
    stays positive semi-definite — a Gauss-Newton door, not one for indefinite curvature; K = 1 is ``cost_ggn`` bit for bit.  A
    singular parametrisation (all K logits of a softmax) is legal but ill-conditioned: use a reference class (K - 1 free logits).
    The lane holds ``J`` as K n scalars: wide K x wide n spills (``stats()["scratch_bytes"]``).  Everything ``cost_ggn`` takes, and
    ``with_prior(mu, W)`` — the ridge term: cost += 1/2 |W (x - mu)|^2, g += W^T r, H += W^T W, still ONE residual — and
    ``shared_scalars``; ``with_loss``, ``with_bounds``, ``bind_ragged`` and the rest are refused with a sentence.  Three-class softmax
    regression with a reference class, d = 25 features (n = 50; an item = 25 features + the class 0, 1 or 2)::

        softmax = ta.JitResidual('''
            T u0 = 0, u1 = 0; for (int j = 0; j < 25; ++j) { u0 += p[j] * x[j]; u1 += p[j] * x[25 + j]; }
            const T mx = fmax(T(0), fmax(u0, u1)), e0 = exp(u0 - mx), e1 = exp(u1 - mx), er = exp(-mx), z = e0 + e1 + er;
            const T q0 = e0 / z, q1 = e1 / z, y = p[25];
            c = log(z) + mx - (y == T(0) ? u0 : y == T(1) ? u1 : T(0));
            if (want_grad) {
              gs[0] = q0 - (y == T(0) ? T(1) : T(0)); gs[1] = q1 - (y == T(1) ? T(1) : T(0));
              Hs[0][0] = q0 * (T(1) - q0); Hs[1][0] = -q0 * q1; Hs[1][1] = q1 * (T(1) - q1);
              for (int a = 0; a < 25; ++a) { J[0][a] = p[a]; J[0][25 + a] = T(0); J[1][a] = T(0); J[1][25 + a] = p[a]; }
            }''', n=50, item_scalars=26, residuals_per_item=2, kind="cost_ggn_multi", dtype=torch.float32)
        out = ta.Optimize(w, softmax.bind(samples).with_prior(mu, lam), ta.Options())   # lam [P, 50]: sqrt of the ridge weights

    Numerical differentiation (the reference's diff/num_diff.h: ``NumEval`` / ``CreateNumDiffFunc1/2``) — ``diff="forward"``,
    ``"central"`` or ``"fast_central"`` with step ``diff_h`` (0 = FloatEpsilon: 1e-4 in float32, 1e-7 in float64) differentiates a
    ``kind="residual"`` or ``kind="cost"`` body by finite differences instead of Jets: the body is only ever instantiated on the
    plain scalar type (``S`` = ``T``), so it need not be generic (tests/diff.cpp:113-132).  Euclidean parameters; 2 n + 1
    evaluations of the body per item and pass; no ``splits`` and no host controls (stop callbacks, max_duration_ms, the log line).
    ``CheckGradient(model, x)`` compares the derivatives of ANY model with those differences.

    Shared item tables — ``shared_scalars=k``: the body sees one more array, ``s[j]`` for ``0 <= j < k`` — for
    item i of EVERY problem row i of ONE table ``[items, k]`` handed over by ``bind(data, shared=table)``: one design matrix for a GLM
    per gene, one time axis for a curve fit per pixel, one map for many poses.  ``p[j]`` stays the item's own scalars
    (``item_scalars=0`` is legal beside a table), ``h[j]`` the header; the caller replicates nothing, and the rows are staged into LDS
    beside the private items (expected to come from the L2 after their first reader; not measured with counters).  ``kind="residual"`` (Jets or ``diff=``), ``"accumulate"`` and
    ``"cost_ggn"``, Euclidean parameters; such a model is a row model at every n up to 63.  ``Optimize`` (LM / GN) and ``accumulate``
    take it, with ``with_loss`` / ``with_prior`` / ``with_bounds`` as the kind allows; ``bind_ragged``, ``splits``, ``keep_order``, the
    stepping ``Optimizer``, host controls, ``Eval`` / ``CalculateJac``, ``CheckGradient``, GradientDescent / L-BFGS, manifolds, the
    other cost kinds and ``large_n`` are refused with a sentence.  Logistic regression at n = 50 on one design matrix::

        glm = ta.JitResidual('''
            T z = 0; for (int j = 0; j < 50; ++j) z += s[j] * x[j];
            const T y = p[0], e = exp(-y * z), sg = T(1) / (T(1) + e);
            c = log(T(1) + e);
            if (want_grad) { gs = -y * (T(1) - sg); hs = sg * (T(1) - sg); for (int a = 0; a < 50; ++a) J[a] = s[a]; }''',
            n=50, item_scalars=1, shared_scalars=50, kind="cost_ggn", dtype=torch.float32)
        out = ta.Optimize(w, glm.bind(labels[:, :, None], shared=X), ta.Options())   # labels [P, items], X [items, 50]

    Beyond 63 parameters — ``large_n=True`` compiles the model for the launch-per-phase pipeline of the wide problems
    (``DenseRowNatural``'s: a rows kernel over the body, the Gram on the matrix cores, the library's own LDL^T / blocked Cholesky)
    instead of a wavefront per problem: ``n`` up to 1024 in float32 and 512 in float64 (1 .. 63 is allowed too, so that one text can
    run through both routes), ``item_scalars`` up to 2048, ``kind="residual"`` (chunked Jets) or ``"accumulate"``, Euclidean
    parameters, ``diff="ad"``.  ``Optimize`` (LM / GN), ``accumulate``, ``Eval`` and ``CalculateJac`` take such a model; everything
    else is refused with a sentence: cost kinds and GradientDescent, manifolds, numerical differentiation, ``CheckGradient``,
    ``with_loss``, ``with_prior``, ``with_bounds``, ``bind_ragged``, ``splits``, the stepping ``Optimizer``, host controls, stream capture of the
    solve.  Without ``large_n`` a model of 64 parameters is refused as before.  ``stats()`` then describes the rows kernel."""

    MANIFOLDS = {"euclid": 0, "se3": 1, "user": 2}
    KINDS = {"residual": 0, "accumulate": 1, "cost": 2, "cost_grad": 3, "cost_hess": 4, "cost_ggn": 5, "cost_ggn_multi": 6}
    COST_KINDS = ("cost", "cost_grad")   # the first-order kinds (GradientDescent); "cost_hess" runs under LM / GN
    COST_HESS_MAX_N = 12
    COST_GGN_MAX_N = 63
    COST_GGN_MULTI_MAX_K = 8
    DIFFS = {"ad": 0, "forward": 1, "central": 2, "fast_central": 3}

    def __init__(self, body: str, n: int, item_scalars: int, residuals_per_item: int = 1, header_scalars: int = 0,
                 dtype: torch.dtype = torch.float64, ctx: Optional["Context"] = None, manifold: str = "euclid", kind: str = "residual",
                 plus_body: Optional[str] = None, x_scalars: int = 0, diff: str = "ad", diff_h: float = 0.0, large_n: bool = False,
                 shared_scalars: int = 0):
        """Round 5 — ``manifold="user"``: the caller's own parameter container (the reference's traits::params_trait<T>, traits.h:103-359).
        x is stored as ``x_scalars`` scalars per problem ([P, x_scalars]), ``n`` is the dimension of its tangent and ``plus_body``
        is the body of ``template <class S> void plus(const T* x, const S* d, S* xp)``: xp = x (+) d, written over the scalar type
        like the residual — the update and the roll-back run it on plain T, the differentiation on Jets seeded on d at d = 0.
        Round 6: at every n (beyond 12 parameters: up to 64 stored scalars; ``kind="accumulate"`` bodies fill J over the tangent)."""
        self.ctx = ctx or default_context()
        self.n, self.kR, self.kD, self.kH, self.dtype = int(n), int(residuals_per_item), int(item_scalars), int(header_scalars), dtype
        self.manifold, self.kind = manifold, kind
        if kind not in self.KINDS:
            raise ValueError(f"unknown kind {kind!r}; one of {sorted(self.KINDS)}")
        if diff not in self.DIFFS:
            raise ValueError(f"unknown diff {diff!r}; one of {sorted(self.DIFFS)}")
        self.diff, self.diff_h = diff, float(diff_h)
        self.large_n = bool(large_n)
        self.kS = int(shared_scalars)
        if self.kS:   # (the library refuses the same, toa_model_compile_ex: here before anything is compiled)
            if not 0 < self.kS <= 512:
                raise ValueError(f"shared_scalars must be in 0 .. 512 (0 = no shared item table), not {self.kS}")
            if kind in self.COST_KINDS or kind == "cost_hess":
                _refuse_shared(f'kind="residual", "accumulate" and "cost_ggn" take a table (the row models stage it), not kind={kind!r}')
            if manifold != "euclid":
                _refuse_shared(f"Euclidean parameters only, not manifold={manifold!r}")
            if self.large_n:
                _refuse_shared("no large_n")
        if kind == "cost_hess":   # (the library refuses the same, toa_model_compile_ex: here before anything is compiled)
            if manifold != "euclid":
                _refuse_cost_hess(f"Euclidean parameters only, not manifold={manifold!r}")
            if diff != "ad":
                _refuse_cost_hess(f'the body brings its own derivatives, nothing is differentiated: diff="ad" only, not diff={diff!r}')
            if self.large_n:
                _refuse_cost_hess("no large_n (the launch-per-phase pipeline is for residual models)")
            if self.kR != 1:
                _refuse_cost_hess(f"an item has one cost term: residuals_per_item = 1, not {self.kR}")
            if not 1 <= self.n <= self.COST_HESS_MAX_N:
                _refuse_cost_hess(f"1 <= n <= {self.COST_HESS_MAX_N} in float32 and float64 (the Hessian's triangle, n (n + 1) / 2 <= 78 accumulators, is "
                                  f"kept in registers), not n = {self.n} ({self.n * (self.n + 1) // 2} accumulators)")
        if kind == "cost_ggn":   # (the library refuses the same, toa_model_compile_ex: here before anything is compiled)
            if manifold != "euclid":
                _refuse_cost_ggn(f"Euclidean parameters only, not manifold={manifold!r}")
            if diff != "ad":
                _refuse_cost_ggn(f'the body brings its own derivatives, nothing is differentiated: diff="ad" only, not diff={diff!r}')
            if self.large_n:
                _refuse_cost_ggn("no large_n (the launch-per-phase pipeline is for residual models)")
            if self.kR != 1:
                _refuse_cost_ggn(f"an item has one cost term: residuals_per_item = 1, not {self.kR}")
            if not 1 <= self.n <= self.COST_GGN_MAX_N:
                _refuse_cost_ggn(f"1 <= n <= {self.COST_GGN_MAX_N} in float32 and float64 (one wavefront per problem), not n = {self.n}")
        if kind == "cost_ggn_multi":   # (the library refuses the same, toa_model_compile_ex: here before anything is compiled)
            if manifold != "euclid":
                _refuse_cost_ggn_multi(f"Euclidean parameters only, not manifold={manifold!r}")
            if diff != "ad":
                _refuse_cost_ggn_multi(f'the body brings its own derivatives, nothing is differentiated: diff="ad" only, not diff={diff!r}')
            if self.large_n:
                _refuse_cost_ggn_multi("no large_n (the launch-per-phase pipeline is for residual models)")
            if not 1 <= self.n <= self.COST_GGN_MAX_N:
                _refuse_cost_ggn_multi(f"1 <= n <= {self.COST_GGN_MAX_N} in float32 and float64 (one wavefront per problem), not n = {self.n}")
            if not 1 <= self.kR <= self.COST_GGN_MULTI_MAX_K:
                _refuse_cost_ggn_multi(f"residuals_per_item is K, the outputs per item: 1 <= K <= {self.COST_GGN_MULTI_MAX_K} (an item is K rows of the "
                                       f"Gram), not {self.kR}")
        if self.large_n:   # (the library refuses the same, toa_model_compile_ex: here before anything is compiled)
            if kind in self.COST_KINDS:
                _refuse_large_n('no scalar costs (kind="cost" / "cost_grad") and no GradientDescent')
            if manifold != "euclid":
                _refuse_large_n(f"Euclidean parameters only, not manifold={manifold!r}")
            if diff != "ad":
                _refuse_large_n(f'diff="ad" only (Jets, or the body\'s own Jacobian rows), not diff={diff!r}')
            nmax = 1024 if dtype == torch.float32 else 512
            if not 1 <= self.n <= nmax:
                _refuse_large_n(f"1 <= n <= 1024 in float32 and <= 512 in float64, not n = {self.n}")
            if not 0 <= self.kD <= 2048:
                _refuse_large_n(f"0 <= item_scalars <= 2048, not {self.kD}")
        self.xdim = 12 if manifold == "se3" else (int(x_scalars) if manifold == "user" else self.n)
        self._h = C.c_void_p()
        log = C.create_string_buffer(1 << 16)
        spec = ToaJitSpec()
        spec.dtype, spec.num_params, spec.residuals_per_item = _dtype_code(dtype), self.n, self.kR
        spec.scalars_per_item, spec.header_scalars = self.kD, self.kH
        spec.manifold, spec.kind = self.MANIFOLDS[manifold], self.KINDS[kind]
        spec.diff, spec.diff_h = self.DIFFS[diff], self.diff_h
        spec.large_n = 1 if self.large_n else 0
        spec.shared_scalars = self.kS
        if manifold == "user":
            if not plus_body or int(x_scalars) < 1:
                raise ValueError('manifold="user" needs plus_body (the body of x (+) d) and x_scalars')
            spec.x_scalars, spec.plus_body = int(x_scalars), plus_body.encode()
        rc = self.ctx.lib.toa_model_compile_ex(self.ctx.h, C.byref(spec), body.encode(), C.byref(self._h), log, len(log))
        self.compile_log = log.value.decode(errors="replace")
        check(rc)
        fc = C.c_int(0)
        check(self.ctx.lib.toa_jit_model_info(self._h, C.byref(fc), None))
        self.from_cache = bool(fc.value)

    def stats(self) -> dict:
        """What the run-time build of the fused kernel (``large_n=True``: of the rows kernel with J) came out as: resident workgroups
        per compute unit, LDS per workgroup, vector registers per lane, scratch bytes per lane (0 = nothing spilled)."""
        v = [C.c_int(0) for _ in range(4)]
        check(self.ctx.lib.toa_jit_model_stats(self._h, *[C.byref(t) for t in v]))
        return dict(wg_per_cu=v[0].value, lds_bytes_per_wg=v[1].value, num_regs=v[2].value, scratch_bytes=v[3].value)

    @staticmethod
    def set_cache_dir(path: Optional[str], ctx: Optional["Context"] = None) -> None:
        """Where compiled code objects are kept (default: $XDG_CACHE_HOME/tinyopt_amd or ~/.cache/tinyopt_amd); "" = no cache."""
        check((ctx or default_context()).lib.toa_jit_set_cache_dir(None if path is None else path.encode()))   # None: back to the default

    def bind(self, data: Optional[torch.Tensor], header: Optional[torch.Tensor] = None, items: int = 1,
             shared: Optional[torch.Tensor] = None) -> "JitModel":
        """data: [P, items, item_scalars] (and header: [P, header_scalars]) on the GPU -> the ``cost`` of Optimize(x, cost).
        data = None for a functor with item_scalars = 0 (e.g. a pose prior: everything is in the header).
        shared: [items, shared_scalars] on the GPU, the model's dtype — the ONE table every problem reads (row i beside item i's own
        scalars, as ``s[k]`` in the body): required by a model with ``shared_scalars``, refused by one without.  With
        ``item_scalars = 0`` the rule above holds: ``bind(None, header=..., items=..., shared=table)`` — the header carries P."""
        kS = getattr(self, "kS", 0)
        if shared is None:
            if kS:
                raise ValueError(f"bind: a model with shared_scalars = {kS} needs shared=, the batch's [items, {kS}] table")
            return JitModel(self, data, header, items)
        if not kS:
            raise ValueError("bind: shared= is the table of a model with shared_scalars > 0; this model has none")
        m = JitModel(self, data, header, items)
        if not isinstance(shared, torch.Tensor) or tuple(shared.shape) != (m.items, kS):
            raise ValueError(f"bind: shared must be an [items, shared_scalars] = [{m.items}, {kS}] tensor, not "
                             f"{list(shared.shape) if isinstance(shared, torch.Tensor) else type(shared).__name__}")
        if shared.dtype != self.dtype or shared.device != m.packed.device:
            raise ValueError(f"bind: shared must have the model's dtype {self.dtype} on the data's device {m.packed.device}, not {shared.dtype} on {shared.device}")
        m.shared = shared.contiguous()
        return m

    def bind_ragged(self, data: torch.Tensor, counts=None, offsets=None, header: Optional[torch.Tensor] = None) -> "RaggedJitModel":
        """A RAGGED batch: every problem has its own item count.  data: [total_items, item_scalars] on the GPU, the items of all
        problems one after another; exactly one of ``counts`` ([P] items per problem) / ``offsets`` ([P + 1], see ``ragged_offsets``);
        header: [P, header_scalars].  A count of 0 is legal (that problem ends with kSkipped, x untouched)."""
        if self.large_n:
            _refuse_large_n("no ragged batches (bind_ragged)")
        if self.kind == "cost_hess":
            _refuse_cost_hess("no ragged batches (bind_ragged)")
        if self.kind == "cost_ggn":
            _refuse_cost_ggn("no ragged batches (bind_ragged)")
        if self.kind == "cost_ggn_multi":
            _refuse_cost_ggn_multi("no ragged batches (bind_ragged)")
        if getattr(self, "kS", 0):
            _refuse_shared("no ragged batches (bind_ragged)")
        return RaggedJitModel(self, data, counts, offsets, header)

    def stats_prior(self, ragged: bool = False) -> dict:
        """``stats_ragged`` of the fused kernel with a Gaussian prior (``with_prior``), uniform or ragged (its plain L2 build,
        compiled by this call if it was not yet)."""
        v = [C.c_int(0) for _ in range(3)]
        check(self.ctx.lib.toa_jit_model_stats_prior(self.ctx.h, self._h, int(bool(ragged)), *[C.byref(t) for t in v]))
        return dict(wg_per_cu=v[0].value, num_regs=v[1].value, scratch_bytes=v[2].value)

    def stats_bounds(self, ragged: bool = False, with_prior: bool = False) -> dict:
        """``stats_ragged`` of the fused kernel with box bounds (``with_bounds``) in the form named by ``ragged`` / ``with_prior`` (its
        plain L2 build, compiled by this call if it was not yet)."""
        v = [C.c_int(0) for _ in range(3)]
        check(self.ctx.lib.toa_jit_model_stats_bounds(self.ctx.h, self._h, int(bool(ragged)), int(bool(with_prior)), *[C.byref(t) for t in v]))
        return dict(wg_per_cu=v[0].value, num_regs=v[1].value, scratch_bytes=v[2].value)

    def stats_lbfgs(self, ragged: bool = False) -> dict:
        """``stats_ragged`` of the L-BFGS fused kernel of a cost model (``Options.LBFGS``), uniform or ragged, compiled by this call if
        it was not yet; ``wg_per_cu`` at the default history of 8 (the ring of pairs is LDS of the launch)."""
        v = [C.c_int(0) for _ in range(3)]
        check(self.ctx.lib.toa_jit_model_stats_lbfgs(self.ctx.h, self._h, int(bool(ragged)), *[C.byref(t) for t in v]))
        return dict(wg_per_cu=v[0].value, num_regs=v[1].value, scratch_bytes=v[2].value)

    def stats_ragged(self) -> dict:
        """``stats`` of the ragged fused kernel (its plain L2 build, compiled by this call if it was not yet)."""
        v = [C.c_int(0) for _ in range(3)]
        check(self.ctx.lib.toa_jit_model_stats_ragged(self.ctx.h, self._h, *[C.byref(t) for t in v]))
        return dict(wg_per_cu=v[0].value, num_regs=v[1].value, scratch_bytes=v[2].value)

    def close(self) -> None:
        if self._h:
            self.ctx.lib.toa_model_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class JitModel(_JitBatch):
    """A JitResidual bound to its problem data ([P][header | items x item_scalars], the layout of the built-in Jet families)."""
    def __init__(self, res: JitResidual, data: Optional[torch.Tensor], header: Optional[torch.Tensor] = None, items: int = 1):
        if data is None:   # a functor whose items carry no data of their own (item_scalars = 0): `items` evaluations of the header
            assert res.kD == 0 and header is not None
            data = torch.zeros(header.shape[0], int(items), 0, dtype=res.dtype, device=header.device)
        assert data.dim() == 3 and data.shape[2] == res.kD and data.is_cuda and data.dtype == res.dtype
        self.res = res
        self.P, self.items, self.n, self.dtype = data.shape[0], data.shape[1], res.n, res.dtype
        self.xdim = res.xdim
        self.m = self.items * res.kR
        flat = data.reshape(self.P, self.items * res.kD)   # (explicit: an empty batch has no size to infer)
        if res.kH:
            assert header is not None and header.shape == (self.P, res.kH) and header.dtype == res.dtype
            flat = torch.cat([header, flat], dim=1)
        self.packed = flat.contiguous()

    def _prior_device(self):
        return self.packed.device

    def _head(self, ctx: "Context", x: torch.Tensor) -> tuple:
        if self.shared is not None:   # (the *_shared entries: the table between the data and x)
            return (ctx.h, self.res._h, self.items, x.shape[0], self.packed.data_ptr(), C.byref(self._shared_pod()), x.data_ptr())
        return (ctx.h, self.res._h, self.items, x.shape[0], self.packed.data_ptr(), x.data_ptr())

    def _shared_pod(self):
        pod = ToaShared()
        pod.table_dev, pod.rows = self.shared.data_ptr(), self.shared.shape[0]
        return pod

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        """Per problem: its own items (the shared table is read once for the whole batch, not per problem)."""
        return self.packed.shape[1] * self.packed.element_size()


def ragged_offsets(counts=None, offsets=None, total_items: Optional[int] = None) -> torch.Tensor:
    """The offsets array of a ragged batch (``JitResidual.bind_ragged``), validated on the CPU: int64 [P + 1], non-decreasing,
    [0] = 0, [P] = total_items; problem p owns items [off[p], off[p + 1]).  Exactly one of ``counts`` ([P], each >= 0) and
    ``offsets`` ([P + 1]) is given; ``total_items``, when given, must be the sum.  Raises ValueError with the reason."""
    if (counts is None) == (offsets is None):
        raise ValueError("ragged_offsets: give exactly one of counts / offsets")
    src = counts if counts is not None else offsets
    t = src.detach().to("cpu") if isinstance(src, torch.Tensor) else torch.as_tensor(list(src))
    if t.numel() and (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool):
        raise ValueError("ragged_offsets: counts / offsets must be integers")
    t = t.to(torch.int64).reshape(-1)
    if counts is not None:
        if bool((t < 0).any()):
            raise ValueError("ragged_offsets: a count is negative")
        off = torch.zeros(t.numel() + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(t, 0)
    else:
        if t.numel() < 1:
            raise ValueError("ragged_offsets: offsets has P + 1 entries (at least one)")
        if int(t[0]) != 0:
            raise ValueError("ragged_offsets: offsets[0] must be 0")
        if bool((t[1:] < t[:-1]).any()):
            raise ValueError("ragged_offsets: offsets must be non-decreasing")
        off = t.clone()
    if total_items is not None and int(off[-1]) != int(total_items):
        raise ValueError(f"ragged_offsets: the counts add up to {int(off[-1])} items, not total_items = {int(total_items)}")
    return off


class RaggedJitModel(_JitBatch):
    """A JitResidual bound to a RAGGED batch: data [total_items, item_scalars] (the items of all problems, one after another), a
    separate header [P, header_scalars] and int64 offsets [P + 1].  Taken by ``Optimize`` (LM, GN; GradientDescent for cost kinds),
    ``accumulate``, ``Eval`` and ``CalculateJac``; every problem computes bit for bit what it would alone in a uniform batch of
    its own count.  No ``splits``, no host controls (stop callbacks, max_duration_ms, the log line), no ``Optimizer`` (stepping)
    and no ``CheckGradient``: a ragged batch runs in the one-launch form only."""
    ragged, _plain = True, (True, None)

    def __init__(self, res: JitResidual, data: torch.Tensor, counts=None, offsets=None, header: Optional[torch.Tensor] = None):
        if data.dim() != 2 or data.shape[1] != res.kD or not data.is_cuda or data.dtype != res.dtype:
            raise ValueError("bind_ragged: data must be a [total_items, item_scalars] GPU tensor of the model's dtype")
        off = ragged_offsets(counts, offsets, total_items=data.shape[0])
        self.res = res
        self.P, self.n, self.xdim, self.dtype = off.numel() - 1, res.n, res.xdim, res.dtype
        self.total_items = int(data.shape[0])
        cnt = off[1:] - off[:-1]
        self.max_items = int(cnt.max()) if self.P else 0
        if self.max_items * res.kR >= 2 ** 31:
            raise ValueError("bind_ragged: a problem has 2^31 residual rows or more")
        self.offsets_host = off
        self.offsets = off.to(data.device)
        self.data = data.contiguous()
        if res.kH:
            if header is None or tuple(header.shape) != (self.P, res.kH) or header.dtype != res.dtype or header.device != data.device:
                raise ValueError("bind_ragged: header must be a [P, header_scalars] tensor of the model's dtype on data's device")
            self.header = header.contiguous()
        else:
            self.header = None

    @property
    def rows(self) -> int:
        """Residual rows of the whole batch: total_items x residuals_per_item."""
        return self.total_items * self.res.kR

    @property
    def algorithmic_bytes_per_pass(self) -> float:
        """The mean per problem."""
        if not self.P:
            return 0.0
        return (self.total_items * self.res.kD / self.P + self.res.kH) * self.data.element_size()

    def _prior_device(self):
        return self.data.device

    def _head(self, ctx: "Context", x: torch.Tensor) -> tuple:
        return (ctx.h, self.res._h, self.offsets.data_ptr(), self.header.data_ptr() if self.header is not None else None, self.max_items,
                self.total_items, x.shape[0], self.data.data_ptr(), x.data_ptr())


class SE3Prior(_Model):
    """SE3 pose prior — the reference's own manifold test (tests/sophus.cpp:26-44): residual(x) = log(prior_inv * x),
    differentiated on the device by dual numbers over the right perturbation (optimize_autodiff.h:48-77, sophus.h:24-26).
    prior_inv: [P, 12] (rotation matrix row-major + translation); x: [P, 12], updated by pose <- pose * exp(delta)."""
    model_id = MODEL_SE3_PRIOR
    xdim = 12

    def __init__(self, prior_inv: torch.Tensor):
        assert prior_inv.dim() == 2 and prior_inv.shape[1] == 12 and prior_inv.is_cuda
        self.P, self.n, self.m, self.dtype = prior_inv.shape[0], 6, 6, prior_inv.dtype
        self.packed = prior_inv.contiguous()

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return 12 * self.packed.element_size()


class MahaPrior(_Model):
    """Gaussian prior with a GENERAL covariance per problem: res = U (x - y) with U the upper Cholesky factor of the
    information matrix (the reference's MahaWhitenedInfoU, losses/mahalanobis.h:160-171; tests/cov.cpp:91-146).
    y: [P, n]; U: [P, n, n] upper triangular.  H = U^T U = cov^-1, so Output.Covariance() returns the prior covariance."""
    model_id = MODEL_MAHA_PRIOR

    def __init__(self, y: torch.Tensor, U: torch.Tensor):
        assert y.dim() == 2 and U.shape == (y.shape[0], y.shape[1], y.shape[1]) and y.is_cuda and U.dtype == y.dtype
        self.P, self.n = y.shape
        self.m, self.dtype = self.n, y.dtype
        self.packed = torch.cat([y, torch.triu(U).reshape(self.P, -1)], dim=1).contiguous()

    @staticmethod
    def from_covariance(y: torch.Tensor, cov: torch.Tensor):
        """`Lt = Cy.inverse().llt().matrixU()` (tests/cov.cpp:96) for a batch; model set-up, not the hot path."""
        info = torch.linalg.inv(cov.to(torch.float64))
        U = torch.linalg.cholesky(info).transpose(-1, -2).to(y.dtype)
        return MahaPrior(y, U.contiguous())

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return (self.n + self.n * self.n) * self.packed.element_size()


class TestFn(_Model):
    """The analytic functions of the reference's optimizer tests (tests/optimize_easy.cpp, tests/optimize_hard.cpp) as
    manual Accumulate callbacks with their exact Hessians: "rosenbrock", "plateau", "powell" (n = 4), "beale",
    "himmelblau".  x: [P, n] is a batch of starting points.  Exercises the bad-step / failed-solve / rollback
    branches of the LM loop on the device."""
    model_id = MODEL_TESTFN
    __test__ = False  # not a pytest class
    FUNCTIONS = {"rosenbrock": (0, 2, 1), "plateau": (1, 2, 1), "powell": (2, 4, 1), "beale": (3, 2, 3), "himmelblau": (4, 2, 2), "x_minus_2": (5, 1, 1)}

    def __init__(self, name: str, P: int, dtype=torch.float64, device="cuda"):
        fid, n, m = self.FUNCTIONS[name]
        self.name, self.P, self.n, self.m, self.dtype = name, int(P), n, m, dtype
        self.packed = torch.full((1,), float(fid), dtype=dtype, device=device)

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return 0


class DenseRowAD6(_LossMixin):
    """The DenseRow residual for n = 6 written the tinyopt way — residual only, Jacobian by device AD.
    A: [P, m, 6], b: [P, m] (natural layout)."""
    model_id = MODEL_DENSE_ROW_AD6

    def __init__(self, A: torch.Tensor, b: torch.Tensor):
        assert A.dim() == 3 and A.shape[2] == 6 and b.shape == A.shape[:2] and A.is_cuda
        self.P, self.m, self.n, self.dtype = A.shape[0], A.shape[1], 6, A.dtype
        self.packed = torch.cat([A, b[..., None]], dim=2).contiguous()

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return self.m * 7 * self.packed.element_size()


class DenseRowAD(_Model):
    """The DenseRow residual for a WIDE parameter block written the tinyopt way — residual only, the Jacobian by device
    AD in the matrix cores' operand layout (csrc/row_model.hpp RowModel over AdRowFunctor, "chunked Jets").  n = 12 or n = 50.
    A: [P, m, n], b: [P, m] (natural layout)."""
    model_id = MODEL_DENSE_ROW_AD

    def __init__(self, A: torch.Tensor, b: torch.Tensor):
        assert A.dim() == 3 and A.shape[2] in (12, 50) and b.shape == A.shape[:2] and A.is_cuda
        self.P, self.m, self.n, self.dtype = A.shape[0], A.shape[1], A.shape[2], A.dtype
        self.packed = torch.cat([A, b[..., None]], dim=2).contiguous()

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return self.m * (self.n + 1) * self.packed.element_size()


class BundleAdjustment(_LossMixin, _ConstantMixin):
    """C SE3 cameras x N 3-D points, pinhole reprojection residuals: the multi-pose problem behind
    config C5's single-pose block.  x: [P, 12*C + 3*N] = poses (rotation matrix row-major + translation) then points;
    data: [P, 8 + 3*C*N] = [f, cx, cy, 0... | uv (C, N, 2) | vis (C, N)].  Solved with the points eliminated (Schur
    complement on the reduced camera system, `toa_ba_run`); the reference would run Optimize on the full dense /
    SimplicialLDLT system (math.h:232-277).  Output.final_hessian is not produced.  ``.with_loss("cauchy", th)``: every
    observation's squared reprojection error through an M-estimator (losses/robust_norms.h:32-316; round 4);
    ``.with_constant(cameras=, points=)`` holds cameras and points constant (``_ConstantMixin``)."""
    route = "ba"

    def __init__(self, data: torch.Tensor, ncam: int, npts: int):
        assert data.dim() == 2 and data.shape[1] == 8 + 3 * ncam * npts and data.is_cuda
        self.P, self.ncam, self.npts, self.dtype = data.shape[0], int(ncam), int(npts), data.dtype
        self.n, self.m, self.xdim = 6 * self.ncam + 3 * self.npts, 2 * self.ncam * self.npts, 12 * self.ncam + 3 * self.npts
        self.packed = data.contiguous()

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return (3 * self.ncam * self.npts + 3 * self.npts) * self.packed.element_size()


class DenseRowNatural(_LossMixin):
    """The DenseRow family beyond one wavefront (n up to 4096): rows (a_i, b_i) in natural layout.
    64 <= n <= 128: the whole loop in one persistent kernel, a workgroup per problem, J^T J on the matrix cores
    without materialising J, blocked LDL^T by the four waves (csrc/large_fused.hip).  Beyond: J^T J through a batched rocBLAS
    GEMM, the damped solve through the workgroup LDL^T / rocSOLVER's batched Cholesky, the LM state machine of
    optimizer.h:242-539 in small kernels between them (csrc/large_n.hip).  A: [P, m, n], b: [P, m]; stored per problem as A
    then b."""
    model_id = MODEL_DENSE_ROW_NATURAL

    def __init__(self, A: torch.Tensor, b: torch.Tensor):
        assert A.dim() == 3 and b.shape == A.shape[:2] and A.is_cuda
        self.P, self.m, self.n, self.dtype = A.shape[0], A.shape[1], A.shape[2], A.dtype
        # per problem: A row-major [m][n] followed by b [m] (SURVEY §8d layout; rows stay 16-byte aligned when n % 4 == 0)
        self.packed = torch.cat([A.reshape(self.P, -1), b], dim=1).contiguous()

    @classmethod
    def from_arrays(cls, A: torch.Tensor, b: torch.Tensor) -> "DenseRowNatural":
        return cls(A, b)

    @property
    def algorithmic_bytes_per_pass(self) -> int:
        return self.m * (self.n + 1) * self.packed.element_size()


@dataclass
class Output:
    """tinyopt::Output (output.h:26-145), one row per problem; tensors live on the GPU.
    final_inlier_ratio = Output::final_cost.inlier_ratio (cost.h:84-95)."""
    stop_reason: torch.Tensor
    num_iters: torch.Tensor
    num_failures: torch.Tensor
    num_consec_failures: torch.Tensor
    final_cost: torch.Tensor
    final_num_residuals: torch.Tensor
    final_rerr_dec: torch.Tensor
    final_hessian: Optional[torch.Tensor] = None
    errs: Optional[torch.Tensor] = None
    deltas2: Optional[torch.Tensor] = None
    successes: Optional[torch.Tensor] = None
    counters: Optional[torch.Tensor] = None  # [acc passes streamed, eval passes, solves, problems, Builds served from the memo, 3 reserved]
    final_inlier_ratio: Optional[torch.Tensor] = None

    def Covariance(self, rescaled: bool = False):
        """Output::Covariance (output.h:80-94): inverse of the final undamped Hessian per problem; with
        rescaled=True multiplied by eps^2/(#eps - dims) where #residuals > dims.  Returns (C [P,n,n], ok [P]);
        ok == 0 where H is not invertible (std::nullopt in the reference)."""
        if self.final_hessian is None:
            raise ValueError("final_hessian was not saved (options.hessian.save_last)")
        C, ok = inv_cov(self.final_hessian)
        if rescaled:
            n = self.final_hessian.shape[1]
            nres = self.final_num_residuals.to(torch.float64)
            scale = torch.where(nres > n, self.final_cost * self.final_cost / (nres - n).clamp(min=1), torch.ones_like(nres))
            C = C * scale[:, None, None]
        return C, ok

    def Succeeded(self) -> torch.Tensor:  # output.h:30
        return self.stop_reason >= 0

    def Converged(self) -> torch.Tensor:  # output.h:33-35
        return (self.stop_reason >= 1) & (self.stop_reason < 5)


def _check_call(x: torch.Tensor, cost):
    if not isinstance(cost, _Model):
        raise TypeError("cost must be a device model (DenseRow, GaussianPrior, Sqrt2, ...); host callables cannot run "
                        "on the GPU path")
    if not x.is_cuda or not x.is_contiguous():
        raise ValueError("x must be a contiguous GPU tensor")
    P, xd = x.shape
    if xd != cost.xdim or P != cost.P or x.dtype != cost.dtype:
        raise ValueError("x shape/dtype does not match the model")  # reference: std::invalid_argument


def _alloc_output(P: int, n: int, options: Options, history: bool, dev, final_hessian: Optional[bool] = None) -> Output:
    """``final_hessian``: whether there is room for the final Hessian; None = what options.hessian.save_last says."""
    i32 = dict(dtype=torch.int32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    out = Output(
        stop_reason=torch.zeros(P, **i32), num_iters=torch.zeros(P, **i32), num_failures=torch.zeros(P, **i32),
        num_consec_failures=torch.zeros(P, **i32), final_cost=torch.zeros(P, **f64),
        final_num_residuals=torch.zeros(P, **i32), final_rerr_dec=torch.zeros(P, **f64),
        counters=torch.zeros(8, dtype=torch.int64, device=dev),
        final_inlier_ratio=torch.ones(P, dtype=torch.float32, device=dev))
    if options.hessian.save_last if final_hessian is None else final_hessian:
        out.final_hessian = torch.zeros(P, n, n, **f64)
    if history:
        hs = options.max_iters + 2
        out.errs = torch.zeros(P, hs, **f64)
        out.deltas2 = torch.zeros(P, hs, **f64)
        out.successes = torch.zeros(P, hs, dtype=torch.uint8, device=dev)
    return out


def _results_pod(out: Output) -> ToaResults:
    res = ToaResults()
    res.stop_reason = out.stop_reason.data_ptr()
    res.num_iters = out.num_iters.data_ptr()
    res.num_failures = out.num_failures.data_ptr()
    res.num_consec_failures = out.num_consec_failures.data_ptr()
    res.final_cost = out.final_cost.data_ptr()
    res.final_num_residuals = out.final_num_residuals.data_ptr()
    res.final_rerr_dec = out.final_rerr_dec.data_ptr()
    res.final_hessian = out.final_hessian.data_ptr() if out.final_hessian is not None else None
    res.errs = out.errs.data_ptr() if out.errs is not None else None
    res.deltas2 = out.deltas2.data_ptr() if out.deltas2 is not None else None
    res.successes = out.successes.data_ptr() if out.successes is not None else None
    res.hist_stride = out.errs.shape[1] if out.errs is not None else 0
    res.final_inlier_ratio = out.final_inlier_ratio.data_ptr() if out.final_inlier_ratio is not None else None
    return res


def _run_prologue(x: torch.Tensor, cost, options: Options, history: bool, ctx: Context, out: Optional[Output], zero_counters: bool, gd_run: bool):
    """What every one-launch run does before its library call: the options as a pod, the caller's ``out`` (its counters zeroed
    unless ``zero_counters`` is off) or a fresh one, the results pod over it, the cost's loss on the handle.  Returns (pod, out, res).
    A path that forms no final Hessian (a GD run, the Schur solve of the BA families) allocates none, whatever options.hessian.save_last says."""
    pod = options.to_pod()
    if out is None:
        out = _alloc_output(x.shape[0], cost.n, options, history, x.device,
                            options.hessian.save_last and not gd_run and cost.route in ("builtin", "jit"))
    elif zero_counters:
        out.counters.zero_()
    res = _results_pod(out)
    _apply_loss(ctx, cost)
    return pod, out, res


def _lbfgs_pod(ctx: Context, options: Options) -> ToaLbfgsOptions:
    lb = ToaLbfgsOptions()
    ctx.lib.toa_lbfgs_options_default(C.byref(lb))
    lb.history, lb.c1, lb.shrink = int(options.lbfgs.history), float(options.lbfgs.c1), float(options.lbfgs.shrink)
    return lb


def _gd_pod(ctx: Context, options: Options) -> ToaGdOptions:
    gd = ToaGdOptions()
    ctx.lib.toa_gd_options_default(C.byref(gd))
    gd.lr = float(options.gd.lr)
    return gd


def Optimize(x: torch.Tensor, cost, options: Optional[Options] = None, *, history: bool = False,
             ctx: Optional[Context] = None, out: Optional[Output] = None, splits: Optional[int] = None,
             zero_counters: bool = True, keep_order: bool = False) -> Output:
    """``tinyopt::Optimize(x, cost, options)`` (optimize.h:16-77) for a batch of independent problems.

    x: [P, n] GPU tensor, updated IN PLACE (the reference takes x by non-const reference).
    cost: a device model (``DenseRow``, ...).  Returns the per-problem Output.  One kernel launch,
    asynchronous on torch's current stream — except ``DenseRowNatural`` beyond n = 128, a host loop over passes that returns
    when the solve is done (it enqueues two passes ahead of the stop counts where every stage is a kernel of this library).  ``out.counters`` is zeroed here and added to by the
    library (every path accumulates); ``zero_counters=False`` skips that fill launch for a caller whose ``out`` is fresh or who
    wants running totals (it is ~8 us of a 50 us single-problem solve; the C-ABI takes the counters as they are).
    ``keep_order`` (ragged batches only): hand the problems out in index order instead of longest first.
    """
    options = options or Options()
    _check_call(x, cost)
    ctx = ctx or default_context(x.device.index)
    route = cost.route
    host, gd = options.has_host_controls(), options.solver_type == _GRADIENT_DESCENT
    lbfgs = options.solver_type == _LBFGS_SOLVER
    gd_run = lbfgs_run = False
    if host or gd or lbfgs or splits is not None or keep_order or cost.large_n:   # (a call with none of these has nothing to refuse)
        asked = {"host": host, "gd": gd, "splits": splits is not None, "keep_order": keep_order,
                 "callbacks": options.stop_callback is not None or options.stop_callback2 is not None,
                 "out with host controls": host and (splits is not None or out is not None),
                 "capture": cost.large_n and torch.cuda.is_current_stream_capturing()}
        if lbfgs:
            lb = options.lbfgs
            asked.update({"lbfgs": True, "grad_clipping": options.grad_clipping != 0, "lbfgs.history": not 1 <= int(lb.history) <= 16,
                          "lbfgs.c1": not 0.0 < lb.c1 < 1.0, "lbfgs.shrink": not 0.0 < lb.shrink < 1.0})
        _refuse(_OPTIMIZE_REFUSES, _who(cost, gd, lbfgs), {what for what, yes in asked.items() if yes})
        if host and route != "ba_lists":   # the stepping form (toa_lm_begin / toa_jit_lm_begin, step, stop)
            return _optimize_with_host_controls(x, cost, options, history, ctx)
        # gd::Optimizer (optimizers/gd.h) on a scalar cost model: no final Hessian (optimizer.h:313)
        gd_run = gd and route == "jit" and cost.res.kind in JitResidual.COST_KINDS
        lbfgs_run = lbfgs   # (whatever is no first-order cost model was refused above)
    if gd_run and not cost.ragged:   # (the uniform GD entry asks for its defaults before the loss is set, the ragged one after: the order each had)
        gdo = _gd_pod(ctx, options)
    pod, out, res = _run_prologue(x, cost, options, history, ctx, out, zero_counters, gd_run or lbfgs_run)
    if gd_run and cost.ragged:
        gdo = _gd_pod(ctx, options)
    if lbfgs_run:
        lbo = _lbfgs_pod(ctx, options)
    lib = ctx.lib
    if route == "builtin":   # (spelled out, not over _head: the single-problem solves pay for every tuple built here)
        if splits is None:   # the library decides (row-split for few, huge problems: P * 4 <= #CUs and m >= 512)
            check(lib.toa_lm_run(ctx.h, cost.model_id, _dtype_code(x.dtype), cost.n, cost.m, x.shape[0], cost.packed.data_ptr(), x.data_ptr(),
                                 C.byref(pod), C.byref(res), out.counters.data_ptr()))
        else:                # explicit row-split execution with `splits` chunks per problem (0 = automatic count)
            check(lib.toa_lm_run_split(ctx.h, cost.model_id, _dtype_code(x.dtype), cost.n, cost.m, x.shape[0], cost.packed.data_ptr(), x.data_ptr(),
                                       C.byref(pod), C.byref(res), out.counters.data_ptr(), int(splits)))
        return out
    if route == "jit" and not (gd_run or lbfgs_run or cost.ragged) and cost.bounds is None and cost.prior is None and cost.shared is None:
        # the plain uniform run-time model, spelled out for the same reason (and the only one with a row-split form)
        if splits is None:
            check(lib.toa_jit_lm_run(ctx.h, cost.res._h, cost.items, x.shape[0], cost.packed.data_ptr(), x.data_ptr(),
                                     C.byref(pod), C.byref(res), out.counters.data_ptr()))
        else:
            check(lib.toa_jit_lm_run_split(ctx.h, cost.res._h, cost.items, x.shape[0], cost.packed.data_ptr(), x.data_ptr(),
                                           C.byref(pod), C.byref(res), out.counters.data_ptr(), int(splits)))
        return out
    run = (C.byref(pod), C.byref(res), out.counters.data_ptr())
    if route == "jit":       # ragged, with a prior or bounds, or a GD run: the member of the family that the model's description selects
        head = cost._head(ctx, x)
        key, extras = cost._extras()
        if key[0]:           # ragged: the flags come last
            run += (1 if keep_order else 0,)
        if gd_run:           # (a loss on a scalar cost is refused by the library)
            res.final_hessian = None
            check(getattr(lib, _JIT_ENTRIES["gd_run"][key])(*head, run[0], C.byref(gdo), *run[1:]))
        elif lbfgs_run:      # (no final Hessian either)
            res.final_hessian = None
            check(getattr(lib, _JIT_ENTRIES["lbfgs_run"][key])(*head, run[0], C.byref(lbo), *run[1:]))
        else:
            check(getattr(lib, _JIT_ENTRIES["lm_run"][key])(*(head + extras + run)))
    else:   # the two BA families (no final Hessian: the library is told so)
        pod.save_last = 0
        P, xp = x.shape[0], x.data_ptr()
        if route == "ba":
            head = (ctx.h, _dtype_code(x.dtype), cost.ncam, cost.npts, P, cost.packed.data_ptr(), xp, *run)
            if cost.constant is None:
                check(lib.toa_ba_run(*head))
            else:            # cameras / points held constant (with_constant): the twin entry, the flags last
                check(lib.toa_ba_run_constant(*head, C.byref(cost._constant_pod())))
        else:
            head = (ctx.h, _dtype_code(x.dtype), cost.ncam, cost.npts, cost.nobs, P, cost.intr.data_ptr(), cost.obs_cam.data_ptr(),
                    cost.obs_pt.data_ptr(), cost.obs_uv.data_ptr(), xp, *run, float(options.max_duration_ms or 0.0))
            if cost.constant is None:
                check(lib.toa_ba_lists_run(*head))
            else:
                check(lib.toa_ba_lists_run_constant(*head, C.byref(cost._constant_pod())))
    return out


class Optimizer:
    """The reference's class / stepping form: ``lm::Optimizer<H_t> optimizer(options)`` then ``optimizer.Step(x, acc, out)``
    one loop pass at a time (optimizer.h:199,331-539), or ``optimizer(x, cost, max_iters)`` for a bounded run — for a
    batch of independent problems.  The per-problem LM state (damping, counters, last step, ...) lives on the device
    between steps; x is updated in place at every step; ``out`` fills in as problems finish."""

    def __init__(self, x: torch.Tensor, cost, options: Optional[Options] = None, *, history: bool = False,
                 ctx: Optional[Context] = None):
        self.options = options or Options()
        _check_call(x, cost)
        _refuse(_OPTIMIZER_REFUSES, _who(cost) | ({"lbfgs"} if self.options.solver_type == _LBFGS_SOLVER else set()), ("Optimizer",))
        self.x, self.cost = x, cost
        self.ctx = ctx or default_context(x.device.index)
        self.pod = self.options.to_pod()
        P, n = x.shape[0], cost.n
        self.out = _alloc_output(P, n, self.options, history, x.device)
        self._res = _results_pod(self.out)
        nbytes = self.ctx.lib.toa_lm_state_bytes(_dtype_code(x.dtype), n, P)
        self._state = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=x.device)
        self._active = torch.zeros(1, dtype=torch.int32, device=x.device)
        _apply_loss(self.ctx, cost)
        self._entries = [getattr(self.ctx.lib, name) for name in _STEP_ENTRIES[cost.route == "jit"]]
        check(self._entries[0](*self._args(), self._state.data_ptr()))

    def _args(self) -> tuple:
        """What begin, step and stop share: the handle, the batch, x, the options, the results."""
        return (*self.cost._head(self.ctx, self.x), C.byref(self.pod), C.byref(self._res))

    def Step(self, sync: bool = True) -> Optional[int]:
        """One pass of the loop body for every running problem.  Returns how many are still running (host sync), or
        None with sync=False (stream-ordered, nothing read back)."""
        self._active.zero_()
        _apply_loss(self.ctx, self.cost)
        check(self._entries[1](*self._args(), self.out.counters.data_ptr(), self._state.data_ptr(), self._active.data_ptr()))
        return int(self._active.item()) if sync else None

    def __call__(self, max_iters: Optional[int] = None) -> Output:
        """``optimizer(x, cost, max_iters)``: step until every problem has stopped (or max_iters passes were made)."""
        limit = self.options.max_iters + 2 if max_iters is None else int(max_iters)
        for _ in range(limit):
            if self.Step() == 0:
                break
        return self.out

    def step_info(self, vectors: bool = False):
        """What the reference hands its stop callbacks after an iteration (optimizer.h:529-534): per problem the cost
        ``err``, ``dx_norm2``, ``grad_norm2`` (float64 tensors [P]) and, with vectors=True, ``dx`` and ``g`` [P, n]."""
        x, cost = self.x, self.cost
        P, n = x.shape[0], cost.n
        f64 = dict(dtype=torch.float64, device=x.device)
        err, dx2, g2 = torch.zeros(P, **f64), torch.zeros(P, **f64), torch.zeros(P, **f64)
        dx = torch.zeros(P, n, dtype=x.dtype, device=x.device) if vectors else None
        g = torch.zeros(P, n, dtype=x.dtype, device=x.device) if vectors else None
        check(self.ctx.lib.toa_lm_step_info(self.ctx.h, _dtype_code(x.dtype), n, P, self._state.data_ptr(), err.data_ptr(),
                                            dx2.data_ptr(), g2.data_ptr(), dx.data_ptr() if vectors else None,
                                            g.data_ptr() if vectors else None))
        return err, dx2, g2, dx, g

    def step_log(self):
        """The rest of what the reference's log line prints (optimizer.h:463-516): per problem the damping lambda, the residual
        count of the iteration's cost and its inlier residuals."""
        x, P = self.x, self.x.shape[0]
        lam = torch.zeros(P, dtype=torch.float64, device=x.device)
        nres = torch.zeros(P, dtype=torch.int32, device=x.device)
        ninl = torch.zeros(P, dtype=torch.int32, device=x.device)
        check(self.ctx.lib.toa_lm_step_log(self.ctx.h, _dtype_code(x.dtype), self.cost.n, P, self._state.data_ptr(), lam.data_ptr(),
                                           nres.data_ptr(), ninl.data_ptr()))
        return lam, nres, ninl

    def stop(self, request: torch.Tensor) -> None:
        """End the still-running problems p with request[p] != 0 (int32, a StopReason such as kUserStopped / kTimedOut):
        their Output rows are finalised exactly as for a problem that stops by itself."""
        request = request.to(device=self.x.device, dtype=torch.int32).contiguous()
        check(self._entries[2](*self._args(), self.out.counters.data_ptr(), self._state.data_ptr(), request.data_ptr()))


def _optimize_with_host_controls(x, cost, options: Options, history: bool, ctx: Context) -> Output:
    """Optimize() when Options carries host-side stop controls: the loop of OptimizeAcc (optimizer.h:266-310) driven
    from the host over the stepping form.  After every pass: the callbacks see (err, |dx|^2, |g|^2) / (err, dx, g) of
    each problem that no numeric stop test has ended (the else-if chain of optimizer.h:519-534), and the accumulated
    wall time is checked against max_duration_ms (one clock for the batch) — kTimedOut overrides whatever reason a
    problem picked up in that same pass, as the unconditional assignment at optimizer.h:303-305 does."""
    opt = Optimizer(x, cost, options, history=history, ctx=ctx)
    out = opt.out
    P = x.shape[0]
    want_vec = options.stop_callback2 is not None
    duration_ms = 0.0
    running_before = torch.ones(P, dtype=torch.bool, device=x.device)
    lg = options.log
    if lg.enable:   # the problems whose iterations are logged, and what the line needs from one iteration to the next
        logged = [0] if lg.problems is None else (list(range(P)) if lg.problems == "all" else [int(q) for q in lg.problems])
        logged = [q for q in logged if 0 <= q < P]
        sink = lg.sink or print
        eps = 1e-4 if x.dtype == torch.float32 else float(np.float32(1e-7))    # FloatEpsilon<Scalar> (math.h:297-301)
        big = float(np.finfo(np.float32 if x.dtype == torch.float32 else np.float64).max)
        final_cost = {q: big for q in logged}
    for it in range(options.max_iters + 2):
        t0 = time.perf_counter()
        x_before = x.clone() if (lg.enable and lg.print_x) else None   # (the line shows the x the iteration STARTED from: it is formed inside Step)
        active = opt.Step()
        if lg.enable and logged:
            # optimizer.h:463-516, one line per logged problem that made this iteration (the same fields in the same order)
            err_t, dx2_t, g2_t, dxv_t, _ = opt.step_info(vectors=lg.print_dx)
            lam_t, nres_t, ninl_t = opt.step_log()
            torch.cuda.synchronize(x.device)
            took = (time.perf_counter() - t0) * 1e3
            rb = running_before.cpu().numpy()
            for q in logged:
                if not rb[q]:
                    continue
                err, dxn2, gn2 = float(err_t[q]), float(dx2_t[q]), float(g2_t[q])
                fc = final_cost[q]
                derr = err - fc
                good = derr < 0.0                                                        # :428-429
                rel = (fc - err) / fc if (fc > eps and fc < big) else 0.0                # :431-434
                line = ""
                if lg.print_emoji:
                    line += ("\u2139\ufe0f" if it == 0 else "\u2705") if (good or it == 0) else "\u274c"
                line += f"#{it} "
                if lg.print_x:
                    line += "x:[" + " ".join(f"{float(v):.6g}" for v in x_before[q].cpu()) + "] "
                line += f"{lg.e}:{err:.4e} n:{int(nres_t[q])} d{lg.e}:{0.0 if it == 0 else derr:+.2e} r{lg.e}:{rel:+.1e} "
                line += f"|\u03b4x|:{dxn2 ** 0.5:.2e} "
                if lg.print_dx:
                    line += "\u03b4x:[" + " ".join(f"{float(v):.6g}" for v in dxv_t[q].cpu()) + "] "
                if options.min_grad_norm2 > 0:                                            # has_grad_norm2 (:413-415)
                    line += f"|\u2207|:{gn2 ** 0.5:.2e} "
                if options.solver_type == Options.LevenbergMarquardt and float(lam_t[q]) > 0:
                    line += f"\u25cb:{1.0 / float(lam_t[q]):.2e} "                       # SolverLM::stateAsString (lm.h:150-154)
                if lg.print_inliers:
                    nr = max(int(nres_t[q]), 1)
                    line += f"in:{100.0 * int(ninl_t[q]) / nr:.2f}% ({int(ninl_t[q])}) "
                if lg.print_t:
                    duration_so_far = duration_ms + took
                    line += f"\u03c4:{duration_so_far:.2f} "
                sink(line)
                if good or it == 0:
                    final_cost[q] = err                                                   # :441-446
        running = out.stop_reason == int(StopReason.kNone)
        running &= running_before          # a row reports kNone until its problem stops
        req = torch.zeros(P, dtype=torch.int32)
        # The reference evaluates the callbacks inside Step on EVERY iteration (optimizer.h:529-534) and labels kMaxIters only
        # after the loop, when stop_reason is still kNone (:320-321): a problem that used up its iterations in this very pass
        # is consulted too, and a callback returning true makes it kUserStopped, not kMaxIters.
        just_max = running_before & (out.stop_reason == int(StopReason.kMaxIters))
        consult = running | just_max
        if bool(consult.any()) and (options.stop_callback is not None or options.stop_callback2 is not None):
            err, dx2, g2, dxv, gv = opt.step_info(vectors=want_vec)
            err_h, dx2_h, g2_h = err.cpu().numpy(), dx2.cpu().numpy(), g2.cpu().numpy()
            dx_h = dxv.cpu().numpy() if want_vec else None
            g_h = gv.cpu().numpy() if want_vec else None
            just_max_h = just_max.cpu().numpy()
            for p in torch.nonzero(consult).flatten().tolist():
                stop = False
                if options.stop_callback is not None:
                    stop = bool(options.stop_callback(float(err_h[p]), float(dx2_h[p]), float(g2_h[p])))
                if not stop and options.stop_callback2 is not None:   # stop_callback2(float(err), dx.cast<float>(), g.cast<float>())
                    stop = bool(options.stop_callback2(float(np.float32(err_h[p])), dx_h[p].astype("float32"), g_h[p].astype("float32")))
                if stop:
                    if just_max_h[p]:
                        out.stop_reason[p] = int(StopReason.kUserStopped)   # already finalised: only the label changes
                    else:
                        req[p] = int(StopReason.kUserStopped)
        torch.cuda.synchronize(x.device)
        duration_ms += (time.perf_counter() - t0) * 1e3
        timed_out = options.max_duration_ms > 0 and duration_ms > options.max_duration_ms
        if timed_out:
            req[running.cpu()] = int(StopReason.kTimedOut)
        if bool(req.any()):
            opt.stop(req)
        if timed_out:   # problems that stopped by themselves in this very pass: the reference overwrites their reason too
            just = running_before & ~running
            out.stop_reason[just] = int(StopReason.kTimedOut)
            break
        running_before = running & (req.to(x.device) == 0)
        if not bool(running_before.any()):
            break
    return out


def accumulate(cost, x: torch.Tensor, want_grad: bool = True, ctx: Optional[Context] = None):
    """The Accumulate callback ``acc(x, grad, H) -> Cost`` (docs/API.md:37-57) for a batch.
    Returns (g [P,n], H [P,n,n], cost [P] float64, nres [P]); g/H are None when want_grad is False."""
    ctx = ctx or default_context(x.device.index)
    P, n = x.shape[0], cost.n
    dev = x.device
    jit = cost.route == "jit"
    want_H = want_grad and not (jit and cost.res.kind in JitResidual.COST_KINDS)   # SolverGD::Build: g and the cost, no H
    g = torch.zeros(P, n, dtype=x.dtype, device=dev) if want_grad else None
    H = torch.zeros(P, n, n, dtype=x.dtype, device=dev) if want_H else None
    c = torch.zeros(P, dtype=torch.float64, device=dev)
    nres = torch.zeros(P, dtype=torch.int32, device=dev)
    _apply_loss(ctx, cost)
    # (bounds: x as given, the active set applied to g and H, with the prior if there is one; ragged: a problem without items gives zeros)
    key, extras = cost._extras() if jit else (None, ())
    entry = getattr(ctx.lib, _JIT_ENTRIES["accumulate"][key]) if jit else ctx.lib.toa_accumulate
    check(entry(*cost._head(ctx, x), *extras, int(want_grad), g.data_ptr() if want_grad else None,
                H.data_ptr() if want_H else None, c.data_ptr(), nres.data_ptr()))
    return g, H, c, nres


class GradientCheck:
    """What ``CheckGradient`` found, per problem: ``ok`` (bool [P]), ``max_dist_g`` / ``max_dist_H`` (float64 [P])."""

    def __init__(self, ok: torch.Tensor, max_dist_g: torch.Tensor, max_dist_H: torch.Tensor, eps: float):
        self.ok, self.max_dist_g, self.max_dist_H, self.eps = ok, max_dist_g, max_dist_H, eps

    def all(self) -> bool:
        return bool(self.ok.all())

    def __bool__(self) -> bool:
        return self.all()


def CheckGradient(model: "JitModel", x: torch.Tensor, eps: Optional[float] = None, method: str = "central", check_H: bool = True,
                  ctx: Optional[Context] = None) -> GradientCheck:
    """``diff::CheckGradient`` / ``diff::CheckResidualsGradient`` (diff/gradient_check.h) for a bound run-time model of any kind, at
    x [P, n]: the model's own derivatives against finite differences of its residuals (or cost terms) with step eps / 10.
    Residual kinds compare g = J^T r and, with ``check_H``, H = J^T J; cost kinds compare g; ``kind="cost_hess"`` compares g and, with
    ``check_H``, the body's H with central differences of the body's own gradient (2 n ``accumulate`` calls on shifted copies of x,
    step eps / 10), returned as ``max_dist_H``; ``kind="cost_ggn"`` does the same with its H = sum w J J^T, which agrees with those
    differences only where u is linear in x or phi' vanishes (the phi'(u) hess u term is dropped).  ``eps`` None: the reference's default
    (1e-2 in float32, 1e-5 in float64).  The first check of a model with a (method, eps) compiles its numeric twin (then cached)."""
    if not isinstance(model, _JitBatch):
        raise TypeError("CheckGradient takes a bound run-time model (JitResidual.bind)")
    _refuse(_CHECK_GRADIENT_REFUSES, _who(model), ("CheckGradient",))
    if method not in ("forward", "central", "fast_central"):
        raise ValueError(f"unknown method {method!r}; one of 'forward', 'central', 'fast_central'")
    _check_call(x, model)
    ctx = ctx or default_context(x.device.index)
    P = x.shape[0]
    dist = torch.zeros(P, 2, dtype=torch.float64, device=x.device)
    ok = torch.zeros(P, dtype=torch.int32, device=x.device)
    _apply_loss(ctx, model)
    e = 0.0 if eps is None else float(eps)
    check(ctx.lib.toa_jit_check_gradient(ctx.h, model.res._h, model.items, P, model.packed.data_ptr(), x.data_ptr(), e,
                                         JitResidual.DIFFS[method], int(bool(check_H)), dist.data_ptr(), ok.data_ptr()))
    if eps is None:
        e = 1e-2 if x.dtype == torch.float32 else 1e-5
    if check_H and (_is_cost_hess(model) or _is_cost_ggn(model) or _is_cost_ggn_multi(model)):
        # The body's H against central differences of the body's OWN gradient with the checker's step eps / 10 (gradient_check.h:96,201):
        # 2 n Accumulate calls on shifted copies of x, no device code of its own.  Column a of the numeric H is (g(x + h e_a) - g(x - h e_a)) / (2 h).
        n, step = model.n, e / 10.0
        H = accumulate(model, x, True, ctx)[1]
        H_num = torch.empty_like(H)
        for a in range(n):
            xp, xm = x.clone(), x.clone()
            xp[:, a] += step
            xm[:, a] -= step
            # (the step as the two points realise it, so that rounding x + h does not enter the quotient)
            H_num[:, :, a] = (accumulate(model, xp, True, ctx)[0] - accumulate(model, xm, True, ctx)[0]) / (xp[:, a] - xm[:, a]).unsqueeze(1)
        dist_H = (H - H_num).abs().reshape(P, -1).amax(dim=1).to(torch.float64)
        dist_H = torch.where(torch.isnan(H - H_num).reshape(P, -1).any(dim=1), torch.full_like(dist_H, float("nan")), dist_H)
        return GradientCheck((ok != 0) & (dist_H < e), dist[:, 0], dist_H, e)
    return GradientCheck(ok != 0, dist[:, 0], dist[:, 1], e)


def _eval_out(t: Optional[torch.Tensor], shape, x: torch.Tensor, what: str) -> torch.Tensor:
    if t is None:
        return torch.empty(shape, dtype=x.dtype, device=x.device)
    if tuple(t.shape) != tuple(shape) or t.dtype != x.dtype or t.device != x.device or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {tuple(shape)} tensor of x's dtype on x's device")
    return t


def Eval(model: "JitModel", x: torch.Tensor, jac: bool = True, ctx: Optional[Context] = None, *,
         res_out: Optional[torch.Tensor] = None, J_out: Optional[torch.Tensor] = None):
    """``diff::Eval(x, f)`` (diff/auto_diff.h:14-138) for a bound run-time model at x [P, xdim]: returns (res [P, m], J [P, m, n]),
    m = items x residuals_per_item in the row order of ``accumulate``; J is None with ``jac=False`` (the body then runs on plain
    scalars).  ``kind="residual"`` bodies are differentiated on Jets, ``kind="accumulate"`` bodies bring their own rows, a
    ``diff=`` model gives the reference's ``NumEval``.  On ``manifold="se3"`` / ``"user"`` J is over the tangent (n columns).
    Not for scalar costs (``accumulate`` already returns their value and gradient) and not with a loss set.  ``res_out`` /
    ``J_out``: write into the caller's tensors (views are fine as long as they are contiguous).  The first call of a model
    compiles its Eval kernels (then cached)."""
    return _eval("Eval", model, x, True, jac, ctx, res_out, J_out)


def CalculateJac(model: "JitModel", x: torch.Tensor, ctx: Optional[Context] = None, *, J_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``diff::CalculateJac(x, f)`` (diff/auto_diff.h:120-138): the Jacobian rows J [P, m, n] alone (see ``Eval``)."""
    return _eval("CalculateJac", model, x, False, True, ctx, None, J_out)[1]


def _eval(what: str, model, x: torch.Tensor, want_res: bool, jac: bool, ctx: Optional[Context], res_out, J_out):
    """``Eval``, and ``CalculateJac`` as the Eval that wants no residuals.  A ragged batch's outputs are concatenated like its items:
    res [rows], J [rows, n]."""
    if not isinstance(model, _JitBatch):
        raise TypeError(f"{what} takes a bound run-time model (JitResidual.bind)")
    _refuse(_ROWS_REFUSES[what], _who(model), (what,))
    _check_call(x, model)
    ctx = ctx or default_context(x.device.index)
    rows = (model.rows,) if model.ragged else (x.shape[0], model.m)
    res = _eval_out(res_out, rows, x, "res_out") if want_res else None
    J = _eval_out(J_out, (*rows, model.n), x, "J_out") if jac else None
    _apply_loss(ctx, model)
    check(getattr(ctx.lib, _JIT_ENTRIES["eval"][model._plain])(*model._head(ctx, x), res.data_ptr() if want_res else None,
                                                                    J.data_ptr() if jac else None))
    return res, J


def solve_damped(H: torch.Tensor, g: torch.Tensor, scale: float = 1.0, ctx: Optional[Context] = None):
    """SolverLM damping (lm.h:108-117, H_ii *= scale) + SolverGN::Solve (gn.h:150-171) for a batch.
    Returns (dx [P,n], ok [P] int32)."""
    ctx = ctx or default_context(H.device.index)
    P, n = g.shape
    H, g = H.contiguous(), g.contiguous()
    dx = torch.zeros_like(g)
    ok = torch.zeros(P, dtype=torch.int32, device=g.device)
    check(ctx.lib.toa_solve_damped(ctx.h, _dtype_code(g.dtype), n, P, H.data_ptr(), g.data_ptr(), float(scale),
                                   dx.data_ptr(), ok.data_ptr()))
    return dx, ok


LOSS_KINDS = {"l2": 0, "truncated": 1, "huber": 2, "tukey": 3, "arctan": 4, "cauchy": 5, "geman_mcclure": 6,
              "blake_zisserman": 7}


def robust_norm(kind: str, n2: torch.Tensor, th2: float, ctx: Optional[Context] = None):
    """The reference's M-estimators in their ``Name(n2, th2, true)`` form (losses/robust_norms.h:32-316,
    docs/API.md:402-406): returns (loss, scale) tensors shaped like ``n2`` (squared norms, GPU, float32/64)."""
    ctx = ctx or default_context(n2.device.index)
    n2 = n2.contiguous()
    loss = torch.empty_like(n2)
    scale = torch.empty_like(n2)
    check(ctx.lib.toa_robust_norm(ctx.h, LOSS_KINDS[kind], _dtype_code(n2.dtype), n2.numel(), n2.data_ptr(), float(th2),
                                  loss.data_ptr(), scale.data_ptr()))
    return loss, scale


def inv_cov(H: torch.Tensor, ctx: Optional[Context] = None):
    """tinyopt::InvCov (math.h:41-91) for a batch: C = H^-1 via LDL^T with the reference's acceptance rule.
    Returns (C [P,n,n], ok [P] int32)."""
    ctx = ctx or default_context(H.device.index)
    H = H.contiguous()
    P, n, _ = H.shape
    Cm = torch.zeros_like(H)
    ok = torch.zeros(P, dtype=torch.int32, device=H.device)
    check(ctx.lib.toa_inv_cov(ctx.h, _dtype_code(H.dtype), n, P, H.data_ptr(), Cm.data_ptr(), ok.data_ptr()))
    return Cm, ok
