// tinyopt_amd/tinyopt.hpp — header-only C++ host adaptor over the C-ABI (include/tinyopt_amd.h).
//
// Mirrors the reference's user surface for the LM hot path so that a tinyopt call site changes by a
// namespace and a cost-functor type only:
//
//   reference (include/tinyopt/optimize.h:16-17)          here
//   ---------------------------------------------          ----------------------------------------
//   tinyopt::Options options;                               tinyopt_amd::Options options;
//   auto out = tinyopt::Optimize(x, cost, options);         auto out = tinyopt_amd::Optimize(x, cost, options);
//     x    : one parameter block, updated in place            x    : P parameter blocks ([P][n] contiguous), in place
//     cost : any C++ callable (residuals or Accumulate)        cost : a DEVICE model (DenseRow, GaussianPrior, Sqrt2, CircleFit, SE3Reproj) — host
//                                                                       lambdas cannot run on the GPU
//     out  : tinyopt::Output                                   out  : BatchOutput (one Output row per problem)
//
// Option names / nesting / defaults follow include/tinyopt/optimizers/options.h:18-156; StopReason
// values follow include/tinyopt/stop_reasons.h:14-43; Output fields follow include/tinyopt/output.h.
// No Eigen, no HIP headers: link with -ltinyopt_amd only.  Errors of use throw std::invalid_argument
// (as the reference does, optimize.h:47,55,75); numeric failures are StopReason values, never exceptions.
#pragma once

#include <array>
#include <chrono>
#include <cstdint>
#include <functional>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#include "../tinyopt_amd.h"

namespace tinyopt_amd {

enum StopReason : int {  // include/tinyopt/stop_reasons.h:14-43
  kOutOfMemory = -4, kSolverFailed = -3, kSystemHasNaNOrInf = -2, kSkipped = -1, kNone = 0, kMinError, kMinRelError,
  kMinDeltaNorm, kMinGradNorm, kMaxIters, kMaxNoDecr, kMaxConsecNoDecr, kTimedOut, kUserStopped
};

struct Options {  // include/tinyopt/optimizers/options.h:18-156 (numeric knobs)
  // GradientDescent, LBFGS: scalar cost models (TOA_JIT_COST / TOA_JIT_COST_GRAD); LBFGS: limited-memory BFGS, Armijo search (`lbfgs`)
  enum Solver { LevenbergMarquardt = 0, GaussNewton = 1, GradientDescent = 2, LBFGS = 3 };
  Solver solver_type = LevenbergMarquardt;
  bool check_final_cost = false;
  bool use_step_quality_approx = false;
  float grad_clipping = 0;
  struct Hessian {
    bool use_ldlt = true;
    bool H_is_full = true;
    float check_min_H_diag = 0;
    bool save_last = true;
  } hessian;
  struct CostScaling {
    bool use_squared_norm = true;
    bool downscale_by_2 = false;
    bool normalize = false;
  } cost;
  uint16_t max_iters = 50;
  float min_error = 1e-12f;
  float min_rerr_dec = 1e-10f;
  float min_step_norm2 = 1e-14f;
  float min_grad_norm2 = 1e-18f;
  uint8_t max_total_failures = 0;
  uint8_t max_consec_failures = 5;
  // Host-side stop controls (options.h:96-106).  When any is set, Optimize() drives the loop through the stepping form
  // and evaluates them between iterations (optimizer.h:302-305, 529-534); per problem of the batch.
  double max_duration_ms = 0;                                          // 0 = no limit -> kTimedOut
  std::function<bool(double, double, double)> stop_callback;           // (err, |dx|^2, |g|^2) -> kUserStopped
  std::function<bool(float, const std::vector<float>&, const std::vector<float>&)> stop_callback2;   // (err, dx, g)
  // The per-iteration log line of Optimizer_::Step (options.h:113-125, optimizer.h:463-516), through the same stepping form.  Off by
  // default here (the reference logs by default; a batched solve would print one line per problem and iteration): the problems
  // named in `problems` (empty = problem 0) are logged to `sink` (empty = std::cout, like TINYOPT_LOG: log.h:23).
  // print_max_stdev / print_J_jet / print_failure are not mirrored.
  struct Log {
    bool enable = false;
    std::string e = "\xCE\xB5\xC2\xB2";   // "ε²"
    bool print_emoji = true;
    bool print_x = false;
    bool print_dx = false;
    bool print_inliers = false;
    bool print_t = true;
    std::vector<int64_t> problems;
    std::function<void(const std::string&)> sink;
  } log;
  bool has_host_controls() const { return max_duration_ms > 0 || stop_callback || stop_callback2 || log.enable; }
  struct LM {
    float damping_init = 1e-4f;
    std::array<float, 2> damping_range{{1e-9f, 1e9f}};
    float good_factor = 1.0f / 3.0f;
    float bad_factor = 2.0f;
  } lm;
  struct GD {   // options.h:147-154
    float lr = 1e-3f;
  } gd;
  toa_gd_options gd_pod() const {
    toa_gd_options g;
    toa_gd_options_default(&g);
    g.lr = gd.lr;
    return g;
  }

  struct Lbfgs {   // toa_lbfgs_options: the textbook values (Nocedal & Wright, chapters 3 and 7)
    int history = 8;       // pairs (s, y) kept, 1 .. 16
    float c1 = 1e-4f;      // the Armijo constant, in (0, 1)
    float shrink = 0.5f;   // alpha *= shrink after a rejected trial, in (0, 1)
  } lbfgs;
  toa_lbfgs_options lbfgs_pod() const {
    toa_lbfgs_options l;
    toa_lbfgs_options_default(&l);
    l.history = lbfgs.history;
    l.c1 = lbfgs.c1;
    l.shrink = lbfgs.shrink;
    return l;
  }

  toa_options to_pod() const {
    toa_options p;
    toa_options_default(&p);
    p.solver_type = solver_type;
    p.max_iters = max_iters;
    p.min_error = min_error;
    p.min_rerr_dec = min_rerr_dec;
    p.min_step_norm2 = min_step_norm2;
    p.min_grad_norm2 = min_grad_norm2;
    p.max_total_failures = max_total_failures;
    p.max_consec_failures = max_consec_failures;
    p.damping_init = lm.damping_init;
    p.damping_min = lm.damping_range[0];
    p.damping_max = lm.damping_range[1];
    p.good_factor = lm.good_factor;
    p.bad_factor = lm.bad_factor;
    p.grad_clipping = grad_clipping;
    p.check_min_H_diag = hessian.check_min_H_diag;
    p.check_final_cost = check_final_cost;
    p.use_step_quality_approx = use_step_quality_approx;
    p.use_ldlt = hessian.use_ldlt;
    p.H_is_full = hessian.H_is_full;
    p.save_last = hessian.save_last;
    p.use_squared_norm = cost.use_squared_norm;
    p.downscale_by_2 = cost.downscale_by_2;
    p.normalize = cost.normalize;
    return p;
  }
};

// benchmarks/options.h:10-27
inline Options CreateBenchmarkOptions() {
  Options o;
  o.max_iters = 10;
  o.min_error = 0;
  o.min_rerr_dec = 1e-12f;
  o.min_step_norm2 = 1e-16f;
  o.max_consec_failures = 3;
  o.hessian.save_last = false;
  return o;
}

inline void check(int rc) {
  if (rc == TOA_OK) return;
  const std::string msg = std::string("tinyopt_amd: ") + toa_last_error();
  if (rc == TOA_E_ARG || rc == TOA_E_UNSUPPORTED) throw std::invalid_argument(msg);
  if (rc == TOA_E_NOMEM) throw std::bad_alloc();
  throw std::runtime_error(msg);
}

// RAII over toa_handle: one per host thread per GPU (the reference's Optimizer_ is equally stateful).
class Context {
 public:
  explicit Context(int device = 0, void* stream = nullptr) {
    // the header and the library must agree on the layout of what crosses the boundary (counters_dev is [TOA_NUM_COUNTERS = 8]
    // since ABI 4; a header compiled against an older library — or the reverse — must not run)
    if (toa_abi_version() != TOA_ABI_VERSION)
      throw std::runtime_error("tinyopt_amd: libtinyopt_amd.so has ABI version " + std::to_string(toa_abi_version()) + ", this header expects " +
                               std::to_string(TOA_ABI_VERSION));
    check(toa_create(&h_, device, stream));
  }
  ~Context() { toa_destroy(h_); }
  // A/B arms of the library as typed per-handle state (toa_tuning; nullptr = the library's own choices)
  void set_tuning(const toa_tuning* t) const { check(toa_set_tuning(h_, t)); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  toa_handle get() const { return h_; }

 private:
  toa_handle h_ = nullptr;
};

template <typename T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(const Context& c, size_t count) : c_(&c), n_(count) {
    void* p = nullptr;
    check(toa_malloc(c.get(), &p, count * sizeof(T)));
    p_ = static_cast<T*>(p);
  }
  ~DeviceBuffer() { if (p_) toa_free(c_->get(), p_); }
  DeviceBuffer(DeviceBuffer&& o) noexcept : c_(o.c_), p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) { if (p_) toa_free(c_->get(), p_); c_ = o.c_; p_ = o.p_; n_ = o.n_; o.p_ = nullptr; }
    return *this;
  }
  T* data() const { return p_; }
  size_t size() const { return n_; }
  void upload(const T* host) { check(toa_memcpy_h2d(c_->get(), p_, host, n_ * sizeof(T))); }
  void download(T* host) const { check(toa_memcpy_d2h(c_->get(), host, p_, n_ * sizeof(T))); }
  void zero() { check(toa_memset(c_->get(), p_, 0, n_ * sizeof(T))); }

 private:
  const Context* c_ = nullptr;
  T* p_ = nullptr;
  size_t n_ = 0;
};

template <typename Scalar>
constexpr int dtype_of() {
  static_assert(std::is_same<Scalar, float>::value || std::is_same<Scalar, double>::value,
                "Scalar must be float or double (the reference's solver Scalar)");
  return std::is_same<Scalar, float>::value ? TOA_F32 : TOA_F64;
}

// The M-estimator part of a cost functor (losses/robust_norms.h:32-316; docs/API.md:396-411 wraps a residual's squared norm
// in `losses::Huber(n2, th2, true)`): `cost.set_loss(TOA_LOSS_HUBER, th)` makes every launch with this model pass each
// residual item through rho — cost += l, the item's J^T J / J^T r scaled by s, inliers in final_inlier_ratio.  Honoured by
// DenseRow, CircleFit (the families toa_set_loss lists); SE3Reproj carries its loss in its data header.
struct LossTag {
  int loss_kind = TOA_LOSS_L2;
  double loss_th2 = 0;
  void set_loss(int kind, double th) { loss_kind = kind; loss_th2 = th * th; }
  bool se3_header_l2 = false;   // SE3Reproj: no problem's data header names a loss -> the kernels without the M-estimator branch (toa_tuning)
};
template <typename Cost>
inline void apply_loss(const Cost& cost) {
  check(toa_set_loss(cost.ctx().get(), cost.loss_kind, cost.loss_th2));
  toa_tuning t;
  check(toa_get_tuning(cost.ctx().get(), &t));
  if ((t.se3_reproj_header_l2 != 0) != cost.se3_header_l2) {   // (the field follows the model: a second host call only when it changes)
    t.se3_reproj_header_l2 = cost.se3_header_l2 ? 1 : 0;
    check(toa_set_tuning(cost.ctx().get(), &t));
  }
}

// Device cost model: r_i(x) = a_i.x + 0.1 sin(a_i.x) - b_i for P problems.  Takes the place of the
// residual functor in Optimize(x, cost) (e.g. benchmarks/dense.cpp:56,71-74).
template <typename Scalar>
class DenseRow : public LossTag {
 public:
  // A: [P][m][n] row-major, b: [P][m] — host arrays; uploaded and packed into the HBM layout once.
  DenseRow(const Context& ctx, int64_t P, int n, int m, const Scalar* A, const Scalar* b) : ctx_(&ctx), P_(P), n_(n), m_(m) {
    size_t bytes = 0;
    check(toa_dense_row_layout(dtype_of<Scalar>(), n, m, nullptr, nullptr, nullptr, nullptr, &bytes));
    packed_ = DeviceBuffer<Scalar>(ctx, size_t(P) * bytes / sizeof(Scalar));
    DeviceBuffer<Scalar> dA(ctx, size_t(P) * m * n), db(ctx, size_t(P) * m);
    dA.upload(A);
    db.upload(b);
    check(toa_dense_row_pack(ctx.get(), dtype_of<Scalar>(), n, m, P, dA.data(), db.data(), packed_.data()));
    check(toa_synchronize(ctx.get()));
  }
  static constexpr int model_id = TOA_MODEL_DENSE_ROW;
  int64_t P() const { return P_; }
  int n() const { return n_; }
  int m() const { return m_; }
  int xdim() const { return n_; }
  const Scalar* data() const { return packed_.data(); }
  const Context& ctx() const { return *ctx_; }

 private:
  const Context* ctx_;
  int64_t P_;
  int n_, m_;
  DeviceBuffer<Scalar> packed_;
};

// Generic holder for the models whose device data is a plain host array uploaded as is.
template <typename Scalar, int ModelId>
class PlainModel : public LossTag {
 public:
  PlainModel(const Context& ctx, int64_t P, int n, int m, int xdim, const Scalar* host, size_t count)
      : ctx_(&ctx), P_(P), n_(n), m_(m), xdim_(xdim), data_(ctx, count ? count : 1) {
    if (count) data_.upload(host);
  }
  static constexpr int model_id = ModelId;
  int64_t P() const { return P_; }
  int n() const { return n_; }
  int m() const { return m_; }
  int xdim() const { return xdim_; }
  const Scalar* data() const { return data_.data(); }
  const Context& ctx() const { return *ctx_; }

 private:
  const Context* ctx_;
  int64_t P_;
  int n_, m_, xdim_;
  DeviceBuffer<Scalar> data_;
};

// r = (x - y) / sigma, m = n: the reference's published dense benchmark (benchmarks/dense.cpp:53-66).
// ys: [P][2][n] = y then sigma per problem.
template <typename Scalar>
struct GaussianPrior : PlainModel<Scalar, TOA_MODEL_GAUSSIAN_PRIOR> {
  GaussianPrior(const Context& ctx, int64_t P, int n, const Scalar* ys)
      : PlainModel<Scalar, TOA_MODEL_GAUSSIAN_PRIOR>(ctx, P, n, n, n, ys, size_t(P) * 2 * n) {}
};
// r = x*x - 2 (tests/sqrt2.cpp:30-70)
template <typename Scalar>
struct Sqrt2 : PlainModel<Scalar, TOA_MODEL_SQRT2> {
  Sqrt2(const Context& ctx, int64_t P) : PlainModel<Scalar, TOA_MODEL_SQRT2>(ctx, P, 1, 1, 1, nullptr, 0) {}
};
// The analytic functions of the reference's optimizer tests as manual Accumulate callbacks (tests/optimize_easy.cpp,
// optimize_hard.cpp, basic.cpp:41-87): fn = 0 Rosenbrock, 1 plateau, 2 Powell (n = 4), 3 Beale, 4 Himmelblau, 5 `x - 2` (n = 1).
template <typename Scalar>
struct TestFn : PlainModel<Scalar, TOA_MODEL_TESTFN> {
  static int dims(int fn) { return fn == 5 ? 1 : (fn == 2 ? 4 : 2); }
  static int residuals(int fn) { return fn == 3 ? 3 : (fn == 4 ? 2 : 1); }
  TestFn(const Context& ctx, int64_t P, int fn) : PlainModel<Scalar, TOA_MODEL_TESTFN>(ctx, P, dims(fn), residuals(fn), dims(fn), id(fn), 1) {}

 private:
  const Scalar* id(int fn) { fn_ = Scalar(fn); return &fn_; }
  Scalar fn_ = 0;
};
// tests/circle.cpp:32-68, differentiated on the device by dual numbers.  obs: [P][npts][2]; x = (cx, cy, radius).
template <typename Scalar>
struct CircleFit : PlainModel<Scalar, TOA_MODEL_CIRCLE_FIT> {
  CircleFit(const Context& ctx, int64_t P, int npts, const Scalar* obs)
      : PlainModel<Scalar, TOA_MODEL_CIRCLE_FIT>(ctx, P, 3, npts, 3, obs, size_t(P) * npts * 2) {}
};
// The DenseRow residual r_i = a_i.x + 0.1 sin(a_i.x) - b_i for parameter blocks beyond one wavefront (1 <= n <= 1024;
// `Dims == Dynamic` in the reference, optimize.h:27-33): batched library GEMM + rocSOLVER Cholesky under the same LM state
// machine.  data: per problem A row-major [m][n] followed by b [m].
template <typename Scalar>
struct DenseRowNatural : PlainModel<Scalar, TOA_MODEL_DENSE_ROW_NATURAL> {
  DenseRowNatural(const Context& ctx, int64_t P, int n, int m, const Scalar* A_then_b)
      : PlainModel<Scalar, TOA_MODEL_DENSE_ROW_NATURAL>(ctx, P, n, m, n, A_then_b, size_t(P) * m * (size_t(n) + 1)) {}
};
// SE3 pinhole reprojection (3rdparty/traits/sophus.h:13-27 update); x: [P][12] = R (row-major) | t; n = 6.
// data: [P][8 + 5*npts] = [f cx cy 0 0 0 0 0 | x y z u v ...].
// Optional M-estimator on each point's squared reprojection error: data[3] = TOA_LOSS_*, data[4] = th^2
// (losses/robust_norms.h:32-316); set them in the host array before constructing the model.
template <typename Scalar>
struct SE3Reproj : PlainModel<Scalar, TOA_MODEL_SE3_REPROJ> {
  SE3Reproj(const Context& ctx, int64_t P, int npts, const Scalar* data)
      : PlainModel<Scalar, TOA_MODEL_SE3_REPROJ>(ctx, P, 6, 2 * npts, 12, data, size_t(P) * (8 + 5 * size_t(npts))) {
    bool any = false;   // (a header that names a loss keeps the kernels with the M-estimator branch)
    for (int64_t p = 0; p < P && !any; ++p) any = data[size_t(p) * (8 + 5 * size_t(npts)) + 3] != Scalar(0);
    this->se3_header_l2 = !any;
  }
};

// A residual supplied as C++ source text at RUN time (toa_model_compile: hiprtc + hipModuleLoad, no rebuild of the library) —
// the device-side form of `tinyopt::Optimize(x, [](const auto& x) { return r(x); })` (optimize.h:16-33, optimizer.h:145-160).
// body: generic in its scalar type S; x[j] parameter j, p[k] the item's scalars, h[k] the header scalars, r[q] the residuals:
//   JitResidual<double> fit(ctx, "const S dx = p[0] - x[0]; const S dy = p[1] - x[1]; r[0] = dx*dx + dy*dy - x[2]*x[2];", 3, 2);
//   auto out = Optimize(x, fit.bind(P, npts, obs));                                            // tests/circle.cpp:32-68
// diff/num_diff.h:20-52: how a run-time body is differentiated numerically (JitResidual's `diff`, diff::CheckGradient's `method`)
namespace diff {
enum Method { kForward = 0, kCentral, kFastCentral };
inline int to_pod(Method m) { return m == kForward ? TOA_DIFF_NUM_FORWARD : (m == kCentral ? TOA_DIFF_NUM_CENTRAL : TOA_DIFF_NUM_FAST_CENTRAL); }
}  // namespace diff
template <typename Scalar>
class JitModel;
template <typename Scalar>
class RaggedJitModel;
// What a body's text is (JitResidual's `kind`): the library's TOA_JIT_* by name
enum JitKind {
  kJitResidual = TOA_JIT_RESIDUAL, kJitAccumulate = TOA_JIT_ACCUMULATE, kJitCost = TOA_JIT_COST, kJitCostGrad = TOA_JIT_COST_GRAD,
  kJitCostHess = TOA_JIT_COST_HESS, kJitCostGgn = TOA_JIT_COST_GGN, kJitCostGgnMulti = TOA_JIT_COST_GGN_MULTI
};
namespace detail {
// What a second-order scalar cost (TOA_JIT_COST_HESS) does not take, in one sentence each
inline void refuse_cost_hess(const char* what) {
  throw std::invalid_argument(std::string("tinyopt_amd: a second-order scalar cost (TOA_JIT_COST_HESS) runs in the uniform one-launch form through Optimize "
                                          "(LM / GN), Accumulate and diff::CheckGradient only: ") + what);
}
// What a rank-one second-order scalar cost (TOA_JIT_COST_GGN) does not take, in one sentence each
inline void refuse_cost_ggn(const char* what) {
  throw std::invalid_argument(std::string("tinyopt_amd: a rank-one second-order scalar cost (TOA_JIT_COST_GGN) runs in the uniform one-launch form through "
                                          "Optimize (LM / GN), Accumulate and diff::CheckGradient only: ") + what);
}
// What a multi-output second-order scalar cost (TOA_JIT_COST_GGN_MULTI) does not take, in one sentence each
inline void refuse_cost_ggn_multi(const char* what) {
  throw std::invalid_argument(std::string("tinyopt_amd: a multi-output second-order scalar cost (TOA_JIT_COST_GGN_MULTI) runs in the uniform one-launch form "
                                          "through Optimize (LM / GN), Accumulate and diff::CheckGradient only, with with_prior and a shared table: ") + what);
}
// What a model with a shared item table (JitResidual's shared_scalars > 0) does not take, in one sentence each
inline void refuse_shared(const char* what) {
  throw std::invalid_argument(std::string("tinyopt_amd: a model with a shared item table (shared_scalars > 0) runs in the uniform one-launch form through "
                                          "Optimize (LM / GN) and Accumulate only: ") + what);
}
}  // namespace detail
template <typename Scalar>
class JitResidual {
 public:
  // manifold: TOA_MANIFOLD_EUCLID, or TOA_MANIFOLD_SE3 — x is ONE pose stored as 12 scalars (R row-major, t), n = 6, the body reads
  //   it through x[0..11] and may call se3_log<S, T>(R, t, xi)  (tests/sophus.cpp:26-44 `Optimize(pose, lambda)`);
  // kind: TOA_JIT_RESIDUAL (differentiated on the device), or TOA_JIT_ACCUMULATE — a manual Accumulate callback: the body fills
  //   r[q] and, inside `if (want_grad)`, its own Jacobian rows J[q][a]  (docs/API.md:37-57);
  // n up to 63, up to 8 residuals per item (beyond 12 parameters a row is a lane on the matrix-core Gram: both kinds, M-estimators, user manifolds —
  //   round 6).  Compiled code objects are cached on disk (toa_jit_set_cache_dir).
  // manifold = TOA_MANIFOLD_USER (round 5): the caller's own parameter container — tinyopt's traits::params_trait<T> (traits.h:103-359) as text:
  //   x_scalars = the container as stored, n = the dimension of its tangent, plus_body = the body of
  //   `template <class S> void plus(const T* x, const S* d, S* xp)`, xp = x (+) d (PlusEq on plain T; differentiated through Jets seeded on d).
  // diff: TOA_DIFF_DEFAULT (Jets, or the body's own derivatives), or TOA_DIFF_NUM_* (diff::to_pod(diff::kCentral) ...) — a TOA_JIT_RESIDUAL /
  //   TOA_JIT_COST body differentiated by finite differences with step diff_h (0 = FloatEpsilon<Scalar>), CreateNumDiffFunc1 / 2 of
  //   diff/num_diff.h: the body runs on plain Scalar only.  Euclidean; no stop callbacks / max_duration_ms / log line.
  // kind = TOA_JIT_COST_HESS (kJitCostHess): a second-order scalar cost, the reference's `f(x, grad, H) -> cost` (optimize.h:26-57) — the body
  //   assigns `c` and, inside `if (want_grad)`, ADDS the item's gradient to G[a] and its Hessian to H(a, b) for a <= b (a > b is discarded);
  //   run by LM / GN (GaussNewton, or lm.damping_init = 0: Newton's method).  Euclidean, one cost term per item, 1 <= n <= 12 in float and
  //   double; loops over a, b need compile-time bounds (H is a register triangle; stats().scratch_bytes shows a spill).  GradientDescent (the
  //   reference throws for this signature too), with_loss, with_prior, with_bounds, bind_ragged, host controls, the stepping Optimizer and
  //   diff::Eval / CalculateJac are refused (std::invalid_argument).
  // kind = TOA_JIT_COST_GGN (kJitCostGgn): a rank-one second-order scalar cost c_i = phi(u_i(x)) with a scalar inner function (logistic and Poisson
  //   regression, any GLM) on the matrix-core Gram of the row models — the body assigns `c` and, inside `if (want_grad)`, `gs` = dc/du, `hs` = the
  //   curvature weight and J[a] = (grad u)[a] for every a < n (assigned, not added); the item adds g += gs J and H += w J J^T, w = hs clamped from
  //   below at wmin (2^-60 in float, 2^-200 in double; a NaN stays): the generalised Gauss-Newton Hessian, positive semi-definite — not a door
  //   for indefinite Hessians (kJitCostHess remains that).  Run by LM / GN (GaussNewton, or lm.damping_init = 0: Newton's method).  Euclidean,
  //   one cost term per item, 1 <= n <= 63 in float and double; loops over a need compile-time bounds (stats().scratch_bytes shows a spill).
  //   GradientDescent, LBFGS, with_loss, with_prior, with_bounds, bind_ragged, host controls, the stepping Optimizer and diff::Eval /
  //   CalculateJac are refused (std::invalid_argument).
  // kind = TOA_JIT_COST_GGN_MULTI (kJitCostGgnMulti): c_i = phi(u_i(x)) with a VECTOR inner function of K = residuals_per_item
  //   outputs, 1 <= K <= 8 (softmax regression, mean + log-variance likelihoods) — the body assigns `c` and, inside `if (want_grad)`, gs[k] = dc/du_k,
  //   Hs[k][l] for l <= k (the lower triangle of the K x K curvature) and J[k][a] = du_k/dx_a for every k < K, a < n; the item adds
  //   g += sum_k gs_k J_k and H += J^T Hs J through a per-item L D L^T with pivots clamped at wmin: positive semi-definite; K = 1 is kJitCostGgn.
  //   1 <= n <= 63; what kJitCostGgn takes, and with_prior (the ridge term: cost += 1/2 |W (x - mu)|^2, still one residual) and bind_shared;
  //   GradientDescent, LBFGS, with_loss, with_bounds, bind_ragged, host controls, the stepping Optimizer and diff::Eval / CalculateJac are
  //   refused (std::invalid_argument).
  // large_n = true: the model is compiled for the launch-per-phase pipeline of the wide problems instead of a wavefront per problem —
  //   n up to 1024 (float) / 512 (double), item_scalars up to 2048; TOA_JIT_RESIDUAL / TOA_JIT_ACCUMULATE, Euclidean, TOA_DIFF_DEFAULT.
  //   Optimize (LM / GN), Accumulate and diff::Eval / CalculateJac take it; with_loss, with_prior, with_bounds, bind_ragged, splits, the stepping
  //   Optimizer, host controls, GradientDescent and diff::CheckGradient are refused (std::invalid_argument).  Without it n = 64 is refused.
  // shared_scalars = kS > 0: the body sees one more array, s[k] for 0 <= k < kS — for item i of EVERY problem row i of ONE
  //   table [items][kS] handed over by bind_shared (one design matrix for a GLM per gene, one time axis for a curve fit per pixel); p[k] stays the
  //   item's own scalars (item_scalars = 0 is legal beside it).  TOA_JIT_RESIDUAL (Jets or TOA_DIFF_NUM_*), TOA_JIT_ACCUMULATE and
  //   TOA_JIT_COST_GGN, Euclidean, not large_n.  Optimize (LM / GN) and Accumulate take it, with_loss / with_prior / with_bounds as the kind
  //   allows; bind, bind_ragged, GradientDescent, LBFGS, host controls, the stepping Optimizer, diff::Eval / CalculateJac and
  //   diff::CheckGradient are refused (std::invalid_argument).
  JitResidual(const Context& ctx, const std::string& body, int n, int item_scalars, int residuals_per_item = 1, int header_scalars = 0,
              int manifold = TOA_MANIFOLD_EUCLID, int kind = TOA_JIT_RESIDUAL, const std::string& plus_body = std::string(), int x_scalars = 0,
              int diff = TOA_DIFF_DEFAULT, float diff_h = 0.f, bool large_n = false, int shared_scalars = 0)
      : ctx_(&ctx), n_(n), kR_(residuals_per_item), kD_(item_scalars), kH_(header_scalars),
        xdim_(manifold == TOA_MANIFOLD_SE3 ? 12 : (manifold == TOA_MANIFOLD_USER ? x_scalars : n)), diff_(diff), manifold_(manifold), kind_(kind), large_n_(large_n),
        kS_(shared_scalars) {
    if (shared_scalars != 0) {   // (the library refuses the same, toa_model_compile_ex: here before anything is compiled)
      if (shared_scalars < 0 || shared_scalars > 512) throw std::invalid_argument("tinyopt_amd::JitResidual: shared_scalars must be in 0 .. 512 (0 = no shared item table)");
      if (kind == TOA_JIT_COST || kind == TOA_JIT_COST_GRAD || kind == TOA_JIT_COST_HESS)
        detail::refuse_shared("kJitResidual, kJitAccumulate and kJitCostGgn take a table (the row models stage it)");
      if (manifold != TOA_MANIFOLD_EUCLID) detail::refuse_shared("Euclidean parameters only");
      if (large_n) detail::refuse_shared("no large_n");
    }
    std::vector<char> log(1 << 16);
    toa_jit_spec spec{};
    spec.dtype = dtype_of<Scalar>(); spec.num_params = n; spec.residuals_per_item = residuals_per_item;
    spec.scalars_per_item = item_scalars; spec.header_scalars = header_scalars; spec.manifold = manifold; spec.kind = kind;
    if (manifold == TOA_MANIFOLD_USER) { spec.x_scalars = x_scalars; spec.plus_body = plus_body.c_str(); }
    spec.diff = diff; spec.diff_h = diff_h;
    spec.large_n = large_n ? 1 : 0;
    spec.shared_scalars = shared_scalars;
    const int rc = toa_model_compile_ex(ctx.get(), &spec, body.c_str(), &h_, log.data(), log.size());
    log_ = log.data();
    check(rc);
  }
  ~JitResidual() { if (h_) (void)toa_model_destroy(h_); }
  JitResidual(const JitResidual&) = delete;
  JitResidual& operator=(const JitResidual&) = delete;
  // data: [P][header_scalars + items * item_scalars] host scalars
  JitModel<Scalar> bind(int64_t P, int items, const Scalar* data) const {
    if (kS_ > 0) detail::refuse_shared("bind has no table: bind_shared(P, items, data, table)");
    return JitModel<Scalar>(*this, P, items, data);
  }
  // ... of a model with shared_scalars: table = [items][shared_scalars] host scalars, ONE for the whole batch (row i beside item i's own
  // scalars, in every problem); data as for bind (null where header_scalars = item_scalars = 0)
  JitModel<Scalar> bind_shared(int64_t P, int items, const Scalar* data, const Scalar* table) const {
    if (kS_ == 0) throw std::invalid_argument("tinyopt_amd::bind_shared: the model has no shared item table (shared_scalars = 0): bind(P, items, data)");
    if (!table) throw std::invalid_argument("tinyopt_amd::bind_shared: table must not be null");
    return JitModel<Scalar>(*this, P, items, data, table);
  }
  // A RAGGED batch: counts[p] items for problem p (0 is legal: that problem ends with kSkipped); data: [sum of counts][item_scalars]
  // host scalars, the items of all problems one after another; header: [P][header_scalars] (null without a header).
  RaggedJitModel<Scalar> bind_ragged(const std::vector<int64_t>& counts, const Scalar* data, const Scalar* header = nullptr) const {
    if (kind_ == TOA_JIT_COST_HESS) detail::refuse_cost_hess("no ragged batches (bind_ragged)");
    if (kind_ == TOA_JIT_COST_GGN) detail::refuse_cost_ggn("no ragged batches (bind_ragged)");
    if (kind_ == TOA_JIT_COST_GGN_MULTI) detail::refuse_cost_ggn_multi("no ragged batches (bind_ragged)");
    if (kS_ > 0) detail::refuse_shared("no ragged batches (bind_ragged)");
    return RaggedJitModel<Scalar>(*this, counts, data, header);
  }
  const std::string& compile_log() const { return log_; }
  toa_jit_model handle() const { return h_; }
  const Context& ctx() const { return *ctx_; }
  int n() const { return n_; }
  int residuals_per_item() const { return kR_; }
  int item_scalars() const { return kD_; }
  int header_scalars() const { return kH_; }
  int xdim() const { return xdim_; }   // stored scalars of x per problem (12 for an SE3 pose)
  int diff() const { return diff_; }   // TOA_DIFF_*
  int manifold() const { return manifold_; }   // TOA_MANIFOLD_*
  int kind() const { return kind_; }           // TOA_JIT_*
  bool large_n() const { return large_n_; }    // compiled for the launch-per-phase pipeline (up to 1024 / 512 parameters)
  int shared_scalars() const { return kS_; }   // columns of the batch's shared item table, 0 = none
  // stats of the fused kernel with a Gaussian prior (with_prior), uniform or ragged: toa_jit_model_stats_prior
  struct PriorBuildStats { int wg_per_cu = 0, num_regs = 0, scratch_bytes = 0; };
  PriorBuildStats stats_prior(bool ragged = false) const {
    PriorBuildStats s;
    check(toa_jit_model_stats_prior(ctx_->get(), h_, ragged ? 1 : 0, &s.wg_per_cu, &s.num_regs, &s.scratch_bytes));
    return s;
  }
  // What the run-time build came out as (toa_jit_model_stats): resident workgroups per compute unit, LDS per workgroup, vector
  // registers per lane, scratch bytes per lane — a body heavy enough to spill or to drop to one workgroup shows up here.
  struct BuildStats { int wg_per_cu = 0, lds_bytes_per_wg = 0, num_regs = 0, scratch_bytes = 0; };
  BuildStats stats() const {
    BuildStats s;
    check(toa_jit_model_stats(h_, &s.wg_per_cu, &s.lds_bytes_per_wg, &s.num_regs, &s.scratch_bytes));
    return s;
  }

 private:
  const Context* ctx_;
  toa_jit_model h_ = nullptr;
  int n_, kR_, kD_, kH_, xdim_, diff_, manifold_, kind_;
  bool large_n_;
  int kS_;
  std::string log_;
};
// A Gaussian prior beside a bound run-time model's items (toa_jit_*_prior): per problem r = W (x - mu) after the item pass —
// cost += |r|^2, g += W^T r, H += W^T W, k more residuals; never robustified.  mu: [P][n] host scalars; W: [P][n] with rows = 0 (the
// diagonal form, W = 1 / sigma: GaussianPrior) or [P][rows][n] row-major with 1 <= rows <= n (W = U: tests/cov.cpp:96).  Euclidean
// residual models, the one-launch form only: no host controls, no stepping Optimizer, no diff::Eval / CalculateJac / CheckGradient.
template <typename Scalar>
class PriorTag {
 public:
  bool has_prior() const { return prior_rows_ >= 0; }
  toa_prior prior_pod() const {
    toa_prior p{};
    p.mu_dev = prior_mu_.data(); p.W_dev = prior_W_.data(); p.rows = prior_rows_;
    return p;
  }

 protected:
  void set_prior(const JitResidual<Scalar>& res, int64_t P, const Scalar* mu, const Scalar* W, int rows) {
    if (res.kind() == TOA_JIT_COST_HESS) detail::refuse_cost_hess("no Gaussian prior (with_prior): a prior is a block of residuals, and it has none");
    if (res.kind() == TOA_JIT_COST_GGN) detail::refuse_cost_ggn("no Gaussian prior (with_prior): hand a ridge term over as extra items whose J is a unit vector");
    if (res.kind() == TOA_JIT_COST || res.kind() == TOA_JIT_COST_GRAD)
      throw std::invalid_argument("tinyopt_amd::with_prior: a scalar cost model has no residuals to add a Gaussian prior to");
    if (res.manifold() != TOA_MANIFOLD_EUCLID)
      throw std::invalid_argument("tinyopt_amd::with_prior: x - mu is not the manifold's minus: Euclidean parameters only");
    if (rows < 0 || rows > res.n()) throw std::invalid_argument("tinyopt_amd::with_prior: rows must be 0 (diagonal) or 1 .. n");
    if (!mu || !W) throw std::invalid_argument("tinyopt_amd::with_prior: mu / W must not be null");
    const size_t n = size_t(res.n()), per = rows ? size_t(rows) * n : n;
    prior_mu_ = DeviceBuffer<Scalar>(res.ctx(), std::max<size_t>(1, size_t(P) * n));
    prior_W_ = DeviceBuffer<Scalar>(res.ctx(), std::max<size_t>(1, size_t(P) * per));
    if (P > 0) {
      check(toa_memcpy_h2d(res.ctx().get(), prior_mu_.data(), mu, size_t(P) * n * sizeof(Scalar)));
      check(toa_memcpy_h2d(res.ctx().get(), prior_W_.data(), W, size_t(P) * per * sizeof(Scalar)));
    }
    prior_rows_ = rows;
  }

 private:
  DeviceBuffer<Scalar> prior_mu_, prior_W_;
  int prior_rows_ = -1;   // -1: no prior
};
// Box bounds and fixed parameters of a bound run-time model (toa_jit_*_bounds): per problem lo <= x <= hi, [P][n]
// host scalars each; nullptr for a side: no bound there (-inf / +inf); lo == hi holds a parameter constant.  x0 is clipped into the
// box, after every Build the parameters on a bound with the gradient pointing outward (and the fixed ones) leave the system (g_j = 0,
// row and column j of H zero, H_jj = 1), every step is clipped: every x visited and returned is inside the box exactly.
// final_hessian is the projected matrix of the last Build (Covariance: the inverse of the free block, 1 on the active diagonal).
// Clip-and-reject, not a trust-region reflection: a small max_consec_failures can stop a solve short of the constrained optimum.
// Euclidean residual models, the one-launch form only: no host controls, no stepping Optimizer, no diff::Eval / CalculateJac /
// CheckGradient.  Composes with with_loss and with_prior in any order.
template <typename Scalar>
class BoundsTag {
 public:
  bool has_bounds() const { return has_bounds_; }
  toa_bounds bounds_pod() const {
    toa_bounds b{};
    b.lo_dev = lo_.data(); b.hi_dev = hi_.data();
    return b;
  }

 protected:
  void set_bounds(const JitResidual<Scalar>& res, int64_t P, const Scalar* lo, const Scalar* hi) {
    if (res.large_n())
      throw std::invalid_argument("tinyopt_amd::with_bounds: a model compiled with large_n takes no box bounds");
    if (res.kind() == TOA_JIT_COST_HESS) detail::refuse_cost_hess("no box bounds (with_bounds): they project the Gauss-Newton system of a residual model");
    if (res.kind() == TOA_JIT_COST_GGN) detail::refuse_cost_ggn("no box bounds (with_bounds)");
    if (res.kind() == TOA_JIT_COST_GGN_MULTI) detail::refuse_cost_ggn_multi("no box bounds (with_bounds)");
    if (res.kind() == TOA_JIT_COST || res.kind() == TOA_JIT_COST_GRAD)
      throw std::invalid_argument("tinyopt_amd::with_bounds: a scalar cost model has no Gauss-Newton system to project");
    if (res.manifold() != TOA_MANIFOLD_EUCLID)
      throw std::invalid_argument("tinyopt_amd::with_bounds: a box on the tangent is not a box on the parameter: Euclidean parameters only");
    const size_t count = size_t(P) * size_t(res.n());
    const Scalar inf = std::numeric_limits<Scalar>::infinity();
    std::vector<Scalar> l(count, -inf), h(count, inf);
    if (lo) l.assign(lo, lo + count);
    if (hi) h.assign(hi, hi + count);
    for (size_t i = 0; i < count; ++i)
      if (!(l[i] <= h[i])) throw std::invalid_argument("tinyopt_amd::with_bounds: lo <= hi must hold for every parameter of every problem, without NaN");
    lo_ = DeviceBuffer<Scalar>(res.ctx(), std::max<size_t>(1, count));
    hi_ = DeviceBuffer<Scalar>(res.ctx(), std::max<size_t>(1, count));
    if (count > 0) {
      check(toa_memcpy_h2d(res.ctx().get(), lo_.data(), l.data(), count * sizeof(Scalar)));
      check(toa_memcpy_h2d(res.ctx().get(), hi_.data(), h.data(), count * sizeof(Scalar)));
    }
    has_bounds_ = true;
  }

 private:
  DeviceBuffer<Scalar> lo_, hi_;
  bool has_bounds_ = false;
};
template <typename Scalar>
class JitModel : public LossTag, public PriorTag<Scalar>, public BoundsTag<Scalar> {
 public:
  JitModel& with_bounds(const Scalar* lo, const Scalar* hi) & { this->set_bounds(*res_, P_, lo, hi); return *this; }
  JitModel&& with_bounds(const Scalar* lo, const Scalar* hi) && { this->set_bounds(*res_, P_, lo, hi); return std::move(*this); }
  JitModel& with_prior(const Scalar* mu, const Scalar* W, int rows = 0) & { this->set_prior(*res_, P_, mu, W, rows); return *this; }
  JitModel&& with_prior(const Scalar* mu, const Scalar* W, int rows = 0) && { this->set_prior(*res_, P_, mu, W, rows); return std::move(*this); }
  JitModel(const JitResidual<Scalar>& res, int64_t P, int items, const Scalar* host)
      : res_(&res), P_(P), items_(items), data_(res.ctx(), size_t(P) * (res.header_scalars() + size_t(items) * res.item_scalars())) {
    data_.upload(host);
  }
  // ... with the batch's shared item table (JitResidual::bind_shared)
  JitModel(const JitResidual<Scalar>& res, int64_t P, int items, const Scalar* host, const Scalar* table)
      : res_(&res), P_(P), items_(items),
        data_(res.ctx(), std::max<size_t>(1, size_t(P) * (res.header_scalars() + size_t(items) * res.item_scalars()))),   // (never a null data pointer)
        table_(res.ctx(), std::max<size_t>(1, size_t(items) * size_t(res.shared_scalars()))) {
    if (size_t(P) * (res.header_scalars() + size_t(items) * res.item_scalars()) > 0) data_.upload(host);
    if (items > 0) table_.upload(table);
    has_shared_ = true;
  }
  bool has_shared() const { return has_shared_; }
  toa_shared shared_pod() const {
    toa_shared s{};
    s.table_dev = table_.data(); s.rows = items_;
    return s;
  }
  static constexpr int model_id = -1;
  int64_t P() const { return P_; }
  int n() const { return res_->n(); }
  int m() const { return items_ * res_->residuals_per_item(); }
  int xdim() const { return res_->xdim(); }
  int items() const { return items_; }
  const Scalar* data() const { return data_.data(); }
  const Context& ctx() const { return res_->ctx(); }
  toa_jit_model jit_handle() const { return res_->handle(); }
  int diff() const { return res_->diff(); }
  int kind() const { return res_->kind(); }   // TOA_JIT_*

 private:
  const JitResidual<Scalar>* res_;
  int64_t P_;
  int items_;
  DeviceBuffer<Scalar> data_, table_;
  bool has_shared_ = false;
};
// A JitResidual bound to a ragged batch (toa_jit_*_ragged): taken by Optimize (LM, GN; GradientDescent for cost kinds), diff::Eval
// and diff::CalculateJac, whose outputs are concatenated like the items.  One-launch form only: no host controls (stop callbacks,
// max_duration_ms, the log line), no stepping Optimizer, no diff::CheckGradient.
template <typename Scalar>
class RaggedJitModel : public LossTag, public PriorTag<Scalar>, public BoundsTag<Scalar> {
 public:
  RaggedJitModel& with_bounds(const Scalar* lo, const Scalar* hi) & { this->set_bounds(*res_, P_, lo, hi); return *this; }
  RaggedJitModel&& with_bounds(const Scalar* lo, const Scalar* hi) && { this->set_bounds(*res_, P_, lo, hi); return std::move(*this); }
  RaggedJitModel& with_prior(const Scalar* mu, const Scalar* W, int rows = 0) & { this->set_prior(*res_, P_, mu, W, rows); return *this; }
  RaggedJitModel&& with_prior(const Scalar* mu, const Scalar* W, int rows = 0) && { this->set_prior(*res_, P_, mu, W, rows); return std::move(*this); }
  RaggedJitModel(const JitResidual<Scalar>& res, const std::vector<int64_t>& counts, const Scalar* host, const Scalar* header)
      : res_(&res), P_(int64_t(counts.size())), offsets_host_(counts.size() + 1, 0) {
    for (size_t p = 0; p < counts.size(); ++p) {
      if (counts[p] < 0) throw std::invalid_argument("tinyopt_amd::bind_ragged: a count is negative");
      if (counts[p] * res.residuals_per_item() >= (int64_t(1) << 31)) throw std::invalid_argument("tinyopt_amd::bind_ragged: a problem has 2^31 residual rows or more");
      offsets_host_[p + 1] = offsets_host_[p] + counts[p];
      if (counts[p] > max_items_) max_items_ = int(counts[p]);
    }
    if (res.header_scalars() > 0 && !header) throw std::invalid_argument("tinyopt_amd::bind_ragged: the model has header scalars: header must not be null");
    offsets_ = DeviceBuffer<int64_t>(res.ctx(), offsets_host_.size());
    offsets_.upload(offsets_host_.data());
    const size_t elems = size_t(total_items()) * size_t(res.item_scalars());
    data_ = DeviceBuffer<Scalar>(res.ctx(), std::max<size_t>(1, elems));   // (never a null data pointer, even without items)
    if (elems > 0) data_.upload(host);
    if (res.header_scalars() > 0) {
      header_ = DeviceBuffer<Scalar>(res.ctx(), std::max<size_t>(1, size_t(P_) * res.header_scalars()));
      if (P_ > 0) header_.upload(header);
    }
  }
  static constexpr int model_id = -1;
  int64_t P() const { return P_; }
  int n() const { return res_->n(); }
  int xdim() const { return res_->xdim(); }
  int max_items() const { return max_items_; }
  int64_t total_items() const { return offsets_host_.back(); }
  int64_t rows() const { return total_items() * res_->residuals_per_item(); }   // residual rows of the whole batch
  const std::vector<int64_t>& offsets() const { return offsets_host_; }
  const int64_t* offsets_dev() const { return offsets_.data(); }
  const Scalar* data() const { return data_.data(); }
  const Scalar* header() const { return res_->header_scalars() > 0 ? header_.data() : nullptr; }
  const Context& ctx() const { return res_->ctx(); }
  toa_jit_model ragged_handle() const { return res_->handle(); }

 private:
  const JitResidual<Scalar>* res_;
  int64_t P_;
  int max_items_ = 0;
  std::vector<int64_t> offsets_host_;
  DeviceBuffer<int64_t> offsets_;
  DeviceBuffer<Scalar> data_, header_;
};
namespace detail {
template <typename C, typename = void> struct is_ragged : std::false_type {};
template <typename C> struct is_ragged<C, std::void_t<decltype(std::declval<const C&>().ragged_handle())>> : std::true_type {};
template <typename C, typename = void> struct is_jit : std::false_type {};
template <typename C> struct is_jit<C, std::void_t<decltype(std::declval<const C&>().jit_handle())>> : std::true_type {};
template <typename C, typename = void> struct takes_prior : std::false_type {};
template <typename C> struct takes_prior<C, std::void_t<decltype(std::declval<const C&>().has_prior())>> : std::true_type {};
template <typename C>
inline bool has_prior(const C& cost) {
  if constexpr (takes_prior<C>::value) return cost.has_prior();
  else return false;
}
template <typename C, typename = void> struct takes_bounds : std::false_type {};
template <typename C> struct takes_bounds<C, std::void_t<decltype(std::declval<const C&>().has_bounds())>> : std::true_type {};
template <typename C>
inline bool has_bounds(const C& cost) {
  if constexpr (takes_bounds<C>::value) return cost.has_bounds();
  else return false;
}
inline void refuse_bounds(const char* what) {
  throw std::invalid_argument(std::string("tinyopt_amd: box bounds (with_bounds) stand on a Euclidean residual model in the one-launch form only: ") + what);
}
inline void refuse_prior(const char* what) {
  throw std::invalid_argument(std::string("tinyopt_amd: a Gaussian prior (with_prior) stands beside a Euclidean residual model in the one-launch form only: ") + what);
}
}  // namespace detail

// include/tinyopt/output.h:26-145, one entry per problem.
struct BatchOutput {
  std::vector<int32_t> stop_reason, num_iters, num_failures, num_consec_failures, final_num_residuals;
  std::vector<double> final_cost, final_rerr_dec;
  std::vector<float> final_inlier_ratio;      // Output::final_cost.inlier_ratio (cost.h:84-95); 1 without a robust loss
  std::vector<double> final_hessian;          // [P][n*n], undamped; empty unless options.hessian.save_last
  std::vector<double> errs, deltas2;          // [P][hist_stride] (only with history = true)
  std::vector<uint8_t> successes;
  int hist_stride = 0;
  bool Succeeded(size_t p) const { return stop_reason[p] >= kNone; }                                  // output.h:30
  bool Converged(size_t p) const { return stop_reason[p] >= kMinError && stop_reason[p] < kMaxIters; } // output.h:33-35
};

// include/tinyopt/output.h:26-145 for ONE problem — what the P == 1 overload of Optimize returns, so that a call site of
// the reference (`const auto& out = Optimize(x, loss, options); REQUIRE(out.Succeeded());`) keeps compiling.
struct Output {
  int32_t stop_reason = kNone;
  int32_t num_iters = 0, num_failures = 0, num_consec_failures = 0;
  struct Cost_ { double cost = 0; int32_t num_resisuals = 0; float inlier_ratio = 1; } final_cost;   // cost.h:18-97
  double final_rerr_dec = 0;
  std::vector<double> final_hessian;   // n*n, undamped; empty unless options.hessian.save_last
  std::vector<double> errs, deltas2;   // one entry per iteration (only with history = true)
  std::vector<bool> successes;
  bool Succeeded() const { return stop_reason >= kNone; }
  bool Converged() const { return stop_reason >= kMinError && stop_reason < kMaxIters; }
};

// In which order the persistent kernel hands out the problems of a ragged batch (Optimize's last argument).
enum class QueueOrder { kLongestFirst = 0, kKeepOrder };

template <typename Scalar, typename Cost>
BatchOutput OptimizeWithHostControls(std::vector<Scalar>& x, const Cost& cost, const Options& options, bool history);

// tinyopt::Optimize(x, cost, options) for a batch.  x: [P][n] contiguous host scalars, updated in place.
// order (ragged batches only): QueueOrder::kKeepOrder hands the problems out in index order instead of longest first
// (TOA_RAGGED_KEEP_ORDER); a type of its own, so that it cannot be passed where `history` goes.
template <typename Scalar, typename Cost>
BatchOutput Optimize(std::vector<Scalar>& x, const Cost& cost, const Options& options = {}, bool history = false,
                     QueueOrder order = QueueOrder::kLongestFirst) {
  const bool keep_order = order == QueueOrder::kKeepOrder;
  const int64_t P = cost.P();
  const int n = cost.n();
  if (int64_t(x.size()) != P * cost.xdim())
    throw std::invalid_argument("tinyopt_amd::Optimize: x must hold P * (parameters per problem) scalars");
  const bool gd = options.solver_type == Options::GradientDescent;
  if (gd && options.has_host_controls())
    throw std::invalid_argument("tinyopt_amd::Optimize: GradientDescent runs as one launch per solve: stop callbacks, max_duration_ms "
                                "and the log line are not supported on this path");
  const bool lbfgs = options.solver_type == Options::LBFGS;
  if (lbfgs) {   // (what is no first-order cost model, and a loss, the library refuses)
    if (options.has_host_controls())
      throw std::invalid_argument("tinyopt_amd::Optimize: L-BFGS runs as one launch per solve: stop callbacks, max_duration_ms and the log "
                                  "line are not supported on this path");
    if (options.grad_clipping != 0)
      throw std::invalid_argument("tinyopt_amd::Optimize: L-BFGS: grad_clipping must be 0 (a clipped gradient makes the pairs' y = g - g_acc meaningless)");
    if (options.lbfgs.history < 1 || options.lbfgs.history > 16) throw std::invalid_argument("tinyopt_amd::Optimize: L-BFGS: lbfgs.history must be in 1 .. 16");
    if (!(options.lbfgs.c1 > 0.0f && options.lbfgs.c1 < 1.0f)) throw std::invalid_argument("tinyopt_amd::Optimize: L-BFGS: lbfgs.c1 must be in (0, 1)");
    if (!(options.lbfgs.shrink > 0.0f && options.lbfgs.shrink < 1.0f))
      throw std::invalid_argument("tinyopt_amd::Optimize: L-BFGS: lbfgs.shrink must be in (0, 1)");
    if (detail::has_bounds(cost)) detail::refuse_bounds("no L-BFGS (and L-BFGS has no box bounds: this is not L-BFGS-B)");
    if (detail::has_prior(cost)) detail::refuse_prior("no L-BFGS");
    if constexpr (!detail::is_jit<Cost>::value && !detail::is_ragged<Cost>::value)
      throw std::invalid_argument("tinyopt_amd::Optimize: L-BFGS (Options::LBFGS) needs a scalar cost model (a JitResidual of a cost kind)");
  }
  if constexpr (detail::is_jit<Cost>::value) {
    if (cost.has_shared()) {
      if (lbfgs) detail::refuse_shared("no L-BFGS");
      if (gd) detail::refuse_shared("no GradientDescent");
      if (options.has_host_controls()) detail::refuse_shared("no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)");
    }
    if (cost.diff() != TOA_DIFF_DEFAULT && options.has_host_controls())
      throw std::invalid_argument("tinyopt_amd::Optimize: a numerically differentiated model runs as one launch per solve: stop callbacks, "
                                  "max_duration_ms and the log line are not supported (it has no stepping form)");
    if (cost.kind() == TOA_JIT_COST_HESS) {
      if (gd) detail::refuse_cost_hess("no GradientDescent: the reference throws for f(x, grad, H) under GradientDescent too (optimize.h:59-75)");
      if (cost.loss_kind != TOA_LOSS_L2) detail::refuse_cost_hess("no M-estimator (with_loss): a scalar cost has no residuals to robustify");
      if (options.has_host_controls()) detail::refuse_cost_hess("no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)");
    }
    if (cost.kind() == TOA_JIT_COST_GGN) {
      if (gd) detail::refuse_cost_ggn("no GradientDescent: run the same cost as kJitCostGrad");
      if (lbfgs) detail::refuse_cost_ggn("no L-BFGS: run the same cost as kJitCostGrad");
      if (cost.loss_kind != TOA_LOSS_L2) detail::refuse_cost_ggn("no M-estimator (with_loss): a scalar cost has no residuals to robustify");
      if (options.has_host_controls()) detail::refuse_cost_ggn("no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)");
    }
    if (cost.kind() == TOA_JIT_COST_GGN_MULTI) {
      if (gd) detail::refuse_cost_ggn_multi("no GradientDescent: run the same cost as kJitCostGrad");
      if (lbfgs) detail::refuse_cost_ggn_multi("no L-BFGS: run the same cost as kJitCostGrad");
      if (cost.loss_kind != TOA_LOSS_L2) detail::refuse_cost_ggn_multi("no M-estimator (with_loss): a scalar cost has no residuals to robustify");
      if (options.has_host_controls()) detail::refuse_cost_ggn_multi("no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)");
    }
  }
  if (detail::has_bounds(cost)) {
    if (options.has_host_controls()) detail::refuse_bounds("no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)");
    if (gd) detail::refuse_bounds("no GradientDescent");
  }
  if (detail::has_prior(cost)) {
    if (options.has_host_controls()) detail::refuse_prior("no stepping form, so no host controls (stop callbacks, max_duration_ms, the log line)");
    if (gd) detail::refuse_prior("no GradientDescent");
  }
  if constexpr (detail::is_ragged<Cost>::value) {
    if (options.has_host_controls())
      throw std::invalid_argument("tinyopt_amd::Optimize: a ragged batch (bind_ragged) runs in the one-launch form only: no stepping form, so "
                                  "no host controls (stop callbacks, max_duration_ms, the log line)");
  } else {
    if (keep_order) throw std::invalid_argument("tinyopt_amd::Optimize: keep_order is the queue order of a ragged batch (bind_ragged)");
    if (options.has_host_controls()) {
      return OptimizeWithHostControls(x, cost, options, history);   // (run-time models too: toa_jit_lm_begin / step / stop)
    }
  }
  const Context& ctx = cost.ctx();
  DeviceBuffer<Scalar> dx(ctx, x.size());
  dx.upload(x.data());
  DeviceBuffer<int32_t> stop(ctx, P), iters(ctx, P), fails(ctx, P), cfails(ctx, P), nres(ctx, P);
  DeviceBuffer<double> fc(ctx, P), fr(ctx, P);
  DeviceBuffer<float> inl(ctx, P);
  DeviceBuffer<double> fH, errs, d2;
  DeviceBuffer<uint8_t> succ;
  toa_results r{};
  r.stop_reason = stop.data(); r.num_iters = iters.data(); r.num_failures = fails.data();
  r.num_consec_failures = cfails.data(); r.final_cost = fc.data(); r.final_num_residuals = nres.data();
  r.final_rerr_dec = fr.data();
  r.final_inlier_ratio = inl.data();
  BatchOutput out;
  const bool save_H = options.hessian.save_last && !gd && !lbfgs;   // (no final Hessian on the first-order paths: optimizer.h:313)
  if (save_H) { fH = DeviceBuffer<double>(ctx, size_t(P) * n * n); fH.zero(); r.final_hessian = fH.data(); }
  if (history) {
    out.hist_stride = options.max_iters + 2;
    errs = DeviceBuffer<double>(ctx, size_t(P) * out.hist_stride); errs.zero();
    d2 = DeviceBuffer<double>(ctx, size_t(P) * out.hist_stride); d2.zero();
    succ = DeviceBuffer<uint8_t>(ctx, size_t(P) * out.hist_stride); succ.zero();
    r.errs = errs.data(); r.deltas2 = d2.data(); r.successes = succ.data(); r.hist_stride = out.hist_stride;
  }
  const toa_options pod = options.to_pod();
  apply_loss(cost);
  if constexpr (detail::is_ragged<Cost>::value) {
    const uint32_t flags = keep_order ? TOA_RAGGED_KEEP_ORDER : 0u;
    if (gd) {
      const toa_gd_options gpod = options.gd_pod();
      check(toa_jit_gd_run_ragged(ctx.get(), cost.ragged_handle(), cost.offsets_dev(), cost.header(), cost.max_items(), cost.total_items(), P,
                                  cost.data(), dx.data(), &pod, &gpod, &r, nullptr, flags));
    } else if (lbfgs) {
      const toa_lbfgs_options lpod = options.lbfgs_pod();
      check(toa_jit_lbfgs_run_ragged(ctx.get(), cost.ragged_handle(), cost.offsets_dev(), cost.header(), cost.max_items(), cost.total_items(), P,
                                     cost.data(), dx.data(), &pod, &lpod, &r, nullptr, flags));
    } else if (cost.has_bounds()) {
      const toa_bounds bd = cost.bounds_pod();
      const toa_prior pr = cost.has_prior() ? cost.prior_pod() : toa_prior{};
      check(toa_jit_lm_run_ragged_bounds(ctx.get(), cost.ragged_handle(), cost.offsets_dev(), cost.header(), cost.max_items(), cost.total_items(), P,
                                         cost.data(), dx.data(), &bd, cost.has_prior() ? &pr : nullptr, &pod, &r, nullptr, flags));
    } else if (cost.has_prior()) {
      const toa_prior pr = cost.prior_pod();
      check(toa_jit_lm_run_ragged_prior(ctx.get(), cost.ragged_handle(), cost.offsets_dev(), cost.header(), cost.max_items(), cost.total_items(), P,
                                        cost.data(), dx.data(), &pr, &pod, &r, nullptr, flags));
    } else {
      check(toa_jit_lm_run_ragged(ctx.get(), cost.ragged_handle(), cost.offsets_dev(), cost.header(), cost.max_items(), cost.total_items(), P,
                                  cost.data(), dx.data(), &pod, &r, nullptr, flags));
    }
  } else if constexpr (detail::is_jit<Cost>::value) {
    if (cost.has_shared()) {   // (GradientDescent and L-BFGS were refused above) the table beside the batch; bounds and prior, each or NULL
      const toa_shared sh = cost.shared_pod();
      const toa_bounds bd = cost.has_bounds() ? cost.bounds_pod() : toa_bounds{};
      const toa_prior pr = cost.has_prior() ? cost.prior_pod() : toa_prior{};
      check(toa_jit_lm_run_shared(ctx.get(), cost.jit_handle(), cost.items(), P, cost.data(), &sh, dx.data(), cost.has_bounds() ? &bd : nullptr,
                                  cost.has_prior() ? &pr : nullptr, &pod, &r, nullptr));
    } else if (gd) {   // gd::Optimizer on a scalar cost model (the library refuses any other model: optimize.h:59-75)
      const toa_gd_options gpod = options.gd_pod();
      check(toa_jit_gd_run(ctx.get(), cost.jit_handle(), cost.items(), P, cost.data(), dx.data(), &pod, &gpod, &r, nullptr));
    } else if (lbfgs) {   // (the library refuses any model that is no first-order scalar cost)
      const toa_lbfgs_options lpod = options.lbfgs_pod();
      check(toa_jit_lbfgs_run(ctx.get(), cost.jit_handle(), cost.items(), P, cost.data(), dx.data(), &pod, &lpod, &r, nullptr));
    } else if (cost.has_bounds()) {
      const toa_bounds bd = cost.bounds_pod();
      const toa_prior pr = cost.has_prior() ? cost.prior_pod() : toa_prior{};
      check(toa_jit_lm_run_bounds(ctx.get(), cost.jit_handle(), cost.items(), P, cost.data(), dx.data(), &bd, cost.has_prior() ? &pr : nullptr, &pod, &r,
                                  nullptr));
    } else if (cost.has_prior()) {
      const toa_prior pr = cost.prior_pod();
      check(toa_jit_lm_run_prior(ctx.get(), cost.jit_handle(), cost.items(), P, cost.data(), dx.data(), &pr, &pod, &r, nullptr));
    } else {
      check(toa_jit_lm_run(ctx.get(), cost.jit_handle(), cost.items(), P, cost.data(), dx.data(), &pod, &r, nullptr));
    }
  } else
    check(toa_lm_run(ctx.get(), Cost::model_id, dtype_of<Scalar>(), n, cost.m(), P, cost.data(), dx.data(), &pod, &r, nullptr));
  check(toa_synchronize(ctx.get()));
  dx.download(x.data());
  auto get = [&](auto& vec, const auto& buf) { vec.resize(buf.size()); buf.download(vec.data()); };
  get(out.stop_reason, stop); get(out.num_iters, iters); get(out.num_failures, fails);
  get(out.num_consec_failures, cfails); get(out.final_num_residuals, nres); get(out.final_cost, fc);
  get(out.final_rerr_dec, fr); get(out.final_inlier_ratio, inl);
  if (save_H) get(out.final_hessian, fH);
  if (history) { get(out.errs, errs); get(out.deltas2, d2); get(out.successes, succ); }
  return out;
}

// diff::CheckGradient / diff::CheckResidualsGradient (diff/gradient_check.h:50-220) for a bound run-time model of any kind, at
// x [P][n]: the model's own derivatives against finite differences of its residuals (cost terms) with step eps / 10 — g = J^T r and,
// with check_H, H = J^T J for residual kinds; g for cost kinds.  eps <= 0: the reference's default (1e-2 for float, 1e-5 for double).
struct GradientCheck {
  std::vector<int32_t> ok;                    // [P]
  std::vector<double> max_dist_g, max_dist_H; // [P]
  bool all() const { for (int32_t v : ok) if (!v) return false; return true; }
  explicit operator bool() const { return all(); }
};
namespace diff {
template <typename Scalar>
GradientCheck CheckGradient(const JitModel<Scalar>& model, const std::vector<Scalar>& x, double eps = 0.0, Method method = kCentral,
                            bool check_H = true) {
  const int64_t P = model.P();
  if (int64_t(x.size()) != P * model.xdim())
    throw std::invalid_argument("tinyopt_amd::diff::CheckGradient: x must hold P * (parameters per problem) scalars");
  if (model.has_shared())
    detail::refuse_shared("no CheckGradient (compare Accumulate of a kJitAccumulate body with Accumulate of its residuals under diff::kCentral, both with the table)");
  if (model.has_bounds()) detail::refuse_bounds("no CheckGradient (it checks the model's own rows)");
  if (model.has_prior()) detail::refuse_prior("no CheckGradient (it checks the model's own rows)");
  const Context& ctx = model.ctx();
  DeviceBuffer<Scalar> dx(ctx, x.size());
  dx.upload(x.data());
  DeviceBuffer<double> dist(ctx, size_t(P) * 2);
  DeviceBuffer<int32_t> ok(ctx, size_t(P));
  apply_loss(model);
  check(toa_jit_check_gradient(ctx.get(), model.jit_handle(), model.items(), P, model.data(), dx.data(), eps, to_pod(method), check_H ? 1 : 0,
                               dist.data(), ok.data()));
  check(toa_synchronize(ctx.get()));
  GradientCheck out;
  out.ok.resize(size_t(P));
  ok.download(out.ok.data());
  std::vector<double> d(size_t(P) * 2);
  dist.download(d.data());
  out.max_dist_g.resize(size_t(P));
  out.max_dist_H.resize(size_t(P));
  for (size_t p = 0; p < size_t(P); ++p) { out.max_dist_g[p] = d[2 * p]; out.max_dist_H[p] = d[2 * p + 1]; }
  return out;
}

// a ragged batch has no gradient checker: check the model on a uniform batch (JitResidual::bind)
template <typename Scalar>
GradientCheck CheckGradient(const RaggedJitModel<Scalar>&, const std::vector<Scalar>&, double = 0.0, Method = kCentral, bool = true) = delete;

// diff::Eval / diff::CalculateJac (diff/auto_diff.h:14-138) for a bound run-time residual model at x [P][xdim]: the residuals
// [P][m] and the Jacobian rows [P][m][n], row-major, m = items x residuals_per_item in the row order of the Accumulate seam; on a
// manifold J is over the tangent.  A numeric model (JitResidual's diff argument) gives NumEval / EstimateNumJac.  Not for scalar
// cost models and not with a loss set (the library refuses both).
template <typename Scalar>
std::pair<std::vector<Scalar>, std::vector<Scalar>> Eval(const JitModel<Scalar>& model, const std::vector<Scalar>& x, bool jac = true) {
  const int64_t P = model.P();
  if (int64_t(x.size()) != P * model.xdim())
    throw std::invalid_argument("tinyopt_amd::diff::Eval: x must hold P * (parameters per problem) scalars");
  if (model.has_shared()) detail::refuse_shared("no Eval / CalculateJac (their kernels read replicated items)");
  if (model.has_bounds()) detail::refuse_bounds("no Eval / CalculateJac (they return the model's own rows)");
  if (model.has_prior()) detail::refuse_prior("no Eval / CalculateJac (they return the model's own rows)");
  const Context& ctx = model.ctx();
  const size_t rows = size_t(P) * size_t(model.m());
  DeviceBuffer<Scalar> dx(ctx, x.size());
  dx.upload(x.data());
  DeviceBuffer<Scalar> res(ctx, rows);
  DeviceBuffer<Scalar> J(ctx, jac ? rows * size_t(model.n()) : size_t(1));
  apply_loss(model);
  check(toa_jit_eval(ctx.get(), model.jit_handle(), model.items(), P, model.data(), dx.data(), res.data(), jac ? J.data() : nullptr));
  check(toa_synchronize(ctx.get()));
  std::pair<std::vector<Scalar>, std::vector<Scalar>> out;
  out.first.resize(rows);
  res.download(out.first.data());
  if (jac) { out.second.resize(rows * size_t(model.n())); J.download(out.second.data()); }
  return out;
}
template <typename Scalar>
std::vector<Scalar> CalculateJac(const JitModel<Scalar>& model, const std::vector<Scalar>& x) {
  const int64_t P = model.P();
  if (int64_t(x.size()) != P * model.xdim())
    throw std::invalid_argument("tinyopt_amd::diff::CalculateJac: x must hold P * (parameters per problem) scalars");
  if (model.has_shared()) detail::refuse_shared("no Eval / CalculateJac (their kernels read replicated items)");
  if (model.has_bounds()) detail::refuse_bounds("no Eval / CalculateJac (they return the model's own rows)");
  if (model.has_prior()) detail::refuse_prior("no Eval / CalculateJac (they return the model's own rows)");
  const Context& ctx = model.ctx();
  const size_t elems = size_t(P) * size_t(model.m()) * size_t(model.n());
  DeviceBuffer<Scalar> dx(ctx, x.size());
  dx.upload(x.data());
  DeviceBuffer<Scalar> J(ctx, elems);
  apply_loss(model);
  check(toa_jit_eval(ctx.get(), model.jit_handle(), model.items(), P, model.data(), dx.data(), nullptr, J.data()));
  check(toa_synchronize(ctx.get()));
  std::vector<Scalar> out(elems);
  J.download(out.data());
  return out;
}
// ... and for a ragged batch: the outputs concatenated like the items — res [rows], J [rows][n], rows = total_items x residuals_per_item.
template <typename Scalar>
std::pair<std::vector<Scalar>, std::vector<Scalar>> Eval(const RaggedJitModel<Scalar>& model, const std::vector<Scalar>& x, bool jac = true, bool res = true) {
  const int64_t P = model.P();
  if (int64_t(x.size()) != P * model.xdim())
    throw std::invalid_argument("tinyopt_amd::diff::Eval: x must hold P * (parameters per problem) scalars");
  if (model.has_bounds()) detail::refuse_bounds("no Eval / CalculateJac (they return the model's own rows)");
  if (model.has_prior()) detail::refuse_prior("no Eval / CalculateJac (they return the model's own rows)");
  const Context& ctx = model.ctx();
  const size_t rows = size_t(model.rows());
  DeviceBuffer<Scalar> dx(ctx, std::max<size_t>(1, x.size()));
  if (!x.empty()) dx.upload(x.data());
  DeviceBuffer<Scalar> rbuf(ctx, std::max<size_t>(1, rows));
  DeviceBuffer<Scalar> J(ctx, jac ? std::max<size_t>(1, rows * size_t(model.n())) : size_t(1));
  apply_loss(model);
  check(toa_jit_eval_ragged(ctx.get(), model.ragged_handle(), model.offsets_dev(), model.header(), model.max_items(), model.total_items(), P,
                            model.data(), dx.data(), res ? rbuf.data() : nullptr, jac ? J.data() : nullptr));
  check(toa_synchronize(ctx.get()));
  std::pair<std::vector<Scalar>, std::vector<Scalar>> out;
  if (res && rows) { std::vector<Scalar> t(rbuf.size()); rbuf.download(t.data()); out.first.assign(t.begin(), t.begin() + rows); }
  if (jac && rows) { std::vector<Scalar> t(J.size()); J.download(t.data()); out.second.assign(t.begin(), t.begin() + rows * size_t(model.n())); }
  return out;
}
template <typename Scalar>
std::vector<Scalar> CalculateJac(const RaggedJitModel<Scalar>& model, const std::vector<Scalar>& x) {
  return Eval(model, x, true, false).second;
}
}  // namespace diff

// The reference's class / stepping form (`lm::Optimizer<H_t> optimizer(options)`; `optimizer.Step(x, acc, out)` one loop
// pass at a time; `optimizer(x, f, max_iters)` — include/tinyopt/optimizers/optimizer.h:199,331-539) for a batch.
// x stays on the device between steps; `x()` downloads the current iterate, `output()` the results so far.
template <typename Scalar, typename Cost>
class Optimizer {
  static_assert(!detail::is_ragged<Cost>::value, "a ragged batch (bind_ragged) runs in the one-launch form only: no stepping Optimizer");

 public:
  Optimizer(std::vector<Scalar>& x, const Cost& cost, const Options& options = {}, bool history = false)
      : x_(&x), cost_(&cost), options_(options), pod_(options.to_pod()), P_(cost.P()), n_(cost.n()),
        dx_(cost.ctx(), x.size()), stop_(cost.ctx(), P_), iters_(cost.ctx(), P_), fails_(cost.ctx(), P_), cfails_(cost.ctx(), P_),
        nres_(cost.ctx(), P_), fc_(cost.ctx(), P_), fr_(cost.ctx(), P_), inl_(cost.ctx(), P_), active_(cost.ctx(), 1),
        state_(cost.ctx(), toa_lm_state_bytes(dtype_of<Scalar>(), n_, P_)) {
    if (int64_t(x.size()) != P_ * cost.xdim())
      throw std::invalid_argument("tinyopt_amd::Optimizer: x must hold P * (parameters per problem) scalars");
    if constexpr (detail::is_jit<Cost>::value) {
      if (cost.has_shared()) detail::refuse_shared("no stepping form (Optimizer)");
    }
    if (detail::has_bounds(cost)) detail::refuse_bounds("no stepping form (Optimizer)");
    if (detail::has_prior(cost)) detail::refuse_prior("no stepping form (Optimizer)");
    dx_.upload(x.data());
    stop_.zero(); iters_.zero(); fc_.zero();
    r_ = toa_results{};
    r_.stop_reason = stop_.data(); r_.num_iters = iters_.data(); r_.num_failures = fails_.data();
    r_.num_consec_failures = cfails_.data(); r_.final_cost = fc_.data(); r_.final_num_residuals = nres_.data();
    r_.final_rerr_dec = fr_.data(); r_.final_inlier_ratio = inl_.data();
    if (options.hessian.save_last) { fH_ = DeviceBuffer<double>(cost.ctx(), size_t(P_) * n_ * n_); fH_.zero(); r_.final_hessian = fH_.data(); }
    if (history) {
      hist_stride_ = options.max_iters + 2;
      errs_ = DeviceBuffer<double>(cost.ctx(), size_t(P_) * hist_stride_); errs_.zero();
      d2_ = DeviceBuffer<double>(cost.ctx(), size_t(P_) * hist_stride_); d2_.zero();
      succ_ = DeviceBuffer<uint8_t>(cost.ctx(), size_t(P_) * hist_stride_); succ_.zero();
      r_.errs = errs_.data(); r_.deltas2 = d2_.data(); r_.successes = succ_.data(); r_.hist_stride = hist_stride_;
    }
    apply_loss(cost);
    if constexpr (detail::is_jit<Cost>::value)
      check(toa_jit_lm_begin(cost.ctx().get(), cost.jit_handle(), cost.items(), P_, cost.data(), dx_.data(), &pod_, &r_, state_.data()));
    else
      check(toa_lm_begin(cost.ctx().get(), Cost::model_id, dtype_of<Scalar>(), n_, cost.m(), P_, cost.data(), dx_.data(), &pod_, &r_,
                         state_.data()));
  }
  // One pass of the loop body for every running problem; returns how many are still running.
  int64_t Step() {
    const Context& ctx = cost_->ctx();
    active_.zero();
    apply_loss(*cost_);
    if constexpr (detail::is_jit<Cost>::value)
      check(toa_jit_lm_step(ctx.get(), cost_->jit_handle(), cost_->items(), P_, cost_->data(), dx_.data(), &pod_, &r_, nullptr,
                            state_.data(), active_.data()));
    else
      check(toa_lm_step(ctx.get(), Cost::model_id, dtype_of<Scalar>(), n_, cost_->m(), P_, cost_->data(), dx_.data(), &pod_, &r_,
                        nullptr, state_.data(), active_.data()));
    check(toa_synchronize(ctx.get()));
    int32_t a = 0;
    active_.download(&a);
    dx_.download(x_->data());  // x by reference, updated in place at every Step (optimizer.h:271-279)
    return a;
  }
  // `optimizer(x, f, max_iters)`
  BatchOutput operator()(int max_iters = -1) {
    const int limit = max_iters < 0 ? int(options_.max_iters) + 2 : max_iters;
    for (int i = 0; i < limit; ++i)
      if (Step() == 0) break;
    return output();
  }
  BatchOutput output() const {
    BatchOutput out;
    auto get = [&](auto& vec, const auto& buf) { vec.resize(buf.size()); buf.download(vec.data()); };
    get(out.stop_reason, stop_); get(out.num_iters, iters_); get(out.num_failures, fails_);
    get(out.num_consec_failures, cfails_); get(out.final_num_residuals, nres_); get(out.final_cost, fc_);
    get(out.final_rerr_dec, fr_); get(out.final_inlier_ratio, inl_);
    if (options_.hessian.save_last) get(out.final_hessian, fH_);
    if (hist_stride_) { out.hist_stride = hist_stride_; get(out.errs, errs_); get(out.deltas2, d2_); get(out.successes, succ_); }
    return out;
  }
  // What the reference hands its stop callbacks after an iteration (optimizer.h:529-534), per problem: the cost, |dx|^2,
  // |g|^2 and — when dx / g are given — the step and gradient vectors ([P][n]).
  void StepInfo(std::vector<double>& err, std::vector<double>& dx2, std::vector<double>& g2, std::vector<Scalar>* dx = nullptr,
                std::vector<Scalar>* g = nullptr) const {
    const Context& ctx = cost_->ctx();
    DeviceBuffer<double> de(ctx, P_), dd(ctx, P_), dg(ctx, P_);
    DeviceBuffer<Scalar> vdx, vg;
    if (dx) vdx = DeviceBuffer<Scalar>(ctx, size_t(P_) * n_);
    if (g) vg = DeviceBuffer<Scalar>(ctx, size_t(P_) * n_);
    check(toa_lm_step_info(ctx.get(), dtype_of<Scalar>(), n_, P_, state_.data(), de.data(), dd.data(), dg.data(),
                           dx ? vdx.data() : nullptr, g ? vg.data() : nullptr));
    check(toa_synchronize(ctx.get()));
    err.resize(P_); dx2.resize(P_); g2.resize(P_);
    de.download(err.data()); dd.download(dx2.data()); dg.download(g2.data());
    if (dx) { dx->resize(size_t(P_) * n_); vdx.download(dx->data()); }
    if (g) { g->resize(size_t(P_) * n_); vg.download(g->data()); }
  }
  // The rest of what the reference's log line prints (optimizer.h:463-516): damping, residual count, inlier residuals.
  void StepLog(std::vector<double>& lambda, std::vector<int32_t>& nres, std::vector<int32_t>& ninl) const {
    const Context& ctx = cost_->ctx();
    DeviceBuffer<double> dl(ctx, P_);
    DeviceBuffer<int32_t> dn(ctx, P_), di(ctx, P_);
    check(toa_lm_step_log(ctx.get(), dtype_of<Scalar>(), n_, P_, state_.data(), dl.data(), dn.data(), di.data()));
    check(toa_synchronize(ctx.get()));
    lambda.resize(P_); nres.resize(P_); ninl.resize(P_);
    dl.download(lambda.data()); dn.download(nres.data()); di.download(ninl.data());
  }
  // Ends the still-running problems p with request[p] != 0 with that StopReason (kUserStopped, kTimedOut).
  void Stop(const std::vector<int32_t>& request) {
    if (int64_t(request.size()) != P_) throw std::invalid_argument("tinyopt_amd::Optimizer::Stop: one request per problem");
    const Context& ctx = cost_->ctx();
    DeviceBuffer<int32_t> dr(ctx, P_);
    dr.upload(request.data());
    if constexpr (detail::is_jit<Cost>::value)
      check(toa_jit_lm_stop(ctx.get(), cost_->jit_handle(), cost_->items(), P_, cost_->data(), dx_.data(), &pod_, &r_, nullptr,
                            state_.data(), dr.data()));
    else
      check(toa_lm_stop(ctx.get(), Cost::model_id, dtype_of<Scalar>(), n_, cost_->m(), P_, cost_->data(), dx_.data(), &pod_, &r_,
                        nullptr, state_.data(), dr.data()));
    check(toa_synchronize(ctx.get()));
  }
  void SetStopReason(const std::vector<int32_t>& stop) { stop_.upload(stop.data()); }

 private:
  std::vector<Scalar>* x_;
  const Cost* cost_;
  Options options_;
  toa_options pod_;
  int64_t P_;
  int n_;
  DeviceBuffer<Scalar> dx_;
  DeviceBuffer<int32_t> stop_, iters_, fails_, cfails_, nres_;
  DeviceBuffer<double> fc_, fr_;
  DeviceBuffer<float> inl_;
  DeviceBuffer<int32_t> active_;
  DeviceBuffer<unsigned char> state_;
  DeviceBuffer<double> fH_, errs_, d2_;
  DeviceBuffer<uint8_t> succ_;
  int hist_stride_ = 0;
  toa_results r_;
};

// Optimize() when Options carries host-side stop controls: the loop of OptimizeAcc (optimizer.h:266-310) driven from the
// host over the stepping form.  After every pass the callbacks see (err, |dx|^2, |g|^2) / (err, dx, g) of each problem no
// numeric stop test has ended (the else-if chain of optimizer.h:519-534); the accumulated wall time is checked against
// max_duration_ms (one clock for the batch) and kTimedOut overrides whatever reason a problem picked up in that same
// pass, as the unconditional assignment at optimizer.h:303-305 does.
template <typename Scalar, typename Cost>
BatchOutput OptimizeWithHostControls(std::vector<Scalar>& x, const Cost& cost, const Options& options, bool history) {
  Optimizer<Scalar, Cost> opt(x, cost, options, history);
  const int64_t P = cost.P();
  const int n = cost.n();
  std::vector<char> running_before(P, 1);
  std::vector<double> err, dx2, g2;
  std::vector<Scalar> dxv, gv;
  std::vector<float> dxf(n), gf(n);
  double duration_ms = 0;
  // the log line's running state (optimizer.h:428-446): the last accepted cost of every logged problem
  std::vector<int64_t> logged;
  if (options.log.enable) {
    if (options.log.problems.empty()) logged.push_back(0);
    for (int64_t q : options.log.problems) if (q >= 0 && q < P) logged.push_back(q);
  }
  const double big = double(std::numeric_limits<Scalar>::max()), eps = sizeof(Scalar) == 4 ? 1e-4 : double(1e-7f);   // math.h:297-301
  std::vector<double> final_cost(logged.size(), big);
  for (int it = 0; it < int(options.max_iters) + 2; ++it) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Scalar> x_before;   // (the line shows the x the iteration STARTED from: the reference forms it inside Step)
    if (!logged.empty() && options.log.print_x) x_before = x;
    const int64_t active = opt.Step();
    if (!logged.empty()) {   // optimizer.h:463-516: the same fields in the same order, one line per logged problem that made this iteration
      std::vector<double> lam;
      std::vector<int32_t> nres, ninl;
      opt.StepInfo(err, dx2, g2, options.log.print_dx ? &dxv : nullptr, nullptr);
      opt.StepLog(lam, nres, ninl);
      const double took = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      const std::vector<Scalar>& xnow = x_before;
      for (size_t li = 0; li < logged.size(); ++li) {
        const int64_t q = logged[li];
        if (!running_before[q]) continue;
        const double fc = final_cost[li], derr = err[q] - fc;
        const bool good = derr < 0.0;
        const double rel = (fc > eps && fc < big) ? (fc - err[q]) / fc : 0.0;
        char buf[256];
        std::string line;
        if (options.log.print_emoji) line += (good || it == 0) ? (it == 0 ? "\xE2\x84\xB9\xEF\xB8\x8F" : "\xE2\x9C\x85") : "\xE2\x9D\x8C";
        std::snprintf(buf, sizeof(buf), "#%d ", it);
        line += buf;
        if (options.log.print_x) {
          const size_t xd = xnow.size() / size_t(P);
          line += "x:[";
          for (size_t j = 0; j < xd; ++j) { std::snprintf(buf, sizeof(buf), j ? " %.6g" : "%.6g", double(xnow[size_t(q) * xd + j])); line += buf; }
          line += "] ";
        }
        std::snprintf(buf, sizeof(buf), "%s:%.4e n:%d d%s:%+.2e r%s:%+.1e |\xCE\xB4x|:%.2e ", options.log.e.c_str(), err[q], int(nres[q]),
                      options.log.e.c_str(), it == 0 ? 0.0 : derr, options.log.e.c_str(), rel, std::sqrt(dx2[q]));
        line += buf;
        if (options.log.print_dx) {
          line += "\xCE\xB4x:[";
          for (int j = 0; j < n; ++j) { std::snprintf(buf, sizeof(buf), j ? " %.6g" : "%.6g", double(dxv[size_t(q) * n + j])); line += buf; }
          line += "] ";
        }
        if (options.min_grad_norm2 > 0) { std::snprintf(buf, sizeof(buf), "|\xE2\x88\x87|:%.2e ", std::sqrt(g2[q])); line += buf; }
        if (options.solver_type == Options::LevenbergMarquardt && lam[q] > 0) {   // SolverLM::stateAsString (lm.h:150-154)
          std::snprintf(buf, sizeof(buf), "\xE2\x97\x8B:%.2e ", 1.0 / lam[q]);
          line += buf;
        }
        if (options.log.print_inliers) {
          std::snprintf(buf, sizeof(buf), "in:%.2f%% (%d) ", 100.0 * ninl[q] / std::max(1, int(nres[q])), int(ninl[q]));
          line += buf;
        }
        if (options.log.print_t) { std::snprintf(buf, sizeof(buf), "\xCF\x84:%.2f ", duration_ms + took); line += buf; }
        if (options.log.sink) options.log.sink(line);
        else std::cout << line << std::endl;
        if (good || it == 0) final_cost[li] = err[q];
      }
    }
    BatchOutput now = opt.output();
    std::vector<char> running(P);
    for (int64_t p = 0; p < P; ++p) running[p] = running_before[p] && now.stop_reason[p] == kNone;
    std::vector<int32_t> req(P, 0);
    bool any = false;
    // The reference evaluates the callbacks inside Step on EVERY iteration (optimizer.h:529-534) and labels kMaxIters only after
    // the loop, when stop_reason is still kNone (:320-321): a problem that used up its iterations in this very pass is
    // consulted too, and a callback returning true makes it kUserStopped, not kMaxIters.
    std::vector<char> just_max(P, 0);
    bool consult = false, relabel = false;
    for (int64_t p = 0; p < P; ++p) {
      just_max[p] = running_before[p] && now.stop_reason[p] == kMaxIters;
      consult = consult || running[p] || just_max[p];
    }
    if (consult && (options.stop_callback || options.stop_callback2)) {
      opt.StepInfo(err, dx2, g2, options.stop_callback2 ? &dxv : nullptr, options.stop_callback2 ? &gv : nullptr);
      for (int64_t p = 0; p < P; ++p) {
        if (!running[p] && !just_max[p]) continue;
        bool stop = options.stop_callback && options.stop_callback(err[p], dx2[p], g2[p]);
        if (!stop && options.stop_callback2) {
          for (int j = 0; j < n; ++j) { dxf[j] = float(dxv[size_t(p) * n + j]); gf[j] = float(gv[size_t(p) * n + j]); }
          stop = options.stop_callback2(float(err[p]), dxf, gf);
        }
        if (stop) {
          if (just_max[p]) { now.stop_reason[p] = kUserStopped; relabel = true; }   // already finalised: only the label changes
          else { req[p] = kUserStopped; any = true; }
        }
      }
      if (relabel) opt.SetStopReason(now.stop_reason);
    }
    (void)active;
    duration_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const bool timed_out = options.max_duration_ms > 0 && duration_ms > options.max_duration_ms;
    if (timed_out)
      for (int64_t p = 0; p < P; ++p)
        if (running[p]) { req[p] = kTimedOut; any = true; }
    if (any) opt.Stop(req);
    if (timed_out) {
      BatchOutput fin = opt.output();
      bool changed = false;
      for (int64_t p = 0; p < P; ++p)
        if (running_before[p] && !running[p]) { fin.stop_reason[p] = kTimedOut; changed = true; }
      if (changed) opt.SetStopReason(fin.stop_reason);
      break;
    }
    bool left = false;
    for (int64_t p = 0; p < P; ++p) { running_before[p] = running[p] && req[p] == 0; left = left || running_before[p]; }
    if (!left) break;
  }
  return opt.output();
}

// ---- C1: a batch sharded over the GPUs of a node, one process per GPU ---------------------------------------
// RAII over toa_comm.  The 128-byte id comes from ONE rank (`Communicator::UniqueId()`) and is handed to the others by the
// host program (MPI_Bcast, a file, a socket): the library has no side channel of its own.
class Communicator {
 public:
  using Id = std::array<char, TOA_COMM_ID_BYTES>;
  static Id UniqueId() { Id id; check(toa_comm_unique_id(id.data())); return id; }
  Communicator(const Context& ctx, const Id& id, int nranks, int rank) : ctx_(&ctx), nranks_(nranks), rank_(rank) {
    check(toa_comm_init_rank(ctx.get(), id.data(), nranks, rank, &c_));
  }
  ~Communicator() { toa_comm_destroy(c_); }
  Communicator(const Communicator&) = delete;
  Communicator& operator=(const Communicator&) = delete;
  toa_comm get() const { return c_; }
  int nranks() const { return nranks_; }
  int rank() const { return rank_; }
  const Context& ctx() const { return *ctx_; }
  // this rank's contiguous block [lo, hi) of the P_total problem ids
  std::pair<int64_t, int64_t> shard(int64_t P_total) const {
    int64_t lo = 0, hi = 0;
    check(toa_shard_range(P_total, rank_, nranks_, &lo, &hi));
    return {lo, hi};
  }

 private:
  const Context* ctx_;
  toa_comm c_ = nullptr;
  int nranks_, rank_;
};

// Optimize() of this rank's shard followed by the ONE collective of the path: x_local / local_cost hold the problems
// comm.shard(P_total) of a batch of P_total.  On the root the returned BatchOutput carries stop_reason / num_iters /
// final_cost of ALL P_total problems in problem-id order and *x_all their parameters; the other ranks get their local
// Output (x_all untouched).  No communication happens during the solve.
template <typename Scalar, typename Cost>
BatchOutput ShardedOptimize(std::vector<Scalar>& x_local, const Cost& local_cost, const Options& options, const Communicator& comm,
                            int64_t P_total, std::vector<Scalar>* x_all, int root = 0) {
  const auto range = comm.shard(P_total);
  if (local_cost.P() != range.second - range.first)
    throw std::invalid_argument("tinyopt_amd::ShardedOptimize: the local model must hold this rank's shard of P_total problems");
  BatchOutput local = Optimize(x_local, local_cost, options);
  const Context& ctx = local_cost.ctx();
  const int xd = local_cost.xdim();
  const int64_t Pl = local_cost.P();
  DeviceBuffer<Scalar> dx(ctx, x_local.size() ? x_local.size() : 1);
  DeviceBuffer<int32_t> ds(ctx, Pl ? Pl : 1), di(ctx, Pl ? Pl : 1);
  DeviceBuffer<double> dc(ctx, Pl ? Pl : 1);
  if (Pl) { dx.upload(x_local.data()); ds.upload(local.stop_reason.data()); di.upload(local.num_iters.data()); dc.upload(local.final_cost.data()); }
  toa_results lr{}, ar{};
  lr.stop_reason = ds.data(); lr.num_iters = di.data(); lr.final_cost = dc.data();
  const bool is_root = comm.rank() == root;
  DeviceBuffer<Scalar> ax;
  DeviceBuffer<int32_t> as, ai;
  DeviceBuffer<double> ac;
  if (is_root) {
    ax = DeviceBuffer<Scalar>(ctx, size_t(P_total) * xd); as = DeviceBuffer<int32_t>(ctx, P_total); ai = DeviceBuffer<int32_t>(ctx, P_total);
    ac = DeviceBuffer<double>(ctx, P_total);
    ar.stop_reason = as.data(); ar.num_iters = ai.data(); ar.final_cost = ac.data();
  }
  check(toa_gather(ctx.get(), comm.get(), dtype_of<Scalar>(), xd, P_total, dx.data(), &lr, root, is_root ? ax.data() : nullptr, &ar));
  check(toa_synchronize(ctx.get()));
  if (!is_root) return local;
  BatchOutput all;
  all.stop_reason.resize(P_total); all.num_iters.resize(P_total); all.final_cost.resize(P_total);
  as.download(all.stop_reason.data()); ai.download(all.num_iters.data()); ac.download(all.final_cost.data());
  if (x_all) { x_all->resize(size_t(P_total) * xd); ax.download(x_all->data()); }
  return all;
}

// ---- the reference's own call shape: ONE parameter block, `Output out = Optimize(x, cost, options)` --------------------
// (include/tinyopt/optimize.h:16-17 takes any `T& x`).  x: a scalar, or any contiguous container with data() / size()
// (std::array, std::vector of another scalar type is excluded by the batch overload above, an Eigen::Matrix, ...) holding
// the parameters of the single problem of `cost` (cost.P() == 1).  Updated in place; returns one Output.
namespace detail {
template <typename X, typename = void> struct is_container : std::false_type {};
template <typename X> struct is_container<X, std::void_t<decltype(std::declval<X&>().data()), decltype(std::declval<X&>().size())>> : std::true_type {};
template <typename S> struct is_std_vector : std::false_type {};
template <typename S, typename A> struct is_std_vector<std::vector<S, A>> : std::true_type {};
inline Output single(const BatchOutput& b, int n, bool history) {
  Output o;
  o.stop_reason = b.stop_reason[0]; o.num_iters = b.num_iters[0]; o.num_failures = b.num_failures[0];
  o.num_consec_failures = b.num_consec_failures[0];
  o.final_cost.cost = b.final_cost[0]; o.final_cost.num_resisuals = b.final_num_residuals[0];
  o.final_cost.inlier_ratio = b.final_inlier_ratio.empty() ? 1.0f : b.final_inlier_ratio[0];
  o.final_rerr_dec = b.final_rerr_dec[0];
  if (!b.final_hessian.empty()) o.final_hessian.assign(b.final_hessian.begin(), b.final_hessian.begin() + size_t(n) * n);
  if (history && b.hist_stride > 0) {
    const int k = std::min<int>(o.num_iters, b.hist_stride);
    o.errs.assign(b.errs.begin(), b.errs.begin() + k);
    o.deltas2.assign(b.deltas2.begin(), b.deltas2.begin() + k);
    for (int i = 0; i < k; ++i) o.successes.push_back(b.successes[i] != 0);
  }
  return o;
}
}  // namespace detail

template <typename X, typename Cost, typename Scalar = std::decay_t<decltype(*std::declval<const Cost&>().data())>,
          std::enable_if_t<!detail::is_std_vector<X>::value && (detail::is_container<X>::value || std::is_arithmetic<X>::value), int> = 0>
Output Optimize(X& x, const Cost& cost, const Options& options = {}, bool history = false) {
  if (cost.P() != 1) throw std::invalid_argument("tinyopt_amd::Optimize(x, cost): this overload solves ONE problem (cost.P() == 1)");
  std::vector<Scalar> xv;
  if constexpr (std::is_arithmetic<X>::value) {
    xv.assign(1, Scalar(x));
  } else {
    xv.resize(x.size());
    for (size_t i = 0; i < xv.size(); ++i) xv[i] = Scalar(x.data()[i]);
  }
  const BatchOutput b = Optimize(xv, cost, options, history);   // throws std::invalid_argument on a size mismatch
  if constexpr (std::is_arithmetic<X>::value) {
    x = X(xv[0]);
  } else {
    for (size_t i = 0; i < xv.size(); ++i) x.data()[i] = static_cast<std::decay_t<decltype(x.data()[0])>>(xv[i]);
  }
  return detail::single(b, cost.n(), history);
}

// The Accumulate-callback seam `acc(x, grad, H) -> Cost` (docs/API.md:37-57) for a batch; grad == nullptr
// (cost only) when g / H are null.  g: [P][n], H: [P][n*n], cost: [P] (= ||r||^2), all host.
template <typename Scalar, typename Cost>
void Accumulate(const Cost& cost, const std::vector<Scalar>& x, std::vector<Scalar>* g, std::vector<Scalar>* H,
                std::vector<double>& cost_out) {
  const int64_t P = cost.P();
  const int n = cost.n();
  const Context& ctx = cost.ctx();
  DeviceBuffer<Scalar> dx(ctx, x.size());
  dx.upload(x.data());
  DeviceBuffer<double> dc(ctx, P);
  const bool want = g && H;
  DeviceBuffer<Scalar> dg, dH;
  if (want) { dg = DeviceBuffer<Scalar>(ctx, size_t(P) * n); dH = DeviceBuffer<Scalar>(ctx, size_t(P) * n * n); }
  apply_loss(cost);
  bool done = false;
  if constexpr (detail::is_jit<Cost>::value) {
    if (cost.has_shared()) {   // a model with a shared item table: the table beside the batch; bounds and prior, each or NULL
      const toa_shared sh = cost.shared_pod();
      const toa_bounds bd = cost.has_bounds() ? cost.bounds_pod() : toa_bounds{};
      const toa_prior pr = cost.has_prior() ? cost.prior_pod() : toa_prior{};
      check(toa_jit_accumulate_shared(ctx.get(), cost.jit_handle(), cost.items(), P, cost.data(), &sh, dx.data(), cost.has_bounds() ? &bd : nullptr,
                                      cost.has_prior() ? &pr : nullptr, want ? 1 : 0, want ? dg.data() : nullptr, want ? dH.data() : nullptr, dc.data(),
                                      nullptr));
      done = true;
    }
  }
  if (!done)
    check(toa_accumulate(ctx.get(), Cost::model_id, dtype_of<Scalar>(), n, cost.m(), P, cost.data(), dx.data(), want ? 1 : 0,
                         want ? dg.data() : nullptr, want ? dH.data() : nullptr, dc.data(), nullptr));
  check(toa_synchronize(ctx.get()));
  cost_out.resize(P);
  dc.download(cost_out.data());
  if (want) { g->resize(size_t(P) * n); dg.download(g->data()); H->resize(size_t(P) * n * n); dH.download(H->data()); }
}

// losses::Huber(n2, th2, true) & co. (losses/robust_norms.h:32-316) for an array of squared norms: kind = TOA_LOSS_*.
template <typename Scalar>
void RobustNorm(const Context& ctx, int kind, const std::vector<Scalar>& n2, Scalar th2, std::vector<Scalar>& loss,
                std::vector<Scalar>& scale) {
  DeviceBuffer<Scalar> dn(ctx, n2.size()), dl(ctx, n2.size()), ds(ctx, n2.size());
  dn.upload(n2.data());
  check(toa_robust_norm(ctx.get(), kind, dtype_of<Scalar>(), int64_t(n2.size()), dn.data(), double(th2), dl.data(), ds.data()));
  check(toa_synchronize(ctx.get()));
  loss.resize(n2.size());
  scale.resize(n2.size());
  dl.download(loss.data());
  ds.download(scale.data());
}

// tinyopt::InvCov (include/tinyopt/math.h:41-91) for a batch of n x n matrices; ok[p] == 0 <=> std::nullopt.
template <typename Scalar>
void InvCov(const Context& ctx, int64_t P, int n, const std::vector<Scalar>& H, std::vector<Scalar>& C, std::vector<int32_t>& ok) {
  DeviceBuffer<Scalar> dH(ctx, H.size()), dC(ctx, H.size());
  DeviceBuffer<int32_t> dok(ctx, P);
  dH.upload(H.data());
  check(toa_inv_cov(ctx.get(), dtype_of<Scalar>(), n, P, dH.data(), dC.data(), dok.data()));
  check(toa_synchronize(ctx.get()));
  C.resize(H.size());
  dC.download(C.data());
  ok.resize(P);
  dok.download(ok.data());
}

}  // namespace tinyopt_amd
