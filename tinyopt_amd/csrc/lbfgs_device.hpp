// Limited-memory BFGS on a scalar cost with a backtracking (Armijo) line search, executed wave-uniformly.
//
// Not a restatement of the reference (its roadmap only names the solver): the state machine is defined in DESIGN section 19
// and restated in numpy by tests/lbfgs_reference.py.  It shares the LDS-resident record of the LM state machine (LmState /
// WaveLds, lm_device.hpp), the results row of the first-order path (gd_finalize, gd_device.hpp) and the reference's stop tests
// in the reference's order (optimizer.h:519-534) on the normalised cost.  What it keeps in the carve:
//   L.xs   the TRIAL point — what the model's pass reads            L.xsv  x_acc, the last accepted point
//   L.g    the gradient of the last pass                            L.hd   g_acc, the gradient at x_acc
//   L.dx   d, the search direction at x_acc
// and behind the carve, in the wave's own LDS (LbfgsRing): the last M pairs (s, y) with rho = 1 / s.y, the two-loop recursion's
// alphas and the scalars of the line search.  Lane j owns component j of every vector; every dot product is a
// wave_allreduce_sum in T (a fixed butterfly: the same bits on every wave); the Armijo comparison is in double.
// Nothing here is a register array: the ring slot and the loop over the pairs index LDS.
//
// A `Model` supplies
//   accumulate(L, n, lane, cost)   g = sum_i grad c_i into L.g[0..n), cost = sum_i c_i (wave-uniform)
#pragma once
#include "gd_device.hpp"

namespace toa {

// the scalars of one problem's line search
template <typename T>
struct LbfgsVars {
  T f_acc;     // the raw (not normalised) cost at x_acc
  T gd;        // g_acc . d
  T alpha;     // the step length of the current trial
  T gamma;     // s.y / y.y of the newest pair: the initial Hessian of the two-loop recursion
  int first;   // no point accepted yet
  int count;   // pairs in the ring
  int head;    // the slot the next pair goes to
  int pad;
};

// The wave's ring behind its carve: [M][2][stride] scalars (pair i: s at 2 i stride, y behind it), rho[M], a[M], the scalars.
template <typename T>
struct LbfgsRing {
  T* pairs;
  T* rho;
  T* a;
  LbfgsVars<T>* v;
  int M, stride;
  static __host__ __device__ int stride_for(int n) { return (n + 3) & ~3; }
  static __host__ __device__ size_t bytes(int M, int n) {
    size_t b = size_t(M) * (2 * size_t(stride_for(n)) + 2) * sizeof(T);
    b = (b + 15) & ~size_t(15);
    return b + ((sizeof(LbfgsVars<T>) + 15) & ~size_t(15));
  }
  __device__ static LbfgsRing carve(char* base, int M, int n) {
    LbfgsRing r;
    r.M = M;
    r.stride = stride_for(n);
    r.pairs = reinterpret_cast<T*>(base);
    r.rho = r.pairs + size_t(M) * 2 * r.stride;
    r.a = r.rho + M;
    const size_t off = (size_t(M) * (2 * size_t(r.stride) + 2) * sizeof(T) + 15) & ~size_t(15);
    r.v = reinterpret_cast<LbfgsVars<T>*>(base + off);
    return r;
  }
  __device__ __forceinline__ T* s(int slot) const { return pairs + size_t(slot) * 2 * stride; }
  __device__ __forceinline__ T* y(int slot) const { return pairs + size_t(slot) * 2 * stride + stride; }
};

template <typename T>
__device__ __forceinline__ bool lbfgs_finite(T v) { return !(isnan(v) || isinf(v)); }

// d = -H g_acc by the two-loop recursion (Nocedal & Wright, algorithm 7.4) over the ring, H0 = gamma I; falls back to the
// scaled steepest descent -g_acc / max(1, |g_acc|) (and empties the ring) when there is no pair or d is no descent direction.
// Leaves d in L.dx and g_acc . d in the scalars.
template <typename T>
__device__ __forceinline__ void lbfgs_direction(WaveLds<T>& L, const LbfgsRing<T>& R, const int n, const int lane) {
  LbfgsVars<T>& V = *R.v;
  const bool in_n = lane < n;
  const T gl = in_n ? L.hd[lane] : T(0);
  T d = T(0), gd = T(0);
  const int count = V.count;
  if (count > 0) {
    T q = gl;
    int slot = V.head;
    for (int k = 0; k < count; ++k) {   // newest to oldest
      slot = slot == 0 ? R.M - 1 : slot - 1;
      const T sl = in_n ? R.s(slot)[lane] : T(0);
      const T yl = in_n ? R.y(slot)[lane] : T(0);
      const T a = R.rho[slot] * wave_allreduce_sum(sl * q);
      q = q - a * yl;
      if (lane == 0) R.a[slot] = a;
    }
    wave_sync();
    T r = V.gamma * q;
    for (int k = 0; k < count; ++k) {   // oldest to newest
      const T sl = in_n ? R.s(slot)[lane] : T(0);
      const T yl = in_n ? R.y(slot)[lane] : T(0);
      const T b = R.rho[slot] * wave_allreduce_sum(yl * r);
      r = r + sl * (R.a[slot] - b);
      slot = slot + 1 == R.M ? 0 : slot + 1;
    }
    d = -r;
    gd = wave_allreduce_sum(gl * d);
  }
  if (count == 0 || !(gd < T(0)) || !lbfgs_finite(gd)) {
    V.count = 0;
    V.head = 0;
    const T nrm = sqrt(wave_allreduce_sum(gl * gl));
    d = -gl / fmax(T(1), nrm);
    gd = wave_allreduce_sum(gl * d);
  }
  L.dx[lane] = in_n ? d : T(0);
  V.gd = gd;
  wave_sync();
}

// One pass and what follows it.  Returns false when the problem has stopped (S.stop set) or the iterations are used up.
template <typename T, typename Model>
__device__ __forceinline__ bool lbfgs_iteration(Model& model, WaveLds<T>& L, const LbfgsRing<T>& R, const int n, const int lane, const long long p,
                                                const float c1, const float shrink) {
  LmState<T>& S = *L.st;
  LbfgsVars<T>& V = *R.v;
  const toa_options& opt = *L.opt;
  const toa_results& res = *L.res;
  const bool in_n = lane < n;
  T c;
  reg_fence();
  model.accumulate(L, n, lane, c);
  reg_fence();
  S.acc_passes++;
  const T gl = in_n ? L.g[lane] : T(0);
  if (!lbfgs_finite(c) || __any(!lbfgs_finite(gl))) { S.stop = TOA_STOP_NAN_OR_INF; return false; }
  const bool first = V.first != 0;
  const bool accepted = first || double(c) <= double(V.f_acc) + double(c1) * double(V.alpha) * double(V.gd);
  const double err = normalize_cost(double(c), 1, opt);
  const T sl = in_n ? L.xs[lane] - L.xsv[lane] : T(0);   // trial - x_acc
  const double step2 = first ? 0.0 : double(wave_allreduce_sum(sl * sl));
  const int hs = res.hist_stride;
  if (lane == 0 && S.num_iters < hs) {
    if (res.errs) res.errs[p * hs + S.num_iters] = err;
    if (res.deltas2) res.deltas2[p * hs + S.num_iters] = step2;
    if (res.successes) res.successes[p * hs + S.num_iters] = accepted ? 1 : 0;
  }
  S.num_iters = S.num_iters + 1;
  S.iter = S.iter + 1;
  if (accepted) {
    if (!first) {
      const T yl = in_n ? gl - L.hd[lane] : T(0);
      const T sy = wave_allreduce_sum(sl * yl);
      const T rho = T(1) / sy;
      if (sy > T(0) && lbfgs_finite(rho)) {   // the newest pair into the ring (the oldest falls out beyond M)
        const T yy = wave_allreduce_sum(yl * yl);
        const int slot = V.head;
        if (in_n) { R.s(slot)[lane] = sl; R.y(slot)[lane] = yl; }
        if (lane == 0) R.rho[slot] = rho;
        V.gamma = sy / yy;
        V.head = slot + 1 == R.M ? 0 : slot + 1;
        V.count = V.count < R.M ? V.count + 1 : R.M;
      }
    }
    const double prev = S.final_cost;
    const double rel = (prev > double(float_epsilon<T>()) && prev < double(NumLimits<T>::max())) ? (prev - err) / prev : 0.0;
    L.xsv[lane] = L.xs[lane];
    L.hd[lane] = gl;
    V.f_acc = c;
    V.first = 0;
    S.num_consec = 0;
    S.final_cost = err;
    S.final_rerr = rel;
    wave_sync();
    // optimizer.h:519-534, the tests that apply to an accepted point
    if (opt.min_error > 0 && err < double(opt.min_error)) S.stop = TOA_STOP_MIN_ERROR;
    else if (!first && opt.min_rerr_dec > 0 && rel > 0.0 && rel < double(opt.min_rerr_dec)) S.stop = TOA_STOP_MIN_REL_ERROR;
    else if (opt.min_grad_norm2 > 0 && double(wave_allreduce_sum(gl * gl)) < double(opt.min_grad_norm2)) S.stop = TOA_STOP_MIN_GRAD_NORM;
    if (S.stop != TOA_STOP_NONE) return false;
    lbfgs_direction<T>(L, R, n, lane);
    V.alpha = T(1);
  } else {
    S.num_consec = S.num_consec + 1;
    S.num_failures = S.num_failures + 1;
    // the round-off floor: a rejected trial whose cost is the accepted one to min_rerr_dec cannot be improved by a shorter step
    if (fabs(double(c) - double(V.f_acc)) < double(opt.min_rerr_dec) * fabs(double(V.f_acc))) { S.stop = TOA_STOP_MIN_REL_ERROR; return false; }
    if (opt.max_consec_failures > 0 && S.num_consec >= unsigned(opt.max_consec_failures)) { S.stop = TOA_STOP_MAX_CONSEC_NO_DECR; return false; }
    if (opt.max_total_failures > 0 && S.num_failures >= unsigned(opt.max_total_failures)) { S.stop = TOA_STOP_MAX_NO_DECR; return false; }
    V.alpha = V.alpha * T(shrink);
  }
  const T step = in_n ? V.alpha * L.dx[lane] : T(0);
  if (double(wave_allreduce_sum(step * step)) < double(opt.min_step_norm2)) { S.stop = TOA_STOP_MIN_DELTA_NORM; return false; }
  wave_sync();
  L.xs[lane] = L.xsv[lane] + step;
  wave_sync();
  return S.iter < S.max_iters;
}

// Runs one problem to its StopReason.  On entry L.xs[] holds x0 (lanes >= n: 0), on exit x_acc: never a rejected trial.
template <typename T, typename Model>
__device__ __forceinline__ void lbfgs_solve_problem(Model& model, WaveLds<T>& L, const LbfgsRing<T>& R, const int n, const int lane, const long long p,
                                                    const float c1, const float shrink) {
  lm_init<T>(L, lane);
  LmState<T>& S = *L.st;
  LbfgsVars<T>& V = *R.v;
  S.max_iters = L.opt->max_iters + 1;   // (check_final_cost has nothing to do: x is always an accepted point)
  S.final_nres = 1;
  S.final_ninl = 1;
  // the ring and the line search start empty for EVERY problem: a wave that pops a second one sees nothing of the first
  V.f_acc = T(0); V.gd = T(0); V.alpha = T(1); V.gamma = T(1);
  V.first = 1; V.count = 0; V.head = 0;
  L.xsv[lane] = L.xs[lane];
  L.hd[lane] = T(0);
  wave_sync();
  while (lbfgs_iteration<T>(model, L, R, n, lane, p, c1, shrink)) {}
  wave_sync();
  L.xs[lane] = L.xsv[lane];
  wave_sync();
  gd_finalize<T>(L, p, lane);
}

}  // namespace toa
