// First-order state machine: gradient descent on a scalar cost, executed wave-uniformly.
//
// Device restatement of Optimizer_::OptimizeAcc / Step (include/tinyopt/optimizers/optimizer.h:242-539) with SolverGD
// (include/tinyopt/solvers/gd.h).  Line references below are to those files.  It shares the LDS-resident record of the
// LM state machine (LmState / WaveLds, lm_device.hpp) and its judging code (lm_judge_step: the LM-only GoodStep / BadStep
// are no-ops there for any solver_type != 0, exactly SolverGD's inherited no-ops, base.h:52-56), so the stop tests, the
// roll-back and the failure counts are the LM path's own.  What differs:
//   * every Step calls Build (SolverGD has no `rebuild` flag; Rebuild is a no-op, base.h:56): the gradient is formed on
//     every pass, evaluate-only iterations included;
//   * the cost is ONE scalar (Cost(Scalar), cost.h:22: num_residuals = 1, so `normalize` divides by 1) and valid unless it
//     is DBL_MAX (isValid, cost.h:83 with nres = 1);
//   * Solve is dx = -lr * g (gd.h: `-options_.gd.lr * grad_`, lr a float promoted to T); it fails only on an invalid cost;
//   * no Hessian is exported (optimizer.h:313: `if constexpr (SolverType::FirstOrder == 0)`).
//
// A `Model` supplies
//   accumulate(L, n, lane, cost)   g = sum_i grad c_i into L.g[0..n), cost = sum_i c_i (wave-uniform)
#pragma once
#include "lm_device.hpp"

namespace toa {

// Build (gd.h Build / Accumulate) + Solve with the retry loop of Step (optimizer.h:354-399).  Returns 0 = got a step (in
// L.dx), 1 = solver failed for good (stop may or may not be set), 2 = early return with stop set.
template <typename T, typename Model>
__device__ __forceinline__ int gd_build_and_solve(Model& model, WaveLds<T>& L, const int n, const int lane, const float lr) {
  LmState<T>& S = *L.st;
  const toa_options& opt = *L.opt;
  const bool in_n = lane < n;
  const unsigned max_tries = opt.max_consec_failures > 0 ? (opt.max_consec_failures > 1 ? opt.max_consec_failures : 1) : 255;
  while (S.num_consec <= max_tries) {  // :358
    T c;
    reg_fence();
    model.accumulate(L, n, lane, c);   // clear + acc(x, grad)
    reg_fence();
    S.acc_passes++;
    S.cost_val = normalize_cost(double(c), 1, opt);   // base.h:41-45 on Cost(Scalar): num_residuals = 1
    S.cost_nres = 1;
    S.cost_ninl = 1;
    if (opt.grad_clipping != 0) {  // gd.h Build: Clamp(grad_, grad_clipping), base.h:29-38
      const T mm = opt.grad_clipping;
      if (in_n) L.g[lane] = fmin(fmax(L.g[lane], -mm), mm);
    }
    if (S.cost_val != kDblMax) {   // Solve: `if (!cost().isValid()) return nullopt; return -lr * grad_`
      if (in_n) L.dx[lane] = T(-lr) * L.g[lane];
      else L.dx[lane] = T(0);
      wave_sync();
      S.solves++;
      return 0;
    }
    // :370-390
    S.num_consec = (S.num_consec + 1) & 0xff;
    S.num_failures = (S.num_failures + 1) & 0xff;
    if (isnan(S.cost_val) || isinf(S.cost_val)) { S.stop = TOA_STOP_NAN_OR_INF; return 2; }
    if (opt.max_consec_failures > 0 && S.num_consec >= unsigned(opt.max_consec_failures)) {
      if (S.final_cost < double(NumLimits<T>::max())) S.stop = TOA_STOP_MAX_CONSEC_NO_DECR;
      return 1;
    }
    // FailedStep: a no-op for SolverGD
  }
  return 1;
}

// One pass of the loop body at optimizer.h:266-310 (uses and advances S.iter).  Returns false when the loop ends.
template <typename T, typename Model>
__device__ __forceinline__ bool gd_iteration(Model& model, WaveLds<T>& L, const int n, const int lane, const long long p, const float lr) {
  LmState<T>& S = *L.st;
  int status = 0;  // bit0 good, bit1 has_dx
  const int rc = gd_build_and_solve<T>(model, L, n, lane, lr);
  if (rc == 1) S.stop = TOA_STOP_SOLVER_FAILED;  // :396-399
  if (rc == 0) status = lm_judge_step<T>(L, n, lane, p);
  wave_sync();
  const toa_options& opt = *L.opt;
  const bool in_n = lane < n;
  if (status & 1) {                 // :271-279
    if (in_n) L.xs[lane] = L.xs[lane] + L.dx[lane];   // PlusEq(x, dx), traits.h:184-190
    L.ldx[lane] = L.dx[lane];
    S.has_last_dx = 1;
    S.last_was_success = 1;
  } else {                          // :281-297
    if (S.has_last_dx) {
      if (in_n) L.xs[lane] = L.xs[lane] + (-L.ldx[lane]);   // roll back: PlusEq(x, -last_dx)
      S.has_last_dx = 0;
    } else if (status & 2) {
      if (in_n) L.xs[lane] = L.xs[lane] + L.dx[lane];
      L.ldx[lane] = L.dx[lane];
      S.has_last_dx = 1;
    }
    S.last_was_success = 0;
  }
  // (eval_only / Rebuild(!eval_only): no-ops for SolverGD, every Step builds — check_final_cost only lengthens the loop)
  (void)opt;
  S.num_iters = S.num_iters + 1;    // :307
  S.iter = S.iter + 1;
  wave_sync();
  return S.stop == TOA_STOP_NONE && S.iter < S.max_iters;   // :309 / loop bound :266
}

template <typename T>
__device__ __forceinline__ void gd_finalize(WaveLds<T>& L, const long long p, const int lane) {
  LmState<T>& S = *L.st;
  if (S.stop == TOA_STOP_NONE && S.num_iters >= S.max_iters) S.stop = TOA_STOP_MAX_ITERS;  // :320-321
  const toa_results& res = *L.res;
  // (no final Hessian: optimizer.h:313, FirstOrder — res.final_hessian is left untouched)
  if (lane == 0) {
    res.stop_reason[p] = S.stop;
    res.num_iters[p] = S.num_iters;
    res.final_cost[p] = S.final_cost;
    if (res.num_failures) res.num_failures[p] = int(S.num_failures);
    if (res.num_consec_failures) res.num_consec_failures[p] = int(S.num_consec);
    if (res.final_num_residuals) res.final_num_residuals[p] = S.final_nres;
    if (res.final_rerr_dec) res.final_rerr_dec[p] = S.final_rerr;
    if (res.final_inlier_ratio) res.final_inlier_ratio[p] = 1.0f;
  }
  S.problems++;
  wave_sync();
}

// Runs one problem to its StopReason.  On entry L.xs[] holds x0 (lanes >= n: 0), on exit the result.
template <typename T, typename Model>
__device__ __forceinline__ void gd_solve_problem(Model& model, WaveLds<T>& L, const int n, const int lane, const long long p, const float lr) {
  lm_init<T>(L, lane);   // (the LM damping fields it sets are never read on this path)
  while (gd_iteration<T>(model, L, n, lane, p, lr)) {}
  gd_finalize<T>(L, p, lane);
}

}  // namespace toa
