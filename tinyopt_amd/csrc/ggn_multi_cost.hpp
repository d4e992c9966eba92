// Multi-output second-order scalar costs (TOA_JIT_COST_GGN_MULTI): a scalar cost summed over items,
// c_i = phi(u_i(x)) with a VECTOR inner function u_i of K outputs, 1 <= K <= 8 — multinomial / softmax regression (K logits), a
// Gaussian likelihood with mean and log-variance predictors, any multi-output GLM — run by LM / GN on the matrix-core Gram of the
// row models.  The item's Hessian is taken as H_i = J^T Hs J with J = du/dx (K x n) and Hs = d2phi/du2 (K x K): the generalised
// Gauss-Newton Hessian (the sum_k dphi/du_k hess u_k term is dropped), exact where u is linear in x.
//
// The body (csrc/jit.hip: UserFunctor::eval_ggn_multi) assigns `c`, the item's cost term, and inside `if (want_grad)`
//   gs[k] = dc/du_k for k < K,   Hs[k][l] for l <= k (the LOWER triangle; the upper one is never read),   J[k][a] = du_k/dx_a
// for every k < K, a < n (ASSIGNED, not added).  The item adds g += sum_k gs_k J_k and H += J^T Hs J.
//
// The row trick of ggn_cost.hpp with K rows per item: once Hs = L D L^T is factored, J^T Hs J is a Gram of K scaled rows.  THE
// RULE, per item, in the lane, in the problem's scalar type, every operation rounded on its own (no contraction), sums in
// ascending q / i from the first term:
//   for j = 0 .. K-1:
//     d_j = Hs_jj - sum_{q<j} L_jq * (L_jq * e_q)
//     d_j >  wmin:  w_j = d_j,  e_j = d_j,  L_ij = (Hs_ij - sum_{q<j} L_iq * (L_jq * e_q)) / d_j   for i > j
//     d_j <= wmin:  w_j = wmin, e_j = 0,    L_ij = 0                                               for i > j
//     (a NaN compares false: it counts as `>` and stays, as hs does in ggn_cost.hpp)
//   y_j = gs_j - sum_{q<j} L_jq * y_q                              (forward substitution, y = L^-1 gs)
//   row j of [J | r] = [ sqrt(w_j) * (J_j + sum_{i>j} L_ij * J_i) | y_j / sqrt(w_j) ]
// wmin = GgnWmin<T> (2^-60 / 2^-200).  The Gram's (J, J) block is then J^T L W L^T J: J^T Hs J for a positive definite Hs, with
// non-positive pivots clamped, so H stays positive semi-definite — a Gauss-Newton door, NOT one for indefinite curvature.  Its
// (J, r) column is J^T L L^-1 gs = J^T gs whatever was clamped.  The (r, r) entry means nothing and is not read: the cost is the
// wave's sum of the items' c, ONE residual, through RowModel's item-cost extension point (no memo), as in ggn_cost.hpp.
// With K = 1 the rule is GgnRowFunctor's code operation for operation: w = hs clamped, the row [sqrt(w) J | gs / sqrt(w)].
//
// A singular parametrisation (all K logits of a softmax: Hs has the null vector 1) is legal but ill-conditioned — its last pivot
// is rounding noise around 0; a reference class (K - 1 free logits) is the form to use.
//
// 1 <= n <= 63, 1 <= K <= 8, fp32 and fp64, Euclidean parameters; a super-step holds 64 / K items.  The lane holds J as K n
// scalars: wide K x wide n spills (toa_jit_model_stats: scratch_bytes; DESIGN section 22 has the table).  Loops over k, l, a in
// the body need COMPILE-TIME bounds.
#pragma once
#include "ggn_cost.hpp"

namespace toa {

// The rule above, in place: gs -> y, the lower triangle of Hs -> L, J -> the scaled rows, r the rows' last column.
template <typename T, int K, int N>
__device__ __forceinline__ void ggn_multi_rows(T* gs, T (*Hs)[K], T (*J)[N], T* r) {
#pragma clang fp contract(off)
  const T wmin = GgnWmin<T>::value;
  T e[K], sq[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    T d = Hs[j][j];
#pragma unroll
    for (int q = 0; q < j; ++q) d = d - Hs[j][q] * (Hs[j][q] * e[q]);
    const bool clamped = d <= wmin;   // (a NaN compares false: it stays)
    const T w = clamped ? wmin : d;
    e[j] = clamped ? T(0) : d;
    sq[j] = sqrt(w);
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      T t = Hs[i][j];
#pragma unroll
      for (int q = 0; q < j; ++q) t = t - Hs[i][q] * (Hs[j][q] * e[q]);
      Hs[i][j] = clamped ? T(0) : t / d;
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    T y = gs[j];
#pragma unroll
    for (int q = 0; q < j; ++q) y = y - Hs[j][q] * gs[q];
    gs[j] = y;
    r[j] = y / sq[j];
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {   // (ascending: row j reads the rows i > j as the body left them)
#pragma unroll
    for (int a = 0; a < N; ++a) {
      T t = J[j][a];
#pragma unroll
      for (int i = j + 1; i < K; ++i) t = t + Hs[i][j] * J[i][a];
      J[j][a] = t * sq[j];
    }
  }
}

// F (all static): kN, kK, kD, kH and
//   template <bool want_grad, class X> eval_ggn_multi(const X& x, const T* h, const T* p, T& c, T* gs, T (*Hs)[kK], T (*J)[kN])
template <typename T, typename F>
struct GgnMultiRowFunctor {
  static constexpr int kN = F::kN, kR = F::kK, kD = F::kD, kH = F::kH;
  static_assert(kR >= 1 && kR <= 8, "outputs per item");
  static constexpr bool kManual = true;
  static constexpr bool kItemCost = true;   // RowModel: eval_item below, the cost is the sum of c
  template <bool want_grad>
  static __device__ __forceinline__ void eval_item(const T* x, const T* h, const T* p, T& c, T* r, T (*J)[kN]) {
    if constexpr (want_grad) {
      T gs[kR], Hs[kR][kR];
#pragma unroll
      for (int k = 0; k < kR; ++k) {
        gs[k] = T(0);
#pragma unroll
        for (int l = 0; l < kR; ++l) Hs[k][l] = T(0);
      }
      F::template eval_ggn_multi<true>(x, h, p, c, gs, Hs, J);
      ggn_multi_rows<T, kR, kN>(gs, Hs, J, r);
    } else {
      F::template eval_ggn_multi<false>(x, h, p, c, static_cast<T*>(nullptr), static_cast<T(*)[kR]>(nullptr), static_cast<T(*)[kN]>(nullptr));
#pragma unroll
      for (int k = 0; k < kR; ++k) r[k] = T(0);
    }
  }
  // ... of a body with a shared item table (shared.hpp): `s` is the item's row of it, after p
  static constexpr int kS = FunctorShared<F>::value;
  template <bool want_grad>
  static __device__ __forceinline__ void eval_item(const T* x, const T* h, const T* p, const T* s, T& c, T* r, T (*J)[kN]) {
    if constexpr (want_grad) {
      T gs[kR], Hs[kR][kR];
#pragma unroll
      for (int k = 0; k < kR; ++k) {
        gs[k] = T(0);
#pragma unroll
        for (int l = 0; l < kR; ++l) Hs[k][l] = T(0);
      }
      F::template eval_ggn_multi<true>(x, h, p, s, c, gs, Hs, J);
      ggn_multi_rows<T, kR, kN>(gs, Hs, J, r);
    } else {
      F::template eval_ggn_multi<false>(x, h, p, s, c, static_cast<T*>(nullptr), static_cast<T(*)[kR]>(nullptr), static_cast<T(*)[kN]>(nullptr));
#pragma unroll
      for (int k = 0; k < kR; ++k) r[k] = T(0);
    }
  }
};

// The Accumulate seam is ggn_accumulate_kernel (ggn_cost.hpp), which takes a prior (TOA_PRIOR) and a shared table (TOA_SHARED).

}  // namespace toa
