// Numerical differentiation of run-time functors: the reference's diff/num_diff.h (NumEval, EstimateNumJac, CreateNumDiffFunc1 / 2
// with Method::{kForward, kCentral, kFastCentral}) as two wrappers around a user functor that is only ever instantiated on plain T —
// so a body that is not generic over its scalar type runs at all (tests/diff.cpp:113-132), and a hand-written Jacobian or gradient
// can be compared against differences of its own residuals (diff/gradient_check.h; csrc/jit.hip toa_jit_check_gradient).
//
//   NumRowFunctor<T, F, METHOD, HS>   presents to RowModel what AdRowFunctor presents (kManual, kComputeBound, kIndexedOperands,
//                                     eval_manual<want_grad>): r at x, then column a of J from F at perturbed parameters —
//                                     NumEval's loop (num_diff.h:93-124), one lane per item.
//   NumCostFunctor<T, F, METHOD, HS>  presents CostModel's kCostKind = 3 interface (eval_grad<want_grad>): G[a] += the same
//                                     differences of the item's cost term c.
//
//   METHOD (TOA_DIFF_NUM_*)   points                                                      column a
//   1 forward                 x + h e_a                                                   (r+ - r) / h
//   2 central                 x + h e_a and x - h e_a, each formed from x                  (r+ - r-) / (2 h)
//   3 fast central            y = x + h e_a, then y + (-2 h) e_a formed from y             (r+ - r-) / (2 h)
//
// HS is a type whose `static constexpr double value` is the step: h and the method are compile-time constants of the generated
// source (which keys the code object cache).
//
// How the columns are formed.  The perturbed parameters are an ACCESSOR, x[j] -> xs[j] + (j == a ? d : 0): no perturbed copy of x
// per lane; a is wave-uniform, so for a uniform j the compare and the select of the two constants are scalar-unit work.  The
// body is NOT instantiated 2 n times (126 inlined copies of user code at n = 63): the columns are walked in chunks of at most
// TOA_AD_CW (twelve), as AdRowFunctor walks its Jets — the chunk is a compile-time constant, the column inside it a RUNNING index (two or
// three copies of the body per chunk).  A register array indexed by that running index would be scratch memory,
// so the column's value is put into its place by a chain of selects over the chunk's (compile-time) positions: <= TOA_AD_CW per column.
//
// So a body behind these wrappers sees x as that accessor, never as a const T*: it may read the parameters only as x[j].  A residual or
// cost body is generic over the accessor anyway; an accumulate / cost_grad body that takes x as a pointer runs as a model and fails
// to build as a checker's twin (jit.hip twin_for reports it with the compiler's log).
//
// The generated functor of a numeric model is compiled with `#pragma clang fp contract(off)` (jit.hip): a difference quotient
// magnifies the last place of its two values by 1 / (2 h), so the body rounds every product and sum on its own, as the reference's
// CPU build does.
//
// Scalar costs: the differences are taken PER ITEM, before the sum over the items.  The reference differences the summed cost
// (CreateNumDiffFunc1 on a Cost); in fp32 over thousands of items that sum has no digits left for a difference of size h * |grad|.
// Per item the two are the same derivative (the sum of the differences is the difference of the sums in exact arithmetic).
#pragma once
#include <type_traits>
#include "wave_utils.hpp"
#include "shared.hpp"   // FunctorShared: a body with a shared item table

#ifndef TOA_AD_CW   // the chunk width of AdRowFunctor's Jets (row_model.hpp): the same columns per chunk here, under the same -DTOA_AD_CW=k
#define TOA_AD_CW 12
#endif

namespace toa {

// d if b else 0, selected as bits: a scalar-unit select when b is wave-uniform and d a constant, a v_cndmask otherwise
__device__ __forceinline__ float num_sel(bool b, float d) { return __builtin_bit_cast(float, b ? __builtin_bit_cast(int, d) : 0); }
__device__ __forceinline__ double num_sel(bool b, double d) { return __builtin_bit_cast(double, b ? __builtin_bit_cast(long long, d) : 0ll); }

// x + d e_a (PlusEq of a dx that is zero elsewhere: num_diff.h:95-98), over whatever indexes like an array
template <typename T, class X>
struct NumPerturbedX {
  const X& xs;
  int a;
  T d;
  __device__ __forceinline__ T operator[](int j) const { return xs[j] + num_sel(j == a, d); }
};
// (x + d1 e_a) + d2 e_a: the second point of kFastCentral, formed from the first (num_diff.h:110-113)
template <typename T, class X>
struct NumPerturbedX2 {
  const X& xs;
  int a;
  T d1, d2;
  __device__ __forceinline__ T operator[](int j) const { return (xs[j] + num_sel(j == a, d1)) + num_sel(j == a, d2); }
};

// what kind of body F is (this header serves kernels.hpp and gd_kernels.hpp alike: its own traits)
template <typename F, typename = void>
struct NumFunctorManual { static constexpr bool value = false; };
template <typename F>
struct NumFunctorManual<F, std::enable_if_t<F::kManual>> { static constexpr bool value = true; };
template <typename F, typename = void>
struct NumFunctorCostKind { static constexpr int value = 0; };
template <typename F>
struct NumFunctorCostKind<F, std::enable_if_t<(F::kCostKind > 0)>> { static constexpr int value = F::kCostKind; };

// Column `a` of the finite differences of `ev(x accessor, out[NR])`: NumEval's loop body.  r0 = ev at x (forward differences only).
template <typename T, int METHOD, int NR, class X, class Ev>
__device__ __forceinline__ void num_diff_column(const X& x, const int a, const T hh, const T (&r0)[NR], T (&dq)[NR], Ev&& ev) {
  static_assert(METHOD >= 1 && METHOD <= 3, "TOA_DIFF_NUM_FORWARD / CENTRAL / FAST_CENTRAL");
  T rp[NR], rm[NR];
  ev(NumPerturbedX<T, X>{x, a, hh}, rp);
  if constexpr (METHOD == 1) {
#pragma unroll
    for (int q = 0; q < NR; ++q) dq[q] = (rp[q] - r0[q]) / hh;
  } else {
    if constexpr (METHOD == 2) ev(NumPerturbedX<T, X>{x, a, -hh}, rm);
    else ev(NumPerturbedX2<T, X>{x, a, hh, T(-2) * hh}, rm);
#pragma unroll
    for (int q = 0; q < NR; ++q) dq[q] = (rp[q] - rm[q]) / (T(2) * hh);
  }
}

template <typename T, typename F, int METHOD, typename HS>
struct NumRowFunctor {
  static constexpr int kN = F::kN, kR = F::kR, kD = F::kD, kH = F::kH;
  static constexpr bool kManual = true;
  static constexpr bool kComputeBound = true;      // (RowModel: one LDS region, every lane an item — the 2 n + 1 evaluations are the bound)
  static constexpr bool kIndexedOperands = true;   // x[j] / p[j] with a running j: straight from LDS
  static constexpr int kChunks = (kN + TOA_AD_CW - 1) / TOA_AD_CW;   // columns in chunks of <= TOA_AD_CW (12; AdRowFunctor's width, and its A/B flag), as balanced as kN allows
  static constexpr int kCW = (kN + kChunks - 1) / kChunks;
  // F's cost-only evaluation: F::eval<T> of a residual body, F::eval_manual<false> of an accumulate body (the checker's twin)
  template <class X>
  static __device__ __forceinline__ void rows(const X& x, const T* hd, const T* p, T* r) {
    if constexpr (NumFunctorManual<F>::value) F::template eval_manual<false>(x, hd, p, r, static_cast<T(*)[kN]>(nullptr));
    else F::template eval<T>(x, hd, p, r);
  }
  template <bool want_grad>
  static __device__ __forceinline__ void eval_manual(const T* x, const T* hd, const T* p, T* r, T (*J)[kN]) {
    T r0[kR];
    rows(x, hd, p, r0);
#pragma unroll
    for (int q = 0; q < kR; ++q) r[q] = r0[q];
    if constexpr (want_grad) {
      const T hh = T(HS::value);
      static_for<kChunks>([&](auto cc) __attribute__((always_inline)) {
        constexpr int c0 = decltype(cc)::value * kCW;
        constexpr int cw = kN - c0 < kCW ? kN - c0 : kCW;
#pragma unroll
        for (int q = 0; q < kR; ++q) {
#pragma unroll
          for (int t = 0; t < cw; ++t) J[q][c0 + t] = T(0);
        }
#pragma unroll 1
        for (int s = 0; s < cw; ++s) {
          T dq[kR];
          num_diff_column<T, METHOD>(x, c0 + s, hh, r0, dq, [&](const auto& xa, T (&out)[kR]) __attribute__((always_inline)) { rows(xa, hd, p, out); });
#pragma unroll
          for (int q = 0; q < kR; ++q) {
#pragma unroll
            for (int t = 0; t < cw; ++t) J[q][c0 + t] = (t == s) ? dq[q] : J[q][c0 + t];   // (J[q][c0 + s] with the running s would be scratch memory)
          }
        }
      });
    }
  }
  // ... of a body with a shared item table (shared.hpp): `sh` is the item's row of it, after p — data, not
  // perturbed.  Residual bodies only (a numeric MODEL never wraps an accumulate body, and such a model has no checker's twin).
  static constexpr int kS = FunctorShared<F>::value;
  template <bool want_grad>
  static __device__ __forceinline__ void eval_manual(const T* x, const T* hd, const T* p, const T* sh, T* r, T (*J)[kN]) {
    T r0[kR];
    F::template eval<T>(x, hd, p, sh, r0);
#pragma unroll
    for (int q = 0; q < kR; ++q) r[q] = r0[q];
    if constexpr (want_grad) {
      const T hh = T(HS::value);
      static_for<kChunks>([&](auto cc) __attribute__((always_inline)) {
        constexpr int c0 = decltype(cc)::value * kCW;
        constexpr int cw = kN - c0 < kCW ? kN - c0 : kCW;
#pragma unroll
        for (int q = 0; q < kR; ++q) {
#pragma unroll
          for (int t = 0; t < cw; ++t) J[q][c0 + t] = T(0);
        }
#pragma unroll 1
        for (int s = 0; s < cw; ++s) {
          T dq[kR];
          num_diff_column<T, METHOD>(x, c0 + s, hh, r0, dq,
                                     [&](const auto& xa, T (&out)[kR]) __attribute__((always_inline)) { F::template eval<T>(xa, hd, p, sh, out); });
#pragma unroll
          for (int q = 0; q < kR; ++q) {
#pragma unroll
            for (int t = 0; t < cw; ++t) J[q][c0 + t] = (t == s) ? dq[q] : J[q][c0 + t];
          }
        }
      });
    }
  }
};

template <typename T, typename F, int METHOD, typename HS>
struct NumCostFunctor {
  static constexpr int kN = F::kN, kD = F::kD, kH = F::kH;
  static constexpr int kCostKind = 3;
  static constexpr int kChunks = (kN + TOA_AD_CW - 1) / TOA_AD_CW;
  static constexpr int kCW = (kN + kChunks - 1) / kChunks;
  // F's cost-only evaluation: F::eval<T> (TOA_JIT_COST), F::eval_grad<false> (TOA_JIT_COST_GRAD: the checker's twin)
  template <class X>
  static __device__ __forceinline__ void term(const X& x, const T* hd, const T* p, T& c) {
    if constexpr (NumFunctorCostKind<F>::value == 3) F::template eval_grad<false>(x, hd, p, c, static_cast<T*>(nullptr));
    else F::template eval<T>(x, hd, p, c);
  }
  template <bool want_grad, class X>
  static __device__ __forceinline__ void eval_grad(const X& x, const T* hd, const T* p, T& c, T* G) {
    T c0[1];
    term(x, hd, p, c0[0]);
    c = c0[0];
    if constexpr (want_grad) {
      const T hh = T(HS::value);
      static_for<kChunks>([&](auto cc) __attribute__((always_inline)) {
        constexpr int c0i = decltype(cc)::value * kCW;
        constexpr int cw = kN - c0i < kCW ? kN - c0i : kCW;
#pragma unroll 1
        for (int s = 0; s < cw; ++s) {
          T dq[1];
          num_diff_column<T, METHOD>(x, c0i + s, hh, c0, dq, [&](const auto& xa, T (&out)[1]) __attribute__((always_inline)) { term(xa, hd, p, out[0]); });
#pragma unroll
          for (int t = 0; t < cw; ++t) G[c0i + t] = (t == s) ? G[c0i + t] + dq[0] : G[c0i + t];
        }
      });
    }
  }
};

// toa_jit_check_gradient's comparison: a wavefront per problem, max |a - b| over g [P][n] and (n_H = n) over H [P][n][n] in T —
// (grad_num - grad).cwiseAbs().maxCoeff() and (H_num - H).cwiseAbs().maxCoeff(), gradient_check.h:97,206 — and ok = both < eps.
// A difference that is not a number makes its distance NaN and ok = 0.  n_H = 0: the H distance is 0 and ignored.
template <typename T>
__global__ void __launch_bounds__(256) check_gradient_kernel(const T* __restrict__ ga, const T* __restrict__ gb, const T* __restrict__ Ha,
                                                             const T* __restrict__ Hb, long long P, int n, int n_H, double eps,
                                                             double* __restrict__ max_dist, int* __restrict__ ok) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long p = (long long)blockIdx.x * 4 + wave; p < P; p += (long long)gridDim.x * 4) {
    T dg = T(0), dh = T(0);
    int bad_g = 0, bad_h = 0;
    for (int e = lane; e < n; e += 64) {
      T d = ga[size_t(p) * n + e] - gb[size_t(p) * n + e];
      d = d < T(0) ? -d : d;
      bad_g |= !(d == d);
      dg = d > dg ? d : dg;
    }
    const size_t nn = size_t(n_H) * n_H;
    for (size_t e = lane; e < nn; e += 64) {
      T d = Ha[size_t(p) * nn + e] - Hb[size_t(p) * nn + e];
      d = d < T(0) ? -d : d;
      bad_h |= !(d == d);
      dh = d > dh ? d : dh;
    }
    dg = wave_allreduce_max(dg);
    dh = wave_allreduce_max(dh);
    bad_g = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_ballot_w64(bad_g != 0) != 0ull);
    bad_h = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_ballot_w64(bad_h != 0) != 0ull);
    if (lane == 0) {
      const double xg = bad_g ? __builtin_nan("") : double(dg), xh = bad_h ? __builtin_nan("") : double(dh);
      if (max_dist) { max_dist[2 * p] = xg; max_dist[2 * p + 1] = xh; }
      if (ok) ok[p] = (xg < eps && (n_H == 0 || xh < eps)) ? 1 : 0;
    }
  }
}

}  // namespace toa
