// Rank-one second-order scalar costs (TOA_JIT_COST_GGN): a scalar cost summed over items, c_i = phi(u_i(x))
// with a SCALAR inner function u_i — logistic and Poisson regression, any GLM, any likelihood of a scalar predictor — run by
// LM / GN on the matrix-core Gram of the row models.  The item's Hessian is taken as H_i = phi''(u) grad u grad u^T: the
// phi'(u) hess u term is dropped, the generalised Gauss-Newton Hessian, exact where u is linear in x.
//
// The body (csrc/jit.hip: UserFunctor::eval_ggn) assigns `c`, the item's cost term, and inside `if (want_grad)` three things:
// `gs` = dc/du, `hs` = the curvature weight, and J[a] = (grad u)[a] for every a < n (ASSIGNED, not added).  The item adds
//   g += gs J        H += w J J^T,       w = hs where hs > wmin, wmin where hs <= wmin, NaN where hs is NaN,
// wmin = 2^-60 in fp32 and 2^-200 in fp64 (powers of four: their roots 2^-30 / 2^-100 are exact, and so is scaling by them).
// A negative or zero curvature therefore contributes its gradient and, up to wmin, nothing to H: H stays positive
// semi-definite.  This is a Gauss-Newton door, NOT a door for indefinite Hessians — TOA_JIT_COST_HESS (hess_cost.hpp) is that.
//
// The row trick: a sum of weighted outer products is a Gram of scaled rows.  With sq = sqrt(w) the lane writes the row
// [sq J | gs / sq] into RowModel's [J | r] image; the Gram's (J, J) block is then sum w J J^T = H and its (J, r) column is
// sum (sq J)(gs / sq) = sum gs J = g, delivered by DenseRowGram::extract_g_diag_cost as for every row model.  The Gram's (r, r)
// entry, sum gs^2 / w, means nothing (and may overflow in fp32): RowModel's item-cost extension point (row_model.hpp
// FunctorItemCost) keeps it out of the cost — the problem's cost is the wave's sum of the items' c, ONE residual, on the
// accumulate pass and on the cost-only pass alike — and the model keeps no memo of the last accepted linearisation (its cost is
// no Gram entry; a rejected step streams the rows again).  Everything behind the model is lm_device.hpp as it stands.
// A non-finite c, gs, hs or J reaches the cost, g or H's diagonal and ends the problem like a NaN in any system.
//
// 1 <= n <= 63 in fp32 and fp64 on this ONE route (RowModel at every n, as the numeric models), one cost term per item,
// Euclidean parameters.  Loops over a in the body need COMPILE-TIME bounds: J is the lane's row in registers, and a row indexed
// by a loop that is not unrolled lands in scratch memory (toa_jit_model_stats: scratch_bytes).
#pragma once
#include "kernels.hpp"

namespace toa {

template <typename T>
struct GgnWmin;
template <>
struct GgnWmin<float> { static constexpr float value = 0x1p-60f; };
template <>
struct GgnWmin<double> { static constexpr double value = 0x1p-200; };

// F (all static): kN, kD, kH and
//   template <bool want_grad, class X> eval_ggn(const X& x, const T* h, const T* p, T& c, T& gs, T& hs, T* J)
template <typename T, typename F>
struct GgnRowFunctor {
  static constexpr int kN = F::kN, kR = 1, kD = F::kD, kH = F::kH;
  static constexpr bool kManual = true;
  static constexpr bool kItemCost = true;   // RowModel: eval_item below, the cost is the sum of c
  template <bool want_grad>
  static __device__ __forceinline__ void eval_item(const T* x, const T* h, const T* p, T& c, T* r, T (*J)[kN]) {
    T gs = T(0), hs = T(0);
    if constexpr (want_grad) {
      F::template eval_ggn<true>(x, h, p, c, gs, hs, J[0]);
      const T wmin = GgnWmin<T>::value;
      const T w = hs <= wmin ? wmin : hs;   // (a NaN compares false: it stays)
      const T sq = sqrt(w);
      r[0] = gs / sq;
#pragma unroll
      for (int a = 0; a < kN; ++a) J[0][a] *= sq;
    } else {
      F::template eval_ggn<false>(x, h, p, c, gs, hs, static_cast<T*>(nullptr));
      r[0] = T(0);
    }
  }
  // ... of a body with a shared item table (shared.hpp): `s` is the item's row of it, after p
  static constexpr int kS = FunctorShared<F>::value;
  template <bool want_grad>
  static __device__ __forceinline__ void eval_item(const T* x, const T* h, const T* p, const T* s, T& c, T* r, T (*J)[kN]) {
    T gs = T(0), hs = T(0);
    if constexpr (want_grad) {
      F::template eval_ggn<true>(x, h, p, s, c, gs, hs, J[0]);
      const T wmin = GgnWmin<T>::value;
      const T w = hs <= wmin ? wmin : hs;   // (a NaN compares false: it stays)
      const T sq = sqrt(w);
      r[0] = gs / sq;
#pragma unroll
      for (int a = 0; a < kN; ++a) J[0][a] *= sq;
    } else {
      F::template eval_ggn<false>(x, h, p, s, c, gs, hs, static_cast<T*>(nullptr));
      r[0] = T(0);
    }
  }
};

// The Accumulate seam (toa_jit_accumulate on a TOA_JIT_COST_GGN / TOA_JIT_COST_GGN_MULTI model): accumulate_kernel's arguments and its loop, with H_ optional —
// g [P][n], the full symmetric H [P][n][n] when H_ is not null, cost [P] = sum_i c_i, nres [P] = 1.
template <typename Model>
__global__ void __launch_bounds__(256) ggn_accumulate_kernel(const void* data_, const void* x_, long long P, int n, int m, int want_grad, void* g_,
                                                             void* H_, double* cost, int* nres, int lds_per_wave, int, double TOA_PRIOR_KARG TOA_SHARED_KARG) {
  using T = typename Model::Scalar;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* X = static_cast<const T*>(x_);
  Model model;
  model.init(n, m, data_);
#ifdef TOA_SHARED
  model.set_shared(shr);
#endif
  WaveLds<T> L = WaveLds<T>::carve(model_bind_stage(model, smem + size_t(wave) * lds_per_wave, n), n);
#ifdef TOA_PRIOR
  model.set_prior(pri, L.M, L.LD);   // (TOA_JIT_COST_GGN_MULTI only: ggn_multi_cost.hpp; PriorModel's item-cost branch, prior.hpp)
#endif
  for (long long p = (long long)blockIdx.x * 4 + wave; p < P; p += (long long)gridDim.x * 4) {
    wave_sync();
    L.xs[lane] = lane < n ? X[size_t(p) * n + lane] : T(0);
    wave_sync();
    model.bind(p);
    T c;
    int nr;
    if (want_grad) {
      model.accumulate(L, n, lane, c, nr);
      if (lane < n) static_cast<T*>(g_)[size_t(p) * n + lane] = L.g[lane];
      if (H_) {
        T* H = static_cast<T*>(H_) + size_t(p) * n * n;
        model.write_sym(H, n, n, lane);
        wave_sync();
        if (lane < n) H[lane * n + lane] = L.hd[lane];  // the (undamped) diagonal always comes from hd
      }
    } else {
      model.evaluate(L, n, lane, c, nr);
    }
    if (lane == 0) { cost[p] = double(c); if (nres) nres[p] = nr; }
  }
}

}  // namespace toa
