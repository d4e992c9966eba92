// Second-order scalar costs: HessCostModel — a scalar cost summed over items whose body fills its own gradient AND its own
// Hessian (the reference's `f(x, grad, H) -> cost`, optimize.h:26-57 secondOrderValid; tests/optimize_easy.cpp is written in this
// form), supplied as run-time text (csrc/jit.hip, TOA_JIT_COST_HESS) and run by LM / GN through lm_fused_kernel as it stands:
// the model concept of the wave path (TestFnModel, models_analytic.hpp) over CostModel's data layout (gd_kernels.hpp).
//
// The pass: item i goes to lane i mod 64; x is a register array read once per pass; every lane keeps its partial cost, its partial
// gradient G[n] and the upper triangle of its partial Hessian, n (n + 1) / 2 scalars, in registers; ONE wave_allreduce_many per pass
// folds gradient and triangle (lane-sequential sums first, then the butterfly: a fixed order).  n <= 12: 78 triangle accumulators,
// the border at which CostModel also keeps x in registers.  After the fold lane a < n keeps ROW a of the symmetric sum (n
// registers), from which write_sym forms the full image — again after a failed fast factorisation, and for final_hessian.
//
// Functor concept (all static): kN, kD, kH and
//   template <bool want_grad, class X, class Hs> eval_hess(const X& x, const T* h, const T* p, T& c, T* G, Hs& H)
// c = the item's cost term; if want_grad, the item's gradient ADDED to G[a] and its Hessian ADDED to H(a, b) for a <= b.  A write
// with a > b lands in a discarded sink, so a body that fills the full symmetric matrix gives the same system.  Loops over a, b need
// compile-time bounds: a triangle indexed by a loop that is not unrolled is scratch memory (toa_jit_model_stats shows it).
// Data per problem: [kH | items x kD].  The problem's cost is sum_i c_i as ONE residual (Cost(Scalar), cost.h:22), inlier ratio 1.
#pragma once
#include "fused_kernels.hpp"

namespace toa {

// H(a, b) of a body: the upper triangle (row-major, diagonal included) of one lane's partial Hessian; a > b: the sink
template <typename T, int N>
struct HessUpper {
  T* t;
  T sink;
  static __host__ __device__ constexpr int index(int a, int b) { return a * N - a * (a - 1) / 2 + (b - a); }
  __device__ __forceinline__ T& operator()(int a, int b) { return a <= b ? t[index(a, b)] : sink; }
};

template <typename T, typename F>
struct HessCostModel {
  using Scalar = T;
  static constexpr int kN = F::kN, kD = F::kD, kH = F::kH;
  static constexpr int kTri = kN * (kN + 1) / 2;
  static constexpr int kXdim = 0;
  static constexpr int kNpad = 16;
  static_assert(kN >= 1 && kN <= 12, "the Hessian's triangle is kept in registers: n <= 12");
  __device__ __forceinline__ void set_loss(int, double) {}  // a scalar cost has no residuals to robustify
  __device__ __forceinline__ void plus_eq(WaveLds<T>& L, const T* d, T sign, int, int lane) const { euclid_plus_eq(L, d, sign, lane); }
  const T* data;
  const T* d;
  int items;
  T row[kN];   // lane a < kN: row a of the folded Hessian of the last Build (undamped)
  __device__ __forceinline__ void init(int, int m, const void* dp) { items = m; data = static_cast<const T*>(dp); }   // (one "residual" per item: m = items)
  __device__ __forceinline__ void bind(long long p) { d = data + size_t(p) * (kH + size_t(items) * kD); }

  __device__ __forceinline__ void accumulate(WaveLds<T>& L, int, int lane, T& cost, int& nres) {
    T x[kN];
#pragma unroll
    for (int a = 0; a < kN; ++a) x[a] = L.xs[a];
    T acc[kN + kTri];   // this lane's gradient, then its triangle: folded together
#pragma unroll
    for (int i = 0; i < kN + kTri; ++i) acc[i] = T(0);
    HessUpper<T, kN> Hs{acc + kN, T(0)};
    T csum = T(0);
    const T* itemsp = d + kH;
    for (int i = lane; i < items; i += 64) {
      T c;
      F::template eval_hess<true>(x, d, itemsp + size_t(i) * kD, c, acc, Hs);
      csum += c;
    }
    wave_allreduce_many(acc, lane);
    cost = wave_allreduce_sum(csum);
    nres = 1;
    // lane a keeps H(a, .): selects over compile-time indices (every lane holds every total)
    static_for<kN>([&](auto ib) __attribute__((always_inline)) {
      constexpr int b = decltype(ib)::value;
      T r = T(0);
      static_for<kN>([&](auto ia) __attribute__((always_inline)) {
        constexpr int a = decltype(ia)::value;
        const T v = acc[kN + HessUpper<T, kN>::index(a < b ? a : b, a < b ? b : a)];
        r = lane == a ? v : r;
      });
      row[b] = r;
    });
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < kN; ++a) {
        L.g[a] = acc[a];
        L.hd[a] = acc[kN + HessUpper<T, kN>::index(a, a)];
      }
    }
    wave_sync();
  }
  __device__ __forceinline__ void evaluate(const WaveLds<T>& L, int, int lane, T& cost, int& nres) const {
    T x[kN];
#pragma unroll
    for (int a = 0; a < kN; ++a) x[a] = L.xs[a];
    HessUpper<T, kN> Hs{nullptr, T(0)};
    T csum = T(0);
    const T* itemsp = d + kH;
    for (int i = lane; i < items; i += 64) {
      T c;
      F::template eval_hess<false>(x, d, itemsp + size_t(i) * kD, c, static_cast<T*>(nullptr), Hs);
      csum += c;
    }
    cost = wave_allreduce_sum(csum);
    nres = 1;
  }
  template <typename O>
  __device__ __forceinline__ void write_sym(O* M, int LD, int, int lane) const {
    if (lane < kN) {
#pragma unroll
      for (int b = 0; b < kN; ++b) M[lane * LD + b] = O(row[b]);
    }
  }
};

// The Accumulate seam (toa_jit_accumulate on a TOA_JIT_COST_HESS model): one wave per problem (grid-stride), g [P][n], the full
// symmetric H [P][n][n] when H_ is not null, cost [P] = sum_i c_i as accumulated, nres [P] = 1.  accumulate_kernel's arguments.
template <typename Model>
__global__ void __launch_bounds__(256) hess_accumulate_kernel(const void* data_, const void* x_, long long P, int n, int m, int want_grad, void* g_,
                                                              void* H_, double* cost, int* nres, int lds_per_wave, int, double) {
  using T = typename Model::Scalar;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* X = static_cast<const T*>(x_);
  Model model;
  model.init(n, m, data_);
  WaveLds<T> L = WaveLds<T>::carve(smem + size_t(wave) * lds_per_wave, n);
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
      if (H_) model.write_sym(static_cast<T*>(H_) + size_t(p) * n * n, n, n, lane);
    } else {
      model.evaluate(L, n, lane, c, nr);
    }
    if (lane == 0) { cost[p] = double(c); if (nres) nres[p] = nr; }
  }
}

}  // namespace toa
