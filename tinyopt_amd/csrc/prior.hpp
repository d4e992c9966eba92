// A Gaussian prior beside a run-time model's items: per problem p, with n parameters,
//
//   mu  [P][n]
//   W   [P][n]      diagonal form (rows = 0):      r_j = W_j (x_j - mu_j),  k = n residuals
//       [P][k][n]   full form (rows = k, 1 <= k <= n, row-major):  r = W (x - mu)
//
// added AFTER the item pass of every Build and every cost-only Evaluate: cost += |r|^2, nres += k, and on a Build g += W^T r,
// H += W^T W — what a user of the reference adds to H, g and the cost at the end of a hand-written Accumulate callback
// (docs/API.md:37-57; W = diag(1 / sigma) is its GaussianPrior, W = U its tests/cov.cpp:96).  The prior's residuals do not go
// through the handle's M-estimator and count as inliers.
//
// The prior kernels are the uniform / ragged ones over PriorModel<Model>, compiled with TOA_PRIOR defined (code objects of their
// own, jit.hip ensure_form).  Nothing here is seen by a build without the macro except the plain struct below.
#pragma once

namespace toa {

// What a prior kernel is given on top of its uniform / ragged parameters.
struct PriorArgs {
  const void* mu;   // [P][n]
  const void* W;    // [P][n] (rows = 0) or [P][rows][n]
  int rows;         // 0: the diagonal form; 1 .. n: rows of the full form (wave-uniform: a kernel argument)
  int reserved_;
};

// the prior code objects' seam kernel takes them as one more kernel argument
#ifdef TOA_PRIOR
#define TOA_PRIOR_KARG , const toa::PriorArgs pri
#else
#define TOA_PRIOR_KARG
#endif

#ifdef TOA_PRIOR
// The wrapper: everything of the model (init / bind / set_loss / set_ragged / stage / memo_save / plus_eq / kNpad / kXdim ...) is
// inherited; accumulate, evaluate, memo_reextract and memo_restore add the prior to the sums the model has FOLDED (items + prior,
// never interleaved), write_sym adds the off-diagonals of W^T W to the image the model wrote.  Lane j owns column j of W: a row of
// W is one lane-contiguous load, its product with x - mu one wave all-reduce (a fixed butterfly: every lane gets the same bits,
// whatever wave runs the problem), and the sums over the k rows run in row order in every lane.  n is the model's compile-time kN,
// k a kernel argument: no register array is indexed by a run-time value.  The model's memo keeps the items' Gram only; the prior
// is recomputed at the restored x.
// a base that sums its items' own cost terms (RowModel over an item-cost functor: ggn_multi_cost.hpp)
template <typename M, typename = void>
struct ModelItemCost { static constexpr bool value = false; };
template <typename M>
struct ModelItemCost<M, std::enable_if_t<M::kItemCost>> { static constexpr bool value = true; };

template <typename Base>
struct PriorModel : Base {
  using T = typename Base::Scalar;
  static constexpr int kN = Base::kN;
  static_assert(Base::kXdim == 0, "a Gaussian prior is x - mu: Euclidean parameters only");
  // Rows of W fetched together: a row is one load per lane whose latency (an L2 hit: ~1 us) nothing else hides on this path, and the
  // full form reads k rows per Build and k rows per sixteen image rows of every write_sym — one at a time that was 45 % of an LM
  // iteration at the C4 shape (section 14 of DESIGN).  Rows beyond k load nothing and add +0.
  static constexpr int kRowBatch = 8;
  PriorArgs pri;
  const T* mu_p;   // the bound problem's mu and W
  const T* W_p;
  T* img;          // the wave's factorisation workspace (WaveLds::M): dead whenever write_sym runs, its staging image
  int img_ld;
  __device__ __forceinline__ void set_prior(const PriorArgs& a, T* M, int LD) { pri = a; img = M; img_ld = LD; mu_p = nullptr; W_p = nullptr; }
  __device__ __forceinline__ void bind(long long p) {
    Base::bind(p);
    mu_p = static_cast<const T*>(pri.mu) + size_t(p) * kN;
    W_p = static_cast<const T*>(pri.W) + size_t(p) * (size_t(pri.rows ? pri.rows : 1) * kN);
  }

  // cost += |r|^2, nres += k; WANT_GRAD: g += W^T r, hd += diag(W^T W) (the UNDAMPED diagonal: damping, clipping and
  // check_min_H_diag see the sum)
  template <bool WANT_GRAD>
  __device__ __forceinline__ void add_prior(WaveLds<T>& L, const int lane, T& cost, int& nres) {
    wave_sync();   // (the model's g / hd are in LDS)
    const bool in = lane < kN;
    const T dl = in ? L.xs[lane] - mu_p[lane] : T(0);
    T gp = T(0), hp = T(0), cp = T(0);
    int k = kN;
    if (pri.rows == 0) {
      const T w = in ? W_p[lane] : T(0);
      const T r = w * dl;
      cp = wave_allreduce_sum(r * r);
      gp = w * r;
      hp = w * w;
    } else {
      k = pri.rows;
      for (int q0 = 0; q0 < k; q0 += kRowBatch) {   // rows in order, in every lane; kRowBatch loads in flight at a time
        T w[kRowBatch];
#pragma unroll
        for (int b = 0; b < kRowBatch; ++b) w[b] = (in && q0 + b < k) ? W_p[size_t(q0 + b) * kN + lane] : T(0);
#pragma unroll
        for (int b = 0; b < kRowBatch; ++b) {   // (a row beyond k is all zeros: it adds +0 to every sum)
          const T r = wave_allreduce_sum(w[b] * dl);
          cp = fma(r, r, cp);
          if constexpr (WANT_GRAD) { gp = fma(w[b], r, gp); hp = fma(w[b], w[b], hp); }
        }
      }
    }
    if constexpr (WANT_GRAD) {
      if (in) { L.g[lane] = L.g[lane] + gp; L.hd[lane] = L.hd[lane] + hp; }
    }
    if constexpr (ModelItemCost<Base>::value) {
      // a scalar cost: the prior is the ridge term (1/2) |W (x - mu)|^2 (the halving is exact), so that g += W^T r stays the gradient
      // of the reported cost and H += W^T W its Hessian; the cost stays ONE residual, the inlier count is left alone
      cost = cost + T(0.5) * cp;
    } else {
      cost = cost + cp;
      nres += k;
      if (Base::ninl >= 0) Base::ninl += k;   // (-1: no loss, every residual an inlier)
    }
    wave_sync();
  }
  __device__ __forceinline__ void accumulate(WaveLds<T>& L, int n, int lane, T& cost, int& nres) {
    Base::accumulate(L, n, lane, cost, nres);
    add_prior<true>(L, lane, cost, nres);
  }
  __device__ __forceinline__ void evaluate(WaveLds<T>& L, int n, int lane, T& cost, int& nres) {
    Base::evaluate(L, n, lane, cost, nres);
    add_prior<false>(L, lane, cost, nres);
  }
  __device__ __forceinline__ void memo_reextract(WaveLds<T>& L, int n, int lane, T& cost, int& nres) {
    Base::memo_reextract(L, n, lane, cost, nres);
    add_prior<true>(L, lane, cost, nres);
  }
  __device__ __forceinline__ void memo_restore(WaveLds<T>& L, int n, int lane, T& cost, int& nres) {
    Base::memo_restore(L, n, lane, cost, nres);
    add_prior<true>(L, lane, cost, nres);
  }

  // image[i][lane] += sum_q W[q][i] W[q][lane], sixteen rows i of the image at a time: the row of W once per lane, its element i
  // by readlane (a compile-time index), sixteen accumulators per lane
  __device__ __forceinline__ void add_wtw(T* M, const int LD, const int lane) const {
    const bool in = lane < kN;
    static_for<(kN + 15) / 16>([&](auto cc) __attribute__((always_inline)) {
      constexpr int c0 = decltype(cc)::value * 16;
      T acc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = T(0);
      for (int q0 = 0; q0 < pri.rows; q0 += kRowBatch) {
        T w[kRowBatch];
#pragma unroll
        for (int b = 0; b < kRowBatch; ++b) w[b] = (in && q0 + b < pri.rows) ? W_p[size_t(q0 + b) * kN + lane] : T(0);
        static_for<kRowBatch>([&](auto bc) __attribute__((always_inline)) {
          constexpr int b = decltype(bc)::value;
          static_for<16>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = decltype(ic)::value;
            if constexpr (c0 + i < kN) acc[i] = fma(wave_bcast(w[b], c0 + i), w[b], acc[i]);
          });
        });
      }
      static_for<16>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        if constexpr (c0 + i < kN) {
          if (in) M[(c0 + i) * LD + lane] = M[(c0 + i) * LD + lane] + acc[i];
        }
      });
    });
  }
  // The symmetric undamped H into an LD-strided image, for every caller (the solve, its re-creation after a failed fast
  // factorisation, final_hessian, the seam).  The diagonal form adds nothing off the diagonal, and every caller takes the diagonal
  // from hd.  The full form adds W^T W in LDS: in place when the image IS the wave's workspace, otherwise (an image in memory, of
  // another scalar type for final_hessian) through the workspace, which is dead then.
  template <typename O>
  __device__ __forceinline__ void write_sym(O* M, int LD, int n, int lane) const {
    if (pri.rows == 0) { Base::write_sym(M, LD, n, lane); return; }
    if (static_cast<const void*>(M) == static_cast<const void*>(img)) {
      Base::write_sym(img, img_ld, n, lane);
      wave_sync();
      add_wtw(img, img_ld, lane);
      return;
    }
    wave_sync();
    Base::write_sym(img, img_ld, n, lane);
    wave_sync();
    add_wtw(img, img_ld, lane);
    wave_sync();
    for (int e = lane; e < kN * kN; e += 64) {
      const int i = e / kN, j = e - i * kN;
      M[i * LD + j] = O(img[i * img_ld + j]);
    }
    wave_sync();
  }
};
#endif  // TOA_PRIOR

}  // namespace toa
