// Box bounds and fixed parameters beside a run-time model: per problem p, with n Euclidean parameters,
//
//   lo [P][n], hi [P][n]     -inf / +inf: no bound; lo_j == hi_j: parameter j is fixed.  Precondition: no NaN, lo <= hi.
//
// 1. Start: x_j <- min(max(x_j, lo_j), hi_j) before the first Build; every x a solve visits satisfies lo <= x <= hi exactly.
// 2. Active set, after EVERY Build (items, then the prior; from the rows, the Gram registers or the memo), from the summed gradient
//    g = J^T r: j is active when lo_j == hi_j, or x_j <= lo_j && g_j > 0, or x_j >= hi_j && g_j < 0.  For an active j: g_j = 0, row and
//    column j of H are 0, H_jj = 1 — on the UNDAMPED system, where a hand-written Accumulate callback would do it: gradient clipping,
//    check_min_H_diag, the damping and the stop test's |g|^2 see the projected system, and the damped solve gives dx_j = 0.  Cost,
//    nres, inliers and the cost-only Evaluate are the model's.
// 3. Step: x_j <- clip(x_j + sign * d_j).  Where the clip moved a component, d_j becomes the step taken (x_new - x_old), so that
//    last_dx — and the roll-back x (+) (-last_dx), which clips too — undoes what was done.  A component the clip left alone keeps
//    its d_j bit for bit: bounds that never bind change nothing of a solve.
//
// The bounds kernels are the uniform / ragged / prior ones over BoxModel<Model> (with a prior: BoxModel<PriorModel<Model>>, so the
// active set sees items + prior), compiled with TOA_BOUNDS defined (code objects of their own, jit.hip ensure_form).  Nothing here
// is seen by a build without the macro except the plain struct below.
#pragma once

namespace toa {

// What a bounds kernel is given on top of its uniform / ragged / prior parameters.
struct BoundsArgs {
  const void* lo;   // [P][n]
  const void* hi;   // [P][n]
};

// the bounds code objects' seam kernel takes them as one more kernel argument
#ifdef TOA_BOUNDS
#define TOA_BOUNDS_KARG , const toa::BoundsArgs bnd
#else
#define TOA_BOUNDS_KARG
#endif

#ifdef TOA_BOUNDS
// The wrapper: everything of the model is inherited (evaluate and memo_save among it); accumulate, memo_restore and memo_reextract
// apply rule 2 to the L.g / L.hd the model has folded, write_sym zeroes the off-diagonals of the active rows and columns in the image
// the model wrote, plus_eq is rule 3.  Lane j owns parameter j: lo_j, hi_j and its active bit are registers of lane j, the wave's
// active set is one 64-bit ballot (wave-uniform).  No register array is indexed by a run-time value.
template <typename Base>
struct BoxModel : Base {
  using T = typename Base::Scalar;
  static constexpr int kN = Base::kN;
  static_assert(Base::kXdim == 0, "a box on a tangent is not a box on the parameter: Euclidean parameters only");
  BoundsArgs bnd;
  T lo_l, hi_l;              // the bound problem's interval of this lane's parameter (lanes >= n: -inf, +inf)
  unsigned long long act;    // the active set of the last Build
  T* img;                    // the wave's factorisation workspace (WaveLds::M): dead whenever write_sym runs, its staging image
  int img_ld;
  __device__ __forceinline__ void set_bounds(const BoundsArgs& a, T* M, int LD) {
    bnd = a; img = M; img_ld = LD; act = 0ull;
    lo_l = -T(__builtin_huge_valf()); hi_l = T(__builtin_huge_valf());
  }
  __device__ __forceinline__ void bind(long long p) {
    Base::bind(p);
    const int lane = lane_id();
    const bool in = lane < kN;
    lo_l = in ? static_cast<const T*>(bnd.lo)[size_t(p) * kN + lane] : -T(__builtin_huge_valf());
    hi_l = in ? static_cast<const T*>(bnd.hi)[size_t(p) * kN + lane] : T(__builtin_huge_valf());
    act = 0ull;
  }
  // comparisons, not fmin / fmax: a NaN stays a NaN (the solve then stops as it does without bounds)
  __device__ __forceinline__ T clip(T v) const { return v < lo_l ? lo_l : (v > hi_l ? hi_l : v); }
  // rule 1: x has just been loaded into L.xs
  __device__ __forceinline__ void project_start(WaveLds<T>& L, const int lane) const { L.xs[lane] = clip(L.xs[lane]); }

  // rule 2 on the sums of the Build that has just been folded
  __device__ __forceinline__ void project(WaveLds<T>& L, const int lane) {
    wave_sync();   // (the model's g / hd are in LDS)
    const T x = L.xs[lane], g = L.g[lane];
    const bool a = lane < kN && (lo_l == hi_l || (x <= lo_l && g > T(0)) || (x >= hi_l && g < T(0)));
    act = __ballot(a);
    if (a) { L.g[lane] = T(0); L.hd[lane] = T(1); }
    wave_sync();
  }
  __device__ __forceinline__ void accumulate(WaveLds<T>& L, int n, int lane, T& cost, int& nres) {
    Base::accumulate(L, n, lane, cost, nres);
    project(L, lane);
  }
  __device__ __forceinline__ void memo_reextract(WaveLds<T>& L, int n, int lane, T& cost, int& nres) {
    Base::memo_reextract(L, n, lane, cost, nres);
    project(L, lane);
  }
  __device__ __forceinline__ void memo_restore(WaveLds<T>& L, int n, int lane, T& cost, int& nres) {
    Base::memo_restore(L, n, lane, cost, nres);
    project(L, lane);
  }

  // Lane j owns column j of the image: it zeroes its elements in the active rows and, when j is active itself, its whole column
  // — every address has one writer, the zeros are symmetric, the diagonal is the caller's (from hd).
  __device__ __forceinline__ void zero_active(T* M, const int LD, const int lane) const {
    const bool in = lane < kN, mine = (act >> lane) & 1ull;
    for (int i = 0; i < kN; ++i) {
      if (in && i != lane && (mine || ((act >> i) & 1ull))) M[i * LD + lane] = T(0);
    }
  }
  // The symmetric undamped H into an LD-strided image, for every caller (the solve, its re-creation after a failed fast
  // factorisation, final_hessian, the seam).  Nothing active: the model's image as it is.  Otherwise in LDS: in place when the
  // image IS the wave's workspace, else (an image in memory, of another scalar type for final_hessian) through the workspace,
  // which is dead then — two lanes never store to one address of memory.
  template <typename O>
  __device__ __forceinline__ void write_sym(O* M, int LD, int n, int lane) const {
    if (act == 0ull) { Base::write_sym(M, LD, n, lane); return; }
    if (static_cast<const void*>(M) == static_cast<const void*>(img)) {
      Base::write_sym(img, img_ld, n, lane);
      wave_sync();
      zero_active(img, img_ld, lane);
      return;
    }
    wave_sync();
    Base::write_sym(img, img_ld, n, lane);
    wave_sync();
    zero_active(img, img_ld, lane);
    wave_sync();
    for (int e = lane; e < kN * kN; e += 64) {
      const int i = e / kN, j = e - i * kN;
      M[i * LD + j] = O(img[i * img_ld + j]);
    }
    wave_sync();
  }

  // rule 3, for both signs (d: L.dx with sign = +1, L.ldx with sign = -1)
  __device__ __forceinline__ void plus_eq(WaveLds<T>& L, T* d, T sign, int, int lane) const {
    const T x0 = L.xs[lane];
    const T x1 = x0 + sign * d[lane];
    const T xc = clip(x1);
    L.xs[lane] = xc;
    if (sign > T(0) && !bits_equal(xc, x1)) d[lane] = xc - x0;
  }
};
#endif  // TOA_BOUNDS

}  // namespace toa
