// The rows of a run-time model with MORE than 63 parameters (toa_jit_spec::large_n): residuals and Jacobian rows
// of a batch written out, one item per lane, for 1 <= n <= 1024 (fp64: 512).
//
//   res [P][m]        m = items x kR; an item's kR rows are consecutive
//   J   [P][jstride]  per problem m rows of ldj >= n scalars, row-major; columns n .. ldj - 1 are written as zeros
//                     (Eval: ldj = n, jstride = m n — the caller's dense tensor; the pipeline: ldj = n rounded up to 16 bytes)
//
// RF is the row functor the model has: UserFunctor with its own Jacobian (eval_manual), or LargeAdRowFunctor below over a residual
// body.  Nothing of size n lives in registers: x is ONE LDS copy per workgroup, an item's scalars are staged lane-linear into the
// wave's raw image, and the body writes its Jacobian rows straight into the wave's J image in LDS (a T (*)[kN] view of it, dense,
// beside the raw items — a body reads p[j] and writes J[q][j] in the same loop).  The image then leaves lane-linear: the rows of a
// super-step are one contiguous run of rows x ldj scalars in memory, stored in 16-byte pieces when the run is 16-byte aligned and
// ldj a multiple of the vector, scalar by scalar otherwise.  Nothing outside the outputs is written.
// Grid (row blocks, problems): wave w of block b takes the super-steps (4 b + w) + k x 4 x gridDim.x of problem blockIdx.y.
//
// What a problem gets is its MODE: 0 = left alone, 1 = residuals only (the body runs cost-only), 2 = residuals and Jacobian.
// mode[p] when the array is there (the large-n pipeline fills it per pass from its state, large_n.hip), else mode_all for every
// problem (the Accumulate seam, Eval).  The code object knows nothing of the pipeline's structures: plain pointers and ints.
//
// gpart (mode 2, optional): the wave's partial J^T r, gpart[p][slot = 4 b + w][n] with gslots = 4 x gridDim.x slots per problem —
// summed over the wave's rows in row order straight from the LDS image, super-step after super-step; a wave without rows writes
// zeros.  large_pre_kernel / large_seam_out_kernel add the slots in slot order: no GEMV, no second pass over J.
// The geometry (items per super-step, the regions) is LargeModelGeom's, which the host launcher evaluates too.
#pragma once
#include "kernels.hpp"
#include "large_model_geom.hpp"

namespace toa {

// Forward-mode AD as a manual-Jacobian functor for wide rows: AdRowFunctor's scheme (row_model.hpp) with the chunks of TOA_AD_CW
// parameters walked by a RUN-TIME loop — static_for would inline the body 86 times at n = 1024.  c0 is wave-uniform (made so for
// the compiler by readfirstlane), so the seeds are still formed on the scalar unit (seed_one); the last chunk of a width that is no
// multiple of TOA_AD_CW is cut by the guard c0 + s < kN.  Cost-only: the body on plain T.
template <typename T, typename F>
struct LargeAdRowFunctor {
  static constexpr int kN = F::kN, kR = F::kR, kD = F::kD, kH = F::kH;
  static constexpr bool kManual = true;
  static constexpr int kCW = TOA_AD_CW;
  template <bool want_grad>
  static __device__ __forceinline__ void eval_manual(const T* x, const T* h, const T* p, T* r, T (*J)[kN]) {
    if constexpr (!want_grad) {
      F::template eval<T>(x, h, p, r);
    } else {
#pragma nounroll
      for (int c = 0; c < kN; c += kCW) {
        const int c0 = __builtin_amdgcn_readfirstlane(c);
        const ChunkSeededX<T, kCW> X{x, c0};
        Jet<T, kCW> rr[kR];
        F::template eval<Jet<T, kCW>>(X, h, p, rr);
#pragma unroll
        for (int q = 0; q < kR; ++q) {
          if (c0 == 0) r[q] = rr[q].a;
#pragma unroll
          for (int s = 0; s < kCW; ++s)
            if (c0 + s < kN) J[q][c0 + s] = rr[q].v[s];
        }
      }
    }
  }
};

template <typename T, typename RF, bool WANT_J>
__global__ void __launch_bounds__(256) large_model_rows_kernel(const T* __restrict__ data, const T* __restrict__ x, const int num_items,
                                                               const long long data_stride, T* __restrict__ res, T* __restrict__ J, const int ldj, const long long jstride,
                                                               const int* __restrict__ mode, const int mode_all, T* __restrict__ gpart, const int gslots) {
  constexpr int kN = RF::kN, kR = RF::kR, kD = RF::kD, kH = RF::kH;
  constexpr LargeModelGeom G = LargeModelGeom::make(int(sizeof(T)), kN, kR, kD, WANT_J);
  static_assert(G.items >= 1 && G.rows <= 64 && G.bytes <= LargeModelGeom::kBudget, "the LDS geometry holds no item (the host refuses such a model)");
  constexpr int IT = G.items, PS = G.ps, VEC = 16 / int(sizeof(T));
  typedef T TV __attribute__((ext_vector_type(16 / sizeof(T))));

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const long long p = blockIdx.y;
  const int md = mode ? mode[p] : mode_all;   // (uniform over the workgroup)
  if (md == 0) return;
  const bool with_j = WANT_J && md == 2;
  constexpr int kG = WANT_J ? (kN + 63) / 64 : 1;   // columns of J^T r per lane
  T gacc[kG];
#pragma unroll
  for (int k = 0; k < kG; ++k) gacc[k] = T(0);
  T* const xs = reinterpret_cast<T*>(smem);
  for (int j = threadIdx.x; j < kN; j += 256) xs[j] = x[size_t(p) * kN + j];
  __syncthreads();
  char* const wbase = smem + G.wave_off + wave * G.wave_bytes;
  T* const raw = reinterpret_cast<T*>(wbase + G.raw_off);
  T* const img = reinterpret_cast<T*>(wbase + G.img_off);
  T* const rl = reinterpret_cast<T*>(wbase + G.r_off);
  const T* const d = data + size_t(p) * size_t(data_stride);   // [kH header scalars | items x kD]
  const T* const itemsp = d + kH;
  const size_t m = size_t(num_items) * kR;
  T* const Rp = res ? res + size_t(p) * m : nullptr;
  T* const Jp = (with_j && J) ? J + size_t(p) * size_t(jstride) : nullptr;
  const int nss = (num_items + IT - 1) / IT;
  for (int ss = blockIdx.x * 4 + wave; ss < nss; ss += int(gridDim.x) * 4) {
    const int it0 = ss * IT;
    const int cnt = min(IT, num_items - it0);
    wave_sync();   // (the previous super-step's copy-out has read the image; its functors their items)
    if constexpr (kD > 0) {   // the items of the super-step, one contiguous run in memory -> item i at i * PS
      const T* const src = itemsp + size_t(it0) * kD;
      const int tot = cnt * kD;
      for (int e = lane; e < tot; e += 64) {
        const int it = e / kD, w = e - it * kD;
        raw[it * PS + w] = src[e];
      }
    }
    wave_sync();
    if (lane < cnt) {
      T rv[kR];
      const T* const pi = raw + lane * PS;
      if constexpr (WANT_J) {
        if (with_j) {
          RF::template eval_manual<true>(xs, d, pi, rv, reinterpret_cast<T(*)[kN]>(img + size_t(lane) * kR * kN));
          if (gpart) {
#pragma unroll
            for (int q = 0; q < kR; ++q) rl[lane * kR + q] = rv[q];
          }
        } else {
          RF::template eval_manual<false>(xs, d, pi, rv, static_cast<T(*)[kN]>(nullptr));
        }
      } else {
        RF::template eval_manual<false>(xs, d, pi, rv, static_cast<T(*)[kN]>(nullptr));
      }
      if (Rp) {
        T* const ro = Rp + size_t(it0 + lane) * kR;
#pragma unroll
        for (int q = 0; q < kR; ++q) ro[q] = rv[q];
      }
    }
    if constexpr (WANT_J) {
      wave_sync();
      if (with_j && gpart) {   // J^T r of the super-step's rows, in row order: lane l owns columns l, l + 64, ...
        const int rows_here = cnt * kR;
        for (int row = 0; row < rows_here; ++row) {
          const T rr = rl[row];
#pragma unroll
          for (int k = 0; k < kG; ++k)
            if (lane + 64 * k < kN) gacc[k] = fma(img[row * kN + lane + 64 * k], rr, gacc[k]);
        }
      }
      if (Jp) {   // rows [it0 * kR, (it0 + cnt) * kR) x ldj: one run
        T* const g0 = Jp + size_t(it0) * kR * size_t(ldj);
        const unsigned total = unsigned(cnt * kR) * unsigned(ldj);
        const bool vec = ldj % VEC == 0 && (reinterpret_cast<size_t>(g0) & 15) == 0;   // (wave-uniform)
        if (vec) {
          for (unsigned v = unsigned(lane); v < total / VEC; v += 64) {
            const unsigned e = v * VEC, row = e / unsigned(ldj), col = e - row * unsigned(ldj);   // (a piece never straddles two rows)
            TV t;
#pragma unroll
            for (int k = 0; k < VEC; ++k) t[k] = col + k < unsigned(kN) ? img[row * kN + col + k] : T(0);
            *reinterpret_cast<TV*>(g0 + e) = t;
          }
        } else {
          for (unsigned e = unsigned(lane); e < total; e += 64) {
            const unsigned row = e / unsigned(ldj), col = e - row * unsigned(ldj);
            g0[e] = col < unsigned(kN) ? img[row * kN + col] : T(0);
          }
        }
      }
    }
  }
  if constexpr (WANT_J) {
    if (with_j && gpart) {
      T* const gp = gpart + (size_t(p) * size_t(gslots) + size_t(blockIdx.x * 4 + wave)) * kN;
#pragma unroll
      for (int k = 0; k < kG; ++k)
        if (lane + 64 * k < kN) gp[lane + 64 * k] = gacc[k];
    }
  }
}

}  // namespace toa
