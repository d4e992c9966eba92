// The first-order hot path: gd_fused_kernel (whole gradient-descent solves of a scalar cost, one wavefront per problem,
// dynamic problem queue) and the Build seam cost_accumulate_kernel (g = sum_i grad c_i, cost), over CostModel — a scalar
// cost summed over items, supplied as run-time text (csrc/jit.hip, TOA_JIT_COST / TOA_JIT_COST_GRAD).
//
// The pass (CostModel::pass) is the only hot loop: the items are dealt to the 64 lanes (item i to lane i mod 64), each lane
// keeps its partial cost and its partial gradient (n <= 63 scalars) in registers, and the wave folds them ONCE per pass
// (wave_allreduce_many).  No Gram, no factorisation: one read of the problem's data per iteration.  The items are loaded
// straight from HBM, no LDS stage: at n = 12 (52-byte items) the pass streams 0.76-0.78 of the 8 TB/s peak in fp32 and fp64
// (profiles/r07_gd_probe.jsonl).
//
// Functor concept (all static): kN parameters, kD scalars per item, kH header scalars per problem, kCostKind:
//   TOA_JIT_COST (2):       template <class S, class X> eval(const X& x, const T* h, const T* p, S& c)
//                           c = the item's cost term, written over the scalar type S: on Jet<T, kN> (n <= 12) or on chunked
//                           Jet<T, <= 12> (one evaluation per chunk of seeded columns) for the gradient, on plain T cost-only;
//   TOA_JIT_COST_GRAD (3):  template <bool want_grad, class X> eval_grad(const X& x, const T* h, const T* p, T& c, T* G)
//                           the reference's f(x, grad) form (tests/unconstrained.cpp:19-42): c on plain T and, if want_grad,
//                           the item's own gradient ADDED to G[a].
// Data per problem: [kH | items x kD] (the layout of the run-time residual models).
#pragma once
#include <hip/hip_runtime.h>

#ifdef __HIPCC_RTC__   // run-time compilation (jit.hip): the headers are handed to hiprtc by NAME, embedded in the library
#include "tinyopt_amd.h"
#else
#include "../../include/tinyopt_amd.h"
#endif
#include "gd_device.hpp"
#include "jet.hpp"
#include "wave_utils.hpp"
#include "ragged.hpp"
#include "num_diff.hpp"   // NumCostFunctor: a cost body differentiated by finite differences (toa_jit_spec::diff)

namespace toa {

struct GdParams {
  const void* data;
  void* x;
  long long P;
  int n, items;
  toa_options opt;
  toa_results res;
  float lr;                        // toa_gd_options::lr (options.h:148)
  int lds_per_wave;
  unsigned long long* counters;    // [TOA_NUM_COUNTERS] or null
  int* queue;                      // [0] pop counter, [16] waves that have left the kernel (lm_fused_kernel's protocol)
};

// a ragged launch's block (ragged.hpp, fused_kernels.hpp RaggedFusedParams)
struct RaggedGdParams {
  GdParams g;
  RaggedArgs ragged;
};

// x as Jets of one chunk of columns [c0, c0 + CW), read from the wave's LDS copy (n > 12: a register array indexed by the
// body's running j would be scratch memory)
template <typename T, int CW>
struct GdSeededX {
  const T* xs;
  int c0;
  __device__ __forceinline__ Jet<T, CW> operator[](int j) const {
    Jet<T, CW> r;
    r.a = xs[j];
#pragma unroll
    for (int s = 0; s < CW; ++s) r.v[s] = (j == c0 + s) ? T(1) : T(0);
    return r;
  }
};

template <typename T, typename F>
struct CostModel {
  using Scalar = T;
  static constexpr int kN = F::kN, kD = F::kD, kH = F::kH;
  static constexpr bool kOwnGrad = F::kCostKind == 3;
  static constexpr int kChunks = (kN + 11) / 12;                 // Jets of <= 12 partials, as balanced as kN allows
  static constexpr int kCW = (kN + kChunks - 1) / kChunks;
  static_assert(kN >= 1 && kN <= 63, "one wavefront per problem: n <= 63");
  const T* data;
  const T* d;
  int items;
  __device__ __forceinline__ void init(int items_, const void* dp) { items = items_; data = static_cast<const T*>(dp); }
#ifdef TOA_RAGGED
  // Ragged batches (ragged.hpp; the ragged code object of a run-time model only)
  RaggedArgs rag;
  const T* ritems;   // the bound problem's first item
  __device__ __forceinline__ void set_ragged(const RaggedArgs& a) { rag = a; }
  __device__ __forceinline__ void bind(long long p) {
    const RaggedRange r = ragged_range(rag, p);
    ritems = data + size_t(r.first) * kD;
    d = static_cast<const T*>(rag.header) + size_t(p) * kH;
    items = r.count;
  }
#else
  __device__ __forceinline__ void bind(long long p) { d = data + size_t(p) * (kH + size_t(items) * kD); }
#endif

  // This lane's share of the pass: its items' cost terms summed into the return value, their gradients into G.
  template <bool WANT_G>
  __device__ __forceinline__ T pass(const WaveLds<T>& L, const int lane, T (&G)[kN]) const {
#pragma unroll
    for (int a = 0; a < kN; ++a) G[a] = T(0);
    T csum = T(0);
#ifdef TOA_RAGGED
    const T* itemsp = ritems;
#else
    const T* itemsp = d + kH;
#endif
    if constexpr (kN <= 12) {
      T x[kN];
#pragma unroll
      for (int a = 0; a < kN; ++a) x[a] = L.xs[a];
      for (int i = lane; i < items; i += 64) {
        const T* item = itemsp + size_t(i) * kD;
        if constexpr (kOwnGrad) {
          T c;
          F::template eval_grad<WANT_G>(x, d, item, c, G);
          csum += c;
        } else if constexpr (!WANT_G) {
          T c;
          F::template eval<T>(x, d, item, c);
          csum += c;
        } else {
          // (seeded Jets formed per access from the LDS copy: a register array of Jets indexed by a loop the compiler does not
          //  unroll — fp64 logistic body at n = 12 — would be scratch memory)
          const GdSeededX<T, kN> xj{L.xs, 0};   // optimize_autodiff.h:56-69
          Jet<T, kN> c;
          F::template eval<Jet<T, kN>>(xj, d, item, c);
          csum += c.a;
#pragma unroll
          for (int a = 0; a < kN; ++a) G[a] += c.v[a];
        }
      }
    } else {
      const T* x = L.xs;
      for (int i = lane; i < items; i += 64) {
        const T* item = itemsp + size_t(i) * kD;
        if constexpr (kOwnGrad) {
          T c;
          F::template eval_grad<WANT_G>(x, d, item, c, G);
          csum += c;
        } else if constexpr (!WANT_G) {
          T c;
          F::template eval<T>(x, d, item, c);
          csum += c;
        } else {
          static_for<kChunks>([&](auto cc) __attribute__((always_inline)) {
            constexpr int c0 = decltype(cc)::value * kCW;
            const GdSeededX<T, kCW> X{x, c0};
            Jet<T, kCW> c;
            F::template eval<Jet<T, kCW>>(X, d, item, c);
            if constexpr (c0 == 0) csum += c.a;
#pragma unroll
            for (int s = 0; s < kCW; ++s)
              if (c0 + s < kN) G[c0 + s] += c.v[s];
          });
        }
      }
    }
    return csum;
  }

  // Build (gd.h Accumulate): g = sum_i grad c_i into L.g[0..kN), the cost sum_i c_i returned in every lane.
  __device__ __forceinline__ void accumulate(WaveLds<T>& L, const int, const int lane, T& cost) const {
    T G[kN];
    const T c = pass<true>(L, lane, G);
    wave_allreduce_many(G, lane);
    cost = wave_allreduce_sum(c);
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < kN; ++a) L.g[a] = G[a];
    }
    wave_sync();
  }
  __device__ __forceinline__ void evaluate(const WaveLds<T>& L, const int lane, T& cost) const {
    T G[kN];
    cost = wave_allreduce_sum(pass<false>(L, lane, G));
  }
};

template <typename Model>
__global__ void __launch_bounds__(256) gd_fused_kernel(const GdParams* __restrict__ prm_g) {
  using T = typename Model::Scalar;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n = prm_g->n;
  // (no factorisation workspace: the carve of a zero-parameter block — x, g, dx, the last step and the state record)
  WaveLds<T> L = WaveLds<T>::carve(smem + size_t(wave) * prm_g->lds_per_wave, 0);
  {
    const int* src_o = reinterpret_cast<const int*>(&prm_g->opt);
    int* dst_o = reinterpret_cast<int*>(L.opt);
    for (int i = lane; i < int(sizeof(toa_options) / 4); i += 64) dst_o[i] = src_o[i];
    const int* src_r = reinterpret_cast<const int*>(&prm_g->res);
    int* dst_r = reinterpret_cast<int*>(L.res);
    for (int i = lane; i < int(sizeof(toa_results) / 4); i += 64) dst_r[i] = src_r[i];
    L.st->acc_passes = 0; L.st->eval_passes = 0; L.st->solves = 0; L.st->problems = 0; L.st->reused_passes = 0;
    L.st->memo_slot = 0;
  }
  wave_sync();
  const long long P = prm_g->P;
  const float lr = prm_g->lr;
  Model model;
  model.init(prm_g->items, prm_g->data);
#ifdef TOA_RAGGED
  const RaggedArgs& rag = reinterpret_cast<const RaggedGdParams*>(prm_g)->ragged;
  model.set_ragged(rag);
  const int* const order = rag.order;   // the q-th problem handed out (null: problem q)
#endif
  T* X = static_cast<T*>(prm_g->x);
  int* queue = prm_g->queue;
  const int nwaves = int(gridDim.x) * 4;
  bool first = true;
  for (;;) {  // one work item = one whole problem; the first one static, the rest from the shared counter
    int p = 0;
    if (first) {
      p = int(blockIdx.x) * 4 + wave;
      first = false;
    } else {
      if (lane == 0) p = atomicAdd(queue, 1) + nwaves;
      p = __builtin_amdgcn_readfirstlane(p);
    }
    if (p >= P) break;
#ifdef TOA_RAGGED
    if (order) p = min(max(order[p], 0), int(P) - 1);   // (wave-uniform: a scalar load; clamped — a slot of a damaged order addresses no problem beyond the batch)
#endif
    model.bind(p);
#ifdef TOA_RAGGED
    if (model.items == 0) {   // no items: kSkipped, x untouched (the LM path's answer to "no residuals", optimizer.h:373-377)
      lm_init<T>(L, lane);
      L.st->stop = TOA_STOP_SKIPPED;
      gd_finalize<T>(L, (long long)p, lane);
      continue;
    }
#endif
    wave_sync();
    L.xs[lane] = lane < n ? X[size_t(p) * n + lane] : T(0);
    wave_sync();
    gd_solve_problem<T>(model, L, n, lane, (long long)p, lr);
    if (lane < n) X[size_t(p) * n + lane] = L.xs[lane];
  }
  unsigned long long* counters = prm_g->counters;
  if (counters && lane == 0) {
    atomicAdd(&counters[0], L.st->acc_passes);
    atomicAdd(&counters[2], L.st->solves);
    atomicAdd(&counters[3], L.st->problems);
  }
  // the work queue cleans itself (lm_fused_kernel): the last wave to leave puts both counters back to zero
  if (lane == 0) {
    const int gone = atomicAdd(&queue[16], 1);
    if (gone == int(gridDim.x) * 4 - 1) {
      __hip_atomic_store(&queue[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&queue[16], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Build seam (SolverGD::Build's accumulation, toa_jit_accumulate): one wave per problem (grid-stride), g [P][n] (want_grad),
// cost [P] = sum_i c_i as accumulated (not normalised, not clamped), nres [P] = 1.
template <typename Model>
__global__ void __launch_bounds__(256) cost_accumulate_kernel(const void* data_, const void* x_, long long P, int items, int want_grad,
                                                              void* g_, double* cost, int* nres, int lds_per_wave TOA_RAGGED_KARG) {
  using T = typename Model::Scalar;
  constexpr int n = Model::kN;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* X = static_cast<const T*>(x_);
  Model model;
  model.init(items, data_);
#ifdef TOA_RAGGED
  model.set_ragged(rag);
#endif
  WaveLds<T> L = WaveLds<T>::carve(smem + size_t(wave) * lds_per_wave, 0);
  for (long long p = (long long)blockIdx.x * 4 + wave; p < P; p += (long long)gridDim.x * 4) {
    wave_sync();
    L.xs[lane] = lane < n ? X[size_t(p) * n + lane] : T(0);
    wave_sync();
    model.bind(p);
    T c;
    if (want_grad) {
      model.accumulate(L, n, lane, c);
      if (lane < n) static_cast<T*>(g_)[size_t(p) * n + lane] = L.g[lane];
    } else {
      model.evaluate(L, lane, c);
    }
#ifdef TOA_RAGGED
    if (lane == 0) { cost[p] = double(c); if (nres) nres[p] = model.items > 0 ? 1 : 0; }
#else
    if (lane == 0) { cost[p] = double(c); if (nres) nres[p] = 1; }
#endif
  }
}

}  // namespace toa
