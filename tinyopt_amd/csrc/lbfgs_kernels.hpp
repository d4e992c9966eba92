// lbfgs_fused_kernel: whole L-BFGS solves of a scalar cost (lbfgs_device.hpp), one wavefront per problem.  The
// twin of gd_fused_kernel (gd_kernels.hpp): its launch shape, its queue protocol, its counters and its TOA_RAGGED branch, over the
// same CostModel.  A wave's LDS is its plain carve, then its ring of (s, y) pairs — as much as the launch's history asks for.
#pragma once
#include "gd_kernels.hpp"
#include "lbfgs_device.hpp"

namespace toa {

struct LbfgsParams {
  const void* data;
  void* x;
  long long P;
  int n, items;
  toa_options opt;
  toa_results res;
  int history;                     // toa_lbfgs_options::history: pairs kept, 1 .. 16
  float c1, shrink;                // ... ::c1 (Armijo), ::shrink (backtracking factor)
  int lds_per_wave;                // the carve and the ring
  int ring_off;                    // where the ring starts in a wave's region
  unsigned long long* counters;    // [TOA_NUM_COUNTERS] or null
  int* queue;                      // [0] pop counter, [16] waves that have left the kernel (lm_fused_kernel's protocol)
};

struct RaggedLbfgsParams {
  LbfgsParams g;
  RaggedArgs ragged;
};

template <typename Model>
__global__ void __launch_bounds__(256) lbfgs_fused_kernel(const LbfgsParams* __restrict__ prm_g) {
  using T = typename Model::Scalar;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  // (made uniform for the compiler: the carve's and the ring's pointers then live in scalar registers across the hot pass — fp64
  //  cost_grad at n = 12: 195 -> 150 vector registers, three waves per SIMD as the GD kernel has)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = prm_g->n;
  char* const region = smem + size_t(wave) * prm_g->lds_per_wave;
  WaveLds<T> L = WaveLds<T>::carve(region, 0);
  const LbfgsRing<T> R = LbfgsRing<T>::carve(region + prm_g->ring_off, prm_g->history, Model::kN);
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
  const float c1 = prm_g->c1, shrink = prm_g->shrink;
  Model model;
  model.init(prm_g->items, prm_g->data);
#ifdef TOA_RAGGED
  const RaggedArgs& rag = reinterpret_cast<const RaggedLbfgsParams*>(prm_g)->ragged;
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
    if (order) p = min(max(order[p], 0), int(P) - 1);   // (wave-uniform: a scalar load; clamped, as in gd_fused_kernel)
#endif
    model.bind(p);
#ifdef TOA_RAGGED
    if (model.items == 0) {   // no items: kSkipped, x untouched
      lm_init<T>(L, lane);
      L.st->stop = TOA_STOP_SKIPPED;
      gd_finalize<T>(L, (long long)p, lane);
      continue;
    }
#endif
    wave_sync();
    L.xs[lane] = lane < n ? X[size_t(p) * n + lane] : T(0);
    wave_sync();
    lbfgs_solve_problem<T>(model, L, R, n, lane, (long long)p, c1, shrink);
    if (lane < n) X[size_t(p) * n + lane] = L.xs[lane];
  }
  unsigned long long* counters = prm_g->counters;
  if (counters && lane == 0) {
    atomicAdd(&counters[0], L.st->acc_passes);
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

}  // namespace toa
