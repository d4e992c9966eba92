// Who factorises the damped n x n systems of the large-n path (n >= 64): the ONE place where that is decided.  Plain C++ with no
// HIP in it, so that a host compiler can check it against the predicates it replaced (tests/test_cpu_large_route.py).
#pragma once
#include <cstddef>

namespace toa {

enum class LargeRoute {
  WorkgroupLdlt,     // n <= 128: the one-workgroup LDL^T on an LDS image of the matrix (ldlt_wg.hpp)
  BlockedCholesky,   // 128 < n: the one-workgroup blocked Cholesky + substitutions (large_chol_solve_kernel), fp32 n <= 1024, fp64 n <= 512
  Library            // rocSOLVER: beyond those, for use_ldlt = false (a general LU), and with toa_tuning::large_library_solver
};

// dynamic LDS of the two kernels, by element size (the templated forms in large_n.hip call these)
inline size_t ldlt_image_bytes(size_t elem_size, int n) { return ((size_t(n) * (n | 1) + 16) * elem_size + 15) & ~size_t(15); }
inline size_t chol_solve_lds_bytes(size_t elem_size, int n) { return (size_t(32) * 36 + size_t(n) * 36 + size_t(n) + 64 + 32) * elem_size + 64; }

struct LargeRouteChoice {
  LargeRoute route;
  size_t lds;   // dynamic LDS bytes of the kernel chosen (0 for the library)
};

// 64 <= n <= 128: the workgroup LDL^T — measured crossover (tools/k3_crossover.py); beyond 128 unknowns the blocked Cholesky while its
// panel fits the LDS; the library otherwise.  P <= 65535: the blocked Cholesky's callers index problems through grid.y elsewhere.
//
// Every entry point calls this with what it has: the LM loop (large_lm_run_t), toa_large_solve, toa_large_solve_each,
// toa_large_solve_inplace and the captured form of toa_ba_lists_run.  Their five hand-written predicates differed in two
// places, neither of which any call can reach:
//   - the LM loop had no P clause: it is only entered with P <= 65535 (toa_large_lm_run slices, toa_large_lm_step refuses);
//   - toa_large_solve_each and toa_ba_lists_run took n <= 128 for "ours" without looking at the LDS: the image of n <= 128 is at
//     most 136 320 bytes (fp64, n = 128, with its 4 096 of slack), and the devices this library is built for have 160 KiB.
inline LargeRouteChoice large_route(size_t max_lds, bool force_library, size_t elem_size, int n, long long P, bool use_ldlt) {
  if (force_library || !use_ldlt) return {LargeRoute::Library, 0};
  if (n <= 128) {
    const size_t lds = ldlt_image_bytes(elem_size, n);
    if (lds + 4096 <= max_lds) return {LargeRoute::WorkgroupLdlt, lds};
    return {LargeRoute::Library, 0};
  }
  const size_t lds = chol_solve_lds_bytes(elem_size, n);
  if (P <= 65535 && lds + 2048 <= max_lds) return {LargeRoute::BlockedCholesky, lds};
  return {LargeRoute::Library, 0};
}

}  // namespace toa
