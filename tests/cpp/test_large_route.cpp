// large_route() against the five hand-written predicates it replaced, restated literally from commit 68b07ee (file:lines cited at
// each).  Prints every (entry, input) at which the route differs; a difference that large_route.hpp declares unreachable is printed
// with the word "declared", any other with "UNEXPECTED".  Last line: the two counts.
#include <cstddef>
#include <cstdio>

#include "../../tinyopt_amd/csrc/large_route.hpp"

using toa::LargeRoute;

struct In {
  size_t max_lds;
  bool force_lib;
  size_t es;   // element size: 4 (TOA_F32) or 8
  int n;
  long long P;
  bool use_ldlt;
};

// large_n.hip:1693, 1696 — the LDS sizes as the templates had them
static size_t chol_solve_lds_bytes_68b07ee(size_t es, int n) { return (size_t(32) * 36 + size_t(n) * 36 + size_t(n) + 64 + 32) * es + 64; }
static size_t ldlt_image_bytes_68b07ee(size_t es, int n) { return ((size_t(n) * (n | 1) + 16) * es + 15) & ~size_t(15); }

// large_n.hip:2082-2091 — large_lm_run_t
static LargeRoute lm_loop(const In& i) {
  const bool lu = !i.use_ldlt;                                    // :2028
  const bool force_lib = i.force_lib;                             // :2082
  const size_t chol_lds = ldlt_image_bytes_68b07ee(i.es, i.n);    // :2083
  const bool own_chol = !lu && !force_lib && i.n <= 128 && chol_lds + 4096 <= i.max_lds;                     // :2084
  const size_t chol2_lds = chol_solve_lds_bytes_68b07ee(i.es, i.n);                                          // :2090
  const bool own_chol2 = !own_chol && !lu && !force_lib && i.n > 128 && chol2_lds + 2048 <= i.max_lds;       // :2091
  return own_chol ? LargeRoute::WorkgroupLdlt : own_chol2 ? LargeRoute::BlockedCholesky : LargeRoute::Library;
}
// large_n.hip:2461-2465 (and :2410 for which of the two kernels large_solve_own_t takes) — toa_large_solve
static LargeRoute solve(const In& i) {
  const bool force_lib = i.force_lib;
  const size_t chol_lds = ((size_t(i.n) * (i.n | 1) + 16) * i.es + 15) & ~size_t(15);
  const size_t chol2_lds = (size_t(32) * 36 + size_t(i.n) * 37 + 96) * i.es + 64;
  const bool own2 = i.n > 128 && i.P <= 65535 && chol2_lds + 2048 <= i.max_lds;
  if (!force_lib && ((i.n <= 128 && chol_lds + 4096 <= i.max_lds) || own2)) return i.n <= 128 ? LargeRoute::WorkgroupLdlt : LargeRoute::BlockedCholesky;
  return LargeRoute::Library;
}
// large_n.hip:2489-2491 — toa_large_solve_each: true = hands the batch to toa_large_solve, false = one library call per matrix
static bool each_is_ours(const In& i) {
  const bool force_lib = i.force_lib;
  const size_t chol2_lds = (size_t(32) * 36 + size_t(i.n) * 37 + 96) * i.es + 64;
  return !force_lib && (i.n <= 128 || (i.P <= 65535 && chol2_lds + 2048 <= i.max_lds));
}
// large_n.hip:2434-2435 — toa_large_solve_inplace: true = the blocked Cholesky in place, false = toa_large_solve_each
static bool inplace_is_ours(const In& i) {
  const size_t lds = (size_t(32) * 36 + size_t(i.n) * 37 + 96) * i.es + 64;
  return !(i.force_lib || i.n <= 128 || i.P > 65535 || lds + 2048 > i.max_lds);
}
// ba_schur.hip:1739-1741 — toa_ba_lists_run under capture: true = not refused for its solver
static bool ba_capture_is_ours(const In& i) {
  const size_t chol2_lds = (size_t(32) * 36 + size_t(i.n) * 37 + 96) * i.es + 64;
  const bool own_solver = i.n <= 128 || (i.P <= 65535 && chol2_lds + 2048 <= i.max_lds);
  return !(!i.use_ldlt || i.force_lib || !own_solver);
}

static const char* name(LargeRoute r) { return r == LargeRoute::WorkgroupLdlt ? "ldlt" : r == LargeRoute::BlockedCholesky ? "chol" : "library"; }

int main() {
  long declared = 0, unexpected = 0;
  const size_t lds_sizes[2] = {65536, 163840};
  const long long batches[3] = {1, 65535, 65536};
  for (size_t max_lds : lds_sizes)
    for (int force = 0; force < 2; ++force)
      for (size_t es = 4; es <= 8; es += 4)
        for (int ldlt = 0; ldlt < 2; ++ldlt)
          for (long long P : batches)
            for (int n = 64; n <= 1100; ++n) {
              const In i{max_lds, force != 0, es, n, P, ldlt != 0};
              auto report = [&](const char* entry, const char* was, const char* is, bool is_declared) {
                std::printf("%s %s: max_lds=%zu force_library=%d elem=%zu n=%d P=%lld use_ldlt=%d: %s -> %s\n", is_declared ? "declared" : "UNEXPECTED",
                            entry, max_lds, force, es, n, P, ldlt, was, is);
                ++(is_declared ? declared : unexpected);
              };
              // the two differences large_route.hpp declares unreachable
              const bool lm_beyond_grid_y = P > 65535;   // the LM loop is entered with at most 65 535 problems
              const bool small_lds = n <= 128 && toa::ldlt_image_bytes(es, n) + 4096 > max_lds;   // needs a device with < 136 320 bytes of LDS
              const LargeRoute r = toa::large_route(max_lds, force != 0, es, n, P, ldlt != 0).route;
              if (r != lm_loop(i)) report("large_lm_run_t", name(lm_loop(i)), name(r), lm_beyond_grid_y);
              // the K3 seams decide for use_ldlt = true (use_ldlt = false has an entry of its own, toa_large_solve_unchecked)
              const LargeRoute rs = toa::large_route(max_lds, force != 0, es, n, P, true).route;
              if (ldlt) {
                if (rs != solve(i)) report("toa_large_solve", name(solve(i)), name(rs), false);
                if ((rs != LargeRoute::Library) != each_is_ours(i)) report("toa_large_solve_each", each_is_ours(i) ? "ours" : "library", name(rs), small_lds);
                if ((rs == LargeRoute::BlockedCholesky) != inplace_is_ours(i)) report("toa_large_solve_inplace", inplace_is_ours(i) ? "chol" : "each", name(rs), false);
              }
              if ((r != LargeRoute::Library) != ba_capture_is_ours(i)) report("toa_ba_lists_run", ba_capture_is_ours(i) ? "ours" : "refused", name(r), small_lds);
              // the byte-size forms against the formulas three of the sites had copied by hand
              if (toa::chol_solve_lds_bytes(es, n) != (size_t(32) * 36 + size_t(n) * 37 + 96) * es + 64 || toa::chol_solve_lds_bytes(es, n) != chol_solve_lds_bytes_68b07ee(es, n) ||
                  toa::ldlt_image_bytes(es, n) != ldlt_image_bytes_68b07ee(es, n))
                report("lds bytes", "?", "?", false);
            }
  std::printf("declared %ld unexpected %ld\n", declared, unexpected);
  return unexpected == 0 ? 0 : 1;
}
