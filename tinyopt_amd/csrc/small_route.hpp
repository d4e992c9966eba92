// Who runs a solve or a data pass of a compiled-in model family (n <= 63; toa_lm_run, toa_lm_run_split, toa_lm_begin / step / stop and
// toa_accumulate): the ONE place where that is decided.  Plain C++ with no HIP in it and no handle: integers and bools in, a family
// out, so that a host compiler can check it against the ladders it replaced (tests/test_cpu_small_route.py).  The caller (capi.hip)
// has checked shape, model and loss before it asks, computes the instance keys (nbm and thin of DenseRowLayout::make, npad) once,
// and launches what the family names; TOA_MODEL_DENSE_ROW_NATURAL never comes here (large_n.hip / large_fused.hip).
//
// The order of decisions of small_lm_route, which is the order a caller who breaks two rules sees:
//   1. the stepping form (mode != 0): TOA_MODEL_DENSE_ROW_AD has a stepping kernel of its own, everything else runs on the
//      launch-per-iteration kernels with one chunk per problem (Wide, splits = 1);
//   2. splits == -1: the automatic choice between row-split (0) and one wavefront per problem (-1);
//   3. DenseRow with an M-estimator on the handle: narrow-fused for a batch where a lane instance exists, else Wide;
//   4. splits >= 0: Wide — or the refusal, for a family that has no row-split form;
//   5. TOA_MODEL_DENSE_ROW_AD, the "misc" families, the narrow routes of DenseRow, DenseRow on the matrix cores: in that order.
// No branch of it is out of reach of a call: nothing here is declared unreachable, and the test allows no difference.
#pragma once
#include "../../include/tinyopt_amd.h"

namespace toa {

enum class SmallFamily {
  DenseFused,         // DenseRowModel<T, nbm, thin> in the fused kernel: sixteen lanes per row, the Gram on the matrix cores
  NarrowFused,        // DenseRow on the narrow routes (inst.hip -DTOA_INST_NARROW): an item / a row per lane
  JetRowFused,        // TOA_MODEL_DENSE_ROW_AD: RowModel over AdRowFunctor, n = 12 and n = 50
  MiscFused,          // every other family (inst.hip -DTOA_INST_MISC)
  Wide,               // the row-split driver (launch_wide: team, persistent or launch-per-iteration form); with mode != 0 the stepping form
  JetRowStepping,     // the stepping form of TOA_MODEL_DENSE_ROW_AD
  NarrowAccumulate, JetRowAccumulate, MiscAccumulate, DenseAccumulate,   // toa_accumulate: one data pass of the same four
  Refused
};

struct SmallRoute {
  SmallFamily family;
  int splits;        // Wide only: what launch_wide is asked for (0 = it chooses the chunking)
  int code;          // Refused only: the TOA_E_* code ...
  const char* why;   // ... and the text of toa_last_error()
};

// the instances of inst.hip's narrow routes of TOA_MODEL_DENSE_ROW (JetModel / RowModel over the packed rows)
inline bool dense_row_lane_route(int dtag, int n, bool robust) {
  if (n >= 1 && n <= (dtag == 0 ? 11 : 5)) return true;      // narrow blocks, with or without an M-estimator
  if (dtag == 1 && n == 6) return true;                      // (fp64 n = 6: JetModel without the estimator branch for L2, RowModel with a loss)
  if (!robust) return false;
  return n == 12 || n == 50;                                  // the BASELINE shapes with an M-estimator on the handle
}

// dtag: 0 = fp32, 1 = fp64.  splits: -1 = choose (toa_lm_run and the stepping entries), >= 0 = toa_lm_run_split's argument.
// mode: 0 = a whole solve, 1 / 2 / 3 = begin / step / stop.  loss_set: toa_set_loss other than L2 on the handle.  The last three
// are toa_tuning's fields of the same names.
inline SmallRoute small_lm_route(int model, int dtag, int n, int m, long long P, int num_cus, int splits, int mode, bool loss_set,
                                 bool narrow_mfma_pass, bool wide_no_autosplit, long long wide_team_max_per_cu) {
  // the stepping form runs on the launch-per-iteration kernels with one chunk per problem (launch_stepping)
  if (mode != 0) return {model == TOA_MODEL_DENSE_ROW_AD ? SmallFamily::JetRowStepping : SmallFamily::Wide, 1, 0, nullptr};
  const bool splittable = model == TOA_MODEL_DENSE_ROW || model == TOA_MODEL_SE3_REPROJ;
  const bool few = P * 4 <= num_cus && m >= 512;
  // splits < 0: automatic — row-split when one-wave-per-problem would leave most of the chip idle
  // (fewer problems than CUs and enough rows to give every chunk >= 256 of them)
  //   or, for small problems (n <= 15, 512..4096 rows), the team form: one workgroup per problem has no co-residency
  //   requirement, so it also pays for whole batches of them — measured (tests/tools/team_probe.py, C2-sized problems):
  //   89-100 us for 1..256 problems against 131-144 us with one wavefront per problem; the crossover is one problem per
  //   compute unit at n = 6 x 1000 rows and two at n = 12 x 2000.  toa_tuning::wide_team_max_per_cu overrides, toa_tuning::wide_no_autosplit disables.
  if (splits == -1) {
    const long long team_per_cu = wide_team_max_per_cu > 0 ? wide_team_max_per_cu : ((long long)m * (n + 1) >= 20000 ? 2 : 1);
    const bool team = n <= 15 && m >= 512 && m <= 4096 && P <= team_per_cu * num_cus;
    splits = (splittable && !wide_no_autosplit && (few || team)) ? 0 : -1;
  }
  // DenseRow with an M-estimator on the handle: the robust data pass lives in the launch-per-iteration form (kernels.hpp
  // RobustOf): chunked automatically for a few huge problems, one chunk per problem for a batch
  // (round 6: where a row-per-lane instance exists — inst.hip — a BATCH runs the loss inside the fused kernel instead)
  if (model == TOA_MODEL_DENSE_ROW && loss_set && splits < 0) {
    if (!few && !narrow_mfma_pass && dense_row_lane_route(dtag, n, true)) return {SmallFamily::NarrowFused, 0, 0, nullptr};
    splits = few ? 0 : 1;
  }
  if (splits >= 0) {
    if (!splittable) return {SmallFamily::Refused, 0, TOA_E_UNSUPPORTED, "row-split execution is available for DenseRow and SE3Reproj"};
    return {SmallFamily::Wide, splits, 0, nullptr};
  }
  if (model == TOA_MODEL_DENSE_ROW_AD) return {SmallFamily::JetRowFused, 0, 0, nullptr};
  if (model != TOA_MODEL_DENSE_ROW) return {SmallFamily::MiscFused, 0, 0, nullptr};
  // narrow fp32 blocks: a row per lane (RowModel) instead of sixteen lanes per row (toa_tuning::narrow_mfma_pass: the old route)
  if (!narrow_mfma_pass && dense_row_lane_route(dtag, n, false)) return {SmallFamily::NarrowFused, 0, 0, nullptr};
  return {SmallFamily::DenseFused, 0, 0, nullptr};
}

// toa_accumulate: the same ladder without the solve (the narrow route's seam serves plain L2 only)
inline SmallFamily small_accumulate_route(int model, int dtag, int n, bool loss_set, bool narrow_mfma_pass) {
  if (model == TOA_MODEL_DENSE_ROW_AD) return SmallFamily::JetRowAccumulate;
  if (model != TOA_MODEL_DENSE_ROW) return SmallFamily::MiscAccumulate;
  if (!loss_set && !narrow_mfma_pass && dense_row_lane_route(dtag, n, false)) return SmallFamily::NarrowAccumulate;
  return SmallFamily::DenseAccumulate;
}

}  // namespace toa
