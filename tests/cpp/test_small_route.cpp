// small_lm_route() / small_accumulate_route() against the two ladders they replaced, restated literally from commit b6c408d: the tail
// of lm_run_impl (capi.hip:810-852) and the ladder of toa_accumulate (capi.hip:695-705), with a handle that holds only what they read
// and every launch replaced by the name of what it launched.  Prints every input at which family, splits or refusal differ; a
// difference that small_route.hpp declares unreachable would be printed with the word "declared" (it declares none), any other with
// "UNEXPECTED".  Last line: the two counts.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../tinyopt_amd/csrc/small_route.hpp"

using toa::SmallFamily;

// ---- what the parent's code read ----
struct Tune { int narrow_mfma_pass, wide_no_autosplit, wide_team_max_per_cu; };
struct Handle { int num_cus; int loss; Tune tune; };
struct Was { SmallFamily family; int splits; int code; std::string why; };
static Was fail(int code, const char* msg) { return {SmallFamily::Refused, 0, code, msg}; }

// capi.hip:208-213
static bool dense_row_lane_route_b6c408d(int dtag, int n, bool robust) {
  if (n >= 1 && n <= (dtag == 0 ? 11 : 5)) return true;
  if (dtag == 1 && n == 6) return true;
  if (!robust) return false;
  return n == 12 || n == 50;
}
// the launches, by what they were (capi.hip:231-273: the dispatchers fan out over dtag and nbm only)
static Was toa_inst_jetrow_wide() { return {SmallFamily::JetRowStepping, 1, 0, ""}; }
static Was toa_inst_wide(int splits) { return {SmallFamily::Wide, splits, 0, ""}; }
static Was toa_inst_narrow_fused() { return {SmallFamily::NarrowFused, 0, 0, ""}; }
static Was toa_inst_jetrow_fused() { return {SmallFamily::JetRowFused, 0, 0, ""}; }
static Was toa_inst_misc_fused() { return {SmallFamily::MiscFused, 0, 0, ""}; }
static Was toa_inst_fused() { return {SmallFamily::DenseFused, 0, 0, ""}; }

// capi.hip:810-852 (state is not null: that test is an argument check and stays in lm_run_impl)
static Was lm_run_impl_tail(const Handle* h, int model, int dtype, int n, int m, long long P, int splits, int mode) {
  if (mode != 0) {
    if (model == TOA_MODEL_DENSE_ROW_AD) return toa_inst_jetrow_wide();
    return toa_inst_wide(1);
  }
  const int dtag = dtype == TOA_F32 ? 0 : 1;
  const bool splittable = model == TOA_MODEL_DENSE_ROW || model == TOA_MODEL_SE3_REPROJ;
  if (splits == -1) {
    const bool no_auto = h->tune.wide_no_autosplit != 0;
    const long long team_env = h->tune.wide_team_max_per_cu;
    const long long team_per_cu = team_env > 0 ? team_env : ((long long)m * (n + 1) >= 20000 ? 2 : 1);
    const bool few = P * 4 <= h->num_cus && m >= 512;
    const bool team = n <= 15 && m >= 512 && m <= 4096 && P <= team_per_cu * h->num_cus;
    splits = (splittable && !no_auto && (few || team)) ? 0 : -1;
  }
  if (model == TOA_MODEL_DENSE_ROW && h->loss != TOA_LOSS_L2 && splits < 0) {
    const bool few = P * 4 <= h->num_cus && m >= 512;
    if (!few && !h->tune.narrow_mfma_pass && dense_row_lane_route_b6c408d(dtag, n, true))
      return toa_inst_narrow_fused();
    splits = few ? 0 : 1;
  }
  if (splits >= 0) {
    if (!splittable) return fail(TOA_E_UNSUPPORTED, "row-split execution is available for DenseRow and SE3Reproj");
    return toa_inst_wide(splits);
  }
  if (model == TOA_MODEL_DENSE_ROW_AD) return toa_inst_jetrow_fused();
  if (model != TOA_MODEL_DENSE_ROW) return toa_inst_misc_fused();
  if (!h->tune.narrow_mfma_pass && dense_row_lane_route_b6c408d(dtag, n, false)) return toa_inst_narrow_fused();
  return toa_inst_fused();
  return fail(TOA_E_ARG, "toa_lm_run: bad block count");
}

// capi.hip:695-705
static SmallFamily toa_accumulate_ladder(const Handle* h, int model, int dtype, int n) {
  const int dtag = dtype == TOA_F32 ? 0 : 1;
  if (model == TOA_MODEL_DENSE_ROW_AD) return SmallFamily::JetRowAccumulate;     // toa_inst_jetrow_accumulate_{0,1}_0
  if (model != TOA_MODEL_DENSE_ROW) return SmallFamily::MiscAccumulate;          // toa_inst_misc_accumulate
  if (h->loss == TOA_LOSS_L2 && !h->tune.narrow_mfma_pass && dense_row_lane_route_b6c408d(dtag, n, false))
    return SmallFamily::NarrowAccumulate;                                         // toa_inst_narrow_accumulate_{0,1}_0
  return SmallFamily::DenseAccumulate;                                            // toa_inst_accumulate
}

int main() {
  long declared = 0, unexpected = 0, compared = 0;
  // every compiled-in family that reaches the ladders (TOA_MODEL_DENSE_ROW_NATURAL, 10, leaves before them)
  const int models[] = {TOA_MODEL_DENSE_ROW, TOA_MODEL_GAUSSIAN_PRIOR, TOA_MODEL_SQRT2, TOA_MODEL_SE3_REPROJ, TOA_MODEL_CIRCLE_FIT,
                        TOA_MODEL_DENSE_ROW_AD6, TOA_MODEL_TESTFN, TOA_MODEL_MAHA_PRIOR, TOA_MODEL_SE3_PRIOR, TOA_MODEL_DENSE_ROW_AD};
  const int fixed_m[] = {1, 2, 255, 256, 511, 512, 513, 1000, 2000, 4096, 4097};
  const int cus[] = {64, 256}, team_max[] = {0, 1, 3}, split_args[] = {-1, 0, 1, 7};
  for (int model : models)
    for (int dtype = TOA_F32; dtype <= TOA_F64; ++dtype)
      for (int n = 1; n <= 63; ++n) {
        int ms[13];
        std::memcpy(ms, fixed_m, sizeof(fixed_m));
        ms[12] = (20000 + n) / (n + 1);   // the first m with m (n + 1) >= 20 000, and the one before it
        ms[11] = ms[12] - 1;
        for (int loss = 0; loss < 2; ++loss)
          for (int nmp = 0; nmp < 2; ++nmp) {
            for (int num_cus : cus) {
              const Handle h0{num_cus, loss ? TOA_LOSS_HUBER : TOA_LOSS_L2, {nmp, 0, 0}};
              const SmallFamily was = toa_accumulate_ladder(&h0, model, dtype, n), is = toa::small_accumulate_route(model, dtype, n, loss != 0, nmp != 0);
              ++compared;
              if (was != is) {
                std::printf("UNEXPECTED toa_accumulate: model=%d dtype=%d n=%d loss=%d narrow_mfma_pass=%d: %d -> %d\n", model, dtype, n, loss, nmp, int(was), int(is));
                ++unexpected;
              }
              const long long Ps[] = {1, num_cus / 4, num_cus / 4 + 1, num_cus, num_cus + 1, 2 * num_cus, 2 * num_cus + 1, 100000};
              for (int m : ms)
                for (long long P : Ps)
                  for (int no_auto = 0; no_auto < 2; ++no_auto)
                    for (int team : team_max)
                      for (int splits : split_args)
                        for (int mode = 0; mode <= 3; ++mode) {
                          const Handle h{num_cus, loss ? TOA_LOSS_HUBER : TOA_LOSS_L2, {nmp, no_auto, team}};
                          const Was w = lm_run_impl_tail(&h, model, dtype, n, m, P, splits, mode);
                          const toa::SmallRoute r = toa::small_lm_route(model, dtype, n, m, P, num_cus, splits, mode, loss != 0, nmp != 0, no_auto != 0, team);
                          ++compared;
                          const bool same = w.family == r.family && (w.family != SmallFamily::Wide || w.splits == r.splits) &&
                                            (w.family != SmallFamily::Refused || (w.code == r.code && r.why && w.why == r.why));
                          if (!same) {
                            std::printf("UNEXPECTED lm_run_impl: model=%d dtype=%d n=%d m=%d P=%lld num_cus=%d loss=%d narrow_mfma_pass=%d wide_no_autosplit=%d "
                                        "wide_team_max_per_cu=%d splits=%d mode=%d: family %d splits %d code %d -> family %d splits %d code %d\n",
                                        model, dtype, n, m, P, num_cus, loss, nmp, no_auto, team, splits, mode, int(w.family), w.splits, w.code, int(r.family), r.splits, r.code);
                            ++unexpected;
                          }
                        }
            }
          }
      }
  std::printf("compared %ld declared %ld unexpected %ld\n", compared, declared, unexpected);
  return unexpected == 0 ? 0 : 1;
}
