// Ragged batches through the header-only C++ adaptor: JitResidual::bind_ragged, and Optimize / diff::Eval / diff::CalculateJac on the
// model it returns.  The circle fit of tests/circle.cpp:32-68 as run-time text, a different number of points in every problem (one
// of them none): every problem must come out bit for bit as the same problem solved alone in a uniform batch of its own count.
// Needs a GPU to run; compiles with plain g++.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static_assert(TOA_ABI_VERSION == 7, "additive change");
static_assert(detail::is_ragged<RaggedJitModel<double>>::value && !detail::is_ragged<JitModel<double>>::value, "trait");
static_assert(!detail::is_jit<RaggedJitModel<double>>::value, "a ragged model never reaches the uniform entry points");

int main() {
  Context ctx(0);
  const char* circle = "const S dx = p[0] - x[0];\nconst S dy = p[1] - x[1];\nr[0] = dx * dx + dy * dy - x[2] * x[2];";
  const std::vector<int64_t> counts = {3, 10, 0, 65, 130};
  const int P = int(counts.size());
  std::vector<double> pts;
  for (int p = 0; p < P; ++p)
    for (int64_t i = 0; i < counts[p]; ++i) {
      const double a = 0.3 * p + 6.283185307179586 * double(i) / double(counts[p]);
      pts.push_back(2.0 + 2.0 * std::cos(a) + 1e-5 * std::sin(17.0 * i + p));
      pts.push_back(7.0 + 2.0 * std::sin(a) + 1e-5 * std::cos(29.0 * i + p));
    }
  JitResidual<double> res(ctx, circle, /*n=*/3, /*item_scalars=*/2);
  const auto model = res.bind_ragged(counts, pts.data());
  REQUIRE(model.P() == P && model.max_items() == 130 && model.total_items() == 208 && model.rows() == 208);
  Options o;
  o.lm.damping_init = 1e1;
  std::vector<double> x(size_t(P) * 3);
  for (int p = 0; p < P; ++p) { x[3 * p] = 0; x[3 * p + 1] = 0; x[3 * p + 2] = 1; }
  const std::vector<double> x0 = x;
  const auto rj = diff::Eval(model, x0);
  const auto jac = diff::CalculateJac(model, x0);
  const auto r_only = diff::Eval(model, x0, false);
  REQUIRE(rj.first.size() == 208 && rj.second.size() == 208 * 3 && jac == rj.second && r_only.first == rj.first && r_only.second.empty());
  const BatchOutput out = Optimize(x, model, o, true);
  std::vector<double> xk = x0;
  const BatchOutput outk = Optimize(xk, model, o, true, QueueOrder::kKeepOrder);
  REQUIRE(xk == x && outk.errs == out.errs && outk.stop_reason == out.stop_reason && outk.num_iters == out.num_iters);
  size_t first = 0;
  for (int p = 0; p < P; ++p) {
    if (counts[p] == 0) {
      REQUIRE(out.stop_reason[p] == kSkipped && out.final_num_residuals[p] == 0);
      REQUIRE(x[3 * p] == 0 && x[3 * p + 1] == 0 && x[3 * p + 2] == 1);
      continue;
    }
    const auto alone = res.bind(1, int(counts[p]), pts.data() + 2 * first);
    std::vector<double> x1 = {0, 0, 1};
    const auto e1 = diff::Eval(alone, x1);
    for (int64_t i = 0; i < counts[p]; ++i) {
      REQUIRE(e1.first[i] == rj.first[first + i]);
      for (int a = 0; a < 3; ++a) REQUIRE(e1.second[3 * i + a] == rj.second[3 * (first + i) + a]);
    }
    const BatchOutput o1 = Optimize(x1, alone, o, true);
    REQUIRE(x1[0] == x[3 * p] && x1[1] == x[3 * p + 1] && x1[2] == x[3 * p + 2]);
    REQUIRE(o1.stop_reason[0] == out.stop_reason[p] && o1.num_iters[0] == out.num_iters[p] && o1.final_cost[0] == out.final_cost[p]);
    REQUIRE(o1.final_num_residuals[0] == out.final_num_residuals[p] && out.final_num_residuals[p] == counts[p]);
    for (int k = 0; k < out.hist_stride; ++k) REQUIRE(o1.errs[k] == out.errs[size_t(p) * out.hist_stride + k]);
    REQUIRE(std::fabs(x[3 * p] - 2) < 1e-4 && std::fabs(x[3 * p + 1] - 7) < 1e-4 && std::fabs(std::fabs(x[3 * p + 2]) - 2) < 1e-4);
    first += size_t(counts[p]);
  }
  {
    // refusals: host controls have no ragged form; a wrong x size throws before any launch; a negative count
    Options oc = o;
    oc.max_duration_ms = 5.0;
    bool threw = false;
    std::vector<double> x2 = x0;
    try { (void)Optimize(x2, model, oc); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
    threw = false;
    std::vector<double> bad(2);
    try { (void)Optimize(bad, model, o); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
    threw = false;
    try { (void)res.bind_ragged({2, -1}, pts.data()); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
