// Box bounds and fixed parameters through the header-only C++ adaptor: JitResidual::bind(...).with_bounds(lo, hi) and
// bind_ragged(...).with_bounds(...).  The circle fit of tests/circle.cpp:32-68 as run-time text: bounds at -inf / +inf leave the solve
// as it is bit for bit, a fixed parameter keeps its start value bit for bit, a binding bound is met exactly, and the refusals throw
// before any launch.  Needs a GPU to run; compiles with plain g++.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static_assert(TOA_ABI_VERSION == 7, "additive change");
static_assert(detail::takes_bounds<JitModel<double>>::value && detail::takes_bounds<RaggedJitModel<double>>::value, "trait");
static_assert(!detail::takes_bounds<DenseRow<double>>::value, "compiled-in families take no bounds");
static_assert(sizeof(toa_bounds) == 2 * sizeof(void*) + 4 * sizeof(int32_t), "toa_bounds layout");

int main() {
  Context ctx(0);
  const char* circle = "const S dx = p[0] - x[0];\nconst S dy = p[1] - x[1];\nr[0] = dx * dx + dy * dy - x[2] * x[2];";
  const int P = 3, items = 10, n = 3;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> pts;
  for (int p = 0; p < P; ++p)
    for (int i = 0; i < items; ++i) {
      const double a = 0.3 * p + 6.283185307179586 * double(i) / double(items);
      pts.push_back(2.0 + 2.0 * std::cos(a) + 1e-5 * std::sin(17.0 * i + p));
      pts.push_back(7.0 + 2.0 * std::sin(a) + 1e-5 * std::cos(29.0 * i + p));
    }
  JitResidual<double> res(ctx, circle, n, /*item_scalars=*/2);
  Options o;
  o.lm.damping_init = 1e1;
  o.max_iters = 100;
  o.max_consec_failures = 30;
  const std::vector<double> x0 = {0, 0, 1, 0, 0, 1, 0, 0, 1};
  std::vector<double> xplain = x0;
  const BatchOutput plain = Optimize(xplain, res.bind(P, items, pts.data()), o, true);
  {
    // no bound anywhere (both sides null: -inf / +inf): the plain solve, bit for bit
    const auto model = res.bind(P, items, pts.data()).with_bounds(nullptr, nullptr);
    REQUIRE(model.has_bounds() && !model.has_prior());
    std::vector<double> x = x0;
    const BatchOutput out = Optimize(x, model, o, true);
    REQUIRE(std::memcmp(x.data(), xplain.data(), x.size() * sizeof(double)) == 0);
    REQUIRE(out.stop_reason == plain.stop_reason && out.num_iters == plain.num_iters && out.num_failures == plain.num_failures);
    REQUIRE(std::memcmp(out.final_cost.data(), plain.final_cost.data(), size_t(P) * sizeof(double)) == 0);
    REQUIRE(std::memcmp(out.errs.data(), plain.errs.data(), out.errs.size() * sizeof(double)) == 0);
    REQUIRE(std::memcmp(out.final_hessian.data(), plain.final_hessian.data(), out.final_hessian.size() * sizeof(double)) == 0);
  }
  {
    // problem 1 holds its radius at 1.5 (lo == hi; the start 1 is clipped onto it), problem 2 keeps its centre's x below 1.8: the
    // fixed value stays bit for bit, the binding bound is met exactly, problem 0 is the plain solve
    std::vector<double> lo(size_t(P) * n, -inf), hi(size_t(P) * n, inf);
    lo[3 + 2] = hi[3 + 2] = 1.5;
    hi[6 + 0] = 1.8;
    const auto model = res.bind(P, items, pts.data()).with_bounds(lo.data(), hi.data());
    std::vector<double> x = x0;
    const BatchOutput out = Optimize(x, model, o);
    for (int p = 0; p < P; ++p) REQUIRE(out.stop_reason[p] != kSolverFailed && out.stop_reason[p] >= 0);
    REQUIRE(std::memcmp(&x[0], &xplain[0], n * sizeof(double)) == 0);
    REQUIRE(x[5] == 1.5);
    REQUIRE(x[6] == 1.8);
    for (size_t i = 0; i < x.size(); ++i) REQUIRE(lo[i] <= x[i] && x[i] <= hi[i]);
    // the last Build's matrix: the fixed parameter's row and column are the unit vector
    const double* H = &out.final_hessian[size_t(1) * n * n];
    REQUIRE(H[2 * n + 2] == 1.0 && H[2 * n + 0] == 0.0 && H[2 * n + 1] == 0.0 && H[0 * n + 2] == 0.0 && H[1 * n + 2] == 0.0);
  }
  {
    // ragged: the same bounds on a batch whose middle problem has no items (skipped: x is its clipped start)
    const std::vector<int64_t> counts = {10, 0, 10};
    std::vector<double> rp(pts.begin(), pts.begin() + 2 * items);
    rp.insert(rp.end(), pts.begin() + 4 * items, pts.end());
    std::vector<double> lo(size_t(P) * n, -inf), hi(size_t(P) * n, inf);
    lo[3 + 2] = hi[3 + 2] = 1.5;
    const auto model = res.bind_ragged(counts, rp.data()).with_bounds(lo.data(), hi.data());
    std::vector<double> x = x0;
    const BatchOutput out = Optimize(x, model, o);
    REQUIRE(out.stop_reason[1] == kSkipped && x[5] == 1.5);
    REQUIRE(std::memcmp(&x[0], &xplain[0], n * sizeof(double)) == 0);
  }
  {
    // refusals, before any launch: host controls, the stepping Optimizer, Eval, lo > hi
    const auto model = res.bind(P, items, pts.data()).with_bounds(nullptr, nullptr);
    Options oc = o;
    oc.max_duration_ms = 5.0;
    std::vector<double> x = x0;
    bool threw = false;
    try { (void)Optimize(x, model, oc); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
    threw = false;
    try { (void)diff::Eval(model, x0); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
    threw = false;
    try { Optimizer<double, JitModel<double>> opt(x, model, o); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
    threw = false;
    std::vector<double> lo(size_t(P) * n, 1.0), hi(size_t(P) * n, 0.0);
    try { (void)res.bind(P, items, pts.data()).with_bounds(lo.data(), hi.data()); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
