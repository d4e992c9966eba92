// A Gaussian prior beside a run-time model through the header-only C++ adaptor: JitResidual::bind(...).with_prior(mu, W, rows) and
// bind_ragged(...).with_prior(...).  The circle fit of tests/circle.cpp:32-68 as run-time text with a diagonal prior: a huge W pins x
// to mu, a negligible one leaves the fit where the data put it, a problem without items converges to mu, and the residual count is
// items + n.  Needs a GPU to run; compiles with plain g++.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static_assert(TOA_ABI_VERSION == 7, "additive change");
static_assert(detail::takes_prior<JitModel<double>>::value && detail::takes_prior<RaggedJitModel<double>>::value, "trait");
static_assert(!detail::takes_prior<DenseRow<double>>::value, "compiled-in families take no prior");
static_assert(sizeof(toa_prior) == 2 * sizeof(void*) + 6 * sizeof(int32_t), "toa_prior layout");

int main() {
  Context ctx(0);
  const char* circle = "const S dx = p[0] - x[0];\nconst S dy = p[1] - x[1];\nr[0] = dx * dx + dy * dy - x[2] * x[2];";
  const int P = 3, items = 10, n = 3;
  std::vector<double> pts;
  for (int p = 0; p < P; ++p)
    for (int i = 0; i < items; ++i) {
      const double a = 0.3 * p + 6.283185307179586 * double(i) / double(items);
      pts.push_back(2.0 + 2.0 * std::cos(a) + 1e-5 * std::sin(17.0 * i + p));
      pts.push_back(7.0 + 2.0 * std::sin(a) + 1e-5 * std::cos(29.0 * i + p));
    }
  JitResidual<double> res(ctx, circle, n, /*item_scalars=*/2);
  std::vector<double> mu(size_t(P) * n), Whuge(size_t(P) * n, 1e6), Wtiny(size_t(P) * n, 1e-6);
  for (int p = 0; p < P; ++p) { mu[3 * p] = 1.5 + 0.1 * p; mu[3 * p + 1] = 6.5; mu[3 * p + 2] = 2.5; }
  Options o;
  o.lm.damping_init = 1e1;
  o.max_iters = 100;
  const std::vector<double> x0 = {0, 0, 1, 0, 0, 1, 0, 0, 1};
  {
    // a huge W pins x to mu (the data's pull is 1e-12 of the prior's); every problem counts items + n residuals
    const auto model = res.bind(P, items, pts.data()).with_prior(mu.data(), Whuge.data(), 0);
    REQUIRE(model.has_prior());
    std::vector<double> x = x0;
    const BatchOutput out = Optimize(x, model, o);
    for (int p = 0; p < P; ++p) {
      REQUIRE(out.Succeeded(size_t(p)) && out.final_num_residuals[p] == items + n && out.final_inlier_ratio[p] == 1.0f);
      for (int a = 0; a < n; ++a) REQUIRE(std::fabs(x[3 * p + a] - mu[3 * p + a]) < 1e-6);
    }
  }
  {
    // a negligible W leaves the circle where the points put it
    const auto model = res.bind(P, items, pts.data()).with_prior(mu.data(), Wtiny.data(), 0);
    std::vector<double> x = x0;
    const BatchOutput out = Optimize(x, model, o);
    for (int p = 0; p < P; ++p) {
      REQUIRE(out.Succeeded(size_t(p)));
      REQUIRE(std::fabs(x[3 * p] - 2) < 1e-4 && std::fabs(x[3 * p + 1] - 7) < 1e-4 && std::fabs(std::fabs(x[3 * p + 2]) - 2) < 1e-4);
    }
  }
  {
    // ragged, the full form (W = the identity as three rows), Gauss-Newton: the problem without items lands on mu and is not skipped
    const std::vector<int64_t> counts = {10, 0, 10};
    std::vector<double> rp(pts.begin(), pts.begin() + 2 * items);
    rp.insert(rp.end(), pts.begin() + 4 * items, pts.end());
    std::vector<double> W(size_t(P) * n * n, 0.0);
    for (int p = 0; p < P; ++p) for (int a = 0; a < n; ++a) W[size_t(p) * n * n + a * n + a] = 1.0;
    const auto model = res.bind_ragged(counts, rp.data()).with_prior(mu.data(), W.data(), n);
    Options g = o;
    g.solver_type = Options::GaussNewton;
    std::vector<double> x = x0;
    x[0] = 2; x[1] = 7; x[2] = 2; x[6] = 2; x[7] = 7; x[8] = 2;   // (Gauss-Newton on the circle starts near it)
    const BatchOutput out = Optimize(x, model, g);
    REQUIRE(out.stop_reason[1] != kSkipped && out.Succeeded(1) && out.final_num_residuals[1] == n);
    for (int a = 0; a < n; ++a) REQUIRE(std::fabs(x[3 + a] - mu[3 + a]) < 1e-12);
    REQUIRE(out.final_num_residuals[0] == items + n && out.final_num_residuals[2] == items + n);
  }
  {
    // refusals, before any launch: host controls, the stepping Optimizer, Eval, rows > n
    const auto model = res.bind(P, items, pts.data()).with_prior(mu.data(), Wtiny.data(), 0);
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
    try { (void)res.bind(P, items, pts.data()).with_prior(mu.data(), Wtiny.data(), n + 1); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
