// A second-order scalar cost through the header-only C++ adaptor, the way the reference's own test calls it
// (tests/optimize_easy.cpp:35-79): Rosenbrock as `f(x, grad, H) -> cost`, here as run-time text (TOA_JIT_COST_HESS), from (-1.2, 1)
// with max_iters = 200, min_rerr_dec = 0, max_consec_failures = 20 -> (1, 1) with the oracle's StopReason (kMinError after 59
// passes: tests/golden/reference_traces.json, the first case).  GradientDescent on it throws, as the reference does.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
  Context ctx(0);
  const char* rosenbrock =
      "const T t1 = T(1.0) - x[0], t2 = x[1] - x[0] * x[0];\n"
      "c = t1 * t1 + T(100.0) * t2 * t2;\n"
      "if (want_grad) {\n"
      "  G[0] += T(-2.0) * t1 - T(400.0) * x[0] * t2;\n"
      "  G[1] += T(200.0) * t2;\n"
      "  H(0, 0) += T(2.0) - T(400.0) * x[1] + T(1200.0) * x[0] * x[0];\n"
      "  H(0, 1) += T(-400.0) * x[0];\n"
      "  H(1, 1) += T(200.0);\n"
      "}";
  JitResidual<double> loss(ctx, rosenbrock, /*n=*/2, /*item_scalars=*/1, 1, 0, TOA_MANIFOLD_EUCLID, kJitCostHess);
  REQUIRE(loss.stats().num_regs > 0);
  const double unused = 0.0;   // the one data scalar of the one item
  const auto cost = loss.bind(1, 1, &unused);
  std::vector<double> x = {-1.2, 1.0};
  Options options;
  options.max_iters = 200;
  options.min_rerr_dec = 0;
  options.max_consec_failures = 20;
  const auto out = Optimize(x, cost, options);
  REQUIRE(out.Succeeded(0));
  REQUIRE(out.Converged(0));
  REQUIRE(out.stop_reason[0] == kMinError);
  REQUIRE(out.num_iters[0] >= 55 && out.num_iters[0] <= 63);   // (59 in the oracle; the last passes trade last bits of a cost of 1e-14)
  REQUIRE(out.num_failures[0] > 0);                            // the bad-step branch ran
  REQUIRE(std::fabs(x[0] - 1.0) < 1e-5 && std::fabs(x[1] - 1.0) < 1e-5);
  REQUIRE(out.final_num_residuals[0] == 1);
  REQUIRE(out.final_hessian.size() == 4 && out.final_hessian[3] == 200.0 && out.final_hessian[1] == out.final_hessian[2]);
  // GradientDescent on f(x, grad, H): refused (optimize.h:59-75 throws for this signature)
  Options gd;
  gd.solver_type = Options::GradientDescent;
  bool threw = false;
  try { std::vector<double> x2 = {-1.2, 1.0}; (void)Optimize(x2, cost, gd); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  REQUIRE(x[0] != -1.2);
  // ... and so are a prior, bounds and a ragged batch
  threw = false;
  try { const double mu[2] = {0, 0}, W[2] = {1, 1}; auto c2 = loss.bind(1, 1, &unused); c2.with_prior(mu, W); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  try { (void)loss.bind_ragged({1}, &unused); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
