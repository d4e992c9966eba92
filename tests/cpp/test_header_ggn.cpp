// A rank-one second-order scalar cost (TOA_JIT_COST_GGN) through the header-only C++ adaptor: c = hs (a . x - b)^2 / 2 over three items
// with dyadic data, whose Newton step from (0, 0) is (1, 2) exactly (tests/test_cpu_ggn_reference.py derives it by hand) — under
// GaussNewton the cost falls from 6 to 0 in one step.  GradientDescent, L-BFGS, a prior and a ragged batch throw.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
  static_assert(kJitCostGgn == TOA_JIT_COST_GGN && TOA_JIT_COST_GGN == 5, "the kind's number");
  Context ctx(0);
  const char* quadratic =
      "T r = -p[2]; for (int j = 0; j < 2; ++j) r += p[j] * x[j];\n"
      "c = T(0.5) * p[3] * r * r;\n"
      "if (want_grad) { gs = p[3] * r; hs = p[3]; for (int a = 0; a < 2; ++a) J[a] = p[a]; }\n";
  JitResidual<double> loss(ctx, quadratic, /*n=*/2, /*item_scalars=*/4, 1, 0, TOA_MANIFOLD_EUCLID, kJitCostGgn);
  REQUIRE(loss.stats().num_regs > 0);
  const double items[12] = {1, 0, 1, 4, 0, 1, 2, 1, 2, 0, 2, 1};   // (a0, a1, b, hs) x 3
  const auto cost = loss.bind(1, 3, items);
  std::vector<double> x = {0.0, 0.0};
  Options options;
  options.solver_type = Options::GaussNewton;
  const auto out = Optimize(x, cost, options);
  REQUIRE(out.Succeeded(0));
  REQUIRE(x[0] == 1.0 && x[1] == 2.0);
  REQUIRE(out.final_cost[0] == 0.0);
  REQUIRE(out.final_num_residuals[0] == 1);
  REQUIRE(out.final_hessian.size() == 4 && out.final_hessian[0] == 8.0 && out.final_hessian[3] == 1.0 && out.final_hessian[1] == 0.0 &&
          out.final_hessian[2] == 0.0);
  // refused, each with std::invalid_argument
  bool threw = false;
  Options gd;
  gd.solver_type = Options::GradientDescent;
  try { std::vector<double> x2 = {0.0, 0.0}; (void)Optimize(x2, cost, gd); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  Options lb;
  lb.solver_type = Options::LBFGS;
  try { std::vector<double> x2 = {0.0, 0.0}; (void)Optimize(x2, cost, lb); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  try { const double mu[2] = {0, 0}, W[2] = {1, 1}; auto c2 = loss.bind(1, 3, items); c2.with_prior(mu, W); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  try { (void)loss.bind_ragged({3}, items); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
