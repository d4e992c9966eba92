// Shared item tables (JitResidual's shared_scalars) through the header-only C++ adaptor: the dyadic quadratic of
// tests/cpp/test_header_ggn.cpp — c = hs (a . x - b)^2 / 2 over three items, whose Newton step from (0, 0) is (1, 2) exactly — with the
// rows a_i in ONE table for two problems and (b, hs) as each item's own scalars; the second problem has b doubled, so its step is
// (2, 4).  Under GaussNewton both costs fall to 0 in one step.  The same body as a residual model inside bounds keeps x in the box.
// GradientDescent, L-BFGS, host controls, the stepping Optimizer, bind / bind_ragged, diff::Eval and diff::CheckGradient throw.  Needs a GPU.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)
#define THROWS(stmt) do { bool threw_ = false; try { stmt; } catch (const std::invalid_argument&) { threw_ = true; } REQUIRE(threw_); } while (0)

int main() {
  static_assert(sizeof(toa_shared) == 32, "toa_shared");
  static_assert(offsetof(toa_jit_spec, shared_scalars) == 52 && offsetof(toa_jit_spec, reserved) == 48 && offsetof(toa_jit_spec, large_n) == 48, "toa_jit_spec");
  Context ctx(0);
  const char* quadratic =
      "T r = -p[0]; for (int j = 0; j < 2; ++j) r += s[j] * x[j];\n"
      "c = T(0.5) * p[1] * r * r;\n"
      "if (want_grad) { gs = p[1] * r; hs = p[1]; for (int a = 0; a < 2; ++a) J[a] = s[a]; }\n";
  JitResidual<double> loss(ctx, quadratic, /*n=*/2, /*item_scalars=*/2, 1, 0, TOA_MANIFOLD_EUCLID, kJitCostGgn, std::string(), 0, TOA_DIFF_DEFAULT, 0.f,
                           false, /*shared_scalars=*/2);
  REQUIRE(loss.shared_scalars() == 2 && loss.stats().num_regs > 0);
  const double table[6] = {1, 0, 0, 1, 2, 0};                           // a_i, one row per item, for both problems
  const double items[12] = {1, 4, 2, 1, 2, 1, 2, 4, 4, 1, 4, 1};        // (b, hs) x 3, two problems
  const auto cost = loss.bind_shared(2, 3, items, table);
  REQUIRE(cost.has_shared() && cost.shared_pod().rows == 3);
  std::vector<double> x = {0.0, 0.0, 0.0, 0.0};
  std::vector<double> g, H;
  std::vector<double> c;
  Accumulate(cost, x, &g, &H, c);
  REQUIRE(c.size() == 2 && c[0] == 6.0 && c[1] == 24.0);
  REQUIRE(g.size() == 4 && g[0] == -8.0 && g[1] == -2.0 && g[2] == -16.0 && g[3] == -4.0);
  REQUIRE(H.size() == 8 && H[0] == 8.0 && H[3] == 1.0 && H[1] == 0.0 && H[4] == 8.0 && H[7] == 1.0);
  Options options;
  options.solver_type = Options::GaussNewton;
  const auto out = Optimize(x, cost, options);
  REQUIRE(out.Succeeded(0) && out.Succeeded(1));
  REQUIRE(x[0] == 1.0 && x[1] == 2.0 && x[2] == 2.0 && x[3] == 4.0);
  REQUIRE(out.final_cost[0] == 0.0 && out.final_cost[1] == 0.0);
  REQUIRE(out.final_num_residuals[0] == 1);
  REQUIRE(out.final_hessian.size() == 8 && out.final_hessian[0] == 8.0 && out.final_hessian[3] == 1.0 && out.final_hessian[4] == 8.0);
  // a residual model on the same table, inside a box that binds: sqrt(hs) (a . x - b), Jets
  JitResidual<double> fit(ctx, "S z = S(-p[0]); for (int j = 0; j < 2; ++j) z += s[j] * x[j];\nr[0] = z * sqrt(p[1]);", 2, 2, 1, 0, TOA_MANIFOLD_EUCLID,
                          kJitResidual, std::string(), 0, TOA_DIFF_DEFAULT, 0.f, false, 2);
  auto boxed = fit.bind_shared(2, 3, items, table);
  const double lo[4] = {-10, -10, -10, -10}, hi[4] = {0.5, 10, 10, 3};
  boxed.with_bounds(lo, hi);
  std::vector<double> xb = {0.0, 0.0, 0.0, 0.0};
  const auto outb = Optimize(xb, boxed, Options());
  REQUIRE(outb.Succeeded(0) && outb.Succeeded(1));
  REQUIRE(xb[0] == 0.5 && std::fabs(xb[1] - 2.0) < 1e-9 && std::fabs(xb[2] - 2.0) < 1e-9 && xb[3] == 3.0);
  // refused, each with std::invalid_argument
  Options gd, lb, host;
  gd.solver_type = Options::GradientDescent;
  lb.solver_type = Options::LBFGS;
  host.max_duration_ms = 5.0;
  std::vector<double> x2 = {0.0, 0.0, 0.0, 0.0};
  THROWS((void)Optimize(x2, cost, gd));
  THROWS((void)Optimize(x2, cost, lb));
  THROWS((void)Optimize(x2, cost, host));
  THROWS((void)loss.bind(2, 3, items));
  THROWS((void)loss.bind_ragged({3, 3}, items));
  THROWS((void)loss.bind_shared(2, 3, items, nullptr));
  THROWS((void)diff::Eval(boxed, x2));
  THROWS((void)diff::CalculateJac(boxed, x2));
  THROWS((void)diff::CheckGradient(cost, x2));
  THROWS((Optimizer<double, JitModel<double>>(x2, cost)));
  THROWS(JitResidual<double>(ctx, "c = s[0];", 2, 1, 1, 0, TOA_MANIFOLD_EUCLID, kJitCost, std::string(), 0, TOA_DIFF_DEFAULT, 0.f, false, 2));
  THROWS(JitResidual<double>(ctx, "r[0] = s[0];", 2, 1, 1, 0, TOA_MANIFOLD_EUCLID, kJitResidual, std::string(), 0, TOA_DIFF_DEFAULT, 0.f, true, 2));
  THROWS(JitResidual<double>(ctx, "r[0] = s[0];", 2, 1, 1, 0, TOA_MANIFOLD_EUCLID, kJitResidual, std::string(), 0, TOA_DIFF_DEFAULT, 0.f, false, 513));
  JitResidual<double> plain(ctx, "r[0] = x[0] - p[0];", 1, 1);
  THROWS((void)plain.bind_shared(2, 3, items, table));
  REQUIRE(x2[0] == 0.0 && x2[3] == 0.0);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
