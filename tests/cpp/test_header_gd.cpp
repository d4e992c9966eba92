// Gradient descent through the header-only C++ adaptor, the way the reference's own test calls it
// (tests/unconstrained.cpp:19-42): a scalar cost with a hand-filled gradient, Options::GradientDescent, lr = 0.01,
// 1000 iterations, min_error = min_rerr_dec = 0 -> Succeeded, Converged, x = 42 +- 1e-5.  Here the cost is run-time text
// (TOA_JIT_COST_GRAD, and the same quartic differentiated on the device as TOA_JIT_COST).  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
  Context ctx(0);
  // p[0] = 42: the quartic's centre, the one data scalar of the one item
  const char* with_grad =
      "const T y = x[0] - p[0];\n"
      "c = T(3) * y * y + y * y * y * y - T(2);\n"
      "if (want_grad) { G[0] += T(2) * T(3) * y + T(4) * (y * y * y); }";
  const char* autodiff = "const S y = x[0] - p[0]; c = T(3) * y * y + y * y * y * y - T(2);";
  for (int kind : {TOA_JIT_COST_GRAD, TOA_JIT_COST}) {
    JitResidual<double> loss(ctx, kind == TOA_JIT_COST ? autodiff : with_grad, /*n=*/1, /*item_scalars=*/1, 1, 0, TOA_MANIFOLD_EUCLID, kind);
    const double centre = 42.0;
    const auto cost = loss.bind(1, 1, &centre);
    double x = 40.1;
    Options options;
    options.solver_type = Options::GradientDescent;
    options.max_iters = 1000;
    options.min_error = 0;
    options.min_rerr_dec = 0;
    options.gd.lr = 0.01f;
    const auto out = Optimize(x, cost, options);
    REQUIRE(out.Succeeded());
    REQUIRE(out.Converged());
    REQUIRE(std::fabs(x - 42.0) < 1e-5);
    REQUIRE(out.final_hessian.empty());
    REQUIRE(out.final_cost.num_resisuals == 1);
    // LM on a scalar cost is refused (optimize.h:41-56)
    Options lm;
    bool threw = false;
    try { double x2 = 40.1; (void)Optimize(x2, cost, lm); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
