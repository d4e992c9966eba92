// L-BFGS through the header-only C++ adaptor: the reference's quartic (tests/unconstrained.cpp:19-42) as run-time text
// (TOA_JIT_COST_GRAD, and differentiated on the device as TOA_JIT_COST) under Options::LBFGS from x0 = 38 -> Succeeded,
// Converged, x = 42 +- 1e-5, in far fewer passes than gradient descent takes; the refusals of the option ranges.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

template <typename F>
static bool refused(F&& f) {
  try { f(); } catch (const std::invalid_argument&) { return true; }
  return false;
}

int main() {
  Context ctx(0);
  const char* with_grad =
      "const T y = x[0] - p[0];\n"
      "c = T(3) * y * y + y * y * y * y - T(2);\n"
      "if (want_grad) { G[0] += T(2) * T(3) * y + T(4) * (y * y * y); }";
  const char* autodiff = "const S y = x[0] - p[0]; c = T(3) * y * y + y * y * y * y - T(2);";
  for (int kind : {TOA_JIT_COST_GRAD, TOA_JIT_COST}) {
    JitResidual<double> loss(ctx, kind == TOA_JIT_COST ? autodiff : with_grad, /*n=*/1, /*item_scalars=*/1, 1, 0, TOA_MANIFOLD_EUCLID, kind);
    const double centre = 42.0;
    const auto cost = loss.bind(1, 1, &centre);
    double x = 38.0;
    Options options;
    options.solver_type = Options::LBFGS;
    options.max_iters = 100;
    options.min_error = 0;   // (the minimum is -2)
    const auto out = Optimize(x, cost, options);
    REQUIRE(out.Succeeded());
    REQUIRE(out.Converged());
    REQUIRE(std::fabs(x - 42.0) < 1e-5);
    REQUIRE(std::fabs(out.final_cost.cost + 2.0) < 1e-9);
    REQUIRE(out.num_iters < 60);
    REQUIRE(out.final_hessian.empty());
    REQUIRE(out.final_cost.num_resisuals == 1);
    // what the adaptor refuses before the library is called
    auto with = [&](auto&& edit) { Options o = options; edit(o); double x2 = 38.0; (void)Optimize(x2, cost, o); };
    REQUIRE(refused([&] { with([](Options& o) { o.lbfgs.history = 0; }); }));
    REQUIRE(refused([&] { with([](Options& o) { o.lbfgs.history = 17; }); }));
    REQUIRE(refused([&] { with([](Options& o) { o.lbfgs.c1 = 0.0f; }); }));
    REQUIRE(refused([&] { with([](Options& o) { o.lbfgs.c1 = 1.0f; }); }));
    REQUIRE(refused([&] { with([](Options& o) { o.lbfgs.shrink = 1.0f; }); }));
    REQUIRE(refused([&] { with([](Options& o) { o.grad_clipping = 0.5f; }); }));
    REQUIRE(refused([&] { with([](Options& o) { o.max_duration_ms = 5.0f; }); }));
    // ... and a history of one pair still gets there
    double x1 = 38.0;
    Options one = options;
    one.lbfgs.history = 1;
    const auto out1 = Optimize(x1, cost, one);
    REQUIRE(out1.Converged());
    REQUIRE(std::fabs(x1 - 42.0) < 1e-5);
  }
  {   // a residual model under L-BFGS: refused by the library
    JitResidual<double> res(ctx, "r[0] = x[0] - p[0];", 1, 1);
    const double v = 1.0;
    const auto cost = res.bind(1, 1, &v);
    Options o;
    o.solver_type = Options::LBFGS;
    REQUIRE(refused([&] { double x = 0.0; (void)Optimize(x, cost, o); }));
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
