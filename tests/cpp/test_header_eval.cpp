// diff::Eval / diff::CalculateJac through the header-only C++ adaptor (the reference's diff/auto_diff.h:14-138, tested in
// tests/diff.cpp:89-111): the circle-fit residual ||p - c||^2 - radius^2 of tests/circle.cpp:32-68 as run-time text, its rows
// against rows written by hand — differentiated on Jets, by central differences, and with its own Jacobian.  Needs a GPU to
// run; compiles with plain g++.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static_assert(TOA_ABI_VERSION == 7, "additive change");

int main() {
  Context ctx(0);
  const char* circle = "const S dx = p[0] - x[0];\nconst S dy = p[1] - x[1];\nr[0] = dx * dx + dy * dy - x[2] * x[2];";
  const char* circle_acc =
      "const T dx = p[0] - x[0], dy = p[1] - x[1];\nr[0] = dx * dx + dy * dy - x[2] * x[2];\n"
      "if (want_grad) { J[0][0] = T(-2) * dx; J[0][1] = T(-2) * dy; J[0][2] = T(-2) * x[2]; }";
  // two problems of five points each; every number a multiple of 1/4, so the hand-written rows are exact
  const int P = 2, items = 5;
  const double pts[P * items * 2] = {1.0, 0.5, -0.25, 2.0, 3.0, -1.5, 0.75, 0.75, -2.0, -0.5,
                                     0.0, 1.25, 2.5, 2.5, -1.0, 0.25, 1.5, -3.0, 0.5, 0.0};
  const std::vector<double> x = {0.5, -0.25, 1.5, -1.0, 0.75, 2.0};
  std::vector<double> r_ref(P * items), J_ref(P * items * 3);
  for (int p = 0; p < P; ++p)
    for (int i = 0; i < items; ++i) {
      const double dx = pts[(p * items + i) * 2] - x[p * 3], dy = pts[(p * items + i) * 2 + 1] - x[p * 3 + 1], rad = x[p * 3 + 2];
      r_ref[p * items + i] = dx * dx + dy * dy - rad * rad;
      J_ref[(p * items + i) * 3 + 0] = -2 * dx;
      J_ref[(p * items + i) * 3 + 1] = -2 * dy;
      J_ref[(p * items + i) * 3 + 2] = -2 * rad;
    }
  {
    JitResidual<double> res(ctx, circle, /*n=*/3, /*item_scalars=*/2);
    const auto model = res.bind(P, items, pts);
    const auto rj = diff::Eval(model, x);
    REQUIRE(rj.first == r_ref);
    REQUIRE(rj.second == J_ref);
    REQUIRE(diff::CalculateJac(model, x) == J_ref);
    const auto r_only = diff::Eval(model, x, false);
    REQUIRE(r_only.first == r_ref && r_only.second.empty());
  }
  {
    JitResidual<double> res(ctx, circle_acc, 3, 2, 1, 0, TOA_MANIFOLD_EUCLID, TOA_JIT_ACCUMULATE);
    const auto rj = diff::Eval(res.bind(P, items, pts), x);
    REQUIRE(rj.first == r_ref && rj.second == J_ref);
  }
  {
    // NumEval: central differences with the default step reproduce the rows of a quadratic to ~h^2 / round-off
    JitResidual<double> res(ctx, circle, 3, 2, 1, 0, TOA_MANIFOLD_EUCLID, TOA_JIT_RESIDUAL, std::string(), 0, diff::to_pod(diff::kCentral));
    const auto rj = diff::Eval(res.bind(P, items, pts), x);
    REQUIRE(rj.first == r_ref);
    for (size_t i = 0; i < J_ref.size(); ++i) REQUIRE(std::fabs(rj.second[i] - J_ref[i]) < 1e-6);
  }
  {
    // refusals: a scalar cost has no rows; a wrong x size throws before any launch
    JitResidual<double> cost(ctx, "const S y = x[0] - p[0]; c = y * y;", 1, 1, 1, 0, TOA_MANIFOLD_EUCLID, TOA_JIT_COST);
    const double one[1] = {1.0};
    bool threw = false;
    try { (void)diff::Eval(cost.bind(1, 1, one), std::vector<double>{0.0}); } catch (const std::exception&) { threw = true; }
    REQUIRE(threw);
    JitResidual<double> res(ctx, circle, 3, 2);
    threw = false;
    try { (void)diff::CalculateJac(res.bind(P, items, pts), std::vector<double>{0.0}); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
