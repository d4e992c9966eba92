// Numerical differentiation and the gradient checker through the header-only C++ adaptor, the way the reference's own tests
// call them: tests/diff.cpp:19-57 (CreateNumDiffFunc1: g == 2 * res for r = 2 (x - y), Method::kCentral and the default step)
// and tests/check_gradient.cpp:18-32 (diag(3, 2) x - 2 with a hand-written Jacobian at (1.4, 7.2) passes CheckResidualsGradient
// with its defaults).  The bodies are run-time text.  Needs a GPU to run; compiles with plain g++.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static_assert(diff::kForward == 0 && diff::kCentral == 1 && diff::kFastCentral == 2, "diff/num_diff.h:20-52");
static_assert(sizeof(toa_jit_spec) == 8 * 4 + sizeof(char*) + 6 * 4, "toa_jit_spec keeps its size");
static_assert(TOA_ABI_VERSION == 7, "additive change");

int main() {
  Context ctx(0);
  {
    // tests/check_gradient.cpp: one item of two residuals, the Jacobian written by hand
    const char* body =
        "r[0] = T(3) * x[0] - T(2); r[1] = T(2) * x[1] - T(2);\n"
        "if (want_grad) { J[0][0] = T(3); J[0][1] = T(0); J[1][0] = T(0); J[1][1] = T(2); }";
    JitResidual<double> res(ctx, body, /*n=*/2, /*item_scalars=*/0, /*residuals_per_item=*/2, 0, TOA_MANIFOLD_EUCLID, TOA_JIT_ACCUMULATE);
    const auto model = res.bind(1, 1, nullptr);
    const std::vector<double> x = {1.4, 7.2};
    const GradientCheck chk = diff::CheckGradient(model, x);
    REQUIRE(chk.all());
    REQUIRE(chk.max_dist_g[0] < 1e-5 && chk.max_dist_H[0] < 1e-5);
    for (diff::Method m : {diff::kForward, diff::kFastCentral}) REQUIRE(diff::CheckGradient(model, x, 0.0, m, true).all());
    // the same residuals with a wrong sign in the Jacobian do not pass
    const char* wrong =
        "r[0] = T(3) * x[0] - T(2); r[1] = T(2) * x[1] - T(2);\n"
        "if (want_grad) { J[0][0] = T(3); J[0][1] = T(0); J[1][0] = T(0); J[1][1] = T(-2); }";
    JitResidual<double> bad(ctx, wrong, 2, 0, 2, 0, TOA_MANIFOLD_EUCLID, TOA_JIT_ACCUMULATE);
    REQUIRE(!diff::CheckGradient(bad.bind(1, 1, nullptr), x).all());
  }
  {
    // tests/diff.cpp:19-32 as a solve: r = 2 (x - y) differentiated by central differences reaches y
    const char* body = "for (int k = 0; k < 3; ++k) r[k] = T(2) * (x[k] - p[k]);";
    JitResidual<double> res(ctx, body, 3, 3, 3, 0, TOA_MANIFOLD_EUCLID, TOA_JIT_RESIDUAL, std::string(), 0, diff::to_pod(diff::kCentral));
    const double y[3] = {0.25, -0.5, 0.75};
    const auto model = res.bind(1, 1, y);
    std::vector<double> x = {0, 0, 0};
    const auto out = Optimize(x, model);
    REQUIRE(out.Succeeded(0));
    for (int k = 0; k < 3; ++k) REQUIRE(std::fabs(x[k] - y[k]) < 1e-5);
    // host controls are refused before any launch
    Options o;
    o.max_duration_ms = 10.0;
    bool threw = false;
    try { (void)Optimize(x, model, o); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
