// A run-time model beyond 63 parameters through the header-only C++ adaptor: JitResidual(..., large_n = true).  The DenseRow residual
// a.x + 0.1 sin(a.x) - b with its own Jacobian rows at n = 72, three problems of 200 rows whose b is made from a known x*: the solve
// lands on x*; without large_n the same model is refused, and so is the stepping Optimizer.  Needs a GPU to run; compiles with plain g++.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static_assert(TOA_ABI_VERSION == 7, "additive change");
static_assert(sizeof(toa_jit_spec) == 8 * sizeof(int32_t) + sizeof(const char*) + 6 * sizeof(int32_t), "toa_jit_spec keeps its size");

int main() {
  Context ctx(0);
  const int P = 3, n = 72, m = 200;
  const std::string N = std::to_string(n);
  const std::string body = "T t = x[0] * p[0];\nfor (int j = 1; j < " + N + "; ++j) t += x[j] * p[j];\nr[0] = t + T(0.1) * sin(t) - p[" + N + "];\n"
                           "if (want_grad) { const T sc = T(1) + T(0.1) * cos(t); for (int j = 0; j < " + N + "; ++j) J[0][j] = sc * p[j]; }";
  // rows a_i from a small generator, b_i = a_i.x* + 0.1 sin(a_i.x*): x* has zero residual
  unsigned long long s = 88172645463325252ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return double(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
  std::vector<double> data(size_t(P) * m * (n + 1)), xs(size_t(P) * n), x(size_t(P) * n);
  for (int p = 0; p < P; ++p) {
    for (int j = 0; j < n; ++j) { xs[size_t(p) * n + j] = 0.5 * rnd(); x[size_t(p) * n + j] = xs[size_t(p) * n + j] + 0.05 * rnd(); }
    for (int i = 0; i < m; ++i) {
      double* row = &data[(size_t(p) * m + i) * (n + 1)];
      double t = 0;
      for (int j = 0; j < n; ++j) { row[j] = rnd(); t += row[j] * xs[size_t(p) * n + j]; }
      row[n] = t + 0.1 * std::sin(t);
    }
  }
  {
    bool threw = false;   // without large_n: one wavefront per problem, 63 parameters at most
    try { JitResidual<double> small(ctx, body, n, n + 1, 1, 0, TOA_MANIFOLD_EUCLID, TOA_JIT_ACCUMULATE); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
  }
  JitResidual<double> res(ctx, body, n, /*item_scalars=*/n + 1, 1, 0, TOA_MANIFOLD_EUCLID, TOA_JIT_ACCUMULATE, std::string(), 0, TOA_DIFF_DEFAULT, 0.f,
                          /*large_n=*/true);
  REQUIRE(res.large_n());
  const auto model = res.bind(P, m, data.data());
  Options o;
  const BatchOutput out = Optimize(x, model, o);
  for (int p = 0; p < P; ++p) {
    REQUIRE(out.Succeeded(size_t(p)) && out.final_num_residuals[p] == m);
    double worst = 0;
    for (int j = 0; j < n; ++j) worst = std::fmax(worst, std::fabs(x[size_t(p) * n + j] - xs[size_t(p) * n + j]));
    REQUIRE(worst < 1e-6);
  }
  {
    bool threw = false;   // no stepping form
    try { Optimizer<double, JitModel<double>> opt(x, model, o); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
