// A multi-output second-order scalar cost (TOA_JIT_COST_GGN_MULTI) through the header-only C++ adaptor: c = (u - b)^T A (u - b) / 2 with
// u = V x, K = 2 outputs per item, over three items with dyadic data whose minimiser is (1, 2) (tests/test_cpu_ggn_multi_reference.py
// has numbers of the same kind): every A = L D L^T has pivots D that are powers of four, so their roots and with them
// H = sum V^T A V = [[8, -1/2], [-1/2, 29/4]] are exact; under GaussNewton the cost falls from 17.5 to 0.  With a
// diagonal prior W = (2, 1) around (1, 2) the minimiser stays and H gains diag(4, 1).  bind_shared is taken too.  GradientDescent, L-BFGS, a loss, a host control,
// bounds and a ragged batch throw.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tinyopt_amd/tinyopt.hpp"

using namespace tinyopt_amd;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::printf("REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
  static_assert(kJitCostGgnMulti == TOA_JIT_COST_GGN_MULTI && TOA_JIT_COST_GGN_MULTI == 6 && TOA_JIT_COST_GGN == 5, "the kind's number");
  Context ctx(0);
  const char* quadratic =
      "T r[2];\n"
      "for (int k = 0; k < 2; ++k) { r[k] = -p[4 + k]; for (int j = 0; j < 2; ++j) r[k] += p[k * 2 + j] * x[j]; }\n"
      "const T t0 = p[6] * r[0] + p[7] * r[1];\n"
      "const T t1 = p[7] * r[0] + p[8] * r[1];\n"
      "c = T(0.5) * (r[0] * t0 + r[1] * t1);\n"
      "if (want_grad) {\n"
      "  gs[0] = t0; gs[1] = t1;\n"
      "  Hs[0][0] = p[6]; Hs[1][0] = p[7]; Hs[1][1] = p[8];\n"
      "  for (int k = 0; k < 2; ++k) for (int a = 0; a < 2; ++a) J[k][a] = p[k * 2 + a];\n"
      "}\n";
  JitResidual<double> loss(ctx, quadratic, /*n=*/2, /*item_scalars=*/9, /*K=*/2, 0, TOA_MANIFOLD_EUCLID, kJitCostGgnMulti);
  REQUIRE(loss.stats().num_regs > 0);
  const double items[27] = {1, 0, 0, 1, 1, 2, 1, 0.5, 4.25, 0, 1, 1, 1, 2, 3, 4, -2, 2, 2, 0, 1, -1, 2, -1, 1, 0, 1};   // (V, b, a00 a10 a11) x 3
  Options options;
  options.solver_type = Options::GaussNewton;
  {
    const auto cost = loss.bind(1, 3, items);
    std::vector<double> x = {0.0, 0.0};
    const auto out = Optimize(x, cost, options);
    REQUIRE(out.Succeeded(0));
    REQUIRE(std::fabs(x[0] - 1.0) < 1e-12 && std::fabs(x[1] - 2.0) < 1e-12);
    REQUIRE(out.final_cost[0] < 1e-20);
    REQUIRE(out.final_num_residuals[0] == 1);
    REQUIRE(out.final_hessian.size() == 4 && out.final_hessian[0] == 8.0 && out.final_hessian[3] == 7.25 && out.final_hessian[1] == -0.5 &&
            out.final_hessian[2] == -0.5);
  }
  {   // with_prior is taken: the ridge term (1/2) |W (x - mu)|^2, still one residual
    const double mu[2] = {1, 2}, W[2] = {2, 1};
    const auto cost = loss.bind(1, 3, items).with_prior(mu, W, 0);
    std::vector<double> x = {0.0, 0.0};
    const auto out = Optimize(x, cost, options);
    REQUIRE(out.Succeeded(0));
    REQUIRE(std::fabs(x[0] - 1.0) < 1e-12 && std::fabs(x[1] - 2.0) < 1e-12);
    REQUIRE(out.final_num_residuals[0] == 1);
    REQUIRE(out.final_hessian.size() == 4 && out.final_hessian[0] == 12.0 && out.final_hessian[3] == 8.25 && out.final_hessian[1] == -0.5);
  }
  // refused, each with std::invalid_argument
  const auto cost = loss.bind(1, 3, items);
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
  try { const double lo[2] = {0, 0}, hi[2] = {1, 1}; auto c2 = loss.bind(1, 3, items); c2.with_bounds(lo, hi); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  try { (void)loss.bind_ragged({3}, items); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  try { auto c2 = loss.bind(1, 3, items); c2.set_loss(TOA_LOSS_HUBER, 1.0); std::vector<double> x2 = {0.0, 0.0}; (void)Optimize(x2, c2, options); }
  catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  Options timed;
  timed.max_duration_ms = 5.0;   // a host control: the kind has no stepping form
  try { std::vector<double> x2 = {0.0, 0.0}; (void)Optimize(x2, cost, timed); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  {   // bind_shared is taken: V in ONE table [items][4] for the batch, (b, A) private; two problems, the second with other targets b
    const char* shared_body =
        "T r[2];\n"
        "for (int k = 0; k < 2; ++k) { r[k] = -p[k]; for (int j = 0; j < 2; ++j) r[k] += s[k * 2 + j] * x[j]; }\n"
        "const T t0 = p[2] * r[0] + p[3] * r[1];\n"
        "const T t1 = p[3] * r[0] + p[4] * r[1];\n"
        "c = T(0.5) * (r[0] * t0 + r[1] * t1);\n"
        "if (want_grad) {\n"
        "  gs[0] = t0; gs[1] = t1;\n"
        "  Hs[0][0] = p[2]; Hs[1][0] = p[3]; Hs[1][1] = p[4];\n"
        "  for (int k = 0; k < 2; ++k) for (int a = 0; a < 2; ++a) J[k][a] = s[k * 2 + a];\n"
        "}\n";
    JitResidual<double> sh(ctx, shared_body, 2, /*item_scalars=*/5, /*K=*/2, 0, TOA_MANIFOLD_EUCLID, kJitCostGgnMulti, std::string(), 0, TOA_DIFF_DEFAULT, 0.f,
                           false, /*shared_scalars=*/4);
    const double table[12] = {1, 0, 0, 1, 0, 1, 1, 1, 2, 0, 1, -1};
    // problem 0: the targets of the private form (minimiser (1, 2)); problem 1: b = V (2, -1) (minimiser (2, -1))
    const double priv[30] = {1, 2, 1, 0.5, 4.25, 2, 3, 4, -2, 2, 2, -1, 1, 0, 1,
                             2, -1, 1, 0.5, 4.25, -1, 1, 4, -2, 2, 4, 3, 1, 0, 1};
    const auto sc = sh.bind_shared(2, 3, priv, table);
    std::vector<double> x = {0.0, 0.0, 0.0, 0.0};
    const auto out = Optimize(x, sc, options);
    REQUIRE(out.Succeeded(0) && out.Succeeded(1));
    REQUIRE(std::fabs(x[0] - 1.0) < 1e-12 && std::fabs(x[1] - 2.0) < 1e-12 && std::fabs(x[2] - 2.0) < 1e-12 && std::fabs(x[3] + 1.0) < 1e-12);
    REQUIRE(out.final_hessian.size() == 8 && out.final_hessian[0] == 8.0 && out.final_hessian[3] == 7.25 && out.final_hessian[4] == 8.0 &&
            out.final_hessian[5] == -0.5);
    threw = false;
    try { (void)sh.bind(2, 3, priv); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
