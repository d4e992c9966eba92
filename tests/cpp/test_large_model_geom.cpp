// LargeModelGeom (csrc/large_model_geom.hpp), the LDS geometry of large_model_rows_kernel, swept with a plain host compiler:
// element size 4 and 8, n = 1 .. 1024 (fp64: 512), kR = 1 .. 8, kD in {0, 1, n + 1, 2048}, with and without the J image.
// Either the geometry says "does not fit" (items = 0) — and then not even one item fits the budget — or items >= 1, rows =
// items x kR <= 64, every region 16-byte aligned and inside the budget, the J image beside (not over) the raw items and large
// enough for its rows, the raw image large enough for its items, and one more item would not fit.
// Prints every violation and, last, "checked <count> violations <count>".
#include <cstdio>
#include <initializer_list>

#include "../../tinyopt_amd/csrc/large_model_geom.hpp"

using toa::LargeModelGeom;

int main() {
  long checked = 0, bad = 0;
  auto fail = [&](const char* what, int sz, int n, int kR, int kD, bool wj) {
    std::printf("VIOLATION %s: sz=%d n=%d kR=%d kD=%d want_j=%d\n", what, sz, n, kR, kD, int(wj));
    ++bad;
  };
  for (int sz = 4; sz <= 8; sz += 4)
    for (int n = 1; n <= (sz == 4 ? 1024 : 512); ++n)
      for (int kR = 1; kR <= 8; ++kR)
        for (int kDi = 0; kDi < 4; ++kDi)
          for (int wj = 0; wj < 2; ++wj) {
            const int kD = kDi == 0 ? 0 : kDi == 1 ? 1 : kDi == 2 ? n + 1 : 2048;
            const bool want_j = wj != 0;
            const LargeModelGeom g = LargeModelGeom::make(sz, n, kR, kD, want_j);
            ++checked;
            auto F = [&](const char* w) { fail(w, sz, n, kR, kD, want_j); };
            const long long one = g.x_bytes + 4 * LargeModelGeom::wave_need(1, sz, n, kR, kD, want_j);
            if (g.items == 0) {
              if (one <= LargeModelGeom::kBudget) F("refused although one item fits");
              continue;
            }
            if (g.items < 1 || g.items > 64 / kR || g.rows != g.items * kR || g.rows > 64) F("items / rows");
            if (g.ps < kD || (kD > 0 && ((g.ps * sz) % 16 != 0 || ((g.ps * sz / 16) & 1) == 0))) F("item stride");
            if (g.x_bytes < n * sz) F("x too small");
            if (g.raw_bytes < g.items * g.ps * sz) F("raw image too small");
            if (want_j && g.img_bytes < g.rows * n * sz) F("J image too small");
            if (!want_j && g.img_bytes != 0) F("J image without J");
            // the regions of a wave do not overlap, nor do the waves, nor the waves and x
            if (g.raw_off < 0 || g.img_off < g.raw_off + g.raw_bytes) F("J image over the raw items");
            if (g.r_off < g.img_off + g.img_bytes) F("residuals over the J image");
            if (want_j && g.r_bytes < g.rows * sz) F("residuals too small");
            if (g.wave_bytes < g.r_off + g.r_bytes) F("a wave's region too small");
            if (g.wave_off < g.x_bytes) F("waves over x");
            if (g.bytes < g.wave_off + 4 * g.wave_bytes) F("workgroup too small");
            if (g.bytes > LargeModelGeom::kBudget) F("beyond the budget");
            for (int v : {g.x_bytes, g.raw_off, g.raw_bytes, g.img_off, g.img_bytes, g.r_off, g.r_bytes, g.wave_off, g.wave_bytes, g.bytes})
              if (v % 16 != 0) F("not 16-byte aligned");
            if (g.items < 64 / kR && g.x_bytes + 4 * LargeModelGeom::wave_need(g.items + 1, sz, n, kR, kD, want_j) <= LargeModelGeom::kBudget)
              F("one more item would fit");
          }
  std::printf("checked %ld violations %ld\n", checked, bad);
  return bad == 0 ? 0 : 1;
}
