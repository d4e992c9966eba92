// LDS geometry of large_model_rows_kernel (large_model_rows.hpp): a function of (sizeof(T), n, kR, kD, WANT_J) and an LDS budget
// only, evaluated by the device template and by the host launcher (jit.hip) alike, as RowStageGeom / EvalRowsGeom are.  No HIP in
// here: tests/cpp/test_large_model_geom.cpp sweeps it with a plain host compiler.
//
// A workgroup of four waves:
//   [0, x_bytes)                    x, ONE copy for the workgroup (n scalars)
//   per wave w, at wave_off + w * wave_bytes:
//     [raw_off, raw_off + raw_bytes)   the raw items of a super-step, item i at i * ps scalars
//     [img_off, img_off + img_bytes)   the J image, row rho at rho * n scalars: item i's kR rows are rows i * kR .. i * kR + kR - 1
//     [r_off, r_off + r_bytes)         the residuals of the super-step's rows (every lane of the J^T r sum reads all of them)
// The image is NOT laid over the raw items: a body with its own Jacobian reads p[j] and writes J[q][j] in the same loop.
// One item per lane, so at most 64 / kR items; at large n fewer fit (n = 1024 in fp32: 4 KiB of J per row) and the other lanes idle.
#pragma once

namespace toa {

struct LargeModelGeom {
  int items;      // items of a super-step, one per lane; 0 = not even one item fits the budget
  int rows;       // items * kR (<= 64)
  int ps;         // item stride of the raw image, scalars (>= kD; its bytes an odd multiple of 16)
  int x_bytes;    // the workgroup's copy of x
  int raw_off, raw_bytes, img_off, img_bytes, r_off, r_bytes;   // inside a wave's region
  int wave_off, wave_bytes;
  int bytes;      // the workgroup's dynamic LDS

  static constexpr int kWaves = 4;
  // the default limit of a workgroup's dynamic LDS: two workgroups on a compute unit of 160 KiB, no attribute to raise
  static constexpr int kBudget = 64 * 1024;

  static constexpr int align16(int b) { return (b + 15) & ~15; }
  // item stride: 16 bytes x an odd number (rows 16-byte aligned, sixteen consecutive lanes on sixteen different bank quads)
  static constexpr int item_stride(int kD, int sz) {
    if (kD <= 0) return 0;
    int q = (kD * sz + 15) / 16;
    if (!(q & 1)) ++q;
    return q * 16 / sz;
  }
  static constexpr long long wave_need(int it, int sz, int n, int kR, int kD, bool want_j) {
    const long long raw = (long long)it * item_stride(kD, sz) * sz;
    const long long img = want_j ? (((long long)it * kR * n * sz + 15) & ~15ll) : 0;
    const long long r = want_j ? (((long long)it * kR * sz + 15) & ~15ll) : 0;
    return (raw > 16 ? raw : 16) + img + r;
  }
  static constexpr LargeModelGeom make(int sz, int n, int kR, int kD, bool want_j, int budget = kBudget) {
    LargeModelGeom g{};
    g.ps = item_stride(kD, sz);
    g.x_bytes = align16(n * sz);
    g.wave_off = g.x_bytes;
    int it = 64 / kR;
    while (it >= 1 && g.x_bytes + kWaves * wave_need(it, sz, n, kR, kD, want_j) > budget) --it;
    if (it < 1) return g;   // items = 0: does not fit
    g.items = it;
    g.rows = it * kR;
    g.raw_off = 0;
    g.raw_bytes = it * g.ps * sz > 16 ? it * g.ps * sz : 16;
    g.img_off = g.raw_bytes;
    g.img_bytes = want_j ? align16(it * kR * n * sz) : 0;
    g.r_off = g.img_off + g.img_bytes;
    g.r_bytes = want_j ? align16(it * kR * sz) : 0;
    g.wave_bytes = g.raw_bytes + g.img_bytes + g.r_bytes;
    g.bytes = g.x_bytes + kWaves * g.wave_bytes;
    return g;
  }
};

}  // namespace toa
