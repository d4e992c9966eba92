// Geometry of a row model's LDS stage (row_model.hpp RowModel::pass).  No HIP in here beyond the optional function attributes:
// tests/cpp/test_row_stage_geom.cpp prints it with a plain host compiler, as tests/cpp/test_large_model_geom.cpp sweeps LargeModelGeom.
#pragma once
#if defined(__HIP__) || defined(__HIPCC__)
#define TOA_GEOM_HD __host__ __device__
#else
#define TOA_GEOM_HD
#endif

namespace toa {

// Geometry of a row model's super-step: a function of (sizeof(T), kN, kR, kD) only, evaluated by the device templates and by
// the host launchers (jit.hip, kernels.hpp) alike.
struct RowStageGeom {
  int items2;  // items per super-step, one per lane, when the stage is a RING of `nbuf` regions (the items of the next nbuf - 1
               // super-steps are on their way while this one is consumed): memory-bound passes — a functor with the user's own
               // Jacobian, every cost-only pass
  int nbuf;    // regions of that ring
  int items1;  // ... when it is ONE region (fetch, wait, compute): the accumulate pass of a compute-bound functor (AD), which
               // wants every lane busy more than it wants the prefetch (0 = the model has no such pass)
  int ps;      // item stride in the raw image, elements (>= kD)
  int pss;     // row stride of the SHARED raw image (a model with a shared item table), elements (>= kS); 0 = none
  int rsp;     // row stride of the [J | r] image, elements (>= the packed row)
  int bytes;   // the wave's LDS stage
  int table_off;   // where the model's own `extra` bytes begin, behind the regions (AdRowFunctor on a manifold: the Jets of x (+) d)
  // Both images are read and written a ROW (an item) PER LANE: a stride of 16 bytes x an odd number makes every 16-byte access of
  // sixteen consecutive lanes hit sixteen different bank quads (ds_read_b128 / ds_write_b128 without conflicts) and keeps every
  // row 16-byte aligned.
  static TOA_GEOM_HD constexpr int stride16(int elems, int sz) {
    int q = (elems * sz + 15) / 16;
    if (!(q & 1)) ++q;
    return q * 16 / sz;
  }
  // bytes of one region for `it` items: their raw image — the private one and, behind it, the rows of the shared table —, then
  // the [J | r] image over both
  static TOA_GEOM_HD constexpr int region(int it, int ps, int rsp, int kR, int sz, int pss = 0) {
    const int raw = it * (ps + pss) * sz, img = ((it * kR + 3) & ~3) * rsp * sz;
    return (raw > img ? raw : img);
  }
  // What a wave's stage may take.  With `waves` = 2 workgroups of four waves on a compute unit a wave has 160 KiB / 8 = 20 KiB of
  // LDS, with 3 (twelve waves) 13.3 KiB; the part of its carve that is alive during a pass (x, g, the diagonal, the last step, the
  // memo's x, the state and option blocks) takes 5 x 64 scalars + ~0.5 KiB of that.
  static TOA_GEOM_HD constexpr int budget(int sz, int waves) { return 160 * 1024 / (4 * waves) - 320 * sz - 512; }
  // Ring depth (TOA_ROW_NBUF) and resident workgroups per compute unit the geometry is sized for (TOA_ROW_WAVES): A/B arms of
  // the run-time build (profiles/r06_ab_log.md); jit.hip reads the same two values out of $TOA_JIT_FLAGS for its LDS sizing.
#ifndef TOA_ROW_NBUF
#define TOA_ROW_NBUF 2
#endif
#ifndef TOA_ROW_WAVES
#define TOA_ROW_WAVES 2
#endif
  static TOA_GEOM_HD constexpr RowStageGeom make(int sz, int n, int kR, int kD, bool compute_bound, int nbuf = TOA_ROW_NBUF,
                                                        int waves = TOA_ROW_WAVES, int extra = 0, int kS = 0) {
    const int rem = n & 15;
    const bool thin = n >= 16 && rem + 1 <= 4;
    const int nbm = thin ? (n >> 4) : (n + 16) / 16;
    const int rs = thin ? 16 * nbm + rem + 1 : nbm * ((n + nbm) / nbm);
    RowStageGeom g{};
    g.rsp = stride16(rs, sz);
    g.ps = kD > 0 ? stride16(kD, sz) : 0;
    g.pss = kS > 0 ? stride16(kS, sz) : 0;
    const int itmax = 64 / kR;           // rows of a super-step <= 64
    const int bud = budget(sz, waves) - extra;
    g.nbuf = nbuf;
    int it = itmax;                      // the largest multiple of 4 (one Gram step = four rows) whose ring fits; else 2, 1
    if (it >= 4) it &= ~3;
    while (it > 1 && g.nbuf * region(it, g.ps, g.rsp, kR, sz, g.pss) > bud) it = it > 4 ? it - 4 : it >> 1;
    g.items2 = it;
    g.bytes = g.nbuf * region(it, g.ps, g.rsp, kR, sz, g.pss);
    g.items1 = 0;
    if (compute_bound) {
      it = itmax;
      if (it >= 4) it &= ~3;
      while (it > 1 && region(it, g.ps, g.rsp, kR, sz, g.pss) > bud) it = it > 4 ? it - 4 : it >> 1;
      g.items1 = it;
      if (region(it, g.ps, g.rsp, kR, sz, g.pss) > g.bytes) g.bytes = region(it, g.ps, g.rsp, kR, sz, g.pss);
    }
    g.bytes = (g.bytes + 15) & ~15;
    g.table_off = g.bytes;
    g.bytes += (extra + 15) & ~15;
    return g;
  }
};

}  // namespace toa
