// RowStageGeom::make (csrc/row_stage_geom.hpp), the LDS geometry of RowModel::pass, printed with a plain host compiler over the grid
//   sz in {4, 8} x n in {1, 4, 12, 13, 16, 50, 63} x kR in {1, 2, 8} x kD in {0, 1, 51} x kS in {0, 1, 3, 4, 5, 51, 130, 512} x compute_bound in {0, 1}
// one line per cell:  sz n kR kD kS compute_bound : items2 nbuf items1 ps pss rsp bytes table_off
// tests/test_cpu_shared.py compares the lines with the numpy restatement (tests/shared_reference.py) and, for kS = 0, with
// tests/golden/row_stage_geom_parent.json — the lines this same program printed when it was compiled against the header of the commit
// before shared item tables, which has no kS: -DROW_STAGE_GEOM_NO_SHARED walks kS = 0 only and calls make without it, and
// -DROW_STAGE_GEOM_HEADER="<path>" names that header.
#include <cstdio>
#include <initializer_list>

#ifndef ROW_STAGE_GEOM_HEADER
#define ROW_STAGE_GEOM_HEADER "../../tinyopt_amd/csrc/row_stage_geom.hpp"
#endif
#include ROW_STAGE_GEOM_HEADER

using toa::RowStageGeom;

int main() {
  for (int sz : {4, 8})
    for (int n : {1, 4, 12, 13, 16, 50, 63})
      for (int kR : {1, 2, 8})
        for (int kD : {0, 1, 51})
          for (int kS : {0, 1, 3, 4, 5, 51, 130, 512})
            for (int cb : {0, 1}) {
#ifdef ROW_STAGE_GEOM_NO_SHARED
              if (kS != 0) continue;
              const RowStageGeom g = RowStageGeom::make(sz, n, kR, kD, cb != 0, 2, 2, 0);
              const int pss = 0;
#else
              const RowStageGeom g = RowStageGeom::make(sz, n, kR, kD, cb != 0, 2, 2, 0, kS);
              const int pss = g.pss;
#endif
              std::printf("%d %d %d %d %d %d : %d %d %d %d %d %d %d %d\n", sz, n, kR, kD, kS, cb, g.items2, g.nbuf, g.items1, g.ps, pss, g.rsp, g.bytes,
                          g.table_off);
            }
  return 0;
}
