// Eval / CalculateJac of a run-time model (the reference's diff/auto_diff.h:14-138; with a numeric functor its NumEval /
// EstimateNumJac, diff/num_diff.h:56-126): the residuals and the Jacobian ROWS of a batch, written out instead of reduced.
//
//   res [P][m]      m = items x kR; an item's kR rows are consecutive (the row order of accumulate_kernel)
//   J   [P][m][n]   row-major; over the TANGENT on a manifold (auto_diff.h:31-39)
//
// RF is the row functor the model already has (UserFunctor with its own Jacobian, AdRowFunctor, NumRowFunctor): "fill r[q] and
// J[q][a] for one item on one lane".  Nothing is reduced over a problem's items, so the unit of work is a (problem, range of
// super-steps) pair, dealt to the wavefronts grid-stride: one problem of 20 000 items fills the device as 12 500 problems do.
//
// One super-step of IT items (one per lane, ROWS = IT x kR rows):
//   HBM -> LDS     the items by RowModel's LDS-DMA pieces (row_model.hpp dma_issue: lane-linear, 1 KiB per instruction), item i at
//                  i x PS elements; x from the wave's own copy (and, on a manifold, the Jets of x (+) d built once per problem)
//   lane i         runs the functor on item i; its residuals go out straight from the registers
//   [J] -> LDS     the rows DENSE, row rho at rho x n scalars, over the raw items (every lane has consumed its own by then).  The
//                  super-step's rows are ONE contiguous run of ROWS x n scalars in memory whose first byte is 16-byte aligned only
//                  by luck (a problem's J starts at p x m x n x sizeof(T)): the image starts `ph` = (address of the run) mod 16
//                  bytes into the region, so a 16-byte piece that is aligned in memory is aligned in LDS too
//   LDS -> HBM     lane-linear 16-byte reads of the image, 16-byte stores over the aligned interior of the run (1 KiB per wave
//                  instruction); the at most 12 bytes in front of and behind it as single scalars.  Nothing outside the run is
//                  written.
// Dense, not padded: the way out needs no gather, and the row writes are single-scalar LDS stores at a stride of n dwords (fp64:
// 2 n) over 32 banks — gcd(stride, 32) lanes of a 32-lane group share a bank: free at odd n, two-way at n = 6 and n = 50 (which a
// 4-byte LDS store absorbs), but 16-way at n = 16 / 48 and 32-way at n = 32 in fp32, and at half those widths in fp64.  Measured at
// n = 6, 32 and 50; the padded image, which would spare the bad widths their conflicts, was not built.
// One region per wave (fetch, wait, compute, copy out): the other waves of the compute unit cover the round trip.
//
// WANT_J = false runs the body cost-only on plain T (eval_manual<false>): no Jets, no differences, no image.
#pragma once
#include "kernels.hpp"

namespace toa {

// A wave's LDS for eval_rows_kernel: a function of (sizeof(T), kN, kR, kD, the functor's table bytes, WANT_J) only.
struct EvalRowsGeom {
  int items;       // items of a super-step, one per lane
  int region;      // bytes of the raw items / of the J image laid over them
  int x_off;       // the wave's copy of x (64 scalars)
  int table_off;   // the Jets of x (+) d (AdRowFunctor on a manifold)
  int bytes;       // all of it
  // eight waves on a compute unit (two workgroups): 160 KiB / 8
  static constexpr int kBudget = 20 * 1024;
  static __host__ __device__ constexpr int region_bytes(int it, int sz, int n, int kR, int kD, bool want_j) {
    const int ps = kD > 0 ? RowStageGeom::stride16(kD, sz) : 0;
    const int raw = it * ps * sz;                                       // (a multiple of 16)
    const int img = want_j ? ((15 + it * kR * n * sz + 15) & ~15) : 0;  // the image starts up to 15 bytes in
    const int r = raw > img ? raw : img;
    return r > 16 ? r : 16;
  }
  static __host__ __device__ constexpr EvalRowsGeom make(int sz, int n, int kR, int kD, int table, bool want_j) {
    EvalRowsGeom g{};
    const int fixed = 64 * sz + ((table + 15) & ~15);
    int it = 64 / kR;
    while (it > 1 && region_bytes(it, sz, n, kR, kD, want_j) + fixed > kBudget) --it;
    g.items = it;
    g.region = region_bytes(it, sz, n, kR, kD, want_j);
    g.x_off = g.region;
    g.table_off = g.x_off + 64 * sz;
    g.bytes = g.region + fixed;
    return g;
  }
};

// The compile-time geometry of one instantiation.  The host does not restate it: the generated source of the code object exports
// kBytes / kItems of its two instantiations in a device array (toa_eval_geom, jit.hip ensure_eval) and the launcher reads them back.
template <typename T, typename RF, int MANIFOLD, bool WANT_J>
struct EvalRowsTraits {
  static constexpr int kN = RF::kN, kR = RF::kR, kD = RF::kD, kH = RF::kH;
  static_assert(kN >= 1 && kN <= 63 && kR >= 1 && kR <= 8, "one wavefront per problem's row block");
  // the row model of this width (DenseRowLayout::make): its LDS-DMA pieces, its item stride, its register / LDS choice for the item
  static constexpr int kRem = kN & 15;
  static constexpr bool kThin = kN >= 16 && kRem + 1 <= 4;
  using RM = RowModel<T, kThin ? (kN >> 4) : (kN + 16) / 16, kThin ? kRem + 1 : 0, RF, MANIFOLD, false>;
  static constexpr int kTable = WANT_J ? RM::kTableBytes : 0;
  static constexpr EvalRowsGeom G = EvalRowsGeom::make(int(sizeof(T)), kN, kR, kD, kTable, WANT_J);
  static constexpr int kBytes = G.bytes, kItems = G.items;
};

template <typename T, typename RF, int MANIFOLD, bool WANT_J>
__global__ void __launch_bounds__(256) eval_rows_kernel(const void* data_, const void* x_, long long P, int num_items, void* res_,
                                                        void* J_, int ss_per_unit TOA_RAGGED_KARG) {
  using TR = EvalRowsTraits<T, RF, MANIFOLD, WANT_J>;
  using RM = typename TR::RM;
  constexpr int kN = TR::kN, kR = TR::kR, kD = TR::kD, kH = TR::kH;
  constexpr int XD = RM::kXdim ? RM::kXdim : kN;   // stored scalars of x
  constexpr int kTable = TR::kTable;
  constexpr EvalRowsGeom G = TR::G;
  constexpr int IT = G.items, ROWS = IT * kR, PS = RM::PS;
  constexpr int PFV = kD > 0 ? (IT * int(RM::kPsBytes) + 1023) / 1024 : 0;   // 1 KiB pieces of a super-step's raw image
  constexpr unsigned kSsBytes = unsigned(IT) * RM::kItemBytes;               // a super-step's items in memory
  static_assert(IT >= 1 && ROWS <= 64 && G.region % 16 == 0 && IT * PS * int(sizeof(T)) <= G.region, "geometry");
  static_assert(!WANT_J || 15 + ROWS * kN * int(sizeof(T)) <= G.region, "geometry");
  typedef unsigned V16 __attribute__((ext_vector_type(4)));

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  unsigned char* const stg = reinterpret_cast<unsigned char*>(__builtin_assume_aligned(smem + size_t(wave) * size_t(G.bytes), 16));
  T* const xs = reinterpret_cast<T*>(stg + G.x_off);
  const unsigned lds0 = unsigned(reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char*)(stg)));
  const T* const X = static_cast<const T*>(x_);
  const T* const data = static_cast<const T*>(data_);
  T* const R = static_cast<T*>(res_);
  T* const Jg = static_cast<T*>(J_);
  const size_t m = size_t(num_items) * kR;
  const long long nss = ((long long)num_items + IT - 1) / IT;          // super-steps of a problem
  const long long upp = (nss + ss_per_unit - 1) / ss_per_unit;         // work units of a problem
  const long long units = P * upp;
  long long pcur = -1;
  for (long long u = (long long)blockIdx.x * 4 + wave; u < units; u += (long long)gridDim.x * 4) {
    const long long p = u / upp;
    const int ss0 = int(u - p * upp) * ss_per_unit;
#ifdef TOA_RAGGED
    // ragged batches (ragged.hpp): num_items is the LARGEST count — it sizes the units — and the problem's own range comes from the
    // offsets; a unit that starts beyond its problem's last super-step has nothing to do.  Outputs are concatenated like the items.
    const RaggedRange rr = ragged_range(rag, p);
    const int nit = rr.count;
    const long long nss_p = ((long long)nit + IT - 1) / IT;
    if (ss0 >= nss_p) continue;
    const int ss1 = int(nss_p < (long long)ss0 + ss_per_unit ? nss_p : (long long)ss0 + ss_per_unit);
    const T* const d = static_cast<const T*>(rag.header) + size_t(p) * kH;
    const T* const itemsp = data + size_t(rr.first) * kD;
    const size_t row0 = size_t(rr.first) * kR;
#else
    const int nit = num_items;
    const int ss1 = int(nss < (long long)ss0 + ss_per_unit ? nss : (long long)ss0 + ss_per_unit);
    const T* const d = data + size_t(p) * (size_t(kH) + size_t(num_items) * kD);
    const T* const itemsp = d + kH;
    const size_t row0 = size_t(p) * m;
#endif
    if (p != pcur) {   // x, and the Jets of x (+) d: once per problem per wave
      wave_sync();
      xs[lane] = lane < XD ? X[size_t(p) * XD + lane] : T(0);
      wave_sync();
      if constexpr (kTable > 0) RF::build_table(xs, reinterpret_cast<typename RF::TabJet*>(stg + G.table_off), lane);
      pcur = p;
    }
    const i32x4 rsrc = make_rsrc(itemsp, unsigned(nit) * unsigned(kD) * unsigned(sizeof(T)));
    for (int ss = ss0; ss < ss1; ++ss) {
      // ---- the items of the super-step -> the region (its last readers, the previous copy-out, have their data: lgkmcnt)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if constexpr (PFV > 0) {
        RM::template dma_issue<IT, 0, PFV>(rsrc, lane, unsigned(__builtin_amdgcn_readfirstlane(int(unsigned(ss) * kSsBytes))), lds0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      wave_sync();
      // ---- the functor, one item per lane
      const int item = ss * IT + lane;
      const bool valid = lane < IT && item < nit;
      T rv[kR];
      T Jv[WANT_J ? kR : 1][kN];
      if (valid) {
        const T* const pi = reinterpret_cast<const T*>(stg) + size_t(lane) * PS;
        T pl[RM::kPRegs ? (kD ? kD : 1) : 1];
        if constexpr (RM::kPRegs) RM::template lds_read_row<kD>(pl, pi);
        const T* const pp = RM::kPRegs ? pl : pi;
        if constexpr (kTable > 0) {
          RF::template eval_manual_tab<true>(xs, reinterpret_cast<const typename RF::TabJet*>(stg + G.table_off), d, pp, rv, Jv);
        } else if constexpr (RM::kTableBytes > 0) {
          RF::template eval_manual_tab<false>(xs, nullptr, d, pp, rv, static_cast<T(*)[kN]>(nullptr));
        } else {
          if constexpr (WANT_J) RF::template eval_manual<true>(xs, d, pp, rv, Jv);
          else RF::template eval_manual<false>(xs, d, pp, rv, static_cast<T(*)[kN]>(nullptr));
        }
        if (R) {   // consecutive lanes, consecutive scalars
          T* const ro = R + row0 + size_t(item) * kR;
#pragma unroll
          for (int q = 0; q < kR; ++q) ro[q] = rv[q];
        }
      }
      if constexpr (WANT_J) {
        // ---- [J], dense, over the raw items; the image starts where a 16-byte boundary of memory is one of LDS
        const int rows_here = int(min((long long)IT, (long long)nit - (long long)ss * IT)) * kR;
        T* const g0 = Jg + (row0 + size_t(ss) * ROWS) * kN;       // the super-step's run in memory
        const unsigned nbytes = unsigned(rows_here) * unsigned(kN) * unsigned(sizeof(T));
        const unsigned ph = unsigned(__builtin_amdgcn_readfirstlane(int(unsigned(reinterpret_cast<size_t>(g0)) & 15u)));
        unsigned char* const img = stg + ph;
        wave_sync();   // (every lane has read its item)
        if (valid) {
#pragma unroll
          for (int q = 0; q < kR; ++q) {
            T* const row = reinterpret_cast<T*>(img) + size_t(lane * kR + q) * kN;
#pragma unroll
            for (int a = 0; a < kN; ++a) row[a] = Jv[q][a];
          }
        }
        wave_sync();
        // ---- the run: [0, head) scalars, [head, head + inter) 16-byte pieces, [head + inter, nbytes) scalars
        unsigned head = (16u - ph) & 15u;
        if (head > nbytes) head = nbytes;
        const unsigned inter = (nbytes - head) & ~15u, t0 = head + inter;
        unsigned char* const gb = reinterpret_cast<unsigned char*>(g0);
        for (unsigned o = unsigned(lane) * 16u; o < inter; o += 1024u)
          *reinterpret_cast<V16*>(gb + head + o) = *reinterpret_cast<const V16*>(img + head + o);
        if (unsigned(lane) * unsigned(sizeof(T)) < head) g0[lane] = reinterpret_cast<const T*>(img)[lane];
        if (unsigned(lane) * unsigned(sizeof(T)) < nbytes - t0)
          reinterpret_cast<T*>(gb + t0)[lane] = reinterpret_cast<const T*>(img + t0)[lane];
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

}  // namespace toa
