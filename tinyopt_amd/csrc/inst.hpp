// The entry points of the pre-instantiated kernels: ONE list.  inst.hip is compiled once per (dtype, family) and once per (dtype,
// block count) — __graft_entry__._hip_jobs() — and defines in each translation unit the few functions below that carry its
// -DTOA_INST_DT / -DTOA_INST_NBM in their names; capi.hip reaches them through toa_inst_table.  inst.hip includes this file too:
// the list has C linkage, so a definition there whose parameters differ from its line here does not compile (with C++ linkage
// it would be a second overload, and the mismatch a missing symbol when the library is loaded).
//
// Keys, computed once by the caller: `thin` and the block count NBM = nbm of DenseRowLayout::make(n, m) — for n <= 63 nbm is
// 1 .. 4, and nbm == 4 only with thin == 0, so every (dtag, nbm) has its entry and no lookup can miss; a `thin` the translation
// unit has no instance for is refused inside inst.hip ("bad thin-tail width") —, npad = 16 * ceil(n / 16), and the model tag.
#pragma once
#include "host_launch.hpp"

#define TOA_INST_DECLARE_NBM(DT, NBM)                                                                        \
  int toa_inst_fused_##DT##_##NBM(int thin, toa_handle h, const toa::FusedParams& prm);                       \
  int toa_inst_wide_##DT##_##NBM(int thin, toa_handle h, const toa::FusedParams& prm, int splits);            \
  int toa_inst_accumulate_##DT##_##NBM(int thin, toa_handle h, const toa::AccumArgs& a);
#define TOA_INST_DECLARE(DT)                                                                                  \
  int toa_inst_solve_##DT##_0(int npad, toa_handle h, int n, int64_t P, const void* H, const void* g, double scale, void* dx, int32_t* ok); \
  int toa_inst_inv_cov_##DT##_0(int npad, toa_handle h, int n, int64_t P, const void* H, void* C, int32_t* ok); \
  int toa_inst_misc_fused_##DT##_0(int model, int npad, toa_handle h, const toa::FusedParams& prm);           \
  int toa_inst_misc_wide_##DT##_0(int model, toa_handle h, const toa::FusedParams& prm, int splits);          \
  int toa_inst_misc_accumulate_##DT##_0(int model, toa_handle h, const toa::AccumArgs& a);                    \
  int toa_inst_jetrow_fused_##DT##_0(int n, toa_handle h, const toa::FusedParams& prm);                       \
  int toa_inst_jetrow_wide_##DT##_0(int n, toa_handle h, const toa::FusedParams& prm);                        \
  int toa_inst_jetrow_accumulate_##DT##_0(toa_handle h, const toa::AccumArgs& a);                             \
  int toa_inst_narrow_fused_##DT##_0(int n, toa_handle h, const toa::FusedParams& prm);                       \
  int toa_inst_narrow_jet_fused_##DT##_0(int n, toa_handle h, const toa::FusedParams& prm);   /* (between the two narrow units) */ \
  int toa_inst_narrow_accumulate_##DT##_0(toa_handle h, const toa::AccumArgs& a);                             \
  TOA_INST_DECLARE_NBM(DT, 1) TOA_INST_DECLARE_NBM(DT, 2) TOA_INST_DECLARE_NBM(DT, 3) TOA_INST_DECLARE_NBM(DT, 4)
extern "C" {
TOA_INST_DECLARE(0)
TOA_INST_DECLARE(1)
}
#undef TOA_INST_DECLARE
#undef TOA_INST_DECLARE_NBM

// One dtype's entries (dtag: 0 = f32, 1 = f64), the DenseRow ones by block count: dense[nbm - 1].
struct toa_inst_table {
  decltype(&toa_inst_solve_0_0) solve;
  decltype(&toa_inst_inv_cov_0_0) inv_cov;
  decltype(&toa_inst_misc_fused_0_0) misc_fused;
  decltype(&toa_inst_misc_wide_0_0) misc_wide;
  decltype(&toa_inst_misc_accumulate_0_0) misc_accumulate;
  decltype(&toa_inst_jetrow_fused_0_0) jetrow_fused, jetrow_wide, narrow_fused;
  decltype(&toa_inst_jetrow_accumulate_0_0) jetrow_accumulate, narrow_accumulate;
  struct Dense {
    decltype(&toa_inst_fused_0_1) fused;
    decltype(&toa_inst_wide_0_1) wide;
    decltype(&toa_inst_accumulate_0_1) accumulate;
  } dense[4];
};
#define TOA_INST_DENSE(DT, NBM) {toa_inst_fused_##DT##_##NBM, toa_inst_wide_##DT##_##NBM, toa_inst_accumulate_##DT##_##NBM}
#define TOA_INST_TABLE(DT)                                                                                                         \
  {toa_inst_solve_##DT##_0, toa_inst_inv_cov_##DT##_0, toa_inst_misc_fused_##DT##_0, toa_inst_misc_wide_##DT##_0,                   \
   toa_inst_misc_accumulate_##DT##_0, toa_inst_jetrow_fused_##DT##_0, toa_inst_jetrow_wide_##DT##_0, toa_inst_narrow_fused_##DT##_0, \
   toa_inst_jetrow_accumulate_##DT##_0, toa_inst_narrow_accumulate_##DT##_0,                                                        \
   {TOA_INST_DENSE(DT, 1), TOA_INST_DENSE(DT, 2), TOA_INST_DENSE(DT, 3), TOA_INST_DENSE(DT, 4)}}
