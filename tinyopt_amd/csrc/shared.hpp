// Shared item tables: a run-time model that declares shared_scalars = kS > 0 reads, beside an item's private
// scalars p[0 .. kD), row i of ONE table [items][kS] that every problem of the batch shares — one design matrix for a GLM per gene,
// one time axis for a curve fit per pixel.  The table is handed over per call (toa_jit_lm_run_shared / toa_jit_accumulate_shared);
// RowModel::pass stages its rows by LDS-DMA next to the private items (row_model.hpp), so HBM streams the private part only
// and the table is expected to be served by the L2 after its first reader (a 400 KB table fits a 4 MiB L2; not measured with counters).
//
// The kernels of such a model are compiled with TOA_SHARED defined (jit.hip puts the define in front of the functor's source, so
// every code object of the model has it) and take one more argument.  Nothing here is seen by a build without the macro except the
// plain struct and the trait below.
#pragma once
#include <type_traits>

namespace toa {

// What a kernel of a shared model is given on top of its other arguments.
struct SharedArgs {
  const void* table;   // [rows][kS], the model's scalar type
  long long rows;      // = the items of every problem (judged by the host: toa_shared::rows == num_items)
};

// the seam kernels take them as one more kernel argument; the fused kernel reads them behind its parameter block
#ifdef TOA_SHARED
#define TOA_SHARED_KARG , const toa::SharedArgs shr
#else
#define TOA_SHARED_KARG
#endif

// Extension point: a functor with kS > 0 takes `const T* s` after `p` in its methods.  No functor without kS sees any of it:
// every use is behind `if constexpr`.
template <typename F, typename = void>
struct FunctorShared { static constexpr int value = 0; };
template <typename F>
struct FunctorShared<F, std::enable_if_t<(F::kS > 0)>> { static constexpr int value = F::kS; };

}  // namespace toa
