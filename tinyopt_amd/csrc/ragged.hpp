// Ragged batches of a run-time model: every problem has its own item count.
//
//   data     [total_items][kD]   the items of all problems, one problem after another
//   header   [P][kH]             the problems' header scalars (null when kH = 0)
//   offsets  int64 [P + 1]       non-decreasing, [0] = 0, [P] = total_items: problem p owns items [off[p], off[p + 1])
//
// The ragged kernels are the uniform ones compiled with TOA_RAGGED defined (a code object of their own, jit.hip
// ensure_form): the models' bind(p) then takes the problem's range from `offsets`, and the persistent kernels walk an
// `order[P]` array (longest problems first) instead of the problem index.  Nothing here is seen by a build without the macro
// except the plain structs below.
#pragma once

namespace toa {

// What a ragged kernel is given on top of its uniform parameters.
struct RaggedArgs {
  const long long* offsets;   // [P + 1]
  const void* header;         // [P][kH] or null
  const int* order;           // [P]: the q-th problem handed out is order[q]; null = index order
  long long total_items;      // items of `data`: a range is clamped into [0, total_items)
  int max_items;              // the largest count the host checked its limits against: counts are clamped to it
  int reserved_;
};

// the ragged code object's seam kernels (accumulate, cost accumulate, eval rows) take them as one more kernel argument
#ifdef TOA_RAGGED
#define TOA_RAGGED_KARG , const toa::RaggedArgs rag
#else
#define TOA_RAGGED_KARG
#endif

struct RaggedRange { long long first; int count; };

// Problem p's items: wave-uniform (p is), so the two loads are scalar.  A damaged offsets array is clamped — the start into
// [0, total_items], the count into [0, min(max_items, total_items - start)]: nothing outside `data`, and nothing beyond the
// per-problem limits the host judged, is ever addressed.
__device__ __forceinline__ RaggedRange ragged_range(const RaggedArgs& r, long long p) {
  long long a = r.offsets[p];
  const long long b = r.offsets[p + 1];
  if (a < 0) a = 0;
  if (a > r.total_items) a = r.total_items;
  long long c = b - a;
  if (c > r.total_items - a) c = r.total_items - a;
  if (c > r.max_items) c = r.max_items;
  if (c < 0) c = 0;
  return RaggedRange{a, int(c)};
}

// The bucket of a count in the longest-first order: 0 for an empty problem, 1 + floor(log2(count)) otherwise (<= 32).
constexpr int kRaggedBuckets = 33;
__device__ __forceinline__ int ragged_bucket(long long c) { return c <= 0 ? 0 : 64 - __builtin_clzll((unsigned long long)c); }

}  // namespace toa
