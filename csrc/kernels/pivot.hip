// The spread of groupBy(keys).pivot(p).agg(...): from the long table, one
// record per (key, pivot value), to the wide one, one row per key and one
// column per listed pivot value.
//
// The m records are in ascending (keys..., pivot) order. offsets [G + 1] is the
// CSR of the G distinct key tuples over them, pivot_words [m] the sort word of
// every record's pivot value (sort_words.h), so the words of one key,
// pivot_words[offsets[g] .. offsets[g + 1]), ascend as UNSIGNED 64-bit words
// and hold each word at most once. value_words [V] are the words of the listed
// values, in the order of the output columns (any order).
//
//   one thread per output cell (g, j): j is the grid's y (V <= kMaxPivotValues
//   fits it), g a grid-stride loop over x, consecutive lanes on consecutive g,
//   so the loads of offsets and the stores of every output coalesce. The
//   thread binary-searches its key's words for value_words[j] and then writes
//   cell j * G + g of every output a: vals[a][hit], or fill[a] where the key
//   has no record of that value. Bit copies of 4 or 8 bytes.
//
// Every cell of every output is written exactly once, by one thread: no
// atomics, no pre-fill launch, the same bits on every run. The per-output
// pointers and fills are a by-value argument struct that stays in the argument
// segment: the output loop is NOT unrolled, its index is uniform, and every
// turn reads its two pointers and its fill with scalar loads. (Expanded with
// compile-time indices the compiler hoists all sixteen outputs' pointers and
// fills out of the cell loop, 6 scalar registers each: more than there are,
// and they spill.) Nothing is indexed in registers at run time, so nothing
// goes to scratch. Cell indices are 64-bit. A thread clamps its range to
// [0, m], so it reads inside pivot_words and vals whatever offsets hold.
#include "hip_common.h"

namespace tfa {
namespace k {

namespace {

constexpr int kPT = 256;  // threads per block

}  // namespace

__global__ __launch_bounds__(kPT) void pivot_spread_kernel(const int64_t* __restrict__ offsets,
                                                           const uint64_t* __restrict__ pivot_words,
                                                           const uint64_t* __restrict__ value_words, int64_t G,
                                                           int64_t m, PivotSpreadCols pc) {
  const int64_t j = blockIdx.y;
  const uint64_t want = value_words[j];
  const int64_t stride = (int64_t)gridDim.x * kPT;
  for (int64_t g = (int64_t)blockIdx.x * kPT + threadIdx.x; g < G; g += stride) {
    int64_t lo = offsets[g], end = offsets[g + 1];
    lo = lo < 0 ? 0 : lo;
    end = end > m ? m : end;
    int64_t hi = end;
    while (lo < hi) {  // the first word of the range that is not below `want`
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (pivot_words[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    const bool hit = lo < end && pivot_words[lo] == want;
    const int64_t cell = j * G + g;
#pragma nounroll
    for (int a = 0; a < pc.n; ++a) {  // (a is uniform: scalar loads from the argument segment, scalar branches)
      if ((pc.wide >> a) & 1u) {
        static_cast<int64_t*>(pc.dst[a])[cell] = hit ? static_cast<const int64_t*>(pc.src[a])[lo] : pc.fill[a];
      } else {
        static_cast<int32_t*>(pc.dst[a])[cell] =
            hit ? static_cast<const int32_t*>(pc.src[a])[lo] : static_cast<int32_t>(pc.fill[a]);
      }
    }
  }
}

int pivot_block_threads() { return kPT; }

void pivot_spread(const int64_t* offsets, const int64_t* pivot_words, const int64_t* value_words, int64_t G, int64_t m,
                  int64_t V, const PivotSpreadCols& pc, hipStream_t s) {
  TFA_CHECK(pc.n >= 1 && pc.n <= kMaxPackCols, "pivot_spread: 1..", kMaxPackCols, " outputs, got ", pc.n);
  TFA_CHECK(V >= 0 && V <= kMaxPivotValues, "pivot_spread: at most ", kMaxPivotValues, " values, got ", V);
  TFA_CHECK(G >= 0 && m >= 0, "pivot_spread: negative sizes");
  if (G == 0 || V == 0) return;
  TFA_CHECK(offsets != nullptr && value_words != nullptr, "pivot_spread: null offsets or value words");
  TFA_CHECK(m == 0 || pivot_words != nullptr, "pivot_spread: null pivot words");
  for (int a = 0; a < pc.n; ++a)
    TFA_CHECK(pc.dst[a] != nullptr && (m == 0 || pc.src[a] != nullptr), "pivot_spread: output ", a, " has no buffer");
  hipLaunchKernelGGL(pivot_spread_kernel, dim3((unsigned)ew_grid(G, kPT), (unsigned)V), dim3(kPT), 0, s, offsets,
                     reinterpret_cast<const uint64_t*>(pivot_words), reinterpret_cast<const uint64_t*>(value_words), G,
                     m, pc);
  TFA_LAUNCH_CHECK("pivot_spread_kernel");
}

}  // namespace k
}  // namespace tfa
