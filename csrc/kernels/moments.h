// The arithmetic of a moments record: n, mean and M2 as f64 and the smallest
// and largest ascending sort word (fields n, mean, m2, lo, hi). stats.hip's
// record is these five; group_stats.hip's holds a sum between m2 and lo, whose
// rule it passes as `extra` (merge(r, a, b) and shfl_xor(o, r, off), run
// between m2 and lo). The build contracts with -ffp-contract=fast: the shape
// and order of these expressions decide the bits of every result.
#pragma once

#include <cstdint>

#include "hip_common.h"

namespace tfa {
namespace k {

struct NoExtraFields {
  template <typename R>
  __device__ __forceinline__ void merge(R&, const R&, const R&) const {}
  template <typename R>
  __device__ __forceinline__ void shfl_xor(R&, const R&, int) const {}
};

// Chan's merge of two records, `a` the earlier rows
template <typename R, typename X = NoExtraFields>
__device__ __forceinline__ R merge_moments(const R& a, const R& b, const X& extra = X()) {
  R r;
  r.n = a.n + b.n;
  const double delta = b.mean - a.mean;
  const double f = r.n > 0.0 ? b.n / r.n : 0.0;
  // (an empty side holds mean 0: selected away, never mixed in)
  r.mean = a.n == 0.0 ? b.mean : (b.n == 0.0 ? a.mean : a.mean + delta * f);
  r.m2 = a.n == 0.0 ? b.m2 : (b.n == 0.0 ? a.m2 : a.m2 + b.m2 + delta * delta * (a.n * f));
  extra.merge(r, a, b);
  r.lo = a.lo < b.lo ? a.lo : b.lo;
  r.hi = a.hi > b.hi ? a.hi : b.hi;
  return r;
}

template <typename R, typename X = NoExtraFields>
__device__ __forceinline__ R shfl_xor_moments(const R& r, int off, const X& extra = X()) {
  R o;
  o.n = __shfl_xor(r.n, off, kWave);
  o.mean = __shfl_xor(r.mean, off, kWave);
  o.m2 = __shfl_xor(r.m2, off, kWave);
  extra.shfl_xor(o, r, off);
  o.lo = __shfl_xor(static_cast<unsigned long long>(r.lo), off, kWave);
  o.hi = __shfl_xor(static_cast<unsigned long long>(r.hi), off, kWave);
  return o;
}

// the lanes' records merged in lane order (xor butterfly, neighbours first):
// the wave's record in lane 0. Lanes from `rows` on hold empty records, and
// merging an empty record changes no bit: the steps at or above `rows` are
// skipped (rows: the same in every lane)
template <typename R, typename X = NoExtraFields>
__device__ __forceinline__ R wave_merge_moments(R r, const X& extra = X(), int64_t rows = kWave) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    if (off >= rows) break;
    const R o = shfl_xor_moments(r, off, extra);
    r = (lane & off) ? merge_moments(o, r, extra) : merge_moments(r, o, extra);
  }
  return r;
}

}  // namespace k
}  // namespace tfa
