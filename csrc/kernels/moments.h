// The arithmetic of a moments record: n, mean and M2 as f64 and the smallest
// and largest ascending sort word (fields n, mean, m2, lo, hi). stats.hip's
// record is these five; group_stats.hip's holds a sum between m2 and lo, whose
// rule it passes as `extra` (merge(r, a, b) and shfl_xor(o, r, off), run
// between m2 and lo). The record of two columns read together (PairRec, for
// corr / covar_samp / covar_pop) follows with its own update, merge, shuffle
// and wave butterfly. The build contracts with -ffp-contract=fast: the shape
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

// ------------------------------------------------------------------ pairs
// The record of two columns read together (corr / covar_samp / covar_pop):
// n, both means, both M2 and the co-moment C = sum (x - mean_x)(y - mean_y) as
// f64, and the count of rows whose x or y is NaN or an infinity (the results
// are decided from that count, not from what such a row left in the floats).
// The empty record is all zeros.
struct PairRec {
  double n, mx, my, m2x, m2y, cxy;
  uint64_t bad;
};

__device__ __forceinline__ PairRec pair_empty() { return PairRec{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0ull}; }

// Welford's update with one row
__device__ __forceinline__ void pair_add_row(PairRec& r, double x, double y) {
  r.n += 1.0;
  const double dx = x - r.mx;
  r.mx += dx / r.n;
  r.m2x += dx * (x - r.mx);
  const double dy = y - r.my;
  r.my += dy / r.n;
  r.m2y += dy * (y - r.my);
  r.cxy += dx * (y - r.my);
  r.bad += (__builtin_isfinite(x) && __builtin_isfinite(y)) ? 0ull : 1ull;
}

// Chan's merge of two pair records, `a` the earlier rows: merge_moments' factor
// order and empty-side selects, the co-moment with dx * dy in delta^2's place
__device__ __forceinline__ PairRec merge_pairs(const PairRec& a, const PairRec& b) {
  PairRec r;
  r.n = a.n + b.n;
  const double dx = b.mx - a.mx, dy = b.my - a.my;
  const double f = r.n > 0.0 ? b.n / r.n : 0.0;
  r.mx = a.n == 0.0 ? b.mx : (b.n == 0.0 ? a.mx : a.mx + dx * f);
  r.my = a.n == 0.0 ? b.my : (b.n == 0.0 ? a.my : a.my + dy * f);
  r.m2x = a.n == 0.0 ? b.m2x : (b.n == 0.0 ? a.m2x : a.m2x + b.m2x + dx * dx * (a.n * f));
  r.m2y = a.n == 0.0 ? b.m2y : (b.n == 0.0 ? a.m2y : a.m2y + b.m2y + dy * dy * (a.n * f));
  r.cxy = a.n == 0.0 ? b.cxy : (b.n == 0.0 ? a.cxy : a.cxy + b.cxy + dx * dy * (a.n * f));
  r.bad = a.bad + b.bad;
  return r;
}

__device__ __forceinline__ PairRec shfl_xor_pairs(const PairRec& r, int off) {
  PairRec o;
  o.n = __shfl_xor(r.n, off, kWave);
  o.mx = __shfl_xor(r.mx, off, kWave);
  o.my = __shfl_xor(r.my, off, kWave);
  o.m2x = __shfl_xor(r.m2x, off, kWave);
  o.m2y = __shfl_xor(r.m2y, off, kWave);
  o.cxy = __shfl_xor(r.cxy, off, kWave);
  o.bad = __shfl_xor(static_cast<unsigned long long>(r.bad), off, kWave);
  return o;
}

// wave_merge_moments for pair records: lane order, neighbours first, the
// wave's record in lane 0; the steps at or above `rows` are skipped
__device__ __forceinline__ PairRec wave_merge_pairs(PairRec r, int64_t rows = kWave) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    if (off >= rows) break;
    const PairRec o = shfl_xor_pairs(r, off);
    r = (lane & off) ? merge_pairs(o, r) : merge_pairs(r, o);
  }
  return r;
}

// a record as kPairRecordFields int64 bit patterns and back
__device__ __forceinline__ void store_pair(int64_t* __restrict__ dst, const PairRec& r) {
  dst[0] = __double_as_longlong(r.n);
  dst[1] = __double_as_longlong(r.mx);
  dst[2] = __double_as_longlong(r.my);
  dst[3] = __double_as_longlong(r.m2x);
  dst[4] = __double_as_longlong(r.m2y);
  dst[5] = __double_as_longlong(r.cxy);
  dst[6] = static_cast<int64_t>(r.bad);
}

__device__ __forceinline__ PairRec load_pair(const int64_t* __restrict__ src) {
  PairRec r;
  r.n = __longlong_as_double(src[0]);
  r.mx = __longlong_as_double(src[1]);
  r.my = __longlong_as_double(src[2]);
  r.m2x = __longlong_as_double(src[3]);
  r.m2y = __longlong_as_double(src[4]);
  r.cxy = __longlong_as_double(src[5]);
  r.bad = static_cast<uint64_t>(src[6]);
  return r;
}

}  // namespace k
}  // namespace tfa
