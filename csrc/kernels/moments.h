// The arithmetic of a moments record: n, mean and M2 as f64 and the smallest
// and largest ascending sort word (fields n, mean, m2, lo, hi). stats.hip's
// record is these five; group_stats.hip's holds a sum between m2 and lo, whose
// rule it passes as `extra` (merge(r, a, b) and shfl_xor(o, r, off), run
// between m2 and lo). The record of two columns read together (PairRec, for
// corr / covar_samp / covar_pop) follows with its own update, merge, shuffle
// and wave butterfly, and after it the record of the third and fourth central
// moments of one column (HighRec, for skewness / kurtosis), and last the
// per-component record of a weighted vector summary (SumRec). The build contracts
// with -ffp-contract=fast: the shape and order of these expressions decide the
// bits of every result.
#pragma once

#include <cstdint>

#include "hip_common.h"
#include "sort_words.h"

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

// ------------------------------------------------------------------ high moments
// The record of one column's central moments up to order four (skewness /
// kurtosis): n, the mean and Mk = sum (x - mean)^k for k = 2, 3, 4 as f64, and
// the count of rows that are NaN or an infinity (the results are decided from
// that count, not from what such a row left in the floats). Everything is a
// sum of powers of deviations from a running mean, updated and merged; a power
// sum of x itself appears nowhere. The empty record is all zeros.
struct HighRec {
  double n, mean, m2, m3, m4;
  uint64_t bad;
};

__device__ __forceinline__ HighRec high_empty() { return HighRec{0.0, 0.0, 0.0, 0.0, 0.0, 0ull}; }

// Welford's update with one row in Terriberry's form. With d = x - mean,
// dn = d / n and t = d * dn * (n - 1) (n the count after the row): m4 first
// (it reads the old m3 and m2), then m3 (the old m2), then m2, then the mean.
// Each sum is written term by term, left to right, as below.
__device__ __forceinline__ void high_add_row(HighRec& r, double x) {
  const double n1 = r.n;
  r.n += 1.0;
  const double n = r.n;
  const double d = x - r.mean;
  const double dn = d / n;
  const double dn2 = dn * dn;
  const double t = d * dn * n1;
  r.m4 += t * dn2 * (n * n - 3.0 * n + 3.0) + 6.0 * dn2 * r.m2 - 4.0 * dn * r.m3;
  r.m3 += t * dn * (n - 2.0) - 3.0 * dn * r.m2;
  r.m2 += t;
  r.mean += dn;
  r.bad += __builtin_isfinite(x) ? 0ull : 1ull;
}

// Pébay's merge of two records, `a` the earlier rows. delta = mean_b - mean_a,
// n = na + nb, dn = delta / n. The terms, in the order they are added:
//   M2 = M2a + M2b + delta^2 na nb / n                  (merge_moments' form)
//   M3 = M3a + M3b + dn^2 delta na nb (na - nb) + 3 dn (na M2b - nb M2a)
//   M4 = M4a + M4b + dn^3 delta na nb (na^2 - na nb + nb^2)
//        + 6 dn^2 (na^2 M2b + nb^2 M2a) + 4 dn (na M3b - nb M3a)
// with merge_moments' empty-side selects: an empty side is selected away and
// never mixed in, so merging an empty record changes no bit.
__device__ __forceinline__ HighRec merge_high(const HighRec& a, const HighRec& b) {
  HighRec r;
  r.n = a.n + b.n;
  const double delta = b.mean - a.mean;
  const double f = r.n > 0.0 ? b.n / r.n : 0.0;
  const double dn = r.n > 0.0 ? delta / r.n : 0.0;
  const double dn2 = dn * dn;
  const double nab = a.n * b.n;
  const double mean = a.mean + delta * f;
  const double m2 = a.m2 + b.m2 + delta * delta * (a.n * f);
  const double m3 = a.m3 + b.m3 + dn2 * delta * (nab * (a.n - b.n)) + 3.0 * dn * (a.n * b.m2 - b.n * a.m2);
  const double m4 = a.m4 + b.m4 + dn2 * dn * delta * (nab * (a.n * a.n - nab + b.n * b.n)) +
                    6.0 * dn2 * (a.n * a.n * b.m2 + b.n * b.n * a.m2) + 4.0 * dn * (a.n * b.m3 - b.n * a.m3);
  r.mean = a.n == 0.0 ? b.mean : (b.n == 0.0 ? a.mean : mean);
  r.m2 = a.n == 0.0 ? b.m2 : (b.n == 0.0 ? a.m2 : m2);
  r.m3 = a.n == 0.0 ? b.m3 : (b.n == 0.0 ? a.m3 : m3);
  r.m4 = a.n == 0.0 ? b.m4 : (b.n == 0.0 ? a.m4 : m4);
  r.bad = a.bad + b.bad;
  return r;
}

__device__ __forceinline__ HighRec shfl_xor_high(const HighRec& r, int off) {
  HighRec o;
  o.n = __shfl_xor(r.n, off, kWave);
  o.mean = __shfl_xor(r.mean, off, kWave);
  o.m2 = __shfl_xor(r.m2, off, kWave);
  o.m3 = __shfl_xor(r.m3, off, kWave);
  o.m4 = __shfl_xor(r.m4, off, kWave);
  o.bad = __shfl_xor(static_cast<unsigned long long>(r.bad), off, kWave);
  return o;
}

// wave_merge_moments for high records: lane order, neighbours first, the
// wave's record in lane 0; the steps at or above `rows` are skipped
__device__ __forceinline__ HighRec wave_merge_high(HighRec r, int64_t rows = kWave) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    if (off >= rows) break;
    const HighRec o = shfl_xor_high(r, off);
    r = (lane & off) ? merge_high(o, r) : merge_high(r, o);
  }
  return r;
}

// a record as kHighRecordFields int64 bit patterns and back
__device__ __forceinline__ void store_high(int64_t* __restrict__ dst, const HighRec& r) {
  dst[0] = __double_as_longlong(r.n);
  dst[1] = __double_as_longlong(r.mean);
  dst[2] = __double_as_longlong(r.m2);
  dst[3] = __double_as_longlong(r.m3);
  dst[4] = __double_as_longlong(r.m4);
  dst[5] = static_cast<int64_t>(r.bad);
}

__device__ __forceinline__ HighRec load_high(const int64_t* __restrict__ src) {
  HighRec r;
  r.n = __longlong_as_double(src[0]);
  r.mean = __longlong_as_double(src[1]);
  r.m2 = __longlong_as_double(src[2]);
  r.m3 = __longlong_as_double(src[3]);
  r.m4 = __longlong_as_double(src[4]);
  r.bad = static_cast<uint64_t>(src[5]);
  return r;
}

// ------------------------------------------------------------------ weighted summary
// One component's record of the weighted summary of a vector column
// (Summarizer, vector_summary.hip): the weighted mean, M2 = sum w (x - mean)^2,
// L1 = sum w |x| and S2 = sum w x^2 as f64, the counts of entries that are not
// zero and of entries that are NaN or an infinity, and the smallest and largest
// ascending sort word of the values as f64. What belongs to a row rather than
// to a component (the weight sum W, sum w^2, the row count) is carried once by
// the caller for all the components it owns. Contraction is off in the two
// functions below and the fused operations are written out: their bits do not
// depend on the caller. The empty record is zeros, all ones in lo.
struct SumRec {
  double mean, m2, l1, s2;
  uint64_t nnz, bad, lo, hi;
};

__device__ __forceinline__ SumRec summary_empty() { return SumRec{0.0, 0.0, 0.0, 0.0, 0ull, 0ull, ~0ull, 0ull}; }

// West's update with one row of weight w > 0; f = w / (W + w) with W the weight
// sum before the row (the caller forms it once per row)
__device__ __forceinline__ void summary_add_row(SumRec& r, double x, double w, double f) {
#pragma clang fp contract(off)
  const double delta = x - r.mean;
  r.mean = __builtin_fma(delta, f, r.mean);
  r.m2 = __builtin_fma(w * delta, x - r.mean, r.m2);
  r.l1 = __builtin_fma(w, __builtin_fabs(x), r.l1);
  r.s2 = __builtin_fma(w * x, x, r.s2);
  r.nnz += x != 0.0 ? 1ull : 0ull;  // (-0.0 is zero, a NaN is not)
  r.bad += __builtin_isfinite(x) ? 0ull : 1ull;
  const uint64_t word = encode_f64(static_cast<uint64_t>(__double_as_longlong(x)));
  r.lo = word < r.lo ? word : r.lo;
  r.hi = word > r.hi ? word : r.hi;
}

// the factor of Chan's weighted merge: the later side's share of the weight
__device__ __forceinline__ double summary_fraction(double wa, double wb) {
  const double w = wa + wb;
  return w > 0.0 ? wb / w : 0.0;
}

// Chan's merge of two records of weight sums wa and wb, `a` the earlier side,
// f = summary_fraction(wa, wb): merge_moments' factor order and empty-side
// selects with weight sums in the counts' place
__device__ __forceinline__ SumRec merge_summary(double wa, const SumRec& a, double wb, const SumRec& b, double f) {
#pragma clang fp contract(off)
  SumRec r;
  const double delta = b.mean - a.mean;
  r.mean = wa == 0.0 ? b.mean : (wb == 0.0 ? a.mean : a.mean + delta * f);
  r.m2 = wa == 0.0 ? b.m2 : (wb == 0.0 ? a.m2 : a.m2 + b.m2 + delta * delta * (wa * f));
  r.l1 = a.l1 + b.l1;
  r.s2 = a.s2 + b.s2;
  r.nnz = a.nnz + b.nnz;
  r.bad = a.bad + b.bad;
  r.lo = a.lo < b.lo ? a.lo : b.lo;
  r.hi = a.hi > b.hi ? a.hi : b.hi;
  return r;
}

}  // namespace k
}  // namespace tfa
