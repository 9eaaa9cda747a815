// Grouped statistics for GroupedData.agg / DataFrame.agg.
//
// A record is six 8-byte fields per (group, value column): n, mean and M2 as
// f64 (every element converted to f64 first, as in stats.hip), the sum (the
// int64 bits of a wrapping sum for the integer dtypes, an f64 running sum for
// the float ones) and the smallest and largest ascending sort word.
//
//   group_moments   rows come as CSR segments (perm, offsets) of segment_csr.
//            The work split is the per-segment chunking: a work item is a
//            (segment, chunk) pair, a chunk at most kGroupChunk rows of one
//            segment (every segment has at least one item, an empty one too).
//            The chunk counts are scanned on the device (join_scan: one stream
//            synchronisation reads the total); an item finds its segment by a
//            binary search in the scanned counts. One wave takes one item: the
//            lanes read the chunk's rows at stride 64 through perm, Welford per
//            lane, the lanes' records merged with Chan's formula in lane order
//            (xor butterfly), sums added in the same order. The column is the
//            grid's y. Segments of more than one chunk are folded in chunk
//            order by a second kernel: one thread per segment and column up
//            to kFoldSerial chunks; a longer segment (measured: half of 10M
//            rows in one key is 9766 chunks, 3.2 ms folded by one thread) is
//            folded by the thread's wave, each lane a run of consecutive
//            chunks, the lanes in lane order. When every segment is one chunk
//            the first kernel writes the result itself. A group's record
//            depends on its own rows in row order alone: not on the other
//            groups, not on the run.
//   merge_group_records   records ordered by (key, partition), CSR offsets
//            over them: one thread per (group, column) folds its records
//            sequentially, starting from the first.
//   group_results   merged records -> typed output columns, up to
//            kMaxPackCols of them in one launch (the output is the grid's y):
//            words decoded back to the column's type, the NaN / infinity rule
//            of describe decided from the extreme words, sqrt(M2 / (n - 1))
//            and the rest.
//
//   pairs    group_pair_moments, merge_pair_records and pair_results are the
//            same three steps for the pair record of moments.h (corr /
//            covar_samp / covar_pop): the same work items (group_items builds
//            them for both), both columns gathered through perm, Welford per
//            lane, pair records merged in lane, chunk and partition order.
//
// No float atomics, no inter-block communication, every loop bounded by the
// row count.
#include <algorithm>
#include <cmath>
#include <limits>

#include "column_types.h"
#include "hip_common.h"
#include "moments.h"
#include "sort_words.h"

namespace tfa {
namespace k {

namespace {

constexpr int kT = 256;  // threads per block of every kernel here
constexpr int kWaves = kT / kWave;
constexpr int kGroupChunk = 512;  // rows per work item
constexpr int kLaneRows = 4;      // independent loads in flight per lane
constexpr int kFoldSerial = 8;    // most chunks of a segment one thread folds on its own

struct GRec {
  double n, mean, m2;
  uint64_t sum, lo, hi;
};
static_assert(sizeof(GRec) == 8 * kGroupRecordFields, "a record is six 8-byte fields");

__device__ __forceinline__ GRec grec_empty() { return GRec{0.0, 0.0, 0.0, 0ull, ~0ull, 0ull}; }

// the sum field in moments.h's merge and shuffle: wrapping for the integer
// dtypes, f64 for the float ones (an empty side selected away, as the mean)
struct SumField {
  bool is_float;
  __device__ __forceinline__ void merge(GRec& r, const GRec& a, const GRec& b) const {
    r.sum = is_float ? (a.n == 0.0 ? b.sum : (b.n == 0.0 ? a.sum : f64_bits(bits_f64(a.sum) + bits_f64(b.sum))))
                     : a.sum + b.sum;
  }
  __device__ __forceinline__ void shfl_xor(GRec& o, const GRec& r, int off) const {
    o.sum = __shfl_xor(static_cast<unsigned long long>(r.sum), off, kWave);
  }
};

__device__ __forceinline__ GRec grec_merge(const GRec& a, const GRec& b, bool is_float) {
  return merge_moments(a, b, SumField{is_float});
}

template <typename T>
struct SumOf {  // integers: wrapping 64-bit; floats: f64
  static __device__ __forceinline__ void add(uint64_t& s, double&, T v) {
    s += static_cast<uint64_t>(static_cast<int64_t>(v));
  }
  static __device__ __forceinline__ uint64_t bits(uint64_t s, double) { return s; }
};
template <>
struct SumOf<float> {
  static __device__ __forceinline__ void add(uint64_t&, double& s, float v) { s += static_cast<double>(v); }
  static __device__ __forceinline__ uint64_t bits(uint64_t, double s) { return f64_bits(s); }
};
template <>
struct SumOf<double> {
  static __device__ __forceinline__ void add(uint64_t&, double& s, double v) { s += v; }
  static __device__ __forceinline__ uint64_t bits(uint64_t, double s) { return f64_bits(s); }
};

// one lane's record of rows perm[lo + lane], perm[lo + lane + 64], ... below hi
// (0 <= lo <= hi <= the length of perm); a perm value outside [0, n) is skipped
template <typename T>
__device__ __forceinline__ GRec lane_rows(const void* __restrict__ src, const int64_t* __restrict__ perm, int64_t lo,
                                          int64_t hi, int64_t n, int lane) {
  const T* __restrict__ p = static_cast<const T*>(src);
  double cnt = 0.0, mean = 0.0, m2 = 0.0, fsum = 0.0;
  uint64_t isum = 0, wlo = ~0ull, whi = 0ull;
  for (int64_t r = lo + lane; r < hi; r += kLaneRows * kWave) {
    int64_t idx[kLaneRows];
    T v[kLaneRows];
#pragma unroll
    for (int j = 0; j < kLaneRows; ++j) {
      const int64_t rr = r + j * kWave;
      idx[j] = rr < hi ? perm[rr] : -1;
    }
#pragma unroll
    for (int j = 0; j < kLaneRows; ++j) v[j] = (idx[j] >= 0 && idx[j] < n) ? p[idx[j]] : T(0);
#pragma unroll
    for (int j = 0; j < kLaneRows; ++j) {
      if (idx[j] >= 0 && idx[j] < n) {
        const double x = static_cast<double>(v[j]);
        cnt += 1.0;
        const double d = x - mean;
        mean += d / cnt;
        m2 += d * (x - mean);
        SumOf<T>::add(isum, fsum, v[j]);
        const uint64_t w = sort_word(v[j]);
        wlo = w < wlo ? w : wlo;
        whi = w > whi ? w : whi;
      }
    }
  }
  GRec out = grec_empty();
  if (cnt > 0.0) out = GRec{cnt, mean, m2, SumOf<T>::bits(isum, fsum), wlo, whi};
  return out;
}

__device__ __forceinline__ void store_rec(int64_t* __restrict__ dst, const GRec& r) {
  dst[0] = static_cast<int64_t>(f64_bits(r.n));
  dst[1] = static_cast<int64_t>(f64_bits(r.mean));
  dst[2] = static_cast<int64_t>(f64_bits(r.m2));
  dst[3] = static_cast<int64_t>(r.sum);
  dst[4] = static_cast<int64_t>(r.lo);
  dst[5] = static_cast<int64_t>(r.hi);
}

__device__ __forceinline__ GRec load_rec(const int64_t* __restrict__ src) {
  GRec r;
  r.n = bits_f64(static_cast<uint64_t>(src[0]));
  r.mean = bits_f64(static_cast<uint64_t>(src[1]));
  r.m2 = bits_f64(static_cast<uint64_t>(src[2]));
  r.sum = static_cast<uint64_t>(src[3]);
  r.lo = static_cast<uint64_t>(src[4]);
  r.hi = static_cast<uint64_t>(src[5]);
  return r;
}

}  // namespace

// cnt[g] = chunks of segment g, at least one
__global__ __launch_bounds__(kT) void group_chunk_count_kernel(const int64_t* __restrict__ offsets, int64_t nseg,
                                                               int64_t nperm, int64_t* __restrict__ cnt) {
  const int64_t g = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (g >= nseg) return;
  const int64_t a = clamp64(offsets[g], 0, nperm), b = clamp64(offsets[g + 1], a, nperm);
  const int64_t c = (b - a + kGroupChunk - 1) / kGroupChunk;
  cnt[g] = c < 1 ? 1 : c;
}

// wave w of block (b, c): item b * kWaves + w of column c -> part[item][c].
// coffs [nseg + 1]: the exclusive scan of the chunk counts, coffs[nseg] == items
__global__ __launch_bounds__(kT) void group_moments_kernel(StatCols cols, int64_t n, const int64_t* __restrict__ perm,
                                                           int64_t nperm, const int64_t* __restrict__ offsets,
                                                           const int64_t* __restrict__ coffs, int64_t nseg,
                                                           int64_t items, int64_t* __restrict__ part) {
  const int lane = threadIdx.x & (kWave - 1);
  const int c = blockIdx.y;
  const int64_t item = (int64_t)blockIdx.x * kWaves +
                       __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x / kWave));
  if (item >= items) return;  // (the whole wave)
  // coffs[0] == 0 <= item < coffs[nseg]: the segment lies in [0, nseg - 1]
  const int64_t g = last_not_above(coffs, 0, 0, nseg - 1, item);
  const int64_t ch = item - coffs[g];
  const int64_t a = clamp64(offsets[g], 0, nperm), b = clamp64(offsets[g + 1], a, nperm);
  const int64_t lo = clamp64(a + ch * kGroupChunk, a, b);
  const int64_t hi = lo + kGroupChunk < b ? lo + kGroupChunk : b;
  const void* src = cols.ptr[c];
  const DType dt = cols.dtype[c];
  // (the dtype is uniform: one scalar branch per block)
  GRec r = dispatch_column(dt, [&](auto tag) { return lane_rows<decltype(tag)>(src, perm, lo, hi, n, lane); });
  // a short chunk stops early (a one-row group merges nothing)
  r = wave_merge_moments(r, SumField{is_float_dtype(dt)}, hi - lo);
  if (lane == 0) store_rec(part + (item * gridDim.y + c) * kGroupRecordFields, r);
}

// thread (g, c): part[coffs[g] .. coffs[g + 1])[c] merged in chunk order -> out[g][c].
// Up to kFoldSerial chunks: the thread folds them one after the other. More
// (a key that holds a large share of the rows): the wave takes the thread's
// pair together, lane l the l-th run of ceil(chunks / 64) consecutive chunks,
// the lanes' records merged in lane order: still chunk order, and a function
// of the segment's chunk count alone.
__global__ __launch_bounds__(kT) void group_fold_kernel(StatCols cols, const int64_t* __restrict__ part,
                                                        const int64_t* __restrict__ coffs, int64_t nseg, int64_t items,
                                                        int64_t* __restrict__ out) {
  const int C = cols.n;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
  const bool valid = t < nseg * C;
  const int64_t g = valid ? t / C : 0;
  const int c = valid ? static_cast<int>(t - g * C) : 0;
  const int64_t a = clamp64(coffs[g], 0, items - 1), b = clamp64(coffs[g + 1], a + 1, items);
  const bool wide = valid && b - a > kFoldSerial;
  if (valid && !wide) {
    const bool fl = is_float_dtype(cols.dtype[c]);
    GRec r = load_rec(part + (a * C + c) * kGroupRecordFields);
    for (int64_t i = a + 1; i < b; ++i) r = grec_merge(r, load_rec(part + (i * C + c) * kGroupRecordFields), fl);
    store_rec(out + t * kGroupRecordFields, r);
  }
  unsigned long long todo = __ballot(wide);  // (the same in every lane: at most 64 rounds)
  while (todo) {
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int64_t sa = __shfl(static_cast<long long>(a), src, kWave), sb = __shfl(static_cast<long long>(b), src, kWave);
    const int64_t st = __shfl(static_cast<long long>(t), src, kWave);
    const int sc = __shfl(c, src, kWave);
    const bool fl = is_float_dtype(cols.dtype[sc]);
    const int64_t per = (sb - sa + kWave - 1) / kWave;
    const int64_t i0 = sa + lane * per < sb ? sa + lane * per : sb, i1 = i0 + per < sb ? i0 + per : sb;
    GRec r = grec_empty();
    if (i0 < i1) r = load_rec(part + (i0 * C + sc) * kGroupRecordFields);
    for (int64_t i = i0 + 1; i < i1; ++i) r = grec_merge(r, load_rec(part + (i * C + sc) * kGroupRecordFields), fl);
    // wave_merge_moments written out: through the helper the compiler schedules
    // this loop nest differently (same registers), and the skewed case of
    // scripts/group_agg_profile.py then measured 0.3 % outside its run-to-run spread
    const SumField sum{fl};
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const GRec o = shfl_xor_moments(r, off, sum);
      r = (lane & off) ? merge_moments(o, r, sum) : merge_moments(r, o, sum);
    }
    if (lane == 0) store_rec(out + st * kGroupRecordFields, r);
  }
}

// thread (g, c): recs[offsets[g] .. offsets[g + 1])[c] merged in order -> out[g][c]
__global__ __launch_bounds__(kT) void merge_group_records_kernel(const int64_t* __restrict__ recs, int64_t m, int C,
                                                                 uint32_t float_mask,
                                                                 const int64_t* __restrict__ offsets, int64_t ng,
                                                                 int64_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (t >= ng * C) return;
  const int64_t g = t / C;
  const int c = static_cast<int>(t - g * C);
  const int64_t a = clamp64(offsets[g], 0, m), b = clamp64(offsets[g + 1], a, m);
  const bool fl = (float_mask >> c) & 1u;
  GRec r = grec_empty();
  if (a < b) r = load_rec(recs + (a * C + c) * kGroupRecordFields);
  for (int64_t i = a + 1; i < b; ++i) r = grec_merge(r, load_rec(recs + (i * C + c) * kGroupRecordFields), fl);
  store_rec(out + t * kGroupRecordFields, r);
}

namespace {

// the value of a float column's word, as f64
__device__ __forceinline__ double word_value(uint64_t w, DType dt) {
  return dt == DType::F32 ? static_cast<double>(__uint_as_float(decode_f32(w)))
                          : bits_f64(decode_f64(w));
}

}  // namespace

// thread g of block (.., o): output o of group g
__global__ __launch_bounds__(kT) void group_results_kernel(const int64_t* __restrict__ recs, int64_t ng, int C,
                                                           GroupResultSpec spec) {
  const int o = blockIdx.y;
  const int64_t g = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (g >= ng) return;
  const int c = spec.col[o];
  const DType dt = spec.dtype[o];
  const GroupStat st = spec.stat[o];
  const GRec r = load_rec(recs + (g * C + c) * kGroupRecordFields);
  void* out = spec.out[o];
  if (st == GroupStat::COUNT) {
    static_cast<int64_t*>(out)[g] = static_cast<int64_t>(r.n);
    return;
  }
  if (st == GroupStat::MIN || st == GroupStat::MAX) {
    const bool has = r.n > 0.0;  // (a group without rows has no extreme: zero)
    const uint64_t w = st == GroupStat::MIN ? r.lo : r.hi;
    store_word(out, g, dt, w, has);
    return;
  }
  const bool fl = is_float_dtype(dt);
  if (st == GroupStat::SUM && !fl) {
    static_cast<int64_t*>(out)[g] = static_cast<int64_t>(r.sum);
    return;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double mean = r.n > 0.0 ? r.mean : nan, m2 = r.n > 0.0 ? r.m2 : nan, sum = fl ? bits_f64(r.sum) : 0.0;
  if (r.n == 0.0) sum = 0.0;
  if (fl && r.n > 0.0) {
    // a NaN or an infinity propagates as in a plain sum / n, whatever the
    // order the rows were met in: the extremes tell what is there
    const double top = word_value(r.hi, dt), bottom = word_value(r.lo, dt);
    if (top != top || (top == inf && bottom == -inf)) {
      mean = m2 = sum = nan;
    } else if (top == inf || bottom == -inf) {
      mean = sum = top == inf ? inf : -inf;
      m2 = nan;
    }
  }
  double v;
  switch (st) {
    case GroupStat::SUM: v = sum; break;
    case GroupStat::AVG: v = mean; break;
    case GroupStat::VAR_SAMP: v = r.n >= 2.0 ? m2 / (r.n - 1.0) : nan; break;
    case GroupStat::VAR_POP: v = r.n >= 1.0 ? m2 / r.n : nan; break;
    case GroupStat::STDDEV_SAMP: v = r.n >= 2.0 ? sqrt(m2 / (r.n - 1.0)) : nan; break;
    default: v = r.n >= 1.0 ? sqrt(m2 / r.n) : nan; break;  // STDDEV_POP
  }
  static_cast<double*>(out)[g] = v;
}

// ------------------------------------------------------------------ pairs
namespace {

// one lane's pair record of rows perm[lo + lane], perm[lo + lane + 64], ...
// below hi of columns x and y (lane_rows' walk; both loads of the kLaneRows
// rows are issued before the first update)
template <typename T>
__device__ __forceinline__ void gather_rows(const void* __restrict__ src, const int64_t (&idx)[kLaneRows], int64_t n,
                                            double (&v)[kLaneRows]) {
  const T* __restrict__ p = static_cast<const T*>(src);
  T t[kLaneRows];
#pragma unroll
  for (int j = 0; j < kLaneRows; ++j) t[j] = (idx[j] >= 0 && idx[j] < n) ? p[idx[j]] : T(0);
#pragma unroll
  for (int j = 0; j < kLaneRows; ++j) v[j] = static_cast<double>(t[j]);
}

__device__ __forceinline__ PairRec lane_pair_rows(const void* __restrict__ px, DType tx, const void* __restrict__ py,
                                                  DType ty, const int64_t* __restrict__ perm, int64_t lo, int64_t hi,
                                                  int64_t n, int lane) {
  PairRec r = pair_empty();
  for (int64_t row = lo + lane; row < hi; row += kLaneRows * kWave) {
    int64_t idx[kLaneRows];
    double x[kLaneRows], y[kLaneRows];
#pragma unroll
    for (int j = 0; j < kLaneRows; ++j) {
      const int64_t rr = row + j * kWave;
      idx[j] = rr < hi ? perm[rr] : -1;
    }
    // (the dtypes are uniform: scalar branches)
    dispatch_column(tx, [&](auto tag) { gather_rows<decltype(tag)>(px, idx, n, x); });
    dispatch_column(ty, [&](auto tag) { gather_rows<decltype(tag)>(py, idx, n, y); });
#pragma unroll
    for (int j = 0; j < kLaneRows; ++j) {
      if (idx[j] >= 0 && idx[j] < n) pair_add_row(r, x[j], y[j]);
    }
  }
  return r;
}

}  // namespace

// group_moments_kernel for pair records: wave w of block (b, q) takes item
// b * kWaves + w of pair q -> part[item][q]
__global__ __launch_bounds__(kT) void group_pair_moments_kernel(StatCols xs, StatCols ys, int64_t n,
                                                                const int64_t* __restrict__ perm, int64_t nperm,
                                                                const int64_t* __restrict__ offsets,
                                                                const int64_t* __restrict__ coffs, int64_t nseg,
                                                                int64_t items, int64_t* __restrict__ part) {
  const int lane = threadIdx.x & (kWave - 1);
  const int q = blockIdx.y;
  const int64_t item = (int64_t)blockIdx.x * kWaves +
                       __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x / kWave));
  if (item >= items) return;  // (the whole wave)
  const int64_t g = last_not_above(coffs, 0, 0, nseg - 1, item);
  const int64_t ch = item - coffs[g];
  const int64_t a = clamp64(offsets[g], 0, nperm), b = clamp64(offsets[g + 1], a, nperm);
  const int64_t lo = clamp64(a + ch * kGroupChunk, a, b);
  const int64_t hi = lo + kGroupChunk < b ? lo + kGroupChunk : b;
  PairRec r = lane_pair_rows(xs.ptr[q], xs.dtype[q], ys.ptr[q], ys.dtype[q], perm, lo, hi, n, lane);
  r = wave_merge_pairs(r, hi - lo);
  if (lane == 0) store_pair(part + (item * gridDim.y + q) * kPairRecordFields, r);
}

// group_fold_kernel for pair records: thread (g, q) folds part[coffs[g] ..
// coffs[g + 1])[q] in chunk order -> out[g][q]; a segment of more than
// kFoldSerial chunks is folded by the thread's wave, lane l the l-th run of
// consecutive chunks, the lanes in lane order
__global__ __launch_bounds__(kT) void group_pair_fold_kernel(int Q, const int64_t* __restrict__ part,
                                                             const int64_t* __restrict__ coffs, int64_t nseg,
                                                             int64_t items, int64_t* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
  const bool valid = t < nseg * Q;
  const int64_t g = valid ? t / Q : 0;
  const int q = valid ? static_cast<int>(t - g * Q) : 0;
  const int64_t a = clamp64(coffs[g], 0, items - 1), b = clamp64(coffs[g + 1], a + 1, items);
  const bool wide = valid && b - a > kFoldSerial;
  if (valid && !wide) {
    PairRec r = load_pair(part + (a * Q + q) * kPairRecordFields);
    for (int64_t i = a + 1; i < b; ++i) r = merge_pairs(r, load_pair(part + (i * Q + q) * kPairRecordFields));
    store_pair(out + t * kPairRecordFields, r);
  }
  unsigned long long todo = __ballot(wide);  // (the same in every lane: at most 64 rounds)
  while (todo) {
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int64_t sa = __shfl(static_cast<long long>(a), src, kWave);
    const int64_t sb = __shfl(static_cast<long long>(b), src, kWave);
    const int64_t st = __shfl(static_cast<long long>(t), src, kWave);
    const int sq = __shfl(q, src, kWave);
    const int64_t per = (sb - sa + kWave - 1) / kWave;
    const int64_t i0 = sa + lane * per < sb ? sa + lane * per : sb, i1 = i0 + per < sb ? i0 + per : sb;
    PairRec r = pair_empty();
    if (i0 < i1) r = load_pair(part + (i0 * Q + sq) * kPairRecordFields);
    for (int64_t i = i0 + 1; i < i1; ++i) r = merge_pairs(r, load_pair(part + (i * Q + sq) * kPairRecordFields));
    r = wave_merge_pairs(r);
    if (lane == 0) store_pair(out + st * kPairRecordFields, r);
  }
}

// thread (g, q): recs[offsets[g] .. offsets[g + 1])[q] merged in order -> out[g][q]
__global__ __launch_bounds__(kT) void merge_pair_records_kernel(const int64_t* __restrict__ recs, int64_t m, int Q,
                                                                const int64_t* __restrict__ offsets, int64_t ng,
                                                                int64_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (t >= ng * Q) return;
  const int64_t g = t / Q;
  const int q = static_cast<int>(t - g * Q);
  const int64_t a = clamp64(offsets[g], 0, m), b = clamp64(offsets[g + 1], a, m);
  PairRec r = pair_empty();
  if (a < b) r = load_pair(recs + (a * Q + q) * kPairRecordFields);
  for (int64_t i = a + 1; i < b; ++i) r = merge_pairs(r, load_pair(recs + (i * Q + q) * kPairRecordFields));
  store_pair(out + t * kPairRecordFields, r);
}

// thread g of block (.., o): output o of group g. A row with a NaN or an
// infinity in either column makes all three NaN, whichever row it was
__global__ __launch_bounds__(kT) void pair_results_kernel(const int64_t* __restrict__ recs, int64_t ng, int Q,
                                                          PairResultSpec spec) {
  const int o = blockIdx.y;
  const int64_t g = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (g >= ng) return;
  const PairRec r = load_pair(recs + (g * Q + spec.pair[o]) * kPairRecordFields);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double v;
  switch (spec.stat[o]) {
    case PairStat::COVAR_POP: v = r.n >= 1.0 ? r.cxy / r.n : nan; break;
    case PairStat::COVAR_SAMP: v = r.n >= 2.0 ? r.cxy / (r.n - 1.0) : nan; break;
    default: v = (r.n >= 1.0 && r.m2x != 0.0 && r.m2y != 0.0) ? r.cxy / sqrt(r.m2x * r.m2y) : nan; break;  // CORR
  }
  spec.out[o][g] = r.bad > 0 ? nan : v;
}

// ------------------------------------------------------------------ host API
namespace {

int64_t max_chunks(int64_t nperm) { return std::max<int64_t>(1, (nperm + kGroupChunk - 1) / kGroupChunk); }

size_t align8(size_t b) { return (b + 7) & ~size_t(7); }

}  // namespace

int group_chunk_rows() { return kGroupChunk; }

// the work items of the CSR segments, built the same way for both record
// kinds. workspace: int64 cnt[nseg] | int64 coffs[nseg + 1] | join_scan's
size_t group_items_workspace_bytes(int64_t nseg) {
  if (nseg <= 0) return 0;
  return align8(8 * nseg) + align8(8 * (nseg + 1)) + align8(join_scan_workspace_bytes(nseg));
}

GroupItems group_items(const int64_t* offsets, int64_t nseg, int64_t nperm, void* ws, size_t ws_size, hipStream_t s) {
  TFA_CHECK(nseg >= 1 && nperm >= 0, "group_items: bad segment or row count");
  TFA_CHECK(nseg < (int64_t(1) << 31) && nseg + max_chunks(nperm) < (int64_t(1) << 31),
            "group_items: too many segments");
  TFA_CHECK(offsets != nullptr && ws != nullptr && reinterpret_cast<uintptr_t>(ws) % 8 == 0,
            "group_items: null or unaligned buffer");
  TFA_CHECK(ws_size >= group_items_workspace_bytes(nseg), "group_items: workspace too small");
  char* w = static_cast<char*>(ws);
  int64_t* cnt = reinterpret_cast<int64_t*>(w);
  w += align8(8 * nseg);
  int64_t* coffs = reinterpret_cast<int64_t*>(w);
  w += align8(8 * (nseg + 1));
  const size_t scan_bytes = align8(join_scan_workspace_bytes(nseg));
  hipLaunchKernelGGL(group_chunk_count_kernel, dim3((unsigned)((nseg + kT - 1) / kT)), dim3(kT), 0, s, offsets, nseg,
                     nperm, cnt);
  TFA_LAUNCH_CHECK("group_chunk_count_kernel");
  GroupItems it;
  it.coffs = coffs;
  it.items = join_scan(cnt, nseg, max_chunks(nperm), coffs, w, scan_bytes, s);  // (synchronises)
  TFA_CHECK(it.items >= nseg && it.items <= nseg + max_chunks(nperm), "group_items: ", it.items, " work items for ",
            nseg, " segments of ", nperm, " rows");
  return it;
}

// workspace: group_items' (unused when the items are given) | records part[nseg + max_chunks][C]
// (items = sum over segments of max(1, ceil(len / chunk)) <= nseg + nperm / chunk)
size_t group_moments_workspace_bytes(int ncols, int64_t nperm, int64_t nseg) {
  if (nseg <= 0 || ncols <= 0) return 0;
  const size_t part = static_cast<size_t>(nseg + max_chunks(nperm)) * ncols * sizeof(GRec);
  return group_items_workspace_bytes(nseg) + part;
}

void group_moments(const StatCols& cols, int64_t n, const int64_t* perm, int64_t nperm, const int64_t* offsets,
                   int64_t nseg, int64_t* records, void* ws, size_t ws_size, hipStream_t s, const GroupItems* given) {
  TFA_CHECK(cols.n >= 1 && cols.n <= kMaxPackCols, "group_moments: 1..", kMaxPackCols, " columns, got ", cols.n);
  TFA_CHECK(n >= 0 && nperm >= 0 && nperm <= n && nseg >= 0, "group_moments: bad row or segment count");
  check_stat_columns("group_moments", cols, n);
  if (n == 0 || nseg == 0) return;
  TFA_CHECK(nseg < (int64_t(1) << 31) && nseg + max_chunks(nperm) < (int64_t(1) << 31),
            "group_moments: too many segments");
  TFA_CHECK(perm != nullptr && offsets != nullptr && records != nullptr && ws != nullptr, "group_moments: null buffer");
  TFA_CHECK(reinterpret_cast<uintptr_t>(records) % 8 == 0 && reinterpret_cast<uintptr_t>(ws) % 8 == 0,
            "group_moments: unaligned buffer");
  TFA_CHECK(ws_size >= group_moments_workspace_bytes(cols.n, nperm, nseg), "group_moments: workspace too small");
  const size_t items_bytes = group_items_workspace_bytes(nseg);
  const GroupItems it = given ? *given : group_items(offsets, nseg, nperm, ws, items_bytes, s);
  TFA_CHECK(it.coffs != nullptr && it.items >= nseg && it.items <= nseg + max_chunks(nperm),
            "group_moments: ", it.items, " work items for ", nseg, " segments of ", nperm, " rows");
  const int64_t items = it.items;
  int64_t* part = reinterpret_cast<int64_t*>(static_cast<char*>(ws) + items_bytes);
  const bool single = items == nseg;  // every segment is one chunk: item == segment
  hipLaunchKernelGGL(group_moments_kernel, dim3((unsigned)((items + kWaves - 1) / kWaves), cols.n), dim3(kT), 0, s,
                     cols, n, perm, nperm, offsets, (const int64_t*)it.coffs, nseg, items, single ? records : part);
  TFA_LAUNCH_CHECK("group_moments_kernel");
  if (single) return;
  hipLaunchKernelGGL(group_fold_kernel, dim3((unsigned)((nseg * cols.n + kT - 1) / kT)), dim3(kT), 0, s, cols,
                     (const int64_t*)part, (const int64_t*)it.coffs, nseg, items, records);
  TFA_LAUNCH_CHECK("group_fold_kernel");
}

// workspace: group_items' (unused when the items are given) | records part[nseg + max_chunks][Q]
size_t group_pair_moments_workspace_bytes(int npairs, int64_t nperm, int64_t nseg) {
  if (nseg <= 0 || npairs <= 0) return 0;
  const size_t part = static_cast<size_t>(nseg + max_chunks(nperm)) * npairs * (8 * kPairRecordFields);
  return group_items_workspace_bytes(nseg) + part;
}

void group_pair_moments(const StatCols& xs, const StatCols& ys, int64_t n, const int64_t* perm, int64_t nperm,
                        const int64_t* offsets, int64_t nseg, int64_t* records, void* ws, size_t ws_size,
                        hipStream_t s, const GroupItems* given) {
  TFA_CHECK(xs.n >= 1 && xs.n <= kMaxPackCols, "group_pair_moments: 1..", kMaxPackCols, " pairs, got ", xs.n);
  TFA_CHECK(xs.n == ys.n, "group_pair_moments: ", xs.n, " first columns, ", ys.n, " second columns");
  TFA_CHECK(n >= 0 && nperm >= 0 && nperm <= n && nseg >= 0, "group_pair_moments: bad row or segment count");
  check_stat_columns("group_pair_moments", xs, n);
  check_stat_columns("group_pair_moments", ys, n);
  if (n == 0 || nseg == 0) return;
  TFA_CHECK(nseg < (int64_t(1) << 31) && nseg + max_chunks(nperm) < (int64_t(1) << 31),
            "group_pair_moments: too many segments");
  TFA_CHECK(perm != nullptr && offsets != nullptr && records != nullptr && ws != nullptr,
            "group_pair_moments: null buffer");
  TFA_CHECK(reinterpret_cast<uintptr_t>(records) % 8 == 0 && reinterpret_cast<uintptr_t>(ws) % 8 == 0,
            "group_pair_moments: unaligned buffer");
  TFA_CHECK(ws_size >= group_pair_moments_workspace_bytes(xs.n, nperm, nseg),
            "group_pair_moments: workspace too small");
  const size_t items_bytes = group_items_workspace_bytes(nseg);
  const GroupItems it = given ? *given : group_items(offsets, nseg, nperm, ws, items_bytes, s);
  TFA_CHECK(it.coffs != nullptr && it.items >= nseg && it.items <= nseg + max_chunks(nperm),
            "group_pair_moments: ", it.items, " work items for ", nseg, " segments of ", nperm, " rows");
  const int64_t items = it.items;
  int64_t* part = reinterpret_cast<int64_t*>(static_cast<char*>(ws) + items_bytes);
  const bool single = items == nseg;  // every segment is one chunk: item == segment
  hipLaunchKernelGGL(group_pair_moments_kernel, dim3((unsigned)((items + kWaves - 1) / kWaves), xs.n), dim3(kT), 0, s,
                     xs, ys, n, perm, nperm, offsets, (const int64_t*)it.coffs, nseg, items, single ? records : part);
  TFA_LAUNCH_CHECK("group_pair_moments_kernel");
  if (single) return;
  hipLaunchKernelGGL(group_pair_fold_kernel, dim3((unsigned)((nseg * xs.n + kT - 1) / kT)), dim3(kT), 0, s, xs.n,
                     (const int64_t*)part, (const int64_t*)it.coffs, nseg, items, records);
  TFA_LAUNCH_CHECK("group_pair_fold_kernel");
}

void merge_pair_records(const int64_t* records, int64_t m, int npairs, const int64_t* offsets, int64_t ng,
                        int64_t* out, hipStream_t s) {
  TFA_CHECK(npairs >= 1 && npairs <= kMaxPackCols, "merge_pair_records: 1..", kMaxPackCols, " pairs, got ", npairs);
  TFA_CHECK(m >= 0 && ng >= 0, "merge_pair_records: negative count");
  if (ng == 0) return;
  TFA_CHECK(offsets != nullptr && out != nullptr && (m == 0 || records != nullptr), "merge_pair_records: null buffer");
  TFA_CHECK(ng * npairs < (int64_t(1) << 38), "merge_pair_records: too many groups");
  hipLaunchKernelGGL(merge_pair_records_kernel, dim3((unsigned)((ng * npairs + kT - 1) / kT)), dim3(kT), 0, s, records,
                     m, npairs, offsets, ng, out);
  TFA_LAUNCH_CHECK("merge_pair_records_kernel");
}

void pair_results(const int64_t* records, int64_t ng, int npairs, const PairResultSpec& spec, hipStream_t s) {
  TFA_CHECK(npairs >= 1 && npairs <= kMaxPackCols, "pair_results: 1..", kMaxPackCols, " pairs, got ", npairs);
  TFA_CHECK(spec.n >= 1 && spec.n <= kMaxPackCols, "pair_results: 1..", kMaxPackCols, " outputs, got ", spec.n);
  TFA_CHECK(ng >= 0, "pair_results: negative group count");
  for (int o = 0; o < spec.n; ++o) {
    TFA_CHECK(spec.pair[o] >= 0 && spec.pair[o] < npairs, "pair_results: output ", o, " names pair ", spec.pair[o],
              " of ", npairs);
    const int st = static_cast<int>(spec.stat[o]);
    TFA_CHECK(st >= 0 && st <= static_cast<int>(PairStat::COVAR_POP), "pair_results: output ", o,
              " asks for an unknown statistic");
    TFA_CHECK(ng == 0 || spec.out[o] != nullptr, "pair_results: output ", o, " has no buffer");
  }
  if (ng == 0) return;
  TFA_CHECK(records != nullptr, "pair_results: null records");
  TFA_CHECK((ng + kT - 1) / kT < (int64_t(1) << 31), "pair_results: too many groups");
  hipLaunchKernelGGL(pair_results_kernel, dim3((unsigned)((ng + kT - 1) / kT), spec.n), dim3(kT), 0, s, records, ng,
                     npairs, spec);
  TFA_LAUNCH_CHECK("pair_results_kernel");
}

void merge_group_records(const int64_t* records, int64_t m, int ncols, uint32_t float_mask, const int64_t* offsets,
                         int64_t ng, int64_t* out, hipStream_t s) {
  TFA_CHECK(ncols >= 1 && ncols <= kMaxPackCols, "merge_group_records: 1..", kMaxPackCols, " columns, got ", ncols);
  TFA_CHECK(m >= 0 && ng >= 0, "merge_group_records: negative count");
  if (ng == 0) return;
  TFA_CHECK(offsets != nullptr && out != nullptr && (m == 0 || records != nullptr), "merge_group_records: null buffer");
  TFA_CHECK(ng * ncols < (int64_t(1) << 38), "merge_group_records: too many groups");
  hipLaunchKernelGGL(merge_group_records_kernel, dim3((unsigned)((ng * ncols + kT - 1) / kT)), dim3(kT), 0, s, records,
                     m, ncols, float_mask, offsets, ng, out);
  TFA_LAUNCH_CHECK("merge_group_records_kernel");
}

void group_results(const int64_t* records, int64_t ng, int ncols, const GroupResultSpec& spec, hipStream_t s) {
  TFA_CHECK(ncols >= 1 && ncols <= kMaxPackCols, "group_results: 1..", kMaxPackCols, " columns, got ", ncols);
  TFA_CHECK(spec.n >= 1 && spec.n <= kMaxPackCols, "group_results: 1..", kMaxPackCols, " outputs, got ", spec.n);
  TFA_CHECK(ng >= 0, "group_results: negative group count");
  for (int o = 0; o < spec.n; ++o) {
    TFA_CHECK(spec.col[o] >= 0 && spec.col[o] < ncols, "group_results: output ", o, " names column ", spec.col[o],
              " of ", ncols);
    TFA_CHECK(is_stat_dtype(spec.dtype[o]), "group_results: output ", o, " has a dtype that is not supported");
    TFA_CHECK(static_cast<int>(spec.stat[o]) >= 0 && static_cast<int>(spec.stat[o]) <= static_cast<int>(GroupStat::STDDEV_POP),
              "group_results: output ", o, " asks for an unknown statistic");
    TFA_CHECK(ng == 0 || spec.out[o] != nullptr, "group_results: output ", o, " has no buffer");
  }
  if (ng == 0) return;
  TFA_CHECK(records != nullptr, "group_results: null records");
  TFA_CHECK((ng + kT - 1) / kT < (int64_t(1) << 31), "group_results: too many groups");
  hipLaunchKernelGGL(group_results_kernel, dim3((unsigned)((ng + kT - 1) / kT), spec.n), dim3(kT), 0, s, records, ng,
                     ncols, spec);
  TFA_LAUNCH_CHECK("group_results_kernel");
}

}  // namespace k
}  // namespace tfa
