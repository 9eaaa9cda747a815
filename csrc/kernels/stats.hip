// Column statistics for DataFrame.describe / summary / approxQuantile.
//
//   moments  per column one record {n, mean, M2, smallest word, largest word}:
//            every element is converted to f64 and goes through Welford's
//            update in the lane that read it (the elements of one 16-byte
//            load together, as one batch); the lanes' records are merged
//            with Chan's formula in lane order (xor butterfly), the waves' in
//            wave order, and every block STORES its record; a second kernel
//            (one block per column) merges the blocks' records in block
//            order. No float atomics: the result depends on the row count and
//            the column's alignment alone, never on the run. Up to
//            kMaxPackCols columns of mixed dtypes in one launch pair (the
//            column is the grid's y).
//   pairs    per pair of columns one record {n, mean_x, mean_y, M2_x, M2_y,
//            C_xy, rows with a NaN or an infinity} (moments.h PairRec) for
//            corr / covar_samp / covar_pop: the structure of moments, the
//            pair on the grid's y. A lane takes runs of 16 consecutive rows of
//            both columns (whole 16-byte vectors of every dtype; a column
//            whose runs are not 16-byte aligned is read with scalar loads), a
//            run entering as one batch. The result depends on the row count
//            alone. Nothing is ever computed as sum(xy) - n mean_x mean_y.
//   hist     one step of a most-significant-digit-first radix select: for up
//            to kMaxPackCols word prefixes, the 256-bin histogram of the next
//            8-bit digit over the rows whose word starts with the prefix. The
//            word is computed from the raw element (sort_words.h); nothing of
//            [n] is written. Per-wave LDS histograms (ds_add) over the tiles a
//            block walks, folded per block, added to the result with 64-bit
//            integer atomics: exact counts whatever the order.
//
// Both read a column where it is: rows [lo, hi) are split into a scalar head
// up to the first 16-byte aligned element, 16-byte vector loads, and a scalar
// tail (fewer than 32 scalar rows in all, one per lane).
#include <algorithm>
#include <cmath>
#include <limits>

#include "column_types.h"
#include "hip_common.h"
#include "moments.h"
#include "radix.h"
#include "sort_words.h"

namespace tfa {
namespace k {

namespace {

constexpr int kT = 256;  // threads per block of every kernel here
constexpr int kWaves = kT / kWave;
constexpr int kMomentRows = 4096;       // fewest rows a moments block takes
constexpr int kMaxMomentBlocks = 1024;  // per column (the merge at a block's end is paid once per block)
constexpr int kMaxHistBlocks = 2048;

struct Rec {
  double n, mean, m2;
  uint64_t lo, hi;
};

__device__ __forceinline__ Rec rec_empty() { return Rec{0.0, 0.0, 0.0, ~0ull, 0ull}; }

// the block's record in thread 0: lanes in lane order (neighbours first), then
// the waves in wave order
__device__ __forceinline__ Rec block_merge(Rec r, Rec* lds /*[kWaves]*/) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  r = wave_merge_moments(r);
  if (lane == 0) lds[w] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < kWaves; ++i) r = merge_moments(r, lds[i]);
  }
  return r;
}

template <typename T>
struct Vec16 {
  static constexpr int V = 16 / sizeof(T);
  typedef T type __attribute__((ext_vector_type(16 / sizeof(T))));
};

// f(element) for the scalar head and tail and g(vector of V elements) for the
// aligned body of rows [lo, hi) of p (lo <= hi), the block's threads together
template <typename T, typename F, typename G>
__device__ __forceinline__ void for_rows(const T* __restrict__ p, int64_t lo, int64_t hi, F&& f, G&& g) {
  constexpr int V = Vec16<T>::V;
  using VT = typename Vec16<T>::type;
  const int tid = threadIdx.x;
  const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p + lo) & 15u);
  const int64_t head = static_cast<int64_t>(((16u - mis) & 15u) / sizeof(T));
  const int64_t v0 = lo + head < hi ? lo + head : hi;  // the first vector's row
  const int64_t nvec = (hi - v0) / V;
  const int64_t t0 = v0 + nvec * V;                    // the tail's first row
  const int nh = static_cast<int>(v0 - lo), ns = nh + static_cast<int>(hi - t0);  // (ns < 2 V <= 32)
  if (tid < ns) f(p[tid < nh ? lo + tid : t0 + (tid - nh)]);
  const VT* __restrict__ pv = reinterpret_cast<const VT*>(p + v0);
  int64_t v = tid;
  for (; v + 3 * kT < nvec; v += 4 * kT) {  // four independent loads in flight per lane
    const VT a = pv[v], b = pv[v + kT], c = pv[v + 2 * kT], d = pv[v + 3 * kT];
    g(a);
    g(b);
    g(c);
    g(d);
  }
  for (; v < nvec; v += kT) g(pv[v]);
}

// f(element) for rows [lo, hi)
template <typename T, typename F>
__device__ __forceinline__ void for_rows(const T* __restrict__ p, int64_t lo, int64_t hi, F&& f) {
  for_rows<T>(p, lo, hi, f, [&f](const typename Vec16<T>::type& x) {
#pragma unroll
    for (int j = 0; j < Vec16<T>::V; ++j) f(static_cast<T>(x[j]));
  });
}

// the extremes are tracked in a narrow key with the words' order and widened
// to the word once per lane: the value itself for the integers (sort_word is
// monotonic), the 32-bit word for float32
template <typename T>
struct ExtremeKey {
  typedef T K;
  static __device__ __forceinline__ K key(T v) { return v; }
  static __device__ __forceinline__ uint64_t word(K k) { return sort_word(k); }
};
template <>
struct ExtremeKey<float> {
  typedef uint32_t K;
  static __device__ __forceinline__ K key(float v) { return static_cast<uint32_t>(sort_word(v)); }
  static __device__ __forceinline__ uint64_t word(K k) { return k; }
};
template <>
struct ExtremeKey<double> {
  typedef uint64_t K;
  static __device__ __forceinline__ K key(double v) { return sort_word(v); }
  static __device__ __forceinline__ uint64_t word(K k) { return k; }
};

// One lane's record of the rows it reads. A scalar row is Welford's update;
// the V rows of one 16-byte load enter together, which is the same update in
// Chan's batched form (the batch's mean and squared deviations, then one
// merge): one division per load, not per row.
template <typename T>
__device__ __forceinline__ Rec lane_moments(const void* __restrict__ src, int64_t lo, int64_t hi) {
  constexpr int V = Vec16<T>::V;
  using VT = typename Vec16<T>::type;
  using EK = ExtremeKey<T>;
  using K = typename EK::K;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  K klo = std::numeric_limits<K>::max(), khi = std::numeric_limits<K>::lowest();
  for_rows<T>(
      static_cast<const T*>(src), lo, hi,
      [&](T v) {
        const double x = static_cast<double>(v);
        n += 1.0;
        const double d = x - mean;
        mean += d / n;
        m2 += d * (x - mean);
        const K k = EK::key(v);
        klo = k < klo ? k : klo;
        khi = k > khi ? k : khi;
      },
      [&](const VT& xv) {
        double x[V], s = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const T v = static_cast<T>(xv[j]);
          x[j] = static_cast<double>(v);
          s += x[j];
          const K k = EK::key(v);
          klo = k < klo ? k : klo;
          khi = k > khi ? k : khi;
        }
        const double bm = s * (1.0 / V);  // (V is a power of two)
        double b2 = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const double d = x[j] - bm;
          b2 = fma(d, d, b2);
        }
        const double tot = n + V;
        const double f = V / tot;
        const double delta = bm - mean;
        mean += delta * f;
        m2 += b2 + ((n * f) * delta) * delta;  // (n == 0: nothing of delta, however large)
        n = tot;
      });
  Rec r = rec_empty();
  if (n > 0.0) r = Rec{n, mean, m2, EK::word(klo), EK::word(khi)};
  return r;
}

}  // namespace

// block (b, c): rows [b * chunk, min(n, (b + 1) * chunk)) of column c -> part[c][b]
__global__ __launch_bounds__(kT) void moments_partial_kernel(StatCols cols, int64_t n, int64_t chunk,
                                                             Rec* __restrict__ part) {
  __shared__ Rec lds[kWaves];
  const int c = blockIdx.y;
  const int64_t first = (int64_t)blockIdx.x * chunk;
  const int64_t lo = first < n ? first : n;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  const void* src = cols.ptr[c];
  // (the dtype is uniform: one scalar branch per block)
  Rec r = dispatch_column(cols.dtype[c], [&](auto tag) { return lane_moments<decltype(tag)>(src, lo, hi); });
  r = block_merge(r, lds);
  if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = r;
}

// block c: part[c][0 .. nb) merged in block order -> moments[c], extremes[c]
__global__ __launch_bounds__(kT) void moments_final_kernel(const Rec* __restrict__ part, int nb,
                                                           double* __restrict__ moments,
                                                           int64_t* __restrict__ extremes) {
  __shared__ Rec lds[kWaves];
  const int c = blockIdx.x;
  const Rec* __restrict__ p = part + (int64_t)c * nb;
  const int per = (nb + kT - 1) / kT;  // consecutive records per thread
  const int a = threadIdx.x * per, b = a + per < nb ? a + per : nb;
  Rec r = rec_empty();
  for (int i = a; i < b; ++i) r = merge_moments(r, p[i]);
  r = block_merge(r, lds);
  if (threadIdx.x == 0) {
    moments[3 * c] = r.n;
    moments[3 * c + 1] = r.mean;
    moments[3 * c + 2] = r.m2;
    extremes[2 * c] = static_cast<int64_t>(r.lo);
    extremes[2 * c + 1] = static_cast<int64_t>(r.hi);
  }
}

// ------------------------------------------------------------------ pairs
namespace {

// The two columns of a pair differ in element width and alignment: a lane
// takes runs of kRun consecutive rows of both, whole 16-byte vectors of every
// dtype (1 for the one-byte types, 8 for the eight-byte ones).
constexpr int kRun = 16;

// rows [lo, ..) of the column start on a 16-byte boundary (lo: uniform)
template <typename T>
__device__ __forceinline__ bool run_aligned(const void* __restrict__ src, int64_t lo) {
  return (reinterpret_cast<uintptr_t>(static_cast<const T*>(src) + lo) & 15u) == 0;
}

// rows [r0, r0 + kRun) as f64: every load is issued before the first use
// (kRun * sizeof(T) / 16 vector loads where `vec`, kRun scalar ones otherwise)
template <typename T>
__device__ __forceinline__ void load_run(const void* __restrict__ src, int64_t r0, bool vec, double (&v)[kRun]) {
  constexpr int V = Vec16<T>::V;
  using VT = typename Vec16<T>::type;
  const T* __restrict__ p = static_cast<const T*>(src) + r0;
  if (vec) {
    const VT* __restrict__ pv = reinterpret_cast<const VT*>(p);
    VT t[kRun / V];
#pragma unroll
    for (int j = 0; j < kRun / V; ++j) t[j] = pv[j];
#pragma unroll
    for (int j = 0; j < kRun / V; ++j) {
#pragma unroll
      for (int i = 0; i < V; ++i) v[j * V + i] = static_cast<double>(static_cast<T>(t[j][i]));
    }
  } else {
    T t[kRun];
#pragma unroll
    for (int j = 0; j < kRun; ++j) t[j] = p[j];
#pragma unroll
    for (int j = 0; j < kRun; ++j) v[j] = static_cast<double>(t[j]);
  }
}

template <typename T>
__device__ __forceinline__ double load_row(const void* __restrict__ src, int64_t r) {
  return static_cast<double>(static_cast<const T*>(src)[r]);
}

// The kRun rows of one run enter together, as the V rows of one load do in
// lane_moments: the run's means, squared deviations and co-deviations, then
// one merge in Chan's form (one division per run, not three per row).
__device__ __forceinline__ void pair_add_run(PairRec& r, const double (&x)[kRun], const double (&y)[kRun]) {
  double sx[4] = {0.0, 0.0, 0.0, 0.0}, sy[4] = {0.0, 0.0, 0.0, 0.0};
  uint64_t bad = 0;
#pragma unroll
  for (int j = 0; j < kRun; ++j) {
    sx[j & 3] += x[j];
    sy[j & 3] += y[j];
    bad += (__builtin_isfinite(x[j]) && __builtin_isfinite(y[j])) ? 0ull : 1ull;
  }
  const double bmx = ((sx[0] + sx[1]) + (sx[2] + sx[3])) * (1.0 / kRun);  // (kRun is a power of two)
  const double bmy = ((sy[0] + sy[1]) + (sy[2] + sy[3])) * (1.0 / kRun);
  double b2x[2] = {0.0, 0.0}, b2y[2] = {0.0, 0.0}, bc[2] = {0.0, 0.0};
#pragma unroll
  for (int j = 0; j < kRun; ++j) {
    const double dx = x[j] - bmx, dy = y[j] - bmy;
    b2x[j & 1] = fma(dx, dx, b2x[j & 1]);
    b2y[j & 1] = fma(dy, dy, b2y[j & 1]);
    bc[j & 1] = fma(dx, dy, bc[j & 1]);
  }
  const double tot = r.n + kRun;
  const double f = kRun / tot;
  const double dx = bmx - r.mx, dy = bmy - r.my;
  const double w = r.n * f;  // (n == 0: nothing of the deltas, however large)
  r.mx += dx * f;
  r.my += dy * f;
  r.m2x += (b2x[0] + b2x[1]) + (w * dx) * dx;
  r.m2y += (b2y[0] + b2y[1]) + (w * dy) * dy;
  r.cxy += (bc[0] + bc[1]) + (w * dx) * dy;
  r.n = tot;
  r.bad += bad;
}

// the block's pair record in thread 0: lanes in lane order, then the waves in
// wave order
__device__ __forceinline__ PairRec block_merge_pairs(PairRec r, PairRec* lds /*[kWaves]*/) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  r = wave_merge_pairs(r);
  if (lane == 0) lds[w] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < kWaves; ++i) r = merge_pairs(r, lds[i]);
  }
  return r;
}

}  // namespace

// block (b, q): rows [b * chunk, min(n, (b + 1) * chunk)) of pair q -> part[q][b].
// chunk is a multiple of kRun. Thread t takes the runs t, t + kT, ...; the
// rows after the last whole run (fewer than kRun, in the last block alone) go
// one to a thread, through Welford's update. Whether a column's runs are read
// as vectors is decided per block from the address of its first row.
__global__ __launch_bounds__(kT) void pair_moments_partial_kernel(StatCols xs, StatCols ys, int64_t n, int64_t chunk,
                                                                  PairRec* __restrict__ part) {
  __shared__ PairRec lds[kWaves];
  const int q = blockIdx.y;
  const int64_t first = (int64_t)blockIdx.x * chunk;
  const int64_t lo = first < n ? first : n;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  const void* px = xs.ptr[q];
  const void* py = ys.ptr[q];
  const DType tx = xs.dtype[q], ty = ys.dtype[q];
  // (dtypes and alignments are uniform: scalar branches)
  const bool vx = dispatch_column(tx, [&](auto tag) { return run_aligned<decltype(tag)>(px, lo); });
  const bool vy = dispatch_column(ty, [&](auto tag) { return run_aligned<decltype(tag)>(py, lo); });
  const int64_t nrun = (hi - lo) / kRun;
  PairRec r = pair_empty();
  for (int64_t j = threadIdx.x; j < nrun; j += kT) {
    const int64_t r0 = lo + j * kRun;
    double x[kRun], y[kRun];
    dispatch_column(tx, [&](auto tag) { load_run<decltype(tag)>(px, r0, vx, x); });
    dispatch_column(ty, [&](auto tag) { load_run<decltype(tag)>(py, r0, vy, y); });
    pair_add_run(r, x, y);
  }
  const int64_t t0 = lo + nrun * kRun + threadIdx.x;
  if (t0 < hi) {
    const double x = dispatch_column(tx, [&](auto tag) { return load_row<decltype(tag)>(px, t0); });
    const double y = dispatch_column(ty, [&](auto tag) { return load_row<decltype(tag)>(py, t0); });
    pair_add_row(r, x, y);
  }
  r = block_merge_pairs(r, lds);
  if (threadIdx.x == 0) part[(int64_t)q * gridDim.x + blockIdx.x] = r;
}

// block q: part[q][0 .. nb) merged in block order -> records[q]
__global__ __launch_bounds__(kT) void pair_moments_final_kernel(const PairRec* __restrict__ part, int nb,
                                                                int64_t* __restrict__ records) {
  __shared__ PairRec lds[kWaves];
  const int q = blockIdx.x;
  const PairRec* __restrict__ p = part + (int64_t)q * nb;
  const int per = (nb + kT - 1) / kT;  // consecutive records per thread
  const int a = threadIdx.x * per, b = a + per < nb ? a + per : nb;
  PairRec r = pair_empty();
  for (int i = a; i < b; ++i) r = merge_pairs(r, p[i]);
  r = block_merge_pairs(r, lds);
  if (threadIdx.x == 0) store_pair(records + (int64_t)q * kPairRecordFields, r);
}

namespace {

struct HistPrefixes {
  uint64_t v[kMaxPackCols];
};

// h: this wave's [P][256] counters
template <typename T>
__device__ __forceinline__ void hist_column(const void* __restrict__ src, int64_t n, const HistPrefixes& pre, int P,
                                            int prefix_bits, uint32_t* h) {
  const T* __restrict__ p = static_cast<const T*>(src);
  const int shift = 64 - radix::kBits - prefix_bits;  // of the digit
  const int above = 64 - prefix_bits;                 // of the prefix (unused when there is none)
  const int64_t ntiles = (n + radix::kTile - 1) / radix::kTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t lo = t * radix::kTile;
    const int64_t hi = lo + radix::kTile < n ? lo + radix::kTile : n;
    if (prefix_bits == 0) {
      for_rows<T>(p, lo, hi, [=](T v) { atomicAdd(&h[(sort_word(v) >> shift) & (radix::kRadix - 1)], 1u); });
    } else {
      for_rows<T>(p, lo, hi, [=, &pre](T v) {
        const uint64_t w = sort_word(v);
        const uint32_t d = static_cast<uint32_t>(w >> shift) & (radix::kRadix - 1);
        for (int q = 0; q < P; ++q)
          if (((w ^ pre.v[q]) >> above) == 0) atomicAdd(&h[q * radix::kRadix + d], 1u);
      });
    }
  }
}

}  // namespace

// dynamic LDS: uint32 [kWaves][P][256] (64 KiB at P = 16). hist is zeroed
// before. The prefixes travel as kernel arguments (uniform: scalar registers).
__global__ __launch_bounds__(kT) void select_hist_kernel(DType dtype, const void* __restrict__ src, int64_t n,
                                                         HistPrefixes pre, int P, int prefix_bits,
                                                         unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  const int bins = P * radix::kRadix;
  for (int i = threadIdx.x; i < kWaves * bins; i += kT) dyn[i] = 0;
  __syncthreads();
  uint32_t* h = dyn + (threadIdx.x / kWave) * bins;
  dispatch_column(dtype, [&](auto tag) { hist_column<decltype(tag)>(src, n, pre, P, prefix_bits, h); });  // (uniform)
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += kT) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += dyn[w * bins + i];
    if (c) atomicAdd(&hist[i], static_cast<unsigned long long>(c));
  }
}

// ------------------------------------------------------------------ host API
namespace {

// blocks per column and rows per block (a multiple of 16: blocks of an aligned
// column start aligned)
void moments_grid(int64_t n, int* nb, int64_t* chunk) {
  int64_t b = std::min<int64_t>(kMaxMomentBlocks, (n + kMomentRows - 1) / kMomentRows);
  b = std::max<int64_t>(b, 1);
  int64_t c = ((n + b - 1) / b + 15) & ~int64_t(15);
  c = std::max<int64_t>(c, 16);
  *chunk = c;
  *nb = static_cast<int>(std::max<int64_t>(1, (n + c - 1) / c));
}

}  // namespace

int stats_tile_rows() { return radix::kTile; }

size_t column_moments_workspace_bytes(int ncols, int64_t n) {
  if (n <= 0 || ncols <= 0) return 0;
  int nb;
  int64_t chunk;
  moments_grid(n, &nb, &chunk);
  return radix::align_up(static_cast<size_t>(ncols) * nb * sizeof(Rec));
}

void column_moments(const StatCols& cols, int64_t n, double* moments, int64_t* extremes, void* ws, size_t ws_size,
                    hipStream_t s) {
  TFA_CHECK(cols.n >= 1 && cols.n <= kMaxPackCols, "column_moments: 1..", kMaxPackCols, " columns, got ", cols.n);
  TFA_CHECK(n >= 0, "column_moments: negative row count");
  check_stat_columns("column_moments", cols, n);
  if (n == 0) return;
  TFA_CHECK(moments != nullptr && extremes != nullptr && ws != nullptr, "column_moments: null buffer");
  TFA_CHECK(reinterpret_cast<uintptr_t>(moments) % 8 == 0 && reinterpret_cast<uintptr_t>(extremes) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(ws) % 8 == 0, "column_moments: unaligned buffer");
  TFA_CHECK(ws_size >= column_moments_workspace_bytes(cols.n, n), "column_moments: workspace too small");
  int nb;
  int64_t chunk;
  moments_grid(n, &nb, &chunk);
  Rec* part = static_cast<Rec*>(ws);
  hipLaunchKernelGGL(moments_partial_kernel, dim3(nb, cols.n), dim3(kT), 0, s, cols, n, chunk, part);
  TFA_LAUNCH_CHECK("moments_partial_kernel");
  hipLaunchKernelGGL(moments_final_kernel, dim3(cols.n), dim3(kT), 0, s, (const Rec*)part, nb, moments, extremes);
  TFA_LAUNCH_CHECK("moments_final_kernel");
}

size_t column_pair_moments_workspace_bytes(int npairs, int64_t n) {
  if (n <= 0 || npairs <= 0) return 0;
  int nb;
  int64_t chunk;
  moments_grid(n, &nb, &chunk);
  return radix::align_up(static_cast<size_t>(npairs) * nb * sizeof(PairRec));
}

void column_pair_moments(const StatCols& xs, const StatCols& ys, int64_t n, int64_t* records, void* ws, size_t ws_size,
                         hipStream_t s) {
  TFA_CHECK(xs.n >= 1 && xs.n <= kMaxPackCols, "column_pair_moments: 1..", kMaxPackCols, " pairs, got ", xs.n);
  TFA_CHECK(xs.n == ys.n, "column_pair_moments: ", xs.n, " first columns, ", ys.n, " second columns");
  TFA_CHECK(n >= 0, "column_pair_moments: negative row count");
  check_stat_columns("column_pair_moments", xs, n);
  check_stat_columns("column_pair_moments", ys, n);
  if (n == 0) return;
  TFA_CHECK(records != nullptr && ws != nullptr, "column_pair_moments: null buffer");
  TFA_CHECK(reinterpret_cast<uintptr_t>(records) % 8 == 0 && reinterpret_cast<uintptr_t>(ws) % 8 == 0,
            "column_pair_moments: unaligned buffer");
  TFA_CHECK(ws_size >= column_pair_moments_workspace_bytes(xs.n, n), "column_pair_moments: workspace too small");
  int nb;
  int64_t chunk;
  moments_grid(n, &nb, &chunk);  // (chunk: a multiple of 16 == kRun)
  static_assert(kRun == 16, "moments_grid rounds a block's rows to 16");
  PairRec* part = static_cast<PairRec*>(ws);
  hipLaunchKernelGGL(pair_moments_partial_kernel, dim3(nb, xs.n), dim3(kT), 0, s, xs, ys, n, chunk, part);
  TFA_LAUNCH_CHECK("pair_moments_partial_kernel");
  hipLaunchKernelGGL(pair_moments_final_kernel, dim3(xs.n), dim3(kT), 0, s, (const PairRec*)part, nb, records);
  TFA_LAUNCH_CHECK("pair_moments_final_kernel");
}

void select_hist(DType dtype, const void* col, int64_t n, const int64_t* prefixes, int P, int prefix_bits,
                 int64_t* hist, hipStream_t s) {
  TFA_CHECK(is_stat_dtype(dtype), "select_hist: the column has a dtype that is not supported");
  TFA_CHECK(P >= 1 && P <= kMaxPackCols, "select_hist: 1..", kMaxPackCols, " prefixes, got ", P);
  TFA_CHECK(prefix_bits >= 0 && prefix_bits <= 64 - radix::kBits && prefix_bits % radix::kBits == 0,
            "select_hist: prefix_bits must be one of 0, 8, ..., 56, got ", prefix_bits);
  TFA_CHECK(prefix_bits != 0 || P == 1, "select_hist: without a prefix there is one histogram, got ", P);
  TFA_CHECK(n >= 0 && n < (int64_t(1) << 40), "select_hist: 0..2^40-1 rows, got ", n);
  TFA_CHECK(n == 0 || col != nullptr, "select_hist: the column has no data");
  TFA_CHECK(reinterpret_cast<uintptr_t>(col) % static_cast<uintptr_t>(dtype_size(dtype)) == 0,
            "select_hist: the column is not aligned to its element size");
  TFA_CHECK(prefixes != nullptr && hist != nullptr && reinterpret_cast<uintptr_t>(hist) % 8 == 0,
            "select_hist: bad prefix or histogram buffer");
  const size_t bins = static_cast<size_t>(P) * radix::kRadix;
  TFA_CHECK(hipMemsetAsync(hist, 0, bins * 8, s) == hipSuccess, "select_hist: memset failed");
  if (n == 0) return;
  const int grid = static_cast<int>(std::min<int64_t>(kMaxHistBlocks, radix::tiles(n)));
  const size_t lds = kWaves * bins * sizeof(uint32_t);
  HistPrefixes pre = {};
  for (int q = 0; q < P; ++q) pre.v[q] = static_cast<uint64_t>(prefixes[q]);
  hipLaunchKernelGGL(select_hist_kernel, dim3(grid), dim3(kT), lds, s, dtype, col, n, pre, P, prefix_bits,
                     reinterpret_cast<unsigned long long*>(hist));
  TFA_LAUNCH_CHECK("select_hist_kernel");
}

}  // namespace k
}  // namespace tfa
