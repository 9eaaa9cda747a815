// The weighted per-component summary of a vector column in one read
// (ml/stat.py: Summarizer).
//
// x is [n][d], row-major, f32 or f64, 1 <= d <= kVectorSummaryMaxD; w is null
// (every weight 1.0, through the same formulas) or [n] of one of the seven
// statistics dtypes. The record is a header {count, W, Q, bad weights} and
// eight fields [field][d] (kernels.h). Two launches, no float atomics, no block
// waits for another one:
//
//   1. vs_partial  grid = (groups of 256 components) x (slices of `slice_rows`
//                  rows). A thread owns one quad of 4 consecutive components on
//                  one row lane: lanes per row = the power of two at or above
//                  ceil(min(d, 256) / 4), rows per pass = 256 / lanes per row.
//                  It walks the rows of the slice that fall on its row lane in
//                  row order, four passes' loads issued before the four
//                  updates. A quad is one 16-byte load (f32) or two (f64) when
//                  d % 4 == 0 and the base is 16-byte aligned, else guarded
//                  scalar loads: the assignment of rows and components to
//                  threads is the same, so both give the same bits.
//                  Weights go through LDS: the block converts the weights of a
//                  tile of 1024 rows to f64 once (a negative, NaN or infinite
//                  one becomes NaN), one barrier, and every thread of a row
//                  reads that row's word. So a weight is read from memory once
//                  per block, not once per thread, and the two barriers fall
//                  once per 1024 rows, not once per pass. A row of weight 0 is
//                  skipped, a NaN word is counted and skipped; a row of
//                  positive weight enters by West's update (moments.h), its
//                  factor w / (W + w) formed once for the quad.
//                  Then the row lanes are merged by Chan's weighted merge in a
//                  halving tree through LDS: at each level the upper half of
//                  the live row lanes writes its records [field][thread], the
//                  lower half merges them in as the later side. Out:
//                  part [slice][8][d]; component group 0 also writes the
//                  slice's header hdr [slice][4].
//   2. vs_fold     one thread per component: the slices merged in slice order
//                  by the same merge; thread 0 folds the headers.
//
// Every row index is compared with the slice's end and every component index
// with d before an address is formed. The order of every operation depends on
// (n, d, slice_rows) alone: the same bits on every run.
#include <algorithm>
#include <cmath>

#include "column_types.h"
#include "hip_common.h"
#include "moments.h"

namespace tfa {
namespace k {

namespace {

constexpr int kT = 256;           // threads per block
constexpr int kGroup = 256;       // components per block
constexpr int kTileRows = 1024;   // rows whose weights are staged at once
constexpr int kAhead = 4;         // passes whose loads are issued together
constexpr int kTreeWords = 4 * kVectorSummaryFields + 4;  // a thread's four records, W, Q, count, bad weights
constexpr int kTargetBlocks = 512;     // the 256 CUs about twice over
constexpr int64_t kMinSliceRows = 4096;
constexpr size_t kMaxWorkspace = size_t(1) << 30;
static_assert(kTreeWords * (kT / 2) >= kTileRows, "the tree's LDS image also holds a tile of weights");

template <typename T>
struct Quad {  // four consecutive components of a row
  T v[4];
};

template <typename T, bool VEC>
__device__ __forceinline__ Quad<T> vs_load4(const T* __restrict__ p, int c0, int d) {
  Quad<T> q;
  if constexpr (VEC) {  // (d % 4 == 0 and c0 < d: the quad lies wholly inside the row)
    if constexpr (sizeof(T) == 4) {
      const float4 t = *reinterpret_cast<const float4*>(p);
      q.v[0] = t.x, q.v[1] = t.y, q.v[2] = t.z, q.v[3] = t.w;
    } else {
      const double2 t = *reinterpret_cast<const double2*>(p), u = *reinterpret_cast<const double2*>(p + 2);
      q.v[0] = t.x, q.v[1] = t.y, q.v[2] = u.x, q.v[3] = u.y;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) q.v[e] = c0 + e < d ? p[e] : T(0);
  }
  return q;
}

// what a row lane carries besides its four records
struct RowSums {
  double W, Q;
  uint64_t count, bad;
};

__device__ __forceinline__ uint64_t vs_bits(double x) { return static_cast<uint64_t>(__double_as_longlong(x)); }
__device__ __forceinline__ double vs_f64(uint64_t b) { return __longlong_as_double(static_cast<long long>(b)); }

// a record's fields in the order of the output; `put(field, bits)`
template <typename F>
__device__ __forceinline__ void vs_each_field(const SumRec& r, F&& put) {
  put(0, vs_bits(r.mean));
  put(1, vs_bits(r.m2));
  put(2, vs_bits(r.l1));
  put(3, vs_bits(r.s2));
  put(4, r.nnz);
  put(5, r.bad);
  put(6, r.lo);
  put(7, r.hi);
}

// the record whose field f is get(f)
template <typename F>
__device__ __forceinline__ SumRec vs_record(F&& get) {
  SumRec r;
  r.mean = vs_f64(get(0));
  r.m2 = vs_f64(get(1));
  r.l1 = vs_f64(get(2));
  r.s2 = vs_f64(get(3));
  r.nnz = get(4);
  r.bad = get(5);
  r.lo = get(6);
  r.hi = get(7);
  return r;
}

// `b`, the later side, merged into (rs, rec)
__device__ __forceinline__ void vs_merge_rows(RowSums& rs, const RowSums& b) {
  rs.W += b.W;
  rs.Q += b.Q;
  rs.count += b.count;
  rs.bad += b.bad;
}

// ------------------------------------------------------------------ 1. partial
template <typename T, bool VEC>
__global__ __launch_bounds__(kT) void vs_partial(const T* __restrict__ x, const void* __restrict__ w, DType wdtype,
                                                 int64_t n, int d, int groups, int lpr_log2, int64_t slice_rows,
                                                 int64_t* __restrict__ hdr, int64_t* __restrict__ part) {
  __shared__ uint64_t lds[kTreeWords * (kT / 2)];  // a tile of weights (f64 bits), then the tree's [word][thread]
  const int tid = threadIdx.x;
  const int lpr = 1 << lpr_log2, rpp = kT >> lpr_log2;  // lanes per row, rows per pass
  const int group = blockIdx.x % (unsigned)groups;
  const int64_t sl = blockIdx.x / (unsigned)groups;
  const int rl = tid >> lpr_log2;  // the row lane
  const int c0 = group * kGroup + (tid & (lpr - 1)) * 4;
  const bool active = c0 < d;
  const int64_t r0 = sl * slice_rows;
  const int64_t r1 = r0 + slice_rows < n ? r0 + slice_rows : n;

  SumRec rec[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) rec[e] = summary_empty();
  RowSums rs{0.0, 0.0, 0ull, 0ull};

  for (int64_t t0 = r0; t0 < r1; t0 += kTileRows) {
    const int rows = (int)(r1 - t0 < kTileRows ? r1 - t0 : kTileRows);
    for (int i = tid; i < rows; i += kT) {
      double wv = 1.0;
      if (w != nullptr) {
        const int64_t row = t0 + i;
        wv = dispatch_column(wdtype, [&](auto tag) {
          return static_cast<double>(static_cast<const decltype(tag)*>(w)[row]);
        });
        if (!(wv >= 0.0) || wv == __builtin_inf()) wv = __builtin_nan("");
      }
      lds[i] = vs_bits(wv);
    }
    __syncthreads();
    if (active) {
      const T* base = x + t0 * d + c0;
      for (int i0 = rl; i0 < rows; i0 += kAhead * rpp) {
        Quad<T> q[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
          const int i = i0 + k * rpp;
          if (i < rows) q[k] = vs_load4<T, VEC>(base + (int64_t)i * d, c0, d);
          else q[k].v[0] = q[k].v[1] = q[k].v[2] = q[k].v[3] = T(0);
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
          const int i = i0 + k * rpp;
          if (i >= rows) break;
          const double wv = vs_f64(lds[i]);
          if (wv > 0.0) {
            const double wn = rs.W + wv;
            const double f = wv / wn;
            rs.W = wn;
            rs.Q = __builtin_fma(wv, wv, rs.Q);
            rs.count += 1ull;
#pragma unroll
            for (int e = 0; e < 4; ++e) summary_add_row(rec[e], static_cast<double>(q[k].v[e]), wv, f);
          } else {
            rs.bad += wv != wv ? 1ull : 0ull;
          }
        }
      }
    }
    __syncthreads();  // (the image is free for the next tile, or for the tree)
  }

  // the row lanes merged in a halving tree: lanes [half, 2 half) write, lanes [0, half) merge them in
  constexpr int kPitch = kT / 2;
  for (int half = rpp >> 1; half >= 1; half >>= 1) {
    const int nthr = half << lpr_log2;
    if (tid >= nthr && tid < 2 * nthr) {
      uint64_t* p = lds + (tid - nthr);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        vs_each_field(rec[e], [&](int f, uint64_t b) { p[(e * kVectorSummaryFields + f) * kPitch] = b; });
      p[(kTreeWords - 4) * kPitch] = vs_bits(rs.W);
      p[(kTreeWords - 3) * kPitch] = vs_bits(rs.Q);
      p[(kTreeWords - 2) * kPitch] = rs.count;
      p[(kTreeWords - 1) * kPitch] = rs.bad;
    }
    __syncthreads();
    if (tid < nthr) {
      const uint64_t* p = lds + tid;
      const RowSums b{vs_f64(p[(kTreeWords - 4) * kPitch]), vs_f64(p[(kTreeWords - 3) * kPitch]),
                      p[(kTreeWords - 2) * kPitch], p[(kTreeWords - 1) * kPitch]};
      const double f = summary_fraction(rs.W, b.W);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const SumRec o = vs_record([&](int fld) { return p[(e * kVectorSummaryFields + fld) * kPitch]; });
        rec[e] = merge_summary(rs.W, rec[e], b.W, o, f);
      }
      vs_merge_rows(rs, b);
    }
    __syncthreads();
  }

  if (tid < lpr && active) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c0 + e < d) {
        int64_t* out = part + sl * kVectorSummaryFields * d + c0 + e;
        vs_each_field(rec[e], [&](int f, uint64_t b) { out[(int64_t)f * d] = static_cast<int64_t>(b); });
      }
    }
  }
  if (tid == 0 && group == 0) {
    int64_t* h = hdr + sl * kVectorSummaryHeader;
    h[0] = static_cast<int64_t>(rs.count);
    h[1] = __double_as_longlong(rs.W);
    h[2] = __double_as_longlong(rs.Q);
    h[3] = static_cast<int64_t>(rs.bad);
  }
}

// ------------------------------------------------------------------ 2. fold
__global__ __launch_bounds__(kT) void vs_fold(const int64_t* __restrict__ hdr, const int64_t* __restrict__ part,
                                              int64_t slices, int d, int64_t* __restrict__ record) {
  const int c = blockIdx.x * kT + threadIdx.x;
  if (c >= d) return;
  SumRec rec = summary_empty();
  RowSums rs{0.0, 0.0, 0ull, 0ull};
#pragma unroll 4
  for (int64_t s = 0; s < slices; ++s) {  // (slice order)
    const int64_t* h = hdr + s * kVectorSummaryHeader;
    const int64_t* p = part + s * kVectorSummaryFields * d + c;
    const RowSums b{__longlong_as_double(h[1]), __longlong_as_double(h[2]), static_cast<uint64_t>(h[0]),
                    static_cast<uint64_t>(h[3])};
    const SumRec o = vs_record([&](int f) { return static_cast<uint64_t>(p[(int64_t)f * d]); });
    rec = merge_summary(rs.W, rec, b.W, o, summary_fraction(rs.W, b.W));
    vs_merge_rows(rs, b);
  }
  int64_t* out = record + kVectorSummaryHeader + c;
  vs_each_field(rec, [&](int f, uint64_t b) { out[(int64_t)f * d] = static_cast<int64_t>(b); });
  if (c == 0) {
    record[0] = static_cast<int64_t>(rs.count);
    record[1] = __double_as_longlong(rs.W);
    record[2] = __double_as_longlong(rs.Q);
    record[3] = static_cast<int64_t>(rs.bad);
  }
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

VectorSummaryPlan vector_summary_plan(int64_t n, int d, int64_t slice_rows) {
  TFA_CHECK(n >= 1 && d >= 1 && d <= kVectorSummaryMaxD, "vector_summary: n >= 1 and 1 <= d <= ", kVectorSummaryMaxD,
            " expected, got n = ", n, ", d = ", d);
  VectorSummaryPlan p;
  p.groups = (d + kGroup - 1) / kGroup;
  const int quads = (std::min(d, kGroup) + 3) / 4;
  while ((1 << p.lpr_log2) < quads) ++p.lpr_log2;
  if (slice_rows <= 0) {
    const int64_t target = std::max<int64_t>(1, kTargetBlocks / p.groups);
    slice_rows = std::max(kMinSliceRows, ceil_div(ceil_div(n, target), kTileRows) * kTileRows);
  }
  p.slice_rows = slice_rows;
  p.slices = ceil_div(n, slice_rows);
  const double words = (double)p.slices * (kVectorSummaryHeader + (double)kVectorSummaryFields * d);
  TFA_CHECK(words * 8 <= (double)kMaxWorkspace && p.slices * p.groups < (int64_t(1) << 31),
            "vector_summary: slice_rows = ", slice_rows, " cuts ", n, " rows into ", p.slices,
            " slices, more than the workspace of ", kMaxWorkspace >> 20, " MB holds; use larger slices");
  p.workspace_bytes = static_cast<size_t>(words) * 8;
  return p;
}

void vector_summary(const void* x, DType dtype, const void* w, DType wdtype, int64_t n, int d,
                    const VectorSummaryPlan& p, int64_t* record, void* workspace, size_t workspace_size,
                    hipStream_t s) {
  TFA_CHECK(dtype == DType::F32 || dtype == DType::F64, "vector_summary: float32 or float64 cells expected");
  TFA_CHECK(w == nullptr || is_stat_dtype(wdtype), "vector_summary: the weights have a dtype that is not supported");
  TFA_CHECK(n >= 1 && d >= 1 && d <= kVectorSummaryMaxD && workspace_size >= p.workspace_bytes,
            "vector_summary: bad arguments");
  int64_t* hdr = static_cast<int64_t*>(workspace);
  int64_t* part = hdr + p.slices * kVectorSummaryHeader;
  const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const dim3 grid((unsigned)(p.slices * p.groups));
#define TFA_VS_PARTIAL(T_, VEC_)                                                                                  \
  hipLaunchKernelGGL((vs_partial<T_, VEC_>), grid, dim3(kT), 0, s, static_cast<const T_*>(x), w, wdtype, n, d,    \
                     p.groups, p.lpr_log2, p.slice_rows, hdr, part)
  if (dtype == DType::F32) {
    if (vec) TFA_VS_PARTIAL(float, true);
    else TFA_VS_PARTIAL(float, false);
  } else {
    if (vec) TFA_VS_PARTIAL(double, true);
    else TFA_VS_PARTIAL(double, false);
  }
#undef TFA_VS_PARTIAL
  TFA_LAUNCH_CHECK("vs_partial");
  hipLaunchKernelGGL(vs_fold, dim3((unsigned)((d + kT - 1) / kT)), dim3(kT), 0, s, hdr, part, p.slices, d, record);
  TFA_LAUNCH_CHECK("vs_fold");
}

}  // namespace k
}  // namespace tfa
