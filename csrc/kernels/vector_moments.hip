// Mean vector and centred Gram matrix of a vector column (ml/stat.py:
// Correlation.corr / Correlation.cov).
//
// x is [n][d], row-major, f32 or f64, 1 <= d <= kVectorMomentsMaxD. The result
// is mean [d] and C [d][d] = sum_r (x_r - mean)(x_r - mean)^T, both f64, C
// exactly symmetric. Three launches, no float atomics, no block waits for
// another one:
//
//   1. vm_means   the rows are cut into `mean_chunks` chunks of
//                 `mean_chunk_rows` rows. A block takes one chunk of up to 64
//                 columns: a thread adds the rows of its column it meets with
//                 stride 256 / lanes-per-row in row order, the row lanes are
//                 folded in lane order. Out: mpart [chunk][d] (sums of x).
//   2. vm_syrk    the output is cut into 64x64 feature tiles; only the tile
//                 pairs bi <= bj are launched, each for every slice of
//                 `slice_rows` rows (grid = pairs x slices). A block first
//                 folds the chunk sums of its 128 features in chunk order and
//                 divides by n: the shift s, the partition's own mean to
//                 within rounding. Then, per stage of 32 rows: the bi and the
//                 bj segment of every row (64 consecutive elements each) are
//                 read in 16-byte loads (scalar loads when the base or d does
//                 not allow them), converted to f64, shifted once and written
//                 to an LDS image [row][feature] (two stages deep; rows past
//                 the slice and features past d as 0.0). With A = Xc^T both
//                 operands of v_mfma_f64_16x16x4_f64 are the same read
//                 pattern of that image: lane l takes xc[r0 + l / 16][f0 + l %
//                 16], 16 consecutive features of 4 consecutive rows. A row
//                 group reads 128 contiguous bytes, half of the 64 four-byte
//                 banks; the row pitch of 144 doubles = 1152 bytes is 128
//                 (mod 256), so row groups 0 and 1 (lanes 0..31) fall on
//                 disjoint halves of the banks, as do groups 2 and 3, while
//                 groups 0 and 2 share theirs: free of conflicts if the
//                 8-byte read is served 32 lanes at a time (by this
//                 arithmetic, not by a counter measurement).
//                 Four waves, one 32x32 quadrant each as 2x2
//                 MFMA tiles; on a diagonal pair the bj segment is neither
//                 read nor stored (both operands come from the bi image) and
//                 the MFMA tiles below the diagonal are skipped, as are tiles
//                 that lie wholly past d. The next stage's global loads are
//                 issued before the current stage's MFMAs. Out: the block's
//                 64x64 partial [slice][pair][64 * 64]; diagonal pairs also
//                 write the column sums of the centred values [slice][feature]
//                 (a thread owns four features for the whole slice: its rows
//                 in row order, then the eight row groups in group order).
//   3. vm_finish  one thread per element i <= j: the partials folded in slice
//                 order, minus the correction n m_i m_j, where m = (the column
//                 sums of the centred values folded in slice order) / n is
//                 carried rather than assumed zero: the shift is a rounded
//                 mean, and with |mean| >> stddev what rounding left in it is
//                 not negligible against C. The thread writes C_ij and its
//                 mirror C_ji; the threads of the diagonal write mean_i = s_i
//                 + m_i. A component whose shift is not finite (a NaN or an
//                 infinity among its values) gets a NaN row and column.
//
// The order of the additions depends on (n, d, slice_rows) alone: the same
// bits on every run. Every row index is compared with the slice's end and
// every feature index with d before an address is formed.
#include <algorithm>
#include <cmath>

#include "hip_common.h"

namespace tfa {
namespace k {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kT = 256;          // threads per block
constexpr int kTileF = 64;       // features per tile
constexpr int kStage = 32;       // rows per stage (the multiple slice_rows comes in)
constexpr int kPitch = 2 * kTileF + 16;  // doubles per LDS row: 144 = 16 (mod 32), consecutive rows 128 bytes (mod 256) apart
constexpr int kTileElems = kTileF * kTileF;
constexpr size_t kSyrkLds = (2 * kStage * kPitch + 2 * kTileF) * sizeof(double);  // two stages and the 128 shifts
constexpr int kTargetBlocks = 512;     // the 256 CUs about twice over
constexpr int64_t kMinSliceRows = 256;
constexpr int64_t kMinChunkRows = 1024;
constexpr size_t kMaxWorkspace = size_t(1) << 30;

// ------------------------------------------------------------------ 1. means
template <typename T>
__global__ __launch_bounds__(kT) void vm_means(const T* __restrict__ x, int64_t n, int d, int lpr_log2,
                                               int64_t chunk_rows, double* __restrict__ mpart) {
  __shared__ double red[kT];
  const int tid = threadIdx.x;
  const int lpr = 1 << lpr_log2, rpb = kT >> lpr_log2;  // lanes per row, rows per block pass
  const int col = blockIdx.x * lpr + (tid & (lpr - 1));
  const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
  const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
  double acc = 0.0;
  if (col < d) {
#pragma unroll 4
    for (int64_t r = r0 + (tid >> lpr_log2); r < r1; r += rpb) acc += (double)x[r * d + col];
  }
  red[tid] = acc;
  __syncthreads();
  if (tid < lpr && col < d) {
    double t = 0.0;
    for (int j = 0; j < rpb; ++j) t += red[j * lpr + tid];  // (lane order)
    mpart[(int64_t)blockIdx.y * d + col] = t;
  }
}

// the fold of the chunk sums of feature f, over n: the shift (vm_syrk and vm_finish: the same bits)
__device__ __forceinline__ double vm_shift(const double* __restrict__ mpart, int chunks, int d, int f, int64_t n) {
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += mpart[(int64_t)c * d + f];
  return s / (double)n;
}

// ------------------------------------------------------------------ 2. centred SYRK
template <typename T>
struct Quad {  // four consecutive elements of a row
  T v[4];
};

template <typename T, bool VEC>
__device__ __forceinline__ Quad<T> vm_load4(const T* __restrict__ p, int f0, int d) {
  Quad<T> q;
  if constexpr (VEC) {  // (d % 4 == 0: a quad lies wholly inside or outside the row)
    if (f0 < d) {
      if constexpr (sizeof(T) == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        q.v[0] = t.x, q.v[1] = t.y, q.v[2] = t.z, q.v[3] = t.w;
      } else {
        const double2 t = *reinterpret_cast<const double2*>(p), u = *reinterpret_cast<const double2*>(p + 2);
        q.v[0] = t.x, q.v[1] = t.y, q.v[2] = u.x, q.v[3] = u.y;
      }
    } else {
      q.v[0] = q.v[1] = q.v[2] = q.v[3] = T(0);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) q.v[e] = f0 + e < d ? p[e] : T(0);
  }
  return q;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kT) void vm_syrk(const T* __restrict__ x, int64_t n, int d, int tiles, int pairs,
                                              int64_t slice_rows, const double* __restrict__ mpart, int chunks,
                                              double* __restrict__ colsum, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double lds[];  // [2][kStage][kPitch], then the 128 shifts
  double* shift_lds = lds + 2 * kStage * kPitch;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int pair = blockIdx.x % (unsigned)pairs;
  const int64_t sl = blockIdx.x / (unsigned)pairs;
  int bi = 0, bj = pair;  // pair -> (bi <= bj), row by row of the upper triangle
  while (bj >= tiles - bi) {
    bj -= tiles - bi;
    ++bi;
  }
  bj += bi;
  const bool diag = bi == bj;
  const int64_t r_begin = sl * slice_rows;
  const int64_t r_end = r_begin + slice_rows < n ? r_begin + slice_rows : n;

  if (tid < 2 * kTileF) {
    const int f = (tid < kTileF ? bi * kTileF : bj * kTileF - kTileF) + tid;
    shift_lds[tid] = f < d ? vm_shift(mpart, chunks, d, f, n) : 0.0;
  }
  __syncthreads();

  // staging: thread -> quad q of the 32 quads of a row image (16 of the bi
  // segment, 16 of the bj segment) and rows g, g + 8, g + 16, g + 24 of a stage
  const int q = tid & 31, g = tid >> 5;
  const bool seg_b = q >= 16;
  const int f0 = (seg_b ? bj : bi) * kTileF + (q & 15) * 4;
  const bool active = !(diag && seg_b);  // a diagonal pair has one segment
  double sh[4], csum[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sh[e] = shift_lds[q * 4 + e];
    csum[e] = 0.0;
  }
  Quad<T> raw[4];
  auto load = [&](int64_t row0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t row = row0 + g + 8 * k;
      if (active && row < r_end) {
        raw[k] = vm_load4<T, VEC>(x + row * d + f0, f0, d);
      } else {
        raw[k].v[0] = raw[k].v[1] = raw[k].v[2] = raw[k].v[3] = T(0);
      }
    }
  };
  auto store = [&](int64_t row0, int buf) __attribute__((always_inline)) {
    if (!active) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool row_ok = row0 + g + 8 * k < r_end;
      double v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = (row_ok && f0 + e < d) ? (double)raw[k].v[e] - sh[e] : 0.0;  // (padding is 0.0, not 0 - shift)
        csum[e] += v[e];
      }
      double* p = lds + (buf * kStage + g + 8 * k) * kPitch + q * 4;
      *reinterpret_cast<double2*>(p) = double2{v[0], v[1]};
      *reinterpret_cast<double2*>(p + 2) = double2{v[2], v[3]};
    }
  };

  // which of the wave's 2x2 MFMA tiles hold anything: not wholly past d, and
  // on a diagonal pair not below the diagonal (vm_finish reads i <= j only)
  bool en[2][2];
  bool any = false;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ti = wm * 2 + i, tj = wn * 2 + j;
      en[i][j] = bi * kTileF + ti * 16 < d && bj * kTileF + tj * 16 < d && !(diag && ti > tj);
      any = any || en[i][j];
    }
  const int a_off = wm * 32 + (lane & 15), b_off = (diag ? 0 : kTileF) + wn * 32 + (lane & 15);
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int64_t stages = (r_end - r_begin + kStage - 1) / kStage;
  load(r_begin);
  store(r_begin, 0);
  __syncthreads();
  for (int64_t st = 0; st < stages; ++st) {
    const int cur = (int)(st & 1);
    const bool more = st + 1 < stages;
    const int64_t next0 = r_begin + (st + 1) * kStage;
    if (more) load(next0);  // in flight under the MFMAs
    if (any) {
      const double* img = lds + (cur * kStage + (lane >> 4)) * kPitch;
#pragma unroll
      for (int kk = 0; kk < kStage / 4; ++kk) {
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = img[kk * 4 * kPitch + a_off + i * 16];
          b[i] = img[kk * 4 * kPitch + b_off + i * 16];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (en[i][j]) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    if (more) store(next0, cur ^ 1);  // (every wave left that image before the previous barrier)
    __syncthreads();
  }

  // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
  double* out = partial + (sl * pairs + pair) * kTileElems;
  static_for<2>([&](auto ic) __attribute__((always_inline)) {
    constexpr int i = decltype(ic)::value;
    static_for<2>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      const f64x4 v = acc[i][j];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(wm * 32 + i * 16 + (lane >> 4) + 4 * r) * kTileF + wn * 32 + j * 16 + (lane & 15)] = v[r];
    });
  });

  if (diag) {  // the column sums of the centred values of this tile's features
    double* red = lds;  // [8][kTileF] (the last barrier of the loop freed the images)
    if (active) {
#pragma unroll
      for (int e = 0; e < 4; ++e) red[g * kTileF + q * 4 + e] = csum[e];
    }
    __syncthreads();
    if (tid < kTileF) {
      double t = 0.0;
      for (int j = 0; j < kT / 32; ++j) t += red[j * kTileF + tid];  // (row group order)
      colsum[(sl * tiles + bi) * kTileF + tid] = t;
    }
  }
}

// ------------------------------------------------------------------ 3. finish
__global__ __launch_bounds__(kT) void vm_finish(int64_t n, int d, int tiles, int pairs, int64_t slices,
                                                const double* __restrict__ mpart, int chunks,
                                                const double* __restrict__ colsum, const double* __restrict__ partial,
                                                double* __restrict__ mean, double* __restrict__ C) {
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= d * d) return;
  const int i = e / d, j = e - i * d;
  if (j < i) return;  // (written by the thread of (j, i))
  const int bi = i / kTileF, bj = j / kTileF;
  const int pair = bi * tiles - bi * (bi - 1) / 2 + (bj - bi);
  const double* p = partial + (int64_t)pair * kTileElems + (i % kTileF) * kTileF + (j % kTileF);
  const int64_t wide = (int64_t)tiles * kTileF;
  double sum = 0.0, ci = 0.0, cj = 0.0;
  for (int64_t s = 0; s < slices; ++s) {  // (slice order)
    sum += p[s * pairs * kTileElems];
    ci += colsum[s * wide + i];
    cj += colsum[s * wide + j];
  }
  const double nd = (double)n;
  const double si = vm_shift(mpart, chunks, d, i, n), sj = vm_shift(mpart, chunks, d, j, n);
  const double mi = ci / nd, mj = cj / nd;
  double c = sum - nd * mi * mj;
  if (!isfinite(si) || !isfinite(sj)) c = __builtin_nan("");
  C[(int64_t)i * d + j] = c;
  C[(int64_t)j * d + i] = c;
  if (i == j) mean[i] = si + mi;
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

VectorMomentsPlan vector_moments_plan(int64_t n, int d, int64_t slice_rows) {
  TFA_CHECK(n >= 1 && d >= 1 && d <= kVectorMomentsMaxD, "vector_moments: n >= 1 and 1 <= d <= ", kVectorMomentsMaxD,
            " expected, got n = ", n, ", d = ", d);
  VectorMomentsPlan p;
  p.tiles = (d + kTileF - 1) / kTileF;
  p.pairs = p.tiles * (p.tiles + 1) / 2;
  if (slice_rows <= 0) {
    const int64_t target = std::max<int64_t>(1, kTargetBlocks / p.pairs);
    slice_rows = std::max(kMinSliceRows, ceil_div(ceil_div(n, target), kStage) * kStage);
  }
  TFA_CHECK(slice_rows % kStage == 0, "vector_moments: slice_rows must be a multiple of ", kStage, ", got ", slice_rows);
  p.slice_rows = slice_rows;
  p.slices = ceil_div(n, slice_rows);
  p.lpr_log2 = 0;
  while (p.lpr_log2 < 6 && (1 << p.lpr_log2) < d) ++p.lpr_log2;
  const int col_tiles = (d + (1 << p.lpr_log2) - 1) >> p.lpr_log2;
  const int64_t max_chunks = std::min<int64_t>(512, std::max<int64_t>(128, 1024 / col_tiles));
  const int64_t chunks = std::min(max_chunks, std::max<int64_t>(1, n / kMinChunkRows));
  const int rpb = kT >> p.lpr_log2;
  p.mean_chunk_rows = ceil_div(ceil_div(n, chunks), rpb) * rpb;
  p.mean_chunks = static_cast<int>(ceil_div(n, p.mean_chunk_rows));
  const double words = (double)p.mean_chunks * d + (double)p.slices * p.tiles * kTileF +
                       (double)p.slices * p.pairs * kTileElems;
  TFA_CHECK(words * 8 <= (double)kMaxWorkspace && p.slices * p.pairs < (int64_t(1) << 31),
            "vector_moments: slice_rows = ", slice_rows, " cuts ", n, " rows into ", p.slices,
            " slices, more than the workspace of ", kMaxWorkspace >> 20, " MB holds; use larger slices");
  p.workspace_bytes = static_cast<size_t>(words) * 8;
  return p;
}

void vector_moments(const void* x, DType dtype, int64_t n, int d, const VectorMomentsPlan& p, double* mean, double* C,
                    void* workspace, size_t workspace_size, hipStream_t s) {
  TFA_CHECK(dtype == DType::F32 || dtype == DType::F64, "vector_moments: float32 or float64 cells expected");
  TFA_CHECK(n >= 1 && d >= 1 && d <= kVectorMomentsMaxD && workspace_size >= p.workspace_bytes,
            "vector_moments: bad arguments");
  double* mpart = static_cast<double*>(workspace);
  double* colsum = mpart + (int64_t)p.mean_chunks * d;
  double* partial = colsum + p.slices * p.tiles * kTileF;
  const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const dim3 mgrid((unsigned)((d + (1 << p.lpr_log2) - 1) >> p.lpr_log2), (unsigned)p.mean_chunks);
  const unsigned sgrid = (unsigned)(p.slices * p.pairs);
#define TFA_VM_SYRK(T_, VEC_)                                                                                      \
  do {                                                                                                             \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vm_syrk<T_, VEC_>),                                   \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSyrkLds);                          \
    hipLaunchKernelGGL((vm_syrk<T_, VEC_>), dim3(sgrid), dim3(kT), kSyrkLds, s, static_cast<const T_*>(x), n, d,   \
                       p.tiles, p.pairs, p.slice_rows, mpart, p.mean_chunks, colsum, partial);                     \
  } while (0)
  if (dtype == DType::F32) {
    hipLaunchKernelGGL(vm_means<float>, mgrid, dim3(kT), 0, s, static_cast<const float*>(x), n, d, p.lpr_log2,
                       p.mean_chunk_rows, mpart);
    TFA_LAUNCH_CHECK("vm_means");
    if (vec) TFA_VM_SYRK(float, true);
    else TFA_VM_SYRK(float, false);
  } else {
    hipLaunchKernelGGL(vm_means<double>, mgrid, dim3(kT), 0, s, static_cast<const double*>(x), n, d, p.lpr_log2,
                       p.mean_chunk_rows, mpart);
    TFA_LAUNCH_CHECK("vm_means");
    if (vec) TFA_VM_SYRK(double, true);
    else TFA_VM_SYRK(double, false);
  }
#undef TFA_VM_SYRK
  TFA_LAUNCH_CHECK("vm_syrk");
  hipLaunchKernelGGL(vm_finish, dim3((unsigned)((d * d + kT - 1) / kT)), dim3(kT), 0, s, n, d, p.tiles, p.pairs,
                     p.slices, mpart, p.mean_chunks, colsum, partial, mean, C);
  TFA_LAUNCH_CHECK("vm_finish");
}

}  // namespace k
}  // namespace tfa
