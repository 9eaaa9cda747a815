// One Lloyd step of k-means over a vector column (ml/clustering.py: KMeans).
//
// x is [n][d], row-major, f32 or f64; centers is [k][d], f64; 1 <= k <=
// kKMeansMaxK, 1 <= d <= kKMeansMaxD, k d <= kKMeansMaxKD. The [n][k] distance
// matrix is never written. Distances do not change under a translation, so
// both operands are shifted by `shift` [d] (the caller's mean of the centres):
// x' = x - shift is subtracted once while staging, c' = c - shift by the
// prologue, and ||c'||^2 - 2 x'.c' does not cancel when the data sit far from
// the origin. All arithmetic is f64 on v_mfma_f64_16x16x4_f64. Four launches,
// no float atomics, no block waits for another one:
//
//   0. km_centres  one block per centre: c' [k][d] and ||c'||^2 [k] (a thread
//                  adds the squares of its features in feature order, the 256
//                  threads are folded in thread order).
//   1. km_assign   a block owns a stripe of 64 rows: four waves, each a 32x32
//                  quadrant (rows x centres) as 2x2 MFMA tiles. It walks the
//                  centres in tiles of 64 and, per centre tile, the features
//                  in chunks of 32. A stage is the x' chunk [64 rows][32] and
//                  the c' chunk [64 centres][32], read in 16-byte loads (scalar
//                  loads when the base or d does not allow them), converted to
//                  f64, shifted once and written to an LDS image [row or
//                  centre][feature], two stages deep; rows past n, centres past
//                  k and features past d are 0.0. The next stage's global loads
//                  are issued before the current stage's MFMAs. Both operands
//                  are the same read pattern: lane l takes img[i0 + l % 16][f0
//                  + l / 16]. The row pitch is 34 doubles = 2 (mod 32), so the
//                  32 lanes that an 8-byte ds_read serves at a time (l % 16 =
//                  0..15, l / 16 = g, g + 1) fall on the 32 distinct 8-byte bank
//                  pairs 2 (l % 16) + l / 16 (mod 32): free of conflicts by this
//                  arithmetic, not by a counter measurement. After the last
//                  chunk of a centre tile the accumulators hold x'.c'; a lane
//                  forms ||c'||^2 - 2 x'.c' for its elements, the (value,
//                  index) minimum is taken over the wave's two column tiles,
//                  over the 16 lanes that share a row (xor shuffles), over the
//                  two waves that share the rows (LDS) and is kept per row
//                  across centre tiles. A tie goes to the smaller index at
//                  every level. ||x'||^2 of a row is added up by its staging
//                  threads during the first centre tile (a thread its quad of
//                  every chunk in feature order, then the eight quads in quad
//                  order). A row whose ||x'||^2 is not finite (a NaN or an
//                  infinity among its values) gets -1. Out: assign [n], dist
//                  [n] = max(||x'||^2 + best, 0) (0 for a -1 row) and per block
//                  the sum of its dist in row order and its count of -1 rows.
//   2. km_update   S[c][f] = sum of x'[r][f] over the rows with assign == c is
//                  a GEMM with a one-hot operand: S = onehot^T . X'. The grid is
//                  (64-centre tile) x (64-feature tile) x (slice of slice_rows
//                  rows). Per stage of 32 rows the x' segment goes to an LDS
//                  image [row][feature] with the pitch of 80 doubles = 640 bytes
//                  = 128 (mod 256): the B operand read (lane l takes img[r0 + l
//                  / 16][f0 + l % 16]) is that of vm_syrk (vector_moments.hip)
//                  and free of conflicts by the arithmetic written there. The A
//                  fragment is built in registers: lane l holds assign[r0 + l /
//                  16] == c0 + l % 16 ? 1.0 : 0.0; there is no LDS image of the
//                  one-hot matrix. A -1 row is staged as 0.0 (0.0 * NaN is not
//                  0.0). The products are exact, so a sum is the rows of the
//                  slice added in row order by the MFMA accumulator. MFMA tiles
//                  wholly past k or d are skipped. The blocks of the first
//                  feature tile also count their rows per centre (int32, LDS
//                  integer atomics). Out: partial [slice][k][d], cnt [slice][k].
//   3. km_finish   one thread per (c, f) folds the partials in slice order; one
//                  thread per c folds the counts (int64); one wave folds the
//                  block costs and -1 counts (a lane its blocks l, l + 64, ...
//                  in block order, then the lanes in lane order).
//
// The order of every addition depends on (n, d, k, slice_rows) alone: the same
// bits on every run. Every row index is compared with n (or the slice's end),
// every centre index with k and every feature index with d before an address
// is formed.
#include <algorithm>
#include <climits>
#include <cmath>

#include "hip_common.h"

namespace tfa {
namespace k {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kT = 256;                // threads per block
constexpr int kTile = 64;              // rows per stripe, centres per tile, features per km_update tile
constexpr int kChunk = 32;             // km_assign: features per stage
constexpr int kPitchA = kChunk + 2;    // km_assign: doubles per LDS row, 34 = 2 (mod 32)
constexpr int kStage = kKMeansStage;   // km_update: rows per stage
constexpr int kPitchU = kTile + 16;    // km_update: doubles per LDS row, 640 bytes = 128 (mod 256)
constexpr int kImgA = 2 * kTile * kPitchA;  // one stage of km_assign: 64 rows of x', 64 centres
// two stages, ||x'||^2 parts [64][8], best values [2][64], dist [64]; best indices [2][64], -1 flags [64]
constexpr size_t kAssignLds = (2 * kImgA + kTile * 8 + 2 * kTile + kTile) * sizeof(double) + 3 * kTile * sizeof(int);
constexpr int kTargetBlocks = 512;     // the 256 CUs about twice over
constexpr int64_t kMinSliceRows = 256;
constexpr size_t kMaxWorkspace = size_t(1) << 30;

template <typename T>
struct Quad {  // four consecutive elements of a row
  T v[4];
};

template <typename T, bool VEC>
__device__ __forceinline__ Quad<T> km_load4(const T* __restrict__ p, int f0, int d) {
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

// (value, index) minimum; a tie goes to the smaller index, a NaN never wins
__device__ __forceinline__ void km_take(double& bv, int& bi, double v, int i) {
  if (v < bv || (v == bv && i < bi)) bv = v, bi = i;
}

// ------------------------------------------------------------------ 0. shifted centres
__global__ __launch_bounds__(kT) void km_centres(const double* __restrict__ centers, const double* __restrict__ shift,
                                                 int d, double* __restrict__ cs, double* __restrict__ cn) {
  __shared__ double red[kT];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * d;  // (the grid is k blocks)
  double acc = 0.0;
  for (int f = tid; f < d; f += kT) {
    const double v = centers[base + f] - shift[f];
    cs[base + f] = v;
    acc += v * v;
  }
  red[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int j = 0; j < kT; ++j) t += red[j];  // (thread order)
    cn[blockIdx.x] = t;
  }
}

// ------------------------------------------------------------------ 1. assignment
template <typename T, bool VEC>
__global__ __launch_bounds__(kT) void km_assign(const T* __restrict__ x, int64_t n, int d, int k,
                                                const double* __restrict__ shift, const double* __restrict__ cs,
                                                const double* __restrict__ cn, int32_t* __restrict__ assign,
                                                double* __restrict__ dist, double* __restrict__ bcost,
                                                int32_t* __restrict__ bbad) {
  extern __shared__ __attribute__((aligned(16))) double lds[];  // see kAssignLds
  double* xn_part = lds + 2 * kImgA;
  double* bestv = xn_part + kTile * 8;
  double* drow = bestv + 2 * kTile;
  int* besti = reinterpret_cast<int*>(drow + kTile);
  int* badrow = besti + 2 * kTile;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t row0 = (int64_t)blockIdx.x * kTile;
  const int chunks = (d + kChunk - 1) / kChunk, ctiles = (k + kTile - 1) / kTile;
  const int total = chunks * ctiles;

  // staging: thread -> quad q of the 8 quads of a chunk, rows r and r + 32 of
  // the stripe and centres r and r + 32 of the centre tile
  const int q = tid & 7, r = tid >> 3;
  Quad<T> xr[2];
  Quad<double> cr[2];
  double sh[4], xn[2] = {0.0, 0.0};
  int ld_ct = 0, ld_f0 = 0;
  auto load = [&](int st) __attribute__((always_inline)) {
    ld_ct = st / chunks;
    ld_f0 = (st - ld_ct * chunks) * kChunk + q * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[e] = ld_f0 + e < d ? shift[ld_f0 + e] : 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t row = row0 + r + 32 * h;
      const int c = ld_ct * kTile + r + 32 * h;
      if (row < n) {
        xr[h] = km_load4<T, VEC>(x + row * d + ld_f0, ld_f0, d);
      } else {
        xr[h].v[0] = xr[h].v[1] = xr[h].v[2] = xr[h].v[3] = T(0);
      }
      if (c < k) {
        cr[h] = km_load4<double, VEC>(cs + (int64_t)c * d + ld_f0, ld_f0, d);
      } else {
        cr[h].v[0] = cr[h].v[1] = cr[h].v[2] = cr[h].v[3] = 0.0;
      }
    }
  };
  auto store = [&](int buf) __attribute__((always_inline)) {  // (what the last load() fetched)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool row_ok = row0 + r + 32 * h < n;
      double v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = (row_ok && ld_f0 + e < d) ? (double)xr[h].v[e] - sh[e] : 0.0;  // (padding is 0.0, not 0 - shift)
        if (ld_ct == 0) xn[h] += v[e] * v[e];
      }
      double* p = lds + buf * kImgA + (r + 32 * h) * kPitchA + q * 4;
      *reinterpret_cast<double2*>(p) = double2{v[0], v[1]};
      *reinterpret_cast<double2*>(p + 2) = double2{v[2], v[3]};
      double* pc = p + kTile * kPitchA;
      *reinterpret_cast<double2*>(pc) = double2{cr[h].v[0], cr[h].v[1]};
      *reinterpret_cast<double2*>(pc + 2) = double2{cr[h].v[2], cr[h].v[3]};
    }
  };

  bool eni[2];  // the wave's row tiles that are not wholly past n
#pragma unroll
  for (int i = 0; i < 2; ++i) eni[i] = row0 + wm * 32 + i * 16 < n;
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  double run_v = INFINITY;  // threads 0..63: the best of row tid so far
  int run_i = INT_MAX;

  const int a_off = (wm * 32 + (lane & 15)) * kPitchA + (lane >> 4);
  const int b_off = (kTile + wn * 32 + (lane & 15)) * kPitchA + (lane >> 4);
  load(0);
  store(0);
  __syncthreads();
  int ct = 0, ch = 0;
  for (int st = 0; st < total; ++st) {
    const int cur = st & 1;
    const bool more = st + 1 < total;
    if (more) load(st + 1);  // in flight under the MFMAs
    const int cw = ct * kTile + wn * 32;  // the wave's first centre
    const bool enj[2] = {cw < k, cw + 16 < k};
    const double* img = lds + cur * kImgA;
#pragma unroll
    for (int kk = 0; kk < kChunk / 4; ++kk) {
      double a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = img[a_off + i * 16 * kPitchA + kk * 4];
        b[i] = img[b_off + i * 16 * kPitchA + kk * 4];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (eni[i] && enj[j]) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (ch == chunks - 1) {  // the accumulators hold x'.c' of this centre tile
      // f64 C/D layout: col (centre) = lane & 15, row = (lane >> 4) + 4 * reg
      const int c0 = cw + (lane & 15), c1 = c0 + 16;
      const double n0 = c0 < k ? cn[c0] : 0.0, n1 = c1 < k ? cn[c1] : 0.0;
      static_for<2>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        const f64x4 v0 = acc[i][0], v1 = acc[i][1];
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          double bv = INFINITY;
          int bi = INT_MAX;
          if (c0 < k) km_take(bv, bi, n0 - 2.0 * v0[rg], c0);
          if (c1 < k) km_take(bv, bi, n1 - 2.0 * v1[rg], c1);
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) {  // the 16 lanes that share the row
            const double ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            km_take(bv, bi, ov, oi);
          }
          if ((lane & 15) == 0) {
            const int rl = wm * 32 + i * 16 + (lane >> 4) + 4 * rg;
            bestv[wn * kTile + rl] = bv;
            besti[wn * kTile + rl] = bi;
          }
        }
        acc[i][0] = f64x4{0.0, 0.0, 0.0, 0.0};
        acc[i][1] = f64x4{0.0, 0.0, 0.0, 0.0};
      });
      __syncthreads();
      if (tid < kTile) {
        km_take(run_v, run_i, bestv[tid], besti[tid]);
        km_take(run_v, run_i, bestv[kTile + tid], besti[kTile + tid]);
      }
      ch = 0;
      ++ct;
    } else {
      ++ch;
    }
    if (more) store(cur ^ 1);  // (every wave left that image before the previous barrier)
    __syncthreads();
  }

#pragma unroll
  for (int h = 0; h < 2; ++h) xn_part[(r + 32 * h) * 8 + q] = xn[h];
  __syncthreads();
  if (tid < kTile) {
    double xnv = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) xnv += xn_part[tid * 8 + j];  // (quad order)
    const int64_t row = row0 + tid;
    double dv = 0.0;
    int bad = 0;
    if (row < n) {
      const bool ok = isfinite(xnv) && run_i != INT_MAX;
      dv = ok ? fmax(xnv + run_v, 0.0) : 0.0;
      bad = ok ? 0 : 1;
      assign[row] = ok ? run_i : -1;
      dist[row] = dv;
    }
    drow[tid] = dv;
    badrow[tid] = bad;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    int b = 0;
    for (int j = 0; j < kTile; ++j) {  // (row order)
      t += drow[j];
      b += badrow[j];
    }
    bcost[blockIdx.x] = t;
    bbad[blockIdx.x] = b;
  }
}

// ------------------------------------------------------------------ 2. per-centre sums
template <typename T, bool VEC>
__global__ __launch_bounds__(kT) void km_update(const T* __restrict__ x, int64_t n, int d, int k,
                                                const double* __restrict__ shift, const int32_t* __restrict__ assign,
                                                int ftiles, int tiles, int64_t slice_rows,
                                                double* __restrict__ partial, int32_t* __restrict__ cnt) {
  __shared__ __attribute__((aligned(16))) double img[2 * kStage * kPitchU];
  __shared__ int asg[2 * kStage];
  __shared__ int cntl[kTile];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int tile = blockIdx.x % (unsigned)tiles;
  const int64_t sl = blockIdx.x / (unsigned)tiles;
  const int ct = tile / ftiles, ft = tile - ct * ftiles;
  const int c0 = ct * kTile, fb = ft * kTile;
  const int64_t r_begin = sl * slice_rows;
  const int64_t r_end = r_begin + slice_rows < n ? r_begin + slice_rows : n;
  if (tid < kTile) cntl[tid] = 0;
  __syncthreads();

  // staging: thread -> quad q of the 16 quads of a row segment, rows g and g + 16 of a stage
  const int q = tid & 15, g = tid >> 4;
  const int f0 = fb + q * 4;
  double sh[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) sh[e] = f0 + e < d ? shift[f0 + e] : 0.0;
  Quad<T> raw[2];
  int ar[2];
  auto load = [&](int64_t rs) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t row = rs + g + 16 * h;
      ar[h] = row < r_end ? assign[row] : -1;
      if (ar[h] >= 0) {  // (a -1 row is staged as 0.0)
        raw[h] = km_load4<T, VEC>(x + row * d + f0, f0, d);
      } else {
        raw[h].v[0] = raw[h].v[1] = raw[h].v[2] = raw[h].v[3] = T(0);
      }
    }
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (ar[h] >= 0 && f0 + e < d) ? (double)raw[h].v[e] - sh[e] : 0.0;
      double* p = img + (buf * kStage + g + 16 * h) * kPitchU + q * 4;
      *reinterpret_cast<double2*>(p) = double2{v[0], v[1]};
      *reinterpret_cast<double2*>(p + 2) = double2{v[2], v[3]};
      if (q == 0) {
        asg[buf * kStage + g + 16 * h] = ar[h];
        if (ft == 0 && ar[h] >= c0 && ar[h] < c0 + kTile) atomicAdd(&cntl[ar[h] - c0], 1);
      }
    }
  };

  bool en[2][2];  // the wave's MFMA tiles that are not wholly past k or d
  bool any = false;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      en[i][j] = c0 + wm * 32 + i * 16 < k && fb + wn * 32 + j * 16 < d;
      any = any || en[i][j];
    }
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int ca = c0 + wm * 32 + (lane & 15);  // the centre of the lane's A elements (tile i: + 16 i)
  const int b_off = (lane >> 4) * kPitchU + wn * 32 + (lane & 15);

  const int64_t stages = (r_end - r_begin + kStage - 1) / kStage;
  load(r_begin);
  store(0);
  __syncthreads();
  for (int64_t st = 0; st < stages; ++st) {
    const int cur = (int)(st & 1);
    const bool more = st + 1 < stages;
    if (more) load(r_begin + (st + 1) * kStage);  // in flight under the MFMAs
    if (any) {
      const double* im = img + cur * kStage * kPitchU + b_off;
      const int* as = asg + cur * kStage + (lane >> 4);
#pragma unroll
      for (int kk = 0; kk < kStage / 4; ++kk) {
        const int arow = as[kk * 4];
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = arow == ca + i * 16 ? 1.0 : 0.0;
          b[i] = im[kk * 4 * kPitchU + i * 16];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (en[i][j]) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    if (more) store(cur ^ 1);  // (every wave left that image before the previous barrier)
    __syncthreads();
  }

  // f64 C/D layout: col (feature) = lane & 15, row (centre) = (lane >> 4) + 4 * reg
  double* out = partial + sl * k * d;
  static_for<2>([&](auto ic) __attribute__((always_inline)) {
    constexpr int i = decltype(ic)::value;
    static_for<2>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      const f64x4 v = acc[i][j];
      const int f = fb + wn * 32 + j * 16 + (lane & 15);
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int c = c0 + wm * 32 + i * 16 + (lane >> 4) + 4 * rg;
        if (c < k && f < d) out[(int64_t)c * d + f] = v[rg];
      }
    });
  });
  if (ft == 0 && tid < kTile && c0 + tid < k) cnt[sl * k + c0 + tid] = cntl[tid];
}

// ------------------------------------------------------------------ 3. finish
__global__ __launch_bounds__(kT) void km_finish(int d, int k, int64_t slices, int64_t blocks,
                                                const double* __restrict__ partial, const int32_t* __restrict__ cnt,
                                                const double* __restrict__ bcost, const int32_t* __restrict__ bbad,
                                                double* __restrict__ sums, int64_t* __restrict__ counts,
                                                double* __restrict__ cost, int64_t* __restrict__ bad) {
  __shared__ double lc[kWave];
  __shared__ int64_t lb[kWave];
  const int tid = threadIdx.x;
  const int kd = k * d;
  if (blockIdx.x + 1 < gridDim.x) {  // the sums
    const int e = blockIdx.x * kT + tid;
    if (e >= kd) return;
    double t = 0.0;
    for (int64_t s = 0; s < slices; ++s) t += partial[s * kd + e];  // (slice order)
    sums[e] = t;
    return;
  }
  for (int c = tid; c < k; c += kT) {  // the last block: the counts, the cost, the -1 rows
    int64_t t = 0;
    for (int64_t s = 0; s < slices; ++s) t += cnt[s * k + c];
    counts[c] = t;
  }
  if (tid < kWave) {
    double t = 0.0;
    int64_t b = 0;
    for (int64_t j = tid; j < blocks; j += kWave) {  // (block order)
      t += bcost[j];
      b += bbad[j];
    }
    lc[tid] = t;
    lb[tid] = b;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    int64_t b = 0;
    for (int j = 0; j < kWave; ++j) {  // (lane order)
      t += lc[j];
      b += lb[j];
    }
    cost[0] = t;
    bad[0] = b;
  }
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the workspace, in doubles, every part a multiple of 16 bytes
struct Layout {
  double cs, cn, bcost, bbad, partial, cnt, words;
};
Layout layout(int64_t n, int d, int k, const KMeansPlan& p) {
  auto even = [](double w) { return 2.0 * std::ceil(w / 2.0); };
  Layout l;
  l.cs = 0;
  l.cn = l.cs + even((double)k * d);
  l.bcost = l.cn + even(k);
  l.bbad = l.bcost + even((double)p.blocks);
  l.partial = l.bbad + even((double)p.blocks / 2.0);
  l.cnt = l.partial + even((double)p.slices * k * d);
  l.words = l.cnt + even((double)p.slices * k / 2.0);
  return l;
}

void check_args(const char* what, DType dtype, int64_t n, int d, int k, const KMeansPlan& p, size_t workspace_size) {
  TFA_CHECK(dtype == DType::F32 || dtype == DType::F64, what, ": float32 or float64 cells expected");
  TFA_CHECK(n >= 1 && d >= 1 && d <= kKMeansMaxD && k >= 1 && k <= kKMeansMaxK && (int64_t)k * d <= kKMeansMaxKD &&
                p.blocks == ceil_div(n, kTile) && p.slices >= 1 && workspace_size >= p.workspace_bytes,
            what, ": bad arguments");
}

}  // namespace

KMeansPlan kmeans_plan(int64_t n, int d, int k, int64_t slice_rows) {
  TFA_CHECK(n >= 1 && d >= 1 && d <= kKMeansMaxD && k >= 1 && k <= kKMeansMaxK && (int64_t)k * d <= kKMeansMaxKD,
            "kmeans: n >= 1, 1 <= d <= ", kKMeansMaxD, ", 1 <= k <= ", kKMeansMaxK, " and k d <= ", kKMeansMaxKD,
            " expected, got n = ", n, ", d = ", d, ", k = ", k);
  KMeansPlan p;
  p.ctiles = (k + kTile - 1) / kTile;
  p.ftiles = (d + kTile - 1) / kTile;
  p.blocks = ceil_div(n, kTile);
  if (slice_rows <= 0) {
    const int64_t target = std::max<int64_t>(1, kTargetBlocks / (p.ctiles * p.ftiles));
    slice_rows = std::max(kMinSliceRows, ceil_div(ceil_div(n, target), kStage) * kStage);
  }
  TFA_CHECK(slice_rows % kStage == 0, "kmeans: slice_rows must be a multiple of ", kStage, ", got ", slice_rows);
  p.slice_rows = slice_rows;
  p.slices = ceil_div(n, slice_rows);
  const double words = layout(n, d, k, p).words;
  TFA_CHECK(words * 8 <= (double)kMaxWorkspace && p.slices * p.ctiles * p.ftiles < (int64_t(1) << 31) &&
                p.blocks < (int64_t(1) << 31),
            "kmeans: slice_rows = ", slice_rows, " cuts ", n, " rows into ", p.slices,
            " slices, more than the workspace of ", kMaxWorkspace >> 20, " MB holds; use larger slices");
  p.workspace_bytes = static_cast<size_t>(words) * 8;
  return p;
}

void kmeans_assign(const void* x, DType dtype, int64_t n, int d, int k, const double* centers, const double* shift,
                   const KMeansPlan& p, int32_t* assign, double* dist, void* workspace, size_t workspace_size,
                   hipStream_t s) {
  check_args("kmeans_assign", dtype, n, d, k, p, workspace_size);
  const Layout l = layout(n, d, k, p);
  double* ws = static_cast<double*>(workspace);
  double* cs = ws + (int64_t)l.cs;
  double* cn = ws + (int64_t)l.cn;
  double* bcost = ws + (int64_t)l.bcost;
  int32_t* bbad = reinterpret_cast<int32_t*>(ws + (int64_t)l.bbad);
  hipLaunchKernelGGL(km_centres, dim3((unsigned)k), dim3(kT), 0, s, centers, shift, d, cs, cn);
  TFA_LAUNCH_CHECK("km_centres");
  const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(cs) & 15) == 0;
#define TFA_KM_ASSIGN(T_, VEC_)                                                                                     \
  do {                                                                                                              \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&km_assign<T_, VEC_>),                                  \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAssignLds);                         \
    hipLaunchKernelGGL((km_assign<T_, VEC_>), dim3((unsigned)p.blocks), dim3(kT), kAssignLds, s,                    \
                       static_cast<const T_*>(x), n, d, k, shift, cs, cn, assign, dist, bcost, bbad);               \
  } while (0)
  if (dtype == DType::F32) {
    if (vec) TFA_KM_ASSIGN(float, true);
    else TFA_KM_ASSIGN(float, false);
  } else {
    if (vec) TFA_KM_ASSIGN(double, true);
    else TFA_KM_ASSIGN(double, false);
  }
#undef TFA_KM_ASSIGN
  TFA_LAUNCH_CHECK("km_assign");
}

void kmeans_step(const void* x, DType dtype, int64_t n, int d, int k, const double* centers, const double* shift,
                 const KMeansPlan& p, int32_t* assign, double* dist, int64_t* counts, double* sums, double* cost,
                 int64_t* bad, void* workspace, size_t workspace_size, hipStream_t s) {
  kmeans_assign(x, dtype, n, d, k, centers, shift, p, assign, dist, workspace, workspace_size, s);
  const Layout l = layout(n, d, k, p);
  double* ws = static_cast<double*>(workspace);
  double* partial = ws + (int64_t)l.partial;
  int32_t* cnt = reinterpret_cast<int32_t*>(ws + (int64_t)l.cnt);
  const int tiles = p.ctiles * p.ftiles;
  const unsigned ugrid = (unsigned)(p.slices * tiles);
  const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
#define TFA_KM_UPDATE(T_, VEC_)                                                                                  \
  hipLaunchKernelGGL((km_update<T_, VEC_>), dim3(ugrid), dim3(kT), 0, s, static_cast<const T_*>(x), n, d, k, shift, \
                     assign, p.ftiles, tiles, p.slice_rows, partial, cnt)
  if (dtype == DType::F32) {
    if (vec) TFA_KM_UPDATE(float, true);
    else TFA_KM_UPDATE(float, false);
  } else {
    if (vec) TFA_KM_UPDATE(double, true);
    else TFA_KM_UPDATE(double, false);
  }
#undef TFA_KM_UPDATE
  TFA_LAUNCH_CHECK("km_update");
  hipLaunchKernelGGL(km_finish, dim3((unsigned)((k * d + kT - 1) / kT + 1)), dim3(kT), 0, s, d, k, p.slices, p.blocks,
                     partial, cnt, ws + (int64_t)l.bcost, reinterpret_cast<const int32_t*>(ws + (int64_t)l.bbad), sums,
                     counts, cost, bad);
  TFA_LAUNCH_CHECK("km_finish");
}

}  // namespace k
}  // namespace tfa
