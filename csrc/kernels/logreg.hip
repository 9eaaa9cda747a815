// One objective evaluation of logistic regression over a vector column
// (ml/classification.py: LogisticRegression), and the model's prediction.
//
// x is [n][d], row-major, f32 or f64; coef is [R][d] and icpt [R], f64; R = 1 is
// the binomial model (K = 2 classes, one margin), R = K >= 2 the multinomial
// one. 1 <= d <= kLogRegMaxD, K <= kLogRegMaxK, R d <= kLogRegMaxRD. All
// arithmetic is f64 on v_mfma_f64_16x16x4_f64. Three launches, no float atomics,
// no block waits for another one:
//
//   1. lr_forward   a block owns a stripe of 64 rows: four waves, each 16 rows
//                   against every class, ct = ceil(R / 16) MFMA tiles whose
//                   accumulators (at R = 128: 32 doubles a lane) hold the
//                   stripe's margins for the whole walk over d and never go to
//                   HBM. It walks the features in chunks of 32. A stage is the
//                   x chunk [64 rows][32] and the coefficient chunk [16 ct
//                   classes][32], read in 16-byte loads (scalar loads when a
//                   base or d does not allow them), converted to f64 and
//                   written to an LDS image [row or class][feature], two
//                   stages deep; rows past n, classes past R and features past
//                   d are 0.0. The next stage's global loads are issued before
//                   the current stage's MFMAs. Both operands are the same read
//                   pattern: lane l takes img[i0 + l % 16][f0 + l / 16]. The
//                   row pitch is 34 doubles = 2 (mod 32), so the 32 lanes that
//                   an 8-byte ds_read serves at a time (l % 16 = 0..15, l / 16
//                   = g, g + 1) fall on the 32 distinct 8-byte bank pairs 2 (l
//                   % 16) + l / 16 (mod 32): free of conflicts by this
//                   arithmetic, not by a counter measurement (the pitch of
//                   km_assign, kmeans.hip). A staging thread notes a NaN or an
//                   infinity among the values it converts. After the last
//                   chunk the staging LDS is dead: the margins m = acc + icpt
//                   are laid out in it once, [64][16 ct + 1], and four lanes
//                   per row (lane s the classes s, s + 4, ...) do the row
//                   epilogue:
//                     multinomial  M = max m, S = sum exp(m - M) (a lane its
//                                  classes in class order, then the xor
//                                  butterfly 1, 2: a + b is commutative, so
//                                  the four lanes hold the same bits), p_c =
//                                  exp(m_c - M) / S, loss w ((M + log S) - m_y),
//                                  q_c = w (p_c - [c == y]);
//                     binomial     e = exp(-|m|), sigma = m >= 0 ? 1 / (1 + e)
//                                  : e / (1 + e), loss w ((max(m, 0) + log1p(e))
//                                  - y m), q = w (sigma - y): no threshold and
//                                  no overflow for any m.
//                   A row is left out (q = 0, no loss, no weight) and counted
//                   once, in the first of: x holds a NaN or an infinity; y is
//                   not an integer in [0, K); w is negative, NaN or infinite. A
//                   row of weight 0 is legal and contributes exact zeros. q
//                   goes back into the image and leaves as one contiguous
//                   [rows][R] store. Out: q [n][R] and per block its loss and
//                   weight sum (64 rows in row order) and the three counts.
//                   In prediction mode the epilogue writes raw [n][K] (the
//                   margins; binomial: [-m, m]), prob [n][K] and pred [n] (the
//                   first largest probability; binomial: m > logit(threshold))
//                   instead; a row of x with a NaN or an infinity gets -1 and
//                   zeros.
//   2. lr_gradient  G [R][d + 1] = q^T [x, 1] is a dense GEMM over (class tile)
//                   x (feature tile) x (slice of slice_rows rows); feature d is
//                   the constant 1.0 of the rows of the slice, so the
//                   intercept column is the column sum of q. R <= 32: the four
//                   waves sit side by side, a block is 32 classes x 128
//                   features; otherwise 2 x 2, 64 x 64. Per stage of 32 rows
//                   the x segment goes to an LDS image [row][feature] with the
//                   pitch of 80 or 144 doubles = 128 bytes (mod 256): the B
//                   operand read (lane l takes img[r0 + l / 16][f0 + l % 16]) is
//                   that of vm_syrk (vector_moments.hip) and free of conflicts
//                   by the arithmetic written there. A value that is not
//                   finite is staged as 0.0: its row has q = 0, and 0.0 * NaN
//                   is not 0.0. The A fragment (lane l: q[r0 + l / 16][c0 + l %
//                   16], 16 lanes 128 contiguous bytes) is read from the
//                   workspace into registers one stage ahead; there is no LDS
//                   image of q. The f64 MFMA adds its four products in row
//                   order, so a sum is the rows of the slice in row order. MFMA
//                   tiles wholly past R or d + 1 are skipped. Out: partial
//                   [slice][R][d + 1].
//   3. lr_finish    one thread per (c, f) folds the partials in slice order; one
//                   wave folds the block records (a lane its blocks l, l + 64,
//                   ... in block order, then the lanes in lane order).
//
// The order of every addition depends on (n, d, R, slice_rows) alone: the same
// bits on every run. Every row index is compared with n (or the slice's end),
// every class index with R and every feature index with d before an address is
// formed.
#include <algorithm>
#include <cmath>

#include "column_types.h"
#include "hip_common.h"

namespace tfa {
namespace k {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kT = 256;              // threads per block
constexpr int kRows = 64;            // rows per stripe of lr_forward
constexpr int kChunk = 32;           // lr_forward: features per stage
constexpr int kPitchF = kChunk + 2;  // lr_forward: doubles per LDS row, 34 = 2 (mod 32)
constexpr int kStage = kLogRegStage; // lr_gradient: rows per stage
constexpr int kTargetBlocks = 512;   // the 256 CUs about twice over
constexpr int64_t kMinSliceRows = 256;
constexpr size_t kMaxWorkspace = size_t(1) << 31;

// lr_forward's LDS for ct class tiles: two stages of (64 rows + 16 ct classes) x
// pitch 34, the rows' loss and weight [2][64]; the rows' count code and x flag
constexpr int fwd_img(int ct) { return (kRows + 16 * ct) * kPitchF; }
constexpr size_t fwd_lds(int ct) { return (2 * fwd_img(ct) + 2 * kRows) * sizeof(double) + 2 * kRows * sizeof(int); }
// lr_gradient's LDS: two stages of 32 rows x (features of the tile + 16)
constexpr size_t grad_lds(int ft) { return 2 * kStage * (ft + 16) * sizeof(double); }

template <typename T>
struct Quad {  // four consecutive elements of a row
  T v[4];
};

template <typename T, bool VEC>
__device__ __forceinline__ Quad<T> lr_load4(const T* __restrict__ p, int f0, int d) {
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

__device__ __forceinline__ double lr_column(const void* p, DType dt, int64_t row) {
  return dispatch_column(dt, [&](auto tag) { return static_cast<double>(static_cast<const decltype(tag)*>(p)[row]); });
}

struct FwdArgs {
  const void* x;
  const void* y;  // null in prediction mode
  const void* w;  // may be null
  DType ydtype, wdtype;
  int64_t n;
  int d, R, K, ct;
  const double* coef;
  const double* icpt;
  int predict;
  double logit_t;
  double* q;       // step: [n][R]
  double* bpart;   // step: [blocks][2] loss, weight sum
  int32_t* bcnt;   // step: [blocks][4] bad x, bad y, bad w, unused
  int32_t* pred;   // predict: [n]
  double* raw;     // predict: [n][K]
  double* prob;    // predict: [n][K]
};

// ------------------------------------------------------------------ 1. margins and the row epilogue
template <typename T, bool VEC, int CTMAX>
__global__ __launch_bounds__(kT) void lr_forward(const FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];  // see fwd_lds
  const int ct = a.ct, d = a.d, R = a.R;
  const int64_t n = a.n;
  const int img = (kRows + 16 * ct) * kPitchF;
  double* rowloss = lds + 2 * img;
  double* roww = rowloss + kRows;
  int* rowbad = reinterpret_cast<int*>(roww + kRows);
  int* xbad = rowbad + kRows;
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const double* __restrict__ coef = a.coef;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int chunks = (d + kChunk - 1) / kChunk;
  if (tid < kRows) xbad[tid] = 0;

  // staging: thread -> quad q of the 8 quads of a chunk, rows r and r + 32 of
  // the stripe and classes r, r + 32, ... of the 16 ct staged
  constexpr int CH = (CTMAX * 16 + 31) / 32;
  const int q = tid & 7, r = tid >> 3;
  Quad<T> xr[2];
  Quad<double> cr[CH];
  int ld_f0 = 0, xb[2] = {0, 0};
  auto load = [&](int st) __attribute__((always_inline)) {
    ld_f0 = st * kChunk + q * 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t row = row0 + r + 32 * h;
      if (row < n) {
        xr[h] = lr_load4<T, VEC>(x + row * d + ld_f0, ld_f0, d);
      } else {
        xr[h].v[0] = xr[h].v[1] = xr[h].v[2] = xr[h].v[3] = T(0);
      }
    }
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      const int c = r + 32 * h;
      if (c < R) {
        cr[h] = lr_load4<double, VEC>(coef + (int64_t)c * d + ld_f0, ld_f0, d);
      } else {
        cr[h].v[0] = cr[h].v[1] = cr[h].v[2] = cr[h].v[3] = 0.0;
      }
    }
  };
  auto store = [&](int buf) __attribute__((always_inline)) {  // (what the last load() fetched)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = (double)xr[h].v[e];  // (load() left 0 past n and past d)
        xb[h] |= !isfinite(v[e]);
      }
      double* p = lds + buf * img + (r + 32 * h) * kPitchF + q * 4;
      *reinterpret_cast<double2*>(p) = double2{v[0], v[1]};
      *reinterpret_cast<double2*>(p + 2) = double2{v[2], v[3]};
    }
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      const int c = r + 32 * h;
      if (c < 16 * ct) {
        double* pc = lds + buf * img + (kRows + c) * kPitchF + q * 4;
        *reinterpret_cast<double2*>(pc) = double2{cr[h].v[0], cr[h].v[1]};
        *reinterpret_cast<double2*>(pc + 2) = double2{cr[h].v[2], cr[h].v[3]};
      }
    }
  };

  const bool en = row0 + wave * 16 < n;  // the wave's row tile is not wholly past n
  f64x4 acc[CTMAX];
#pragma unroll
  for (int j = 0; j < CTMAX; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int a_off = (wave * 16 + (lane & 15)) * kPitchF + (lane >> 4);
  const int b_off = (kRows + (lane & 15)) * kPitchF + (lane >> 4);
  load(0);
  store(0);
  __syncthreads();
  for (int st = 0; st < chunks; ++st) {
    const int cur = st & 1;
    const bool more = st + 1 < chunks;
    if (more) load(st + 1);  // in flight under the MFMAs
    const double* im = lds + cur * img;
    if (en) {
#pragma unroll
      for (int kk = 0; kk < kChunk / 4; ++kk) {
        const double av = im[a_off + kk * 4];
        static_for<CTMAX>([&](auto jc) __attribute__((always_inline)) {
          constexpr int j = decltype(jc)::value;
          if (j < ct) {
            const double bv = im[b_off + j * 16 * kPitchF + kk * 4];
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[j], 0, 0, 0);
          }
        });
      }
    }
    if (more) store(cur ^ 1);  // (every wave left that image before the previous barrier)
    __syncthreads();
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (xb[h]) atomicOr(&xbad[r + 32 * h], 1);

  // the margins, once: f64 C/D layout: col (class) = lane & 15, row = (lane >> 4) + 4 * reg
  const int MP = 16 * ct + 1;
  double* mg = lds;
  static_for<CTMAX>([&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    if (j < ct) {
      const int c = j * 16 + (lane & 15);
      const double ic = c < R ? a.icpt[c] : 0.0;
      const f64x4 v = acc[j];
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) mg[(wave * 16 + (lane >> 4) + 4 * rg) * MP + c] = v[rg] + ic;
    }
  });
  __syncthreads();

  // one contiguous [rows][cols] store of the image's first cols columns
  auto flush = [&](double* __restrict__ dst, int cols) __attribute__((always_inline)) {
    for (int e = tid; e < kRows * cols; e += kT) {
      const int rr = e / cols, c = e - rr * cols;
      if (row0 + rr < n) dst[row0 * cols + e] = mg[rr * MP + c];
    }
  };

  // the row epilogue: lanes sub = 0..3 of row rl
  const int rl = tid >> 2, sub = tid & 3;
  const int64_t row = row0 + rl;
  const bool live = row < n;
  const bool predict = a.predict != 0;
  double yv = 0.0, wv = 1.0;
  int code = 0;  // 1: x, 2: y, 3: w
  if (live) {
    if (!predict) {
      yv = lr_column(a.y, a.ydtype, row);
      if (a.w != nullptr) wv = lr_column(a.w, a.wdtype, row);
    }
    if (xbad[rl]) code = 1;
    else if (!predict && !(yv >= 0.0 && yv < (double)a.K && yv == floor(yv))) code = 2;
    else if (!(wv >= 0.0) || wv == __builtin_inf()) code = 3;
  }
  const bool use = live && code == 0;
  const bool counted = use && wv != 0.0;  // (a row of weight 0 contributes exact zeros)
  double loss = 0.0;
  if (R == 1) {  // binomial
    double* mr = mg + rl * MP;
    const double m = mr[0];
    const double e = exp(-fabs(m));
    const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
    const double s1 = m >= 0.0 ? big : small;  // sigma(m)
    if (!predict) {
      loss = counted ? wv * ((fmax(m, 0.0) + log1p(e)) - yv * m) : 0.0;
      if (sub == 0) mr[0] = counted ? wv * (s1 - yv) : 0.0;
      __syncthreads();
      flush(a.q, 1);
    } else {
      if (sub == 0) {  // (m is in a register; the four lanes of a row are in one wave)
        mr[0] = use ? -m : 0.0;
        mr[1] = use ? m : 0.0;
      }
      __syncthreads();
      flush(a.raw, 2);
      __syncthreads();
      if (sub == 0) {
        mr[0] = use ? (m >= 0.0 ? small : big) : 0.0;
        mr[1] = use ? s1 : 0.0;
        if (live) a.pred[row] = use ? (m > a.logit_t ? 1 : 0) : -1;
      }
      __syncthreads();
      flush(a.prob, 2);
    }
  } else {
    double* mr = mg + rl * MP;
    const int yi = (use && !predict) ? (int)yv : 0;
    double M = -__builtin_inf();
    for (int c = sub; c < R; c += 4) M = fmax(M, mr[c]);
    M = fmax(M, __shfl_xor(M, 1, 64));
    M = fmax(M, __shfl_xor(M, 2, 64));
    double S = 0.0, my = 0.0;
    for (int c = sub; c < R; c += 4) {
      const double mc = mr[c];
      if (c == yi) my = mc;
      const double e = exp(mc - M);
      if (!predict) mr[c] = e;
      S += e;
    }
    S += __shfl_xor(S, 1, 64);
    S += __shfl_xor(S, 2, 64);
    my = __shfl(my, (lane & ~3) | (yi & 3), 64);
    if (!predict) {
      loss = counted ? wv * ((M + log(S)) - my) : 0.0;
      for (int c = sub; c < R; c += 4) mr[c] = counted ? wv * (mr[c] / S - (c == yi ? 1.0 : 0.0)) : 0.0;
      __syncthreads();
      flush(a.q, R);
    } else {
      if (!use)
        for (int c = sub; c < R; c += 4) mr[c] = 0.0;
      __syncthreads();
      flush(a.raw, R);
      __syncthreads();
      double bv = -1.0;
      int bi = R;
      for (int c = sub; c < R; c += 4) {
        const double p = use ? exp(mr[c] - M) / S : 0.0;
        mr[c] = p;
        if (p > bv) bv = p, bi = c;  // (class order: the first of equal ones)
      }
#pragma unroll
      for (int off = 1; off < 4; off <<= 1) {
        const double ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
      }
      if (sub == 0 && live) a.pred[row] = use ? bi : -1;
      __syncthreads();
      flush(a.prob, R);
    }
  }
  if (predict) return;
  if (sub == 0) {
    rowloss[rl] = loss;
    roww[rl] = counted ? wv : 0.0;
    rowbad[rl] = code;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0, ws = 0.0;
    int b[4] = {0, 0, 0, 0};
    for (int j = 0; j < kRows; ++j) {  // (row order)
      t += rowloss[j];
      ws += roww[j];
      b[rowbad[j]] += 1;
    }
    a.bpart[2 * (int64_t)blockIdx.x] = t;
    a.bpart[2 * (int64_t)blockIdx.x + 1] = ws;
#pragma unroll
    for (int j = 0; j < 4; ++j) a.bcnt[4 * (int64_t)blockIdx.x + j] = j == 0 ? 0 : b[j];
  }
}

// ------------------------------------------------------------------ 2. q^T [x, 1]
template <typename T, bool VEC, int WM>
__global__ __launch_bounds__(kT) void lr_gradient(const T* __restrict__ x, int64_t n, int d, int R,
                                                  const double* __restrict__ qm, int ftiles, int tiles,
                                                  int64_t slice_rows, double* __restrict__ partial) {
  constexpr int WN = 4 / WM, CTL = 32 * WM, FT = 32 * WN, PX = FT + 16;
  constexpr int QPR = FT / 4, RPP = kT / QPR, H = kStage / RPP;  // quads per row, rows per pass, passes
  extern __shared__ __attribute__((aligned(16))) double ximg[];  // see grad_lds
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wm = wave / WN, wn = wave % WN;
  const int tile = blockIdx.x % (unsigned)tiles;
  const int64_t sl = blockIdx.x / (unsigned)tiles;
  const int ct = tile / ftiles, ft = tile - ct * ftiles;
  const int c0 = ct * CTL, fb = ft * FT;
  const int d1 = d + 1;
  const int64_t r_begin = sl * slice_rows;
  const int64_t r_end = r_begin + slice_rows < n ? r_begin + slice_rows : n;

  bool en[2][2];  // the wave's MFMA tiles that are not wholly past R or d + 1
  bool any = false;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      en[i][j] = c0 + wm * 32 + i * 16 < R && fb + wn * 32 + j * 16 < d1;
      any = any || en[i][j];
    }

  // staging: thread -> quad q of the row segment, rows g, g + RPP, ... of a stage
  const int q = tid % QPR, g = tid / QPR;
  const int f0 = fb + q * 4;
  Quad<T> raw[H];
  bool rin[H];
  const int ca = c0 + wm * 32 + (lane & 15);  // the class of the lane's A elements (tile i: + 16 i)
  double an[kStage / 4][2], ac[kStage / 4][2];
  auto load = [&](int64_t rs) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int64_t row = rs + g + RPP * h;
      rin[h] = row < r_end;
      if (rin[h]) {
        raw[h] = lr_load4<T, VEC>(x + row * d + f0, f0, d);
      } else {
        raw[h].v[0] = raw[h].v[1] = raw[h].v[2] = raw[h].v[3] = T(0);
      }
    }
#pragma unroll
    for (int kk = 0; kk < kStage / 4; ++kk) {
      const int64_t row = rs + kk * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = ca + i * 16;
        an[kk][i] = (any && row < r_end && c < R) ? qm[row * R + c] : 0.0;
      }
    }
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      double v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double t = (double)raw[h].v[e];  // (0 past d and past the slice)
        v[e] = isfinite(t) ? t : 0.0;
        if (f0 + e == d && rin[h]) v[e] = 1.0;  // the intercept's column
      }
      double* p = ximg + (buf * kStage + g + RPP * h) * PX + q * 4;
      *reinterpret_cast<double2*>(p) = double2{v[0], v[1]};
      *reinterpret_cast<double2*>(p + 2) = double2{v[2], v[3]};
    }
  };

  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int b_off = (lane >> 4) * PX + wn * 32 + (lane & 15);

  const int64_t stages = (r_end - r_begin + kStage - 1) / kStage;
  load(r_begin);
  store(0);
  __syncthreads();
  for (int64_t st = 0; st < stages; ++st) {
    const int cur = (int)(st & 1);
    const bool more = st + 1 < stages;
#pragma unroll
    for (int kk = 0; kk < kStage / 4; ++kk) ac[kk][0] = an[kk][0], ac[kk][1] = an[kk][1];
    if (more) load(r_begin + (st + 1) * kStage);  // in flight under the MFMAs
    if (any) {
      const double* im = ximg + cur * kStage * PX + b_off;
#pragma unroll
      for (int kk = 0; kk < kStage / 4; ++kk) {
        double b[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = im[kk * 4 * PX + j * 16];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (en[i][j]) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[kk][i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    if (more) store(cur ^ 1);  // (every wave left that image before the previous barrier)
    __syncthreads();
  }

  // f64 C/D layout: col (feature) = lane & 15, row (class) = (lane >> 4) + 4 * reg
  double* out = partial + sl * R * d1;
  static_for<2>([&](auto ic) __attribute__((always_inline)) {
    constexpr int i = decltype(ic)::value;
    static_for<2>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      const f64x4 v = acc[i][j];
      const int f = fb + wn * 32 + j * 16 + (lane & 15);
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int c = c0 + wm * 32 + i * 16 + (lane >> 4) + 4 * rg;
        if (c < R && f < d1) out[(int64_t)c * d1 + f] = v[rg];
      }
    });
  });
}

// ------------------------------------------------------------------ 3. finish
__global__ __launch_bounds__(kT) void lr_finish(int cells, int64_t slices, int64_t blocks,
                                                const double* __restrict__ partial, const double* __restrict__ bpart,
                                                const int32_t* __restrict__ bcnt, double* __restrict__ grad,
                                                double* __restrict__ loss, double* __restrict__ wsum,
                                                int64_t* __restrict__ bad) {
  __shared__ double ll[kWave], lw[kWave];
  __shared__ int64_t lb[3][kWave];
  const int tid = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {  // the gradient
    const int e = blockIdx.x * kT + tid;
    if (e >= cells) return;
    double t = 0.0;
    for (int64_t s = 0; s < slices; ++s) t += partial[s * cells + e];  // (slice order)
    grad[e] = t;
    return;
  }
  if (tid < kWave) {  // the last block: the block records
    double t = 0.0, ws = 0.0;
    int64_t b[3] = {0, 0, 0};
    for (int64_t j = tid; j < blocks; j += kWave) {  // (block order)
      t += bpart[2 * j];
      ws += bpart[2 * j + 1];
#pragma unroll
      for (int c = 0; c < 3; ++c) b[c] += bcnt[4 * j + 1 + c];
    }
    ll[tid] = t;
    lw[tid] = ws;
#pragma unroll
    for (int c = 0; c < 3; ++c) lb[c][tid] = b[c];
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0, ws = 0.0;
    int64_t b[3] = {0, 0, 0};
    for (int j = 0; j < kWave; ++j) {  // (lane order)
      t += ll[j];
      ws += lw[j];
#pragma unroll
      for (int c = 0; c < 3; ++c) b[c] += lb[c][j];
    }
    loss[0] = t;
    wsum[0] = ws;
#pragma unroll
    for (int c = 0; c < 3; ++c) bad[c] = b[c];
  }
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

template <typename T, bool VEC, int CTMAX>
void launch_forward_ct(const FwdArgs& a, unsigned blocks, hipStream_t s) {
  const size_t lds = fwd_lds(a.ct);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&lr_forward<T, VEC, CTMAX>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)fwd_lds(CTMAX));
  hipLaunchKernelGGL((lr_forward<T, VEC, CTMAX>), dim3(blocks), dim3(kT), lds, s, a);
}

template <typename T, bool VEC>
void launch_forward_tv(const FwdArgs& a, unsigned blocks, hipStream_t s) {
  if (a.ct <= 1) launch_forward_ct<T, VEC, 1>(a, blocks, s);
  else if (a.ct <= 2) launch_forward_ct<T, VEC, 2>(a, blocks, s);
  else if (a.ct <= 4) launch_forward_ct<T, VEC, 4>(a, blocks, s);
  else launch_forward_ct<T, VEC, 8>(a, blocks, s);
}

void launch_forward(DType dtype, const FwdArgs& a, hipStream_t s) {
  const unsigned blocks = (unsigned)ceil_div(a.n, kRows);
  const bool vec = a.d % 4 == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.coef) & 15) == 0;
  if (dtype == DType::F32) {
    if (vec) launch_forward_tv<float, true>(a, blocks, s);
    else launch_forward_tv<float, false>(a, blocks, s);
  } else {
    if (vec) launch_forward_tv<double, true>(a, blocks, s);
    else launch_forward_tv<double, false>(a, blocks, s);
  }
  TFA_LAUNCH_CHECK("lr_forward");
}

template <typename T, bool VEC, int WM>
void launch_gradient_wm(const void* x, int64_t n, int d, int R, const double* q, const LogRegPlan& p, double* partial,
                        hipStream_t s) {
  constexpr int FT = 32 * (4 / WM);
  const int tiles = p.ctiles * p.ftiles;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&lr_gradient<T, VEC, WM>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)grad_lds(FT));
  hipLaunchKernelGGL((lr_gradient<T, VEC, WM>), dim3((unsigned)(p.slices * tiles)), dim3(kT), grad_lds(FT), s,
                     static_cast<const T*>(x), n, d, R, q, p.ftiles, tiles, p.slice_rows, partial);
}

template <typename T, bool VEC>
void launch_gradient_tv(const void* x, int64_t n, int d, int R, const double* q, const LogRegPlan& p, double* partial,
                        hipStream_t s) {
  if (p.wm == 1) launch_gradient_wm<T, VEC, 1>(x, n, d, R, q, p, partial, s);
  else launch_gradient_wm<T, VEC, 2>(x, n, d, R, q, p, partial, s);
}

void check_shape(const char* what, DType dtype, int64_t n, int d, int R) {
  TFA_CHECK(dtype == DType::F32 || dtype == DType::F64, what, ": float32 or float64 cells expected");
  TFA_CHECK(n >= 1 && d >= 1 && d <= kLogRegMaxD && R >= 1 && R <= kLogRegMaxK && (int64_t)R * d <= kLogRegMaxRD,
            what, ": n >= 1, 1 <= d <= ", kLogRegMaxD, ", K <= ", kLogRegMaxK, " and R d <= ", kLogRegMaxRD,
            " expected, got n = ", n, ", d = ", d, ", R = ", R);
  TFA_CHECK(ceil_div(n, kRows) < (int64_t(1) << 31), what, ": too many rows for one call");
}

// the workspace, in doubles: q [n][R], the block records, the slice partials
struct Layout {
  double q, bpart, bcnt, partial, words;
};
Layout layout(int64_t n, int d, int R, const LogRegPlan& p) {
  Layout l;
  l.q = 0;
  l.bpart = l.q + (double)n * R;
  l.bcnt = l.bpart + 2.0 * (double)p.blocks;
  l.partial = l.bcnt + 2.0 * (double)p.blocks;  // (four int32 a block)
  l.words = l.partial + (double)p.slices * R * (d + 1);
  return l;
}

}  // namespace

LogRegPlan logreg_plan(int64_t n, int d, int R, int64_t slice_rows) {
  check_shape("logreg", DType::F64, n, d, R);
  LogRegPlan p;
  p.wm = R <= 32 ? 1 : 2;
  p.ctiles = (R + 32 * p.wm - 1) / (32 * p.wm);
  const int ft = 32 * (4 / p.wm);
  p.ftiles = (d + 1 + ft - 1) / ft;
  p.blocks = ceil_div(n, kRows);
  if (slice_rows <= 0) {
    const int64_t target = std::max<int64_t>(1, kTargetBlocks / (p.ctiles * p.ftiles));
    slice_rows = std::max(kMinSliceRows, ceil_div(ceil_div(n, target), kStage) * kStage);
  }
  TFA_CHECK(slice_rows % kStage == 0, "logreg: slice_rows must be a multiple of ", kStage, ", got ", slice_rows);
  p.slice_rows = slice_rows;
  p.slices = ceil_div(n, slice_rows);
  const double words = layout(n, d, R, p).words;
  TFA_CHECK(words * 8 <= (double)kMaxWorkspace && p.slices * p.ctiles * p.ftiles < (int64_t(1) << 31),
            "logreg: ", n, " rows x ", R, " multipliers and ", p.slices, " slices need more than the workspace of ",
            kMaxWorkspace >> 20, " MB; use smaller partitions or larger slices");
  p.workspace_bytes = static_cast<size_t>(words) * 8;
  return p;
}

void logreg_step(const void* x, DType dtype, const void* y, DType ydtype, const void* w, DType wdtype, int64_t n,
                 int d, int R, const double* coef, const double* icpt, const LogRegPlan& p, double* loss,
                 double* grad, double* wsum, int64_t* bad, void* workspace, size_t workspace_size, hipStream_t s) {
  check_shape("logreg_step", dtype, n, d, R);
  TFA_CHECK(y != nullptr && is_stat_dtype(ydtype), "logreg_step: the labels have a dtype that is not supported");
  TFA_CHECK(w == nullptr || is_stat_dtype(wdtype), "logreg_step: the weights have a dtype that is not supported");
  TFA_CHECK(p.blocks == ceil_div(n, kRows) && p.slices == ceil_div(n, p.slice_rows) && p.slice_rows % kStage == 0 &&
                (p.wm == 1 || p.wm == 2) && workspace_size >= p.workspace_bytes,
            "logreg_step: bad arguments");
  const Layout l = layout(n, d, R, p);
  double* ws = static_cast<double*>(workspace);
  double* q = ws + (int64_t)l.q;
  double* bpart = ws + (int64_t)l.bpart;
  int32_t* bcnt = reinterpret_cast<int32_t*>(ws + (int64_t)l.bcnt);
  double* partial = ws + (int64_t)l.partial;
  FwdArgs a{};
  a.x = x, a.y = y, a.w = w, a.ydtype = ydtype, a.wdtype = wdtype, a.n = n, a.d = d, a.R = R;
  a.K = R == 1 ? 2 : R, a.ct = (R + 15) / 16, a.coef = coef, a.icpt = icpt, a.predict = 0, a.logit_t = 0.0;
  a.q = q, a.bpart = bpart, a.bcnt = bcnt;
  launch_forward(dtype, a, s);
  const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (dtype == DType::F32) {
    if (vec) launch_gradient_tv<float, true>(x, n, d, R, q, p, partial, s);
    else launch_gradient_tv<float, false>(x, n, d, R, q, p, partial, s);
  } else {
    if (vec) launch_gradient_tv<double, true>(x, n, d, R, q, p, partial, s);
    else launch_gradient_tv<double, false>(x, n, d, R, q, p, partial, s);
  }
  TFA_LAUNCH_CHECK("lr_gradient");
  const int cells = R * (d + 1);
  hipLaunchKernelGGL(lr_finish, dim3((unsigned)((cells + kT - 1) / kT + 1)), dim3(kT), 0, s, cells, p.slices, p.blocks,
                     partial, bpart, bcnt, grad, loss, wsum, bad);
  TFA_LAUNCH_CHECK("lr_finish");
}

void logreg_predict(const void* x, DType dtype, int64_t n, int d, int R, const double* coef, const double* icpt,
                    double logit_threshold, int32_t* pred, double* raw, double* prob, hipStream_t s) {
  check_shape("logreg_predict", dtype, n, d, R);
  FwdArgs a{};
  a.x = x, a.n = n, a.d = d, a.R = R, a.K = R == 1 ? 2 : R, a.ct = (R + 15) / 16, a.coef = coef, a.icpt = icpt;
  a.ydtype = a.wdtype = DType::F64, a.predict = 1, a.logit_t = logit_threshold;
  a.pred = pred, a.raw = raw, a.prob = prob;
  launch_forward(dtype, a, s);
}

}  // namespace k
}  // namespace tfa
