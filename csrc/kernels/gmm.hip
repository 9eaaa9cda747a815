// One EM step of a Gaussian mixture over a vector column (ml/clustering.py:
// GaussianMixture), and the model's prediction.
//
// x is [n][d], row-major, f32 or f64; means is [k][d], transforms [k][d][d] and
// logconst [k], f64. T_j = L_j^-1 is lower triangular with Sigma_j = L_j L_j^T,
// c_j = log w_j - (d / 2) log 2 pi - sum_i log L_j,ii, so that log p_ij = c_j -
// ||T_j (x_i - mu_j)||^2 / 2. 1 <= k <= kGmmMaxK, 1 <= d <= kGmmMaxD, k d^2 <=
// kGmmMaxKDD. All arithmetic is f64 on v_mfma_f64_16x16x4_f64. Three launches,
// no float atomics, no block waits for another one; no [n][k][d] array exists:
//
//   1. gm_estep   a block owns a stripe of 64 rows: it reads them from HBM
//                 once, converts them to f64 and keeps them in an LDS image
//                 [64][xp], xp = 32 ceil(d / 32) + 2, for all k components
//                 (features past d and rows past n are 0.0). A staging thread
//                 notes a NaN or an infinity among the values it converts.
//                 Four waves, each 16 rows against every z index: nt = ceil(d
//                 / 16) MFMA tiles whose accumulators hold z = T_j (x - mu_j)
//                 of the stripe. The walk is over (component j) x (chunk c of
//                 16 features). A stage is the rows 16 c .. 16 nt of T_j's
//                 columns 16 c .. 16 c + 15 as an LDS image [z index][feature]
//                 of pitch 18 doubles, and the 16 means of the chunk; two
//                 stages deep, the next stage's global loads issued before
//                 the current stage's MFMAs. The rows of T_j above 16 c are
//                 not read and the MFMA tiles t < c are skipped: they lie
//                 wholly above the diagonal (at d = 128, 36 of 64 tile-chunks
//                 are left); inside a diagonal tile an element above the
//                 diagonal is staged as 0.0 whatever the caller left there.
//                 The A fragment is lane l: x[r0 + l % 16][f0 + l / 16] -
//                 mu_j[f0 + l / 16], the mean subtracted as the fragment is
//                 read (no offset T_j mu_j, which would cancel for a
//                 component far from the origin); the B fragment is lane l:
//                 T_j[i0 + l % 16][f0 + l / 16]. Both are the read pattern
//                 img[i + l % 16][f + l / 16]: with a pitch of 2 (mod 32) (x
//                 image) or 18 (T image) doubles the 32 lanes that an 8-byte
//                 ds_read serves at a time fall on 32 distinct 8-byte bank
//                 pairs (2 m + g or 18 m + g (mod 32), m = 0..15, g two
//                 consecutive values: 18 m (mod 32) runs through the 16 even
//                 residues): free of conflicts by this arithmetic, not by a
//                 counter measurement. After the last chunk of a component a
//                 lane squares its accumulator elements and adds them in tile
//                 order, the 16 lanes that share a row are folded by the xor
//                 butterfly 1, 2, 4, 8 (a + b is commutative: the same bits in
//                 every lane), and log p_ij = c_j - ||z||^2 / 2 goes to an LDS
//                 table [64][k + 1]. The row epilogue (four lanes a row, lane
//                 s the components s, s + 4, ... in order, then the butterfly
//                 1, 2): M = max_j log p, lse = M + log sum exp(log p - M),
//                 r_j = exp(log p_j - lse). A row that holds a NaN or an
//                 infinity, or whose lse is not finite, gets r = 0 and is
//                 counted. r leaves as one contiguous [rows][k] store. Out: r
//                 [n][k] and per block the sum of its lse in row order and
//                 its count of left-out rows. In prediction mode r is the
//                 output `prob`, and pred [n] is the first largest r_j (-1
//                 for a left-out row).
//   2. gm_mstep   with y = [x - mu_j, 1] (d + 1 entries: the appended ones
//                 column carries N and S), G_j = sum_i r_ij y_i y_i^T holds
//                 C_j (the leading d x d), S_j (the last column) and N_j (the
//                 corner). The grid is (slice of slice_rows rows) x
//                 (component) x (pair bi <= bj of 64-wide tiles of the d + 1
//                 entries). Per stage of 32 rows the bi and the bj segment of
//                 every row go to an LDS image [row][entry] exactly as in
//                 vm_syrk (vector_moments.hip: pitch 144 doubles, the same
//                 conflict arithmetic), centred at the component's current
//                 mean; a value that is not finite is staged as 0.0 (its row
//                 has r = 0, and 0.0 * NaN is not 0.0), entry d is 1.0 for
//                 the rows of the slice. The r_ij of the stage sit in LDS
//                 [32]. Lane l reads y[r0 + l / 16][e0 + l % 16] for both
//                 operands and scales the A fragment by r[r0 + l / 16] in
//                 registers; B is the plain fragment. The f64 MFMA adds its
//                 four products in row order, so a sum is the rows of the
//                 slice in row order. On a diagonal pair the tiles below the
//                 diagonal are skipped, as are tiles wholly past d + 1. Out:
//                 partial [slice][component][pair][64 * 64].
//   3. gm_finish  one thread per (j, e, f), e <= f <= d, folds the partials
//                 in slice order and writes C_j,ef and its mirror (exactly
//                 symmetric), S_j,e (f = d) or N_j (e = f = d); one wave folds
//                 the block records (a lane its blocks l, l + 64, ... in block
//                 order, then the lanes in lane order): loglik and bad.
//
// At d <= 15 one of the sixteen 16 x 16 MFMA tiles of a gm_mstep block is live
// and three of its waves only stage; gm_estep's 16-wide z tiles waste 16 ceil(d
// / 16) - d columns. At d = 64 and d = 128 the ones column opens a tile of its
// own: 3 pairs instead of 1, 6 instead of 3, the extra blocks with one live
// MFMA column. docs/PERFORMANCE.md says what that costs.
//
// The order of every addition depends on (n, d, k, slice_rows) alone: the same
// bits on every run. Every row index is compared with n (or the slice's end),
// every component index with k and every feature index with d before an
// address is formed.
#include <algorithm>
#include <cmath>

#include "hip_common.h"

namespace tfa {
namespace k {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kT = 256;             // threads per block
constexpr int kRows = 64;           // rows per stripe of gm_estep
constexpr int kChunk = 16;          // gm_estep: features per stage, z indices per MFMA tile
constexpr int kPitchT = kChunk + 2; // gm_estep: doubles per row of the T image
constexpr int kTileF = 64;          // gm_mstep: entries per tile
constexpr int kStage = kGmmStage;   // gm_mstep: rows per stage
constexpr int kPitchM = 2 * kTileF + 16;  // gm_mstep: doubles per LDS row, 144 (vm_syrk's)
constexpr int kTileElems = kTileF * kTileF;
constexpr size_t kMstepLds = (2 * kStage * kPitchM + 2 * kTileF + 2 * kStage) * sizeof(double);
constexpr int kTargetBlocks = 512;  // the 256 CUs about twice over
constexpr int64_t kMinSliceRows = 256;

// gm_estep's LDS in doubles: the x image, two T stages with their 16 means, the
// log p table, the rows' lse; then the rows' x flag and left-out flag (ints)
constexpr int est_xp(int d) { return 32 * ((d + 31) / 32) + 2; }
constexpr int est_stage(int nt) { return 16 * nt * kPitchT + kChunk; }
constexpr size_t est_lds(int d, int k) {
  return (size_t)(kRows * est_xp(d) + 2 * est_stage((d + 15) / 16) + kRows * (k + 1) + kRows) * sizeof(double) +
         2 * kRows * sizeof(int);
}

template <typename T>
struct Quad {  // four consecutive elements of a row
  T v[4];
};

template <typename T, bool VEC>
__device__ __forceinline__ Quad<T> gm_load4(const T* __restrict__ p, int f0, int d) {
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

struct EArgs {
  const void* x;
  int64_t n;
  int d, k, nt;
  const double* means;
  const double* transforms;
  const double* logconst;
  double* r;       // [n][k]: the responsibilities (prediction mode: prob)
  double* bll;     // step: [blocks] sum of lse
  int32_t* bbad;   // step: [blocks] left-out rows
  int32_t* pred;   // predict: [n]
};

// ------------------------------------------------------------------ 1. E step
template <typename T, bool VEC, bool TVEC, int NT>
__global__ __launch_bounds__(kT) void gm_estep(const EArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];  // see est_lds
  const int d = a.d, k = a.k, nt = a.nt;
  const int64_t n = a.n;
  const int xp = est_xp(d), stage = est_stage(nt), kp = k + 1;
  double* ximg = lds;
  double* timg = ximg + kRows * xp;
  double* logp = timg + 2 * stage;
  double* rowl = logp + kRows * kp;
  int* xbad = reinterpret_cast<int*>(rowl + kRows);
  int* rowbad = xbad + kRows;
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const double* __restrict__ tr = a.transforms;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  if (tid < kRows) xbad[tid] = 0;
  __syncthreads();

  // the stripe, once: thread -> quads e, e + 256, ... of the 64 x (xp - 2) / 4
  {
    const int qpr = (xp - 2) / 4;
    for (int e = tid; e < kRows * qpr; e += kT) {
      const int rr = e / qpr, f0 = (e - rr * qpr) * 4;
      const int64_t row = row0 + rr;
      Quad<T> q;
      if (row < n) {
        q = gm_load4<T, VEC>(x + row * d + f0, f0, d);
      } else {
        q.v[0] = q.v[1] = q.v[2] = q.v[3] = T(0);
      }
      double v[4];
      int nf = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        v[c] = (double)q.v[c];
        nf |= !isfinite(v[c]);
      }
      if (nf) atomicOr(&xbad[rr], 1);
      double* p = ximg + rr * xp + f0;
      *reinterpret_cast<double2*>(p) = double2{v[0], v[1]};
      *reinterpret_cast<double2*>(p + 2) = double2{v[2], v[3]};
    }
  }

  // staging of T_j: thread -> quad q of the chunk's 4 quads, z indices 16 c + r and 16 c + r + 64
  const int q = tid & 3, r = tid >> 2;
  Quad<double> tq[2];
  double mu = 0.0;
  int ld_c = 0;
  auto load = [&](int st) __attribute__((always_inline)) {
    const int j = st / nt;
    ld_c = st - j * nt;
    const int f0 = ld_c * kChunk + q * 4;
    const double* tj = tr + (int64_t)j * d * d;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = ld_c * kChunk + r + 64 * h;
      if (i < d) {
        tq[h] = gm_load4<double, TVEC>(tj + (int64_t)i * d + f0, f0, d);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (f0 + e > i) tq[h].v[e] = 0.0;  // (above the diagonal: zero by contract)
      } else {
        tq[h].v[0] = tq[h].v[1] = tq[h].v[2] = tq[h].v[3] = 0.0;
      }
    }
    if (tid < kChunk) {
      const int f = ld_c * kChunk + tid;
      mu = f < d ? a.means[(int64_t)j * d + f] : 0.0;
    }
  };
  auto store = [&](int buf) __attribute__((always_inline)) {  // (what the last load() fetched)
    double* img = timg + buf * stage;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = ld_c * kChunk + r + 64 * h;
      if (i < 16 * nt) {
        double* p = img + i * kPitchT + q * 4;
        *reinterpret_cast<double2*>(p) = double2{tq[h].v[0], tq[h].v[1]};
        *reinterpret_cast<double2*>(p + 2) = double2{tq[h].v[2], tq[h].v[3]};
      }
    }
    if (tid < kChunk) img[16 * nt * kPitchT + tid] = mu;
  };

  const bool en = row0 + wave * 16 < n;  // the wave's row tile is not wholly past n
  f64x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int a_off = (wave * 16 + (lane & 15)) * xp + (lane >> 4);
  const int b_off = (lane & 15) * kPitchT + (lane >> 4);
  const int total = k * nt;
  load(0);
  store(0);
  __syncthreads();
  int j = 0, c = 0;
  for (int st = 0; st < total; ++st) {
    const int cur = st & 1;
    const bool more = st + 1 < total;
    if (more) load(st + 1);  // in flight under the MFMAs
    const double* img = timg + cur * stage;
    const double* mus = img + 16 * nt * kPitchT;
    if (en) {
#pragma unroll
      for (int kk = 0; kk < kChunk / 4; ++kk) {
        const double av = ximg[a_off + c * kChunk + kk * 4] - mus[kk * 4 + (lane >> 4)];
        static_for<NT>([&](auto tc) __attribute__((always_inline)) {
          constexpr int t = decltype(tc)::value;
          if (t >= c && t < nt) {  // (tiles t < c lie wholly above the diagonal)
            const double bv = img[b_off + t * 16 * kPitchT + kk * 4];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
          }
        });
      }
    }
    if (c == nt - 1) {  // the accumulators hold z of component j
      // f64 C/D layout: col (z index) = lane & 15, row = (lane >> 4) + 4 * reg
      const double cj = a.logconst[j];
      double s[4] = {0.0, 0.0, 0.0, 0.0};
      static_for<NT>([&](auto tc) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value;
        if (t < nt) {
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) s[rg] += acc[t][rg] * acc[t][rg];  // (tile order)
          acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
        }
      });
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) s[rg] += __shfl_xor(s[rg], off, 64);
        if ((lane & 15) == 0) logp[(wave * 16 + (lane >> 4) + 4 * rg) * kp + j] = cj - 0.5 * s[rg];
      }
      c = 0;
      ++j;
    } else {
      ++c;
    }
    if (more) store(cur ^ 1);  // (every wave left that image before the previous barrier)
    __syncthreads();
  }

  // the row epilogue: lanes sub = 0..3 of row rl
  const int rl = tid >> 2, sub = tid & 3;
  const int64_t row = row0 + rl;
  const bool live = row < n;
  double* lp = logp + rl * kp;
  double M = -__builtin_inf();
  for (int cc = sub; cc < k; cc += 4) M = fmax(M, lp[cc]);
  M = fmax(M, __shfl_xor(M, 1, 64));
  M = fmax(M, __shfl_xor(M, 2, 64));
  double S = 0.0;
  for (int cc = sub; cc < k; cc += 4) S += exp(lp[cc] - M);
  S += __shfl_xor(S, 1, 64);
  S += __shfl_xor(S, 2, 64);
  const double lse = M + log(S);
  const bool use = live && xbad[rl] == 0 && isfinite(lse);
  double bv = -1.0;
  int bi = k;
  for (int cc = sub; cc < k; cc += 4) {
    const double p = use ? exp(lp[cc] - lse) : 0.0;
    lp[cc] = p;
    if (p > bv) bv = p, bi = cc;  // (component order: the first of equal ones)
  }
  if (a.pred != nullptr) {
#pragma unroll
    for (int off = 1; off < 4; off <<= 1) {
      const double ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    if (sub == 0 && live) a.pred[row] = use ? bi : -1;
  }
  if (sub == 0) {
    rowl[rl] = use ? lse : 0.0;
    rowbad[rl] = (live && !use) ? 1 : 0;
  }
  __syncthreads();
  for (int e = tid; e < kRows * k; e += kT) {  // one contiguous [rows][k] store
    const int rr = e / k, cc = e - rr * k;
    if (row0 + rr < n) a.r[row0 * k + e] = logp[rr * kp + cc];
  }
  if (tid == 0 && a.bll != nullptr) {
    double t = 0.0;
    int b = 0;
    for (int i = 0; i < kRows; ++i) {  // (row order)
      t += rowl[i];
      b += rowbad[i];
    }
    a.bll[blockIdx.x] = t;
    a.bbad[blockIdx.x] = b;
  }
}

// ------------------------------------------------------------------ 2. M step: k weighted SYRKs of [x - mu_j, 1]
template <typename T, bool VEC>
__global__ __launch_bounds__(kT) void gm_mstep(const T* __restrict__ x, int64_t n, int d, int k, int tiles, int pairs,
                                               int64_t slice_rows, const double* __restrict__ means,
                                               const double* __restrict__ rw, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double lds[];  // [2][kStage][kPitchM], the 128 means, r [2][kStage]
  double* shift_lds = lds + 2 * kStage * kPitchM;
  double* rimg = shift_lds + 2 * kTileF;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int pair = blockIdx.x % (unsigned)pairs;
  const unsigned rest = blockIdx.x / (unsigned)pairs;
  const int j = rest % (unsigned)k;
  const int64_t sl = rest / (unsigned)k;
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
    shift_lds[tid] = f < d ? means[(int64_t)j * d + f] : 0.0;
  }
  __syncthreads();

  // staging: thread -> quad q of the 32 quads of a row image (16 of the bi
  // segment, 16 of the bj segment) and rows g, g + 8, g + 16, g + 24 of a stage
  const int q = tid & 31, g = tid >> 5;
  const bool seg_b = q >= 16;
  const int f0 = (seg_b ? bj : bi) * kTileF + (q & 15) * 4;
  const bool active = !(diag && seg_b);  // a diagonal pair has one segment
  double sh[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) sh[e] = shift_lds[q * 4 + e];
  Quad<T> raw[4];
  double rr[4];
  auto load = [&](int64_t rs) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int64_t row = rs + g + 8 * h;
      if (active && row < r_end) {
        raw[h] = gm_load4<T, VEC>(x + row * d + f0, f0, d);
      } else {
        raw[h].v[0] = raw[h].v[1] = raw[h].v[2] = raw[h].v[3] = T(0);
      }
      rr[h] = (q == 0 && row < r_end) ? rw[row * k + j] : 0.0;
    }
  };
  auto store = [&](int64_t rs, int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      if (q == 0) rimg[buf * kStage + g + 8 * h] = rr[h];
      if (!active) continue;
      const bool row_ok = rs + g + 8 * h < r_end;
      double v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double t = (double)raw[h].v[e];
        v[e] = (row_ok && f0 + e < d && isfinite(t)) ? t - sh[e] : 0.0;  // (padding is 0.0, not 0 - mean)
        if (row_ok && f0 + e == d) v[e] = 1.0;                           // the ones column
      }
      double* p = lds + (buf * kStage + g + 8 * h) * kPitchM + q * 4;
      *reinterpret_cast<double2*>(p) = double2{v[0], v[1]};
      *reinterpret_cast<double2*>(p + 2) = double2{v[2], v[3]};
    }
  };

  // which of the wave's 2x2 MFMA tiles hold anything: not wholly past d + 1,
  // and on a diagonal pair not below the diagonal (gm_finish reads e <= f only)
  const int d1 = d + 1;
  bool en[2][2];
  bool any = false;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int ti = wm * 2 + i, tj = wn * 2 + jj;
      en[i][jj] = bi * kTileF + ti * 16 < d1 && bj * kTileF + tj * 16 < d1 && !(diag && ti > tj);
      any = any || en[i][jj];
    }
  const int a_off = wm * 32 + (lane & 15), b_off = (diag ? 0 : kTileF) + wn * 32 + (lane & 15);
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) acc[i][jj] = f64x4{0.0, 0.0, 0.0, 0.0};

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
      const double* img = lds + (cur * kStage + (lane >> 4)) * kPitchM;
      const double* rs = rimg + cur * kStage + (lane >> 4);
#pragma unroll
      for (int kk = 0; kk < kStage / 4; ++kk) {
        const double rv = rs[kk * 4];
        double av[2], bv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          av[i] = img[kk * 4 * kPitchM + a_off + i * 16] * rv;  // (the scaled fragment)
          bv[i] = img[kk * 4 * kPitchM + b_off + i * 16];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
            if (en[i][jj]) acc[i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[jj], acc[i][jj], 0, 0, 0);
      }
    }
    if (more) store(next0, cur ^ 1);  // (every wave left that image before the previous barrier)
    __syncthreads();
  }

  // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
  double* out = partial + ((sl * k + j) * pairs + pair) * kTileElems;
  static_for<2>([&](auto ic) __attribute__((always_inline)) {
    constexpr int i = decltype(ic)::value;
    static_for<2>([&](auto jc) __attribute__((always_inline)) {
      constexpr int jj = decltype(jc)::value;
      const f64x4 v = acc[i][jj];
#pragma unroll
      for (int rg = 0; rg < 4; ++rg)
        out[(wm * 32 + i * 16 + (lane >> 4) + 4 * rg) * kTileF + wn * 32 + jj * 16 + (lane & 15)] = v[rg];
    });
  });
}

// ------------------------------------------------------------------ 3. finish
__global__ __launch_bounds__(kT) void gm_finish(int d, int k, int tiles, int pairs, int64_t slices, int64_t blocks,
                                                const double* __restrict__ partial, const double* __restrict__ bll,
                                                const int32_t* __restrict__ bbad, double* __restrict__ N,
                                                double* __restrict__ S, double* __restrict__ C,
                                                double* __restrict__ loglik, int64_t* __restrict__ bad) {
  __shared__ double ll[kWave];
  __shared__ int64_t lb[kWave];
  const int tid = threadIdx.x;
  const int d1 = d + 1;
  if (blockIdx.x + 1 < gridDim.x) {  // the sums
    const int e = blockIdx.x * kT + tid;
    if (e >= k * d1 * d1) return;
    const int j = e / (d1 * d1), rem = e - j * d1 * d1;
    const int fi = rem / d1, fj = rem - fi * d1;
    if (fj < fi) return;  // (written by the thread of (fj, fi))
    const int bi = fi / kTileF, bj = fj / kTileF;
    const int pair = bi * tiles - bi * (bi - 1) / 2 + (bj - bi);
    const double* p = partial + ((int64_t)j * pairs + pair) * kTileElems + (fi % kTileF) * kTileF + (fj % kTileF);
    const int64_t stride = (int64_t)k * pairs * kTileElems;
    double t = 0.0;
    for (int64_t s = 0; s < slices; ++s) t += p[s * stride];  // (slice order)
    if (fj < d) {
      C[((int64_t)j * d + fi) * d + fj] = t;
      C[((int64_t)j * d + fj) * d + fi] = t;
    } else if (fi < d) {
      S[(int64_t)j * d + fi] = t;
    } else {
      N[j] = t;
    }
    return;
  }
  if (tid < kWave) {  // the last block: the block records
    double t = 0.0;
    int64_t b = 0;
    for (int64_t i = tid; i < blocks; i += kWave) {  // (block order)
      t += bll[i];
      b += bbad[i];
    }
    ll[tid] = t;
    lb[tid] = b;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    int64_t b = 0;
    for (int i = 0; i < kWave; ++i) {  // (lane order)
      t += ll[i];
      b += lb[i];
    }
    loglik[0] = t;
    bad[0] = b;
  }
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

void check_shape(const char* what, DType dtype, int64_t n, int d, int k) {
  TFA_CHECK(dtype == DType::F32 || dtype == DType::F64, what, ": float32 or float64 cells expected");
  TFA_CHECK(n >= 1 && d >= 1 && d <= kGmmMaxD && k >= 1 && k <= kGmmMaxK && (int64_t)k * d * d <= kGmmMaxKDD, what,
            ": n >= 1, 1 <= d <= ", kGmmMaxD, ", 1 <= k <= ", kGmmMaxK, " and k d^2 <= ", kGmmMaxKDD,
            " expected, got n = ", n, ", d = ", d, ", k = ", k);
  TFA_CHECK(ceil_div(n, kRows) < (int64_t(1) << 31), what, ": too many rows for one call");
}

// the workspace, in doubles: r [n][k], the block records, the slice partials
struct Layout {
  double r, bll, bbad, partial, words;
};
Layout layout(int64_t n, int k, const GmmPlan& p) {
  auto even = [](double w) { return 2.0 * std::ceil(w / 2.0); };
  Layout l;
  l.r = 0;
  l.bll = l.r + even((double)n * k);
  l.bbad = l.bll + even((double)p.blocks);
  l.partial = l.bbad + even((double)p.blocks / 2.0);
  l.words = l.partial + (double)p.slices * k * p.pairs * kTileElems;
  return l;
}

template <typename T, bool VEC, bool TVEC, int NT>
void launch_estep_nt(const EArgs& a, unsigned blocks, hipStream_t s) {
  const size_t lds = est_lds(a.d, a.k);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gm_estep<T, VEC, TVEC, NT>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)est_lds(kGmmMaxD, kGmmMaxK));
  hipLaunchKernelGGL((gm_estep<T, VEC, TVEC, NT>), dim3(blocks), dim3(kT), lds, s, a);
}

template <typename T, bool VEC, bool TVEC>
void launch_estep_tv(const EArgs& a, unsigned blocks, hipStream_t s) {
  if (a.nt <= 1) launch_estep_nt<T, VEC, TVEC, 1>(a, blocks, s);
  else if (a.nt <= 2) launch_estep_nt<T, VEC, TVEC, 2>(a, blocks, s);
  else if (a.nt <= 4) launch_estep_nt<T, VEC, TVEC, 4>(a, blocks, s);
  else launch_estep_nt<T, VEC, TVEC, 8>(a, blocks, s);
}

void launch_estep(DType dtype, const EArgs& a, hipStream_t s) {
  const unsigned blocks = (unsigned)ceil_div(a.n, kRows);
  const bool vec = a.d % 4 == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
  const bool tvec = a.d % 4 == 0 && (reinterpret_cast<uintptr_t>(a.transforms) & 15) == 0;
  // (the T image is the same for both; the scalar-load T path goes with the scalar-load x path)
  if (dtype == DType::F32) {
    if (vec && tvec) launch_estep_tv<float, true, true>(a, blocks, s);
    else launch_estep_tv<float, false, false>(a, blocks, s);
  } else {
    if (vec && tvec) launch_estep_tv<double, true, true>(a, blocks, s);
    else launch_estep_tv<double, false, false>(a, blocks, s);
  }
  TFA_LAUNCH_CHECK("gm_estep");
}

EArgs estep_args(const void* x, int64_t n, int d, int k, const double* means, const double* transforms,
                 const double* logconst) {
  EArgs a{};
  a.x = x, a.n = n, a.d = d, a.k = k, a.nt = (d + kChunk - 1) / kChunk;
  a.means = means, a.transforms = transforms, a.logconst = logconst;
  return a;
}

}  // namespace

GmmPlan gmm_plan(int64_t n, int d, int k, int64_t slice_rows) {
  check_shape("gmm", DType::F64, n, d, k);
  GmmPlan p;
  p.tiles = (d + 1 + kTileF - 1) / kTileF;
  p.pairs = p.tiles * (p.tiles + 1) / 2;
  p.blocks = ceil_div(n, kRows);
  if (slice_rows <= 0) {
    const int64_t target = std::max<int64_t>(1, kTargetBlocks / (k * p.pairs));
    slice_rows = std::max(kMinSliceRows, ceil_div(ceil_div(n, target), kStage) * kStage);
  }
  TFA_CHECK(slice_rows % kStage == 0, "gmm: slice_rows must be a multiple of ", kStage, ", got ", slice_rows);
  p.slice_rows = slice_rows;
  p.slices = ceil_div(n, slice_rows);
  const double words = layout(n, k, p).words;
  TFA_CHECK(words * 8 <= (double)kGmmMaxWorkspace && p.slices * k * p.pairs < (int64_t(1) << 31),
            "gmm: ", n, " rows x ", k, " responsibilities and ", p.slices, " slices need more than the workspace of ",
            kGmmMaxWorkspace >> 20, " MB; use smaller partitions or larger slices");
  p.workspace_bytes = static_cast<size_t>(words) * 8;
  return p;
}

void gmm_step(const void* x, DType dtype, int64_t n, int d, int k, const double* means, const double* transforms,
              const double* logconst, const GmmPlan& p, double* N, double* S, double* C, double* loglik, int64_t* bad,
              void* workspace, size_t workspace_size, hipStream_t s) {
  check_shape("gmm_step", dtype, n, d, k);
  TFA_CHECK(p.blocks == ceil_div(n, kRows) && p.slice_rows >= 1 && p.slice_rows % kStage == 0 &&
                p.slices == ceil_div(n, p.slice_rows) && p.tiles == (d + 1 + kTileF - 1) / kTileF &&
                p.pairs == p.tiles * (p.tiles + 1) / 2 && workspace_size >= p.workspace_bytes,
            "gmm_step: bad arguments");
  const Layout l = layout(n, k, p);
  double* ws = static_cast<double*>(workspace);
  double* r = ws + (int64_t)l.r;
  double* bll = ws + (int64_t)l.bll;
  int32_t* bbad = reinterpret_cast<int32_t*>(ws + (int64_t)l.bbad);
  double* partial = ws + (int64_t)l.partial;
  EArgs a = estep_args(x, n, d, k, means, transforms, logconst);
  a.r = r, a.bll = bll, a.bbad = bbad;
  launch_estep(dtype, a, s);
  const unsigned grid = (unsigned)(p.slices * k * p.pairs);
  const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
#define TFA_GM_MSTEP(T_, VEC_)                                                                                     \
  do {                                                                                                             \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gm_mstep<T_, VEC_>),                                  \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMstepLds);                         \
    hipLaunchKernelGGL((gm_mstep<T_, VEC_>), dim3(grid), dim3(kT), kMstepLds, s, static_cast<const T_*>(x), n, d,  \
                       k, p.tiles, p.pairs, p.slice_rows, means, r, partial);                                      \
  } while (0)
  if (dtype == DType::F32) {
    if (vec) TFA_GM_MSTEP(float, true);
    else TFA_GM_MSTEP(float, false);
  } else {
    if (vec) TFA_GM_MSTEP(double, true);
    else TFA_GM_MSTEP(double, false);
  }
#undef TFA_GM_MSTEP
  TFA_LAUNCH_CHECK("gm_mstep");
  const int cells = k * (d + 1) * (d + 1);
  hipLaunchKernelGGL(gm_finish, dim3((unsigned)((cells + kT - 1) / kT + 1)), dim3(kT), 0, s, d, k, p.tiles, p.pairs,
                     p.slices, p.blocks, partial, bll, bbad, N, S, C, loglik, bad);
  TFA_LAUNCH_CHECK("gm_finish");
}

void gmm_predict(const void* x, DType dtype, int64_t n, int d, int k, const double* means, const double* transforms,
                 const double* logconst, double* prob, int32_t* pred, hipStream_t s) {
  check_shape("gmm_predict", dtype, n, d, k);
  EArgs a = estep_args(x, n, d, k, means, transforms, logconst);
  a.r = prob, a.pred = pred;
  launch_estep(dtype, a, s);
}

}  // namespace k
}  // namespace tfa
