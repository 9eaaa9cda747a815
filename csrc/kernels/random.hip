// Counter-based random draws per row (DataFrame.sample / randomSplit /
// sampleBy, F.rand / F.randn).
//
// Every draw is a pure function of (seed, global row index, purpose):
// Philox4x32-10 (Salmon et al., SC'11) with the key (seed low, seed high) and
// the counter (row low, row high, purpose, 0); one call serves one row and
// gives four words w0..w3:
//
//   uniform  u  = (((w0 << 32) | w1) >> 11) * 2^-53            in [0, 1), exact
//   normal   u1 = ((((w0 << 32) | w1) >> 11) + 1) * 2^-53      in (0, 1]
//            u2 = (((w2 << 32) | w3) >> 11) * 2^-53
//            z  = sqrt(-2 ln u1) * cospi(2 u2)
//   poisson  the number of entries <= u of a host-built cdf table (<= 64
//            doubles, staged in LDS): no transcendental on the device
//
// The kernels read no memory but the tables: they are bound by the 20
// 32x32->64 multiplies per row and by the output store. A lane takes
// kRowsPerLane consecutive rows in an unrolled loop (the draws stay in
// registers) and stores them as one 8-byte word (mask bytes) or as 16-byte
// vectors (doubles, int64); the rows of the last, partial lane go out one by
// one. Row and counter arithmetic is 64-bit: row0 + i may carry into counter
// word 1 inside a tile. Plain stores only; no block talks to another.
#include <algorithm>

#include "hip_common.h"

// float64 sqrt / log / the products around them are evaluated as written
#pragma clang fp contract(off)

namespace tfa {
namespace k {

namespace {

constexpr int kRT = 256;                            // threads per block
constexpr int kRowsPerLane = 8;                     // consecutive rows of a lane
constexpr int kRandomTile = kRT * kRowsPerLane;     // rows per block
constexpr int kSmallStrata = 256;                   // sampleBy tables up to this size: 4 KiB of LDS
constexpr int kMaskByBlocks = 256 * 4;              // sampleBy: blocks stride over the tiles (table staged once)

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr double kTwoPow53Inv = 1.0 / 9007199254740992.0;  // 2^-53

enum : uint32_t { kPurposeUniform = 0, kPurposeNormal = 1, kPurposePoisson = 2 };

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));

struct Words4 {
  uint32_t w0, w1, w2, w3;
};

__device__ __forceinline__ Words4 philox(uint64_t seed, uint64_t row, uint32_t purpose) {
  uint32_t c0 = (uint32_t)row, c1 = (uint32_t)(row >> 32), c2 = purpose, c3 = 0;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
    const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return {c0, c1, c2, c3};
}

// the 53 high bits of (a << 32 | b)
__device__ __forceinline__ uint64_t bits53(uint32_t a, uint32_t b) { return (((uint64_t)a << 32) | b) >> 11; }

__device__ __forceinline__ double uniform_of(uint64_t seed, uint64_t row, uint32_t purpose) {
  const Words4 w = philox(seed, row, purpose);
  return (double)bits53(w.w0, w.w1) * kTwoPow53Inv;  // (an integer below 2^53 times a power of two: exact)
}

__device__ __forceinline__ double normal_of(uint64_t seed, uint64_t row) {
  const Words4 w = philox(seed, row, kPurposeNormal);
  const double u1 = (double)(bits53(w.w0, w.w1) + 1) * kTwoPow53Inv;
  const double u2 = (double)bits53(w.w2, w.w3) * kTwoPow53Inv;
  return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// the first row of this lane in the tile `tile`
__device__ __forceinline__ int64_t lane_row(int64_t tile) {
  return tile * kRandomTile + (int64_t)threadIdx.x * kRowsPerLane;
}

// v[0 .. kRowsPerLane) -> out[i0 ..), 16 bytes at a time when the lane is whole
template <typename T, typename V2>
__device__ __forceinline__ void store_lane8(T* __restrict__ out, int64_t i0, int64_t n, const T (&v)[kRowsPerLane],
                                            bool aligned16) {
  if (aligned16 && i0 + kRowsPerLane <= n) {
    V2* o = reinterpret_cast<V2*>(out + i0);
#pragma unroll
    for (int j = 0; j < kRowsPerLane / 2; ++j) {
      V2 p;
      p.x = v[2 * j];
      p.y = v[2 * j + 1];
      o[j] = p;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j)
      if (i0 + j < n) out[i0 + j] = v[j];
  }
}

// bit j of `bits` -> byte j of the lane's 8 mask bytes (0 / 1)
__device__ __forceinline__ void store_mask8(uint8_t* __restrict__ out, int64_t i0, int64_t n, uint32_t bits,
                                            bool aligned8) {
  if (aligned8 && i0 + kRowsPerLane <= n) {
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) w |= (uint64_t)((bits >> j) & 1u) << (8 * j);
    *reinterpret_cast<uint64_t*>(out + i0) = w;
  } else {
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j)
      if (i0 + j < n) out[i0 + j] = (uint8_t)((bits >> j) & 1u);
  }
}

}  // namespace

__global__ __launch_bounds__(kRT) void random_uniform_kernel(uint64_t seed, uint64_t row0, int64_t n,
                                                            double* __restrict__ out, int aligned) {
  const int64_t i0 = lane_row(blockIdx.x);
  if (i0 >= n) return;
  double v[kRowsPerLane];
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) v[j] = uniform_of(seed, row0 + (uint64_t)(i0 + j), kPurposeUniform);
  store_lane8<double, f64x2>(out, i0, n, v, aligned != 0);
}

__global__ __launch_bounds__(kRT) void random_normal_kernel(uint64_t seed, uint64_t row0, int64_t n,
                                                           double* __restrict__ out, int aligned) {
  const int64_t i0 = lane_row(blockIdx.x);
  if (i0 >= n) return;
  double v[kRowsPerLane];
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) v[j] = normal_of(seed, row0 + (uint64_t)(i0 + j));
  store_lane8<double, f64x2>(out, i0, n, v, aligned != 0);
}

// mask[i] = lo <= u_i < hi
__global__ __launch_bounds__(kRT) void random_mask_kernel(uint64_t seed, uint64_t row0, int64_t n, double lo,
                                                         double hi, uint8_t* __restrict__ out, int aligned) {
  const int64_t i0 = lane_row(blockIdx.x);
  if (i0 >= n) return;
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    const double u = uniform_of(seed, row0 + (uint64_t)(i0 + j), kPurposeUniform);
    bits |= (u >= lo && u < hi) ? (1u << j) : 0u;
  }
  store_mask8(out, i0, n, bits, aligned != 0);
}

// mask[i] = u_i < fraction of the stratum whose word is words[i] (0 when the
// table does not hold the word). table_words [S] ascending as unsigned,
// distinct; S <= CAP. The table is staged in LDS once per block, the blocks
// stride over the tiles.
template <int CAP>
__global__ __launch_bounds__(kRT) void random_mask_by_kernel(uint64_t seed, uint64_t row0, int64_t n,
                                                            const uint64_t* __restrict__ words,
                                                            const uint64_t* __restrict__ table_words,
                                                            const double* __restrict__ table_fractions, int S,
                                                            uint8_t* __restrict__ out, int aligned) {
  __shared__ uint64_t tw[CAP];
  __shared__ double tf[CAP];
  for (int i = threadIdx.x; i < S; i += kRT) {
    tw[i] = table_words[i];
    tf[i] = table_fractions[i];
  }
  __syncthreads();
  const int64_t ntiles = (n + kRandomTile - 1) / kRandomTile;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t i0 = lane_row(tile);
    if (i0 >= n) continue;
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
      const int64_t i = i0 + j;
      const uint64_t w = words[i < n ? i : n - 1];
      int a = 0, b = S;  // the first table entry that is not below w
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (tw[mid] < w) a = mid + 1;
        else b = mid;
      }
      const int at = a < S ? a : S - 1;  // (S >= 1)
      const double f = (a < S && tw[at] == w) ? tf[at] : 0.0;
      const double u = uniform_of(seed, row0 + (uint64_t)i, kPurposeUniform);
      bits |= (u < f) ? (1u << j) : 0u;
    }
    store_mask8(out, i0, n, bits, aligned != 0);
  }
}

// counts[i] = entries of cdf [len] (non-decreasing, len in 1..64) that are <= u_i
__global__ __launch_bounds__(kRT) void random_poisson_kernel(uint64_t seed, uint64_t row0, int64_t n,
                                                            const double* __restrict__ cdf, int len,
                                                            int64_t* __restrict__ out, int aligned) {
  __shared__ double table[kMaxPoissonTable];
  if (threadIdx.x < len) table[threadIdx.x] = cdf[threadIdx.x];
  __syncthreads();
  const int64_t i0 = lane_row(blockIdx.x);
  if (i0 >= n) return;
  long long v[kRowsPerLane];
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    const double u = uniform_of(seed, row0 + (uint64_t)(i0 + j), kPurposePoisson);
    int a = 0, b = len;  // the first entry above u
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (table[mid] <= u) a = mid + 1;
      else b = mid;
    }
    v[j] = a;
  }
  store_lane8<long long, i64x2>(reinterpret_cast<long long*>(out), i0, n, v, aligned != 0);
}

// offs [n + 1]: the exclusive scan of the counts (offs[n] == total). Row i is
// written to idx[offs[i] .. offs[i + 1]): neighbouring lanes write
// neighbouring ranges. Whatever offs holds, nothing outside [0, total) is
// written.
__global__ __launch_bounds__(kRT) void random_expand_kernel(const int64_t* __restrict__ offs, int64_t n,
                                                           int64_t total, int64_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * kRT + threadIdx.x;
  if (i >= n) return;
  int64_t a = offs[i], b = offs[i + 1];
  a = a < 0 ? 0 : a;
  b = b > total ? total : b;
  for (int64_t j = a; j < b; ++j) idx[j] = i;
}

// ------------------------------------------------------------------ host API
int random_tile_rows() { return kRandomTile; }

namespace {

unsigned random_blocks(const char* what, uint64_t row0, int64_t n) {
  TFA_CHECK(n > 0, what, ": negative row count");
  TFA_CHECK(row0 <= ~uint64_t(0) - static_cast<uint64_t>(n), what, ": row0 + n passes 2^64");
  const int64_t tiles = (n + kRandomTile - 1) / kRandomTile;
  TFA_CHECK(tiles < (int64_t(1) << 31), what, ": too many rows for one call");
  return static_cast<unsigned>(tiles);
}

template <typename T>
int aligned_to(const T* p, uintptr_t a) {
  return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0 ? 1 : 0;
}

}  // namespace

void random_uniform(uint64_t seed, uint64_t row0, int64_t n, double* out, hipStream_t s) {
  if (n == 0) return;
  const unsigned blocks = random_blocks("random_uniform", row0, n);
  TFA_CHECK(out != nullptr, "random_uniform: null buffer");
  hipLaunchKernelGGL(random_uniform_kernel, dim3(blocks), dim3(kRT), 0, s, seed, row0, n, out, aligned_to(out, 16));
  TFA_LAUNCH_CHECK("random_uniform_kernel");
}

void random_normal(uint64_t seed, uint64_t row0, int64_t n, double* out, hipStream_t s) {
  if (n == 0) return;
  const unsigned blocks = random_blocks("random_normal", row0, n);
  TFA_CHECK(out != nullptr, "random_normal: null buffer");
  hipLaunchKernelGGL(random_normal_kernel, dim3(blocks), dim3(kRT), 0, s, seed, row0, n, out, aligned_to(out, 16));
  TFA_LAUNCH_CHECK("random_normal_kernel");
}

void random_mask(uint64_t seed, uint64_t row0, int64_t n, double lo, double hi, uint8_t* out, hipStream_t s) {
  if (n == 0) return;
  const unsigned blocks = random_blocks("random_mask", row0, n);
  TFA_CHECK(out != nullptr, "random_mask: null buffer");
  hipLaunchKernelGGL(random_mask_kernel, dim3(blocks), dim3(kRT), 0, s, seed, row0, n, lo, hi, out,
                     aligned_to(out, 8));
  TFA_LAUNCH_CHECK("random_mask_kernel");
}

void random_mask_by(uint64_t seed, uint64_t row0, int64_t n, const int64_t* words, const int64_t* table_words,
                    const double* table_fractions, int strata, uint8_t* out, hipStream_t s) {
  if (n == 0) return;
  const unsigned tiles = random_blocks("random_mask_by", row0, n);
  TFA_CHECK(strata >= 1 && strata <= kMaxStrata, "random_mask_by: 1..", kMaxStrata, " strata, got ", strata);
  TFA_CHECK(words != nullptr && table_words != nullptr && table_fractions != nullptr && out != nullptr,
            "random_mask_by: null buffer");
  const unsigned blocks = std::min<unsigned>(tiles, kMaskByBlocks);
  const uint64_t* w = reinterpret_cast<const uint64_t*>(words);
  const uint64_t* t = reinterpret_cast<const uint64_t*>(table_words);
  if (strata <= kSmallStrata)
    hipLaunchKernelGGL((random_mask_by_kernel<kSmallStrata>), dim3(blocks), dim3(kRT), 0, s, seed, row0, n, w, t,
                       table_fractions, strata, out, aligned_to(out, 8));
  else
    hipLaunchKernelGGL((random_mask_by_kernel<kMaxStrata>), dim3(blocks), dim3(kRT), 0, s, seed, row0, n, w, t,
                       table_fractions, strata, out, aligned_to(out, 8));
  TFA_LAUNCH_CHECK("random_mask_by_kernel");
}

void random_poisson(uint64_t seed, uint64_t row0, int64_t n, const double* cdf, int len, int64_t* out,
                    hipStream_t s) {
  if (n == 0) return;
  const unsigned blocks = random_blocks("random_poisson", row0, n);
  TFA_CHECK(len >= 1 && len <= kMaxPoissonTable, "random_poisson: a table of 1..", kMaxPoissonTable,
            " entries, got ", len);
  TFA_CHECK(cdf != nullptr && out != nullptr, "random_poisson: null buffer");
  hipLaunchKernelGGL(random_poisson_kernel, dim3(blocks), dim3(kRT), 0, s, seed, row0, n, cdf, len, out,
                     aligned_to(out, 16));
  TFA_LAUNCH_CHECK("random_poisson_kernel");
}

void random_expand(const int64_t* offs, int64_t n, int64_t total, int64_t* idx, hipStream_t s) {
  TFA_CHECK(n >= 0 && total >= 0, "random_expand: negative row count");
  if (n == 0 || total == 0) return;
  TFA_CHECK(offs != nullptr && idx != nullptr, "random_expand: null buffer");
  const int64_t blocks = (n + kRT - 1) / kRT;
  TFA_CHECK(blocks < (int64_t(1) << 31), "random_expand: too many rows");
  hipLaunchKernelGGL(random_expand_kernel, dim3((unsigned)blocks), dim3(kRT), 0, s, offs, n, total, idx);
  TFA_LAUNCH_CHECK("random_expand_kernel");
}

}  // namespace k
}  // namespace tfa
