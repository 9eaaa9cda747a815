// Zero-word packing of a contiguous device buffer before its device-to-host
// copy (pack_layout.h has the format; runtime/unpack.cpp expands it).
//
// One block packs one tile of kPackTileRows rows. Its four waves take one
// contiguous quarter of the tile each, 64 words (one per lane) at a time:
//
//   pass 1  a 64-bit ballot of "word != 0" is two mask words, written as they
//           come; its popcount adds to the wave's count;
//   reserve the block sums the four counts and takes [base, base + count) of
//           the value region with ONE atomicAdd on the 64-bit cursor
//           (header[0]); tiles therefore land in arbitrary order, which the
//           per-tile {offset, count} header entries make irrelevant;
//   pass 2  the tile (64 KiB at 512 words per row: still in L2) is read again
//           and every non-zero word goes to base + words kept before it,
//           from the wave's running count and the ballot bits below the lane.
//
// Only the bit pattern 0x00000000 is dropped: -0.0, NaN and denormals stay,
// so the expansion is bit-identical for every dtype.
#include "hip_common.h"
#include "pack_layout.h"

namespace tfa {
namespace k {

namespace {

constexpr int kPT = 256;  // threads per block
constexpr int kPW = kPT / kWave;
constexpr int kPU = 4;    // 64-word groups in flight per wave

__global__ __launch_bounds__(kPT) void pack_words_kernel(const uint32_t* __restrict__ src, int64_t rows, int64_t wpr,
                                                         uint64_t* __restrict__ header, uint32_t* __restrict__ mask,
                                                         uint32_t* __restrict__ values) {
  __shared__ uint32_t wtot[kPW];
  __shared__ unsigned long long sbase;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t t = blockIdx.x;
  const int64_t r0 = t * kPackTileRows;
  const int64_t r1 = r0 + kPackTileRows < rows ? r0 + kPackTileRows : rows;
  const int64_t e0 = r0 * wpr;                       // a multiple of 32
  const uint32_t n = (uint32_t)((r1 - r0) * wpr);    // < 2^31 (checked by the launcher)
  const uint32_t ngroups = (n + 63u) / 64u, per = (ngroups + kPW - 1) / kPW;
  const uint32_t g0 = min((uint32_t)wave * per, ngroups), g1 = min(g0 + per, ngroups);
  const uint32_t* __restrict__ s = src + e0;
  uint32_t* __restrict__ mw = mask + e0 / 32;
  const unsigned long long below = (1ull << lane) - 1ull;

  // mask words 2g and 2g + 1 of the tile, by lanes 0 and 1; the upper one may
  // belong to the next tile (n % 64 == 32) or lie past the mask
  auto put_mask = [&](uint32_t g, unsigned long long b) {
    if (lane < 2 && g * 64u + (uint32_t)lane * 32u < n) mw[2 * g + lane] = (uint32_t)(b >> (32 * lane));
  };

  uint32_t cnt = 0;
  uint32_t g = g0;
  for (; g + kPU <= g1 && (g + kPU) * 64u <= n; g += kPU) {  // whole groups: no bounds inside
    uint32_t w[kPU];
#pragma unroll
    for (int j = 0; j < kPU; ++j) w[j] = s[(g + j) * 64u + lane];
#pragma unroll
    for (int j = 0; j < kPU; ++j) {
      const unsigned long long b = __ballot(w[j] != 0u);
      put_mask(g + j, b);
      cnt += __popcll(b);
    }
  }
  for (; g < g1; ++g) {
    const uint32_t i = g * 64u + lane;
    const uint32_t w = i < n ? s[i] : 0u;
    const unsigned long long b = __ballot(w != 0u);
    put_mask(g, b);
    cnt += __popcll(b);
  }
  if (lane == 0) wtot[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kPW; ++w) total += wtot[w];
    const unsigned long long base = atomicAdd(reinterpret_cast<unsigned long long*>(header), total);
    header[1 + 2 * t] = base;
    header[2 + 2 * t] = total;
    sbase = base;
  }
  __syncthreads();
  unsigned long long pos = sbase;
#pragma unroll
  for (int w = 0; w < kPW; ++w)
    if (w < wave) pos += wtot[w];
  uint32_t* __restrict__ vout = values + pos;

  uint32_t run = 0;
  g = g0;
  for (; g + kPU <= g1 && (g + kPU) * 64u <= n; g += kPU) {
    uint32_t w[kPU];
#pragma unroll
    for (int j = 0; j < kPU; ++j) w[j] = s[(g + j) * 64u + lane];
#pragma unroll
    for (int j = 0; j < kPU; ++j) {
      const unsigned long long b = __ballot(w[j] != 0u);
      if (w[j] != 0u) vout[run + __popcll(b & below)] = w[j];
      run += __popcll(b);
    }
  }
  for (; g < g1; ++g) {
    const uint32_t i = g * 64u + lane;
    const uint32_t w = i < n ? s[i] : 0u;
    const unsigned long long b = __ballot(w != 0u);
    if (w != 0u) vout[run + __popcll(b & below)] = w;
    run += __popcll(b);
  }
}

}  // namespace

size_t pack_words_max_bytes(int64_t rows, int64_t wpr) { return pack_layout(rows, wpr).max_bytes; }

void pack_words(const void* src, int64_t rows, int64_t wpr, void* packed, hipStream_t s) {
  TFA_CHECK(rows >= 0 && wpr >= 0, "pack_words: negative shape");
  TFA_CHECK((reinterpret_cast<uintptr_t>(src) & 3) == 0 && (reinterpret_cast<uintptr_t>(packed) & 63) == 0,
            "pack_words: source must be 4-byte, destination 64-byte aligned");
  // the cursor (header[0]: total value words once the kernel is done)
  TFA_CHECK(hipMemsetAsync(packed, 0, 8, s) == hipSuccess, "pack_words: memset of the cursor failed");
  if (rows == 0 || wpr == 0) return;
  const PackLayout L = pack_layout(rows, wpr);
  TFA_CHECK(L.tiles < (int64_t(1) << 31), "pack_words: more than 2^31 tiles");
  TFA_CHECK(wpr * kPackTileRows < (int64_t(1) << 31), "pack_words: rows of ", wpr, " words are too wide");
  char* p = static_cast<char*>(packed);
  hipLaunchKernelGGL(pack_words_kernel, dim3((unsigned)L.tiles), dim3(kPT), 0, s, static_cast<const uint32_t*>(src),
                     rows, wpr, reinterpret_cast<uint64_t*>(p), reinterpret_cast<uint32_t*>(p + L.mask_off),
                     reinterpret_cast<uint32_t*>(p + L.values_off));
  TFA_LAUNCH_CHECK("pack_words_kernel");
}

}  // namespace k
}  // namespace tfa
