// First row of every run of equal key tuples in a sorted order
// (DataFrame.dropDuplicates / distinct).
//
// words [W][n] are sort_encode's words, perm [n] the stable order of
// sort_argsort (null: the rows are in order already). Position i of the order
// is a head when i == 0 or when any word of row perm[i] differs from that word
// of row perm[i - 1]; kept [m] lists perm[i] of the heads, in order. Like
// compact.hip: plan, a single-block scan, write.
//
//   plan   one block per tile of kUniqueTile positions, 8 consecutive
//          positions per lane. Word after word, a lane gathers the word of
//          its own rows once and compares neighbours in registers; the row
//          before its first one is the last row of the lane below (a wave
//          shuffle), of the wave below (through LDS) or, for the first
//          position of a tile, one more load. The head bits of a lane are one
//          byte of a bit array of ceil(n / 8) bytes; heads are counted with
//          64-bit ballots and ONE count is written per tile;
//   scan   the tile counts become 64-bit output offsets and the total
//          (compact.hip's single-block scan), which the host reads with one
//          stream synchronisation (to size `kept`);
//   write  each block reads its tile's head bits (no word is gathered again),
//          ranks them (ballots, per-wave prefix in LDS), lists the tile's
//          heads in LDS and stores perm of them at [tile offset, + count):
//          the stores are linear, the loads of perm stay inside the tile.
//
// Positions, row indices, counts and offsets are 64-bit; only positions
// INSIDE one tile are 16-bit. Every loop is bounded by W, the tile or the
// lane's 8 positions; no block reads what another block of its launch wrote.
#include "hip_common.h"

namespace tfa {
namespace k {

namespace {

constexpr int kUT = 256;                        // threads per plan / write block
constexpr int kPerLane = 8;                     // positions per lane: one byte of head bits
constexpr int kUniqueTile = kUT * kPerLane;     // positions per tile
constexpr int kWaves = kUT / kWave;

static_assert(kUniqueTile <= 65536, "in-tile positions are kept as uint16");

// heads of the lower lanes of this wave (prefix) and of the whole wave
// (total); a lane's positions are consecutive, so lane order is position order
__device__ __forceinline__ void wave_rank(uint32_t bits, int lane, int& prefix, int& total) {
  const unsigned long long below = (1ull << lane) - 1ull;
  prefix = 0;
  total = 0;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const unsigned long long b = __ballot((bits >> j) & 1u);
    prefix += __popcll(b & below);
    total += __popcll(b);
  }
}

}  // namespace

__global__ __launch_bounds__(kUT) void unique_plan_kernel(const int64_t* __restrict__ words, int W, int64_t n,
                                                          const int64_t* __restrict__ perm,
                                                          uint8_t* __restrict__ head_bits,
                                                          int32_t* __restrict__ tile_counts) {
  __shared__ int64_t wlast[kMaxSortKeys][kWaves];  // word w of the last position of every wave
  __shared__ int wtot[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t tile0 = (int64_t)blockIdx.x * kUniqueTile;
  const int64_t pos0 = tile0 + (int64_t)tid * kPerLane;
  // the source rows of the lane's positions; a position past the end repeats
  // the last row, so every load below stays inside [0, n)
  int64_t src[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int64_t p = pos0 + j < n ? pos0 + j : n - 1;
    src[j] = perm != nullptr ? perm[p] : p;
  }
  // (tile0 < n for every block of the launch; tile0 - 1 >= 0 past the first tile)
  const int64_t before = tile0 > 0 ? (perm != nullptr ? perm[tile0 - 1] : tile0 - 1) : 0;
  uint32_t bits = 0;
  for (int w = 0; w < W; ++w) {  // (W is the same for the whole block: the barrier is met by all)
    const int64_t* __restrict__ col = words + (int64_t)w * n;
    int64_t v[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) v[j] = col[src[j]];
    if (lane == kWave - 1) wlast[w][wave] = v[kPerLane - 1];
    int64_t prev = __shfl_up(v[kPerLane - 1], 1, kWave);
    __syncthreads();
    if (lane == 0) prev = wave > 0 ? wlast[w][wave - 1] : col[before];
    if (v[0] != prev) bits |= 1u;
#pragma unroll
    for (int j = 1; j < kPerLane; ++j)
      if (v[j] != v[j - 1]) bits |= 1u << j;
  }
  if (pos0 == 0) bits |= 1u;  // the first position of the order
  // positions past the end hold no row
  const int64_t left = n - pos0;
  bits &= left >= kPerLane ? 0xffu : left > 0 ? (1u << left) - 1u : 0u;
  if (left > 0) head_bits[pos0 / kPerLane] = (uint8_t)bits;
  int prefix, total;
  wave_rank(bits, lane, prefix, total);
  if (lane == 0) wtot[wave] = total;
  __syncthreads();
  if (tid == 0) {
    int c = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) c += wtot[i];
    tile_counts[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(kUT) void unique_write_kernel(const uint8_t* __restrict__ head_bits, int64_t n,
                                                           const int64_t* __restrict__ perm,
                                                           const int64_t* __restrict__ tile_offs,
                                                           int64_t* __restrict__ kept) {
  __shared__ uint16_t heads[kUniqueTile];
  __shared__ int wtot[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t tile0 = (int64_t)blockIdx.x * kUniqueTile;
  const int64_t pos0 = tile0 + (int64_t)tid * kPerLane;
  const int64_t out0 = tile_offs[blockIdx.x];
  // (the plan masked the bits of positions past the end)
  const uint32_t bits = pos0 < n ? head_bits[pos0 / kPerLane] : 0u;
  int prefix, total;
  wave_rank(bits, lane, prefix, total);
  if (lane == 0) wtot[wave] = total;
  __syncthreads();
  int wbase = 0, count = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    if (i < wave) wbase += wtot[i];
    count += wtot[i];
  }
  int r = wbase + prefix;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j)
    if ((bits >> j) & 1u) heads[r++] = (uint16_t)(tid * kPerLane + j);
  __syncthreads();
  // count <= rows of the tile, so tile0 + heads[i] < n
  for (int i = tid; i < count; i += kUT) {
    const int64_t p = tile0 + heads[i];
    kept[out0 + i] = perm != nullptr ? perm[p] : p;
  }
}

int unique_tile_rows() { return kUniqueTile; }

static int64_t unique_tiles(int64_t n) { return (n + kUniqueTile - 1) / kUniqueTile; }

// workspace: int64 total | int64 offs[ntiles] | int32 counts[ntiles, padded to even] | head bits [ceil(n / 8)]
size_t unique_workspace_bytes(int64_t n) {
  const int64_t t = unique_tiles(n);
  return static_cast<size_t>(8 + 8 * t + 4 * (t + (t & 1)) + (n + 7) / 8);
}

int64_t unique_plan(const int64_t* words, int W, int64_t n, const int64_t* perm, void* ws, size_t ws_size,
                    hipStream_t s) {
  if (n <= 0) return 0;
  TFA_CHECK(W >= 1 && W <= kMaxSortKeys, "unique: 1..", kMaxSortKeys, " words per row, got ", W);
  const int64_t ntiles = unique_tiles(n);
  TFA_CHECK(ntiles < (int64_t(1) << 31), "unique: more than 2^31 tiles in one block of rows");
  TFA_CHECK(ws_size >= unique_workspace_bytes(n), "unique: workspace too small");
  int64_t* total = static_cast<int64_t*>(ws);
  int64_t* offs = total + 1;
  int32_t* counts = reinterpret_cast<int32_t*>(offs + ntiles);
  uint8_t* bits = reinterpret_cast<uint8_t*>(counts + ntiles + (ntiles & 1));
  hipLaunchKernelGGL(unique_plan_kernel, dim3((unsigned)ntiles), dim3(kUT), 0, s, words, W, n, perm, bits, counts);
  TFA_LAUNCH_CHECK("unique_plan_kernel");
  compact_scan_counts(counts, ntiles, offs, total, s);
  int64_t got = 0;
  TFA_CHECK(hipMemcpyAsync(&got, total, sizeof(got), hipMemcpyDeviceToHost, s) == hipSuccess,
            "unique: D2H of the head count failed");
  TFA_CHECK(hipStreamSynchronize(s) == hipSuccess, "unique: sync failed");
  TFA_CHECK(got >= 1 && got <= n, "unique: head count ", got, " out of range for ", n, " rows");
  return got;
}

void unique_write(const int64_t* perm, int64_t n, int64_t total, const void* ws, int64_t* kept, hipStream_t s) {
  if (n <= 0 || total <= 0) return;
  const int64_t ntiles = unique_tiles(n);
  const int64_t* offs = static_cast<const int64_t*>(ws) + 1;
  const int32_t* counts = reinterpret_cast<const int32_t*>(offs + ntiles);
  const uint8_t* bits = reinterpret_cast<const uint8_t*>(counts + ntiles + (ntiles & 1));
  hipLaunchKernelGGL(unique_write_kernel, dim3((unsigned)ntiles), dim3(kUT), 0, s, bits, n, perm, offs, kept);
  TFA_LAUNCH_CHECK("unique_write_kernel");
}

}  // namespace k
}  // namespace tfa
