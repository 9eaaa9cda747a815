// Stable stream compaction of whole rows by a byte mask (DataFrame.filter).
//
// A partition's dense columns ([n, row_bytes[c]] each, up to kMaxPackCols of
// them) keep the rows whose mask byte is non-zero, in order, in about one pass
// over the data and without a per-row position array in HBM:
//
//   plan    one block per tile of kCompactTile rows reads the tile's mask with
//           8-byte loads (8 rows per lane), counts the kept rows with 64-bit
//           ballots and writes ONE count per tile; a single-block scan turns
//           the tile counts into 64-bit output offsets and the total, which
//           the host reads with one stream synchronisation (to size the
//           outputs exactly);
//   gather  each block recomputes its tile's in-tile ranks (ballots, lane
//           prefix count, per-wave prefix in LDS), lists the kept rows of the
//           tile in LDS (2 bytes each) and copies, column after column, those
//           rows into [tile_offset, tile_offset + count) of the output. That
//           range is contiguous, so lanes walk the OUTPUT linearly and look
//           the source row up in the LDS list: stores are fully coalesced,
//           loads are row-granular. Accesses are 16 bytes when the row size
//           and both bases allow it, 4 bytes when the row size is a multiple
//           of 4, single bytes otherwise (decided per column on the host).
//           Several neighbouring blocks share a tile's output when rows are
//           wide (each recomputes the ranks: 2 KiB of mask).
//
// Row counts, row indices and byte offsets are 64-bit (a 2.5 M x 2048 B
// partition is past 4 GiB); only offsets INSIDE one tile's copy are 32-bit
// where the path bounds them. Copies are bitwise.
#include <algorithm>

#include "hip_common.h"

namespace tfa {
namespace k {

namespace {

constexpr int kCT = 256;                             // threads per plan / gather block
constexpr int kMaskPerLane = 8;                      // mask bytes (rows) per lane
constexpr int kCompactTile = kCT * kMaskPerLane;     // rows per tile
constexpr int kScanT = 1024;                         // threads of the tile-count scan
constexpr int kSmallRowUnits = 256;                  // rows of up to this many access units: linear walk
constexpr int64_t kSliceBytes = 64 << 10;            // kept bytes per gather block to aim for
constexpr int kMaxSlices = 64;
constexpr int kUnroll = 4;                           // copies in flight per lane

static_assert(kCompactTile <= 65536, "in-tile row indices are kept as uint16");

// 16-byte access unit: a native vector (loads of the uint4 struct are copied as
// aggregates, which ties every load to its store and leaves one in flight)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// bit j = row row0 + j is kept (non-zero mask byte); rows >= n are dropped
__device__ __forceinline__ uint32_t lane_keep_bits(const uint8_t* __restrict__ mask, int64_t n, int64_t row0,
                                                   bool aligned8) {
  uint32_t bits = 0;
  if (aligned8 && row0 + kMaskPerLane <= n) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(mask + row0);
#pragma unroll
    for (int j = 0; j < kMaskPerLane; ++j) bits |= ((w >> (8 * j)) & 0xffull) ? (1u << j) : 0u;
  } else {
#pragma unroll
    for (int j = 0; j < kMaskPerLane; ++j)
      if (row0 + j < n && mask[row0 + j]) bits |= 1u << j;
  }
  return bits;
}

// kept rows of the lower lanes of this wave (prefix) and of the whole wave
// (total); a lane's rows are consecutive, so lane order is row order
__device__ __forceinline__ void wave_rank(uint32_t bits, int lane, int& prefix, int& total) {
  const unsigned long long below = (1ull << lane) - 1ull;
  prefix = 0;
  total = 0;
#pragma unroll
  for (int j = 0; j < kMaskPerLane; ++j) {
    const unsigned long long b = __ballot((bits >> j) & 1u);
    prefix += __popcll(b & below);
    total += __popcll(b);
  }
}

}  // namespace

__global__ __launch_bounds__(kCT) void compact_plan_kernel(const uint8_t* __restrict__ mask, int64_t n,
                                                           int32_t* __restrict__ tile_counts) {
  __shared__ int wtot[kCT / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kCompactTile + (int64_t)tid * kMaskPerLane;
  const bool aligned8 = (reinterpret_cast<uintptr_t>(mask) & 7) == 0;
  const uint32_t bits = lane_keep_bits(mask, n, row0, aligned8);
  int prefix, total;
  wave_rank(bits, lane, prefix, total);
  if (lane == 0) wtot[wave] = total;
  __syncthreads();
  if (tid == 0) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kCT / kWave; ++w) c += wtot[w];
    tile_counts[blockIdx.x] = c;
  }
}

// exclusive scan of the tile counts (one block): offs[t] = rows kept before
// tile t, *total = rows kept
__global__ __launch_bounds__(kScanT) void compact_scan_kernel(const int32_t* __restrict__ counts, int64_t ntiles,
                                                              int64_t* __restrict__ offs,
                                                              int64_t* __restrict__ total) {
  __shared__ int64_t wsum[kScanT / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t per = (ntiles + kScanT - 1) / kScanT;
  const int64_t a = (int64_t)tid * per < ntiles ? (int64_t)tid * per : ntiles;
  const int64_t b = a + per < ntiles ? a + per : ntiles;
  int64_t s = 0;
  for (int64_t i = a; i < b; ++i) s += counts[i];
  int64_t inc = s;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int64_t u = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += u;
  }
  if (lane == kWave - 1) wsum[wave] = inc;
  __syncthreads();
  int64_t base = 0, tot = 0;
  for (int w = 0; w < kScanT / kWave; ++w) {
    if (w < wave) base += wsum[w];
    tot += wsum[w];
  }
  int64_t run = base + inc - s;
  for (int64_t i = a; i < b; ++i) {
    offs[i] = run;
    run += counts[i];
  }
  if (tid == 0) *total = tot;
}

namespace {

// rows kept[0 .. count) of the tile at `sp` -> rows 0 .. count of `dp`, in
// units of V (upr units per row). The blocks that share a tile take its block
// passes (wide rows: its rows) in turn, slice, slice + nslices, ...: blocks
// in flight together then move through the same few MiB of the source and of
// the output, not each through a range of its own.
template <typename V>
__device__ __forceinline__ void copy_kept_rows(const char* __restrict__ sp, char* __restrict__ dp,
                                               const uint16_t* kept, int count, int64_t upr, int slice,
                                               int nslices, int tid) {
  const V* __restrict__ s = reinterpret_cast<const V*>(sp);
  V* __restrict__ d = reinterpret_cast<V*>(dp);
  if (upr <= kSmallRowUnits) {
    // the output units of the tile, linearly: unit u = (row r, unit k of the
    // row); kUnroll loads in flight per lane, then their stores
    const uint32_t w = (uint32_t)upr;
    const uint32_t units = (uint32_t)count * w;  // <= kCompactTile * kSmallRowUnits
    const uint32_t step_r = kCT / w, step_k = kCT % w;
    constexpr uint32_t kPass = kCT * kUnroll;
    for (uint32_t base = (uint32_t)slice * kPass; base < units; base += (uint32_t)nslices * kPass) {
      uint32_t u = base + tid;
      uint32_t r = u / w, kk = u - r * w;
      if (base + kPass <= units) {  // a whole pass (the same for the block): no bounds inside
        V v[kUnroll];
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {
          v[j] = s[(uint32_t)kept[r] * w + kk];
          r += step_r;
          kk += step_k;
          if (kk >= w) {
            kk -= w;
            ++r;
          }
        }
        // (keeps the loads together ahead of the stores: scheduled one load,
        // one wait, one store at a time a lane has a single load in flight)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) d[u + j * kCT] = v[j];
      } else {
        for (; u < units; u += kCT) {
          d[u] = s[(uint32_t)kept[r] * w + kk];
          r += step_r;
          kk += step_k;
          if (kk >= w) {
            kk -= w;
            ++r;
          }
        }
      }
    }
  } else {
    // wide rows: row after row, the lanes side by side along the row
    for (int r = slice; r < count; r += nslices) {
      const V* __restrict__ sr = s + (int64_t)kept[r] * upr;
      V* __restrict__ dr = d + (int64_t)r * upr;
      int64_t kk = tid;
      for (; kk + (kUnroll - 1) * kCT < upr; kk += kUnroll * kCT) {
        V v[kUnroll];
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) v[j] = sr[kk + j * kCT];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) dr[kk + j * kCT] = v[j];
      }
      for (; kk < upr; kk += kCT) dr[kk] = sr[kk];
    }
  }
}

}  // namespace

// src.off[c] holds column c's access width in bytes (16, 4 or 1); dst.ptr[c]
// is the column's output
__global__ __launch_bounds__(kCT) void compact_gather_kernel(PackCols src, PackCols dst,
                                                             const uint8_t* __restrict__ mask, int64_t n,
                                                             const int64_t* __restrict__ tile_offs,
                                                             int64_t* __restrict__ index_out, int nslices) {
  __shared__ uint16_t kept[kCompactTile];
  __shared__ int wtot[kCT / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  // the slices of a tile are neighbouring blocks: the blocks in flight sweep
  // the source and the output in address order
  const uint32_t tile = blockIdx.x / (uint32_t)nslices;
  const int slice = (int)(blockIdx.x - tile * (uint32_t)nslices);
  const int64_t tile_row0 = (int64_t)tile * kCompactTile;
  const int64_t out0 = tile_offs[tile];  // (asked for early: the ranks do not wait for it)
  const bool aligned8 = (reinterpret_cast<uintptr_t>(mask) & 7) == 0;
  const uint32_t bits = lane_keep_bits(mask, n, tile_row0 + (int64_t)tid * kMaskPerLane, aligned8);
  int prefix, total;
  wave_rank(bits, lane, prefix, total);
  if (lane == 0) wtot[wave] = total;
  __syncthreads();
  int wbase = 0, count = 0;
#pragma unroll
  for (int w = 0; w < kCT / kWave; ++w) {
    if (w < wave) wbase += wtot[w];
    count += wtot[w];
  }
  if (count == 0) return;  // (the same for the whole block)
  int r = wbase + prefix;
#pragma unroll
  for (int j = 0; j < kMaskPerLane; ++j)
    if ((bits >> j) & 1u) kept[r++] = (uint16_t)(tid * kMaskPerLane + j);
  __syncthreads();
  if (index_out != nullptr && slice == 0)
    for (int i = tid; i < count; i += kCT) index_out[out0 + i] = tile_row0 + kept[i];
  for (int c = 0; c < src.n; ++c) {
    const int64_t rb = src.row_bytes[c];
    if (rb == 0) continue;  // cells without elements
    const char* sp = static_cast<const char*>(src.ptr[c]) + tile_row0 * rb;
    char* dp = static_cast<char*>(const_cast<void*>(dst.ptr[c])) + out0 * rb;
    const int64_t width = src.off[c];
    if (width == 16)
      copy_kept_rows<u32x4>(sp, dp, kept, count, rb / 16, slice, nslices, tid);
    else if (width == 4)
      copy_kept_rows<uint32_t>(sp, dp, kept, count, rb / 4, slice, nslices, tid);
    else
      copy_kept_rows<uint8_t>(sp, dp, kept, count, rb, slice, nslices, tid);
  }
}

int compact_tile_rows() { return kCompactTile; }

static int64_t compact_tiles(int64_t n) { return (n + kCompactTile - 1) / kCompactTile; }

// workspace: int64 total | int64 offs[ntiles] | int32 counts[ntiles]
size_t compact_workspace_bytes(int64_t n) {
  const int64_t t = compact_tiles(n);
  return static_cast<size_t>(8 + 8 * t + 4 * t);
}

void compact_scan_counts(const int32_t* counts, int64_t ntiles, int64_t* offs, int64_t* total, hipStream_t s) {
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kScanT), 0, s, counts, ntiles, offs, total);
  TFA_LAUNCH_CHECK("compact_scan_kernel");
}

int64_t compact_plan(const uint8_t* mask, int64_t n, void* ws, size_t ws_size, hipStream_t s) {
  if (n <= 0) return 0;
  const int64_t ntiles = compact_tiles(n);
  TFA_CHECK(ntiles < (int64_t(1) << 31), "compact: more than 2^31 tiles in one block of rows");
  TFA_CHECK(ws_size >= compact_workspace_bytes(n), "compact: workspace too small");
  int64_t* total = static_cast<int64_t*>(ws);
  int64_t* offs = total + 1;
  int32_t* counts = reinterpret_cast<int32_t*>(offs + ntiles);
  hipLaunchKernelGGL(compact_plan_kernel, dim3((unsigned)ntiles), dim3(kCT), 0, s, mask, n, counts);
  TFA_LAUNCH_CHECK("compact_plan_kernel");
  compact_scan_counts(counts, ntiles, offs, total, s);
  int64_t got = 0;
  TFA_CHECK(hipMemcpyAsync(&got, total, sizeof(got), hipMemcpyDeviceToHost, s) == hipSuccess,
            "compact: D2H of the kept count failed");
  TFA_CHECK(hipStreamSynchronize(s) == hipSuccess, "compact: sync failed");
  TFA_CHECK(got >= 0 && got <= n, "compact: kept count ", got, " out of range for ", n, " rows");
  return got;
}

void compact_gather(const PackCols& src0, const PackCols& dst, const uint8_t* mask, int64_t n, int64_t total,
                    const void* ws, int64_t* index, hipStream_t s) {
  TFA_CHECK(src0.n >= 0 && src0.n <= kMaxPackCols && dst.n == src0.n, "compact: 0..", kMaxPackCols, " columns");
  if (n <= 0 || total <= 0 || (src0.n == 0 && index == nullptr)) return;
  const int64_t ntiles = compact_tiles(n);
  PackCols src = src0;
  int64_t row_bytes = 0;
  for (int c = 0; c < src.n; ++c) {
    const int64_t rb = src.row_bytes[c];
    TFA_CHECK(rb >= 0, "compact: negative row size");
    const uintptr_t both = reinterpret_cast<uintptr_t>(src.ptr[c]) | reinterpret_cast<uintptr_t>(dst.ptr[c]);
    src.off[c] = (rb % 16 == 0 && (both & 15) == 0) ? 16 : (rb % 4 == 0 && (both & 3) == 0) ? 4 : 1;
    row_bytes += rb;
  }
  // a tile keeps total / ntiles rows on average: split its copy so that a
  // block moves about kSliceBytes
  const double avg = static_cast<double>(total) / static_cast<double>(ntiles) * static_cast<double>(row_bytes);
  const int slices = static_cast<int>(std::min<double>(kMaxSlices, std::max(1.0, avg / kSliceBytes + 0.5)));
  const int64_t* offs = static_cast<const int64_t*>(ws) + 1;
  TFA_CHECK(ntiles * slices < (int64_t(1) << 31), "compact: too many blocks");
  hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)(ntiles * slices)), dim3(kCT), 0, s, src, dst, mask, n,
                     offs, index, slices);
  TFA_LAUNCH_CHECK("compact_gather_kernel");
}

}  // namespace k
}  // namespace tfa
