// Equi-join probe and expansion for DataFrame.join (broadcast join).
//
// Both sides' keys arrive as the order-preserving 64-bit words of sort_encode
// (kernels.h: every NaN one word, -0.0 the word of 0.0), word-major. The build
// (right) side is sorted once with sort_argsort (stable: equal tuples keep
// right row order) and its words are gathered into that order (gather_words),
// so the probe reads them without the permutation's indirection.
//
//   probe   one thread per left row: the first sorted right position whose
//           tuple is not below the row's (lexicographic, unsigned) and the
//           number of equal tuples after it. The upper end is found by
//           galloping from the lower one (1, 2, 4, ... positions) and a binary
//           search inside the last step: a unique build key costs two probes,
//           a run of c equal keys about 2 log2(c). The row's own tuple lives
//           in registers (the kernel is compiled per word count);
//   scan    exclusive 64-bit scan of the counts into offs[n + 1]: per-tile
//           sums, one block over the tile sums, per-tile rescan;
//   expand  a block owns a tile of consecutive OUTPUT rows. Two lanes find the
//           left rows of the tile's first and last output row; when that range
//           is short its offsets are staged in LDS, else every lane searches
//           offs in global memory (a long run of left rows without a match
//           makes the range arbitrarily long). Output row j of left row i is
//           right row perm[lo[i] + (j - offs[i])]. Lanes next to each other
//           hold neighbouring output rows: a hot key fills whole tiles with
//           coalesced reads of perm and never serialises a wave.
//
// Row counts, positions and offsets are 64-bit.
#include <algorithm>

#include "column_types.h"
#include "hip_common.h"

namespace tfa {
namespace k {

namespace {

constexpr int kJT = 256;                         // threads per block of every kernel here
constexpr int kRowsPerLane = 8;
constexpr int kJoinTile = kJT * kRowsPerLane;    // output rows per expand block, rows per scan tile
constexpr int kStage = kJoinTile;                // left-row offsets an expand block stages in LDS at most
constexpr int kTopT = 1024;                      // threads of the scan over the tile sums

// tuple at column `pos` of words [W][m] compared with key: -1 below, 0 equal, 1 above
template <int W>
__device__ __forceinline__ int cmp_tuple(const uint64_t* __restrict__ words, int64_t m, int64_t pos,
                                         const uint64_t (&key)[W]) {
  int r = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    if (r == 0) {
      const uint64_t a = words[(int64_t)w * m + pos];
      r = a < key[w] ? -1 : (a > key[w] ? 1 : 0);
    }
  }
  return r;
}

}  // namespace

// mask_mode 0: no mask; 1: mask[i] = (cnt[i] != 0); 2: mask[i] = (cnt[i] == 0)
template <int W>
__global__ __launch_bounds__(kJT) void join_probe_kernel(const uint64_t* __restrict__ left, int64_t n,
                                                         const uint64_t* __restrict__ right, int64_t m,
                                                         int64_t* __restrict__ lo_out, int64_t* __restrict__ cnt_out,
                                                         uint8_t* __restrict__ mask, int mask_mode) {
  const int64_t i = (int64_t)blockIdx.x * kJT + threadIdx.x;
  if (i >= n) return;
  uint64_t key[W];
#pragma unroll
  for (int w = 0; w < W; ++w) key[w] = left[(int64_t)w * n + i];
  int64_t lo = 0, hi = m;
  while (lo < hi) {  // first position whose tuple is >= key
    const int64_t mid = lo + (hi - lo) / 2;
    if (cmp_tuple<W>(right, m, mid, key) < 0) lo = mid + 1;
    else hi = mid;
  }
  // first position in [lo, m) whose tuple is > key: gallop, then bisect
  int64_t a = lo, step = 1;  // every position in [lo, a) holds key
  int64_t b = m;             // position b holds a larger tuple (or b == m)
  while (a < m) {
    const int64_t p = a + step - 1 < m - 1 ? a + step - 1 : m - 1;
    if (cmp_tuple<W>(right, m, p, key) > 0) {
      b = p;
      break;
    }
    a = p + 1;
    step <<= 1;
  }
  while (a < b) {
    const int64_t mid = a + (b - a) / 2;
    if (cmp_tuple<W>(right, m, mid, key) > 0) b = mid;
    else a = mid + 1;
  }
  const int64_t cnt = a - lo;
  lo_out[i] = lo;
  cnt_out[i] = cnt;
  if (mask_mode != 0) mask[i] = (uint8_t)((cnt != 0) == (mask_mode == 1));
}

// out[w][j] = words[w][perm[j]] (blockIdx.y = w)
__global__ __launch_bounds__(kJT) void join_gather_words_kernel(const uint64_t* __restrict__ words,
                                                                const int64_t* __restrict__ perm, int64_t m,
                                                                uint64_t* __restrict__ out) {
  const uint64_t* __restrict__ src = words + (int64_t)blockIdx.y * m;
  uint64_t* __restrict__ dst = out + (int64_t)blockIdx.y * m;
  const int64_t step = (int64_t)gridDim.x * kJT;
  for (int64_t j = (int64_t)blockIdx.x * kJT + threadIdx.x; j < m; j += step) {
    const int64_t r = perm[j];
    dst[j] = src[(uint64_t)r < (uint64_t)m ? r : 0];  // never read outside the words
  }
}

// sums[t] = sum of cnt over tile t
__global__ __launch_bounds__(kJT) void join_tile_sum_kernel(const int64_t* __restrict__ cnt, int64_t n,
                                                            int64_t* __restrict__ sums) {
  __shared__ int64_t part[kJT / kWave];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kJoinTile;
  int64_t s = 0;
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    const int64_t i = row0 + j * kJT + tid;
    if (i < n) s += cnt[i];
  }
  s = wave_sum(s);
  if ((tid & (kWave - 1)) == 0) part[tid / kWave] = s;
  __syncthreads();
  if (tid == 0) {
    int64_t t = 0;
#pragma unroll
    for (int w = 0; w < kJT / kWave; ++w) t += part[w];
    sums[blockIdx.x] = t;
  }
}

// exclusive scan of the tile sums in place (one block); *total = their sum
__global__ __launch_bounds__(kTopT) void join_top_scan_kernel(int64_t* __restrict__ sums, int64_t ntiles,
                                                              int64_t* __restrict__ total) {
  __shared__ int64_t wsum[kTopT / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t per = (ntiles + kTopT - 1) / kTopT;
  const int64_t a = (int64_t)tid * per < ntiles ? (int64_t)tid * per : ntiles;
  const int64_t b = a + per < ntiles ? a + per : ntiles;
  int64_t s = 0;
  for (int64_t i = a; i < b; ++i) s += sums[i];
  int64_t inc = s;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int64_t u = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += u;
  }
  if (lane == kWave - 1) wsum[wave] = inc;
  __syncthreads();
  int64_t base = 0, tot = 0;
  for (int w = 0; w < kTopT / kWave; ++w) {
    if (w < wave) base += wsum[w];
    tot += wsum[w];
  }
  int64_t run = base + inc - s;
  for (int64_t i = a; i < b; ++i) {
    const int64_t c = sums[i];
    sums[i] = run;
    run += c;
  }
  if (tid == 0) *total = tot;
}

// offs[i] = tile_offs[tile] + sum of cnt over the tile's rows before i; a lane
// holds kRowsPerLane consecutive rows
__global__ __launch_bounds__(kJT) void join_tile_scan_kernel(const int64_t* __restrict__ cnt, int64_t n,
                                                             const int64_t* __restrict__ tile_offs,
                                                             int64_t* __restrict__ offs) {
  __shared__ int64_t wsum[kJT / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kJoinTile + (int64_t)tid * kRowsPerLane;
  int64_t c[kRowsPerLane];
  int64_t s = 0;
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    c[j] = row0 + j < n ? cnt[row0 + j] : 0;
    s += c[j];
  }
  int64_t inc = s;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int64_t u = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += u;
  }
  if (lane == kWave - 1) wsum[wave] = inc;
  __syncthreads();
  int64_t run = tile_offs[blockIdx.x] + inc - s;
#pragma unroll
  for (int w = 0; w < kJT / kWave; ++w)
    if (w < wave) run += wsum[w];
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    if (row0 + j < n) offs[row0 + j] = run;
    run += c[j];
  }
}

// block b: output rows [b * kJoinTile, min(total, (b + 1) * kJoinTile)).
// offs [n + 1] with offs[n] == total; lo [n]; perm [m]
__global__ __launch_bounds__(kJT) void join_expand_kernel(const int64_t* __restrict__ offs,
                                                          const int64_t* __restrict__ lo,
                                                          const int64_t* __restrict__ perm, int64_t n, int64_t m,
                                                          int64_t total, int64_t* __restrict__ left_idx,
                                                          int64_t* __restrict__ right_idx) {
  __shared__ int64_t staged[kStage];
  __shared__ int64_t range[2];
  const int tid = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * kJoinTile;
  const int64_t j1 = j0 + kJoinTile < total ? j0 + kJoinTile : total;  // (j0 < total: the host sizes the grid)
  // the left rows of output rows j0 and j1 - 1: offs[0] == 0 <= j and
  // offs[n] == total > j, so the answer lies in [0, n - 1]
  if (tid < 2) range[tid] = last_not_above(offs, 0, 0, n - 1, tid == 0 ? j0 : j1 - 1);
  __syncthreads();
  const int64_t ia = range[0], ib = range[1];
  const bool in_lds = ib - ia + 1 <= kStage;  // (the same for the whole block)
  if (in_lds) {
    for (int64_t i = ia + tid; i <= ib; i += kJT) staged[i - ia] = offs[i];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kRowsPerLane; ++k) {
    const int64_t j = j0 + k * kJT + tid;
    if (j >= j1) break;
    int64_t i, first;
    if (in_lds) {
      i = last_not_above(staged, ia, ia, ib, j);
      first = staged[i - ia];
    } else {
      i = last_not_above(offs, 0, ia, ib, j);
      first = offs[i];
    }
    int64_t pos = lo[i] + (j - first);
    pos = pos < 0 ? 0 : (pos < m ? pos : m - 1);  // never read outside perm
    left_idx[j] = i;
    right_idx[j] = perm[pos];
  }
}

// ------------------------------------------------------------------ host API
int join_tile_rows() { return kJoinTile; }

void join_probe(const int64_t* left, int W, int64_t n, const int64_t* right_sorted, int64_t m, int64_t* lo,
                int64_t* cnt, uint8_t* mask, int mask_mode, hipStream_t s) {
  TFA_CHECK(W >= 1 && W <= kMaxSortKeys, "join_probe: 1..", kMaxSortKeys, " words per row, got ", W);
  TFA_CHECK(n >= 0 && m >= 0, "join_probe: negative row count");
  TFA_CHECK(mask_mode >= 0 && mask_mode <= 2, "join_probe: mask mode 0, 1 or 2 expected");
  if (n == 0) return;
  TFA_CHECK(left != nullptr && lo != nullptr && cnt != nullptr, "join_probe: null buffer");
  TFA_CHECK(m == 0 || right_sorted != nullptr, "join_probe: null build words");
  TFA_CHECK(mask_mode == 0 || mask != nullptr, "join_probe: null mask buffer");
  const int64_t blocks = (n + kJT - 1) / kJT;
  TFA_CHECK(blocks < (int64_t(1) << 31), "join_probe: too many rows");
  const uint64_t* l = reinterpret_cast<const uint64_t*>(left);
  const uint64_t* r = reinterpret_cast<const uint64_t*>(right_sorted);
#define TFA_JOIN_PROBE(w)                                                                                        \
  case w:                                                                                                        \
    hipLaunchKernelGGL((join_probe_kernel<w>), dim3((unsigned)blocks), dim3(kJT), 0, s, l, n, r, m, lo, cnt, mask, \
                       mask_mode);                                                                               \
    break;
  switch (W) {
    TFA_JOIN_PROBE(1)
    TFA_JOIN_PROBE(2)
    TFA_JOIN_PROBE(3)
    TFA_JOIN_PROBE(4)
    TFA_JOIN_PROBE(5)
    TFA_JOIN_PROBE(6)
    TFA_JOIN_PROBE(7)
    default:
      TFA_JOIN_PROBE(8)
  }
#undef TFA_JOIN_PROBE
  TFA_LAUNCH_CHECK("join_probe_kernel");
}

void join_gather_words(const int64_t* words, int W, int64_t m, const int64_t* perm, int64_t* out, hipStream_t s) {
  TFA_CHECK(W >= 1 && W <= kMaxSortKeys, "join_gather_words: 1..", kMaxSortKeys, " words per row, got ", W);
  if (m <= 0) return;
  TFA_CHECK(words != nullptr && perm != nullptr && out != nullptr && words != out, "join_gather_words: bad buffer");
  hipLaunchKernelGGL(join_gather_words_kernel, dim3(ew_grid(m, kJT), W), dim3(kJT), 0, s,
                     reinterpret_cast<const uint64_t*>(words), perm, m, reinterpret_cast<uint64_t*>(out));
  TFA_LAUNCH_CHECK("join_gather_words_kernel");
}

static int64_t join_tiles(int64_t n) { return (n + kJoinTile - 1) / kJoinTile; }

// workspace: int64 sums[tiles]
size_t join_scan_workspace_bytes(int64_t n) { return static_cast<size_t>(8 * std::max<int64_t>(join_tiles(n), 1)); }

int64_t join_scan(const int64_t* cnt, int64_t n, int64_t m, int64_t* offs, void* ws, size_t ws_size, hipStream_t s) {
  TFA_CHECK(n >= 0 && m >= 0, "join_scan: negative row count");
  TFA_CHECK(offs != nullptr && reinterpret_cast<uintptr_t>(offs) % 8 == 0, "join_scan: bad offsets buffer");
  if (n == 0) {
    TFA_CHECK(hipMemsetAsync(offs, 0, 8, s) == hipSuccess, "join_scan: memset failed");
    return 0;
  }
  const int64_t ntiles = join_tiles(n);
  TFA_CHECK(ntiles < (int64_t(1) << 31), "join_scan: too many rows");
  TFA_CHECK(cnt != nullptr && ws != nullptr && ws_size >= join_scan_workspace_bytes(n), "join_scan: bad buffer");
  int64_t* sums = static_cast<int64_t*>(ws);
  hipLaunchKernelGGL(join_tile_sum_kernel, dim3((unsigned)ntiles), dim3(kJT), 0, s, cnt, n, sums);
  TFA_LAUNCH_CHECK("join_tile_sum_kernel");
  hipLaunchKernelGGL(join_top_scan_kernel, dim3(1), dim3(kTopT), 0, s, sums, ntiles, offs + n);
  TFA_LAUNCH_CHECK("join_top_scan_kernel");
  hipLaunchKernelGGL(join_tile_scan_kernel, dim3((unsigned)ntiles), dim3(kJT), 0, s, cnt, n, sums, offs);
  TFA_LAUNCH_CHECK("join_tile_scan_kernel");
  int64_t total = 0;
  TFA_CHECK(hipMemcpyAsync(&total, offs + n, sizeof(total), hipMemcpyDeviceToHost, s) == hipSuccess,
            "join_scan: D2H of the match count failed");
  TFA_CHECK(hipStreamSynchronize(s) == hipSuccess, "join_scan: sync failed");
  // every count is at most m: anything else means the counts were not a probe's
  TFA_CHECK(total >= 0 && (m == 0 ? total == 0 : total / m <= n), "join_scan: match count ", total,
            " out of range for ", n, " x ", m, " rows");
  return total;
}

void join_expand(const int64_t* offs, const int64_t* lo, const int64_t* perm, int64_t n, int64_t m, int64_t total,
                 int64_t* left_idx, int64_t* right_idx, hipStream_t s) {
  TFA_CHECK(n >= 0 && m >= 0 && total >= 0, "join_expand: negative row count");
  if (total == 0) return;
  TFA_CHECK(n > 0 && m > 0, "join_expand: matches without rows");
  TFA_CHECK(offs != nullptr && lo != nullptr && perm != nullptr && left_idx != nullptr && right_idx != nullptr,
            "join_expand: null buffer");
  const int64_t blocks = (total + kJoinTile - 1) / kJoinTile;
  TFA_CHECK(blocks < (int64_t(1) << 31), "join_expand: too many output rows");
  hipLaunchKernelGGL(join_expand_kernel, dim3((unsigned)blocks), dim3(kJT), 0, s, offs, lo, perm, n, m, total,
                     left_idx, right_idx);
  TFA_LAUNCH_CHECK("join_expand_kernel");
}

}  // namespace k
}  // namespace tfa
