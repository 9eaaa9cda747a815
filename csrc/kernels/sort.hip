// Row ordering for DataFrame.orderBy / sortWithinPartitions.
//
//   encode   every sort key -> one unsigned 64-bit word per row whose unsigned
//            order is the key's order (the table in kernels.h); all keys in one
//            launch, words stored word-major [W][n];
//   argsort  stable LSD radix sort over the words (last word first) on top of
//            radix.h. One reduction computes, per word, the OR over the rows of
//            word ^ word of row 0: only the 8-bit digits whose mask byte is
//            non-zero are sorted (an int32 key in [0, 1000) takes 2 passes, a
//            constant key none). The permutation travels as 32-bit row indices
//            and a word whose varying bits all lie in its low half as 32-bit
//            keys; the last kernel widens the permutation to int64;
//   permute  dst row j = src row perm[j] for up to kMaxPackCols columns in one
//            launch. A block owns a tile of consecutive OUTPUT rows (their
//            source rows staged in LDS) and walks, column after column, the
//            tile's output linearly in access units of 16, 8, 4 or 1 bytes: the
//            lanes next to each other cover one row with consecutive pieces, so
//            stores are fully coalesced and loads are coalesced inside a row
//            (random only from row to row, which narrow rows cannot avoid).
//            kUnroll independent loads are in flight per lane. take_rows is
//            the same kernel with a source row count of its own (any index
//            list: fewer or more output rows than source rows, repeats);
//   bounds   lower bounds of splitter tuples in the sorted order (one thread
//            per splitter, binary search through perm).
//
// Row counts and byte offsets are 64-bit; offsets inside one tile's output
// are 32-bit (the host bounds them).
#include <algorithm>

#include "hip_common.h"
#include "radix.h"
#include "sort_words.h"

namespace tfa {
namespace k {

namespace {

constexpr int kST = 256;            // threads per block of every kernel here
constexpr int kPermTile = 2048;     // most output rows per permute block
constexpr int64_t kPermTileBytes = 64 << 10;  // output bytes per permute block to aim for
constexpr int kUnroll = 4;          // loads in flight per lane

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// one key column: rows grid-stride; `flip` is the descending complement
template <typename T, typename F>
__device__ __forceinline__ void encode_column(const void* __restrict__ src, uint64_t* __restrict__ out, int64_t n,
                                              uint64_t flip, F f) {
  const T* __restrict__ p = static_cast<const T*>(src);
  const int64_t step = (int64_t)gridDim.x * kST;
  for (int64_t i = (int64_t)blockIdx.x * kST + threadIdx.x; i < n; i += step) out[i] = f(p[i]) ^ flip;
}

}  // namespace

__global__ __launch_bounds__(kST) void sort_encode_kernel(SortKeys keys, int64_t n, uint64_t* __restrict__ words) {
  for (int c = 0; c < keys.n; ++c) {
    const void* src = keys.ptr[c];
    uint64_t* out = words + (int64_t)c * n;
    const bool desc = keys.descending[c] != 0;
    switch (keys.dtype[c]) {  // (uniform: one scalar branch per column)
      case DType::F32:
        encode_column<uint32_t>(src, out, n, desc ? 0xffffffffull : 0ull, [](uint32_t b) { return encode_f32(b); });
        break;
      case DType::F64:
        encode_column<uint64_t>(src, out, n, desc ? ~0ull : 0ull, [](uint64_t b) { return encode_f64(b); });
        break;
      case DType::I64:
        encode_column<int64_t>(src, out, n, desc ? ~0ull : 0ull, [](int64_t v) { return encode_int(v); });
        break;
      case DType::I32:
        encode_column<int32_t>(src, out, n, desc ? ~0ull : 0ull, [](int32_t v) { return encode_int(v); });
        break;
      case DType::I16:
        encode_column<int16_t>(src, out, n, desc ? ~0ull : 0ull, [](int16_t v) { return encode_int(v); });
        break;
      case DType::I8:
        encode_column<int8_t>(src, out, n, desc ? ~0ull : 0ull, [](int8_t v) { return encode_int(v); });
        break;
      default:  // BOOL, U8: the value
        encode_column<uint8_t>(src, out, n, desc ? ~0ull : 0ull, [](uint8_t v) { return static_cast<uint64_t>(v); });
        break;
    }
  }
}

// masks[w] |= OR over rows of words[w][i] ^ words[w][0] (masks zeroed before)
__global__ __launch_bounds__(kST) void sort_digit_mask_kernel(const uint64_t* __restrict__ words, int64_t n,
                                                              unsigned long long* __restrict__ masks) {
  __shared__ unsigned long long part[kST / kWave];
  const uint64_t* __restrict__ w = words + (int64_t)blockIdx.y * n;
  const uint64_t first = w[0];
  uint64_t m = 0;
  const int64_t step = (int64_t)gridDim.x * kST;
  for (int64_t i = (int64_t)blockIdx.x * kST + threadIdx.x; i < n; i += step) m |= w[i] ^ first;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m |= __shfl_xor(m, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long b = 0;
#pragma unroll
    for (int i = 0; i < kST / kWave; ++i) b |= part[i];
    if (b) atomicOr(&masks[blockIdx.y], b);
  }
}

// keys[i] = word of row perm[i] (perm null: row i), as K
template <typename K>
__global__ __launch_bounds__(kST) void sort_gather_keys_kernel(const uint64_t* __restrict__ word,
                                                               const uint32_t* __restrict__ perm, int64_t n,
                                                               K* __restrict__ keys) {
  const int64_t step = (int64_t)gridDim.x * kST;
  for (int64_t i = (int64_t)blockIdx.x * kST + threadIdx.x; i < n; i += step)
    keys[i] = static_cast<K>(word[perm ? (int64_t)perm[i] : i]);
}

// out[i] = perm[i] (perm null: i)
__global__ __launch_bounds__(kST) void sort_widen_perm_kernel(const uint32_t* __restrict__ perm, int64_t n,
                                                              int64_t* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * kST;
  for (int64_t i = (int64_t)blockIdx.x * kST + threadIdx.x; i < n; i += step) out[i] = perm ? (int64_t)perm[i] : i;
}

namespace {

struct PermuteMeta {
  int width[kMaxPackCols];       // access unit in bytes: 16, 8, 4 or 1 (0: no bytes in the column's rows)
  FastDivU32 upr[kMaxPackCols];  // units per row
};

// units [0, units) of this tile's output for one column: unit u = (row u / upr
// of the tile, unit u % upr of the row)
template <typename V>
__device__ __forceinline__ void permute_tile(const char* __restrict__ sp, char* __restrict__ dp, const uint32_t* rows,
                                             uint32_t units, const FastDivU32& upr, int64_t row_bytes, int tid) {
  V* __restrict__ d = reinterpret_cast<V*>(dp);
  constexpr uint32_t kPass = kST * kUnroll;
  for (uint32_t base = 0; base < units; base += kPass) {
    V v[kUnroll] = {};
    if (base + kPass <= units) {  // a whole pass (the same for the block): no bounds inside
#pragma unroll
      for (int j = 0; j < kUnroll; ++j) {
        const uint32_t u = base + j * kST + tid;
        const uint32_t r = fdiv(u, upr), kk = u - r * upr.d;
        v[j] = *reinterpret_cast<const V*>(sp + (int64_t)rows[r] * row_bytes + (int64_t)kk * sizeof(V));
      }
      // (keeps the loads together ahead of the stores: kUnroll in flight per lane)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < kUnroll; ++j) d[base + j * kST + tid] = v[j];
    } else {  // the last, partial pass: the same shape, every access guarded
#pragma unroll
      for (int j = 0; j < kUnroll; ++j) {
        const uint32_t u = base + j * kST + tid;
        if (u < units) {
          const uint32_t r = fdiv(u, upr), kk = u - r * upr.d;
          v[j] = *reinterpret_cast<const V*>(sp + (int64_t)rows[r] * row_bytes + (int64_t)kk * sizeof(V));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < kUnroll; ++j) {
        const uint32_t u = base + j * kST + tid;
        if (u < units) d[u] = v[j];
      }
    }
  }
}

}  // namespace

// block b: output rows [b * tile, min(n, (b + 1) * tile)) of every column; the
// source columns hold n_src rows
__global__ __launch_bounds__(kST) void permute_rows_kernel(PackCols src, PackCols dst, PermuteMeta meta,
                                                           const int64_t* __restrict__ perm, int64_t n, int64_t n_src,
                                                           int tile) {
  __shared__ uint32_t rows[kPermTile];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * tile;
  const int count = (int)(n - row0 < tile ? n - row0 : tile);
  for (int i = tid; i < count; i += kST) {
    const int64_t p = perm[row0 + i];
    rows[i] = (uint64_t)p < (uint64_t)n_src ? (uint32_t)p : 0u;  // never read outside the column
  }
  __syncthreads();
  for (int c = 0; c < src.n; ++c) {
    const int width = meta.width[c];
    if (width == 0) continue;
    const int64_t rb = src.row_bytes[c];
    const char* sp = static_cast<const char*>(src.ptr[c]);
    char* dp = static_cast<char*>(const_cast<void*>(dst.ptr[c])) + row0 * rb;
    const FastDivU32 upr = meta.upr[c];
    const uint32_t units = (uint32_t)count * upr.d;
    if (width == 16)
      permute_tile<u32x4>(sp, dp, rows, units, upr, rb, tid);
    else if (width == 8)
      permute_tile<u32x2>(sp, dp, rows, units, upr, rb, tid);
    else if (width == 4)
      permute_tile<uint32_t>(sp, dp, rows, units, upr, rb, tid);
    else
      permute_tile<uint8_t>(sp, dp, rows, units, upr, rb, tid);
  }
}

// out[i] = first position of the sorted order whose tuple is >= splitter i
__global__ __launch_bounds__(kST) void sort_bounds_kernel(const uint64_t* __restrict__ words, int W, int64_t n,
                                                          const int64_t* __restrict__ perm,
                                                          const uint64_t* __restrict__ splitters, int64_t S,
                                                          int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kST + threadIdx.x;
  if (i >= S) return;
  const uint64_t* __restrict__ sp = splitters + i * W;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    int64_t r = perm[mid];
    r = (uint64_t)r < (uint64_t)n ? r : 0;
    bool less = false;
    for (int w = 0; w < W; ++w) {
      const uint64_t a = words[(int64_t)w * n + r], b = sp[w];
      if (a != b) {
        less = a < b;
        break;
      }
    }
    if (less) lo = mid + 1;
    else hi = mid;
  }
  out[i] = lo;
}

// ------------------------------------------------------------------ host API
int sort_tile_rows() { return radix::kTile; }

void sort_encode(const SortKeys& keys, int64_t n, int64_t* words, hipStream_t s) {
  TFA_CHECK(keys.n >= 1 && keys.n <= kMaxSortKeys, "sort_encode: 1..", kMaxSortKeys, " keys, got ", keys.n);
  TFA_CHECK(n >= 0, "sort_encode: negative row count");
  for (int c = 0; c < keys.n; ++c) {
    const DType d = keys.dtype[c];
    TFA_CHECK(d == DType::F32 || d == DType::F64 || d == DType::I64 || d == DType::I32 || d == DType::I16 ||
                  d == DType::I8 || d == DType::U8 || d == DType::BOOL,
              "sort_encode: key ", c, " has a dtype that is not supported as a sort key");
    TFA_CHECK(n == 0 || keys.ptr[c] != nullptr, "sort_encode: key ", c, " has no data");
    TFA_CHECK(reinterpret_cast<uintptr_t>(keys.ptr[c]) % static_cast<uintptr_t>(dtype_size(d)) == 0,
              "sort_encode: key ", c, " is not aligned to its element size");
  }
  if (n == 0) return;
  TFA_CHECK(words != nullptr && reinterpret_cast<uintptr_t>(words) % 8 == 0, "sort_encode: unaligned output");
  hipLaunchKernelGGL(sort_encode_kernel, dim3(ew_grid(n, kST)), dim3(kST), 0, s, keys, n,
                     reinterpret_cast<uint64_t*>(words));
  TFA_LAUNCH_CHECK("sort_encode_kernel");
}

namespace {
size_t masks_bytes(int W) { return radix::align_up(static_cast<size_t>(W) * 8); }
}  // namespace

// workspace: masks [W] | perm a, perm b (uint32 [n]) | keys in, keys out (uint64 [n]) | radix workspace
size_t sort_argsort_workspace_bytes(int W, int64_t n) {
  const size_t rows = static_cast<size_t>(std::max<int64_t>(n, 0));
  return masks_bytes(W) + 2 * radix::align_up(rows * 4) + 2 * radix::align_up(rows * 8) +
         radix::sort_ws_bytes<uint64_t, uint32_t>(n);
}

int sort_argsort(const int64_t* words, int W, int64_t n, int64_t* perm, void* ws, size_t ws_size, hipStream_t s) {
  TFA_CHECK(W >= 1 && W <= kMaxSortKeys, "sort_argsort: 1..", kMaxSortKeys, " words per row, got ", W);
  TFA_CHECK(n >= 0 && n < (int64_t(1) << 32) - 1, "sort_argsort: 0..2^32-2 rows, got ", n);
  if (n == 0) return 0;
  TFA_CHECK(words != nullptr && perm != nullptr && ws != nullptr, "sort_argsort: null buffer");
  TFA_CHECK(reinterpret_cast<uintptr_t>(words) % 8 == 0 && reinterpret_cast<uintptr_t>(perm) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(ws) % 8 == 0, "sort_argsort: unaligned buffer");
  TFA_CHECK(ws_size >= sort_argsort_workspace_bytes(W, n), "sort_argsort: workspace too small");
  const uint64_t* wd = reinterpret_cast<const uint64_t*>(words);
  char* p = static_cast<char*>(ws);
  unsigned long long* masks = reinterpret_cast<unsigned long long*>(p);
  p += masks_bytes(W);
  uint32_t* pa = reinterpret_cast<uint32_t*>(p);
  p += radix::align_up(n * 4);
  uint32_t* pb = reinterpret_cast<uint32_t*>(p);
  p += radix::align_up(n * 4);
  uint64_t* kin = reinterpret_cast<uint64_t*>(p);
  p += radix::align_up(n * 8);
  uint64_t* kout = reinterpret_cast<uint64_t*>(p);
  p += radix::align_up(n * 8);
  const size_t radix_ws = radix::sort_ws_bytes<uint64_t, uint32_t>(n);

  TFA_CHECK(hipMemsetAsync(masks, 0, static_cast<size_t>(W) * 8, s) == hipSuccess, "sort_argsort: memset failed");
  hipLaunchKernelGGL(sort_digit_mask_kernel, dim3(ew_grid(n, kST), W), dim3(kST), 0, s, wd, n, masks);
  TFA_LAUNCH_CHECK("sort_digit_mask_kernel");
  unsigned long long hm[kMaxSortKeys];
  TFA_CHECK(hipMemcpyAsync(hm, masks, static_cast<size_t>(W) * 8, hipMemcpyDeviceToHost, s) == hipSuccess,
            "sort_argsort: D2H of the digit masks failed");
  TFA_CHECK(hipStreamSynchronize(s) == hipSuccess, "sort_argsort: sync failed");

  const int grid = ew_grid(n, kST);
  const uint32_t* cur = nullptr;  // the order so far (null: the input order)
  int passes = 0;
  for (int w = W - 1; w >= 0; --w) {
    int shifts[8], ns = 0;
    for (int d = 0; d < 8; ++d)
      if ((hm[w] >> (8 * d)) & 0xffull) shifts[ns++] = 8 * d;
    if (ns == 0) continue;  // the word is the same in every row
    uint32_t* nxt = cur == pa ? pb : pa;
    const uint64_t* word = wd + (int64_t)w * n;
    if ((hm[w] >> 32) == 0) {  // the varying bits fit 32-bit keys
      uint32_t* k32 = reinterpret_cast<uint32_t*>(kin);
      hipLaunchKernelGGL((sort_gather_keys_kernel<uint32_t>), dim3(grid), dim3(kST), 0, s, word, cur, n, k32);
      TFA_LAUNCH_CHECK("sort_gather_keys_kernel");
      radix::sort_pairs_digits<uint32_t, uint32_t>(k32, cur, reinterpret_cast<uint32_t*>(kout), nxt, n, shifts, ns, p,
                                                   radix_ws, s);
    } else {
      const uint64_t* keys = word;
      if (cur != nullptr) {
        hipLaunchKernelGGL((sort_gather_keys_kernel<uint64_t>), dim3(grid), dim3(kST), 0, s, word, cur, n, kin);
        TFA_LAUNCH_CHECK("sort_gather_keys_kernel");
        keys = kin;
      }
      radix::sort_pairs_digits<uint64_t, uint32_t>(keys, cur, kout, nxt, n, shifts, ns, p, radix_ws, s);
    }
    TFA_LAUNCH_CHECK("radix sort");
    cur = nxt;
    passes += ns;
  }
  hipLaunchKernelGGL(sort_widen_perm_kernel, dim3(grid), dim3(kST), 0, s, cur, n, perm);
  TFA_LAUNCH_CHECK("sort_widen_perm_kernel");
  return passes;
}

namespace {

// dst row j = src row idx[j] for j < n; the source columns hold n_src rows
void gather_rows_impl(const char* what, const PackCols& src, const PackCols& dst, const int64_t* perm, int64_t n,
                      int64_t n_src, hipStream_t s) {
  TFA_CHECK(src.n >= 1 && src.n <= kMaxPackCols && dst.n == src.n, what, ": 1..", kMaxPackCols, " columns");
  TFA_CHECK(n >= 0 && n < (int64_t(1) << 32) - 1, what, ": 0..2^32-2 rows, got ", n);
  TFA_CHECK(n_src >= 0 && n_src < (int64_t(1) << 32) - 1, what, ": 0..2^32-2 source rows, got ", n_src);
  if (n == 0) return;
  TFA_CHECK(n_src > 0, what, ": rows asked of columns without rows");
  TFA_CHECK(perm != nullptr && reinterpret_cast<uintptr_t>(perm) % 8 == 0, what, ": bad index buffer");
  int64_t total = 0, widest = 0;
  for (int c = 0; c < src.n; ++c) {
    const int64_t rb = src.row_bytes[c];
    TFA_CHECK(rb >= 0 && rb == dst.row_bytes[c], what, ": column ", c, " row sizes differ or are negative");
    TFA_CHECK(rb == 0 || (src.ptr[c] != nullptr && dst.ptr[c] != nullptr), what, ": column ", c, " has no data");
    TFA_CHECK(rb == 0 || src.ptr[c] != dst.ptr[c], what, ": column ", c, " cannot be gathered in place");
    total += rb;
    widest = std::max(widest, rb);
  }
  if (total == 0) return;
  // rows per block: about kPermTileBytes of output, and 32-bit offsets inside it
  TFA_CHECK(widest < (int64_t(1) << 31), what, ": rows of 2 GiB or more");
  int64_t tile = std::max<int64_t>(1, std::min<int64_t>(kPermTile, kPermTileBytes / total));
  tile = std::min(tile, std::max<int64_t>(1, ((int64_t(1) << 31) - 1) / widest));
  const int64_t blocks = (n + tile - 1) / tile;
  TFA_CHECK(blocks < (int64_t(1) << 31), what, ": too many blocks");
  PermuteMeta meta;
  for (int c = 0; c < kMaxPackCols; ++c) {
    meta.width[c] = 0;
    meta.upr[c] = make_fastdiv(1);
  }
  for (int c = 0; c < src.n; ++c) {
    const int64_t rb = src.row_bytes[c];
    if (rb == 0) continue;
    const uintptr_t both = reinterpret_cast<uintptr_t>(src.ptr[c]) | reinterpret_cast<uintptr_t>(dst.ptr[c]);
    const int width = (rb % 16 == 0 && (both & 15) == 0) ? 16
                      : (rb % 8 == 0 && (both & 7) == 0) ? 8
                      : (rb % 4 == 0 && (both & 3) == 0) ? 4 : 1;
    meta.width[c] = width;
    meta.upr[c] = make_fastdiv(static_cast<uint32_t>(rb / width));
  }
  hipLaunchKernelGGL(permute_rows_kernel, dim3((unsigned)blocks), dim3(kST), 0, s, src, dst, meta, perm, n, n_src,
                     (int)tile);
  TFA_LAUNCH_CHECK("permute_rows_kernel");
}

}  // namespace

void permute_rows(const PackCols& src, const PackCols& dst, const int64_t* perm, int64_t n, hipStream_t s) {
  gather_rows_impl("permute_rows", src, dst, perm, n, n, s);
}

void take_rows(const PackCols& src, const PackCols& dst, const int64_t* idx, int64_t n_out, int64_t n_src,
               hipStream_t s) {
  gather_rows_impl("take_rows", src, dst, idx, n_out, n_src, s);
}

void sort_bounds(const int64_t* words, int W, int64_t n, const int64_t* perm, const int64_t* splitters, int64_t S,
                 int64_t* out, hipStream_t s) {
  TFA_CHECK(W >= 1 && W <= kMaxSortKeys, "sort_bounds: 1..", kMaxSortKeys, " words per row, got ", W);
  TFA_CHECK(n >= 0 && S >= 0 && S < (int64_t(1) << 31), "sort_bounds: bad row or splitter count");
  if (S == 0) return;
  TFA_CHECK(out != nullptr && splitters != nullptr, "sort_bounds: null buffer");
  TFA_CHECK(n == 0 || (words != nullptr && perm != nullptr), "sort_bounds: null buffer");
  hipLaunchKernelGGL(sort_bounds_kernel, dim3((unsigned)((S + kST - 1) / kST)), dim3(kST), 0, s,
                     reinterpret_cast<const uint64_t*>(words), W, n, perm,
                     reinterpret_cast<const uint64_t*>(splitters), S, out);
  TFA_LAUNCH_CHECK("sort_bounds_kernel");
}

}  // namespace k
}  // namespace tfa
