// Holistic aggregates per group for GroupedData.agg / DataFrame.agg
// (frame/order_agg.py): median / percentile, percentile_approx, mode and
// countDistinct.
//
// The n rows of one partition are sorted by (group keys, value columns) and
// come as their order-preserving words [W][n]: the first P words define the
// groups, all W the peer runs (rows with an equal full tuple), the last word
// is the value. starts [ng + 1] lists the group heads (unique.hip over the
// first P words) and ph [n] the head row of every row's peer run
// (window_scan.hip, the PEER_HEAD channel).
//
//   group_order_summary   per group the number of peer heads (the distinct
//            count) and the first longest peer run (the mode). A run's length
//            is known at its last row i as i - ph[i] + 1; a run never leaves
//            its group, so the mode is the largest packed key
//            (length << 32) | (0xFFFFFFFF - head row) over the group's
//            run-last rows: the longer run, then the earlier head. The work
//            split is group_stats.hip's (group_items): a work item is at most
//            group_chunk_rows() rows of one group, taken by one wave, each
//            lane two consecutive rows a step (one 16-byte load where the
//            address allows); the lanes combine by shuffles. A group's chunk
//            records are folded in chunk order by a second kernel: one thread
//            up to kFoldSerial chunks, the thread's wave together beyond.
//            Integers only, so the fold order changes no bit.
//   group_order_finish    per group and output: the distinct count, the mode
//            word, the word at rank max(ceil(p N) - 1, 0), or Spark's
//            interpolated percentile of the two words around p (N - 1), up to
//            kMaxPackCols outputs in one launch (the output is the grid's y,
//            the percentage its z).
//
// No float atomics, no inter-block communication, every index clamped to the
// row count before it is used.
#include <cmath>

#include "column_types.h"
#include "hip_common.h"
#include "sort_words.h"

namespace tfa {
namespace k {

namespace {

constexpr int kT = 256;  // threads per block of every kernel here
constexpr int kWaves = kT / kWave;
constexpr int kFoldSerial = 8;  // most chunks of a group one thread folds on its own
constexpr uint64_t kLow32 = 0xffffffffull;

__device__ __forceinline__ uint64_t mode_key(int64_t len, int64_t head) {
  return (static_cast<uint64_t>(len) << 32) | (kLow32 - (static_cast<uint64_t>(head) & kLow32));
}

__device__ __forceinline__ void wave_combine(int64_t& cnt, uint64_t& key) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    cnt += __shfl_xor(static_cast<long long>(cnt), off, kWave);
    const uint64_t o = __shfl_xor(static_cast<unsigned long long>(key), off, kWave);
    key = o > key ? o : key;
  }
}

// the value a word of a column of dtype dt came from, as f64
__device__ __forceinline__ double word_f64(uint64_t w, DType dt) {
  switch (dt) {
    case DType::F32: return static_cast<double>(__uint_as_float(decode_f32(w)));
    case DType::F64: return bits_f64(decode_f64(w));
    case DType::U8: return static_cast<double>(w);
    default: return static_cast<double>(decode_int(w));
  }
}

}  // namespace

// wave w of block b: item b * kWaves + w -> part[item] = (peer heads, largest mode key)
// of rows [lo, hi) of its group. coffs [ng + 1]: the exclusive scan of the
// groups' chunk counts, coffs[ng] == items
__global__ __launch_bounds__(kT) void group_order_chunk_kernel(const int64_t* __restrict__ ph, int64_t n,
                                                               const int64_t* __restrict__ starts,
                                                               const int64_t* __restrict__ coffs, int64_t ng,
                                                               int64_t items, int chunk, int64_t* __restrict__ part) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t item = (int64_t)blockIdx.x * kWaves +
                       __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x / kWave));
  if (item >= items) return;  // (the whole wave)
  // coffs[0] == 0 <= item < coffs[ng]: the group lies in [0, ng - 1]
  const int64_t g = last_not_above(coffs, 0, 0, ng - 1, item);
  const int64_t ch = item - coffs[g];
  const int64_t a = clamp64(starts[g], 0, n), b = clamp64(starts[g + 1], a, n);
  const int64_t lo = clamp64(a + ch * chunk, a, b);
  const int64_t hi = lo + chunk < b ? lo + chunk : b;
  int64_t cnt = 0;
  uint64_t key = 0ull;
  // the lane's rows base, base + 1 (base even) and the head of the row after them
  for (int64_t base = (lo & ~int64_t(1)) + 2 * lane; base < hi; base += 2 * kWave) {
    int64_t p0, p1;
    if (base + 1 < n && (reinterpret_cast<uintptr_t>(ph + base) & 15) == 0) {
      const longlong2 t = *reinterpret_cast<const longlong2*>(ph + base);
      p0 = t.x;
      p1 = t.y;
    } else {
      p0 = base < n ? ph[base] : base;
      p1 = base + 1 < n ? ph[base + 1] : base + 1;
    }
    const int64_t p2 = base + 2 < n ? ph[base + 2] : base + 2;  // (past the end: a head)
    if (base >= lo) {  // (base < hi)
      const int64_t p = clamp64(p0, a, base);
      cnt += p == base;
      if (p1 == base + 1) {
        const uint64_t kk = mode_key(base - p + 1, p);
        key = kk > key ? kk : key;
      }
    }
    if (base + 1 >= lo && base + 1 < hi) {
      const int64_t p = clamp64(p1, a, base + 1);
      cnt += p == base + 1;
      if (p2 == base + 2) {
        const uint64_t kk = mode_key(base + 2 - p, p);
        key = kk > key ? kk : key;
      }
    }
  }
  wave_combine(cnt, key);
  if (lane == 0) {
    part[2 * item] = cnt;
    part[2 * item + 1] = static_cast<int64_t>(key);
  }
}

// thread g: part[coffs[g] .. coffs[g + 1]) folded in chunk order -> distinct,
// mode_pos, mode_len of group g. More than kFoldSerial chunks (a key that holds
// a large share of the rows): the thread's wave takes them together, lane l
// the chunks l, l + 64, ...
__global__ __launch_bounds__(kT) void group_order_fold_kernel(const int64_t* __restrict__ part,
                                                              const int64_t* __restrict__ coffs, int64_t ng,
                                                              int64_t items, int64_t* __restrict__ distinct,
                                                              int64_t* __restrict__ mode_pos,
                                                              int64_t* __restrict__ mode_len) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
  const bool valid = t < ng;
  const int64_t g = valid ? t : 0;
  const int64_t a = clamp64(coffs[g], 0, items - 1), b = clamp64(coffs[g + 1], a + 1, items);
  const bool wide = valid && b - a > kFoldSerial;
  if (valid && !wide) {
    int64_t cnt = 0;
    uint64_t key = 0ull;
    for (int64_t i = a; i < b; ++i) {
      cnt += part[2 * i];
      const uint64_t kk = static_cast<uint64_t>(part[2 * i + 1]);
      key = kk > key ? kk : key;
    }
    distinct[g] = cnt;
    mode_len[g] = static_cast<int64_t>(key >> 32);
    mode_pos[g] = static_cast<int64_t>(kLow32 - (key & kLow32));
  }
  unsigned long long todo = __ballot(wide);  // (the same in every lane: at most 64 rounds)
  while (todo) {
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int64_t sa = __shfl(static_cast<long long>(a), src, kWave), sb = __shfl(static_cast<long long>(b), src, kWave);
    const int64_t sg = __shfl(static_cast<long long>(g), src, kWave);
    int64_t cnt = 0;
    uint64_t key = 0ull;
    for (int64_t i = sa + lane; i < sb; i += kWave) {
      cnt += part[2 * i];
      const uint64_t kk = static_cast<uint64_t>(part[2 * i + 1]);
      key = kk > key ? kk : key;
    }
    wave_combine(cnt, key);
    if (lane == 0) {
      distinct[sg] = cnt;
      mode_len[sg] = static_cast<int64_t>(key >> 32);
      mode_pos[sg] = static_cast<int64_t>(kLow32 - (key & kLow32));
    }
  }
}

// thread g of block (.., o, q): percentage q of output o of group g
__global__ __launch_bounds__(kT) void group_order_finish_kernel(const int64_t* __restrict__ value_words, int64_t n,
                                                                const int64_t* __restrict__ starts,
                                                                const int64_t* __restrict__ distinct,
                                                                const int64_t* __restrict__ mode_pos, int64_t ng,
                                                                GroupOrderSpec sp) {
  // (no contraction below: the intrinsics' bodies are inlined under the file's mode, the pragma governs what is
  // written here, so the arithmetic is spelled out)
#pragma clang fp contract(off)
  const int o = blockIdx.y, q = blockIdx.z;
  const int Q = sp.nq[o];
  const int64_t g = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (g >= ng || q >= Q) return;
  const GroupOrderFn fn = sp.fn[o];
  void* out = sp.out[o];
  if (fn == GroupOrderFn::COUNT_DISTINCT) {
    static_cast<int64_t*>(out)[g] = distinct[g];
    return;
  }
  const uint64_t* __restrict__ vw = reinterpret_cast<const uint64_t*>(value_words);
  const int64_t a = clamp64(starts[g], 0, n - 1), b = clamp64(starts[g + 1], a + 1, n);
  const int64_t N = b - a;  // (a group has rows)
  const DType dt = sp.dtype;
  if (fn == GroupOrderFn::MODE) {
    store_word(out, g, dt, vw[clamp64(mode_pos[g], a, b - 1)]);
    return;
  }
  const double p = sp.pct[o][q];
  const int64_t at = g * Q + q;
  if (fn == GroupOrderFn::PERCENTILE_APPROX) {
    const double r = ceil(p * static_cast<double>(N)) - 1.0;
    store_word(out, at, dt, vw[a + clamp64(static_cast<int64_t>(r), 0, N - 1)]);
    return;
  }
  // PERCENTILE: Spark's interpolation, two rounded products and one rounded sum
  const double pos = p * static_cast<double>(N - 1);
  const double lo = floor(pos), hi = ceil(pos);
  const double vlo = word_f64(vw[a + clamp64(static_cast<int64_t>(lo), 0, N - 1)], dt);
  double v = vlo;
  if (lo != hi) {
    const double vhi = word_f64(vw[a + clamp64(static_cast<int64_t>(hi), 0, N - 1)], dt);
    const double wl = hi - pos, wh = pos - lo;
    const double tl = wl * vlo, th = wh * vhi;
    v = tl + th;
  }
  // (every NaN leaves as the quiet NaN, as the typed results do)
  static_cast<uint64_t*>(out)[at] = v != v ? 0x7ff8000000000000ull : f64_bits(v);
}

// ------------------------------------------------------------------ host API
namespace {

int64_t max_chunks(int64_t n) {
  const int64_t c = group_chunk_rows();
  return n <= 0 ? 1 : (n + c - 1) / c;
}

size_t align16(size_t b) { return (b + 15) & ~size_t(15); }

}  // namespace

int group_order_chunk_rows() { return group_chunk_rows(); }

// workspace: int64 ph[n] | window_scan's | group_items' | int64 part[ng + max_chunks][2]
size_t group_order_summary_workspace_bytes(int64_t n, int64_t ng) {
  if (n <= 0 || ng <= 0) return 0;
  return align16(8 * static_cast<size_t>(n)) + align16(window_scan_workspace_bytes(1, n)) +
         align16(group_items_workspace_bytes(ng)) + 16 * static_cast<size_t>(ng + max_chunks(n));
}

void group_order_summary(const int64_t* words, int W, int P, int64_t n, const int64_t* starts, int64_t ng,
                         int64_t* distinct, int64_t* mode_pos, int64_t* mode_len, void* ws, size_t ws_size,
                         hipStream_t s) {
  TFA_CHECK(W >= 0 && W <= kMaxSortKeys && P >= 0 && P <= W, "group_order_summary: 0 <= P <= W <= ", kMaxSortKeys,
            " expected, got P = ", P, ", W = ", W);
  TFA_CHECK(n >= 0 && ng >= 0 && ng <= n, "group_order_summary: bad row or group count");
  if (n == 0 || ng == 0) return;
  TFA_CHECK(n < (int64_t(1) << 31), "group_order_summary: ", n, " rows; a row index is packed in 32 bits");
  TFA_CHECK((W == 0 || words != nullptr) && starts != nullptr && distinct != nullptr && mode_pos != nullptr &&
                mode_len != nullptr && ws != nullptr,
            "group_order_summary: null buffer");
  TFA_CHECK(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "group_order_summary: unaligned workspace");
  TFA_CHECK(ws_size >= group_order_summary_workspace_bytes(n, ng), "group_order_summary: workspace too small");
  char* w = static_cast<char*>(ws);
  int64_t* ph = reinterpret_cast<int64_t*>(w);
  w += align16(8 * static_cast<size_t>(n));
  void* scan_ws = w;
  const size_t scan_bytes = align16(window_scan_workspace_bytes(1, n));
  w += scan_bytes;
  void* items_ws = w;
  const size_t items_bytes = align16(group_items_workspace_bytes(ng));
  w += items_bytes;
  int64_t* part = reinterpret_cast<int64_t*>(w);
  WindowChans ch;
  ch.n = 1;
  ch.kind[0] = static_cast<int>(WindowChan::PEER_HEAD);
  ch.dtype[0] = DType::U8;
  ch.ptr[0] = nullptr;
  window_scan(words, W, P, n, false, ch, ph, scan_ws, scan_bytes, s);
  const GroupItems it = group_items(starts, ng, n, items_ws, items_bytes, s);  // (synchronises)
  TFA_CHECK(it.coffs != nullptr && it.items >= ng && it.items <= ng + max_chunks(n), "group_order_summary: ",
            it.items, " work items for ", ng, " groups of ", n, " rows");
  hipLaunchKernelGGL(group_order_chunk_kernel, dim3((unsigned)((it.items + kWaves - 1) / kWaves)), dim3(kT), 0, s,
                     (const int64_t*)ph, n, starts, it.coffs, ng, it.items, group_chunk_rows(), part);
  TFA_LAUNCH_CHECK("group_order_chunk_kernel");
  hipLaunchKernelGGL(group_order_fold_kernel, dim3((unsigned)((ng + kT - 1) / kT)), dim3(kT), 0, s,
                     (const int64_t*)part, it.coffs, ng, it.items, distinct, mode_pos, mode_len);
  TFA_LAUNCH_CHECK("group_order_fold_kernel");
}

void group_order_finish(const int64_t* value_words, int64_t n, const int64_t* starts, const int64_t* distinct,
                        const int64_t* mode_pos, int64_t ng, const GroupOrderSpec& sp, hipStream_t s) {
  TFA_CHECK(sp.n_out >= 1 && sp.n_out <= kMaxPackCols, "group_order_finish: 1..", kMaxPackCols, " outputs, got ",
            sp.n_out);
  TFA_CHECK(n >= 0 && ng >= 0 && ng <= n, "group_order_finish: bad row or group count");
  TFA_CHECK(is_stat_dtype(sp.dtype), "group_order_finish: the value dtype is not supported");
  int qmax = 1;
  for (int o = 0; o < sp.n_out; ++o) {
    TFA_CHECK(static_cast<int>(sp.fn[o]) >= 0 && static_cast<int>(sp.fn[o]) <= static_cast<int>(GroupOrderFn::PERCENTILE),
              "group_order_finish: output ", o, " asks for an unknown function");
    TFA_CHECK(sp.nq[o] >= 1 && sp.nq[o] <= kMaxPercentages, "group_order_finish: output ", o, " has ", sp.nq[o],
              " percentages, 1..", kMaxPercentages, " expected");
    for (int q = 0; q < sp.nq[o]; ++q)
      TFA_CHECK(sp.pct[o][q] >= 0.0 && sp.pct[o][q] <= 1.0, "group_order_finish: a percentage outside [0, 1]");
    TFA_CHECK(ng == 0 || sp.out[o] != nullptr, "group_order_finish: output ", o, " has no buffer");
    qmax = sp.nq[o] > qmax ? sp.nq[o] : qmax;
  }
  if (ng == 0) return;
  TFA_CHECK(value_words != nullptr && starts != nullptr && distinct != nullptr && mode_pos != nullptr,
            "group_order_finish: null buffer");
  TFA_CHECK((ng + kT - 1) / kT < (int64_t(1) << 31), "group_order_finish: too many groups");
  hipLaunchKernelGGL(group_order_finish_kernel, dim3((unsigned)((ng + kT - 1) / kT), sp.n_out, qmax), dim3(kT), 0, s,
                     value_words, n, starts, distinct, mode_pos, ng, sp);
  TFA_LAUNCH_CHECK("group_order_finish_kernel");
}

}  // namespace k
}  // namespace tfa
