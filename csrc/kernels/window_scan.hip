// Segmented scans for Window / .over() (frame/window.py).
//
// The n rows of one partition are sorted by (partition keys, order keys) and
// come as their order-preserving words [W][n]. A row is a group head when one
// of its first P words differs from the previous row's, a peer head when one
// of the W words does; row 0 is both. Every channel is an inclusive scan
// under the segmented operator
//     (fa, a) (+) (fb, b) = (fa | fb, fb ? b : op(a, b))
// with the group-head flag and op one of: wrapping int64 add, f64 add, min and
// max of unsigned words. The head indexes are max-scans of (head ? row : 0),
// the peer-head count an add-scan of the peer-head flags. In reverse the
// scan runs over the mirrored index m = n - 1 - i (a head is then a row that
// differs from the next one) and an index channel gives n - 1 - m: the last
// row of the row's group / peer run.
//
//   window_scan    reduce-then-scan, three launches, no block waits for
//            another one:
//            1. every tile of kTile rows: the aggregate of every channel,
//            2. one block: wave w scans the tile aggregates of channels w,
//               w + 4, ..., 64 tiles a step, the carry running in a register,
//            3. every tile again, from its exclusive prefix, writes [C][n].
//            Inside a tile a lane takes kR consecutive rows (the words in
//            16-byte loads where the address allows), the lanes of a wave
//            are combined with six __shfl_up steps, the four waves through
//            LDS. The order of the additions depends on n and kTile alone.
//   window_finish  one elementwise launch: per row and output column the
//            carry-in of the partition's first group, the gather per frame
//            (the row, its last peer, the group's last row or the folded
//            total) and the decode to the output dtype.
//
// No float atomics, no inter-block communication, every index clamped to the
// row count before it is used.
#include <algorithm>
#include <limits>

#include "column_types.h"
#include "hip_common.h"
#include "sort_words.h"

namespace tfa {
namespace k {

namespace {

constexpr int kT = 256;  // threads per block
constexpr int kWaves = kT / kWave;
constexpr int kR = 8;  // consecutive rows per lane
constexpr int kTile = kT * kR;

enum : int { OP_ADD_I64 = 0, OP_ADD_F64 = 1, OP_MIN = 2, OP_MAX = 3 };

__host__ __device__ __forceinline__ int op_of(int kind) {
  switch (static_cast<WindowChan>(kind)) {
    case WindowChan::PEER_COUNT:
    case WindowChan::SUM_I64: return OP_ADD_I64;
    case WindowChan::SUM_F64: return OP_ADD_F64;
    case WindowChan::MIN_WORD: return OP_MIN;
    default: return OP_MAX;  // GROUP_HEAD, PEER_HEAD, MAX_WORD
  }
}

// identities that change no bit of the other operand (x + -0.0 == x for every x)
template <int OP>
__device__ __forceinline__ uint64_t ident() {
  return OP == OP_ADD_F64 ? kSign64 : (OP == OP_MIN ? ~0ull : 0ull);
}

template <int OP>
__device__ __forceinline__ uint64_t comb(uint64_t a, uint64_t b) {  // a: the earlier rows
  if (OP == OP_ADD_I64) return a + b;
  if (OP == OP_ADD_F64) return f64_bits(bits_f64(a) + bits_f64(b));
  if (OP == OP_MIN) return a < b ? a : b;
  return a > b ? a : b;
}

__device__ __forceinline__ uint64_t comb_rt(int op, uint64_t a, uint64_t b) {
  switch (op) {
    case OP_ADD_I64: return comb<OP_ADD_I64>(a, b);
    case OP_ADD_F64: return comb<OP_ADD_F64>(a, b);
    case OP_MIN: return comb<OP_MIN>(a, b);
    default: return comb<OP_MAX>(a, b);
  }
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int off) {
  return __shfl_up(static_cast<unsigned long long>(v), off, kWave);
}

// v[j] = the 8-byte element of mirrored row m0 + j (0 past the last row): the
// original rows lo .. lo + kR - 1, in one run of 16-byte loads when all of
// them exist and the first is 16-byte aligned
__device__ __forceinline__ void load_rows(const uint64_t* __restrict__ p, int64_t m0, int64_t n, bool rev,
                                          uint64_t (&v)[kR]) {
  const int64_t lo = rev ? n - m0 - kR : m0;
  if (lo >= 0 && lo + kR <= n && (reinterpret_cast<uintptr_t>(p + lo) & 15) == 0) {
    const ulonglong2* __restrict__ q = reinterpret_cast<const ulonglong2*>(p + lo);
#pragma unroll
    for (int j = 0; j < kR / 2; ++j) {
      const ulonglong2 t = q[j];
      v[2 * j] = t.x;
      v[2 * j + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kR; ++j) v[j] = (lo + j >= 0 && lo + j < n) ? p[lo + j] : 0ull;
  }
  if (rev) {
#pragma unroll
    for (int j = 0; j < kR / 2; ++j) {
      const uint64_t t = v[j];
      v[j] = v[kR - 1 - j];
      v[kR - 1 - j] = t;
    }
  }
}

// the channel's input of mirrored rows m0 .. m0 + kR - 1 of a value column
template <typename T>
__device__ __forceinline__ void load_vals(const void* __restrict__ src, int64_t m0, int64_t n, bool rev, int kind,
                                          uint64_t idv, uint64_t (&x)[kR]) {
  const T* __restrict__ p = static_cast<const T*>(src);
  T v[kR];
#pragma unroll
  for (int j = 0; j < kR; ++j) {
    const int64_t m = m0 + j;
    v[j] = m < n ? p[rev ? n - 1 - m : m] : T(0);
  }
  // (the kind is the same in every lane: one scalar branch around each loop)
  if (kind == static_cast<int>(WindowChan::SUM_I64)) {
#pragma unroll
    for (int j = 0; j < kR; ++j) x[j] = static_cast<uint64_t>(static_cast<int64_t>(v[j]));
  } else if (kind == static_cast<int>(WindowChan::SUM_F64)) {
#pragma unroll
    for (int j = 0; j < kR; ++j) x[j] = f64_bits(static_cast<double>(v[j]));
  } else {
#pragma unroll
    for (int j = 0; j < kR; ++j) x[j] = sort_word(v[j]);
  }
#pragma unroll
  for (int j = 0; j < kR; ++j)
    if (m0 + j >= n) x[j] = idv;
}

struct TileFlags {
  uint32_t g, p;  // bit j: mirrored row m0 + j is a group / peer head (rows past the end: neither)
};

__device__ __forceinline__ TileFlags tile_flags(const int64_t* __restrict__ words, int W, int P, int64_t n, bool rev,
                                                int64_t m0) {
  TileFlags f{0u, 0u};
  for (int w = 0; w < W; ++w) {
    const uint64_t* __restrict__ p = reinterpret_cast<const uint64_t*>(words) + (int64_t)w * n;
    uint64_t v[kR];
    load_rows(p, m0, n, rev, v);
    uint64_t prev = 0ull;  // mirrored row m0 - 1
    if (m0 > 0 && m0 - 1 < n) prev = p[rev ? n - m0 : m0 - 1];
    uint32_t d = 0u;
#pragma unroll
    for (int j = 0; j < kR; ++j) {
      d |= (v[j] != prev ? 1u : 0u) << j;
      prev = v[j];
    }
    f.p |= d;
    if (w < P) f.g |= d;
  }
  if (m0 == 0) {  // row 0 heads both
    f.g |= 1u;
    f.p |= 1u;
  }
  const int64_t left = n - m0;  // rows of this lane that exist
  const uint32_t valid = left >= kR ? 0xffu : (left > 0 ? (1u << left) - 1u : 0u);
  f.g &= valid;
  f.p &= valid;
  return f;
}

// One channel of one tile. x: the lane's inputs, g: its group-head bits.
// kWrite false: the tile's aggregate (value, any head) comes back in thread 0.
// kWrite true: x becomes the inclusive scan, started from the tile's prefix.
template <int OP, bool kWrite>
__device__ __forceinline__ void tile_scan(uint64_t (&x)[kR], uint32_t g, uint64_t tile_prefix, uint64_t* s_v,
                                          int* s_f, uint64_t& agg_v, int& agg_f) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x / kWave));
  uint64_t acc = x[0];
#pragma unroll
  for (int j = 1; j < kR; ++j) acc = ((g >> j) & 1u) ? x[j] : comb<OP>(acc, x[j]);
  int f = g != 0u;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint64_t ov = shfl_up64(acc, off);
    const int of = __shfl_up(f, off, kWave);
    if (lane >= off) {
      acc = f ? acc : comb<OP>(ov, acc);
      f |= of;
    }
  }
  if (lane == kWave - 1) {
    s_v[wave] = acc;
    s_f[wave] = f;
  }
  __syncthreads();
  if (!kWrite) {
    if (threadIdx.x == 0) {
      uint64_t v = s_v[0];
      int ff = s_f[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        v = s_f[w] ? s_v[w] : comb<OP>(v, s_v[w]);
        ff |= s_f[w];
      }
      agg_v = v;
      agg_f = ff;
    }
  } else {
    uint64_t ev = shfl_up64(acc, 1);
    int ef = __shfl_up(f, 1, kWave);
    if (lane == 0) {
      ev = ident<OP>();
      ef = 0;
    }
    uint64_t pv = tile_prefix;
    for (int w = 0; w < wave; ++w) pv = s_f[w] ? s_v[w] : comb<OP>(pv, s_v[w]);
    uint64_t c = ef ? ev : comb<OP>(pv, ev);
#pragma unroll
    for (int j = 0; j < kR; ++j) {
      c = ((g >> j) & 1u) ? x[j] : comb<OP>(c, x[j]);
      x[j] = c;
    }
  }
  __syncthreads();  // (the next channel writes s_v / s_f again)
}

template <bool kWrite>
__device__ __forceinline__ void tile_scan_rt(int op, uint64_t (&x)[kR], uint32_t g, uint64_t tile_prefix,
                                             uint64_t* s_v, int* s_f, uint64_t& agg_v, int& agg_f) {
  switch (op) {  // (uniform)
    case OP_ADD_I64: tile_scan<OP_ADD_I64, kWrite>(x, g, tile_prefix, s_v, s_f, agg_v, agg_f); break;
    case OP_ADD_F64: tile_scan<OP_ADD_F64, kWrite>(x, g, tile_prefix, s_v, s_f, agg_v, agg_f); break;
    case OP_MIN: tile_scan<OP_MIN, kWrite>(x, g, tile_prefix, s_v, s_f, agg_v, agg_f); break;
    default: tile_scan<OP_MAX, kWrite>(x, g, tile_prefix, s_v, s_f, agg_v, agg_f); break;
  }
}

__device__ __forceinline__ uint64_t ident_rt(int op) {
  return op == OP_ADD_F64 ? kSign64 : (op == OP_MIN ? ~0ull : 0ull);
}

// the lane's inputs of channel c
__device__ __forceinline__ void chan_inputs(const WindowChans& ch, int c, const TileFlags& fl, int64_t m0, int64_t n,
                                            bool rev, uint64_t (&x)[kR]) {
  const int kind = ch.kind[c];
  if (kind == static_cast<int>(WindowChan::GROUP_HEAD) || kind == static_cast<int>(WindowChan::PEER_HEAD)) {
    const uint32_t h = kind == static_cast<int>(WindowChan::GROUP_HEAD) ? fl.g : fl.p;
#pragma unroll
    for (int j = 0; j < kR; ++j) x[j] = ((h >> j) & 1u) ? static_cast<uint64_t>(m0 + j) : 0ull;
    return;
  }
  if (kind == static_cast<int>(WindowChan::PEER_COUNT)) {
#pragma unroll
    for (int j = 0; j < kR; ++j) x[j] = (fl.p >> j) & 1u;
    return;
  }
  const uint64_t idv = ident_rt(op_of(kind));
  const void* src = ch.ptr[c];
  dispatch_column(ch.dtype[c], [&](auto tag) { load_vals<decltype(tag)>(src, m0, n, rev, kind, idv, x); });  // (uniform)
}

}  // namespace

// block t: the aggregates of tile t -> agg_v[c][t], agg_f[t]
__global__ __launch_bounds__(kT) void window_tile_reduce_kernel(const int64_t* __restrict__ words, int W, int P,
                                                                int64_t n, int rev, WindowChans ch, int64_t ntiles,
                                                                uint64_t* __restrict__ agg_v,
                                                                int* __restrict__ agg_f) {
  __shared__ uint64_t s_v[kWaves];
  __shared__ int s_f[kWaves];
  const int64_t tile = blockIdx.x;
  const int64_t m0 = tile * kTile + (int64_t)threadIdx.x * kR;
  const TileFlags fl = tile_flags(words, W, P, n, rev != 0, m0);
  for (int c = 0; c < ch.n; ++c) {
    uint64_t x[kR];
    chan_inputs(ch, c, fl, m0, n, rev != 0, x);
    uint64_t av = 0ull;
    int af = 0;
    tile_scan_rt<false>(op_of(ch.kind[c]), x, fl.g, 0ull, s_v, s_f, av, af);
    if (threadIdx.x == 0) {
      agg_v[(int64_t)c * ntiles + tile] = av;
      if (c == 0) agg_f[tile] = af;
    }
  }
}

namespace {

template <int OP>
__device__ __forceinline__ void scan_tiles(const uint64_t* __restrict__ av, const int* __restrict__ af,
                                           int64_t ntiles, uint64_t* __restrict__ pre) {
  const int lane = threadIdx.x & (kWave - 1);
  uint64_t carry = ident<OP>();
  for (int64_t base = 0; base < ntiles; base += kWave) {
    const int64_t t = base + lane;
    uint64_t v = t < ntiles ? av[t] : ident<OP>();
    int f = t < ntiles ? af[t] : 0;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const uint64_t ov = shfl_up64(v, off);
      const int of = __shfl_up(f, off, kWave);
      if (lane >= off) {
        v = f ? v : comb<OP>(ov, v);
        f |= of;
      }
    }
    uint64_t ev = shfl_up64(v, 1);
    int ef = __shfl_up(f, 1, kWave);
    if (lane == 0) {
      ev = ident<OP>();
      ef = 0;
    }
    if (t < ntiles) pre[t] = ef ? ev : comb<OP>(carry, ev);
    const uint64_t lv = __shfl(static_cast<unsigned long long>(v), kWave - 1, kWave);
    const int lf = __shfl(f, kWave - 1, kWave);
    carry = lf ? lv : comb<OP>(carry, lv);
  }
}

}  // namespace

// one block: pre[c][t] = the segmented fold of tiles 0 .. t - 1 of channel c
__global__ __launch_bounds__(kT) void window_tile_scan_kernel(WindowChans ch, int64_t ntiles,
                                                              const uint64_t* __restrict__ agg_v,
                                                              const int* __restrict__ agg_f,
                                                              uint64_t* __restrict__ pre) {
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x / kWave));
  for (int c = wave; c < ch.n; c += kWaves) {
    const uint64_t* av = agg_v + (int64_t)c * ntiles;
    uint64_t* pv = pre + (int64_t)c * ntiles;
    switch (op_of(ch.kind[c])) {
      case OP_ADD_I64: scan_tiles<OP_ADD_I64>(av, agg_f, ntiles, pv); break;
      case OP_ADD_F64: scan_tiles<OP_ADD_F64>(av, agg_f, ntiles, pv); break;
      case OP_MIN: scan_tiles<OP_MIN>(av, agg_f, ntiles, pv); break;
      default: scan_tiles<OP_MAX>(av, agg_f, ntiles, pv); break;
    }
  }
}

// block t: tile t scanned from pre[c][t] -> out[c][row]
__global__ __launch_bounds__(kT) void window_tile_write_kernel(const int64_t* __restrict__ words, int W, int P,
                                                               int64_t n, int rev, WindowChans ch, int64_t ntiles,
                                                               const uint64_t* __restrict__ pre,
                                                               int64_t* __restrict__ out) {
  __shared__ uint64_t s_v[kWaves];
  __shared__ int s_f[kWaves];
  const int64_t tile = blockIdx.x;
  const int64_t m0 = tile * kTile + (int64_t)threadIdx.x * kR;
  const TileFlags fl = tile_flags(words, W, P, n, rev != 0, m0);
  for (int c = 0; c < ch.n; ++c) {
    uint64_t x[kR];
    chan_inputs(ch, c, fl, m0, n, rev != 0, x);
    uint64_t av = 0ull;
    int af = 0;
    tile_scan_rt<true>(op_of(ch.kind[c]), x, fl.g, pre[(int64_t)c * ntiles + tile], s_v, s_f, av, af);
    const int kind = ch.kind[c];
    const bool index = kind == static_cast<int>(WindowChan::GROUP_HEAD) ||
                       kind == static_cast<int>(WindowChan::PEER_HEAD);
    uint64_t* __restrict__ o = reinterpret_cast<uint64_t*>(out) + (int64_t)c * n;
    if (rev) {
#pragma unroll
      for (int j = 0; j < kR; ++j) {
        const int64_t m = m0 + j;
        if (m < n) o[n - 1 - m] = index ? static_cast<uint64_t>(n - 1) - x[j] : x[j];
      }
    } else if (m0 + kR <= n && (reinterpret_cast<uintptr_t>(o + m0) & 15) == 0) {
      ulonglong2* __restrict__ q = reinterpret_cast<ulonglong2*>(o + m0);
#pragma unroll
      for (int j = 0; j < kR / 2; ++j) q[j] = make_ulonglong2(x[2 * j], x[2 * j + 1]);
    } else {
#pragma unroll
      for (int j = 0; j < kR; ++j)
        if (m0 + j < n) o[m0 + j] = x[j];
    }
  }
}

// thread i of block (.., o): output o of row i
__global__ __launch_bounds__(kT) void window_finish_kernel(const int64_t* __restrict__ fwd,
                                                           const int64_t* __restrict__ rev, int64_t n,
                                                           WindowFinishSpec sp) {
  const int o = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const int64_t gh = clamp64(fwd[i], 0, i), ph = clamp64(fwd[n + i], gh, i);
  const int64_t gl = clamp64(rev[i], i, n - 1), pl = clamp64(rev[n + i], i, gl);
  const bool first = sp.has_carry && gh == 0;             // the group began in an earlier partition
  const bool open = sp.has_total && gl == n - 1;          // the group runs on into a later one
  const int64_t before = first ? sp.carry_rows : 0;
  const WindowFn fn = sp.fn[o];
  const WindowFrame fr = sp.frame[o];
  void* out = sp.out[o];
  if (fn == WindowFn::ROW_NUMBER) {
    static_cast<int32_t*>(out)[i] = static_cast<int32_t>(i - gh + 1 + before);
    return;
  }
  if (fn == WindowFn::RANK) {
    static_cast<int32_t*>(out)[i] = static_cast<int32_t>(ph - gh + 1 + before);
    return;
  }
  const int64_t t = fr == WindowFrame::ROWS ? i : (fr == WindowFrame::RANGE ? pl : gl);
  const bool whole = fr == WindowFrame::WHOLE && open;
  const int64_t rows = whole ? sp.total_rows : t - gh + 1 + before;
  if (fn == WindowFn::COUNT) {
    static_cast<int64_t*>(out)[i] = rows;
    return;
  }
  const int c = sp.chan[o];
  uint64_t v;
  if (whole) {
    v = sp.total[c];
  } else {
    v = static_cast<uint64_t>(fwd[(int64_t)c * n + t]);
    if (first) v = comb_rt(sp.op[c], sp.carry[c], v);
  }
  const DType dt = sp.dtype[o];
  switch (fn) {
    case WindowFn::DENSE_RANK: static_cast<int32_t*>(out)[i] = static_cast<int32_t>(v); break;
    case WindowFn::SUM: static_cast<uint64_t*>(out)[i] = v; break;  // (int64 or f64 bits: the channel's)
    case WindowFn::AVG: static_cast<double*>(out)[i] = bits_f64(v) / static_cast<double>(rows); break;
    default: store_word(out, i, dt, v); break;  // MIN, MAX: the word back to the column's type
  }
}

// ------------------------------------------------------------------ host API
namespace {

bool value_kind(int kind) { return kind >= static_cast<int>(WindowChan::SUM_I64); }

int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

size_t align16(size_t b) { return (b + 15) & ~size_t(15); }

}  // namespace

int window_tile_rows() { return kTile; }

// workspace: u64 agg_v[C][ntiles] | u64 pre[C][ntiles] | int agg_f[ntiles]
size_t window_scan_workspace_bytes(int nchan, int64_t n) {
  if (n <= 0 || nchan <= 0) return 0;
  const size_t nt = static_cast<size_t>(tiles_of(n));
  return 2 * align16(8 * nt * nchan) + align16(4 * nt);
}

void window_scan(const int64_t* words, int W, int P, int64_t n, bool reverse, const WindowChans& ch, int64_t* out,
                 void* ws, size_t ws_size, hipStream_t s) {
  TFA_CHECK(ch.n >= 1 && ch.n <= kMaxPackCols, "window_scan: 1..", kMaxPackCols, " channels, got ", ch.n);
  TFA_CHECK(W >= 0 && W <= kMaxSortKeys && P >= 0 && P <= W, "window_scan: 0 <= P <= W <= ", kMaxSortKeys,
            " expected, got P = ", P, ", W = ", W);
  TFA_CHECK(n >= 0, "window_scan: negative row count");
  for (int c = 0; c < ch.n; ++c) {
    TFA_CHECK(ch.kind[c] >= 0 && ch.kind[c] <= static_cast<int>(WindowChan::MAX_WORD), "window_scan: channel ", c,
              " is of an unknown kind");
    if (value_kind(ch.kind[c])) check_stat_column("window_scan", "channel", c, ch.dtype[c], ch.ptr[c], n);
  }
  if (n == 0) return;
  const int64_t nt = tiles_of(n);
  TFA_CHECK(nt < (int64_t(1) << 31), "window_scan: too many rows");
  TFA_CHECK((W == 0 || words != nullptr) && out != nullptr && ws != nullptr, "window_scan: null buffer");
  TFA_CHECK(reinterpret_cast<uintptr_t>(words) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(ws) % 8 == 0,
            "window_scan: unaligned buffer");
  TFA_CHECK(ws_size >= window_scan_workspace_bytes(ch.n, n), "window_scan: workspace too small");
  char* w = static_cast<char*>(ws);
  uint64_t* agg_v = reinterpret_cast<uint64_t*>(w);
  w += align16(8 * static_cast<size_t>(nt) * ch.n);
  uint64_t* pre = reinterpret_cast<uint64_t*>(w);
  w += align16(8 * static_cast<size_t>(nt) * ch.n);
  int* agg_f = reinterpret_cast<int*>(w);
  const int rv = reverse ? 1 : 0;
  hipLaunchKernelGGL(window_tile_reduce_kernel, dim3((unsigned)nt), dim3(kT), 0, s, words, W, P, n, rv, ch, nt, agg_v,
                     agg_f);
  TFA_LAUNCH_CHECK("window_tile_reduce_kernel");
  hipLaunchKernelGGL(window_tile_scan_kernel, dim3(1), dim3(kT), 0, s, ch, nt, (const uint64_t*)agg_v,
                     (const int*)agg_f, pre);
  TFA_LAUNCH_CHECK("window_tile_scan_kernel");
  hipLaunchKernelGGL(window_tile_write_kernel, dim3((unsigned)nt), dim3(kT), 0, s, words, W, P, n, rv, ch, nt,
                     (const uint64_t*)pre, out);
  TFA_LAUNCH_CHECK("window_tile_write_kernel");
}

void window_finish(const int64_t* fwd, const int64_t* rev, int64_t n, const WindowFinishSpec& sp, hipStream_t s) {
  TFA_CHECK(sp.n_out >= 1 && sp.n_out <= kMaxPackCols, "window_finish: 1..", kMaxPackCols, " outputs, got ", sp.n_out);
  TFA_CHECK(sp.n_chan >= 2 && sp.n_chan <= kMaxPackCols, "window_finish: 2..", kMaxPackCols, " channels, got ",
            sp.n_chan);
  TFA_CHECK(n >= 0, "window_finish: negative row count");
  for (int c = 0; c < sp.n_chan; ++c)
    TFA_CHECK(sp.op[c] >= OP_ADD_I64 && sp.op[c] <= OP_MAX, "window_finish: channel ", c, " has an unknown operator");
  for (int o = 0; o < sp.n_out; ++o) {
    TFA_CHECK(static_cast<int>(sp.fn[o]) >= 0 && static_cast<int>(sp.fn[o]) <= static_cast<int>(WindowFn::MAX),
              "window_finish: output ", o, " asks for an unknown function");
    TFA_CHECK(static_cast<int>(sp.frame[o]) >= 0 && static_cast<int>(sp.frame[o]) <= static_cast<int>(WindowFrame::WHOLE),
              "window_finish: output ", o, " asks for an unknown frame");
    TFA_CHECK(sp.chan[o] >= 0 && sp.chan[o] < sp.n_chan, "window_finish: output ", o, " names channel ", sp.chan[o],
              " of ", sp.n_chan);
    TFA_CHECK(is_stat_dtype(sp.dtype[o]), "window_finish: output ", o, " has a dtype that is not supported");
    TFA_CHECK(n == 0 || sp.out[o] != nullptr, "window_finish: output ", o, " has no buffer");
  }
  if (n == 0) return;
  TFA_CHECK(fwd != nullptr && rev != nullptr, "window_finish: null buffer");
  TFA_CHECK((n + kT - 1) / kT < (int64_t(1) << 31), "window_finish: too many rows");
  hipLaunchKernelGGL(window_finish_kernel, dim3((unsigned)((n + kT - 1) / kT), sp.n_out), dim3(kT), 0, s, fwd, rev, n,
                     sp);
  TFA_LAUNCH_CHECK("window_finish_kernel");
}

int window_chan_op(int kind) { return op_of(kind); }

}  // namespace k
}  // namespace tfa
