#include "unpack.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#if defined(__linux__)
#include <sched.h>
#endif
#if defined(__x86_64__)
#include <immintrin.h>
#define TFA_UNPACK_X86 1
#else
#define TFA_UNPACK_X86 0
#endif

namespace tfa {
namespace unpack {

namespace {

// One tile: `mask` and `out` point at the tile's first mask word / element,
// n is its word count, v its values, vend the end of the whole value region
// (a vector variant never loads past it).
using TileFn = void (*)(const uint32_t* mask, const uint32_t* v, const uint32_t* vend, uint32_t* out, int64_t n);

inline uint32_t tail_bits(int64_t n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1u); }

// groups [j0, ...) of 32 words and the ragged tail, one mask bit at a time
void scalar_from(const uint32_t* mask, const uint32_t* v, uint32_t* out, int64_t n, int64_t j0) {
  for (int64_t j = j0; j * 32 < n; ++j) {
    const int64_t left = n - j * 32;
    const int w = static_cast<int>(std::min<int64_t>(32, left));
    uint32_t m = mask[j] & tail_bits(left);
    uint32_t* o = out + j * 32;
    std::memset(o, 0, static_cast<size_t>(w) * 4);
    while (m) {
      o[__builtin_ctz(m)] = *v++;
      m &= m - 1;
    }
  }
}

void tile_scalar(const uint32_t* mask, const uint32_t* v, const uint32_t*, uint32_t* out, int64_t n) {
  scalar_from(mask, v, out, n, 0);
}

#if TFA_UNPACK_X86
__attribute__((target("avx512f,popcnt"))) void tile_avx512(const uint32_t* mask, const uint32_t* v,
                                                           const uint32_t*, uint32_t* out, int64_t n) {
  const int64_t full = n / 32;
  const bool stream = (reinterpret_cast<uintptr_t>(out) & 63) == 0;
  if (stream) {
    for (int64_t j = 0; j < full; ++j) {
      const uint32_t m = mask[j];
      const __mmask16 lo = static_cast<__mmask16>(m & 0xffffu), hi = static_cast<__mmask16>(m >> 16);
      // a masked expand-load touches only the words it takes
      const __m512i a = _mm512_maskz_expandloadu_epi32(lo, v);
      v += __builtin_popcount(m & 0xffffu);
      const __m512i b = _mm512_maskz_expandloadu_epi32(hi, v);
      v += __builtin_popcount(m >> 16);
      _mm512_stream_si512(reinterpret_cast<__m512i*>(out + j * 32), a);
      _mm512_stream_si512(reinterpret_cast<__m512i*>(out + j * 32 + 16), b);
    }
    _mm_sfence();
  } else {
    for (int64_t j = 0; j < full; ++j) {
      const uint32_t m = mask[j];
      const __mmask16 lo = static_cast<__mmask16>(m & 0xffffu), hi = static_cast<__mmask16>(m >> 16);
      const __m512i a = _mm512_maskz_expandloadu_epi32(lo, v);
      v += __builtin_popcount(m & 0xffffu);
      const __m512i b = _mm512_maskz_expandloadu_epi32(hi, v);
      v += __builtin_popcount(m >> 16);
      _mm512_storeu_si512(out + j * 32, a);
      _mm512_storeu_si512(out + j * 32 + 16, b);
    }
  }
  scalar_from(mask, v, out, n, full);
}

// per 8-bit mask: the lane permutation that spreads the next popcount(m)
// loaded words to the set bit positions (unset lanes are zeroed by an AND)
struct Avx2Lut {
  alignas(32) uint32_t idx[256][8];
  Avx2Lut() {
    for (int m = 0; m < 256; ++m) {
      int k = 0;
      for (int i = 0; i < 8; ++i) idx[m][i] = ((m >> i) & 1) ? static_cast<uint32_t>(k++) : 0u;
    }
  }
};

__attribute__((target("avx2,popcnt"))) void tile_avx2(const uint32_t* mask, const uint32_t* v, const uint32_t* vend,
                                                      uint32_t* out, int64_t n) {
  static const Avx2Lut lut;
  const int64_t full = n / 32;
  const bool stream = (reinterpret_cast<uintptr_t>(out) & 31) == 0;
  const __m256i bit = _mm256_setr_epi32(1, 2, 4, 8, 16, 32, 64, 128);
  for (int64_t j = 0; j < full; ++j) {
    const uint32_t m = mask[j];
    for (int q = 0; q < 4; ++q) {
      const uint32_t mb = (m >> (8 * q)) & 0xffu;
      uint32_t* o = out + j * 32 + q * 8;
      const int pc = __builtin_popcount(mb);
      if (v + 8 <= vend) {
        const __m256i src = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(v));
        const __m256i perm =
            _mm256_permutevar8x32_epi32(src, _mm256_load_si256(reinterpret_cast<const __m256i*>(lut.idx[mb])));
        const __m256i keep = _mm256_cmpeq_epi32(_mm256_and_si256(_mm256_set1_epi32(static_cast<int>(mb)), bit), bit);
        const __m256i r = _mm256_and_si256(perm, keep);
        if (stream)
          _mm256_stream_si256(reinterpret_cast<__m256i*>(o), r);
        else
          _mm256_storeu_si256(reinterpret_cast<__m256i*>(o), r);
      } else {  // the last few words of the value region
        const uint32_t* vv = v;
        for (int i = 0; i < 8; ++i) o[i] = ((mb >> i) & 1u) ? *vv++ : 0u;
      }
      v += pc;
    }
  }
  if (stream) _mm_sfence();
  scalar_from(mask, v, out, n, full);
}
#endif

std::atomic<int> g_forced{kAuto};

int best_variant() {
#if TFA_UNPACK_X86
  static const int best = [] {
    if (__builtin_cpu_supports("avx512f") && __builtin_cpu_supports("popcnt")) return static_cast<int>(kAvx512);
    if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("popcnt")) return static_cast<int>(kAvx2);
    return static_cast<int>(kScalar);
  }();
  return best;
#else
  return kScalar;
#endif
}

TileFn tile_fn(int v) {
#if TFA_UNPACK_X86
  if (v == kAvx512) return tile_avx512;
  if (v == kAvx2) return tile_avx2;
#endif
  (void)v;
  return tile_scalar;
}

}  // namespace

bool variant_available(int v) {
  if (v == kScalar || v == kAuto) return true;
#if TFA_UNPACK_X86
  if (v == kAvx2) return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("popcnt");
  if (v == kAvx512) return __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("popcnt");
#endif
  return false;
}

void force_variant(int v) {
  if (v < kAuto || v > kAvx512 || !variant_available(v))
    throw std::runtime_error("unpack: variant " + std::to_string(v) + " is not available on this CPU");
  g_forced.store(v);
}

int current_variant() {
  const int f = g_forced.load();
  return f == kAuto ? best_variant() : f;
}

void unpack_words(const uint64_t* header, const uint32_t* mask, const uint32_t* values, uint32_t* out,
                  int64_t rows, int64_t wpr, int64_t tile_begin, int64_t tile_end) {
  const int64_t tiles = (rows + kPackTileRows - 1) / kPackTileRows;
  if (tile_begin < 0 || tile_end > tiles || tile_begin > tile_end)
    throw std::runtime_error("unpack: tile range out of bounds");
  const TileFn fn = tile_fn(current_variant());
  const uint64_t total = header[0];
  for (int64_t t = tile_begin; t < tile_end; ++t) {
    const int64_t r0 = t * kPackTileRows, r1 = std::min<int64_t>(rows, r0 + kPackTileRows);
    const int64_t e0 = r0 * wpr, n = (r1 - r0) * wpr;
    const uint64_t off = header[1 + 2 * t], cnt = header[2 + 2 * t];
    const uint32_t* m = mask + e0 / 32;  // e0 is a multiple of 32
    // the mask decides how many values the expansion reads: it has to agree
    // with the header before anything is read through it
    uint64_t bits = 0;
    for (int64_t j = 0; j * 32 < n; ++j) bits += __builtin_popcount(m[j] & tail_bits(n - j * 32));
    if (bits != cnt || off > total || cnt > total - off)
      throw std::runtime_error("unpack: tile " + std::to_string(t) + ": header {" + std::to_string(off) + ", " +
                               std::to_string(cnt) + "} against a mask of " + std::to_string(bits) + " words and " +
                               std::to_string(total) + " values");
    fn(m, values + off, values + total, out + e0, n);
  }
}

// ------------------------------------------------------------------ pool

void Job::wait() {
  std::unique_lock<std::mutex> lk(mu_);
  cv_.wait(lk, [&] { return pending_ == 0; });
  if (error_) {
    std::exception_ptr e = error_;
    error_ = nullptr;
    std::rethrow_exception(e);
  }
}

bool Job::done() {
  std::lock_guard<std::mutex> lk(mu_);
  return pending_ == 0;
}

Pool::Pool(int threads) {
  threads = std::max(1, threads);
  workers_.reserve(threads);
  for (int i = 0; i < threads; ++i) workers_.emplace_back([this] { worker(); });
}

Pool::~Pool() {
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  for (auto& w : workers_) w.join();
}

void Pool::worker() {
  for (;;) {
    std::function<void()> task;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
      if (q_.empty()) return;  // stop_ and drained
      task = std::move(q_.front());
      q_.pop_front();
    }
    task();
  }
}

std::shared_ptr<Job> Pool::post(int parts, std::function<void(int)> fn) {
  auto job = std::make_shared<Job>();
  if (parts <= 0) return job;
  job->pending_ = parts;
  auto shared_fn = std::make_shared<std::function<void(int)>>(std::move(fn));
  {
    std::lock_guard<std::mutex> lk(mu_);
    for (int p = 0; p < parts; ++p)
      q_.emplace_back([job, shared_fn, p] {
        std::exception_ptr err;
        try {
          (*shared_fn)(p);
        } catch (...) {
          err = std::current_exception();
        }
        std::lock_guard<std::mutex> jl(job->mu_);
        if (err && !job->error_) job->error_ = err;
        if (--job->pending_ == 0) job->cv_.notify_all();
      });
  }
  cv_.notify_all();
  return job;
}

std::shared_ptr<Job> Pool::post_unpack(const void* packed, void* out, int64_t rows, int64_t wpr) {
  const int64_t tiles = (rows + kPackTileRows - 1) / kPackTileRows;
  const int parts = static_cast<int>(std::min<int64_t>(threads(), tiles));
  return post(parts, [=](int p) {
    unpack_buffer(packed, out, rows, wpr, tiles * p / parts, tiles * (p + 1) / parts);
  });
}

int default_threads() {
  if (const char* e = std::getenv("TFA_UNPACK_THREADS")) {
    const int n = std::atoi(e);
    if (n > 0) return std::min(n, 64);
  }
  int budget = 0;
  if (const char* e = std::getenv("OMP_NUM_THREADS")) budget = std::atoi(e);
#if defined(__linux__)
  if (budget <= 0) {
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) budget = CPU_COUNT(&set);
  }
#endif
  if (budget <= 0) budget = 4;
  return std::max(1, std::min(12, budget - 2));
}

namespace {
std::mutex g_pool_mu;
std::unique_ptr<Pool> g_pool;
}  // namespace

Pool& global_pool() {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  if (!g_pool) g_pool = std::make_unique<Pool>(default_threads());
  return *g_pool;
}

void shutdown_pool() {
  std::unique_ptr<Pool> p;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    p = std::move(g_pool);
  }
  p.reset();
}

}  // namespace unpack
}  // namespace tfa
