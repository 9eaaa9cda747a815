// Stand-alone check of csrc/runtime/unpack.cpp for host sanitizer builds
// (tests/test_unpack_words.py compiles it with unpack.cpp under
// -fsanitize=address,undefined and -fsanitize=thread and runs it):
// every available variant over the shapes and contents of the Python test,
// exact-size buffers (so a read or write past an end is caught), a
// multi-threaded pool run with several chunks in flight, and a worker that
// throws.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "runtime/unpack.h"

using namespace tfa;

static int g_failures = 0;
#define EXPECT(cond, ...)                  \
  do {                                     \
    if (!(cond)) {                         \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);            \
      std::printf("\n");                   \
      ++g_failures;                        \
    }                                      \
  } while (0)

// packed buffer of exactly values_off + 4 * total bytes; tiles placed in a
// shuffled order when `shuffle`
static std::vector<char> pack(const std::vector<uint32_t>& w, int64_t rows, int64_t wpr, bool shuffle,
                                  std::mt19937& rng) {
  const PackLayout L = pack_layout(rows, wpr);
  std::vector<int64_t> order(L.tiles);
  for (int64_t t = 0; t < L.tiles; ++t) order[t] = t;
  if (shuffle) std::shuffle(order.begin(), order.end(), rng);
  std::vector<uint64_t> cnt(L.tiles, 0), off(L.tiles, 0);
  for (int64_t t = 0; t < L.tiles; ++t) {
    const int64_t e0 = t * kPackTileRows * wpr, e1 = std::min<int64_t>(rows, (t + 1) * kPackTileRows) * wpr;
    for (int64_t e = e0; e < e1; ++e) cnt[t] += w[e] != 0;
  }
  uint64_t total = 0;
  for (int64_t t : order) {
    off[t] = total;
    total += cnt[t];
  }
  std::vector<char> buf(L.values_off + total * 4, 0);  // exact: heap storage is 16-byte aligned
  char* p = buf.data();
  uint64_t* hdr = reinterpret_cast<uint64_t*>(p);
  uint32_t* mask = reinterpret_cast<uint32_t*>(p + L.mask_off);
  uint32_t* val = reinterpret_cast<uint32_t*>(p + L.values_off);
  hdr[0] = total;
  for (int64_t t = 0; t < L.tiles; ++t) {
    hdr[1 + 2 * t] = off[t];
    hdr[2 + 2 * t] = cnt[t];
    const int64_t e0 = t * kPackTileRows * wpr, e1 = std::min<int64_t>(rows, (t + 1) * kPackTileRows) * wpr;
    uint64_t k = off[t];
    for (int64_t e = e0; e < e1; ++e)
      if (w[e]) {
        mask[e >> 5] |= 1u << (e & 31);
        val[k++] = w[e];
      }
  }
  return buf;
}

static std::vector<uint32_t> make(int kind, int64_t n, std::mt19937& rng) {
  std::vector<uint32_t> w(n);
  const uint32_t special[] = {0x80000000u, 0x7fc00000u, 0x7f800000u, 0xff800000u, 0x00000001u};
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t r = rng();
    switch (kind) {
      case 0: w[i] = 0; break;
      case 1: w[i] = r | 1u; break;
      case 2: w[i] = (r & 1u) ? (r | 2u) : 0u; break;
      case 3: w[i] = (r % 7u == 0) ? special[r % 5u] : ((r & 1u) ? 0u : (0x3f800000u | (r >> 9))); break;
      default: w[i] = static_cast<uint32_t>(static_cast<int32_t>(r % 7u) - 3); break;
    }
  }
  return w;
}

int main() {
  std::mt19937 rng(7);
  const int64_t T = kPackTileRows;
  const int64_t rows_list[] = {1, T - 1, T, T + 1, 3 * T + 7};
  const int64_t wpr_list[] = {1, 15, 16, 17, 31, 32, 33, 512};
  int variants = 0;
  for (int v = 0; v <= 2; ++v) {
    if (!unpack::variant_available(v)) {
      std::printf("variant %d: not on this CPU\n", v);
      continue;
    }
    ++variants;
    unpack::force_variant(v);
    for (int kind = 0; kind < 5; ++kind)
      for (int64_t rows : rows_list)
        for (int64_t wpr : wpr_list)
          for (int mis = 0; mis < 2; ++mis) {
            const int64_t n = rows * wpr;
            const auto w = make(kind, n, rng);
            const auto packed = pack(w, rows, wpr, mis == 1, rng);
            // exact-size output, 64-byte aligned or 4 bytes past it
            void* raw = nullptr;
            if (posix_memalign(&raw, 64, static_cast<size_t>(n) * 4 + 64) != 0) return 3;
            uint32_t* out = reinterpret_cast<uint32_t*>(static_cast<char*>(raw) + (mis ? 4 : 0));
            std::memset(raw, 0xAB, static_cast<size_t>(n) * 4 + 64);
            unpack::unpack_buffer(packed.data(), out, rows, wpr, 0, pack_layout(rows, wpr).tiles);
            EXPECT(std::memcmp(out, w.data(), static_cast<size_t>(n) * 4) == 0,
                   "variant %d kind %d %lldx%lld mis %d", v, kind, (long long)rows, (long long)wpr, mis);
            // nothing written past the end
            const unsigned char* tail = reinterpret_cast<unsigned char*>(out + n);
            EXPECT(tail[0] == 0xAB && tail[3] == 0xAB, "variant %d wrote past the end", v);
            std::free(raw);
          }
    // a pool with several chunks in flight, each split over the workers
    for (int threads : {1, 3, 8}) {
      unpack::Pool pool(threads);
      const int64_t rows = 9 * T + 7, wpr = 512, n = rows * wpr;
      std::vector<std::vector<uint32_t>> src, dst;
      std::vector<std::vector<char>> pk;
      std::vector<std::shared_ptr<unpack::Job>> jobs;
      for (int c = 0; c < 4; ++c) {
        src.push_back(make(2 + c % 2, n, rng));
        pk.push_back(pack(src.back(), rows, wpr, true, rng));
        dst.emplace_back(n, 0xABABABABu);
      }
      for (int c = 0; c < 4; ++c) jobs.push_back(pool.post_unpack(pk[c].data(), dst[c].data(), rows, wpr));
      for (int c = 0; c < 4; ++c) {
        jobs[c]->wait();
        EXPECT(dst[c] == src[c], "pool of %d threads, chunk %d", threads, c);
      }
      // a worker that throws: the waiter sees it, the pool lives on
      bool caught = false;
      try {
        pool.post(8, [](int p) {
          if (p == 5) throw std::runtime_error("part 5");
        })->wait();
      } catch (const std::runtime_error& e) {
        caught = std::string(e.what()) == "part 5";
      }
      EXPECT(caught, "worker exception lost (%d threads)", threads);
      pool.post(3, [](int) {})->wait();
    }
    // a header that disagrees with the mask is refused before anything is read through it
    {
      const int64_t rows = T + 1, wpr = 32;
      const auto w = make(2, rows * wpr, rng);
      auto packed = pack(w, rows, wpr, false, rng);
      reinterpret_cast<uint64_t*>(packed.data())[2] -= 1;
      std::vector<uint32_t> out(rows * wpr);
      bool caught = false;
      try {
        unpack::unpack_buffer(packed.data(), out.data(), rows, wpr, 0, 2);
      } catch (const std::runtime_error&) {
        caught = true;
      }
      EXPECT(caught, "inconsistent header accepted");
    }
  }
  unpack::force_variant(unpack::kAuto);
  // the process-wide pool: lazily made, joined by shutdown_pool
  {
    const int64_t rows = 5 * T, wpr = 64;
    const auto w = make(2, rows * wpr, rng);
    const auto packed = pack(w, rows, wpr, true, rng);
    std::vector<uint32_t> out(rows * wpr, 1u);
    unpack::global_pool().post_unpack(packed.data(), out.data(), rows, wpr)->wait();
    EXPECT(out == w, "global pool");
    unpack::shutdown_pool();
  }
  if (g_failures || !variants) {
    std::printf("unpack_main: %d failures\n", g_failures);
    return 1;
  }
  std::printf("unpack_main: ok (%d variants)\n", variants);
  return 0;
}
