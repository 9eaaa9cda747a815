// Go/no-go probe for packing sparse pipeline outputs before the D2H copy
// (docs/PERFORMANCE.md, "Packed D2H: step 0"). No pipeline code involved: it
// replays the copy pattern of one bench.py step (153 chunks of 128 MiB in)
// with pinned DMA on two streams and measures
//   1. H2D 128 MiB beside D2H 128 MiB (today's traffic) and beside D2H of a
//      packed chunk (mask + non-zero words of a ~50 % zero chunk);
//   2. the same with N host threads expanding every landed packed chunk into
//      a second pinned buffer (runtime/unpack.cpp), staging slots reused only
//      after their expansion finished.
// Prints one JSON object per case.
//
//   hipcc -O3 --offload-arch=gfx950 -I csrc scripts/pack_d2h_probe.hip \
//       csrc/runtime/unpack.cpp -o labbin/pack_d2h_probe -lpthread
//   labbin/pack_d2h_probe [chunks=153] [zero_percent=50]
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "runtime/unpack.h"

#define CK(x)                                                                                   \
  do {                                                                                          \
    hipError_t e_ = (x);                                                                        \
    if (e_ != hipSuccess) {                                                                     \
      std::fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      std::exit(1);                                                                             \
    }                                                                                           \
  } while (0)

using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

// host reference packer (tiles in order); returns the packed byte count
static size_t pack_host(const uint32_t* dense, int64_t rows, int64_t wpr, char* packed) {
  const tfa::PackLayout L = tfa::pack_layout(rows, wpr);
  uint64_t* hdr = reinterpret_cast<uint64_t*>(packed);
  uint32_t* mask = reinterpret_cast<uint32_t*>(packed + L.mask_off);
  uint32_t* val = reinterpret_cast<uint32_t*>(packed + L.values_off);
  std::memset(packed, 0, L.values_off);
  uint64_t total = 0;
  for (int64_t t = 0; t < L.tiles; ++t) {
    const int64_t e0 = t * tfa::kPackTileRows * wpr;
    const int64_t e1 = std::min<int64_t>(rows, (t + 1) * tfa::kPackTileRows) * wpr;
    hdr[1 + 2 * t] = total;
    for (int64_t e = e0; e < e1; ++e)
      if (dense[e]) {
        mask[e >> 5] |= 1u << (e & 31);
        val[total++] = dense[e];
      }
    hdr[2 + 2 * t] = total - hdr[1 + 2 * t];
  }
  hdr[0] = total;
  return L.values_off + total * 4;
}

int main(int argc, char** argv) {
  const int chunks = argc > 1 ? std::atoi(argv[1]) : 153;
  const int zero_pct = argc > 2 ? std::atoi(argv[2]) : 50;
  const int64_t rows = 65536, wpr = 512;
  const size_t dense_bytes = static_cast<size_t>(rows) * wpr * 4;  // 128 MiB
  const tfa::PackLayout L = tfa::pack_layout(rows, wpr);
  constexpr int kIn = 4, kStage = 3, kOut = 8;

  char *h_in[kIn], *h_stage[kStage], *h_out[kOut], *d_in[kStage], *d_packed, *d_dense;
  for (auto& p : h_in) {
    CK(hipHostMalloc(reinterpret_cast<void**>(&p), dense_bytes, hipHostMallocDefault));
    std::memset(p, 1, dense_bytes);
  }
  for (auto& p : h_stage) {
    CK(hipHostMalloc(reinterpret_cast<void**>(&p), L.max_bytes, hipHostMallocDefault));
    std::memset(p, 0, L.max_bytes);
  }
  for (auto& p : h_out) {
    CK(hipHostMalloc(reinterpret_cast<void**>(&p), dense_bytes, hipHostMallocDefault));
    std::memset(p, 2, dense_bytes);
  }
  for (auto& p : d_in) CK(hipMalloc(reinterpret_cast<void**>(&p), dense_bytes));
  CK(hipMalloc(reinterpret_cast<void**>(&d_packed), L.max_bytes));
  CK(hipMalloc(reinterpret_cast<void**>(&d_dense), dense_bytes));

  // a relu-like chunk: zero_pct % of the words are zero
  std::vector<uint32_t> dense(static_cast<size_t>(rows) * wpr);
  {
    std::mt19937 rng(1);
    for (auto& w : dense) w = (rng() % 100u) < static_cast<uint32_t>(zero_pct) ? 0u : (rng() | 1u);
  }
  std::vector<char> packed(L.max_bytes);
  const size_t packed_bytes = pack_host(dense.data(), rows, wpr, packed.data());
  CK(hipMemcpy(d_packed, packed.data(), packed_bytes, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_dense, dense.data(), dense_bytes, hipMemcpyHostToDevice));
  std::printf("{\"case\": \"setup\", \"chunks\": %d, \"dense_MiB\": %.1f, \"packed_MiB\": %.1f, \"packed_fraction\": %.4f, "
              "\"unpack_variant\": %d}\n",
              chunks, dense_bytes / 1048576.0, packed_bytes / 1048576.0, double(packed_bytes) / dense_bytes,
              tfa::unpack::current_variant());

  hipStream_t s_h2d, s_d2h;
  CK(hipStreamCreateWithFlags(&s_h2d, hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&s_d2h, hipStreamNonBlocking));
  hipEvent_t h0, h1;
  CK(hipEventCreate(&h0));
  CK(hipEventCreate(&h1));
  std::vector<hipEvent_t> ev(chunks);
  for (auto& e : ev) CK(hipEventCreateWithFlags(&e, hipEventDisableTiming));

  // threads == 0: copies only. d2h_bytes: what one D2H moves.
  auto run = [&](const char* name, const char* d2h_src, size_t d2h_bytes, int threads) {
    std::unique_ptr<tfa::unpack::Pool> pool;
    if (threads > 0) pool = std::make_unique<tfa::unpack::Pool>(threads);
    double best_wall = 1e30, best_h2d = 0, best_expand = 0;
    for (int rep = 0; rep < 3; ++rep) {  // rep 0 warms up
      CK(hipDeviceSynchronize());
      std::vector<std::shared_ptr<tfa::unpack::Job>> job(kStage);
      double expand_wait_ms = 0;
      const auto t0 = Clock::now();
      CK(hipEventRecord(h0, s_h2d));
      for (int c = 0; c < chunks; ++c)
        CK(hipMemcpyAsync(d_in[c % kStage], h_in[c % kIn], dense_bytes, hipMemcpyHostToDevice, s_h2d));
      CK(hipEventRecord(h1, s_h2d));
      // D2H runs one chunk ahead of the expansion: chunk c is enqueued, then
      // chunk c-1 is waited for and handed to the pool
      for (int c = 0; c <= chunks; ++c) {
        if (c < chunks) {
          if (job[c % kStage]) {  // the slot's last expansion
            const auto w0 = Clock::now();
            job[c % kStage]->wait();
            expand_wait_ms += ms_since(w0);
          }
          CK(hipMemcpyAsync(h_stage[c % kStage], d2h_src, d2h_bytes, hipMemcpyDeviceToHost, s_d2h));
          CK(hipEventRecord(ev[c], s_d2h));
        }
        if (c > 0 && pool) {
          CK(hipEventSynchronize(ev[c - 1]));
          job[(c - 1) % kStage] = pool->post_unpack(h_stage[(c - 1) % kStage], h_out[(c - 1) % kOut], rows, wpr);
        }
      }
      CK(hipStreamSynchronize(s_d2h));
      const double copies_ms = ms_since(t0);
      for (auto& j : job)
        if (j) j->wait();
      CK(hipStreamSynchronize(s_h2d));
      const double wall = ms_since(t0);
      float h2d_ms = 0;
      CK(hipEventElapsedTime(&h2d_ms, h0, h1));
      if (rep > 0 && wall < best_wall) {
        best_wall = wall;
        best_h2d = double(chunks) * dense_bytes / 1e9 / (h2d_ms / 1e3);
        best_expand = threads > 0 ? double(chunks) * dense_bytes / 1e9 / (wall / 1e3) : 0;
      }
      std::printf("{\"case\": \"%s\", \"rep\": %d, \"threads\": %d, \"d2h_MiB\": %.1f, \"wall_ms\": %.1f, "
                  "\"copies_done_ms\": %.1f, \"h2d_ms\": %.1f, \"h2d_GBps\": %.2f, \"slot_wait_ms\": %.1f}\n",
                  name, rep, threads, d2h_bytes / 1048576.0, wall, copies_ms, h2d_ms,
                  double(chunks) * dense_bytes / 1e9 / (h2d_ms / 1e3), expand_wait_ms);
      std::fflush(stdout);
    }
    std::printf("{\"case\": \"%s\", \"best\": true, \"threads\": %d, \"wall_ms\": %.1f, \"h2d_GBps\": %.2f, "
                "\"dense_written_GBps\": %.2f}\n",
                name, threads, best_wall, best_h2d, best_expand);
    if (pool && std::memcmp(h_out[(chunks - 1) % kOut], dense.data(), dense_bytes) != 0) {
      std::fprintf(stderr, "expansion mismatch in case %s\n", name);
      std::exit(2);
    }
  };

  run("dense_128_128", d_dense, dense_bytes, 0);
  run("packed_copy_only", d_packed, packed_bytes, 0);
  for (int n : {4, 8, 12}) run("packed_expand", d_packed, packed_bytes, n);
  run("dense_128_128_again", d_dense, dense_bytes, 0);

  // the expansion alone, no DMA beside it
  for (int n : {4, 8, 12}) {
    tfa::unpack::Pool pool(n);
    std::memcpy(h_stage[0], packed.data(), packed_bytes);
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
      const auto t0 = Clock::now();
      for (int c = 0; c < 16; ++c) pool.post_unpack(h_stage[0], h_out[c % kOut], rows, wpr)->wait();
      best = std::min(best, ms_since(t0));
    }
    std::printf("{\"case\": \"expand_alone\", \"threads\": %d, \"dense_written_GBps\": %.2f}\n", n,
                16.0 * dense_bytes / 1e9 / (best / 1e3));
  }
  return 0;
}
