// Host side of zero-word packing (see kernels/pack_layout.h for the format):
// expansion of a packed buffer into its dense form, and a small worker pool
// that splits one buffer by tile ranges. Pure C++17: no HIP, no ATen.
#pragma once

#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../kernels/pack_layout.h"

namespace tfa {
namespace unpack {

enum Variant : int { kAuto = -1, kScalar = 0, kAvx2 = 1, kAvx512 = 2 };

// compiled in and supported by this CPU
bool variant_available(int v);
// test hook: kAuto picks the best available variant (the default); forcing a
// variant the CPU lacks throws
void force_variant(int v);
// the variant unpack_words runs now
int current_variant();

// Expands tiles [tile_begin, tile_end) of a packed rows x wpr buffer into
// `out` (the dense buffer's base, not the tile's). Every word of those tiles
// is written, zeros included. Throws std::runtime_error when the header and
// the mask disagree (a tile's count is not its mask's popcount, or its value
// range leaves [0, total)).
void unpack_words(const uint64_t* header, const uint32_t* mask, const uint32_t* values, uint32_t* out,
                  int64_t rows, int64_t wpr, int64_t tile_begin, int64_t tile_end);

// Whole packed buffer laid out by pack_layout(rows, wpr).
inline void unpack_buffer(const void* packed, void* out, int64_t rows, int64_t wpr, int64_t tile_begin,
                          int64_t tile_end) {
  const PackLayout L = pack_layout(rows, wpr);
  const char* p = static_cast<const char*>(packed);
  unpack_words(reinterpret_cast<const uint64_t*>(p), reinterpret_cast<const uint32_t*>(p + L.mask_off),
               reinterpret_cast<const uint32_t*>(p + L.values_off), static_cast<uint32_t*>(out), rows, wpr,
               tile_begin, tile_end);
}

// A group of tasks posted together; wait() returns when all ran and rethrows
// the first exception one of them raised.
class Job {
 public:
  void wait();
  bool done();

 private:
  friend class Pool;
  std::mutex mu_;
  std::condition_variable cv_;
  int64_t pending_ = 0;
  std::exception_ptr error_;
};

class Pool {
 public:
  explicit Pool(int threads);
  ~Pool();  // runs what is queued, then joins
  Pool(const Pool&) = delete;
  Pool& operator=(const Pool&) = delete;
  int threads() const { return static_cast<int>(workers_.size()); }

  // posts fn(part) for part in [0, parts); the tasks run on the workers
  std::shared_ptr<Job> post(int parts, std::function<void(int)> fn);
  // unpack_buffer split into one tile range per worker
  std::shared_ptr<Job> post_unpack(const void* packed, void* out, int64_t rows, int64_t wpr);

 private:
  void worker();
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
  bool stop_ = false;
  std::vector<std::thread> workers_;
};

// TFA_UNPACK_THREADS, else min(12, budget - 2) with budget = OMP_NUM_THREADS
// if set, else the calling thread's affinity count; at least 1.
int default_threads();

// The process-wide pool: created on first use (never at import), joined by
// shutdown_pool() (module teardown) or at exit.
Pool& global_pool();
void shutdown_pool();

}  // namespace unpack
}  // namespace tfa
