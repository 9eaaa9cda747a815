// The per-dtype vocabulary of the analytics kernels (stats.hip,
// group_stats.hip, window_scan.hip, join.hip): the seven column dtypes in one
// switch, the store of a word (sort_words.h) back as its column's type, and the
// small bit and index helpers. One definition each: what these kernels compute
// must stay bit-identical across the features built on them.
#pragma once

#include <cstdint>

#include "hip_common.h"
#include "sort_words.h"

namespace tfa {
namespace k {

// the dtypes a statistics / window value column may have
__host__ __device__ __forceinline__ bool is_stat_dtype(DType d) {
  return d == DType::F32 || d == DType::F64 || d == DType::I64 || d == DType::I32 || d == DType::I16 ||
         d == DType::I8 || d == DType::U8;
}

__host__ __device__ __forceinline__ bool is_float_dtype(DType d) { return d == DType::F32 || d == DType::F64; }

// f(T{}) for the element type T of a column of dtype dt (is_stat_dtype), e.g.
//   r = dispatch_column(dt, [&](auto tag) { return lane_rows<decltype(tag)>(...); });
// dt is uniform wherever the kernels use this: one scalar branch.
template <typename F>
__device__ __forceinline__ auto dispatch_column(DType dt, F&& f) {
  switch (dt) {
    case DType::F32: return f(float{});
    case DType::F64: return f(double{});
    case DType::I64: return f(int64_t{});
    case DType::I32: return f(int32_t{});
    case DType::I16: return f(int16_t{});
    case DType::I8: return f(int8_t{});
    default: return f(uint8_t{});  // U8
  }
}

// out[i] = the value word w came from, out a column of dtype dt (floats as
// their bits: -0.0 comes back as 0.0, every NaN as the quiet NaN). The caller
// may have no word to store (`has` false): zero takes its place
__device__ __forceinline__ void store_word(void* out, int64_t i, DType dt, uint64_t w, bool has = true) {
  switch (dt) {
    case DType::F32: static_cast<uint32_t*>(out)[i] = has ? decode_f32(w) : 0u; break;
    case DType::F64: static_cast<uint64_t*>(out)[i] = has ? decode_f64(w) : 0ull; break;
    case DType::I64: static_cast<int64_t*>(out)[i] = has ? decode_int(w) : 0; break;
    case DType::I32: static_cast<int32_t*>(out)[i] = has ? static_cast<int32_t>(decode_int(w)) : 0; break;
    case DType::I16: static_cast<int16_t*>(out)[i] = has ? static_cast<int16_t>(decode_int(w)) : 0; break;
    case DType::I8: static_cast<int8_t*>(out)[i] = has ? static_cast<int8_t>(decode_int(w)) : 0; break;
    default: static_cast<uint8_t*>(out)[i] = has ? static_cast<uint8_t>(w) : 0; break;  // U8
  }
}

__device__ __forceinline__ uint64_t f64_bits(double x) { return static_cast<uint64_t>(__double_as_longlong(x)); }
__device__ __forceinline__ double bits_f64(uint64_t b) { return __longlong_as_double(static_cast<long long>(b)); }

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the last i in [a, b] with p[i - base] <= j (p[a - base] <= j is given)
__device__ __forceinline__ int64_t last_not_above(const int64_t* p, int64_t base, int64_t a, int64_t b, int64_t j) {
  while (a < b) {
    const int64_t mid = a + (b - a + 1) / 2;
    if (p[mid - base] <= j) a = mid;
    else b = mid - 1;
  }
  return a;
}

// host: column c of a set (`what`: the caller, `item`: "column" / "channel")
// has a supported dtype, data unless there are no rows, and an aligned pointer
inline void check_stat_column(const char* what, const char* item, int c, DType dtype, const void* ptr, int64_t n) {
  TFA_CHECK(is_stat_dtype(dtype), what, ": ", item, " ", c, " has a dtype that is not supported");
  TFA_CHECK(n == 0 || ptr != nullptr, what, ": ", item, " ", c, " has no data");
  TFA_CHECK(reinterpret_cast<uintptr_t>(ptr) % static_cast<uintptr_t>(dtype_size(dtype)) == 0, what, ": ", item, " ",
            c, " is not aligned to its element size");
}

inline void check_stat_columns(const char* what, const StatCols& cols, int64_t n) {
  for (int c = 0; c < cols.n; ++c) check_stat_column(what, "column", c, cols.dtype[c], cols.ptr[c], n);
}

}  // namespace k
}  // namespace tfa
