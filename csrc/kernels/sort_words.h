// The order-preserving 64-bit word of one scalar (the table in kernels.h, sort
// section; ascending): the one definition that sort.hip, stats.hip,
// group_stats.hip and window_scan.hip encode with, and that column_types.h
// decodes with.
#pragma once

#include <cstdint>

#include "hip_common.h"

namespace tfa {
namespace k {

constexpr uint64_t kSign64 = 0x8000000000000000ull;

__device__ __forceinline__ uint64_t encode_f32(uint32_t b) {
  if ((b & 0x7fffffffu) > 0x7f800000u) b = 0x7fc00000u;  // every NaN: the canonical quiet NaN
  if (b == 0x80000000u) b = 0u;                          // -0.0 == +0.0
  return (b & 0x80000000u) ? static_cast<uint32_t>(~b) : (b | 0x80000000u);
}

__device__ __forceinline__ uint64_t encode_f64(uint64_t b) {
  if ((b & ~kSign64) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
  if (b == kSign64) b = 0ull;
  return (b & kSign64) ? ~b : (b | kSign64);
}

template <typename T>
__device__ __forceinline__ uint64_t encode_int(T v) {
  return static_cast<uint64_t>(static_cast<int64_t>(v)) ^ kSign64;
}

// the inverses: the bits (the value, for the integers) a word came from. Words
// canonicalise, so -0.0 comes back as 0.0 and every NaN as the quiet NaN
__device__ __forceinline__ uint32_t decode_f32(uint64_t w) {
  const uint32_t e = static_cast<uint32_t>(w);
  return (e & 0x80000000u) ? (e ^ 0x80000000u) : ~e;
}

__device__ __forceinline__ uint64_t decode_f64(uint64_t w) { return (w & kSign64) ? (w ^ kSign64) : ~w; }

__device__ __forceinline__ int64_t decode_int(uint64_t w) { return static_cast<int64_t>(w ^ kSign64); }

// the word of a typed value (BOOL / U8: the value)
__device__ __forceinline__ uint64_t sort_word(float v) { return encode_f32(__float_as_uint(v)); }
__device__ __forceinline__ uint64_t sort_word(double v) {
  return encode_f64(static_cast<uint64_t>(__double_as_longlong(v)));
}
__device__ __forceinline__ uint64_t sort_word(int64_t v) { return encode_int(v); }
__device__ __forceinline__ uint64_t sort_word(int32_t v) { return encode_int(v); }
__device__ __forceinline__ uint64_t sort_word(int16_t v) { return encode_int(v); }
__device__ __forceinline__ uint64_t sort_word(int8_t v) { return encode_int(v); }
__device__ __forceinline__ uint64_t sort_word(uint8_t v) { return static_cast<uint64_t>(v); }

}  // namespace k
}  // namespace tfa
