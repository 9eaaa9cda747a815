// Wire format of a zero-word-packed buffer (pack_words.hip writes it on the
// device, runtime/unpack.cpp expands it on the host). Plain C++: no HIP, no
// ATen.
//
// A buffer of rows x wpr 32-bit words is cut into tiles of kPackTileRows rows
// (the last one may be short). A word is dropped only if its bit pattern is
// 0x00000000. The packed buffer is, in order:
//
//   header  uint64[1 + 2 * tiles]   [0] total value words, then per tile
//                                   {value offset, value count} in words
//   mask    uint32[ceil(rows*wpr/32)]   bit i of word j is element 32*j + i
//                                   (row-major over the whole buffer)
//   values  uint32[total]           each tile's non-zero words in element
//                                   order; tiles in arbitrary order
//
// header and mask are each padded to a multiple of 64 bytes, so the value
// region starts 64-byte aligned. kPackTileRows is a multiple of 32, so every
// tile starts on a mask word boundary whatever wpr is.
#pragma once

#include <cstddef>
#include <cstdint>

namespace tfa {

constexpr int kPackTileRows = 32;

struct PackLayout {
  int64_t rows = 0, wpr = 0;
  int64_t tiles = 0;
  int64_t mask_words = 0;
  size_t mask_off = 0;    // bytes from the start of the buffer
  size_t values_off = 0;  // bytes from the start of the buffer
  size_t max_bytes = 0;   // values_off + 4 * rows * wpr: nothing dropped
};

inline PackLayout pack_layout(int64_t rows, int64_t wpr) {
  PackLayout L;
  L.rows = rows;
  L.wpr = wpr;
  L.tiles = (rows + kPackTileRows - 1) / kPackTileRows;
  L.mask_words = (rows * wpr + 31) / 32;
  const size_t hdr = (static_cast<size_t>(1 + 2 * L.tiles) * 8 + 63) / 64 * 64;
  const size_t msk = (static_cast<size_t>(L.mask_words) * 4 + 63) / 64 * 64;
  L.mask_off = hdr;
  L.values_off = hdr + msk;
  L.max_bytes = L.values_off + static_cast<size_t>(rows) * static_cast<size_t>(wpr) * 4;
  return L;
}

}  // namespace tfa
