// records.hpp -- the compact per-triangle record: ONE 64-bit word per triangle and view where TriFrag (common.hpp) takes sixteen
// bytes.  The only place that knows the layout; plain C++, host and device (tests/records_driver.cpp compiles it with the host
// compiler under sanitizers).
//
//   bits  0 .. 35   mask of a box of at most 6 x 6 pixels, bit dx * 6 + dy -- ascending bits are the pixel order of TriFrag's
//                   dx * 8 + dy (x, then y), so a walk over set bits makes the same additions in the same order
//   bits 36 .. 48   x0        bits 49 .. 61   y0      (images of at most 8 192 x 8 192: rec_image_fits)
//   bits 62 .. 63   kind:  0 nothing emitted
//                          1 small (box <= 6 x 6): the word is the whole record
//                          2 TriFrag's kind 2 (box over 8 x 8, near-plane crossing)
//                          3 small, but 7 or 8 pixels in x or y
//                   kinds 2 and 3: the full TriFrag (kind 2, or kind 1 with its 64-bit mask) lies in the SECOND plane of the same
//                   allocation, rec_full_offset(F) bytes behind the words; the word only says "look there".
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SMESH_REC_HD __host__ __device__ inline
#else
#define SMESH_REC_HD inline
#endif

namespace smesh {

constexpr int kRecBox = 6;                 // pixels per side the mask of a word covers
constexpr uint32_t kRecMaxImage = 8192;    // x0, y0 have 13 bits
constexpr uint64_t kRecMask36 = (1ull << 36) - 1ull;

// May a W x H view leave compact records?
SMESH_REC_HD bool rec_image_fits(uint64_t W, uint64_t H) { return W <= kRecMaxImage && H <= kRecMaxImage; }

// Bytes from the start of a view's record allocation to its plane of full TriFrag records (16-byte records, 256-byte aligned),
// and the size of the allocation that holds both planes.
SMESH_REC_HD uint64_t rec_full_offset(uint64_t F) { return (F * 8ull + 255ull) & ~255ull; }
SMESH_REC_HD uint64_t rec_alloc_bytes(uint64_t F) { return rec_full_offset(F) + F * 16ull; }

// The compact kind of a triangle whose TriFrag kind is `kind16` (0, 1, 2) and whose box measures bw x bh pixels.
SMESH_REC_HD uint32_t rec_kind_of(uint32_t kind16, int bw, int bh) {
  if (kind16 != 1u) return kind16;
  return (bw > kRecBox || bh > kRecBox) ? 3u : 1u;
}

// TriFrag's mask (bit dx * 8 + dy) of a box of at most 6 x 6 <-> the word's (bit dx * 6 + dy): three columns per 32-bit half.
SMESH_REC_HD uint64_t rec_mask36(uint64_t m64) {
  const uint32_t lo = (uint32_t)m64 & 0x00FFFFFFu, hi = (uint32_t)(m64 >> 24) & 0x00FFFFFFu;
  const uint32_t a = (lo & 0x3Fu) | ((lo >> 2) & 0xFC0u) | ((lo >> 4) & 0x3F000u);
  const uint32_t b = (hi & 0x3Fu) | ((hi >> 2) & 0xFC0u) | ((hi >> 4) & 0x3F000u);
  return (uint64_t)a | ((uint64_t)b << 18);
}
SMESH_REC_HD uint64_t rec_mask64(uint64_t m36) {
  const uint32_t a = (uint32_t)m36 & 0x3FFFFu, b = (uint32_t)(m36 >> 18) & 0x3FFFFu;
  const uint32_t lo = (a & 0x3Fu) | ((a & 0xFC0u) << 2) | ((a & 0x3F000u) << 4);
  const uint32_t hi = (b & 0x3Fu) | ((b & 0xFC0u) << 2) | ((b & 0x3F000u) << 4);
  return (uint64_t)lo | ((uint64_t)hi << 24);
}

// `mask64`: TriFrag's mask; kept only for kind 1 (the other kinds' words carry no mask).
SMESH_REC_HD uint64_t rec_pack(uint32_t x0, uint32_t y0, uint32_t kind, uint64_t mask64) {
  return (kind == 1u ? rec_mask36(mask64) : 0ull) | ((uint64_t)(x0 & 0x1FFFu) << 36) | ((uint64_t)(y0 & 0x1FFFu) << 49) | ((uint64_t)(kind & 3u) << 62);
}
SMESH_REC_HD uint32_t rec_kind(uint64_t w) { return (uint32_t)(w >> 62); }
SMESH_REC_HD uint32_t rec_x0(uint64_t w) { return (uint32_t)(w >> 36) & 0x1FFFu; }
SMESH_REC_HD uint32_t rec_y0(uint64_t w) { return (uint32_t)(w >> 49) & 0x1FFFu; }
SMESH_REC_HD uint64_t rec_word_mask64(uint64_t w) { return rec_mask64(w & kRecMask36); }

// The bit of a kind-1 word that stands for pixel (x0 + dx, y0 + dy): what the tile resolve clears for a fragment that lost.
SMESH_REC_HD int rec_bit(int dx, int dy) { return dx * kRecBox + dy; }

}  // namespace smesh
