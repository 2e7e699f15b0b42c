// fragments.hpp -- the packed fragment-queue entry: ONE 64-bit word per queued fragment where the 10-byte format takes a 64-bit
// depth-test key ({float_bits(z), primitive}) in FragQueues::key and a 16-bit pixel-in-tile in FragQueues::pix.  The only place that
// knows the layout; plain C++, host and device (tests/fragments_driver.cpp compiles it with the host compiler under sanitizers).
//
//   bits 33 .. 63   float_bits(z), 31 bits: a queued fragment has z > 0 and finite, so its sign bit is 0
//   bits 22 .. 32   pixel inside the 32 x 64 tile, (x mod 32) * 64 + (y mod 64)
//   bits  0 .. 21   primitive id
//
// Every candidate of ONE pixel has the same pixel field, so the unsigned order of packed entries of a pixel is the order of their
// keys: nearer z first, equal z -> lower id.  The depth test of a tile (ds_min_u64 on the pixel's slot) takes them as they are.
//   null entry        all ones: what the writers store for an uncovered sample or a rejected depth.  Its z field is a NaN pattern:
//                     no fragment has it, and it lies above every other entry.
//   background(pixel) +inf in the z field, the pixel, id all ones: above every fragment of that pixel (their z is finite), below null.
//                     (Not one constant for every pixel: "the winner is still the background" is then a comparison with the entry the
//                     slot was seeded with, and lost() compares entries of one pixel among themselves.)
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SMESH_FRAG_HD __host__ __device__ inline
#else
#define SMESH_FRAG_HD inline
#endif

namespace smesh {

constexpr int kFragTileW = 32, kFragTileH = 64;              // the screen tile of a fragment queue (raster.hip: kQW, kQH)
constexpr int kFragPixelBits = 11, kFragIdBits = 22;
constexpr uint32_t kFragIdMask = (1u << kFragIdBits) - 1u;
constexpr uint32_t kFragPixelMask = (1u << kFragPixelBits) - 1u;
constexpr uint64_t kFragMaxPrimitives = 1ull << kFragIdBits;  // ids 0 .. 2^22 - 1
constexpr uint64_t kFragNull = ~0ull;
constexpr uint64_t kFragKeyBackground = (0x7F800000ull << 32) | 0xFFFFFFFFull;   // the 10-byte format's background key {+inf, -1}
static_assert(kFragTileW * kFragTileH <= (1 << kFragPixelBits), "the pixel field holds a tile's pixels");
static_assert(31 + kFragPixelBits + kFragIdBits == 64, "z without its sign bit, pixel and id fill the word");

// May the launches of this renderer use packed entries?  Triangle primitives (a texel renderer's key holds a texel id, up to 2^32)
// whose every id -- the position in the face list, or the caller's id from the renderer's prim_id table, both below F -- fits 22 bits.
SMESH_FRAG_HD bool frag_packed_allowed(bool texels, uint64_t F) { return !texels && F <= kFragMaxPrimitives; }

// `zbits`: float_bits(z) of z > 0, finite (or +inf: the background); `pixel` < 2048; `id` < 2^22.
SMESH_FRAG_HD uint64_t frag_pack(uint32_t zbits, uint32_t pixel, uint32_t id) {
  return ((uint64_t)zbits << 33) | ((uint64_t)(pixel & kFragPixelMask) << kFragIdBits) | (uint64_t)(id & kFragIdMask);
}
SMESH_FRAG_HD uint32_t frag_zbits(uint64_t e) { return (uint32_t)(e >> 33); }
SMESH_FRAG_HD uint32_t frag_pixel(uint64_t e) { return (uint32_t)(e >> kFragIdBits) & kFragPixelMask; }
SMESH_FRAG_HD uint32_t frag_id(uint64_t e) { return (uint32_t)e & kFragIdMask; }
SMESH_FRAG_HD uint64_t frag_background(uint32_t pixel) { return frag_pack(0x7F800000u, pixel, kFragIdMask); }
SMESH_FRAG_HD bool frag_is_background(uint64_t e) { return frag_zbits(e) == 0x7F800000u; }

// A 64-bit key of the 10-byte format (a fragment's, the background key, or the null key) as the packed entry of `pixel`, and back.
SMESH_FRAG_HD uint64_t frag_from_key(uint64_t key, uint32_t pixel) {
  if (key == kFragNull) return kFragNull;
  if (key == kFragKeyBackground) return frag_background(pixel);
  return frag_pack((uint32_t)(key >> 32), pixel, (uint32_t)key);
}
SMESH_FRAG_HD uint64_t frag_key(uint64_t e) {
  if (e == kFragNull) return kFragNull;
  if (frag_is_background(e)) return kFragKeyBackground;
  return ((uint64_t)frag_zbits(e) << 32) | (uint64_t)frag_id(e);
}

}  // namespace smesh
