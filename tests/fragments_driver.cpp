// Stand-alone driver of the packed fragment-queue entry (semantic_meshes_amd/csrc/fragments.hpp): plain host C++ with its own main,
// meant to be compiled under -fsanitize=address,undefined and run on the CPU (tests/test_fragments_host.py does so).
// Exit status 0 and "fragments driver ok".
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../semantic_meshes_amd/csrc/fragments.hpp"

using namespace smesh;

static int fails = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      if (fails < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
      fails++;                                                \
    }                                                         \
  } while (0)

static uint32_t bits_of(float z) { uint32_t b; std::memcpy(&b, &z, 4); return b; }
// the 10-byte format's depth-test key
static uint64_t key_of(uint32_t zbits, uint32_t id) { return ((uint64_t)zbits << 32) | id; }

int main() {
  // round trips at the extremes of every field
  const uint32_t ids[] = {0u, 1u, 2999u, (1u << 22) - 2u, (1u << 22) - 1u};
  const uint32_t pixels[] = {0u, 1u, 63u, 64u, 2046u, 2047u};
  const uint32_t zs[] = {1u, bits_of(FLT_MIN), bits_of(1.0f), bits_of(FLT_MAX), 0x7F7FFFFFu};
  for (uint32_t id : ids)
    for (uint32_t p : pixels)
      for (uint32_t z : zs) {
        const uint64_t e = frag_pack(z, p, id);
        CHECK(frag_zbits(e) == z && frag_pixel(e) == p && frag_id(e) == id, "fields of %016llx", (unsigned long long)e);
        CHECK(frag_key(e) == key_of(z, id), "key of %016llx", (unsigned long long)e);
        CHECK(frag_from_key(key_of(z, id), p) == e, "entry of the key {%08x, %u} at pixel %u", z, id, p);
        CHECK(e != kFragNull && !frag_is_background(e), "a fragment is neither null nor background");
        // null is above the background, the background above every fragment of its pixel
        CHECK(e < frag_background(p) && frag_background(p) < kFragNull, "order of %016llx, background, null", (unsigned long long)e);
      }
  // null and background: what they unpack to, and where a null entry points (inside the tile's 2048 slots)
  CHECK(frag_key(kFragNull) == kFragNull && frag_from_key(kFragNull, 5u) == kFragNull, "null round trip");
  CHECK(frag_pixel(kFragNull) == 2047u, "a null entry names slot %u", frag_pixel(kFragNull));
  for (uint32_t p : pixels) {
    const uint64_t b = frag_background(p);
    CHECK(frag_is_background(b) && frag_pixel(b) == p && frag_key(b) == kFragKeyBackground, "background of pixel %u", p);
    CHECK(frag_from_key(kFragKeyBackground, p) == b, "the background key at pixel %u", p);
    CHECK((uint32_t)frag_key(b) == 0xFFFFFFFFu && (uint32_t)(frag_key(b) >> 32) == 0x7F800000u, "the planes of a background pixel: -1, +inf");
  }
  CHECK(!frag_is_background(kFragNull), "null is not the background");
  // order: for random pairs of (z > 0 finite, id) at one pixel the packed order is the key order, equal z included
  std::mt19937_64 rng(20252);
  for (int rep = 0; rep < 200000; rep++) {
    const uint32_t p = (uint32_t)(rng() % 2048u);
    auto zbits = [&]() -> uint32_t {
      switch (rng() % 4u) {
        case 0: return 1u + (uint32_t)(rng() % 0x7F7FFFFFu);            // any positive finite pattern, subnormals included
        case 1: return bits_of(0.5f + (float)(rng() % 1000u) * 1e-3f);  // a scene's depths
        case 2: return bits_of(1.0f) + (uint32_t)(rng() % 3u);          // neighbours
        default: return bits_of(1.0f);
      }
    };
    const uint32_t za = zbits(), zb = (rng() % 3u) ? zbits() : za;
    const uint32_t ia = (uint32_t)(rng() & kFragIdMask), ib = (rng() % 5u) ? (uint32_t)(rng() & kFragIdMask) : ia;
    const uint64_t ka = key_of(za, ia), kb = key_of(zb, ib), ea = frag_pack(za, p, ia), eb = frag_pack(zb, p, ib);
    CHECK((ka < kb) == (ea < eb) && (ka == kb) == (ea == eb), "order of {%08x, %u} and {%08x, %u} at pixel %u", za, ia, zb, ib, p);
    CHECK(ea < frag_background(p) && eb < frag_background(p), "below the background");
  }
  // the predicate
  CHECK(frag_packed_allowed(false, 0) && frag_packed_allowed(false, 1ull << 22), "F = 2^22 takes packed entries");
  CHECK(!frag_packed_allowed(false, (1ull << 22) + 1), "F = 2^22 + 1 does not");
  CHECK(!frag_packed_allowed(true, 1) && !frag_packed_allowed(true, 1ull << 22), "texel renderers do not");
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("fragments driver ok\n");
  return 0;
}
