// Stand-alone driver of the compact per-triangle record (semantic_meshes_amd/csrc/records.hpp): plain host C++ with its own main,
// meant to be compiled under -fsanitize=address,undefined and run on the CPU (tests/test_records_host.py does so).
// Exit status 0 and "records driver ok".
#include <cstdint>
#include <cstdio>
#include <random>

#include "../semantic_meshes_amd/csrc/records.hpp"

using namespace smesh;

static int fails = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      if (fails < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
      fails++;                                                \
    }                                                         \
  } while (0)

// A random TriFrag-order mask (bit dx * 8 + dy) inside a bw x bh box.
static uint64_t random_mask(std::mt19937_64& rng, int bw, int bh) {
  uint64_t m = 0;
  for (int dx = 0; dx < bw; dx++)
    for (int dy = 0; dy < bh; dy++)
      if (rng() & 1u) m |= 1ull << (dx * 8 + dy);
  return m;
}

int main() {
  std::mt19937_64 rng(20251);
  // origins: 0, 1, the largest 13-bit value, and the largest origin of a bw x bh box inside an 8 192-pixel image
  for (int bw = 1; bw <= 8; bw++)
    for (int bh = 1; bh <= 8; bh++) {
      const uint32_t xs[4] = {0u, 1u, 8191u, kRecMaxImage - (uint32_t)bw}, ys[4] = {0u, 1u, 8191u, kRecMaxImage - (uint32_t)bh};
      for (int ix = 0; ix < 4; ix++)
        for (int iy = 0; iy < 4; iy++)
          for (int rep = 0; rep < 8; rep++) {
            const uint64_t m = rep == 0 ? random_mask(rng, bw, bh) | 1ull | (1ull << ((bw - 1) * 8 + (bh - 1))) : random_mask(rng, bw, bh);
            // kind 3 exactly when a small box exceeds 6 in x or y
            const uint32_t kind = rec_kind_of(1u, bw, bh);
            CHECK(kind == ((bw > 6 || bh > 6) ? 3u : 1u), "box %d x %d -> kind %u", bw, bh, kind);
            CHECK(rec_kind_of(0u, bw, bh) == 0u && rec_kind_of(2u, bw, bh) == 2u, "kinds 0 and 2 pass through");
            const uint64_t w = rec_pack(xs[ix], ys[iy], kind, m);
            CHECK(rec_kind(w) == kind && rec_x0(w) == xs[ix] && rec_y0(w) == ys[iy], "fields of %016llx", (unsigned long long)w);
            if (kind == 1u) {
              CHECK(rec_word_mask64(w) == m, "mask round trip %016llx -> %016llx", (unsigned long long)m, (unsigned long long)rec_word_mask64(w));
              CHECK((w & kRecMask36) == rec_mask36(m) && rec_mask36(m) <= kRecMask36, "36-bit field");
              // ascending set bits name the same pixels in the same order in both layouts, and rec_bit is the word's index of a pixel
              uint64_t a = m, b = w & kRecMask36;
              while (a && b) {
                const int ka = __builtin_ctzll(a), kb = __builtin_ctzll(b);
                CHECK((ka >> 3) == kb / kRecBox && (ka & 7) == kb % kRecBox, "bit order: %d against %d", ka, kb);
                CHECK(rec_bit(ka >> 3, ka & 7) == kb, "rec_bit(%d, %d)", ka >> 3, ka & 7);
                // clearing that pixel in the word (the tile resolve's atomicAnd) clears it in the unpacked mask, and nothing else
                const uint64_t cleared = w & ~(1ull << rec_bit(ka >> 3, ka & 7));
                CHECK(rec_word_mask64(cleared) == (m & ~(1ull << ka)), "clearing pixel %d", ka);
                CHECK(rec_kind(cleared) == 1u && rec_x0(cleared) == xs[ix] && rec_y0(cleared) == ys[iy], "clearing leaves the fields");
                a &= a - 1; b &= b - 1;
              }
              CHECK(a == 0 && b == 0, "the two masks hold the same number of pixels");
            } else {
              CHECK((w & kRecMask36) == 0, "a kind-%u word carries no mask", kind);
            }
          }
    }
  // every single pixel of the 6 x 6 box
  for (int dx = 0; dx < kRecBox; dx++)
    for (int dy = 0; dy < kRecBox; dy++) {
      const uint64_t m = 1ull << (dx * 8 + dy);
      CHECK(rec_mask36(m) == 1ull << rec_bit(dx, dy), "pixel (%d, %d)", dx, dy);
      CHECK(rec_mask64(1ull << rec_bit(dx, dy)) == m, "pixel (%d, %d) back", dx, dy);
    }
  CHECK(rec_mask64(kRecMask36) == 0x00003F3F3F3F3F3Full, "the full box");
  // the two planes: 256-byte aligned, disjoint, inside the allocation
  const uint64_t Fs[] = {0, 1, 31, 32, 33, 3000, 1000000, 0xFFFFFFFFull};
  for (uint64_t F : Fs) {
    CHECK(rec_full_offset(F) % 256 == 0 && rec_full_offset(F) >= F * 8 && rec_full_offset(F) < F * 8 + 256, "offset of F = %llu", (unsigned long long)F);
    CHECK(rec_alloc_bytes(F) == rec_full_offset(F) + F * 16, "allocation of F = %llu", (unsigned long long)F);
  }
  CHECK(rec_image_fits(8192, 8192) && rec_image_fits(1, 8192) && !rec_image_fits(8193, 8) && !rec_image_fits(8, 8193), "image bound");
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("records driver ok\n");
  return 0;
}
