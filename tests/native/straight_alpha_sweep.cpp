// Host replay of the product's straight-alpha arithmetic: csrc/bt709_premultiply.h and csrc/bt709_unpremultiply.h,
// the text hipcc compiles into the premultiplying encode kernels and the straight-alpha decode kernels, compiled here by g++ and
// run over all 65 536 (colour byte, alpha byte) pairs.  The caller (tests/test_straight_alpha_cpu.py) holds the definition, in
// Python integers, and compares.
//
// The word sweeps put the pair's colour byte c into R, c + 85 into G and c + 170 into B (mod 256): over the sweep every byte lane
// of the word meets every (value, alpha) pair, and a lane that leaked into its neighbour would show.
#include <cmath>
#include <cstdint>

#include "bt709_premultiply.h"
#include "bt709_unpremultiply.h"

namespace {
uint32_t word_of(uint32_t c, uint32_t a) { return (a << 24) | (c << 16) | (((c + 85u) & 255u) << 8) | ((c + 170u) & 255u); }
}  // namespace

extern "C" {

// out[c * 256 + a]
void sweep_premultiply_byte(uint8_t *out) {
  for (uint32_t c = 0; c < 256; ++c)
    for (uint32_t a = 0; a < 256; ++a) out[c * 256 + a] = static_cast<uint8_t>(bt709::premultiply_byte(c, a));
}

void sweep_words_in(uint32_t *out) {
  for (uint32_t c = 0; c < 256; ++c)
    for (uint32_t a = 0; a < 256; ++a) out[c * 256 + a] = word_of(c, a);
}

void sweep_premultiply_word(uint32_t *out) {
  for (uint32_t c = 0; c < 256; ++c)
    for (uint32_t a = 0; a < 256; ++a) out[c * 256 + a] = bt709::premultiply_word(word_of(c, a));
}

// the reciprocal the kernels take from v_rcp_f32 (1 ulp): here the correctly rounded 1 / A moved by `ulps` representable floats;
// the byte the kernels take from v_cvt_pk_u8_f32: rounded to nearest (ties to even), saturated to 0..255, placed in its lane
void sweep_unpremultiply_word(int ulps, uint32_t *out) {
  const auto rcp = [ulps](float v) {
    float r = 1.0f / v;
    for (int i = 0; i < (ulps < 0 ? -ulps : ulps); ++i) r = std::nextafterf(r, ulps < 0 ? 0.0f : 2.0f);
    return r;
  };
  const auto byte_into = [](float v, uint32_t lane, uint32_t word) {
    const float n = std::nearbyintf(v);  // the default rounding mode
    const uint32_t b = n <= 0.0f ? 0u : (n >= 255.0f ? 255u : static_cast<uint32_t>(n));
    return (word & ~(0xffu << (8 * lane))) | (b << (8 * lane));
  };
  for (uint32_t c = 0; c < 256; ++c)
    for (uint32_t a = 0; a < 256; ++a) {
      const uint32_t w = word_of(c, a);
      out[c * 256 + a] = bt709::unpremultiply_pixel((w >> 16) & 0xffu, (w >> 8) & 0xffu, w & 0xffu, w >> 24, rcp, byte_into);
    }
}

}  // extern "C"
