// The alpha step of the paired half encoder (BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA) -- written ONCE for the device
// and for the host, as bt709_quantise.h is: hipcc compiles half_alpha_luma into encode_rgba16f_alpha / encode_rgba16f_alpha_blocks
// (bt709_encode_half_alpha.h), and tests/native/half_alpha_step.cpp compiles the very same text with g++ (-ffp-contract=off) to
// replay it over all 65536 half codes against tests/golden/alpha_luma.json.
//
// The alpha frame of a pair is what DESIGN.md 3.12 writes under (LINEAR, LINEAR) for the surface whose R, G, B are its A: the
// reference's alpha clip is the grey picture (A,A,A) with the gamma forced to linear (srgb_to_bt709/srgb_to_bt709.m:842-954), and
// BT709_from_linear(v, Linear) is (int)round(v * 255.0f) (Renderer/BT709.h:1150-1167).  Per pixel:
//   a = sat(float(hA))       exact half -> float; NaN -> 0, a < 0 (and -0) -> 0, a > 1 (and +inf) -> 1
//   e = quantise_exact(a)    equal to the reference's round for every float in [0, 1] (bt709_quantise.h)
//   Y = T[e]                 T = the alpha frames' luma table (bt709_alpha_luma.h)
// and Cb = Cr = 128: the average of four a goes through the same round to a grey byte again.
#pragma once

#include <cstdint>
#include <cstring>

#include "bt709_quantise.h"

namespace bt709 {

// Table: whatever a byte code indexes -- the kernels pass an LDS byte pointer (one ds_read_u8), the host replay a plain array
template <typename Table>
BT709_HD uint32_t half_alpha_luma(Table t, float a) {
  return t[quantise_exact(a)];
}

// sat(float(half)) in portable C++, for the host replay: the value the kernels get from v_cvt_f32_f16 with the clamp bit
// (bt709_encode_half.h half_sat).  Every half is exactly a float; subnormal halves are not flushed.
inline float half_sat_value(uint16_t h) {
  const uint32_t exponent = (h >> 10) & 31u, fraction = h & 1023u;
  if (exponent == 31u) return fraction != 0u || (h & 0x8000u) ? 0.0f : 1.0f;  // NaN -> 0, -inf -> 0, +inf -> 1
  if (h & 0x8000u) return 0.0f;                                                 // negative values and -0
  uint32_t bits;
  if (exponent != 0u) {
    bits = ((exponent + 112u) << 23) | (fraction << 13);
  } else {  // zero and the subnormals: fraction * 2^-24, exact in a float
    const float v = static_cast<float>(fraction) * 5.9604644775390625e-08f;
    std::memcpy(&bits, &v, sizeof bits);
  }
  float v;
  std::memcpy(&v, &bits, sizeof v);
  return v > 1.0f ? 1.0f : v;
}

}  // namespace bt709
