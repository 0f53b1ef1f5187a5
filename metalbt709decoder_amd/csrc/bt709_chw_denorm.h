// Per-element arithmetic of planar CHW encoder INPUT (BT709HIP_CTX_OPT_ENCODE_CHW_INPUT with BT709HIP_FORMAT_CHW_F16 /
// _F32 surfaces), the way back of bt709_chw_norm.h and written ONCE for the device and for the host as that file is: hipcc compiles
// this text into the kernels of bt709_encode_chw.h, and tests/native/chw_denorm_sweep.cpp compiles it with g++ to replay every half
// code and the float32 edge set under a list of (scale, bias) pairs against the definition
//
//   t   = the element (a binary16 converts to binary32 exactly)
//   u   = t * scale;  u = u + bias            binary32, every operation rounded on its own: no fused multiply-add
//   x   = sat(u)                              NaN -> 0, u < 0 (and -0) -> 0, u > 1 (and +inf) -> 1
//   s   = quantise_exact(x)                   bt709_quantise.h: round-half-away of x * 255.0f, exact for every float in [0, 1]
//
// s is the byte the BGRA8_SRGB encoder would have been handed.  scale and bias are +-0 or finite with 2^-64 <= |x| <= 2^64
// (chw_norm_bits_valid), t is ANY bit pattern: a product that overflows is +-inf and saturates, inf * 0 and inf - inf are NaN and
// give 0.  Comparisons and not v_max / v_min / v_med3: what those return for a NaN operand depends on MODE.ieee, a compare does not.
#pragma once

#include <cstdint>
#include <cstring>

#include "bt709_quantise.h"

// as bt709_quantise.h: the two statements of `u` are two roundings whatever the including file's flags say
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace bt709 {

// binary32 of a binary16, exact: subnormals, infinities and NaN (payload kept in the upper mantissa bits) included
BT709_HD float chw_half_value(uint16_t h) {
#if defined(__clang__)
  return static_cast<float>(__builtin_bit_cast(_Float16, h));  // hipcc, device (v_cvt_f32_f16) and host
#else  // a host compiler without the type: the same conversion in integers
  const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
  uint32_t bits;
  if (exp == 0u) {  // +-0, or a subnormal man * 2^-24: the product is exact
    const float v = static_cast<float>(man) * 5.9604644775390625e-08f;
    std::memcpy(&bits, &v, sizeof bits);
    bits |= sign;
  } else if (exp == 31u) {
    bits = sign | 0x7f800000u | (man << 13);
  } else {
    bits = sign | ((exp + 112u) << 23) | (man << 13);
  }
  float out;
  std::memcpy(&out, &bits, sizeof out);
  return out;
#endif
}

// sat(t * scale + bias): three statements, two roundings and two compares.  !(u > 0) is true for NaN, -0 and everything below 0.
BT709_HD float chw_denorm_unit(float t, float scale, float bias) {
  const float m = t * scale;
  const float u = m + bias;
  if (!(u > 0.0f)) return 0.0f;
  return u > 1.0f ? 1.0f : u;
}

// the byte of a float element
BT709_HD uint32_t chw_denorm(float t, float scale, float bias) { return quantise_exact(chw_denorm_unit(t, scale, bias)); }

}  // namespace bt709
