// Per-code arithmetic of the planar CHW decode targets (BT709HIP_FORMAT_CHW_F16 / _F32), written ONCE for the
// device and for the host, as bt709_split_lookup.h and bt709_premultiply.h are: hipcc compiles this text into the kernels of
// bt709_chw.hip, and tests/native/chw_norm_sweep.cpp compiles it with g++ to replay every code under a list of (scale, bias)
// pairs against the definition
//
//   v   = float(s) * (1.0f / 255.0f)         s the byte a BGRA8_SRGB target would hold; byteNorm, as DESIGN.md 3.5
//   t   = v * scale;  t = t + bias           binary32, every operation rounded on its own: no fused multiply-add
//   out = t, or binary16(t) rounded to nearest even (overflow: +-inf, as IEEE 754 says)
//   alpha plane: v alone
//
// scale and bias are +-0 or finite with 2^-64 <= |x| <= 2^64 (chw_norm_bits_valid: what bt709hip_decoder_set_option accepts), so
// no product or sum here is a binary32 subnormal or overflows binary32.
// In the kernel and not in a 3 x 256 table: per value a conversion, two multiplies and an add (v_cvt_f32_ubyteN straight off the
// packed word, v_mul_f32 x 2, v_add_f32) against a byte extract, an address and a ds_read plus 3 KiB staged per workgroup.
#pragma once

#include <cstdint>
#include <cstring>

#include "bt709_constants.h"

#ifndef BT709_HD
#if defined(__HIPCC__)
#define BT709_HD __host__ __device__ __forceinline__
#else
#define BT709_HD inline
#endif
#endif

namespace bt709 {

// byteNorm: the alpha plane's value
BT709_HD float chw_unit(float code) { return code * kInv255; }

// A colour plane's value for the byte `code` (an integer-valued float, 0..255): three statements, three roundings.  Nothing here
// may be contracted: the product is built with -ffp-contract=off (build.py FLAGS; a CPU test reads the kernels' code for a
// stray fused multiply-add), and so is the host replay.
BT709_HD float chw_norm(float code, float scale, float bias) {
  const float v = code * kInv255;
  const float t = v * scale;
  return t + bias;
}

// binary16 of a binary32, round to nearest even; subnormals kept, overflow to infinity, NaN stays NaN
BT709_HD uint16_t chw_half_bits(float t) {
#if defined(__clang__)
  return __builtin_bit_cast(uint16_t, static_cast<_Float16>(t));  // hipcc, device (v_cvt_f16_f32) and host
#else  // a host compiler without the type: the same conversion in integers
  uint32_t b;
  std::memcpy(&b, &t, sizeof b);
  const uint32_t sign = (b >> 16) & 0x8000u, mag = b & 0x7fffffffu;
  if (mag >= 0x7f800000u) return static_cast<uint16_t>(sign | 0x7c00u | (mag > 0x7f800000u ? 0x200u : 0u));
  if (mag >= 0x477ff000u) return static_cast<uint16_t>(sign | 0x7c00u);  // rounds to 2^16 or beyond
  if (mag < 0x33000001u) return static_cast<uint16_t>(sign);            // at most half of the smallest subnormal: ties to even, 0
  const int exp = static_cast<int>(mag >> 23) - 127;                    // unbiased
  uint32_t frac = (mag & 0x7fffffu) | 0x800000u;                        // 24 significant bits
  const int drop = exp < -14 ? 13 + (-14 - exp) : 13;                   // bits below the binary16 result's last place
  const uint32_t rest = frac & ((1u << drop) - 1u), half = 1u << (drop - 1);
  frac >>= drop;
  if (rest > half || (rest == half && (frac & 1u))) ++frac;
  // normal: frac has its leading one at bit 10 (a carry out of the rounding moves into the exponent by the addition)
  const uint32_t h = exp < -14 ? frac : (static_cast<uint32_t>(exp + 14) << 10) + frac;
  return static_cast<uint16_t>(sign | h);
#endif
}

// what BT709HIP_OPT_CHW_SCALE_* / _BIAS_* accept: the bit pattern of +-0 or of a finite binary32 with 2^-64 <= |x| <= 2^64
inline bool chw_norm_bits_valid(uint32_t bits) {
  const uint32_t mag = bits & 0x7fffffffu;
  return mag == 0u || (mag >= 0x1f800000u && mag <= 0x5f800000u);
}

}  // namespace bt709
