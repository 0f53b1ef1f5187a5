// The source-over blend in linear light, device code shared by the 1:1 kernels (bt709_kernels.hip:
// BT709HIP_OPT_COMPOSITE_OVER) and the any-ratio rescale kernels (bt709_scaled_strip.h: BT709HIP_OPT_SCALED_OVER)
// -- one copy, so both options blend bit for bit alike.  Per pixel, s the 8-bit word the same call writes with the option off, d
// the background (what the output held, or a solid colour with A_d = 255), every float operation rounded on its own:
//     k     = float(255 - A_s) * (1/255f)                    byteNorm of the complement (sRGB.h:32-36)
//     v_c   = min(1, lin[s_c] + k * lin[d_c])                lin[b] = sRGB_nonLinearNormToLinear(byteNorm(b)), the colour premultiplied
//     out_c = the LINEAR-mode composite of v_c               the rescale kernels' log-bucket encode table
//     out_A = A_s + ((255 - A_s) * A_d + 127) / 255          integer
#pragma once
#include "bt709_device.h"

namespace bt709 {
namespace {

typedef __attribute__((address_space(3))) const float *LdsFloatPtr;  // ds_read_b32

struct OverLookup {
  float enc_add;     // encode table: bucket of v = (bits(v + enc_add) >> 16) - first
  uint32_t enc_off;  // its LDS address - (first << 3)
  uint32_t lin_off;  // LDS address of lin[256]
};

__device__ __forceinline__ float over_lin(const OverLookup &o, uint32_t byte) {
  return *reinterpret_cast<LdsFloatPtr>((byte << 2) + o.lin_off);
}

// sRGB byte of a linear-light v in [0, 1], the table's edges staged as they are (unit range): the index is a plain add (the host
// files the thresholds under the same one, transfer_tables.cpp bucket_index_log), the bucket's edge settles it
__device__ __forceinline__ uint32_t over_encode(const OverLookup &o, float v) {
  const uint32_t t = __float_as_uint(__fadd_rn(v, o.enc_add)) >> 16;
  const u32x2 e = *reinterpret_cast<LdsPairPtr>((t << 3) + o.enc_off);
  return e.y + (v >= __uint_as_float(e.x) ? 1u : 0u);
}

// One pixel from its BYTES: sr, sg, sb, as = the source word's channels, bg the background word (kOverDestination) -- colour_lin
// the background's three linear values otherwise.  encode(v): the sRGB byte of a unit-range v -- over_encode, or the caller's own
// lookup where its copy of the table is staged in another domain.
template <int OVER, typename Encode>
__device__ __forceinline__ uint32_t over_blend(const OverLookup &o, const float *colour_lin, uint32_t sr, uint32_t sg, uint32_t sb, uint32_t as,
                                               uint32_t bg, const Encode &encode) {
  const uint32_t inv = 255u - as;
  const float k = __fmul_rn(static_cast<float>(inv), kInv255);
  float d[3];
  uint32_t a = 255u;  // an opaque background: A_s + (255 - A_s)
  if (OVER == kOverDestination) {
    d[0] = over_lin(o, (bg >> 16) & 0xffu);
    d[1] = over_lin(o, (bg >> 8) & 0xffu);
    d[2] = over_lin(o, bg & 0xffu);
    a = as + (inv * (bg >> 24) + 127u) / 255u;
  } else {
    d[0] = colour_lin[0], d[1] = colour_lin[1], d[2] = colour_lin[2];
  }
  const uint32_t s[3] = {sr, sg, sb};
  uint32_t byte[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)  // the sum is in [0, 2): the add's clamp is the min with 1
    byte[c] = encode(add_sat(over_lin(o, s[c]), __fmul_rn(k, d[c])));
  return pack_bgra(byte[0], byte[1], byte[2], a << 24);
}

}  // namespace
}  // namespace bt709
