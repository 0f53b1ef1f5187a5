// Luma of an ALPHA frame -- written ONCE for the shim and for the host test, as bt709_split_lookup.h is: shim_convert.cpp
// builds the 256-byte table the two alpha kernels (bt709_encode.hip encode_alpha_y / encode_alpha_y_blocks) look up, and
// tests/native/alpha_luma_table.cpp compiles the same text with g++ against tests/golden/alpha_luma.json.
//
// The reference encodes an alpha clip (srgb_to_bt709 -alpha, srgb_to_bt709/srgb_to_bt709.m:842-954) by copying each pixel's A
// over R, G and B, forcing the gamma to linear and running the ordinary encoder.  For a grey (A,A,A) picture under
// (Linear, Linear) every step of cvpbu_ycbcr_subsample -> BT709_average_pixel_values is a function of single bytes:
//   Y[i]     = sRGB_from_sRGB_convertRGBToYCbCr(e, e, e)[0],  e = per_byte[A_i].enc_norm          BT709.h:1423-1487
//            = round(((Kr*e + Kg*e) + Kb*e) * 219 + 16)       each operation rounded to float      BT709.h:222, 233, 244
//   (Cb, Cr) = (128, 128): the averaged byte is a grey byte again, and B - Ey, R - Ey of a grey are below half a code.
// So the whole frame is T[A] per pixel, T monotone with 220 distinct values.
#pragma once

#include <cmath>
#include <cstdint>

#include "bt709_constants.h"
#include "transfer_tables.h"

namespace bt709 {

// T[A] from the (Linear, Linear) per-byte table of build_encode_tables: the expression of encode_block
// (bt709_encode.hip), operation by operation.  Compile with -ffp-contract=off, as everything that restates the reference.
inline void build_alpha_luma(const EncodeByteEntry per_byte[256], uint8_t out[256]) {
  for (int a = 0; a < 256; ++a) {
    const float e = per_byte[a].enc_norm;
    const float kr = kKr * e, kg = kKg * e, kb = kKb * e;
    const float rg = kr + kg;
    const float ey = rg + kb;                                             // BT709.h:222
    const float scaled = ey * static_cast<float>(kYMax - kYMin);
    const float v = scaled + 16.0f;                                       // BT709.h:233
    out[a] = static_cast<uint8_t>(static_cast<int>(std::round(v)));       // BT709.h:244
  }
}

}  // namespace bt709
