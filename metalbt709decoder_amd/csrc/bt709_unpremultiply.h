// Premultiplied -> straight alpha on the bytes of a decoded BGRA word (BT709HIP_OPT_UNPREMULTIPLY), written ONCE
// for the device and for the host, as bt709_split_lookup.h is: hipcc compiles this text into the straight-alpha instantiations of
// decode_quads / decode_blocks, and tests/native/straight_alpha_sweep.cpp compiles the same text with g++ to replay it over all
// 65 536 (c', A) pairs against the definition
//
//   c = A == 0 ? 0 : min(255, (255 * c' + A / 2) / A)        c', A in 0..255, integer division; A stays what it is
//
// (the reference's twin, +[BGRAToBT709Converter unpremultiply:] (Renderer/BGRAToBT709Converter.m:1128-1182), is a vImage call --
// a closed box, DESIGN.md 8: the rounding is ours, to nearest).  A = 255 is the identity, A = 0 gives colour 0, and c' > A -- no
// premultiplied value, but any Y, Cb, Cr triple can decode to it -- saturates at 255.
//
// The division.  The alpha kernels hold no LDS table, so it is a reciprocal, no lookup -- and needs no fix-up: with
// n = 255 c' + A / 2 (<= 65 152, exact as a float) the quotient floor(n / A) is also floor((n + 1/2) / A), and (n + 1/2) / A
// lies at least 1 / (2 A) away from every integer (n mod A is a whole number of A-ths).  So c is the round-to-nearest of
//     v = (n + 1/2) r - 1/2 = fma(n, r, k),   k = fma(r, 1/2, -1/2),   r ~ 1 / A,   n = fma(c', 255, A / 2) exactly
// as long as v is within 1 / (2 A) of its real value; with r within 4 ulp of 1 / A the error of v stays below
// 65 153 / A x 2^-20 < 0.07 / A, and a tie cannot occur.  Round-to-nearest and the saturation at 255 (c' > A) are one instruction
// on the device, v_cvt_pk_u8_f32, which also drops the byte into its lane of the word.  A = 0: r = 0, every v is -1/2, every byte
// 0: no select.  `r` is v_rcp_f32's result on the device (1 ulp), whatever its last bits are: the host sweep replays every pair
// with the correctly rounded reciprocal moved by -2 .. +2 floats.  The fmas are the division's own steps, not a contraction
// of reference arithmetic.
#pragma once

#include <cstdint>

#ifndef BT709_HD
#if defined(__HIPCC__)
#define BT709_HD __host__ __device__ __forceinline__
#else
#define BT709_HD inline
#endif
#endif

namespace bt709 {

// One pixel from its premultiplied bytes R, G, B and its alpha byte a: the word (a<<24)|(R<<16)|(G<<8)|B with R, G, B divided by
// a; a = 0: the word 0.  `rcp` maps a float in 1..255 to its reciprocal (the kernels: v_rcp_f32; the host sweep: the exact one,
// perturbed); `byte_into(v, lane, word)` returns `word` with byte `lane` replaced by v rounded to nearest and saturated to 0..255
// (the kernels: v_cvt_pk_u8_f32 under the default rounding mode, which the decode kernels never change).
template <class Rcp, class ByteInto>
BT709_HD uint32_t unpremultiply_pixel(uint32_t R, uint32_t G, uint32_t B, uint32_t a, Rcp rcp, ByteInto byte_into) {
  const float r = a ? rcp(static_cast<float>(a)) : 0.0f;
  const float k = __builtin_fmaf(r, 0.5f, -0.5f);
  const float half_a = static_cast<float>(a >> 1);  // n is formed in floats (exact: <= 65 152): an integer multiply-add of values the
  uint32_t w = a << 24;                              // compiler cannot bound is a 64-bit one on gfx950
  w = byte_into(__builtin_fmaf(__builtin_fmaf(static_cast<float>(B), 255.0f, half_a), r, k), 0u, w);
  w = byte_into(__builtin_fmaf(__builtin_fmaf(static_cast<float>(G), 255.0f, half_a), r, k), 1u, w);
  w = byte_into(__builtin_fmaf(__builtin_fmaf(static_cast<float>(R), 255.0f, half_a), r, k), 2u, w);
  return w;
}

}  // namespace bt709
