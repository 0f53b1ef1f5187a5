// Straight -> premultiplied alpha on the bytes of a BGRA word (BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY), written
// ONCE for the device and for the host, as bt709_split_lookup.h is: hipcc compiles this text into the premultiplying
// instantiations of encode_bgra / encode_bgra_blocks, and tests/native/straight_alpha_sweep.cpp compiles the same text with g++
// to replay it over all 65 536 (c, A) pairs against the definition
//
//   c' = (c * A + 127) / 255            c, A in 0..255, integer division; A stays what it is
//
// (what CoreGraphics does when it renders into a kCGImageAlphaPremultipliedFirst bitmap is a closed box, DESIGN.md 8: the
// rounding is the `+ 127) / 255` of 3.5's out_A).  A = 255 is the identity, A = 0 gives colour 0.
//
// The division: n / 255 == (n + 1 + (n >> 8)) >> 8 for every n < 65 535, and n = c * A + 127 <= 65 152.  Nothing on that way
// leaves 16 bits (n + 1 + (n >> 8) <= 65 407), so B and R -- bytes 0 and 2 of the word -- go through it side by side in the two
// halves of one register: a 24-bit multiply-add, a shift, a mask, a three-operand add, a shift and a mask for the pair.
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

// one channel: the definition's c' for c, a in 0..255
BT709_HD uint32_t premultiply_byte(uint32_t c, uint32_t a) {
  const uint32_t n = c * a + 127u;
  return (n + 1u + (n >> 8)) >> 8;
}

// (A<<24)|(R<<16)|(G<<8)|B -> the same word with R, G, B premultiplied by A
BT709_HD uint32_t premultiply_word(uint32_t w) {
  const uint32_t a = w >> 24;
  const uint32_t rb = (w & 0x00ff00ffu) * a + 0x007f007fu;  // {R * A + 127, B * A + 127}, 16 bits each
  const uint32_t g = ((w >> 8) & 0xffu) * a + 127u;
  const uint32_t rb8 = ((rb + 0x00010001u + ((rb >> 8) & 0x00ff00ffu)) >> 8) & 0x00ff00ffu;
  const uint32_t g8 = (g + 1u + (g >> 8)) & 0xff00u;  // the quotient, already in byte 1
  return (w & 0xff000000u) | rb8 | g8;
}

}  // namespace bt709
