// Device code of the 1:1 decode kernels (bt709_kernels.hip), shared by both chroma layouts (NV12, planar I420): the per-quad and
// per-block arithmetic, the composite-over staging, the body of the fast kernels (quads_body) and the walk of the general-path
// kernels (blocks_body).  Only the tile front end -- which chroma bytes reach which quad -- and the general path's chroma fetch
// depend on the layout (bt709_tile.h TileIn<LAYOUT, ...>).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bt709_device.h"
#include "bt709_over.h"
#include "bt709_unpremultiply.h"

namespace bt709 {
namespace {

// BT709HIP_OPT_UNPREMULTIPLY: the pixel an alpha decoder would store, its R, G, B divided by its own alpha byte
// (bt709_unpremultiply.h: per pixel one reciprocal; per channel a conversion, the division's two fmas and the v_cvt_pk_u8_f32
// that rounds, saturates and drops the byte into the word -- in registers, no table, no LDS).
__device__ __forceinline__ uint32_t straight_pixel(uint32_t R, uint32_t G, uint32_t B, uint32_t a) {
  return unpremultiply_pixel(R, G, B, a, [](float v) { return __builtin_amdgcn_rcpf(v); },
                             [](float v, uint32_t lane, uint32_t word) { return __builtin_amdgcn_cvt_pk_u8_f32(v, lane, word); });
}

// One 4x2 quad: 8 pixels x (R, G, B) = 24 lookups.  Pixel p = 0..3 top row, 4..7 bottom row.
// QUANT: the decoder's mode is sRGB, whose composite is the plain quantiser ("no curve at all", BT709.h:977-983):
// every channel is quantise_byte of its saturated value -- no table, no LDS.  Always set for alpha decoders
// (hasAlphaChannel forces the sRGB mode, MetalBT709Decoder.m:165-169).
template <bool HAS_ALPHA, bool QUANT, bool LOGIDX>
__device__ __forceinline__ void decode_quad(const UnitLookup &u, uint32_t ya, uint32_t yb, uint32_t cw, uint32_t aa,
                                            uint32_t ab, uint32_t alpha_word, u32x4 &top, u32x4 &bot) {
  const Chroma c0 = chroma_terms(byte_of(cw, 0), byte_of(cw, 1));
  const Chroma c1 = chroma_terms(byte_of(cw, 2), byte_of(cw, 3));
  float x[24];
#pragma unroll
  for (int px = 0; px < 8; ++px)
    pixel_rgb(byte_of(px < 4 ? ya : yb, px & 3), (px & 2) ? c1 : c0, x[3 * px], x[3 * px + 1], x[3 * px + 2]);
  static_assert(QUANT || !HAS_ALPHA, "an alpha decoder runs the sRGB mode");
  uint32_t byte[24], al[8];
  if (QUANT) {
#pragma unroll
    for (int i = 0; i < 24; ++i) byte[i] = quantise_byte(x[i]);
  } else {
    uint32_t t[24];
    magic_index12(x, t, u.magic);
    magic_index12(x + 12, t + 12, u.magic);
    if (LOGIDX) {  // log-bucket table (the LINEAR mode): the sum's exponent and top 7 mantissa bits
#pragma unroll
      for (int i = 0; i < 24; ++i) t[i] >>= 16;
    }
#pragma unroll
    for (int i = 0; i < 24; ++i) byte[i] = bucket_byte(u, x[i], t[i]);
  }
#pragma unroll
  for (int px = 0; px < 8; ++px)
    al[px] = HAS_ALPHA ? quantise_byte(alpha_value(byte_of(px < 4 ? aa : ab, px & 3))) << 24 : alpha_word;
  top.x = pack_bgra(byte[0], byte[1], byte[2], al[0]);
  top.y = pack_bgra(byte[3], byte[4], byte[5], al[1]);
  top.z = pack_bgra(byte[6], byte[7], byte[8], al[2]);
  top.w = pack_bgra(byte[9], byte[10], byte[11], al[3]);
  bot.x = pack_bgra(byte[12], byte[13], byte[14], al[4]);
  bot.y = pack_bgra(byte[15], byte[16], byte[17], al[5]);
  bot.z = pack_bgra(byte[18], byte[19], byte[20], al[6]);
  bot.w = pack_bgra(byte[21], byte[22], byte[23], al[7]);
}

// decode_quad of an alpha decoder with every pixel through straight_pixel (BT709HIP_OPT_UNPREMULTIPLY)
__device__ __forceinline__ void straight_quad(uint32_t ya, uint32_t yb, uint32_t cw, uint32_t aa, uint32_t ab, u32x4 &top, u32x4 &bot) {
  const Chroma c0 = chroma_terms(byte_of(cw, 0), byte_of(cw, 1));
  const Chroma c1 = chroma_terms(byte_of(cw, 2), byte_of(cw, 3));
  uint32_t w[8];
#pragma unroll
  for (int px = 0; px < 8; ++px) {
    float x[3];
    pixel_rgb(byte_of(px < 4 ? ya : yb, px & 3), (px & 2) ? c1 : c0, x[0], x[1], x[2]);
    w[px] = straight_pixel(quantise_byte(x[0]), quantise_byte(x[1]), quantise_byte(x[2]), quantise_byte(alpha_value(byte_of(px < 4 ? aa : ab, px & 3))));
  }
  top.x = w[0], top.y = w[1], top.z = w[2], top.w = w[3];
  bot.x = w[4], bot.y = w[5], bot.z = w[6], bot.w = w[7];
}

// One 2x2 block (general path): 4 pixels x (R, G, B); y = {tl, tr, bl, br}
template <bool HAS_ALPHA, bool QUANT, bool STRAIGHT = false>
__device__ __forceinline__ void decode_block(const UnitLookup &u, const float y[4], float cb, float cr, const float a[4],
                                             uint32_t alpha_word, uint32_t out[4]) {
  const Chroma c = chroma_terms(cb, cr);
  float x[12];
#pragma unroll
  for (int px = 0; px < 4; ++px) pixel_rgb(y[px], c, x[3 * px], x[3 * px + 1], x[3 * px + 2]);
  static_assert((HAS_ALPHA && QUANT) || !STRAIGHT, "there is nothing to divide by without an alpha channel");
  if constexpr (STRAIGHT) {
#pragma unroll
    for (int px = 0; px < 4; ++px)
      out[px] = straight_pixel(quantise_byte(x[3 * px]), quantise_byte(x[3 * px + 1]), quantise_byte(x[3 * px + 2]), quantise_byte(alpha_value(a[px])));
    return;
  }
  if (QUANT) {  // sRGB mode: the plain quantiser for every channel (see decode_quad)
#pragma unroll
    for (int px = 0; px < 4; ++px)
      out[px] = pack_bgra(quantise_byte(x[3 * px]), quantise_byte(x[3 * px + 1]), quantise_byte(x[3 * px + 2]),
                          HAS_ALPHA ? quantise_byte(alpha_value(a[px])) << 24 : alpha_word);
    return;
  }
  uint32_t t[12];
  magic_index12(x, t, u.magic);
#pragma unroll
  for (int i = 0; i < 12; ++i) t[i] >>= u.shift;  // general path: the table's form is a run-time value
#pragma unroll
  for (int px = 0; px < 4; ++px)
    out[px] = pack_bgra(bucket_byte(u, x[3 * px], t[3 * px]), bucket_byte(u, x[3 * px + 1], t[3 * px + 1]),
                        bucket_byte(u, x[3 * px + 2], t[3 * px + 2]), alpha_word);
}

// ---------------------------------------------------------------------------
// BT709HIP_OPT_COMPOSITE_OVER: an alpha decoder's word goes source-over a background in linear light, the
// two-pass equivalent of "decode, then blend the 8-bit result".  The blend itself: bt709_over.h (shared with the rescale kernels).
// LDS: the encode table (DecodeParams::table_encode, ~5 KiB) and lin[256] (1 KiB) behind it.
// ---------------------------------------------------------------------------
// Stages both tables (the caller synchronises) and returns the lookup constants.
__device__ __forceinline__ OverLookup stage_over_tables(unsigned char *lds_raw, const DecodeParams &p) {
  stage_table(lds_raw, p.table_encode, p.table_encode_bytes);
  stage_table(lds_raw + p.table_encode_bytes, p.over_table_lin, kOverLinBytes);
  OverLookup o;
  o.enc_add = p.encode_log_add;
  o.enc_off = lds_address(lds_raw) - (p.encode_log_first << 3);
  o.lin_off = lds_address(lds_raw) + p.table_encode_bytes;
  return o;
}

// One pixel: x = its saturated R, G, B (pixel_rgb), abyte its alpha-frame sample, bg the background word (kOverDestination) --
// colour_lin the background's three linear values otherwise.
template <int OVER>
__device__ __forceinline__ uint32_t over_pixel(const OverLookup &o, const float *colour_lin, const float *x, float abyte, uint32_t bg) {
  return over_blend<OVER>(o, colour_lin, quantise_byte(x[0]), quantise_byte(x[1]), quantise_byte(x[2]), quantise_byte(alpha_value(abyte)), bg,
                          [&](float v) { return over_encode(o, v); });
}

// decode_quad's pixels through over_pixel; bt / bb: what the output's two rows held (kOverDestination)
template <int OVER>
__device__ __forceinline__ void over_quad(const OverLookup &o, const DecodeParams &p, uint32_t ya, uint32_t yb, uint32_t cw, uint32_t aa,
                                          uint32_t ab, const u32x4 &bt, const u32x4 &bb, u32x4 &top, u32x4 &bot) {
  const Chroma c0 = chroma_terms(byte_of(cw, 0), byte_of(cw, 1));
  const Chroma c1 = chroma_terms(byte_of(cw, 2), byte_of(cw, 3));
  const uint32_t bg[8] = {bt.x, bt.y, bt.z, bt.w, bb.x, bb.y, bb.z, bb.w};
  uint32_t w[8];
#pragma unroll
  for (int px = 0; px < 8; ++px) {
    float x[3];
    pixel_rgb(byte_of(px < 4 ? ya : yb, px & 3), (px & 2) ? c1 : c0, x[0], x[1], x[2]);
    w[px] = over_pixel<OVER>(o, p.over_lin, x, byte_of(px < 4 ? aa : ab, px & 3), bg[px]);
  }
  top.x = w[0], top.y = w[1], top.z = w[2], top.w = w[3];
  bot.x = w[4], bot.y = w[5], bot.z = w[6], bot.w = w[7];
}


// ---------------------------------------------------------------------------
// Fast path.  Preconditions (checked by the host shim): width % 4 == 0; y, cbcr,
// alpha pointers and strides 4-byte aligned; output pointer and stride 16-byte
// aligned.  grid = (tiles, H/2, frames); a tile is blockDim * kQuadsPerLane quads.
// ---------------------------------------------------------------------------
// LOGIDX: the table is in log-bucket form (one shift more per channel).  (The body once covered 2 or 4 row pairs per workgroup: that
// served the LINEAR mode's 33 KiB uniform table until its log-bucket form made it 5 KiB, decode_quads_log.)
// OVER (kOverDestination / kOverColour; alpha decoders): the composite-over form -- the tile's front end also loads what the
// output held (destination mode), both of its tables are staged behind the loads, and the quads go through over_quad.
// LAYOUT: the chroma layout, handed to the tile front end, which leaves cw = {Cb0, Cr0, Cb1, Cr1} per quad for either.
// STRAIGHT (BT709HIP_OPT_UNPREMULTIPLY; alpha decoders, never with OVER): the quads' pixels through straight_pixel.
template <uint32_t LAYOUT, bool HAS_ALPHA, bool NT, bool QUANT, bool LOGIDX = false, int OVER = kOverOff, bool STRAIGHT = false>
__device__ __forceinline__ void quads_body(const DecodeParams &p, unsigned char *lds_raw) {
  constexpr int UNROLL = kQuadsPerLane;
  const BandedWork work = banded_work<true>(p.xcd_bands, p.frames_per_band);  // XCD-aware work map: bt709_tile.h
  const FramePlanes f = frame_planes(p, work.frame);
  const uint32_t quads = p.width >> 2;
  const uint32_t row_pairs = p.height >> 1;
  // blockDim.y > 1 only for narrow frames: a workgroup then covers blockDim.y consecutive row
  // pairs so that it still has ~8 waves (1920-wide: 256 x 2).  blockDim.x is a whole number of
  // waves, so threadIdx.y is the same in every lane of a wave: taking it from the first lane
  // makes the row pointers scalar (SGPR base + per-lane offset addressing, no 64-bit VALU
  // address arithmetic).
  const uint32_t rp_raw = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);
  const uint32_t q0 = work.tile * (blockDim.x * UNROLL) + threadIdx.x;

  // straight-line: loads, table, pin, arithmetic, predicated stores (bt709_tile.h TileIn)
  static_assert(OVER == kOverOff || HAS_ALPHA, "there is nothing to composite without an alpha channel");
  static_assert(OVER == kOverOff || !STRAIGHT, "a blend needs the premultiplied source");
  static_assert(HAS_ALPHA || !STRAIGHT, "there is nothing to divide by without an alpha channel");
  TileIn<LAYOUT, UNROLL, HAS_ALPHA, OVER == kOverDestination> in;
  in.template load<NT>(f, p, rp_raw, row_pairs, q0, quads);
  OverLookup ol = {};
  if constexpr (OVER != kOverOff) {
    ol = stage_over_tables(lds_raw, p);  // after the tile's loads are in flight
    __syncthreads();
  }
  if (!QUANT) {  // the sRGB mode needs no table (decode_quad)
    stage_table(lds_raw, p.table_unit, p.table_unit_bytes);  // after the tile's loads are in flight
    __syncthreads();
  }
  in.pin();

  const UnitLookup ul = unit_lookup(p, lds_raw);
  uint8_t *o0 = f.out + static_cast<size_t>(2 * min(rp_raw, row_pairs - 1)) * p.out_stride;
  uint8_t *o1 = o0 + p.out_stride;
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {  // one walk: the quads through the blend, their pixels through the division, or plain
    const uint32_t q = q0 + u * blockDim.x;
    u32x4 top, bot;
    if constexpr (OVER != kOverOff)
      over_quad<OVER>(ol, p, in.ya[u], in.yb[u], in.cw[u], in.aa[u], in.ab[u], in.da[OVER == kOverDestination ? u : 0], in.db[OVER == kOverDestination ? u : 0], top, bot);
    else if constexpr (STRAIGHT)
      straight_quad(in.ya[u], in.yb[u], in.cw[u], in.aa[u], in.ab[u], top, bot);
    else
      decode_quad<HAS_ALPHA, QUANT, LOGIDX>(ul, in.ya[u], in.yb[u], in.cw[u], HAS_ALPHA ? in.aa[u] : 0u, HAS_ALPHA ? in.ab[u] : 0u, p.alpha_word, top, bot);
    if (q < quads && rp_raw < row_pairs) {
      store16<NT>(o0 + 16 * q, top);
      store16<NT>(o1 + 16 * q, bot);
    }
  }
}

// ---------------------------------------------------------------------------
// General path: any even width/height, any stride, byte-aligned planes, 4-byte
// aligned output.  One lane per 2x2 block, grid-strided over row pairs.  Correctness
// first; used for ragged or misaligned frames only.  That correctness is pinned by tests/test_decode_variants.py: all 2^24
// triples through every instantiation of decode_blocks and decode_blocks_over, and the grid-stride loop, both forms of
// frame_planes and the over kernels at launch shapes computed from the device.
// Block bx of row pair rp takes its chroma from bytes 2 bx, 2 bx + 1 of the CbCr row (kChromaNV12), or from byte bx of the U row
// and of the V row v_offset bytes behind it (kChromaI420; bx < W/2: inside the row's W/2 bytes of either plane).
// ---------------------------------------------------------------------------
// One walk for decode_blocks and decode_blocks_over.  OVER (alpha decoders): each 2x2 block through over_pixel; each output word
// is read (destination mode) and written by one lane alone.  STRAIGHT (alpha decoders, never with OVER): decode_block's pixels
// through straight_pixel.
// The __global__ kernel stages the tables (the unit table unless QUANT; both over tables) and hands in the lookup constants, ul or
// ol: nothing is in flight ahead of the staging here, and staged from inside this body the kernels gain ten instructions -- this
// body is simplified as a function of its own before it is inlined, the block count that blockDim.x (the staging) and gridDim.x
// (the row-pair stride) both read becomes one load with two users, and the compiler's fold of blockDim.x to the uniform workgroup
// size, which wants one user per load, no longer applies (a global_load_ushort, a compare and a select instead of one packed dword).
// __restrict__: the parameter block is not written through the plane pointers it holds, so that simplification hoists the loads of
// the pitches out of the loops together with the arithmetic, in the order the kernels' own text had (profiles/r16_one_walk_isa.txt).
template <uint32_t LAYOUT, bool HAS_ALPHA, bool QUANT, int OVER = kOverOff, bool STRAIGHT = false>
__device__ __forceinline__ void blocks_body(const DecodeParams &__restrict__ p, const UnitLookup &ul, const OverLookup &ol) {
  constexpr bool PLANAR = LAYOUT == kChromaI420;
  static_assert(OVER == kOverOff || (HAS_ALPHA && QUANT && !STRAIGHT), "a blend needs an alpha decoder's premultiplied source");
  const FramePlanes f = frame_planes(p, blockIdx.y);
  const uint32_t bw = p.width >> 1;
  const uint32_t row_pairs = p.height >> 1;

  for (uint32_t rp = blockIdx.x; rp < row_pairs; rp += gridDim.x) {
    const uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    const uint8_t *y1 = y0 + p.y_stride;
    const uint8_t *cc = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;  // the CbCr row, or the U row
    const uint8_t *vv = PLANAR ? cc + p.v_offset : nullptr;
    uint32_t *o0 = reinterpret_cast<uint32_t *>(f.out + static_cast<size_t>(2 * rp) * p.out_stride);
    uint32_t *o1 = reinterpret_cast<uint32_t *>(f.out + static_cast<size_t>(2 * rp + 1) * p.out_stride);
    for (uint32_t bx = threadIdx.x; bx < bw; bx += kBlockThreads) {
      const float y[4] = {byte_value(y0[2 * bx]), byte_value(y0[2 * bx + 1]), byte_value(y1[2 * bx]), byte_value(y1[2 * bx + 1])};
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      if (HAS_ALPHA) {
        const uint8_t *a0 = f.alpha + static_cast<size_t>(2 * rp) * p.alpha_stride;
        const uint8_t *a1 = a0 + p.alpha_stride;
        a[0] = byte_value(a0[2 * bx]);
        a[1] = byte_value(a0[2 * bx + 1]);
        a[2] = byte_value(a1[2 * bx]);
        a[3] = byte_value(a1[2 * bx + 1]);
      }
      uint32_t bg[4] = {0u, 0u, 0u, 0u};
      if (OVER == kOverDestination) bg[0] = o0[2 * bx], bg[1] = o0[2 * bx + 1], bg[2] = o1[2 * bx], bg[3] = o1[2 * bx + 1];
      const float cb = byte_value(PLANAR ? cc[bx] : cc[2 * bx]), cr = byte_value(PLANAR ? vv[bx] : cc[2 * bx + 1]);
      uint32_t out[4];
      if constexpr (OVER != kOverOff) {
        const Chroma c = chroma_terms(cb, cr);
#pragma unroll
        for (int px = 0; px < 4; ++px) {
          float x[3];
          pixel_rgb(y[px], c, x[0], x[1], x[2]);
          out[px] = over_pixel<OVER>(ol, p.over_lin, x, a[px], bg[px]);
        }
      } else {
        decode_block<HAS_ALPHA, QUANT, STRAIGHT>(ul, y, cb, cr, a, p.alpha_word, out);
      }
      o0[2 * bx] = out[0];
      o0[2 * bx + 1] = out[1];
      o1[2 * bx] = out[2];
      o1[2 * bx + 1] = out[3];
    }
  }
}
}  // namespace
}  // namespace bt709
