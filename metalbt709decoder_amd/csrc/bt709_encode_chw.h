// The planar-tensor encoder's kernels (BT709HIP_CTX_OPT_ENCODE_CHW_INPUT); included by bt709_encode.hip alone, behind
// the helpers it shares with the BGRA8 encoder's kernels (encode_block, quantize_quad, quantize_block, store_quad_chroma,
// store_block_chroma, second_byte, stage_encode_tables, encode_frame, v_plane_offset ...) and behind every kernel that existed.
//
// A planar C x H x W tensor of bytes, halves or floats -> 4:2:0 NV12 / I420, the mirror of decode_quads_chw (bt709_chw.hip): 3 e bytes
// read and 1.5 written per pixel, e = 1, 2 or 4.  Plane c of a surface starts c * height * bgra_stride bytes behind plane 0
// (EncodeFrame::bgra; a 64-bit product); planes R, G, B are read, a fourth is never touched.  Per element
//   u8:        s_c = the byte
//   f16, f32:  s_c = chw_denorm(t, scale_c, bias_c)       bt709_chw_denorm.h: two rounded operations, saturation, quantise_exact
// and the frame is the BGRA8 encoder's frame of the texels (B, G, R) = (s_B, s_G, s_R): the three bytes are packed into the word
// encode_block takes, and from there the code IS the BGRA8 kernels' (per-byte table, 2x2 average in linear light, matrix, quantiser,
// stores), so every gamma pair and DESIGN.md 3.4's proof carry over.  scale and bias ride in EncodeParams::chw (kernel arguments:
// SGPRs, nothing staged); the u8 kernels do not read them.
#pragma once

#include "bt709_chw_denorm.h"

namespace bt709 {
namespace {

// four consecutive elements of a plane row as loaded: 4, 8 or 16 bytes
template <uint32_t ELEM> struct ChwQuadBits { typedef uint32_t type; };
template <> struct ChwQuadBits<kChwF16> { typedef u32x2 type; };
template <> struct ChwQuadBits<kChwF32> { typedef u32x4 type; };

template <uint32_t ELEM>
__device__ __forceinline__ typename ChwQuadBits<ELEM>::type load_chw_quad(const uint8_t *row, uint32_t q) {
  return __builtin_nontemporal_load(reinterpret_cast<const typename ChwQuadBits<ELEM>::type *>(row + 4u * chw_elem_bytes(ELEM) * q));
}

// the bytes s of a quad's four elements of one plane, pixel i in bits [8 i, 8 i + 7]
template <uint32_t ELEM>
__device__ __forceinline__ uint32_t chw_quad_bytes(const typename ChwQuadBits<ELEM>::type &v, float scale, float bias) {
  if constexpr (ELEM == kChwU8) {
    return v;
  } else if constexpr (ELEM == kChwF16) {
    const uint32_t s0 = chw_denorm(chw_half_value(static_cast<uint16_t>(v.x)), scale, bias), s1 = chw_denorm(chw_half_value(static_cast<uint16_t>(v.x >> 16)), scale, bias);
    const uint32_t s2 = chw_denorm(chw_half_value(static_cast<uint16_t>(v.y)), scale, bias), s3 = chw_denorm(chw_half_value(static_cast<uint16_t>(v.y >> 16)), scale, bias);
    return s0 | (s1 << 8) | (s2 << 16) | (s3 << 24);
  } else {
    const uint32_t s0 = chw_denorm(__uint_as_float(v.x), scale, bias), s1 = chw_denorm(__uint_as_float(v.y), scale, bias);
    const uint32_t s2 = chw_denorm(__uint_as_float(v.z), scale, bias), s3 = chw_denorm(__uint_as_float(v.w), scale, bias);
    return s0 | (s1 << 8) | (s2 << 16) | (s3 << 24);
  }
}

// pixel I of a quad as the word encode_block reads: B | G << 8 | R << 16 (byte 3, the A it ignores, stays 0)
template <int I>
__device__ __forceinline__ uint32_t chw_word(uint32_t r, uint32_t g, uint32_t b) {
  return ((b >> (8 * I)) & 0xffu) | (((g >> (8 * I)) & 0xffu) << 8) | (((r >> (8 * I)) & 0xffu) << 16);
}

// the byte s of ONE element (general kernel): row points at the plane row, x is the pixel
template <uint32_t ELEM>
__device__ __forceinline__ uint32_t chw_element_byte(const uint8_t *row, uint32_t x, float scale, float bias) {
  if constexpr (ELEM == kChwU8) return row[x];
  else if constexpr (ELEM == kChwF16) return chw_denorm(chw_half_value(reinterpret_cast<const uint16_t *>(row)[x]), scale, bias);
  else return chw_denorm(reinterpret_cast<const float *>(row)[x], scale, bias);
}

}  // namespace

// Preconditions of the fast kernel (checked by the host shim): width % 4 == 0; plane 0 and the pitch 4 e-aligned (every plane and
// every row of it then is: a plane starts height * pitch bytes behind the one before); Y 4-byte aligned; NV12: the CbCr pointer and
// pitch 4-byte aligned; I420: the U pointer and the chroma pitch 2-byte aligned -- what encode_bgra needs of its output.
// grid = (tiles, row-pair groups, frames), banded_work, one quad (4 x 2 pixels) per lane: encode_bgra's walk, with six loads per row
// pair (three planes x two rows) where it has two.  Consecutive lanes read consecutive 4 e bytes of each plane row.
// BOUNDS: q <= quads - 1 = W/4 - 1, so a lane reads bytes [4 e q, 4 e q + 4 e - 1] <= e W - 1 of a row of e W bytes; rows 2 rp and
// 2 rp + 1 with rp < rp_end <= H/2, so row <= H - 1, of planes 0, 1 and 2: the last byte read is byte e W - 1 of row H - 1 of plane 2,
// at offset (3 H - 1) * pitch + e W - 1 from plane 0 -- inside the three planes the surface describes; no load reaches a fourth plane.
// The prefetch is issued for rp + 1 < rp_end alone.  Only lanes with q_raw < quads store: bytes [4 q, 4 q + 3] <= W - 1 of a Y or CbCr
// row (I420: [2 q, 2 q + 1] <= W/2 - 1 of a U or V row), rows as encode_bgra.
template <uint32_t LAYOUT, uint32_t ELEM>
__global__ void __launch_bounds__(kMaxBlockThreads)
encode_chw(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  typedef typename ChwQuadBits<ELEM>::type Bits;
  const BandedWork work = banded_work(p.xcd_bands, p.frames_per_band);  // XCD-aware work map: bt709_tile.h
  const EncodeFrame f = encode_frame(p, work.frame);
  const uint32_t quads = p.width >> 2;
  const uint32_t row_pairs = p.height >> 1;
  const uint32_t q_raw = work.tile * blockDim.x + threadIdx.x;
  const uint32_t q = min(q_raw, quads - 1);
  const uint32_t rp0 = blockIdx.y * p.row_pairs_per_block;
  const uint32_t rp_end = min(rp0 + p.row_pairs_per_block, row_pairs);
  const size_t plane = static_cast<size_t>(p.height) * p.bgra_stride;  // uniform: two scalar multiplies

  // plane and row pointers are uniform (SGPR base), the lane adds a 32-bit offset: no 64-bit VALU address arithmetic
  const uint8_t *s0 = f.bgra + static_cast<size_t>(2 * rp0) * p.bgra_stride;
  Bits rt = load_chw_quad<ELEM>(s0, q), rb = load_chw_quad<ELEM>(s0 + p.bgra_stride, q);
  Bits gt = load_chw_quad<ELEM>(s0 + plane, q), gb = load_chw_quad<ELEM>(s0 + plane + p.bgra_stride, q);
  Bits bt = load_chw_quad<ELEM>(s0 + 2 * plane, q), bb = load_chw_quad<ELEM>(s0 + 2 * plane + p.bgra_stride, q);

  const EncodeLds t = stage_encode_tables(lds_raw, p);  // after the first loads are in flight
  __syncthreads();
  const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);

  for (uint32_t rp = rp0; rp < rp_end; ++rp) {
    // the next row pair's six loads ahead of the arithmetic; nothing on the workgroup's last pair, as encode_bgra
    Bits nrt = rt, nrb = rb, ngt = gt, ngb = gb, nbt = bt, nbb = bb;
    if (rp + 1 < rp_end) {
      const uint8_t *s1 = f.bgra + static_cast<size_t>(2 * (rp + 1)) * p.bgra_stride;
      nrt = load_chw_quad<ELEM>(s1, q), nrb = load_chw_quad<ELEM>(s1 + p.bgra_stride, q);
      ngt = load_chw_quad<ELEM>(s1 + plane, q), ngb = load_chw_quad<ELEM>(s1 + plane + p.bgra_stride, q);
      nbt = load_chw_quad<ELEM>(s1 + 2 * plane, q), nbb = load_chw_quad<ELEM>(s1 + 2 * plane + p.bgra_stride, q);
    }

    const uint32_t r0 = chw_quad_bytes<ELEM>(rt, p.chw.scale[0], p.chw.bias[0]), r1 = chw_quad_bytes<ELEM>(rb, p.chw.scale[0], p.chw.bias[0]);
    const uint32_t g0 = chw_quad_bytes<ELEM>(gt, p.chw.scale[1], p.chw.bias[1]), g1 = chw_quad_bytes<ELEM>(gb, p.chw.scale[1], p.chw.bias[1]);
    const uint32_t b0 = chw_quad_bytes<ELEM>(bt, p.chw.scale[2], p.chw.bias[2]), b1 = chw_quad_bytes<ELEM>(bb, p.chw.scale[2], p.chw.bias[2]);
    float va[6], vb[6];
    {
      const uint32_t blk[4] = {chw_word<0>(r0, g0, b0), chw_word<1>(r0, g0, b0), chw_word<0>(r1, g1, b1), chw_word<1>(r1, g1, b1)};
      encode_block(t, quarter_n, blk, va);
    }
    {
      const uint32_t blk[4] = {chw_word<2>(r0, g0, b0), chw_word<3>(r0, g0, b0), chw_word<2>(r1, g1, b1), chw_word<3>(r1, g1, b1)};
      encode_block(t, quarter_n, blk, vb);
    }
    uint32_t ytop, ybot, cbcr;
    quantize_quad<LAYOUT>(va, vb, ytop, ybot, cbcr);
    if (q_raw < quads) {
      uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
      __builtin_nontemporal_store(ytop, reinterpret_cast<uint32_t *>(y0 + 4u * q));
      __builtin_nontemporal_store(ybot, reinterpret_cast<uint32_t *>(y0 + p.y_stride + 4u * q));
      store_quad_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, q, cbcr);
    }
    rt = nrt, rb = nrb, gt = ngt, gb = ngb, bt = nbt, bb = nbb;
  }
}

// General layout: one lane per 2x2 block, element loads (1, 2 or 4 bytes: planes e-aligned, any even W and H), byte stores at any
// alignment.  grid = (block tiles, row pairs, frames), grid-strided in x, as encode_bgra_blocks.
// BOUNDS: bx < W/2, so a lane reads elements 2 bx and 2 bx + 1 <= W - 1 of rows 2 rp and 2 rp + 1 <= H - 1 (rp = blockIdx.y < H/2) of
// planes 0, 1 and 2 -- the last byte read is the fast kernel's -- and writes bytes 2 bx, 2 bx + 1 <= W - 1 of two Y rows and of one
// CbCr row (I420: byte bx <= W/2 - 1 of a U and a V row).
template <uint32_t LAYOUT, uint32_t ELEM>
__global__ void __launch_bounds__(kBlockThreads)
encode_chw_blocks(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const EncodeLds t = stage_encode_tables(lds_raw, p);
  __syncthreads();
  const EncodeFrame f = encode_frame(p, blockIdx.z);
  const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);
  const uint32_t bw = p.width >> 1;
  const uint32_t rp = blockIdx.y;
  const size_t plane = static_cast<size_t>(p.height) * p.bgra_stride;
  const uint8_t *rows[3][2];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rows[c][0] = f.bgra + c * plane + static_cast<size_t>(2 * rp) * p.bgra_stride;
    rows[c][1] = rows[c][0] + p.bgra_stride;
  }
  for (uint32_t bx = blockIdx.x * blockDim.x + threadIdx.x; bx < bw; bx += gridDim.x * blockDim.x) {
    uint32_t blk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t x = 2 * bx + (i & 1);
      const uint32_t r = chw_element_byte<ELEM>(rows[0][i >> 1], x, p.chw.scale[0], p.chw.bias[0]);
      const uint32_t g = chw_element_byte<ELEM>(rows[1][i >> 1], x, p.chw.scale[1], p.chw.bias[1]);
      const uint32_t b = chw_element_byte<ELEM>(rows[2][i >> 1], x, p.chw.scale[2], p.chw.bias[2]);
      blk[i] = b | (g << 8) | (r << 16);
    }
    float v[6];
    encode_block(t, quarter_n, blk, v);
    uint32_t ytop, ybot, cbcr;
    quantize_block(v, ytop, ybot, cbcr);
    uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    uint8_t *y1 = y0 + p.y_stride;
    // byte stores, whatever the alignment (second_byte<kChromaI420> keeps byte 1 a value of its own); the NV12 Cb Cr pair leaves as
    // one 2-byte store at whatever address the row has, as encode_bgra_blocks' does (legal on gfx950)
    y0[2 * bx] = static_cast<uint8_t>(ytop);
    y0[2 * bx + 1] = second_byte<kChromaI420>(ytop);
    y1[2 * bx] = static_cast<uint8_t>(ybot);
    y1[2 * bx + 1] = second_byte<kChromaI420>(ybot);
    store_block_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, bx, static_cast<uint8_t>(cbcr), second_byte<kChromaI420>(cbcr));
  }
}

}  // namespace bt709
