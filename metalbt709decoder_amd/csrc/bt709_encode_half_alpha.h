// The paired half-input encoder's kernels (BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA); included by bt709_encode.hip
// alone, behind bt709_encode_half.h (half_sat, stage_from_linear, encode_half_block) and the pair's helpers (pair_frame, AlphaPlanes,
// stage_alpha_luma).
//
// One RGBA16Float surface in, TWO frames out of one read: the colour frame encode_rgba16f writes (3.12, byte for byte), and the alpha
// frame -- Y = T[round(255 sat(A))] per pixel (bt709_half_alpha_step.h), Cb = Cr = 128 when it has a chroma plane -- which is what
// 3.12 writes under (LINEAR, LINEAR) for the surface whose R, G, B are its A.  The route it replaces is three launches (the half
// encode, a 1:1 render into a BGRA8 scratch surface, a BGRA8_ALPHA encode): about 26.5 B/pixel against 10.5-11 here.
//
// Shape: encode_rgba16f's, unchanged -- a 2x2 block per lane, two 16-byte non-temporal loads with the next pair's issued ahead, the
// lane clamp, predicated stores, the plain half encoder's launch plan.  The rider: the lane already holds its four A halves in the
// upper words of top.y, top.w, bot.y and bot.w: four clamped v_cvt_f32_f16, four quantise_exact (5 VALU each), four ds_read_u8, two
// 2-byte stores to the alpha Y rows, and with alpha chroma one 2-byte 0x8080 store (NV12) or two byte stores of 0x80 (I420).
//
// T is a TABLE in LDS, not arithmetic: T[e] in registers, operation by operation as build_alpha_luma does, is a conversion, a multiply
// by 1/255, three multiplies, two adds, a multiply, two adds and a truncating conversion -- 11 VALU per pixel, 44 per lane and row
// pair, against 4 ds_read_u8 whose address is the code itself plus T's base (compiled side by side:
// profiles/r20_encode_half_alpha_isa.txt).  The 256 bytes are one dword per LDS bank, as for encode_alpha_y, and the kernel stays at
// the memory rate with them (profiles/r20_encode_half_alpha.txt).
//
// __global__ templates of their own and not an `if constexpr` in encode_rgba16f / encode_rgba16f_blocks: with the pair's rider in
// encode_bgra's text the plain instantiations changed their register assignment (profiles/r18_encode_pair_isa.txt); here every
// existing kernel compiles to the text it had (profiles/r20_encode_half_alpha_isa.txt).
//
// LDS: stage_from_linear needs the dynamic segment at address 0, so these kernels have no static LDS either; T's 256 bytes sit in
// the dynamic segment behind the from_linear table, and launch_encode sizes the segment for them.
#pragma once

#include "bt709_half_alpha_step.h"

namespace bt709 {
namespace {

typedef __attribute__((address_space(3))) const uint8_t *LdsBytePtr;  // one ds_read_u8

// where T is staged: behind the from_linear table (16-byte granular) that stage_from_linear puts at address 0
__device__ __forceinline__ uint32_t *half_pair_alpha_lut(unsigned char *lds_raw, const EncodeParams &p) {
  return reinterpret_cast<uint32_t *>(lds_raw + p.from_linear_bytes);
}
// ... and where it is read: the dynamic segment starts at LDS address 0 (stage_from_linear traps otherwise)
__device__ __forceinline__ LdsBytePtr half_pair_alpha_table(const EncodeParams &p) {
  return reinterpret_cast<LdsBytePtr>(p.from_linear_bytes);
}

// T[round(255 sat(A))] of the two texels of a block's row, {R | G << 16, B | A << 16} each: two bytes in memory order
__device__ __forceinline__ uint32_t half_alpha_luma2(LdsBytePtr t, uint32_t ba_left, uint32_t ba_right) {
  return half_alpha_luma(t, half_sat<1>(ba_left)) | (half_alpha_luma(t, half_sat<1>(ba_right)) << 8);
}

}  // namespace

// Preconditions of the fast kernel (checked by the host shim): encode_rgba16f's, and the alpha Y pointer, pitch and batch step
// 2-byte aligned; NV12: the alpha CbCr pointer and pitch 2-byte aligned; I420: none on the alpha U and V (byte stores).
// grid = (tiles, row-pair groups, pairs), as encode_rgba16f.
// BOUNDS: b <= blocks - 1 = W/2 - 1, so a lane reads bytes [16 b, 16 b + 15] <= 8 W - 1 of a row of 8 W bytes, rows 2 rp and
// 2 rp + 1 with rp < H/2; only lanes with b_raw < blocks store, bytes [2 b, 2 b + 1] <= W - 1 of a Y or CbCr row (I420: byte b of a
// U or V row of W/2) of the colour frame AND of the alpha frame, whose rows are its own pitches apart (>= W, planar chroma >= W/2)
// and whose V plane lies (H/2) x its chroma pitch behind its U plane; the alpha chroma is touched under with_cbcr alone.
template <uint32_t LAYOUT>
__global__ void __launch_bounds__(kMaxBlockThreads)
encode_rgba16f_alpha(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const BandedWork work = banded_work(p.xcd_bands, p.frames_per_band);  // XCD-aware work map: bt709_tile.h
  AlphaPlanes a;
  const EncodeFrame f = pair_frame(p, work.frame, a);
  const uint32_t blocks = p.width >> 1;
  const uint32_t row_pairs = p.height >> 1;
  const uint32_t b_raw = work.tile * blockDim.x + threadIdx.x;
  const uint32_t b = min(b_raw, blocks - 1);
  const uint32_t rp0 = blockIdx.y * p.row_pairs_per_block;
  const uint32_t rp_end = min(rp0 + p.row_pairs_per_block, row_pairs);

  // row pointers are uniform (SGPR base), the lane adds a 32-bit offset: no 64-bit VALU address arithmetic
  const uint8_t *s0 = f.bgra + static_cast<size_t>(2 * rp0) * p.bgra_stride;
  u32x4 top = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + 16u * b));
  u32x4 bot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + p.bgra_stride + 16u * b));

  const EncodeLds t = stage_from_linear(lds_raw, p);  // after the first loads are in flight
  stage_alpha_luma(half_pair_alpha_lut(lds_raw, p), p);
  __syncthreads();
  const LdsBytePtr ta = half_pair_alpha_table(p);
  const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);

  for (uint32_t rp = rp0; rp < rp_end; ++rp) {
    u32x4 ntop = top, nbot = bot;
    if (rp + 1 < rp_end) {  // nothing on the workgroup's last pair, as encode_bgra
      const uint8_t *s1 = f.bgra + static_cast<size_t>(2 * (rp + 1)) * p.bgra_stride;
      ntop = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + 16u * b));
      nbot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + p.bgra_stride + 16u * b));
    }
    const uint32_t atop = half_alpha_luma2(ta, top.y, top.w), abot = half_alpha_luma2(ta, bot.y, bot.w);  // the rider
    float v[6];
    encode_half_block(t, p.from_linear_scale, quarter_n, top, bot, v);
    uint32_t ytop, ybot, cbcr;
    quantize_block(v, ytop, ybot, cbcr);
    if (b_raw < blocks) {
      uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
      __builtin_nontemporal_store(static_cast<uint16_t>(ytop), reinterpret_cast<uint16_t *>(y0 + 2u * b));
      __builtin_nontemporal_store(static_cast<uint16_t>(ybot), reinterpret_cast<uint16_t *>(y0 + p.y_stride + 2u * b));
      uint8_t *c = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;
      if (LAYOUT == kChromaI420) {
        __builtin_nontemporal_store(static_cast<uint8_t>(cbcr), c + b);
        __builtin_nontemporal_store(static_cast<uint8_t>(cbcr >> 8), c + v_plane_offset(p) + b);
      } else {
        __builtin_nontemporal_store(static_cast<uint16_t>(cbcr), reinterpret_cast<uint16_t *>(c + 2u * b));
      }
      uint8_t *a0 = a.y + static_cast<size_t>(2 * rp) * a.y_stride;
      __builtin_nontemporal_store(static_cast<uint16_t>(atop), reinterpret_cast<uint16_t *>(a0 + 2u * b));
      __builtin_nontemporal_store(static_cast<uint16_t>(abot), reinterpret_cast<uint16_t *>(a0 + a.y_stride + 2u * b));
      if (a.with_cbcr) {
        uint8_t *ac = a.cbcr + static_cast<size_t>(rp) * a.cbcr_stride;
        if (LAYOUT == kChromaI420) {
          __builtin_nontemporal_store(static_cast<uint8_t>(0x80), ac + b);
          __builtin_nontemporal_store(static_cast<uint8_t>(0x80), ac + v_plane_offset(a) + b);
        } else {
          __builtin_nontemporal_store(static_cast<uint16_t>(0x8080), reinterpret_cast<uint16_t *>(ac + 2u * b));
        }
      }
    }
    top = ntop;
    bot = nbot;
  }
}

// General layout, the twin of encode_rgba16f_blocks with the rider: one lane per 2x2 block, 8-byte loads (a texel), byte stores: any
// even W and H, texels 8-byte aligned, the five planes at any alignment.  grid = (block tiles, row pairs, pairs), grid-strided in x.
// BOUNDS: bx < W/2 and rp = blockIdx.y < H/2: texels 2 bx and 2 bx + 1 of rows 2 rp and 2 rp + 1; bytes 2 bx and 2 bx + 1 of those
// rows of either Y plane, bytes 2 bx, 2 bx + 1 of row rp of either CbCr plane (I420: byte bx of the U and of the V row).
template <uint32_t LAYOUT>
__global__ void __launch_bounds__(kBlockThreads)
encode_rgba16f_alpha_blocks(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const EncodeLds t = stage_from_linear(lds_raw, p);
  stage_alpha_luma(half_pair_alpha_lut(lds_raw, p), p);
  __syncthreads();
  const LdsBytePtr ta = half_pair_alpha_table(p);
  AlphaPlanes a;
  const EncodeFrame f = pair_frame(p, blockIdx.z, a);
  const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);
  const uint32_t bw = p.width >> 1;
  const uint32_t rp = blockIdx.y;
  for (uint32_t bx = blockIdx.x * blockDim.x + threadIdx.x; bx < bw; bx += gridDim.x * blockDim.x) {
    const u32x2 *r0 = reinterpret_cast<const u32x2 *>(f.bgra + static_cast<size_t>(2 * rp) * p.bgra_stride);
    const u32x2 *r1 = reinterpret_cast<const u32x2 *>(f.bgra + static_cast<size_t>(2 * rp + 1) * p.bgra_stride);
    const u32x2 tl = r0[2 * bx], tr = r0[2 * bx + 1], bl = r1[2 * bx], br = r1[2 * bx + 1];
    u32x4 top, bot;
    top.x = tl.x, top.y = tl.y, top.z = tr.x, top.w = tr.y;
    bot.x = bl.x, bot.y = bl.y, bot.z = br.x, bot.w = br.y;
    uint8_t *a0 = a.y + static_cast<size_t>(2 * rp) * a.y_stride + 2u * bx;
    uint8_t *a1 = a0 + a.y_stride;
    __builtin_nontemporal_store(static_cast<uint8_t>(half_alpha_luma(ta, half_sat<1>(top.y))), a0);
    __builtin_nontemporal_store(static_cast<uint8_t>(half_alpha_luma(ta, half_sat<1>(top.w))), a0 + 1);
    __builtin_nontemporal_store(static_cast<uint8_t>(half_alpha_luma(ta, half_sat<1>(bot.y))), a1);
    __builtin_nontemporal_store(static_cast<uint8_t>(half_alpha_luma(ta, half_sat<1>(bot.w))), a1 + 1);
    if (a.with_cbcr) {  // two bytes of 128, the second kept a value of its own so that both stay byte stores (second_byte)
      uint8_t *ac = a.cbcr + static_cast<size_t>(rp) * a.cbcr_stride;
      __builtin_nontemporal_store(static_cast<uint8_t>(0x80), LAYOUT == kChromaI420 ? ac + bx : ac + 2 * bx);
      __builtin_nontemporal_store(second_byte<kChromaI420>(0x8080u), LAYOUT == kChromaI420 ? ac + v_plane_offset(a) + bx : ac + 2 * bx + 1);
    }
    float v[6];
    encode_half_block(t, p.from_linear_scale, quarter_n, top, bot, v);
    uint32_t ytop, ybot, cbcr;
    quantize_block(v, ytop, ybot, cbcr);
    uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    uint8_t *y1 = y0 + p.y_stride;
    // byte stores, whatever the alignment; non-temporal as the fast kernel's (second_byte<kChromaI420> keeps byte 1 a value of its own)
    __builtin_nontemporal_store(static_cast<uint8_t>(ytop), y0 + 2 * bx);
    __builtin_nontemporal_store(second_byte<kChromaI420>(ytop), y0 + 2 * bx + 1);
    __builtin_nontemporal_store(static_cast<uint8_t>(ybot), y1 + 2 * bx);
    __builtin_nontemporal_store(second_byte<kChromaI420>(ybot), y1 + 2 * bx + 1);
    uint8_t *c = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;
    uint8_t *cr = LAYOUT == kChromaI420 ? c + v_plane_offset(p) + bx : c + 2 * bx + 1;
    __builtin_nontemporal_store(static_cast<uint8_t>(cbcr), LAYOUT == kChromaI420 ? c + bx : c + 2 * bx);
    __builtin_nontemporal_store(second_byte<kChromaI420>(cbcr), cr);
  }
}

}  // namespace bt709
