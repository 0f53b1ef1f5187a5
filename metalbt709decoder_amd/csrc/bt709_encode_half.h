// The half-input encoder's kernels (BT709HIP_CTX_OPT_ENCODE_HALF_INPUT); included by bt709_encode.hip alone, behind the
// helpers it shares with the BGRA8 encoder's kernels (from_linear, quant_arg, div_const, quantize_block, encode_frame, v_plane_offset ...).
//
// RGBA16Float linear-light texels -> 4:2:0 NV12 / I420, the mirror of decode_nv12_rgba16f (bt709_rgba16f.hip): 8 B read and 1.5 B
// written per pixel.  Per 2x2 block (pixels TL, TR, BL, BR; a texel is binary16 R, G, B, A in memory order, A is not read) this is
// BT709_average_pixel_values (Renderer/BT709.h:1349-1509) with the result of BT709_tolinearNorm replaced by the texel's own values:
//   v[i][c]    = sat(float(h[i][c]))                  exact half -> float; NaN -> 0, v < 0 -> 0, v > 1 -> 1
//   byte[i][c] = BT709_from_linear(v[i][c], outputGamma)                       BT709.h:1150-1167
//   Y[i]       = Y of sRGB_from_sRGB_convertRGBToYCbCr(byte[i][R,G,B])         BT709.h:914-944 -> 199-268
//   ave[c]     = (((v[0][c] + v[1][c]) + v[2][c]) + v[3][c]) / 4.0f            BT709.h:1171-1190
//   (Cb, Cr)   = Cb, Cr of sRGB_from_sRGB_convertRGBToYCbCr(BT709_from_linear(ave[c], outputGamma))
//
// Arithmetic:
//   * conversion and saturation are ONE instruction: v_cvt_f32_f16 with the clamp bit.  Under DX10_CLAMP (the mode every HIP kernel
//     runs in) the clamp turns NaN into 0 whatever MODE.ieee holds, which v_max / v_min / v_med3 do not promise; SDWA selects the
//     upper half of a dword (G) in the same instruction.  Subnormal halves convert exactly (half denormals are on by default);
//   * there is no per-byte table: every pixel channel goes through the two-resolution BT709_from_linear table (bt709_split_lookup.h,
//     equal to the reference for every float in [0, 1]), as the 2x2 average does.  Against a byte table indexed by the saturated half
//     code (15361 entries): see profiles/LAB.md, round 19;
//   * v * n_fine and sum * (0.25 * n_fine) are exact (powers of two); every other product and sum is a single rounded operation in
//     the reference's order (no contraction); div_const's two FMAs are the division's own correction steps (bt709_encode.hip).
//
// Shape: encode_bgra's row-pair walk (tables staged once per workgroup, the next pair's loads issued ahead of the arithmetic, lanes
// past the row's end clamped, stores predicated), with a 2x2 BLOCK per lane instead of a quad: a lane reads two 16-byte rows (two
// texels each) and consecutive lanes read consecutive 16 bytes, so a wave's load covers 1 KiB of one row; it writes 2 + 2 bytes of Y
// and 2 of CbCr (I420: 1 + 1), a wave 128 contiguous bytes per store.  LDS: the from_linear table alone (6-10 KiB), at address 0.
#pragma once

namespace bt709 {
namespace {

// sat(float(half)) of the lower (HI = 0) or upper (HI = 1) 16 bits of a dword
template <int HI>
__device__ __forceinline__ float half_sat(uint32_t word) {
  float v;
  if (HI) asm("v_cvt_f32_f16_sdwa %0, %1 clamp dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(v) : "v"(word));
  else asm("v_cvt_f32_f16_sdwa %0, %1 clamp dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0" : "=v"(v) : "v"(word));
  return v;
}

// the from_linear table at LDS address 0 (these kernels have no static LDS; trapped if that ever changes, as stage_encode_tables does)
__device__ __forceinline__ EncodeLds stage_from_linear(unsigned char *lds_raw, const EncodeParams &p) {
  u32x4 *d = reinterpret_cast<u32x4 *>(lds_raw);
  const u32x4 *sf = reinterpret_cast<const u32x4 *>(p.from_linear);
  stage_batched(d, p.from_linear_bytes / 16, threadIdx.x, blockDim.x, [&](uint32_t i) { return sf[i]; });
  if (static_cast<uint32_t>(reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char *)lds_raw)) != 0u)
    __builtin_trap();
  EncodeLds t;
  t.fl = 0u;
  t.offset = p.from_linear_offset;
  t.coarse_shift = split_coarse_shift(__float_as_uint(p.from_linear_coarse));
  t.three = 0u;  // no SDWA byte select here
  return t;
}

// byteNorm(BT709_from_linear(x)) of xs = x * n_fine (or the sum of four times n_fine / 4)
__device__ __forceinline__ float encoded_norm(const EncodeLds &t, float xs) {
  return __fmul_rn(static_cast<float>(from_linear(t, xs)), kInv255);
}

// one 2x2 block: top / bot = the two texels of its upper / lower row, each {R | G << 16, B | A << 16};
// v = {Y tl, Y tr, Y bl, Y br, Cb, Cr} ready for truncation, as encode_block's
__device__ __forceinline__ void encode_half_block(const EncodeLds &t, float fl_n, float fl_quarter_n, const u32x4 top, const u32x4 bot, float v[6]) {
  const uint32_t rg[4] = {top.x, top.z, bot.x, bot.z}, ba[4] = {top.y, top.w, bot.y, bot.w};
  float sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float r = half_sat<0>(rg[i]), g = half_sat<1>(rg[i]), b = half_sat<0>(ba[i]);
    sr = i ? __fadd_rn(sr, r) : r;
    sg = i ? __fadd_rn(sg, g) : g;
    sb = i ? __fadd_rn(sb, b) : b;
    const float rn = encoded_norm(t, __fmul_rn(r, fl_n)), gn = encoded_norm(t, __fmul_rn(g, fl_n)), bn = encoded_norm(t, __fmul_rn(b, fl_n));
    const float ey = __fadd_rn(__fadd_rn(__fmul_rn(kKr, rn), __fmul_rn(kKg, gn)), __fmul_rn(kKb, bn));  // BT709.h:222
    v[i] = quant_arg(ey, static_cast<float>(kYMax - kYMin), 16.0f);                                      // BT709.h:233, 244
  }
  const float rn = encoded_norm(t, __fmul_rn(sr, fl_quarter_n)), gn = encoded_norm(t, __fmul_rn(sg, fl_quarter_n)), bn = encoded_norm(t, __fmul_rn(sb, fl_quarter_n));
  const float ey = __fadd_rn(__fadd_rn(__fmul_rn(kKr, rn), __fmul_rn(kKg, gn)), __fmul_rn(kKb, bn));
  const float eb = div_const(__fadd_rn(bn, -ey), kCbSpan, kRcCb);                      // BT709.h:223
  const float er = div_const(__fadd_rn(rn, -ey), kCrSpan, kRcCr);                      // BT709.h:224
  v[4] = quant_arg(eb, static_cast<float>(kCMax - kCMin), 128.0f);                     // BT709.h:234, 245
  v[5] = quant_arg(er, static_cast<float>(kCMax - kCMin), 128.0f);                     // BT709.h:235, 246
}

}  // namespace

// Preconditions of the fast kernel (checked by the host shim): width even (every valid call); the texel pointer and pitch 16-byte
// aligned; the Y pointer and pitch 2-byte aligned; NV12: the CbCr pointer and pitch 2-byte aligned; I420: none on U and V (byte
// stores).  grid = (tiles, row-pair groups, frames), as encode_bgra, a tile being blockDim.x BLOCKS (2 blockDim.x pixels) wide.
// BOUNDS: b <= blocks - 1 = W/2 - 1, so a lane reads bytes [16 b, 16 b + 15] <= 8 W - 1 of a row of 8 W bytes, rows 2 rp and
// 2 rp + 1 with rp < H/2; only lanes with b_raw < blocks store, bytes [2 b, 2 b + 1] <= W - 1 of a Y or CbCr row (I420: byte b of a
// U or V row of W/2).
template <uint32_t LAYOUT>
__global__ void __launch_bounds__(kMaxBlockThreads)
encode_rgba16f(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const BandedWork work = banded_work(p.xcd_bands, p.frames_per_band);  // XCD-aware work map: bt709_tile.h
  const EncodeFrame f = encode_frame(p, work.frame);
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
  __syncthreads();
  const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);

  for (uint32_t rp = rp0; rp < rp_end; ++rp) {
    u32x4 ntop = top, nbot = bot;
    if (rp + 1 < rp_end) {  // nothing on the workgroup's last pair, as encode_bgra
      const uint8_t *s1 = f.bgra + static_cast<size_t>(2 * (rp + 1)) * p.bgra_stride;
      ntop = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + 16u * b));
      nbot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + p.bgra_stride + 16u * b));
    }
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
    }
    top = ntop;
    bot = nbot;
  }
}

// General layout: one lane per 2x2 block, 8-byte loads (a texel), byte stores: any even W and H, texels 8-byte aligned, planes at
// any alignment.  grid = (block tiles, row pairs, frames), grid-strided in x, as encode_bgra_blocks.
template <uint32_t LAYOUT>
__global__ void __launch_bounds__(kBlockThreads)
encode_rgba16f_blocks(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const EncodeLds t = stage_from_linear(lds_raw, p);
  __syncthreads();
  const EncodeFrame f = encode_frame(p, blockIdx.z);
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
