// The per-pixel converter's kernels (BT709HIP_CTX_OPT_ENCODE_CONVERT); included by bt709_encode.hip alone, behind the
// helpers it shares with the encoder's kernels (div_const, quant_arg, quantize_quad, store_quad_chroma, texel, encode_frame ...).
//
// Restates +convert: (Renderer/BGRAToBT709Converter.h:34-46, .m:31-59 -> convertSoftware), per pixel and in floats end to end:
//   n[c]        = curve[byte c]                                   transfer_tables.h build_convert_curve (LUT, exact)
//   Ey          = (Kr*R + Kg*G) + Kb*B                            BT709.h:222
//   Eb, Er      = (B - Ey) / 1.8556f, (R - Ey) / 1.5748f          BT709.h:223-224
//   Y, Cb, Cr   = round(Ey*219 + 16), round(E*224 + 128)          BT709.h:233-246
//   word        = (Cr << 16) | (Cb << 8) | Y                      BGRAToBT709Converter.m:52-56
// kFormPacked instantiations store the words (BT709HIP_CONVERT_PACKED444); the others are +convert: followed by
// copyBT709ToCoreVideo (BGRAToBT709Converter.m:1042-1099) with no packed intermediate (BT709HIP_CONVERT_POINT420): every pixel's Y,
// and for each 2x2 block the Cb, Cr of the pixel in its ODD row and EVEN column -- every row of the reference's copy overwrites
// chroma row `row / 2`, so the odd row's pair is what remains.
//
// div_const's exhaustive proof covers 1e-30 <= |x| <= 4.  Its operands here are B - Ey and R - Ey with R, G, B curve values:
// each is 0 or lies in [3.0e-4, 1 + 2^-22] for all four curves (smallest non-zero entry: LINEAR's srgb_to_linear(1/255) =
// 3.035e-4; largest: ITU709's 1.099 * 1 - 0.099 narrowed to float), Ey is a convex combination of them up to three roundings, so
// |x| <= 1.0001; a non-zero Ey is at least Kb * 3.0e-4 = 2.2e-5, and a non-zero difference of two floats that are 0 or at least
// that large is at least one ulp of the smaller, 2^-39: inside the range.  A zero operand only differs in the sign of zero, which
// "+ 128" erases.
//
// Shape: encode_bgra's / encode_bgra_blocks' -- same tile, work map, row-pair walk, prefetch, lane clamp and launch plan.  LDS is the
// 1 KiB curve alone (static, so the dynamic segment of the launch is empty); per pixel three byte-select lookups (one SDWA shift
// and one ds_read_b32 each), 5 mul + 4 add for Ey / Y, and per chroma pair 2 sub, 2 x (mul + 2 fma), 2 x (mul + 2 add).
#pragma once

namespace bt709 {
namespace {

typedef __attribute__((address_space(3))) const float *LdsFloatPtr;  // one ds_read_b32, the table's base in the offset field

struct ConvertLds {
  uint32_t base;  // LDS address of curve[0]
  uint32_t two;   // VGPR holding 2: SDWA operands cannot be inline constants
};

__device__ __forceinline__ ConvertLds stage_convert_curve(float *curve, const EncodeParams &p) {
  // 256 floats = 64 x 16 bytes: the first wave (every workgroup has one)
  if (threadIdx.x < 64) reinterpret_cast<u32x4 *>(curve)[threadIdx.x] = reinterpret_cast<const u32x4 *>(p.convert_curve)[threadIdx.x];
  ConvertLds t;
  t.base = static_cast<uint32_t>(reinterpret_cast<size_t>((__attribute__((address_space(3))) float *)curve));
  t.two = 2u;
  asm("" : "+v"(t.two));
  return t;
}

// curve[byte LANE of a BGRA word]: v_lshlrev_b32_sdwa selects the byte and scales it to the 4-byte entry in one instruction
template <int LANE>
__device__ __forceinline__ float curve_entry(const ConvertLds &t, uint32_t word) {
  uint32_t a;
  if (LANE == 0)
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(a) : "v"(t.two), "v"(word));
  else if (LANE == 1)
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(a) : "v"(t.two), "v"(word));
  else
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(a) : "v"(t.two), "v"(word));
  return *reinterpret_cast<LdsFloatPtr>(a + t.base);
}

// A row's base address held in scalar registers: the loop's loads and stores then take it as their SGPR base and the lane's 32-bit
// byte offset as their only VGPR operand (without this the compiler turns the row walk into per-lane 64-bit pointers and advances
// them with VALU adds)
#define BT709_GLOBAL __attribute__((address_space(1)))  // the rebuilt pointer says so itself: nothing is left to infer it from
template <typename T>
__device__ __forceinline__ BT709_GLOBAL T *uniform_row(T *row) {
  const uint64_t a = reinterpret_cast<uint64_t>(row);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(a)), hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(a >> 32));
  return reinterpret_cast<BT709_GLOBAL T *>(static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32));
}

// One pixel.  v = {Y, Cb, Cr} ready for truncation; CHROMA = false: v[0] alone
template <bool CHROMA>
__device__ __forceinline__ void convert_pixel(const ConvertLds &t, uint32_t word, float *v) {
  const float r = curve_entry<2>(t, word), g = curve_entry<1>(t, word), b = curve_entry<0>(t, word);
  const float ey = __fadd_rn(__fadd_rn(__fmul_rn(kKr, r), __fmul_rn(kKg, g)), __fmul_rn(kKb, b));  // BT709.h:222
  v[0] = quant_arg(ey, static_cast<float>(kYMax - kYMin), 16.0f);                                   // BT709.h:233, 244
  if (CHROMA) {
    const float eb = div_const(__fadd_rn(b, -ey), kCbSpan, kRcCb);        // BT709.h:223
    const float er = div_const(__fadd_rn(r, -ey), kCrSpan, kRcCr);        // BT709.h:224
    v[1] = quant_arg(eb, static_cast<float>(kCMax - kCMin), 128.0f);      // BT709.h:234, 245
    v[2] = quant_arg(er, static_cast<float>(kCMax - kCMin), 128.0f);      // BT709.h:235, 246
  }
}

// Truncate the {Y, Cb, Cr} of four pixels and place each triple in its word: Y in byte 0, Cb in 1, Cr in 2, byte 3 zero.  One asm
// statement per four words: the conversions must not be separated from the mode switch around them (quantize_quad_lanes).
__device__ __forceinline__ u32x4 quantize_words(const float v[12]) {
  uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
  asm("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\t"
      "v_cvt_pk_u8_f32 %0, %4, 0, %0\n\tv_cvt_pk_u8_f32 %0, %5, 1, %0\n\tv_cvt_pk_u8_f32 %0, %6, 2, %0\n\t"
      "v_cvt_pk_u8_f32 %1, %7, 0, %1\n\tv_cvt_pk_u8_f32 %1, %8, 1, %1\n\tv_cvt_pk_u8_f32 %1, %9, 2, %1\n\t"
      "v_cvt_pk_u8_f32 %2, %10, 0, %2\n\tv_cvt_pk_u8_f32 %2, %11, 1, %2\n\tv_cvt_pk_u8_f32 %2, %12, 2, %2\n\t"
      "v_cvt_pk_u8_f32 %3, %13, 0, %3\n\tv_cvt_pk_u8_f32 %3, %14, 1, %3\n\tv_cvt_pk_u8_f32 %3, %15, 2, %3\n\t"
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0"
      : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3)
      : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]), "v"(v[8]), "v"(v[9]), "v"(v[10]),
        "v"(v[11]));
  u32x4 w;
  w.x = w0, w.y = w1, w.z = w2, w.w = w3;
  return w;
}

__device__ __forceinline__ u32x4 convert_words(const ConvertLds &t, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  float v[12];
  convert_pixel<true>(t, a, v);
  convert_pixel<true>(t, b, v + 3);
  convert_pixel<true>(t, c, v + 6);
  convert_pixel<true>(t, d, v + 9);
  return quantize_words(v);
}

// one 2x2 block of the point-sampled 4:2:0 form: p and v as encode_block's; the chroma is the bottom-left pixel's
__device__ __forceinline__ void convert_block(const ConvertLds &t, const uint32_t p[4], float v[6]) {
  float bl[3];
  convert_pixel<false>(t, p[0], v + 0);
  convert_pixel<false>(t, p[1], v + 1);
  convert_pixel<true>(t, p[2], bl);
  convert_pixel<false>(t, p[3], v + 3);
  v[2] = bl[0], v[4] = bl[1], v[5] = bl[2];
}

}  // namespace

// FORM = chroma layout | kFormStraight | kFormPacked.  The packed instantiations exist under kChromaNV12 alone (they write no plane).
// Preconditions of the fast kernel (checked by the host shim): width % 4 == 0, BGRA pointer and pitch 16-byte aligned; packed: the
// word pointer and pitch 16-byte aligned; else the encoder's (Y 4-byte; CbCr 4-byte, or U and the chroma pitch 2-byte).
// grid = (tiles, row-pair groups, frames), as encode_bgra.
template <uint32_t FORM>
__global__ void __launch_bounds__(kMaxBlockThreads)
convert_bgra(const EncodeParams p) {
  __shared__ __attribute__((aligned(16))) float curve[256];
  constexpr uint32_t LAYOUT = form_layout(FORM);
  const BandedWork work = banded_work(p.xcd_bands, p.frames_per_band);
  const EncodeFrame f = encode_frame(p, work.frame);
  const uint32_t quads = p.width >> 2;
  const uint32_t row_pairs = p.height >> 1;
  const uint32_t q_raw = work.tile * blockDim.x + threadIdx.x;
  const uint32_t q = min(q_raw, quads - 1);
  const uint32_t rp0 = blockIdx.y * p.row_pairs_per_block;
  const uint32_t rp_end = min(rp0 + p.row_pairs_per_block, row_pairs);

  // row pointers are uniform (SGPR base), the lane adds a 32-bit offset: no 64-bit VALU address arithmetic
  const uint8_t *s0 = f.bgra + static_cast<size_t>(2 * rp0) * p.bgra_stride;
  u32x4 top = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + 16u * q));
  u32x4 bot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + p.bgra_stride + 16u * q));

  const ConvertLds t = stage_convert_curve(curve, p);  // after the first loads are in flight
  __syncthreads();

  for (uint32_t rp = rp0; rp < rp_end; ++rp) {
    // the lane's byte offsets, kept inside the loop body (volatile: not hoisted) so that each access sees a 32-bit offset to extend
    uint32_t in16 = 16u * q, out4 = 4u * q;
    asm volatile("" : "+v"(in16), "+v"(out4));
    u32x4 ntop = top, nbot = bot;
    if (rp + 1 < rp_end) {  // nothing on the workgroup's last pair, as encode_bgra
      const BT709_GLOBAL uint8_t *s1 = uniform_row(f.bgra + static_cast<size_t>(2 * (rp + 1)) * p.bgra_stride);
      const BT709_GLOBAL uint8_t *s2 = s1 + p.bgra_stride;
      ntop = __builtin_nontemporal_load(reinterpret_cast<const BT709_GLOBAL u32x4 *>(s1 + in16));
      nbot = __builtin_nontemporal_load(reinterpret_cast<const BT709_GLOBAL u32x4 *>(s2 + in16));
    }
    if constexpr (form_straight(FORM)) {  // behind the prefetch, ahead of everything that reads a texel
      premultiply_row(top);
      premultiply_row(bot);
    }
    BT709_GLOBAL uint8_t *y0 = uniform_row(f.y + static_cast<size_t>(2 * rp) * p.y_stride);
    BT709_GLOBAL uint8_t *y1 = y0 + p.y_stride;
    if constexpr (form_packed(FORM)) {
      const u32x4 wtop = convert_words(t, top.x, top.y, top.z, top.w);
      const u32x4 wbot = convert_words(t, bot.x, bot.y, bot.z, bot.w);
      if (q_raw < quads) {
        __builtin_nontemporal_store(wtop, reinterpret_cast<BT709_GLOBAL u32x4 *>(y0 + 4u * out4));
        __builtin_nontemporal_store(wbot, reinterpret_cast<BT709_GLOBAL u32x4 *>(y1 + 4u * out4));
      }
    } else {
      float va[6], vb[6];
      {
        const uint32_t blk[4] = {top.x, top.y, bot.x, bot.y};
        convert_block(t, blk, va);
      }
      {
        const uint32_t blk[4] = {top.z, top.w, bot.z, bot.w};
        convert_block(t, blk, vb);
      }
      uint32_t ytop, ybot, cbcr;
      quantize_quad<LAYOUT>(va, vb, ytop, ybot, cbcr);
      if (q_raw < quads) {
        __builtin_nontemporal_store(ytop, reinterpret_cast<BT709_GLOBAL uint32_t *>(y0 + out4));
        __builtin_nontemporal_store(ybot, reinterpret_cast<BT709_GLOBAL uint32_t *>(y1 + out4));
        store_quad_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, q, cbcr);
      }
    }
    top = ntop;
    bot = nbot;
  }
}

// General layout: one lane per 2x2 block, dword loads; packed: dword stores (the words are 4-byte aligned by contract), else byte
// stores at any alignment, as encode_bgra_blocks.
template <uint32_t FORM>
__global__ void __launch_bounds__(kBlockThreads)
convert_bgra_blocks(const EncodeParams p) {
  __shared__ __attribute__((aligned(16))) float curve[256];
  constexpr uint32_t LAYOUT = form_layout(FORM);
  const ConvertLds t = stage_convert_curve(curve, p);
  __syncthreads();
  const EncodeFrame f = encode_frame(p, blockIdx.z);
  const uint32_t bw = p.width >> 1;
  const uint32_t rp = blockIdx.y;
  for (uint32_t bx = blockIdx.x * blockDim.x + threadIdx.x; bx < bw; bx += gridDim.x * blockDim.x) {
    const uint32_t *r0 = reinterpret_cast<const uint32_t *>(f.bgra + static_cast<size_t>(2 * rp) * p.bgra_stride);
    const uint32_t *r1 = reinterpret_cast<const uint32_t *>(f.bgra + static_cast<size_t>(2 * rp + 1) * p.bgra_stride);
    const uint32_t blk[4] = {texel<FORM>(r0[2 * bx]), texel<FORM>(r0[2 * bx + 1]), texel<FORM>(r1[2 * bx]), texel<FORM>(r1[2 * bx + 1])};
    uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    uint8_t *y1 = y0 + p.y_stride;
    if constexpr (form_packed(FORM)) {
      const u32x4 w = convert_words(t, blk[0], blk[1], blk[2], blk[3]);
      reinterpret_cast<uint32_t *>(y0)[2 * bx] = w.x;
      reinterpret_cast<uint32_t *>(y0)[2 * bx + 1] = w.y;
      reinterpret_cast<uint32_t *>(y1)[2 * bx] = w.z;
      reinterpret_cast<uint32_t *>(y1)[2 * bx + 1] = w.w;
    } else {
      float v[6];
      convert_block(t, blk, v);
      uint32_t ytop, ybot, cbcr;
      quantize_block(v, ytop, ybot, cbcr);
      y0[2 * bx] = static_cast<uint8_t>(ytop);
      y0[2 * bx + 1] = second_byte<LAYOUT>(ytop);
      y1[2 * bx] = static_cast<uint8_t>(ybot);
      y1[2 * bx + 1] = second_byte<LAYOUT>(ybot);
      store_block_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, bx, static_cast<uint8_t>(cbcr), static_cast<uint8_t>(cbcr >> 8));
    }
  }
}

#undef BT709_GLOBAL

}  // namespace bt709
