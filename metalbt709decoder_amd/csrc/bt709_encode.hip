// CDNA4 (gfx950) kernel of the step BEFORE the decode path: 8-bit BGRA -> 4:2:0 NV12
// BT.709 video range, with the reference's linear-light 2x2 chroma averaging.
//
// Restates, per 2x2 block, cvpbu_ycbcr_subsample (Renderer/CVPixelBufferUtils.h:241-399)
// -> BT709_average_pixel_values (Renderer/BT709.h:1349-1509):
//   lin[i][c]  = BT709_tolinearNorm(byte)                      BT709.h:1100-1146   (LUT, exact)
//   ave[c]     = (((l0 + l1) + l2) + l3) / 4.0f                BT709.h:1171-1190, 1404-1406
//   avgByte[c] = BT709_from_linear(ave[c], outputGamma)         BT709.h:1150-1167   (bucket table, exact)
//   (., Cb, Cr) = sRGB_from_sRGB_convertRGBToYCbCr(avgByte)     BT709.h:914-944 -> 199-268
//   Y[i]       = sRGB_from_sRGB_convertRGBToYCbCr(BT709_from_linear(lin[i][c], outputGamma))[0]
//                                                               BT709.h:1423-1487   (per-byte LUT, exact)
// with the matrix of BT709.h:222-246: Ey = (Kr*R + Kg*G) + Kb*B, Eb = (B-Ey)/1.8556f,
// Er = (R-Ey)/1.5748f, Y = round(Ey*219 + 16), C = round(E*224 + 128).
//
// Exactness notes:
//   * the per-byte LUT holds {lin, byteNorm(encoded byte)} -- one 2 KiB table for the three channels
//     (a 6 KiB version with the K_c products folded in saved three 2-cycle multiplies per pixel and
//     cost 4 KiB more staging per workgroup);
//   * x / c for the two constant divisors is computed as q0 = x*rc, q = fma(fma(-c, q0, x), rc, q0)
//     with rc = fl(1/c): this equals the correctly rounded quotient for EVERY float with
//     1e-30 <= |x| <= 4 (exhaustive check over all 2^32 patterns: tools/div_exact.hip, run by
//     tests/test_encoder.py); operands here are in [-1.1, 1.1], and a zero operand only differs in
//     the sign of zero, which the following "+ 128" erases.  These two FMAs are the division's own
//     error-correction steps, not a contracted multiply-add of the reference's expression;
//   * round() of a positive float v < 256 is trunc(v + 0.5f), and v + 0.5f is exact there (a sum
//     that moves into the next binade lands in [2^m, 2^m + 1/2), where rounding cannot reach the
//     next integer).  v_cvt_pk_u8_f32 converts AND places the byte in its lane of the output word;
//     it rounds to nearest even by default (so 209 / 193 / 283 of the 2^24 Y / Cb / Cr inputs, the
//     exact ties, would come out one low) but honours MODE.fp_round (tools/cvt_probe.hip), so the
//     twelve conversions of a quad sit in one asm statement under round-toward-zero.
//
// VALU budget (tools/valu_ops.hip): only v_add/mul/mov_f32 are 2-cycle instructions on gfx950,
// everything else this kernel uses costs 4, and at 1 Tpixel/s the VALU is ~70 % busy: the byte
// -> LUT address is one SDWA shift (byte select + << 3, table bases in the ds_read offset field)
// instead of bfe + shift-add, the split-table index is a min() of the two index functions.
//
// A lane owns a 4x2-pixel quad (two blocks): two 16-byte loads, three 4-byte stores; lanes
// of a wave are consecutive quads of one row pair; grid = (tiles, row-pair groups, frames).  LDS holds
// the 2 KiB per-byte table and the two-resolution BT709_from_linear table.
//
// The same pictures as three planes (I420: Y, U, V -- the YUV4MPEG2 FRAME payload) come from the same kernels: each is a template
// on the layout; only the placement of a quad's four chroma bytes and their stores differ.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bt709_constants.h"
#include "bt709_launch.h"
#include "bt709_premultiply.h"
#include "bt709_split_lookup.h"
#include "bt709_stage.h"
#include "bt709_tile.h"

namespace bt709 {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr float kRcCb = 1.0f / kCbSpan;  // fl(1/1.8556f)
constexpr float kRcCr = 1.0f / kCrSpan;  // fl(1/1.5748f)

__device__ __forceinline__ float div_const(float x, float c, float rc) {
  const float q0 = __fmul_rn(x, rc);
  return __fmaf_rn(__fmaf_rn(-c, q0, x), rc, q0);
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const u32x2 *LdsPairPtr;  // one ds_read_b64, base in the offset field

struct EncodeLds {
  // The per-byte table sits at LDS address 0: these kernels have no static LDS, so the dynamic
  // segment starts at 0 -- stage_encode_tables traps if that ever changes.
  uint32_t fl;     // ... of the two-resolution BT709_from_linear table (transfer_tables.h SplitTable)
  uint32_t offset, coarse_shift;
  uint32_t three;  // VGPR holding 3: SDWA operands cannot be inline constants
};

// {lin, enc_norm} of byte LANE of a BGRA word: v_lshlrev_b32_sdwa selects the byte and scales it to
// the 8-byte entry in one instruction
template <int LANE>
__device__ __forceinline__ u32x2 byte_entry(const EncodeLds &t, uint32_t word) {
  uint32_t a;
  if (LANE == 0)
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(a) : "v"(t.three), "v"(word));
  else if (LANE == 1)
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(a) : "v"(t.three), "v"(word));
  else
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(a) : "v"(t.three), "v"(word));
  return *reinterpret_cast<LdsPairPtr>(a);
}

// BT709_from_linear through the two-resolution table in LDS: the arithmetic is bt709_split_lookup.h's (shared with the
// every-float host sweep), the ds_read_b64 is this file's
__device__ __forceinline__ uint32_t from_linear(const EncodeLds &t, float xs) {
  return split_table_lookup(xs, t.coarse_shift, t.offset, [&](uint32_t q) {
    const u32x2 e = *reinterpret_cast<LdsPairPtr>((q << 3) + t.fl);
    return TransferBucket{__uint_as_float(e.x), e.y};
  });
}

// v = e * scale + offset as the reference's float expression, plus the exact 0.5f: trunc(result)
// is (int)round(v)
__device__ __forceinline__ float quant_arg(float e, float scale, float offset) {
  return __fadd_rn(__fadd_rn(__fmul_rn(e, scale), offset), 0.5f);
}

// one 2x2 block: p = {top-left, top-right, bottom-left, bottom-right} BGRA words;
// v = {Y tl, Y tr, Y bl, Y br, Cb, Cr} ready for truncation
__device__ __forceinline__ void encode_block(const EncodeLds &t, float fl_quarter_n, const uint32_t p[4], float v[6]) {
  float sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u32x2 r = byte_entry<2>(t, p[i]);
    const u32x2 g = byte_entry<1>(t, p[i]);
    const u32x2 b = byte_entry<0>(t, p[i]);
    sr = i ? __fadd_rn(sr, __uint_as_float(r.x)) : __uint_as_float(r.x);
    sg = i ? __fadd_rn(sg, __uint_as_float(g.x)) : __uint_as_float(g.x);
    sb = i ? __fadd_rn(sb, __uint_as_float(b.x)) : __uint_as_float(b.x);
    const float ey = __fadd_rn(__fadd_rn(__fmul_rn(kKr, __uint_as_float(r.y)), __fmul_rn(kKg, __uint_as_float(g.y))),
                               __fmul_rn(kKb, __uint_as_float(b.y)));  // BT709.h:222
    v[i] = quant_arg(ey, static_cast<float>(kYMax - kYMin), 16.0f);                                            // BT709.h:233, 244
  }
  // ave = sum / 4.0f, then scaled into the table's domain: sum * (0.25 * N), both powers of two
  const float rn = __fmul_rn(static_cast<float>(from_linear(t, __fmul_rn(sr, fl_quarter_n))), kInv255);
  const float gn = __fmul_rn(static_cast<float>(from_linear(t, __fmul_rn(sg, fl_quarter_n))), kInv255);
  const float bn = __fmul_rn(static_cast<float>(from_linear(t, __fmul_rn(sb, fl_quarter_n))), kInv255);
  const float ey = __fadd_rn(__fadd_rn(__fmul_rn(kKr, rn), __fmul_rn(kKg, gn)), __fmul_rn(kKb, bn));
  const float eb = div_const(__fadd_rn(bn, -ey), kCbSpan, kRcCb);                      // BT709.h:223
  const float er = div_const(__fadd_rn(rn, -ey), kCrSpan, kRcCr);                      // BT709.h:224
  v[4] = quant_arg(eb, static_cast<float>(kCMax - kCMin), 128.0f);                     // BT709.h:234, 245
  v[5] = quant_arg(er, static_cast<float>(kCMax - kCMin), 128.0f);                     // BT709.h:235, 246
}

// Truncate the twelve values of a quad (two blocks) and place them: Y rows top / bottom, and the four chroma bytes in one word,
// Cr of the first block in byte lane CR0 and Cb of the second in lane CB1 (quantize_quad below).  One asm statement: the
// conversions must not be separated from the mode switch around them.
template <int CR0, int CB1>
__device__ __forceinline__ void quantize_quad_lanes(const float a[6], const float b[6], uint32_t &ytop, uint32_t &ybot,
                                              uint32_t &cbcr) {
  ytop = ybot = cbcr = 0;
  asm("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\t"
      "v_cvt_pk_u8_f32 %0, %3, 0, %0\n\tv_cvt_pk_u8_f32 %0, %4, 1, %0\n\t"
      "v_cvt_pk_u8_f32 %1, %5, 0, %1\n\tv_cvt_pk_u8_f32 %1, %6, 1, %1\n\t"
      "v_cvt_pk_u8_f32 %2, %7, 0, %2\n\tv_cvt_pk_u8_f32 %2, %8, %15, %2\n\t"
      "v_cvt_pk_u8_f32 %0, %9, 2, %0\n\tv_cvt_pk_u8_f32 %0, %10, 3, %0\n\t"
      "v_cvt_pk_u8_f32 %1, %11, 2, %1\n\tv_cvt_pk_u8_f32 %1, %12, 3, %1\n\t"
      "v_cvt_pk_u8_f32 %2, %13, %16, %2\n\tv_cvt_pk_u8_f32 %2, %14, 3, %2\n\t"
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0"
      : "+v"(ytop), "+v"(ybot), "+v"(cbcr)
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]),
        "v"(b[4]), "v"(b[5]), "n"(CR0), "n"(CB1));
}

// NV12: Cb0 Cr0 Cb1 Cr1, Cb in the low byte (CVPixelBufferUtils.h:358-361) -- the CbCr plane's dword.
// I420: Cb0 Cb1 Cr0 Cr1 -- the low half is the U plane's two bytes, the high half the V plane's.  v_cvt_pk_u8_f32 takes the byte
// lane as an operand, so either placement costs the same twelve instructions.
template <uint32_t LAYOUT>
__device__ __forceinline__ void quantize_quad(const float a[6], const float b[6], uint32_t &ytop, uint32_t &ybot, uint32_t &cbcr) {
  if (LAYOUT == kChromaI420) quantize_quad_lanes<2, 1>(a, b, ytop, ybot, cbcr);
  else quantize_quad_lanes<1, 2>(a, b, ytop, ybot, cbcr);
}

// one block (general kernel): bytes 0,1 of each word
__device__ __forceinline__ void quantize_block(const float a[6], uint32_t &ytop, uint32_t &ybot, uint32_t &cbcr) {
  ytop = ybot = cbcr = 0;
  asm("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\t"
      "v_cvt_pk_u8_f32 %0, %3, 0, %0\n\tv_cvt_pk_u8_f32 %0, %4, 1, %0\n\t"
      "v_cvt_pk_u8_f32 %1, %5, 0, %1\n\tv_cvt_pk_u8_f32 %1, %6, 1, %1\n\t"
      "v_cvt_pk_u8_f32 %2, %7, 0, %2\n\tv_cvt_pk_u8_f32 %2, %8, 1, %2\n\t"
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0"
      : "+v"(ytop), "+v"(ybot), "+v"(cbcr)
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]));
}

__device__ __forceinline__ EncodeLds stage_encode_tables(unsigned char *lds_raw, const EncodeParams &p) {
  u32x4 *d = reinterpret_cast<u32x4 *>(lds_raw);
  const u32x4 *sb = reinterpret_cast<const u32x4 *>(p.per_byte);
  const u32x4 *sf = reinterpret_cast<const u32x4 *>(p.from_linear);
  const uint32_t nb = 256 * sizeof(EncodeByteEntry) / 16, nf = p.from_linear_bytes / 16;
  // (The first version staged a uniform 33 KiB BT709_from_linear table here -- ten dependent L2
  // round trips per workgroup -- and a version that left it in global memory was bound by the
  // 64-line gathers; the two-resolution table is 6-10 KiB.)
  stage_batched(d, nb + nf, threadIdx.x, blockDim.x, [&](uint32_t i) { return i < nb ? sb[i] : sf[i - nb]; });
  EncodeLds t;
  if (static_cast<uint32_t>(reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char *)lds_raw)) != 0u)
    __builtin_trap();
  t.fl = 256u * static_cast<uint32_t>(sizeof(EncodeByteEntry));
  t.offset = p.from_linear_offset;
  t.coarse_shift = split_coarse_shift(__float_as_uint(p.from_linear_coarse));
  t.three = 3u;
  asm("" : "+v"(t.three));
  return t;
}

__device__ __forceinline__ EncodeFrame encode_frame(const EncodeParams &p, uint32_t i) {
  if (!p.uniform) return p.frames[i];
  EncodeFrame f = p.frames[0];
  f.bgra += static_cast<int64_t>(i) * p.step_bgra;
  f.y += static_cast<int64_t>(i) * p.step_y;
  f.cbcr += static_cast<int64_t>(i) * p.step_cbcr;
  return f;
}

// Where a quad's / block's chroma goes.  LAYOUT is EncodeParams::chroma_layout, uniform over the launch:
//   kChromaNV12: `row` of the CbCr plane, Cb Cr pairs -- one dword per quad;
//   kChromaI420: `row` of the U plane and the same row of the V plane (H/2) x cbcr_stride bytes behind it (v_plane_offset: 64 bits) -- the
//                word quantize_quad<kChromaI420> packed, low half to U, high half to V: a wave writes 128 contiguous bytes to each.
__device__ __forceinline__ uint64_t v_plane_offset(const EncodeParams &p) {
  return static_cast<uint64_t>(p.height >> 1) * p.cbcr_stride;  // uniform: two scalar multiplies
}
// The alpha frame of a pair (the paired kernels, kFormPair; BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA): its planes, its own
// pitches, its V plane behind its U plane by its own chroma pitch
struct AlphaPlanes {
  uint8_t *y, *cbcr;  // cbcr: nullptr in every pair of the launch = the alpha frames have no chroma plane
  uint32_t y_stride, cbcr_stride, height;
  bool with_cbcr;     // uniform over the launch
};
__device__ __forceinline__ uint64_t v_plane_offset(const AlphaPlanes &a) { return static_cast<uint64_t>(a.height >> 1) * a.cbcr_stride; }
// (Planes: EncodeParams, or -- the paired kernels' alpha frame -- AlphaPlanes: whatever v_plane_offset takes)
template <uint32_t LAYOUT, typename Planes>
__device__ __forceinline__ void store_quad_chroma(const Planes &p, uint8_t *row, uint32_t q, uint32_t word) {
  if (LAYOUT == kChromaI420) {
    __builtin_nontemporal_store(static_cast<uint16_t>(word), reinterpret_cast<uint16_t *>(row + 2u * q));
    __builtin_nontemporal_store(static_cast<uint16_t>(word >> 16), reinterpret_cast<uint16_t *>(row + v_plane_offset(p) + 2u * q));
  } else {
    __builtin_nontemporal_store(word, reinterpret_cast<uint32_t *>(row + 4u * q));
  }
}
// general kernels: bytes, any alignment
// Byte 1 of a word quantize_block packed, for the byte store beside byte 0's.  The NV12 kernel's compiler merges the two into one
// 2-byte store at whatever address the row has (legal on gfx950); the planar twin keeps the value opaque so that every store of
// it stays a byte store, as its contract (any alignment, byte stores) reads.
template <uint32_t LAYOUT>
__device__ __forceinline__ uint8_t second_byte(uint32_t word) {
  uint32_t b = word >> 8;
  if (LAYOUT == kChromaI420) asm("" : "+v"(b));
  return static_cast<uint8_t>(b);
}
template <uint32_t LAYOUT, typename Planes>
__device__ __forceinline__ void store_block_chroma(const Planes &p, uint8_t *row, uint32_t bx, uint8_t cb, uint8_t cr) {
  if (LAYOUT == kChromaI420) {
    row[bx] = cb;
    (row + v_plane_offset(p))[bx] = cr;
  } else {
    row[2 * bx] = cb;
    row[2 * bx + 1] = cr;
  }
}

// The BGRA word a kernel of `FORM` encodes for a loaded one: itself, or -- the premultiplying instantiations -- its B, G, R times A
template <uint32_t FORM>
__device__ __forceinline__ uint32_t texel(uint32_t word) {
  if constexpr (form_straight(FORM)) return premultiply_word(word);
  return word;
}
// the four texels of a quad's row premultiplied in place (called from the premultiplying instantiations alone: in the plain ones
// even a call that does nothing moved the fast kernel's code)
__device__ __forceinline__ void premultiply_row(u32x4 &row) {
  row.x = premultiply_word(row.x), row.y = premultiply_word(row.y), row.z = premultiply_word(row.z), row.w = premultiply_word(row.w);
}

// ---- T[A], the alpha frames' luma table (bt709_alpha_luma.h): 256 bytes in LDS, for the alpha kernels and the paired colour kernels
__device__ __forceinline__ void stage_alpha_luma(uint32_t *lut, const EncodeParams &p) {
  if (threadIdx.x < 64) lut[threadIdx.x] = p.alpha_luma[threadIdx.x];  // every workgroup has at least one wave
}

// T[byte 3] of four BGRA words, packed in memory order
__device__ __forceinline__ uint32_t alpha_luma4(const uint32_t *lut, const u32x4 w) {
  const uint8_t *t = reinterpret_cast<const uint8_t *>(lut);
  return static_cast<uint32_t>(t[w.x >> 24]) | (static_cast<uint32_t>(t[w.y >> 24]) << 8) |
         (static_cast<uint32_t>(t[w.z >> 24]) << 16) | (static_cast<uint32_t>(t[w.w >> 24]) << 24);
}

// ---- the paired kernels: the colour frame of pair i, and its alpha frame through `a`
__device__ __forceinline__ EncodeFrame pair_frame(const EncodeParams &p, uint32_t i, AlphaPlanes &a) {
  a.y_stride = static_cast<uint32_t>(p.pairs[0].spare);
  a.cbcr_stride = static_cast<uint32_t>(static_cast<uint64_t>(p.pairs[0].spare) >> 32);
  a.with_cbcr = p.pairs[0].alpha_cbcr != nullptr;
  a.height = p.height;
  const EncodePair &e = p.pairs[p.uniform ? 0u : i];
  EncodeFrame f = {e.bgra, e.y, e.cbcr};
  a.y = e.alpha_y, a.cbcr = e.alpha_cbcr;
  if (p.uniform) {
    f.bgra += static_cast<int64_t>(i) * p.step_bgra;
    f.y += static_cast<int64_t>(i) * p.step_y;
    f.cbcr += static_cast<int64_t>(i) * p.step_cbcr;
    a.y += static_cast<int64_t>(i) * p.pairs[1].spare;
    a.cbcr += static_cast<int64_t>(i) * p.pairs[2].spare;  // of a null plane: never dereferenced (with_cbcr)
  }
  return f;
}
// T sits in the dynamic segment behind the two tables stage_encode_tables puts at address 0 (these kernels may have no static
// LDS): launch_encode sizes the segment for it
__device__ __forceinline__ uint32_t *pair_alpha_lut(unsigned char *lds_raw, const EncodeParams &p) {
  return reinterpret_cast<uint32_t *>(lds_raw + 256u * static_cast<uint32_t>(sizeof(EncodeByteEntry)) + p.from_linear_bytes);
}
constexpr size_t kAlphaLumaLdsBytes = 256;

}  // namespace

// The four kernels, each written once over the chroma layout (EncodeParams::chroma_layout, uniform over the launch): LAYOUT
// reaches quantize_quad, store_quad_chroma, store_block_chroma and second_byte, nothing else.  kChromaI420
// (BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT = BT709HIP_CHROMA_I420) writes three planes, Y then U then V, the YUV4MPEG2 FRAME
// payload (Renderer/y4m_writer.h:194-241).  Preconditions of its fast kernels (checked by the host shim): width % 4 == 0; BGRA
// pointer and pitch 16-byte aligned, Y 4-byte, the U pointer and the chroma pitch 2-byte (the V plane then is, too).  The layout
// is a parameter of the __global__ kernels themselves and not of a body inlined under them: that layer changed the NV12 kernels'
// code (profiles/r14_layout_template_isa.txt).
// FORM, the template argument of the two colour kernels, is the layout plus kFormStraight for their premultiplying instantiations
// (BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY): a straight-alpha picture comes in, and each texel's B, G, R are replaced
// by (c * A + 127) / 255 -- bt709_premultiply.h, integer VALU on the loaded word, the A byte is already in it -- before anything
// else looks at them, so the planes are those of the plain encode of the premultiplied picture.  One argument and not a second:
// the instantiations that existed keep their symbols (the ISA tests and profiles name them) and their code
// (profiles/r15_straight_alpha_isa.txt).
// grid = (tiles, row-pair groups, frames); a workgroup walks row_pairs_per_block consecutive row
// pairs of one frame, prefetching the next pair while it encodes the current one.
template <uint32_t FORM>
__global__ void __launch_bounds__(kMaxBlockThreads)
encode_bgra(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr uint32_t LAYOUT = form_layout(FORM);
  const BandedWork work = banded_work(p.xcd_bands, p.frames_per_band);  // XCD-aware work map: bt709_tile.h
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

  const EncodeLds t = stage_encode_tables(lds_raw, p);  // after the first loads are in flight
  __syncthreads();
  const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);

  for (uint32_t rp = rp0; rp < rp_end; ++rp) {
    // prefetch the next row pair before the arithmetic; nothing on the workgroup's last pair (a
    // clamped re-read of the own rows cost 8 % extra HBM reads at 9 row pairs per workgroup:
    // non-temporal loads do not stay in L2)
    u32x4 ntop = top, nbot = bot;
    if (rp + 1 < rp_end) {
      const uint8_t *s1 = f.bgra + static_cast<size_t>(2 * (rp + 1)) * p.bgra_stride;
      ntop = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + 16u * q));
      nbot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + p.bgra_stride + 16u * q));
    }

    if constexpr (form_straight(FORM)) {  // behind the prefetch, ahead of everything that reads a texel
      premultiply_row(top);
      premultiply_row(bot);
    }
    float va[6], vb[6];
    {
      const uint32_t blk[4] = {top.x, top.y, bot.x, bot.y};
      encode_block(t, quarter_n, blk, va);
    }
    {
      const uint32_t blk[4] = {top.z, top.w, bot.z, bot.w};
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
    top = ntop;
    bot = nbot;
  }
}

// General layout: one lane per 2x2 block, scalar loads/stores, any alignment.
template <uint32_t FORM>
__global__ void __launch_bounds__(kBlockThreads)
encode_bgra_blocks(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr uint32_t LAYOUT = form_layout(FORM);
  const EncodeLds t = stage_encode_tables(lds_raw, p);
  [[maybe_unused]] uint32_t *alpha_lut = nullptr;  // kFormPair alone
  if constexpr (form_pair(FORM)) stage_alpha_luma(alpha_lut = pair_alpha_lut(lds_raw, p), p);
  __syncthreads();
  [[maybe_unused]] AlphaPlanes a;  // kFormPair alone
  const EncodeFrame f = [&] {
    if constexpr (form_pair(FORM)) return pair_frame(p, blockIdx.z, a);
    else return encode_frame(p, blockIdx.z);
  }();
  const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);
  const uint32_t bw = p.width >> 1;
  const uint32_t rp = blockIdx.y;
  for (uint32_t bx = blockIdx.x * blockDim.x + threadIdx.x; bx < bw; bx += gridDim.x * blockDim.x) {
    const uint32_t *r0 = reinterpret_cast<const uint32_t *>(f.bgra + static_cast<size_t>(2 * rp) * p.bgra_stride);
    const uint32_t *r1 = reinterpret_cast<const uint32_t *>(f.bgra + static_cast<size_t>(2 * rp + 1) * p.bgra_stride);
    const uint32_t blk[4] = {texel<FORM>(r0[2 * bx]), texel<FORM>(r0[2 * bx + 1]), texel<FORM>(r1[2 * bx]), texel<FORM>(r1[2 * bx + 1])};
    if constexpr (form_pair(FORM)) {  // the rider: T[A] of the words as loaded, byte stores as encode_alpha_y_blocks
      const uint8_t *ta = reinterpret_cast<const uint8_t *>(alpha_lut);
      uint8_t *a0 = a.y + static_cast<size_t>(2 * rp) * a.y_stride + 2u * bx;
      uint8_t *a1 = a0 + a.y_stride;
      a0[0] = ta[r0[2 * bx] >> 24];
      a0[1] = ta[r0[2 * bx + 1] >> 24];
      a1[0] = ta[r1[2 * bx] >> 24];
      a1[1] = ta[r1[2 * bx + 1] >> 24];
      if (a.with_cbcr) store_block_chroma<LAYOUT>(a, a.cbcr + static_cast<size_t>(rp) * a.cbcr_stride, bx, 128, 128);
    }
    float v[6];
    encode_block(t, quarter_n, blk, v);
    uint32_t ytop, ybot, cbcr;
    quantize_block(v, ytop, ybot, cbcr);
    uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    uint8_t *y1 = y0 + p.y_stride;
    y0[2 * bx] = static_cast<uint8_t>(ytop);
    y0[2 * bx + 1] = second_byte<LAYOUT>(ytop);
    y1[2 * bx] = static_cast<uint8_t>(ybot);
    y1[2 * bx + 1] = second_byte<LAYOUT>(ybot);
    store_block_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, bx, static_cast<uint8_t>(cbcr), static_cast<uint8_t>(cbcr >> 8));
  }
}

// ---------------------------------------------------------------- alpha frames (BT709HIP_FORMAT_BGRA8_ALPHA)
// The reference's alpha clip is the ordinary encode of the grey picture (A,A,A) under (Linear, Linear)
// (srgb_to_bt709/srgb_to_bt709.m:842-954), which is Y = T[A] per pixel and Cb = Cr = 128 (bt709_alpha_luma.h).  Same tile
// shape, work map, prefetch and clamps as encode_bgra; the arithmetic is one byte lookup per pixel.
// TABLE, not arithmetic: the float expression costs a conversion, four multiplies, three adds and a converting pack per pixel
// (9 VALU, 4 of them 4-cycle); the lookup is a shift, a ds_read_u8 and a share of three v_perm/v_lshl_or per word.  The 256
// bytes are 64 dwords = one per LDS bank: lanes that hit the same dword broadcast, different dwords never conflict.
// (stage_alpha_luma and alpha_luma4 stand above the colour kernels: their paired instantiations use them, too)
// grid = (tiles, row-pair groups, frames), as encode_bgra
template <uint32_t LAYOUT>
__global__ void __launch_bounds__(kMaxBlockThreads)
encode_alpha_y(const EncodeParams p) {
  __shared__ uint32_t lut[64];
  const BandedWork work = banded_work(p.xcd_bands, p.frames_per_band);
  const EncodeFrame f = encode_frame(p, work.frame);
  const uint32_t quads = p.width >> 2;
  const uint32_t row_pairs = p.height >> 1;
  const uint32_t q_raw = work.tile * blockDim.x + threadIdx.x;
  const uint32_t q = min(q_raw, quads - 1);
  const uint32_t rp0 = blockIdx.y * p.row_pairs_per_block;
  const uint32_t rp_end = min(rp0 + p.row_pairs_per_block, row_pairs);
  const bool with_cbcr = p.frames[0].cbcr != nullptr;  // uniform over the launch

  const uint8_t *s0 = f.bgra + static_cast<size_t>(2 * rp0) * p.bgra_stride;
  u32x4 top = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + 16u * q));
  u32x4 bot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + p.bgra_stride + 16u * q));

  stage_alpha_luma(lut, p);  // after the first loads are in flight
  __syncthreads();

  for (uint32_t rp = rp0; rp < rp_end; ++rp) {
    u32x4 ntop = top, nbot = bot;
    if (rp + 1 < rp_end) {  // nothing on the workgroup's last pair, as encode_bgra
      const uint8_t *s1 = f.bgra + static_cast<size_t>(2 * (rp + 1)) * p.bgra_stride;
      ntop = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + 16u * q));
      nbot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + p.bgra_stride + 16u * q));
    }
    const uint32_t ytop = alpha_luma4(lut, top), ybot = alpha_luma4(lut, bot);
    if (q_raw < quads) {
      uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
      __builtin_nontemporal_store(ytop, reinterpret_cast<uint32_t *>(y0 + 4u * q));
      __builtin_nontemporal_store(ybot, reinterpret_cast<uint32_t *>(y0 + p.y_stride + 4u * q));
      if (with_cbcr) store_quad_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, q, 0x80808080u);
    }
    top = ntop;
    bot = nbot;
  }
}

// The planar instantiations write 128 to every U and every V byte; they are only launched with chroma planes: an alpha frame
// without them has nothing to lay out and arrives as kChromaNV12.
// General layout: one lane per 2x2 block, byte loads of the four A's and byte stores, any alignment.
template <uint32_t LAYOUT>
__global__ void __launch_bounds__(kBlockThreads)
encode_alpha_y_blocks(const EncodeParams p) {
  __shared__ uint32_t lut[64];
  stage_alpha_luma(lut, p);
  __syncthreads();
  const uint8_t *t = reinterpret_cast<const uint8_t *>(lut);
  const EncodeFrame f = encode_frame(p, blockIdx.z);
  const bool with_cbcr = p.frames[0].cbcr != nullptr;
  const uint32_t bw = p.width >> 1;
  const uint32_t rp = blockIdx.y;
  for (uint32_t bx = blockIdx.x * blockDim.x + threadIdx.x; bx < bw; bx += gridDim.x * blockDim.x) {
    const uint8_t *r0 = f.bgra + static_cast<size_t>(2 * rp) * p.bgra_stride + 8u * bx;
    const uint8_t *r1 = r0 + p.bgra_stride;
    uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride + 2u * bx;
    uint8_t *y1 = y0 + p.y_stride;
    y0[0] = t[r0[3]];
    y0[1] = t[r0[7]];
    y1[0] = t[r1[3]];
    y1[1] = t[r1[7]];
    if (with_cbcr) store_block_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, bx, 128, 128);
  }
}

}  // namespace bt709

#include "bt709_encode_pair.h"     // BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA: encode_bgra_alpha over the helpers above
#include "bt709_encode_convert.h"  // BT709HIP_CTX_OPT_ENCODE_CONVERT: convert_bgra, convert_bgra_blocks over the helpers above
#include "bt709_encode_half.h"     // BT709HIP_CTX_OPT_ENCODE_HALF_INPUT: encode_rgba16f, encode_rgba16f_blocks over the helpers above
#include "bt709_encode_half_alpha.h"  // BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA: encode_rgba16f_alpha, encode_rgba16f_alpha_blocks over both
#include "bt709_encode_chw.h"      // BT709HIP_CTX_OPT_ENCODE_CHW_INPUT: encode_chw, encode_chw_blocks over the helpers above

namespace bt709 {
namespace {

// One row per selectable kernel: the selector, the kernel for either chroma layout, the two names bt709hip_last_kernel_name
// reports, and whether the kernel stages its tables in dynamic LDS (the alpha kernels' 256 bytes and the converter's 1 KiB are
// static) -- prepare_encode_kernels raises the cap of exactly those.  A selector field is a value or kAny; the first matching row
// is the launch's kernel.
struct EncodeKernel {
  int fast, alpha, premultiply, convert;  // alpha: 0 colour, 1 alpha frame, 2 the pair; convert: EncodeParams::convert_mode
  bool stages_table;
  void (*fn[2])(const EncodeParams);  // [chroma layout]
  const char *name[2];
};
// KERNEL<layout | FORM>; both names from one stem and one suffix: colour kernels spell the layout (encode_bgra_i420<premul>), the
// alpha kernels' NV12 form names none (encode_alpha_y, encode_alpha_y<i420>)
#define ENCODE_COLOUR(fast, premultiply, suffix, KERNEL, FORM) \
  {fast, 0, premultiply, kConvertOff, true, {KERNEL<kChromaNV12 | (FORM)>, KERNEL<kChromaI420 | (FORM)>}, {"encode_bgra_nv12" suffix, "encode_bgra_i420" suffix}}
// the paired kernels (EncodeParams: alpha_luma and per_byte both non-null): encode_bgra_alpha (bt709_encode_pair.h) and the general
// colour kernel's kFormPair instantiations
#define ENCODE_PAIR(fast, premultiply, suffix, KERNEL, FORM) \
  {fast, 2, premultiply, kConvertOff, true, {KERNEL<kChromaNV12 | kFormPair | (FORM)>, KERNEL<kChromaI420 | kFormPair | (FORM)>}, {"encode_bgra_alpha_nv12" suffix, "encode_bgra_alpha_i420" suffix}}
#define ENCODE_ALPHA(fast, stem, KERNEL) {fast, 1, kAny, kConvertOff, false, {KERNEL<kChromaNV12>, KERNEL<kChromaI420>}, {stem, stem "<i420>"}}
// the converter (the shim hands it BGRA8_SRGB input alone): the packed form writes no plane, one instantiation under both layouts
#define CONVERT_PACKED(fast, premultiply, suffix, KERNEL, FORM) \
  {fast, 0, premultiply, kConvertPacked444, false, {KERNEL<kFormPacked | (FORM)>, KERNEL<kFormPacked | (FORM)>}, {"convert_bgra_packed444" suffix, "convert_bgra_packed444" suffix}}
#define CONVERT_POINT(fast, premultiply, suffix, KERNEL, FORM) \
  {fast, 0, premultiply, kConvertPoint420, false, {KERNEL<kChromaNV12 | (FORM)>, KERNEL<kChromaI420 | (FORM)>}, {"convert_bgra_nv12" suffix, "convert_bgra_i420" suffix}}
const EncodeKernel kEncodeKernels[] = {
    CONVERT_PACKED(1, 1, "<premul>", convert_bgra, kFormStraight),
    CONVERT_PACKED(1, 0, "", convert_bgra, 0),
    CONVERT_PACKED(0, 1, "_blocks<premul>", convert_bgra_blocks, kFormStraight),
    CONVERT_PACKED(0, 0, "_blocks", convert_bgra_blocks, 0),
    CONVERT_POINT(1, 1, "<premul>", convert_bgra, kFormStraight),
    CONVERT_POINT(1, 0, "", convert_bgra, 0),
    CONVERT_POINT(0, 1, "_blocks<premul>", convert_bgra_blocks, kFormStraight),
    CONVERT_POINT(0, 0, "_blocks", convert_bgra_blocks, 0),
    ENCODE_PAIR(1, 1, "<premul>", encode_bgra_alpha, kFormStraight),
    ENCODE_PAIR(1, 0, "", encode_bgra_alpha, 0),
    ENCODE_PAIR(0, 1, "_blocks<premul>", encode_bgra_blocks, kFormStraight),
    ENCODE_PAIR(0, 0, "_blocks", encode_bgra_blocks, 0),
    ENCODE_ALPHA(1, "encode_alpha_y", encode_alpha_y),
    ENCODE_COLOUR(1, 1, "<premul>", encode_bgra, kFormStraight),
    ENCODE_COLOUR(1, 0, "", encode_bgra, 0),
    ENCODE_ALPHA(0, "encode_alpha_y_blocks", encode_alpha_y_blocks),
    ENCODE_COLOUR(0, 1, "_blocks<premul>", encode_bgra_blocks, kFormStraight),
    ENCODE_COLOUR(0, 0, "_blocks", encode_bgra_blocks, 0),
};
#undef ENCODE_COLOUR
#undef ENCODE_ALPHA
#undef ENCODE_PAIR
#undef CONVERT_PACKED
#undef CONVERT_POINT

// RGBA16Float input (EncodeParams::input_format): a table of its own, [fast][pair]; the shim refuses every option the rows above
// select by.  pair: the alpha frame rides along (BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA, bt709_encode_half_alpha.h)
const EncodeKernel kEncodeHalfKernels[2][2] = {
    {{0, 0, 0, kConvertOff, true, {encode_rgba16f_blocks<kChromaNV12>, encode_rgba16f_blocks<kChromaI420>}, {"encode_rgba16f_nv12_blocks", "encode_rgba16f_i420_blocks"}},
     {0, 2, 0, kConvertOff, true, {encode_rgba16f_alpha_blocks<kChromaNV12>, encode_rgba16f_alpha_blocks<kChromaI420>}, {"encode_rgba16f_alpha_nv12_blocks", "encode_rgba16f_alpha_i420_blocks"}}},
    {{1, 0, 0, kConvertOff, true, {encode_rgba16f<kChromaNV12>, encode_rgba16f<kChromaI420>}, {"encode_rgba16f_nv12", "encode_rgba16f_i420"}},
     {1, 2, 0, kConvertOff, true, {encode_rgba16f_alpha<kChromaNV12>, encode_rgba16f_alpha<kChromaI420>}, {"encode_rgba16f_alpha_nv12", "encode_rgba16f_alpha_i420"}}},
};

// Planar-tensor input (EncodeParams::input_format kEncodeInputCHW*): [fast][element]; the shim refuses every option the first table
// selects by, and the pair
#define ENCODE_CHW(fast, suffix, KERNEL, ELEM, elem) \
  {fast, 0, 0, kConvertOff, true, {KERNEL<kChromaNV12, ELEM>, KERNEL<kChromaI420, ELEM>}, {"encode_chw_nv12" suffix "<" elem ">", "encode_chw_i420" suffix "<" elem ">"}}
const EncodeKernel kEncodeChwKernels[2][3] = {
    {ENCODE_CHW(0, "_blocks", encode_chw_blocks, kChwU8, "u8"), ENCODE_CHW(0, "_blocks", encode_chw_blocks, kChwF16, "f16"), ENCODE_CHW(0, "_blocks", encode_chw_blocks, kChwF32, "f32")},
    {ENCODE_CHW(1, "", encode_chw, kChwU8, "u8"), ENCODE_CHW(1, "", encode_chw, kChwF16, "f16"), ENCODE_CHW(1, "", encode_chw, kChwF32, "f32")},
};
#undef ENCODE_CHW

// The kernel of a launch that launch_encode has planned and recorded
const char *launch_encode_kernel(const EncodeParams &p, const dim3 &grid, const dim3 &block, size_t lds, bool fast, int alpha, hipStream_t stream) {
  const uint32_t layout = p.chroma_layout == kChromaI420 ? kChromaI420 : kChromaNV12;
  if (p.input_format == kEncodeInputRGBA16F) {
    const EncodeKernel &k = kEncodeHalfKernels[fast ? 1 : 0][alpha == 2 ? 1 : 0];
    hipLaunchKernelGGL(k.fn[layout], grid, block, lds, stream, p);
    return k.name[layout];
  }
  if (encode_input_chw(p.input_format)) {
    const EncodeKernel &k = kEncodeChwKernels[fast ? 1 : 0][encode_chw_elem(p.input_format) - kChwU8];
    hipLaunchKernelGGL(k.fn[layout], grid, block, lds, stream, p);
    return k.name[layout];
  }
  for (const EncodeKernel &k : kEncodeKernels) {
    if (k.fast != fast || k.alpha != alpha || !selects(k.premultiply, p.premultiply != 0) || k.convert != static_cast<int>(p.convert_mode)) continue;
    hipLaunchKernelGGL(k.fn[layout], grid, block, lds, stream, p);
    return k.name[layout];
  }
  return nullptr;  // unreachable: the rows cover fast x {colour, alpha, pair} x premultiply, and fast x premultiply for either converter mode
}

}  // namespace

const char *launch_encode(const EncodeParams &params, int frames, bool fast, bool xcd_bands, hipStream_t stream) {
  const BandPlan plan = plan_bands(frames, fast && xcd_bands, params.uniform, kXcdBandMinFrames);
  if (plan.banded && plan.tail) {
    launch_encode(params, plan.banded, fast, xcd_bands, stream);
    EncodeParams tail = params;
    advance_frames(tail, plan.banded);
    return launch_encode(tail, plan.tail, fast, false, stream);
  }
  EncodeParams p = params;
  // RGBA16Float input: a lane of the fast kernel owns a 2x2 block, not a quad -- the plan of a BGRA8 picture twice as wide
  const bool half = p.input_format == kEncodeInputRGBA16F;
  const uint32_t plan_width = half ? 2 * p.width : p.width;
  if (p.row_pairs_per_block == 0) p.row_pairs_per_block = encode_row_pairs_per_block(plan_width, p.height, frames);
  // BT709HIP_FORMAT_BGRA8_ALPHA: same plan, the alpha kernels (static LDS); with the colour's tables as well: the pair, T behind them
  const int alpha = p.convert_mode != kConvertOff ? 0 : encode_pair(p) ? 2 : p.alpha_luma != nullptr ? 1 : 0;
  const size_t lds = half ? p.from_linear_bytes + (alpha == 2 ? kAlphaLumaLdsBytes : 0) : alpha == 1 || p.convert_mode != kConvertOff ? 0 : 256 * sizeof(EncodeByteEntry) + p.from_linear_bytes + (alpha == 2 ? kAlphaLumaLdsBytes : 0);  // the converter's curve is static, too
  dim3 grid((p.width / 2 + kBlockThreads - 1) / kBlockThreads, p.height / 2, frames), block(kBlockThreads);
  if (fast) {
    const uint32_t quads = plan_width / 4;
    uint32_t threads = p.block_threads ? p.block_threads : encode_block_threads(plan_width);
    // One picture per launch (what a caller of +convertIntoCoreVideoBuffer: issues) is one under-filled generation of
    // workgroups: tiles of up to 512 lanes (3840 -> 2 x 512 instead of 3 x 320) ran 7-8 % faster there
    // (tools/encode_single_shapes.sh, round 3: 665 -> 718-722 Gpixel/s); batched launches keep the 320-lane tiles.
    if (p.block_threads == 0 && frames == 1) {
      const uint32_t tiles = (quads + 511) / 512;
      threads = ((quads + tiles - 1) / tiles + 63) / 64 * 64;
      if (threads < 64) threads = 64;
    }
    if (threads > static_cast<uint32_t>(kMaxBlockThreads)) threads = kMaxBlockThreads;
    grid = dim3((quads + threads - 1) / threads, (p.height / 2 + p.row_pairs_per_block - 1) / p.row_pairs_per_block, frames);
    block = dim3(threads);
    if (plan.banded) grid = band_grid(p, 1, grid);
  }
  record_launch(grid, block, fast ? p.xcd_bands : 0);
  // the plan does not depend on the layout, only the kernel does (an alpha frame without chroma planes arrives as kChromaNV12)
  return launch_encode_kernel(p, grid, block, lds, fast, alpha, stream);
}

hipError_t prepare_encode_kernels() {
  for (const EncodeKernel &k : kEncodeKernels) {
    const void *fns[] = {reinterpret_cast<const void *>(k.fn[0]), reinterpret_cast<const void *>(k.fn[1])};
    if (const hipError_t e = k.stages_table ? raise_lds_cap(fns, kRepLdsBytes) : hipSuccess) return e;
  }
  for (const auto &row : kEncodeHalfKernels)
    for (const EncodeKernel &k : row) {
      const void *fns[] = {reinterpret_cast<const void *>(k.fn[0]), reinterpret_cast<const void *>(k.fn[1])};
      if (const hipError_t e = raise_lds_cap(fns, kRepLdsBytes)) return e;
    }
  for (const auto &row : kEncodeChwKernels)
    for (const EncodeKernel &k : row) {
      const void *fns[] = {reinterpret_cast<const void *>(k.fn[0]), reinterpret_cast<const void *>(k.fn[1])};
      if (const hipError_t e = raise_lds_cap(fns, kRepLdsBytes)) return e;
    }
  return hipSuccess;
}

}  // namespace bt709
