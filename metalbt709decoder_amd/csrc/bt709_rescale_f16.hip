// CDNA4 (gfx950) kernel of the FUSED decode + rescale to any output size THROUGH THE RGBA16Float INTERMEDIATE: what
// bt709hip_decode into an RGBA16F surface followed by bt709hip_render_scaled from it produces, in one launch and without the
// surface (BT709HIP_OPT_SCALE_INTERMEDIATE = BT709HIP_FORMAT_RGBA16F).  Where sRGB texture writes are unavailable the reference
// renders pass 1 into RGBA16Float holding linear light and runs -renderScaled: over that (Renderer/AAPLRenderer.m:132-207).
//
//   decode_nv12_scaled_f16   geometry, tap fetch, row cache, strip walk and store of decode_nv12_scaled (bt709_scaled_strip.h: the
//                            same taps, weights and summation order), with another conversion of a decoded tap and another encode:
//     colour tap   float(H(x)), H = the RGBA16F target's per-channel half (bt709_half_lookup.h; a mode without a curve: the
//                  round-to-nearest-even conversion alone)
//     alpha tap    float(half(alpha_value(a)))
//     sums         saturated (a unorm render target clamps); R, G, B through the sRGB-encode table in unit range, as
//                  render_scaled<true> stages it (quarter_unscale = 1, edges as they are); alpha through alpha_word_of
//     no alpha     A = 0xFF whatever the decoder's alpha fill says: the half target holds 1.0 (see HalfLight::opaque_word)
// LDS: the half lookup's plan as decode_nv12_rgba16f has it -- thresholds from byte 0, candidate entries from kHalfCandLds, under
// 40 KiB together -- and the 5 KiB of encode buckets behind it at kHalfPlanLds: 45 KiB, three 256-lane workgroups per CU.  Staging
// that per item of 256 x 32 output pixels would be 5.6 B per output pixel from L2, more than the kernel's HBM traffic, so EVERY
// tap form runs the persistent item loop here (decode_nv12_scaled keeps its by-wave forms out of it for 5 VGPRs = one wave per
// SIMD; at three workgroups = 12 waves per CU the LDS is the limit, not the registers).  A mode without a curve stages the encode
// buckets alone, at byte 0.
#include "bt709_half_lookup.h"
#include "bt709_scaled_strip.h"

namespace bt709 {
namespace {

// The RGBA16Float intermediate (see the head of the file).  CURVE: the decoder's gamma has a half table.
template <bool CURVE>
struct HalfLight {
  const HalfLookup &t;
  const RescaleLookup &r;
  // one source pixel (TAPS_ONCE): the pairs (R, G) and (B, A)
  template <int N>
  __device__ __forceinline__ void one(const float *x, uint32_t a, float *own) const {
    float v[4] = {x[0], x[1], x[2], 0.0f};
    if (N == 4) v[3] = alpha_value(byte_of(a, 0));
    half_lights<CURVE ? 3 : 0, N - (CURVE ? 3 : 0)>(t, v, own);
  }
  // the two horizontal taps of a source row: (R0, G0), (B0, R1), (G1, B1) and, with an alpha plane, (A0, A1)
  template <int N>
  __device__ __forceinline__ void two(const float *x, uint32_t a, RowLin<N> &rl) const {
    float v[8] = {x[0], x[1], x[2], x[3], x[4], x[5], 0.0f, 0.0f}, lin[8];
    if (N == 4) v[6] = alpha_value(byte_of(a, 0)), v[7] = alpha_value(byte_of(a, 1));
    half_lights<CURVE ? 6 : 0, 2 * N - (CURVE ? 6 : 0)>(t, v, lin);
#pragma unroll
    for (int tap = 0; tap < 2; ++tap) {
#pragma unroll
      for (int k = 0; k < 3; ++k) rl.v[tap][k] = lin[3 * tap + k];
      if (N == 4) rl.v[tap][3] = lin[6 + tap];
    }
  }
  __device__ __forceinline__ uint32_t encode(float sum) const { return encode_byte(r, add_sat(sum, 0.0f)); }
  __device__ __forceinline__ uint32_t encode_unit(float v) const { return encode_byte(r, v); }  // the blend's v: the table's own domain
  // Without an alpha plane pass 1 stores A = 1.0 and pass 2 filters four taps of it: alpha_word_of(((w00 + w01) + w10) + w11)
  // with w00 = gx gy, w01 = fx gy, w10 = gx fy, w11 = fx fy, gx = RN(1 - fx), gy = RN(1 - fy), fx, fy in [0, 1).  That is 255 for
  // EVERY weight set, so the constant is stored: gx + fx and gy + fy are within 2^-25 of 1 (1 - f is exact for f >= 1/2 and
  // rounds a value in (1/2, 1] otherwise), each of the four products (<= 1) and each of the three sums (<= 1 + 2^-20) adds at
  // most 2^-24, so the sum s has |s - 1| < 2^-21, and round(255 saturate(s)) = 255 for every s > 254.5 / 255 = 1 - 2^-8.99.
  __device__ __forceinline__ uint32_t opaque_word(const DecodeParams &) const { return 0xff000000u; }
};

}  // namespace

// The kernel's body as TEXT: decode_nv12_scaled_f16_over below is the same kernel with lin[256] of the blend behind the encode
// buckets and the strips in their over form, and the body has to sit in the kernel function itself (bt709_rescale_scaled.hip,
// BT709_SCALED_WALK: the plain kernels' instruction streams are pinned).
#define BT709_SCALED_F16_BODY(HAS_ALPHA, CURVE, OVER)                                                                                    \
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];                                                                \
  constexpr uint32_t kEncodeLds = CURVE ? kHalfPlanLds : 0u;                                                                             \
  OverLookup ov = {};                                                                                                                    \
  {                                                                                                                                      \
    if (CURVE) stage_half_tables(lds_raw, p.half_table, p.half_cand_offset, p.half_table_bytes);                                         \
    const u32x4 *e = reinterpret_cast<const u32x4 *>(p.table_encode);                                                                    \
    stage_batched(reinterpret_cast<u32x4 *>(lds_raw + kEncodeLds), p.table_encode_bytes / 16, threadIdx.x, blockDim.x, [&](uint32_t i) { return e[i]; }); \
    /* the half lookup addresses LDS absolutely: this kernel has no static LDS, so its dynamic segment starts at byte 0 */               \
    if (CURVE && lds_address(lds_raw) != 0u) __builtin_trap();                                                                           \
    if constexpr (OVER != kOverOff) ov = stage_over_lin(lds_raw, p, kEncodeLds + p.table_encode_bytes);                                  \
  }                                                                                                                                      \
  __syncthreads();                                                                                                                       \
  RescaleLookup r = unit_encode_lookup(lds_address(lds_raw) + kEncodeLds, p.encode_log_add, p.encode_log_first);                         \
  asm volatile("" : "+v"(r.enc_log_off)); /* ONE addend of the v_lshl_add */                                                             \
  HalfLookup t;                                                                                                                          \
  t.index_scale = p.half_index_scale;                                                                                                    \
  t.below2 = (p.half_h_min - 1u) * 0x10001u;                                                                                             \
  const HalfLight<CURVE> light = {t, r};                                                                                                 \
  BT709_SCALED_ITEM_LOOP(HAS_ALPHA, OVER, light, ov)

template <int TAPS, bool HAS_ALPHA, bool CURVE>
__global__ void __launch_bounds__(kBlockThreads)
decode_nv12_scaled_f16(const DecodeParams p) {
  BT709_SCALED_F16_BODY(HAS_ALPHA, CURVE, kOverOff)
}

// BT709HIP_OPT_SCALED_OVER through the RGBA16Float intermediate: an alpha decoder runs the sRGB mode, which has a
// curve.  46 KiB of LDS: still three workgroups per CU.  Kernels of their own: the plain instantiations keep their code.
template <int TAPS, int OVER>
__global__ void __launch_bounds__(kBlockThreads)
decode_nv12_scaled_f16_over(const DecodeParams p) {
  BT709_SCALED_F16_BODY(true, true, OVER)
}
#undef BT709_SCALED_F16_BODY

// The rows of this file's kernels (bt709_rescale.h ScaledKernel: {taps, alpha, curve, over, persistent, kernel, name}), stamped out
// per tap form; launch_decode_scaled looks them up.  Every form runs the item loop (see the head of the file).  An alpha decoder
// runs the sRGB mode, which has a curve: its rows take any `curve`.  The name does not say whether a colour decoder's gamma has one.
#define SCALED_F16_KERNELS(T)                                                                                                            \
  {T, 1, kAny, kOverDestination, true, decode_nv12_scaled_f16_over<T, kOverDestination>, "decode_nv12_scaled_f16<alpha,over>"},          \
  {T, 1, kAny, kOverColour, true, decode_nv12_scaled_f16_over<T, kOverColour>, "decode_nv12_scaled_f16<alpha,over-colour>"},             \
  {T, 1, kAny, kOverOff, true, decode_nv12_scaled_f16<T, true, true>, "decode_nv12_scaled_f16<alpha>"},                                  \
  {T, 0, 1, kAny, true, decode_nv12_scaled_f16<T, false, true>, "decode_nv12_scaled_f16"},                                               \
  {T, 0, 0, kAny, true, decode_nv12_scaled_f16<T, false, false>, "decode_nv12_scaled_f16"}
static const ScaledKernel kScaledF16Kernels[] = {
    SCALED_F16_KERNELS(TAPS_ONCE), SCALED_F16_KERNELS(TAPS_SHARED), SCALED_F16_KERNELS(TAPS_WIDE), SCALED_F16_KERNELS(TAPS_PAIRS), SCALED_F16_KERNELS(TAPS_BYTES),
};
#undef SCALED_F16_KERNELS

ScaledKernels scaled_f16_kernels() { return kScaledF16Kernels; }

}  // namespace bt709
