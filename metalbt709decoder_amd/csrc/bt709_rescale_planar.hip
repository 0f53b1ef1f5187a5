// CDNA4 (gfx950) kernels of the FUSED decode + rescale to any output size FROM PLANAR I420 FRAMES (BT709HIP_OPT_SCALED_PLANAR with
// BT709HIP_OPT_CHROMA_LAYOUT = BT709HIP_CHROMA_I420): a Y4M / yuv420p frame -- Y, then U, then V -- to a BGRA8 view or
// a planar CHW tensor of another size in one launch, where "interleave the chroma into an NV12 staging plane, then rescale" takes a
// pass over a scratch plane per frame.
//
//   decode_i420_scaled   decode_nv12_scaled (bt709_rescale_scaled.hip) and decode_nv12_scaled_chw (bt709_rescale_chw.hip) with
//                        another FRONT END: the chroma of pixel (x, y) is U[y/2][x/2], V[y/2][x/2] of two planes of pitch cbcr_stride,
//                        V v_offset bytes behind U.  From the tap word {Cb0, Cr0, Cb1, Cr1} on it is the same text
//                        (bt709_scaled_strip.h scaled_strip: chroma-row cache, pixel_rgb, tables, filter, encode, both store
//                        epilogues), so the bytes are those of the NV12 kernels on the interleaved twin of the planes.
// Tap forms (scaled_strip, LAYOUT): TAPS_ONCE, TAPS_WIDE and TAPS_BYTES, each with the persistence of its NV12 twin.  There is no
// planar TAPS_PAIRS (a plane's sample is one byte: where NV12 takes PAIRS these frames take BYTES, the same count of loads) and no
// planar TAPS_SHARED (scale_y < 1 with scale_x > 0.95: the launcher takes the per-lane form there).
//
// Kernels of their own: scaled_strip's layout selector defaults to NV12 and nothing here is inlined under a kernel of the NV12 files,
// whose code stays what it was (profiles/r24_scaled_planar_isa.txt).
#include "bt709_scaled_strip.h"

namespace bt709 {

// BT709_SCALED_ITEM_LOOP hands its OVER argument on as scaled_strip's template arguments behind HAS_ALPHA: never blended, the
// element (kChwNone: the BGRA8 word), the layout
#define BT709_SCALED_PLANAR_FORM kOverOff, ELEM, kChromaI420

template <int TAPS, uint32_t ELEM, bool HAS_ALPHA, bool PERSISTENT>
__global__ void __launch_bounds__(kBlockThreads)
decode_i420_scaled(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const RescaleLookup r = stage_rescale_tables<false>(lds_raw, p, 0, 0, 0);
  __syncthreads();
  if (PERSISTENT) {
    BT709_SCALED_ITEM_LOOP(HAS_ALPHA, BT709_SCALED_PLANAR_FORM, Srgb8Light{r}, OverLookup{})
    return;
  }
  const FramePlanes f = frame_planes(p, blockIdx.z);
  const uint32_t ox = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t oy0 = blockIdx.y * p.scaled_rows;  // < out_height: the grid has exactly the strips
  const StripTaps vt = strip_taps(oy0, p.scale_y);  // before any lane leaves
  if (TAPS != TAPS_ONCE && ox >= p.out_width) return;  // TAPS_ONCE: the wave works together
  scaled_strip<TAPS, HAS_ALPHA, BT709_SCALED_PLANAR_FORM>(p, Srgb8Light{r}, f, ox, oy0, min(oy0 + p.scaled_rows, p.out_height), vt);
}
#undef BT709_SCALED_PLANAR_FORM

namespace {

// The rows of this file's kernels (bt709_rescale.h ScaledKernel: {taps, alpha, curve, over, persistent, kernel, name}), one table per
// element type, stamped out per tap form with the persistence of bt709_rescale_scaled.hip's rows.
#define SCALED_PLANAR_KERNELS(T, P, ELEM, name)                                                   \
  {T, 1, kAny, kAny, P, decode_i420_scaled<T, ELEM, true, P>, name(",alpha", "<alpha>")},          \
  {T, 0, kAny, kAny, P, decode_i420_scaled<T, ELEM, false, P>, name("", "")}
#define SCALED_PLANAR_TABLE(ELEM, name)                                                            \
  {SCALED_PLANAR_KERNELS(TAPS_ONCE, false, ELEM, name), SCALED_PLANAR_KERNELS(TAPS_WIDE, true, ELEM, name), SCALED_PLANAR_KERNELS(TAPS_BYTES, true, ELEM, name)}
// name(alpha suffix inside a CHW kernel's brackets, alpha suffix of the BGRA8 kernel)
#define NAME_BGRA8(in_brackets, bare) "decode_i420_scaled" bare
#define NAME_U8(in_brackets, bare) "decode_i420_scaled_chw<u8" in_brackets ">"
#define NAME_F16(in_brackets, bare) "decode_i420_scaled_chw<f16" in_brackets ">"
#define NAME_F32(in_brackets, bare) "decode_i420_scaled_chw<f32" in_brackets ">"
const ScaledKernel kScaledPlanar[] = SCALED_PLANAR_TABLE(kChwNone, NAME_BGRA8);
const ScaledKernel kScaledPlanarU8[] = SCALED_PLANAR_TABLE(kChwU8, NAME_U8);
const ScaledKernel kScaledPlanarF16[] = SCALED_PLANAR_TABLE(kChwF16, NAME_F16);
const ScaledKernel kScaledPlanarF32[] = SCALED_PLANAR_TABLE(kChwF32, NAME_F32);
#undef NAME_F32
#undef NAME_F16
#undef NAME_U8
#undef NAME_BGRA8
#undef SCALED_PLANAR_TABLE
#undef SCALED_PLANAR_KERNELS

}  // namespace

ScaledKernels scaled_planar_kernels(uint32_t elem) {
  switch (elem) {
    case kChwU8: return ScaledKernels(kScaledPlanarU8);
    case kChwF16: return ScaledKernels(kScaledPlanarF16);
    case kChwF32: return ScaledKernels(kScaledPlanarF32);
    default: return ScaledKernels(kScaledPlanar);
  }
}

}  // namespace bt709
