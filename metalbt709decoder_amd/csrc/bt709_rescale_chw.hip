// CDNA4 (gfx950) kernels of the FUSED decode + rescale to any output size INTO PLANAR C x OH x OW TENSORS (BT709HIP_OPT_SCALED_CHW;
// BT709HIP_FORMAT_CHW_U8 / _F16 / _F32 targets of bt709hip_decode_scaled[_batch] and bt709hip_decode_half[_batch]):
// a frame to a normalised view of the model's size in one launch, where "rescale to BGRA8, then permute, convert and normalise"
// takes a second pass over a scratch surface.
//
//   decode_nv12_scaled_chw   decode_nv12_scaled (bt709_rescale_scaled.hip) up to the bytes R, G, B, A of an output pixel -- the same
//                            geometry, tap forms, row cache, strip walk, tables and summation order (bt709_scaled_strip.h
//                            scaled_strip, one text) -- and then, in place of the one 4-byte word, one element per plane:
//     CHW_U8           the byte
//     CHW_F16 / _F32   bt709_chw_norm.h of the byte: (byte * (1/255f)) * scale_c + bias_c, three roundings, binary16 behind them;
//                      the A plane (alpha decoders) byte * (1/255f) alone
// A lane owns an output column, so a wave's store instruction fills 64 / 128 / 256 contiguous bytes of a plane's row: no interleave,
// no transpose.  An opaque decoder writes three planes and its alpha fill nowhere.
//
// Kernels of their own: scaled_strip's element selector defaults to "BGRA word", and nothing here is inlined under a kernel of
// bt709_rescale_scaled.hip or bt709_rescale_f16.hip, whose code stays what it was (profiles/r23_scaled_chw_isa.txt).  Each tap form
// has the persistence of its BGRA8 twin: the by-wave forms run one workgroup per item, the per-lane forms the persistent item loop.
#include "bt709_scaled_strip.h"

namespace bt709 {

// BT709_SCALED_ITEM_LOOP hands its OVER argument on as scaled_strip's template arguments behind HAS_ALPHA: never blended, then the element
#define BT709_SCALED_CHW_FORM kOverOff, ELEM

template <int TAPS, uint32_t ELEM, bool HAS_ALPHA, bool PERSISTENT>
__global__ void __launch_bounds__(kBlockThreads)
decode_nv12_scaled_chw(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const RescaleLookup r = stage_rescale_tables<false>(lds_raw, p, 0, 0, 0);
  __syncthreads();
  if (PERSISTENT) {
    BT709_SCALED_ITEM_LOOP(HAS_ALPHA, BT709_SCALED_CHW_FORM, Srgb8Light{r}, OverLookup{})
    return;
  }
  const FramePlanes f = frame_planes(p, blockIdx.z);
  const uint32_t ox = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t oy0 = blockIdx.y * p.scaled_rows;  // < out_height: the grid has exactly the strips
  const StripTaps vt = strip_taps(oy0, p.scale_y);  // before any lane leaves
  if (TAPS != TAPS_SHARED && TAPS != TAPS_ONCE && ox >= p.out_width) return;  // TAPS_SHARED / TAPS_ONCE: the wave works together
  scaled_strip<TAPS, HAS_ALPHA, BT709_SCALED_CHW_FORM>(p, Srgb8Light{r}, f, ox, oy0, min(oy0 + p.scaled_rows, p.out_height), vt);
}
#undef BT709_SCALED_CHW_FORM

namespace {

// The rows of this file's kernels (bt709_rescale.h ScaledKernel: {taps, alpha, curve, over, persistent, kernel, name}), one table per
// element type, stamped out per tap form with the persistence of bt709_rescale_scaled.hip's rows.
#define SCALED_CHW_KERNELS(T, P, ELEM, ename)                                                                        \
  {T, 1, kAny, kAny, P, decode_nv12_scaled_chw<T, ELEM, true, P>, "decode_nv12_scaled_chw<" ename ",alpha>"},        \
  {T, 0, kAny, kAny, P, decode_nv12_scaled_chw<T, ELEM, false, P>, "decode_nv12_scaled_chw<" ename ">"}
#define SCALED_CHW_TABLE(ELEM, ename)                                                                                \
  {SCALED_CHW_KERNELS(TAPS_ONCE, false, ELEM, ename), SCALED_CHW_KERNELS(TAPS_SHARED, false, ELEM, ename),           \
   SCALED_CHW_KERNELS(TAPS_WIDE, true, ELEM, ename), SCALED_CHW_KERNELS(TAPS_PAIRS, true, ELEM, ename),              \
   SCALED_CHW_KERNELS(TAPS_BYTES, true, ELEM, ename)}
const ScaledKernel kScaledChwU8[] = SCALED_CHW_TABLE(kChwU8, "u8");
const ScaledKernel kScaledChwF16[] = SCALED_CHW_TABLE(kChwF16, "f16");
const ScaledKernel kScaledChwF32[] = SCALED_CHW_TABLE(kChwF32, "f32");
#undef SCALED_CHW_TABLE
#undef SCALED_CHW_KERNELS

}  // namespace

ScaledKernels scaled_chw_kernels(uint32_t elem) {
  return elem == kChwU8 ? ScaledKernels(kScaledChwU8) : (elem == kChwF16 ? ScaledKernels(kScaledChwF16) : ScaledKernels(kScaledChwF32));
}

}  // namespace bt709
