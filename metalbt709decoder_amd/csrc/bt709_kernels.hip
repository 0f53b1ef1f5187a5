// CDNA4 (gfx950) kernels of the BT.709 NV12 / planar I420 -> sRGB BGRA decode path.
//
// What the reference does in its first Metal pass -- BT709ToLinearSRGBKernel & friends
// (Renderer/AAPLShaders.metal:336-407: read Y(gid) and CbCr(gid/2), 3x3 matrix, video-gamma
// removal, write into an sRGB8 texture whose store hardware applies the sRGB OETF) -- with the
// arithmetic of the reference's CPU path (bt709_device.h).  The transfer step is a table:
//       byte = bucket[q].base + (x >= bucket[q].edge),  q = floor(x N)
// (transfer_tables.h), x the saturated R, G or B.
//
// Memory plan (HBM-bound: 1.5 B read + 4 B written per pixel, no reuse between workgroups -- nothing to keep in an L2 --
// but the ORDER in which the eight XCDs walk a long launch decides how the DRAM streams interleave: batched launches of 64
// frames or more give each XCD a contiguous band of the frames, bt709_tile.h banded_work):
//   * a lane owns 4-wide x 2-high pixel "quads": one dword of each luma row, one dword of CbCr
//     (two Cb,Cr pairs, each shared by a 2x2 block -- chroma is REPLICATED, not interpolated:
//     AAPLShaders.metal:350, BGRAToBT709Converter.m:267-277) and two 16-byte non-temporal
//     stores per quad;
//   * consecutive lanes own consecutive quads of the same row pair, so a wave reads 3 x 256
//     contiguous bytes and writes 2 x 1 KiB contiguous, fully coalesced;
//   * grid = (tiles per row pair, row pairs, frames): one short-lived workgroup per tile,
//     dispatched in address order (x fastest).  Measured: long-lived grid-strided workgroups
//     lose ~20 % of the bandwidth, fewer than 4 resident workgroups per CU lose 1-40 %, and
//     every VALU instruction shows up in run time (bt709_device.h, VALU BUDGET), so the kernels
//     have no loops and no integer divisions;
//   * the tile's global loads are issued before the 4 KiB table is staged into LDS.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "bt709_decode_body.h"
#include "bt709_launch.h"

namespace bt709 {

// Every 1:1 kernel is written once over the chroma layout (LAYOUT = DecodeParams::chroma_layout, uniform over the launch;
// BT709HIP_OPT_CHROMA_LAYOUT).  kChromaI420 is planar 4:2:0 -- the YUV4MPEG2 C420jpeg payload, Y then U then V
// (Renderer/y4m_writer.h:194-241; a software decoder's yuv420p): pixel (x, y) takes Y[y][x], U[y/2][x/2], V[y/2][x/2], and the
// output is byte for byte what the NV12 instantiation writes for the interleaved twin of the planes.  Same traffic as NV12,
// 1.5 B read + 4 B written per pixel, where "interleave the planes, then decode" moves 6.5 B in two launches.  The arithmetic
// is one text (bt709_decode_body.h); the layout only decides which chroma bytes reach which pixel: the fast kernels' tile front
// end (bt709_tile.h TileIn) and the general kernels' chroma fetch below.  It is a parameter of the __global__ kernels and of
// that front end, never of a body inlined under a kernel that had none: that layer changed the NV12 kernels' code
// (profiles/r14_layout_template_isa.txt).
//
// Fast path.  Preconditions (checked by the host shim): width % 4 == 0; y, cbcr and alpha pointers and strides 4-byte aligned
// (kChromaI420: the U pointer and the chroma pitch 2-byte aligned; v_offset = (H/2) x pitch then is, too); output pointer and
// stride 16-byte aligned.
//
// FORM, the first template argument of decode_quads and decode_blocks, is the layout plus kFormStraight for the straight-alpha
// instantiations of their alpha forms (BT709HIP_OPT_UNPREMULTIPLY, DESIGN.md 3.9: each pixel's R, G, B divided by its alpha byte
// before the word is packed -- bt709_unpremultiply.h).  One argument and not a fifth: the instantiations that existed keep their
// symbols (the ISA tests and profiles name them) and their code (profiles/r15_straight_alpha_isa.txt).
template <uint32_t FORM, bool HAS_ALPHA, bool NT, bool QUANT>
__global__ void __launch_bounds__(kMaxBlockThreads)
decode_quads(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  quads_body<form_layout(FORM), HAS_ALPHA, NT, QUANT, false, kOverOff, form_straight(FORM)>(p, lds_raw);
}

// The plain kernel over a LOG-bucket table (DecodeParams::unit1_shift == 16; transfer_tables.h TransferTable::buckets_log):
// the LINEAR mode's 4 096 uniform buckets become 645 -- 5 KiB staged per workgroup instead of 33 -- for one shift per channel.
// One process, one ring, 4K, LINEAR mode (profiles/r05_ab_linear_log.txt), against the first half of round 5's answer to the
// 33 KiB table (the same body over 2 / 4 row pairs per workgroup, `decode_nv12_quads_rows`, itself 0.706 -> 0.777 over the plain
// kernel): 256 / 64 / 32 / 8 / 1 frames per launch 0.788 / 0.763 / 0.767 / 0.721 / 0.472 against 0.778 / 0.706 / 0.708 /
// 0.648 / 0.451.  The rows kernel is gone.
template <uint32_t LAYOUT, bool NT>
__global__ void __launch_bounds__(kMaxBlockThreads)
decode_quads_log(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  quads_body<LAYOUT, false, NT, false, true>(p, lds_raw);
}

// The alpha decoder's kernel with the composite-over blend (BT709HIP_OPT_COMPOSITE_OVER): LDS- and VALU-bound where the plain
// kernel is HBM-bound -- 48 to 72 LDS reads per quad.  Streaming accesses throughout.
template <uint32_t LAYOUT, int OVER>
__global__ void __launch_bounds__(kMaxBlockThreads)
decode_quads_over(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  quads_body<LAYOUT, true, true, true, false, OVER>(p, lds_raw);
}

// ---------------------------------------------------------------------------
// General path: any even width/height, any stride, byte-aligned planes, 4-byte
// aligned output.  One lane per 2x2 block, grid-strided over row pairs.  Correctness
// first; used for ragged or misaligned frames only.  That correctness is pinned by tests/test_decode_variants.py: all 2^24
// triples through every instantiation below, and the grid-stride loop, both forms of frame_planes and the over kernels at
// launch shapes computed from the device.
// Block bx of row pair rp takes its chroma from bytes 2 bx, 2 bx + 1 of the CbCr row (kChromaNV12), or from byte bx of the U row
// and of the V row v_offset bytes behind it (kChromaI420; bx < W/2: inside the row's W/2 bytes of either plane).
// ---------------------------------------------------------------------------
template <uint32_t FORM, bool HAS_ALPHA, bool QUANT>
__global__ void __launch_bounds__(kBlockThreads)
decode_blocks(const DecodeParams p) {
  constexpr bool PLANAR = form_layout(FORM) == kChromaI420;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  if (!QUANT) {
    stage_table(lds_raw, p.table_unit, p.table_unit_bytes);
    __syncthreads();
  }

  const UnitLookup ul = unit_lookup(p, lds_raw);
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
      const float y[4] = {byte_value(y0[2 * bx]), byte_value(y0[2 * bx + 1]), byte_value(y1[2 * bx]),
                          byte_value(y1[2 * bx + 1])};
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      if (HAS_ALPHA) {
        const uint8_t *a0 = f.alpha + static_cast<size_t>(2 * rp) * p.alpha_stride;
        const uint8_t *a1 = a0 + p.alpha_stride;
        a[0] = byte_value(a0[2 * bx]);
        a[1] = byte_value(a0[2 * bx + 1]);
        a[2] = byte_value(a1[2 * bx]);
        a[3] = byte_value(a1[2 * bx + 1]);
      }
      uint32_t out[4];
      decode_block<HAS_ALPHA, QUANT, form_straight(FORM)>(ul, y, byte_value(PLANAR ? cc[bx] : cc[2 * bx]), byte_value(PLANAR ? vv[bx] : cc[2 * bx + 1]), a, p.alpha_word, out);
      o0[2 * bx] = out[0];
      o0[2 * bx + 1] = out[1];
      o1[2 * bx] = out[2];
      o1[2 * bx + 1] = out[3];
    }
  }
}

// The alpha decoder's general path with the composite-over blend (BT709HIP_OPT_COMPOSITE_OVER): the same walk, each 2x2 block
// through over_pixel.  A kernel of its own: the plain kernel's code stays what it was.  Each output word is read (destination
// mode) and written by one lane alone.
template <uint32_t LAYOUT, int OVER>
__global__ void __launch_bounds__(kBlockThreads)
decode_blocks_over(const DecodeParams p) {
  constexpr bool PLANAR = LAYOUT == kChromaI420;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const OverLookup ol = stage_over_tables(lds_raw, p);
  __syncthreads();

  const FramePlanes f = frame_planes(p, blockIdx.y);
  const uint32_t bw = p.width >> 1;
  const uint32_t row_pairs = p.height >> 1;

  for (uint32_t rp = blockIdx.x; rp < row_pairs; rp += gridDim.x) {
    const uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    const uint8_t *y1 = y0 + p.y_stride;
    const uint8_t *a0 = f.alpha + static_cast<size_t>(2 * rp) * p.alpha_stride;
    const uint8_t *a1 = a0 + p.alpha_stride;
    const uint8_t *cc = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;  // the CbCr row, or the U row
    const uint8_t *vv = PLANAR ? cc + p.v_offset : nullptr;
    uint32_t *o0 = reinterpret_cast<uint32_t *>(f.out + static_cast<size_t>(2 * rp) * p.out_stride);
    uint32_t *o1 = reinterpret_cast<uint32_t *>(f.out + static_cast<size_t>(2 * rp + 1) * p.out_stride);
    for (uint32_t bx = threadIdx.x; bx < bw; bx += kBlockThreads) {
      const float y[4] = {byte_value(y0[2 * bx]), byte_value(y0[2 * bx + 1]), byte_value(y1[2 * bx]), byte_value(y1[2 * bx + 1])};
      const float a[4] = {byte_value(a0[2 * bx]), byte_value(a0[2 * bx + 1]), byte_value(a1[2 * bx]), byte_value(a1[2 * bx + 1])};
      uint32_t bg[4] = {0u, 0u, 0u, 0u};
      if (OVER == kOverDestination) bg[0] = o0[2 * bx], bg[1] = o0[2 * bx + 1], bg[2] = o1[2 * bx], bg[3] = o1[2 * bx + 1];
      const Chroma c = chroma_terms(byte_value(PLANAR ? cc[bx] : cc[2 * bx]), byte_value(PLANAR ? vv[bx] : cc[2 * bx + 1]));
      uint32_t out[4];
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        float x[3];
        pixel_rgb(y[px], c, x[0], x[1], x[2]);
        out[px] = over_pixel<OVER>(ol, p.over_lin, x, a[px], bg[px]);
      }
      o0[2 * bx] = out[0];
      o0[2 * bx + 1] = out[1];
      o1[2 * bx] = out[2];
      o1[2 * bx + 1] = out[3];
    }
  }
}

// ---------------------------------------------------------------------------
// +[BGRAToBT709Converter unconvert:outBGRAPixels:width:height:type:] on its actual input
// (Renderer/BGRAToBT709Converter.h:34-46; .m:146-198 unconvertSoftware): PACKED 4:4:4 words Y | Cb << 8 | Cr << 16, one
// per pixel, every pixel with its own chroma -> BGRA words.  Same per-pixel function as the NV12 kernels (the decoder's
// gamma; the reference hard-selects Apple196 at .m:165-173), alpha byte = the decoder's alpha fill (0 reproduces
// unconvertSoftware's words, .m:187-193).  4 B read + 4 B written per pixel.  VEC: a lane owns 4 consecutive pixels
// (16-byte load and store); otherwise one pixel per lane.  grid = (tiles, rows).
// ---------------------------------------------------------------------------
struct UnconvertParams {
  const uint8_t *in;   // packed words (frame blockIdx.z: in + z * in_step, or ins[z] when the table is used)
  uint8_t *out;        // BGRA words
  int64_t in_step, out_step;  // evenly spaced frames (bt709hip_unconvert_batch)
  const uint8_t *ins[kMaxBatch];
  uint8_t *outs[kMaxBatch];
  uint32_t use_table;
  uint32_t in_stride, out_stride, width, height;
  const void *table_unit;
  uint32_t table_unit_bytes;
  float unit1_magic;  // DecodeParams::unit1_*
  uint32_t unit1_first, unit1_shift;
  uint32_t alpha_word;
};

template <bool VEC, bool QUANT>
__global__ void __launch_bounds__(kBlockThreads)
unconvert_packed444(const UnconvertParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  // VEC: a lane owns 4 consecutive pixels of TWO consecutive rows (height is even: BGRAToBT709Converter.m:69-74), both 16-byte
  // loads issued before the table is staged -- the table's 4 KiB are then shared by 2 048 pixels instead of 1 024 and the
  // loads overlap the staging, as in the 1:1 kernel (round 4: 12.7 -> 11.x us per 4K frame, tools/bench_unconvert.py).
  // Frame words are touched once: non-temporal.  !VEC: one pixel per lane, one row per workgroup row, any alignment.
  constexpr uint32_t N = VEC ? 4 : 1, ROWS = VEC ? 2 : 1;
  const uint32_t row0 = blockIdx.y * ROWS;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // group of N pixels
  const uint8_t *frame_in = p.use_table ? p.ins[blockIdx.z] : p.in + static_cast<int64_t>(blockIdx.z) * p.in_step;
  uint8_t *frame_out = p.use_table ? p.outs[blockIdx.z] : p.out + static_cast<int64_t>(blockIdx.z) * p.out_step;
  const bool live = i * N < p.width;
  const uint32_t ic = live ? i : 0u;  // lanes past the row's end load a valid group and do not store (every lane stages the table)
  uint32_t w[ROWS][N];
#pragma unroll
  for (uint32_t r = 0; r < ROWS; ++r) {
    const uint8_t *in = frame_in + static_cast<size_t>(row0 + r) * p.in_stride;
    if (VEC) {
      const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(in + 16 * ic));
      w[r][0] = v.x, w[r][N > 1 ? 1 : 0] = v.y, w[r][N > 2 ? 2 : 0] = v.z, w[r][N > 3 ? 3 : 0] = v.w;
    } else {
      w[r][0] = *reinterpret_cast<const uint32_t *>(in + 4 * ic);
    }
  }
  if (!QUANT) {
    stage_table(lds_raw, p.table_unit, p.table_unit_bytes);  // after the loads are in flight
    __syncthreads();
  }
  const UnitLookup ul = unit_lookup(p, lds_raw);
  if (!live) return;
#pragma unroll
  for (uint32_t r = 0; r < ROWS; ++r) {
    float x[3 * N];
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
      const Chroma c = chroma_terms(byte_of(w[r][k], 1), byte_of(w[r][k], 2));
      pixel_rgb(byte_of(w[r][k], 0), c, x[3 * k], x[3 * k + 1], x[3 * k + 2]);
    }
    uint32_t o[N];
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
      uint32_t b[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        b[ch] = QUANT ? quantise_byte(x[3 * k + ch]) : bucket_byte(ul, x[3 * k + ch], __float_as_uint(__fadd_rn(x[3 * k + ch], ul.magic)) >> ul.shift);
      o[k] = pack_bgra(b[0], b[1], b[2], p.alpha_word);
    }
    uint8_t *out = frame_out + static_cast<size_t>(row0 + r) * p.out_stride;
    if (VEC) {
      u32x4 v;
      v.x = o[0], v.y = o[N > 1 ? 1 : 0], v.z = o[N > 2 ? 2 : 0], v.w = o[N > 3 ? 3 : 0];
      __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(out + 16 * i));
    } else {
      *reinterpret_cast<uint32_t *>(out + 4 * i) = o[0];
    }
  }
}

const char *launch_unconvert(const DecodeParams &t, const UnconvertBatch &b, size_t in_stride, size_t out_stride, uint32_t width, uint32_t height,
                             bool vec, bool quantiser, hipStream_t stream) {
  UnconvertParams p;
  std::memset(&p, 0, sizeof p);
  p.in = static_cast<const uint8_t *>(b.in[0]);
  p.out = static_cast<uint8_t *>(b.out[0]);
  p.in_step = b.in_step;
  p.out_step = b.out_step;
  p.use_table = b.uniform ? 0u : 1u;
  if (!b.uniform)
    for (int i = 0; i < b.count && i < kMaxBatch; ++i) p.ins[i] = static_cast<const uint8_t *>(b.in[i]), p.outs[i] = static_cast<uint8_t *>(b.out[i]);
  p.in_stride = static_cast<uint32_t>(in_stride);
  p.out_stride = static_cast<uint32_t>(out_stride);
  p.width = width;
  p.height = height;
  p.table_unit = t.table_unit;
  p.table_unit_bytes = t.table_unit_bytes;
  p.unit1_magic = t.unit1_magic;
  p.unit1_first = t.unit1_first;
  p.unit1_shift = t.unit1_shift;
  p.alpha_word = t.alpha_word;
  const uint32_t groups = vec ? width / 4 : width;
  const dim3 grid((groups + kBlockThreads - 1) / kBlockThreads, vec ? height / 2 : height, static_cast<uint32_t>(b.count));  // vec: two rows per workgroup row
  const size_t lds = quantiser ? 0 : t.table_unit_bytes;
  if (vec) {
    if (quantiser) hipLaunchKernelGGL((unconvert_packed444<true, true>), grid, dim3(kBlockThreads), lds, stream, p);
    else hipLaunchKernelGGL((unconvert_packed444<true, false>), grid, dim3(kBlockThreads), lds, stream, p);
  } else {
    if (quantiser) hipLaunchKernelGGL((unconvert_packed444<false, true>), grid, dim3(kBlockThreads), lds, stream, p);
    else hipLaunchKernelGGL((unconvert_packed444<false, false>), grid, dim3(kBlockThreads), lds, stream, p);
  }
  return vec ? "unconvert_packed444<vec>" : "unconvert_packed444";
}

// ---------------------------------------------------------------------------
// host-callable launchers (no HIP types in the signature beyond hipStream_t)
// ---------------------------------------------------------------------------
LaunchShape &last_launch_shape() {
  static thread_local LaunchShape shape = {};
  return shape;
}

namespace {

// The kernel of a launch that launch_decode has planned and recorded -- its grid, block and LDS bytes, the band map in `p` --
// for `variant`, `over`, `quant` (the sRGB mode or an alpha decoder) and `nontemporal`.  The names are what
// bt709hip_last_kernel_name reports.
template <uint32_t LAYOUT>
const char *launch_decode_kernel(const DecodeParams &p, const dim3 &grid, const dim3 &block, size_t lds, int variant, uint32_t over,
                                 bool has_alpha, bool quant, bool nontemporal, hipStream_t stream) {
  constexpr bool PLANAR = LAYOUT == kChromaI420;
  if (variant == kVariantQuads) {
    if (over == kOverDestination) {
      hipLaunchKernelGGL((decode_quads_over<LAYOUT, kOverDestination>), grid, block, lds, stream, p);
      return PLANAR ? "decode_i420_quads<alpha,over>" : "decode_nv12_quads<alpha,over>";
    }
    if (over != kOverOff) {
      hipLaunchKernelGGL((decode_quads_over<LAYOUT, kOverColour>), grid, block, lds, stream, p);
      return PLANAR ? "decode_i420_quads<alpha,over-colour>" : "decode_nv12_quads<alpha,over-colour>";
    }
    if (has_alpha && p.straight_alpha) {
      hipLaunchKernelGGL((decode_quads<LAYOUT | kFormStraight, true, true, true>), grid, block, lds, stream, p);
      return PLANAR ? "decode_i420_quads<alpha,straight>" : "decode_nv12_quads<alpha,straight>";
    }
    if (has_alpha) {
      hipLaunchKernelGGL((decode_quads<LAYOUT, true, true, true>), grid, block, lds, stream, p);
      return PLANAR ? "decode_i420_quads<alpha>" : "decode_nv12_quads<alpha>";
    }
    if (quant) {
      if (nontemporal) hipLaunchKernelGGL((decode_quads<LAYOUT, false, true, true>), grid, block, lds, stream, p);
      else hipLaunchKernelGGL((decode_quads<LAYOUT, false, false, true>), grid, block, lds, stream, p);
      if (nontemporal) return PLANAR ? "decode_i420_quads<nt,quantiser>" : "decode_nv12_quads<nt,quantiser>";
      return PLANAR ? "decode_i420_quads<quantiser>" : "decode_nv12_quads<quantiser>";
    }
    if (p.unit1_shift != 0) {  // log-bucket table (the LINEAR mode)
      if (nontemporal) hipLaunchKernelGGL((decode_quads_log<LAYOUT, true>), grid, block, lds, stream, p);
      else hipLaunchKernelGGL((decode_quads_log<LAYOUT, false>), grid, block, lds, stream, p);
      if (nontemporal) return PLANAR ? "decode_i420_quads_log<nt>" : "decode_nv12_quads_log<nt>";
      return PLANAR ? "decode_i420_quads_log" : "decode_nv12_quads_log";
    }
    if (nontemporal) {
      hipLaunchKernelGGL((decode_quads<LAYOUT, false, true, false>), grid, block, lds, stream, p);
      return PLANAR ? "decode_i420_quads<nt>" : "decode_nv12_quads<nt>";
    }
    hipLaunchKernelGGL((decode_quads<LAYOUT, false, false, false>), grid, block, lds, stream, p);
    return PLANAR ? "decode_i420_quads" : "decode_nv12_quads";
  }
  if (over == kOverDestination) {
    hipLaunchKernelGGL((decode_blocks_over<LAYOUT, kOverDestination>), grid, block, lds, stream, p);
    return PLANAR ? "decode_i420_blocks<alpha,over>" : "decode_nv12_blocks<alpha,over>";
  }
  if (over != kOverOff) {
    hipLaunchKernelGGL((decode_blocks_over<LAYOUT, kOverColour>), grid, block, lds, stream, p);
    return PLANAR ? "decode_i420_blocks<alpha,over-colour>" : "decode_nv12_blocks<alpha,over-colour>";
  }
  if (has_alpha && p.straight_alpha) {
    hipLaunchKernelGGL((decode_blocks<LAYOUT | kFormStraight, true, true>), grid, block, lds, stream, p);
    return PLANAR ? "decode_i420_blocks<alpha,straight>" : "decode_nv12_blocks<alpha,straight>";
  }
  if (has_alpha) {
    hipLaunchKernelGGL((decode_blocks<LAYOUT, true, true>), grid, block, lds, stream, p);
    return PLANAR ? "decode_i420_blocks<alpha>" : "decode_nv12_blocks<alpha>";
  }
  if (quant) {
    hipLaunchKernelGGL((decode_blocks<LAYOUT, false, true>), grid, block, lds, stream, p);
    return PLANAR ? "decode_i420_blocks<quantiser>" : "decode_nv12_blocks<quantiser>";
  }
  hipLaunchKernelGGL((decode_blocks<LAYOUT, false, false>), grid, block, lds, stream, p);
  return PLANAR ? "decode_i420_blocks" : "decode_nv12_blocks";
}

}  // namespace

const char *launch_decode(const DecodeParams &p_in, int frames, int variant, bool has_alpha, bool quantiser, bool nontemporal,
                          int xcd_bands, uint32_t grid_x, uint32_t block_threads, hipStream_t stream) {
  const bool quant = quantiser || has_alpha;  // the sRGB mode: arithmetic, no table
  const uint32_t over = has_alpha ? p_in.over_mode : kOverOff;  // BT709HIP_OPT_COMPOSITE_OVER: the *_over kernels and their two tables
  const size_t lds = over != kOverOff ? p_in.table_encode_bytes + kOverLinBytes : (quant ? 0 : p_in.table_unit_bytes);
  const BandPlan plan = plan_bands(frames, variant == kVariantQuads && xcd_bands, p_in.uniform, kXcdBandMinFrames);
  if (plan.banded && plan.tail) {
    launch_decode(p_in, plan.banded, variant, has_alpha, quantiser, nontemporal, xcd_bands, grid_x, block_threads, stream);
    DecodeParams tail = p_in;
    advance_frames(tail, plan.banded);
    return launch_decode(tail, plan.tail, variant, has_alpha, quantiser, nontemporal, 0, grid_x, block_threads, stream);
  }
  DecodeParams p = p_in;
  // general path: grid_x = workgroups per frame, grid-strided over row pairs
  dim3 grid(grid_x, static_cast<uint32_t>(frames), 1), block(kBlockThreads, 1, 1);
  if (variant == kVariantQuads) {
    // grid_x = tiles per row pair; narrow frames stack row pairs in blockDim.y
    const uint32_t by = quads_rows_per_block(block_threads, grid_x);
    grid = dim3(grid_x, (p.height / 2 + by - 1) / by, static_cast<uint32_t>(frames));
    block = dim3(block_threads, by, 1);
    if (plan.banded) grid = band_grid(p, static_cast<uint32_t>(xcd_bands), grid);
  }
  record_launch(grid, block, variant == kVariantQuads ? p.xcd_bands : 0);
  // the plan does not depend on the chroma layout, only the kernel does
  if (p.chroma_layout == kChromaI420) return launch_decode_kernel<kChromaI420>(p, grid, block, lds, variant, over, has_alpha, quant, nontemporal, stream);
  return launch_decode_kernel<kChromaNV12>(p, grid, block, lds, variant, over, has_alpha, quant, nontemporal, stream);
}

// the table kernels' dynamic-LDS cap
hipError_t prepare_kernels() {
  const void *fns[] = {
      reinterpret_cast<const void *>(&decode_quads<kChromaNV12, true, true, true>),
      reinterpret_cast<const void *>(&decode_quads<kChromaNV12, false, true, true>),
      reinterpret_cast<const void *>(&decode_quads<kChromaNV12, false, false, true>),
      reinterpret_cast<const void *>(&decode_quads<kChromaNV12, false, true, false>),
      reinterpret_cast<const void *>(&decode_quads<kChromaNV12, false, false, false>),
      reinterpret_cast<const void *>(&decode_quads_log<kChromaNV12, true>),
      reinterpret_cast<const void *>(&decode_quads_log<kChromaNV12, false>),
      reinterpret_cast<const void *>(&unconvert_packed444<true, false>),
      reinterpret_cast<const void *>(&unconvert_packed444<false, false>),
      reinterpret_cast<const void *>(&decode_blocks<kChromaNV12, true, true>),
      reinterpret_cast<const void *>(&decode_blocks<kChromaNV12, false, true>),
      reinterpret_cast<const void *>(&decode_blocks<kChromaNV12, false, false>),
      reinterpret_cast<const void *>(&decode_quads<kChromaI420, false, true, false>),
      reinterpret_cast<const void *>(&decode_quads<kChromaI420, false, false, false>),
      reinterpret_cast<const void *>(&decode_quads_log<kChromaI420, true>),
      reinterpret_cast<const void *>(&decode_quads_log<kChromaI420, false>),
      reinterpret_cast<const void *>(&decode_blocks<kChromaI420, false, false>),
  };
  return raise_lds_cap(fns, kRepLdsBytes);
}

}  // namespace bt709
