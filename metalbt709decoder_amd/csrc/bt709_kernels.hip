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
// end (bt709_tile.h TileIn) and the general kernels' chroma fetch (blocks_body).  It is a parameter of the __global__ kernels and of
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

// General path: ragged or misaligned frames, one lane per 2x2 block.  The walk is bt709_decode_body.h blocks_body (its contract and
// the tests that pin it are described there); the kernel stages the table ahead of it.  FORM as for decode_quads.
template <uint32_t FORM, bool HAS_ALPHA, bool QUANT>
__global__ void __launch_bounds__(kBlockThreads)
decode_blocks(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  if (!QUANT) {
    stage_table(lds_raw, p.table_unit, p.table_unit_bytes);
    __syncthreads();
  }
  blocks_body<form_layout(FORM), HAS_ALPHA, QUANT, kOverOff, form_straight(FORM)>(p, unit_lookup(p, lds_raw), OverLookup{});
}

// The alpha decoder's general path with the composite-over blend (BT709HIP_OPT_COMPOSITE_OVER): the same walk, each 2x2 block
// through over_pixel.  A kernel of its own: the plain kernel's code stays what it was.
template <uint32_t LAYOUT, int OVER>
__global__ void __launch_bounds__(kBlockThreads)
decode_blocks_over(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const OverLookup ol = stage_over_tables(lds_raw, p);
  __syncthreads();
  blocks_body<LAYOUT, true, true, OVER>(p, UnitLookup{}, ol);
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

namespace {
// The four instantiations: the selector, the kernel, and whether it stages the table in dynamic LDS (prepare_kernels)
struct UnconvertKernel {
  bool vec, quantiser;
  void (*fn)(const UnconvertParams);
  bool stages_table;
};
const UnconvertKernel kUnconvertKernels[] = {
    {true, true, unconvert_packed444<true, true>, false},
    {true, false, unconvert_packed444<true, false>, true},
    {false, true, unconvert_packed444<false, true>, false},
    {false, false, unconvert_packed444<false, false>, true},
};
}  // namespace

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
  for (const UnconvertKernel &k : kUnconvertKernels)
    if (k.vec == vec && k.quantiser == quantiser) hipLaunchKernelGGL(k.fn, grid, dim3(kBlockThreads), lds, stream, p);
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

// One row per selectable 1:1 kernel: the selector, the kernel for either chroma layout, the two names bt709hip_last_kernel_name
// reports, and whether the kernel stages a table in dynamic LDS -- prepare_kernels raises the cap of exactly those, so a kernel
// cannot be launched from here and be missing there.  A selector field is a value or kAny; the FIRST row that matches is the
// launch's kernel, so the rows of a variant run from the most specific form to the plain one.  `quant`: the sRGB mode or an alpha
// decoder (arithmetic, no table); `log`: a log-bucket table (the LINEAR mode; the general path takes the shift at run time).
struct DecodeKernel {
  int variant, over, alpha, straight, quant, log, nt;
  bool stages_table;
  void (*fn[2])(const DecodeParams);  // [chroma layout]
  const char *name[2];
};
// KERNEL<layout | FORM, ...>; both names from one suffix
#define DECODE_KERNEL(variant, over, alpha, straight, quant, log, nt, stages_table, suffix, KERNEL, FORM, ...)                               \
  {variant, over, alpha, straight, quant, log, nt, stages_table, {KERNEL<kChromaNV12 | (FORM), __VA_ARGS__>, KERNEL<kChromaI420 | (FORM), __VA_ARGS__>}, \
   {"decode_nv12_" suffix, "decode_i420_" suffix}}
const DecodeKernel kDecodeKernels[] = {
    //            variant         over              alpha straight quant log   nt    stages
    DECODE_KERNEL(kVariantQuads,  kOverDestination, kAny, kAny,    kAny, kAny, kAny, true,  "quads<alpha,over>", decode_quads_over, 0, kOverDestination),
    DECODE_KERNEL(kVariantQuads,  kOverColour,      kAny, kAny,    kAny, kAny, kAny, true,  "quads<alpha,over-colour>", decode_quads_over, 0, kOverColour),
    DECODE_KERNEL(kVariantQuads,  kOverOff,         1,    1,       kAny, kAny, kAny, false, "quads<alpha,straight>", decode_quads, kFormStraight, true, true, true),
    DECODE_KERNEL(kVariantQuads,  kOverOff,         1,    kAny,    kAny, kAny, kAny, false, "quads<alpha>", decode_quads, 0, true, true, true),
    DECODE_KERNEL(kVariantQuads,  kOverOff,         0,    kAny,    1,    kAny, 1,    false, "quads<nt,quantiser>", decode_quads, 0, false, true, true),
    DECODE_KERNEL(kVariantQuads,  kOverOff,         0,    kAny,    1,    kAny, 0,    false, "quads<quantiser>", decode_quads, 0, false, false, true),
    DECODE_KERNEL(kVariantQuads,  kOverOff,         0,    kAny,    0,    1,    1,    true,  "quads_log<nt>", decode_quads_log, 0, true),
    DECODE_KERNEL(kVariantQuads,  kOverOff,         0,    kAny,    0,    1,    0,    true,  "quads_log", decode_quads_log, 0, false),
    DECODE_KERNEL(kVariantQuads,  kOverOff,         0,    kAny,    0,    0,    1,    true,  "quads<nt>", decode_quads, 0, false, true, false),
    DECODE_KERNEL(kVariantQuads,  kOverOff,         0,    kAny,    0,    0,    0,    true,  "quads", decode_quads, 0, false, false, false),
    DECODE_KERNEL(kVariantBlocks, kOverDestination, kAny, kAny,    kAny, kAny, kAny, true,  "blocks<alpha,over>", decode_blocks_over, 0, kOverDestination),
    DECODE_KERNEL(kVariantBlocks, kOverColour,      kAny, kAny,    kAny, kAny, kAny, true,  "blocks<alpha,over-colour>", decode_blocks_over, 0, kOverColour),
    DECODE_KERNEL(kVariantBlocks, kOverOff,         1,    1,       kAny, kAny, kAny, false, "blocks<alpha,straight>", decode_blocks, kFormStraight, true, true),
    DECODE_KERNEL(kVariantBlocks, kOverOff,         1,    kAny,    kAny, kAny, kAny, false, "blocks<alpha>", decode_blocks, 0, true, true),
    DECODE_KERNEL(kVariantBlocks, kOverOff,         0,    kAny,    1,    kAny, kAny, false, "blocks<quantiser>", decode_blocks, 0, false, true),
    DECODE_KERNEL(kVariantBlocks, kOverOff,         0,    kAny,    0,    kAny, kAny, true,  "blocks", decode_blocks, 0, false, false),
};
#undef DECODE_KERNEL

// The kernel of a launch that launch_decode has planned and recorded -- its grid, block and LDS bytes, the band map in `p` --
// for `variant`, `over`, `quant` (the sRGB mode or an alpha decoder) and `nontemporal`.
const char *launch_decode_kernel(const DecodeParams &p, const dim3 &grid, const dim3 &block, size_t lds, int variant, uint32_t over,
                                 bool has_alpha, bool quant, bool nontemporal, hipStream_t stream) {
  const uint32_t layout = p.chroma_layout == kChromaI420 ? kChromaI420 : kChromaNV12;
  for (const DecodeKernel &k : kDecodeKernels) {
    if (k.variant != variant || !selects(k.over, static_cast<int>(over)) || !selects(k.alpha, has_alpha) || !selects(k.straight, p.straight_alpha != 0) ||
        !selects(k.quant, quant) || !selects(k.log, p.unit1_shift != 0) || !selects(k.nt, nontemporal))
      continue;
    hipLaunchKernelGGL(k.fn[layout], grid, block, lds, stream, p);
    return k.name[layout];
  }
  return nullptr;  // unreachable: the rows of a variant end in one that takes every remaining selector
}

}  // namespace

const char *launch_decode(const DecodeParams &p_in, int frames, int variant, bool has_alpha, bool quantiser, bool nontemporal,
                          int xcd_bands, uint32_t grid_x, uint32_t block_threads, hipStream_t stream) {
  // a planar CHW target (BT709HIP_FORMAT_CHW_*): the same plan over the kernels of bt709_chw.hip
  if (p_in.chw_elem != kChwNone) return launch_decode_chw(p_in, frames, variant, has_alpha, quantiser, nontemporal, xcd_bands, grid_x, block_threads, stream);
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
  return launch_decode_kernel(p, grid, block, lds, variant, over, has_alpha, quant, nontemporal, stream);
}

// the dynamic-LDS cap of every kernel above that stages a table, both layouts
hipError_t prepare_kernels() {
  for (const DecodeKernel &k : kDecodeKernels) {
    const void *fns[] = {reinterpret_cast<const void *>(k.fn[0]), reinterpret_cast<const void *>(k.fn[1])};
    if (const hipError_t e = k.stages_table ? raise_lds_cap(fns, kRepLdsBytes) : hipSuccess) return e;
  }
  for (const UnconvertKernel &k : kUnconvertKernels) {
    const void *fns[] = {reinterpret_cast<const void *>(k.fn)};
    if (const hipError_t e = k.stages_table ? raise_lds_cap(fns, kRepLdsBytes) : hipSuccess) return e;
  }
  return prepare_chw_kernels();  // the CHW twins of the 1:1 kernels (bt709_chw.hip)
}

}  // namespace bt709
