// CDNA4 (gfx950) kernels of pass 1 into PLANAR C x H x W tensors (BT709HIP_FORMAT_CHW_U8 / _F16 / _F32): what an
// inference pipeline takes -- planes R, G, B (and A from an alpha decoder) of bytes, or of binary16 / binary32 values scaled by
// 1/255 and normalised per channel -- written by the decode itself: 1.5 B read + 3, 6 or 12 B written per pixel, where "decode to
// BGRA8, then permute, convert and normalise" moves 12.5, 15.5 or 21.5 in two launches and holds a scratch surface.
//
// The arithmetic is the 1:1 kernels' own text (bt709_decode_body.h decode_quad / decode_block): these kernels take the BGRA words
// it produces and take them apart again -- CHW_U8 is the BGRA8 decode's bytes by construction, in every gamma form and either
// chroma layout -- and the float elements are bt709_chw_norm.h on those bytes.  They are __global__ kernels of their own with a
// body of their own: nothing here is inlined under a kernel of bt709_kernels.hip, whose code stays what it was
// (profiles/r21_chw_isa.txt).
//
// Fast path (decode_quads_chw).  quads_body's shape and launch plans: TileIn load, table staging, pin, arithmetic, predicated
// stores; grid (tiles, row pairs, frames), the XCD-band map and the tail split of launch_decode.  Preconditions (host shim): the
// 1:1 fast path's on the input side, width % 4 == 0, plane 0 and the pitch 4 e-aligned (e = bytes per element; the plane offsets
// c x H x pitch then are, too).  A lane owns quad q: per plane and row ONE store of 4 e bytes at 4 e q, consecutive lanes owning
// consecutive quads -- a store instruction of a wave fills 256 B, 512 B or 1 KiB of whole lines (the rule of bt709_tile.h and
// bt709_rgba16f.hip: half lines cost 2.4x, a lane owning adjacent quads 3x).
// General path (decode_blocks_chw): blocks_body's walk, one lane per 2x2 block, element-sized stores, any even size, any
// e-aligned base and pitch; the element type is a uniform run-time branch at the store (correctness first, as its BGRA8 twin).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bt709_chw_norm.h"
#include "bt709_decode_body.h"
#include "bt709_launch.h"

namespace bt709 {
namespace {

// Four BGRA words of one row of a quad -> the row's four bytes of each plane, one dword per plane: {B, G, R, A}[k] holds pixel
// 0..3's byte, LSB first.  Two levels of v_perm_b32 (selector bytes LSB first; 0-3: the second operand, 4-7: the first):
// 4 + 3 per row, 4 + 4 with the alpha plane.
struct QuadBytes {
  uint32_t b, g, r, a;
};
template <bool HAS_ALPHA>
__device__ __forceinline__ QuadBytes transpose_quad(const u32x4 &w) {
  const uint32_t br01 = __builtin_amdgcn_perm(w.y, w.x, 0x06020400u);  // B0 B1 R0 R1
  const uint32_t br23 = __builtin_amdgcn_perm(w.w, w.z, 0x06020400u);
  const uint32_t ga01 = __builtin_amdgcn_perm(w.y, w.x, 0x07030501u);  // G0 G1 A0 A1
  const uint32_t ga23 = __builtin_amdgcn_perm(w.w, w.z, 0x07030501u);
  QuadBytes q;
  q.b = __builtin_amdgcn_perm(br23, br01, 0x05040100u);
  q.r = __builtin_amdgcn_perm(br23, br01, 0x07060302u);
  q.g = __builtin_amdgcn_perm(ga23, ga01, 0x05040100u);
  q.a = HAS_ALPHA ? __builtin_amdgcn_perm(ga23, ga01, 0x07060302u) : 0u;
  return q;
}

// two values -> their binary16 codes in one word: v_cvt_pk_f16_f32, chw_half_bits' conversion (round to nearest even) two at a time
__device__ __forceinline__ uint32_t half_pair(float lo, float hi) {
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
}

// What a lane stores for one row of one plane of its quad: 4 e bytes
template <uint32_t ELEM>
struct ChwRow;
template <>
struct ChwRow<kChwU8> {
  uint32_t v;
};
template <>
struct ChwRow<kChwF16> {
  u32x2 v;
};
template <>
struct ChwRow<kChwF32> {
  u32x4 v;
};

// plane c (0 R, 1 G, 2 B, 3 A) of a quad's row from its words; BYTE: where the plane's byte sits in a BGRA word
template <uint32_t ELEM, int BYTE, bool COLOUR>
__device__ __forceinline__ ChwRow<ELEM> chw_row(const u32x4 &w, float scale, float bias) {
  ChwRow<ELEM> out;
  float t[4];
  const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float code = static_cast<float>((word[k] >> (8 * BYTE)) & 0xffu);  // v_cvt_f32_ubyteN
    t[k] = COLOUR ? chw_norm(code, scale, bias) : chw_unit(code);
  }
  if constexpr (ELEM == kChwF16) {
    // rounded to binary32 first and THEN to binary16, as the definition says: the pin keeps the conversion a conversion
#pragma unroll
    for (int k = 0; k < 4; ++k) asm("" : "+v"(t[k]));
    out.v = u32x2{half_pair(t[0], t[1]), half_pair(t[2], t[3])};
  } else {
    out.v = u32x4{__float_as_uint(t[0]), __float_as_uint(t[1]), __float_as_uint(t[2]), __float_as_uint(t[3])};
  }
  return out;
}

template <bool NT>
__device__ __forceinline__ void store_row(uint8_t *p, const ChwRow<kChwU8> &r) {
  if (NT) __builtin_nontemporal_store(r.v, reinterpret_cast<uint32_t *>(p));
  else *reinterpret_cast<uint32_t *>(p) = r.v;
}
template <bool NT>
__device__ __forceinline__ void store_row(uint8_t *p, const ChwRow<kChwF16> &r) {
  store8<NT>(p, r.v);
}
template <bool NT>
__device__ __forceinline__ void store_row(uint8_t *p, const ChwRow<kChwF32> &r) {
  store16<NT>(p, r.v);
}

// The planes' rows of one quad (rows[plane][0 top / 1 bottom]) from its decoded words
template <uint32_t ELEM, bool HAS_ALPHA>
__device__ __forceinline__ void chw_quad(const DecodeParams &p, const u32x4 &top, const u32x4 &bot, ChwRow<ELEM> (&rows)[HAS_ALPHA ? 4 : 3][2]) {
  if constexpr (ELEM == kChwU8) {
    const QuadBytes t = transpose_quad<HAS_ALPHA>(top), b = transpose_quad<HAS_ALPHA>(bot);
    rows[0][0].v = t.r, rows[0][1].v = b.r;
    rows[1][0].v = t.g, rows[1][1].v = b.g;
    rows[2][0].v = t.b, rows[2][1].v = b.b;
    if constexpr (HAS_ALPHA) rows[3][0].v = t.a, rows[3][1].v = b.a;
  } else {
    rows[0][0] = chw_row<ELEM, 2, true>(top, p.chw_scale[0], p.chw_bias[0]), rows[0][1] = chw_row<ELEM, 2, true>(bot, p.chw_scale[0], p.chw_bias[0]);
    rows[1][0] = chw_row<ELEM, 1, true>(top, p.chw_scale[1], p.chw_bias[1]), rows[1][1] = chw_row<ELEM, 1, true>(bot, p.chw_scale[1], p.chw_bias[1]);
    rows[2][0] = chw_row<ELEM, 0, true>(top, p.chw_scale[2], p.chw_bias[2]), rows[2][1] = chw_row<ELEM, 0, true>(bot, p.chw_scale[2], p.chw_bias[2]);
    if constexpr (HAS_ALPHA) rows[3][0] = chw_row<ELEM, 3, false>(top, 0.0f, 0.0f), rows[3][1] = chw_row<ELEM, 3, false>(bot, 0.0f, 0.0f);
  }
}

}  // namespace

// quads_body (bt709_decode_body.h) with the CHW store: the same front end, the same straight-line rule -- lanes past the row's end
// and row pairs past the frame's compute on a clamped quad, and only the stores are predicated: none is issued for q >= quads or
// rp >= row_pairs.  BOUNDS of a store: plane c <= planes - 1, row 2 rp + {0, 1} <= H - 1, bytes [4 e q, 4 e q + 4 e) with
// q <= W/4 - 1: inside the W e bytes of a row of a plane the surface has.
template <uint32_t LAYOUT, uint32_t ELEM, bool HAS_ALPHA, bool NT, bool QUANT, bool LOGIDX>
__global__ void __launch_bounds__(kMaxBlockThreads)
decode_quads_chw(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr int UNROLL = kQuadsPerLane;
  constexpr int PLANES = HAS_ALPHA ? 4 : 3;
  constexpr uint32_t QUAD_BYTES = 4 * chw_elem_bytes(ELEM);
  const BandedWork work = banded_work<true>(p.xcd_bands, p.frames_per_band);
  const FramePlanes f = frame_planes(p, work.frame);
  const uint32_t quads = p.width >> 2;
  const uint32_t row_pairs = p.height >> 1;
  const uint32_t rp_raw = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);  // scalar row pointers: quads_body has the why
  const uint32_t q0 = work.tile * (blockDim.x * UNROLL) + threadIdx.x;

  TileIn<LAYOUT, UNROLL, HAS_ALPHA> in;
  in.template load<NT>(f, p, rp_raw, row_pairs, q0, quads);
  if (!QUANT) {
    stage_table(lds_raw, p.table_unit, p.table_unit_bytes);  // after the tile's loads are in flight
    __syncthreads();
  }
  in.pin();

  const UnitLookup ul = unit_lookup(p, lds_raw);
  const uint64_t plane = static_cast<uint64_t>(p.height) * p.out_stride;  // plane c starts c x H x pitch behind plane 0: a 64-bit product
  uint8_t *o0 = f.out + static_cast<size_t>(2 * min(rp_raw, row_pairs - 1)) * p.out_stride;
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const uint32_t q = q0 + u * blockDim.x;
    u32x4 top, bot;
    decode_quad<HAS_ALPHA, QUANT, LOGIDX>(ul, in.ya[u], in.yb[u], in.cw[u], HAS_ALPHA ? in.aa[u] : 0u, HAS_ALPHA ? in.ab[u] : 0u, p.alpha_word, top, bot);
    ChwRow<ELEM> rows[PLANES][2];
    chw_quad<ELEM, HAS_ALPHA>(p, top, bot, rows);
    if (q < quads && rp_raw < row_pairs) {
#pragma unroll
      for (int c = 0; c < PLANES; ++c) {
        uint8_t *o = o0 + c * plane + static_cast<size_t>(QUAD_BYTES) * q;
        store_row<NT>(o, rows[c][0]);
        store_row<NT>(o + p.out_stride, rows[c][1]);
      }
    }
  }
}

namespace {
// one element of a plane (general path): `byte` as is, or normalised
__device__ __forceinline__ void store_elem(uint8_t *row, uint32_t x, uint32_t elem, uint32_t byte, bool colour, float scale, float bias) {
  if (elem == kChwU8) {
    row[x] = static_cast<uint8_t>(byte);
    return;
  }
  float t = colour ? chw_norm(static_cast<float>(byte), scale, bias) : chw_unit(static_cast<float>(byte));
  asm("" : "+v"(t));  // binary32 first, then binary16 (chw_row)
  if (elem == kChwF16) reinterpret_cast<uint16_t *>(row)[x] = chw_half_bits(t);
  else reinterpret_cast<float *>(row)[x] = t;
}
}  // namespace

// blocks_body's walk (bt709_decode_body.h) with the CHW store: one lane per 2x2 block, grid-strided over row pairs, every load a
// byte load and every store one element.  BOUNDS: rp < H/2 and bx < W/2 by the loops, so a store hits element 2 bx + {0, 1} <= W - 1
// of row 2 rp + {0, 1} <= H - 1 of plane c <= planes - 1.
template <uint32_t LAYOUT, bool HAS_ALPHA, bool QUANT>
__global__ void __launch_bounds__(kBlockThreads)
decode_blocks_chw(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr bool PLANAR = LAYOUT == kChromaI420;
  constexpr int PLANES = HAS_ALPHA ? 4 : 3;
  if (!QUANT) {
    stage_table(lds_raw, p.table_unit, p.table_unit_bytes);
    __syncthreads();
  }
  const UnitLookup ul = unit_lookup(p, lds_raw);
  const FramePlanes f = frame_planes(p, blockIdx.y);
  const uint32_t bw = p.width >> 1;
  const uint32_t row_pairs = p.height >> 1;
  const uint32_t elem = p.chw_elem;
  const uint64_t plane = static_cast<uint64_t>(p.height) * p.out_stride;

  for (uint32_t rp = blockIdx.x; rp < row_pairs; rp += gridDim.x) {
    const uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    const uint8_t *y1 = y0 + p.y_stride;
    const uint8_t *cc = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;  // the CbCr row, or the U row
    const uint8_t *vv = PLANAR ? cc + p.v_offset : nullptr;
    uint8_t *o0 = f.out + static_cast<size_t>(2 * rp) * p.out_stride;
    for (uint32_t bx = threadIdx.x; bx < bw; bx += kBlockThreads) {
      const float y[4] = {byte_value(y0[2 * bx]), byte_value(y0[2 * bx + 1]), byte_value(y1[2 * bx]), byte_value(y1[2 * bx + 1])};
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      if (HAS_ALPHA) {
        const uint8_t *a0 = f.alpha + static_cast<size_t>(2 * rp) * p.alpha_stride;
        const uint8_t *a1 = a0 + p.alpha_stride;
        a[0] = byte_value(a0[2 * bx]);
        a[1] = byte_value(a0[2 * bx + 1]);
        a[2] = byte_value(a1[2 * bx]);
        a[3] = byte_value(a1[2 * bx + 1]);
      }
      const float cb = byte_value(PLANAR ? cc[bx] : cc[2 * bx]), cr = byte_value(PLANAR ? vv[bx] : cc[2 * bx + 1]);
      uint32_t out[4];  // {tl, tr, bl, br}
      decode_block<HAS_ALPHA, QUANT>(ul, y, cb, cr, a, p.alpha_word, out);
#pragma unroll
      for (int c = 0; c < PLANES; ++c) {
        const int shift = c == 3 ? 24 : 16 - 8 * c;  // R, G, B, A of (A<<24)|(R<<16)|(G<<8)|B
        const float scale = p.chw_scale[c % 3], bias = p.chw_bias[c % 3];  // not read for the alpha plane
        uint8_t *r0 = o0 + c * plane, *r1 = r0 + p.out_stride;
        store_elem(r0, 2 * bx, elem, (out[0] >> shift) & 0xffu, c < 3, scale, bias);
        store_elem(r0, 2 * bx + 1, elem, (out[1] >> shift) & 0xffu, c < 3, scale, bias);
        store_elem(r1, 2 * bx, elem, (out[2] >> shift) & 0xffu, c < 3, scale, bias);
        store_elem(r1, 2 * bx + 1, elem, (out[3] >> shift) & 0xffu, c < 3, scale, bias);
      }
    }
  }
}

namespace {

// One row per selectable kernel, first match wins: bt709_kernels.hip kDecodeKernels' scheme with the element type among the
// selectors of the fast path.  `quant`: the sRGB mode or an alpha decoder; `log`: a log-bucket table (the LINEAR mode).
struct ChwKernel {
  int variant, elem, alpha, quant, log, nt;
  bool stages_table;
  void (*fn[2])(const DecodeParams);  // [chroma layout]
  const char *name[2];
};
// the selectors, then the kernel's own arguments <alpha, nt, quant, log>
#define CHW_QUADS(ELEM, ename, alpha, quant, log, nt, stages, suffix, ...)                                           \
  {kVariantQuads, static_cast<int>(ELEM), alpha, quant, log, nt, stages,                                             \
   {decode_quads_chw<kChromaNV12, ELEM, __VA_ARGS__>, decode_quads_chw<kChromaI420, ELEM, __VA_ARGS__>},             \
   {"decode_nv12_quads_chw<" ename suffix ">", "decode_i420_quads_chw<" ename suffix ">"}}
// the alpha decoder streams (as decode_quads<alpha>); the opaque decoder's three gamma forms, streaming or not
#define CHW_QUADS_ELEM(ELEM, ename)                                                              \
  CHW_QUADS(ELEM, ename, 1, kAny, kAny, kAny, false, ",alpha", true, true, true, false),         \
  CHW_QUADS(ELEM, ename, 0, 1, kAny, 1, false, ",nt,quantiser", false, true, true, false),       \
  CHW_QUADS(ELEM, ename, 0, 1, kAny, 0, false, ",quantiser", false, false, true, false),         \
  CHW_QUADS(ELEM, ename, 0, 0, 1, 1, true, ",nt,log", false, true, false, true),                 \
  CHW_QUADS(ELEM, ename, 0, 0, 1, 0, true, ",log", false, false, false, true),                   \
  CHW_QUADS(ELEM, ename, 0, 0, 0, 1, true, ",nt", false, true, false, false),                    \
  CHW_QUADS(ELEM, ename, 0, 0, 0, 0, true, "", false, false, false, false)
// the general path: one kernel per <alpha, quant> whatever the element type; the name says which it stored
#define CHW_BLOCKS_ELEM(ELEM, ename, alpha, quant, stages, suffix, ...)                                              \
  {kVariantBlocks, static_cast<int>(ELEM), alpha, quant, kAny, kAny, stages,                                         \
   {decode_blocks_chw<kChromaNV12, __VA_ARGS__>, decode_blocks_chw<kChromaI420, __VA_ARGS__>},                       \
   {"decode_nv12_blocks_chw<" ename suffix ">", "decode_i420_blocks_chw<" ename suffix ">"}}
#define CHW_BLOCKS(alpha, quant, stages, suffix, ...)                            \
  CHW_BLOCKS_ELEM(kChwU8, "u8", alpha, quant, stages, suffix, __VA_ARGS__),      \
  CHW_BLOCKS_ELEM(kChwF16, "f16", alpha, quant, stages, suffix, __VA_ARGS__),    \
  CHW_BLOCKS_ELEM(kChwF32, "f32", alpha, quant, stages, suffix, __VA_ARGS__)
const ChwKernel kChwKernels[] = {
    CHW_QUADS_ELEM(kChwU8, "u8"),
    CHW_QUADS_ELEM(kChwF16, "f16"),
    CHW_QUADS_ELEM(kChwF32, "f32"),
    CHW_BLOCKS(1, kAny, false, ",alpha", true, true),
    CHW_BLOCKS(0, 1, false, ",quantiser", false, true),
    CHW_BLOCKS(0, 0, true, "", false, false),
};
#undef CHW_BLOCKS
#undef CHW_BLOCKS_ELEM
#undef CHW_QUADS_ELEM
#undef CHW_QUADS

}  // namespace

// launch_decode's plan (bt709_kernels.hip) over the CHW kernels: the band map from kXcdBandMinFrames frames on, the tail of a
// uniform batch under the plain map, the same grid, block and launch record.  advance_frames moves plane 0; the planes follow it.
const char *launch_decode_chw(const DecodeParams &p_in, int frames, int variant, bool has_alpha, bool quantiser, bool nontemporal,
                              int xcd_bands, uint32_t grid_x, uint32_t block_threads, hipStream_t stream) {
  const bool quant = quantiser || has_alpha;
  const BandPlan plan = plan_bands(frames, variant == kVariantQuads && xcd_bands, p_in.uniform, kXcdBandMinFrames);
  if (plan.banded && plan.tail) {
    launch_decode_chw(p_in, plan.banded, variant, has_alpha, quantiser, nontemporal, xcd_bands, grid_x, block_threads, stream);
    DecodeParams tail = p_in;
    advance_frames(tail, plan.banded);
    return launch_decode_chw(tail, plan.tail, variant, has_alpha, quantiser, nontemporal, 0, grid_x, block_threads, stream);
  }
  DecodeParams p = p_in;
  const size_t lds = quant ? 0 : p.table_unit_bytes;
  dim3 grid(grid_x, static_cast<uint32_t>(frames), 1), block(kBlockThreads, 1, 1);
  if (variant == kVariantQuads) {
    const uint32_t by = quads_rows_per_block(block_threads, grid_x);
    grid = dim3(grid_x, (p.height / 2 + by - 1) / by, static_cast<uint32_t>(frames));
    block = dim3(block_threads, by, 1);
    if (plan.banded) grid = band_grid(p, static_cast<uint32_t>(xcd_bands), grid);
  }
  record_launch(grid, block, variant == kVariantQuads ? p.xcd_bands : 0);
  const uint32_t layout = p.chroma_layout == kChromaI420 ? kChromaI420 : kChromaNV12;
  for (const ChwKernel &k : kChwKernels) {
    if (k.variant != variant || k.elem != static_cast<int>(p.chw_elem) || !selects(k.alpha, has_alpha) || !selects(k.quant, quant) ||
        !selects(k.log, p.unit1_shift != 0) || !selects(k.nt, nontemporal))
      continue;
    hipLaunchKernelGGL(k.fn[layout], grid, block, lds, stream, p);
    return k.name[layout];
  }
  return nullptr;  // unreachable for chw_elem in kChwU8..kChwF32: the rows of a variant and element end in one that takes every remaining selector
}

hipError_t prepare_chw_kernels() {
  for (const ChwKernel &k : kChwKernels) {
    const void *fns[] = {reinterpret_cast<const void *>(k.fn[0]), reinterpret_cast<const void *>(k.fn[1])};
    if (const hipError_t e = k.stages_table ? raise_lds_cap(fns, kRepLdsBytes) : hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace bt709
