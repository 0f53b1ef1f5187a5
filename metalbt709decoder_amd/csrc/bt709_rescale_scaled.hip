// CDNA4 (gfx950) kernels of the FUSED decode + rescale to ANY output size, and of pass 2 alone
// (-[MetalScaleRenderContext renderScaled:...] + samplingShader: Renderer/MetalScaleRenderContext.m:55-105,
// Renderer/AAPLShaders.metal:73-85).  Arithmetic and tables: bt709_rescale.h.
//
//   decode_nv12_scaled     any output size, bilinear taps, one lane per output column walking strips of rows
//   decode_nv12_scaled_over   the same for an alpha decoder, each word blended over the destination or a colour before the store
//   render_scaled          pass 2 alone from an 8-bit or RGBA16Float intermediate
// Both walk a strip with walk_strip; each keeps its own fetch, its own conversion to linear light, its encode and its store.
// Launch selection is a table: kScaledKernels here, bt709_rescale_f16.hip's rows behind scaled_f16_kernels(), bt709_rescale_chw.hip's
// (planar CHW views) behind scaled_chw_kernels(), bt709_rescale_planar.hip's (planar I420 frames) behind scaled_planar_kernels(), kRenderKernels for pass 2 -- a launch looks its row up, prepare_scaled_kernels walks them all.
#include <atomic>

#include "bt709_scaled_strip.h"

namespace bt709 {

// ---------------------------------------------------------------------------
// Fused decode + bilinear rescale to ANY output size (MetalScaleRenderContext -renderScaled:
// for a view that is not an exact 2:1 of the frame).  Definition (ours: the reference leaves it
// to the sampler hardware):
//   sx = (ox + 0.5f) * (W / OW) - 0.5f,  x0 = floor(sx), fx = sx - x0, taps clamped to the edge
//   (same in y); each tap is decoded to its 8-bit sRGB value and linearised as the sRGB8 sampler
//   does; v = (((w00*l00 + w01*l01) + w10*l10) + w11*l11) with w00 = (1-fx)(1-fy), ...;
//   sRGB-encode, quantise.  For an exact 2:1 ratio every weight is 0.25 and this is bit for bit
//   the decode_nv12_half result.
// One lane per output column, walking a strip of `rows` consecutive output rows (grid = (ceil(OW /
// blockDim), strips, frames)): the horizontal tap positions and weights are computed once per lane, the
// vertical ones once per strip (lane i does row i; rows read them with v_readlane_b32), the 14 KiB of
// tables are staged once per workgroup -- of the launch, in the persistent form (see the kernel).  What round 2
// changed (4K -> 1440p, 8 frames per launch: 204 -> 255 Gpixel/s out; DESIGN 6.5 has every shape and every step):
//   * the ROW CACHE (RowCache): the two linearised rows of the previous output row stay in registers and only rows not
//     seen yet are decoded; the chroma products are kept the same way.  12 lookups per output pixel become 6 * scale_y;
//   * fetches are unconditional, rows ahead of the row being produced, in explicit register sets (walk_strip);
//   * planes are raw buffer resources (scalar row offset, 32-bit lane offset: no VALU address arithmetic).
// Tap fetch, as wide as the layout allows:
//   TAPS_WIDE  (planes and strides 4-byte aligned, width % 4 == 0, width >= 8): per source row ONE
//              aligned 8-byte load per plane that contains both horizontal taps, and one v_perm_b32 with
//              a per-lane selector (computed once) picks them out;
//   TAPS_PAIRS (CbCr plane 2-byte aligned): a tap's Cb,Cr with one 2-byte load;
//   TAPS_BYTES any layout: byte loads.
// 4-byte coalesced stores.
// ---------------------------------------------------------------------------
// (Closed: six whole alternative structures sat behind macros here until the commit before this comment, which holds the code.
//  Two strips per workgroup in a blockDim.y dimension: 224 against 240 Gpixel/s, 4K -> 1440p x 8 (profiles/r02_ab_scaled.txt).
//  The 24 KiB uniform encode table, 9 fewer VALU instructions per pixel but 32 KiB staged and 5 workgroups per CU: 194 (same file).
//  2 / 4 interleaved copies of the decode-side table: -2...-6 % / -2...-29 % on the five tuned shapes, occupancy being what the
//  copies cost (profiles/r03_ab_scaled_copies.txt); with 512- / 1 024-lane workgroups to hold them -3...-35 %, and 2 / 4 copies of
//  the 5 KiB encode-side table 1 % / 2-20 % slower (profiles/r05_ab_scaled_strips_copies.txt).
//  TAPS_ONCE as persistent workgroups: 1080p -> 4K x 8 24.7 against 19.8 us (profiles/r06_ab_scaled_share.txt).
//  No one-generation cut of short launches: one 4K -> 1440p frame 19.6 against 18.8 us (profiles/r06_ab_scaled_ahead.txt).)

// The kernel's walk behind its staged tables, as TEXT: decode_nv12_scaled_over below runs the same walk with scaled_strip in its
// over form, and the walk has to sit in the kernel function itself -- in a function that both kernels call, hipcc takes blockIdx /
// blockDim through the generic implicit-argument code and schedules the plain kernels' persistent forms differently, and their
// instruction streams are pinned (profiles/LAB.md, "Round 11").
#define BT709_SCALED_WALK(HAS_ALPHA, OVER, ov)                                                                                           \
  if (PERSISTENT) {                                                                                                                      \
    BT709_SCALED_ITEM_LOOP(HAS_ALPHA, OVER, Srgb8Light{r}, ov)                                                                           \
    return;                                                                                                                              \
  }                                                                                                                                      \
  const FramePlanes f = frame_planes(p, blockIdx.z);                                                                                     \
  const uint32_t ox = blockIdx.x * blockDim.x + threadIdx.x;                                                                             \
  const uint32_t oy0 = blockIdx.y * p.scaled_rows; /* < out_height: the grid has exactly the strips */                                   \
  const StripTaps vt = strip_taps(oy0, p.scale_y); /* before any lane leaves */                                                          \
  if (TAPS != TAPS_SHARED && TAPS != TAPS_ONCE && ox >= p.out_width) return; /* TAPS_SHARED / TAPS_ONCE: the wave works together */      \
  scaled_strip<TAPS, HAS_ALPHA, OVER>(p, Srgb8Light{r}, f, ox, oy0, min(oy0 + p.scaled_rows, p.out_height), vt, ov)

// A workgroup = 256 output columns x one strip of `scaled_rows` output rows of one frame; its waves share nothing but
// the single-copy tables (14 KiB staged per workgroup).
// PERSISTENT: the launch has as many workgroups as the chip holds at once and workgroup g takes the work items g,
// g + G, ... (an item = 256 columns x one strip of one frame, column tiles fastest, so the items in
// flight are neighbours in memory): the 14 KiB of tables are staged once per workgroup of the LAUNCH instead of
// once per 4 096 output pixels.  Same call, 4K -> 1440p x 8: 240 -> 258 Gpixel/s; one frame 167 -> 175.  Not used
// with TAPS_SHARED: the loop costs that variant 5 VGPRs = one wave per SIMD of occupancy (1080p -> 4K: 396 -> 352).
template <int TAPS, bool HAS_ALPHA, bool PERSISTENT>
__global__ void __launch_bounds__(kBlockThreads)
decode_nv12_scaled(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const RescaleLookup r = stage_rescale_tables<false>(lds_raw, p, 0, 0, 0);
  __syncthreads();
  BT709_SCALED_WALK(HAS_ALPHA, kOverOff, OverLookup{});
}

// BT709HIP_OPT_SCALED_OVER (alpha decoders): decode_nv12_scaled<TAPS, true, PERSISTENT> whose strips blend each word
// source-over the destination or a colour before they store it (scaled_strip's over form).  lin[256] rides behind the two tables:
// 15 KiB per workgroup.  Kernels of their own: the plain instantiations keep their code.
template <int TAPS, bool PERSISTENT, int OVER>
__global__ void __launch_bounds__(kBlockThreads)
decode_nv12_scaled_over(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const RescaleLookup r = stage_rescale_tables<false>(lds_raw, p, 0, 0, 0);
  const OverLookup ov = stage_over_lin(lds_raw, p, p.table_linear_bytes + p.table_encode_bytes);
  __syncthreads();
  BT709_SCALED_WALK(true, OVER, ov);
}
#undef BT709_SCALED_WALK

// ---------------------------------------------------------------------------
// Pass 2 ALONE: -[MetalScaleRenderContext renderScaled:...] + samplingShader
// (Renderer/MetalScaleRenderContext.m:55-105, AAPLShaders.metal:73-85) for a caller that keeps the
// reference's two passes, or whose pass 1 rendered into RGBA16Float.  Same sampling geometry,
// weights and summation order as decode_nv12_scaled (the same walk_strip), so pass 1 into a BGRA8 intermediate
// followed by this kernel equals the fused kernel bit for bit.  One lane per output column walking `rows` rows.
//   IN_RGBA16F = false: a tap is a BGRA8 word; rgb linearised through lin[256] (the sRGB8 sampler's
//                decode), alpha a plain unorm (byte * (1/255f))
//   IN_RGBA16F = true:  a tap is four halves, linear light already (v_cvt_f32_f16)
// The sum is saturated (a unorm render target clamps), rgb goes through the sRGB-encode table,
// alpha is round(255 v) in arithmetic (alpha_word_of).
// ---------------------------------------------------------------------------
template <bool IN_RGBA16F>
__global__ void __launch_bounds__(kBlockThreads)
render_scaled(const RenderParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  {  // stage: lin[256] | encode buckets.  lin[] sits at LDS address 0 (this kernel has no static LDS, so its dynamic segment
     // starts there; trapped below if that ever changes): a texel's byte then becomes its table address by ONE SDWA shift.
    const uint32_t tid = threadIdx.x, n = blockDim.x;
    u32x4 *d = reinterpret_cast<u32x4 *>(lds_raw);
    const u32x4 *e = reinterpret_cast<const u32x4 *>(p.table_encode);
    const u32x4 *l = reinterpret_cast<const u32x4 *>(p.table_lin);
    const uint32_t ne = p.table_encode_bytes / 16;
    stage_batched(d, ne + 64u, tid, n, [&](uint32_t i) { return i < 64u ? l[i] : e[i - 64u]; });  // one batch: both tables' loads in flight together
    if (lds_address(lds_raw) != 0u) __builtin_trap();
  }
  __syncthreads();
  const RescaleLookup r = unit_encode_lookup(1024u, p.encode_log_add, p.encode_log_first);  // behind lin[256]
  typedef __attribute__((address_space(3))) const float *LdsFloatPtr;
  uint32_t two = 2u;  // SDWA operands cannot be inline constants
  asm("" : "+v"(two));

  const uint32_t oy0 = blockIdx.y * p.rows, oy1 = min(oy0 + p.rows, p.out_height);
  const StripTaps vt = strip_taps(oy0, p.scale_y);  // before any lane leaves
  const uint32_t ox = blockIdx.x * blockDim.x + threadIdx.x;
  if (ox >= p.out_width) return;
  const ColumnTaps ct = column_taps(ox, p.scale_x, p.width);
  constexpr uint32_t kTexel = IN_RGBA16F ? 8u : 4u;

  // surface blockIdx.z of a batched launch (bt709hip_render_scaled_batch: evenly spaced surfaces); the intermediate as a raw
  // buffer resource (scalar row offset)
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t *>(p.in) + static_cast<int64_t>(blockIdx.z) * p.in_step, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rout =
      __builtin_amdgcn_make_buffer_rsrc(p.out + static_cast<int64_t>(blockIdx.z) * p.out_step, 0, 0x7fffffff, 0x00020000);
  struct Fetched {  // the two texels of a source row, untouched
    uint32_t w[IN_RGBA16F ? 4 : 2];
  };
  auto fetch_row = [&](int srow) {
    Fetched v;
    const int ro = srow * static_cast<int>(p.in_stride);
    if (IN_RGBA16F) {
      const u32x2 t0 = __builtin_amdgcn_raw_buffer_load_b64(rin, ct.xs[0] * kTexel, ro, 0);
      const u32x2 t1 = __builtin_amdgcn_raw_buffer_load_b64(rin, ct.xs[1] * kTexel, ro, 0);
      v.w[0] = t0.x, v.w[1] = t0.y, v.w[2] = t1.x, v.w[3] = t1.y;
    } else {
      v.w[0] = __builtin_amdgcn_raw_buffer_load_b32(rin, ct.xs[0] * kTexel, ro, 0);
      v.w[1] = __builtin_amdgcn_raw_buffer_load_b32(rin, ct.xs[1] * kTexel, ro, 0);
    }
    return v;
  };
  auto landed = [&](const Fetched &v) {
    if (IN_RGBA16F) asm volatile("" ::"v"(v.w[0]), "v"(v.w[1]), "v"(v.w[2]), "v"(v.w[3]));
    else asm volatile("" ::"v"(v.w[0]), "v"(v.w[1]));
  };
  auto convert_row = [&](const Fetched &f, int) {  // R, G, B, A of tap 0; R, G, B, A of tap 1
    RowLin<4> rl;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float *s = rl.v[t];
      if (IN_RGBA16F) {
        const uint32_t lo = f.w[2 * t], hi = f.w[2 * t + 1];
        s[0] = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(lo & 0xffffu)));
        s[1] = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(lo >> 16)));
        s[2] = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(hi & 0xffffu)));
        s[3] = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(hi >> 16)));
      } else {
        const uint32_t v = f.w[t];
        // lin[byte]: byte select and << 2 in one v_lshlrev_b32_sdwa (the encoder's form, bt709_encode.hip byte_entry)
        uint32_t ar, ag, ab;
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(ar) : "v"(two), "v"(v));
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(ag) : "v"(two), "v"(v));
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(ab) : "v"(two), "v"(v));
        s[0] = *reinterpret_cast<LdsFloatPtr>(ar);  // R: byte 2
        s[1] = *reinterpret_cast<LdsFloatPtr>(ag);  // G: byte 1
        s[2] = *reinterpret_cast<LdsFloatPtr>(ab);  // B: byte 0
        s[3] = __fmul_rn(byte_of(v, 3), kInv255);                                // byteNorm
      }
    }
    return rl;
  };
  RowCache<4> cache;
  auto output_row = [&](uint32_t oy, const RowTaps &rt, const Fetched &f0, const Fetched &f1) {
    float acc[4];
    cache.filter(ct, rt, f0, f1, convert_row, acc);
    const uint32_t R = encode_byte(r, add_sat(acc[0], 0.0f));
    const uint32_t G = encode_byte(r, add_sat(acc[1], 0.0f));
    const uint32_t B = encode_byte(r, add_sat(acc[2], 0.0f));
    const uint32_t A = alpha_word_of(acc[3]);
    __builtin_amdgcn_raw_buffer_store_b32(pack_bgra(R, G, B, A), rout, ox * 4u, oy * p.out_stride, kScaledStoreAux);
  };
  walk_strip<IN_RGBA16F ? kRenderAhead16 : kRenderAhead8, false>(vt, oy0, oy1, p.height, fetch_row, landed, output_row);
}

namespace {

// rows per strip: as many as still leave `want` workgroups in the launch (table staging is per workgroup), 1 ... max_rows
uint32_t rows_per_strip(uint32_t cols, uint32_t out_height, uint32_t frames, uint64_t want, uint32_t max_rows) {
  const uint32_t rows = static_cast<uint32_t>(static_cast<uint64_t>(cols) * out_height * frames / want);
  return rows < 1 ? 1 : (rows > max_rows ? max_rows : rows);
}

// widest tap fetch the layout allows (see the kernel); the frame spacing of a uniform batch counts too
// Planar frames (`layout` kChromaI420): in_align covers the luma and alpha planes, `chroma_align` the U pointers and the chroma pitch
// (hence v_offset, a whole number of rows, and the V plane).  TAPS_WIDE or TAPS_BYTES per lane, TAPS_ONCE by the wave.
int scaled_taps(const DecodeParams &p, uint32_t in_align, uint32_t layout, uint32_t chroma_align) {
  uint32_t align = in_align > 4 ? 4 : in_align;
  auto fold = [&align](uint64_t v) { while (align > 1 && v % align) align /= 2; };
  if (layout == kChromaI420) {
    fold(chroma_align > 4 ? 4 : chroma_align);
    if (p.uniform) fold(static_cast<uint64_t>(p.step_y)), fold(static_cast<uint64_t>(p.step_cbcr)), fold(static_cast<uint64_t>(p.step_alpha));
    // the wide form's chroma window is clamped to W/2 - 8, which is 4-aligned only when W % 8 == 0; where NV12 would load pairs
    // a plane's sample is a byte; where NV12 would fetch by the wave (TAPS_SHARED: not built for these frames) the per-lane form
    const int taps = (align == 4 && p.width % 8 == 0 && p.width >= 16) ? TAPS_WIDE : TAPS_BYTES;
    // the lane's own pixel is three byte loads: no alignment is asked of the chroma planes
    return p.scale_x <= BT709_SCALED_ONCE_BELOW && p.scale_y < BT709_SCALED_SHARED_BELOW ? TAPS_ONCE : taps;
  }
  if (p.uniform) fold(static_cast<uint64_t>(p.step_y)), fold(static_cast<uint64_t>(p.step_cbcr)), fold(static_cast<uint64_t>(p.step_alpha));
  int taps = (align == 4 && p.width % 4 == 0 && p.width >= 8) ? TAPS_WIDE : (align >= 2 ? TAPS_PAIRS : TAPS_BYTES);
  // Fetching by the wave pays when most fetched rows are not decoded (enlarging: the two loads per output
  // row dominate) and costs when they are (four ds_bpermute per decoded row on an LDS pipe the lookups
  // keep busy): 1080p -> 4K +6.6 %, 4K -> 1440p -8 % (same call).  A wave's 64 windows must fit one 256-byte span.
  if (taps == TAPS_WIDE && p.scale_y < BT709_SCALED_SHARED_BELOW && p.scale_x * 64.0f + 12.0f <= 252.0f) taps = TAPS_SHARED;
  // Enlarging horizontally: the wave decodes each source pixel once (TAPS_ONCE).  A wave's taps must lie within 64
  // source columns of lane 0's left tap: x0(lane 63) - x0(lane 0) <= floor(63 scale_x) + 1, plus one for the right tap.
  if (align >= 2 && p.scale_x <= BT709_SCALED_ONCE_BELOW && p.scale_y < BT709_SCALED_SHARED_BELOW) taps = TAPS_ONCE;
  return taps;
}

// Planar frames: the largest power of two <= 16 that divides every U pointer the launch reads and the chroma pitch -- what the shim's
// BatchInfo::chroma_align holds, worked out HERE from the block the kernel itself reads (the launcher's signature is the one its test
// doubles link against, and in_align covers the luma and alpha planes alone).  An evenly spaced batch reads frames[0] + i * step_cbcr
// (scaled_taps folds the step), any other its pointer table.
uint32_t planar_chroma_align(const DecodeParams &p, uint32_t frames) {
  uint32_t align = 16;
  auto fold = [&align](uint64_t v) { while (align > 1 && v % align) align /= 2; };
  fold(p.cbcr_stride), fold(p.v_offset);
  const uint32_t listed = p.uniform ? 1u : (frames < static_cast<uint32_t>(kMaxBatch) ? frames : static_cast<uint32_t>(kMaxBatch));
  for (uint32_t i = 0; i < listed; ++i) fold(reinterpret_cast<uintptr_t>(p.frames[i].cbcr));
  return align;
}

// The rows of this file's kernels (bt709_rescale.h ScaledKernel: {taps, alpha, curve, over, persistent, kernel, name}), stamped out
// per tap form.  The by-wave forms run one workgroup per item (dispatched by the hardware), the per-lane forms persistent
// workgroups: SCALED_KERNELS' second argument is both the template argument and the row's `persistent`.
#define SCALED_KERNELS(T, P)                                                                                                             \
  {T, 1, kAny, kOverDestination, P, decode_nv12_scaled_over<T, P, kOverDestination>, "decode_nv12_scaled<alpha,over>"},                  \
  {T, 1, kAny, kOverColour, P, decode_nv12_scaled_over<T, P, kOverColour>, "decode_nv12_scaled<alpha,over-colour>"},                     \
  {T, 1, kAny, kOverOff, P, decode_nv12_scaled<T, true, P>, "decode_nv12_scaled<alpha>"},                                                \
  {T, 0, kAny, kAny, P, decode_nv12_scaled<T, false, P>, "decode_nv12_scaled"}
const ScaledKernel kScaledKernels[] = {
    SCALED_KERNELS(TAPS_ONCE, false), SCALED_KERNELS(TAPS_SHARED, false), SCALED_KERNELS(TAPS_WIDE, true), SCALED_KERNELS(TAPS_PAIRS, true), SCALED_KERNELS(TAPS_BYTES, true),
};
#undef SCALED_KERNELS

// pass 2 alone: [the intermediate is RGBA16Float]
const struct RenderKernel {
  void (*fn)(const RenderParams);
  const char *name;
} kRenderKernels[2] = {{render_scaled<false>, "render_scaled<bgra8>"}, {render_scaled<true>, "render_scaled<rgba16f>"}};

// the row of a launch: from planar frames (`layout` kChromaI420) bt709_rescale_planar.hip's, whatever the target; else into a planar
// CHW target (`elem`) bt709_rescale_chw.hip's, through the RGBA16Float intermediate (`f16`) bt709_rescale_f16.hip's, else this file's
const ScaledKernel *scaled_kernel(uint32_t layout, uint32_t elem, bool f16, int taps, bool has_alpha, bool curve, uint32_t over) {
  const ScaledKernels nv12 = elem != kChwNone ? scaled_chw_kernels(elem) : (f16 ? scaled_f16_kernels() : ScaledKernels(kScaledKernels));
  for (const ScaledKernel &k : layout == kChromaI420 ? scaled_planar_kernels(elem) : nv12)
    if (selects(k.taps, taps) && selects(k.alpha, has_alpha) && selects(k.curve, curve) && selects(k.over, static_cast<int>(over))) return &k;
  return nullptr;  // unreachable: the rows of a tap form end in one that takes every remaining selector (planar: of the three forms scaled_taps picks)
}

// As many workgroups as the chip holds at once (what the registers and the tables' LDS allow per CU).  The answer
// depends on the kernel variant, on the dynamic LDS (the decode-side table's size follows the gamma's bucket count)
// and on the device: a small cache keyed on all three (a miss just asks
// again; a torn entry can only mis-size the grid -- the item loop strides by gridDim.x -- never change a result)
uint64_t resident_workgroups(const void *fn, size_t lds, uint32_t cus) {
  struct Occupancy {
    std::atomic<const void *> fn{nullptr};
    std::atomic<uint64_t> key{0};
    std::atomic<int> per_cu{0};
  };
  static Occupancy cache[16];
  int device = 0;
  (void)hipGetDevice(&device);
  const uint64_t key = (static_cast<uint64_t>(lds) << 16) | static_cast<uint32_t>(device & 0xffff);
  Occupancy &slot = cache[((reinterpret_cast<uintptr_t>(fn) >> 4) ^ lds ^ static_cast<uint32_t>(device)) & 15];
  int per_cu = 0;
  if (slot.fn.load(std::memory_order_acquire) == fn && slot.key.load(std::memory_order_relaxed) == key)
    per_cu = slot.per_cu.load(std::memory_order_relaxed);
  if (per_cu == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, static_cast<int>(kBlockThreads), lds) != hipSuccess || per_cu < 1)
      per_cu = 4;
    slot.fn.store(nullptr, std::memory_order_release);  // invalidate while the fields change
    slot.key.store(key, std::memory_order_relaxed);
    slot.per_cu.store(per_cu, std::memory_order_relaxed);
    slot.fn.store(fn, std::memory_order_release);
  }
  return static_cast<uint64_t>(per_cu) * cus;
}

// ONE GENERATION (round 6): the resident workgroups take the items w, w + G, ...  A launch small enough for every workgroup
// to get ONE item should be cut that way: one 4K -> 1440p frame in strips of 7 rows (the 8-per-CU rule) is 2 057 items for
// 1 280 workgroups -- two for most, one for the rest -- in strips of 12 rows 1 200 items, one each: 19.6 -> 18.8 us.  Longer
// launches keep the rule (balancing them by the same count of items per workgroup measured 4-7 % SLOWER: the workgroups do not
// march in generations; profiles/r06_ab_scaled_ahead.txt).
// The forms that are not persistent (one workgroup per item, dispatched by the hardware) have the same tail: 2 700 workgroups
// for 2 048 places are 1.3 generations.  The by-wave forms' strips stay whole trips of the fetch loop (kScaledAheadWave + 1 rows).
// -> the rows per strip that give every resident workgroup at most one item, 0 when the launch is too long for that
uint32_t one_generation_rows(uint32_t cols, uint32_t out_height, uint32_t frames, uint64_t resident, uint32_t max_rows, bool by_wave) {
  if (static_cast<uint64_t>(cols) * out_height * frames > resident * max_rows) return 0;
  const uint32_t step = by_wave ? static_cast<uint32_t>(kScaledAheadWave + 1) : 1u;
  for (uint32_t r = 4; r <= max_rows; r += step)
    if (static_cast<uint64_t>(cols) * ((out_height + r - 1) / r) * frames <= resident) return r;
  return 0;
}

}  // namespace

const char *launch_render_scaled(const RenderParams &p_in, int frames, bool in_rgba16f, uint32_t compute_units, hipStream_t stream) {
  RenderParams p = p_in;
  const uint32_t cols = (p.out_width + kBlockThreads - 1) / kBlockThreads;
  const uint32_t rows = rows_per_strip(cols, p.out_height, static_cast<uint32_t>(frames), 8ull * (compute_units ? compute_units : 256u), 16);
  p.rows = rows;
  if (!render_planes_fit(p)) return nullptr;  // row offsets are formed in 32 bits (bt709_kernels.h)
  const dim3 grid(cols, (p.out_height + rows - 1) / rows, static_cast<uint32_t>(frames));
  const size_t lds = static_cast<size_t>(p.table_encode_bytes) + 1024;
  record_scaled_launch(ScaledLaunchRecord{{grid.x, grid.y, grid.z}, {kBlockThreads, 1, 1}, 0, rows, 0, 0, 0, 0, static_cast<uint64_t>(grid.x) * grid.y * grid.z});
  const RenderKernel &k = kRenderKernels[in_rgba16f];
  hipLaunchKernelGGL(k.fn, grid, dim3(kBlockThreads), lds, stream, p);
  return k.name;
}

const char *launch_decode_scaled(const DecodeParams &p_in, int frames, bool has_alpha, uint32_t in_align,
                                 uint32_t compute_units, hipStream_t stream) {
  DecodeParams p = p_in;
  const uint32_t cus = compute_units ? compute_units : 256u, nframes = static_cast<uint32_t>(frames);
  if (!scaled_planes_fit(p, has_alpha)) return nullptr;  // row offsets are formed in 32 bits (bt709_kernels.h)
  // planar I420 frames (BT709HIP_OPT_SCALED_PLANAR; gather_batch set chroma_layout and v_offset): the kernels of
  // bt709_rescale_planar.hip, the same plan.  Neither through the RGBA16Float intermediate nor blended: the shim refuses both first.
  const uint32_t layout = p.chroma_layout;
  if (layout == kChromaI420 && (p.scale_f16 != 0 || (has_alpha && p.over_mode != kOverOff))) return nullptr;
  const int taps = scaled_taps(p, in_align, layout, layout == kChromaI420 ? planar_chroma_align(p, nframes) : 0u);
  // through the RGBA16Float intermediate (bt709_rescale_f16.hip): the same plan; every row of that file is persistent
  const bool f16 = p.scale_f16 != 0;
  // BT709HIP_OPT_SCALED_OVER: the *_over kernels (the one launched is the one whose occupancy sizes the grid), lin[256] behind their tables
  const uint32_t over = has_alpha ? p.over_mode : kOverOff;
  // a planar CHW target (BT709HIP_OPT_SCALED_CHW; gather_batch set chw_elem): the kernels of bt709_rescale_chw.hip, the same plan.
  // Their scales move to over_lin HERE, in the private copy: tiles_x and tile_rows below are the words of chw_scale[1..2]
  // (bt709_kernels.h).  Neither through the RGBA16Float intermediate nor blended: the shim refuses both before it gets here.
  const uint32_t elem = p.chw_elem;
  if (elem != kChwNone) {
    if (elem > kChwF32 || f16 || over != kOverOff) return nullptr;
    for (int c = 0; c < 3; ++c) p.over_lin[c] = p.chw_scale[c];
  }
  const ScaledKernel *k = scaled_kernel(layout, elem, f16, taps, has_alpha, p.half_table_bytes != 0, over);
  if (!k) return nullptr;
  const void *fn = reinterpret_cast<const void *>(k->fn);
  const bool by_wave = taps == TAPS_ONCE || taps == TAPS_SHARED, persistent = k->persistent;
  // variant builds: 0 = the by-wave forms of that mode get one workgroup per item (the item loop makes one trip), as the 8-bit
  // kernel's do -- and stage their 45 KiB of tables per item (profiles/LAB.md, "Round 9")
#ifndef BT709_SCALED_F16_WAVE_LOOP
#define BT709_SCALED_F16_WAVE_LOOP 1
#endif
  const bool one_trip = f16 && by_wave && !BT709_SCALED_F16_WAVE_LOOP;
  const uint32_t cols = (p.out_width + kBlockThreads - 1) / kBlockThreads;
  const uint32_t max_rows = by_wave ? BT709_SCALED_MAX_ROWS_WAVE : BT709_SCALED_MAX_ROWS;
  uint32_t rows = rows_per_strip(cols, p.out_height, nframes, static_cast<uint64_t>(BT709_SCALED_WG_PER_CU) * cus, max_rows);
  // the by-wave forms produce kScaledAheadWave + 1 rows per trip of their loop: whole trips only (a partial trip still fetches for all its rows)
  if (by_wave && rows > static_cast<uint32_t>(kScaledAheadWave + 1)) rows -= rows % static_cast<uint32_t>(kScaledAheadWave + 1);
  const size_t lds = f16 ? scaled_f16_lds(p) : static_cast<size_t>(p.table_linear_bytes) + p.table_encode_bytes;
  const dim3 block(kBlockThreads);
  const size_t lds_launch = lds + (over != kOverOff ? kOverLinBytes : 0u);
  const uint64_t resident = resident_workgroups(fn, lds_launch, cus);
  const uint32_t balanced_rows = one_generation_rows(cols, p.out_height, nframes, resident, max_rows, by_wave);
  if (balanced_rows) rows = balanced_rows;
  p.scaled_rows = rows;
  const uint32_t strips = (p.out_height + rows - 1) / rows;
  dim3 grid(cols, strips, nframes);
  const uint64_t items = static_cast<uint64_t>(cols) * strips * nframes;
  if (persistent) {
    if (items > 0x7fffffffull) return nullptr;
    p.tiles_x = cols;
    p.tile_rows = static_cast<uint32_t>(items);
    grid = dim3(static_cast<uint32_t>(items < resident || one_trip ? items : resident), 1, 1);
  }
  record_scaled_launch(ScaledLaunchRecord{{grid.x, grid.y, grid.z}, {block.x, block.y, block.z}, static_cast<uint32_t>(taps), rows, persistent ? 1u : 0u,
                                          balanced_rows ? 1u : 0u, static_cast<uint32_t>(resident), 0, items});
  void *args[] = {&p};
  (void)hipLaunchKernel(fn, grid, block, args, lds_launch, stream);  // a failure is picked up by the caller's hipGetLastError
  return k->name;
}

hipError_t prepare_scaled_kernels() {
  for (const ScaledKernels &rows : {ScaledKernels(kScaledKernels), scaled_f16_kernels(), scaled_chw_kernels(kChwU8), scaled_chw_kernels(kChwF16), scaled_chw_kernels(kChwF32),
                                    scaled_planar_kernels(kChwNone), scaled_planar_kernels(kChwU8), scaled_planar_kernels(kChwF16), scaled_planar_kernels(kChwF32)})
    for (const ScaledKernel &k : rows)
      if (const hipError_t e = raise_lds_cap(k.fn, kRepLdsBytes)) return e;
  for (const RenderKernel &k : kRenderKernels)
    if (const hipError_t e = raise_lds_cap(k.fn, kRepLdsBytes)) return e;
  return hipSuccess;
}

}  // namespace bt709
