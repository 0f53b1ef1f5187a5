// Device-side building blocks shared by the any-ratio rescale kernels: decode_nv12_scaled and render_scaled
// (bt709_rescale_scaled.hip) and decode_nv12_scaled_f16 (bt709_rescale_f16.hip).  The sampling geometry (strip_taps, column_taps,
// row_taps), the row cache and the filter (RowCache), the strip walk (walk_strip) and the fused kernels' strip (scaled_strip:
// fetch, tap forms, store) and the persistent item loop of the fused kernels (BT709_SCALED_ITEM_LOOP) -- one copy of each, so the
// kernels agree bit for bit on taps, weights and summation order.
#pragma once
#include "bt709_over.h"
#include "bt709_rescale.h"
// behind the HIP runtime's header (bt709_rescale.h): its functions are __host__ __device__ __forceinline__ under hipcc
#include "bt709_chw_norm.h"

namespace bt709 {
namespace {

// the tap forms: enum TAPS_* of bt709_kernels.h

// ---- tunables: each places a number on an axis that was measured (variant builds: build.py --variant, tools/ab_scaled.sh) ----
// output rows whose source rows are fetched ahead of the row being produced (walk_strip, "HOW FAR AHEAD"): per-lane tap
// fetches (8 VGPRs per row in flight) and the two by-wave forms (4 per row)
#ifndef BT709_SCALED_AHEAD
#define BT709_SCALED_AHEAD 1
#endif
#ifndef BT709_SCALED_AHEAD_WAVE
#define BT709_SCALED_AHEAD_WAVE 3
#endif
// cache-policy bits of the output store (buffer instruction aux operand): bit 1 = nt (non-temporal) on gfx942 / gfx950, a streaming
// store (the output is written once and not read again: 1080p -> 4K +6 %, one frame per launch +13 %, profiles/r06_ab_scaled_ahead.txt)
#ifndef BT709_SCALED_STORE_AUX
#define BT709_SCALED_STORE_AUX 2
#endif
// pass 2 alone (render_scaled): rows fetched ahead from a BGRA8 (4 VGPRs per row in flight) / RGBA16Float (8) intermediate
#ifndef BT709_RENDER_AHEAD8
#define BT709_RENDER_AHEAD8 1
#endif
#ifndef BT709_RENDER_AHEAD16
#define BT709_RENDER_AHEAD16 1
#endif
// the wave fetches (TAPS_SHARED) / decodes (TAPS_ONCE) a source row when the ratios are below these (scaled_taps)
#ifndef BT709_SCALED_SHARED_BELOW
#define BT709_SCALED_SHARED_BELOW 1.0f
#endif
#ifndef BT709_SCALED_ONCE_BELOW
#define BT709_SCALED_ONCE_BELOW 0.95f  // 63 * 0.95 + 2 = 61.85: within the 64 lanes with margin for the rounding of sx
#endif
// rows per strip: as many as still leave this many workgroups per CU, up to a cap (rows_per_strip)
#ifndef BT709_SCALED_WG_PER_CU
#define BT709_SCALED_WG_PER_CU 8
#endif
#ifndef BT709_SCALED_MAX_ROWS
#define BT709_SCALED_MAX_ROWS 16
#endif
#ifndef BT709_SCALED_MAX_ROWS_WAVE
#define BT709_SCALED_MAX_ROWS_WAVE 32  // the by-wave forms fetch 3 rows ahead: a longer strip pays its prologue and drain less often
#endif
constexpr int kScaledAhead = BT709_SCALED_AHEAD, kScaledAheadWave = BT709_SCALED_AHEAD_WAVE;
constexpr int kScaledStoreAux = BT709_SCALED_STORE_AUX;
constexpr int kRenderAhead8 = BT709_RENDER_AHEAD8, kRenderAhead16 = BT709_RENDER_AHEAD16;
static_assert(BT709_SCALED_MAX_ROWS <= 64 && BT709_SCALED_MAX_ROWS_WAVE <= 64, "one lane per row of a strip works out its vertical taps");

// Vertical taps of a strip of at most 64 output rows starting at oy0: lane i holds row oy0 + i (sy = (oy + 0.5f) *
// scale_y - 0.5f, y0 = floor(sy), fy = sy - y0).  gfx950 has no scalar float unit, so one evaluation costs 8 VALU
// instructions per row whichever way it is written; done once per strip by the lanes in parallel, a row takes its
// two numbers with v_readlane_b32 -- which also puts them in SGPRs, so row offsets and the row-cache tests are scalar
// work.  MUST run while all 64 lanes of the wave are alive: v_readlane_b32 reads a lane's register whatever EXEC says,
// but a lane that left before this point never wrote it.
struct StripTaps {
  float fy;
  int yi;
};
__device__ __forceinline__ StripTaps strip_taps(uint32_t oy0, float scale_y) {
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const float sy = __fadd_rn(__fmul_rn(__fadd_rn(static_cast<float>(oy0 + lane), 0.5f), scale_y), -0.5f);
  const float y0f = __builtin_floorf(sy);
  StripTaps t;
  t.fy = __fadd_rn(sy, -y0f);
  t.yi = static_cast<int>(y0f);
  // pinned HERE: the values are pure functions of the lane id, and hipcc otherwise sinks them past the caller's
  // early return of the lanes beyond the row's end -- whose registers the other lanes read
  asm volatile("" : "+v"(t.fy), "+v"(t.yi));
  return t;
}

// horizontal taps of output column ox: source columns xs[0], xs[1] (clamped to the edge), weights gx = 1 - fx and fx
struct ColumnTaps {
  uint32_t xs[2];
  float fx, gx;
};
__device__ __forceinline__ ColumnTaps column_taps(uint32_t ox, float scale_x, uint32_t width) {
  const float sx = __fadd_rn(__fmul_rn(__fadd_rn(static_cast<float>(ox), 0.5f), scale_x), -0.5f);
  const float x0f = __builtin_floorf(sx);
  const int wmax = static_cast<int>(width) - 1, xi = static_cast<int>(x0f);
  ColumnTaps c;
  c.fx = __fadd_rn(sx, -x0f), c.gx = __fadd_rn(1.0f, -c.fx);
  c.xs[0] = static_cast<uint32_t>(min(max(xi, 0), wmax)), c.xs[1] = static_cast<uint32_t>(min(max(xi + 1, 0), wmax));
  return c;
}

// vertical taps of output row oy of the strip that starts at oy0: the same for every lane, taken from the strip's lanes (strip_taps)
struct RowTaps {
  int ys[2];
  float fy;
};
__device__ __forceinline__ RowTaps row_taps(const StripTaps &vt, uint32_t oy0, uint32_t oy, int hmax) {
  RowTaps rt;
  const int k = static_cast<int>(oy - oy0);
  rt.fy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vt.fy), k));
  const int yi = __builtin_amdgcn_readlane(vt.yi, k);
  rt.ys[0] = min(max(yi, 0), hmax);
  rt.ys[1] = min(max(yi + 1, 0), hmax);
  return rt;
}

// one source row of a lane in linear light: N channels of its two horizontal taps -- what the sampler hands the filter
template <int N>
struct RowLin {
  float v[2][N];
};

// THE ROW CACHE and the filter of both kernels.  Consecutive output rows share source rows whenever the vertical ratio is below 2
// (always when enlarging), and which rows an output row needs is the same for every lane, so the two linearised rows of the
// previous output row stay in registers and only rows not seen yet go through lin_row(fetched, srow) -> RowLin<N> (scalar
// branches): the conversion is the work that is saved, not the fetch (walk_strip).  filter(): the N values of an output row,
// acc[k] = (((w00 * top0 + w01 * top1) + w10 * bot0) + w11 * bot1), each product and sum rounded on its own.
// (A struct the kernels' own output_row uses, not a part of walk_strip: with the cache inside the walk hipcc gave the TAPS_ONCE
// kernels 2 / 4 VGPRs more for the same instructions, profiles/r07_refactor_scaled_isa.txt.)
template <int N>
struct RowCache {
  int have_top = -1, have_bot = -1;  // source rows held in `top` / `bot`
  RowLin<N> top = {}, bot = {};
  template <typename Fetched, typename LinRow>
  __device__ __forceinline__ void filter(const ColumnTaps &ct, const RowTaps &rt, const Fetched &f0, const Fetched &f1, LinRow &lin_row, float *acc) {
    if (rt.ys[0] == have_bot) top = bot;  // the previous bottom row is this row's top row
    else if (rt.ys[0] != have_top) top = lin_row(f0, rt.ys[0]);
    if (rt.ys[1] == rt.ys[0]) bot = top;  // both taps clamped onto one row
    else if (rt.ys[1] != have_bot) bot = lin_row(f1, rt.ys[1]);
    have_top = rt.ys[0];
    have_bot = rt.ys[1];
    const float fy = rt.fy, gy = __fadd_rn(1.0f, -fy);
    const float w[4] = {__fmul_rn(ct.gx, gy), __fmul_rn(ct.fx, gy), __fmul_rn(ct.gx, fy), __fmul_rn(ct.fx, fy)};
#pragma unroll
    for (int k = 0; k < N; ++k) {
      acc[k] = __fmul_rn(w[0], top.v[0][k]);
      acc[k] = __fadd_rn(acc[k], __fmul_rn(w[1], top.v[1][k]));
      acc[k] = __fadd_rn(acc[k], __fmul_rn(w[2], bot.v[0][k]));
      acc[k] = __fadd_rn(acc[k], __fmul_rn(w[3], bot.v[1][k]));
    }
  }
};

// THE STRIP WALK of both kernels: output rows [oy0, oy1) (at most 64) of one lane's column.  `vt` = the strip's vertical taps,
// worked out by ALL 64 lanes of the wave before any of them left (strip_taps).  The caller supplies
//   fetch_row(srow)             the loads of this lane for source row srow, returned untouched: nothing consumes a load inside the
//                               block that issues it, so the wait sits in front of the next row's conversion, a whole iteration later;
//   landed(fetched)             an empty asm that names the loaded registers: no instruction is emitted, only the s_waitcnt;
//   output_row(oy, rt, f0, f1)  one output row from the fetched bytes of its two source rows: RowCache::filter, encode, store.
// The FETCH is unconditional and ahead of the row being produced (a load the row does not need after all is an L2 hit; fetching
// only the new rows was measured: -22 % instructions, but the waits then covered the loads just issued); the CONVERSION is what
// is skipped.  The rows in flight sit in explicit register sets, one trip of the loop going through all of them: rotating one
// set through copies made hipcc drain vmcnt -- the row's STORE included -- at the end of every row.
// Past the strip's end the fetch repeats the last row instead of being branched around: hipcc's vmcnt accounting takes the path
// with the fewest loads in flight, so one conditional fetch turns every wait of the loop into a full drain.
// The loads of a fetched row are waited for (landed) whether or not the row gets converted: a load still in flight at a skipped
// conversion would leave its destination registers pending, and hipcc then drains vmcnt (stores included) wherever it reuses one
// of them.  For the same reason nothing stays in flight past the strip: a dangling load is a pending write to registers the
// next strip reuses, i.e. a drain in every trip of ITS loop.
// HOW FAR AHEAD (round 6).  gfx950 counts loads and stores in ONE in-order counter (vmcnt): waiting for the loads of row j also
// waits for every store issued before them.  One row ahead, the store of row j - 2 must have been acknowledged when row j starts
// -- and a wave's row takes ~1.2 us here, about what a store takes to come back from HBM under this write load: with the stores
// deleted, or the loads, the enlarging launch runs 27 % faster, with every lookup and all arithmetic deleted 9 %
// (profiles/r06_ab_scaled_parts.txt).  Fetching D rows ahead gives a store D row-times.  D + 1 register sets, D + 1 rows per trip.
// PAIR (D = 1 only): the two-set loop written out by hand -- it stops after the last row of an odd-length strip instead of
// fetching once more -- which the per-lane tap forms of the fused kernel run (scaled_strip has the measurement).
template <int D, bool PAIR, typename FetchRow, typename Landed, typename OutputRow>
__device__ __forceinline__ void walk_strip(const StripTaps &vt, uint32_t oy0, uint32_t oy1, uint32_t src_height,
                                           FetchRow &fetch_row, Landed &landed, OutputRow &output_row) {
  static_assert(!PAIR || D == 1, "the hand-written loop has two register sets");
  using Fetched = decltype(fetch_row(0));
  struct RowFetch {
    RowTaps rt;
    Fetched f0, f1;
  };
  const int hmax = static_cast<int>(src_height) - 1;
  const uint32_t last = oy1 - 1;
  auto fetch_at = [&](uint32_t oy) {
    RowFetch q;
    q.rt = row_taps(vt, oy0, oy, hmax);
    q.f0 = fetch_row(q.rt.ys[0]);
    q.f1 = fetch_row(q.rt.ys[1]);
    return q;
  };
  auto fetch_for = [&](uint32_t oy) { return fetch_at(min(oy, last)); };  // past the strip's end the last row again
  auto arrived = [&](const RowFetch &q) {
    landed(q.f0);
    landed(q.f1);
  };
  auto produce = [&](uint32_t oy, const RowFetch &q) {
    arrived(q);
    output_row(oy, q.rt, q.f0, q.f1);
  };
  if constexpr (PAIR) {
    RowFetch a = fetch_at(oy0), b;
    for (uint32_t oy = oy0; oy < oy1; oy += 2) {
      b = fetch_for(oy + 1);
      produce(oy, a);
      if (oy + 1 >= oy1) {  // uniform
        arrived(b);
        break;
      }
      a = fetch_for(oy + 2);
      produce(oy + 1, b);
    }
    arrived(a);
  } else {
    RowFetch s[D + 1];
#pragma unroll
    for (int k = 0; k < D; ++k) s[k] = fetch_for(oy0 + static_cast<uint32_t>(k));
    for (uint32_t oy = oy0; oy < oy1; oy += D + 1) {
#pragma unroll
      for (int u = 0; u <= D; ++u) {
        s[(u + D) % (D + 1)] = fetch_for(oy + static_cast<uint32_t>(u + D));
        if (oy + static_cast<uint32_t>(u) < oy1) produce(oy + static_cast<uint32_t>(u), s[u]);  // uniform
        else arrived(s[u]);
      }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) arrived(s[k]);
  }
}

// lin[256] of the blend (DecodeParams::over_table_lin, 1 KiB) into LDS at byte `at` of the dynamic segment; the caller synchronises
__device__ __forceinline__ OverLookup stage_over_lin(unsigned char *lds_raw, const DecodeParams &p, uint32_t at) {
  const u32x4 *l = reinterpret_cast<const u32x4 *>(p.over_table_lin);
  stage_batched(reinterpret_cast<u32x4 *>(lds_raw + at), kOverLinBytes / 16, threadIdx.x, blockDim.x, [&](uint32_t i) { return l[i]; });
  OverLookup ov = {};  // the encode side is the kernel's own table (TapLight::encode_unit)
  ov.lin_off = lds_address(lds_raw) + at;
  return ov;
}

// The 8-bit sRGB intermediate: a tap is decoded to its byte and linearised as the sRGB8 sampler does (one lookup, times 2^-40:
// bt709_rescale.h), an alpha tap is byteNorm of its decoded byte, the sums go to the encode table as they are (edges staged in
// the sums' domain), and a decoder without an alpha channel writes its alpha fill.
struct Srgb8Light {
  const RescaleLookup &r;
  // one source pixel (TAPS_ONCE): x = R, G, B, padding; byte 0 of `a` = its alpha sample -> N values
  template <int N>
  __device__ __forceinline__ void one(const float *x, uint32_t a, float *own) const {
    linearise3(r, x, own);
    if (N == 4) own[3] = alpha_norm_arith(byte_of(a, 0));
  }
  // the two horizontal taps of a source row: x = R, G, B of tap 0, of tap 1; bytes 0 and 1 of `a` = their alpha samples
  template <int N>
  __device__ __forceinline__ void two(const float *x, uint32_t a, RowLin<N> &rl) const {
    float lin[6];
    linearise6(r, x, lin);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int k = 0; k < 3; ++k) rl.v[t][k] = lin[3 * t + k];
      if (N == 4) rl.v[t][N - 1] = alpha_norm_arith(byte_of(a, t));
    }
  }
  __device__ __forceinline__ uint32_t encode(float sum) const { return encode_byte(r, sum); }
  // the blend's unit-range v (the over form of scaled_strip): into the sums' domain, where this table's edges are staged -- times
  // 2^-40, exact on both sides of the comparison, and the index fma's product gives v back
  __device__ __forceinline__ uint32_t encode_unit(float v) const {
    return encode_byte(r, __fmul_rn(v, __uint_as_float(static_cast<uint32_t>(127 + kLinearScaleLog2) << 23)));
  }
  __device__ __forceinline__ uint32_t opaque_word(const DecodeParams &p) const { return p.alpha_word; }
};

// Output column `ox_raw` of frame `f`, output rows [oy0, oy1) (at most 64).  `vt` = the strip's vertical taps,
// worked out by ALL 64 lanes of the wave before any of them left (strip_taps): lane i holds row oy0 + i.
//   TAPS_BYTES / TAPS_PAIRS / TAPS_WIDE: the lane fetches its own taps (see above); lanes past the
//     row's end must not call (a predicated store in their place cost 8 % in the same call).
//   TAPS_SHARED (layout as TAPS_WIDE, 64 * scale_x + 12 <= 252): the WAVE fetches a source row -- lane l
//     loads the l-th dword of the 256-byte span that starts at lane 0's window, one fully coalesced
//     access per plane (4 cache accesses per wave instruction against ~17 for per-lane 8-byte windows at
//     4-byte granularity) -- and a lane picks its windows out of its neighbours' registers with four
//     ds_bpermute_b32 when (and only when) the row is decoded.  Pays when most fetched rows are not
//     decoded, i.e. when enlarging; the launcher picks it for scale_y < 1.  All 64 lanes must call;
//     `live` masks the store.
//   TAPS_ONCE (CbCr plane 2-byte aligned, 63 * scale_x + 2 <= 63: enlarging): the WAVE decodes a source row ONCE.
//     Neighbouring output columns of an enlargement sit on the same source columns (at 2x every source pixel is a tap
//     of four lanes), and with per-lane taps every one of them runs the matrix and the three lookups again.  Here lane
//     l fetches and decodes source column wx0 + l (wx0 = lane 0's left tap; the 64 columns cover every tap of the
//     wave) -- one byte + one CbCr pair loaded, one pixel_rgb, three lookups instead of six -- and a lane takes the
//     linear values of its two taps out of its neighbours' registers with six ds_bpermute_b32 (no LDS bank conflicts,
//     no table traffic).  Same floats per source pixel whoever computes them: bit-identical output.  All 64 lanes must
//     call; `live` masks the store.
//   TapLight: what a decoded tap is when the filter sees it, and what becomes of the filter's sums -- Srgb8Light below (the 8-bit
//     sRGB intermediate of decode_nv12_scaled) or HalfLight (bt709_rescale_f16.hip: the RGBA16Float intermediate).
//   OVER (kOverDestination / kOverColour; alpha decoders: BT709HIP_OPT_SCALED_OVER): the row's word -- the BYTES the
//     plain form stores -- goes through bt709_over.h over_blend before the store, `ov` locating lin[256] in LDS.  The epilogue sees
//     bytes only, so it is the same for both intermediates; its encode is the TapLight's own table (encode_unit).  Destination
//     mode: the lane loads the word it is about to overwrite at the top of output_row (the row's conversion and filter hide the
//     latency; the wait also covers the rows fetched ahead, issued before it -- vmcnt is in order).  A by-wave lane past the row's
//     end loads the last column's word again (in bounds) and drops it with its store.
//   ELEM (kChwU8 / kChwF16 / kChwF32; bt709_rescale_chw.hip; never together with OVER): the output is a planar CHW
//     surface -- f.out the base of plane 0, p.out_stride the pitch of every plane, plane c starting c * OH * pitch behind it.  R, G, B
//     and the alpha byte are worked out exactly as for the word; in place of the word's store the lane stores, per plane, ONE element
//     (bt709_chw_norm.h of that byte) at vector offset ox * e, the plane and the row riding in the scalar offset.  Consecutive lanes
//     own consecutive columns: a wave's store instruction fills 64 e contiguous bytes of a plane's row.  The scales travel in
//     p.over_lin (launch_decode_scaled moves them there: bt709_kernels.h).  BOUNDS of a store: c < PLANES, oy < oy1 <= OH, ox < OW
//     (the caller's early return, or `live`): inside the OW e bytes of a row of a plane the surface has; the launcher holds
//     PLANES * OH * pitch under 2 GiB (scaled_planes_fit), so the 32-bit offsets do not wrap.
//   LAYOUT (kChromaI420: bt709_rescale_planar.hip; BT709HIP_OPT_SCALED_PLANAR): f.cbcr is the U plane, W/2 bytes a row at
//     pitch p.cbcr_stride, and V the same shape p.v_offset bytes behind it -- its base formed in 64 bits, a buffer resource of its own
//     (U and V together may pass 2 GiB; each alone is below it: scaled_planes_fit).  Pixel x takes U[x >> 1], V[x >> 1] of chroma row
//     srow >> 1.  Only the FRONT END differs -- the loads, what `landed` names and how the tap word {Cb0, Cr0, Cb1, Cr1} is put
//     together; from that word on this is the NV12 text.  Three tap forms (never TAPS_PAIRS or TAPS_SHARED):
//       TAPS_ONCE   the lane's own pixel: Y[own_x], U[own_x >> 1], V[own_x >> 1], three byte loads (no alignment asked of anything)
//       TAPS_BYTES  U[k0], V[k0], U[k1], V[k1] with k = xs >> 1: four byte loads, as many as NV12's TAPS_BYTES
//       TAPS_WIDE   (W % 8 == 0, W >= 16, every plane and pitch 4-byte aligned) the taps' columns are neighbours, so k1 is k0 or k0 + 1:
//                   ONE aligned 8-byte window per chroma plane, starting at min(k0 & ~3, W/2 - 8), holds both samples -- an 8-byte load
//                   at 4-byte granularity, the access the NV12 form makes; two v_perm_b32 pick the samples, a third interleaves them
//     BOUNDS of a chroma load: chroma row (srow >> 1) <= H/2 - 1, byte k <= (W - 1) >> 1 = W/2 - 1 (a window: [base, base + 8) with
//     base + 8 <= W/2): inside the W/2 bytes of a row of a plane the frame has, whatever the pitch.
template <int TAPS, bool HAS_ALPHA, int OVER = kOverOff, uint32_t ELEM = kChwNone, uint32_t LAYOUT = kChromaNV12, typename TapLight>
__device__ __forceinline__ void scaled_strip(const DecodeParams &p, const TapLight &light, const FramePlanes &f, uint32_t ox_raw, uint32_t oy0,
                                             uint32_t oy1, const StripTaps &vt, const OverLookup &ov = OverLookup{}) {
  static_assert(OVER == kOverOff || HAS_ALPHA, "there is nothing to composite without an alpha channel");
  static_assert(ELEM == kChwNone || OVER == kOverOff, "a planar CHW view is never blended");
  constexpr bool PLANAR = LAYOUT == kChromaI420;
  static_assert(!PLANAR || ((TAPS == TAPS_ONCE || TAPS == TAPS_WIDE || TAPS == TAPS_BYTES) && OVER == kOverOff), "planar frames: three tap forms, never blended");
  // TAPS_SHARED / TAPS_ONCE: every lane of the wave stays alive; one past the row's end works on the last column again and does not store
  constexpr bool BY_WAVE = TAPS == TAPS_SHARED || TAPS == TAPS_ONCE;
  constexpr int N = HAS_ALPHA ? 4 : 3;  // R, G, B and the byteNorm of the alpha tap (alpha decoders)
  const bool live = ox_raw < p.out_width;
  const uint32_t ox = BY_WAVE ? min(ox_raw, p.out_width - 1u) : ox_raw;

  const ColumnTaps ct = column_taps(ox, p.scale_x, p.width);
  const uint32_t xs[2] = {ct.xs[0], ct.xs[1]};
  const uint32_t cx[2] = {2u * (xs[0] >> 1), 2u * (xs[1] >> 1)};
  // TAPS_WIDE / TAPS_SHARED: 8-byte windows [ybase, ybase + 8) and [cbase, cbase + 8) hold both taps of a row
  const uint32_t ybase = min(xs[0] & ~3u, p.width - 8u), cbase = min(cx[0] & ~3u, p.width - 8u);
  const uint32_t ysel = ((xs[1] - ybase) << 8) | (xs[0] - ybase);  // v_perm_b32 selector: {Y0, Y1, -, -}
  const uint32_t k0 = cx[0] - cbase, k1 = cx[1] - cbase;
  const uint32_t csel = ((k1 + 1u) << 24) | (k1 << 16) | ((k0 + 1u) << 8) | k0;  // {Cb0, Cr0, Cb1, Cr1}
  // TAPS_SHARED: the wave's spans start at lane 0's windows (the windows move right with the lane);
  // ysrc / csrc = 4 * (lane that holds the first dword of this lane's window): the ds_bpermute address
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const uint32_t wybase = __builtin_amdgcn_readfirstlane(ybase), wcbase = __builtin_amdgcn_readfirstlane(cbase);
  const uint32_t yoff = min(wybase + 4u * lane, p.width - 4u), coff = min(wcbase + 4u * lane, p.width - 4u);
  const uint32_t ysrc = ybase - wybase, csrc = cbase - wcbase;
  // TAPS_ONCE: this lane's own source column (the wave's columns start at lane 0's left tap) and the ds_bpermute
  // addresses (4 * lane) of the lanes that hold its two taps
  const uint32_t wx0 = __builtin_amdgcn_readfirstlane(xs[0]);
  const uint32_t own_x = min(wx0 + lane, p.width - 1u), own_c = 2u * (own_x >> 1);
  const uint32_t tap_lane[2] = {4u * (xs[0] - wx0), 4u * (xs[1] - wx0)};
  // PLANAR: the taps' chroma columns k = xs >> 1 (<= W/2 - 1), k[1] = k[0] or k[0] + 1.  TAPS_WIDE (W % 8 == 0, W >= 16): the 8-byte
  // window [pbase, pbase + 8) of a U or V row holds both -- pbase is 4-aligned (W/2 % 4 == 0) and pbase + 8 <= W/2
  const uint32_t pk[2] = {xs[0] >> 1, xs[1] >> 1};
  const uint32_t pbase = min(pk[0] & ~3u, (p.width >> 1) - 8u);
  const uint32_t psel = ((pk[1] - pbase) << 8) | (pk[0] - pbase);  // v_perm_b32 selector: {U0, U1, -, -} of a U window, {V0, V1, -, -} of a V window

  // what the loads of one source row return
  struct Fetched1 {
    uint32_t y[2], c[4], a[2];
  };
  // Planes as raw buffer resources: a row's offset rides in the instruction's SCALAR offset operand and the
  // lane's position in its 32-bit vector offset, so no address is formed in the VALU (with 64-bit global
  // pointers hipcc kept plane + lane offset in a VGPR pair and added the row offset per load).  The launcher
  // refuses planes of 2 GiB and more.
  auto plane = [](const uint8_t *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(base), 0, 0x7fffffff, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t ry = plane(f.y), rc = plane(f.cbcr), ra = plane(HAS_ALPHA ? f.alpha : f.y), ro = plane(f.out);
  const __amdgpu_buffer_rsrc_t rv = plane(PLANAR ? f.cbcr + p.v_offset : f.cbcr);  // PLANAR: the V plane, its base a 64-bit sum
  auto fetch_row = [&](int srow) {
    Fetched1 v = {};
    const int yo = srow * static_cast<int>(p.y_stride), co = (srow >> 1) * static_cast<int>(p.cbcr_stride);
    const int ao = HAS_ALPHA ? srow * static_cast<int>(p.alpha_stride) : 0;
    if constexpr (PLANAR) {  // co: chroma row srow >> 1 <= H/2 - 1 of U and of V; every byte offset below <= W/2 - 1 (see BOUNDS above)
      if (TAPS == TAPS_ONCE) {
        v.y[0] = __builtin_amdgcn_raw_buffer_load_b8(ry, own_x, yo, 0);
        v.c[0] = __builtin_amdgcn_raw_buffer_load_b8(rc, own_x >> 1, co, 0);  // own_x <= W - 1
        v.c[1] = __builtin_amdgcn_raw_buffer_load_b8(rv, own_x >> 1, co, 0);
        if (HAS_ALPHA) v.a[0] = __builtin_amdgcn_raw_buffer_load_b8(ra, own_x, ao, 0);
      } else if (TAPS == TAPS_WIDE) {
        const u32x2 yw = __builtin_amdgcn_raw_buffer_load_b64(ry, ybase, yo, 0);
        const u32x2 uw = __builtin_amdgcn_raw_buffer_load_b64(rc, pbase, co, 0);  // [pbase, pbase + 8), pbase + 8 <= W/2
        const u32x2 vw = __builtin_amdgcn_raw_buffer_load_b64(rv, pbase, co, 0);
        v.y[0] = yw.x, v.y[1] = yw.y, v.c[0] = uw.x, v.c[1] = uw.y, v.c[2] = vw.x, v.c[3] = vw.y;
        if (HAS_ALPHA) {
          const u32x2 aw = __builtin_amdgcn_raw_buffer_load_b64(ra, ybase, ao, 0);
          v.a[0] = aw.x, v.a[1] = aw.y;
        }
      } else {
        v.y[0] = __builtin_amdgcn_raw_buffer_load_b8(ry, xs[0], yo, 0);
        v.y[1] = __builtin_amdgcn_raw_buffer_load_b8(ry, xs[1], yo, 0);
        if (HAS_ALPHA) {
          v.a[0] = __builtin_amdgcn_raw_buffer_load_b8(ra, xs[0], ao, 0);
          v.a[1] = __builtin_amdgcn_raw_buffer_load_b8(ra, xs[1], ao, 0);
        }
        v.c[0] = __builtin_amdgcn_raw_buffer_load_b8(rc, pk[0], co, 0);  // pk <= (W - 1) >> 1
        v.c[1] = __builtin_amdgcn_raw_buffer_load_b8(rv, pk[0], co, 0);
        v.c[2] = __builtin_amdgcn_raw_buffer_load_b8(rc, pk[1], co, 0);
        v.c[3] = __builtin_amdgcn_raw_buffer_load_b8(rv, pk[1], co, 0);
      }
      return v;
    }
    if (TAPS == TAPS_ONCE) {
      v.y[0] = __builtin_amdgcn_raw_buffer_load_b8(ry, own_x, yo, 0);
      v.c[0] = __builtin_amdgcn_raw_buffer_load_b16(rc, own_c, co, 0);
      if (HAS_ALPHA) v.a[0] = __builtin_amdgcn_raw_buffer_load_b8(ra, own_x, ao, 0);
    } else if (TAPS == TAPS_SHARED) {
      v.y[0] = __builtin_amdgcn_raw_buffer_load_b32(ry, yoff, yo, 0);
      v.c[0] = __builtin_amdgcn_raw_buffer_load_b32(rc, coff, co, 0);
      if (HAS_ALPHA) v.a[0] = __builtin_amdgcn_raw_buffer_load_b32(ra, yoff, ao, 0);
    } else if (TAPS == TAPS_WIDE) {
      const u32x2 yw = __builtin_amdgcn_raw_buffer_load_b64(ry, ybase, yo, 0);
      const u32x2 cw = __builtin_amdgcn_raw_buffer_load_b64(rc, cbase, co, 0);
      v.y[0] = yw.x, v.y[1] = yw.y, v.c[0] = cw.x, v.c[1] = cw.y;
      if (HAS_ALPHA) {
        const u32x2 aw = __builtin_amdgcn_raw_buffer_load_b64(ra, ybase, ao, 0);
        v.a[0] = aw.x, v.a[1] = aw.y;
      }
    } else {
      v.y[0] = __builtin_amdgcn_raw_buffer_load_b8(ry, xs[0], yo, 0);
      v.y[1] = __builtin_amdgcn_raw_buffer_load_b8(ry, xs[1], yo, 0);
      if (HAS_ALPHA) {
        v.a[0] = __builtin_amdgcn_raw_buffer_load_b8(ra, xs[0], ao, 0);
        v.a[1] = __builtin_amdgcn_raw_buffer_load_b8(ra, xs[1], ao, 0);
      }
      if (TAPS == TAPS_PAIRS) {
        v.c[0] = __builtin_amdgcn_raw_buffer_load_b16(rc, cx[0], co, 0);
        v.c[1] = __builtin_amdgcn_raw_buffer_load_b16(rc, cx[1], co, 0);
      } else {
        v.c[0] = __builtin_amdgcn_raw_buffer_load_b8(rc, cx[0], co, 0);
        v.c[1] = __builtin_amdgcn_raw_buffer_load_b8(rc, cx[0] + 1, co, 0);
        v.c[2] = __builtin_amdgcn_raw_buffer_load_b8(rc, cx[1], co, 0);
        v.c[3] = __builtin_amdgcn_raw_buffer_load_b8(rc, cx[1] + 1, co, 0);
      }
    }
    return v;
  };
  auto landed = [&](const Fetched1 &v) {
    if constexpr (PLANAR) {  // every loaded register of the row: ONCE Y, U, V; WIDE two luma dwords and the two windows; BYTES as NV12's
      if (TAPS == TAPS_ONCE) asm volatile("" ::"v"(v.y[0]), "v"(v.c[0]), "v"(v.c[1]));
      else asm volatile("" ::"v"(v.y[0]), "v"(v.y[1]), "v"(v.c[0]), "v"(v.c[1]), "v"(v.c[2]), "v"(v.c[3]));
      if (HAS_ALPHA) {
        if (TAPS == TAPS_ONCE) asm volatile("" ::"v"(v.a[0]));
        else asm volatile("" ::"v"(v.a[0]), "v"(v.a[1]));
      }
      return;
    }
    if (BY_WAVE) asm volatile("" ::"v"(v.y[0]), "v"(v.c[0]));
    else if (TAPS == TAPS_BYTES) asm volatile("" ::"v"(v.y[0]), "v"(v.y[1]), "v"(v.c[0]), "v"(v.c[1]), "v"(v.c[2]), "v"(v.c[3]));
    else asm volatile("" ::"v"(v.y[0]), "v"(v.y[1]), "v"(v.c[0]), "v"(v.c[1]));
    if (HAS_ALPHA) {
      if (BY_WAVE) asm volatile("" ::"v"(v.a[0]));
      else asm volatile("" ::"v"(v.a[0]), "v"(v.a[1]));
    }
  };
  // this lane's two taps of that row: Y0 | Y1 << 8, Cb0 | Cr0 << 8 | Cb1 << 16 | Cr1 << 24, A0 | A1 << 8
  struct TapBytes {
    uint32_t yy, cc, aa;
  };
  auto tap_bytes = [&](const Fetched1 &v) {
    TapBytes t;
    t.aa = 0;
    if (TAPS == TAPS_SHARED) {
      const int ylo = __builtin_amdgcn_ds_bpermute(static_cast<int>(ysrc), static_cast<int>(v.y[0]));
      const int yhi = __builtin_amdgcn_ds_bpermute(static_cast<int>(ysrc + 4u), static_cast<int>(v.y[0]));
      const int clo = __builtin_amdgcn_ds_bpermute(static_cast<int>(csrc), static_cast<int>(v.c[0]));
      const int chi = __builtin_amdgcn_ds_bpermute(static_cast<int>(csrc + 4u), static_cast<int>(v.c[0]));
      t.yy = __builtin_amdgcn_perm(static_cast<uint32_t>(yhi), static_cast<uint32_t>(ylo), ysel);
      t.cc = __builtin_amdgcn_perm(static_cast<uint32_t>(chi), static_cast<uint32_t>(clo), csel);
      if (HAS_ALPHA) {
        const int alo = __builtin_amdgcn_ds_bpermute(static_cast<int>(ysrc), static_cast<int>(v.a[0]));
        const int ahi = __builtin_amdgcn_ds_bpermute(static_cast<int>(ysrc + 4u), static_cast<int>(v.a[0]));
        t.aa = __builtin_amdgcn_perm(static_cast<uint32_t>(ahi), static_cast<uint32_t>(alo), ysel);
      }
    } else if (PLANAR && TAPS == TAPS_WIDE) {  // {U0, U1, -, -} and {V0, V1, -, -} out of their windows, then interleaved
      t.yy = __builtin_amdgcn_perm(v.y[1], v.y[0], ysel);
      const uint32_t uu = __builtin_amdgcn_perm(v.c[1], v.c[0], psel), vv = __builtin_amdgcn_perm(v.c[3], v.c[2], psel);
      t.cc = __builtin_amdgcn_perm(vv, uu, 0x05010400u);
      if (HAS_ALPHA) t.aa = __builtin_amdgcn_perm(v.a[1], v.a[0], ysel);
    } else if (TAPS == TAPS_WIDE) {
      t.yy = __builtin_amdgcn_perm(v.y[1], v.y[0], ysel);
      t.cc = __builtin_amdgcn_perm(v.c[1], v.c[0], csel);
      if (HAS_ALPHA) t.aa = __builtin_amdgcn_perm(v.a[1], v.a[0], ysel);
    } else {
      t.yy = v.y[0] | (v.y[1] << 8);
      if (HAS_ALPHA) t.aa = v.a[0] | (v.a[1] << 8);
      t.cc = TAPS == TAPS_PAIRS ? (v.c[0] | (v.c[1] << 16)) : (v.c[0] | (v.c[1] << 8) | (v.c[2] << 16) | (v.c[3] << 24));
    }
    return t;
  };

  // One source row of this lane: its two horizontal taps, linearised (times 2^-40).  The chroma products are kept
  // across rows the way RowCache keeps the rows: two luma rows share a CbCr row.
  int chroma_row = -1;
  Chroma ch0 = {}, ch1 = {};
  auto decode_row = [&](const Fetched1 &raw, int srow) {
    if (TAPS == TAPS_ONCE) {  // this lane's OWN source pixel, then the two taps from the lanes that hold them
      if ((srow >> 1) != chroma_row) {
        ch0 = PLANAR ? chroma_terms(byte_of(raw.c[0], 0), byte_of(raw.c[1], 0)) : chroma_terms(byte_of(raw.c[0], 0), byte_of(raw.c[0], 1));
        chroma_row = srow >> 1;
      }
      float x[4], own[4];
      pixel_rgb(byte_of(raw.y[0], 0), ch0, x[0], x[1], x[2]);
      x[3] = 0.0f;
      light.template one<N>(x, raw.a[0], own);
      RowLin<N> rl;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int k = 0; k < N; ++k)
          rl.v[t][k] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(static_cast<int>(tap_lane[t]), __builtin_bit_cast(int, own[k])));
      }
      return rl;
    }
    const TapBytes fr = tap_bytes(raw);
    if ((srow >> 1) != chroma_row) {
      ch0 = chroma_terms(byte_of(fr.cc, 0), byte_of(fr.cc, 1));
      ch1 = chroma_terms(byte_of(fr.cc, 2), byte_of(fr.cc, 3));
      chroma_row = srow >> 1;
    }
    float x[6];  // R, G, B of tap 0; R, G, B of tap 1
    pixel_rgb(byte_of(fr.yy, 0), ch0, x[0], x[1], x[2]);
    pixel_rgb(byte_of(fr.yy, 1), ch1, x[3], x[4], x[5]);
    RowLin<N> rl;
    light.template two<N>(x, fr.aa, rl);
    return rl;
  };
  RowCache<N> cache;
  // one output row from the fetched bytes of its two source rows
  auto output_row = [&](uint32_t oy, const RowTaps &rt, const Fetched1 &f0, const Fetched1 &f1) {
    uint32_t bg = 0u;  // what the output holds: read once, by the lane that writes it
    if constexpr (OVER == kOverDestination) bg = __builtin_amdgcn_raw_buffer_load_b32(ro, ox * 4u, oy * p.out_stride, kScaledStoreAux);
    float acc[N];
    cache.filter(ct, rt, f0, f1, decode_row, acc);
    const uint32_t R = light.encode(acc[0]);
    const uint32_t G = light.encode(acc[1]);
    const uint32_t B = light.encode(acc[2]);
    const uint32_t aw = HAS_ALPHA ? alpha_word_of(acc[N - 1]) : light.opaque_word(p);
    if constexpr (OVER != kOverOff) {
      if (!BY_WAVE || live)
        __builtin_amdgcn_raw_buffer_store_b32(over_blend<OVER>(ov, p.over_lin, R, G, B, aw >> 24, bg, [&](float v) { return light.encode_unit(v); }), ro,
                                              ox * 4u, oy * p.out_stride, kScaledStoreAux);
      return;
    }
    if constexpr (ELEM != kChwNone) {
      constexpr int PLANES = HAS_ALPHA ? 4 : 3;
      const uint32_t code[4] = {R, G, B, aw >> 24};
      const uint32_t plane = p.out_height * p.out_stride, row = oy * p.out_stride;  // uniform: scalar arithmetic
#pragma unroll
      for (int c = 0; c < PLANES; ++c) {
        const uint32_t so = static_cast<uint32_t>(c) * plane + row;
        if constexpr (ELEM == kChwU8) {
          if (!BY_WAVE || live) __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(code[c]), ro, ox, so, kScaledStoreAux);
        } else {
          float t = c < 3 ? chw_norm(static_cast<float>(code[c]), p.over_lin[c], p.chw_bias[c % 3]) : chw_unit(static_cast<float>(code[c]));
          asm("" : "+v"(t));  // binary32 first, then binary16 (bt709_chw.hip chw_row): the pin keeps the conversion a conversion
          if constexpr (ELEM == kChwF16) {
            if (!BY_WAVE || live) __builtin_amdgcn_raw_buffer_store_b16(chw_half_bits(t), ro, ox * 2u, so, kScaledStoreAux);
          } else {
            if (!BY_WAVE || live) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(t), ro, ox * 4u, so, kScaledStoreAux);
          }
        }
      }
      return;
    }
    if (!BY_WAVE || live)
      __builtin_amdgcn_raw_buffer_store_b32(pack_bgra(R, G, B, aw), ro, ox * 4u, oy * p.out_stride, kScaledStoreAux);
  };
  // The per-lane forms one row ahead run walk_strip's hand-written pair loop.  The generic loop at D = 1 takes 14-32 VGPRs less
  // (TAPS_WIDE 71 / 83 against 85 / 101) and measured SLOWER where it counts: one 4K -> 1440p frame per launch 19.73 against
  // 18.77 us (+5.1 %), 8 per launch 14.07 against 13.88 (+1.2 %); 8K -> 4K x 4 and 1080p -> 1366x768 x 16 -1.2 % / -1.0 %
  // (profiles/r07_refactor_scaled_ab.txt).
  constexpr int D = BY_WAVE ? kScaledAheadWave : kScaledAhead;
  walk_strip<D, D == 1 && !BY_WAVE>(vt, oy0, oy1, p.height, fetch_row, landed, output_row);
}

// The PERSISTENT ITEM LOOP of a fused kernel <TAPS, ...> with parameter block `p`, as TEXT (it has to sit in the kernel function
// itself: bt709_rescale_scaled.hip, BT709_SCALED_WALK): workgroup g takes the items g, g + G, ... of the launch, an item = 256 output
// columns x one strip of one frame, column tiles fastest (launch_decode_scaled fills tiles_x and tile_rows).  `light`: the TapLight.
// OVER is handed on as scaled_strip's template arguments behind HAS_ALPHA: bt709_rescale_chw.hip passes "kOverOff, ELEM" through it,
// bt709_rescale_planar.hip "kOverOff, ELEM, kChromaI420".
#define BT709_SCALED_ITEM_LOOP(HAS_ALPHA, OVER, light, ov)                                                                               \
  const uint32_t strips = (p.out_height + p.scaled_rows - 1) / p.scaled_rows;                                                            \
  for (uint32_t item = blockIdx.x; item < p.tile_rows; item += gridDim.x) {                                                              \
    const uint32_t tile = item % p.tiles_x, rest = item / p.tiles_x;                                                                     \
    const uint32_t strip = rest % strips, frame = rest / strips;                                                                         \
    const FramePlanes f = frame_planes(p, frame);                                                                                        \
    const uint32_t ox = tile * blockDim.x + threadIdx.x;                                                                                 \
    const uint32_t oy0 = strip * p.scaled_rows;                                                                                          \
    const StripTaps vt = strip_taps(oy0, p.scale_y); /* before any lane is masked off */                                                 \
    if (TAPS == TAPS_SHARED || TAPS == TAPS_ONCE || ox < p.out_width)                                                                    \
      scaled_strip<TAPS, HAS_ALPHA, OVER>(p, light, f, ox, oy0, min(oy0 + p.scaled_rows, p.out_height), vt, ov);                         \
  }

}  // namespace
}  // namespace bt709
