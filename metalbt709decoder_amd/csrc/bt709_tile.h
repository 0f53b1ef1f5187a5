// Front end of the SHORT-LIVED tile kernels (device code only): which tile of which frame a workgroup owns (banded_work:
// decode_quads, decode_nv12_rgba16f, encode_bgra) and how a lane loads its part of the tile (TileIn: decode_quads over either
// chroma layout, the WIDE branch of decode_nv12_half; decode_nv12_rgba16f follows the same rule with 2-byte units in code of its own).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bt709_kernels.h"

namespace bt709 {
namespace {

// XCD-AWARE WORK MAP (xcd_bands; launches of a multiple of 8 frames, from the launcher's threshold on: bt709_launch.h plan_bands).
// Workgroups are dealt round-robin over the 8 XCDs in dispatch order, so with the plain map (tile, row pair, frame) XCD k owns the
// tile rows = k mod 8 of ONE address stream -- and an XCD that runs a few percent ahead of another (they sit at different
// distances from the HBM stacks) widens the band of rows in flight for the whole launch: measured, the longer a launch, the slower
// (1:1 kernel, 64 / 128 / 256 frames per launch: 0.75 / 0.71 / 0.70 of the roofline against 0.77 for 32).  With the map, grid.x =
// 8 x tiles, so x & 7 IS the workgroup's position in the round-robin, and XCD-class b gets a contiguous band of the launch's frames
// [b F/8, (b + 1) F/8): eight sequential streams that cannot drift into each other.  Long launches then GAIN (no tail, no
// boundary): 256 frames per launch 0.80-0.81.  Speed only: nothing depends on which XCD a workgroup really lands on.
// Map 0: plain.  Map 1: bands.  Map 2 (INTERLEAVED kernels only -- the others take any non-zero value as map 1): frame =
// 8 z + b, the eight classes on neighbouring frames.
struct BandedWork {
  uint32_t tile, frame;
};
template <bool INTERLEAVED = false>
__device__ __forceinline__ BandedWork banded_work(uint32_t xcd_bands, uint32_t frames_per_band) {
  const uint32_t band = blockIdx.x & 7u;
  BandedWork w;
  w.tile = xcd_bands ? blockIdx.x >> 3 : blockIdx.x;
  if (INTERLEAVED) w.frame = xcd_bands == 1 ? band * frames_per_band + blockIdx.z : (xcd_bands == 2 ? blockIdx.z * 8u + band : blockIdx.z);
  else w.frame = xcd_bands ? band * frames_per_band + blockIdx.z : blockIdx.z;
  return w;
}

// Frame bytes are touched exactly once: stream them past the caches (measured +1.3 % on 4K)
template <bool NT>
__device__ __forceinline__ uint32_t load32(const uint8_t *p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p));
  return *reinterpret_cast<const uint32_t *>(p);
}
template <bool NT>
__device__ __forceinline__ uint32_t load16(const uint8_t *p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(p));
  return *reinterpret_cast<const uint16_t *>(p);
}

// What a lane holds of its tile: N quads of one row pair as loaded -- a dword of the luma top / bottom row, of the alpha top /
// bottom row each, and the quad's chroma as cw = {Cb0, Cr0, Cb1, Cr1}, the word the arithmetic takes.
// LAYOUT (DecodeParams::chroma_layout, uniform over the launch) says where cw comes from:
//   kChromaNV12: the CbCr plane's dword, as loaded;
//   kChromaI420: f.cbcr is the U plane, rows cbcr_stride apart, and V the same plane v_offset bytes on.  A quad's chroma is 2 bytes
//     of U and 2 of V: two 2-byte loads (cu, cv: one VMEM instruction per quad more than NV12), and after the pin one v_perm_b32
//     builds cw.  Alignment: U pointer, pitch and v_offset even.  BOUND: q <= quads - 1 = W/4 - 1, so a lane reads bytes [2q, 2q + 1]
//     <= W/2 - 1 of a chroma row of W/2 bytes, and rp <= row_pairs - 1 = H/2 - 1 is a row of each plane: no load leaves a row's W/2
//     bytes, in either plane, whatever the pitch.
// The layout is a parameter of this front end, which the kernels' body already takes (bt709_decode_body.h quads_body), and adds
// no inlining layer of its own.
// THE STRAIGHT-LINE RULE of these kernels: every load of the tile is issued first (load), then the table is staged, then every
// loaded word is pinned (pin), then the arithmetic runs and only the STORES are predicated.  Lanes past the row's end and row
// pairs past the frame's load a clamped (valid) quad.  Why: a divergent `if (q < quads)` around the arithmetic makes hipcc put
// s_waitcnt vmcnt(0) at the join, and an unpinned word lets it put one between the first quad's stores and the second quad's
// arithmetic -- either way each wave waits for the WRITE ACKNOWLEDGEMENT of its first stores before it touches its next quad.
// Pinned, there is one wait for all of the tile's loads, before any store is issued.
// DEST (the composite-over kernels' destination mode): the lane also holds what the OUTPUT held -- the two 16-byte words of each
// quad, loaded with the rest (the same clamp: a lane that stores nothing reads a quad it does not own and drops it) and pinned.
typedef uint32_t TileWord16 __attribute__((ext_vector_type(4)));
template <uint32_t LAYOUT, int N, bool HAS_ALPHA, bool DEST = false>
struct TileIn {
  static constexpr bool PLANAR = LAYOUT == kChromaI420;
  uint32_t ya[N], yb[N], cu[PLANAR ? N : 1], cv[PLANAR ? N : 1], cw[N], aa[N], ab[N];
  TileWord16 da[DEST ? N : 1], db[DEST ? N : 1];  // top / bottom row of the background (DEST only)

  // quad j: min(q0 + j * blockDim.x, quads - 1) of row pair min(rp, row_pairs - 1) -- consecutive lanes own consecutive quads (a
  // store instruction must fill whole lines: a lane owning ADJACENT quads measured 3x slower, tools/lab_quads_variants.hip)
  template <bool NT>
  __device__ __forceinline__ void load(const FramePlanes &f, const DecodeParams &p, uint32_t rp, uint32_t row_pairs, uint32_t q0, uint32_t quads) {
    rp = min(rp, row_pairs - 1);
    const uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    const uint8_t *y1 = y0 + p.y_stride;
    const uint8_t *cc = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;
    const uint8_t *vv = PLANAR ? cc + p.v_offset : nullptr;  // cc is the U row then
    const uint8_t *a0 = HAS_ALPHA ? f.alpha + static_cast<size_t>(2 * rp) * p.alpha_stride : nullptr;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const uint32_t q = min(q0 + j * blockDim.x, quads - 1);
      ya[j] = load32<NT>(y0 + 4 * q);
      yb[j] = load32<NT>(y1 + 4 * q);
      if constexpr (PLANAR) {
        cu[j] = load16<NT>(cc + 2 * q);
        cv[j] = load16<NT>(vv + 2 * q);
      } else {
        cw[j] = load32<NT>(cc + 4 * q);
      }
      if (HAS_ALPHA) {
        aa[j] = load32<NT>(a0 + 4 * q);
        ab[j] = load32<NT>(a0 + p.alpha_stride + 4 * q);
      }
      if (DEST) {  // touched once: non-temporal whatever NT says
        const uint8_t *o0 = f.out + static_cast<size_t>(2 * rp) * p.out_stride + 16 * static_cast<size_t>(q);
        da[DEST ? j : 0] = __builtin_nontemporal_load(reinterpret_cast<const TileWord16 *>(o0));
        db[DEST ? j : 0] = __builtin_nontemporal_load(reinterpret_cast<const TileWord16 *>(o0 + p.out_stride));
      }
    }
  }

  __device__ __forceinline__ void pin() {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if constexpr (PLANAR) asm volatile("" : "+v"(ya[j]), "+v"(yb[j]), "+v"(cu[j]), "+v"(cv[j]));
      else asm volatile("" : "+v"(ya[j]), "+v"(yb[j]), "+v"(cw[j]));
      if (HAS_ALPHA) asm volatile("" : "+v"(aa[j]), "+v"(ab[j]));
      if (DEST) asm volatile("" : "+v"(da[DEST ? j : 0]), "+v"(db[DEST ? j : 0]));
      // selector bytes, LSB first: U byte 0, V byte 0, U byte 1, V byte 1 (0-3: the second operand, 4-7: the first)
      if constexpr (PLANAR) cw[j] = __builtin_amdgcn_perm(cv[j], cu[j], 0x05010400u);
    }
  }
};

}  // namespace
}  // namespace bt709
