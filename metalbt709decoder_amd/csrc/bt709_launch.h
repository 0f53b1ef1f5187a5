// Host-side helpers of the kernel launchers (the .hip files only: they use dim3 and the HIP function attributes).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "bt709_kernels.h"

namespace bt709 {

// XCD-band plan of a launch (the work map: bt709_tile.h banded_work): `banded` frames go out under the map -- 0, or a multiple
// of 8 -- and `tail` frames under the plain map, back to back on the stream.  min_frames: the count from which the map pays for
// the kernel; a launch from there on takes it when its count is a multiple of 8.  A uniform batch of more than kXcdBandMinFrames
// frames takes it for ANY count: the map over the multiple of 8, the plain map over the (up to 7) frames left.  Shorter launches
// are never split (a second launch would cost more than the map returns).
struct BandPlan {
  int banded, tail;
};
inline BandPlan plan_bands(int frames, bool wanted, bool uniform, int min_frames) {
  if (wanted && uniform && frames > kXcdBandMinFrames && frames % 8 != 0) return {frames - frames % 8, frames % 8};
  if (wanted && frames >= min_frames && frames % 8 == 0) return {frames, 0};
  return {0, frames};
}
// The banded launch of a plain grid (tiles, rows, frames): 8 x tiles, rows, frames / 8; fills the kernel's two map fields.
template <typename Params>
inline dim3 band_grid(Params &p, uint32_t map, const dim3 &plain) {
  p.xcd_bands = map;
  p.frames_per_band = plain.z / 8u;
  return dim3(plain.x * 8u, plain.y, p.frames_per_band);
}

// frames[0] moved `head` frames on: the tail of a split uniform batch
inline void advance_frames(DecodeParams &p, int head) {
  FramePlanes &f = p.frames[0];
  f.y += static_cast<int64_t>(head) * p.step_y;
  f.cbcr += static_cast<int64_t>(head) * p.step_cbcr;
  if (f.alpha) f.alpha += static_cast<int64_t>(head) * p.step_alpha;
  f.out += static_cast<int64_t>(head) * p.step_out;
}
inline void advance_frames(EncodeParams &p, int head) {
  p.frames[0].bgra += static_cast<int64_t>(head) * p.step_bgra;
  p.frames[0].y += static_cast<int64_t>(head) * p.step_y;
  if (p.frames[0].cbcr) p.frames[0].cbcr += static_cast<int64_t>(head) * p.step_cbcr;  // alpha frames may have none
  if (encode_pair(p)) {  // pairs[0] begins as frames[0]: the alpha planes behind it
    p.pairs[0].alpha_y += static_cast<int64_t>(head) * p.pairs[1].spare;
    if (p.pairs[0].alpha_cbcr) p.pairs[0].alpha_cbcr += static_cast<int64_t>(head) * p.pairs[2].spare;
  }
}

// the plan of the call's FIRST launch, for bt709hip_last_launch_info
inline void record_launch(const dim3 &grid, const dim3 &block, uint32_t xcd_bands) {
  LaunchShape &shape = last_launch_shape();
  if (shape.launches++ == 0) {
    shape.grid[0] = grid.x, shape.grid[1] = grid.y, shape.grid[2] = grid.z;
    shape.block[0] = block.x, shape.block[1] = block.y, shape.block[2] = block.z;
    shape.xcd_bands = static_cast<int32_t>(xcd_bands);
  }
}

// A field of a launch table's selector (bt709_kernels.hip, bt709_encode.hip, the rescale files): a value, or kAny
constexpr int kAny = -1;
inline bool selects(int want, int have) { return want == kAny || want == have; }

// Raise the dynamic-LDS cap of the kernels (tables can exceed the 64 KiB default; gfx950 has 160 KiB per workgroup).
template <size_t N>
inline hipError_t raise_lds_cap(const void *const (&kernels)[N], uint32_t bytes) {
  for (const void *fn : kernels) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
template <typename... Params>
inline hipError_t raise_lds_cap(void (*kernel)(Params...), uint32_t bytes) {  // of one row of a launch table
  return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
}

}  // namespace bt709
