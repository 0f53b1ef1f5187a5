// The RGBA16Float target's per-channel half H(x) = half(curve_to_linear(x)) as a lookup in LDS (transfer_tables.h HalfTable;
// the method: bt709_rgba16f.hip), shared by pass 1 into such a target (decode_nv12_rgba16f) and by the fused decode + rescale
// through that intermediate (bt709_rescale_f16.hip decode_nv12_scaled_f16).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bt709_device.h"

namespace bt709 {
namespace {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const float *LdsFloatPtr;

struct HalfLookup {
  float index_scale;  // HalfTable::index_scale
  uint32_t below2;    // (h_min - 1) in both halves: the saturating subtraction that indexes T
};
// LDS address of a bucket's entry = its (masked) binary16 bits + this: the ds_read_b64's immediate offset.  ABSOLUTE LDS
// addresses: the dynamic allocation is the kernel's only LDS and starts at byte 0 (no __shared__ variable in this file; a CPU
// test reads .group_segment_fixed_size = 0 from the code object's metadata).
constexpr uint32_t kCandBias = kHalfCandLds - kHalfCandFloor;
static_assert((kHalfCandFloor & 7u) == 0 && (kHalfCandLds & 15u) == 0 && kHalfCandLds - kHalfCandFloor + 0x3ff8u < 0x10000u, "candidate entries: aligned, and the offset fits the instruction");

// The table image of a launch (thresholds, then candidate entries) -> LDS: the thresholds to byte 0, the entries to
// kHalfCandLds.  Batched staging (bt709_stage.h), five loads at a time: at most 40 KiB = 2 560 sixteen-byte words, one round for
// a 512-lane workgroup, two for 256 lanes, more for the 64-lane workgroups of very narrow frames.
__device__ __forceinline__ void stage_half_tables(unsigned char *lds, const void *src, uint32_t cand_offset, uint32_t bytes) {
  const u32x4 *s = reinterpret_cast<const u32x4 *>(src);
  const uint32_t tid = threadIdx.y * blockDim.x + threadIdx.x, nthreads = blockDim.x * blockDim.y;
  const uint32_t n = bytes / 16, n_thresholds = cand_offset / 16, gap = (kHalfCandLds - cand_offset) / 16;
  stage_batched<5>(reinterpret_cast<u32x4 *>(lds), n, tid, nthreads, [&](uint32_t i) { return s[i]; },
                   [&](uint32_t i) { return i < n_thresholds ? i : i + gap; });
}

// two values -> their binary16 codes in one word (v_cvt_pk_f16_f32, round to nearest even: the same conversion as
// v_cvt_f16_f32, two at a time)
__device__ __forceinline__ uint32_t half_bits2(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
}

// float(H) of NC curve channels x[0 .. NC) followed by NR values that have no curve (alpha samples; every channel of a mode
// without a curve) -- what a sampler reads back from the RGBA16Float texel pass 1 would have stored.  The method of half_texels
// (bt709_rgba16f.hip), on as many PAIRS as the caller has: values 2i and 2i + 1 share the packed instructions (index product,
// round-toward-zero conversion, floor; the conversion to binary16 and the saturating subtraction that indexes T), the entry
// reads are issued together and waited for once, then the threshold reads.  The fma is the CANDIDATE's, except in bucket 0,
// where it is the reference's product x * low_scale rounded to binary32 first: the empty asm keeps it from fusing with the
// conversion (v_fma_mixlo_f16: one rounding instead of two).
template <int NC, int NR>
__device__ __forceinline__ void half_lights(const HalfLookup &t, const float *x, float *out) {
  constexpr int N = NC + NR, NP = (N + 1) / 2, NCP = (NC + 1) / 2;  // pairs; pairs that hold a curve channel
  float p[2 * NP];
#pragma unroll
  for (int k = 0; k < 2 * NP; ++k) p[k] = k < N ? x[k] : 0.0f;
  uint32_t w[NP];
  if constexpr (NC > 0) {
    u32x2 c[NC];
    const u16x2 floor2 = {static_cast<uint16_t>(kHalfCandFloor), static_cast<uint16_t>(kHalfCandFloor)};
#pragma unroll
    for (int i = 0; i < NCP; ++i) {
      const f32x2 u = f32x2{x[2 * i], x[2 * i + 1 < NC ? 2 * i + 1 : 2 * i]} * t.index_scale;  // binary32 products (v_pk_mul_f32)
      u16x2 hb = __builtin_bit_cast(u16x2, __builtin_amdgcn_cvt_pkrtz(u.x, u.y));
      hb = __builtin_elementwise_max(hb, floor2);
      const uint32_t pk = __builtin_bit_cast(uint32_t, hb);
      c[2 * i] = *reinterpret_cast<LdsPairPtr>((pk & 0xfff8u) + kCandBias);  // {intercept, slope}
      if (2 * i + 1 < NC) c[2 * i + 1] = *reinterpret_cast<LdsPairPtr>(((pk >> 16) & 0xfff8u) + kCandBias);
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) asm volatile("" : "+v"(c[k]));  // one wait for the batch
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      p[k] = __builtin_fmaf(x[k], __uint_as_float(c[k].y), __uint_as_float(c[k].x));
      asm("" : "+v"(p[k]));
    }
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) w[i] = half_bits2(p[2 * i], p[2 * i + 1]);
  if constexpr (NC > 0) {
    // T[h0 + 1] at LDS byte 4 * (h0 - (h_min - 1)) + 4, the subtraction saturating at 0 (half_texels has the why)
    float e[NC];
    const u16x2 below = __builtin_bit_cast(u16x2, t.below2);
#pragma unroll
    for (int i = 0; i < NCP; ++i) {
      const uint32_t d = __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, w[i]), below));
      e[2 * i] = *reinterpret_cast<LdsFloatPtr>(((d & 0xffffu) << 2) + 4u);
      if (2 * i + 1 < NC) e[2 * i + 1] = *reinterpret_cast<LdsFloatPtr>(((d >> 16) << 2) + 4u);
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) asm volatile("" : "+v"(e[k]));  // one wait for the batch
#pragma unroll
    for (int i = 0; i < NCP; ++i) {
      uint32_t step = x[2 * i] >= e[2 * i] ? 1u : 0u;
      if (2 * i + 1 < NC) step += x[2 * i + 1] >= e[2 * i + 1] ? 0x10000u : 0u;  // no carry between the halves: H <= 0x3c00
      w[i] += step;
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k)
    out[k] = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(k & 1 ? w[k / 2] >> 16 : w[k / 2] & 0xffffu)));
}

}  // namespace
}  // namespace bt709
