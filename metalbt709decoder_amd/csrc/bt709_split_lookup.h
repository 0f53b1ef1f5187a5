// Lookup in the two-resolution bucket table (transfer_tables.h SplitTable) -- the encoder's BT709_from_linear
// (Renderer/BT709.h:1150-1167) -- written ONCE for the device and for the host, as bt709_quantise.h is: hipcc compiles
// this text into encode_bgra / encode_bgra_blocks, and tests/native/split_table_sweep.cpp compiles the same
// text with g++ to replay it over EVERY float in [0, 1] against the oracle's thresholds.
//
//   xs   = x * n_fine                          (n_fine a power of two: exact; the kernel folds the 2x2 average's / 4 in)
//   q    = min((uint)xs, ((uint)xs >> coarse_shift) + coarse_offset)
//   byte = bucket[q].base + (xs >= bucket[q].edge)                  edges are stored times n_fine
//
// The table is read through `read(q)` (-> TransferBucket), so that the kernel's LDS address-space load stays in the
// kernel and the host replay reads a plain array.
#pragma once

#include <cstdint>

#include "transfer_tables.h"

#ifndef BT709_HD
#if defined(__HIPCC__)
#define BT709_HD __host__ __device__ __forceinline__
#else
#define BT709_HD inline
#endif
#endif

namespace bt709 {

// log2(1 / coarse_scale) from the float's exponent field; coarse_scale = 2^-k, k >= 0
BT709_HD uint32_t split_coarse_shift(uint32_t coarse_scale_bits) { return 127u - (coarse_scale_bits >> 23); }

// unsigned minimum: HIP's own min() under hipcc (one v_min_u32), the plain comparison elsewhere
BT709_HD uint32_t split_min(uint32_t a, uint32_t b) {
#if defined(__HIPCC__)
  return min(a, b);
#else
  return a < b ? a : b;
#endif
}

template <class ReadBucket>
BT709_HD uint32_t split_table_lookup(float xs, uint32_t coarse_shift, uint32_t coarse_offset, ReadBucket read) {
  // fine index below the split, coarse above; the two index functions cross at the split and the
  // fine one grows faster, so the smaller is the right one
  const uint32_t qf = static_cast<uint32_t>(xs);
  const TransferBucket e = read(split_min(qf, (qf >> coarse_shift) + coarse_offset));
  return e.base + (xs >= e.edge ? 1u : 0u);
}

}  // namespace bt709
