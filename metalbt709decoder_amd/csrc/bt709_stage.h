// LDS staging helper shared by every kernel file (device code only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bt709 {

// LDS staging of n elements, d[dst_of(i)] = src_of(i): a lane issues up to kBatch of its loads before its first write.  Written as
// `for (i = tid; i < n; i += nthreads) d[i] = s[i]` hipcc makes every round load -> wait -> ds_write, i.e. one L2 round
// trip per round inside the workgroup's lifetime (SQ_WAIT_INST_LDS 442 M against 33 M cycles per launch for the LINEAR mode's
// 33 KiB table against the 4 KiB one, +28 % wave cycles; round 3).  kBatch: 5 covers the 1:1 kernels' large tables (33 KiB,
// 40 KiB) in one round for a 512-lane workgroup.
template <int kBatch = 4, typename T, typename SrcOf, typename DstOf>
__device__ __forceinline__ void stage_batched(T *d, uint32_t n, uint32_t tid, uint32_t nthreads, SrcOf src_of, DstOf dst_of) {
  for (uint32_t base = tid; base < n; base += nthreads * kBatch) {
    T v[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      const uint32_t i = base + static_cast<uint32_t>(k) * nthreads;
      if (i < n) v[k] = src_of(i);
    }
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      const uint32_t i = base + static_cast<uint32_t>(k) * nthreads;
      if (i < n) d[dst_of(i)] = v[k];
    }
  }
}

template <int kBatch = 4, typename T, typename SrcOf>
__device__ __forceinline__ void stage_batched(T *d, uint32_t n, uint32_t tid, uint32_t nthreads, SrcOf src_of) {
  stage_batched<kBatch>(d, n, tid, nthreads, src_of, [](uint32_t i) { return i; });
}

}  // namespace bt709
