// TEST INFRASTRUCTURE.  Host replay of the encoder's BT709_from_linear lookup
// (metalbt709decoder_amd/csrc/bt709_split_lookup.h -- the SAME source text hipcc compiles into encode_bgra_nv12 and
// encode_bgra_nv12_blocks) over the two-resolution table the product's own builder makes (transfer_tables.cpp
// build_split_table), for EVERY float in [0, 1], against the oracle's thresholds (oracle/bt709_oracle.h
// bt709o_thresholds): byte(x) = number of thresholds <= x, which bt709o_check_thresholds(kind) == 0 makes the reference's
// BT709_from_linear for every float.  Built by tests/test_encoder.py with
//   g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC ... transfer_tables.cpp -loracle
// and called through ctypes.  Multithreaded; a kind takes seconds on 8 cores.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "bt709_split_lookup.h"
#include "transfer_tables.h"

extern "C" {
#include "bt709_oracle.h"
}

namespace {

float bits_to_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

uint32_t float_to_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

}  // namespace

extern "C" {

// Every float with bits in [lo_bits, hi_bits] (inclusive; [0, 0x3f800000] = all of [0, 1]) through the split table of
// `kind` (bt709::kGammaSRGB, kGammaLinear, kTableEncodeApple: what build_encode_tables picks).
// out[0] = floats where the lookup differs from the count of oracle thresholds <= x (must be 0)
// out[1] = bits of the first such float (~0 if none)
// out[2] = buckets in the table, out[3] = n_fine, out[4] = floats swept
// Returns 0, or -1 if the table cannot be built.
int sweep_split_table(int kind, uint32_t lo_bits, uint32_t hi_bits, int nthreads, uint64_t out[5]) {
  bt709::SplitTable st;
  if (!bt709::build_split_table(kind, &st)) return -1;
  float thr[255];
  bt709o_thresholds(kind, thr);
  const float scale = static_cast<float>(st.n_fine);                                    // EncodeParams::from_linear_scale
  const uint32_t shift = bt709::split_coarse_shift(float_to_bits(st.coarse_scale));    // as stage_encode_tables derives it
  const uint32_t offset = st.coarse_offset;
  const bt709::TransferBucket *buckets = st.buckets.data();
  const uint64_t n_buckets = st.buckets.size();

  if (nthreads < 1) nthreads = 1;
  std::atomic<uint64_t> bad{0}, first{~0ull}, outside{0};
  std::vector<std::thread> pool;
  const uint64_t lo = lo_bits, hi = static_cast<uint64_t>(hi_bits) + 1;
  const uint64_t span = (hi - lo + nthreads - 1) / nthreads;
  for (int t = 0; t < nthreads; ++t) {
    const uint64_t a = lo + span * t, b = a + span < hi ? a + span : hi;
    if (a >= b) break;
    pool.emplace_back([=, &bad, &first, &outside] {
      uint64_t mine = 0, f = ~0ull, out_of_table = 0;
      uint32_t want = 0;  // thresholds <= x: x ascends with its bits, so this only grows
      for (uint64_t u = a; u < b; ++u) {
        const float x = bits_to_float(static_cast<uint32_t>(u));
        while (want < 255 && thr[want] <= x) ++want;
        const uint32_t got = bt709::split_table_lookup(x * scale, shift, offset, [&](uint32_t q) {
          if (q >= n_buckets) {  // the kernel would read past its staged table
            ++out_of_table;
            return bt709::TransferBucket{0.0f, 0xffffu};
          }
          return buckets[q];
        });
        if (got != want) {
          ++mine;
          if (u < f) f = u;
        }
      }
      bad += mine;
      outside += out_of_table;
      uint64_t cur = first.load();
      while (f < cur && !first.compare_exchange_weak(cur, f)) {
      }
    });
  }
  for (auto &th : pool) th.join();
  out[0] = bad + outside;
  out[1] = first;
  out[2] = n_buckets;
  out[3] = st.n_fine;
  out[4] = hi - lo;
  return 0;
}

}  // extern "C"
