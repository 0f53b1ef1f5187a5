// TEST INFRASTRUCTURE.  The alpha step of the paired half encoder exactly as the kernels compile it
// (metalbt709decoder_amd/csrc/bt709_half_alpha_step.h -- the SAME source text bt709_encode_half_alpha.h includes), replayed on the
// host over all 65536 half codes.  Built by tests/test_encode_half_alpha_cpu.py with plain g++ (-ffp-contract=off) and called
// through ctypes; the result is held against the definition (tests/encode_half_alpha_cases.py) and tests/golden/alpha_luma.json.
#include <cstdint>

#include "bt709_half_alpha_step.h"

// out[code] = T[quantise_exact(sat(float(half code)))]
extern "C" void half_alpha_step_all(const uint8_t T[256], uint8_t out[65536]) {
  for (uint32_t code = 0; code < 65536u; ++code) out[code] = static_cast<uint8_t>(bt709::half_alpha_luma(T, bt709::half_sat_value(static_cast<uint16_t>(code))));
}

// the host restatement of the clamped conversion, for the test that holds it against numpy's float16
extern "C" void half_sat_all(float out[65536]) {
  for (uint32_t code = 0; code < 65536u; ++code) out[code] = bt709::half_sat_value(static_cast<uint16_t>(code));
}
