// TEST INFRASTRUCTURE.  The luma table of BGRA8_ALPHA input exactly as the shim builds it
// (metalbt709decoder_amd/csrc/shim_convert.cpp alpha_luma_table): the product's (Linear, Linear) per-byte table
// (transfer_tables.cpp build_encode_tables) through csrc/bt709_alpha_luma.h -- the SAME source text the shim compiles.
// Built by tests/test_alpha_encode_cpu.py with plain g++ (-ffp-contract=off) and called through ctypes; the result is held
// against tests/golden/alpha_luma.json, which the reference's own headers produced.
#include <cstdint>

#include "bt709_alpha_luma.h"
#include "transfer_tables.h"

extern "C" int alpha_luma_table(uint8_t out[256]) {
  bt709::EncodeTables host;
  if (!bt709::build_encode_tables(bt709::kGammaLinear, bt709::kGammaLinear, &host)) return -1;
  bt709::build_alpha_luma(host.per_byte, out);
  return 0;
}
