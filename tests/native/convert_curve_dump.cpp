// Prints the per-pixel converter's curve tables (transfer_tables.h build_convert_curve; BT709HIP_CTX_OPT_ENCODE_CONVERT): one line
// per output gamma, "<gamma> <256 float bit patterns in hex>".  Stand-alone (its own main, linked with transfer_tables.cpp alone):
// tests/test_convert_cpu.py holds the bits against the oracle's compositions.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "transfer_tables.h"

int main() {
  for (int gamma = 0; gamma < bt709::kGammaCount; ++gamma) {
    float curve[256];
    if (!bt709::build_convert_curve(gamma, curve)) return 1;
    std::printf("%d", gamma);
    for (float v : curve) {
      uint32_t bits;
      std::memcpy(&bits, &v, sizeof bits);
      std::printf(" %08x", bits);
    }
    std::printf("\n");
  }
  float none[256];
  return bt709::build_convert_curve(bt709::kGammaCount, none) || bt709::build_convert_curve(-1, none) || bt709::build_convert_curve(0, nullptr) ? 2 : 0;
}
