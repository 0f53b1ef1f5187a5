// Host replay of the product's CHW normalisation: csrc/bt709_chw_norm.h, the text hipcc compiles into the kernels
// of csrc/bt709_chw.hip, compiled here by g++ and run over every byte code under the (scale, bias) pairs given on the command line
// as float32 bit patterns (hex).  The caller (tests/test_chw_cpu.py) holds the definition, in numpy, and compares.
//
//   chw_norm_sweep unit                      256 lines "code f32bits f16bits": the alpha plane's value of every code
//   chw_norm_sweep SCALE BIAS [SCALE BIAS]...   per pair 256 lines "pair code f32bits f16bits"
//   chw_norm_sweep half BITS...              per float32 bit pattern one line "f32bits f16bits": the conversion alone
//   chw_norm_sweep valid BITS...             per bit pattern one line "bits 0|1": what the option setters accept
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bt709_chw_norm.h"

namespace {
uint32_t bits_of(float f) {
  uint32_t b;
  std::memcpy(&b, &f, sizeof b);
  return b;
}
float float_of(uint32_t b) {
  float f;
  std::memcpy(&f, &b, sizeof f);
  return f;
}
uint32_t parse(const char *s) { return static_cast<uint32_t>(std::strtoul(s, nullptr, 16)); }
}  // namespace

int main(int argc, char **argv) {
  if (argc >= 2 && std::strcmp(argv[1], "unit") == 0) {
    for (uint32_t code = 0; code < 256; ++code) {
      const float v = bt709::chw_unit(static_cast<float>(code));
      std::printf("%u %08x %04x\n", code, bits_of(v), bt709::chw_half_bits(v));
    }
    return 0;
  }
  if (argc >= 2 && std::strcmp(argv[1], "half") == 0) {
    for (int i = 2; i < argc; ++i) std::printf("%08x %04x\n", parse(argv[i]), bt709::chw_half_bits(float_of(parse(argv[i]))));
    return 0;
  }
  if (argc >= 2 && std::strcmp(argv[1], "valid") == 0) {
    for (int i = 2; i < argc; ++i) std::printf("%08x %d\n", parse(argv[i]), bt709::chw_norm_bits_valid(parse(argv[i])) ? 1 : 0);
    return 0;
  }
  if (argc < 3 || (argc - 1) % 2 != 0) return 2;
  for (int pair = 0; 2 * pair + 2 < argc; ++pair) {
    const float scale = float_of(parse(argv[2 * pair + 1])), bias = float_of(parse(argv[2 * pair + 2]));
    for (uint32_t code = 0; code < 256; ++code) {
      const float t = bt709::chw_norm(static_cast<float>(code), scale, bias);
      std::printf("%d %u %08x %04x\n", pair, code, bits_of(t), bt709::chw_half_bits(t));
    }
  }
  return 0;
}
