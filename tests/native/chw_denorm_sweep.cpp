// Host replay of csrc/bt709_chw_denorm.h (the float -> byte step of planar CHW encoder input): the text the device
// compiles, compiled with g++ -ffp-contract=off.  tests/test_encode_chw_cpu.py holds its output against a numpy restatement.
//   chw_denorm_sweep half  <scale> <bias>                    -> 65536 bytes on stdout: the byte of every half code
//   chw_denorm_sweep f32   <scale> <bias>   (uint32 patterns on stdin) -> one byte per pattern on stdout
//   chw_denorm_sweep value <scale> <bias>   (uint16 half codes on stdin) -> the float32 bits of chw_half_value per code
//   chw_denorm_sweep trip16 | trip32 <norm scale> <norm bias> <denorm scale> <denorm bias>
//                                                            -> 256 bytes: chw_norm of every code (through binary16 or not), then back
// scale and bias are float32 bit patterns in hex.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bt709_chw_denorm.h"
#include "bt709_chw_norm.h"

static float arg_float(const char *hex) {
  const uint32_t bits = static_cast<uint32_t>(std::strtoul(hex, nullptr, 16));
  float f;
  std::memcpy(&f, &bits, sizeof f);
  return f;
}

template <typename T>
static std::vector<T> read_stdin() {
  std::vector<T> v;
  T chunk[4096];
  size_t n;
  while ((n = std::fread(chunk, sizeof(T), 4096, stdin)) > 0) v.insert(v.end(), chunk, chunk + n);
  return v;
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const char *mode = argv[1];
  const float scale = arg_float(argv[2]), bias = arg_float(argv[3]);
  std::vector<uint8_t> out;
  if (!std::strcmp(mode, "half")) {
    for (uint32_t h = 0; h < 65536u; ++h) out.push_back(static_cast<uint8_t>(bt709::chw_denorm(bt709::chw_half_value(static_cast<uint16_t>(h)), scale, bias)));
  } else if (!std::strcmp(mode, "f32")) {
    for (uint32_t bits : read_stdin<uint32_t>()) {
      float t;
      std::memcpy(&t, &bits, sizeof t);
      out.push_back(static_cast<uint8_t>(bt709::chw_denorm(t, scale, bias)));
    }
  } else if (!std::strcmp(mode, "value")) {
    for (uint16_t h : read_stdin<uint16_t>()) {
      const float v = bt709::chw_half_value(h);
      out.resize(out.size() + 4);
      std::memcpy(out.data() + out.size() - 4, &v, 4);
    }
  } else if ((!std::strcmp(mode, "trip16") || !std::strcmp(mode, "trip32")) && argc == 6) {
    const float back_scale = arg_float(argv[4]), back_bias = arg_float(argv[5]);
    for (int code = 0; code < 256; ++code) {
      float t = bt709::chw_norm(static_cast<float>(code), scale, bias);
      if (mode[4] == '1') t = bt709::chw_half_value(bt709::chw_half_bits(t));
      out.push_back(static_cast<uint8_t>(bt709::chw_denorm(t, back_scale, back_bias)));
    }
  } else {
    return 2;
  }
  return std::fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 1;
}
