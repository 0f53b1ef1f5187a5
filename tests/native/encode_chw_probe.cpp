// A launch_encode that keeps the argument block it was handed and passes the call on to the fake HIP runtime's own
// (tests/native/fake_hip/fake_hip.cpp compiled with -Dlaunch_encode=fake_hip_launch_encode): tests/test_encode_chw_cpu.py reads back
// what bt709hip_encode_batch put into EncodeParams for a planar CHW call -- the element selector, the six floats, the table.
#include <cstring>

#include "bt709_kernels.h"

namespace bt709 {

const char *fake_hip_launch_encode(const EncodeParams &p, int frames, bool fast, bool xcd_bands, hipStream_t stream);

namespace {
EncodeParams g_params;
int g_frames = 0, g_fast = 0;
}  // namespace

const char *launch_encode(const EncodeParams &p, int frames, bool fast, bool xcd_bands, hipStream_t stream) {
  g_params = p;
  g_frames = frames;
  g_fast = fast ? 1 : 0;
  return fake_hip_launch_encode(p, frames, fast, xcd_bands, stream);
}

}  // namespace bt709

extern "C" {

struct encode_chw_probe_record {
  uint32_t scale_bias[6];  // bit patterns: scale R, G, B, bias R, G, B
  int32_t input_format, fast, frames, uniform;
  uint32_t width, height, bgra_stride, chroma_layout, premultiply, convert_mode;
  const void *first_bgra, *last_table_bgra;  // frames[0].bgra, frames[kMaxChwBatch - 1].bgra
  int64_t step_bgra;
  uint32_t params_bytes, table_entries;
};

void encode_chw_probe_last(encode_chw_probe_record *r) {
  const bt709::EncodeParams &p = bt709::g_params;
  std::memcpy(r->scale_bias, p.chw.scale, 12);
  std::memcpy(r->scale_bias + 3, p.chw.bias, 12);
  r->input_format = p.input_format, r->fast = bt709::g_fast, r->frames = bt709::g_frames, r->uniform = static_cast<int32_t>(p.uniform);
  r->width = p.width, r->height = p.height, r->bgra_stride = p.bgra_stride, r->chroma_layout = p.chroma_layout;
  r->premultiply = p.premultiply, r->convert_mode = p.convert_mode;
  r->first_bgra = p.frames[0].bgra, r->last_table_bgra = p.chw.frames[bt709::kMaxChwBatch - 1].bgra;
  r->step_bgra = p.step_bgra;
  r->params_bytes = sizeof(bt709::EncodeParams), r->table_entries = bt709::kMaxChwBatch;
}

}
