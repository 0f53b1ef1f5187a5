// A launch_decode_scaled that keeps what it was handed and passes the call on to the fake HIP runtime's own
// (tests/native/fake_hip/fake_hip.cpp compiled with -Dlaunch_decode_scaled=fake_hip_launch_decode_scaled):
// tests/test_scaled_planar_cpu.py reads back what the four rescale entry points put into DecodeParams for planar I420 frames -- the
// layout, the V plane's offset, the U planes' step -- and the alignment and alpha flag that travel beside the block.
#include "bt709_kernels.h"

namespace bt709 {

const char *fake_hip_launch_decode_scaled(const DecodeParams &p, int frames, bool has_alpha, uint32_t in_align, uint32_t compute_units, hipStream_t stream);

namespace {
DecodeParams g_params;
int g_frames = 0, g_has_alpha = 0, g_calls = 0;
uint32_t g_in_align = 0;
}  // namespace

const char *launch_decode_scaled(const DecodeParams &p, int frames, bool has_alpha, uint32_t in_align, uint32_t compute_units, hipStream_t stream) {
  g_params = p;
  g_frames = frames, g_has_alpha = has_alpha ? 1 : 0, g_in_align = in_align;
  ++g_calls;
  return fake_hip_launch_decode_scaled(p, frames, has_alpha, in_align, compute_units, stream);
}

}  // namespace bt709

extern "C" {

struct scaled_planar_probe_record {
  int32_t calls, frames, has_alpha, uniform;
  uint32_t in_align, chroma_layout, chw_elem, scale_f16, over_mode;
  uint32_t width, height, out_width, out_height, y_stride, cbcr_stride, alpha_stride;
  uint64_t v_offset;
  int64_t step_y, step_cbcr, step_alpha, step_out;
  const void *first_y, *first_cbcr, *second_cbcr;
  uint32_t params_bytes, reserved;
};

void scaled_planar_probe_last(scaled_planar_probe_record *r) {
  const bt709::DecodeParams &p = bt709::g_params;
  r->calls = bt709::g_calls, r->frames = bt709::g_frames, r->has_alpha = bt709::g_has_alpha, r->uniform = static_cast<int32_t>(p.uniform);
  r->in_align = bt709::g_in_align, r->chroma_layout = p.chroma_layout, r->chw_elem = p.chw_elem, r->scale_f16 = p.scale_f16, r->over_mode = p.over_mode;
  r->width = p.width, r->height = p.height, r->out_width = p.out_width, r->out_height = p.out_height;
  r->y_stride = p.y_stride, r->cbcr_stride = p.cbcr_stride, r->alpha_stride = p.alpha_stride;
  r->v_offset = p.v_offset;
  r->step_y = p.step_y, r->step_cbcr = p.step_cbcr, r->step_alpha = p.step_alpha, r->step_out = p.step_out;
  r->first_y = p.frames[0].y, r->first_cbcr = p.frames[0].cbcr, r->second_cbcr = p.frames[1].cbcr;
  r->params_bytes = sizeof(bt709::DecodeParams), r->reserved = 0;
}

}
