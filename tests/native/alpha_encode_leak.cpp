// TESTS ONLY -- the BGRA8_ALPHA encode path of the host shim on the fake HIP runtime (tests/native/fake_hip/), built with
// -fsanitize=address,undefined by tests/test_alpha_encode_cpu.py: the context's alpha luma table is built (by
// bt709hip_encoder_prepare and lazily by the first encode), used by single and batched calls with and without a CbCr plane,
// and freed with the context -- LeakSanitizer and the fake runtime's allocation count both see a table that is not.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/bt709hip_ext.h"
#include "fake_hip/fake_hip.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                                   \
    }                                                                               \
  } while (0)

int main() {
  fake_hip_reset();
  const uint64_t before = fake_hip_allocations(0);
  for (int lazy = 0; lazy < 2; ++lazy) {
    bt709hip_context *ctx = nullptr;
    CHECK(bt709hip_context_create(0, &ctx) == BT709HIP_OK);
    if (!lazy) CHECK(bt709hip_encoder_prepare(ctx, BT709HIP_GAMMA_LINEAR, BT709HIP_GAMMA_LINEAR) == BT709HIP_OK);
    const int w = 64, h = 16, n = 5;
    void *src = nullptr, *dst = nullptr;
    CHECK(bt709hip_malloc(ctx, static_cast<size_t>(n) * w * h * 4, &src) == BT709HIP_OK);
    CHECK(bt709hip_malloc(ctx, static_cast<size_t>(n) * w * h * 3 / 2, &dst) == BT709HIP_OK);
    std::vector<bt709hip_surface> ins(n);
    std::vector<bt709hip_frame> outs(n), ys(n);
    for (int i = 0; i < n; ++i) {
      std::memset(&ins[i], 0, sizeof ins[i]);
      std::memset(&outs[i], 0, sizeof outs[i]);
      ins[i].bgra = static_cast<uint8_t *>(src) + static_cast<size_t>(i) * w * h * 4;
      ins[i].stride = w * 4, ins[i].width = w, ins[i].height = h, ins[i].format = BT709HIP_FORMAT_BGRA8_ALPHA;
      uint8_t *base = static_cast<uint8_t *>(dst) + static_cast<size_t>(i) * w * h * 3 / 2;
      outs[i].y = base, outs[i].y_stride = w, outs[i].cbcr = base + w * h, outs[i].cbcr_stride = w;
      outs[i].width = w, outs[i].height = h;
      ys[i] = outs[i];
      ys[i].cbcr = nullptr, ys[i].cbcr_stride = 0;
    }
    CHECK(bt709hip_encode(ctx, &ins[0], &outs[0], BT709HIP_GAMMA_LINEAR, BT709HIP_GAMMA_LINEAR, nullptr, 1) == BT709HIP_OK);
    CHECK(bt709hip_encode_batch(ctx, n, ins.data(), outs.data(), BT709HIP_GAMMA_LINEAR, BT709HIP_GAMMA_LINEAR, nullptr, 1) == BT709HIP_OK);
    CHECK(bt709hip_encode_batch(ctx, n, ins.data(), ys.data(), BT709HIP_GAMMA_LINEAR, BT709HIP_GAMMA_LINEAR, nullptr, 1) == BT709HIP_OK);
    CHECK(bt709hip_encode(ctx, &ins[0], &outs[0], BT709HIP_GAMMA_SRGB, BT709HIP_GAMMA_SRGB, nullptr, 1) == BT709HIP_ERR_ALPHA_TRANSFER);
    CHECK(bt709hip_free(ctx, src) == BT709HIP_OK && bt709hip_free(ctx, dst) == BT709HIP_OK);
    CHECK(bt709hip_context_destroy(ctx) == BT709HIP_OK);
    CHECK(fake_hip_allocations(0) == before);
  }
  if (failures == 0) std::printf("ok: alpha encode on the fake HIP runtime, 0 failures\n");
  return failures ? 1 : 0;
}
