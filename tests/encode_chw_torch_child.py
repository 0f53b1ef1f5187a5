"""The torch route of planar CHW encoder input in a process of its own (tests/test_encode_chw_gpu.py starts it): torch is imported
BEFORE the library is loaded, as INTEGRATION.md 4 prescribes -- both then share one HIP runtime -- which a test inside the pytest
process, where other tests have loaded the library long since, cannot arrange.

    python tests/encode_chw_torch_child.py OUT.npz

A contiguous float16 NCHW tensor of 5 small images, normalised with ImageNet's constants and holding values outside the range, NaN
and infinities; each image is wrapped with CHWTexture.fromTensor without a copy and all are encoded as ONE evenly spaced batch on
torch's current stream under setEncodeCHWMeanStd.  Writes the tensor and the frames, read back, to OUT.npz (the caller holds them to
the definition and the oracle) and prints "ok".  Exit status 77: torch does not import (the one reason to skip)."""
import sys

try:
    import torch
except ImportError as exc:
    print("torch does not import: %s" % (exc,))
    sys.exit(77)

import ctypes as C  # noqa: E402
import os  # noqa: E402

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import chw_cases as cc  # noqa: E402
import encode_chw_cases as ec  # noqa: E402
import gpu_helpers as gh  # noqa: E402
import metalbt709decoder_amd as mb  # noqa: E402
from metalbt709decoder_amd import _capi  # noqa: E402

N, W, H = ec.TORCH_N, ec.TORCH_W, ec.TORCH_H


def main(out_path):
    assert torch.cuda.is_available() and torch.cuda.device_count() > 0, "torch %s sees no GPU" % torch.__version__
    torch.cuda.init()  # torch's runtime is up before the library's first call
    ctx = gh.context()
    assert ctx.setEncodeCHWMeanStd(cc.IMAGENET_MEAN, cc.IMAGENET_STD)
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            batch = torch.from_numpy(ec.torch_tensor_values()).to("cuda:%d" % ctx.device)
            assert batch.is_contiguous()
            texs = [mb.CHWTexture.fromTensor(ctx, batch[i]) for i in range(N)]
            assert texs[0].ptr == batch.data_ptr() and texs[1].ptr - texs[0].ptr == 3 * H * W * 2 and texs[0].stride == W * 2
            bufs = [mb.CVPixelBuffer(ctx, W, H) for _ in range(N)]
            stream = torch.cuda.current_stream().cuda_stream
            assert stream != 0
            assert mb.BGRAToBT709Converter.convertCHWIntoCoreVideoBuffers(texs, bufs, mb.MetalBT709GammaSRGB, mb.MetalBT709GammaApple,
                                                                          commandBuffer=mb.CommandBuffer(ctx, stream))
            name = ctx.lib.bt709hip_last_kernel_name()
            assert name in (b"encode_chw_nv12<f16>", b"encode_chw_nv12_blocks<f16>"), name
            info = _capi.LaunchInfo()
            _capi.check(ctx.lib.bt709hip_last_launch_info(C.byref(info)))
            assert info.launches == 1 and info.grid[2] == N, (tuple(info.grid), info.launches)
            held = batch.cpu().numpy()  # waits for the stream
            planes = [b.download_planes() for b in bufs]
    finally:
        ctx.setEncodeCHWNormalisation()
    np.savez(out_path, tensor=held, y=np.stack([p[0] for p in planes]), c=np.stack([p[1] for p in planes]), kernel=np.frombuffer(name, np.uint8))
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
