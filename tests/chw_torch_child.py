"""The torch route of the planar CHW targets in a process of its own (tests/test_chw_gpu.py starts it): torch is imported BEFORE the
library is loaded, as INTEGRATION.md 4 prescribes -- both then share one HIP runtime -- which a test inside the pytest process,
where other tests have loaded the library long since, cannot arrange.

    python tests/chw_torch_child.py OUT.npy

A float16 NCHW tensor of 40 tiny frames; each image is wrapped with CHWTexture.fromTensor without a copy and all are decoded as ONE
evenly spaced batch on torch's current stream.  Writes the tensor, read back, to OUT.npy (the caller compares it with the
definition) and prints "ok".  Exit status 77: torch does not import (the one reason to skip); any other failure is an error."""
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
import gpu_helpers as gh  # noqa: E402
import metalbt709decoder_amd as mb  # noqa: E402
from metalbt709decoder_amd import _capi  # noqa: E402
from metalbt709decoder_amd.decoder import DeviceBuffer  # noqa: E402

N, W, H = 40, 16, 4  # tests/test_chw_gpu.py builds the same frames from the same seeds


def frames():
    return [gh.random_nv12(W, H, seed=500 + i) for i in range(N)]


def refused(make):
    try:
        make()
    except ValueError:
        return True
    return False


def main(out_path):
    assert torch.cuda.is_available() and torch.cuda.device_count() > 0, "torch %s sees no GPU" % torch.__version__
    torch.cuda.init()  # torch's runtime is up before the library's first call
    ctx = gh.context()
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    assert dec.setCHWMeanStd(cc.IMAGENET_MEAN, cc.IMAGENET_STD)
    # the frames evenly spaced in one allocation: Y then CbCr, 96 bytes each
    slab = DeviceBuffer(ctx, N * W * H * 3 // 2)
    host = np.concatenate([np.concatenate([y.reshape(-1), c.reshape(-1)]) for y, c in frames()])
    _capi.check(ctx.lib.bt709hip_upload(ctx.handle, slab.ptr, host.size, host.ctypes.data, host.size, host.size, 1, None))
    ctx._sync(None)
    bufs = []
    for i in range(N):
        base = slab.ptr + i * W * H * 3 // 2
        b = mb.CVPixelBuffer(ctx, W, H, y_stride=W, cbcr_stride=W, planes=(base, base + W * H))
        b.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
        b.setAttachment("TransferFunction", gh.TRANSFER_FOR_GAMMA[mb.MetalBT709GammaApple])
        bufs.append(b)
    # a stream of torch's made current: its default stream is the null handle, which the library reads as the context's own stream
    with torch.cuda.stream(torch.cuda.Stream()):
        batch = torch.full((N, 3, H, W), -1.0, dtype=torch.float16, device="cuda:%d" % ctx.device)
        texs = [mb.CHWTexture.fromTensor(ctx, batch[i]) for i in range(N)]
        assert texs[0].ptr == batch.data_ptr() and texs[1].ptr - texs[0].ptr == 3 * H * W * 2 and texs[0].stride == W * 2
        assert refused(lambda: mb.CHWTexture.fromTensor(ctx, batch[0].permute(0, 2, 1)))  # W is not dense
        assert refused(lambda: mb.CHWTexture.fromTensor(ctx, batch[0].to(torch.float64)))
        assert refused(lambda: mb.CHWTexture.fromTensor(ctx, batch[0].cpu()))
        stream = torch.cuda.current_stream().cuda_stream
        assert stream != 0
        assert dec.decodeBT709Batch(bufs, texs, commandBuffer=mb.CommandBuffer(ctx, stream)), dec.lastStatus
        name = ctx.lib.bt709hip_last_kernel_name()
        assert name == b"decode_nv12_quads_chw<f16,nt>", name
        info = _capi.LaunchInfo()
        _capi.check(ctx.lib.bt709hip_last_launch_info(C.byref(info)))
        assert (tuple(info.grid), info.launches) == ((1, 1, N), 1), (tuple(info.grid), info.launches)  # one launch: the images are evenly spaced
        got = batch.cpu().numpy()  # waits for the stream
    np.save(out_path, got)
    slab.free()
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
