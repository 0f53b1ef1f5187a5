"""The torch route of the planar CHW views in a process of its own (tests/test_scaled_chw_gpu.py starts it): torch is imported BEFORE
the library is loaded, as INTEGRATION.md 4 prescribes -- both then share one HIP runtime -- which a test inside the pytest process,
where other tests have loaded the library long since, cannot arrange.

    python tests/scaled_chw_torch_child.py OUT.npy

A torch.empty((N, 3, OH, OW), dtype=float16) batch; each image is wrapped with CHWTexture.fromTensor without a copy and all are filled
by ONE decodeBT709ScaledBatch -- evenly spaced frames, evenly spaced views -- on torch's current stream.  Writes the tensor, read
back, to OUT.npy (the caller compares it with the definition) and prints "ok".  Exit status 77: torch does not import (the one
reason to skip); any other failure is an error."""
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
import scaled_chw_cases as sc  # noqa: E402
from metalbt709decoder_amd import _capi  # noqa: E402
from metalbt709decoder_amd.decoder import DeviceBuffer  # noqa: E402


def main(out_path):
    assert torch.cuda.is_available() and torch.cuda.device_count() > 0, "torch %s sees no GPU" % torch.__version__
    torch.cuda.init()  # torch's runtime is up before the library's first call
    n = sc.TORCH_FRAMES
    (w, h), (ow, oh), _, _ = sc.SHAPES[sc.TORCH_SHAPE]
    ctx = gh.context()
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    assert dec.setCHWMeanStd(cc.IMAGENET_MEAN, cc.IMAGENET_STD) and dec.setScaledCHW(True)
    # the frames evenly spaced in one allocation: Y then CbCr
    frame_bytes = w * h * 3 // 2
    slab = DeviceBuffer(ctx, n * frame_bytes)
    host = np.concatenate([np.concatenate([p.reshape(-1) for p in sc.planes(sc.TORCH_SHAPE, i)[:2]]) for i in range(n)])
    _capi.check(ctx.lib.bt709hip_upload(ctx.handle, slab.ptr, host.size, host.ctypes.data, host.size, host.size, 1, None))
    ctx._sync(None)
    bufs = []
    for i in range(n):
        base = slab.ptr + i * frame_bytes
        b = mb.CVPixelBuffer(ctx, w, h, y_stride=w, cbcr_stride=w, planes=(base, base + w * h))
        b.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
        b.setAttachment("TransferFunction", gh.TRANSFER_FOR_GAMMA[mb.MetalBT709GammaApple])
        bufs.append(b)
    # a stream of torch's made current: its default stream is the null handle, which the library reads as the context's own stream
    with torch.cuda.stream(torch.cuda.Stream()):
        batch = torch.empty((n, 3, oh, ow), dtype=torch.float16, device="cuda:%d" % ctx.device)
        texs = [mb.CHWTexture.fromTensor(ctx, batch[i]) for i in range(n)]
        assert texs[0].ptr == batch.data_ptr() and texs[1].ptr - texs[0].ptr == 3 * oh * ow * 2 and texs[0].stride == ow * 2
        assert (texs[0].width, texs[0].height, texs[0].planes) == (ow, oh, 3)
        stream = torch.cuda.current_stream().cuda_stream
        assert stream != 0
        assert dec.decodeBT709ScaledBatch(bufs, texs, commandBuffer=mb.CommandBuffer(ctx, stream)), dec.lastStatus
        name = ctx.lib.bt709hip_last_kernel_name()
        assert name == b"decode_nv12_scaled_chw<f16>", name
        info = _capi.ScaledLaunchInfo()
        _capi.check(ctx.lib.bt709hip_last_scaled_launch_info(C.byref(info)))
        cols, strips = -(-ow // 256), -(-oh // info.rows)
        assert info.items == cols * strips * n, (info.items, cols, strips, n)  # one launch covers every image: they are evenly spaced
        got = batch.cpu().numpy()  # waits for the stream
    np.save(out_path, got)
    slab.free()
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
