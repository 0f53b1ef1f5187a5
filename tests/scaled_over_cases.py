"""BT709HIP_OPT_SCALED_OVER: what the CPU and the GPU tests of the blended rescale share.  The definition is
the composition of two pinned halves -- the option-off view of the same call (the oracle's fused rescale in the intermediate
BT709HIP_OPT_SCALE_INTERMEDIATE selects), then over_cases.composite_over on its 8-bit words:

    composite_over(W, background, *tables(oracle))
    W = oracle.decode_nv12_scaled(GAMMA_SRGB, y, uv, OW, OH, alpha=a)                               (BGRA8_SRGB intermediate)
    W = oracle.render_scaled(oracle.decode_nv12_rgba16f(GAMMA_SRGB, y, uv, a), OW, OH)              (RGBA16F intermediate)"""
import numpy as np

import over_cases as oc
import rescale_arith_cases as rc
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_SRGB

OPT = _capi.OPT_SCALED_OVER
DEST = _capi.OVER_DESTINATION
COLOUR = 0x3C7FB2
F16, SRGB8 = _capi.FORMAT_RGBA16F, _capi.FORMAT_BGRA8_SRGB
MODES = ["destination", "colour"]
INTERMEDIATES = [("bgra8", SRGB8), ("rgba16f", F16)]


def kernel_name(intermediate, destination):
    base = b"decode_nv12_scaled_f16" if intermediate == F16 else b"decode_nv12_scaled"
    return base + (b"<alpha,over>" if destination else b"<alpha,over-colour>")


def plain_name(intermediate):
    return b"decode_nv12_scaled_f16<alpha>" if intermediate == F16 else b"decode_nv12_scaled<alpha>"


def option_off_view(oracle, planes, ow, oh, intermediate):
    """W: the words the same call writes with the option off, (oh, ow, 4) B, G, R, A."""
    y, uv, a = (np.ascontiguousarray(p) for p in planes)
    if intermediate == F16:
        view = oracle.render_scaled(oracle.decode_nv12_rgba16f(GAMMA_SRGB, y, uv, a), ow, oh)
    else:
        view = oracle.decode_nv12_scaled(GAMMA_SRGB, y, uv, ow, oh, alpha=a)
    return view.reshape(oh, ow, 4)


def want_over(oracle, tabs, planes, ow, oh, intermediate, background):
    """The expected words, (oh, ow, 4); background: (oh, ow, 4) bytes, or a colour R<<16 | G<<8 | B."""
    return oc.composite_over(option_off_view(oracle, planes, ow, oh, intermediate), background, *tabs)


def assert_the_blend_shows(view, want, label):
    """The bar of the tap-form cases, on the oracle's arrays: a test must not pass because the blend did nothing.  At least
    half the pixels' words differ from the option-off view, and at least a quarter differ in a colour byte."""
    pixels = view.shape[0] * view.shape[1]
    words = int((view != want).any(axis=2).sum())
    colours = int((view[..., :3] != want[..., :3]).any(axis=2).sum())
    print("%s: %d of %d words differ from the option-off view, %d in a colour byte" % (label, words, pixels, colours))
    assert 2 * words >= pixels, (label, words, pixels)
    assert 4 * colours >= pixels, (label, colours, pixels)


def canvas(ow, oh, i):
    """What the target of frame i holds before the call: random words, random A_d included, another for every frame."""
    return np.random.default_rng(7000 + i).integers(0, 256, (oh, ow, 4), dtype=np.uint8)


def over_batch_class():
    """test_scaled_f16_gpu._Batch -- the frames of one of its SHAPES in that shape's layout, padded views between guard bands
    in a slab pre-filled with a canary -- with canvases: fill() puts a background into every view.  (A function: the module it
    comes from needs a GPU context only when a batch is made, but it is a test module and is imported where it is used.)"""
    import test_scaled_f16_gpu as f16t

    class OverBatch(f16t._Batch):
        def fill(self, canvases):
            slab = self.slab_out
            host = np.full(slab.nbytes, rc.FILL, np.uint8)
            for i, bg in enumerate(canvases or []):
                o = slab.offsets[i]
                host[o:o + self.stride * self.oh].reshape(self.oh, self.stride)[:, :4 * self.ow] = np.asarray(bg, np.uint8).reshape(self.oh, 4 * self.ow)
            _capi.check(self.ctx.lib.bt709hip_upload(self.ctx.handle, slab.buf.ptr, host.size, host.ctypes.data, host.size, host.size, 1, None), "upload")
            self.ctx._sync(None)

    return OverBatch
