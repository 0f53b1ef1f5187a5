"""The planar CHW decode targets (BT709HIP_FORMAT_CHW_U8 / _F16 / _F32) in numpy, shared by tests/test_chw_cpu.py
and tests/test_chw_gpu.py:

  * chw_of: the definition -- planes R, G, B (and A) of the bytes of BGRA words, or of float32(byte) * float32(1/255) * scale +
    bias with every operation rounded to float32 on its own, then float16 by round to nearest even;
  * the (scale, bias) list the host replay (tests/native/chw_norm_sweep.cpp) and the GPU tests share, and the search for a code
    on which a fused multiply-add would differ;
  * ChwJob: variant_cases.Job's input slabs with planar targets in a canary-filled slab of their own -- collect() hands back the
    planes and asserts that every other byte of the slab is what it was: the row padding inside and between planes, the gaps
    between surfaces, the guard bands and, for an opaque decoder, the place where a fourth plane would lie."""
import ctypes as C

import numpy as np

from metalbt709decoder_amd import _capi
from metalbt709decoder_amd._capi import Surface

FORMATS = {"uint8": _capi.FORMAT_CHW_U8, "float16": _capi.FORMAT_CHW_F16, "float32": _capi.FORMAT_CHW_F32}
ELEM_NAMES = {"uint8": "u8", "float16": "f16", "float32": "f32"}
INV255 = np.float32(1.0) / np.float32(255.0)

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def mean_std(mean, std):
    """MetalBT709Decoder.setCHWMeanStd's recipe: scale = float32(1) / float32(std), bias = float32(-mean) / float32(std)."""
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    return tuple(np.float32(1.0) / std), tuple(-mean / std)


IMAGENET = mean_std(IMAGENET_MEAN, IMAGENET_STD)


def bits(x):
    """The int an option of the C ABI takes for the float32 x."""
    return int(np.array([x], np.float32).view(np.int32)[0])


def norm(code, scale, bias):
    """One colour plane's float32 values for an array of byte codes: three float32 operations, one rounding each."""
    v = np.asarray(code).astype(np.float32) * INV255
    t = v * np.float32(scale)
    return t + np.float32(bias)


def chw_of(bgra_words, dtype, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0), planes=3):
    """(H, W) words (A<<24)|(R<<16)|(G<<8)|B -> (planes, H, W) of `dtype`: planes R, G, B and, with planes = 4, A."""
    words = np.asarray(bgra_words, np.uint32)
    dtype = np.dtype(dtype)
    out = np.empty((planes,) + words.shape, dtype)
    for c in range(planes):
        code = (words >> np.uint32(24 if c == 3 else 16 - 8 * c)) & np.uint32(0xFF)
        if dtype == np.uint8:
            out[c] = code
            continue
        t = norm(code, scale[c], bias[c]) if c < 3 else code.astype(np.float32) * INV255
        with np.errstate(over="ignore"):  # float16 overflow is +-inf, as IEEE 754 says
            out[c] = t.astype(dtype)
    return out


def words_of(bgra_bytes):
    """(H, W, 4) or (H, 4 W) bytes B, G, R, A -> (H, W) words."""
    b = np.ascontiguousarray(bgra_bytes, np.uint8)
    return b.reshape(b.shape[0], -1).view(np.uint32)


def round_to_float32(x):
    """A rational (fractions.Fraction) -> the nearest float32, ties to even: the ONE rounding a fused multiply-add makes."""
    from fractions import Fraction
    near = np.float32(float(x))  # within a float32 step of x (float() rounds correctly to float64, then once more)
    best = None
    for cand in (np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - x)
        even = (int(np.array([cand], np.float32).view(np.uint32)[0]) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    return best[1]


def fma_differs(scale, bias):
    """Codes 0..255 for which float32(fma(v, scale, bias)) != float32(float32(v * scale) + bias), v = float32(code) * float32(1/255).
    The fused form is computed EXACTLY -- the product and the sum as rationals, then one rounding to float32, ties to even -- so no
    double rounding can claim a difference a real fused multiply-add would not produce."""
    from fractions import Fraction
    code = np.arange(256)
    v = code.astype(np.float32) * INV255
    separate = (v * np.float32(scale)) + np.float32(bias)
    s, b = Fraction(float(np.float32(scale))), Fraction(float(np.float32(bias)))
    fused = np.array([round_to_float32(Fraction(float(x)) * s + b) for x in v], np.float32)
    return code[fused != separate]  # by value: a rational has no signed zero, and an exact zero is one in both forms


# The (scale, bias) pairs of the host replay and of the GPU normalisation test: the identity; ImageNet's three channels (on some
# code of each a fused multiply-add gives another float32: the tests assert it); binary16 subnormals (2^-16); +inf in binary16 but
# not in binary32 (2^17); a negative scale; a -0 bias; the ends of the accepted domain.
NORM_PAIRS = [(1.0, 0.0)] + [(float(IMAGENET[0][c]), float(IMAGENET[1][c])) for c in range(3)] + \
    [(2.0 ** -16, 0.0), (2.0 ** 17, 0.0), (-3.5, 0.25), (1.0, -0.0), (-0.0, -0.0), (2.0 ** 64, -2.0 ** 64), (2.0 ** -64, 2.0 ** -64), (0.1, 0.7)]


def pairs_in_threes():
    """NORM_PAIRS as (scale_rgb, bias_rgb) settings of a decoder, three pairs at a time (the last one padded with the identity)."""
    pairs = NORM_PAIRS + [(1.0, 0.0)] * (-len(NORM_PAIRS) % 3)
    return [(tuple(p[0] for p in pairs[i:i + 3]), tuple(p[1] for p in pairs[i:i + 3])) for i in range(0, len(pairs), 3)]


def interleave_to_planar(uv):
    """(H/2, W) CbCr rows -> U, V planes (H/2, W/2)."""
    return np.ascontiguousarray(uv[:, 0::2]), np.ascontiguousarray(uv[:, 1::2])


class ChwJob:
    """`n` frames (variant_cases.Job's input slab: planes [(y, cbcr, alpha)]) and `n` planar targets of `dtype` in a canary slab.
    A target is ALWAYS given room for four planes, so an opaque decoder's missing fourth plane is slab the check covers.
    row_pad: bytes added to width * e; out_offset: bytes added to every plane-0 pointer; spacing "table": a gap before the last
    slot; step_pad: (input, output) bytes added to the slot distance; reverse: the surfaces run backwards through the slab (an
    evenly spaced batch with a negative step); chroma_pad: None = NV12, else the frames are planar I420 with a chroma pitch of
    W/2 + chroma_pad."""

    def __init__(self, rig, planes, dtype, pads=(0, 0, 0), row_pad=0, out_offset=0, spacing="even", step_pad=(0, 0), reverse=False,
                 chroma_pad=None, transfer=None, inp=None):
        """inp: a variant_cases.Job that holds `planes` already (NV12, the pads given): its input slab is shared, not freed here."""
        import variant_cases as vc
        self.rig, self.n, self.dtype = rig, len(planes), np.dtype(dtype)
        self.h, self.w = planes[0][0].shape
        w, h, e = self.w, self.h, self.dtype.itemsize
        self.has_alpha = planes[0][2] is not None
        cpad = pads[1] if chroma_pad is None else 2 * chroma_pad
        self.shared = inp is not None
        self.inp = inp or vc.Job(rig, planes, pads=(pads[0], cpad, pads[2], 0), spacing=spacing, out_size=(2, 2), step_pad=(step_pad[0], 0),
                                 transfer=transfer if transfer is not None else vc.SRGB)
        if chroma_pad is not None:  # U then V, each H/2 rows of W/2 + chroma_pad bytes, over the bytes Job laid the CbCr rows in
            pitch = w // 2 + chroma_pad
            for i, (_, uv, _) in enumerate(planes):
                img = np.full((2, h // 2, pitch), vc.CANARY, np.uint8)
                img[0, :, :w // 2], img[1, :, :w // 2] = interleave_to_planar(uv)
                rig.upload(self.inp.frames[i].cbcr, img)
                self.inp.frames[i].cbcr_stride = pitch
        self.frames, self.alphas = self.inp.frames, self.inp.alphas
        self.stride = w * e + row_pad
        self.plane_bytes = self.stride * h
        slot = vc._up(4 * self.plane_bytes, 256) + step_pad[1]
        gap = lambda i: vc.GUARD if spacing == "table" and i == self.n - 1 and self.n > 1 else 0
        self.out_off = [vc.GUARD + i * slot + gap(i) + out_offset for i in range(self.n)]
        self.out_bytes = self.out_off[-1] + slot + vc.GUARD
        if reverse:
            self.out_off = self.out_off[::-1]
        self.d_out = rig.DeviceBuffer(rig.ctx, self.out_bytes, placement_tries=1)
        self.surfs = (Surface * self.n)(*[Surface(self.d_out.ptr + o, self.stride, w, h, FORMATS[self.dtype.name], 0) for o in self.out_off])
        self.before = np.full(self.out_bytes, vc.CANARY, np.uint8)
        rig.upload(self.d_out.ptr, self.before)

    def decode_batch(self, dec, stream=None, wait=1):
        return self.rig.lib.bt709hip_decode_batch(dec, self.n, self.frames, self.alphas, self.surfs, stream, wait)

    def decode_one(self, dec, i=0, stream=None, wait=1):
        alpha = C.byref(self.alphas[i]) if self.alphas is not None else None
        return self.rig.lib.bt709hip_decode(dec, C.byref(self.frames[i]), alpha, C.byref(self.surfs[i]), self.w, self.h, stream, wait)

    def collect(self, planes, label=""):
        """-> [(planes, H, W) of dtype] per slot; every byte outside those planes' rows must be what it was."""
        raw = self.rig.download(self.d_out.ptr, self.out_bytes)
        outside = np.ones(raw.size, bool)
        row = self.w * self.dtype.itemsize
        got = []
        for o in self.out_off:
            view = lambda a: a[o:o + planes * self.plane_bytes].reshape(planes * self.h, self.stride)[:, :row]
            got.append(view(raw).copy().view(self.dtype).reshape(planes, self.h, self.w))
            view(outside)[...] = False
        stray = np.flatnonzero(outside & (raw != self.before))
        assert stray.size == 0, "%s: %d bytes written outside the planes' rows, first at slab offset %d" % (label, stray.size, stray[0])
        return got

    def free(self):
        if not self.shared:
            self.inp.free()
        self.d_out.free()


NORM_CROP = slice(3 * 512, 4 * 512)  # columns of gpu_helpers.exhaustive_frame(): the chroma band bx >> 8 == 3, every row


def norm_picture(y, c):
    """A crop of the every-colour frame, 512 x 4096: every (Cb, Cr) pair under 32 luma codes spread over the whole range.  What it
    decodes to carries every output code in every channel at every position of a quad and in both rows (code_coverage; asserted
    by the tests that use it)."""
    return np.ascontiguousarray(y[:, NORM_CROP]), np.ascontiguousarray(c[:, NORM_CROP])


def code_coverage(bgra_words):
    """(H, W) words -> (3, 2, 4, 256) bool: [channel R G B, row & 1, column & 3, code] occurs."""
    seen = np.zeros((3, 2, 4, 256), bool)
    for c in range(3):
        code = (bgra_words >> np.uint32(16 - 8 * c)) & np.uint32(0xFF)
        for r in range(2):
            for q in range(4):
                seen[c, r, q, np.unique(code[r::2, q::4])] = True
    return seen


def assert_planes(got, want, label):
    """Bit for bit (floats by their bit patterns: -0 and the infinities count)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.view(np.uint8).reshape(got.shape + (-1,)), want.view(np.uint8).reshape(want.shape + (-1,))
    if np.array_equal(g, w):
        return
    c, r, x = np.argwhere((g != w).any(axis=-1))[0]
    raise AssertionError("%s: plane %s row %d column %d: got %r, want %r; %d elements differ"
                         % (label, "RGBA"[c], r, x, got[c, r, x], want[c, r, x], int((g != w).any(axis=-1).sum())))
