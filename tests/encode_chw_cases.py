"""Planar CHW encoder INPUT (BT709HIP_CTX_OPT_ENCODE_CHW_INPUT) in numpy, shared by tests/test_encode_chw_cpu.py and
tests/test_encode_chw_gpu.py:

  * the definition: byte_of() -- u8 the byte itself; a float element t -> u = t * scale; u = u + bias (float32, one rounding each);
    x = sat(u) (NaN -> 0, u < 0 -> 0, u > 1 -> 1); s = round-half-away of float32(x * 255) -- and words_of_planes(), the BGRA8
    picture (B, G, R, A) = (s_B, s_G, s_R, 255) whose encode the CHW encode must equal byte for byte;
  * the (scale, bias) settings every sweep uses: the identity, ImageNet's (std, mean) and one with negative scales;
  * the float32 edge set: for each byte k the floats around (k + 0.5) / 255 (+-3 ulp), zeros, subnormals, infinities, NaNs, values
    below 0 and above 1;
  * Plan / Rig: tensors in a poison-filled input slab (0xFF: the byte 255, a NaN half, a NaN float -- row padding, the gaps
    between surfaces and the fourth plane hold it) and frames in a canary-filled output slab that is compared WHOLE, so guard
    bands and the row padding of Y, CbCr, U and V are part of every comparison.
Expected bytes never come from the code under test: they are the oracle's encode of the byte picture."""
import ctypes as C

import numpy as np

import chw_cases as cc
import encoder_cases as ec
from metalbt709decoder_amd import _capi

OPT_CHW_INPUT, OPT_SCALE_R, OPT_BIAS_R = 18, 20, 23  # stated here, not taken from the bindings
OPT_ROW_PAIRS, OPT_THREADS, OPT_XCD_BANDS, OPT_LAYOUT = 2, 3, 4, 6
NV12, I420 = 0, 1
FORMATS = cc.FORMATS
ELEM_NAMES = cc.ELEM_NAMES
DTYPES = ("uint8", "float16", "float32")
MAX_TABLE = 31  # kMaxChwBatch: surfaces in the pointer table of a CHW launch (BT709HIP_MAX_BATCH - 1)
POISON, FILL, GUARD = 0xFF, ec.FILL, 4096

IDENTITY = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
IMAGENET = (tuple(np.asarray(cc.IMAGENET_STD, np.float32)), tuple(np.asarray(cc.IMAGENET_MEAN, np.float32)))  # setEncodeCHWMeanStd: (std, mean)
NEGATIVE = ((-1.0, -0.5, -2.0), (1.0, 0.75, 1.5))
SETTINGS = {"identity": IDENTITY, "imagenet": IMAGENET, "negative": NEGATIVE}


def kernel_name(dtype, layout, fast):
    return "encode_chw_%s%s<%s>" % ("i420" if layout == I420 else "nv12", "" if fast else "_blocks", ELEM_NAMES[np.dtype(dtype).name])


# ------------------------------------------------------------------ the definition

def saturate(u):
    u = np.asarray(u, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(u > 0, np.where(u > 1, np.float32(1.0), u), np.float32(0.0)).astype(np.float32)


def quantise(x):
    """round-half-away-from-zero of float32(x * 255) for x in [0, 1] (csrc/bt709_quantise.h quantise_exact)."""
    v = np.asarray(x, np.float32) * np.float32(255.0)
    t = np.trunc(v)
    return (t + ((v - t) >= np.float32(0.5))).astype(np.uint8)


def byte_of(t, scale, bias):
    """Elements of any dtype of DTYPES -> bytes."""
    t = np.asarray(t)
    if t.dtype == np.uint8:
        return t.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        u = t.astype(np.float32) * np.float32(scale)
        u = u + np.float32(bias)
    return quantise(saturate(u))


def bytes_of_planes(planes, setting=IDENTITY):
    """(>= 3, H, W) tensor -> (3, H, W) bytes of planes R, G, B."""
    return np.stack([byte_of(planes[c], setting[0][c], setting[1][c]) for c in range(3)])


def words_of_planes(planes, setting=IDENTITY):
    """The BGRA8 picture the tensor stands for: (H, W) words (255 << 24) | (R << 16) | (G << 8) | B."""
    s = bytes_of_planes(planes, setting).astype(np.uint32)
    return np.uint32(0xFF000000) | (s[0] << np.uint32(16)) | (s[1] << np.uint32(8)) | s[2]


def float_edges():
    """The float32 edge set as uint32 bit patterns."""
    k = np.arange(256, dtype=np.float64)
    mid = ((k + 0.5) / 255.0).astype(np.float32).view(np.uint32).astype(np.int64)
    around = (mid[:, None] + np.arange(-3, 4)[None, :]).reshape(-1)
    special = [0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001,
               0x7FFFFFFF, 0xFFFFFFFF, 0xFF800001, 0x3F800000, 0x3F800001, 0x3F7FFFFF, 0xBF800000, 0x40000000, 0xC0000000, 0x7F7FFFFF, 0xFF7FFFFF,
               0x3B808081, 0x3B008081, 0x3B008080, 0x3B00807F, 0x3F000000, 0xBF000000, 0x42FE0000, 0x437F0000, 0xB3000000, 0x33000000]
    return np.concatenate([around, np.array(special, np.int64)]).astype(np.uint32)


TORCH_N, TORCH_W, TORCH_H = 5, 24, 6


def torch_tensor_values():
    """(N, 3, H, W) float16: ImageNet-normalised pixels, a little outside [0, 1] on both sides, with NaNs and infinities sprinkled in
    -- the same array in tests/encode_chw_torch_child.py and in the test that starts it"""
    rng = np.random.default_rng(2200)
    x = rng.random((TORCH_N, 3, TORCH_H, TORCH_W), dtype=np.float32) * np.float32(1.3) - np.float32(0.15)
    mean, std = np.asarray(cc.IMAGENET_MEAN, np.float32).reshape(1, 3, 1, 1), np.asarray(cc.IMAGENET_STD, np.float32).reshape(1, 3, 1, 1)
    t = ((x - mean) / std).astype(np.float16)
    flat = t.reshape(-1)
    flat[::97] = np.float16(np.nan)
    flat[5::131] = np.float16(np.inf)
    flat[7::113] = -np.float16(np.inf)
    return t


def planar(uv):
    """(H/2, W) CbCr rows -> (2, H/2, W/2): U rows then V rows."""
    return np.stack(cc.interleave_to_planar(uv))


# ------------------------------------------------------------------ slabs

def _up(v, a):
    return (v + a - 1) // a * a


class Plan:
    """`n` tensors of (planes, h, w) elements of `dtype` and `n` frames.
    row_pad: elements added to a plane row; shift: bytes added to every plane-0 pointer; planes: 3, or 4 (a poisoned fourth plane lies
    behind B); spacing "even" / "table" (a gap before the last slot: a pointer table); slot_pad: (input, output) bytes added to the
    slot distance; y_pad / c_pad: bytes added to the Y and chroma pitch; out_shift: bytes added to every Y and chroma pointer."""

    def __init__(self, w, h, n, dtype, layout, row_pad=0, shift=0, planes=3, spacing="even", slot_pad=(0, 0), y_pad=0, c_pad=0, out_shift=0):
        self.w, self.h, self.n, self.dtype, self.layout, self.planes = w, h, n, np.dtype(dtype), layout, planes
        e = self.e = self.dtype.itemsize
        self.stride = (w + row_pad) * e
        self.plane_bytes = self.stride * h
        gap = lambda i: 4096 if spacing == "table" and n > 1 and i == n - 1 else 0
        in_slot = _up(planes * self.plane_bytes, 256) + slot_pad[0]
        self.in_off = [GUARD + i * in_slot + gap(i) + shift for i in range(n)]
        self.in_bytes = self.in_off[-1] + in_slot + GUARD
        self.y_pitch = w + y_pad
        self.c_pitch = (w // 2 if layout == I420 else w) + c_pad
        self.c_rows = h if layout == I420 else h // 2
        y_bytes, c_bytes = _up(h * self.y_pitch, 256), _up(self.c_rows * self.c_pitch, 256)
        out_slot = y_bytes + c_bytes + slot_pad[1]
        self.y_off = [GUARD + i * out_slot + gap(i) + out_shift for i in range(n)]
        self.c_off = [o + y_bytes for o in self.y_off]
        self.out_bytes = self.y_off[-1] + out_slot + GUARD

    def fast(self):
        e4, chroma = 4 * self.e, 2 if self.layout == I420 else 4
        return (self.w % 4 == 0 and self.stride % e4 == 0 and all(o % e4 == 0 for o in self.in_off) and self.y_pitch % 4 == 0
                and self.c_pitch % chroma == 0 and all(o % 4 == 0 for o in self.y_off) and all(o % chroma == 0 for o in self.c_off))

    def input_slab(self, tensors):
        slab = np.full(self.in_bytes, POISON, np.uint8)
        row = self.w * self.e
        for o, t in zip(self.in_off, tensors):
            t = np.ascontiguousarray(t[:3], self.dtype)
            view = slab[o:o + 3 * self.plane_bytes].reshape(3 * self.h, self.stride)
            view[:, :row] = t.view(np.uint8).reshape(3 * self.h, row)
        return slab

    def expected(self, frames):
        """frames: [(y (h, w), cbcr (h/2, w) interleaved)] -> the whole output slab"""
        slab = np.full(self.out_bytes, FILL, np.uint8)
        for i, (y, c) in enumerate(frames):
            slab[self.y_off[i]:self.y_off[i] + self.h * self.y_pitch].reshape(self.h, self.y_pitch)[:, :self.w] = y
            cw = self.w // 2 if self.layout == I420 else self.w
            rows = planar(c).reshape(self.h, cw) if self.layout == I420 else c
            slab[self.c_off[i]:self.c_off[i] + self.c_rows * self.c_pitch].reshape(self.c_rows, self.c_pitch)[:, :cw] = rows
        return slab

    def describe(self, got, want):
        if np.array_equal(got, want):
            return None
        at = int(np.flatnonzero(got != want)[0])
        where = "outside every plane"
        for i in range(self.n):
            if self.y_off[i] <= at < self.y_off[i] + self.h * self.y_pitch:
                r, x = divmod(at - self.y_off[i], self.y_pitch)
                where = "frame %d Y row %d column %d%s" % (i, r, x, " (row padding)" if x >= self.w else "")
            elif self.c_off[i] <= at < self.c_off[i] + self.c_rows * self.c_pitch:
                r, x = divmod(at - self.c_off[i], self.c_pitch)
                where = "frame %d chroma row %d byte %d" % (i, r, x)
        return "%d bytes differ, first at slab offset %d (%s): got %d, want %d" % (int((got != want).sum()), at, where, got[at], want[at])


class Result:
    def __init__(self, slab, kernel, info):
        self.slab, self.kernel = slab, kernel
        self.record = (tuple(info.grid), info.block[0], info.launches, info.xcd_bands)


class Rig(ec.Harness):
    """bt709hip_encode[_batch] of CHW tensors on a Plan's slabs, and of their BGRA8 twins on the same output plan.  Every option is
    set for the call and put back after it whatever happens (the context is the process's)."""

    def set(self, option, value):
        rc = self.lib.bt709hip_context_set_option(self.h, option, value)
        assert rc == _capi.OK, "bt709hip_context_set_option(%d, %d): %s" % (option, value, _capi.strerror(rc))

    def set_norm(self, setting):
        for i, v in enumerate(tuple(setting[0]) + tuple(setting[1])):
            self.set(OPT_SCALE_R + i, cc.bits(v))

    def _call(self, P, surfaces, d_out, gammas, options, gate):
        _capi.check(self.lib.bt709hip_memset(self.h, d_out.ptr, FILL, P.out_bytes, None))
        _capi.check(self.lib.bt709hip_stream_synchronize(self.h, None))
        surfs = (_capi.Surface * P.n)(*surfaces)
        frames = (_capi.Frame * P.n)(*[_capi.Frame(d_out.ptr + P.y_off[i], P.y_pitch, d_out.ptr + P.c_off[i], P.c_pitch, P.w, P.h, 0, 0) for i in range(P.n)])
        options = dict(options or {})
        options[OPT_LAYOUT] = P.layout
        if gate:
            options[OPT_CHW_INPUT] = 1
        defaults = {OPT_LAYOUT: NV12, OPT_CHW_INPUT: 0, OPT_ROW_PAIRS: 0, OPT_THREADS: 0, OPT_XCD_BANDS: 1}
        try:
            for o, v in options.items():
                self.set(o, v)
            if P.n == 1:
                rc = self.lib.bt709hip_encode(self.h, surfs, frames, gammas[0], gammas[1], None, 1)
            else:
                rc = self.lib.bt709hip_encode_batch(self.h, P.n, surfs, frames, gammas[0], gammas[1], None, 1)
        finally:
            for o in options:
                self.set(o, defaults[o])
        return rc

    def _result(self, d_out, P):
        kernel = self.lib.bt709hip_last_kernel_name().decode()
        info = _capi.LaunchInfo()
        _capi.check(self.lib.bt709hip_last_launch_info(C.byref(info)))
        return Result(self._download(d_out.ptr, P.out_bytes), kernel, info)

    def encode(self, P, tensors, gammas, setting=IDENTITY, options=None, expect_rc=_capi.OK):
        d_in = self.DeviceBuffer(self.ctx, P.in_bytes, placement_tries=1)
        d_out = self.DeviceBuffer(self.ctx, P.out_bytes, placement_tries=1)
        try:
            assert d_in.ptr % 256 == 0 and d_out.ptr % 256 == 0  # alignment is reasoned on offsets inside the slabs
            self._upload(d_in.ptr, P.input_slab(tensors))
            surfaces = [_capi.Surface(d_in.ptr + o, P.stride, P.w, P.h, FORMATS[P.dtype.name], 0) for o in P.in_off]
            self.set_norm(setting)
            try:
                rc = self._call(P, surfaces, d_out, gammas, options, True)
            finally:
                self.set_norm(IDENTITY)
            assert rc == expect_rc, "bt709hip_encode of CHW input: %s" % _capi.strerror(rc)
            return self._result(d_out, P)
        finally:
            d_in.free()
            d_out.free()

    def encode_bgra(self, P, pictures, gammas, options=None):
        """The product's own BGRA8 encode of the (h, w) word pictures into P's output plan (tight input, 16-byte aligned)."""
        slot = _up(4 * P.w * P.h, 256)
        d_in = self.DeviceBuffer(self.ctx, slot * P.n, placement_tries=1)
        d_out = self.DeviceBuffer(self.ctx, P.out_bytes, placement_tries=1)
        try:
            host = np.zeros(slot * P.n, np.uint8)
            for i, words in enumerate(pictures):
                host[i * slot:i * slot + 4 * P.w * P.h] = np.ascontiguousarray(words, np.uint32).view(np.uint8).reshape(-1)
            self._upload(d_in.ptr, host)
            surfaces = [_capi.Surface(d_in.ptr + i * slot, 4 * P.w, P.w, P.h, _capi.FORMAT_BGRA8_SRGB, 0) for i in range(P.n)]
            _capi.check(self._call(P, surfaces, d_out, gammas, options, False), "bt709hip_encode of the BGRA8 twin")
            return self._result(d_out, P)
        finally:
            d_in.free()
            d_out.free()


def check(rig, oracle, P, tensors, gammas, setting=IDENTITY, options=None, fast=None, label=""):
    """Encodes `tensors` on P; the whole output slab must equal the oracle's encode of the byte pictures AND the product's own BGRA8
    encode of them; the kernel must be the one the plan was built to reach.  -> the Result"""
    fast = P.fast() if fast is None else fast
    pictures = [words_of_planes(t, setting) for t in tensors]
    want = P.expected([ec.threaded_encode(oracle, words, P.w, P.h, gammas[0], gammas[1]) for words in pictures])
    res = rig.encode(P, tensors, gammas, setting, options)
    assert res.kernel == kernel_name(P.dtype, P.layout, fast), (label, res.kernel)
    problem = P.describe(res.slab, want)
    assert problem is None, (label, problem)
    twin = rig.encode_bgra(P, pictures, gammas, options)
    problem = P.describe(res.slab, twin.slab)
    assert problem is None, (label, "against the BGRA8 encode", problem)
    return res, twin
