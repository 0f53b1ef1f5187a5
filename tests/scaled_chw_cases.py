"""The fused decode + rescale into planar CHW views (BT709HIP_OPT_SCALED_CHW), shared by tests/test_scaled_chw_cpu.py
and tests/test_scaled_chw_gpu.py (numpy only until a ViewJob is made):

  * the shapes -- the smallest that still cross a wave, a 256-column tile and a strip boundary, one per tap form -- their frames
    (seeded) and what the oracle makes of them, computed once per process and never written;
  * ViewJob: `n` frames of a shape in the shape's input layout and `n` views in a canary slab of their own -- planar (always with
    room for a fourth plane) or BGRA8 -- driven through the four C entry points; collect() hands back the planes / words and
    asserts that every other byte of the slab is what it was.

The definition itself is chw_cases.chw_of over the 8-bit words of the same view."""
import ctypes as C
import zlib

import numpy as np

import chw_cases as cc
import metalbt709decoder_amd as mb
import variant_cases as vc
from metalbt709decoder_amd import _capi
from metalbt709decoder_amd._capi import Frame, Surface

APPLE, SRGB = mb.MetalBT709GammaApple, mb.MetalBT709GammaSRGB
DTYPES = ("uint8", "float16", "float32")
OPT = _capi.OPT_SCALED_CHW
TAPS_NAME = {_capi.SCALED_TAPS_BYTES: "bytes", _capi.SCALED_TAPS_PAIRS: "pairs", _capi.SCALED_TAPS_WIDE: "wide",
             _capi.SCALED_TAPS_SHARED: "shared", _capi.SCALED_TAPS_ONCE: "once"}
BY_WAVE = ("once", "shared")

# name -> (source W x H, view OW x OH, input layout, the tap form(s) the launcher's record must name).  layout: "aligned" -- plane
# addresses and pitches multiples of 4; "off2" -- planes 2 bytes past that, pitches 2 mod 4; "off1" -- planes 1 byte past it, odd pitches
SHAPES = {
    "once": ((96, 54), (300, 170), "aligned", ("once",)),          # two column tiles, a partial last trip
    "wide": ((520, 292), (346, 194), "aligned", ("wide",)),        # ratio 1.5, persistent; OW = 2 mod 4
    "pairs": ((520, 292), (346, 194), "off2", ("pairs",)),
    "bytes": ((520, 292), (346, 194), "off1", ("bytes",)),
    "shared": ((300, 36), (264, 40), "aligned", ("shared",)),      # reducing in x, enlarging in y
    "decimate": ((200, 120), (60, 36), "aligned", ("bytes", "pairs", "wide")),  # ratio above 2
    "identity": ((40, 24), (40, 24), "aligned", ("bytes", "pairs", "wide")),
}

TORCH_SHAPE, TORCH_FRAMES = "decimate", 5  # tests/scaled_chw_torch_child.py fills a (5, 3, 36, 60) tensor from frames 0..4 of that shape

_memo = {}


def add_shape(name, src, view, layout="aligned", taps=("bytes", "pairs", "wide")):
    SHAPES.setdefault(name, (src, view, layout, taps))
    return name


def planes(shape, i=0):
    """Frame i of a shape: uniform random bytes (y, cbcr, alpha), read-only."""
    key = ("planes", shape, i)
    if key not in _memo:
        w, h = SHAPES[shape][0]
        rng = np.random.default_rng([zlib.crc32(shape.encode()), w, h, i])  # the name, not its place in the table: shapes may be added
        _memo[key] = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8),
                      rng.integers(0, 256, (h, w), dtype=np.uint8))
        for a in _memo[key]:
            a.setflags(write=False)
    return _memo[key]


def want_words(oracle, shape, gamma, alpha, i=0, view=None, frame=None):
    """(OH, OW) words of the 8-bit view of frame i (or of `frame` = (key, y, cbcr, alpha)): the oracle's decode_nv12_scaled."""
    ow, oh = view or SHAPES[shape][1]
    key = ("want", frame[0] if frame else shape, gamma, alpha, i, ow, oh)
    if key not in _memo:
        y, c, a = frame[1:] if frame else planes(shape, i)
        _memo[key] = cc.words_of(oracle.decode_nv12_scaled(gamma, y, c, ow, oh, alpha=a if alpha else None))
        _memo[key].setflags(write=False)
    return _memo[key]


def kernel_name(dtype, alpha):
    return ("decode_nv12_scaled_chw<%s%s>" % (cc.ELEM_NAMES[np.dtype(dtype).name], ",alpha" if alpha else "")).encode()


def norm_options(scale, bias):
    return [(_capi.OPT_CHW_SCALE_R + i, cc.bits(v)) for i, v in enumerate(tuple(scale) + tuple(bias))]


def plan(lib):
    info = _capi.ScaledLaunchInfo()
    _capi.check(lib.bt709hip_last_scaled_launch_info(C.byref(info)))
    return dict(grid=tuple(info.grid), block=tuple(info.block), taps=TAPS_NAME.get(info.taps, info.taps), rows=info.rows,
                persistent=info.persistent, balanced=info.balanced, resident=info.resident, items=info.items)


_LAYOUTS = {"aligned": lambda w: (0, vc._up(w, 4), vc._up(w, 4)), "off2": lambda w: (2, w + 2, w + 2), "off1": lambda w: (1, w + 1, w + 3)}


class ViewJob:
    """frames: [(y, cbcr, alpha)] of one size, laid out as `layout` says; views of `view` = (OW, OH): dtype None -- BGRA8 surfaces
    with 16 bytes of row padding; else planar surfaces of that element type in slots with room for FOUR planes, rows padded by
    row_pad bytes, every plane-0 pointer moved by out_offset bytes.  spacing "table": a gap before the last slot on both sides;
    reverse: the views run backwards through the slab (an evenly spaced batch with a negative output step)."""

    def __init__(self, rig, frames, layout, view, dtype=None, has_alpha=False, row_pad=0, out_offset=0, spacing="even", reverse=False,
                 transfer=None):
        self.rig, self.n, self.has_alpha = rig, len(frames), has_alpha
        self.dtype = None if dtype is None else np.dtype(dtype)
        self.h, self.w = frames[0][0].shape
        self.ow, self.oh = view
        w, h = self.w, self.h
        off, ys, cs = _LAYOUTS[layout](w)
        c_off = vc._up(off + ys * h, 256) + off
        a_off = vc._up(c_off + cs * (h // 2), 256) + off
        in_pitch = vc._up(a_off + ys * h, 256)
        gap = lambda i: vc.GUARD if spacing == "table" and i == self.n - 1 and self.n > 1 else 0
        in_off = [vc.GUARD + i * in_pitch + gap(i) for i in range(self.n)]
        host = np.full(in_off[-1] + in_pitch + vc.GUARD, vc.CANARY, np.uint8)
        for i, (y, uv, a) in enumerate(frames):
            for plane, o, stride, rows in ((y, off, ys, h), (uv, c_off, cs, h // 2), (a if has_alpha else None, a_off, ys, h)):
                if plane is not None:
                    host[in_off[i] + o:in_off[i] + o + stride * rows].reshape(rows, stride)[:, :w] = plane
        self.d_in = rig.DeviceBuffer(rig.ctx, host.size, placement_tries=1)
        rig.upload(self.d_in.ptr, host)
        transfer = transfer if transfer is not None else vc.SRGB
        base = self.d_in.ptr
        self.frames = (Frame * self.n)(*[Frame(base + o + off, ys, base + o + c_off, cs, w, h, vc.MATRIX, transfer) for o in in_off])
        self.alphas = (Frame * self.n)(*[Frame(base + o + a_off, ys, base + o + c_off, cs, w, h, vc.MATRIX, vc.LINEAR)
                                         for o in in_off]) if has_alpha else None
        e = 4 if self.dtype is None else self.dtype.itemsize
        self.stride = self.ow * e + (16 if self.dtype is None else row_pad)
        self.plane_bytes = self.stride * self.oh
        slot = vc._up((1 if self.dtype is None else 4) * self.plane_bytes, 256)
        self.out_off = [vc.GUARD + i * slot + gap(i) + out_offset for i in range(self.n)]
        self.out_bytes = self.out_off[-1] + slot + vc.GUARD
        if reverse:
            self.out_off = self.out_off[::-1]
        self.d_out = rig.DeviceBuffer(rig.ctx, self.out_bytes, placement_tries=1)
        fmt = _capi.FORMAT_BGRA8_SRGB if self.dtype is None else cc.FORMATS[self.dtype.name]
        self.surfs = (Surface * self.n)(*[Surface(self.d_out.ptr + o, self.stride, self.ow, self.oh, fmt, 0) for o in self.out_off])
        self.refill()

    def refill(self):
        self.before = np.full(self.out_bytes, vc.CANARY, np.uint8)
        self.rig.upload(self.d_out.ptr, self.before)

    def launch(self, dec, entry="bt709hip_decode_scaled_batch", stream=None, wait=1):
        """One call of a C entry point over the whole job (the single-frame ones: n == 1) -> its return code."""
        fn = getattr(self.rig.lib, entry)
        if entry.endswith("_batch"):
            return fn(dec, self.n, self.frames, self.alphas, self.surfs, stream, wait)
        assert self.n == 1
        return fn(dec, C.byref(self.frames[0]), C.byref(self.alphas[0]) if self.alphas is not None else None, C.byref(self.surfs[0]), stream, wait)

    def collect(self, label=""):
        """-> per slot (planes, OH, OW) of dtype, or (OH, OW) words of a BGRA8 view; every byte outside them must be what it was."""
        raw = self.rig.download(self.d_out.ptr, self.out_bytes)
        outside = np.ones(raw.size, bool)
        count = 1 if self.dtype is None else (4 if self.has_alpha else 3)
        row = self.ow * (4 if self.dtype is None else self.dtype.itemsize)
        got = []
        for o in self.out_off:
            view = lambda a: a[o:o + count * self.plane_bytes].reshape(count * self.oh, self.stride)[:, :row]
            px = view(raw).copy()
            got.append(px.view(np.uint32).reshape(self.oh, self.ow) if self.dtype is None else px.view(self.dtype).reshape(count, self.oh, self.ow))
            view(outside)[...] = False
        stray = np.flatnonzero(outside & (raw != self.before))
        assert stray.size == 0, "%s: %d bytes written outside the views' rows, first at slab offset %d" % (label, stray.size, stray[0])
        return got

    def free(self):
        self.d_in.free()
        self.d_out.free()
