"""Planar I420 frames through the fused decode + rescale (BT709HIP_OPT_SCALED_PLANAR = 24), shared by
tests/test_scaled_planar_cpu.py and tests/test_scaled_planar_gpu.py (numpy only until a PlanarViewJob is made):

  * the shapes -- tests/scaled_chw_cases.py's, the smallest that still cross a wave, a 256-column tile and a strip boundary, plus the
    planar front end's own edges (W % 8 == 4, the smallest wide frame, a frame below it) -- each with the layout of its input planes
    and the tap form the launcher's record must name;
  * the chroma planes: test_planar_gpu.random_yuv's construction (every sample differs from its left and upper neighbour, U from V,
    so a sample that reaches the wrong pixel changes the output) and a uniform random set;
  * what the oracle's decode_nv12_scaled makes of the INTERLEAVED TWIN of the planes, computed once per process and never written;
  * PlanarViewJob: scaled_chw_cases.ViewJob over planar frames -- per slot Y, then U and (H/2) pitches behind it V, then alpha,
    every input byte that is no sample (row padding, the gap behind V, guard bands) holding `fill`.

The arithmetic is the NV12 kernels' by construction (one text from the tap word on); what is pinned here is the front end: which
chroma bytes reach which pixel, at which sizes, pitches and alignments, in which tap form."""
import zlib

import numpy as np

import chw_cases as cc
import scaled_chw_cases as sc
import variant_cases as vc
from metalbt709decoder_amd import _capi
from metalbt709decoder_amd._capi import Frame, Surface

OPT = 24
I420_ON = [(_capi.OPT_CHROMA_LAYOUT, _capi.CHROMA_I420), (OPT, 1)]

# name -> (source W x H, view OW x OH, input layout, the tap form the launcher's record must name)
SHAPES = {
    "once": ((96, 54), (300, 170), "aligned", "once"),            # two column tiles, a partial last trip
    "wide": ((520, 292), (346, 194), "aligned", "wide"),          # every plane, pitch and step 4-aligned
    "chroma-off1": ((520, 292), (346, 194), "chroma-off1", "bytes"),  # U pointer 1 byte off, odd chroma pitch, luma aligned
    "luma-off2": ((520, 292), (346, 194), "luma-off2", "bytes"),  # luma and alpha 2 bytes off, chroma aligned
    "w8r4": ((300, 36), (264, 40), "aligned", "bytes"),           # W % 8 == 4: W/2 - 8 is not 4-aligned, so never the wide form
    "decimate": ((200, 120), (60, 36), "aligned", "wide"),        # ratio above 2
    "smallest-wide": ((16, 4), (12, 6), "aligned", "wide"),       # W/2 == 8: the chroma window is the whole row
    "below-wide": ((12, 4), (10, 6), "aligned", "bytes"),
    "identity": ((40, 24), (40, 24), "aligned", "wide"),
    "half": ((64, 8), (32, 4), "aligned", "wide"),
}

# layout -> (offset of Y and alpha past a 256-byte boundary, their pitch, offset of U, the chroma pitch) of a frame W wide
_LAYOUTS = {
    "aligned": lambda w: (0, vc._up(w, 4), 0, vc._up(w // 2, 4)),
    "chroma-off1": lambda w: (0, vc._up(w, 4), 1, (w // 2 + 1) | 1),
    "luma-off2": lambda w: (2, vc._up(w, 4) + 2, 0, vc._up(w // 2, 4)),
}

_memo = {}


def interleave(u, v):
    """The NV12 twin of two planar chroma planes."""
    c = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    c[:, 0::2], c[:, 1::2] = u, v
    return c


def planes(shape, i=0, chroma="neighbours"):
    """Frame i of a shape: (y, u, v, alpha), read-only.  chroma "neighbours": every U and V sample differs from its left and upper
    neighbour, and U from V; "uniform": uniform random bytes."""
    key = ("planes", shape, i, chroma)
    if key not in _memo:
        w, h = SHAPES[shape][0]
        rng = np.random.default_rng([zlib.crc32(shape.encode()), w, h, i, 0 if chroma == "neighbours" else 1])
        ch, cw = h // 2, w // 2
        y, a = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
        if chroma == "neighbours":
            step = np.arange(cw)[None, :] * 37 + np.arange(ch)[:, None] * 101  # odd multipliers: neighbours differ mod 256
            u = ((int(rng.integers(0, 256)) + step) & 255).astype(np.uint8)
            v = ((u.astype(np.int64) + 1 + rng.integers(0, 254)) & 255).astype(np.uint8)
            assert (u[:, 1:] != u[:, :-1]).all() and (v[:, 1:] != v[:, :-1]).all() and (u[1:] != u[:-1]).all() and (v[1:] != v[:-1]).all() and (u != v).all()
        else:
            u, v = rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)
        _memo[key] = (y, u, v, a)
        for p in _memo[key]:
            p.setflags(write=False)
    return _memo[key]


def twin(frame):
    """(y, cbcr, alpha): the NV12 frame a planar frame is the de-interleaved form of."""
    y, u, v, a = frame
    return np.ascontiguousarray(y), interleave(u, v), a


def want_words(oracle, shape, gamma, alpha, i=0, chroma="neighbours", view=None):
    """(OH, OW) words of the 8-bit view of frame i: the oracle's decode_nv12_scaled of the interleaved twin."""
    ow, oh = view or SHAPES[shape][1]
    key = ("want", shape, gamma, alpha, i, chroma, ow, oh)
    if key not in _memo:
        y, c, a = twin(planes(shape, i, chroma))
        _memo[key] = cc.words_of(oracle.decode_nv12_scaled(gamma, y, c, ow, oh, alpha=a if alpha else None))
        _memo[key].setflags(write=False)
    return _memo[key]


def assert_words(got, want, label):
    """Two (OH, OW) arrays of BGRA8 words."""
    if not np.array_equal(got, want):
        r, x = np.argwhere(got != want)[0]
        raise AssertionError("%s: differs first at row %d, column %d (got %08x, want %08x); %d of %d words differ"
                             % (label, r, x, got[r, x], want[r, x], int((got != want).sum()), got.size))


def kernel_name(dtype, alpha):
    if dtype is None:
        return b"decode_i420_scaled<alpha>" if alpha else b"decode_i420_scaled"
    return ("decode_i420_scaled_chw<%s%s>" % (cc.ELEM_NAMES[np.dtype(dtype).name], ",alpha" if alpha else "")).encode()


class PlanarViewJob(sc.ViewJob):
    """frames: [(y, u, v, alpha)] of one size, laid out as `layout` says; the views as scaled_chw_cases.ViewJob lays them out (dtype
    None: BGRA8 surfaces with 16 bytes of row padding; else planar surfaces in slots with room for four planes).  Every input byte
    that is no sample holds `fill`.  spacing "table": a gap before the last slot on both sides; slot_extra: bytes added to the
    spacing of the input slots (an odd one makes every step of an evenly spaced batch odd)."""

    def __init__(self, rig, frames, layout, view, dtype=None, has_alpha=False, row_pad=0, spacing="even", fill=0x00, slot_extra=0, transfer=None):
        self.rig, self.n, self.has_alpha = rig, len(frames), has_alpha
        self.dtype = None if dtype is None else np.dtype(dtype)
        self.h, self.w = frames[0][0].shape
        self.ow, self.oh = view
        w, h = self.w, self.h
        y_off, ys, u_off, cs = _LAYOUTS[layout](w)
        c_off = vc._up(y_off + ys * h, 256) + u_off
        a_off = vc._up(c_off + cs * h, 256) + y_off          # U and V: 2 x (H/2) rows
        in_pitch = vc._up(a_off + ys * h, 256) + slot_extra
        gap = lambda i: vc.GUARD if spacing == "table" and i == self.n - 1 and self.n > 1 else 0
        in_off = [vc.GUARD + i * in_pitch + gap(i) for i in range(self.n)]
        host = np.full(in_off[-1] + in_pitch + vc.GUARD, fill, np.uint8)
        for i, (y, u, v, a) in enumerate(frames):
            for plane, o, stride, rows, cols in ((y, y_off, ys, h, w), (u, c_off, cs, h // 2, w // 2), (v, c_off + (h // 2) * cs, cs, h // 2, w // 2),
                                                 (a if has_alpha else None, a_off, ys, h, w)):
                if plane is not None:
                    host[in_off[i] + o:in_off[i] + o + stride * rows].reshape(rows, stride)[:, :cols] = plane
        self.d_in = rig.DeviceBuffer(rig.ctx, host.size, placement_tries=1)
        rig.upload(self.d_in.ptr, host)
        transfer = transfer if transfer is not None else vc.SRGB
        base = self.d_in.ptr
        self.frames = (Frame * self.n)(*[Frame(base + o + y_off, ys, base + o + c_off, cs, w, h, vc.MATRIX, transfer) for o in in_off])
        self.alphas = (Frame * self.n)(*[Frame(base + o + a_off, ys, None, ys, w, h, vc.MATRIX, vc.LINEAR) for o in in_off]) if has_alpha else None
        e = 4 if self.dtype is None else self.dtype.itemsize
        self.stride = self.ow * e + (16 if self.dtype is None else row_pad)
        self.plane_bytes = self.stride * self.oh
        slot = vc._up((1 if self.dtype is None else 4) * self.plane_bytes, 256)
        self.out_off = [vc.GUARD + i * slot + gap(i) for i in range(self.n)]
        self.out_bytes = self.out_off[-1] + slot + vc.GUARD
        self.d_out = rig.DeviceBuffer(rig.ctx, self.out_bytes, placement_tries=1)
        fmt = _capi.FORMAT_BGRA8_SRGB if self.dtype is None else cc.FORMATS[self.dtype.name]
        self.surfs = (Surface * self.n)(*[Surface(self.d_out.ptr + o, self.stride, self.ow, self.oh, fmt, 0) for o in self.out_off])
        self.refill()
