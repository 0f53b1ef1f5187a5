"""Case builders shared by tests/test_decode_variants.py and tests/test_over_gpu.py (numpy only until a Rig is made):

  * Rig / Job: frames of one geometry in canary-filled device slabs with guard bands and padded pitches, driven through the C
    ABI; Job.collect() hands back the pixels and asserts that every other byte of the target slab is what it was;
  * Colours: gpu_helpers.exhaustive_frame() -- every (Y,Cb,Cr) once -- and, per gamma, the 4096 x 4096 BGRA image the oracle's
    table says it decodes to (the inverse of gpu_helpers.exhaustive_to_table);
  * the alpha plane that carries every alpha code in every position of a 2x2 block, the packed 4:4:4 frames that hold every
    24-bit word under every value of byte 3, and their expected words;
  * a pure-Python mirror of the shim's grid_x_for and the general path's launch-shape cases computed from it."""
import ctypes as C

import numpy as np

import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi
from metalbt709decoder_amd._capi import Frame, Surface

import rescale_arith_cases as rc

CANARY = 0x5A
GUARD = 256
MATRIX, SRGB, LINEAR = mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2, mb.kCVImageBufferTransferFunction_sRGB, mb.kCVImageBufferTransferFunction_Linear


def _up(v, a):
    return (v + a - 1) // a * a


class Rig:
    def __init__(self, gh):
        from metalbt709decoder_amd.decoder import DeviceBuffer
        self.DeviceBuffer = DeviceBuffer
        self.ctx = gh.context()
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.decoders = []

    def decoder(self, over=None, options=(), setup=True, gamma=mb.MetalBT709GammaSRGB, has_alpha=True):
        d = C.c_void_p()
        _capi.check(self.lib.bt709hip_decoder_create(self.h, gamma, 1 if has_alpha else 0, C.byref(d)))
        self.decoders.append(d)
        for opt, val in options:
            _capi.check(self.lib.bt709hip_decoder_set_option(d, opt, val))
        if over is not None:
            self.set_over(d, over)
        if setup:
            _capi.check(self.lib.bt709hip_decoder_setup(d), "decoder setup")
        return d

    def set_over(self, dec, over):
        _capi.check(self.lib.bt709hip_decoder_set_option(dec, _capi.OPT_COMPOSITE_OVER, over), "set composite over")

    def option(self, dec, opt):
        v = C.c_int(-12345)
        _capi.check(self.lib.bt709hip_decoder_get_option(dec, opt, C.byref(v)))
        return v.value

    def sync(self, stream=None):
        _capi.check(self.lib.bt709hip_stream_synchronize(self.h, stream))

    def kernel(self):
        return self.lib.bt709hip_last_kernel_name()

    def launch(self):
        """The launch on record: (grid, block, launches, xcd_bands)."""
        info = _capi.LaunchInfo()
        _capi.check(self.lib.bt709hip_last_launch_info(C.byref(info)))
        return tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr).reshape(-1)
        _capi.check(self.lib.bt709hip_upload(self.h, dptr, arr.size, arr.ctypes.data, arr.size, arr.size, 1, None), "upload")
        self.sync()

    def download(self, dptr, nbytes):
        out = np.empty(nbytes, np.uint8)
        _capi.check(self.lib.bt709hip_download(self.h, out.ctypes.data, nbytes, dptr, nbytes, nbytes, 1, None), "download")
        self.sync()
        return out

    def close(self):
        for d in self.decoders:
            self.lib.bt709hip_decoder_destroy(d)
        self.decoders = []


class Job:
    """`n` frames of one geometry in device memory -- Y, CbCr and alpha planes with their own pitches in one slab, the targets in
    another, each slab with guard bands -- and the descriptors for them.  planes: [(y, cbcr, alpha)], alpha None throughout for
    an opaque decoder; pads: extra bytes per row of (Y, CbCr, alpha, output); out_offset: bytes added to every output pointer;
    spacing "table": a gap before the last slot, so that no single step reaches every frame and the launch takes the pointer
    table; step_pad: bytes added to the (256-byte multiple) distance between two input / two output slots, so that the step
    itself can misalign the frames; transfer: the frames' transfer tag."""

    def __init__(self, rig, planes, pads=(0, 0, 0, 0), out_offset=0, spacing="even", fmt=_capi.FORMAT_BGRA8_SRGB, out_size=None,
                 step_pad=(0, 0), transfer=SRGB):
        self.rig, self.n = rig, len(planes)
        self.h, self.w = planes[0][0].shape
        w, h = self.w, self.h
        self.ow, self.oh = out_size or (w, h)
        self.px = 8 if fmt == _capi.FORMAT_RGBA16F else 4
        self.sy, self.sc, self.sa, self.so = w + pads[0], w + pads[1], w + pads[2], self.px * self.ow + pads[3]
        has_alpha = planes[0][2] is not None
        c_off = _up(self.sy * h, 256)
        a_off = c_off + _up(self.sc * (h // 2), 256)
        in_pitch = a_off + (_up(self.sa * h, 256) if has_alpha else 0) + step_pad[0]
        out_pitch = _up(self.so * self.oh, 256) + step_pad[1]
        gap = lambda i: GUARD if spacing == "table" and i == self.n - 1 and self.n > 1 else 0
        self.in_off = [GUARD + i * in_pitch + gap(i) for i in range(self.n)]
        self.out_off = [GUARD + i * out_pitch + gap(i) + out_offset for i in range(self.n)]
        host = np.full(self.in_off[-1] + in_pitch + GUARD, CANARY, np.uint8)
        for i, (y, uv, a) in enumerate(planes):
            for plane, off, stride, rows in ((y, 0, self.sy, h), (uv, c_off, self.sc, h // 2), (a, a_off, self.sa, h)):
                if plane is not None:
                    host[self.in_off[i] + off:self.in_off[i] + off + stride * rows].reshape(rows, stride)[:, :w] = plane
        self.d_in = rig.DeviceBuffer(rig.ctx, host.size, placement_tries=1)
        rig.upload(self.d_in.ptr, host)
        self.out_bytes = self.out_off[-1] + out_pitch + GUARD
        self.d_out = rig.DeviceBuffer(rig.ctx, self.out_bytes, placement_tries=1)
        self.frames = (Frame * self.n)(*[Frame(self.d_in.ptr + o, self.sy, self.d_in.ptr + o + c_off, self.sc, w, h, MATRIX, transfer) for o in self.in_off])
        self.alphas = (Frame * self.n)(*[Frame(self.d_in.ptr + o + a_off, self.sa, self.d_in.ptr + o + c_off, self.sc, w, h, MATRIX, LINEAR)
                                         for o in self.in_off]) if has_alpha else None
        self.surfs = (Surface * self.n)(*[Surface(self.d_out.ptr + o, self.so, self.ow, self.oh, fmt, 0) for o in self.out_off])
        self.fill(None)

    def fill(self, backgrounds):
        """The target slab: the canary everywhere, then background i (oh, ow, 4 bytes) in the pixels of slot i."""
        self.before = np.full(self.out_bytes, CANARY, np.uint8)
        for i, bg in enumerate(backgrounds or []):
            self._pixels(self.before, i)[...] = np.asarray(bg, np.uint8).reshape(self.oh, self.px * self.ow)
        self.rig.upload(self.d_out.ptr, self.before)

    def _pixels(self, slab, i):
        o = self.out_off[i]
        return slab[o:o + self.so * self.oh].reshape(self.oh, self.so)[:, :self.px * self.ow]

    def decode_batch(self, dec, stream=None, wait=1):
        return self.rig.lib.bt709hip_decode_batch(dec, self.n, self.frames, self.alphas, self.surfs, stream, wait)

    def decode_one(self, dec, i=0, stream=None, wait=1):
        alpha = C.byref(self.alphas[i]) if self.alphas is not None else None
        return self.rig.lib.bt709hip_decode(dec, C.byref(self.frames[i]), alpha, C.byref(self.surfs[i]), self.w, self.h, stream, wait)

    def collect(self, label=""):
        """-> the pixels of every slot [(oh, ow, 4)]; every byte outside them must be what it was."""
        raw = self.rig.download(self.d_out.ptr, self.out_bytes)
        outside = np.ones(raw.size, bool)
        got = []
        for i in range(self.n):
            got.append(self._pixels(raw, i).reshape(self.oh, self.ow, self.px).copy())
            self._pixels(outside, i)[...] = False
        stray = np.flatnonzero(outside & (raw != self.before))
        assert stray.size == 0, "%s: %d bytes written outside the pixels, first at slab offset %d" % (label, stray.size, stray[0])
        return got

    def untouched(self):
        return np.array_equal(self.rig.download(self.d_out.ptr, self.out_bytes), self.before)

    def free(self):
        self.d_in.free()
        self.d_out.free()


def random_planes(w, h, seed, n=1, alpha=True):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8),
             rng.integers(0, 256, (h, w), dtype=np.uint8) if alpha else None) for _ in range(n)]


def random_backgrounds(w, h, seed, n=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(n)]


def assert_equal(got, want, label):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, x, c = bad[0]
        raise AssertionError("%s: differs first at row %d, column %d, channel %s (got %d, want %d); %d of %d pixels differ"
                             % (label, r, x, "BGRA"[c], got[r, x, c], want[r, x, c], int((got != want).any(axis=2).sum()), got.shape[0] * got.shape[1]))


# ------------------------------------------------------------------ every colour

class Colours:
    """gpu_helpers.exhaustive_frame() and what it decodes to.  image(oracle, gamma): (4096, 4096, 4) B, G, R, 0xFF -- the oracle's
    decode_table indexed by the frame's own triples -- built on first use, then shared and never written."""

    def __init__(self):
        import gpu_helpers  # numpy only until context() is called
        self.y, self.c = gpu_helpers.exhaustive_frame()
        self.blocks = rc.blocks_of(self.y, self.c)  # per-pixel Y, Cb, Cr
        self._image = {}

    def image(self, oracle, gamma):
        if gamma not in self._image:
            img = rc.table_image(oracle.decode_table(gamma), *self.blocks).reshape(self.y.shape[0], self.y.shape[1], 4)
            img.setflags(write=False)
            self._image[gamma] = img
        return self._image[gamma]

    def assert_image(self, got, want, label):
        """got, want: (4096, 4096, 4).  The message names the first triple that differs."""
        if np.array_equal(got, want):
            return
        r, x, ch = np.argwhere(got != want)[0]
        Y, Cb, Cr = (int(a[r, x]) for a in self.blocks)
        raise AssertionError("%s: (Y, Cb, Cr) = (%d, %d, %d) channel %s: got %d, want %d; %d bytes differ"
                             % (label, Y, Cb, Cr, "BGRA"[ch], got[r, x, ch], want[r, x, ch], int((got != want).sum())))


def alpha_ramp(h, w):
    """An alpha plane with every code in every position of a 2x2 block: the 256-entry ramp along x, shifted by one per ROW PAIR.
    (A shift of one per row would not do: the code's parity would be that of x + row, which the position fixes.)"""
    return ((np.arange(w)[None, :] + (np.arange(h)[:, None] >> 1)) & 255).astype(np.uint8)


def alpha_ramp_coverage(a):
    """-> (4, 256) bool: [2 * (row & 1) + (column & 1), code] occurs in `a`."""
    seen = np.zeros((4, 256), bool)
    for pos in range(4):
        seen[pos, np.unique(a[pos >> 1::2, pos & 1::2])] = True
    return seen


# ------------------------------------------------------------------ +unconvert:, every word

UNCONVERT_LAYOUTS = {"vec": (4096, 4096), "per-pixel": (4094, 4100)}  # (width, height); 4094 = 2 (mod 4), 4094 x 4100 >= 2^24


def unconvert_words(w, h):
    """(h, w) packed 4:4:4 words Y | Cb << 8 | Cr << 16: word i is i & 0xFFFFFF, so every triple occurs; byte 3 -- the slot
    unconvertSoftware leaves to alpha -- is the row's low byte, so it takes every value and never the same one down a column."""
    i = np.arange(w * h, dtype=np.uint32).reshape(h, w)
    return (i & np.uint32(0xFFFFFF)) | ((np.arange(h, dtype=np.uint32) & np.uint32(0xFF)) << np.uint32(24))[:, None]


def unconvert_expected(table, words):
    """oracle.decode_table(gamma) -> the words R << 16 | G << 8 | B (alpha byte 0: the decoder's alpha fill) of `words`."""
    idx = ((words & 0xFF) << 16) | (words & 0xFF00) | ((words >> 16) & 0xFF)
    rgb = table.reshape(-1, 3)[idx.reshape(-1)].astype(np.uint32)
    return ((rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]).reshape(words.shape)


# ------------------------------------------------------------------ general-path launch shapes

GRID_MULT = 2  # BT709HIP_CTX_OPT_GRID_MULT at its default


def grid_x_for(compute_units, row_pairs, frames, grid_mult=GRID_MULT):
    """The shim's grid_x_for: workgroups per frame of a general-path launch (grid.x; grid.y = frames)."""
    per_frame = max(1, compute_units * 8 * grid_mult // max(frames, 1))
    return min(row_pairs, per_frame)


def _strided_rows(per_frame, extra):
    """2 * per_frame + extra row pairs: three trips of the grid-stride loop, the last one ragged.  Where `extra` is a multiple of
    per_frame (5 workgroups per frame: a part of 10 to 26 compute units, depending on the batch) one more row pair keeps the
    last trip ragged; with ONE workgroup per frame no trip can be ragged and the loop simply takes that many trips."""
    rows = 2 * per_frame + extra
    return rows + 1 if per_frame > 1 and rows % per_frame == 0 else rows


# name -> (frames, spacing, step_pad, alpha decoder, composite over)
LAUNCH_CASES = {
    "one-frame": (1, "even", (0, 0), False, None),
    "table-32": (32, "table", (0, 0), False, None),
    "step-40": (40, "even", (1, 4), False, None),
    "step-40-alpha": (40, "even", (1, 4), True, None),
    "table-32-over": (32, "table", (0, 0), True, "destination"),
    "table-32-over-colour": (32, "table", (0, 0), True, "colour"),
    "bands-72": (72, "even", (1, 4), False, None),
}
LAUNCH_WIDTH = 6  # one lane column


def launch_case(name, compute_units):
    """-> dict(frames, spacing, step_pad, alpha, over, per_frame, row_pairs, grid) of the case on a part of that many CUs."""
    n, spacing, step_pad, alpha, over = LAUNCH_CASES[name]
    G = compute_units * 8 * GRID_MULT
    per_frame = max(1, G // n)
    row_pairs = _strided_rows(per_frame, 3 if n == 1 else 5)
    return dict(frames=n, spacing=spacing, step_pad=step_pad, alpha=alpha, over=over, per_frame=per_frame, row_pairs=row_pairs,
                grid=(grid_x_for(compute_units, row_pairs, n), n, 1))
