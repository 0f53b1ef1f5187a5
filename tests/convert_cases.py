"""Helpers of tests/test_convert_gpu.py: layouts of pictures and outputs in device slabs, the fast-kernel
predicates restated, expected slabs from the oracle, and the harness that makes ONE bt709hip_encode_batch call under
BT709HIP_CTX_OPT_ENCODE_CONVERT over canary-filled slabs and reads the slabs back whole.

Expected values come from oracle.convert_packed, oracle.packed_to_nv12 and straight_alpha_cases.premultiply only."""
import ctypes as C

import numpy as np

import encoder_cases as ec

OPT, OFF, PACKED, POINT = 10, 0, 1, 2
NV12, I420 = 0, 1
GAMMA_APPLE, GAMMA_SRGB, GAMMA_LINEAR, GAMMA_ITU709 = 0, 1, 2, 3
GAMMAS = (GAMMA_APPLE, GAMMA_SRGB, GAMMA_LINEAR, GAMMA_ITU709)
GUARD, FILL = ec.GUARD, ec.FILL


class Layout:
    """n pictures of w x h: byte offsets of each picture's BGRA rows in the input slab, of its words (PACKED) or Y plane (POINT)
    in the first output slab and of its chroma in the second (POINT: a CbCr plane, or U with V (h/2) x sc bytes behind it).
    Offsets may descend (a negative step)."""

    def __init__(self, mode, w, h, strides, in_off, y_off, c_off=None, chroma=NV12):
        self.mode, self.w, self.h, self.chroma = mode, w, h, chroma
        self.sb, self.sy, self.sc = strides
        self.in_off, self.y_off = list(in_off), list(y_off)
        self.n = len(self.in_off)
        self.c_off = list(c_off) if c_off is not None else [0] * self.n
        self.y_px = 4 if mode == PACKED else 1
        self.in_span = (h - 1) * self.sb + 4 * w
        self.y_span = (h - 1) * self.sy + self.y_px * w
        self.c_rows, self.c_width = (h, w // 2) if chroma == I420 else (h // 2, w)  # U's rows then V's, or CbCr's
        self.c_span = (self.c_rows - 1) * self.sc + self.c_width
        self.in_bytes = max(self.in_off) + self.in_span + GUARD
        self.y_bytes = max(self.y_off) + self.y_span + GUARD
        self.c_bytes = max(self.c_off) + self.c_span + GUARD if mode == POINT else 0
        spans = [(self.in_off, self.in_span), (self.y_off, self.y_span)] + ([(self.c_off, self.c_span)] if mode == POINT else [])
        for offs, span in spans:
            o = sorted(offs)
            assert o[0] >= GUARD and all(b - a >= span for a, b in zip(o, o[1:])), "pictures overlap or leave no guard band"

    def uniform(self):
        if self.n < 2:
            return False
        steps = lambda o: {b - a for a, b in zip(o, o[1:])}
        return all(len(steps(o)) == 1 for o in (self.in_off, self.y_off) + ((self.c_off,) if self.mode == POINT else ()))

    def fast(self):
        """shim_convert.cpp bt709hip_encode_batch, restated.  (Slab bases are 256-byte aligned: the harness asserts it.)"""
        ok = self.w % 4 == 0 and self.sb % 16 == 0 and all(o % 16 == 0 for o in self.in_off)
        if self.mode == PACKED:
            return ok and self.sy % 16 == 0 and all(o % 16 == 0 for o in self.y_off)
        ca = 2 if self.chroma == I420 else 4
        return ok and self.sy % 4 == 0 and self.sc % ca == 0 and all(o % 4 == 0 for o in self.y_off) and all(o % ca == 0 for o in self.c_off)

    def kernel(self, premultiply=False):
        stem = "convert_bgra_packed444" if self.mode == PACKED else ("convert_bgra_i420" if self.chroma == I420 else "convert_bgra_nv12")
        return stem + ("" if self.fast() else "_blocks") + ("<premul>" if premultiply else "")


def evenly(mode, w, h, n, strides=None, misalign=(0, 0, 0), gaps=(0, 0, 0), descending=False, chroma=NV12):
    """n pictures evenly spaced in each slab (descending: the last picture first in memory -- a negative step)."""
    y_px = 4 if mode == PACKED else 1
    sb, sy, sc = strides or (4 * w, y_px * w, w // 2 if chroma == I420 else w)
    c_rows = h if chroma == I420 else h // 2
    pitch = [h * sb + gaps[0], h * sy + gaps[1], c_rows * sc + gaps[2]]
    order = list(range(n))[::-1] if descending else list(range(n))
    offs = [[GUARD + misalign[j] + k * pitch[j] for k in order] for j in range(3)]
    return Layout(mode, w, h, (sb, sy, sc), offs[0], offs[1], offs[2] if mode == POINT else None, chroma)


def irregular(mode, w, h, n, **kw):
    """The same pictures at spacings that differ from slot to slot: the pointer table."""
    L = evenly(mode, w, h, n, **kw)
    extra = np.cumsum([256 * (1 + (i * i) % 5) for i in range(n)])
    bump = lambda offs: [o + int(extra[i]) for i, o in enumerate(offs)]
    return Layout(mode, w, h, (L.sb, L.sy, L.sc), bump(L.in_off), bump(L.y_off), bump(L.c_off) if mode == POINT else None, L.chroma)


def expected_slabs(L, outputs):
    """outputs(i) -> PACKED: (h, w) uint32 words of slot i; POINT: (y (h, w), cbcr (h/2, w)) as oracle.packed_to_nv12 returns them.
    -> the output slabs as they must read back (the second is empty under PACKED)."""
    ys, cs = np.full(L.y_bytes, FILL, np.uint8), np.full(L.c_bytes, FILL, np.uint8)
    for i in range(L.n):
        if L.mode == PACKED:
            words = np.ascontiguousarray(outputs(i), dtype=np.uint32).reshape(L.h, L.w)
            ec._rows_view(ys, L.y_off[i], L.h, L.sy, 4 * L.w)[:] = words.view(np.uint8).reshape(L.h, 4 * L.w)
            continue
        y, c = outputs(i)
        ec._rows_view(ys, L.y_off[i], L.h, L.sy, L.w)[:] = y
        if L.chroma == I420:
            ec._rows_view(cs, L.c_off[i], L.h // 2, L.sc, L.w // 2)[:] = c[:, 0::2]
            ec._rows_view(cs, L.c_off[i] + (L.h // 2) * L.sc, L.h // 2, L.sc, L.w // 2)[:] = c[:, 1::2]
        else:
            ec._rows_view(cs, L.c_off[i], L.h // 2, L.sc, L.w)[:] = c
    return ys, cs


def describe(L, name, got, want, offs, stride, width):
    diff = np.flatnonzero(got != want)
    if diff.size == 0:
        return None
    p = int(diff[0])
    where = "outside every picture (guard band)"
    for i, o in enumerate(offs):
        if o <= p < o + stride * (L.h if name != "CbCr" else L.h // 2):
            r, col = divmod(p - o, stride)
            where = "slot %d row %d byte %d%s" % (i, r, col, " (row padding)" if col >= width else "")
            break
    return "%s slab: %d bytes differ, first at byte %d = %s: got %d, want %d" % (name, diff.size, p, where, got[p], want[p])


def differences(L, res, outputs):
    want_y, want_c = expected_slabs(L, outputs)
    out = [describe(L, "words" if L.mode == PACKED else "Y", res.y_slab, want_y, L.y_off, L.sy, L.y_px * L.w)]
    if L.mode == POINT:
        out.append(describe(L, "CbCr" if L.chroma == NV12 else "U/V", res.c_slab, want_c, L.c_off, L.sc, L.c_width))
    return [d for d in out if d]


class Harness(ec.Harness):
    """encoder_cases.Harness with the context's converter mode (and chroma layout, premultiply flag and launch knobs) set for the
    call and put back after it, whatever happens: the context is the process's."""

    def convert(self, L, in_slab, gamma, premultiply=False, knobs=()):
        """knobs: ((context option, value), ...) set for the call and back to 0 / the default after it."""
        capi = self.capi
        assert in_slab.size == L.in_bytes
        sizes = (L.in_bytes, L.y_bytes) + ((L.c_bytes,) if L.mode == POINT else ())
        bufs = [self.DeviceBuffer(self.ctx, nb, placement_tries=1) for nb in sizes]
        try:
            assert all(d.ptr % 256 == 0 for d in bufs)
            self._upload(bufs[0].ptr, in_slab)
            for d, nb in zip(bufs[1:], sizes[1:]):
                capi.check(self.lib.bt709hip_memset(self.h, d.ptr, FILL, nb, None))
            capi.check(self.lib.bt709hip_stream_synchronize(self.h, None))
            surfs = (capi.Surface * L.n)(*[capi.Surface(bufs[0].ptr + o, L.sb, L.w, L.h, capi.FORMAT_BGRA8_SRGB, 0) for o in L.in_off])
            if L.mode == PACKED:
                frames = (capi.Frame * L.n)(*[capi.Frame(bufs[1].ptr + o, L.sy, None, 12345, L.w, L.h, 0, 0) for o in L.y_off])
            else:
                frames = (capi.Frame * L.n)(*[capi.Frame(bufs[1].ptr + oy, L.sy, bufs[2].ptr + oc, L.sc, L.w, L.h, 0, 0) for oy, oc in zip(L.y_off, L.c_off)])
            options = [(OPT, L.mode, OFF), (capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, L.chroma, NV12), (capi.CTX_OPT_ENCODE_PREMULTIPLY, int(premultiply), 0)]
            options += [(o, v, 1 if o == capi.CTX_OPT_XCD_BANDS else 0) for o, v in knobs]
            try:
                for o, v, _ in options:
                    capi.check(self.lib.bt709hip_context_set_option(self.h, o, v))
                capi.check(self.lib.bt709hip_encode_batch(self.h, L.n, surfs, frames, GAMMA_SRGB, gamma, None, 1), "bt709hip_encode_batch")
            finally:
                for o, _, back in options:
                    capi.check(self.lib.bt709hip_context_set_option(self.h, o, back))
            kernel = self.lib.bt709hip_last_kernel_name().decode()
            info = capi.LaunchInfo()
            capi.check(self.lib.bt709hip_last_launch_info(C.byref(info)))
            c_slab = self._download(bufs[2].ptr, L.c_bytes) if L.mode == POINT else np.zeros(0, np.uint8)
            return ec.Result(self._download(bufs[1].ptr, L.y_bytes), c_slab, kernel, info)
        finally:
            for d in bufs:
                d.free()


def expected_plan(L, bands=True):
    """The plain encoder's plan for the same size and count (encoder_cases.expected_plan) under this layout's predicate."""
    return ec.expected_plan(L.w, L.h, L.n, fast=L.fast(), uniform=L.uniform(), bands=bands)
