"""What bt709hip_encode[_batch] must write under BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA: two frames per RGBA16Float
surface.  The expectation is never the code under test:

    colour frame = encode_half_cases.Expect.planes(t, go)                       the option-0 half encode (3.12)
    alpha frame  = encode_half_cases.Expect.planes(grey(t[..., 3]), LINEAR)     3.12 under (LINEAR, LINEAR) of the surface whose
                                                                               R, G and B are replaced by its A

PairPlan is encode_half_cases.Plan with two more arenas in the same output slab (the alpha Y and the alpha chroma planes), so that
all five planes of a call are compared whole, canaries included.  Shared by tests/test_encode_half_alpha_cpu.py and
tests/test_encode_half_alpha_gpu.py."""
import json
import os

import numpy as np

import encode_half_cases as hc
from oracle_lib import GAMMA_LINEAR

OPT_HALF_WITH_ALPHA = 16     # stated here, not taken from the bindings
NV12, I420 = hc.NV12, hc.I420
FILL = hc.FILL
ALPHA_PLANES = ("ay", "ac")
LUMA = np.array(json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alpha_luma.json")))["luma"], np.uint8)


def grey(a):
    """(H, W) uint16 half codes -> (H, W, 4) texels whose R, G, B (and A) are that code"""
    a = np.asarray(a, np.uint16)
    return np.repeat(a[..., None], 4, axis=-1)


def alpha_planes(expect, texels):
    """texels (H, W, 4) -> (y, cbcr) of the alpha frame, by the definition"""
    return expect.planes(grey(np.asarray(texels, np.uint16)[..., 3]), GAMMA_LINEAR)


def alpha_code(codes):
    """(int)round(sat(a) * 255.0f) of half codes, in float32 as the reference's BT709_from_linear(v, Linear): numpy restatement used
    by the CPU tests to NAME the definition's closed form; Expect.planes is the authority it is held against."""
    v = hc.saturate(codes) * np.float32(255.0)
    assert v.dtype == np.float32
    return np.floor(v.astype(np.float64) + 0.5).astype(np.uint8)  # round half away from zero of a non-negative value


def kernel_name(layout, fast):
    return "encode_rgba16f_alpha_" + ("i420" if layout == I420 else "nv12") + ("" if fast else "_blocks")


class PairPlan(hc.Plan):
    """pitches: (in, y, c, ay, ac); shift / steps take the keys "in", "y", "c", "ay", "ac"."""

    def __init__(self, w, h, n=1, layout=NV12, alpha_chroma=True, pitches=None, shift=None, steps=None, spacing="even"):
        super().__init__(w, h, n, layout, pitches=pitches[:3] if pitches else None, shift=shift, steps=steps, spacing=spacing)
        self.alpha_chroma = alpha_chroma
        self.colour_bytes = self.out_bytes  # the colour frames' arenas end here
        cw = w // 2 if layout == I420 else w
        self.pitch["ay"], self.pitch["ac"] = pitches[3:] if pitches else (w, cw)
        pc = self.pitch["ac"]
        self.span["ay"] = (h - 1) * self.pitch["ay"] + w
        self.span["ac"] = (h // 2) * pc + (h // 2 - 1) * pc + w // 2 if layout == I420 else (h // 2 - 1) * pc + w
        shift, steps = shift or {}, steps or {}
        cursor = self.out_bytes
        for k in ALPHA_PLANES:
            step = steps.get(k, (self.span[k] + 255) // 256 * 256 + 256)
            assert abs(step) >= self.span[k], "pairs overlap"
            rel = [i * step if step > 0 else (n - 1 - i) * -step for i in range(n)]
            if spacing == "table":
                extra = np.cumsum([256 * ((i * i + 2) % 5) for i in range(n)])
                rel = [r + int(e) for r, e in zip(rel, extra)]
            base = cursor + self.GUARD + shift.get(k, 0)
            self.off[k] = [base + r for r in rel]
            cursor = (base + max(rel) + self.span[k] + self.GUARD + 255) // 256 * 256
        self.out_bytes = cursor

    def uniform(self):
        return all(len({b - a for a, b in zip(o, o[1:])}) <= 1 for o in self.off.values())

    def _chroma(self, slab, k, i, c):
        h2 = self.h // 2
        if self.layout == I420:
            self.rows(slab, k, i, h2, self.w // 2)[:] = c[:, 0::2]
            self.rows(slab, k, i, h2, self.w // 2, h2 * self.pitch[k])[:] = c[:, 1::2]
        else:
            self.rows(slab, k, i, h2, self.w)[:] = c

    def expected(self, colour, alpha):
        """colour[i], alpha[i] = (y, cbcr) NV12 of pair i -> the output slab as it must read back"""
        slab = np.full(self.out_bytes, FILL, np.uint8)
        for i in range(self.n):
            y, c = colour[i]
            self.rows(slab, "y", i, self.h, self.w)[:] = y
            self._chroma(slab, "c", i, c)
            y, c = alpha[i]
            self.rows(slab, "ay", i, self.h, self.w)[:] = y
            if self.alpha_chroma:
                self._chroma(slab, "ac", i, c)
        return slab

    def describe(self, got, want):
        diff = np.flatnonzero(got != want)
        if diff.size == 0:
            return None
        p = int(diff[0])
        where = "outside every plane (guard bytes or row padding)"
        for k in ("y", "c") + ALPHA_PLANES:
            for i, o in enumerate(self.off[k]):
                if o <= p < o + self.span[k]:
                    where = "plane %s of pair %d, byte %d of it (pitch %d)" % (k, i, p - o, self.pitch[k])
        return "%d bytes differ, first at %d = %s: got %d, want %d" % (diff.size, p, where, got[p], want[p])
