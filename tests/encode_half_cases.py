"""What bt709hip_encode[_batch] must write for RGBA16Float input (BT709HIP_CTX_OPT_ENCODE_HALF_INPUT), composed of
oracle calls and float32 numpy sums -- never of the code under test:

    v[i][c]    = sat(float(h[i][c]))                         NaN -> 0, v < 0 -> 0, v > 1 -> 1
    byte[i][c] = F(v) = bt709o_quantize(curve(v))            curve: bt709o_linear_to_srgb / bt709o_linear_to_apple196 / identity
    Y[i]       = Y of oracle.encode_pixel(1, byte[i][R, G, B])              the pure byte matrix
    ave[c]     = (((v0 + v1) + v2) + v3) / 4.0f              float32, in this order
    (Cb, Cr)   = Cb, Cr of oracle.encode_pixel(1, F(ave[R, G, B]))

For a flat block (four equal texels) the sums are exact, ave = v, and the block is the (LINEAR, LINEAR) encode of the BGRA8 twin
whose bytes are F(v): twin_words().  Shared by tests/test_encode_half_cpu.py and tests/test_encode_half_gpu.py."""
import numpy as np

from oracle_lib import GAMMA_APPLE, GAMMA_LINEAR, GAMMA_SRGB

OPT_HALF_INPUT = 14          # stated here, not taken from the bindings
FORMAT_RGBA16F = 1
ONE = 0x3C00                 # half(1.0); codes 0 .. ONE are the 15361 halves in [0, 1]
OUT_GAMMAS = (GAMMA_APPLE, GAMMA_SRGB, GAMMA_LINEAR)
NV12, I420 = 0, 1
FILL = 0x5A


def saturate(codes):
    """uint16 half codes -> float32 in [0, 1]: exact conversion, NaN -> 0, negative (and -0) -> 0, above 1 (and +inf) -> 1."""
    v = np.asarray(codes, np.uint16).view(np.float16).astype(np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, np.float32(0), np.float32(1)).astype(np.float32) + np.float32(0)  # + 0: -0 -> +0


def saturated_code(codes):
    """The half code in 0 .. ONE of the saturated value (every half in [0, 1] is its own float)."""
    return saturate(codes).astype(np.float16).view(np.uint16)


class Expect:
    """The composition, with the oracle's scalars applied to the distinct values of an array."""

    def __init__(self, oracle):
        self.oracle, self._tables, self._matrix = oracle, {}, {}

    def curve_byte(self, out_gamma, v):
        L = self.oracle.lib
        v = float(np.float32(v))
        if out_gamma == GAMMA_SRGB:
            v = L.bt709o_linear_to_srgb(v)
        elif out_gamma == GAMMA_APPLE:
            v = L.bt709o_linear_to_apple196(v)
        else:
            assert out_gamma == GAMMA_LINEAR
        return L.bt709o_quantize(v)

    def from_linear(self, out_gamma, values):
        """F of a float32 array in [0, 1] -> uint8"""
        values = np.asarray(values, np.float32)
        uniq, inverse = np.unique(values.reshape(-1), return_inverse=True)
        b = np.array([self.curve_byte(out_gamma, v) for v in uniq], np.int64)
        assert b.min() >= 0 and b.max() <= 255
        return b.astype(np.uint8)[inverse].reshape(values.shape)

    def code_table(self, out_gamma):
        """(ONE + 1,) uint8: F of every half in [0, 1], by code"""
        if out_gamma not in self._tables:
            self._tables[out_gamma] = self.from_linear(out_gamma, saturate(np.arange(ONE + 1, dtype=np.uint16)))
        return self._tables[out_gamma]

    def matrix(self, rgb):
        """(..., 3) uint8 R, G, B -> (..., 3) uint8 Y, Cb, Cr: oracle.encode_pixel(1, R, G, B) of the distinct triples"""
        rgb = np.asarray(rgb, np.uint8)
        key = (rgb[..., 0].astype(np.uint32) << 16) | (rgb[..., 1].astype(np.uint32) << 8) | rgb[..., 2]
        uniq, inverse = np.unique(key.reshape(-1), return_inverse=True)
        out = np.empty((uniq.size, 3), np.uint8)
        for i, k in enumerate(uniq.tolist()):
            if k not in self._matrix:
                self._matrix[k] = self.oracle.encode_pixel(GAMMA_SRGB, k >> 16, (k >> 8) & 255, k & 255)
            out[i] = self._matrix[k]
        return out[inverse].reshape(rgb.shape)

    def planes(self, texels, out_gamma):
        """texels: (H, W, 4) uint16 half codes R, G, B, A -> (y (H, W), cbcr (H/2, W)) uint8, NV12"""
        t = np.asarray(texels, np.uint16)
        h, w = t.shape[:2]
        rgb = t[..., :3]
        y = self.matrix(self.code_table(out_gamma)[saturated_code(rgb)])[..., 0]
        v = saturate(rgb)
        ave = (((v[0::2, 0::2] + v[0::2, 1::2]) + v[1::2, 0::2]) + v[1::2, 1::2]) / np.float32(4.0)  # TL, TR, BL, BR
        assert ave.dtype == np.float32
        c = self.matrix(self.from_linear(out_gamma, ave))
        cbcr = np.empty((h // 2, w), np.uint8)
        cbcr[:, 0::2], cbcr[:, 1::2] = c[..., 1], c[..., 2]
        return y, cbcr


def twin_words(rgb_bytes):
    """(..., 3) uint8 R, G, B -> BGRA8 words (A = 255): the picture whose (LINEAR, LINEAR) encode is the half picture's, block by
    flat block"""
    b = np.asarray(rgb_bytes, np.uint32)
    return (np.uint32(255) << 24) | (b[..., 0] << 16) | (b[..., 1] << 8) | b[..., 2]


def representatives(table):
    """table: code_table() -> (lowest, highest) uint16 arrays of 256: the smallest and the largest half code that give byte k"""
    codes = np.arange(table.size)
    lo = np.array([codes[table == k].min() for k in range(256)], np.uint16)
    hi = np.array([codes[table == k].max() for k in range(256)], np.uint16)
    return lo, hi


def split_chroma(cbcr):
    """NV12 chroma rows -> (U, V)"""
    return cbcr[:, 0::2], cbcr[:, 1::2]


SPECIALS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x0400, 0x3BFF, 0x3C00, 0x3C01, 0x7BFF, 0x7C00, 0xFC00, 0x7C01, 0x7E00,
                     0xFE00, 0xFFFF, 0xBC00, 0x7DFF], np.uint16)  # zeros, subnormals, around 1, max, infinities, NaNs, -1


def random_texels(rng, h, w):
    """Halves drawn from [-0.25, 1.25] with the specials sprinkled in (one texel channel in eight); A is noise, too"""
    t = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(np.float16).view(np.uint16)
    mask = rng.random((h, w, 4)) < 0.125
    t[mask] = rng.choice(SPECIALS, int(mask.sum()))
    return t


# ------------------------------------------------------------------ slabs (GPU tests)

class Plan:
    """Where n pictures of w x h live: the texels in an input slab; Y and chroma planes in ONE output slab that is canary-filled
    and compared whole.  pitches: (in, y, c); shift: bytes added to every offset of a plane; steps: byte distance from one
    picture's plane to the next (negative = descending); spacing "table": uneven distances."""
    GUARD = 1024

    def __init__(self, w, h, n=1, layout=NV12, pitches=None, shift=None, steps=None, spacing="even"):
        self.w, self.h, self.n, self.layout = w, h, n, layout
        cw = w // 2 if layout == I420 else w
        self.pitch = dict(zip(("in", "y", "c"), pitches or (8 * w, w, cw)))
        p = self.pitch
        chroma = (h // 2) * p["c"] + (h // 2 - 1) * p["c"] + w // 2 if layout == I420 else (h // 2 - 1) * p["c"] + w
        self.span = {"in": (h - 1) * p["in"] + 8 * w, "y": (h - 1) * p["y"] + w, "c": chroma}
        shift, steps = shift or {}, steps or {}
        self.off, cursor = {}, {"in": 0, "out": 0}
        for k in ("in", "y", "c"):
            slab = "in" if k == "in" else "out"
            step = steps.get(k, (self.span[k] + 255) // 256 * 256 + 256)
            assert abs(step) >= self.span[k], "pictures overlap"
            rel = [i * step if step > 0 else (n - 1 - i) * -step for i in range(n)]
            if spacing == "table":
                extra = np.cumsum([256 * ((i * i) % 5) for i in range(n)])
                rel = [r + int(e) for r, e in zip(rel, extra)]
            base = cursor[slab] + self.GUARD + shift.get(k, 0)
            self.off[k] = [base + r for r in rel]
            cursor[slab] = (base + max(rel) + self.span[k] + self.GUARD + 255) // 256 * 256
        self.in_bytes, self.out_bytes = cursor["in"], cursor["out"]

    def rows(self, slab, k, i, rows, width, plane_offset=0):
        start = self.off[k][i] + plane_offset
        return np.lib.stride_tricks.as_strided(slab[start:], shape=(rows, width), strides=(self.pitch[k], 1))

    def input_slab(self, pictures):
        slab = np.full(self.in_bytes, FILL, np.uint8)
        for i in range(self.n):
            self.rows(slab, "in", i, self.h, 8 * self.w)[:] = np.ascontiguousarray(pictures[i], np.uint16).view(np.uint8).reshape(self.h, 8 * self.w)
        return slab

    def expected(self, planes):
        """planes[i] = (y, cbcr) NV12 of picture i -> the output slab as it must read back"""
        slab = np.full(self.out_bytes, FILL, np.uint8)
        h2 = self.h // 2
        for i in range(self.n):
            y, c = planes[i]
            self.rows(slab, "y", i, self.h, self.w)[:] = y
            if self.layout == I420:
                self.rows(slab, "c", i, h2, self.w // 2)[:] = c[:, 0::2]
                self.rows(slab, "c", i, h2, self.w // 2, h2 * self.pitch["c"])[:] = c[:, 1::2]
            else:
                self.rows(slab, "c", i, h2, self.w)[:] = c
        return slab

    def describe(self, got, want):
        diff = np.flatnonzero(got != want)
        if diff.size == 0:
            return None
        p = int(diff[0])
        where = "outside every plane (guard bytes or row padding)"
        for k in ("y", "c"):
            for i, o in enumerate(self.off[k]):
                if o <= p < o + self.span[k]:
                    where = "plane %s of picture %d, byte %d of it (pitch %d)" % (k, i, p - o, self.pitch[k])
        return "%d bytes differ, first at %d = %s: got %d, want %d" % (diff.size, p, where, got[p], want[p])


def kernel_name(layout, fast):
    return "encode_rgba16f_" + ("i420" if layout == I420 else "nv12") + ("" if fast else "_blocks")
