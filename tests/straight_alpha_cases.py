"""Straight alpha in and out stated in numpy / plain integers, and the inputs the CPU and the GPU tests share.

    premultiply:    c' = (c * A + 127) // 255
    unpremultiply:  c  = 0 if A == 0 else min(255, (255 * c' + A // 2) // A)

A stays what it is.  CoreGraphics and vImage, which do these steps for the reference, are closed boxes: the definition is the
project's.  Nothing here is taken from the code under test."""
import numpy as np

CTX_OPT_ENCODE_PREMULTIPLY, OPT_UNPREMULTIPLY = 8, 12  # stated here, not taken from the bindings


def premultiply_int(c, a):
    return (c * a + 127) // 255


def unpremultiply_int(c, a):
    return 0 if a == 0 else min(255, (255 * c + a // 2) // a)


def sweep_word(c, a):
    """The word tests/native/straight_alpha_sweep.cpp builds for the pair (c, a): R = c, G = c + 85, B = c + 170 (mod 256)."""
    return (a << 24) | (c << 16) | (((c + 85) & 255) << 8) | ((c + 170) & 255)


def premultiply(words):
    """(A<<24)|(R<<16)|(G<<8)|B words, any shape -> the premultiplied words."""
    w = np.asarray(words, np.uint32)
    a = (w >> 24).astype(np.uint32)
    out = w & np.uint32(0xFF000000)
    for shift in (0, 8, 16):
        c = (w >> shift) & np.uint32(0xFF)
        out = out | (((c * a + np.uint32(127)) // np.uint32(255)) << np.uint32(shift))
    return out.astype(np.uint32)


def unpremultiply(bgra):
    """uint8 (..., 4) B, G, R, A as an alpha decoder writes them -> the same with B, G, R divided by A."""
    px = np.asarray(bgra, np.uint8)
    a = px[..., 3].astype(np.int64)
    out = px.copy()
    safe = np.maximum(a, 1)
    for c in range(3):
        q = np.minimum(255, (255 * px[..., c].astype(np.int64) + a // 2) // safe)
        out[..., c] = np.where(a == 0, 0, q)
    return out


# ------------------------------------------------------------------ the encoder's picture: every (c, A) pair

PAIRS_W, PAIRS_H = 1024, 256
_PICTURE = []


def every_pair_picture():
    """1024 x 256 words.  Row y has A = y.  Along a row each of R, G, B runs through 0..255 four times, the ramp moved on by one
    every 256 columns -- so every value sits in each of the four pixel positions of a quad -- with its own phase per channel and
    moved on by one per row; every value therefore meets every A, in the top rows (A even) and the bottom rows (A odd) of blocks.
    Computed once and shared read-only."""
    if not _PICTURE:
        x = np.arange(PAIRS_W, dtype=np.uint32)[None, :]
        y = np.arange(PAIRS_H, dtype=np.uint32)[:, None]
        ramp = x + x // 256 + y
        r, g, b = (ramp & 255), ((ramp + 85) & 255), ((ramp + 170) & 255)
        words = ((y << 24) | (r << 16) | (g << 8) | b).astype(np.uint32)
        words.setflags(write=False)
        _PICTURE.append(words)
    return _PICTURE[0]


def crop(w, h, row0=0):
    """w x h words of every_pair_picture()'s content from row `row0` on (rows and columns wrap round)."""
    pic = every_pair_picture()
    rows = (row0 + np.arange(h)) % PAIRS_H
    cols = np.arange(w) % PAIRS_W
    return np.ascontiguousarray(pic[rows][:, cols])


def check_every_pair_picture():
    """The coverage the picture claims, by counting: every (value, A) for each channel, and every value in each quad position."""
    pic = every_pair_picture()
    a = pic >> 24
    assert (a == np.arange(PAIRS_H, dtype=np.uint32)[:, None]).all()
    for shift in (0, 8, 16):
        c = (pic >> shift) & 255
        seen = np.zeros((256, 256), bool)
        seen[c, a] = True
        assert seen.all()
        for pos in range(4):
            assert np.unique(c[0, pos::4]).size == 256 and np.unique(c[1, pos::4]).size == 256


# ------------------------------------------------------------------ the decoder's frames: every pair that can occur

def decoder_planes(triples, rows=256):
    """Column block k (2 pixels wide) carries covering triple k in every row; row r of the alpha plane holds the byte r.
    -> (y (rows, 2n), cbcr (rows/2, 2n), alpha (rows, 2n)), 2n rounded up to a multiple of 4 by repeating the last triple."""
    t = np.asarray(triples, np.uint8)
    if len(t) % 2:
        t = np.concatenate([t, t[-1:]])
    n = len(t)
    y = np.broadcast_to(np.repeat(t[:, 0], 2)[None, :], (rows, 2 * n)).copy()
    uv = np.broadcast_to(np.stack([t[:, 1], t[:, 2]], 1).reshape(1, 2 * n), (rows // 2, 2 * n)).copy()
    a = np.broadcast_to(np.arange(rows, dtype=np.uint8)[:, None], (rows, 2 * n)).copy()
    return y, uv, a


def bands_picture(w=64, h=32):
    """A straight-alpha picture whose rows fall into bands of A = 0, 1, 128, 254, 255 (the last band takes the remainder), colour
    from a seeded generator."""
    rng = np.random.default_rng(39)
    words = rng.integers(0, 1 << 24, (h, w), dtype=np.uint32)
    alphas = np.array([0, 1, 128, 254, 255], np.uint32)
    band = np.minimum(np.arange(h) // (h // 5), 4)
    return (words | (alphas[band][:, None] << 24)).astype(np.uint32)
