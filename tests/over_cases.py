"""The composite-over definition (BT709HIP_OPT_COMPOSITE_OVER) in numpy, and the inputs the CPU and the GPU tests
share.  The reference leaves the blend to the OS compositor, so the definition is the project's: the two-pass equivalent --
decode to the 8-bit word, then blend source-over in linear light -- composed of the reference's own inlines (byteNorm and
sRGB_nonLinearNormToLinear, sRGB.h:18-60, as the oracle's lin[] table; the LINEAR-mode composite as its 255 thresholds)."""
import numpy as np

OVER_OFF, OVER_DESTINATION = -1, -2


def colour_word(colour):
    """The background pixel of colour mode: sRGB bytes R<<16 | G<<8 | B, opaque."""
    return np.array([colour & 0xFF, (colour >> 8) & 0xFF, (colour >> 16) & 0xFF, 255], np.uint8)


def composite_over(src_bgra, dst_bgra_or_colour, lin, thresholds):
    """src_bgra: uint8 (..., 4) B, G, R, A words as bt709hip_decode writes them for an alpha decoder (premultiplied colour).
    dst_bgra_or_colour: an array of the same shape (what the target held), or an int R<<16 | G<<8 | B.
    lin = Oracle.to_linear_table(GAMMA_SRGB), thresholds = Oracle.thresholds(GAMMA_LINEAR).  Float32 throughout, every
    operation rounded on its own:
        k     = float(255 - A_s) * (1.0f / 255.0f)
        v_c   = min(1.0f, lin[s_c] + k * lin[d_c])
        out_c = number of thresholds <= v_c
        out_A = A_s + ((255 - A_s) * A_d + 127) / 255          (integer)"""
    src = np.asarray(src_bgra, np.uint8)
    assert src.shape[-1] == 4
    if np.ndim(dst_bgra_or_colour) == 0:
        dst = np.broadcast_to(colour_word(int(dst_bgra_or_colour)), src.shape)
    else:
        dst = np.asarray(dst_bgra_or_colour, np.uint8)
        assert dst.shape == src.shape
    lin = np.asarray(lin, np.float32)
    thresholds = np.asarray(thresholds, np.float32)
    assert lin.shape == (256,) and thresholds.shape == (255,)
    a_s = src[..., 3].astype(np.int32)
    k = (255 - a_s).astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    out = np.empty(src.shape, np.uint8)
    for c in range(3):
        product = k * lin[dst[..., c]]          # float32 * float32, rounded
        v = np.minimum(np.float32(1.0), lin[src[..., c]] + product)
        assert v.dtype == np.float32
        out[..., c] = np.searchsorted(thresholds, v, side="right")
    out[..., 3] = a_s + ((255 - a_s) * dst[..., 3].astype(np.int32) + 127) // 255
    return out


def expected_source(oracle, y, uv, a):
    """The word the plain alpha decode writes: (H, W, 4) B, G, R, A."""
    from oracle_lib import GAMMA_SRGB
    h, w = y.shape
    return oracle.decode_nv12(GAMMA_SRGB, np.ascontiguousarray(y), np.ascontiguousarray(uv), alpha=np.ascontiguousarray(a)).reshape(h, w, 4)


def tables(oracle):
    from oracle_lib import GAMMA_LINEAR, GAMMA_SRGB
    return oracle.to_linear_table(GAMMA_SRGB), oracle.thresholds(GAMMA_LINEAR)


def covering_triples(oracle):
    """(Y, Cb, Cr) triples, at most 768, whose alpha-decoder words between them take every byte value 0..255 in each of R, G
    and B.  Greedy over a fixed candidate list: the grey ramp reaches the bytes the luma scale lands on, saturated chroma pushes
    single channels to the values it skips.  Returns (triples (n, 3) uint8, their decoded (n, 4) BGRA words)."""
    ys = np.arange(256, dtype=np.uint8)
    cand = [np.stack([ys, np.full(256, cb, np.uint8), np.full(256, cr, np.uint8)], 1)
            for cb, cr in ((128, 128), (127, 129), (129, 127), (120, 136), (136, 120), (100, 156), (156, 100), (64, 192), (192, 64),
                           (128, 100), (128, 156), (100, 128), (156, 128), (110, 110), (146, 146), (90, 90), (166, 166))]
    cand = np.concatenate(cand)
    words = decode_triples(oracle, cand)
    missing = [set(range(256)) for _ in range(3)]
    keep = []
    for i, wd in enumerate(words):
        hit = [c for c in range(3) if int(wd[c]) in missing[c]]
        if hit:
            keep.append(i)
            for c in hit:
                missing[c].discard(int(wd[c]))
        if not any(missing):
            break
    return cand[keep], words[keep]


def decode_triples(oracle, triples):
    """The opaque-alpha words of (n, 3) Y, Cb, Cr triples: each triple fills one 2x2 block of a two-row frame."""
    n = len(triples)
    y = np.repeat(triples[:, 0], 2)[None, :].repeat(2, 0)
    uv = np.stack([triples[:, 1], triples[:, 2]], 1).reshape(1, 2 * n)
    a = np.full((2, 2 * n), 235, np.uint8)
    return expected_source(oracle, y, uv, a)[0, 0::2]


def channel_table(lin, thresholds):
    """out_c as a function of (A_s, d_c, s_c) and out_A as a function of (A_s, A_d), tabulated BY composite_over (the
    exhaustive sweeps index these instead of running the definition over tens of millions of pixels twice).  composite_over
    treats B, G and R alike, so one call carries three background bytes per pixel, one in each channel: T[A_s, d, s] (256^3
    uint8) and TA[A_s, A_d]."""
    a, s = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    src = np.stack([s, s, s, a], -1)
    table = np.empty((256, 256, 256), np.uint8)
    for d0 in range(0, 256, 3):
        d = [min(d0 + c, 255) for c in range(3)]
        dst = np.broadcast_to(np.array(d + [255], np.uint8), src.shape)
        out = composite_over(src, dst, lin, thresholds)
        for c in range(3):
            table[:, d[c], :] = out[..., c]
    a_s, a_d = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    zero = np.zeros_like(a_s)
    alpha = composite_over(np.stack([zero, zero, zero, a_s], -1), np.stack([zero, zero, zero, a_d], -1), lin, thresholds)[..., 3]
    return table, alpha
