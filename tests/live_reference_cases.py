"""Inputs of the live-reference tests of tests/test_oracle_golden.py (test_live_reference_pixels,
test_live_reference_encode_frame, test_pass2_oracle_equals_reference_live) and the outputs an implementation
(the oracle, or the reference's own headers through oracle_lib.Reference) gives for them.
tests/golden/live_reference.npz records the reference's outputs (tests/golden/make_golden.py --live-reference),
so the tests hold the oracle to them on any machine; where the reference library has been built they compare
with it live as well.  Inputs are seeded PRNG values (numpy PCG64: the same everywhere)."""
import numpy as np

GAMMAS = (0, 1, 2, 3)
ENCODE_GAMMAS = ((1, 0), (1, 1), (0, 0), (2, 2))  # (input gamma, output gamma) of encode_nv12


def pixel_outputs(impl):
    """2000 (Y, Cb, Cr) decodes and 2000 (R, G, B) encodes per gamma mode, one PRNG stream (seed 1)."""
    rng = np.random.default_rng(1)
    out = {}
    for gamma in GAMMAS:
        ycc = rng.integers(0, 256, (2000, 3))
        rgb = rng.integers(0, 256, (2000, 3))
        out["decode_pixel/g%d" % gamma] = np.array([impl.decode_pixel(gamma, int(Y), int(Cb), int(Cr)) for Y, Cb, Cr in ycc], np.int32)
        out["encode_pixel/g%d" % gamma] = np.array([impl.encode_pixel(gamma, int(R), int(G), int(B)) for R, G, B in rgb], np.int32)
    return out


def encode_frame_outputs(impl):
    """One seeded 32x16 BGRA frame (seed 2) through encode_nv12 in four gamma pairings."""
    bgra = np.random.default_rng(2).integers(0, 1 << 24, 32 * 16, dtype=np.uint32)
    out = {}
    for ig, og in ENCODE_GAMMAS:
        y, uv = impl.encode_nv12(bgra, 32, 16, ig, og)
        out["encode_nv12/y/%d-%d" % (ig, og)], out["encode_nv12/uv/%d-%d" % (ig, og)] = y, uv
    return out


def pass2_outputs(impl):
    """12 seeded frames of random size and gamma (seed 77; every third with an alpha plane): the fused 2:1 decode and an
    any-ratio decode to a random output size."""
    rng = np.random.default_rng(77)
    out = {}
    for case in range(12):
        w, h = 4 * int(rng.integers(1, 40)), 4 * int(rng.integers(1, 12))
        gamma = int(rng.integers(0, 4))
        y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        c = rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
        a = rng.integers(0, 256, (h, w), dtype=np.uint8) if case % 3 == 0 else None
        out["pass2/half/%d" % case] = impl.decode_nv12_half(gamma, y, c, alpha=a)
        ow, oh = int(rng.integers(1, 2 * w)), int(rng.integers(1, 2 * h))
        out["pass2/scaled/%d" % case] = impl.decode_nv12_scaled(gamma, y, c, ow, oh, alpha=a)
    return out


def npz_key(key):
    return key.replace("/", "_")
