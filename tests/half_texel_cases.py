"""Cases of pass 2 from an RGBA16Float surface a CALLER filled (tests/test_pass2_texels.py): NumPy + the CPU oracle, nothing else.
bt709hip_render_scaled[_batch] is a public entry point, so a texel may hold any of the 65 536 half codes, not only what pass 1
leaves.  Every image is built from uint16 codes viewed as float16: a NaN's payload travels bit for bit.

  * every_code_image: every code in every channel as flat 2x2 blocks.  A flat block's four-tap sum at exactly 2:1,
    ((h/4 + h/4) + h/4) + h/4, is h without a rounding for every finite half (|h| >= 2^-24, so no product is subnormal), an
    infinity for an infinity and a NaN for a NaN: the block's byte is the saturate + encode of float(h).
  * half_edge_quads: four halves a >= b >= c >= d >= 0 whose sum in the oracle's order lands ON an encode threshold and on the
    float just BELOW it (the nearest reachable sums where the threshold is too fine for halves), by a greedy split of 4 T;
    half_edge_frame lays them out as rescale_arith_cases.bgra_edge_frame does for bytes.
  * wild_image: random finite codes of either sign and any magnitude; the same with infinities and NaNs sprinkled in.
"""
import numpy as np

import rescale_arith_cases as rc

ONE, INF, NEG_ZERO, NEG_INF = 0x3c00, 0x7c00, 0x8000, 0xfc00
FINITE_CODES = np.concatenate([np.arange(0, INF), np.arange(NEG_ZERO, NEG_INF)]).astype(np.uint16)  # 63 488
assert FINITE_CODES.size == 2 * 31 * 1024


def is_nan_code(codes):
    codes = np.asarray(codes).astype(np.uint32)
    return ((codes & 0x7c00) == 0x7c00) & ((codes & 0x03ff) != 0)


def as_halves(codes):
    """uint16 codes (..., 4) -> the float16 image of the same bits."""
    return np.ascontiguousarray(codes, dtype=np.uint16).view(np.float16)


# ------------------------------------------------------------------ every code

def every_code_blocks(transposed=False):
    """(256, 256, 4) uint16: channel k of block i holds code (i + 16384 k) & 0xffff -- every channel sees every code and no two
    channels of a texel hold the same one; block i sits at (row i >> 8, column i & 255), or at the transposed place (so that a
    code's low byte is not tied to its lane)."""
    i = np.arange(65536, dtype=np.uint32).reshape(256, 256)
    if transposed:
        i = i.T
    return ((i[:, :, None] + 16384 * np.arange(4, dtype=np.uint32)[None, None, :]) & 0xffff).astype(np.uint16)


def every_code_image(transposed=False):
    """-> (image (512, 512, 4) float16 of flat 2x2 blocks, to be rendered to 256 x 256; the blocks' codes (256, 256, 4))."""
    codes = every_code_blocks(transposed)
    return as_halves(np.repeat(np.repeat(codes, 2, axis=0), 2, axis=1)), codes


def by_code(out, codes):
    """The oracle's / the kernel's 256 x 256 BGRA output of an every-code image -> (65 536, 4) bytes indexed [code, channel],
    channels in the texel's order R, G, B, A."""
    px = out.reshape(256, 256, 4)[:, :, [2, 1, 0, 3]]
    table = np.full((65536, 4), -1, np.int32)
    for k in range(4):
        table[codes[:, :, k].reshape(-1), k] = px[:, :, k].reshape(-1)
    assert (table >= 0).all()
    return table.astype(np.uint8)


def closed_form_by_code(unit_map):
    """What a channel makes of a flat block of code c, from the definition: `unit_map` (the encode of every code in [0, 1.0],
    0x3c01 entries) on 0 ... 0x3c00, 255 above 1.0 up to and including +inf, 0 for -0, every negative, -inf and every NaN."""
    want = np.zeros(65536, np.uint8)
    want[:ONE + 1] = unit_map
    want[ONE:INF + 1] = 255
    return want


def first_code_difference(got, want, codes):
    """Message naming the code, channel, got and want of the first byte of an every-code output that differs."""
    g, w = got.reshape(256, 256, 4), want.reshape(256, 256, 4)
    r, c, b = np.argwhere(g != w)[0]
    k = (2, 1, 0, 3)[b]  # output byte B, G, R, A -> texel channel
    return "half code 0x%04x in channel %s (block row %d, column %d): got %d, want %d; %d bytes differ" % (
        codes[r, c, k], "RGBA"[k], r, c, g[r, c, b], w[r, c, b], int((g != w).sum()))


# ------------------------------------------------------------------ both sides of every encode threshold, from halves

def half_tap_sum(q):
    """((a/4 + b/4) + c/4) + d/4 in float32, the oracle's order at exactly 2:1; q: (..., 4) uint16 codes."""
    v = as_halves(q).astype(np.float32) * np.float32(0.25)  # exact: a power of two, nothing subnormal
    s = (v[..., 0] + v[..., 1]).astype(np.float32)
    s = (s + v[..., 2]).astype(np.float32)
    return (s + v[..., 3]).astype(np.float32)


def _greedy(total):
    """Greedy split of `total` (a float64 holding an exact dyadic number >= 0): four times the largest half not above the
    remainder.  -> (codes [a, b, c, d], remainder).  Every subtraction is exact (total has at most 26 significant bits above
    2^-36, a half 11)."""
    q, rest = [], np.float64(total)
    for _ in range(4):
        h = np.float16(rest)
        if np.float64(h) > rest:  # rounded up: the half below
            h = np.nextafter(h, np.float16(0))
        q.append(int(h.view(np.uint16)))
        rest = rest - np.float64(h)
    assert rest >= 0
    return q, rest


def half_edge_quads(thresholds):
    """For each of the 255 thresholds T: `upper`, four halves a >= b >= c >= d >= 0 whose sum is T, and `lower`, four whose sum
    is the float just below T.  Halves stop at 2^-24, so a sum of four quarters is a multiple of 2^-26: where 4 T (or four times
    the float below T) has bits under 2^-24 the greedy split leaves a remainder, and the quad is then the smallest reachable sum
    >= T (the split of 4 T - remainder + 2^-24) / the largest reachable sum < T (the split as it is).
    -> dict(upper, lower (255, 4) uint16, up_ulps, lo_ulps (255,) int64: float32 steps from the threshold, 0 = on it / 1 = the
    float just below it), as rescale_arith_cases.edge_search reports them."""
    T = np.asarray(thresholds, np.float32)
    below = np.nextafter(T, np.float32(-np.inf), dtype=np.float32)
    upper, lower = np.zeros((255, 4), np.uint16), np.zeros((255, 4), np.uint16)
    unit = np.float64(2.0) ** -24
    for i in range(255):
        t4 = np.float64(T[i]) * 4.0
        q, rest = _greedy(t4)
        if rest:
            q, rest = _greedy(t4 - rest + unit)
            assert rest == 0
        upper[i] = q
        lower[i], _ = _greedy(np.float64(below[i]) * 4.0)
    for q in (upper, lower):
        v = as_halves(q).astype(np.float32)
        assert (v[:, :-1] >= v[:, 1:]).all() and (v >= 0).all() and (q < INF).all()
    su, sl = half_tap_sum(upper), half_tap_sum(lower)
    assert (su >= T).all() and (sl < T).all()
    bits = lambda a: a.view(np.uint32).astype(np.int64)  # positive floats order as their bit patterns
    return dict(upper=upper, lower=lower, up_ulps=bits(su) - bits(T), lo_ulps=bits(T) - bits(sl))


def half_edge_counts(e):
    """(thresholds hit exactly, hit one float below)."""
    return int((e["up_ulps"] == 0).sum()), int((e["lo_ulps"] == 1).sum())


def _classify(T, quads, i):
    """Side and exactness of probe quadruples AS ORDERED (a permutation may move the float32 sum)."""
    s = half_tap_sum(quads)
    below = np.nextafter(T[i], np.float32(-np.inf), dtype=np.float32)
    return (s >= T[i]).astype(np.int32), ((s == T[i]) | (s == below)).astype(np.int32)


def half_edge_frame(thresholds, seed=4709):
    """-> (EdgeFrame, image (2 rows, 2 COLS, 4) float16) for pass 2 at exactly 2:1: every quad of half_edge_quads in all 24 tap
    orders at both output-column parities, between seeded random blocks of halves in [0, 1].  R, G and B are independent: the
    texels of a block carry threshold i in R, i + 85 in G and i + 170 (other side) in B, each in its own tap order; alpha
    carries a ramp over [0, 1]."""
    T = np.asarray(thresholds, np.float32)
    e = half_edge_quads(T)
    e["have_upper"] = e["have_lower"] = np.ones(255, bool)
    probes = rc._probe_list(e)
    ef = rc.EdgeFrame(len(probes), seed)
    ef.edges = e
    i, side, order = probes.T
    n = len(probes)
    texels = np.empty((n, 4, 4), np.uint16)  # block, tap, R G B A
    m = np.empty((n, 3, 4), np.int32)        # channels in output byte order B, G, R
    for ch, (di, flip, do) in ((2, (0, 0, 0)), (1, (85, 0, 5)), (0, (170, 1, 11))):
        ci, cs, co = (i + di) % 255, side ^ flip, (order + do) % len(rc.ORDERS)
        q = np.where(cs[:, None] == 1, e["upper"][ci], e["lower"][ci])
        texels[:, :, 2 - ch] = np.take_along_axis(q, np.array(rc.ORDERS)[co], axis=1)
        cs, exact = _classify(T, texels[:, :, 2 - ch], ci)
        m[:, ch] = np.stack([ci, cs, co, exact], axis=1)
    ramp = (np.arange(4 * n, dtype=np.float32) % 1021) / np.float32(1020)
    texels[:, :, 3] = ramp.astype(np.float16).view(np.uint16).reshape(n, 4)
    nb = ef.rows * ef.COLS
    X = ef.place(ef.rng.integers(0, ONE + 1, (nb, 4, 4), dtype=np.uint16), texels).reshape(ef.rows, ef.COLS, 4, 4)
    ef.place(ef.meta, m)
    img = np.empty((2 * ef.rows, 2 * ef.COLS, 4), np.uint16)
    img[0::2, 0::2], img[0::2, 1::2], img[1::2, 0::2], img[1::2, 1::2] = X[:, :, 0], X[:, :, 1], X[:, :, 2], X[:, :, 3]
    return ef, as_halves(img)


# ------------------------------------------------------------------ wild texels

def wild_image(w, h, seed):
    """-> (finite, nonfinite), each (h, w, 4) float16.  finite: codes drawn uniformly from all 63 488 finite ones -- negatives,
    zeros of both signs, subnormals, values up to 65504.  nonfinite: the same image with about 1 % of its texels replaced,
    every channel of such a texel by +inf, -inf or a NaN (either sign, a random payload)."""
    rng = np.random.default_rng(seed)
    codes = FINITE_CODES[rng.integers(0, FINITE_CODES.size, (h, w, 4))]
    hit = rng.random((h, w)) < 0.01
    kind = rng.integers(0, 3, (h, w, 4))
    nan = (INF | rng.integers(1, 1024, (h, w, 4)) | (rng.integers(0, 2, (h, w, 4)) << 15)).astype(np.uint16)
    special = np.where(kind == 0, np.uint16(INF), np.where(kind == 1, np.uint16(NEG_INF), nan)).astype(np.uint16)
    wild = np.where(hit[:, :, None], special, codes).astype(np.uint16)
    assert is_nan_code(nan).all() and not is_nan_code(codes).any() and ((codes & 0x7c00) != 0x7c00).all()
    return as_halves(codes), as_halves(wild)


def one_infinity_image():
    """A 4 x 2 image of 0.5 with one +inf texel, for a 1:1 render: -> (image (2, 4, 4) float16, (row, column) of the texel)."""
    codes = np.full((2, 4, 4), 0x3800, np.uint16)
    codes[0, 2] = INF  # not in the last row or column: there the texel is its own clamped neighbour, under a weight of 0
    return as_halves(codes), (0, 2)


# ------------------------------------------------------------------ every byte of the BGRA8 form

def every_byte_image():
    """(512, 128 * 4) uint8 BGRA8 rows of flat 2x2 blocks, 256 rows of 64: block (r, c) holds byte (r + c + 64 k) & 255 in
    channel k (B, G, R, A) -- every byte value in every channel at every lane position of a wave; rendered to 64 x 256."""
    r, c = np.meshgrid(np.arange(256), np.arange(64), indexing="ij")
    blocks = ((r[:, :, None] + c[:, :, None] + 64 * np.arange(4)[None, None, :]) & 255).astype(np.uint8)
    return np.repeat(np.repeat(blocks, 2, axis=0), 2, axis=1).reshape(512, 128 * 4), blocks
