"""Cases and helpers of the encoder's parity sweeps (tests/test_encoder.py): everything here is NumPy + the CPU oracle,
except Harness, which drives bt709hip_encode_batch through the C ABI on slabs it lays out itself.

  * threaded_encode: the oracle's encoder over a thread pool (2x2 blocks are independent, so bands of whole row pairs
    compose exactly; ctypes releases the GIL).
  * all_colours_strip: every (R,G,B) once as a flat 2x2 block (8192 x 8192 in all), cut into horizontal strips.
  * edge_blocks: 2x2 blocks whose linear-light average lands ON and just BELOW each of the 255 BT709_from_linear
    thresholds, found by a meet-in-the-middle search in float32, in every summation order.
  * the launch plan restated (encode_block_threads, encode_row_pairs_per_block, expected_plan) and the case table.
  * Harness: pictures at chosen offsets / strides inside 0x5A-filled slabs; the whole slabs are compared afterwards, so
    padding bytes and the guard bands in front of, between and behind the planes are part of every comparison.
"""
import ctypes as C
import itertools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle_lib import GAMMA_APPLE, GAMMA_LINEAR, GAMMA_SRGB

PAIRS = [(GAMMA_SRGB, GAMMA_APPLE), (GAMMA_SRGB, GAMMA_SRGB), (GAMMA_LINEAR, GAMMA_LINEAR),
         (GAMMA_APPLE, GAMMA_APPLE), (GAMMA_SRGB, GAMMA_LINEAR)]
TABLE_ENCODE_APPLE = 4
FILL = 0x5A
GUARD = 4096  # bytes of 0x5A kept in front of and behind everything a case writes


def from_linear_kind(out_gamma):
    """Threshold table (oracle.thresholds kind) that IS BT709_from_linear(., out_gamma): transfer_tables.cpp build_encode_tables."""
    return {GAMMA_SRGB: GAMMA_LINEAR, GAMMA_LINEAR: GAMMA_SRGB, GAMMA_APPLE: TABLE_ENCODE_APPLE}[out_gamma]


def threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


# ------------------------------------------------------------------ the oracle, threaded

def threaded_encode(oracle, words, w, h, in_gamma, out_gamma):
    """oracle.encode_nv12 of an (h, w) picture of BGRA words (alpha ignored), in bands of whole row pairs."""
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(h, w)
    y = np.empty((h, w), np.uint8)
    c = np.empty((h // 2, w), np.uint8)
    n = threads()
    pairs_per_band = max(1, (h // 2 + 4 * n - 1) // (4 * n))
    bands = [(2 * r, min(h, 2 * (r + pairs_per_band))) for r in range(0, h // 2, pairs_per_band)]

    def one(band):
        r0, r1 = band
        by, bc = oracle.encode_nv12(words[r0:r1] & 0xFFFFFF, w, r1 - r0, in_gamma, out_gamma)
        y[r0:r1], c[r0 // 2:r1 // 2] = by, bc

    with ThreadPoolExecutor(n) as ex:
        list(ex.map(one, bands))
    return y, c


# ------------------------------------------------------------------ A: every colour

ALL_COLOURS_SIDE = 8192   # 4096 x 4096 blocks of 2x2
ALL_COLOURS_STRIPS = 8    # 8192 x 1024 each: 2^21 colours


def all_colours_strip(strip, seed):
    """Strip `strip` of the 8192 x 8192 picture whose block (by, bx) is flat colour index by * 4096 + bx
    (R = index >> 16, G = (index >> 8) & 255, B = index & 255), with random alpha bytes.  -> (rows, 8192) words."""
    rows = ALL_COLOURS_SIDE // ALL_COLOURS_STRIPS
    by = np.arange(strip * rows // 2, (strip + 1) * rows // 2, dtype=np.uint32)
    idx = by[:, None] * np.uint32(4096) + np.arange(4096, dtype=np.uint32)[None, :]
    words = np.repeat(np.repeat(idx, 2, axis=0), 2, axis=1)
    alpha = np.random.default_rng(seed).integers(0, 256, words.shape, dtype=np.uint8).astype(np.uint32) << np.uint32(24)
    return words | alpha


# ------------------------------------------------------------------ B2: blocks on and beside every threshold

# The 12 summation orders of four values that can differ in float32: which two are added first (commutative), which third.
ORDERS = [p for p in itertools.permutations(range(4)) if p[0] < p[1]]
assert len(ORDERS) == 12 and ORDERS[0] == (0, 1, 2, 3)


def average_f32(lin, b):
    """(((l0 + l1) + l2) + l3) / 4 in float32, the reference's order (BT709.h:1171-1190); b: (..., 4) bytes."""
    l = lin[b]
    s = (l[..., 0] + l[..., 1]).astype(np.float32)
    s = (s + l[..., 2]).astype(np.float32)
    s = (s + l[..., 3]).astype(np.float32)
    return (s / np.float32(4.0)).astype(np.float32)


def _edge_search(lin, T):
    """For each threshold T[k-1], k = 1..255: bytes (b0, b1, b2, b3) whose float32 average is the smallest reachable one
    >= T[k-1] (`upper`) and the largest reachable one < T[k-1] (`lower`).  Meet in the middle: all distinct float32 sums
    (l0 + l1) + l2 with one representative triple each, sorted; for each l3 the sum + l3 is monotone in the sum, so the
    boundary against 4 T (exact: a power of two) is found by searchsorted and settled by exact re-evaluation of the
    neighbours.  -> upper (255, 4) uint8, lower (255, 4) uint8, have_lower (255,) bool."""
    lin = lin.astype(np.float32)
    b = np.arange(256)
    s2 = (lin[:, None] + lin[None, :]).astype(np.float32).reshape(-1)
    s2u, i2 = np.unique(s2, return_index=True)
    s3 = (s2u[:, None] + lin[None, :]).astype(np.float32).reshape(-1)
    s3u, i3 = np.unique(s3, return_index=True)
    rep = np.stack([b[i2[i3 // 256] // 256], b[i2[i3 // 256] % 256], b[i3 % 256]], axis=1).astype(np.uint8)  # (n3, 3)
    n3 = s3u.size
    T4 = (T.astype(np.float32) * np.float32(4.0)).astype(np.float32)  # (255,)
    # guess of the boundary for every (k, l3); window of neighbours re-evaluated exactly
    guess = np.searchsorted(s3u, (T4[:, None].astype(np.float64) - lin[None, :].astype(np.float64)))  # (255, 256)
    win = np.arange(-4, 5)
    cand = np.clip(guess[:, :, None] + win[None, None, :], 0, n3 - 1)                          # (255, 256, 9)
    tot = (s3u[cand] + lin[None, :, None]).astype(np.float32)                                   # exact float32 re-evaluation
    ge = tot >= T4[:, None, None]
    # the window brackets the boundary (monotone in the sum): its low end is below or at the array's start, its high end is
    # at or above the threshold or at the array's end
    assert np.all(~ge[:, :, 0] | (cand[:, :, 0] == 0)) and np.all(ge[:, :, -1] | (cand[:, :, -1] == n3 - 1))
    up = np.where(ge, tot, np.float32(np.inf)).reshape(255, -1)
    lo = np.where(~ge, tot, np.float32(-np.inf)).reshape(255, -1)
    iu, il = up.argmin(axis=1), lo.argmax(axis=1)
    k = np.arange(255)
    assert np.all(np.isfinite(up[k, iu]))
    have_lower = np.isfinite(lo[k, il])
    flat = cand.reshape(255, -1)

    def blocks(sel):
        c3 = flat[k, sel]
        l3 = (sel // win.size).astype(np.uint8)
        return np.concatenate([rep[c3], l3[:, None]], axis=1)

    return blocks(iu), blocks(il), have_lower


class EdgeBlocks:
    """All blocks of one gamma pair.  rgb: (n, 4, 3) bytes, pixel order top-left, top-right, bottom-left, bottom-right;
    meta: (n, 5) = channel, k, side (1 upper / 0 lower), order index, exact (upper average == threshold)."""

    def __init__(self, rgb, meta, lin, T, lower_ulps):
        self.rgb, self.meta, self.lin, self.T, self.lower_ulps = rgb, meta, lin, T, lower_ulps


def edge_blocks(oracle, pair, seed=709):
    in_gamma, out_gamma = pair
    lin = oracle.to_linear_table(in_gamma)
    T = oracle.thresholds(from_linear_kind(out_gamma))
    upper, lower, have_lower = _edge_search(lin, T)
    assert have_lower.all(), "a threshold with no reachable average below it"
    avg_u, avg_l = average_f32(lin, upper), average_f32(lin, lower)
    assert np.all(avg_u >= T) and np.all(avg_l < T)
    # distance of the lower block from the threshold, in float32 steps (positive floats order as their bit patterns)
    lower_ulps = T.view(np.uint32).astype(np.int64) - avg_l.view(np.uint32).astype(np.int64)
    rng = np.random.default_rng(seed + 16 * in_gamma + out_gamma)
    rgb, meta = [], []
    for c in range(3):
        others = [o for o in range(3) if o != c]
        for k in range(1, 256):
            ub, lb = upper[k - 1], lower[k - 1]
            # flat bytes for the two other channels that make the flip of channel c's averaged byte visible in Cb or Cr
            for _ in range(400):
                o = rng.integers(0, 256, 2)
                bu, bl = np.zeros((4, 3), np.uint8), np.zeros((4, 3), np.uint8)
                bu[:, c], bl[:, c] = ub, lb
                bu[:, others], bl[:, others] = o, o
                if oracle.subsample_block(bu.reshape(-1).tolist(), *pair)[4:] != oracle.subsample_block(bl.reshape(-1).tolist(), *pair)[4:]:
                    break
            else:
                raise AssertionError("no visible flip for channel %d threshold %d" % (c, k))
            for side, blk in ((1, bu), (0, bl)):
                for oi, order in enumerate(ORDERS):
                    rgb.append(blk[list(order)])
                    meta.append((c, k, side, oi, int(avg_u[k - 1] == T[k - 1])))
    return EdgeBlocks(np.array(rgb, np.uint8), np.array(meta, np.int32), lin, T, lower_ulps)


EDGE_BLOCKS_PER_ROW = 270  # 540 pixels: 135 quads, a partly filled third wave


def _edge_pad(n):
    return 1 if n % 2 == 0 else 2


def edge_block_at(eb, row_pair, column):
    """Index into eb.rgb / eb.meta of the block at chroma row `row_pair`, byte column `column` of edge_picture(eb); None for filler."""
    n = len(eb.rgb)
    pos = row_pair * EDGE_BLOCKS_PER_ROW + column // 2
    if pos < n:
        return pos
    pos -= n + _edge_pad(n)
    return pos if 0 <= pos < n else None


def edge_picture(eb):
    """All blocks of eb in one picture, laid out twice: the second copy shifted by one block, so every block sits once in
    the low half of a quad (top.xy / bot.xy) and once in the high half (top.zw / bot.zw).  -> (h, w) words."""
    words = (eb.rgb[..., 0].astype(np.uint32) << 16) | (eb.rgb[..., 1].astype(np.uint32) << 8) | eb.rgb[..., 2].astype(np.uint32)
    n = len(words)
    pad = np.zeros((_edge_pad(n), 4), np.uint32)  # an odd shift between the copies
    seq = np.concatenate([words, pad, words])
    assert (n + len(pad)) % 2 == 1
    bw = EDGE_BLOCKS_PER_ROW
    rows = (len(seq) + bw - 1) // bw
    seq = np.concatenate([seq, np.zeros((rows * bw - len(seq), 4), np.uint32)])
    pic = np.empty((2 * rows, 2 * bw), np.uint32)
    s = seq.reshape(rows, bw, 4)
    pic[0::2, 0::2], pic[0::2, 1::2], pic[1::2, 0::2], pic[1::2, 1::2] = s[..., 0], s[..., 1], s[..., 2], s[..., 3]
    return pic


# ------------------------------------------------------------------ C: the launch plan, restated

MAX_BLOCK_THREADS = 512    # bt709_kernels.h kMaxBlockThreads
GENERAL_THREADS = 256      # kBlockThreads
XCD_BAND_MIN_FRAMES = 64   # kXcdBandMinFrames
MAX_BATCH = 32             # kMaxBatch: pictures in the pointer table


def encode_block_threads(width):
    """bt709_kernels.h: equal tiles of <= 320 lanes, whole waves."""
    quads = width // 4
    tiles = 1 if quads == 0 else (quads + 319) // 320
    t = ((quads + tiles - 1) // tiles + 63) // 64 * 64
    return max(t, 64)


def encode_row_pairs_per_block(width, height, frames):
    """bt709_kernels.h: 3 to 9 row pairs, the most that still leaves the launch >= 4096 workgroups."""
    t = encode_block_threads(width)
    tiles = (width // 4 + t - 1) // t
    for rp in range(9, 3, -1):
        if tiles * ((height // 2 + rp - 1) // rp) * frames >= 4096:
            return rp
    return 3


def fast_path(width, bgra_stride, y_stride, cbcr_stride, bgra_bases, y_bases, cbcr_bases):
    """shim_convert.cpp bt709hip_encode_batch: the aligned kernel's predicate."""
    return (width % 4 == 0 and bgra_stride % 16 == 0 and y_stride % 4 == 0 and cbcr_stride % 4 == 0
            and all(p % 16 == 0 for p in bgra_bases) and all(p % 4 == 0 for p in y_bases) and all(p % 4 == 0 for p in cbcr_bases))


def expected_plan(width, height, frames, fast=True, uniform=None, bands=True):
    """bt709_encode.hip launch_encode with default context options -> dict(grid, block, launches, xcd_bands, row_pairs,
    kernel).  grid / block / xcd_bands / row_pairs describe the FIRST launch, as bt709hip_last_launch_info does."""
    if uniform is None:
        uniform = frames > 1
    if fast and bands and uniform and frames > XCD_BAND_MIN_FRAMES and frames % 8:
        plan = expected_plan(width, height, frames - frames % 8, fast, uniform, bands)
        plan["launches"] = 2
        plan["tail"] = expected_plan(width, height, frames % 8, fast, uniform, False)
        return plan
    if not fast:
        return dict(grid=((width // 2 + GENERAL_THREADS - 1) // GENERAL_THREADS, height // 2, frames), block=GENERAL_THREADS,
                    launches=1, xcd_bands=0, row_pairs=1, kernel="encode_bgra_nv12_blocks")
    rp = encode_row_pairs_per_block(width, height, frames)
    quads = width // 4
    t = encode_block_threads(width)
    if frames == 1:  # one picture per launch: tiles of up to 512 lanes
        tiles = (quads + 511) // 512
        t = max(((quads + tiles - 1) // tiles + 63) // 64 * 64, 64)
    t = min(t, MAX_BLOCK_THREADS)
    grid = ((quads + t - 1) // t, (height // 2 + rp - 1) // rp, frames)
    banded = int(bands and frames >= XCD_BAND_MIN_FRAMES and frames % 8 == 0)
    if banded:
        grid = (grid[0] * 8, grid[1], frames // 8)
    return dict(grid=grid, block=t, launches=1, xcd_bands=banded, row_pairs=rp, kernel="encode_bgra_nv12")


class Case:
    """One row of the launch table.  expect: what the row is FOR, stated by hand -- tiles, lanes, row pairs per workgroup,
    groups (of the first launch), banded, launches -- and held against expected_plan() by a CPU test, against the
    recorded launch by the GPU test."""

    def __init__(self, name, w, h, n, pair, expect, spacing="even", strides=None, gaps=(0, 0, 0), misalign=(0, 0, 0), bases=1):
        self.name, self.w, self.h, self.n, self.pair, self.expect = name, w, h, n, pair, expect
        self.spacing = spacing      # "even": evenly spaced slots (any count); "table": irregular offsets (pointer table, <= 32)
        self.strides = strides or (4 * w, w, w)   # bgra, y, cbcr
        self.gaps = gaps            # extra bytes between consecutive slots: bgra, y, cbcr
        self.misalign = misalign    # byte offsets added to the three bases
        self.bases = bases          # distinct base pictures the slots cycle through

    def __repr__(self):
        return self.name


def E(tiles, lanes, rp, groups, banded=0, launches=1, kernel="encode_bgra_nv12"):
    return dict(tiles=tiles, lanes=lanes, row_pairs=rp, groups=groups, banded=banded, launches=launches, kernel=kernel)


CASES = [
    Case("4k-single", 3840, 2160, 1, PAIRS[0], E(2, 512, 3, 360)),
    Case("2052x38-second-tile-mostly-empty", 2052, 38, 1, PAIRS[1], E(2, 320, 3, 7)),
    Case("4096x8-two-full-tiles", 4096, 8, 1, PAIRS[3], E(2, 512, 3, 2)),
    Case("3840x32x32-pointer-table", 3840, 32, 32, PAIRS[0], E(3, 320, 3, 6), spacing="table", bases=2),
    Case("1284x20x64-banded-two-tiles", 1284, 20, 64, PAIRS[4], E(2, 192, 3, 4, banded=1), bases=2),
    Case("1284x20x71-head-and-tail", 1284, 20, 71, PAIRS[1], E(2, 192, 3, 4, banded=1, launches=2), bases=2),
    Case("64x38x2048-nine-row-pairs", 64, 38, 2048, PAIRS[0], E(1, 64, 9, 3, banded=1), bases=3),
    Case("64x36x1203-five-then-three", 64, 36, 1203, PAIRS[2], E(1, 64, 5, 4, banded=1, launches=2), bases=3),
    Case("4kx64-readme-row", 3840, 2160, 64, PAIRS[0], E(3, 320, 9, 120, banded=1), bases=4),
    Case("1920x54-padded-strides-fast", 1920, 54, 1, PAIRS[3], E(1, 512, 3, 9), strides=(7680 + 64, 2048, 1936)),
    Case("1920x54x3-padded-strides-fast-table", 1920, 54, 3, PAIRS[0], E(2, 256, 3, 9), spacing="table", strides=(7680 + 64, 2048, 1936)),
    Case("1918x22-padded-strides-general", 1918, 22, 1, PAIRS[1], E(4, 256, 1, 11, kernel="encode_bgra_nv12_blocks"),
         strides=(4 * 1918 + 12, 1918 + 5, 1918 + 3), misalign=(4, 1, 3)),
    Case("1918x22x5-general-table", 1918, 22, 5, PAIRS[0], E(4, 256, 1, 11, kernel="encode_bgra_nv12_blocks"), spacing="table",
         strides=(4 * 1918 + 12, 1918 + 5, 1918 + 3), misalign=(8, 3, 1)),
    Case("256x16x40-gaps-separate-slabs", 256, 16, 40, PAIRS[4], E(1, 64, 3, 3), gaps=(4096, 512, 256), bases=2),
]


def case_plan(case):
    L = case_layout(case)
    fast = fast_path(L.w, L.sb, L.sy, L.sc, L.in_off, L.y_off, L.c_off)  # slab bases are at least 256-byte aligned
    return expected_plan(case.w, case.h, case.n, fast=fast, uniform=layout_is_uniform(L))


def plan_as_expect(plan):
    banded = plan["xcd_bands"]
    return dict(tiles=plan["grid"][0] // (8 if banded else 1), lanes=plan["block"], row_pairs=plan["row_pairs"], groups=plan["grid"][1],
                banded=banded, launches=plan["launches"], kernel=plan["kernel"])


# ------------------------------------------------------------------ pictures

def mixed_picture(seed, w, h):
    """Uniform random words in some 16x16 cells, smooth content elsewhere: a horizontal and a vertical ramp and a dark
    diagonal one (random bytes make every 2x2 average mid-grey; ramps walk the averages through the table, the dark one
    through its fine region near zero), with one bit of noise."""
    rng = np.random.default_rng(seed)
    x = np.arange(w, dtype=np.uint32)[None, :]
    y = np.arange(h, dtype=np.uint32)[:, None]
    r = (x * 255 // max(w - 1, 1)) + 0 * y
    g = (y * 255 // max(h - 1, 1)) + 0 * x
    b = ((x + y) * 40 // max(w + h - 2, 1))
    noise = rng.integers(0, 2, (3, h, w), dtype=np.uint32)
    smooth = (np.minimum(r + noise[0], 255) << 16) | (np.minimum(g + noise[1], 255) << 8) | np.minimum(b + noise[2], 255)
    rand = rng.integers(0, 1 << 32, (h, w), dtype=np.uint32)
    cells = rng.integers(0, 3, ((h + 15) // 16, (w + 15) // 16)) == 0
    mask = np.repeat(np.repeat(cells, 16, axis=0), 16, axis=1)[:h, :w]
    alpha = rng.integers(0, 256, (h, w), dtype=np.uint32) << 24
    return np.where(mask, rand, smooth | alpha).astype(np.uint32)


def slot_rows(h):
    """Row pairs a slot's own pattern overwrites: top, middle, bottom."""
    return sorted({0, (h // 2) // 2, h // 2 - 1})


def build_slots(oracle, case, seed):
    """-> base pictures [(words, y, cbcr)], per-slot patches: words (n, k, 2, w) and their oracle planes y (n, k, 2, w),
    cbcr (n, k, w) for the k row pairs of slot_rows(h).  Every slot's content is distinct (its patch is seeded by the slot)
    without paying the oracle for whole slots: 2x2 blocks are independent, so a slot's expected planes are its base's with
    those row pairs replaced by the oracle's answer for the patch."""
    w, h, n = case.w, case.h, case.n
    bases = []
    for i in range(case.bases):
        words = mixed_picture(seed * 131 + i, w, h)
        y, c = threaded_encode(oracle, words, w, h, *case.pair)
        bases.append((words, y, c))
    if n == 1:
        return bases, None
    rows = slot_rows(h)
    k = len(rows)
    rng = np.random.default_rng(seed * 977 + 1)
    patch = rng.integers(0, 1 << 32, (n, k, 2, w), dtype=np.uint32)
    patch[:, :, :, 0] = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761))[:, None, None]  # the slot's number, hashed
    py, pc = threaded_encode(oracle, patch.reshape(n * k * 2, w), w, n * k * 2, *case.pair)
    return bases, (patch, py.reshape(n, k, 2, w), pc.reshape(n, k, w))


# ------------------------------------------------------------------ GPU harness

def _rows_view(slab, off, rows, stride, width):
    """(rows, width) strided view of slab bytes starting at off."""
    return np.lib.stride_tricks.as_strided(slab[off:], shape=(rows, width), strides=(stride, 1))


class Layout:
    """Where n pictures of w x h live: byte offsets of each picture's BGRA rows in the input slab and of its planes in the Y slab
    and the CbCr slab, and the three strides."""

    def __init__(self, w, h, strides, in_off, y_off, c_off):
        self.w, self.h = w, h
        self.sb, self.sy, self.sc = strides
        self.in_off, self.y_off, self.c_off = list(in_off), list(y_off), list(c_off)
        self.n = len(self.in_off)
        # bytes a picture spans (the last row is only as long as the picture)
        self.in_span = (h - 1) * self.sb + 4 * w
        self.y_span = (h - 1) * self.sy + w
        self.c_span = (h // 2 - 1) * self.sc + w
        self.in_bytes = max(self.in_off) + self.in_span + GUARD
        self.y_bytes = max(self.y_off) + self.y_span + GUARD
        self.c_bytes = max(self.c_off) + self.c_span + GUARD
        for offs, span in ((self.in_off, self.in_span), (self.y_off, self.y_span), (self.c_off, self.c_span)):
            o = sorted(offs)
            assert o[0] >= GUARD and all(b - a >= span for a, b in zip(o, o[1:])), "pictures overlap or leave no guard band"


def case_layout(case):
    w, h, n = case.w, case.h, case.n
    sb, sy, sc = case.strides
    pitch = [h * sb + case.gaps[0], h * sy + case.gaps[1], (h // 2) * sc + case.gaps[2]]
    offs = []
    for j in range(3):
        if case.spacing == "even":
            offs.append([GUARD + case.misalign[j] + i * pitch[j] for i in range(n)])
        else:  # irregular: an extra multiple of 256 bytes that grows and shrinks from slot to slot
            extra = np.cumsum([256 * ((i * i) % 5) for i in range(n)])
            offs.append([GUARD + case.misalign[j] + i * pitch[j] + int(extra[i]) for i in range(n)])
    return Layout(w, h, (sb, sy, sc), *offs)


class Result:
    def __init__(self, y_slab, c_slab, kernel, info):
        self.y_slab, self.c_slab, self.kernel = y_slab, c_slab, kernel
        self.grid, self.block = tuple(info.grid), tuple(info.block)
        self.launches, self.xcd_bands = info.launches, info.xcd_bands


class Harness:
    """bt709hip_encode_batch on slabs of this module's making, default context options."""

    ROW = 1 << 16  # slabs move as 2-D copies of 64 KiB rows plus one short row

    def __init__(self, gh):
        from metalbt709decoder_amd import _capi
        from metalbt709decoder_amd.decoder import DeviceBuffer
        self.capi, self.DeviceBuffer = _capi, DeviceBuffer
        self.ctx = gh.context()
        self.lib, self.h = self.ctx.lib, self.ctx.handle

    def _pieces(self, nbytes):
        rows = nbytes // self.ROW
        if rows:
            yield 0, self.ROW, rows
        if nbytes % self.ROW:
            yield rows * self.ROW, nbytes % self.ROW, 1

    def _upload(self, dptr, arr):
        for o, width, rows in self._pieces(arr.size):
            self.capi.check(self.lib.bt709hip_upload(self.h, dptr + o, width, arr.ctypes.data + o, width, width, rows, None), "upload")
        self.capi.check(self.lib.bt709hip_stream_synchronize(self.h, None))

    def _download(self, dptr, nbytes):
        out = np.empty(nbytes, np.uint8)
        for o, width, rows in self._pieces(nbytes):
            self.capi.check(self.lib.bt709hip_download(self.h, out.ctypes.data + o, width, dptr + o, width, width, rows, None), "download")
        self.capi.check(self.lib.bt709hip_stream_synchronize(self.h, None))
        return out

    def encode(self, layout, in_slab, pair):
        """in_slab: host bytes of the whole input slab.  The output slabs are filled with 0x5A, the pictures encoded in ONE
        bt709hip_encode_batch call, the whole slabs read back."""
        capi, L = self.capi, layout
        assert in_slab.size == L.in_bytes
        d_in, d_y, d_c = (self.DeviceBuffer(self.ctx, nb, placement_tries=1) for nb in (L.in_bytes, L.y_bytes, L.c_bytes))
        try:
            assert all(d.ptr % 256 == 0 for d in (d_in, d_y, d_c))  # fast_path() reasons on offsets inside the slabs
            self._upload(d_in.ptr, in_slab)
            for d, nb in ((d_y, L.y_bytes), (d_c, L.c_bytes)):
                capi.check(self.lib.bt709hip_memset(self.h, d.ptr, FILL, nb, None))
            capi.check(self.lib.bt709hip_stream_synchronize(self.h, None))
            surfs = (capi.Surface * L.n)(*[capi.Surface(d_in.ptr + o, L.sb, L.w, L.h, capi.FORMAT_BGRA8_SRGB, 0) for o in L.in_off])
            frames = (capi.Frame * L.n)(*[capi.Frame(d_y.ptr + oy, L.sy, d_c.ptr + oc, L.sc, L.w, L.h, 0, 0)
                                          for oy, oc in zip(L.y_off, L.c_off)])
            capi.check(self.lib.bt709hip_encode_batch(self.h, L.n, surfs, frames, pair[0], pair[1], None, 1), "bt709hip_encode_batch")
            kernel = self.lib.bt709hip_last_kernel_name().decode()
            info = capi.LaunchInfo()
            capi.check(self.lib.bt709hip_last_launch_info(C.byref(info)))
            return Result(self._download(d_y.ptr, L.y_bytes), self._download(d_c.ptr, L.c_bytes), kernel, info)
        finally:
            for d in (d_in, d_y, d_c):
                d.free()


def fill_input(layout, pictures):
    """pictures(i) -> (h, w) words of slot i.  -> the input slab's host bytes (0x5A outside the pictures)."""
    L = layout
    slab = np.full(L.in_bytes, FILL, np.uint8)
    for i, off in enumerate(L.in_off):
        _rows_view(slab, off, L.h, L.sb, 4 * L.w)[:] = np.ascontiguousarray(pictures(i)).view(np.uint8).reshape(L.h, 4 * L.w)
    return slab


def expected_slabs(layout, planes):
    """planes(i) -> (y (h, w), cbcr (h/2, w)) of slot i.  -> the two output slabs as they must read back."""
    L = layout
    ys, cs = np.full(L.y_bytes, FILL, np.uint8), np.full(L.c_bytes, FILL, np.uint8)
    for i in range(L.n):
        y, c = planes(i)
        _rows_view(ys, L.y_off[i], L.h, L.sy, L.w)[:] = y
        _rows_view(cs, L.c_off[i], L.h // 2, L.sc, L.w)[:] = c
    return ys, cs


def describe_difference(layout, got, want, plane):
    """Where two slabs first differ, in the layout's terms (slot, row, column, or 'outside every picture')."""
    diff = np.flatnonzero(got != want)
    if diff.size == 0:
        return None
    L = layout
    offs, stride, width, rows = (L.y_off, L.sy, L.w, L.h) if plane == "y" else (L.c_off, L.sc, L.w, L.h // 2)
    p = int(diff[0])
    where = "outside every picture (guard band)"
    for i, o in enumerate(offs):
        if o <= p < o + (rows - 1) * stride + width:
            r, col = divmod(p - o, stride)
            where = "slot %d row %d column %d%s" % (i, r, col, " (row padding)" if col >= width else "")
            break
    return "%s plane: %d bytes differ, first at byte %d = %s: got %d, want %d" % (plane, diff.size, p, where, got[p], want[p])


def run_case(harness, oracle, case, seed):
    """Encode the case's pictures in one call; -> (Result, list of differences (empty = equal))."""
    L = case_layout(case)
    bases, patches = build_slots(oracle, case, seed)
    rows = slot_rows(case.h)

    def picture(i):
        words = bases[i % len(bases)][0]
        if patches is not None:
            words = words.copy()
            for j, rp in enumerate(rows):
                words[2 * rp:2 * rp + 2] = patches[0][i, j]
        return words

    def planes(i):
        _, y, c = bases[i % len(bases)]
        if patches is not None:
            y, c = y.copy(), c.copy()
            for j, rp in enumerate(rows):
                y[2 * rp:2 * rp + 2], c[rp] = patches[1][i, j], patches[2][i, j]
        return y, c

    res = harness.encode(L, fill_input(L, picture), case.pair)
    want_y, want_c = expected_slabs(L, planes)
    diffs = [d for d in (describe_difference(L, res.y_slab, want_y, "y"), describe_difference(L, res.c_slab, want_c, "cbcr")) if d]
    return res, diffs


def recorded_expect(res, case):
    """The recorded launch in the table's terms.  row_pairs follows from grid[1]: the table's heights give different group
    counts for neighbouring values."""
    banded = res.xcd_bands
    groups = res.grid[1]
    pairs = case.h // 2
    rp = [r for r in range(1, 65) if (pairs + r - 1) // r == groups]
    return dict(tiles=res.grid[0] // (8 if banded else 1), lanes=res.block[0], groups=groups, banded=banded, launches=res.launches,
                kernel=res.kernel, row_pairs_candidates=rp, grid_z=res.grid[2])


# ------------------------------------------------------------------ fuzzed geometry

FUZZ_CASES = 300
FUZZ_WIDTH_CENTRES = [16, 1024, 5120, 8192]  # 4, 256, 1280 and 2048 quads


def fuzz_case(i, seed=20709):
    """Case i of the seeded sequence -> (Layout, pair, pictures as a list of (h, w) words)."""
    rng = np.random.default_rng([seed, i])
    pair = PAIRS[int(rng.integers(0, len(PAIRS)))]
    kind = int(rng.integers(0, 4))
    if kind == 0:    # around and across a tile-count boundary
        w = max(2, FUZZ_WIDTH_CENTRES[int(rng.integers(0, 4))] + 2 * int(rng.integers(-6, 7)))
        h = 2 * int(rng.integers(1, 8))
    elif kind == 1:  # small
        w, h = 2 * int(rng.integers(1, 40)), 2 * int(rng.integers(1, 12))
    else:            # anything moderate
        w, h = 2 * int(rng.integers(1, 700)), 2 * int(rng.integers(1, 24))
    n = 1 if rng.integers(0, 2) else int(rng.integers(2, 6))
    aligned = bool(rng.integers(0, 2))  # half of the cases satisfy the fast path's alignment (then w % 4 decides)
    if aligned:
        if rng.integers(0, 2):
            w += w % 4
        sb = 4 * w + 16 * int(rng.integers(0, 5))
        sb += -sb % 16
        sy, sc = (w + 4 * int(rng.integers(0, 9)) + (-w % 4) for _ in range(2))
        mis = (16 * int(rng.integers(0, 3)), 4 * int(rng.integers(0, 4)), 4 * int(rng.integers(0, 4)))
        slot_quantum = 16
    else:
        sb = 4 * w + 4 * int(rng.integers(0, 9))
        sy, sc = w + int(rng.integers(0, 9)), w + int(rng.integers(0, 9))
        mis = (4 * int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 8)))
        slot_quantum = 4
    even = bool(rng.integers(0, 2))
    offs = []
    for j, (stride, rows, q) in enumerate(((sb, h, slot_quantum), (sy, h, 4 if aligned else 1), (sc, h // 2, 4 if aligned else 1))):
        pitch = stride * rows + q * int(rng.integers(0, 40))
        pitch += -pitch % q
        extra = [0] * n if even else list(np.cumsum([q * int(rng.integers(0, 9)) for _ in range(n)]))
        offs.append([GUARD + mis[j] + k * pitch + int(extra[k]) for k in range(n)])
    layout = Layout(w, h, (sb, sy, sc), *offs)
    pics = []
    for k in range(n):
        pics.append(mixed_picture(int(rng.integers(0, 1 << 31)), w, h) if rng.integers(0, 2) else
                    rng.integers(0, 1 << 32, (h, w), dtype=np.uint32))
    return layout, pair, pics


def layout_is_uniform(L):
    """bt709hip_encode_batch's `uniform`: more than one picture, and each of the three offsets of picture i is i times picture 1's."""
    if L.n < 2:
        return False
    return all(o[i] - o[0] == i * (o[1] - o[0]) for o in (L.in_off, L.y_off, L.c_off) for i in range(2, L.n))
