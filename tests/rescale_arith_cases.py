"""Cases of the rescale family's arithmetic sweeps (tests/test_rescale_arith.py): NumPy + the CPU oracle, nothing else.

  * flat_frame / full_sweep_blocks / reduced_sweep_blocks: every (Y,Cb,Cr) -- or the slice that carries every R and every B
    input -- as flat 2x2 blocks.  A flat block's four-tap sum is 4 lin and the x 0.25 is exact, so an exact 2:1 rescale of it
    is the 1:1 decode of the triple (guarded on the CPU by the tests, not assumed).
  * edge_search: ordered byte quadruples whose sum in the oracle's order, (((l[a] + l[b]) + l[c]) + l[d]) * 0.25f, lands ON
    an encode threshold and on the float just BELOW it (the nearest reachable sums where none does), by a meet-in-the-middle
    search in float32.  free_byte_edges: any four bytes (a BGRA8 intermediate); nv12_edges: the R bytes one Y lattice reaches
    (the four pixels of an NV12 block share their chroma).
  * EdgeFrame: the found quadruples in all 24 orders, at both output-column parities, between seeded random neighbours, with the
    threshold index and side of every output pixel kept for the failure message.
  * the persistent 2:1 kernel's launch arithmetic restated from its header (half_rep_plan) and the cursor case table.
"""
import itertools

import numpy as np

from oracle_lib import GAMMA_LINEAR, GAMMA_SRGB

FILL = 0x5A
GREY_CHROMA = (128, 126, 130, 123, 133, 119, 137, 112)
ORDERS = list(itertools.permutations(range(4)))  # every order of the four taps: a changed summation order shows in some of them
assert len(ORDERS) == 24 and ORDERS[0] == (0, 1, 2, 3)


# ------------------------------------------------------------------ flat blocks

def flat_frame(Y, Cb, Cr):
    """NV12 frame whose 2x2 block (r, c) is flat (Y[r, c], Cb[r, c], Cr[r, c]) -> y (2R, 2C), cbcr (R, 2C)."""
    y = np.repeat(np.repeat(np.asarray(Y, np.uint8), 2, axis=0), 2, axis=1)
    cbcr = np.empty((Y.shape[0], 2 * Y.shape[1]), np.uint8)
    cbcr[:, 0::2], cbcr[:, 1::2] = Cb, Cr
    return y, cbcr


def blocks_of(y, cbcr):
    """Per-PIXEL (Y, Cb, Cr) of an NV12 frame, each (H, W): the block values of the frame twice its size."""
    cb = np.repeat(np.repeat(cbcr[:, 0::2], 2, axis=0), 2, axis=1)
    cr = np.repeat(np.repeat(cbcr[:, 1::2], 2, axis=0), 2, axis=1)
    return y, cb, cr


def table_image(table, Y, Cb, Cr, alpha=0xFF):
    """oracle.decode_table laid out as the BGRA image (R, C * 4) of blocks (Y, Cb, Cr)."""
    idx = (Y.astype(np.uint32) << 16) | (Cb.astype(np.uint32) << 8) | Cr.astype(np.uint32)
    rgb = table.reshape(-1, 3)[idx.reshape(-1)]
    out = np.empty((idx.size, 4), np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = rgb[:, 2], rgb[:, 1], rgb[:, 0], alpha
    return out.reshape(Y.shape[0], Y.shape[1] * 4)


def reduced_sweep_blocks():
    """The 131 072 blocks (Y, 128, Cr) and (Y, Cb, 128), 256 rows of 512: every R and every B input value, a slice of G."""
    Y = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 512, axis=1)
    v = np.arange(256, dtype=np.uint8)
    Cb = np.tile(np.concatenate([np.full(256, 128, np.uint8), v])[None, :], (256, 1))
    Cr = np.tile(np.concatenate([v, np.full(256, 128, np.uint8)])[None, :], (256, 1))
    return Y, Cb, Cr


def sample_blocks(oracle, gamma, seed, n=1 << 16):
    """n seeded random triples plus, per channel and output byte, one triple that decodes to it (from the oracle's own table):
    -> Y, Cb, Cr of shape (rows, 256), and the table."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 1 << 24, n, dtype=np.uint32)
    table = oracle.decode_table(gamma).reshape(-1, 3)
    extra = []
    for ch in range(3):
        vals, first = np.unique(table[:, ch], return_index=True)
        extra.append(first.astype(np.uint32))
    t = np.concatenate([t] + extra)
    t = np.concatenate([t, rng.integers(0, 1 << 24, -t.size % 512, dtype=np.uint32)]).reshape(-1, 256)  # an even number of rows
    return (t >> 16).astype(np.uint8), ((t >> 8) & 255).astype(np.uint8), (t & 255).astype(np.uint8), table


# ------------------------------------------------------------------ both sides of every encode threshold

def tap_sum(lin, q):
    """(((l[a] + l[b]) + l[c]) + l[d]) * 0.25f in float32, the oracle's order; q: (..., 4) bytes."""
    l = lin.astype(np.float32)[q]
    s = (l[..., 0] + l[..., 1]).astype(np.float32)
    s = (s + l[..., 2]).astype(np.float32)
    s = (s + l[..., 3]).astype(np.float32)
    return (s * np.float32(0.25)).astype(np.float32)


def _split(total, sums, lv):
    """total == float32(s + lv[j]) for some s of the sorted array `sums`: -> (s, j).  The s that round to `total` with a given j
    are the ones within half an ulp of total - lv[j], a contiguous run around that number's insertion point."""
    g = np.searchsorted(sums, np.float64(total) - lv.astype(np.float64))
    cand = np.clip(g[:, None] + np.arange(-2, 3)[None, :], 0, sums.size - 1)
    ok = (sums[cand] + lv[:, None]).astype(np.float32) == np.float32(total)
    j, w = np.argwhere(ok)[0]
    return sums[cand[j, w]], int(j)


def edge_search(lin, values, T):
    """For each threshold T[i]: four of the bytes `values` (sorted, distinct), in the oracle's order, whose tap sum is the smallest
    reachable one >= T[i] (`upper`) and the largest reachable one < T[i] (`lower`).  Meet in the middle: the distinct float32 pair
    sums, then the distinct triple sums, sorted; for each fourth byte the total is monotone in the triple sum, so the boundary
    against 4 T (exact: a power of two) is found by searchsorted and settled by exact re-evaluation of its neighbours.
    -> dict(upper (255, 4) u8, lower (255, 4) u8, have_upper, have_lower (255,) bool, up_ulps, lo_ulps (255,) int64: float32
    steps from the threshold, 0 = on it / 1 = the float just below it)."""
    lin = lin.astype(np.float32)
    values = np.asarray(values)
    lv = lin[values]
    s2u = np.unique((lv[:, None] + lv[None, :]).astype(np.float32))
    s3u = np.unique((s2u[:, None] + lv[None, :]).astype(np.float32))
    n3 = s3u.size
    T = T.astype(np.float32)
    T4 = (T * np.float32(4.0)).astype(np.float32)
    guess = np.searchsorted(s3u, T4[:, None].astype(np.float64) - lv[None, :].astype(np.float64))  # (255, m)
    win = np.arange(-4, 5)
    cand = np.clip(guess[:, :, None] + win[None, None, :], 0, n3 - 1)
    tot = (s3u[cand] + lv[None, :, None]).astype(np.float32)
    ge = tot >= T4[:, None, None]
    # the window brackets the boundary: its low end is below the threshold or the array's start, its high end at or above it
    # or the array's end
    assert np.all(~ge[:, :, 0] | (cand[:, :, 0] == 0)) and np.all(ge[:, :, -1] | (cand[:, :, -1] == n3 - 1))
    up = np.where(ge, tot, np.float32(np.inf)).reshape(255, -1)
    lo = np.where(~ge, tot, np.float32(-np.inf)).reshape(255, -1)
    iu, il = up.argmin(axis=1), lo.argmax(axis=1)
    k = np.arange(255)
    have_upper, have_lower = np.isfinite(up[k, iu]), np.isfinite(lo[k, il])
    flat = cand.reshape(255, -1)

    def quads(sel, have):
        out = np.zeros((255, 4), np.uint8)
        for i in np.flatnonzero(have):
            d = sel[i] // win.size
            s2, c = _split(s3u[flat[i, sel[i]]], s2u, lv)
            a_val, b = _split(s2, lv, lv)
            a = int(np.flatnonzero(lv == a_val)[0])
            out[i] = values[[a, b, c, d]]
        return out

    upper, lower = quads(iu, have_upper), quads(il, have_lower)
    su, sl = tap_sum(lin, upper), tap_sum(lin, lower)
    assert np.all(su[have_upper] >= T[have_upper]) and np.all(sl[have_lower] < T[have_lower])
    assert np.array_equal(su[have_upper] * np.float32(4.0), up[k, iu][have_upper]) and np.array_equal(sl[have_lower] * np.float32(4.0), lo[k, il][have_lower])
    bits = lambda a: a.view(np.uint32).astype(np.int64)  # positive floats order as their bit patterns
    return dict(upper=upper, lower=lower, have_upper=have_upper, have_lower=have_lower,
                up_ulps=np.where(have_upper, bits(su) - bits(T), -1), lo_ulps=np.where(have_lower, bits(T) - bits(sl), -1))


def encode_tables(oracle):
    """The tap values lin[b] (the sampler's linearisation of an sRGB8 byte) and the 255 thresholds of quantize(linear_to_srgb(.))."""
    return oracle.to_linear_table(GAMMA_SRGB), oracle.thresholds(GAMMA_LINEAR)


def edge_counts(e):
    """(thresholds hit exactly, hit one float below, hit on both sides)."""
    on, below = e["have_upper"] & (e["up_ulps"] == 0), e["have_lower"] & (e["lo_ulps"] == 1)
    return int(on.sum()), int(below.sum()), int((on & below).sum())


def free_byte_edges(oracle):
    lin, T = encode_tables(oracle)
    return edge_search(lin, np.arange(256), T)


def nv12_edges(oracle, gamma):
    """The same search over the R bytes of NV12 blocks with Cr in GREY_CHROMA (R does not depend on Cb): per threshold and side the
    best quadruple over the eight lattices.  Adds y_upper / y_lower (255, 4) luma bytes and cr_upper / cr_lower (255,)."""
    lin, T = encode_tables(oracle)
    best = None
    for cr in GREY_CHROMA:
        r = np.array([oracle.decode_pixel(gamma, Y, 128, cr)[0] for Y in range(256)])
        values, first_y = np.unique(r, return_index=True)
        e = edge_search(lin, values, T)
        y_of = np.zeros(256, np.uint8)
        y_of[values] = first_y
        for side, have, ulps in (("upper", "have_upper", "up_ulps"), ("lower", "have_lower", "lo_ulps")):
            e["y_" + side] = y_of[e[side]]
            e["cr_" + side] = np.full(255, cr, np.uint8)
        if best is None:
            best = e
            continue
        for side, have, ulps in (("upper", "have_upper", "up_ulps"), ("lower", "have_lower", "lo_ulps")):
            better = e[have] & (~best[have] | (e[ulps] < best[ulps]))
            for key in (side, "y_" + side, "cr_" + side, have, ulps):
                best[key][better] = e[key][better]
    return best


class EdgeFrame:
    """Probe blocks between random ones.  blocks: (rows, cols) grid; meta (rows, cols, channels, 4) int32 = threshold index i
    (0-based: T[i]), side (1: the sum as ordered is on / above the threshold, 0: below), order index, exact (that sum IS T[i] / the
    float below it);
    i = -1 for a block or channel that probes nothing.  channels are in output byte order B, G, R."""

    COLS = 272  # blocks per row: 136 quads, a partly filled third wave of the 2:1 kernels

    def __init__(self, n_probes, seed):
        self.rng = np.random.default_rng(seed)
        # probes at even block columns, a random block after each; one more random block; the same again: probes at odd columns
        total = 4 * n_probes + 1
        self.rows = -(-total // self.COLS)
        self.rows += self.rows & 1  # the source height is a multiple of 4
        self.n = n_probes
        pos = 2 * np.arange(n_probes)
        self.slots = np.concatenate([pos, 2 * n_probes + 1 + pos])
        assert (self.slots[:n_probes] % 2 == 0).all() and (self.slots[n_probes:] % 2 == 1).all() and self.COLS % 2 == 0
        self.meta = np.full((self.rows * self.COLS, 3, 4), -1, np.int32)

    def place(self, values, probes):
        """values: (rows * COLS, ...) random filler; probes (n, ...) -> values with the probes in their two slots."""
        values[self.slots] = np.concatenate([probes, probes])
        return values

    def describe(self, row, col, ch):
        i, side, order, exact = self.meta.reshape(self.rows, self.COLS, 3, 4)[row, col, ch]
        if i < 0:
            return "a random block"
        return "threshold index %d, %s side (%s), tap order %r, output column parity %d" % (
            i, "upper" if side else "lower", "exact" if exact else "nearest reachable", ORDERS[order], col & 1)


def _probe_list(e):
    """(i, side, order) of every probe block, and the quadruple table per side."""
    out = []
    for i in range(255):
        for side, have in ((1, "have_upper"), (0, "have_lower")):
            if e[have][i]:
                out += [(i, side, o) for o in range(len(ORDERS))]
    return np.array(out, np.int32)


def _classify(oracle, quads, i):
    """Side and exactness of probe quadruples AS ORDERED (a permutation may move the float32 sum): side 1 when the sum is at
    or above T[i], exact when it is T[i] itself / the float just below it."""
    lin, T = encode_tables(oracle)
    s = tap_sum(lin, quads)
    below = np.nextafter(T[i], np.float32(-np.inf), dtype=np.float32)
    side = (s >= T[i]).astype(np.int32)
    return side, ((s == T[i]) | (s == below)).astype(np.int32)


def nv12_edge_frame(oracle, gamma, seed=2709):
    """-> (EdgeFrame, y, cbcr): the NV12 frame of nv12_edges(gamma); the probed channel is R."""
    e = nv12_edges(oracle, gamma)
    probes = _probe_list(e)
    ef = EdgeFrame(len(probes), seed + gamma)
    ef.edges = e
    i, side, order = probes.T
    perm = np.array(ORDERS)[order]                                        # (n, 4)
    yq = np.where(side[:, None] == 1, e["y_upper"][i], e["y_lower"][i])  # (n, 4)
    yq = np.take_along_axis(yq, perm, axis=1)
    side_as_ordered, exact = _classify(oracle, np.take_along_axis(np.where(side[:, None] == 1, e["upper"][i], e["lower"][i]), perm, axis=1), i)
    cr = np.where(side == 1, e["cr_upper"][i], e["cr_lower"][i])
    cb = ef.rng.choice(np.array(GREY_CHROMA, np.uint8), len(probes))
    nb = ef.rows * ef.COLS
    Y = ef.place(ef.rng.integers(0, 256, (nb, 4), dtype=np.uint8), yq)
    Cb = ef.place(ef.rng.integers(0, 256, nb, dtype=np.uint8), cb)
    Cr = ef.place(ef.rng.integers(0, 256, nb, dtype=np.uint8), cr)
    m = np.full((len(probes), 3, 4), -1, np.int32)
    m[:, 2] = np.stack([i, side_as_ordered, order, exact], axis=1)
    ef.place(ef.meta, m)
    Y = Y.reshape(ef.rows, ef.COLS, 4)
    y = np.empty((2 * ef.rows, 2 * ef.COLS), np.uint8)
    y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = Y[..., 0], Y[..., 1], Y[..., 2], Y[..., 3]
    cbcr = np.empty((ef.rows, 2 * ef.COLS), np.uint8)
    cbcr[:, 0::2], cbcr[:, 1::2] = Cb.reshape(ef.rows, ef.COLS), Cr.reshape(ef.rows, ef.COLS)
    return ef, y, cbcr


def bgra_edge_frame(oracle, seed=3709):
    """-> (EdgeFrame, src (2 rows, 2 COLS * 4) BGRA8 bytes): free-byte quadruples for pass 2 alone at exactly 2:1, where the
    three channels are independent: the texels of a block carry threshold i in R, i + 85 in G and i + 170 (other side) in B,
    each in its own tap order."""
    e = free_byte_edges(oracle)
    assert e["have_upper"].all() and e["have_lower"].all()
    probes = _probe_list(e)
    ef = EdgeFrame(len(probes), seed)
    ef.edges = e
    i, side, order = probes.T
    n = len(probes)
    texels = np.empty((n, 4, 4), np.uint8)  # block, tap, B G R A
    m = np.empty((n, 3, 4), np.int32)
    for ch, (di, flip, do) in ((2, (0, 0, 0)), (1, (85, 0, 5)), (0, (170, 1, 11))):
        ci, cs, co = (i + di) % 255, side ^ flip, (order + do) % len(ORDERS)
        q = np.where(cs[:, None] == 1, e["upper"][ci], e["lower"][ci])
        texels[:, :, ch] = np.take_along_axis(q, np.array(ORDERS)[co], axis=1)
        cs, exact = _classify(oracle, texels[:, :, ch], ci)
        m[:, ch] = np.stack([ci, cs, co, exact], axis=1)
    texels[:, :, 3] = ef.rng.integers(0, 256, (n, 4), dtype=np.uint8)
    nb = ef.rows * ef.COLS
    X = ef.place(ef.rng.integers(0, 256, (nb, 4, 4), dtype=np.uint8), texels).reshape(ef.rows, ef.COLS, 4, 4)
    ef.place(ef.meta, m)
    src = np.empty((2 * ef.rows, 2 * ef.COLS, 4), np.uint8)
    src[0::2, 0::2], src[0::2, 1::2], src[1::2, 0::2], src[1::2, 1::2] = X[:, :, 0], X[:, :, 1], X[:, :, 2], X[:, :, 3]
    return ef, src.reshape(2 * ef.rows, 2 * ef.COLS * 4)


def check_probes_against(ef, out):
    """The oracle's own output `out` (rows, COLS * 4) on an edge frame: where the search reports a hit the probed channel is
    i + 1 on the edge and i one float below; a nearest-reachable probe lies on its side of the threshold."""
    px = out.reshape(ef.rows, ef.COLS, 4)[..., :3].astype(np.int32)
    meta = ef.meta.reshape(ef.rows, ef.COLS, 3, 4)
    i, side, exact = meta[..., 0], meta[..., 1], meta[..., 3]
    probe = i >= 0
    want = i + side
    assert (px[probe & (exact == 1)] == want[probe & (exact == 1)]).all()
    assert (px[probe & (side == 1)] >= want[probe & (side == 1)]).all() and (px[probe & (side == 0)] <= want[probe & (side == 0)]).all()
    return int((probe & (exact == 1)).sum()), int(probe.sum())


def first_difference(ef, got, want):
    """Message naming the first output pixel of an edge frame where `got` differs from the oracle's `want`."""
    diff = np.argwhere(got != want)
    probed = ef.meta.reshape(ef.rows, ef.COLS, 3, 4)[diff[:, 0], diff[:, 1] // 4, np.minimum(diff[:, 1] % 4, 2), 0] >= 0
    r, b = diff[np.flatnonzero(probed & (diff[:, 1] % 4 < 3))[0]] if (probed & (diff[:, 1] % 4 < 3)).any() else diff[0]  # a probed channel first
    ch = b % 4
    what = ef.describe(r, b // 4, ch) if ch < 3 else "the alpha channel"
    return "output row %d, column %d, channel %s: got %d, want %d; %s; %d bytes differ" % (
        r, b // 4, "BGRA"[ch], got[r, b], want[r, b], what, int((got != want).sum()))


# ------------------------------------------------------------------ the persistent 2:1 kernel's launch, restated

REP_BLOCK_THREADS = 1024        # bt709_kernels.h kRepBlockThreads


def uniform_encode_bytes(oracle):
    """Size of the persistent kernel's encode table (transfer_tables.h UniformTable), from the builder's documented rule: n + 2
    buckets of 8 bytes, n the smallest multiple of 32 from 256 up for which q = round(v n) -- ONE fma onto 2^23, round to
    nearest even -- files the 255 thresholds of quantize(linear_to_srgb(.)) in 255 different buckets."""
    from fractions import Fraction
    T = [Fraction(float(t)) for t in oracle.thresholds(GAMMA_LINEAR)]
    for n in range(256, 65537, 32):
        q = {round(t * n) for t in T}  # exact; round() of a Fraction rounds halves to even
        if len(q) == len(T):
            return (n + 2) * 8
    raise AssertionError("no uniform table")


def half_rep_plan(width, height, frames, workgroups):
    """bt709_rescale_half.hip launch_decode_half_rep: tile rows, grid, block and the cursor step (workgroups decomposed into
    tile, row pair, frame)."""
    quads, row_pairs = width // 4, height // 2
    tiles_x = -(-quads // REP_BLOCK_THREADS)
    threads = (-(-quads // tiles_x) + 63) // 64 * 64
    tile_rows = tiles_x * row_pairs * frames
    g = max(1, min(workgroups, tile_rows))
    return dict(tiles_x=tiles_x, row_pairs=row_pairs, tile_rows=tile_rows, grid=(g, 1, 1), block=(threads, 1, 1),
                cursor=(g % tiles_x, (g // tiles_x) % row_pairs, (g // tiles_x) // row_pairs))


def rep_copies(buckets, encode_bytes, lds_kb):
    """launch_decode_half_rep's choice for a gamma whose decode-side table has `buckets` uniform buckets (N + 1 entries of 16
    bytes) under a budget of `lds_kb` KiB (clamped to 16 ... 160): (log2 copies of the decode side, log2 copies of the encode
    side) -- decode side first, up to 16 copies, then the encode side with what is left, up to 32 -- or None where one copy
    of each does not fit (the short-lived kernel runs instead)."""
    budget = min(max(lds_kb, 16), 160) * 1024
    dec = (buckets + 1) * 16
    r1, r2 = 4, 0
    while r1 > 0 and (dec << r1) + encode_bytes > budget:
        r1 -= 1
    if (dec << r1) + encode_bytes > budget:
        return None
    while r2 < 5 and (dec << r1) + (encode_bytes << (r2 + 1)) <= budget:
        r2 += 1
    return r1, r2


LDS_BUDGETS_KB = tuple(range(16, 161, 16))
UNIFORM_BUCKETS = {0: 512, 1: 256, 2: 4096, 3: 1024}  # N per gamma (bt709hip_gamma_lookup reports it; the tests assert these)


# name, (width, height), frames, workgroups, tiles_x, tile rows, cursor step
CURSOR_CASES = [("A", (4104, 4), 6, 7, 2, 24, (1, 1, 1)),
                ("B", (8200, 8), 5, 17, 3, 60, (2, 1, 1)),
                ("C", (72, 20), 40, 13, 1, 400, (0, 3, 1))]
