"""How MUCH one launch carries (tests/test_extents_cpu.py, tests/test_extents_gpu.py; numpy and ctypes only).

tests/batch_spacing_cases.py pins how every kernel finds a frame, tests/row_pitch_cases.py how it finds a row.  This module takes
the same routes -- row_pitch_cases.ROUTES: a route for every kernel body the project launches; the names it can report beside
them are instantiations of those bodies, listed with the routed form in batch_spacing_cases.FORMS_NOT_ROUTED -- to the other
end of the same index space:
the most rows, frames and columns an entry point accepts ("Extents"), and one past it.  build(name, cls) derives a
RESIZED copy of the route (resized(): other sizes, every pitch congruent to the route's own mod 16 and every base a multiple of
256, so the kernel on record stays the route's, and batch_spacing_cases.want() keeps calling the oracle the route's own tests
use) and lays its planes out, frame after frame, in one input and one output slab under an EXTENT CLASS:

    tallest            one frame at the largest height the entry point accepts: 131070 rows (decode, encode; a planar CHW surface:
                       131070 rows in each of its 3 or 4 stacked planes), 131068 (half: H % 4
                       == 0), 65534 (unconvert), chroma height 65535 (the plane shuffles), out height 65535 from a source of FOUR
                       rows (scaled, render: every output row between the same few source rows, both edge clamps).  The width is
                       the smallest that still selects the kernel (8, 4 or 6; scaled, render: 8 -> 16 or 16 -> 10 columns, the
                       route's own ratio, on which the tap form depends)
    tallest-from-tall  scaled, render: out height 65535 from a source of 131072 rows
    too-tall           the first refused height: +2 rows, +4 for half, out height 65536, chroma height 65536
    longest            65535 evenly spaced items through the batched entry point, each the smallest geometry that selects the
                       kernel (at most 16 x 4).  Routes whose launch splits under the XCD-band map (Route.bands) run with the map
                       at its default: 65528 frames under it, grid.z 8191, and 7 behind advance_frames.  An item of a paired
                       encode is a PAIR: the call passes 2 x 65535 frames, all five planes evenly spaced
    longest-unbanded   the same with BT709HIP_OPT_XCD_BANDS (the encoder: BT709HIP_CTX_OPT_XCD_BANDS) at 0: one launch, grid.z 65535
    too-many           65536 evenly spaced items: refused
    wide               one frame of width 2^20 + 12 (+ the route's own width mod 4; chroma width 2^20 + 8 / + 6 for the plane
                       shuffles), height 2 (4 for half): the last tile, wave and 256-column group are ragged.  scaled, render: an
                       OUTPUT of 2^20 + 12 columns
    wide-down          scaled, render: from a source of 2^20 + 12 columns down to 1000

What each entry point returns one past its limit is pinned by REFUSAL: BT709HIP_ERR_UNSUPPORTED everywhere but
bt709hip_render_scaled_batch over 65535 surfaces, which checks its count with its other arguments: BT709HIP_ERR_INVALID_ARG.

Item k of a layout holds frame_data(route, k % 251) (and, where the route reads its destination, background(route, k % 251)), so
the expected bytes of 65535 items take 251 oracle calls.  251 is prime: an item index cut to 13 or 15 bits, taken modulo the
8191 frames of a band, moved by a multiple of 8 under 2008, or counted twice lands on an item of other content
(tests/test_extents_cpu.py has the argument, and the one mistake it does NOT cover at every k: an index cut to 8 bits is 64256 =
256 x 251 short for the items 64256..64511, and wrong content everywhere else).

The slabs are SLAB_BYTES (the largest case, tens of MB: the four float32 planes of a wide CHW view -- nothing here needs the
addressing modules' 4 GiB); a layout is ONE window a side, [0, total): a guard band of canary either end, ITEM_GAP bytes
between two items (behind an opaque decoder's planar CHW target first the room of a fourth plane), every pitch's padding.  The
helpers below are batch_spacing_cases.upload_inputs / reset_outputs / collect over such a layout without their per-row Python
loop (a layout has up to 262140 rows); tests/test_extents_cpu.py holds them to those on a small layout."""
import copy

import numpy as np

import batch_spacing_cases as bs
import row_pitch_cases as rp
from batch_spacing_cases import CANARY, F16, GUARD, Plane
from metalbt709decoder_amd import _capi

ROUTES = rp.ROUTES
ROUTE = rp.ROUTE
CLASSES = ["tallest", "tallest-from-tall", "too-tall", "longest", "longest-unbanded", "too-many", "wide", "wide-down"]
REFUSED = ("too-tall", "too-many")
PERIOD = 251
MOST_ITEMS, MOST_ROWS = 65535, 65535  # kMaxUniformBatch; gridDim.y: rows, row pairs or output rows, as the kernel walks them
ITEM_GAP = 32
WIDE = (1 << 20) + 12
SINGLES = [0, 8190, 8191, 65527, 65528, 65534]  # the band edges (8191 frames a band) and the split (65528 under the map, 7 behind)
ONCE, SHARED, WIDE_TAPS, PAIRS = _capi.SCALED_TAPS_ONCE, _capi.SCALED_TAPS_SHARED, _capi.SCALED_TAPS_WIDE, _capi.SCALED_TAPS_PAIRS


def rescales(route):
    return route.entry in ("scaled", "render")


def shuffles(route):
    return route.entry in ("interleave", "deinterleave")


def general(route):
    """The routes whose own pitches demote them to a kernel that takes any width: they run at width 6."""
    return route.name in ("blocks", "unconvert-pixel", "encode-blocks", "interleave-bytes", "deinterleave-bytes", "chw-blocks-f16", "encode-chw-f32-blocks",
                          "encode-i420-blocks-premul", "convert-packed-blocks", "encode-pair-i420-blocks", "encode-half-i420-blocks")


def refusal(route, cls):
    """What the batched entry point returns one past the limit (the single-frame call: BT709HIP_ERR_UNSUPPORTED throughout)."""
    return _capi.ERR_INVALID_ARG if route.entry == "render" and cls == "too-many" else _capi.ERR_UNSUPPORTED


# ------------------------------------------------------------------ which classes a route runs

def classes(route):
    out = ["tallest"] + (["tallest-from-tall"] if rescales(route) else []) + ["too-tall"]
    if not shuffles(route):
        out += ["longest"] + (["longest-unbanded"] if route.bands else []) + ["too-many"]
    return out + ["wide"] + (["wide-down"] if rescales(route) else [])


def _why_not(route, cls):
    if cls in ("tallest-from-tall", "wide-down"):
        return "the target has the source's size (or half of it): tallest / wide is the one case"
    if shuffles(route):
        return "the plane shuffles have no batched entry point"
    return "the launch is never split (no XCD-band map for this kernel): longest is the one launch"


PAIRS_ALL = [(r.name, c) for c in CLASSES for r in ROUTES if c in classes(r)]
PAIRS_RUN = [rc for rc in PAIRS_ALL if rc[1] not in REFUSED]
PAIRS_REFUSED = [rc for rc in PAIRS_ALL if rc[1] in REFUSED]
CLASSES_NOT_RUN = {(r.name, c): _why_not(r, c) for r in ROUTES for c in CLASSES if c not in classes(r)}


# ------------------------------------------------------------------ the resized route

def geometry(route, cls):
    """(w, h, ow, oh, frames) of the class; the plane shuffles: (chroma width, chroma height) twice."""
    e, (w0, h0), (ow0, oh0) = route.entry, route.size, route.out_size
    narrow = 6 if general(route) else (4 if route.name == "unconvert-vec" else 8)
    if e == "half":
        narrow = 8  # W % 4 == 0 and two output columns: the narrow kernel is selected by the route's pitches
    up = w0 < ow0  # scaled-once: the one route that enlarges
    n = {"longest": MOST_ITEMS, "longest-unbanded": MOST_ITEMS, "too-many": MOST_ITEMS + 1}.get(cls, 1)
    if cls in ("tallest", "too-tall", "tallest-from-tall"):
        extra = cls == "too-tall"
        if rescales(route):  # W small: the longest class's item widths, the route's own ratio
            h = 131072 if cls == "tallest-from-tall" else 4
            return (8, h, 16, MOST_ROWS + extra, n) if up else (16, h, 10, MOST_ROWS + extra, n)
        if shuffles(route):
            return narrow, MOST_ROWS + extra, narrow, MOST_ROWS + extra, n
        if e == "half":
            h = 131068 + 4 * extra
            return narrow, h, narrow // 2, h // 2, n
        h = (65534 if e == "unconvert" else 131070) + 2 * extra
        return narrow, h, narrow, h, n
    if cls in ("longest", "longest-unbanded", "too-many"):
        if rescales(route):
            return (8, 2, 16, 4, n) if up else (16, 4, 10, 2, n)
        if e == "half":
            return narrow, 4, narrow // 2, 2, n
        return narrow, 2, narrow, 2, n
    if cls == "wide":
        if rescales(route):  # an output of WIDE columns at the route's own ratios (1 : 2 and 1.6 : 1)
            return (WIDE // 2, 2, WIDE, 4, n) if up else (1677740, 4, WIDE, 2, n)
        if shuffles(route):
            cw = (1 << 20) + (6 if general(route) else 8)
            return cw, 2, cw, 2, n
        w = WIDE + w0 % 4
        return (w, 4, w // 2, 2, n) if e == "half" else (w, 2, w, 2, n)
    assert cls == "wide-down" and rescales(route)
    return WIDE, 4, 1000, 2, n


def _shape(route, p, which, w, h, ow, oh):
    """(row bytes, rows) of plane p of a frame of w x h (target ow x oh)."""
    e = route.entry
    if shuffles(route):
        return (2 * w if p.name == "cbcr" else w), h
    if p.name == "y" and p.unit == 4:  # the packed converter's words, through the frame's `y`
        return 4 * w, h
    if p.name in ("y", "alpha", "alpha_y"):
        return w, h
    if p.name in ("cbcr", "alpha_cbcr"):
        return (w // 2, h) if route.planar_chroma else (w, h // 2)
    if route.chw and p.name in ("out", "chw"):  # a planar CHW surface: its planes stacked at one pitch
        return (route.elem * w, 3 * h) if which == "in" else (route.elem * ow, route.chw_planes * oh)
    if which == "in":  # texels: 8 bytes each of an RGBA16Float surface (pass 2's source, the half encoder's input), else 4
        return (8 if route.in_fmt == F16 else 4) * w, h
    return (8 if route.fmt == F16 else 4) * ow, oh


def scaled_plan(route):
    """(tap form, persistent) the any-ratio launcher settles on for a route whose bases, pitches and steps are multiples of 4
    (bt709_rescale_scaled.hip scaled_taps; every rescale route here is one): by the wave when enlarging vertically -- every
    source pixel decoded once where the wave's 64 taps lie within 64 columns, the shared fetch where its windows fit 256 bytes
    -- else one lane a column, persistent; through the RGBA16Float intermediate every form is persistent."""
    (w, h), (ow, oh) = route.size, route.out_size
    sx, sy = np.float32(w) / np.float32(ow), np.float32(h) / np.float32(oh)
    taps = WIDE_TAPS if w % 4 == 0 and w >= 8 else PAIRS
    if taps == WIDE_TAPS and sy < 1.0 and sx * np.float32(64.0) + np.float32(12.0) <= 252.0:
        taps = SHARED
    if sx <= np.float32(0.95) and sy < 1.0:
        taps = ONCE
    f16 = dict(route.options).get(_capi.OPT_SCALE_INTERMEDIATE) == F16
    return taps, 1 if f16 or taps not in (ONCE, SHARED) else 0


def resized(route, cls):
    """The route at the class's sizes: every plane's pitch the smallest >= its row that is congruent to the route's mod 16."""
    w, h, ow, oh, _ = geometry(route, cls)
    r = copy.copy(route)
    r.key = "%s@%s" % (route.name, cls)  # frame_data / want keep its frames apart from the route's own
    r.size, r.out_size = (w, h), (ow, oh)

    def swap(planes, which):
        out = []
        for p in planes:
            row_bytes, rows = _shape(route, p, which, w, h, ow, oh)
            stride = rp._at_least(row_bytes, p.stride % 16)
            out.append(Plane(p.name, row_bytes, rows, stride, p.unit, room=rows // 3 * stride if p.room else 0, stacked=p.stacked))  # room: a fourth plane's
        return out
    r.ins, r.outs = swap(route.ins, "in"), swap(route.outs, "out")
    if cls == "longest-unbanded" and route.entry != "encode":  # the encoder's map is the context's (the GPU test sets and restores it)
        r.options = route.options + ((_capi.OPT_XCD_BANDS, 0),)
    if route.name == "half-wide":  # launches this large take the persistent kernel by default (half-rep-alpha's): the route is the short-lived one
        r.options = r.options + ((_capi.OPT_HALF_KERNEL, 0),)
    if route.taps is not None:
        r.taps = scaled_plan(r)
    return r


# ------------------------------------------------------------------ layouts

class _Evenly:
    """The offsets first + i * step, i < n, without holding them (batch_spacing_cases.Call reads them by index)."""

    def __init__(self, first, step, n):
        self.first, self.step, self.n = first, step, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        return self.first + i * self.step


class Layout:
    """route: the resized route; base: the route as its module has it.  The attributes batch_spacing_cases.Call and the window
    helpers read are a batch_spacing_cases.Layout's: in_off / out_off (plane name -> offset of every item's plane), steps, one
    window a side, no alias windows; source[i] = i % PERIOD."""

    def __init__(self, base, cls):
        self.base, self.cls, self.route = base, cls, resized(base, cls)
        self.n = geometry(base, cls)[4]
        self.uniform = True
        self.in_off, self.out_off, self.steps = {}, {}, {}
        self.in_windows, self.out_windows, self.in_alias, self.out_alias = [], [], [], []
        self.total = {}

    @property
    def source(self):
        return [i % PERIOD for i in range(self.n)]

    def side(self, which):
        return (self.route.ins, self.in_off, self.in_windows, self.in_alias) if which == "in" else (self.route.outs, self.out_off, self.out_windows, self.out_alias)

    def check(self):
        name, cls, n = self.base.name, self.cls, self.n
        assert len(self.base.ins + self.base.outs) == len(self.route.ins + self.route.outs)
        for old, new in zip(self.base.ins + self.base.outs, self.route.ins + self.route.outs):  # the same kernel: the same folds
            assert (new.name, new.unit) == (old.name, old.unit) and new.stride % 16 == old.stride % 16, (name, cls, new.name)
            assert new.row_bytes <= new.stride < new.row_bytes + 16
        for which in ("in", "out"):
            planes, off, windows, alias = self.side(which)
            assert windows == [(0, self.total[which])] and not alias and self.total[which] <= SLAB_BYTES, (name, cls, which)
            ext = []
            for p in planes:
                o, step = off[p.name], self.steps[p.name]
                assert len(o) == n and o[0] % 256 == 0 and step % 16 == 0 and (n == 1 or step >= p.extent + ITEM_GAP), (name, cls, p.name)
                ext.append((o[0], o[n - 1] + p.extent + p.room))  # the items of a plane (each with its room), a gap apart, lie in one run
            ext.sort()
            assert ext[0][0] >= GUARD and ext[-1][1] + GUARD <= self.total[which], (name, cls, which, "outside the window")
            assert all(b[0] - a[1] >= GUARD for a, b in zip(ext, ext[1:])), (name, cls, which, "overlapping or adjacent")
        return self


def _lay(L):
    for which in ("in", "out"):
        planes, off, windows, _ = L.side(which)
        cursor = GUARD
        for p in planes:
            first = bs._up(cursor, 256)
            step = bs._up(p.extent + p.room + ITEM_GAP, 16) if L.n > 1 else 0
            off[p.name] = _Evenly(first, step, L.n)
            L.steps[p.name] = step
            cursor = first + (L.n - 1) * step + p.extent + p.room + GUARD
        L.total[which] = bs._up(cursor, 256)
        windows.append((0, L.total[which]))
    return L


def slab_bytes():
    """The largest window of any case, rounded up to a MiB."""
    most = max(max(_lay(Layout(ROUTE[name], cls)).total.values()) for name, cls in PAIRS_ALL)
    return bs._up(most, 1 << 20)


SLAB_BYTES = slab_bytes()


def build(name, cls):
    return _lay(Layout(ROUTE[name], cls)).check()


# ------------------------------------------------------------------ the windows (whole arrays: no loop over rows)

def _items(buf, L, which, p):
    """The samples of plane p in a window image: (items, rows, row bytes), a view."""
    _, off, _, _ = L.side(which)
    first, step = off[p.name].first, off[p.name].step
    assert first + (L.n - 1) * step + p.extent <= buf.size
    return np.lib.stride_tricks.as_strided(buf[first:], shape=(L.n, p.rows, p.row_bytes), strides=(step * buf.itemsize, p.stride * buf.itemsize, buf.itemsize))


def _per_item(L, arrays):
    """[array of item j, j < min(n, PERIOD)] -> (items, ...): item k's is array k % PERIOD."""
    stack = np.stack(arrays)
    return stack if L.n == 1 else stack[np.arange(L.n) % PERIOD]


def periods(L):
    return min(L.n, PERIOD)


def input_image(L, fill):
    host = np.full(L.total["in"], fill, np.uint8)
    for p in L.route.ins:
        _items(host, L, "in", p)[...] = _per_item(L, [bs.frame_data(L.route, j)[p.name] for j in range(periods(L))])
    return host


def output_image(L):
    host = np.full(L.total["out"], CANARY, np.uint8)
    if L.route.reads_destination:
        for p in L.route.outs:
            _items(host, L, "out", p)[...] = _per_item(L, [bs.background(L.route, j) for j in range(periods(L))])
    return host


def upload_inputs(rig, d_in, L, fill):
    """The input window: `fill` in every byte that is no sample (row padding, the gaps between items, the guard bands)."""
    rig.upload(d_in, input_image(L, fill))


def reset_outputs(rig, d_out, L):
    """The output window: the canary, and where the route reads its destination background k % PERIOD in the pixels of target k.
    -> the window as uploaded."""
    host = output_image(L)
    rig.upload(d_out, host)
    return host


def collect(rig, d_out, L, before, label):
    """-> {plane name: (items, rows, row bytes)}; every byte of the window outside the pixels must be what it was."""
    raw = rig.download(d_out, L.total["out"])
    outside = np.ones(raw.size, bool)
    got = {}
    for p in L.route.outs:
        got[p.name] = _items(raw, L, "out", p).copy()
        _items(outside, L, "out", p)[...] = False
    stray = np.flatnonzero(outside & (raw != before))
    assert stray.size == 0, "%s: %d bytes written outside the pixels, first at slab offset %d" % (label, stray.size, stray[0])
    return got


def expected(L, oracle, tabs, T):
    """{plane name: (min(items, PERIOD), rows, row bytes)}: what item k must become is entry k % PERIOD."""
    wants = [bs.want(L.route, oracle, tabs, T, j, j) for j in range(periods(L))]
    return {p.name: np.stack([w[p.name] for w in wants]) for p in L.route.outs}


def assert_items(got, wanted, items, label):
    """got[k] == wanted[k % len(wanted)] for every k of `items` (None: all)."""
    ks = np.arange(got.shape[0]) if items is None else np.asarray(items)
    want_of = wanted[ks % wanted.shape[0]]
    if np.array_equal(got[ks], want_of):
        return
    bad = np.flatnonzero((got[ks] != want_of).reshape(len(ks), -1).any(axis=1))
    k = int(ks[bad[0]])
    bs.assert_plane(got[k], wanted[k % wanted.shape[0]], "%s, item %d (%d of %d items differ)" % (label, k, bad.size, len(ks)))


def forget(L):
    """Drop the frames and expected bytes batch_spacing_cases remembers for this layout's route (tens of MB in the wide classes)."""
    for cache in (bs._data, bs._want):
        for key in [k for k in cache if k[0] == L.route.key]:
            del cache[key]
