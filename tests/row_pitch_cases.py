"""Where the ROWS of a plane lie (tests/test_row_pitch_cpu.py, tests/test_row_pitch_gpu.py; numpy and ctypes only).

Every kernel forms two address products: frame i = frame 0 + i * step (tests/batch_spacing_cases.py) and, inside a frame,
row * pitch.  Every entry point accepts any pitch up to 2^32 - 1 on every plane; the rest of the suite never leaves a few
thousand bytes.  build(route, cls) lays the planes of a route of batch_spacing_cases.ROUTES (or of the four plane-shuffle routes
below) out in the same two slabs of 4 GiB + 1 MiB under a PITCH CLASS, which replaces every plane's pitch by one congruent to
it mod 16 -- the alignment folds pick the same kernel, the kernel name and tap form on record stay the route's:

    past-2^31    plane k's base at 2^31 + 2^19 + k * 8 KiB, the pitch such that the LAST row's offset is 2^31 + d: taken as a signed
                 32-bit number it lands 2^32 lower, inside the slab, where the plane's alias window is
    past-2^32    base at k * 8 KiB, the pitch the route's residue rounded up from (2^32 + d) / (rows - 1): the last row lies
                 above 2^32, the rows before it sweep [2^31, 2^32); a product cut to 32 bits lands on base + d, the alias window.
                 The planar routes' "cbcr" plane is U's rows, then V's: U's stay below 2^32, V's last passes it (v_offset + row
                 offset is the sum under test)
    under-2-GiB  the any-ratio and pass-2 routes only (they form row offsets in 32 bits and refuse planes with rows x pitch >=
                 2^31): every plane at the LARGEST pitch of its residue the contract accepts
    at-2-GiB     the same routes: one plane at the SMALLEST pitch of its residue with rows x pitch >= 2^31, the others at the
                 route's own; the call is refused (BT709HIP_ERR_UNSUPPORTED), one test per plane

A kernel that walks row PAIRS forms the product for the even row and adds one pitch: for such a plane (Y, alpha, a 1:1 target)
the product itself stops one row short of the class's boundary, and it is the chroma plane, the general kernels' odd-row
product and every single-row kernel that cross it.

A planar CHW surface (batch_spacing_cases: planes R, G, B (A) stacked at one pitch) is ONE plane of planes x H rows here, too, and
its address is a SUM: c x H x pitch + row x pitch.  Under the past- classes every plane but the last lies below the boundary,
the last one begins below it and the sum crosses it for that plane's last row alone.  (A slab ends 1 MiB past 2^32, so ONE row
of a plane can lie past a boundary: the sum for the last EVEN row, which the 1:1 kernels and the encoder form before they add
one pitch, stops a row short of it as a Y plane's product does.)  Behind the fused rescale the same sum rides in 32 bits and
the contract is planes x OH x pitch < 2^31 (scaled_planes_fit): under-2-GiB and at-2-GiB take rows = planes x OH.  The room of
a fourth plane batch_spacing_cases gives an opaque decoder's target is NOT given here: at these pitches it lies outside the
slab (the spacing and extent suites and the CHW families' own tests watch that place).

The encoder's families (batch_spacing_cases: I420, the converter, the pairs, RGBA16Float input) each spell these products out in
a header of their own.  The packed converter's "y" plane is 4-byte words and a single-row product (every row is formed on its
own, as a BGRA target's); a pair's "alpha_y" is walked in row pairs as Y is, with the alpha frame's own pitch, and its
"alpha_cbcr" -- under I420 v_plane_offset(AlphaPlanes) + the row offset -- crosses the boundary in its last row as "cbcr" does.

A layout holds two frames, frame 1's planes 4 KiB behind frame 0's, and names the WINDOWS the host touches: one per row (the
samples and a guard band either side) and the alias windows.  Layout.check() asserts, on the CPU, that all of them lie inside
their slab, apart from one another, that the class's inequality holds for every plane and that every alias window is where the
wrong arithmetic would land."""
import copy

import batch_spacing_cases as bs
from batch_spacing_cases import GUARD, SLAB_BYTES, Plane, Route

SLOT, FRAME_GAP = 8 << 10, 4 << 10  # a plane's slot of the low MiB; frame 1 behind frame 0
WHOLE_SLOT, WHOLE_GAP = 64 << 10, 32 << 10  # at-2-GiB: the planes that keep the route's pitch lie there whole
TWO31, TWO32 = 1 << 31, 1 << 32
HIGH_ORIGIN = TWO31 + (1 << 19)
FRAMES = 2

CW, CH = 32, 8  # chroma planes of the plane-shuffle routes
PLANE_ROUTES = [
    # bt709hip_interleave_cbcr / bt709hip_deinterleave_cbcr (context-level, one frame a call): the wide branch -- chroma width a
    # multiple of 8, every alignment met -- and the byte branch
    Route("interleave-wide", "interleave", (CW, CH), (CW, CH), [Plane("u", CW, CH, 40, unit=8), Plane("v", CW, CH, 48, unit=8)],
          [Plane("cbcr", 2 * CW, CH, 80, unit=16)], b"interleave_cbcr"),
    Route("interleave-bytes", "interleave", (30, CH), (30, CH), [Plane("u", 30, CH, 31), Plane("v", 30, CH, 33)], [Plane("cbcr", 60, CH, 61)],
          b"interleave_cbcr"),
    Route("deinterleave-wide", "deinterleave", (CW, CH), (CW, CH), [Plane("cbcr", 2 * CW, CH, 80, unit=16)],
          [Plane("u", CW, CH, 40, unit=8), Plane("v", CW, CH, 48, unit=8)], b"deinterleave_cbcr"),
    Route("deinterleave-bytes", "deinterleave", (30, CH), (30, CH), [Plane("cbcr", 60, CH, 61)], [Plane("u", 30, CH, 31), Plane("v", 30, CH, 33)],
          b"deinterleave_cbcr"),
]
ROUTES = bs.ROUTES + PLANE_ROUTES
ROUTE = {r.name: r for r in ROUTES}
CLASSES = ["past-2^31", "past-2^32", "under-2-GiB", "at-2-GiB"]
PAST, LIMIT = CLASSES[:2], CLASSES[2:]


def limited(route):
    """The routes whose kernels form row offsets in 32 bits (bt709_kernels.h plane_fits)."""
    return route.entry in ("scaled", "render")


# every past-2^31 pair before the past-2^32 pairs: a signed 32-bit mistake fails a comparison inside the slab under the first and
# would leave the slab under the second
PAIRS_RUN = [(r.name, c) for c in PAST for r in ROUTES if not limited(r)] + [(r.name, "under-2-GiB") for r in ROUTES if limited(r)]
# at-2-GiB: one case per plane of the route
AT_LIMIT = [(r.name, p.name) for r in ROUTES if limited(r) for p in r.ins + r.outs]
CLASSES_NOT_RUN = {(r.name, c): "the entry point refuses planes of 2 GiB or more (at-2-GiB asserts it)" for r in ROUTES if limited(r) for c in PAST}
CLASSES_NOT_RUN.update({(r.name, c): "no limit on rows x pitch applies to this kernel" for r in ROUTES if not limited(r) for c in LIMIT})


def _at_least(v, residue):
    """The smallest pitch >= v that is congruent to `residue` mod 16."""
    return v + (residue - v) % 16


def _at_most(v, residue):
    return v - (v - residue) % 16


def alias_gap(p):
    """d: how far above the boundary the last row lies at least -- the alias window clears row 0 and its guard bands."""
    return bs._up(p.row_bytes + 2 * GUARD, 16)


def pitch_for(p, cls, victim=False):
    residue = p.stride % 16
    if cls == "past-2^31":
        return _at_least(-(-(TWO31 + alias_gap(p)) // (p.rows - 1)), residue)
    if cls == "past-2^32":
        return _at_least(-(-(TWO32 + alias_gap(p)) // (p.rows - 1)), residue)
    if cls == "under-2-GiB":
        return _at_most((TWO31 - 1) // p.rows, residue)
    return _at_least(-(-TWO31 // p.rows), residue) if victim else p.stride


def repitched(route, cls, victim=None):
    """The route with every plane at the class's pitch (at-2-GiB: plane `victim` alone)."""
    r = copy.copy(route)
    swap = lambda planes: [Plane(p.name, p.row_bytes, p.rows, pitch_for(p, cls, p.name == victim), p.unit, stacked=p.stacked) for p in planes]
    r.ins, r.outs = swap(route.ins), swap(route.outs)
    return r


def _apart(p):
    return p.stride >= p.row_bytes + 2 * GUARD


def _extents(p, o):
    return [(o + r * p.stride, o + r * p.stride + p.row_bytes) for r in range(p.rows)] if _apart(p) else [(o, o + p.extent)]


class Layout:
    """route: the re-pitched route; base: the route as batch_spacing_cases / PLANE_ROUTES has it.  in_off / out_off: plane name ->
    byte offset of each frame's plane in its slab; *_windows: [(lo, hi)] the host touches; *_alias: [(lo, hi)] among them that
    hold no row.  The attributes batch_spacing_cases.Call and its window helpers read are a batch_spacing_cases.Layout's."""

    def __init__(self, base, cls, victim=None):
        self.base, self.cls, self.victim, self.route = base, cls, victim, repitched(base, cls, victim)
        self.n, self.uniform, self.source = FRAMES, True, list(range(FRAMES))
        self.in_off, self.out_off, self.steps = {}, {}, {}
        self.in_windows, self.out_windows, self.in_alias, self.out_alias = [], [], [], []

    def side(self, which):
        return (self.route.ins, self.in_off, self.in_windows, self.in_alias) if which == "in" else (self.route.outs, self.out_off, self.out_windows, self.out_alias)

    def rows(self, which):
        """(lo, hi) of every row of samples, each once; of the whole plane where its rows are closer than two guard bands (the
        planes of at-2-GiB that keep the route's pitch)."""
        planes, off, _, _ = self.side(which)
        return sorted(e for p in planes for o in off[p.name] for e in _extents(p, o))

    def check(self):
        name, cls = self.base.name, self.cls
        assert len(self.base.ins + self.base.outs) == len(self.route.ins + self.route.outs)
        for old, new in zip(self.base.ins + self.base.outs, self.route.ins + self.route.outs):  # the same kernel: the same folds
            assert (new.name, new.rows, new.row_bytes, new.unit) == (old.name, old.rows, old.row_bytes, old.unit)
            assert new.stride % 16 == old.stride % 16 and new.row_bytes <= new.stride <= 0xFFFFFFFF, (name, cls, new.name)
        for which in ("in", "out"):
            planes, off, windows, alias = self.side(which)
            rows = self.rows(which)
            assert len(rows) == self.n * sum(p.rows if _apart(p) else 1 for p in planes)
            ext = sorted(rows + alias)
            assert all(0 <= lo < hi <= SLAB_BYTES for lo, hi in ext), (name, cls, which, "outside the slab")
            assert all(b[0] - a[1] >= GUARD for a, b in zip(ext, ext[1:])), (name, cls, which, "overlapping or adjacent")
            ws = sorted(windows)
            assert all(0 <= lo < hi <= SLAB_BYTES for lo, hi in ws) and all(a[1] <= b[0] for a, b in zip(ws, ws[1:])), (name, cls, which)
            for lo, hi in ext:  # each, with its guard bands, in exactly one window
                g = 0 if (lo, hi) in alias else GUARD
                assert sum(1 for wl, wh in ws if wl <= lo - g and hi + g <= wh) == 1, (name, cls, which, lo, hi)
            assert len(alias) == (self.n * len(planes) if cls in PAST else 0)
            for p in planes:
                o = off[p.name]
                assert len(o) == self.n and all(v % 16 == 0 for v in o) and self.steps[p.name] == o[1] - o[0] > 0
                last, area = (p.rows - 1) * p.stride, p.rows * p.stride
                if cls == "past-2^31":  # the last row alone is past 2^31; as int32 its offset is last - 2^32
                    assert (p.rows - 2) * p.stride < TWO31 <= last < TWO32 and min(o) >= TWO31, (name, p.name)
                    landed = [v + last - TWO32 for v in o]
                elif cls == "past-2^32":  # the last row alone is past 2^32; cut to 32 bits its offset is last - 2^32 too, from a low base
                    assert TWO31 <= (p.rows - 2) * p.stride < TWO32 <= last and max(o) < (1 << 20), (name, p.name)
                    assert last - TWO32 >= p.row_bytes + 2 * GUARD  # not row 0
                    landed = [v + (last & 0xFFFFFFFF) for v in o]
                    if self.base.planar_chroma and p.name in ("cbcr", "alpha_cbcr"):  # U's rows below 2^32, V's last above: v_offset + row offset crosses it
                        assert (p.rows // 2 - 1) * p.stride + p.row_bytes < TWO32 <= (p.rows // 2) * p.stride + (p.rows // 2 - 1) * p.stride
                elif cls == "under-2-GiB":  # the largest accepted pitch of the residue
                    assert area < TWO31 <= p.rows * (p.stride + 16), (name, p.name)
                    landed = []
                else:
                    if p.name == self.victim:  # the smallest refused pitch of the residue
                        assert p.rows * (p.stride - 16) < TWO31 <= area, (name, p.name)
                    else:
                        assert p.stride == self.base.plane(p.name).stride
                    landed = []
                assert (p.stacked > 1) == (bool(self.base.chw) and p.name in ("out", "chw")), (name, p.name)
                if cls in PAST and p.stacked > 1:
                    # the planes of a CHW surface: every plane but the last lies below the boundary, the last one BEGINS below it,
                    # and c x H x pitch + row x pitch crosses it for that plane's last row alone
                    boundary, h = (TWO31 if cls == "past-2^31" else TWO32), p.rows // p.stacked
                    plane = h * p.stride
                    assert p.stacked in (3, 4) and h == self.base.out_size[1] and h >= 2
                    assert (p.stacked - 1) * plane + p.row_bytes <= boundary, (name, p.name)  # planes 0 .. count - 2 whole, and row 0 of the last
                    assert (p.stacked - 1) * plane + (h - 2) * p.stride + p.row_bytes <= boundary <= (p.stacked - 1) * plane + (h - 1) * p.stride, (name, p.name)
                for v in landed:
                    assert (v, v + p.row_bytes) in alias, (name, cls, p.name)
        if cls == "at-2-GiB":
            assert self.victim in [p.name for p in self.route.ins + self.route.outs]
        return self


def build(base, cls, victim=None):
    assert (cls == "at-2-GiB") == (victim is not None)
    L = Layout(base, cls, victim)
    for which in ("in", "out"):
        planes, off, windows, alias = L.side(which)
        slot, gap = (WHOLE_SLOT, WHOLE_GAP) if cls == "at-2-GiB" else (SLOT, FRAME_GAP)
        for k, p in enumerate(planes, 1):
            origin = (HIGH_ORIGIN if cls == "past-2^31" else 0) + k * slot
            off[p.name] = [origin + i * gap for i in range(FRAMES)]
            L.steps[p.name] = gap
            for o in off[p.name]:
                windows += [(lo - GUARD, hi + GUARD) for lo, hi in _extents(p, o)]
                if cls in PAST:
                    a = o + (p.rows - 1) * p.stride - TWO32  # both classes: the last row, 2^32 lower
                    alias.append((a, a + p.row_bytes))
                    windows.append((a, a + p.row_bytes))
    return L.check()


# ------------------------------------------------------------------ calls

class Call(bs.Call):
    """batch_spacing_cases.Call over a row-pitch layout; the plane-shuffle routes have no batched entry point: one call a frame."""

    def __init__(self, layout, in_base, out_base):
        self.planes = layout.route.entry in ("interleave", "deinterleave")
        if not self.planes:
            bs.Call.__init__(self, layout.route, layout, in_base, out_base)
            return
        r = layout.route
        self.route, self.n = r, layout.n
        self.args = []
        for i in range(layout.n):
            at = {p.name: ((in_base + layout.in_off[p.name][i]) if p in r.ins else (out_base + layout.out_off[p.name][i]), p.stride) for p in r.ins + r.outs}
            self.args.append(at)

    def single(self, lib, ctx, dec, i, stream=None, wait=1):
        if not self.planes:
            return bs.Call.single(self, lib, ctx, dec, i, stream, wait)
        a, (cw, ch) = self.args[i], self.route.size
        if self.route.entry == "interleave":
            return lib.bt709hip_interleave_cbcr(ctx, a["u"][0], a["u"][1], a["v"][0], a["v"][1], a["cbcr"][0], a["cbcr"][1], cw, ch, stream, wait)
        return lib.bt709hip_deinterleave_cbcr(ctx, a["cbcr"][0], a["cbcr"][1], a["u"][0], a["u"][1], a["v"][0], a["v"][1], cw, ch, stream, wait)

    def batch(self, lib, ctx, dec, stream=None, wait=1, count=None):
        if not self.planes:
            return bs.Call.batch(self, lib, ctx, dec, stream, wait, count)
        for i in range(self.n if count is None else count):
            rc = self.single(lib, ctx, dec, i, stream, wait)
            if rc:
                return rc
        return 0


def unchecked(base, strides):
    """A layout of `base` with the pitches of `strides` (plane name -> pitch) in place of the route's, the planes at their low
    slots, NO windows and no self-check: for calls on the fake runtime, which dereferences nothing."""
    L = Layout(base, "at-2-GiB", None)
    swap = lambda planes: [Plane(p.name, p.row_bytes, p.rows, max(strides.get(p.name, p.stride), p.row_bytes), p.unit, stacked=p.stacked) for p in planes]
    L.route.ins, L.route.outs = swap(base.ins), swap(base.outs)
    for p in L.route.ins + L.route.outs:  # Plane() asserts pitch >= row; a smaller one under test is put in afterwards
        p.stride = strides.get(p.name, p.stride)
    for which in ("in", "out"):
        planes, off, _, _ = L.side(which)
        for k, p in enumerate(planes, 1):
            off[p.name] = [k * SLOT + i * FRAME_GAP for i in range(FRAMES)]
            L.steps[p.name] = FRAME_GAP
    return L
