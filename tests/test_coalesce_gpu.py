"""GPU tests (-m gpu) of the coalescing submit (BT709HIP_OPT_COALESCE): one-frame calls made in stream order go out as one launch
whose items run concurrently.  Every decoder state the 1:1 decode accepts goes through the queue (a. the matrix), every term that
closes a queue closes it (b.), a state change between queued calls divides them (c.), and calls that share bytes -- a target
written twice, clips layered over one canvas, a target read back as a frame -- keep their order (d.).

Bit for bit against tests/coalesce_cases.py `expected` (numpy over the oracle), whole allocations compared: row padding and the
guard bands round every target included.  Every frame is queued on a stream of its own: the test's uploads and downloads run on
the context's default stream, and any call that takes a stream issues what is queued for THAT stream.

The launch record (bt709hip_last_launch_info) is per thread and keeps the last launch, so before a call whose launches matter
a MARKER launch of seven tiny frames is put on record: a call that launches nothing leaves the seven there, a call that issues k
queued frames leaves k.  The frame count of a launch is grid[2] of the fast and the RGBA16F kernels and grid[1] of the general
(`_blocks`) kernels, whose grid is (workgroups per frame, frames, 1)."""
import ctypes as C

import numpy as np
import pytest

import coalesce_cases as cc
import over_cases as oc
from metalbt709decoder_amd import _capi
from metalbt709decoder_amd._capi import Frame, Surface
from variant_cases import Rig

pytestmark = pytest.mark.gpu

CANARY, GUARD, MARKER = 0x5A, 256, 7
FAST, GENERAL = ((64, 8), (4, 8, 12, 16)), ((66, 6), (1, 3, 2, 8))  # (size, pads of Y, chroma, alpha and target rows)


def _up(v, a=256):
    return (v + a - 1) // a * a


def rect(arr, off, stride, rows, row):
    """A writable (rows, row) view of the bytes of a plane inside `arr`."""
    assert off >= 0 and off + (rows - 1) * stride + row <= arr.size
    return np.lib.stride_tricks.as_strided(arr[off:], shape=(rows, row), strides=(stride, 1))


class Buf:
    """One device allocation and two host images of it: `host`, what is uploaded, and `want`, what it must hold in the end."""

    def __init__(self, rig, nbytes):
        self.rig, self.n = rig, nbytes
        self.dev = rig.DeviceBuffer(rig.ctx, nbytes, placement_tries=1)
        self.ptr = self.dev.ptr
        self.clear()

    def clear(self):
        self.host = np.full(self.n, CANARY, np.uint8)
        self.want = self.host

    def upload(self):
        self.rig.upload(self.ptr, self.host)
        self.want = self.host.copy()

    def untouched(self):
        return np.array_equal(self.rig.download(self.ptr, self.n), self.host)

    def check(self, label):
        got = self.rig.download(self.ptr, self.n)
        if not np.array_equal(got, self.want):
            bad = np.flatnonzero(got != self.want)
            raise AssertionError("%s: %d bytes differ, first at offset %d of the allocation (got %d, want %d)"
                                 % (label, bad.size, bad[0], got[bad[0]], self.want[bad[0]]))

    def free(self):
        self.dev.free()


class Mem:
    """The allocations every case carves its frames and targets from: five for inputs and five for targets (sorted by address),
    a slab of each, all cleared to the canary between cases."""

    def __init__(self, rig):
        self.ins = sorted((Buf(rig, 64 << 10) for _ in range(5)), key=lambda b: b.ptr)
        self.outs = sorted((Buf(rig, 128 << 10) for _ in range(5)), key=lambda b: b.ptr)
        self.in_slab, self.out_slab = Buf(rig, 512 << 10), Buf(rig, 1 << 20)

    def all(self):
        return self.ins + self.outs + [self.in_slab, self.out_slab]

    def clear(self):
        for b in self.all():
            b.clear()

    def upload(self):
        for b in self.all():
            b.upload()

    def check(self, label):
        for k, b in enumerate(self.all()):
            b.check("%s, allocation %d" % (label, k))

    def free(self):
        for b in self.all():
            b.free()


class Geo:
    """Pitches and plane offsets of one frame and one target of `state` at w x h."""

    def __init__(self, state, size, pads, alpha_plane=None):
        self.state, (self.w, self.h) = state, size
        w, h = size
        self.px = cc.pixel_bytes(state)
        self.planar = state.layout == cc.I420
        self.has_a = state.alpha if alpha_plane is None else alpha_plane
        self.sy, self.sc, self.sa, self.so = w + pads[0], (w // 2 if self.planar else w) + pads[1], w + pads[2], self.px * w + pads[3]
        self.c_off = _up(self.sy * h)
        self.a_off = self.c_off + _up(self.sc * (h // 2) * (2 if self.planar else 1))
        self.in_bytes = self.a_off + (_up(self.sa * h) if self.has_a else 0)
        self.out_bytes = _up(self.so * h)


class Src:
    """A frame in device memory: descriptors and the planes they name.  `y_from` = (Buf, offset): the Y plane is read from there
    -- whatever those bytes hold when the call's turn comes."""

    def __init__(self, geo, buf, off, planes, y_from=None, y_stride=None):
        g, w, h = geo, geo.w, geo.h
        y, u, v, a = planes
        self.geo, self.planes, self.y_from = geo, planes, y_from
        self.sy = y_stride or g.sy
        if y_from is None:
            rect(buf.host, off, g.sy, h, w)[...] = y
        if g.planar:
            rect(buf.host, off + g.c_off, g.sc, h // 2, w // 2)[...] = u
            rect(buf.host, off + g.c_off + (h // 2) * g.sc, g.sc, h // 2, w // 2)[...] = v
        else:
            rect(buf.host, off + g.c_off, g.sc, h // 2, w)[...] = cc.interleave(u, v)
        y_ptr = y_from[0].ptr + y_from[1] if y_from else buf.ptr + off
        self.frame = Frame(y_ptr, self.sy, buf.ptr + off + g.c_off, g.sc, w, h, 1, cc.TRANSFER[g.state.gamma])
        self.alpha = None
        if g.has_a:
            rect(buf.host, off + g.a_off, g.sa, h, w)[...] = a
            self.alpha = Frame(buf.ptr + off + g.a_off, g.sa, buf.ptr + off + g.c_off, g.sc, w, h, 1, cc.TRANSFER_LINEAR)

    def current_planes(self):
        if self.y_from is None:
            return self.planes
        buf, off = self.y_from
        return (rect(buf.want, off, self.sy, self.geo.h, self.geo.w).copy(),) + tuple(self.planes[1:])


class Dst:
    """A target: `fill` (h, w, px) is what its pixels hold before anything runs (None: what the allocation holds already)."""

    def __init__(self, geo, buf, off, fill=None):
        self.geo, self.buf, self.off = geo, buf, off
        if fill is not None:
            rect(buf.host, off, geo.so, geo.h, geo.px * geo.w)[...] = fill.reshape(geo.h, geo.px * geo.w)
        self.surface = Surface(buf.ptr + off, geo.so, geo.w, geo.h, geo.state.fmt, 0)

    def pixels(self):
        return rect(self.buf.want, self.off, self.geo.so, self.geo.h, self.geo.px * self.geo.w)


class Queue:
    """A coalescing decoder, a stream of its own, and the book-keeping of what the calls made so far must leave behind."""

    def __init__(self, rig, oracle, tabs, marker, state, n=4, extra=()):
        self.rig, self.oracle, self.tabs, self.marker, self.state = rig, oracle, tabs, marker, state
        self.dec = rig.decoder(options=cc.options(state) + [(cc.OPT_COALESCE, n)] + list(extra), gamma=state.gamma, has_alpha=state.alpha)
        if state.alpha_fill != 0xFF:
            _capi.check(rig.lib.bt709hip_decoder_set_alpha_fill(self.dec, state.alpha_fill))
        if state.fmt == cc.RGBA16F:
            _capi.check(rig.lib.bt709hip_decoder_prepare_format(self.dec, cc.RGBA16F))
        self.cb = rig.ctx.commandQueue.commandBuffer(new_stream=True)
        self.S = self.cb.stream
        self.marking = True  # False while the stream records: the marker's launch waits for the device

    def mark(self):
        if self.marking:
            self.marker()

    def expect(self, src, dst, state=None):
        """Applies, to the host image, what a decode of `src` into `dst` under `state` writes -- in the order of the calls."""
        state = state or self.state
        px = dst.pixels()
        before = px.reshape(dst.geo.h, dst.geo.w, dst.geo.px).copy() if state.over == cc.OVER_DESTINATION else None
        px[...] = cc.expected(self.oracle, self.tabs, state, src.current_planes(), before).reshape(px.shape)

    def submit(self, items, issued=0, general=False, name=cc.QUEUED, rc=_capi.OK, state=None, alphas=True):
        """One call over items = [(Src, Dst)]: bt709hip_decode for one, bt709hip_decode_batch for more.  issued: the frames the call
        must launch (0: none; the frame dimension of the launch on record is checked against the marker's otherwise)."""
        self.mark()
        n = len(items)
        frames = (Frame * n)(*[s.frame for s, _ in items])
        al = (Frame * n)(*[s.alpha for s, _ in items]) if alphas and items[0][0].alpha is not None else None
        surfs = (Surface * n)(*[d.surface for _, d in items])
        if n == 1:
            got = self.rig.lib.bt709hip_decode(self.dec, frames, al, surfs, items[0][0].geo.w, items[0][0].geo.h, self.S, 0)
        else:
            got = self.rig.lib.bt709hip_decode_batch(self.dec, n, frames, al, surfs, self.S, 0)
        assert got == rc, "status %d, expected %d" % (got, rc)
        if rc == _capi.OK:
            assert self.rig.kernel() == name, self.rig.kernel()
            for s, d in items:
                self.expect(s, d, state)
        self.issued(issued, general)

    def issued(self, frames, general=False):
        grid, _, launches, _ = self.rig.launch()
        assert launches == 1, launches
        got = grid[1] if general and frames else grid[2]
        assert got == (frames or MARKER), "the launch on record holds %d frames, expected %s" % (got, frames or "none (the marker's %d)" % MARKER)

    def flush(self, issued, general=False, name=None):
        self.mark()
        _capi.check(self.rig.lib.bt709hip_decoder_flush(self.dec, self.S))
        self.issued(issued, general)
        if name is not None and issued:
            assert self.rig.kernel() == name, self.rig.kernel()
        self.rig.sync(self.S)

    def set_option(self, opt, value, issued, general=False, name=None):
        self.mark()
        _capi.check(self.rig.lib.bt709hip_decoder_set_option(self.dec, opt, value))
        self.issued(issued, general)
        if name is not None:
            assert self.rig.kernel() == name, self.rig.kernel()

    def close(self):
        self.rig.decoders.remove(self.dec)
        self.rig.lib.bt709hip_decoder_destroy(self.dec)  # what is still queued goes out on its way
        self.rig.sync(self.S)
        self.cb.release()


@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


@pytest.fixture(scope="module")
def tabs(oracle):
    return oc.tables(oracle)


@pytest.fixture(scope="module")
def rig(gh):
    r = Rig(gh)
    yield r
    r.close()


@pytest.fixture(scope="module")
def pool(rig):
    m = Mem(rig)
    yield m
    m.free()


@pytest.fixture()
def mem(pool):
    pool.clear()
    return pool


@pytest.fixture(scope="module")
def marker(rig):
    """-> a function that puts a launch of MARKER frames (4 x 2 pixels each, the context's default stream) on record."""
    w, h, n = 4, 2, MARKER
    src, dst = Buf(rig, n * 256), Buf(rig, n * 256)
    src.host[...] = 128
    src.upload()
    dec = rig.decoder(gamma=cc.GAMMA_APPLE, has_alpha=False)
    frames = (Frame * n)(*[Frame(src.ptr + 256 * i, w, src.ptr + 256 * i + 64, w, w, h, 1, cc.TRANSFER_709) for i in range(n)])
    surfs = (Surface * n)(*[Surface(dst.ptr + 256 * i, 4 * w, w, h, cc.BGRA8, 0) for i in range(n)])

    def mark():
        _capi.check(rig.lib.bt709hip_decode_batch(dec, n, frames, None, surfs, None, 1))
        grid, _, launches, _ = rig.launch()
        assert (grid[2], launches) == (MARKER, 1)
    yield mark
    src.free()
    dst.free()


def planes_for(geo, seed, n):
    return cc.random_planes(geo.w, geo.h, seed, n, alpha=geo.has_a)


def fills(geo, seed, n):
    return [cc.random_words(geo.w, geo.h, seed + i, geo.px) for i in range(n)]


# ------------------------------------------------------------------ a. every state through the queue

GEOMETRIES = {"fast": (FAST, 0), "general": (GENERAL, 0), "misaligned": (FAST, 4)}  # name -> ((size, pads), bytes the target base is off 16-byte alignment)


def lay_out(mem, geo, form, seed, out_offset):
    """-> [(Src, Dst)] in submission order.  table: five frames in allocations of their own, submitted in the address order
    0, 2, 1, 4, 3 -- no single step reaches them; slab: five, evenly spaced; step0: one frame into three targets."""
    if form == "table":
        planes, fill = planes_for(geo, seed, 5), fills(geo, seed + 100, 5)
        items = [(Src(geo, mem.ins[i], GUARD, planes[i]), Dst(geo, mem.outs[i], GUARD + out_offset, fill[i])) for i in range(5)]
        return [items[i] for i in (0, 2, 1, 4, 3)]
    if form == "slab":
        planes, fill = planes_for(geo, seed, 5), fills(geo, seed + 100, 5)
        return [(Src(geo, mem.in_slab, GUARD + i * geo.in_bytes, planes[i]),
                 Dst(geo, mem.out_slab, GUARD + out_offset + i * (geo.out_bytes + 256), fill[i])) for i in range(5)]
    planes, fill = planes_for(geo, seed, 1), fills(geo, seed + 100, 3)
    src = Src(geo, mem.in_slab, GUARD, planes[0])
    return [(src, Dst(geo, mem.out_slab, GUARD + out_offset + i * (geo.out_bytes + 256), fill[i])) for i in range(3)]


@pytest.mark.parametrize("form", ["table", "slab", "step0"])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("state", cc.STATES, ids=lambda s: s.name)
def test_state_matrix(rig, oracle, tabs, marker, mem, state, geometry, form):
    """n one-frame calls, wait = 0, COALESCE = 4: three queue, the fourth fills the queue -- one launch of four --, the fifth
    queues and the flush issues it alone; one frame into three targets: a launch of three at the flush."""
    (size, pads), off = GEOMETRIES[geometry]
    if off and state.fmt == cc.RGBA16F:
        off = 8  # a half-float texel is 8 bytes: the base cannot be 4 off, it can be 8 off the 16 the wide stores need
    geo = Geo(state, size, pads)
    general = state.fmt != cc.RGBA16F and geometry != "fast"
    name = cc.kernel(state, general)
    items = lay_out(mem, geo, form, seed=len(state.name) * 31 + size[0], out_offset=off)
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, state)
    try:
        for k, item in enumerate(items):
            if k == 3:
                assert all(b.untouched() for b in mem.outs + [mem.out_slab])  # three calls in, nothing has run
                q.submit([item], issued=4, general=general, name=name)
            else:
                q.submit([item])
        q.flush(issued=len(items) % 4, general=general, name=name)
        mem.check("%s %s %s" % (state.name, geometry, form))
    finally:
        q.close()


@pytest.mark.parametrize("state", cc.ILLEGAL, ids=lambda s: s.name)
def test_refusals_are_the_calls_own_and_leave_the_queue_alone(rig, oracle, tabs, marker, mem, state):
    """What the 1:1 decode refuses stays refused under the option, as the status of the call itself: two legal frames wait in the
    queue (BGRA8 targets; none where the options alone are the illegal pair), the refused call launches and writes nothing,
    and the two go out together at the flush."""
    legal = state._replace(fmt=cc.BGRA8)
    always = state.straight and state.over != cc.OVER_OFF
    geo, bad = Geo(legal, *FAST), Geo(state, *FAST)
    planes = planes_for(geo, 77, 3)
    items = [(Src(geo, mem.ins[i], GUARD, planes[i]), Dst(geo, mem.outs[i], GUARD, cc.random_words(64, 8, 70 + i))) for i in range(2)]
    refused = (Src(geo, mem.ins[2], GUARD, planes[2]), Dst(bad, mem.outs[2], GUARD))
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, legal)
    try:
        for item in items:
            q.submit([item], rc=_capi.ERR_UNSUPPORTED if always else _capi.OK)
        q.submit([refused], rc=_capi.ERR_UNSUPPORTED)
        q.flush(issued=0 if always else 2)
        mem.check(state.name)
    finally:
        q.close()


# ------------------------------------------------------------------ b. every term that closes a queue

APPLE, ALPHA = cc.BY_NAME["apple"], cc.BY_NAME["alpha"]
CLOSERS = {  # name -> (the queued frames' state, size, pads, alpha passed), (the differing call's)
    "width": ((APPLE, (64, 8), (4, 8, 12, 16), None), (APPLE, (60, 8), (8, 12, 16, 32), None)),  # the pitches stay what they were
    "height": ((APPLE, (64, 8), (4, 8, 12, 16), None), (APPLE, (64, 6), (4, 8, 12, 16), None)),
    "y_stride": ((APPLE, (64, 8), (4, 8, 12, 16), None), (APPLE, (64, 8), (8, 8, 12, 16), None)),
    "cbcr_stride": ((APPLE, (64, 8), (4, 8, 12, 16), None), (APPLE, (64, 8), (4, 12, 12, 16), None)),
    "target-stride": ((APPLE, (64, 8), (4, 8, 12, 16), None), (APPLE, (64, 8), (4, 8, 12, 32), None)),
    "bgra8-to-f16": ((APPLE, (64, 8), (4, 8, 12, 256 + 16), None), (cc.BY_NAME["f16"], (64, 8), (4, 8, 12, 16), None)),  # one target pitch: 528
    "f16-to-bgra8": ((cc.BY_NAME["f16"], (64, 8), (4, 8, 12, 16), None), (APPLE, (64, 8), (4, 8, 12, 256 + 16), None)),
    "alpha-stride": ((ALPHA, (64, 8), (4, 8, 12, 16), None), (ALPHA, (64, 8), (4, 8, 16, 16), None)),
    "alpha-appears": ((APPLE, (64, 8), (4, 8, 12, 16), False), (APPLE, (64, 8), (4, 8, 12, 16), True)),  # an opaque decoder validates an alpha frame and does not read it
    "alpha-goes": ((APPLE, (64, 8), (4, 8, 12, 16), True), (APPLE, (64, 8), (4, 8, 12, 16), False)),
}


@pytest.mark.parametrize("term", list(CLOSERS))
def test_a_call_that_differs_in_one_term_closes_the_queue(rig, oracle, tabs, marker, mem, term):
    """Two frames queued, then a call that differs in exactly one of the terms a launch shares among its frames: the two go out
    alone (the launch on record after the call), the third at the flush, and all three hold the right bytes."""
    (s0, size0, pads0, a0), (s1, size1, pads1, a1) = CLOSERS[term]
    g0 = Geo(s0, size0, pads0, alpha_plane=True if a0 is not None else None)
    g1 = Geo(s1, size1, pads1, alpha_plane=True if a1 is not None else None)
    if term in ("width", "height", "bgra8-to-f16", "f16-to-bgra8"):  # 60 + 8 = 64 + 4 and so on: no pitch differs
        assert (g0.sy, g0.sc, g0.so) == (g1.sy, g1.sc, g1.so)
    p0, p1 = planes_for(g0, 5, 2), planes_for(g1, 6, 1)
    items = [(Src(g0, mem.ins[i], GUARD, p0[i]), Dst(g0, mem.outs[i], GUARD, cc.random_words(g0.w, g0.h, 40 + i, g0.px))) for i in range(2)]
    third = (Src(g1, mem.ins[2], GUARD, p1[0]), Dst(g1, mem.outs[2], GUARD, cc.random_words(g1.w, g1.h, 42, g1.px)))
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, s0)
    if s1.fmt == cc.RGBA16F:
        _capi.check(rig.lib.bt709hip_decoder_prepare_format(q.dec, cc.RGBA16F))
    try:
        for item in items:
            q.submit([item], alphas=a0 is not False)
        q.submit([third], issued=2, state=s1, alphas=a1 is not False)
        q.flush(issued=1, name=cc.kernel(s1, False))
        mem.check(term)
    finally:
        q.close()


def test_a_frame_of_another_transfer_is_refused_before_it_reaches_the_queue(rig, oracle, tabs, marker, mem):
    """`transfer` is one of the terms a queue compares, but a decoder accepts one transfer tag only (BT709HIP_ERR_TRANSFER from the
    call's own validation): such a call never closes a queue, it is refused and the queue stays as it was."""
    geo = Geo(APPLE, *FAST)
    planes = planes_for(geo, 9, 3)
    items = [(Src(geo, mem.ins[i], GUARD, planes[i]), Dst(geo, mem.outs[i], GUARD)) for i in range(3)]
    items[2][0].frame.transfer = cc.TRANSFER_SRGB
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, APPLE)
    try:
        q.submit([items[0]])
        q.submit([items[1]])
        q.submit([items[2]], rc=_capi.ERR_TRANSFER)
        q.flush(issued=2, name=cc.kernel(APPLE, False))
        mem.check("transfer")
    finally:
        q.close()


def test_count_edges(rig, oracle, tabs, marker, mem):
    """COALESCE = 4.  A decode_batch of 3 arrives at a queue of 2: the queue is issued, the batch queues.  A decode_batch of 4
    (count >= n) arrives at a queue of 2: the queue is issued and the batch launched at once, behind it."""
    geo = Geo(APPLE, *FAST)
    planes = planes_for(geo, 11, 11)
    items = [(Src(geo, mem.in_slab, GUARD + i * geo.in_bytes, planes[i]),
              Dst(geo, mem.out_slab, GUARD + i * (geo.out_bytes + 256), cc.random_words(64, 8, 50 + i))) for i in range(11)]
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, APPLE)
    name = cc.kernel(APPLE, False)
    try:
        q.submit([items[0]])
        q.submit([items[1]])
        q.submit(items[2:5], issued=2)
        q.flush(issued=3, name=name)
        q.submit([items[5]])
        q.submit([items[6]])
        q.submit(items[7:11], issued=4, name=name)  # the record keeps the call's last launch: the four
        q.flush(issued=0)                           # and nothing was left behind
        mem.check("count edges")
    finally:
        q.close()


# ------------------------------------------------------------------ c. a state change between queued calls

CHANGES = {  # name -> (state before, state after, how to get there: ("fill", byte) or (option, value))
    "alpha-fill": (APPLE, cc.BY_NAME["apple-fill0"], ("fill", 0)),
    "unpremultiply": (ALPHA, cc.BY_NAME["straight"], (cc.OPT_UNPREMULTIPLY, 1)),
    "colour-to-destination": (cc.BY_NAME["over-colour"], cc.BY_NAME["over-destination"], (cc.OPT_COMPOSITE_OVER, cc.OVER_DESTINATION)),
    "nv12-to-i420": (APPLE, cc.BY_NAME["i420"], (cc.OPT_CHROMA_LAYOUT, cc.I420)),
    "nontemporal": (APPLE, APPLE._replace(fast="quads"), (cc.OPT_NONTEMPORAL, 0)),
    "xcd-bands": (APPLE, APPLE, (cc.OPT_XCD_BANDS, 0)),
}


@pytest.mark.parametrize("change", list(CHANGES))
def test_a_state_change_divides_the_queue(rig, oracle, tabs, marker, mem, change):
    """Two frames queued, the state changed, two more: the change issues the first pair under the state it was submitted with
    (the launch on record, and its kernel), the second pair carries the new state's bytes."""
    before, after, (opt, value) = CHANGES[change]
    g0, g1 = Geo(before, *FAST), Geo(after, *FAST)
    p0, p1 = planes_for(g0, 21, 2), planes_for(g1, 22, 2)
    first = [(Src(g0, mem.ins[i], GUARD, p0[i]), Dst(g0, mem.outs[i], GUARD, cc.random_words(64, 8, 60 + i))) for i in range(2)]
    second = [(Src(g1, mem.ins[2 + i], GUARD, p1[i]), Dst(g1, mem.outs[2 + i], GUARD, cc.random_words(64, 8, 62 + i))) for i in range(2)]
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, before)
    try:
        for item in first:
            q.submit([item])
        if opt == "fill":
            q.mark()
            _capi.check(rig.lib.bt709hip_decoder_set_alpha_fill(q.dec, value))
            q.issued(2)
            assert rig.kernel() == cc.kernel(before, False)
        else:
            q.set_option(opt, value, issued=2, name=cc.kernel(before, False))
        for item in second:
            q.submit([item], state=after)
        q.flush(issued=2, name=cc.kernel(after, False))
        mem.check(change)
    finally:
        q.close()


# ------------------------------------------------------------------ d. calls that share bytes keep their order

BIG = ((256, 64), (0, 0, 0, 0))  # 32 row pairs x 64 quads a frame: one launch holds many workgroups


@pytest.mark.parametrize("path", ["fast", "general"])
@pytest.mark.parametrize("n", [2, 4])
def test_decodes_into_one_surface_leave_the_last_frame(rig, oracle, tabs, marker, mem, n, path):
    """No call between them: each call finds its predecessor queued for the same surface and issues it, alone."""
    geo = Geo(APPLE, *BIG)
    general = path == "general"
    planes = planes_for(geo, 31, n)
    dst = Dst(geo, mem.outs[0], GUARD + (4 if general else 0), cc.random_words(256, 64, 30))
    srcs = [Src(geo, mem.ins[i], GUARD, planes[i]) for i in range(n)]
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, APPLE)
    try:
        for i, src in enumerate(srcs):
            q.submit([(src, dst)], issued=1 if i else 0, general=general)
        q.flush(issued=1, general=general, name=cc.kernel(APPLE, general))
        mem.check("%d frames into one surface" % n)
        assert np.array_equal(dst.pixels().reshape(64, 256, 4), cc.expected(oracle, tabs, APPLE, planes[-1]))
    finally:
        q.close()


def layered(mem, geo, seed):
    """Three alpha clips for one canvas (mem.outs[0]); -> (the canvas as a target, [Src])."""
    planes = planes_for(geo, seed, 3)
    return Dst(geo, mem.outs[0], GUARD, cc.random_words(geo.w, geo.h, seed + 1)), [Src(geo, mem.ins[i], GUARD, planes[i]) for i in range(3)]


def test_clips_layered_over_one_canvas_fold_in_call_order(rig, oracle, tabs, marker, mem):
    state = cc.BY_NAME["over-destination"]
    geo = Geo(state, *BIG)
    canvas, clips = layered(mem, geo, 41)
    start = rect(canvas.buf.host, canvas.off, geo.so, geo.h, 4 * geo.w).reshape(geo.h, geo.w, 4).copy()
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, state)
    try:
        for i, clip in enumerate(clips):
            q.submit([(clip, canvas)], issued=1 if i else 0)
        q.flush(issued=1, name=cc.kernel(state, False))
        mem.check("three clips over one canvas")
        fold = start
        for clip in clips:  # the definition, spelt out: composite_over folded in call order
            fold = oc.composite_over(oracle.decode_nv12(cc.GAMMA_SRGB, clip.planes[0], cc.interleave(*clip.planes[1:3]), alpha=clip.planes[3]).reshape(geo.h, geo.w, 4),
                                     fold, *tabs)
        assert np.array_equal(canvas.pixels().reshape(geo.h, geo.w, 4), fold)
    finally:
        q.close()


def test_a_target_four_rows_down_the_same_canvas(rig, oracle, tabs, marker, mem):
    geo = Geo(APPLE, *BIG)
    planes = planes_for(geo, 43, 2)
    a = (Src(geo, mem.ins[0], GUARD, planes[0]), Dst(geo, mem.outs[0], GUARD))
    b = (Src(geo, mem.ins[1], GUARD, planes[1]), Dst(geo, mem.outs[0], GUARD + 4 * geo.so))
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, APPLE)
    try:
        q.submit([a])
        q.submit([b], issued=1)
        q.flush(issued=1)
        mem.check("partial overlap")
    finally:
        q.close()


@pytest.mark.parametrize("order", ["read-after-write", "write-after-read"])
def test_a_target_that_is_also_a_frame(rig, oracle, tabs, marker, mem, order):
    """Read after write: call 1 decodes into X, call 2 names bytes inside X as its Y plane and decodes into Z -- Z is the decode of
    what call 1 wrote.  Write after read: call 1 reads its Y plane from X (random words), call 2 overwrites X -- Z is the decode
    of what X held."""
    geo = Geo(APPLE, *BIG)
    planes = planes_for(geo, 47, 2)
    x = Dst(geo, mem.outs[0], GUARD, cc.random_words(256, 64, 48))
    z = Dst(geo, mem.outs[1], GUARD)
    plain = Src(geo, mem.ins[0], GUARD, planes[0])
    reads_x = Src(geo, mem.ins[1], GUARD, planes[1], y_from=(mem.outs[0], GUARD + 8 * geo.so + 64), y_stride=256)
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, APPLE)
    try:
        calls = [(plain, x), (reads_x, z)] if order == "read-after-write" else [(reads_x, z), (plain, x)]
        q.submit([calls[0]])
        q.submit([calls[1]], issued=1)
        q.flush(issued=1)
        mem.check(order)
    finally:
        q.close()


def test_a_wall_of_four_windows_is_one_launch(rig, oracle, tabs, marker, mem):
    """Four 64 x 8 windows of one 128 x 16 canvas, all with the canvas's pitch: disjoint rectangles whose byte ranges interleave.
    Nothing conflicts: the fourth call fills the queue and the four go out together."""
    geo = Geo(APPLE, (64, 8), (0, 0, 0, 256))  # the target pitch: 128 pixels
    planes = planes_for(geo, 53, 4)
    canvas = cc.random_words(128, 16, 54)
    rect(mem.outs[0].host, GUARD, 512, 16, 512)[...] = canvas.reshape(16, 512)
    items = [(Src(geo, mem.ins[i], GUARD, planes[i]), Dst(geo, mem.outs[0], GUARD + (i // 2) * 8 * 512 + (i % 2) * 256)) for i in range(4)]
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, APPLE)
    try:
        for i, item in enumerate(items):
            q.submit([item], issued=4 if i == 3 else 0, name=cc.kernel(APPLE, False) if i == 3 else cc.QUEUED)
        q.flush(issued=0)
        mem.check("wall")
    finally:
        q.close()


def test_layered_sequence_recorded_into_a_graph(rig, oracle, tabs, marker, mem):
    """The three clips between beginRecording and endRecording: one stream, so the kernel nodes stand in a row, no parallel
    branches.  No marker launch can be made while the stream records, so a clip for a target of its own rides along: the
    launches on record then read none, none, 2, 1 -- each call's distinguishable from the one before.  Nothing runs while
    recording; the canvas is refilled and the graph replayed once: the layered result, over the new canvas."""
    state = cc.BY_NAME["over-destination"]
    geo = Geo(state, *BIG)
    canvas, clips = layered(mem, geo, 59)
    aside = Dst(geo, mem.outs[1], GUARD, cc.random_words(geo.w, geo.h, 60))
    calls = [(clips[0], canvas), (clips[1], aside), (clips[1], canvas), (clips[2], canvas)]
    mem.upload()
    q = Queue(rig, oracle, tabs, marker, state)
    rec = None
    try:
        q.mark()
        q.marking = False
        q.cb.beginRecording()
        for call, issued in zip(calls, (0, 0, 2, 1)):
            q.submit([call], issued=issued)
        rec = q.cb.endRecording()  # the last clip is recorded by the end of the capture
        q.marking = True
        assert all(b.untouched() for b in mem.outs)
        for dst, seed in ((canvas, 61), (aside, 62)):
            rect(dst.buf.host, dst.off, geo.so, geo.h, 4 * geo.w)[...] = cc.random_words(geo.w, geo.h, seed).reshape(geo.h, 4 * geo.w)
        mem.upload()  # the refill; the expectation starts again from it
        for clip, dst in calls:
            q.expect(clip, dst)
        rec.replay(q.cb)
        q.cb.waitUntilCompleted()
        mem.check("graph replay")
    finally:
        if rec is not None:
            rec.release()
        q.close()
