"""GPU tests (-m gpu) of BT709HIP_OPT_COMPOSITE_OVER: an alpha decoder's 1:1 decode blended over a solid colour or over what the
target holds, inside the decode kernel.  Everything goes through the C ABI; every output byte -- row padding and guard bands
included -- is compared with tests/over_cases.py composite_over on the oracle's decode."""
import ctypes as C

import numpy as np
import pytest

import over_cases as oc
from metalbt709decoder_amd import _capi
from variant_cases import Job, Rig, assert_equal, random_backgrounds, random_planes

pytestmark = pytest.mark.gpu

OPT = _capi.OPT_COMPOSITE_OVER
DEST = _capi.OVER_DESTINATION
NAME = {("quads", True): b"decode_nv12_quads<alpha,over>", ("quads", False): b"decode_nv12_quads<alpha,over-colour>",
        ("blocks", True): b"decode_nv12_blocks<alpha,over>", ("blocks", False): b"decode_nv12_blocks<alpha,over-colour>"}


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


def want_over(oracle, tabs, planes, background):
    return oc.composite_over(oc.expected_source(oracle, *planes), background, *tabs)


# ------------------------------------------------------------------ 1. arithmetic sweep

@pytest.fixture(scope="module")
def sweep(oracle, tabs):
    """Every alpha-frame code x every background byte x the source triples S (every byte value in each of R, G and B).
    A 4096-wide row holds the 256 alpha codes (x & 255) sixteen times over; x >> 8 is the low part of the second index."""
    triples, words = oc.covering_triples(oracle)
    assert len(triples) <= 768
    for c in range(3):
        assert np.unique(words[:, c]).size == 256  # the coverage the sweep claims
    table, alpha_table = oc.channel_table(*tabs)
    a_row = (np.arange(4096) & 255).astype(np.uint8)
    # A_s of every alpha-frame code, from the oracle: a grey frame whose alpha plane is the ramp
    a_s = oc.expected_source(oracle, np.full((2, 4096), 128, np.uint8), np.full((1, 4096), 128, np.uint8), np.stack([a_row, a_row]))[0, :, 3]
    return dict(triples=triples, words=words, table=table, alpha_table=alpha_table, a_row=a_row, a_s=a_s)


def test_arithmetic_sweep_over_the_destination(rig, sweep, oracle, tabs):
    """One uniform batch: frame t = triple t, 4096 x 16; pixel (r, x): alpha code x & 255, background byte d = (x >> 8) + 16 r as
    the word (d, d, d, A_d = 255 - d)."""
    triples, words, n = sweep["triples"], sweep["words"], len(sweep["triples"])
    w, h = 4096, 16
    a = np.broadcast_to(sweep["a_row"], (h, w))
    planes = [(np.full((h, w), t[0], np.uint8), np.tile(np.array([t[1], t[2]], np.uint8), (h // 2, w // 2)), a) for t in triples]
    d = ((np.arange(w) >> 8)[None, :] + 16 * np.arange(h)[:, None]).astype(np.uint8)
    bg = np.stack([d, d, d, 255 - d], -1)
    job = Job(rig, planes)
    try:
        job.fill([bg] * n)
        dec = rig.decoder(DEST)
        _capi.check(job.decode_batch(dec))
        assert rig.kernel() == NAME["quads", True]
        got = np.stack(job.collect("sweep, destination"))  # (n, h, w, 4)
    finally:
        job.free()
    a_s = np.broadcast_to(sweep["a_s"], (h, w))
    want = np.empty_like(got)
    for c in range(3):
        want[..., c] = sweep["table"][a_s[None], d[None], words[:, c][:, None, None]]
    want[..., 3] = sweep["alpha_table"][a_s, 255 - d][None]
    # the tabulated definition IS the definition: three whole frames through composite_over itself
    for t in (0, n // 2, n - 1):
        assert np.array_equal(want[t], want_over(oracle, tabs, planes[t], bg))
    for t in range(n):
        assert_equal(got[t], want[t], "sweep over the destination, triple %s" % (triples[t],))


def test_arithmetic_sweep_over_a_colour(rig, sweep, oracle, tabs):
    """Per background byte d one launch over the colour (d, d, d): a uniform batch of 4096 x 2 frames; pixel x of frame f: alpha
    code x & 255, triple (x >> 8) + 16 f (the last frame wraps round to the first triples)."""
    triples, words, n = sweep["triples"], sweep["words"], len(sweep["triples"])
    w, h = 4096, 2
    frames = (n + 15) // 16
    a = np.broadcast_to(sweep["a_row"], (h, w))
    index = ((np.arange(w) >> 8)[None, :] + 16 * np.arange(frames)[:, None]) % n  # (frames, w): the triple of a pixel
    planes = []
    for f in range(frames):
        t = triples[index[f]]
        uv = np.empty((1, w), np.uint8)
        uv[0, 0::2], uv[0, 1::2] = t[0::2, 1], t[0::2, 2]
        planes.append((np.broadcast_to(t[:, 0], (h, w)), uv, a))
    job = Job(rig, planes)
    dec = rig.decoder(0)
    got = []
    try:
        for d in range(256):
            rig.set_over(dec, d << 16 | d << 8 | d)
            _capi.check(job.decode_batch(dec, wait=0))
            assert rig.kernel() == NAME["quads", False]
            got.append(np.stack(job.collect("sweep, colour %d" % d)))  # (frames, h, w, 4)
    finally:
        job.free()
    a_s = np.broadcast_to(sweep["a_s"], (frames, h, w))
    s = np.broadcast_to(words[index][:, None, :, :], (frames, h, w, 4))
    for f in (0, frames - 1):  # the tabulated definition is the definition
        assert np.array_equal(np.stack([sweep["table"][a_s[f], 77, s[f, ..., c]] for c in range(3)] + [np.full((h, w), 255, np.uint8)], -1),
                              want_over(oracle, tabs, planes[f], 77 << 16 | 77 << 8 | 77))
    for d in range(256):
        want = np.stack([sweep["table"][a_s, d, s[..., c]] for c in range(3)] + [np.full((frames, h, w), 255, np.uint8)], -1)
        for f in range(frames):
            assert_equal(got[d][f], want[f], "sweep over the colour (%d, %d, %d), frame %d" % (d, d, d, f))


# ------------------------------------------------------------------ 2. geometry

GEOMETRY = [  # (w, h), pads of (Y, CbCr, alpha, output) rows, output pointer offset, path
    ((8, 4), (4, 8, 12, 16), 0, "quads"),       # the smallest fast-path frames
    ((4, 2), (4, 8, 12, 16), 0, "quads"),
    ((260, 6), (4, 8, 12, 16), 0, "quads"),     # 65 quads: a tile tail
    ((1028, 4), (4, 8, 12, 16), 0, "quads"),    # a wide row: 257 quads, two per lane
    ((6, 2), (1, 3, 2, 4), 0, "blocks"),        # the smallest general-path frame
    ((1022, 4), (1, 3, 2, 8), 4, "blocks"),     # an output that is only 4-byte aligned
]


@pytest.mark.parametrize("mode", ["destination", "colour"])
@pytest.mark.parametrize("size,pads,out_offset,path", GEOMETRY, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) and len(v) == 2 else None)
def test_geometry(rig, oracle, tabs, size, pads, out_offset, path, mode):
    """Padded pitches on all four planes, the padding of the target pre-filled with a canary: it comes back untouched, the pixels
    come back blended (destination mode) / over the colour, whatever they held."""
    w, h = size
    planes = random_planes(w, h, seed=w * 7 + h)
    bg = random_backgrounds(w, h, seed=w * 11 + h)
    colour = 0x3C7FB2
    job = Job(rig, planes, pads=pads, out_offset=out_offset)
    try:
        job.fill(bg)
        dec = rig.decoder(DEST if mode == "destination" else colour)
        _capi.check(job.decode_one(dec))
        assert rig.kernel() == NAME[path, mode == "destination"]
        got = job.collect("%dx%d %s" % (w, h, mode))[0]
    finally:
        job.free()
    assert_equal(got, want_over(oracle, tabs, planes[0], bg[0] if mode == "destination" else colour), "%dx%d %s" % (w, h, mode))


# ------------------------------------------------------------------ 3. destination over a fill == colour mode

def test_destination_over_a_uniform_fill_equals_colour_mode(rig, oracle, tabs):
    w, h = 64, 8
    planes = random_planes(w, h, seed=3)
    job = Job(rig, planes)
    try:
        for colour in (0, 0xFFFFFF, 0x10C0F8):
            job.fill([np.broadcast_to(oc.colour_word(colour), (h, w, 4))])
            _capi.check(job.decode_one(rig.decoder(DEST)))
            over_fill = job.collect()[0]
            job.fill(random_backgrounds(w, h, seed=colour & 0xFF))  # colour mode does not read the target
            _capi.check(job.decode_one(rig.decoder(colour)))
            over_colour = job.collect()[0]
            assert_equal(over_fill, over_colour, "fill %06x" % colour)
            assert_equal(over_colour, want_over(oracle, tabs, planes[0], colour), "colour %06x" % colour)
    finally:
        job.free()


# ------------------------------------------------------------------ 4. batches

@pytest.mark.parametrize("n,spacing,launches", [(72, "even", 1), (76, "even", 2), (3, "table", 1)], ids=["uniform-72", "uniform-76", "table-3"])
def test_batches_over_per_frame_destinations(rig, oracle, tabs, n, spacing, launches):
    """Evenly spaced frames under the XCD-band map (bt709_launch.h plan_bands): 72, a multiple of 8, go out as ONE banded launch
    of nine frames per XCD class; 76 as 72 under the map and a tail of 4 under the plain one, two launches, so both branches of
    the launcher's split carry the option.  3 frames that no single step reaches: the pointer table.  Every frame over a
    background of its own."""
    w, h = 64, 8
    planes = random_planes(w, h, seed=n, n=n)
    bg = random_backgrounds(w, h, seed=n + 1, n=n)
    job = Job(rig, planes, spacing=spacing)
    try:
        job.fill(bg)
        _capi.check(job.decode_batch(rig.decoder(DEST)))
        assert rig.kernel() == NAME["quads", True]
        info = _capi.LaunchInfo()
        _capi.check(rig.lib.bt709hip_last_launch_info(C.byref(info)))
        assert (info.launches, info.xcd_bands != 0) == (launches, spacing == "even")
        got = job.collect("batch of %d" % n)
    finally:
        job.free()
    for i in range(n):
        assert_equal(got[i], want_over(oracle, tabs, planes[i], bg[i]), "frame %d of %d" % (i, n))


# ------------------------------------------------------------------ 5. coalescing

def test_coalescing_submit_carries_the_value_the_frames_were_queued_under(rig, oracle, tabs):
    """The frames are queued on a stream of their own: the test's uploads and downloads run on the context's default stream,
    and every call that takes a stream issues what is queued for THAT stream first."""
    w, h = 64, 8
    planes = random_planes(w, h, seed=21, n=4)
    a_colour, b_colour = 0x204060, 0xE0A010
    job = Job(rig, planes)
    cb = rig.ctx.commandQueue.commandBuffer(new_stream=True)
    S = cb.stream
    try:
        direct = rig.decoder(a_colour)
        for i in range(4):
            _capi.check(job.decode_one(direct, i))
        want = job.collect("direct")
        for i in range(4):
            assert_equal(want[i], want_over(oracle, tabs, planes[i], a_colour), "direct %d" % i)
        # four queued decodes: the fourth fills the queue, one launch over the four
        job.fill(None)
        dec = rig.decoder(a_colour, options=[(_capi.OPT_COALESCE, 4)])
        for i in range(3):
            _capi.check(job.decode_one(dec, i, stream=S, wait=0))
            assert rig.kernel() == b"(queued: coalescing submit)"
        assert job.untouched()  # nothing has run
        _capi.check(job.decode_one(dec, 3, stream=S, wait=0))
        assert rig.kernel() == NAME["quads", False]
        _capi.check(rig.lib.bt709hip_decoder_flush(dec, S))
        rig.sync(S)
        got = job.collect("coalesced")
        for i in range(4):
            assert_equal(got[i], want[i], "coalesced %d" % i)
        # two frames, another colour, two more: the change issues the first two under the colour they were queued with
        job.fill(None)
        for i in (0, 1):
            _capi.check(job.decode_one(dec, i, stream=S, wait=0))
        assert rig.kernel() == b"(queued: coalescing submit)"
        rig.set_over(dec, b_colour)
        assert rig.kernel() == NAME["quads", False]  # the option's change flushed the queue
        for i in (2, 3):
            _capi.check(job.decode_one(dec, i, stream=S, wait=0))
        _capi.check(rig.lib.bt709hip_decoder_flush(dec, S))
        rig.sync(S)
        got = job.collect("coalesced, two colours")
        for i in range(4):
            assert_equal(got[i], want_over(oracle, tabs, planes[i], a_colour if i < 2 else b_colour), "two colours %d" % i)
    finally:
        cb.release()
        job.free()


# ------------------------------------------------------------------ 6. refusals

def test_refusals_leave_the_targets_untouched(rig, oracle):
    """The option is the 1:1 path's into BGRA8 targets: an RGBA16F target, the 2:1 and the any-ratio decode answer
    ERR_UNSUPPORTED after their usual validation and write nothing; with the option off again the decoder is the plain one."""
    w, h = 64, 8
    planes = random_planes(w, h, seed=5)
    dec = rig.decoder(DEST)
    lib = rig.lib
    jobs = [Job(rig, planes, fmt=_capi.FORMAT_RGBA16F), Job(rig, planes, out_size=(w // 2, h // 2)), Job(rig, planes, out_size=(48, 6)), Job(rig, planes)]
    try:
        f16, half, scaled, plain = jobs
        for value in (DEST, 0xFFFFFF):
            rig.set_over(dec, value)
            assert f16.decode_one(dec) == _capi.ERR_UNSUPPORTED and f16.decode_batch(dec) == _capi.ERR_UNSUPPORTED
            assert lib.bt709hip_decode_half(dec, half.frames, half.alphas, half.surfs, None, 1) == _capi.ERR_UNSUPPORTED
            assert lib.bt709hip_decode_half_batch(dec, 1, half.frames, half.alphas, half.surfs, None, 1) == _capi.ERR_UNSUPPORTED
            assert lib.bt709hip_decode_scaled(dec, scaled.frames, scaled.alphas, scaled.surfs, None, 1) == _capi.ERR_UNSUPPORTED
            assert lib.bt709hip_decode_scaled_batch(dec, 1, scaled.frames, scaled.alphas, scaled.surfs, None, 1) == _capi.ERR_UNSUPPORTED
            # the usual validation still comes first: a frame without its alpha buffer
            assert lib.bt709hip_decode_half(dec, half.frames, None, half.surfs, None, 1) == _capi.ERR_INVALID_ARG
            rig.sync()
            assert f16.untouched() and half.untouched() and scaled.untouched()
        rig.set_over(dec, _capi.OVER_OFF)
        _capi.check(plain.decode_one(dec))
        assert rig.kernel() == b"decode_nv12_quads<alpha>"
        assert_equal(plain.collect("option off")[0], oc.expected_source(oracle, *planes[0]), "option off")
        _capi.check(lib.bt709hip_decode_half(dec, half.frames, half.alphas, half.surfs, None, 1))  # and the other paths are back
    finally:
        for j in jobs:
            j.free()


# ------------------------------------------------------------------ 7. graphs

def test_graph_replays_over_a_refilled_canvas_and_refuses_a_missing_table(rig, oracle, tabs):
    w, h = 64, 8
    planes = random_planes(w, h, seed=8)
    job = Job(rig, planes)
    cb = rig.ctx.commandQueue.commandBuffer(new_stream=True)
    rec = None
    try:
        dec = rig.decoder(DEST)  # the option first, then bt709hip_decoder_setup: the table is there before the capture
        cb.beginRecording()
        _capi.check(job.decode_one(dec, stream=cb.stream, wait=0))
        rec = cb.endRecording()
        assert job.untouched()  # recorded, not run
        for seed in (1, 2):
            bg = random_backgrounds(w, h, seed=seed)
            job.fill(bg)
            rec.replay(cb)
            cb.waitUntilCompleted()
            assert_equal(job.collect("replay %d" % seed)[0], want_over(oracle, tabs, planes[0], bg[0]), "replay %d" % seed)
        # a decoder that is set up but has never seen the option: its first composite decode may not build the table in a capture
        job.fill(None)
        late = rig.decoder()
        rig.set_over(late, DEST)
        cb.beginRecording()
        assert job.decode_one(late, stream=cb.stream, wait=0) == _capi.ERR_NOT_SETUP
        cb.endRecording().release()
        # and a fresh one, whose setup has not run at all
        fresh = rig.decoder(DEST, setup=False)
        cb.beginRecording()
        assert job.decode_one(fresh, stream=cb.stream, wait=0) == _capi.ERR_NOT_SETUP
        cb.endRecording().release()
        assert job.untouched()
        # outside a capture both build what they miss; bt709hip_decoder_setup does it for a decoder that is set up already
        _capi.check(rig.lib.bt709hip_decoder_setup(late))
        bg = random_backgrounds(w, h, seed=3)
        for d in (late, fresh):
            job.fill(bg)
            _capi.check(job.decode_one(d, stream=cb.stream, wait=1))
            assert_equal(job.collect()[0], want_over(oracle, tabs, planes[0], bg[0]), "after the capture")
    finally:
        if rec is not None:
            rec.release()
        cb.release()
        job.free()
