"""GPU tests (-m gpu) of BT709HIP_OPT_SCALED_OVER: an alpha decoder's fused decode + rescale blended over the
destination or a colour inside the rescale kernel.  Everything goes through the C ABI.  Expected bytes, everywhere:

    composite_over(W, background, *tables(oracle))          W: the oracle's option-off view of the same frames

(tests/scaled_over_cases.py), every output byte compared -- row padding and 256-byte guard bands, pre-filled with a canary,
included.  Colour mode blends over 0x3C7FB2."""
import ctypes as C

import numpy as np
import pytest

import metalbt709decoder_amd as mb
import over_cases as oc
import scaled_over_cases as sc
from metalbt709decoder_amd import _capi
from scaled_over_cases import COLOUR, DEST, F16, INTERMEDIATES, MODES, OPT, SRGB8
from test_scaled_f16_gpu import SHAPE, SHAPES, SPACINGS, _planes
from variant_cases import Job, Rig, assert_equal, random_backgrounds, random_planes

pytestmark = pytest.mark.gpu

OPT9, OPT_INTER = _capi.OPT_COMPOSITE_OVER, _capi.OPT_SCALE_INTERMEDIATE
IDS = [tag for tag, _ in INTERMEDIATES]
FORMATS = [fmt for _, fmt in INTERMEDIATES]


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


def _decoder(rig, over, intermediate=SRGB8, over9=None, setup=True):
    """An alpha decoder with option 10 at `over` (None: untouched), the intermediate, and option 9 at `over9`."""
    options = [(OPT_INTER, intermediate)] + ([(OPT, over)] if over is not None else [])
    return rig.decoder(over9, options=options, setup=setup)


def _scaled(job, dec, i=None, stream=None, wait=1, entry="bt709hip_decode_scaled"):
    """bt709hip_decode_scaled / _half on frame i of a job, or the _batch form over all of them (i None)."""
    lib = job.rig.lib
    if i is None:
        return getattr(lib, entry + "_batch")(dec, job.n, job.frames, job.alphas, job.surfs, stream, wait)
    return getattr(lib, entry)(dec, C.byref(job.frames[i]), C.byref(job.alphas[i]), C.byref(job.surfs[i]), stream, wait)


def _background(mode, canvas):
    return canvas if mode == "destination" else COLOUR


def _value(mode):
    return DEST if mode == "destination" else COLOUR


# ------------------------------------------------------------------ 1. every tap form, both launch kinds

_views = {}


def _view(oracle, shape, i, intermediate):
    key = (shape, i, intermediate)
    if key not in _views:
        ow, oh = SHAPE[shape][2]
        _views[key] = sc.option_off_view(oracle, _planes(shape, i), ow, oh, intermediate)
    return _views[key]


@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_every_tap_form_and_launch_kind(gh, oracle, tabs, shape):
    """The eight shapes of the RGBA16F-intermediate tests in their layouts, {destination, colour} x {BGRA8_SRGB, RGBA16F
    intermediate}, one frame per launch -- `once` and `wide` also as three frames, evenly spaced and through the pointer table.
    Every frame over a canvas of its own (random words, A_d included; colour mode must not read it).  The launch record names the
    shape's tap form; the 8-bit kernel's by-wave forms are dispatched by the hardware, everything else runs the item loop."""
    OverBatch = sc.over_batch_class()
    _, _, (ow, oh), _, taps = SHAPE[shape]
    spacings = SPACINGS if shape in ("once", "wide") else SPACINGS[:1]
    assert [s[0] for s in spacings][:1] == ["x1"]
    for itag, intermediate in INTERMEDIATES:
        for mode in MODES:
            dec = gh.make_decoder(mb.MetalBT709GammaSRGB, has_alpha=True, options={OPT_INTER: intermediate, OPT: _value(mode)})
            for tag, count, spacing in spacings:
                label = "%s %s %s %s" % (shape, itag, mode, tag)
                canvases = [sc.canvas(ow, oh, i) for i in range(count)]
                want = []
                for i in range(count):
                    view = _view(oracle, shape, i, intermediate)
                    want.append(oc.composite_over(view, _background(mode, canvases[i]), *tabs))
                    sc.assert_the_blend_shows(view, want[i], "%s frame %d" % (label, i))  # the bar, on the oracle's arrays
                batch = OverBatch(gh, shape, mb.MetalBT709GammaSRGB, True, count, spacing)
                batch.fill(canvases)
                name, plan = batch.launch(dec)
                assert name == sc.kernel_name(intermediate, mode == "destination"), (label, name)
                assert plan["taps"] in taps and plan["block"] == (256, 1, 1), (label, plan)
                by_wave = plan["taps"] in ("once", "shared")
                assert plan["persistent"] == (1 if intermediate == F16 or not by_wave else 0), (label, plan)
                assert plan["items"] == -(-ow // 256) * (-(-oh // plan["rows"])) * count, (label, plan)
                batch.views(label, [w.reshape(oh, 4 * ow) for w in want])


# ------------------------------------------------------------------ 2. the epilogue's arithmetic, exhaustive over its inputs

@pytest.fixture(scope="module")
def sweep(oracle, tabs):
    """Every alpha-frame code x every background byte x the covering triples (every byte value in each of R, G and B), as in
    tests/test_over_gpu.py.  At identity size the option-off view is a flat function of a pixel's own inputs (fx = fy = 0: the
    filter's sum is its first tap plus exact zeros), so the tabulated definition carries over -- with s and A_s taken from the
    ORACLE's option-off view: source(intermediate)[t, a] is its word for triple t under alpha code a."""
    triples, _ = oc.covering_triples(oracle)
    n = len(triples)
    assert n <= 768
    table, alpha_table = oc.channel_table(*tabs)
    a_row = (np.arange(4096) & 255).astype(np.uint8)
    sources = {}

    def source(intermediate):
        if intermediate not in sources:  # one 256-wide frame, row pair t = triple t, column a = alpha code a
            y = np.repeat(triples[:, 0], 2)[:, None].repeat(256, 1)
            uv = np.tile(triples[:, 1:3], (1, 128))
            a = np.broadcast_to(np.arange(256, dtype=np.uint8), (2 * n, 256))
            sources[intermediate] = sc.option_off_view(oracle, (y, uv, a), 256, 2 * n, intermediate)[0::2].copy()
            if intermediate == SRGB8:  # the view holds the decoded bytes themselves: the coverage the sweep claims
                for c in range(3):
                    assert np.unique(sources[intermediate][..., c]).size == 256
        return sources[intermediate]

    return dict(triples=triples, table=table, alpha_table=alpha_table, a_row=a_row, source=source)


@pytest.mark.parametrize("intermediate", FORMATS, ids=IDS)
def test_arithmetic_sweep_over_the_destination(rig, sweep, oracle, tabs, intermediate):
    """One uniform batch at identity size: frame t = triple t, 4096 x 16 -> 4096 x 16; pixel (r, x): alpha code x & 255,
    background byte d = (x >> 8) + 16 r as the word (d, d, d, A_d = 255 - d)."""
    triples, n = sweep["triples"], len(sweep["triples"])
    w, h = 4096, 16
    a = np.broadcast_to(sweep["a_row"], (h, w))
    planes = [(np.full((h, w), t[0], np.uint8), np.tile(np.array([t[1], t[2]], np.uint8), (h // 2, w // 2)), a) for t in triples]
    d = ((np.arange(w) >> 8)[None, :] + 16 * np.arange(h)[:, None]).astype(np.uint8)
    bg = np.stack([d, d, d, 255 - d], -1)
    job = Job(rig, planes, out_size=(w, h))
    try:
        job.fill([bg] * n)
        _capi.check(_scaled(job, _decoder(rig, DEST, intermediate)))
        assert rig.kernel() == sc.kernel_name(intermediate, True)
        got = np.stack(job.collect("sweep, destination"))  # (n, h, w, 4)
    finally:
        job.free()
    s = sweep["source"](intermediate)[:, sweep["a_row"]]  # (n, w, 4): the option-off word of column x of frame t
    a_s = s[:, None, :, 3]
    want = np.empty_like(got)
    for c in range(3):
        want[..., c] = sweep["table"][a_s, d[None], s[:, None, :, c]]
    want[..., 3] = sweep["alpha_table"][a_s, (255 - d)[None]]
    # the tabulated definition IS the definition: three whole frames through the oracle's view and composite_over itself
    for t in (0, n // 2, n - 1):
        assert np.array_equal(want[t], sc.want_over(oracle, tabs, planes[t], w, h, intermediate, bg))
    for t in range(n):
        assert_equal(got[t], want[t], "sweep over the destination, triple %s" % (triples[t],))


def test_arithmetic_sweep_over_a_colour(rig, sweep, oracle, tabs):
    """8-bit intermediate.  Per background byte d one launch over the colour (d, d, d): a uniform batch of 4096 x 2 frames at
    identity size; pixel x of frame f: alpha code x & 255, triple (x >> 8) + 16 f (the last frame wraps round)."""
    triples, n = sweep["triples"], len(sweep["triples"])
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
    job = Job(rig, planes, out_size=(w, h))
    dec = _decoder(rig, 0)
    got = []
    try:
        for d in range(256):
            _capi.check(rig.lib.bt709hip_decoder_set_option(dec, OPT, d << 16 | d << 8 | d))
            _capi.check(_scaled(job, dec, wait=0))
            assert rig.kernel() == sc.kernel_name(SRGB8, False)
            got.append(np.stack(job.collect("sweep, colour %d" % d)))  # (frames, h, w, 4)
    finally:
        job.free()
    s = sweep["source"](SRGB8)[index, sweep["a_row"][None, :]]  # (frames, w, 4)
    s = np.broadcast_to(s[:, None], (frames, h, w, 4))
    a_s = s[..., 3]
    for f in (0, frames // 2, frames - 1):  # the tabulated definition is the definition
        assert np.array_equal(np.stack([sweep["table"][a_s[f], 77, s[f, ..., c]] for c in range(3)] + [np.full((h, w), 255, np.uint8)], -1),
                              sc.want_over(oracle, tabs, planes[f], w, h, SRGB8, 77 << 16 | 77 << 8 | 77))
    for d in range(256):
        want = np.stack([sweep["table"][a_s, d, s[..., c]] for c in range(3)] + [np.full((frames, h, w), 255, np.uint8)], -1)
        for f in range(frames):
            assert_equal(got[d][f], want[f], "sweep over the colour (%d, %d, %d), frame %d" % (d, d, d, f))


# ------------------------------------------------------------------ 3. product against product

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [(40, 24), (260, 6)], ids=["40x24", "260x6"])
def test_identity_size_equals_the_one_to_one_decode_under_option_9(rig, oracle, tabs, size, mode):
    """8-bit intermediate, identity size: bt709hip_decode_scaled under option 10 against bt709hip_decode under option 9 with the
    same background, byte for byte."""
    w, h = size
    planes = random_planes(w, h, seed=w * 13 + h)
    bg = random_backgrounds(w, h, seed=w * 17 + h)
    scaled, plain = Job(rig, planes, out_size=(w, h)), Job(rig, planes)
    try:
        scaled.fill(bg), plain.fill(bg)
        _capi.check(_scaled(scaled, _decoder(rig, _value(mode)), 0))
        assert rig.kernel() == sc.kernel_name(SRGB8, mode == "destination")
        _capi.check(plain.decode_one(_decoder(rig, None, over9=_value(mode))))
        assert rig.kernel().startswith(b"decode_nv12_quads<alpha,over")
        a, b = scaled.collect("scaled %dx%d %s" % (w, h, mode))[0], plain.collect("1:1 %dx%d %s" % (w, h, mode))[0]
    finally:
        scaled.free(), plain.free()
    assert_equal(a, b, "option 10 at identity size against option 9, %dx%d %s" % (w, h, mode))
    assert_equal(a, sc.want_over(oracle, tabs, planes[0], w, h, SRGB8, _background(mode, bg[0])), "%dx%d %s" % (w, h, mode))


# ------------------------------------------------------------------ 4. decode_half under the option

@pytest.mark.parametrize("intermediate", FORMATS, ids=IDS)
@pytest.mark.parametrize("size", [(64, 36), (520, 292)], ids=["64x36", "520x292"])
def test_decode_half_equals_decode_scaled_at_exactly_half(rig, oracle, tabs, size, intermediate):
    """Both run the any-ratio kernel's over form (by name: there is no 2:1 over kernel), give equal bytes, and the definition's."""
    w, h = size
    ow, oh = w // 2, h // 2
    planes = random_planes(w, h, seed=w * 19 + h)
    bg = random_backgrounds(ow, oh, seed=w * 23 + h)
    for mode in MODES:
        dec = _decoder(rig, _value(mode), intermediate)
        got = {}
        for entry in ("bt709hip_decode_half", "bt709hip_decode_scaled"):
            job = Job(rig, planes, out_size=(ow, oh))
            try:
                job.fill(bg)
                _capi.check(_scaled(job, dec, 0, entry=entry))
                assert rig.kernel() == sc.kernel_name(intermediate, mode == "destination"), (entry, rig.kernel())
                got[entry] = job.collect("%s %dx%d %s" % (entry, w, h, mode))[0]
            finally:
                job.free()
        assert_equal(got["bt709hip_decode_half"], got["bt709hip_decode_scaled"], "half against scaled, %dx%d %s" % (w, h, mode))
        assert_equal(got["bt709hip_decode_half"], sc.want_over(oracle, tabs, planes[0], ow, oh, intermediate, _background(mode, bg[0])),
                     "half %dx%d %s" % (w, h, mode))


# ------------------------------------------------------------------ 5. destination over a fill == colour mode

@pytest.mark.parametrize("intermediate", FORMATS, ids=IDS)
@pytest.mark.parametrize("size,out_size", [((520, 292), (346, 194)), ((96, 54), (300, 170))], ids=["down", "up"])
def test_destination_over_a_uniform_fill_equals_colour_mode(rig, oracle, tabs, size, out_size, intermediate):
    (w, h), (ow, oh) = size, out_size
    planes = random_planes(w, h, seed=w + 3)
    job = Job(rig, planes, out_size=out_size)
    try:
        for colour in (0x10C0F8, 0xFFFFFF):
            job.fill([np.broadcast_to(oc.colour_word(colour), (oh, ow, 4))])
            _capi.check(_scaled(job, _decoder(rig, DEST, intermediate), 0))
            over_fill = job.collect()[0]
            job.fill(random_backgrounds(ow, oh, seed=colour & 0xFF))  # colour mode does not read the target
            _capi.check(_scaled(job, _decoder(rig, colour, intermediate), 0))
            over_colour = job.collect()[0]
            assert_equal(over_fill, over_colour, "fill %06x" % colour)
            assert_equal(over_colour, sc.want_over(oracle, tabs, planes[0], ow, oh, intermediate, colour), "colour %06x" % colour)
    finally:
        job.free()


# ------------------------------------------------------------------ 6. switching

def test_switching_the_option_and_the_two_options_side_by_side(rig, oracle, tabs):
    """Option 10 back to off: the plain bytes under the plain kernel name.  Options 9 and 10 at different colours: a rescale
    shows option 10's, a 1:1 decode option 9's."""
    (w, h), (ow, oh) = (64, 36), (48, 20)
    nine, ten = 0xE0A010, 0x204060
    planes = random_planes(w, h, seed=31)
    scaled, plain = Job(rig, planes, out_size=(ow, oh)), Job(rig, planes)
    try:
        dec = _decoder(rig, DEST)
        bg = random_backgrounds(ow, oh, seed=32)
        scaled.fill(bg)
        _capi.check(_scaled(scaled, dec, 0))
        assert rig.kernel() == sc.kernel_name(SRGB8, True)
        assert_equal(scaled.collect()[0], sc.want_over(oracle, tabs, planes[0], ow, oh, SRGB8, bg[0]), "option on")
        _capi.check(rig.lib.bt709hip_decoder_set_option(dec, OPT, _capi.OVER_OFF))
        scaled.fill(bg)
        _capi.check(_scaled(scaled, dec, 0))
        assert rig.kernel() == sc.plain_name(SRGB8)
        assert_equal(scaled.collect()[0], sc.option_off_view(oracle, planes[0], ow, oh, SRGB8), "option off again")
        # both options on, at different colours
        rig.set_over(dec, nine)
        _capi.check(rig.lib.bt709hip_decoder_set_option(dec, OPT, ten))
        _capi.check(_scaled(scaled, dec, 0))
        assert rig.kernel() == sc.kernel_name(SRGB8, False)
        assert_equal(scaled.collect()[0], sc.want_over(oracle, tabs, planes[0], ow, oh, SRGB8, ten), "the rescale shows option 10's colour")
        _capi.check(plain.decode_one(dec))
        assert rig.kernel() == b"decode_nv12_quads<alpha,over-colour>"
        assert_equal(plain.collect()[0], oc.composite_over(oc.expected_source(oracle, *planes[0]), nine, *tabs), "the 1:1 decode shows option 9's colour")
        assert not np.array_equal(sc.want_over(oracle, tabs, planes[0], ow, oh, SRGB8, ten), sc.want_over(oracle, tabs, planes[0], ow, oh, SRGB8, nine))
    finally:
        scaled.free(), plain.free()


# ------------------------------------------------------------------ 7. graphs

def test_graph_replays_over_a_refilled_canvas_and_refuses_a_missing_table(rig, oracle, tabs):
    """One stream, one kernel node: a destination-mode bt709hip_decode_scaled captured after bt709hip_decoder_setup, replayed
    twice over a refilled canvas.  A decoder without the table refuses inside a capture and launches nothing."""
    (w, h), (ow, oh) = (64, 36), (100, 28)
    planes = random_planes(w, h, seed=41)
    job = Job(rig, planes, out_size=(ow, oh))
    cb = rig.ctx.commandQueue.commandBuffer(new_stream=True)
    rec = None
    try:
        dec = _decoder(rig, DEST)  # the option first, then bt709hip_decoder_setup: the table is there before the capture
        cb.beginRecording()
        _capi.check(_scaled(job, dec, 0, stream=cb.stream, wait=0))
        rec = cb.endRecording()
        assert job.untouched()  # recorded, not run
        for seed in (1, 2):
            bg = random_backgrounds(ow, oh, seed=seed)
            job.fill(bg)
            rec.replay(cb)
            cb.waitUntilCompleted()
            assert_equal(job.collect("replay %d" % seed)[0], sc.want_over(oracle, tabs, planes[0], ow, oh, SRGB8, bg[0]), "replay %d" % seed)
        # a decoder that is set up but met the option afterwards: its first blended rescale may not build the table in a capture
        job.fill(None)
        late = _decoder(rig, None)
        _capi.check(rig.lib.bt709hip_decoder_set_option(late, OPT, DEST))
        cb.beginRecording()
        assert _scaled(job, late, 0, stream=cb.stream, wait=0) == _capi.ERR_NOT_SETUP
        cb.endRecording().release()
        assert job.untouched()
        # bt709hip_decoder_setup builds it for a decoder that is set up already
        _capi.check(rig.lib.bt709hip_decoder_setup(late))
        bg = random_backgrounds(ow, oh, seed=3)
        job.fill(bg)
        _capi.check(_scaled(job, late, 0, stream=cb.stream, wait=1))
        assert_equal(job.collect()[0], sc.want_over(oracle, tabs, planes[0], ow, oh, SRGB8, bg[0]), "after the capture")
    finally:
        if rec is not None:
            rec.release()
        cb.release()
        job.free()
