"""GPU tests (-m gpu) of straight alpha in and out: BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY -- bt709hip_encode[_batch]
multiplying each texel's B, G, R by its A inside the encode kernel -- and BT709HIP_OPT_UNPREMULTIPLY -- an alpha decoder's 1:1
decode dividing them out again inside the decode kernel.  Everything goes through the C ABI.  Expected bytes come from the CPU
oracle plus the numpy statement of 3.9 in tests/straight_alpha_cases.py, never from the code under test; every output slab is
canary-filled and compared whole (encoder) or outside its pixels (decoder), and every case asserts the kernel it was built to
reach.  On a tree without the feature each test fails at its first set_option (BT709HIP_ERR_INVALID_ARG)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import encoder_cases as ec
import metalbt709decoder_amd as mb
import over_cases as oc
import straight_alpha_cases as sc
import variant_cases as vc
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_LINEAR, GAMMA_SRGB

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NV12, I420 = 0, 1
CTX_OPT, DEC_OPT = sc.CTX_OPT_ENCODE_PREMULTIPLY, sc.OPT_UNPREMULTIPLY
GUARD = ec.GUARD
ENCODE_NAME = {(NV12, True): "encode_bgra_nv12", (NV12, False): "encode_bgra_nv12_blocks", (I420, True): "encode_bgra_i420", (I420, False): "encode_bgra_i420_blocks"}
DECODE_NAME = {(NV12, "quads"): b"decode_nv12_quads<alpha", (NV12, "blocks"): b"decode_nv12_blocks<alpha",
               (I420, "quads"): b"decode_i420_quads<alpha", (I420, "blocks"): b"decode_i420_blocks<alpha"}


@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


# ================================================================== the encoder

def _planar():
    import test_encode_planar_gpu as planar  # its harness sets the context's layout for the call and restores it
    return planar


@pytest.fixture(scope="module")
def harness(gh):
    planar = _planar()

    class Harness(planar.Harness):
        """The planar tests' harness with the context's premultiply option set for the call (and back at 0 after it, whatever
        happens: the context is the process's)."""

        def encode(self, layout, in_slab, pair, premultiply, option=NV12):
            rc = self.lib.bt709hip_context_set_option(self.h, CTX_OPT, 1 if premultiply else 0)
            assert rc == _capi.OK, "bt709hip_context_set_option(%d, %d): %s" % (CTX_OPT, premultiply, _capi.strerror(rc))
            try:
                return super().encode(layout, in_slab, pair, option=option)
            finally:
                assert self.lib.bt709hip_context_set_option(self.h, CTX_OPT, 0) == _capi.OK

    return Harness(gh)


def _record(res):
    return res.grid, res.block, res.launches, res.xcd_bands


def _expected(layout, option, planes):
    """planes(i) -> (y, cbcr) of slot i -> the two output slabs as they must read back under `option`."""
    if option == I420:
        return _planar().expected_slabs(layout, lambda i: (planes(i)[0], planes(i)[1][:, 0::2], planes(i)[1][:, 1::2]))
    return ec.expected_slabs(layout, planes)


def _compare(layout, option, res, want, label):
    want_y, want_c = want
    diffs = [ec.describe_difference(layout, res.y_slab, want_y, "y")]
    if option == I420:
        diffs.append(_planar().describe_chroma(layout, res.c_slab, want_c))
    else:
        diffs.append(ec.describe_difference(layout, res.c_slab, want_c, "cbcr"))
    diffs = [d for d in diffs if d]
    assert not diffs, label + ": " + "\n".join(diffs)


def run_encoder_case(harness, oracle, layout, option, pair, pictures, fast, label):
    """pictures: the straight-alpha words of each slot.  Encodes them with the option on; encodes their numpy-premultiplied twins
    with it off; both must read back -- canary bytes included -- as the oracle's planes of the premultiplied pictures, under the
    names of the premultiplying and of the plain kernel, with one and the same launch on record."""
    L, n = layout, layout.n
    w, h = L.w, L.h
    pre = [sc.premultiply(p) for p in pictures]
    y, c = ec.threaded_encode(oracle, np.concatenate(pre), w, h * n, *pair)  # whole row pairs of every slot: blocks do not mix
    want = _expected(L, option, lambda i: (y[i * h:(i + 1) * h], c[i * h // 2:(i + 1) * h // 2]))
    on = harness.encode(L, ec.fill_input(L, lambda i: pictures[i]), pair, True, option)
    assert on.kernel == ENCODE_NAME[option, fast] + "<premul>", on.kernel
    _compare(L, option, on, want, label + ", option on")
    off = harness.encode(L, ec.fill_input(L, lambda i: pre[i]), pair, False, option)
    assert off.kernel == ENCODE_NAME[option, fast], off.kernel
    _compare(L, option, off, want, label + ", plain encode of the premultiplied picture")
    assert np.array_equal(on.y_slab, off.y_slab) and np.array_equal(on.c_slab, off.c_slab)
    assert _record(on) == _record(off), "the launch plan is not the plain encoder's"
    return on


@pytest.mark.parametrize("pair", ec.PAIRS, ids=["%d-%d" % p for p in ec.PAIRS])
def test_encoder_every_pair(harness, oracle, pair):
    """Every (colour byte, A) pair in every channel, in each pixel position of a quad and in both rows of a block, under each
    gamma pair."""
    w, h = sc.PAIRS_W, sc.PAIRS_H
    L = ec.Layout(w, h, (4 * w, w, w), [GUARD], [GUARD], [GUARD])
    res = run_encoder_case(harness, oracle, L, NV12, pair, [sc.every_pair_picture()], True, "every pair, %s" % (pair,))
    plan = ec.expected_plan(w, h, 1)
    assert _record(res) == (tuple(plan["grid"]), (plan["block"], 1, 1), 1, 0)


def _single(w, h, option, strides=None, misalign=(0, 0, 0)):
    if option == I420:
        return _planar().single(w, h, strides, misalign)
    return ec.Layout(w, h, strides or (4 * w, w, w), *[[GUARD + m] for m in misalign])


def _batch(w, h, n, option, spacing):
    case = ec.Case("%dx%dx%d" % (w, h, n), w, h, n, None, None, spacing=spacing, strides=(4 * w, w, w // 2 if option == I420 else w))
    return _planar().case_layout(case) if option == I420 else ec.case_layout(case)


# name -> (layout builder, option, fast, what the launch on record must be: (tiles, lanes, launches, banded) or None)
ENCODER_SHAPES = {
    "single-1536x8": (lambda: _single(1536, 8, NV12), NV12, True, (1, 384, 1, 0)),             # one picture per launch: a 384-lane tile
    "even-1536x8x3": (lambda: _batch(1536, 8, 3, NV12, "even"), NV12, True, (2, 192, 1, 0)),   # a batch: two 192-lane tiles
    "general-1022x6": (lambda: _single(1022, 6, NV12), NV12, False, None),                      # width = 2 mod 4
    "general-1024x6-pitch+4": (lambda: _single(1024, 6, NV12, (4 * 1024 + 4, 1024, 1024), (4, 0, 0)), NV12, False, None),  # an odd number of words a row, a 4-byte base
    "i420-1536x8": (lambda: _single(1536, 8, I420), I420, True, (1, 384, 1, 0)),
    "i420-general-1022x6": (lambda: _single(1022, 6, I420), I420, False, None),
    "table-260x6x3": (lambda: _batch(260, 6, 3, NV12, "table"), NV12, True, (1, 128, 1, 0)),   # the pointer table
    "even-1284x20x64": (lambda: _batch(1284, 20, 64, NV12, "even"), NV12, True, (2, 192, 1, 1)),  # the XCD-band plan
    "even-1284x20x71": (lambda: _batch(1284, 20, 71, NV12, "even"), NV12, True, (2, 192, 2, 1)),  # its head of 64 and a plain tail of 7
}


@pytest.mark.parametrize("name", ENCODER_SHAPES)
def test_encoder_shapes(harness, oracle, name):
    build, option, fast, shape = ENCODER_SHAPES[name]
    L = build()
    k = list(ENCODER_SHAPES).index(name)
    pair = ec.PAIRS[k % len(ec.PAIRS)]
    pictures = [sc.crop(L.w, L.h, row0=(2 * k + 14 * i) % sc.PAIRS_H) for i in range(L.n)]  # every slot its own rows, its own A's
    if name.startswith("table"):
        assert not ec.layout_is_uniform(L)
    res = run_encoder_case(harness, oracle, L, option, pair, pictures, fast, name)
    if shape is not None:
        tiles, lanes, launches, banded = shape
        assert (res.grid[0] // (8 if banded else 1), res.block[0], res.launches, res.xcd_bands) == shape, (res.grid, res.block, res.launches, res.xcd_bands)
    else:
        assert res.block[0] == ec.GENERAL_THREADS and res.launches == 1 and res.xcd_bands == 0


def test_encoder_alpha_frames_are_unaffected(harness):
    """BGRA8_ALPHA input reads A alone: with the option on, the same kernel under the same name writes the same bytes."""
    planar = _planar()
    w, h = 64, 8
    L = planar.single(w, h, (4 * w + 16, 68, 38))
    words = np.random.default_rng(64).integers(0, 1 << 32, (h, w), dtype=np.uint32)
    in_slab = ec.fill_input(L, lambda i: words)
    luma = np.array(json.load(open(os.path.join(HERE, "golden", "alpha_luma.json")))["luma"], np.uint8)
    got = []
    for on in (1, 0):
        assert harness.lib.bt709hip_context_set_option(harness.h, CTX_OPT, on) == _capi.OK
        try:
            got.append(planar.Harness.encode(harness, L, in_slab, (GAMMA_LINEAR, GAMMA_LINEAR), option=NV12, fmt=planar.ALPHA_FORMAT, with_cbcr=False))
        finally:
            assert harness.lib.bt709hip_context_set_option(harness.h, CTX_OPT, 0) == _capi.OK
        assert got[-1].kernel == "encode_alpha_y"
    assert np.array_equal(got[0].y_slab, got[1].y_slab) and (got[0].c_slab == ec.FILL).all() and (got[1].c_slab == ec.FILL).all()
    want_y = np.full(L.y_bytes, ec.FILL, np.uint8)
    ec._rows_view(want_y, L.y_off[0], h, L.sy, w)[:] = luma[(words >> 24).astype(np.uint8)]
    assert np.array_equal(got[0].y_slab, want_y) and _record(got[0]) == _record(got[1])


def test_encoder_option_off_after_on(harness, oracle):
    """A context that had the option on and off again encodes as one that never had it: the plain kernel, the oracle's planes of
    the picture as it stands."""
    w, h = 260, 6
    L = _single(w, h, NV12)
    words = sc.crop(w, h, row0=100)
    pair = ec.PAIRS[0]
    harness.encode(L, ec.fill_input(L, lambda i: words), pair, True)
    res = harness.encode(L, ec.fill_input(L, lambda i: words), pair, False)
    assert res.kernel == "encode_bgra_nv12"
    y, c = oracle.encode_nv12(words & 0xFFFFFF, w, h, *pair)
    _compare(L, NV12, res, ec.expected_slabs(L, lambda i: (y, c)), "off after on")


# ================================================================== the decoder

@pytest.fixture(scope="module")
def rig(gh):
    class Rig(vc.Rig):
        def straight(self, value=1, options=()):
            """An alpha decoder with BT709HIP_OPT_UNPREMULTIPLY at `value`."""
            d = self.decoder(options=options)
            rc = self.lib.bt709hip_decoder_set_option(d, DEC_OPT, value)
            assert rc == _capi.OK, "bt709hip_decoder_set_option(%d, %d): %s" % (DEC_OPT, value, _capi.strerror(rc))
            return d

    r = Rig(gh)
    yield r
    r.close()


@pytest.fixture(scope="module")
def every_pair(oracle):
    """The decoder's sweep frame and what it must decode to, computed once and left unchanged: columns are the covering triples
    (every byte value in each of R, G, B), each a 2-wide block; row r's alpha-plane byte is r.  -> planes, the premultiplied
    words the oracle decodes them to, and their numpy unpremultiply."""
    triples, words = oc.covering_triples(oracle)
    for c in range(3):
        assert np.unique(words[:, c]).size == 256  # the coverage the sweep claims
    y, uv, a = sc.decoder_planes(triples)
    assert y.shape[1] % 4 == 0
    source = oc.expected_source(oracle, y, uv, a)
    assert np.unique(source[..., 3]).size > 200  # the alpha codes reach (nearly) every alpha byte; what they reach is the oracle's business
    want = sc.unpremultiply(source)
    # the properties 3.9 names show in the expectation: A = 0 gives the word 0, A = 255 leaves the colour, colour > A saturates
    assert (want[source[..., 3] == 0] == 0).all()
    opaque = source[..., 3] == 255
    assert opaque.any() and np.array_equal(want[opaque], source[opaque])
    over = (source[..., :3] > source[..., 3:]) & (source[..., 3:] > 0)
    assert over.any() and (want[..., :3][over] == 255).all()
    for arr in (y, uv, a, source, want):
        arr.setflags(write=False)
    return dict(y=y, uv=uv, a=a, source=source, want=want)


def _frames(every_pair, mode):
    """The sweep frame cut for `mode` -> [(row0, rows)]: one frame of 256 rows, four of 64, or sixty-four of 4: every way, all 256 alpha codes."""
    n = {"single": 1, "table": 4, "even64": 64}[mode]
    return [(i * (256 // n), 256 // n) for i in range(n)]


def _job(rig, every_pair, layout, path, mode):
    y, uv, a = every_pair["y"], every_pair["uv"], every_pair["a"]
    cuts = _frames(every_pair, mode)
    spacing = "table" if mode == "table" else "even"
    pads, out_offset = ((4, 8, 12, 16), 0) if path == "quads" else ((1, 3, 2, 4), 4)  # general: odd plane pitches, a 4-byte-aligned output
    if layout == I420:
        from test_planar_gpu import PlanarJob
        planes = [(y[r:r + n], uv[r // 2:(r + n) // 2, 0::2], uv[r // 2:(r + n) // 2, 1::2], a[r:r + n]) for r, n in cuts]
        if path == "blocks":
            pads = (1, 3, 2, 4)
        job = PlanarJob(rig, planes, pads=pads, out_offset=out_offset, spacing=spacing)
    else:
        planes = [(y[r:r + n], uv[r // 2:(r + n) // 2], a[r:r + n]) for r, n in cuts]
        job = vc.Job(rig, planes, pads=pads, out_offset=out_offset, spacing=spacing)
    return job, cuts


@pytest.mark.parametrize("mode", ["single", "table", "even64"])
@pytest.mark.parametrize("path", ["quads", "blocks"])
@pytest.mark.parametrize("layout", [NV12, I420], ids=["nv12", "i420"])
def test_decoder_every_pair(rig, every_pair, layout, path, mode):
    """Every alpha code against every colour byte of each channel, on the fast and the general kernel of either chroma layout, as
    one frame, through the pointer table and as an evenly spaced batch of 64 (the XCD-band map on the fast path)."""
    job, cuts = _job(rig, every_pair, layout, path, mode)
    try:
        dec = rig.straight()
        if layout == I420:
            _capi.check(rig.lib.bt709hip_decoder_set_option(dec, _capi.OPT_CHROMA_LAYOUT, I420))
        _capi.check(job.decode_one(dec) if mode == "single" else job.decode_batch(dec))
        assert rig.kernel() == DECODE_NAME[layout, path] + b",straight>", rig.kernel()
        grid, block, launches, bands = rig.launch()
        assert launches == 1 and (bands != 0) == (mode == "even64" and path == "quads")
        if mode != "single":
            assert (grid[2] * (8 if bands else 1) if path == "quads" else grid[1]) == len(cuts)
        got = job.collect("%s %s %s" % (layout, path, mode))  # asserts the canaries around every target
    finally:
        job.free()
    for (r, n), g in zip(cuts, got):
        vc.assert_equal(g, every_pair["want"][r:r + n], "rows %d..%d" % (r, r + n))


def test_decoder_option_off_after_on(rig, every_pair):
    """A decoder that had the option on and off again is the plain alpha decoder: its kernel, its (premultiplied) words."""
    job, cuts = _job(rig, every_pair, NV12, "quads", "table")
    try:
        dec = rig.straight()
        _capi.check(job.decode_batch(dec))
        assert rig.kernel() == b"decode_nv12_quads<alpha,straight>"
        _capi.check(rig.lib.bt709hip_decoder_set_option(dec, DEC_OPT, 0))
        assert rig.option(dec, DEC_OPT) == 0
        job.fill(None)
        _capi.check(job.decode_batch(dec))
        assert rig.kernel() == b"decode_nv12_quads<alpha>"
        got = job.collect("off after on")
        never = rig.decoder()
        job.fill(None)
        _capi.check(job.decode_batch(never))
        assert rig.kernel() == b"decode_nv12_quads<alpha>"
        plain = job.collect("never on")
    finally:
        job.free()
    for (r, n), g, p in zip(cuts, got, plain):
        vc.assert_equal(g, every_pair["source"][r:r + n], "off after on, rows %d.." % r)
        vc.assert_equal(g, p, "against a decoder that never had it, rows %d.." % r)


def test_decoder_through_a_ring_and_a_coalesced_pair(rig, gh, every_pair):
    """Everything that launches through bt709hip_decode_batch carries the option: a ring's decode and two queued single-frame
    decodes equal the direct call on the same planes."""
    ctx = gh.context()
    y, uv, a, want = every_pair["y"], every_pair["uv"], every_pair["a"], every_pair["want"]
    w, h, rows = y.shape[1], 8, (0, 248)  # two frames: the alpha codes 0..7 and 248..255
    planes = [(y[r:r + h], uv[r // 2:(r + h) // 2], a[r:r + h]) for r in rows]
    job = vc.Job(rig, planes)
    cb = ctx.commandQueue.commandBuffer(new_stream=True)
    ring = None
    try:
        _capi.check(job.decode_batch(rig.straight()))
        direct = job.collect("direct")
        for r, g in zip(rows, direct):
            vc.assert_equal(g, want[r:r + h], "direct, rows %d.." % r)
        # the coalesced pair
        job.fill(None)
        dec = rig.straight(options=[(_capi.OPT_COALESCE, 2)])
        _capi.check(job.decode_one(dec, 0, stream=cb.stream, wait=0))
        assert rig.kernel() == b"(queued: coalescing submit)" and job.untouched()
        _capi.check(job.decode_one(dec, 1, stream=cb.stream, wait=0))
        assert rig.kernel() == b"decode_nv12_quads<alpha,straight>"
        assert rig.launch()[0][2] == 2  # one launch over the two frames
        _capi.check(rig.lib.bt709hip_decoder_flush(dec, cb.stream))
        rig.sync(cb.stream)
        for i, g in enumerate(job.collect("coalesced")):
            vc.assert_equal(g, direct[i], "coalesced %d" % i)
        # the ring, through the Python mirror's property
        d = gh.make_decoder(mb.MetalBT709GammaSRGB, has_alpha=True)
        d.straightAlpha = True
        assert d.lastStatus == _capi.OK and d.straightAlpha is True
        ring = mb.FrameRing(d, (w, h), 2, tries=1)
        for i, (py, puv, pa) in enumerate(planes):
            ring.pixelBuffer(i).upload_planes(py, puv)
            ab = ring.alphaPixelBuffer(i)
            ctx._upload(ab.y_ptr, ab.y_stride, pa, None)
        ctx._sync(None)
        assert ring.decode(0, 2, waitUntilCompleted=True), d.lastStatus
        assert ctx.lib.bt709hip_last_kernel_name() == b"decode_nv12_quads<alpha,straight>"
        for i in range(2):
            got = ctx.getBGRATexturePixels(ring.texture(i)).view(np.uint8).reshape(h, w, 4)
            vc.assert_equal(got, direct[i], "ring frame %d" % i)
        # the mirror carries the refusals: a rescale while the option is on
        small = ctx.makeBGRATexture((w // 2, h // 2))
        buf, abuf = gh.make_buffer(planes[0][0], planes[0][1], d.gamma), gh.make_alpha_buffer(planes[0][2])
        assert not d.decodeBT709Scaled(buf, small, ctx.commandQueue.commandBuffer(), True, alphaPixelBuffer=abuf)
        assert d.lastStatus == _capi.ERR_UNSUPPORTED
    finally:
        if ring is not None:
            ring.release()
        cb.release()
        job.free()


# ================================================================== both together

def test_round_trip_at_the_interface(gh, oracle):
    """A straight-alpha picture in bands of A = 0, 1, 128, 254, 255: the premultiplying encode and the alpha-frame encode, then
    the alpha decode with the option on, equal the numpy composition of the same three steps.  No identity with the input is
    claimed (3.9): at A = 1 every colour comes back 0 or 255."""
    conv, ctx = mb.BGRAToBT709Converter, gh.context()
    w, h = 64, 32
    words = sc.bands_picture(w, h)
    assert sorted(np.unique(words >> 24).tolist()) == [0, 1, 128, 254, 255]
    tex = ctx.makeBGRATexture((w, h), pixels=words)
    colour, alpha = conv.createCoreVideoYCbCrBuffer(ctx, (w, h)), conv.createCoreVideoYCbCrBuffer(ctx, (w, h))
    assert ctx.setEncodePremultiply(True)
    try:
        assert conv.convertIntoCoreVideoBuffer(tex, colour, mb.MetalBT709GammaSRGB, mb.MetalBT709GammaSRGB)
        assert ctx.lib.bt709hip_last_kernel_name() == b"encode_bgra_nv12<premul>"
        assert conv.convertAlphaIntoCoreVideoBuffer(tex, alpha)
        assert ctx.lib.bt709hip_last_kernel_name() == b"encode_alpha_y"
    finally:
        assert ctx.setEncodePremultiply(False)
    colour.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
    colour.setAttachment("TransferFunction", mb.kCVImageBufferTransferFunction_sRGB)
    d = gh.make_decoder(mb.MetalBT709GammaSRGB, has_alpha=True)
    assert d.setStraightAlpha(True)
    out = ctx.makeBGRATexture((w, h))
    assert d.decodeBT709(colour, alpha, out, ctx.commandQueue.commandBuffer(), None, w, h, True), d.lastStatus
    assert ctx.lib.bt709hip_last_kernel_name() == b"decode_nv12_quads<alpha,straight>"
    got = ctx.getBGRATexturePixels(out).view(np.uint8).reshape(h, w, 4)
    # the same three steps in numpy + the oracle
    y, c = oracle.encode_nv12(sc.premultiply(words) & 0xFFFFFF, w, h, GAMMA_SRGB, GAMMA_SRGB)
    luma = np.array(json.load(open(os.path.join(HERE, "golden", "alpha_luma.json")))["luma"], np.uint8)
    ay = luma[(words >> 24).astype(np.uint8)]
    gy, gc = colour.download_planes()
    assert np.array_equal(gy, y) and np.array_equal(gc, c) and np.array_equal(alpha.download_planes()[0], ay)
    want = sc.unpremultiply(oc.expected_source(oracle, y, c, ay))
    vc.assert_equal(got, want, "round trip")
    assert (got[(words >> 24) == 0] == 0).all()
