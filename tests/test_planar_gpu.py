"""GPU tests (-m gpu) of BT709HIP_OPT_CHROMA_LAYOUT = BT709HIP_CHROMA_I420: planar Y, U, V frames decoded in place.
The arithmetic is the NV12 kernels'; what these tests pin is the front end -- which chroma bytes reach which pixel, at which
sizes, pitches and alignments, in which kernel.  Expected bytes: the oracle's decode_nv12 of the interleaved twin of the planes;
wherever the NV12 path can run the same picture, equality with it too.  Everything but the Y4M / Python-mirror tests goes through
the C ABI, planes inside canary slabs, every byte outside the W x H output words checked."""
import ctypes as C

import numpy as np
import pytest

import metalbt709decoder_amd as mb
import over_cases as oc
import variant_cases as vc
from metalbt709decoder_amd import _capi
from metalbt709decoder_amd._capi import Frame, Surface

pytestmark = pytest.mark.gpu

OPT, NV12, I420 = _capi.OPT_CHROMA_LAYOUT, _capi.CHROMA_NV12, _capi.CHROMA_I420
APPLE, SRGB, LINEAR, ITU709 = mb.MetalBT709GammaApple, mb.MetalBT709GammaSRGB, mb.MetalBT709GammaLinear, mb.MetalBT709GammaITU709
GAMMAS = (APPLE, SRGB, LINEAR, ITU709)
# (path, gamma) -> kernel name with BT709HIP_OPT_NONTEMPORAL at 1 / at 0
QUADS = {APPLE: (b"decode_i420_quads<nt>", b"decode_i420_quads"), ITU709: (b"decode_i420_quads<nt>", b"decode_i420_quads"),
         SRGB: (b"decode_i420_quads<nt,quantiser>", b"decode_i420_quads<quantiser>"), LINEAR: (b"decode_i420_quads_log<nt>", b"decode_i420_quads_log")}
BLOCKS = {APPLE: b"decode_i420_blocks", ITU709: b"decode_i420_blocks", LINEAR: b"decode_i420_blocks", SRGB: b"decode_i420_blocks<quantiser>"}


def interleave(u, v):
    """The NV12 twin of two planar chroma planes."""
    c = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    c[:, 0::2], c[:, 1::2] = u, v
    return c


class PlanarJob(vc.Job):
    """variant_cases.Job over planar frames.  planes: [(y, u, v, alpha)]; per slot Y at pitch W + pads[0], then -- c_offset bytes
    past a 256-byte boundary -- U and, (H/2) pitches behind it, V at pitch W/2 + pads[1], then the alpha plane.  Every input byte
    that is no sample (row padding, the gap behind V's last row, guard bands) holds pad_fill."""

    def __init__(self, rig, planes, pads=(0, 0, 0, 0), c_offset=0, out_offset=0, spacing="even", pad_fill=0x00, transfer=vc.SRGB):
        self.rig, self.n = rig, len(planes)
        self.h, self.w = planes[0][0].shape
        w, h = self.w, self.h
        self.ow, self.oh, self.px = w, h, 4
        self.sy, self.sc, self.sa, self.so = w + pads[0], w // 2 + pads[1], w + pads[2], 4 * w + pads[3]
        has_alpha = planes[0][3] is not None
        c_off = vc._up(self.sy * h, 256) + c_offset
        a_off = vc._up(c_off + self.sc * h, 256)
        in_pitch = a_off + (vc._up(self.sa * h, 256) if has_alpha else 0)
        out_pitch = vc._up(self.so * h, 256)
        gap = lambda i: vc.GUARD if spacing == "table" and i == self.n - 1 and self.n > 1 else 0
        self.in_off = [vc.GUARD + i * in_pitch + gap(i) for i in range(self.n)]
        self.out_off = [vc.GUARD + i * out_pitch + gap(i) + out_offset for i in range(self.n)]
        host = np.full(self.in_off[-1] + in_pitch + vc.GUARD, pad_fill, np.uint8)
        for i, (y, u, v, a) in enumerate(planes):
            for plane, off, stride, rows, cols in ((y, 0, self.sy, h, w), (u, c_off, self.sc, h // 2, w // 2),
                                                   (v, c_off + (h // 2) * self.sc, self.sc, h // 2, w // 2), (a, a_off, self.sa, h, w)):
                if plane is not None:
                    host[self.in_off[i] + off:self.in_off[i] + off + stride * rows].reshape(rows, stride)[:, :cols] = plane
        self.d_in = rig.DeviceBuffer(rig.ctx, host.size, placement_tries=1)
        rig.upload(self.d_in.ptr, host)
        self.out_bytes = self.out_off[-1] + out_pitch + vc.GUARD
        self.d_out = rig.DeviceBuffer(rig.ctx, self.out_bytes, placement_tries=1)
        self.frames = (Frame * self.n)(*[Frame(self.d_in.ptr + o, self.sy, self.d_in.ptr + o + c_off, self.sc, w, h, vc.MATRIX, transfer) for o in self.in_off])
        self.alphas = (Frame * self.n)(*[Frame(self.d_in.ptr + o + a_off, self.sa, None, self.sa, w, h, vc.MATRIX, vc.LINEAR)
                                         for o in self.in_off]) if has_alpha else None
        self.surfs = (Surface * self.n)(*[Surface(self.d_out.ptr + o, self.so, w, h, _capi.FORMAT_BGRA8_SRGB, 0) for o in self.out_off])
        self.fill(None)


def random_yuv(w, h, seed, n=1, alpha=False):
    """Random luma (and alpha); chroma planes from a random start in which every U and V sample differs from its left and upper
    neighbour, and U from V: a sample that reaches the wrong pixel changes the output."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ch, cw = h // 2, w // 2
        step = np.arange(cw)[None, :] * 37 + np.arange(ch)[:, None] * 101  # odd multipliers: neighbours differ mod 256
        u = ((int(rng.integers(0, 256)) + step) & 255).astype(np.uint8)
        v = ((u.astype(np.int64) + 1 + rng.integers(0, 254)) & 255).astype(np.uint8)
        assert cw < 2 or (u[:, 1:] != u[:, :-1]).all() and (v[:, 1:] != v[:, :-1]).all()
        assert ch < 2 or (u[1:] != u[:-1]).all() and (v[1:] != v[:-1]).all()
        assert (u != v).all()
        out.append((rng.integers(0, 256, (h, w), dtype=np.uint8), u, v, rng.integers(0, 256, (h, w), dtype=np.uint8) if alpha else None))
    return out


def want_of(oracle, gamma, planes):
    y, u, v, a = planes
    return oracle.decode_nv12(gamma, np.ascontiguousarray(y), interleave(u, v), alpha=a).reshape(y.shape[0], y.shape[1], 4)


@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


@pytest.fixture(scope="module")
def rig(gh):
    r = vc.Rig(gh)
    yield r
    r.close()


@pytest.fixture(scope="module")
def tabs(oracle):
    return oc.tables(oracle)


@pytest.fixture(scope="module")
def tile_quads(rig, gh):
    """Quads of a full tile of the fast kernels, from the launch on record: an 8192-wide frame takes grid.x tiles of
    block.x lanes, each lane the same number of quads."""
    job = PlanarJob(rig, random_yuv(8192, 2, 1), transfer=gh.TRANSFER_FOR_GAMMA[APPLE])
    try:
        _capi.check(job.decode_one(rig.decoder(gamma=APPLE, has_alpha=False, options=[(OPT, I420)])))
        grid, block, launches, bands = rig.launch()
    finally:
        job.free()
    assert launches == 1 and grid[0] >= 2 and (8192 // 4) % (grid[0] * block[0]) == 0
    return (8192 // 4) // grid[0]


# ------------------------------------------------------------------ 1. pairing, and padding that is never used

# name -> (w or a function of the tile's quads, h, pads of (Y, chroma, alpha, output) rows, bytes added to the U pointer, path)
FAST = {
    "4x2": (4, 2, (4, 6, 0, 16), 0), "8x2": (8, 2, (4, 6, 0, 16), 0), "12x2": (12, 2, (4, 6, 0, 16), 0), "20x6": (20, 6, (4, 6, 0, 16), 0),
    "20x6-tight": (20, 6, (0, 0, 0, 0), 0),       # the Y4M shape: pitch W/2 = 10, V ten bytes behind U's last row
    "20x6-u+2": (20, 6, (4, 2, 0, 16), 2),        # planes that are 2-byte but not 4-byte aligned stay on the fast path
    "tile+1": (lambda t: 4 * (t + 1), 2, (4, 6, 0, 16), 0),
    "2tiles-1": (lambda t: 4 * (2 * t - 1), 6, (4, 6, 0, 16), 0),
}
GENERAL = {
    "2x2": (2, 2, (0, 0, 0, 0), 0), "6x2": (6, 2, (2, 1, 0, 8), 0), "1918x4": (1918, 4, (2, 6, 0, 8), 0),
    "u-odd": (8, 4, (0, 0, 0, 0), 1),             # a U pointer at an odd address
    "pitch-odd": (8, 4, (0, 1, 0, 0), 0),         # cbcr_stride = 5: every other row of either plane at an odd address
    "pitch+6": (6, 2, (0, 6, 0, 0), 0),           # W/2 + 6
}
SIZES = [("quads", k) for k in FAST] + [("blocks", k) for k in GENERAL]


@pytest.fixture(scope="module")
def decoders(rig):
    """(gamma, BT709HIP_OPT_NONTEMPORAL) -> an opaque decoder with the layout option on."""
    return {(g, nt): rig.decoder(gamma=g, has_alpha=False, options=[(OPT, I420), (_capi.OPT_NONTEMPORAL, nt)]) for g in GAMMAS for nt in (1, 0)}


@pytest.mark.parametrize("path,case", SIZES, ids=[k for _, k in SIZES])
def test_pairing_and_padding(rig, gh, oracle, tile_quads, decoders, path, case):
    """Every gamma, streaming and temporal kernels, the planes' padding filled with 0x00 and then with 0xFF: the oracle's bytes
    both times, the expected kernel, the expected tile count, nothing written outside the pixels."""
    w, h, pads, c_offset = (FAST if path == "quads" else GENERAL)[case]
    w = w(tile_quads) if callable(w) else w
    planes = random_yuv(w, h, seed=w * 131 + h)
    first = {}
    for pad_fill in (0x00, 0xFF):
        job = PlanarJob(rig, planes, pads=pads, c_offset=c_offset, pad_fill=pad_fill)
        try:
            for (g, nt), dec in decoders.items():
                label = "%s, gamma %d, nt %d, padding %#04x" % (case, g, nt, pad_fill)
                job.frames[0].transfer = gh.TRANSFER_FOR_GAMMA[g]
                job.fill(None)
                _capi.check(job.decode_one(dec), label)
                name, (grid, block, launches, bands) = rig.kernel(), rig.launch()
                assert name == (QUADS[g][1 - nt] if path == "quads" else BLOCKS[g]), (label, name)
                if path == "quads":
                    assert launches == 1 and grid[0] == (w // 4 + tile_quads - 1) // tile_quads, (label, grid, block)
                got = job.collect(label)[0]
                vc.assert_equal(got, want_of(oracle, g, planes[0]), label)
                assert np.array_equal(first.setdefault((g, nt), got), got), label  # the padding's bytes reach no pixel
        finally:
            job.free()


# ------------------------------------------------------------------ 2. every colour, once per instantiation

LAYOUTS = {"aligned": ((0, 0, 0, 0), False), "odd": ((1, 3, 0, 0), False), "aligned-alpha": ((0, 0, 0, 0), True), "odd-alpha": ((1, 3, 5, 0), True)}
EVERY_COLOUR = [("aligned", APPLE, b"decode_i420_quads<nt>"), ("aligned", SRGB, b"decode_i420_quads<nt,quantiser>"),
                ("aligned", LINEAR, b"decode_i420_quads_log<nt>"), ("aligned-alpha", SRGB, b"decode_i420_quads<alpha>"),
                ("odd", APPLE, b"decode_i420_blocks"), ("odd", SRGB, b"decode_i420_blocks<quantiser>"), ("odd-alpha", SRGB, b"decode_i420_blocks<alpha>")]


@pytest.fixture(scope="module")
def colours():
    return vc.Colours()


@pytest.fixture(scope="module")
def colour_frames(rig, colours):
    """The every-colour frame, de-interleaved on the host, in device memory: uploaded once per layout."""
    jobs = {}

    def job(layout):
        if layout not in jobs:
            pads, alpha = LAYOUTS[layout]
            planes = (colours.y, colours.c[:, 0::2], colours.c[:, 1::2], vc.alpha_ramp(*colours.y.shape) if alpha else None)
            jobs[layout] = PlanarJob(rig, [planes], pads=pads)
        return jobs[layout]
    yield job
    for j in jobs.values():
        j.free()


@pytest.mark.parametrize("layout,gamma,kernel", EVERY_COLOUR, ids=[k.decode() for _, _, k in EVERY_COLOUR])
def test_every_colour_through_every_instantiation(rig, gh, oracle, colours, colour_frames, layout, gamma, kernel):
    job = colour_frames(layout)
    alpha = LAYOUTS[layout][1]
    job.frames[0].transfer = gh.TRANSFER_FOR_GAMMA[gamma]
    job.fill(None)
    dec = rig.decoder(gamma=gamma, has_alpha=alpha, options=[(OPT, I420)])
    _capi.check(job.decode_one(dec), kernel.decode())
    assert rig.kernel() == kernel, rig.kernel()
    got = job.collect(kernel.decode())[0]
    want = colours.image(oracle, gamma)
    if alpha:
        want = want.copy()
        want[..., 3] = np.array([oracle.decode_alpha(v) for v in range(256)], np.uint8)[vc.alpha_ramp(*colours.y.shape)]
    colours.assert_image(got, want, kernel.decode())


# ------------------------------------------------------------------ 3. batches

def test_batch_through_the_pointer_table(rig, gh, oracle):
    """Three frames, a gap before the last: no single step reaches them all."""
    planes = random_yuv(20, 6, seed=31, n=3)
    job = PlanarJob(rig, planes, pads=(4, 6, 0, 16), spacing="table", transfer=gh.TRANSFER_FOR_GAMMA[APPLE])
    try:
        _capi.check(job.decode_batch(rig.decoder(gamma=APPLE, has_alpha=False, options=[(OPT, I420)])))
        assert rig.kernel() == b"decode_i420_quads<nt>"
        grid, block, launches, bands = rig.launch()
        assert launches == 1 and grid[2] == 3 and bands == 0
        got = job.collect("table of 3")
    finally:
        job.free()
    for i in range(3):
        vc.assert_equal(got[i], want_of(oracle, APPLE, planes[i]), "table of 3, frame %d" % i)


def test_batch_of_70_takes_the_band_map_and_a_plain_tail(rig, gh, oracle):
    """70 evenly spaced 64 x 4 frames: the XCD-band map over 64 of them, the plain map over the other 6 -- two launches, the
    first on record -- and V follows each frame's own U plane."""
    n, w, h = 70, 64, 4
    planes = random_yuv(w, h, seed=70, n=n)
    job = PlanarJob(rig, planes, pads=(0, 2, 0, 0), transfer=gh.TRANSFER_FOR_GAMMA[LINEAR])
    try:
        dec = rig.decoder(gamma=LINEAR, has_alpha=False, options=[(OPT, I420)])
        assert rig.option(dec, _capi.OPT_XCD_BANDS) == 1
        _capi.check(job.decode_batch(dec))
        assert rig.kernel() == b"decode_i420_quads_log<nt>"
        grid, block, launches, bands = rig.launch()
        assert launches == 2 and bands == 1 and grid[0] == 8 and grid[2] == 8, (grid, block, launches, bands)
        got = job.collect("70 frames")
    finally:
        job.free()
    for i in range(n):
        vc.assert_equal(got[i], want_of(oracle, LINEAR, planes[i]), "70 frames, frame %d" % i)


# ------------------------------------------------------------------ 4. alpha decoders and the composite-over option

OVER_COLOUR = 0x3C7FB2
OVER_NAMES = {None: b"<alpha>", "destination": b"<alpha,over>", "colour": b"<alpha,over-colour>"}


@pytest.mark.parametrize("over", [None, "destination", "colour"])
@pytest.mark.parametrize("size,pads,path", [((64, 8), (4, 6, 12, 16), "quads"), ((62, 6), (1, 3, 2, 4), "blocks")], ids=["64x8", "62x6"])
def test_alpha_and_composite_over(rig, oracle, tabs, size, pads, path, over):
    """An alpha decoder, plain and blended over a colour and over the destination: the definition's bytes (tests/over_cases.py),
    and the NV12 kernels' bytes for the interleaved twin."""
    w, h = size
    planes = random_yuv(w, h, seed=w + h, n=2, alpha=True)
    bg = vc.random_backgrounds(w, h, seed=w * h, n=2) if over == "destination" else None
    value = {None: None, "destination": _capi.OVER_DESTINATION, "colour": OVER_COLOUR}[over]
    dec = rig.decoder(value)
    got = {}
    for layout in (I420, NV12):
        if layout == I420:
            job = PlanarJob(rig, planes, pads=pads)
        else:
            job = vc.Job(rig, [(y, interleave(u, v), a) for y, u, v, a in planes], pads=(pads[0], 2 * pads[1] + (pads[1] & 1), pads[2], pads[3]))
        try:
            job.fill(bg)
            _capi.check(rig.lib.bt709hip_decoder_set_option(dec, OPT, layout))
            _capi.check(job.decode_batch(dec))
            assert rig.kernel() == (b"decode_i420_" if layout == I420 else b"decode_nv12_") + path.encode() + OVER_NAMES[over], rig.kernel()
            got[layout] = job.collect("%s, over %s" % (path, over))
        finally:
            job.free()
    for i in range(2):
        want = want_of(oracle, SRGB, planes[i])
        if over:
            want = oc.composite_over(want, bg[i] if bg else OVER_COLOUR, *tabs)
        vc.assert_equal(got[I420][i], want, "%s, over %s, frame %d" % (path, over, i))
        vc.assert_equal(got[I420][i], got[NV12][i], "%s, over %s, frame %d against the NV12 path" % (path, over, i))


# ------------------------------------------------------------------ 5. a Y4M payload in place, and the Python mirror

def test_y4m_payload_decoded_in_place(rig, gh, oracle):
    """One tight FRAME payload -- Y, U, V back to back -- uploaded as a single blob: y = base, cbcr = base + W*H, pitch W/2.  It
    decodes to what the interleave detour (i420_to_pixel_buffer + the NV12 decode) gives."""
    from metalbt709decoder_amd import y4m
    w, h = 64, 16
    (y, u, v, _), = random_yuv(w, h, seed=420)
    blob = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])
    assert blob.size == w * h * 3 // 2
    d_in, d_out = rig.DeviceBuffer(rig.ctx, blob.size, placement_tries=1), rig.DeviceBuffer(rig.ctx, w * h * 4, placement_tries=1)
    try:
        rig.upload(d_in.ptr, blob)
        frame = Frame(d_in.ptr, w, d_in.ptr + w * h, w // 2, w, h, vc.MATRIX, gh.TRANSFER_FOR_GAMMA[APPLE])
        surf = Surface(d_out.ptr, 4 * w, w, h, _capi.FORMAT_BGRA8_SRGB, 0)
        dec = rig.decoder(gamma=APPLE, has_alpha=False, options=[(OPT, I420)])
        _capi.check(rig.lib.bt709hip_decode(dec, C.byref(frame), None, C.byref(surf), w, h, None, 1))
        assert rig.kernel() == b"decode_i420_quads<nt>"
        got = rig.download(d_out.ptr, w * h * 4).reshape(h, w * 4)
    finally:
        d_in.free()
        d_out.free()
    # the path the feature replaces
    ctx = gh.context()
    buf = y4m.i420_to_pixel_buffer(ctx, y, u, v)
    tex = ctx.makeBGRATexture((w, h))
    nv12_dec = gh.make_decoder(APPLE)
    assert nv12_dec.decodeBT709(buf, None, tex, ctx.commandQueue.commandBuffer(), None, w, h, True)
    assert ctx.lib.bt709hip_last_kernel_name() == b"decode_nv12_quads<nt>"
    detour = ctx.getBGRATexturePixels(tex).view(np.uint8).reshape(h, w * 4)
    assert np.array_equal(got, detour)
    assert np.array_equal(got.reshape(h, w, 4), want_of(oracle, APPLE, (y, u, v, None)))


def test_python_mirror_picks_the_layout_from_the_buffer(gh, oracle):
    from metalbt709decoder_amd import y4m
    ctx = gh.context()
    w, h = 64, 16
    (y, u, v, _), = random_yuv(w, h, seed=421)
    want = want_of(oracle, APPLE, (y, u, v, None)).reshape(h, w * 4)
    dec = gh.make_decoder(APPLE)
    planar = y4m.i420_to_pixel_buffer(ctx, y, u, v, planar=True)  # three uploads, no launch
    assert planar.planar and planar.cbcr_stride == 32 and len(planar.planes()) == 3
    back = y4m.pixel_buffer_to_i420(planar)  # a plain download
    assert all(np.array_equal(a, b) for a, b in zip(back, (y, u, v)))
    nv12 = y4m.i420_to_pixel_buffer(ctx, y, u, v)
    tex = ctx.makeBGRATexture((w, h))
    for buf, layout, name in ((planar, I420, b"decode_i420_quads<nt>"), (nv12, NV12, b"decode_nv12_quads<nt>"), (planar, I420, b"decode_i420_quads<nt>")):
        assert dec.decodeBT709(buf, None, tex, ctx.commandQueue.commandBuffer(), None, w, h, True), dec.lastStatus
        assert ctx.lib.bt709hip_last_kernel_name() == name
        assert dec._options.get(OPT, NV12) == layout
        assert np.array_equal(ctx.getBGRATexturePixels(tex).view(np.uint8).reshape(h, w * 4), want)
    # the refused combinations: False, lastStatus ERR_UNSUPPORTED, the target untouched
    for size in ((w // 2, h // 2), (48, 10)):  # the exact 2:1 kernels and the any-ratio kernel
        small = ctx.makeBGRATexture(size)
        before = ctx.getBGRATexturePixels(small).copy()
        assert not dec.decodeBT709Scaled(planar, small, ctx.commandQueue.commandBuffer(), True)
        assert dec.lastStatus == _capi.ERR_UNSUPPORTED
        assert np.array_equal(ctx.getBGRATexturePixels(small), before)
        assert dec.decodeBT709Scaled(nv12, small, ctx.commandQueue.commandBuffer(), True), dec.lastStatus
    half = ctx.makeBGRATexture((w, h), pixelFormat=mb.MTLPixelFormatRGBA16Float)
    assert not dec.decodeBT709(planar, None, half, ctx.commandQueue.commandBuffer(), None, w, h, True)
    assert dec.lastStatus == _capi.ERR_UNSUPPORTED
    assert dec.decodeBT709(nv12, None, half, ctx.commandQueue.commandBuffer(), None, w, h, True), dec.lastStatus


# ------------------------------------------------------------------ 6. rings stay NV12

def test_ring_stays_nv12_with_the_option_on(gh, oracle):
    ctx = gh.context()
    w, h, n = 64, 16, 4
    dec = gh.make_decoder(APPLE, options={OPT: I420})
    ring = mb.FrameRing(dec, (w, h), n, tries=1)
    try:
        frames = [gh.random_nv12(w, h, seed=900 + i) for i in range(n)]
        for i, (y, c) in enumerate(frames):
            buf = ring.pixelBuffer(i)
            assert not buf.planar and buf.cbcr_stride >= w  # it keeps describing NV12 planes
            buf.upload_planes(y, c)
        assert ring.decode(0, n, waitUntilCompleted=True), dec.lastStatus
        assert ctx.lib.bt709hip_last_kernel_name() == b"decode_nv12_quads<nt>"
        v = C.c_int(-1)
        _capi.check(ctx.lib.bt709hip_decoder_get_option(dec._handle, OPT, C.byref(v)))
        assert v.value == I420
        for i, (y, c) in enumerate(frames):
            got = ctx.getBGRATexturePixels(ring.texture(i)).view(np.uint8).reshape(h, w * 4)
            assert np.array_equal(got, oracle.decode_nv12(APPLE, y, c).reshape(h, w * 4)), i
    finally:
        ring.release()
