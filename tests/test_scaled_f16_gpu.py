"""The fused decode + rescale through the RGBA16Float intermediate (BT709HIP_OPT_SCALE_INTERMEDIATE = RGBA16F) on
the GPU: bytes against the oracle's composition of its two pinned halves,

    oracle.render_scaled(oracle.decode_nv12_rgba16f(gamma, y, uv, alpha), OW, OH)

(pass 2: tests/golden/pass2.json; the RGBA16F decode: the 2^24 half-float sweep), every pixel compared, and against the
product's own two launches.  The reference leaves the filter to the sampler hardware: PARITY UNPINNED, as for the 8-bit mode."""
import ctypes as C

import numpy as np
import pytest

import metalbt709decoder_amd as mb
import rescale_arith_cases as rc
from metalbt709decoder_amd import _capi
from metalbt709decoder_amd.decoder import Frame, Surface

F16, SRGB8 = _capi.FORMAT_RGBA16F, _capi.FORMAT_BGRA8_SRGB
TAPS_NAME = {_capi.SCALED_TAPS_BYTES: "bytes", _capi.SCALED_TAPS_PAIRS: "pairs", _capi.SCALED_TAPS_WIDE: "wide",
             _capi.SCALED_TAPS_SHARED: "shared", _capi.SCALED_TAPS_ONCE: "once"}

# The smallest shapes that still cross a wave, a 256-column tile and a strip boundary.  layout: "aligned" -- plane addresses
# and pitches multiples of 4; "off2" -- planes 2 bytes past that, pitches 2 mod 4; "off1" -- planes 1 byte past it, odd pitches.
# taps: the form(s) the launcher's record must name (bt709_rescale_scaled.hip scaled_taps).
# "x-up-y-down" is the shape the feature's request lists for the wave-fetches form; scaled_taps gives that form only when the
# view is TALLER than the frame (scale_y < 1) and not much wider (scale_x > 0.95), so that shape runs `wide` and the case after
# it, the same two sizes the other way round, is the one that runs `shared`.  Both stay.
SHAPES = [
    ("once", (96, 54), (300, 170), "aligned", ("once",)),            # two tiles, a partial last trip
    ("wide", (520, 292), (346, 194), "aligned", ("wide",)),          # ratio 1.5, persistent
    ("pairs", (520, 292), (346, 194), "off2", ("pairs",)),
    ("bytes", (520, 292), (346, 194), "off1", ("bytes",)),
    ("x-up-y-down", (264, 40), (300, 36), "aligned", ("wide",)),     # enlarging in x, reducing in y
    ("shared", (300, 36), (264, 40), "aligned", ("shared",)),        # reducing in x, enlarging in y
    ("decimate", (200, 120), (60, 36), "aligned", ("bytes", "pairs", "wide")),   # ratio above 2
    ("identity", (40, 24), (40, 24), "aligned", ("bytes", "pairs", "wide")),
]
SHAPE = {s[0]: s for s in SHAPES}
DECODERS = [(0, False), (1, False), (2, False), (3, False), (mb.MetalBT709GammaSRGB, True)]  # the four gammas, an alpha decoder
SPACINGS = [("x1", 1, "ring"), ("x3-table", 3, "table"), ("x3-ring", 3, "ring")]


@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


def _round_up(v, a):
    return (v + a - 1) // a * a


# ------------------------------------------------------------------ frames and what the oracle makes of them, computed once

_memo = {}


def _planes(shape, i):
    """Frame i of a shape: uniform random bytes (y, cbcr, alpha)."""
    key = ("planes", shape, i)
    if key not in _memo:
        (w, h) = SHAPE[shape][1]
        rng = np.random.default_rng(1600 + 16 * [s[0] for s in SHAPES].index(shape) + i)
        _memo[key] = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8),
                      rng.integers(0, 256, (h, w), dtype=np.uint8))
    return _memo[key]


def _want(oracle, shape, gamma, alpha, i, mode=F16):
    """The view of frame i: the RGBA16F composition (the definition of the mode), or the 8-bit composition."""
    key = ("want", shape, gamma, alpha, i, mode)
    if key not in _memo:
        y, c, a = _planes(shape, i)
        ow, oh = SHAPE[shape][2]
        a = a if alpha else None
        if mode == F16:
            _memo[key] = oracle.render_scaled(oracle.decode_nv12_rgba16f(gamma, y, c, a), ow, oh)
        else:
            _memo[key] = oracle.decode_nv12_scaled(gamma, y, c, ow, oh, alpha=a)
    return _memo[key]


# ------------------------------------------------------------------ device side

class _Slots:
    """`count` slots in one device allocation pre-filled with 0x5A, a 256-byte guard in front: evenly spaced ("ring"), or with a
    gap before the last one ("table": no single step reaches every frame, so the launch takes the pointer table)."""

    def __init__(self, ctx, count, slot_bytes, pitch, spacing):
        from metalbt709decoder_amd.decoder import DeviceBuffer
        self.offsets = [256 + i * pitch + (256 if spacing == "table" and i == count - 1 and count > 1 else 0) for i in range(count)]
        self.nbytes = self.offsets[-1] + slot_bytes + 256
        self.ctx, self.buf = ctx, DeviceBuffer(ctx, self.nbytes)
        _capi.check(ctx.lib.bt709hip_memset(ctx.handle, self.buf.ptr, rc.FILL, self.nbytes, None))
        ctx._sync(None)

    def ptr(self, i):
        return self.buf.ptr + self.offsets[i]

    def download(self):
        raw = np.empty(self.nbytes, np.uint8)
        _capi.check(self.ctx.lib.bt709hip_download(self.ctx.handle, raw.ctypes.data, self.nbytes, self.buf.ptr, self.nbytes, self.nbytes, 1, None))
        self.ctx._sync(None)
        return raw


def _plan(ctx):
    info = _capi.ScaledLaunchInfo()
    _capi.check(ctx.lib.bt709hip_last_scaled_launch_info(C.byref(info)))
    return dict(grid=tuple(info.grid), block=tuple(info.block), taps=TAPS_NAME.get(info.taps, info.taps), rows=info.rows,
                persistent=info.persistent, balanced=info.balanced, resident=info.resident, items=info.items)


class _Batch:
    """`count` frames of a shape in device memory in the shape's layout, and padded views for them."""

    def __init__(self, gh, shape, gamma, alpha, count, spacing, out_size=None):
        self.gh, self.ctx, self.shape, self.alpha, self.count = gh, gh.context(), shape, alpha, count
        _, (w, h), dst, layout, _ = SHAPE[shape]
        self.ow, self.oh = out_size or dst
        off, ys, cs = {"aligned": (0, _round_up(w, 4), _round_up(w, 4)), "off2": (2, w + 2, w + 2), "off1": (1, w + 1, w + 3)}[layout]
        c_off = _round_up(off + ys * h, 256) + off
        a_off = _round_up(c_off + cs * (h // 2), 256) + off
        in_pitch = _round_up(a_off + ys * h, 256)
        self.stride = 4 * self.ow + 16
        self.slab_in = _Slots(self.ctx, count, in_pitch, in_pitch, spacing)
        self.slab_out = _Slots(self.ctx, count, self.stride * self.oh, _round_up(self.stride * self.oh, 256), spacing)
        self.bufs, self.abufs, self.texs = [], [], []
        for i in range(count):
            y, c, a = _planes(shape, i)
            base = self.slab_in.ptr(i)
            self.ctx._upload(base + off, ys, y, None, wait=False)
            self.ctx._upload(base + c_off, cs, c, None, wait=False)
            b = mb.CVPixelBuffer(self.ctx, w, h, ys, cs, planes=(base + off, base + c_off))
            b.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
            b.setAttachment("TransferFunction", gh.TRANSFER_FOR_GAMMA[gamma])
            self.bufs.append(b)
            if alpha:
                self.ctx._upload(base + a_off, ys, a, None, wait=False)
                ab = mb.CVPixelBuffer(self.ctx, w, h, ys, cs, planes=(base + a_off, base + c_off))
                ab.setAttachment("TransferFunction", mb.kCVImageBufferTransferFunction_Linear)
                self.abufs.append(ab)
            self.ctx._sync(None)
            self.texs.append(mb.BGRATexture(self.ctx, self.ow, self.oh, self.stride, ptr=self.slab_out.ptr(i)))

    def launch(self, dec, entry="bt709hip_decode_scaled_batch"):
        """One launch over the batch through the C entry point (called directly: the Python wrapper picks between them itself)."""
        n = self.count
        frames = (Frame * n)(*[b.frame() for b in self.bufs])
        surfs = (Surface * n)(*[t.surface() for t in self.texs])
        alphas = (Frame * n)(*[b.frame() for b in self.abufs]) if self.alpha else None
        if entry.endswith("_batch"):
            _capi.check(getattr(self.ctx.lib, entry)(dec._handle, n, frames, alphas, surfs, None, 1), entry)
        else:
            assert n == 1
            _capi.check(getattr(self.ctx.lib, entry)(dec._handle, C.byref(frames[0]), C.byref(alphas[0]) if alphas else None,
                                                      C.byref(surfs[0]), None, 1), entry)
        return self.ctx.lib.bt709hip_last_kernel_name(), _plan(self.ctx)

    def views(self, label, want=None):
        """-> the views' bytes [(oh, 4 ow)]; everything else in the slab must still hold the fill; `want`: compared, every byte."""
        raw = self.slab_out.download()
        untouched = np.ones(raw.size, bool)
        got = []
        for i in range(self.count):
            o = self.slab_out.offsets[i]
            rows = raw[o:o + self.stride * self.oh].reshape(self.oh, self.stride)
            got.append(rows[:, :4 * self.ow].copy())
            untouched[o:o + self.stride * self.oh].reshape(self.oh, self.stride)[:, :4 * self.ow] = False
        stray = np.flatnonzero(untouched & (raw != rc.FILL))
        assert stray.size == 0, "%s: %d bytes written outside the views, first at slab offset %d" % (label, stray.size, stray[0])
        for i, w in enumerate(want or []):
            if not np.array_equal(got[i], w):
                r, b = np.argwhere(got[i] != w)[0]
                raise AssertionError("%s: frame %d differs first at row %d, column %d, channel %s (got %d, want %d); %d of %d pixels differ"
                                     % (label, i, r, b // 4, "BGRA"[b % 4], got[i][r, b], w[r, b],
                                        int((got[i] != w).reshape(self.oh, self.ow, 4).any(axis=2).sum()), self.ow * self.oh))
        return got


def _decoder(gh, gamma, alpha, mode=F16, alpha_fill=0xFF):
    return gh.make_decoder(gamma, has_alpha=alpha, alpha_fill=alpha_fill, options={_capi.OPT_SCALE_INTERMEDIATE: mode})


def _name(alpha, mode=F16):
    base = b"decode_nv12_scaled_f16" if mode == F16 else b"decode_nv12_scaled"
    return base + b"<alpha>" if alpha else base


# ------------------------------------------------------------------ 1. every tap form, both launch kinds

@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_gpu_every_tap_form_and_launch_kind(gh, oracle, shape):
    """Each shape with the four gammas and an alpha decoder, one frame, three through the pointer table and three evenly
    spaced: the launcher's record names the tap form, every tap form runs the persistent item loop in this mode, and every
    byte of every view is the composition's; padded output rows between guard bands stay untouched."""
    _, (w, h), (ow, oh), _, taps = SHAPE[shape]
    cols = -(-ow // 256)
    for gamma, alpha in DECODERS:
        dec = _decoder(gh, gamma, alpha)
        for tag, count, spacing in SPACINGS:
            label = "%s gamma %d%s %s" % (shape, gamma, " alpha" if alpha else "", tag)
            batch = _Batch(gh, shape, gamma, alpha, count, spacing)
            name, plan = batch.launch(dec)
            assert name == _name(alpha), (label, name)
            assert plan["taps"] in taps and plan["persistent"] == 1 and plan["block"] == (256, 1, 1), (label, plan)
            assert plan["items"] == cols * (-(-oh // plan["rows"])) * count, (label, plan)
            assert plan["grid"] == (min(plan["items"], plan["resident"]), 1, 1), (label, plan)
            if shape == "once":  # two column tiles; strips of whole trips (4 rows) with a partial last one
                assert cols == 2 and plan["rows"] % 4 == 0 and oh % plan["rows"] % 4 != 0, (label, plan)
            batch.views(label, [_want(oracle, shape, gamma, alpha, i) for i in range(count)])


# ------------------------------------------------------------------ 2. the mode is not a no-op

@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s[0] for s in SHAPES if s[0] != "identity"])
def test_gpu_the_mode_changes_the_output_and_can_be_switched_back(gh, oracle, shape):
    """From the oracle alone: the 8-bit composition and the RGBA16F composition of the same random frame differ in at least a
    tenth of the pixels (26-31 % where it was measured), so a kernel that ignored the option could not pass.  The GPU gives the
    RGBA16F composition with the option on and, the same decoder, the 8-bit composition again with it back at 0."""
    ow, oh = SHAPE[shape][2]
    want16, want8 = _want(oracle, shape, 0, False, 0), _want(oracle, shape, 0, False, 0, SRGB8)
    differing = int((want16 != want8).reshape(oh, ow, 4).any(axis=2).sum())
    print("%s: the two definitions differ in %d of %d pixels (%.1f %%)" % (shape, differing, ow * oh, 100.0 * differing / (ow * oh)))
    assert differing >= 0.10 * ow * oh, (shape, differing)
    dec = _decoder(gh, 0, False)
    batch = _Batch(gh, shape, 0, False, 1, "ring")
    assert batch.launch(dec)[0] == _name(False)
    batch.views(shape + " option at RGBA16F", [want16])
    dec.setOption(_capi.OPT_SCALE_INTERMEDIATE, SRGB8)
    assert batch.launch(dec)[0] == _name(False, SRGB8)
    batch.views(shape + " option back at 0", [want8])


# ------------------------------------------------------------------ 3. equal to the product's own two passes

@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [False, True], ids=["opaque", "alpha"])
@pytest.mark.parametrize("shape", ["once", "wide", "bytes"])
def test_gpu_equals_decode_to_rgba16f_then_render_scaled(gh, oracle, shape, alpha):
    """bt709hip_decode into an RGBA16F surface of the frame's size followed by bt709hip_render_scaled from it, byte for byte --
    with the decoder's alpha fill at 0: the half target of a decoder without an alpha channel holds 1.0, so both write A = 0xFF."""
    ctx = gh.context()
    _, (w, h), (ow, oh), _, _ = SHAPE[shape]
    gamma = mb.MetalBT709GammaSRGB if alpha else mb.MetalBT709GammaApple
    dec = _decoder(gh, gamma, alpha, alpha_fill=0)
    batch = _Batch(gh, shape, gamma, alpha, 1, "ring")
    assert batch.launch(dec, "bt709hip_decode_scaled")[0] == _name(alpha)
    fused = batch.views(shape + " fused")[0]
    inter = ctx.makeBGRATexture((w, h), pixelFormat=mb.MTLPixelFormatRGBA16Float)
    view = ctx.makeBGRATexture((ow, oh))
    assert dec.decodeBT709(batch.bufs[0], batch.abufs[0] if alpha else None, inter, None, None, w, h, True), dec.lastStatus
    scale = mb.MetalScaleRenderContext()
    assert scale.setupRenderPipelines(ctx)
    assert scale.renderScaled(ctx, view, ow, oh, None, None, inter, True), scale.lastStatus
    assert ctx.lib.bt709hip_last_kernel_name() == b"render_scaled<rgba16f>"
    two_pass = ctx.getBGRATexturePixels(view).view(np.uint8).reshape(oh, ow * 4)
    assert np.array_equal(fused, two_pass), (shape, alpha, int((fused != two_pass).sum()))
    if not alpha:
        assert (fused[:, 3::4] == 0xFF).all()


# ------------------------------------------------------------------ 4. every colour

def _code_to_byte(oracle):
    """byte of a channel whose four taps all hold half code k, for every k in [0, 0x3c00]: pass 2 of the oracle over an image
    of flat 2x2 blocks, block k = code k in all four channels, to exactly half its size.  -> (colour bytes, alpha bytes)."""
    side = 124  # 124^2 = 15 376 blocks >= 0x3c01 codes
    codes = np.minimum(np.arange(side * side, dtype=np.uint16), 0x3c00).reshape(side, side)
    img = np.repeat(np.repeat(codes, 2, axis=0), 2, axis=1)[:, :, None].repeat(4, axis=2).view(np.float16)
    out = oracle.render_scaled(np.ascontiguousarray(img), side, side).reshape(side * side, 4)
    return out[:0x3c01, 2].copy(), out[:0x3c01, 3].copy()


@pytest.fixture(scope="module")
def every_colour(gh):
    """All 2^24 triples as flat 2x2 blocks, 8192 x 8192, uploaded once."""
    from test_rescale_arith import DeviceFrame
    Y, Cb, Cr = rc.blocks_of(*gh.exhaustive_frame())
    idx = ((Y.astype(np.uint32) << 16) | (Cb.astype(np.uint32) << 8) | Cr.astype(np.uint32)).reshape(-1)
    return dict(dev=DeviceFrame(gh, *rc.flat_frame(Y, Cb, Cr)), idx=idx, blocks=(Y, Cb, Cr), maps={})


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", [0, 1, 2, 3])
def test_gpu_every_colour_through_the_half_lookup(gh, oracle, every_colour, gamma):
    """All 2^24 (Y, Cb, Cr) as flat 2x2 blocks through bt709hip_decode_half_batch in this mode.  Expected, per channel: the
    encode of float(half code), the code from oracle.half_table, the code -> byte map from oracle.render_scaled over a flat half
    image per code.  That IS the composition: the four taps of a flat block hold one half H, every weight of an exact 2:1 is
    0.25, and ((0.25 H + 0.25 H) + 0.25 H) + 0.25 H is H without a rounding (a half is at least 2^-24, so no product or sum is
    subnormal): pass 2's output for the block is its encode of float(H), which is what the map records."""
    from test_rescale_arith import Target
    ctx = gh.context()
    if "byte" not in every_colour["maps"]:
        every_colour["maps"]["byte"] = _code_to_byte(oracle)[0]
    byte_of = every_colour["maps"]["byte"]
    rgb = byte_of[oracle.half_table(gamma)[every_colour["idx"]]]  # (2^24 blocks in image order, 3)
    want = np.empty((rgb.shape[0], 4), np.uint8)
    want[:, 0], want[:, 1], want[:, 2], want[:, 3] = rgb[:, 2], rgb[:, 1], rgb[:, 0], 0xFF
    want = want.reshape(4096, 4096 * 4)
    dec = _decoder(gh, gamma, False)
    dev, target = every_colour["dev"], Target(ctx, 4096, 4096)
    frame, surf = (Frame * 1)(dev.frame(gamma)), (Surface * 1)(target.tex.surface())
    _capi.check(ctx.lib.bt709hip_decode_half_batch(dec._handle, 1, frame, None, surf, None, 1))
    assert ctx.lib.bt709hip_last_kernel_name() == b"decode_nv12_scaled_f16"
    got = target.read()
    if not np.array_equal(got, want):
        r, b = np.argwhere(got != want)[0]
        Y, Cb, Cr = (int(a[r, b // 4]) for a in every_colour["blocks"])
        raise AssertionError("gamma %d: (Y, Cb, Cr) = (%d, %d, %d) channel %s: got %d, want %d; %d bytes differ"
                             % (gamma, Y, Cb, Cr, "BGRA"[b % 4], got[r, b], want[r, b], int((got != want).sum())))


@pytest.mark.gpu
def test_gpu_every_alpha_code_in_every_lane_position(gh, oracle):
    """The alpha decoder: flat 2x2 alpha blocks, block (r, c) = code (r + c) mod 256, 256 rows of 64 -- every code in every lane
    position of a wave -- through bt709hip_decode_half_batch in this mode, against the composition; and, as for the colours,
    against the encode of float(half(alpha_value(code))) read from the flat-image map."""
    from test_rescale_arith import DeviceFrame, Target
    ctx = gh.context()
    r, c = np.meshgrid(np.arange(256), np.arange(64), indexing="ij")
    codes = ((r + c) & 255).astype(np.uint8)
    a = np.repeat(np.repeat(codes, 2, axis=0), 2, axis=1)
    rng = np.random.default_rng(416)
    y, cbcr = rng.integers(0, 256, (512, 128), dtype=np.uint8), rng.integers(0, 256, (256, 128), dtype=np.uint8)
    gamma = mb.MetalBT709GammaSRGB
    inter = oracle.decode_nv12_rgba16f(gamma, y, cbcr, a)
    want = oracle.render_scaled(inter, 64, 256)
    alpha_byte = _code_to_byte(oracle)[1]
    assert np.array_equal(want[:, 3::4], alpha_byte[inter[0::2, 0::2, 3].view(np.uint16)])  # the two statements of the expectation agree
    assert len(np.unique(want[:, 3::4])) > 200
    dec = _decoder(gh, gamma, True)
    dev, adev, target = DeviceFrame(gh, y, cbcr), DeviceFrame(gh, a, cbcr), Target(ctx, 64, 256)
    aframe = adev.frame(gamma)
    aframe.transfer = mb.kCVImageBufferTransferFunction_Linear
    frame, alphas, surf = (Frame * 1)(dev.frame(gamma)), (Frame * 1)(aframe), (Surface * 1)(target.tex.surface())
    _capi.check(ctx.lib.bt709hip_decode_half_batch(dec._handle, 1, frame, alphas, surf, None, 1))
    assert ctx.lib.bt709hip_last_kernel_name() == b"decode_nv12_scaled_f16<alpha>"
    got = target.read()
    assert np.array_equal(got[:, 3::4], want[:, 3::4]), int((got[:, 3::4] != want[:, 3::4]).sum())
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 5. the 2:1 entry points run the same kernel

@pytest.mark.gpu
@pytest.mark.parametrize("shape", [("once", (64, 36)), ("wide", (520, 292))], ids=["64x36", "520x292"])
def test_gpu_decode_half_equals_decode_scaled_at_exactly_half(gh, oracle, shape):
    """bt709hip_decode_half against bt709hip_decode_scaled at exactly W/2 x H/2 in this mode: the same kernel at ratio 2.0, equal
    bytes -- and the composition's."""
    base, (w, h) = shape
    key = "half-%dx%d" % (w, h)
    if key not in SHAPE:  # the planes of a frame of this size, under a name of its own
        SHAPE[key] = (key, (w, h), (w // 2, h // 2), "aligned", ("wide",))
        rng = np.random.default_rng(5000 + w)
        _memo[("planes", key, 0)] = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8),
                                     rng.integers(0, 256, (h, w), dtype=np.uint8))
    for gamma, alpha in ((0, False), (2, False), (mb.MetalBT709GammaSRGB, True)):
        dec = _decoder(gh, gamma, alpha)
        want = _want(oracle, key, gamma, alpha, 0)
        got = {}
        for entry in ("bt709hip_decode_half", "bt709hip_decode_scaled"):
            batch = _Batch(gh, key, gamma, alpha, 1, "ring")
            name, plan = batch.launch(dec, entry)
            assert name == _name(alpha) and plan["persistent"] == 1, (entry, name, plan)
            got[entry] = batch.views("%s %s gamma %d" % (key, entry, gamma), [want])[0]
        assert np.array_equal(got["bt709hip_decode_half"], got["bt709hip_decode_scaled"])
