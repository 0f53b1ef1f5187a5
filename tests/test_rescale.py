"""Fused decode + rescale to any view size (reference pass 2 =
Renderer/MetalScaleRenderContext.m:55-105 + AAPLShaders.metal:73-85).  The reference leaves the
filtering arithmetic to the sampler hardware and has no test of it: PARITY UNPINNED, the oracle
holds our definition and the GPU is checked against it bit for bit."""
import numpy as np
import pytest

import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi


def _frame(w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)


# ------------------------------------------------------------------ CPU (definition)

def test_scaled_equals_half_at_exact_2_to_1(oracle):
    """Every weight is exactly 0.25 at a 2:1 ratio, so the general definition reproduces the
    2:1 kernel's (((a+b)+c)+d)*0.25f bit for bit."""
    for gamma in range(4):
        y, c = _frame(48, 24, 3 + gamma)
        assert np.array_equal(oracle.decode_nv12_scaled(gamma, y, c, 24, 12), oracle.decode_nv12_half(gamma, y, c))


def test_scaled_identity_is_plain_decode(oracle):
    """1:1: every sample falls on a texel centre (fx = fy = 0): linearise, re-encode = the byte itself."""
    y, c = _frame(32, 16, 9)
    for gamma in range(4):
        assert np.array_equal(oracle.decode_nv12_scaled(gamma, y, c, 32, 16), oracle.decode_nv12(gamma, y, c))


def test_scaled_flat_frame_any_ratio(oracle):
    y = np.full((20, 36), 150, np.uint8)
    c = np.full((10, 36), 128, np.uint8)
    px = oracle.decode_nv12(0, y, c).reshape(-1, 4)[0]
    for ow, oh in [(7, 5), (36, 20), (50, 33), (1, 1), (100, 3)]:
        out = oracle.decode_nv12_scaled(0, y, c, ow, oh).reshape(-1, 4)
        # weights sum to 1 only up to float rounding; a flat field may move by at most one code
        assert (np.abs(out.astype(int) - px.astype(int)) <= 1).all()


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


def gpu_scaled(gh, y, c, ow, oh, gamma, alpha=None):
    got = gh.gpu_decode_scaled(y, c, (ow, oh), gamma, alpha=alpha)
    assert got is not None
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [((64, 32), (40, 20)), ((64, 32), (17, 9)), ((30, 18), (64, 40)), ((1920, 64), (1280, 43)),
                                   ((50, 22), (1, 1)), ((48, 24), (24, 12)), ((32, 16), (32, 16))])
def test_gpu_scaled_matches_oracle(gh, oracle, gamma, shape):
    (w, h), (ow, oh) = shape
    y, c = _frame(w, h, w + h + ow + gamma)
    got = gpu_scaled(gh, y, c, ow, oh, gamma)
    assert np.array_equal(got, oracle.decode_nv12_scaled(gamma, y, c, ow, oh))


@pytest.mark.gpu
@pytest.mark.parametrize("strides", [(67, 65), (64, 66), (80, 64)])
def test_gpu_scaled_odd_strides_and_many_rows(gh, oracle, strides):
    """Odd plane strides take the byte-gather form of the kernel (an even CbCr plane: one 2-byte load
    per tap); a tall output makes a workgroup walk several rows."""
    ctx = gh.context()
    y, c = _frame(64, 600, 5)
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    buf = gh.make_buffer(y, c, dec.gamma, y_stride=strides[0], cbcr_stride=strides[1])
    tex = ctx.makeBGRATexture((300, 4000))
    assert dec.decodeBT709Scaled(buf, tex, ctx.commandQueue.commandBuffer(), True), dec.lastStatus
    got = ctx.getBGRATexturePixels(tex).view(np.uint8).reshape(4000, 300 * 4)
    assert np.array_equal(got, oracle.decode_nv12_scaled(0, y, c, 300, 4000))


@pytest.mark.gpu
def test_gpu_view_fit_like_the_renderer(gh, oracle):
    """AAPLRenderer's case: a 1920x1080 frame into a view of another aspect and size
    (AAPLRenderer.m:891-977 takes the 2-pass route whenever the sizes differ)."""
    y, c = _frame(1920, 1080, 77)
    got = gpu_scaled(gh, y, c, 1366, 768, mb.MetalBT709GammaApple)
    assert np.array_equal(got, oracle.decode_nv12_scaled(0, y, c, 1366, 768))


@pytest.mark.gpu
def test_gpu_scaled_bad_tags_and_missing_alpha(gh):
    ctx = gh.context()
    y, c = _frame(16, 8, 1)
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    srgb_tagged = gh.make_buffer(y, c, mb.MetalBT709GammaSRGB)
    assert not dec.decodeBT709Scaled(srgb_tagged, ctx.makeBGRATexture((5, 3)), None, True)
    assert dec.lastStatus == _capi.ERR_TRANSFER
    da = gh.make_decoder(mb.MetalBT709GammaSRGB, has_alpha=True)
    assert not da.decodeBT709Scaled(srgb_tagged, ctx.makeBGRATexture((5, 3)), None, True)  # an alpha decoder needs its alpha buffer
    assert da.lastStatus == _capi.ERR_INVALID_ARG
    rgba16 = ctx.makeBGRATexture((5, 3), pixelFormat=mb.MTLPixelFormatRGBA16Float)
    assert not dec.decodeBT709Scaled(gh.make_buffer(y, c, dec.gamma), rgba16, None, True)  # pass 2 writes the 8-bit view
    assert dec.lastStatus == _capi.ERR_UNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [((64, 32), (40, 20)), ((30, 18), (64, 40)), ((1920, 64), (1280, 43)), ((48, 24), (24, 12)),
                                   ((50, 22), (1, 1))])
def test_gpu_scaled_with_alpha(gh, oracle, shape):
    """Alpha clips through the view-fit path: the alpha channel is filtered as a plain unorm with the
    same taps and weights (AAPLShaders.metal:411-438 -> MetalScaleRenderContext.m:55-105)."""
    (w, h), (ow, oh) = shape
    y, c = _frame(w, h, w + ow)
    a = np.random.default_rng(h + oh).integers(0, 256, (h, w), dtype=np.uint8)
    got = gpu_scaled(gh, y, c, ow, oh, mb.MetalBT709GammaSRGB, alpha=a)
    assert np.array_equal(got, oracle.decode_nv12_scaled(mb.MetalBT709GammaSRGB, y, c, ow, oh, alpha=a))


@pytest.mark.gpu
@pytest.mark.parametrize("count", [2, 5, 40])
def test_gpu_scaled_batch(gh, oracle, count):
    """bt709hip_decode_scaled_batch: `count` same-geometry frames into same-sized views, one launch
    (pointer table up to 32 frames, evenly spaced ring beyond)."""
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = gh.context()
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    (w, h), (ow, oh) = (96, 40), (61, 27)
    in_pitch, out_pitch = w * h * 3 // 2, ow * oh * 4
    slab_in, slab_out = DeviceBuffer(ctx, count * in_pitch), DeviceBuffer(ctx, count * out_pitch)
    frames = [_frame(w, h, 40 + i) for i in range(count)]
    bufs, texs = [], []
    for i, (y, c) in enumerate(frames):
        base = slab_in.ptr + i * in_pitch
        b = mb.CVPixelBuffer(ctx, w, h, w, w, planes=(base, base + w * h))
        mb.BGRAToBT709Converter.setBT709Attributes(b)
        b.upload_planes(y, c)
        bufs.append(b)
        texs.append(mb.BGRATexture(ctx, ow, oh, ow * 4, ptr=slab_out.ptr + i * out_pitch))
    assert dec.decodeBT709ScaledBatch(bufs, texs, ctx.commandQueue.commandBuffer(), True), dec.lastStatus
    assert ctx.lib.bt709hip_last_kernel_name() == b"decode_nv12_scaled"
    for (y, c), t in zip(frames, texs):
        got = ctx.getBGRATexturePixels(t).view(np.uint8).reshape(oh, ow * 4)
        assert np.array_equal(got, oracle.decode_nv12_scaled(0, y, c, ow, oh))
    if count > _capi.MAX_BATCH:  # not evenly spaced any more: the pointer-table limit applies
        bufs[1], bufs[2] = bufs[2], bufs[1]
        assert not dec.decodeBT709ScaledBatch(bufs, texs, None, True) and dec.lastStatus == _capi.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_gpu_half_alpha_in_the_persistent_kernel(gh, oracle):
    """The persistent 2:1 kernel computes the alpha channel WITHOUT tables (decoded alpha byte =
    trunc(255 x + 0.5), byteNorm, sum * 63.75, trunc(. + 0.5)): every alpha byte as a constant 2x2 block, every
    byte against every other in one block, and random planes -- equal to the oracle and to the per-tile kernel
    (which goes through the byteNorm / quantiser tables)."""
    w, h = 1024, 64
    y, c = _frame(w, h, 4242)
    a = np.random.default_rng(77).integers(0, 256, (h, w), dtype=np.uint8)
    codes = np.arange(256, dtype=np.uint8)
    a[0:2, 0:512] = np.repeat(codes, 2)[None, :]            # 256 constant blocks
    a[2, 0:512:2], a[2, 1:512:2] = codes, codes[::-1]         # mixed blocks: (b, 255 - b) over (b, b)
    a[3, 0:512] = np.repeat(codes, 2)
    a[4:6, 512:1024] = np.repeat(np.roll(codes, 1), 2)[None, :] ^ np.tile(np.array([0, 1], np.uint8), 256)[None, :]
    want = oracle.decode_nv12_half(mb.MetalBT709GammaSRGB, y, c, alpha=a)
    got = {}
    for kernel in (1, 0):
        dec = gh.make_decoder(mb.MetalBT709GammaSRGB, has_alpha=True, options={_capi.OPT_HALF_KERNEL: kernel, _capi.OPT_HALF_WORKGROUPS: 5})
        got[kernel] = gh.gpu_decode_half(y, c, mb.MetalBT709GammaSRGB, decoder=dec, alpha=a)
        name = gh.context().lib.bt709hip_last_kernel_name()
        assert name == (b"decode_nv12_half_rep<alpha>" if kernel else b"decode_nv12_half<wide,alpha>"), name
        assert np.array_equal(got[kernel], want), kernel
    assert np.array_equal(got[0], got[1])


@pytest.mark.gpu
def test_gpu_scaled_strips_with_a_ragged_last_wave(gh, oracle):
    """The vertical taps of a strip are worked out by its first lanes (lane i: row i) and read with
    v_readlane_b32: an output width that leaves the last wave with FEWER live columns than a strip has rows
    must not change that.  8 frames of 64x600 -> 65x600 / 130x300: several rows per strip, one live column in
    the last wave; pass 2 alone on the same shapes."""
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = gh.context()
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    scale = mb.MetalScaleRenderContext()
    assert scale.setupRenderPipelines(ctx)
    for (w, h), (ow, oh), count in (((64, 600), (65, 600), 8), ((64, 600), (129, 1100), 8), ((256, 64), (321, 2500), 1)):
        in_pitch, out_pitch = w * h * 3 // 2, ow * oh * 4
        slab_in, slab_out = DeviceBuffer(ctx, count * in_pitch), DeviceBuffer(ctx, count * out_pitch)
        frames = [_frame(w, h, 900 + i) for i in range(count)]
        bufs, texs = [], []
        for i, (y, c) in enumerate(frames):
            base = slab_in.ptr + i * in_pitch
            b = mb.CVPixelBuffer(ctx, w, h, w, w, planes=(base, base + w * h))
            mb.BGRAToBT709Converter.setBT709Attributes(b)
            b.upload_planes(y, c)
            bufs.append(b)
            texs.append(mb.BGRATexture(ctx, ow, oh, ow * 4, ptr=slab_out.ptr + i * out_pitch))
        assert dec.decodeBT709ScaledBatch(bufs, texs, ctx.commandQueue.commandBuffer(), True), dec.lastStatus
        for (y, c), t in zip(frames, texs):
            got = ctx.getBGRATexturePixels(t).view(np.uint8).reshape(oh, ow * 4)
            assert np.array_equal(got, oracle.decode_nv12_scaled(0, y, c, ow, oh)), (w, h, ow, oh)
        # pass 2 alone from the 8-bit intermediate of frame 0
        y, c = frames[0]
        inter, view = ctx.makeBGRATexture((w, h)), ctx.makeBGRATexture((ow, oh))
        assert dec.decodeBT709(bufs[0], None, inter, None, None, w, h, False)
        assert scale.renderScaled(ctx, view, ow, oh, None, None, inter, True)
        got = ctx.getBGRATexturePixels(view).view(np.uint8).reshape(oh, ow * 4)
        assert np.array_equal(got, oracle.decode_nv12_scaled(0, y, c, ow, oh)), ("pass 2", w, h, ow, oh)


@pytest.mark.gpu
@pytest.mark.parametrize("rep", ["0", "1"])
def test_fuzzed_rescale_geometry(gh, oracle, rep):
    """Seeded fuzz over the rescale entry points: any 4-multiple source size, any plane pitch and
    byte alignment, any output pitch; exact 2:1 through the per-tile kernel (rep=0) or the persistent
    one with a random workgroup count (rep=1), and an arbitrary output size through the bilinear
    kernel.  Bytes must equal the oracle's and nothing outside the output rows may be written."""
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = gh.context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(709 + int(rep))
    for case in range(40):
        w = 4 * int(rng.integers(1, 120))
        hgt = 4 * int(rng.integers(1, 12))
        gamma = int(rng.integers(0, 4))
        aligned = bool(rng.integers(0, 2))
        ys = w + (int(rng.integers(0, 5)) * 4 if aligned else int(rng.integers(0, 37)))
        cs = w + (int(rng.integers(0, 5)) * 4 if aligned else int(rng.integers(0, 37)))
        oy, oc = (0, 0) if aligned else (int(rng.integers(0, 16)) for _ in range(2))
        exact = bool(rng.integers(0, 2))
        ow, oh = (w // 2, hgt // 2) if exact else (int(rng.integers(1, 2 * w)), int(rng.integers(1, 3 * hgt)))
        os_ = 4 * ow + (int(rng.integers(0, 3)) * 8 if aligned else 4 * int(rng.integers(0, 9)))
        oo = 0 if aligned else 4 * int(rng.integers(0, 4))
        use_alpha = bool(rng.integers(0, 4) == 0)
        dec = gh.make_decoder(gamma, has_alpha=use_alpha, options={_capi.OPT_HALF_KERNEL: int(rep),
                                                                  _capi.OPT_HALF_WORKGROUPS: int(rng.integers(1, 300))})
        gamma = dec.gamma  # an alpha decoder runs the sRGB mode
        y, c = _frame(w, hgt, 2000 + case)
        a = rng.integers(0, 256, (hgt, w), dtype=np.uint8) if use_alpha else None

        def plane(arr, pitch, off):
            buf = DeviceBuffer(ctx, pitch * arr.shape[0] + off + 64)
            ctx._upload(buf.ptr + off, pitch, np.ascontiguousarray(arr), None)
            return buf, buf.ptr + off

        by, py = plane(y, ys, oy)
        bc, pc = plane(c, cs, oc)
        src = mb.CVPixelBuffer(ctx, w, hgt, ys, cs, planes=(py, pc))
        src.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
        src.setAttachment("TransferFunction", gh.TRANSFER_FOR_GAMMA[dec.gamma])
        abuf = None
        if use_alpha:
            ba, pa = plane(a, ys, int(rng.integers(0, 16)) if not aligned else 0)
            abuf = mb.CVPixelBuffer(ctx, w, hgt, ys, cs, planes=(pa, pc))
            abuf.setAttachment("TransferFunction", mb.kCVImageBufferTransferFunction_Linear)
        out_bytes = os_ * oh + oo + 64
        bo = DeviceBuffer(ctx, out_bytes)
        _capi.check(lib.bt709hip_memset(h, bo.ptr, 0x5A, out_bytes, None))
        ctx._sync(None)
        tex = mb.BGRATexture(ctx, ow, oh, os_, ptr=bo.ptr + oo)
        assert dec.decodeBT709Scaled(src, tex, None, True, alphaPixelBuffer=abuf), (case, dec.lastStatus)
        raw = np.empty(out_bytes, np.uint8)
        _capi.check(lib.bt709hip_download(h, raw.ctypes.data, out_bytes, bo.ptr, out_bytes, out_bytes, 1, None))
        ctx._sync(None)
        rows = raw[oo:oo + os_ * oh].reshape(oh, os_)
        want = (oracle.decode_nv12_half(gamma, y, c, alpha=a) if exact
                else oracle.decode_nv12_scaled(gamma, y, c, ow, oh, alpha=a))
        info = (case, w, hgt, ow, oh, gamma, use_alpha, exact, ys, cs, os_, oy, oc, oo, lib.bt709hip_last_kernel_name())
        assert np.array_equal(rows[:, :4 * ow], want), info
        assert (rows[:, 4 * ow:] == 0x5A).all() and (raw[:oo] == 0x5A).all() and (raw[oo + os_ * oh:] == 0x5A).all(), info


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", [0, 2])
@pytest.mark.parametrize("shape", [((640, 64), (1280, 128)), ((100, 40), (333, 77)), ((1900, 32), (2000, 36)), ((1920, 32), (2021, 40)),
                                   ((322, 18), (1287, 31)), ((64, 16), (4096, 16)), ((480, 270), (960, 540))])
def test_gpu_enlarging_wave_decodes_each_source_pixel_once(gh, oracle, gamma, shape):
    """Round 6: when the view is wider than the frame (AAPLRenderer.m:891-977, a 1080p clip in a larger view) the 64 lanes of a
    wave decode 64 consecutive SOURCE columns once and take their two taps from each other's registers (ds_bpermute) instead of
    each lane decoding both of its taps.  Shapes: exact 2x, an odd ratio with a ragged last wave, scale_x = 0.95 (the widest
    span the form accepts: 61 of its 64 columns) and just above it (per-lane taps again), a wave whose taps all sit on a
    handful of columns (64x), the right-edge clamp."""
    (w, h), (ow, oh) = shape
    y, c = _frame(w, h, w + h + ow + gamma)
    got = gpu_scaled(gh, y, c, ow, oh, gamma)
    assert np.array_equal(got, oracle.decode_nv12_scaled(gamma, y, c, ow, oh))


@pytest.mark.gpu
def test_gpu_enlarging_with_alpha_and_odd_luma_stride(gh, oracle):
    """The same form with an alpha plane (a fourth value travels between the lanes) and with a luma plane at an odd pitch and
    address (the form only needs the CbCr plane 2-byte aligned)."""
    ctx = gh.context()
    (w, h), (ow, oh) = (200, 24), (517, 50)
    y, c = _frame(w, h, 61)
    a = np.random.default_rng(62).integers(0, 256, (h, w), dtype=np.uint8)
    got = gpu_scaled(gh, y, c, ow, oh, mb.MetalBT709GammaSRGB, alpha=a)
    assert np.array_equal(got, oracle.decode_nv12_scaled(mb.MetalBT709GammaSRGB, y, c, ow, oh, alpha=a))
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    buf = gh.make_buffer(y, c, dec.gamma, y_stride=203, cbcr_stride=202)
    tex = ctx.makeBGRATexture((ow, oh))
    assert dec.decodeBT709Scaled(buf, tex, ctx.commandQueue.commandBuffer(), True), dec.lastStatus
    got = ctx.getBGRATexturePixels(tex).view(np.uint8).reshape(oh, ow * 4)
    assert np.array_equal(got, oracle.decode_nv12_scaled(0, y, c, ow, oh))


# ------------------------------------------------------------------ the launch regimes the rescale ships in
#
# launch_decode_scaled picks, per launch, a tap form, a strip length, a persistent item loop or one workgroup per item and --
# when cols x out_height x frames <= resident x max_rows -- the one-generation ("balanced") cut instead of the 8-workgroups-per-CU
# rule.  Every shape above this line is small enough for the balanced cut with strips of a few rows and at most one item per
# workgroup; the shapes the README quotes are not.  The cases below are narrow and tall (one 256-lane column of workgroups:
# cheap for the oracle) with out_height x frames past resident x max_rows for ANY occupancy up to 8 workgroups per CU, so they
# run under the rule at the longest strips, and the plan is asserted from bt709hip_last_scaled_launch_info, not from a copy of
# the launcher's arithmetic.  ONE table: the GPU tests run it, test_regime_cases_can_reach_their_regime (CPU) guards it.

RULE_WG_PER_CU = 8   # the launcher's rule, and the most workgroups of 256 lanes a CU holds
RULE_CUS = 256       # MI355X; a partitioned card reports fewer and _regime_frames sizes the batch from that
MAX_ROWS = {"bytes": 16, "pairs": 16, "wide": 16, "shared": 32, "once": 32}
TAPS_NAME = {_capi.SCALED_TAPS_BYTES: "bytes", _capi.SCALED_TAPS_PAIRS: "pairs", _capi.SCALED_TAPS_WIDE: "wide",
             _capi.SCALED_TAPS_SHARED: "shared", _capi.SCALED_TAPS_ONCE: "once"}
PERSISTENT = {"bytes": 1, "pairs": 1, "wide": 1, "shared": 0, "once": 0}


def _case(name, src, dst, frames, taps, layout="aligned", spacing="ring", gamma=0, alpha=False, two_items=False, grid_y=None):
    """layout: how the planes of a frame lie ("aligned": pointers and pitches multiples of 4 -- "even": tight at the frame's own
    width -- "odd": odd pitches and odd plane addresses -- "ring2": aligned planes in slots whose pitch is 2 mod 4);
    spacing: "ring" = evenly spaced slots (the launch steps from frame 0), "table" = uneven (the 32-entry pointer table).
    taps: the form(s) the record may name; two_items: the record must show items >= 2 x grid[0]."""
    return dict(name=name, src=src, dst=dst, frames=frames, taps=taps if isinstance(taps, tuple) else (taps,), layout=layout,
                spacing=spacing, gamma=gamma, alpha=alpha, two_items=two_items, grid_y=grid_y)


ONCE_RULE = dict(src=(128, 1100), dst=(256, 2203), frames=32, taps="once", spacing="table", grid_y=69)  # last strip: 27 rows, a partial trip
WIDE_RULE = dict(src=(384, 3300), dst=(256, 2200), frames=32, taps="wide", spacing="table", two_items=True)
REGIME_CASES = [
    _case("once-rule", **ONCE_RULE),
    _case("shared-rule", (384, 1100), (256, 2203), 32, "shared"),
    _case("wide-rule", **WIDE_RULE),
    _case("pairs-rule", (386, 3300), (256, 2200), 32, "pairs", layout="even", two_items=True),
    _case("bytes-rule", (386, 3300), (256, 2200), 32, "bytes", layout="odd", spacing="table"),
    # an evenly spaced ring past the pointer table.  51 strips of 16 rows a frame: 48 frames are 2 448 items, fewer than two for
    # each of the 2 560 = 2 x 5 x 256 workgroups a 256-CU device holds at 5 per CU, so the batch is sized for two items at ANY
    # occupancy up to 8 per CU: 51 x 81 >= 2 x 8 x 256
    _case("decimate-rule", (512, 4320), (200, 811), 81, ("bytes", "pairs", "wide"), two_items=True),
    _case("once-rule-alpha", alpha=True, gamma=mb.MetalBT709GammaSRGB, **ONCE_RULE),
    _case("wide-rule-alpha", alpha=True, gamma=mb.MetalBT709GammaSRGB, **WIDE_RULE),
] + [_case("once-rule-gamma%d" % g, gamma=g, **ONCE_RULE) for g in (1, 2, 3)] + [
    _case("wide-rule-gamma%d" % g, gamma=g, **WIDE_RULE) for g in (1, 2, 3)] + [
    _case("ring-spacing", (384, 3300), (256, 2200), 40, "pairs", layout="ring2", two_items=True),
]


def _ceil_div(a, b):
    return -(-a // b)


def _regime_frames(case, cus):
    """Frames of the batch on a device of `cus` compute units: the case's own count wherever that reaches the regime (any device
    up to RULE_CUS units), more on a larger one -- out_height x frames > 8 x CUs x max_rows, and two items per workgroup where
    the case says so."""
    cols, oh = _ceil_div(case["dst"][0], 256), case["dst"][1]
    max_rows = max(MAX_ROWS[t] for t in case["taps"])
    n = max(case["frames"], RULE_WG_PER_CU * cus * max_rows // (cols * oh) + 1)
    if case["two_items"]:
        n = max(n, _ceil_div(2 * RULE_WG_PER_CU * cus, cols * _ceil_div(oh, min(MAX_ROWS[t] for t in case["taps"]))))
    return n


def test_regime_cases_can_reach_their_regime():
    """A guard on the table, not a second launcher: plain inequalities on each case's own numbers, against the conditions the
    kernel file's header documents for each form, on a 256-CU device at any occupancy up to 8 workgroups per CU."""
    assert len({c["name"] for c in REGIME_CASES}) == len(REGIME_CASES)
    for name in ("once-rule", "shared-rule", "wide-rule", "pairs-rule", "bytes-rule", "decimate-rule", "once-rule-alpha",
                 "wide-rule-alpha", "ring-spacing"):
        assert any(c["name"] == name for c in REGIME_CASES), name
    for base in ("once-rule", "wide-rule"):  # all four gamma modes: the base case is mode 0
        assert sorted(c["gamma"] for c in REGIME_CASES if c["name"] == base or c["name"].startswith(base + "-gamma")) == [0, 1, 2, 3]
    for c in REGIME_CASES:
        (w, h), (ow, oh), n = c["src"], c["dst"], c["frames"]
        assert _regime_frames(c, RULE_CUS) == n, c["name"]  # the table's own count is enough on the device it is written for
        cols = _ceil_div(ow, 256)
        sx, sy = w / ow, h / oh
        assert w % 2 == 0 and h % 2 == 0 and oh <= 65535
        for taps in c["taps"]:
            max_rows = MAX_ROWS[taps]
            # past the one-generation cut whatever the occupancy (and so the rule asks for the longest strip)
            assert cols * oh * n > RULE_WG_PER_CU * RULE_CUS * max_rows, c["name"]
            strips = _ceil_div(oh, max_rows)
            if c["two_items"]:
                assert PERSISTENT[taps] and cols * strips * n >= 2 * RULE_WG_PER_CU * RULE_CUS, c["name"]
            if c["grid_y"] is not None:
                assert strips == c["grid_y"] and oh % max_rows and (oh % max_rows) % 4, c["name"]  # a last strip that is a partial trip
        layout_align = {"aligned": 4, "even": 2 if w % 4 else 4, "odd": 1, "ring2": 2}[c["layout"]]
        if c["taps"] == ("once",):      # CbCr plane 2-byte aligned, enlarging: scale_x <= 0.95, scale_y < 1
            assert layout_align >= 2 and sx <= 0.95 and sy < 1.0
        elif c["taps"] == ("shared",):  # layout as wide, scale_y < 1, a wave's 64 windows within one 256-byte span, not `once`
            assert layout_align == 4 and w % 4 == 0 and w >= 8 and sy < 1.0 and 64 * sx + 12 <= 252 and sx > 0.95
        elif c["taps"] == ("wide",):    # planes and strides 4-byte aligned, width % 4 == 0, width >= 8; not enlarging vertically
            assert layout_align == 4 and w % 4 == 0 and w >= 8 and sy >= 1.0
        elif c["taps"] == ("pairs",):   # CbCr plane 2-byte aligned and no more
            assert layout_align == 2 and sy >= 1.0
        elif c["taps"] == ("bytes",):
            assert layout_align == 1 and sy >= 1.0
        else:                           # any per-lane form
            assert set(c["taps"]) == {"bytes", "pairs", "wide"} and sy >= 1.0
        if c["spacing"] == "table":
            assert n <= _capi.MAX_BATCH, c["name"]
        if c["name"] in ("decimate-rule", "ring-spacing"):
            assert n > _capi.MAX_BATCH and c["spacing"] == "ring"
        if c["alpha"]:
            assert c["gamma"] == mb.MetalBT709GammaSRGB  # an alpha decoder runs the sRGB mode


def _expected_frames(fn, jobs):
    """[fn(*job) for job in jobs] on at most 16 threads (the oracle is called through ctypes, which releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    if len(jobs) < 2:
        return [fn(*job) for job in jobs]
    with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as pool:
        return list(pool.map(lambda job: fn(*job), jobs))


def _scaled_record(ctx):
    import ctypes as C
    info = _capi.ScaledLaunchInfo()
    _capi.check(ctx.lib.bt709hip_last_scaled_launch_info(C.byref(info)))
    return dict(grid=tuple(info.grid), block=tuple(info.block), taps=TAPS_NAME.get(info.taps, info.taps), taps_id=info.taps,
                rows=info.rows, persistent=info.persistent, balanced=info.balanced, resident=info.resident, items=info.items)


def _round_up(v, a):
    return (v + a - 1) // a * a


class _Slab:
    """`count` slots in one device allocation, pre-filled with 0x5A: slot i starts at base + offsets[i]."""

    def __init__(self, ctx, count, slot_bytes, pitch, spacing):
        from metalbt709decoder_amd.decoder import DeviceBuffer
        # "table": a gap after every third slot, so that no single step reaches every frame (multiples of 256: alignment stays)
        self.offsets = [i * pitch + (256 * (i // 3) if spacing == "table" else 0) for i in range(count)]
        self.nbytes = self.offsets[-1] + slot_bytes + 64
        self.ctx, self.buf = ctx, DeviceBuffer(ctx, self.nbytes)
        _capi.check(ctx.lib.bt709hip_memset(ctx.handle, self.buf.ptr, 0x5A, self.nbytes, None))
        ctx._sync(None)

    def ptr(self, i):
        return self.buf.ptr + self.offsets[i]

    def download(self):
        raw = np.empty(self.nbytes, np.uint8)
        _capi.check(self.ctx.lib.bt709hip_download(self.ctx.handle, raw.ctypes.data, self.nbytes, self.buf.ptr, self.nbytes, self.nbytes, 1, None))
        self.ctx._sync(None)
        return raw


def _check_views(case_name, raw, slab, views, ow, oh, stride, want, plan):
    """Every byte of every view against the oracle's, everything else in the slab still 0x5A; the message of a mismatch names
    the case, the frame, the first differing row / column / channel and the plan."""
    untouched = np.ones(raw.size, bool)
    for i in range(views):
        o = slab.offsets[i]
        rows = raw[o:o + stride * oh].reshape(oh, stride)
        got = rows[:, :4 * ow]
        if not np.array_equal(got, want[i]):
            r, b = np.argwhere(got != want[i])[0]
            bad_rows = np.flatnonzero((got != want[i]).any(axis=1))
            raise AssertionError("%s: frame %d differs from the oracle first at row %d, column %d, channel %d (got %d, want %d); %d rows "
                                 "differ, from %d to %d; plan %r" % (case_name, i, r, b // 4, b % 4, got[r, b], want[i][r, b],
                                                                      bad_rows.size, bad_rows[0], bad_rows[-1], plan))
        untouched[o:o + stride * oh].reshape(oh, stride)[:, :4 * ow] = False
    stray = np.flatnonzero(untouched & (raw != 0x5A))
    assert stray.size == 0, "%s: %d bytes written outside the views, first at slab offset %d; plan %r" % (case_name, stray.size, stray[0], plan)


def _run_decode_scaled(gh, oracle, name, src, dst, frames, layout, spacing, gamma, alpha, seed, out_pad=16, known=None):
    """`frames` seeded frames through decodeBT709ScaledBatch in ONE launch; returns (plan, check) where check() compares every
    byte with the oracle.  The plan is read before the comparison so that a mismatch can name it.  known: {seed: expected
    view} of frames an earlier run of the same geometry already asked the oracle for (filled here)."""
    ctx = gh.context()
    (w, h), (ow, oh) = src, dst
    dec = gh.make_decoder(gamma, has_alpha=alpha)
    gamma = dec.gamma
    # a frame's slot: Y plane, CbCr plane, alpha plane
    if layout == "odd":
        ys, cs, y_off = w + 1, w + 3, 1
        c_off = (y_off + ys * h) | 1
        a_off = (c_off + cs * (h // 2) + 2) | 1
        in_pitch = _round_up(a_off + ys * h, 256)
    else:
        ys = cs = w if layout in ("even", "ring2") else _round_up(w, 4)
        y_off, c_off = 0, ys * h if layout == "even" else _round_up(ys * h, 256)
        a_off = c_off + cs * (h // 2) if layout == "even" else _round_up(c_off + cs * (h // 2), 256)
        in_pitch = _round_up(a_off + ys * h, 256) + (2 if layout == "ring2" else 0)
    stride = 4 * ow + out_pad
    out_pitch = _round_up(stride * oh, 256)
    slab_in = _Slab(ctx, frames, in_pitch, in_pitch, spacing)
    slab_out = _Slab(ctx, frames, stride * oh, out_pitch, spacing)
    planes, bufs, abufs, texs = [], [], [], []
    for i in range(frames):
        y, c = _frame(w, h, seed + i)
        a = np.random.default_rng(seed + 5000 + i).integers(0, 256, (h, w), dtype=np.uint8) if alpha else None
        base = slab_in.ptr(i)
        ctx._upload(base + y_off, ys, y, None, wait=False)
        ctx._upload(base + c_off, cs, c, None, wait=False)
        b = mb.CVPixelBuffer(ctx, w, h, ys, cs, planes=(base + y_off, base + c_off))
        b.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
        b.setAttachment("TransferFunction", gh.TRANSFER_FOR_GAMMA[gamma])
        bufs.append(b)
        if alpha:
            ctx._upload(base + a_off, ys, a, None, wait=False)
            ab = mb.CVPixelBuffer(ctx, w, h, ys, cs, planes=(base + a_off, base + c_off))
            ab.setAttachment("TransferFunction", mb.kCVImageBufferTransferFunction_Linear)
            abufs.append(ab)
        ctx._sync(None)
        planes.append((gamma, y, c, ow, oh, 0xFF, a))
        texs.append(mb.BGRATexture(ctx, ow, oh, stride, ptr=slab_out.ptr(i)))
    assert dec.decodeBT709ScaledBatch(bufs, texs, ctx.commandQueue.commandBuffer(), True, alphaPixelBuffers=abufs or None), (name, dec.lastStatus)
    assert ctx.lib.bt709hip_last_kernel_name() == (b"decode_nv12_scaled<alpha>" if alpha else b"decode_nv12_scaled")
    plan = _scaled_record(ctx)
    print("PLAN %s: %dx%d -> %dx%d x %d: %r" % (name, w, h, ow, oh, frames, plan))

    def check():
        memo = {} if known is None else known
        todo = [i for i in range(frames) if seed + i not in memo]
        for i, view in zip(todo, _expected_frames(oracle.decode_nv12_scaled, [planes[i] for i in todo])):
            memo[seed + i] = view
        want = [memo[seed + i] for i in range(frames)]
        _check_views(name, slab_out.download(), slab_out, frames, ow, oh, stride, want, plan)
    return plan, check


def _assert_plan_shape(name, plan, cols, oh, frames):
    """What any record must satisfy whatever the regime: the grid and the items follow from rows / persistent as documented."""
    strips = _ceil_div(oh, plan["rows"])
    assert plan["items"] == cols * strips * frames, (name, plan)
    if plan["persistent"]:
        assert plan["grid"] == (min(plan["items"], plan["resident"]), 1, 1), (name, plan)
    else:
        assert plan["grid"] == (cols, strips, frames), (name, plan)
    assert plan["block"] == (256, 1, 1), (name, plan)
    if plan["balanced"]:
        assert plan["items"] <= plan["resident"], (name, plan)


@pytest.mark.gpu
@pytest.mark.parametrize("case", REGIME_CASES, ids=[c["name"] for c in REGIME_CASES])
def test_gpu_scaled_in_the_rule_regime(gh, oracle, case):
    """decode_nv12_scaled where the README's numbers are taken: under the 8-per-CU rule at the longest strips (32 rows for the
    by-wave forms, 16 for the per-lane ones), persistent workgroups walking two and more items, a last strip that is a partial
    trip, the pointer table and a ring past it, every tap form, alpha, all four gammas.  Bit for bit against the oracle, every
    frame, nothing written outside the views -- and the plan asserted from the launcher's own record: a case that lands in
    another regime than the one it names FAILS."""
    cus = gh.context().info().compute_units
    frames = _regime_frames(case, cus)
    name, (ow, oh) = case["name"], case["dst"]
    plan, check = _run_decode_scaled(gh, oracle, name, case["src"], case["dst"], frames, case["layout"], case["spacing"], case["gamma"],
                                     case["alpha"], seed=7000 + 100 * REGIME_CASES.index(case))
    assert plan["taps"] in case["taps"], (name, plan)
    assert plan["rows"] == MAX_ROWS[plan["taps"]] and plan["balanced"] == 0, (name, plan)
    assert plan["persistent"] == PERSISTENT[plan["taps"]], (name, plan)
    assert 1 <= plan["resident"] <= RULE_WG_PER_CU * cus, (name, plan)
    _assert_plan_shape(name, plan, _ceil_div(ow, 256), oh, frames)
    if case["two_items"]:
        assert plan["items"] >= 2 * plan["grid"][0], (name, plan)
    if case["grid_y"] is not None and frames == case["frames"]:
        assert plan["grid"][1] == case["grid_y"], (name, plan)
    check()


# the shapes bench_scaled / the README quote, laid out as they are timed: tight pitches, slots of a ring rounded to 256 bytes
BENCH_SHAPES = [("1080p-4k", (1920, 1080), (3840, 2160), "once", 32, 0), ("4k-1440p", (3840, 2160), (2560, 1440), "wide", 16, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BENCH_SHAPES, ids=[s[0] for s in BENCH_SHAPES])
def test_gpu_scaled_in_the_shapes_the_readme_quotes(gh, oracle, shape):
    """1080p -> 4K x 8 and 4K -> 1440p x 8 in the exact shape that is timed (record: `once`, 32 rows, rule; `wide`, 16 rows, rule,
    persistent), then ONE frame of each (the reference's cadence): rule or balanced by the device's occupancy, a strip of at
    least 7 rows either way, and what the record implies -- balanced => every workgroup has at most one item."""
    name, src, dst, taps, rows, persistent = shape
    cols, known = _ceil_div(dst[0], 256), {}
    plan, check = _run_decode_scaled(gh, oracle, name + "-x8", src, dst, 8, "aligned", "ring", 0, False, seed=8100, out_pad=0, known=known)
    assert (plan["taps"], plan["rows"], plan["balanced"], plan["persistent"]) == (taps, rows, 0, persistent), plan
    _assert_plan_shape(name, plan, cols, dst[1], 8)
    check()
    plan, check = _run_decode_scaled(gh, oracle, name + "-x1", src, dst, 1, "aligned", "ring", 0, False, seed=8100, out_pad=0, known=known)
    assert plan["taps"] == taps and plan["persistent"] == persistent and plan["balanced"] in (0, 1) and plan["rows"] >= 7, plan
    _assert_plan_shape(name, plan, cols, dst[1], 1)
    check()


def _random_intermediate(fmt, w, h, seed):
    """An intermediate as pass 1 leaves it: random BGRA8 bytes, or random linear halves in [0, 1] with exact zeros and ones."""
    rng = np.random.default_rng(seed)
    if fmt != mb.MTLPixelFormatRGBA16Float:
        return rng.integers(0, 256, (h, w * 4), dtype=np.uint8)
    v = rng.random((h, w, 4), dtype=np.float32)
    v[rng.random((h, w, 4), dtype=np.float32) < 0.02] = 0.0
    v[rng.random((h, w, 4), dtype=np.float32) < 0.02] = 1.0
    return v.astype(np.float16)


RENDER_CASES = [("wide-shape-bgra8", mb.MTLPixelFormatBGRA8Unorm_sRGB, (384, 3300), (256, 2200), 32),
                ("wide-shape-rgba16f", mb.MTLPixelFormatRGBA16Float, (384, 3300), (256, 2200), 32),
                ("once-shape-bgra8", mb.MTLPixelFormatBGRA8Unorm_sRGB, (128, 1100), (256, 2203), 32),
                ("once-shape-rgba16f", mb.MTLPixelFormatRGBA16Float, (128, 1100), (256, 2203), 32),
                ("4k-1440p-x16-bgra8", mb.MTLPixelFormatBGRA8Unorm_sRGB, (3840, 2160), (2560, 1440), 16)]


def _run_render_scaled(gh, oracle, name, fmt, src, dst, n, seed, out_pad=16):
    """`n` intermediates of format `fmt`, evenly spaced, through renderScaledBatch in ONE launch; every byte against the oracle,
    nothing written outside the views.  Returns the plan (rows = cols x out_height x n / (8 x CUs), capped at 16)."""
    (w, h), (ow, oh) = src, dst
    ctx = gh.context()
    bpp = 8 if fmt == mb.MTLPixelFormatRGBA16Float else 4
    in_stride, stride = w * bpp, ow * 4 + out_pad
    in_pitch, out_pitch = _round_up(in_stride * h, 256), _round_up(stride * oh, 256)
    slab_in, slab_out = _Slab(ctx, n, in_stride * h, in_pitch, "ring"), _Slab(ctx, n, stride * oh, out_pitch, "ring")
    inters, views, jobs = [], [], []
    for i in range(n):
        inter = _random_intermediate(fmt, w, h, seed + i)
        t = mb.BGRATexture(ctx, w, h, in_stride, ptr=slab_in.ptr(i), pixelFormat=fmt)
        ctx.fillBGRATexture(t, inter)
        inters.append(t)
        views.append(mb.BGRATexture(ctx, ow, oh, stride, ptr=slab_out.ptr(i)))
        jobs.append((inter, ow, oh))
    scale = mb.MetalScaleRenderContext()
    assert scale.setupRenderPipelines(ctx)
    assert scale.renderScaledBatch(ctx, views, None, inters, True), scale.lastStatus
    assert ctx.lib.bt709hip_last_kernel_name() == (b"render_scaled<rgba16f>" if bpp == 8 else b"render_scaled<bgra8>")
    plan = dict(_scaled_record(ctx), taps=None)  # pass 2 has no tap forms: taps_id is 0
    print("PLAN render-%s: %dx%d -> %dx%d x %d: %r" % (name, w, h, ow, oh, n, plan))
    want = _expected_frames(oracle.render_scaled, jobs)
    _check_views("render-" + name, slab_out.download(), slab_out, n, ow, oh, stride, want, plan)
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("case", RENDER_CASES, ids=[c[0] for c in RENDER_CASES])
def test_gpu_render_scaled_at_16_row_strips(gh, oracle, case):
    """Pass 2 alone at the strip length it is benched at (every other shape of the suite gives it 1-4 rows): a ring of BGRA8 /
    RGBA16Float intermediates through bt709hip_render_scaled_batch in one launch, and 4K -> 1440p x 16 as benched; record:
    rows 16."""
    name, fmt, src, (ow, oh), n = case
    cols = _ceil_div(ow, 256)
    n = max(n, _ceil_div(16 * RULE_WG_PER_CU * gh.context().info().compute_units, cols * oh))  # enough for 16 rows on any device
    plan = _run_render_scaled(gh, oracle, name, fmt, src, (ow, oh), n, seed=9000, out_pad=0 if name.startswith("4k") else 16)
    assert (plan["rows"], plan["taps_id"], plan["persistent"], plan["balanced"], plan["resident"]) == (16, 0, 0, 0, 0), plan
    assert plan["grid"] == (cols, _ceil_div(oh, 16), n) and plan["items"] == cols * _ceil_div(oh, 16) * n, plan
