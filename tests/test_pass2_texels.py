"""Pass 2 alone from an RGBA16Float surface the CALLER filled (bt709hip_render_scaled[_batch], render_scaled<rgba16f>): every
other test of that kernel feeds it what pass 1 leaves, halves in [0, 1].  Here

  1. every one of the 65 536 half codes in every channel -- negatives, values above 1.0, infinities, all 2 046 NaNs -- as flat
     2x2 blocks at exactly 2:1: the extraction of the four halves from the two loaded dwords, the saturate outside [0, 1]
     (a NaN sum is 0: oracle/bt709_oracle.h), the encode of a clamped argument;
  2. four-tap sums of halves on and one float below each of the 255 encode thresholds, every tap order, both column parities;
  3. random texels of any finite code, and the same with infinities and NaNs among them, at weights that are not 1/4 -- reducing,
     enlarging and 1:1 (where three weights are exactly 0 and 0 * inf is a NaN) -- through padded pitches, alone and in a batch;
  4. every byte value in every channel of the BGRA8 form (lin[256] through the three byte selects).

Every expected byte is the oracle's (half_texel_cases.py builds the images).  The unmarked tests guard the oracle and the
builders on the CPU."""
import numpy as np
import pytest

import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi

import half_texel_cases as hc
import rescale_arith_cases as rc
from oracle_lib import GAMMA_LINEAR

# what the greedy split reached against this oracle when these tests were specified
HALF_EDGE_HITS = (178, 179)  # thresholds hit exactly, hit one float below

_memo = {}


def _every_code(oracle, transposed):
    """-> (image, block codes, the oracle's 256 x 256 output), computed once per arrangement."""
    if ("codes", transposed) not in _memo:
        img, codes = hc.every_code_image(transposed)
        _memo["codes", transposed] = (img, codes, oracle.render_scaled(img, 256, 256))
    return _memo["codes", transposed]


def _unit_maps(oracle):
    """tests/test_scaled_f16_gpu.py _code_to_byte: the byte of a flat block of code k, k in [0, 0x3c00] -> (colour, alpha)."""
    if "unit" not in _memo:
        from test_scaled_f16_gpu import _code_to_byte
        _memo["unit"] = _code_to_byte(oracle)
    return _memo["unit"]


def _closed_form(oracle):
    """(65 536, 4) bytes [code, channel R G B A] from the definition alone (hc.closed_form_by_code)."""
    colour, alpha = _unit_maps(oracle)
    return np.stack([hc.closed_form_by_code(colour)] * 3 + [hc.closed_form_by_code(alpha)], axis=1)


def _edge_frame(oracle):
    if "edges" not in _memo:
        ef, img = hc.half_edge_frame(oracle.thresholds(GAMMA_LINEAR))
        _memo["edges"] = (ef, img, oracle.render_scaled(img, ef.COLS, ef.rows))
    return _memo["edges"]


# reducing, enlarging, 1:1 (fx = fy = 0: the zero-weight case)
WILD_GEOMETRIES = [("reduce", (96, 40), (61, 23)), ("enlarge", (40, 24), (101, 50)), ("one-to-one", (64, 16), (64, 16))]


def _wild(oracle, name, which):
    """-> (image, the oracle's output) of a wild geometry; which: "finite" / "nonfinite"."""
    _, (w, h), (ow, oh) = next(g for g in WILD_GEOMETRIES if g[0] == name)
    if ("wild", name) not in _memo:
        _memo["wild", name] = dict(zip(("finite", "nonfinite"), hc.wild_image(w, h, seed=5709 + w)))
    if ("wild", name, which) not in _memo:
        img = _memo["wild", name][which]
        _memo["wild", name, which] = (img, oracle.render_scaled(img, ow, oh))
    return _memo["wild", name, which]


# ------------------------------------------------------------------ CPU guards

@pytest.mark.parametrize("transposed", [False, True], ids=["by-rows", "transposed"])
def test_oracle_on_every_half_code(oracle, transposed):
    """Per channel, indexed by the channel's code: zeros of both signs, every negative and -inf give 0; 1.0 and everything above
    it up to +inf give 255; all 2 046 NaNs give 0 (defined, not what a cast of round(NaN) happens to give); the byte does not
    decrease over 0 ... +inf; on [0, 1.0] it is _code_to_byte's map."""
    img, codes, out = _every_code(oracle, transposed)
    assert img.shape == (512, 512, 4) and img.dtype == np.float16 and out.shape == (256, 1024)
    raw = img.view(np.uint16)
    for k in range(4):  # every channel sees every code, no two channels of a texel the same one, blocks flat
        assert np.array_equal(np.sort(codes[:, :, k].reshape(-1)), np.arange(65536))
    assert all((codes[:, :, a] != codes[:, :, b]).all() for a in range(4) for b in range(a))
    assert all(np.array_equal(raw[dy::2, dx::2], codes) for dy in (0, 1) for dx in (0, 1))
    assert codes[1, 2, 0] == (0x0201 if transposed else 0x0102) and codes[0, 0, 3] == 0xc000
    table = hc.by_code(out, codes)
    nan = hc.is_nan_code(np.arange(65536))
    assert nan.sum() == 2046 and (table[nan] == 0).all()
    assert (table[0] == 0).all() and (table[hc.NEG_ZERO] == 0).all()
    assert (table[hc.NEG_ZERO + 1:hc.NEG_INF + 1] == 0).all()
    assert (table[hc.ONE:hc.INF + 1] == 255).all()
    assert (np.diff(table[:hc.INF + 1].astype(np.int32), axis=0) >= 0).all()
    colour, alpha = _unit_maps(oracle)
    for k in range(3):
        assert np.array_equal(table[:hc.ONE + 1, k], colour)
    assert np.array_equal(table[:hc.ONE + 1, 3], alpha)
    assert np.array_equal(table, _closed_form(oracle))  # the same, as the GPU test states it
    assert np.unique(table[:, 0]).size == 256 and np.unique(table[:, 3]).size == 256


def test_half_quadruples_reach_the_thresholds(oracle):
    """Every threshold has an upper and a lower quad; in the canonical order the oracle gives byte k on / above threshold k and
    k - 1 below it; the counts of exact hits do not fall below what the greedy split reached."""
    T = oracle.thresholds(GAMMA_LINEAR)
    e = hc.half_edge_quads(T)
    on, below = hc.half_edge_counts(e)
    print("halves: %d thresholds hit exactly, %d one float below; worst gap above %d ulp, below %d ulp"
          % (on, below, e["up_ulps"].max(), e["lo_ulps"].max()))
    assert e["upper"].shape == (255, 4) and e["lower"].shape == (255, 4)
    assert (e["up_ulps"] >= 0).all() and (e["lo_ulps"] >= 1).all()  # all 255 have both probes, each on its side
    assert on >= HALF_EDGE_HITS[0] and below >= HALF_EDGE_HITS[1]
    # the oracle itself on the canonical order: one 2x2 block per quad, the quad in all of R, G, B and A
    for side, quads in ((1, e["upper"]), (0, e["lower"])):
        img = np.empty((2, 510, 4), np.uint16)
        img[0, 0::2], img[0, 1::2], img[1, 0::2], img[1, 1::2] = (quads[:, t, None].repeat(4, axis=1) for t in range(4))
        out = oracle.render_scaled(hc.as_halves(img), 255, 1).reshape(255, 4)
        for ch in range(3):
            assert np.array_equal(out[:, ch], np.arange(255) + side), (side, ch)
    # the frame: every probe in all 24 orders at both column parities, three thresholds per block
    ef, img, want = _edge_frame(oracle)
    exact, probes = rc.check_probes_against(ef, want)
    assert probes == 3 * 2 * 2 * 255 * 24 and img.shape == (2 * ef.rows, 2 * ef.COLS, 4) and ef.rows % 2 == 0
    meta = ef.meta.reshape(ef.rows, ef.COLS, 3, 4)
    for parity in (0, 1):
        for ch in range(3):
            m = meta[:, parity::2, ch]
            assert np.unique(m[m[..., 0] >= 0][:, [0, 2]], axis=0).shape[0] == 255 * 24
    assert np.unique(want[:, 3::4]).size == 256  # the alpha ramp reaches every byte


def test_an_infinite_texel_under_a_zero_weight(oracle):
    """1:1: every output pixel's four taps have the weights 1, 0, 0, 0 and all four are multiplied, so the left neighbour of an
    infinite texel (its right tap: 0 * inf) is a NaN sum -> 0; the texel itself is inf -> 255; the rest is the byte of 0.5."""
    img, (r, c) = hc.one_infinity_image()
    out = oracle.render_scaled(img, 4, 2).reshape(2, 4, 4)
    half = oracle.render_scaled(hc.as_halves(np.full((2, 4, 4), 0x3800, np.uint16)), 4, 2).reshape(2, 4, 4)
    assert (half[..., :3] == 188).all() and (half[..., 3] == 128).all()
    want = half.copy()
    want[r, c], want[r, c - 1] = 255, 0
    assert np.array_equal(out, want)


def test_wild_images_hold_what_they_claim(oracle):
    for name, (w, h), (ow, oh) in WILD_GEOMETRIES:
        finite, _ = _wild(oracle, name, "finite")
        wild, want = _wild(oracle, name, "nonfinite")
        f, v = finite.view(np.uint16), wild.view(np.uint16)
        assert f.shape == (h, w, 4) and np.isfinite(finite.astype(np.float32)).all()
        assert (f > hc.NEG_ZERO).any() and (f < hc.INF).any()  # both signs
        assert ((f & 0x7fff) < 0x0400).any() and ((f & 0x7fff) > 0x7800).any()  # subnormals, values above 32768
        changed = (f != v).any(axis=2)
        assert 0 < changed.sum() <= 0.03 * w * h and ((v[changed] & 0x7c00) == 0x7c00).all()
        assert (v == hc.INF).any() and (v == hc.NEG_INF).any() and hc.is_nan_code(v).any()
        assert want.shape == (oh, ow * 4)
    bytes_, blocks = hc.every_byte_image()
    assert bytes_.shape == (512, 512) and blocks.shape == (256, 64, 4)
    for k in range(4):  # every byte value in every channel at every one of a wave's 64 lane positions
        assert all(np.unique(blocks[:, c, k]).size == 256 for c in range(64))
    assert oracle.render_scaled(bytes_, 64, 256).shape == (256, 256)


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


F16 = mb.MTLPixelFormatRGBA16Float
CANARY = rc.FILL


def _render(gh, img, ow, oh, in_pad=0, name=b"render_scaled<rgba16f>"):
    """One surface through -renderScaled: into a canary-filled target (test_rescale_arith.Target: padded rows, guard bands, all
    checked on read-back); img: (h, w, 4) float16, or (h, 4 w) uint8 BGRA8 rows."""
    from test_rescale_arith import Target
    ctx = gh.context()
    f16 = img.dtype == np.float16
    h, w = img.shape[0], img.shape[1] if f16 else img.shape[1] // 4
    inter = ctx.makeBGRATexture((w, h), pixels=img, stride=w * (8 if f16 else 4) + in_pad,
                                pixelFormat=F16 if f16 else mb.MTLPixelFormatBGRA8Unorm_sRGB)
    scale = mb.MetalScaleRenderContext()
    assert scale.setupRenderPipelines(ctx)
    target = Target(ctx, ow, oh)
    assert scale.renderScaled(ctx, target.tex, ow, oh, None, None, inter, True), scale.lastStatus
    assert ctx.lib.bt709hip_last_kernel_name() == name, ctx.lib.bt709hip_last_kernel_name()
    return target.read()


def _first_pixel_difference(got, want, img, ow, oh):
    r, b = np.argwhere(got != want)[0]
    return "output row %d, column %d, channel %s: got %d, want %d; %d bytes differ (%d x %d -> %d x %d)" % (
        r, b // 4, "BGRA"[b % 4], got[r, b], want[r, b], int((got != want).sum()), img.shape[1], img.shape[0], ow, oh)


@pytest.mark.gpu
@pytest.mark.parametrize("transposed", [False, True], ids=["by-rows", "transposed"])
def test_gpu_every_half_code_in_every_channel(gh, oracle, transposed):
    """v_cvt_f32_f16 of each of the four halves of a texel, the saturate and the encode, for all 65 536 codes per channel:
    512 x 512 -> 256 x 256, against the oracle and, separately, against the closed form the CPU guard states."""
    img, codes, want = _every_code(oracle, transposed)
    got = _render(gh, img, 256, 256)
    assert np.array_equal(got, want), hc.first_code_difference(got, want, codes)
    table, closed = hc.by_code(got, codes), _closed_form(oracle)
    if not np.array_equal(table, closed):
        c, k = np.argwhere(table != closed)[0]
        raise AssertionError("half code 0x%04x in channel %s: got %d, the closed form says %d; %d entries differ"
                             % (c, "RGBA"[k], table[c, k], closed[c, k], int((table != closed).sum())))


@pytest.mark.gpu
def test_gpu_both_sides_of_every_encode_threshold_from_halves(gh, oracle):
    """render_scaled at exactly 2:1 from an RGBA16Float surface: four halves whose sum is an encode threshold or the float below
    it, every tap order, both column parities -- the twin of test_gpu_both_sides_of_every_encode_threshold_in_pass_2."""
    ef, img, want = _edge_frame(oracle)
    got = _render(gh, img, ef.COLS, ef.rows)
    assert np.array_equal(got, want), "render_scaled<rgba16f>: %s" % rc.first_difference(ef, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["finite", "nonfinite"])
@pytest.mark.parametrize("geometry", [g[0] for g in WILD_GEOMETRIES])
def test_gpu_wild_texels_at_any_weights(gh, oracle, geometry, which):
    """Any finite half, then infinities and NaNs among them, under weights that are not 1/4 (and, 1:1, exactly 0): a padded
    input pitch, a canary-filled target whose padding and guard bytes must come back untouched."""
    _, (w, h), (ow, oh) = next(g for g in WILD_GEOMETRIES if g[0] == geometry)
    img, want = _wild(oracle, geometry, which)
    got = _render(gh, img, ow, oh, in_pad=40)
    assert np.array_equal(got, want), _first_pixel_difference(got, want, img, ow, oh)


@pytest.mark.gpu
def test_gpu_wild_texels_in_a_batch(gh, oracle):
    """The finite image and the one with infinities and NaNs alternating in a ring of 5 surfaces, one launch of
    bt709hip_render_scaled_batch: non-finite lanes beside finite ones of other blockIdx.z; every surface against the oracle,
    nothing written outside the views."""
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = gh.context()
    n, (_, (w, h), (ow, oh)) = 5, WILD_GEOMETRIES[0]
    pairs = [_wild(oracle, "reduce", "nonfinite" if i & 1 else "finite") for i in range(n)]
    in_stride, out_stride = w * 8 + 40, ow * 4 + 16
    in_pitch, out_pitch = in_stride * h + 64, out_stride * oh + 64
    slab_in, slab_out = DeviceBuffer(ctx, n * in_pitch), DeviceBuffer(ctx, n * out_pitch)
    inters = [mb.BGRATexture(ctx, w, h, in_stride, ptr=slab_in.ptr + i * in_pitch, pixelFormat=F16) for i in range(n)]
    views = [mb.BGRATexture(ctx, ow, oh, out_stride, ptr=slab_out.ptr + i * out_pitch) for i in range(n)]
    for (img, _), t in zip(pairs, inters):
        ctx.fillBGRATexture(t, img)
    _capi.check(ctx.lib.bt709hip_memset(ctx.handle, slab_out.ptr, CANARY, n * out_pitch, None))
    ctx._sync(None)
    scale = mb.MetalScaleRenderContext()
    assert scale.setupRenderPipelines(ctx)
    assert scale.renderScaledBatch(ctx, views, None, inters, True), scale.lastStatus
    assert ctx.lib.bt709hip_last_kernel_name() == b"render_scaled<rgba16f>"
    raw = np.empty(n * out_pitch, np.uint8)
    _capi.check(ctx.lib.bt709hip_download(ctx.handle, raw.ctypes.data, raw.size, slab_out.ptr, raw.size, raw.size, 1, None))
    ctx._sync(None)
    raw = raw.reshape(n, out_pitch)
    assert (raw[:, out_stride * oh:] == CANARY).all(), "bytes written between the views"
    rows = raw[:, :out_stride * oh].reshape(n, oh, out_stride)
    assert (rows[:, :, ow * 4:] == CANARY).all(), "bytes written into the rows' padding"
    for i, (img, want) in enumerate(pairs):
        got = rows[i, :, :ow * 4]
        assert np.array_equal(got, want), "surface %d: %s" % (i, _first_pixel_difference(got, want, img, ow, oh))


@pytest.mark.gpu
def test_gpu_every_byte_in_every_channel_of_the_bgra8_form(gh, oracle):
    """lin[256] through the three SDWA byte selects, alpha through v_cvt_f32_ubyte3: flat 2x2 blocks, block (r, c) = byte
    (r + c + 64 k) & 255 in channel k, 128 x 512 -> 64 x 256."""
    src, blocks = hc.every_byte_image()
    want = oracle.render_scaled(src, 64, 256)
    got = _render(gh, src, 64, 256, name=b"render_scaled<bgra8>")
    if not np.array_equal(got, want):
        r, b = np.argwhere(got != want)[0]
        raise AssertionError("byte %d in channel %s (block row %d, column %d): got %d, want %d; %d bytes differ"
                             % (blocks[r, b // 4, b % 4], "BGRA"[b % 4], r, b // 4, got[r, b], want[r, b], int((got != want).sum())))
