"""GPU tests (-m gpu) of BT709HIP_CTX_OPT_ENCODE_CONVERT: bt709hip_encode[_batch] as the reference's per-pixel +convert:
(BT709HIP_CONVERT_PACKED444) and as +convert: followed by copyBT709ToCoreVideo in one launch (BT709HIP_CONVERT_POINT420);
DESIGN.md 3.10.

Every comparison is whole-slab byte equality, no tolerance.  Expected values come from oracle.convert_packed,
oracle.packed_to_nv12 and, for premultiplied input, straight_alpha_cases.premultiply -- never from the code under test.  Every
output slab is filled with 0x5A first, so row padding, the gaps between pictures, the bytes behind the last row and the guard bands
are part of every comparison.  Every case asserts the kernel it was built to reach."""
import numpy as np
import pytest

import convert_cases as cc
import encoder_cases as ec
import metalbt709decoder_amd as mb
import straight_alpha_cases as sc
from convert_cases import GAMMA_APPLE, GAMMA_ITU709, GAMMA_LINEAR, GAMMA_SRGB, GAMMAS, I420, NV12, PACKED, POINT
from metalbt709decoder_amd import _capi

pytestmark = pytest.mark.gpu

GAMMA_IDS = {GAMMA_APPLE: "apple", GAMMA_SRGB: "srgb", GAMMA_LINEAR: "linear", GAMMA_ITU709: "itu709"}


@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


@pytest.fixture(scope="module")
def harness(gh):
    return cc.Harness(gh)


_WORDS = {}


def converted(oracle, words, gamma):
    """oracle.convert_packed of a picture, computed once per (picture, gamma) and shared read-only."""
    key = (id(words), gamma)
    if key not in _WORDS:
        h, w = words.shape
        out = oracle.convert_packed(gamma, words, w, h).reshape(h, w)
        out.setflags(write=False)
        _WORDS[key] = (words, out)  # the picture is kept alive: its id is the key
    return _WORDS[key][1]


_PICTURES = {}


def picture(seed, w, h):
    """encoder_cases.mixed_picture with the rows' chroma made to differ between even and odd rows (odd rows: R and B swapped), so
    that which row a block's chroma comes from is visible.  Once per (seed, size), shared read-only."""
    key = (seed, w, h)
    if key not in _PICTURES:
        p = ec.mixed_picture(seed, w, h).copy()
        odd = p[1::2]
        p[1::2] = (odd & np.uint32(0xFF00FF00)) | ((odd & np.uint32(0xFF)) << np.uint32(16)) | ((odd >> np.uint32(16)) & np.uint32(0xFF))
        p.setflags(write=False)
        _PICTURES[key] = p
    return _PICTURES[key]


def outputs_of(oracle, L, gamma, pictures):
    """pictures(i) -> the (h, w) BGRA words the converter is to see for slot i -> what expected_slabs wants for slot i."""
    def one(i):
        words = converted(oracle, pictures(i), gamma)
        return words if L.mode == PACKED else oracle.packed_to_nv12(words, L.w, L.h)
    return one


def run(harness, oracle, L, gamma, pictures, kernel, plan=None, premultiply=False, knobs=(), seen=None):
    """One call over L; the slabs compared whole.  pictures(i): slot i's input words; seen(i): the words the arithmetic is to see
    (premultiplied input), default the input itself."""
    assert L.kernel(premultiply) == kernel, "the case does not reach the kernel it names: %s" % L.kernel(premultiply)
    res = harness.convert(L, ec.fill_input(L, pictures), gamma, premultiply=premultiply, knobs=knobs)
    assert res.kernel == kernel
    d = cc.differences(L, res, outputs_of(oracle, L, gamma, seen or pictures))
    assert not d, "\n".join(d)
    if plan is not None:
        assert (res.grid, res.block[0], res.launches, res.xcd_bands) == (plan["grid"], plan["block"], plan["launches"], plan["xcd_bands"]), (res.grid, res.block, plan)
    return res


# ------------------------------------------------------------------ 1. every colour

@pytest.fixture(scope="module")
def all_colours():
    """4096 x 4096: pixel i holds (R, G, B) = the three bytes of i -- all 2^24 colours -- and A = a hash of i."""
    i = np.arange(1 << 24, dtype=np.uint32)
    words = (i | ((i * np.uint32(2654435761)) & np.uint32(0xFF000000))).reshape(4096, 4096)
    words.setflags(write=False)
    return words


@pytest.fixture(scope="module")
def all_colours_words(oracle, all_colours):
    """The oracle's words for the whole picture, once per gamma (module scope), read-only."""
    cache = {}

    def get(gamma):
        if gamma not in cache:
            out = oracle.convert_packed(gamma, all_colours, 4096, 4096).reshape(4096, 4096)
            out.setflags(write=False)
            # what the sweep spans: video range in every channel, a top byte of 0
            assert (int((out & 0xFF).min()), int((out & 0xFF).max())) == (16, 235) and int((out >> 24).max()) == 0
            assert (int(((out >> 8) & 0xFF).min()), int(((out >> 8) & 0xFF).max())) == (16, 240)
            assert (int(((out >> 16) & 0xFF).min()), int(((out >> 16) & 0xFF).max())) == (16, 240)
            cache[gamma] = out
        return cache[gamma]
    return get


@pytest.mark.parametrize("path", ["fast", "blocks"])
@pytest.mark.parametrize("gamma", GAMMAS, ids=[GAMMA_IDS[g] for g in GAMMAS])
def test_every_colour(harness, all_colours, all_colours_words, gamma, path):
    """All 2^24 (R, G, B) under each output gamma, through the fast kernel and -- a word pitch of 4W + 4 -- the general one."""
    w = h = 4096
    L = cc.evenly(PACKED, w, h, 1, strides=(4 * w, 4 * w + (4 if path == "blocks" else 0), 0))
    kernel = "convert_bgra_packed444" + ("_blocks" if path == "blocks" else "")
    assert L.kernel() == kernel
    res = harness.convert(L, ec.fill_input(L, lambda i: all_colours), gamma)
    assert res.kernel == kernel and res.launches == 1
    want = all_colours_words(gamma)
    d = cc.differences(L, res, lambda i: want)
    if d:  # name the first colour that differs
        got = ec._rows_view(res.y_slab, L.y_off[0], h, L.sy, 4 * w).copy().view(np.uint32).reshape(h, w)
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        if bad.size:
            k = int(bad[0])
            d.append("%d colours differ, first RGB %06x: got %06x, want %06x" % (bad.size, k, got.reshape(-1)[k], want.reshape(-1)[k]))
    assert not d, "\n".join(d)


# ------------------------------------------------------------------ 2. geometry

WIDTHS, HEIGHTS = (2, 6, 30, 64, 260, 1284), (2, 6, 38)


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_packed_geometry(harness, oracle, w, h):
    """Partial tiles, the clamped last lane (260 = 65 quads, 1284 = 321), the row-pair group tail (38 rows = 19 pairs) under
    BT709HIP_CTX_OPT_ENCODE_ROW_PAIRS = default, 1, 4 and 9; widths 2 (mod 4) take the general kernel."""
    p = picture(w * 131 + h, w, h)
    gamma = GAMMAS[(w + h) % 4]
    L = cc.evenly(PACKED, w, h, 1, strides=((4 * w + 15) // 16 * 16, (4 * w + 15) // 16 * 16 + 16, 0))
    kernel = "convert_bgra_packed444" + ("" if w % 4 == 0 else "_blocks")
    run(harness, oracle, L, gamma, lambda i: p, kernel, plan=cc.expected_plan(L))
    if w % 4 == 0:
        for rp in (1, 4, 9):
            res = run(harness, oracle, L, gamma, lambda i: p, kernel, knobs=((_capi.CTX_OPT_ENCODE_ROW_PAIRS, rp),))
            assert res.grid[1] == (h // 2 + rp - 1) // rp


@pytest.mark.parametrize("name", ["odd-word-pitch", "odd-bgra-pitch", "word-pointer+4", "bgra-pointer+4", "all-odd"])
def test_packed_odd_pitches_and_pointers(harness, oracle, name):
    """Each alignment the fast kernel asks for, taken away on its own: the general kernel, the same words, padding untouched."""
    w, h = 260, 6
    strides, mis = {"odd-word-pitch": ((4 * w, 4 * w + 4, 0), (0, 0, 0)), "odd-bgra-pitch": ((4 * w + 4, 4 * w, 0), (0, 0, 0)),
                    "word-pointer+4": ((4 * w, 4 * w, 0), (0, 4, 0)), "bgra-pointer+4": ((4 * w, 4 * w, 0), (4, 0, 0)),
                    "all-odd": ((4 * w + 12, 4 * w + 20, 0), (8, 12, 0))}[name]
    p = picture(11, w, h)
    L = cc.evenly(PACKED, w, h, 1, strides=strides, misalign=mis)
    run(harness, oracle, L, GAMMA_APPLE, lambda i: p, "convert_bgra_packed444_blocks", plan=cc.expected_plan(L))


# ------------------------------------------------------------------ 3. batches

def slot_pictures(n, w, h, seed):
    """n pictures, each its own (a shared base with the slot's number hashed into every fourth column)."""
    base = picture(seed, w, h)
    pics = []
    for i in range(n):
        p = base.copy()
        p[:, (i % 4)::4] ^= np.uint32((i * 2654435761 + 12345) & 0x00FFFFFF)
        p.setflags(write=False)
        pics.append(p)
    return pics


@pytest.mark.parametrize("name", ["table-3", "even-5-negative-step", "even-2", "table-3-blocks", "even-5-blocks"])
def test_packed_batches(harness, oracle, name):
    w, h = (64, 6) if "blocks" not in name else (30, 6)
    n = int(name.split("-")[1])
    kw = dict(gaps=(256, 512, 0))
    L = cc.irregular(PACKED, w, h, n, **kw) if name.startswith("table") else cc.evenly(PACKED, w, h, n, descending="negative" in name, **kw)
    assert L.uniform() == (not name.startswith("table"))
    pics = slot_pictures(n, w, h, 3)
    kernel = "convert_bgra_packed444" + ("_blocks" if "blocks" in name else "")
    res = run(harness, oracle, L, GAMMA_ITU709, lambda i: pics[i], kernel, plan=cc.expected_plan(L))
    assert res.grid[2] == n


# ------------------------------------------------------------------ 4. launch regimes

def test_single_picture_reaches_the_512_lane_tiles(harness, oracle):
    w, h = 2560, 8  # 640 quads: two tiles of 320 lanes for a batch, 2 x 320 ... one picture: tiles of up to 512 lanes
    p = picture(5, w, h)
    L = cc.evenly(PACKED, w, h, 1)
    plan = cc.expected_plan(L)
    assert plan["block"] == 320 and plan["grid"][0] == 2
    run(harness, oracle, L, GAMMA_SRGB, lambda i: p, "convert_bgra_packed444", plan=plan)
    w = 1920  # 480 quads: one tile of 512 lanes where a batch takes two of 256
    p, L = picture(6, w, h), cc.evenly(PACKED, w, h, 1)
    plan = cc.expected_plan(L)
    assert plan["block"] == 512 and plan["grid"][0] == 1
    run(harness, oracle, L, GAMMA_SRGB, lambda i: p, "convert_bgra_packed444", plan=plan)


@pytest.mark.parametrize("n", [64, 65])
def test_band_map_and_tail(harness, oracle, n):
    """64 pictures of 64 x 8: the XCD band map; 65: 64 banded plus a tail launch of one.  With BT709HIP_CTX_OPT_XCD_BANDS = 0: one
    plain launch."""
    w, h = 64, 8
    pics = slot_pictures(n, w, h, 9)
    L = cc.evenly(PACKED, w, h, n)
    plan = cc.expected_plan(L)
    assert plan["xcd_bands"] == 1 and plan["launches"] == (2 if n == 65 else 1)
    run(harness, oracle, L, GAMMA_LINEAR, lambda i: pics[i], "convert_bgra_packed444", plan=plan)
    plain = cc.expected_plan(L, bands=False)
    assert plain["xcd_bands"] == 0 and plain["launches"] == 1
    run(harness, oracle, L, GAMMA_LINEAR, lambda i: pics[i], "convert_bgra_packed444", plan=plain, knobs=((_capi.CTX_OPT_XCD_BANDS, 0),))


def test_encode_threads_64(harness, oracle):
    w, h = 1284, 6
    p, L = picture(13, w, h), cc.evenly(PACKED, w, h, 1)
    res = run(harness, oracle, L, GAMMA_APPLE, lambda i: p, "convert_bgra_packed444", knobs=((_capi.CTX_OPT_ENCODE_THREADS, 64),))
    assert res.block[0] == 64 and res.grid[0] == (321 + 63) // 64


# ------------------------------------------------------------------ 5. POINT420

POINT_CASES = {
    # name: (w, h, n, chroma, strides (None: tight), misalign, kernel)
    "nv12-fast-260x6": (260, 6, 1, NV12, None, (0, 0, 0), "convert_bgra_nv12"),
    "nv12-fast-1284x38-padded": (1284, 38, 1, NV12, (5200, 1288, 1300), (0, 0, 0), "convert_bgra_nv12"),
    "nv12-blocks-62x6": (62, 6, 1, NV12, None, (0, 0, 0), "convert_bgra_nv12_blocks"),
    "nv12-blocks-odd-everything": (260, 6, 1, NV12, (4 * 260 + 4, 263, 261), (4, 1, 3), "convert_bgra_nv12_blocks"),
    "i420-fast-260x6": (260, 6, 1, I420, None, (0, 0, 0), "convert_bgra_i420"),
    "i420-fast-u+2": (1284, 6, 1, I420, (4 * 1284, 1284, 646), (0, 0, 2), "convert_bgra_i420"),
    "i420-blocks-62x6": (62, 6, 1, I420, None, (0, 0, 0), "convert_bgra_i420_blocks"),
    "i420-blocks-u-odd": (64, 8, 1, I420, (256, 64, 33), (0, 0, 1), "convert_bgra_i420_blocks"),
    "nv12-fast-batch-5": (64, 6, 5, NV12, None, (0, 0, 0), "convert_bgra_nv12"),
    "i420-fast-batch-64": (64, 8, 64, I420, None, (0, 0, 0), "convert_bgra_i420"),
}


@pytest.mark.parametrize("name", POINT_CASES)
def test_point420(harness, oracle, name):
    """+convert: then copyBT709ToCoreVideo: every pixel's Y, a block's chroma from its odd row and even column -- the picture's odd
    rows have R and B swapped, so the other row's chroma would show.  Both layouts, fast and general kernels."""
    w, h, n, chroma, strides, mis, kernel = POINT_CASES[name]
    L = cc.evenly(POINT, w, h, n, strides=strides, misalign=mis, chroma=chroma)
    pics = slot_pictures(n, w, h, 21)
    gamma = GAMMAS[len(name) % 4]
    words = converted(oracle, pics[0], gamma)
    y, c = oracle.packed_to_nv12(words, w, h)
    even_row = np.stack([(words[0::2, 0::2] >> 8) & 0xFF, (words[0::2, 0::2] >> 16) & 0xFF], -1).reshape(h // 2, w)
    assert (c != even_row).any(), "the picture does not tell the odd row's chroma from the even row's"
    run(harness, oracle, L, gamma, lambda i: pics[i], kernel, plan=cc.expected_plan(L))


# ------------------------------------------------------------------ 6. premultiply composes

@pytest.mark.parametrize("mode", [PACKED, POINT], ids=["packed444", "point420"])
def test_premultiply_then_convert(harness, oracle, mode):
    """BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY: B, G, R times A first (straight_alpha_cases.premultiply), then converted."""
    w, h = 260, 6
    p = picture(31, w, h)
    pre = sc.premultiply(p)
    pre.setflags(write=False)
    assert (pre != p).any()
    L = cc.evenly(mode, w, h, 1)
    kernel = ("convert_bgra_packed444" if mode == PACKED else "convert_bgra_nv12") + "<premul>"
    run(harness, oracle, L, GAMMA_APPLE, lambda i: p, kernel, premultiply=True, seen=lambda i: pre, plan=cc.expected_plan(L))
    Lb = cc.evenly(mode, 62, h, 1)
    pb = picture(32, 62, h)
    preb = sc.premultiply(pb)
    preb.setflags(write=False)
    run(harness, oracle, Lb, GAMMA_SRGB, lambda i: pb, kernel.replace("<premul>", "_blocks<premul>"), premultiply=True, seen=lambda i: preb)


# ------------------------------------------------------------------ 7. the host mirror and the reference's flow on the device

def test_python_mirror_convert_and_unconvert_round_trip(gh, oracle):
    """BGRAToBT709Converter.convert / convertBatch: host arrays in and out; the option is back at OFF afterwards (a plain encode
    with a chroma plane goes through)."""
    ctx = gh.context()
    w, h = 30, 6
    pics = slot_pictures(3, w, h, 41)
    outs = [np.zeros(w * h, np.uint32) for _ in pics]
    assert mb.BGRAToBT709Converter.convertBatch(ctx, pics, outs, w, h, mb.MetalBT709GammaLinear)
    for p, o in zip(pics, outs):
        assert (o == oracle.convert_packed(GAMMA_LINEAR, p, w, h)).all()
    tex = ctx.makeBGRATexture((w, h), pixels=pics[0])
    one = np.zeros((h, w), np.uint32)
    assert mb.BGRAToBT709Converter.convert(ctx, tex, one, w, h, mb.MetalBT709GammaITU709)
    assert (one.reshape(-1) == oracle.convert_packed(GAMMA_ITU709, pics[0], w, h)).all()
    assert not mb.BGRAToBT709Converter.convert(ctx, pics[0][:, :29], np.zeros(29 * h, np.uint32), 29, h)  # odd sizes are refused
    buf = mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (w, h))
    assert mb.BGRAToBT709Converter.convertIntoCoreVideoBuffer(tex, buf, mb.MetalBT709GammaSRGB, mb.MetalBT709GammaApple)
    assert ctx.lib.bt709hip_last_kernel_name().decode() == "encode_bgra_nv12_blocks"


def test_reference_test_flow_on_the_device(gh, oracle, vectors):
    """MetalBT709DecoderTests.m:189-277: +convert:, copyBT709ToCoreVideo, -decodeBT709:.  The colours of tests/golden/vectors.json:
    the one-launch device form of the first two steps, then the decode, gives the texels the existing host-side flow gives
    (tests/test_gpu_parity.py:43-60, the numpy copyBT709ToCoreVideo over the oracle's +convert: words) -- and, wherever the
    oracle's +convert: of the colour is the vector's YCbCr, the vector's golden RGB."""
    ctx = gh.context()
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    golden = 0
    for r in vectors["metal_decode"]:
        R, G, B = r["rgb_in"]
        bgra = np.full((2, 2), (0xFF << 24) | (R << 16) | (G << 8) | B, dtype=np.uint32)
        words = oracle.convert_packed(GAMMA_APPLE, bgra, 2, 2)
        host = mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (2, 2))
        mb.BGRAToBT709Converter.setBT709Attributes(host)
        mb.BGRAToBT709Converter.copyBT709ToCoreVideo(words, host)
        device = mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (2, 2))
        assert mb.BGRAToBT709Converter.convertIntoCoreVideoBufferPointSampled(ctx.makeBGRATexture((2, 2), pixels=bgra), device, mb.MetalBT709GammaApple)
        assert ctx.lib.bt709hip_last_kernel_name().decode() == "convert_bgra_nv12_blocks"
        got = []
        for buf in (host, device):
            tex = ctx.makeBGRATexture((2, 2))
            assert dec.decodeBT709(buf, None, tex, ctx.commandQueue.commandBuffer(), None, 2, 2, True), r["test"]
            got.append(ctx.getBGRATexturePixels(tex))
        assert (got[0] == got[1]).all(), (r["test"], got)
        if [int(words[0]) & 0xFF, (int(words[0]) >> 8) & 0xFF, (int(words[0]) >> 16) & 0xFF] == r["ycbcr"]:
            golden += 1
            for word in got[1].reshape(-1):
                assert [(int(word) >> 16) & 0xFF, (int(word) >> 8) & 0xFF, int(word) & 0xFF] == r["rgb_out"] and int(word) >> 24 == 0xFF, r["test"]
    assert golden >= 1, "no vector's YCbCr is the per-pixel converter's: the golden leg checked nothing"
