"""Planar CHW decode targets on the GPU (BT709HIP_FORMAT_CHW_U8 / _F16 / _F32), through the C ABI and held to the
definition bit for bit (tests/chw_cases.py: chw_of over the oracle's decode, and over the product's own BGRA8 decode of the same
frames):

  1. every (Y,Cb,Cr) through the fast kernel in its three gamma forms and through the general kernel (CHW_U8), and through the
     float elements under the ImageNet scale and bias;
  2. geometry: the smallest widths, one tile +- one quad, widths 2 (mod 4), heights 2 and 6, row padding of e and of 16 bytes, a base
     offset by e -- every element type, both chroma layouts, every byte outside the written rows checked against the canary;
  3. alpha decoders (four planes), I420 against its NV12 twin, batches through the pointer table and the step (the band map and
     the tail split read from bt709hip_last_launch_info), the host replay's (scale, bias) list, the Python mirror and torch tensors.

Every test asserts the exact kernel name.  The unmarked test guards the normalisation picture's coverage on the CPU."""
import numpy as np
import pytest

import chw_cases as cc
import metalbt709decoder_amd as mb
import variant_cases as vc
from metalbt709decoder_amd import _capi

APPLE, SRGB, LINEAR = mb.MetalBT709GammaApple, mb.MetalBT709GammaSRGB, mb.MetalBT709GammaLinear
DTYPES = ("uint8", "float16", "float32")
FORM = {APPLE: "", SRGB: ",quantiser", LINEAR: ",log"}


def quads_name(dtype, gamma=APPLE, layout="nv12", nt=True, alpha=False):
    if alpha:
        return ("decode_%s_quads_chw<%s,alpha>" % (layout, cc.ELEM_NAMES[dtype])).encode()
    return ("decode_%s_quads_chw<%s%s%s>" % (layout, cc.ELEM_NAMES[dtype], ",nt" if nt else "", FORM[gamma])).encode()


def blocks_name(dtype, gamma=APPLE, layout="nv12", alpha=False):
    suffix = ",alpha" if alpha else (",quantiser" if gamma == SRGB else "")
    return ("decode_%s_blocks_chw<%s%s>" % (layout, cc.ELEM_NAMES[dtype], suffix)).encode()


def norm_options(scale, bias):
    return [(_capi.OPT_CHW_SCALE_R + i, cc.bits(v)) for i, v in enumerate(tuple(scale) + tuple(bias))]


@pytest.fixture(scope="module")
def colours():
    return vc.Colours()


@pytest.fixture(scope="module")
def norm_words(oracle, colours):
    """What the normalisation picture decodes to in the sRGB mode: (4096, 512) words, shared and never written."""
    y, c = cc.norm_picture(colours.y, colours.c)
    words = cc.words_of(oracle.decode_nv12(SRGB, y, c))
    words.setflags(write=False)
    return y, c, words


def test_normalisation_picture_carries_every_code_everywhere(oracle, colours, norm_words):
    """Every output code, in every channel, at every position of a quad and in both rows -- and the crop is a crop."""
    y, c, words = norm_words
    assert y.shape == (4096, 512) and c.shape == (2048, 512)
    assert cc.code_coverage(words).all()
    assert np.array_equal(words, cc.words_of(colours.image(oracle, SRGB)[:, cc.NORM_CROP]))


# ------------------------------------------------------------------ GPU plumbing

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
def every(rig, colours):
    """The every-colour frame in device memory, uploaded once."""
    job = vc.Job(rig, [(colours.y, colours.c, None)], out_size=(2, 2))
    yield job
    job.free()


@pytest.fixture(scope="module")
def own_bgra(rig, gh, colours):
    """The product's own BGRA8 decode of the every-colour frame per gamma, (4096, 4096) words, decoded on first use."""
    memo = {}

    def words(gamma):
        if gamma not in memo:
            job = vc.Job(rig, [(colours.y, colours.c, None)], transfer=gh.TRANSFER_FOR_GAMMA[gamma])
            _capi.check(job.decode_one(rig.decoder(gamma=gamma, has_alpha=False)))
            memo[gamma] = cc.words_of(job.collect("BGRA8, gamma %d" % gamma)[0])
            memo[gamma].setflags(write=False)
            job.free()
        return memo[gamma]
    return words


def bgra_of(rig, planes, gamma, has_alpha, transfer, chroma=None):
    """The product's BGRA8 decode of `planes`: [(H, W) words]."""
    job = vc.Job(rig, planes, transfer=transfer)
    _capi.check(job.decode_batch(rig.decoder(gamma=gamma, has_alpha=has_alpha)))
    got = [cc.words_of(g) for g in job.collect("BGRA8")]
    job.free()
    return got


# ------------------------------------------------------------------ 1. every colour

@pytest.mark.gpu
@pytest.mark.parametrize("case", ["u8-apple", "u8-srgb", "u8-linear", "u8-general", "f16-apple", "f32-apple"])
def test_gpu_every_colour(rig, gh, oracle, colours, every, own_bgra, case):
    dtype = {"u8": "uint8", "f16": "float16", "f32": "float32"}[case.split("-")[0]]
    gamma = {"apple": APPLE, "srgb": SRGB, "linear": LINEAR, "general": APPLE}[case.split("-")[1]]
    general = case == "u8-general"
    scale, bias = cc.IMAGENET if dtype != "uint8" else ((1.0,) * 3, (0.0,) * 3)
    every.frames[0].transfer = gh.TRANSFER_FOR_GAMMA[gamma]
    job = cc.ChwJob(rig, [(colours.y, colours.c, None)], dtype, row_pad=1 if general else 0, inp=every)
    try:
        dec = rig.decoder(gamma=gamma, has_alpha=False, options=norm_options(scale, bias))
        _capi.check(job.decode_one(dec), case)
        name, launch = rig.kernel(), rig.launch()
        assert name == (blocks_name(dtype) if general else quads_name(dtype, gamma)), name
        if not general:
            assert launch == ((1, 2048, 1), (512, 1, 1), 1, 0), launch
        got = job.collect(3, case)[0]
        cc.assert_planes(got, cc.chw_of(cc.words_of(colours.image(oracle, gamma)), dtype, scale, bias), case + " against the oracle")
        cc.assert_planes(got, cc.chw_of(own_bgra(gamma), dtype, scale, bias), case + " against the product's BGRA8 decode")
    finally:
        job.free()


# ------------------------------------------------------------------ 2. geometry

@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nv12", "i420"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_geometry(rig, gh, oracle, dtype, layout):
    e = np.dtype(dtype).itemsize
    scale, bias = cc.IMAGENET
    chroma = _capi.CHROMA_I420 if layout == "i420" else _capi.CHROMA_NV12
    dec = rig.decoder(gamma=APPLE, has_alpha=False, options=norm_options(scale, bias) + [(_capi.OPT_CHROMA_LAYOUT, chroma)])
    transfer = gh.TRANSFER_FOR_GAMMA[APPLE]

    def run(w, h, row_pad=0, out_offset=0, seed=0):
        y, c = gh.random_nv12(w, h, seed=1000 + 7 * w + h + seed)
        job = cc.ChwJob(rig, [(y, c, None)], dtype, row_pad=row_pad, out_offset=out_offset, chroma_pad=0 if layout == "i420" else None, transfer=transfer)
        try:
            label = "%s %s %dx%d pad %d offset %d" % (dtype, layout, w, h, row_pad, out_offset)
            _capi.check(job.decode_one(dec), label)
            fast = w % 4 == 0 and row_pad % (4 * e) == 0 and out_offset % (4 * e) == 0
            assert rig.kernel() == (quads_name(dtype, layout=layout) if fast else blocks_name(dtype, layout=layout)), (label, rig.kernel())
            launch = rig.launch()
            got = job.collect(3, label)[0]  # ... and nothing outside the three planes' rows, the fourth plane's place included
            cc.assert_planes(got, cc.chw_of(cc.words_of(oracle.decode_nv12(APPLE, y, c)), dtype, scale, bias), label)
            return launch
        finally:
            job.free()

    # the tile of the fast path, as the launch reports it: a 4096-wide row pair is one tile of block x quads-per-lane quads
    grid, block, launches, bands = run(4096, 2)
    assert grid[0] == 1 and 1024 % block[0] == 0
    tile_quads = block[0] * (1024 // block[0])
    assert run(4 * (tile_quads - 1), 2)[0][0] == 1 and run(4 * (tile_quads + 1), 2)[0][0] == 2  # one tile - a quad, one tile + a quad
    for w, h in ((4, 2), (8, 2), (12, 2), (4, 6), (12, 6), (6, 2), (18, 2), (6, 6), (18, 6)):
        for row_pad, out_offset in ((0, 0), (e, 0), (16, 0), (0, e), (16, 4 * e)):
            run(w, h, row_pad, out_offset)
    run(4 * (tile_quads + 1), 6, row_pad=e)  # the general kernel's column loop takes more than one trip
    run(4 * (tile_quads + 1), 6, row_pad=16)


# ------------------------------------------------------------------ 3. alpha decoders, I420, batches, normalisation, mirror

@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fast", "general"])
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_gpu_alpha_decoders_write_four_planes(rig, gh, oracle, dtype, path):
    w, h = 264, 8  # more than one wave's worth of quads; every alpha code in every position of a block
    y, c = gh.random_nv12(w, h, seed=5)
    a = vc.alpha_ramp(h, w)
    scale, bias = cc.IMAGENET
    job = cc.ChwJob(rig, [(y, c, a)], dtype, row_pad=0 if path == "fast" else np.dtype(dtype).itemsize)
    try:
        dec = rig.decoder(gamma=SRGB, has_alpha=True, options=norm_options(scale, bias))
        _capi.check(job.decode_one(dec))
        assert rig.kernel() == (quads_name(dtype, alpha=True) if path == "fast" else blocks_name(dtype, alpha=True)), rig.kernel()
        got = job.collect(4, "alpha %s %s" % (dtype, path))[0]
        own = bgra_of(rig, [(y, c, a)], SRGB, True, vc.SRGB)[0]
        want = cc.chw_of(own, dtype, scale, bias, planes=4)
        cc.assert_planes(got, want, "alpha decoder, %s, %s: against the product's BGRA8 decode" % (dtype, path))
        cc.assert_planes(got, cc.chw_of(cc.words_of(oracle.decode_nv12(SRGB, y, c, alpha=a)), dtype, scale, bias, planes=4), "... against the oracle")
        # the A plane: the BGRA8 decode's alpha bytes, or A x (1/255); the colour planes: its premultiplied bytes
        alpha_bytes = (own >> 24).astype(np.uint8)
        if dtype == "uint8":
            assert np.array_equal(got[3], alpha_bytes) and np.array_equal(got[0], ((own >> 16) & 0xFF).astype(np.uint8))
        else:
            assert np.array_equal(got[3], (alpha_bytes.astype(np.float32) * cc.INV255).astype(np.float16))
    finally:
        job.free()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_i420_equals_its_nv12_twin(rig, gh, dtype):
    w, h = 264, 6
    y, c = gh.random_nv12(w, h, seed=11)
    scale, bias = cc.IMAGENET
    dec = rig.decoder(gamma=APPLE, has_alpha=False, options=norm_options(scale, bias))
    transfer = gh.TRANSFER_FOR_GAMMA[APPLE]
    twin = cc.ChwJob(rig, [(y, c, None)], dtype, transfer=transfer)
    _capi.check(twin.decode_one(dec))
    assert rig.kernel() == quads_name(dtype)
    want = twin.collect(3, "nv12")[0]
    twin.free()
    _capi.check(rig.lib.bt709hip_decoder_set_option(dec, _capi.OPT_CHROMA_LAYOUT, _capi.CHROMA_I420))
    for chroma_pad, name in ((0, quads_name(dtype, layout="i420")), (1, blocks_name(dtype, layout="i420"))):  # an odd chroma pitch: the general path
        job = cc.ChwJob(rig, [(y, c, None)], dtype, chroma_pad=chroma_pad, transfer=transfer)
        try:
            _capi.check(job.decode_one(dec))
            assert rig.kernel() == name, rig.kernel()
            cc.assert_planes(job.collect(3, "i420 pad %d" % chroma_pad)[0], want, "I420, chroma pitch W/2 + %d, %s" % (chroma_pad, dtype))
        finally:
            job.free()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_batches(rig, gh, oracle, dtype):
    """Tiny 16x4 frames: 1, 2 and 32 through the pointer table (unevenly spaced), 33, 64, 70 and 72 through the step -- the band
    map from 64 on: 72, a multiple of 8, whole (nine frames a band), 70 as 64 under the map + 6 plain, launch_decode's own plan
    (bt709_launch.h plan_bands) -- and 40 with a negative step."""
    w, h = 16, 4
    scale, bias = cc.IMAGENET
    dec = rig.decoder(gamma=APPLE, has_alpha=False, options=norm_options(scale, bias))
    transfer = gh.TRANSFER_FOR_GAMMA[APPLE]
    for n, spacing, reverse, want_launch in ((1, "even", False, ((1, 1, 1), 1, 0)), (2, "table", False, ((1, 1, 2), 1, 0)), (32, "table", False, ((1, 1, 32), 1, 0)),
                                             (33, "even", False, ((1, 1, 33), 1, 0)), (64, "even", False, ((8, 1, 8), 1, 1)),
                                             (70, "even", False, ((8, 1, 8), 2, 1)), (72, "even", False, ((8, 1, 9), 1, 1)),
                                             (40, "even", True, ((1, 1, 40), 1, 0))):
        planes = [gh.random_nv12(w, h, seed=100 * n + i) + (None,) for i in range(n)]
        job = cc.ChwJob(rig, planes, dtype, spacing=spacing, reverse=reverse, transfer=transfer)
        try:
            if reverse:
                assert job.surfs[1].bgra < job.surfs[0].bgra
            _capi.check(job.decode_batch(dec), "n = %d" % n)
            assert rig.kernel() == quads_name(dtype), (n, rig.kernel())
            grid, block, launches, bands = rig.launch()
            assert (grid, launches, bands) == want_launch and block == (64, 8, 1), (n, grid, block, launches, bands)
            got = job.collect(3, "batch of %d" % n)
            for i, (y, c, _) in enumerate(planes):
                cc.assert_planes(got[i], cc.chw_of(cc.words_of(oracle.decode_nv12(APPLE, y, c)), dtype, scale, bias), "frame %d of %d" % (i, n))
        finally:
            job.free()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_gpu_normalisation_list(rig, norm_words, dtype):
    """The host replay's (scale, bias) pairs on a picture that carries every code in every channel at every quad position and in
    both rows: fused, reordered or double-rounded arithmetic in any lane position would show."""
    y, c, words = norm_words
    assert cc.code_coverage(words).all()
    inp = vc.Job(rig, [(y, c, None)], out_size=(2, 2), transfer=vc.SRGB)
    try:
        for scale, bias in cc.pairs_in_threes():
            dec = rig.decoder(gamma=SRGB, has_alpha=False, options=norm_options(scale, bias))
            job = cc.ChwJob(rig, [(y, c, None)], dtype, inp=inp)
            try:
                _capi.check(job.decode_one(dec))
                assert rig.kernel() == quads_name(dtype, SRGB), rig.kernel()
                cc.assert_planes(job.collect(3)[0], cc.chw_of(words, dtype, scale, bias), "%s, scale %s, bias %s" % (dtype, scale, bias))
            finally:
                job.free()
    finally:
        inp.free()


@pytest.mark.gpu
def test_gpu_mirror_decodes_into_a_chw_texture(gh, oracle):
    ctx = gh.context()
    w, h = 64, 16
    y, c = gh.random_nv12(w, h, seed=31)
    words = cc.words_of(oracle.decode_nv12(APPLE, y, c))
    dec = gh.make_decoder(APPLE)
    assert dec.setCHWMeanStd(cc.IMAGENET_MEAN, cc.IMAGENET_STD)
    buf = gh.make_buffer(y, c, APPLE)
    for dtype in DTYPES:
        tex = ctx.makeCHWTexture((w, h), dtype)
        assert dec.decodeBT709(buf, None, tex, None, None, w, h, True), dec.lastStatus
        assert ctx.lib.bt709hip_last_kernel_name() == quads_name(dtype)
        cc.assert_planes(ctx.getCHWTexturePixels(tex), cc.chw_of(words, dtype, *cc.IMAGENET), "mirror, " + dtype)
    # a batch into pitched textures, planar buffers: the layout option follows the buffers
    planar = mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (w, h), planar=True)
    planar.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
    planar.setAttachment("TransferFunction", gh.TRANSFER_FOR_GAMMA[APPLE])
    planar.upload_yuv(y, *cc.interleave_to_planar(c))
    texs = [ctx.makeCHWTexture((w, h), "float32", stride=w * 4 + 16) for _ in range(2)]
    assert dec.decodeBT709Batch([planar, planar], texs, waitUntilCompleted=True), dec.lastStatus
    assert ctx.lib.bt709hip_last_kernel_name() == quads_name("float32", layout="i420")
    for tex in texs:
        cc.assert_planes(ctx.getCHWTexturePixels(tex), cc.chw_of(words, "float32", *cc.IMAGENET), "mirror, batch")
    # a BGRA8 decode behind it is what it was
    bgra = ctx.makeBGRATexture((w, h))
    assert dec.decodeBT709(buf, None, bgra, None, None, w, h, True)
    assert np.array_equal(ctx.getBGRATexturePixels(bgra), words)


@pytest.mark.gpu
def test_gpu_torch_nchw_tensor_in_one_launch(oracle, tmp_path):
    """A float16 NCHW tensor of 40 tiny frames, each image wrapped without a copy, decoded as ONE evenly spaced batch on torch's
    current stream -- in a fresh process that imports torch before the library, as INTEGRATION.md prescribes (this process loaded
    the library long ago): tests/chw_torch_child.py asserts the wrapping, the kernel and the single launch and hands the tensor
    back; the values are held to the definition here.  Skipped only where torch does not import."""
    import os
    import subprocess
    import sys
    import gpu_helpers
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "tensor.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(here, "chw_torch_child.py"), out], capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(here), env=env)
    if r.returncode == 77:
        pytest.skip("torch is not installed: CHWTexture.fromTensor has nothing to wrap (%s)" % r.stdout.strip())
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    n, w, h = 40, 16, 4  # the child's N, W, H and seeds
    got = np.load(out)
    assert got.shape == (n, 3, h, w) and got.dtype == np.float16
    for i in range(n):
        y, c = gpu_helpers.random_nv12(w, h, seed=500 + i)
        cc.assert_planes(got[i], cc.chw_of(cc.words_of(oracle.decode_nv12(APPLE, y, c)), "float16", *cc.IMAGENET), "tensor image %d" % i)
