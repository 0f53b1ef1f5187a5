"""GPU tests (-m gpu) of BT709HIP_CTX_OPT_ENCODE_CHW_INPUT: bt709hip_encode[_batch] of planar CHW_U8 / _F16 / _F32
tensors into NV12 / I420, bit for bit.  Expected bytes never come from the code under test: they are the oracle's encode of the byte
picture tests/encode_chw_cases.py builds from the definition -- and in the same test they must equal the product's own BGRA8 encode
of that picture.  The frames of a call live in ONE output slab that is canary-filled and compared whole; the tensors lie in a slab
filled with 0xFF (the byte 255, a NaN half, a NaN float), so a read outside a plane row shows in the frame.  Every case asserts the
kernel it was built to reach.  On a tree without the feature each test fails at its first set_option (BT709HIP_ERR_INVALID_ARG)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chw_cases as cc
import encode_chw_cases as ec
import encoder_cases
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_APPLE, GAMMA_LINEAR, GAMMA_SRGB

pytestmark = pytest.mark.gpu

NV12, I420 = ec.NV12, ec.I420
SRGB_APPLE = (GAMMA_SRGB, GAMMA_APPLE)
FAST, GENERAL = "fast", "general"


@pytest.fixture(scope="module")
def rig():
    import gpu_helpers
    return ec.Rig(gpu_helpers)


def path_plan(path, w, h, n, dtype, layout, **kw):
    """fast: everything aligned; general: plane 0 one element off"""
    P = ec.Plan(w, h, n, dtype, layout, shift=np.dtype(dtype).itemsize if path == GENERAL else 0, **kw)
    assert P.fast() == (path == FAST)
    return P


# ------------------------------------------------------------------ 1: the gather, every colour

@pytest.mark.parametrize("strip", range(encoder_cases.ALL_COLOURS_STRIPS))
def test_every_colour_as_bytes_through_the_fast_kernel(rig, oracle, strip):
    """All 2^24 (R, G, B) as flat 2x2 blocks once, in eight strips of 8192 x 1024, under (sRGB, Apple)."""
    words = encoder_cases.all_colours_strip(strip, seed=2200 + strip)
    tensor = cc.chw_of(words, "uint8")
    P = path_plan(FAST, words.shape[1], words.shape[0], 1, "uint8", NV12)
    ec.check(rig, oracle, P, [tensor], SRGB_APPLE, label="strip %d" % strip)


def colour_subset():
    """2^16 distinct colours spread over the cube, as flat 2x2 blocks: 512 x 512"""
    idx = (np.arange(1 << 16, dtype=np.uint32) * np.uint32(257) + np.uint32(77)) & np.uint32(0xFFFFFF)
    assert np.unique(idx).size == 1 << 16
    return np.repeat(np.repeat(idx.reshape(256, 256), 2, axis=0), 2, axis=1)


@pytest.mark.parametrize("layout,path", [(NV12, GENERAL), (I420, FAST), (I420, GENERAL)])
def test_a_colour_subset_through_the_general_kernel_and_under_i420(rig, oracle, layout, path):
    words = colour_subset()
    P = path_plan(path, 512, 512, 1, "uint8", layout)
    ec.check(rig, oracle, P, [cc.chw_of(words, "uint8")], SRGB_APPLE)


# ------------------------------------------------------------------ 2: floats

def half_picture():
    """256 x 256 float16: every half code in R, a permutation of them in G and another in B"""
    codes = np.arange(65536, dtype=np.uint16)
    rng = np.random.default_rng(2216)
    return np.stack([codes, rng.permutation(codes), rng.permutation(codes)]).reshape(3, 256, 256).view(np.float16)


def float_picture():
    """64 x 30 float32: the sweep's edge set (specials included) in R, rolled in G, reversed in B"""
    edges = ec.float_edges()
    flat = np.resize(edges, 64 * 30)
    assert flat.size >= edges.size
    return np.stack([flat, np.roll(flat, 7), flat[::-1]]).reshape(3, 30, 64).view(np.float32)


@pytest.mark.parametrize("path", [FAST, GENERAL])
@pytest.mark.parametrize("layout", [NV12, I420])
@pytest.mark.parametrize("setting", sorted(ec.SETTINGS))
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_float_elements(rig, oracle, dtype, setting, layout, path):
    """Every half code -- NaNs, infinities, subnormals, both zeros, values above 1 and below 0 -- and the float32 edge set around
    every quantiser threshold, under the identity, ImageNet's (std, mean) and negative scales, through both kernels and layouts."""
    tensor = half_picture() if dtype == "float16" else float_picture()
    P = path_plan(path, tensor.shape[2], tensor.shape[1], 1, dtype, layout)
    ec.check(rig, oracle, P, [tensor], SRGB_APPLE, ec.SETTINGS[setting])
    if setting == "identity":  # the bytes cover the whole range
        assert np.unique(ec.bytes_of_planes(tensor)).size == 256


@pytest.mark.parametrize("gammas", [(GAMMA_LINEAR, GAMMA_LINEAR), (GAMMA_APPLE, GAMMA_SRGB)])
def test_every_input_gamma_works(rig, oracle, gammas):
    P = path_plan(FAST, 256, 256, 1, "float16", NV12)
    ec.check(rig, oracle, P, [half_picture()], gammas, ec.IMAGENET)


# ------------------------------------------------------------------ 3: geometry with canaries

def random_tensor(rng, dtype, planes, h, w):
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, (planes, h, w), dtype=np.uint8)
    return (rng.random((planes, h, w), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)).astype(dtype)


@pytest.mark.parametrize("layout", [NV12, I420])
@pytest.mark.parametrize("dtype", ec.DTYPES)
def test_geometry_with_canaries(rig, oracle, dtype, layout):
    """Widths 2 .. 258, heights 2, 4, 6; padded pitches whose padding holds poison; plane 0 off by e and by 2 e; a poisoned fourth
    plane; Y, CbCr, U and V with padded pitches: the whole output slab is compared."""
    e = np.dtype(dtype).itemsize
    rng = np.random.default_rng(2203)
    reached = set()
    for w in (2, 4, 6, 8, 12, 258):
        for h in (2, 4, 6):
            for kw in (dict(row_pad=4, y_pad=4, c_pad=4), dict(row_pad=3, shift=e, y_pad=1, c_pad=3), dict(shift=2 * e, row_pad=1), dict(row_pad=0, y_pad=0, out_shift=2)):
                P = ec.Plan(w, h, 2, dtype, layout, planes=4, **kw)
                tensors = [random_tensor(rng, dtype, 3, h, w) for _ in range(2)]
                res, _ = ec.check(rig, oracle, P, tensors, SRGB_APPLE, ec.IMAGENET, label=(w, h, kw))
                reached.add(res.kernel)
    assert reached == {ec.kernel_name(dtype, layout, True), ec.kernel_name(dtype, layout, False)}


# ------------------------------------------------------------------ 4: launch regimes

@pytest.mark.parametrize("dtype", ec.DTYPES)
def test_launch_regimes(rig, oracle, dtype):
    """ENCODE_ROW_PAIRS 1 and a value that does not divide H/2, ENCODE_THREADS 64 and the maximum, a width that ends mid-tile; the
    band map on and off over 64 evenly spaced surfaces.  The plan on record is the BGRA8 encoder's for the same size and count."""
    rng = np.random.default_rng(2204)
    w, h = 4 * 67, 34  # 67 quads: a second tile of 3 lanes under 64 threads; 17 row pairs
    tensor = random_tensor(rng, dtype, 3, h, w)
    for options in ({ec.OPT_ROW_PAIRS: 1}, {ec.OPT_ROW_PAIRS: 5}, {ec.OPT_THREADS: 64}, {ec.OPT_THREADS: 512}, {ec.OPT_THREADS: 64, ec.OPT_ROW_PAIRS: 4}):
        for layout in (NV12, I420):
            P = path_plan(FAST, w, h, 1, dtype, layout)
            res, twin = ec.check(rig, oracle, P, [tensor], SRGB_APPLE, ec.NEGATIVE, options=options, label=options)
            assert res.record == twin.record and res.record[2] == 1, (options, res.record, twin.record)
            if ec.OPT_THREADS in options:
                assert res.record[1] == options[ec.OPT_THREADS]
            if options == {ec.OPT_THREADS: 64}:
                assert res.record[0][0] == 2
    tensors = [random_tensor(rng, dtype, 3, 4, 16) for _ in range(64)]
    for bands in (1, 0):
        P = path_plan(FAST, 16, 4, 64, dtype, NV12)
        res, twin = ec.check(rig, oracle, P, tensors, SRGB_APPLE, ec.IMAGENET, options={ec.OPT_XCD_BANDS: bands})
        assert res.record == twin.record and res.record[3] == bands and res.record[2] == 1, (res.record, twin.record)


# ------------------------------------------------------------------ 5: batches

@pytest.mark.parametrize("dtype", ec.DTYPES)
def test_batches(rig, oracle, dtype):
    rng = np.random.default_rng(2205)
    w, h = 12, 4
    tensors = [random_tensor(rng, dtype, 3, h, w) for _ in range(ec.MAX_TABLE + 1)]
    # an uneven pointer table at its limit, through both kernels
    for path in (FAST, GENERAL):
        P = path_plan(path, w, h, ec.MAX_TABLE, dtype, NV12, spacing="table")
        res, _ = ec.check(rig, oracle, P, tensors[:ec.MAX_TABLE], SRGB_APPLE, ec.IMAGENET, label="table")
        assert res.record[0][2] == ec.MAX_TABLE and res.record[2] == 1
    # one past it is refused and nothing is written
    P = path_plan(FAST, w, h, ec.MAX_TABLE + 1, dtype, NV12, spacing="table")
    res = rig.encode(P, tensors, SRGB_APPLE, expect_rc=_capi.ERR_UNSUPPORTED)
    assert (res.slab == ec.FILL).all()
    # 5 evenly spaced surfaces -- an NCHW tensor -- at a spacing of more than one frame; and 40: more than any table holds
    for n, layout in ((5, NV12), (5, I420), (40, NV12)):
        P = path_plan(FAST, w, h, n, dtype, layout, planes=4, slot_pad=(4096, 512))
        res, _ = ec.check(rig, oracle, P, (tensors * 2)[:n], SRGB_APPLE, ec.IMAGENET, label="uniform %d" % n)
        assert res.record[0][2] == n and res.record[2] == 1


# ------------------------------------------------------------------ 6: addressing

@pytest.mark.parametrize("path", [FAST, GENERAL])
@pytest.mark.parametrize("dtype", ec.DTYPES)
def test_plane_offsets_past_2_to_the_32(rig, oracle, dtype, path):
    """One surface of width 4, height 2 whose pitch is 2^30 + 1 KiB: plane B starts 2 * height * stride = 2^32 + 4 KiB behind plane
    R.  The allocation is filled with 0xFF and only the six rows are written, so an offset cut to 32 bits reads poison."""
    e = np.dtype(dtype).itemsize
    w, h, stride = 4, 2, (1 << 30) + 1024
    shift = e if path == GENERAL else 0
    assert 2 * h * stride > 1 << 32
    rng = np.random.default_rng(2206)
    tensor = random_tensor(rng, dtype, 3, h, w)
    setting = ec.IMAGENET
    words = ec.words_of_planes(tensor, setting)
    y, c = oracle.encode_nv12(words & 0xFFFFFF, w, h, *SRGB_APPLE)
    nbytes = (3 * h - 1) * stride + 4096
    d_in = rig.DeviceBuffer(rig.ctx, nbytes, placement_tries=1)
    d_out = rig.DeviceBuffer(rig.ctx, 4096, placement_tries=1)
    try:
        _capi.check(rig.lib.bt709hip_memset(rig.h, d_in.ptr, ec.POISON, nbytes, None))
        _capi.check(rig.lib.bt709hip_memset(rig.h, d_out.ptr, ec.FILL, 4096, None))
        rows = np.ascontiguousarray(tensor).view(np.uint8).reshape(3 * h, w * e)
        for r in range(3 * h):  # one short copy per row: no 2-D copy is asked to carry a 1 GiB pitch
            _capi.check(rig.lib.bt709hip_upload(rig.h, d_in.ptr + shift + r * stride, w * e, rows.ctypes.data + r * w * e, w * e, w * e, 1, None))
        _capi.check(rig.lib.bt709hip_stream_synchronize(rig.h, None))
        surf = _capi.Surface(d_in.ptr + shift, stride, w, h, ec.FORMATS[np.dtype(dtype).name], 0)
        frame = _capi.Frame(d_out.ptr + 256, w, d_out.ptr + 512, w, w, h, 0, 0)
        rig.set_norm(setting)
        rig.set(ec.OPT_CHW_INPUT, 1)
        try:
            rc = rig.lib.bt709hip_encode(rig.h, surf, frame, SRGB_APPLE[0], SRGB_APPLE[1], None, 1)
        finally:
            rig.set(ec.OPT_CHW_INPUT, 0)
            rig.set_norm(ec.IDENTITY)
        _capi.check(rc, "bt709hip_encode of a surface with a 1 GiB pitch")
        assert rig.lib.bt709hip_last_kernel_name().decode() == ec.kernel_name(dtype, NV12, path == FAST)
        got = rig._download(d_out.ptr, 4096)
        want = np.full(4096, ec.FILL, np.uint8)
        want[256:256 + w * h] = y.reshape(-1)
        want[512:512 + w * h // 2] = c.reshape(-1)
        assert np.array_equal(got, want), (got[256:256 + w * h], y.reshape(-1), got[512:512 + w * h // 2], c.reshape(-1))
    finally:
        d_in.free()
        d_out.free()


# ------------------------------------------------------------------ 7: composition with the decode

@pytest.mark.parametrize("planar", [False, True])
def test_decode_into_a_tensor_then_encode_equals_the_bgra8_round(rig, planar):
    """A random frame decoded into CHW_U8 / _F16 / _F32 (ImageNet's normalisation) and into BGRA8: the encode of each tensor under
    the inverse constants equals the encode of the BGRA8 surface, byte for byte."""
    import gpu_helpers as gh
    import metalbt709decoder_amd as mb
    ctx = gh.context()
    w, h = 64, 16
    y, c = gh.random_nv12(w, h, seed=2207)
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    assert dec.setCHWMeanStd(cc.IMAGENET_MEAN, cc.IMAGENET_STD)
    buf = gh.make_buffer(y, c, mb.MetalBT709GammaApple)
    bgra = ctx.makeBGRATexture((w, h))
    assert dec.decodeBT709(buf, None, bgra, None, None, w, h, True)
    make = lambda: mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (w, h), planar=planar)
    want = make()
    assert mb.BGRAToBT709Converter.convertIntoCoreVideoBuffer(bgra, want, mb.MetalBT709GammaSRGB, mb.MetalBT709GammaApple)
    want_planes = want.download_yuv() if planar else want.download_planes()
    assert ctx.setEncodeCHWMeanStd(cc.IMAGENET_MEAN, cc.IMAGENET_STD)
    try:
        for dtype in ec.DTYPES:
            tex = ctx.makeCHWTexture((w, h), dtype)
            assert dec.decodeBT709(buf, None, tex, None, None, w, h, True)
            out = make()
            assert mb.BGRAToBT709Converter.convertCHWIntoCoreVideoBuffers([tex], [out], mb.MetalBT709GammaSRGB, mb.MetalBT709GammaApple)
            assert ctx.lib.bt709hip_last_kernel_name().decode() == ec.kernel_name(dtype, I420 if planar else NV12, True)
            got = out.download_yuv() if planar else out.download_planes()
            for g, wnt in zip(got, want_planes):
                assert np.array_equal(g, wnt), dtype
    finally:
        assert ctx.setEncodeCHWNormalisation()


# ------------------------------------------------------------------ 8: the tensor route

def test_torch_nchw_tensor_in_one_launch(oracle, tmp_path):
    """A contiguous float16 NCHW tensor, each image wrapped with CHWTexture.fromTensor without a copy, encoded as ONE batch on
    torch's current stream -- in a fresh process that imports torch before the library, as INTEGRATION.md prescribes:
    tests/encode_chw_torch_child.py asserts the wrapping, the kernel and the single launch and hands tensor and frames back; the
    frames are held to the oracle here.  Skipped only where torch does not import."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "frames.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(here, "encode_chw_torch_child.py"), out], capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(here), env=env)
    if r.returncode == 77:
        pytest.skip("torch is not installed: CHWTexture.fromTensor has nothing to wrap (%s)" % r.stdout.strip())
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    got = np.load(out)
    tensor = ec.torch_tensor_values()
    assert got["tensor"].shape == (ec.TORCH_N, 3, ec.TORCH_H, ec.TORCH_W) and np.array_equal(got["tensor"].view(np.uint16), tensor.view(np.uint16))  # read, not written
    for i in range(ec.TORCH_N):
        words = ec.words_of_planes(tensor[i], ec.IMAGENET)
        y, c = oracle.encode_nv12(words & 0xFFFFFF, ec.TORCH_W, ec.TORCH_H, GAMMA_SRGB, GAMMA_APPLE)
        assert np.array_equal(got["y"][i], y) and np.array_equal(got["c"][i], c), i
