"""GPU tests (-m gpu) of the alpha-frame encoder: BT709HIP_FORMAT_BGRA8_ALPHA input of bt709hip_encode[_batch], through the
C ABI, bytes against tests/golden/alpha_luma.json (the reference headers' own table T) and the CPU oracle.  Exact: Y = T[A] for
every pixel, every Cb and Cr = 128, nothing outside the planes is written.  The launch regimes, the layouts and the fuzzed
geometry are the colour encoder's (tests/encoder_cases.py, imported and not edited)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import encoder_cases as ec
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_LINEAR, GAMMA_SRGB

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIN = GAMMA_LINEAR
ALPHA = 3  # BT709HIP_FORMAT_BGRA8_ALPHA
KERNEL_OF = {"encode_bgra_nv12": "encode_alpha_y", "encode_bgra_nv12_blocks": "encode_alpha_y_blocks"}


@pytest.fixture(scope="module")
def T():
    return np.array(json.load(open(os.path.join(HERE, "golden", "alpha_luma.json")))["luma"], np.uint8)


@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


class AlphaHarness(ec.Harness):
    """ec.Harness with the surface format and the presence of the CbCr plane as parameters."""

    def encode_as(self, layout, in_slab, fmt=ALPHA, pair=(LIN, LIN), cbcr=True):
        capi, L = self.capi, layout
        assert in_slab.size == L.in_bytes
        d_in, d_y, d_c = (self.DeviceBuffer(self.ctx, nb, placement_tries=1) for nb in (L.in_bytes, L.y_bytes, L.c_bytes))
        try:
            assert all(d.ptr % 256 == 0 for d in (d_in, d_y, d_c))
            self._upload(d_in.ptr, in_slab)
            for d, nb in ((d_y, L.y_bytes), (d_c, L.c_bytes)):
                capi.check(self.lib.bt709hip_memset(self.h, d.ptr, ec.FILL, nb, None))
            capi.check(self.lib.bt709hip_stream_synchronize(self.h, None))
            surfs = (capi.Surface * L.n)(*[capi.Surface(d_in.ptr + o, L.sb, L.w, L.h, fmt, 0) for o in L.in_off])
            frames = (capi.Frame * L.n)(*[capi.Frame(d_y.ptr + oy, L.sy, d_c.ptr + oc if cbcr else None, L.sc if cbcr else 0, L.w, L.h, 0, 0)
                                          for oy, oc in zip(L.y_off, L.c_off)])
            capi.check(self.lib.bt709hip_encode_batch(self.h, L.n, surfs, frames, pair[0], pair[1], None, 1), "bt709hip_encode_batch")
            kernel = self.lib.bt709hip_last_kernel_name().decode()
            info = capi.LaunchInfo()
            capi.check(self.lib.bt709hip_last_launch_info(C.byref(info)))
            return ec.Result(self._download(d_y.ptr, L.y_bytes), self._download(d_c.ptr, L.c_bytes), kernel, info)
        finally:
            for d in (d_in, d_y, d_c):
                d.free()


@pytest.fixture(scope="module")
def harness(gh):
    return AlphaHarness(gh)


def single_layout(w, h, strides=None):
    sb, sy, sc = strides or (4 * w, w, w)
    return ec.Layout(w, h, (sb, sy, sc), [ec.GUARD], [ec.GUARD], [ec.GUARD])


def fast_path(L, cbcr):
    """The colour encoder's predicate; without a CbCr plane its stride and bases are not looked at."""
    if cbcr:
        return ec.fast_path(L.w, L.sb, L.sy, L.sc, L.in_off, L.y_off, L.c_off)
    return ec.fast_path(L.w, L.sb, L.sy, 0, L.in_off, L.y_off, [0])


def differences(L, res, pictures, T, cbcr):
    """pictures(i) -> (h, w) words of slot i.  The whole slabs, row padding and guard bands included, against Y = T[A] and
    CbCr = 128 (or, without a CbCr plane, a CbCr slab that kept its 0x5A fill everywhere)."""
    full = np.full((L.h // 2, L.w), 128, np.uint8)
    want_y, want_c = ec.expected_slabs(L, lambda i: (T[pictures(i) >> np.uint32(24)], full))
    if not cbcr:
        want_c = np.full(L.c_bytes, ec.FILL, np.uint8)
    return [d for d in (ec.describe_difference(L, res.y_slab, want_y, "y"), ec.describe_difference(L, res.c_slab, want_c, "cbcr")) if d]


def test_every_alpha_in_every_lane_position(harness, T):
    """All 256 values of A at all four columns of a quad, on the top and on the bottom row of a row pair; R, G and B are
    random and are encoded twice with different bytes: they must not matter.  Fast and general kernel."""
    w, h = 1024, 8
    x = np.arange(w, dtype=np.uint32)[None, :]
    s = (np.arange(h, dtype=np.uint32) // 2)[:, None]                  # the row pair shifts the ramp by one column
    a = (x + s + np.where(np.arange(h)[:, None] % 2 == 1, 128, 0).astype(np.uint32)) & np.uint32(255)
    for row in (0, 1):
        for col in range(4):
            assert np.unique(a[row::2, col::4]).size == 256
    for strides, kernel in (((4 * w, w, w), "encode_alpha_y"), ((4 * w + 4, w + 1, w + 3), "encode_alpha_y_blocks")):
        L = single_layout(w, h, strides)
        results = []
        for seed in (1, 2):
            rgb = np.random.default_rng(seed).integers(0, 1 << 24, (h, w), dtype=np.uint32)
            pic = (a << np.uint32(24)) | rgb
            res = harness.encode_as(L, ec.fill_input(L, lambda i: pic))
            assert res.kernel == kernel
            assert not differences(L, res, lambda i: pic, T, True), kernel
            results.append(res)
        assert np.array_equal(results[0].y_slab, results[1].y_slab) and np.array_equal(results[0].c_slab, results[1].c_slab)


@pytest.mark.parametrize("size", [(644, 36), (646, 10), (3840, 64)], ids=str)
def test_alpha_format_equals_the_colour_encoder_on_the_grey_picture(harness, size):
    """The reference's own definition: format 3 on P == BGRA8_SRGB under (Linear, Linear) on the host-expanded grey copy
    (A,A,A) of P, both planes, whole slabs."""
    w, h = size
    P = np.random.default_rng(w * 31 + h).integers(0, 1 << 32, (h, w), dtype=np.uint32)
    A = P >> np.uint32(24)
    grey = (A << np.uint32(16)) | (A << np.uint32(8)) | A | (np.random.default_rng(5).integers(0, 256, (h, w), dtype=np.uint32) << np.uint32(24))
    L = single_layout(w, h)
    got = harness.encode_as(L, ec.fill_input(L, lambda i: P))
    ref = harness.encode_as(L, ec.fill_input(L, lambda i: grey), fmt=_capi.FORMAT_BGRA8_SRGB)
    assert got.kernel == KERNEL_OF[ref.kernel]
    assert np.array_equal(got.y_slab, ref.y_slab) and np.array_equal(got.c_slab, ref.c_slab)


def case_pictures(case, seed):
    """Slot pictures of a launch-table case: base pictures the slots cycle through, every slot distinct in three row pairs."""
    rng = np.random.default_rng(seed)
    bases = [rng.integers(0, 1 << 32, (case.h, case.w), dtype=np.uint32) for _ in range(case.bases)]
    rows = ec.slot_rows(case.h)
    patch = rng.integers(0, 1 << 32, (case.n, len(rows), 2, case.w), dtype=np.uint32)
    patch[:, :, :, 0] = (np.arange(case.n, dtype=np.uint32) * np.uint32(2654435761))[:, None, None]
    cache = {}

    def picture(i):
        if case.n == 1:
            return bases[0]
        if i not in cache:
            if len(cache) > 4:
                cache.clear()
            words = bases[i % len(bases)].copy()
            for j, rp in enumerate(rows):
                words[2 * rp:2 * rp + 2] = patch[i, j]
            cache[i] = words
        return cache[i]

    return picture


RUNS = [(c, True) for c in ec.CASES] + [(c, False) for c in ec.CASES if c.name != "4kx64-readme-row"]


@pytest.mark.parametrize("case,cbcr", RUNS, ids=lambda v: repr(v) if isinstance(v, ec.Case) else ("cbcr" if v else "y-only"))
def test_alpha_encoder_shipped_launches(harness, T, case, cbcr):
    """Every launch regime of the colour encoder's table (one picture, pointer table, evenly spaced past 32, 64 and more under
    the XCD bands, head and tail, padded strides, the general kernel with odd strides and misaligned bases), with and without
    a CbCr plane: the kernel and the plan on record are the table's, the bytes are T[A] / 128, row padding, gaps and guard
    bands keep their 0x5A -- and so does the whole CbCr slab when no plane was given."""
    L = ec.case_layout(case)
    plan = ec.expected_plan(case.w, case.h, case.n, fast=fast_path(L, cbcr), uniform=ec.layout_is_uniform(L))
    assert ec.plan_as_expect(plan) == case.expect  # a missing CbCr plane moves no row of the table to another kernel
    picture = case_pictures(case, seed=len(case.name) * 11 + case.w)
    res = harness.encode_as(L, ec.fill_input(L, picture), cbcr=cbcr)
    got = ec.recorded_expect(res, case)
    assert (res.grid, res.block, res.launches, res.xcd_bands, res.kernel) == (
        tuple(plan["grid"]), (plan["block"], 1, 1), plan["launches"], plan["xcd_bands"], KERNEL_OF[plan["kernel"]]), (got, case.expect)
    assert case.expect["row_pairs"] in got["row_pairs_candidates"] or res.kernel.endswith("blocks")
    diffs = differences(L, res, picture, T, cbcr)
    assert not diffs, "\n".join(diffs)


FUZZ_CASES = 240


def test_alpha_encoder_fuzzed_geometry(harness, T):
    """The colour encoder's seeded geometry sequence (ec.fuzz_case: any even size, strides, alignments, single pictures and
    small batches, evenly spaced or not), every case checked; a seeded half of them without a CbCr plane.  Kernel and plan
    as the predicate and ec.expected_plan say, bytes exact, padding and guard bands untouched."""
    bad, kernels, checked = [], {}, 0
    for i in range(FUZZ_CASES):
        L, _, pics = ec.fuzz_case(i)
        cbcr = bool(np.random.default_rng([709, i]).integers(0, 2))
        res = harness.encode_as(L, ec.fill_input(L, lambda k: pics[k]), cbcr=cbcr)
        plan = ec.expected_plan(L.w, L.h, L.n, fast=fast_path(L, cbcr), uniform=ec.layout_is_uniform(L))
        what = "case %d: %dx%d x %d, strides %d/%d/%d, cbcr %s" % (i, L.w, L.h, L.n, L.sb, L.sy, L.sc, cbcr)
        if (res.kernel, res.grid, res.block[0], res.launches, res.xcd_bands) != (
                KERNEL_OF[plan["kernel"]], tuple(plan["grid"]), plan["block"], plan["launches"], plan["xcd_bands"]):
            bad.append("%s: launched %s %s x %s, expected %s" % (what, res.kernel, res.grid, res.block, plan))
        kernels[(res.kernel, cbcr)] = kernels.get((res.kernel, cbcr), 0) + 1
        bad += ["%s: %s" % (what, d) for d in differences(L, res, lambda k: pics[k], T, cbcr)]
        checked += 1
    assert checked == FUZZ_CASES >= 200
    assert not bad, "\n".join(bad[:10])
    assert all(kernels.get((k, c), 0) >= FUZZ_CASES // 16 for k in KERNEL_OF.values() for c in (True, False)), kernels


def test_alpha_encode_statuses_on_the_device(gh):
    ctx = gh.context()
    tex = ctx.makeBGRATexture((8, 4))
    buf = mb.CVPixelBuffer(ctx, 8, 4)
    surf, frame = tex.surface(), buf.frame()
    surf.format = ALPHA
    lib, h = ctx.lib, ctx.handle
    assert lib.bt709hip_encode(h, C.byref(surf), C.byref(frame), 1, 1, None, 1) == _capi.ERR_ALPHA_TRANSFER
    assert lib.bt709hip_encode(h, C.byref(surf), C.byref(frame), 3, LIN, None, 1) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_encode(h, C.byref(surf), C.byref(frame), LIN, LIN, None, 1) == 0
    assert lib.bt709hip_last_kernel_name() == b"encode_alpha_y"
    frame.cbcr = None
    assert lib.bt709hip_encode(h, C.byref(surf), C.byref(frame), LIN, LIN, None, 1) == 0
    surf.format = 0
    assert lib.bt709hip_encode(h, C.byref(surf), C.byref(frame), LIN, LIN, None, 1) == _capi.ERR_INVALID_ARG
    out = tex.surface()
    out.format = ALPHA
    dec = gh.make_decoder()
    y, c = gh.random_nv12(8, 4, 1)
    f = gh.make_buffer(y, c, dec.gamma).frame()
    rc = lib.bt709hip_decode(dec._handle, C.byref(f), None, C.byref(out), 8, 4, None, 1)
    out.format = 7
    assert rc == lib.bt709hip_decode(dec._handle, C.byref(f), None, C.byref(out), 8, 4, None, 1) != 0  # an unknown format, as before


@pytest.mark.parametrize("y_only", [False, True], ids=["with-cbcr", "y-only"])
def test_full_round_trip_on_the_device(gh, oracle, T, y_only):
    """Random BGRA+A -> colour frame (sRGB, sRGB) + alpha frame -> -decodeBT709:alphaPixelBuffer: with the alpha decoder
    (sRGB): the alpha byte is oracle.decode_alpha(T[A]) everywhere, the colour bytes are the oracle's decode of the oracle's
    encode; the same through the fused decode + rescale (exact 2:1 and a view-fit size)."""
    ctx = gh.context()
    w, h = 324, 36
    words = np.random.default_rng(7093 + y_only).integers(0, 1 << 32, (h, w), dtype=np.uint32)
    A = (words >> np.uint32(24)).astype(np.uint8)
    tex = ctx.makeBGRATexture((w, h), pixels=words)
    colour = mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (w, h))
    assert mb.BGRAToBT709Converter.convertIntoCoreVideoBuffer(tex, colour, mb.MetalBT709GammaSRGB, mb.MetalBT709GammaSRGB)
    colour.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
    colour.setAttachment("TransferFunction", mb.kCVImageBufferTransferFunction_sRGB)
    if y_only:
        from metalbt709decoder_amd.decoder import DeviceBuffer
        plane = DeviceBuffer(ctx, w * h, placement_tries=1)
        alpha = mb.CVPixelBuffer(ctx, w, h, w, w, planes=(plane.ptr, None))
    else:
        alpha = mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (w, h))
    assert mb.BGRAToBT709Converter.convertAlphaIntoCoreVideoBuffer(tex, alpha)
    assert alpha.getAttachment("TransferFunction") == mb.kCVImageBufferTransferFunction_Linear
    assert alpha.getAttachment("YCbCrMatrix") == mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2

    oy, oc = oracle.encode_nv12(words & np.uint32(0xFFFFFF), w, h, GAMMA_SRGB, GAMMA_SRGB)
    gy, gc = colour.download_planes()
    assert np.array_equal(gy, oy) and np.array_equal(gc, oc)
    want_alpha = np.array([oracle.decode_alpha(int(t)) for t in T], np.uint8)[A]
    dec = gh.make_decoder(mb.MetalBT709GammaSRGB, has_alpha=True)
    assert dec.gamma == mb.MetalBT709GammaSRGB
    out = ctx.makeBGRATexture((w, h))
    assert dec.decodeBT709(colour, alpha, out, ctx.commandQueue.commandBuffer(), None, w, h, True), dec.lastStatus
    got = ctx.getBGRATexturePixels(out).view(np.uint8).reshape(h, w * 4)
    assert np.array_equal(got[:, 3::4], want_alpha)
    want = oracle.decode_nv12(GAMMA_SRGB, oy, oc, alpha=T[A])
    assert np.array_equal(want[:, 3::4], want_alpha) and np.array_equal(got, want)
    for ow, oh in ((w // 2, h // 2), (200, 25)):
        view = ctx.makeBGRATexture((ow, oh))
        assert dec.decodeBT709Scaled(colour, view, ctx.commandQueue.commandBuffer(), True, alphaPixelBuffer=alpha), dec.lastStatus
        got = ctx.getBGRATexturePixels(view).view(np.uint8).reshape(oh, ow * 4)
        assert np.array_equal(got, oracle.decode_nv12_scaled(GAMMA_SRGB, oy, oc, ow, oh, alpha=T[A])), (ow, oh)


def test_alpha_encode_in_a_recorded_command_buffer(gh, T):
    """bt709hip_encoder_prepare(LINEAR, LINEAR) builds the alpha table, so a capture that encodes alpha records (nothing runs
    while recording) and every replay encodes what the texture holds THEN."""
    ctx = gh.context()
    w, h, n = 256, 16, 3
    _capi.check(ctx.lib.bt709hip_encoder_prepare(ctx.handle, LIN, LIN))
    rng = np.random.default_rng(99)
    texs = [ctx.makeBGRATexture((w, h), pixels=rng.integers(0, 1 << 32, (h, w), dtype=np.uint32)) for _ in range(n)]
    bufs = [mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (w, h)) for _ in range(n)]
    for b in bufs:
        b.upload_planes(np.full((h, w), ec.FILL, np.uint8), np.full((h // 2, w), ec.FILL, np.uint8))
    cb = ctx.commandQueue.commandBuffer(new_stream=True)
    cb.beginRecording()
    assert mb.BGRAToBT709Converter.convertAlphaIntoCoreVideoBuffers(texs, bufs, cb, waitUntilCompleted=False)
    rec = cb.endRecording()
    assert all(np.all(b.download_planes()[0] == ec.FILL) for b in bufs)  # recorded, not run
    for round_ in range(2):
        pics = [rng.integers(0, 1 << 32, (h, w), dtype=np.uint32) for _ in range(n)]
        for t, p in zip(texs, pics):
            ctx.fillBGRATexture(t, p)
        rec.replay(cb)
        cb.waitUntilCompleted()
        for b, p in zip(bufs, pics):
            y, c = b.download_planes()
            assert np.array_equal(y, T[p >> np.uint32(24)]) and np.all(c == 128), round_
    rec.release()
    cb.release()


def test_alpha_encode_issues_a_coalescing_decoders_queue_first(gh, oracle, T):
    """Stream order with BT709HIP_OPT_COALESCE on: a decode QUEUED on the stream writes the texture the alpha encode on that
    stream then reads.  The encode must issue the queued frame first: its Y plane is T[the decoded alpha fill], not T[what
    the texture held before]."""
    ctx = gh.context()
    lib = ctx.lib
    w, h = 320, 24
    dec = gh.make_decoder(mb.MetalBT709GammaApple, alpha_fill=0xC3, options={_capi.OPT_COALESCE: 8})
    y, c = gh.random_nv12(w, h, seed=4242)
    buf = gh.make_buffer(y, c, dec.gamma)
    tex = ctx.makeBGRATexture((w, h), pixels=np.full((h, w), 0x11000000, np.uint32))
    alpha = mb.CVPixelBuffer(ctx, w, h)
    cb = ctx.commandQueue.commandBuffer(new_stream=True)
    assert dec.decodeBT709(buf, None, tex, cb, None, w, h, False), dec.lastStatus
    assert lib.bt709hip_last_kernel_name() == b"(queued: coalescing submit)"
    assert mb.BGRAToBT709Converter.convertAlphaIntoCoreVideoBuffer(tex, alpha, cb, waitUntilCompleted=True)
    assert lib.bt709hip_last_kernel_name() == b"encode_alpha_y"
    ay, ac = alpha.download_planes(cb)
    assert T[0xC3] != T[0x11] and np.all(ay == T[0xC3]) and np.all(ac == 128)
    got = ctx.getBGRATexturePixels(tex, cb).view(np.uint8).reshape(h, w * 4)
    assert np.array_equal(got, oracle.decode_nv12(0, y, c, alpha_fill=0xC3))
    dec.setOption(_capi.OPT_COALESCE, 0)
    cb.release()


def test_alpha_clip_through_y4m(gh, T, tmp_path):
    """The reference's <name>_alpha.y4m: frames of an alpha buffer WITH a CbCr plane through Y4MWriter.write_pixel_buffer,
    read back: Y = T[A], U = V = 128."""
    from metalbt709decoder_amd import y4m
    ctx = gh.context()
    w, h, n = 96, 20, 3
    rng = np.random.default_rng(31)
    pics = [rng.integers(0, 1 << 32, (h, w), dtype=np.uint32) for _ in range(n)]
    path = str(tmp_path / "clip_alpha.y4m")
    with y4m.Y4MWriter(path, w, h, fps=30) as wr:
        for p in pics:
            buf = mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (w, h))
            assert mb.BGRAToBT709Converter.convertAlphaIntoCoreVideoBuffer(ctx.makeBGRATexture((w, h), pixels=p), buf)
            wr.write_pixel_buffer(buf)
    with y4m.Y4MReader(path) as rd:
        frames = list(rd)
    assert len(frames) == n
    for (y, u, v), p in zip(frames, pics):
        assert np.array_equal(y, T[p >> np.uint32(24)]) and np.all(u == 128) and np.all(v == 128)
