"""Planar I420 frames through the fused decode + rescale on the GPU (BT709HIP_OPT_SCALED_PLANAR = 24 under BT709HIP_OPT_CHROMA_LAYOUT =
BT709HIP_CHROMA_I420), through the C ABI and held byte for byte to

    oracle.decode_nv12_scaled(gamma, y, interleave(u, v), OW, OH, alpha=a)

-- CHW views: chw_cases.chw_of over those words -- and, as a second statement of the same thing, to what the product's own NV12 call
writes for the interleaved twin.  The arithmetic is the NV12 kernels' (one text from the tap word on); what these tests pin is the
front end: which chroma bytes reach which pixel, at which sizes, pitches and alignments, in which tap form.  Every test asserts the
kernel's name and the tap form on the launcher's record; every target sits in a canary slab and every byte outside the views' rows
must be what it was; every input byte that is no sample is filled once with 0x00 and once with 0xFF, and the output may not know."""
import numpy as np
import pytest

import chw_cases as cc
import scaled_chw_cases as sc
import scaled_planar_cases as sp
import variant_cases as vc
from metalbt709decoder_amd import _capi

pytestmark = pytest.mark.gpu

APPLE, SRGB = sc.APPLE, sc.SRGB
NORM = ((1.5, -2.25, 1.0 / 0.225), (0.125, -0.406 / 0.225, 3.0))  # a distinct scale and bias per channel


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


def decoder(rig, gamma, alpha, planar, dtype=None, norm=NORM):
    options = list(sp.I420_ON) if planar else []
    if dtype is not None:
        options += sc.norm_options(*norm) + [(sc.OPT, 1)]
    return rig.decoder(gamma=gamma, has_alpha=alpha, options=options)


_twins = {}


def twin_view(rig, gh, shape, gamma, alpha, dtype, n, chroma, view, entry):
    """What the product's own NV12 call writes for the interleaved twins of frames 0..n-1 of a shape (aligned planes), once."""
    key = (shape, gamma, alpha, dtype, n, chroma, view, entry)
    if key not in _twins:
        job = sc.ViewJob(rig, [sp.twin(sp.planes(shape, i, chroma)) for i in range(n)], "aligned", view, dtype, alpha, row_pad=0 if dtype is None else 4,
                         transfer=gh.TRANSFER_FOR_GAMMA[gamma])
        try:
            _capi.check(job.launch(decoder(rig, gamma, alpha, False, dtype), entry))
            assert rig.kernel().startswith(b"decode_nv12_"), rig.kernel()
            _twins[key] = job.collect("NV12 twin of " + shape)
        finally:
            job.free()
    return _twins[key]


def run(rig, gh, oracle, shape, gamma, alpha, dtype=None, n=1, spacing="even", chroma="neighbours", fills=(0x00, 0xFF), slot_extra=0, taps=None,
        entry="bt709hip_decode_scaled_batch", twin_entry=None, view=None):
    """One planar call per fill into the views of frames 0..n-1 of a shape: the kernel's name, the tap form on record, the canary, and
    every word or element against the oracle and against the product's NV12 call on the twin.  -> what the last call wrote"""
    src, dst, layout, want_taps = sp.SHAPES[shape]
    view = view or dst
    count = 4 if alpha else 3
    got = None
    for fill in fills:
        label = "%s %s gamma %d%s x%d %s %s fill %02x %s" % (shape, dtype or "bgra8", gamma, " alpha" if alpha else "", n, spacing, chroma, fill, entry)
        job = sp.PlanarViewJob(rig, [sp.planes(shape, i, chroma) for i in range(n)], layout, view, dtype, alpha, row_pad=0 if dtype is None else 4, spacing=spacing,
                               fill=fill, slot_extra=slot_extra, transfer=gh.TRANSFER_FOR_GAMMA[gamma])
        try:
            _capi.check(job.launch(decoder(rig, gamma, alpha, True, dtype), entry), label)
            assert rig.kernel() == sp.kernel_name(dtype, alpha), (label, rig.kernel())
            plan = sc.plan(rig.lib)
            assert plan["taps"] == (taps or want_taps), (label, plan)
            assert plan["persistent"] == (0 if plan["taps"] == "once" else 1) and plan["block"] == (256, 1, 1) and plan["grid"][2] == (1 if plan["persistent"] else n), (label, plan)
            got = job.collect(label)
        finally:
            job.free()
        twins = twin_view(rig, gh, shape, gamma, alpha, dtype, n, chroma, view, twin_entry or entry)
        for i in range(n):
            words = sp.want_words(oracle, shape, gamma, alpha, i, chroma, view)
            if dtype is None:
                sp.assert_words(got[i], words, label + ": frame %d against the oracle" % i)
                sp.assert_words(got[i], twins[i], label + ": frame %d against the NV12 call on the twin" % i)
            else:
                cc.assert_planes(got[i], cc.chw_of(words, dtype, NORM[0], NORM[1], count), label + ": frame %d against the oracle" % i)
                cc.assert_planes(got[i], twins[i], label + ": frame %d against the NV12 call on the twin" % i)
    return got


# ------------------------------------------------------------------ 1. every shape, every tap form, both decoders, both chroma sets

@pytest.mark.parametrize("alpha", [False, True], ids=["opaque", "alpha"])
@pytest.mark.parametrize("shape", [s for s in sp.SHAPES if s != "half"])
def test_parity_per_shape(rig, gh, oracle, shape, alpha):
    """The shapes of scaled_planar_cases.SHAPES, each recording the tap form its frames must take, under an opaque Apple-gamma decoder
    and an alpha decoder: chroma whose every sample differs from its neighbours under both fills, uniform random chroma under one."""
    gamma = SRGB if alpha else APPLE
    got = run(rig, gh, oracle, shape, gamma, alpha, entry="bt709hip_decode_scaled")
    run(rig, gh, oracle, shape, gamma, alpha, chroma="uniform", fills=(0xFF,), entry="bt709hip_decode_scaled")
    if shape == "w8r4":  # W % 8 == 4: the last four output columns sit on the chroma row's last, unaligned, bytes
        assert np.array_equal(got[0][:, -4:], sp.want_words(oracle, shape, gamma, alpha)[:, -4:])
    if shape == "identity":  # ratio 1: the filter's weights are 1, 0, 0, 0 and the view is the 1:1 decode of the same planar frame
        (w, h), _, layout, _ = sp.SHAPES[shape]
        job = sp.PlanarViewJob(rig, [sp.planes(shape)], layout, (w, h), None, alpha, transfer=gh.TRANSFER_FOR_GAMMA[gamma])
        try:
            _capi.check(job.launch(decoder(rig, gamma, alpha, True), "bt709hip_decode_batch"))
            assert rig.kernel().startswith(b"decode_i420_") and b"scaled" not in rig.kernel(), rig.kernel()
            sp.assert_words(got[0], job.collect("1:1 decode")[0], "identity view against bt709hip_decode of the same planar frame")
        finally:
            job.free()


@pytest.mark.parametrize("gamma", [0, 1, 2, 3])
def test_every_gamma(rig, gh, oracle, gamma):
    run(rig, gh, oracle, "wide", gamma, False, fills=(0xFF,), entry="bt709hip_decode_scaled")
    run(rig, gh, oracle, "once", gamma, False, fills=(0x00,), entry="bt709hip_decode_scaled")


# ------------------------------------------------------------------ 2. CHW views

@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("shape", ["once", "wide"])
def test_chw_views(rig, gh, oracle, shape, dtype):
    """u8, f16 and f32 planes with a distinct scale and bias per channel on the by-wave form and on a persistent one (whose launcher
    writes tiles_x and tile_rows over the words gather_batch put two scales in), opaque and alpha."""
    for gamma, alpha in ((APPLE, False), (SRGB, True)):
        run(rig, gh, oracle, shape, gamma, alpha, dtype, fills=(0xFF,), entry="bt709hip_decode_scaled")


# ------------------------------------------------------------------ 3. batches

@pytest.mark.parametrize("spacing,slot_extra,taps", [("even", 0, None), ("table", 0, None), ("even", 1, "bytes")], ids=["even", "table", "even-odd-step"])
@pytest.mark.parametrize("shape", ["once", "wide"])
def test_batches_of_three(rig, gh, oracle, shape, spacing, slot_extra, taps):
    """Three frames evenly spaced (V follows from the U step) and through the pointer table; an evenly spaced batch whose steps are
    odd puts frames 1 and 2 off every alignment, so the wide form must give way to byte loads -- the by-wave form asks for none."""
    run(rig, gh, oracle, shape, SRGB, True, n=3, spacing=spacing, slot_extra=slot_extra, fills=(0xFF,), taps=taps if shape == "wide" else None)
    run(rig, gh, oracle, shape, APPLE, False, "float16", n=3, spacing=spacing, slot_extra=slot_extra, fills=(0x00,), taps=taps if shape == "wide" else None)


# ------------------------------------------------------------------ 4. the half calls

@pytest.mark.parametrize("alpha", [False, True], ids=["opaque", "alpha"])
def test_half_calls_run_the_any_ratio_kernel(rig, gh, oracle, alpha):
    """bt709hip_decode_half[_batch] of planar frames: the any-ratio kernel at ratio 2.0 -- equal to bt709hip_decode_scaled at exactly
    half, to the oracle's any-ratio view, and to the NV12 bt709hip_decode_half (the 2:1 kernels) of the twin."""
    gamma = SRGB if alpha else APPLE
    scaled = run(rig, gh, oracle, "half", gamma, alpha, entry="bt709hip_decode_scaled")
    for entry, n in (("bt709hip_decode_half", 1), ("bt709hip_decode_half_batch", 3)):
        got = run(rig, gh, oracle, "half", gamma, alpha, n=n, fills=(0xFF,), entry=entry)
        sp.assert_words(got[0], scaled[0], entry + " against bt709hip_decode_scaled at exactly half")
    run(rig, gh, oracle, "half", gamma, alpha, "uint8", fills=(0x00,), entry="bt709hip_decode_half")


# ------------------------------------------------------------------ 5. the Python mirror: a Y4M payload in place

def test_python_mirror_y4m_payload(gh, oracle, tmp_path):
    """Two frames written as a YUV4MPEG2 clip, read back and uploaded as planar buffers: decodeBT709Scaled is refused until
    scaledPlanar is set (the target untouched), then writes what the oracle makes of the twin, in the planar kernel."""
    from metalbt709decoder_amd import y4m
    ctx = gh.context()
    (w, h), view = sp.SHAPES["wide"][0], (173, 97)
    path = str(tmp_path / "clip.y4m")
    with y4m.Y4MWriter(path, w, h) as out:
        for i in range(2):
            out.write_frame(*sp.planes("wide", i)[:3])
    dec = gh.make_decoder(APPLE)
    assert dec.scaledPlanar is False
    tex = ctx.makeBGRATexture(view)
    with y4m.Y4MReader(path) as clip:
        for i, (y, u, v) in enumerate(clip):
            buf = y4m.i420_to_pixel_buffer(ctx, y, u, v, planar=True)  # three uploads, no launch
            if i == 0:
                before = ctx.getBGRATexturePixels(tex).copy()
                assert not dec.decodeBT709Scaled(buf, tex, ctx.commandQueue.commandBuffer(), True) and dec.lastStatus == _capi.ERR_UNSUPPORTED
                assert np.array_equal(ctx.getBGRATexturePixels(tex), before)
                assert dec.setScaledPlanar(True) and dec.scaledPlanar is True
            assert dec.decodeBT709Scaled(buf, tex, ctx.commandQueue.commandBuffer(), True), dec.lastStatus
            assert ctx.lib.bt709hip_last_kernel_name() == b"decode_i420_scaled"
            want = sp.want_words(oracle, "wide", APPLE, False, i, view=view)
            assert np.array_equal(ctx.getBGRATexturePixels(tex).view(np.uint32).reshape(view[1], view[0]), want), i
    assert i == 1
