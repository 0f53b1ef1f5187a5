"""The fused decode + rescale into planar CHW views on the GPU (BT709HIP_OPT_SCALED_CHW), through the C ABI and held
to the definition bit for bit, floats by their bit patterns:

    chw_of(oracle.decode_nv12_scaled(gamma, y, c, OW, OH, alpha=a), dtype, scale, bias, planes)

and, as a second statement of the same thing, chw_of over the product's own BGRA8 bt709hip_decode_scaled of the same frames.  The
shapes are the smallest that still cross a wave, a 256-column tile and a strip boundary, one per tap form
(tests/scaled_chw_cases.py).  Every test asserts the kernel's name and the tap form on the launcher's record; every target sits in
a canary slab with padded rows and room for a fourth plane, and every byte outside the planes' rows must be what it was."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chw_cases as cc
import metalbt709decoder_amd as mb
import scaled_chw_cases as sc
import variant_cases as vc
from metalbt709decoder_amd import _capi

APPLE, SRGB = sc.APPLE, sc.SRGB
ITEM = {"uint8": 1, "float16": 2, "float32": 4}


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


def decoder(rig, gamma, alpha, scale=None, bias=None, on=True):
    scale, bias = (scale, bias) if scale is not None else cc.IMAGENET
    return rig.decoder(gamma=gamma, has_alpha=alpha, options=sc.norm_options(scale, bias) + ([(sc.OPT, 1)] if on else []))


_own = {}


def own_view(rig, gh, shape, gamma, alpha, n=1, view=None, spacing="even"):
    """The product's BGRA8 bt709hip_decode_scaled_batch of frames 0..n-1 of a shape: ([(OH, OW) words], the launch's plan), once."""
    src, dst, layout, _ = sc.SHAPES[shape]
    key = (shape, gamma, alpha, n, view or dst, spacing)
    if key not in _own:
        job = sc.ViewJob(rig, [sc.planes(shape, i) for i in range(n)], layout, view or dst, None, alpha, spacing=spacing, transfer=gh.TRANSFER_FOR_GAMMA[gamma])
        try:
            _capi.check(job.launch(decoder(rig, gamma, alpha, on=False)))
            assert rig.kernel() == (b"decode_nv12_scaled<alpha>" if alpha else b"decode_nv12_scaled"), rig.kernel()
            _own[key] = (job.collect("BGRA8 view of " + shape), sc.plan(rig.lib))
        finally:
            job.free()
    return _own[key]


def check_plan(plan, twin, taps, label):
    assert plan["taps"] in taps and plan["taps"] == twin["taps"], (label, plan, twin)  # the form the BGRA8 call of the same frames takes
    assert plan["persistent"] == (0 if plan["taps"] in sc.BY_WAVE else 1) == twin["persistent"] and plan["block"] == (256, 1, 1), (label, plan)
    assert (plan["rows"], plan["items"]) == (twin["rows"], twin["items"]) or plan["resident"] != twin["resident"], (label, plan, twin)


def run_view(rig, gh, oracle, shape, dtype, gamma, alpha, n=1, spacing="even", reverse=False, entry="bt709hip_decode_scaled_batch", dec=None,
             scale=None, bias=None, row_pad=None, out_offset=0, view=None, own=True, label=""):
    """One call into planar views of frames 0..n-1 of a shape; name, plan, canary and every element checked.  -> (planes per frame, plan)"""
    src, dst, layout, taps = sc.SHAPES[shape]
    view = view or dst
    scale, bias = (scale, bias) if scale is not None else cc.IMAGENET
    count = 4 if alpha else 3
    label = "%s %s %s gamma %d%s x%d %s%s %s" % (label, shape, dtype, gamma, " alpha" if alpha else "", n, spacing, " reversed" if reverse else "", entry)
    job = sc.ViewJob(rig, [sc.planes(shape, i) for i in range(n)], layout, view, dtype, alpha, row_pad=ITEM[dtype] if row_pad is None else row_pad,
                     out_offset=out_offset, spacing=spacing, reverse=reverse, transfer=gh.TRANSFER_FOR_GAMMA[gamma])
    try:
        _capi.check(job.launch(dec or decoder(rig, gamma, alpha, scale, bias), entry), label)
        assert rig.kernel() == sc.kernel_name(dtype, alpha), (label, rig.kernel())
        plan = sc.plan(rig.lib)
        got = job.collect(label)
        twin_words, twin_plan = own_view(rig, gh, shape, gamma, alpha, n, view, spacing) if own else (None, None)
        if own:
            check_plan(plan, twin_plan, taps, label)
        for i in range(n):
            cc.assert_planes(got[i], cc.chw_of(sc.want_words(oracle, shape, gamma, alpha, i, view), dtype, scale, bias, count), label + ": frame %d against the oracle" % i)
            if own:
                cc.assert_planes(got[i], cc.chw_of(twin_words[i], dtype, scale, bias, count), label + ": frame %d against the product's BGRA8 view" % i)
        return got, plan
    finally:
        job.free()


# ------------------------------------------------------------------ 1. parity per tap form

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_gpu_parity_per_tap_form(rig, gh, oracle, shape, dtype):
    """Every shape under an opaque Apple-gamma decoder and an alpha decoder -- `wide` and `once` under all four gammas -- against the
    oracle AND the product's BGRA8 view; an opaque decoder leaves the place of a fourth plane alone (the slot has room for one)."""
    decoders = [(APPLE, False), (SRGB, True)] + ([(g, False) for g in (1, 2, 3)] if shape in ("wide", "once") else [])
    for gamma, alpha in decoders:
        run_view(rig, gh, oracle, shape, dtype, gamma, alpha, entry="bt709hip_decode_scaled")


# ------------------------------------------------------------------ 2. the normalisation in both launch kinds

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("shape", ["wide", "once"])
def test_gpu_normalisation_in_every_launch_kind(rig, gh, oracle, shape, dtype):
    """A distinct scale and bias per channel (the host replay's list, three pairs at a time) on a persistent form, whose launcher
    writes tiles_x and tile_rows into the words gather_batch put scale G and B in, and on a by-wave form."""
    for scale, bias in cc.pairs_in_threes():
        _, plan = run_view(rig, gh, oracle, shape, dtype, APPLE, False, scale=scale, bias=bias, label="scale %s bias %s" % (scale, bias))
        assert plan["persistent"] == (1 if shape == "wide" else 0)


# ------------------------------------------------------------------ 3. every code

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_gpu_every_code_in_every_channel(rig, gh, oracle, dtype):
    """chw_cases.norm_picture at ratio 1: the expected view carries every code 0..255 in every channel, at every position of a quad
    and in both rows (asserted on the expectation), under the ImageNet mean and std."""
    y, c = cc.norm_picture(*gh.exhaustive_frame())
    h, w = y.shape
    name = sc.add_shape("every-code", (w, h), (w, h), "aligned", ("wide",))
    sc._memo[("planes", name, 0)] = (y, c, None)
    want = sc.want_words(oracle, name, SRGB, False)
    assert cc.code_coverage(want).all()
    run_view(rig, gh, oracle, name, dtype, SRGB, False, row_pad=0)


# ------------------------------------------------------------------ 4. batches

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("shape", ["wide", "shared"])
def test_gpu_batches(rig, gh, oracle, shape, dtype):
    """One frame; three through the pointer table; three evenly spaced (an NCHW tensor's slices: the slot IS four planes, the step
    positive); three evenly spaced running backwards (the tensor flipped along N: a negative step)."""
    for n, spacing, reverse in ((1, "even", False), (3, "table", False), (3, "even", False), (3, "even", True)):
        _, plan = run_view(rig, gh, oracle, shape, dtype, APPLE, False, n=n, spacing=spacing, reverse=reverse, row_pad=0)
        assert plan["items"] % n == 0 and plan["items"] >= n, plan
    run_view(rig, gh, oracle, shape, dtype, SRGB, True, n=3, spacing="even", reverse=True)


@pytest.mark.gpu
def test_gpu_the_persistent_loop_takes_more_than_one_trip(rig, gh, oracle):
    """As many tiny frames as give the resident workgroups more than one item each -- the count worked out from `resident` on the
    launcher's record of a one-frame launch, not from a constant.  Seven distinct frames in turn: a workgroup that took the wrong
    item would show."""
    shape, dtype = "identity", "uint8"
    (w, h), view, layout, taps = sc.SHAPES[shape]
    _, one = run_view(rig, gh, oracle, shape, dtype, APPLE, False)
    assert one["persistent"] == 1 and one["resident"] >= 1
    # a strip has at most 16 rows (per-lane forms), so a frame is at least ceil(OH / 16) items: n frames of them exceed 1.5 x resident
    per_frame = -(-view[1] // 16)
    n = 3 * one["resident"] // (2 * per_frame) + 8
    assert n <= 65535
    frames = [sc.planes(shape, i % 7) for i in range(n)]
    job = sc.ViewJob(rig, frames, layout, view, dtype, False, row_pad=1, transfer=gh.TRANSFER_FOR_GAMMA[APPLE])
    try:
        _capi.check(job.launch(decoder(rig, APPLE, False)))
        assert rig.kernel() == sc.kernel_name(dtype, False)
        plan = sc.plan(rig.lib)
        assert plan["persistent"] == 1 and plan["taps"] in taps and plan["items"] > plan["grid"][0] == plan["resident"], plan
        got = job.collect("x%d" % n)
        want = [cc.chw_of(sc.want_words(oracle, shape, APPLE, False, i), dtype) for i in range(7)]
        for i in range(n):
            cc.assert_planes(got[i], want[i % 7], "frame %d of %d" % (i, n))
    finally:
        job.free()


# ------------------------------------------------------------------ 5. the half calls

@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [False, True], ids=["opaque", "alpha"])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("size", [(64, 40), (520, 292)], ids=["64x40", "520x292"])
def test_gpu_half_calls(rig, gh, oracle, size, dtype, alpha):
    """bt709hip_decode_half[_batch] into CHW = chw_of of the 2:1 KERNELS' BGRA8 bytes of the same frames = bt709hip_decode_scaled at
    exactly half -- the any-ratio kernel at ratio 2.0, as the record says."""
    w, h = size
    shape = sc.add_shape("half-%dx%d" % size, size, (w // 2, h // 2), "aligned", ("wide",))
    gamma = SRGB if alpha else APPLE
    count = 4 if alpha else 3
    # the 2:1 kernels' own bytes
    src = sc.ViewJob(rig, [sc.planes(shape, i) for i in range(2)], "aligned", (w // 2, h // 2), None, alpha, transfer=gh.TRANSFER_FOR_GAMMA[gamma])
    try:
        _capi.check(src.launch(decoder(rig, gamma, alpha, on=False), "bt709hip_decode_half_batch"))
        assert rig.kernel().startswith(b"decode_nv12_half"), rig.kernel()
        half_words = src.collect("2:1 kernels")
    finally:
        src.free()
    scaled, _ = run_view(rig, gh, oracle, shape, dtype, gamma, alpha, entry="bt709hip_decode_scaled")
    one, plan = run_view(rig, gh, oracle, shape, dtype, gamma, alpha, entry="bt709hip_decode_half")
    two, _ = run_view(rig, gh, oracle, shape, dtype, gamma, alpha, n=2, entry="bt709hip_decode_half_batch")
    assert plan["taps"] == "wide" and plan["persistent"] == 1
    cc.assert_planes(one[0], scaled[0], "decode_half against decode_scaled at exactly half")
    for i in range(2):
        cc.assert_planes(two[i], cc.chw_of(half_words[i], dtype, *cc.IMAGENET, planes=count), "decode_half_batch frame %d against the 2:1 kernels' bytes" % i)


# ------------------------------------------------------------------ 6. odd geometry

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_gpu_odd_geometry(rig, gh, oracle, dtype):
    """The output side has no fast / general split: one kernel takes widths that are no multiple of 4 (346 is `wide`'s; 37 and 301
    here), views one column wide and one row tall, a plane base that is only e-aligned and a pitch of OW e + e."""
    e = ITEM[dtype]
    for view in ((37, 5), (301, 7), (1, 24), (40, 1), (1, 1)):
        for out_offset in (0, e):
            run_view(rig, gh, oracle, "identity", dtype, APPLE, False, view=view, row_pad=e, out_offset=out_offset, label="view %dx%d" % view)
    run_view(rig, gh, oracle, "identity", dtype, SRGB, True, view=(37, 5), row_pad=e, out_offset=e)
    run_view(rig, gh, oracle, "once", dtype, APPLE, False, view=(301, 170), row_pad=e, out_offset=e)  # a by-wave form: the last wave is partly past the row


# ------------------------------------------------------------------ 7. graph, option off, mirror, torch

@pytest.mark.gpu
def test_gpu_graph_replays_into_refilled_targets(rig, gh, oracle):
    shape, dtype = "decimate", "float16"
    src, view, layout, _ = sc.SHAPES[shape]
    job = sc.ViewJob(rig, [sc.planes(shape)], layout, view, dtype, False, row_pad=2, transfer=gh.TRANSFER_FOR_GAMMA[APPLE])
    cb = rig.ctx.commandQueue.commandBuffer(new_stream=True)
    rec = None
    try:
        dec = rig.decoder(gamma=APPLE, has_alpha=False, options=sc.norm_options(*cc.IMAGENET))  # set up; the option is set while recording
        cb.beginRecording()
        _capi.check(rig.lib.bt709hip_decoder_set_option(dec, sc.OPT, 1))
        _capi.check(job.launch(dec, "bt709hip_decode_scaled", stream=cb.stream, wait=0))
        rec = cb.endRecording()
        assert np.array_equal(rig.download(job.d_out.ptr, job.out_bytes), job.before)  # recorded, not run
        want = cc.chw_of(sc.want_words(oracle, shape, APPLE, False), dtype, *cc.IMAGENET)
        for replay in (1, 2):
            job.refill()
            rec.replay(cb)
            cb.waitUntilCompleted()
            cc.assert_planes(job.collect("replay %d" % replay)[0], want, "replay %d" % replay)
    finally:
        if rec is not None:
            rec.release()
        cb.release()
        job.free()


@pytest.mark.gpu
def test_gpu_option_off_refuses_and_writes_nothing_and_the_mirror(rig, gh, oracle):
    shape = "decimate"
    src, view, layout, _ = sc.SHAPES[shape]
    job = sc.ViewJob(rig, [sc.planes(shape)], layout, view, "float32", False, transfer=gh.TRANSFER_FOR_GAMMA[APPLE])
    try:
        assert job.launch(decoder(rig, APPLE, False, on=False), "bt709hip_decode_scaled") == _capi.ERR_INVALID_ARG
        assert np.array_equal(rig.download(job.d_out.ptr, job.out_bytes), job.before)
    finally:
        job.free()
    # the Python mirror: a CHWTexture through decodeBT709Scaled, a general view and an exact half view (the half call)
    ctx = gh.context()
    y, c, _ = sc.planes(shape)
    (w, h) = src
    dec = gh.make_decoder(APPLE)
    assert dec.setCHWMeanStd(cc.IMAGENET_MEAN, cc.IMAGENET_STD)
    buf = gh.make_buffer(y, c, APPLE)
    tex = ctx.makeCHWTexture(view, "float16")
    assert dec.decodeBT709Scaled(buf, tex, waitUntilCompleted=True) is False and dec.lastStatus == _capi.ERR_INVALID_ARG
    assert dec.setScaledCHW(True) and dec.scaledCHW
    for size in (view, (w // 2, h // 2)):
        tex = ctx.makeCHWTexture(size, "float16")
        assert dec.decodeBT709Scaled(buf, tex, waitUntilCompleted=True), dec.lastStatus
        assert ctx.lib.bt709hip_last_kernel_name() == b"decode_nv12_scaled_chw<f16>"
        cc.assert_planes(ctx.getCHWTexturePixels(tex), cc.chw_of(sc.want_words(oracle, shape, APPLE, False, 0, size), "float16", *cc.IMAGENET), "mirror %dx%d" % size)


@pytest.mark.gpu
def test_gpu_torch_nchw_batch_in_one_launch(oracle, tmp_path):
    """A float16 (N, 3, OH, OW) tensor filled by ONE decodeBT709ScaledBatch on torch's current stream, in a fresh process that imports
    torch before the library (tests/scaled_chw_torch_child.py asserts the wrapping, the kernel and the single launch); the values are
    held to the definition here.  Skipped only where torch does not import."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "tensor.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(here, "scaled_chw_torch_child.py"), out], capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(here), env=env)
    if r.returncode == 77:
        pytest.skip("torch is not installed: CHWTexture.fromTensor has nothing to wrap (%s)" % r.stdout.strip())
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    shape, n = sc.TORCH_SHAPE, sc.TORCH_FRAMES  # the child's frames: sc.planes(shape, i)
    got = np.load(out)
    ow, oh = sc.SHAPES[shape][1]
    assert got.shape == (n, 3, oh, ow) and got.dtype == np.float16
    for i in range(n):
        want = cc.chw_of(sc.want_words(oracle, shape, APPLE, False, i), "float16", *cc.IMAGENET)
        cc.assert_planes(got[i], want, "tensor image %d" % i)
