"""The fused decode + rescale into planar CHW views (BT709HIP_OPT_SCALED_CHW = 22), the parts that need no GPU: the
ids and the option's domain on a context-less decoder, and -- on the shim built against the fake HIP runtime, as
tests/test_chw_cpu.py builds it -- what the four calls return with the option off, their routing with it on, validation, the
three new refusals and their place behind the old ones, batches, graph capture and the Python mirror; then the generated code of
the thirty new kernels beside their BGRA8 twins.

The fake runtime's launcher stands in for launch_decode_scaled, the one launcher all four calls go through with a CHW target: it
reports "decode_nv12_scaled" whatever the element type and refuses what bt709_kernels.h scaled_planes_fit refuses, so what is
asserted here is the PATH, the frame count and the addressing handed to the launcher; the kernels' own names and the tap forms
are asserted on the GPU (tests/test_scaled_chw_gpu.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_headers
import chw_cases as cc
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi
from test_chw_cpu import ELEM, F16, F32, U8, Rig, _get, fake  # noqa: F401  (fake: the module-scoped fixture, built once per module that asks)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = 22
FORMATS = (U8, F16, F32)
SCALED = "kernel:decode_nv12_scaled"
W, H = Rig.W, Rig.H          # 64 x 16 frames
VIEW = (48, 10)              # a general view; the half view is W/2 x H/2
RGBA16F = _capi.FORMAT_RGBA16F


# ------------------------------------------------------------------ ids, ABI, option domain

@pytest.fixture(scope="module")
def lib():
    return mb.load_library()


def test_ids_agree_and_nothing_was_exported(lib):
    header = open(os.path.join(ROOT, "include", "bt709hip_ext.h")).read()
    assert int(re.search(r"#define\s+BT709HIP_OPT_SCALED_CHW\s+(\d+)", header).group(1)) == OPT == _capi.OPT_SCALED_CHW
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    for word in ("BT709HIP_OPT_SCALED_CHW", "setScaledCHW", "scaledCHW()"):
        assert word in hpp, word
    comment = re.search(r"/\* PLANAR CHW VIEWS.*?\*/", header, flags=re.S).group(0)
    for word in ("bt709hip_decode_scaled", "bt709hip_decode_half", "64-bit product", "2 GiB", "BT709HIP_ERR_STRIDE", "ratio 2.0", "graph capture",
                 "NOT covered", "decode_nv12_scaled_chw<f16,alpha>"):
        assert word in comment, word
    targets = re.search(r"/\* PLANAR CHW TARGETS\..*?\*/", header, flags=re.S).group(0)
    assert "bt709hip_decode_scaled[_batch]" in targets and "BT709HIP_OPT_SCALED_CHW" in targets
    # an option, not an export: the ABI and the export list are what they were
    assert lib.bt709hip_abi_version() == 504 == _capi.ABI_VERSION
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103 == len(_capi.SYMBOLS)


@pytest.mark.parametrize("has_alpha", [0, 1])
def test_option_domain_and_round_trip(lib, has_alpha):
    dec = C.c_void_p()
    assert lib.bt709hip_decoder_create(None, mb.MetalBT709GammaApple, has_alpha, C.byref(dec)) == _capi.OK
    try:
        assert _get(lib, dec, OPT) == 0  # the default
        for held in (1, 0, 1):
            assert lib.bt709hip_decoder_set_option(dec, OPT, held) == _capi.OK and _get(lib, dec, OPT) == held
            for bad in (2, -1, 7, 1 << 30, -(1 << 31)):
                assert lib.bt709hip_decoder_set_option(dec, OPT, bad) == _capi.ERR_INVALID_ARG, bad
                assert _get(lib, dec, OPT) == held  # a refused value leaves the option as it was
        # it moves no neighbour, and the gaps around it stay gaps
        assert [_get(lib, dec, o) for o in range(14, 20)] == [cc.bits(1.0)] * 3 + [cc.bits(0.0)] * 3
        for unknown in (13, 20, 21, 23, 99):
            assert lib.bt709hip_decoder_set_option(dec, unknown, 0) == _capi.ERR_INVALID_ARG
            assert lib.bt709hip_decoder_get_option(dec, unknown, C.byref(C.c_int())) == _capi.ERR_INVALID_ARG
    finally:
        lib.bt709hip_decoder_destroy(dec)


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(params=[0, 1], ids=["opaque", "alpha"])
def rig(fake, request):
    r = Rig(fake, has_alpha=request.param)
    assert fake.bt709hip_decoder_setup(r.dec) == 0
    yield r
    r.close()


def four_calls(r, fmt, n=3, which=(0, 1, 2, 3), **kw):
    """The four entry points (or those of `which`) on `n` frames, the single-frame ones on the first: [(label, return code)].
    kw: Rig.surfs' for BOTH views."""
    lib = r.lib
    f, a = r.frames(n), r.alphas(n)
    half, view = r.surfs(fmt, n=n, w=W // 2, h=H // 2, **kw), r.surfs(fmt, n=n, w=VIEW[0], h=VIEW[1], **kw)
    calls = [("half", lambda: lib.bt709hip_decode_half(r.dec, f, a, half, None, 1)), ("half_batch", lambda: lib.bt709hip_decode_half_batch(r.dec, n, f, a, half, None, 1)),
             ("scaled", lambda: lib.bt709hip_decode_scaled(r.dec, f, a, view, None, 1)), ("scaled_batch", lambda: lib.bt709hip_decode_scaled_batch(r.dec, n, f, a, view, None, 1))]
    return [(calls[i][0], calls[i][1]()) for i in which]


def codes(calls):
    return [rc for _, rc in calls]


def test_option_off_the_four_calls_treat_chw_as_an_unknown_format(fake, rig):
    r = rig
    mark = fake.fake_hip_log_size()
    unknown = codes(four_calls(r, 7))
    assert all(rc != 0 for rc in unknown)
    for fmt in FORMATS:
        assert codes(four_calls(r, fmt)) == unknown, fmt
    # switched on and off again: the same
    assert r.set(OPT, 1) == 0 and r.set(OPT, 0) == 0
    for fmt in FORMATS:
        assert codes(four_calls(r, fmt)) == unknown, fmt
    assert r.kernels(mark) == []
    # on: format 7 is still no format
    assert r.set(OPT, 1) == 0
    assert codes(four_calls(r, 7)) == unknown and r.kernels(mark) == []


@pytest.mark.parametrize("fmt", FORMATS)
def test_option_on_each_call_is_one_rescale_launch(fake, rig, fmt):
    r, n = rig, 3
    assert r.set(OPT, 1) == 0
    mark = fake.fake_hip_log_size()
    calls = four_calls(r, fmt, n)
    issued = r.kernels(mark)
    assert codes(calls) == [0] * 4, calls
    assert [(k[0], k[2]) for k in issued] == [(SCALED, 1), (SCALED, n), (SCALED, 1), (SCALED, n)], issued  # exactly one launch each
    info = _capi.ScaledLaunchInfo()
    assert fake.bt709hip_last_scaled_launch_info(C.byref(info)) == 0 and info.grid[2] == n
    # the BGRA8 calls are what they were
    mark = fake.fake_hip_log_size()
    assert codes(four_calls(r, 0)) == [0] * 4
    names = [k[0] for k in r.kernels(mark)]
    assert names[2:] == [SCALED] * 2 and all(nm.startswith("kernel:decode_nv12_half") for nm in names[:2]), names
    # RGBA16F stays a target of the 1:1 decode alone
    assert codes(four_calls(r, RGBA16F)) == [_capi.ERR_UNSUPPORTED] * 4


@pytest.mark.parametrize("fmt", FORMATS)
def test_batches_pointer_table_and_even_spacing(fake, rig, fmt):
    r, e = rig, ELEM[fmt]
    assert r.set(OPT, 1) == 0
    ow, oh = VIEW
    slot = 4 * ow * e * oh
    for entry, (vw, vh) in (("bt709hip_decode_scaled_batch", VIEW), ("bt709hip_decode_half_batch", (W // 2, H // 2))):
        fn = getattr(fake, entry)
        for n, uneven, step in ((2, False, slot), (32, True, slot), (33, False, slot), (40, False, -slot)):
            f = r.frames(n, uneven=uneven, step=16 if n > 8 else None)
            s = r.surfs(fmt, n=n, w=vw, h=vh, step=step, base=0 if step > 0 else 50 * slot)
            mark = fake.fake_hip_log_size()
            assert fn(r.dec, n, f, r.alphas(n, step=16 if n > 8 else None), s, None, 1) == 0, (entry, n)
            issued = r.kernels(mark)
            assert len(issued) == 1 and issued[0][0] == SCALED and issued[0][2] == n and issued[0][3] == s[0].bgra, (entry, n, issued)
            uniform, frames, steps = r.addressing()
            assert (uniform, frames) == (0 if uneven else 1, n), (entry, n)
            if not uneven:
                assert steps[3] == step
        # 33 unevenly placed surfaces exceed the pointer table
        mark = fake.fake_hip_log_size()
        assert fn(r.dec, 33, r.frames(33, step=16, uneven=True), r.alphas(33, step=16), r.surfs(fmt, n=33, w=vw, h=vh, step=16 * e), None, 1) == _capi.ERR_UNSUPPORTED
        assert r.kernels(mark) == []


@pytest.mark.parametrize("fmt", FORMATS)
def test_layout_validation_is_the_rescales_own(fake, rig, fmt):
    r, e = rig, ELEM[fmt]
    assert r.set(OPT, 1) == 0
    mark = fake.fake_hip_log_size()
    for vw, vh, which in ((VIEW[0], VIEW[1], (2, 3)), (W // 2, H // 2, (0, 1))):
        pick = lambda **kw: codes(four_calls(r, fmt, which=which, **kw))
        assert pick(stride=vw * e - e) == [_capi.ERR_STRIDE] * 2           # a pitch below OW e
        assert pick(stride=(1 << 32) + 4 * e) == [_capi.ERR_STRIDE] * 2    # a pitch the launch cannot carry in 32 bits
        if e > 1:
            assert pick(stride=vw * e + 1) == [_capi.ERR_STRIDE] * 2       # no multiple of e
            assert pick(base=e // 2) == [_capi.ERR_STRIDE] * 2            # a base that is not e-aligned
        assert pick(reserved=1) == [_capi.ERR_INVALID_ARG] * 2
    f, a = r.frames(2), r.alphas(2)
    # the half calls want exactly W/2 x H/2, and W, H % 4 == 0
    for bad in ((W // 2 + 2, H // 2), (W // 2, H // 2 + 1), VIEW):
        s = r.surfs(fmt, n=2, w=bad[0], h=bad[1])
        assert fake.bt709hip_decode_half(r.dec, f, a, s, None, 1) == fake.bt709hip_decode_half_batch(r.dec, 2, f, a, s, None, 1) == _capi.ERR_SIZE_MISMATCH
    assert fake.bt709hip_decode_half(r.dec, r.frames(w=66, h=16), r.alphas(w=66, h=16), r.surfs(fmt, w=33, h=8, stride=64 * e), None, 1) == _capi.ERR_ODD_DIMENSIONS
    # surfaces of a batch share one size and one format; a CHW surface among others is INVALID_ARG, as for the 1:1 decode
    s = r.surfs(fmt, n=2, w=VIEW[0], h=VIEW[1], stride=VIEW[0] * 8)
    s[1].width += 2
    assert fake.bt709hip_decode_scaled_batch(r.dec, 2, f, a, s, None, 1) == _capi.ERR_SIZE_MISMATCH
    for other in (0,) + tuple(o for o in FORMATS if o != fmt):
        for first, second in ((fmt, other), (other, fmt)):
            for entry, (vw, vh) in (("bt709hip_decode_scaled_batch", VIEW), ("bt709hip_decode_half_batch", (W // 2, H // 2))):
                mixed = r.surfs(fmt, n=2, w=vw, h=vh, stride=vw * 8)
                mixed[0].format, mixed[1].format = first, second
                assert getattr(fake, entry)(r.dec, 2, f, a, mixed, None, 1) == _capi.ERR_INVALID_ARG, (entry, first, second)
    # OH = 65536 is one row too many, as for the BGRA8 view
    for probe in (fmt, 0):
        assert fake.bt709hip_decode_scaled(r.dec, f, a, r.surfs(probe, w=2, h=65536), None, 1) == _capi.ERR_UNSUPPORTED
    assert r.kernels(mark) == []
    assert fake.bt709hip_decode_scaled(r.dec, f, a, r.surfs(fmt, w=2, h=65535), None, 1) == 0 and len(r.kernels(mark)) == 1


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_new_refusals_and_their_place(fake, rig, fmt):
    """RGBA16F intermediate, SCALED_OVER, planes reaching 2 GiB: ERR_UNSUPPORTED with nothing launched, behind the usual validation
    (a bad pitch is still ERR_STRIDE) and beside the refusals the BGRA8 view meets in the same state."""
    r, e = rig, ELEM[fmt]
    assert r.set(OPT, 1) == 0
    mark = fake.fake_hip_log_size()
    log_mark = fake.fake_hip_log_size()
    states = [(_capi.OPT_SCALE_INTERMEDIATE, RGBA16F, _capi.FORMAT_BGRA8_SRGB)]
    if r.has_alpha:  # the option is an alpha decoder's
        states += [(_capi.OPT_SCALED_OVER, _capi.OVER_DESTINATION, _capi.OVER_OFF), (_capi.OPT_SCALED_OVER, 0x204060, _capi.OVER_OFF)]
    for opt, value, off in states:
        assert r.set(opt, value) == 0
        assert codes(four_calls(r, fmt)) == [_capi.ERR_UNSUPPORTED] * 4, (opt, value)
        assert codes(four_calls(r, fmt, stride=8)) == [_capi.ERR_STRIDE] * 4   # the usual validation comes first
        assert r.set(opt, off) == 0
    assert r.kernels(mark) == [] and fake.fake_hip_log_size() == log_mark     # nothing launched, nothing copied, nothing built
    # the old refusals stand in front: each state that refuses the BGRA8 view refuses the CHW view with the same code
    olds = [(_capi.OPT_CHROMA_LAYOUT, _capi.CHROMA_I420, _capi.CHROMA_NV12)]
    if r.has_alpha:
        olds += [(_capi.OPT_COMPOSITE_OVER, 0x102030, _capi.OVER_OFF), (_capi.OPT_UNPREMULTIPLY, 1, 0)]
    for opt, value, off in olds:
        assert r.set(opt, value) == 0
        assert r.set(_capi.OPT_SCALE_INTERMEDIATE, RGBA16F) == 0              # a new refusal's state on top: the code is the old one's
        assert codes(four_calls(r, fmt)) == codes(four_calls(r, 0)) == [_capi.ERR_UNSUPPORTED] * 4, opt
        assert r.set(_capi.OPT_SCALE_INTERMEDIATE, _capi.FORMAT_BGRA8_SRGB) == 0 and r.set(opt, off) == 0
    assert r.kernels(mark) == []
    # planes x OH x pitch reaching 2 GiB: one row fewer passes.  The kernels form offsets into the surface in 32 bits.
    planes, pitch = (4 if r.has_alpha else 3), 1 << 20
    rows = -(-(1 << 31) // (planes * pitch))  # the first OH at which the planes together reach 2^31 bytes
    assert planes * rows * pitch >= 1 << 31 > planes * (rows - 1) * pitch
    f, a = r.frames(), r.alphas()
    for entry in ("bt709hip_decode_scaled", "bt709hip_decode_scaled_batch"):
        call = lambda s: getattr(fake, entry)(*((r.dec, 1, f, a, s, None, 1) if entry.endswith("batch") else (r.dec, f, a, s, None, 1)))
        before = len(r.kernels(mark))
        assert call(r.surfs(fmt, w=16, h=rows, stride=pitch)) == _capi.ERR_UNSUPPORTED and len(r.kernels(mark)) == before, entry
        assert call(r.surfs(0, w=16, h=rows, stride=pitch)) == 0                # one BGRA8 plane of that shape fits
        assert call(r.surfs(fmt, w=16, h=rows - 1, stride=pitch)) == 0, entry
    # the half call (W, H % 4 == 0: an even OH): the first even OH that reaches the bound, and two rows fewer
    even = rows + rows % 2
    hf, ha = r.frames(w=32, h=2 * even), r.alphas(w=32, h=2 * even)
    before = len(r.kernels(mark))
    assert fake.bt709hip_decode_half(r.dec, hf, ha, r.surfs(fmt, w=16, h=even, stride=pitch), None, 1) == _capi.ERR_UNSUPPORTED
    assert len(r.kernels(mark)) == before
    hf, ha = r.frames(w=32, h=2 * even - 4), r.alphas(w=32, h=2 * even - 4)
    assert fake.bt709hip_decode_half(r.dec, hf, ha, r.surfs(fmt, w=16, h=even - 2, stride=pitch), None, 1) == 0
    assert r.kernels(mark)[-1][0] == SCALED


def test_graph_capture_takes_the_option_and_the_rescale(fake, rig):
    """Nothing is staged for a CHW view: the option can be set, and each call into each format issued, while a stream records."""
    lib, r = fake, rig
    mark, allocs = lib.fake_hip_log_size(), lib.fake_hip_allocations(0)
    g = C.c_void_p()
    f, a = r.frames(), r.alphas()
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    assert r.set(OPT, 1) == 0  # while the stream records
    targets = []
    for i, fmt in enumerate(FORMATS):
        view, half = r.surfs(fmt, w=VIEW[0], h=VIEW[1], base=i << 16), r.surfs(fmt, w=W // 2, h=H // 2, base=(i << 16) + (1 << 15))
        assert lib.bt709hip_decode_scaled(r.dec, f, a, view, r.stream, 0) == 0 and lib.bt709hip_decode_half(r.dec, f, a, half, r.stream, 0) == 0
        targets += [view[0].bgra, half[0].bgra]
    assert r.set(_capi.OPT_CHW_SCALE_R, cc.bits(3.0)) == 0
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0
    assert lib.fake_hip_log_size() == mark and lib.fake_hip_allocations(0) == allocs  # recorded, not run; nothing allocated or copied
    assert lib.bt709hip_graph_launch(r.ctx, g, r.stream) == 0 and lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    from test_fake_hip import log
    ops = log(lib, mark)
    assert [o[0].split(":")[0] for o in ops] == ["graph_launch"] + ["kernel"] * 6 and all(o[0] == SCALED for o in ops[1:]), ops
    assert [o[3] for o in ops[1:]] == targets
    assert lib.bt709hip_graph_destroy(r.ctx, g) == 0


# ------------------------------------------------------------------ the Python mirror

def test_python_mirror_on_the_fake_library(fake):
    ctx = mb.MetalRenderContext()
    h = C.c_void_p()
    assert fake.bt709hip_context_create(0, C.byref(h)) == 0
    ctx.lib, ctx.handle = fake, h.value
    mem = C.c_void_p()
    assert fake.bt709hip_malloc(ctx.handle, 1 << 22, C.byref(mem)) == 0
    try:
        dec = mb.MetalBT709Decoder()
        assert dec.scaledCHW is False and dec.setScaledCHW(True) and dec.scaledCHW is True  # kept before setup, like every option
        assert dec._options[_capi.OPT_SCALED_CHW] == 1
        dec.scaledCHW = False
        assert dec.scaledCHW is False
        dec.metalRenderContext = ctx
        assert dec.setupMetal()
        assert _get(fake, dec._handle, OPT) == 0

        def buffer(i=0):
            base = mem.value + i * W * H * 3 // 2
            b = mb.CVPixelBuffer(ctx, W, H, W, W, planes=(base, base + W * H))
            b.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
            b.setAttachment("TransferFunction", mb.kCVImageBufferTransferFunction_ITU_R_709_2)
            return b

        def texture(size, dtype, i=0):
            e = np.dtype(dtype).itemsize
            return mb.CHWTexture(ctx, size[0], size[1], dtype, ptr=mem.value + (1 << 21) + i * 4 * size[0] * size[1] * e)

        mark = fake.fake_hip_log_size()
        kernels = lambda: [o for o in __import__("test_fake_hip").log(fake, mark) if o[0].startswith("kernel:")]
        # off: the status the C call gives an unknown format, through _fail
        assert dec.decodeBT709Scaled(buffer(), texture(VIEW, "float16"), waitUntilCompleted=True) is False and dec.lastStatus == _capi.ERR_INVALID_ARG
        assert dec.decodeBT709ScaledBatch([buffer(0), buffer(1)], [texture(VIEW, "uint8", 0), texture(VIEW, "uint8", 1)]) is False
        assert dec.lastStatus == _capi.ERR_INVALID_ARG and kernels() == []
        # on, set on a live decoder: applied at once
        assert dec.setScaledCHW(True) and _get(fake, dec._handle, OPT) == 1 and dec.lastStatus == _capi.OK
        for dtype in ("uint8", "float16", "float32"):
            before = len(kernels())
            general, half = texture(VIEW, dtype), texture((W // 2, H // 2), dtype)
            assert dec.decodeBT709Scaled(buffer(), general, waitUntilCompleted=True), dec.lastStatus
            assert dec.decodeBT709Scaled(buffer(), half, waitUntilCompleted=True), dec.lastStatus  # exactly half: the half call
            batch = [texture(VIEW, dtype, i) for i in range(3)]
            assert dec.decodeBT709ScaledBatch([buffer(i) for i in range(3)], batch, waitUntilCompleted=True), dec.lastStatus
            halves = [texture((W // 2, H // 2), dtype, i) for i in range(3)]
            assert dec.decodeBT709ScaledBatch([buffer(i) for i in range(3)], halves, waitUntilCompleted=True), dec.lastStatus
            issued = kernels()[before:]
            assert [(k[0], k[2], k[3]) for k in issued] == [(SCALED, 1, general.ptr), (SCALED, 1, half.ptr), (SCALED, 3, batch[0].ptr), (SCALED, 3, halves[0].ptr)], issued
        # a refusal comes back as a status
        dec.resizeTexturePixelFormat = mb.MTLPixelFormatRGBA16Float
        assert dec.decodeBT709Scaled(buffer(), texture(VIEW, "float32")) is False and dec.lastStatus == _capi.ERR_UNSUPPORTED
        dec.release()
    finally:
        assert fake.bt709hip_free(ctx.handle, mem) == 0
        ctx.handle = None
        assert fake.bt709hip_context_destroy(h) == 0


# ------------------------------------------------------------------ the generated code

FMA = r"^\s*(v_(?:pk_)?(?:fma|fmac|fmamk|fmaak|mad|mac|madmk|madak)_(?:f32|f16|legacy|mix)\w*\s[^\n]*)"  # tests/test_host_cpu.py's class
CENTRE_NORM = r"v_fmamk_f32 v\d+, v\d+, 0x3b808081, v\d+|v_fmac_f32_e32 v\d+, 0x3b808081, v\d+"
LOG_INDEX = r"v_fmamk_f32 v\d+, v\d+, 0x5[23]800000, v\d+$|v_fmac_f32_e32 v\d+, 0x5[23]800000, v\d+$"


def test_isa_of_the_scaled_chw_kernels():
    """Thirty kernels, none spilled.  Each carries exactly the fused multiply-adds of its BGRA8 twin -- centre_norm's 1/255 and the
    log-bucket index -- so none sits on the normalisation; nothing packed in float32, no transcendental; per output row one buffer
    store per plane, of the width of the element and of no other; the float16 kernels convert with v_cvt_f16_f32."""
    from metalbt709decoder_amd import build
    asm = open(build.emit_asm()).read()
    body_of = lambda stem: dict(re.findall(r"^(_ZN5bt709\d+%sI\w+):[^\n]*\n(.*?)^\.Lfunc_end" % stem, asm, flags=re.S | re.M))
    chw, twins = body_of("decode_nv12_scaled_chw"), body_of("decode_nv12_scaled")
    assert len(chw) == 5 * 3 * 2 and len(twins) == 5 * 2
    store_of = {"1": "buffer_store_byte", "2": "buffer_store_short", "3": "buffer_store_dword"}
    classify = lambda body: sorted("norm" if re.match(CENTRE_NORM, l.strip()) else "index" if re.match(LOG_INDEX, l.strip()) else l.strip()
                                   for l in re.findall(FMA, body, flags=re.M))
    for name, body in chw.items():
        taps, elem, alpha, persistent = re.match(r"_ZN5bt70922decode_nv12_scaled_chwILi(\d)ELj(\d)ELb(\d)ELb(\d)E", name).groups()
        assert persistent == ("1" if taps in "012" else "0"), name  # the per-lane forms run the item loop, as their twins do
        twin = twins["_ZN5bt70918decode_nv12_scaledILi%sELb%sELb%sEEEvNS_12DecodeParamsE" % (taps, alpha, persistent)]
        fused = classify(body)
        assert set(fused) <= {"norm", "index"} and fused == classify(twin), (name, fused)
        assert not re.search(r"\bv_pk_(mul|add|fma)_f32|\bv_(log|exp)_f32|s_setreg|v_cvt_pkrtz", body), name
        assert "scratch_" not in body, name
        meta = re.search(r"\.name:\s+%s\b.*?\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), asm, flags=re.S)
        assert meta and int(meta.group(1)) == 0, name
        planes = 4 if alpha == "1" else 3
        rows = len(re.findall(r"^\s*buffer_store_dword ", twin, flags=re.M))  # the twin stores one word per output row
        assert rows in (2, 4), (name, rows)
        stores = re.findall(r"^\s*(buffer_store_\w+) ([^\n]*)", body, flags=re.M)
        assert [s[0] for s in stores] == [store_of[elem]] * (planes * rows), (name, [s[0] for s in stores])
        assert all(s[1].rstrip().endswith(" nt") for s in stores), name  # kScaledStoreAux: streaming, as the word's store
        assert len(re.findall(r"\bv_cvt_f16_f32", body)) == (planes * rows if elem == "2" else 0), name
