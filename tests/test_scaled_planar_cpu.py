"""Planar I420 frames through the fused decode + rescale (BT709HIP_OPT_SCALED_PLANAR = 24), the parts that need no GPU:
the ids and the option's domain on a context-less decoder, and -- on the shim built against the fake HIP runtime -- what the four
rescale calls return with the option off, that NV12 frames meet nothing new with it on, the routing of planar frames, validation,
the refusals that stay, batches, graph capture and the Python mirror; then the generated code of the twenty-four new kernels.

The fake runtime's launcher stands in for launch_decode_scaled and reports "decode_nv12_scaled" whatever it is handed, so a probe
(tests/native/scaled_planar_probe.cpp) sits in front of it and keeps the parameter block: what is asserted here is the PATH -- one
any-ratio launch per call -- and what selects the kernel inside the real launcher: chroma_layout, v_offset, the element type, the
alpha flag, the U planes' step.  The names the real launcher reports for them are asserted against its table's text here and on the
GPU (tests/test_scaled_planar_gpu.py), with the tap forms."""
import ctypes as C
import os
import re
import subprocess

import pytest

import abi_headers
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi
from test_chw_cpu import F16, F32, U8, Addressing, Rig, _get

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "metalbt709decoder_amd", "csrc")
OPT, LAYOUT, NV12, I420 = 24, _capi.OPT_CHROMA_LAYOUT, _capi.CHROMA_NV12, _capi.CHROMA_I420
SCALED = "kernel:decode_nv12_scaled"  # what the fake launcher reports for every any-ratio launch
W, H = Rig.W, Rig.H          # 64 x 16 frames
VIEW = (48, 10)              # a general view; the half view is W/2 x H/2
RGBA16F = _capi.FORMAT_RGBA16F


# ------------------------------------------------------------------ ids, ABI, option domain

@pytest.fixture(scope="module")
def lib():
    return mb.load_library()


def test_ids_agree_and_nothing_was_exported(lib):
    header = open(os.path.join(ROOT, "include", "bt709hip_ext.h")).read()
    assert int(re.search(r"#define\s+BT709HIP_OPT_SCALED_PLANAR\s+(\d+)", header).group(1)) == OPT == _capi.OPT_SCALED_PLANAR
    assert "ids 13, 20, 21 and 23 are no option" in header
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    for word in ("BT709HIP_OPT_SCALED_PLANAR", "setScaledPlanar", "scaledPlanar()"):
        assert word in hpp, word
    comment = re.search(r"/\* PLANAR FRAMES INTO THE RESCALES.*?\*/", header, flags=re.S).group(0)
    for word in ("bt709hip_decode_scaled", "bt709hip_decode_half", "byte for byte", "ratio 2.0", "graph capture", "BT709HIP_ERR_STRIDE", "2 GiB", "W % 8 == 0",
                 "BT709HIP_SCALED_TAPS_SHARED is not built", "BT709HIP_OPT_SCALE_INTERMEDIATE", "BT709HIP_OPT_SCALED_OVER", "NOT covered", "decode_i420_scaled_chw<f16,alpha>"):
        assert word in comment, word
    for section in (r"/\* BT709HIP_OPT_CHROMA_LAYOUT\..*?\*/", r"/\* PLANAR CHW VIEWS.*?\*/"):  # the two NOT-covered lists point at the new section
        assert "BT709HIP_OPT_SCALED_PLANAR" in re.search(section, header, flags=re.S).group(0), section
    # the names the real launcher reports, in its table's text
    table = open(os.path.join(CSRC, "bt709_rescale_planar.hip")).read()
    for piece in ('"decode_i420_scaled" bare', '"decode_i420_scaled_chw<u8" in_brackets ">"', '"decode_i420_scaled_chw<f16" in_brackets ">"',
                  '"decode_i420_scaled_chw<f32" in_brackets ">"', 'name(",alpha", "<alpha>")', 'name("", "")'):
        assert piece in table, piece
    # an option, not an export: the ABI and the export list are what they were
    assert lib.bt709hip_abi_version() == 504 == _capi.ABI_VERSION
    assert int(re.search(r"#define\s+BT709HIP_VERSION\s+(\d+)", abi_headers.text()).group(1)) == 504
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
        assert _get(lib, dec, _capi.OPT_SCALED_CHW) == 0 and _get(lib, dec, LAYOUT) == NV12
        for unknown in (23, 25, 99):
            assert lib.bt709hip_decoder_set_option(dec, unknown, 0) == _capi.ERR_INVALID_ARG
            assert lib.bt709hip_decoder_get_option(dec, unknown, C.byref(C.c_int())) == _capi.ERR_INVALID_ARG
    finally:
        lib.bt709hip_decoder_destroy(dec)


# ------------------------------------------------------------------ the shim on the fake HIP runtime, a probe in front of the launcher

class Probe(C.Structure):  # tests/native/scaled_planar_probe.cpp scaled_planar_probe_record
    _fields_ = [("calls", C.c_int32), ("frames", C.c_int32), ("has_alpha", C.c_int32), ("uniform", C.c_int32),
                ("in_align", C.c_uint32), ("chroma_layout", C.c_uint32), ("chw_elem", C.c_uint32), ("scale_f16", C.c_uint32), ("over_mode", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("out_width", C.c_uint32), ("out_height", C.c_uint32), ("y_stride", C.c_uint32),
                ("cbcr_stride", C.c_uint32), ("alpha_stride", C.c_uint32), ("v_offset", C.c_uint64),
                ("step_y", C.c_int64), ("step_cbcr", C.c_int64), ("step_alpha", C.c_int64), ("step_out", C.c_int64),
                ("first_y", C.c_void_p), ("first_cbcr", C.c_void_p), ("second_cbcr", C.c_void_p), ("params_bytes", C.c_uint32), ("reserved", C.c_uint32)]


@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    """The shim on the fake runtime with the probe in front of the fake launch_decode_scaled: fake_hip.cpp is compiled with its
    launcher renamed, the probe defines the name the shim calls."""
    from test_fake_hip import CXX, FAKE, SHIM_SOURCES, FakeOp
    d = tmp_path_factory.mktemp("fake_scaled_planar")
    obj, so = str(d / "fake_hip.o"), str(d / "libbt709hip_fake.so")
    r = subprocess.run(CXX + ["-fPIC", "-c", "-Dlaunch_decode_scaled=fake_hip_launch_decode_scaled", os.path.join(FAKE, "fake_hip.cpp"), "-o", obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    sources = [s for s in SHIM_SOURCES if not s.endswith("fake_hip.cpp")] + [os.path.join(HERE, "native", "scaled_planar_probe.cpp"), obj]
    r = subprocess.run(CXX + ["-shared", "-fPIC", "-I" + CSRC] + sources + ["-o", so, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_allocations.restype = C.c_uint64
    lib.fake_hip_last_addressing.argtypes = [C.POINTER(Addressing)]
    lib.scaled_planar_probe_last.argtypes = [C.POINTER(Probe)]
    lib.fake_hip_set_device_count(1)
    return lib


@pytest.fixture(params=[0, 1], ids=["opaque", "alpha"])
def rig(fake, request):
    r = Rig(fake, has_alpha=request.param)
    assert fake.bt709hip_decoder_setup(r.dec) == 0
    yield r
    r.close()


def probe(lib):
    p = Probe()
    lib.scaled_planar_probe_last(C.byref(p))
    return p


def four_calls(r, fmt=0, n=3, planar=True, chroma_stride=None, which=(0, 1, 2, 3), **kw):
    """The four entry points (or those of `which`) on `n` frames -- planar: U then V at pitch W/2 (or chroma_stride); else NV12 -- the
    single-frame ones on the first: [(label, return code, the probe's record after the call)].  kw: Rig.surfs' for BOTH views."""
    lib = r.lib
    f, a = r.frames(n, chroma_stride=chroma_stride or (W // 2 if planar else W)), r.alphas(n)
    half, view = r.surfs(fmt, n=n, w=W // 2, h=H // 2, **kw), r.surfs(fmt, n=n, w=VIEW[0], h=VIEW[1], **kw)
    calls = [("half", lambda: lib.bt709hip_decode_half(r.dec, f, a, half, None, 1)), ("half_batch", lambda: lib.bt709hip_decode_half_batch(r.dec, n, f, a, half, None, 1)),
             ("scaled", lambda: lib.bt709hip_decode_scaled(r.dec, f, a, view, None, 1)), ("scaled_batch", lambda: lib.bt709hip_decode_scaled_batch(r.dec, n, f, a, view, None, 1))]
    return [(calls[i][0], calls[i][1](), probe(lib)) for i in which]


def codes(calls):
    return [c[1] for c in calls]


def test_option_off_the_four_calls_refuse_planar_frames_as_before(fake, rig):
    r = rig
    assert r.set(LAYOUT, I420) == 0
    mark = fake.fake_hip_log_size()
    assert codes(four_calls(r)) == [_capi.ERR_UNSUPPORTED] * 4
    assert codes(four_calls(r, planar=False)) == [_capi.ERR_UNSUPPORTED] * 4  # an NV12-shaped frame is a padded planar one
    assert r.set(OPT, 1) == 0 and r.set(OPT, 0) == 0  # switched on and off again: the same
    assert codes(four_calls(r)) == [_capi.ERR_UNSUPPORTED] * 4
    assert codes(four_calls(r, chroma_stride=W // 2 - 1)) == [_capi.ERR_STRIDE] * 4  # behind the usual validation
    assert fake.fake_hip_log_size() == mark
    assert r.set(LAYOUT, NV12) == 0


def test_option_on_nv12_frames_meet_the_kernels_they_met(fake, rig):
    r = rig
    issued = []
    for value in (0, 1):
        assert r.set(OPT, value) == 0
        mark = fake.fake_hip_log_size()
        calls = four_calls(r, planar=False)
        assert codes(calls) == [0] * 4
        issued.append([(k[0], k[2]) for k in r.kernels(mark)])
        last = calls[-1][2]
        assert (last.chroma_layout, last.v_offset, last.cbcr_stride) == (0, 0, W) and last.in_align >= 4
    assert issued[0] == issued[1] and len(issued[0]) == 4
    assert [nm for nm, _ in issued[1][2:]] == [SCALED] * 2 and all(nm.startswith("kernel:decode_nv12_half") for nm, _ in issued[1][:2]), issued
    assert r.set(OPT, 0) == 0


@pytest.mark.parametrize("fmt", [0, U8, F16, F32], ids=["bgra8", "u8", "f16", "f32"])
def test_option_on_planar_frames_take_one_any_ratio_launch_per_call(fake, rig, fmt):
    """Each of the four calls -- the half calls too -- is ONE launch of the any-ratio launcher, handed the layout, the V plane's
    offset, the element type and the alpha flag: what its table selects decode_i420_scaled[_chw<...>] by."""
    r, n = rig, 3
    assert r.set(LAYOUT, I420) == 0 and r.set(OPT, 1) == 0 and r.set(_capi.OPT_SCALED_CHW, 1 if fmt else 0) == 0
    mark = fake.fake_hip_log_size()
    before = probe(fake).calls
    calls = four_calls(r, fmt, n)
    assert codes(calls) == [0] * 4, calls
    assert [(k[0], k[2]) for k in r.kernels(mark)] == [(SCALED, 1), (SCALED, n), (SCALED, 1), (SCALED, n)]
    assert [c[2].calls for c in calls] == [before + i for i in (1, 2, 3, 4)]
    for (label, _, p), frames, (ow, oh) in zip(calls, (1, n, 1, n), ((W // 2, H // 2),) * 2 + (VIEW,) * 2):
        assert (p.chroma_layout, p.v_offset, p.cbcr_stride) == (1, (H // 2) * (W // 2), W // 2), label
        assert (p.frames, p.has_alpha, p.chw_elem, p.scale_f16, p.over_mode) == (frames, r.has_alpha, {0: 0, U8: 1, F16: 2, F32: 3}[fmt], 0, 0), label
        assert (p.width, p.height, p.out_width, p.out_height, p.params_bytes) == (W, H, ow, oh, 1288), label
        assert p.in_align >= 4  # the luma and alpha planes'; the chroma planes' alignment is the launcher's to work out from the block
    info = _capi.ScaledLaunchInfo()
    assert fake.bt709hip_last_scaled_launch_info(C.byref(info)) == 0 and info.grid[2] == n
    # a padded planar frame (chroma rows W bytes apart): V follows from the pitch
    p = four_calls(r, fmt, n, chroma_stride=W, which=(3,))[0][2]
    assert (p.chroma_layout, p.v_offset, p.cbcr_stride) == (1, (H // 2) * W, W)
    assert r.set(LAYOUT, NV12) == 0 and r.set(OPT, 0) == 0 and r.set(_capi.OPT_SCALED_CHW, 0) == 0


def test_validation_is_the_planar_decodes(fake, rig):
    r = rig
    assert r.set(LAYOUT, I420) == 0 and r.set(OPT, 1) == 0
    mark = fake.fake_hip_log_size()
    assert codes(four_calls(r, chroma_stride=W // 2 - 1)) == [_capi.ERR_STRIDE] * 4
    assert r.kernels(mark) == []
    assert codes(four_calls(r, chroma_stride=W // 2)) == [0] * 4 and len(r.kernels(mark)) == 4
    f, a = r.frames(2, chroma_stride=W // 2), r.alphas(2)
    # the half calls want exactly W/2 x H/2, and W, H % 4 == 0
    for bad in ((W // 2 + 2, H // 2), VIEW):
        s = r.surfs(0, n=2, w=bad[0], h=bad[1])
        assert fake.bt709hip_decode_half(r.dec, f, a, s, None, 1) == fake.bt709hip_decode_half_batch(r.dec, 2, f, a, s, None, 1) == _capi.ERR_SIZE_MISMATCH
    assert fake.bt709hip_decode_half(r.dec, r.frames(w=66, h=16, chroma_stride=33), r.alphas(w=66, h=16), r.surfs(0, w=33, h=8), None, 1) == _capi.ERR_ODD_DIMENSIONS
    # one geometry per batch: the chroma pitch too
    f[1].cbcr_stride = W // 2 + 2
    assert fake.bt709hip_decode_scaled_batch(r.dec, 2, f, a, r.surfs(0, n=2, w=VIEW[0], h=VIEW[1]), None, 1) == _capi.ERR_SIZE_MISMATCH
    f = r.frames(1, chroma_stride=W // 2)
    # OH = 65536 is one row too many, as for NV12 frames
    before = len(r.kernels(mark))
    assert fake.bt709hip_decode_scaled(r.dec, f, r.alphas(), r.surfs(0, w=2, h=65536), None, 1) == _capi.ERR_UNSUPPORTED and len(r.kernels(mark)) == before
    assert fake.bt709hip_decode_scaled(r.dec, f, r.alphas(), r.surfs(0, w=2, h=65535), None, 1) == 0
    # every plane on its own under 2 GiB: a U plane of (H/2) x pitch = 2^31 bytes is refused; two rows fewer pass, U and V together beyond 2 GiB
    pitch = 1 << 20
    for h, rc in ((4096, _capi.ERR_UNSUPPORTED), (4092, 0)):
        tall, talpha = r.frames(w=W, h=h, chroma_stride=pitch), r.alphas(w=W, h=h)
        before = len(r.kernels(mark))
        assert fake.bt709hip_decode_scaled(r.dec, tall, talpha, r.surfs(0, w=VIEW[0], h=VIEW[1]), None, 1) == rc, h
        assert len(r.kernels(mark)) == before + (1 if rc == 0 else 0)
    assert probe(fake).v_offset == 2046 * pitch and 2 * 2046 * pitch > 1 << 31
    assert r.set(LAYOUT, NV12) == 0 and r.set(OPT, 0) == 0


def test_the_refusals_that_stay(fake, rig):
    """RGBA16F intermediate and SCALED_OVER under planar frames: ERR_UNSUPPORTED with nothing launched, built or copied, behind the
    usual validation (a bad pitch is still ERR_STRIDE); NV12 frames in the same state are served as ever; RGBA16F targets of the 1:1
    decode stay refused."""
    r = rig
    assert r.set(OPT, 1) == 0
    states = [(_capi.OPT_SCALE_INTERMEDIATE, RGBA16F, _capi.FORMAT_BGRA8_SRGB)]
    if r.has_alpha:  # the option is an alpha decoder's
        states += [(_capi.OPT_SCALED_OVER, _capi.OVER_DESTINATION, _capi.OVER_OFF), (_capi.OPT_SCALED_OVER, 0x204060, _capi.OVER_OFF)]
    for opt, value, off in states:
        assert r.set(opt, value) == 0 and r.set(LAYOUT, I420) == 0
        log_mark = fake.fake_hip_log_size()
        assert codes(four_calls(r)) == [_capi.ERR_UNSUPPORTED] * 4, (opt, value)
        assert codes(four_calls(r, chroma_stride=W // 2 - 1)) == [_capi.ERR_STRIDE] * 4   # the usual validation comes first
        assert fake.fake_hip_log_size() == log_mark                                        # nothing launched, nothing copied, nothing built
        assert r.set(LAYOUT, NV12) == 0
        assert codes(four_calls(r, planar=False)) == [0] * 4                               # the option changes nothing for NV12 frames
        assert r.set(opt, off) == 0
    # the old refusals of the rescales are met behind the planar one and keep their code
    if r.has_alpha:
        for opt, value, off in ((_capi.OPT_COMPOSITE_OVER, 0x102030, _capi.OVER_OFF), (_capi.OPT_UNPREMULTIPLY, 1, 0)):
            assert r.set(opt, value) == 0 and r.set(LAYOUT, I420) == 0
            mark = fake.fake_hip_log_size()
            assert codes(four_calls(r)) == [_capi.ERR_UNSUPPORTED] * 4 and r.kernels(mark) == []
            assert r.set(opt, off) == 0 and r.set(LAYOUT, NV12) == 0
    # CHW views of planar frames want BT709HIP_OPT_SCALED_CHW as ever: without it a CHW surface is no format of the rescales
    assert r.set(LAYOUT, I420) == 0
    mark = fake.fake_hip_log_size()
    unknown = codes(four_calls(r, 7))
    assert all(rc != 0 for rc in unknown) and codes(four_calls(r, F16)) == unknown and r.kernels(mark) == []
    # an RGBA16F target of the 1:1 decode
    f = r.frames(1, chroma_stride=W // 2)
    assert r.decode(f, r.surfs(RGBA16F)) == _capi.ERR_UNSUPPORTED and r.kernels(mark) == []
    assert r.decode(f, r.surfs(0)) == 0 and len(r.kernels(mark)) == 1
    assert r.set(LAYOUT, NV12) == 0 and r.set(OPT, 0) == 0


def test_batches_pointer_table_and_even_spacing(fake, rig):
    """An evenly spaced batch is one whose U planes are evenly spaced (V follows from cbcr): any count in one launch, the U step in
    the block; anything else goes through the pointer table, 32 at most."""
    r = rig
    assert r.set(LAYOUT, I420) == 0 and r.set(OPT, 1) == 0
    for entry, (vw, vh) in (("bt709hip_decode_scaled_batch", VIEW), ("bt709hip_decode_half_batch", (W // 2, H // 2))):
        fn = getattr(fake, entry)
        for n, uneven, step in ((2, False, None), (32, True, 16), (33, False, 16), (40, False, 48)):
            f = r.frames(n, chroma_stride=W // 2, uneven=uneven, step=step)
            s = r.surfs(0, n=n, w=vw, h=vh)
            mark = fake.fake_hip_log_size()
            assert fn(r.dec, n, f, r.alphas(n, step=step), s, None, 1) == 0, (entry, n)
            issued = r.kernels(mark)
            assert len(issued) == 1 and issued[0][0] == SCALED and issued[0][2] == n and issued[0][3] == s[0].bgra, (entry, n, issued)
            uniform, frames, steps = r.addressing()
            p = probe(fake)
            assert (uniform, frames, p.uniform, p.chroma_layout, p.v_offset) == (0 if uneven else 1, n, 0 if uneven else 1, 1, (H // 2) * (W // 2)), (entry, n)
            assert p.first_cbcr == f[0].cbcr and p.second_cbcr == f[1].cbcr
            if not uneven:
                want = W * H * 3 // 2 if step is None else step
                assert steps[0] == steps[1] == p.step_cbcr == want == f[1].cbcr - f[0].cbcr, (entry, n, steps)
        mark = fake.fake_hip_log_size()
        assert fn(r.dec, 33, r.frames(33, chroma_stride=W // 2, step=16, uneven=True), r.alphas(33, step=16), r.surfs(0, n=33, w=vw, h=vh, step=64), None, 1) == _capi.ERR_UNSUPPORTED
        assert r.kernels(mark) == []
    assert r.set(LAYOUT, NV12) == 0 and r.set(OPT, 0) == 0


def test_graph_capture_takes_the_option_and_the_rescale(fake, rig):
    """Nothing is staged for planar frames: the option can be set, and the calls issued, while a stream records."""
    lib, r = fake, rig
    assert r.set(LAYOUT, I420) == 0
    mark, allocs = lib.fake_hip_log_size(), lib.fake_hip_allocations(0)
    g = C.c_void_p()
    f, a = r.frames(chroma_stride=W // 2), r.alphas()
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    assert r.set(OPT, 1) == 0  # while the stream records
    view, half = r.surfs(0, w=VIEW[0], h=VIEW[1]), r.surfs(0, w=W // 2, h=H // 2, base=1 << 15)
    assert lib.bt709hip_decode_scaled(r.dec, f, a, view, r.stream, 0) == 0 and lib.bt709hip_decode_half(r.dec, f, a, half, r.stream, 0) == 0
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0
    assert lib.fake_hip_log_size() == mark and lib.fake_hip_allocations(0) == allocs  # recorded, not run; nothing allocated or copied
    assert lib.bt709hip_graph_launch(r.ctx, g, r.stream) == 0 and lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    from test_fake_hip import log
    ops = log(lib, mark)
    assert [o[0] for o in ops] == ["graph_launch", SCALED, SCALED] and [o[3] for o in ops[1:]] == [view[0].bgra, half[0].bgra], ops
    assert lib.bt709hip_graph_destroy(r.ctx, g) == 0
    assert r.set(LAYOUT, NV12) == 0 and r.set(OPT, 0) == 0


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
        assert dec.scaledPlanar is False and dec.setScaledPlanar(True) and dec.scaledPlanar is True  # kept before setup, like every option
        assert dec._options[_capi.OPT_SCALED_PLANAR] == 1
        dec.scaledPlanar = False
        assert dec.scaledPlanar is False
        dec.metalRenderContext = ctx
        assert dec.setupMetal()
        assert _get(fake, dec._handle, OPT) == 0

        def buffer(i=0, planar=True):
            base = mem.value + i * W * H * 3 // 2
            b = mb.CVPixelBuffer(ctx, W, H, W, W // 2 if planar else W, planes=(base, base + W * H), planar=planar)
            b.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
            b.setAttachment("TransferFunction", mb.kCVImageBufferTransferFunction_ITU_R_709_2)
            return b

        texture = lambda size, i=0: mb.BGRATexture(ctx, size[0], size[1], ptr=mem.value + (1 << 21) + i * 4 * size[0] * size[1])
        mark = fake.fake_hip_log_size()
        kernels = lambda: [o for o in __import__("test_fake_hip").log(fake, mark) if o[0].startswith("kernel:")]
        # off: the planar buffer sets the layout, the rescale refuses
        assert dec.decodeBT709Scaled(buffer(), texture(VIEW), waitUntilCompleted=True) is False and dec.lastStatus == _capi.ERR_UNSUPPORTED
        assert dec.decodeBT709ScaledBatch([buffer(0), buffer(1)], [texture(VIEW, 0), texture(VIEW, 1)]) is False and dec.lastStatus == _capi.ERR_UNSUPPORTED
        assert kernels() == [] and _get(fake, dec._handle, LAYOUT) == I420
        # on, set on a live decoder: applied at once
        assert dec.setScaledPlanar(True) and _get(fake, dec._handle, OPT) == 1 and dec.lastStatus == _capi.OK
        general, half = texture(VIEW), texture((W // 2, H // 2))
        assert dec.decodeBT709Scaled(buffer(), general, waitUntilCompleted=True), dec.lastStatus
        assert dec.decodeBT709Scaled(buffer(), half, waitUntilCompleted=True), dec.lastStatus  # exactly half: the half call
        batch = [texture(VIEW, i) for i in range(3)]
        assert dec.decodeBT709ScaledBatch([buffer(i) for i in range(3)], batch, waitUntilCompleted=True), dec.lastStatus
        assert [(k[0], k[2], k[3]) for k in kernels()] == [(SCALED, 1, general.ptr), (SCALED, 1, half.ptr), (SCALED, 3, batch[0].ptr)]
        p = probe(fake)
        assert (p.chroma_layout, p.v_offset, p.cbcr_stride, p.step_cbcr) == (1, (H // 2) * (W // 2), W // 2, W * H * 3 // 2)
        # an NV12 buffer on the same decoder: the layout follows the buffer, the kernels are the NV12 calls'
        assert dec.decodeBT709Scaled(buffer(planar=False), general, waitUntilCompleted=True) and probe(fake).chroma_layout == 0
        # a refusal that stays comes back as a status
        dec.resizeTexturePixelFormat = mb.MTLPixelFormatRGBA16Float
        assert dec.decodeBT709Scaled(buffer(), general) is False and dec.lastStatus == _capi.ERR_UNSUPPORTED
        dec.release()
    finally:
        assert fake.bt709hip_free(ctx.handle, mem) == 0
        ctx.handle = None
        assert fake.bt709hip_context_destroy(h) == 0


# ------------------------------------------------------------------ the generated code

FMA = r"^\s*(v_(?:pk_)?(?:fma|fmac|fmamk|fmaak|mad|mac|madmk|madak)_(?:f32|f16|legacy|mix)\w*\s[^\n]*)"  # tests/test_host_cpu.py's class
CENTRE_NORM = r"v_fmamk_f32 v\d+, v\d+, 0x3b808081, v\d+|v_fmac_f32_e32 v\d+, 0x3b808081, v\d+"
LOG_INDEX = r"v_fmamk_f32 v\d+, v\d+, 0x5[23]800000, v\d+$|v_fmac_f32_e32 v\d+, 0x5[23]800000, v\d+$"


def test_isa_of_the_planar_rescale_kernels():
    """Twenty-four kernels (three tap forms x four targets x opaque / alpha), none spilled.  Each carries exactly the fused multiply-adds
    and the stores of its NV12 twin (the arithmetic and both epilogues are one text).  The front end: the per-lane byte form makes as
    many byte loads as NV12's; the by-wave form three byte loads per fetched row where NV12 makes a byte and a 2-byte load; the wide
    form nothing but 8-byte loads -- three planes' windows where NV12 has two -- and no kernel a 2-byte or a lone 4-byte load."""
    from metalbt709decoder_amd import build
    asm = open(build.emit_asm()).read()
    body_of = lambda stem: dict(re.findall(r"^(_ZN5bt709\d+%sI\w+):[^\n]*\n(.*?)^\.Lfunc_end" % stem, asm, flags=re.S | re.M))
    planar, twins, chw_twins = body_of("decode_i420_scaled"), body_of("decode_nv12_scaled"), body_of("decode_nv12_scaled_chw")
    assert len(planar) == 3 * 4 * 2
    classify = lambda body: sorted("norm" if re.match(CENTRE_NORM, l.strip()) else "index" if re.match(LOG_INDEX, l.strip()) else l.strip()
                                   for l in re.findall(FMA, body, flags=re.M))
    count = lambda body, what: len(re.findall(r"^\s*%s " % what, body, flags=re.M))
    loads = lambda body: set(re.findall(r"^\s*(buffer_load_\w+) ", body, flags=re.M))
    for name, body in planar.items():
        taps, elem, alpha, persistent = re.match(r"_ZN5bt70918decode_i420_scaledILi(\d)ELj(\d)ELb(\d)ELb(\d)E", name).groups()
        assert taps in "024" and persistent == ("0" if taps == "4" else "1"), name  # BYTES, WIDE, ONCE; the per-lane forms run the item loop
        twin = (twins["_ZN5bt70918decode_nv12_scaledILi%sELb%sELb%sEEEvNS_12DecodeParamsE" % (taps, alpha, persistent)] if elem == "0" else
                chw_twins["_ZN5bt70922decode_nv12_scaled_chwILi%sELj%sELb%sELb%sEEEvNS_12DecodeParamsE" % (taps, elem, alpha, persistent)])
        fused = classify(body)
        assert set(fused) <= {"norm", "index"} and fused == classify(twin), (name, fused)
        assert not re.search(r"\bv_pk_(mul|add|fma)_f32|\bv_(log|exp)_f32|s_setreg|v_cvt_pkrtz", body), name
        assert "scratch_" not in body, name
        meta = re.search(r"\.name:\s+%s\b.*?\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), asm, flags=re.S)
        assert meta and int(meta.group(1)) == 0, name
        stores = lambda b: re.findall(r"^\s*(buffer_store_\w+) [^\n]*?( nt)?$", b, flags=re.M)
        assert stores(body) == stores(twin) and all(nt for _, nt in stores(body)), name
        planes_in = 4 if alpha == "1" else 3  # Y, U, V and alpha; the twin reads Y, CbCr and alpha
        if taps == "0":
            assert loads(body) == {"buffer_load_ubyte"} and count(body, "buffer_load_ubyte") == count(twin, "buffer_load_ubyte"), name
        elif taps == "4":
            assert loads(body) == {"buffer_load_ubyte"}, name
            assert count(body, "buffer_load_ubyte") * (planes_in - 1) == (count(twin, "buffer_load_ubyte") + count(twin, "buffer_load_ushort")) * planes_in, name
        else:
            assert loads(body) == {"buffer_load_dwordx2"} == loads(twin), name
            assert count(body, "buffer_load_dwordx2") * (planes_in - 1) == count(twin, "buffer_load_dwordx2") * planes_in, name
