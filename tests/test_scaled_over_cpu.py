"""BT709HIP_OPT_SCALED_OVER, the parts that need no GPU: the option and its refusals on a context-less decoder,
its independence of BT709HIP_OPT_COMPOSITE_OVER, the constants of the four bindings, the Python mirror, the shim's routing on
the fake HIP runtime, and the bar of the GPU tap-form cases -- the blend must show -- on the oracle's arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_headers
import metalbt709decoder_amd as mb
import over_cases as oc
import scaled_over_cases as sc
from metalbt709decoder_amd import _capi
from test_over_cpu import FakeRig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT, OPT9 = _capi.OPT_SCALED_OVER, _capi.OPT_COMPOSITE_OVER


@pytest.fixture(scope="module")
def lib():
    return mb.load_library()


def _bare_decoder(lib, has_alpha):
    h = C.c_void_p()
    assert lib.bt709hip_decoder_create(None, mb.MetalBT709GammaApple, has_alpha, C.byref(h)) == _capi.OK
    return h


def _get(lib, dec, opt=OPT):
    v = C.c_int(-12345)
    assert lib.bt709hip_decoder_get_option(dec, opt, C.byref(v)) == _capi.OK
    return v.value


def test_option_round_trip_and_refusals(lib):
    """A decoder without a context: the option is a plain property with option 9's domain, nothing touches a device."""
    dec = _bare_decoder(lib, 1)
    try:
        assert _get(lib, dec) == -1  # off
        for held in (-2, 0, 0xFFFFFF, 0x123456, -1, 0x00FF00):
            assert lib.bt709hip_decoder_set_option(dec, OPT, held) == _capi.OK
            assert _get(lib, dec) == held
            for bad in (-3, 0x1000000, -(1 << 31), (1 << 31) - 1):
                assert lib.bt709hip_decoder_set_option(dec, OPT, bad) == _capi.ERR_INVALID_ARG
                assert _get(lib, dec) == held  # a refused value leaves the option as it was
    finally:
        lib.bt709hip_decoder_destroy(dec)
    opaque = _bare_decoder(lib, 0)
    try:
        for value in (-2, 0, 0xFFFFFF):
            assert lib.bt709hip_decoder_set_option(opaque, OPT, value) == _capi.ERR_UNSUPPORTED  # nothing to composite
            assert _get(lib, opaque) == -1
        assert lib.bt709hip_decoder_set_option(opaque, OPT, -3) == _capi.ERR_INVALID_ARG
    finally:
        lib.bt709hip_decoder_destroy(opaque)


def test_the_two_over_options_are_independent(lib):
    dec = _bare_decoder(lib, 1)
    try:
        held = -1
        for nine, ten in ((0x102030, -2), (-2, 0xA0B0C0), (-1, 0), (0, -1), (-1, -1)):
            assert lib.bt709hip_decoder_set_option(dec, OPT9, nine) == _capi.OK
            assert (_get(lib, dec, OPT9), _get(lib, dec)) == (nine, held)  # setting 9 leaves 10 alone
            held = ten
            assert lib.bt709hip_decoder_set_option(dec, OPT, ten) == _capi.OK
            assert (_get(lib, dec, OPT9), _get(lib, dec)) == (nine, ten)
            assert lib.bt709hip_decoder_set_option(dec, OPT, -3) == _capi.ERR_INVALID_ARG
            assert (_get(lib, dec, OPT9), _get(lib, dec)) == (nine, ten)
    finally:
        lib.bt709hip_decoder_destroy(dec)


def test_constants_agree_across_the_bindings(lib):
    """One more option value, the named values of option 9, no export: the header, the ctypes twin, the C++ host and the
    Objective-C class extension."""
    header = open(os.path.join(ROOT, "include", "bt709hip_ext.h")).read()
    assert int(re.search(r"\bBT709HIP_OPT_SCALED_OVER\s*=\s*(\d+)", header).group(1)) == 10 == _capi.OPT_SCALED_OVER
    assert _capi.OPT_SCALED_OVER != _capi.OPT_COMPOSITE_OVER
    assert (_capi.OVER_OFF, _capi.OVER_DESTINATION) == (-1, -2) == (oc.OVER_OFF, oc.OVER_DESTINATION)
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    assert re.search(r"setScaledCompositeOver\(int \w+\) \{ return setOption\(BT709HIP_OPT_SCALED_OVER, \w+\); \}", hpp)
    assert re.search(r"int scaledCompositeOver\(\) const \{\s*int background = BT709HIP_OVER_OFF;", hpp)
    objc = open(os.path.join(ROOT, "objc", "MetalBT709Decoder+HIP.h")).read()
    assert "@property (nonatomic, assign) int hipScaledCompositeOver;" in objc
    impl = open(os.path.join(ROOT, "objc", "MetalBT709Decoder+HIP.m")).read()
    assert "bt709hip_decoder_set_option(_hipDecoder, BT709HIP_OPT_SCALED_OVER, self.hipScaledCompositeOver)" in impl
    assert "_hipScaledCompositeOverSet ? _hipScaledCompositeOver : BT709HIP_OVER_OFF" in impl  # an unset int property is not "over black"
    # no export, no ABI bump
    assert lib.bt709hip_abi_version() == 504 == _capi.ABI_VERSION
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103


def test_python_mirror_maps_the_three_forms():
    d = mb.MetalBT709Decoder()
    d.hasAlphaChannel = True
    assert d.scaledCompositeOver is None
    for value, word in (("destination", -2), ((0, 0, 0), 0), ((255, 255, 255), 0xFFFFFF), ((1, 2, 3), 0x010203), (None, -1)):
        d.scaledCompositeOver = value  # before setupMetal: applied at setup, like every option
        assert d._options[OPT] == word
        assert d.scaledCompositeOver == value
        assert OPT9 not in d._options and d.compositeOver is None  # a value of its own
    for bad in ("colour", (0, 0, 256), (-1, 0, 0)):
        with pytest.raises(ValueError):
            d.scaledCompositeOver = bad
    assert d.scaledCompositeOver is None
    d.compositeOver = (9, 8, 7)
    d.scaledCompositeOver = "destination"
    assert (d.compositeOver, d.scaledCompositeOver) == ((9, 8, 7), "destination")
    opaque = mb.MetalBT709Decoder()
    opaque.scaledCompositeOver = None  # nothing to switch off: setupMetal must not hand the option to a decoder without alpha
    assert OPT not in opaque._options


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_scaled_over") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_set_device_count(1)
    return lib


@pytest.fixture()
def fake_rig(fake):
    r = FakeRig(fake)
    yield r
    r.close()


def _set(r, opt, value):
    return r.lib.bt709hip_decoder_set_option(r.dec, opt, value)


ENTRIES = ("bt709hip_decode_half", "bt709hip_decode_scaled")


def test_shim_launches_the_rescale_paths_under_option_10_alone(fake, fake_rig):
    """Option 10 on: each of the four rescale entry points launches exactly one kernel, the any-ratio one (bt709hip_decode_half
    too: there is no 2:1 over kernel) -- after the usual validation.  Option 9 on and 10 off: the refusal stays.  Both on: the
    rescale launches under 10 and the 1:1 decode under 9."""
    lib, r = fake, fake_rig
    s, half, scaled = r.surfs(), r.surfs(r.w // 2, r.h // 2), r.surfs(48, 10)
    for value in (-2, 0, 0xFFFFFF):
        assert _set(r, OPT, value) == 0
        for entry, out in zip(ENTRIES, (half, scaled)):
            mark = lib.fake_hip_log_size()
            assert getattr(lib, entry)(r.dec, r.frames, r.alphas, out, None, 1) == 0
            assert [k[0] for k in r.kernels(mark)] == ["kernel:decode_nv12_scaled"]
            mark = lib.fake_hip_log_size()
            assert getattr(lib, entry + "_batch")(r.dec, r.n, r.frames, r.alphas, out, None, 1) == 0
            assert [(k[0], k[2]) for k in r.kernels(mark)] == [("kernel:decode_nv12_scaled", r.n)]
            # the usual validation comes first, in the usual order
            mark = lib.fake_hip_log_size()
            assert getattr(lib, entry)(r.dec, r.frames, None, out, None, 1) == _capi.ERR_INVALID_ARG
            assert r.kernels(mark) == []
        mark = lib.fake_hip_log_size()
        assert lib.bt709hip_decode_half(r.dec, r.frames, r.alphas, scaled, None, 1) == _capi.ERR_SIZE_MISMATCH
        assert r.kernels(mark) == []
        # the 1:1 decode never reads the option
        assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, s, None, 1) == 0
        assert [k[0] for k in r.kernels(mark)] == ["kernel:decode_nv12_quads<alpha>"]
    # 9 on, 10 off: still refused, nothing launched
    assert _set(r, OPT, -1) == 0 and _set(r, OPT9, 0x204060) == 0
    mark = lib.fake_hip_log_size()
    for entry, out in zip(ENTRIES, (half, scaled)):
        assert getattr(lib, entry)(r.dec, r.frames, r.alphas, out, None, 1) == _capi.ERR_UNSUPPORTED
        assert getattr(lib, entry + "_batch")(r.dec, r.n, r.frames, r.alphas, out, None, 1) == _capi.ERR_UNSUPPORTED
    assert r.kernels(mark) == []
    # both on
    assert _set(r, OPT, -2) == 0
    for entry, out in zip(ENTRIES, (half, scaled)):
        assert getattr(lib, entry + "_batch")(r.dec, r.n, r.frames, r.alphas, out, None, 1) == 0
    assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, s, None, 1) == 0
    assert [k[0] for k in r.kernels(mark)] == ["kernel:decode_nv12_scaled", "kernel:decode_nv12_scaled", "kernel:decode_nv12_quads<alpha>"]
    # both off: the plain paths, the persistent-or-not 2:1 kernel included
    assert _set(r, OPT, -1) == 0 and _set(r, OPT9, -1) == 0
    mark = lib.fake_hip_log_size()
    assert lib.bt709hip_decode_half_batch(r.dec, r.n, r.frames, r.alphas, half, None, 1) == 0
    assert [k[0] for k in r.kernels(mark)] == ["kernel:decode_nv12_half"]


def test_shim_builds_the_table_at_setup_and_not_inside_a_capture(fake, fake_rig):
    """A decoder set up before the option was turned on holds no lin[] table: its first blended rescale builds it, unless the
    stream records a graph -- then ERR_NOT_SETUP until bt709hip_decoder_setup (a no-op otherwise) has built it.  Only option 10
    is on throughout."""
    lib, r = fake, fake_rig
    scaled, g = r.surfs(48, 10), C.c_void_p()
    assert lib.bt709hip_decoder_setup(r.dec) == 0
    mark = lib.fake_hip_log_size()
    assert _set(r, OPT, -2) == 0 and _set(r, OPT, 0x808080) == 0 and _set(r, OPT, -2) == 0
    assert lib.fake_hip_log_size() == mark  # setting the option never touches the device
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    assert lib.bt709hip_decode_scaled(r.dec, r.frames, r.alphas, scaled, r.stream, 0) == _capi.ERR_NOT_SETUP
    assert lib.bt709hip_decode_half(r.dec, r.frames, r.alphas, r.surfs(r.w // 2, r.h // 2), r.stream, 0) == _capi.ERR_NOT_SETUP
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0 and lib.bt709hip_graph_destroy(r.ctx, g) == 0
    assert r.kernels(mark) == []
    assert lib.bt709hip_decoder_setup(r.dec) == 0  # builds what the option needs
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    assert lib.bt709hip_decode_scaled(r.dec, r.frames, r.alphas, scaled, r.stream, 0) == 0
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0
    assert r.kernels(mark) == []  # recorded, not run
    assert lib.bt709hip_graph_launch(r.ctx, g, r.stream) == 0 and lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    assert len(r.kernels(mark)) == 1
    assert lib.bt709hip_graph_destroy(r.ctx, g) == 0
    # a fresh decoder with only option 10 on: bt709hip_decoder_setup builds the table with the others
    fresh = C.c_void_p()
    assert lib.bt709hip_decoder_create(r.ctx, 0, 1, C.byref(fresh)) == 0
    assert lib.bt709hip_decoder_set_option(fresh, OPT, 0x112233) == 0 and lib.bt709hip_decoder_setup(fresh) == 0
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    assert lib.bt709hip_decode_scaled(fresh, r.frames, r.alphas, scaled, r.stream, 0) == 0
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0 and lib.bt709hip_graph_destroy(r.ctx, g) == 0
    # and one that meets the option outside a capture: the first blended rescale builds the table
    late = C.c_void_p()
    assert lib.bt709hip_decoder_create(r.ctx, 0, 1, C.byref(late)) == 0 and lib.bt709hip_decoder_setup(late) == 0
    assert lib.bt709hip_decoder_set_option(late, OPT, -2) == 0
    assert lib.bt709hip_decode_scaled(late, r.frames, r.alphas, scaled, None, 1) == 0
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    assert lib.bt709hip_decode_scaled(late, r.frames, r.alphas, scaled, r.stream, 0) == 0
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0 and lib.bt709hip_graph_destroy(r.ctx, g) == 0
    assert lib.bt709hip_decoder_destroy(fresh) == 0 and lib.bt709hip_decoder_destroy(late) == 0


# ------------------------------------------------------------------ the bar of the GPU tap-form cases, from the oracle alone

def test_the_blend_shows_in_every_tap_form_case(oracle):
    """tests/test_scaled_over_gpu.py, test 1: in every case -- shape, frame, mode, intermediate -- the expected words differ from
    the option-off view in at least half the pixels and in a colour byte in at least a quarter of them.  The same function
    asserts it there, on the same arrays; here it runs without a GPU."""
    from test_scaled_f16_gpu import SHAPES, _planes
    tabs = oc.tables(oracle)
    for shape, _, (ow, oh), _, _ in SHAPES:
        for i in range(3 if shape in ("once", "wide") else 1):
            canvas = sc.canvas(ow, oh, i)
            for tag, intermediate in sc.INTERMEDIATES:
                view = sc.option_off_view(oracle, _planes(shape, i), ow, oh, intermediate)
                for mode in sc.MODES:
                    want = oc.composite_over(view, canvas if mode == "destination" else sc.COLOUR, *tabs)
                    sc.assert_the_blend_shows(view, want, "%s frame %d %s %s" % (shape, i, tag, mode))
