"""Straight alpha in and out -- BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY and BT709HIP_OPT_UNPREMULTIPLY -- the parts that
need no GPU: the two shared arithmetic headers replayed on the host over all 65 536 (colour, alpha) pairs, the constants of the
bindings, and -- on the shim built against the fake HIP runtime -- the options' domains, every refusal, the coalescing queue and
a graph capture.  (The fake runtime's launchers report fixed kernel names: the names are the GPU tests' business.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_headers
import metalbt709decoder_amd as mb
import straight_alpha_cases as sc
from metalbt709decoder_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CTX_OPT, DEC_OPT = sc.CTX_OPT_ENCODE_PREMULTIPLY, sc.OPT_UNPREMULTIPLY
SRGB, APPLE, LIN = mb.MetalBT709GammaSRGB, mb.MetalBT709GammaApple, mb.MetalBT709GammaLinear
ALPHA_FORMAT = 3  # BT709HIP_FORMAT_BGRA8_ALPHA
BAD_VALUES = (-1, 2, 255)
PAIRS = [(c, a) for c in range(256) for a in range(256)]  # index c * 256 + a, as the native sweep's


# ------------------------------------------------------------------ the arithmetic headers, every pair

@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """tests/native/straight_alpha_sweep.cpp + the two headers, plain g++ (as test_quantiser_exact.py builds its sweep)."""
    out = str(tmp_path_factory.mktemp("native") / "libstraight_alpha_sweep.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "metalbt709decoder_amd", "csrc"), os.path.join(HERE, "native", "straight_alpha_sweep.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return C.CDLL(out)


def _words(fn, *args):
    out = (C.c_uint32 * 65536)()
    fn(*args, out)
    return list(out)


def _expected_words(channel):
    """The sweep's word for every pair with each colour byte through `channel(c, A)`, in Python integers."""
    want = []
    for c, a in PAIRS:
        w = sc.sweep_word(c, a)
        want.append((a << 24) | (channel((w >> 16) & 255, a) << 16) | (channel((w >> 8) & 255, a) << 8) | channel(w & 255, a))
    return want


def test_the_sweeps_words_cover_every_pair_in_every_byte_lane(sweep):
    words = _words(sweep.sweep_words_in)
    assert words == [sc.sweep_word(c, a) for c, a in PAIRS]
    for shift in (0, 8, 16):
        assert len({((w >> shift) & 255, w >> 24) for w in words}) == 65536


def test_premultiply_header_every_pair(sweep):
    got = (C.c_uint8 * 65536)()
    sweep.sweep_premultiply_byte(got)
    assert list(got) == [sc.premultiply_int(c, a) for c, a in PAIRS]
    assert _words(sweep.sweep_premultiply_word) == _expected_words(sc.premultiply_int)
    # what the definition promises: A = 255 the identity, A = 0 colour 0
    assert all(sc.premultiply_int(c, 255) == c and sc.premultiply_int(c, 0) == 0 for c in range(256))


@pytest.mark.parametrize("ulps", [0, 1, -1, 2, -2, 4, -4])
def test_unpremultiply_header_every_pair_whatever_the_reciprocals_last_bits(sweep, ulps):
    """The kernels take 1 / A from v_rcp_f32 (1 ulp): the host replay moves the correctly rounded reciprocal by up to four floats
    either way, and the rounded, saturated value is the definition's quotient every time (the header's margin argument)."""
    want = _expected_words(sc.unpremultiply_int)
    want = [w if (w >> 24) else 0 for w in want]  # A = 0: the word 0
    assert _words(sweep.sweep_unpremultiply_word, ulps) == want
    assert all(sc.unpremultiply_int(c, 255) == c and sc.unpremultiply_int(c, 0) == 0 for c in range(256))
    assert all(sc.unpremultiply_int(c, a) == 255 for a in range(1, 255) for c in range(a + 1, 256))  # c' > A saturates


def test_numpy_statements_are_the_integer_definitions():
    """The case module's vectorised forms (what the GPU tests expect) against the one-line integer definitions, every pair."""
    c, a = np.array(PAIRS, np.uint32).T
    words = (a << 24) | (c << 16) | (((c + 85) & 255) << 8) | ((c + 170) & 255)
    assert sc.premultiply(words).tolist() == _expected_words(sc.premultiply_int)
    bgra = np.stack([words & 255, (words >> 8) & 255, (words >> 16) & 255, words >> 24], -1).astype(np.uint8)
    got = sc.unpremultiply(bgra)
    packed = (got[:, 3].astype(np.uint32) << 24) | (got[:, 2].astype(np.uint32) << 16) | (got[:, 1].astype(np.uint32) << 8) | got[:, 0]
    assert packed.tolist() == _expected_words(sc.unpremultiply_int)
    sc.check_every_pair_picture()


# ------------------------------------------------------------------ constants

def test_constants_agree_and_nothing_was_exported(tmp_path):
    """The header's two enumerators, read by a C compiler, against the bindings; the hosts' mirrors; no export, no ABI bump."""
    src, exe = tmp_path / "ids.c", tmp_path / "ids"
    src.write_text('#include <stdio.h>\n#include "bt709hip_ext.h"\nint main(void) {\n'
                   '  printf("%d %d %d\\n", (int)BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY, (int)BT709HIP_OPT_UNPREMULTIPLY, (int)BT709HIP_VERSION);\n  return 0;\n}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ids = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert ids == [8, 12, 504]
    assert (_capi.CTX_OPT_ENCODE_PREMULTIPLY, _capi.OPT_UNPREMULTIPLY, _capi.ABI_VERSION) == (CTX_OPT, DEC_OPT, 504) == (8, 12, 504)
    header = abi_headers.ext_text()
    for block, words in (("BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY", ("(c * A + 127) / 255", "BT709HIP_ERR_INVALID_ARG", "not clamped", "BGRA8_ALPHA", "never touches the device",
                                                               "encode_bgra_nv12<premul>", "encode_bgra_i420_blocks<premul>", "bt709hip_last_launch_info")),
                         ("BT709HIP_OPT_UNPREMULTIPLY", ("min(255, (255 * c' + A / 2) / A)", "BT709HIP_ERR_INVALID_ARG", "BT709HIP_ERR_UNSUPPORTED", "RGBA16F",
                                                         "bt709hip_decode_half[_batch]", "bt709hip_decode_scaled[_batch]", "BT709HIP_OPT_COMPOSITE_OVER",
                                                         "never touches the device", "decode_nv12_quads<alpha,straight>", "decode_i420_blocks<alpha,straight>"))):
        comment = re.search(r"/\* %s[ .].*?\*/" % block, header, flags=re.S).group(0)
        for word in words:
            assert word in comment, (block, word)
    assert "not premultiplied" not in abi_headers.core_text()
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    assert "kEncodePremultiplyOption = BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY" in hpp and "bool setEncodePremultiply(bool on)" in hpp
    assert re.search(r"setStraightAlpha\(bool on\) \{ return setOption\(BT709HIP_OPT_UNPREMULTIPLY, on \? 1 : 0\); \}", hpp)
    objc = open(os.path.join(ROOT, "objc", "MetalBT709Decoder+HIP.h")).read()
    assert "@property (nonatomic, assign) BOOL hipStraightAlpha;" in objc
    impl = open(os.path.join(ROOT, "objc", "MetalBT709Decoder+HIP.m")).read()
    assert "bt709hip_decoder_set_option(_hipDecoder, BT709HIP_OPT_UNPREMULTIPLY, self.hipStraightAlpha ? 1 : 0)" in impl
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103


def test_python_mirror_keeps_the_flag_until_setup():
    d = mb.MetalBT709Decoder()
    d.hasAlphaChannel = True
    assert d.straightAlpha is False
    d.straightAlpha = True
    assert d.straightAlpha is True and d._options[DEC_OPT] == 1
    d.straightAlpha = False
    assert d.straightAlpha is False and d._options[DEC_OPT] == 0
    opaque = mb.MetalBT709Decoder()
    opaque.straightAlpha = False  # nothing to switch off: setupMetal must not hand the option to a decoder without alpha
    assert DEC_OPT not in opaque._options


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_straight") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.bt709hip_abi_version() == 504
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_set_device_count(1)
    return lib


@pytest.fixture()
def enc(fake):
    from test_encode_planar_cpu import Rig
    r = Rig(fake)
    yield r
    r.close()


@pytest.fixture()
def dec(fake):
    from test_over_cpu import FakeRig
    r = FakeRig(fake)
    yield r
    r.close()


def _get(lib, handle, opt=DEC_OPT):
    v = C.c_int(-12345)
    assert lib.bt709hip_decoder_get_option(handle, opt, C.byref(v)) == _capi.OK
    return v.value


def _calls(lib, mark):
    """Everything the runtime was asked to do since `mark`, as (what, stream, frames) -- the fake's log."""
    from test_fake_hip import log
    return [o[:3] for o in log(lib, mark)]


def test_decoder_option_domain(fake, dec):
    lib, r = fake, dec
    assert lib.bt709hip_decoder_set_option(None, DEC_OPT, 1) == _capi.ERR_INVALID_ARG
    assert _get(lib, r.dec) == 0  # the default
    for held in (1, 0, 1):
        assert lib.bt709hip_decoder_set_option(r.dec, DEC_OPT, held) == _capi.OK
        assert _get(lib, r.dec) == held
        for bad in BAD_VALUES:
            assert lib.bt709hip_decoder_set_option(r.dec, DEC_OPT, bad) == _capi.ERR_INVALID_ARG, bad  # refused ...
            assert _get(lib, r.dec) == held                                                              # ... and kept
    opaque = C.c_void_p()
    assert lib.bt709hip_decoder_create(r.ctx, 0, 0, C.byref(opaque)) == 0
    try:
        for value in (1, 0):
            assert lib.bt709hip_decoder_set_option(opaque, DEC_OPT, value) == _capi.ERR_UNSUPPORTED  # nothing to divide by
            assert _get(lib, opaque) == 0
        assert lib.bt709hip_decoder_set_option(opaque, DEC_OPT, 2) == _capi.ERR_INVALID_ARG
    finally:
        assert lib.bt709hip_decoder_destroy(opaque) == 0
    # the ids next to the new ones are what they were
    assert lib.bt709hip_decoder_set_option(r.dec, 99, 0) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_decoder_get_option(r.dec, 99, C.byref(C.c_int())) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_decoder_set_option(r.dec, 13, 0) == _capi.ERR_INVALID_ARG


def test_context_option_domain(fake, enc):
    lib, r = fake, enc
    assert lib.bt709hip_context_set_option(None, CTX_OPT, 1) == _capi.ERR_INVALID_ARG
    mark = lib.fake_hip_log_size()
    for held in (1, 0, 1, 0):
        assert lib.bt709hip_context_set_option(r.ctx, CTX_OPT, held) == _capi.OK
        for bad in BAD_VALUES + (1 << 30, -(1 << 31)):
            assert lib.bt709hip_context_set_option(r.ctx, CTX_OPT, bad) == _capi.ERR_INVALID_ARG, bad  # refused, not clamped
    assert lib.fake_hip_log_size() == mark  # setting it never touches the device
    assert lib.bt709hip_context_set_option(r.ctx, 7, 0) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_context_set_option(r.ctx, 9, 0) == _capi.ERR_INVALID_ARG
    # the clamping neighbours still clamp, the refusing neighbour still refuses
    for opt in (_capi.CTX_OPT_ENCODE_ROW_PAIRS, _capi.CTX_OPT_ENCODE_THREADS, _capi.CTX_OPT_XCD_BANDS):
        assert lib.bt709hip_context_set_option(r.ctx, opt, 1 << 30) == _capi.OK and lib.bt709hip_context_set_option(r.ctx, opt, 0) == _capi.OK
    assert lib.bt709hip_context_set_option(r.ctx, _capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, 2) == _capi.ERR_INVALID_ARG


def test_encode_calls_are_the_plain_encoders_with_the_option_on(fake, enc):
    """Validation, launches and launch plans do not depend on the option -- for colour pictures and for BGRA8_ALPHA input, whose
    call sequence is the same with it on and off."""
    lib, r = fake, enc
    info = _capi.LaunchInfo()
    seen = {}
    for on in (0, 1):
        assert lib.bt709hip_context_set_option(r.ctx, CTX_OPT, on) == _capi.OK
        assert lib.bt709hip_encoder_prepare(r.ctx, SRGB, APPLE) == 0 and lib.bt709hip_encoder_prepare(r.ctx, LIN, LIN) == 0
        mark = lib.fake_hip_log_size()
        plans = []
        assert lib.bt709hip_encode(r.ctx, r.surfs(), r.frames(r.w), SRGB, APPLE, None, 1) == 0
        assert lib.bt709hip_last_launch_info(C.byref(info)) == 0
        plans.append((tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands))
        assert lib.bt709hip_encode_batch(r.ctx, r.n, r.surfs(), r.frames(r.w), SRGB, APPLE, None, 1) == 0
        assert lib.bt709hip_last_launch_info(C.byref(info)) == 0
        plans.append((tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands))
        assert lib.bt709hip_encode_batch(r.ctx, r.n, r.surfs(ALPHA_FORMAT), r.frames(r.w), LIN, LIN, None, 1) == 0
        assert lib.bt709hip_encode_batch(r.ctx, r.n, r.surfs(ALPHA_FORMAT), r.frames(0, cbcr=False), LIN, LIN, None, 1) == 0
        assert lib.bt709hip_encode(r.ctx, r.surfs(ALPHA_FORMAT), r.frames(r.w), SRGB, APPLE, None, 1) == _capi.ERR_ALPHA_TRANSFER
        assert lib.bt709hip_encode(r.ctx, r.surfs(), r.frames(r.w - 1), SRGB, APPLE, None, 1) == _capi.ERR_STRIDE
        assert lib.bt709hip_encode(r.ctx, r.surfs(w=62, h=15), r.frames(r.w, w=62, h=15), SRGB, APPLE, None, 1) == _capi.ERR_ODD_DIMENSIONS
        seen[on] = (_calls(lib, mark), plans)
        assert [c[2] for c in seen[on][0] if c[0].startswith("kernel:")] == [1, r.n, r.n, r.n]
    assert seen[0] == seen[1]
    assert lib.bt709hip_context_set_option(r.ctx, CTX_OPT, 0) == _capi.OK


def test_both_options_work_inside_a_capture_and_need_no_table(fake, enc, dec):
    lib = fake
    # the encoder: its tables are the plain encoder's
    r = enc
    assert lib.bt709hip_encoder_prepare(r.ctx, SRGB, APPLE) == 0
    S, g = C.c_void_p(), C.c_void_p()
    assert lib.bt709hip_stream_create(r.ctx, C.byref(S)) == 0
    mark = lib.fake_hip_log_size()
    assert lib.bt709hip_graph_begin_capture(r.ctx, S) == 0
    assert lib.bt709hip_context_set_option(r.ctx, CTX_OPT, 1) == _capi.OK  # while the stream is being captured
    assert lib.bt709hip_context_set_option(r.ctx, CTX_OPT, 2) == _capi.ERR_INVALID_ARG
    assert lib.fake_hip_log_size() == mark
    assert lib.bt709hip_encode_batch(r.ctx, r.n, r.surfs(), r.frames(r.w), SRGB, APPLE, S, 0) == 0
    assert lib.bt709hip_graph_end_capture(r.ctx, S, C.byref(g)) == 0
    assert r.kernels(mark) == []  # recorded, not run
    assert lib.bt709hip_graph_launch(r.ctx, g, S) == 0 and lib.bt709hip_stream_synchronize(r.ctx, S) == 0
    issued = r.kernels(mark)
    assert len(issued) == 1 and issued[0][0].startswith("kernel:encode") and issued[0][2] == r.n
    assert lib.bt709hip_graph_destroy(r.ctx, g) == 0 and lib.bt709hip_stream_destroy(r.ctx, S) == 0
    # the decoder: set up without the option, which then needs nothing more
    d = dec
    assert lib.bt709hip_decoder_setup(d.dec) == 0
    mark = lib.fake_hip_log_size()
    assert lib.bt709hip_graph_begin_capture(d.ctx, d.stream) == 0
    assert lib.bt709hip_decoder_set_option(d.dec, DEC_OPT, 1) == _capi.OK
    assert lib.bt709hip_decoder_set_option(d.dec, DEC_OPT, -1) == _capi.ERR_INVALID_ARG
    assert lib.fake_hip_log_size() == mark
    assert lib.bt709hip_decode(d.dec, d.frames, d.alphas, d.surfs(), d.w, d.h, d.stream, 0) == 0
    assert lib.bt709hip_graph_end_capture(d.ctx, d.stream, C.byref(g)) == 0
    assert d.kernels(mark) == []
    assert lib.bt709hip_graph_launch(d.ctx, g, d.stream) == 0 and lib.bt709hip_stream_synchronize(d.ctx, d.stream) == 0
    issued = d.kernels(mark)
    assert len(issued) == 1 and issued[0][0].startswith("kernel:decode") and issued[0][2] == 1
    assert lib.bt709hip_graph_destroy(d.ctx, g) == 0


def test_every_refusal_comes_after_the_validation_and_enqueues_nothing(fake, dec):
    lib, r = fake, dec
    s, f16, half, scaled = r.surfs(), r.surfs(fmt=_capi.FORMAT_RGBA16F), r.surfs(r.w // 2, r.h // 2), r.surfs(48, 10)
    # each of these succeeds with the option off
    mark = lib.fake_hip_log_size()
    assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, f16, None, 1) == 0
    assert lib.bt709hip_decode_half_batch(r.dec, r.n, r.frames, r.alphas, half, None, 1) == 0
    assert lib.bt709hip_decode_scaled_batch(r.dec, r.n, r.frames, r.alphas, scaled, None, 1) == 0
    assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COMPOSITE_OVER, 0x204060) == 0
    assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, s, None, 1) == 0
    assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COMPOSITE_OVER, _capi.OVER_OFF) == 0
    assert len(r.kernels(mark)) == 4
    assert lib.bt709hip_decoder_set_option(r.dec, DEC_OPT, 1) == 0
    assert lib.bt709hip_stream_synchronize(r.ctx, None) == 0
    mark = lib.fake_hip_log_size()
    # RGBA16F targets
    assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, f16, None, 1) == _capi.ERR_UNSUPPORTED
    assert lib.bt709hip_decode(r.dec, r.frames, r.alphas, f16, r.w, r.h, None, 1) == _capi.ERR_UNSUPPORTED
    # the rescales
    for entry, out in (("bt709hip_decode_half", half), ("bt709hip_decode_scaled", scaled)):
        assert getattr(lib, entry)(r.dec, r.frames, r.alphas, out, None, 1) == _capi.ERR_UNSUPPORTED
        assert getattr(lib, entry + "_batch")(r.dec, r.n, r.frames, r.alphas, out, None, 1) == _capi.ERR_UNSUPPORTED
        assert getattr(lib, entry)(r.dec, r.frames, None, out, None, 1) == _capi.ERR_INVALID_ARG  # the usual validation first
    assert lib.bt709hip_decode_half(r.dec, r.frames, r.alphas, scaled, None, 1) == _capi.ERR_SIZE_MISMATCH
    assert lib.bt709hip_decode(r.dec, r.frames, None, s, r.w, r.h, None, 1) == _capi.ERR_INVALID_ARG
    # SCALED_OVER on does not let a rescale through either
    assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_SCALED_OVER, 0x808080) == 0
    assert lib.bt709hip_decode_scaled_batch(r.dec, r.n, r.frames, r.alphas, scaled, None, 1) == _capi.ERR_UNSUPPORTED
    assert lib.bt709hip_decode_half_batch(r.dec, r.n, r.frames, r.alphas, half, None, 1) == _capi.ERR_UNSUPPORTED
    assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_SCALED_OVER, _capi.OVER_OFF) == 0
    # a 1:1 decode under COMPOSITE_OVER, in each of its forms; the coalescing submit refuses at the call, too
    for over in (_capi.OVER_DESTINATION, 0, 0xFFFFFF):
        assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COMPOSITE_OVER, over) == 0
        assert _get(lib, r.dec) == 1  # the two options are held independently
        assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, s, None, 1) == _capi.ERR_UNSUPPORTED
        assert lib.bt709hip_decode(r.dec, r.frames, r.alphas, s, r.w, r.h, None, 1) == _capi.ERR_UNSUPPORTED
        assert lib.bt709hip_decode(r.dec, r.frames, None, s, r.w, r.h, None, 1) == _capi.ERR_INVALID_ARG
        assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COALESCE, 4) == 0
        assert lib.bt709hip_decode(r.dec, r.frames, r.alphas, s, r.w, r.h, r.stream, 0) == _capi.ERR_UNSUPPORTED
        assert lib.bt709hip_decode(r.dec, r.frames, r.alphas, f16, r.w, r.h, r.stream, 0) == _capi.ERR_UNSUPPORTED
        assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COALESCE, 0) == 0
    assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COMPOSITE_OVER, _capi.OVER_OFF) == 0
    assert lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    assert _calls(lib, mark) == [], "a refused call enqueued something"
    # and the covered call goes through; off again, so does everything else
    assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, s, None, 1) == 0
    assert lib.bt709hip_decode(r.dec, r.frames, r.alphas, s, r.w, r.h, None, 1) == 0
    assert [k[2] for k in r.kernels(mark)] == [r.n, 1]
    assert lib.bt709hip_decoder_set_option(r.dec, DEC_OPT, 0) == 0
    assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, f16, None, 1) == 0
    assert lib.bt709hip_decode_half_batch(r.dec, r.n, r.frames, r.alphas, half, None, 1) == 0
    assert lib.bt709hip_decode_scaled_batch(r.dec, r.n, r.frames, r.alphas, scaled, None, 1) == 0
    assert len(r.kernels(mark)) == 5


def test_coalescing_queue_goes_out_before_the_flip_takes_effect(fake, dec):
    """Three frames: two queued at 0, the option flipped to 1, one queued.  The flip issues the first queue (under the value it
    was queued with: the option changes behind the launch); the third frame goes out on its own.  Two launches, in order."""
    lib, r = fake, dec
    s = r.surfs()
    assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COALESCE, 4) == 0
    mark = lib.fake_hip_log_size()
    for i in (0, 1):
        assert lib.bt709hip_decode(r.dec, C.byref(r.frames[i]), C.byref(r.alphas[i]), C.byref(s[i]), r.w, r.h, r.stream, 0) == 0
    assert r.kernels(mark) == [] and _get(lib, r.dec) == 0  # queued
    assert lib.bt709hip_decoder_set_option(r.dec, DEC_OPT, 1) == 0
    issued = r.kernels(mark)
    assert len(issued) == 1 and issued[0][2] == 2 and _get(lib, r.dec) == 1  # out at the flip, not later
    assert lib.bt709hip_decode(r.dec, C.byref(r.frames[2]), C.byref(r.alphas[2]), C.byref(s[2]), r.w, r.h, r.stream, 0) == 0
    assert len(r.kernels(mark)) == 1  # queued
    assert lib.bt709hip_decoder_flush(r.dec, r.stream) == 0 and lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    issued = r.kernels(mark)
    assert [k[2] for k in issued] == [2, 1]
    # a refused value changes nothing, but leaves nothing queued behind it either
    assert lib.bt709hip_decode(r.dec, C.byref(r.frames[3]), C.byref(r.alphas[3]), C.byref(s[3]), r.w, r.h, r.stream, 0) == 0
    assert lib.bt709hip_decoder_set_option(r.dec, DEC_OPT, 2) == _capi.ERR_INVALID_ARG
    assert [k[2] for k in r.kernels(mark)] == [2, 1, 1] and _get(lib, r.dec) == 1
