"""BT709HIP_CTX_OPT_ENCODE_CONVERT (bt709hip_encode[_batch] as the reference's per-pixel +convert:), the parts that
need no GPU: the option's domain, the call's validation, launch plans and capture rules on the fake HIP runtime
(tests/native/fake_hip/), the curve table's bits against the oracle's compositions, the header's text and the generated code of the
packed fast kernel."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import abi_headers
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
OPT, OFF, PACKED, POINT = 10, 0, 1, 2  # stated here, not taken from the bindings
ALPHA = 3                              # BT709HIP_FORMAT_BGRA8_ALPHA
APPLE, SRGB, LIN, ITU = 0, 1, 2, 3
BAD_VALUES = (-1, 3, 255, 1 << 30, -(1 << 31))
KERNEL_NAMES = ("convert_bgra_packed444", "convert_bgra_packed444_blocks", "convert_bgra_nv12", "convert_bgra_i420",
                "convert_bgra_nv12_blocks", "convert_bgra_i420_blocks")


def test_constants_agree_and_nothing_was_exported(tmp_path):
    src, exe = tmp_path / "ids.c", tmp_path / "ids"
    src.write_text('#include <stdio.h>\n#include "bt709hip_ext.h"\nint main(void) {\n'
                   '  printf("%d %d %d %d %d\\n", (int)BT709HIP_CTX_OPT_ENCODE_CONVERT, BT709HIP_CONVERT_OFF, BT709HIP_CONVERT_PACKED444,\n'
                   '         BT709HIP_CONVERT_POINT420, (int)BT709HIP_VERSION);\n  return 0;\n}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ids = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert ids == [OPT, OFF, PACKED, POINT, 504]
    assert (_capi.CTX_OPT_ENCODE_CONVERT, _capi.CONVERT_OFF, _capi.CONVERT_PACKED444, _capi.CONVERT_POINT420, _capi.ABI_VERSION) == (OPT, OFF, PACKED, POINT, 504)
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103  # no export
    assert open(os.path.join(ROOT, "include", "bt709hip.h")).read().count("\n") <= 250
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    assert "kEncodeConvertOption = BT709HIP_CTX_OPT_ENCODE_CONVERT" in hpp and "static bool convert(MetalRenderContext &mrc" in hpp


def test_header_block_states_the_contract():
    header = abi_headers.ext_text()
    comment = re.search(r"/\* BT709HIP_CTX_OPT_ENCODE_CONVERT\..*?\*/", header, flags=re.S).group(0)
    for word in ("BT709HIP_CONVERT_OFF", "BT709HIP_CONVERT_PACKED444", "BT709HIP_CONVERT_POINT420", "(Cr<<16)|(Cb<<8)|Y", "top byte", "ODD row",
                 "EVEN column", "BT709HIP_ERR_INVALID_ARG", "BT709HIP_ERR_UNSUPPORTED", "BT709HIP_ERR_STRIDE", "BT709HIP_ERR_NOT_SETUP", "not clamped",
                 "never touches the device", "ITU709", "BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY", "bt709hip_last_launch_info", "<premul>") + KERNEL_NAMES:
        assert word in comment, word
    assert "BT709HIP_CTX_OPT_ENCODE_CONVERT" in abi_headers.core_text()


# ------------------------------------------------------------------ the curve table

def test_curve_table_bits_are_the_oracles_compositions(tmp_path, oracle):
    """tests/native/convert_curve_dump.cpp (its own main, transfer_tables.cpp alone) prints the 4 x 256 entries' bit patterns."""
    exe = str(tmp_path / "convert_curve_dump")
    csrc = os.path.join(ROOT, "metalbt709decoder_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I", csrc,
                        os.path.join(HERE, "native", "convert_curve_dump.cpp"), os.path.join(csrc, "transfer_tables.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = {int(line.split()[0]): [int(x, 16) for x in line.split()[1:]] for line in out.stdout.strip().split("\n")}
    assert sorted(got) == [APPLE, SRGB, LIN, ITU] and all(len(v) == 256 for v in got.values())
    L = oracle.lib
    bits = lambda f: struct.unpack("<I", struct.pack("<f", f))[0]
    norm = [float(np.float32(b) * np.float32(1.0 / 255.0)) for b in range(256)]  # byteNorm: a float product
    lin = [L.bt709o_srgb_to_linear(n) for n in norm]
    want = {SRGB: norm, LIN: lin, APPLE: [L.bt709o_linear_to_apple196(v) for v in lin], ITU: [L.bt709o_linear_to_itu709(v) for v in lin]}
    for g in got:
        assert got[g] == [bits(v) for v in want[g]], g
    # the operand range of the kernels' constant division (bt709_encode_convert.h): every entry 0 or in [3.0e-4, 1 + 2^-22]
    for g, table in want.items():
        assert table[0] == 0.0 and all(3.0e-4 <= v <= 1.0 + 2.0 ** -22 for v in table[1:]), g
    # and a pixel through the table is the oracle's pixel: encode_pixel's own curve step, every byte
    for g in got:
        for b in (0, 1, 10, 11, 127, 254, 255):
            y = oracle.encode_pixel(g, b, b, b)[0]
            v = np.float32(want[g][b])
            ey = (np.float32(0.2126) * v + np.float32(0.7152) * v) + np.float32(0.0722) * v
            assert y == int(np.floor(np.float32(ey * np.float32(219) + np.float32(16)) + np.float32(0.5))), (g, b)


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_convert") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.bt709hip_abi_version() == 504
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_set_device_count(1)
    return lib


class Rig:
    """A context, `n` w x h pictures, `n` word pictures and `n` NV12 frames carved evenly from three allocations."""

    def __init__(self, lib, n=4, w=64, h=16):
        self.lib, self.n, self.w, self.h = lib, n, w, h
        self.ctx = C.c_void_p()
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0
        self.src, self.words, self.dst = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.bt709hip_malloc(self.ctx, n * w * h * 4, C.byref(self.src)) == 0
        assert lib.bt709hip_malloc(self.ctx, n * w * h * 4 + 64, C.byref(self.words)) == 0
        assert lib.bt709hip_malloc(self.ctx, n * w * h * 3 // 2, C.byref(self.dst)) == 0

    def set(self, value):
        return self.lib.bt709hip_context_set_option(self.ctx, OPT, value)

    def surfs(self, fmt=0, w=None, h=None, n=None):
        w, h, n = w or self.w, h or self.h, n or self.n
        return (_capi.Surface * n)(*[_capi.Surface(self.src.value + (i % self.n) * self.w * self.h * 4, w * 4, w, h, fmt, 0) for i in range(n)])

    def packed(self, stride=None, cbcr=None, cbcr_stride=0, w=None, h=None, shift=0, n=None):
        w, h, n = w or self.w, h or self.h, n or self.n
        stride = 4 * w if stride is None else stride
        return (_capi.Frame * n)(*[_capi.Frame(self.words.value + shift + (i % self.n) * self.w * self.h * 4, stride, cbcr, cbcr_stride, w, h, 0, 0)
                                   for i in range(n)])

    def frames(self, w=None, h=None):
        w, h = w or self.w, h or self.h
        out = []
        for i in range(self.n):
            base = self.dst.value + i * self.w * self.h * 3 // 2
            out.append(_capi.Frame(base, w, base + self.w * self.h, w, w, h, 0, 0))
        return (_capi.Frame * self.n)(*out)

    def kernels(self, mark):
        from test_fake_hip import log
        return [o for o in log(self.lib, mark) if o[0].startswith("kernel:")]

    def plan(self):
        info = _capi.LaunchInfo()
        assert self.lib.bt709hip_last_launch_info(C.byref(info)) == 0
        return tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands

    def close(self):
        lib = self.lib
        for p in (self.src, self.words, self.dst):
            assert lib.bt709hip_free(self.ctx, p) == 0
        assert lib.bt709hip_context_destroy(self.ctx) == 0


@pytest.fixture()
def rig(fake):
    r = Rig(fake)
    yield r
    r.close()


def held(rig):
    """There is no getter (no export was added): the held value shows in what the next call accepts -- output gamma ITU709 only
    with the option on, a frame with a chroma plane only under OFF and POINT420, word frames only under PACKED444."""
    lib = rig.lib
    if lib.bt709hip_encode(rig.ctx, rig.surfs(), rig.packed(), SRGB, ITU, None, 1) == 0:
        return PACKED
    rc = lib.bt709hip_encode(rig.ctx, rig.surfs(), rig.frames(), SRGB, ITU, None, 1)
    assert rc in (0, _capi.ERR_INVALID_ARG)
    return POINT if rc == 0 else OFF


def test_option_domain(fake, rig):
    lib = fake
    assert lib.bt709hip_context_set_option(None, OPT, PACKED) == _capi.ERR_INVALID_ARG
    assert held(rig) == OFF  # the default
    for value in (PACKED, POINT, OFF, POINT, PACKED):
        mark = lib.fake_hip_log_size()
        assert rig.set(value) == _capi.OK
        for bad in BAD_VALUES:
            assert rig.set(bad) == _capi.ERR_INVALID_ARG, bad  # refused, not clamped ...
        assert lib.fake_hip_log_size() == mark                 # setting it never touches the device
        assert held(rig) == value                              # ... and the option is what it was
    assert rig.set(OFF) == _capi.OK
    # the ids next to it are still no options; the refusing and clamping neighbours are what they were; no ABI bump
    for other in (7, 9, 11):
        assert lib.bt709hip_context_set_option(rig.ctx, other, 0) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_context_set_option(rig.ctx, _capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, 2) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_context_set_option(rig.ctx, _capi.CTX_OPT_ENCODE_PREMULTIPLY, 2) == _capi.ERR_INVALID_ARG
    for opt in (_capi.CTX_OPT_ENCODE_ROW_PAIRS, _capi.CTX_OPT_ENCODE_THREADS, _capi.CTX_OPT_XCD_BANDS):
        assert lib.bt709hip_context_set_option(rig.ctx, opt, 1 << 30) == _capi.OK and lib.bt709hip_context_set_option(rig.ctx, opt, 0) == _capi.OK
    assert lib.bt709hip_abi_version() == 504


def test_off_is_the_plain_encoder(fake, rig):
    lib = fake
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(), rig.frames(), SRGB, ITU, None, 1) == _capi.ERR_INVALID_ARG  # gamma 3 stays refused
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(), rig.packed(), SRGB, APPLE, None, 1) == _capi.ERR_INVALID_ARG  # a colour picture needs its chroma
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(), rig.frames(), LIN, LIN, None, 1) == 0
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(), rig.frames(), APPLE, SRGB, None, 1) == 0


def test_packed_validation_and_refusals_enqueue_nothing(fake, rig):
    lib, n, w, h = fake, rig.n, rig.w, rig.h
    assert rig.set(PACKED) == 0
    assert lib.bt709hip_encoder_prepare(rig.ctx, SRGB, APPLE) == 0
    mark = lib.fake_hip_log_size()
    s = rig.surfs()
    one = lambda f, gi=SRGB, go=APPLE, surfs=None: lib.bt709hip_encode(rig.ctx, surfs or s, f, gi, go, None, 1)
    batch = lambda f, gi=SRGB, go=APPLE, surfs=None, count=None: lib.bt709hip_encode_batch(rig.ctx, count or n, surfs or s, f, gi, go, None, 1)
    # cbcr must be NULL, in every frame
    assert one(rig.packed(cbcr=rig.dst.value, cbcr_stride=w)) == _capi.ERR_INVALID_ARG
    mixed = rig.packed()
    mixed[2].cbcr = rig.dst.value
    assert batch(mixed) == _capi.ERR_INVALID_ARG
    # the word pitch and pointer
    assert one(rig.packed(stride=4 * w - 4)) == _capi.ERR_STRIDE      # y_stride < 4W
    assert one(rig.packed(stride=w)) == _capi.ERR_STRIDE              # a luma pitch is no word pitch
    assert one(rig.packed(stride=4 * w + 2)) == _capi.ERR_STRIDE      # not a multiple of 4
    assert one(rig.packed(shift=2)) == _capi.ERR_STRIDE               # a misaligned pointer
    assert batch(rig.packed(shift=1)) == _capi.ERR_STRIDE
    assert one(rig.packed(stride=1 << 32)) == _capi.ERR_STRIDE        # the 32-bit pitch limit
    # gammas and formats: after the usual validation
    assert one(rig.packed(), APPLE, APPLE) == _capi.ERR_UNSUPPORTED and one(rig.packed(), LIN, LIN) == _capi.ERR_UNSUPPORTED
    assert batch(rig.packed(), LIN, SRGB) == _capi.ERR_UNSUPPORTED
    assert one(rig.packed(), surfs=rig.surfs(ALPHA), gi=LIN, go=LIN) == _capi.ERR_UNSUPPORTED
    assert one(rig.packed(), surfs=rig.surfs(ALPHA)) == _capi.ERR_ALPHA_TRANSFER  # the alpha clip's own gamma check still comes first
    assert one(rig.packed(), SRGB, 4) == _capi.ERR_INVALID_ARG and one(rig.packed(), 3, APPLE) == _capi.ERR_INVALID_ARG and one(rig.packed(), -1, APPLE) == _capi.ERR_INVALID_ARG
    assert one(rig.packed(stride=4 * w - 4), LIN, LIN) == _capi.ERR_STRIDE  # ... the pitch check before the gamma refusal
    # the usual checks come first
    assert one(rig.packed(w=62, h=15), surfs=rig.surfs(w=62, h=15)) == _capi.ERR_ODD_DIMENSIONS
    assert one(rig.packed(), surfs=rig.surfs(w=32)) == _capi.ERR_SIZE_MISMATCH
    tall = 2 * 65536
    assert one(rig.packed(h=tall), surfs=rig.surfs(h=tall)) == _capi.ERR_UNSUPPORTED  # height / 2 <= 65535
    uneven = rig.packed(n=33)
    uneven[32].y = uneven[32].y + 16
    assert batch(uneven, surfs=rig.surfs(n=33), count=33) == _capi.ERR_UNSUPPORTED  # 33 pictures through the pointer table
    differing = rig.packed()
    differing[1].y_stride = 4 * w + 16
    assert batch(differing) == _capi.ERR_SIZE_MISMATCH
    assert rig.kernels(mark) == [] and lib.fake_hip_log_size() == mark, "a refused call enqueued something"
    # what goes through: all four output gammas (ITU709 with the option on), cbcr_stride and the tags not looked at
    for go in (APPLE, SRGB, LIN, ITU):
        assert one(rig.packed(), SRGB, go) == 0, go
    f = rig.packed(cbcr_stride=12345)
    f[0].matrix, f[0].transfer = 77, 78
    assert one(f) == 0 and batch(rig.packed()) == 0 and one(rig.packed(stride=4 * w + 4)) == 0
    # 33 evenly spaced word pictures (steps of the BGRA and the word pointers): one launch
    even33 = (_capi.Frame * 33)(*[_capi.Frame(rig.words.value + 16 * i, 4 * w, None, 0, w, h, 0, 0) for i in range(33)])
    even_surfs = (_capi.Surface * 33)(*[_capi.Surface(rig.src.value + 16 * i, 4 * w, w, h, 0, 0) for i in range(33)])
    assert batch(even33, surfs=even_surfs, count=33) == 0
    assert [k[2] for k in rig.kernels(mark)] == [1, 1, 1, 1, 1, n, 1, 33]
    for zw, zh in ((0, 16), (64, 0)):  # zero-sized pictures: OK, no launch
        zs = (_capi.Surface * 1)(_capi.Surface(rig.src.value, 4 * max(zw, 1), zw, zh, 0, 0))
        assert one((_capi.Frame * 1)(_capi.Frame(rig.words.value, 4 * max(zw, 1), None, 0, zw, zh, 0, 0)), surfs=zs) == 0
    assert len(rig.kernels(mark)) == 8
    assert rig.set(OFF) == 0


def test_point420_validation_is_the_encoders(fake, rig):
    lib, n, w = fake, rig.n, rig.w
    assert rig.set(POINT) == 0
    mark = lib.fake_hip_log_size()
    s = rig.surfs()
    assert lib.bt709hip_encode(rig.ctx, s, rig.packed(), SRGB, APPLE, None, 1) == _capi.ERR_INVALID_ARG  # an ordinary frame: it needs its chroma plane
    short = rig.frames()
    short[0].cbcr_stride = w - 1
    assert lib.bt709hip_encode(rig.ctx, s, short, SRGB, APPLE, None, 1) == _capi.ERR_STRIDE
    assert lib.bt709hip_encode(rig.ctx, s, rig.frames(), LIN, LIN, None, 1) == _capi.ERR_UNSUPPORTED
    assert lib.bt709hip_encode(rig.ctx, s, rig.frames(), APPLE, APPLE, None, 1) == _capi.ERR_UNSUPPORTED
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(ALPHA), rig.frames(), LIN, LIN, None, 1) == _capi.ERR_UNSUPPORTED
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(w=62, h=15), rig.frames(w=62, h=15), SRGB, APPLE, None, 1) == _capi.ERR_ODD_DIMENSIONS
    assert rig.kernels(mark) == []
    for go in (APPLE, SRGB, LIN, ITU):
        assert lib.bt709hip_encode_batch(rig.ctx, n, s, rig.frames(), SRGB, go, None, 1) == 0
    assert lib.bt709hip_context_set_option(rig.ctx, _capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, _capi.CHROMA_I420) == 0
    planar = rig.frames()
    for f in planar:
        f.cbcr_stride = w // 2
    assert lib.bt709hip_encode_batch(rig.ctx, n, s, planar, SRGB, ITU, None, 1) == 0  # three planes: the encoder's planar pitch rule
    assert lib.bt709hip_context_set_option(rig.ctx, _capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, _capi.CHROMA_NV12) == 0
    assert [k[2] for k in rig.kernels(mark)] == [n] * 5
    assert rig.set(OFF) == 0


@pytest.mark.parametrize("shape", [(64, 16, 4), (3840, 2160, 1), (64, 8, 64), (64, 8, 65), (1284, 38, 3), (62, 6, 2)])
def test_launch_plan_is_the_plain_encoders(fake, shape):
    """Same size, same count, same alignments: bt709hip_last_launch_info reads the same under OFF, PACKED444 and POINT420 -- the
    single-picture 512-lane tiles, the XCD band split and the general kernel's grid included.  (Launches touch nothing on the fake
    runtime, so the pictures may overlap.)"""
    w, h, n = shape
    rig = Rig(fake, n=1, w=64, h=16)
    try:
        lib = fake
        step = 16 * 4
        surfs = (_capi.Surface * n)(*[_capi.Surface(rig.src.value + i * step, 4 * w, w, h, 0, 0) for i in range(n)])
        nv12 = (_capi.Frame * n)(*[_capi.Frame(rig.dst.value + i * step, w, rig.dst.value + 512 + i * step, w, w, h, 0, 0) for i in range(n)])
        words = (_capi.Frame * n)(*[_capi.Frame(rig.words.value + i * step, 4 * w, None, 0, w, h, 0, 0) for i in range(n)])
        plans = {}
        for mode, frames in ((OFF, nv12), (PACKED, words), (POINT, nv12)):
            assert rig.set(mode) == 0
            mark = lib.fake_hip_log_size()
            assert lib.bt709hip_encode_batch(rig.ctx, n, surfs, frames, SRGB, APPLE, None, 1) == 0
            plans[mode] = rig.plan() + (tuple(k[2] for k in rig.kernels(mark)),)
        assert plans[OFF] == plans[PACKED] == plans[POINT], plans
    finally:
        rig.close()


def test_capture_needs_the_table_prepared(fake):
    lib = fake
    rig = Rig(fake)  # a context of its own: no table yet
    try:
        S, g = C.c_void_p(), C.c_void_p()
        assert lib.bt709hip_stream_create(rig.ctx, C.byref(S)) == 0
        assert lib.bt709hip_encoder_prepare(rig.ctx, SRGB, 4) == _capi.ERR_INVALID_ARG
        assert lib.bt709hip_encoder_prepare(rig.ctx, LIN, ITU) == _capi.ERR_INVALID_ARG  # ITU709: the converter's table alone, sRGB input
        assert lib.bt709hip_encoder_prepare(rig.ctx, SRGB, APPLE) == 0                    # the encoder's tables and the APPLE curve
        mark = lib.fake_hip_log_size()
        assert lib.bt709hip_graph_begin_capture(rig.ctx, S) == 0
        assert rig.set(PACKED) == _capi.OK and rig.set(7) == _capi.ERR_INVALID_ARG  # while the stream is being captured
        assert lib.fake_hip_log_size() == mark
        assert lib.bt709hip_encode_batch(rig.ctx, rig.n, rig.surfs(), rig.packed(), SRGB, ITU, S, 0) == _capi.ERR_NOT_SETUP  # no ITU709 curve yet
        assert lib.bt709hip_encode_batch(rig.ctx, rig.n, rig.surfs(), rig.packed(), SRGB, APPLE, S, 0) == 0
        assert lib.bt709hip_graph_end_capture(rig.ctx, S, C.byref(g)) == 0
        assert rig.kernels(mark) == []  # recorded, not run
        assert lib.bt709hip_graph_launch(rig.ctx, g, S) == 0 and lib.bt709hip_stream_synchronize(rig.ctx, S) == 0
        issued = rig.kernels(mark)
        assert len(issued) == 1 and issued[0][2] == rig.n
        assert lib.bt709hip_graph_destroy(rig.ctx, g) == 0
        # prepared: the same call records
        assert lib.bt709hip_encoder_prepare(rig.ctx, SRGB, ITU) == 0
        mark = lib.fake_hip_log_size()
        assert lib.bt709hip_graph_begin_capture(rig.ctx, S) == 0
        assert lib.bt709hip_encode_batch(rig.ctx, rig.n, rig.surfs(), rig.packed(), SRGB, ITU, S, 0) == 0
        assert rig.set(POINT) == _capi.OK
        assert lib.bt709hip_encode_batch(rig.ctx, rig.n, rig.surfs(), rig.frames(), SRGB, ITU, S, 0) == 0
        assert lib.bt709hip_graph_end_capture(rig.ctx, S, C.byref(g)) == 0
        assert rig.kernels(mark) == []
        assert lib.bt709hip_graph_launch(rig.ctx, g, S) == 0 and lib.bt709hip_stream_synchronize(rig.ctx, S) == 0
        assert len(rig.kernels(mark)) == 2
        assert lib.bt709hip_graph_destroy(rig.ctx, g) == 0 and lib.bt709hip_stream_destroy(rig.ctx, S) == 0
        assert rig.set(OFF) == 0
    finally:
        rig.close()


def test_python_mirror_sets_and_restores_the_option():
    """The mirror's methods exist; the context manager they share puts CONVERT_OFF back whatever the call did."""
    for name in ("convert", "convertBatch", "convertIntoWords", "convertIntoCoreVideoBufferPointSampled"):
        assert callable(getattr(mb.BGRAToBT709Converter, name)), name
    calls = []

    class Lib:
        def bt709hip_context_set_option(self, handle, option, value):
            calls.append((option, value))
            return _capi.OK if value in (OFF, PACKED, POINT) else _capi.ERR_INVALID_ARG

    ctx = mb.MetalRenderContext(0)
    ctx.lib, ctx.handle = Lib(), 1
    with pytest.raises(RuntimeError):
        with ctx._encode_convert(_capi.CONVERT_PACKED444, "test") as ok:
            assert ok
            raise RuntimeError("the call failed")
    assert calls == [(OPT, PACKED), (OPT, OFF)]
    del calls[:]
    with ctx._encode_convert(5, "test") as ok:
        assert not ok
    assert calls == [(OPT, 5)]
    ctx.handle = None


# ------------------------------------------------------------------ the generated code

def kernel(asm, name, form):
    sym = "_ZN5bt709%d%sILj%dEEEvNS_12EncodeParamsE" % (len(name), name, form)
    assert len(re.findall(r"^%s:" % sym, asm, re.M)) == 1, sym
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % sym, asm, re.S | re.M)
    lines = [l.split(";")[0].strip() for l in m.group(1).split("\n")]
    meta = re.search(r"\.name:\s+%s\b.*?(?=\n  - \.a|\Z)" % re.escape(sym), asm, flags=re.S)
    assert meta, name
    return [l for l in lines if l and not l.startswith(".") and not l.endswith(":")], meta.group(0)


def test_isa_of_the_packed_fast_kernel():
    """convert_bgra_packed444 = convert_bgra<kFormPacked> (and its premultiplying twin): per row pair two 16-byte non-temporal
    loads (the prefetch makes it four in the text) and two 16-byte non-temporal stores; the lookups are ds_read_b32 behind one SDWA
    shift each; every access of the loop takes its row's base from scalar registers and a 32-bit lane offset -- no 64-bit VALU
    address arithmetic; the conversions sit between the rounding-mode writes; 1 KiB of static LDS and no scratch."""
    from metalbt709decoder_amd import build
    asm = open(build.emit_asm()).read()
    for form in (4, 6):  # kFormPacked, kFormPacked | kFormStraight
        ins, meta = kernel(asm, "convert_bgra", form)
        ops = [i.split()[0] for i in ins]
        loads = [i for i in ins if i.startswith("global_load")]
        nt_loads = [i for i in loads if re.search(r"\bnt\b", i)]
        assert len(nt_loads) == 4 and all(i.startswith("global_load_dwordx4") for i in nt_loads), loads
        assert len(loads) == 5 and [i for i in loads if i not in nt_loads][0].startswith("global_load_dwordx4")  # the curve's staging: cached
        stores = [i for i in ins if i.startswith(("global_store", "flat_store", "buffer_store"))]
        assert len(stores) == 2 and all(i.startswith("global_store_dwordx4") and re.search(r"\bnt\b", i) for i in stores), stores
        assert not [o for o in ops if o.startswith(("flat_", "scratch_"))]
        for i in loads + stores:  # SGPR base, one VGPR offset
            assert re.search(r"\bs\[\d+:\d+\]", i) and not re.search(r"\boff\b", i), i
        assert not [o for o in ops if o in ("v_lshl_add_u64", "v_addc_co_u32_e32", "v_addc_co_u32_e64", "v_mad_u64_u32", "v_add_co_u32_e32", "v_add_co_u32_e64")], form
        assert ops.count("ds_read_b32") == 24 and ops.count("v_lshlrev_b32_sdwa") == 24  # 8 pixels x 3 channels
        assert not [o for o in ops if o.startswith("ds_read") and o != "ds_read_b32"]
        assert ops.count("v_cvt_pk_u8_f32") == 24
        setreg = [k for k, o in enumerate(ops) if o.startswith("s_setreg")]
        assert len(setreg) == 4
        for a, b in ((setreg[0], setreg[1]), (setreg[2], setreg[3])):
            assert [ops[k] for k in range(a + 1, b)] == ["v_cvt_pk_u8_f32"] * 12, "something sits between the conversions and the mode switch around them"
        assert not [o for o in ops if o.startswith(("v_fma_f32", "v_mad_f32", "v_pk_"))], "a contracted or packed multiply-add"
        assert ops.count("v_fmac_f32_e32") + ops.count("v_fmac_f32_e64") == 32  # div_const's own two correction steps, 2 per chroma sample
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0
        sym = "_ZN5bt70912convert_bgraILj%dEEEvNS_12EncodeParamsE" % form
        descriptor = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), asm, flags=re.S).group(1)
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", descriptor).group(1)) == 1024
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 64  # eight waves per SIMD
    # the point-sampled and the general kernels: no scratch either, the general packed kernel stores dwords
    for name, form in (("convert_bgra", 0), ("convert_bgra", 1), ("convert_bgra", 2), ("convert_bgra", 3), ("convert_bgra_blocks", 0),
                       ("convert_bgra_blocks", 1), ("convert_bgra_blocks", 4), ("convert_bgra_blocks", 6)):
        ins, meta = kernel(asm, name, form)
        assert not [i for i in ins if i.startswith(("scratch_", "flat_"))], (name, form)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0
    stores = [i.split()[0] for i in kernel(asm, "convert_bgra_blocks", 4)[0] if i.startswith("global_store")]
    assert sorted(stores) in (["global_store_dword"] * 4, ["global_store_dwordx2"] * 2), stores
