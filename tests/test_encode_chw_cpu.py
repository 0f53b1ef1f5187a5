"""BT709HIP_CTX_OPT_ENCODE_CHW_INPUT (bt709hip_encode[_batch] of planar CHW_U8 / _F16 / _F32 surfaces), the parts that
need no GPU: the enumerators and the ABI, the header's contract, the domains of the seven options, the closed gate, and -- on the shim
built against the fake HIP runtime (tests/native/fake_hip/) -- one launch per call, every validation code in the encoder's order, the
refusals, mixed batches, the table limit, the uniform path and the plan; the argument block a CHW call hands the launcher (a probe
in front of the fake launcher: tests/native/encode_chw_probe.cpp); the host replay of csrc/bt709_chw_denorm.h against the numpy
restatement; the round trip with csrc/bt709_chw_norm.h; the Python mirror; the generated code of the new kernels.  On a tree without
the feature the tests here fail at the first set_option (BT709HIP_ERR_INVALID_ARG), at the missing binding, header or kernel.

The fake runtime's launcher reports one name for every encoder kernel, so the twelve kernel names are held against the launch table's
strings in the built library here and asserted call by call in tests/test_encode_chw_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_headers
import chw_cases as cc
import encode_chw_cases as ec
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "metalbt709decoder_amd", "csrc")
OPT, NORM_OPTS = 18, list(range(20, 26))  # stated here, not taken from the bindings
ROW_PAIRS_OPT, THREADS_OPT, LAYOUT_OPT, PREMULTIPLY_OPT, CONVERT_OPT, WITH_ALPHA_OPT, HALF_OPT, HALF_WITH_ALPHA_OPT = 2, 3, 6, 8, 10, 12, 14, 16
U8, F16, F32, BGRA8, HALF = 4, 5, 6, 0, 1
ELEM = {U8: 1, F16: 2, F32: 4}
APPLE, SRGB, LIN = 0, 1, 2
W, H = 64, 16
NAMES = ["encode_chw_%s%s<%s>" % (l, b, e) for l in ("nv12", "i420") for b in ("", "_blocks") for e in ("u8", "f16", "f32")]


# ------------------------------------------------------------------ ids, the header

def test_enumerators_and_bindings_agree_and_nothing_was_exported(tmp_path):
    names = ["BT709HIP_CTX_OPT_ENCODE_CHW_INPUT"] + ["BT709HIP_CTX_OPT_ENCODE_CHW_%s_%s" % (k, c) for k in ("SCALE", "BIAS") for c in "RGB"]
    src, exe = tmp_path / "ids.c", tmp_path / "ids"
    src.write_text('#include <stdio.h>\n#include "bt709hip_ext.h"\nint main(void) {\n  printf("%s\\n", %s, (int)BT709HIP_VERSION);\n  return 0;\n}\n'
                   % (" ".join(["%d"] * 8), ", ".join("(int)" + n for n in names)))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ids = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert ids == [OPT] + NORM_OPTS + [504]
    assert _capi.CTX_OPT_ENCODE_CHW_INPUT == OPT == ec.OPT_CHW_INPUT and _capi.ABI_VERSION == 504
    assert [_capi.CTX_OPT_ENCODE_CHW_SCALE_R, _capi.CTX_OPT_ENCODE_CHW_SCALE_G, _capi.CTX_OPT_ENCODE_CHW_SCALE_B, _capi.CTX_OPT_ENCODE_CHW_BIAS_R,
            _capi.CTX_OPT_ENCODE_CHW_BIAS_G, _capi.CTX_OPT_ENCODE_CHW_BIAS_B] == NORM_OPTS
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103 == len(_capi.SYMBOLS)  # no export
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    for word in ("kEncodeCHWInputOption = BT709HIP_CTX_OPT_ENCODE_CHW_INPUT", "setEncodeCHWNormalisation(", "setEncodeCHWMeanStd(", "convertCHWIntoCoreVideoBuffers("):
        assert word in hpp, word


def test_header_states_the_contract():
    text = abi_headers.ext_text()
    comment = re.search(r"/\* PLANAR CHW INPUT.*?\*/", text, flags=re.S).group(0)
    for word in ("BT709HIP_CTX_OPT_ENCODE_CHW_INPUT", "ins[0]", "BT709HIP_ERR_SIZE_MISMATCH", "e-aligned", "64-bit product", "NEVER read", "no fused multiply-add",
                 "NaN -> 0", "+inf", "(int)round(x * 255.0f)", "byte for byte", "(s_B, s_G, s_R, 255)", "BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT", "20, 21, 22",
                 "23, 24, 25", "BIT PATTERN", "2^-64", "BT709HIP_ERR_INVALID_ARG", "INVERSE", "(std, mean)", "kernel arguments", "CHW_U8 ignores them",
                 "no getter", "BT709HIP_ERR_STRIDE", "_ENCODE_ROW_PAIRS", "_ENCODE_THREADS", "_XCD_BANDS", "BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY", "_ENCODE_CONVERT",
                 "_ENCODE_WITH_ALPHA", "_ENCODE_HALF_WITH_ALPHA", "BT709HIP_ERR_UNSUPPORTED", "BT709HIP_CTX_OPT_ENCODE_HALF_INPUT is independent", "65535",
                 "BT709HIP_MAX_BATCH - 1 = 31", "general kernel", "bt709hip_last_launch_info", "not clamped", "never touches the device", "OUT OF SCOPE",
                 "linear light", "fourth plane", "straight-alpha tensors", "HWC tensors", "encode_chw_nv12<u8>", "encode_chw_i420<f32>", "encode_chw_nv12_blocks<f16>"):
        assert word in comment, word
    targets = re.search(r"/\* PLANAR CHW TARGETS\..*?\*/", text, flags=re.S).group(0)
    assert "as OUTPUT alone" not in targets and "as INPUT by bt709hip_encode" in targets


def test_the_twelve_kernel_names_are_the_launch_tables():
    from metalbt709decoder_amd import build
    blob = open(build.build(), "rb").read()
    for name in NAMES:
        assert name.encode() + b"\0" in blob, name


# ------------------------------------------------------------------ the shim on the fake HIP runtime

class Probe(C.Structure):  # tests/native/encode_chw_probe.cpp encode_chw_probe_record
    _fields_ = [("scale_bias", C.c_uint32 * 6), ("input_format", C.c_int32), ("fast", C.c_int32), ("frames", C.c_int32), ("uniform", C.c_int32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("bgra_stride", C.c_uint32), ("chroma_layout", C.c_uint32), ("premultiply", C.c_uint32),
                ("convert_mode", C.c_uint32), ("first_bgra", C.c_void_p), ("last_table_bgra", C.c_void_p), ("step_bgra", C.c_int64),
                ("params_bytes", C.c_uint32), ("table_entries", C.c_uint32)]


@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    """The shim on the fake runtime, with the probe in front of the fake launch_encode: fake_hip.cpp is compiled with its
    launch_encode renamed, the probe defines the name the shim calls."""
    from test_fake_hip import CXX, FAKE, SHIM_SOURCES, FakeOp
    d = tmp_path_factory.mktemp("fake_encode_chw")
    obj, so = str(d / "fake_hip.o"), str(d / "libbt709hip_fake.so")
    r = subprocess.run(CXX + ["-fPIC", "-c", "-Dlaunch_encode=fake_hip_launch_encode", os.path.join(FAKE, "fake_hip.cpp"), "-o", obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    sources = [s for s in SHIM_SOURCES if not s.endswith("fake_hip.cpp")] + [os.path.join(HERE, "native", "encode_chw_probe.cpp"), obj]
    r = subprocess.run(CXX + ["-shared", "-fPIC", "-I" + CSRC] + sources + ["-o", so, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_allocations.restype = C.c_uint64
    lib.encode_chw_probe_last.argtypes = [C.POINTER(Probe)]
    lib.fake_hip_set_device_count(1)
    return lib


class Rig:
    """A context and two allocations, tensors and frames (launches touch nothing on the fake runtime, so pictures may overlap)."""

    def __init__(self, lib):
        self.lib = lib
        self.ctx = C.c_void_p()
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0
        self.src, self.dst = C.c_void_p(), C.c_void_p()
        for p in (self.src, self.dst):
            assert lib.bt709hip_malloc(self.ctx, 1 << 20, C.byref(p)) == 0

    def set(self, value, option=OPT):
        return self.lib.bt709hip_context_set_option(self.ctx, option, value)

    def surfs(self, n=1, fmt=F16, w=W, h=H, step=None, stride=None, base=0):
        e = ELEM.get(fmt, 8 if fmt == HALF else 4)
        stride = e * w if stride is None else stride
        step = 3 * stride * h if step is None else step
        return (_capi.Surface * n)(*[_capi.Surface(self.src.value + base + i * step, stride, w, h, fmt, 0) for i in range(n)])

    def frames(self, n=1, w=W, h=H, step=W * H * 2, cbcr_stride=None):
        return (_capi.Frame * n)(*[_capi.Frame(self.dst.value + i * step, w, self.dst.value + i * step + W * H, cbcr_stride or w, w, h, 0, 0) for i in range(n)])

    def encode(self, n, surfs, frames, gi=SRGB, go=APPLE, stream=None, wait=1):
        if n == 1:
            return self.lib.bt709hip_encode(self.ctx, surfs, frames, gi, go, stream, wait)
        return self.lib.bt709hip_encode_batch(self.ctx, n, surfs, frames, gi, go, stream, wait)

    def kernels(self, mark):
        from test_fake_hip import log
        return [o for o in log(self.lib, mark) if o[0].startswith("kernel:")]

    def launch(self):
        info = _capi.LaunchInfo()
        assert self.lib.bt709hip_last_launch_info(C.byref(info)) == 0
        return tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands

    def probe(self):
        p = Probe()
        self.lib.encode_chw_probe_last(C.byref(p))
        return p

    def close(self):
        for p in (self.src, self.dst):
            assert self.lib.bt709hip_free(self.ctx, p) == 0
        assert self.lib.bt709hip_context_destroy(self.ctx) == 0


@pytest.fixture()
def rig(fake):
    r = Rig(fake)
    yield r
    r.close()


def held(rig, fmt=F16):
    """There is no getter: the held value shows in what the next call does with CHW input."""
    rc = rig.encode(1, rig.surfs(fmt=fmt), rig.frames())
    assert rc in (0, _capi.ERR_UNSUPPORTED)
    return 0 if rc else 1


def test_option_domains(fake, rig):
    lib = fake
    assert lib.bt709hip_context_set_option(None, OPT, 1) == _capi.ERR_INVALID_ARG
    assert held(rig) == 0
    for value in (1, 0, 1):
        mark = lib.fake_hip_log_size()
        assert rig.set(value) == _capi.OK
        for bad in (2, -1, 1 << 30):
            assert rig.set(bad) == _capi.ERR_INVALID_ARG, bad  # refused, not clamped ...
        assert lib.fake_hip_log_size() == mark                 # setting it never touches the device
        assert all(held(rig, f) == value for f in (U8, F16, F32))  # ... and the option keeps its value
    for other in (17, 19, 26, 27):  # the ids around the seven are no options
        for v in (0, 1, cc.bits(1.0)):
            assert rig.set(v, other) == _capi.ERR_INVALID_ARG, other
    # the six values: float32 bit patterns, +-0 or finite with 2^-64 <= |x| <= 2^64; a refused value changes nothing
    sub = int(np.array([1], np.uint32).view(np.int32)[0])
    bad = [cc.bits(np.nan), cc.bits(np.inf), cc.bits(-np.inf), cc.bits(2.0 ** -65), cc.bits(-2.0 ** 65), sub, cc.bits(2.0 ** 64) + 1, cc.bits(2.0 ** -64) - 1]
    good = [cc.bits(-0.0), cc.bits(0.0), cc.bits(-2.5), cc.bits(2.0 ** 64), cc.bits(-2.0 ** -64), cc.bits(0.229), cc.bits(0.485)]
    assert [rig.probe().params_bytes, rig.probe().table_entries] == [880, ec.MAX_TABLE]  # the argument block did not grow
    assert list(rig.probe().scale_bias) == [cc.bits(1.0)] * 3 + [0] * 3  # the defaults, as the last call carried them
    mark = lib.fake_hip_log_size()
    for i, opt in enumerate(NORM_OPTS):
        for value in good:
            assert rig.set(value, opt) == _capi.OK, (opt, value)
            for b in bad:
                assert rig.set(b, opt) == _capi.ERR_INVALID_ARG, (opt, hex(b & 0xFFFFFFFF))
        assert lib.fake_hip_log_size() == mark
        assert rig.encode(1, rig.surfs(), rig.frames()) == 0
        mark = lib.fake_hip_log_size()
        assert rig.probe().scale_bias[i] == good[-1] & 0xFFFFFFFF
    assert lib.bt709hip_abi_version() == 504


def test_with_the_gate_closed_chw_input_is_the_unknown_format(fake, rig):
    mark = fake.fake_hip_log_size()
    for n in (1, 3):
        for gi, go in ((SRGB, APPLE), (LIN, LIN)):
            unknown = rig.encode(n, rig.surfs(n, fmt=7), rig.frames(n), gi, go)
            assert unknown != 0
            for fmt in (U8, F16, F32):
                assert rig.encode(n, rig.surfs(n, fmt=fmt), rig.frames(n), gi, go) == unknown, (n, fmt)
    assert rig.set(1, HALF_OPT) == 0  # the other gate does not open this one
    assert rig.encode(1, rig.surfs(fmt=F16), rig.frames(), LIN, APPLE) == _capi.ERR_UNSUPPORTED
    assert rig.set(0, HALF_OPT) == 0
    assert fake.fake_hip_log_size() == mark


@pytest.mark.parametrize("fmt", [U8, F16, F32])
def test_calls_are_one_launch_each_and_the_arguments_arrive(fake, rig, fmt):
    e = ELEM[fmt]
    assert rig.set(1) == 0
    values = [0.229, 0.224, 0.225, 0.485, 0.456, -0.0]
    for opt, v in zip(NORM_OPTS, values):
        assert rig.set(cc.bits(v), opt) == 0
    mark = fake.fake_hip_log_size()
    for gi, go in ((SRGB, APPLE), (APPLE, SRGB), (LIN, LIN)):  # all three input gammas: the path starts from a byte
        assert rig.encode(1, rig.surfs(fmt=fmt), rig.frames(), gi, go) == 0
    p = rig.probe()
    assert (p.input_format, p.fast, p.frames, p.uniform, p.width, p.height, p.bgra_stride) == (2 + fmt - U8, 1, 1, 0, W, H, W * e)
    assert [v for v in p.scale_bias] == [cc.bits(v) & 0xFFFFFFFF for v in values] and (p.premultiply, p.convert_mode, p.chroma_layout) == (0, 0, 0)
    assert rig.encode(4, rig.surfs(4, fmt=fmt), rig.frames(4)) == 0
    assert rig.set(_capi.CHROMA_I420, LAYOUT_OPT) == 0
    assert rig.encode(2, rig.surfs(2, fmt=fmt), rig.frames(2, cbcr_stride=W // 2)) == 0
    assert rig.probe().chroma_layout == 1
    assert rig.set(_capi.CHROMA_NV12, LAYOUT_OPT) == 0
    assert rig.encode(1, rig.surfs(fmt=fmt, w=0, h=0), rig.frames(w=0, h=0)) == 0  # an empty picture: nothing to do
    assert [k[2] for k in rig.kernels(mark)] == [1, 1, 1, 4, 2]
    # the fast / general choice: width % 4, plane 0 and the pitch 4 e-aligned, the frame as encode_bgra needs it
    for label, surfs, frames, fast in (("aligned", rig.surfs(fmt=fmt), rig.frames(), 1), ("padded by 4 e", rig.surfs(fmt=fmt, stride=W * e + 4 * e), rig.frames(), 1),
                                       ("base + e", rig.surfs(fmt=fmt, base=e), rig.frames(), 0), ("base + 2 e", rig.surfs(fmt=fmt, base=2 * e), rig.frames(), 0),
                                       ("pitch = e mod 4 e", rig.surfs(fmt=fmt, stride=W * e + e), rig.frames(), 0),
                                       ("W = 6", rig.surfs(fmt=fmt, w=6, stride=32), rig.frames(w=6), 0), ("Y pitch", rig.surfs(fmt=fmt), None, 0)):
        if frames is None:
            frames = rig.frames()
            frames[0].y_stride = W + 2
        assert rig.encode(1, surfs, frames) == 0, label
        assert rig.probe().fast == fast, label
    # a contiguous NCHW tensor of 70 images: the uniform path, more than any table holds; and 5 images of a 4-plane tensor
    for n, planes in ((70, 3), (5, 4)):
        small = rig.surfs(n, fmt=fmt, w=8, h=2, step=planes * 8 * e * 2)
        assert rig.encode(n, small, rig.frames(n, w=8, h=2, step=32)) == 0
        p = rig.probe()
        assert (p.uniform, p.frames, p.step_bgra, p.first_bgra) == (1, n, planes * 8 * e * 2, small[0].bgra)
    # the plan is the BGRA8 encoder's for the same size and count, under the launch options too
    for options in ({}, {ROW_PAIRS_OPT: 5}, {THREADS_OPT: 64}):
        for o, v in options.items():
            assert rig.set(v, o) == 0
        for n, w, h in ((1, W, H), (3, 1024, 64), (64, 8, 4)):
            assert rig.encode(n, rig.surfs(n, fmt=fmt, w=w, h=h, step=4096 if n == 64 else None), rig.frames(n, w=w, h=h, step=64 if n == 64 else W * H * 2)) == 0
            plan = rig.launch()
            assert rig.encode(n, rig.surfs(n, fmt=BGRA8, w=w, h=h, step=4096 if n == 64 else None), rig.frames(n, w=w, h=h, step=64 if n == 64 else W * H * 2)) == 0
            assert rig.launch() == plan and plan[2] == 1, (n, w, h, plan)
        for o in options:
            assert rig.set(0, o) == 0


def test_every_refusal_alone_and_in_a_batch_enqueues_nothing(fake, rig):
    lib = fake
    assert rig.set(1) == 0
    for gi, go in ((SRGB, APPLE), (LIN, LIN)):
        assert lib.bt709hip_encoder_prepare(rig.ctx, gi, go) == 0
    mark = lib.fake_hip_log_size()

    def call(n, fmt, edit_surf=None, edit_frame=None, gi=SRGB, go=APPLE, **kw):
        surfs, frames = rig.surfs(n, fmt=fmt, **kw), rig.frames(n, **{k: v for k, v in kw.items() if k in ("w", "h")})
        if edit_surf:
            edit_surf(surfs[n - 1])
        if edit_frame:
            edit_frame(frames[n - 1])
        return rig.encode(n, surfs, frames, gi, go)

    def put(name, value):
        return lambda s: setattr(s, name, value)

    for fmt in (U8, F16, F32):
        e = ELEM[fmt]
        for n in (1, 3):
            whole = n == 1  # a pitch is one per call: changed in one picture of a batch it is a size mismatch first, as for BGRA8 input
            same = lambda code: code if whole else _capi.ERR_SIZE_MISMATCH
            # the encoder's order: sizes, odd dimensions, the grid limit, the format, the batch's sameness, NULLs, strides
            assert call(n, fmt, put("width", -2)) == _capi.ERR_INVALID_ARG
            assert call(n, fmt, edit_frame=put("width", W + 2)) == _capi.ERR_SIZE_MISMATCH
            assert call(n, fmt, w=W - 1) == _capi.ERR_ODD_DIMENSIONS
            assert call(n, fmt, w=2, h=131072) == call(n, BGRA8, w=2, h=131072) == _capi.ERR_UNSUPPORTED  # H/2 = 65536 row pairs
            assert call(n, fmt, put("reserved", 1)) == _capi.ERR_UNSUPPORTED
            assert call(n, fmt, put("format", 7)) == _capi.ERR_UNSUPPORTED
            assert call(n, fmt, put("bgra", None)) == _capi.ERR_INVALID_ARG
            assert call(n, fmt, edit_frame=put("y", None)) == _capi.ERR_INVALID_ARG
            assert call(n, fmt, edit_frame=put("cbcr", None)) == _capi.ERR_INVALID_ARG
            assert call(n, fmt, put("stride", W * e - e)) == same(_capi.ERR_STRIDE)       # a pitch below W e
            assert call(n, fmt, put("stride", 1 << 32)) == same(_capi.ERR_STRIDE)         # a pitch the launch cannot carry in 32 bits
            assert call(n, fmt, edit_frame=put("y_stride", W - 1)) == same(_capi.ERR_STRIDE)
            if e > 1:
                assert call(n, fmt, put("stride", W * e + 1)) == same(_capi.ERR_STRIDE)   # a pitch that is no multiple of e
                assert call(n, fmt, put("bgra", rig.src.value + 1)) == _capi.ERR_STRIDE   # a base that is not e-aligned
                assert call(n, fmt, put("bgra", rig.src.value + e // 2)) == _capi.ERR_STRIDE
            for go in (3, 4, -1):  # output gammas outside the encoder's three: what the BGRA8 encoder answers
                assert call(n, fmt, go=go) == call(n, BGRA8, go=go) == _capi.ERR_INVALID_ARG
            if n > 1:  # mixed formats in a batch, either way round
                for other in (BGRA8,) + tuple(o for o in (U8, F16, F32) if o != fmt):
                    assert call(n, fmt, put("format", other), stride=W * 4) == _capi.ERR_SIZE_MISMATCH, other
                    assert call(n, other, put("format", fmt), stride=W * 4) == _capi.ERR_SIZE_MISMATCH, other
            # the options that are out of scope, each away from its default: behind the usual validation
            for option, value in ((PREMULTIPLY_OPT, 1), (CONVERT_OPT, _capi.CONVERT_PACKED444), (CONVERT_OPT, _capi.CONVERT_POINT420), (WITH_ALPHA_OPT, 1),
                                  (HALF_WITH_ALPHA_OPT, 1)):
                assert rig.set(value, option) == 0
                try:
                    assert call(n, fmt) == _capi.ERR_UNSUPPORTED, (option, value)
                    assert call(n, fmt, w=W - 1) == _capi.ERR_ODD_DIMENSIONS  # ... which still comes first
                    assert call(n, fmt, put("stride", W * e - e)) == same(_capi.ERR_STRIDE)
                    assert call(n, fmt, put("bgra", None)) == _capi.ERR_INVALID_ARG
                finally:
                    assert rig.set(0, option) == 0
        # the pointer table of a CHW launch holds 31 surfaces
        uneven = rig.surfs(ec.MAX_TABLE + 1, fmt=fmt, w=8, h=2, step=256)
        uneven[5].bgra += 16
        assert rig.encode(ec.MAX_TABLE + 1, uneven, rig.frames(ec.MAX_TABLE + 1, w=8, h=2, step=32)) == _capi.ERR_UNSUPPORTED
    assert rig.kernels(mark) == [] and lib.fake_hip_log_size() == mark, "a refused call enqueued something"
    for fmt in (U8, F32):
        uneven = rig.surfs(ec.MAX_TABLE, fmt=fmt, w=8, h=2, step=256)
        uneven[5].bgra += 16
        mark = lib.fake_hip_log_size()
        assert rig.encode(ec.MAX_TABLE, uneven, rig.frames(ec.MAX_TABLE, w=8, h=2, step=32)) == 0
        p = rig.probe()
        assert [k[2] for k in rig.kernels(mark)] == [ec.MAX_TABLE] and (p.uniform, p.last_table_bgra) == (0, uneven[ec.MAX_TABLE - 1].bgra)
        assert list(p.scale_bias) == [cc.bits(1.0)] * 3 + [0] * 3  # the table's last entry did not run into the six values
    # RGBA16F input stays independent: its gate, its gamma rule; BGRA8 keeps its 32
    assert rig.encode(1, rig.surfs(fmt=HALF), rig.frames(), LIN, APPLE) == _capi.ERR_UNSUPPORTED
    assert rig.set(1, HALF_OPT) == 0
    assert rig.encode(1, rig.surfs(fmt=HALF), rig.frames(), LIN, APPLE) == 0 and rig.encode(1, rig.surfs(fmt=F16), rig.frames(), LIN, APPLE) == 0
    assert rig.set(0, HALF_OPT) == 0
    uneven = rig.surfs(32, fmt=BGRA8, w=8, h=2, step=256)
    uneven[5].bgra += 16
    assert rig.encode(32, uneven, rig.frames(32, w=8, h=2, step=32)) == 0


def test_bgra8_calls_issue_the_same_launches_with_the_gate_at_either_value(fake, rig):
    from test_fake_hip import log
    issued = {}
    for value in (0, 1):
        assert rig.set(value) == 0
        mark = fake.fake_hip_log_size()
        records = []
        for n, fmt, gi, go in ((1, BGRA8, SRGB, APPLE), (4, BGRA8, SRGB, SRGB), (1, 3, LIN, LIN)):
            assert rig.encode(n, rig.surfs(n, fmt=fmt, step=4 * W * H), rig.frames(n), gi, go) == 0
            records.append(rig.launch())
        issued[value] = ([(o[0], o[2], o[3]) for o in log(fake, mark)], records)
    assert issued[0] == issued[1] and len(issued[0][0]) == 3


# ------------------------------------------------------------------ host replay of csrc/bt709_chw_denorm.h

@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chw_denorm") / "chw_denorm_sweep")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + CSRC, os.path.join(HERE, "native", "chw_denorm_sweep.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(mode, *floats, data=None):
        args = ["%08x" % (cc.bits(v) & 0xFFFFFFFF) for v in floats]
        out = subprocess.run([exe, mode] + args, input=b"" if data is None else data.tobytes(), capture_output=True)
        assert out.returncode == 0, out.stderr
        return np.frombuffer(out.stdout, np.uint8)
    return run


def channel_pairs():
    return [(float(s[0][c]), float(s[1][c])) for s in ec.SETTINGS.values() for c in range(3)]


def test_numpy_definition_by_hand():
    f = lambda t, s=1.0, b=0.0: int(ec.byte_of(np.array([t], np.float32), s, b)[0])
    assert [f(np.nan), f(-0.0), f(-1.0), f(np.inf), f(-np.inf), f(2.0), f(1.0), f(0.5), f(0.0)] == [0, 0, 0, 255, 0, 255, 255, 128, 0]
    assert f(np.inf, 0.0) == 0 and f(np.inf, 1.0, -np.inf) == 0  # inf * 0 and inf - inf are NaN
    assert f(0.5 / 255) == 1 and f(np.nextafter(np.float32(0.5 / 255), np.float32(0))) in (0, 1)
    x = np.array([0x3B008080], np.uint32).view(np.float32)  # v = 0x1.fffffep-2: v + 0.5f would round up, the exact form gives 0
    assert int(ec.quantise(x)[0]) == 0
    assert int(ec.byte_of(np.array([0x7E00], np.uint16).view(np.float16), 1.0, 0.0)[0]) == 0
    assert [int(v) for v in ec.byte_of(np.array([3, 200], np.uint8), 5.0, 7.0)] == [3, 200]  # u8 ignores the pair


def test_host_replay_over_every_half_code(sweep):
    codes = np.arange(65536, dtype=np.uint16)
    values = np.frombuffer(sweep("value", 1.0, 0.0, data=codes).tobytes(), np.uint32)
    want = codes.view(np.float16).astype(np.float32).view(np.uint32)
    nan = np.isnan(codes.view(np.float16))
    assert np.array_equal(values[~nan], want[~nan]) and np.isnan(values.view(np.float32)[nan]).all()  # a half converts exactly
    for scale, bias in channel_pairs():
        got = sweep("half", scale, bias)
        assert got.size == 65536
        assert np.array_equal(got, ec.byte_of(codes.view(np.float16), scale, bias)), (scale, bias)
    assert np.unique(sweep("half", 1.0, 0.0)).size == 256


def test_host_replay_over_float32_edges_and_random_patterns(sweep):
    rng = np.random.default_rng(22)
    edges = ec.float_edges()
    assert edges.size >= 256 * 7 + 30
    patterns = np.concatenate([edges, rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32),
                               (rng.integers(0x3A800000, 0x3F900000, 1 << 18, dtype=np.uint64)).astype(np.uint32)])  # and a crowd inside [2^-10, 1.1]
    for scale, bias in channel_pairs():
        got = sweep("f32", scale, bias, data=patterns)
        want = ec.byte_of(patterns.view(np.float32), scale, bias)
        assert np.array_equal(got, want), (scale, bias, patterns[np.flatnonzero(got != want)[:4]])
    # under the identity the thresholds sit where the definition puts them: (k + 0.5) / 255 itself rounds away
    mid = ((np.arange(255) + 0.5) / 255.0).astype(np.float32)
    exact = mid.astype(np.float64) * 255.0 >= np.arange(255) + 0.5 - 1e-12
    got = sweep("f32", 1.0, 0.0, data=mid.view(np.uint32))
    assert np.array_equal(got, ec.byte_of(mid, 1.0, 0.0)) and set(np.unique(got.astype(int) - np.arange(255))) <= {0, 1} and exact.any()


def test_round_trip_with_the_decode_side_is_the_identity(sweep):
    """chw_norm then the de-normalisation over all 256 codes, in float32 and through binary16: the identity for (1, 0) -- required:
    the binary16 error is at most 2^-11 * 255 ~ 0.12 of a code -- and, per channel, for the ImageNet constants (decode side
    (1 / std, -mean / std), this side (std, mean)), where the same bound scaled by |t| * std gives ~0.15 of a code."""
    code = np.arange(256, dtype=np.uint8)
    for mode in ("trip32", "trip16"):
        assert np.array_equal(sweep(mode, 1.0, 0.0, 1.0, 0.0), code), mode
        for c in range(3):
            got = sweep(mode, cc.IMAGENET[0][c], cc.IMAGENET[1][c], ec.IMAGENET[0][c], ec.IMAGENET[1][c])
            assert np.array_equal(got, code), (mode, c, np.flatnonzero(got != code))
    # the numpy restatements agree with the replay
    for c in range(3):
        t = cc.norm(code, cc.IMAGENET[0][c], cc.IMAGENET[1][c])
        assert np.array_equal(ec.byte_of(t, ec.IMAGENET[0][c], ec.IMAGENET[1][c]), code)
        assert np.array_equal(ec.byte_of(t.astype(np.float16), ec.IMAGENET[0][c], ec.IMAGENET[1][c]), code)


# ------------------------------------------------------------------ the Python mirror

def test_python_mirror_sets_and_restores_the_gate():
    calls = []

    class Lib:
        rc = _capi.OK

        def bt709hip_context_set_option(self, handle, option, value):
            calls.append(("set", option, value))
            return _capi.OK

        def bt709hip_encode_batch(self, handle, n, surfs, frames, gi, go, stream, wait):
            calls.append(("encode", n, [s.format for s in surfs], [s.stride for s in surfs], gi, go))
            if isinstance(self.rc, Exception):
                raise self.rc
            return self.rc

    ctx = mb.MetalRenderContext(0)
    ctx.lib, ctx.handle = Lib(), 1
    try:
        conv = mb.BGRAToBT709Converter
        texs = [mb.CHWTexture(ctx, W, H, "float16", planes=4, ptr=0x10000 * (i + 1)) for i in range(2)]
        outs = [mb.CVPixelBuffer(ctx, W, H, planes=(0x100000 * (i + 1), 0x100000 * (i + 1) + W * H)) for i in range(2)]
        assert conv.convertCHWIntoCoreVideoBuffers(texs, outs, SRGB, APPLE)
        assert calls == [("set", OPT, 1), ("encode", 2, [F16, F16], [2 * W, 2 * W], SRGB, APPLE), ("set", OPT, 0)]
        del calls[:]
        ctx.lib.rc = _capi.ERR_STRIDE  # a refused call: False, the gate back at 0
        assert not conv.convertCHWIntoCoreVideoBuffers(texs, outs, SRGB, APPLE)
        assert calls[0] == ("set", OPT, 1) and calls[-1] == ("set", OPT, 0)
        del calls[:]
        ctx.lib.rc = RuntimeError("the call raised")
        with pytest.raises(RuntimeError):
            conv.convertCHWIntoCoreVideoBuffers(texs, outs, SRGB, APPLE)
        assert calls[0] == ("set", OPT, 1) and calls[-1] == ("set", OPT, 0)
        del calls[:]
        ctx.lib.rc = _capi.OK
        assert not conv.convertCHWIntoCoreVideoBuffers([mb.BGRATexture(ctx, W, H, ptr=0x90000)], outs[:1], SRGB, APPLE) and calls == []
        with pytest.raises(ValueError):
            conv.convertCHWIntoCoreVideoBuffers(texs, outs[:1], SRGB, APPLE)
        planar = [mb.CVPixelBuffer(ctx, W, H, planes=(0x300000, 0x300000 + W * H), planar=True)]
        assert conv.convertCHWIntoCoreVideoBuffers(texs[:1], planar, LIN, LIN)
        assert calls[0] == ("set", LAYOUT_OPT, _capi.CHROMA_I420) and calls[1:] == [("set", OPT, 1), ("encode", 1, [F16], [2 * W], LIN, LIN), ("set", OPT, 0)]
        del calls[:]
        # the setters: float32 bit patterns, (std, mean) as they are, refused outside the domain with nothing set
        assert ctx.setEncodeCHWMeanStd(cc.IMAGENET_MEAN, cc.IMAGENET_STD)
        assert calls == [("set", 20 + i, cc.bits(v)) for i, v in enumerate(cc.IMAGENET_STD + cc.IMAGENET_MEAN)]
        del calls[:]
        assert ctx.setEncodeCHWNormalisation((2.0, -3.0, 0.5), (-0.0, 0.25, 7.0))
        assert calls == [("set", 20 + i, cc.bits(v)) for i, v in enumerate((2.0, -3.0, 0.5, -0.0, 0.25, 7.0))]
        del calls[:]
        for bad in (((1.0, np.inf, 1.0), (0.0,) * 3), ((1.0,) * 3, (0.0, 2.0 ** 65, 0.0)), ((1.0, 1.0), (0.0,) * 3)):
            with pytest.raises(ValueError):
                ctx.setEncodeCHWNormalisation(*bad)
        assert calls == []
        assert "setCHWMeanStd" in mb.MetalRenderContext.setEncodeCHWMeanStd.__doc__ and "inverse" in mb.MetalRenderContext.setEncodeCHWMeanStd.__doc__
    finally:
        ctx.handle = None


# ------------------------------------------------------------------ the generated code

def kernel(asm, name, layout, elem):
    sym = "_ZN5bt709%d%sILj%dELj%dEEEvNS_12EncodeParamsE" % (len(name), name, layout, elem)
    assert len(re.findall(r"^%s:" % sym, asm, re.M)) == 1, sym
    body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % sym, asm, re.S | re.M).group(1)
    ins = [l.split(";")[0].strip() for l in body.split("\n")]
    meta = re.search(r"\.name:\s+%s\b.*?(?=\n  - \.a|\Z)" % re.escape(sym), asm, flags=re.S).group(0)
    block = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), asm, re.S).group(1)
    return [l for l in ins if l and not l.startswith(".") and not l.endswith(":")], meta, {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", block)}


FUSED = r"v_(?:pk_)?(?:fma|fmac|fmamk|fmaak|mad|mac|madmk|madak)_(?:f32|f16|legacy|mix)"


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("elem", [1, 2, 3])
def test_isa_of_the_chw_encode_kernels(layout, elem):
    """No fused multiply-add on the de-normalisation: the only ones are div_const's two per chroma sample, the BGRA8 kernels' count
    (a quad: two blocks x two samples x two; a block: four).  Six plane loads per row pair and their six prefetched twins, of 4, 8 or
    16 bytes, non-temporal; nothing spilled; the argument block did not grow; stores as encode_bgra's."""
    from metalbt709decoder_amd import build
    asm = open(build.emit_asm()).read()
    load_of = {1: "global_load_dword", 2: "global_load_dwordx2", 3: "global_load_dwordx4"}
    ins, meta, kd = kernel(asm, "encode_chw", layout, elem)
    fused = [i for i in ins if re.match(FUSED, i)]
    assert len(fused) == 8 and all(i.split()[0] in ("v_fmac_f32_e32", "v_fma_f32") for i in fused), fused
    assert not [i for i in ins if re.match(r"v_pk_(mul|add|fma)_f32|scratch_|flat_|buffer_", i)]
    plane_loads = [i for i in ins if i.startswith("global_load") and re.search(r"\bnt\b", i)]
    assert len(plane_loads) == 12 and all(i.split()[0] == load_of[elem] for i in plane_loads), plane_loads
    assert kd["kernarg_size"] == 880 + 256 and kd["private_segment_fixed_size"] == 0 and kd["group_segment_fixed_size"] == 0
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= (64 if elem < 3 else 72)
    stores = sorted(i.split()[0].replace("_d16_hi", "") for i in ins if i.startswith("global_store"))
    assert stores == (["global_store_dword"] * 2 + ["global_store_short"] * 2 if layout else ["global_store_dword"] * 3), stores
    if elem > 1:  # twelve values a row pair and plane pair: 24 products, 24 sums, each on its own
        assert len([i for i in ins if re.match(r"v_mul_f32", i)]) >= 24 and len([i for i in ins if re.match(r"v_add_f32", i)]) >= 24
    if elem == 2:
        assert len([i for i in ins if i.startswith("v_cvt_f32_f16")]) == 24
    ins, meta, kd = kernel(asm, "encode_chw_blocks", layout, elem)
    fused = [i for i in ins if re.match(FUSED, i)]
    assert len(fused) == 4 and all(i.split()[0] in ("v_fmac_f32_e32", "v_fma_f32") for i in fused), fused
    assert kd["kernarg_size"] == 880 + 256 and kd["private_segment_fixed_size"] == 0
    stores = [i.split()[0] for i in ins if i.startswith(("global_store", "flat_store", "buffer_store"))]
    stores = sorted(s.replace("_d16_hi", "") for s in stores)
    # Y: four byte stores; chroma: a byte to each of U and V, or -- NV12, as encode_bgra_blocks -- the Cb Cr pair as one 2-byte store
    # at whatever address the row has (legal on gfx950)
    assert stores == (["global_store_byte"] * 6 if layout else ["global_store_byte"] * 4 + ["global_store_short"]), stores
    loads = {i.split()[0] for i in ins if i.startswith("global_load") and "off" in i and not i.startswith("global_load_dwordx4")}
    assert loads <= {{1: "global_load_ubyte", 2: "global_load_ushort", 3: "global_load_dword"}[elem], "global_load_ushort", "global_load_dword", "global_load_dwordx2",
                     "global_load_ubyte_d16", "global_load_ubyte_d16_hi", "global_load_short_d16", "global_load_short_d16_hi"}, loads
