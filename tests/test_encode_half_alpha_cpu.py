"""BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA (bt709hip_encode[_batch] of an RGBA16Float surface into its colour frame AND its alpha
frame), the parts that need no GPU: the enumerator and the ABI, the header's contract, the option's domain and every
validation row of a paired half call on the fake HIP runtime (tests/native/fake_hip/) alone and in a batch, the capture rule, the
Python mirror's set-and-restore of both options, the definition reduced to T[round(255 sat(a))] and Cb = Cr = 128 from the oracle
composition, the device's alpha step replayed on the host over all 65536 half codes, the descriptors of the new fast kernels, and
the round trip through the decoder's RGBA16F alpha.  On a tree without the option the tests here fail at the first set_option
(BT709HIP_ERR_INVALID_ARG), at the missing binding, header or kernel.

The fake runtime's launcher reports one name for every encoder kernel, so the four kernel names are held against the launch table's
strings in the built library here and asserted call by call in tests/test_encode_half_alpha_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_headers
import encode_half_alpha_cases as ac
import encode_half_cases as hc
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_APPLE, GAMMA_LINEAR, GAMMA_SRGB
from test_encode_half_cpu import Rig, descriptor, kernel, meta_int

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "metalbt709decoder_amd", "csrc")
OPT = 16                                # stated here, not taken from the bindings
HALF_OPT, LAYOUT_OPT, PREMULTIPLY_OPT, CONVERT_OPT, WITH_ALPHA_OPT = 14, 6, 8, 10, 12
HALF, BGRA8, ALPHA = 1, 0, 3            # BT709HIP_FORMAT_RGBA16F, _BGRA8_SRGB, _BGRA8_ALPHA
APPLE, SRGB, LIN = 0, 1, 2
W, H = 64, 16
ALPHA_AT = 0x80000                      # where the alpha frames start in the rig's output allocation
NAMES = ("encode_rgba16f_alpha_nv12", "encode_rgba16f_alpha_i420", "encode_rgba16f_alpha_nv12_blocks", "encode_rgba16f_alpha_i420_blocks")


def test_enumerator_and_bindings_agree_and_nothing_was_exported(tmp_path):
    src, exe = tmp_path / "ids.c", tmp_path / "ids"
    src.write_text('#include <stdio.h>\n#include "bt709hip_ext.h"\nint main(void) {\n'
                   '  printf("%d %d %d\\n", (int)BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA, (int)BT709HIP_CTX_OPT_ENCODE_HALF_INPUT, (int)BT709HIP_VERSION);\n  return 0;\n}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ids = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert ids == [OPT, HALF_OPT, 504]
    assert (_capi.CTX_OPT_ENCODE_HALF_WITH_ALPHA, _capi.ABI_VERSION, ac.OPT_HALF_WITH_ALPHA) == (OPT, 504, OPT)
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103  # no export
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    assert "kEncodeHalfWithAlphaOption = BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA" in hpp and "convertHalfIntoCoreVideoBuffersWithAlpha(" in hpp


def test_header_block_states_the_contract():
    comment = re.search(r"/\* BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA\..*?\*/", abi_headers.ext_text(), flags=re.S).group(0)
    for word in ("BT709HIP_FORMAT_RGBA16F", "BT709HIP_CTX_OPT_ENCODE_HALF_INPUT", "TWO bt709hip_frames", "outs[count + i]", "byte for byte", "(A,A,A)",
                 "NaN -> 0", "round(", "Cb = Cr = 128", "BT709HIP_GAMMA_LINEAR", "BT709HIP_ERR_TRANSFER", "BT709HIP_ERR_SIZE_MISMATCH",
                 "BT709HIP_ERR_INVALID_ARG", "BT709HIP_ERR_STRIDE", "BT709HIP_MAX_BATCH / 2", "16 PAIRS", "65535", "BT709HIP_ERR_UNSUPPORTED",
                 "BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA", "_ENCODE_PREMULTIPLY", "_ENCODE_CONVERT", "BT709HIP_CHROMA_I420", "2-byte", "general kernel",
                 "bt709hip_encoder_prepare", "BT709HIP_ERR_NOT_SETUP", "bt709hip_last_launch_info", "_ENCODE_ROW_PAIRS", "_ENCODE_THREADS", "_XCD_BANDS",
                 "OUT OF SCOPE", "alpha frame alone", "straight-alpha halves", "+convert:", "not clamped", "never touches the device", "once, on entry") + NAMES:
        assert word in comment, word
    # the half-input block keeps its words (tests/test_encode_half_cpu.py greps them)
    assert "no alpha frame from a half surface's A" in abi_headers.ext_text()


def test_the_four_kernel_names_are_the_launch_tables():
    from metalbt709decoder_amd import build
    blob = open(build.build(), "rb").read()
    for name in NAMES:
        assert name.encode() + b"\0" in blob, name


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_half_alpha") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_allocations.restype = C.c_uint64
    lib.fake_hip_set_device_count(1)
    return lib


@pytest.fixture()
def rig(fake):
    r = Rig(fake)
    yield r
    r.close()


def pair_frames(rig, n=1, w=W, h=H, step=W * H * 2, cbcr_stride=None, alpha_chroma=True, alpha_step=None, alpha_y_stride=None, alpha_cbcr_stride=None):
    """2 n frames: the colour frames of Rig.frames, then pair i's alpha frame at n + i, ALPHA_AT bytes further on"""
    colour = list(rig.frames(n, w=w, h=h, step=step, cbcr_stride=cbcr_stride))
    a_step = step if alpha_step is None else alpha_step
    base = rig.dst.value + ALPHA_AT
    alpha = [_capi.Frame(base + i * a_step, alpha_y_stride or w, base + i * a_step + W * H if alpha_chroma else None,
                         (alpha_cbcr_stride or cbcr_stride or w) if alpha_chroma else 0, w, h, 0, 0) for i in range(n)]
    return (_capi.Frame * (2 * n))(*(colour + alpha))


def both_on(rig):
    assert rig.set(1, HALF_OPT) == 0 and rig.set(1, OPT) == 0


def held(rig):
    """There is no getter (no export was added): the held value shows in what a half call with ONE frame's worth of valid output and
    an alpha frame whose y is NULL does -- encoded at 0 (the second frame is not looked at), BT709HIP_ERR_INVALID_ARG at 1."""
    frames = pair_frames(rig)
    frames[1].y = None
    rc = rig.encode(1, rig.surfs(), frames)
    assert rc in (0, _capi.ERR_INVALID_ARG)
    return 1 if rc else 0


def test_option_domain(fake, rig):
    lib = fake
    assert lib.bt709hip_context_set_option(None, OPT, 1) == _capi.ERR_INVALID_ARG
    assert rig.set(1, HALF_OPT) == 0
    assert held(rig) == 0  # the default
    for value in (1, 0, 1):
        mark = lib.fake_hip_log_size()
        assert rig.set(value, OPT) == _capi.OK
        for bad in (2, -1, 1 << 30):
            assert rig.set(bad, OPT) == _capi.ERR_INVALID_ARG, bad  # refused, not clamped ...
        assert lib.fake_hip_log_size() == mark                      # setting it logs nothing: it never touches the device
        assert held(rig) == value                                   # ... and the option keeps its value
    assert rig.set(0, OPT) == _capi.OK
    for other in (15, 17):  # the ids next to it are no options
        assert lib.bt709hip_context_set_option(rig.ctx, other, 0) == _capi.ERR_INVALID_ARG
        assert lib.bt709hip_context_set_option(rig.ctx, other, 1) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_abi_version() == 504


def test_paired_half_calls_are_one_launch_each_under_both_layouts(fake, rig):
    both_on(rig)
    mark = fake.fake_hip_log_size()
    for go in (APPLE, SRGB, LIN):
        assert rig.encode(1, rig.surfs(), pair_frames(rig), LIN, go) == 0
    assert rig.encode(4, rig.surfs(4), pair_frames(rig, 4)) == 0
    assert rig.encode(2, rig.surfs(2), pair_frames(rig, 2, alpha_chroma=False)) == 0
    assert rig.set(_capi.CHROMA_I420, LAYOUT_OPT) == 0
    assert rig.encode(2, rig.surfs(2), pair_frames(rig, 2, cbcr_stride=W // 2)) == 0
    assert rig.set(_capi.CHROMA_NV12, LAYOUT_OPT) == 0
    assert rig.encode(1, rig.surfs(w=0, h=0), pair_frames(rig, w=0, h=0)) == 0  # an empty picture: nothing to do
    assert [k[2] for k in rig.kernels(mark)] == [1, 1, 1, 4, 2, 2]
    # the plan is the plain half encoder's for the same size and count
    plans = []
    for value in (0, 1):
        assert rig.set(value, OPT) == 0
        for n in (1, 5):
            assert rig.encode(n, rig.surfs(n), pair_frames(rig, n)) == 0
            info = _capi.LaunchInfo()
            assert fake.bt709hip_last_launch_info(C.byref(info)) == 0
            plans.append((tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands))
    assert plans[:2] == plans[2:]
    # odd alpha pitches and an odd alpha pointer are valid calls (the general kernel's)
    f = pair_frames(rig, alpha_y_stride=W + 1, alpha_cbcr_stride=W + 3)
    f[1].y += 1
    assert rig.encode(1, rig.surfs(), f) == 0
    # 70 evenly spaced pairs: more than the pointer table holds
    assert rig.encode(70, rig.surfs(70, step=64), pair_frames(rig, 70, step=32, alpha_step=48)) == 0


def test_every_refusal_alone_and_in_a_batch_enqueues_nothing(fake, rig):
    lib = fake
    both_on(rig)
    for go in (APPLE, SRGB, LIN):
        assert lib.bt709hip_encoder_prepare(rig.ctx, LIN, go) == 0
    mark = lib.fake_hip_log_size()

    def call(n, edit_surf=None, edit_frame=None, edit_alpha=None, gi=LIN, go=APPLE, index=None, w=W, fmt=HALF, **kw):
        surfs, frames = rig.surfs(n, w=w, fmt=fmt), pair_frames(rig, n, w=w, **kw)
        i = n - 1 if index is None else index
        if edit_surf:
            edit_surf(surfs[i])
        if edit_frame:
            edit_frame(frames[i])
        if edit_alpha:
            edit_alpha(frames[n + i])
        return rig.encode(n, surfs, frames, gi, go)

    def put(name, value):
        return lambda s: setattr(s, name, value)

    for n in (1, 3):
        whole = n == 1  # a pitch is one per call: changed in one frame of a batch it is a size mismatch first
        assert call(n) == 0
        # the alpha frame: the BGRA8 pair's rows, in that call's order
        assert call(n, edit_alpha=put("width", W + 2)) == _capi.ERR_SIZE_MISMATCH
        assert call(n, edit_alpha=put("height", H + 2)) == _capi.ERR_SIZE_MISMATCH
        assert call(n, edit_alpha=put("y", None)) == _capi.ERR_INVALID_ARG
        assert call(n, edit_alpha=put("cbcr", None), index=n - 1) == (0 if whole else _capi.ERR_INVALID_ARG)  # NULL in every alpha frame or in none
        if n > 1:
            assert call(n, edit_alpha=put("cbcr", rig.dst.value + 0xF0000), alpha_chroma=False) == _capi.ERR_INVALID_ARG
        assert call(n, edit_alpha=put("y_stride", W - 1)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)
        assert call(n, edit_alpha=put("y_stride", 1 << 32)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)
        assert call(n, edit_alpha=put("cbcr_stride", W - 2)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)
        assert call(n, edit_alpha=put("cbcr_stride", 1 << 32)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)
        assert call(n, alpha_y_stride=W - 1) == _capi.ERR_STRIDE            # the same pitch in every alpha frame: too short
        assert call(n, alpha_cbcr_stride=W - 2) == _capi.ERR_STRIDE
        assert call(n, alpha_chroma=False, alpha_cbcr_stride=1) == 0       # without a chroma plane its pitch is not looked at
        # the colour frame and the texels: the half encoder's rules hold
        assert call(n, put("bgra", rig.src.value + 4)) == _capi.ERR_STRIDE
        assert call(n, put("stride", 8 * W - 8)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)
        assert call(n, put("reserved", 1)) == _capi.ERR_UNSUPPORTED
        assert call(n, gi=SRGB) == _capi.ERR_TRANSFER
        assert call(n, gi=APPLE, go=LIN) == _capi.ERR_TRANSFER
        for go in (3, 4, -1):
            assert call(n, go=go) == _capi.ERR_INVALID_ARG
        assert call(n, w=W - 1) == _capi.ERR_ODD_DIMENSIONS
        assert call(n, edit_frame=put("y", None)) == _capi.ERR_INVALID_ARG
        assert call(n, edit_frame=put("y_stride", W - 1)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)
        # everything else stays as it is: the three BGRA8 options away from their defaults, behind the usual validation
        for option, value, default in ((PREMULTIPLY_OPT, 1, 0), (CONVERT_OPT, _capi.CONVERT_PACKED444, 0), (CONVERT_OPT, _capi.CONVERT_POINT420, 0),
                                       (WITH_ALPHA_OPT, 1, 0)):
            assert rig.set(value, option) == 0
            try:
                assert call(n) == _capi.ERR_UNSUPPORTED, (option, value)
                assert call(n, w=W - 1) == _capi.ERR_ODD_DIMENSIONS          # ... which still comes first
                assert call(n, gi=SRGB) == _capi.ERR_TRANSFER
                assert call(n, edit_alpha=put("y", None)) == _capi.ERR_INVALID_ARG
            finally:
                assert rig.set(default, option) == 0
        # RGBA16F input with HALF_INPUT = 0 is refused whatever the new option holds
        assert rig.set(0, HALF_OPT) == 0
        try:
            assert call(n) == _capi.ERR_UNSUPPORTED
        finally:
            assert rig.set(1, HALF_OPT) == 0
    # the pointer table holds 16 pairs
    uneven = rig.surfs(17, step=64)
    uneven[5].bgra += 16
    assert rig.encode(17, uneven, pair_frames(rig, 17, step=32)) == _capi.ERR_UNSUPPORTED
    spaced = pair_frames(rig, 17, step=32)
    spaced[17 + 5].y += 2  # an alpha plane out of step is enough
    assert rig.encode(17, rig.surfs(17, step=64), spaced) == _capi.ERR_UNSUPPORTED
    kernels = [k for k in rig.kernels(mark)]
    passed = 2 * 3  # per n: the sound call, the single call whose cbcr is NULL in its one alpha frame (n == 1 only), the Y-only call
    assert len(kernels) == passed - 1, kernels
    mark = lib.fake_hip_log_size()
    uneven = rig.surfs(16, step=64)
    uneven[5].bgra += 16
    assert rig.encode(16, uneven, pair_frames(rig, 16, step=32)) == 0
    assert [k[2] for k in rig.kernels(mark)] == [16]


def test_with_the_option_at_0_half_and_bgra8_calls_log_the_same_launches(fake, rig):
    """BGRA8_SRGB and BGRA8_ALPHA input do not read the option, the BGRA8 pair neither; half input at 0 is the call of before."""
    from test_fake_hip import log
    lib = fake
    assert rig.set(1, HALF_OPT) == 0
    issued = {}
    for value in (0, 1):
        assert rig.set(value, OPT) == 0
        mark = lib.fake_hip_log_size()
        records = []
        calls = [(1, BGRA8, SRGB, APPLE, 0), (4, BGRA8, SRGB, SRGB, 0), (70, BGRA8, LIN, LIN, 0), (1, ALPHA, LIN, LIN, 0), (3, ALPHA, LIN, LIN, 0), (3, BGRA8, SRGB, APPLE, 1)]
        if value == 0:
            calls += [(1, HALF, LIN, APPLE, 0), (5, HALF, LIN, SRGB, 0)]
        for n, fmt, gi, go, with_alpha in calls:
            px = 8 if fmt == HALF else 4
            assert rig.set(with_alpha, WITH_ALPHA_OPT) == 0
            try:
                rc = rig.encode(n, rig.surfs(n, fmt=fmt, step=px * W * H if n < 70 else 64), pair_frames(rig, n, step=W * H * 2 if n < 70 else 32), gi, go)
            finally:
                assert rig.set(0, WITH_ALPHA_OPT) == 0
            assert rc == 0, (n, fmt)
            info = _capi.LaunchInfo()
            assert lib.bt709hip_last_launch_info(C.byref(info)) == 0
            records.append((tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands))
        issued[value] = ([(o[0], o[2], o[3]) for o in log(lib, mark)], records)
    assert issued[0][0][:6] == issued[1][0] and issued[0][1][:6] == issued[1][1] and len(issued[1][0]) == 6
    # ... and the half calls at 0 are what they are without the option ever having been touched
    other = Rig(lib)
    try:
        assert other.set(1, HALF_OPT) == 0
        mark = lib.fake_hip_log_size()
        assert other.encode(1, other.surfs(), other.frames(), LIN, APPLE) == 0 and other.encode(5, other.surfs(5), other.frames(5), LIN, SRGB) == 0
        assert [(o[0], o[2]) for o in log(lib, mark) if o[0].startswith("kernel:")] == [(o[0], o[1]) for o in issued[0][0][6:] if o[0].startswith("kernel:")]
    finally:
        other.close()


def test_capture_needs_one_prepare(fake):
    """bt709hip_encoder_prepare(ctx, LINEAR, out) with the option at 1 makes everything the paired half path needs, T included: the
    encode behind it uploads nothing and can be captured; prepared with the option at 0 (T missing) or not at all, a captured paired
    half encode returns BT709HIP_ERR_NOT_SETUP and enqueues nothing."""
    lib = fake
    for prepared in ("no", "option at 0", "option at 1"):
        rig = Rig(lib)
        try:
            S, g = C.c_void_p(), C.c_void_p()
            assert lib.bt709hip_stream_create(rig.ctx, C.byref(S)) == 0
            assert rig.set(1, HALF_OPT) == 0
            if prepared == "option at 0":
                assert lib.bt709hip_encoder_prepare(rig.ctx, LIN, APPLE) == 0
            assert rig.set(1, OPT) == 0
            if prepared == "option at 1":
                assert lib.bt709hip_encoder_prepare(rig.ctx, LIN, APPLE) == 0
            allocations = lib.fake_hip_allocations(0)
            mark = lib.fake_hip_log_size()
            assert lib.bt709hip_graph_begin_capture(rig.ctx, S) == 0
            assert rig.set(0, OPT) == 0 and rig.set(1, OPT) == 0  # the setter works while the stream is being captured
            rc = rig.encode(2, rig.surfs(2), pair_frames(rig, 2), LIN, APPLE, S, 0)
            assert lib.bt709hip_graph_end_capture(rig.ctx, S, C.byref(g)) == 0
            assert rc == (_capi.OK if prepared == "option at 1" else _capi.ERR_NOT_SETUP), prepared
            assert lib.fake_hip_allocations(0) == allocations and rig.kernels(mark) == []
            if rc == _capi.OK:
                assert lib.bt709hip_graph_launch(rig.ctx, g, S) == 0 and lib.bt709hip_stream_synchronize(rig.ctx, S) == 0
                issued = rig.kernels(mark)
                assert len(issued) == 1 and issued[0][2] == 2
            assert lib.bt709hip_graph_destroy(rig.ctx, g) == 0 and lib.bt709hip_stream_destroy(rig.ctx, S) == 0
        finally:
            rig.close()


# ------------------------------------------------------------------ the Python mirror

def test_python_mirror_sets_and_restores_both_options():
    """convertHalfIntoCoreVideoBuffersWithAlpha sets CTX_OPT_ENCODE_HALF_INPUT and CTX_OPT_ENCODE_HALF_WITH_ALPHA around the one call
    and puts 0 back in both, also when the call is refused or raises; the alpha buffers leave tagged; the pinned keyword of
    convertIntoCoreVideoBuffers keeps its meaning."""
    calls = []

    class Lib:
        rc = _capi.OK
        refuse = None

        def bt709hip_context_set_option(self, handle, option, value):
            calls.append(("set", option, value))
            return _capi.ERR_INVALID_ARG if (option, value) == self.refuse else _capi.OK

        def bt709hip_encode_batch(self, handle, n, surfs, frames, gi, go, stream, wait):
            calls.append(("encode", n, [s.format for s in surfs], len(frames), [f.y for f in frames], gi, go))
            if isinstance(self.rc, Exception):
                raise self.rc
            return self.rc

    ctx = mb.MetalRenderContext(0)
    ctx.lib, ctx.handle = Lib(), 1
    try:
        conv = mb.BGRAToBT709Converter
        halves = [mb.BGRATexture(ctx, W, H, ptr=0x10000 * (i + 1), pixelFormat=mb.MTLPixelFormatRGBA16Float) for i in range(2)]
        bytes_ = [mb.BGRATexture(ctx, W, H, ptr=0x10000 * (i + 9)) for i in range(2)]
        outs = [mb.CVPixelBuffer(ctx, W, H, planes=(0x100000 * (i + 1), 0x100000 * (i + 1) + W * H)) for i in range(2)]
        alphas = [mb.CVPixelBuffer(ctx, W, H, planes=(0x900000 + 0x10000 * i, None)) for i in range(2)]
        sets = lambda: [c for c in calls if c[0] == "set" and c[1] in (HALF_OPT, OPT)]
        assert conv.convertHalfIntoCoreVideoBuffersWithAlpha(halves, outs, alphas, APPLE)
        assert sets() == [("set", HALF_OPT, 1), ("set", OPT, 1), ("set", OPT, 0), ("set", HALF_OPT, 0)]
        encodes = [c for c in calls if c[0] == "encode"]
        assert encodes == [("encode", 2, [HALF, HALF], 4, [0x100000, 0x200000, 0x900000, 0x910000], LIN, APPLE)]  # colour frames, then alpha frames
        assert calls.index(encodes[0]) == calls.index(("set", OPT, 1)) + 1
        for b in alphas:
            assert b.attachments["TransferFunction"] == mb.kCVImageBufferTransferFunction_Linear
            assert b.attachments["YCbCrMatrix"] == mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2
        del calls[:]
        ctx.lib.rc = _capi.ERR_STRIDE  # a refused call: False, both options back at 0
        assert not conv.convertHalfIntoCoreVideoBuffersWithAlpha(halves, outs, alphas, SRGB)
        assert sets()[:2] == [("set", HALF_OPT, 1), ("set", OPT, 1)] and sets()[-2:] == [("set", OPT, 0), ("set", HALF_OPT, 0)]
        del calls[:]
        ctx.lib.rc = RuntimeError("the call raised")
        with pytest.raises(RuntimeError):
            conv.convertHalfIntoCoreVideoBuffersWithAlpha(halves, outs, alphas, APPLE)
        assert sets()[:2] == [("set", HALF_OPT, 1), ("set", OPT, 1)] and sets()[-2:] == [("set", OPT, 0), ("set", HALF_OPT, 0)]
        del calls[:]
        ctx.lib.rc = _capi.OK
        ctx.lib.refuse = (OPT, 1)  # a library without the option: nothing is encoded, the half option is put back
        assert not conv.convertHalfIntoCoreVideoBuffersWithAlpha(halves, outs, alphas, APPLE)
        assert sets() == [("set", HALF_OPT, 1), ("set", OPT, 1), ("set", HALF_OPT, 0)] and not [c for c in calls if c[0] == "encode"]
        ctx.lib.refuse = None
        del calls[:]
        assert not conv.convertHalfIntoCoreVideoBuffersWithAlpha(bytes_, outs, alphas, APPLE)  # BGRA8 textures: not this method's
        assert calls == []
        with pytest.raises(ValueError):
            conv.convertHalfIntoCoreVideoBuffersWithAlpha(halves, outs, alphas[:1], APPLE)
        assert conv.convertHalfIntoCoreVideoBuffersWithAlpha([], [], [], APPLE) and calls == []
        # the pinned keyword: no alpha frame from halves through convertIntoCoreVideoBuffers, no call issued
        assert not conv.convertIntoCoreVideoBuffers(halves[:1], outs[:1], LIN, APPLE, alphaPixelBuffers=alphas[:1])
        assert calls == []
    finally:
        ctx.handle = None


# ------------------------------------------------------------------ the definition

@pytest.fixture(scope="module")
def expect(oracle):
    return hc.Expect(oracle)


@pytest.fixture(scope="module")
def definition(expect):
    """(65536,) uint8: the alpha frame's Y for every half code in A, by the oracle composition -- the code of pixel (y, x) of a
    256 x 256 grey surface is 256 y + x, so no block is flat -- with the chroma plane it gives"""
    codes = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    y, c = expect.planes(ac.grey(codes), GAMMA_LINEAR)
    return y.reshape(-1), c


def test_the_definition_is_T_of_the_rounded_saturated_alpha_for_all_65536_codes(definition):
    y, c = definition
    codes = np.arange(65536, dtype=np.uint16)
    assert np.array_equal(y, ac.LUMA[ac.alpha_code(codes)])
    assert np.all(c == 128)  # and every block of that surface is non-flat
    # NaN -> 0, negative and -0 -> 0, above 1 and +inf -> 1
    f = codes.view(np.float16).astype(np.float64)
    assert np.all(y[np.isnan(f)] == ac.LUMA[0]) and np.all(y[f <= 0] == ac.LUMA[0]) and np.all(y[f >= 1] == ac.LUMA[255])
    assert (ac.LUMA[0], ac.LUMA[255]) == (16, 235) and np.unique(y).size == 220


def test_alpha_chroma_is_128_on_random_blocks_with_the_specials(expect):
    rng = np.random.default_rng(2113)
    t = hc.random_texels(rng, 64, 64)
    t[0:2, 0:2, 3] = [[0x7E00, 0x3C00], [0x0000, 0x7C00]]  # NaN, 1, 0, +inf in one block
    t[0:2, 2:4, 3] = [[0xFC00, 0x3BFF], [0x0001, 0xBC00]]  # -inf, just below 1, the smallest subnormal, -1
    y, c = ac.alpha_planes(expect, t)
    assert np.all(c == 128)
    assert np.array_equal(y, ac.LUMA[ac.alpha_code(t[..., 3])])
    # the averaged alpha goes through the same round to a grey byte: the oracle's own average of grey bytes is a grey byte
    a = hc.saturate(t[..., 3])
    ave = (((a[0::2, 0::2] + a[0::2, 1::2]) + a[1::2, 0::2]) + a[1::2, 1::2]) / np.float32(4.0)
    grey_byte = expect.from_linear(GAMMA_LINEAR, ave)
    assert np.all(expect.matrix(np.repeat(grey_byte[..., None], 3, -1))[..., 1:] == 128)
    assert np.all(expect.matrix(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, -1))[..., 1:] == 128)  # a grey's Cb, Cr for EVERY byte


def test_flat_grey_blocks_equal_the_oracles_linear_encode_of_the_bgra8_twin(expect, oracle):
    rng = np.random.default_rng(2114)
    blocks = rng.integers(0, hc.ONE + 1, (8, 16), dtype=np.uint16)
    a = np.repeat(np.repeat(blocks, 2, 0), 2, 1)
    y, c = expect.planes(ac.grey(a), GAMMA_LINEAR)
    byte = expect.code_table(GAMMA_LINEAR)[a]
    ty, tc = oracle.encode_nv12(hc.twin_words(np.repeat(byte[..., None], 3, -1)), 32, 16, GAMMA_LINEAR, GAMMA_LINEAR)
    assert np.array_equal(y, ty) and np.array_equal(c, tc)
    assert np.array_equal(y, ac.LUMA[byte])  # which is the BGRA8_ALPHA encode of a surface whose A is that byte


# ------------------------------------------------------------------ the device's alpha step, replayed on the host

def test_host_replay_of_the_alpha_step_over_all_65536_codes(tmp_path, definition):
    """csrc/bt709_half_alpha_step.h -- the text the kernels compile -- with plain g++ and -ffp-contract=off, against the definition."""
    out = str(tmp_path / "libhalf_alpha_step.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC,
           os.path.join(HERE, "native", "half_alpha_step.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(out)
    sat = np.empty(65536, np.float32)
    lib.half_sat_all(sat.ctypes.data_as(C.c_void_p))
    assert np.array_equal(sat.view(np.uint32), hc.saturate(np.arange(65536, dtype=np.uint16)).view(np.uint32))  # bit for bit, +0 included
    got = np.empty(65536, np.uint8)
    T = np.ascontiguousarray(ac.LUMA)
    lib.half_alpha_step_all(T.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p))
    assert np.array_equal(got, definition[0])
    # the kernels include that header and call that function
    text = open(os.path.join(CSRC, "bt709_encode_half_alpha.h")).read()
    assert '#include "bt709_half_alpha_step.h"' in text and text.count("half_alpha_luma(") >= 5


# ------------------------------------------------------------------ the generated code

@pytest.mark.parametrize("layout", [0, 1])
def test_descriptors_of_the_paired_fast_kernels(layout):
    """Descriptor fields alone: the clamp that turns NaN into 0, half denormals kept, no scratch, no static LDS (T and the
    from_linear table share the dynamic segment from address 0), EncodeParams as large as it was."""
    from metalbt709decoder_amd import build
    asm = open(build.emit_asm()).read()
    for name in ("encode_rgba16f_alpha", "encode_rgba16f_alpha_blocks"):
        _, meta = kernel(asm, name, layout)
        kd = descriptor(asm, name, layout)
        assert kd["dx10_clamp"] == 1 and kd["float_denorm_mode_16_64"] == 3 and kd["float_round_mode_32"] == 0
        assert meta_int(meta, "private_segment_fixed_size") == 0 and kd["private_segment_fixed_size"] == 0 and kd["group_segment_fixed_size"] == 0
        assert kd["kernarg_size"] == 880 + 256
    _, meta = kernel(asm, "encode_rgba16f_alpha", layout)
    assert meta_int(meta, "vgpr_count") <= 64  # eight waves per SIMD, as the plain kernel


# ------------------------------------------------------------------ the round trip through the decoder's RGBA16F alpha

def test_round_trip_of_every_alpha_frame_code(oracle):
    """An alpha frame's code 0..255 -> the oracle's decode into RGBA16F (A = the half the decoder writes) -> the definition.  What the
    composition gives: every code of the video range 16..235 returns to itself, codes below 16 return as 16 and codes above 235 as
    235 (the decoder saturates them to A = 0 and A = 1)."""
    codes = np.arange(256, dtype=np.uint8).reshape(16, 16)
    y = np.full((16, 16), 128, np.uint8)
    c = np.full((8, 16), 128, np.uint8)
    back = {}
    for gamma in (GAMMA_APPLE, GAMMA_SRGB, GAMMA_LINEAR):
        texels = oracle.decode_nv12_rgba16f(gamma, y, c, alpha=codes).view(np.uint16)
        back[gamma] = ac.LUMA[ac.alpha_code(texels[..., 3])].reshape(-1)
        assert np.array_equal(back[gamma], back[GAMMA_APPLE])  # the alpha does not depend on the colour's gamma
    got = back[GAMMA_APPLE]
    returned = int(np.sum(got[16:236] == np.arange(16, 236)))
    print("round trip: %d of the 220 codes 16..235 return to themselves" % returned)
    assert returned == 220
    assert np.array_equal(got, np.clip(np.arange(256), 16, 235))
