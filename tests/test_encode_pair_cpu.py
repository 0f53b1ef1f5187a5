"""BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA (a BGRA surface's colour frame and alpha frame from one bt709hip_encode[_batch] launch,
DESIGN.md 3.11), the parts that need no GPU: the option's domain, the paired call's validation, refusals and launch counts on the
fake HIP runtime (tests/native/fake_hip/), the header's enumerator, the capture rule after one bt709hip_encoder_prepare, and the
Python mirror's set-and-restore.  On a tree without the option every test here fails at its first set_option
(BT709HIP_ERR_INVALID_ARG) or at the missing binding."""
import ctypes as C
import os
import re
import subprocess

import pytest

import abi_headers
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = 12                               # stated here, not taken from the bindings
CONVERT_OPT, LAYOUT_OPT = 10, 6
ALPHA = 3                              # BT709HIP_FORMAT_BGRA8_ALPHA
APPLE, SRGB, LIN = 0, 1, 2
MAX_PAIRS = 16                         # BT709HIP_MAX_BATCH / 2: pairs in the pointer table
W, H = 64, 16


def test_enumerator_and_bindings_agree_and_nothing_was_exported(tmp_path):
    src, exe = tmp_path / "ids.c", tmp_path / "ids"
    src.write_text('#include <stdio.h>\n#include "bt709hip_ext.h"\nint main(void) {\n'
                   '  printf("%d %d %d\\n", (int)BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA, (int)BT709HIP_VERSION, (int)BT709HIP_MAX_BATCH);\n  return 0;\n}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ids = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert ids == [OPT, 504, 2 * MAX_PAIRS]
    assert (_capi.CTX_OPT_ENCODE_WITH_ALPHA, _capi.ABI_VERSION) == (OPT, 504)
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103  # no export
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    assert "kEncodeWithAlphaOption = BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA" in hpp and "static bool convertIntoCoreVideoBuffers(MetalRenderContext &mrc" in hpp


def test_header_block_states_the_contract():
    comment = re.search(r"/\* BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA\..*?\*/", abi_headers.ext_text(), flags=re.S).group(0)
    for word in ("TWO bt709hip_frames", "out[0]", "out[1]", "outs[count + i]", "Y = T[A]", "BT709HIP_ERR_SIZE_MISMATCH", "BT709HIP_ERR_STRIDE",
                 "BT709HIP_ERR_INVALID_ARG", "BT709HIP_ERR_UNSUPPORTED", "BT709HIP_ERR_NOT_SETUP", "16 PAIRS", "65535", "not clamped",
                 "never touches the device", "bt709hip_encoder_prepare", "bt709hip_last_launch_info", "<premul>", "encode_bgra_alpha_nv12",
                 "encode_bgra_alpha_i420", "encode_bgra_alpha_nv12_blocks", "encode_bgra_alpha_i420_blocks"):
        assert word in comment, word
    assert "BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA" in abi_headers.core_text()


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_pair") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_allocations.restype = C.c_uint64
    lib.fake_hip_set_device_count(1)
    return lib


class Rig:
    """A context and three allocations: BGRA pictures, colour frames, alpha frames, each large enough for 33 evenly spaced ones
    (launches touch nothing on the fake runtime, so pictures may overlap)."""

    def __init__(self, lib):
        self.lib = lib
        self.ctx = C.c_void_p()
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0
        self.src, self.dst, self.adst = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for p in (self.src, self.dst, self.adst):
            assert lib.bt709hip_malloc(self.ctx, 1 << 20, C.byref(p)) == 0

    def set(self, value):
        return self.lib.bt709hip_context_set_option(self.ctx, OPT, value)

    def surfs(self, n=1, fmt=0, w=W, h=H, step=4 * W * H):
        return (_capi.Surface * n)(*[_capi.Surface(self.src.value + i * step, 4 * w, w, h, fmt, 0) for i in range(n)])

    def pairs(self, n=1, w=W, h=H, alpha_cbcr=True, step=W * H * 2, alpha_step=W * H * 2, alpha_base=0):
        """2 * n frames: the colour frames, then the alpha frames.  alpha_step may be negative (alpha_base then sits high)."""
        colour = [_capi.Frame(self.dst.value + i * step, w, self.dst.value + i * step + W * H, w, w, h, 0, 0) for i in range(n)]
        base = self.adst.value + alpha_base
        alpha = [_capi.Frame(base + i * alpha_step, w, base + i * alpha_step + W * H if alpha_cbcr else None, w if alpha_cbcr else 0, w, h, 0, 0) for i in range(n)]
        return (_capi.Frame * (2 * n))(*(colour + alpha))

    def encode(self, n, surfs, frames, gi=SRGB, go=APPLE, stream=None, wait=1):
        if n == 1:
            return self.lib.bt709hip_encode(self.ctx, surfs, frames, gi, go, stream, wait)
        return self.lib.bt709hip_encode_batch(self.ctx, n, surfs, frames, gi, go, stream, wait)

    def kernels(self, mark):
        from test_fake_hip import log
        return [o for o in log(self.lib, mark) if o[0].startswith("kernel:")]

    def close(self):
        for p in (self.src, self.dst, self.adst):
            assert self.lib.bt709hip_free(self.ctx, p) == 0
        assert self.lib.bt709hip_context_destroy(self.ctx) == 0


@pytest.fixture()
def rig(fake):
    r = Rig(fake)
    yield r
    r.close()


def held(rig):
    """There is no getter (no export was added): the held value shows in what the next call does with BGRA8_ALPHA input --
    encoded at 0, BT709HIP_ERR_UNSUPPORTED at 1."""
    rc = rig.lib.bt709hip_encode(rig.ctx, rig.surfs(fmt=ALPHA), rig.pairs(), LIN, LIN, None, 1)
    assert rc in (0, _capi.ERR_UNSUPPORTED)
    return 1 if rc else 0


def test_option_domain(fake, rig):
    lib = fake
    assert lib.bt709hip_context_set_option(None, OPT, 1) == _capi.ERR_INVALID_ARG
    assert held(rig) == 0  # the default
    for value in (1, 0, 1):
        mark = lib.fake_hip_log_size()
        assert rig.set(value) == _capi.OK
        for bad in (2, -1, 1 << 30):
            assert rig.set(bad) == _capi.ERR_INVALID_ARG, bad  # refused, not clamped ...
        assert lib.fake_hip_log_size() == mark                 # setting it logs nothing: it never touches the device
        assert held(rig) == value                              # ... and the option keeps its value
    assert rig.set(0) == _capi.OK
    for other in (7, 9, 11, 13):  # the ids next to it are still no options
        assert lib.bt709hip_context_set_option(rig.ctx, other, 0) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_abi_version() == 504


def test_paired_calls_are_one_launch_each(fake, rig):
    lib = fake
    assert rig.set(1) == 0
    mark = lib.fake_hip_log_size()
    assert rig.encode(1, rig.surfs(), rig.pairs()) == 0
    assert rig.encode(4, rig.surfs(4), rig.pairs(4)) == 0
    assert rig.encode(1, rig.surfs(), rig.pairs(alpha_cbcr=False), LIN, SRGB) == 0  # an alpha frame without a chroma plane; any colour gammas
    assert [k[2] for k in rig.kernels(mark)] == [1, 4, 1]
    # the launch on record is the colour encoder's for the same size and count
    info, plain = _capi.LaunchInfo(), _capi.LaunchInfo()
    assert rig.encode(4, rig.surfs(4), rig.pairs(4)) == 0 and lib.bt709hip_last_launch_info(C.byref(info)) == 0
    assert rig.set(0) == 0
    assert rig.encode(4, rig.surfs(4), rig.pairs(4)) == 0 and lib.bt709hip_last_launch_info(C.byref(plain)) == 0
    assert (tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands) == (tuple(plain.grid), tuple(plain.block), plain.launches, plain.xcd_bands)


def test_refusals_return_their_code_and_enqueue_nothing(fake, rig):
    lib = fake
    assert rig.set(1) == 0
    assert lib.bt709hip_encoder_prepare(rig.ctx, SRGB, APPLE) == 0
    mark = lib.fake_hip_log_size()

    def changed(n, edit, **kw):
        frames = rig.pairs(n, **kw)
        edit(frames)
        return rig.encode(n, rig.surfs(n), frames)

    def field(index, name, value):
        return lambda frames: setattr(frames[index], name, value)

    # the alpha frame's size
    assert changed(1, field(1, "width", W - 2)) == _capi.ERR_SIZE_MISMATCH
    assert changed(4, field(4 + 2, "height", H + 2)) == _capi.ERR_SIZE_MISMATCH
    # its planes
    assert changed(1, field(1, "y", None)) == _capi.ERR_INVALID_ARG
    assert changed(4, field(4 + 3, "cbcr", None)) == _capi.ERR_INVALID_ARG                        # NULL in one alpha frame of four
    assert changed(4, field(4 + 1, "cbcr", rig.adst.value), alpha_cbcr=False) == _capi.ERR_INVALID_ARG  # non-NULL in one of four
    # its pitches: short, and past 32 bits
    assert changed(1, field(1, "y_stride", W - 1)) == _capi.ERR_STRIDE
    assert changed(1, field(1, "cbcr_stride", W - 1)) == _capi.ERR_STRIDE
    assert changed(1, field(1, "y_stride", 1 << 32)) == _capi.ERR_STRIDE
    assert changed(1, field(1, "cbcr_stride", 1 << 32)) == _capi.ERR_STRIDE
    assert changed(4, field(4 + 2, "y_stride", W + 4)) == _capi.ERR_SIZE_MISMATCH                 # equal pitches across the batch
    assert changed(4, field(4 + 2, "cbcr_stride", W + 4)) == _capi.ERR_SIZE_MISMATCH
    # the planar layout's chroma pitch rule covers the alpha frame: W/2 is enough there, and too little under NV12
    assert changed(1, field(1, "cbcr_stride", W // 2)) == _capi.ERR_STRIDE
    # 17 unevenly spaced pairs: the pointer table holds 16 (an uneven ALPHA Y plane alone makes the batch uneven)
    n = MAX_PAIRS + 1
    assert changed(n, field(n + 5, "y", rig.adst.value + 5 * W * H * 2 + 64), step=64, alpha_step=64) == _capi.ERR_UNSUPPORTED
    uneven_chroma = rig.pairs(n, step=64, alpha_step=64)
    uneven_chroma[n + 7].cbcr = uneven_chroma[n + 7].cbcr + 16
    assert rig.encode(n, rig.surfs(n, step=64), uneven_chroma) == _capi.ERR_UNSUPPORTED
    # not with the per-pixel converter, not for BGRA8_ALPHA input: after the usual validation
    assert lib.bt709hip_context_set_option(rig.ctx, CONVERT_OPT, _capi.CONVERT_POINT420) == 0
    assert rig.encode(1, rig.surfs(), rig.pairs(), SRGB, APPLE) == _capi.ERR_UNSUPPORTED
    assert rig.encode(1, rig.surfs(w=W - 1), rig.pairs(w=W - 1), SRGB, APPLE) == _capi.ERR_ODD_DIMENSIONS
    assert lib.bt709hip_context_set_option(rig.ctx, CONVERT_OPT, _capi.CONVERT_OFF) == 0
    assert rig.encode(1, rig.surfs(fmt=ALPHA), rig.pairs(), LIN, LIN) == _capi.ERR_UNSUPPORTED
    assert rig.encode(1, rig.surfs(fmt=ALPHA), rig.pairs(), SRGB, APPLE) == _capi.ERR_ALPHA_TRANSFER  # the alpha clip's own gamma check still comes first
    assert rig.kernels(mark) == [] and lib.fake_hip_log_size() == mark, "a refused call enqueued something"
    # what goes through: exactly 16 uneven pairs
    n = MAX_PAIRS
    assert changed(n, field(n + 5, "y", rig.adst.value + 5 * W * H * 2 + 64), step=64, alpha_step=64) == 0
    assert [k[2] for k in rig.kernels(mark)] == [n]


def test_33_evenly_spaced_pairs_with_a_negative_alpha_step(fake, rig):
    lib = fake
    assert rig.set(1) == 0
    mark = lib.fake_hip_log_size()
    n = 33
    frames = rig.pairs(n, step=48, alpha_step=-80, alpha_base=80 * n)
    assert rig.encode(n, rig.surfs(n, step=32), frames) == 0
    assert [k[2] for k in rig.kernels(mark)] == [n]
    assert rig.encode(n, rig.surfs(n, step=32), rig.pairs(n, step=48, alpha_step=-80, alpha_base=80 * n, alpha_cbcr=False)) == 0
    # under the planar layout the alpha frame's U plane takes a W/2 pitch
    assert lib.bt709hip_context_set_option(rig.ctx, LAYOUT_OPT, _capi.CHROMA_I420) == 0
    planar = rig.pairs(2)
    for f in planar:
        f.cbcr_stride = W // 2
    assert rig.encode(2, rig.surfs(2), planar) == 0
    assert lib.bt709hip_context_set_option(rig.ctx, LAYOUT_OPT, _capi.CHROMA_NV12) == 0
    assert len(rig.kernels(mark)) == 3


def test_one_prepare_under_the_option_builds_the_alpha_table(fake):
    """bt709hip_encoder_prepare(ctx, gi, go) with the option at 1 builds T beside the pair's tables: the paired encode behind it
    uploads nothing (no allocation on the fake device) and can be captured; prepared with the option at 0, a captured paired
    encode finds T missing."""
    lib = fake
    for on_at_prepare in (0, 1):
        rig = Rig(lib)
        try:
            S, g = C.c_void_p(), C.c_void_p()
            assert lib.bt709hip_stream_create(rig.ctx, C.byref(S)) == 0
            assert rig.set(on_at_prepare) == 0
            assert lib.bt709hip_encoder_prepare(rig.ctx, SRGB, APPLE) == 0
            assert rig.set(1) == 0
            allocations = lib.fake_hip_allocations(0)
            mark = lib.fake_hip_log_size()
            assert lib.bt709hip_graph_begin_capture(rig.ctx, S) == 0
            rc = rig.encode(2, rig.surfs(2), rig.pairs(2), SRGB, APPLE, S, 0)
            assert lib.bt709hip_graph_end_capture(rig.ctx, S, C.byref(g)) == 0
            assert rc == (_capi.OK if on_at_prepare else _capi.ERR_NOT_SETUP)
            assert lib.fake_hip_allocations(0) == allocations and rig.kernels(mark) == []
            if on_at_prepare:
                assert lib.bt709hip_graph_launch(rig.ctx, g, S) == 0 and lib.bt709hip_stream_synchronize(rig.ctx, S) == 0
                issued = rig.kernels(mark)
                assert len(issued) == 1 and issued[0][2] == 2
                assert rig.encode(1, rig.surfs(), rig.pairs()) == 0 and lib.fake_hip_allocations(0) == allocations  # nor outside a capture
            assert lib.bt709hip_graph_destroy(rig.ctx, g) == 0 and lib.bt709hip_stream_destroy(rig.ctx, S) == 0
        finally:
            rig.close()


# ------------------------------------------------------------------ the Python mirror

def test_python_mirror_sets_and_restores_the_option():
    """convertIntoCoreVideoBuffer[s](..., alphaPixelBuffer[s]=...) sets the option around the one call and puts 0 back, also when
    the call raises; the alpha buffers leave tagged 709 / Linear; without alpha buffers the option is never touched."""
    calls = []

    class Lib:
        rc = _capi.OK

        def bt709hip_context_set_option(self, handle, option, value):
            calls.append(("set", option, value))
            return _capi.OK

        def bt709hip_encode_batch(self, handle, n, surfs, frames, gi, go, stream, wait):
            calls.append(("encode", n, len(frames), [f.y for f in frames]))
            if isinstance(self.rc, Exception):
                raise self.rc
            return self.rc

    ctx = mb.MetalRenderContext(0)
    ctx.lib, ctx.handle = Lib(), 1
    try:
        conv = mb.BGRAToBT709Converter
        texs = [mb.BGRATexture(ctx, W, H, ptr=0x1000 * (i + 1)) for i in range(2)]
        colour = [mb.CVPixelBuffer(ctx, W, H, planes=(0x100000 * (i + 1), 0x100000 * (i + 1) + W * H)) for i in range(2)]
        alpha = [mb.CVPixelBuffer(ctx, W, H, planes=(0x900000 + 0x100000 * i, None)) for i in range(2)]
        assert conv.convertIntoCoreVideoBuffers(texs, colour, SRGB, APPLE, alphaPixelBuffers=alpha)
        assert calls == [("set", OPT, 1), ("encode", 2, 4, [0x100000, 0x200000, 0x900000, 0xA00000]), ("set", OPT, 0)]
        for b in alpha:
            assert b.getAttachment("YCbCrMatrix") == mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2
            assert b.getAttachment("TransferFunction") == mb.kCVImageBufferTransferFunction_Linear
        del calls[:]
        assert conv.convertIntoCoreVideoBuffer(texs[0], colour[0], SRGB, APPLE, alphaPixelBuffer=alpha[0])
        assert [c[:3] for c in calls] == [("set", OPT, 1), ("encode", 1, 2), ("set", OPT, 0)]
        del calls[:]
        ctx.lib.rc = _capi.ERR_STRIDE  # a refused call: False, the option back at 0
        assert not conv.convertIntoCoreVideoBuffers(texs, colour, SRGB, APPLE, alphaPixelBuffers=alpha)
        assert calls[0] == ("set", OPT, 1) and calls[-1] == ("set", OPT, 0)
        del calls[:]
        ctx.lib.rc = RuntimeError("the call raised")
        with pytest.raises(RuntimeError):
            conv.convertIntoCoreVideoBuffers(texs, colour, SRGB, APPLE, alphaPixelBuffers=alpha)
        assert calls[0] == ("set", OPT, 1) and calls[-1] == ("set", OPT, 0)
        del calls[:]
        ctx.lib.rc = _capi.OK  # no alpha buffers: the call of before, the option untouched
        assert conv.convertIntoCoreVideoBuffers(texs, colour, SRGB, APPLE)
        assert calls == [("encode", 2, 2, [0x100000, 0x200000])]
        with pytest.raises(ValueError):
            conv.convertIntoCoreVideoBuffers(texs, colour, SRGB, APPLE, alphaPixelBuffers=alpha[:1])
    finally:
        ctx.handle = None
