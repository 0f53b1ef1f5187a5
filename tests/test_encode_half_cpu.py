"""BT709HIP_CTX_OPT_ENCODE_HALF_INPUT (bt709hip_encode[_batch] of RGBA16Float linear-light surfaces), the parts that
need no GPU: the enumerator and the ABI, the option's domain, every validation row of a half-input call on the fake HIP runtime
(tests/native/fake_hip/) alone and in a batch, the capture rule, the Python mirror's set-and-restore, the facts about the 15361
halves in [0, 1] that the GPU sweeps rest on, the expectation helper against the reference's own inlines where they are built, and
the generated code of the new fast kernel.  On a tree without the option every test here fails at its first set_option
(BT709HIP_ERR_INVALID_ARG), at the missing binding or at the missing kernel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_headers
import encode_half_cases as hc
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_APPLE, GAMMA_LINEAR, GAMMA_SRGB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = 14                                # stated here, not taken from the bindings
LAYOUT_OPT, PREMULTIPLY_OPT, CONVERT_OPT, WITH_ALPHA_OPT = 6, 8, 10, 12
HALF, BGRA8, ALPHA = 1, 0, 3            # BT709HIP_FORMAT_RGBA16F, _BGRA8_SRGB, _BGRA8_ALPHA
APPLE, SRGB, LIN = 0, 1, 2
W, H = 64, 16


def test_enumerator_and_bindings_agree_and_nothing_was_exported(tmp_path):
    src, exe = tmp_path / "ids.c", tmp_path / "ids"
    src.write_text('#include <stdio.h>\n#include "bt709hip_ext.h"\nint main(void) {\n'
                   '  printf("%d %d %d\\n", (int)BT709HIP_CTX_OPT_ENCODE_HALF_INPUT, (int)BT709HIP_VERSION, (int)BT709HIP_FORMAT_RGBA16F);\n  return 0;\n}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ids = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert ids == [OPT, 504, HALF]
    assert (_capi.CTX_OPT_ENCODE_HALF_INPUT, _capi.ABI_VERSION, hc.OPT_HALF_INPUT) == (OPT, 504, OPT)
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103  # no export
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    assert "kEncodeHalfInputOption = BT709HIP_CTX_OPT_ENCODE_HALF_INPUT" in hpp


def test_header_block_states_the_contract():
    comment = re.search(r"/\* BT709HIP_CTX_OPT_ENCODE_HALF_INPUT\..*?\*/", abi_headers.ext_text(), flags=re.S).group(0)
    for word in ("BT709HIP_FORMAT_RGBA16F", "A is not read", "NaN -> 0", "BT709_from_linear", "/ 4.0f", "BT709HIP_GAMMA_LINEAR", "BT709HIP_ERR_TRANSFER",
                 "BT709HIP_ERR_STRIDE", "8-byte aligned", "BT709HIP_ERR_UNSUPPORTED", "OUT OF SCOPE", "BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY",
                 "BT709HIP_CTX_OPT_ENCODE_CONVERT", "BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA", "BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT", "BT709HIP_ERR_NOT_SETUP",
                 "bt709hip_encoder_prepare", "encode_rgba16f_nv12", "encode_rgba16f_i420", "encode_rgba16f_nv12_blocks", "encode_rgba16f_i420_blocks",
                 "bt709hip_last_launch_info", "TWICE AS WIDE", "BT709HIP_CTX_OPT_ENCODE_ROW_PAIRS", "_ENCODE_THREADS", "_XCD_BANDS", "are ignored",
                 "not clamped", "never touches the device", "65535"):
        assert word in comment, word
    assert "BT709HIP_CTX_OPT_ENCODE_HALF_INPUT" in abi_headers.core_text()


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_half") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
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
    """A context and two allocations, texels and frames (launches touch nothing on the fake runtime, so pictures may overlap)."""

    def __init__(self, lib):
        self.lib = lib
        self.ctx = C.c_void_p()
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0
        self.src, self.dst = C.c_void_p(), C.c_void_p()
        for p in (self.src, self.dst):
            assert lib.bt709hip_malloc(self.ctx, 1 << 20, C.byref(p)) == 0

    def set(self, value, option=OPT):
        return self.lib.bt709hip_context_set_option(self.ctx, option, value)

    def surfs(self, n=1, fmt=HALF, w=W, h=H, step=None):
        px = 8 if fmt == HALF else 4
        step = px * w * h if step is None else step
        return (_capi.Surface * n)(*[_capi.Surface(self.src.value + i * step, px * w, w, h, fmt, 0) for i in range(n)])

    def frames(self, n=1, w=W, h=H, step=W * H * 2, cbcr_stride=None):
        return (_capi.Frame * n)(*[_capi.Frame(self.dst.value + i * step, w, self.dst.value + i * step + W * H, cbcr_stride or w, w, h, 0, 0) for i in range(n)])

    def encode(self, n, surfs, frames, gi=LIN, go=APPLE, stream=None, wait=1):
        if n == 1:
            return self.lib.bt709hip_encode(self.ctx, surfs, frames, gi, go, stream, wait)
        return self.lib.bt709hip_encode_batch(self.ctx, n, surfs, frames, gi, go, stream, wait)

    def kernels(self, mark):
        from test_fake_hip import log
        return [o for o in log(self.lib, mark) if o[0].startswith("kernel:")]

    def close(self):
        for p in (self.src, self.dst):
            assert self.lib.bt709hip_free(self.ctx, p) == 0
        assert self.lib.bt709hip_context_destroy(self.ctx) == 0


@pytest.fixture()
def rig(fake):
    r = Rig(fake)
    yield r
    r.close()


def held(rig):
    """There is no getter (no export was added): the held value shows in what the next call does with RGBA16F input --
    BT709HIP_ERR_UNSUPPORTED at 0, encoded at 1."""
    rc = rig.encode(1, rig.surfs(), rig.frames())
    assert rc in (0, _capi.ERR_UNSUPPORTED)
    return 0 if rc else 1


def test_option_domain(fake, rig):
    lib = fake
    assert lib.bt709hip_context_set_option(None, OPT, 1) == _capi.ERR_INVALID_ARG
    assert held(rig) == 0  # the default: format 1 is still refused
    for value in (1, 0, 1):
        mark = lib.fake_hip_log_size()
        assert rig.set(value) == _capi.OK
        for bad in (2, -1, 1 << 30):
            assert rig.set(bad) == _capi.ERR_INVALID_ARG, bad  # refused, not clamped ...
        assert lib.fake_hip_log_size() == mark                 # setting it logs nothing: it never touches the device
        assert held(rig) == value                              # ... and the option keeps its value
    assert rig.set(0) == _capi.OK
    for other in (13, 15):  # the ids next to it are no options
        assert lib.bt709hip_context_set_option(rig.ctx, other, 0) == _capi.ERR_INVALID_ARG
        assert lib.bt709hip_context_set_option(rig.ctx, other, 1) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_abi_version() == 504


def test_with_the_option_off_half_input_is_refused_as_it_was(fake, rig):
    mark = fake.fake_hip_log_size()
    assert rig.encode(1, rig.surfs(), rig.frames()) == _capi.ERR_UNSUPPORTED
    assert rig.encode(3, rig.surfs(3), rig.frames(3)) == _capi.ERR_UNSUPPORTED
    assert rig.encode(1, rig.surfs(), rig.frames(), SRGB, APPLE) == _capi.ERR_UNSUPPORTED
    assert fake.fake_hip_log_size() == mark


def test_half_calls_are_one_launch_each_under_both_layouts(fake, rig):
    assert rig.set(1) == 0
    mark = fake.fake_hip_log_size()
    for go in (APPLE, SRGB, LIN):
        assert rig.encode(1, rig.surfs(), rig.frames(), LIN, go) == 0
    assert rig.encode(4, rig.surfs(4), rig.frames(4)) == 0
    assert rig.set(_capi.CHROMA_I420, LAYOUT_OPT) == 0
    assert rig.encode(2, rig.surfs(2), rig.frames(2, cbcr_stride=W // 2)) == 0
    assert rig.set(_capi.CHROMA_NV12, LAYOUT_OPT) == 0
    assert rig.encode(1, rig.surfs(w=0, h=0), rig.frames(w=0, h=0)) == 0  # an empty picture: nothing to do
    assert [k[2] for k in rig.kernels(mark)] == [1, 1, 1, 4, 2]
    # 8-byte aligned texels and odd plane pitches are valid calls (the general kernel's)
    s = rig.surfs()
    s[0].bgra += 8
    f = rig.frames()
    f[0].y_stride, f[0].cbcr_stride = W + 1, W + 3
    assert rig.encode(1, s, f) == 0
    # 70 evenly spaced pictures: more than the pointer table holds
    assert rig.encode(70, rig.surfs(70, step=64), rig.frames(70, step=32)) == 0


def test_every_refusal_alone_and_in_a_batch_enqueues_nothing(fake, rig):
    lib = fake
    assert rig.set(1) == 0
    for go in (APPLE, SRGB, LIN):
        assert lib.bt709hip_encoder_prepare(rig.ctx, LIN, go) == 0
    mark = lib.fake_hip_log_size()

    def call(n, edit_surf=None, edit_frame=None, gi=LIN, go=APPLE, index=None, **kw):
        surfs, frames = rig.surfs(n, **kw), rig.frames(n, **{k: v for k, v in kw.items() if k in ("w", "h")})
        i = n - 1 if index is None else index
        if edit_surf:
            edit_surf(surfs[i])
        if edit_frame:
            edit_frame(frames[i])
        return rig.encode(n, surfs, frames, gi, go)

    def put(name, value):
        return lambda s: setattr(s, name, value)

    for n in (1, 3):
        whole = n == 1  # a pitch is one per call: changed in one picture of a batch it is a size mismatch first, as for BGRA8 input
        # the texel pointer and pitch: the rule of an RGBA16F decode target
        assert call(n, put("bgra", rig.src.value + 4)) == _capi.ERR_STRIDE
        assert call(n, put("bgra", rig.src.value + 2)) == _capi.ERR_STRIDE
        assert call(n, put("stride", 8 * W + 4)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)
        assert call(n, put("stride", 8 * W - 8)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)
        assert call(n, put("stride", 4 * W)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)  # a BGRA8 picture's pitch
        assert call(n, put("stride", 1 << 32)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)
        # reserved, formats
        assert call(n, put("reserved", 1)) == _capi.ERR_UNSUPPORTED
        assert call(n, put("format", 2)) == _capi.ERR_UNSUPPORTED
        if n > 1:
            assert call(n, put("format", BGRA8)) == _capi.ERR_SIZE_MISMATCH  # mixed formats in a batch
            assert call(n, put("format", HALF), fmt=BGRA8) == _capi.ERR_SIZE_MISMATCH
        # the input gamma: the texels hold linear light
        assert call(n, gi=SRGB) == _capi.ERR_TRANSFER
        assert call(n, gi=APPLE, go=LIN) == _capi.ERR_TRANSFER
        # output gammas outside the encoder's three: what the BGRA8 encoder answers
        for go in (3, 4, -1):
            assert call(n, go=go) == call(n, go=go, fmt=BGRA8, gi=SRGB) == _capi.ERR_INVALID_ARG
        # the encoder's own rules hold
        assert call(n, w=W - 1) == _capi.ERR_ODD_DIMENSIONS
        assert call(n, edit_frame=put("width", W + 2)) == _capi.ERR_SIZE_MISMATCH
        assert call(n, edit_frame=put("y", None)) == _capi.ERR_INVALID_ARG
        assert call(n, put("bgra", None)) == _capi.ERR_INVALID_ARG
        assert call(n, edit_frame=put("y_stride", W - 1)) == (_capi.ERR_STRIDE if whole else _capi.ERR_SIZE_MISMATCH)
        # the three options that are out of scope, each away from its default: after the usual validation
        for option, value, default in ((PREMULTIPLY_OPT, 1, 0), (CONVERT_OPT, _capi.CONVERT_PACKED444, 0), (CONVERT_OPT, _capi.CONVERT_POINT420, 0),
                                       (WITH_ALPHA_OPT, 1, 0)):
            assert rig.set(value, option) == 0
            try:
                assert call(n) == _capi.ERR_UNSUPPORTED, (option, value)
                assert call(n, w=W - 1) == _capi.ERR_ODD_DIMENSIONS          # ... which still comes first
                assert call(n, gi=SRGB) == _capi.ERR_TRANSFER
                assert call(n, put("bgra", rig.src.value + 4)) == _capi.ERR_STRIDE
            finally:
                assert rig.set(default, option) == 0
    # a pointer table holds 32 pictures
    uneven = rig.surfs(33, step=64)
    uneven[5].bgra += 16
    assert rig.encode(33, uneven, rig.frames(33, step=32)) == _capi.ERR_UNSUPPORTED
    assert rig.kernels(mark) == [] and lib.fake_hip_log_size() == mark, "a refused call enqueued something"
    uneven = rig.surfs(32, step=64)
    uneven[5].bgra += 16
    assert rig.encode(32, uneven, rig.frames(32, step=32)) == 0
    assert [k[2] for k in rig.kernels(mark)] == [32]


def test_bgra8_calls_issue_the_same_launches_with_the_option_at_either_value(fake, rig):
    from test_fake_hip import log
    lib = fake
    issued = {}
    for value in (0, 1):
        assert rig.set(value) == 0
        mark = lib.fake_hip_log_size()
        records = []
        for n, fmt, gi, go in ((1, BGRA8, SRGB, APPLE), (4, BGRA8, SRGB, SRGB), (70, BGRA8, LIN, LIN), (1, ALPHA, LIN, LIN), (3, ALPHA, LIN, LIN)):
            assert rig.encode(n, rig.surfs(n, fmt=fmt, step=4 * W * H if n < 70 else 64), rig.frames(n, step=W * H * 2 if n < 70 else 32), gi, go) == 0
            info = _capi.LaunchInfo()
            assert lib.bt709hip_last_launch_info(C.byref(info)) == 0
            records.append((tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands))
        issued[value] = ([(o[0], o[2], o[3]) for o in log(lib, mark)], records)
    assert issued[0] == issued[1] and len(issued[0][0]) == 5


def test_capture_needs_one_prepare(fake):
    """bt709hip_encoder_prepare(ctx, LINEAR, out) makes everything the half path needs: the half encode behind it uploads nothing
    and can be captured; without it a captured half encode finds the table missing."""
    lib = fake
    for prepared in (0, 1):
        rig = Rig(lib)
        try:
            S, g = C.c_void_p(), C.c_void_p()
            assert lib.bt709hip_stream_create(rig.ctx, C.byref(S)) == 0
            assert rig.set(1) == 0
            if prepared:
                assert lib.bt709hip_encoder_prepare(rig.ctx, LIN, APPLE) == 0
            allocations = lib.fake_hip_allocations(0)
            mark = lib.fake_hip_log_size()
            assert lib.bt709hip_graph_begin_capture(rig.ctx, S) == 0
            assert rig.set(0) == 0 and rig.set(1) == 0  # the setter works while the stream is being captured
            rc = rig.encode(2, rig.surfs(2), rig.frames(2), LIN, APPLE, S, 0)
            assert lib.bt709hip_graph_end_capture(rig.ctx, S, C.byref(g)) == 0
            assert rc == (_capi.OK if prepared else _capi.ERR_NOT_SETUP)
            assert lib.fake_hip_allocations(0) == allocations and rig.kernels(mark) == []
            if prepared:
                assert lib.bt709hip_graph_launch(rig.ctx, g, S) == 0 and lib.bt709hip_stream_synchronize(rig.ctx, S) == 0
                issued = rig.kernels(mark)
                assert len(issued) == 1 and issued[0][2] == 2
            assert lib.bt709hip_graph_destroy(rig.ctx, g) == 0 and lib.bt709hip_stream_destroy(rig.ctx, S) == 0
        finally:
            rig.close()


# ------------------------------------------------------------------ the Python mirror

def test_python_mirror_sets_and_restores_the_option():
    """convertIntoCoreVideoBuffer[s] of RGBA16Float textures sets the option around the one call and puts 0 back, also when the call
    is refused or raises; BGRA8 textures never touch it."""
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

        def bt709hip_encode(self, handle, surf, frame, gi, go, stream, wait):
            calls.append(("encode1", gi, go))
            return self.rc

    ctx = mb.MetalRenderContext(0)
    ctx.lib, ctx.handle = Lib(), 1
    try:
        conv = mb.BGRAToBT709Converter
        halves = [mb.BGRATexture(ctx, W, H, ptr=0x10000 * (i + 1), pixelFormat=mb.MTLPixelFormatRGBA16Float) for i in range(2)]
        bytes_ = [mb.BGRATexture(ctx, W, H, ptr=0x10000 * (i + 9)) for i in range(2)]
        outs = [mb.CVPixelBuffer(ctx, W, H, planes=(0x100000 * (i + 1), 0x100000 * (i + 1) + W * H)) for i in range(2)]
        assert conv.convertIntoCoreVideoBuffers(halves, outs, LIN, APPLE)
        assert calls == [("set", OPT, 1), ("encode", 2, [HALF, HALF], [8 * W, 8 * W], LIN, APPLE), ("set", OPT, 0)]
        del calls[:]
        assert conv.convertIntoCoreVideoBuffer(halves[0], outs[0], LIN, SRGB)
        assert calls == [("set", OPT, 1), ("encode", 1, [HALF], [8 * W], LIN, SRGB), ("set", OPT, 0)]
        del calls[:]
        ctx.lib.rc = _capi.ERR_TRANSFER  # a refused call: False, the option back at 0
        assert not conv.convertIntoCoreVideoBuffers(halves, outs, SRGB, APPLE)
        assert calls[0] == ("set", OPT, 1) and calls[-1] == ("set", OPT, 0)
        del calls[:]
        ctx.lib.rc = RuntimeError("the call raised")
        with pytest.raises(RuntimeError):
            conv.convertIntoCoreVideoBuffers(halves, outs, LIN, APPLE)
        assert calls[0] == ("set", OPT, 1) and calls[-1] == ("set", OPT, 0)
        del calls[:]
        ctx.lib.rc = _capi.OK
        alpha = [mb.CVPixelBuffer(ctx, W, H, planes=(0x900000, None))]
        assert not conv.convertIntoCoreVideoBuffers(halves[:1], outs[:1], LIN, APPLE, alphaPixelBuffers=alpha)  # no alpha frame from halves
        assert calls == []
        assert conv.convertIntoCoreVideoBuffers(bytes_, outs, SRGB, APPLE)  # BGRA8 textures: the call of before, the option untouched
        assert conv.convertIntoCoreVideoBuffer(bytes_[0], outs[0], SRGB, APPLE)
        assert not [c for c in calls if c[0] == "set" and c[1] == OPT]
    finally:
        ctx.handle = None


# ------------------------------------------------------------------ the facts the GPU sweeps rest on

@pytest.fixture(scope="module")
def expect(oracle):
    return hc.Expect(oracle)


@pytest.mark.parametrize("out_gamma,fewest", [(GAMMA_SRGB, 10), (GAMMA_APPLE, 8), (GAMMA_LINEAR, 5)])
def test_the_halves_in_unit_range_reach_every_byte_monotonically(expect, out_gamma, fewest):
    table = expect.code_table(out_gamma)
    assert table.size == 15361 and table[0] == 0 and table[-1] == 255
    assert np.all(np.diff(table.astype(np.int32)) >= 0), "F is not monotone over the half codes"
    counts = np.bincount(table, minlength=256)
    assert counts.min() == fewest, counts.min()  # every byte is reached, the rarest by this many halves
    lo, hi = hc.representatives(table)
    assert np.array_equal(lo[1:], hi[:-1] + 1)   # thresholds sit between neighbouring codes


def test_flat_blocks_average_to_the_value_itself():
    """((h + h) + h) + h and / 4 are exact in float32 for every half in [0, 1]: a flat block's average is the texel's value, so its
    expectation is the byte matrix of F(v) alone -- the (LINEAR, LINEAR) encode of the BGRA8 twin."""
    v = hc.saturate(np.arange(hc.ONE + 1, dtype=np.uint16))
    s = ((v + v) + v) + v
    assert s.dtype == np.float32
    assert np.array_equal(s.astype(np.float64), 4.0 * v.astype(np.float64))
    assert np.array_equal(s / np.float32(4.0), v)


def test_saturation_of_every_half_code():
    codes = np.arange(65536, dtype=np.uint16)
    v = hc.saturate(codes)
    f = codes.view(np.float16).astype(np.float64)
    assert v.dtype == np.float32 and not np.isnan(v).any() and not np.signbit(v).any()
    assert np.all(v[np.isnan(f)] == 0) and np.all(v[f < 0] == 0) and np.all(v[f > 1] == 1) and v[0x8000] == 0 and v[0x7C00] == 1 and v[0xFC00] == 0
    inside = (f >= 0) & (f <= 1)
    assert np.array_equal(v[inside].astype(np.float64), f[inside]) and inside.sum() == 15361 + 1  # and -0
    assert np.array_equal(hc.saturated_code(codes)[:hc.ONE + 1], codes[:hc.ONE + 1])


def test_flat_blocks_equal_the_twin_encode(expect, oracle):
    rng = np.random.default_rng(19)
    for out_gamma in hc.OUT_GAMMAS:
        blocks = rng.integers(0, hc.ONE + 1, (8, 16, 4), dtype=np.uint16)
        texels = np.repeat(np.repeat(blocks, 2, 0), 2, 1)
        y, c = expect.planes(texels, out_gamma)
        twin = hc.twin_words(expect.code_table(out_gamma)[texels[..., :3]])
        ty, tc = oracle.encode_nv12(twin, 32, 16, GAMMA_LINEAR, GAMMA_LINEAR)
        assert np.array_equal(y, ty) and np.array_equal(c, tc)


def test_helper_against_the_references_own_inlines(expect, oracle, reference):
    """Where the reference's headers are built: F over all 15361 codes and over averages between them, and the byte matrix over
    random triples, from ref_linear_to_*, ref_transfer_to_byte and ref_encode_pixel."""
    if reference is None:
        return  # nothing to hold it against on this machine: the oracle itself is held to the reference's recorded outputs elsewhere
    R = reference.lib
    v = hc.saturate(np.arange(hc.ONE + 1, dtype=np.uint16))
    mids = ((v[:-1] + v[1:]) + v[1:] + v[1:]) / np.float32(4.0)
    for values in (v, mids[::7]):
        for out_gamma in hc.OUT_GAMMAS:
            want = []
            for x in values.tolist():
                if out_gamma == GAMMA_SRGB:
                    want.append(R.ref_transfer_to_byte(GAMMA_SRGB, R.ref_linear_to_srgb(x)))     # round(255 * sRGB curve)
                elif out_gamma == GAMMA_APPLE:
                    want.append(R.ref_transfer_to_byte(GAMMA_SRGB, R.ref_linear_to_apple196(x)))
                else:
                    want.append(R.ref_transfer_to_byte(GAMMA_SRGB, x))                            # round(255 * v)
            assert np.array_equal(expect.from_linear(out_gamma, values), np.array(want, np.uint8)), out_gamma
    rng = np.random.default_rng(1919)
    rgb = rng.integers(0, 256, (2000, 3), dtype=np.uint8)
    got = expect.matrix(rgb)
    for (r, g, b), ycc in zip(rgb.tolist(), got.tolist()):
        assert tuple(ycc) == reference.encode_pixel(GAMMA_SRGB, r, g, b)


# ------------------------------------------------------------------ the generated code

def kernel(asm, name, layout):
    sym = "_ZN5bt709%d%sILj%dEEEvNS_12EncodeParamsE" % (len(name), name, layout)
    assert len(re.findall(r"^%s:" % sym, asm, re.M)) == 1, sym
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % sym, asm, re.S | re.M)
    lines = [l.split(";")[0].strip() for l in m.group(1).split("\n")]
    meta = re.search(r"\.name:\s+%s\b.*?(?=\n  - \.a|\Z)" % re.escape(sym), asm, flags=re.S)
    assert meta, name
    return [l for l in lines if l and not l.startswith(".") and not l.endswith(":")], meta.group(0)


def meta_int(meta, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def descriptor(asm, name, layout):
    """The .amdhsa_ directives of the kernel's descriptor -> {key: int}"""
    sym = "_ZN5bt709%d%sILj%dEEEvNS_12EncodeParamsE" % (len(name), name, layout)
    block = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), asm, re.S).group(1)
    return {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", block)}


@pytest.mark.parametrize("layout", [0, 1])
def test_isa_of_the_half_kernels(layout):
    from metalbt709decoder_amd import build
    asm = open(build.emit_asm()).read()
    ins, meta = kernel(asm, "encode_rgba16f", layout)
    ops = [i.split()[0] for i in ins]
    # input: 16-byte non-temporal loads, the first pair and the prefetched pair; the only other global loads stage the table
    loads = [i for i in ins if i.startswith("global_load")]
    texel_loads = [i for i in loads if re.search(r"\bnt\b", i)]
    assert len(texel_loads) == 4 and all(i.startswith("global_load_dwordx4") for i in texel_loads), loads
    assert all(i.startswith("global_load_dwordx4") for i in loads)
    # no scratch, no flat accesses, no static LDS (the table sits at address 0 of the dynamic segment)
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))]
    kd = descriptor(asm, "encode_rgba16f", layout)
    assert meta_int(meta, "private_segment_fixed_size") == 0 and kd["private_segment_fixed_size"] == 0 and kd["group_segment_fixed_size"] == 0
    assert kd["kernarg_size"] == 880 + 256  # EncodeParams did not grow
    # the modes the saturating conversion rests on: the clamp bit turns NaN into 0 under DX10_CLAMP, subnormal halves are not flushed
    assert kd["dx10_clamp"] == 1 and kd["float_denorm_mode_16_64"] == 3 and kd["float_round_mode_32"] == 0
    # one conversion with the clamp bit per pixel channel, nothing else converts a half
    cvt = [i for i in ins if i.startswith("v_cvt_f32_f16")]
    assert len(cvt) == 12 and all(" clamp " in i + " " for i in cvt), cvt
    # fifteen table lookups (12 pixel channels, 3 averages)
    assert ops.count("ds_read_b64") == 15
    # no contracted multiply-add apart from div_const's two per chroma sample
    assert ops.count("v_fmac_f32_e32") + ops.count("v_fma_f32") == 4 and not [o for o in ops if o.startswith(("v_mad_f32", "v_pk_"))]
    # the mode switch brackets the six conversions, nothing between
    setreg = [k for k, o in enumerate(ops) if o.startswith("s_setreg")]
    assert len(setreg) == 2 and [k for k, o in enumerate(ops) if o == "v_cvt_pk_u8_f32"] == list(range(setreg[0] + 1, setreg[1])) and setreg[1] - setreg[0] == 7
    # stores: non-temporal, 2 + 2 bytes of Y and 2 of CbCr, or 1 + 1 of U and V
    stores = [i for i in ins if i.startswith("global_store")]
    assert all(re.search(r"\bnt\b", s) for s in stores), stores
    kinds = sorted(s.split()[0].replace("_d16_hi", "") for s in stores)
    assert kinds == (["global_store_byte", "global_store_byte", "global_store_short", "global_store_short"] if layout else ["global_store_short"] * 3), kinds
    assert meta_int(meta, "vgpr_count") <= 64  # eight waves per SIMD
    # the general kernel: bytes, whatever the alignment
    ins, meta = kernel(asm, "encode_rgba16f_blocks", layout)
    stores = [i.split()[0] for i in ins if i.startswith(("global_store", "flat_store", "buffer_store"))]
    assert len(stores) == 6 and set(stores) <= {"global_store_byte", "global_store_byte_d16_hi"}, stores
    assert meta_int(meta, "private_segment_fixed_size") == 0 and not [i for i in ins if i.startswith(("scratch_", "flat_"))]
    # texels: two per row, which the compiler fetches as one 16-byte load at the texels' 8-byte alignment (legal in global memory)
    loads = {i.split()[0] for i in ins if i.startswith(("global_load", "flat_load", "buffer_load"))}
    assert loads <= {"global_load_dwordx2", "global_load_dwordx4"}, loads
