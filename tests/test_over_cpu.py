"""BT709HIP_OPT_COMPOSITE_OVER, the parts that need no GPU: the option and its refusals on a context-less
decoder, the constants of the four bindings, the two identities the definition rests on, and the Python mirror."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_headers
import metalbt709decoder_amd as mb
import over_cases as oc
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_LINEAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = _capi.OPT_COMPOSITE_OVER


@pytest.fixture(scope="module")
def lib():
    return mb.load_library()


def _bare_decoder(lib, has_alpha):
    h = C.c_void_p()
    assert lib.bt709hip_decoder_create(None, mb.MetalBT709GammaApple, has_alpha, C.byref(h)) == _capi.OK
    return h


def _get(lib, dec):
    v = C.c_int(-12345)
    assert lib.bt709hip_decoder_get_option(dec, OPT, C.byref(v)) == _capi.OK
    return v.value


def test_option_round_trip_and_refusals(lib):
    """A decoder without a context: the option is a plain property, nothing touches a device."""
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


def test_constants_agree_across_the_bindings(lib):
    """One option value and two named values, no export: the header, the ctypes twin, the C++ host and the Objective-C header."""
    header = open(os.path.join(ROOT, "include", "bt709hip_ext.h")).read()
    assert int(re.search(r"\bBT709HIP_OPT_COMPOSITE_OVER\s*=\s*(\d+)", header).group(1)) == 9 == _capi.OPT_COMPOSITE_OVER
    assert int(re.search(r"#define\s+BT709HIP_OVER_OFF\s+\((-?\d+)\)", header).group(1)) == -1 == _capi.OVER_OFF == oc.OVER_OFF
    assert int(re.search(r"#define\s+BT709HIP_OVER_DESTINATION\s+\((-?\d+)\)", header).group(1)) == -2 == _capi.OVER_DESTINATION == oc.OVER_DESTINATION
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    assert re.search(r"setCompositeOver\(int \w+\) \{ return setOption\(BT709HIP_OPT_COMPOSITE_OVER, \w+\); \}", hpp)
    assert "int background = BT709HIP_OVER_OFF;" in hpp
    objc = open(os.path.join(ROOT, "objc", "MetalBT709Decoder+HIP.h")).read()
    assert re.search(r"BT709HIPCompositeOverOff = -1, BT709HIPCompositeOverDestination = -2", objc)
    assert "@property (nonatomic, assign) int hipCompositeOver;" in objc
    impl = open(os.path.join(ROOT, "objc", "MetalBT709Decoder+HIP.m")).read()
    assert "bt709hip_decoder_set_option(_hipDecoder, BT709HIP_OPT_COMPOSITE_OVER, self.hipCompositeOver)" in impl
    assert "_hipCompositeOverSet ? _hipCompositeOver : BT709HIP_OVER_OFF" in impl  # an unset int property is not "over black"
    # no export, no ABI bump
    assert lib.bt709hip_abi_version() == 504 == _capi.ABI_VERSION
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103


def test_the_two_identities_of_the_definition(lib, oracle):
    """A_s = 255: the output is the source word.  A_s = 0 and s = 0: the output is the background word.  Both for all 256 bytes,
    and both rest on encode(lin[b]) == b and 255 * (1.0f / 255.0f) == 1.0f, checked here on the oracle's tables and on the
    table the kernels read (the library's replay of its log-bucket lookup).  Colour mode: every output alpha is 255."""
    lin, thr = oc.tables(oracle)
    b = np.arange(256)
    assert np.array_equal(np.searchsorted(thr, lin, side="right"), b)
    assert np.float32(255.0) * (np.float32(1.0) / np.float32(255.0)) == np.float32(1.0)
    for v in lin:  # what over_encode looks up (bt709_kernels.hip): the LINEAR composite's log-bucket table
        assert lib.bt709hip_gamma_lookup_decode(GAMMA_LINEAR, C.c_float(float(v)), None, None, None) == int(np.searchsorted(thr, v, side="right"))
    s, d = np.meshgrid(b, b, indexing="ij")  # every source byte over every background byte
    opaque = np.stack([s, s, s, np.full_like(s, 255)], -1).astype(np.uint8)
    background = np.stack([d, d, d, 255 - d], -1).astype(np.uint8)
    assert np.array_equal(oc.composite_over(opaque, background, lin, thr), opaque)
    clear = np.zeros_like(opaque)
    assert np.array_equal(oc.composite_over(clear, background, lin, thr), background)
    for colour in (0, 0xFFFFFF, 0x4080C0):
        assert np.array_equal(oc.composite_over(opaque, colour, lin, thr), opaque)
        assert np.array_equal(oc.composite_over(clear, colour, lin, thr), np.broadcast_to(oc.colour_word(colour), clear.shape))
        ramp = np.stack([s // 2, s // 3, s // 4, s], -1).astype(np.uint8)  # premultiplied: colour <= alpha
        assert np.all(oc.composite_over(ramp, colour, lin, thr)[..., 3] == 255)
    # the blend's values reach the table the same way: a sample of (s, A_s, d) against the library's lookup
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, (512, 4), dtype=np.uint8)
    dst = rng.integers(0, 256, (512, 4), dtype=np.uint8)
    want = oc.composite_over(src, dst, lin, thr)
    k = (255 - src[:, 3].astype(np.int32)).astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    for i in range(512):
        v = min(np.float32(1.0), lin[src[i, 1]] + k[i] * lin[dst[i, 1]])
        assert lib.bt709hip_gamma_lookup_decode(GAMMA_LINEAR, C.c_float(float(v)), None, None, None) == want[i, 1]


def test_python_mirror_maps_the_three_forms():
    d = mb.MetalBT709Decoder()
    d.hasAlphaChannel = True
    assert d.compositeOver is None
    for value, word in (("destination", -2), ((0, 0, 0), 0), ((255, 255, 255), 0xFFFFFF), ((1, 2, 3), 0x010203), (None, -1)):
        d.compositeOver = value  # before setupMetal: applied at setup, like every option
        assert d._options[OPT] == word
        assert d.compositeOver == value
    for bad in ("colour", (0, 0, 256), (-1, 0, 0)):
        with pytest.raises(ValueError):
            d.compositeOver = bad
    assert d.compositeOver is None
    opaque = mb.MetalBT709Decoder()
    opaque.compositeOver = None  # nothing to switch off: setupMetal must not hand the option to a decoder without alpha
    assert OPT not in opaque._options


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_over") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_set_device_count(1)
    return lib


class FakeRig:
    """A context, an alpha decoder and four 64 x 16 frames with alpha planes and targets carved evenly from three allocations."""

    def __init__(self, lib, w=64, h=16, n=4):
        self.lib, self.w, self.h, self.n = lib, w, h, n
        self.ctx, self.dec, self.stream = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0
        assert lib.bt709hip_decoder_create(self.ctx, 0, 1, C.byref(self.dec)) == 0
        assert lib.bt709hip_stream_create(self.ctx, C.byref(self.stream)) == 0
        self.mem = []
        for nbytes in (n * w * h * 3 // 2, n * w * h * 3 // 2, n * w * h * 8):
            p = C.c_void_p()
            assert lib.bt709hip_malloc(self.ctx, nbytes, C.byref(p)) == 0
            self.mem.append(p.value)
        step = w * h * 3 // 2
        self.frames = (_capi.Frame * n)(*[_capi.Frame(self.mem[0] + i * step, w, self.mem[0] + i * step + w * h, w, w, h, 1, 2) for i in range(n)])
        self.alphas = (_capi.Frame * n)(*[_capi.Frame(self.mem[1] + i * step, w, self.mem[1] + i * step + w * h, w, w, h, 1, 3) for i in range(n)])

    def surfs(self, w=None, h=None, fmt=0):
        w, h = w or self.w, h or self.h
        px = 8 if fmt == _capi.FORMAT_RGBA16F else 4
        return (_capi.Surface * self.n)(*[_capi.Surface(self.mem[2] + i * self.w * self.h * 8, w * px, w, h, fmt, 0) for i in range(self.n)])

    def set_over(self, value):
        return self.lib.bt709hip_decoder_set_option(self.dec, OPT, value)

    def kernels(self, mark):
        from test_fake_hip import log
        return [o for o in log(self.lib, mark) if o[0].startswith("kernel:")]

    def close(self):
        lib = self.lib
        assert lib.bt709hip_decoder_destroy(self.dec) == 0
        for p in self.mem:
            assert lib.bt709hip_free(self.ctx, p) == 0
        assert lib.bt709hip_stream_destroy(self.ctx, self.stream) == 0 and lib.bt709hip_context_destroy(self.ctx) == 0


@pytest.fixture()
def fake_rig(fake):
    r = FakeRig(fake)
    yield r
    r.close()


def test_shim_refuses_the_other_paths_after_their_validation(fake, fake_rig):
    lib, r = fake, fake_rig
    s, f16, half, scaled = r.surfs(), r.surfs(fmt=_capi.FORMAT_RGBA16F), r.surfs(r.w // 2, r.h // 2), r.surfs(48, 10)
    for value in (-2, 0, 0xFFFFFF):
        assert r.set_over(value) == 0
        mark = lib.fake_hip_log_size()
        assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, f16, None, 1) == _capi.ERR_UNSUPPORTED
        assert lib.bt709hip_decode(r.dec, r.frames, r.alphas, f16, r.w, r.h, None, 1) == _capi.ERR_UNSUPPORTED
        for entry, out in (("bt709hip_decode_half", half), ("bt709hip_decode_scaled", scaled)):
            assert getattr(lib, entry)(r.dec, r.frames, r.alphas, out, None, 1) == _capi.ERR_UNSUPPORTED
            assert getattr(lib, entry + "_batch")(r.dec, r.n, r.frames, r.alphas, out, None, 1) == _capi.ERR_UNSUPPORTED
            # the usual validation comes first, in the usual order
            assert getattr(lib, entry)(r.dec, r.frames, None, out, None, 1) == _capi.ERR_INVALID_ARG
        assert lib.bt709hip_decode_half(r.dec, r.frames, r.alphas, scaled, None, 1) == _capi.ERR_SIZE_MISMATCH
        assert r.kernels(mark) == []  # nothing was launched
        assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, s, None, 1) == 0
        assert len(r.kernels(mark)) == 1
    assert r.set_over(-1) == 0
    mark = lib.fake_hip_log_size()
    assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames, r.alphas, f16, None, 1) == 0
    assert lib.bt709hip_decode_half_batch(r.dec, r.n, r.frames, r.alphas, half, None, 1) == 0
    assert lib.bt709hip_decode_scaled_batch(r.dec, r.n, r.frames, r.alphas, scaled, None, 1) == 0
    assert len(r.kernels(mark)) == 3


def test_shim_builds_the_table_at_setup_and_not_inside_a_capture(fake, fake_rig):
    """A decoder that was set up before the option was turned on holds no lin[] table: its first composite decode builds it,
    unless the stream records a graph -- then ERR_NOT_SETUP, until bt709hip_decoder_setup (a no-op otherwise) has built it."""
    lib, r = fake, fake_rig
    s, g = r.surfs(), C.c_void_p()
    assert lib.bt709hip_decoder_setup(r.dec) == 0
    mark = lib.fake_hip_log_size()
    assert r.set_over(-2) == 0 and r.set_over(0x808080) == 0 and r.set_over(-2) == 0
    assert lib.fake_hip_log_size() == mark  # setting the option never touches the device
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    assert lib.bt709hip_decode(r.dec, r.frames, r.alphas, s, r.w, r.h, r.stream, 0) == _capi.ERR_NOT_SETUP
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0 and lib.bt709hip_graph_destroy(r.ctx, g) == 0
    assert r.kernels(mark) == []
    assert lib.bt709hip_decoder_setup(r.dec) == 0  # builds what the option needs
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    assert lib.bt709hip_decode(r.dec, r.frames, r.alphas, s, r.w, r.h, r.stream, 0) == 0
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0
    assert r.kernels(mark) == []  # recorded, not run
    assert lib.bt709hip_graph_launch(r.ctx, g, r.stream) == 0 and lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    assert len(r.kernels(mark)) == 1
    assert lib.bt709hip_graph_destroy(r.ctx, g) == 0
    # a fresh decoder with the option on: bt709hip_decoder_setup builds the table with the others
    fresh = C.c_void_p()
    assert lib.bt709hip_decoder_create(r.ctx, 0, 1, C.byref(fresh)) == 0
    assert lib.bt709hip_decoder_set_option(fresh, OPT, -2) == 0 and lib.bt709hip_decoder_setup(fresh) == 0
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    assert lib.bt709hip_decode(fresh, r.frames, r.alphas, s, r.w, r.h, r.stream, 0) == 0
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0 and lib.bt709hip_graph_destroy(r.ctx, g) == 0
    assert lib.bt709hip_decoder_destroy(fresh) == 0


def test_shim_issues_queued_frames_before_the_option_changes(fake, fake_rig):
    """The option's value is decoder state: frames a coalescing decoder has queued go out under the value they were queued
    with, so a change issues them first (and a refused value changes nothing but still leaves nothing queued behind it)."""
    lib, r = fake, fake_rig
    s = r.surfs()
    assert r.set_over(0x102030) == 0 and lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COALESCE, 4) == 0
    mark = lib.fake_hip_log_size()
    for i in (0, 1):
        assert lib.bt709hip_decode(r.dec, C.byref(r.frames[i]), C.byref(r.alphas[i]), C.byref(s[i]), r.w, r.h, r.stream, 0) == 0
    assert r.kernels(mark) == []  # queued
    assert r.set_over(0xFFFFFF) == 0
    assert lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    issued = r.kernels(mark)
    assert len(issued) == 1 and issued[0][2] == 2  # one launch over the two frames
    for i in (2, 3):
        assert lib.bt709hip_decode(r.dec, C.byref(r.frames[i]), C.byref(r.alphas[i]), C.byref(s[i]), r.w, r.h, r.stream, 0) == 0
    assert lib.bt709hip_decoder_flush(r.dec, r.stream) == 0 and lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    issued = r.kernels(mark)
    assert len(issued) == 2 and issued[1][2] == 2


# ------------------------------------------------------------------ the generated code

def test_isa_of_the_over_kernels():
    """The blend rounds every operation on its own: the only fused multiply-adds are centre_norm's (bt709_device.h), as in the
    plain kernels.  Fast path: the background's 16-byte words are loaded non-temporally with the tile's other loads, before any
    table is staged (destination mode; colour mode loads none), the stores stream, no wait on memory sits between the first
    store and the last, and nothing spills.  Per lane (two quads): 48 lin[s] reads, 48 more for lin[d], 48 encode buckets."""
    from metalbt709decoder_amd import build
    asm = open(build.emit_asm()).read()
    # the kChromaNV12 (= 0: the leading ILj0E) instantiations
    bodies = dict(re.findall(r"^(_ZN5bt709\d+decode_(?:quads|blocks)_overILj0E\w*):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M))
    assert sorted(bodies) == sorted(["_ZN5bt70917decode_quads_overILj0ELi%dEEEvNS_12DecodeParamsE" % m for m in (1, 2)] +
                                    ["_ZN5bt70918decode_blocks_overILj0ELi%dEEEvNS_12DecodeParamsE" % m for m in (1, 2)])
    for name, body in bodies.items():
        for line in re.findall(r"^\s*(v_(?:pk_)?(?:fma|fmac|fmamk|fmaak|mad|mac|madmk|madak)_(?:f32|f16|legacy|mix)\w*\s[^\n]*)", body, flags=re.M):
            assert re.match(r"v_fmamk_f32 v\d+, v\d+, 0x3b808081, v\d+|v_fmac_f32_e32 v\d+, 0x3b808081, v\d+", line.strip()), (name, line)
        assert not re.search(r"\bv_pk_(mul|add|fma)_f32|\bv_(log|exp)_f32|s_setreg", body), name
        assert "scratch_" not in body, name
        meta = re.search(r"\.name:\s+%s\b.*?\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), asm, flags=re.S)
        assert meta and int(meta.group(1)) == 0, name
        destination = "ILj0ELi1E" in name  # OVER == kOverDestination
        if "quads" not in name:
            continue
        assert len(re.findall(r"global_load_dwordx4 [^\n]* nt\b", body)) == (4 if destination else 0), name
        assert len(re.findall(r"global_load_dword [^\n]* nt\b", body)) == 10, name  # 2 quads x (2 luma, 1 CbCr, 2 alpha rows)
        assert body.count("global_store_dwordx4") == 4 == len(re.findall(r"global_store_dwordx4 [^\n]* nt\b", body)), name
        first_write = body.index("ds_write")
        assert body.rindex(" nt") > first_write  # (the stores)
        assert all(m.start() < first_write for m in re.finditer(r"global_load_dword(?:x4)? [^\n]* nt\b", body)), name  # the tile first, then the tables
        first, last = body.index("global_store_dwordx4"), body.rindex("global_store_dwordx4")
        assert "vmcnt" not in body[first:last], name
        assert body.count("ds_read_b32") == (96 if destination else 48) and body.count("ds_read_b64") == 48, name
