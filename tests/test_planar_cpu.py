"""BT709HIP_OPT_CHROMA_LAYOUT (planar I420 frames), the parts that need no GPU: the option's domain on a
context-less decoder, the constants of the bindings, and -- on the shim built against the fake HIP runtime -- validation under
either layout, the refusals, the coalescing queue, rings that stay NV12; then the generated code of the new kernels.  (The fake
runtime's launchers report the NV12 kernel names whatever the layout: the names are the GPU tests' business.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_headers
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT, NV12, I420 = 11, 0, 1


@pytest.fixture(scope="module")
def lib():
    return mb.load_library()


def _get(lib, dec, opt=OPT):
    v = C.c_int(-12345)
    assert lib.bt709hip_decoder_get_option(dec, opt, C.byref(v)) == _capi.OK
    return v.value


@pytest.mark.parametrize("has_alpha", [0, 1])
def test_option_domain_and_round_trip(lib, has_alpha):
    """A decoder without a context: the option is a plain property, nothing touches a device."""
    dec = C.c_void_p()
    assert lib.bt709hip_decoder_create(None, mb.MetalBT709GammaApple, has_alpha, C.byref(dec)) == _capi.OK
    try:
        assert _get(lib, dec) == NV12  # the default
        for held in (I420, NV12, I420):
            assert lib.bt709hip_decoder_set_option(dec, OPT, held) == _capi.OK
            assert _get(lib, dec) == held
            for bad in (-1, 2, 7, 1 << 30, -(1 << 31)):
                assert lib.bt709hip_decoder_set_option(dec, OPT, bad) == _capi.ERR_INVALID_ARG
                assert _get(lib, dec) == held  # a refused value leaves the option as it was
    finally:
        lib.bt709hip_decoder_destroy(dec)


def test_constants_agree_and_nothing_was_exported(lib):
    header = open(os.path.join(ROOT, "include", "bt709hip_ext.h")).read()
    assert int(re.search(r"\bBT709HIP_OPT_CHROMA_LAYOUT\s*=\s*(\d+)", header).group(1)) == 11 == _capi.OPT_CHROMA_LAYOUT
    assert int(re.search(r"#define\s+BT709HIP_CHROMA_NV12\s+(\d+)", header).group(1)) == 0 == _capi.CHROMA_NV12
    assert int(re.search(r"#define\s+BT709HIP_CHROMA_I420\s+(\d+)", header).group(1)) == 1 == _capi.CHROMA_I420
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    assert "kChromaLayoutOption = BT709HIP_OPT_CHROMA_LAYOUT" in hpp
    assert "kChromaNV12 = BT709HIP_CHROMA_NV12, kChromaI420 = BT709HIP_CHROMA_I420" in hpp
    # the header states each thing the option does not cover
    comment = re.search(r"/\* BT709HIP_OPT_CHROMA_LAYOUT\..*?\*/", header, flags=re.S).group(0)
    for word in ("RGBA16F targets", "bt709hip_decode_half[_batch]", "bt709hip_decode_scaled[_batch]", "ring, ring set, pool, shard",
                 "bt709hip_unconvert", "YV12"):
        assert word in comment, word
    # no export, no ABI bump
    assert lib.bt709hip_abi_version() == 504 == _capi.ABI_VERSION
    assert int(re.search(r"#define\s+BT709HIP_VERSION\s+(\d+)", abi_headers.text()).group(1)) == 504
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103


def test_python_mirror_planar_buffer_shape():
    """CVPixelBuffer(planar=True) over borrowed planes: U at cbcr_ptr, V (H/2) pitches behind it, the default pitch W/2 rounded
    as the class rounds pitches."""
    b = mb.CVPixelBuffer(None, 70, 10, planes=(0x1000, 0x9000), planar=True)
    assert b.planar and b.chroma_layout == _capi.CHROMA_I420
    assert b.y_stride == 80 and b.cbcr_stride == 48
    assert b.planes() == [(0x1000, 80), (0x9000, 48), (0x9000 + 5 * 48, 48)]
    f = b.frame()
    assert (f.cbcr, f.cbcr_stride, f.width, f.height) == (0x9000, 48, 70, 10)
    n = mb.CVPixelBuffer(None, 70, 10, planes=(0x1000, 0x9000))
    assert not n.planar and n.chroma_layout == _capi.CHROMA_NV12 and n.cbcr_stride == 80
    assert n.planes() == [(0x1000, 80), (0x9000, 80)]


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_planar") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_set_device_count(1)
    return lib


class FakeRig:
    """A context, a decoder and `n` w x h frames carved evenly from one allocation, each Y then W x H/2 bytes of chroma -- an NV12
    plane, or U then V at pitch W/2 -- plus alpha planes and targets from two more."""

    def __init__(self, lib, has_alpha=0, w=64, h=16, n=4):
        self.lib, self.w, self.h, self.n, self.has_alpha = lib, w, h, n, has_alpha
        self.ctx, self.dec, self.stream = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0
        assert lib.bt709hip_decoder_create(self.ctx, 1 if has_alpha else 0, has_alpha, C.byref(self.dec)) == 0
        assert lib.bt709hip_stream_create(self.ctx, C.byref(self.stream)) == 0
        self.mem = []
        for nbytes in (n * w * h * 3 // 2, n * w * h * 3 // 2, n * w * h * 8):
            p = C.c_void_p()
            assert lib.bt709hip_malloc(self.ctx, nbytes, C.byref(p)) == 0
            self.mem.append(p.value)
        self.step = w * h * 3 // 2
        transfer = 2 if has_alpha else 1  # sRGB for the alpha decoder (its gamma is forced), ITU-R 709 for Apple
        self.transfer = transfer
        self.frames = self.frames_at(w)
        self.alphas = (_capi.Frame * n)(*[_capi.Frame(self.mem[1] + i * self.step, w, None, w, w, h, 1, 3) for i in range(n)]) if has_alpha else None

    def frames_at(self, cbcr_stride, step=None):
        step = step or self.step
        return (_capi.Frame * self.n)(*[_capi.Frame(self.mem[0] + i * step, self.w, self.mem[0] + i * step + self.w * self.h, cbcr_stride,
                                                    self.w, self.h, 1, self.transfer) for i in range(self.n)])

    def surfs(self, w=None, h=None, fmt=0):
        w, h = w or self.w, h or self.h
        px = 8 if fmt == _capi.FORMAT_RGBA16F else 4
        return (_capi.Surface * self.n)(*[_capi.Surface(self.mem[2] + i * self.w * self.h * 8, w * px, w, h, fmt, 0) for i in range(self.n)])

    def set_layout(self, value):
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


@pytest.fixture(params=[0, 1], ids=["opaque", "alpha"])
def fake_rig(fake, request):
    r = FakeRig(fake, has_alpha=request.param)
    yield r
    r.close()


def test_shim_validates_the_chroma_pitch_by_layout(fake, fake_rig):
    lib, r = fake, fake_rig
    s, w, h = r.surfs(), r.w, r.h
    tight, short, nv12 = r.frames_at(w // 2), r.frames_at(w // 2 - 1), r.frames_at(w)
    decode = lambda f: lib.bt709hip_decode(r.dec, f, r.alphas, s, w, h, None, 1)
    batch = lambda f: lib.bt709hip_decode_batch(r.dec, r.n, f, r.alphas, s, None, 1)
    mark = lib.fake_hip_log_size()
    # NV12 (the default): a chroma row is W bytes
    assert decode(tight) == _capi.ERR_STRIDE and batch(tight) == _capi.ERR_STRIDE
    assert decode(r.frames_at(w - 1)) == _capi.ERR_STRIDE
    assert r.kernels(mark) == []
    assert decode(nv12) == 0 and batch(nv12) == 0
    assert len(r.kernels(mark)) == 2
    # I420: W/2 bytes; a frame as wide-pitched as NV12's is a padded planar frame
    assert r.set_layout(I420) == 0
    mark = lib.fake_hip_log_size()
    assert decode(short) == _capi.ERR_STRIDE and batch(short) == _capi.ERR_STRIDE
    assert r.kernels(mark) == []
    assert decode(tight) == 0 and batch(tight) == 0 and decode(nv12) == 0
    assert len(r.kernels(mark)) == 3
    # the other checks are what they were: a NULL chroma pointer on a colour frame, odd sizes, a short luma pitch
    broken = r.frames_at(w // 2)
    broken[0].cbcr = None
    assert decode(broken) == _capi.ERR_INVALID_ARG
    broken = r.frames_at(w // 2)
    broken[0].y_stride = w - 1
    assert decode(broken) == _capi.ERR_STRIDE
    broken = r.frames_at(w // 2)
    broken[0].cbcr_stride = 1 << 32
    assert decode(broken) == _capi.ERR_STRIDE  # the 32-bit pitch limit, on the U plane's pitch
    broken = r.frames_at(w // 2)
    broken[2].cbcr_stride = w // 2 + 2
    assert batch(broken) == _capi.ERR_SIZE_MISMATCH  # one geometry per batch
    assert len(r.kernels(mark)) == 3
    assert r.set_layout(NV12) == 0


def test_shim_uniform_batch_rule_is_unchanged(fake, fake_rig):
    """Evenly spaced frames (V follows from cbcr) go out as one launch of any count's worth; frames that are not take the pointer
    table, 32 at most -- under either layout."""
    lib, r = fake, fake_rig
    w, h, n = r.w, r.h, 40
    # 40 frames over the rig's memory: the descriptors may overlap, a fake launch touches nothing
    step = 16
    def make(stride, count, uneven):
        bump = lambda i: 16 if uneven and i == count - 1 else 0
        return (_capi.Frame * count)(*[_capi.Frame(r.mem[0] + i * step + bump(i), w, r.mem[0] + i * step + bump(i) + w * h, stride, w, h, 1, r.transfer)
                                       for i in range(count)])
    surfs = (_capi.Surface * n)(*[_capi.Surface(r.mem[2] + i * step, w * 4, w, h, 0, 0) for i in range(n)])
    alphas = (_capi.Frame * n)(*[_capi.Frame(r.mem[1] + i * step, w, None, w, w, h, 1, 3) for i in range(n)]) if r.has_alpha else None
    for layout, stride in ((NV12, w), (I420, w // 2)):
        assert r.set_layout(layout) == 0
        mark = lib.fake_hip_log_size()
        assert lib.bt709hip_decode_batch(r.dec, n, make(stride, n, False), alphas, surfs, None, 1) == 0
        issued = r.kernels(mark)
        assert len(issued) == 1 and issued[0][2] == n
        assert lib.bt709hip_decode_batch(r.dec, n, make(stride, n, True), alphas, surfs, None, 1) == _capi.ERR_UNSUPPORTED  # more than 32 through the table
        assert lib.bt709hip_decode_batch(r.dec, 32, make(stride, 32, True), alphas, surfs, None, 1) == 0
        issued = r.kernels(mark)
        assert len(issued) == 2 and issued[1][2] == 32
    assert r.set_layout(NV12) == 0


def test_shim_refuses_the_other_paths_after_their_validation(fake, fake_rig):
    lib, r = fake, fake_rig
    planar, nv12 = r.frames_at(r.w // 2), r.frames
    s, f16, half, scaled = r.surfs(), r.surfs(fmt=_capi.FORMAT_RGBA16F), r.surfs(r.w // 2, r.h // 2), r.surfs(48, 10)
    assert r.set_layout(I420) == 0
    mark = lib.fake_hip_log_size()
    for frames in (planar, nv12):  # an NV12-shaped frame is a padded planar one: refused all the same
        assert lib.bt709hip_decode_batch(r.dec, r.n, frames, r.alphas, f16, None, 1) == _capi.ERR_UNSUPPORTED
        assert lib.bt709hip_decode(r.dec, frames, r.alphas, f16, r.w, r.h, None, 1) == _capi.ERR_UNSUPPORTED
        for entry, out in (("bt709hip_decode_half", half), ("bt709hip_decode_scaled", scaled)):
            assert getattr(lib, entry)(r.dec, frames, r.alphas, out, None, 1) == _capi.ERR_UNSUPPORTED
            assert getattr(lib, entry + "_batch")(r.dec, r.n, frames, r.alphas, out, None, 1) == _capi.ERR_UNSUPPORTED
    # the usual validation comes first, in the usual order
    assert lib.bt709hip_decode_half(r.dec, planar, r.alphas, scaled, None, 1) == _capi.ERR_SIZE_MISMATCH
    assert lib.bt709hip_decode_scaled(r.dec, r.frames_at(r.w // 2 - 1), r.alphas, scaled, None, 1) == _capi.ERR_STRIDE
    assert lib.bt709hip_decode_batch(r.dec, r.n, r.frames_at(r.w // 2 - 1), r.alphas, f16, None, 1) == _capi.ERR_STRIDE
    assert r.kernels(mark) == []  # nothing was launched
    assert lib.bt709hip_decode_batch(r.dec, r.n, planar, r.alphas, s, None, 1) == 0
    assert len(r.kernels(mark)) == 1
    # a coalescing decoder refuses at the call, not when the queue goes out
    assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COALESCE, 4) == 0
    assert lib.bt709hip_decode(r.dec, planar, r.alphas, f16, r.w, r.h, r.stream, 0) == _capi.ERR_UNSUPPORTED
    assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COALESCE, 0) == 0
    assert len(r.kernels(mark)) == 1
    # with the option off the same calls succeed
    assert r.set_layout(NV12) == 0
    mark = lib.fake_hip_log_size()
    assert lib.bt709hip_decode_batch(r.dec, r.n, nv12, r.alphas, f16, None, 1) == 0
    assert lib.bt709hip_decode_half_batch(r.dec, r.n, nv12, r.alphas, half, None, 1) == 0
    assert lib.bt709hip_decode_scaled_batch(r.dec, r.n, nv12, r.alphas, scaled, None, 1) == 0
    assert lib.bt709hip_decode_half(r.dec, nv12, r.alphas, half, None, 1) == 0
    assert lib.bt709hip_decode_scaled(r.dec, nv12, r.alphas, scaled, None, 1) == 0
    assert len(r.kernels(mark)) == 5


def test_shim_setting_the_option_never_touches_the_device_and_works_in_a_capture(fake, fake_rig):
    lib, r = fake, fake_rig
    s, g = r.surfs(), C.c_void_p()
    assert lib.bt709hip_decoder_setup(r.dec) == 0
    mark = lib.fake_hip_log_size()
    assert r.set_layout(I420) == 0 and r.set_layout(7) == _capi.ERR_INVALID_ARG and r.set_layout(NV12) == 0 and r.set_layout(I420) == 0
    assert lib.fake_hip_log_size() == mark
    planar = r.frames_at(r.w // 2)
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    assert lib.bt709hip_decode(r.dec, planar, r.alphas, s, r.w, r.h, r.stream, 0) == 0  # no table to prepare
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0
    assert r.kernels(mark) == []  # recorded, not run
    assert lib.bt709hip_graph_launch(r.ctx, g, r.stream) == 0 and lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    assert len(r.kernels(mark)) == 1
    assert lib.bt709hip_graph_destroy(r.ctx, g) == 0
    assert r.set_layout(NV12) == 0


def test_shim_issues_queued_frames_before_the_layout_changes(fake, fake_rig):
    """The layout is decoder state: frames a coalescing decoder has queued go out under the layout they were queued with, so a
    change issues them first -- and frames of two layouts never share a launch."""
    lib, r = fake, fake_rig
    s = r.surfs()
    one = lambda frames, i: lib.bt709hip_decode(r.dec, C.byref(frames[i]), C.byref(r.alphas[i]) if r.alphas else None, C.byref(s[i]), r.w, r.h, r.stream, 0)
    # an NV12-pitched frame is valid under both layouts: same geometry, so only the layout keeps the launches apart
    assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COALESCE, 4) == 0
    mark = lib.fake_hip_log_size()
    assert one(r.frames, 0) == 0
    assert r.kernels(mark) == []  # queued under NV12
    assert r.set_layout(I420) == 0
    assert lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    issued = r.kernels(mark)
    assert len(issued) == 1 and issued[0][2] == 1  # the queued frame went out first, alone
    assert one(r.frames, 1) == 0 and one(r.frames, 2) == 0  # queued under I420
    assert len(r.kernels(mark)) == 1
    assert r.set_layout(7) == _capi.ERR_INVALID_ARG  # a refused value changes nothing but leaves nothing queued behind it
    assert lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    issued = r.kernels(mark)
    assert len(issued) == 2 and issued[1][2] == 2
    assert one(r.frames, 3) == 0
    assert r.set_layout(NV12) == 0
    assert one(r.frames, 0) == 0
    assert lib.bt709hip_decoder_flush(r.dec, r.stream) == 0 and lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    issued = r.kernels(mark)
    assert [k[2] for k in issued] == [1, 2, 1, 1]  # I420's frame 3 and NV12's frame 0 in launches of their own
    assert lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_COALESCE, 0) == 0


def test_ring_and_pool_stay_nv12_whatever_the_option_holds(fake, fake_rig):
    """A ring's frames are its own NV12 planes: its launches pass the layout, so the decode (1:1, 2:1 and into RGBA16F -- all
    refused for the caller's frames under I420) still launches, and the option's value is what it was afterwards."""
    lib, r = fake, fake_rig
    assert r.set_layout(I420) == 0
    for half, fmt in ((0, _capi.FORMAT_BGRA8_SRGB), (1, _capi.FORMAT_BGRA8_SRGB), (0, _capi.FORMAT_RGBA16F)):
        ring, opt = C.c_void_p(), _capi.RingOptions(0, 0, 0, fmt, 0)
        assert lib.bt709hip_ring_create_ex(r.dec, 64, 16, 4, half, 1, C.byref(opt), C.byref(ring)) == 0
        f, a, o = _capi.Frame(), _capi.Frame(), _capi.Surface()
        assert lib.bt709hip_ring_frame(ring, 1, C.byref(f), C.byref(a), C.byref(o)) == 0
        assert f.cbcr_stride == 64 and f.cbcr == f.y + 64 * 16  # it keeps describing NV12 planes
        mark = lib.fake_hip_log_size()
        assert lib.bt709hip_ring_decode(ring, 0, 4, None, 1) == 0
        issued = r.kernels(mark)
        assert len(issued) == 1 and issued[0][2] == 4
        assert _get(lib, r.dec) == I420
        assert lib.bt709hip_ring_destroy(ring) == 0
    pool = C.c_void_p()
    assert lib.bt709hip_pool_create(r.dec, 64, 16, 2, C.byref(pool)) == 0
    slot, y, ys, c, cs = C.c_int(-1), C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
    assert lib.bt709hip_pool_acquire(pool, C.byref(slot), C.byref(y), C.byref(ys), C.byref(c), C.byref(cs)) == 0
    assert cs.value == 64  # an interleaved CbCr plane
    mark = lib.fake_hip_log_size()
    assert lib.bt709hip_pool_submit(pool, slot.value) == 0
    out, stride = C.c_void_p(), C.c_size_t()
    assert lib.bt709hip_pool_wait(pool, slot.value, C.byref(out), C.byref(stride)) == 0
    assert len(r.kernels(mark)) == 1 and _get(lib, r.dec) == I420
    assert lib.bt709hip_pool_destroy(pool) == 0
    assert r.set_layout(NV12) == 0


# ------------------------------------------------------------------ the generated code

# the kChromaI420 (= 1: the leading ILj1E) instantiations of the five 1:1 kernel shapes
I420_KERNELS = ["_ZN5bt70912decode_quadsILj1ELb%dELb%dELb%dEEEvNS_12DecodeParamsE" % t for t in ((1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 1, 0), (0, 0, 0))] + \
    ["_ZN5bt70916decode_quads_logILj1ELb%dEEEvNS_12DecodeParamsE" % nt for nt in (1, 0)] + \
    ["_ZN5bt70917decode_quads_overILj1ELi%dEEEvNS_12DecodeParamsE" % m for m in (1, 2)] + \
    ["_ZN5bt70913decode_blocksILj1ELb%dELb%dEEEvNS_12DecodeParamsE" % t for t in ((1, 1), (0, 1), (0, 0))] + \
    ["_ZN5bt70918decode_blocks_overILj1ELi%dEEEvNS_12DecodeParamsE" % m for m in (1, 2)]


def test_isa_of_the_planar_kernels():
    """The arithmetic is the NV12 kernels': the only fused multiply-adds are centre_norm's (bt709_device.h), nothing transcendental,
    nothing spilled.  The fast kernels' front end: per lane (two quads) four luma dwords and four 2-byte chroma loads -- two per
    plane -- issued with the tile's other loads before any table is staged; the streaming table kernel keeps the NV12 kernel's
    store shape (four 16-byte non-temporal stores, no wait on memory between the first and the last) and its register budget."""
    from metalbt709decoder_amd import build
    asm = open(build.emit_asm()).read()
    bodies = dict(re.findall(r"^(_ZN5bt709\d+decode_(?:quads|blocks)(?:_log|_over)?ILj1E\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M))
    assert len(I420_KERNELS) == 14 and sorted(bodies) == sorted(I420_KERNELS)
    for name, body in bodies.items():
        for line in re.findall(r"^\s*(v_(?:pk_)?(?:fma|fmac|fmamk|fmaak|mad|mac|madmk|madak)_(?:f32|f16|legacy|mix)\w*\s[^\n]*)", body, flags=re.M):
            assert re.match(r"v_fmamk_f32 v\d+, v\d+, 0x3b808081, v\d+|v_fmac_f32_e32 v\d+, 0x3b808081, v\d+", line.strip()), (name, line)
        assert not re.search(r"\bv_pk_(mul|add|fma)_f32|\bv_(log|exp)_f32|s_setreg", body), name
        assert "scratch_" not in body, name
        meta = re.search(r"\.name:\s+%s\b.*?\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), asm, flags=re.S)
        assert meta and int(meta.group(1)) == 0, name
        if "quads" not in name:
            assert "global_load_ushort" not in body and len(re.findall(r"global_load_ubyte\s", body)) >= 6, name  # byte loads: any alignment
            continue
        alpha = "quadsILj1ELb1E" in name or "_over" in name
        nt = r"[^\n]* nt\b" if ("_over" in name or re.search(r"quadsILj1ELb[01]ELb1E|quads_logILj1ELb1E", name)) else r"[^\n]*"
        if re.search(r"quadsILj1ELb0ELb0E|quads_logILj1ELb0E", name):
            assert " nt" not in body, name  # BT709HIP_OPT_NONTEMPORAL = 0: the default cache policy throughout
        assert len(re.findall(r"global_load_ushort " + nt, body)) == 4, name                     # 2 quads x (U, V)
        assert len(re.findall(r"global_load_dword " + nt, body)) == (8 if alpha else 4), name    # 2 quads x (2 luma rows [+ 2 alpha rows])
        assert body.count("global_store_dwordx4") == 4, name
        tile_loads = [m.start() for m in re.finditer(r"global_load_(?:ushort|dword) ", body)]
        if "ds_write" in body:
            assert max(tile_loads) < body.index("ds_write"), name  # the tile first, then the tables
        first, last = body.index("global_store_dwordx4"), body.rindex("global_store_dwordx4")
        assert "vmcnt" not in body[first:last], name
    stream = "_ZN5bt70912decode_quadsILj1ELb0ELb1ELb0EEEvNS_12DecodeParamsE"  # no alpha, streaming, table
    assert len(re.findall(r"global_store_dwordx4 [^\n]* nt\b", bodies[stream])) == 4
    assert bodies[stream].count("ds_read_b64") == 48  # 16 pixels x 3 channels
    meta = re.search(r"\.name:\s+%s\b.*?\.vgpr_count:\s+(\d+)" % re.escape(stream), asm, flags=re.S)
    assert meta and int(meta.group(1)) <= 64

