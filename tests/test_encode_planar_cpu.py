"""BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT (the encoder writing planar I420 frames), the parts that need no GPU: the
constants of the bindings, and -- on the shim built against the fake HIP runtime -- the option's domain, validation under either
layout, alpha frames, batches, a capture; then the generated code of the new kernels.  (The fake runtime's launcher reports the
NV12 kernel names whatever the layout: the names are the GPU tests' business.)"""
import ctypes as C
import os
import re

import pytest

import abi_headers
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT, NV12, I420 = 6, 0, 1  # stated here, not taken from the bindings
ALPHA = 3                  # BT709HIP_FORMAT_BGRA8_ALPHA
SRGB, APPLE, LIN = mb.MetalBT709GammaSRGB, mb.MetalBT709GammaApple, mb.MetalBT709GammaLinear
BAD_VALUES = (-1, 2, 7, 1 << 30, -(1 << 31))


def test_constants_agree_and_nothing_was_exported():
    header = open(os.path.join(ROOT, "include", "bt709hip_ext.h")).read()
    assert int(re.search(r"\bBT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT\s*=\s*(\d+)", header).group(1)) == OPT == _capi.CTX_OPT_ENCODE_CHROMA_LAYOUT
    assert int(re.search(r"#define\s+BT709HIP_CHROMA_NV12\s+(\d+)", header).group(1)) == NV12 == _capi.CHROMA_NV12
    assert int(re.search(r"#define\s+BT709HIP_CHROMA_I420\s+(\d+)", header).group(1)) == I420 == _capi.CHROMA_I420
    # the five options before it keep their values
    assert [int(v) for v in re.findall(r"\bBT709HIP_CTX_OPT_[A-Z_]+\s*=\s*(\d+)", header)] == [1, 2, 3, 4, 5, 6]
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    assert "kEncodeChromaLayoutOption = BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT" in hpp and "BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT = 6" in hpp
    # the header says that this option refuses where the others clamp, and no longer says the encoder has nothing to lay out
    comment = re.search(r"/\* BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT\..*?\*/", header, flags=re.S).group(0)
    for word in ("BT709HIP_ERR_INVALID_ARG", "this one does not", "cbcr_stride >= W/2", "(height/2) * cbcr_stride", "encode_bgra_i420_blocks",
                 "encode_alpha_y<i420>", "never touches the device"):
        assert word in comment, word
    assert "the encoder have no chroma plane" not in header
    # no export, no ABI bump
    assert _capi.ABI_VERSION == 504
    assert int(re.search(r"#define\s+BT709HIP_VERSION\s+(\d+)", abi_headers.text()).group(1)) == 504
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103


def test_python_mirror_planar_buffer_is_what_the_encoder_is_handed():
    """CVPixelBuffer(planar=True) over borrowed planes: the frame an encode call passes carries U and the planar pitch."""
    b = mb.CVPixelBuffer(None, 70, 10, planes=(0x1000, 0x9000), planar=True)
    f = b.frame()
    assert (f.y, f.y_stride, f.cbcr, f.cbcr_stride, f.width, f.height) == (0x1000, 80, 0x9000, 48, 70, 10)
    assert b.chroma_layout == _capi.CHROMA_I420 and b.v_ptr == 0x9000 + 5 * 48


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_encode_planar") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
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
    """A context and `n` w x h pictures / frames carved evenly from two allocations: each frame Y, then W x H/2 bytes of chroma
    -- an NV12 plane, or U then V at pitch W/2."""

    def __init__(self, lib, n=4, w=64, h=16):
        self.lib, self.n, self.w, self.h = lib, n, w, h
        self.ctx = C.c_void_p()
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0
        self.src, self.dst = C.c_void_p(), C.c_void_p()
        assert lib.bt709hip_malloc(self.ctx, n * w * h * 4, C.byref(self.src)) == 0
        assert lib.bt709hip_malloc(self.ctx, n * w * h * 3 // 2, C.byref(self.dst)) == 0

    def surfs(self, fmt=0, w=None, h=None):
        w, h = w or self.w, h or self.h
        return (_capi.Surface * self.n)(*[_capi.Surface(self.src.value + i * self.w * self.h * 4, w * 4, w, h, fmt, 0) for i in range(self.n)])

    def frames(self, cbcr_stride, cbcr=True, w=None, h=None):
        w, h = self.w if w is None else w, self.h if h is None else h
        out = []
        for i in range(self.n):
            base = self.dst.value + i * self.w * self.h * 3 // 2
            out.append(_capi.Frame(base, max(w, 1), base + self.w * self.h if cbcr else None, cbcr_stride, w, h, 0, 0))
        return (_capi.Frame * self.n)(*out)

    def set_layout(self, value):
        return self.lib.bt709hip_context_set_option(self.ctx, OPT, value)

    def kernels(self, mark):
        from test_fake_hip import log
        return [o for o in log(self.lib, mark) if o[0].startswith("kernel:")]

    def close(self):
        lib = self.lib
        assert lib.bt709hip_free(self.ctx, self.src) == 0 and lib.bt709hip_free(self.ctx, self.dst) == 0
        assert lib.bt709hip_context_destroy(self.ctx) == 0


@pytest.fixture()
def rig(fake):
    r = Rig(fake)
    yield r
    r.close()


def held_layout(rig):
    """There is no getter (no export was added): the held value shows in which chroma pitch the next encode accepts -- W/2 only
    under I420.  Nothing is launched by the probe that fails."""
    rc = rig.lib.bt709hip_encode(rig.ctx, rig.surfs(), rig.frames(rig.w // 2), SRGB, APPLE, None, 1)
    assert rc in (0, _capi.ERR_STRIDE)
    return I420 if rc == 0 else NV12


def test_option_domain(fake, rig):
    assert fake.bt709hip_context_set_option(None, OPT, I420) == _capi.ERR_INVALID_ARG
    assert held_layout(rig) == NV12  # the default
    for held in (I420, NV12, I420):
        assert rig.set_layout(held) == _capi.OK
        assert held_layout(rig) == held
        for bad in BAD_VALUES:
            assert rig.set_layout(bad) == _capi.ERR_INVALID_ARG, bad  # refused, not clamped ...
            assert held_layout(rig) == held                            # ... and the option is what it was
    # the clamping neighbours still clamp
    for opt in (_capi.CTX_OPT_ENCODE_ROW_PAIRS, _capi.CTX_OPT_ENCODE_THREADS, _capi.CTX_OPT_XCD_BANDS):
        assert fake.bt709hip_context_set_option(rig.ctx, opt, 1 << 30) == _capi.OK and fake.bt709hip_context_set_option(rig.ctx, opt, 0) == _capi.OK
    assert fake.bt709hip_context_set_option(rig.ctx, 7, 0) == _capi.ERR_INVALID_ARG


def test_pitch_validation_by_layout(fake, rig):
    lib, n, w = fake, rig.n, rig.w
    s = rig.surfs()
    one = lambda f: lib.bt709hip_encode(rig.ctx, s, f, SRGB, APPLE, None, 1)
    batch = lambda f: lib.bt709hip_encode_batch(rig.ctx, n, s, f, SRGB, APPLE, None, 1)
    mark = lib.fake_hip_log_size()
    # NV12 (the default): a chroma row is W bytes
    assert one(rig.frames(32)) == _capi.ERR_STRIDE and batch(rig.frames(32)) == _capi.ERR_STRIDE
    assert one(rig.frames(w - 1)) == _capi.ERR_STRIDE
    assert rig.kernels(mark) == []
    assert one(rig.frames(w)) == 0 and batch(rig.frames(w)) == 0
    assert len(rig.kernels(mark)) == 2
    # I420: W/2 bytes; a frame as wide-pitched as NV12's is a padded planar frame
    assert rig.set_layout(I420) == 0
    mark = lib.fake_hip_log_size()
    assert one(rig.frames(31)) == _capi.ERR_STRIDE and batch(rig.frames(31)) == _capi.ERR_STRIDE
    assert rig.kernels(mark) == []
    assert one(rig.frames(32)) == 0 and batch(rig.frames(32)) == 0 and one(rig.frames(w)) == 0
    issued = rig.kernels(mark)
    assert len(issued) == 3 and [k[2] for k in issued] == [1, n, 1]
    # the other checks and limits are what they were
    assert one(rig.frames(1 << 32)) == _capi.ERR_STRIDE  # the 32-bit pitch limit, on the U plane's pitch
    assert one(rig.frames(32, cbcr=False)) == _capi.ERR_INVALID_ARG  # a colour picture needs its chroma planes
    broken = rig.frames(32)
    broken[0].y_stride = w - 1
    assert one(broken) == _capi.ERR_STRIDE
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(w=62, h=15), rig.frames(32, w=62, h=15), SRGB, APPLE, None, 1) == _capi.ERR_ODD_DIMENSIONS
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(w=32), rig.frames(32), SRGB, APPLE, None, 1) == _capi.ERR_SIZE_MISMATCH
    assert lib.bt709hip_encode(rig.ctx, s, rig.frames(32), 3, APPLE, None, 1) == _capi.ERR_INVALID_ARG  # the gamma domain
    tall = 2 * 65536
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(h=tall), rig.frames(32, h=tall), SRGB, APPLE, None, 1) == _capi.ERR_UNSUPPORTED  # height / 2 <= 65535
    assert len(rig.kernels(mark)) == 3
    # zero-sized frames: OK, no launch -- whatever the pitch says
    for zw, zh in ((0, 16), (64, 0), (0, 0)):
        assert lib.bt709hip_encode_batch(rig.ctx, n, _zero_surfs(rig, zw, zh), rig.frames(0, w=zw, h=zh), SRGB, APPLE, None, 1) == 0, (zw, zh)
    assert lib.bt709hip_encode_batch(rig.ctx, 0, s, rig.frames(31), SRGB, APPLE, None, 1) == 0
    assert len(rig.kernels(mark)) == 3


def _zero_surfs(rig, w, h):
    return (_capi.Surface * rig.n)(*[_capi.Surface(rig.src.value, max(4 * w, 4), w, h, 0, 0) for _ in range(rig.n)])


def test_alpha_frames_under_both_layouts(fake, rig):
    lib, n, w = fake, rig.n, rig.w
    s = rig.surfs(ALPHA)
    for layout, pitch in ((NV12, w), (I420, w // 2)):
        assert rig.set_layout(layout) == 0
        mark = lib.fake_hip_log_size()
        assert lib.bt709hip_encode_batch(rig.ctx, n, s, rig.frames(pitch), LIN, LIN, None, 1) == 0          # no NULL
        assert lib.bt709hip_encode_batch(rig.ctx, n, s, rig.frames(0, cbcr=False), LIN, LIN, None, 1) == 0  # all NULL: the pitch is not looked at
        assert lib.bt709hip_encode(rig.ctx, s, rig.frames(5, cbcr=False), LIN, LIN, None, 1) == 0
        assert len(rig.kernels(mark)) == 3
        mixed = rig.frames(pitch)
        mixed[2].cbcr = None
        assert lib.bt709hip_encode_batch(rig.ctx, n, s, mixed, LIN, LIN, None, 1) == _capi.ERR_INVALID_ARG
        assert lib.bt709hip_encode_batch(rig.ctx, n, s, rig.frames(pitch - 1), LIN, LIN, None, 1) == _capi.ERR_STRIDE
        for gi, go in ((SRGB, APPLE), (LIN, SRGB), (SRGB, LIN)):
            assert lib.bt709hip_encode_batch(rig.ctx, n, s, rig.frames(pitch), gi, go, None, 1) == _capi.ERR_ALPHA_TRANSFER, (gi, go)
            assert lib.bt709hip_encode_batch(rig.ctx, n, s, rig.frames(0, cbcr=False), gi, go, None, 1) == _capi.ERR_ALPHA_TRANSFER, (gi, go)
        assert len(rig.kernels(mark)) == 3
    # under NV12 a planar pitch is short for an alpha frame with planes, too
    assert rig.set_layout(NV12) == 0
    assert lib.bt709hip_encode_batch(rig.ctx, n, s, rig.frames(w // 2), LIN, LIN, None, 1) == _capi.ERR_STRIDE


def test_batches_under_both_layouts(fake, rig):
    """Evenly spaced pictures (V follows from U) go out as one launch of any count's worth; pictures that are not take the
    pointer table, 32 at most -- under either layout."""
    lib, w, h, n = fake, rig.w, rig.h, 40
    step = 16  # the descriptors may overlap: a fake launch touches nothing

    def make(stride, count, uneven):
        bump = lambda i: 16 if uneven and i == count - 1 else 0
        return (_capi.Frame * count)(*[_capi.Frame(rig.dst.value + i * step + bump(i), w, rig.dst.value + i * step + bump(i) + w * h, stride, w, h, 0, 0)
                                       for i in range(count)])

    surfs = (_capi.Surface * n)(*[_capi.Surface(rig.src.value + i * step, w * 4, w, h, 0, 0) for i in range(n)])
    for layout, stride in ((NV12, w), (I420, w // 2)):
        assert rig.set_layout(layout) == 0
        mark = lib.fake_hip_log_size()
        assert lib.bt709hip_encode_batch(rig.ctx, n, surfs, make(stride, n, False), SRGB, APPLE, None, 1) == 0
        issued = rig.kernels(mark)
        assert len(issued) == 1 and issued[0][2] == n
        assert lib.bt709hip_encode_batch(rig.ctx, n, surfs, make(stride, n, True), SRGB, APPLE, None, 1) == _capi.ERR_UNSUPPORTED  # more than 32 through the table
        assert lib.bt709hip_encode_batch(rig.ctx, 32, surfs, make(stride, 32, True), SRGB, APPLE, None, 1) == 0
        issued = rig.kernels(mark)
        assert len(issued) == 2 and issued[1][2] == 32
        differing = make(stride, 4, False)
        differing[2].cbcr_stride = stride + 2
        assert lib.bt709hip_encode_batch(rig.ctx, 4, surfs, differing, SRGB, APPLE, None, 1) == _capi.ERR_SIZE_MISMATCH  # one geometry per batch
        assert len(rig.kernels(mark)) == 2
    # the plan on record is the NV12 encoder's for the same size and count
    info = _capi.LaunchInfo()
    plans = []
    for layout, stride in ((NV12, w), (I420, w // 2)):
        assert rig.set_layout(layout) == 0
        assert lib.bt709hip_encode_batch(rig.ctx, 4, surfs, make(stride, 4, False), SRGB, APPLE, None, 1) == 0
        assert lib.bt709hip_last_launch_info(C.byref(info)) == 0
        plans.append((tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands))
    assert plans[0] == plans[1] == ((1, 3, 4), (64, 1, 1), 1, 0)


def test_setting_the_option_never_touches_the_device_and_works_in_a_capture(fake, rig):
    lib = fake
    assert lib.bt709hip_encoder_prepare(rig.ctx, SRGB, APPLE) == 0
    S, g = C.c_void_p(), C.c_void_p()
    assert lib.bt709hip_stream_create(rig.ctx, C.byref(S)) == 0
    mark = lib.fake_hip_log_size()
    assert rig.set_layout(I420) == 0 and rig.set_layout(7) == _capi.ERR_INVALID_ARG and rig.set_layout(NV12) == 0
    assert lib.fake_hip_log_size() == mark
    assert lib.bt709hip_graph_begin_capture(rig.ctx, S) == 0
    assert rig.set_layout(I420) == 0  # while the stream is being captured
    assert lib.fake_hip_log_size() == mark
    assert lib.bt709hip_encode_batch(rig.ctx, rig.n, rig.surfs(), rig.frames(rig.w // 2), SRGB, APPLE, S, 0) == 0  # no table to prepare for the layout
    assert lib.bt709hip_graph_end_capture(rig.ctx, S, C.byref(g)) == 0
    assert rig.kernels(mark) == []  # recorded, not run
    assert lib.bt709hip_graph_launch(rig.ctx, g, S) == 0 and lib.bt709hip_stream_synchronize(rig.ctx, S) == 0
    issued = rig.kernels(mark)
    assert len(issued) == 1 and issued[0][0].startswith("kernel:encode") and issued[0][2] == rig.n
    assert lib.bt709hip_graph_destroy(rig.ctx, g) == 0 and lib.bt709hip_stream_destroy(rig.ctx, S) == 0


# ------------------------------------------------------------------ the generated code

def kernel(asm, name, layout):
    """-> (instruction lines of the kernel template's instantiation for `layout` (0: NV12, 1: I420), its metadata block)."""
    sym = "_ZN5bt709%d%sILj%dEEEvNS_12EncodeParamsE" % (len(name), name, layout)
    assert len(re.findall(r"^%s:" % sym, asm, re.M)) == 1, sym
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % sym, asm, re.S | re.M)
    assert m, "%s is not in the generated code" % name
    lines = [l.split(";")[0].strip() for l in m.group(1).split("\n")]
    meta = re.search(r"\.name:\s+%s\b.*?(?=\n  - \.a|\Z)" % re.escape(sym), asm, flags=re.S)
    assert meta, name
    return [l for l in lines if l and not l.startswith(".") and not l.endswith(":")], meta.group(0)


def meta_int(meta, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def waves_per_simd(vgprs):
    """gfx950: 512 VGPRs per lane of a SIMD, handed out in blocks of 8, eight waves at the most."""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def test_isa_of_the_planar_encoder_kernels():
    """No scratch; the twelve conversions of the fast kernel between the two rounding-mode writes; every store of the fast kernels
    non-temporal; per row pair two dword luma stores and two 2-byte chroma stores (the shipped design: the low half of the packed
    word to U, the high half to V); the general kernels store bytes only; and the fast kernel costs no occupancy against the NV12
    fast kernel of the same file."""
    from metalbt709decoder_amd import build
    asm = open(build.emit_asm()).read()
    names = {"encode_bgra_i420": "encode_bgra", "encode_bgra_i420_blocks": "encode_bgra_blocks", "encode_alpha_y_i420": "encode_alpha_y",
             "encode_alpha_y_blocks_i420": "encode_alpha_y_blocks"}  # what the kernel is called: the template it instantiates for I420
    code = {n: kernel(asm, template, 1) for n, template in names.items()}
    for n, (ins, meta) in code.items():
        assert not [i for i in ins if i.startswith("scratch_")], n
        assert meta_int(meta, "private_segment_fixed_size") == 0, n
    # the fast colour kernel
    ins, meta = code["encode_bgra_i420"]
    ops = [i.split()[0] for i in ins]
    setreg = [k for k, o in enumerate(ops) if o.startswith("s_setreg")]
    cvt = [k for k, o in enumerate(ops) if o == "v_cvt_pk_u8_f32"]
    assert len(setreg) == 2 and len(cvt) == 12 and setreg[0] < min(cvt) and max(cvt) < setreg[1]
    assert cvt == list(range(setreg[0] + 1, setreg[1])), "something sits between the conversions and the mode switch around them"
    stores = [i for i in ins if i.startswith("global_store")]
    assert all(re.search(r"\bnt\b", s) for s in stores), stores
    assert sorted(s.split()[0] for s in stores) == ["global_store_dword", "global_store_dword", "global_store_short", "global_store_short_d16_hi"], stores
    nv12_ops = [i.split()[0] for i in kernel(asm, "encode_bgra", 0)[0]]
    for op in ("global_load_dwordx4", "ds_read_b64", "v_lshlrev_b32_sdwa"):  # the NV12 kernel's front end, staging and arithmetic
        assert ops.count(op) == nv12_ops.count(op) > 0, op
    # the fast alpha kernel: two dwords of luma, 0x8080 to each plane
    ins, _ = code["encode_alpha_y_i420"]
    stores = [i for i in ins if i.startswith("global_store")]
    assert all(re.search(r"\bnt\b", s) for s in stores), stores
    assert sorted(s.split()[0] for s in stores) == ["global_store_dword", "global_store_dword", "global_store_short", "global_store_short"], stores
    assert not [i for i in ins if i.startswith("s_setreg")]
    # the general kernels: bytes, whatever the alignment
    for n in ("encode_bgra_i420_blocks", "encode_alpha_y_blocks_i420"):
        stores = [i.split()[0] for i in code[n][0] if i.startswith(("global_store", "flat_store", "buffer_store"))]
        assert len(stores) == 6 and set(stores) <= {"global_store_byte", "global_store_byte_d16_hi"}, (n, stores)
    ops = [i.split()[0] for i in code["encode_bgra_i420_blocks"][0]]
    setreg = [k for k, o in enumerate(ops) if o.startswith("s_setreg")]
    assert len(setreg) == 2 and [k for k, o in enumerate(ops) if o == "v_cvt_pk_u8_f32"] == list(range(setreg[0] + 1, setreg[1]))
    # occupancy: not above the VGPR count at which the NV12 fast kernel's waves per SIMD would drop
    nv12 = meta_int(kernel(asm, "encode_bgra", 0)[1], "vgpr_count")
    i420 = meta_int(code["encode_bgra_i420"][1], "vgpr_count")
    assert waves_per_simd(i420) >= waves_per_simd(nv12), (i420, nv12)
