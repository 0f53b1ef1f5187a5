"""Planar CHW decode targets (BT709HIP_FORMAT_CHW_U8 / _F16 / _F32), the parts that need no GPU: the definition in
numpy (tests/chw_cases.py), the ids and the option domain on a context-less decoder, and -- on the shim built against the fake HIP
runtime -- validation, the other entry points' refusals, routing, batches, the coalescing queue and graph capture; the host replay
of csrc/bt709_chw_norm.h against the definition; the Python mirror; the generated code of the new kernels.

The fake runtime's launcher stands in for launch_decode, the one launcher a CHW decode goes through: it reports the NV12 BGRA8
kernel names ("decode_nv12_quads<nt>" fast, "decode_nv12_blocks" general) and one launch whatever the count, so what is asserted
here is the PATH and the plan handed to the launcher; the kernels' own names, the band map and the tail split of a long batch
are asserted on the GPU (tests/test_chw_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_headers
import chw_cases as cc
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, F16, F32 = _capi.FORMAT_CHW_U8, _capi.FORMAT_CHW_F16, _capi.FORMAT_CHW_F32
ELEM = {U8: 1, F16: 2, F32: 4}
NORM_OPTS = list(range(14, 20))
FAST, GENERAL = ("kernel:decode_nv12_quads<nt>", "kernel:decode_nv12_quads<alpha>"), ("kernel:decode_nv12_blocks",)


# ------------------------------------------------------------------ the definition

def test_definition_in_numpy():
    assert np.float32(255.0) * cc.INV255 == np.float32(1.0)
    scale, bias = cc.IMAGENET
    words = (np.arange(256, dtype=np.uint32) * 0x010101 | 0xFF000000).reshape(1, 256)
    for dtype in ("float16", "float32"):
        planes = cc.chw_of(words, dtype, scale, bias)
        assert planes.shape == (3, 1, 256) and planes.dtype == np.dtype(dtype)
        for c in range(3):
            assert np.isfinite(planes[c]).all() and np.unique(planes[c]).size == 256, (dtype, c)  # 256 distinct finite values per channel
    u8 = cc.chw_of(np.array([[0x80402010]], np.uint32), "uint8", planes=4)
    assert [int(v) for v in u8.reshape(-1)] == [0x40, 0x20, 0x10, 0x80]  # R, G, B, A
    a = cc.chw_of(np.array([[0xFF000000, 0x33000000]], np.uint32), "float32", scale, bias, planes=4)[3]
    assert a[0, 0] == np.float32(1.0) and a[0, 1] == np.float32(0x33) * cc.INV255  # the alpha plane: no scale, no bias
    assert cc.chw_of(np.array([[0x00FF0000]], np.uint32), "float16", (2.0 ** 17,) * 3, (0.0,) * 3)[0, 0, 0] == np.inf
    # every ImageNet channel has a code on which a contraction would show
    for c in range(3):
        assert cc.fma_differs(scale[c], bias[c]).size > 0, c


# ------------------------------------------------------------------ ids, ABI, option domain

@pytest.fixture(scope="module")
def lib():
    return mb.load_library()


def test_ids_agree_and_nothing_was_exported(lib):
    header = open(os.path.join(ROOT, "include", "bt709hip_ext.h")).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert (define("BT709HIP_FORMAT_CHW_U8"), define("BT709HIP_FORMAT_CHW_F16"), define("BT709HIP_FORMAT_CHW_F32")) == (4, 5, 6) == (U8, F16, F32)
    assert (mb.FORMAT_CHW_U8, mb.FORMAT_CHW_F16, mb.FORMAT_CHW_F32) == (4, 5, 6)
    for i, ch in enumerate("RGB"):
        assert define("BT709HIP_OPT_CHW_SCALE_" + ch) == 14 + i == getattr(_capi, "OPT_CHW_SCALE_" + ch)
        assert define("BT709HIP_OPT_CHW_BIAS_" + ch) == 17 + i == getattr(_capi, "OPT_CHW_BIAS_" + ch)
    hpp = open(os.path.join(ROOT, "host", "MetalBT709Decoder.hpp")).read()
    for word in ("BT709HIP_FORMAT_CHW_U8", "BT709HIP_FORMAT_CHW_F16", "BT709HIP_FORMAT_CHW_F32", "setCHWNormalisation"):
        assert word in hpp, word
    comment = re.search(r"/\* PLANAR CHW TARGETS\..*?\*/", header, flags=re.S).group(0)
    for word in ("caller's race", "BT709HIP_ERR_STRIDE", "never queued", "64-bit product", "2^-64"):
        assert word in comment, word
    # no export, no ABI bump, the base header at its cap
    assert lib.bt709hip_abi_version() == 504 == _capi.ABI_VERSION
    assert int(re.search(r"#define\s+BT709HIP_VERSION\s+(\d+)", abi_headers.text()).group(1)) == 504
    stripped = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", stripped))) == 103 == len(_capi.SYMBOLS)
    assert len(open(os.path.join(ROOT, "include", "bt709hip.h")).read().splitlines()) <= 250
    for f in os.listdir(os.path.join(ROOT, "metalbt709decoder_amd", "csrc")):
        assert len(open(os.path.join(ROOT, "metalbt709decoder_amd", "csrc", f)).read().splitlines()) <= 900, f


def _get(lib, dec, opt):
    v = C.c_int(-12345)
    assert lib.bt709hip_decoder_get_option(dec, opt, C.byref(v)) == _capi.OK
    return v.value


@pytest.mark.parametrize("has_alpha", [0, 1])
def test_option_domain_and_round_trip(lib, has_alpha):
    """A decoder without a context: the six options are plain properties holding float32 bit patterns."""
    dec = C.c_void_p()
    assert lib.bt709hip_decoder_create(None, mb.MetalBT709GammaApple, has_alpha, C.byref(dec)) == _capi.OK
    try:
        assert [_get(lib, dec, o) for o in NORM_OPTS] == [cc.bits(1.0)] * 3 + [cc.bits(0.0)] * 3  # the defaults
        sub = int(np.array([1], np.uint32).view(np.int32)[0])  # the smallest float32 subnormal
        bad = [cc.bits(np.nan), cc.bits(np.inf), cc.bits(-np.inf), cc.bits(2.0 ** -65), cc.bits(-2.0 ** -65), cc.bits(2.0 ** 65), cc.bits(-2.0 ** 65),
               sub, int(np.array([0x807FFFFF], np.uint32).view(np.int32)[0]), cc.bits(2.0 ** 64) + 1, cc.bits(2.0 ** -64) - 1]
        good = [cc.bits(-0.0), cc.bits(0.0), cc.bits(-2.5), cc.bits(2.0 ** 64), cc.bits(-2.0 ** 64), cc.bits(2.0 ** -64), cc.bits(-2.0 ** -64),
                cc.bits(1.0 / 0.229), cc.bits(-0.485 / 0.229)]
        for opt in NORM_OPTS:
            for held in good:
                assert lib.bt709hip_decoder_set_option(dec, opt, held) == _capi.OK, (opt, held)
                assert _get(lib, dec, opt) == held  # the bits round-trip, negative values and -0 too
                for b in bad:
                    assert lib.bt709hip_decoder_set_option(dec, opt, b) == _capi.ERR_INVALID_ARG, (opt, hex(b & 0xFFFFFFFF))
                    assert _get(lib, dec, opt) == held  # a refused value leaves the option as it was
        # one option does not move another
        for i, opt in enumerate(NORM_OPTS):
            assert lib.bt709hip_decoder_set_option(dec, opt, cc.bits(1.5 + i)) == _capi.OK
        assert [_get(lib, dec, o) for o in NORM_OPTS] == [cc.bits(1.5 + i) for i in range(6)]
        # the ids around them are what they were
        for unknown in (13, 20, 99):
            assert lib.bt709hip_decoder_set_option(dec, unknown, 0) == _capi.ERR_INVALID_ARG
            assert lib.bt709hip_decoder_get_option(dec, unknown, C.byref(C.c_int())) == _capi.ERR_INVALID_ARG
    finally:
        lib.bt709hip_decoder_destroy(dec)


# ------------------------------------------------------------------ the shim on the fake HIP runtime

class Addressing(C.Structure):  # fake_hip_addressing
    _fields_ = [("uniform", C.c_int32), ("frames", C.c_int32), ("steps", C.c_int64 * 6)]


@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_chw") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_allocations.restype = C.c_uint64
    lib.fake_hip_last_addressing.argtypes = [C.POINTER(Addressing)]
    lib.fake_hip_set_device_count(1)
    return lib


class Rig:
    """A context, a decoder, a stream and three allocations: frames (Y then CbCr, or U then V), alpha planes, targets.  The fake
    launches touch nothing, so descriptors may overlap and point anywhere inside them."""
    W, H = 64, 16

    def __init__(self, lib, has_alpha=0, gamma=0):
        self.lib, self.has_alpha = lib, has_alpha
        self.ctx, self.dec, self.stream = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0
        assert lib.bt709hip_decoder_create(self.ctx, 1 if has_alpha else gamma, has_alpha, C.byref(self.dec)) == 0
        assert lib.bt709hip_stream_create(self.ctx, C.byref(self.stream)) == 0
        self.mem = []
        for nbytes in (1 << 20, 1 << 20, 1 << 22):
            p = C.c_void_p()
            assert lib.bt709hip_malloc(self.ctx, nbytes, C.byref(p)) == 0
            self.mem.append(p.value)
        self.transfer = 2 if has_alpha or gamma == 1 else 1

    def frames(self, n=1, w=None, h=None, step=None, chroma_stride=None, base=0, uneven=False):
        w, h = w or self.W, h or self.H
        step = w * h * 3 // 2 if step is None else step
        at = lambda i: self.mem[0] + base + i * step + (16 if uneven and i == n - 1 else 0)
        return (_capi.Frame * n)(*[_capi.Frame(at(i), w, at(i) + w * h, chroma_stride or w, w, h, 1, self.transfer) for i in range(n)])

    def alphas(self, n=1, w=None, h=None, step=None):
        if not self.has_alpha:
            return None
        w, h = w or self.W, h or self.H
        step = w * h if step is None else step
        return (_capi.Frame * n)(*[_capi.Frame(self.mem[1] + i * step, w, None, w, w, h, 1, 3) for i in range(n)])

    def surfs(self, fmt, n=1, w=None, h=None, stride=None, base=0, step=None, reserved=0):
        w, h = w or self.W, h or self.H
        stride = w * ELEM.get(fmt, 8 if fmt == _capi.FORMAT_RGBA16F else 4) if stride is None else stride
        step = 4 * stride * h if step is None else step
        return (_capi.Surface * n)(*[_capi.Surface(self.mem[2] + (1 << 21) + base + i * step, stride, w, h, fmt, reserved) for i in range(n)])

    def decode(self, frames, surfs, alphas=None, stream=None, wait=1, w=None, h=None):
        return self.lib.bt709hip_decode(self.dec, frames, alphas if alphas is not None else self.alphas(w=w, h=h), surfs, w or self.W, h or self.H, stream, wait)

    def batch(self, n, frames, surfs, alphas=None, stream=None, wait=1):
        return self.lib.bt709hip_decode_batch(self.dec, n, frames, alphas if alphas is not None else self.alphas(n), surfs, stream, wait)

    def set(self, opt, value):
        return self.lib.bt709hip_decoder_set_option(self.dec, opt, value)

    def kernels(self, mark):
        from test_fake_hip import log
        return [o for o in log(self.lib, mark) if o[0].startswith("kernel:")]

    def launch(self):
        info = _capi.LaunchInfo()
        assert self.lib.bt709hip_last_launch_info(C.byref(info)) == 0
        return tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands

    def addressing(self):
        a = Addressing()
        assert self.lib.fake_hip_last_addressing(C.byref(a)) == 0
        return a.uniform, a.frames, list(a.steps)

    def close(self):
        lib = self.lib
        assert lib.bt709hip_decoder_destroy(self.dec) == 0
        for p in self.mem:
            assert lib.bt709hip_free(self.ctx, p) == 0
        assert lib.bt709hip_stream_destroy(self.ctx, self.stream) == 0 and lib.bt709hip_context_destroy(self.ctx) == 0


@pytest.fixture(params=[0, 1], ids=["opaque", "alpha"])
def rig(fake, request):
    r = Rig(fake, has_alpha=request.param)
    yield r
    r.close()


@pytest.mark.parametrize("fmt", [U8, F16, F32])
def test_shim_validates_pitch_alignment_and_limits(fake, rig, fmt):
    r, e, w, h = rig, ELEM[fmt], Rig.W, Rig.H
    f = r.frames()
    mark = fake.fake_hip_log_size()
    assert r.decode(f, r.surfs(fmt, stride=w * e - e)) == _capi.ERR_STRIDE          # a pitch below W e
    assert r.decode(f, r.surfs(fmt, stride=(1 << 32) + 4 * e)) == _capi.ERR_STRIDE  # a pitch the launch cannot carry in 32 bits
    if e > 1:
        assert r.decode(f, r.surfs(fmt, stride=w * e + 1)) == _capi.ERR_STRIDE      # a pitch that is no multiple of e
        assert r.decode(f, r.surfs(fmt, base=1)) == _capi.ERR_STRIDE                # a base that is not e-aligned
        assert r.batch(1, f, r.surfs(fmt, base=e // 2)) == _capi.ERR_STRIDE
    bgra = r.surfs(0)
    assert r.decode(f, r.surfs(fmt, reserved=1)) == r.decode(f, r.surfs(0, reserved=1)) == _capi.ERR_INVALID_ARG  # reserved != 0: what it was
    assert r.decode(f, r.surfs(fmt, w=w + 2)) == _capi.ERR_SIZE_MISMATCH
    # mixed formats in a batch
    for other in (0, 1) + tuple(o for o in (U8, F16, F32) if o != fmt):
        mixed = r.surfs(fmt, n=2, stride=w * 8)
        mixed[1].format = other
        assert r.batch(2, r.frames(2), mixed) == _capi.ERR_INVALID_ARG, other
        mixed[0].format, mixed[1].format = other, fmt
        assert r.batch(2, r.frames(2), mixed) == _capi.ERR_INVALID_ARG, other
    # 33 unevenly placed surfaces exceed the pointer table; 32 do not
    assert r.batch(33, r.frames(33, step=16, uneven=True), r.surfs(fmt, n=33, step=16 * e)) == _capi.ERR_UNSUPPORTED
    assert r.kernels(mark) == []
    assert r.batch(32, r.frames(32, step=16, uneven=True), r.surfs(fmt, n=32, step=16 * e)) == 0
    assert r.addressing()[:2] == (0, 32)
    # H/2 = 65536 is one row pair too many for the grid, as for every decode
    tall = 131072
    assert r.decode(r.frames(w=2, h=tall), r.surfs(fmt, w=2, h=tall), alphas=r.alphas(w=2, h=tall), w=2, h=tall) == _capi.ERR_UNSUPPORTED
    assert r.decode(r.frames(w=2, h=tall), r.surfs(0, w=2, h=tall), alphas=r.alphas(w=2, h=tall), w=2, h=tall) == _capi.ERR_UNSUPPORTED
    assert len(r.kernels(mark)) == 1
    assert r.decode(f, bgra) == 0 and r.decode(f, r.surfs(fmt)) == 0
    assert len(r.kernels(mark)) == 3


def test_every_other_entry_point_treats_chw_as_an_unknown_format(fake, rig):
    """Each call with format 4, 5 or 6 returns what the same call returns with the unassigned 7 -- and launches nothing."""
    lib, r, w, h = fake, rig, Rig.W, Rig.H
    f, a = r.frames(4), r.alphas(4)
    assert lib.bt709hip_decoder_setup(r.dec) == 0 and lib.bt709hip_render_scaled_prepare(r.ctx) == 0 and lib.bt709hip_encoder_prepare(r.ctx, 1, 0) == 0
    mark = fake.fake_hip_log_size()

    def calls(fmt):
        half, scaled, same = r.surfs(fmt, n=4, w=w // 2, h=h // 2), r.surfs(fmt, n=4, w=48, h=10), r.surfs(fmt, n=4)
        bgra, view = r.surfs(0, n=4), r.surfs(0, n=4, w=48, h=10, base=1 << 20)
        out = [lib.bt709hip_decode_half(r.dec, f, a, half, None, 1), lib.bt709hip_decode_half_batch(r.dec, 4, f, a, half, None, 1),
               lib.bt709hip_decode_scaled(r.dec, f, a, scaled, None, 1), lib.bt709hip_decode_scaled_batch(r.dec, 4, f, a, scaled, None, 1),
               lib.bt709hip_render_scaled(r.ctx, same, view, None, 1), lib.bt709hip_render_scaled(r.ctx, bgra, scaled, None, 1),
               lib.bt709hip_render_scaled_batch(r.ctx, 4, same, view, None, 1), lib.bt709hip_render_scaled_batch(r.ctx, 4, bgra, scaled, None, 1),
               lib.bt709hip_encode(r.ctx, same, f, 1, 0, None, 1), lib.bt709hip_encode_batch(r.ctx, 4, same, f, 1, 0, None, 1),
               lib.bt709hip_unconvert(r.dec, r.mem[0], w * 4, w, h, same, None, 1),
               lib.bt709hip_decoder_prepare_format(r.dec, fmt), lib.bt709hip_decoder_set_option(r.dec, _capi.OPT_SCALE_INTERMEDIATE, fmt)]
        for half_scale in (0, 1):
            ring, opt = C.c_void_p(), _capi.RingOptions(0, 0, 0, fmt, 0)
            out.append(lib.bt709hip_ring_create_ex(r.dec, w, h, 4, half_scale, 1, C.byref(opt), C.byref(ring)))
            assert ring.value is None
        for opt_id in (_capi.CTX_OPT_ENCODE_HALF_INPUT,):  # the encoder with its RGBA16F gate open
            assert lib.bt709hip_context_set_option(r.ctx, opt_id, 1) == 0
            out.append(lib.bt709hip_encode(r.ctx, same, f, 2, 0, None, 1))
            assert lib.bt709hip_context_set_option(r.ctx, opt_id, 0) == 0
        return out

    unknown = calls(7)
    assert all(rc != 0 for rc in unknown), unknown
    for fmt in (U8, F16, F32):
        assert calls(fmt) == unknown, fmt
    assert r.kernels(mark) == []
    assert _get(lib, r.dec, _capi.OPT_SCALE_INTERMEDIATE) == _capi.FORMAT_BGRA8_SRGB


def test_composite_over_and_unpremultiply_refuse_chw_before_anything_is_launched(fake):
    r = Rig(fake, has_alpha=1)
    try:
        f = r.frames(2)
        assert fake.bt709hip_decoder_setup(r.dec) == 0
        mark = fake.fake_hip_log_size()
        for opt, value, off in ((_capi.OPT_COMPOSITE_OVER, _capi.OVER_DESTINATION, _capi.OVER_OFF), (_capi.OPT_COMPOSITE_OVER, 0x102030, _capi.OVER_OFF),
                                (_capi.OPT_UNPREMULTIPLY, 1, 0)):
            assert r.set(opt, value) == 0
            for fmt in (U8, F16, F32):
                assert r.decode(f, r.surfs(fmt)) == _capi.ERR_UNSUPPORTED and r.batch(2, f, r.surfs(fmt, n=2)) == _capi.ERR_UNSUPPORTED
                # the order of checks is RGBA16F's: the usual validation first
                assert r.decode(f, r.surfs(fmt, stride=8)) == r.decode(f, r.surfs(1, stride=8)) == _capi.ERR_STRIDE
                assert r.set(_capi.OPT_COALESCE, 4) == 0
                assert r.decode(f, r.surfs(fmt), stream=r.stream, wait=0) == _capi.ERR_UNSUPPORTED
                assert r.set(_capi.OPT_COALESCE, 0) == 0
            assert r.decode(f, r.surfs(1)) == _capi.ERR_UNSUPPORTED
            assert r.set(opt, off) == 0
        assert r.kernels(mark) == [] and fake.fake_hip_log_size() == mark
        assert r.decode(f, r.surfs(U8)) == 0 and len(r.kernels(mark)) == 1
    finally:
        r.close()


@pytest.mark.parametrize("fmt", [U8, F16, F32])
def test_routing_fast_and_general(fake, rig, fmt):
    """The fast kernel at 4 e alignment and W % 4 == 0; the general one at W = 6, at a base off by e and at a pitch = e (mod 4 e) --
    under both chroma layouts; grid (tiles, H/2, frames) for the fast path."""
    r, e, w, h = rig, ELEM[fmt], Rig.W, Rig.H
    for layout, cstride in ((_capi.CHROMA_NV12, None), (_capi.CHROMA_I420, w // 2)):
        assert r.set(_capi.OPT_CHROMA_LAYOUT, layout) == 0
        cases = [("aligned", r.frames(chroma_stride=cstride), r.surfs(fmt), w, FAST),
                 ("padded by 4 e", r.frames(chroma_stride=cstride), r.surfs(fmt, stride=w * e + 4 * e), w, FAST),
                 ("base + e", r.frames(chroma_stride=cstride), r.surfs(fmt, base=e), w, GENERAL),
                 ("pitch = e mod 4 e", r.frames(chroma_stride=cstride), r.surfs(fmt, stride=w * e + e), w, GENERAL),
                 ("W = 6", r.frames(w=6, chroma_stride=3 if cstride else None), r.surfs(fmt, w=6, stride=32), 6, GENERAL)]
        if e > 1:
            cases.append(("base + 2 e", r.frames(chroma_stride=cstride), r.surfs(fmt, base=2 * e), w, GENERAL))
        for label, f, s, width, want in cases:
            mark = fake.fake_hip_log_size()
            assert r.decode(f, s, alphas=r.alphas(w=width), w=width) == 0, (label, layout)
            issued = r.kernels(mark)
            assert len(issued) == 1 and issued[0][0] in want and issued[0][3] == s[0].bgra, (label, layout, issued)
            grid, block, launches, bands = r.launch()
            if want is FAST:
                assert (grid, block[0], launches, bands) == ((1, h // 2, 1), 64, 1, 0), (label, grid, block)
    assert r.set(_capi.OPT_CHROMA_LAYOUT, _capi.CHROMA_NV12) == 0
    # a wide frame: two tiles of 512 lanes x 2 quads
    wide = 4 * 2 * 512 + 8
    mark = fake.fake_hip_log_size()
    assert r.decode(r.frames(w=wide, h=2), r.surfs(fmt, w=wide, h=2), alphas=r.alphas(w=wide, h=2), w=wide, h=2) == 0
    assert r.kernels(mark)[0][0] in FAST and r.launch()[0] == (2, 1, 1)


@pytest.mark.parametrize("fmt", [U8, F32])
def test_batches_take_the_existing_forms(fake, rig, fmt):
    """Up to 32 through the pointer table, any number evenly spaced through the signed 64-bit step; the band map from 64 evenly
    spaced frames on (the tail split of a count that is no multiple of 8 is the real launcher's: the GPU test sees it)."""
    r, e, w, h = rig, ELEM[fmt], 16, 4
    plane4 = 4 * w * e * h
    for n, uneven, step_out in ((2, False, plane4), (32, True, plane4), (33, False, plane4), (64, False, plane4), (72, False, plane4), (40, False, -plane4)):
        f = r.frames(n, w=w, h=h, uneven=uneven)
        s = r.surfs(fmt, n=n, w=w, h=h, step=step_out, base=0 if step_out > 0 else 100 * plane4)
        mark = fake.fake_hip_log_size()
        assert r.batch(n, f, s, alphas=r.alphas(n, w=w, h=h)) == 0, n
        issued = r.kernels(mark)
        assert len(issued) == 1 and issued[0][0] in FAST and issued[0][2] == n and issued[0][3] == s[0].bgra, (n, issued)
        uniform, frames, steps = r.addressing()
        assert (uniform, frames) == (0 if uneven else 1, n)
        if not uneven:
            assert steps[3] == step_out and steps[0] == w * h * 3 // 2
        grid, block, launches, bands = r.launch()
        assert grid == (1, h // 2, n) and bands == (1 if n in (64, 72) and n % 8 == 0 else 0), (n, grid, bands)


def test_graph_capture_records_and_replays_each_format(fake, rig):
    """Scale and bias travel as kernel arguments: nothing is staged, so a decode into each CHW format records inside a capture --
    no allocation, no copy -- and setting the options never touches the device."""
    lib, r = fake, rig
    assert lib.bt709hip_decoder_setup(r.dec) == 0
    mark, allocs = lib.fake_hip_log_size(), lib.fake_hip_allocations(0)
    for i, opt in enumerate(NORM_OPTS):
        assert r.set(opt, cc.bits(0.5 + i)) == 0
    assert lib.fake_hip_log_size() == mark
    g = C.c_void_p()
    f, a = r.frames(), r.alphas()
    assert lib.bt709hip_graph_begin_capture(r.ctx, r.stream) == 0
    targets = [r.surfs(fmt, base=i << 16) for i, fmt in enumerate((U8, F16, F32))]
    for s in targets:
        assert lib.bt709hip_decode(r.dec, f, a, s, Rig.W, Rig.H, r.stream, 0) == 0
    assert r.set(NORM_OPTS[0], cc.bits(3.0)) == 0  # works while the stream records
    assert lib.bt709hip_graph_end_capture(r.ctx, r.stream, C.byref(g)) == 0
    assert lib.fake_hip_log_size() == mark and lib.fake_hip_allocations(0) == allocs  # recorded, not run; nothing allocated or copied
    assert lib.bt709hip_graph_launch(r.ctx, g, r.stream) == 0 and lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0
    from test_fake_hip import log
    ops = log(lib, mark)
    assert [o[0].split(":")[0] for o in ops] == ["graph_launch", "kernel", "kernel", "kernel"] and [o[3] for o in ops[1:]] == [s[0].bgra for s in targets]
    assert lib.bt709hip_graph_destroy(r.ctx, g) == 0


def test_a_chw_call_on_a_coalescing_decoder_is_never_queued(fake, rig):
    """Decoder A coalesces and has a frame queued on S; a CHW decode on A and S issues the queued frame first, then launches
    on its own -- and is itself not queued."""
    lib, r = fake, rig
    assert r.set(_capi.OPT_COALESCE, 8) == 0
    f, a = r.frames(3), r.alphas(3)
    one = lambda i, s: lib.bt709hip_decode(r.dec, C.byref(f[i]), C.byref(a[i]) if a else None, s, Rig.W, Rig.H, r.stream, 0)
    for fmt in (U8, F16, F32):
        bgra, chw = r.surfs(0, base=0), r.surfs(fmt, base=1 << 18)
        mark = lib.fake_hip_log_size()
        assert one(0, bgra) == 0
        assert r.kernels(mark) == [] and lib.bt709hip_last_kernel_name() == b"(queued: coalescing submit)"
        assert one(1, chw) == 0
        issued = r.kernels(mark)
        assert [k[3] for k in issued] == [bgra[0].bgra, chw[0].bgra] and all(k[1] == r.stream.value and k[2] == 1 for k in issued), issued
        assert lib.bt709hip_last_kernel_name() != b"(queued: coalescing submit)"
        # nothing is left queued, and a BGRA8 call behind it queues again
        assert lib.bt709hip_stream_synchronize(r.ctx, r.stream) == 0 and len(r.kernels(mark)) == 2
        assert one(2, bgra) == 0 and len(r.kernels(mark)) == 2
        assert lib.bt709hip_decoder_flush(r.dec, r.stream) == 0 and len(r.kernels(mark)) == 3
        # a batch call with CHW targets: the same
        assert one(0, bgra) == 0
        assert lib.bt709hip_decode_batch(r.dec, 2, f, a, r.surfs(fmt, n=2, base=1 << 18), r.stream, 0) == 0
        issued = r.kernels(mark)
        assert len(issued) == 5 and issued[3][2] == 1 and issued[4][2] == 2
    assert r.set(_capi.OPT_COALESCE, 0) == 0


# ------------------------------------------------------------------ host replay of csrc/bt709_chw_norm.h

@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chw_norm") / "chw_norm_sweep")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "metalbt709decoder_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "chw_norm_sweep.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        out = subprocess.run([exe] + list(args), capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return [line.split() for line in out.stdout.strip().split("\n")]
    return run


def test_host_replay_of_the_normalisation(sweep):
    """Every code under every pair of chw_cases.NORM_PAIRS: the header's float32 bits and float16 bits are the definition's."""
    pairs = cc.NORM_PAIRS
    hexbits = lambda x: "%08x" % (cc.bits(x) & 0xFFFFFFFF)
    rows = sweep(*[hexbits(v) for p in pairs for v in p])
    assert len(rows) == 256 * len(pairs)
    code = np.arange(256)
    with np.errstate(over="ignore"):
        for i, (scale, bias) in enumerate(pairs):
            want32 = cc.norm(code, scale, bias)
            want16 = want32.astype(np.float16)
            got = rows[256 * i:256 * (i + 1)]
            assert [int(g[0]) for g in got] == [i] * 256 and [int(g[1]) for g in got] == list(range(256))
            assert [int(g[2], 16) for g in got] == [int(v) for v in want32.view(np.uint32)], (scale, bias)
            assert [int(g[3], 16) for g in got] == [int(v) for v in want16.view(np.uint16)], (scale, bias)
    # what the list must hold
    assert any(cc.fma_differs(s, b).size for s, b in pairs), "no pair on which a contraction would show"
    with np.errstate(over="ignore"):
        halves = {p: cc.norm(code, *p).astype(np.float16) for p in pairs}
    sub = halves[(2.0 ** -16, 0.0)].view(np.uint16)
    assert ((sub & 0x7C00) == 0).all() and np.unique(sub).size > 200                      # binary16 subnormals
    assert np.isinf(halves[(2.0 ** 17, 0.0)]).any() and np.isfinite(cc.norm(code, 2.0 ** 17, 0.0)).all()  # +inf in F16 alone
    assert any(s < 0 for s, _ in pairs) and any(np.signbit(np.float32(b)) and b == 0 for _, b in pairs)  # a negative scale, a -0 bias
    assert cc.norm(np.array([0]), 1.0, -0.0).view(np.uint32)[0] == 0                      # +0 + -0 = +0
    assert cc.norm(np.array([0]), -0.0, -0.0).view(np.uint32)[0] == 0x80000000            # -0 + -0 = -0
    # the alpha plane
    unit = sweep("unit")
    want = code.astype(np.float32) * cc.INV255
    assert [int(g[1], 16) for g in unit] == [int(v) for v in want.view(np.uint32)]
    assert [int(g[2], 16) for g in unit] == [int(v) for v in want.astype(np.float16).view(np.uint16)]


def test_host_replay_of_the_conversion_and_the_domain(sweep):
    """chw_half_bits on the host is round to nearest even for every class of float32 -- ties, subnormals, the overflow edge, the
    infinities, NaN -- and chw_norm_bits_valid is the domain the header states."""
    rng = np.random.default_rng(21)
    edge = np.array([0x00000000, 0x80000000, 0x33000000, 0x33000001, 0x337FFFFF, 0x33800000, 0x387FC000, 0x387FE000, 0x38800000, 0x477FE000, 0x477FEFFF,
                     0x477FF000, 0x47800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x3F801000, 0x3F803000, 0x3F801001, 0x00000001, 0x007FFFFF], np.uint32)
    exps = rng.integers(0x31, 0x49, 4000).astype(np.uint32) << np.uint32(23)
    rand = exps | rng.integers(0, 1 << 23, 4000).astype(np.uint32) | (rng.integers(0, 2, 4000).astype(np.uint32) << np.uint32(31))
    ties = (exps & np.uint32(0x7F800000)) | (rng.integers(0, 1 << 10, 4000).astype(np.uint32) << np.uint32(13)) | np.uint32(0x1000)
    values = np.concatenate([edge, rand, ties])
    rows = sweep("half", *["%08x" % v for v in values])
    with np.errstate(over="ignore"):
        want = values.view(np.float32).astype(np.float16).view(np.uint16)
    assert [int(g[1], 16) for g in rows] == [int(v) for v in want]
    nan = sweep("half", "7fc00000", "ffc00001")
    assert all((int(g[1], 16) & 0x7C00) == 0x7C00 and (int(g[1], 16) & 0x3FF) != 0 for g in nan)
    probe = {0x00000000: 1, 0x80000000: 1, 0x1F800000: 1, 0x1F7FFFFF: 0, 0x9F800000: 1, 0x5F800000: 1, 0x5F800001: 0, 0xDF800000: 1, 0xDF800001: 0,
             0x00000001: 0, 0x007FFFFF: 0, 0x7F800000: 0, 0xFF800000: 0, 0x7FC00000: 0, 0x3F800000: 1, 0xBF000000: 1}
    rows = sweep("valid", *["%08x" % v for v in probe])
    assert {int(g[0], 16): int(g[1]) for g in rows} == probe


# ------------------------------------------------------------------ the Python mirror

def test_python_mirror_on_the_fake_library(fake):
    ctx = mb.MetalRenderContext()
    h = C.c_void_p()
    assert fake.bt709hip_context_create(0, C.byref(h)) == 0
    ctx.lib, ctx.handle = fake, h.value
    try:
        for dtype, e in (("uint8", 1), ("float16", 2), ("float32", 4)):
            for planes in (3, 4):
                t = ctx.makeCHWTexture((70, 10), dtype, planes=planes)
                assert (t.stride, t.planeBytes, t.planes, t.itemsize, t.dtype) == (70 * e, 700 * e, planes, e, np.dtype(dtype))
                s = t.surface()
                assert (s.bgra, s.stride, s.width, s.height, s.format, s.reserved) == (t.ptr, 70 * e, 70, 10, cc.FORMATS[dtype], 0)
                assert t._buf.nbytes == planes * 700 * e
                got = ctx.getCHWTexturePixels(t)
                assert got.shape == (planes, 10, 70) and got.dtype == np.dtype(dtype) and not got.any()  # zeroed
                t._buf.free()
        t = mb.CHWTexture(None, 6, 4, np.float16, planes=4, stride=32, ptr=0x1000)  # borrowed memory, a padded pitch, a numpy dtype
        assert (t.stride, t.planeBytes, t.surface().format, t.surface().bgra) == (32, 128, _capi.FORMAT_CHW_F16, 0x1000)
        for bad in ("int8", "float64", np.uint16, "bfloat16"):
            with pytest.raises((ValueError, TypeError)):
                mb.CHWTexture(None, 6, 4, bad, ptr=0x1000)
        with pytest.raises(ValueError):
            mb.CHWTexture(None, 6, 4, "uint8", planes=2, ptr=0x1000)
        with pytest.raises(ValueError):
            mb.CHWTexture(None, 6, 4, "float32", stride=26, ptr=0x1000)
        # the setters: kept before setup, applied at once on a live decoder, refused outside the domain
        dec = mb.MetalBT709Decoder()
        assert dec.setCHWMeanStd(cc.IMAGENET_MEAN, cc.IMAGENET_STD)
        scale, bias = cc.IMAGENET
        want = [cc.bits(v) for v in scale + bias]
        assert [dec._options[o] for o in NORM_OPTS] == want
        one, mean, std = np.float32(1.0), np.float32(0.485), np.float32(0.229)
        assert dec._options[14] == cc.bits(one / std) and dec._options[17] == cc.bits(-mean / std)  # the documented float32 recipe
        with pytest.raises(ValueError):
            dec.setCHWNormalisation((1.0, np.inf, 1.0))
        with pytest.raises(ValueError):
            dec.setCHWNormalisation((1.0, 1.0, 1.0), (0.0, 2.0 ** 65, 0.0))
        with pytest.raises(ValueError):
            dec.setCHWMeanStd((0.5, 0.5, 0.5), (1.0, 0.0, 1.0))  # 1 / 0
        assert [dec._options[o] for o in NORM_OPTS] == want
        d = C.c_void_p()
        assert fake.bt709hip_decoder_create(ctx.handle, 0, 0, C.byref(d)) == 0
        dec.metalRenderContext, dec._handle = ctx, d.value
        assert dec.setCHWNormalisation((2.0, -3.0, 0.5), (-0.0, 0.25, 7.0))
        assert [_get(fake, d, o) for o in NORM_OPTS] == [cc.bits(v) for v in (2.0, -3.0, 0.5, -0.0, 0.25, 7.0)]
        dec._handle = None
        assert fake.bt709hip_decoder_destroy(d) == 0
    finally:
        ctx.handle = None
        assert fake.bt709hip_context_destroy(h) == 0


# ------------------------------------------------------------------ the generated code

def test_isa_of_the_chw_kernels():
    """The arithmetic is the 1:1 kernels': the only fused multiply-adds are centre_norm's (bt709_device.h) -- none on the
    normalisation -- nothing packed in float32, nothing spilled.  Fast kernels: per lane (two quads) one store per plane and row --
    4, 8 or 16 bytes -- streaming where the kernel streams, with no wait on memory between the first and the last; the float16
    kernels convert two values at a time."""
    from metalbt709decoder_amd import build
    asm = open(build.emit_asm()).read()
    bodies = dict(re.findall(r"^(_ZN5bt709\d+decode_(?:quads|blocks)_chw\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M))
    quads = {n: b for n, b in bodies.items() if "quads" in n}
    assert len(quads) == 2 * 3 * 7 and len(bodies) - len(quads) == 2 * 3
    store_of = {1: "global_store_dword", 2: "global_store_dwordx2", 3: "global_store_dwordx4"}
    for name, body in bodies.items():
        for line in re.findall(r"^\s*(v_(?:pk_)?(?:fma|fmac|fmamk|fmaak|mad|mac|madmk|madak)_(?:f32|f16|legacy|mix)\w*\s[^\n]*)", body, flags=re.M):
            assert re.match(r"v_fmamk_f32 v\d+, v\d+, 0x3b808081, v\d+|v_fmac_f32_e32 v\d+, 0x3b808081, v\d+", line.strip()), (name, line)
        assert not re.search(r"\bv_pk_(mul|add|fma)_f32|\bv_(log|exp)_f32|s_setreg|v_cvt_pkrtz", body), name
        assert "scratch_" not in body, name
        meta = re.search(r"\.name:\s+%s\b.*?\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), asm, flags=re.S)
        assert meta and int(meta.group(1)) == 0, name
        if name not in quads:
            continue
        layout, elem, alpha, nt = re.match(r"_ZN5bt70916decode_quads_chwILj(\d)ELj(\d)ELb(\d)ELb(\d)E", name).groups()
        planes = 4 if alpha == "1" else 3
        stores = re.findall(r"^\s*(global_store_\w+) ([^\n]*)", body, flags=re.M)
        assert [s[0] for s in stores] == [store_of[int(elem)]] * (2 * 2 * planes), (name, stores)
        assert all((" nt" in s[1]) == (nt == "1") for s in stores), name
        first, last = body.index("global_store_"), body.rindex("global_store_")
        assert "vmcnt" not in body[first:last], name
        assert len(re.findall(r"\bv_cvt_pk_f16_f32", body)) == (2 * 2 * planes * 2 if elem == "2" else 0), name
        meta = re.search(r"\.name:\s+%s\b.*?\.vgpr_count:\s+(\d+)" % re.escape(name), asm, flags=re.S)
        assert meta and int(meta.group(1)) <= 64, name  # 8 waves per SIMD, as the BGRA8 kernels


def test_from_tensor_reads_a_tensors_layout():
    """CHWTexture.fromTensor on a stand-in with a device tensor's attributes (no GPU here): a contiguous CHW tensor, one image of
    an NCHW batch and a row-padded view wrap without a copy; a wrong dtype, rank, channel count, device or stride is refused."""
    torch = pytest.importorskip("torch", reason="torch is not installed: CHWTexture.fromTensor has nothing to read")

    class Device:
        index = 0

    class Stub:
        is_cuda, device = True, Device()

        def __init__(self, dtype, shape, stride, ptr=0x7000, item=None):
            self.dtype, self.shape, self._stride, self._ptr = dtype, shape, stride, ptr
            self._item = item or torch.empty((), dtype=dtype).element_size()

        def dim(self):
            return len(self.shape)

        def stride(self):
            return self._stride

        def element_size(self):
            return self._item

        def data_ptr(self):
            return self._ptr

    ctx = mb.MetalRenderContext(0)
    t = mb.CHWTexture.fromTensor(ctx, Stub(torch.float16, (3, 4, 16), (64, 16, 1)))
    assert (t.ptr, t.width, t.height, t.planes, t.stride, t.dtype, t.surface().format) == (0x7000, 16, 4, 3, 32, np.dtype("float16"), _capi.FORMAT_CHW_F16)
    assert t._buf is None  # borrowed: nothing allocated, nothing to free
    t = mb.CHWTexture.fromTensor(ctx, Stub(torch.float32, (4, 4, 16), (80, 20, 1)))  # rows padded by 4 elements
    assert (t.stride, t.planes, t.planeBytes, t.surface().format) == (80, 4, 320, _capi.FORMAT_CHW_F32)
    assert mb.CHWTexture.fromTensor(ctx, Stub(torch.uint8, (3, 2, 6), (12, 6, 1))).surface().format == _capi.FORMAT_CHW_U8
    for bad in (Stub(torch.float64, (3, 4, 16), (64, 16, 1)), Stub(torch.int8, (3, 4, 16), (64, 16, 1)),
                Stub(torch.float16, (2, 3, 4, 16), (192, 64, 16, 1)),  # a whole batch: index it
                Stub(torch.float16, (2, 4, 16), (64, 16, 1)),          # two planes
                Stub(torch.float16, (3, 16, 4), (64, 1, 16)),          # W is not dense
                Stub(torch.float16, (3, 4, 16), (128, 16, 1)),         # planes further apart than H rows
                Stub(torch.float16, (3, 4, 16), (32, 8, 1))):          # rows that overlap
        with pytest.raises(ValueError):
            mb.CHWTexture.fromTensor(ctx, bad)
    cpu, other = Stub(torch.float16, (3, 4, 16), (64, 16, 1)), Stub(torch.float16, (3, 4, 16), (64, 16, 1))
    cpu.is_cuda = False
    other.device = type("D", (), {"index": 1})()
    for bad in (cpu, other):
        with pytest.raises(ValueError):
            mb.CHWTexture.fromTensor(ctx, bad)
