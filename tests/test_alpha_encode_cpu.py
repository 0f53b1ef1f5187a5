"""CPU tests of the alpha-frame encoder (BT709HIP_FORMAT_BGRA8_ALPHA input of bt709hip_encode[_batch]): no GPU needed.

The reference encodes an alpha clip (srgb_to_bt709 -alpha, srgb_to_bt709/srgb_to_bt709.m:842-954) by copying each pixel's A
over R, G and B, forcing the gamma to linear and running the ordinary encoder.  For such a grey picture the result is a
256-entry byte table T for Y and 128 for every Cb, Cr -- exact, nothing here is a tolerance:

  * the oracle's T (and the reference's own, where it has been built) equals tests/golden/alpha_luma.json, with the facts
    DESIGN.md 3.4 states about it;
  * the product's host-built T (csrc/bt709_alpha_luma.h, the text shim_convert.cpp compiles) equals the golden, compiled
    natively with g++;
  * the shim's validation of the new format on the fake HIP runtime, and that no OTHER entry point's answer moved;
  * the generated code of the two alpha kernels.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle_lib import GAMMA_LINEAR, GAMMA_SRGB
from test_fake_hip import SHIM_SOURCES, FakeOp, build, log

from metalbt709decoder_amd import _capi
from metalbt709decoder_amd import build as product_build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "metalbt709decoder_amd", "csrc")
LIN = GAMMA_LINEAR
ALPHA = 3  # BT709HIP_FORMAT_BGRA8_ALPHA, stated here and not taken from the bindings
UNKNOWN = 7


@pytest.fixture(scope="module")
def golden():
    doc = json.load(open(os.path.join(HERE, "golden", "alpha_luma.json")))
    assert len(doc["luma"]) == 256 and doc["cbcr"] == 128
    return doc["luma"]


def grey_block(a):
    return [a, a, a] * 4


def test_bindings_carry_the_new_value():
    import metalbt709decoder_amd as mb
    assert _capi.FORMAT_BGRA8_ALPHA == ALPHA == mb.FORMAT_BGRA8_ALPHA and _capi.ABI_VERSION == 504
    hdr = open(os.path.join(ROOT, "include", "bt709hip.h")).read()
    assert re.search(r"BT709HIP_FORMAT_BGRA8_ALPHA\s*=\s*3\b", hdr) and re.search(r"#define BT709HIP_VERSION 504\b", hdr)
    assert not re.search(r"BT709HIP_FORMAT_\w+\s*=\s*2\b", hdr) and "2 is unassigned" in hdr


def test_alpha_luma_table_of_the_oracle_and_the_reference_is_the_golden(oracle, reference, golden):
    T = []
    for a in range(256):
        out = oracle.subsample_block(grey_block(a), LIN, LIN)
        assert out[0] == out[1] == out[2] == out[3] and out[4:] == (128, 128), (a, out)
        if reference is not None:
            assert tuple(reference.subsample_block(grey_block(a), LIN, LIN)) == tuple(out), a
        T.append(out[0])
    assert T == golden
    assert all(x <= y for x, y in zip(T, T[1:])) and len(set(T)) == 220
    assert T[:5] == [16, 17, 18, 19, 19] and T[251:] == [232, 232, 233, 234, 235]
    back = [oracle.decode_alpha(t) for t in T]
    assert sum(1 for a in range(256) if back[a] == a) == 220 and max(abs(back[a] - a) for a in range(256)) == 1


def test_mixed_grey_blocks_are_the_table_per_pixel(oracle, golden):
    """20 000 seeded 2x2 blocks of four different greys: Y[i] = T[A_i], (Cb, Cr) = (128, 128).  And for EVERY block: the
    averaged byte the chroma matrix is fed is a grey byte, and every grey byte gives (128, 128) (the flat blocks above)."""
    rng = np.random.default_rng(709003)
    blocks = rng.integers(0, 256, (20000, 4))
    for a4 in blocks.tolist():
        rgb = [c for a in a4 for c in (a, a, a)]
        out = oracle.subsample_block(rgb, LIN, LIN)
        assert list(out[:4]) == [golden[a] for a in a4] and out[4:] == (128, 128), (a4, out)
    for a4 in blocks[:2000].tolist() + [[0, 0, 0, 255], [255, 255, 255, 0], [1, 0, 0, 0]]:
        avg = oracle.average_bytes([c for a in a4 for c in (a, a, a)], LIN, LIN)
        assert avg[0] == avg[1] == avg[2], (a4, avg)


def test_host_built_table_equals_the_golden(tmp_path, golden):
    """csrc/bt709_alpha_luma.h + transfer_tables.cpp, plain g++: the table the shim uploads, all 256 entries."""
    out = str(tmp_path / "libalpha_luma_table.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC,
           os.path.join(HERE, "native", "alpha_luma_table.cpp"), os.path.join(CSRC, "transfer_tables.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(out)
    T = (C.c_uint8 * 256)()
    assert lib.alpha_luma_table(T) == 0
    assert list(T) == golden


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    so = build(str(tmp_path_factory.mktemp("fake_alpha") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.bt709hip_abi_version() == 504
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_set_device_count(2)
    return lib


class Rig:
    """A context and `n` 64 x 16 pictures / frames carved evenly from two allocations."""

    def __init__(self, lib, n=4, w=64, h=16):
        self.lib, self.n, self.w, self.h = lib, n, w, h
        self.ctx = C.c_void_p()
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0
        self.src, self.dst = C.c_void_p(), C.c_void_p()
        assert lib.bt709hip_malloc(self.ctx, n * w * h * 4, C.byref(self.src)) == 0
        assert lib.bt709hip_malloc(self.ctx, n * w * h * 3 // 2, C.byref(self.dst)) == 0

    def surfs(self, fmt=ALPHA, w=None, h=None, formats=None):
        w, h = w or self.w, h or self.h
        formats = formats or [fmt] * self.n
        return (_capi.Surface * self.n)(*[_capi.Surface(self.src.value + i * self.w * self.h * 4, w * 4, w, h, formats[i], 0) for i in range(self.n)])

    def frames(self, cbcr=True, w=None, h=None, null_at=()):
        w, h = w or self.w, h or self.h
        out = []
        for i in range(self.n):
            base = self.dst.value + i * self.w * self.h * 3 // 2
            has = cbcr and i not in null_at
            out.append(_capi.Frame(base, w, base + w * h if has else None, w if has else 0, w, h, 0, 0))
        return (_capi.Frame * self.n)(*out)

    def close(self):
        lib = self.lib
        assert lib.bt709hip_free(self.ctx, self.src) == 0 and lib.bt709hip_free(self.ctx, self.dst) == 0
        assert lib.bt709hip_context_destroy(self.ctx) == 0


@pytest.fixture()
def rig(fake):
    r = Rig(fake)
    yield r
    r.close()


def test_alpha_format_encodes_and_leaves_the_encoders_plan_on_record(fake, rig):
    lib, n = fake, rig.n
    info = _capi.LaunchInfo()
    mark = lib.fake_hip_log_size()
    assert lib.bt709hip_encode_batch(rig.ctx, n, rig.surfs(), rig.frames(), LIN, LIN, None, 1) == 0
    kernels = [o for o in log(lib, mark) if o[0].startswith("kernel:")]
    assert len(kernels) == 1 and kernels[0][2] == n and kernels[0][3] == rig.dst.value
    assert lib.bt709hip_last_launch_info(C.byref(info)) == 0
    # 16 quads -> one tile of one wave; 8 row pairs in groups of 3; n pictures; one launch, plain map: the colour encoder's plan
    assert (tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands) == ((1, 3, n), (64, 1, 1), 1, 0)
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(), rig.frames(), LIN, LIN, None, 1) == 0
    assert lib.bt709hip_last_launch_info(C.byref(info)) == 0 and (tuple(info.grid), info.launches) == ((1, 3, 1), 1)


def test_null_cbcr_is_for_alpha_frames_only(fake, rig):
    lib, n = fake, rig.n
    assert lib.bt709hip_encode_batch(rig.ctx, n, rig.surfs(), rig.frames(cbcr=False), LIN, LIN, None, 1) == 0
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(), rig.frames(cbcr=False), LIN, LIN, None, 1) == 0
    assert lib.bt709hip_encode_batch(rig.ctx, n, rig.surfs(0), rig.frames(cbcr=False), LIN, LIN, None, 1) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(0), rig.frames(cbcr=False), GAMMA_SRGB, 0, None, 1) == _capi.ERR_INVALID_ARG
    # all frames of a batch agree on NULL or non-NULL
    for null_at in ((0,), (2,), (0, 1, 2)):
        assert lib.bt709hip_encode_batch(rig.ctx, n, rig.surfs(), rig.frames(null_at=null_at), LIN, LIN, None, 1) == _capi.ERR_INVALID_ARG, null_at


def test_alpha_gammas_formats_and_sizes(fake, rig):
    lib, n = fake, rig.n
    s, f = rig.surfs(), rig.frames()
    for gi, go in ((GAMMA_SRGB, GAMMA_SRGB), (LIN, GAMMA_SRGB), (GAMMA_SRGB, LIN), (0, 0), (LIN, 0)):
        assert lib.bt709hip_encode_batch(rig.ctx, n, s, f, gi, go, None, 1) == _capi.ERR_ALPHA_TRANSFER, (gi, go)
        assert lib.bt709hip_encode(rig.ctx, s, f, gi, go, None, 1) == _capi.ERR_ALPHA_TRANSFER, (gi, go)
    for gi, go in ((3, LIN), (LIN, 3), (-1, LIN)):  # the range check comes first
        assert lib.bt709hip_encode_batch(rig.ctx, n, s, f, gi, go, None, 1) == _capi.ERR_INVALID_ARG, (gi, go)
    # differing formats in one batch, either way round
    for formats in ([ALPHA, 0, ALPHA, ALPHA], [0, ALPHA, 0, 0], [ALPHA, ALPHA, ALPHA, 0]):
        assert lib.bt709hip_encode_batch(rig.ctx, n, rig.surfs(formats=formats), f, LIN, LIN, None, 1) == _capi.ERR_SIZE_MISMATCH, formats
    # a format nobody knows stays what it was, alone or in a batch; so does the unassigned 2, and a set `reserved`
    for formats in ([UNKNOWN] * 4, [ALPHA, UNKNOWN, ALPHA, ALPHA], [2] * 4, [1] * 4):
        assert lib.bt709hip_encode_batch(rig.ctx, n, rig.surfs(formats=formats), f, LIN, LIN, None, 1) == _capi.ERR_UNSUPPORTED, formats
    r = rig.surfs()
    r[0].reserved = 1
    assert lib.bt709hip_encode(rig.ctx, r, f, LIN, LIN, None, 1) == _capi.ERR_UNSUPPORTED
    for w, h in ((63, 16), (64, 15), (63, 15)):
        assert lib.bt709hip_encode_batch(rig.ctx, n, rig.surfs(w=w, h=h), rig.frames(w=w, h=h), LIN, LIN, None, 1) == _capi.ERR_ODD_DIMENSIONS
    assert lib.bt709hip_encode(rig.ctx, rig.surfs(w=32), rig.frames(), LIN, LIN, None, 1) == _capi.ERR_SIZE_MISMATCH
    # strides as the colour encoder's; cbcr_stride is looked at only when there is a plane
    short = rig.frames()
    short[0].cbcr_stride = rig.w - 2
    assert lib.bt709hip_encode(rig.ctx, s, short, LIN, LIN, None, 1) == _capi.ERR_STRIDE
    short = rig.frames(cbcr=False)
    short[0].cbcr_stride = 5
    assert lib.bt709hip_encode(rig.ctx, s, short, LIN, LIN, None, 1) == 0
    assert lib.bt709hip_encode_batch(rig.ctx, 0, s, f, LIN, LIN, None, 1) == 0


def test_encoder_prepare_builds_the_alpha_table_for_a_capture(fake):
    lib = fake
    for prepared in (False, True):
        rig = Rig(lib)
        if prepared:
            assert lib.bt709hip_encoder_prepare(rig.ctx, LIN, LIN) == 0
        S, g = C.c_void_p(), C.c_void_p()
        assert lib.bt709hip_stream_create(rig.ctx, C.byref(S)) == 0
        assert lib.bt709hip_graph_begin_capture(rig.ctx, S) == 0
        mark = lib.fake_hip_log_size()
        rc = lib.bt709hip_encode_batch(rig.ctx, rig.n, rig.surfs(), rig.frames(cbcr=False), LIN, LIN, S, 0)
        assert rc == (0 if prepared else _capi.ERR_NOT_SETUP)
        assert lib.bt709hip_graph_end_capture(rig.ctx, S, C.byref(g)) == 0
        assert log(lib, mark) == []  # nothing ran: it is in the graph
        if prepared:
            assert lib.bt709hip_graph_launch(rig.ctx, g, S) == 0 and lib.bt709hip_stream_synchronize(rig.ctx, S) == 0
            ops = [o[0] for o in log(lib, mark) if o[1] == S.value]
            assert ops[0] == "graph_launch" and sum(o.startswith("kernel:encode") for o in ops) == 1, ops
        assert lib.bt709hip_graph_destroy(rig.ctx, g) == 0 and lib.bt709hip_stream_destroy(rig.ctx, S) == 0
        rig.close()


def test_alpha_encode_issues_the_queued_frames_of_a_coalescing_decoder_first(fake, rig):
    lib = fake
    dec = C.c_void_p()
    assert lib.bt709hip_decoder_create(rig.ctx, 0, 0, C.byref(dec)) == 0 and lib.bt709hip_decoder_set_option(dec, _capi.OPT_COALESCE, 8) == 0
    assert lib.bt709hip_encoder_prepare(rig.ctx, LIN, LIN) == 0
    w, h = rig.w, rig.h
    fin, fout = C.c_void_p(), C.c_void_p()
    assert lib.bt709hip_malloc(rig.ctx, w * h * 3 // 2, C.byref(fin)) == 0 and lib.bt709hip_malloc(rig.ctx, w * h * 4, C.byref(fout)) == 0
    S = C.c_void_p()
    assert lib.bt709hip_stream_create(rig.ctx, C.byref(S)) == 0
    fa, sa = _capi.Frame(fin.value, w, fin.value + w * h, w, w, h, 1, 1), _capi.Surface(fout.value, w * 4, w, h, 0, 0)
    mark = lib.fake_hip_log_size()
    assert lib.bt709hip_decode(dec, C.byref(fa), None, C.byref(sa), w, h, S, 0) == 0  # validated and queued
    assert log(lib, mark) == []
    assert lib.bt709hip_encode_batch(rig.ctx, rig.n, rig.surfs(), rig.frames(), LIN, LIN, S, 0) == 0
    ops = [o for o in log(lib, mark) if o[1] == S.value]
    assert [o[0].split(":")[0] for o in ops] == ["kernel", "kernel"]
    assert ops[0][0].startswith("kernel:decode_nv12") and ops[0][3] == fout.value and ops[1][0].startswith("kernel:encode") and ops[1][3] == rig.dst.value
    assert lib.bt709hip_stream_synchronize(rig.ctx, S) == 0 and lib.bt709hip_stream_destroy(rig.ctx, S) == 0
    assert lib.bt709hip_decoder_destroy(dec) == 0
    assert lib.bt709hip_free(rig.ctx, fin) == 0 and lib.bt709hip_free(rig.ctx, fout) == 0


def test_every_other_entry_point_treats_the_value_as_an_unknown_format(fake, rig):
    """decode, decode_half, decode_scaled, render_scaled (in and out), unconvert and ring_create_ex: format 3 gets exactly
    the status the unknown format 7 gets (and that is an error) -- nothing but the encoder's input learned the value."""
    lib = fake
    dec = C.c_void_p()
    assert lib.bt709hip_decoder_create(rig.ctx, 0, 0, C.byref(dec)) == 0 and lib.bt709hip_decoder_setup(dec) == 0
    assert lib.bt709hip_render_scaled_prepare(rig.ctx) == 0
    w, h = rig.w, rig.h
    frame = rig.frames()
    frame[0].matrix = frame[0].transfer = 1

    def out(fmt, ww=w, hh=h):
        return _capi.Surface(rig.src.value, ww * 4, ww, hh, fmt, 0)

    def ring(fmt):
        opt, r = _capi.RingOptions(0, 0, 0, fmt, 0), C.c_void_p()
        rc = lib.bt709hip_ring_create_ex(dec, w, h, 2, 0, 1, C.byref(opt), C.byref(r))
        if rc == 0:
            lib.bt709hip_ring_destroy(r)
        return rc

    calls = {
        "decode": lambda fmt: lib.bt709hip_decode(dec, frame, None, C.byref(out(fmt)), w, h, None, 1),
        "decode_batch": lambda fmt: lib.bt709hip_decode_batch(dec, 1, frame, None, C.byref(out(fmt)), None, 1),
        "decode_half": lambda fmt: lib.bt709hip_decode_half(dec, frame, None, C.byref(out(fmt, w // 2, h // 2)), None, 1),
        "decode_scaled": lambda fmt: lib.bt709hip_decode_scaled(dec, frame, None, C.byref(out(fmt, 40, 10)), None, 1),
        "render_scaled in": lambda fmt: lib.bt709hip_render_scaled(rig.ctx, C.byref(out(fmt)), C.byref(_capi.Surface(rig.dst.value, 160, 40, 10, 0, 0)), None, 1),
        "render_scaled out": lambda fmt: lib.bt709hip_render_scaled(rig.ctx, C.byref(out(0)), C.byref(_capi.Surface(rig.dst.value, 160, 40, 10, fmt, 0)), None, 1),
        "unconvert": lambda fmt: lib.bt709hip_unconvert(dec, rig.dst, w * 4, w, h // 2, C.byref(out(fmt, w, h // 2)), None, 1),
        "ring_create_ex": ring,
        "prepare_format": lambda fmt: lib.bt709hip_decoder_prepare_format(dec, fmt),
    }
    for name, call in calls.items():
        assert call(0) == 0, name  # the call itself is sound
        assert call(ALPHA) == call(UNKNOWN) != 0, (name, call(ALPHA), call(UNKNOWN))
    assert lib.bt709hip_decoder_destroy(dec) == 0


def test_alpha_encode_path_is_sanitizer_and_leak_clean(tmp_path):
    """tests/native/alpha_encode_leak.cpp under ASan + UBSan + LeakSanitizer: the context's table is freed with the context."""
    exe = build(str(tmp_path / "alpha_encode_leak"), ["-fsanitize=address,undefined"], SHIM_SOURCES + [os.path.join(HERE, "native", "alpha_encode_leak.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "ok: alpha encode on the fake HIP runtime, 0 failures" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "ERROR: LeakSanitizer" not in r.stderr and "runtime error:" not in r.stderr


# ------------------------------------------------------------------ generated code

def kernel_body(asm, name):
    sym = "_ZN5bt709%d%sILj0EEEvNS_12EncodeParamsE" % (len(name), name)  # the template's NV12 instantiation
    assert len(re.findall(r"^%s:" % sym, asm, re.M)) == 1, sym
    m = re.search(r"^%s:.*?\n(.*?)^\s*\.end_amdhsa_kernel" % sym, asm, re.S | re.M)
    assert m, "%s is not in the generated code" % name
    return m.group(1)


def test_alpha_kernels_generated_code():
    """Both kernels exist; the fast one loads its quad with 16-byte loads, looks the bytes up in LDS (the TABLE was chosen,
    so no multiply-add of any kind), stores dwords, keeps no scratch; and neither holds an instruction of the list this pool
    forbids (tests/ISA_FORBIDDEN.md -- kept in a document, read from there)."""
    asm = open(product_build.emit_asm()).read()
    fast, general = kernel_body(asm, "encode_alpha_y"), kernel_body(asm, "encode_alpha_y_blocks")
    ins = [l.split()[0] for l in fast.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    assert ins.count("global_load_dwordx4") == 4, ins  # a row pair up front, the next one inside the loop
    assert ins.count("ds_read_u8") == 8 and ins.count("global_store_dword") == 3
    assert not [i for i in ins if i.startswith(("v_fma", "v_mad", "v_pk_fma", "v_mul_f", "v_add_f", "scratch_", "buffer_"))], ins
    assert re.search(r"\.amdhsa_group_segment_fixed_size 256\b", fast) and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", fast)
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", general)
    doc = open(os.path.join(HERE, "ISA_FORBIDDEN.md")).read()
    patterns = re.findall(r"`(s_[a-z_]+\*?)`", doc)
    assert len(patterns) >= 6, patterns
    for body in (fast, general):
        for pat in patterns:
            rx = re.compile(r"^\s*" + pat.replace("*", r"\w*") + r"\b", re.M)
            assert not rx.search(body), pat
        assert "s_setreg" not in body  # nothing here depends on a rounding mode
