"""CPU-side tests of the product (no GPU, no compute calls): the C-ABI library loads
and exports everything include/bt709hip.h and include/bt709hip_ext.h declare, the host-built tables and constants
equal the reference-pinned goldens, the kernel ISA honours the no-FMA contract, the
failure behaviour without a device is loud, and the N>1 control flow works over gloo.
"""
import ctypes as C
import json
import os
import re
import socket
import subprocess
import threading
import sys

import numpy as np
import pytest

import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi, build
from oracle_lib import GAMMA_NAMES
import abi_headers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return mb.load_library()


def test_library_is_not_older_than_its_sources(lib):
    """A failed rebuild must not leave tests running against a stale library."""
    assert not build.is_stale(), "libbt709hip.so is older than csrc/ or include/: the build failed or was skipped"


def test_library_exports_every_declared_symbol(lib):
    header = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    declared = set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", header))
    assert len(declared) == 103  # ABI 503: bt709hip_last_scaled_launch_info joined the 102 of ABI 502
    for name in declared:
        assert hasattr(lib, name), "library does not export " + name
    # and the ctypes table binds exactly that set
    assert declared == set(_capi.SYMBOLS)


def test_no_thread_local_crosses_translation_units():
    """Round 6's split shim first shipped `extern thread_local` variables shared between its files: every access from another
    translation unit goes through a TLS wrapper that tests a weak hidden init symbol, which clang resolves to the library's
    load address in -fPIC code -- the first kernel launch on a GPU jumped there (no CPU test launches anything).  The
    thread-locals are file-local now and reached through functions; the library must hold no TLS wrapper / init symbols."""
    csrc = os.path.join(os.path.dirname(mb.__file__), "csrc")
    for f in sorted(os.listdir(csrc)):
        assert "extern thread_local" not in open(os.path.join(csrc, f), encoding="utf-8").read(), f
    syms = subprocess.run(["nm", build.LIB], capture_output=True, text=True).stdout
    assert "_ZTW" not in syms and "_ZTH" not in syms


def test_header_compiles_as_plain_c(tmp_path):
    src = tmp_path / "t.c"
    for header in ("bt709hip.h", "bt709hip_ext.h"):  # each on its own (the second includes the first)
        src.write_text('#include "%s"\nint main(void){bt709hip_frame f; (void)f; return BT709HIP_MAX_BATCH==32?0:1;}\n' % header)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                            "-o", str(tmp_path / "t")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# the calls SURVEY 8(b) / the reference's headers name (Renderer/MetalRenderContext.h:17-105, MetalBT709Decoder.h:15-72,
# MetalScaleRenderContext.h:34-40, BGRAToBT709Converter.h:34-76, y4m_writer.h:194-241): what include/bt709hip.h declares
REFERENCE_TWINNED = {
    "bt709hip_context_create", "bt709hip_context_destroy", "bt709hip_device_count", "bt709hip_abi_version",
    "bt709hip_stream_create", "bt709hip_stream_destroy", "bt709hip_stream_synchronize",
    "bt709hip_malloc", "bt709hip_free", "bt709hip_memset", "bt709hip_upload", "bt709hip_download",
    "bt709hip_decoder_create", "bt709hip_decoder_destroy", "bt709hip_decoder_set_context", "bt709hip_decoder_set_alpha_fill",
    "bt709hip_decoder_get_gamma", "bt709hip_decoder_has_alpha", "bt709hip_decoder_context", "bt709hip_decoder_setup",
    "bt709hip_decode", "bt709hip_decode_batch", "bt709hip_decode_half", "bt709hip_decode_scaled", "bt709hip_render_scaled",
    "bt709hip_unconvert", "bt709hip_encode", "bt709hip_interleave_cbcr", "bt709hip_deinterleave_cbcr",
    "bt709hip_strerror", "bt709hip_last_hip_error", "bt709hip_last_hip_error_string",
}


def test_boundary_is_split_into_reference_twins_and_extensions():
    """Round 6: include/bt709hip.h is the thin boundary SURVEY 8(b) describes -- at most 250 lines, exactly the calls that replace
    a reference interface -- and everything without a twin (rings, ring sets, shards, pools, coalescing, graphs, events,
    options, batched side paths, introspection) sits in include/bt709hip_ext.h, which includes it.  The shim is split along the
    same line and no file of csrc/ exceeds 900 lines."""
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    core = set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", strip(abi_headers.core_text())))
    ext = set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", strip(abi_headers.ext_text())))
    assert core == REFERENCE_TWINNED
    assert not core & ext and len(core | ext) == 103
    assert abi_headers.core_text().count("\n") <= 250
    assert '#include "bt709hip.h"' in abi_headers.ext_text() and "bt709hip_ext.h" not in strip(abi_headers.core_text())
    csrc = os.path.join(os.path.dirname(mb.__file__), "csrc")
    for f in sorted(os.listdir(csrc)):
        assert open(os.path.join(csrc, f), encoding="utf-8").read().count("\n") <= 900, f
    # the pool / ring / shard handles are extension types: the core header does not even name them
    for word in ("bt709hip_pool", "bt709hip_ring", "bt709hip_shard", "coalesc", "graph", "event"):
        assert word not in strip(abi_headers.core_text()), word


def test_matrix_constants_bit_patterns(lib, oracle):
    """BT709.h:386-397 evaluated in float; patterns recorded in SURVEY.md section 7."""
    c = (C.c_float * 8)()
    assert lib.bt709hip_matrix_constants(c) == 0
    bits = np.array(list(c), dtype=np.float32).view(np.uint32)
    assert [hex(b) for b in bits[:6]] == ["0x3b808081", "0x3f950a85", "0x3fe5788a", "0xbe5a5dd8", "0xbf086cbf",
                                          "0x40073197"]
    # the same numbers drive the oracle: Y=235 grey -> 1.0 exactly after saturation, etc.
    inv255, my, mcr_r, mcb_g, mcr_g, mcb_b = [np.float32(v) for v in list(c)[:6]]
    for (Y, Cb, Cr) in [(16, 128, 128), (235, 128, 128), (81, 90, 240), (145, 54, 34), (41, 240, 110), (255, 0, 255)]:
        yv = np.float32(np.float32(np.float32(Y - 16) * inv255) * my)
        cbn = np.float32(np.float32(Cb - 128) * inv255)
        crn = np.float32(np.float32(Cr - 128) * inv255)
        r = np.float32(yv + np.float32(crn * mcr_r))
        g = np.float32(np.float32(yv + np.float32(cbn * mcb_g)) + np.float32(crn * mcr_g))
        b = np.float32(yv + np.float32(cbn * mcb_b))
        want = oracle.ycbcr_to_rgbn(Y, Cb, Cr)
        got = np.clip(np.array([r, g, b], np.float32), 0, 1)
        assert np.array_equal(got.view(np.uint32) & 0x7FFFFFFF, want.view(np.uint32) & 0x7FFFFFFF)


@pytest.mark.parametrize("gamma", [0, 1, 2, 3])
def test_host_built_thresholds_equal_reference(lib, refdata, oracle, gamma):
    """The table the kernel looks up is built by the product's own host code at
    -setupMetal time; it must equal the thresholds derived from the reference headers."""
    t = np.zeros(255, np.float32)
    assert lib.bt709hip_gamma_thresholds(gamma, t.ctypes.data_as(C.POINTER(C.c_float))) == 0
    want = np.array([int(x, 16) for x in refdata["thresholds_hex"][GAMMA_NAMES[gamma]]], dtype=np.uint32)
    assert np.array_equal(t.view(np.uint32), want)
    assert np.array_equal(t.view(np.uint32), oracle.thresholds(gamma).view(np.uint32))
    assert lib.bt709hip_gamma_thresholds(7, t.ctypes.data_as(C.POINTER(C.c_float))) == _capi.ERR_INVALID_ARG


@pytest.mark.parametrize("gamma", [0, 1, 2, 3])
def test_host_decode_table_lookup_is_exact_at_every_breakpoint(lib, oracle, gamma):
    """The table the 1:1 kernels stage (bt709hip_gamma_lookup_decode): for the LINEAR mode the LOG-bucket form -- bucket =
    (bits(x + 2^-5) >> 16) - first, 645 buckets instead of 4 096 -- replayed on the host with the kernels' own index function.
    Breakpoints are the thresholds and the bucket boundaries (the floats x where x + 2^-5 crosses a multiple of 2^16 in its
    bit pattern): every float within 2 ulps of each against the oracle's composite, plus a strided sweep; the index is
    monotone and ends at the last bucket."""
    n, q, log_form = C.c_int(), C.c_int(), C.c_int()
    assert lib.bt709hip_gamma_lookup_decode(gamma, 0.0, C.byref(n), C.byref(q), C.byref(log_form)) == oracle.transfer_to_byte(gamma, 0.0)
    assert q.value == 0 and log_form.value == (1 if gamma == 2 else 0)
    N = n.value
    if not log_form.value:
        m = C.c_int()
        lib.bt709hip_gamma_lookup(gamma, 0.0, C.byref(m), None)
        assert N == m.value  # the uniform table: covered by the test below
        return
    assert N == 645
    pts = set()
    thr = oracle.thresholds(gamma)
    for t in thr[np.isfinite(thr)].view(np.uint32):
        pts.update(range(max(int(t) - 2, 0), int(t) + 3))
    add = np.float32(2.0 ** -5)
    for k in range(int(np.array([add], np.float32).view(np.uint32)[0]) >> 16, (0x3F800000 >> 16) + 8):
        edge = np.array([k << 16], np.uint32).view(np.float32)[0] - add  # exact: both are multiples of 2^-28 here or coarser
        if 0.0 <= edge <= 1.0:
            b = int(np.array([edge], np.float32).view(np.uint32)[0])
            pts.update(range(max(b - 3, 0), b + 4))
    pts.update(range(0, 0x3F800000, 104729))
    one = 0x3F800000
    xs = np.array(sorted(p for p in pts if p <= one), dtype=np.uint32).view(np.float32)
    last_q, seen = -1, set()
    for x in xs:
        got = lib.bt709hip_gamma_lookup_decode(gamma, float(x), None, C.byref(q), None)
        assert got == oracle.transfer_to_byte(gamma, float(x)), (gamma, float(x).hex())
        assert last_q <= q.value < N
        last_q = q.value
        seen.add(q.value)
    assert last_q == N - 1 and len(seen) == N  # every bucket visited, x == 1.0 in the last one
    assert lib.bt709hip_gamma_lookup_decode(gamma, 1.5, None, None, None) == _capi.ERR_INVALID_ARG


@pytest.mark.parametrize("gamma", [0, 1, 2, 3])
def test_host_bucket_lookup_is_exact_at_every_breakpoint(lib, oracle, gamma):
    """The kernels' lookup (bucket index by one float add, then one compare) replayed on the host:
    a piecewise-constant function can only be wrong next to a breakpoint, and its breakpoints are
    the 255 thresholds and the bucket boundaries -- every float within 2 ulps of each is checked
    against the oracle's composite (double pow inside), plus a strided sweep of [0, 1]."""
    n, q = C.c_int(), C.c_int()
    assert lib.bt709hip_gamma_lookup(gamma, 0.0, C.byref(n), C.byref(q)) == oracle.transfer_to_byte(gamma, 0.0)
    N = n.value
    assert N in (256, 512, 1024, 2048, 4096) and q.value == 0
    pts = set()
    thr = oracle.thresholds(gamma)
    for t in thr[np.isfinite(thr)].view(np.uint32):
        pts.update(range(max(int(t) - 2, 0), int(t) + 3))
    for k in range(N + 1):  # boundaries sit near (k +- 0.5) / N (and k / N for the round-1 floor form)
        for c in (np.float32(k / N), np.float32((k + 0.5) / N)):
            b = int(np.array([min(c, np.float32(1.0))], np.float32).view(np.uint32)[0])
            pts.update(range(max(b - 2, 0), b + 3))
    pts.update(range(0, 0x3F800000, 104729))
    one = 0x3F800000
    xs = np.array(sorted(p for p in pts if p <= one), dtype=np.uint32).view(np.float32)
    last_q = -1
    for x in xs:
        got = lib.bt709hip_gamma_lookup(gamma, float(x), None, C.byref(q))
        assert got == oracle.transfer_to_byte(gamma, float(x)), (gamma, float(x).hex())
        assert last_q <= q.value <= N  # the index function is monotone
        last_q = q.value
    assert last_q == N  # x == 1.0 lands in the last bucket
    assert lib.bt709hip_gamma_lookup(gamma, 1.5, None, None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_gamma_lookup(9, 0.5, None, None) == _capi.ERR_INVALID_ARG


def test_decoder_and_context_options(lib):
    """Tuning knobs are per-object options, not environment variables; values are clamped."""
    d, v = C.c_void_p(), C.c_int()
    assert lib.bt709hip_decoder_create(None, 0, 0, C.byref(d)) == 0
    for opt, default in ((_capi.OPT_NONTEMPORAL, 1), (_capi.OPT_HALF_KERNEL, -1), (_capi.OPT_HALF_WORKGROUPS, 0),
                         (_capi.OPT_HALF_LDS_KB, 0)):
        assert lib.bt709hip_decoder_get_option(d, opt, C.byref(v)) == 0 and v.value == default
    assert lib.bt709hip_decoder_set_option(d, _capi.OPT_HALF_KERNEL, 7) == 0
    assert lib.bt709hip_decoder_get_option(d, _capi.OPT_HALF_KERNEL, C.byref(v)) == 0 and v.value == 1
    assert lib.bt709hip_decoder_set_option(d, _capi.OPT_HALF_WORKGROUPS, -5) == 0
    assert lib.bt709hip_decoder_get_option(d, _capi.OPT_HALF_WORKGROUPS, C.byref(v)) == 0 and v.value == 0
    assert lib.bt709hip_decoder_set_option(d, _capi.OPT_HALF_LDS_KB, 9999) == 0
    assert lib.bt709hip_decoder_get_option(d, _capi.OPT_HALF_LDS_KB, C.byref(v)) == 0 and v.value == 160
    assert lib.bt709hip_decoder_set_option(d, 99, 1) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_decoder_get_option(d, 99, C.byref(v)) == _capi.ERR_INVALID_ARG
    # round 4: the coalescing submit is off by default, clamped to 2..32 frames per launch, 0 / 1 turn it off; a decoder
    # without a render context queues nothing (decode fails with NOT_SETUP as before) and flushes trivially
    assert lib.bt709hip_decoder_get_option(d, _capi.OPT_COALESCE, C.byref(v)) == 0 and v.value == 0
    for asked, got in ((8, 8), (1000, 32), (1, 0), (-3, 0), (2, 2)):
        assert lib.bt709hip_decoder_set_option(d, _capi.OPT_COALESCE, asked) == 0
        assert lib.bt709hip_decoder_get_option(d, _capi.OPT_COALESCE, C.byref(v)) == 0 and v.value == got
    assert lib.bt709hip_decoder_flush(d, None) == 0 and lib.bt709hip_decoder_flush_all(d) == 0
    assert lib.bt709hip_decoder_flush(None, None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_decoder_has_alpha(d) == 0 and lib.bt709hip_decoder_context(d) is None
    f = _capi.Frame(1, 16, 1, 16, 16, 2, 1, 1)
    o = _capi.Surface(1, 64, 16, 2, 0, 0)
    assert lib.bt709hip_decode(d, C.byref(f), None, C.byref(o), 16, 2, None, 0) == _capi.ERR_NOT_SETUP
    lib.bt709hip_decoder_destroy(d)
    # the frame ring: argument errors need no GPU; a decoder without a context cannot make one
    r = C.c_void_p()
    assert lib.bt709hip_ring_create(None, 64, 16, 4, 0, 1, C.byref(r)) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_decoder_create(None, 0, 0, C.byref(d)) == 0
    assert lib.bt709hip_ring_create(d, 64, 16, 4, 0, 1, None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_ring_create(d, 63, 16, 4, 0, 1, C.byref(r)) == _capi.ERR_ODD_DIMENSIONS
    assert lib.bt709hip_ring_create(d, 64, 16, 70000, 0, 1, C.byref(r)) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_ring_create(d, 64, 16, 4, 0, 1, C.byref(r)) == _capi.ERR_NOT_SETUP and not r.value
    lib.bt709hip_decoder_destroy(d)
    assert lib.bt709hip_ring_destroy(None) == 0 and lib.bt709hip_ring_frames(None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_ring_decode(None, 0, 1, None, 0) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_ring_placement_info(None, None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_mem_info(None, None, None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_last_launch_info(None) == _capi.ERR_INVALID_ARG
    # the rescale launchers' record: NULL is an argument error; a thread that has launched no rescale has no record, and the struct is left alone
    assert lib.bt709hip_last_scaled_launch_info(None) == _capi.ERR_INVALID_ARG
    seen = []

    def fresh_thread():
        info = _capi.ScaledLaunchInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        seen.append((lib.bt709hip_last_scaled_launch_info(C.byref(info)), bytes(info)))
    t = threading.Thread(target=fresh_thread)
    t.start(), t.join()
    assert seen == [(_capi.ERR_NOT_SETUP, b"\x5a" * C.sizeof(_capi.ScaledLaunchInfo))]
    assert lib.bt709hip_context_set_option(None, _capi.CTX_OPT_GRID_MULT, 2) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_abi_version() == _capi.ABI_VERSION
    hdr = abi_headers.core_text()
    assert "#define BT709HIP_VERSION %d" % _capi.ABI_VERSION in hdr
    src = "".join(open(os.path.join(os.path.dirname(mb.__file__), "csrc", f)).read()
                  for f in os.listdir(os.path.join(os.path.dirname(mb.__file__), "csrc")))
    assert "getenv" not in src  # no knob is read from the environment, least of all per launch


def test_no_device_fails_loudly(lib):
    """No GPU here: nothing silently falls back to a CPU path."""
    import torch  # noqa: F401  (only to learn whether a GPU exists)
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert lib.bt709hip_device_count() == 0
    h = C.c_void_p()
    assert lib.bt709hip_context_create(0, C.byref(h)) == _capi.ERR_NO_DEVICE and not h.value
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal() is False
    dec = mb.MetalBT709Decoder()
    dec.metalRenderContext = ctx
    assert dec.setupMetal() is False and dec.lastStatus == _capi.ERR_NO_DEVICE
    assert dec.decodeBT709(None, None, None) is False
    with pytest.raises(RuntimeError):
        import gpu_helpers
        gpu_helpers._ctx = None
        gpu_helpers.context()


def test_decoder_without_context(lib):
    """-setupMetal returns FALSE when metalRenderContext is nil (MetalBT709Decoder.m:48-54)."""
    d = C.c_void_p()
    assert lib.bt709hip_decoder_create(None, 0, 0, C.byref(d)) == 0
    assert lib.bt709hip_decoder_setup(d) == _capi.ERR_NOT_SETUP
    assert lib.bt709hip_decoder_get_gamma(d) == 0
    assert lib.bt709hip_decoder_set_alpha_fill(d, 300) == _capi.ERR_INVALID_ARG
    f, s = _capi.Frame(), _capi.Surface()
    assert lib.bt709hip_decode(d, C.byref(f), None, C.byref(s), 0, 0, None, 1) == _capi.ERR_NOT_SETUP
    assert lib.bt709hip_decoder_destroy(d) == 0
    # hasAlphaChannel forces the sRGB function (.m:165-169)
    assert lib.bt709hip_decoder_create(None, 0, 1, C.byref(d)) == 0
    assert lib.bt709hip_decoder_get_gamma(d) == mb.MetalBT709GammaSRGB
    lib.bt709hip_decoder_destroy(d)
    assert lib.bt709hip_decoder_create(None, 9, 0, C.byref(d)) == _capi.ERR_INVALID_ARG


def test_pool_entry_points_reject_bad_arguments(lib):
    h, slot, y, c = C.c_void_p(), C.c_int(), C.c_void_p(), C.c_void_p()
    assert lib.bt709hip_pool_create(None, 64, 32, 2, C.byref(h)) == _capi.ERR_INVALID_ARG and not h.value
    d = C.c_void_p()
    assert lib.bt709hip_decoder_create(None, 0, 0, C.byref(d)) == 0
    assert lib.bt709hip_pool_create(d, 63, 32, 2, C.byref(h)) == _capi.ERR_ODD_DIMENSIONS
    assert lib.bt709hip_pool_create(d, 64, 32, 0, C.byref(h)) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_pool_create(d, 64, 32, 2, C.byref(h)) == _capi.ERR_NOT_SETUP      # decoder has no context
    lib.bt709hip_decoder_destroy(d)
    assert lib.bt709hip_pool_acquire(None, C.byref(slot), C.byref(y), None, C.byref(c), None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_pool_submit(None, 0) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_pool_wait(None, 0, C.byref(y), None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_pool_destroy(None) == 0


def test_shard_entry_points_reject_bad_arguments(lib):
    """bt709hip_shard_*: argument errors before any device is touched, and NO_DEVICE (never a CPU path) here."""
    h = C.c_void_p()
    dev = (C.c_int * 2)(0, 0)
    assert lib.bt709hip_shard_create(None, 2, 0, 0, 64, 32, 2, C.byref(h)) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_shard_create(dev, 0, 0, 0, 64, 32, 2, C.byref(h)) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_shard_create(dev, 2, 9, 0, 64, 32, 2, C.byref(h)) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_shard_create(dev, 2, 0, 0, 64, 32, 0, C.byref(h)) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_shard_create(dev, 2, 0, 0, 63, 32, 2, C.byref(h)) == _capi.ERR_ODD_DIMENSIONS
    assert lib.bt709hip_shard_create(dev, 2, 0, 0, 64, 32, 2, None) == _capi.ERR_INVALID_ARG
    if lib.bt709hip_device_count() <= 0:
        assert lib.bt709hip_shard_create(dev, 2, 0, 0, 64, 32, 2, C.byref(h)) == _capi.ERR_NO_DEVICE and not h.value
        sh = mb.FrameSharder([0, 0], (64, 32))
        assert sh.handle is None and sh.lastStatus == _capi.ERR_NO_DEVICE and sh.submit(np.zeros((32, 64), np.uint8), np.zeros((16, 64), np.uint8)) is None
    t = C.c_uint64()
    p = C.c_void_p()
    assert lib.bt709hip_shard_submit(None, None, None, C.byref(t)) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_shard_wait(None, 0, C.byref(p), None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_shard_commit(None, 0) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_shard_cancel(None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_shard_lanes(None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_shard_destroy(None) == _capi.OK
    assert lib.bt709hip_pool_release(None, 0) == _capi.ERR_INVALID_ARG


def test_graph_entry_points_reject_bad_arguments(lib):
    """No device needed: argument checks come first, and a NULL context never reaches HIP."""
    g = C.c_void_p()
    assert lib.bt709hip_graph_begin_capture(None, None) == _capi.ERR_INVALID_ARG   # capture needs a created stream
    assert lib.bt709hip_graph_begin_capture(None, 1) == _capi.ERR_INVALID_ARG      # ... and a context
    assert lib.bt709hip_graph_end_capture(None, None, C.byref(g)) == _capi.ERR_INVALID_ARG and not g.value
    assert lib.bt709hip_graph_launch(None, None, None) == _capi.ERR_INVALID_ARG
    assert lib.bt709hip_graph_destroy(None, None) == 0                              # destroying nothing is fine


def test_strerror_covers_every_status(lib):
    seen = set()
    for code in range(0, -12, -1):
        msg = lib.bt709hip_strerror(code).decode()
        assert msg and msg != "unknown status"
        seen.add(msg)
    assert len(seen) == 12
    assert lib.bt709hip_strerror(-99).decode() == "unknown status"


def test_copyBT709ToCoreVideo_packing(oracle):
    """Host plumbing twin of BGRAToBT709Converter.m:1042-1099, checked against the oracle's
    restatement without touching a device."""
    rng = np.random.default_rng(5)
    w, h = 12, 6
    packed = rng.integers(0, 1 << 24, w * h, dtype=np.uint32)
    captured = {}

    class FakeBuf:
        width, height = w, h

        def upload_planes(self, y, c):
            captured["y"], captured["c"] = y.copy(), c.copy()

    assert mb.BGRAToBT709Converter.copyBT709ToCoreVideo(packed, FakeBuf())
    y, c = oracle.packed_to_nv12(packed, w, h)
    assert np.array_equal(captured["y"], y) and np.array_equal(captured["c"], c)


# ------------------------------------------------------------------ ISA contract

@pytest.fixture(scope="module")
def asm():
    return open(build.emit_asm()).read()


def _kernel_bodies(asm, mangled_fragment):
    found = re.findall(r"^_ZN5bt709\w*%s\w*:[^\n]*\n(.*?)^\.Lfunc_end" % mangled_fragment, asm, flags=re.S | re.M)
    assert found, mangled_fragment
    return found


def _kernel_body(asm, mangled_fragment):
    return _kernel_bodies(asm, mangled_fragment)[0]


def test_isa_fused_multiply_adds_are_only_the_proven_one(asm):
    """Every multiply and add of the matrix step must round separately (BT709.h:424-426 is evaluated
    without contraction on the CPU).  The ONE fused multiply-add the decode kernels contain is
    centre_norm's byte * (1/255f) - off * (1/255f) (bt709_device.h): the same single rounding of
    (byte - off) / 255f as the reference's exact integer subtract + one multiply.  So: every fma-class
    instruction has 1/255f (0x3b808081) as its multiplier, and a multiply fused with the float -> half
    conversion (v_fma_mix*: one rounding instead of two) appears nowhere."""
    n = fused = 0
    for kernel in ("12decode_quadsILj0E", "16decode_quads_logILj0E", "13decode_blocksILj0E", "16decode_nv12_half", "20decode_nv12_half_rep",
                   "18decode_nv12_scaled", "19decode_nv12_rgba16fILi0E", "19decode_nv12_rgba16fILi1E", "13render_scaled"):
        # RGBA16F curve variant: the half CANDIDATE (bt709_rgba16f.hip half_texels; not reference arithmetic -- the threshold
        # table settles it, and tests/test_rgba16f.py sweeps it over every float) is slope * x + intercept: one fma with three
        # REGISTER operands per channel, 4 pixels x 3 channels per 2x2 block, NB x RP blocks per lane (the three shipped
        # shapes, template arguments 4 and 5), nothing else; and its bucket index comes from the ONE packed float instruction
        # of these kernels, v_pk_mul_f32 by the index scale, a pair of channels per instruction (6 per block): an index
        # function, not reference arithmetic.  No v_log_f32 / v_exp_f32 (round 4 took them out), no comparison with the
        # split point, no select (round 5, packed-pair form).
        for body in _kernel_bodies(asm, kernel):
            candidate_fmas = index_muls = 0
            if kernel == "19decode_nv12_rgba16fILi1E":
                nb, rp = map(int, re.search(r"19decode_nv12_rgba16fILi1ELb[01]ELb[01]ELi(\d+)ELi(\d+)EE", body).groups())
                assert (nb, rp) in ((4, 2), (4, 3), (2, 3))
                candidate_fmas, index_muls = 12 * nb * rp, 6 * nb * rp
                assert len(re.findall(r"\bv_cvt_pkrtz_f16_f32", body)) == index_muls and len(re.findall(r"\bv_pk_max_u16", body)) == index_muls
                assert len(re.findall(r"\bv_cvt_pk_f16_f32", body)) == 8 * nb * rp       # (R, G) and (B, A) of every pixel
                assert len(re.findall(r"\bds_read_b64", body)) == 12 * nb * rp and len(re.findall(r"\bds_read_b32", body)) == 12 * nb * rp
                assert not re.search(r"\bv_cmp_(lt|gt)_f32", body)                      # nothing is compared with the split point
            if kernel == "19decode_nv12_rgba16fILi0E":
                assert "ds_read" not in body and not re.search(r"\bv_cvt_f16_f32", body)  # LINEAR: the packed conversion alone
            candidate = 0
            for line in re.findall(r"^\s*(v_(?:pk_)?(?:fma|fmac|fmamk|fmaak|mad|mac|madmk|madak)_(?:f32|f16|legacy|mix)\w*\s[^\n]*)", body, flags=re.M):
                if candidate_fmas and re.match(r"v_fmac_f32_e32 v\d+, v\d+, v\d+$|v_fma_f32 v\d+, v\d+, v\d+, v\d+$", line.strip()):
                    candidate += 1
                    continue
                if re.match(r"v_fmaak_f32 v\d+, [sv]\d+, v\d+, 0x4b000000$", line.strip()):
                    continue  # the uniform encode table's index, bits(fma(sum, k, 2^23)): an index function, not reference arithmetic
                if re.match(r"v_fmamk_f32 v\d+, v\d+, 0x5[23]800000, v\d+$|v_fmac_f32_e32 v\d+, 0x5[23]800000, v\d+$", line.strip()):
                    continue  # the log-bucket encode table's index, bits(fma(sum, 2^38 | 2^40, 2^-5)) >> 16: the product is exact (a power of two)
                assert re.match(r"v_fmamk_f32 v\d+, v\d+, 0x3b808081, v\d+|v_fmac_f32_e32 v\d+, 0x3b808081, v\d+", line), (kernel, line)
                fused += 1
            assert not re.search(r"\bv_pk_(fma|add)_f32", body), kernel  # half-rate packed f32 ops stay out (-fno-slp-vectorize)
            assert len(re.findall(r"\bv_pk_mul_f32", body)) == index_muls, kernel
            assert candidate == candidate_fmas, (kernel, candidate)
            assert not re.search(r"\bv_(log|exp)_f32", body), kernel  # no transcendental left in any decode kernel
            n += 1
    assert n == 55  # every instantiation the launchers can pick (round 5: the RGBA16F kernel in three shapes, the 1:1 kernel's big-table form; round 6: the any-ratio kernel's wave-decodes-once form, with and without alpha)
    # the RGBA16F kernels address LDS absolutely (table at byte 0): the dynamic allocation must be their only LDS
    seen = 0
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\s.*?\.name:\s+(\S+)", asm, flags=re.S):
        if "decode_nv12_rgba16f" in m.group(2):
            assert int(m.group(1)) == 0, m.group(2)
            seen += 1
    assert seen == 24
    assert fused > 300


def test_isa_memory_shape(asm):
    body = _kernel_body(asm, "12decode_quadsILj0ELb0ELb1ELb0EE")
    assert body.count("global_store_dwordx4") == 4          # 2 quads x 2 rows, 16 B per lane
    assert len(re.findall(r"global_store_dwordx4 .* nt", body)) == 4  # streaming (non-temporal) stores
    assert len(re.findall(r"global_load_dword\s", body)) == 6  # 2 quads x (2 luma rows + 1 CbCr row)
    assert "ds_read_b64" in body                            # one 8-byte table bucket per lookup
    assert body.count("ds_read_b64") == 48                  # 16 pixels x 3 channels
    assert not re.search(r"\bv_pk_(mul|add|fma)_f32", body)  # half-rate packed f32 ops stay out (-fno-slp-vectorize)
    assert "v_perm_b32" in body                             # 2-op BGRA pack
    # no wait on VMEM between the first quad's stores and the last ones: the wave never waits
    # for a write acknowledgement
    first, last = body.index("global_store_dwordx4"), body.rindex("global_store_dwordx4")
    assert "vmcnt" not in body[first:last]
    assert "scratch_" not in body                           # no spills
    meta = re.search(r"\.name:\s+_ZN5bt70912decode_quadsILj0ELb0ELb1ELb0EE.*?\.vgpr_count:\s+(\d+)", asm, flags=re.S)
    assert meta and int(meta.group(1)) <= 64                # 8 waves per SIMD


def test_isa_valu_budget_contract(asm):
    """The cycle-count decisions of DESIGN 6.0 hold in the generated code: bytes become floats with
    v_cvt_f32_ubyte (not the integer SDWA add + v_cvt_f32_i32 hipcc prefers), bucket indices come
    from a plain float add (no v_cvt_u32_f32 in the 1:1 kernel), the decode kernels never touch the
    MODE register (round-to-nearest bucket index), and in the encoder every switch of the rounding
    mode is undone inside the same asm statement."""
    quads = _kernel_body(asm, "12decode_quadsILj0ELb0ELb1ELb0EE")
    assert len(re.findall(r"\bv_cvt_f32_ubyte[0-3]", quads)) == 24          # 16 luma + 8 chroma bytes per 16 pixels
    assert not re.search(r"\bv_cvt_f32_i32|\bv_cvt_u32_f32|\bv_add_u32_sdwa", quads)
    assert len(re.findall(r"v_add_f32_e64 .* clamp", quads)) == 48            # saturation rides on the adds
    n = 0
    for kernel in ("12decode_quadsILj0E", "13decode_blocksILj0E", "16decode_nv12_half", "20decode_nv12_half_rep",
                   "18decode_nv12_scaled"):
        for body in _kernel_bodies(asm, kernel):
            assert "s_setreg" not in body, kernel
            n += 1
    assert n == 27
    for kernel in ("11encode_bgraILj0E", "18encode_bgra_blocksILj0E"):  # the NV12 instantiations
        assert len(_kernel_bodies(asm, kernel)) == 1, kernel
        for body in _kernel_bodies(asm, kernel):
            to_zero = len(re.findall(r"s_setreg_imm32_b32 hwreg\(HW_REG_MODE, 0, 2\), 3", body))
            to_even = len(re.findall(r"s_setreg_imm32_b32 hwreg\(HW_REG_MODE, 0, 2\), 0", body))
            assert to_zero == to_even and to_zero > 0, kernel
            # between a switch and its undo there is nothing but the instructions of that asm statement
            for block in re.findall(r"HW_REG_MODE, 0, 2\), 3\n(.*?)s_setreg_imm32_b32 hwreg\(HW_REG_MODE, 0, 2\), 0", body, flags=re.S):
                ops = {line.split()[0] for line in block.strip().split("\n") if line.strip()}
                assert ops <= {"v_add_f32", "v_cvt_pk_u8_f32"}, (kernel, ops)
    rep = _kernel_body(asm, "20decode_nv12_half_repILb1E")
    assert "ds_read_b128" in rep and not re.search(r"\bv_cvt_u32_f32\b.*\n.*v_and_or", rep)
    enc = _kernel_body(asm, "11encode_bgraILj0EE")
    assert enc.count("v_cvt_pk_u8_f32") == 12 and enc.count("v_lshlrev_b32_sdwa") == 24


def test_integration_doc_shows_the_shipped_objc_binding():
    """INTEGRATION.md section 2 embeds objc/MetalBT709Decoder+HIP.m verbatim (from its first #import), and
    that file implements the reference's selector unchanged (Renderer/MetalBT709Decoder.h:65-72)."""
    src = open(os.path.join(ROOT, "objc", "MetalBT709Decoder+HIP.m")).read()
    body = src[src.index('#import "MetalBT709Decoder.h"'):]
    assert body in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    flat = re.sub(r"\s+", "", body)
    for part in ("-(BOOL)decodeBT709:(CVPixelBufferRef)yCbCrPixelBuffer", "alphaPixelBuffer:(CVPixelBufferRef)alphaPixelBuffer",
                 "bgraSRGBTexture:(id<MTLTexture>)bgraSRGBTexture", "commandBuffer:(id<MTLCommandBuffer>)commandBuffer",
                 "renderPassDescriptor:(MTLRenderPassDescriptor*)renderPassDescriptor", "renderWidth:(int)renderWidth",
                 "renderHeight:(int)renderHeight", "waitUntilCompleted:(BOOL)waitUntilCompleted", "-(BOOL)setupMetal"):
        assert part in flat, part
    for call in ("bt709hip_pool_acquire", "bt709hip_pool_submit", "bt709hip_pool_wait", "bt709hip_pool_alpha_plane",
                 "bt709hip_pool_release"):
        assert call in body
    # the one-pass route: a nil texture is guarded and the render pass descriptor's attachment is the target
    assert "bgraSRGBTexture!=nil&&" in flat and "renderPassDescriptor.colorAttachments[0].texture" in body
    assert "__unsafe_unretained" not in body  # pending textures are held strongly


CLANG = "/opt/rocm/lib/llvm/bin/clang"
REF_RENDERER = "/root/reference/Renderer"


def _objc_syntax_check(path):
    return subprocess.run([CLANG, "-x", "objective-c", "-fsyntax-only", "-fobjc-arc", "-fobjc-runtime=macosx-10.14", "-Wall",
                           "-Werror", "-I", os.path.join(ROOT, "tests", "objc_stubs"), "-I", REF_RENDERER,
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "objc"), path],
                          capture_output=True, text=True)


@pytest.mark.skipif(not (os.path.exists(CLANG) and os.path.exists(os.path.join(REF_RENDERER, "MetalBT709Decoder.h"))),
                    reason="needs ROCm clang and the reference's headers (not on the GPU box)")
def test_objc_binding_parses(tmp_path):
    """The shipped Objective-C binding is at least WELL-FORMED against the reference's real public headers
    (Renderer/MetalBT709Decoder.h:27-72, MetalRenderContext.h): ROCm clang -fsyntax-only -fobjc-arc -Werror, with a
    tests-only stand-in for the Foundation / CoreVideo / Metal declarations it touches (tests/objc_stubs; no runtime, nothing
    built).  Round 3's file used self.hipDeferredCompletion without declaring it: the check must reject such a file."""
    src = os.path.join(ROOT, "objc", "MetalBT709Decoder+HIP.m")
    r = _objc_syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]
    # the check bites: the same file without the class extension's header fails exactly on the property
    broken = tmp_path / "broken.m"
    text = open(src).read()
    assert '#import "MetalBT709Decoder+HIP.h"' in text
    broken.write_text(text.replace('#import "MetalBT709Decoder+HIP.h"', "").replace("  [self finishHIPFrames];\n", ""))
    r = _objc_syntax_check(str(broken))
    assert r.returncode != 0 and "hipDeferredCompletion" in r.stderr
    # and the selector implemented is the one the reference declares: a mismatch would be an 'incomplete implementation' error
    hdr = open(os.path.join(REF_RENDERER, "MetalBT709Decoder.h")).read()
    assert "- (BOOL) decodeBT709:(CVPixelBufferRef)yCbCrInputTexture" in hdr


def test_no_experiment_gates_in_the_product_sources():
    """Wrong-output stubs and A/B forms live in tools/lab_variants.py (patches applied to a COPY of csrc/), never one -D away
    from the shipped kernels: no BT709_LAB_ macro, none of the round 1-3 A/B macros, no lab field in the kernarg block."""
    csrc = os.path.join(os.path.dirname(mb.__file__), "csrc")
    banned = ("BT709_LAB_", "BT709_NO_FMA_CENTRE", "BT709_INDEX_RTZ", "BT709_UNIFORM_INDEX_TWO_STEP", "BT709_REP_SPLIT_ENCODE",
              "walk_stagger", "walk_cus")
    for f in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, f), encoding="utf-8").read()
        for macro in banned:
            if macro == "BT709_INDEX_RTZ" and f == "transfer_tables.h":
                continue
            assert macro not in text, (f, macro)
    # every conditional left in the kernels is a correct-output tunable with a default (#ifndef X / #define X / #endif),
    # a header guard or the host / device switch of the shared quantiser header
    for f in sorted(os.listdir(csrc)):
        for line in open(os.path.join(csrc, f), encoding="utf-8"):
            if line.startswith("#if") and not line.startswith("#ifndef BT709_"):
                assert line.strip() in ("#if defined(__HIPCC__)", "#if defined(__clang__)"), (f, line)
    # the lab script still applies: its anchors exist exactly once in today's sources
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lab_variants
    for name, product, _ in lab_variants.GATES:
        assert lab_variants.resolve(csrc, name, product) is not None, (name, product[:60])


def test_documents_cite_evidence_that_exists():
    """Round 6: DESIGN.md is a contract a reader can use -- at most 30 KB, one evidence file per number -- and every
    `profiles/...` path DESIGN.md or README.md cites is a file in the repository (a pattern with * must match at least one)."""
    import glob
    assert os.path.getsize(os.path.join(ROOT, "DESIGN.md")) <= 30 * 1024
    for doc in ("DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc), encoding="utf-8").read()
        cited = set(re.findall(r"`(profiles/[A-Za-z0-9_\-./*+]+)`", text))
        assert doc != "DESIGN.md" or len(cited) >= 15, cited
        for path in sorted(cited):
            path = path.rstrip(".")
            hits = glob.glob(os.path.join(ROOT, path)) if "*" in path else [path] * os.path.exists(os.path.join(ROOT, path))
            assert hits, "%s cites %s, which does not exist" % (doc, path)
        for line in text.split("\n"):  # table cells a reader can take in: 300 characters in DESIGN.md's kernel table
            if doc == "DESIGN.md" and line.startswith("| `") and "evidence" not in line[:40]:
                for cell in line.strip("|").split("|"):
                    assert len(cell.strip()) <= 330, (len(cell), cell[:80])


def test_product_never_touches_the_oracle():
    pkg = os.path.dirname(mb.__file__)
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f), encoding="utf-8").read()
                assert "oracle_lib" not in text and "liboracle" not in text and "bt709_oracle" not in text, f
    assert "oracle" not in abi_headers.text()


# ------------------------------------------------------------------ N > 1 control flow

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_bench_two_ranks_gloo_dry_run():
    """world_size 2 on CPU: rendezvous, barriers, MAX over ranks, exactly one JSON line,
    whole-job value = 2 x per-rank work / slowest rank."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "1", "--dry-run", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 5 and res["scaling"] == "weak"
    assert res["repeats"] >= 5 and res["value_min"] <= res["value"] <= res["value_max"]
    assert res["unit"] == "Gpixel/s" and res["roofline"]["bound"] == "hbm"
    # 2 ranks x 5 steps x 256 x 4K pixels over >= 5 x 2 ms (dry run sleeps 2 ms per step)
    px = 2 * 5 * 256 * 3840 * 2160
    assert res["value"] <= px / (5 * 0.002) / 1e9
    assert abs(res["value"] - px / (res["ms_per_step"] * 5e-3) / 1e9) / res["value"] < 1e-3
    assert "cpu_baseline" not in res
    # the K-step region of the contract is timed and reported; the quoted figure comes from regions stretched to
    # >= 100 ms: K x m steps, m agreed between the ranks (5 steps x 2 ms -> m = 10)
    # (the stretch factor comes from ONE calibration region; on a loaded CPU box that region can be slow and the timed ones
    # fast, so the product is held to half the target here, not to the target)
    assert res["region_steps"] % res["steps"] == 0 and res["region_steps"] >= 2 * res["steps"] and res["region_steps"] * res["ms_per_step"] >= 50.0
    assert 9.0 <= res["k_step_region_ms"] <= 120.0


def test_bench_two_ranks_gloo_dry_run_batch8():
    """BASELINE config 5's shape on 2 ranks: a step is 8 frames over the whole job, each rank one
    launch of 4; strong scaling; the median of >= 5 repeats is reported."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "1", "--dry-run",
           "--workload", "4k-batch8", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["scaling"] == "strong" and res["config"]["frames_per_step_per_gpu"] == 4
    assert res["repeats"] >= 5 and res["value_min"] <= res["value"] <= res["value_max"]
    px = 5 * 8 * 3840 * 2160  # 5 steps x 8 frames, whatever the rank count
    assert abs(res["value"] - px / (res["ms_per_step"] * 5e-3) / 1e9) / res["value"] < 1e-3


@pytest.mark.parametrize("n", [2, 8])
def test_bench_plain_command_launches_its_own_ranks(n):
    """`python3 bench.py --gpus N` with no launcher around it (the driver's recorded command is a plain python3 line): the
    process starts its N ranks itself, relays ONE JSON line and nothing else on stdout, rc 0."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "5", "--warmup", "1",
                        "--dry-run"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[:500]
    res = json.loads(lines[0])
    assert res["n_gpus"] == n and res["steps"] == 5 and res["scaling"] == "weak"
    assert res["config"]["launcher"] == "self (bench.py started its %d ranks)" % n
    px = n * 5 * 256 * 3840 * 2160
    assert abs(res["value"] - px / (res["ms_per_step"] * 5e-3) / 1e9) / res["value"] < 1e-3


def test_bench_eight_rank_plan_fits_the_node():
    """Round 6: the 8-GPU line is the driver's to measure; what can be checked here is that the job FITS.  `python3 bench.py
    --gpus 8 --dry-run` runs the real geometry code and reports config.memory_plan for one rank: the two resident rings and the
    placement hunt's budget under the library's default (twice the ring) against a 288 GB MI355X, and the host memory of all
    eight ranks (frames are generated one at a time and uploaded; a rank keeps only the spot check's frames) against 16 GB --
    printed, so the number is in the test log."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    for workload in ("4k", "4k-batch8", "8k-half"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--dry-run",
                            "--workload", workload], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        res = json.loads(r.stdout.splitlines()[0])
        plan = res["config"]["memory_plan"]
        print("%s x 8 ranks: ring %.1f GB, device peak %.1f GB per GPU during the hunt (budget %.1f GB), %.1f GB steady; host %.2f GB per rank, %.2f GB for the job"
              % (workload, plan["ring_bytes"] / 1e9, plan["device_peak_bytes_per_gpu"] / 1e9, plan["hunt_budget_bytes"] / 1e9,
                 plan["device_steady_bytes_per_gpu"] / 1e9, plan["host_bytes_per_rank"] / 1e9, plan["host_bytes_all_ranks"] / 1e9))
        assert res["n_gpus"] == 8 and plan["ranks"] == 8 and plan["fits_288GB_per_gpu"]
        assert plan["hunt_budget_bytes"] == 2 * plan["ring_bytes"]  # item 2's default: the incumbent pair + one candidate pair
        assert plan["device_peak_bytes_per_gpu"] == 3 * plan["ring_bytes"] <= 0.25 * 288e9
        assert plan["host_bytes_all_ranks"] <= 16e9 and plan["host_bytes_per_rank"] < 1.0e9
    import bench
    g = bench.geometry("4k", 0, 65535)
    assert bench.memory_plan(g, bench.parse_args([]))["ring_bytes"] == 256 * (3840 * 2160 * 3 // 2 + 3840 * 2160 * 4)  # 11.7 GB


def test_bench_plain_command_fails_when_a_rank_fails():
    """No GPU here and no --dry-run: every rank exits 'no HIP device'; the launcher must return non-zero, print no JSON
    line and leave no rank behind (it ends them by PID)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0 and r.stdout.strip() == "" and "no HIP device" in r.stderr


def _plain_bench(n, extra=(), env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "5", "--warmup", "1", "--dry-run",
                           "--full", *extra], capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)


@pytest.mark.parametrize("n", [2, 8])
def test_bench_every_rank_spot_checks_its_own_ring_and_reports_its_device(n):
    """The one line an N-GPU run prints must verify and describe itself (the reference's test flow reads back what it decoded,
    EmptyiOSTests/MetalBT709DecoderTests.m:189-277): every rank runs the parity spot check on its OWN ring, the line names each
    rank's device (ordinal + PCI bus id through the C ABI) and n_gpus counts DISTINCT devices, per-rank clocks beside the MAX."""
    r = _plain_bench(n)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.splitlines()[0])
    assert res["parity_spot_check"] == "ok" and res["parity_spot_check_ranks"] == n
    assert res["n_gpus"] == n and res["ranks"] == n and res["shared_devices"] is False
    devs = res["config"]["devices"]
    assert [d["rank"] for d in devs] == list(range(n)) and len({d["pci_bus_id"] for d in devs}) == n
    assert [d["ordinal"] for d in devs] == list(range(n))
    per = res["per_rank"]
    assert [p["rank"] for p in per] == list(range(n)) and all(p["parity_spot_check"] == "ok" for p in per)
    # value comes from the MAX over ranks: no rank's own clock is slower than the line's
    assert max(p["ms_per_step"] for p in per) <= res["ms_per_step"] * 1.001
    assert all(set(p["placement"]) >= {"chosen", "first_GBps", "chosen_GBps"} for p in per)


def test_bench_a_mismatch_on_any_rank_fails_the_job():
    """Rank 1's ring decodes wrong (forced on the dry-run path): value is null, the line says which rank, every rank exits 1."""
    r = _plain_bench(2, env_extra={"BT709_BENCH_DRY_MISMATCH_RANK": "1"})
    assert r.returncode != 0
    res = json.loads(r.stdout.splitlines()[0])
    assert res["value"] is None and res["parity_spot_check"].startswith("rank 1: MISMATCH") and res["parity_spot_check_ranks"] == 2
    assert [p["parity_spot_check"] == "ok" for p in res["per_rank"]] == [True, False]
    r = _plain_bench(8, env_extra={"BT709_BENCH_DRY_MISMATCH_RANK": "5"})
    assert r.returncode != 0 and json.loads(r.stdout.splitlines()[0])["parity_spot_check"].startswith("rank 5: MISMATCH")


def test_bench_refuses_ranks_that_wrap_onto_one_device():
    """world > visible devices: refused (rc 2, no JSON line) unless --allow-shared-devices, and then labelled: n_gpus = the
    DISTINCT devices, ranks = the processes (round 4 printed n_gpus 2 for two ranks on one GPU)."""
    r = _plain_bench(2, env_extra={"BT709_BENCH_DRY_DEVICES": "1"})
    assert r.returncode != 0 and r.stdout.strip() == "" and "--allow-shared-devices" in r.stderr
    r = _plain_bench(2, extra=("--allow-shared-devices",), env_extra={"BT709_BENCH_DRY_DEVICES": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.splitlines()[0])
    assert res["n_gpus"] == 1 and res["ranks"] == 2 and res["shared_devices"] is True and res["parity_spot_check_ranks"] == 2
    assert len({d["pci_bus_id"] for d in res["config"]["devices"]}) == 1 and [d["ordinal"] for d in res["config"]["devices"]] == [0, 0]
    r = _plain_bench(8, extra=("--allow-shared-devices",), env_extra={"BT709_BENCH_DRY_DEVICES": "4"})
    res = json.loads(r.stdout.splitlines()[0])
    assert res["n_gpus"] == 4 and res["ranks"] == 8 and res["shared_devices"] is True


def test_bench_per_rank_clocks_show_a_straggler():
    """Only the MAX over ranks makes `value`; the per-rank records tell a slow GPU from a launcher problem."""
    r = _plain_bench(2, env_extra={"BT709_BENCH_DRY_SLOW_RANK": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.splitlines()[0])
    fast, slow = res["per_rank"]
    assert slow["ms_per_step"] > 1.3 * fast["ms_per_step"] and abs(res["ms_per_step"] - slow["ms_per_step"]) / res["ms_per_step"] < 0.05


@pytest.mark.parametrize("n", [2, 8])
def test_bench_one_process_driving_n_gpus_prints_the_same_line_shape(n):
    """--launcher threads: ONE process, N devices (bt709hip_ringset_*; the reference's one-process shape,
    Renderer/AAPLRenderer.m:874-985).  No ranks are started; the line has the keys of the process-per-GPU form, one per_rank /
    config.devices record per LANE, n_gpus = the distinct devices."""
    procs = json.loads(_plain_bench(n).stdout.splitlines()[0])
    r = _plain_bench(n, extra=("--launcher", "threads"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.splitlines()) == 1
    res = json.loads(r.stdout.splitlines()[0])
    assert set(res) == set(procs) and set(res["config"]) == set(procs["config"]) and set(res["per_rank"][0]) == set(procs["per_rank"][0])
    assert res["n_gpus"] == n and res["ranks"] == n and res["shared_devices"] is False and res["parity_spot_check_ranks"] == n
    assert res["config"]["launcher"].startswith("threads (ONE process drives %d GPUs" % n)
    assert [d["rank"] for d in res["config"]["devices"]] == list(range(n)) and len({d["pci_bus_id"] for d in res["config"]["devices"]}) == n
    px = n * 5 * 256 * 3840 * 2160
    assert abs(res["value"] - px / (res["ms_per_step"] * 5e-3) / 1e9) / res["value"] < 1e-3
    # a lane that decodes wrong fails the job; lanes that wrap onto one device are refused unless asked for
    r = _plain_bench(n, extra=("--launcher", "threads"), env_extra={"BT709_BENCH_DRY_MISMATCH_RANK": str(n - 1)})
    assert r.returncode != 0 and json.loads(r.stdout.splitlines()[0])["parity_spot_check"].startswith("rank %d: MISMATCH" % (n - 1))
    r = _plain_bench(n, extra=("--launcher", "threads"), env_extra={"BT709_BENCH_DRY_DEVICES": "1"})
    assert r.returncode == 2 and r.stdout.strip() == ""
    r = _plain_bench(n, extra=("--launcher", "threads", "--allow-shared-devices"), env_extra={"BT709_BENCH_DRY_DEVICES": "1"})
    res = json.loads(r.stdout.splitlines()[0])
    assert res["n_gpus"] == 1 and res["ranks"] == n and res["shared_devices"] is True


def test_bench_geometry():
    import bench
    g = bench.geometry("4k", 0, 65535)
    assert (g["ring"], g["per_launch"], g["launches"]) == (256, 256, 1)  # one launch over the whole ring (XCD-aware work map)
    g = bench.geometry("1080p", 0, 65535)
    assert (g["ring"], g["per_launch"], g["launches"]) == (1024, 1024, 1)
    g = bench.geometry("4k", 0, 65535, 64)
    assert (g["ring"], g["per_launch"], g["launches"]) == (256, 64, 4)
    g = bench.geometry("4k", 64, 65535, 32)
    assert (g["ring"], g["per_launch"], g["launches"]) == (64, 32, 2)    # rounds 1-2's shape
    assert g["bytes_per_frame"] == 45_619_200
    g = bench.geometry("1080p", 0, 32)
    assert g["bytes_per_frame"] == 11_404_800
    g = bench.geometry("8k-half", 0, 32)
    assert g["bytes_per_frame"] == 82_944_000 and (g["OW"], g["OH"]) == (3840, 2160)
    g = bench.geometry("4k", 40, 32)
    assert g["ring"] == 32 and g["launches"] == 1
    for world, share in ((1, 8), (2, 4), (4, 2), (8, 1)):  # BASELINE config 5: frame i -> GPU i mod n
        g = bench.geometry("4k-batch8", 0, 65535, 0, world)
        assert (g["per_launch"], g["launches"], g["frames_per_step"], g["ring"]) == (share, 1, share, 64)
    assert bench.geometry("4k-batch8", 0, 65535, 0, 1, 2)["per_launch"] == 2  # --share: one GPU plays a rank of a 4-GPU job
    # every default ring's INPUT is several times the 256 MB memory-side cache (a ring that fits it measures the cache)
    for wl in bench.WORKLOADS:
        assert bench.geometry(wl, 0, 65535)["ring_input_over_cache"] >= 2.9, wl
    assert bench.geometry("4k", 16, 65535)["ring_input_over_cache"] < 1.0  # 16 x 12.4 MB: refused by main()


def test_bench_spot_check_samples_every_xcd_band():
    """bench.py's parity tripwire reads one ring frame out of each eighth of the ring (= each XCD band of a whole-ring launch),
    first and last frame included (round 3 read ring frame 0 only)."""
    import bench
    assert bench.sample_frames(256) == [0, 37, 70, 103, 136, 169, 202, 255]
    for ring in (8, 16, 64, 256, 1024):
        picks = bench.sample_frames(ring)
        assert len(picks) == 8 and picks[0] == 0 and picks[-1] == ring - 1
        assert sorted({p * 8 // ring for p in picks}) == list(range(8))
    assert bench.sample_frames(4) == [0, 1, 2, 3]


def test_bench_plain_run_times_exactly_the_steps():
    """A plain run (no --full) times ONE region of exactly --steps steps and does nothing its headline does not need: no
    stretched repeats, no parity spot check, no CPU baseline; ms_per_step is that region over --steps."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dry-run"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 7 and res["warmup"] == 2 and res["region_steps"] == 7 and res["repeats"] == 1
    assert res["value_min"] == res["value"] == res["value_max"]
    assert abs(res["ms_per_step"] * 7 - res["k_step_region_ms"]) < 1e-3 * res["k_step_region_ms"] + 1e-3
    px = 7 * 256 * 3840 * 2160
    assert abs(res["value"] - px / (res["ms_per_step"] * 7e-3) / 1e9) / res["value"] < 1e-3
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert key in res
    assert "cpu_baseline" not in res and res["parity_spot_check_ranks"] == 0 and res["parity_spot_check"].startswith("not run")
    assert "first_allocation_frac" not in res["roofline"] and "same_run_copy_GBps" not in res["roofline"]
    # a dry run computes nothing to dump: refused before it starts
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--dump-outputs", os.path.join(ROOT, "no_such_dir")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr and not os.path.exists(os.path.join(ROOT, "no_such_dir"))


def test_bench_dump_plan_is_fixed_and_bounded():
    """--dump-outputs samples the last step's output by a fixed plan: the same rows every run, inside the frames that step
    decoded and inside each frame, one frame per XCD band among them, at most 64 MB as float32 for every workload."""
    import bench
    sizes = [bench.geometry(wl, 0, 65535) for wl in bench.WORKLOADS]
    sizes.append(dict(bench.geometry("4k", 0, 65535), OW=7680, OH=4320))  # a wide clip (--y4m)
    sizes.append(dict(bench.geometry("4k", 0, 65535), OW=64, OH=8))       # a tiny one
    for g in sizes:
        for frames in (list(range(g["ring"])), list(range(16, 24)), [5]):
            plan = bench.dump_plan(g, frames)
            assert plan == bench.dump_plan(g, frames) and set(plan) == {"bgra_band_rows", "bgra_sampled_rows"}
            rows = 0
            for parts in plan.values():
                for f, r0, n in parts:
                    assert f in frames and 0 <= r0 and n >= 1 and r0 + n <= g["OH"]
                    rows += n
            assert rows * g["OW"] * 4 * 4 <= 64 << 20
            assert len(plan["bgra_sampled_rows"]) == 64
            band_frames = sorted({f for f, _, _ in plan["bgra_band_rows"]})
            assert band_frames == [frames[i] for i in bench.sample_frames(len(frames))]


def build_cpp_selftest(tmpdir):
    """g++ compile + link of the C++ host mirror against the C-ABI library."""
    exe = os.path.join(str(tmpdir), "decoder_selftest")
    libdir = os.path.dirname(build.LIB)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "host", "decoder_selftest.cpp"),
                        "-L" + libdir, "-lbt709hip", "-Wl,-rpath," + libdir, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_host_mirror_builds_and_fails_without_gpu(lib, tmp_path):
    exe = build_cpp_selftest(tmp_path)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([exe, "235", "128", "128", "255", "255", "255"], capture_output=True, text=True)
    assert r.returncode == 3  # setupMetal() false: no device, no fallback


def test_profile_summary_cuts_a_kernel_trace_to_the_sentinel_bracketed_regions(tmp_path):
    """tools/pmc_summary.py: bench.py brackets every timed region with two sentinel dispatches (copy_probe, 512 work-items
    opening, 1024 closing); only the decode dispatches between a pair are averaged -- set-up probes, warm-up, spot check and
    side legs run the same kernel and must not count (round 3's rocprof mean was off for that reason)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_summary
    rows = [("Kernel_Name", "Grid_Size", "Start_Timestamp", "End_Timestamp", "Dispatch_Id", "Counter_Name", "Counter_Value")]
    t = [1000]

    def add(name, grid, dur, did):
        rows.append((name, grid, t[0], t[0] + dur, did, "X", dur))
        t[0] += dur + 10
    dq = "void bt709::decode_quads<0u, false, true, false>(bt709::DecodeParams)"
    did = 0
    for dur in (374, 375):                      # the hunt's probes: outside any region
        did += 1; add(dq, 1 << 20, dur, did)
    did += 1; add("bt709::copy_probe(...)", 1 << 22, 5000, did)   # a big copy (the ring copy): not a sentinel
    for region in ((413, 414, 415), (412, 416)):
        did += 1; add("bt709::copy_probe(...)", 512, 2, did)
        for dur in region:
            did += 1; add(dq, 1 << 20, dur, did)
        did += 1; add("bt709::copy_probe(...)", 1024, 2, did)
        did += 1; add(dq, 1 << 20, 999, did)    # spot check / side leg between regions
    did += 1; add("bt709::copy_probe(...)", 512, 2, did)           # an opening sentinel that never closes
    did += 1; add(dq, 1 << 20, 777, did)
    trace = tmp_path / "trace.csv"
    import csv
    with open(trace, "w", newline="") as f:
        csv.writer(f).writerows(rows)
    timed = pmc_summary.timed_dispatches(str(trace), pmc_summary.DECODE_NV12)
    assert timed["regions"] == 2 and sorted(timed["by_kernel"][dq]) == [412, 413, 414, 415, 416]  # the region that never closed is dropped
    out = tmp_path / "stats.csv"
    pmc_summary.write_timed_stats(str(out), {"regions": 2, "by_kernel": {dq: [413, 414, 415, 412, 416]}})
    rec = list(csv.DictReader(open(out)))[0]
    assert rec["Calls"] == "5" and float(rec["AverageNs"]) == 414.0 and rec["MedianNs"] == "414" and "2 sentinel-bracketed" in rec["Scope"]
    # the same cut for a --pmc pass (by dispatch id): the probes and the unclosed tail stay out
    keep = pmc_summary.timed_dispatch_ids(list(csv.DictReader(open(trace))))
    durs = sorted(int(r["Counter_Value"]) for r in csv.DictReader(open(trace)) if r["Dispatch_Id"] in keep and "decode" in r["Kernel_Name"])
    assert durs == [412, 413, 414, 415, 416]
    # a trace without sentinels (another program than bench.py): no cut
    plain = tmp_path / "plain.csv"
    with open(plain, "w", newline="") as f:
        csv.writer(f).writerows([rows[0], rows[1], rows[2]])
    assert pmc_summary.timed_dispatches(str(plain), pmc_summary.DECODE_NV12) is None
    assert pmc_summary.timed_dispatch_ids(list(csv.DictReader(open(plain)))) is None


def test_ctypes_structs_match_the_header(tmp_path):
    """Every struct of include/bt709hip.h that crosses the C ABI by value or by pointer has a ctypes twin in _capi.py: a C program
    compiled against the header prints sizeof and the offset of every field, and they must equal ctypes' own layout -- a field
    added to the header alone (or to the bindings alone) fails here, before it mis-calls the library."""
    pairs = {"bt709hip_frame": _capi.Frame, "bt709hip_surface": _capi.Surface, "bt709hip_ring_placement": _capi.RingPlacement,
             "bt709hip_ring_options": _capi.RingOptions, "bt709hip_launch_info": _capi.LaunchInfo, "bt709hip_device_info": _capi.DeviceInfo,
             "bt709hip_scaled_launch_info": _capi.ScaledLaunchInfo}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bt709hip_ext.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr  # a field the header does not have is a compile error
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, cls in pairs.items():
        assert int(got["%s size" % cname]) == C.sizeof(cls), cname
        for field, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, field)]) == getattr(cls, field).offset, (cname, field)
    # and the header has no struct the bindings do not know (opaque handles aside)
    hdr = abi_headers.text()
    named = set(re.findall(r"^\} (bt709hip_\w+);", hdr, flags=re.M)) - {"bt709hip_status", "bt709hip_gamma", "bt709hip_matrix_tag",
                                                                        "bt709hip_transfer_tag", "bt709hip_format",
                                                                        "bt709hip_context_option", "bt709hip_decoder_option"}
    assert named == set(pairs), named ^ set(pairs)


def test_ctypes_constants_match_the_header():
    """Status codes, render-target formats and option ids of _capi.py against the enumerators of include/bt709hip.h, by name:
    BT709HIP_<NAME> = value  <->  _capi.<NAME> (BT709HIP_OK -> OK); every enumerator of those enums has a twin."""
    hdr = abi_headers.text()
    seen = 0
    for enum in ("bt709hip_status", "bt709hip_format", "bt709hip_context_option", "bt709hip_decoder_option"):
        body = re.search(r"typedef enum \{([^}]*)\} %s;" % enum, hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        for name, value in re.findall(r"BT709HIP_(\w+)\s*=\s*(-?\d+)", body):
            assert getattr(_capi, name) == int(value), (enum, name)
            seen += 1
    assert seen >= 12 + 2 + 5 + 7
    # the tap forms of bt709hip_scaled_launch_info.taps (an anonymous enum)
    taps = re.findall(r"BT709HIP_(SCALED_TAPS_\w+)\s*=\s*(\d+)", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert len(taps) == 5 and all(getattr(_capi, name) == int(value) for name, value in taps)
