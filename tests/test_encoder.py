"""BGRA -> NV12 encoder (the step before the decode path).

CPU part: the product's host-built encoder tables against the oracle, and the oracle's
encoder against numbers the reference asserts / produces; the kernel's own BT709_from_linear
lookup (csrc/bt709_split_lookup.h) replayed over EVERY float in [0, 1] for the three table kinds
(tests/native/split_table_sweep.cpp); guards that keep the generators of the GPU sweeps honest.
GPU part (-m gpu): the HIP encoder through the C ABI against the oracle, bit-exact -- small random
pictures, EVERY (R,G,B) as a flat block in the five gamma pairs, 2x2 blocks built to land on and one
step below each of the 255 thresholds in every summation order, the launch regimes the encoder ships
with (plan on record: bt709hip_last_launch_info) with padding and guard bands checked, fuzzed geometry
-- plus the full GPU round trip BGRA -> NV12 -> BGRA against the reference's own exhaustive-histogram
semantics.  Cases and helpers: tests/encoder_cases.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import encoder_cases as ec
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_APPLE, GAMMA_LINEAR, GAMMA_SRGB

PAIRS = ec.PAIRS
assert PAIRS == [(GAMMA_SRGB, GAMMA_APPLE), (GAMMA_SRGB, GAMMA_SRGB), (GAMMA_LINEAR, GAMMA_LINEAR),
                 (GAMMA_APPLE, GAMMA_APPLE), (GAMMA_SRGB, GAMMA_LINEAR)]
TABLE_ENCODE_APPLE = 4
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "metalbt709decoder_amd", "csrc")


# ------------------------------------------------------------------ CPU

def test_apple_encode_composite_is_a_threshold_function(oracle):
    """round(255*Apple196enc(v)) is monotone in v and equals its threshold table for every
    float in [0,1] -- the property the encoder's BT709_from_linear lookup rests on."""
    assert oracle.check_thresholds(TABLE_ENCODE_APPLE) == 0


def test_host_built_encode_thresholds_equal_oracle(oracle):
    lib = mb.load_library()
    t = np.zeros(255, np.float32)
    assert lib.bt709hip_gamma_thresholds(TABLE_ENCODE_APPLE, t.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert np.array_equal(t.view(np.uint32), oracle.thresholds(TABLE_ENCODE_APPLE).view(np.uint32))


def test_reference_subsample_vectors(oracle, refdata):
    """BT709_average_pixel_values outputs produced by the reference headers (golden)."""
    for b in refdata["subsample_blocks"]:
        assert list(oracle.subsample_block(b["rgb"], b["in"], b["out"])) == b["y4cbcr"]


def test_flat_block_equals_per_pixel_encode(oracle):
    """A 2x2 block of one colour subsamples to that colour's own (Y,Cb,Cr): the encode
    expectations of the reference's Metal tests are built this way
    (MetalBT709DecoderTests.m:137-185, encode type 'VImage' = the subsample path)."""
    rng = np.random.default_rng(11)
    for R, G, B in rng.integers(0, 256, (300, 3)):
        y4cbcr = oracle.subsample_block([int(R), int(G), int(B)] * 4, GAMMA_SRGB, GAMMA_APPLE)
        assert len(set(y4cbcr[:4])) == 1


@pytest.fixture(scope="module")
def split_sweep(tmp_path_factory, oracle):
    """tests/native/split_table_sweep.cpp + the product's table builder, plain g++ (as test_quantiser_exact.py builds its sweep)."""
    out = str(tmp_path_factory.mktemp("native") / "libsplit_table_sweep.so")
    odir = os.path.join(ROOT, "oracle")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wall", "-Werror",
           "-I", CSRC, "-I", odir, os.path.join(HERE, "native", "split_table_sweep.cpp"), os.path.join(CSRC, "transfer_tables.cpp"),
           "-o", out, "-L", odir, "-loracle", "-Wl,-rpath," + odir, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return C.CDLL(out)


@pytest.mark.parametrize("kind", [GAMMA_LINEAR, GAMMA_SRGB, TABLE_ENCODE_APPLE])
def test_split_table_lookup_is_from_linear_for_every_float(split_sweep, oracle, kind):
    """The encoder's BT709_from_linear: csrc/bt709_split_lookup.h (the text the two encode kernels compile) over the table
    build_split_table makes, for all 1 065 353 217 floats in [0, 1], equals the number of oracle thresholds <= x -- which is
    the reference's BT709_from_linear there, because the composite is a threshold function (checked for the same kinds by
    test_composite_is_a_threshold_function / test_apple_encode_composite_is_a_threshold_function).  The three kinds are what
    build_encode_tables selects: sRGB output -> the LINEAR decode composite, linear output -> the plain quantiser, Apple
    output -> kind 4.  A `>` for `>=`, an edge one step off, a wrong bucket at the fine / coarse split or an index past the
    table all count."""
    assert sorted({ec.from_linear_kind(o) for _, o in PAIRS}) == sorted([GAMMA_LINEAR, GAMMA_SRGB, TABLE_ENCODE_APPLE])
    out = (C.c_uint64 * 5)()
    assert split_sweep.sweep_split_table(kind, 0, 0x3F800000, ec.threads(), out) == 0
    assert out[4] == 0x3F800000 + 1
    assert out[0] == 0, "lookup differs from the thresholds on %d floats, first bits 0x%08x (table of %d buckets, n_fine %d)" % (
        out[0], out[1], out[2], out[3])


@pytest.fixture(scope="module")
def edge_sets(oracle):
    cache = {}

    def get(pair):
        if pair not in cache:
            cache[pair] = ec.edge_blocks(oracle, pair)
        return cache[pair]
    return get


@pytest.mark.parametrize("pair", PAIRS)
def test_edge_block_generator_lands_on_the_thresholds(oracle, reference, edge_sets, pair):
    """Keeps ec.edge_blocks honest, from the oracle alone (no GPU):
      * every threshold k = 1..255 of every channel has an upper and a lower block, in all 12 summation orders;
      * in the reference's order the oracle's averaged byte of that channel is k for the upper block and k - 1 for the lower;
      * for EVERY block (all orders) the NumPy float32 average, counted against the thresholds, is the oracle's averaged byte
        (a NumPy / C difference in summation order or rounding would show here);
      * at least 150 thresholds per pair are hit EXACTLY (average == threshold) and the median lower block lies one float32
        step below its threshold (Linear -> Linear is exempt from the median: only 1 366 sums are reachable there);
      * upper and lower block give different (Cb, Cr);
      * where the reference's headers are built, its averaged bytes equal the oracle's on every block."""
    eb = edge_sets(pair)
    meta, rgb = eb.meta, eb.rgb
    assert len(meta) == 3 * 255 * 2 * 12
    assert {(int(c), int(k), int(s)) for c, k, s, _, _ in meta} == {(c, k, s) for c in range(3) for k in range(1, 256) for s in (0, 1)}
    avg = np.array([oracle.average_bytes(b.reshape(-1).tolist(), *pair) for b in rgb])
    mine = np.stack([np.searchsorted(eb.T, ec.average_f32(eb.lin, rgb[:, :, c]), side="right") for c in range(3)], axis=1)
    assert np.array_equal(mine, avg)
    canon = meta[:, 3] == 0
    ch = meta[:, 0]
    own = avg[np.arange(len(meta)), ch]
    assert np.array_equal(own[canon], meta[canon, 1] - 1 + meta[canon, 2])
    exact = {int(k) for k in meta[(meta[:, 4] == 1) & canon, 1]}
    assert len(exact) >= 150, len(exact)
    hit = ec.average_f32(eb.lin, rgb[:, :, 0][canon & (ch == 0) & (meta[:, 2] == 1)])
    assert int((hit == eb.T).sum()) == len(exact)
    if pair != (GAMMA_LINEAR, GAMMA_LINEAR):
        assert np.median(eb.lower_ulps) <= 1, np.median(eb.lower_ulps)
    assert (eb.lower_ulps >= 1).all()
    up, lo = rgb[canon & (meta[:, 2] == 1)], rgb[canon & (meta[:, 2] == 0)]
    assert len(up) == len(lo) == 3 * 255
    for u, l in zip(up, lo):
        assert oracle.subsample_block(u.reshape(-1).tolist(), *pair)[4:] != oracle.subsample_block(l.reshape(-1).tolist(), *pair)[4:]
    if reference is not None:
        assert np.array_equal(avg, np.array([reference.average_bytes(b.reshape(-1).tolist(), *pair) for b in rgb]))


def test_flat_blocks_average_to_their_own_byte_for_equal_gammas(oracle):
    """What the every-colour picture reaches: for the pairs with equal gammas from_linear(to_linear(b)) == b, so flat blocks
    feed all 2^24 averaged triples into the Cb / Cr arithmetic; the mixed pairs reach 242 (sRGB -> Apple) and 183
    (sRGB -> Linear) averaged bytes per channel."""
    reach = {}
    for pair in PAIRS:
        got = [oracle.average_bytes([b] * 12, *pair)[0] for b in range(256)]
        reach[pair] = len(set(got))
        if pair[0] == pair[1]:
            assert got == list(range(256)), pair
    assert reach[(GAMMA_SRGB, GAMMA_APPLE)] == 242 and reach[(GAMMA_SRGB, GAMMA_LINEAR)] == 183


def test_launch_table_is_in_the_regimes_it_names(tmp_path):
    """The case table of the shipped launches against the launcher's rules, without a GPU: each row's hand-stated plan
    (tiles x lanes, row pairs per workgroup, groups, banded, launches, kernel) equals ec.expected_plan(), and the two header
    functions that plan rests on (bt709_kernels.h encode_block_threads / encode_row_pairs_per_block and its constants),
    compiled here, equal their restatement over a sweep of geometries -- so a change of the launcher's rules fails here
    instead of silently moving a case into another regime."""
    for case in ec.CASES:
        assert ec.plan_as_expect(ec.case_plan(case)) == case.expect, case
    # the regimes the table is for are all present
    plans = [ec.case_plan(c) for c in ec.CASES]
    assert {p["row_pairs"] for p in plans} >= {1, 3, 5, 9}
    assert any(p["launches"] == 2 and p["row_pairs"] != p["tail"]["row_pairs"] for p in plans)
    assert any(p["xcd_bands"] and p["grid"][0] == 16 for p in plans) and any(p["block"] == 512 and p["grid"][0] == 2 for p in plans)
    assert any(c.n == ec.MAX_BATCH and c.spacing == "table" for c in ec.CASES)
    src = tmp_path / "plan_probe.cpp"
    src.write_text('#include "bt709_kernels.h"\nextern "C" {\n'
                   "unsigned probe_threads(unsigned w) { return bt709::encode_block_threads(w); }\n"
                   "unsigned probe_row_pairs(unsigned w, unsigned h, unsigned n) { return bt709::encode_row_pairs_per_block(w, h, n); }\n"
                   "int probe_constant(int i) { const int v[] = {bt709::kMaxBlockThreads, bt709::kBlockThreads, bt709::kXcdBandMinFrames,\n"
                   "                                             bt709::kMaxBatch}; return v[i]; }\n}\n")
    so = str(tmp_path / "libplan_probe.so")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", os.path.join(HERE, "native", "fake_hip"), "-I", CSRC,
                        str(src), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(so)
    assert [lib.probe_constant(i) for i in range(4)] == [ec.MAX_BLOCK_THREADS, ec.GENERAL_THREADS, ec.XCD_BAND_MIN_FRAMES, ec.MAX_BATCH]
    assert ec.MAX_BATCH == _capi.MAX_BATCH
    rng = np.random.default_rng(3)
    geoms = [(c.w, c.h, c.n) for c in ec.CASES] + [(4 * q, 2 * int(rng.integers(1, 1100)), int(rng.integers(1, 3000)))
                                                   for q in list(range(1, 40)) + [319, 320, 321, 639, 640, 641, 959, 960, 961, 1280, 2048, 2049]]
    for w, h, n in geoms:
        assert lib.probe_threads(w) == ec.encode_block_threads(w), w
        assert lib.probe_row_pairs(w, h, n) == ec.encode_row_pairs_per_block(w, h, n), (w, h, n)


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


def gpu_encode(gh, bgra_words, w, h, in_gamma, out_gamma, stride=None, y_stride=None, c_stride=None):
    ctx = gh.context()
    tex = ctx.makeBGRATexture((w, h), pixels=bgra_words, stride=stride)
    buf = mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (w, h), y_stride, c_stride)
    ok = mb.BGRAToBT709Converter.convertIntoCoreVideoBuffer(tex, buf, in_gamma, out_gamma)
    return buf.download_planes() if ok else None


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("size", [(2, 2), (4, 2), (6, 4), (64, 16), (250, 6), (1920, 64)])
def test_gpu_encoder_matches_oracle(gh, oracle, pair, size):
    w, h = size
    rng = np.random.default_rng(w * 7 + h + pair[0] * 3 + pair[1])
    bgra = rng.integers(0, 1 << 32, w * h, dtype=np.uint32)
    got = gpu_encode(gh, bgra, w, h, *pair)
    assert got is not None
    want = oracle.encode_nv12(bgra & 0xFFFFFF, w, h, *pair)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.gpu
def test_gpu_encoder_general_layout(gh, oracle):
    """Odd strides / width % 4 != 0 take the scalar kernel; same bytes."""
    w, h = 18, 6
    bgra = np.random.default_rng(5).integers(0, 1 << 24, w * h, dtype=np.uint32)
    got = gpu_encode(gh, bgra, w, h, GAMMA_SRGB, GAMMA_APPLE, y_stride=19, c_stride=21)
    want = oracle.encode_nv12(bgra, w, h, GAMMA_SRGB, GAMMA_APPLE)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert "blocks" in mb.load_library().bt709hip_last_kernel_name().decode()


@pytest.mark.gpu
def test_gpu_encoder_reference_blocks(gh, refdata):
    """The reference-produced BT709_average_pixel_values vectors, through the GPU."""
    for b in refdata["subsample_blocks"]:
        rgb = b["rgb"]
        words = np.array([(rgb[3 * i] << 16) | (rgb[3 * i + 1] << 8) | rgb[3 * i + 2] for i in range(4)], np.uint32)
        y, c = gpu_encode(gh, words, 2, 2, b["in"], b["out"])
        assert [int(y[0, 0]), int(y[0, 1]), int(y[1, 0]), int(y[1, 1]), int(c[0, 0]), int(c[0, 1])] == b["y4cbcr"]


@pytest.mark.gpu
def test_gpu_encoder_xctest_average_of_4_vectors(gh, vectors):
    """The reference's own asserted 2x2-averaging numbers (CoreImageMetalFilterTests.m:1683-2096), through the GPU encoder."""
    for b in vectors["average_blocks"]:
        rgb = b["rgb"]
        words = np.array([(rgb[3 * i] << 16) | (rgb[3 * i + 1] << 8) | rgb[3 * i + 2] for i in range(4)], np.uint32)
        y, c = gpu_encode(gh, words, 2, 2, b["in"], b["out"])
        assert [int(y[0, 0]), int(y[0, 1]), int(y[1, 0]), int(y[1, 1]), int(c[0, 0]), int(c[0, 1])] == b["y4cbcr"], b["test"]


@pytest.mark.gpu
def test_gpu_encoder_all_grey_levels_and_primaries(gh, oracle):
    cols = [(v, v, v) for v in range(256)] + [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255),
                                              (255, 0, 255)]
    w, h = 2 * len(cols), 2
    bgra = np.zeros((h, w), np.uint32)
    for i, (r, g, b) in enumerate(cols):
        bgra[:, 2 * i:2 * i + 2] = (r << 16) | (g << 8) | b
    for pair in PAIRS:
        got = gpu_encode(gh, bgra.reshape(-1), w, h, *pair)
        want = oracle.encode_nv12(bgra.reshape(-1), w, h, *pair)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.gpu
def test_gpu_round_trip_on_device(gh, oracle):
    """Encode then decode without leaving the GPU: flat 2x2 blocks of sampled colours come
    back within the error the reference's exhaustive Apple196 round trip allows (max
    channel error 2: CoreImageMetalFilterTests.m:676-691) and equal the oracle's round trip."""
    ctx = gh.context()
    rng = np.random.default_rng(42)
    n = 4096
    cols = rng.integers(0, 256, (n, 3))
    w, h = 2 * n, 2
    bgra = np.zeros((h, w), np.uint32)
    words = (cols[:, 0].astype(np.uint32) << 16) | (cols[:, 1].astype(np.uint32) << 8) | cols[:, 2].astype(np.uint32)
    bgra[:, 0::2] = words
    bgra[:, 1::2] = words
    tex = ctx.makeBGRATexture((w, h), pixels=bgra.reshape(-1))
    buf = mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (w, h))
    mb.BGRAToBT709Converter.setBT709Attributes(buf)
    assert mb.BGRAToBT709Converter.convertIntoCoreVideoBuffer(tex, buf, mb.MetalBT709GammaSRGB, mb.MetalBT709GammaApple)
    out = ctx.makeBGRATexture((w, h))
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    assert dec.decodeBT709(buf, None, out, None, None, w, h, True)
    px = ctx.getBGRATexturePixels(out)
    got = np.stack([(px[0, 0::2] >> 16) & 0xFF, (px[0, 0::2] >> 8) & 0xFF, px[0, 0::2] & 0xFF], axis=1).astype(int)
    # the subsample path quantises to gamma-encoded bytes before the matrix, so it is a little
    # lossier than the per-pixel encoder's exhaustive bound of 2 (CoreImageMetalFilterTests.m:676-691)
    assert np.abs(got - cols).max() <= 4
    for i in range(0, n, 16):
        y4cbcr = oracle.subsample_block([int(v) for v in cols[i]] * 4, GAMMA_SRGB, GAMMA_APPLE)
        assert tuple(got[i]) == oracle.decode_pixel(GAMMA_APPLE, y4cbcr[0], y4cbcr[4], y4cbcr[5])


@pytest.mark.gpu
def test_constant_division_shortcut_is_exact_for_every_float(gh, tmp_path):
    """The encoder divides by 1.8556f / 1.5748f as q0 = x*rc, q = fma(fma(-c,q0,x), rc, q0).
    tools/div_exact.hip compares that with __fdiv_rn for all 2^32 float bit patterns; it must
    report zero mismatches for 1e-30 <= |x| <= 4 (the encoder's operands are within [-1.1, 1.1])."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "div_exact")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17",
                        os.path.join(root, "tools", "div_exact.hip"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    lines = [l for l in out.splitlines() if l.startswith("c=")]
    assert len(lines) == 2, out
    for l in lines:
        assert l.rstrip().endswith("<=4: 0"), l


@pytest.mark.gpu
def test_gpu_encoder_errors(gh):
    ctx = gh.context()
    tex = ctx.makeBGRATexture((8, 4))
    assert not mb.BGRAToBT709Converter.convertIntoCoreVideoBuffer(tex, mb.CVPixelBuffer(ctx, 8, 6), 1, 0)
    assert not mb.BGRAToBT709Converter.convertIntoCoreVideoBuffer(tex, mb.CVPixelBuffer(ctx, 8, 4), 3, 0)  # ITU: not an encoder gamma
    odd = ctx.makeBGRATexture((7, 4))
    assert not mb.BGRAToBT709Converter.convertIntoCoreVideoBuffer(odd, mb.CVPixelBuffer(ctx, 7, 4), 1, 0)
    assert mb.BGRAToBT709Converter.convertIntoCoreVideoBuffer(ctx.makeBGRATexture((0, 0)), mb.CVPixelBuffer(ctx, 0, 0), 1, 0)


@pytest.mark.gpu
def test_gpu_encoder_batch_matches_single(gh, oracle):
    """bt709hip_encode_batch: separately allocated pictures (pointer table) and a ring carved
    from one allocation (evenly spaced, beyond the table limit) give the single-call bytes."""
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = gh.context()
    w, h = 64, 12
    rng = np.random.default_rng(41)
    # pointer table
    pics = [rng.integers(0, 1 << 32, w * h, dtype=np.uint32) for _ in range(5)]
    texs = [ctx.makeBGRATexture((w, h), pixels=p) for p in pics]
    bufs = [mb.BGRAToBT709Converter.createCoreVideoYCbCrBuffer(ctx, (w, h)) for _ in pics]
    assert mb.BGRAToBT709Converter.convertIntoCoreVideoBuffers(texs, bufs, 1, 0)
    for p, b in zip(pics, bufs):
        want = oracle.encode_nv12(p & 0xFFFFFF, w, h, 1, 0)
        got = b.download_planes()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # evenly spaced ring, more pictures than BT709HIP_MAX_BATCH
    n = _capi.MAX_BATCH + 9
    in_pitch, out_pitch = w * h * 4, w * h * 3 // 2
    slab_in, slab_out = DeviceBuffer(ctx, n * in_pitch), DeviceBuffer(ctx, n * out_pitch)
    pics = [rng.integers(0, 1 << 32, w * h, dtype=np.uint32) for _ in range(n)]
    texs, bufs = [], []
    for i, p in enumerate(pics):
        t = mb.BGRATexture(ctx, w, h, w * 4, ptr=slab_in.ptr + i * in_pitch)
        ctx.fillBGRATexture(t, p)
        texs.append(t)
        base = slab_out.ptr + i * out_pitch
        bufs.append(mb.CVPixelBuffer(ctx, w, h, w, w, planes=(base, base + w * h)))
    assert mb.BGRAToBT709Converter.convertIntoCoreVideoBuffers(texs, bufs, 1, 0)
    for p, b in zip(pics, bufs):
        want = oracle.encode_nv12(p & 0xFFFFFF, w, h, 1, 0)
        got = b.download_planes()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # 64 pictures (a multiple of 8, at the threshold): the XCD-aware work map; 70: 64 under the map + 6 plain; same bytes as the plain order
    for bands, n64 in ((1, 64), (0, 64), (1, 70)):
        _capi.check(ctx.lib.bt709hip_context_set_option(ctx.handle, _capi.CTX_OPT_XCD_BANDS, bands))
        s_in, s_out = DeviceBuffer(ctx, n64 * in_pitch), DeviceBuffer(ctx, n64 * out_pitch)
        pics64 = [rng.integers(0, 1 << 32, w * h, dtype=np.uint32) for _ in range(n64)]
        t64, b64 = [], []
        for i, p in enumerate(pics64):
            t = mb.BGRATexture(ctx, w, h, w * 4, ptr=s_in.ptr + i * in_pitch)
            ctx.fillBGRATexture(t, p)
            t64.append(t)
            base = s_out.ptr + i * out_pitch
            b64.append(mb.CVPixelBuffer(ctx, w, h, w, w, planes=(base, base + w * h)))
        assert mb.BGRAToBT709Converter.convertIntoCoreVideoBuffers(t64, b64, 1, 0)
        for p, b in zip(pics64, b64):
            want = oracle.encode_nv12(p & 0xFFFFFF, w, h, 1, 0)
            got = b.download_planes()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), bands
    _capi.check(ctx.lib.bt709hip_context_set_option(ctx.handle, _capi.CTX_OPT_XCD_BANDS, 1))
    # shuffled: not evenly spaced any more -> the table limit applies; mixed sizes are refused
    order = list(range(n))
    order[2], order[5] = order[5], order[2]
    assert not mb.BGRAToBT709Converter.convertIntoCoreVideoBuffers([texs[i] for i in order], [bufs[i] for i in order], 1, 0)
    other = ctx.makeBGRATexture((w, h + 2))
    assert not mb.BGRAToBT709Converter.convertIntoCoreVideoBuffers(
        [texs[0], other], [bufs[0], mb.CVPixelBuffer(ctx, w, h + 2)], 1, 0)


# ------------------------------------------------------------------ GPU: the sweeps of tests/encoder_cases.py

@pytest.fixture(scope="module")
def harness(gh):
    return ec.Harness(gh)


def single_layout(w, h, strides=None):
    sb, sy, sc = strides or (4 * w, w, w)
    return ec.Layout(w, h, (sb, sy, sc), [ec.GUARD], [ec.GUARD], [ec.GUARD])


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_gpu_encoder_every_colour(harness, oracle, pair):
    """EVERY (R,G,B) once as a flat 2x2 block (2^24 blocks, 8192 x 8192, in 8 strips of 8192 x 1024), random alpha bytes:
    Y and CbCr planes equal the oracle's.  This covers every entry of the per-byte {lin, enc_norm} table in every channel
    position; for every triple the Y matrix, quant_arg and the truncation under the switched rounding mode (all 209 Y ties);
    and, because from_linear(to_linear(b)) == b for the pairs with equal gammas
    (test_flat_blocks_average_to_their_own_byte_for_equal_gammas), for (sRGB, sRGB), (Linear, Linear) and (Apple, Apple) all
    2^24 averaged triples through div_const and the Cb / Cr quantiser (all 193 / 283 ties).  The mixed pairs reach fewer
    averaged bytes from flat blocks (242 for sRGB -> Apple, 183 for sRGB -> Linear): expected."""
    side, strips = ec.ALL_COLOURS_SIDE, ec.ALL_COLOURS_STRIPS
    rows = side // strips
    L = single_layout(side, rows)
    bad = []
    for strip in range(strips):
        words = ec.all_colours_strip(strip, seed=1000 * pair[0] + 10 * pair[1] + strip)
        res = harness.encode(L, ec.fill_input(L, lambda i: words), pair)
        assert res.kernel == "encode_bgra_nv12"
        wy, wc = ec.threaded_encode(oracle, words, side, rows, *pair)
        want_y, want_c = ec.expected_slabs(L, lambda i: (wy, wc))
        for plane, got, want in (("y", res.y_slab, want_y), ("cbcr", res.c_slab, want_c)):
            d = ec.describe_difference(L, got, want, plane)
            if d:
                bad.append("strip %d (colours 0x%06x..): %s" % (strip, strip << 21, d))
    assert not bad, "\n".join(bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_gpu_encoder_on_and_beside_every_threshold(harness, oracle, edge_sets, pair):
    """The blocks of ec.edge_blocks -- per channel and threshold an average exactly on (or the first one above) the
    threshold and the last one below it, the other two channels chosen so that the flip shows in Cb / Cr, each in the 12
    summation orders -- in one picture, every block once in each half of a quad, through the aligned kernel (tight strides)
    and the general one (odd luma stride): planes equal the oracle's."""
    eb = edge_sets(pair)
    pic = ec.edge_picture(eb)
    h, w = pic.shape
    wy, wc = oracle.encode_nv12(pic, w, h, *pair)
    for strides, kernel in (((4 * w, w, w), "encode_bgra_nv12"), ((4 * w, w + 1, w), "encode_bgra_nv12_blocks")):
        L = single_layout(w, h, strides)
        res = harness.encode(L, ec.fill_input(L, lambda i: pic), pair)
        assert res.kernel == kernel
        want_y, want_c = ec.expected_slabs(L, lambda i: (wy, wc))
        diffs = [d for d in (ec.describe_difference(L, res.y_slab, want_y, "y"), ec.describe_difference(L, res.c_slab, want_c, "cbcr")) if d]
        if diffs:  # name the blocks: (channel, threshold, upper / lower, order)
            got_c = ec._rows_view(res.c_slab, L.c_off[0], h // 2, L.sc, w)
            rp, col = np.nonzero(got_c != wc)
            idx = sorted({ec.edge_block_at(eb, int(r), int(c)) for r, c in zip(rp, col)} - {None})
            diffs.append("blocks (channel, k, upper, order, exact): %s" % [tuple(int(v) for v in eb.meta[i]) for i in idx[:12]])
        assert not diffs, "%s: %s" % (kernel, "\n".join(diffs))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ec.CASES, ids=repr)
def test_gpu_encoder_shipped_launches(harness, oracle, case):
    """The launch regimes the encoder ships with, default context options, one bt709hip_encode_batch call each: every picture
    of every case equals the oracle (slots differ from each other in three row pairs), the padding between rows, the gaps
    between pictures and the guard bands around the planes keep their 0x5A fill, and the launch on record
    (bt709hip_last_launch_info, bt709hip_last_kernel_name) is the plan the table states for the row."""
    res, diffs = ec.run_case(harness, oracle, case, seed=len(case.name) * 7 + case.w)
    got = ec.recorded_expect(res, case)
    want = case.expect
    plan = ec.case_plan(case)
    assert ec.plan_as_expect(plan) == want
    assert (res.grid, res.block, res.launches, res.xcd_bands, res.kernel) == (
        tuple(plan["grid"]), (plan["block"], 1, 1), plan["launches"], plan["xcd_bands"], plan["kernel"]), (got, want)
    assert want["row_pairs"] in got["row_pairs_candidates"] or want["kernel"].endswith("blocks")
    assert not diffs, "\n".join(diffs)


@pytest.mark.gpu
def test_gpu_encoder_fuzzed_geometry(harness, oracle):
    """The encoder's twin of test_fuzzed_geometry: seeded cases of any even width and height (widths around and across 4,
    256, 1280 and 2048 quads included), any bgra_stride >= 4 W that is a multiple of 4, any y_stride, cbcr_stride >= W,
    base pointers at any allowed alignment (BGRA 4, planes 1), all five pairs, single pictures and small batches, evenly
    spaced or not.  The fast-path predicate is stated here (ec.fast_path: width % 4, bgra_stride % 16, plane strides % 4,
    bases 16 / 4 / 4) and bt709hip_last_kernel_name must agree with it, the recorded launch with ec.expected_plan; bytes equal
    the oracle; padding and guard bands untouched."""
    bad, kernels = [], {}
    for i in range(ec.FUZZ_CASES):
        L, pair, pics = ec.fuzz_case(i)
        res = harness.encode(L, ec.fill_input(L, lambda k: pics[k]), pair)
        fast = ec.fast_path(L.w, L.sb, L.sy, L.sc, L.in_off, L.y_off, L.c_off)
        plan = ec.expected_plan(L.w, L.h, L.n, fast=fast, uniform=ec.layout_is_uniform(L))
        what = "case %d: %dx%d x %d, strides %d/%d/%d, pair %s" % (i, L.w, L.h, L.n, L.sb, L.sy, L.sc, pair)
        if (res.kernel, res.grid, res.block[0], res.launches, res.xcd_bands) != (
                plan["kernel"], tuple(plan["grid"]), plan["block"], plan["launches"], plan["xcd_bands"]):
            bad.append("%s: launched %s %s x %s, expected %s" % (what, res.kernel, res.grid, res.block, plan))
        kernels[res.kernel] = kernels.get(res.kernel, 0) + 1
        want = [oracle.encode_nv12(p & 0xFFFFFF, L.w, L.h, *pair) for p in pics]
        want_y, want_c = ec.expected_slabs(L, lambda k: want[k])
        for plane, g, w_ in (("y", res.y_slab, want_y), ("cbcr", res.c_slab, want_c)):
            d = ec.describe_difference(L, g, w_, plane)
            if d:
                bad.append("%s: %s" % (what, d))
    assert not bad, "\n".join(bad[:10])
    assert min(kernels.get("encode_bgra_nv12", 0), kernels.get("encode_bgra_nv12_blocks", 0)) >= ec.FUZZ_CASES // 8, kernels
