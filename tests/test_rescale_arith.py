"""Arithmetic parity of the fused decode + rescale family (bt709_rescale_half.hip, bt709_rescale_scaled.hip, the lookups of
bt709_rescale.h) where a piecewise-constant lookup can be wrong: next to its breakpoints.

  1. every (Y,Cb,Cr) through the decode-side lookup: all 2^24 triples as flat 2x2 blocks through both 2:1 kernels and the
     any-ratio kernel at exactly 2:1 (`wide`), against the oracle's 1:1 table; a 131 072-block slice through `pairs`, `bytes`,
     `shared` and `once`, against the oracle's rescale of the whole frame;
  2. both sides of every encode threshold: blocks whose four-tap sum IS a threshold of quantize(linear_to_srgb(.)) and the float
     just below it, in all 24 tap orders at both output-column parities, through both 2:1 kernels, the any-ratio kernel and
     pass 2 alone;
  3. the persistent 2:1 kernel's launches nothing else visits: every LDS budget (every pair of replication factors, and the
     fallback), cursor steps with all three components non-zero, the ring past the pointer table -- the plan asserted from
     bt709hip_last_launch_info.

Every expected byte is the oracle's.  The unmarked tests guard the generators on the CPU (rescale_arith_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi

import rescale_arith_cases as rc

GAMMAS = (0, 1, 2, 3)
# the counts a deliberately narrow search reached when these tests were specified; a fuller search can only find more
FREE_BYTE_HITS = (180, 172)                             # thresholds hit exactly, hit one float below
NV12_BOTH_SIDES = {0: 162, 1: 165, 2: 126, 3: 162}      # R channel, grey chroma: thresholds hit on both sides


# ------------------------------------------------------------------ CPU guards

_edge_memo = {}


def _nv12_edge_frame(oracle, gamma):
    if ("nv12", gamma) not in _edge_memo:
        ef, y, c = rc.nv12_edge_frame(oracle, gamma)
        _edge_memo["nv12", gamma] = (ef, y, c, oracle.decode_nv12_half(gamma, y, c))
    return _edge_memo["nv12", gamma]


def _bgra_edge_frame(oracle):
    if "bgra" not in _edge_memo:
        ef, src = rc.bgra_edge_frame(oracle)
        _edge_memo["bgra"] = (ef, src, oracle.render_scaled(src, ef.COLS, ef.rows))
    return _edge_memo["bgra"]


def test_encode_of_a_linearised_byte_is_the_byte(oracle):
    """quantize(linear_to_srgb(lin[b])) == b for every byte: with (4 lin) * 0.25f exact, a flat block's 2:1 rescale is its decode."""
    lin, T = rc.encode_tables(oracle)
    assert [oracle.transfer_to_byte(rc.GAMMA_LINEAR, float(v)) for v in lin] == list(range(256))
    assert np.array_equal(np.searchsorted(T, lin, side="right"), np.arange(256))  # the same through the threshold table
    four = (lin * np.float32(4.0)).astype(np.float32)
    assert np.array_equal(rc.tap_sum(lin, np.repeat(np.arange(256)[:, None], 4, axis=1)), lin) and np.array_equal(four * np.float32(0.25), lin)


@pytest.mark.parametrize("gamma", GAMMAS)
def test_flat_blocks_rescale_to_their_decode(oracle, gamma):
    """The identity the full sweep leans on, through the oracle itself: on 2^16 seeded triples and one triple per channel and
    output byte, decode_nv12_half of flat blocks is the 1:1 table entry, and decode_nv12_scaled at 2:1 is decode_nv12_half."""
    Y, Cb, Cr, table = rc.sample_blocks(oracle, gamma, seed=1709 + gamma)
    assert Y.size >= (1 << 16) + 3 * 256 - 3
    want = rc.table_image(table, Y, Cb, Cr)
    for ch in range(3):
        assert np.unique(want.reshape(-1, 4)[:, ch]).size == np.unique(table[:, 2 - ch]).size  # every output byte of the channel
    y, c = rc.flat_frame(Y, Cb, Cr)
    half = oracle.decode_nv12_half(gamma, y, c)
    assert np.array_equal(half, want)
    assert np.array_equal(oracle.decode_nv12(gamma, y, c).reshape(y.shape[0], y.shape[1], 4)[::2, ::2].reshape(want.shape), want)
    assert np.array_equal(oracle.decode_nv12_scaled(gamma, y, c, Y.shape[1], Y.shape[0]), half)


def test_sweep_frames_hold_what_they_claim():
    import gpu_helpers  # numpy only until context() is called
    Y, Cb, Cr = rc.reduced_sweep_blocks()
    t = (Y.astype(np.uint32) << 16 | Cb.astype(np.uint32) << 8 | Cr).reshape(-1)
    assert Y.shape == (256, 512) and np.unique(t).size == 131072 - 256  # (Y, 128, 128) sits in both halves
    for y in (0, 77, 255):  # per luma value: every Cr beside a grey Cb (all R inputs), every Cb beside a grey Cr (all B inputs)
        row = t[t >> 16 == y]
        assert np.unique(row[(row >> 8 & 255) == 128] & 255).size == 256 and np.unique(row[(row & 255) == 128] >> 8 & 255).size == 256
    y, c = rc.flat_frame(Y, Cb, Cr)
    assert y.shape == (512, 1024) and c.shape == (256, 1024)
    # the full frame: every triple once, as blocks (checked on a strip; the whole is the same np.repeat)
    ey, ec = gpu_helpers.exhaustive_frame()
    By, Bcb, Bcr = rc.blocks_of(ey, ec)
    idx = (By.astype(np.uint32) << 16) | (Bcb.astype(np.uint32) << 8) | Bcr
    assert idx.shape == (4096, 4096) and np.unique(idx).size == 1 << 24
    fy, fc = rc.flat_frame(By[:8], Bcb[:8], Bcr[:8])
    assert fy.shape == (16, 8192) and (fy[0::2, 0::2] == By[:8]).all() and (fy[1::2, 1::2] == By[:8]).all() and (fc[:, 1::2] == Bcr[:8]).all()


def test_free_byte_quadruples_reach_the_thresholds(oracle):
    e = rc.free_byte_edges(oracle)
    on, below, both = rc.edge_counts(e)
    print("free bytes: %d thresholds hit exactly, %d one float below, %d on both sides; worst gap above %d ulp, below %d ulp (T[0]: %d)"
          % (on, below, both, e["up_ulps"].max(), e["lo_ulps"][1:].max(), e["lo_ulps"][0]))
    assert on >= FREE_BYTE_HITS[0] and below >= FREE_BYTE_HITS[1]
    assert e["have_upper"].all() and e["have_lower"].all()
    ef, src, want = _bgra_edge_frame(oracle)
    exact, probes = rc.check_probes_against(ef, want)
    assert probes == 3 * 2 * 2 * 255 * 24 and src.shape == (2 * ef.rows, 8 * ef.COLS) and ef.rows % 2 == 0


@pytest.mark.parametrize("gamma", GAMMAS)
def test_nv12_quadruples_reach_the_thresholds(oracle, gamma):
    ef, y, c, want = _nv12_edge_frame(oracle, gamma)
    e = ef.edges
    on, below, both = rc.edge_counts(e)
    print("gamma %d: %d thresholds hit exactly, %d one float below, %d on both sides; worst gap above %d ulp, below %d ulp (T[0]: %d)"
          % (gamma, on, below, both, e["up_ulps"].max(), e["lo_ulps"][1:].max(), e["lo_ulps"][0]))
    assert both >= NV12_BOTH_SIDES[gamma]
    assert e["have_upper"].all() and e["have_lower"].all()
    # the R bytes the search used are the ones the luma bytes of the frame decode to
    for side in ("upper", "lower"):
        for i in (0, 100, 254):
            assert [oracle.decode_pixel(gamma, int(v), 128, int(e["cr_" + side][i]))[0] for v in e["y_" + side][i]] == list(e[side][i])
    exact, probes = rc.check_probes_against(ef, want)
    assert probes == 2 * 2 * 255 * 24 and y.shape == (2 * ef.rows, 2 * ef.COLS) and y.shape[0] % 4 == 0 and y.shape[1] % 4 == 0
    # both output-column parities of every probe
    meta = ef.meta.reshape(ef.rows, ef.COLS, 3, 4)[:, :, 2]
    for parity in (0, 1):
        m = meta[:, parity::2]
        assert np.unique(m[m[..., 0] >= 0][:, [0, 2]], axis=0).shape[0] == 255 * 24


def test_half_rep_cases_reach_what_they_name(oracle):
    """The cursor step of each case from the launcher's documented decomposition, and the budgets' replication factors."""
    for name, (w, h), frames, wg, tiles_x, tile_rows, cursor in rc.CURSOR_CASES:
        plan = rc.half_rep_plan(w, h, frames, wg)
        assert (plan["tiles_x"], plan["tile_rows"], plan["cursor"], plan["grid"]) == (tiles_x, tile_rows, cursor, (wg, 1, 1)), name
        assert w % 4 == 0 and h % 4 == 0 and tile_rows > 2 * wg  # every workgroup goes past its first step of two tile rows
        if name in ("A", "B"):
            assert all(cursor), name
        else:
            assert frames > _capi.MAX_BATCH and cursor[1] and cursor[2], name
    enc = rc.uniform_encode_bytes(oracle)
    assert 16 * 1024 < enc < 32 * 1024 and enc % 16 == 0
    seen = {g: [rc.rep_copies(rc.UNIFORM_BUCKETS[g], enc, kb) for kb in rc.LDS_BUDGETS_KB] for g in GAMMAS}
    print("uniform encode table: %d bytes; copies per gamma and budget: %r" % (enc, seen))
    pairs = {p for row in seen.values() for p in row}
    assert None in pairs and {p[0] for p in pairs if p} == {0, 1, 2, 3, 4} and {p[1] for p in pairs if p} >= {0, 1}
    assert all(row[-1] is not None for row in seen.values())  # the default budget holds every gamma's tables


def test_uniform_bucket_counts_are_the_librarys():
    lib = _capi.load()
    for g in GAMMAS:
        n = C.c_int()
        assert lib.bt709hip_gamma_lookup(g, 0.5, C.byref(n), None) >= 0 and n.value == rc.UNIFORM_BUCKETS[g]


# ------------------------------------------------------------------ GPU plumbing

@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


def _round_up(v, a):
    return (v + a - 1) // a * a


class DeviceFrame:
    """One NV12 frame in device memory in a chosen layout (tests/test_rescale.py's names): "aligned" -- plane addresses and
    pitches multiples of 4; "even" -- 2-byte aligned and no more; "odd" -- odd pitches and odd plane addresses."""

    def __init__(self, gh, y, c, layout="aligned"):
        from metalbt709decoder_amd.decoder import DeviceBuffer
        self.gh, self.ctx = gh, gh.context()
        self.h, self.w = y.shape
        self.ys, self.cs, y_off, c_off = {"aligned": (_round_up(self.w, 4), _round_up(self.w, 4), 0, 0),
                                          "even": (self.w + 2, self.w + 6, 2, 6),
                                          "odd": (self.w + 1, self.w + 3, 1, 3)}[layout]
        self.by = DeviceBuffer(self.ctx, self.ys * self.h + 64)
        self.bc = DeviceBuffer(self.ctx, self.cs * (self.h // 2) + 64)
        self.y_ptr, self.c_ptr = self.by.ptr + y_off, self.bc.ptr + c_off
        self.ctx._upload(self.y_ptr, self.ys, np.ascontiguousarray(y), None)
        self.ctx._upload(self.c_ptr, self.cs, np.ascontiguousarray(c), None)

    def frame(self, gamma):
        b = mb.CVPixelBuffer(self.ctx, self.w, self.h, self.ys, self.cs, planes=(self.y_ptr, self.c_ptr))
        b.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
        b.setAttachment("TransferFunction", self.gh.TRANSFER_FOR_GAMMA[gamma])
        return b.frame()


class Target:
    """A (ow, oh) BGRA8 view inside a 0x5A-filled allocation: padded rows, a guard band in front and behind."""

    GUARD = 256

    def __init__(self, ctx, ow, oh, pad=16):
        from metalbt709decoder_amd.decoder import DeviceBuffer
        self.ctx, self.ow, self.oh, self.stride = ctx, ow, oh, 4 * ow + pad
        self.nbytes = 2 * self.GUARD + self.stride * oh
        self.buf = DeviceBuffer(ctx, self.nbytes)
        _capi.check(ctx.lib.bt709hip_memset(ctx.handle, self.buf.ptr, rc.FILL, self.nbytes, None))
        ctx._sync(None)
        self.tex = mb.BGRATexture(ctx, ow, oh, self.stride, ptr=self.buf.ptr + self.GUARD)

    def read(self):
        """-> the view's bytes (oh, 4 ow); asserts that everything else still holds the fill."""
        raw = np.empty(self.nbytes, np.uint8)
        _capi.check(self.ctx.lib.bt709hip_download(self.ctx.handle, raw.ctypes.data, self.nbytes, self.buf.ptr, self.nbytes, self.nbytes, 1, None))
        self.ctx._sync(None)
        rows = raw[self.GUARD:self.GUARD + self.stride * self.oh].reshape(self.oh, self.stride)
        assert (raw[:self.GUARD] == rc.FILL).all() and (raw[self.GUARD + self.stride * self.oh:] == rc.FILL).all(), "bytes written outside the output rows"
        assert (rows[:, 4 * self.ow:] == rc.FILL).all(), "bytes written into the rows' padding"
        return rows[:, :4 * self.ow]


def _launch_record(ctx):
    info = _capi.LaunchInfo()
    _capi.check(ctx.lib.bt709hip_last_launch_info(C.byref(info)))
    return dict(grid=tuple(info.grid), block=tuple(info.block), launches=info.launches, xcd_bands=info.xcd_bands)


def _scaled_taps(ctx):
    info = _capi.ScaledLaunchInfo()
    _capi.check(ctx.lib.bt709hip_last_scaled_launch_info(C.byref(info)))
    return {_capi.SCALED_TAPS_BYTES: "bytes", _capi.SCALED_TAPS_PAIRS: "pairs", _capi.SCALED_TAPS_WIDE: "wide",
            _capi.SCALED_TAPS_SHARED: "shared", _capi.SCALED_TAPS_ONCE: "once"}[info.taps]


# route -> (C entry point, OPT_HALF_KERNEL, plane layout, kernel name, tap form, further decoder options)
ROUTES = {"half": ("bt709hip_decode_half", 0, "aligned", b"decode_nv12_half<wide>", None, {}),
          "half-rep": ("bt709hip_decode_half", 1, "aligned", b"decode_nv12_half_rep", None, {}),
          # odd pitches and plane addresses: one output pixel per lane, 256 per workgroup
          "half-narrow": ("bt709hip_decode_half", None, "odd", b"decode_nv12_half<narrow>", None, {}),
          # the wide kernel with the default cache policy: the same name, so the option is read back
          "half-temporal": ("bt709hip_decode_half", 0, "aligned", b"decode_nv12_half<wide>", None, {_capi.OPT_NONTEMPORAL: 0}),
          "scaled-wide": ("bt709hip_decode_scaled", None, "aligned", b"decode_nv12_scaled", "wide", {}),
          "scaled-pairs": ("bt709hip_decode_scaled", None, "even", b"decode_nv12_scaled", "pairs", {}),
          "scaled-bytes": ("bt709hip_decode_scaled", None, "odd", b"decode_nv12_scaled", "bytes", {}),
          "scaled-shared": ("bt709hip_decode_scaled", None, "aligned", b"decode_nv12_scaled", "shared", {}),
          "scaled-once": ("bt709hip_decode_scaled", None, "aligned", b"decode_nv12_scaled", "once", {})}


def _run_route(gh, route, gamma, dev, ow, oh):
    """One frame through the route's C entry point (called directly: the Python wrapper reroutes an exact 2:1 to the 2:1 kernels);
    asserts the kernel, the tap form and the plan on record; -> the view's bytes."""
    entry, half_kernel, layout, name, taps, options = ROUTES[route]
    ctx = gh.context()
    options = dict(options)
    if half_kernel is not None:
        options[_capi.OPT_HALF_KERNEL] = half_kernel
    dec = gh.make_decoder(gamma, options=options)
    for opt, value in options.items():  # the options took: the kernel's name does not show every one
        have = C.c_int(-1)
        _capi.check(ctx.lib.bt709hip_decoder_get_option(dec._handle, opt, C.byref(have)))
        assert have.value == value, (route, opt, have.value)
    frame, target = dev.frame(gamma), Target(ctx, ow, oh)
    surf = target.tex.surface()
    _capi.check(getattr(ctx.lib, entry)(dec._handle, C.byref(frame), None, C.byref(surf), None, 1), route)
    assert ctx.lib.bt709hip_last_kernel_name() == name, (route, ctx.lib.bt709hip_last_kernel_name())
    if taps is not None:
        assert _scaled_taps(ctx) == taps, (route, _scaled_taps(ctx))
    else:
        record = _launch_record(ctx)
        assert record["launches"] == 1 and record["xcd_bands"] == 0, record
        if half_kernel:
            plan = rc.half_rep_plan(dev.w, dev.h, 1, ctx.info().compute_units)
            assert (record["grid"], record["block"]) == (plan["grid"], plan["block"]), (record, plan)
        else:
            assert record["grid"][2] == 1 and record["grid"][1] * record["block"][1] >= oh and record["block"][0] % 64 == 0, record
            if name.endswith(b"<narrow>"):  # 256 output pixels per workgroup, one output row per workgroup row
                assert (record["grid"], record["block"]) == (((ow + 255) // 256, oh, 1), (256, 1, 1)), record
    return target.read()


# ------------------------------------------------------------------ 1. every colour through the decode-side lookup

@pytest.fixture(scope="module")
def full_sweep(gh):
    """All 2^24 triples as flat blocks, 8192 x 8192, uploaded once per plane layout; the expected images are filled per gamma on first use."""
    Y, Cb, Cr = rc.blocks_of(*gh.exhaustive_frame())
    planes = rc.flat_frame(Y, Cb, Cr)
    return dict(dev={"aligned": DeviceFrame(gh, *planes)}, planes=planes, blocks=(Y, Cb, Cr), want={})


# the narrow 2:1 kernel in every gamma; the wide one with the default cache policy in one (its arithmetic is the wide kernel's)
FULL_SWEEP_CASES = [(r, g) for r in ("half", "half-rep", "scaled-wide", "half-narrow") for g in GAMMAS] + [("half-temporal", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("route,gamma", FULL_SWEEP_CASES, ids=["%s-%d" % c for c in FULL_SWEEP_CASES])
def test_gpu_every_colour_as_flat_blocks(gh, oracle, full_sweep, route, gamma):
    """linearise12 + encode_byte, the pipelined copy + the uniform table, linearise6: an exact 2:1 rescale of the flat-block
    frame is, block for block, the oracle's 1:1 table (test_flat_blocks_rescale_to_their_decode holds the identity)."""
    if gamma not in full_sweep["want"]:
        full_sweep["want"][gamma] = rc.table_image(oracle.decode_table(gamma), *full_sweep["blocks"])
    want = full_sweep["want"][gamma]
    layout = ROUTES[route][2]
    if layout not in full_sweep["dev"]:  # the narrow kernel's: uploaded once more, at odd pitches and addresses
        full_sweep["dev"][layout] = DeviceFrame(gh, *full_sweep["planes"], layout)
    got = _run_route(gh, route, gamma, full_sweep["dev"][layout], 4096, 4096)
    if not np.array_equal(got, want):
        r, b = np.argwhere(got != want)[0]
        Y, Cb, Cr = (int(a[r, b // 4]) for a in full_sweep["blocks"])
        raise AssertionError("%s, gamma %d: (Y, Cb, Cr) = (%d, %d, %d) channel %s: got %d, want %d; %d bytes differ"
                             % (route, gamma, Y, Cb, Cr, "BGRA"[b % 4], got[r, b], want[r, b], int((got != want).sum())))


@pytest.fixture(scope="module")
def reduced_sweep(gh):
    y, c = rc.flat_frame(*rc.reduced_sweep_blocks())
    return dict(y=y, c=c, dev={}, want={})


# form -> output size of the 1024 x 512 frame
REDUCED_FORMS = {"scaled-pairs": (512, 256), "scaled-bytes": (512, 256), "scaled-shared": (1024, 1024), "scaled-once": (2048, 1024)}
REDUCED_CASES = [("scaled-pairs", 0), ("scaled-bytes", 1), ("scaled-shared", 2)] + [("scaled-once", g) for g in GAMMAS]


@pytest.mark.gpu
@pytest.mark.parametrize("case", REDUCED_CASES, ids=["%s-gamma%d" % c for c in REDUCED_CASES])
def test_gpu_every_r_and_b_input_through_the_other_tap_forms(gh, oracle, reduced_sweep, case):
    """The forms the full frame does not reach: byte and 2-byte tap fetches at 2:1, the wave-fetches form (scale_x = 1, rows
    doubled) and the wave-decodes-once form (linearise3; 1:2 both ways), on the blocks (Y, 128, Cr) and (Y, Cb, 128)."""
    route, gamma = case
    ow, oh = REDUCED_FORMS[route]
    layout = ROUTES[route][2]
    if layout not in reduced_sweep["dev"]:
        reduced_sweep["dev"][layout] = DeviceFrame(gh, reduced_sweep["y"], reduced_sweep["c"], layout)
    if (gamma, ow, oh) not in reduced_sweep["want"]:
        reduced_sweep["want"][gamma, ow, oh] = oracle.decode_nv12_scaled(gamma, reduced_sweep["y"], reduced_sweep["c"], ow, oh)
    want = reduced_sweep["want"][gamma, ow, oh]
    got = _run_route(gh, route, gamma, reduced_sweep["dev"][layout], ow, oh)
    if not np.array_equal(got, want):
        r, b = np.argwhere(got != want)[0]
        raise AssertionError("%s, gamma %d: output row %d, column %d, channel %s: got %d, want %d; %d bytes differ"
                             % (route, gamma, r, b // 4, "BGRA"[b % 4], got[r, b], want[r, b], int((got != want).sum())))


# ------------------------------------------------------------------ 2. both sides of every encode threshold

@pytest.mark.gpu
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("route", ["half", "half-rep", "scaled-wide", "scaled-pairs", "scaled-bytes", "half-narrow", "half-temporal"])
def test_gpu_both_sides_of_every_encode_threshold(gh, oracle, route, gamma):
    """encode_byte (log buckets) and encode_load / encode_use (the uniform table, edges rescaled at staging): R sums on and one
    float below each of the 255 thresholds, every tap order, both halves of a lane's quad."""
    ef, y, c, want = _nv12_edge_frame(oracle, gamma)
    got = _run_route(gh, route, gamma, DeviceFrame(gh, y, c, ROUTES[route][2]), ef.COLS, ef.rows)
    assert np.array_equal(got, want), "%s, gamma %d: %s" % (route, gamma, rc.first_difference(ef, got, want))


@pytest.mark.gpu
def test_gpu_both_sides_of_every_encode_threshold_in_pass_2(gh, oracle):
    """render_scaled at exactly 2:1 from a BGRA8 intermediate: every weight is 1/4 and the channels are independent, so one texel
    carries three thresholds."""
    ef, src, want = _bgra_edge_frame(oracle)
    ctx = gh.context()
    scale = mb.MetalScaleRenderContext()
    assert scale.setupRenderPipelines(ctx)
    inter = ctx.makeBGRATexture((2 * ef.COLS, 2 * ef.rows), pixels=src)
    target = Target(ctx, ef.COLS, ef.rows)
    assert scale.renderScaled(ctx, target.tex, ef.COLS, ef.rows, None, None, inter, True), scale.lastStatus
    assert ctx.lib.bt709hip_last_kernel_name() == b"render_scaled<bgra8>"
    got = target.read()
    assert np.array_equal(got, want), "render_scaled: %s" % rc.first_difference(ef, got, want)


# ------------------------------------------------------------------ 3. the persistent 2:1 kernel's unvisited launches

@pytest.mark.gpu
@pytest.mark.parametrize("gamma", GAMMAS)
def test_gpu_half_rep_at_every_lds_budget(gh, oracle, gamma):
    """OPT_HALF_LDS_KB chooses the replication factors and with them every LDS address of the persistent kernel: 16 ... 160 KiB
    visits every pair the launcher can choose; where one copy of each table does not fit, the short-lived kernel must run."""
    ctx = gh.context()
    w, h = 1024, 64
    y, c = gh.random_nv12(w, h, seed=5709 + gamma)
    want = oracle.decode_nv12_half(gamma, y, c)
    dev = DeviceFrame(gh, y, c)
    n = C.c_int()
    assert ctx.lib.bt709hip_gamma_lookup(gamma, 0.5, C.byref(n), None) >= 0 and n.value == rc.UNIFORM_BUCKETS[gamma]
    dec = gh.make_decoder(gamma, options={_capi.OPT_HALF_KERNEL: 1, _capi.OPT_HALF_WORKGROUPS: 5})
    frame, enc = dev.frame(gamma), rc.uniform_encode_bytes(oracle)
    for kb in rc.LDS_BUDGETS_KB:
        dec.setOption(_capi.OPT_HALF_LDS_KB, kb)
        target = Target(ctx, w // 2, h // 2)
        surf = target.tex.surface()
        _capi.check(ctx.lib.bt709hip_decode_half(dec._handle, C.byref(frame), None, C.byref(surf), None, 1))
        copies = rc.rep_copies(n.value, enc, kb)
        name, record = ctx.lib.bt709hip_last_kernel_name(), _launch_record(ctx)
        assert name == (b"decode_nv12_half_rep" if copies else b"decode_nv12_half<wide>"), (gamma, kb, copies, name)
        if copies:
            assert (record["grid"], record["block"]) == ((5, 1, 1), (256, 1, 1)), (gamma, kb, record)
        got = target.read()
        assert np.array_equal(got, want), "gamma %d, %d KiB (copies 2^%r): %d bytes differ, first at %r" % (
            gamma, kb, copies, int((got != want).sum()), tuple(np.argwhere(got != want)[0]))


CURSOR_RUNS = [("A", False, 1), ("B", False, 1), ("C", False, 1), ("A", True, 1), ("A", False, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("run", CURSOR_RUNS, ids=["%s%s%s" % (n, "-alpha" if a else "", "" if nt else "-temporal") for n, a, nt in CURSOR_RUNS])
def test_gpu_half_rep_cursor_steps(gh, oracle, run):
    """The persistent kernel's cursor with a step whose tile, row-pair and frame components are all non-zero (A, B: the carries
    from tile to row pair to frame all happen), and a ring past the 32-entry pointer table (C); with an alpha plane and with
    the default cache policy.  One launch through decodeBT709ScaledBatch, every frame against the oracle."""
    from metalbt709decoder_amd.decoder import DeviceBuffer
    name, alpha, nontemporal = run
    _, (w, h), frames, wg, _, _, _ = next(c for c in rc.CURSOR_CASES if c[0] == name)
    ctx = gh.context()
    dec = gh.make_decoder(mb.MetalBT709GammaApple, has_alpha=alpha, options={
        _capi.OPT_HALF_KERNEL: 1, _capi.OPT_HALF_WORKGROUPS: wg, _capi.OPT_NONTEMPORAL: nontemporal})
    gamma = dec.gamma
    ow, oh = w // 2, h // 2
    c_off, a_off = w * h, w * h * 3 // 2
    in_pitch = _round_up(w * h * (5 if alpha else 3) // 2, 256)
    stride = 4 * ow + 16
    out_pitch = _round_up(stride * oh, 256) + 256
    slab_in, out_bytes = DeviceBuffer(ctx, frames * in_pitch), frames * out_pitch + 256
    slab_out = DeviceBuffer(ctx, out_bytes)
    _capi.check(ctx.lib.bt709hip_memset(ctx.handle, slab_out.ptr, rc.FILL, out_bytes, None))
    ctx._sync(None)
    rng = np.random.default_rng(6709 + ord(name))
    planes, bufs, abufs, texs = [], [], [], []
    for i in range(frames):
        y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        c = rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
        a = rng.integers(0, 256, (h, w), dtype=np.uint8) if alpha else None
        base = slab_in.ptr + i * in_pitch
        b = mb.CVPixelBuffer(ctx, w, h, w, w, planes=(base, base + c_off))
        b.setAttachment("YCbCrMatrix", mb.kCVImageBufferYCbCrMatrix_ITU_R_709_2)
        b.setAttachment("TransferFunction", gh.TRANSFER_FOR_GAMMA[gamma])
        b.upload_planes(y, c)
        bufs.append(b)
        if alpha:
            ctx._upload(base + a_off, w, a, None)
            ab = mb.CVPixelBuffer(ctx, w, h, w, w, planes=(base + a_off, base + c_off))
            ab.setAttachment("TransferFunction", mb.kCVImageBufferTransferFunction_Linear)
            abufs.append(ab)
        planes.append((y, c, a))
        texs.append(mb.BGRATexture(ctx, ow, oh, stride, ptr=slab_out.ptr + 256 + i * out_pitch))
    assert dec.decodeBT709ScaledBatch(bufs, texs, None, True, alphaPixelBuffers=abufs or None), dec.lastStatus
    assert ctx.lib.bt709hip_last_kernel_name() == (b"decode_nv12_half_rep<alpha>" if alpha else b"decode_nv12_half_rep")
    plan, record = rc.half_rep_plan(w, h, frames, wg), _launch_record(ctx)
    assert (record["grid"], record["block"], record["launches"]) == ((wg, 1, 1), plan["block"], 1), (record, plan)
    raw = np.empty(out_bytes, np.uint8)
    _capi.check(ctx.lib.bt709hip_download(ctx.handle, raw.ctypes.data, out_bytes, slab_out.ptr, out_bytes, out_bytes, 1, None))
    ctx._sync(None)
    untouched = np.ones(out_bytes, bool)
    for i, (y, c, a) in enumerate(planes):
        o = 256 + i * out_pitch
        got = raw[o:o + stride * oh].reshape(oh, stride)[:, :4 * ow]
        want = oracle.decode_nv12_half(gamma, y, c, alpha=a)
        assert np.array_equal(got, want), "case %s frame %d: %d bytes differ, first at row, byte %r; plan %r" % (
            name, i, int((got != want).sum()), tuple(np.argwhere(got != want)[0]), plan)
        untouched[o:o + stride * oh].reshape(oh, stride)[:, :4 * ow] = False
    assert (raw[untouched] == rc.FILL).all(), "case %s: bytes written outside the views" % name
