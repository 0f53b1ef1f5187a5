"""GPU tests (-m gpu) of BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT = BT709HIP_CHROMA_I420: bt709hip_encode[_batch] writing planar Y, U, V
frames in place.  The arithmetic is the NV12 encoder's and is swept by tests/test_encoder.py; what these tests pin
is PLACEMENT -- which byte goes to which plane, row and column, at which sizes, pitches and alignments, in which kernel -- and the
two things a planar twin can break quietly: the rounding mode around the converting pack (every colour) and the 64-bit V offset.

Expected planes come from the CPU oracle: encoder_cases.threaded_encode (or oracle.encode_nv12), then U = c[:, 0::2] and
V = c[:, 1::2]; never from the code under test.  Every output slab is filled with 0x5A and compared whole, so row padding, the gap
between U's last row and V's first, the bytes behind V and the guard bands are part of every comparison.  Every case asserts the
kernel it was built to reach."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import encoder_cases as ec
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_APPLE, GAMMA_LINEAR, GAMMA_SRGB

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NV12, I420 = 0, 1
FAST, GENERAL = "encode_bgra_i420", "encode_bgra_i420_blocks"
GUARD, FILL = ec.GUARD, ec.FILL
ALPHA_FORMAT = 3  # BT709HIP_FORMAT_BGRA8_ALPHA
LIN = (GAMMA_LINEAR, GAMMA_LINEAR)


# ------------------------------------------------------------------ layouts, expectations, the harness

class PlanarLayout:
    """encoder_cases.Layout whose third slab holds, per picture, the U plane and -- (H/2) x sc bytes behind it -- the V plane:
    H rows of W/2 bytes at pitch sc."""

    def __init__(self, w, h, strides, in_off, y_off, c_off):
        self.w, self.h = w, h
        self.sb, self.sy, self.sc = strides
        self.in_off, self.y_off, self.c_off = list(in_off), list(y_off), list(c_off)
        self.n = len(self.in_off)
        self.in_span = (h - 1) * self.sb + 4 * w
        self.y_span = (h - 1) * self.sy + w
        self.c_span = (h - 1) * self.sc + w // 2  # U's H/2 rows, then V's
        self.in_bytes = max(self.in_off) + self.in_span + GUARD
        self.y_bytes = max(self.y_off) + self.y_span + GUARD
        self.c_bytes = max(self.c_off) + self.c_span + GUARD
        assert self.sc >= w // 2
        for offs, span in ((self.in_off, self.in_span), (self.y_off, self.y_span), (self.c_off, self.c_span)):
            o = sorted(offs)
            assert o[0] >= GUARD and all(b - a >= span for a, b in zip(o, o[1:])), "pictures overlap or leave no guard band"

    def v_off(self, i):
        return self.c_off[i] + (self.h // 2) * self.sc


def single(w, h, strides=None, misalign=(0, 0, 0)):
    return PlanarLayout(w, h, strides or (4 * w, w, w // 2), *[[GUARD + m] for m in misalign])


def planar_fast_path(L):
    """The fast kernel's predicate under I420, restated: W % 4; BGRA pointer and pitch 16-byte aligned; Y 4-byte; the U pointer
    2-byte aligned and cbcr_stride even.  (Slab bases are 256-byte aligned: the harness asserts it.)"""
    return (L.w % 4 == 0 and L.sb % 16 == 0 and L.sy % 4 == 0 and L.sc % 2 == 0 and all(o % 16 == 0 for o in L.in_off)
            and all(o % 4 == 0 for o in L.y_off) and all(o % 2 == 0 for o in L.c_off))


def planar_plan(L, bands=True):
    """encoder_cases.expected_plan (the NV12 encoder's plan for the same width, height and count) under the planar predicate and
    the planar kernel names."""
    fast = planar_fast_path(L)
    plan = ec.expected_plan(L.w, L.h, L.n, fast=fast, uniform=ec.layout_is_uniform(L), bands=bands)
    plan["kernel"] = FAST if fast else GENERAL
    return plan


def split(c):
    return c[:, 0::2], c[:, 1::2]


def expected_slabs(L, planes):
    """planes(i) -> (y (h, w), u (h/2, w/2), v (h/2, w/2)) of slot i -> the Y slab and the chroma slab as they must read back."""
    ys, cs = np.full(L.y_bytes, FILL, np.uint8), np.full(L.c_bytes, FILL, np.uint8)
    for i in range(L.n):
        y, u, v = planes(i)
        ec._rows_view(ys, L.y_off[i], L.h, L.sy, L.w)[:] = y
        ec._rows_view(cs, L.c_off[i], L.h // 2, L.sc, L.w // 2)[:] = u
        ec._rows_view(cs, L.v_off(i), L.h // 2, L.sc, L.w // 2)[:] = v
    return ys, cs


def describe_chroma(L, got, want):
    diff = np.flatnonzero(got != want)
    if diff.size == 0:
        return None
    p = int(diff[0])
    where = "outside every picture (guard band)"
    for i in range(L.n):
        for plane, o in (("U", L.c_off[i]), ("V", L.v_off(i))):
            if o <= p < o + (L.h // 2 - 1) * L.sc + L.w // 2:
                r, col = divmod(p - o, L.sc)
                where = "slot %d %s row %d column %d%s" % (i, plane, r, col, " (row padding)" if col >= L.w // 2 else "")
    return "chroma slab: %d bytes differ, first at byte %d = %s: got %d, want %d" % (diff.size, p, where, got[p], want[p])


def differences(L, res, planes):
    want_y, want_c = expected_slabs(L, planes)
    return [d for d in (ec.describe_difference(L, res.y_slab, want_y, "y"), describe_chroma(L, res.c_slab, want_c)) if d]


class Harness(ec.Harness):
    """encoder_cases.Harness with the context's encoder layout set for the call (and back at NV12 after it, whatever happens:
    the context is the process's), any input format, and frames without a chroma plane."""

    def encode(self, layout, in_slab, pair, option=I420, fmt=_capi.FORMAT_BGRA8_SRGB, with_cbcr=True):
        capi, L = self.capi, layout
        assert in_slab.size == L.in_bytes
        d_in, d_y, d_c = (self.DeviceBuffer(self.ctx, nb, placement_tries=1) for nb in (L.in_bytes, L.y_bytes, L.c_bytes))
        try:
            assert all(d.ptr % 256 == 0 for d in (d_in, d_y, d_c))
            self._upload(d_in.ptr, in_slab)
            for d, nb in ((d_y, L.y_bytes), (d_c, L.c_bytes)):
                capi.check(self.lib.bt709hip_memset(self.h, d.ptr, FILL, nb, None))
            capi.check(self.lib.bt709hip_stream_synchronize(self.h, None))
            surfs = (capi.Surface * L.n)(*[capi.Surface(d_in.ptr + o, L.sb, L.w, L.h, fmt, 0) for o in L.in_off])
            frames = (capi.Frame * L.n)(*[capi.Frame(d_y.ptr + oy, L.sy, d_c.ptr + oc if with_cbcr else None, L.sc if with_cbcr else 0, L.w, L.h, 0, 0)
                                          for oy, oc in zip(L.y_off, L.c_off)])
            assert self.ctx.setEncodeChromaLayout(option)
            try:
                capi.check(self.lib.bt709hip_encode_batch(self.h, L.n, surfs, frames, pair[0], pair[1], None, 1), "bt709hip_encode_batch")
            finally:
                assert self.ctx.setEncodeChromaLayout(NV12)
            kernel = self.lib.bt709hip_last_kernel_name().decode()
            info = capi.LaunchInfo()
            capi.check(self.lib.bt709hip_last_launch_info(C.byref(info)))
            return ec.Result(self._download(d_y.ptr, L.y_bytes), self._download(d_c.ptr, L.c_bytes), kernel, info)
        finally:
            for d in (d_in, d_y, d_c):
                d.free()


@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


@pytest.fixture(scope="module")
def harness(gh):
    return Harness(gh)


_REFERENCE = {}


def reference(oracle, seed, w, h, pair):
    """mixed_picture(seed, w, h) and its oracle planes, computed once per (seed, size, pair) and shared; never written to."""
    key = (seed, w, h, pair)
    if key not in _REFERENCE:
        words = ec.mixed_picture(seed, w, h)
        y, c = ec.threaded_encode(oracle, words, w, h, *pair)
        for a in (words, y, c):
            a.setflags(write=False)
        _REFERENCE[key] = (words, y, c)
    return _REFERENCE[key]


def run_single(harness, oracle, L, pair, seed, kernel):
    assert planar_fast_path(L) == (kernel == FAST), "the case does not reach the kernel it names"
    words, y, c = reference(oracle, seed, L.w, L.h, pair)
    assert (c[:, 0::2] != c[:, 1::2]).any()
    res = harness.encode(L, ec.fill_input(L, lambda i: words), pair)
    assert res.kernel == kernel
    assert res.launches == 1
    d = differences(L, res, lambda i: (y,) + split(c))
    assert not d, "\n".join(d)
    return res


# ------------------------------------------------------------------ 1. pairing and padding, one picture per launch

FAST_CASES = {
    "8x2": (8, 2, None, (0, 0, 0)),                                          # two quads
    "260x6": (260, 6, None, (0, 0, 0)),                                      # 65 quads: a second wave with one live lane
    "2052x38": (2052, 38, None, (0, 0, 0)),                                  # two tiles, the second mostly empty; 19 row pairs = 6 x 3 + 1
    "1920x54-padded": (1920, 54, (7744, 2048, 976), (0, 0, 0)),              # padding in every plane, and between U's last row and V's first
    "1284x20-u+2": (1284, 20, (4 * 1284, 1284, 646), (0, 0, 2)),             # 2-byte alignment only: still the fast kernel
}
GENERAL_CASES = {
    "62x6": (62, 6, None, (0, 0, 0)),
    "1918x22-odd-everything": (1918, 22, (4 * 1918 + 12, 1918 + 5, 963), (4, 1, 3)),  # odd U pointer and odd pitch
    "64x8-u-odd": (64, 8, None, (0, 0, 1)),                                  # a fast-eligible width pushed over by alignment alone
}


@pytest.mark.parametrize("name", FAST_CASES)
def test_fast_kernel_pairing_and_padding(harness, oracle, name):
    w, h, strides, mis = FAST_CASES[name]
    k = list(FAST_CASES).index(name)
    res = run_single(harness, oracle, single(w, h, strides, mis), ec.PAIRS[k % len(ec.PAIRS)], 4200 + k, FAST)
    if name == "2052x38":
        assert res.grid == (2, 7, 1)


@pytest.mark.parametrize("name", GENERAL_CASES)
def test_general_kernel_any_alignment(harness, oracle, name):
    w, h, strides, mis = GENERAL_CASES[name]
    k = list(GENERAL_CASES).index(name)
    run_single(harness, oracle, single(w, h, strides, mis), ec.PAIRS[(k + 1) % len(ec.PAIRS)], 4300 + k, GENERAL)


# ------------------------------------------------------------------ 2. every colour: the rounding mode around the pack

EVERY_COLOUR_PAIR = (GAMMA_SRGB, GAMMA_APPLE)
BLOCKS_STRIP = 5
_STRIP = {}


def colour_strip(oracle, strip):
    """Strip `strip` of the all-colours picture and its oracle planes; the one strip two tests use is kept."""
    if strip in _STRIP:
        return _STRIP[strip]
    side, rows = ec.ALL_COLOURS_SIDE, ec.ALL_COLOURS_SIDE // ec.ALL_COLOURS_STRIPS
    words = ec.all_colours_strip(strip, seed=7090 + strip)
    y, c = ec.threaded_encode(oracle, words, side, rows, *EVERY_COLOUR_PAIR)
    if strip == BLOCKS_STRIP:
        for a in (words, y, c):
            a.setflags(write=False)
        _STRIP[strip] = (words, y, c)
    return words, y, c


@pytest.mark.parametrize("strip", range(ec.ALL_COLOURS_STRIPS))
def test_every_colour_through_the_fast_kernel(harness, oracle, strip):
    """Every (R,G,B) once as a flat 2x2 block, 2^21 colours a strip: the exact ties of the Y, Cb and Cr quantisers are among them
    and come out one low when the twelve conversions lose round-toward-zero."""
    side, rows = ec.ALL_COLOURS_SIDE, ec.ALL_COLOURS_SIDE // ec.ALL_COLOURS_STRIPS
    L = single(side, rows)
    words, y, c = colour_strip(oracle, strip)
    res = harness.encode(L, ec.fill_input(L, lambda i: words), EVERY_COLOUR_PAIR)
    assert res.kernel == FAST
    d = differences(L, res, lambda i: (y,) + split(c))
    assert not d, "strip %d (colours 0x%06x..): %s" % (strip, strip << 21, "\n".join(d))


def test_one_colour_strip_through_the_general_kernel(harness, oracle):
    side, rows = ec.ALL_COLOURS_SIDE, ec.ALL_COLOURS_SIDE // ec.ALL_COLOURS_STRIPS
    L = single(side, rows, misalign=(0, 0, 1))  # a 1-byte U misalignment
    assert not planar_fast_path(L)
    words, y, c = colour_strip(oracle, BLOCKS_STRIP)
    res = harness.encode(L, ec.fill_input(L, lambda i: words), EVERY_COLOUR_PAIR)
    assert res.kernel == GENERAL
    d = differences(L, res, lambda i: (y,) + split(c))
    assert not d, "\n".join(d)


# ------------------------------------------------------------------ 3. against the product's own two launches

def test_equals_nv12_encode_then_deinterleave(harness, oracle):
    """The route the new path replaces -- bt709hip_encode under NV12, then bt709hip_deinterleave_cbcr into planes laid out like
    the planar frame's -- leaves the same three planes, padding and gaps included."""
    w, h, strides, mis = FAST_CASES["1920x54-padded"]
    pair = ec.PAIRS[3]
    L = single(w, h, strides, mis)
    words, y, c = reference(oracle, 4203, w, h, pair)
    in_slab = ec.fill_input(L, lambda i: words)
    res = harness.encode(L, in_slab, pair)
    assert res.kernel == FAST
    capi, lib, hd = harness.capi, harness.lib, harness.h
    N = ec.Layout(w, h, (L.sb, L.sy, 1936), [GUARD], [GUARD], [GUARD])
    d_in, d_y, d_c, d_p = (harness.DeviceBuffer(harness.ctx, nb, placement_tries=1) for nb in (N.in_bytes, N.y_bytes, N.c_bytes, L.c_bytes))
    try:
        harness._upload(d_in.ptr, in_slab)
        for d, nb in ((d_y, N.y_bytes), (d_c, N.c_bytes), (d_p, L.c_bytes)):
            capi.check(lib.bt709hip_memset(hd, d.ptr, FILL, nb, None))
        surf = capi.Surface(d_in.ptr + GUARD, N.sb, w, h, capi.FORMAT_BGRA8_SRGB, 0)
        frame = capi.Frame(d_y.ptr + GUARD, N.sy, d_c.ptr + GUARD, N.sc, w, h, 0, 0)
        capi.check(lib.bt709hip_encode(hd, C.byref(surf), C.byref(frame), pair[0], pair[1], None, 1))
        assert lib.bt709hip_last_kernel_name() == b"encode_bgra_nv12"
        u_ptr = d_p.ptr + L.c_off[0]
        capi.check(lib.bt709hip_deinterleave_cbcr(hd, d_c.ptr + GUARD, N.sc, u_ptr, L.sc, u_ptr + (h // 2) * L.sc, L.sc, w // 2, h // 2, None, 1))
        two_y, two_c = harness._download(d_y.ptr, N.y_bytes), harness._download(d_p.ptr, L.c_bytes)
    finally:
        for d in (d_in, d_y, d_c, d_p):
            d.free()
    assert np.array_equal(two_y, res.y_slab) and np.array_equal(two_c, res.c_slab)
    assert not differences(L, res, lambda i: (y,) + split(c))


# ------------------------------------------------------------------ 4. batches

def case_layout(case):
    """encoder_cases.case_layout for planar frames: a slot of the chroma slab is U then V, H rows of the chroma pitch."""
    w, h, n = case.w, case.h, case.n
    sb, sy, sc = case.strides
    pitch = [h * sb + case.gaps[0], h * sy + case.gaps[1], h * sc + case.gaps[2]]
    offs = []
    for j in range(3):
        extra = np.zeros(n, np.int64) if case.spacing == "even" else np.cumsum([256 * ((i * i) % 5) for i in range(n)])
        offs.append([GUARD + case.misalign[j] + i * pitch[j] + int(extra[i]) for i in range(n)])
    return PlanarLayout(w, h, (sb, sy, sc), *offs)


def run_case(harness, oracle, case, seed):
    """encoder_cases.run_case on a planar layout: every slot's content is distinct (build_slots)."""
    L = case_layout(case)
    bases, patches = ec.build_slots(oracle, case, seed)
    rows = ec.slot_rows(case.h)

    def picture(i):
        words = bases[i % len(bases)][0].copy()
        for j, rp in enumerate(rows):
            words[2 * rp:2 * rp + 2] = patches[0][i, j]
        return words

    def planes(i):
        _, y, c = bases[i % len(bases)]
        y, c = y.copy(), c.copy()
        for j, rp in enumerate(rows):
            y[2 * rp:2 * rp + 2], c[rp] = patches[1][i, j], patches[2][i, j]
        return (y,) + split(c)

    res = harness.encode(L, ec.fill_input(L, picture), case.pair)
    return L, res, differences(L, res, planes)


def assert_plan(L, res, bands=True):
    plan = planar_plan(L, bands)
    assert (res.kernel, res.grid, res.block, res.launches, res.xcd_bands) == (
        plan["kernel"], tuple(plan["grid"]), (plan["block"], 1, 1), plan["launches"], plan["xcd_bands"]), plan
    return plan


def planar_case(name, w, h, n, pair, **kw):
    kw.setdefault("strides", (4 * w, w, w // 2))
    return ec.Case(name, w, h, n, pair, None, **kw)


def test_batch_through_the_pointer_table(harness, oracle):
    case = planar_case("260x6x3-table", 260, 6, 3, ec.PAIRS[1], spacing="table", bases=2)
    L, res, diffs = run_case(harness, oracle, case, 51)
    assert not ec.layout_is_uniform(L) and res.kernel == FAST and res.grid[2] == 3
    assert_plan(L, res)
    assert not diffs, "\n".join(diffs)


def test_batch_evenly_spaced_band_map_and_tail(harness, oracle):
    case = planar_case("64x8x70-even", 64, 8, 70, ec.PAIRS[0], bases=2)
    L, res, diffs = run_case(harness, oracle, case, 52)
    assert ec.layout_is_uniform(L) and res.kernel == FAST
    assert res.launches == 2 and res.xcd_bands == 1  # the band map over 64 frames, a plain tail of 6
    assert res.grid == (8, 2, 8)
    assert_plan(L, res)
    assert not diffs, "\n".join(diffs)


def test_batch_chroma_slab_spaced_differently_from_luma(harness, oracle):
    """40 pictures, the U planes in a slab of their own at another spacing than Y's: V follows from U, not from Y.  Then the same
    call with BT709HIP_CTX_OPT_XCD_BANDS at 0."""
    case = planar_case("256x16x40-gaps", 256, 16, 40, ec.PAIRS[4], gaps=(4096, 512, 256), bases=2)
    L = case_layout(case)
    assert L.y_off[1] - L.y_off[0] != L.c_off[1] - L.c_off[0]
    L, res, diffs = run_case(harness, oracle, case, 53)
    assert res.kernel == FAST and res.grid[2] == 40
    assert_plan(L, res)
    assert not diffs, "\n".join(diffs)
    lib, hd = harness.lib, harness.h
    _capi.check(lib.bt709hip_context_set_option(hd, _capi.CTX_OPT_XCD_BANDS, 0))
    try:
        L, res, diffs = run_case(harness, oracle, case, 53)
    finally:
        _capi.check(lib.bt709hip_context_set_option(hd, _capi.CTX_OPT_XCD_BANDS, 1))
    assert res.kernel == FAST
    assert_plan(L, res, bands=False)
    assert not diffs, "\n".join(diffs)


# ------------------------------------------------------------------ 5. the launch plan is the NV12 encoder's

PLAN_SHAPES = {
    "4k-single": (3840, 2160, 1),            # the single-picture tile shape: 2 x 512 lanes
    "1284x20x71-head-and-tail": (1284, 20, 71),
    "64x38x2048-nine-row-pairs": (64, 38, 2048),
    "1918x22-general": (1918, 22, 1),
}


@pytest.mark.parametrize("name", PLAN_SHAPES)
def test_launch_plan_is_the_nv12_encoders(harness, name):
    """bt709hip_last_launch_info equals encoder_cases.expected_plan for the same width, height and count in everything but the
    kernel name; the same call under NV12 leaves the same record.  (Content is not compared here: noise in, planes out.)"""
    w, h, n = PLAN_SHAPES[name]
    rng = np.random.default_rng(len(name))
    pic = rng.integers(0, 1 << 32, (h, w), dtype=np.uint32)
    records = []
    for option in (I420, NV12):
        case = ec.Case(name, w, h, n, ec.PAIRS[0], None, strides=(4 * w, w, w // 2 if option == I420 else w))
        L = case_layout(case) if option == I420 else ec.case_layout(case)
        res = harness.encode(L, ec.fill_input(L, lambda i: pic), case.pair, option=option)
        records.append((res.grid, res.block, res.launches, res.xcd_bands))
        if option == I420:
            plan = assert_plan(L, res)
            assert plan["kernel"] == (GENERAL if w % 4 else FAST)
        else:
            assert res.kernel == ("encode_bgra_nv12_blocks" if w % 4 else "encode_bgra_nv12")
    assert records[0] == records[1]


# ------------------------------------------------------------------ 6. alpha frames

@pytest.fixture(scope="module")
def alpha_luma():
    doc = json.load(open(os.path.join(HERE, "golden", "alpha_luma.json")))
    assert len(doc["luma"]) == 256 and doc["cbcr"] == 128
    return np.array(doc["luma"], np.uint8)


ALPHA_CASES = {"64x8-fast": (64, 8, (4 * 64 + 16, 68, 38), "encode_alpha_y"), "62x6-general": (62, 6, (4 * 62 + 4, 63, 35), "encode_alpha_y_blocks")}


@pytest.mark.parametrize("name", ALPHA_CASES)
def test_alpha_frames(harness, alpha_luma, name):
    """BGRA8_ALPHA input: Y is the table's.  With chroma planes under I420 every U and every V byte is 128 and the padding keeps
    its fill; with cbcr NULL only Y is written, by the NV12 kernels under their own names, whatever the option holds."""
    w, h, strides, stem = ALPHA_CASES[name]
    L = single(w, h, strides)
    words = np.random.default_rng(w).integers(0, 1 << 32, (h, w), dtype=np.uint32)
    in_slab = ec.fill_input(L, lambda i: words)
    y = alpha_luma[(words >> 24).astype(np.uint8)]
    grey = np.full((h // 2, w // 2), 128, np.uint8)
    res = harness.encode(L, in_slab, LIN, fmt=ALPHA_FORMAT)
    assert res.kernel == stem + "<i420>"
    d = differences(L, res, lambda i: (y, grey, grey))
    assert not d, "\n".join(d)
    for option in (I420, NV12):
        res = harness.encode(L, in_slab, LIN, option=option, fmt=ALPHA_FORMAT, with_cbcr=False)
        assert res.kernel == stem
        want_y, _ = expected_slabs(L, lambda i: (y, grey, grey))
        assert np.array_equal(res.y_slab, want_y) and (res.c_slab == FILL).all()


# ------------------------------------------------------------------ 7. the V plane more than 2^32 bytes behind U

TWO32 = 1 << 32
WINDOW_GUARD = 256


@pytest.mark.parametrize("kernel", [FAST, GENERAL])
def test_v_offset_past_2_32(harness, oracle, kernel):
    """Two chroma rows a plane at a pitch of 2 GiB and a little: (H/2) x cbcr_stride = 2^32 + 2d, so V starts past 2^32 from U.  A
    product cut to 32 bits would put V's rows 2d (+ r pitches) behind U -- the alias windows, inside the slab, which must keep
    their fill.  The host touches only the rows' windows and the alias windows of a 6 GiB allocation."""
    w, h = (64, 4) if kernel == FAST else (62, 4)
    d, u_off = (4096, GUARD) if kernel == FAST else (4097, GUARD + 1)  # general: odd pitch, odd U pointer
    sc = (1 << 31) + d
    pair = ec.PAIRS[0]
    rows, rb = h // 2, w // 2
    v_offset = rows * sc
    assert v_offset > TWO32 and sc <= 0xFFFFFFFF
    slab_bytes = u_off + (h - 1) * sc + rb + GUARD
    samples = {("U", r): u_off + r * sc for r in range(rows)}
    samples.update({("V", r): u_off + v_offset + r * sc for r in range(rows)})
    alias = {r: u_off + (v_offset & 0xFFFFFFFF) + r * sc for r in range(rows)}
    windows = sorted([(o - WINDOW_GUARD, o + rb + WINDOW_GUARD) for o in samples.values()] + [(o, o + rb) for o in alias.values()])
    # on the CPU, before anything is launched: every window inside the slab, apart from the others; the alias windows where
    # the wrong arithmetic would land and on no sample
    assert all(0 <= lo < hi <= slab_bytes for lo, hi in windows)
    assert all(a[1] <= b[0] for a, b in zip(windows, windows[1:]))
    assert all(o == samples[("U", r)] + 2 * d for r, o in alias.items())
    assert samples[("V", rows - 1)] + rb + GUARD <= slab_bytes

    Ly = single(w, h, (4 * w, w, rb))  # BGRA and Y of ordinary layouts; the chroma slab is this test's own
    assert (w % 4 == 0 and sc % 2 == 0 and u_off % 2 == 0) == (kernel == FAST)
    words, y, c = reference(oracle, 4400 + w, w, h, pair)
    u, v = split(c)
    capi, lib, hd = harness.capi, harness.lib, harness.h
    d_in, d_y, d_c = (harness.DeviceBuffer(harness.ctx, nb, placement_tries=1) for nb in (Ly.in_bytes, Ly.y_bytes, slab_bytes))
    try:
        assert all(b.ptr % 256 == 0 for b in (d_in, d_y, d_c))
        harness._upload(d_in.ptr, ec.fill_input(Ly, lambda i: words))
        capi.check(lib.bt709hip_memset(hd, d_y.ptr, FILL, Ly.y_bytes, None))
        for lo, hi in windows:
            capi.check(lib.bt709hip_memset(hd, d_c.ptr + lo, FILL, hi - lo, None))
        capi.check(lib.bt709hip_stream_synchronize(hd, None))
        surf = capi.Surface(d_in.ptr + GUARD, Ly.sb, w, h, capi.FORMAT_BGRA8_SRGB, 0)
        frame = capi.Frame(d_y.ptr + GUARD, Ly.sy, d_c.ptr + u_off, sc, w, h, 0, 0)
        assert harness.ctx.setEncodeChromaLayout(I420)
        try:
            capi.check(lib.bt709hip_encode(hd, C.byref(surf), C.byref(frame), pair[0], pair[1], None, 1), "bt709hip_encode")
        finally:
            assert harness.ctx.setEncodeChromaLayout(NV12)
        assert lib.bt709hip_last_kernel_name().decode() == kernel
        got_y = harness._download(d_y.ptr, Ly.y_bytes)
        got = {(lo, hi): harness._download(d_c.ptr + lo, hi - lo) for lo, hi in windows}
    finally:
        for b in (d_in, d_y, d_c):
            b.free()
    want_y = np.full(Ly.y_bytes, FILL, np.uint8)
    ec._rows_view(want_y, GUARD, h, Ly.sy, w)[:] = y
    assert np.array_equal(got_y, want_y)
    for r, o in alias.items():
        assert (got[(o, o + rb)] == FILL).all(), "V row %d was written where a 32-bit product lands" % r
    for (plane, r), o in samples.items():
        want = np.full(rb + 2 * WINDOW_GUARD, FILL, np.uint8)
        want[WINDOW_GUARD:WINDOW_GUARD + rb] = (u if plane == "U" else v)[r]
        assert np.array_equal(got[(o - WINDOW_GUARD, o + rb + WINDOW_GUARD)], want), (plane, r)


# ------------------------------------------------------------------ 8. round trip = the file format; the Python mirror

def test_round_trip_is_the_file_format(gh, oracle, tmp_path):
    """64 x 16 encoded into ONE tight planar allocation: a contiguous download is Y | U | V of the NV12 route, the Y4M files of
    the two buffers are byte-identical, and the planar buffer decodes in place to what the NV12 buffer decodes to."""
    from metalbt709decoder_amd import y4m
    conv, ctx = mb.BGRAToBT709Converter, gh.context()
    w, h, pair = 64, 16, (mb.MetalBT709GammaSRGB, mb.MetalBT709GammaApple)
    words, y, c = reference(oracle, 4500, w, h, (GAMMA_SRGB, GAMMA_APPLE))
    tex = ctx.makeBGRATexture((w, h), pixels=words)
    planar = conv.createCoreVideoYCbCrBuffer(ctx, (w, h), y_stride=w, cbcr_stride=w // 2, planar=True)
    nv12 = conv.createCoreVideoYCbCrBuffer(ctx, (w, h), y_stride=w, cbcr_stride=w)
    assert planar.cbcr_ptr == planar.y_ptr + w * h  # a tight FRAME payload
    try:
        assert conv.convertIntoCoreVideoBuffer(tex, planar, *pair)
        assert ctx.lib.bt709hip_last_kernel_name() == FAST.encode()
        assert conv.convertIntoCoreVideoBuffer(tex, nv12, *pair)
        assert ctx.lib.bt709hip_last_kernel_name() == b"encode_bgra_nv12"
    finally:
        assert ctx.setEncodeChromaLayout(NV12)
    payload = np.empty(w * h * 3 // 2, np.uint8)
    _capi.check(ctx.lib.bt709hip_download(ctx.handle, payload.ctypes.data, payload.size, planar.y_ptr, payload.size, payload.size, 1, None))
    ctx._sync(None)
    ny, nc = nv12.download_planes()
    assert np.array_equal(ny, y) and np.array_equal(nc, c)  # the NV12 route is the oracle's
    assert payload.tobytes() == ny.tobytes() + nc[:, 0::2].tobytes() + nc[:, 1::2].tobytes()
    files = []
    for name, buf in (("planar.y4m", planar), ("nv12.y4m", nv12)):
        path = str(tmp_path / name)
        with y4m.Y4MWriter(path, w, h) as wr:
            wr.write_pixel_buffer(buf)
        files.append(open(path, "rb").read())
    assert files[0] == files[1] and files[0].endswith(payload.tobytes())
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    out = []
    for buf, name in ((planar, b"decode_i420_quads<nt>"), (nv12, b"decode_nv12_quads<nt>")):
        conv.setBT709Attributes(buf)
        t = ctx.makeBGRATexture((w, h))
        assert dec.decodeBT709(buf, None, t, ctx.commandQueue.commandBuffer(), None, w, h, True), dec.lastStatus
        assert ctx.lib.bt709hip_last_kernel_name() == name
        out.append(ctx.getBGRATexturePixels(t).copy())
    assert np.array_equal(out[0], out[1])


def test_python_mirror_sets_the_layout_from_the_buffers(gh, oracle):
    """convertIntoCoreVideoBuffer into a planar buffer, an NV12 one, a planar one: each right, the kernel names alternating (the
    buffer's flag is authoritative, the setter called on a change).  A mixed list is refused before anything is launched."""
    conv, ctx = mb.BGRAToBT709Converter, gh.context()
    w, h, pair = 64, 16, (mb.MetalBT709GammaSRGB, mb.MetalBT709GammaApple)
    words, y, c = reference(oracle, 4500, w, h, (GAMMA_SRGB, GAMMA_APPLE))
    tex = ctx.makeBGRATexture((w, h), pixels=words)
    planar = conv.createCoreVideoYCbCrBuffer(ctx, (w, h), planar=True)
    nv12 = conv.createCoreVideoYCbCrBuffer(ctx, (w, h))

    def wipe(buf):
        _capi.check(ctx.lib.bt709hip_memset(ctx.handle, buf._buf.ptr, FILL, buf._buf.nbytes, None))
        ctx._sync(None)

    def raw(buf):
        out = np.empty(buf._buf.nbytes, np.uint8)
        _capi.check(ctx.lib.bt709hip_download(ctx.handle, out.ctypes.data, out.size, buf._buf.ptr, out.size, out.size, 1, None))
        ctx._sync(None)
        return out

    try:
        for buf, layout, name in ((planar, I420, FAST), (nv12, NV12, "encode_bgra_nv12"), (planar, I420, FAST)):
            wipe(buf)
            assert conv.convertIntoCoreVideoBuffer(tex, buf, *pair)
            assert ctx.lib.bt709hip_last_kernel_name().decode() == name and ctx._encode_layout == layout
            if buf.planar:
                gy, gu, gv = buf.download_yuv()
                assert np.array_equal(gy, y) and np.array_equal(gu, c[:, 0::2]) and np.array_equal(gv, c[:, 1::2])
            else:
                gy, gc = buf.download_planes()
                assert np.array_equal(gy, y) and np.array_equal(gc, c)
        wipe(planar), wipe(nv12)
        held = ctx._encode_layout
        assert conv.convertIntoCoreVideoBuffers([tex, tex], [planar, nv12], *pair) is False
        assert conv.convertIntoCoreVideoBuffers([tex, tex], [nv12, planar], *pair) is False
        assert ctx._encode_layout == held
        assert (raw(planar) == FILL).all() and (raw(nv12) == FILL).all()
        # two planar buffers in one call: one launch, both right
        other = conv.createCoreVideoYCbCrBuffer(ctx, (w, h), planar=True)
        assert conv.convertIntoCoreVideoBuffers([tex, tex], [planar, other], *pair)
        assert ctx.lib.bt709hip_last_kernel_name().decode() == FAST
        for buf in (planar, other):
            gy, gu, gv = buf.download_yuv()
            assert np.array_equal(gy, y) and np.array_equal(gu, c[:, 0::2]) and np.array_equal(gv, c[:, 1::2])
    finally:
        assert ctx.setEncodeChromaLayout(NV12)


# ------------------------------------------------------------------ 9. fuzzed geometry

FUZZ_CASES, FUZZ_CHUNK = 60, 10


def fuzz_case(i, seed=30709):
    """Case i of the seeded sequence, modelled on encoder_cases.fuzz_case with chroma pitches >= W/2: half of the cases meet the
    fast predicate's alignment (2 bytes on the U plane; then W % 4 decides), one to five pictures, evenly or irregularly spaced.
    -> (PlanarLayout, pair, rng for the pictures)."""
    rng = np.random.default_rng([seed, i])
    pair = ec.PAIRS[int(rng.integers(0, len(ec.PAIRS)))]
    kind = int(rng.integers(0, 4))
    if kind == 0:    # around and across a tile-count boundary
        w = max(2, ec.FUZZ_WIDTH_CENTRES[int(rng.integers(0, 4))] + 2 * int(rng.integers(-6, 7)))
        h = 2 * int(rng.integers(1, 8))
    elif kind == 1:  # small
        w, h = 2 * int(rng.integers(1, 40)), 2 * int(rng.integers(1, 12))
    else:            # anything moderate
        w, h = 2 * int(rng.integers(1, 700)), 2 * int(rng.integers(1, 24))
    n = 1 if rng.integers(0, 2) else int(rng.integers(2, 6))
    aligned = bool(rng.integers(0, 2))
    if aligned:
        if rng.integers(0, 2):
            w += w % 4
        sb = 4 * w + 16 * int(rng.integers(0, 5))
        sb += -sb % 16
        sy = w + 4 * int(rng.integers(0, 9)) + (-w % 4)
        sc = w // 2 + 2 * int(rng.integers(0, 9)) + (w // 2) % 2
        mis = (16 * int(rng.integers(0, 3)), 4 * int(rng.integers(0, 4)), 2 * int(rng.integers(0, 8)))
        quanta = (16, 4, 2)
    else:
        sb = 4 * w + 4 * int(rng.integers(0, 9))
        sy, sc = w + int(rng.integers(0, 9)), w // 2 + int(rng.integers(0, 9))
        mis = (4 * int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 8)))
        quanta = (4, 1, 1)
    even = bool(rng.integers(0, 2))
    offs = []
    for j, (stride, rows, q) in enumerate(((sb, h, quanta[0]), (sy, h, quanta[1]), (sc, h, quanta[2]))):  # a chroma slot: U then V, H rows
        pitch = stride * rows + q * int(rng.integers(0, 40))
        pitch += -pitch % q
        extra = [0] * n if even else list(np.cumsum([q * int(rng.integers(0, 9)) for _ in range(n)]))
        offs.append([GUARD + mis[j] + k * pitch + int(extra[k]) for k in range(n)])
    return PlanarLayout(w, h, (sb, sy, sc), *offs), pair, rng


def test_fuzz_reaches_both_kernels():
    """No GPU work: the predicate, restated above, sends a good share of the sequence to either kernel."""
    fast = sum(planar_fast_path(fuzz_case(i)[0]) for i in range(FUZZ_CASES))
    assert min(fast, FUZZ_CASES - fast) >= FUZZ_CASES // 8, fast


@pytest.mark.parametrize("chunk", range(FUZZ_CASES // FUZZ_CHUNK))
def test_fuzzed_geometry(harness, oracle, chunk):
    bad = []
    for i in range(chunk * FUZZ_CHUNK, (chunk + 1) * FUZZ_CHUNK):
        L, pair, rng = fuzz_case(i)
        pics = [ec.mixed_picture(int(rng.integers(0, 1 << 31)), L.w, L.h) if rng.integers(0, 2) else rng.integers(0, 1 << 32, (L.h, L.w), dtype=np.uint32)
                for _ in range(L.n)]
        res = harness.encode(L, ec.fill_input(L, lambda k: pics[k]), pair)
        plan = planar_plan(L)
        what = "case %d: %dx%d x %d, strides %d/%d/%d, pair %s" % (i, L.w, L.h, L.n, L.sb, L.sy, L.sc, pair)
        if (res.kernel, res.grid, res.block[0], res.launches, res.xcd_bands) != (plan["kernel"], tuple(plan["grid"]), plan["block"], plan["launches"], plan["xcd_bands"]):
            bad.append("%s: launched %s %s x %s, expected %s" % (what, res.kernel, res.grid, res.block, plan))
        want = [oracle.encode_nv12(p & 0xFFFFFF, L.w, L.h, *pair) for p in pics]
        bad += ["%s: %s" % (what, d) for d in differences(L, res, lambda k: (want[k][0],) + split(want[k][1]))]
    assert not bad, "\n".join(bad[:10])
