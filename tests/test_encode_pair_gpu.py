"""GPU tests (-m gpu) of BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA: bt709hip_encode[_batch] writing a BGRA surface's colour
frame AND its alpha frame from one launch.  Everything goes through the C ABI.  Expected bytes never come from the code under test:
the colour planes are the CPU oracle's (of the numpy-premultiplied picture where the premultiply option is on), the alpha plane is
tests/golden/alpha_luma.json's T[A], its chroma 128.  All five planes of a call live in ONE output slab that is canary-filled and
compared whole, so the guard bytes around every plane -- row padding, the gaps between pairs, the gap between U and V -- are part
of every comparison; every case asserts the kernel it was built to reach.  On a tree without the option each test fails at its
first set_option (BT709HIP_ERR_INVALID_ARG)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import encoder_cases as ec
import straight_alpha_cases as sc
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_APPLE, GAMMA_LINEAR, GAMMA_SRGB

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NV12, I420 = 0, 1
OPT_ROW_PAIRS, OPT_THREADS, OPT_XCD_BANDS, OPT_LAYOUT, OPT_PREMULTIPLY, OPT_WITH_ALPHA = 2, 3, 4, 6, 8, 12  # stated here
ALPHA_FORMAT = 3  # BT709HIP_FORMAT_BGRA8_ALPHA
FILL, GUARD = ec.FILL, 1024
PLANES = ("y", "c", "ay", "ac")
LUMA = np.array(json.load(open(os.path.join(HERE, "golden", "alpha_luma.json")))["luma"], np.uint8)
PAIRS = [(GAMMA_SRGB, GAMMA_APPLE), (GAMMA_SRGB, GAMMA_SRGB), (GAMMA_LINEAR, GAMMA_LINEAR)]


def kernel_name(layout, fast, premultiply):
    return "encode_bgra_alpha_" + ("i420" if layout == I420 else "nv12") + ("" if fast else "_blocks") + ("<premul>" if premultiply else "")


class Plan:
    """Where n pairs of w x h live.  The BGRA pictures in an input slab; the colour Y, colour chroma, alpha Y and alpha chroma planes
    in one arena each of ONE output slab.  pitches: (bgra, y, c, ay, ac); shift: bytes added to every offset of a plane (a
    misaligned pointer); steps: byte distance from one pair's plane to the next, per plane, negative = descending (default: the
    plane's span rounded up to 256, plus 256); spacing "table": a further multiple of 256 that grows and shrinks from pair to pair."""

    def __init__(self, w, h, n=1, layout=NV12, alpha_chroma=True, pitches=None, shift=None, steps=None, spacing="even"):
        self.w, self.h, self.n, self.layout, self.alpha_chroma = w, h, n, layout, alpha_chroma
        cw = w // 2 if layout == I420 else w
        self.pitch = dict(zip(("in",) + PLANES, pitches or (4 * w, w, cw, w, cw)))
        p = self.pitch
        chroma = lambda s: (h // 2) * s + (h // 2 - 1) * s + w // 2 if layout == I420 else (h // 2 - 1) * s + w
        self.span = {"in": (h - 1) * p["in"] + 4 * w, "y": (h - 1) * p["y"] + w, "c": chroma(p["c"]), "ay": (h - 1) * p["ay"] + w, "ac": chroma(p["ac"])}
        shift, steps = shift or {}, steps or {}
        self.off, cursor = {}, {"in": 0, "out": 0}
        for k in ("in",) + PLANES:
            slab = "in" if k == "in" else "out"
            step = steps.get(k, (self.span[k] + 255) // 256 * 256 + 256)
            assert abs(step) >= self.span[k], "pairs overlap"
            rel = [i * step if step > 0 else (n - 1 - i) * -step for i in range(n)]
            if spacing == "table":
                extra = np.cumsum([256 * ((i * i) % 5) for i in range(n)])
                rel = [r + int(e) for r, e in zip(rel, extra)]
            base = cursor[slab] + GUARD + shift.get(k, 0)
            self.off[k] = [base + r for r in rel]
            cursor[slab] = (base + max(rel) + self.span[k] + GUARD + 255) // 256 * 256
        self.in_bytes, self.out_bytes = cursor["in"], cursor["out"]

    def uniform(self):
        return all(len({b - a for a, b in zip(o, o[1:])}) <= 1 for o in self.off.values())

    def rows(self, slab, k, i, rows, width, plane_offset=0):
        return ec._rows_view(slab, self.off[k][i] + plane_offset, rows, self.pitch[k], width)

    def input_slab(self, pictures):
        slab = np.full(self.in_bytes, FILL, np.uint8)
        for i in range(self.n):
            self.rows(slab, "in", i, self.h, 4 * self.w)[:] = np.ascontiguousarray(pictures[i]).view(np.uint8).reshape(self.h, 4 * self.w)
        return slab

    def _chroma(self, slab, k, i, c):
        h2, w = self.h // 2, self.w
        if self.layout == I420:
            self.rows(slab, k, i, h2, w // 2)[:] = c[:, 0::2]
            self.rows(slab, k, i, h2, w // 2, h2 * self.pitch[k])[:] = c[:, 1::2]
        else:
            self.rows(slab, k, i, h2, w)[:] = c

    def expected(self, pictures, colour):
        """colour[i] = (y, cbcr) of pair i from the oracle -> the output slab as it must read back."""
        slab = np.full(self.out_bytes, FILL, np.uint8)
        for i in range(self.n):
            y, c = colour[i]
            self.rows(slab, "y", i, self.h, self.w)[:] = y
            self._chroma(slab, "c", i, c)
            self.rows(slab, "ay", i, self.h, self.w)[:] = LUMA[(np.asarray(pictures[i]) >> 24).astype(np.uint8)]
            if self.alpha_chroma:
                self._chroma(slab, "ac", i, np.full((self.h // 2, self.w), 128, np.uint8))
        return slab

    def describe(self, got, want):
        diff = np.flatnonzero(got != want)
        if diff.size == 0:
            return None
        p = int(diff[0])
        where = "outside every plane (guard bytes)"
        for k in PLANES:
            for i, o in enumerate(self.off[k]):
                if o <= p < o + self.span[k]:
                    where = "plane %s of pair %d, byte %d of it (pitch %d)" % (k, i, p - o, self.pitch[k])
        return "%d bytes differ, first at %d = %s: got %d, want %d" % (diff.size, p, where, got[p], want[p])


class Result:
    def __init__(self, slab, kernel, info):
        self.slab, self.kernel = slab, kernel
        self.record = (tuple(info.grid), tuple(info.block), info.launches, info.xcd_bands)


@pytest.fixture(scope="module")
def rig():
    import gpu_helpers
    return Rig(gpu_helpers.context())


class Rig(ec.Harness):
    """bt709hip_encode[_batch] on a Plan's slabs, the context's options set for the call and put back after it whatever happens
    (the context is the process's)."""

    def __init__(self, ctx):
        from metalbt709decoder_amd.decoder import DeviceBuffer
        self.capi, self.DeviceBuffer, self.ctx = _capi, DeviceBuffer, ctx
        self.lib, self.h = ctx.lib, ctx.handle

    def set(self, option, value):
        rc = self.lib.bt709hip_context_set_option(self.h, option, value)
        assert rc == _capi.OK, "bt709hip_context_set_option(%d, %d): %s" % (option, value, _capi.strerror(rc))

    def frames(self, P, d_out, which):
        ky, kc = which
        has_c = kc == "c" or P.alpha_chroma
        return [_capi.Frame(d_out + P.off[ky][i], P.pitch[ky], d_out + P.off[kc][i] if has_c else None, P.pitch[kc] if has_c else 0, P.w, P.h, 0, 0)
                for i in range(P.n)]

    def surfaces(self, P, d_in, fmt=_capi.FORMAT_BGRA8_SRGB):
        return (_capi.Surface * P.n)(*[_capi.Surface(d_in + o, P.pitch["in"], P.w, P.h, fmt, 0) for o in P.off["in"]])

    def run(self, P, pictures, pair, call, premultiply=False, options=()):
        """Uploads the pictures, canary-fills the output slab, sets the layout / premultiply / further options, runs call(d_in, d_out),
        reads the whole slab back."""
        d_in, d_out = (self.DeviceBuffer(self.ctx, nb, placement_tries=1) for nb in (P.in_bytes, P.out_bytes))
        opts = [(OPT_LAYOUT, P.layout, NV12), (OPT_PREMULTIPLY, int(premultiply), 0)] + [(o, v, d) for o, v, d in options]
        try:
            assert d_in.ptr % 256 == 0 and d_out.ptr % 256 == 0  # alignment is reasoned on offsets inside the slabs
            self._upload(d_in.ptr, P.input_slab(pictures))
            _capi.check(self.lib.bt709hip_memset(self.h, d_out.ptr, FILL, P.out_bytes, None))
            _capi.check(self.lib.bt709hip_stream_synchronize(self.h, None))
            for o, v, _ in opts:
                self.set(o, v)
            try:
                out = call(d_in.ptr, d_out.ptr)
            finally:
                for o, _, default in opts:
                    self.set(o, default)
                self.set(OPT_WITH_ALPHA, 0)
            return out if out is not None else self._download(d_out.ptr, P.out_bytes)
        finally:
            d_in.free()
            d_out.free()

    def paired_call(self, P, pair, d_in, d_out, stream=None, wait=1):
        surfs = self.surfaces(P, d_in)
        frames = (_capi.Frame * (2 * P.n))(*(self.frames(P, d_out, ("y", "c")) + self.frames(P, d_out, ("ay", "ac"))))
        self.set(OPT_WITH_ALPHA, 1)
        if P.n == 1:
            return self.lib.bt709hip_encode(self.h, surfs, frames, pair[0], pair[1], stream, wait)
        return self.lib.bt709hip_encode_batch(self.h, P.n, surfs, frames, pair[0], pair[1], stream, wait)

    def paired(self, P, pictures, pair, premultiply=False, options=()):
        box = {}

        def call(d_in, d_out):
            _capi.check(self.paired_call(P, pair, d_in, d_out), "paired bt709hip_encode")
            box["kernel"] = self.lib.bt709hip_last_kernel_name().decode()
            box["info"] = _capi.LaunchInfo()
            _capi.check(self.lib.bt709hip_last_launch_info(C.byref(box["info"])))
        slab = self.run(P, pictures, pair, call, premultiply, options)
        return Result(slab, box["kernel"], box["info"])

    def two_launches(self, P, pictures, pair, premultiply=False):
        """The product's own two launches on the same slabs: the colour encode, then the BGRA8_ALPHA encode."""
        def call(d_in, d_out):
            colour = (_capi.Frame * P.n)(*self.frames(P, d_out, ("y", "c")))
            alpha = (_capi.Frame * P.n)(*self.frames(P, d_out, ("ay", "ac")))
            _capi.check(self.lib.bt709hip_encode_batch(self.h, P.n, self.surfaces(P, d_in), colour, pair[0], pair[1], None, 1))
            _capi.check(self.lib.bt709hip_encode_batch(self.h, P.n, self.surfaces(P, d_in, ALPHA_FORMAT), alpha, GAMMA_LINEAR, GAMMA_LINEAR, None, 1))
        return self.run(P, pictures, pair, call, premultiply)


def oracle_planes(oracle, pictures, pair, premultiply=False):
    """The oracle's (y, cbcr) of each picture (premultiplied in numpy first where the option is on): one threaded call over the
    pictures stacked -- whole row pairs of each, and 2x2 blocks do not mix."""
    h, w = pictures[0].shape
    stack = np.concatenate([sc.premultiply(p) if premultiply else p for p in pictures])
    y, c = ec.threaded_encode(oracle, stack, w, h * len(pictures), *pair)
    return [(y[i * h:(i + 1) * h], c[i * h // 2:(i + 1) * h // 2]) for i in range(len(pictures))]


def random_pictures(seed, w, h, n=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << 32, (h, w), dtype=np.uint32) for _ in range(n)]


def check(rig, oracle, P, pictures, pair, fast, premultiply=False, options=(), label=""):
    res = rig.paired(P, pictures, pair, premultiply, options)
    assert res.kernel == kernel_name(P.layout, fast, premultiply), res.kernel
    diff = P.describe(res.slab, P.expected(pictures, oracle_planes(oracle, pictures, pair, premultiply)))
    assert diff is None, "%s: %s" % (label or res.kernel, diff)
    return res


# ------------------------------------------------------------------ every A in every lane position

def every_alpha_strip():
    """1024 x 2 words: along row 0, A runs through 0..255 four times, moved on by one every 256 columns, so every value sits in each
    of the four pixel positions of a quad; row 1 is the same moved on by 128.  Colour from a seeded generator."""
    x = np.arange(1024, dtype=np.uint32)[None, :]
    a = (x + x // 256 + np.array([[0], [128]], np.uint32)) & 255
    for row in range(2):
        for pos in range(4):
            assert np.unique(a[row, pos::4]).size == 256
    return ((a << 24) | np.random.default_rng(12).integers(0, 1 << 24, (2, 1024), dtype=np.uint32)).astype(np.uint32)


@pytest.mark.parametrize("premultiply", [False, True], ids=["plain", "premul"])
@pytest.mark.parametrize("alpha_chroma", [True, False], ids=["alpha-cbcr", "alpha-y-only"])
@pytest.mark.parametrize("layout", [NV12, I420], ids=["nv12", "i420"])
def test_every_alpha_in_every_lane_position(rig, oracle, layout, alpha_chroma, premultiply):
    strip = every_alpha_strip()
    P = Plan(1024, 2, layout=layout, alpha_chroma=alpha_chroma)
    res = check(rig, oracle, P, [strip], PAIRS[0], True, premultiply)
    plan = ec.expected_plan(1024, 2, 1)
    assert res.record == (tuple(plan["grid"]), (plan["block"], 1, 1), 1, 0)  # the colour encoder's plan for the size


# ------------------------------------------------------------------ the colour arithmetic of the new instantiations

@pytest.mark.parametrize("pair", PAIRS, ids=["%d-%d" % p for p in PAIRS])
def test_colour_arithmetic_threshold_edges_and_a_random_picture(rig, oracle, pair):
    edges = ec.edge_picture(ec.edge_blocks(oracle, pair))
    edges = (edges | (np.random.default_rng(5).integers(0, 256, edges.shape, dtype=np.uint32) << 24)).astype(np.uint32)
    h, w = edges.shape
    assert w % 4 == 0 and h % 2 == 0
    check(rig, oracle, Plan(w, h), [edges], pair, True, label="threshold edges %s" % (pair,))
    check(rig, oracle, Plan(256, 64, layout=I420), [ec.mixed_picture(18, 256, 64)], pair, True, label="random 256x64 %s" % (pair,))


# ------------------------------------------------------------------ against the product's own two launches

def test_equals_the_two_launches_on_a_1024_square(rig):
    pictures = random_pictures(1024, 1024, 1024)
    P = Plan(1024, 1024)
    one = rig.paired(P, pictures, PAIRS[0])
    assert one.kernel == "encode_bgra_alpha_nv12"
    two = rig.two_launches(P, pictures, PAIRS[0])
    assert P.describe(one.slab, two) is None, P.describe(one.slab, two)
    assert (one.slab != FILL).sum() > 2 * 1024 * 1024  # and something was written


# ------------------------------------------------------------------ the fast kernel's geometry

@pytest.mark.parametrize("w", [4, 8, 252, 260])
def test_fast_kernel_widths_at_height_2(rig, oracle, w):
    """One lane and 63 clamped idle ones; two lanes; 63 of a wave; a partial second wave."""
    for layout in (NV12, I420):
        pitches = None if w % 8 == 0 or layout == NV12 else (4 * w, w, w // 2 + 2, w, w // 2 + 2)  # W/2 odd: a 2-byte-aligned chroma pitch all the same
        check(rig, oracle, Plan(w, 2, layout=layout, pitches=pitches), random_pictures(w, w, 2), PAIRS[0], True)


def test_fast_kernel_short_last_group_of_row_pairs(rig, oracle):
    """Height 14 at three row pairs per workgroup: groups of 3, 3 and 1 -- the prefetch guard on a short last group."""
    res = check(rig, oracle, Plan(64, 14), random_pictures(14, 64, 14), PAIRS[1], True, options=[(OPT_ROW_PAIRS, 3, 0)])
    assert res.record[0][1] == 3


def test_fast_kernel_several_tiles(rig, oracle):
    """64-lane workgroups at width 520: 130 quads in tiles of 64, 64 and 2."""
    res = check(rig, oracle, Plan(520, 4, layout=I420), random_pictures(520, 520, 4), PAIRS[0], True, premultiply=True, options=[(OPT_THREADS, 64, 0)])
    assert res.record[0][0] == 3 and res.record[1][0] == 64


# ------------------------------------------------------------------ the general kernel

GENERAL = {
    "width-2": dict(w=2, h=4),
    "width-6": dict(w=6, h=2),
    "width-6-i420": dict(w=6, h=4, layout=I420),
    "odd-pitches": dict(w=16, h=4, pitches=(4 * 16 + 4, 17, 19, 21, 23)),
    "odd-pitches-i420": dict(w=16, h=4, layout=I420, pitches=(4 * 16, 17, 9, 19, 11)),
    "odd-alpha-pitch-alone": dict(w=16, h=4, pitches=(4 * 16, 16, 16, 18, 16)),
    "colour-y-pointer-off-by-2-alone": dict(w=16, h=4, shift={"y": 2}),
    "alpha-y-pointer-off-by-1-alone": dict(w=16, h=4, shift={"ay": 1}),
    "alpha-chroma-pointer-off-by-2-alone": dict(w=16, h=4, shift={"ac": 2}),
    "alpha-y-only-off-by-3": dict(w=16, h=4, alpha_chroma=False, shift={"ay": 3}),
}


@pytest.mark.parametrize("name", GENERAL)
def test_general_kernel(rig, oracle, name):
    """Everything the fast kernel's preconditions exclude takes encode_bgra_alpha_*_blocks and writes the same bytes; a
    misalignment of the colour side alone or of the alpha side alone is enough."""
    kw = dict(GENERAL[name])
    P = Plan(kw.pop("w"), kw.pop("h"), **kw)
    k = list(GENERAL).index(name)
    res = check(rig, oracle, P, random_pictures(100 + k, P.w, P.h), PAIRS[k % 3], False, premultiply=bool(k & 1), label=name)
    assert res.record[1][0] == ec.GENERAL_THREADS and res.record[2] == 1 and res.record[3] == 0
    # the aligned twin of the same size takes the fast kernel: it is the misalignment that selected _blocks
    if P.w % 4 == 0:
        assert rig.paired(Plan(P.w, P.h, layout=P.layout), random_pictures(1, P.w, P.h), PAIRS[0]).kernel == kernel_name(P.layout, True, False)


# ------------------------------------------------------------------ batches

def test_batch_of_3_through_the_pointer_table(rig, oracle):
    P = Plan(260, 6, n=3, spacing="table")
    assert not P.uniform()
    res = check(rig, oracle, P, random_pictures(3, 260, 6, 3), PAIRS[0], True)
    assert res.record[0][2] == 3 and res.record[2] == 1


def test_batch_of_16_through_the_pointer_table(rig, oracle):
    """The table's limit in this mode: BT709HIP_MAX_BATCH / 2 pairs; one more is refused."""
    P = Plan(16, 4, n=16, layout=I420, alpha_chroma=False, spacing="table")
    assert not P.uniform()
    res = check(rig, oracle, P, random_pictures(16, 16, 4, 16), PAIRS[1], True, premultiply=True)
    assert res.record[0][2] == 16
    P17 = Plan(16, 4, n=17, spacing="table")

    def refused(d_in, d_out):
        assert rig.paired_call(P17, PAIRS[0], d_in, d_out) == _capi.ERR_UNSUPPORTED
    slab = rig.run(P17, random_pictures(17, 16, 4, 17), PAIRS[0], refused)
    assert (slab == FILL).all()  # nothing was written


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "general"])
def test_batch_of_33_evenly_spaced_with_a_step_per_plane(rig, oracle, fast):
    """33 pairs, every plane its own step, the colour Y and the alpha Y planes descending; the general leg misaligns the alpha Y
    plane (an odd step keeps every second pair off 4 bytes)."""
    w, h = 16, 4
    steps = {"in": 4 * w * h + 64, "y": -(w * h + 32), "c": w * h // 2 + 48, "ay": -(w * h + (16 if fast else 17)), "ac": w * h // 2 + 80}
    P = Plan(w, h, n=33, steps=steps)
    assert P.uniform() and len({P.off[k][1] - P.off[k][0] for k in P.off}) == 5
    res = check(rig, oracle, P, random_pictures(33, w, h, 33), PAIRS[0], fast)
    assert res.record[2] == 1 and res.record[0][2 if fast else 2] == 33


def test_batch_of_67_under_the_xcd_band_map(rig, oracle):
    """67 evenly spaced 8x4 pairs with XCD_BANDS on: 64 under the band map and a plain tail of 3 behind advance_frames -- two
    launches, and every pair checked (the alpha planes must move with the colour planes through the split)."""
    n = ec.XCD_BAND_MIN_FRAMES + 3  # the build's kXcdBandMinFrames, restated by encoder_cases
    steps = {"ay": -(8 * 4 + 32)}
    for alpha_chroma in (True, False):
        P = Plan(8, 4, n=n, alpha_chroma=alpha_chroma, steps=steps)
        res = check(rig, oracle, P, random_pictures(67, 8, 4, n), PAIRS[0], True, options=[(OPT_XCD_BANDS, 1, 1)])
        assert res.record[2] == 2 and res.record[3] == 1 and res.record[0][2] == 8  # 64 / 8 pictures per band in the first launch


# ------------------------------------------------------------------ graph capture

def test_captured_after_one_prepare_and_replayed(rig, oracle):
    """bt709hip_encoder_prepare with the option on builds the pair's tables and T; the paired encode is then captured into a graph
    (one kernel node) and replayed once: the bytes of the direct call."""
    from metalbt709decoder_amd.decoder import CommandBuffer
    pair = (GAMMA_APPLE, GAMMA_SRGB)  # a pair nothing else in this module has built
    P = Plan(64, 8, n=2)
    pictures = random_pictures(77, 64, 8, 2)
    want = P.expected(pictures, oracle_planes(oracle, pictures, pair))
    lib, ctx = rig.lib, rig.ctx

    def call(d_in, d_out):
        rig.set(OPT_WITH_ALPHA, 1)
        _capi.check(lib.bt709hip_encoder_prepare(rig.h, pair[0], pair[1]))
        cb = ctx.commandQueue.commandBuffer(new_stream=True)
        try:
            assert isinstance(cb, CommandBuffer)
            cb.beginRecording()
            rc = rig.paired_call(P, pair, d_in, d_out, stream=cb.stream, wait=0)
            recorded = cb.endRecording()
            try:
                _capi.check(rc, "paired encode while capturing")
                assert lib.bt709hip_last_kernel_name() == b"encode_bgra_alpha_nv12"
                cb.waitUntilCompleted()
                assert (rig._download(d_out, P.out_bytes) == FILL).all()  # recorded, not run
                recorded.replay(cb)
                cb.waitUntilCompleted()
            finally:
                recorded.release()
        finally:
            cb.release()
    got = rig.run(P, pictures, pair, call)
    assert P.describe(got, want) is None, P.describe(got, want)
