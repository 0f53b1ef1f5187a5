"""GPU tests (-m gpu) of BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA: bt709hip_encode[_batch] writing an RGBA16Float
surface's colour frame AND its alpha frame from one launch, bit for bit.  Everything goes through the C ABI.  Expected bytes never
come from the code under test: the colour planes are encode_half_cases.Expect.planes(t, go), the alpha planes
Expect.planes(grey(t[..., 3]), LINEAR) (tests/encode_half_alpha_cases.py).  All five planes of a call live in ONE output slab that is
canary-filled and compared whole, so row padding, the gaps between pairs and the bytes behind every plane are part of every
comparison; every case asserts the kernel it was built to reach.  On a tree without the option each test fails at its first
set_option (BT709HIP_ERR_INVALID_ARG)."""
import ctypes as C
import functools

import numpy as np
import pytest

import encode_half_alpha_cases as ac
import encode_half_cases as hc
import encoder_cases as ec
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_APPLE, GAMMA_LINEAR, GAMMA_SRGB

pytestmark = pytest.mark.gpu

NV12, I420 = hc.NV12, hc.I420
OPT_ROW_PAIRS, OPT_THREADS, OPT_XCD_BANDS, OPT_LAYOUT = 2, 3, 4, 6  # stated here
ALPHA_FORMAT, BGRA8_FORMAT = 3, 0
FILL = hc.FILL
FAST, IN8, ODD = "fast", "general: texels 8-byte aligned only", "general: odd alpha and colour pitches"


class Result:
    def __init__(self, slab, kernel, info):
        self.slab, self.kernel = slab, kernel
        self.record = (tuple(info.grid), info.block[0], info.launches, info.xcd_bands)


class Rig(ec.Harness):
    """bt709hip_encode[_batch] of half pictures on an ac.PairPlan's slabs; the options are set for the call and put back after it
    whatever happens (the context is the process's)."""

    def set(self, option, value):
        rc = self.lib.bt709hip_context_set_option(self.h, option, value)
        assert rc == _capi.OK, "bt709hip_context_set_option(%d, %d): %s" % (option, value, _capi.strerror(rc))

    def frames(self, P, d_out, pair):
        colour = [_capi.Frame(d_out + P.off["y"][i], P.pitch["y"], d_out + P.off["c"][i], P.pitch["c"], P.w, P.h, 0, 0) for i in range(P.n)]
        if not pair:
            return colour
        return colour + [_capi.Frame(d_out + P.off["ay"][i], P.pitch["ay"], d_out + P.off["ac"][i] if P.alpha_chroma else None,
                                     P.pitch["ac"] if P.alpha_chroma else 0, P.w, P.h, 0, 0) for i in range(P.n)]

    def call(self, P, surfs, d_out, out_gamma, pair, stream=None, wait=1):
        frames = self.frames(P, d_out, pair)
        frames = (_capi.Frame * len(frames))(*frames)
        if P.n == 1:
            return self.lib.bt709hip_encode(self.h, surfs, frames, GAMMA_LINEAR, out_gamma, stream, wait)
        return self.lib.bt709hip_encode_batch(self.h, P.n, surfs, frames, GAMMA_LINEAR, out_gamma, stream, wait)

    def run(self, P, pictures, body, surfaces=None, pair=True, options=()):
        """Uploads the pictures (or takes device `surfaces`), canary-fills the output slab, sets the options, runs
        body(surfs, d_out) and reads the whole slab back."""
        d_out = self.DeviceBuffer(self.ctx, P.out_bytes, placement_tries=1)
        d_in = self.DeviceBuffer(self.ctx, P.in_bytes, placement_tries=1) if surfaces is None else None
        opts = [(hc.OPT_HALF_INPUT, 1, 0), (ac.OPT_HALF_WITH_ALPHA, int(pair), 0), (OPT_LAYOUT, P.layout, NV12)] + list(options)
        try:
            assert d_out.ptr % 256 == 0 and (d_in is None or d_in.ptr % 256 == 0)  # alignment is reasoned on offsets inside the slabs
            if surfaces is None:
                self._upload(d_in.ptr, P.input_slab(pictures))
                surfaces = [_capi.Surface(d_in.ptr + o, P.pitch["in"], P.w, P.h, hc.FORMAT_RGBA16F, 0) for o in P.off["in"]]
            _capi.check(self.lib.bt709hip_memset(self.h, d_out.ptr, FILL, P.out_bytes, None))
            _capi.check(self.lib.bt709hip_stream_synchronize(self.h, None))
            surfs = (_capi.Surface * P.n)(*surfaces)
            for o, v, _ in opts:
                self.set(o, v)
            try:
                body(surfs, d_out.ptr)
            finally:
                for o, _, default in reversed(opts):
                    self.set(o, default)
            return self._download(d_out.ptr, P.out_bytes)
        finally:
            d_out.free()
            if d_in is not None:
                d_in.free()

    def encode(self, P, pictures, out_gamma, pair=True, surfaces=None, options=()):
        box = {}

        def body(surfs, d_out):
            _capi.check(self.call(P, surfs, d_out, out_gamma, pair), "bt709hip_encode of RGBA16F input, pair = %r" % pair)
            box["kernel"] = self.lib.bt709hip_last_kernel_name().decode()
            box["info"] = _capi.LaunchInfo()
            _capi.check(self.lib.bt709hip_last_launch_info(C.byref(box["info"])))
        slab = self.run(P, pictures, body, surfaces, pair, options)
        return Result(slab, box["kernel"], box["info"])


@pytest.fixture(scope="module")
def rig():
    import gpu_helpers
    return Rig(gpu_helpers)


@pytest.fixture(scope="module")
def expect(oracle):
    return hc.Expect(oracle)


def path_plan(path, w, h, n, layout, alpha_chroma=True, **kw):
    """The PairPlan that reaches `path`: fast = everything aligned; IN8 = every picture's texels at 8 mod 16; ODD = odd pitches of the
    four planes"""
    cw = w // 2 if layout == I420 else w
    if path == IN8:
        return ac.PairPlan(w, h, n, layout, alpha_chroma, shift={"in": 8}, **kw)
    if path == ODD:
        return ac.PairPlan(w, h, n, layout, alpha_chroma, pitches=(8 * w, w + 1, cw + 1, w + 3, cw + 5), **kw)
    return ac.PairPlan(w, h, n, layout, alpha_chroma, **kw)


def check(P, res, colour, alpha, kernel, label=""):
    assert res.kernel == kernel, (label, res.kernel)
    problem = P.describe(res.slab, P.expected(colour, alpha))
    assert problem is None, (label, problem)


def both(expect, pictures, out_gamma):
    return [expect.planes(t, out_gamma) for t in pictures], [ac.alpha_planes(expect, t) for t in pictures]


def half_plan(w, h, n, uniform):
    """The plan the header promises: the plain half encoder's, i.e. the BGRA8 encoder's for a picture twice as wide"""
    plan = ec.expected_plan(2 * w, h, n, True, uniform)
    return (tuple(plan["grid"]), plan["block"], plan["launches"], plan["xcd_bands"])


# ------------------------------------------------------------------ 1: every half code in A

SIDE = 256
ROLLS = (0, 1, SIDE, SIDE + 1)  # the code of pixel (y, x) is 256 y + x - roll: every code at each of the four block positions
SWEEP_GAMMA = GAMMA_SRGB


@functools.lru_cache(None)
def sweep_pictures():
    """4 pictures of 256 x 256: A swept over all 65536 codes under the four rolls; R, G, B noise with the specials"""
    rng = np.random.default_rng(2101)
    out = []
    for roll in ROLLS:
        t = hc.random_texels(rng, SIDE, SIDE)
        t[..., 3] = np.roll(np.arange(65536, dtype=np.uint16), roll).reshape(SIDE, SIDE)
        out.append(t)
    return out


_sweep_expected = []


def sweep_expected(expect):
    if not _sweep_expected:
        _sweep_expected.extend(both(expect, sweep_pictures(), SWEEP_GAMMA))
    return _sweep_expected


@pytest.mark.parametrize("path", [FAST, IN8, ODD])
@pytest.mark.parametrize("alpha_chroma", [True, False], ids=["alpha-cbcr", "alpha-y-only"])
@pytest.mark.parametrize("layout", [NV12, I420], ids=["nv12", "i420"])
def test_every_half_code_in_alpha(rig, expect, layout, alpha_chroma, path):
    """All 65536 codes -- NaNs, infinities, subnormals, both zeros, values above 1 and below 0 -- in A at each block position,
    through the fast kernel and through the general kernel reached both ways; both frames are checked."""
    pictures = sweep_pictures()
    colour, alpha = sweep_expected(expect)
    P = path_plan(path, SIDE, SIDE, len(pictures), layout, alpha_chroma)
    check(P, rig.encode(P, pictures, SWEEP_GAMMA), colour, alpha, ac.kernel_name(layout, path == FAST))


# ------------------------------------------------------------------ 2: the colour frame is the option-0 call's

@pytest.mark.parametrize("out_gamma", hc.OUT_GAMMAS)
def test_colour_planes_equal_the_option_0_call(rig, expect, out_gamma):
    rng = np.random.default_rng(2102 + out_gamma)
    t = hc.random_texels(rng, 64, 128)
    for layout in (NV12, I420):
        P = ac.PairPlan(128, 64, 1, layout)
        one = rig.encode(P, [t], out_gamma)
        zero = rig.encode(P, [t], out_gamma, pair=False)
        assert one.kernel == ac.kernel_name(layout, True) and zero.kernel == hc.kernel_name(layout, True)
        assert np.array_equal(one.slab[:P.colour_bytes], zero.slab[:P.colour_bytes])
        assert np.all(zero.slab[P.colour_bytes:] == FILL)  # at 0 the second frame is not looked at
        assert one.record == zero.record                   # the plain half encoder's plan
        check(P, one, *both(expect, [t], out_gamma), ac.kernel_name(layout, True))


# ------------------------------------------------------------------ 3: geometry

def test_fast_kernel_widths_at_height_2(rig, expect):
    """One lane and 63 clamped idle ones; two; three; 127 of two waves; a partial third wave"""
    rng = np.random.default_rng(2103)
    for k, w in enumerate((2, 4, 6, 254, 258)):
        for layout in (NV12, I420):
            t = hc.random_texels(rng, 2, w)
            P = ac.PairPlan(w, 2, 1, layout, alpha_chroma=bool((k + layout) & 1))
            check(P, rig.encode(P, [t], hc.OUT_GAMMAS[k % 3]), *both(expect, [t], hc.OUT_GAMMAS[k % 3]), ac.kernel_name(layout, True), label=w)


def test_fast_kernel_short_last_group_of_row_pairs(rig, expect):
    """Height 14 at three row pairs per workgroup: groups of 3, 3 and 1 -- the prefetch guard on a short last group"""
    t = hc.random_texels(np.random.default_rng(2104), 14, 64)
    P = ac.PairPlan(64, 14)
    res = rig.encode(P, [t], GAMMA_APPLE, options=[(OPT_ROW_PAIRS, 3, 0)])
    check(P, res, *both(expect, [t], GAMMA_APPLE), "encode_rgba16f_alpha_nv12")
    assert res.record[0][1] == 3


def test_fast_kernel_several_tiles(rig, expect):
    """64-lane workgroups at width 260: 130 blocks in tiles of 64, 64 and 2"""
    t = hc.random_texels(np.random.default_rng(2105), 4, 260)
    P = ac.PairPlan(260, 4, 1, I420)
    res = rig.encode(P, [t], GAMMA_LINEAR, options=[(OPT_THREADS, 64, 0)])
    check(P, res, *both(expect, [t], GAMMA_LINEAR), "encode_rgba16f_alpha_i420")
    assert res.record[0][0] == 3 and res.record[1] == 64


GENERAL = {
    "alpha-y-pointer-odd-alone": dict(shift={"ay": 1}),
    "alpha-y-pitch-odd-alone": dict(pitches=(8 * 16, 16, 16, 17, 16)),
    "alpha-chroma-pitch-odd-alone": dict(pitches=(8 * 16, 16, 16, 16, 19)),
    "alpha-chroma-pointer-odd-alone": dict(shift={"ac": 1}),
    "alpha-y-only-pointer-odd": dict(alpha_chroma=False, shift={"ay": 3}),
    "colour-y-pointer-odd-alone": dict(shift={"y": 1}),
}


@pytest.mark.parametrize("name", GENERAL)
def test_general_kernel(rig, expect, name):
    """Everything the fast kernel's preconditions exclude takes encode_rgba16f_alpha_*_blocks and writes the same bytes; a
    misalignment of the alpha side alone is enough.  (Planar alpha chroma takes byte stores: an odd U pointer or pitch stays fast.)"""
    k = list(GENERAL).index(name)
    t = hc.random_texels(np.random.default_rng(2110 + k), 4, 16)
    out_gamma = hc.OUT_GAMMAS[k % 3]
    colour, alpha = both(expect, [t], out_gamma)
    for layout in (NV12, I420):
        kw = dict(GENERAL[name])
        if layout == I420 and "pitches" in kw:
            p = kw["pitches"]
            kw["pitches"] = (p[0], p[1], 8, p[3], p[4] - 8)
        P = ac.PairPlan(16, 4, 1, layout, **kw)
        fast = layout == I420 and "alpha-chroma" in name
        res = rig.encode(P, [t], out_gamma)
        check(P, res, colour, alpha, ac.kernel_name(layout, fast), label=(name, layout))
        if not fast:
            assert res.record[1] == ec.GENERAL_THREADS and res.record[2:] == (1, 0)
    # the aligned twin of the same size takes the fast kernel: it is the misalignment that selected _blocks
    assert rig.encode(ac.PairPlan(16, 4), [t], out_gamma).kernel == "encode_rgba16f_alpha_nv12"


# ------------------------------------------------------------------ 4: batches

def test_batch_of_3_through_the_pointer_table(rig, expect):
    rng = np.random.default_rng(2120)
    pictures = [hc.random_texels(rng, 6, 130) for _ in range(3)]
    P = ac.PairPlan(130, 6, 3, spacing="table")
    assert not P.uniform()
    res = rig.encode(P, pictures, GAMMA_APPLE)
    check(P, res, *both(expect, pictures, GAMMA_APPLE), "encode_rgba16f_alpha_nv12")
    assert res.record == half_plan(130, 6, 3, False)


def test_batch_of_16_through_the_pointer_table_and_17_refused(rig, expect):
    """The table's limit in this mode: BT709HIP_MAX_BATCH / 2 pairs; one more is refused and nothing is written."""
    rng = np.random.default_rng(2121)
    pictures = [hc.random_texels(rng, 4, 16) for _ in range(17)]
    P = ac.PairPlan(16, 4, 16, I420, alpha_chroma=False, spacing="table")
    assert not P.uniform()
    res = rig.encode(P, pictures[:16], GAMMA_SRGB)
    check(P, res, *both(expect, pictures[:16], GAMMA_SRGB), "encode_rgba16f_alpha_i420")
    assert res.record[0][2] == 16
    P17 = ac.PairPlan(16, 4, 17, spacing="table")

    def refused(surfs, d_out):
        assert rig.call(P17, surfs, d_out, GAMMA_SRGB, True) == _capi.ERR_UNSUPPORTED
    assert np.all(rig.run(P17, pictures, refused) == FILL)


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "general"])
def test_batch_of_33_evenly_spaced_with_a_step_per_plane(rig, expect, fast):
    """33 pairs, every plane its own step, the colour Y and the alpha Y planes descending; the general leg gives the alpha Y plane
    an odd step (every second pair off 2 bytes)."""
    w, h = 16, 4
    rng = np.random.default_rng(2122)
    pictures = [hc.random_texels(rng, h, w) for _ in range(33)]
    steps = {"in": 8 * w * h + 64, "y": -(w * h + 32), "c": w * h // 2 + 48, "ay": -(w * h + (16 if fast else 17)), "ac": w * h // 2 + 80}
    P = ac.PairPlan(w, h, 33, steps=steps)
    assert P.uniform() and len({P.off[k][1] - P.off[k][0] for k in P.off}) == 5
    res = rig.encode(P, pictures, GAMMA_APPLE)
    check(P, res, *both(expect, pictures, GAMMA_APPLE), ac.kernel_name(NV12, fast))
    assert res.record[2] == 1 and res.record[0][2] == 33


def test_batch_of_67_under_the_xcd_band_map(rig, expect):
    """67 evenly spaced 64x16 pairs with XCD_BANDS on: 64 under the band map and a plain tail of 3 behind advance_frames -- two
    launches, and every pair checked (the alpha planes must move with the colour planes through the split)."""
    n = ec.XCD_BAND_MIN_FRAMES + 3
    rng = np.random.default_rng(2123)
    pictures = [hc.random_texels(rng, 16, 64) for _ in range(n)]
    colour, alpha = both(expect, pictures, GAMMA_SRGB)
    for alpha_chroma, layout in ((True, NV12), (False, I420)):
        P = ac.PairPlan(64, 16, n, layout, alpha_chroma, steps={"ay": -(64 * 16 + 256)})
        res = rig.encode(P, pictures, GAMMA_SRGB, options=[(OPT_XCD_BANDS, 1, 1)])
        check(P, res, colour, alpha, ac.kernel_name(layout, True))
        assert res.record == half_plan(64, 16, n, True) and res.record[2:] == (2, 1)


# ------------------------------------------------------------------ 5: the three launches it replaces

def test_equals_the_three_launches_on_a_1024_square(rig):
    """Colour = the plain half encode; alpha = bt709hip_render_scaled 1:1 into a BGRA8 scratch surface followed by a BGRA8_ALPHA
    encode of it.  Finite texels in [-0.25, 1.25]: pass 2's 0 * inf differs by definition."""
    side = 1024
    t = np.random.default_rng(2130).uniform(-0.25, 1.25, (side, side, 4)).astype(np.float16).view(np.uint16)
    P = ac.PairPlan(side, side)
    one = rig.encode(P, [t], GAMMA_APPLE)
    assert one.kernel == "encode_rgba16f_alpha_nv12"
    lib = rig.lib
    scratch = rig.DeviceBuffer(rig.ctx, 4 * side * side, placement_tries=1)
    try:
        def three(surfs, d_out):
            frames = rig.frames(P, d_out, True)
            _capi.check(rig.call(P, surfs, d_out, GAMMA_APPLE, False), "the plain half encode")
            bgra = _capi.Surface(scratch.ptr, 4 * side, side, side, BGRA8_FORMAT, 0)
            _capi.check(lib.bt709hip_render_scaled(rig.h, C.byref(surfs[0]), C.byref(bgra), None, 1), "bt709hip_render_scaled 1:1")
            bgra.format = ALPHA_FORMAT
            _capi.check(lib.bt709hip_encode(rig.h, C.byref(bgra), C.byref(frames[1]), GAMMA_LINEAR, GAMMA_LINEAR, None, 1), "the BGRA8_ALPHA encode")
        two = rig.run(P, [t], three, pair=False)
    finally:
        scratch.free()
    problem = P.describe(one.slab, two)
    assert problem is None, problem
    assert (one.slab != FILL).sum() > 2 * side * side  # and something was written


# ------------------------------------------------------------------ 6: round trip with the product's own decode

def test_round_trip_with_the_decode(rig, expect, oracle):
    """bt709hip_decode of a frame AND an alpha frame into RGBA16F, then the paired encode of that surface as it lies in device memory.
    The alpha frame holds every code 0..255 in every block position.  Both frames are the oracle's decode_nv12_rgba16f -> the
    definition; the alpha frame's video-range codes return to themselves."""
    import gpu_helpers as gh
    import metalbt709decoder_amd as mb
    w, h = 1024, 2
    y, c = gh.random_nv12(w, h, 2140, legal=True)
    x = np.arange(w, dtype=np.uint32)[None, :]
    a = ((x + x // 256 + np.array([[0], [128]], np.uint32)) & 255).astype(np.uint8)
    for row in range(2):
        for pos in range(2):
            assert np.unique(a[row, pos::2]).size == 256
    ctx = gh.context()
    dec = gh.make_decoder(mb.MetalBT709GammaSRGB, has_alpha=True)  # hasAlphaChannel forces the sRGB function, as the reference (MetalBT709Decoder.m:165-169)
    assert dec.gamma == mb.MetalBT709GammaSRGB == GAMMA_SRGB
    tex = ctx.makeBGRATexture((w, h), pixelFormat=mb.MTLPixelFormatRGBA16Float)
    assert dec.decodeBT709(gh.make_buffer(y, c, dec.gamma), gh.make_alpha_buffer(a), tex, ctx.commandQueue.commandBuffer(), None, w, h, True), dec.lastStatus
    texels = oracle.decode_nv12_rgba16f(GAMMA_SRGB, y, c, alpha=a).view(np.uint16)
    P = ac.PairPlan(w, h)
    res = rig.encode(P, None, GAMMA_SRGB, surfaces=[tex.surface()])
    colour, alpha = both(expect, [texels], GAMMA_SRGB)
    check(P, res, colour, alpha, "encode_rgba16f_alpha_nv12")
    assert np.array_equal(alpha[0][0], np.clip(a, 16, 235))  # the CPU composition: tests/test_encode_half_alpha_cpu.py


# ------------------------------------------------------------------ 7: graph capture

def test_captured_after_one_prepare_and_replayed(rig, expect):
    """bt709hip_encoder_prepare(LINEAR, go) with the option on builds the from_linear table and T; the paired half encode is then
    captured into a graph and replayed once: the bytes of the definition."""
    from metalbt709decoder_amd.decoder import CommandBuffer
    rng = np.random.default_rng(2150)
    pictures = [hc.random_texels(rng, 8, 64) for _ in range(2)]
    P = ac.PairPlan(64, 8, 2)
    lib, ctx = rig.lib, rig.ctx

    def body(surfs, d_out):
        _capi.check(lib.bt709hip_encoder_prepare(rig.h, GAMMA_LINEAR, GAMMA_SRGB))
        cb = ctx.commandQueue.commandBuffer(new_stream=True)
        try:
            assert isinstance(cb, CommandBuffer)
            cb.beginRecording()
            rc = rig.call(P, surfs, d_out, GAMMA_SRGB, True, stream=cb.stream, wait=0)
            recorded = cb.endRecording()
            try:
                _capi.check(rc, "paired half encode while capturing")
                assert lib.bt709hip_last_kernel_name() == b"encode_rgba16f_alpha_nv12"
                cb.waitUntilCompleted()
                assert np.all(rig._download(d_out, P.out_bytes) == FILL)  # recorded, not run
                recorded.replay(cb)
                cb.waitUntilCompleted()
            finally:
                recorded.release()
        finally:
            cb.release()
    got = rig.run(P, pictures, body)
    problem = P.describe(got, P.expected(*both(expect, pictures, GAMMA_SRGB)))
    assert problem is None, problem
