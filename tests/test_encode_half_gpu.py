"""GPU tests (-m gpu) of BT709HIP_CTX_OPT_ENCODE_HALF_INPUT: bt709hip_encode[_batch] of RGBA16Float linear-light
surfaces into NV12 / I420, bit for bit.  Everything goes through the C ABI.  Expected bytes never come from the code under test:
they are tests/encode_half_cases.py's composition of oracle calls (or, for flat blocks, the oracle's (LINEAR, LINEAR) encode of the
BGRA8 twin).  The planes of a call live in ONE output slab that is canary-filled and compared whole, so row padding, the gaps
between pictures and the bytes behind every plane are part of every comparison; every case asserts the kernel it was built to
reach.  On a tree without the option each test fails at its first set_option (BT709HIP_ERR_INVALID_ARG)."""
import ctypes as C
import functools

import numpy as np
import pytest

import encode_half_cases as hc
import encoder_cases as ec
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_APPLE, GAMMA_LINEAR, GAMMA_SRGB

pytestmark = pytest.mark.gpu

NV12, I420 = hc.NV12, hc.I420
OPT_LAYOUT = 6
FAST, IN8, ODD = "fast", "general: texels 8-byte aligned only", "general: odd plane pitches"


class Result:
    def __init__(self, slab, kernel, info):
        self.slab, self.kernel = slab, kernel
        self.record = (tuple(info.grid), info.block[0], info.launches, info.xcd_bands)


class Rig(ec.Harness):
    """bt709hip_encode[_batch] of half pictures on an hc.Plan's slabs; the option and the layout are set for the call and put back
    after it whatever happens (the context is the process's)."""

    def set(self, option, value):
        rc = self.lib.bt709hip_context_set_option(self.h, option, value)
        assert rc == _capi.OK, "bt709hip_context_set_option(%d, %d): %s" % (option, value, _capi.strerror(rc))

    def encode(self, P, pictures, out_gamma, surfaces=None, in_gamma=GAMMA_LINEAR):
        """pictures: the texel arrays (uploaded into P's input slab), or None with `surfaces` = device surfaces to read instead"""
        d_out = self.DeviceBuffer(self.ctx, P.out_bytes, placement_tries=1)
        d_in = self.DeviceBuffer(self.ctx, P.in_bytes, placement_tries=1) if surfaces is None else None
        try:
            assert d_out.ptr % 256 == 0 and (d_in is None or d_in.ptr % 256 == 0)  # alignment is reasoned on offsets inside the slabs
            if surfaces is None:
                self._upload(d_in.ptr, P.input_slab(pictures))
                surfaces = [_capi.Surface(d_in.ptr + o, P.pitch["in"], P.w, P.h, hc.FORMAT_RGBA16F, 0) for o in P.off["in"]]
            _capi.check(self.lib.bt709hip_memset(self.h, d_out.ptr, hc.FILL, P.out_bytes, None))
            _capi.check(self.lib.bt709hip_stream_synchronize(self.h, None))
            surfs = (_capi.Surface * P.n)(*surfaces)
            frames = (_capi.Frame * P.n)(*[_capi.Frame(d_out.ptr + P.off["y"][i], P.pitch["y"], d_out.ptr + P.off["c"][i], P.pitch["c"], P.w, P.h, 0, 0)
                                           for i in range(P.n)])
            self.set(hc.OPT_HALF_INPUT, 1)
            self.set(OPT_LAYOUT, P.layout)
            try:
                if P.n == 1:
                    rc = self.lib.bt709hip_encode(self.h, surfs, frames, in_gamma, out_gamma, None, 1)
                else:
                    rc = self.lib.bt709hip_encode_batch(self.h, P.n, surfs, frames, in_gamma, out_gamma, None, 1)
            finally:
                self.set(OPT_LAYOUT, NV12)
                self.set(hc.OPT_HALF_INPUT, 0)
            _capi.check(rc, "bt709hip_encode of RGBA16F input")
            kernel = self.lib.bt709hip_last_kernel_name().decode()
            info = _capi.LaunchInfo()
            _capi.check(self.lib.bt709hip_last_launch_info(C.byref(info)))
            return Result(self._download(d_out.ptr, P.out_bytes), kernel, info)
        finally:
            d_out.free()
            if d_in is not None:
                d_in.free()


@pytest.fixture(scope="module")
def rig():
    import gpu_helpers
    return Rig(gpu_helpers)


@pytest.fixture(scope="module")
def expect(oracle):
    return hc.Expect(oracle)


def path_plan(path, w, h, n, layout, **kw):
    """The Plan that reaches `path`: fast = everything aligned; IN8 = every picture's texels at 8 mod 16; ODD = odd Y and chroma pitches"""
    cw = w // 2 if layout == I420 else w
    if path == IN8:
        return hc.Plan(w, h, n, layout, shift={"in": 8}, **kw)
    if path == ODD:
        return hc.Plan(w, h, n, layout, pitches=(8 * w, w + 1, cw + 1), **kw)
    return hc.Plan(w, h, n, layout, **kw)


def check(P, res, planes, kernel):
    assert res.kernel == kernel, res.kernel
    problem = P.describe(res.slab, P.expected(planes))
    assert problem is None, problem


# ------------------------------------------------------------------ 1: every half code

SIDE = 256
FIXED = (0x3400, 0x3A00)  # 0.25 and 0.75: the two channels that are not swept
ROLLS = (0, 1, SIDE, SIDE + 1)  # the code of pixel (y, x) is 256 y + x - roll: every code at each of the four block positions


@functools.lru_cache(None)
def sweep_pictures():
    """12 pictures of 256 x 256: R, G, B swept over all 65536 codes in turn, under the four rolls; A = the code, too"""
    out = []
    for channel in range(3):
        for roll in ROLLS:
            codes = np.roll(np.arange(65536, dtype=np.uint16), roll).reshape(SIDE, SIDE)
            t = np.empty((SIDE, SIDE, 4), np.uint16)
            others = iter(FIXED)
            for c in range(3):
                t[..., c] = codes if c == channel else next(others)
            t[..., 3] = codes[::-1]
            out.append(t)
    return out


_sweep_expected = {}


def sweep_expected(expect, out_gamma):
    if out_gamma not in _sweep_expected:
        _sweep_expected[out_gamma] = [expect.planes(t, out_gamma) for t in sweep_pictures()]
    return _sweep_expected[out_gamma]


@pytest.mark.parametrize("path", [FAST, IN8, ODD])
@pytest.mark.parametrize("layout", [NV12, I420])
@pytest.mark.parametrize("out_gamma", hc.OUT_GAMMAS)
def test_every_half_code(rig, expect, out_gamma, layout, path):
    """All 65536 codes -- NaNs, infinities, subnormals, both zeros, values above 1 and below 0 -- in each of R, G, B and at each
    block position, through the fast kernel and through the general kernel reached both ways."""
    pictures = sweep_pictures()
    P = path_plan(path, SIDE, SIDE, len(pictures), layout)
    res = rig.encode(P, pictures, out_gamma)
    check(P, res, sweep_expected(expect, out_gamma), hc.kernel_name(layout, path == FAST))


# ------------------------------------------------------------------ 2: every byte triple

SLICES = 16
SLICE_W, SLICE_H = 4096, 1024  # 2048 x 512 blocks = 2^20 triples; 32 MiB of texels


@pytest.mark.parametrize("part", range(SLICES))
def test_every_byte_triple(rig, expect, oracle, part):
    """2^24 flat blocks, one per (R, G, B) byte triple, each byte entered as one representative half (the smallest code that gives
    it) under each output gamma.  A flat block's expectation is the byte matrix alone, the same for the three gammas: the oracle's
    (LINEAR, LINEAR) encode of the BGRA8 twin."""
    t = (np.uint32(part) << 20) + np.arange(1 << 20, dtype=np.uint32).reshape(SLICE_H // 2, SLICE_W // 2)
    rgb = np.stack([(t >> 16) & 255, (t >> 8) & 255, t & 255], -1).astype(np.uint8)
    rgb_px = np.repeat(np.repeat(rgb, 2, 0), 2, 1)
    planes = ec.threaded_encode(oracle, hc.twin_words(rgb_px), SLICE_W, SLICE_H, GAMMA_LINEAR, GAMMA_LINEAR)
    P = hc.Plan(SLICE_W, SLICE_H)
    for out_gamma in hc.OUT_GAMMAS:
        lo, _ = hc.representatives(expect.code_table(out_gamma))
        texels = np.empty((SLICE_H, SLICE_W, 4), np.uint16)
        texels[..., :3] = lo[rgb_px]
        texels[..., 3] = hc.ONE
        check(P, rig.encode(P, [texels], out_gamma), [planes], "encode_rgba16f_nv12")


# ------------------------------------------------------------------ 3: both sides of every threshold

def threshold_pictures(expect, out_gamma, seed):
    """Two 64 x 64 pictures.  [0]: every pixel channel one of the 510 codes that sit on a threshold of F (for every byte k the
    smallest half that gives k and the largest that gives k - 1).  [1]: 1020 blocks (a, a, a, b), (a, a, b, b), (a, b, b, b),
    (b, a, a, a) with a, b the two neighbouring codes either side of threshold k -- a different k per channel -- so that the average
    lands on the quarter steps between them, which no single half reaches."""
    lo, hi = hc.representatives(expect.code_table(out_gamma))
    edges = np.concatenate([lo[1:], hi[:-1]])
    rng = np.random.default_rng(seed)
    per_pixel = np.empty((64, 64, 4), np.uint16)
    per_pixel[..., :3] = rng.choice(edges, (64, 64, 3))
    per_pixel[..., 3] = rng.choice(edges, (64, 64))
    assert set(edges.tolist()) <= set(per_pixel[..., :3].reshape(-1).tolist())  # 12288 draws of 510: every one is there
    blocks = np.zeros((32, 32, 2, 2, 4), np.uint16)  # [block row, block column, y, x, channel]
    patterns = [(0, 0, 0, 1), (0, 0, 1, 1), (0, 1, 1, 1), (1, 0, 0, 0)]  # TL, TR, BL, BR: 0 = a, 1 = b
    flat = blocks.reshape(1024, 2, 2, 4)
    for k in range(1, 256):
        for j, pattern in enumerate(patterns):
            for c, kc in enumerate((k, (k * 7 + 3) % 255 + 1, (k * 13 + 5) % 255 + 1)):
                a, b = hi[kc - 1], lo[kc]
                assert b == a + 1
                flat[(k - 1) * 4 + j, :, :, c] = np.array([b if s else a for s in pattern], np.uint16).reshape(2, 2)
    averages = blocks.transpose(0, 2, 1, 3, 4).reshape(64, 64, 4)
    return [per_pixel, averages]


@pytest.mark.parametrize("path", [FAST, IN8])
@pytest.mark.parametrize("out_gamma", hc.OUT_GAMMAS)
def test_both_sides_of_every_threshold(rig, expect, out_gamma, path):
    pictures = threshold_pictures(expect, out_gamma, 1900 + out_gamma)
    planes = [expect.planes(t, out_gamma) for t in pictures]
    for layout in (NV12, I420):
        P = path_plan(path, 64, 64, 2, layout)
        check(P, rig.encode(P, pictures, out_gamma), planes, hc.kernel_name(layout, path == FAST))


# ------------------------------------------------------------------ 4: geometry

def test_geometry(rig, expect):
    """Widths and heights around a lane, a wave, a tile and a row-pair group, padded pitches, canaries behind every plane and in
    every row's padding (the slab is compared whole), random halves from [-0.25, 1.25] plus specials."""
    rng = np.random.default_rng(1912)
    probe = hc.Plan(1024, 36)
    res = rig.encode(probe, [hc.random_texels(rng, 36, 1024)], GAMMA_APPLE)
    grid, lanes, launches, _ = res.record
    assert launches == 1 and grid[0] == 1 and res.kernel == "encode_rgba16f_nv12"
    tile = 2 * lanes           # pixels: a lane owns a 2x2 block
    group = 2 * (18 // grid[1])  # rows a workgroup walks
    assert tile == 1024 and group == 6, (tile, group)  # 512 lanes for one picture; 3 row pairs for a small launch
    case = 0
    for w in (2, 4, 6, 62, 64, 66, tile - 2, tile, tile + 2):
        for h in (2, 4, group - 2, group, group + 2):
            layout = (NV12, I420)[case % 2]
            fast = case % 3 != 2
            cw = w // 2 if layout == I420 else w
            # fast: pitches padded and still aligned (16 / 2 / 2 bytes; planar chroma needs none); general: odd plane pitches
            pitches = (8 * w + 32, w + 6, cw + (3 if layout == I420 else 4)) if fast else (8 * w + 8, w + 3, cw + 5)
            out_gamma = hc.OUT_GAMMAS[case % 3]
            case += 1
            P = hc.Plan(w, h, 1, layout, pitches=pitches)
            t = hc.random_texels(rng, h, w)
            res = rig.encode(P, [t], out_gamma)
            assert res.kernel == hc.kernel_name(layout, fast), (w, h, res.kernel)
            problem = P.describe(res.slab, P.expected([expect.planes(t, out_gamma)]))
            assert problem is None, (w, h, layout, fast, problem)


# ------------------------------------------------------------------ 5: batches

def half_plan(w, h, n, uniform):
    """The plan the header promises for the fast kernel: the BGRA8 encoder's for a picture twice as wide (a lane owns a block)"""
    plan = ec.expected_plan(2 * w, h, n, True, uniform)
    return (tuple(plan["grid"]), plan["block"], plan["launches"], plan["xcd_bands"])


@pytest.mark.parametrize("name,n,kw,uniform", [
    ("pointer table of 3", 3, dict(spacing="table"), False),
    ("70 evenly spaced: bands over 64, a plain tail of 6", 70, {}, True),
    ("descending spacing", 5, dict(steps={"in": -(8 * 64 * 16 + 256), "y": -(64 * 16 + 512), "c": -(64 * 8 + 256)}), True),
])
def test_batches(rig, expect, name, n, kw, uniform):
    w, h = 64, 16
    rng = np.random.default_rng(1950 + n)
    pictures = [hc.random_texels(rng, h, w) for _ in range(n)]
    planes = [expect.planes(t, GAMMA_SRGB) for t in pictures]
    for layout in (NV12, I420):
        P = hc.Plan(w, h, n, layout, **kw)
        res = rig.encode(P, pictures, GAMMA_SRGB)
        check(P, res, planes, hc.kernel_name(layout, True))
        assert res.record == half_plan(w, h, n, uniform), (name, res.record)
    if n == 70:
        assert res.record[2:] == (2, 1)  # two launches, the first under the band map


# ------------------------------------------------------------------ 6: round trip with the product's own decode

def test_round_trip_with_the_decode(rig, expect, oracle):
    """bt709hip_decode of a random NV12 frame into RGBA16F (gamma APPLE), then the half encode (LINEAR, APPLE) of that surface as
    it lies in device memory: the planes are the oracle's decode_nv12_rgba16f -> the helper's composition."""
    import gpu_helpers as gh
    import metalbt709decoder_amd as mb
    w, h = 64, 16
    y, c = gh.random_nv12(w, h, 1960, legal=True)
    ctx = gh.context()
    dec = gh.make_decoder(mb.MetalBT709GammaApple)
    tex = ctx.makeBGRATexture((w, h), pixelFormat=mb.MTLPixelFormatRGBA16Float)
    assert dec.decodeBT709(gh.make_buffer(y, c, dec.gamma), None, tex, ctx.commandQueue.commandBuffer(), None, w, h, True), dec.lastStatus
    texels = oracle.decode_nv12_rgba16f(GAMMA_APPLE, y, c).view(np.uint16)
    P = hc.Plan(w, h)
    res = rig.encode(P, None, GAMMA_APPLE, surfaces=[tex.surface()])
    want_y, want_c = expect.planes(texels, GAMMA_APPLE)
    check(P, res, [(want_y, want_c)], "encode_rgba16f_nv12")
    print("round trip: %.1f %% of the Y bytes return unchanged" % (100.0 * np.mean(want_y == y)))
