"""GPU tests (-m gpu): every batched kernel at any frame spacing (tests/batch_spacing_cases.py has the routes, the classes and
the layouts).  One test per (route, class): the frames' planes lie in two slabs of 4 GiB + 1 MiB as the class says,
the batched entry point runs once, and

  * the kernel (and, for the rescale routes, the tap form and persistence) on record is the route's -- the demoted one under a
    skewed step -- and bands-tail-descending took two launches, the first under the band map;
  * every frame's bytes equal the oracle's, bit for bit, and equal the single-frame call's on the same descriptors;
  * the run is made twice, with every input byte that is no sample at 0x00 and at 0xFF: the outputs are equal;
  * every output byte outside the pixels is what it was (the canary), the far classes' alias windows -- where a step cut to
    32 bits would have landed -- included.

The slabs are allocated once (module fixture), never filled or read whole: the host touches the layouts' windows only.
Not run, with the reason: batch_spacing_cases.CLASSES_NOT_RUN (the skewed classes on routes whose pointers must be texel
aligned or whose kernel is already the general one -- variant_cases.LAUNCH_CASES' step_pad pins that one -- plane-skew on
routes with one plane a side, the split launch on kernels that never split)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import batch_spacing_cases as bs
import metalbt709decoder_amd as mb
import over_cases as oc
import variant_cases as vc
from metalbt709decoder_amd import _capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GAMMA = {bs.GAMMA_APPLE: mb.MetalBT709GammaApple, bs.GAMMA_SRGB: mb.MetalBT709GammaSRGB, bs.GAMMA_LINEAR: mb.MetalBT709GammaLinear}
SINGLES = 3  # frames of a long batch that are also run through the single-frame call: the first, the middle, the last


@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


@pytest.fixture(scope="module")
def rig(gh):
    r = vc.Rig(gh)
    yield r
    r.close()


@pytest.fixture(scope="module")
def tabs(oracle):
    return oc.tables(oracle)


@pytest.fixture(scope="module")
def alpha_luma():
    return np.array(json.load(open(os.path.join(HERE, "golden", "alpha_luma.json")))["luma"], np.uint8)


class Slabs:
    def __init__(self, d_in, d_out):
        self.d_in, self.d_out = d_in, d_out


@pytest.fixture(scope="module")
def slabs(rig):
    """The input and the output slab, bs.SLAB_BYTES each, for every test of the module; the canary is put on the output slab
    by the device.  Freed when the module is done."""
    ptrs = []
    try:
        for _ in range(2):
            p = C.c_void_p()
            _capi.check(rig.lib.bt709hip_malloc(rig.h, bs.SLAB_BYTES, C.byref(p)), "bt709hip_malloc of %d bytes" % bs.SLAB_BYTES)
            assert p.value % 256 == 0
            ptrs.append(p.value)
        _capi.check(rig.lib.bt709hip_memset(rig.h, ptrs[1], bs.CANARY, bs.SLAB_BYTES, None))
        rig.sync()
        yield Slabs(*ptrs)
    finally:
        for p in ptrs:
            _capi.check(rig.lib.bt709hip_free(rig.h, p))


@pytest.fixture(scope="module")
def decoders(rig):
    """route name -> its decoder (None for the context-level entry points), made on first use."""
    made = {}

    def get(route):
        if route.name not in made:
            if route.entry in ("render", "encode"):
                made[route.name] = None
            else:
                d = rig.decoder(over=route.over, options=route.options, setup=False, gamma=GAMMA[route.gamma], has_alpha=route.alpha)
                if route.entry == "unconvert":
                    _capi.check(rig.lib.bt709hip_decoder_set_alpha_fill(d, 0))  # the oracle's +unconvert: leaves byte 3 at 0
                _capi.check(rig.lib.bt709hip_decoder_setup(d), "decoder setup")
                made[route.name] = d
        return made[route.name]
    return get


# ------------------------------------------------------------------ samples, backgrounds and what they must become

_data, _want = {}, {}


def frame_data(route, k):
    """plane name -> (rows, row_bytes) bytes of frame k: random, another for every frame and route."""
    key = (route.name, k)
    if key not in _data:
        rng = np.random.default_rng(100000 + 1000 * bs.ROUTES.index(route) + k)
        w, h = route.size
        d = {}
        for p in route.ins:
            if route.entry == "render" and route.in_fmt == bs.F16:  # finite halves, some above 1.0
                d[p.name] = (rng.random((h, w, 4)) * 1.25).astype(np.float16).view(np.uint8).reshape(h, 8 * w)
            elif route.entry == "unconvert":  # Y | Cb << 8 | Cr << 16
                d[p.name] = rng.integers(0, 1 << 24, (h, w), dtype=np.uint32).view(np.uint8).reshape(h, 4 * w)
            else:
                d[p.name] = rng.integers(0, 256, (p.rows, p.row_bytes), dtype=np.uint8)
        _data[key] = d
    return _data[key]


def background(route, i):
    ow, oh = route.out_size
    return np.random.default_rng(7000 + i).integers(0, 256, (oh, 4 * ow), dtype=np.uint8)


def _interleave(uv_planes):
    """The NV12 twin of an I420 "cbcr" plane (U's rows, then V's)."""
    half = uv_planes.shape[0] // 2
    c = np.empty((half, 2 * uv_planes.shape[1]), np.uint8)
    c[:, 0::2], c[:, 1::2] = uv_planes[:half], uv_planes[half:]
    return c


def want(route, oracle, tabs, T, k, bg_index):
    """plane name -> (rows, row_bytes) bytes frame k's samples must become (over the background of target bg_index, where the
    route reads its destination): the oracle call the route's own tests use."""
    key = (route.name, k, bg_index if route.reads_destination else None)
    if key in _want:
        return _want[key]
    d = frame_data(route, k)
    w, h = route.size
    ow, oh = route.out_size
    g = route.gamma
    if route.entry in ("decode", "half", "scaled"):
        y, a = d["y"], d.get("alpha")
        c = _interleave(d["cbcr"]) if route.name == "i420" else d["cbcr"]
        if route.entry == "decode":
            out = oracle.decode_nv12_rgba16f(g, y, c, a).view(np.uint8).reshape(h, 8 * w) if route.fmt == bs.F16 else oracle.decode_nv12(g, y, c, alpha=a)
        elif route.entry == "half":
            out = oracle.decode_nv12_half(g, y, c, alpha=a)
        elif dict(route.options).get(_capi.OPT_SCALE_INTERMEDIATE) == bs.F16:
            out = oracle.render_scaled(oracle.decode_nv12_rgba16f(g, y, c, a), ow, oh)
        else:
            out = oracle.decode_nv12_scaled(g, y, c, ow, oh, alpha=a)
        assert out is not None
        if route.reads_destination:
            out = oc.composite_over(out.reshape(oh, ow, 4), background(route, bg_index).reshape(oh, ow, 4), *tabs).reshape(oh, 4 * ow)
        res = {"out": out}
    elif route.entry == "render":
        src = d["in"].view(np.float16).reshape(h, w, 4) if route.in_fmt == bs.F16 else d["in"]
        res = {"out": oracle.render_scaled(src, ow, oh)}
    elif route.entry == "unconvert":
        res = {"out": oracle.unconvert_packed(g, d["in"].view(np.uint32).reshape(h, w), w, h).view(np.uint8).reshape(h, 4 * w)}
    elif route.in_fmt == bs.ALPHA8:
        res = {"y": T[d["bgra"].reshape(h, w, 4)[:, :, 3]]}
    else:
        y, c = oracle.encode_nv12(d["bgra"].view(np.uint32).reshape(h, w), w, h, route.pair[0], route.pair[1])
        res = {"y": y, "cbcr": c}
    for name, arr in res.items():
        p = route.plane(name)
        res[name] = np.ascontiguousarray(arr).reshape(p.rows, p.row_bytes)
    _want[key] = res
    return res


# ------------------------------------------------------------------ the slabs' windows

def upload_inputs(rig, slabs, L, fill):
    """Every input window: `fill` in every byte that is no sample (row padding, guard bands, the alias windows)."""
    for lo, hi in L.in_windows:
        host = np.full(hi - lo, fill, np.uint8)
        for p in L.route.ins:
            for i in range(L.n):
                off = L.in_off[p.name][i]
                if lo <= off < hi:
                    host[p.index(off - lo)] = frame_data(L.route, L.source[i])[p.name]
        rig.upload(slabs.d_in + lo, host)


def reset_outputs(rig, slabs, L):
    """Every output window: the canary, and where the route reads its destination background i in the pixels of target i.
    -> the windows' bytes as uploaded."""
    before = []
    for lo, hi in L.out_windows:
        host = np.full(hi - lo, bs.CANARY, np.uint8)
        if L.route.reads_destination:
            p = L.route.plane("out")
            for i, off in enumerate(L.out_off["out"]):
                if lo <= off < hi:
                    host[p.index(off - lo)] = background(L.route, i)
        rig.upload(slabs.d_out + lo, host)
        before.append(host)
    return before


def collect(rig, slabs, L, before, label):
    """-> {(plane name, frame): (rows, row_bytes)} of every output window; every byte outside the pixels must be what it was."""
    got = {}
    for (lo, hi), was in zip(L.out_windows, before):
        raw = rig.download(slabs.d_out + lo, hi - lo)
        outside = np.ones(raw.size, bool)
        for p in L.route.outs:
            for i, off in enumerate(L.out_off[p.name]):
                if lo <= off < hi:
                    idx = p.index(off - lo)
                    got[(p.name, i)] = raw[idx]
                    outside[idx] = False
        stray = np.flatnonzero(outside & (raw != was))
        assert stray.size == 0, "%s: %d bytes written outside the pixels, first at slab offset %d (window %d..%d%s)" % (
            label, stray.size, lo + stray[0], lo, hi, ", an alias window" if (lo, hi) in L.out_alias else "")
    assert len(got) == L.n * len(L.route.outs)
    return got


def assert_plane(got, wanted, label):
    if not np.array_equal(got, wanted):
        bad = np.argwhere(got != wanted)
        r, x = bad[0]
        raise AssertionError("%s: differs first at row %d, byte %d (got %d, want %d); %d of %d bytes differ"
                             % (label, r, x, got[r, x], wanted[r, x], len(bad), got.size))


def scaled_record(rig):
    info = _capi.ScaledLaunchInfo()
    _capi.check(rig.lib.bt709hip_last_scaled_launch_info(C.byref(info)))
    return info.taps, info.persistent


# ------------------------------------------------------------------ the tests

@pytest.mark.parametrize("name,cls", bs.PAIRS_RUN, ids=["%s-%s" % rc for rc in bs.PAIRS_RUN])
def test_route_at_spacing(rig, slabs, decoders, oracle, tabs, alpha_luma, name, cls):
    route = bs.ROUTE[name]
    L = bs.build(route, cls)  # asserts, on the CPU, that every window lies inside the slabs, apart from the others
    call = bs.Call(route, L, slabs.d_in, slabs.d_out)
    dec, lib, n = decoders(route), rig.lib, L.n
    label = "%s, %s" % (name, cls)
    kernel, taps = route.skew[bs.SKEW[cls]] if cls in bs.SKEW else (route.kernel, route.taps)

    if route.entry == "render" and not L.uniform:  # no pointer table behind this entry point: refused, nothing written
        upload_inputs(rig, slabs, L, 0x00)
        before = reset_outputs(rig, slabs, L)
        assert call.batch(lib, rig.h, dec) == _capi.ERR_UNSUPPORTED
        rig.sync()
        for (lo, hi), was in zip(L.out_windows, before):
            assert np.array_equal(rig.download(slabs.d_out + lo, hi - lo), was)
        return

    runs = {}
    for fill in (0x00, 0xFF):
        upload_inputs(rig, slabs, L, fill)
        before = reset_outputs(rig, slabs, L)
        _capi.check(call.batch(lib, rig.h, dec), label)
        assert rig.kernel() == kernel, (label, rig.kernel())
        if taps is not None:
            assert scaled_record(rig) == taps, (label, scaled_record(rig))
        if cls == "bands-tail-descending":
            grid, block, launches, bands = rig.launch()
            assert launches == 2 and bands == 1, (label, grid, block, launches, bands)
        elif route.entry in ("decode", "encode"):
            assert rig.launch()[2] == 1, (label, rig.launch())
        runs[fill] = collect(rig, slabs, L, before, "%s, fill %#04x" % (label, fill))
    for (plane, i), got in runs[0x00].items():
        assert_plane(got, want(route, oracle, tabs, alpha_luma, L.source[i], i)[plane], "%s, frame %d, plane %s" % (label, i, plane))
        assert_plane(runs[0xFF][(plane, i)], got, "%s, frame %d, plane %s: fill 0xFF against fill 0x00" % (label, i, plane))

    # the single-frame call on the same descriptors (the inputs still hold the 0xFF fill)
    before = reset_outputs(rig, slabs, L)
    chosen = sorted({0, n // 2, n - 1}) if n > SINGLES else list(range(n))
    for i in chosen:
        _capi.check(call.single(lib, rig.h, dec, i), "%s, single call on frame %d" % (label, i))
    singles = collect(rig, slabs, L, before, label + ", single calls")
    for (plane, i), got in singles.items():
        if i in chosen:
            assert_plane(got, runs[0x00][(plane, i)], "%s, frame %d, plane %s: the single call against the batch" % (label, i, plane))


@pytest.mark.parametrize("name", ["quads", "i420"])
def test_coalescing_queue_of_two_with_the_second_frame_lower(rig, slabs, oracle, tabs, alpha_luma, name):
    """BT709HIP_OPT_COALESCE = 2: two single-frame bt709hip_decode calls on one stream, the second frame at the LOWER address in
    every plane, go out as one launch -- two frames, so the uniform path with negative steps -- when the queue fills; then
    bt709hip_decoder_flush."""
    route = bs.ROUTE[name]
    L = bs.build(route, "descending-2")
    call = bs.Call(route, L, slabs.d_in, slabs.d_out)
    lib = rig.lib
    dec = rig.decoder(options=route.options + ((_capi.OPT_COALESCE, 2),), gamma=GAMMA[route.gamma], has_alpha=False)
    stream = C.c_void_p()
    _capi.check(lib.bt709hip_stream_create(rig.h, C.byref(stream)))
    try:
        upload_inputs(rig, slabs, L, 0x00)
        before = reset_outputs(rig, slabs, L)
        for i in range(2):
            _capi.check(call.single(lib, rig.h, dec, i, stream=stream, wait=0))
        _capi.check(lib.bt709hip_decoder_flush(dec, stream))
        rig.sync(stream)
        assert rig.kernel() == route.kernel
        grid, block, launches, bands = rig.launch()
        assert launches == 1 and grid[2] == 2, (grid, block, launches)  # grid.z: both frames in the one launch
        got = collect(rig, slabs, L, before, name + ", coalesced")
    finally:
        _capi.check(lib.bt709hip_stream_destroy(rig.h, stream))
    for (plane, i), g in got.items():
        assert_plane(g, want(route, oracle, tabs, alpha_luma, i, i)[plane], "%s coalesced, frame %d" % (name, i))
