"""GPU tests (-m gpu): every batched kernel at any frame spacing (tests/batch_spacing_cases.py has the routes, the classes and
the layouts).  One test per (route, class): the frames' planes lie in two slabs of 4 GiB + 1 MiB as the class says,
the batched entry point runs once, and

  * the kernel (and, for the rescale routes, the tap form and persistence) on record is the route's -- the demoted one under a
    skewed step -- and bands-tail-descending took two launches, the first under the band map;
  * every frame's bytes equal the oracle's, bit for bit, and equal the single-frame call's on the same descriptors;
  * the run is made twice, with every input byte that is no sample at 0x00 and at 0xFF: the outputs are equal;
  * every output byte outside the pixels is what it was (the canary), the far classes' alias windows -- where a step cut to
    32 bits would have landed -- included.

A paired encode route (colour + alpha frames of one picture) passes 2n frames -- the colour frames, then the alpha frames -- and
its single call the two frames of one pair; all five planes take part in every comparison above.

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


# samples, backgrounds, what they must become and the slabs' windows: batch_spacing_cases (shared with tests/test_row_pitch_gpu.py)
want, assert_plane = bs.want, bs.assert_plane


def upload_inputs(rig, slabs, L, fill):
    bs.upload_inputs(rig, slabs.d_in, L, fill)


def reset_outputs(rig, slabs, L):
    return bs.reset_outputs(rig, slabs.d_out, L)


def collect(rig, slabs, L, before, label):
    return bs.collect(rig, slabs.d_out, L, before, label)


def scaled_record(rig):
    return bs.scaled_record(rig.lib)


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
