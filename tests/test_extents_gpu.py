"""GPU tests (-m gpu): every kernel at its tallest frame, its longest batch and a frame of a million columns
(tests/extent_cases.py has the routes, the extent classes and the layouts; DESIGN.md 4, "Extents").  One test per (route, class):
the items' planes lie in two slabs of extent_cases.SLAB_BYTES, the batched entry point runs once, and

  * the kernel (and, for the rescale routes, the tap form and persistence the class's ratios select) on record is the route's;
  * the launch on record has the shape the class is about: the ragged last workgroup of the kernels that stack row pairs in
    blockDim.y, a full gridDim.y of the others, 65528 frames under the XCD-band map and 7 behind it (or, with the map off, a
    grid.z of 65535), cols x strips x 65535 items of the persistent rescale kernels, more than one tile of a wide frame;
  * every item's bytes equal the oracle's, bit for bit, and -- the six items of extent_cases.SINGLES of a long batch, every item
    of the others -- the single-frame call's on the same descriptors;
  * the run is made twice, with every input byte that is no sample at 0x00 and at 0xFF: the outputs are equal;
  * every output byte outside the pixels is what it was.

One past each limit (extent_cases.PAIRS_REFUSED) the batched and the single-frame call are refused with the code on record in
extent_cases.refusal, the kernel name stays what it was and nothing is written.  Not run, with the reason:
extent_cases.CLASSES_NOT_RUN."""
import ctypes as C

import numpy as np
import pytest

import batch_spacing_cases as bs
import encoder_cases as enc
import extent_cases as ec
import row_pitch_cases as rp
from metalbt709decoder_amd import _capi
from test_batch_spacing_gpu import GAMMA, Slabs, alpha_luma, gh, rig, tabs  # noqa: F401  (the module fixtures; the slabs are this module's own)

pytestmark = pytest.mark.gpu

CHW_QUADS = ("chw-quads-u8", "chw-quads-f16-alpha", "chw-quads-f32-i420")  # launch_decode's plan over the planar CHW kernels
CHW_ENCODE = ("encode-chw-f16", "encode-chw-u8-i420")                      # launch_encode's own plan
ENCODE_HALF = ("encode-half", "encode-half-pair")  # launch_encode's plan of a BGRA8 picture twice as wide (a 2x2 block a lane)
ENCODE_FAMILIES = ("encode-i420", "convert-packed", "convert-point-i420", "encode-pair") + ENCODE_HALF  # launch_encode's plan, fast kernels
ENCODE_GENERAL = ("encode-i420-blocks-premul", "convert-packed-blocks", "encode-pair-i420-blocks", "encode-half-i420-blocks")
STACKED = ("quads", "quads-over", "i420", "half-wide") + CHW_QUADS  # narrow frames: row pairs stacked in blockDim.y (quads_rows_per_block)
FULL_GRID_Y = ("half-narrow", "encode-blocks", "encode-chw-f32-blocks", "interleave-wide", "interleave-bytes", "deinterleave-wide", "deinterleave-bytes") + ENCODE_GENERAL
WALKS_ROW_PAIRS = ("encode-fast", "encode-alpha-y") + CHW_ENCODE + ENCODE_FAMILIES  # 3 to 9 row pairs a workgroup
TILED = ("quads", "quads-over", "i420", "rgba16f-alpha", "half-wide", "half-rep-alpha", "encode-fast", "encode-alpha-y") + CHW_QUADS + CHW_ENCODE + ENCODE_FAMILIES
GENERAL_DECODE = ("blocks", "chw-blocks-f16")                   # grid-strided over the row pairs; the frames live in gridDim.y
RECORDS_LAUNCH = ("decode", "half", "encode", "interleave", "deinterleave")  # bt709hip_last_launch_info


@pytest.fixture(scope="module")
def slabs(rig):  # noqa: F811
    ptrs = []
    try:
        for _ in range(2):
            p = C.c_void_p()
            _capi.check(rig.lib.bt709hip_malloc(rig.h, ec.SLAB_BYTES, C.byref(p)), "bt709hip_malloc of %d bytes" % ec.SLAB_BYTES)
            assert p.value % 256 == 0
            ptrs.append(p.value)
        yield Slabs(*ptrs)
    finally:
        for p in ptrs:
            _capi.check(rig.lib.bt709hip_free(rig.h, p))


@pytest.fixture(scope="module")
def decoders(rig):  # noqa: F811
    """(route name, options) -> its decoder (None for the context-level entry points), made on first use."""
    made = {}

    def get(route):
        if route.entry in ("render", "encode", "interleave", "deinterleave"):
            return None
        key = (route.name, route.options)
        if key not in made:
            d = rig.decoder(over=route.over, options=route.options, setup=False, gamma=GAMMA[route.gamma], has_alpha=route.alpha)
            if route.entry == "unconvert":
                _capi.check(rig.lib.bt709hip_decoder_set_alpha_fill(d, 0))  # the oracle's +unconvert: leaves byte 3 at 0
            _capi.check(rig.lib.bt709hip_decoder_setup(d), "decoder setup")
            made[key] = d
        return made[key]
    return get


def _rows_walked(route):
    """What the route's kernel counts in gridDim.y: row pairs (the 2:1 kernels: output rows, as many), chroma rows."""
    return route.size[1] if ec.shuffles(route) else route.size[1] // 2


def _ceil(a, b):
    return -(-a // b)


def _scaled_info(lib):
    info = _capi.ScaledLaunchInfo()
    _capi.check(lib.bt709hip_last_scaled_launch_info(C.byref(info)))
    return info


def _check_record(rig, L, label):  # noqa: F811
    """The launch on record against what the class is about."""
    base, route, cls, n = L.base, L.route, L.cls, L.n
    name = base.name
    if route.taps is not None or route.entry == "render":
        info = _scaled_info(rig.lib)
        cols, strips = _ceil(route.out_size[0], 256), _ceil(route.out_size[1], info.rows)
        assert info.items == cols * strips * n, (label, info.items, cols, strips, n)
        if route.taps is not None:
            assert (info.taps, info.persistent) == route.taps, (label, info.taps, info.persistent)
            if info.persistent:
                assert tuple(info.grid)[1:] == (1, 1) and info.grid[0] <= info.items
            else:
                assert tuple(info.grid) == (cols, strips, n), (label, tuple(info.grid))
        else:
            assert tuple(info.grid) == (cols, strips, n), (label, tuple(info.grid))
        if cls in ("wide", "wide-down"):
            assert cols == (4097 if cls == "wide" else 4)
        return
    if route.entry not in RECORDS_LAUNCH:
        return
    grid, block, launches, bands = rig.launch()
    rows = _rows_walked(route)
    if name in ENCODE_HALF + ("encode-half-i420-blocks",):
        # RGBA16Float input: the BGRA8 encoder's plan of a picture TWICE AS WIDE, same height and count (the general kernel's: of
        # the picture itself, a 2x2 block a lane either way) -- from the restated plan, not from the record
        fast = name in ENCODE_HALF
        plan = enc.expected_plan(2 * route.size[0] if fast else route.size[0], route.size[1], n, fast=fast, bands=cls != "longest-unbanded")
        assert (tuple(grid), block[0], launches, bands) == (tuple(plan["grid"]), plan["block"], plan["launches"], plan["xcd_bands"]), (label, grid, block, launches, bands, plan)
    if cls == "tallest":
        assert launches == 1, (label, launches)
        if name in STACKED:  # the ragged last workgroup: its loads are clamped to the last row pair
            by = block[1]
            assert by > 1 and rows % by != 0 and grid[1] == _ceil(rows, by), (label, grid, block, rows)
        elif name in FULL_GRID_Y:
            assert grid[1] == rows and rows >= ec.MOST_ROWS - 1, (label, grid, rows)
        elif name in WALKS_ROW_PAIRS:
            assert grid[1] in [_ceil(rows, k) for k in range(3, 10)], (label, grid, rows)
        elif name in GENERAL_DECODE:
            assert grid[1:] == (1, 1), (label, grid)
    elif cls in ("longest", "longest-unbanded"):
        if base.bands and cls == "longest":
            assert launches == 2 and grid[2] == 8191 and bands == 1, (label, grid, block, launches, bands)
        elif name in GENERAL_DECODE:  # the general path's frames live in gridDim.y
            assert launches == 1 and grid[1] == n and bands == 0, (label, grid, launches)
        elif name == "half-rep-alpha":
            assert launches == 1 and grid == (3, 1, 1), (label, grid)
        else:
            assert launches == 1 and grid[2] == n and bands == 0, (label, grid, block, launches, bands)
    elif cls == "wide":
        assert launches == 1, (label, launches)
        if name in TILED and name != "half-rep-alpha":
            assert grid[0] > 1, (label, grid, block)


class _EncoderMap:
    """BT709HIP_CTX_OPT_XCD_BANDS at 0 for the encoder's longest-unbanded case, the default back afterwards."""

    def __init__(self, rig, L):  # noqa: F811
        self.rig, self.on = rig, L.cls == "longest-unbanded" and L.route.entry == "encode"

    def __enter__(self):
        if self.on:
            _capi.check(self.rig.lib.bt709hip_context_set_option(self.rig.h, _capi.CTX_OPT_XCD_BANDS, 0))

    def __exit__(self, *exc):
        if self.on:
            _capi.check(self.rig.lib.bt709hip_context_set_option(self.rig.h, _capi.CTX_OPT_XCD_BANDS, 1))


@pytest.mark.parametrize("name,cls", ec.PAIRS_RUN, ids=["%s-%s" % rc for rc in ec.PAIRS_RUN])
def test_route_at_extent(rig, slabs, decoders, oracle, tabs, alpha_luma, name, cls):  # noqa: F811
    L = ec.build(name, cls)  # asserts, on the CPU, that every item lies inside the window, apart from the others
    route, lib, n = L.route, rig.lib, L.n
    call = rp.Call(L, slabs.d_in, slabs.d_out)
    dec = decoders(route)
    label = "%s, %s" % (name, cls)
    try:
        with _EncoderMap(rig, L):
            runs = {}
            for fill in (0x00, 0xFF):
                ec.upload_inputs(rig, slabs.d_in, L, fill)
                before = ec.reset_outputs(rig, slabs.d_out, L)
                _capi.check(call.batch(lib, rig.h, dec), label)
                assert rig.kernel() == route.kernel, (label, rig.kernel())
                _check_record(rig, L, label)
                runs[fill] = ec.collect(rig, slabs.d_out, L, before, "%s, fill %#04x" % (label, fill))
        wanted = ec.expected(L, oracle, tabs, alpha_luma)
        for plane, got in runs[0x00].items():
            ec.assert_items(got, wanted[plane], None, "%s, plane %s" % (label, plane))
            assert np.array_equal(runs[0xFF][plane], got), "%s, plane %s: fill 0xFF against fill 0x00" % (label, plane)

        if call.planes:  # no batched entry point: the run above was the per-frame call
            return
        before = ec.reset_outputs(rig, slabs.d_out, L)  # the single-frame call on the same descriptors (the inputs still hold the 0xFF fill)
        chosen = ec.SINGLES if n > 1 else [0]
        for i in chosen:
            _capi.check(call.single(lib, rig.h, dec, i), "%s, single call on item %d" % (label, i))
        singles = ec.collect(rig, slabs.d_out, L, before, label + ", single calls")
        for plane, got in singles.items():
            batch = runs[0x00][plane]
            if not np.array_equal(got[chosen], batch[chosen]):
                k = next(i for i in chosen if not np.array_equal(got[i], batch[i]))
                bs.assert_plane(got[k], batch[k], "%s, item %d, plane %s: the single call against the batch" % (label, k, plane))
    finally:
        ec.forget(L)


@pytest.mark.parametrize("name,cls", ec.PAIRS_REFUSED, ids=["%s-%s" % rc for rc in ec.PAIRS_REFUSED])
def test_first_refused_extent(rig, slabs, decoders, name, cls):  # noqa: F811
    """One past the limit: the code on record from the batched call (and, too-tall, from the single-frame call), the kernel name
    on record is what it was, the output window holds what it held."""
    L = ec.build(name, cls)
    call = rp.Call(L, slabs.d_in, slabs.d_out)
    dec = decoders(L.route)
    before = ec.reset_outputs(rig, slabs.d_out, L)
    on_record = rig.kernel()
    assert call.batch(rig.lib, rig.h, dec) == ec.refusal(L.route, cls), (name, cls)
    if cls == "too-tall":
        assert call.single(rig.lib, rig.h, dec, 0) == _capi.ERR_UNSUPPORTED, (name, cls)
    rig.sync()
    assert rig.kernel() == on_record
    assert np.array_equal(rig.download(slabs.d_out, L.total["out"]), before), (name, cls)
