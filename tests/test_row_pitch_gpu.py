"""GPU tests (-m gpu): every kernel where row x pitch passes 2^31 and 2^32 (tests/row_pitch_cases.py has the routes, the pitch
classes and the layouts).  One test per (route, class): two frames' planes lie in two slabs of 4 GiB + 1 MiB at
the class's pitches, the batched entry point runs once, and

  * the kernel (and, for the rescale routes, the tap form and persistence) on record is the route's: the new pitches are
    congruent to the route's own mod 16;
  * every frame's bytes equal the oracle's, bit for bit, and equal the single-frame call's on the same descriptors;
  * the run is made twice, with every input byte that is no sample (the rows' guard bands, the input alias windows) at 0x00 and
    at 0xFF: the outputs are equal;
  * every output byte of every window outside the pixels is the canary, the alias windows -- where a row offset taken as a signed
    32-bit number (past-2^31) or cut to 32 bits (past-2^32) would have landed -- included.

The any-ratio and pass-2 routes form row offsets in 32 bits and refuse planes of 2 GiB or more: under-2-GiB runs them at the
largest pitches they accept, at-2-GiB asserts the refusal at the first pitch they do not, one plane at a time.

Every past-2^31 test comes before the past-2^32 tests (row_pitch_cases.PAIRS_RUN): a signed 32-bit mistake fails a comparison
inside the slab under the first and would leave the slab under the second.  The slabs are allocated once (module fixture),
never filled or read whole: the host touches the layouts' windows only.  Not run, with the reason: row_pitch_cases.CLASSES_NOT_RUN."""
import numpy as np
import pytest

import batch_spacing_cases as bs
import row_pitch_cases as rp
from metalbt709decoder_amd import _capi
from test_batch_spacing_gpu import alpha_luma, decoders, gh, rig, slabs, tabs  # noqa: F401  (the module fixtures: this module gets its own slabs)

pytestmark = pytest.mark.gpu


def _decoder(decoders, route):  # noqa: F811
    return None if route.entry in ("interleave", "deinterleave") else decoders(route)


@pytest.mark.parametrize("name,cls", rp.PAIRS_RUN, ids=["%s-%s" % rc for rc in rp.PAIRS_RUN])
def test_route_at_pitch(rig, slabs, decoders, oracle, tabs, alpha_luma, name, cls):  # noqa: F811
    base = rp.ROUTE[name]
    L = rp.build(base, cls)  # asserts, on the CPU, that every window lies inside the slabs, apart from the others
    route, lib, n = L.route, rig.lib, L.n
    call = rp.Call(L, slabs.d_in, slabs.d_out)
    dec = _decoder(decoders, base)
    label = "%s, %s" % (name, cls)

    runs = {}
    for fill in (0x00, 0xFF):
        bs.upload_inputs(rig, slabs.d_in, L, fill)
        before = bs.reset_outputs(rig, slabs.d_out, L)
        _capi.check(call.batch(lib, rig.h, dec), label)
        assert rig.kernel() == route.kernel, (label, rig.kernel())
        if route.taps is not None:
            assert bs.scaled_record(lib) == route.taps, (label, bs.scaled_record(lib))
        runs[fill] = bs.collect(rig, slabs.d_out, L, before, "%s, fill %#04x" % (label, fill))
    for (plane, i), got in runs[0x00].items():
        bs.assert_plane(got, bs.want(route, oracle, tabs, alpha_luma, i, i)[plane], "%s, frame %d, plane %s" % (label, i, plane))
        bs.assert_plane(runs[0xFF][(plane, i)], got, "%s, frame %d, plane %s: fill 0xFF against fill 0x00" % (label, i, plane))

    if call.planes:  # no batched entry point: the run above was the per-frame calls
        return
    before = bs.reset_outputs(rig, slabs.d_out, L)  # the single-frame call on the same descriptors (the inputs still hold the 0xFF fill)
    for i in range(n):
        _capi.check(call.single(lib, rig.h, dec, i), "%s, single call on frame %d" % (label, i))
    singles = bs.collect(rig, slabs.d_out, L, before, label + ", single calls")
    for (plane, i), got in singles.items():
        bs.assert_plane(got, runs[0x00][(plane, i)], "%s, frame %d, plane %s: the single call against the batch" % (label, i, plane))


@pytest.mark.parametrize("name,plane", rp.AT_LIMIT, ids=["%s-at-2-GiB-%s" % a for a in rp.AT_LIMIT])
def test_first_refused_pitch(rig, slabs, decoders, name, plane):  # noqa: F811
    """One plane at the smallest pitch of its residue with rows x pitch >= 2^31: BT709HIP_ERR_UNSUPPORTED from the batched and the
    single-frame call, the kernel name on record is what it was, the output windows hold what they held."""
    base = rp.ROUTE[name]
    L = rp.build(base, "at-2-GiB", plane)
    call = rp.Call(L, slabs.d_in, slabs.d_out)
    dec = _decoder(decoders, base)
    before = bs.reset_outputs(rig, slabs.d_out, L)
    on_record = rig.kernel()
    assert call.batch(rig.lib, rig.h, dec) == _capi.ERR_UNSUPPORTED, (name, plane)
    assert call.single(rig.lib, rig.h, dec, 0) == _capi.ERR_UNSUPPORTED, (name, plane)
    rig.sync()
    assert rig.kernel() == on_record
    for (lo, hi), was in zip(L.out_windows, before):
        assert np.array_equal(rig.download(slabs.d_out + lo, hi - lo), was), (name, plane, lo, hi)
