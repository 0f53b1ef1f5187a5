"""Row-pitch addressing, the parts that need no GPU (tests/row_pitch_cases.py; the GPU half is tests/test_row_pitch_gpu.py): the
layout builder's own guarantees for every (route, class) the GPU file runs, and -- on the shim built against the fake HIP runtime,
which dereferences nothing, so the true boundaries are free to test --

  * the pitch rule at the 32-bit edge for EVERY stride argument of every entry point (every pitch <= 2^32 - 1, the
    alpha frame's included): 2^32 and 2^32 + a valid pitch are BT709HIP_ERR_STRIDE with nothing launched, the largest 32-bit pitch
    the plane's alignment allows is not a pitch error;
  * plane_fits (rows x pitch < 2^31, the any-ratio and pass-2 entry points) from both sides for every plane."""
import pytest

import batch_spacing_cases as bs
import row_pitch_cases as rp
from metalbt709decoder_amd import _capi
from test_batch_spacing_cpu import IN_BASE, OUT_BASE, FakeRig, fake  # noqa: F401  (`fake` is the module's fixture)


# ------------------------------------------------------------------ the builder

def test_every_layout_passes_its_self_checks():
    """Layout.check() for every (route, class) and every at-2-GiB plane of the GPU file, and beyond check(): the pitches are the
    extreme ones of their residue, what the host touches stays small, and the two past- classes really differ by 2^32."""
    assert len(set(rp.PAIRS_RUN)) == len(rp.PAIRS_RUN) == 2 * 34 + 8 and len(set(rp.AT_LIMIT)) == len(rp.AT_LIMIT) == 24
    for name, cls in rp.PAIRS_RUN:
        L = rp.build(rp.ROUTE[name], cls)
        assert L.n == 2
        for which in ("in", "out"):
            planes, off, windows, alias = L.side(which)
            assert sum(hi - lo for lo, hi in windows) < (1 << 18)
            for p in planes:
                last = (p.rows - 1) * p.stride
                if cls in rp.PAST:
                    boundary = rp.TWO31 if cls == "past-2^31" else rp.TWO32
                    assert 0 <= last - boundary - rp.alias_gap(p) < 17 * (p.rows - 1)  # rounded up to a whole pitch of the residue, no further
                    assert (p.stacked > 1) == (p.name in ("out", "chw") and bool(rp.ROUTE[name].chw))  # a planar CHW surface: its planes in one
                    assert max(off[p.name]) + last + p.row_bytes > rp.TWO32     # the last row's ADDRESS is past 2^32 in both
                else:
                    assert p.rows * p.stride < rp.TWO31 <= p.rows * (p.stride + 16)
    for name, victim in rp.AT_LIMIT:
        L = rp.build(rp.ROUTE[name], "at-2-GiB", victim)
        v = L.route.plane(victim)
        assert v.rows * v.stride >= rp.TWO31 > v.rows * (v.stride - 16)
    # the order the GPU file runs them in: every past-2^31 pair first
    firsts = [i for i, (_, c) in enumerate(rp.PAIRS_RUN) if c == "past-2^32"]
    assert all(c == "past-2^31" for _, c in rp.PAIRS_RUN[:firsts[0]]) and firsts[0] == 34


def test_every_route_runs_every_class_or_says_why_not():
    run = set(rp.PAIRS_RUN) | {(name, "at-2-GiB") for name, _ in rp.AT_LIMIT}
    assert [r.name for r in rp.ROUTES[:len(bs.ROUTES)]] == [r.name for r in bs.ROUTES]  # every route of the batch-spacing module
    for r in rp.ROUTES:
        for cls in rp.CLASSES:
            assert ((r.name, cls) in run) != bool(rp.CLASSES_NOT_RUN.get((r.name, cls))), (r.name, cls)
    # the list holds the two contract-based groups and nothing else
    for (name, cls), reason in rp.CLASSES_NOT_RUN.items():
        assert reason and (cls in rp.PAST) == rp.limited(rp.ROUTE[name]) and (cls in rp.LIMIT) != rp.limited(rp.ROUTE[name])
    assert sorted(r.name for r in rp.ROUTES if rp.limited(r)) == ["render-bgra8", "render-rgba16f", "scaled-chw-f32-alpha", "scaled-chw-u8", "scaled-f16", "scaled-once", "scaled-over", "scaled-wide"]
    # the encoder's families form 64-bit row products: none is limited, each runs both past- classes, the alpha frame's planes included
    for name, planes in (("encode-pair", ["bgra", "y", "cbcr", "alpha_y", "alpha_cbcr"]), ("encode-pair-i420-blocks", ["bgra", "y", "cbcr", "alpha_y"]),
                         ("encode-half-pair", ["rgba16f", "y", "cbcr", "alpha_y", "alpha_cbcr"]), ("convert-packed", ["bgra", "y"])):
        r = rp.ROUTE[name]
        assert not rp.limited(r) and [p.name for p in r.ins + r.outs] == planes and all((name, c) in run for c in rp.PAST)
    assert {(n, p) for n, p in rp.AT_LIMIT if n == "scaled-over"} == {("scaled-over", p) for p in ("y", "cbcr", "alpha", "out")}


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture
def fake_rig(fake):
    r = FakeRig(fake)
    yield r
    r.close()


def _decoder(rig, route):
    return None if route.entry in ("interleave", "deinterleave") else rig.decoder(route)


def _run(rig, route, strides, which):
    """(return code, kernels logged) of the batched (`which` "batch") or the single-frame call of `route` with `strides`."""
    call = rp.Call(rp.unchecked(route, strides), IN_BASE, OUT_BASE)
    mark = rig.lib.fake_hip_log_size()
    dec = _decoder(rig, route)
    rc = call.batch(rig.lib, rig.ctx, dec) if which == "batch" else call.single(rig.lib, rig.ctx, dec, 0)
    return rc, rig.kernels(mark)


def _pitch_arguments():
    """(route name, plane name) for every stride argument: bt709hip_decode[_batch] (Y, CbCr -- interleaved and planar --, alpha,
    both target formats), _decode_half[_batch], _decode_scaled[_batch], _render_scaled[_batch], _unconvert[_batch], _encode[_batch]
    (a NULL cbcr included) and the two plane shuffles."""
    return [(r.name, p.name) for r in rp.ROUTES for p in r.ins + r.outs]


@pytest.mark.parametrize("name,plane", _pitch_arguments(), ids=["%s-%s" % a for a in _pitch_arguments()])
def test_pitch_validation_at_the_32_bit_edge(fake, fake_rig, name, plane):
    """Each pitch in turn at 2^32 and at 2^32 + the route's own (valid) pitch: BT709HIP_ERR_STRIDE from the batched and from the
    single-frame entry point, nothing launched -- narrowed to 32 bits the second would be the valid pitch, the first 0.  At the
    largest 32-bit pitch the plane's alignment allows (0xfffffff0, 0xffffffff where any pitch goes) the call launches; behind the
    any-ratio and pass-2 entry points such a plane is 2 GiB or more and BT709HIP_ERR_UNSUPPORTED, not a pitch error.
    quads-over / rgba16f-alpha / half-rep-alpha / scaled-over x alpha: the alpha frame's pitch, which the parent commit accepted at
    2^32 + 96 and read at 96."""
    route, rig = rp.ROUTE[name], fake_rig
    p = route.plane(plane)
    assert _run(rig, route, {}, "batch")[0] == 0  # the route as it stands launches
    for which in ("batch", "single"):
        for pitch in (1 << 32, (1 << 32) + p.stride):
            rc, issued = _run(rig, route, {plane: pitch}, which)
            assert rc == _capi.ERR_STRIDE and issued == [], (name, plane, which, hex(pitch), rc, issued)
        top = 0xFFFFFFFF if p.unit == 1 else 0xFFFFFFF0
        rc, issued = _run(rig, route, {plane: top}, which)
        if rp.limited(route):
            assert rc == _capi.ERR_UNSUPPORTED and issued == [], (name, plane, which, rc, issued)
        else:
            calls = 2 if which == "batch" and route in rp.PLANE_ROUTES else 1  # the plane shuffles: one call a frame
            assert rc == 0 and len(issued) == calls, (name, plane, which, rc, issued)


@pytest.mark.parametrize("name,plane", rp.AT_LIMIT, ids=["%s-%s" % a for a in rp.AT_LIMIT])
def test_plane_fits_from_both_sides(fake, fake_rig, name, plane):
    """rows x pitch < 2^31 for every plane of the any-ratio and pass-2 routes: the exact last pitch that fits (a multiple of what
    the plane's pitch must be a multiple of) launches, the next one is BT709HIP_ERR_UNSUPPORTED with nothing launched; and the
    same for the two layouts the GPU file runs (the extreme pitches of the route's residue mod 16)."""
    route, rig = rp.ROUTE[name], fake_rig
    p = route.plane(plane)
    last = (rp.TWO31 - 1) // p.rows // p.unit * p.unit
    assert p.rows * last < rp.TWO31 <= p.rows * (last + p.unit)
    for which in ("batch", "single"):
        rc, issued = _run(rig, route, {plane: last}, which)
        assert rc == 0 and len(issued) == 1, (name, plane, which, rc, issued)
        rc, issued = _run(rig, route, {plane: last + p.unit}, which)
        assert rc == _capi.ERR_UNSUPPORTED and issued == [], (name, plane, which, rc, issued)
    dec = rig.decoder(route)
    for L, want, launches in ((rp.build(route, "under-2-GiB"), 0, 1), (rp.build(route, "at-2-GiB", plane), _capi.ERR_UNSUPPORTED, 0)):
        call = rp.Call(L, IN_BASE, OUT_BASE)
        mark = rig.lib.fake_hip_log_size()
        assert call.batch(rig.lib, rig.ctx, dec) == want and len(rig.kernels(mark)) == launches, (name, plane, L.cls)
        assert call.single(rig.lib, rig.ctx, dec, 1) == want
