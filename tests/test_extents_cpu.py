"""Extents, the parts that need no GPU (tests/extent_cases.py; the GPU half is tests/test_extents_gpu.py): the layout builder's
own guarantees for every (route, class), the argument for a period of 251 items, that a resized route still selects its
kernel, that every kernel name the project can report meets every extent, and -- on the shim built against the fake HIP runtime,
whose launch log shows what was launched -- every limit from both sides."""
import numpy as np
import pytest

import batch_spacing_cases as bs
import extent_cases as ec
import row_pitch_cases as rp
from metalbt709decoder_amd import _capi
from test_batch_spacing_cpu import IN_BASE, OUT_BASE, FakeRig, fake  # noqa: F401  (`fake` is the module's fixture)


# ------------------------------------------------------------------ the builder

def test_every_layout_passes_its_self_checks():
    """Layout.check() for every (route, class), refused ones included: one window a side inside the slab, every plane's items in
    a run of their own, a guard band from the next and from either end; and beyond check(): the extent is the one the class
    names, the slabs are tens of MB, two items of a plane are ITEM_GAP or more apart."""
    assert len(set(ec.PAIRS_ALL)) == len(ec.PAIRS_ALL) == len(ec.PAIRS_RUN) + len(ec.PAIRS_REFUSED)
    # the largest case: scaled-chw-f32-alpha's wide target, 4 planes x 4 rows of 2^20 + 12 floats = 64 MiB + 768 bytes
    assert (1 << 20) <= ec.SLAB_BYTES == (67 << 20)
    for name, cls in ec.PAIRS_ALL:
        L = ec.build(name, cls)
        base, r = L.base, L.route
        (w, h), (ow, oh) = r.size, r.out_size
        assert L.n == {"longest": 65535, "longest-unbanded": 65535, "too-many": 65536}.get(cls, 1)
        for p in r.ins + r.outs:  # a planar CHW surface: 3 or 4 planes of the frame's (the view's) size each, a target's fourth given room
            assert (p.stacked > 1) == (bool(base.chw) and p.name in ("out", "chw"))
            if p.stacked > 1:
                pw, ph = (w, h) if p in r.ins else (ow, oh)
                assert p.stacked == base.chw_planes and (p.row_bytes, p.rows) == (base.elem * pw, p.stacked * ph)
                assert p.room == ((4 - p.stacked) * ph * p.stride if p in r.outs else 0)
        for which in ("in", "out"):
            planes, off, windows, _ = L.side(which)
            for p in planes:
                o = off[p.name]
                assert L.n == 1 or (o[1] - o[0] == L.steps[p.name] >= p.extent + ec.ITEM_GAP and o[L.n - 1] == o[0] + (L.n - 1) * L.steps[p.name])
        if base.entry == "encode":  # texels of 4 bytes, 8 of an RGBA16Float surface; elements of a CHW tensor
            texel = base.elem if base.chw else 8 if base.in_fmt == bs.F16 else 4
            assert r.ins[0].row_bytes == texel * w and r.ins[0].unit == texel, (name, cls)
            assert [p.name for p in r.outs] == [p.name for p in base.outs] and ("alpha_y" in [p.name for p in r.outs]) == base.paired
        if cls in ("longest", "longest-unbanded", "too-many"):
            assert w <= 16 and h <= 4 and ow <= 16 and oh <= 4
        elif cls in ("tallest", "tallest-from-tall", "too-tall"):
            past = cls == "too-tall"
            if ec.rescales(base):
                assert oh == 65535 + past and h == (131072 if cls == "tallest-from-tall" else 4)
            elif ec.shuffles(base):
                assert h == 65535 + past
            elif base.entry == "half":
                assert h == 131068 + 4 * past and h % 4 == 0 and oh == h // 2
            elif base.entry == "unconvert":
                assert h == 65534 + 2 * past
            else:
                assert h == 131070 + 2 * past and h // 2 == 65535 + past
            assert w <= 16
        elif cls == "wide":
            widest = ow if ec.rescales(base) else w
            assert (1 << 20) < widest <= (1 << 20) + 16 and widest % 256 != 0 and max(h, oh) <= 4
            if not ec.shuffles(base) and not ec.general(base):
                assert (widest // 4) % 64 != 0  # the last wave of quads is ragged
            if base.name.endswith("-wide") and ec.shuffles(base):
                assert w % 8 == 0 and (w // 8) % 256 != 0  # the last 256-lane group of 8-sample lanes
        else:
            assert cls == "wide-down" and w == ec.WIDE and ow == 1000


def test_every_route_runs_every_class_or_says_why_not():
    run = set(ec.PAIRS_ALL)
    assert [r.name for r in ec.ROUTES] == [r.name for r in bs.ROUTES] + [r.name for r in rp.PLANE_ROUTES]
    for r in ec.ROUTES:
        for cls in ec.CLASSES:
            assert ((r.name, cls) in run) != bool(ec.CLASSES_NOT_RUN.get((r.name, cls))), (r.name, cls)
    # the plane shuffles have no batched form; the rescale entry points alone have a target of another size; the map splits
    # only the routes that say so
    for (name, cls), reason in ec.CLASSES_NOT_RUN.items():
        r = ec.ROUTE[name]
        assert reason and ((cls in ("longest", "longest-unbanded", "too-many") and ec.shuffles(r)) or (cls == "longest-unbanded" and not r.bands)
                           or (cls in ("tallest-from-tall", "wide-down") and not ec.rescales(r))), (name, cls)
    assert len(ec.PAIRS_RUN) == 42 + 8 + 38 + 17 + 42 + 8 and len(ec.PAIRS_REFUSED) == 42 + 38  # ten routes, six of them banded, more than 32 / 28 / 11


def test_every_kernel_name_meets_every_extent():
    """Every kernel name a route can leave on record appears in a tallest, a wide and -- where a batched form exists -- a longest
    case, and the resized route still asks for it."""
    names = {r.kernel for r in ec.ROUTES}
    assert len(names) == 39  # of 42 routes: decode_nv12_scaled in two tap forms, the plane-shuffle kernels in a wide and a byte branch
    assert not names & {n.encode() for n in bs.FORMS_NOT_ROUTED}  # the names without a route: instantiations of these bodies
    for cls in ("tallest", "longest", "wide"):
        met = {ec.resized(ec.ROUTE[name], c).kernel for name, c in ec.PAIRS_RUN if c == cls}
        batched = {r.kernel for r in ec.ROUTES if not ec.shuffles(r)}
        assert met == (batched if cls == "longest" else names), (cls, names - met)
    for r in ec.ROUTES:
        assert (r.name, "tallest") in ec.PAIRS_RUN and (r.name, "wide") in ec.PAIRS_RUN and (ec.shuffles(r) or (r.name, "longest") in ec.PAIRS_RUN)


# ------------------------------------------------------------------ the period

def test_an_item_index_gone_wrong_lands_on_other_content():
    """Item k holds frame k % 251.  For every k from 251 on, the index a kernel would form by mistake -- cut to 13 or 15 bits,
    modulo the 8191 frames of a band, a band late or early by a multiple of 8 (under 8 x 251), the item before or after -- has
    another residue mod 251 wherever it is another index.  (16 bits hold every index.)  Cut to EIGHT bits it has another
    residue for every k but the 256 from 64256 = 256 x 251 on: the mistake is seen at the other 65024 items."""
    k = np.arange(ec.PERIOD, ec.MOST_ITEMS)
    wrongs = {"13 bits": k & 0x1FFF, "15 bits": k & 0x7FFF, "16 bits": k & 0xFFFF, "mod 8191": k % 8191, "before": k - 1, "after": k + 1}
    wrongs.update({"band %+d" % (8 * j): k + 8 * j for j in range(-250, 251) if j})
    for what, wrong in wrongs.items():
        other = wrong != k
        assert np.all((wrong % ec.PERIOD != k % ec.PERIOD)[other]), what
        assert other.any() or what == "16 bits"
    blind = k[((k & 0xFF) != k) & ((k & 0xFF) % ec.PERIOD == k % ec.PERIOD)]
    assert np.array_equal(blind, np.arange(64256, 64512))
    # the six items the single-frame call repeats: the ends, the last frame of band 0 and the first of band 1, the split
    assert ec.SINGLES == [0, 8191 - 1, 8191, 8 * 8191 - 1, 8 * 8191, ec.MOST_ITEMS - 1] and 8 * 8191 == ec.MOST_ITEMS - ec.MOST_ITEMS % 8


@pytest.mark.parametrize("name", ["quads", "half-narrow", "scaled-wide", "scaled-over", "unconvert-pixel", "encode-fast", "convert-packed", "encode-pair-i420-blocks",
                                  "encode-half-pair"])
def test_two_residues_give_distinct_expected_bytes(oracle, name):
    import json
    import os
    import over_cases as oc
    T = np.array(json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alpha_luma.json")))["luma"], np.uint8)
    L = ec.build(name, "longest")
    try:
        want = ec.expected(L, oracle, oc.tables(oracle), T)
    finally:
        ec.forget(L)
    flat = np.concatenate([want[p.name].reshape(ec.PERIOD, -1) for p in L.route.outs], axis=1)
    assert len({row.tobytes() for row in flat}) == ec.PERIOD


# ------------------------------------------------------------------ the resized routes

def test_resized_routes_keep_what_selects_their_kernel():
    """_shape() gives every route's own planes back at its own sizes; a resized plane keeps its pitch's residue mod 16, its unit
    and -- the fast forms -- a width the form takes; the mirror of the any-ratio launcher's tap choice agrees with the records
    the routes' own tests pin, and the resized rescale routes land on a form by the wave or a persistent one as the class says."""
    for r in ec.ROUTES:
        (w, h), (ow, oh) = r.size, r.out_size
        for which, planes in (("in", r.ins), ("out", r.outs)):
            for p in planes:
                assert ec._shape(r, p, which, w, h, ow, oh) == (p.row_bytes, p.rows), (r.name, p.name)
        if r.taps is not None:
            assert ec.scaled_plan(r) == r.taps, r.name
    for name, cls in ec.PAIRS_ALL:
        base, r = ec.ROUTE[name], ec.resized(ec.ROUTE[name], cls)
        assert r.name == base.name and r.key != base.key and r.kernel == base.kernel
        for old, new in zip(base.ins + base.outs, r.ins + r.outs):
            assert new.stride % 16 == old.stride % 16 and new.unit == old.unit and new.stride % new.unit == 0
        w = r.size[0]
        assert w % 2 == 0 and (ec.general(base) or ec.rescales(base) or w % 4 == 0) and (base.entry != "half" or w % 4 == 0)
        if ec.general(base):
            # a byte plane off a 4-byte pitch, a plane of texels or words (its pitch is a multiple of 4 by contract) off a 16-byte one
            assert any(p.stride % (4 if p.unit == 1 else 16) for p in r.ins + r.outs) or w % 4 or name.endswith("-bytes")
        if name.endswith("-wide") and ec.shuffles(base):
            assert w % 8 == 0
        if base.taps is not None:
            sy = r.size[1] / r.out_size[1]
            assert r.taps[1] == (1 if sy >= 1 or name == "scaled-f16" else 0), (name, cls, r.taps)
            assert r.taps[0] == {"scaled-once": ec.ONCE, "scaled-chw-f32-alpha": ec.ONCE}.get(name, ec.SHARED) if sy < 1 else r.taps[0] == ec.WIDE_TAPS, (name, cls, r.taps)


class _Memory:
    """A rig whose device is a numpy array: upload / download at offsets from `base`."""

    def __init__(self, size, base=1 << 40):
        self.base, self.mem = base, np.zeros(size, np.uint8)

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr).reshape(-1)
        self.mem[dptr - self.base:dptr - self.base + arr.size] = arr

    def download(self, dptr, nbytes):
        return self.mem[dptr - self.base:dptr - self.base + nbytes].copy()


@pytest.mark.parametrize("name,cls", [("quads-over", "wide"), ("encode-blocks", "wide"), ("i420", "wide"), ("scaled-over", "wide-down")])
def test_whole_array_helpers_are_the_per_row_helpers(name, cls):
    """upload_inputs / reset_outputs / collect of this module against batch_spacing_cases' own (a Python loop over the rows) on
    one-item layouts: the same window images, the same pixels collected, the same stray byte caught."""
    L = ec.build(name, cls)
    try:
        mine, theirs = _Memory(max(L.total.values())), _Memory(max(L.total.values()))
        for fill in (0x00, 0xFF):
            ec.upload_inputs(mine, mine.base, L, fill)
            bs.upload_inputs(theirs, theirs.base, L, fill)
            assert np.array_equal(mine.mem, theirs.mem)
        before = ec.reset_outputs(mine, mine.base, L)
        before_theirs = bs.reset_outputs(theirs, theirs.base, L)
        assert len(before_theirs) == 1 and np.array_equal(before, before_theirs[0]) and np.array_equal(mine.mem, theirs.mem)
        rng = np.random.default_rng(5)
        for p in L.route.outs:  # "the kernel": random bytes in every pixel
            ec._items(mine.mem, L, "out", p)[...] = rng.integers(0, 256, (1, p.rows, p.row_bytes), dtype=np.uint8)
        theirs.mem[:] = mine.mem
        got, got_theirs = ec.collect(mine, mine.base, L, before, "mine"), bs.collect(theirs, theirs.base, L, before_theirs, "theirs")
        for p in L.route.outs:
            assert np.array_equal(got[p.name][0], got_theirs[(p.name, 0)])
        p = L.route.outs[-1]
        stray = L.out_off[p.name][0] + p.extent  # the first byte behind the last row
        mine.mem[stray] ^= 0xFF
        with pytest.raises(AssertionError, match="outside the pixels, first at slab offset %d" % stray):
            ec.collect(mine, mine.base, L, before, "mine")
    finally:
        ec.forget(L)


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture
def fake_rig(fake):  # noqa: F811
    r = FakeRig(fake)
    yield r
    r.close()


def _decoder(rig, route):
    return None if ec.shuffles(route) else rig.decoder(route)


@pytest.mark.parametrize("name", [r.name for r in ec.ROUTES])
def test_every_limit_from_both_sides(fake, fake_rig, name):  # noqa: F811
    """The tallest frame, the longest batch and the widest frame launch; one past a limit the batched call returns the code on
    record in extent_cases.refusal (BT709HIP_ERR_UNSUPPORTED; bt709hip_render_scaled_batch over 65535 surfaces:
    BT709HIP_ERR_INVALID_ARG), the single-frame call BT709HIP_ERR_UNSUPPORTED, and the fake runtime's log shows no launch."""
    rig, base = fake_rig, ec.ROUTE[name]
    for cls in ec.classes(base):
        L = ec.build(name, cls)
        if cls == "longest-unbanded" and base.entry == "encode":
            continue  # the context's option: the decoder's is the resized route's own
        dec = None
        if not ec.shuffles(base) and base.entry not in ("render", "encode"):
            if name in rig.decs:  # FakeRig keeps one decoder a route name: this class's options
                assert rig.lib.bt709hip_decoder_destroy(rig.decs.pop(name)) == 0
            dec = rig.decoder(L.route)
        call = rp.Call(L, IN_BASE, OUT_BASE)
        mark = rig.lib.fake_hip_log_size()
        rc = call.batch(rig.lib, rig.ctx, dec)
        issued = rig.kernels(mark)
        if cls in ec.REFUSED:
            assert rc == ec.refusal(base, cls) and issued == [], (name, cls, rc, issued)
            if cls == "too-tall":
                assert call.single(rig.lib, rig.ctx, dec, 0) == _capi.ERR_UNSUPPORTED and rig.kernels(mark) == [], (name, cls)
            else:  # one item fewer is the longest batch
                assert call.batch(rig.lib, rig.ctx, dec, count=ec.MOST_ITEMS) == 0 and len(rig.kernels(mark)) >= 1, (name, cls)
        else:
            assert rc == 0 and len(issued) >= 1 and sum(k[2] for k in issued) == L.n, (name, cls, rc, issued)
            for i in (ec.SINGLES if L.n > 1 else [0]):
                if not ec.shuffles(base):
                    assert call.single(rig.lib, rig.ctx, dec, i) == 0, (name, cls, i)
