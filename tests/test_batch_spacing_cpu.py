"""Batch addressing at any frame spacing, the parts that need no GPU (tests/batch_spacing_cases.py; the GPU half is
tests/test_batch_spacing_gpu.py): the layout builder's own guarantees for every (route, class) the GPU file runs, and -- on the
shim built against the fake HIP runtime, whose launchers keep the addressing of the last launch (fake_hip.h
fake_hip_last_addressing) -- which of the two ways to find frame i each batched entry point takes, with which steps."""
import ctypes as C

import pytest

import batch_spacing_cases as bs
from metalbt709decoder_amd import _capi

IN_BASE, OUT_BASE = 1 << 44, 1 << 45  # "device" addresses: a fake launch touches nothing, validation looks at alignment only


class Addressing(C.Structure):  # fake_hip_addressing
    _fields_ = [("uniform", C.c_int32), ("frames", C.c_int32), ("steps", C.c_int64 * 6)]


# ------------------------------------------------------------------ the builder

def test_every_layout_passes_its_self_checks():
    """Layout.check() for every (route, class) of the GPU file: every true and every alias window inside its slab, pairwise
    disjoint, a guard band apart; the steps are what the class says; and beyond check(): the far classes really leave the low
    4 GiB, their windows are all the host touches, and the small classes stay a GiB away from either end of the slab."""
    assert len(set(bs.PAIRS_RUN)) == len(bs.PAIRS_RUN) == 438  # 215 before the nine planar CHW routes, 324 before the ten of the encoder's other families
    for name, cls in bs.PAIRS_RUN:
        route = bs.ROUTE[name]
        L = bs.build(route, cls)
        assert L.n == bs.CLASSES[cls][1]
        for which in ("in", "out"):
            planes, off, windows, alias = L.side(which)
            touched = sum(hi - lo for lo, hi in windows)
            if L.kind in ("far", "far-descending"):
                assert touched < (1 << 20) and max(hi for lo, hi in windows) > bs.FAR
                for p in planes:
                    assert abs(off[p.name][1] - off[p.name][0]) > bs.FAR
                    assert (off[p.name][0] > bs.FAR) == (L.kind == "far-descending")
            else:
                assert not alias and len(windows) == 1 and touched < (8 << 20)
                assert windows[0][0] == bs.NEAR_ORIGIN and windows[0][1] < bs.SLAB_BYTES - bs.NEAR_ORIGIN
        if cls == "table-twin":  # the descending-3 frames with the middle one moved
            D = bs.build(route, "descending-3")
            for p in route.ins + route.outs:
                a, b = (L.in_off if p in route.ins else L.out_off)[p.name], (D.in_off if p in route.ins else D.out_off)[p.name]
                assert (a[0], a[2]) == (b[0], b[2]) and a[1] != b[1]


def test_every_route_runs_every_class_or_says_why_not():
    run = set(bs.PAIRS_RUN)
    for r in bs.ROUTES:
        for cls in bs.CLASSES:
            assert ((r.name, cls) in run) != bool(bs.CLASSES_NOT_RUN.get((r.name, cls))), (r.name, cls)
    # the forms the issue names, each behind the entry point that launches it
    entries = {}
    for r in bs.ROUTES:
        entries.setdefault(r.entry, []).append(r.kernel)
    # the planar CHW routes: the fast kernels split under the band map (two launches, the first banded: the GPU file asserts it)
    chw = [r for r in bs.ROUTES if r.chw]
    assert [r.name for r in chw] == [r.name for r in bs.ROUTES[19:28]] and all(p.stacked == r.chw_planes for r in chw for p in r.ins + r.outs if p.name in ("out", "chw"))
    assert sorted(r.name for r in chw if r.bands) == ["chw-quads-f16-alpha", "chw-quads-f32-i420", "chw-quads-u8", "encode-chw-f16", "encode-chw-u8-i420"]
    assert all((r.name, "bands-tail-descending") in run for r in chw if r.bands)
    assert all((r.name, c) in run for r in chw for c in ("far", "far-descending", "fan-out", "plane-skew", "descending-33", "table-twin"))
    assert {k: len(v) for k, v in entries.items()} == {"decode": 9, "half": 3, "scaled": 6, "render": 2, "unconvert": 2, "encode": 16}
    # the encoder's other families, appended behind them: five families, a fast and a general kernel of each but the last
    new = bs.ROUTES[28:]
    assert [r.name for r in new] == ["encode-i420", "encode-i420-blocks-premul", "convert-packed", "convert-packed-blocks", "convert-point-i420",
                                     "encode-pair", "encode-pair-i420-blocks", "encode-half", "encode-half-i420-blocks", "encode-half-pair"]
    assert all(r.entry == "encode" and r.size == r.out_size == (64, 16) and r.ctx_options and set(dict(r.ctx_options)) <= set(bs.CTX_DEFAULTS) for r in new)
    assert sorted(r.name for r in new if r.bands) == ["convert-packed", "convert-point-i420", "encode-half", "encode-half-pair", "encode-i420", "encode-pair"]
    assert all((r.name, c) in run for r in new for c in ("far", "far-descending", "fan-out", "crossed-up-down", "descending-33", "table-twin"))
    assert all(((r.name, "plane-skew") in run) == (not r.name.startswith("convert-packed")) for r in new)
    assert all((r.name, "bands-tail-descending") in run for r in new if r.bands)
    assert [r.name for r in new if r.paired] == ["encode-pair", "encode-pair-i420-blocks", "encode-half-pair"] and all((r.table == 16) == r.paired for r in new)
    # the skewed classes run on the five fast routes that have a byte-addressed plane; what they must report follows from the
    # header's alignment rules: dword stores to Y (and alpha Y) demote the BGRA8 forms under either skew, the RGBA16Float forms
    # store halves -- a step = 2 (mod 4) keeps the fast kernel, an odd one demotes
    skewed = {r.name: {k: v[0] for k, v in r.skew.items()} for r in new if r.skew}
    assert skewed == {"encode-i420": {2: b"encode_bgra_i420_blocks", 1: b"encode_bgra_i420_blocks"},
                      "convert-point-i420": {2: b"convert_bgra_i420_blocks", 1: b"convert_bgra_i420_blocks"},
                      "encode-pair": {2: b"encode_bgra_alpha_nv12_blocks", 1: b"encode_bgra_alpha_nv12_blocks"},
                      "encode-half": {2: b"encode_rgba16f_nv12", 1: b"encode_rgba16f_nv12_blocks"},
                      "encode-half-pair": {2: b"encode_rgba16f_alpha_nv12", 1: b"encode_rgba16f_alpha_nv12_blocks"}}
    assert all((name, c) in run for name in skewed for c in bs.SKEW)
    assert all("no byte-addressed plane" in bs.CLASSES_NOT_RUN[(name, c)] for name in ("convert-packed", "convert-packed-blocks") for c in bs.SKEW)
    assert len(run) - 324 == 114


def test_forms_without_a_route_say_whose_body_they_share():
    """FORMS_NOT_ROUTED: no listed name is one a route (or a route's skew class) leaves on record, and every reason names one
    that is."""
    assert bs.FORMS_NOT_ROUTED and {r.kernel.decode() for r in bs.ROUTES} <= bs.REPORTED
    for name, reason in bs.FORMS_NOT_ROUTED.items():
        assert name not in bs.REPORTED and reason, name
        assert any(reason.endswith("body %s addresses through" % routed) for routed in bs.REPORTED), (name, reason)
    for name in ("decode_nv12_quads<alpha,straight>", "decode_nv12_blocks<alpha,over-colour>", "decode_nv12_rgba16f", "decode_nv12_scaled_f16<alpha>",
                 "decode_nv12_scaled_f16<alpha,over>", "encode_alpha_y<i420>", "encode_bgra_nv12<premul>", "encode_bgra_alpha_i420", "convert_bgra_nv12",
                 "convert_bgra_packed444<premul>", "encode_rgba16f_i420", "encode_rgba16f_alpha_i420_blocks"):
        assert name in bs.FORMS_NOT_ROUTED, name


# ------------------------------------------------------------------ the shim on the fake HIP runtime

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    from test_fake_hip import SHIM_SOURCES, FakeOp, build
    so = build(str(tmp_path_factory.mktemp("fake_spacing") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES)
    lib = C.CDLL(so)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_last_addressing.argtypes = [C.POINTER(Addressing)]
    lib.fake_hip_set_device_count(1)
    return lib


class FakeRig:
    """A context and, per route, the decoder the route asks for."""

    def __init__(self, lib):
        self.lib, self.ctx, self.decs = lib, C.c_void_p(), {}
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0

    def decoder(self, route):
        if route.entry in ("render", "encode"):
            return None
        if route.name not in self.decs:
            d = C.c_void_p()
            assert self.lib.bt709hip_decoder_create(self.ctx, route.gamma, 1 if route.alpha else 0, C.byref(d)) == 0
            for opt, val in route.options + (((_capi.OPT_COMPOSITE_OVER, route.over),) if route.over is not None else ()):
                assert self.lib.bt709hip_decoder_set_option(d, opt, val) == 0
            assert self.lib.bt709hip_decoder_setup(d) == 0
            self.decs[route.name] = d
        return self.decs[route.name]

    def kernels(self, mark):
        from test_fake_hip import log
        return [o for o in log(self.lib, mark) if o[0].startswith("kernel:")]

    def addressing(self):
        a = Addressing()
        assert self.lib.fake_hip_last_addressing(C.byref(a)) == 0
        return a.uniform, a.frames, list(a.steps)

    def close(self):
        for d in self.decs.values():
            assert self.lib.bt709hip_decoder_destroy(d) == 0
        assert self.lib.bt709hip_context_destroy(self.ctx) == 0


@pytest.fixture
def fake_rig(fake):
    r = FakeRig(fake)
    yield r
    r.close()


def _bump(call, route, i, nbytes):
    """Move frame i's first input plane: the batch is no longer evenly spaced."""
    if route.entry in ("decode", "half", "scaled"):
        call.frames[i].y += nbytes
    elif route.entry == "unconvert":
        call.ptrs[i] += nbytes
    else:
        call.ins[i].bgra += nbytes


@pytest.mark.parametrize("entry", ["decode", "half", "scaled", "render", "unconvert", "encode"])
def test_entry_point_takes_the_uniform_path_with_the_builders_steps(fake, fake_rig, entry):
    """bt709hip_{decode, decode_half, decode_scaled, render_scaled, unconvert, encode}_batch over every route and class of the
    GPU file: one launch of all the frames; counts 2 and 3 (and 33, and 70) evenly spaced launch WITHOUT the table, with the steps
    the builder computed -- negative, zero, 2^32 + d, another for every plane; table-twin launches with the table (the one entry
    point without a table refuses it); 33 frames of which one is moved are BT709HIP_ERR_UNSUPPORTED, nothing launched.  A PAIRED
    encode (colour + alpha frames, from BGRA8 or RGBA16Float) has five steps: the alpha frames' two must arrive in the spare slots
    pair_frame and advance_frames read them from -- the fake launcher reports those slots -- and its table holds 16 pairs."""
    lib, rig = fake, fake_rig
    routes = [r for r in bs.ROUTES if r.entry == entry]
    assert routes
    for route in routes:
        dec = rig.decoder(route)
        for cls in route.classes():
            L = bs.build(route, cls)
            call = bs.Call(route, L, IN_BASE, OUT_BASE)
            mark = lib.fake_hip_log_size()
            rc = call.batch(lib, rig.ctx, dec)
            if entry == "render" and not L.uniform:
                assert rc == _capi.ERR_UNSUPPORTED and rig.kernels(mark) == [], (route.name, cls)
                continue
            assert rc == 0, (route.name, cls, rc)
            issued = rig.kernels(mark)
            assert len(issued) == 1 and issued[0][2] == L.n, (route.name, cls, issued)
            assert issued[0][3] == OUT_BASE + L.out_off[route.outs[0].name][0]
            uniform, frames, steps = rig.addressing()
            assert frames == L.n
            if L.uniform:
                assert uniform == 1 and steps == call.expected_steps(L), (route.name, cls, steps, call.expected_steps(L))
            else:
                assert uniform == 0 and steps == [0] * 6, (route.name, cls, uniform, steps)
            if L.uniform and route.paired:  # all five steps of a paired batch, each its own plane's (plane-skew: five different ones)
                s = L.steps
                assert steps[:5] == [s[route.ins[0].name], s["y"], s["cbcr"], s["alpha_y"], s.get("alpha_cbcr", 0)], (route.name, cls, steps)
        # past the table: evenly spaced is accepted (above), anything else refused before a launch
        L = bs.build(route, "descending-33")
        call = bs.Call(route, L, IN_BASE, OUT_BASE)
        assert route.table in (16, 31, 32)  # 31: a planar CHW encode, whose table gives one entry to the scale and bias; 16: PAIRS
        _bump(call, route, min(17, route.table - 1), 16)  # a frame the table's own count still holds
        mark = lib.fake_hip_log_size()
        assert call.batch(lib, rig.ctx, dec) == _capi.ERR_UNSUPPORTED, route.name
        if route.table < 32:
            assert call.batch(lib, rig.ctx, dec, count=32) == _capi.ERR_UNSUPPORTED and rig.kernels(mark) == [], route.name
            assert call.batch(lib, rig.ctx, dec, count=route.table + 1) == _capi.ERR_UNSUPPORTED and rig.kernels(mark) == [], route.name
        assert call.batch(lib, rig.ctx, dec, count=route.table) == (_capi.ERR_UNSUPPORTED if entry == "render" else 0), route.name
        assert len(rig.kernels(mark)) == (0 if entry == "render" else 1)
        if entry != "render":
            assert rig.addressing()[:2] == (0, route.table)


@pytest.mark.parametrize("count", [2, 3])
@pytest.mark.parametrize("side", ["in", "out"])
@pytest.mark.parametrize("name,texel", [("render-bgra8", 4), ("render-rgba16f", 8)])
def test_render_scaled_batch_checks_every_surfaces_alignment(fake, fake_rig, name, texel, side, count):
    """A surface i >= 1 whose base is no multiple of its texel size -- 4 bytes for BGRA8, 8 for RGBA16F intermediates -- is
    refused with BT709HIP_ERR_STRIDE as bt709hip_render_scaled refuses it, on either side, before anything is launched.  The
    surfaces stay evenly spaced: it is the STEP that is off the texel size (by half a texel: surface 2 is aligned again; by
    one byte: no surface but the first is)."""
    lib, rig, route = fake, fake_rig, bs.ROUTE[name]
    L = bs.build(route, "descending-3")
    size = texel if side == "in" else 4
    for skew in (size // 2, 1):
        call = bs.Call(route, L, IN_BASE, OUT_BASE)
        surfs = call.ins if side == "in" else call.surfs
        for i in range(3):
            surfs[i].bgra += i * skew
        mark = lib.fake_hip_log_size()
        assert call.batch(lib, rig.ctx, None, count=count) == _capi.ERR_STRIDE, (skew, count)
        for i in range(1, count):  # what the single call says of the same surface
            want = _capi.ERR_STRIDE if (i * skew) % size else 0
            assert call.single(lib, rig.ctx, None, i) == want, (skew, i)
        assert [k for k in rig.kernels(mark) if k[2] != 1] == []  # nothing but the aligned surfaces' single calls
    call = bs.Call(route, L, IN_BASE, OUT_BASE)
    for i in range(3):
        (call.ins if side == "in" else call.surfs)[i].bgra += i * 2 * size  # a step that keeps every surface aligned
    mark = lib.fake_hip_log_size()
    assert call.batch(lib, rig.ctx, None, count=count) == 0
    issued = rig.kernels(mark)
    assert len(issued) == 1 and issued[0][2] == count
