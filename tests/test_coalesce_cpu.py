"""CPU tests of the coalescing submit's ORDER rule on the fake HIP runtime (tests/native/fake_hip/, built as tests/test_fake_hip.py
builds it): with BT709HIP_OPT_COALESCE on, calls made in stream order become one launch whose items run concurrently, so a call
that writes what a queued call reads or writes -- or reads what one writes -- must not join that queue.  The launch log is the
witness: (frames, first target) per launch, in order.  No GPU, no sanitizer (tests/native/shim_stress.cpp's `overlap` leg runs
under both, from test_fake_hip.py)."""
import ctypes as C
import random

import pytest

import coalesce_cases as cc
from metalbt709decoder_amd import _capi
from test_fake_hip import SHIM_SOURCES, FakeOp, build, log

W, H = 64, 8
PITCH = 128 * 4  # the canvases: 128 pixels wide


@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    lib = C.CDLL(build(str(tmp_path_factory.mktemp("coalesce") / "libbt709hip_fake.so"), ["-shared", "-fPIC"], SHIM_SOURCES))
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.fake_hip_log_size.restype = C.c_uint64
    lib.fake_hip_log_get.argtypes = [C.c_uint64, C.POINTER(FakeOp)]
    lib.fake_hip_set_device_count(1)
    return lib


class World:
    """One context, one stream, device memory to carve frames and targets from, and decoders on demand."""

    def __init__(self, lib):
        self.lib = lib
        self.ctx = C.c_void_p()
        assert lib.bt709hip_context_create(0, C.byref(self.ctx)) == 0
        s = C.c_void_p()
        assert lib.bt709hip_stream_create(self.ctx, C.byref(s)) == 0
        self.stream = s.value
        self.decoders, self.mem = [], []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.lib.bt709hip_malloc(self.ctx, nbytes, C.byref(p)) == 0
        self.mem.append(p)
        return p.value

    def decoder(self, state=cc.BY_NAME["apple"], n=8, setup=True):
        d = C.c_void_p()
        assert self.lib.bt709hip_decoder_create(self.ctx, state.gamma, 1 if state.alpha else 0, C.byref(d)) == 0
        self.decoders.append(d)
        for opt, val in cc.options(state) + [(cc.OPT_COALESCE, n)]:
            assert self.lib.bt709hip_decoder_set_option(d, opt, val) == 0
        if setup:
            assert self.lib.bt709hip_decoder_setup(d) == 0
        return d

    def frame(self, base, state=cc.BY_NAME["apple"], y=None, w=W, h=H):
        """An NV12 or I420 frame at `base` (tight pitches; I420: U then V); y: the Y plane somewhere else."""
        planar = state.layout == cc.I420
        return _capi.Frame(y or base, w, base + w * h, w // 2 if planar else w, w, h, 1, cc.TRANSFER[state.gamma])

    def alpha(self, base, w=W, h=H):
        return _capi.Frame(base, w, base, w, w, h, 1, cc.TRANSFER_LINEAR)

    def surface(self, base, pitch=PITCH, fmt=cc.BGRA8, w=W, h=H):
        return _capi.Surface(base, pitch, w, h, fmt, 0)

    def submit(self, dec, frames, surfaces, alphas=None):
        """One call: bt709hip_decode for one item, bt709hip_decode_batch for more."""
        n = len(frames)
        fa, sa = (_capi.Frame * n)(*frames), (_capi.Surface * n)(*surfaces)
        aa = (_capi.Frame * n)(*alphas) if alphas else None
        if n == 1:
            return self.lib.bt709hip_decode(dec, fa, aa, sa, frames[0].width, frames[0].height, self.stream, 0)
        return self.lib.bt709hip_decode_batch(dec, n, fa, aa, sa, self.stream, 0)

    def mark(self):
        return self.lib.fake_hip_log_size()

    def launches(self, mark, dec=None):
        """[(frames, first target)] of the decode kernels issued on the stream since `mark` (the fake logs at issue time); with
        `dec`, after a flush of its queue."""
        if dec is not None:
            assert self.lib.bt709hip_decoder_flush(dec, self.stream) == 0
            assert self.lib.bt709hip_stream_synchronize(self.ctx, self.stream) == 0
        return [(o[2], o[3]) for o in log(self.lib, mark) if o[1] == self.stream and o[0].startswith("kernel:decode")]

    def close(self):
        for d in self.decoders:
            assert self.lib.bt709hip_decoder_destroy(d) == 0
        assert self.lib.bt709hip_stream_destroy(self.ctx, self.stream) == 0
        for p in self.mem:
            assert self.lib.bt709hip_free(self.ctx, p) == 0
        assert self.lib.bt709hip_context_destroy(self.ctx) == 0


@pytest.fixture()
def world(fake):
    w = World(fake)
    yield w
    w.close()


def window(canvas, x, y, px=4, pitch=PITCH):
    return canvas + y * pitch + x * px


# ------------------------------------------------------------------ the sequences of tests/test_coalesce_gpu.py, section d

def test_three_calls_two_into_one_surface_one_four_rows_down(world):
    """The probe that found the hole: on the parent the log held ONE launch of three frames."""
    dec = world.decoder()
    ins, canvas = world.alloc(3 * W * H * 2), world.alloc(PITCH * 32)
    targets = [canvas, canvas, window(canvas, 0, 4)]
    mark = world.mark()
    for i, t in enumerate(targets):
        assert world.submit(dec, [world.frame(ins + i * W * H * 2)], [world.surface(t)]) == 0
    assert world.launches(mark, dec) == [(1, t) for t in targets]


@pytest.mark.parametrize("n", [2, 4])
def test_decodes_into_one_surface_go_out_one_by_one(world, n):
    dec = world.decoder()
    ins, canvas = world.alloc(n * W * H * 2), world.alloc(PITCH * 32)
    mark = world.mark()
    for i in range(n):
        assert world.submit(dec, [world.frame(ins + i * W * H * 2)], [world.surface(canvas)]) == 0
        assert world.launches(mark) == [(1, canvas)] * i  # each call issues its predecessor, alone
    assert world.launches(mark, dec) == [(1, canvas)] * n


def test_clips_layered_over_one_canvas(world):
    """BT709HIP_OVER_DESTINATION reads the target as well: three clips over one canvas are three launches."""
    dec = world.decoder(cc.BY_NAME["over-destination"])
    ins, canvas = world.alloc(3 * W * H * 3), world.alloc(PITCH * 32)
    mark = world.mark()
    for i in range(3):
        base = ins + i * W * H * 3
        assert world.submit(dec, [world.frame(base, cc.BY_NAME["alpha"])], [world.surface(canvas)], [world.alpha(base + W * H * 2)]) == 0
    assert world.launches(mark, dec) == [(1, canvas)] * 3


def test_read_after_write_and_write_after_read(world):
    dec = world.decoder()
    ins, x, z = world.alloc(2 * W * H * 2), world.alloc(PITCH * (H + 1)), world.alloc(PITCH * H)
    # call 1 decodes into X; call 2 reads bytes inside X as its Y plane (X's row 1) and decodes into Z
    mark = world.mark()
    assert world.submit(dec, [world.frame(ins)], [world.surface(x)]) == 0
    assert world.submit(dec, [world.frame(ins + W * H * 2, y=x + PITCH)], [world.surface(z)]) == 0
    assert world.launches(mark, dec) == [(1, x), (1, z)]
    # the mirror: call 1 reads a buffer (X's last row) that call 2 overwrites as its target
    mark = world.mark()
    assert world.submit(dec, [world.frame(ins, y=x + 7 * PITCH)], [world.surface(z)]) == 0
    assert world.submit(dec, [world.frame(ins + W * H * 2)], [world.surface(x)]) == 0
    assert world.launches(mark, dec) == [(1, z), (1, x)]
    # a plane that begins at the byte behind X's last pixel touches nothing of it: the call joins
    mark = world.mark()
    assert world.submit(dec, [world.frame(ins)], [world.surface(x)]) == 0
    assert world.submit(dec, [world.frame(ins + W * H * 2, y=x + 7 * PITCH + 4 * W)], [world.surface(z)]) == 0
    assert world.launches(mark, dec) == [(2, x)]


def test_planar_v_plane_and_alpha_plane_count_as_read(world):
    """I420: the V plane sits (H/2) * cbcr_stride behind U.  A target that only the V plane reaches conflicts; so does one that
    only the alpha plane reaches."""
    state = cc.BY_NAME["i420"]
    dec = world.decoder(state)
    ins, arena, z = world.alloc(4 * W * H * 2), world.alloc(PITCH * 64), world.alloc(PITCH * H)
    x = arena + 4096
    plane = (H // 2) * (W // 2)  # bytes of the U plane, and of the V plane behind it
    for chroma_at, want in ((x - plane, [(1, x), (1, z)]), (x - 2 * plane, [(2, x)])):  # V inside X / U and V both in front of X
        f = world.frame(ins + W * H * 2, state)
        f.cbcr = chroma_at
        mark = world.mark()
        assert world.submit(dec, [world.frame(ins, state)], [world.surface(x)]) == 0
        assert world.submit(dec, [f], [world.surface(z)]) == 0
        assert world.launches(mark, dec) == want
    alpha = cc.BY_NAME["alpha"]
    dec = world.decoder(alpha)
    for a_at, want in ((x + 8, [(1, x), (1, z)]), (ins + 3 * W * H * 2, [(2, x)])):
        mark = world.mark()
        assert world.submit(dec, [world.frame(ins, alpha)], [world.surface(x)], [world.alpha(ins + W * H * 3 // 2)]) == 0
        assert world.submit(dec, [world.frame(ins + W * H * 2, alpha)], [world.surface(z)], [world.alpha(a_at)]) == 0
        assert world.launches(mark, dec) == want


def test_wall_and_separate_allocations_share_one_launch(world):
    """Four 64 x 8 windows of one 128 x 16 canvas: disjoint rectangles, interleaved byte ranges.  One launch; so are four
    allocations of their own."""
    dec = world.decoder()
    ins, canvas = world.alloc(4 * W * H * 2), world.alloc(PITCH * 16)
    wall = [window(canvas, x, y) for y in (0, 8) for x in (0, 64)]
    mark = world.mark()
    for i, t in enumerate(wall):
        assert world.submit(dec, [world.frame(ins + i * W * H * 2)], [world.surface(t)]) == 0
    assert world.launches(mark) == []
    assert world.launches(mark, dec) == [(4, canvas)]
    own = [world.alloc(PITCH * H) for _ in range(4)]
    mark = world.mark()
    for i in (2, 0, 3, 1):
        assert world.submit(dec, [world.frame(ins + i * W * H * 2)], [world.surface(own[i])]) == 0
    assert world.launches(mark, dec) == [(4, own[2])]
    # a fifth window that straddles the wall's tiles meets them: the four go out, then the one
    mark = world.mark()
    for i, t in enumerate(wall + [window(canvas, 32, 4)]):
        assert world.submit(dec, [world.frame(ins + (i % 4) * W * H * 2)], [world.surface(t)]) == 0
    assert world.launches(mark, dec) == [(4, canvas), (1, window(canvas, 32, 4))]


def test_a_half_float_row_is_eight_bytes_a_pixel(world):
    """Two RGBA16F windows 64 pixels apart on a 128-pixel canvas are disjoint; 32 pixels apart they overlap -- where two BGRA8
    windows 256 bytes apart do not."""
    dec = world.decoder()
    ins, canvas = world.alloc(2 * W * H * 2), world.alloc(2 * PITCH * H)
    for fmt, pitch, step, want in ((cc.RGBA16F, 2 * PITCH, 512, 1), (cc.RGBA16F, 2 * PITCH, 256, 2), (cc.BGRA8, 2 * PITCH, 256, 1), (cc.BGRA8, 2 * PITCH, 252, 2)):
        mark = world.mark()
        for i in range(2):
            assert world.submit(dec, [world.frame(ins + i * W * H * 2)], [world.surface(canvas + i * step, pitch, fmt)]) == 0
        assert len(world.launches(mark, dec)) == want, (fmt, step)


def test_a_batch_call_conflicts_through_any_of_its_items(world):
    """A call of three whose LAST target meets the queue's FIRST: the queue goes out, the call queues whole.  Overlap inside one
    call stays the caller's business: it is launched as it was given."""
    dec = world.decoder()
    ins, canvas, own = world.alloc(4 * W * H * 2), world.alloc(PITCH * 16), world.alloc(3 * PITCH * H)
    f = [world.frame(ins + i * W * H * 2) for i in range(4)]
    mark = world.mark()
    assert world.submit(dec, f[:2], [world.surface(canvas), world.surface(window(canvas, 64, 0))]) == 0
    assert world.submit(dec, f[1:], [world.surface(own), world.surface(own + PITCH * H), world.surface(window(canvas, 0, 4))]) == 0
    assert world.launches(mark) == [(2, canvas)]
    assert world.submit(dec, f[:2], [world.surface(own + 2 * PITCH * H), world.surface(own + 2 * PITCH * H)]) == 0
    assert world.launches(mark, dec) == [(2, canvas), (5, own)]


def test_layered_sequence_recorded_into_a_graph(world):
    """Between begin and end of a capture the same rule holds: three kernel nodes, in order, on every replay."""
    lib = world.lib
    dec = world.decoder(cc.BY_NAME["over-destination"])
    ins, canvas = world.alloc(3 * W * H * 3), world.alloc(PITCH * 32)
    targets = [canvas, canvas, window(canvas, 0, 4)]
    g = C.c_void_p()
    mark = world.mark()
    assert lib.bt709hip_graph_begin_capture(world.ctx, world.stream) == 0
    for i, t in enumerate(targets):
        base = ins + i * W * H * 3
        assert world.submit(dec, [world.frame(base, cc.BY_NAME["alpha"])], [world.surface(t)], [world.alpha(base + W * H * 2)]) == 0
    assert lib.bt709hip_graph_end_capture(world.ctx, world.stream, C.byref(g)) == 0
    assert log(lib, mark) == []  # recorded, not run
    for replay in (1, 2):
        assert lib.bt709hip_graph_launch(world.ctx, g, world.stream) == 0
        assert world.launches(mark) == [(1, t) for t in targets] * replay
    assert lib.bt709hip_graph_destroy(world.ctx, g) == 0


# ------------------------------------------------------------------ refusals are the call's own status

@pytest.mark.parametrize("state", cc.ILLEGAL, ids=lambda s: s.name)
def test_illegal_combinations_are_refused_by_the_call_and_leave_the_queue_alone(world, state):
    """A decoder under the state's options with two frames queued into BGRA8 targets -- legal, unless the options alone are the
    illegal pair -- then the refused call.  Its status is its own, it launches nothing, and the two still go out together."""
    dec = world.decoder(state)
    ins, outs = world.alloc(3 * W * H * 3), world.alloc(3 * 2 * PITCH * H)
    frames = [world.frame(ins + i * W * H * 3, state) for i in range(3)]
    alphas = [world.alpha(ins + i * W * H * 3 + W * H * 2) for i in range(3)] if state.alpha else None
    always = state.straight and state.over != cc.OVER_OFF  # refused whatever the target
    mark = world.mark()
    for i in range(2):
        rc = world.submit(dec, [frames[i]], [world.surface(outs + i * 2 * PITCH * H)], alphas and [alphas[i]])
        assert rc == (_capi.ERR_UNSUPPORTED if always else 0)
    rc = world.submit(dec, [frames[2]], [world.surface(outs + 2 * 2 * PITCH * H, 2 * PITCH, state.fmt)], alphas and [alphas[2]])
    assert rc == _capi.ERR_UNSUPPORTED
    assert world.launches(mark) == []  # nothing launched, nothing dropped
    assert world.launches(mark, dec) == ([] if always else [(2, outs)])


# ------------------------------------------------------------------ the rule against its model

def _universe(world):
    """Targets and inputs to draw from: two canvases with the wall's windows, windows that straddle them and one whose rows wrap
    the canvas's right edge; separate buffers of the canvas's pitch; tight buffers of a pitch of their own, two of them four
    rows apart in one allocation; frames of an input slab, and two whose Y plane is bytes of the first canvas."""
    targets = []
    for _ in range(2):
        canvas = world.alloc(PITCH * 40)
        targets += [(window(canvas, x, y), PITCH) for x, y in ((0, 0), (64, 0), (0, 8), (64, 8), (32, 4), (0, 4), (96, 2), (64, 12))]
    first_canvas = targets[0][0]
    targets += [(world.alloc(PITCH * H), PITCH) for _ in range(3)]
    tight = world.alloc(4 * W * 4 * H)
    targets += [(tight, W * 4), (tight + 4 * W * 4, W * 4), (tight + 2 * W * 4 * H, W * 4), (tight + 3 * W * 4 * H, W * 4)]
    ins = world.alloc(8 * W * H * 2)
    inputs = [(ins + i * W * H * 2, None) for i in range(8)] + [(ins, first_canvas), (ins + W * H * 2, first_canvas + 8 * PITCH + 256)]
    return targets, inputs


def test_random_sequences_match_the_model(world):
    """A few hundred seeded sequences of calls of 1..3 items.  The log must equal the model's launch list (coalesce_cases.model,
    the rule as the header states it); every item appears in exactly one launch, in submission order; and -- stated without the
    rule, from the rows' bytes -- no launch holds items of two calls of which one writes what the other reads or writes."""
    n = 8
    dec = world.decoder(n=n)
    targets, inputs = _universe(world)
    spare = world.alloc(PITCH * H)  # a target nothing else touches
    rng = random.Random(20261020)
    met = shared = 0
    for seq in range(300):
        calls, descriptors = [], []
        for _ in range(rng.randint(2, 12)):
            count = rng.randint(1, 3)
            pitch = rng.choice([PITCH] * 5 + [W * 4])
            pool = [t for t in targets if t[1] == pitch]
            items, frames, surfaces = [], [], []
            while len(items) < count:
                out, (base, y) = rng.choice(pool)[0], rng.choice(inputs)
                item = cc.Item(out, pitch, H, W * 4, [(y or base, W, H, W), (base + W * H, W, H // 2, W)])
                if any(cc.really_conflict(item, other) for other in items) or cc.really_conflict(item, item._replace(out=spare)):
                    continue  # overlap inside one call, or a frame decoded onto itself, is the caller's error: the sequences make neither
                items.append(item)
                frames.append(world.frame(base, y=y))
                surfaces.append(world.surface(out, pitch))
            calls.append(items)
            descriptors.append((frames, surfaces))
        mark = world.mark()
        for frames, surfaces in descriptors:
            assert world.submit(dec, frames, surfaces) == 0
        got = world.launches(mark, dec)
        want = cc.model(calls, n)
        assert got == [(len(l), l[0].out) for l in want], "sequence %d" % seq
        assert sum(g[0] for g in got) == sum(len(c) for c in calls)
        owner = [k for k, c in enumerate(calls) for _ in c]
        flat = [i for c in calls for i in c]
        at = 0
        for size, first in got:
            assert first == flat[at].out, "sequence %d: submission order" % seq
            group = range(at, at + size)
            for a in group:
                for b in group:
                    if owner[a] < owner[b]:
                        assert not cc.really_conflict(flat[a], flat[b]), "sequence %d: calls %d and %d share a launch" % (seq, owner[a], owner[b])
            shared += size > 1
            at += size
        met += sum(any(cc.really_conflict(a, b) for a in calls[k] for b in calls[k + 1]) for k in range(len(calls) - 1))
    assert shared > 100 and met > 100, (shared, met)  # the sequences do gather, and do meet conflicts


def test_model_agrees_with_the_bytes_where_it_claims_to_be_exact():
    """The rectangle test is exact where the later target's rows lie on the earlier one's grid; the byte-range fallback may only
    err towards a conflict."""
    base = 1 << 20
    for dy in range(0, 12):
        for dx in range(0, PITCH, 4):
            i = cc.Item(base, PITCH, H, W * 4, [])
            j = cc.Item(base + dy * PITCH + dx, PITCH, H, W * 4, [])
            real, rule = cc.really_conflict(i, j), cc.rule_conflict(i, j)
            assert rule == real if dx + W * 4 <= PITCH else (rule or not real), (dy, dx)
