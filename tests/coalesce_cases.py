"""The decoder states the 1:1 decode accepts, for the coalescing submit's tests (BT709HIP_OPT_COALESCE, tests/test_coalesce_gpu.py
and tests/test_coalesce_cpu.py): per state the kernel it must launch and what it must write, in numpy.  The expectation is built
from oracle_lib.Oracle, over_cases.composite_over / tables and straight_alpha_cases.unpremultiply alone -- never from a second
run of the product.  Also the rule that keeps calls of one stream in order (two calls conflict when one writes a byte the other
reads or writes), stated twice: as the shim applies it (`Model`) and as plain byte arithmetic (`rows_of`, `rows_meet`).

Numpy only; constants are stated here, not taken from the bindings."""
from collections import namedtuple

import numpy as np

import over_cases as oc
import straight_alpha_cases as sa
from oracle_lib import GAMMA_APPLE, GAMMA_ITU709, GAMMA_LINEAR, GAMMA_SRGB

NV12, I420 = 0, 1
BGRA8, RGBA16F = 0, 1
TRANSFER_709, TRANSFER_SRGB, TRANSFER_LINEAR = 1, 2, 3  # bt709hip_transfer_tag
OPT_NONTEMPORAL, OPT_XCD_BANDS, OPT_COALESCE, OPT_COMPOSITE_OVER, OPT_CHROMA_LAYOUT, OPT_UNPREMULTIPLY = 1, 5, 6, 9, 11, 12
OVER_OFF, OVER_DESTINATION = oc.OVER_OFF, oc.OVER_DESTINATION
COLOUR = 0x3C7FB2
QUEUED = b"(queued: coalescing submit)"
TRANSFER = {GAMMA_APPLE: TRANSFER_709, GAMMA_ITU709: TRANSFER_709, GAMMA_SRGB: TRANSFER_SRGB, GAMMA_LINEAR: TRANSFER_LINEAR}

# over: OVER_OFF, OVER_DESTINATION or a colour.  fast / general: the kernel-name stems of the two geometries' kernels.
State = namedtuple("State", "name gamma alpha layout fmt over straight alpha_fill fast general")


def _state(name, gamma=GAMMA_SRGB, alpha=False, layout=NV12, fmt=BGRA8, over=OVER_OFF, straight=False, alpha_fill=0xFF, fast="", general=""):
    return State(name, gamma, alpha, layout, fmt, over, straight, alpha_fill, fast, general)


STATES = [
    _state("apple", GAMMA_APPLE, fast="quads<nt>", general="blocks"),
    _state("srgb", GAMMA_SRGB, fast="quads<nt,quantiser>", general="blocks<quantiser>"),
    _state("linear", GAMMA_LINEAR, fast="quads_log<nt>", general="blocks"),
    _state("itu709", GAMMA_ITU709, fast="quads<nt>", general="blocks"),
    _state("apple-fill0", GAMMA_APPLE, alpha_fill=0, fast="quads<nt>", general="blocks"),
    _state("alpha", alpha=True, fast="quads<alpha>", general="blocks<alpha>"),
    _state("over-colour", alpha=True, over=COLOUR, fast="quads<alpha,over-colour>", general="blocks<alpha,over-colour>"),
    _state("over-destination", alpha=True, over=OVER_DESTINATION, fast="quads<alpha,over>", general="blocks<alpha,over>"),
    _state("straight", alpha=True, straight=True, fast="quads<alpha,straight>", general="blocks<alpha,straight>"),
    _state("i420", GAMMA_APPLE, layout=I420, fast="quads<nt>", general="blocks"),
    _state("i420-alpha", alpha=True, layout=I420, fast="quads<alpha>", general="blocks<alpha>"),
    _state("i420-over-destination", alpha=True, layout=I420, over=OVER_DESTINATION, fast="quads<alpha,over>", general="blocks<alpha,over>"),
    _state("i420-straight", alpha=True, layout=I420, straight=True, fast="quads<alpha,straight>", general="blocks<alpha,straight>"),
    _state("f16", GAMMA_APPLE, fmt=RGBA16F, fast="rgba16f", general="rgba16f"),
    _state("f16-alpha", alpha=True, fmt=RGBA16F, fast="rgba16f<alpha>", general="rgba16f<alpha>"),
]
BY_NAME = {s.name: s for s in STATES}

# what stays refused -- under the option as the status of the call itself, the queue untouched
ILLEGAL = [
    _state("over-into-f16", alpha=True, fmt=RGBA16F, over=OVER_DESTINATION),
    _state("colour-into-f16", alpha=True, fmt=RGBA16F, over=COLOUR),
    _state("straight-over", alpha=True, straight=True, over=COLOUR),
    _state("straight-into-f16", alpha=True, straight=True, fmt=RGBA16F),
    _state("i420-into-f16", GAMMA_APPLE, layout=I420, fmt=RGBA16F),
]


def kernel(state, general):
    """bt709hip_last_kernel_name of the state's launch; general: the geometry or an alignment takes the `_blocks` kernels."""
    prefix = "decode_i420_" if state.layout == I420 else "decode_nv12_"
    return (prefix + (state.general if general else state.fast)).encode()


def pixel_bytes(state):
    return 8 if state.fmt == RGBA16F else 4


def options(state):
    """(option, value) pairs that put a fresh decoder of (state.gamma, state.alpha) into the state; alpha_fill has its own setter."""
    out = []
    if state.layout != NV12:
        out.append((OPT_CHROMA_LAYOUT, state.layout))
    if state.over != OVER_OFF:
        out.append((OPT_COMPOSITE_OVER, state.over))
    if state.straight:
        out.append((OPT_UNPREMULTIPLY, 1))
    return out


def random_planes(w, h, seed, n=1, alpha=True):
    """[(y, u, v, a)]: planar frames of random bytes (a is None for an opaque decoder)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        u = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
        v = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
        out.append((y, u, v, rng.integers(0, 256, (h, w), dtype=np.uint8) if alpha else None))
    return out


def interleave(u, v):
    uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return uv


def random_words(w, h, seed, px=4):
    """What a target holds before the decode: random bytes, alpha bytes included."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, px), dtype=np.uint8)


def expected(oracle, tabs, state, planes, before=None):
    """-> (H, W, pixel_bytes) uint8: what the state's decode of `planes` = (y, u, v, a) leaves in a target that held `before`
    (H, W, 4; read by OVER_DESTINATION alone)."""
    y, u, v, a = planes
    h, w = y.shape
    y, uv = np.ascontiguousarray(y), interleave(u, v)
    a = np.ascontiguousarray(a) if state.alpha else None
    if state.fmt == RGBA16F:
        return np.ascontiguousarray(oracle.decode_nv12_rgba16f(state.gamma, y, uv, alpha=a)).view(np.uint8).reshape(h, w, 8)
    word = oracle.decode_nv12(state.gamma, y, uv, alpha=a, alpha_fill=state.alpha_fill).reshape(h, w, 4)
    if state.over == OVER_DESTINATION:
        return oc.composite_over(word, before, *tabs)
    if state.over != OVER_OFF:
        return oc.composite_over(word, state.over, *tabs)
    return sa.unpremultiply(word) if state.straight else word


# ------------------------------------------------------------------ the order rule

Item = namedtuple("Item", "out stride rows row reads")  # a target (base, pitch, rows, bytes per row) and the planes read: [(base, pitch, rows, bytes per row)]


def rows_of(base, stride, rows, row):
    """The bytes of a plane, exactly: one [lo, hi) per row."""
    return [(base + r * stride, base + r * stride + row) for r in range(rows)]


def rows_meet(a, b):
    return any(p < y and x < q for p, q in a for x, y in b)


def really_conflict(i, j):
    """Does one item write a byte the other reads or writes?  Exact, from the rows."""
    wi, wj = rows_of(i.out, i.stride, i.rows, i.row), rows_of(j.out, j.stride, j.rows, j.row)
    return (rows_meet(wi, wj) or any(rows_meet(wi, rows_of(*p)) for p in j.reads) or any(rows_meet(wj, rows_of(*p)) for p in i.reads))


def _span(base, stride, rows, row):
    return base, base + (rows - 1) * stride + row


def _meet(a, b):
    return a[0] < b[1] and b[0] < a[1]


def rule_conflict(i, j):
    """The rule as include/bt709hip_ext.h states it for two items of one geometry and pitch: targets as rectangles where the later
    one's rows lie on the earlier one's pitch grid, else as byte ranges; inputs against targets as byte ranges."""
    lo, hi = min(i.out, j.out), max(i.out, j.out)
    dy, dx = divmod(hi - lo, i.stride)
    if (dy < i.rows and dx < i.row) if dx + i.row <= i.stride else hi - lo < (i.rows - 1) * i.stride + i.row:
        return True
    wi, wj = _span(i.out, i.stride, i.rows, i.row), _span(j.out, j.stride, j.rows, j.row)
    return any(_meet(wi, _span(*p)) for p in j.reads) or any(_meet(wj, _span(*p)) for p in i.reads)


def model(calls, n):
    """calls: [[Item]] in submission order (each of fewer than n items, one geometry; the pitch may differ from call to call)
    -> the launches [[Item]] of a stream that ends in a flush."""
    launches, queue = [], []
    for call in calls:
        joins = queue and len(queue) + len(call) <= n and queue[0].stride == call[0].stride and \
            not any(rule_conflict(i, j) for i in call for j in queue)
        if queue and not joins:
            launches.append(queue)
            queue = []
        queue = queue + list(call)
        if len(queue) >= n:
            launches.append(queue)
            queue = []
    return launches + ([queue] if queue else [])
