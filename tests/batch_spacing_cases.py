"""Where the frames of a batched call lie (tests/test_batch_spacing_cpu.py, tests/test_batch_spacing_gpu.py; numpy and ctypes only).

Every batched entry point finds frame i of a launch either in a pointer table (32 entries; 31 for an encode of planar CHW
tensors) or, when the caller's pointers are evenly spaced, as frame 0 + i * step with one signed 64-bit step per plane -- and
ANY two frames are evenly spaced.  The rest
of the suite carves its frames in ascending order at one positive pitch from one slab.  build(route, cls) lays the planes of a
ROUTE (an entry point and a kernel form: its planes, sizes, decoder options and the kernel it must report) out in one input and
one output slab under a SPACING CLASS:

    descending-2 / -3 / -33   every step negative; 33 frames are past the pointer table
    crossed-up-down / -down-up  inputs ascending and outputs descending, and the reverse
    fan-out                   every input step 0 (one frame, one alpha plane), the outputs ascending
    plane-skew                each plane evenly spaced at a step of its own: input plane j steps by j + 1 slots of its size, output
                              plane j by j + 2, every second plane of a side downwards
    far / far-descending      two frames 2^32 + d bytes apart on every plane (d small, a multiple of 16), the high one second / first
    bands-tail-descending     70 frames, all steps negative: 64 under the XCD-band map, 6 behind advance_frames
    skewed-step-2 / -1        frame 0 16-byte aligned, the step of every byte-addressed plane = 2 (mod 4) / odd
    table-twin                the descending-3 frames with the middle one moved: no step reaches every frame, the table is used

The slabs are the two of 4 GiB + 1 MiB the far classes need; the other classes lie 1 GiB inside them (an address that is off by
less than that is still memory of the test's own).  A layout names WINDOWS: the byte ranges the test uploads, downloads and
checks.  Below 2^32 + 1 MiB of slab only the windows are ever touched by the host: the small classes have one window (their
whole span), the far classes one per frame and plane -- the samples with a guard band either side -- and one ALIAS window per
plane where a step cut to its low 32 bits would land: frame 0 + d (far: zero- or sign-extended alike), frame 0 - d
(far-descending, sign-extended; zero-extended it leaves the slab, which is why that class is never run against a variant that
cuts the step).  Layout.check() asserts, on the CPU, that all of them lie inside their slab, apart from one another by at least
a guard band.

A plane is rows at one pitch.  Two kinds of plane STACK several: the "cbcr" plane of an I420 frame (U's rows, then V's) and a
planar CHW surface (planes R, G, B and, from an alpha decoder, A; plane c starts c x H x pitch behind
plane 0) -- one Plane of planes x H rows of W x e bytes, unit e.  An opaque decoder's CHW target is given the ROOM of a fourth
plane behind its three, inside the frame's window: that nothing is written there is part of every comparison.  The CHW routes
close the table: the 1:1 decode into CHW targets (fast and general kernel, u8 / f16 / f32, NV12 and I420 frames), the fused
rescale into CHW views (a per-lane and a by-wave tap form) and the encoder reading CHW tensors (into NV12 and into I420).

The encoder's other families follow them, each with address products of its own (bt709_encode.hip, bt709_encode_pair.h,
bt709_encode_convert.h, bt709_encode_half.h, bt709_encode_half_alpha.h): BGRA into planar I420 (V's rows (H/2) x pitch behind
U's), the per-pixel converter (packed 4-byte words through the "y" pointer and pitch: a plane of unit 4 and no "cbcr"; and its
subsampled frame), the colour + alpha PAIR (two frames a picture: the planes "alpha_y" and "alpha_cbcr" have pitches and steps
of their own, which ride in spare slots of the pointer table -- which therefore holds 16 pairs), RGBA16Float input (8-byte
texels; its fast kernel stores halves, so a step = 2 (mod 4) keeps it) and the RGBA16Float pair.  FORMS_NOT_ROUTED names the
kernel forms that have no route, each with the routed form whose body it instantiates."""
import ctypes as C
import zlib

import numpy as np

import chw_cases as cc
import encode_chw_cases as ecc
import encode_half_alpha_cases as ehac
import encode_half_cases as ehc
import straight_alpha_cases as sac
from metalbt709decoder_amd import _capi
from metalbt709decoder_amd._capi import Frame, Surface

CANARY = 0x5A
GUARD = 256
FAR = 1 << 32
SLAB_BYTES = FAR + (1 << 20)
NEAR_ORIGIN = 1 << 30
MATRIX_709, TRANSFER_709, TRANSFER_SRGB, TRANSFER_LINEAR = 1, 1, 2, 3  # the frame tags (kCVImageBuffer...: metalbt709decoder_amd)
GAMMA_APPLE, GAMMA_SRGB, GAMMA_LINEAR = 0, 1, 2
F16, SRGB8, ALPHA8 = _capi.FORMAT_RGBA16F, _capi.FORMAT_BGRA8_SRGB, _capi.FORMAT_BGRA8_ALPHA

# class -> (kind, frames)
CLASSES = {
    "descending-2": ("descending", 2), "descending-3": ("descending", 3), "descending-33": ("descending", 33),
    "crossed-up-down": ("crossed-up-down", 3), "crossed-down-up": ("crossed-down-up", 3),
    "fan-out": ("fan-out", 3), "plane-skew": ("plane-skew", 3),
    "far": ("far", 2), "far-descending": ("far-descending", 2),
    "bands-tail-descending": ("descending", 70),
    "skewed-step-2": ("skewed", 3), "skewed-step-1": ("skewed", 3),
    "table-twin": ("table-twin", 3),
}
SKEW = {"skewed-step-2": 2, "skewed-step-1": 1}
TWIN_SLOTS = [2, 3, 0]


def _up(v, a):
    return (v + a - 1) // a * a


class Plane:
    """rows x row_bytes samples at pitch `stride`; unit: what the entry point requires a base pointer to be a multiple of (1: any
    address is accepted, so the skewed classes apply); room: bytes behind the last row that hold no sample and lie inside a
    window all the same (an opaque decoder's planar CHW target: where a fourth plane would be); stacked: how many planes of a
    planar CHW surface the rows are (1: no such surface)."""

    def __init__(self, name, row_bytes, rows, stride, unit=1, room=0, stacked=1):
        assert stride >= row_bytes and rows % stacked == 0
        self.name, self.row_bytes, self.rows, self.stride, self.unit, self.room, self.stacked = name, row_bytes, rows, stride, unit, room, stacked
        self.extent = stride * (rows - 1) + row_bytes

    def index(self, off):
        """Indices of the samples, (rows, row_bytes), in an array whose element 0 is `off` bytes before the plane."""
        return off + np.arange(self.rows)[:, None] * self.stride + np.arange(self.row_bytes)[None, :]


class Route:
    """entry: "decode" | "half" | "scaled" | "render" | "unconvert" | "encode".  size / out_size: (w, h) of a frame and of its
    target.  kernel: what bt709hip_last_kernel_name must report; taps: (tap form, persistent) of bt709hip_last_scaled_launch_info;
    skew: skew residue -> (kernel, taps) of the demoted launch; bands: the launch splits under bands-tail-descending.
    chw: the element type ("uint8" / "float16" / "float32") of the route's planar CHW side -- the target of a decode, the input
    of an encode -- which is ONE plane of chw_planes x H rows of W x e bytes; norm: its (scale, bias) setting, which the decoder
    options / context options carry; ctx_options: context options set for every call and put back to CTX_DEFAULTS after it;
    table: the most frames the entry point's pointer table holds (a paired encode: pairs)."""

    def __init__(self, name, entry, size, out_size, ins, outs, kernel, gamma=GAMMA_APPLE, alpha=False, options=(), over=None, fmt=SRGB8,
                 in_fmt=SRGB8, taps=None, skew=None, bands=False, reads_destination=False, pair=None, no_skew=None, chw=None, norm=None,
                 ctx_options=(), table=32):
        self.name, self.entry, self.size, self.out_size, self.ins, self.outs, self.kernel = name, entry, size, out_size, ins, outs, kernel
        self.gamma, self.alpha, self.options, self.over, self.fmt, self.in_fmt = gamma, alpha, tuple(options), over, fmt, in_fmt
        self.taps, self.skew, self.bands, self.reads_destination, self.pair, self.no_skew = taps, skew, bands, reads_destination, pair, no_skew
        self.chw, self.norm, self.ctx_options, self.table = chw, norm, tuple(ctx_options), table
        self.key = name  # what frame_data / want remember a route's frames under: a resized copy (tests/extent_cases.py) takes its own

    @property
    def planar_chroma(self):
        """The "cbcr" plane is U's rows, then V's, at one pitch (I420): the frames a decoder reads, or the ones the encoder writes."""
        return (dict(self.options).get(_capi.OPT_CHROMA_LAYOUT) == _capi.CHROMA_I420
                or dict(self.ctx_options).get(_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT) == _capi.CHROMA_I420)

    @property
    def paired(self):
        """Two frames a picture (BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA / _HALF_WITH_ALPHA): the colour frames, then the alpha frames."""
        o = dict(self.ctx_options)
        return bool(o.get(_capi.CTX_OPT_ENCODE_WITH_ALPHA) or o.get(_capi.CTX_OPT_ENCODE_HALF_WITH_ALPHA))

    @property
    def convert(self):
        return dict(self.ctx_options).get(_capi.CTX_OPT_ENCODE_CONVERT, _capi.CONVERT_OFF)

    @property
    def elem(self):
        return np.dtype(self.chw).itemsize

    @property
    def chw_planes(self):
        return 4 if self.alpha and self.entry != "encode" else 3

    def plane(self, name):
        return next(p for p in self.ins + self.outs if p.name == name)

    def classes(self):
        """The classes that apply (see CLASSES_NOT_RUN for the others)."""
        out = ["descending-2", "descending-3", "descending-33", "crossed-up-down", "crossed-down-up", "fan-out"]
        if len(self.ins) > 1 or len(self.outs) > 1:
            out.append("plane-skew")
        out += ["far", "far-descending"]
        if self.bands:
            out.append("bands-tail-descending")
        if self.skew:
            out += [c for c in SKEW if SKEW[c] in self.skew]
        out.append("table-twin")
        return out


def _nv12(w, h, sy, sc, sa=None):
    planes = [Plane("y", w, h, sy), Plane("cbcr", w, h // 2, sc)]
    return planes + ([Plane("alpha", w, h, sa)] if sa else [])


def _out(ow, oh, pad, px=4):
    return [Plane("out", px * ow, oh, px * ow + pad, unit=px)]


def _chw_out(ow, oh, dtype, planes, pad):
    """A planar CHW target: planes R, G, B (and A) stacked at one pitch, as the "cbcr" plane of an I420 frame stacks U and V.  An
    opaque decoder's three planes are given the room of a fourth behind them."""
    e = np.dtype(dtype).itemsize
    return [Plane("out", e * ow, planes * oh, e * ow + pad, unit=e, room=(4 - planes) * oh * (e * ow + pad), stacked=planes)]


def _chw_in(w, h, dtype, pad):
    """A planar CHW tensor the encoder reads: planes R, G, B (a fourth is never touched)."""
    e = np.dtype(dtype).itemsize
    return [Plane("chw", e * w, 3 * h, e * w + pad, unit=e, stacked=3)]


def _settings(first, setting):
    return tuple((first + i, cc.bits(v)) for i, v in enumerate(tuple(setting[0]) + tuple(setting[1])))


CHW_NORM = _settings(_capi.OPT_CHW_SCALE_R, cc.IMAGENET)  # BT709HIP_OPT_CHW_SCALE_R .. _BIAS_B of a decoder
NV12, I420 = _capi.CHROMA_NV12, _capi.CHROMA_I420
# what a context holds before and after a call of a route with ctx_options
CTX_DEFAULTS = dict(((_capi.CTX_OPT_ENCODE_CHW_INPUT, 0), (_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, NV12), (_capi.CTX_OPT_ENCODE_PREMULTIPLY, 0),
                     (_capi.CTX_OPT_ENCODE_CONVERT, _capi.CONVERT_OFF), (_capi.CTX_OPT_ENCODE_WITH_ALPHA, 0), (_capi.CTX_OPT_ENCODE_HALF_INPUT, 0),
                     (_capi.CTX_OPT_ENCODE_HALF_WITH_ALPHA, 0)) + _settings(_capi.CTX_OPT_ENCODE_CHW_SCALE_R, ecc.IDENTITY))
_encode_chw = lambda layout: ((_capi.CTX_OPT_ENCODE_CHW_INPUT, 1), (_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, layout)) + _settings(_capi.CTX_OPT_ENCODE_CHW_SCALE_R, ecc.IMAGENET)
_chw_kernel = lambda dtype, layout, fast: ecc.kernel_name(dtype, layout, fast).encode()

_LAYOUT_I420 = (_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, I420)
_PREMUL, _WITH_ALPHA = (_capi.CTX_OPT_ENCODE_PREMULTIPLY, 1), (_capi.CTX_OPT_ENCODE_WITH_ALPHA, 1)
_HALF_INPUT, _HALF_WITH_ALPHA = (_capi.CTX_OPT_ENCODE_HALF_INPUT, 1), (_capi.CTX_OPT_ENCODE_HALF_WITH_ALPHA, 1)
_convert = lambda mode: (_capi.CTX_OPT_ENCODE_CONVERT, mode)
PAIR_TABLE = 16  # BT709HIP_MAX_BATCH / 2: the pointer table of a paired launch


def _bgra_in(w, h, pad):
    return [Plane("bgra", 4 * w, h, 4 * w + pad, unit=4)]


def _half_in(w, h, pad):
    return [Plane("rgba16f", 8 * w, h, 8 * w + pad, unit=8)]


def _i420(w, h, sy, sc):
    """The planes an I420 encode writes: Y, and U's H/2 rows then V's at one pitch."""
    return [Plane("y", w, h, sy), Plane("cbcr", w // 2, h, sc)]


def _alpha_nv12(w, h, sy, sc=None):
    """The alpha frame of a pair, behind the colour frame's planes: its Y and (sc) its interleaved chroma plane."""
    return [Plane("alpha_y", w, h, sy)] + ([Plane("alpha_cbcr", w, h // 2, sc)] if sc else [])


def _words(w, h, pad):
    """The packed converter's target: W x H 4-byte words through the frame's `y` pointer and pitch, no chroma plane."""
    return [Plane("y", 4 * w, h, 4 * w + pad, unit=4)]


_both = lambda kernel: {2: (kernel, None), 1: (kernel, None)}
NO_BYTE_PLANE = "no byte-addressed plane: texels in, 4-byte words out (BT709HIP_ERR_STRIDE off a multiple of 4)"
_demoted = lambda name: "already the kernel a skewed step demotes to (the %s route runs the class)" % name

W, H = 64, 16
HALF_REP =((_capi.OPT_HALF_KERNEL, 1), (_capi.OPT_HALF_WORKGROUPS, 3))  # three persistent workgroups: the cursor wraps from frame to frame
ONCE, WIDE, PAIRS, BYTES = _capi.SCALED_TAPS_ONCE, _capi.SCALED_TAPS_WIDE, _capi.SCALED_TAPS_PAIRS, _capi.SCALED_TAPS_BYTES
DOWN = dict(size=(W, H), out_size=(40, 10))  # 1.6 : 1 both ways, the per-lane (persistent) forms
_scaled_skew = lambda kernel: {2: (kernel, (PAIRS, 1)), 1: (kernel, (BYTES, 1))}

ROUTES = [
    # ---- bt709hip_decode_batch
    Route("quads", "decode", (W, H), (W, H), _nv12(W, H, 80, 80), _out(W, H, 16), b"decode_nv12_quads<nt>", bands=True,
          skew={2: (b"decode_nv12_blocks", None), 1: (b"decode_nv12_blocks", None)}),
    Route("blocks", "decode", (W, H), (W, H), _nv12(W, H, 65, 67), _out(W, H, 4), b"decode_nv12_blocks",
          no_skew="variant_cases.LAUNCH_CASES step-40 / bands-72 (step_pad (1, 4)) pin the general kernel at an odd step"),
    Route("quads-over", "decode", (W, H), (W, H), _nv12(W, H, 80, 80, 96), _out(W, H, 16), b"decode_nv12_quads<alpha,over>", gamma=GAMMA_SRGB, alpha=True,
          over=_capi.OVER_DESTINATION, reads_destination=True, bands=True,
          skew={2: (b"decode_nv12_blocks<alpha,over>", None), 1: (b"decode_nv12_blocks<alpha,over>", None)}),
    # planar chroma: the "cbcr" plane is U's H/2 rows, then V's, at one pitch -- V follows each frame's own U
    Route("i420", "decode", (W, H), (W, H), [Plane("y", W, H, 80), Plane("cbcr", W // 2, H, 48)], _out(W, H, 16), b"decode_i420_quads<nt>",
          options=((_capi.OPT_CHROMA_LAYOUT, _capi.CHROMA_I420),), bands=True,
          skew={2: (b"decode_i420_blocks", None), 1: (b"decode_i420_blocks", None)}),
    Route("rgba16f-alpha", "decode", (W, H), (W, H), _nv12(W, H, 80, 80, 96), _out(W, H, 16, px=8), b"decode_nv12_rgba16f<alpha>", gamma=GAMMA_SRGB,
          alpha=True, fmt=F16, bands=True, skew={2: (b"decode_nv12_rgba16f<alpha>", None), 1: (b"decode_nv12_rgba16f<alpha>", None)}),
    # ---- bt709hip_decode_half_batch
    Route("half-wide", "half", (W, H), (W // 2, H // 2), _nv12(W, H, 80, 80), _out(W // 2, H // 2, 16), b"decode_nv12_half<wide>",
          skew={2: (b"decode_nv12_half<narrow>", None), 1: (b"decode_nv12_half<narrow>", None)}),
    Route("half-narrow", "half", (W, H), (W // 2, H // 2), _nv12(W, H, 65, 67), _out(W // 2, H // 2, 4), b"decode_nv12_half<narrow>",
          no_skew="already the kernel a skewed step demotes to (the half-wide route runs the class)"),
    Route("half-rep-alpha", "half", (W, H), (W // 2, H // 2), _nv12(W, H, 80, 80, 96), _out(W // 2, H // 2, 16), b"decode_nv12_half_rep<alpha>",
          gamma=GAMMA_SRGB, alpha=True, options=HALF_REP,
          skew={2: (b"decode_nv12_half<narrow,alpha>", None), 1: (b"decode_nv12_half<narrow,alpha>", None)}),
    # ---- bt709hip_decode_scaled_batch
    Route("scaled-once", "scaled", (32, 8), (64, 16), _nv12(32, 8, 48, 48), _out(64, 16, 16), b"decode_nv12_scaled", taps=(ONCE, 0),
          skew={2: (b"decode_nv12_scaled", (ONCE, 0)), 1: (b"decode_nv12_scaled", (BYTES, 1))}),
    Route("scaled-wide", "scaled", ins=_nv12(W, H, 80, 80), outs=_out(40, 10, 16), kernel=b"decode_nv12_scaled", taps=(WIDE, 1),
          skew=_scaled_skew(b"decode_nv12_scaled"), **DOWN),
    Route("scaled-f16", "scaled", ins=_nv12(W, H, 80, 80), outs=_out(40, 10, 16), kernel=b"decode_nv12_scaled_f16", taps=(WIDE, 1),
          options=((_capi.OPT_SCALE_INTERMEDIATE, F16),), skew=_scaled_skew(b"decode_nv12_scaled_f16"), **DOWN),
    Route("scaled-over", "scaled", ins=_nv12(W, H, 80, 80, 96), outs=_out(40, 10, 16), kernel=b"decode_nv12_scaled<alpha,over>", taps=(WIDE, 1),
          gamma=GAMMA_SRGB, alpha=True, options=((_capi.OPT_SCALED_OVER, _capi.OVER_DESTINATION),), reads_destination=True,
          skew=_scaled_skew(b"decode_nv12_scaled<alpha,over>"), **DOWN),
    # ---- bt709hip_render_scaled_batch (no pointer table: surfaces that are not evenly spaced are refused)
    Route("render-bgra8", "render", (W, H), (40, 10), [Plane("in", 4 * W, H, 4 * W + 16, unit=4)], _out(40, 10, 16), b"render_scaled<bgra8>",
          no_skew="every surface base must be a multiple of the texel size (BT709HIP_ERR_STRIDE: tests/test_batch_spacing_cpu.py)"),
    Route("render-rgba16f", "render", (W, H), (40, 10), [Plane("in", 8 * W, H, 8 * W + 16, unit=8)], _out(40, 10, 16), b"render_scaled<rgba16f>",
          in_fmt=F16, no_skew="every surface base must be a multiple of the texel size (BT709HIP_ERR_STRIDE: tests/test_batch_spacing_cpu.py)"),
    # ---- bt709hip_unconvert_batch
    Route("unconvert-vec", "unconvert", (W, 8), (W, 8), [Plane("in", 4 * W, 8, 4 * W + 16, unit=4)], _out(W, 8, 16), b"unconvert_packed444<vec>",
          no_skew="words and texels must be 4-byte aligned"),
    Route("unconvert-pixel", "unconvert", (30, 6), (30, 6), [Plane("in", 120, 6, 124, unit=4)], _out(30, 6, 8), b"unconvert_packed444",
          no_skew="words and texels must be 4-byte aligned"),
    # ---- bt709hip_encode_batch
    Route("encode-fast", "encode", (W, H), (W, H), [Plane("bgra", 4 * W, H, 4 * W + 16, unit=4)], _nv12(W, H, 80, 80), b"encode_bgra_nv12",
          pair=(GAMMA_SRGB, GAMMA_APPLE), bands=True, skew={2: (b"encode_bgra_nv12_blocks", None), 1: (b"encode_bgra_nv12_blocks", None)}),
    Route("encode-blocks", "encode", (W, H), (W, H), [Plane("bgra", 4 * W, H, 4 * W + 4, unit=4)], _nv12(W, H, 65, 67), b"encode_bgra_nv12_blocks",
          pair=(GAMMA_SRGB, GAMMA_APPLE), no_skew="already the kernel a skewed step demotes to (the encode-fast route runs the class)"),
    # an alpha clip's luma with cbcr == NULL in every frame: the split launch's tail passes advance_frames' `if (cbcr)`
    Route("encode-alpha-y", "encode", (W, H), (W, H), [Plane("bgra", 4 * W, H, 4 * W + 16, unit=4)], [Plane("y", W, H, 80)], b"encode_alpha_y",
          pair=(GAMMA_LINEAR, GAMMA_LINEAR), in_fmt=ALPHA8, bands=True, skew={2: (b"encode_alpha_y_blocks", None), 1: (b"encode_alpha_y_blocks", None)}),
    # ---- planar CHW: plane c of a surface starts c x H x pitch behind plane 0, the one address product no
    # route above forms.  Appended: _route_seed is the index.
    # bt709hip_decode_batch into CHW targets.  A u8 plane is byte-addressed: a skewed step skews the target as well
    Route("chw-quads-u8", "decode", (W, H), (W, H), _nv12(W, H, 80, 80), _chw_out(W, H, "uint8", 3, 16), b"decode_nv12_quads_chw<u8,nt>",
          fmt=cc.FORMATS["uint8"], chw="uint8", bands=True, skew={2: (b"decode_nv12_blocks_chw<u8>", None), 1: (b"decode_nv12_blocks_chw<u8>", None)}),
    Route("chw-quads-f16-alpha", "decode", (W, H), (W, H), _nv12(W, H, 80, 80, 96), _chw_out(W, H, "float16", 4, 16), b"decode_nv12_quads_chw<f16,alpha>",
          gamma=GAMMA_SRGB, alpha=True, options=CHW_NORM, fmt=cc.FORMATS["float16"], chw="float16", norm=cc.IMAGENET, bands=True,
          skew={2: (b"decode_nv12_blocks_chw<f16,alpha>", None), 1: (b"decode_nv12_blocks_chw<f16,alpha>", None)}),
    Route("chw-quads-f32-i420", "decode", (W, H), (W, H), [Plane("y", W, H, 80), Plane("cbcr", W // 2, H, 48)], _chw_out(W, H, "float32", 3, 16),
          b"decode_i420_quads_chw<f32,nt>", options=((_capi.OPT_CHROMA_LAYOUT, I420),) + CHW_NORM, fmt=cc.FORMATS["float32"], chw="float32",
          norm=cc.IMAGENET, bands=True, skew={2: (b"decode_i420_blocks_chw<f32>", None), 1: (b"decode_i420_blocks_chw<f32>", None)}),
    Route("chw-blocks-f16", "decode", (W, H), (W, H), _nv12(W, H, 65, 67), _chw_out(W, H, "float16", 3, 2), b"decode_nv12_blocks_chw<f16>",
          options=CHW_NORM, fmt=cc.FORMATS["float16"], chw="float16", norm=cc.IMAGENET,
          no_skew="already the kernel a skewed step demotes to (the chw-quads routes run the class)"),
    # bt709hip_decode_scaled_batch under BT709HIP_OPT_SCALED_CHW: the plane offset rides in 32 bits (scaled_planes_fit)
    Route("scaled-chw-u8", "scaled", ins=_nv12(W, H, 80, 80), outs=_chw_out(40, 10, "uint8", 3, 16), kernel=b"decode_nv12_scaled_chw<u8>", taps=(WIDE, 1),
          options=((_capi.OPT_SCALED_CHW, 1),), fmt=cc.FORMATS["uint8"], chw="uint8", skew=_scaled_skew(b"decode_nv12_scaled_chw<u8>"), **DOWN),
    Route("scaled-chw-f32-alpha", "scaled", (32, 8), (64, 16), _nv12(32, 8, 48, 48, 64), _chw_out(64, 16, "float32", 4, 16), b"decode_nv12_scaled_chw<f32,alpha>",
          gamma=GAMMA_SRGB, alpha=True, taps=(ONCE, 0), options=((_capi.OPT_SCALED_CHW, 1),) + CHW_NORM, fmt=cc.FORMATS["float32"], chw="float32",
          norm=cc.IMAGENET, skew={2: (b"decode_nv12_scaled_chw<f32,alpha>", (ONCE, 0)), 1: (b"decode_nv12_scaled_chw<f32,alpha>", (BYTES, 1))}),
    # bt709hip_encode_batch under BT709HIP_CTX_OPT_ENCODE_CHW_INPUT: the pointer table of such a launch holds 31 surfaces
    Route("encode-chw-f16", "encode", (W, H), (W, H), _chw_in(W, H, "float16", 16), _nv12(W, H, 80, 80), _chw_kernel("float16", NV12, True),
          pair=(GAMMA_SRGB, GAMMA_APPLE), in_fmt=cc.FORMATS["float16"], chw="float16", norm=ecc.IMAGENET, ctx_options=_encode_chw(NV12), table=ecc.MAX_TABLE,
          bands=True, skew={2: (_chw_kernel("float16", NV12, False), None), 1: (_chw_kernel("float16", NV12, False), None)}),
    Route("encode-chw-f32-blocks", "encode", (W, H), (W, H), _chw_in(W, H, "float32", 4), _nv12(W, H, 65, 67), _chw_kernel("float32", NV12, False),
          pair=(GAMMA_SRGB, GAMMA_APPLE), in_fmt=cc.FORMATS["float32"], chw="float32", norm=ecc.IMAGENET, ctx_options=_encode_chw(NV12), table=ecc.MAX_TABLE,
          no_skew="already the kernel a skewed step demotes to (the encode-chw-f16 route runs the class)"),
    # into planar I420: the "cbcr" plane as the i420 decode route has it
    Route("encode-chw-u8-i420", "encode", (W, H), (W, H), _chw_in(W, H, "uint8", 16), [Plane("y", W, H, 80), Plane("cbcr", W // 2, H, 48)],
          _chw_kernel("uint8", I420, True), pair=(GAMMA_SRGB, GAMMA_APPLE), in_fmt=cc.FORMATS["uint8"], chw="uint8", norm=ecc.IMAGENET,
          ctx_options=_encode_chw(I420), table=ecc.MAX_TABLE, bands=True,
          skew={2: (_chw_kernel("uint8", I420, False), None), 1: (_chw_kernel("uint8", I420, False), None)}),
    # ---- the encoder's other families (appended: _route_seed is the index).  Pad 16 selects a fast kernel, pad 4 (8 for half
    # texels) the general one; a skewed route's demotion is read off the alignment rules of include/bt709hip_ext.h: the BGRA8 forms
    # and the BGRA8 pair store dwords to Y and alpha Y (pointer, pitch and step 4-byte aligned), the RGBA16Float forms halves
    # BGRA -> planar I420: V's rows lie (H/2) x pitch behind U's (v_plane_offset)
    Route("encode-i420", "encode", (W, H), (W, H), _bgra_in(W, H, 16), _i420(W, H, 80, 48), b"encode_bgra_i420", pair=(GAMMA_SRGB, GAMMA_APPLE),
          ctx_options=(_LAYOUT_I420,), bands=True, skew=_both(b"encode_bgra_i420_blocks")),
    Route("encode-i420-blocks-premul", "encode", (W, H), (W, H), _bgra_in(W, H, 4), _i420(W, H, 65, 35), b"encode_bgra_i420_blocks<premul>",
          pair=(GAMMA_SRGB, GAMMA_APPLE), ctx_options=(_LAYOUT_I420, _PREMUL), no_skew=_demoted("encode-i420")),
    # +convert: packed words through the `y` pointer and pitch, and the point-sampled frame
    Route("convert-packed", "encode", (W, H), (W, H), _bgra_in(W, H, 16), _words(W, H, 32), b"convert_bgra_packed444", pair=(GAMMA_SRGB, GAMMA_APPLE),
          ctx_options=(_convert(_capi.CONVERT_PACKED444),), bands=True, no_skew=NO_BYTE_PLANE),
    Route("convert-packed-blocks", "encode", (W, H), (W, H), _bgra_in(W, H, 4), _words(W, H, 4), b"convert_bgra_packed444_blocks",
          pair=(GAMMA_SRGB, GAMMA_APPLE), ctx_options=(_convert(_capi.CONVERT_PACKED444),), no_skew=NO_BYTE_PLANE),
    Route("convert-point-i420", "encode", (W, H), (W, H), _bgra_in(W, H, 16), _i420(W, H, 80, 48), b"convert_bgra_i420", pair=(GAMMA_SRGB, GAMMA_APPLE),
          ctx_options=(_convert(_capi.CONVERT_POINT420), _LAYOUT_I420), bands=True, skew=_both(b"convert_bgra_i420_blocks")),
    # the colour + alpha pair: five planes, the alpha frame's pitches and steps in the table's spare slots, 16 pairs in the table
    Route("encode-pair", "encode", (W, H), (W, H), _bgra_in(W, H, 16), _nv12(W, H, 80, 80) + _alpha_nv12(W, H, 96, 112), b"encode_bgra_alpha_nv12",
          pair=(GAMMA_SRGB, GAMMA_APPLE), ctx_options=(_WITH_ALPHA,), table=PAIR_TABLE, bands=True, skew=_both(b"encode_bgra_alpha_nv12_blocks")),
    # ... into I420, premultiplying, the alpha frames without a chroma plane (NULL in every pair)
    Route("encode-pair-i420-blocks", "encode", (W, H), (W, H), _bgra_in(W, H, 4), _i420(W, H, 65, 35) + _alpha_nv12(W, H, 67),
          b"encode_bgra_alpha_i420_blocks<premul>", pair=(GAMMA_SRGB, GAMMA_APPLE), ctx_options=(_WITH_ALPHA, _LAYOUT_I420, _PREMUL), table=PAIR_TABLE,
          no_skew=_demoted("encode-pair")),
    # RGBA16Float input (linear light): the fast kernel needs 2-byte Y and CbCr only -- a step = 2 (mod 4) keeps it, an odd one demotes
    Route("encode-half", "encode", (W, H), (W, H), _half_in(W, H, 16), _nv12(W, H, 80, 80), b"encode_rgba16f_nv12", pair=(GAMMA_LINEAR, GAMMA_APPLE),
          in_fmt=F16, ctx_options=(_HALF_INPUT,), bands=True, skew={2: (b"encode_rgba16f_nv12", None), 1: (b"encode_rgba16f_nv12_blocks", None)}),
    Route("encode-half-i420-blocks", "encode", (W, H), (W, H), _half_in(W, H, 8), _i420(W, H, 65, 35), b"encode_rgba16f_i420_blocks",
          pair=(GAMMA_LINEAR, GAMMA_APPLE), in_fmt=F16, ctx_options=(_HALF_INPUT, _LAYOUT_I420), no_skew=_demoted("encode-half")),
    # the RGBA16Float pair, under a second output curve
    Route("encode-half-pair", "encode", (W, H), (W, H), _half_in(W, H, 16), _nv12(W, H, 80, 80) + _alpha_nv12(W, H, 96, 112), b"encode_rgba16f_alpha_nv12",
          pair=(GAMMA_LINEAR, GAMMA_SRGB), in_fmt=F16, ctx_options=(_HALF_INPUT, _HALF_WITH_ALPHA), table=PAIR_TABLE, bands=True,
          skew={2: (b"encode_rgba16f_alpha_nv12", None), 1: (b"encode_rgba16f_alpha_nv12_blocks", None)}),
]
ROUTE = {r.name: r for r in ROUTES}
PAIRS_RUN = [(r.name, c) for r in ROUTES for c in r.classes()]
# what is not run, and why: (route, class) -> reason
CLASSES_NOT_RUN = {(r.name, c): r.no_skew for r in ROUTES if r.no_skew for c in SKEW}
CLASSES_NOT_RUN.update({(r.name, "plane-skew"): "one input plane and one output plane" for r in ROUTES if len(r.ins) == 1 and len(r.outs) == 1})
CLASSES_NOT_RUN.update({(r.name, "bands-tail-descending"): "the launch is never split (no XCD-band map for this kernel)" for r in ROUTES if not r.bands})
# every kernel name a route leaves on record: its own, and the one a skewed step demotes it to
REPORTED = {r.kernel.decode() for r in ROUTES} | {k.decode() for r in ROUTES if r.skew for k, _ in r.skew.values()}


def _forms_not_routed():
    """kernel name -> why it has no route: the name on record (above) whose body it instantiates.  The names
    bt709hip_last_kernel_name can report for the 1:1 alpha decodes, the RGBA16Float target, the fused rescales and the encoder
    that no route or skew class reaches -- every layout and <premul> combination of the encoder; of the decode side the forms
    that differ from a routed one in what they do with A alone (no census of its quantiser and log-table instantiations, which
    the decoder's state selects, not its addressing)."""
    same = lambda what, routed: "%s of the body %s addresses through" % (what, routed)
    forms = {}
    for layout in ("nv12", "i420"):
        for shape, over in (("quads", "decode_nv12_quads<alpha,over>"), ("blocks", "decode_nv12_blocks<alpha,over>")):
            plain = "decode_nv12_quads<nt>" if shape == "quads" else "decode_nv12_blocks"
            forms["decode_%s_%s<alpha,straight>" % (layout, shape)] = same("the alpha instantiation that divides A out in registers,", plain)
            forms["decode_%s_%s<alpha,over-colour>" % (layout, shape)] = same("the composite over a constant colour,", over)
    forms["decode_nv12_rgba16f"] = same("the opaque instantiation", "decode_nv12_rgba16f<alpha>")
    forms["decode_nv12_scaled<alpha,over-colour>"] = same("the composite over a constant colour,", "decode_nv12_scaled<alpha,over>")
    for suffix in ("<alpha>", "<alpha,over>", "<alpha,over-colour>"):
        forms["decode_nv12_scaled_f16" + suffix] = same("the alpha / composite instantiation through the RGBA16Float intermediate,", "decode_nv12_scaled_f16")
    # the encoder: every family is one fast and one general body over the chroma layout (and, BGRA8 input, the premultiply bit)
    families = [("encode_bgra_%s", "encode_bgra_nv12", "encode_bgra_nv12_blocks", True),
                ("convert_bgra_%s", "convert_bgra_i420", "convert_bgra_i420_blocks", True),
                ("encode_bgra_alpha_%s", "encode_bgra_alpha_nv12", "encode_bgra_alpha_nv12_blocks", True),
                ("encode_rgba16f_%s", "encode_rgba16f_nv12", "encode_rgba16f_nv12_blocks", False),
                ("encode_rgba16f_alpha_%s", "encode_rgba16f_alpha_nv12", "encode_rgba16f_alpha_nv12_blocks", False)]
    for stem, fast, blocks, premul in families:
        for layout in ("nv12", "i420"):
            for general in (False, True):
                for straight in ((False, True) if premul else (False,)):
                    name = stem % layout + ("_blocks" if general else "") + ("<premul>" if straight else "")
                    forms[name] = same("the %s%s instantiation" % (layout.upper(), ", premultiplying" if straight else ""), blocks if general else fast)
    for general in (False, True):  # the packed words: one instantiation under both layouts
        name = "convert_bgra_packed444" + ("_blocks" if general else "")
        forms[name + "<premul>"] = same("the premultiplying instantiation", name)
    for elem in ("u8", "f16", "f32"):
        for layout in ("nv12", "i420"):
            forms["encode_chw_%s<%s>" % (layout, elem)] = same("the %s, %s instantiation" % (layout.upper(), elem), "encode_chw_nv12<f16>")
            forms["encode_chw_%s_blocks<%s>" % (layout, elem)] = same("the %s, %s instantiation" % (layout.upper(), elem), "encode_chw_nv12_blocks<f32>")
    forms["encode_alpha_y<i420>"] = same("the alpha frame with U and V planes of 128,", "encode_alpha_y")
    forms["encode_alpha_y_blocks<i420>"] = same("the alpha frame with U and V planes of 128,", "encode_alpha_y_blocks")
    return {name: why for name, why in forms.items() if name not in REPORTED}


FORMS_NOT_ROUTED = _forms_not_routed()


class Layout:
    """in_off / out_off: plane name -> byte offset of every frame's plane in its slab; steps: plane name -> step, None under
    table-twin; source[i]: which frame's samples frame i reads (fan-out: all read frame 0's); *_windows: [(lo, hi)] the host
    touches; *_alias: [(lo, hi)] among them that hold no frame."""

    def __init__(self, route, cls):
        self.route, self.cls = route, cls
        self.kind, self.n = CLASSES[cls]
        self.uniform = self.kind != "table-twin"
        self.in_off, self.out_off, self.steps = {}, {}, {}
        self.in_windows, self.out_windows, self.in_alias, self.out_alias = [], [], [], []
        self.source = [0] * self.n if self.kind == "fan-out" else list(range(self.n))

    def side(self, which):
        return (self.route.ins, self.in_off, self.in_windows, self.in_alias) if which == "in" else (self.route.outs, self.out_off, self.out_windows, self.out_alias)

    def extents(self, which):
        """The byte ranges that hold samples or are an alias window, each once."""
        planes, off, _, alias = self.side(which)
        return sorted({(o, o + p.extent) for p in planes for o in off[p.name]} | set(alias))

    def check(self):
        r, n = self.route, self.n
        for which in ("in", "out"):
            planes, off, windows, alias = self.side(which)
            ext = self.extents(which)
            assert all(0 <= lo < hi <= SLAB_BYTES for lo, hi in ext), (r.name, self.cls, which, "outside the slab")
            # pairwise disjoint and not adjacent: a guard band between any two
            assert all(b[0] - a[1] >= GUARD for a, b in zip(ext, ext[1:])), (r.name, self.cls, which, "overlapping or adjacent")
            # every one of them, with its guard bands, lies in exactly one window; the windows are disjoint and inside the slab
            assert all(0 <= lo < hi <= SLAB_BYTES for lo, hi in windows)
            ws = sorted(windows)
            assert all(a[1] <= b[0] for a, b in zip(ws, ws[1:]))
            for lo, hi in ext:
                g = 0 if (lo, hi) in alias else GUARD
                assert sum(1 for wl, wh in windows if wl <= lo - g and hi + g <= wh) == 1, (r.name, self.cls, which, lo, hi)
            for p in planes:
                o, step = off[p.name], self.steps[p.name]
                if p.room:  # the place of a fourth plane: in the frame's own window, and no other frame or alias window in it
                    for v in o:
                        assert sum(1 for wl, wh in windows if wl <= v and v + p.extent + p.room + GUARD <= wh) == 1, (r.name, self.cls, p.name)
                        assert all(hi <= v or lo >= v + p.extent + p.room + GUARD for lo, hi in ext if lo != v), (r.name, self.cls, p.name)
                assert len(o) == n and all(v % p.unit == 0 for v in o) and o[0] % 16 == 0
                if self.uniform:
                    assert all(o[i] == o[0] + i * step for i in range(n)), (r.name, self.cls, p.name)
                else:
                    assert step is None and n > 2 and any(o[i] - o[0] != i * (o[1] - o[0]) for i in range(n)), (r.name, self.cls, p.name)
        steps = [self.steps[p.name] for p in r.ins + r.outs]
        ins, outs = [self.steps[p.name] for p in r.ins], [self.steps[p.name] for p in r.outs]
        if self.kind == "descending":
            assert all(s < 0 for s in steps)
        elif self.kind in ("crossed-up-down", "crossed-down-up"):
            up = self.kind == "crossed-up-down"
            assert all((s > 0) == up for s in ins) and all((s < 0) == up for s in outs)
        elif self.kind == "fan-out":
            assert all(s == 0 for s in ins) and all(s > 0 for s in outs)
        elif self.kind == "plane-skew":
            assert len(set(steps)) == len(steps) and any(s < 0 for s in steps) and any(s > 0 for s in steps)
        elif self.kind in ("far", "far-descending"):
            sign = 1 if self.kind == "far" else -1
            for which in ("in", "out"):
                planes, off, _, alias = self.side(which)
                assert len(alias) == len(planes)
                for p in planes:
                    o, d = off[p.name], sign * self.steps[p.name] - FAR
                    assert 0 < d < (1 << 20) and d % 16 == 0 and max(o) >= FAR and min(o) < (1 << 20)
                    cut = self.steps[p.name] & 0xFFFFFFFF  # the step's low 32 bits: zero-extended as they are, sign-extended below
                    landed = o[0] + (cut if sign > 0 else cut - FAR)
                    assert (landed, landed + p.extent) in alias, (r.name, self.cls, p.name)
        elif self.kind == "skewed":
            k = SKEW[self.cls]
            for p in r.ins + r.outs:
                s = self.steps[p.name]
                assert s > 0 and (s % 4 == 2 if k == 2 else s % 2 == 1) if p.unit == 1 else s % 16 == 0
            assert any(p.unit == 1 for p in r.ins + r.outs)
        return self


def _slots(kind, n, which, j):
    """Which slot of plane j's region frame i lies in."""
    up, down = list(range(n)), list(range(n - 1, -1, -1))
    if kind == "descending":
        return down
    if kind in ("crossed-up-down", "crossed-down-up"):
        return up if (which == "in") == (kind == "crossed-up-down") else down
    if kind == "fan-out":
        return [0] * n if which == "in" else up
    if kind == "plane-skew":  # outputs a slot more than inputs: an output plane as large as an input plane still steps differently
        return [k * (j + (1 if which == "in" else 2)) for k in (down if j % 2 else up)]
    if kind == "table-twin":
        return TWIN_SLOTS
    return up  # skewed


def build(route, cls):
    L = Layout(route, cls)
    kind, n = L.kind, L.n
    for which in ("in", "out"):
        planes, off, windows, alias = L.side(which)
        if kind in ("far", "far-descending"):
            cursor = 0
            for p in planes:
                span = p.extent + p.room
                d = _up(span + 2 * GUARD + 16, 16)
                low = cursor + GUARD
                high = low + FAR + d
                off[p.name] = [low, high] if kind == "far" else [high, low]
                L.steps[p.name] = off[p.name][1] - off[p.name][0]
                a = low + d if kind == "far" else low + FAR  # frame 0 + the step's low 32 bits
                alias.append((a, a + p.extent))
                windows += [(low - GUARD, low + span + GUARD), (high - GUARD, high + span + GUARD), (a, a + p.extent)]
                cursor += _up(2 * GUARD + d + span, 256)
            assert cursor <= (1 << 20) - GUARD
        else:
            cursor = NEAR_ORIGIN
            for j, p in enumerate(planes):
                pitch = _up(p.extent + p.room + 2 * GUARD, 256) + (SKEW.get(cls, 0) if p.unit == 1 else 0)
                slots = _slots(kind, n, which, j)
                off[p.name] = [cursor + GUARD + k * pitch for k in slots]
                L.steps[p.name] = off[p.name][1] - off[p.name][0] if L.uniform else None
                cursor = _up(cursor + GUARD + max(max(slots) + 1, 4) * pitch + GUARD, 256)  # at least table-twin's four slots: its frames 0 and 2 are descending-3's
            windows.append((NEAR_ORIGIN, cursor))
    return L.check()


# ------------------------------------------------------------------ descriptors and calls (the product library or the fake-runtime build)

class Call:
    """The descriptor arrays of one batched call over `layout` with the slabs at in_base / out_base."""

    def __init__(self, route, layout, in_base, out_base):
        r, L, n = route, layout, layout.n
        self.route, self.n = r, n
        w, h = r.size
        ow, oh = r.out_size
        i_ptr = lambda name, i: in_base + L.in_off[name][i]
        o_ptr = lambda name, i: out_base + L.out_off[name][i]
        transfer = {GAMMA_APPLE: TRANSFER_709, GAMMA_SRGB: TRANSFER_SRGB, GAMMA_LINEAR: TRANSFER_LINEAR}[r.gamma]
        if r.entry in ("decode", "half", "scaled"):
            y, c = r.plane("y"), r.plane("cbcr")
            self.frames = (Frame * n)(*[Frame(i_ptr("y", i), y.stride, i_ptr("cbcr", i), c.stride, w, h, MATRIX_709, transfer) for i in range(n)])
            self.alphas = None
            if r.alpha:
                a = r.plane("alpha")
                self.alphas = (Frame * n)(*[Frame(i_ptr("alpha", i), a.stride, None, a.stride, w, h, MATRIX_709, TRANSFER_LINEAR) for i in range(n)])
            self.surfs = (Surface * n)(*[Surface(o_ptr("out", i), r.plane("out").stride, ow, oh, r.fmt, 0) for i in range(n)])
        elif r.entry == "render":
            self.ins = (Surface * n)(*[Surface(i_ptr("in", i), r.plane("in").stride, w, h, r.in_fmt, 0) for i in range(n)])
            self.surfs = (Surface * n)(*[Surface(o_ptr("out", i), r.plane("out").stride, ow, oh, SRGB8, 0) for i in range(n)])
        elif r.entry == "unconvert":
            self.ptrs = (C.c_void_p * n)(*[i_ptr("in", i) for i in range(n)])
            self.surfs = (Surface * n)(*[Surface(o_ptr("out", i), r.plane("out").stride, w, h, SRGB8, 0) for i in range(n)])
        else:
            src = r.ins[0]  # "bgra", "rgba16f", or the "chw" tensor: plane 0 and the pitch of every plane's rows
            self.ins = (Surface * n)(*[Surface(i_ptr(src.name, i), src.stride, w, h, r.in_fmt, 0) for i in range(n)])

            def frame(y, c, i):  # a plane the route does not have: NULL, pitch 0 (the packed words: no "cbcr"; an alpha frame without chroma)
                has = any(p.name == c for p in r.outs)
                return Frame(o_ptr(y, i), r.plane(y).stride, o_ptr(c, i) if has else None, r.plane(c).stride if has else 0, w, h, 0, 0)
            frames = [frame("y", "cbcr", i) for i in range(n)]
            if r.paired:  # 2n frames: the colour frames, then the alpha frames
                frames += [frame("alpha_y", "alpha_cbcr", i) for i in range(n)]
            self.frames = (Frame * len(frames))(*frames)

    def _under_ctx_options(self, lib, ctx, call):
        """The route's context options for this call alone: the context is shared, so they are put back whatever happens."""
        try:
            for opt, val in self.route.ctx_options:
                rc = lib.bt709hip_context_set_option(ctx, opt, val)
                assert rc == 0, (self.route.name, opt, val, rc)
            return call()
        finally:
            for opt, _ in self.route.ctx_options:
                assert lib.bt709hip_context_set_option(ctx, opt, CTX_DEFAULTS[opt]) == 0, (self.route.name, opt)

    def batch(self, lib, ctx, dec, stream=None, wait=1, count=None):
        if self.route.ctx_options:
            return self._under_ctx_options(lib, ctx, lambda: self._batch(lib, ctx, dec, stream, wait, count))
        return self._batch(lib, ctx, dec, stream, wait, count)

    def single(self, lib, ctx, dec, i, stream=None, wait=1):
        if self.route.ctx_options:
            return self._under_ctx_options(lib, ctx, lambda: self._single(lib, ctx, dec, i, stream, wait))
        return self._single(lib, ctx, dec, i, stream, wait)

    def _batch(self, lib, ctx, dec, stream=None, wait=1, count=None):
        r, n = self.route, self.n if count is None else count
        if r.entry == "decode":
            return lib.bt709hip_decode_batch(dec, n, self.frames, self.alphas, self.surfs, stream, wait)
        if r.entry == "half":
            return lib.bt709hip_decode_half_batch(dec, n, self.frames, self.alphas, self.surfs, stream, wait)
        if r.entry == "scaled":
            return lib.bt709hip_decode_scaled_batch(dec, n, self.frames, self.alphas, self.surfs, stream, wait)
        if r.entry == "render":
            return lib.bt709hip_render_scaled_batch(ctx, n, self.ins, self.surfs, stream, wait)
        if r.entry == "unconvert":
            return lib.bt709hip_unconvert_batch(dec, n, self.ptrs, r.plane("in").stride, r.size[0], r.size[1], self.surfs, stream, wait)
        return lib.bt709hip_encode_batch(ctx, n, self.ins, self._pairs(range(n)) if r.paired and n != self.n else self.frames, r.pair[0], r.pair[1], stream, wait)

    def _pairs(self, items):
        """The frames of a paired call over `items` of the layout: their colour frames, then their alpha frames."""
        items = list(items)
        return (Frame * (2 * len(items)))(*[self.frames[i] for i in items] + [self.frames[self.n + i] for i in items])

    def _single(self, lib, ctx, dec, i, stream=None, wait=1):
        r = self.route
        if r.entry in ("decode", "half", "scaled"):
            f, a, s = C.byref(self.frames[i]), C.byref(self.alphas[i]) if self.alphas is not None else None, C.byref(self.surfs[i])
            if r.entry == "decode":
                return lib.bt709hip_decode(dec, f, a, s, r.size[0], r.size[1], stream, wait)
            return (lib.bt709hip_decode_half if r.entry == "half" else lib.bt709hip_decode_scaled)(dec, f, a, s, stream, wait)
        if r.entry == "render":
            return lib.bt709hip_render_scaled(ctx, C.byref(self.ins[i]), C.byref(self.surfs[i]), stream, wait)
        if r.entry == "unconvert":
            return lib.bt709hip_unconvert(dec, self.ptrs[i], r.plane("in").stride, r.size[0], r.size[1], C.byref(self.surfs[i]), stream, wait)
        out = self._pairs([i]) if r.paired else C.byref(self.frames[i])  # a paired call: `out` points to the pair's two frames
        return lib.bt709hip_encode(ctx, C.byref(self.ins[i]), out, r.pair[0], r.pair[1], stream, wait)

    def expected_steps(self, layout):
        """What the launch's step fields must hold, in the order the fake runtime reports them (fake_hip.h fake_hip_addressing):
        six values; the last but one pair are the alpha frames' of a paired encode, where the kernels read them."""
        r, s = self.route, layout.steps
        if r.entry in ("decode", "half", "scaled"):
            return [s["y"], s["cbcr"], s["alpha"] if r.alpha else 0, s["out"], 0, 0]
        if r.entry in ("render", "unconvert"):
            return [s["in"], s["out"], 0, 0, 0, 0]
        return [s[r.ins[0].name], s["y"], s.get("cbcr", 0), s["alpha_y"] if r.paired else 0, s.get("alpha_cbcr", 0), 0]


# ------------------------------------------------------------------ samples, backgrounds and what they must become
# (shared by tests/test_batch_spacing_gpu.py and tests/test_row_pitch_gpu.py, which lays the same routes out at other pitches:
# a route is looked up by NAME, so both modules draw the same samples and compute each reference once)

_data, _want = {}, {}


def _route_seed(route):
    names = [r.name for r in ROUTES]
    return names.index(route.name) if route.name in names else 500 + zlib.crc32(route.name.encode()) % 400


def frame_data(route, k):
    """plane name -> (rows, row_bytes) bytes of frame k: random, another for every frame and route."""
    key = (route.key, k)
    if key not in _data:
        rng = np.random.default_rng(100000 + 1000 * _route_seed(route) + k)
        w, h = route.size
        d = {}
        for p in route.ins:
            if route.entry == "render" and route.in_fmt == F16:  # finite halves, some above 1.0
                d[p.name] = (rng.random((h, w, 4)) * 1.25).astype(np.float16).view(np.uint8).reshape(h, 8 * w)
            elif route.entry == "unconvert":  # Y | Cb << 8 | Cr << 16
                d[p.name] = rng.integers(0, 1 << 24, (h, w), dtype=np.uint32).view(np.uint8).reshape(h, 4 * w)
            elif p.name == "chw" and route.chw != "uint8":  # finite elements; de-normalised (ImageNet's std and mean) they span -0.2 .. 1.2
                d[p.name] = (rng.random((3 * h, w)) * 6.0 - 3.0).astype(route.chw).view(np.uint8).reshape(3 * h, route.elem * w)
            elif p.name == "rgba16f":  # the half encoder's own texels: -0.25 .. 1.25, zeros, subnormals, infinities and NaNs among them
                d[p.name] = ehc.random_texels(rng, h, w).view(np.uint8).reshape(h, 8 * w)
            else:  # BGRA8 words: A is random, too (the premultiplying and the paired kernels read it)
                d[p.name] = rng.integers(0, 256, (p.rows, p.row_bytes), dtype=np.uint8)
        _data[key] = d
    return _data[key]


def background(route, i):
    ow, oh = route.out_size
    return np.random.default_rng(7000 + i).integers(0, 256, (oh, 4 * ow), dtype=np.uint8)


def interleave(uv_planes):
    """The NV12 twin of an I420 "cbcr" plane (U's rows, then V's)."""
    half = uv_planes.shape[0] // 2
    c = np.empty((half, 2 * uv_planes.shape[1]), np.uint8)
    c[:, 0::2], c[:, 1::2] = uv_planes[:half], uv_planes[half:]
    return c


_expects = {}


def _half_expect(oracle):
    """encode_half_cases.Expect(oracle), one for all routes: it remembers the oracle's answers."""
    if id(oracle) not in _expects:
        _expects[id(oracle)] = (oracle, ehc.Expect(oracle))
    return _expects[id(oracle)][1]


def _frames_of(route, colour, alpha):
    """(y, cbcr) NV12 of an encoder route's colour frame (and of its alpha frame) -> the route's planes: an I420 route's chroma
    planes are encode_chw_cases.planar of the NV12 rows, a plane the route does not have is left out."""
    w, h = route.size
    chroma = lambda c: ecc.planar(c).reshape(h, w // 2) if route.planar_chroma else c
    res = {"y": colour[0], "cbcr": chroma(colour[1])}
    if alpha is not None:
        res["alpha_y"] = alpha[0]
        if any(p.name == "alpha_cbcr" for p in route.outs):
            res["alpha_cbcr"] = chroma(alpha[1])
    return res


def want(route, oracle, tabs, T, k, bg_index):
    """plane name -> (rows, row_bytes) bytes frame k's samples must become (over the background of target bg_index, where the
    route reads its destination): the oracle call the route's own tests use.  tabs: over_cases.tables(oracle); T: the alpha
    luma table (tests/golden/alpha_luma.json)."""
    key = (route.key, k, bg_index if route.reads_destination else None)
    if key in _want:
        return _want[key]
    d = frame_data(route, k)
    w, h = route.size
    ow, oh = route.out_size
    g = route.gamma
    if route.entry in ("decode", "half", "scaled"):
        y, a = d["y"], d.get("alpha")
        c = interleave(d["cbcr"]) if route.planar_chroma else d["cbcr"]
        if route.entry == "decode":
            out = oracle.decode_nv12_rgba16f(g, y, c, a).view(np.uint8).reshape(h, 8 * w) if route.fmt == F16 else oracle.decode_nv12(g, y, c, alpha=a)
        elif route.entry == "half":
            out = oracle.decode_nv12_half(g, y, c, alpha=a)
        elif dict(route.options).get(_capi.OPT_SCALE_INTERMEDIATE) == F16:
            out = oracle.render_scaled(oracle.decode_nv12_rgba16f(g, y, c, a), ow, oh)
        else:
            out = oracle.decode_nv12_scaled(g, y, c, ow, oh, alpha=a)
        assert out is not None
        if route.reads_destination:
            import over_cases as oc
            out = oc.composite_over(out.reshape(oh, ow, 4), background(route, bg_index).reshape(oh, ow, 4), *tabs).reshape(oh, 4 * ow)
        if route.chw:  # the definition (chw_cases.chw_of) over the 8-bit words: planes R, G, B (A), stacked
            out = cc.chw_of(cc.words_of(out), route.chw, *(route.norm or ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))), planes=route.chw_planes).view(np.uint8)
        res = {"out": out}
    elif route.entry == "render":
        src = d["in"].view(np.float16).reshape(h, w, 4) if route.in_fmt == F16 else d["in"]
        res = {"out": oracle.render_scaled(src, ow, oh)}
    elif route.entry == "unconvert":
        res = {"out": oracle.unconvert_packed(g, d["in"].view(np.uint32).reshape(h, w), w, h).view(np.uint8).reshape(h, 4 * w)}
    elif route.entry == "interleave":  # numpy's interleave
        c = np.empty((d["u"].shape[0], 2 * d["u"].shape[1]), np.uint8)
        c[:, 0::2], c[:, 1::2] = d["u"], d["v"]
        res = {"cbcr": c}
    elif route.entry == "deinterleave":
        res = {"u": d["cbcr"][:, 0::2], "v": d["cbcr"][:, 1::2]}
    elif route.in_fmt == ALPHA8:
        res = {"y": T[d["bgra"].reshape(h, w, 4)[:, :, 3]]}
    elif route.chw:  # the BGRA8 picture the tensor stands for (encode_chw_cases.words_of_planes), encoded by the oracle
        tensor = np.ascontiguousarray(d["chw"]).view(route.chw).reshape(3, h, w)
        y, c = oracle.encode_nv12(ecc.words_of_planes(tensor, route.norm) & np.uint32(0xFFFFFF), w, h, route.pair[0], route.pair[1])
        res = {"y": y, "cbcr": ecc.planar(c).reshape(h, w // 2) if route.planar_chroma else c}
    elif route.in_fmt == F16:  # RGBA16Float input: the composition of encode_half_cases; the pair's alpha frame is encode_half_alpha_cases'
        texels = np.ascontiguousarray(d["rgba16f"]).view(np.uint16).reshape(h, w, 4)
        expect = _half_expect(oracle)
        res = _frames_of(route, expect.planes(texels, route.pair[1]), ehac.alpha_planes(expect, texels) if route.paired else None)
    else:
        words = np.ascontiguousarray(d["bgra"]).view(np.uint32).reshape(h, w)
        colour = sac.premultiply(words) if dict(route.ctx_options).get(_capi.CTX_OPT_ENCODE_PREMULTIPLY) else words
        if route.convert != _capi.CONVERT_OFF:  # +convert: of the picture; POINT420: copyBT709ToCoreVideo of those words
            packed = oracle.convert_packed(route.pair[1], colour, w, h)
            assert packed is not None
            if route.convert == _capi.CONVERT_PACKED444:
                res = {"y": packed.astype(np.uint32).view(np.uint8).reshape(h, 4 * w)}
            else:
                res = _frames_of(route, oracle.packed_to_nv12(packed, w, h), None)
        else:  # the pair's alpha frame reads A as stored, premultiplying or not: Y = T[A], every chroma byte 128
            alpha = (T[(words >> 24).astype(np.uint8)], np.full((h // 2, w), 128, np.uint8)) if route.paired else None
            res = _frames_of(route, oracle.encode_nv12(colour, w, h, route.pair[0], route.pair[1]), alpha)
    for name, arr in res.items():
        p = route.plane(name)
        res[name] = np.ascontiguousarray(arr).reshape(p.rows, p.row_bytes)
    _want[key] = res
    return res


# ------------------------------------------------------------------ the slabs' windows (rig: variant_cases.Rig; a window may hold
# whole planes -- the layouts above -- or single rows: tests/row_pitch_cases.py)

def _rows_in(planes, off, n, lo, hi):
    """(plane, frame, row, offset in the window) of every row of samples that lies in window lo..hi."""
    for p in planes:
        for i in range(n):
            first = off[p.name][i]
            if first + p.extent <= lo or first >= hi:
                continue
            for r in range(p.rows):
                a = first + r * p.stride
                if lo <= a and a + p.row_bytes <= hi:
                    yield p, i, r, a - lo


def upload_inputs(rig, d_in, L, fill):
    """Every input window: `fill` in every byte that is no sample (row padding, guard bands, the alias windows)."""
    for lo, hi in L.in_windows:
        host = np.full(hi - lo, fill, np.uint8)
        for p, i, r, at in _rows_in(L.route.ins, L.in_off, L.n, lo, hi):
            host[at:at + p.row_bytes] = frame_data(L.route, L.source[i])[p.name][r]
        rig.upload(d_in + lo, host)


def reset_outputs(rig, d_out, L):
    """Every output window: the canary, and where the route reads its destination background i in the pixels of target i.
    -> the windows' bytes as uploaded."""
    before = []
    for lo, hi in L.out_windows:
        host = np.full(hi - lo, CANARY, np.uint8)
        if L.route.reads_destination:
            for p, i, r, at in _rows_in(L.route.outs, L.out_off, L.n, lo, hi):
                host[at:at + p.row_bytes] = background(L.route, i)[r]
        rig.upload(d_out + lo, host)
        before.append(host)
    return before


def collect(rig, d_out, L, before, label):
    """-> {(plane name, frame): (rows, row_bytes)} of every output window; every byte outside the pixels must be what it was."""
    got = {(p.name, i): np.empty((p.rows, p.row_bytes), np.uint8) for p in L.route.outs for i in range(L.n)}
    seen = 0
    for (lo, hi), was in zip(L.out_windows, before):
        raw = rig.download(d_out + lo, hi - lo)
        outside = np.ones(raw.size, bool)
        for p, i, r, at in _rows_in(L.route.outs, L.out_off, L.n, lo, hi):
            got[(p.name, i)][r] = raw[at:at + p.row_bytes]
            outside[at:at + p.row_bytes] = False
            seen += 1
        stray = np.flatnonzero(outside & (raw != was))
        assert stray.size == 0, "%s: %d bytes written outside the pixels, first at slab offset %d (window %d..%d%s)" % (
            label, stray.size, lo + stray[0], lo, hi, ", an alias window" if (lo, hi) in L.out_alias else "")
    assert seen == L.n * sum(p.rows for p in L.route.outs)  # every row of every frame lay in exactly one window
    return got


def assert_plane(got, wanted, label):
    if not np.array_equal(got, wanted):
        bad = np.argwhere(got != wanted)
        r, x = bad[0]
        raise AssertionError("%s: differs first at row %d, byte %d (got %d, want %d); %d of %d bytes differ"
                             % (label, r, x, got[r, x], wanted[r, x], len(bad), got.size))


def scaled_record(lib):
    info = _capi.ScaledLaunchInfo()
    _capi.check(lib.bt709hip_last_scaled_launch_info(C.byref(info)))
    return info.taps, info.persistent
