"""ctypes binding of the C ABI declared in include/bt709hip.h (the reference-twinned calls) and include/bt709hip_ext.h.

Loading never falls back to anything: if libbt709hip.so is missing and cannot be
built, importing the product raises.
"""
import ctypes as C
import os

from . import build as _build

c_void_pp = C.POINTER(C.c_void_p)


class Frame(C.Structure):  # bt709hip_frame
    _fields_ = [("y", C.c_void_p), ("y_stride", C.c_size_t),
                ("cbcr", C.c_void_p), ("cbcr_stride", C.c_size_t),
                ("width", C.c_int32), ("height", C.c_int32),
                ("matrix", C.c_int32), ("transfer", C.c_int32)]


class Surface(C.Structure):  # bt709hip_surface
    _fields_ = [("bgra", C.c_void_p), ("stride", C.c_size_t),
                ("width", C.c_int32), ("height", C.c_int32),
                ("format", C.c_int32), ("reserved", C.c_int32)]


ABI_VERSION = 504  # BT709HIP_VERSION of the two headers these bindings were written against

# bt709hip_format
FORMAT_BGRA8_SRGB = 0
FORMAT_RGBA16F = 1
FORMAT_BGRA8_ALPHA = 3  # input of bt709hip_encode[_batch] only: BGRA8 texels read as the grey picture (A,A,A); 2 is unassigned

# bt709hip_decoder_option / bt709hip_context_option
OPT_NONTEMPORAL = 1
OPT_HALF_KERNEL = 2
OPT_HALF_WORKGROUPS = 3
OPT_HALF_LDS_KB = 4
OPT_XCD_BANDS = 5
OPT_COALESCE = 6
OPT_COALESCE_MAX_AGE_US = 7
OPT_SCALE_INTERMEDIATE = 8  # value: FORMAT_BGRA8_SRGB (default) or FORMAT_RGBA16F
OPT_COMPOSITE_OVER = 9  # alpha decoders: OVER_OFF (default), OVER_DESTINATION, or an sRGB colour R<<16 | G<<8 | B
OPT_SCALED_OVER = 10  # alpha decoders, the rescale paths (decode_scaled / decode_half): the same three forms, held separately
OVER_OFF = -1
OVER_DESTINATION = -2
OPT_CHROMA_LAYOUT = 11  # how the 1:1 decode reads the caller's colour frames: CHROMA_NV12 (default) or CHROMA_I420 (planar: U, then V)
CHROMA_NV12 = 0
CHROMA_I420 = 1
OPT_UNPREMULTIPLY = 12  # alpha decoders: 0 (default) the 1:1 decode writes premultiplied colour; 1: straight alpha
# planar CHW targets of bt709hip_decode[_batch] (bt709hip_ext.h, PLANAR CHW TARGETS)
FORMAT_CHW_U8 = 4
FORMAT_CHW_F16 = 5
FORMAT_CHW_F32 = 6
OPT_CHW_SCALE_R, OPT_CHW_SCALE_G, OPT_CHW_SCALE_B = 14, 15, 16  # value: the bit pattern of a float32; default 1.0f
OPT_CHW_BIAS_R, OPT_CHW_BIAS_G, OPT_CHW_BIAS_B = 17, 18, 19     # default 0.0f
OPT_SCALED_PLANAR = 24  # 0 (default) / 1: under OPT_CHROMA_LAYOUT = CHROMA_I420, decode_scaled / decode_half and their batches read planar frames in place; 23 is no option
OPT_SCALED_CHW = 22  # 0 (default) / 1: decode_scaled / decode_half and their batches take planar CHW targets of the view's size
CTX_OPT_GRID_MULT = 1
CTX_OPT_ENCODE_ROW_PAIRS = 2
CTX_OPT_ENCODE_THREADS = 3
CTX_OPT_XCD_BANDS = 4
CTX_OPT_STREAMING_TRIES = 5
CTX_OPT_ENCODE_CHROMA_LAYOUT = 6  # the planes bt709hip_encode[_batch] writes: CHROMA_NV12 (default) or CHROMA_I420; any other value is refused
CTX_OPT_ENCODE_PREMULTIPLY = 8  # 0 (default): BGRA8_SRGB input is encoded as it is; 1: it is straight alpha, premultiplied in the encode kernel; any other value is refused
CTX_OPT_ENCODE_CONVERT = 10  # CONVERT_OFF (default): bt709hip_encode[_batch] is the subsampling encoder; CONVERT_PACKED444 / CONVERT_POINT420: the reference's per-pixel +convert:; any other value is refused
CTX_OPT_ENCODE_WITH_ALPHA = 12  # 0 (default): one frame per picture; 1: bt709hip_encode[_batch] of BGRA8_SRGB input writes the alpha frame as well, `out` holds 2 x count frames (colour frames, then the alpha frames); any other value is refused
CTX_OPT_ENCODE_HALF_WITH_ALPHA = 16  # 0 (default): one frame per picture; 1: bt709hip_encode[_batch] of RGBA16F input (under CTX_OPT_ENCODE_HALF_INPUT = 1) writes the surface's alpha frame as well, `out` holds 2 x count frames (colour frames, then the alpha frames); any other value is refused
CTX_OPT_ENCODE_CHW_INPUT = 18  # 0 (default): planar CHW input to bt709hip_encode[_batch] is refused as any unknown format is; 1: FORMAT_CHW_U8 / _F16 / _F32 surfaces are encoded; any other value is refused
CTX_OPT_ENCODE_CHW_SCALE_R, CTX_OPT_ENCODE_CHW_SCALE_G, CTX_OPT_ENCODE_CHW_SCALE_B = 20, 21, 22  # float32 bit patterns (default 1.0): an element t of float CHW input becomes the byte round(255 * sat(t * scale + bias))
CTX_OPT_ENCODE_CHW_BIAS_R, CTX_OPT_ENCODE_CHW_BIAS_G, CTX_OPT_ENCODE_CHW_BIAS_B = 23, 24, 25     # float32 bit patterns (default 0.0); +-0 or finite with 2^-64 <= |x| <= 2^64, anything else is refused
CTX_OPT_ENCODE_HALF_INPUT = 14 # 0 (default): RGBA16F input to bt709hip_encode[_batch] is refused (ERR_UNSUPPORTED); 1: it is encoded as linear light (input gamma LINEAR); any other value is refused
CONVERT_OFF = 0
CONVERT_PACKED444 = 1  # out.y: W x H 32-bit words (Cr<<16)|(Cb<<8)|Y, out.cbcr NULL
CONVERT_POINT420 = 2   # +convert: then copyBT709ToCoreVideo in one launch: an NV12 / I420 frame, a block's chroma from its odd row, even column


class RingPlacement(C.Structure):  # bt709hip_ring_placement
    _fields_ = [("tries", C.c_int32), ("in_candidates", C.c_int32), ("out_candidates", C.c_int32),
                ("chosen_in", C.c_int32), ("chosen_out", C.c_int32), ("probes", C.c_int32),
                ("first_GBps", C.c_float), ("chosen_GBps", C.c_float), ("best_GBps", C.c_float), ("worst_GBps", C.c_float),
                ("out_prescan_GBps", C.c_float * 18), ("out_kept", C.c_int32 * 18),
                ("hunt_ms", C.c_float), ("stopped_by", C.c_int32), ("peak_bytes", C.c_uint64), ("budget_bytes", C.c_uint64),
                ("evicted", C.c_int32), ("reserved", C.c_int32)]


class RingOptions(C.Structure):  # bt709hip_ring_options
    _fields_ = [("max_bytes", C.c_uint64), ("max_ms", C.c_uint32), ("frugal", C.c_int32), ("format", C.c_int32), ("reserved", C.c_int32)]


class LaunchInfo(C.Structure):  # bt709hip_launch_info
    _fields_ = [("grid", C.c_uint32 * 3), ("block", C.c_uint32 * 3), ("launches", C.c_int32), ("xcd_bands", C.c_int32)]


class ScaledLaunchInfo(C.Structure):  # bt709hip_scaled_launch_info
    _fields_ = [("grid", C.c_uint32 * 3), ("block", C.c_uint32 * 3), ("taps", C.c_uint32), ("rows", C.c_uint32),
                ("persistent", C.c_uint32), ("balanced", C.c_uint32), ("resident", C.c_uint32), ("reserved", C.c_uint32),
                ("items", C.c_uint64)]


# bt709hip_scaled_launch_info.taps (BT709HIP_SCALED_TAPS_*)
SCALED_TAPS_BYTES, SCALED_TAPS_PAIRS, SCALED_TAPS_WIDE, SCALED_TAPS_SHARED, SCALED_TAPS_ONCE = range(5)


class DeviceInfo(C.Structure):  # bt709hip_device_info
    _fields_ = [("device_ordinal", C.c_int32), ("compute_units", C.c_int32),
                ("wavefront_size", C.c_int32), ("lds_bytes_per_block", C.c_int32),
                ("memory_clock_khz", C.c_int32), ("memory_bus_width_bits", C.c_int32),
                ("l2_bytes", C.c_int32), ("clock_khz", C.c_int32),
                ("total_memory_bytes", C.c_uint64),
                ("name", C.c_char * 128), ("arch", C.c_char * 64),
                ("pci_bus_id", C.c_char * 32), ("uuid", C.c_char * 40)]


# status codes (bt709hip_status)
OK = 0
ERR_INVALID_ARG = -1
ERR_NOT_SETUP = -2
ERR_SIZE_MISMATCH = -3
ERR_ODD_DIMENSIONS = -4
ERR_MATRIX = -5
ERR_TRANSFER = -6
ERR_ALPHA_TRANSFER = -7
ERR_STRIDE = -8
ERR_HIP = -9
ERR_NO_DEVICE = -10
ERR_UNSUPPORTED = -11

MAX_BATCH = 32

# every symbol the two headers declare: name -> (restype, argtypes)
_P, _I, _Z = C.c_void_p, C.c_int, C.c_size_t
_FP, _SP = C.POINTER(Frame), C.POINTER(Surface)
SYMBOLS = {
    "bt709hip_device_count": (_I, []),
    "bt709hip_abi_version": (_I, []),
    "bt709hip_context_set_option": (_I, [_P, _I, _I]),
    "bt709hip_context_create": (_I, [_I, c_void_pp]),
    "bt709hip_context_destroy": (_I, [_P]),
    "bt709hip_context_info": (_I, [_P, C.POINTER(DeviceInfo)]),
    "bt709hip_stream_create": (_I, [_P, c_void_pp]),
    "bt709hip_stream_create_with_priority": (_I, [_P, _I, c_void_pp]),
    "bt709hip_stream_destroy": (_I, [_P, _P]),
    "bt709hip_stream_synchronize": (_I, [_P, _P]),
    "bt709hip_event_create": (_I, [_P, c_void_pp]),
    "bt709hip_event_destroy": (_I, [_P, _P]),
    "bt709hip_event_record": (_I, [_P, _P, _P]),
    "bt709hip_event_synchronize": (_I, [_P, _P]),
    "bt709hip_stream_wait_event": (_I, [_P, _P, _P]),
    "bt709hip_event_elapsed_ms": (_I, [_P, _P, _P, C.POINTER(C.c_float)]),
    "bt709hip_pool_create": (_I, [_P, _I, _I, _I, C.POINTER(C.c_void_p)]),
    "bt709hip_pool_destroy": (_I, [_P]),
    "bt709hip_pool_acquire": (_I, [_P, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "bt709hip_pool_alpha_plane": (_I, [_P, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "bt709hip_pool_submit": (_I, [_P, _I]),
    "bt709hip_pool_wait": (_I, [_P, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "bt709hip_pool_release": (_I, [_P, _I]),
    "bt709hip_shard_create": (_I, [C.POINTER(C.c_int), _I, _I, _I, _I, _I, _I, C.POINTER(C.c_void_p)]),
    "bt709hip_shard_destroy": (_I, [_P]),
    "bt709hip_shard_lanes": (_I, [_P]),
    "bt709hip_shard_lane_device": (_I, [_P, _I]),
    "bt709hip_shard_lane_decoder": (_P, [_P, _I]),
    "bt709hip_shard_acquire": (_I, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_size_t)]),
    "bt709hip_shard_commit": (_I, [_P, C.c_uint64]),
    "bt709hip_shard_cancel": (_I, [_P]),
    "bt709hip_shard_submit": (_I, [_P, _FP, _FP, C.POINTER(C.c_uint64)]),
    "bt709hip_shard_wait": (_I, [_P, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "bt709hip_graph_begin_capture": (_I, [_P, _P]),
    "bt709hip_graph_end_capture": (_I, [_P, _P, C.POINTER(C.c_void_p)]),
    "bt709hip_graph_launch": (_I, [_P, _P, _P]),
    "bt709hip_graph_destroy": (_I, [_P, _P]),
    "bt709hip_mem_info": (_I, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "bt709hip_decoder_has_alpha": (_I, [_P]),
    "bt709hip_decoder_context": (_P, [_P]),
    "bt709hip_decoder_flush": (_I, [_P, _P]),
    "bt709hip_decoder_flush_all": (_I, [_P]),
    "bt709hip_ring_create": (_I, [_P, _I, _I, _I, _I, _I, c_void_pp]),
    "bt709hip_ring_create_ex": (_I, [_P, _I, _I, _I, _I, _I, C.POINTER(RingOptions), c_void_pp]),
    "bt709hip_ring_destroy": (_I, [_P]),
    "bt709hip_ringset_create": (_I, [C.POINTER(C.c_int), _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(RingOptions), c_void_pp]),
    "bt709hip_ringset_destroy": (_I, [_P]),
    "bt709hip_ringset_lanes": (_I, [_P]),
    "bt709hip_ringset_lane_context": (_P, [_P, _I]),
    "bt709hip_ringset_lane_decoder": (_P, [_P, _I]),
    "bt709hip_ringset_lane_ring": (_P, [_P, _I]),
    "bt709hip_ringset_decode": (_I, [_P, _I, _I, _I]),
    "bt709hip_ringset_synchronize": (_I, [_P]),
    "bt709hip_ring_frames": (_I, [_P]),
    "bt709hip_ring_frame": (_I, [_P, _I, _FP, _FP, _SP]),
    "bt709hip_ring_placement_info": (_I, [_P, C.POINTER(RingPlacement)]),
    "bt709hip_ring_decode": (_I, [_P, _I, _I, _P, _I]),
    "bt709hip_malloc": (_I, [_P, _Z, c_void_pp]),
    "bt709hip_free": (_I, [_P, _P]),
    "bt709hip_host_alloc": (_I, [_P, _Z, c_void_pp]),
    "bt709hip_host_free": (_I, [_P, _P]),
    "bt709hip_memset": (_I, [_P, _P, _I, _Z, _P]),
    "bt709hip_upload": (_I, [_P, _P, _Z, _P, _Z, _Z, _Z, _P]),
    "bt709hip_download": (_I, [_P, _P, _Z, _P, _Z, _Z, _Z, _P]),
    "bt709hip_decoder_create": (_I, [_P, _I, _I, c_void_pp]),
    "bt709hip_decoder_destroy": (_I, [_P]),
    "bt709hip_decoder_set_context": (_I, [_P, _P]),
    "bt709hip_decoder_set_alpha_fill": (_I, [_P, _I]),
    "bt709hip_decoder_get_gamma": (_I, [_P]),
    "bt709hip_decoder_set_option": (_I, [_P, _I, _I]),
    "bt709hip_decoder_get_option": (_I, [_P, _I, C.POINTER(C.c_int)]),
    "bt709hip_decoder_setup": (_I, [_P]),
    "bt709hip_decode": (_I, [_P, _FP, _FP, _SP, _I, _I, _P, _I]),
    "bt709hip_decode_batch": (_I, [_P, _I, _FP, _FP, _SP, _P, _I]),
    "bt709hip_unconvert": (_I, [_P, _P, _Z, _I, _I, _SP, _P, _I]),
    "bt709hip_unconvert_batch": (_I, [_P, _I, C.POINTER(C.c_void_p), _Z, _I, _I, _SP, _P, _I]),
    "bt709hip_decode_half": (_I, [_P, _FP, _FP, _SP, _P, _I]),
    "bt709hip_decode_half_batch": (_I, [_P, _I, _FP, _FP, _SP, _P, _I]),
    "bt709hip_decode_scaled": (_I, [_P, _FP, _FP, _SP, _P, _I]),
    "bt709hip_decode_scaled_batch": (_I, [_P, _I, _FP, _FP, _SP, _P, _I]),
    "bt709hip_render_scaled": (_I, [_P, _SP, _SP, _P, _I]),
    "bt709hip_render_scaled_batch": (_I, [_P, _I, _SP, _SP, _P, _I]),
    "bt709hip_render_scaled_prepare": (_I, [_P]),
    "bt709hip_decoder_prepare_format": (_I, [_P, _I]),
    "bt709hip_encoder_prepare": (_I, [_P, _I, _I]),
    "bt709hip_encode": (_I, [_P, _SP, _FP, _I, _I, _P, _I]),
    "bt709hip_encode_batch": (_I, [_P, _I, _SP, _FP, _I, _I, _P, _I]),
    "bt709hip_interleave_cbcr": (_I, [_P, _P, _Z, _P, _Z, _P, _Z, _I, _I, _P, _I]),
    "bt709hip_deinterleave_cbcr": (_I, [_P, _P, _Z, _P, _Z, _P, _Z, _I, _I, _P, _I]),
    "bt709hip_copy_probe": (_I, [_P, _P, _P, _Z, _P]),
    "bt709hip_malloc_streaming": (_I, [_P, _Z, _I, c_void_pp, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "bt709hip_strerror": (C.c_char_p, [_I]),
    "bt709hip_last_hip_error": (_I, []),
    "bt709hip_last_hip_error_string": (C.c_char_p, []),
    "bt709hip_gamma_thresholds": (_I, [_I, C.POINTER(C.c_float)]),
    "bt709hip_gamma_lookup": (_I, [_I, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bt709hip_gamma_lookup_decode": (_I, [_I, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bt709hip_matrix_constants": (_I, [C.POINTER(C.c_float)]),
    "bt709hip_half_thresholds": (_I, [_I, C.POINTER(C.c_float), _I]),
    "bt709hip_half_lookup": (_I, [_I, C.c_float, _I, C.POINTER(C.c_int)]),
    "bt709hip_last_kernel_name": (C.c_char_p, []),
    "bt709hip_last_launch_info": (_I, [C.POINTER(LaunchInfo)]),
    "bt709hip_last_scaled_launch_info": (_I, [C.POINTER(ScaledLaunchInfo)]),
}

_lib = None


def library_path():
    return _build.LIB


def load(path=None):
    """Return the loaded C-ABI library, building it in-tree first if it is stale.  Never runs a
    library older than its sources or of another ABI version: when the library is stale and no
    compiler is present, or the loaded library reports a BT709HIP_VERSION other than these
    bindings', this raises (no fallback of any kind).
    path: load THIS build of the library instead (A/B runs of tools/build_variant.py; must be the
    first load of the process); it is not rebuilt, only ABI-checked."""
    global _lib
    if _lib is not None:
        if path is not None and os.path.realpath(path) != os.path.realpath(_lib._name):
            raise RuntimeError("another build of the library is already loaded: %s" % _lib._name)
        return _lib
    if path is None and _build.is_stale():
        path = _build.LIB
        try:
            _build.build()  # a compile error propagates
        except OSError as exc:  # no hipcc on this machine
            raise ImportError("libbt709hip.so is %s and could not be (re)built: %s"
                              % ("stale" if os.path.exists(path) else "missing", exc))
    lib = C.CDLL(path or _build.LIB)
    path = path or _build.LIB
    try:
        lib.bt709hip_abi_version.restype = C.c_int
        have = lib.bt709hip_abi_version()
    except AttributeError:
        have = None
    if have != ABI_VERSION:
        raise ImportError("%s reports ABI version %s, these bindings need %d" % (path, have, ABI_VERSION))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def strerror(status):
    return load().bt709hip_strerror(int(status)).decode()


class Bt709Error(RuntimeError):
    def __init__(self, status, what=""):
        self.status = int(status)
        msg = "%s: %s" % (what, strerror(status)) if what else strerror(status)
        if self.status == ERR_HIP:
            msg += " (%s)" % load().bt709hip_last_hip_error_string().decode()
        super().__init__(msg)


def check(status, what=""):
    if status != OK:
        raise Bt709Error(status, what)
