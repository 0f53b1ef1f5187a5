#!/usr/bin/env python3
"""The blended rescale (BT709HIP_OPT_SCALED_OVER) against the plain fused rescale it extends, in ONE process on the
SAME slabs (placement cancels): an alpha decoder, frames resident in HBM, 3840x2160 -> 2560x1440 and 1920x1080 ->
3840x2160, 8 frames per launch and one frame per launch, at three settings -- option off (the parent's launch), over a solid
colour, over the destination -- plus bt709hip_copy_probe over a buffer of the output's size: option-off time + that copy is
roughly what a caller's separate blend pass would cost at best (it reads the view and writes it again), the yardstick a blended
launch is held against.  Not the headline bench (that is bench.py).  Method as tools/bench_over.py: three untimed steps, then
each figure is the median of 5 regions of >= 100 ms between two HIP events on the launch stream.

    python tools/bench_scaled_over.py [--ring 8] [--intermediate 0|1] [--library <another build>]

A library that predates the option runs the option-off legs and the copy alone.  Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import metalbt709decoder_amd as mb  # noqa: E402
from metalbt709decoder_amd import _capi  # noqa: E402

OPT_SCALE_INTERMEDIATE, OPT_SCALED_OVER, OVER_OFF, OVER_DESTINATION = 8, 10, -1, -2  # spelled out: --library may load a build whose _capi twin predates the option
SHAPES = [("4k_to_1440p", (3840, 2160), (2560, 1440)), ("1080p_to_4k", (1920, 1080), (3840, 2160))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=8, help="frames resident in HBM = frames of the batched launch (<= 32)")
    ap.add_argument("--colour", type=lambda v: int(v, 0), default=0xFFFFFF, help="the solid background, R<<16 | G<<8 | B")
    ap.add_argument("--intermediate", type=int, default=0, help="BT709HIP_OPT_SCALE_INTERMEDIATE: 0 = BGRA8_SRGB, 1 = RGBA16F")
    ap.add_argument("--library", default=None, help="a variant build of libbt709hip.so")
    args = ap.parse_args()
    ring = args.ring
    if args.library:
        _capi.load(os.path.abspath(args.library))
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal()
    lib, h = ctx.lib, ctx.handle

    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.bt709hip_event_create(h, C.byref(e0))
    lib.bt709hip_event_create(h, C.byref(e1))

    def region(step, reps):
        lib.bt709hip_event_record(h, e0, None)
        for _ in range(reps):
            step()
        lib.bt709hip_event_record(h, e1, None)
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        ms = C.c_float()
        lib.bt709hip_event_elapsed_ms(h, e0, e1, C.byref(ms))
        return ms.value

    def measure(step, frames_per_step):
        for _ in range(3):
            step()
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        reps = max(2, int(np.ceil(130.0 / max(region(step, 4) / 4, 1e-3))))
        while True:
            samples = sorted(region(step, reps) for _ in range(5))
            if samples[0] >= 100.0:  # every region is long enough for the event timer
                break
            reps *= 2
        return samples[2] * 1e3 / (reps * frames_per_step), samples, reps  # us per frame (median)

    dec = C.c_void_p()
    _capi.check(lib.bt709hip_decoder_create(h, mb.MetalBT709GammaSRGB, 1, C.byref(dec)))
    _capi.check(lib.bt709hip_decoder_set_option(dec, OPT_SCALE_INTERMEDIATE, args.intermediate))
    _capi.check(lib.bt709hip_decoder_setup(dec))
    f_size, s_size = C.sizeof(_capi.Frame), C.sizeof(_capi.Surface)
    result = {"workload": "NV12 + alpha frame -> BGRA8 view, fused rescale: option off / over the colour %06x / over the destination, same slabs, "
                          "random content, intermediate %d" % (args.colour, args.intermediate), "shapes": {}}
    rng = np.random.default_rng(0x5CA1)
    for shape, (W, H), (OW, OH) in SHAPES:
        # one input slot = Y, CbCr and the alpha frame's Y plane; random bytes (content does not change the kernels' work)
        in_pitch, out_pitch = W * H * 5 // 2, OW * OH * 4
        slab_in, slab_out, spare = DeviceBuffer(ctx, ring * in_pitch, 1), DeviceBuffer(ctx, ring * out_pitch, 1), DeviceBuffer(ctx, out_pitch, 1)
        distinct = min(ring, 4)  # random frames from the host; the rest of the ring are device-side copies of them
        for i in range(distinct):
            host = rng.integers(0, 256, in_pitch, dtype=np.uint8)
            _capi.check(lib.bt709hip_upload(h, slab_in.ptr + i * in_pitch, in_pitch, host.ctypes.data, in_pitch, in_pitch, 1, None))
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for i in range(distinct, ring, distinct):
            _capi.check(lib.bt709hip_copy_probe(h, slab_in.ptr + i * in_pitch, slab_in.ptr, min(distinct, ring - i) * in_pitch, None))
        _capi.check(lib.bt709hip_memset(h, slab_out.ptr, 0x80, ring * out_pitch, None))  # the canvas destination mode blends over
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        frames = (_capi.Frame * ring)(*[_capi.Frame(slab_in.ptr + i * in_pitch, W, slab_in.ptr + i * in_pitch + W * H, W, W, H, 1, 2) for i in range(ring)])
        alphas = (_capi.Frame * ring)(*[_capi.Frame(slab_in.ptr + i * in_pitch + W * H * 3 // 2, W, slab_in.ptr + i * in_pitch + W * H, W, W, H, 1, 3)
                                        for i in range(ring)])
        surfs = (_capi.Surface * ring)(*[_capi.Surface(slab_out.ptr + i * out_pitch, OW * 4, OW, OH, _capi.FORMAT_BGRA8_SRGB, 0) for i in range(ring)])

        legs = {}
        for name, value in (("off", OVER_OFF), ("over_colour", args.colour), ("over_destination", OVER_DESTINATION)):
            if lib.bt709hip_decoder_set_option(dec, OPT_SCALED_OVER, value) != _capi.OK:
                continue  # a build that predates the option
            _capi.check(lib.bt709hip_decoder_setup(dec))  # builds the option's table

            def batch():
                _capi.check(lib.bt709hip_decode_scaled_batch(dec, ring, frames, alphas, surfs, None, 0))

            state = {"i": 0}

            def single():
                i = state["i"] = (state["i"] + 1) % ring
                _capi.check(lib.bt709hip_decode_scaled_batch(dec, 1, C.cast(C.byref(frames, i * f_size), C.POINTER(_capi.Frame)),
                                                             C.cast(C.byref(alphas, i * f_size), C.POINTER(_capi.Frame)),
                                                             C.cast(C.byref(surfs, i * s_size), C.POINTER(_capi.Surface)), None, 0))

            for leg, step, per in (("%d_per_launch" % ring, batch, ring), ("1_per_launch", single, 1)):
                us, samples, reps = measure(step, per)
                legs["%s/%s" % (name, leg)] = {"us_per_frame": round(us, 3), "gpixel_per_s_out": round(OW * OH / us / 1e3, 1),
                                               "kernel": lib.bt709hip_last_kernel_name().decode(), "region_ms": [round(v, 1) for v in samples], "reps": reps}
        lib.bt709hip_decoder_set_option(dec, OPT_SCALED_OVER, OVER_OFF)

        # the copy a separate blend pass cannot beat: the view read once and written once (16 bytes per lane, non-temporal)
        state = {"i": 0}

        def copy_one():
            i = state["i"] = (state["i"] + 1) % ring
            _capi.check(lib.bt709hip_copy_probe(h, spare.ptr, slab_out.ptr + i * out_pitch, out_pitch, None))

        us, samples, reps = measure(copy_one, 1)
        legs["copy_of_the_view"] = {"us_per_frame": round(us, 3), "bytes": out_pitch, "tbyte_per_s_read_plus_written": round(2 * out_pitch / us / 1e6, 3),
                                    "region_ms": [round(v, 1) for v in samples], "reps": reps}
        summary = {"legs": legs}
        for leg in ("%d_per_launch" % ring, "1_per_launch"):
            yard = legs["off/" + leg]["us_per_frame"] + legs["copy_of_the_view"]["us_per_frame"]
            summary["yardstick_us/" + leg] = round(yard, 3)
            for name in ("over_colour", "over_destination"):
                if "%s/%s" % (name, leg) in legs:
                    t = legs["%s/%s" % (name, leg)]["us_per_frame"]
                    summary["%s/%s over off" % (name, leg)] = round(t / legs["off/" + leg]["us_per_frame"], 4)
                    summary["%s/%s over yardstick" % (name, leg)] = round(t / yard, 4)
        result["shapes"][shape] = summary
        for b in (slab_in, slab_out, spare):
            b.free()
    lib.bt709hip_decoder_destroy(dec)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
