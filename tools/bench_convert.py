#!/usr/bin/env python3
"""The per-pixel converter (BT709HIP_CTX_OPT_ENCODE_CONVERT) against its yardsticks, in ONE process on the SAME slabs
(placement cancels): 3840x2160 pictures resident in HBM, 1, 8 and 32 per launch;
  * PACKED444 (BGRA -> words, 8 B per pixel) against bt709hip_unconvert_batch on the same two slabs (words -> BGRA, the same 8 B per
    pixel; its code is not this change's) and against bt709hip_copy_probe over the same bytes (the streaming-copy ceiling);
  * POINT420 (BGRA -> NV12, 5.5 B per pixel) against the plain NV12 encode on the same slabs.
Not the headline bench (that is bench.py).  The legs of a group ALTERNATE: `--rounds` times a, b, c, a, b, c ...; a sample is one
region of >= 100 ms between two HIP events on the launch stream, after untimed steps; a figure is the median of its leg's samples,
and a yardstick leg's max / min over its samples is the spread a ratio has to be read against.  No target: the ratios say which leg
bounds the converter.

    python tools/bench_convert.py [--rounds 5] [--counts 1,8,32]

Prints one JSON line.
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

SRGB, APPLE = mb.MetalBT709GammaSRGB, mb.MetalBT709GammaApple


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--counts", default="1,8,32", help="pictures per launch")
    ap.add_argument("--rounds", type=int, default=5, help="samples per leg; the legs of a group alternate")
    args = ap.parse_args()
    W, H = args.width, args.height
    counts = [int(c) for c in args.counts.split(",")]
    ring = max(counts)
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal()
    lib, h = ctx.lib, ctx.handle

    # a slab of BGRA pictures, a slab of words and a slab of NV12 frames; random bytes: content does not change the kernels' work
    px = W * H
    slab_bgra, slab_words, slab_nv12 = (DeviceBuffer(ctx, ring * nb, 1) for nb in (4 * px, 4 * px, px * 3 // 2))
    rng = np.random.default_rng(0x444)
    host = rng.integers(0, 256, 4 * px, dtype=np.uint8)
    for slab in (slab_bgra, slab_words):
        _capi.check(lib.bt709hip_upload(h, slab.ptr, 4 * px, host.ctypes.data, 4 * px, 4 * px, 1, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for i in range(1, ring):
            _capi.check(lib.bt709hip_copy_probe(h, slab.ptr + i * 4 * px, slab.ptr, 4 * px, None))
    _capi.check(lib.bt709hip_stream_synchronize(h, None))
    surfs = (_capi.Surface * ring)(*[_capi.Surface(slab_bgra.ptr + i * 4 * px, 4 * W, W, H, _capi.FORMAT_BGRA8_SRGB, 0) for i in range(ring)])
    words = (_capi.Frame * ring)(*[_capi.Frame(slab_words.ptr + i * 4 * px, 4 * W, None, 0, W, H, 0, 0) for i in range(ring)])
    word_ptrs = (C.c_void_p * ring)(*[slab_words.ptr + i * 4 * px for i in range(ring)])
    nv12 = (_capi.Frame * ring)(*[_capi.Frame(slab_nv12.ptr + i * (px * 3 // 2), W, slab_nv12.ptr + i * (px * 3 // 2) + px, W, W, H, 0, 0) for i in range(ring)])

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

    def calibrate(step):
        for _ in range(3):
            step()
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        reps = max(2, int(np.ceil(130.0 / max(region(step, 4) / 4, 1e-3))))
        while region(step, reps) < 100.0:  # every region long enough for the event timer
            reps *= 2
        return reps

    dec = C.c_void_p()
    _capi.check(lib.bt709hip_decoder_create(h, APPLE, 0, C.byref(dec)))
    _capi.check(lib.bt709hip_decoder_setup(dec))
    _capi.check(lib.bt709hip_encoder_prepare(h, SRGB, APPLE))

    def set_mode(mode):
        _capi.check(lib.bt709hip_context_set_option(h, _capi.CTX_OPT_ENCODE_CONVERT, mode))

    # one picture per launch walks the ring, so that no leg finds its picture in the cache its own last launch left it in
    state = {"i": 0}
    f_size, s_size, p_size = C.sizeof(_capi.Frame), C.sizeof(_capi.Surface), C.sizeof(C.c_void_p)

    def advance(count):
        state["i"] = (state["i"] + 1) % ring if count == 1 else 0
        return state["i"]

    def at(array, size, kind):
        return C.cast(C.byref(array, state["i"] * size), C.POINTER(kind))

    def convert(count, mode, frames):
        def step():
            advance(count)
            set_mode(mode)
            _capi.check(lib.bt709hip_encode_batch(h, count, at(surfs, s_size, _capi.Surface), at(frames, f_size, _capi.Frame), SRGB, APPLE, None, 0))
            set_mode(_capi.CONVERT_OFF)
        return step

    def unconvert(count):
        def step():
            advance(count)
            _capi.check(lib.bt709hip_unconvert_batch(dec, count, at(word_ptrs, p_size, C.c_void_p), 4 * W, W, H, at(surfs, s_size, _capi.Surface), None, 0))
        return step

    def copy(count):
        def step():
            i = advance(count)
            _capi.check(lib.bt709hip_copy_probe(h, slab_words.ptr + i * 4 * px, slab_bgra.ptr + i * 4 * px, count * 4 * px, None))
        return step

    legs, ratios = {}, {}
    for count in counts:
        groups = (("packed444", 8.0, (("convert_packed444", convert(count, _capi.CONVERT_PACKED444, words)), ("unconvert", unconvert(count)), ("copy_probe", copy(count)))),
                  ("point420", 5.5, (("convert_point420", convert(count, _capi.CONVERT_POINT420, nv12)), ("encode_nv12", convert(count, _capi.CONVERT_OFF, nv12)))))
        for group, bpp, members in groups:
            reps = {name: calibrate(step) for name, step in members}
            samples, kernels = {name: [] for name, _ in members}, {}
            for _ in range(args.rounds):  # alternating legs
                for name, step in members:
                    step()
                    samples[name].append(region(step, reps[name]))
                    kernels[name] = lib.bt709hip_last_kernel_name().decode()
            for name, _ in members:
                s = sorted(samples[name])
                us = s[len(s) // 2] * 1e3 / (reps[name] * count)
                legs["%s/%d_per_launch" % (name, count)] = {
                    "us_per_picture": round(us, 3), "gpixel_per_s": round(px / us / 1e3, 1), "algorithmic_bytes": int(px * bpp),
                    "frac_of_8TBps": round(px * bpp / us / 1e3 / 8000, 4), "kernel": kernels[name], "region_ms": [round(v, 1) for v in samples[name]],
                    "spread_max_over_min": round(s[-1] / s[0], 4), "reps": reps[name]}
            new = members[0][0]
            for name, _ in members[1:]:
                ratios["%s over %s, time, %d_per_launch" % (new, name, count)] = round(
                    legs["%s/%d_per_launch" % (new, count)]["us_per_picture"] / legs["%s/%d_per_launch" % (name, count)]["us_per_picture"], 4)
    lib.bt709hip_decoder_destroy(dec)
    print(json.dumps({"workload": "%dx%d, %d resident: BGRA8 -> packed 4:4:4 words / point-sampled NV12 (sRGB in, Apple out) against unconvert, "
                                  "copy_probe and the NV12 encode; same slabs, random content, alternating legs" % (W, H, ring), "legs": legs, "ratios": ratios}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
