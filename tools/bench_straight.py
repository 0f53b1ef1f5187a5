#!/usr/bin/env python3
"""Straight alpha in and out against the plain kernels it extends, in ONE process on the SAME slabs (placement
cancels): 3840x2160 pictures / alpha frames resident in HBM, 32 per launch and one per launch;
  * bt709hip_encode_batch, plain (the yardstick: 5.5 B per pixel) against BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY = 1 (the same traffic);
  * bt709hip_decode_batch of an alpha decoder, plain (6.5 B per pixel) against BT709HIP_OPT_UNPREMULTIPLY = 1 (the same traffic).
Not the headline bench (that is bench.py).  The two legs of a pair ALTERNATE: `--rounds` times plain, new, plain, new ...; a sample
is one region of >= 100 ms between two HIP events on the launch stream, after three untimed steps; a figure is the median of its
leg's samples, and the plain leg's max / min over its samples is the spread a ratio has to be read against.  The plain kernels'
code is the parent commit's, instruction for instruction (profiles/r15_straight_alpha_isa.txt): "time x plain" is time x the
parent's.

    python tools/bench_straight.py [--ring 32] [--rounds 5] [--batched-only] [--library <another build>]

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

CTX_OPT_ENCODE_PREMULTIPLY, OPT_UNPREMULTIPLY = 8, 12  # spelled out: --library may load a build whose _capi twin differs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=32, help="pictures / frames resident in HBM = items of the batched launch (<= 32)")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=5, help="samples per leg; the legs of a pair alternate")
    ap.add_argument("--batched-only", action="store_true", help="skip the one-per-launch legs (a counters pass under a profiler: fewer dispatches)")
    ap.add_argument("--library", default=None, help="a variant build of libbt709hip.so")
    args = ap.parse_args()
    W, H, ring = args.width, args.height, args.ring
    if args.library:
        _capi.load(os.path.abspath(args.library))
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal()
    lib, h = ctx.lib, ctx.handle

    # one slab of BGRA words (the encoder's input, the decoder's output) and one of planes: Y, CbCr and the alpha frame's Y plane
    # (the encoder writes the first two, the decoder reads all three); random bytes: content does not change the kernels' work
    plane_pitch, bgra_pitch = W * H * 5 // 2, W * H * 4
    slab_planes, slab_bgra = DeviceBuffer(ctx, ring * plane_pitch, 1), DeviceBuffer(ctx, ring * bgra_pitch, 1)
    rng = np.random.default_rng(0x39)
    distinct = min(ring, 4)  # random items from the host; the rest are device-side copies of them
    for slab, pitch in ((slab_planes, plane_pitch), (slab_bgra, bgra_pitch)):
        for i in range(distinct):
            host = rng.integers(0, 256, pitch, dtype=np.uint8)
            _capi.check(lib.bt709hip_upload(h, slab.ptr + i * pitch, pitch, host.ctypes.data, pitch, pitch, 1, None))
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for i in range(distinct, ring, distinct):
            _capi.check(lib.bt709hip_copy_probe(h, slab.ptr + i * pitch, slab.ptr, min(distinct, ring - i) * pitch, None))
    _capi.check(lib.bt709hip_stream_synchronize(h, None))
    frames = (_capi.Frame * ring)(*[_capi.Frame(slab_planes.ptr + i * plane_pitch, W, slab_planes.ptr + i * plane_pitch + W * H, W, W, H, 1, 2) for i in range(ring)])
    alphas = (_capi.Frame * ring)(*[_capi.Frame(slab_planes.ptr + i * plane_pitch + W * H * 3 // 2, W, slab_planes.ptr + i * plane_pitch + W * H, W, W, H, 1, 3)
                                    for i in range(ring)])
    surfs = (_capi.Surface * ring)(*[_capi.Surface(slab_bgra.ptr + i * bgra_pitch, W * 4, W, H, _capi.FORMAT_BGRA8_SRGB, 0) for i in range(ring)])
    f_size, s_size = C.sizeof(_capi.Frame), C.sizeof(_capi.Surface)

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
    _capi.check(lib.bt709hip_decoder_create(h, mb.MetalBT709GammaSRGB, 1, C.byref(dec)))
    _capi.check(lib.bt709hip_decoder_setup(dec))
    _capi.check(lib.bt709hip_encoder_prepare(h, mb.MetalBT709GammaSRGB, mb.MetalBT709GammaSRGB))
    state = {"i": 0}

    def at(array, size, kind):
        return C.cast(C.byref(array, state["i"] * size), C.POINTER(kind))

    def encode(count):
        def step():
            state["i"] = (state["i"] + 1) % ring if count == 1 else 0
            _capi.check(lib.bt709hip_encode_batch(h, count, at(surfs, s_size, _capi.Surface), at(frames, f_size, _capi.Frame),
                                                  mb.MetalBT709GammaSRGB, mb.MetalBT709GammaSRGB, None, 0))
        return step

    def decode(count):
        def step():
            state["i"] = (state["i"] + 1) % ring if count == 1 else 0
            _capi.check(lib.bt709hip_decode_batch(dec, count, at(frames, f_size, _capi.Frame), at(alphas, f_size, _capi.Frame),
                                                  at(surfs, s_size, _capi.Surface), None, 0))
        return step

    def set_encode(on):
        return lib.bt709hip_context_set_option(h, CTX_OPT_ENCODE_PREMULTIPLY, on)

    def set_decode(on):
        return lib.bt709hip_decoder_set_option(dec, OPT_UNPREMULTIPLY, on)

    legs, ratios = {}, {}
    for what, make, switch, new, bpp in (("encode", encode, set_encode, "premultiply", 5.5), ("decode_alpha", decode, set_decode, "straight", 6.5)):
        if switch(1) != _capi.OK:
            continue  # a build that predates the options
        switch(0)
        for count in ((ring,) if args.batched_only else (ring, 1)):
            step = make(count)
            reps = calibrate(step)
            samples, kernels = {"plain": [], new: []}, {}
            for _ in range(args.rounds):  # alternating legs
                for name, on in (("plain", 0), (new, 1)):
                    _capi.check(switch(on))
                    step()  # one untimed step under the new setting
                    samples[name].append(region(step, reps))
                    kernels[name] = lib.bt709hip_last_kernel_name().decode()
            _capi.check(switch(0))
            for name in ("plain", new):
                s = sorted(samples[name])
                us = s[len(s) // 2] * 1e3 / (reps * count)
                legs["%s/%s/%d_per_launch" % (what, name, count)] = {
                    "us_per_frame": round(us, 3), "gpixel_per_s": round(W * H / us / 1e3, 1), "algorithmic_bytes": int(W * H * bpp),
                    "frac_of_8TBps": round(W * H * bpp / us / 1e3 / 8000, 4), "kernel": kernels[name], "region_ms": [round(v, 1) for v in samples[name]],
                    "spread_max_over_min": round(s[-1] / s[0], 4), "reps": reps}
            ratios["%s/%s over plain, time, %d_per_launch" % (what, new, count)] = round(
                legs["%s/%s/%d_per_launch" % (what, new, count)]["us_per_frame"] / legs["%s/plain/%d_per_launch" % (what, count)]["us_per_frame"], 4)
    lib.bt709hip_decoder_destroy(dec)
    print(json.dumps({"workload": "%dx%d, %d resident: BGRA8 -> NV12 plain / premultiplying; NV12 + alpha frame -> BGRA8 plain / straight alpha; same slabs, "
                                  "random content, alternating legs" % (W, H, ring), "legs": legs, "ratios": ratios}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
