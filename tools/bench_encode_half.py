#!/usr/bin/env python3
"""RGBA16Float linear-light surfaces -> NV12 / I420 in ONE launch (BT709HIP_CTX_OPT_ENCODE_HALF_INPUT) against what it
replaces and against its mirror image, in ONE process on the SAME slabs (placement cancels): 3840x2160 pictures
resident in HBM, 32 per launch and one per launch.  Legs, per regime:
  * half/nv12, half/i420   (a) the new kernel: 8 read + 1.5 written = 9.5 B per pixel;
  * two                    (b) what it replaces, the parent commit's code: bt709hip_render_scaled RGBA16F -> BGRA8 at the same size
                           (8 + 4), then bt709hip_encode (SRGB, out) of that (4 + 1.5): 17.5 B per pixel, two launches;
  * decode                 (c) decode_nv12_rgba16f of the frames leg (a) wrote: the same 9.5 B per pixel the other way;
  * copy                   (d) the streaming copy that moves the same bytes: 4.75 B per pixel read and as many written.
Not the headline bench (that is bench.py).  The legs ALTERNATE: `--rounds` times through all of them; a sample is one region of
>= 100 ms between two HIP events on the launch stream, after three untimed steps; a figure is the median of its leg's samples, and
each yardstick's own max / min over its samples is the spread a ratio has to be read against.

    python tools/bench_encode_half.py [--ring 32] [--rounds 5] [--out-gamma 0]

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

SRGB, LINEAR = mb.MetalBT709GammaSRGB, mb.MetalBT709GammaLinear
BYTES_PER_PIXEL = {"half/nv12": 9.5, "half/i420": 9.5, "two": 17.5, "decode": 9.5, "copy": 9.5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=32, help="pictures resident in HBM = pictures of the batched launch")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=5, help="samples per leg; the legs alternate")
    ap.add_argument("--out-gamma", type=int, default=mb.MetalBT709GammaApple, help="output gamma of legs (a) and (b), the decoder's of (c)")
    args = ap.parse_args()
    W, H, ring, out_gamma = args.width, args.height, args.ring, args.out_gamma
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal()
    lib, h = ctx.lib, ctx.handle

    half_pitch, bgra_pitch, frame_bytes = W * H * 8, W * H * 4, W * H * 3 // 2
    slab_half, slab_bgra, slab_out = (DeviceBuffer(ctx, ring * nb, 1) for nb in (half_pitch, bgra_pitch, frame_bytes))
    slab_decoded = DeviceBuffer(ctx, ring * half_pitch, 1)  # leg (c) writes here: the encoders' input stays what it is
    rng = np.random.default_rng(0x19)
    distinct = min(ring, 4)  # random pictures from the host (every half in [0, 1], A too); the rest are device-side copies of them
    for i in range(distinct):
        host = rng.integers(0, 0x3C01, W * H * 4, dtype=np.uint16)
        _capi.check(lib.bt709hip_upload(h, slab_half.ptr + i * half_pitch, half_pitch, host.ctypes.data, half_pitch, half_pitch, 1, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
    for i in range(distinct, ring, distinct):
        _capi.check(lib.bt709hip_copy_probe(h, slab_half.ptr + i * half_pitch, slab_half.ptr, min(distinct, ring - i) * half_pitch, None))
    _capi.check(lib.bt709hip_stream_synchronize(h, None))

    transfer = {0: 1, 1: 2, 2: 3}[out_gamma]  # the tag leg (c)'s decoder asks of a frame of this gamma

    def frames(planar):
        return (_capi.Frame * ring)(*[_capi.Frame(slab_out.ptr + i * frame_bytes, W, slab_out.ptr + i * frame_bytes + W * H, W // 2 if planar else W, W, H, 1, transfer)
                                      for i in range(ring)])

    def surfaces(slab, pitch, px, fmt):
        return (_capi.Surface * ring)(*[_capi.Surface(slab.ptr + i * pitch, W * px, W, H, fmt, 0) for i in range(ring)])

    halves = surfaces(slab_half, half_pitch, 8, _capi.FORMAT_RGBA16F)
    decoded = surfaces(slab_decoded, half_pitch, 8, _capi.FORMAT_RGBA16F)
    bytes8 = surfaces(slab_bgra, bgra_pitch, 4, _capi.FORMAT_BGRA8_SRGB)
    out = {False: frames(False), True: frames(True)}
    f_size, s_size = C.sizeof(_capi.Frame), C.sizeof(_capi.Surface)

    dec = mb.MetalBT709Decoder()
    dec.metalRenderContext, dec.gamma = ctx, out_gamma
    assert dec.setupMetal(), dec.lastStatus
    _capi.check(lib.bt709hip_decoder_prepare_format(dec._handle, _capi.FORMAT_RGBA16F))
    _capi.check(lib.bt709hip_render_scaled_prepare(h))
    for gi in (SRGB, LINEAR):
        _capi.check(lib.bt709hip_encoder_prepare(h, gi, out_gamma))

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

    state = {"i": 0}

    def at(array, size, kind, i):
        return C.cast(C.byref(array, i * size), C.POINTER(kind))

    def option(name, value):
        _capi.check(lib.bt709hip_context_set_option(h, name, value))

    def make(leg, count):
        planar = leg == "half/i420"

        def step():
            i = state["i"] = (state["i"] + 1) % ring if count == 1 else 0
            if leg.startswith("half"):
                _capi.check(lib.bt709hip_encode_batch(h, count, at(halves, s_size, _capi.Surface, i), at(out[planar], f_size, _capi.Frame, i), LINEAR, out_gamma, None, 0))
            elif leg == "two":
                _capi.check(lib.bt709hip_render_scaled_batch(h, count, at(halves, s_size, _capi.Surface, i), at(bytes8, s_size, _capi.Surface, i), None, 0))
                _capi.check(lib.bt709hip_encode_batch(h, count, at(bytes8, s_size, _capi.Surface, i), at(out[False], f_size, _capi.Frame, i), SRGB, out_gamma, None, 0))
            elif leg == "decode":
                _capi.check(lib.bt709hip_decode_batch(dec._handle, count, at(out[False], f_size, _capi.Frame, i), None, at(decoded, s_size, _capi.Surface, i), None, 0))
            else:
                nb = count * W * H * 19 // 4  # 4.75 B per pixel read, as many written
                _capi.check(lib.bt709hip_copy_probe(h, slab_decoded.ptr + i * half_pitch, slab_half.ptr + i * half_pitch, nb, None))
        return step

    def enter(leg):  # the options a leg runs under, set once per region (as a C caller would hold them)
        option(_capi.CTX_OPT_ENCODE_HALF_INPUT, int(leg.startswith("half")))
        option(_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, _capi.CHROMA_I420 if leg == "half/i420" else _capi.CHROMA_NV12)

    names = list(BYTES_PER_PIXEL)
    legs, ratios = {}, {}
    for count in (ring, 1):
        steps = {n: make(n, count) for n in names}
        reps = {}
        for n in names:  # "half/nv12" first: the frames leg (c) decodes are written before it runs
            enter(n)
            reps[n] = calibrate(steps[n])
        samples, kernels = {n: [] for n in names}, {}
        for _ in range(args.rounds):  # alternating legs
            for n in names:
                enter(n)
                steps[n]()  # one untimed step
                samples[n].append(region(steps[n], reps[n]))
                kernels[n] = lib.bt709hip_last_kernel_name().decode()
        for n in names:
            s = sorted(samples[n])
            us = s[len(s) // 2] * 1e3 / (reps[n] * count)
            legs["%s/%d_per_launch" % (n, count)] = {
                "us_per_picture": round(us, 3), "gpixel_per_s": round(W * H / us / 1e3, 1), "algorithmic_bytes": int(W * H * BYTES_PER_PIXEL[n]),
                "frac_of_8TBps": round(W * H * BYTES_PER_PIXEL[n] / us / 1e3 / 8000, 4), "last_kernel": kernels[n],
                "region_ms": [round(v, 1) for v in samples[n]], "spread_max_over_min": round(s[-1] / s[0], 4), "reps": reps[n]}
        us = lambda n: legs["%s/%d_per_launch" % (n, count)]["us_per_picture"]
        for a in ("half/nv12", "half/i420"):
            for b, what in (("two", "render_scaled + encode"), ("decode", "decode_nv12_rgba16f"), ("copy", "the streaming copy")):
                ratios["%s over %s, time, %d_per_launch" % (a, what, count)] = round(us(a) / us(b), 4)
    enter("two")  # the defaults back
    print(json.dumps({"workload": "%dx%d, %d resident: RGBA16F linear -> NV12 / I420 in one launch against render_scaled + encode, the RGBA16F decode and "
                                  "the copy; same slabs, random halves in [0, 1], alternating legs, output gamma %d" % (W, H, ring, out_gamma),
                      "legs": legs, "ratios": ratios}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
