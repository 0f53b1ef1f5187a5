#!/usr/bin/env python3
"""An RGBA16Float surface's colour frame AND alpha frame in ONE launch (BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA) against
the plain half encode and against the three launches it replaces, in ONE process on the SAME slabs (placement cancels):
3840x2160 pictures resident in HBM, 32 per launch and one per launch, NV12 and I420, the alpha frame with and without a chroma plane.
Legs, per regime:
  * pair/<layout>/<cbcr|y>    the new kernel: 8 read + 1.5 + 1.5 (or + 1) written = 11 (10.5) B per pixel;
  * half/<layout>             the plain half encode (option at 0): 9.5 B per pixel;
  * three/<layout>/<cbcr|y>   what the pair replaces, code the parent commit has: the half encode (9.5), bt709hip_render_scaled
                              RGBA16F -> BGRA8 at the same size (8 + 4), a BGRA8_ALPHA encode of that scratch surface (4 + 1.5 or 1):
                              27 (26.5) B per pixel, three launches.
Not the headline bench (that is bench.py).  The legs ALTERNATE: `--rounds` times through all of them; a sample is one region of
>= 100 ms between two HIP events on the launch stream, after untimed steps; a figure is the median of its leg's samples, and each
leg's own max / min over its samples is the spread a ratio has to be read against.

    python tools/bench_encode_half_alpha.py [--ring 32] [--rounds 5] [--out-gamma 0]

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

LINEAR = mb.MetalBT709GammaLinear
LAYOUTS = {"nv12": _capi.CHROMA_NV12, "i420": _capi.CHROMA_I420}


def bytes_per_pixel(leg):
    kind, _, rest = leg.partition("/")
    alpha = 1.5 if rest.endswith("cbcr") else 1.0
    return {"half": 9.5, "pair": 9.5 + alpha, "three": 9.5 + 12.0 + 4.0 + alpha}[kind]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=32, help="pictures resident in HBM = pictures of the batched launch")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=5, help="samples per leg; the legs alternate")
    ap.add_argument("--out-gamma", type=int, default=mb.MetalBT709GammaApple)
    args = ap.parse_args()
    W, H, ring, out_gamma = args.width, args.height, args.ring, args.out_gamma
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal()
    lib, h = ctx.lib, ctx.handle

    half_pitch, bgra_pitch, frame_bytes = W * H * 8, W * H * 4, W * H * 3 // 2
    slab_half, slab_bgra, slab_out, slab_alpha = (DeviceBuffer(ctx, ring * nb, 1) for nb in (half_pitch, bgra_pitch, frame_bytes, frame_bytes))
    rng = np.random.default_rng(0x21)
    distinct = min(ring, 4)  # random pictures from the host (every half in [0, 1], A too); the rest are device-side copies of them
    for i in range(distinct):
        host = rng.integers(0, 0x3C01, W * H * 4, dtype=np.uint16)
        _capi.check(lib.bt709hip_upload(h, slab_half.ptr + i * half_pitch, half_pitch, host.ctypes.data, half_pitch, half_pitch, 1, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
    for i in range(distinct, ring, distinct):
        _capi.check(lib.bt709hip_copy_probe(h, slab_half.ptr + i * half_pitch, slab_half.ptr, min(distinct, ring - i) * half_pitch, None))
    _capi.check(lib.bt709hip_stream_synchronize(h, None))

    def frames(slab, planar, chroma=True):
        return [_capi.Frame(slab.ptr + i * frame_bytes, W, slab.ptr + i * frame_bytes + W * H if chroma else None, (W // 2 if planar else W) if chroma else 0, W, H, 0, 0)
                for i in range(ring)]

    def surfaces(slab, pitch, px, fmt):
        return (_capi.Surface * ring)(*[_capi.Surface(slab.ptr + i * pitch, W * px, W, H, fmt, 0) for i in range(ring)])

    halves = surfaces(slab_half, half_pitch, 8, _capi.FORMAT_RGBA16F)
    scratch = surfaces(slab_bgra, bgra_pitch, 4, _capi.FORMAT_BGRA8_SRGB)
    scratch_alpha = surfaces(slab_bgra, bgra_pitch, 4, _capi.FORMAT_BGRA8_ALPHA)
    f_size, s_size = C.sizeof(_capi.Frame), C.sizeof(_capi.Surface)

    def at(array, size, kind, i):
        return C.cast(C.byref(array, i * size), C.POINTER(kind))

    def pair_frames(planar, chroma, i, count):
        """colour frames i .. i + count, then their alpha frames: the 2 x count array a paired call takes"""
        colour, alpha = frames(slab_out, planar)[i:i + count], frames(slab_alpha, planar, chroma)[i:i + count]
        return (_capi.Frame * (2 * count))(*(colour + alpha))

    _capi.check(lib.bt709hip_render_scaled_prepare(h))
    _capi.check(lib.bt709hip_context_set_option(h, _capi.CTX_OPT_ENCODE_HALF_WITH_ALPHA, 1))
    _capi.check(lib.bt709hip_encoder_prepare(h, LINEAR, out_gamma))
    _capi.check(lib.bt709hip_encoder_prepare(h, LINEAR, LINEAR))
    _capi.check(lib.bt709hip_context_set_option(h, _capi.CTX_OPT_ENCODE_HALF_WITH_ALPHA, 0))

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

    def option(name, value):
        _capi.check(lib.bt709hip_context_set_option(h, name, value))

    state = {"i": 0}

    def make(leg, count):
        kind, layout, chroma = (leg.split("/") + ["cbcr"])[:3]
        planar, chroma = layout == "i420", chroma == "cbcr"
        colour = (_capi.Frame * ring)(*frames(slab_out, planar))
        alpha = (_capi.Frame * ring)(*frames(slab_alpha, planar, chroma))
        paired = [pair_frames(planar, chroma, i, count) for i in (range(ring) if count == 1 else [0])] if kind == "pair" else None

        def step():
            i = state["i"] = (state["i"] + 1) % ring if count == 1 else 0
            if kind == "pair":
                _capi.check(lib.bt709hip_encode_batch(h, count, at(halves, s_size, _capi.Surface, i), paired[i], LINEAR, out_gamma, None, 0))
                return
            _capi.check(lib.bt709hip_encode_batch(h, count, at(halves, s_size, _capi.Surface, i), at(colour, f_size, _capi.Frame, i), LINEAR, out_gamma, None, 0))
            if kind == "three":
                _capi.check(lib.bt709hip_render_scaled_batch(h, count, at(halves, s_size, _capi.Surface, i), at(scratch, s_size, _capi.Surface, i), None, 0))
                _capi.check(lib.bt709hip_encode_batch(h, count, at(scratch_alpha, s_size, _capi.Surface, i), at(alpha, f_size, _capi.Frame, i), LINEAR, LINEAR, None, 0))
        return step

    def enter(leg):  # the options a leg runs under, set once per region (as a C caller would hold them)
        kind, layout = leg.split("/")[:2]
        option(_capi.CTX_OPT_ENCODE_HALF_INPUT, 1)
        option(_capi.CTX_OPT_ENCODE_HALF_WITH_ALPHA, int(kind == "pair"))
        option(_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, LAYOUTS[layout])

    names = [k + "/" + lay + c for lay in LAYOUTS for k, c in (("pair", "/cbcr"), ("pair", "/y"), ("half", ""), ("three", "/cbcr"), ("three", "/y"))]
    legs, ratios = {}, {}
    for count in (ring, 1):
        steps = {n: make(n, count) for n in names}
        reps = {}
        for n in names:
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
                "us_per_picture": round(us, 3), "gpixel_per_s": round(W * H / us / 1e3, 1), "algorithmic_bytes": int(W * H * bytes_per_pixel(n)),
                "frac_of_8TBps": round(W * H * bytes_per_pixel(n) / us / 1e3 / 8000, 4), "last_kernel": kernels[n],
                "region_ms": [round(v, 1) for v in samples[n]], "spread_max_over_min": round(s[-1] / s[0], 4), "reps": reps[n]}
        us = lambda n: legs["%s/%d_per_launch" % (n, count)]["us_per_picture"]
        for lay in LAYOUTS:
            for c in ("cbcr", "y"):
                ratios["pair/%s/%s over the plain half encode, time, %d_per_launch" % (lay, c, count)] = round(us("pair/%s/%s" % (lay, c)) / us("half/" + lay), 4)
                ratios["pair/%s/%s over the three launches, time, %d_per_launch" % (lay, c, count)] = round(us("pair/%s/%s" % (lay, c)) / us("three/%s/%s" % (lay, c)), 4)
    option(_capi.CTX_OPT_ENCODE_HALF_WITH_ALPHA, 0)  # the defaults back
    option(_capi.CTX_OPT_ENCODE_HALF_INPUT, 0)
    option(_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, _capi.CHROMA_NV12)
    print(json.dumps({"workload": "%dx%d, %d resident: RGBA16F -> colour frame + alpha frame in one launch against the plain half encode and the three "
                                  "launches (half encode, render_scaled 1:1, BGRA8_ALPHA encode); same slabs, random halves in [0, 1], alternating legs, "
                                  "output gamma %d" % (W, H, ring, out_gamma), "legs": legs, "ratios": ratios}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
