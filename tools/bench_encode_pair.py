#!/usr/bin/env python3
"""A picture's colour frame and alpha frame from ONE launch (BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA) against the two
launches it replaces, in ONE process on the SAME slabs (placement cancels): 3840x2160 BGRA pictures resident in HBM, 32
per launch and one per launch.  Legs, per regime:
  * fused/alpha_cbcr, fused/alpha_y   the paired bt709hip_encode_batch, the alpha frame with / without a chroma plane
                                      (4 read + 1.5 + 1.5 = 7, or + 1 = 6.5 B per pixel);
  * two/alpha_cbcr, two/alpha_y       the yardstick: the colour encode, then the BGRA8_ALPHA encode of the same surface
                                      (5.5 + 5.5 = 11, or + 5 = 10.5 B per pixel);
  * colour                            the plain colour encode alone (5.5 B per pixel).
Not the headline bench (that is bench.py).  The legs ALTERNATE: `--rounds` times through all five; a sample is one region of
>= 100 ms between two HIP events on the launch stream, after three untimed steps; a figure is the median of its leg's samples, and
each yardstick's own max / min over its samples is the spread a ratio has to be read against.  The yardsticks' kernels are the
parent commit's, instruction for instruction (profiles/r18_encode_pair_isa.txt): "time x two launches" is time x the parent's.
`--library <build>` runs the legs a build has (one that predates the option: the three yardstick legs alone).

    python tools/bench_encode_pair.py [--ring 32] [--rounds 5] [--library <another build>]

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

CTX_OPT_ENCODE_WITH_ALPHA, FORMAT_BGRA8_ALPHA = 12, 3  # spelled out: --library may load a build whose _capi twin differs
SRGB, LINEAR = mb.MetalBT709GammaSRGB, mb.MetalBT709GammaLinear
BYTES_PER_PIXEL = {"fused/alpha_cbcr": 7.0, "fused/alpha_y": 6.5, "two/alpha_cbcr": 11.0, "two/alpha_y": 10.5, "colour": 5.5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=32, help="pictures resident in HBM = pairs of the batched launch")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=5, help="samples per leg; the legs alternate")
    ap.add_argument("--library", default=None, help="a variant build of libbt709hip.so")
    args = ap.parse_args()
    W, H, ring = args.width, args.height, args.ring
    if args.library:
        _capi.load(os.path.abspath(args.library))
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal()
    lib, h = ctx.lib, ctx.handle

    # one slab of BGRA words and one of frames: per picture a colour frame (Y, CbCr) and an alpha frame (Y, CbCr); random words:
    # content does not change the kernels' work
    frame_bytes, bgra_pitch = W * H * 3 // 2, W * H * 4
    out_pitch = 2 * frame_bytes
    slab_out, slab_bgra = DeviceBuffer(ctx, ring * out_pitch, 1), DeviceBuffer(ctx, ring * bgra_pitch, 1)
    rng = np.random.default_rng(0x12)
    distinct = min(ring, 4)  # random pictures from the host; the rest are device-side copies of them
    for i in range(distinct):
        host = rng.integers(0, 256, bgra_pitch, dtype=np.uint8)
        _capi.check(lib.bt709hip_upload(h, slab_bgra.ptr + i * bgra_pitch, bgra_pitch, host.ctypes.data, bgra_pitch, bgra_pitch, 1, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
    for i in range(distinct, ring, distinct):
        _capi.check(lib.bt709hip_copy_probe(h, slab_bgra.ptr + i * bgra_pitch, slab_bgra.ptr, min(distinct, ring - i) * bgra_pitch, None))
    _capi.check(lib.bt709hip_stream_synchronize(h, None))

    def frame(i, alpha, cbcr=True):
        base = slab_out.ptr + i * out_pitch + (frame_bytes if alpha else 0)
        return _capi.Frame(base, W, base + W * H if cbcr else None, W if cbcr else 0, W, H, 1, 3 if alpha else 2)

    def surfaces(fmt):
        return (_capi.Surface * ring)(*[_capi.Surface(slab_bgra.ptr + i * bgra_pitch, W * 4, W, H, fmt, 0) for i in range(ring)])

    surfs, alpha_surfs = surfaces(_capi.FORMAT_BGRA8_SRGB), surfaces(FORMAT_BGRA8_ALPHA)
    colour = (_capi.Frame * ring)(*[frame(i, False) for i in range(ring)])
    alpha = {c: (_capi.Frame * ring)(*[frame(i, True, c) for i in range(ring)]) for c in (True, False)}
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

    has_option = lib.bt709hip_context_set_option(h, CTX_OPT_ENCODE_WITH_ALPHA, 1) == _capi.OK
    _capi.check(lib.bt709hip_encoder_prepare(h, SRGB, SRGB))  # under the option: T as well
    _capi.check(lib.bt709hip_encoder_prepare(h, LINEAR, LINEAR))
    if has_option:
        _capi.check(lib.bt709hip_context_set_option(h, CTX_OPT_ENCODE_WITH_ALPHA, 0))
    state = {"i": 0}

    def at(array, size, kind, i):
        return C.cast(C.byref(array, i * size), C.POINTER(kind))

    def make(leg, count):
        cbcr = leg.endswith("alpha_cbcr")
        # a paired call's frames: the colour frames, then the alpha frames -- built ahead of the timed regions (the option is set
        # once per region, as a C caller would hold it)
        pairs = [(_capi.Frame * (2 * count))(*([colour[i + k] for k in range(count)] + [alpha[cbcr][i + k] for k in range(count)]))
                 for i in (range(ring) if count == 1 else (0,))] if leg.startswith("fused") else None

        def step():
            i = state["i"] = (state["i"] + 1) % ring if count == 1 else 0
            if pairs is not None:
                _capi.check(lib.bt709hip_encode_batch(h, count, at(surfs, s_size, _capi.Surface, i), pairs[i], SRGB, SRGB, None, 0))
                return
            _capi.check(lib.bt709hip_encode_batch(h, count, at(surfs, s_size, _capi.Surface, i), at(colour, f_size, _capi.Frame, i), SRGB, SRGB, None, 0))
            if leg.startswith("two"):
                _capi.check(lib.bt709hip_encode_batch(h, count, at(alpha_surfs, s_size, _capi.Surface, i), at(alpha[cbcr], f_size, _capi.Frame, i),
                                                      LINEAR, LINEAR, None, 0))
        return step

    names = [n for n in BYTES_PER_PIXEL if has_option or not n.startswith("fused")]
    legs, ratios = {}, {}
    for count in (ring, 1):
        steps = {n: make(n, count) for n in names}
        reps = {}
        for n in names:
            if has_option:
                _capi.check(lib.bt709hip_context_set_option(h, CTX_OPT_ENCODE_WITH_ALPHA, int(n.startswith("fused"))))
            reps[n] = calibrate(steps[n])
        samples, kernels = {n: [] for n in names}, {}
        for _ in range(args.rounds):  # alternating legs
            for n in names:
                if has_option:
                    _capi.check(lib.bt709hip_context_set_option(h, CTX_OPT_ENCODE_WITH_ALPHA, int(n.startswith("fused"))))
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
        if has_option:
            us = lambda n: legs["%s/%d_per_launch" % (n, count)]["us_per_picture"]
            for kind in ("alpha_cbcr", "alpha_y"):
                ratios["fused/%s over two launches, time, %d_per_launch" % (kind, count)] = round(us("fused/" + kind) / us("two/" + kind), 4)
                ratios["fused/%s over colour alone, time, %d_per_launch" % (kind, count)] = round(us("fused/" + kind) / us("colour"), 4)
    print(json.dumps({"workload": "%dx%d, %d resident: BGRA8 -> colour NV12 + alpha frame, one launch against two; same slabs, random content, "
                                  "alternating legs" % (W, H, ring), "legs": legs, "ratios": ratios}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
