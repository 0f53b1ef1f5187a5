#!/usr/bin/env python3
"""Planar I420 frames through the fused decode + rescale (BT709HIP_OPT_SCALED_PLANAR) against its yardsticks, in ONE
process over the SAME resident frames and the SAME slabs (placement cancels).  The frames lie as a Y4M payload does --
Y, then U, then V, tight -- and an NV12 chroma plane per frame lies in a staging slab beside them.  Per workload:

    (a) nv12     bt709hip_decode_scaled_batch of the NV12 twin (Y from the frames, CbCr from the staging slab) -- kernels the parent
                 commit has, instruction for instruction (profiles/r24_scaled_planar_isa.txt): the yardstick
    (b) detour   what the feature replaces: bt709hip_interleave_cbcr of every frame's U and V into the staging slab, then (a)
    (c) planar   the planar call: the frames as they lie, no staging slab

Workloads: 1080p -> 224x224 x 32 per launch into CHW_F16 (ImageNet mean and std), 4K -> 2560x1440 x 8 and x 1 into BGRA8, 1080p -> 4K
x 8 into BGRA8 (the by-wave form).  (c)'s view 0 is compared with (a)'s before anything is timed.  The legs are interleaved and the
round repeated --rounds times, each sample a region of >= --region-ms between two HIP events; the table gives every leg's median and
its own max / min, then (c) / (a) and (c) / (b).  Not the headline bench (that is bench.py).

    python tools/bench_scaled_planar.py [--out profiles/r24_scaled_planar.txt]
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

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (source, view, frames per launch, target format, bytes per element of a row, planes)
WORKLOADS = [((1920, 1080), (224, 224), 32, _capi.FORMAT_CHW_F16, 2, 3), ((3840, 2160), (2560, 1440), 8, _capi.FORMAT_BGRA8_SRGB, 4, 1),
             ((3840, 2160), (2560, 1440), 1, _capi.FORMAT_BGRA8_SRGB, 4, 1), ((1920, 1080), (3840, 2160), 8, _capi.FORMAT_BGRA8_SRGB, 4, 1)]
TAPS_NAME = {0: "bytes", 1: "pairs", 2: "wide", 3: "shared", 4: "once"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="interleaved repeats of the legs")
    ap.add_argument("--region-ms", type=float, default=40.0, help="least length of a timed region")
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
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

    scale = np.float32(1.0) / np.array(STD, np.float32)
    bias = -np.array(MEAN, np.float32) / np.array(STD, np.float32)
    decs = {}
    for name, options in (("nv12", []), ("planar", [(_capi.OPT_CHROMA_LAYOUT, _capi.CHROMA_I420), (_capi.OPT_SCALED_PLANAR, 1)])):
        dec = C.c_void_p()
        _capi.check(lib.bt709hip_decoder_create(h, mb.MetalBT709GammaApple, 0, C.byref(dec)))
        _capi.check(lib.bt709hip_decoder_setup(dec))
        for opt, value in options + [(_capi.OPT_SCALED_CHW, 1)] + [(_capi.OPT_CHW_SCALE_R + i, int(np.array([v], np.float32).view(np.int32)[0])) for i, v in enumerate(list(scale) + list(bias))]:
            _capi.check(lib.bt709hip_decoder_set_option(dec, opt, value))
        decs[name] = dec
    f_size = C.sizeof(_capi.Frame)
    lines, results = [], {}

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit("# tools/bench_scaled_planar.py: %s, %d rounds of interleaved legs, regions >= %.0f ms; us per frame: median [min .. max] max/min"
         % ((ctx.info().name or ctx.info().arch).decode(), args.rounds, args.region_ms))
    for (W, H), (OW, OH), n, fmt, e, planes in WORKLOADS:
        ring = 2 * n if n > 1 else 8
        slot, chroma = W * H * 3 // 2, W * H // 2
        slab_in, slab_stage = DeviceBuffer(ctx, ring * slot, 1), DeviceBuffer(ctx, ring * chroma, 1)
        rng = np.random.default_rng(0xC5)
        for i in range(min(ring, 4)):
            host = rng.integers(0, 256, slot, dtype=np.uint8)
            _capi.check(lib.bt709hip_upload(h, slab_in.ptr + i * slot, slot, host.ctypes.data, slot, slot, 1, None))
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for i in range(4, ring, 4):
            _capi.check(lib.bt709hip_copy_probe(h, slab_in.ptr + i * slot, slab_in.ptr, min(4, ring - i) * slot, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        y_of, u_of, stage_of = (lambda i: slab_in.ptr + i * slot), (lambda i: slab_in.ptr + i * slot + W * H), (lambda i: slab_stage.ptr + i * chroma)
        planar = (_capi.Frame * ring)(*[_capi.Frame(y_of(i), W, u_of(i), W // 2, W, H, 1, 1) for i in range(ring)])
        nv12 = (_capi.Frame * ring)(*[_capi.Frame(y_of(i), W, stage_of(i), W, W, H, 1, 1) for i in range(ring)])
        out_pitch = planes * OW * e * OH
        slab_out = DeviceBuffer(ctx, n * out_pitch, 1)
        surfs = (_capi.Surface * n)(*[_capi.Surface(slab_out.ptr + k * out_pitch, OW * e, OW, OH, fmt, 0) for k in range(n)])

        def interleave(i, count):
            for k in range(i, i + count):
                _capi.check(lib.bt709hip_interleave_cbcr(h, u_of(k), W // 2, u_of(k) + chroma // 2, W // 2, stage_of(k), W, W // 2, H // 2, None, 0))

        def rescale(dec, frames, i, wait=0):
            _capi.check(lib.bt709hip_decode_scaled_batch(decs[dec], n, C.cast(C.byref(frames, i * f_size), C.POINTER(_capi.Frame)), None, surfs, None, wait))

        # what is timed computes one thing: the first launch's views from the planar frames against those from their NV12 twins
        interleave(0, ring)
        views = []
        for dec, frames in (("nv12", nv12), ("planar", planar)):
            rescale(dec, frames, 0, 1)
            got = np.empty(n * out_pitch, np.uint8)
            _capi.check(lib.bt709hip_download(h, got.ctypes.data, got.size, slab_out.ptr, got.size, got.size, 1, None))
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
            views.append(got)
        assert np.array_equal(views[0], views[1]), "%dx%d -> %dx%d: the planar call does not write what the NV12 call writes for the twin" % (W, H, OW, OH)

        state = {"i": 0}

        def window():
            i = state["i"]
            state["i"] = (i + n) % ring if i + 2 * n <= ring else 0
            return i

        def detour():
            i = window()
            interleave(i, n)
            rescale("nv12", nv12, i)

        legs = [("nv12", lambda: rescale("nv12", nv12, window())), ("detour", detour), ("planar", lambda: rescale("planar", planar, window()))]
        reps, kernels, taps = {}, {}, {}
        for name, step in legs:  # untimed: code objects, clocks, and the repeat count of a region
            for _ in range(3):
                step()
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
            kernels[name] = lib.bt709hip_last_kernel_name().decode()
            info = _capi.ScaledLaunchInfo()
            _capi.check(lib.bt709hip_last_scaled_launch_info(C.byref(info)))
            taps[name] = TAPS_NAME.get(info.taps, str(info.taps))
            reps[name] = max(2, int(np.ceil(args.region_ms * 1.3 / max(region(step, 4) / 4, 1e-3))))
        samples = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, step in legs:
                samples[name].append(region(step, reps[name]) * 1e3 / (reps[name] * n))
        row = {}
        emit("%dx%d -> %dx%d, %d per launch, %s" % (W, H, OW, OH, n, "CHW_F16" if fmt == _capi.FORMAT_CHW_F16 else "BGRA8"))
        for name, _ in legs:
            s = sorted(samples[name])
            row[name] = {"us_per_frame": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3), "max_over_min": round(s[-1] / s[0], 4),
                         "kernel": kernels[name], "taps": taps[name], "reps": reps[name]}
            what = kernels[name] + " (" + taps[name] + ")"
            emit("  %-7s %9.3f [%9.3f .. %9.3f] %.3f  %s" % (name, row[name]["us_per_frame"], s[0], s[-1], s[-1] / s[0], ("interleave_cbcr x %d + " % n if name == "detour" else "") + what))
        med = lambda name: row[name]["us_per_frame"]
        row["c_over_a"], row["c_over_b"] = round(med("planar") / med("nv12"), 4), round(med("planar") / med("detour"), 4)
        emit("  (c) / (a) %.3f   (c) / (b) %.3f" % (row["c_over_a"], row["c_over_b"]))
        results["%dx%d->%dx%d/%d" % (W, H, OW, OH, n)] = row
        for slab in (slab_in, slab_stage, slab_out):
            slab.free()
    for dec in decs.values():
        lib.bt709hip_decoder_destroy(dec)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"workload": "fused decode + rescale of resident planar I420 frames against the NV12 call on their twins and the interleave detour, same frames, same slabs",
                      "legs": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
