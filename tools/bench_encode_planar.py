#!/usr/bin/env python3
"""The planar (I420) encode (BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT) against its two yardsticks, in ONE process over
the SAME resident pictures (placement cancels):

    nv12        the NV12 encode                                                5.5 B per pixel, one launch
    i420        the planar encode, in place                                    5.5 B per pixel, one launch
    detour      the NV12 encode, then bt709hip_deinterleave_cbcr per frame     6.5 B per pixel, 1 + N launches
                (what metalbt709decoder_amd.y4m.pixel_buffer_to_i420 does to an NV12 buffer: the route the option replaces)

A ring of --ring pictures (default 256: larger than the memory-side cache at either size) is resident as BGRA; per slot the output
slab holds Y, the CbCr plane, and the U and V planes of the same picture, so every leg has the same frame spacing.  A launch
covers N = 1, 8, 32 or 256 consecutive slots and successive launches walk the ring.  Per size and N the legs are interleaved and
the round is repeated --rounds times (nv12 i420 detour nv12 i420 ...), each sample a region of >= --region-ms between two HIP
events; the table gives every leg's median and spread, so the I420 figure can be read beside the spread of the NV12 runs of the
same session.  Not the headline bench (that is bench.py).

    python tools/bench_encode_planar.py [--library <another build>] [--sizes 3840x2160,1920x1080] [--out profiles/r13_encode_planar.txt]

A library that predates the option runs the nv12 and detour legs alone.  Prints the table and one JSON line.
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

CTX_OPT_ENCODE_CHROMA_LAYOUT, CHROMA_NV12, CHROMA_I420 = 6, 0, 1  # spelled out: --library may load a build whose _capi twin predates the option


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=256, help="pictures resident in HBM")
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--counts", default="1,8,32,256", help="pictures per launch")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved repeats of the legs")
    ap.add_argument("--region-ms", type=float, default=60.0, help="least length of a timed region")
    ap.add_argument("--input-gamma", type=int, default=mb.MetalBT709GammaSRGB)
    ap.add_argument("--output-gamma", type=int, default=mb.MetalBT709GammaApple)
    ap.add_argument("--library", default=None, help="a variant build of libbt709hip.so")
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
    if args.library:
        _capi.load(os.path.abspath(args.library))
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal()
    lib, h = ctx.lib, ctx.handle
    gi, go = args.input_gamma, args.output_gamma
    _capi.check(lib.bt709hip_encoder_prepare(h, gi, go))

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

    has_option = lib.bt709hip_context_set_option(h, CTX_OPT_ENCODE_CHROMA_LAYOUT, CHROMA_NV12) == _capi.OK
    f_size, s_size = C.sizeof(_capi.Frame), C.sizeof(_capi.Surface)
    lines, results = [], {}

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit("# tools/bench_encode_planar.py: %s, ring %d, %d rounds of interleaved legs, regions >= %.0f ms; us per picture: median [min .. max]"
         % ((ctx.info().name or ctx.info().arch).decode(), args.ring, args.rounds, args.region_ms))
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        ring = args.ring
        # one output slot: Y, CbCr, U, V -- the two chroma forms of one picture side by side
        in_pitch, slot = 4 * W * H, 2 * W * H
        slab_in, slab_out = DeviceBuffer(ctx, ring * in_pitch, 1), DeviceBuffer(ctx, ring * slot, 1)
        rng = np.random.default_rng(0x1420)
        distinct = min(ring, 4)  # random pictures from the host; the rest of the ring are device-side copies of them
        for i in range(distinct):
            host = rng.integers(0, 256, in_pitch, dtype=np.uint8)
            _capi.check(lib.bt709hip_upload(h, slab_in.ptr + i * in_pitch, in_pitch, host.ctypes.data, in_pitch, in_pitch, 1, None))
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for i in range(distinct, ring, distinct):
            _capi.check(lib.bt709hip_copy_probe(h, slab_in.ptr + i * in_pitch, slab_in.ptr, min(distinct, ring - i) * in_pitch, None))
        _capi.check(lib.bt709hip_memset(h, slab_out.ptr, 0, ring * slot, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        base = lambda i: slab_out.ptr + i * slot
        u_of = lambda i: base(i) + W * H * 3 // 2
        surfs = (_capi.Surface * ring)(*[_capi.Surface(slab_in.ptr + i * in_pitch, W * 4, W, H, _capi.FORMAT_BGRA8_SRGB, 0) for i in range(ring)])
        nv12 = (_capi.Frame * ring)(*[_capi.Frame(base(i), W, base(i) + W * H, W, W, H, 0, 0) for i in range(ring)])
        i420 = (_capi.Frame * ring)(*[_capi.Frame(base(i), W, u_of(i), W // 2, W, H, 0, 0) for i in range(ring)])

        def set_layout(layout):
            if has_option:
                _capi.check(lib.bt709hip_context_set_option(h, CTX_OPT_ENCODE_CHROMA_LAYOUT, layout))

        def deinterleave(k, wait=0):
            _capi.check(lib.bt709hip_deinterleave_cbcr(h, base(k) + W * H, W, u_of(k), W // 2, u_of(k) + W * H // 4, W // 2, W // 2, H // 2, None, wait))

        def planes_of_slot0():
            got = np.empty(slot, np.uint8)
            _capi.check(lib.bt709hip_download(h, got.ctypes.data, slot, base(0), slot, slot, 1, None))
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
            return np.concatenate([got[:W * H], got[W * H * 3 // 2:]])  # Y, U, V

        if has_option:  # what is timed computes the same picture: slot 0 through both routes, byte for byte
            set_layout(CHROMA_NV12)
            _capi.check(lib.bt709hip_encode_batch(h, 1, surfs, nv12, gi, go, None, 1))
            deinterleave(0, 1)
            two = planes_of_slot0()
            _capi.check(lib.bt709hip_memset(h, base(0), 0, slot, None))
            set_layout(CHROMA_I420)
            _capi.check(lib.bt709hip_encode_batch(h, 1, surfs, i420, gi, go, None, 1))
            assert np.array_equal(planes_of_slot0(), two), "%dx%d: the planar encode differs from NV12 encode + de-interleave of the same picture" % (W, H)

        for n in (int(v) for v in args.counts.split(",")):
            if n > ring:
                continue
            state = {"i": 0}

            def window():
                i = state["i"]
                state["i"] = (i + n) % ring if i + 2 * n <= ring else 0
                return i

            def encode(frames, layout, i):
                set_layout(layout)
                _capi.check(lib.bt709hip_encode_batch(h, n, C.cast(C.byref(surfs, i * s_size), C.POINTER(_capi.Surface)),
                                                      C.cast(C.byref(frames, i * f_size), C.POINTER(_capi.Frame)), gi, go, None, 0))

            def leg_nv12():
                encode(nv12, CHROMA_NV12, window())

            def leg_i420():
                encode(i420, CHROMA_I420, window())

            def leg_detour():
                i = window()
                encode(nv12, CHROMA_NV12, i)
                for k in range(i, i + n):  # the slot's CbCr plane -> U, V, one launch per picture
                    deinterleave(k)

            legs = [("nv12", leg_nv12), ("detour", leg_detour)] + ([("i420", leg_i420)] if has_option else [])
            reps, kernels = {}, {}
            for name, step in legs:  # untimed: code objects, clocks, and the repeat count of a region
                for _ in range(3):
                    step()
                _capi.check(lib.bt709hip_stream_synchronize(h, None))
                kernels[name] = lib.bt709hip_last_kernel_name().decode()
                reps[name] = max(2, int(np.ceil(args.region_ms * 1.3 / max(region(step, 4) / 4, 1e-3))))
            samples = {name: [] for name, _ in legs}
            for _ in range(args.rounds):
                for name, step in legs:
                    samples[name].append(region(step, reps[name]) * 1e3 / (reps[name] * n))
            row = {}
            for name, _ in legs:
                s = sorted(samples[name])
                row[name] = {"us_per_picture": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3), "kernel": kernels[name],
                             "gpixel_per_s": round(W * H / s[len(s) // 2] / 1e3, 2), "reps": reps[name]}
            med = lambda name: row[name]["us_per_picture"]
            text = "%dx%d %3d per launch:" % (W, H, n)
            for name, _ in legs:
                text += "  %s %.3f [%.3f .. %.3f]" % (name, med(name), row[name]["min"], row[name]["max"])
            if has_option:
                row["i420_over_nv12"] = round(med("i420") / med("nv12"), 4)
                row["i420_over_detour"] = round(med("i420") / med("detour"), 4)
                row["nv12_spread"] = round(row["nv12"]["max"] / row["nv12"]["min"], 4)
                text += "  i420/nv12 %.3f (nv12 max/min %.3f)  i420/detour %.3f  %.2f Gpixel/s" % (
                    row["i420_over_nv12"], row["nv12_spread"], row["i420_over_detour"], row["i420"]["gpixel_per_s"])
            emit(text)
            results["%dx%d/%d" % (W, H, n)] = row
        set_layout(CHROMA_NV12)
        slab_in.free()
        slab_out.free()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"workload": "encode of resident pictures, NV12 / planar I420 in place / NV12 + de-interleave, same pictures, same slabs",
                      "library": args.library or "in-tree", "legs": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
