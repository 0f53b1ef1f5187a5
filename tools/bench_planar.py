#!/usr/bin/env python3
"""The planar (I420) 1:1 decode (BT709HIP_OPT_CHROMA_LAYOUT) against its two yardsticks, in ONE process over
the SAME resident pictures (placement cancels):

    nv12        the NV12 decode of the interleaved twin                       5.5 B per pixel, one launch
    i420        the planar decode, in place                                   5.5 B per pixel, one launch
    detour      bt709hip_interleave_cbcr per frame, then the NV12 decode      6.5 B per pixel, N + 1 launches
                (what metalbt709decoder_amd.y4m.i420_to_pixel_buffer + decodeBT709 do without the option)

A ring of --ring frames (default 256: larger than the memory-side cache at either size) holds, per slot, Y, the CbCr plane, and
the U and V planes of the same picture; a launch covers N = 1, 8, 32 or 256 consecutive slots and successive launches walk the
ring.  Per size and N the legs are interleaved and the round is repeated --rounds times (nv12 i420 detour nv12 i420 ...), each
sample a region of >= --region-ms between two HIP events; the table gives every leg's median and spread, so the I420 figure can
be read beside the spread of the NV12 runs of the same session.  Not the headline bench (that is bench.py).

    python tools/bench_planar.py [--library <another build>] [--sizes 3840x2160,1920x1080] [--out profiles/r12_planar.txt]

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

OPT_CHROMA_LAYOUT, CHROMA_NV12, CHROMA_I420 = 11, 0, 1  # spelled out: --library may load a build whose _capi twin predates the option


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=256, help="frames resident in HBM")
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--counts", default="1,8,32,256", help="frames per launch")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved repeats of the legs")
    ap.add_argument("--region-ms", type=float, default=60.0, help="least length of a timed region")
    ap.add_argument("--gamma", type=int, default=mb.MetalBT709GammaApple)
    ap.add_argument("--library", default=None, help="a variant build of libbt709hip.so")
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
    if args.library:
        _capi.load(os.path.abspath(args.library))
    from metalbt709decoder_amd.decoder import DeviceBuffer
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal()
    lib, h = ctx.lib, ctx.handle
    transfer = {mb.MetalBT709GammaSRGB: 2, mb.MetalBT709GammaLinear: 3}.get(args.gamma, 1)

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

    dec = C.c_void_p()
    _capi.check(lib.bt709hip_decoder_create(h, args.gamma, 0, C.byref(dec)))
    _capi.check(lib.bt709hip_decoder_setup(dec))
    has_option = lib.bt709hip_decoder_set_option(dec, OPT_CHROMA_LAYOUT, CHROMA_NV12) == _capi.OK
    f_size, s_size = C.sizeof(_capi.Frame), C.sizeof(_capi.Surface)
    lines, results = [], {}

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit("# tools/bench_planar.py: %s, ring %d, %d rounds of interleaved legs, regions >= %.0f ms; us per frame: median [min .. max]"
         % ((ctx.info().name or ctx.info().arch).decode(), args.ring, args.rounds, args.region_ms))
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        ring = args.ring
        # one slot: Y, CbCr, U, V -- the two chroma forms of one picture side by side, so every leg has the same frame spacing
        slot, out_pitch = 2 * W * H, 4 * W * H
        slab_in, slab_out = DeviceBuffer(ctx, ring * slot, 1), DeviceBuffer(ctx, ring * out_pitch, 1)
        rng = np.random.default_rng(0x1420)
        distinct = min(ring, 4)  # random frames from the host; the rest of the ring are device-side copies of them
        for i in range(distinct):
            y = rng.integers(0, 256, W * H, dtype=np.uint8)
            c = rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
            host = np.concatenate([y, c.reshape(-1), c[:, 0::2].reshape(-1), c[:, 1::2].reshape(-1)])
            _capi.check(lib.bt709hip_upload(h, slab_in.ptr + i * slot, slot, host.ctypes.data, slot, slot, 1, None))
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for i in range(distinct, ring, distinct):
            _capi.check(lib.bt709hip_copy_probe(h, slab_in.ptr + i * slot, slab_in.ptr, min(distinct, ring - i) * slot, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        base = lambda i: slab_in.ptr + i * slot
        nv12 = (_capi.Frame * ring)(*[_capi.Frame(base(i), W, base(i) + W * H, W, W, H, 1, transfer) for i in range(ring)])
        i420 = (_capi.Frame * ring)(*[_capi.Frame(base(i), W, base(i) + W * H * 3 // 2, W // 2, W, H, 1, transfer) for i in range(ring)])
        surfs = (_capi.Surface * ring)(*[_capi.Surface(slab_out.ptr + i * out_pitch, W * 4, W, H, _capi.FORMAT_BGRA8_SRGB, 0) for i in range(ring)])

        if has_option:  # what is timed computes the same picture: slot 0 through both layouts, byte for byte
            got = []
            for frames, layout in ((nv12, CHROMA_NV12), (i420, CHROMA_I420)):
                _capi.check(lib.bt709hip_decoder_set_option(dec, OPT_CHROMA_LAYOUT, layout))
                _capi.check(lib.bt709hip_decode_batch(dec, 1, frames, None, surfs, None, 1))
                got.append(np.empty(out_pitch, np.uint8))
                _capi.check(lib.bt709hip_download(h, got[-1].ctypes.data, out_pitch, slab_out.ptr, out_pitch, out_pitch, 1, None))
                _capi.check(lib.bt709hip_stream_synchronize(h, None))
            assert np.array_equal(got[0], got[1]), "%dx%d: the planar decode differs from the NV12 decode of the same picture" % (W, H)

        for n in (int(v) for v in args.counts.split(",")):
            if n > ring:
                continue
            state = {"i": 0}

            def window():
                i = state["i"]
                state["i"] = (i + n) % ring if i + 2 * n <= ring else 0
                return i

            def decode(frames, layout, i):
                if has_option:
                    _capi.check(lib.bt709hip_decoder_set_option(dec, OPT_CHROMA_LAYOUT, layout))
                _capi.check(lib.bt709hip_decode_batch(dec, n, C.cast(C.byref(frames, i * f_size), C.POINTER(_capi.Frame)), None,
                                                      C.cast(C.byref(surfs, i * s_size), C.POINTER(_capi.Surface)), None, 0))

            def leg_nv12():
                decode(nv12, CHROMA_NV12, window())

            def leg_i420():
                decode(i420, CHROMA_I420, window())

            def leg_detour():
                i = window()
                for k in range(i, i + n):  # U, V -> the slot's CbCr plane, one launch per frame
                    u = base(k) + W * H * 3 // 2
                    _capi.check(lib.bt709hip_interleave_cbcr(h, u, W // 2, u + W * H // 4, W // 2, base(k) + W * H, W, W // 2, H // 2, None, 0))
                decode(nv12, CHROMA_NV12, i)

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
                row[name] = {"us_per_frame": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3), "kernel": kernels[name],
                             "gpixel_per_s": round(W * H / s[len(s) // 2] / 1e3, 2), "reps": reps[name]}
            med = lambda name: row[name]["us_per_frame"]
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
        slab_in.free()
        slab_out.free()
    lib.bt709hip_decoder_destroy(dec)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"workload": "1:1 decode of resident frames, NV12 / planar I420 in place / interleave + NV12, same pictures, same slabs",
                      "library": args.library or "in-tree", "legs": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
