#!/usr/bin/env python3
"""The fused decode + rescale through the RGBA16Float intermediate (BT709HIP_OPT_SCALE_INTERMEDIATE = RGBA16F) against what it
replaces and against the 8-bit mode, in ONE process on the same buffers, the three alternating region by region:

    (a) f16     bt709hip_decode_scaled_batch with the option at RGBA16F: one launch, no intermediate
    (b) 2pass   bt709hip_decode_batch into RGBA16F surfaces of the frame's size + bt709hip_render_scaled[_batch] from them: the
                two launches (a) equals bit for bit.  The intermediates are `frames-per-launch` surfaces, written and read again
                by every group of frames -- what a caller with that many frames in flight keeps alive
    (c) srgb8   bt709hip_decode_scaled_batch with the option at its default: the fused 8-bit kernel

Method of bench.py / tools/bench_scaled.py: frames in a ring carved from one allocation (several times the 256 MB memory-side
cache), HIP events on the launch stream around regions of at least 100 ms (the step count is sized from a timed step), every
mode warmed up, median of 5 regions per mode; `spread` = (max - min) / median of a mode's five regions, the run-to-run noise a
difference has to exceed.  One JSON line.

    python tools/bench_scaled_f16.py [--width 3840 --height 2160 --out-width 2560 --out-height 1440 --frames-per-launch 8]
    python tools/bench_scaled_f16.py --modes c --library <another build>     # the 8-bit mode of a build without the option
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gpu_helpers as gh  # noqa: E402
import metalbt709decoder_amd as mb  # noqa: E402
from metalbt709decoder_amd import _capi  # noqa: E402
from metalbt709decoder_amd.decoder import DeviceBuffer  # noqa: E402

OPT_SCALE_INTERMEDIATE = 8  # spelled out: --library may load a build whose _capi twin predates the option
NAMES = {"a": "f16", "b": "2pass", "c": "srgb8"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=64)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--out-width", type=int, default=2560)
    ap.add_argument("--out-height", type=int, default=1440)
    ap.add_argument("--frames-per-launch", type=int, default=8)
    ap.add_argument("--region-ms", type=float, default=120.0, help="least length of a timed region")
    ap.add_argument("--modes", default="abc", help="which of a (f16), b (2pass), c (srgb8) to time")
    ap.add_argument("--gamma", default="apple", choices=["apple", "srgb", "linear", "itu709"])
    ap.add_argument("--library", default=None, help="a variant build of libbt709hip.so")
    args = ap.parse_args()
    if args.library:
        _capi.load(os.path.abspath(args.library))
    W, H, OW, OH = args.width, args.height, args.out_width, args.out_height
    fpl = max(1, min(args.frames_per_launch, args.ring))
    ring = args.ring - args.ring % fpl
    modes = [m for m in "abc" if m in args.modes]
    ctx = gh.context()
    lib, h = ctx.lib, ctx.handle
    gamma = {"apple": mb.MetalBT709GammaApple, "srgb": mb.MetalBT709GammaSRGB, "linear": mb.MetalBT709GammaLinear,
             "itu709": mb.MetalBT709GammaITU709}[args.gamma]
    dec8 = gh.make_decoder(gamma)
    dec16 = gh.make_decoder(gamma, options={OPT_SCALE_INTERMEDIATE: _capi.FORMAT_RGBA16F}) if "a" in modes else None

    in_pitch = (W * H * 3 // 2 + 255) // 256 * 256
    out_pitch = (OW * OH * 4 + 255) // 256 * 256
    mid_pitch = (W * H * 8 + 255) // 256 * 256
    slab_in, slab_out = DeviceBuffer(ctx, ring * in_pitch), DeviceBuffer(ctx, ring * out_pitch)
    slab_mid = DeviceBuffer(ctx, fpl * mid_pitch) if "b" in modes else None
    frames, surfs, mids = (_capi.Frame * ring)(), (_capi.Surface * ring)(), (_capi.Surface * fpl)()
    for i in range(ring):
        y, c = gh.random_nv12(W, H, seed=0x709 + i)
        base = slab_in.ptr + i * in_pitch
        ctx._upload(base, W, y, None)
        ctx._upload(base + W * H, W, c, None)
        ctx._sync(None)
        frames[i] = _capi.Frame(base, W, base + W * H, W, W, H, 1, gh.TRANSFER_FOR_GAMMA[dec8.gamma])
        surfs[i] = _capi.Surface(slab_out.ptr + i * out_pitch, OW * 4, OW, OH, _capi.FORMAT_BGRA8_SRGB, 0)
    for k in range(fpl if slab_mid is not None else 0):
        mids[k] = _capi.Surface(slab_mid.ptr + k * mid_pitch, W * 8, W, H, _capi.FORMAT_RGBA16F, 0)
    fsz, ssz = C.sizeof(_capi.Frame), C.sizeof(_capi.Surface)
    kernels = {}

    def step(mode):
        for i in range(0, ring, fpl):
            fp = C.cast(C.byref(frames, i * fsz), C.POINTER(_capi.Frame))
            sp = C.cast(C.byref(surfs, i * ssz), C.POINTER(_capi.Surface))
            if mode == "a":
                _capi.check(lib.bt709hip_decode_scaled_batch(dec16._handle, fpl, fp, None, sp, None, 0), "f16")
            elif mode == "c":
                _capi.check(lib.bt709hip_decode_scaled_batch(dec8._handle, fpl, fp, None, sp, None, 0), "srgb8")
            else:
                _capi.check(lib.bt709hip_decode_batch(dec8._handle, fpl, fp, None, mids, None, 0), "pass 1")
                if fpl == 1:
                    _capi.check(lib.bt709hip_render_scaled(h, mids, sp, None, 0), "pass 2")
                else:
                    _capi.check(lib.bt709hip_render_scaled_batch(h, fpl, mids, sp, None, 0), "pass 2")
        kernels.setdefault(mode, lib.bt709hip_last_kernel_name().decode())

    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.bt709hip_event_create(h, C.byref(e0))
    lib.bt709hip_event_create(h, C.byref(e1))

    def timed(mode, steps):
        ctx._sync(None)
        lib.bt709hip_event_record(h, e0, None)
        for _ in range(steps):
            step(mode)
        lib.bt709hip_event_record(h, e1, None)
        ctx._sync(None)
        ms = C.c_float()
        lib.bt709hip_event_elapsed_ms(h, e0, e1, C.byref(ms))
        return ms.value

    steps = {}
    for m in modes:  # warm-up (code objects, tables built on first use, clocks), then the step count for a region of region-ms
        t_end = time.perf_counter() + 0.3
        while time.perf_counter() < t_end:
            step(m)
            ctx._sync(None)
        steps[m] = max(1, int(args.region_ms / max(timed(m, 2) / 2, 1e-3)) + 1)
    regions = {m: [] for m in modes}
    for _ in range(5):  # the modes alternate: drift of the clocks or of a shared host lands on all of them
        for m in modes:
            regions[m].append(timed(m, steps[m]) * 1e3 / (steps[m] * ring))  # us per frame
    nbytes = W * H * 3 // 2 + OW * OH * 4  # what the fused rescale has to move per frame
    out = {"workload": "%dx%d -> %dx%d, %d frame(s) per launch, ring %d, gamma %s" % (W, H, OW, OH, fpl, ring, args.gamma),
           "algorithmic_bytes_per_frame": nbytes, "region_ms": {NAMES[m]: round(min(regions[m]) * steps[m] * ring / 1e3, 1) for m in modes}}
    for m in modes:
        r = sorted(regions[m])
        out[NAMES[m]] = {"us_per_frame": round(r[2], 3), "spread": round((r[4] - r[0]) / r[2], 4),
                         "out_gpixel_per_s": round(OW * OH / r[2] / 1e3, 1), "frac_of_8TBps": round(nbytes / r[2] / 1e3 / 8000, 4),
                         "kernel": kernels[m]}
    if "a" in modes and "b" in modes:
        out["f16_over_2pass"] = round(sorted(regions["a"])[2] / sorted(regions["b"])[2], 4)
    if "a" in modes and "c" in modes:
        out["f16_over_srgb8"] = round(sorted(regions["a"])[2] / sorted(regions["c"])[2], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
