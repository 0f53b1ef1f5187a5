#!/usr/bin/env python3
"""The fused decode + rescale into planar CHW views (BT709HIP_OPT_SCALED_CHW) against its yardsticks, in ONE process
over the SAME resident frames and the SAME slabs (placement cancels).  Per shape and element type (u8 / f16 / f32, ImageNet
mean and std):

    (a) chw_*    the fused launch: frames -> normalised planar views
    (b) bgra8    bt709hip_decode_scaled_batch of the same frames and view into BGRA8 -- kernels the parent commit has, instruction for
                 instruction (profiles/r23_scaled_chw_isa.txt): what the planar epilogue costs is (a) / (b)
    (c) lean_*   what (a) replaces, written for speed as tools/bench_chw.py writes it: (b) into a uint8 tensor, one strided copy_ per
                 channel into a preallocated NCHW tensor, then mul_ and add_ in place with 1/255 folded into the scale; on torch's
                 current stream, like the rescale in front of it.  Left out (and said so) where torch does not import.

Shapes: 1080p -> 224x224 x 32 per launch, 1080p -> 384x384 x 32, 4K -> 1280x720 x 8 and x 1.  The legs are interleaved and the round
repeated --rounds times, each sample a region of >= --region-ms between two HIP events; the table gives every leg's median and its
own max / min, (a) / (b) beside the ratio of the two kernels' static instruction counts (the twin's plus the epilogue's, read from
build.emit_asm()'s output when it is there), and (c) / (a) beside the larger of the two legs' spreads: (a) is FASTER than (c) by more
than the legs' own noise when the first exceeds the second.  Not the headline bench (that is bench.py).

    python tools/bench_scaled_chw.py [--out profiles/r23_scaled_chw.txt]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import metalbt709decoder_amd as mb  # noqa: E402
from metalbt709decoder_amd import _capi  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SHAPES = [((1920, 1080), (224, 224), 32), ((1920, 1080), (384, 384), 32), ((3840, 2160), (1280, 720), 8), ((3840, 2160), (1280, 720), 1)]
ELEMS = [("u8", _capi.FORMAT_CHW_U8, 1), ("f16", _capi.FORMAT_CHW_F16, 2), ("f32", _capi.FORMAT_CHW_F32, 4)]
TAPS_ID = {"bytes": 0, "pairs": 1, "wide": 2, "shared": 3, "once": 4}
TAPS_NAME = {v: k for k, v in TAPS_ID.items()}


def instruction_counts():
    """{mangled kernel name: static instruction count} of the any-ratio kernels, from the assembly build.emit_asm() leaves; {} without it."""
    path = os.path.join(ROOT, "metalbt709decoder_amd", "build", "bt709_kernels.s")
    if not os.path.exists(path):
        return {}
    asm = open(path).read()
    bodies = re.findall(r"^(_ZN5bt709\d+decode_nv12_scaled(?:_chw)?I\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M)
    return {n: sum(1 for l in b.split("\n") if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";"))) for n, b in bodies}


def predicted(counts, taps, elem):
    """instructions of decode_nv12_scaled_chw<taps, elem, opaque> over its twin's: the epilogue's share of the kernel's text"""
    p = "1" if taps in ("bytes", "pairs", "wide") else "0"
    chw = counts.get("_ZN5bt70922decode_nv12_scaled_chwILi%dELj%dELb0ELb%sEEEvNS_12DecodeParamsE" % (TAPS_ID[taps], elem, p))
    twin = counts.get("_ZN5bt70918decode_nv12_scaledILi%dELb0ELb%sEEEvNS_12DecodeParamsE" % (TAPS_ID[taps], p))
    return chw / twin if chw and twin else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="interleaved repeats of the legs")
    ap.add_argument("--region-ms", type=float, default=40.0, help="least length of a timed region")
    ap.add_argument("--no-torch", action="store_true", help="leave the two-pass legs out")
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
    from metalbt709decoder_amd.decoder import DeviceBuffer
    torch = None
    if not args.no_torch:  # before the library is loaded: both then share one HIP runtime
        try:
            import torch
            if not (torch.cuda.is_available() and torch.cuda.device_count() > 0):
                raise RuntimeError("torch %s sees no GPU" % torch.__version__)
        except Exception as exc:  # the legs are optional: say why they are missing
            print("# (c) left out: %s" % (exc,), flush=True)
            torch = None
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal()
    lib, h = ctx.lib, ctx.handle
    stream = None
    if torch is not None:  # every leg on ONE stream: a stream of torch's made current
        torch_stream = torch.cuda.Stream()
        torch.cuda.set_stream(torch_stream)
        stream = torch_stream.cuda_stream

    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.bt709hip_event_create(h, C.byref(e0))
    lib.bt709hip_event_create(h, C.byref(e1))

    def region(step, reps):
        lib.bt709hip_event_record(h, e0, stream)
        for _ in range(reps):
            step()
        lib.bt709hip_event_record(h, e1, stream)
        _capi.check(lib.bt709hip_stream_synchronize(h, stream))
        ms = C.c_float()
        lib.bt709hip_event_elapsed_ms(h, e0, e1, C.byref(ms))
        return ms.value

    dec = C.c_void_p()
    _capi.check(lib.bt709hip_decoder_create(h, mb.MetalBT709GammaApple, 0, C.byref(dec)))
    _capi.check(lib.bt709hip_decoder_setup(dec))
    _capi.check(lib.bt709hip_decoder_set_option(dec, _capi.OPT_SCALED_CHW, 1))
    scale = np.float32(1.0) / np.array(STD, np.float32)
    bias = -np.array(MEAN, np.float32) / np.array(STD, np.float32)
    for i, v in enumerate(list(scale) + list(bias)):
        _capi.check(lib.bt709hip_decoder_set_option(dec, _capi.OPT_CHW_SCALE_R + i, int(np.array([v], np.float32).view(np.int32)[0])))
    f_size = C.sizeof(_capi.Frame)
    counts = instruction_counts()
    lines, results = [], {}

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit("# tools/bench_scaled_chw.py: %s, %d rounds of interleaved legs, regions >= %.0f ms; us per frame: median [min .. max] max/min"
         % ((ctx.info().name or ctx.info().arch).decode(), args.rounds, args.region_ms))
    for (W, H), (OW, OH), n in SHAPES:
        ring = 2 * n if n > 1 else 8
        slot = W * H * 3 // 2
        slab_in = DeviceBuffer(ctx, ring * slot, 1)
        rng = np.random.default_rng(0xC5)
        for i in range(min(ring, 4)):
            host = rng.integers(0, 256, slot, dtype=np.uint8)
            _capi.check(lib.bt709hip_upload(h, slab_in.ptr + i * slot, slot, host.ctypes.data, slot, slot, 1, None))
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for i in range(4, ring, 4):
            _capi.check(lib.bt709hip_copy_probe(h, slab_in.ptr + i * slot, slab_in.ptr, min(4, ring - i) * slot, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        frames = (_capi.Frame * ring)(*[_capi.Frame(slab_in.ptr + i * slot, W, slab_in.ptr + i * slot + W * H, W, W, H, 1, 1) for i in range(ring)])
        out_pitch = 12 * OW * OH  # the widest view: three planes of binary32
        slab_out = DeviceBuffer(ctx, n * out_pitch, 1)
        surfs = {name: (_capi.Surface * n)(*[_capi.Surface(slab_out.ptr + k * out_pitch, OW * e, OW, OH, fmt, 0) for k in range(n)]) for name, fmt, e in ELEMS}
        surfs["bgra8"] = (_capi.Surface * n)(*[_capi.Surface(slab_out.ptr + k * out_pitch, OW * 4, OW, OH, _capi.FORMAT_BGRA8_SRGB, 0) for k in range(n)])

        def rescale(target, i, wait=0):
            _capi.check(lib.bt709hip_decode_scaled_batch(dec, n, C.cast(C.byref(frames, i * f_size), C.POINTER(_capi.Frame)), None, target, stream, wait))

        # what is timed computes the definition: view 0 into CHW_F32 against the BGRA8 view of the same frame
        rescale(surfs["bgra8"], 0, 1)
        words = np.empty((OH, OW), np.uint32)
        _capi.check(lib.bt709hip_download(h, words.ctypes.data, OW * 4, slab_out.ptr, OW * 4, OW * 4, OH, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        rescale(surfs["f32"], 0, 1)
        planes = np.empty((3, OH, OW), np.float32)
        _capi.check(lib.bt709hip_download(h, planes.ctypes.data, OW * 4, slab_out.ptr, OW * 4, OW * 4, 3 * OH, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for c in range(3):
            v = ((words >> np.uint32(16 - 8 * c)) & np.uint32(0xFF)).astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
            assert np.array_equal(planes[c], v * scale[c] + bias[c]), "%dx%d -> %dx%d: CHW_F32 plane %d is not the definition" % (W, H, OW, OH, c)

        state = {"i": 0}

        def window():
            i = state["i"]
            state["i"] = (i + n) % ring if i + 2 * n <= ring else 0
            return i

        legs = [("bgra8", lambda: rescale(surfs["bgra8"], window()))]
        for name, fmt, e in ELEMS:
            legs.append(("chw_" + name, lambda name=name: rescale(surfs[name], window())))
        if torch is not None:
            dev = "cuda:%d" % ctx.device
            bgra = torch.empty((n, OH, OW, 4), dtype=torch.uint8, device=dev)
            tsurfs = (_capi.Surface * n)(*[_capi.Surface(bgra[k].data_ptr(), OW * 4, OW, OH, _capi.FORMAT_BGRA8_SRGB, 0) for k in range(n)])
            for name, dtype in (("u8", torch.uint8), ("f16", torch.float16), ("f32", torch.float32)):
                out = torch.empty((n, 3, OH, OW), dtype=dtype, device=dev)
                kind = dtype if dtype != torch.uint8 else torch.float32
                mul = torch.tensor(scale / np.float32(255.0), dtype=torch.float32, device=dev).to(kind).view(1, 3, 1, 1)
                add = torch.tensor(bias, dtype=torch.float32, device=dev).to(kind).view(1, 3, 1, 1)

                def lean(out=out, mul=mul, add=add, dtype=dtype):
                    rescale(tsurfs, window())
                    for c in range(3):
                        out[:, c].copy_(bgra[..., 2 - c])
                    if dtype != torch.uint8:
                        out.mul_(mul).add_(add)
                legs.append(("lean_" + name, lean))

        reps, kernels, taps = {}, {}, {}
        for name, step in legs:  # untimed: code objects, clocks, and the repeat count of a region
            for _ in range(3):
                step()
            _capi.check(lib.bt709hip_stream_synchronize(h, stream))
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
        emit("%dx%d -> %dx%d, %d per launch (tap form %s)" % (W, H, OW, OH, n, taps["bgra8"]))
        for name, _ in legs:
            s = sorted(samples[name])
            row[name] = {"us_per_frame": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3), "max_over_min": round(s[-1] / s[0], 4),
                         "kernel": kernels[name], "reps": reps[name]}
            emit("  %-9s %9.3f [%9.3f .. %9.3f] %.3f  %s" % (name, row[name]["us_per_frame"], s[0], s[-1], s[-1] / s[0], kernels[name] if not name.startswith("lean") else "(b) + copy_ x 3 + mul_ + add_"))
        med = lambda name: row[name]["us_per_frame"]
        for k, (name, fmt, e) in enumerate(ELEMS):
            leg = "chw_" + name
            pred = predicted(counts, taps[leg], k + 1)
            ratios = {"a_over_b": med(leg) / med("bgra8")}
            text = "  %s: (a) / (b) %.3f (instruction counts predict %s)" % (leg, ratios["a_over_b"], "%.3f" % pred if pred else "n/a: no assembly here")
            if "lean_" + name in row:
                ratios["c_over_a"] = med("lean_" + name) / med(leg)
                ratios["noise"] = max(row[leg]["max_over_min"], row["lean_" + name]["max_over_min"])
                row[leg]["faster_than_two_pass"] = bool(ratios["c_over_a"] > ratios["noise"])
                text += "  (c) / (a) %.3f against the legs' spread %.3f: %s" % (ratios["c_over_a"], ratios["noise"], "FASTER" if row[leg]["faster_than_two_pass"] else "NOT faster")
            row[leg]["ratios"] = {k2: round(v, 4) for k2, v in ratios.items()}
            emit(text)
        emit("  chw_u8 / chw_f16 %.3f" % (med("chw_u8") / med("chw_f16")))
        results["%dx%d->%dx%d/%d" % (W, H, OW, OH, n)] = row
        slab_in.free()
        slab_out.free()
    lib.bt709hip_decoder_destroy(dec)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"workload": "fused decode + rescale of resident frames into BGRA8 and the three planar CHW formats, same frames, same slabs", "legs": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
