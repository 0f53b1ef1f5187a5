#!/usr/bin/env python3
"""The planar CHW decode targets (BT709HIP_FORMAT_CHW_U8 / _F16 / _F32) against their yardsticks, in ONE process
over the SAME resident pictures and the SAME two slabs (placement cancels):

    bgra8       the BGRA8 decode                                    1.5 + 4 B per pixel   (its kernels are the parent commit's,
    rgba16f     the RGBA16F decode                                  1.5 + 8               instruction for instruction:
                                                                                          profiles/r21_chw_isa.txt)
    chw_u8      planes of bytes                                     1.5 + 3
    chw_f16     planes of binary16, scaled and normalised           1.5 + 6
    chw_f32     planes of binary32, scaled and normalised           1.5 + 12
    copy@B      bt709hip_copy_probe moving B bytes per pixel in all (half read, half written), for each B above
    torch_*     the two-pass route a torch caller runs without the formats, if torch imports: the BGRA8 decode into a uint8
                tensor, then x[..., :3].flip(-1) (drops A, swaps B and R: a copy), one copy_ that transposes and converts into
                a preallocated NCHW tensor, and for the float types mul_ and add_ in place with 1/255 folded into the scale;
                on torch's current stream, like the decode in front of it
    lean_*      the same route written for speed: one strided copy_ per channel in place of flip + copy_, then mul_ / add_
                (neither is a hand-written second pass; the copy legs bound what one could reach)

A ring of --ring 4K frames; a launch covers N = 32 or 1 consecutive slots and successive launches walk the ring.  Per N the legs
are interleaved and the round repeated --rounds times, each sample a region of >= --region-ms between two HIP events; the table
gives every leg's median and its own max / min, and each CHW leg's ratio to bgra8, rgba16f, the copy of its bytes and the two-pass
route beside what the byte counts predict.  Not the headline bench (that is bench.py).

    python tools/bench_chw.py [--sizes 3840x2160] [--counts 32,1] [--out profiles/r21_chw.txt]
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
OUT_BYTES = {"bgra8": 4, "rgba16f": 8, "chw_u8": 3, "chw_f16": 6, "chw_f32": 12}
FORMAT = {"bgra8": _capi.FORMAT_BGRA8_SRGB, "rgba16f": _capi.FORMAT_RGBA16F, "chw_u8": _capi.FORMAT_CHW_U8, "chw_f16": _capi.FORMAT_CHW_F16,
          "chw_f32": _capi.FORMAT_CHW_F32}
ROW_BYTES = {"bgra8": 4, "rgba16f": 8, "chw_u8": 1, "chw_f16": 2, "chw_f32": 4}  # per pixel of a row: the surface's pitch / W
PREDICTED = {("chw_u8", "bgra8"): 4.5 / 5.5, ("chw_f16", "bgra8"): 7.5 / 5.5, ("chw_f32", "bgra8"): 13.5 / 5.5, ("chw_f16", "rgba16f"): 7.5 / 9.5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=64, help="frames resident in HBM")
    ap.add_argument("--sizes", default="3840x2160")
    ap.add_argument("--counts", default="32,1", help="frames per launch")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved repeats of the legs")
    ap.add_argument("--region-ms", type=float, default=60.0, help="least length of a timed region")
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
            print("# torch legs left out: %s" % (exc,), flush=True)
            torch = None
    ctx = mb.MetalRenderContext(0)
    assert ctx.setupMetal()
    lib, h = ctx.lib, ctx.handle
    # every leg on ONE stream: the context's, or -- with torch -- a stream of torch's made current (its default stream is the null
    # handle, which the library reads as "the context's own stream")
    stream = None
    if torch is not None:
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
    _capi.check(lib.bt709hip_decoder_prepare_format(dec, _capi.FORMAT_RGBA16F))
    scale = np.float32(1.0) / np.array(STD, np.float32)
    bias = -np.array(MEAN, np.float32) / np.array(STD, np.float32)
    for i, v in enumerate(list(scale) + list(bias)):
        _capi.check(lib.bt709hip_decoder_set_option(dec, _capi.OPT_CHW_SCALE_R + i, int(np.array([v], np.float32).view(np.int32)[0])))
    f_size, s_size = C.sizeof(_capi.Frame), C.sizeof(_capi.Surface)
    lines, results = [], {}

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit("# tools/bench_chw.py: %s, ring %d, %d rounds of interleaved legs, regions >= %.0f ms; us per frame: median [min .. max] max/min"
         % ((ctx.info().name or ctx.info().arch).decode(), args.ring, args.rounds, args.region_ms))
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        ring = args.ring
        slot, out_pitch = W * H * 3 // 2, 12 * W * H  # the widest target: three planes of binary32
        slab_in, slab_out = DeviceBuffer(ctx, ring * slot, 1), DeviceBuffer(ctx, ring * out_pitch, 1)
        slab_copy = DeviceBuffer(ctx, max(int(c) for c in args.counts.split(",")) * W * H * 7, 1)  # the copy legs' source: up to 13.5 / 2 B per pixel
        rng = np.random.default_rng(0xC4)
        distinct = min(ring, 4)
        for i in range(distinct):
            host = rng.integers(0, 256, slot, dtype=np.uint8)
            _capi.check(lib.bt709hip_upload(h, slab_in.ptr + i * slot, slot, host.ctypes.data, slot, slot, 1, None))
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for i in range(distinct, ring, distinct):
            _capi.check(lib.bt709hip_copy_probe(h, slab_in.ptr + i * slot, slab_in.ptr, min(distinct, ring - i) * slot, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        frames = (_capi.Frame * ring)(*[_capi.Frame(slab_in.ptr + i * slot, W, slab_in.ptr + i * slot + W * H, W, W, H, 1, 1) for i in range(ring)])
        surfs = {leg: (_capi.Surface * ring)(*[_capi.Surface(slab_out.ptr + i * out_pitch, W * ROW_BYTES[leg], W, H, FORMAT[leg], 0) for i in range(ring)])
                 for leg in FORMAT}

        # what is timed computes the definition: slot 0 into CHW_F32 against the BGRA8 decode of the same frame
        _capi.check(lib.bt709hip_decode_batch(dec, 1, frames, None, surfs["bgra8"], None, 1))
        words = np.empty((H, W), np.uint32)
        _capi.check(lib.bt709hip_download(h, words.ctypes.data, W * 4, slab_out.ptr, W * 4, W * 4, H, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        _capi.check(lib.bt709hip_decode_batch(dec, 1, frames, None, surfs["chw_f32"], None, 1))
        planes = np.empty((3, H, W), np.float32)
        _capi.check(lib.bt709hip_download(h, planes.ctypes.data, W * 4, slab_out.ptr, W * 4, W * 4, 3 * H, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for c in range(3):
            v = ((words >> np.uint32(16 - 8 * c)) & np.uint32(0xFF)).astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
            assert np.array_equal(planes[c], v * scale[c] + bias[c]), "%dx%d: CHW_F32 plane %d is not the definition" % (W, H, c)

        for n in (int(v) for v in args.counts.split(",")):
            if n > ring:
                continue
            state = {"i": 0}

            def window():
                i = state["i"]
                state["i"] = (i + n) % ring if i + 2 * n <= ring else 0
                return i

            def decode_leg(leg):
                def step():
                    i = window()
                    _capi.check(lib.bt709hip_decode_batch(dec, n, C.cast(C.byref(frames, i * f_size), C.POINTER(_capi.Frame)), None,
                                                          C.cast(C.byref(surfs[leg], i * s_size), C.POINTER(_capi.Surface)), stream, 0))
                return step

            def copy_leg(per_pixel):
                nbytes = int(n * W * H * per_pixel / 2) // 16 * 16  # half read, half written: into the window a decode would write

                def step():
                    _capi.check(lib.bt709hip_copy_probe(h, slab_out.ptr + window() * out_pitch, slab_copy.ptr, nbytes, stream))
                return step

            legs = [(leg, decode_leg(leg)) for leg in ("bgra8", "rgba16f", "chw_u8", "chw_f16", "chw_f32")]
            legs += [("copy@%.1f" % b, copy_leg(b)) for b in (4.5, 5.5, 7.5, 9.5, 13.5)]
            if torch is not None:
                dev = "cuda:%d" % ctx.device
                bgra = torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev)
                tsurfs = (_capi.Surface * n)(*[_capi.Surface(bgra[k].data_ptr(), W * 4, W, H, _capi.FORMAT_BGRA8_SRGB, 0) for k in range(n)])
                for name, dtype in (("torch_u8", torch.uint8), ("torch_f16", torch.float16), ("torch_f32", torch.float32)):
                    out = torch.empty((n, 3, H, W), dtype=dtype, device=dev)
                    mul = torch.tensor(scale / np.float32(255.0), dtype=torch.float32, device=dev).to(dtype if dtype != torch.uint8 else torch.float32).view(1, 3, 1, 1)
                    add = torch.tensor(bias, dtype=torch.float32, device=dev).to(dtype if dtype != torch.uint8 else torch.float32).view(1, 3, 1, 1)

                    def step(out=out, mul=mul, add=add, dtype=dtype):
                        i = window()
                        _capi.check(lib.bt709hip_decode_batch(dec, n, C.cast(C.byref(frames, i * f_size), C.POINTER(_capi.Frame)), None, tsurfs, stream, 0))
                        out.copy_(bgra[..., :3].flip(-1).permute(0, 3, 1, 2))
                        if dtype != torch.uint8:
                            out.mul_(mul).add_(add)
                    legs.append((name, step))

                    # the same route written for speed: one strided copy_ per channel (drops A, swaps B and R, transposes and
                    # converts in one pass over the words' lines), then the fused scale and the bias in place
                    def lean(out=out, mul=mul, add=add, dtype=dtype):
                        i = window()
                        _capi.check(lib.bt709hip_decode_batch(dec, n, C.cast(C.byref(frames, i * f_size), C.POINTER(_capi.Frame)), None, tsurfs, stream, 0))
                        for c in range(3):
                            out[:, c].copy_(bgra[..., 2 - c])
                        if dtype != torch.uint8:
                            out.mul_(mul).add_(add)
                    legs.append((name.replace("torch_", "lean_"), lean))

            reps, kernels = {}, {}
            for name, step in legs:  # untimed: code objects, clocks, and the repeat count of a region
                for _ in range(3):
                    step()
                _capi.check(lib.bt709hip_stream_synchronize(h, stream))
                kernels[name] = lib.bt709hip_last_kernel_name().decode()
                reps[name] = max(2, int(np.ceil(args.region_ms * 1.3 / max(region(step, 4) / 4, 1e-3))))
            samples = {name: [] for name, _ in legs}
            for _ in range(args.rounds):
                for name, step in legs:
                    samples[name].append(region(step, reps[name]) * 1e3 / (reps[name] * n))
            row = {}
            emit("%dx%d, %d per launch" % (W, H, n))
            for name, _ in legs:
                s = sorted(samples[name])
                row[name] = {"us_per_frame": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3), "max_over_min": round(s[-1] / s[0], 4),
                             "kernel": kernels[name], "reps": reps[name]}
                emit("  %-10s %9.3f [%9.3f .. %9.3f] %.3f  %s" % (name, row[name]["us_per_frame"], s[0], s[-1], s[-1] / s[0], kernels[name] if not name.startswith("copy") else ""))
            med = lambda name: row[name]["us_per_frame"]
            for leg in ("chw_u8", "chw_f16", "chw_f32"):
                ratios = {"bgra8": med(leg) / med("bgra8"), "rgba16f": med(leg) / med("rgba16f"), "copy": med(leg) / med("copy@%.1f" % (1.5 + OUT_BYTES[leg]))}
                text = "  %s: x bgra8 %.3f (bytes predict %.2f)  x rgba16f %.3f%s  x copy of its bytes %.3f" % (
                    leg, ratios["bgra8"], PREDICTED[(leg, "bgra8")], ratios["rgba16f"],
                    " (bytes predict %.2f)" % PREDICTED[(leg, "rgba16f")] if (leg, "rgba16f") in PREDICTED else "", ratios["copy"])
                two_pass = "torch_" + leg[4:]
                if two_pass in row:
                    ratios["two_pass"] = med(leg) / med(two_pass)
                    ratios["two_pass_lean"] = med(leg) / med("lean_" + leg[4:])
                    text += "  x two-pass route %.3f  x its per-channel form %.3f" % (ratios["two_pass"], ratios["two_pass_lean"])
                row[leg]["ratios"] = {k: round(v, 4) for k, v in ratios.items()}
                emit(text)
            results["%dx%d/%d" % (W, H, n)] = row
        slab_in.free()
        slab_out.free()
        slab_copy.free()
    lib.bt709hip_decoder_destroy(dec)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"workload": "1:1 decode of resident 4K frames into BGRA8, RGBA16F and the three planar CHW formats, same pictures, same slabs",
                      "legs": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
