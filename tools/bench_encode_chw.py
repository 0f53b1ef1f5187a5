#!/usr/bin/env python3
"""Planar CHW encoder input (BT709HIP_CTX_OPT_ENCODE_CHW_INPUT) against its yardsticks, in ONE process over the SAME
resident pictures and the SAME slabs (placement cancels):

    bgra8[_i420]     the BGRA8 encode of the same pictures               4 + 1.5 B per pixel   (its kernels are the parent commit's,
                                                                                               instruction for instruction:
                                                                                               profiles/r22_encode_chw_isa.txt)
    chw_u8[_i420]    planes of bytes                                     3 + 1.5
    chw_f16[_i420]   planes of binary16, ImageNet-normalised             6 + 1.5
    chw_f32[_i420]   planes of binary32, ImageNet-normalised             12 + 1.5
    copy@B           bt709hip_copy_probe moving B bytes per pixel in all (half read, half written), for each B above
    torch_*          the two-pass route a torch caller writes today, if torch imports: x * std + mean, clamp, * 255, round, to uint8
                     (floats), permute to HWC, an alpha channel appended, flipped to B, G, R, A -- then bt709hip_encode_batch of the
                     BGRA8 tensor; on torch's current stream, like the encode behind it
    lean_*           the same route written for speed: one strided copy_ per channel into a preallocated BGRA8 tensor whose alpha is
                     set once (floats: the de-normalisation in place on a scratch tensor first), then the encode

A ring of --ring 4K pictures; a launch covers N = 32 or 1 consecutive slots and successive launches walk the ring.  Per N the legs
are interleaved and the round repeated --rounds times, each sample a region of >= --region-ms between two HIP events; the table
gives every leg's median and its own max / min, and each CHW leg's ratio to bgra8, the copy of its bytes and the two-pass route
beside what the byte counts predict.  Before anything is timed the frames of slot 0 from each CHW leg are held to the BGRA8 encode's
(the tensors hold the normalised bytes of the BGRA8 pictures).  Not the headline bench (that is bench.py).

    python tools/bench_encode_chw.py [--sizes 3840x2160] [--counts 32,1] [--out profiles/r22_encode_chw.txt]
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
IN_BYTES = {"bgra8": 4, "chw_u8": 3, "chw_f16": 6, "chw_f32": 12}
FORMAT = {"bgra8": _capi.FORMAT_BGRA8_SRGB, "chw_u8": _capi.FORMAT_CHW_U8, "chw_f16": _capi.FORMAT_CHW_F16, "chw_f32": _capi.FORMAT_CHW_F32}
ROW_BYTES = {"bgra8": 4, "chw_u8": 1, "chw_f16": 2, "chw_f32": 4}  # per pixel of a row: the surface's pitch / W
DTYPE = {"chw_u8": np.uint8, "chw_f16": np.float16, "chw_f32": np.float32}
PREDICTED = {"chw_u8": 4.5 / 5.5, "chw_f16": 7.5 / 5.5, "chw_f32": 13.5 / 5.5}
SRGB, APPLE = 1, 0


def bits(v):
    return int(np.array([v], np.float32).view(np.int32)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=64, help="pictures resident in HBM")
    ap.add_argument("--sizes", default="3840x2160")
    ap.add_argument("--counts", default="32,1", help="pictures per launch")
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

    def option(o, v):
        _capi.check(lib.bt709hip_context_set_option(h, o, v))

    _capi.check(lib.bt709hip_encoder_prepare(h, SRGB, APPLE))
    std, mean = np.array(STD, np.float32), np.array(MEAN, np.float32)
    for i, v in enumerate(list(std) + list(mean)):  # the encoder holds (std, mean): the inverse of the decode's (1 / std, -mean / std)
        option(_capi.CTX_OPT_ENCODE_CHW_SCALE_R + i, bits(v))
    option(_capi.CTX_OPT_ENCODE_CHW_INPUT, 1)
    f_size, s_size = C.sizeof(_capi.Frame), C.sizeof(_capi.Surface)
    lines, results = [], {}

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit("# tools/bench_encode_chw.py: %s, ring %d, %d rounds of interleaved legs, regions >= %.0f ms; us per picture: median [min .. max] max/min"
         % ((ctx.info().name or ctx.info().arch).decode(), args.ring, args.rounds, args.region_ms))
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        ring, px = args.ring, W * H
        out_slot = px * 3 // 2
        slabs = {leg: DeviceBuffer(ctx, ring * IN_BYTES[leg] * px, 1) for leg in IN_BYTES}
        slab_out = DeviceBuffer(ctx, ring * out_slot, 1)
        slab_copy = DeviceBuffer(ctx, max(int(c) for c in args.counts.split(",")) * px * 7, 1)  # the copy legs' source: up to 13.5 / 2 B per pixel
        rng = np.random.default_rng(0xC5)
        distinct = min(ring, 2)
        for i in range(distinct):  # the same picture in all four forms: the tensors hold the (normalised) bytes of the BGRA8 words
            rgb = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
            words = np.uint32(0xFF000000) | (rgb[0].astype(np.uint32) << np.uint32(16)) | (rgb[1].astype(np.uint32) << np.uint32(8)) | rgb[2]
            forms = {"bgra8": words, "chw_u8": rgb}
            t = rgb.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
            t = t * (np.float32(1.0) / std).reshape(3, 1, 1) + (-mean / std).reshape(3, 1, 1)  # the decode side's recipe
            forms["chw_f32"], forms["chw_f16"] = t, t.astype(np.float16)
            for leg, arr in forms.items():
                raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
                nbytes, piece = raw.size, 1 << 24
                for o in range(0, nbytes, piece):
                    n_ = min(piece, nbytes - o)
                    _capi.check(lib.bt709hip_upload(h, slabs[leg].ptr + i * nbytes + o, n_, raw.ctypes.data + o, n_, n_, 1, None))
                _capi.check(lib.bt709hip_stream_synchronize(h, None))
        for leg in IN_BYTES:
            nbytes = IN_BYTES[leg] * px
            for i in range(distinct, ring, distinct):
                _capi.check(lib.bt709hip_copy_probe(h, slabs[leg].ptr + i * nbytes, slabs[leg].ptr, min(distinct, ring - i) * nbytes, None))
        _capi.check(lib.bt709hip_stream_synchronize(h, None))
        surfs = {leg: (_capi.Surface * ring)(*[_capi.Surface(slabs[leg].ptr + i * IN_BYTES[leg] * px, W * ROW_BYTES[leg], W, H, FORMAT[leg], 0) for i in range(ring)])
                 for leg in IN_BYTES}
        frames = {0: (_capi.Frame * ring)(*[_capi.Frame(slab_out.ptr + i * out_slot, W, slab_out.ptr + i * out_slot + px, W, W, H, 0, 0) for i in range(ring)]),
                  1: (_capi.Frame * ring)(*[_capi.Frame(slab_out.ptr + i * out_slot, W, slab_out.ptr + i * out_slot + px, W // 2, W, H, 0, 0) for i in range(ring)])}

        def frame_bytes():
            got = np.empty(out_slot, np.uint8)
            _capi.check(lib.bt709hip_download(h, got.ctypes.data, W, slab_out.ptr, W, W, out_slot // W, None))
            _capi.check(lib.bt709hip_stream_synchronize(h, None))
            return got

        # what is timed computes the definition: slot 0 from each tensor form against the BGRA8 encode of the same picture
        for layout in (0, 1):
            option(_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, layout)
            _capi.check(lib.bt709hip_encode_batch(h, 1, surfs["bgra8"], frames[layout], SRGB, APPLE, None, 1))
            want = frame_bytes()
            for leg in ("chw_u8", "chw_f16", "chw_f32"):
                _capi.check(lib.bt709hip_memset(h, slab_out.ptr, 0, out_slot, None))
                _capi.check(lib.bt709hip_encode_batch(h, 1, surfs[leg], frames[layout], SRGB, APPLE, None, 1))
                assert np.array_equal(frame_bytes(), want), "%dx%d: the %s encode is not the BGRA8 encode's frame (layout %d)" % (W, H, leg, layout)
        option(_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, 0)

        for n in (int(v) for v in args.counts.split(",")):
            if n > ring:
                continue
            state = {"i": 0}

            def window():
                i = state["i"]
                state["i"] = (i + n) % ring if i + 2 * n <= ring else 0
                return i

            def encode_leg(leg, layout):
                def step():
                    i = window()
                    option(_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, layout)
                    _capi.check(lib.bt709hip_encode_batch(h, n, C.cast(C.byref(surfs[leg], i * s_size), C.POINTER(_capi.Surface)),
                                                          C.cast(C.byref(frames[layout], i * f_size), C.POINTER(_capi.Frame)), SRGB, APPLE, stream, 0))
                return step

            def copy_leg(per_pixel):
                nbytes = int(n * px * per_pixel / 2) // 16 * 16  # half read, half written

                def step():
                    _capi.check(lib.bt709hip_copy_probe(h, slabs["chw_f32"].ptr + window() * 12 * px, slab_copy.ptr, nbytes, stream))
                return step

            legs = [(leg + ("_i420" if layout else ""), encode_leg(leg, layout)) for layout in (0, 1) for leg in ("bgra8", "chw_u8", "chw_f16", "chw_f32")]
            legs += [("copy@%.1f" % b, copy_leg(b)) for b in (4.5, 5.5, 7.5, 13.5)]
            if torch is not None:
                dev = "cuda:%d" % ctx.device
                bgra = torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev)
                bgra[..., 3] = 255
                tsurfs = (_capi.Surface * n)(*[_capi.Surface(bgra[k].data_ptr(), W * 4, W, H, _capi.FORMAT_BGRA8_SRGB, 0) for k in range(n)])
                alpha = torch.full((n, H, W, 1), 255, dtype=torch.uint8, device=dev)
                hold = []  # the tensors' surfaces, kept alive
                for leg, dtype in (("chw_u8", torch.uint8), ("chw_f16", torch.float16), ("chw_f32", torch.float32)):
                    src = torch.empty((n, 3, H, W), dtype=dtype, device=dev)
                    _capi.check(lib.bt709hip_copy_probe(h, src.data_ptr(), slabs[leg].ptr, n * IN_BYTES[leg] * px // 16 * 16, stream))
                    scratch = torch.empty_like(src)
                    mul = torch.tensor(std, dtype=torch.float32, device=dev).to(dtype if dtype != torch.uint8 else torch.float32).view(1, 3, 1, 1)
                    add = torch.tensor(mean, dtype=torch.float32, device=dev).to(dtype if dtype != torch.uint8 else torch.float32).view(1, 3, 1, 1)
                    hold.append((src, scratch, mul, add))

                    def encode_tensor(out):
                        tsurfs_ = tsurfs if out is bgra else (_capi.Surface * n)(*[_capi.Surface(out[k].data_ptr(), W * 4, W, H, _capi.FORMAT_BGRA8_SRGB, 0) for k in range(n)])
                        i = window()
                        option(_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, 0)
                        _capi.check(lib.bt709hip_encode_batch(h, n, tsurfs_, C.cast(C.byref(frames[0], i * f_size), C.POINTER(_capi.Frame)), SRGB, APPLE, stream, 0))

                    def step(src=src, mul=mul, add=add, dtype=dtype):  # as a caller writes it
                        x = src if dtype == torch.uint8 else (src * mul + add).clamp(0, 1).mul(255).round().to(torch.uint8)
                        out = torch.cat([x.permute(0, 2, 3, 1), alpha], dim=-1)[..., [2, 1, 0, 3]].contiguous()
                        encode_tensor(out)
                    legs.append(("torch_" + leg[4:], step))

                    def lean(src=src, scratch=scratch, mul=mul, add=add, dtype=dtype):  # written for speed
                        x = src
                        if dtype != torch.uint8:
                            torch.mul(src, mul, out=scratch)
                            x = scratch.add_(add).clamp_(0, 1).mul_(255).round_()
                        for c in range(3):
                            bgra[..., 2 - c].copy_(x[:, c])
                        encode_tensor(bgra)
                    legs.append(("lean_" + leg[4:], lean))

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
                row[name] = {"us_per_picture": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3), "max_over_min": round(s[-1] / s[0], 4),
                             "kernel": kernels[name], "reps": reps[name]}
                emit("  %-14s %9.3f [%9.3f .. %9.3f] %.3f  %s" % (name, row[name]["us_per_picture"], s[0], s[-1], s[-1] / s[0], kernels[name] if not name.startswith("copy") else ""))
            med = lambda name: row[name]["us_per_picture"]
            for leg in ("chw_u8", "chw_f16", "chw_f32"):
                for suffix in ("", "_i420"):
                    ratios = {"bgra8": med(leg + suffix) / med("bgra8" + suffix), "copy": med(leg + suffix) / med("copy@%.1f" % (1.5 + IN_BYTES[leg]))}
                    text = "  %s: x bgra8%s %.3f (bytes predict %.2f)  x copy of its bytes %.3f" % (leg + suffix, suffix, ratios["bgra8"], PREDICTED[leg], ratios["copy"])
                    if "torch_" + leg[4:] in row and not suffix:
                        ratios["two_pass"] = med(leg) / med("torch_" + leg[4:])
                        ratios["two_pass_lean"] = med(leg) / med("lean_" + leg[4:])
                        text += "  x two-pass route %.3f  x the route written for speed %.3f (its own max/min %.3f)" % (
                            ratios["two_pass"], ratios["two_pass_lean"], row["lean_" + leg[4:]]["max_over_min"])
                    row[leg + suffix]["ratios"] = {k: round(v, 4) for k, v in ratios.items()}
                    emit(text)
            results["%dx%d/%d" % (W, H, n)] = row
        for d in list(slabs.values()) + [slab_out, slab_copy]:
            d.free()
    option(_capi.CTX_OPT_ENCODE_CHROMA_LAYOUT, 0)
    option(_capi.CTX_OPT_ENCODE_CHW_INPUT, 0)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"workload": "encode of resident 4K pictures from BGRA8 and from the three planar CHW formats, same pictures, same slabs", "legs": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
