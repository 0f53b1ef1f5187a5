// CDNA4 (gfx950) kernels of the 1:1 decode over PLANAR 4:2:0 chroma (I420: the YUV4MPEG2 C420jpeg payload, Y then U then V,
// Renderer/y4m_writer.h:194-241; a software decoder's yuv420p) -- BT709HIP_OPT_CHROMA_LAYOUT = BT709HIP_CHROMA_I420.
//
// Pixel (x, y) takes Y[y][x], U[y/2][x/2], V[y/2][x/2]; the output is byte for byte what the NV12 kernels (bt709_kernels.hip)
// write for the interleaved twin of the planes.  The arithmetic IS theirs (bt709_decode_body.h: decode_quad, decode_block,
// over_quad, over_pixel and the fast kernels' body); what is new here is the front end -- which chroma bytes reach which
// pixel.  Same traffic as NV12, 1.5 B read + 4 B written per pixel, where "interleave the planes, then decode" moves 6.5 B in
// two launches.
//   * fast path (decode_i420_quads*): the NV12 fast kernels' shape -- a lane owns kQuadsPerLane 4x2 quads of one row pair,
//     consecutive lanes consecutive quads, straight-line (loads, table, pin, arithmetic, predicated 16-byte stores).  A quad's
//     chroma is a 2-byte load from each plane and one v_perm_b32 (bt709_tile.h TileInI420): one VMEM instruction per quad more
//     than NV12, chroma planes only 2-byte aligned.
//   * general path (decode_i420_blocks*): one lane per 2x2 block, byte loads of U and V, the grid-strided walk of
//     decode_nv12_blocks; any even size, any pitch, any alignment of the input planes.
// Launch plans (tiles, XCD bands, the banded part plus a plain tail) are launch_decode's: it calls launch_decode_i420 below with
// the grid it planned and recorded.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bt709_decode_body.h"
#include "bt709_launch.h"

namespace bt709 {

// ---------------------------------------------------------------------------
// Fast path.  Preconditions (checked by the host shim): width % 4 == 0; y and alpha pointers and strides 4-byte aligned; the U
// pointer and the chroma pitch 2-byte aligned (v_offset = (H/2) x pitch then is, too); output pointer and stride 16-byte aligned.
// ---------------------------------------------------------------------------
template <bool HAS_ALPHA, bool NT, bool QUANT>
__global__ void __launch_bounds__(kMaxBlockThreads)
decode_i420_quads(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  quads_body<HAS_ALPHA, NT, QUANT, false, kOverOff, TileInI420>(p, lds_raw);
}

// log-bucket table (the LINEAR mode): decode_nv12_quads_log's twin
template <bool NT>
__global__ void __launch_bounds__(kMaxBlockThreads)
decode_i420_quads_log(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  quads_body<false, NT, false, true, kOverOff, TileInI420>(p, lds_raw);
}

// BT709HIP_OPT_COMPOSITE_OVER: decode_nv12_quads_over's twin
template <int OVER>
__global__ void __launch_bounds__(kMaxBlockThreads)
decode_i420_quads_over(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  quads_body<true, true, true, false, OVER, TileInI420>(p, lds_raw);
}

// ---------------------------------------------------------------------------
// General path: any even width / height, any pitch, byte-aligned planes, 4-byte aligned output.  Block bx of row pair rp reads
// U[rp][bx] and V[rp][bx], bx < W/2: inside the row's W/2 bytes of either plane.
// ---------------------------------------------------------------------------
template <bool HAS_ALPHA, bool QUANT>
__global__ void __launch_bounds__(kBlockThreads)
decode_i420_blocks(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  if (!QUANT) {
    stage_table(lds_raw, p.table_unit, p.table_unit_bytes);
    __syncthreads();
  }

  const UnitLookup ul = unit_lookup(p, lds_raw);
  const FramePlanes f = frame_planes(p, blockIdx.y);
  const uint32_t bw = p.width >> 1;
  const uint32_t row_pairs = p.height >> 1;

  for (uint32_t rp = blockIdx.x; rp < row_pairs; rp += gridDim.x) {
    const uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    const uint8_t *y1 = y0 + p.y_stride;
    const uint8_t *uu = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;
    const uint8_t *vv = uu + p.v_offset;
    uint32_t *o0 = reinterpret_cast<uint32_t *>(f.out + static_cast<size_t>(2 * rp) * p.out_stride);
    uint32_t *o1 = reinterpret_cast<uint32_t *>(f.out + static_cast<size_t>(2 * rp + 1) * p.out_stride);
    for (uint32_t bx = threadIdx.x; bx < bw; bx += kBlockThreads) {
      const float y[4] = {byte_value(y0[2 * bx]), byte_value(y0[2 * bx + 1]), byte_value(y1[2 * bx]),
                          byte_value(y1[2 * bx + 1])};
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      if (HAS_ALPHA) {
        const uint8_t *a0 = f.alpha + static_cast<size_t>(2 * rp) * p.alpha_stride;
        const uint8_t *a1 = a0 + p.alpha_stride;
        a[0] = byte_value(a0[2 * bx]);
        a[1] = byte_value(a0[2 * bx + 1]);
        a[2] = byte_value(a1[2 * bx]);
        a[3] = byte_value(a1[2 * bx + 1]);
      }
      uint32_t out[4];
      decode_block<HAS_ALPHA, QUANT>(ul, y, byte_value(uu[bx]), byte_value(vv[bx]), a, p.alpha_word, out);
      o0[2 * bx] = out[0];
      o0[2 * bx + 1] = out[1];
      o1[2 * bx] = out[2];
      o1[2 * bx + 1] = out[3];
    }
  }
}

// BT709HIP_OPT_COMPOSITE_OVER: decode_nv12_blocks_over's twin
template <int OVER>
__global__ void __launch_bounds__(kBlockThreads)
decode_i420_blocks_over(const DecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const OverLookup ol = stage_over_tables(lds_raw, p);
  __syncthreads();

  const FramePlanes f = frame_planes(p, blockIdx.y);
  const uint32_t bw = p.width >> 1;
  const uint32_t row_pairs = p.height >> 1;

  for (uint32_t rp = blockIdx.x; rp < row_pairs; rp += gridDim.x) {
    const uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    const uint8_t *y1 = y0 + p.y_stride;
    const uint8_t *a0 = f.alpha + static_cast<size_t>(2 * rp) * p.alpha_stride;
    const uint8_t *a1 = a0 + p.alpha_stride;
    const uint8_t *uu = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;
    const uint8_t *vv = uu + p.v_offset;
    uint32_t *o0 = reinterpret_cast<uint32_t *>(f.out + static_cast<size_t>(2 * rp) * p.out_stride);
    uint32_t *o1 = reinterpret_cast<uint32_t *>(f.out + static_cast<size_t>(2 * rp + 1) * p.out_stride);
    for (uint32_t bx = threadIdx.x; bx < bw; bx += kBlockThreads) {
      const float y[4] = {byte_value(y0[2 * bx]), byte_value(y0[2 * bx + 1]), byte_value(y1[2 * bx]), byte_value(y1[2 * bx + 1])};
      const float a[4] = {byte_value(a0[2 * bx]), byte_value(a0[2 * bx + 1]), byte_value(a1[2 * bx]), byte_value(a1[2 * bx + 1])};
      uint32_t bg[4] = {0u, 0u, 0u, 0u};
      if (OVER == kOverDestination) bg[0] = o0[2 * bx], bg[1] = o0[2 * bx + 1], bg[2] = o1[2 * bx], bg[3] = o1[2 * bx + 1];
      const Chroma c = chroma_terms(byte_value(uu[bx]), byte_value(vv[bx]));
      uint32_t out[4];
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        float x[3];
        pixel_rgb(y[px], c, x[0], x[1], x[2]);
        out[px] = over_pixel<OVER>(ol, p.over_lin, x, a[px], bg[px]);
      }
      o0[2 * bx] = out[0];
      o0[2 * bx + 1] = out[1];
      o1[2 * bx] = out[2];
      o1[2 * bx + 1] = out[3];
    }
  }
}

// The kernel selection of launch_decode (bt709_kernels.hip), over the twins above.
const char *launch_decode_i420(const DecodeParams &p, const dim3 &grid, const dim3 &block, size_t lds, int variant, uint32_t over,
                               bool has_alpha, bool quant, bool nontemporal, hipStream_t stream) {
  if (variant == kVariantQuads) {
    if (over == kOverDestination) {
      hipLaunchKernelGGL((decode_i420_quads_over<kOverDestination>), grid, block, lds, stream, p);
      return "decode_i420_quads<alpha,over>";
    }
    if (over != kOverOff) {
      hipLaunchKernelGGL((decode_i420_quads_over<kOverColour>), grid, block, lds, stream, p);
      return "decode_i420_quads<alpha,over-colour>";
    }
    if (has_alpha) {
      hipLaunchKernelGGL((decode_i420_quads<true, true, true>), grid, block, lds, stream, p);
      return "decode_i420_quads<alpha>";
    }
    if (quant) {
      if (nontemporal) hipLaunchKernelGGL((decode_i420_quads<false, true, true>), grid, block, lds, stream, p);
      else hipLaunchKernelGGL((decode_i420_quads<false, false, true>), grid, block, lds, stream, p);
      return nontemporal ? "decode_i420_quads<nt,quantiser>" : "decode_i420_quads<quantiser>";
    }
    if (p.unit1_shift != 0) {  // log-bucket table (the LINEAR mode)
      if (nontemporal) hipLaunchKernelGGL((decode_i420_quads_log<true>), grid, block, lds, stream, p);
      else hipLaunchKernelGGL((decode_i420_quads_log<false>), grid, block, lds, stream, p);
      return nontemporal ? "decode_i420_quads_log<nt>" : "decode_i420_quads_log";
    }
    if (nontemporal) {
      hipLaunchKernelGGL((decode_i420_quads<false, true, false>), grid, block, lds, stream, p);
      return "decode_i420_quads<nt>";
    }
    hipLaunchKernelGGL((decode_i420_quads<false, false, false>), grid, block, lds, stream, p);
    return "decode_i420_quads";
  }
  if (over == kOverDestination) {
    hipLaunchKernelGGL((decode_i420_blocks_over<kOverDestination>), grid, block, lds, stream, p);
    return "decode_i420_blocks<alpha,over>";
  }
  if (over != kOverOff) {
    hipLaunchKernelGGL((decode_i420_blocks_over<kOverColour>), grid, block, lds, stream, p);
    return "decode_i420_blocks<alpha,over-colour>";
  }
  if (has_alpha) {
    hipLaunchKernelGGL((decode_i420_blocks<true, true>), grid, block, lds, stream, p);
    return "decode_i420_blocks<alpha>";
  }
  if (quant) {
    hipLaunchKernelGGL((decode_i420_blocks<false, true>), grid, block, lds, stream, p);
    return "decode_i420_blocks<quantiser>";
  }
  hipLaunchKernelGGL((decode_i420_blocks<false, false>), grid, block, lds, stream, p);
  return "decode_i420_blocks";
}

// the table kernels' dynamic-LDS cap, as prepare_kernels raises the NV12 twins'
hipError_t prepare_planar_kernels() {
  const void *fns[] = {
      reinterpret_cast<const void *>(&decode_i420_quads<false, true, false>),
      reinterpret_cast<const void *>(&decode_i420_quads<false, false, false>),
      reinterpret_cast<const void *>(&decode_i420_quads_log<true>),
      reinterpret_cast<const void *>(&decode_i420_quads_log<false>),
      reinterpret_cast<const void *>(&decode_i420_blocks<false, false>),
  };
  return raise_lds_cap(fns, kRepLdsBytes);
}

}  // namespace bt709
