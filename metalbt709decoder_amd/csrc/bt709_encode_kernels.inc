// The encoder's four kernels, written once and compiled once per chroma layout: bt709_encode.hip includes this file with
//   BT709_ENCODE_LAYOUT                 kChromaNV12 / kChromaI420 (store_quad_chroma, store_block_chroma, quantize_quad)
//   BT709_ENCODE_KERNEL[_BLOCKS]        the colour kernels' names: encode_bgra_nv12[_blocks] / encode_bgra_i420[_blocks]
//   BT709_ENCODE_ALPHA_KERNEL[_BLOCKS]  the alpha kernels' names: encode_alpha_y[_blocks] / encode_alpha_y[_blocks]_i420
// defined.  Text inclusion and not a templated body: a body inlined into the NV12 kernels changed their generated code (the
// workgroup-size query stopped folding to one scalar load in the general kernels, registers moved in the fast ones); as kernels
// of their own text they compile to the instruction streams they had before the planar twins existed.

// grid = (tiles, row-pair groups, frames); a workgroup walks row_pairs_per_block consecutive row
// pairs of one frame, prefetching the next pair while it encodes the current one.
__global__ void __launch_bounds__(kMaxBlockThreads)
BT709_ENCODE_KERNEL(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const BandedWork work = banded_work(p.xcd_bands, p.frames_per_band);  // XCD-aware work map: bt709_tile.h
  const EncodeFrame f = encode_frame(p, work.frame);
  const uint32_t quads = p.width >> 2;
  const uint32_t row_pairs = p.height >> 1;
  const uint32_t q_raw = work.tile * blockDim.x + threadIdx.x;
  const uint32_t q = min(q_raw, quads - 1);
  const uint32_t rp0 = blockIdx.y * p.row_pairs_per_block;
  const uint32_t rp_end = min(rp0 + p.row_pairs_per_block, row_pairs);

  // row pointers are uniform (SGPR base), the lane adds a 32-bit offset: no 64-bit VALU address arithmetic
  const uint8_t *s0 = f.bgra + static_cast<size_t>(2 * rp0) * p.bgra_stride;
  u32x4 top = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + 16u * q));
  u32x4 bot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + p.bgra_stride + 16u * q));

  const EncodeLds t = stage_encode_tables(lds_raw, p);  // after the first loads are in flight
  __syncthreads();
  const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);

  for (uint32_t rp = rp0; rp < rp_end; ++rp) {
    // prefetch the next row pair before the arithmetic; nothing on the workgroup's last pair (a
    // clamped re-read of the own rows cost 8 % extra HBM reads at 9 row pairs per workgroup:
    // non-temporal loads do not stay in L2)
    u32x4 ntop = top, nbot = bot;
    if (rp + 1 < rp_end) {
      const uint8_t *s1 = f.bgra + static_cast<size_t>(2 * (rp + 1)) * p.bgra_stride;
      ntop = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + 16u * q));
      nbot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + p.bgra_stride + 16u * q));
    }

    float va[6], vb[6];
    {
      const uint32_t blk[4] = {top.x, top.y, bot.x, bot.y};
      encode_block(t, quarter_n, blk, va);
    }
    {
      const uint32_t blk[4] = {top.z, top.w, bot.z, bot.w};
      encode_block(t, quarter_n, blk, vb);
    }
    uint32_t ytop, ybot, cbcr;
    quantize_quad<BT709_ENCODE_LAYOUT>(va, vb, ytop, ybot, cbcr);
    if (q_raw < quads) {
      uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
      __builtin_nontemporal_store(ytop, reinterpret_cast<uint32_t *>(y0 + 4u * q));
      __builtin_nontemporal_store(ybot, reinterpret_cast<uint32_t *>(y0 + p.y_stride + 4u * q));
      store_quad_chroma<BT709_ENCODE_LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, q, cbcr);
    }
    top = ntop;
    bot = nbot;
  }
}

// General layout: one lane per 2x2 block, scalar loads/stores, any alignment.
__global__ void __launch_bounds__(kBlockThreads)
BT709_ENCODE_KERNEL_BLOCKS(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const EncodeLds t = stage_encode_tables(lds_raw, p);
  __syncthreads();
  const EncodeFrame f = encode_frame(p, blockIdx.z);
  const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);
  const uint32_t bw = p.width >> 1;
  const uint32_t rp = blockIdx.y;
  for (uint32_t bx = blockIdx.x * blockDim.x + threadIdx.x; bx < bw; bx += gridDim.x * blockDim.x) {
    const uint32_t *r0 = reinterpret_cast<const uint32_t *>(f.bgra + static_cast<size_t>(2 * rp) * p.bgra_stride);
    const uint32_t *r1 = reinterpret_cast<const uint32_t *>(f.bgra + static_cast<size_t>(2 * rp + 1) * p.bgra_stride);
    const uint32_t blk[4] = {r0[2 * bx], r0[2 * bx + 1], r1[2 * bx], r1[2 * bx + 1]};
    float v[6];
    encode_block(t, quarter_n, blk, v);
    uint32_t ytop, ybot, cbcr;
    quantize_block(v, ytop, ybot, cbcr);
    uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    uint8_t *y1 = y0 + p.y_stride;
    y0[2 * bx] = static_cast<uint8_t>(ytop);
    y0[2 * bx + 1] = second_byte<BT709_ENCODE_LAYOUT>(ytop);
    y1[2 * bx] = static_cast<uint8_t>(ybot);
    y1[2 * bx + 1] = second_byte<BT709_ENCODE_LAYOUT>(ybot);
    store_block_chroma<BT709_ENCODE_LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, bx, static_cast<uint8_t>(cbcr), static_cast<uint8_t>(cbcr >> 8));
  }
}

// ---------------------------------------------------------------- alpha frames (BT709HIP_FORMAT_BGRA8_ALPHA): bt709_encode.hip

// grid = (tiles, row-pair groups, frames), as encode_bgra_nv12
__global__ void __launch_bounds__(kMaxBlockThreads)
BT709_ENCODE_ALPHA_KERNEL(const EncodeParams p) {
  __shared__ uint32_t lut[64];
  const BandedWork work = banded_work(p.xcd_bands, p.frames_per_band);
  const EncodeFrame f = encode_frame(p, work.frame);
  const uint32_t quads = p.width >> 2;
  const uint32_t row_pairs = p.height >> 1;
  const uint32_t q_raw = work.tile * blockDim.x + threadIdx.x;
  const uint32_t q = min(q_raw, quads - 1);
  const uint32_t rp0 = blockIdx.y * p.row_pairs_per_block;
  const uint32_t rp_end = min(rp0 + p.row_pairs_per_block, row_pairs);
  const bool with_cbcr = p.frames[0].cbcr != nullptr;  // uniform over the launch

  const uint8_t *s0 = f.bgra + static_cast<size_t>(2 * rp0) * p.bgra_stride;
  u32x4 top = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + 16u * q));
  u32x4 bot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + p.bgra_stride + 16u * q));

  stage_alpha_luma(lut, p);  // after the first loads are in flight
  __syncthreads();

  for (uint32_t rp = rp0; rp < rp_end; ++rp) {
    u32x4 ntop = top, nbot = bot;
    if (rp + 1 < rp_end) {  // nothing on the workgroup's last pair, as encode_bgra_nv12
      const uint8_t *s1 = f.bgra + static_cast<size_t>(2 * (rp + 1)) * p.bgra_stride;
      ntop = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + 16u * q));
      nbot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + p.bgra_stride + 16u * q));
    }
    const uint32_t ytop = alpha_luma4(lut, top), ybot = alpha_luma4(lut, bot);
    if (q_raw < quads) {
      uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
      __builtin_nontemporal_store(ytop, reinterpret_cast<uint32_t *>(y0 + 4u * q));
      __builtin_nontemporal_store(ybot, reinterpret_cast<uint32_t *>(y0 + p.y_stride + 4u * q));
      if (with_cbcr) store_quad_chroma<BT709_ENCODE_LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, q, 0x80808080u);
    }
    top = ntop;
    bot = nbot;
  }
}

// General layout: one lane per 2x2 block, byte loads of the four A's and byte stores, any alignment.
__global__ void __launch_bounds__(kBlockThreads)
BT709_ENCODE_ALPHA_KERNEL_BLOCKS(const EncodeParams p) {
  __shared__ uint32_t lut[64];
  stage_alpha_luma(lut, p);
  __syncthreads();
  const uint8_t *t = reinterpret_cast<const uint8_t *>(lut);
  const EncodeFrame f = encode_frame(p, blockIdx.z);
  const bool with_cbcr = p.frames[0].cbcr != nullptr;
  const uint32_t bw = p.width >> 1;
  const uint32_t rp = blockIdx.y;
  for (uint32_t bx = blockIdx.x * blockDim.x + threadIdx.x; bx < bw; bx += gridDim.x * blockDim.x) {
    const uint8_t *r0 = f.bgra + static_cast<size_t>(2 * rp) * p.bgra_stride + 8u * bx;
    const uint8_t *r1 = r0 + p.bgra_stride;
    uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride + 2u * bx;
    uint8_t *y1 = y0 + p.y_stride;
    y0[0] = t[r0[3]];
    y0[1] = t[r0[7]];
    y1[0] = t[r1[3]];
    y1[1] = t[r1[7]];
    if (with_cbcr) store_block_chroma<BT709_ENCODE_LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, bx, 128, 128);
  }
}

