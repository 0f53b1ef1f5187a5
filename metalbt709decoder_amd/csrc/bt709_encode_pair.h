// The paired fast kernel (BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA); included by bt709_encode.hip alone, behind the helpers it
// shares with encode_bgra and encode_alpha_y (stage_encode_tables, encode_block, quantize_quad, store_quad_chroma, premultiply_row,
// stage_alpha_luma, alpha_luma4, pair_frame ...).
//
// One BGRA surface in, TWO frames out of one read: the colour frame encode_bgra<FORM> writes, and the alpha frame encode_alpha_y
// writes for BGRA8_ALPHA input -- Y = T[A] per pixel (bt709_alpha_luma.h), Cb = Cr = 128 when it has a chroma plane.  The
// reference's `srgb_to_bt709 -alpha` makes the two clips from one picture (srgb_to_bt709/srgb_to_bt709.m:842-954); two launches
// read the 4 B/pixel surface twice.
//
// Shape: encode_bgra's -- same tile, work map, row-pair walk, prefetch, lane clamp, launch plan and arithmetic.  The rider: the
// lane that holds a quad's two u32x4 rows looks up T[word >> 24] for its eight texels (eight ds_read_u8) and stores two more
// dwords, plus 0x80808080 through store_quad_chroma when the alpha frame has chroma.  A is read from the words AS LOADED, ahead of
// the premultiply (which leaves A alone, but nothing here depends on that).
//
// A __global__ template of its own and not a further FORM bit of encode_bgra: with the rider under `if constexpr` in encode_bgra's
// text the plain instantiations kept every instruction but swapped the registers of the two prefetched rows
// (profiles/r18_encode_pair_isa.txt); encode_bgra_blocks takes the bit (kFormPair) and keeps its code.  kFormPair in FORM is
// accepted and means nothing here: one row macro of the launch table serves both kernels.
//
// LDS: stage_encode_tables needs the dynamic segment at address 0, so this kernel has no static LDS either; T's 256 bytes sit in
// the dynamic segment behind the two tables (pair_alpha_lut), and launch_encode sizes the segment for them.
#pragma once

namespace bt709 {

// Preconditions of the fast kernel (checked by the host shim): encode_bgra's, and the alpha Y pointer, pitch and step 4-byte
// aligned, the alpha chroma plane aligned as the colour's.  grid = (tiles, row-pair groups, pairs), as encode_bgra.
template <uint32_t FORM>
__global__ void __launch_bounds__(kMaxBlockThreads)
encode_bgra_alpha(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr uint32_t LAYOUT = form_layout(FORM);
  const BandedWork work = banded_work(p.xcd_bands, p.frames_per_band);
  AlphaPlanes a;
  const EncodeFrame f = pair_frame(p, work.frame, a);
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
  uint32_t *const alpha_lut = pair_alpha_lut(lds_raw, p);
  stage_alpha_luma(alpha_lut, p);
  __syncthreads();
  const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);

  for (uint32_t rp = rp0; rp < rp_end; ++rp) {
    u32x4 ntop = top, nbot = bot;
    if (rp + 1 < rp_end) {  // nothing on the workgroup's last pair, as encode_bgra
      const uint8_t *s1 = f.bgra + static_cast<size_t>(2 * (rp + 1)) * p.bgra_stride;
      ntop = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + 16u * q));
      nbot = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + p.bgra_stride + 16u * q));
    }

    const uint32_t atop = alpha_luma4(alpha_lut, top), abot = alpha_luma4(alpha_lut, bot);  // T[A] of the words as loaded
    if constexpr (form_straight(FORM)) {  // behind the prefetch, ahead of everything that reads a colour byte
      premultiply_row(top);
      premultiply_row(bot);
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
    quantize_quad<LAYOUT>(va, vb, ytop, ybot, cbcr);
    if (q_raw < quads) {
      uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
      __builtin_nontemporal_store(ytop, reinterpret_cast<uint32_t *>(y0 + 4u * q));
      __builtin_nontemporal_store(ybot, reinterpret_cast<uint32_t *>(y0 + p.y_stride + 4u * q));
      store_quad_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, q, cbcr);
      uint8_t *a0 = a.y + static_cast<size_t>(2 * rp) * a.y_stride;
      __builtin_nontemporal_store(atop, reinterpret_cast<uint32_t *>(a0 + 4u * q));
      __builtin_nontemporal_store(abot, reinterpret_cast<uint32_t *>(a0 + a.y_stride + 4u * q));
      if (a.with_cbcr) store_quad_chroma<LAYOUT>(a, a.cbcr + static_cast<size_t>(rp) * a.cbcr_stride, q, 0x80808080u);
    }
    top = ntop;
    bot = nbot;
  }
}

}  // namespace bt709
