// C-ABI shim, the converters either side of the decode (include/bt709hip.h): +unconvert: on packed 4:4:4 words
// (Renderer/BGRAToBT709Converter.h:34-46), pass 2 alone (-renderScaled:, Renderer/MetalScaleRenderContext.h:34-40), the
// BGRA -> NV12 / I420 encoder (+convertIntoCoreVideoBuffer:, BGRAToBT709Converter.h:73-76) and the planar <-> NV12 chroma layouts
// of the reference's Y4M files (Renderer/y4m_writer.h:194-241).
#include "shim_internal.h"

#include "bt709_alpha_luma.h"

namespace bt709shim __attribute__((visibility("hidden"))) {

// Builds (once) the device tables of one (input gamma, output gamma) encoder pair.  Both uploads go
// into locals and are published together: a failed second upload leaves the pair unbuilt, not half
// built.  Refused while `s` records a graph (hipMalloc / blocking copies are illegal there): call
// bt709hip_encoder_prepare before bt709hip_graph_begin_capture.
int encoder_tables(bt709hip_context *ctx, int input_gamma, int output_gamma, hipStream_t s) {
  EncoderTables &t = ctx->encoders[input_gamma][output_gamma];
  std::lock_guard<std::mutex> lock(ctx->encoder_mutex);
  if (t.d_per_byte != nullptr) return BT709HIP_OK;
  if (capturing(s)) return BT709HIP_ERR_NOT_SETUP;
  EncodeTables host;
  SplitTable fl;
  if (!build_encode_tables(input_gamma, output_gamma, &host) || !build_split_table(host.from_linear_kind, &fl))
    return BT709HIP_ERR_UNSUPPORTED;
  void *d_fl = nullptr, *d_pb = nullptr;
  const uint32_t fl_bytes = static_cast<uint32_t>(fl.buckets.size() * sizeof(TransferBucket));
  if (int rc = upload_table(fl.buckets.data(), fl_bytes, &d_fl)) return rc;
  if (int rc = upload_table(host.per_byte, sizeof host.per_byte, &d_pb)) {
    (void)hipFree(d_fl);
    return rc;
  }
  t.from_linear_n = fl.n_fine;
  t.split = fl.split;
  t.coarse_scale = fl.coarse_scale;
  t.coarse_offset = fl.coarse_offset;
  t.from_linear_bytes = fl_bytes;
  t.d_from_linear = d_fl;
  t.d_per_byte = d_pb;  // the "built" marker: last
  return BT709HIP_OK;
}

// Builds (once) the device copy of T[A], the luma table of BGRA8_ALPHA input (bt709_alpha_luma.h), from the product's own
// (Linear, Linear) per-byte table.  Same rules as encoder_tables: refused while `s` records a graph.
int alpha_luma_table(bt709hip_context *ctx, hipStream_t s) {
  std::lock_guard<std::mutex> lock(ctx->encoder_mutex);
  if (ctx->d_alpha_luma != nullptr) return BT709HIP_OK;
  if (capturing(s)) return BT709HIP_ERR_NOT_SETUP;
  EncodeTables host;
  if (!build_encode_tables(kGammaLinear, kGammaLinear, &host)) return BT709HIP_ERR_UNSUPPORTED;
  alignas(4) uint8_t luma[256];
  build_alpha_luma(host.per_byte, luma);
  return upload_table(luma, sizeof luma, &ctx->d_alpha_luma);
}

// Builds (once) the device copy of the per-pixel converter's curve for one output gamma (BT709HIP_CTX_OPT_ENCODE_CONVERT;
// transfer_tables.h build_convert_curve).  Same rules as encoder_tables: refused while `s` records a graph.
int convert_curve_table(bt709hip_context *ctx, int output_gamma, hipStream_t s) {
  std::lock_guard<std::mutex> lock(ctx->encoder_mutex);
  if (ctx->d_convert_curve[output_gamma] != nullptr) return BT709HIP_OK;
  if (capturing(s)) return BT709HIP_ERR_NOT_SETUP;
  alignas(16) float curve[256];
  if (!build_convert_curve(output_gamma, curve)) return BT709HIP_ERR_UNSUPPORTED;
  return upload_table(curve, sizeof curve, &ctx->d_convert_curve[output_gamma]);
}

}  // namespace bt709shim

extern "C" {

int bt709hip_unconvert_batch(bt709hip_decoder *dec, int count, const void *const *ycbcr_words, size_t in_stride, int width, int height,
                             const bt709hip_surface *outs, void *stream, int wait_until_completed) {
  if (dec == nullptr || outs == nullptr || ycbcr_words == nullptr || width < 0 || height < 0 || count < 0) return BT709HIP_ERR_INVALID_ARG;
  if (int rc = ensure_setup(dec, stream)) return rc;
  FLUSH_STREAM(dec->ctx, stream);
  if (dec->has_alpha) return BT709HIP_ERR_UNSUPPORTED;  // the packed words carry no alpha sample
  if (count == 0) return BT709HIP_OK;
  const size_t row = static_cast<size_t>(width) * 4;
  bool vec = (width % 4) == 0 && (in_stride % 16) == 0;
  bool uniform = count > 1;
  std::vector<void *> out_ptrs(static_cast<size_t>(count));
  for (int i = 0; i < count; ++i) {
    const bt709hip_surface &o = outs[i];
    if (o.width != width || o.height != height) return BT709HIP_ERR_SIZE_MISMATCH;
    if ((width & 1) || (height & 1)) return BT709HIP_ERR_ODD_DIMENSIONS;  // BGRAToBT709Converter.m:69-74
    if (o.format != BT709HIP_FORMAT_BGRA8_SRGB || o.reserved != 0) return BT709HIP_ERR_UNSUPPORTED;
    if (o.stride != outs[0].stride) return BT709HIP_ERR_SIZE_MISMATCH;
    if (width == 0 || height == 0) continue;
    if (ycbcr_words[i] == nullptr || o.bgra == nullptr) return BT709HIP_ERR_INVALID_ARG;
    if (in_stride < row || (in_stride & 3) || !aligned(ycbcr_words[i], 4) || o.stride < row || (o.stride & 3) || !aligned(o.bgra, 4) ||
        in_stride > 0xffffffffu || o.stride > 0xffffffffu)
      return BT709HIP_ERR_STRIDE;
    vec = vec && (o.stride % 16) == 0 && aligned(ycbcr_words[i], 16) && aligned(o.bgra, 16);
    out_ptrs[static_cast<size_t>(i)] = o.bgra;
    if (i >= 2)
      uniform = uniform && byte_step(ycbcr_words[0], ycbcr_words[i]) == byte_step(ycbcr_words[0], ycbcr_words[1]) * i &&
                byte_step(outs[0].bgra, o.bgra) == byte_step(outs[0].bgra, outs[1].bgra) * i;
  }
  if (width == 0 || height == 0) return BT709HIP_OK;
  if (count > (uniform ? kMaxUniformBatch : kMaxBatch)) return BT709HIP_ERR_UNSUPPORTED;
  if (height > kMaxGridYZ) return BT709HIP_ERR_UNSUPPORTED;
  if (int rc = bind(dec->ctx)) return rc;
  DecodeParams t;
  std::memset(&t, 0, sizeof t);
  set_tables(&t, dec);
  t.alpha_word = dec->alpha_fill << 24;
  UnconvertBatch batch;
  batch.count = count;
  batch.uniform = uniform;
  batch.in = ycbcr_words;
  batch.out = out_ptrs.data();
  batch.in_step = uniform ? byte_step(ycbcr_words[0], ycbcr_words[1]) : 0;
  batch.out_step = uniform ? byte_step(outs[0].bgra, outs[1].bgra) : 0;
  hipStream_t s = pick(dec->ctx, stream);
  set_kernel_name(launch_unconvert(t, batch, in_stride, outs[0].stride, static_cast<uint32_t>(width), static_cast<uint32_t>(height), vec,
                                    dec->gamma == kGammaSRGB, s));
  return finish_launch(s, wait_until_completed);
}

int bt709hip_unconvert(bt709hip_decoder *dec, const void *ycbcr_words, size_t in_stride, int width, int height,
                       const bt709hip_surface *out, void *stream, int wait_until_completed) {
  if (out == nullptr) return BT709HIP_ERR_INVALID_ARG;
  return bt709hip_unconvert_batch(dec, 1, &ycbcr_words, in_stride, width, height, out, stream, wait_until_completed);
}

extern "C++" {  // helpers with C++ linkage inside the C-ABI block
namespace {

// Tables of the stand-alone pass 2, built once per context: the two-resolution sRGB-encode buckets
// (as a decoder's) and lin[256] = sRGB_nonLinearNormToLinear(byteNorm(b)) (the sRGB8 sampler's decode).
int render_tables(bt709hip_context *ctx, hipStream_t s) {
  std::lock_guard<std::mutex> lock(ctx->encoder_mutex);
  if (ctx->d_render_lin != nullptr) return BT709HIP_OK;
  if (capturing(s)) return BT709HIP_ERR_NOT_SETUP;
  TransferTable enc;
  if (!build_transfer_table(kGammaLinear, &enc) || enc.buckets_log.empty()) return BT709HIP_ERR_UNSUPPORTED;
  float lin[256];
  for (int b = 0; b < 256; ++b) lin[b] = srgb_to_linear(b * (1.0f / 255.0f));
  void *d_enc = nullptr, *d_lin = nullptr;
  const uint32_t enc_bytes = static_cast<uint32_t>(enc.buckets_log.size() * sizeof(TransferBucket));
  int rc = upload_table(enc.buckets_log.data(), enc_bytes, &d_enc);
  if (rc == BT709HIP_OK) rc = upload_table(lin, sizeof lin, &d_lin);
  if (rc != BT709HIP_OK) {
    if (d_enc) (void)hipFree(d_enc);
    return rc;
  }
  ctx->render_encode_bytes = enc_bytes;
  ctx->render_encode_log_add = enc.log_add;
  ctx->render_encode_log_first = enc.log_first;
  ctx->d_render_encode = d_enc;
  ctx->d_render_lin = d_lin;  // the "built" marker: last
  return BT709HIP_OK;
}

}  // namespace
}  // extern "C++"

int bt709hip_render_scaled_prepare(bt709hip_context *ctx) {
  if (int rc = bind(ctx)) return rc;
  return render_tables(ctx, nullptr);
}

static int render_scaled_launch(bt709hip_context *ctx, int count, const bt709hip_surface *in, const bt709hip_surface *out,
                                int64_t in_step, int64_t out_step, void *stream, int wait_until_completed);

int bt709hip_render_scaled_batch(bt709hip_context *ctx, int count, const bt709hip_surface *in, const bt709hip_surface *out,
                                 void *stream, int wait_until_completed) {
  if (ctx == nullptr || in == nullptr || out == nullptr || count < 0 || count > kMaxUniformBatch) return BT709HIP_ERR_INVALID_ARG;
  if (count == 0) return BT709HIP_OK;
  // one geometry, surfaces evenly spaced in memory (a ring carved from one allocation): surface i = surface 0 + i * step
  int64_t in_step = 0, out_step = 0;
  if (count > 1) {
    in_step = static_cast<const uint8_t *>(in[1].bgra) - static_cast<const uint8_t *>(in[0].bgra);
    out_step = static_cast<const uint8_t *>(out[1].bgra) - static_cast<const uint8_t *>(out[0].bgra);
  }
  for (int i = 1; i < count; ++i) {
    if (in[i].width != in[0].width || in[i].height != in[0].height || in[i].stride != in[0].stride || in[i].format != in[0].format ||
        in[i].reserved != 0 || out[i].width != out[0].width || out[i].height != out[0].height || out[i].stride != out[0].stride ||
        out[i].format != out[0].format || out[i].reserved != 0)
      return BT709HIP_ERR_SIZE_MISMATCH;
    if (static_cast<const uint8_t *>(in[i].bgra) != static_cast<const uint8_t *>(in[0].bgra) + static_cast<int64_t>(i) * in_step ||
        static_cast<const uint8_t *>(out[i].bgra) != static_cast<const uint8_t *>(out[0].bgra) + static_cast<int64_t>(i) * out_step)
      return BT709HIP_ERR_UNSUPPORTED;
  }
  return render_scaled_launch(ctx, count, in, out, in_step, out_step, stream, wait_until_completed);
}

int bt709hip_render_scaled(bt709hip_context *ctx, const bt709hip_surface *in, const bt709hip_surface *out, void *stream,
                           int wait_until_completed) {
  return render_scaled_launch(ctx, 1, in, out, 0, 0, stream, wait_until_completed);
}

static int render_scaled_launch(bt709hip_context *ctx, int count, const bt709hip_surface *in, const bt709hip_surface *out,
                                int64_t in_step, int64_t out_step, void *stream, int wait_until_completed) {
  if (ctx == nullptr || in == nullptr || out == nullptr) return BT709HIP_ERR_INVALID_ARG;
  if (in->width < 0 || in->height < 0 || out->width < 0 || out->height < 0 || in->reserved != 0 || out->reserved != 0)
    return BT709HIP_ERR_INVALID_ARG;
  if (in->format != BT709HIP_FORMAT_BGRA8_SRGB && in->format != BT709HIP_FORMAT_RGBA16F) return BT709HIP_ERR_INVALID_ARG;
  if (out->format != BT709HIP_FORMAT_BGRA8_SRGB) return BT709HIP_ERR_UNSUPPORTED;  // the view is an 8-bit sRGB drawable
  if (in->width == 0 || in->height == 0 || out->width == 0 || out->height == 0) return BT709HIP_OK;
  if (in->bgra == nullptr || out->bgra == nullptr) return BT709HIP_ERR_INVALID_ARG;
  const size_t ipx = in->format == BT709HIP_FORMAT_RGBA16F ? 8 : 4;
  if (in->stride < static_cast<size_t>(in->width) * ipx || (in->stride & (ipx - 1)) || !aligned(in->bgra, ipx) ||
      out->stride < static_cast<size_t>(out->width) * 4 || (out->stride & 3) || !aligned(out->bgra, 4) ||
      in->stride > 0xffffffffu || out->stride > 0xffffffffu)
    return BT709HIP_ERR_STRIDE;
  // the other surfaces of a batch share surface 0's geometry; their bases are checked as its base was (a step that is no
  // multiple of the texel size misaligns surface 1 onwards)
  for (int i = 1; i < count; ++i)
    if (!aligned(in[i].bgra, ipx) || !aligned(out[i].bgra, 4)) return BT709HIP_ERR_STRIDE;
  if (out->height > kMaxGridYZ) return BT709HIP_ERR_UNSUPPORTED;
  if (int rc = bind(ctx)) return rc;
  FLUSH_STREAM(ctx, stream);
  hipStream_t s = pick(ctx, stream);
  if (int rc = render_tables(ctx, s)) return rc;
  RenderParams p;
  std::memset(&p, 0, sizeof p);
  p.in = static_cast<const uint8_t *>(in->bgra);
  p.out = static_cast<uint8_t *>(out->bgra);
  p.in_stride = static_cast<uint32_t>(in->stride);
  p.out_stride = static_cast<uint32_t>(out->stride);
  p.width = static_cast<uint32_t>(in->width);
  p.height = static_cast<uint32_t>(in->height);
  p.out_width = static_cast<uint32_t>(out->width);
  p.out_height = static_cast<uint32_t>(out->height);
  p.scale_x = static_cast<float>(in->width) / static_cast<float>(out->width);
  p.scale_y = static_cast<float>(in->height) / static_cast<float>(out->height);
  p.table_encode = ctx->d_render_encode;
  p.table_lin = ctx->d_render_lin;
  p.table_encode_bytes = ctx->render_encode_bytes;
  p.encode_log_add = ctx->render_encode_log_add;
  p.encode_log_first = ctx->render_encode_log_first;
  p.in_step = in_step;
  p.out_step = out_step;
  const char *name = launch_render_scaled(p, count, in->format == BT709HIP_FORMAT_RGBA16F,
                                          static_cast<uint32_t>(ctx->props.multiProcessorCount), s);
  if (name == nullptr) return BT709HIP_ERR_UNSUPPORTED;  // a surface of 2 GiB or more
  set_kernel_name(name);
  return finish_launch(s, wait_until_completed);
}

// ------------------------------------------------------------------ encoder

int bt709hip_encode_batch(bt709hip_context *ctx, int count, const bt709hip_surface *ins, const bt709hip_frame *outs,
                          int input_gamma, int output_gamma, void *stream, int wait_until_completed) {
  if (ctx == nullptr || ins == nullptr || outs == nullptr || count < 0) return BT709HIP_ERR_INVALID_ARG;
  // BT709HIP_CTX_OPT_ENCODE_CONVERT, read once: the call is the per-pixel converter (+convert:), whose output gamma may be ITU709;
  // PACKED444 writes 32-bit words (Cr<<16)|(Cb<<8)|Y through out->y and takes no chroma plane; POINT420 writes an ordinary frame
  // BT709HIP_CTX_OPT_ENCODE_HALF_INPUT, read once: with it at 1 RGBA16F surfaces (linear light) are input; the call
  // takes its format from ins[0], a batch of mixed formats is a size mismatch as ever.  The half path has no converter, no pair
  // and no premultiply: it is validated as the plain encoder's call and refused behind that if one of those options is set.
  const bool half_input = ctx->encode_half_input != 0;
  const bool half = count > 0 && half_input && ins[0].format == BT709HIP_FORMAT_RGBA16F;
  // BT709HIP_CTX_OPT_ENCODE_CHW_INPUT, read once: with it at 1 planar CHW_U8 / _F16 / _F32 surfaces are input, again by
  // ins[0]'s format.  Such a call is the plain BGRA8 encoder's call with the element size in place of the texel's; the converter, the
  // pair and the premultiply are refused behind the usual validation.  At 0 the three formats are what they were: unknown.
  const bool chw_input = ctx->encode_chw_input != 0;
  const bool chw = count > 0 && chw_input && is_chw(ins[0].format);
  const int convert_option = ctx->encode_convert;
  const int convert = half || chw ? BT709HIP_CONVERT_OFF : convert_option;
  const bool packed = convert == BT709HIP_CONVERT_PACKED444;
  if (input_gamma < 0 || input_gamma > 2 || output_gamma < 0 || output_gamma > (convert != BT709HIP_CONVERT_OFF ? 3 : 2)) return BT709HIP_ERR_INVALID_ARG;
  if (count == 0) return BT709HIP_OK;
  const bt709hip_surface &in0 = ins[0];
  const bt709hip_frame &out0 = outs[0];
  // BGRA8_ALPHA: the texels read as the grey picture (A,A,A) of the reference's alpha clip; only its Y plane is ever decoded,
  // so cbcr may be NULL -- in every frame of the call or in none -- and cbcr_stride is not looked at then
  const bool alpha = in0.format == BT709HIP_FORMAT_BGRA8_ALPHA;
  const bool no_cbcr = packed || (alpha && out0.cbcr == nullptr);  // the packed words: cbcr must be NULL in every frame, cbcr_stride is not looked at
  // BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT, read once: cbcr is the U plane, W/2 bytes a row, V (H/2) x cbcr_stride bytes behind it.
  // Without a chroma plane there is nothing to lay out: such a call is what it was, whatever the option holds.
  const bool planar = ctx->encode_chroma_layout == BT709HIP_CHROMA_I420 && !no_cbcr;
  // BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY, read once: BGRA8_SRGB texels are straight alpha.  BGRA8_ALPHA input reads A alone: unaffected.
  const bool premultiply = ctx->encode_premultiply != 0 && !alpha && !half && !chw;
  const size_t chroma_align = planar ? 2 : 4;  // the fast kernels' chroma store: a 2-byte half per plane, or the CbCr dword
  // BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA, read once: BGRA8_SRGB input writes two frames, the colour into outs[i] and the alpha frame
  // (BGRA8_ALPHA output's rules) into outs[count + i], from one launch.  Not with the per-pixel converter and not for BGRA8_ALPHA
  // input: refused behind the usual validation.
  const bool with_alpha = ctx->encode_with_alpha != 0;
  // BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA, read once: the same two frames per picture from RGBA16F input, the alpha
  // frame from the texel's A half.  An option of its own: WITH_ALPHA with half input stays refused.  No other input reads it.
  const bool half_pair = half && ctx->encode_half_with_alpha != 0;
  const bool pair = half_pair || (with_alpha && !alpha && !half && !chw && convert == BT709HIP_CONVERT_OFF);
  const bt709hip_frame &alpha0 = outs[pair ? count : 0];
  const bool alpha_no_cbcr = pair && alpha0.cbcr == nullptr;
  bool uniform = count > 1;
  const size_t y_px = packed ? 4 : 1, y_align = packed ? 16 : 4;  // bytes of a pixel in the plane out->y points to; the fast kernels' store to it
  bool fast = (in0.width % 4) == 0 && (in0.stride % 16) == 0 && (out0.y_stride % y_align) == 0 && (no_cbcr || (out0.cbcr_stride % chroma_align) == 0);
  // encode_rgba16f: a 2x2 block per lane -- any even width; 2-byte stores to Y and CbCr, byte stores to U and V
  const size_t half_chroma_align = planar ? 1 : 2;
  if (half) fast = (in0.stride % 16) == 0 && (out0.y_stride % 2) == 0 && (out0.cbcr_stride % half_chroma_align) == 0;
  const size_t in_px = chw ? element_bytes(in0.format) : half ? 8 : 4;  // bytes of a texel, or of a CHW plane's element
  // encode_chw: a quad per lane and plane -- 4 elements a load; its stores are encode_bgra's
  const size_t chw_align = 4 * in_px;
  if (chw) fast = (in0.width % 4) == 0 && (in0.stride % chw_align) == 0 && (out0.y_stride % y_align) == 0 && (out0.cbcr_stride % chroma_align) == 0;
  // the paired fast kernels store to the alpha frame as they do to the colour's: encode_bgra_alpha dwords, encode_rgba16f_alpha halves
  const size_t pair_y_align = half ? 2 : 4, pair_chroma_align = half ? half_chroma_align : chroma_align;
  if (pair) fast = fast && (alpha0.y_stride % pair_y_align) == 0 && (alpha_no_cbcr || (alpha0.cbcr_stride % pair_chroma_align) == 0);
  EncodeParams p;
  std::memset(&p, 0, sizeof p);
  for (int i = 0; i < count; ++i) {
    const bt709hip_surface &in = ins[i];
    const bt709hip_frame &out = outs[i];
    if (in.width < 0 || in.height < 0) return BT709HIP_ERR_INVALID_ARG;
    if (in.width != out.width || in.height != out.height) return BT709HIP_ERR_SIZE_MISMATCH;
    if ((in.width & 1) || (in.height & 1)) return BT709HIP_ERR_ODD_DIMENSIONS;  // BGRAToBT709Converter.m:540-541
    if (in.height / 2 > kMaxGridYZ) return BT709HIP_ERR_UNSUPPORTED;            // row pairs live in gridDim.y
    if ((in.format != BT709HIP_FORMAT_BGRA8_SRGB && in.format != BT709HIP_FORMAT_BGRA8_ALPHA &&
         !(in.format == BT709HIP_FORMAT_RGBA16F && half_input) && !(is_chw(in.format) && chw_input)) || in.reserved != 0)
      return BT709HIP_ERR_UNSUPPORTED;
    if (in.width != in0.width || in.height != in0.height || in.stride != in0.stride || in.format != in0.format ||
        out.y_stride != out0.y_stride || (!(packed || (alpha && (no_cbcr || out.cbcr == nullptr))) && out.cbcr_stride != out0.cbcr_stride))
      return BT709HIP_ERR_SIZE_MISMATCH;
    // the reference forces an alpha clip's gamma to linear (srgb_to_bt709.m:842-954); anything else is "alpha is not linear"
    if (alpha && (input_gamma != BT709HIP_GAMMA_LINEAR || output_gamma != BT709HIP_GAMMA_LINEAR)) return BT709HIP_ERR_ALPHA_TRANSFER;
    if (half && input_gamma != BT709HIP_GAMMA_LINEAR) return BT709HIP_ERR_TRANSFER;  // the texels hold linear light
    if (in.width == 0 || in.height == 0) continue;
    if (in.bgra == nullptr || out.y == nullptr || (out.cbcr == nullptr) != no_cbcr) return BT709HIP_ERR_INVALID_ARG;
    const size_t w = static_cast<size_t>(in.width);
    if (in.stride < in_px * w || (in.stride & (in_px - 1)) || !aligned(in.bgra, in_px) || out.y_stride < y_px * w || (!no_cbcr && out.cbcr_stride < (planar ? w / 2 : w)))
      return BT709HIP_ERR_STRIDE;
    if (packed && ((out.y_stride & 3) || !aligned(out.y, 4))) return BT709HIP_ERR_STRIDE;  // words
    if (in.stride > 0xffffffffu || out.y_stride > 0xffffffffu || (!no_cbcr && out.cbcr_stride > 0xffffffffu)) return BT709HIP_ERR_STRIDE;
    if (half) fast = fast && aligned(in.bgra, 16) && aligned(out.y, 2) && aligned(out.cbcr, half_chroma_align);
    else if (chw) fast = fast && aligned(in.bgra, chw_align) && aligned(out.y, y_align) && aligned(out.cbcr, chroma_align);
    else fast = fast && aligned(in.bgra, 16) && aligned(out.y, y_align) && aligned(out.cbcr, chroma_align);
    if (i >= 2)
      uniform = uniform && byte_step(ins[0].bgra, in.bgra) == byte_step(ins[0].bgra, ins[1].bgra) * i &&
                byte_step(outs[0].y, out.y) == byte_step(outs[0].y, outs[1].y) * i &&
                byte_step(outs[0].cbcr, out.cbcr) == byte_step(outs[0].cbcr, outs[1].cbcr) * i;
    if (pair) {  // the pair's alpha frame: what a BGRA8_ALPHA call checks of its output, in that call's order
      const bt709hip_frame &af = outs[count + i];
      if (af.width != in.width || af.height != in.height) return BT709HIP_ERR_SIZE_MISMATCH;
      if (af.y_stride != alpha0.y_stride || (!alpha_no_cbcr && af.cbcr != nullptr && af.cbcr_stride != alpha0.cbcr_stride)) return BT709HIP_ERR_SIZE_MISMATCH;
      if (af.y == nullptr || (af.cbcr == nullptr) != alpha_no_cbcr) return BT709HIP_ERR_INVALID_ARG;
      if (af.y_stride < w || (!alpha_no_cbcr && af.cbcr_stride < (planar ? w / 2 : w))) return BT709HIP_ERR_STRIDE;
      if (af.y_stride > 0xffffffffu || (!alpha_no_cbcr && af.cbcr_stride > 0xffffffffu)) return BT709HIP_ERR_STRIDE;
      fast = fast && aligned(af.y, pair_y_align) && aligned(af.cbcr, pair_chroma_align);
      if (i >= 2)
        uniform = uniform && byte_step(alpha0.y, af.y) == byte_step(alpha0.y, outs[count + 1].y) * i &&
                  byte_step(alpha0.cbcr, af.cbcr) == byte_step(alpha0.cbcr, outs[count + 1].cbcr) * i;
      if (i < kMaxPairBatch) {  // the frames[] area as 16 pairs (bt709_kernels.h EncodePair): never both tables
        EncodePair &e = p.pairs[i];
        e.bgra = static_cast<const uint8_t *>(in.bgra);
        e.y = static_cast<uint8_t *>(const_cast<void *>(out.y));
        e.cbcr = static_cast<uint8_t *>(const_cast<void *>(out.cbcr));
        e.alpha_y = static_cast<uint8_t *>(const_cast<void *>(af.y));
        e.alpha_cbcr = static_cast<uint8_t *>(const_cast<void *>(af.cbcr));
      }
    } else if (i < (chw ? kMaxChwBatch : kMaxBatch)) {  // a CHW launch: one entry fewer, scale and bias in its place
      p.frames[i].bgra = static_cast<const uint8_t *>(in.bgra);
      p.frames[i].y = static_cast<uint8_t *>(const_cast<void *>(out.y));
      p.frames[i].cbcr = static_cast<uint8_t *>(const_cast<void *>(out.cbcr));
    }
  }
  if (count > (uniform ? kMaxUniformBatch : pair ? kMaxPairBatch : chw ? kMaxChwBatch : kMaxBatch)) return BT709HIP_ERR_UNSUPPORTED;
  // the reference's per-pixel converters take sRGB bytes only, and no alpha clip goes through them
  if (convert != BT709HIP_CONVERT_OFF && (alpha || input_gamma != BT709HIP_GAMMA_SRGB)) return BT709HIP_ERR_UNSUPPORTED;
  if (with_alpha && (!pair || half)) return BT709HIP_ERR_UNSUPPORTED;  // the converter writes no alpha frame; an alpha clip has none beside itself; halves have an option of their own
  // half input composes with the chroma layout alone: the converter, the pair and the premultiply are BGRA8 paths
  if (half && (convert_option != BT709HIP_CONVERT_OFF || ctx->encode_premultiply != 0)) return BT709HIP_ERR_UNSUPPORTED;
  // so does CHW input; the half pair's option is an option of another input, but away from its default it is refused all the same
  if (chw && (convert_option != BT709HIP_CONVERT_OFF || ctx->encode_premultiply != 0 || ctx->encode_half_with_alpha != 0)) return BT709HIP_ERR_UNSUPPORTED;
  if (in0.width == 0 || in0.height == 0) return BT709HIP_OK;
  if (int rc = bind(ctx)) return rc;
  FLUSH_STREAM(ctx, stream);

  hipStream_t s = pick(ctx, stream);
  if (convert != BT709HIP_CONVERT_OFF) {
    if (int rc = convert_curve_table(ctx, output_gamma, s)) return rc;
    p.convert_curve = static_cast<const float *>(ctx->d_convert_curve[output_gamma]);
    p.convert_mode = static_cast<uint16_t>(convert);
  } else if (alpha) {
    if (int rc = alpha_luma_table(ctx, s)) return rc;
    p.alpha_luma = static_cast<const uint32_t *>(ctx->d_alpha_luma);
  } else {
    EncoderTables &t = ctx->encoders[input_gamma][output_gamma];
    if (int rc = encoder_tables(ctx, input_gamma, output_gamma, s)) return rc;
    p.per_byte = static_cast<const EncodeByteEntry *>(t.d_per_byte);
    p.from_linear = static_cast<const TransferBucket *>(t.d_from_linear);
    p.from_linear_bytes = t.from_linear_bytes;
    p.from_linear_scale = static_cast<float>(t.from_linear_n);
    p.from_linear_coarse = t.coarse_scale;
    p.from_linear_offset = t.coarse_offset;
    if (pair) {  // both sets of tables: launch_encode's selector of the paired kernels
      if (int rc = alpha_luma_table(ctx, s)) return rc;
      p.alpha_luma = static_cast<const uint32_t *>(ctx->d_alpha_luma);
    }
  }

  if (uniform) {
    p.uniform = 1;
    p.step_bgra = byte_step(ins[0].bgra, ins[1].bgra);
    p.step_y = byte_step(outs[0].y, outs[1].y);
    p.step_cbcr = byte_step(outs[0].cbcr, outs[1].cbcr);
    if (pair) {
      p.pairs[1].spare = byte_step(alpha0.y, outs[count + 1].y);
      p.pairs[2].spare = byte_step(alpha0.cbcr, outs[count + 1].cbcr);
    }
  }
  if (pair)  // the alpha frames' pitches: the spare slot of pair 0
    p.pairs[0].spare = static_cast<int64_t>(static_cast<uint64_t>(alpha0.y_stride) | (alpha_no_cbcr ? 0ull : static_cast<uint64_t>(alpha0.cbcr_stride) << 32));
  p.row_pairs_per_block = static_cast<uint32_t>(ctx->encode_row_pairs);  // 0: sized per launch
  p.block_threads = static_cast<uint32_t>(ctx->encode_threads);
  p.width = static_cast<uint32_t>(in0.width);
  p.height = static_cast<uint32_t>(in0.height);
  p.bgra_stride = static_cast<uint32_t>(in0.stride);
  p.y_stride = static_cast<uint32_t>(out0.y_stride);
  p.cbcr_stride = no_cbcr ? 0u : static_cast<uint32_t>(out0.cbcr_stride);
  p.chroma_layout = planar ? kChromaI420 : kChromaNV12;
  p.premultiply = premultiply ? 1 : 0;
  p.input_format = half ? kEncodeInputRGBA16F : kEncodeInputBGRA8;  // per_byte is built with the pair's tables and not read
  if (chw) {  // the element type, and the six values, each read once: kernel arguments, nothing staged (CHW_U8 ignores them)
    p.input_format = static_cast<uint8_t>(kEncodeInputCHWU8 + (in0.format - BT709HIP_FORMAT_CHW_U8));
    for (int c = 0; c < 3; ++c) {
      const uint32_t scale = ctx->encode_chw_norm[c], bias = ctx->encode_chw_norm[3 + c];
      std::memcpy(&p.chw.scale[c], &scale, sizeof scale);
      std::memcpy(&p.chw.bias[c], &bias, sizeof bias);
    }
  }
  last_launch_shape() = LaunchShape{};
  set_kernel_name(launch_encode(p, count, fast, ctx->xcd_bands != 0, s));
  HIP_TRY(hipGetLastError());
  if (wait_until_completed) HIP_TRY(hipStreamSynchronize(s));
  return BT709HIP_OK;
}

int bt709hip_encoder_prepare(bt709hip_context *ctx, int input_gamma, int output_gamma) {
  if (ctx == nullptr) return BT709HIP_ERR_INVALID_ARG;
  // ITU709 is an output gamma of the per-pixel converter alone (BT709HIP_CTX_OPT_ENCODE_CONVERT), which reads sRGB bytes only
  if (input_gamma < 0 || input_gamma > 2 || output_gamma < 0 || output_gamma > 3 || (output_gamma == 3 && input_gamma != BT709HIP_GAMMA_SRGB))
    return BT709HIP_ERR_INVALID_ARG;
  if (int rc = bind(ctx)) return rc;
  if (input_gamma == BT709HIP_GAMMA_SRGB)  // the converter's curve as well: 1 KiB
    if (int rc = convert_curve_table(ctx, output_gamma, nullptr)) return rc;
  if (output_gamma == 3) return BT709HIP_OK;  // no subsampling encoder writes ITU709
  // T: the one gamma pair BGRA8_ALPHA input encodes with; under BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA every pair's alpha frame reads it
  // (and under BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA every half pair's, whose input gamma is LINEAR)
  if ((input_gamma == BT709HIP_GAMMA_LINEAR && (output_gamma == BT709HIP_GAMMA_LINEAR || ctx->encode_half_with_alpha != 0)) || ctx->encode_with_alpha != 0)
    if (int rc = alpha_luma_table(ctx, nullptr)) return rc;
  return encoder_tables(ctx, input_gamma, output_gamma, nullptr);
}

int bt709hip_encode(bt709hip_context *ctx, const bt709hip_surface *in, const bt709hip_frame *out, int input_gamma,
                    int output_gamma, void *stream, int wait_until_completed) {
  if (in == nullptr || out == nullptr) return BT709HIP_ERR_INVALID_ARG;
  return bt709hip_encode_batch(ctx, 1, in, out, input_gamma, output_gamma, stream, wait_until_completed);
}

// ------------------------------------------------------------ plane layouts

static int planes_call(bt709hip_context *ctx, const void *u, size_t u_stride, const void *v, size_t v_stride,
                       void *cbcr, size_t cbcr_stride, int cw, int ch, bool interleave, void *stream, int wait) {
  if (ctx == nullptr || cw < 0 || ch < 0) return BT709HIP_ERR_INVALID_ARG;
  if (cw == 0 || ch == 0) return BT709HIP_OK;
  if (u == nullptr || v == nullptr || cbcr == nullptr) return BT709HIP_ERR_INVALID_ARG;
  const size_t w = static_cast<size_t>(cw);
  if (u_stride < w || v_stride < w || cbcr_stride < 2 * w) return BT709HIP_ERR_STRIDE;
  if (u_stride > 0xffffffffu || v_stride > 0xffffffffu || cbcr_stride > 0xffffffffu) return BT709HIP_ERR_STRIDE;
  if (ch > kMaxGridYZ) return BT709HIP_ERR_UNSUPPORTED;  // one chroma row per gridDim.y
  if (int rc = bind(ctx)) return rc;
  FLUSH_STREAM(ctx, stream);
  PlaneParams p;
  std::memset(&p, 0, sizeof p);
  p.u = static_cast<const uint8_t *>(u);
  p.v = static_cast<const uint8_t *>(v);
  p.cbcr = static_cast<uint8_t *>(cbcr);
  p.u_stride = static_cast<uint32_t>(u_stride);
  p.v_stride = static_cast<uint32_t>(v_stride);
  p.cbcr_stride = static_cast<uint32_t>(cbcr_stride);
  p.chroma_width = static_cast<uint32_t>(cw);
  p.chroma_height = static_cast<uint32_t>(ch);
  p.wide = (cw % 8) == 0 && (u_stride % 8) == 0 && (v_stride % 8) == 0 && (cbcr_stride % 16) == 0 && aligned(u, 8) &&
           aligned(v, 8) && aligned(cbcr, 16);
  hipStream_t s = pick(ctx, stream);
  last_launch_shape() = LaunchShape{};
  set_kernel_name(launch_planes(p, interleave, s));
  HIP_TRY(hipGetLastError());
  if (wait) HIP_TRY(hipStreamSynchronize(s));
  return BT709HIP_OK;
}

int bt709hip_interleave_cbcr(bt709hip_context *ctx, const void *u, size_t u_stride, const void *v, size_t v_stride,
                             void *cbcr, size_t cbcr_stride, int chroma_width, int chroma_height, void *stream,
                             int wait_until_completed) {
  return planes_call(ctx, u, u_stride, v, v_stride, cbcr, cbcr_stride, chroma_width, chroma_height, true, stream,
                     wait_until_completed);
}

int bt709hip_deinterleave_cbcr(bt709hip_context *ctx, const void *cbcr, size_t cbcr_stride, void *u, size_t u_stride,
                               void *v, size_t v_stride, int chroma_width, int chroma_height, void *stream,
                               int wait_until_completed) {
  return planes_call(ctx, u, u_stride, v, v_stride, const_cast<void *>(cbcr), cbcr_stride, chroma_width, chroma_height,
                     false, stream, wait_until_completed);
}

}  // extern "C"
