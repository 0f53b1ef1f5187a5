/*
 * bt709hip_ext.h -- the part of the C ABI of libbt709hip.so that has NO twin in the reference: what a discrete HBM
 * device needs around the decode operator (frames resident in a ring whose placement is hunted for, rings on several
 * GPUs, frames fed from host memory through an in-flight pool or a multi-GPU sharder), what keeps the reference's
 * one-call-per-frame cadence fast (coalescing submit, graphs), batched forms of the side paths, tuning options,
 * timing events and the introspection calls the parity tests use.  bt709hip.h holds the reference-twinned calls; both
 * headers describe ONE library and ONE ABI number (BT709HIP_VERSION).
 */
#ifndef BT709HIP_EXT_H
#define BT709HIP_EXT_H

#include "bt709hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bt709hip_pool bt709hip_pool; /* ~ CVPixelBufferPool + texture cache + in-flight semaphore */

/* ------------------------------------------------------------ device, options */
typedef struct {
  int32_t device_ordinal;
  int32_t compute_units;
  int32_t wavefront_size;
  int32_t lds_bytes_per_block;
  int32_t memory_clock_khz;
  int32_t memory_bus_width_bits;
  int32_t l2_bytes;
  int32_t clock_khz;
  uint64_t total_memory_bytes;
  char name[128];
  char arch[64];
  /* Which physical device this is, for callers that must prove N contexts sit on N GPUs (bench.py's per-rank records; device
   * ordinals are per process and say nothing once HIP_VISIBLE_DEVICES differs between ranks): hipDeviceGetPCIBusId
   * ("0000:c1:00.0") and the 16 bytes of hipDeviceGetUuid -- as they are when they are printable text (ROCm: the 16 characters
   * rocm-smi shows as the unique id), as 32 hex digits otherwise.  MTLDevice has registryID for this
   * (the reference keeps one device, Renderer/MetalRenderContext.m:59-63, and never needs it). */
  char pci_bus_id[32];
  char uuid[40];
} bt709hip_device_info;
int bt709hip_context_info(const bt709hip_context *ctx, bt709hip_device_info *info);

/* Launch-shape knobs of a context (tuning and test hooks; no reference twin).  Values are
 * clamped to their valid range; 0 restores the default.  BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT,
 * BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY, BT709HIP_CTX_OPT_ENCODE_CONVERT, BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA,
 * BT709HIP_CTX_OPT_ENCODE_HALF_INPUT, BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA, BT709HIP_CTX_OPT_ENCODE_CHW_INPUT and the six
 * BT709HIP_CTX_OPT_ENCODE_CHW_SCALE_* / _BIAS_* are no knobs and are NOT clamped: see below. */
typedef enum {
  BT709HIP_CTX_OPT_GRID_MULT = 1,       /* general (unaligned-layout) kernels: workgroups per launch = CUs x 8 x this; default 2 */
  BT709HIP_CTX_OPT_ENCODE_ROW_PAIRS = 2,/* encoder: consecutive row pairs per workgroup; default 0 = sized per launch */
  BT709HIP_CTX_OPT_ENCODE_THREADS = 3,  /* encoder: lanes per workgroup (rounded down to whole waves); default 0 = from the width */
  BT709HIP_CTX_OPT_XCD_BANDS = 4,       /* encoder: 1 (default) XCD-aware work map for launches of a multiple of 8 pictures; 0 plain order */
  BT709HIP_CTX_OPT_STREAMING_TRIES = 5, /* device buffers of 256 MB or more that the library allocates itself (in-flight pool slots, the sharder's lanes) go through bt709hip_malloc_streaming with this many candidates; default 4, 1 = plain allocation */
  BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT = 6, /* BT709HIP_CHROMA_NV12 (default) or BT709HIP_CHROMA_I420: the planes bt709hip_encode[_batch] writes; any other value is refused */
  BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY = BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT + 2, /* (eight; seven is no option) 0 (default): BGRA8_SRGB input is encoded as it is; 1: it is straight alpha and is premultiplied first; any other value is refused */
  BT709HIP_CTX_OPT_ENCODE_CONVERT = BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY + 2, /* (ten; nine is no option) BT709HIP_CONVERT_OFF (default), _PACKED444 or _POINT420: bt709hip_encode[_batch] is the reference's per-pixel +convert:; any other value is refused */
  BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA = BT709HIP_CTX_OPT_ENCODE_CONVERT + 2, /* (twelve; eleven is no option) 0 (default): one frame per picture; 1: bt709hip_encode[_batch] of BGRA8_SRGB input writes the picture's alpha frame as well, `out` holds TWO frames per picture; any other value is refused */
  BT709HIP_CTX_OPT_ENCODE_HALF_INPUT = BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA + 2, /* (fourteen; thirteen is no option) 0 (default): RGBA16F input to bt709hip_encode[_batch] is BT709HIP_ERR_UNSUPPORTED; 1: it is encoded as linear light; any other value is refused */
  BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA = BT709HIP_CTX_OPT_ENCODE_HALF_INPUT + 2, /* (sixteen; fifteen and seventeen are no options) 0 (default): one frame per picture; 1: bt709hip_encode[_batch] of RGBA16F input (under _ENCODE_HALF_INPUT = 1) writes the surface's alpha frame as well, `out` holds TWO frames per picture; any other value is refused */
  BT709HIP_CTX_OPT_ENCODE_CHW_INPUT = BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA + 2, /* (eighteen; seventeen and nineteen are no options) 0 (default): planar CHW input to bt709hip_encode[_batch] is what any unknown format is; 1: CHW_U8 / _F16 / _F32 surfaces are encoded; any other value is refused */
  BT709HIP_CTX_OPT_ENCODE_CHW_SCALE_R = BT709HIP_CTX_OPT_ENCODE_CHW_INPUT + 2, /* (twenty) twenty to twenty-five: the BIT PATTERN of a binary32 each -- scale (default 1.0f) and bias (default 0.0f) of the R, G and B plane of float CHW input; +-0 or finite with 2^-64 <= |x| <= 2^64, anything else is refused */
  BT709HIP_CTX_OPT_ENCODE_CHW_SCALE_G = BT709HIP_CTX_OPT_ENCODE_CHW_SCALE_R + 1,
  BT709HIP_CTX_OPT_ENCODE_CHW_SCALE_B = BT709HIP_CTX_OPT_ENCODE_CHW_SCALE_G + 1,
  BT709HIP_CTX_OPT_ENCODE_CHW_BIAS_R = BT709HIP_CTX_OPT_ENCODE_CHW_SCALE_B + 1,
  BT709HIP_CTX_OPT_ENCODE_CHW_BIAS_G = BT709HIP_CTX_OPT_ENCODE_CHW_BIAS_R + 1,
  BT709HIP_CTX_OPT_ENCODE_CHW_BIAS_B = BT709HIP_CTX_OPT_ENCODE_CHW_BIAS_G + 1 /* (twenty-five) */
} bt709hip_context_option;
#define BT709HIP_CONVERT_OFF 0       /* bt709hip_encode[_batch] is the subsampling encoder (+convertIntoCoreVideoBuffer:) */
#define BT709HIP_CONVERT_PACKED444 1 /* +convert: -- one 32-bit word (Cr<<16)|(Cb<<8)|Y per pixel */
#define BT709HIP_CONVERT_POINT420 2  /* +convert: then copyBT709ToCoreVideo in one launch: an NV12 / I420 frame, chroma point-sampled */
int bt709hip_context_set_option(bt709hip_context *ctx, int option, int value);
/* BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT.  The reference's encoder exists to write YUV4MPEG2 files, whose FRAME is planar: Y, then
 * U, then V (Renderer/y4m_writer.h:194-241).  With the option at BT709HIP_CHROMA_I420 (the values are BT709HIP_OPT_CHROMA_LAYOUT's,
 * defined below) the bt709hip_frame that bt709hip_encode and bt709hip_encode_batch WRITE is three planes, in the convention of
 * the decode side, with no de-interleave pass and no scratch plane:
 *   y, y_stride   as before;
 *   cbcr          the U (Cb) plane: (W/2) x (H/2) bytes, rows cbcr_stride bytes apart, cbcr_stride >= W/2;
 *   the V (Cr) plane has the same pitch and starts at cbcr + (height/2) * cbcr_stride (a 64-bit product).
 * U[r][c] and V[r][c] are bytes 2c and 2c+1 of row r of the CbCr plane the NV12 encode of the same picture writes, Y is that
 * encode's Y; nothing outside the three planes' samples is written (row padding, a gap between U's last row and V's first, bytes
 * behind V).  A tight FRAME payload is y = base, y_stride = W, cbcr = base + W*H, cbcr_stride = W/2: one contiguous download of
 * W*H*3/2 bytes is the payload.  Validation: cbcr_stride < W/2 is BT709HIP_ERR_STRIDE (NV12: < W); every other check and limit
 * is NV12's; an evenly spaced batch is one whose BGRA, Y and U pointers are (V follows from U).  The fast kernel needs
 * W % 4 == 0, the BGRA pointer and pitch 16-byte aligned, Y 4-byte, the U pointer and cbcr_stride 2-byte; any other call takes
 * the general kernel.  Launch plans (bt709hip_last_launch_info) are the NV12 encoder's for the same size and count, and
 * BT709HIP_CTX_OPT_ENCODE_ROW_PAIRS, _ENCODE_THREADS and _XCD_BANDS apply as they do there.  bt709hip_last_kernel_name:
 * "encode_bgra_i420", "encode_bgra_i420_blocks".  BGRA8_ALPHA input with chroma planes: every U and V byte is 128
 * ("encode_alpha_y<i420>", "encode_alpha_y_blocks<i420>"); with cbcr == NULL only Y is written, by the same kernels under the
 * same names as under NV12.  The call reads the option once, on entry.  Any value but the two: BT709HIP_ERR_INVALID_ARG, the
 * option keeps its value (the other context options clamp; this one does not).  Setting it never touches the device and needs
 * no table: it works while a stream is being captured.  Under BT709HIP_CHROMA_NV12 nothing changes. */
/* BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY.  Every alpha path here works on PREMULTIPLIED colour, because the reference's does: its
 * encoder tool renders the picture into a kCGImageAlphaPremultipliedFirst bitmap (Renderer/CGFrameBuffer.m:417,
 * srgb_to_bt709.m:805-811) and CoreGraphics multiplies on the way.  A PNG, an RGBA tensor and a compositor's export hold STRAIGHT
 * alpha.  With the option at 1, bt709hip_encode and bt709hip_encode_batch replace B, G, R of each BGRA8_SRGB texel by
 *   c' = (c * A + 127) / 255        c, A in 0..255, integer division; A = 255: c' = c, A = 0: c' = 0
 * inside the encode kernel, before anything else reads them (definition: DESIGN.md 3.9; CoreGraphics is a closed box, the rounding
 * is ours): the planes written are bit for bit those of the plain encode of the premultiplied picture, with no pass over it and
 * no scratch picture.  Covered: every gamma pair, both chroma layouts, fast and general kernels, pointer-table and evenly spaced
 * batches; validation, limits and launch plans (bt709hip_last_launch_info) are the plain encoder's.  BGRA8_ALPHA input reads A
 * alone and is unaffected: same kernels, same names, same bytes.  bt709hip_last_kernel_name: "encode_bgra_nv12<premul>",
 * "encode_bgra_nv12_blocks<premul>", "encode_bgra_i420<premul>", "encode_bgra_i420_blocks<premul>".  The call reads the option
 * once, on entry.  Any value but 0 and 1: BT709HIP_ERR_INVALID_ARG, the option keeps its value (it is not clamped).  Setting it
 * never touches the device and needs no table: it works while a stream is being captured.  At 0 nothing changes. */
/* BT709HIP_CTX_OPT_ENCODE_CONVERT.  The reference has a SECOND BGRA -> BT.709 converter, the per-pixel pair +convert: /
 * +unconvert: (Renderer/BGRAToBT709Converter.h:34-46); every reference XCTest builds its input frame as +convert: then
 * copyBT709ToCoreVideo then -decodeBT709: (MetalBT709DecoderTests.m:189-277).  It is not the subsampling encoder: it keeps floats
 * end to end (no byte-quantised intermediate) and samples per pixel (no 2x2 average), so its bytes differ.  Per pixel, with
 * n[c] = curve(byteNorm(c)) for c = R, G, B (A is ignored):
 *   Ey = (Kr*n[R] + Kg*n[G]) + Kb*n[B];  Eb = (n[B] - Ey) / 1.8556f;  Er = (n[R] - Ey) / 1.5748f          (BT709.h:199-268)
 *   Y = round(Ey*219 + 16), Cb = round(Eb*224 + 128), Cr = round(Er*224 + 128)
 * and curve, by output_gamma: SRGB the identity (BT709.h:914-944); LINEAR sRGB -> linear; APPLE sRGB -> linear -> Apple 1.961
 * (Apple196_from_sRGB_convertRGBToYCbCr, BT709.h:743-817); ITU709 sRGB -> linear -> BT.709 (BT709_from_sRGB_convertRGBToYCbCr(., 1),
 * the else branch of convertSoftware) -- +unconvert:'s four modes.  With the option at
 *   BT709HIP_CONVERT_OFF (0, the default): nothing changes -- same kernels, same names, same bytes; output_gamma ITU709 stays
 *     BT709HIP_ERR_INVALID_ARG;
 *   BT709HIP_CONVERT_PACKED444 (1), the +convert: twin: out->y points to W x H 32-bit words (Cr<<16)|(Cb<<8)|Y, the top byte of
 *     each word 0, rows y_stride bytes apart -- what bt709hip_unconvert reads.  out->cbcr must be NULL in every frame
 *     (BT709HIP_ERR_INVALID_ARG otherwise); cbcr_stride and the tags are not looked at.  y_stride >= 4*W, a multiple of 4, the
 *     pointer 4-byte aligned (BT709HIP_ERR_STRIDE otherwise).  An evenly spaced batch is one whose BGRA and word pointers are;
 *   BT709HIP_CONVERT_POINT420 (2), +convert: followed by copyBT709ToCoreVideo (BGRAToBT709Converter.m:1042-1099) in one launch
 *     with no packed intermediate: `out` is an ordinary NV12 frame, or three planes under BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT =
 *     BT709HIP_CHROMA_I420.  Y of pixel (r, c) is the converted pixel's Y; Cb and Cr of block (r/2, c/2) are those of the converted
 *     pixel in the block's ODD row and EVEN column (the odd-row rule: every row of the reference's copy overwrites chroma row
 *     r/2, so the odd row's pair survives).
 * Under 1 and 2: input_gamma must be BT709HIP_GAMMA_SRGB (the reference's per-pixel converters take sRGB bytes only) and
 * in->format BGRA8_SRGB -- any other input gamma, and BGRA8_ALPHA input, is BT709HIP_ERR_UNSUPPORTED after the usual validation;
 * output_gamma may be APPLE, SRGB, LINEAR or ITU709.  BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY composes: B, G, R are premultiplied
 * first, then converted.  Every other check, its order and its limit are the encoder's (even and equal sizes, height/2 <= 65535,
 * pitches <= 2^32 - 1, 32 pictures in a pointer table, 65535 evenly spaced).  Launch plans (bt709hip_last_launch_info) are the
 * plain encoder's for the same size and count; BT709HIP_CTX_OPT_ENCODE_ROW_PAIRS, _ENCODE_THREADS and _XCD_BANDS apply as they do
 * there.  The fast kernels need W % 4 == 0 and the BGRA pointer and pitch 16-byte aligned, and for the words a 16-byte aligned
 * pointer and pitch (for a frame: the encoder's alignments); any other call takes the general kernel.
 * bt709hip_last_kernel_name: "convert_bgra_packed444", "convert_bgra_packed444_blocks", "convert_bgra_nv12", "convert_bgra_i420",
 * "convert_bgra_nv12_blocks", "convert_bgra_i420_blocks", and the same names with "<premul>" behind them.  The one table is 256
 * floats per output gamma, built per context by the first call that needs it or by bt709hip_encoder_prepare(ctx,
 * BT709HIP_GAMMA_SRGB, output_gamma) -- which accepts ITU709 for this table alone; a call that finds it missing while its stream is
 * being captured returns BT709HIP_ERR_NOT_SETUP.  The call reads the option once, on entry.  Any value but the three:
 * BT709HIP_ERR_INVALID_ARG, the option keeps its value (it is not clamped).  Setting it never touches the device: it works while
 * a stream is being captured. */
/* BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA.  The reference's `srgb_to_bt709 -alpha` turns ONE BGRA picture into TWO clips: the colour as
 * a BT.709 frame and the A channel as a second, linear frame (<name>_alpha.y4m; srgb_to_bt709.m:842-954).  bt709hip_decode takes
 * the pair back in one launch (frame + alpha); with this option at 1 and in->format == BT709HIP_FORMAT_BGRA8_SRGB the encode side
 * writes the pair in one launch, from one read of the surface:
 *   bt709hip_encode(ctx, in, out, gi, go, ...): `out` points to TWO bt709hip_frames.  out[0] receives the colour frame, byte for
 *     byte what the call writes with the option at 0 (same gammas, BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT, _ENCODE_PREMULTIPLY);
 *     out[1] receives the alpha frame, byte for byte what a BGRA8_ALPHA call on the same surface writes: Y = T[A], and
 *     Cb = Cr = 128 if it has a chroma plane.  gi and go govern the colour alone: the alpha frame is the (Linear, Linear) one
 *     whatever they are.  A is read from the texel as stored, premultiplying or not;
 *   bt709hip_encode_batch(ctx, count, ins, outs, ...): `outs` holds 2 * count frames; the colour frames are outs[0 .. count),
 *     pair i's alpha frame is outs[count + i].
 * The alpha frames follow BGRA8_ALPHA output's rules: the surface's width and height (BT709HIP_ERR_SIZE_MISMATCH); y non-NULL;
 * W <= y_stride <= 2^32 - 1 (BT709HIP_ERR_STRIDE); cbcr NULL in EVERY alpha frame of the call or in none
 * (BT709HIP_ERR_INVALID_ARG); a chroma plane follows the layout option -- under BT709HIP_CHROMA_I420 a U plane with V
 * (H/2) * cbcr_stride behind it, every byte 128, cbcr_stride >= W/2, under NV12 >= W; equal pitches across the batch
 * (BT709HIP_ERR_SIZE_MISMATCH).  Evenly spaced batches: all five planes (BGRA, Y, CbCr, alpha Y, alpha CbCr when present) must be
 * evenly spaced, then any count up to 65535 goes; any two pairs always are.  Otherwise a pointer table, which holds
 * BT709HIP_MAX_BATCH / 2 = 16 PAIRS here (the kernel argument block does not grow): more is BT709HIP_ERR_UNSUPPORTED.  The fast
 * kernel needs, beside the colour encoder's alignments, the alpha Y pointer, pitch and step 4-byte aligned and the alpha chroma
 * plane aligned as the colour's; any other call takes the general kernel and writes the same bytes.  Refused with
 * BT709HIP_ERR_UNSUPPORTED after the usual validation, nothing enqueued: the option at 1 together with
 * BT709HIP_CTX_OPT_ENCODE_CONVERT != BT709HIP_CONVERT_OFF, and the option at 1 with BGRA8_ALPHA input.  Colour and alpha planes
 * that overlap are the caller's error.  bt709hip_encoder_prepare(ctx, gi, go) builds T as well when the option is 1 at the time
 * of the call: a paired encode can be captured into a graph after that one prepare (BT709HIP_ERR_NOT_SETUP while capturing
 * otherwise).  bt709hip_last_kernel_name: "encode_bgra_alpha_nv12", "encode_bgra_alpha_i420", "encode_bgra_alpha_nv12_blocks",
 * "encode_bgra_alpha_i420_blocks", and the same names with "<premul>" behind them.  bt709hip_last_launch_info: the colour
 * encoder's plan for the same size and count; BT709HIP_CTX_OPT_ENCODE_ROW_PAIRS, _ENCODE_THREADS and _XCD_BANDS apply as they do
 * there.  The call reads the option once, on entry.  Any value but 0 and 1: BT709HIP_ERR_INVALID_ARG, the option keeps its value
 * (it is not clamped).  Setting it never touches the device: it works while a stream is being captured.  At 0 nothing changes. */
/* BT709HIP_CTX_OPT_ENCODE_HALF_INPUT.  The decoder writes two target formats, BGRA8_SRGB and RGBA16F (linear light); a caller who
 * decodes into RGBA16F, blends, filters or grades there and wants a frame for an H.264 encoder needs the way back.  With the
 * option at 1, bt709hip_encode and bt709hip_encode_batch accept in->format == BT709HIP_FORMAT_RGBA16F: texels of four binary16
 * values R, G, B, A in memory order, A is not read.  The definition is BT709_average_pixel_values
 * (BT709.h:1349-1509) with the result of BT709_tolinearNorm replaced by the texel's own values; per 2x2 block, pixels TL, TR, BL, BR:
 *   v[i][c]    = sat(float(h[i][c]))      exact half -> float; sat: NaN -> 0, v < 0 (and -0) -> 0, v > 1 (and +inf) -> 1
 *   byte[i][c] = BT709_from_linear(v[i][c], output_gamma)                                      (BT709.h:1150-1167)
 *   Y[i]       = Y of sRGB_from_sRGB_convertRGBToYCbCr(byte[i][R,G,B])                           (BT709.h:914-944 -> 199-268)
 *   ave[c]     = (((v[0][c] + v[1][c]) + v[2][c]) + v[3][c]) / 4.0f                             (BT709.h:1171-1190)
 *   (Cb, Cr)   = Cb, Cr of sRGB_from_sRGB_convertRGBToYCbCr(BT709_from_linear(ave[R,G,B], output_gamma))
 * bit for bit, in one launch that reads 8 and writes 1.5 bytes per pixel.  input_gamma must be BT709HIP_GAMMA_LINEAR (the texels
 * hold linear light): anything else is BT709HIP_ERR_TRANSFER.  output_gamma is APPLE, SRGB or LINEAR, as for BGRA8 input.
 * BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT is honoured: NV12 and I420 both work.  Validation follows the encoder's order and writes
 * and enqueues nothing on refusal: in->bgra not 8-byte aligned, in->stride no multiple of 8 or below 8 * W is
 * BT709HIP_ERR_STRIDE (the rule of an RGBA16F decode target); reserved != 0 and a batch of mixed formats are what they were
 * (BT709HIP_ERR_UNSUPPORTED, BT709HIP_ERR_SIZE_MISMATCH).  OUT OF SCOPE, refused with BT709HIP_ERR_UNSUPPORTED behind the usual
 * validation: BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY, BT709HIP_CTX_OPT_ENCODE_CONVERT or BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA away from its
 * default while the input is RGBA16F (no straight-alpha halves, no alpha frame from a half surface's A, no +convert: from halves,
 * no ITU709 output).  Sizes, the even-dimension rule, height / 2 <= 65535, BT709HIP_MAX_BATCH pictures in a pointer table, 65535
 * evenly spaced, wait_until_completed and the flush of coalescing queues on the stream are the BGRA8 encoder's.  The fast kernel
 * needs the texel pointer and pitch 16-byte aligned, the Y pointer and pitch 2-byte aligned and, under NV12, the CbCr pointer and
 * pitch 2-byte aligned (any even W; U and V take any alignment); every other valid call takes the general kernel (byte stores)
 * and writes the same bytes.  bt709hip_last_kernel_name: "encode_rgba16f_nv12", "encode_rgba16f_i420", "encode_rgba16f_nv12_blocks",
 * "encode_rgba16f_i420_blocks".  bt709hip_last_launch_info: a lane of the fast kernel owns a 2x2 block where the BGRA8 kernel's
 * owns a 4x2 quad, so the plan is the BGRA8 encoder's plan for a picture TWICE AS WIDE, same height and count;
 * BT709HIP_CTX_OPT_ENCODE_ROW_PAIRS, _ENCODE_THREADS (lanes = blocks per tile) and _XCD_BANDS are read as they are there;
 * BT709HIP_CTX_OPT_GRID_MULT and _STREAMING_TRIES are ignored.  Tables: the (LINEAR, output_gamma) encoder's own
 * BT709_from_linear table, built by the first call that needs it or by bt709hip_encoder_prepare(ctx, BT709HIP_GAMMA_LINEAR,
 * output_gamma) -- which makes everything the half path needs; a call that finds the table missing while its stream is being
 * captured returns BT709HIP_ERR_NOT_SETUP.  BGRA8_SRGB and BGRA8_ALPHA input behave exactly as before with the option at either
 * value: same kernels, same names, same bytes.  The call reads the option once, on entry.  Any value but 0 and 1:
 * BT709HIP_ERR_INVALID_ARG, the option keeps its value (it is not clamped).  Setting it never touches the device: it works while a
 * stream is being captured.  At 0 (the default) nothing changes: RGBA16F input is BT709HIP_ERR_UNSUPPORTED. */
/* BT709HIP_CTX_OPT_ENCODE_HALF_WITH_ALPHA.  bt709hip_decode of a frame and an alpha frame into an RGBA16F surface writes premultiplied
 * linear colour and a linear A; with this option at 1, BT709HIP_CTX_OPT_ENCODE_HALF_INPUT at 1 and in->format ==
 * BT709HIP_FORMAT_RGBA16F the encode side writes the two frames back in one launch, from one read of the surface:
 *   bt709hip_encode(ctx, in, out, BT709HIP_GAMMA_LINEAR, go, ...): `out` points to TWO bt709hip_frames.  out[0] receives the colour
 *     frame, byte for byte what the call writes with the option at 0 (same output gamma, BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT);
 *     out[1] receives the alpha frame: what the option-0 call writes under (LINEAR, LINEAR) for the surface whose R, G and B are
 *     replaced by its A -- the reference's alpha clip is the grey picture (A,A,A) with the gamma forced to linear
 *     (srgb_to_bt709.m:842-954), and BT709_from_linear(v, Linear) is (int)round(v * 255.0f) (BT709.h:1150-1167).  Per pixel
 *       a = sat(float(hA))     exact half -> float; NaN -> 0, a < 0 (and -0) -> 0, a > 1 (and +inf) -> 1
 *       Y = T[round(a * 255)]  T: the alpha frames' luma table (BGRA8_ALPHA input's)
 *     and Cb = Cr = 128 if it has a chroma plane.  go governs the colour alone; input_gamma must be BT709HIP_GAMMA_LINEAR
 *     (BT709HIP_ERR_TRANSFER);
 *   bt709hip_encode_batch(ctx, count, ins, outs, ...): `outs` holds 2 * count frames; the colour frames are outs[0 .. count),
 *     pair i's alpha frame is outs[count + i].
 * The alpha frames are validated as BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA's, in that order: the surface's width and height
 * (BT709HIP_ERR_SIZE_MISMATCH); y non-NULL; cbcr NULL in EVERY alpha frame of the call or in none (BT709HIP_ERR_INVALID_ARG);
 * W <= y_stride <= 2^32 - 1, cbcr_stride >= W, or >= W/2 under BT709HIP_CHROMA_I420 (BT709HIP_ERR_STRIDE); equal pitches across the
 * batch.  The layout option covers both frames of a pair.  Evenly spaced batches: all five planes evenly spaced, then any count up
 * to 65535 goes; otherwise a pointer table of BT709HIP_MAX_BATCH / 2 = 16 PAIRS (the kernel argument block does not grow): more is
 * BT709HIP_ERR_UNSUPPORTED.  The fast kernel needs, beside the half encoder's alignments, the alpha Y pointer, pitch and step 2-byte
 * aligned and, under NV12, the alpha CbCr pointer and pitch 2-byte aligned; any other valid call takes the general kernel and writes
 * the same bytes.  Everything else stays: BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA, _ENCODE_PREMULTIPLY or _ENCODE_CONVERT away from its
 * default with half input is BT709HIP_ERR_UNSUPPORTED behind the usual validation; BGRA8_SRGB and BGRA8_ALPHA input do not read this
 * option; RGBA16F input with _ENCODE_HALF_INPUT at 0 is refused whatever it holds.  bt709hip_encoder_prepare(ctx,
 * BT709HIP_GAMMA_LINEAR, go) builds T as well when the option is 1 at the time of the call: a paired half encode can be captured
 * into a graph after that one prepare (BT709HIP_ERR_NOT_SETUP while capturing otherwise, nothing enqueued).
 * bt709hip_last_kernel_name: "encode_rgba16f_alpha_nv12", "encode_rgba16f_alpha_i420", "encode_rgba16f_alpha_nv12_blocks",
 * "encode_rgba16f_alpha_i420_blocks".  bt709hip_last_launch_info: the plain half encoder's plan for the same size and count;
 * BT709HIP_CTX_OPT_ENCODE_ROW_PAIRS, _ENCODE_THREADS and _XCD_BANDS apply as they do there.  OUT OF SCOPE: an alpha frame alone from
 * a half surface, straight-alpha halves (the surface is premultiplied, as the decoder writes it), +convert: from halves.  The call
 * reads the option once, on entry.  Any value but 0 and 1: BT709HIP_ERR_INVALID_ARG, the option keeps its value (it is not clamped).
 * Setting it never touches the device: it works while a stream is being captured.  At 0 (the default) nothing changes. */

/* A stream with a scheduling priority (hipStreamCreateWithPriority): 0 = normal, negative = higher, positive = lower; clamped
 * to the device's range.  (MTLCommandQueue has no twin; a renderer that decodes ahead of what it presents puts the look-ahead
 * frames on a lower-priority stream.) */
int bt709hip_stream_create_with_priority(bt709hip_context *ctx, int priority, void **stream);

/* Events (timing only; no reference twin). elapsed: milliseconds start->stop. */
int bt709hip_event_create(bt709hip_context *ctx, void **event);
int bt709hip_event_destroy(bt709hip_context *ctx, void *event);
int bt709hip_event_record(bt709hip_context *ctx, void *event, void *stream);
int bt709hip_event_synchronize(bt709hip_context *ctx, void *event);
/* Makes `stream` wait for `event` (recorded on another stream): joins the per-frame streams of a
 * pipeline without blocking the host -- MTLCommandBuffer ordering across queues / encodeWaitForEvent:. */
int bt709hip_stream_wait_event(bt709hip_context *ctx, void *stream, void *event);
int bt709hip_event_elapsed_ms(bt709hip_context *ctx, void *start, void *stop, float *ms);

/* Recorded command buffers.  The reference encodes a frame's passes into an MTLCommandBuffer
 * and commits it (MetalBT709Decoder.h:65-72 takes the buffer; AAPLRenderer.m:891-977 builds one
 * per frame); the HIP twin of a command buffer that is recorded once and replayed is a graph.
 * Between begin and end every bt709hip_decode* / _encode* / upload / download / memset issued
 * on `stream` (a created stream, not NULL) is recorded instead of executed; `graph` then
 * replays them all with one launch -- for pipelines of small frames, where the per-launch host
 * cost exceeds the kernel (a 1080p decode is ~2 us of GPU time).  Decoders must have been set up
 * (bt709hip_decoder_setup) before capture begins; do not wait inside a capture. */
int bt709hip_graph_begin_capture(bt709hip_context *ctx, void *stream);
int bt709hip_graph_end_capture(bt709hip_context *ctx, void *stream, void **graph);
int bt709hip_graph_launch(bt709hip_context *ctx, void *graph, void *stream);
int bt709hip_graph_destroy(bt709hip_context *ctx, void *graph);

/* Free and total device memory of the context's GPU right now (hipMemGetInfo), for callers that size rings or a placement
 * hunt against what is left.  Either pointer may be NULL. */
int bt709hip_mem_info(bt709hip_context *ctx, size_t *free_bytes, size_t *total_bytes);
/* Pinned host memory: uploads from / downloads into it are asynchronous (bt709hip.h, "Device memory"). */
int bt709hip_host_alloc(bt709hip_context *ctx, size_t bytes, void **hptr);
int bt709hip_host_free(bt709hip_context *ctx, void *hptr);

/* Kernel-selection knobs of a decoder (tuning and test hooks; no reference twin).  They may be
 * changed between calls, not during one. */
typedef enum {
  BT709HIP_OPT_NONTEMPORAL = 1,      /* 1 (default): streaming loads / stores in the fast kernels; 0: default cache policy */
  BT709HIP_OPT_HALF_KERNEL = 2,      /* 2:1 rescale: -1 (default) persistent kernel when the launch is large enough, 0 never, 1 always */
  BT709HIP_OPT_HALF_WORKGROUPS = 3,  /* persistent 2:1 kernel: workgroups; 0 (default) = one per compute unit */
  BT709HIP_OPT_HALF_LDS_KB = 4,      /* persistent 2:1 kernel: KiB of LDS a workgroup may fill with table copies; 0 (default) = 160 */
  BT709HIP_OPT_XCD_BANDS = 5,        /* 1 (default): batched 1:1 launches of 64 frames or more give each XCD a contiguous band of the frames (a count that is not a multiple of 8: that map over the multiple of 8, the plain map over the rest); 0: plain (tile, row pair, frame) order */
  BT709HIP_OPT_COALESCE = 6,         /* 0 (default) off; n in 2..32: coalescing submit, see bt709hip_decode */
  BT709HIP_OPT_COALESCE_MAX_AGE_US = 7, /* 0 (default): queued frames wait for their stream's next call, however long; t > 0: a queue whose oldest frame was queued more than t microseconds ago is issued by the next bt709hip_* call that touches ANY stream of the context (or any decode of any decoder of it) */
  BT709HIP_OPT_COMPOSITE_OVER = 9,   /* alpha decoders: BT709HIP_OVER_OFF (default), BT709HIP_OVER_DESTINATION, or an sRGB colour R<<16 | G<<8 | B; see below */
  BT709HIP_OPT_SCALED_OVER = 10,     /* alpha decoders, the rescale paths: the values of BT709HIP_OPT_COMPOSITE_OVER, held separately; see below */
  BT709HIP_OPT_CHROMA_LAYOUT = 11,   /* BT709HIP_CHROMA_NV12 (default) or BT709HIP_CHROMA_I420: how the 1:1 decode reads the caller's colour frames; see below */
  BT709HIP_OPT_UNPREMULTIPLY = 12,   /* alpha decoders: 0 (default) the 1:1 decode writes premultiplied colour, as the frames hold it; 1: straight alpha; see below */
  BT709HIP_OPT_SCALE_INTERMEDIATE = 8  /* the intermediate the FUSED rescales filter, a bt709hip_format: BT709HIP_FORMAT_BGRA8_SRGB (default) or BT709HIP_FORMAT_RGBA16F; any other value: BT709HIP_ERR_INVALID_ARG, option unchanged.  See below */
} bt709hip_decoder_option;
int bt709hip_decoder_set_option(bt709hip_decoder *dec, int option, int value);
int bt709hip_decoder_get_option(const bt709hip_decoder *dec, int option, int *value);
/* BT709HIP_OPT_SCALE_INTERMEDIATE.  The reference renders pass 1 into BGRA8Unorm_sRGB where sRGB texture writes exist and into
 * RGBA16Float holding linear light where they do not (Renderer/AAPLRenderer.m:132-207), then runs -renderScaled: over whichever
 * it made.  With the option at BT709HIP_FORMAT_RGBA16F, bt709hip_decode_scaled[_batch] and bt709hip_decode_half[_batch] produce,
 * bit for bit and in one launch without the surface, what bt709hip_decode into an RGBA16F surface of the frame's size followed
 * by bt709hip_render_scaled from it produces: the filter sees linear light at half precision instead of bytes quantised to
 * 8-bit sRGB (about 3 output pixels in 10 differ by one code).  The output stays BGRA8_SRGB.  Differences from the 8-bit mode:
 *   - a decoder WITHOUT an alpha channel writes A = 0xFF whatever bt709hip_decoder_set_alpha_fill says (the half target holds
 *     1.0 and the two passes do the same);
 *   - bt709hip_decode_half[_batch] runs the any-ratio kernel at ratio 2.0: there is no persistent 2:1 variant, and
 *     BT709HIP_OPT_HALF_KERNEL, _HALF_WORKGROUPS, _HALF_LDS_KB and _NONTEMPORAL are ignored; the limits are
 *     bt709hip_decode_scaled's, and bt709hip_last_scaled_launch_info reports the plan;
 *   - the half lookup table is built on the first such call, as for RGBA16F targets: before a graph capture call
 *     bt709hip_decoder_prepare_format(dec, BT709HIP_FORMAT_RGBA16F) (a call that finds it missing during a capture returns
 *     BT709HIP_ERR_NOT_SETUP).
 * bt709hip_last_kernel_name: "decode_nv12_scaled_f16" / "decode_nv12_scaled_f16<alpha>".  Definition: DESIGN.md 3.3. */
/* BT709HIP_OPT_COMPOSITE_OVER (decoders created with has_alpha != 0).  The reference decodes an alpha clip into a non-opaque
 * MTKView over a pattern image or over plain black / white (Application/AAPLViewController.m:30-66) and leaves the blend to the
 * system compositor; the colour frame holds PREMULTIPLIED colour (srgb_to_bt709.m:805-811; AAPLShaders.metal:432-436).  With the
 * option on, the 1:1 decode -- bt709hip_decode, bt709hip_decode_batch and everything that launches through them: ring, ring
 * set, pool, shard, the coalescing submit -- blends each decoded pixel source-over a background in linear light inside the
 * decode kernel, bit for bit what "decode, then blend the 8-bit result" gives (definition: DESIGN.md 3.5):
 *   BT709HIP_OVER_OFF          nothing changes: the same kernels, names and bytes;
 *   BT709HIP_OVER_DESTINATION  the background is what `out` holds when the kernel runs (Metal: loadAction = Load with blending
 *                              on); each output word is read once and written once, by the same lane;
 *   0 ... 0xFFFFFF             an opaque solid colour, sRGB bytes R<<16 | G<<8 | B (black 0, white 0xFFFFFF); `out` is not
 *                              read and every output alpha is 255.
 * Any other value: BT709HIP_ERR_INVALID_ARG; on a decoder without an alpha channel: BT709HIP_ERR_UNSUPPORTED; either way the
 * option keeps its value.  Setting it never touches the device (frames a coalescing decoder has queued go out first, under the
 * value they were queued with).  Targets are BGRA8_SRGB: with the option on, an RGBA16F target, bt709hip_decode_half[_batch]
 * and bt709hip_decode_scaled[_batch] return BT709HIP_ERR_UNSUPPORTED after their usual validation and write nothing (the
 * rescale paths blend under BT709HIP_OPT_SCALED_OVER, below, and then do not read this option).  The
 * kernels need one more 1 KiB device table: bt709hip_decoder_setup builds it when called with the option on (also on a decoder
 * that is set up already), and so does the first such decode -- but a decode that finds it missing while its stream records a
 * graph returns BT709HIP_ERR_NOT_SETUP.  bt709hip_last_kernel_name: "decode_nv12_quads<alpha,over>" /
 * "decode_nv12_quads<alpha,over-colour>", and "decode_nv12_blocks<alpha,over>" / "decode_nv12_blocks<alpha,over-colour>" on the
 * general path (ragged or misaligned frames). */
/* BT709HIP_OPT_SCALED_OVER (decoders created with has_alpha != 0): the blend of BT709HIP_OPT_COMPOSITE_OVER for the alpha clip
 * that is played view-fit -- pass 1, -renderScaled: to the view's size, then the compositor's blend over the app's background
 * -- in the one fused launch.  Values, refusals and the device table are those of BT709HIP_OPT_COMPOSITE_OVER
 * (BT709HIP_OVER_OFF the default, BT709HIP_OVER_DESTINATION, 0 ... 0xFFFFFF; INVALID_ARG / UNSUPPORTED with the option kept;
 * setting it never touches the device; bt709hip_decoder_setup builds the table when either option is on, the first blended
 * rescale otherwise, BT709HIP_ERR_NOT_SETUP inside a capture).  The two options are independent:
 *   - bt709hip_decode_scaled[_batch] and bt709hip_decode_half[_batch], and everything that launches through them (a ring created
 *     with half_scale), read THIS option: on, each output word is composite_over(s, d) of DESIGN.md 3.5 with s the 8-bit word the
 *     same call writes with the option off -- in whichever intermediate BT709HIP_OPT_SCALE_INTERMEDIATE selects -- bit for bit
 *     "decode_scaled, then blend" (definition: DESIGN.md 3.6), whatever BT709HIP_OPT_COMPOSITE_OVER holds; off, nothing changes,
 *     the refusal under BT709HIP_OPT_COMPOSITE_OVER included;
 *   - the 1:1 decode never reads it; bt709hip_render_scaled has no decoder and does not blend.
 * On, bt709hip_decode_half[_batch] runs the any-ratio kernel at ratio 2.0 (as under BT709HIP_FORMAT_RGBA16F above: no persistent
 * 2:1 variant, the half-kernel options ignored) and equals bt709hip_decode_scaled at exactly half.  Validation, limits and
 * bt709hip_last_scaled_launch_info are the plain rescale's.  bt709hip_last_kernel_name: "decode_nv12_scaled<alpha,over>" /
 * "decode_nv12_scaled<alpha,over-colour>", "decode_nv12_scaled_f16<alpha,over>" / "decode_nv12_scaled_f16<alpha,over-colour>". */
/* BT709HIP_OPT_UNPREMULTIPLY (decoders created with has_alpha != 0).  The colour frame of an alpha clip holds premultiplied
 * colour, and that is what the decode writes; the reference divides it out again on the CPU where it needs straight alpha
 * (+[BGRAToBT709Converter unpremultiply:], Renderer/BGRAToBT709Converter.h:129-133 -- a vImage call, a closed box: the rounding
 * is ours).  With the option at 1, the 1:1 decode into BGRA8_SRGB -- bt709hip_decode, bt709hip_decode_batch and everything that
 * launches through them: ring, ring set, pool, shard, the coalescing submit; both chroma layouts, fast and general kernels --
 * writes, for each pixel, the word it writes at 0 with B, G, R replaced by
 *   c = A == 0 ? 0 : min(255, (255 * c' + A / 2) / A)        c', A in 0..255, integer division
 * A being that word's own alpha byte, which stays (definition: DESIGN.md 3.9).  A = 255: c = c'; A = 0: the word 0; c' > A -- no
 * premultiplied value, but a Y, Cb, Cr triple can decode to it -- gives 255.  No round trip with
 * BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY is promised for small A.  The division happens in the decode kernel's registers: no pass
 * over the surface, no table.  Any value but 0 and 1: BT709HIP_ERR_INVALID_ARG; on a decoder without an alpha channel:
 * BT709HIP_ERR_UNSUPPORTED; either way the option keeps its value.  Setting it never touches the device (it works inside a graph
 * capture); frames a coalescing decoder has queued go out first, under the value they were queued with, and frames of two
 * values never share a launch.  Refused with BT709HIP_ERR_UNSUPPORTED after the usual validation, writing nothing, while the
 * option is 1: RGBA16F targets; bt709hip_decode_half[_batch] and bt709hip_decode_scaled[_batch] (a filter wants premultiplied
 * colour); any 1:1 decode while BT709HIP_OPT_COMPOSITE_OVER is not BT709HIP_OVER_OFF (a blend needs the premultiplied source).
 * bt709hip_last_kernel_name: "decode_nv12_quads<alpha,straight>", "decode_nv12_blocks<alpha,straight>",
 * "decode_i420_quads<alpha,straight>", "decode_i420_blocks<alpha,straight>".  At 0 nothing changes. */
#define BT709HIP_OVER_OFF (-1)
#define BT709HIP_OVER_DESTINATION (-2)
/* BT709HIP_OPT_CHROMA_LAYOUT.  The reference's on-disk format is PLANAR 4:2:0 -- a YUV4MPEG2 C420jpeg FRAME is Y, then U, then V
 * (Renderer/y4m_writer.h:194-241) -- and so is every software decoder's yuv420p.  With the option at BT709HIP_CHROMA_I420 the
 * colour bt709hip_frame of bt709hip_decode and bt709hip_decode_batch (pointer table or evenly spaced frames, the coalescing
 * submit included) is read as three planes, with no interleave pass and no staging buffer:
 *   y, y_stride   as before;
 *   cbcr          the U (Cb) plane: (W/2) x (H/2) bytes, rows cbcr_stride bytes apart, cbcr_stride >= W/2;
 *   the V (Cr) plane has the same pitch and starts at cbcr + (height/2) * cbcr_stride.
 * A tight Y4M FRAME payload uploaded as one blob is y = base, y_stride = W, cbcr = base + W*H, cbcr_stride = W/2.  Pixel (x, y)
 * takes Y[y][x], U[y/2][x/2], V[y/2][x/2]; the output is byte for byte what the NV12 decode of the interleaved twin of the planes
 * writes -- BGRA8_SRGB targets, every gamma, decoders with and without an alpha channel (alpha frames are Y-only and do not
 * change), BT709HIP_OPT_COMPOSITE_OVER in both modes.  Validation: cbcr_stride < W/2 is BT709HIP_ERR_STRIDE (NV12: < W); the
 * other checks and limits are NV12's, applied to the U plane's extent and the V plane's; an evenly spaced batch is one whose U
 * planes are (V follows from cbcr).  Fast kernels need W % 4 == 0, luma / alpha planes 4-byte aligned, the U pointer and
 * cbcr_stride 2-byte aligned and the output 16-byte aligned; any other frame takes the general kernel.
 * bt709hip_last_kernel_name: the NV12 names with "decode_i420_" for "decode_nv12_" ("decode_i420_quads<nt>",
 * "decode_i420_quads<alpha>", "decode_i420_blocks", ...).  Any value but the two: BT709HIP_ERR_INVALID_ARG, the option keeps
 * its value.  Setting it never touches the device and needs no device table (it works inside a graph capture); frames a
 * coalescing decoder has queued go out first, under the layout they were queued with, and frames of two layouts never share a
 * launch.  NOT covered:
 *   - RGBA16F targets, bt709hip_decode_half[_batch] and bt709hip_decode_scaled[_batch] return BT709HIP_ERR_UNSUPPORTED after
 *     their usual validation and write nothing while the option is BT709HIP_CHROMA_I420 (their strip loaders read NV12);
 *     with BT709HIP_OPT_SCALED_PLANAR at 1 the four rescale calls DO read planar frames (PLANAR FRAMES INTO THE RESCALES, below),
 *     RGBA16F targets stay refused;
 *   - objects that allocate their own frames -- ring, ring set, pool, shard -- stay NV12 whatever the option holds (their
 *     launches pass the layout instead of reading the option; bt709hip_ring_frame keeps describing NV12 planes);
 *   - bt709hip_unconvert and bt709hip_render_scaled have no chroma plane to lay out and are unchanged; the encoder WRITES one,
 *     and its layout is the context's own option, BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT (above), not this one;
 *   - YV12 (V before U), and planar frames whose V plane is anywhere but (height/2) * cbcr_stride behind U. */
#define BT709HIP_CHROMA_NV12 0
#define BT709HIP_CHROMA_I420 1
/* PLANAR CHW TARGETS.  Three further values of bt709hip_surface.format, accepted as OUTPUT by bt709hip_decode and
 * bt709hip_decode_batch, by bt709hip_decode_scaled[_batch] and bt709hip_decode_half[_batch] once BT709HIP_OPT_SCALED_CHW is 1 (PLANAR
 * CHW VIEWS, below), and as INPUT by bt709hip_encode and bt709hip_encode_batch once BT709HIP_CTX_OPT_ENCODE_CHW_INPUT is 1 (PLANAR
 * CHW INPUT, below) -- every other entry point (the rescales with that option at 0, bt709hip_render_scaled, the encoder with that option at 0,
 * bt709hip_unconvert, ring options, pools, shards, bt709hip_decoder_prepare_format) returns what it returns for any unknown format.  The decode writes the frame as
 * the planar C x H x W tensor an inference pipeline takes, with no second pass and no scratch surface (definition: DESIGN.md 3.14).
 * With e = 1, 2 or 4 bytes per element:
 *   bgra     the base of plane 0, e-aligned;
 *   stride   the row pitch of EVERY plane in bytes: >= width * e, a multiple of e, <= 2^32 - 1 (else BT709HIP_ERR_STRIDE);
 *   plane c  starts at bgra + c * height * stride (a 64-bit product).  Planes R, G, B; a decoder created with has_alpha != 0
 *            writes a fourth, A; an opaque decoder writes three and ignores bt709hip_decoder_set_alpha_fill.
 * stride == width * e is a contiguous CHW tensor; an NCHW tensor is a batch of evenly spaced surfaces.  Nothing outside the
 * width * e bytes of each plane row is written.  Per pixel, with s the word the same call writes into a BGRA8_SRGB target (same
 * decoder, same frames, premultiplied as the frames hold it):
 *   CHW_U8            plane c holds the byte s_c, the A plane s_A;
 *   CHW_F16, CHW_F32  v = float(s_c) * (1.0f / 255.0f);  t = v * scale_c;  t = t + bias_c  -- binary32, every operation rounded
 *                     on its own, no fused multiply-add; the element is t, or binary16(t) rounded to nearest even (overflow:
 *                     +-inf).  The A plane: float(s_A) * (1.0f / 255.0f), no scale, no bias.
 * scale_c, bias_c: BT709HIP_OPT_CHW_SCALE_R / _G / _B and BT709HIP_OPT_CHW_BIAS_R / _G / _B, whose int value is the BIT PATTERN of a
 * binary32: defaults 1.0f and 0.0f; accepted: +-0 or a finite value with 2^-64 <= |x| <= 2^64 (no binary32 subnormal and no
 * binary32 overflow can then arise); anything else BT709HIP_ERR_INVALID_ARG, the option keeps its value.  bt709hip_decoder_get_option
 * returns the bits.  Decoders with and without an alpha channel take them; CHW_U8 ignores them.  A call reads each ONCE and they
 * travel as kernel arguments (nothing is staged on the device: setting them and decoding both work inside a graph capture);
 * setting one while a call that uses them is in flight on another thread is the caller's race -- that call may run with the old
 * value of one and the new value of another.
 * BT709HIP_OPT_CHROMA_LAYOUT = I420 is supported.  BT709HIP_OPT_COMPOSITE_OVER != OFF or BT709HIP_OPT_UNPREMULTIPLY = 1 with a CHW
 * target: BT709HIP_ERR_UNSUPPORTED after the usual validation, nothing launched (the order of checks is RGBA16F's).  A batch whose
 * surfaces differ in format: BT709HIP_ERR_INVALID_ARG.  The limits are every decode's (height / 2 <= 65535; 32 surfaces through
 * the pointer table, any number evenly spaced).  On a coalescing decoder a call with a CHW target is never queued: the stream's
 * queued frames are issued first, then the call launches on its own.  Fast kernels need the fast path's input alignment,
 * width % 4 == 0 and plane 0 and the pitch 4 e-aligned; any other surface takes the general kernel.  bt709hip_last_kernel_name:
 * "decode_nv12_quads_chw<u8,nt>", "decode_i420_quads_chw<f32,alpha>", "decode_nv12_blocks_chw<f16,quantiser>", ...;
 * bt709hip_last_launch_info is filled as for the BGRA8 launch. */
#define BT709HIP_FORMAT_CHW_U8 4  /* planes of bytes */
#define BT709HIP_FORMAT_CHW_F16 5 /* planes of IEEE binary16 */
#define BT709HIP_FORMAT_CHW_F32 6 /* planes of IEEE binary32 */
#define BT709HIP_OPT_CHW_SCALE_R 14
#define BT709HIP_OPT_CHW_SCALE_G 15
#define BT709HIP_OPT_CHW_SCALE_B 16
#define BT709HIP_OPT_CHW_BIAS_R 17
#define BT709HIP_OPT_CHW_BIAS_G 18
#define BT709HIP_OPT_CHW_BIAS_B 19
/* PLANAR CHW VIEWS (BT709HIP_OPT_SCALED_CHW; definition: DESIGN.md 3.16).  A model rarely takes a frame at its own size: with this
 * decoder option at 1, bt709hip_decode_scaled, bt709hip_decode_scaled_batch, bt709hip_decode_half and bt709hip_decode_half_batch
 * accept BT709HIP_FORMAT_CHW_U8 / _F16 / _F32 surfaces of the view's size OW x OH (the half calls: W/2 x H/2) as OUTPUT and write the
 * rescaled, normalised planar tensor in the one fused launch -- no BGRA8 scratch surface and no second pass.  Values 0 (default) and 1;
 * anything else BT709HIP_ERR_INVALID_ARG, the option keeps its value; bt709hip_decoder_get_option returns it.  Setting it never
 * touches the device and works during a graph capture; decoders with and without an alpha channel take it.  At 0 nothing changes:
 * the same kernels, names, bytes and return codes (a CHW surface is then an unknown format to the rescales).
 * The surface is laid out as under PLANAR CHW TARGETS with the view's size for the frame's: bgra the e-aligned base of plane 0,
 * stride the pitch of every plane (a multiple of e, OW * e <= stride <= 2^32 - 1, else BT709HIP_ERR_STRIDE), plane c starting
 * c * OH * stride bytes (a 64-bit product) behind plane 0; planes R, G, B, and A from an alpha decoder; an opaque decoder ignores
 * bt709hip_decoder_set_alpha_fill.  Nothing outside the OW * e bytes of each plane row is written.
 * Per output pixel, with s the word the same call, on the same decoder and frames, writes into a BGRA8_SRGB target of the same size
 * with BT709HIP_OPT_SCALE_INTERMEDIATE at its default (DESIGN.md 3.3's filter in linear light on sRGB bytes): the element of plane c
 * is PLANAR CHW TARGETS' function of the byte s_c -- CHW_U8 the byte; CHW_F16 / _F32 float(s_c) * (1/255f), * scale_c, + bias_c in
 * three separately rounded binary32 operations (BT709HIP_OPT_CHW_SCALE_* / _BIAS_*, each read once per call, travelling as kernel
 * arguments), then binary16 for CHW_F16; the A plane float(s_A) * (1/255f) of the FILTERED alpha, colour staying premultiplied.
 * bt709hip_decode_half[_batch] with a CHW target runs the any-ratio kernel at ratio 2.0 (as under BT709HIP_OPT_SCALED_OVER: no
 * persistent 2:1 variant, the half-kernel options ignored; W, H % 4 == 0 stays) and equals bt709hip_decode_scaled at exactly half.
 * Validation order, codes and limits are the rescale's own (OH <= 65535; 32 surfaces through the pointer table, 65535 evenly
 * spaced); a batch whose surfaces differ in format where one is CHW: BT709HIP_ERR_INVALID_ARG.  Refused with
 * BT709HIP_ERR_UNSUPPORTED behind the usual validation and the I420 / COMPOSITE_OVER / UNPREMULTIPLY refusals, nothing written or
 * launched: a CHW target while BT709HIP_OPT_SCALE_INTERMEDIATE is BT709HIP_FORMAT_RGBA16F; a CHW target while
 * BT709HIP_OPT_SCALED_OVER is not BT709HIP_OVER_OFF; a CHW surface whose planes together (planes * OH * stride) reach 2 GiB (the
 * kernels form offsets into the surface in 32 bits).  bt709hip_last_kernel_name: "decode_nv12_scaled_chw<u8>",
 * "decode_nv12_scaled_chw<f16,alpha>", "decode_nv12_scaled_chw<f32>", ...; bt709hip_last_scaled_launch_info is filled as for the
 * BGRA8 launch, with the tap form the BGRA8 call of the same frames and view takes (the count of resident workgroups is the launched
 * kernel's own).  NOT covered: CHW through the RGBA16Float intermediate; blended or straight-alpha CHW views; I420 input to the
 * rescales (unless BT709HIP_OPT_SCALED_PLANAR is 1: PLANAR FRAMES INTO THE RESCALES, below); bt709hip_render_scaled into CHW; rings (half_scale), pools and shards with CHW targets; bt709hip_decoder_prepare_format
 * of a CHW format; an antialiased (area) filter -- the filter is bt709hip_decode_scaled's two-tap bilinear. */
#define BT709HIP_OPT_SCALED_CHW 22 /* 0 (default) / 1; ids 13, 20, 21 and 23 are no option */
/* PLANAR FRAMES INTO THE RESCALES (BT709HIP_OPT_SCALED_PLANAR; definition: DESIGN.md 3.17).  A Y4M or yuv420p clip is planar, and
 * a caller who wants its frames at another size would have to interleave each into an NV12 staging plane first
 * (bt709hip_interleave_cbcr).  With this decoder option at 1 AND BT709HIP_OPT_CHROMA_LAYOUT = BT709HIP_CHROMA_I420,
 * bt709hip_decode_scaled, bt709hip_decode_scaled_batch, bt709hip_decode_half and bt709hip_decode_half_batch read the colour frame
 * as BT709HIP_OPT_CHROMA_LAYOUT (above) defines it -- cbcr the U plane at pitch cbcr_stride >= W/2, V of the same pitch
 * (height/2) * cbcr_stride behind it, pixel (x, y) taking U[y/2][x/2] and V[y/2][x/2] -- in the one fused launch.  Values 0
 * (default) and 1; anything else BT709HIP_ERR_INVALID_ARG, the option keeps its value; bt709hip_decoder_get_option returns it.
 * Setting it never touches the device and works during a graph capture; decoders with and without an alpha channel take it.  At 0
 * nothing changes, and at 1 nothing changes for NV12 frames: the same kernels, names, launch plans, bytes and return codes.
 * The output is byte for byte what the same call, on the same decoder, writes for the NV12 interleaved twin of the planes:
 * BGRA8_SRGB views, CHW_U8 / _F16 / _F32 views (BT709HIP_OPT_SCALED_CHW at 1), every gamma, decoders with and without an alpha
 * channel (alpha frames are Y-only and do not change).  bt709hip_decode_half[_batch] of planar frames runs the any-ratio kernel at
 * ratio 2.0 (as for CHW and blended views: no persistent 2:1 planar kernel, the half-kernel options ignored; W, H % 4 == 0 stays)
 * and equals bt709hip_decode_scaled at exactly half, hence the NV12 bt709hip_decode_half of the twin.
 * Validation is the I420 decode's: cbcr_stride < W/2 is BT709HIP_ERR_STRIDE, extents are the U plane's and the V plane's, an evenly
 * spaced batch is one whose U planes are.  The rescale's own limits hold with each of the Y, U, V and alpha planes taken on its own:
 * OH <= 65535, every plane under 2 GiB (U and V TOGETHER may pass it), 32 surfaces through the pointer table, 65535 evenly spaced.
 * Tap forms (bt709hip_last_scaled_launch_info reports the one launched): BT709HIP_SCALED_TAPS_ONCE under the ratio conditions of
 * the NV12 call, whatever the alignment (three byte loads per lane); _WIDE when W % 8 == 0, W >= 16 and the luma, alpha and U
 * pointers, every pitch and an evenly spaced batch's steps are 4-byte aligned; _BYTES for every other frame (where NV12 would take
 * _PAIRS, too).  BT709HIP_SCALED_TAPS_SHARED is not built for planar frames: where an NV12 call takes it (scale_y < 1 with
 * scale_x > 0.95) the planar call takes the per-lane form.  bt709hip_last_kernel_name: "decode_i420_scaled",
 * "decode_i420_scaled<alpha>", "decode_i420_scaled_chw<u8>", "decode_i420_scaled_chw<f16,alpha>", ...
 * Still refused with BT709HIP_ERR_UNSUPPORTED while the frames are I420, behind the usual validation and where the I420 refusal has
 * always stood (in front of the COMPOSITE_OVER, UNPREMULTIPLY and CHW refusals), nothing launched, built or copied:
 * BT709HIP_OPT_SCALE_INTERMEDIATE = BT709HIP_FORMAT_RGBA16F; BT709HIP_OPT_SCALED_OVER other than BT709HIP_OVER_OFF; an RGBA16F
 * target of the 1:1 decode.  NOT covered: rings (half_scale), ring sets, pools and shards with planar frames (they stay NV12);
 * a planar TAPS_SHARED; a persistent 2:1 planar kernel; YV12.  bt709hip_render_scaled and bt709hip_unconvert are unchanged. */
#define BT709HIP_OPT_SCALED_PLANAR 24 /* 0 (default) / 1; id 23 is no option */
/* PLANAR CHW INPUT (BT709HIP_CTX_OPT_ENCODE_CHW_INPUT; definition: DESIGN.md 3.15).  The way back of the targets above: a model's output
 * -- super-resolution, denoising, interpolation -- is a CHW or NCHW tensor, and with the option at 1 bt709hip_encode and
 * bt709hip_encode_batch take it as it lies, in ONE launch that reads 3 e and writes 1.5 bytes per pixel (e = 1, 2 or 4): no
 * de-normalising, rounding, permuting or interleaving pass by the caller.  The call takes its format from ins[0]; a batch of mixed
 * formats is BT709HIP_ERR_SIZE_MISMATCH, as ever.  The layout is the targets': bgra is the base of plane 0 and is e-aligned; stride is
 * the pitch of EVERY plane in bytes, a multiple of e with width * e <= stride <= 2^32 - 1 (else BT709HIP_ERR_STRIDE); plane c starts at
 * bgra + c * height * stride (a 64-bit product).  Planes R, G, B are read; a fourth plane may lie behind them and is NEVER read (the
 * BGRA8_SRGB encode ignores A, too).  Per element, t being its value (a binary16 converts to binary32 exactly):
 *   CHW_U8            s_c = t, the byte itself;
 *   CHW_F16, CHW_F32  u = t * scale_c;  u = u + bias_c  -- binary32, every operation rounded on its own, no fused multiply-add;
 *                     x = sat(u): NaN -> 0, u < 0 (and -0) -> 0, u > 1 (and +inf) -> 1;
 *                     s_c = (int)round(x * 255.0f), halves away from zero (exact for every float in [0, 1]).
 * The frame written is, byte for byte, the frame the same call writes for the BGRA8_SRGB surface whose texels are
 * (B, G, R, A) = (s_B, s_G, s_R, 255): same input gamma (all three work: the path starts from a byte), same output gamma, same
 * BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT (NV12 and I420).  scale_c, bias_c: BT709HIP_CTX_OPT_ENCODE_CHW_SCALE_R / _G / _B = 20, 21, 22
 * and BT709HIP_CTX_OPT_ENCODE_CHW_BIAS_R / _G / _B = 23, 24, 25, whose int value is the BIT PATTERN of a binary32: defaults 1.0f and
 * 0.0f; accepted: +-0 or a finite value with 2^-64 <= |x| <= 2^64; anything else BT709HIP_ERR_INVALID_ARG, the option keeps its value.
 * They are the INVERSE of the decode's pair: where a decoder holds (1 / std, -mean / std), the encoder holds (std, mean).  A call
 * reads each ONCE and they travel as kernel arguments (nothing is staged on the device: setting them and encoding both work inside a
 * graph capture once the encoder's tables exist); CHW_U8 ignores them; there is no getter.  Setting one while a call that uses them
 * is in flight on another thread is the caller's race.
 * Validation keeps the encoder's order and codes -- sizes, odd dimensions, height / 2 <= 65535, strides, NULLs -- with the element
 * size in place of the texel size, and enqueues nothing on refusal.  BT709HIP_CTX_OPT_ENCODE_ROW_PAIRS, _ENCODE_THREADS and _XCD_BANDS
 * apply as they do to BGRA8_SRGB input, and bt709hip_last_launch_info is the BGRA8 encoder's plan for the same size and count.
 * BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY, _ENCODE_CONVERT, _ENCODE_WITH_ALPHA or _ENCODE_HALF_WITH_ALPHA away from its default with CHW
 * input: BT709HIP_ERR_UNSUPPORTED behind the usual validation, nothing launched.  BT709HIP_CTX_OPT_ENCODE_HALF_INPUT is independent.
 * Batches: any count of evenly spaced surfaces up to 65535 (a contiguous NCHW tensor is one); otherwise a pointer table of
 * BT709HIP_MAX_BATCH - 1 = 31 surfaces (the kernel argument block does not grow: the six values ride in the table's last entry):
 * more is BT709HIP_ERR_UNSUPPORTED.  The fast kernel needs width % 4 == 0, plane 0 and the pitch 4 e-aligned and the frame aligned as
 * the BGRA8 fast kernel needs it; every other valid call takes the general kernel (element loads, byte stores) and writes the same
 * bytes.  bt709hip_last_kernel_name: "encode_chw_nv12<u8>", "encode_chw_i420<f32>", "encode_chw_nv12_blocks<f16>", ... .  Tables: the
 * (input_gamma, output_gamma) encoder's own, built by the first call or by bt709hip_encoder_prepare.  BGRA8 and RGBA16F input behave
 * exactly as before with the option at either value.  Any value but 0 and 1: BT709HIP_ERR_INVALID_ARG, the option keeps its value (it
 * is not clamped); setting it never touches the device.  OUT OF SCOPE: float tensors as linear light without the 8-bit step (the
 * RGBA16F route exists for that); an alpha frame from a fourth plane; straight-alpha tensors; HWC tensors. */

/* COALESCING SUBMIT (extension, opt-in: bt709hip_decoder_set_option(dec, BT709HIP_OPT_COALESCE, n), n = 2..32).
 * The reference's cadence is one -decodeBT709: call per frame (MetalBT709Decoder.h:65-72, AAPLRenderer.m:914-957), each call
 * encoding into the caller's command buffer; on an MI355X a 4K frame is a ~7.6 us kernel and a launch boundary on one stream
 * costs ~3.8 us of idle GPU, so that cadence reaches 0.49 of the roofline where one launch over many frames reaches 0.75-0.81.
 * With the option on, a 1:1 decode of device-resident frames with wait_until_completed == 0 -- bt709hip_decode, or
 * bt709hip_decode_batch with a count below n -- is VALIDATED at once (its status is the call's status, as before) but only
 * QUEUED: up to n frames of one geometry and target format per stream gather and go out as ONE bt709hip_decode_batch launch
 * (evenly spaced frames as a uniform batch, any others through the pointer table).  The queue of a stream is issued
 *   - when it holds n frames, or a call with another geometry / format / decoder state arrives for that stream,
 *   - when a call arrives that reads or writes what a queued call writes, or writes what a queued call reads (the items of a
 *     launch run concurrently; calls made one after the other do not): the queue goes out first and the call starts a new one,
 *     so two decodes into one surface, clips layered onto one canvas under BT709HIP_OVER_DESTINATION and a target read back
 *     as a frame keep the order of the calls.  Targets of one pitch whose rows share a pitch grid -- windows of one canvas --
 *     are compared as rectangles, exactly, and gather when disjoint; everything else (targets against inputs: Y, CbCr or
 *     U + V, alpha) by byte range [base, base + (rows - 1) * pitch + row bytes), which may issue a queue early and never
 *     late.  Overlap INSIDE one batch call stays the caller's error (THE UNIFORM RULE, below),
 *   - by any bt709hip_* call that takes that stream (stream_synchronize, event_record, stream_wait_event, download, upload,
 *     memset, graph capture, copy_probe, a decode with wait_until_completed != 0, every other decode / encode / rescale
 *     entry point -- of THIS decoder or of any other decoder of the context, coalescing or not) -- so the stream keeps its
 *     order for everything issued through this API (a CPU test parses this header's `void *stream` exports and checks
 *     each one of them),
 *   - by bt709hip_decoder_flush, and when the decoder is destroyed or the option is turned off.
 * There is no timer thread: a queue is only ever issued from inside a bt709hip_* call.  A caller that may go idle with frames
 * queued either flushes before it does, or sets BT709HIP_OPT_COALESCE_MAX_AGE_US, which bounds the wait by the time to the
 * context's NEXT call of any kind (a renderer's per-frame bt709hip_stream_synchronize / event poll on another stream is enough).
 * The command-buffer analogy: queued frames are "encoded, not yet committed".  What the caller gives up: work submitted to
 * the raw hipStream_t behind this API's back (its own kernels, hipStreamSynchronize) is not ordered after queued frames --
 * call bt709hip_decoder_flush first.  Frame and surface descriptors are copied at the call; the buffers they point to must
 * stay alive until the stream has passed the launch, as always.  A launch failure at issue time is returned by the call that
 * issued the queue.  Thread safety: as without the option (several threads may share a decoder; each queue is per stream); while any decoder of a
 * context coalesces, that context's stream-taking calls serialise on one mutex for the length of the launch calls they issue, and a
 * call made while its stream records a graph issues that stream's queue only (aged queues of other streams wait for the next call). */
int bt709hip_decoder_flush(bt709hip_decoder *dec, void *stream /* NULL = the context's default stream */);
/* every stream's queue of this decoder */
int bt709hip_decoder_flush_all(bt709hip_decoder *dec);

/* ------------------------------------------------------------- batched forms */
/* `count` frames / pictures / surfaces of one geometry in ONE launch (grid.z = item), like bt709hip_decode_batch and with
 * its limits: up to BT709HIP_MAX_BATCH arbitrary buffers, or any number up to 65535 when item i sits at item 0 + i * (item 1
 * - item 0) in every plane.  No reference twin (the reference converts, rescales and encodes one frame per call: a 4K frame
 * is a 12-22 us kernel, too short to fill the chip; one 4K +unconvert: per call runs at 0.58 of the roofline).  Differing sizes,
 * strides or formats: BT709HIP_ERR_SIZE_MISMATCH.  More than 65535 evenly spaced items: BT709HIP_ERR_UNSUPPORTED, but from
 * bt709hip_render_scaled_batch, which checks count with its other arguments, BT709HIP_ERR_INVALID_ARG.  The single calls' row
 * limits (bt709hip.h) hold for every item.  bt709hip_render_scaled_batch takes evenly spaced surfaces only
 * (BT709HIP_ERR_UNSUPPORTED otherwise), each base a multiple of its texel size (BT709HIP_ERR_STRIDE, as the single call).
 * THE UNIFORM RULE, for every batched entry point (bt709hip_decode_batch and the coalescing queue included): a batch is evenly
 * spaced when, plane by plane (Y, CbCr, alpha, target; the encoder's BGRA, Y, CbCr), item i's pointer is item 0's + i * step, the
 * step being item 1's pointer - item 0's as a signed 64-bit byte count.  ANY TWO items are evenly spaced: a batch of two always
 * launches this way, whatever its pointers.  A step may be negative (items in descending order), 4 GiB or more, another for
 * every plane and of another sign, and 0 on the input side (one frame, one alpha plane, decoded into several targets).  It is
 * folded into the alignment the fast kernels need: a step off that alignment selects the general kernel, same bytes out.
 * Output items that overlap one another (an output step smaller than a target's extent, 0 included) are the caller's error:
 * the result is undefined and nothing checks for it.  bt709hip_encode_batch with BT709HIP_FORMAT_BGRA8_ALPHA input (alpha frames, bt709hip.h):
 * every out[i].cbcr NULL or none (else BT709HIP_ERR_INVALID_ARG); bt709hip_encoder_prepare(ctx, LINEAR, LINEAR) also builds its table.
 * Pitches follow bt709hip.h's rule in every batched form: each at most 2^32 - 1, the alpha frames' included (BT709HIP_ERR_STRIDE);
 * bt709hip_decode_scaled_batch and bt709hip_render_scaled_batch additionally need rows x pitch < 2^31 for every plane and the
 * output (BT709HIP_ERR_UNSUPPORTED). */
int bt709hip_unconvert_batch(bt709hip_decoder *dec, int count, const void *const *ycbcr_words, size_t in_stride, int width, int height,
                             const bt709hip_surface *outs, void *stream, int wait_until_completed);
int bt709hip_decode_half_batch(bt709hip_decoder *dec, int count, const bt709hip_frame *frames, const bt709hip_frame *alphas,
                               const bt709hip_surface *outs, void *stream, int wait_until_completed);
int bt709hip_decode_scaled_batch(bt709hip_decoder *dec, int count, const bt709hip_frame *frames, const bt709hip_frame *alphas,
                                 const bt709hip_surface *outs, void *stream, int wait_until_completed);
int bt709hip_render_scaled_batch(bt709hip_context *ctx, int count, const bt709hip_surface *ins, const bt709hip_surface *outs,
                                 void *stream, int wait_until_completed);
int bt709hip_encode_batch(bt709hip_context *ctx, int count, const bt709hip_surface *ins, const bt709hip_frame *outs, int input_gamma,
                          int output_gamma, void *stream, int wait_until_completed);
/* Lookup tables that are built on first use (device allocation + blocking copies) cannot be built while a stream records a
 * graph: call these before bt709hip_graph_begin_capture (a call that finds its tables missing during a capture returns
 * BT709HIP_ERR_NOT_SETUP).  Idempotent.  render_scaled_prepare: pass 2 alone; decoder_prepare_format: RGBA16F targets;
 * encoder_prepare: one (input_gamma, output_gamma) pair of the encoder. */
int bt709hip_render_scaled_prepare(bt709hip_context *ctx);
int bt709hip_decoder_prepare_format(bt709hip_decoder *dec, int format);
int bt709hip_encoder_prepare(bt709hip_context *ctx, int input_gamma, int output_gamma);

/* --------------------------------------------------------------- frame pool */
/* Frames that live in HOST memory.  The reference hands the decoder CVPixelBuffers the GPU reads
 * in place (unified memory) and keeps MaxBuffersInFlight = 3 frames in flight behind a semaphore
 * (AAPLRenderer.m:34, 891-977); a discrete GPU needs the copies, so the pool owns, per in-flight
 * slot, one HIP stream, pinned host staging and device buffers:
 *   acquire  -> pointers to the slot's pinned Y / CbCr planes (waits for the slot's previous frame)
 *   submit   -> upload, decode, download enqueued on the slot's stream; returns at once
 *   wait     -> the slot's pinned BGRA rows, valid until the slot is acquired again
 * Slots are handed out round-robin, so `depth` frames overlap their copies and kernels.  The decoder
 * must outlive the pool; a pool is used from one thread at a time (decoders and contexts may be
 * shared between threads, each thread with pools / streams of its own).  For a decoder with an
 * alpha channel every slot also owns an alpha plane: fetch its pinned pointer with
 * bt709hip_pool_alpha_plane after acquire and fill it before submit. */
int bt709hip_pool_create(bt709hip_decoder *dec, int width, int height, int depth, bt709hip_pool **out);
int bt709hip_pool_destroy(bt709hip_pool *pool);
int bt709hip_pool_acquire(bt709hip_pool *pool, int *slot, void **y, size_t *y_stride, void **cbcr,
                          size_t *cbcr_stride);
int bt709hip_pool_alpha_plane(bt709hip_pool *pool, int slot, void **alpha, size_t *alpha_stride);
int bt709hip_pool_submit(bt709hip_pool *pool, int slot);
int bt709hip_pool_wait(bt709hip_pool *pool, int slot, const void **bgra, size_t *stride);
/* Hands an acquired slot back without submitting it (nothing is enqueued).  A FAILED bt709hip_pool_submit
 * hands its slot back by itself: a slot never stays "acquired" behind an error. */
int bt709hip_pool_release(bt709hip_pool *pool, int slot);

/* --------------------------------------------------------------- frame ring */
/* Frames that live in DEVICE memory: a ring of `frames` same-sized NV12 inputs carved from one slab and their outputs (BGRA8, or
 * RGBA16F through bt709hip_ring_options.format) from another (frame i at slab + i * spacing: any count goes out as one launch,
 * bt709hip_decode_batch's "evenly spaced" form) -- what a streaming application keeps resident, and what bench.py times.  The
 * reference's twin is the set of CVPixelBuffers + the render texture it keeps per in-flight frame (AAPLRenderer.m:34, 530-862);
 * unified memory has no placement to choose, a discrete HBM device does: where the two slabs land decides how fast the launch
 * streams (the same 256-frame 4K launch runs at 0.74-0.82 of the HBM roofline on allocations made one after the other by one
 * process, each keeping its rate).  bt709hip_ring_create therefore allocates candidates -- `tries` sets how many
 * (0 = the default, 6; 1 = first allocation, no probing; rings under 256 MB never probe) -- times the DECODER'S OWN LAUNCH over
 * the ring on them (~15 ms each: every output candidate under the first input, 2-3 x `tries` of them; then the pairings with the
 * other inputs; then the best pairings and the first-allocated one again, six times as long), keeps the fastest pairing and frees
 * the rest.  TRANSIENT FOOTPRINT: the hunt runs under a BUDGET (bt709hip_ring_options).  By default (round 6) it is FRUGAL: it
 * never holds more than TWICE the ring -- the incumbent pair + one candidate pair; a new candidate evicts the slower of the two
 * outputs alive -- because freeing and allocating again hands out other physical pages, so holding every candidate buys nothing
 * (the 11.7 GB 4K ring: 0.80-0.82 of the roofline within 23 GB in ~1 s, against 0.81 within 58-148 GB in 2-5 s;
 * profiles/r05_hunt_budget.txt, profiles/r06_hunt_default.txt), and always leaves 4 GiB of the device free.  max_bytes names a
 * wider budget.  Duration and peak footprint are reported (hunt_ms, peak_bytes).  half_scale != 0: outputs are (W/2) x (H/2) and
 * the ring decodes through bt709hip_decode_half_batch.  A decoder with an alpha channel gets an alpha plane per frame (third
 * plane of the input slab).  The memory is NOT cleared.  The decoder must outlive the ring. */
typedef struct bt709hip_ring bt709hip_ring;
typedef struct {
  int32_t tries;                     /* candidates per slab asked for (after clamping) */
  int32_t in_candidates;             /* input slabs allocated */
  int32_t out_candidates;            /* output slabs allocated (up to 3 x tries) */
  int32_t chosen_in, chosen_out;     /* allocation-order index of the slabs kept */
  int32_t probes;                    /* pairings probed */
  float first_GBps;                  /* probe of the first-allocated pairing (input 0, output 0): what tries = 1 keeps */
  float chosen_GBps;                 /* the pairing kept, on the longer confirming probe */
  float best_GBps, worst_GBps;       /* over the pairing probes */
  float out_prescan_GBps[18];        /* output candidates under input 0, allocation order; 0 = none */
  int32_t out_kept[18];              /* allocation-order indices of the outputs that went on to the pairing probes; -1 = none */
  float hunt_ms;                     /* wall-clock time of the whole hunt (allocations, probes, frees); 0 without a hunt */
  int32_t stopped_by;                /* 0: ran to its end; 1: the byte budget cut candidates; 2: the time budget ended it early */
  uint64_t peak_bytes;               /* most device memory this call held at once, the ring's own two slabs included */
  uint64_t budget_bytes;             /* the byte budget it ran under (after defaults and clamping) */
  int32_t evicted;                   /* candidate slabs freed before the choice to make room (0 when the budget held them all) */
  int32_t reserved;
} bt709hip_ring_placement;
/* Budget of the placement hunt.  A zeroed struct (or NULL) = the defaults. */
typedef struct {
  uint64_t max_bytes;   /* most device memory the call may hold at once, the ring's two slabs included; 0 = the default: twice the
                           ring (frugal).  A budget that cannot hold the ring plus one more output slab leaves nothing to compare:
                           the ring is then allocated without a hunt */
  uint32_t max_ms;      /* wall-clock budget of the hunt in milliseconds (checked before every probe); 0 = none */
  int32_t frugal;       /* != 0: twice the ring whatever max_bytes says, one input candidate: the incumbent pair and the pair being
                           probed are all that ever lives (what max_bytes = 0 selects since round 6) */
  int32_t format;       /* render target of the ring's outputs: BT709HIP_FORMAT_BGRA8_SRGB (0, the default) or BT709HIP_FORMAT_RGBA16F
                           (8 bytes per pixel, linear-light halves: the reference's fallback intermediate, AAPLRenderer.m:143-170; not
                           with half_scale).  The hunt then probes with THAT launch: the RGBA16F kernel's 84 %-written stream lands
                           in the slow or the fast regime by the same lottery (0.70 against 0.77) (ABI 502) */
  int32_t reserved;
} bt709hip_ring_options;
int bt709hip_ring_create(bt709hip_decoder *dec, int width, int height, int frames, int half_scale, int tries, bt709hip_ring **out);
/* the same with an explicit budget (bt709hip_ring_create = options NULL) */
int bt709hip_ring_create_ex(bt709hip_decoder *dec, int width, int height, int frames, int half_scale, int tries,
                            const bt709hip_ring_options *options, bt709hip_ring **out);
int bt709hip_ring_destroy(bt709hip_ring *ring);
int bt709hip_ring_frames(const bt709hip_ring *ring);
/* Descriptors of frame `index` (any of the three pointers may be NULL; alpha is zeroed for an opaque decoder). */
int bt709hip_ring_frame(const bt709hip_ring *ring, int index, bt709hip_frame *frame, bt709hip_frame *alpha, bt709hip_surface *out);
int bt709hip_ring_placement_info(const bt709hip_ring *ring, bt709hip_ring_placement *info);
/* Frames [first, first + count) in ONE launch on `stream`. */
int bt709hip_ring_decode(bt709hip_ring *ring, int first, int count, void *stream, int wait_until_completed);

/* ----------------------------------------------------------------- ring set */
/* ONE process, SEVERAL GPUs, frames resident in DEVICE memory: a bt709hip_ring per lane, each with a context and a decoder of
 * its own on device_ordinals[lane] (ordinals may repeat), driven by ONE thread -- the reference's shape, one process that drives
 * everything (Renderer/AAPLRenderer.m:874-985), widened to the GPUs of a node.  bt709hip_ringset_decode issues ONE ring launch
 * per lane, in lane order, on each lane's default stream and returns (the launches run concurrently, one per device; a launch
 * call costs ~10 us of host time against ~1.8 ms of kernel for a 256-frame 4K ring); _synchronize waits for every lane.  No
 * collective, no peer access: nothing crosses GPUs.  The host-frame counterpart is the frame sharder below.  Each lane's ring
 * is created like bt709hip_ring_create_ex's (placement hunt per device, same budget semantics, per device).  Fill the rings
 * through bt709hip_ringset_lane_ring + bt709hip_ring_frame + bt709hip_upload on bt709hip_ringset_lane_context. */
typedef struct bt709hip_ringset bt709hip_ringset;
int bt709hip_ringset_create(const int *device_ordinals, int lanes, int gamma, int has_alpha, int width, int height, int frames,
                            int half_scale, int tries, const bt709hip_ring_options *options, bt709hip_ringset **out);
int bt709hip_ringset_destroy(bt709hip_ringset *set);
int bt709hip_ringset_lanes(const bt709hip_ringset *set);
bt709hip_context *bt709hip_ringset_lane_context(bt709hip_ringset *set, int lane);
bt709hip_decoder *bt709hip_ringset_lane_decoder(bt709hip_ringset *set, int lane);
bt709hip_ring *bt709hip_ringset_lane_ring(bt709hip_ringset *set, int lane);
/* frames [first, first + count) of EVERY lane's ring: one launch per lane, issued from the calling thread */
int bt709hip_ringset_decode(bt709hip_ringset *set, int first, int count, int wait_until_completed);
int bt709hip_ringset_synchronize(bt709hip_ringset *set);

/* ------------------------------------------------------------ frame sharder */
/* ONE process driving SEVERAL GPUs: independent frames shard with no exchange step, frame i (in submission
 * order) goes to lane i mod n.  The reference is one process with one device, one queue and N frames in
 * flight (Renderer/MetalRenderContext.m:59-63, Renderer/AAPLRenderer.m:34, 874-985); its counterpart on an
 * 8-GPU node is this dispatcher over n lanes, each lane = its own bt709hip_context + decoder + in-flight pool
 * of `depth` slots (one HIP stream, pinned staging and device buffers per slot) on device_ordinals[lane].
 * Ordinals may repeat (several lanes on one GPU).  No collective, no peer access, nothing crosses GPUs.
 *   acquire -> ticket + pinned Y / CbCr (/ alpha) planes of the next frame's slot (waits for that slot's previous frame)
 *   commit  -> upload, decode, download enqueued on the slot's stream of the ticket's lane; returns at once
 *   submit  -> acquire + copy of caller-owned host planes (any pitch; tags validated as -decodeBT709: does) + commit
 *   wait    -> the frame's pinned BGRA rows, valid until its slot is handed out again: lanes * depth frames later (sooner if
 *              frames of its lane were cancelled or failed in between); BT709HIP_ERR_INVALID_ARG once recycled
 *   cancel  -> hands an acquired, uncommitted ticket back
 * Threading: a shard is driven by ONE thread at a time (like a pool); that thread only enqueues, the lanes'
 * streams run concurrently.  Several feeding threads use a shard each (contexts are per shard).
 * Frames that already live in device memory: bt709hip_ringset_* above. */
typedef struct bt709hip_shard bt709hip_shard;
int bt709hip_shard_create(const int *device_ordinals, int lanes, int gamma, int has_alpha, int width, int height, int depth,
                          bt709hip_shard **out);
int bt709hip_shard_destroy(bt709hip_shard *shard);
int bt709hip_shard_lanes(const bt709hip_shard *shard);
int bt709hip_shard_lane_device(const bt709hip_shard *shard, int lane);
bt709hip_decoder *bt709hip_shard_lane_decoder(bt709hip_shard *shard, int lane); /* for set_option / set_alpha_fill */
int bt709hip_shard_acquire(bt709hip_shard *shard, uint64_t *ticket, void **y, size_t *y_stride, void **cbcr, size_t *cbcr_stride,
                           void **alpha, size_t *alpha_stride);
int bt709hip_shard_commit(bt709hip_shard *shard, uint64_t ticket);
int bt709hip_shard_cancel(bt709hip_shard *shard);
int bt709hip_shard_submit(bt709hip_shard *shard, const bt709hip_frame *host_frame, const bt709hip_frame *host_alpha,
                          uint64_t *ticket);
int bt709hip_shard_wait(bt709hip_shard *shard, uint64_t ticket, const void **bgra, size_t *stride);

/* -------------------------------------------------------------- diagnostics */
/* Streaming copy of `bytes` (a multiple of 16, both pointers 16-byte aligned) with 16-byte
 * non-temporal loads and stores, one launch: the bandwidth a plain copy reaches on this device, for
 * benchmarks that want to report a kernel against the same box's copy rate (no reference twin). */
int bt709hip_copy_probe(bt709hip_context *ctx, void *dst, const void *src, size_t bytes, void *stream);
/* Placement-aware allocation of ONE streaming slab.  Takes up to `tries` candidates of `bytes` ONE AT A TIME against the incumbent
 * (two slabs are alive while one is probed, three for the moment of an allocation: the slab that lost stays until the next
 * candidate has its memory, so the allocator cannot hand the same block straight back; holding them all buys nothing), times a streaming copy (lower half onto upper half) plus a fill of the whole slab over each and keeps the fastest;
 * the slab kept has been overwritten by the probe (zero-filled) whenever a probe ran, and is NOT cleared otherwise (tries = 1, a slab
 * under 2 MiB).  rates_GBps (optional, `tries` floats; always fully written: 0 where no probe ran) receives the probe rates,
 * *chosen (optional) the index kept.  tries = 1 is bt709hip_malloc.
 * This is the WEAKER, cheaper probe: it ranks a slab by itself, with a generic kernel.  A frame ring should use
 * bt709hip_ring_create, which probes with the decoder's own launch and chooses the input x output PAIRING (worth a further
 * 1-2 %, profiles/r03_placement_cross.txt).  No reference twin (unified memory has no placement to choose). */
int bt709hip_malloc_streaming(bt709hip_context *ctx, size_t bytes, int tries, void **dptr, float *rates_GBps, int *chosen);

/* Introspection used by the parity tests (host memory out).
 * thresholds: 255 floats, t[k-1] = smallest x in [0,1] whose output byte is >= k.
 * constants:  8 floats {1/255, M_y, M_cr_r, M_cb_g, M_cr_g, M_cb_b, 16, 128}
 *             (matrix built as BT709.h:386-397). */
int bt709hip_gamma_thresholds(int gamma, float thresholds[255]);
/* The kernels' lookup of one saturated channel value x in [0,1], replayed on the host from the
 * host-built bucket table (same index function, same compare): the byte the GPU would produce, and
 * optionally the bucket count N and the bucket index.  Returns the byte, or <0 on a bad argument. */
int bt709hip_gamma_lookup(int gamma, float x, int *bucket_count, int *bucket_index);
/* The same for the table the 1:1 kernels (decode, +unconvert:) stage: where the uniform table is large because the thresholds
 * crowd near zero (the LINEAR mode: 4 096 buckets) they use a LOG-bucket form of it, bucket = (bits(x + a) >> 16) - first, a = 2^-5
 * (645 buckets); for the other modes this is bt709hip_gamma_lookup.  *log_form (optional) = 1 / 0. */
int bt709hip_gamma_lookup_decode(int gamma, float x, int *bucket_count, int *bucket_index, int *log_form);
int bt709hip_matrix_constants(float constants[8]);
/* RGBA16F targets: the threshold table of the half-float composite H(x) = half(curve_to_linear(x))
 * (host memory out).  thresholds: up to `capacity` floats, T[i] = smallest x with H(x) >= first_code + i;
 * returns the number of entries the table has (0: the gamma has no curve), or <0. */
int bt709hip_half_thresholds(int gamma, float *thresholds, int capacity);
/* The kernels' settlement of one saturated x replayed on the host: the candidate is the exact code
 * H(x) moved by candidate_offset (0 or -1: the kernel's candidate, one fma over a tangent of the curve, lies below the true value and lands on
 * H or H - 1), then corrected against the one threshold above it.  Returns the half code;
 * *table_entries (optional) as above. */
int bt709hip_half_lookup(int gamma, float x, int candidate_offset, int *table_entries);
/* Name of the kernel the last decode on this thread launched (for profiling). */
const char *bt709hip_last_kernel_name(void);
/* Launch shape of the last decode, encode or plane shuffle this thread issued -- bt709hip_decode / _decode_batch (1:1, BGRA8 or RGBA16F target),
 * bt709hip_decode_half / _decode_half_batch (the short-lived 2:1 kernel: grid = tiles, groups of output rows, frames; the persistent one:
 * grid = (workgroups, 1, 1), block = the lanes of a tile row; launches 1, xcd_bands 0) or
 * bt709hip_encode / _encode_batch (grid = tiles [x 8 under the XCD-aware map], row-pair groups, pictures [per band]) or
 * bt709hip_interleave_cbcr / _deinterleave_cbcr (grid = 256-lane groups, chroma rows, 1): grid and block of its
 * first kernel launch, the number of launches it took (2: the XCD-aware map over a multiple of 8 frames plus the plain map
 * over the rest) and the work map of the first (bt709hip_decoder_option BT709HIP_OPT_XCD_BANDS value actually used; 0 plain). */
typedef struct {
  uint32_t grid[3], block[3];
  int32_t launches, xcd_bands;
} bt709hip_launch_info;
int bt709hip_last_launch_info(bt709hip_launch_info *info);
/* The plan of the last bt709hip_decode_scaled(_batch) / bt709hip_render_scaled(_batch) this thread issued, as its launcher settled it
 * (tests assert the regime a shape ran in through it: tap form, strip length, persistent item loop, one-generation cut or per-CU
 * rule).  BT709HIP_ERR_NOT_SETUP while this thread has launched neither (ABI 503). */
enum { BT709HIP_SCALED_TAPS_BYTES = 0, BT709HIP_SCALED_TAPS_PAIRS = 1, BT709HIP_SCALED_TAPS_WIDE = 2, BT709HIP_SCALED_TAPS_SHARED = 3,
       BT709HIP_SCALED_TAPS_ONCE = 4 };
typedef struct {
  uint32_t grid[3], block[3];
  uint32_t taps;        /* tap form as launched (BT709HIP_SCALED_TAPS_*); render_scaled: 0 */
  uint32_t rows;        /* output rows per strip */
  uint32_t persistent;  /* 1: workgroups walk `items` by gridDim.x */
  uint32_t balanced;    /* 1: the one-generation cut chose `rows`, 0: the per-CU rule */
  uint32_t resident;    /* workgroups the chip holds at once, as the launcher worked it out (0 for render_scaled) */
  uint32_t reserved;
  uint64_t items;       /* work items = column tiles x strips x frames */
} bt709hip_scaled_launch_info;
int bt709hip_last_scaled_launch_info(bt709hip_scaled_launch_info *info);

#ifdef __cplusplus
}
#endif
#endif /* BT709HIP_EXT_H */
