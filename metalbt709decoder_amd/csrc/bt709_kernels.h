// Kernel parameter block and launchers shared by bt709_kernels.hip and the C-ABI shim.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "transfer_tables.h"

namespace bt709 {

constexpr int kBlockThreads = 256;     // general-path workgroup: 4 waves of 64
// (tools/decode_lab overrides these two with -D to A/B other tile shapes)
#ifndef BT709_MAX_BLOCK_THREADS
#define BT709_MAX_BLOCK_THREADS 512
#endif
#ifndef BT709_QUADS_PER_LANE
#define BT709_QUADS_PER_LANE 2
#endif
constexpr int kMaxBlockThreads = BT709_MAX_BLOCK_THREADS;  // fast-path workgroup is sized per frame width, up to 8 waves
constexpr int kQuadsPerLane = BT709_QUADS_PER_LANE;        // 4x2-pixel quads a fast-path lane owns per row pair
constexpr int kMaxBatch = 32;          // == BT709HIP_MAX_BATCH: frames in the kernarg table
// XCD-aware work map (bt709_tile.h banded_work; bt709_launch.h plan_bands): used for launches of a multiple of 8 frames from this many on.
// Measured (round 3, same call, plain vs banded): decode 32 frames 0.756 / 0.741-0.761, 64 0.741 / 0.745-0.760, 128 0.72 / 0.77,
// 256 0.70 / 0.76-0.81; encoder 32 pictures 0.70 / 0.67, 256 0.69 / 0.73: a band needs ~8 frames to pay.
#ifndef BT709_XCD_BAND_MIN_FRAMES
#define BT709_XCD_BAND_MIN_FRAMES 64
#endif
constexpr int kXcdBandMinFrames = BT709_XCD_BAND_MIN_FRAMES;
constexpr int kMaxUniformBatch = 65535;  // evenly spaced frames per launch (grid.z limit)

enum KernelVariant : int {
  kVariantQuads = 0,   // aligned fast path, 4x2 pixels per lane
  kVariantBlocks = 1,  // general path, 2x2 pixels per lane
};

struct FramePlanes {
  const uint8_t *y;
  const uint8_t *cbcr;
  const uint8_t *alpha;  // nullptr unless the decoder has an alpha channel
  uint8_t *out;
};

// Passed by value in the kernarg segment (32 frames x 32 B + ~150 B).
struct DecodeParams {
  FramePlanes frames[kMaxBatch];
  // decode kernels: TransferBucket[N + 1], edges in x units (transfer_tables.h buckets_unit)
  const void *table_unit;
  // rescale kernels: TransferBucketLinear[N + 1] (edges in x units) and the sRGB-encode table in LOG-bucket form
  // (transfer_tables.h TransferTable::buckets_log of the LINEAR composite): bucket of a mean v = (bits(v + encode_log_add) >> 16) - encode_log_first
  const void *table_linear;
  const void *table_encode;
  // persistent 2:1 kernel, encode side: the same composite as a uniform table with a non-power-of-two
  // bucket count (transfer_tables.h UniformTable): index by two multiplies and an add
  const void *table_encode_u;
  uint32_t table_encode_u_bytes;
  float encode_u_n;
  uint32_t table_unit_bytes;
  uint32_t table_linear_bytes;
  uint32_t table_encode_bytes;
  float encode_log_add;
  uint32_t encode_log_first;
  float unit_magic;    // 2^23 / N: floats in [M, 2M) have ulp 1/N (bt709_device.h magic_index12): table_linear's index
  // table_unit's index (the 1:1 kernels): q = (bits(x + unit1_magic) >> unit1_shift) - unit1_first.  Uniform form: the same M,
  // shift 0, first = bits(M); log-bucket form (transfer_tables.h TransferTable::buckets_log): log_add, 16, log_first.
  float unit1_magic;
  uint32_t unit1_first, unit1_shift;
  uint32_t width;      // luma (source) dimensions
  uint32_t height;
  uint32_t y_stride;
  uint32_t cbcr_stride;
  uint32_t alpha_stride;
  uint32_t out_stride;
  uint32_t alpha_word;  // alpha_fill << 24
  // decode_nv12_scaled only: output size and source-per-output-pixel ratios W/OW, H/OH (float)
  uint32_t out_width, out_height;
  float scale_x, scale_y;
  uint32_t scaled_rows;  // output rows of a strip (filled by launch_decode_scaled)
  // uniform != 0: frame i = frames[0] + i * step_* (bytes); lets one launch cover any number of frames
  uint32_t uniform;
  int64_t step_y, step_cbcr, step_alpha, step_out;
  // decode_nv12_half_rep only (persistent workgroups, replicated LDS tables): table_linear is held
  // in 2^rep_dec_log2 interleaved copies (<= 16: one per lane of a ds_read_b128 lane group),
  // table_encode in 2^rep_enc_log2; a tile row is one tile of one row pair of one frame, tile_rows
  // of them in the launch, walked gridDim.x at a time; cursor_* = gridDim.x decomposed into
  // (tiles, row pairs, frames).  Filled by launch_decode_half_rep.
  // The planar CHW targets of the 1:1 decode (bt709_chw.hip; BT709HIP_FORMAT_CHW_*) never meet that kernel, and
  // their launch carries its element type and normalisation in the same seven words: a field of its own would move every field
  // and implicit argument behind it, and with them the code of every kernel that takes this block.  chw_elem != kChwNone routes
  // launch_decode to launch_decode_chw; frames[i].out is then the base of plane 0 and out_stride the row pitch of every plane.
  union {
    struct {
      uint32_t rep_dec_log2, rep_enc_log2;
      uint32_t tiles_x, tile_rows;
      uint32_t cursor_tx, cursor_rp, cursor_f;
    };
    struct {
      uint32_t chw_elem;                 // kChwNone / kChwU8 / kChwF16 / kChwF32
      float chw_scale[3], chw_bias[3];  // R, G, B: BT709HIP_OPT_CHW_SCALE_* / _BIAS_* (bt709_chw_norm.h)
    };
  };
  // XCD-aware work map of the short-lived kernels (filled by the launchers): grid.x = 8 x tiles, x & 7 = the workgroup's
  // place in the round-robin over the XCDs, which owns frames [(x & 7) * frames_per_band, ...) of the launch
  uint32_t xcd_bands, frames_per_band;
  // The any-ratio rescale through the RGBA16Float intermediate (bt709_rescale_f16.hip decode_nv12_scaled_f16;
  // BT709HIP_OPT_SCALE_INTERMEDIATE): scale_f16 != 0 selects it in launch_decode_scaled, and the decoder's half lookup rides
  // along -- HalfParams' table (nullptr / 0 bytes: no curve), where its candidate entries start, and the lookup's two constants
  uint32_t scale_f16;
  uint32_t half_table_bytes, half_cand_offset, half_h_min;
  float half_index_scale;
  const void *half_table;
  // BT709HIP_OPT_COMPOSITE_OVER (alpha decoders, the 1:1 kernels) and BT709HIP_OPT_SCALED_OVER (the any-ratio
  // rescale kernels; 3.6): the word goes source-over a background in linear light before it is stored.  over_mode selects the
  // *_over kernels in launch_decode / launch_decode_scaled (each filled by the shim from its own option); over_table_lin is
  // lin[256] = sRGB_nonLinearNormToLinear(byteNorm(b)) as floats (the encode side is table_encode); kOverColour: the three
  // lin[] of the solid colour's R, G, B, looked up on the host
  uint32_t over_mode;  // kOverOff / kOverDestination / kOverColour
  float over_lin[3];
  const void *over_table_lin;
  // BT709HIP_OPT_CHROMA_LAYOUT (the 1:1 kernels of the caller's frames): kChromaI420 = frames[i].cbcr is the U (Cb) plane, W/2 x
  // H/2 bytes at pitch cbcr_stride, and the V (Cr) plane the same shape v_offset = (H/2) * cbcr_stride bytes behind it;
  // launch_decode then runs the kChromaI420 instantiations of its kernels, and launch_decode_scaled (BT709HIP_OPT_SCALED_PLANAR: the
  // shim hands it such a block only with that option on) the kernels of bt709_rescale_planar.hip.  Every other launcher reads NV12 whatever this holds.
  uint32_t chroma_layout;  // kChromaNV12 / kChromaI420
  // BT709HIP_OPT_UNPREMULTIPLY (alpha decoders, the 1:1 kernels into BGRA8_SRGB): != 0 selects the straight-alpha
  // instantiations in launch_decode; the shim never sets it together with over_mode.  (It sits in what was a reserved word: every
  // other field's offset is what it was.)
  uint32_t straight_alpha;
  uint64_t v_offset;
};
// The CHW words ARE the persistent 2:1 kernel's seven, no more and no fewer, and the block is the size it was: a field that moved
// would change every kernel that takes the block (profiles/r21_chw_isa.txt).  launch_decode reads chw_elem as its route, so a block
// handed to it must have come from a zeroed one (gather_batch) -- launch_decode_half_rep fills rep_* in a private copy that never
// reaches launch_decode.
static_assert(offsetof(DecodeParams, chw_elem) == offsetof(DecodeParams, rep_dec_log2) && offsetof(DecodeParams, chw_scale) == offsetof(DecodeParams, rep_enc_log2) &&
                  offsetof(DecodeParams, chw_bias) == offsetof(DecodeParams, cursor_tx) && offsetof(DecodeParams, chw_bias) + sizeof(float[3]) == offsetof(DecodeParams, xcd_bands),
              "the CHW fields alias rep_dec_log2 .. cursor_f exactly");
// The any-ratio rescale into CHW targets (bt709_rescale_chw.hip) meets the same union from its other side: gather_batch
// fills chw_elem, chw_scale and chw_bias, and launch_decode_scaled fills tiles_x and tile_rows for its persistent forms -- the words of
// chw_scale[1] and chw_scale[2].  So that launcher moves the three scales, in its private copy and before it plans the grid, into
// over_lin[3], which a CHW launch never needs (it is never blended) and which is the only place the CHW rescale kernels read them from;
// chw_elem and chw_bias lie on rep_dec_log2 and cursor_*, which no any-ratio kernel reads or launcher writes, and stay where they are.
static_assert(offsetof(DecodeParams, tiles_x) == offsetof(DecodeParams, chw_scale) + sizeof(float) &&
                  offsetof(DecodeParams, tile_rows) == offsetof(DecodeParams, chw_scale) + 2 * sizeof(float) &&
                  offsetof(DecodeParams, chw_bias) == offsetof(DecodeParams, cursor_tx),
              "launch_decode_scaled's tiles_x / tile_rows overwrite chw_scale[1..2] and nothing else of the CHW fields");
static_assert(offsetof(DecodeParams, over_lin) >= offsetof(DecodeParams, xcd_bands) && sizeof(DecodeParams::over_lin) == sizeof(DecodeParams::chw_scale),
              "the CHW rescale's scales travel in over_lin, outside the words the launcher fills");
static_assert(sizeof(DecodeParams) == 1288 && offsetof(DecodeParams, v_offset) == 1280, "a field added to DecodeParams moves the implicit kernel arguments behind it: every decode kernel's code changes");
enum : uint32_t { kChromaNV12 = 0, kChromaI420 = 1 };  // == BT709HIP_CHROMA_*
enum : uint32_t { kChwNone = 0, kChwU8 = 1, kChwF16 = 2, kChwF32 = 3 };  // DecodeParams::chw_elem: BT709HIP_FORMAT_CHW_* - 3
constexpr uint32_t chw_elem_bytes(uint32_t elem) { return elem == kChwF32 ? 4u : (elem == kChwF16 ? 2u : 1u); }
// First template argument of the 1:1 decode kernels and the colour encoder's kernels that have a straight-alpha twin: the chroma
// layout, plus kFormStraight for the twin (decode: R, G, B divided by A behind the arithmetic; encode: multiplied by A ahead of it)
enum : uint32_t { kFormStraight = 2 };
constexpr uint32_t form_layout(uint32_t form) { return form & 1u; }
constexpr bool form_straight(uint32_t form) { return (form & kFormStraight) != 0; }
enum : uint32_t { kOverOff = 0, kOverDestination = 1, kOverColour = 2 };
constexpr uint32_t kOverLinBytes = 256 * sizeof(float);

// Pass 1 into an RGBA16Float target (bt709_rgba16f.hip): the threshold table of transfer_tables.h
// HalfTable and the constants of the candidate.  Travels beside DecodeParams (frames, pitches).
struct HalfParams {
  const void *table;     // float T[]: T[i] = smallest x with H(x) >= h_min + i, then the candidate entries; nullptr: no curve (LINEAR)
  uint32_t table_bytes;  // 0 without a table; else thresholds + candidates
  uint32_t cand_offset;  // byte offset of the candidate entries {intercept, slope} (transfer_tables.h HalfTable::cand) in `table` = bytes of the thresholds
  float index_scale;     // HalfTable::index_scale: the split point lands on the bucket boundary 2^-4
  uint32_t h_min;        // first code the table covers
  uint32_t wide_store;   // 16-byte stores (target 16-byte aligned), else 8-byte; filled by the launcher
};
// LDS plan of decode_nv12_rgba16f: the thresholds from byte 0, the candidate entries from this FIXED byte on -- so that the
// address of a bucket's entry is its binary16 bits plus a compile-time constant (the ds_read's immediate offset).  Above the
// largest threshold image (sRGB: 8 602 floats), and low enough that thresholds + candidates stay under 40 KiB: four
// workgroups per CU.
constexpr uint32_t kHalfCandLds = 34560;
// decode_nv12_scaled_f16 keeps the same plan and puts its sRGB-encode buckets behind it: the host holds thresholds + candidates
// under 40 KiB (shim_decode.cpp ensure_half_table)
constexpr uint32_t kHalfPlanLds = 40u * 1024u;
const char *launch_decode_rgba16f(const DecodeParams &p, const HalfParams &hp, int frames, bool has_alpha,
                                  uint32_t in_align, uint32_t out_align, uint32_t compute_units, bool xcd_bands, hipStream_t stream);
hipError_t prepare_rgba16f_kernels();  // bt709_rgba16f.hip

// Pass 1 into planar CHW tensors (bt709_chw.hip): reached through launch_decode alone (chw_elem, above), which hands on what it
// was handed.  Fast path (kVariantQuads): launch_decode's plan, tile for tile; general path: its grid-strided walk.
const char *launch_decode_chw(const DecodeParams &p, int frames, int variant, bool has_alpha, bool quantiser, bool nontemporal,
                              int xcd_bands, uint32_t grid_x, uint32_t block_threads, hipStream_t stream);
hipError_t prepare_chw_kernels();  // called by prepare_kernels

// Pass 2 alone (bt709_rescale_scaled.hip render_scaled): an intermediate surface -> a BGRA8 sRGB surface of any size.
struct RenderParams {
  const uint8_t *in;   // BGRA8 sRGB words or RGBA16Float texels
  uint8_t *out;        // BGRA8 sRGB
  uint32_t in_stride, out_stride;
  uint32_t width, height, out_width, out_height;
  float scale_x, scale_y;
  uint32_t rows;       // output rows a workgroup walks (filled by the launcher)
  // tables (device): log-bucket sRGB-encode buckets and lin[256] = sRGB_nonLinearNormToLinear(byteNorm(b))
  // (the alpha channel is filtered and quantised in arithmetic)
  const void *table_encode, *table_lin;
  uint32_t table_encode_bytes;
  float encode_log_add;        // table_encode is the log-bucket form (as DecodeParams)
  uint32_t encode_log_first;
  int64_t in_step, out_step;  // batched launches: surface i of the launch = surface 0 + i * step (evenly spaced, as in a ring)
};
// The plan a rescale launcher settled on (bt709hip_last_scaled_launch_info: tests assert the regime a shape ran in through it).
// The tap forms' values are part of the C ABI (BT709HIP_SCALED_TAPS_*).
enum : int { TAPS_BYTES = 0, TAPS_PAIRS = 1, TAPS_WIDE = 2, TAPS_SHARED = 3, TAPS_ONCE = 4 };
struct ScaledLaunchRecord {
  uint32_t grid[3], block[3];
  uint32_t taps, rows, persistent, balanced, resident, reserved;
  uint64_t items;  // cols x strips x frames
};
// The two rescale launchers hand the plan of every launch they make to the host shim, which keeps it per thread next to the kernel
// name (shim_core.cpp defines this).  A call and not an out-parameter: the launchers' signatures stay what test doubles link against.
void record_scaled_launch(const ScaledLaunchRecord &record);
// The any-ratio kernels and pass 2 alone form row offsets in 32 bits (the scalar offset of a raw buffer resource of 2^31 - 1
// records): a plane of `rows` rows must end below 2 GiB.  What the two launchers refuse with nullptr (and their test doubles with them).
inline bool plane_fits(uint64_t rows, uint64_t stride) { return rows * stride < (1ull << 31); }
// A planar CHW target (chw_elem set): its 3 or 4 planes are ONE surface to the kernels, which reach plane c through a 32-bit offset
// c x OH x pitch -- all of them together must end below 2 GiB.
inline bool scaled_planes_fit(const DecodeParams &p, bool has_alpha) {
  const uint64_t out_planes = p.chw_elem != kChwNone ? (has_alpha ? 4u : 3u) : 1u;
  return plane_fits(p.height, p.y_stride) && plane_fits(p.height / 2, p.cbcr_stride) && (!has_alpha || plane_fits(p.height, p.alpha_stride)) &&
         plane_fits(out_planes * p.out_height, p.out_stride);
}
inline bool render_planes_fit(const RenderParams &p) { return plane_fits(p.height, p.in_stride) && plane_fits(p.out_height, p.out_stride); }
// grid = (column tiles, strips of `rows` output rows, frames)
const char *launch_render_scaled(const RenderParams &p, int frames, bool in_rgba16f, uint32_t compute_units, hipStream_t stream);

// BGRA -> NV12 / I420 encoder (bt709_encode.hip).
struct EncodeFrame {
  const uint8_t *bgra;  // W x H words (A<<24)|(R<<16)|(G<<8)|B, alpha ignored
  uint8_t *y;
  uint8_t *cbcr;        // alpha kernels: nullptr in EVERY frame of the launch = write no CbCr plane
};
// BT709HIP_CTX_OPT_ENCODE_WITH_ALPHA: a picture's colour frame and its alpha frame (Y = T[A]) from one launch.  The
// frames[] area read as kMaxPairBatch entries; entry 0 begins as frames[0] does.  The spare slots carry what has no field:
//   pairs[0].spare = alpha_y_stride | alpha_cbcr_stride << 32, pairs[1].spare = the alpha Y step, pairs[2].spare = the alpha chroma step
// (bytes, as step_y / step_cbcr; read under `uniform` alone).  alpha_cbcr: nullptr in EVERY pair of the launch = no alpha chroma plane.
struct EncodePair {
  const uint8_t *bgra;
  uint8_t *y, *cbcr;
  uint8_t *alpha_y, *alpha_cbcr;
  int64_t spare;
};
constexpr int kMaxPairBatch = kMaxBatch / 2;  // pairs in the kernarg table
static_assert(sizeof(EncodePair[kMaxPairBatch]) == sizeof(EncodeFrame[kMaxBatch]), "the pair table is the frame table's bytes");
// BT709HIP_CTX_OPT_ENCODE_CHW_INPUT: a planar-tensor launch (input_format kEncodeInputCHW*).  The frames[] area again, as
// EncodePair shortened it: one entry fewer, and in its 24 bytes the six binary32 the float kernels read -- s = sat(t * scale[c] + bias[c]),
// c = R, G, B (bt709_chw_denorm.h).  Entry i IS frames[i]: encode_frame and advance_frames read it through that member.
constexpr int kMaxChwBatch = kMaxBatch - 1;  // surfaces in the kernarg table of a CHW launch
struct EncodeChwTable {
  EncodeFrame frames[kMaxChwBatch];  // bgra: the base of plane 0 (R); plane c is c * height * bgra_stride bytes behind it
  float scale[3], bias[3];
};
static_assert(sizeof(EncodeChwTable) == sizeof(EncodeFrame[kMaxBatch]), "the CHW table is the frame table's bytes");
struct EncodeParams {
  union {
    EncodeFrame frames[kMaxBatch];
    EncodePair pairs[kMaxPairBatch];  // a paired launch: alpha_luma AND per_byte non-null (below)
    EncodeChwTable chw;               // a planar-tensor launch: input_format kEncodeInputCHW*
  };
  // uniform != 0: frame i = frames[0] + i * step_* (bytes), as in DecodeParams
  uint32_t uniform;
  // BT709HIP_CTX_OPT_ENCODE_CHROMA_LAYOUT: kChromaI420 = frames[i].cbcr is the U (Cb) plane, W/2 x H/2 bytes at pitch cbcr_stride,
  // and the V (Cr) plane the same shape (H/2) * cbcr_stride bytes (a 64-bit product, formed by the kernels) behind it;
  // launch_encode then runs the kChromaI420 instantiations of its kernels.  kChromaNV12 whenever the frames carry no chroma plane (alpha frames).
  // (It sits in what was padding: the kernarg block and every other field's offset are what they were.)
  uint32_t chroma_layout;  // kChromaNV12 / kChromaI420
  int64_t step_bgra, step_y, step_cbcr;
  // BT709HIP_CTX_OPT_ENCODE_CONVERT: convert_mode != kConvertOff selects the per-pixel converter's kernels in
  // launch_encode (convert_bgra / convert_bgra_blocks, bt709_encode_convert.h), which read convert_curve -- 256 floats,
  // transfer_tables.h build_convert_curve -- and none of per_byte / from_linear* / alpha_luma.
  //   kConvertPacked444: frames[i].y is W x H 32-bit words (Cr<<16)|(Cb<<8)|Y at pitch y_stride, frames[i].cbcr nullptr;
  //   kConvertPoint420:  frames[i] is an NV12 / I420 frame as above; a block's chroma is its bottom-left pixel's.
  // Neither is a field of its own: a field appended to this block moves the implicit arguments behind it and with them one
  // s_load offset and the kernarg size of EVERY encoder kernel (profiles/r15_straight_alpha_isa.txt).  The curve travels in the slot
  // of the table the converter does not read, the mode in the upper half of the selector word no kernel reads.
  union {
    const EncodeByteEntry *per_byte;  // 256 entries for the (input gamma, output gamma) pair
    const float *convert_curve;       // convert_mode != kConvertOff
  };
  const TransferBucket *from_linear;  // two-resolution BT709_from_linear(., output gamma) table (SplitTable)
  uint32_t from_linear_bytes;
  float from_linear_scale;    // its n_fine
  // BT709HIP_CTX_OPT_ENCODE_PREMULTIPLY (BGRA8_SRGB input): != 0 selects the premultiplying instantiations of
  // encode_bgra / encode_bgra_blocks in launch_encode; no kernel reads it.  (It sits where the split point of the two-resolution
  // table was carried, which nothing had read since the index became a min(): every other field's offset, and the kernarg
  // block's size, are what they were.)
  uint8_t premultiply;
  // BT709HIP_CTX_OPT_ENCODE_HALF_INPUT: kEncodeInputRGBA16F = frames[i].bgra holds RGBA16Float linear-light texels
  // (8 bytes each, bgra_stride their pitch) and launch_encode runs encode_rgba16f / encode_rgba16f_blocks (bt709_encode_half.h), which
  // read from_linear* and not per_byte.  A selector of launch_encode, read by no kernel; the upper byte of what `premultiply`
  // (0 or 1) occupied: no offset and no size changes.
  // kEncodeInputCHWU8 / F16 / F32: frames[i].bgra is plane 0 of a planar tensor of that element type, bgra_stride
  // the pitch of every plane's rows, and launch_encode runs encode_chw / encode_chw_blocks (bt709_encode_chw.h).
  uint8_t input_format;  // kEncodeInput*
  uint16_t convert_mode;  // kConvert*: a selector of launch_encode as well, read by no kernel
  float from_linear_coarse;   // fine buckets below the table's split point, coarse ones above: q = (uint)(xs * coarse) + offset
  uint32_t from_linear_offset;
  uint32_t row_pairs_per_block;  // consecutive row pairs a fast-path workgroup walks; 0 = encode_row_pairs_per_block()
  uint32_t block_threads;        // fast-path workgroup size (one quad per lane); 0 = encode_block_threads(width)
  uint32_t width, height;
  uint32_t bgra_stride, y_stride, cbcr_stride;
  uint32_t xcd_bands, frames_per_band;  // XCD-aware work map, as in DecodeParams (filled by launch_encode)
  // BT709HIP_FORMAT_BGRA8_ALPHA: non-null selects the alpha kernels (encode_alpha_y / encode_alpha_y_blocks): 256 bytes
  // T[A], four per word (bt709_alpha_luma.h); per_byte / from_linear* are not read then.
  // Non-null TOGETHER WITH per_byte (convert_mode kConvertOff) is the selector of the paired kernels (encode_pair): they read both
  // sets of tables and pairs[] in place of frames[].  No field or bit of its own: the alpha kernels alone leave per_byte null.
  const uint32_t *alpha_luma;
};
inline bool encode_pair(const EncodeParams &p) { return p.alpha_luma != nullptr && p.per_byte != nullptr; }
static_assert(sizeof(EncodeParams) == 880, "a field appended to EncodeParams moves the implicit kernel arguments behind it: every encoder kernel's code changes");
enum : uint8_t { kEncodeInputBGRA8 = 0, kEncodeInputRGBA16F = 1, kEncodeInputCHWU8 = 2, kEncodeInputCHWF16 = 3, kEncodeInputCHWF32 = 4 };
constexpr bool encode_input_chw(uint8_t format) { return format >= kEncodeInputCHWU8 && format <= kEncodeInputCHWF32; }
constexpr uint32_t encode_chw_elem(uint8_t format) { return static_cast<uint32_t>(format - kEncodeInputCHWU8) + 1u; }  // kChwU8 / kChwF16 / kChwF32
enum : uint32_t { kConvertOff = 0, kConvertPacked444 = 1, kConvertPoint420 = 2 };  // == BT709HIP_CONVERT_*
// Further bit of the converter kernels' FORM (beside the layout and kFormStraight): the packed 4:4:4 output
enum : uint32_t { kFormPacked = 4 };
constexpr bool form_packed(uint32_t form) { return (form & kFormPacked) != 0; }
// Further bit of the colour encoder kernels' FORM: the alpha frame rides along (EncodePair)
enum : uint32_t { kFormPair = 8 };
constexpr bool form_pair(uint32_t form) { return (form & kFormPair) != 0; }
const char *launch_encode(const EncodeParams &p, int frames, bool fast, bool xcd_bands, hipStream_t stream);
hipError_t prepare_encode_kernels();
// Encoder fast-path geometry, measured on 4K (tools/encode_shapes.sh sweeps):
// one quad per lane, equal tiles of <= 320 lanes rounded up to whole waves (3840 -> 3 x 320,
// 1920 -> 2 x 256); a workgroup walks 3 to 9 consecutive row pairs (amortising its 8 KiB of
// table staging): the most that still leaves the launch >= 4096 workgroups.
inline uint32_t encode_block_threads(uint32_t width) {
  const uint32_t quads = width / 4, tiles = quads == 0 ? 1 : (quads + 319) / 320;
  uint32_t t = ((quads + tiles - 1) / tiles + 63) / 64 * 64;
  return t < 64 ? 64 : t;
}
inline uint32_t encode_row_pairs_per_block(uint32_t width, uint32_t height, uint32_t frames) {
  const uint32_t threads = encode_block_threads(width);
  const uint64_t tiles = (width / 4 + threads - 1) / threads;
  for (uint32_t rp = 9; rp > 3; --rp)
    if (tiles * ((height / 2 + rp - 1) / rp) * frames >= 4096) return rp;
  return 3;
}

// Planar U,V <-> interleaved CbCr (bt709_planes.hip).  The kernel that reads a plane never writes it.
struct PlaneParams {
  const uint8_t *u;  // chroma_width x chroma_height bytes (written by deinterleave_cbcr)
  const uint8_t *v;
  uint8_t *cbcr;     // chroma_width byte pairs per row (read by deinterleave_cbcr)
  uint32_t u_stride, v_stride, cbcr_stride;
  uint32_t chroma_width, chroma_height;
  uint32_t wide;     // 1: 8 samples per lane with 8/16-byte accesses
};
const char *launch_planes(const PlaneParams &p, bool interleave, hipStream_t stream);
// 16-byte-per-lane non-temporal streaming copy (bt709_planes.hip): the same-box copy ceiling benchmarks report.
const char *launch_copy_probe(void *dst, const void *src, size_t bytes, hipStream_t stream);

// Shape of the kernel launches the last bt709hip_decode[_batch] or bt709hip_encode[_batch] call of this thread made (tests
// assert the XCD-aware map and the encoder's launch regimes through it: bt709hip_last_launch_info): grid and block of its FIRST
// launch, how many launches it took.
struct LaunchShape {
  uint32_t grid[3], block[3];
  int32_t launches, xcd_bands;
};
LaunchShape &last_launch_shape();  // thread-local (bt709_kernels.hip)

// Launchers return the kernel's name (static string) for profiling; launch errors
// are read by the caller with hipGetLastError().
// decode: variant kVariantQuads -> grid = (grid_x tiles, H/2, frames) x block_threads;
//         variant kVariantBlocks -> grid = (grid_x, frames) x kBlockThreads, grid-strided.
// quantiser: the decoder's mode is sRGB (arithmetic transfer step, no table); implied by has_alpha
// xcd_bands: use the XCD-aware work map when the launch allows it (fast path, frames a multiple of 8)
const char *launch_decode(const DecodeParams &p, int frames, int variant, bool has_alpha, bool quantiser, bool nontemporal,
                          int xcd_bands, uint32_t grid_x, uint32_t block_threads, hipStream_t stream);
// +unconvert: on packed 4:4:4 words (bt709_kernels.hip unconvert_packed444); `tables` supplies table_unit*, unit_magic, alpha_word.
// `count` frames of one geometry in one launch (grid.z): evenly spaced (in[0] + i * in_step), or through a pointer table of up to kMaxBatch
struct UnconvertBatch {
  int count;
  bool uniform;
  const void *const *in;  // count input pointers (uniform: only in[0] is read)
  void *const *out;
  int64_t in_step, out_step;
};
const char *launch_unconvert(const DecodeParams &tables, const UnconvertBatch &batch, size_t in_stride, size_t out_stride, uint32_t width,
                             uint32_t height, bool vec, bool quantiser, hipStream_t stream);
// half: grid = (grid_x, H/2 output rows, frames) x block_threads.
const char *launch_decode_half(const DecodeParams &p, int frames, bool wide, bool has_alpha, bool nontemporal,
                               uint32_t grid_x, uint32_t block_threads, hipStream_t stream);

// half, conflict-free form: grid = workgroups (<= compute units, one resident per CU) x block_threads,
// each walking tile rows workgroup, workgroup + grid, ...; fills the rep_*, tiles_x, tile_rows and cursor_*
// fields of its copy of `p`.  Returns nullptr when the tables do not fit LDS (caller falls back).
// lds_budget: LDS bytes one workgroup may take (kRepLdsBytes = one workgroup per CU).
const char *launch_decode_half_rep(const DecodeParams &p, int frames, bool has_alpha, bool nontemporal, uint32_t workgroups,
                                   uint32_t lds_budget, hipStream_t stream);
constexpr int kRepBlockThreads = 1024;      // one workgroup per CU: 16 waves
constexpr uint32_t kRepLdsBytes = 160 * 1024;

// scaled: grid = (ceil(OW / kBlockThreads), ceil(OH / rows), frames) x kBlockThreads, rows chosen from the CU count.
// in_align: largest power of two dividing every input plane pointer, pitch and frame spacing (picks the tap fetch width).
// nullptr: a plane of 2 GiB or more (row offsets are formed in 32 bits)
const char *launch_decode_scaled(const DecodeParams &p, int frames, bool has_alpha, uint32_t in_align,
                                 uint32_t compute_units, hipStream_t stream);

// Fast-path launch geometry for a frame width: tiles (workgroups) per row pair and the
// workgroup size -- ceil(quads per tile / kQuadsPerLane) rounded up to a whole wave.
//   3840 -> 1 tile x 512 threads (480 rounded up to whole waves), 1920 -> 1 x 256, 7680 -> 2 x 512.
inline uint32_t quads_tiles(uint32_t width) {
  const uint32_t quads = width / 4, cap = kMaxBlockThreads * kQuadsPerLane;
  return quads == 0 ? 1 : (quads + cap - 1) / cap;
}
inline uint32_t quads_block_threads(uint32_t width) {
  const uint32_t tiles = quads_tiles(width);
  const uint32_t per_tile = (width / 4 + tiles - 1) / tiles;
  uint32_t t = (per_tile + kQuadsPerLane - 1) / kQuadsPerLane;
  t = (t + 63) / 64 * 64;
  if (t < 64) t = 64;
  if (t > static_cast<uint32_t>(kMaxBlockThreads)) t = kMaxBlockThreads;
  return t;
}

// Row pairs stacked in one workgroup (blockDim.y): only when one tile spans the row and the
// row needs few threads, so the workgroup still has up to kMaxBlockThreads threads.
inline uint32_t quads_rows_per_block(uint32_t block_threads, uint32_t tiles) {
  if (tiles != 1 || block_threads == 0) return 1;
  const uint32_t by = kMaxBlockThreads / block_threads;
  return by < 1 ? 1 : by;
}

// Raise the dynamic-LDS cap of the kernels (bt709_launch.h raise_lds_cap).
hipError_t prepare_kernels();          // bt709_kernels.hip
hipError_t prepare_rescale_kernels();  // bt709_rescale_half.hip (+ bt709_rescale_scaled.hip's)

}  // namespace bt709
