#!/usr/bin/env python3
"""Lab builds of libbt709hip.so: the product sources plus the experiment gates that used to live in csrc/.

    python tools/lab_variants.py <out.so> [MACRO[=VALUE] | -flag ...]
    python tools/lab_variants.py --list
    python tools/lab_variants.py --sources      (only writes tools/bin/lab_src/, for tools/decode_lab.hip -DBT709_LAB_SRC)

Until round 4 the shipped translation units carried `#if defined(BT709_LAB_...)` branches (several of them WRONG-OUTPUT stubs
that delete work to measure a ceiling) one -D away from the product.  They are gone from csrc/: this script copies csrc/ to
tools/bin/lab_src/, re-inserts the gates below by exact text substitution (it fails loudly when the product text it
anchors on has changed -- then the experiment has to be re-stated against the new kernel, which is the point), and compiles
the copy with the requested macros through metalbt709decoder_amd.build's own flags.  The result is for bench.py --library /
tools/ab_libs.py only; nothing under tools/ is part of the product and a CPU test asserts csrc/ holds none of these macros.

Gates (macro -> what it does; profiles/ file it produced):
  BT709_LAB_NO_ARITH      1:1 kernel, WRONG OUTPUT: loads and stores with (almost) no arithmetic   r03_ab_ceiling.txt
  BT709_LAB_NO_LOADS      with NO_ARITH: the launch's stores alone                                  r03_ab_loads_stores_only.txt
  BT709_LAB_NO_STORES     with NO_ARITH: the launch's loads alone                                   r03_ab_loads_stores_only.txt
  BT709_LAB_NO_TABLE      with NO_ARITH: no table staging / barrier
  BT709_NO_FMA_CENTRE     centre_norm as add + multiply instead of one fma (same bytes out)         r02 ab_fma
  BT709_INDEX_RTZ         bucket index by a round-toward-zero add between two s_setreg (same bytes) r02 ab_index
  BT709_UNIFORM_INDEX_TWO_STEP   2:1 kernel encode index as multiply, then add (same bytes)
  BT709_REP_SPLIT_ENCODE  persistent 2:1 kernel with the two-resolution encode table (same bytes)
  BT709_LAB_BOUND_SHARED_INDEX   2:1 kernel, WRONG OUTPUT: 4 index adds per block instead of 12     r03_half_bounds.txt
  BT709_LAB_BOUND_ONE_ENCODE     2:1 kernel, WRONG OUTPUT: one encode lookup instead of three       r03_half_bounds.txt
  BT709_LAB_HALF_TABLE    2:1 kernel, WRONG OUTPUT: half-size decode-side table                     r03_ab_half_table.txt
  BT709_LAB_F16_NO_ARITH  RGBA16F kernel, WRONG OUTPUT: loads + stores, no lookups (_NO_TABLE: no staging)   r05_ab_rgba16f_ceiling.txt
  BT709_LAB_F16_CVT_ONLY  RGBA16F kernel, WRONG OUTPUT: matrix + conversion, no candidate / settlement      r05_ab_rgba16f_ceiling.txt
  BT709_LAB_F16_NO_CAND_GATHER / _NO_T_GATHER  RGBA16F kernel, WRONG OUTPUT: one of its two LDS gathers removed r05_ab_rgba16f_packed.txt
  BT709_LAB_ENC_NO_ARITH  encoder, WRONG OUTPUT: loads + stores only                                         r05_ab_encode_ceiling.txt
  BT709_LAB_UNC_NO_ARITH  +unconvert: kernel, WRONG OUTPUT: loads + stores only                              r05_ab_unconvert_ceiling.txt
  BT709_LAB_HALF_ENCODE_B32  persistent 2:1 kernel, WRONG OUTPUT: 4-byte encode entries, twice the copies        r05_ab_half_encode_b32.txt
  BT709_LAB_SCALED_QUARTER_FEWER_TAPS  any-ratio kernel, WRONG OUTPUT: a quarter of the tap decodes deleted   r05_ab_scaled_r15_bound.txt
  BT709_LAB_SCALED_HALF_FEWER_TAPS     any-ratio kernel, WRONG OUTPUT: the right tap a copy of the left one (half the decodes)  r06_ab_scaled_share.txt
  BT709_LAB_SCALED_PAIR_DPP            the same with the copy taken from the next lane by a DPP move (lane-pair exchange)      r06_ab_scaled_share.txt
  BT709_LAB_SCALED_ONCE_LDS            wave-decodes-once form exchanging through a wave-private LDS tile (same bytes out)      r06_ab_scaled_share.txt
  BT709_LAB_SCALED_NO_FETCH / _NO_DECODE / _NO_ENCODE / _NO_STORE  any-ratio kernel, WRONG OUTPUT: one part deleted each      r06_ab_scaled_parts.txt
  BT709_LAB_I420_PAIRED                planar 1:1 fast kernels: ONE chroma dword per quad, shared by lane pairs over DPP, instead of two 2-byte loads (same bytes out; frames without W % 8 == 0, 4-byte aligned chroma planes and V less than 4 GiB behind U take the general kernel)   r12_planar.txt
  BT709_LAB_ENC_I420_PAIRED            planar encode, fast kernels: lane pairs exchange the packed chroma word over DPP; the even lane stores ONE U dword, the odd lane ONE V dword, instead of two 2-byte stores a lane (same bytes out for W % 8 == 0 and 4-byte aligned chroma planes ONLY: no shim gate sends the other frames elsewhere -- bench sizes only)   r13_encode_planar.txt
  BT709_LAB_ENC_I420_WIDE              planar encode, fast colour kernel: a lane owns 8x2 pixels (two quads): four 16-byte loads, two 8-byte luma stores, one U and one V dword a row pair; half the lanes a row (same bytes out for W % 8 == 0, 8-byte aligned luma and 4-byte aligned chroma ONLY -- bench sizes only)   r13_encode_planar.txt
  BT709_LAB_STEP32                     frame_planes, WRONG ADDRESSES: every step of a uniform batch cut to its low 32 bits, zero-extended.  Shows that tests/test_batch_spacing_gpu.py bites: run ONLY -k "far and not descending" against it (frames 2^32 + d apart: the cut step lands on the alias windows inside the test's own slabs); with a NEGATIVE step the cut address leaves the allocation
  BT709_LAB_ROW32                      TileIn::load, decode_nv12_half<wide>'s target row, encode_bgra's chroma row, WRONG ADDRESSES: row x pitch cut to its low 32 bits, zero-extended.  Shows that tests/test_row_pitch_gpu.py bites: run ONLY the past-2^32 ids (-k "past and 32": `^` is no character of a -k expression; the cut offset lands on the alias windows inside the test's own slabs) and the past-2^31 ids (-k "past and 31"; must pass: zero-extension is right below 2^32).  There is no sign-extending twin: under past-2^32 it would leave the allocation
  BT709_LAB_HUNT_TRACE                 bt709hip_ring_create prints where its hunt's wall-clock time went (stderr; same ring)   r06_hunt_default.txt
"""
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAB_SRC = os.path.join(ROOT, "tools", "bin", "lab_src")

# (file, product text, lab text).  Every product text must occur exactly once.
GATES = [
    ("bt709_tile.h",  # TileIn::load: the 1:1 kernel and the WIDE branch of the short-lived 2:1 kernel
     """      ya[j] = load32<NT>(y0 + 4 * q);
      yb[j] = load32<NT>(y1 + 4 * q);
      if constexpr (PLANAR) {
""",
     """#if defined(BT709_LAB_NO_LOADS)  // with BT709_LAB_NO_ARITH: the launch's stores alone (NV12 launches only: the planar branch below still loads)
      ya[j] = q * 3u, yb[j] = q * 5u, cw[j] = q * 7u + rp;
      if constexpr (PLANAR) {
#else
      ya[j] = load32<NT>(y0 + 4 * q);
      yb[j] = load32<NT>(y1 + 4 * q);
      if constexpr (PLANAR) {
#endif
"""),
    ("bt709_tile.h",
     """        cw[j] = load32<NT>(cc + 4 * q);
""",
     """#if !defined(BT709_LAB_NO_LOADS)
        cw[j] = load32<NT>(cc + 4 * q);
#endif
"""),
    ("bt709_decode_body.h",
     """  if (!QUANT) {  // the sRGB mode needs no table (decode_quad)
    stage_table(lds_raw, p.table_unit, p.table_unit_bytes);  // after the tile's loads are in flight
    __syncthreads();
  }
""",
     """#if !defined(BT709_LAB_NO_TABLE)  // with BT709_LAB_NO_ARITH: without the per-workgroup table staging and its barrier too
  if (!QUANT) {
    stage_table(lds_raw, p.table_unit, p.table_unit_bytes);
    __syncthreads();
  }
#endif
"""),
    ("bt709_decode_body.h",
     """    decode_quad<HAS_ALPHA, QUANT, LOGIDX>(ul, in.ya[u], in.yb[u], in.cw[u], HAS_ALPHA ? in.aa[u] : 0u, HAS_ALPHA ? in.ab[u] : 0u, p.alpha_word, top, bot);
    if (q < quads && rp_raw < row_pairs) {
""",
     """#if defined(BT709_LAB_NO_ARITH)  // WRONG OUTPUT: the launch's loads and stores with (almost) no arithmetic
    top = u32x4{in.ya[u], in.yb[u], in.cw[u], in.ya[u] ^ in.cw[u]};
    bot = u32x4{in.yb[u], in.cw[u], in.ya[u], in.yb[u] ^ in.cw[u]};
#else
    decode_quad<HAS_ALPHA, QUANT, LOGIDX>(ul, in.ya[u], in.yb[u], in.cw[u], HAS_ALPHA ? in.aa[u] : 0u, HAS_ALPHA ? in.ab[u] : 0u, p.alpha_word, top, bot);
#endif
#if defined(BT709_LAB_NO_STORES)  // with BT709_LAB_NO_ARITH: the loads alone (a store about once in 2^32 quads keeps them alive)
    if (q < quads && rp_raw < row_pairs && (top.w ^ bot.w) == 0x9e3779b9u) {
#else
    if (q < quads && rp_raw < row_pairs) {
#endif
"""),
    ("bt709_device.h",
     """  return __builtin_fmaf(v, kInv255, -off * kInv255);
""",
     """#if defined(BT709_NO_FMA_CENTRE)  // the two-instruction form
  return __fmul_rn(__fadd_rn(v, -off), kInv255);
#else
  return __builtin_fmaf(v, kInv255, -off * kInv255);
#endif
"""),
    ("bt709_device.h",
     """__device__ __forceinline__ void magic_index12(const float *x, uint32_t *t, float magic) {
#pragma unroll
  for (int i = 0; i < 12; ++i) t[i] = __float_as_uint(__fadd_rn(x[i], magic));
}

__device__ __forceinline__ void magic_index4(const float *x, uint32_t *t, float magic) {
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = __float_as_uint(__fadd_rn(x[i], magic));
}
""",
     """#if defined(BT709_INDEX_RTZ)  // round 1: floor(x N); the adds of a batch sit between two writes of MODE.fp_round
__device__ __forceinline__ void magic_index12(const float *x, uint32_t *t, float magic) {
  asm("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\\n\\t"
      "v_add_f32 %0, %24, %12\\n\\tv_add_f32 %1, %24, %13\\n\\tv_add_f32 %2, %24, %14\\n\\tv_add_f32 %3, %24, %15\\n\\t"
      "v_add_f32 %4, %24, %16\\n\\tv_add_f32 %5, %24, %17\\n\\tv_add_f32 %6, %24, %18\\n\\tv_add_f32 %7, %24, %19\\n\\t"
      "v_add_f32 %8, %24, %20\\n\\tv_add_f32 %9, %24, %21\\n\\tv_add_f32 %10, %24, %22\\n\\tv_add_f32 %11, %24, %23\\n\\t"
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0"
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6]), "=&v"(t[7]),
        "=&v"(t[8]), "=&v"(t[9]), "=&v"(t[10]), "=&v"(t[11])
      : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "v"(x[8]), "v"(x[9]),
        "v"(x[10]), "v"(x[11]), "s"(magic));
}

__device__ __forceinline__ void magic_index4(const float *x, uint32_t *t, float magic) {
  asm("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\\n\\t"
      "v_add_f32 %0, %8, %4\\n\\tv_add_f32 %1, %8, %5\\n\\tv_add_f32 %2, %8, %6\\n\\tv_add_f32 %3, %8, %7\\n\\t"
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0"
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])
      : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "s"(magic));
}
#else
__device__ __forceinline__ void magic_index12(const float *x, uint32_t *t, float magic) {
#pragma unroll
  for (int i = 0; i < 12; ++i) t[i] = __float_as_uint(__fadd_rn(x[i], magic));
}

__device__ __forceinline__ void magic_index4(const float *x, uint32_t *t, float magic) {
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = __float_as_uint(__fadd_rn(x[i], magic));
}
#endif
"""),
    ("transfer_tables.cpp",
     """  volatile float s = x + magic;  // binary32 add, round to nearest even (volatile: no excess precision, no folding)
""",
     """#if defined(BT709_INDEX_RTZ)
  const int mode = std::fegetround();
  std::fesetround(FE_TOWARDZERO);
  volatile float s = x + magic;
  std::fesetround(mode);
#else
  volatile float s = x + magic;
#endif
"""),
    ("bt709_rescale.hip",
     """  const uint32_t t = __float_as_uint(__builtin_fmaf(s, r.sum_to_xs, 8388608.0f));
""",
     """#if defined(BT709_UNIFORM_INDEX_TWO_STEP)  // round 2's first form: multiply, then add
  const uint32_t t = __float_as_uint(__fadd_rn(__fmul_rn(s, r.sum_to_xs), 8388608.0f));
#else
  const uint32_t t = __float_as_uint(__builtin_fmaf(s, r.sum_to_xs, 8388608.0f));
#endif
"""),
    ("transfer_tables.cpp",
     """  volatile float t = std::fmaf(v, n, 8388608.0f);  // one rounding of v n + 2^23, as the kernel's v_fma_f32
""",
     """#if defined(BT709_UNIFORM_INDEX_TWO_STEP)
  volatile float xs = v * n;
  volatile float t = xs + 8388608.0f;
#else
  volatile float t = std::fmaf(v, n, 8388608.0f);
#endif
"""),
    ("bt709_rescale.hip",
     """  magic_index12(x, t, r.magic);
#pragma unroll
  for (int h = 0; h < 12 / kLinBatch; ++h) {""",
     """#if defined(BT709_LAB_BOUND_SHARED_INDEX)
  // WRONG OUTPUT: G and B reuse R's four bucket indices -- what the launch would take if the index of a block's 12
  // evaluations cost 4 adds instead of 12 (the ceiling of any "index from the luma term alone" form)
  magic_index4(x, t, r.magic);
#pragma unroll
  for (int i = 4; i < 12; ++i) t[i] = t[i & 3];
#else
  magic_index12(x, t, r.magic);
#endif
#pragma unroll
  for (int h = 0; h < 12 / kLinBatch; ++h) {"""),
    ("bt709_rescale.hip",
     """  if (UNIFORM_ENCODE) return pack_bgra(encode_byte_uniform(r, sr), encode_byte_uniform(r, sg), encode_byte_uniform(r, sb), alpha_word);
""",
     """#if defined(BT709_LAB_BOUND_ONE_ENCODE)
  // WRONG OUTPUT: one encode-side lookup instead of three (sg, sb still formed and consumed)
  if (UNIFORM_ENCODE) {
    const uint32_t e = encode_byte_uniform(r, sr);
    return pack_bgra(e, e + (sg > sr ? 1u : 0u), e + (sb > sr ? 1u : 0u), alpha_word);
  }
#endif
  if (UNIFORM_ENCODE) return pack_bgra(encode_byte_uniform(r, sr), encode_byte_uniform(r, sg), encode_byte_uniform(r, sb), alpha_word);
"""),
    ("bt709_rescale.hip",
     """constexpr bool kRepUniformEncode = true;
""",
     """#if defined(BT709_REP_SPLIT_ENCODE)
constexpr bool kRepUniformEncode = false;
#else
constexpr bool kRepUniformEncode = true;
#endif
"""),
    ("bt709_rescale.hip",
     """  DecodeParams p = p_in;
  const uint64_t kRepLdsBytes =""",
     """  DecodeParams p = p_in;
#if defined(BT709_LAB_HALF_TABLE)  // WRONG OUTPUT: half as many (coarser) decode-side buckets = the LDS footprint of 8-byte entries
  p.unit_magic = p.unit_magic * 2.0f;
  p.table_linear_bytes = (p.table_linear_bytes / 2 + 31u) & ~15u;
#endif
  const uint64_t kRepLdsBytes ="""),
    # ---- round 5: traffic-pattern ceilings of the kernels that claim to be memory-bound below 0.75 (Missing 4)
    ("bt709_rgba16f.hip",
     """    stage_half_tables(lds_raw, hp.table, hp.cand_offset, hp.table_bytes);
""",
     """#if !defined(BT709_LAB_F16_NO_TABLE)  // with BT709_LAB_F16_NO_ARITH / _CVT_ONLY: without the per-workgroup table staging too
    stage_half_tables(lds_raw, hp.table, hp.cand_offset, hp.table_bytes);
#endif
"""),
    ("bt709_rgba16f.hip",
     """  if (!HAS_TABLE) {  // no curve: the conversion alone
""",
     """#if defined(BT709_LAB_F16_CVT_ONLY)  // WRONG OUTPUT: the conversion alone, no candidate, no settlement (matrix + v_cvt_pk_f16_f32)
  if (true) {
#else
  if (!HAS_TABLE) {  // no curve: the conversion alone
#endif
"""),
    ("bt709_rgba16f.hip",
     """      half_texels<HAS_TABLE>(t, x, alpha, w);
""",
     """#if defined(BT709_LAB_F16_NO_ARITH)  // WRONG OUTPUT: the launch's loads and stores with (almost) no arithmetic
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = __float_as_uint(x[i]);
#else
      half_texels<HAS_TABLE>(t, x, alpha, w);
#endif
"""),
    ("bt709_rgba16f.hip",
     """    const f32x2 u = f32x2{x[2 * i], x[2 * i + 1]} * t.index_scale;  // binary32 products (v_pk_mul_f32; -ffp-contract=off)
""",
     """#if defined(BT709_LAB_F16_NO_INDEX_SCALE)  // WRONG OUTPUT: what the v_pk_mul_f32 that puts the split point on a bucket boundary costs
    const f32x2 u = f32x2{x[2 * i], x[2 * i + 1]};
#else
    const f32x2 u = f32x2{x[2 * i], x[2 * i + 1]} * t.index_scale;  // binary32 products (v_pk_mul_f32; -ffp-contract=off)
#endif
"""),
    # CORRECT output: the table staged by LDS DMA (global_load_lds_dwordx4: L2 -> LDS without the trip through VGPRs and ds_write)
    ("bt709_half_lookup.h",
     """  stage_batched<5>(reinterpret_cast<u32x4 *>(lds), n, tid, nthreads, [&](uint32_t i) { return s[i]; },
""",
     """#if defined(BT709_LAB_F16_DMA_STAGING)
  {
    const uint32_t cand16 = n_thresholds + gap, total16 = cand16 + (n - n_thresholds);  // the LDS image in 16-byte words
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63u, waves = nthreads >> 6;
    for (uint32_t c = wave; c * 64u < total16; c += waves) {  // a wave fills 1 KiB of LDS per instruction
      const uint32_t L = c * 64u + lane;
      if (L < n_thresholds || (L >= cand16 && L < total16))
        __builtin_amdgcn_global_load_lds(s + (L < n_thresholds ? L : L - gap), (__attribute__((address_space(3))) void *)(lds + c * 1024u), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return;
  }
#endif
  stage_batched<5>(reinterpret_cast<u32x4 *>(lds), n, tid, nthreads, [&](uint32_t i) { return s[i]; },
"""),
    # the two gathers of the packed-pair form, one at a time (WRONG OUTPUT; the VALU work around them stays)
    ("bt709_rgba16f.hip",
     """    c[2 * i] = *reinterpret_cast<LdsPairPtr>((pk & 0xfff8u) + kCandBias);  // {intercept, slope}
    c[2 * i + 1] = *reinterpret_cast<LdsPairPtr>(((pk >> 16) & 0xfff8u) + kCandBias);
""",
     """#if defined(BT709_LAB_F16_NO_CAND_GATHER)
    c[2 * i] = u32x2{(pk & 0xfff8u) + kCandBias, 0x3f000000u};
    c[2 * i + 1] = u32x2{((pk >> 16) & 0xfff8u) + kCandBias, 0x3f000000u};
#else
    c[2 * i] = *reinterpret_cast<LdsPairPtr>((pk & 0xfff8u) + kCandBias);  // {intercept, slope}
    c[2 * i + 1] = *reinterpret_cast<LdsPairPtr>(((pk >> 16) & 0xfff8u) + kCandBias);
#endif
"""),
    ("bt709_rgba16f.hip",
     """    e[3 * px] = *reinterpret_cast<LdsFloatPtr>(((drg & 0xffffu) << 2) + 4u);
    e[3 * px + 1] = *reinterpret_cast<LdsFloatPtr>(((drg >> 16) << 2) + 4u);
    e[3 * px + 2] = *reinterpret_cast<LdsFloatPtr>((db << 2) + 4u);
""",
     """#if defined(BT709_LAB_F16_NO_T_GATHER)
    e[3 * px] = __uint_as_float(((drg & 0xffffu) << 2) + 4u);
    e[3 * px + 1] = __uint_as_float(((drg >> 16) << 2) + 4u);
    e[3 * px + 2] = __uint_as_float((db << 2) + 4u);
#else
    e[3 * px] = *reinterpret_cast<LdsFloatPtr>(((drg & 0xffffu) << 2) + 4u);
    e[3 * px + 1] = *reinterpret_cast<LdsFloatPtr>(((drg >> 16) << 2) + 4u);
    e[3 * px + 2] = *reinterpret_cast<LdsFloatPtr>((db << 2) + 4u);
#endif
"""),
    # ---- round 5: what 4-byte encode entries (24-bit edge | byte) in TWICE the copies would buy the persistent 2:1 kernel
    # (VERDICT r4, item 5).  WRONG OUTPUT in general (the edge loses its low 8 bits and no proof covers that); VALU-neutral: the
    # byte rides in the SDWA operand of the add-with-carry.  The encode table stays one 26 KiB image in LDS, now holding two
    # interleaved copies of 4-byte entries; ds_read_b32 instead of ds_read_b64.
    ("bt709_rescale.hip",
     """    stage_batched(d2, n2, tid, nthreads, [&](uint32_t i) {
      u32x2 e = src2[i >> r2];
      e.x = __float_as_uint(__fmul_rn(__uint_as_float(e.x), to_sum));
      return e;
    });
""",
     """#if defined(BT709_LAB_HALF_ENCODE_B32)
    stage_batched(reinterpret_cast<uint32_t *>(d2), n2 * 2u, tid, nthreads, [&](uint32_t i) {
      const u32x2 e = src2[i >> (r2 + 1u)];
      return (__float_as_uint(__fmul_rn(__uint_as_float(e.x), to_sum)) & 0xffffff00u) | (e.y & 0xffu);
    });
#else
    stage_batched(d2, n2, tid, nthreads, [&](uint32_t i) {
      u32x2 e = src2[i >> r2];
      e.x = __float_as_uint(__fmul_rn(__uint_as_float(e.x), to_sum));
      return e;
    });
#endif
"""),
    ("bt709_rescale.hip",
     """  r.enc_off = base + dec_bytes + (tid & ((1u << r2) - 1u)) * 8u;
""",
     """#if defined(BT709_LAB_HALF_ENCODE_B32)
  r.enc_off = base + dec_bytes + (tid & ((2u << r2) - 1u)) * 4u;
#else
  r.enc_off = base + dec_bytes + (tid & ((1u << r2) - 1u)) * 8u;
#endif
"""),
    ("bt709_rescale.hip",
     """    q.e[k] = *reinterpret_cast<LdsPairPtr>((t << r.enc_shift) + r.enc_u_off);
""",
     """#if defined(BT709_LAB_HALF_ENCODE_B32)
    q.e[k].x = *reinterpret_cast<__attribute__((address_space(3))) const uint32_t *>((t << r.enc_shift) + r.enc_u_off);
    q.e[k].y = 0u;
#else
    q.e[k] = *reinterpret_cast<LdsPairPtr>((t << r.enc_shift) + r.enc_u_off);
#endif
"""),
    ("bt709_rescale.hip",
     """  for (int k = 0; k < 3; ++k) b[k] = q.e[k].y + (q.s[k] >= __uint_as_float(q.e[k].x) ? 1u : 0u);
""",
     """#if defined(BT709_LAB_HALF_ENCODE_B32)
  for (int k = 0; k < 3; ++k)
    asm("v_cmp_ge_f32 vcc, %1, %2\\n\\tv_addc_co_u32_sdwa %0, vcc, %3, %2, vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0"
        : "=v"(b[k]) : "v"(q.s[k]), "v"(q.e[k].x), "v"(q.e[k].y) : "vcc");
#else
  for (int k = 0; k < 3; ++k) b[k] = q.e[k].y + (q.s[k] >= __uint_as_float(q.e[k].x) ? 1u : 0u);
#endif
"""),
    # ---- round 5: what a ratio-1.5 specialisation of decode_nv12_scaled could save AT MOST: a lane owning a
    # 3x3 source block -> 2x2 outputs decodes 27 taps per 4 output pixels instead of 36, i.e. a quarter of the tap decodes
    # (matrix + 3 lookups each) go.  The stub deletes exactly that share outright -- on every odd source row the second tap
    # reuses the first tap's values, no pixel_rgb, no lookups for it -- and keeps everything else: an upper bound on the gain.
    ("bt709_rescale.hip",
     """    float x[6];  // R, G, B of tap 0; R, G, B of tap 1
    pixel_rgb(byte_of(fr.yy, 0), ch0, x[0], x[1], x[2]);
    pixel_rgb(byte_of(fr.yy, 1), ch1, x[3], x[4], x[5]);
    RowLin<N> rl;
    light.template two<N>(x, fr.aa, rl);
    return rl;
""",
     """    float x[6];
#if defined(BT709_LAB_SCALED_HALF_FEWER_TAPS) || defined(BT709_LAB_SCALED_PAIR_DPP) || defined(BT709_LAB_SCALED_QUARTER_FEWER_TAPS)
    float lin[6];
    const RescaleLookup &r = light.r;  // the stubs are written against the 8-bit intermediate's lookup
#endif
#if defined(BT709_LAB_SCALED_HALF_FEWER_TAPS) || defined(BT709_LAB_SCALED_PAIR_DPP)  // WRONG OUTPUT: tap 0 decoded, tap 1 a copy of it / of the next lane's
    pixel_rgb(byte_of(fr.yy, 0), ch0, x[0], x[1], x[2]);
    {
      uint32_t t3[4];
      const float xp[4] = {x[0], x[1], x[2], 0.0f};
      magic_index4(xp, t3, r.magic);
      u32x4 e3[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) e3[i] = *reinterpret_cast<LdsQuadPtr>((t3[i] << r.dec_shift) + r.dec_off);
      asm volatile("" : "+v"(e3[0]), "+v"(e3[1]), "+v"(e3[2]));
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        lin[i] = __builtin_amdgcn_fmed3f(__uint_as_float(e3[i].y), __uint_as_float(e3[i].z), __fadd_rn(x[i], -__uint_as_float(e3[i].x)));
#if defined(BT709_LAB_SCALED_PAIR_DPP)  // the lane-pair exchange as a DPP move (row_shl:1): what sharing between lane l and l + 1 costs
        lin[3 + i] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, lin[i]), 0x101, 0xf, 0xf, false));
#else
        lin[3 + i] = lin[i];
#endif
      }
    }
#elif defined(BT709_LAB_SCALED_QUARTER_FEWER_TAPS)  // WRONG OUTPUT
    pixel_rgb(byte_of(fr.yy, 0), ch0, x[0], x[1], x[2]);
    if (srow & 1) {  // wave-uniform
      uint32_t t3[4];
      const float xp[4] = {x[0], x[1], x[2], 0.0f};
      magic_index4(xp, t3, r.magic);
      u32x4 e3[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) e3[i] = *reinterpret_cast<LdsQuadPtr>((t3[i] << r.dec_shift) + r.dec_off);
      asm volatile("" : "+v"(e3[0]), "+v"(e3[1]), "+v"(e3[2]));
#pragma unroll
      for (int i = 0; i < 3; ++i)
        lin[i] = lin[3 + i] = __builtin_amdgcn_fmed3f(__uint_as_float(e3[i].y), __uint_as_float(e3[i].z), __fadd_rn(x[i], -__uint_as_float(e3[i].x)));
    } else {
      pixel_rgb(byte_of(fr.yy, 1), ch1, x[3], x[4], x[5]);
      linearise6(r, x, lin);
    }
#else
    pixel_rgb(byte_of(fr.yy, 0), ch0, x[0], x[1], x[2]);
    pixel_rgb(byte_of(fr.yy, 1), ch1, x[3], x[4], x[5]);
#endif
    RowLin<N> rl;
#if defined(BT709_LAB_SCALED_HALF_FEWER_TAPS) || defined(BT709_LAB_SCALED_PAIR_DPP) || defined(BT709_LAB_SCALED_QUARTER_FEWER_TAPS)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int k = 0; k < 3; ++k) rl.v[t][k] = lin[3 * t + k];
      if (HAS_ALPHA) rl.v[t][N - 1] = alpha_norm_arith(byte_of(fr.aa, t));
    }
#else
    light.template two<N>(x, fr.aa, rl);
#endif
    return rl;
"""),
    # round 6: where the placement hunt's wall-clock time goes (stderr, one line per ring): allocation, free, hipMemGetInfo, warm-up launches, probes
    ("bt709_ring.cpp",
     """  void *take(size_t bytes) {
    void *p = nullptr;
    if (bt709hip_malloc(ctx, bytes, &p) != BT709HIP_OK || p == nullptr) return nullptr;
""",
     """  void *take(size_t bytes) {
    void *p = nullptr;
#if defined(BT709_LAB_HUNT_TRACE)
    const double t0 = now_s();
    const int rc_ = bt709hip_malloc(ctx, bytes, &p);
    lab_trace()[0] += now_s() - t0;
    if (rc_ != BT709HIP_OK || p == nullptr) return nullptr;
#else
    if (bt709hip_malloc(ctx, bytes, &p) != BT709HIP_OK || p == nullptr) return nullptr;
#endif
"""),
    ("bt709_ring.cpp",
     """    if (p == nullptr) return;
    (void)bt709hip_free(ctx, p);
    held -= bytes;
""",
     """    if (p == nullptr) return;
#if defined(BT709_LAB_HUNT_TRACE)
    const double t0 = now_s();
    (void)bt709hip_free(ctx, p);
    lab_trace()[1] += now_s() - t0;
#else
    (void)bt709hip_free(ctx, p);
#endif
    held -= bytes;
"""),
    ("bt709_ring.cpp",
     """    size_t free_b = 0;
    return bt709hip_mem_info(ctx, &free_b, nullptr) == BT709HIP_OK && free_b >= bytes + kReserveBytes;
""",
     """    size_t free_b = 0;
#if defined(BT709_LAB_HUNT_TRACE)
    const double t0 = now_s();
    const bool ok_ = bt709hip_mem_info(ctx, &free_b, nullptr) == BT709HIP_OK && free_b >= bytes + kReserveBytes;
    lab_trace()[2] += now_s() - t0;
    return ok_;
#else
    return bt709hip_mem_info(ctx, &free_b, nullptr) == BT709HIP_OK && free_b >= bytes + kReserveBytes;
#endif
"""),
    ("bt709_ring.cpp",
     """double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
""",
     """double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
#if defined(BT709_LAB_HUNT_TRACE)
double *lab_trace() {  // seconds: malloc, free, mem_info, warm-up, probe
  static double t[5] = {0, 0, 0, 0, 0};
  return t;
}
#endif
"""),
    ("bt709_ring.cpp",
     """    bind_slabs(r, in, out);
    const double t_end = now_s() + warm_s;
    do {
      if ((rc = launch(r, 0, r->frames, nullptr, 1)) != BT709HIP_OK) return 0.0f;
    } while (now_s() < t_end);
""",
     """    bind_slabs(r, in, out);
#if defined(BT709_LAB_HUNT_TRACE)
    const double lab_t0 = now_s();
    struct LabProbe { double t0; ~LabProbe() { lab_trace()[4] += now_s() - t0; } };
#endif
    const double t_end = now_s() + warm_s;
    do {
      if ((rc = launch(r, 0, r->frames, nullptr, 1)) != BT709HIP_OK) return 0.0f;
    } while (now_s() < t_end);
#if defined(BT709_LAB_HUNT_TRACE)
    lab_trace()[3] += now_s() - lab_t0;
    LabProbe lab_probe{now_s()};
#endif
"""),
    ("bt709_ring.cpp",
     """  if (pl.tries > 1) pl.hunt_ms = static_cast<float>((now_s() - t_start) * 1e3);
""",
     """  if (pl.tries > 1) pl.hunt_ms = static_cast<float>((now_s() - t_start) * 1e3);
#if defined(BT709_LAB_HUNT_TRACE)
  if (pl.tries > 1) {
    double *t = lab_trace();
    std::fprintf(stderr, "hunt trace: total %.0f ms = malloc %.0f + free %.0f + mem_info %.0f + warm-up %.0f + probes %.0f + rest %.0f (candidates %d + %d)\\n", pl.hunt_ms,
                 t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, t[3] * 1e3, t[4] * 1e3, pl.hunt_ms - (t[0] + t[1] + t[2] + t[3] + t[4]) * 1e3, pl.in_candidates, pl.out_candidates);
    for (int k = 0; k < 5; ++k) t[k] = 0.0;
  }
#endif
"""),
    # round 6: what bounds the any-ratio kernel at ratio >= 1 -- stubs that delete ONE part each (WRONG OUTPUT)
    ("bt709_rescale.hip",
     """  auto fetch_row = [&](int srow) {
    Fetched1 v = {};
""",
     """  auto fetch_row = [&](int srow) {
    Fetched1 v = {};
#if defined(BT709_LAB_SCALED_NO_FETCH)  // no vector memory loads: the source bytes are made up from registers
    v.y[0] = (ybase + static_cast<uint32_t>(srow)) * 0x9e3779b9u, v.y[1] = v.y[0] >> 3, v.c[0] = v.y[0] ^ 0x55aa55aau, v.c[1] = ~v.y[0];
    v.c[2] = v.y[1], v.c[3] = v.c[0], v.a[0] = v.y[0], v.a[1] = v.y[1];
    asm volatile("" : "+v"(v.y[0]), "+v"(v.y[1]), "+v"(v.c[0]), "+v"(v.c[1]));
    if (true) return v;
#endif
"""),
    ("bt709_rescale.hip",
     """  auto decode_row = [&](const Fetched1 &raw, int srow) {
    if (TAPS == TAPS_ONCE) {""",
     """  auto decode_row = [&](const Fetched1 &raw, int srow) {
#if defined(BT709_LAB_SCALED_NO_DECODE)  // no matrix, no decode-side lookups: six floats straight from the fetched bytes
    {
      RowLin<N> rl = {};
      const float tiny = __uint_as_float(0x2b800000u);
#pragma unroll
      for (int k = 0; k < 6; ++k) rl.v[k / 3][k % 3] = __fmul_rn(byte_of(k < 4 ? raw.y[0] : raw.c[0], k & 3), tiny);
      (void)srow;
      if (true) return rl;
    }
#endif
    if (TAPS == TAPS_ONCE) {"""),
    ("bt709_rescale.hip",
     """    const uint32_t R = light.encode(acc[0]);
    const uint32_t G = light.encode(acc[1]);
    const uint32_t B = light.encode(acc[2]);
""",
     """#if defined(BT709_LAB_SCALED_NO_ENCODE)  // no encode-side lookups: a byte cut out of each float
    const uint32_t R = (__float_as_uint(acc[0]) >> 15) & 0xffu, G = (__float_as_uint(acc[1]) >> 15) & 0xffu, B = (__float_as_uint(acc[2]) >> 15) & 0xffu;
#else
    const uint32_t R = light.encode(acc[0]);
    const uint32_t G = light.encode(acc[1]);
    const uint32_t B = light.encode(acc[2]);
#endif
"""),
    ("bt709_rescale.hip",
     """    if (!BY_WAVE || live)
      __builtin_amdgcn_raw_buffer_store_b32(pack_bgra(R, G, B, aw), ro, ox * 4u, oy * p.out_stride, kScaledStoreAux);
""",
     """#if defined(BT709_LAB_SCALED_NO_STORE)  // (almost) no stores: about one pixel in 2^32
    if ((!BY_WAVE || live) && pack_bgra(R, G, B, aw) + oy == 0x9e3779b9u)
#else
    if (!BY_WAVE || live)
#endif
#if defined(BT709_LAB_SCALED_STORE_ONE_LINE)  // every store instruction is issued, but all of a wave's rows go to ONE row of the frame: the lines stay in L2
      __builtin_amdgcn_raw_buffer_store_b32(pack_bgra(R, G, B, aw), ro, ox * 4u, (oy & 1u) * p.out_stride, kScaledStoreAux);
#else
      __builtin_amdgcn_raw_buffer_store_b32(pack_bgra(R, G, B, aw), ro, ox * 4u, oy * p.out_stride, kScaledStoreAux);
#endif
"""),
    # round 6: consecutive one-frame launches on ONE stream without the in-order barrier between them (hipExtAnyOrderLaunch; the header says "not supported on GFX9xx")
    # (the launch table's one launch line: the experiment's kernel is the row "quads<nt>", decode_quads<layout, false, true, false>)
    ("bt709_kernels.hip",
     """    hipLaunchKernelGGL(k.fn[layout], grid, block, lds, stream, p);
    return k.name[layout];
""",
     """#if defined(BT709_LAB_ANY_ORDER)
    if (k.fn[0] == decode_quads<kChromaNV12, false, true, false>) {
      hipExtLaunchKernelGGL(k.fn[layout], grid, block, lds, stream, nullptr, nullptr, hipExtAnyOrderLaunch, p);
    } else {
      hipLaunchKernelGGL(k.fn[layout], grid, block, lds, stream, p);
    }
#else
    hipLaunchKernelGGL(k.fn[layout], grid, block, lds, stream, p);
#endif
    return k.name[layout];
"""),
    ("bt709_kernels.hip",
     """#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
""",
     """#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>
#include <cstring>
"""),
    # round 6: the persistent 2:1 kernel (BASELINE config 4) with its loads or its stores deleted (WRONG OUTPUT): is its memory side anywhere near mattering?
    ("bt709_rescale.hip",
     """  in.ya = load32<NT>(y0 + 4 * q);
  in.yb = load32<NT>(y0 + p.y_stride + 4 * q);
  in.cw = load32<NT>(cc + 4 * q);
  in.aa = in.ab = 0;
""",
     """#if defined(BT709_LAB_HALF_NO_FETCH)
  in.ya = q * 0x9e3779b9u + c.rp, in.yb = in.ya >> 3, in.cw = ~in.ya;
  asm volatile("" : "+v"(in.ya), "+v"(in.yb), "+v"(in.cw));
  (void)y0, (void)cc;
#else
  in.ya = load32<NT>(y0 + 4 * q);
  in.yb = load32<NT>(y0 + p.y_stride + 4 * q);
  in.cw = load32<NT>(cc + 4 * q);
#endif
  in.aa = in.ab = 0;
"""),
    ("bt709_rescale.hip",
     """      const uint32_t q = min(c.tx * blockDim.x + threadIdx.x, quads - 1);
      store8<NT>(o + 8 * q, v);
""",
     """      const uint32_t q = min(c.tx * blockDim.x + threadIdx.x, quads - 1);
#if defined(BT709_LAB_HALF_NO_STORE)
      if (v.x + v.y == 0x9e3779b9u)
#endif
      store8<NT>(o + 8 * q, v);
"""),
    # round 6: which XCD takes which band of the launch's frames (rotation / reversal of the band index): does a placement's level follow it?
    # (banded_work: every kernel that uses the map, and both of its banded forms)
    ("bt709_tile.h",
     """  const uint32_t band = blockIdx.x & 7u;
""",
     """#if defined(BT709_LAB_BAND_ROT)
  const uint32_t band = (((blockIdx.x & 7u) + BT709_LAB_BAND_ROT) & 7u) ^ BT709_LAB_BAND_XOR;
#else
  const uint32_t band = blockIdx.x & 7u;
#endif
"""),
    # round 6: the wave-decodes-once form's exchange through a wave-private LDS tile instead of ds_bpermute (same bytes out)
    ("bt709_rescale.hip",
     """      RowLin<N> rl;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int k = 0; k < N; ++k)
          rl.v[t][k] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(static_cast<int>(tap_lane[t]), __builtin_bit_cast(int, own[k])));
      }
      return rl;
""",
     """      RowLin<N> rl;
#if defined(BT709_LAB_SCALED_ONCE_LDS)  // the decode-once TILE: own pixel written to LDS (16 bytes per lane, behind the tables), taps read back
      {
        typedef __attribute__((address_space(3))) u32x4 *LdsQuadW;
        const uint32_t tile = p.lab_tile_off + (threadIdx.x & ~63u) * 16u;  // this wave's 1 KiB
        if (!HAS_ALPHA) own[3] = 0.0f;
        u32x4 w = {__float_as_uint(own[0]), __float_as_uint(own[1]), __float_as_uint(own[2]), __float_as_uint(own[3])};
        *reinterpret_cast<LdsQuadW>(tile + lane * 16u) = w;
        asm volatile("" ::: "memory");
        const u32x4 t0 = *reinterpret_cast<LdsQuadPtr>(tile + tap_lane[0] * 4u), t1 = *reinterpret_cast<LdsQuadPtr>(tile + tap_lane[1] * 4u);
        asm volatile("" ::: "memory");
        rl.v[0][0] = __uint_as_float(t0.x), rl.v[0][1] = __uint_as_float(t0.y), rl.v[0][2] = __uint_as_float(t0.z);
        rl.v[1][0] = __uint_as_float(t1.x), rl.v[1][1] = __uint_as_float(t1.y), rl.v[1][2] = __uint_as_float(t1.z);
        if (HAS_ALPHA) rl.v[0][N - 1] = __uint_as_float(t0.w), rl.v[1][N - 1] = __uint_as_float(t1.w);
      }
#else
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int k = 0; k < N; ++k)
          rl.v[t][k] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(static_cast<int>(tap_lane[t]), __builtin_bit_cast(int, own[k])));
      }
#endif
      return rl;
"""),
    ("bt709_rescale.hip",
     """  const size_t lds = f16 ? scaled_f16_lds(p) : static_cast<size_t>(p.table_linear_bytes) + p.table_encode_bytes;
  const dim3 block(kBlockThreads);""",
     """#if defined(BT709_LAB_SCALED_ONCE_LDS)
  const size_t lds_tables = static_cast<size_t>(p.table_linear_bytes) + p.table_encode_bytes;
  p.lab_tile_off = static_cast<uint32_t>(lds_tables);  // the kernel's dynamic LDS starts at address 0 (no static LDS)
  const size_t lds = lds_tables + 16u * kBlockThreads;
#else
  const size_t lds = f16 ? scaled_f16_lds(p) : static_cast<size_t>(p.table_linear_bytes) + p.table_encode_bytes;
#endif
  const dim3 block(kBlockThreads);"""),
    ("bt709_kernels.h",
     """  uint32_t scaled_rows;  // output rows of a strip (filled by launch_decode_scaled)""",
     """  uint32_t lab_tile_off;  // BT709_LAB_SCALED_ONCE_LDS
  uint32_t scaled_rows;"""),
    ("bt709_encode.hip",  # the encoder's kernels are templates on the chroma layout: a gate reaches the NV12 and the I420 instantiation
     """    uint32_t ytop, ybot, cbcr;
    quantize_quad<LAYOUT>(va, vb, ytop, ybot, cbcr);
    if (q_raw < quads) {""",
     """    uint32_t ytop, ybot, cbcr;
#if defined(BT709_LAB_ENC_NO_ARITH)  // WRONG OUTPUT: the launch's loads and stores with no table lookups and no arithmetic
    ytop = top.x ^ top.y ^ top.z ^ top.w, ybot = bot.x ^ bot.y ^ bot.z ^ bot.w, cbcr = ytop + ybot;
    (void)va, (void)vb;
#else
    quantize_quad<LAYOUT>(va, vb, ytop, ybot, cbcr);
#endif
    if (q_raw < quads) {"""),
    ("bt709_encode.hip",
     """    {
      const uint32_t blk[4] = {top.x, top.y, bot.x, bot.y};
      encode_block(t, quarter_n, blk, va);
    }
    {
      const uint32_t blk[4] = {top.z, top.w, bot.z, bot.w};
      encode_block(t, quarter_n, blk, vb);
    }
""",
     """#if !defined(BT709_LAB_ENC_NO_ARITH)
    {
      const uint32_t blk[4] = {top.x, top.y, bot.x, bot.y};
      encode_block(t, quarter_n, blk, va);
    }
    {
      const uint32_t blk[4] = {top.z, top.w, bot.z, bot.w};
      encode_block(t, quarter_n, blk, vb);
    }
#endif
"""),
    ("bt709_kernels.hip",
     """      uint32_t b[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        b[ch] = QUANT ? quantise_byte(x[3 * k + ch]) : bucket_byte(ul, x[3 * k + ch], __float_as_uint(__fadd_rn(x[3 * k + ch], ul.magic)) >> ul.shift);
      o[k] = pack_bgra(b[0], b[1], b[2], p.alpha_word);
""",
     """#if defined(BT709_LAB_UNC_NO_ARITH)  // WRONG OUTPUT: +unconvert:'s loads and stores with no lookups
      o[k] = w[r][k] ^ p.alpha_word;
#else
      uint32_t b[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        b[ch] = QUANT ? quantise_byte(x[3 * k + ch]) : bucket_byte(ul, x[3 * k + ch], __float_as_uint(__fadd_rn(x[3 * k + ch], ul.magic)) >> ul.shift);
      o[k] = pack_bgra(b[0], b[1], b[2], p.alpha_word);
#endif
"""),
]

MACROS = ["BT709_LAB_ENC_I420_PAIRED", "BT709_LAB_ENC_I420_WIDE", "BT709_LAB_I420_PAIRED", "BT709_LAB_NO_ARITH", "BT709_LAB_NO_LOADS", "BT709_LAB_NO_STORES", "BT709_LAB_NO_TABLE", "BT709_NO_FMA_CENTRE",
          "BT709_INDEX_RTZ", "BT709_UNIFORM_INDEX_TWO_STEP", "BT709_REP_SPLIT_ENCODE", "BT709_LAB_BOUND_SHARED_INDEX",
          "BT709_LAB_BOUND_ONE_ENCODE", "BT709_LAB_HALF_TABLE", "BT709_LAB_F16_NO_ARITH", "BT709_LAB_F16_NO_TABLE",
          "BT709_LAB_F16_CVT_ONLY", "BT709_LAB_F16_NO_CAND_GATHER", "BT709_LAB_F16_NO_T_GATHER", "BT709_LAB_F16_NO_INDEX_SCALE", "BT709_LAB_F16_DMA_STAGING", "BT709_LAB_ENC_NO_ARITH", "BT709_LAB_UNC_NO_ARITH", "BT709_LAB_SCALED_QUARTER_FEWER_TAPS", "BT709_LAB_HALF_ENCODE_B32",
          "BT709_LAB_SCALED_HALF_FEWER_TAPS", "BT709_LAB_SCALED_PAIR_DPP", "BT709_LAB_SCALED_ONCE_LDS", "BT709_LAB_HUNT_TRACE", "BT709_LAB_SCALED_NO_FETCH", "BT709_LAB_SCALED_NO_DECODE", "BT709_LAB_SCALED_NO_ENCODE", "BT709_LAB_SCALED_NO_STORE", "BT709_LAB_SCALED_STORE_ONE_LINE", "BT709_LAB_ANY_ORDER", "BT709_LAB_HALF_NO_FETCH", "BT709_LAB_HALF_NO_STORE", "BT709_LAB_BAND_ROT", "BT709_LAB_BAND_XOR", "BT709_LAB_STEP32", "BT709_LAB_ROW32"]


GATES += [
    ("bt709_device.h",
     """  f.y += static_cast<int64_t>(i) * p.step_y;
  f.cbcr += static_cast<int64_t>(i) * p.step_cbcr;
  if (f.alpha) f.alpha += static_cast<int64_t>(i) * p.step_alpha;
  f.out += static_cast<int64_t>(i) * p.step_out;
""",
     """#if defined(BT709_LAB_STEP32)  // WRONG ADDRESSES: the steps' low 32 bits, zero-extended
  f.y += static_cast<int64_t>(i) * static_cast<int64_t>(static_cast<uint32_t>(p.step_y));
  f.cbcr += static_cast<int64_t>(i) * static_cast<int64_t>(static_cast<uint32_t>(p.step_cbcr));
  if (f.alpha) f.alpha += static_cast<int64_t>(i) * static_cast<int64_t>(static_cast<uint32_t>(p.step_alpha));
  f.out += static_cast<int64_t>(i) * static_cast<int64_t>(static_cast<uint32_t>(p.step_out));
#else
  f.y += static_cast<int64_t>(i) * p.step_y;
  f.cbcr += static_cast<int64_t>(i) * p.step_cbcr;
  if (f.alpha) f.alpha += static_cast<int64_t>(i) * p.step_alpha;
  f.out += static_cast<int64_t>(i) * p.step_out;
#endif
"""),
]

GATES += [
    # the row products of three kernels cut to 32 bits (tests/test_row_pitch_gpu.py, past-2^32: the last chroma row / target row lies above 2^32)
    ("bt709_tile.h",
     """    const uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    const uint8_t *y1 = y0 + p.y_stride;
    const uint8_t *cc = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;
    const uint8_t *vv = PLANAR ? cc + p.v_offset : nullptr;  // cc is the U row then
    const uint8_t *a0 = HAS_ALPHA ? f.alpha + static_cast<size_t>(2 * rp) * p.alpha_stride : nullptr;
""",
     """#if defined(BT709_LAB_ROW32)  // WRONG ADDRESSES: the products' low 32 bits, zero-extended
    const uint8_t *y0 = f.y + static_cast<size_t>(static_cast<uint32_t>(2 * rp * p.y_stride));
    const uint8_t *y1 = y0 + p.y_stride;
    const uint8_t *cc = f.cbcr + static_cast<size_t>(static_cast<uint32_t>(rp * p.cbcr_stride));
    const uint8_t *vv = PLANAR ? cc + p.v_offset : nullptr;
    const uint8_t *a0 = HAS_ALPHA ? f.alpha + static_cast<size_t>(static_cast<uint32_t>(2 * rp * p.alpha_stride)) : nullptr;
#else
    const uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
    const uint8_t *y1 = y0 + p.y_stride;
    const uint8_t *cc = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;
    const uint8_t *vv = PLANAR ? cc + p.v_offset : nullptr;  // cc is the U row then
    const uint8_t *a0 = HAS_ALPHA ? f.alpha + static_cast<size_t>(2 * rp) * p.alpha_stride : nullptr;
#endif
"""),
    ("bt709_rescale_half.hip",
     """  uint8_t *o = f.out + static_cast<size_t>(orow) * p.out_stride;
""",
     """#if defined(BT709_LAB_ROW32)  // the wide form only
  uint8_t *o = f.out + (WIDE ? static_cast<size_t>(static_cast<uint32_t>(orow * p.out_stride)) : static_cast<size_t>(orow) * p.out_stride);
#else
  uint8_t *o = f.out + static_cast<size_t>(orow) * p.out_stride;
#endif
"""),
    ("bt709_encode.hip",
     """      store_quad_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, q, cbcr);
""",
     """#if defined(BT709_LAB_ROW32)
      store_quad_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(static_cast<uint32_t>(rp * p.cbcr_stride)), q, cbcr);
#else
      store_quad_chroma<LAYOUT>(p, f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride, q, cbcr);
#endif
"""),
]

RESCALE_FILES = ("bt709_rescale.h", "bt709_rescale_half.hip", "bt709_rescale_scaled.hip", "bt709_scaled_strip.h")  # round 6 split bt709_rescale.hip; the strip shared with bt709_rescale_f16.hip moved to a header


GATES += [
    # round 12: the planar front end's other chroma-fetch design (profiles/LAB.md, "Round 12").  A lane whose quad q
    # is even loads the U dword of quads q, q + 1, its odd neighbour the V dword; quad_perm:[1,0,3,2] hands each the other's, and one
    # v_perm_b32 with a per-lane selector picks the lane's two U and two V bytes.  As many VMEM instructions as NV12.  In bounds only
    # while quads is even (the last even lane's dword ends at the row's last byte), the chroma planes are 4-byte aligned and V sits
    # less than 4 GiB behind U: the third gate below makes the shim send every other frame to the general kernel.
    ("bt709_tile.h",
     """        cu[j] = load16<NT>(cc + 2 * q);
        cv[j] = load16<NT>(vv + 2 * q);
""",
     """#if defined(BT709_LAB_I420_PAIRED)
        cu[j] = load32<NT>(cc + (4 * (q >> 1) + ((q & 1) ? static_cast<uint32_t>(p.v_offset) : 0u)));
        cv[j] = (q & 1) ? 0x07030602u : 0x01050004u;  // the perm's selector: bytes 0-3 the partner's dword, 4-7 the lane's own
#else
        cu[j] = load16<NT>(cc + 2 * q);
        cv[j] = load16<NT>(vv + 2 * q);
#endif
"""),
    ("bt709_tile.h",
     """      if constexpr (PLANAR) cw[j] = __builtin_amdgcn_perm(cv[j], cu[j], 0x05010400u);
""",
     """#if defined(BT709_LAB_I420_PAIRED)
      if constexpr (PLANAR) cw[j] = __builtin_amdgcn_perm(cu[j], static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(cu[j]), 0xB1, 0xF, 0xF, false)), cv[j]);
#else
      if constexpr (PLANAR) cw[j] = __builtin_amdgcn_perm(cv[j], cu[j], 0x05010400u);
#endif
"""),
    ("shim_decode.cpp",
     """  const bool fast = (p.width % 4) == 0 && info.in_align >= 4 && info.out_align >= out_need && (layout != BT709HIP_CHROMA_I420 || info.chroma_align >= 2);
""",
     """#if defined(BT709_LAB_I420_PAIRED)  // the paired fetch is in bounds for these frames only; the others take the general kernel
  const bool fast = (p.width % 4) == 0 && info.in_align >= 4 && info.out_align >= out_need &&
                    (layout != BT709HIP_CHROMA_I420 || ((p.width % 8) == 0 && info.chroma_align >= 4 && p.v_offset + p.width / 2 <= 0xffffffffull));
#else
  const bool fast = (p.width % 4) == 0 && info.in_align >= 4 && info.out_align >= out_need && (layout != BT709HIP_CHROMA_I420 || info.chroma_align >= 2);
#endif
"""),
]

GATES += [
    # round 13: the planar ENCODER's two other chroma-store designs (profiles/LAB.md, "Round 13").  The shipped one packs Cb0 Cb1
    # in the low half and Cr0 Cr1 in the high half of a quad's chroma word and issues two 2-byte stores a lane.
    # PAIRED: quad_perm:[1,0,3,2] hands each lane its neighbour's word; one v_perm_b32 builds U0..U3 in the even lane and V0..V3 in
    # the odd one, and each stores one dword -- as many VMEM instructions as NV12.
    ("bt709_encode.hip",
     """    __builtin_nontemporal_store(static_cast<uint16_t>(word), reinterpret_cast<uint16_t *>(row + 2u * q));
    __builtin_nontemporal_store(static_cast<uint16_t>(word >> 16), reinterpret_cast<uint16_t *>(row + v_plane_offset(p) + 2u * q));
""",
     """#if defined(BT709_LAB_ENC_I420_PAIRED)
    const uint32_t other = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(word), 0xB1, 0xF, 0xF, false));
    const bool odd = (q & 1u) != 0u;
    const uint32_t both = odd ? __builtin_amdgcn_perm(word, other, 0x07060302u) : __builtin_amdgcn_perm(other, word, 0x05040100u);
    __builtin_nontemporal_store(both, reinterpret_cast<uint32_t *>(row + (odd ? v_plane_offset(p) : 0ull) + 4u * (q >> 1)));
#else
    __builtin_nontemporal_store(static_cast<uint16_t>(word), reinterpret_cast<uint16_t *>(row + 2u * q));
    __builtin_nontemporal_store(static_cast<uint16_t>(word >> 16), reinterpret_cast<uint16_t *>(row + v_plane_offset(p) + 2u * q));
#endif
"""),
    # WIDE: the kernel is a template on the layout; the body below replaces the I420 instantiation of the colour kernel alone, and the
    # launcher gives it tiles of lane PAIRS of quads.
    ("bt709_encode.hip",
     """encode_bgra(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
""",
     """encode_bgra(const EncodeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
#if defined(BT709_LAB_ENC_I420_WIDE)
  if constexpr (LAYOUT == kChromaI420) {
    const BandedWork work = banded_work(p.xcd_bands, p.frames_per_band);
    const EncodeFrame f = encode_frame(p, work.frame);
    const uint32_t pairs = p.width >> 3;
    const uint32_t row_pairs = p.height >> 1;
    const uint32_t l_raw = work.tile * blockDim.x + threadIdx.x;
    const uint32_t l = min(l_raw, pairs - 1);
    const uint32_t rp0 = blockIdx.y * p.row_pairs_per_block;
    const uint32_t rp_end = min(rp0 + p.row_pairs_per_block, row_pairs);
    const uint8_t *s0 = f.bgra + static_cast<size_t>(2 * rp0) * p.bgra_stride;
    u32x4 top[2], bot[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      top[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + 32u * l + 16u * j));
      bot[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s0 + p.bgra_stride + 32u * l + 16u * j));
    }
    const EncodeLds t = stage_encode_tables(lds_raw, p);
    __syncthreads();
    const float quarter_n = __fmul_rn(0.25f, p.from_linear_scale);
    for (uint32_t rp = rp0; rp < rp_end; ++rp) {
      u32x4 ntop[2] = {top[0], top[1]}, nbot[2] = {bot[0], bot[1]};
      if (rp + 1 < rp_end) {
        const uint8_t *s1 = f.bgra + static_cast<size_t>(2 * (rp + 1)) * p.bgra_stride;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          ntop[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + 32u * l + 16u * j));
          nbot[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s1 + p.bgra_stride + 32u * l + 16u * j));
        }
      }
      uint32_t yt[2], yb[2], cc[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float va[6], vb[6];
        const uint32_t blk0[4] = {top[j].x, top[j].y, bot[j].x, bot[j].y};
        encode_block(t, quarter_n, blk0, va);
        const uint32_t blk1[4] = {top[j].z, top[j].w, bot[j].z, bot[j].w};
        encode_block(t, quarter_n, blk1, vb);
        quantize_quad<kChromaI420>(va, vb, yt[j], yb[j], cc[j]);
      }
      if (l_raw < pairs) {
        uint8_t *y0 = f.y + static_cast<size_t>(2 * rp) * p.y_stride;
        __builtin_nontemporal_store(u32x2{yt[0], yt[1]}, reinterpret_cast<u32x2 *>(y0 + 8u * l));
        __builtin_nontemporal_store(u32x2{yb[0], yb[1]}, reinterpret_cast<u32x2 *>(y0 + p.y_stride + 8u * l));
        uint8_t *row = f.cbcr + static_cast<size_t>(rp) * p.cbcr_stride;
        __builtin_nontemporal_store(__builtin_amdgcn_perm(cc[1], cc[0], 0x05040100u), reinterpret_cast<uint32_t *>(row + 4u * l));
        __builtin_nontemporal_store(__builtin_amdgcn_perm(cc[1], cc[0], 0x07060302u), reinterpret_cast<uint32_t *>(row + v_plane_offset(p) + 4u * l));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) top[j] = ntop[j], bot[j] = nbot[j];
    }
    return;
  }
#endif
"""),
    ("bt709_encode.hip",
     """    grid = dim3((quads + threads - 1) / threads, (p.height / 2 + p.row_pairs_per_block - 1) / p.row_pairs_per_block, frames);
""",
     """#if defined(BT709_LAB_ENC_I420_WIDE)
    uint32_t units = quads;
    if (p.chroma_layout == kChromaI420 && !alpha) {  // a lane owns two quads: the NV12 plan's rules over half as many lanes
      units = quads / 2;
      threads = p.block_threads ? p.block_threads : encode_block_threads(p.width / 2);
      if (p.block_threads == 0 && frames == 1) {
        const uint32_t tiles = (units + 511) / 512;
        threads = ((units + tiles - 1) / tiles + 63) / 64 * 64;
        if (threads < 64) threads = 64;
      }
      if (threads > static_cast<uint32_t>(kMaxBlockThreads)) threads = kMaxBlockThreads;
    }
    grid = dim3((units + threads - 1) / threads, (p.height / 2 + p.row_pairs_per_block - 1) / p.row_pairs_per_block, frames);
#else
    grid = dim3((quads + threads - 1) / threads, (p.height / 2 + p.row_pairs_per_block - 1) / p.row_pairs_per_block, frames);
#endif
"""),
]


def resolve(csrc, name, product):
    """The file of `csrc` a gate anchors on: `name`, or -- for gates written against the former bt709_rescale.hip -- whichever of
    its three successors holds the product text exactly once.  None when no file does."""
    names = [name] if os.path.exists(os.path.join(csrc, name)) else (RESCALE_FILES if name == "bt709_rescale.hip" else ())
    hits = [n for n in names if open(os.path.join(csrc, n)).read().count(product) == 1]
    return hits[0] if len(hits) == 1 else None


def make_lab_sources(dst=LAB_SRC):
    """csrc/ copied to `dst` with every gate re-inserted; returns dst."""
    from metalbt709decoder_amd import build as b
    if os.path.isdir(dst):
        shutil.rmtree(dst)
    shutil.copytree(b.CSRC, dst)
    for name, product, lab in GATES:
        found = resolve(dst, name, product)
        if found is None:
            raise SystemExit("tools/lab_variants.py: the product text this gate anchors on does not occur exactly once in csrc/%s "
                             "(or its successors): re-state the experiment against the current kernel\n---\n%s" % (name, product))
        path = os.path.join(dst, found)
        text = open(path).read()
        open(path, "w").write(text.replace(product, lab))
    # the copy sits two levels deeper than csrc/: point its includes of the public headers at the real ones
    for name in os.listdir(dst):
        path = os.path.join(dst, name)
        text = open(path).read()
        for header in ("bt709hip.h", "bt709hip_ext.h"):
            text = text.replace('"../../include/%s"' % header, '"%s"' % os.path.join(ROOT, "include", header))
        open(path, "w").write(text)
    return dst


def main(argv):
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    if argv[0] == "--list":
        print("\n".join(MACROS))
        return 0
    if argv[0] == "--sources":
        print(make_lab_sources())
        return 0
    from metalbt709decoder_amd import build as b
    out = os.path.abspath(argv[0])
    src = make_lab_sources()
    print("built", b.build_variant(out, argv[1:], csrc=src))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
