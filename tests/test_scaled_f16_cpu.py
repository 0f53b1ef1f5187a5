"""The fused decode + rescale through the RGBA16Float intermediate (BT709HIP_OPT_SCALE_INTERMEDIATE), the parts
that need no GPU: the option itself, the ABI it must not move, and the arithmetic-fusing contract of its kernels' ISA."""
import ctypes as C
import os
import re

import pytest

import abi_headers
import metalbt709decoder_amd as mb
from metalbt709decoder_amd import _capi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return mb.load_library()


@pytest.fixture()
def bare_decoder(lib):
    """A decoder that has no context: options are plain properties, settable before anything touches a device."""
    h = C.c_void_p()
    assert lib.bt709hip_decoder_create(None, mb.MetalBT709GammaApple, 0, C.byref(h)) == _capi.OK
    yield h
    lib.bt709hip_decoder_destroy(h)


def _get(lib, dec, option):
    v = C.c_int(-12345)
    assert lib.bt709hip_decoder_get_option(dec, option, C.byref(v)) == _capi.OK
    return v.value


def test_option_constant_is_the_headers():
    header = open(os.path.join(ROOT, "include", "bt709hip_ext.h")).read()
    m = re.search(r"\bBT709HIP_OPT_SCALE_INTERMEDIATE\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == 8 == _capi.OPT_SCALE_INTERMEDIATE
    assert (_capi.FORMAT_BGRA8_SRGB, _capi.FORMAT_RGBA16F) == (0, 1)


def test_option_default_set_get_and_refusals(lib, bare_decoder):
    opt = _capi.OPT_SCALE_INTERMEDIATE
    assert _get(lib, bare_decoder, opt) == _capi.FORMAT_BGRA8_SRGB  # the default: the 8-bit intermediate
    for held in (_capi.FORMAT_RGBA16F, _capi.FORMAT_BGRA8_SRGB):
        assert lib.bt709hip_decoder_set_option(bare_decoder, opt, held) == _capi.OK
        assert _get(lib, bare_decoder, opt) == held
        for bad in (2, 3, -1):  # 3 is a bt709hip_format too (BGRA8_ALPHA), but no intermediate
            assert lib.bt709hip_decoder_set_option(bare_decoder, opt, bad) == _capi.ERR_INVALID_ARG
            assert _get(lib, bare_decoder, opt) == held  # a refused value leaves the option as it was


def test_python_mirror_property_names_the_resize_texture_format():
    d = mb.MetalBT709Decoder()
    assert d.resizeTexturePixelFormat == mb.MTLPixelFormatBGRA8Unorm_sRGB
    d.resizeTexturePixelFormat = mb.MTLPixelFormatRGBA16Float  # before setupMetal: applied at setup, like every option
    assert d.resizeTexturePixelFormat == mb.MTLPixelFormatRGBA16Float
    assert d._options[_capi.OPT_SCALE_INTERMEDIATE] == _capi.FORMAT_RGBA16F
    with pytest.raises(ValueError):
        d.resizeTexturePixelFormat = 80  # MTLPixelFormatBGRA8Unorm: not a format the reference's _resizeTexture takes
    assert d.resizeTexturePixelFormat == mb.MTLPixelFormatRGBA16Float


def test_abi_is_unchanged(lib):
    """A new VALUE of an existing enum: no export, no signature, no struct layout, so no ABI bump."""
    assert lib.bt709hip_abi_version() == 504
    header = re.sub(r"/\*.*?\*/", "", abi_headers.text(), flags=re.S)
    assert len(set(re.findall(r"\b(bt709hip_[a-z0-9_]+)\s*\(", header))) == 103


TAPS_ONCE = 4  # bt709_kernels.h TAPS_*: the wave decodes a source pixel once, the pairs (R, G) and (B, A)


def test_isa_of_the_f16_kernels_fuses_nothing_but_the_proven():
    """Arithmetic fusing only.  In every decode_nv12_scaled_f16 instantiation the fma-class instructions are: centre_norm's
    byte * (1/255f) - off * (1/255f) (bt709_device.h: the same single rounding as the reference's subtract + multiply); the half
    CANDIDATE's slope * x + intercept, three register operands, one per curve channel of every place a source row is converted
    -- 3 per pixel where the wave decodes a pixel once, 6 per row of two taps otherwise, counted here against the packed index
    conversions (v_cvt_pkrtz_f16_f32: one per PAIR, so 2 per pixel / 3 per row) -- none in the instantiations without a
    curve; and the encode table's index fma should hipcc choose to emit one (its multiplier is 1.0 in unit range: today it
    is a plain add).  No multiply fused with the float -> half conversion (v_fma_mix*: bucket 0's product must round to
    binary32 first), no transcendental, no half-rate packed fma / add, and no scratch."""
    asm = open(build.emit_asm()).read()
    bodies = re.findall(r"^(_ZN5bt70922decode_nv12_scaled_f16\w*):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M)
    assert len(bodies) == 15  # 5 tap forms x (curve, curve + alpha plane, no curve)
    for name, body in bodies:
        taps, alpha, curve = re.search(r"scaled_f16ILi(\d)ELb([01])ELb([01])E", name).groups()
        pairs = len(re.findall(r"\bv_cvt_pkrtz_f16_f32", body))
        want_candidates = 0 if curve == "0" else (pairs * 3 // 2 if int(taps) == TAPS_ONCE else pairs * 2)
        assert (pairs > 0) == (curve == "1"), name
        candidates = 0
        for line in re.findall(r"^\s*(v_(?:pk_)?(?:fma|fmac|fmamk|fmaak|mad|mac|madmk|madak)_(?:f32|f16|legacy|mix)\w*\s[^\n]*)", body, flags=re.M):
            line = line.strip()
            if re.match(r"v_fmac_f32_e32 v\d+, v\d+, v\d+$|v_fma_f32 v\d+, v\d+, v\d+, v\d+$", line):
                candidates += 1
                continue
            if re.match(r"v_fmamk_f32 v\d+, v\d+, 0x3f800000, v\d+$|v_fmac_f32_e32 v\d+, (1\.0|0x3f800000), v\d+$", line):
                continue  # the log-bucket encode table's index, bits(fma(sum, 1.0, 2^-5)) >> 16: the product is exact
            assert re.match(r"v_fmamk_f32 v\d+, v\d+, 0x3b808081, v\d+|v_fmac_f32_e32 v\d+, 0x3b808081, v\d+", line), (name, line)
        assert candidates == want_candidates, (name, candidates, want_candidates)
        assert not re.search(r"\bv_fma_mix|\bv_mad_mix", body), name
        assert not re.search(r"\bv_(log|exp)_f32", body), name
        assert not re.search(r"\bv_pk_(fma|add)_f32", body), name
        meta = re.search(r"\.name:\s+%s\b.*?\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), asm, flags=re.S)
        assert meta and int(meta.group(1)) == 0, name  # no scratch
