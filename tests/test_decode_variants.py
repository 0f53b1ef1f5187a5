"""The 1:1 instantiations and launch shapes a caller lands in without asking -- a plane pitch that is no multiple of 4, a target
at a 4-byte offset, streaming stores turned off -- held to the oracle byte for byte (tests/variant_cases.py builds the cases):

  1. every (Y,Cb,Cr) through the temporal quads kernels, through the general path (decode_block: the 12-wide index, the table's
     form as a run-time shift) entered by the input pitches and by the output pitch, through the general path's alpha
     decoder with every alpha code in every position of a 2x2 block, and every packed 4:4:4 word, under every value of the
     byte +unconvert: ignores, through the vectorised and the per-pixel unconvert kernel;
  2. the general path's launch shapes: a grid-stride loop that takes three trips with a ragged last one, batches through
     the pointer table and through the even step, the composite-over kernels over per-frame backgrounds, and a batch the
     XCD-band map must leave alone -- sizes computed from the device, the launch asserted from bt709hip_last_launch_info,
     every byte outside the pixels checked.

Every test asserts the exact kernel name: no case can pass on a neighbouring instantiation.  The unmarked tests guard the
case builders on the CPU."""
import hashlib

import numpy as np
import pytest

import metalbt709decoder_amd as mb
import over_cases as oc
import variant_cases as vc
from metalbt709decoder_amd import _capi
from oracle_lib import GAMMA_NAMES

APPLE, SRGB, LINEAR, ITU709 = mb.MetalBT709GammaApple, mb.MetalBT709GammaSRGB, mb.MetalBT709GammaLinear, mb.MetalBT709GammaITU709
GAMMAS = (APPLE, SRGB, LINEAR, ITU709)
TEMPORAL_QUADS = {APPLE: b"decode_nv12_quads", SRGB: b"decode_nv12_quads<quantiser>", LINEAR: b"decode_nv12_quads_log"}
# the LINEAR mode runs the plain general-path kernel over its log-bucket table: the run-time shift of 16
BLOCKS = {APPLE: b"decode_nv12_blocks", SRGB: b"decode_nv12_blocks<quantiser>", LINEAR: b"decode_nv12_blocks", ITU709: b"decode_nv12_blocks"}
UNCONVERT = {"vec": b"unconvert_packed444<vec>", "per-pixel": b"unconvert_packed444"}


@pytest.fixture(scope="module")
def colours():
    return vc.Colours()


@pytest.fixture(scope="module")
def tables(oracle):
    """oracle.decode_table per gamma, built on first use."""
    memo = {}

    def table(gamma):
        if gamma not in memo:
            memo[gamma] = oracle.decode_table(gamma)
        return memo[gamma]
    return table


@pytest.fixture(scope="module")
def words():
    return {name: vc.unconvert_words(*size) for name, size in vc.UNCONVERT_LAYOUTS.items()}


# ------------------------------------------------------------------ CPU guards

@pytest.mark.parametrize("gamma", GAMMAS)
def test_expected_image_is_the_reference_table(oracle, refdata, colours, gamma):
    """The expected image is the oracle's table indexed by the frame's triples; the table hashes to what the reference's own
    headers produced, and gpu_helpers.exhaustive_to_table takes the image back to it."""
    import gpu_helpers
    table = oracle.decode_table(gamma)
    assert hashlib.sha256(table.tobytes()).hexdigest() == refdata["table_sha256"][GAMMA_NAMES[gamma]]
    img = colours.image(oracle, gamma)
    assert img.shape == (4096, 4096, 4) and (img[..., 3] == 0xFF).all()
    assert np.array_equal(gpu_helpers.exhaustive_to_table(img, colours.y, colours.c), table)
    for r, x in ((0, 0), (1, 3), (2049, 1022), (4095, 4095)):
        Y, Cb, Cr = (int(a[r, x]) for a in colours.blocks)
        assert tuple(int(v) for v in img[r, x, 2::-1]) == oracle.decode_pixel(gamma, Y, Cb, Cr)


def test_alpha_ramp_carries_every_code_in_every_position(oracle):
    a = vc.alpha_ramp(4096, 4096)
    assert a.shape == (4096, 4096) and vc.alpha_ramp_coverage(a).all()  # all 4 x 256 (position, code) pairs
    per_row = ((np.arange(4096)[None, :] + np.arange(4096)[:, None]) & 255).astype(np.uint8)
    assert vc.alpha_ramp_coverage(per_row).sum() == 4 * 128  # why the shift is per row PAIR: a position fixes x + row's parity
    # the alpha bytes the GPU test expects are the oracle's decode of a frame, not only of a code
    y, c = np.full((4, 512), 128, np.uint8), np.full((2, 512), 128, np.uint8)
    alpha_map = np.array([oracle.decode_alpha(v) for v in range(256)], np.uint8)
    assert np.array_equal(oracle.decode_nv12(SRGB, y, c, alpha=a[:4, :512]).reshape(4, 512, 4)[..., 3], alpha_map[a[:4, :512]])


@pytest.mark.parametrize("gamma", GAMMAS)
def test_unconvert_expectation_is_the_oracles(oracle, tables, words, gamma):
    for name, (w, h) in vc.UNCONVERT_LAYOUTS.items():
        v = words[name]
        assert v.shape == (h, w) and w % 2 == 0 and h % 2 == 0 and (w % 4 == 0) == (name == "vec")
        if gamma == GAMMAS[0]:  # the coverage the test claims: every triple, byte 3 every value
            assert np.bincount((v & 0xFFFFFF).reshape(-1), minlength=1 << 24).min() >= 1
            assert np.unique(v[:, 0] >> 24).size == 256 and np.array_equal(v >> 24, np.broadcast_to((np.arange(h) & 255)[:, None], v.shape))
        rows = np.r_[0:2, 254:258, h - 2:h]  # byte 3 = 0, 1, 254, 255, 0, 1 and the last rows
        want = vc.unconvert_expected(tables(gamma), v[rows])
        assert np.array_equal(want.reshape(-1), oracle.unconvert_packed(gamma, v[rows], w, rows.size))
        assert (want >> 24 == 0).all()


def test_launch_shape_cases_stride_on_any_part():
    """Three trips of the grid-stride loop with a ragged last one, on any compute-unit count: the grid a case will assert is the
    mirror of the shim's grid_x_for, and it is smaller than half the row pairs.  (One workgroup per frame -- a part of fewer
    than ~9 CUs -- cannot have a ragged trip; the loop then takes row_pairs >= 7 trips.)"""
    for cus in range(1, 513):
        for name in vc.LAUNCH_CASES:
            case = vc.launch_case(name, cus)
            n, pf, rows = case["frames"], case["per_frame"], case["row_pairs"]
            assert pf == max(1, cus * 8 * 2 // n) and case["grid"] == (pf, n, 1), (name, cus)
            assert rows > 2 * pf, (name, cus, case)
            assert rows % pf != 0 or pf == 1, (name, cus, case)
            assert rows in (2 * pf + (3 if n == 1 else 5), 2 * pf + 6)
            if cus == 256:  # this part: the sizes the cases are named after
                assert rows == 2 * pf + (3 if n == 1 else 5) and n * vc.LAUNCH_WIDTH * 2 * rows < 200_000, (name, case)
    assert vc.launch_case("one-frame", 256)["row_pairs"] == 8195
    assert vc.LAUNCH_CASES["step-40"][0] > _capi.MAX_BATCH and vc.LAUNCH_CASES["table-32"][0] == _capi.MAX_BATCH
    assert vc.grid_x_for(256, 27, 1) == 27 and vc.grid_x_for(256, 8195, 1) == 4096 and vc.grid_x_for(1, 7, 72) == 1


# ------------------------------------------------------------------ GPU plumbing

@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    gpu_helpers.context()
    return gpu_helpers


@pytest.fixture(scope="module")
def rig(gh):
    r = vc.Rig(gh)
    yield r
    r.close()


@pytest.fixture(scope="module")
def tabs(oracle):
    return oc.tables(oracle)


# layout -> pads of the (Y, CbCr, alpha, output) rows, alpha plane
LAYOUTS = {"aligned": ((0, 0, 0, 0), False),    # the fast path
           "odd": ((1, 3, 0, 0), False),        # luma pitch 4097, chroma pitch 4099
           "out+4": ((0, 0, 0, 4), False),      # aligned planes, an output pitch of 4 * 4096 + 4
           "odd-alpha": ((1, 3, 5, 0), True)}   # and an alpha plane of pitch 4101


@pytest.fixture(scope="module")
def frames(rig, colours):
    """The every-colour frame in device memory, uploaded once per layout."""
    jobs = {}

    def job(layout):
        if layout not in jobs:
            pads, alpha = LAYOUTS[layout]
            jobs[layout] = vc.Job(rig, [(colours.y, colours.c, vc.alpha_ramp(*colours.y.shape) if alpha else None)], pads=pads)
        return jobs[layout]
    yield job
    for j in jobs.values():
        j.free()


def _decode_every_colour(rig, gh, frames, layout, gamma, options=(), has_alpha=False):
    job = frames(layout)
    job.frames[0].transfer = gh.TRANSFER_FOR_GAMMA[gamma]
    job.fill(None)
    dec = rig.decoder(gamma=gamma, has_alpha=has_alpha, options=options)
    _capi.check(job.decode_one(dec), "%s, gamma %d" % (layout, gamma))
    name, launch = rig.kernel(), rig.launch()
    return dec, name, launch, job.collect("%s, gamma %d" % (layout, gamma))[0]


# ------------------------------------------------------------------ 1. every colour through every 1:1 instantiation

@pytest.mark.gpu
@pytest.mark.parametrize("gamma", sorted(TEMPORAL_QUADS))
def test_gpu_every_colour_through_the_temporal_quads(rig, gh, oracle, colours, frames, gamma):
    """BT709HIP_OPT_NONTEMPORAL = 0: the fast path's three kernels with the default cache policy (ITU-709 shares Apple's)."""
    dec, name, launch, got = _decode_every_colour(rig, gh, frames, "aligned", gamma, options=[(_capi.OPT_NONTEMPORAL, 0)])
    assert name == TEMPORAL_QUADS[gamma], name
    assert rig.option(dec, _capi.OPT_NONTEMPORAL) == 0
    colours.assert_image(got, colours.image(oracle, gamma), "%s, gamma %d" % (name.decode(), gamma))


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", GAMMAS)
def test_gpu_every_colour_through_the_general_path(rig, gh, oracle, colours, frames, gamma):
    """A luma pitch of 4097 and a chroma pitch of 4099: decode_block in every gamma, the LINEAR mode's shift of 16 included."""
    dec, name, launch, got = _decode_every_colour(rig, gh, frames, "odd", gamma)
    assert name == BLOCKS[gamma], name
    cus = rig.ctx.info().compute_units
    assert launch == ((vc.grid_x_for(cus, 2048, 1), 1, 1), (256, 1, 1), 1, 0), launch
    colours.assert_image(got, colours.image(oracle, gamma), "%s, odd pitches, gamma %d" % (name.decode(), gamma))


@pytest.mark.gpu
def test_gpu_every_colour_through_the_general_path_by_the_output_pitch(rig, gh, oracle, colours, frames):
    """Aligned planes into a target whose pitch is only a multiple of 4: the other way into the general path (out_align)."""
    dec, name, launch, got = _decode_every_colour(rig, gh, frames, "out+4", APPLE)
    assert name == b"decode_nv12_blocks", name
    assert frames("out+4").so == 4 * 4096 + 4 and launch[1:] == ((256, 1, 1), 1, 0), launch
    colours.assert_image(got, colours.image(oracle, APPLE), "decode_nv12_blocks, output pitch 4 * 4096 + 4")


@pytest.mark.gpu
def test_gpu_every_colour_through_the_general_path_alpha_decoder(rig, gh, oracle, refdata, colours, frames):
    """decode_nv12_blocks<alpha>: the colours are the sRGB mode's (they hash to the reference's table), the alpha bytes the
    oracle's for every code in every position of a block."""
    dec, name, launch, got = _decode_every_colour(rig, gh, frames, "odd-alpha", SRGB, has_alpha=True)
    assert name == b"decode_nv12_blocks<alpha>", name
    a = vc.alpha_ramp(*colours.y.shape)
    want = colours.image(oracle, SRGB).copy()
    want[..., 3] = np.array([oracle.decode_alpha(v) for v in range(256)], np.uint8)[a]
    colours.assert_image(got, want, "decode_nv12_blocks<alpha>")
    table = gh.exhaustive_to_table(got, colours.y, colours.c)
    assert hashlib.sha256(table.tobytes()).hexdigest() == refdata["table_sha256"][GAMMA_NAMES[SRGB]]


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("layout", sorted(vc.UNCONVERT_LAYOUTS))
def test_gpu_every_word_through_unconvert(gh, oracle, tables, words, layout, gamma):
    """+unconvert: on every 24-bit word, byte 3 taking every value: it must not reach the output (alpha fill 0)."""
    ctx = gh.context()
    w, h = vc.UNCONVERT_LAYOUTS[layout]
    dec = gh.make_decoder(gamma, alpha_fill=0)
    tex = ctx.makeBGRATexture((w, h))
    assert mb.BGRAToBT709Converter.unconvert(dec, words[layout], tex, w, h), dec.lastStatus
    name = ctx.lib.bt709hip_last_kernel_name()
    assert name == UNCONVERT[layout], name
    assert ctx.lib.bt709hip_decoder_get_gamma(dec._handle) == gamma  # the quantiser / table form follows the gamma alone
    got, want = ctx.getBGRATexturePixels(tex), vc.unconvert_expected(tables(gamma), words[layout])
    if not np.array_equal(got, want):
        r, x = np.argwhere(got != want)[0]
        v = int(words[layout][r, x])
        raise AssertionError("%s, gamma %d: word %#010x (Y, Cb, Cr) = (%d, %d, %d): got %#010x, want %#010x; %d words differ"
                             % (name.decode(), gamma, v, v & 255, v >> 8 & 255, v >> 16 & 255, got[r, x], want[r, x], int((got != want).sum())))


# ------------------------------------------------------------------ 2. general-path launch shapes

LAUNCH_RUNS = [("one-frame", LINEAR), ("one-frame", APPLE), ("table-32", APPLE), ("step-40", APPLE), ("step-40-alpha", SRGB),
               ("table-32-over", SRGB), ("table-32-over-colour", SRGB), ("bands-72", APPLE)]
OVER_NAME = {"destination": b"decode_nv12_blocks<alpha,over>", "colour": b"decode_nv12_blocks<alpha,over-colour>"}
OVER_COLOUR = 0x3C7FB2


@pytest.mark.gpu
@pytest.mark.parametrize("run", LAUNCH_RUNS, ids=["%s-gamma%d" % r for r in LAUNCH_RUNS])
def test_gpu_general_path_launch_shapes(rig, gh, oracle, tabs, run):
    """Width 6, one lane column, tall enough for three trips of `for (rp = blockIdx.x; rp < row_pairs; rp += gridDim.x)` with a
    ragged last one; frame_planes(p, blockIdx.y) through the pointer table (a gap before the last frame) and through the even
    step (a step that itself misaligns the frames, more frames than BT709HIP_MAX_BATCH); decode_nv12_blocks_over reading and
    rewriting its target inside the loop; 72 evenly spaced frames that BT709HIP_OPT_XCD_BANDS, at its default, must leave one
    plain launch (plan_bands is asked for the quads variant only).  Every frame its own random content."""
    name, gamma = run
    case = vc.launch_case(name, rig.ctx.info().compute_units)
    n, w, h = case["frames"], vc.LAUNCH_WIDTH, 2 * case["row_pairs"]
    assert case["row_pairs"] > 2 * case["per_frame"] and n * w * h < 200_000
    planes = vc.random_planes(w, h, seed=9000 + n + gamma, n=n, alpha=case["alpha"])
    bg = vc.random_backgrounds(w, h, seed=9100 + n, n=n) if case["over"] == "destination" else None
    over = {None: None, "destination": _capi.OVER_DESTINATION, "colour": OVER_COLOUR}[case["over"]]
    job = vc.Job(rig, planes, pads=(1, 3, 2, 4), spacing=case["spacing"], step_pad=case["step_pad"], transfer=gh.TRANSFER_FOR_GAMMA[gamma])
    try:
        job.fill(bg)
        dec = rig.decoder(over, gamma=gamma, has_alpha=case["alpha"])
        if name == "bands-72":
            assert rig.option(dec, _capi.OPT_XCD_BANDS) == 1
        _capi.check(job.decode_batch(dec) if n > 1 else job.decode_one(dec), name)
        kernel, launch = rig.kernel(), rig.launch()
        got = job.collect(name)
    finally:
        job.free()
    assert kernel == (OVER_NAME[case["over"]] if case["over"] else b"decode_nv12_blocks<alpha>" if case["alpha"] else BLOCKS[gamma]), kernel
    assert launch == ((case["per_frame"], n, 1), (256, 1, 1), 1, 0), (launch, case)
    for i, (y, c, a) in enumerate(planes):
        want = oracle.decode_nv12(gamma, y, c, alpha=a).reshape(h, w, 4)
        if case["over"]:
            want = oc.composite_over(want, bg[i] if bg else OVER_COLOUR, *tabs)
        vc.assert_equal(got[i], want, "%s, frame %d of %d" % (name, i, n))
