"""Analytic known-answer streams on the CPU: scripted streams (tests/scripted_h264.py) whose expected pictures no decoder computed.

Three layers, each resting on the one before:
  1. the closed forms and the vectorised restatements of tests/analytic_expect.py against the literal clause restatements that the suite already had
     (tests/test_mc_packed.py::luma_literal, the 8-270 chroma formula) on random parameters -- no decoder is involved at all;
  2. every scripted stream through the CPU oracle, both output formats: frames == the analytic expectation, byte for byte;
  3. every scripted stream through a parse_only product handle: the host parser accepts a typing of the syntax that is not the generator's.
The GPU half is tests/test_analytic_gpu.py."""
import functools

import numpy as np
import pytest

import analytic_cases as ac
import analytic_expect as ae
import deblock_ref
import scripted_h264 as sw
from jmcodec_amd import api
from test_mc_packed import luma_literal

CASES = [(n, s) for n in sorted(ac.H264_CASES) for s in ac.case_sizes(n)]
IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]


def padded(R, pad):
    """R with `pad` clamped samples on every side: position (x, y) of R is (x + pad, y + pad) here."""
    return np.pad(R, pad, mode="edge")


# ---- 1. closed forms and vectorised restatements, no decoder ------------------------------------------------------------------------------------
def test_vectorised_luma_is_luma_literal():
    rng = np.random.default_rng(0xA001)
    R = rng.integers(0, 256, (40, 48), dtype=np.uint8)
    pad = 64
    Rp = padded(R, pad)
    for trial in range(64):
        mv = (int(rng.integers(-200, 200)), int(rng.integers(-160, 160)))
        if trial < 16:
            mv = (4 * int(rng.integers(-8, 8)) + trial % 4, 4 * int(rng.integers(-8, 8)) + trial // 4)
        w, h = [(16, 16), (16, 8), (8, 16)][trial % 3]
        x0, y0 = int(rng.integers(0, 48 - w + 1)), int(rng.integers(0, 40 - h + 1))
        got = ae.mc_luma(R, x0, y0, w, h, mv)
        xi, yi = x0 + (mv[0] >> 2), y0 + (mv[1] >> 2)
        for (dy, dx) in [(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0), (int(rng.integers(0, h)), int(rng.integers(0, w)))]:
            # edge padding IS the clamp of 8-239 / 8-240 as long as the footprint stays inside the padding (|mv| <= 50 samples, pad 64)
            assert got[dy, dx] == luma_literal(Rp, xi + dx + pad, yi + dy + pad, mv[0] & 3, mv[1] & 3), (trial, mv, x0, y0, dx, dy)


def test_vectorised_chroma_is_equation_8_270():
    rng = np.random.default_rng(0xA002)
    R = rng.integers(0, 256, (20, 24), dtype=np.uint8)
    for trial in range(128):
        mv = (8 * int(rng.integers(-30, 30)) + trial % 8, 8 * int(rng.integers(-30, 30)) + (trial // 8) % 8)
        x0, y0 = int(rng.integers(0, 17)), int(rng.integers(0, 13))
        got = ae.mc_chroma(R, x0, y0, 8, 8, mv)
        fx, fy = mv[0] & 7, mv[1] & 7
        S = lambda x, y: int(R[min(max(y, 0), 19), min(max(x, 0), 23)])
        for dy in range(8):
            for dx in range(8):
                x, y = x0 + dx + (mv[0] >> 3), y0 + dy + (mv[1] >> 3)
                want = ((8 - fx) * (8 - fy) * S(x, y) + fx * (8 - fy) * S(x + 1, y) + (8 - fx) * fy * S(x, y + 1) + fx * fy * S(x + 1, y + 1) + 32) >> 6
                assert got[dy, dx] == want, (trial, mv, dx, dy)


def test_ramp_closed_forms_against_the_literal_restatements():
    """Slopes -2 .. 2, every fractional position, random offsets: ramp_luma_closed == luma_literal where the six-tap footprint is inside, and
    ramp_chroma_closed == 8-270."""
    rng = np.random.default_rng(0xA003)
    for a in range(-2, 3):
        for c in range(-2, 3):
            lo, hi = -min(0, a * 23) - min(0, c * 19), 255 - max(0, a * 23) - max(0, c * 19)
            d = int(rng.integers(lo, hi + 1))
            R = ae.ramp(20, 24, a, c, d)
            for fy in range(4):
                for fx in range(4):
                    for (x, y) in [(2, 2), (20, 16), (int(rng.integers(2, 21)), int(rng.integers(2, 17)))]:
                        assert ae.ramp_luma_closed(int(R[y, x]), a, c, fx, fy) == luma_literal(R, x, y, fx, fy), (a, c, d, fx, fy, x, y)
            for fy in range(8):
                for fx in range(8):
                    x, y = int(rng.integers(0, 23)), int(rng.integers(0, 19))
                    want = int(ae.mc_chroma(R, x, y, 1, 1, (fx, fy))[0, 0])
                    assert ae.ramp_chroma_closed(int(R[y, x]), a, c, fx, fy) == want, (a, c, d, fx, fy, x, y)


def test_half_sample_chroma_is_the_rounded_mean():
    rng = np.random.default_rng(0xA004)
    R = rng.integers(0, 256, (12, 12), dtype=np.uint8)
    A, B, C, D = (R[:8, :8].astype(int), R[:8, 1:9].astype(int), R[1:9, :8].astype(int), R[1:9, 1:9].astype(int))
    assert np.array_equal(ae.mc_chroma(R, 0, 0, 8, 8, (4, 0)), (A + B + 1) >> 1)
    assert np.array_equal(ae.mc_chroma(R, 0, 0, 8, 8, (0, 4)), (A + C + 1) >> 1)
    assert np.array_equal(ae.mc_chroma(R, 0, 0, 8, 8, (4, 4)), (A + B + C + D + 2) >> 2)


def test_plane_prediction_continues_a_ramp_and_dc_forms():
    """8.3.3.4 / 8.3.4.4 on a ramp with slopes within -4 .. 4 give the ramp (derivation: analytic_cases.intra16_beside_pcm); DC over flat neighbours is
    that value; DC without neighbours is 128."""
    for (a, c, d) in [(1, 1, 20), (-3, 2, 160), (4, -4, 130), (0, 0, 77), (-4, 1, 200), (2, -1, 60)]:
        Y = ae.ramp(32, 32, a, c, d) if max(abs(a), abs(c)) * 31 + 0 <= 255 and 0 <= d + min(0, a * 31) + min(0, c * 31) and \
            d + max(0, a * 31) + max(0, c * 31) <= 255 else None
        if Y is None:
            continue
        assert np.array_equal(ae.intra16_luma(Y, 16, 16, 3, True, True), Y[16:, 16:]), (a, c, d)
        assert np.array_equal(ae.intra_chroma(Y, 16, 16, 3, True, True), Y[16:24, 16:24]), (a, c, d)
    F = np.full((32, 32), 93, np.uint8)
    for (al, at) in [(True, True), (True, False), (False, True)]:
        assert (ae.intra16_luma(F, 16, 16, 2, al, at) == 93).all() and (ae.intra_chroma(F, 16, 16, 0, al, at) == 93).all()
    assert (ae.intra16_luma(F, 16, 16, 2, False, False) == 128).all() and (ae.intra_chroma(F, 16, 16, 0, False, False) == 128).all()


def test_weight_forms_on_flat_fields():
    """8-273 on flat u, v is (u + v + 1) >> 1; the implicit case's pictures hit w1 inside and outside -64 .. 128 and equal order counts."""
    u, v = np.full((4, 4), 10), np.full((4, 4), 255)
    assert (ae.weighted(u, v, 0, 5, (0, 0), (0, 0)) == 133).all()
    assert (ae.weighted(u, None, 1, 0, (3, -100), None) == 0).all() and (ae.weighted(v, None, 1, 1, (3, -100), None) == 255).all()
    assert ae.implicit_weights(4, 0, 16) == (48, 16) and ae.implicit_weights(20, 16, 0) == (80, -16) and ae.implicit_weights(20, 0, 16) == (-16, 80)
    assert ae.implicit_weights(60, 16, 0) == (32, 32) and ae.implicit_weights(60, 0, 16) == (32, 32) and ae.implicit_weights(8, 16, 16) == (32, 32)
    seq, pics = ac.H264_CASES["implicit_weights_b"](96, 80)
    seen = set()
    for p in pics:
        for m in p["mbs"]:
            if p["kind"] == "B" and m.get("l0") and m.get("l1"):
                p0, p1 = pics[m["l0"][0]]["poc"], pics[m["l1"][0]]["poc"]
                tb, td = p["poc"] - p0, p1 - p0
                w1 = None if td == 0 else max(-1024, min(1023, (tb * int((16384 + abs(int(td / 2))) / td) + 32) >> 6)) >> 2
                seen.add("equal" if w1 is None else ("outside" if w1 < -64 or w1 > 128 else ("inside" if w1 != 32 else "half")))
    assert {"equal", "outside", "inside"} <= seen, seen


def test_ramp_case_closed_form_covers_80_percent_and_equals_the_literal_restatement():
    for (w, h) in ac.SIZES:
        seq, pics = ac.H264_CASES["fractional_positions_ramps"](w, h)
        planes = ae.expect_h264(seq, pics)
        params = {k: ac.RAMP_PARAMS[k] for k in range(3)}
        fracs_y, fracs_c = set(), set()
        for k, p in enumerate(pics):
            if k < 3:
                continue
            assert all(abs(m["l0"][1][0]) <= 12 and abs(m["l0"][1][1]) <= 12 for m in p["mbs"])      # within +-3 samples
            Y, Cb, Cr, mY, mC = ae.ramp_closed_frame(seq, p, params)
            assert mY.mean() >= 0.80, (w, h, k, mY.mean())
            assert np.array_equal(Y[mY], planes[k][0][mY]) and np.array_equal(Cb[mC], planes[k][1][mC]) and np.array_equal(Cr[mC], planes[k][2][mC]), (w, h, k)
            fracs_y |= {(m["l0"][1][0] & 3, m["l0"][1][1] & 3) for m in p["mbs"]}
            fracs_c |= {(m["l0"][1][0] & 7, m["l0"][1][1] & 7) for m in p["mbs"]}
        assert len(fracs_y) == 16 and len(fracs_c) == 64


def test_noise_case_visits_every_fractional_position():
    seq, pics = ac.H264_CASES["fractional_positions_noise"](96, 80)
    mvs = [m["l0"][1] for p in pics[1:] for m in p["mbs"]]
    assert len({(x & 3, y & 3) for x, y in mvs}) == 16 and len({(x & 7, y & 7) for x, y in mvs}) == 64
    assert len(set(mvs)) == len(mvs) and any(abs(x) > 800 or abs(y) > 800 for x, y in mvs)


# ---- deblocking where it filters: the restatement's own pins, and the conditions that keep the filtering cases from passing vacuously ---------------
@functools.lru_cache(maxsize=None)
def filter_case(name, size):
    """(seq, pics, expected planes, counters of deblock_ref, the pictures before 8.7) of a deblock_filters_* case: computed once, never modified"""
    seq, pics = ac.H264_CASES[name](*size)
    stats, raw = {}, []
    planes = ae.expect_h264(seq, pics, stats, raw)
    return seq, pics, planes, stats, raw


def test_dc_only_residual_and_bs_of_vector_pairs_worked_by_hand():
    # 8.5.12.1: qP 16: (-1 * 16 * 16 + 2) >> 2 = -64, (-64 + 32) >> 6 = -1;  qP 30: (16 * 10) << 1 = 320, 352 >> 6 = 5;  qP 51: (16 * 14) << 4 = 3584, 3616 >> 6 = 56
    # qP 23: (16 * 18 + 1) >> 1 = 144, 176 >> 6 = 2;  qP 24, level -1: -160 << 0, -128 >> 6 = -2
    assert [ae.dc_only_residual(q, s) for q, s in ((16, -1), (16, 1), (30, 1), (51, 1), (51, -1), (23, 1), (24, -1))] == [-1, 1, 5, 56, -56, 2, -2]
    A, B, C = (4, -8), (-16, 20), (7, -8)
    bs = deblock_ref.motion_bs
    assert bs([(0, A)], [(0, C)]) == 0 and bs([(0, A)], [(0, (8, -8))]) == 1 and bs([(0, A)], [(1, A)]) == 1            # |4 - 7| = 3; |4 - 8| = 4; pictures
    assert bs([(0, A)], [(0, A), (1, B)]) == 1                                                                          # number of vectors
    assert bs([(0, A), (1, B)], [(1, B), (0, A)]) == 0 and bs([(0, A), (1, B)], [(1, B), (0, (8, -8))]) == 1            # crosswise equal; same pictures, far vector
    assert bs([(0, A), (0, B)], [(0, B), (0, A)]) == 0 and bs([(0, A), (0, B)], [(0, A), (0, A)]) == 1                  # one picture twice: both pairings tried
    assert bs([(0, A), (0, B)], [(0, A), (1, B)]) == 1                                                                  # {0, 0} against {0, 1}


REQUIRED_PER_DIRECTION = (
    ["Y%s:on_bS1", "Y%s:on_bS2", "Y%s:on_bS3", "Y%s:on_bS4", "Y%s:off_alpha_only", "Y%s:off_beta_p_only", "Y%s:off_beta_q_only", "Y%s:ap0_aq0", "Y%s:ap0_aq1",
     "Y%s:ap1_aq0", "Y%s:ap1_aq1", "Y%s:delta_clip_pos", "Y%s:delta_clip_neg", "Y%s:delta_unclipped", "Y%s:clip1_at_0", "Y%s:clip1_at_255", "Y%s:strong_both",
     "Y%s:strong_p", "Y%s:strong_q", "Y%s:strong_neither", "C%s:on_lt4", "C%s:on_4", "C%s:off_lt4", "C%s:off_4", "%s:indexA_clipped_at_0",
     "%s:indexB_clipped_at_0", "%s:indexA_clipped_at_51", "%s:indexB_clipped_at_51", "%s:qPav_of_unequal_QPs", "%s:qPav_of_I_PCM_and_51",
     "%s:chroma_qp_from_table_with_offset", "%s:idc2_slice_edge_left_alone", "%s:idc0_slice_edge_filtered_with_q_offsets",
     "%s:mb_edge_vectors_differ_by_3_bS0", "%s:mb_edge_vectors_differ_by_4_bS1"])


@pytest.mark.parametrize("size", ac.SIZES_FILTER, ids=lambda s: "%dx%d" % s)
def test_filter_cases_take_every_path_of_the_clause_in_both_directions(size):
    """Conditions, not measurements: over the five deblock_filters_* cases at this size, the restatement's own counters show every path of 8.7.2 taken by
    at least one line across a vertical edge and one across a horizontal edge (luma_mb moves data differently for the two); every picture has a changed
    sample in at least half of its macroblocks; and in deblock_filters_refs every P picture differs from what it would be had its reference been read
    before that reference was filtered."""
    total = {}
    for name in ac.H264_FILTER_CASES:
        seq, pics, planes, stats, raw = filter_case(name, size)
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
        mbw, mbh = ac.dims(*size)
        for k, (o, r) in enumerate(zip(planes, raw)):
            changed = np.zeros((mbh, mbw), bool)
            for c, s in ((0, 16), (1, 8), (2, 8)):
                changed |= (o[c] != r[c]).reshape(mbh, s, mbw, s).any(axis=(1, 3))
            assert changed.mean() >= 0.5, f"{name} {size} picture {k}: the filter changes {changed.mean():.2f} of the macroblocks"
    missed = [key % d for d in "VH" for key in REQUIRED_PER_DIRECTION if total.get(key % d, 0) == 0]
    assert not missed, f"{size}: paths of 8.7 that no filtering case takes: {missed}"
    seq, pics, planes, stats, raw = filter_case("deblock_filters_refs", size)
    assert [p["kind"] for p in pics] == ["I", "P", "P", "P", "P"]
    for k in range(1, 5):
        assert all(m["l0"][0] == k - 1 for m in pics[k]["mbs"])
        stale = ae.expect_h264(seq, pics[:k + 1], stale_ref_of=k)[k]
        assert any(not np.array_equal(a, b) for a, b in zip(stale, planes[k])), f"{size} picture {k}: reading the unfiltered reference would not show"


# ---- 2. / 3. the streams through the CPU oracle and the host parser -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_scripted_stream_writer_is_deterministic(name, size):
    a = sw.write(*ac.H264_CASES[name](*size))
    assert a == sw.write(*ac.H264_CASES[name](*size)) and a[:5] == b"\x00\x00\x00\x01\x67"


@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_oracle_decodes_the_analytic_expectation(oracle, name, size):
    seq, pics = ac.H264_CASES[name](*size)
    data = sw.write(seq, pics)
    planes = filter_case(name, size)[2] if name in ac.H264_FILTER_CASES else ae.expect_h264(seq, pics)
    for fmt in (1, 0):
        got, n, w, h = oracle.decode(data, fmt)
        assert (n, w, h) == (len(pics), size[0], size[1])
        fs = w * h * 3 // 2
        diff = ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], fmt, planes)
        assert diff is None, f"{name} {size} format {fmt}: {diff}"


@pytest.mark.parametrize("name", ac.H264_INTER_CASES)
def test_oracle_decodes_the_inter_cases_with_the_filter_on_at_low_qp(oracle, name):
    """analytic_cases.with_filter_on: the variants the GPU test feeds through chain launches (which need the deblocking stage) -- the same pictures."""
    seq, pics = ac.H264_CASES[name](96, 80)
    on = ac.with_filter_on(pics)
    data = sw.write(seq, on)
    assert data != sw.write(seq, pics)
    got, n, w, h = oracle.decode(data, 1)
    fs = w * h * 3 // 2
    diff = ae.first_difference(seq, on, [got[i * fs:(i + 1) * fs] for i in range(n)], 1, ae.expect_h264(seq, pics))
    assert diff is None, f"{name}: {diff}"


def parse_only(data, codec=0):
    with api.JmAmdDec(codec, 1, options={"parse_only": 1}) as d:
        try:
            n = d.decode_stream(data, keep=False)
            failed = None
        except RuntimeError as e:
            n, failed = None, str(e)
        return n, d.stat("errors"), api.jm_nvdec_stream_info(d.h), api.lib().jm_amddec_last_error(d.h).decode(), failed


@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_host_parser_accepts_the_scripted_stream(name, size):
    seq, pics = ac.H264_CASES[name](*size)
    n, errors, info, err, failed = parse_only(sw.write(seq, pics))
    assert failed is None and errors == 0 and err == "", (failed, errors, err)
    assert n == len(pics) and info == size


# ---- the slice limit of the job list ------------------------------------------------------------------------------------------------------------
def one_slice_per_mb_stream(w, h):
    """An I_PCM noise picture and a P picture with one slice per macroblock (integer vectors)."""
    rng = np.random.default_rng(0xA120 + w)
    mbw, mbh = ac.dims(w, h)
    pics = [ac.noise_pic(rng, mbw, mbh),
            ac.p_pic(2, [ac.l0(0, 4 * int(rng.integers(-20, 20)), 4 * int(rng.integers(-20, 20))) for _ in range(mbw * mbh)], is_ref=False)]
    return dict(width=w, height=h), pics


def test_255_slices_per_picture_decode_and_256_are_refused_loudly(oracle):
    """The job list numbers a picture's slices with eight bits: 255 slices (272x240, one per macroblock) decode; the 256th slice of a picture (256x256)
    fails the handle with a text that names the limit -- no frame with undecoded macroblocks is handed out, nothing is dropped in silence.  The oracle
    has no such limit and shows that both streams are what the script says."""
    seq, pics = one_slice_per_mb_stream(272, 240)
    data = sw.write(seq, pics)
    got, n, w, h = oracle.decode(data, 1)
    fs = w * h * 3 // 2
    assert ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], 1) is None
    n, errors, info, err, failed = parse_only(data)
    assert (n, errors, info, failed) == (2, 0, (272, 240), None)
    seq, pics = one_slice_per_mb_stream(256, 256)
    data = sw.write(seq, pics)
    got, n, w, h = oracle.decode(data, 1)
    fs = w * h * 3 // 2
    assert ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], 1) is None
    n, errors, info, err, failed = parse_only(data)
    assert failed is not None and "255 slices" in failed and "255 slices" in err and errors >= 1, (n, errors, err, failed)


# ---- pictures taller than the banded kernels -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tall_script():
    seq, pics = ac.tall_filter_script()
    return seq, pics, sw.write(seq, pics), ae.expect_h264(seq, pics)


def test_tall_picture_decodes_on_the_cpu_and_one_beyond_the_limit_is_refused_loudly(oracle):
    """16x8208 is 1 x 513 macroblocks: above the 512 rows of the banded kernels the GPU decoder runs k_deblock and k_recon_intra, which keep a progress
    word per macroblock row in LDS -- kMaxMbRows = 1056 of them (kernels.h).  The CPU oracle decodes the script to the numpy expectation (the GPU test
    compares the same script).  A frame of 1058 rows (the next height a stream can have past 1056: frame_mbs_only_flag = 0 counts field rows) fails a
    parse_only handle at activation with a text that names the limit; 1056 rows are accepted."""
    seq, pics, data, planes = tall_script()
    assert ac.dims(seq["width"], seq["height"]) == (1, 513)
    got, n, w, h = oracle.decode(data, 1)
    fs = w * h * 3 // 2
    diff = ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], 1, planes)
    assert (n, w, h) == (4, 16, 8208) and diff is None, diff
    raw = []
    ae.expect_h264(seq, pics[:1], None, raw)
    assert not np.array_equal(raw[0][0], planes[0][0])              # it filters
    n, errors, info, err, failed = parse_only(data)
    assert (n, errors, info, failed, err) == (4, 0, (16, 8208), None, "")
    n, errors, info, err, failed = parse_only(sw.write(*ac.too_tall_stream(1058)))
    assert failed is not None and "1056 macroblock rows" in failed and "1056 macroblock rows" in err and errors >= 1, (n, errors, err, failed)
    n, errors, info, err, failed = parse_only(sw.write(*ac.too_tall_stream(1056)))
    assert (n, errors, info, failed, err) == (1, 0, (16, 16896), None, "")


# ---- H.265 -------------------------------------------------------------------------------------------------------------------------------------
import analytic_hevc as ah          # noqa: E402
import scripted_hevc as hw          # noqa: E402
from test_hevc_mc_packed import chroma_literal as hevc_chroma_literal, luma_literal as hevc_luma_literal          # noqa: E402
from tools import streams           # noqa: E402

HCASES = [(n, s) for n in sorted(ah.HEVC_CASES) for s in ah.SIZES]
HIDS = [f"{n}-{s[0]}x{s[1]}" for n, s in HCASES]


@pytest.fixture(scope="module")
def oracle_hevc():
    return streams.OracleHevc()


def test_hevc_vectorised_interpolation_is_the_literal_restatement():
    rng = np.random.default_rng(0xB001)
    R = rng.integers(0, 256, (40, 48), dtype=np.uint8)
    pad = 64
    Rp = padded(R, pad)
    for trial in range(96):
        chroma = trial % 2 == 1
        sh = 3 if chroma else 2
        mv = ((int(rng.integers(-40, 40)) << sh) + (trial // 2) % (1 << sh), (int(rng.integers(-40, 40)) << sh) + (trial // (2 << sh)) % (1 << sh))
        x0, y0 = int(rng.integers(0, 33)), int(rng.integers(0, 25))
        got = ah.mc14(R, x0, y0, 16, 16, mv, chroma)
        lit = hevc_chroma_literal if chroma else hevc_luma_literal
        xi, yi = x0 + (mv[0] >> sh), y0 + (mv[1] >> sh)
        for (dy, dx) in [(0, 0), (15, 15), (0, 15), (15, 0), (int(rng.integers(0, 16)), int(rng.integers(0, 16)))]:
            assert got[dy, dx] == lit(Rp, xi + dx + pad, yi + dy + pad, mv[0] & ((1 << sh) - 1), mv[1] & ((1 << sh) - 1)), (trial, mv, x0, y0, dx, dy)


def test_hevc_ramp_closed_form_against_the_literal_restatement():
    """analytic_hevc's module docstring derives sample = f + ((a Mx + c My + 32) >> 6); here against luma_literal / chroma_literal of
    tests/test_hevc_mc_packed.py, slopes -2 .. 2, every fraction."""
    assert ah.M_LUMA == [0, 15, 32, 49] and ah.M_CHROMA == [0, 8, 16, 26, 32, 38, 48, 56]
    rng = np.random.default_rng(0xB002)
    clip = lambda v: max(0, min(255, v))
    for a in range(-2, 3):
        for c in range(-2, 3):
            lo, hi = -min(0, a * 23) - min(0, c * 19), 255 - max(0, a * 23) - max(0, c * 19)
            R = ae.ramp(20, 24, a, c, int(rng.integers(lo, hi + 1)))
            for fy in range(8):
                for fx in range(8):
                    x, y = int(rng.integers(3, 20)), int(rng.integers(3, 16))
                    if fx < 4 and fy < 4:
                        assert ah.ramp_closed(int(R[y, x]), a, c, fx, fy, False) == clip((hevc_luma_literal(R, x, y, fx, fy) + 32) >> 6), (a, c, fx, fy, x, y)
                    assert ah.ramp_closed(int(R[y, x]), a, c, fx, fy, True) == clip((hevc_chroma_literal(R, x, y, fx, fy) + 32) >> 6), (a, c, fx, fy, x, y)


def test_hevc_ramp_case_closed_form_share_and_flat_weight_forms():
    for (w, h) in ah.SIZES:
        seq, pics = ah.HEVC_CASES["fractional_positions_ramps"](w, h)
        planes = ah.expect_hevc(seq, pics)
        fr_y, fr_c = set(), set()
        for k, p in enumerate(pics[3:], 3):
            Y, Cb, Cr, mY, mC = ah.ramp_closed_frame(seq, p, {i: ah.RAMP_PARAMS[i] for i in range(3)})
            assert mY.mean() >= 0.80, (w, h, k, mY.mean())
            assert np.array_equal(Y[mY], planes[k][0][mY]) and np.array_equal(Cb[mC], planes[k][1][mC]) and np.array_equal(Cr[mC], planes[k][2][mC]), (w, h, k)
            fr_y |= {(u["l0"][1][0] & 3, u["l0"][1][1] & 3) for u in p["cus"]}
            fr_c |= {(u["l0"][1][0] & 7, u["l0"][1][1] & 7) for u in p["cus"]}
        assert len(fr_y) == 16 and len(fr_c) == 64
    # flat fields: default bi-prediction of u and v is (64 u + 64 v + 64) >> 7 = (u + v + 1) >> 1; a skipped unit over a flat reference is that value
    u, v = np.full((2, 2), 10 << 6), np.full((2, 2), 255 << 6)
    assert (ah.weighted(u, v, False, 0, None, None) == 133).all() and (ah.weighted(u, None, False, 0, None, None) == 10).all()
    seq, pics = ah.HEVC_CASES["fractional_positions_noise"](96, 80)
    mvs = [c["l0"][1] for p in pics[1:] for c in p["cus"]]
    assert len({(x & 3, y & 3) for x, y in mvs}) == 16 and len({(x & 7, y & 7) for x, y in mvs}) == 64


@pytest.mark.parametrize("name,size", HCASES, ids=HIDS)
def test_hevc_oracle_decodes_the_analytic_expectation(oracle_hevc, name, size):
    seq, pics = ah.HEVC_CASES[name](*size)
    data = hw.write(seq, pics)
    assert data == hw.write(*ah.HEVC_CASES[name](*size)), "the writer is deterministic"
    planes = ah.expect_hevc(seq, pics)
    for fmt in (1, 0):
        got, n, w, h = oracle_hevc.decode(data, fmt)
        assert (n, w, h) == (len(pics), size[0], size[1])
        fs = w * h * 3 // 2
        diff = ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], fmt, planes, "cus")
        assert diff is None, f"{name} {size} format {fmt}: {diff}"


@pytest.mark.parametrize("name,size", HCASES, ids=HIDS)
def test_hevc_host_parser_accepts_the_scripted_stream(name, size):
    seq, pics = ah.HEVC_CASES[name](*size)
    n, errors, info, err, failed = parse_only(hw.write(seq, pics), codec=1)
    assert failed is None and errors == 0 and err == "", (failed, errors, err)
    assert n == len(pics) and info == size


def test_hevc_one_slice_per_ctb_of_272_ctbs(oracle_hevc):
    """272x256 with 16x16 CTBs and one slice per CTB: 272 slice segments in a picture -- more than the 255 the H.264 job list can number; the H.265
    path numbers them with 16 bits and refuses only beyond 600, the most any level allows (Table A.8).  Both decoders take the stream."""
    seq, pics = ah.one_slice_per_ctb_stream(272, 256)
    data = hw.write(seq, pics)
    got, n, w, h = oracle_hevc.decode(data, 1)
    fs = w * h * 3 // 2
    assert ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], 1, ah.expect_hevc(seq, pics), "cus") is None
    n, errors, info, err, failed = parse_only(data, codec=1)
    assert (n, errors, info, failed, err) == (2, 0, (272, 256), None, "")


def test_hevc_more_than_600_slice_segments_are_refused_loudly():
    """416x400 with one slice per CTB has 650 slice segments in a picture, beyond what any level allows (600, Table A.8): not a conforming stream at any
    level, so nothing has to decode it -- but the product fails the handle at the 601st segment with a text that names the limit instead of handing out
    a picture that is decoded in part (the oracle refuses the stream as well)."""
    seq, pics = ah.one_slice_per_ctb_stream(416, 400)
    n, errors, info, err, failed = parse_only(hw.write(seq, pics), codec=1)
    assert failed is not None and "600 slice segments" in failed and "600 slice segments" in err and errors >= 1, (n, errors, err, failed)
