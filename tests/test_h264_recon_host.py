"""H.264 intra prediction (8.3.1, 8.3.2) and residual reconstruction (8.5) pinned to the clauses, on the CPU.

The scripted cases of tests/analytic_h264_recon.py carry Intra4x4 / Intra8x8 macroblocks and coded residuals in every macroblock kind; their expected
pictures come from the restatement tests/h264_recon_ref.py, computed from the script alone.  Here:
  1. hand-worked values typed into the test pin the restatement itself;
  2. every case's expectation equals the CPU oracle's pictures bit for bit (I420 and NV12), and a parse_only product handle accepts every stream and
     counts the intra macroblocks and stored coefficients that the script implies;
  3. every wrong-on-purpose switch of the restatement changes the expected picture of the case named beside it -- so a decoder wrong in that way
     fails that case;
  4. every case covers what it is there for: asserted from the restatement's and the writer's counters and from the scripts.
The GPU half is tests/test_h264_recon_gpu.py."""
import numpy as np
import pytest

import analytic_expect as ae
import analytic_h264_recon as hr
import h264_recon_ref as rr
import scripted_h264 as sw
from jmcodec_amd import api
from spec_tables_h264 import DEFAULT_4x4_INTER, DEFAULT_4x4_INTRA, DEFAULT_8x8_INTER, DEFAULT_8x8_INTRA, ZIGZAG_4x4, ZIGZAG_8x8

CASES = [(n, s) for n in sorted(hr.CASES) for s in hr.case_sizes(n)]
IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]


# ---- 1. worked by hand ---------------------------------------------------------------------------------------------------------------------------
def test_one_4x4_block_of_8_5_12_by_hand():
    """qP 28 (qP % 6 = 4, qP / 6 = 4: no shift), flat lists: LevelScale(0, 0) = 16 * 16 = 256, LevelScale(0, 1) = 16 * 20 = 320.  c00 = 2, c01 = 1:
    d00 = 512, d01 = 320.  Row 0: e = (512, 512, 160, 320), f = (832, 672, 352, 192); the other rows are 0.  Every column holds its f in row 0 only:
    e0 = e1 = f, e2 = e3 = 0, so all four rows equal row 0.  r = (h + 32) >> 6 = (13, 11, 6, 3) in every row."""
    m = dict(t="16x16", l0=(0, (0, 0)), coef=dict(y={0: [2, 1] + [0] * 14}))
    R = rr.mb_residual(dict(width=16, height=16), m, 28)
    assert R[0][0:4, 0:4].tolist() == [[13, 11, 6, 3]] * 4 and not R[0][4:].any() and not R[0][:, 4:].any() and not R[1].any() and not R[2].any()
    # the same levels transposed (c10 = 1): the answer is transposed -- rows and columns are told apart
    m = dict(t="16x16", l0=(0, (0, 0)), coef=dict(y={0: [2, 0, 0, 0, 1] + [0] * 11}))
    assert rr.mb_residual(dict(width=16, height=16), m, 28)[0][0:4, 0:4].T.tolist() == [[13, 11, 6, 3]] * 4
    # qP 22 (m = 4, qP / 6 = 3): d = (c * LevelScale + 1) >> 1 = 256, 160: half of the above: f = (416, 336, 176, 96): r = (7, 5, 3, 2)
    m = dict(t="16x16", l0=(0, (0, 0)), coef=dict(y={0: [2, 1] + [0] * 14}))
    assert rr.mb_residual(dict(width=16, height=16), m, 22)[0][0, 0:4].tolist() == [7, 5, 3, 2]


def test_one_intra16x16_dc_matrix_by_hand():
    """c00 = 3, c01 = -1: A c has [3, -1, 0, 0] in every row; times A: 3 * (1, 1, 1, 1) - (1, 1, -1, -1) = (2, 2, 4, 4) in every row.  qP 40 (m = 4,
    qP / 6 = 6): dcY = f * 256; qP 30 (m = 0: LevelScale 160, qP / 6 = 5): (f * 160 + 1) >> 1 = (160, 160, 320, 320)."""
    c = [[3, -1, 0, 0]] + [[0] * 4] * 3
    assert rr.intra16_dc(c, 256, 40).tolist() == [[512, 512, 1024, 1024]] * 4
    assert rr.intra16_dc(c, 160, 30).tolist() == [[160, 160, 320, 320]] * 4
    assert rr.intra16_dc(c, 160, 36).tolist() == [[320, 320, 640, 640]] * 4 and rr.intra16_dc(c, 288, 35).tolist() == [[288, 288, 576, 576]] * 4


def test_chroma_dc_at_qpc_0_and_39_by_hand():
    """c = [[3, 0], [0, 0]]: f = 3 everywhere.  QPc 0: LevelScale(0, 0, 0) = 160: ((3 * 160) << 0) >> 5 = 15.  QPc 39 (m = 3: 16 * 14 = 224, QPc / 6 = 6):
    ((3 * 224) << 6) >> 5 = 1344.  c = [[1, -1], [0, 0]]: f = [[0, 2], [0, 2]]; QPc 1 (LevelScale 176): (2 * 176) >> 5 = 11."""
    assert rr.chroma_dc([3, 0, 0, 0], 160, 0).tolist() == [[15, 15], [15, 15]]
    assert rr.chroma_dc([3, 0, 0, 0], 224, 39).tolist() == [[1344, 1344], [1344, 1344]]
    assert rr.chroma_dc([1, -1, 0, 0], 176, 1).tolist() == [[0, 11], [0, 11]]
    assert [rr.qp_chroma(q, o) for q, o in ((20, -12), (5, -12), (29, 0), (30, 0), (39, 12), (51, 12), (45, 0))] == [8, 0, 29, 29, 39, 39, 38]


def test_one_levelscale8x8_entry_per_class_by_hand():
    """8.5.9 with Flat_8x8_16 at qP % 6 = 0: 16 * (20, 18, 32, 19, 25, 24) by position class"""
    ls = 16 * rr.norm_adjust8(0)
    by_class = {320: [(0, 0), (4, 4), (0, 4)], 288: [(1, 1), (3, 5), (7, 7)], 512: [(2, 2), (6, 2)], 304: [(0, 1), (4, 3), (1, 4), (7, 0)],
                400: [(0, 2), (4, 6), (2, 4)], 384: [(1, 2), (2, 3), (1, 6), (6, 5)]}
    for v, where in by_class.items():
        assert all(ls[i, j] == v for i, j in where), (v, where)
    assert (16 * rr.norm_adjust4(5)).tolist() == [[288, 368, 288, 368], [368, 464, 368, 464]] * 2


def test_scaling_list_fall_back_rules():
    """Table 7-2 on the three scaling_lists_* scripts: which list each of the eight matrices really is"""
    mat = lambda v, n, zz: np.array([v[zz.index(i)] for i in range(n * n)]).reshape(n, n)
    d4i, d4p = mat(DEFAULT_4x4_INTRA, 4, ZIGZAG_4x4), mat(DEFAULT_4x4_INTER, 4, ZIGZAG_4x4)
    d8i, d8p = mat(DEFAULT_8x8_INTRA, 8, ZIGZAG_8x8), mat(DEFAULT_8x8_INTER, 8, ZIGZAG_8x8)
    eq = np.array_equal
    s = rr.scaling_matrices(hr.scripted("scaling_lists_sps")[0])
    assert s[0][0, 1] == 71 and s[0][1, 0] == 9 and s[6][0, 1] == 71 and s[6][1, 0] == 9 and s[0][0, 0] != 16
    assert eq(s[1], s[0]) and eq(s[2], d4i) and eq(s[3], d4p) and eq(s[5], s[4]) and not eq(s[4], s[3]) and eq(s[7], d8p) and not eq(s[6], d8i)
    seq = hr.scripted("scaling_lists_pps_over_sps")[0]
    b, s = rr.scaling_matrices(seq), rr.scaling_matrices({k: v for k, v in seq.items() if k != "pps_lists"})       # s: what the SPS alone gives
    assert eq(b[0], s[0]) and eq(b[6], s[6]) and not eq(b[1], b[0]) and eq(b[2], b[1]) and eq(b[3], d4p) and eq(b[4], d4p) and not eq(b[5], b[4])
    assert not eq(b[7], s[7]) and b[7][0, 1] == 71
    o = rr.scaling_matrices(hr.scripted("scaling_lists_pps_only")[0])
    assert eq(o[0], d4i) and eq(o[1], d4i) and not eq(o[2], o[1]) and eq(o[3], d4p) and not eq(o[4], o[3]) and eq(o[5], o[4]) and eq(o[6], d8i) and eq(o[7], d8p)
    flat = rr.scaling_matrices(dict(width=16, height=16))
    assert all((m == 16).all() for m in flat)


def test_the_nine_modes_on_a_ramp_and_the_substitution():
    """On neighbours that continue one ramp p(x, y) = 100 + 8 x + 4 y nothing tells the three-tap means from the samples: Diagonal_Down_Left of a 4x4 block
    gives p(x + y + 1, -1) but for the last sample, whose taps are (1, 3): (p(6, -1) + 3 p(7, -1) + 2) >> 2 = p(7, -1) - 2.  Without the upper right
    block, p(3, -1) fills positions 4 .. 7: the same block ends in p(3, -1) from x + y = 3 on (and (p(2, -1) + 3 p(3, -1) + 2) >> 2 at x + y = 2)."""
    p = lambda x, y: 100 + 8 * x + 4 * y
    Y = np.array([[p(x - 1, y - 1) for x in range(18)] for y in range(18)], np.int64)           # the macroblock starts at (1, 1)
    P, pat = rr.neighbours(Y, Y, 1, 1, 0, 0, 4, 0, lambda dx, dy: True)
    assert pat == "TLCR"
    got = rr.predict(P, 4, 3)
    assert all(got[y, x] == p(x + y + 1, -1) for y in range(4) for x in range(4) if (x, y) != (3, 3)) and got[3, 3] == p(7, -1) - 2
    P, pat = rr.neighbours(Y, Y, 1, 1, 0, 0, 4, 0, lambda dx, dy: (dx, dy) != (1, -1))
    assert pat == "TLCR"                                                                      # block 0's upper right is the macroblock ABOVE
    P, pat = rr.neighbours(Y, Y, 1, 1, 12, 0, 4, 5, lambda dx, dy: (dx, dy) != (1, -1))       # block 5's is the macroblock above and to the right
    assert pat == "TLC" and [P[(x, -1)] for x in range(4, 8)] == [p(15, -1)] * 4
    got = rr.predict(P, 4, 3)
    assert got[0, 0] == p(13, -1) and got[1, 1] == (p(14, -1) + 3 * p(15, -1) + 2) >> 2 and all(got[y, x] == p(15, -1) for y in range(4) for x in range(4)
                                                                                                if x + y >= 3)
    for idx, has in ((1, True), (2, True), (3, False), (4, True), (6, True), (7, False), (11, False), (13, False), (15, False), (12, True), (14, True)):
        bx, by = rr.blk_xy(idx)
        assert ("R" in rr.pattern(bx, by, 4, idx, lambda dx, dy: True)) == has, idx
    # Vertical / Horizontal / DC of an 8x8 block read the FILTERED neighbours: on a ramp the inner ones are unchanged, the ends are not
    P, pat = rr.neighbours(Y, Y, 1, 1, 0, 0, 8, 0, lambda dx, dy: True)
    F = rr.filter_reference(P)
    assert all(F[(x, -1)] == p(x, -1) for x in range(0, 15)) and F[(15, -1)] == p(15, -1) - 2 and F[(-1, 7)] == p(-1, 7) - 1 and F[(-1, -1)] == p(-1, -1) + 3
    assert (rr.predict(F, 8, 0) == np.array([p(x, -1) for x in range(8)])).all() and (rr.predict(F, 8, 1)[:, 0] == [p(-1, y) - (y == 7) for y in range(8)]).all()


# ---- 2. the oracle and the host parser -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_oracle_decodes_the_restated_expectation(oracle, name, size):
    seq, pics, data, planes, _ = hr.scripted(name, size)
    assert data == sw.write(*hr.CASES[name](*size)), "the case builder and the writer are deterministic"
    for fmt in (1, 0):
        got, n, w, h = oracle.decode(data, fmt)
        assert (n, w, h) == (len(pics), size[0], size[1])
        fs = w * h * 3 // 2
        diff = ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], fmt, planes)
        assert diff is None, f"{name} {size} format {fmt}: {diff}"


@pytest.mark.parametrize("name", hr.ROUTE_CASES)
def test_oracle_decodes_the_cases_with_deblocking_on(oracle, name):
    """The variants the GPU test feeds through chain launches: tests/deblock_ref.py with the coded blocks of the script, transform_size_8x8_flag and each
    chroma plane's own offset; the filter changes every picture that has an intra macroblock or a coded block (below indexA 16 alpha is 0: the QPY 6
    pictures of transform_8x8 are evaluated and left alone)."""
    seq, pics, data, planes, stats = hr.scripted_deblocked(name)
    raw = hr.scripted(name)[3]
    assert all(any(not np.array_equal(a, b) for a, b in zip(P, Q)) for P, Q, p in zip(planes, raw, pics)
               if p["qp"] >= 20 and any(m["t"] != "pcm" for m in p["mbs"]))
    assert stats.get("YV:on_bS2", 0) + stats.get("YH:on_bS2", 0) > 0 or name not in hr.P_CASES
    got, n, w, h = oracle.decode(data, 1)
    fs = w * h * 3 // 2
    diff = ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], 1, planes)
    assert n == len(pics) and diff is None, f"{name}: {diff}"


def test_oracle_decodes_the_tall_intra4x4_picture(oracle):
    seq, pics, data, planes = hr.tall_intra_script()
    got, n, w, h = oracle.decode(data, 1)
    assert (n, w, h) == (1, 16, 8208) and ae.first_difference(seq, pics, [got], 1, planes) is None


def stored_coefficients(m):
    """int16 slots the job list holds for macroblock m: 192 for the samples of I_PCM; else 16 for the Intra16x16 DC block (always), 16 per luma 4x4 block
    with a level (64 per 8x8 with one under the 8x8 transform), 4 per chroma plane with a DC level, 16 per chroma block with an AC level"""
    if m["t"] == "pcm":
        return 192
    if "resid" in m:
        return 16
    if m["t"] == "skip" or ("coef" not in m and m["t"] != "i16"):
        return 0
    lv = sw.mb_levels(m)
    n = 16 if m["t"] == "i16" else 0
    if lv["t8"]:
        n += 64 * sum(any(any(lv["y"][4 * b8 + i]) for i in range(4)) for b8 in range(4))
    else:
        n += 16 * sum(any(q) for q in lv["y"])
    return n + 4 * sum(any(q) for q in lv["cdc"]) + 16 * sum(any(q) for pl in lv["cac"] for q in pl)


@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_host_parser_accepts_the_stream_and_counts_what_the_script_implies(name, size):
    seq, pics, data, _, _ = hr.scripted(name, size)
    with api.JmAmdDec(0, 1, options={"parse_only": 1}) as d:
        n = d.decode_stream(data, keep=False)
        assert d.stat("errors") == 0 and api.lib().jm_amddec_last_error(d.h).decode() == ""
        assert n == len(pics) and api.jm_nvdec_stream_info(d.h) == size
        assert d.stat("intra_mbs") == sum(i for i, _ in hr.intra_counts(seq, pics))
        assert d.stat("coef_int16") == sum(stored_coefficients(m) for p in pics for m in p["mbs"])


@pytest.mark.parametrize("name", sorted(hr.CASES))
def test_writer_codes_the_modes_that_the_restated_clause_predicts(name):
    """prev_intraNxN_pred_mode_flag / rem_intraNxN_pred_mode as the writer's own derivation wrote them == 8.3.1.1 / 8.3.2.1 typed literally"""
    seq, pics, _, _, _ = hr.scripted(name)
    coded = {}
    sw.write(seq, pics, None, coded)
    for k, p in enumerate(pics):
        want = rr.mode_tables(seq, p)[0]
        assert {a: v for (kk, a), v in coded.items() if kk == k} == want, (name, k)


# ---- 3. wrong on purpose --------------------------------------------------------------------------------------------------------------------------
NOTICED_BY = {
    "list_transposed": "scaling_lists_sps", "inter_uses_intra_list": "scaling_lists_pps_over_sps", "cr_uses_cb_list": "scaling_lists_sps",
    "norm8_class_3_4_swapped": "transform_8x8", "no_rounding_below_24": "qp_sweep_default_lists", "no_rounding_below_36": "qp_sweep_flat",
    "shift_branch_at_24": "qp_sweep_flat", "shift_branch_at_36": "qp_sweep_flat", "chroma_dc_shift_5_first": "qp_sweep_flat",
    "cr_uses_cb_offset": "qp_sweep_flat", "columns_before_rows_4x4": "qp_sweep_default_lists", "columns_before_rows_8x8": "transform_8x8",
    "i16_dc_without_hadamard": "i16_and_chroma_residual", "i4_left_from_prediction": "i4_modes", "upper_right_of_block_3_available": "i4_modes",
    "upper_right_of_block_5_unavailable": "i4_modes", "no_substitution_of_upper_right": "i4_modes",
    "i8_first_sample_unfiltered_without_corner": "i8_modes", "i8_unfiltered": "i8_modes", "mode_max": "i4_i8_mode_prediction",
    "i8_neighbour_wrong_block": "i4_i8_mode_prediction", "n1_n2_swapped": "i4_i8_mode_prediction",
    "constrained_inter_stored_mode": "i4_i8_mode_prediction_constrained", "rem_without_plus_1": "i4_modes"}


def test_every_switch_has_a_named_case():
    assert set(NOTICED_BY) == set(rr.SWITCHES)


@pytest.mark.parametrize("switch", rr.SWITCHES)
def test_wrong_on_purpose_is_noticed_by_its_named_case(switch):
    """A decoder with this defect computes another picture for the named case (or, for a mode derivation gone wrong, lands on a mode whose neighbours
    do not exist, which the restatement refuses): the case fails on it.  With flat lists the rounding term of 8.5.12.1 never matters (LevelScale is a
    multiple of 16 and the shift at most 4), and the order of the 4x4 passes shows only where d is odd: both need lists, hence qp_sweep_default_lists."""
    name = NOTICED_BY[switch]
    seq, pics, _, planes, _ = hr.scripted(name)
    try:
        wrong = ae.expect_h264(seq, pics, wrong={switch})
    except (AssertionError, KeyError):
        assert switch in rr.MODE_SWITCHES or switch in ("list_transposed",), switch      # only these may leave what a conforming stream can say
        return
    assert any(not np.array_equal(a, b) for P, Q in zip(wrong, planes) for a, b in zip(P, Q)), f"{switch} does not show in {name}"


# ---- 4. the cases cover what they are there for ---------------------------------------------------------------------------------------------------
def missing(cov, wanted):
    return sorted(str(q) for q in wanted if q not in cov)


def test_i4_modes_covers_every_mode_in_every_block_on_every_availability():
    cov = hr.scripted("i4_modes")[4]
    want = [("mode", 4, idx, mode) for idx in range(16) for mode in range(9)] + [("residual", 4, idx) for idx in range(16)]
    want += [("pattern", 4, pat) for pat in ("", "L", "TR", "TLC", "TLCR")]
    # picture corner, top row, left column, right column (no macroblock above and to the right), interior, one slice per macroblock
    want += [("kind", "I", "i4", pat) for pat in ("", "L", "TR", "TLC", "TLCR")]
    # vertical-left / diagonal-down-left in the blocks whose upper right block never exists, and in block 5 with and without macroblock C
    want += [("upper_right_mode", 4, idx, False) for idx in (3, 5, 7, 11, 13, 15)] + [("upper_right_mode", 4, 5, True)]
    assert not missing(cov, want)
    seq, pics = hr.scripted("i4_modes")[:2]
    assert any(p.get("layout") == "mb" for p in pics) and all(len(m["coef"]["y"]) == 16 and all(any(v) for v in m["coef"]["y"].values())
                                                              for p in pics for m in p["mbs"] if m["t"] == "i4")


def test_i8_modes_covers_every_mode_in_every_block_on_every_availability():
    """The patterns of (above, left, corner, upper right) that a frame picture WITHOUT constrained_intra_pred can produce for an 8x8 block: none, left
    only, above with upper right, all but upper right, all.  Corner without left (or without above) needs an inter neighbour under
    constrained_intra_pred_flag: i4_i8_mode_prediction_constrained has them."""
    cov = hr.scripted("i8_modes")[4]
    want = [("mode", 8, idx, mode) for idx in range(4) for mode in range(9)] + [("residual", 8, idx) for idx in range(4)]
    want += [("pattern", 8, pat) for pat in ("", "L", "TR", "TLC", "TLCR")] + [("kind", "I", "i8", pat) for pat in ("", "L", "TR", "TLC", "TLCR")]
    want += [("upper_right_mode", 8, idx, has) for idx, has in ((0, True), (1, True), (1, False), (2, True), (3, False))]
    assert not missing(cov, want)
    assert not missing(hr.scripted("i4_i8_mode_prediction_constrained")[4], [("pattern", 8, "LC"), ("pattern", 8, "C"), ("pattern", 4, "TCR")])


def test_mode_prediction_cases_take_every_path_of_the_derivation():
    for name, inter in (("i4_i8_mode_prediction", "inter"), ("i4_i8_mode_prediction_constrained", "inter_constrained")):
        cov = hr.scripted(name)[4]
        want = [("neighbour", N, t) for N in (4, 8) for t in ("i4", "i8", "i16", "pcm", "unavailable", inter)]
        want += [("coded", N, how) for N in (4, 8) for how in ("predicted", "below", "above")]
        assert not missing(cov, want), name


def test_i16_case_has_every_mode_with_dc_only_ac_only_and_both():
    seq, pics, _, _, cov = hr.scripted("i16_and_chroma_residual")
    i16 = [q for q in cov if q[0] == "i16"]
    for mode in range(4):
        assert {(q[3], q[4]) for q in i16 if q[1] == mode} >= {(True, False), (False, True), (True, True)}, mode
        assert {(q[5], q[6]) for q in i16 if q[2] == mode} >= {(True, False), (False, True), (True, True)}, mode
    single = [m["coef"] for m in pics[-1]["mbs"]]
    assert {c["ydc"].index(v) for c in single for v in c["ydc"] if v} == set(range(16)) and \
        {v > 0 for c in single for v in c["ydc"] if v} == {True, False} and all(sum(1 for v in c["ydc"] if v) == 1 for c in single)
    assert {(pl, c["cdc"][pl].index(v)) for c in single for pl in (0, 1) for v in c["cdc"][pl] if v} == {(pl, i) for pl in (0, 1) for i in range(4)}
    assert not missing(cov, [("residual_sign", "i16", c, True, True) for c in (0, 1, 2)])


def test_qp_sweep_visits_every_qp_both_wraps_and_every_chroma_range():
    ranges = set()
    for name in ("qp_sweep_flat", "qp_sweep_default_lists", "qp_sweep_coded_lists"):
        seq, pics, _, _, cov = hr.scripted(name)
        assert {q[2] for q in cov if q[0] == "qp"} == set(range(52)), name
        assert all({q[2] for q in cov if q[0] == "qp" and q[1] == t} >= {23, 24, 35, 36} for t in ("i4", "i8", "i16")), name
        wraps = set()
        for p in pics:
            qps, pred = sw.mb_qps(seq, p), p["qp"]
            for m, qp in zip(p["mbs"], qps):
                wraps.add("up" if pred + m["dqp"] > 51 else ("down" if pred + m["dqp"] < 0 else "none"))
                for off in (seq["chroma_qp_off"], seq["second_chroma_qp_off"]):
                    ranges.add("below_0" if qp + off < 0 else ("above_51" if qp + off > 51 else ("table" if qp + off >= 30 else "identity")))
                pred = qp
        assert wraps == {"up", "down", "none"}, name
        assert seq["chroma_qp_off"] != seq["second_chroma_qp_off"]
    assert ranges == {"below_0", "above_51", "table", "identity"}
    assert {hr.scripted(n)[0]["chroma_qp_off"] for n in ("qp_sweep_flat", "qp_sweep_default_lists", "qp_sweep_coded_lists")} == {-12, 0, 12}


def test_transform_8x8_case_has_the_single_coefficients_and_the_near_overflow():
    seq, pics, _, _, cov = hr.scripted("transform_8x8")
    spots = {(0, 0), (0, 7), (7, 0), (7, 7), (7, 3), (2, 7), (7, 6), (5, 7)}
    for kind in ("i8", "16x16"):
        blocks = [lv for p in pics for m in p["mbs"] if m["t"] == kind for lv in m["coef"]["y8"].values()]
        singles = {divmod(max(range(64), key=lambda i: abs(lv[i])), 8) for lv in blocks if sum(1 for v in lv if v) == 1}
        assert singles >= spots, (kind, singles)
        assert any(sum(1 for v in lv if v) >= 48 for lv in blocks), kind
        assert {lv[0] for lv in blocks} >= {3276, -3276}, kind
    # what 3276 becomes: within 8 of the 16-bit limit, and inside it
    assert int(rr.scale(np.array([3276]), 320, 6, 36, frozenset())[0]) == 32760
    assert not missing(cov, [("kind", "P", "inter_t8", ""), ("level_prefix", 16, 0)])


def test_cavlc_case_takes_every_path_of_the_level_and_run_coding():
    cov = hr.scripted("cavlc_levels")[4]
    want = [("suffixLength", n) for n in range(7)] + [("level_prefix", 14, 0), ("level_prefix", 15, 0), ("level_prefix", 16, 0)]
    want += [("nC", col) for col in range(5)] + ["minus_2_after_fewer_than_3_trailing_ones", "more_than_10_coefficients_fewer_than_3_trailing_ones",
                                                 "run_before_above_6"]
    assert not missing(cov, want)


def test_level_prefix_16_is_refused_below_profile_100():
    seq, pics = hr.CASES["cavlc_levels"](48, 16)
    with pytest.raises(AssertionError, match="level_prefix 16"):
        sw.write(dict(seq, profile=77), pics)


def touching(intra, mbw):
    out = set()
    for a in intra:
        x = a % mbw
        out |= {name for name, d, ok in (("horizontal", 1, x + 1 < mbw), ("vertical", mbw, True), ("diagonal_down_right", mbw + 1, x + 1 < mbw),
                                         ("diagonal_down_left", mbw - 1, x > 0)) if ok and a + d in intra}
    return out


def test_p_intra_cases_select_the_kernel_they_are_there_for():
    """decoder.cpp:1970: a picture whose intra macroblocks are fewer than 1/16 of all runs k_recon_intra, else k_intra_band"""
    for name in hr.P_CASES:
        for size in hr.case_sizes(name):
            seq, pics, _, _, cov = hr.scripted(name, size)
            mbw = (size[0] + 15) // 16
            touch, kinds = set(), set()
            for p, (n_intra, n_mbs) in list(zip(pics, hr.intra_counts(seq, pics)))[1:]:
                assert n_intra > 0 and ((n_intra * 16 >= n_mbs) if "dense" in name else (n_intra * 16 < n_mbs)), (name, size, n_intra, n_mbs)
                intra = {a for a, m in enumerate(p["mbs"]) if m["t"] in sw.INTRA}
                touch |= touching(intra, mbw)
                kinds |= {m["t"] for m in p["mbs"] if m["t"] in sw.INTRA}
            assert kinds == {"i4", "i8", "i16"}, (name, size)
            if size == (128, 128) or "dense" in name:
                assert touch == {"horizontal", "vertical", "diagonal_down_right", "diagonal_down_left"}, (name, size, touch)
            assert not missing(cov, [("kind", "P", "inter", ""), ("kind", "P", "inter_t8", "")])


def test_clip1_case_clips_at_both_ends_in_every_kind_and_plane():
    cov = hr.scripted("clip1")[4]
    want = [(end, t) for end in ("clip1_at_0", "clip1_at_255") for t in ("i4", "i8")]
    want += [(end, t, c) for end in ("clip1_at_0", "clip1_at_255") for t, cs in (("i16", (0, 1, 2)), ("16x16", (0, 1, 2)), ("i4", (1, 2)), ("i8", (1, 2)))
             for c in cs]
    assert not missing(cov, want) and ("kind", "P", "inter_t8", "") in cov
