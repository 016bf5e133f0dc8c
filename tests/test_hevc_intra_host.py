"""H.265 intra prediction against clause 8.4.4.2 on the CPU: scripted streams (tests/scripted_hevc.py, cases of tests/analytic_hevc_intra.py) whose
expected pictures tests/hevc_intra_ref.py computes from the clauses -- no decoder computed them.

  1. the restatement's own pins: values worked by hand;
  2. the writer: the streams of the earlier HEVC cases still come out byte for byte (tests/golden/scripted_hevc_digests.json), and it is deterministic;
  3. every case through the CPU oracle, I420 and NV12, bit for bit, and through a parse_only product handle;
  4. coverage, from the expectation's own records: conditions on the inputs that keep a case from passing vacuously;
  5. discrimination: the restatement made wrong on purpose must differ where the case was built to notice.
The GPU half is tests/test_hevc_intra_gpu.py."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import analytic_hevc as ah
import analytic_hevc_intra as ai
import hevc_intra_ref as ir
import scripted_hevc as hw
from test_analytic_host import parse_only
from tools import streams
from util import ROOT

NAMES = sorted(ai.CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(seq, pics, stream, expected planes, records) of a case: computed once, never modified"""
    seq, pics = ai.CASES[name]()
    planes, records = ir.expect(seq, pics)
    return seq, pics, hw.write(seq, pics), planes, records


def all_records():
    return [r for name in NAMES for r in case(name)[4]]


@pytest.fixture(scope="module")
def oracle_hevc():
    return streams.OracleHevc()


# ---- 1. worked by hand ----------------------------------------------------------------------------------------------------------------------------
# the neighbours of a 4x4 block: p[-1][-1] = 10, the left column p[-1][0 .. 7] = 20 30 40 50 60 70 80 90, the row above p[0 .. 7][-1] = 12 24 .. 96
LEFT = [20, 30, 40, 50, 60, 70, 80, 90]
TOP = [12, 24, 36, 48, 60, 72, 84, 96]
V4 = np.array(LEFT[::-1] + [10] + TOP, np.int64)


def test_planar_dc_and_negative_angles_worked_by_hand():
    # planar (8.4.4.2.4): ((3 - x) p[-1][y] + (x + 1) p[4][-1] + (3 - y) p[x][-1] + (y + 1) p[-1][4] + 4) >> 3 with p[4][-1] = p[-1][4] = 60:
    #   (0,0): 3*20 + 60 + 3*12 + 60 + 4 = 220 -> 27     (3,0): 4*60 + 3*48 + 60 + 4 = 448 -> 56
    #   (0,3): 3*50 + 60 + 4*60 + 4 = 454 -> 56          (3,3): 4*60 + 4*60 + 4 = 484 -> 60
    p = ir.predict(V4, 4, 0, 0)[0]
    assert (p[0, 0], p[0, 3], p[3, 0], p[3, 3]) == (27, 56, 56, 60)
    # DC (8.4.4.2.5): (12 + 24 + 36 + 48 + 20 + 30 + 40 + 50 + 4) >> 3 = 264 >> 3 = 33; luma edges: (20 + 66 + 12 + 2) >> 2 = 25;
    #   row 0: (24 + 99 + 2) >> 2 = 31, (36 + 101) >> 2 = 34, (48 + 101) >> 2 = 37; column 0: (30 + 101) >> 2 = 32, (40 + 101) >> 2 = 35, (50 + 101) >> 2 = 37
    p = ir.predict(V4, 4, 1, 0)[0]
    assert p.tolist() == [[25, 31, 34, 37], [32, 33, 33, 33], [35, 33, 33, 33], [37, 33, 33, 33]]
    assert (ir.predict(V4, 4, 1, 1)[0] == 33).all()                 # chroma: no edge filter
    # mode 18 (angle -32, invAngle -256): ref[0 .. 4] = 10 12 24 36 48, ref[-1 .. -4] = p[-1][-1 + ((256 k + 128) >> 8)] = p[-1][k - 1] = 20 30 40 50;
    #   iIdx = -(y + 1), iFact = 0: pred[y][x] = ref[x - y]
    p = ir.predict(V4, 4, 18, 0)[0]
    assert p.tolist() == [[10, 12, 24, 36], [20, 10, 12, 24], [30, 20, 10, 12], [40, 30, 20, 10]]
    # mode 20 (angle -21, invAngle -390): (4 * -21) >> 5 = -3: ref[-1] = p[-1][-1 + (518 >> 8)] = p[-1][1] = 30, ref[-2] = p[-1][-1 + (908 >> 8)] = 40,
    #   ref[-3] = p[-1][-1 + (1298 >> 8)] = p[-1][4] = 60.  y = 0: iIdx = -1, iFact = 11: (21 * ref[0] + 11 * ref[1] + 16) >> 5 = (210 + 132 + 16) >> 5 = 11
    #   y = 3: -84 >> 5 = -3, iFact = -84 & 31 = 12: x = 0: (20 * ref[-2] + 12 * ref[-1] + 16) >> 5 = (800 + 360 + 16) >> 5 = 36
    p = ir.predict(V4, 4, 20, 0)[0]
    assert (p[0, 0], p[3, 0]) == (11, 36)
    # mode 10 is mode 26 mirrored; its edge filter: p[-1][0] + ((p[x][-1] - p[-1][-1]) >> 1) = 20 + (2 >> 1), 20 + 7, 20 + 13, 20 + 19
    assert ir.predict(V4, 4, 10, 0)[0].tolist() == [[21, 27, 33, 39], [30] * 4, [40] * 4, [50] * 4]
    assert ir.predict(V4, 4, 26, 0)[0][:, 0].tolist() == [12 + 5, 12 + 10, 12 + 15, 12 + 20] and ir.predict(V4, 4, 26, 1)[0].tolist() == [TOP[:4]] * 4


def test_substitution_and_smoothing_worked_by_hand():
    v = np.arange(100, 117)
    ok = np.ones(17, bool)
    ok[:6] = False; ok[9:11] = False; ok[15:] = False               # the search finds v[6] (in the column); a gap takes 108; the end takes 114
    got, start = ir.substitute(v, ok)
    assert got.tolist() == [106] * 6 + [106, 107, 108, 108, 108, 111, 112, 113, 114, 114, 114] and start == "column"
    assert ir.substitute(v, np.zeros(17, bool))[0].tolist() == [128] * 17
    assert ir.substitute(v, np.arange(17) >= 8)[1] == "corner" and ir.substitute(v, np.arange(17) >= 9)[1] == "top" and ir.substitute(v, ok | True)[1] is None
    # [1 2 1] on an 8x8 block, mode 2: corner (p[-1][0] + 2 p[-1][-1] + p[0][-1] + 2) >> 2 = (20 + 20 + 12 + 2) >> 2 = 13; p[-1][0]: (30 + 40 + 10 + 2) >> 2 = 20;
    #   p[0][-1]: (24 + 24 + 10 + 2) >> 2 = 15; the ends p[-1][15], p[15][-1] stay
    left = np.array([10] + LEFT + LEFT, np.int64)
    top = np.array([10] + TOP + TOP, np.int64)
    fl, ft, which, _ = ir.smooth(left, top, 8, 2, False, {})
    assert which == "121" and (fl[0], ft[0], fl[1], ft[1], fl[16], ft[16]) == (13, 13, 20, 15, 90, 96)
    assert ir.smooth(left, top, 8, 3, False, {})[2] == "none" and ir.smooth(left, top, 8, 1, False, {})[2] == "none"
    # bi-linear, 32x32: corner 100, p[-1][63] = 164, p[63][-1] = 36: p[-1][y] = (63 - y) * 100 + (y + 1) * 164 + 32) >> 6 = 100 + y + 1
    left = np.full(65, 100, np.int64); left[32], left[64] = 132, 164
    top = np.full(65, 100, np.int64); top[32], top[64] = 68, 36
    fl, ft, which, vals = ir.smooth(left, top, 32, 2, True, {})
    assert which == "strong" and vals == (0, 0) and fl.tolist() == list(range(100, 165)) and ft.tolist() == list(range(100, 35, -1))
    top[32] = 72                                                    # Abs(100 + 36 - 144) = 8: refused
    assert ir.smooth(left, top, 32, 2, True, {})[2:] == ("121", (8, 0))
    top[32] = 71                                                    # Abs(100 + 36 - 142) = 6
    assert ir.smooth(left, top, 32, 2, True, {})[2:] == ("strong", (6, 0))


def test_dc_only_residual_worked_by_hand():
    # level 5 at qP 24 (levelScale 40, << 4): 5 * 16 * 40 * 16 = 51200
    #   4x4 DCT: (51200 + 16) >> 5 = 1600; (64 * 1600 + 64) >> 7 = 800; (64 * 800 + 2048) >> 12 = 13
    #   8x8: (51200 + 32) >> 6 = 800; 400; (25600 + 2048) >> 12 = 6     16x16: 400; 200; (12800 + 2048) >> 12 = 3     32x32: 200; 100; (6400 + 2048) >> 12 = 2
    assert [int(ir.dc_residual(5, 24, lg, False)[0, 0]) for lg in (2, 3, 4, 5)] == [13, 6, 3, 2]
    #   4x4 DST, d = 1600: first stage (29, 55, 74, 84) * 1600 + 64 >> 7 = 363, 688, 925, 1050; [y][x] = (c[x] * g[y] + 2048) >> 12:
    #   [0][0] (29 * 363 + 2048) >> 12 = 3, [3][3] (84 * 1050 + 2048) >> 12 = 22, [1][2] (74 * 688 + 2048) >> 12 = 12, [0][3] (84 * 363 + 2048) >> 12 = 7
    r = ir.dc_residual(5, 24, 2, True)
    assert (r[0, 0], r[3, 3], r[1, 2], r[0, 3]) == (3, 22, 12, 7)
    # level -3 at qP 17 (levelScale 72, << 2): -13824
    #   4x4 DCT: (-13824 + 16) >> 5 = -432; (-27648 + 64) >> 7 = -216; (-13824 + 2048) >> 12 = -3
    #   8x8: -216; -108; (-6912 + 2048) >> 12 = -2     16x16: -108; -54; (-3456 + 2048) >> 12 = -1     32x32: -54; -27; (-1728 + 2048) >> 12 = 0
    assert [int(ir.dc_residual(-3, 17, lg, False)[0, 0]) for lg in (2, 3, 4, 5)] == [-3, -2, -1, 0]
    #   DST, d = -432: first stage -98, -186, -250, -283; [0][0] (29 * -98 + 2048) >> 12 = -1, [3][3] (84 * -283 + 2048) >> 12 = -6, [1][2] (74 * -186 + 2048) >> 12 = -3
    r = ir.dc_residual(-3, 17, 2, True)
    assert (r[0, 0], r[3, 3], r[1, 2]) == (-1, -6, -3)
    # a level that drives the scaled coefficient into the 16-bit clip: 1500 * 16 * 72 << 8 >> 5 is far beyond 32767
    assert int(ir.dc_residual(1500, 51, 2, False)[0, 0]) == (64 * ((64 * 32767 + 64) >> 7) + 2048) >> 12
    assert ir.chroma_qp(29) == 29 and ir.chroma_qp(30) == 29 and ir.chroma_qp(40) == 36 and ir.chroma_qp(43) == 37 and ir.chroma_qp(51) == 45
    assert [ir.chroma_mode(v, 5) for v in range(5)] == [0, 26, 10, 1, 5] and [ir.chroma_mode(v, m) for v, m in ((0, 0), (1, 26), (2, 10), (3, 1))] == [34] * 4


def test_z_scan_order_and_candidate_lists():
    # 6.5.2: inside a 16x16 CTB the 4x4 blocks count 0 1 4 5 / 2 3 6 7 / 8 9 12 13 / 10 11 14 15; the next CTB starts at 16
    assert [[hw.zscan(x, y, 4, 3) for x in range(0, 16, 4)] for y in range(0, 16, 4)] == [[0, 1, 4, 5], [2, 3, 6, 7], [8, 9, 12, 13], [10, 11, 14, 15]]
    assert hw.zscan(16, 0, 4, 3) == 16 and hw.zscan(0, 16, 4, 3) == 48
    xs, ys = np.meshgrid(np.arange(0, 136, 4), np.arange(0, 104, 4))
    assert np.array_equal(ir.zorder(xs, ys, 6, 3), np.vectorize(lambda x, y: hw.zscan(x, y, 6, 3))(xs, ys))
    # 8.4.2
    assert hw.mpm_candidates(1, 1) == [0, 1, 26] and hw.mpm_candidates(0, 0) == [0, 1, 26]
    assert hw.mpm_candidates(10, 10) == [10, 9, 11] and hw.mpm_candidates(2, 2) == [2, 33, 3] and hw.mpm_candidates(34, 34) == [34, 33, 3]
    assert hw.mpm_candidates(5, 7) == [5, 7, 0] and hw.mpm_candidates(0, 7) == [0, 7, 1] and hw.mpm_candidates(1, 0) == [1, 0, 26]


# ---- 2. the writer --------------------------------------------------------------------------------------------------------------------------------
def test_the_earlier_hevc_streams_still_come_out_byte_for_byte():
    """tests/golden/scripted_hevc_digests.json was recorded before the writer learnt quadtrees and intra units"""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "scripted_hevc_digests.json")))
    want = {k: v for k, v in want.items() if not k.startswith(("resid_", "inter_", "loop_"))}       # (those streams' digests: tests/test_hevc_resid_host.py, tests/test_hevc_inter_host.py, tests/test_hevc_loop_host.py)
    got = {f"{n}-{s[0]}x{s[1]}": hw.write(*ah.HEVC_CASES[n](*s)) for n in sorted(ah.HEVC_CASES) for s in ah.SIZES}
    got["full_hd_rows-1920x1080"] = hw.write(*ah.full_hd_rows())
    got["one_slice_per_ctb_stream-272x256"] = hw.write(*ah.one_slice_per_ctb_stream(272, 256))
    assert sorted(got) == sorted(want)
    moved = [k for k in sorted(got) if hashlib.sha256(got[k]).hexdigest() != want[k]]
    assert not moved, moved


@pytest.mark.parametrize("name", NAMES)
def test_writer_is_deterministic(name):
    assert hw.write(*ai.CASES[name]()) == case(name)[2]


def test_skip_units_in_larger_slices_only_where_every_inter_unit_is_skipped():
    seq, pics = ah.HEVC_CASES["skip_copies"](96, 80)
    pics[1]["layout"] = "row"                                       # skipped and moved units mixed
    with pytest.raises(AssertionError):
        hw.write(seq, pics)


# ---- 3. the oracle and the host parser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_decodes_the_intra_expectation(oracle_hevc, name):
    seq, pics, data, planes, records = case(name)
    for fmt in (1, 0):
        got, n, w, h = oracle_hevc.decode(data, fmt)
        assert (n, w, h) == (len(pics), seq["width"], seq["height"])
        fs = w * h * 3 // 2
        diff = ir.difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], fmt, planes, records)
        assert diff is None, f"{name} format {fmt}: {diff}"


@pytest.mark.parametrize("name", NAMES)
def test_host_parser_accepts_the_intra_stream(name):
    seq, pics, data, planes, records = case(name)
    n, errors, info, err, failed = parse_only(data, codec=1)
    assert failed is None and errors == 0 and err == "", (failed, errors, err)
    assert n == len(pics) and info == (seq["width"], seq["height"])


def test_a_wrong_block_is_named_with_its_record():
    seq, pics, data, planes, records = case("intra_substitution-ctb16")
    import analytic_expect as ae
    frames = ae.expected_frames(seq, pics, 1, planes)
    assert ir.difference(seq, pics, frames, 1, planes, records) is None
    r = next(r for r in records if r["pic"] == 1 and r["plane"] == 1 and r["x"] > 8)
    bad = [tuple(c.copy() for c in pl) for pl in planes]
    bad[1][1][r["y"] + 1, r["x"] + 2] ^= 1
    text = ir.difference(seq, pics, ae.expected_frames(seq, pics, 0, bad), 0, planes, records)
    for part in ("picture 1", "plane Cb", f"block at ({r['x']}, {r['y']})", f"{r['n']}x{r['n']}", f"mode {r['mode']}", "below_left", "above_right",
                 f"first at ({r['x'] + 2}, {r['y'] + 1})"):
        assert part in text, (part, text)


# ---- 4. coverage ----------------------------------------------------------------------------------------------------------------------------------
def test_every_luma_size_and_mode_with_all_neighbours_and_with_substitution():
    seen = {(r["n"], r["mode"], r["all_avail"]) for r in all_records() if r["plane"] == 0}
    missing = [(n, m, a) for n in (4, 8, 16, 32) for m in range(35) for a in (True, False) if (n, m, a) not in seen]
    assert not missing, f"(size, mode, all neighbours available) that no case has: {missing}"


def test_every_chroma_size_and_derivation():
    """intra_chroma_pred_mode 0 .. 3 as the table mode and replaced by 34, and 4 (the luma mode of the unit's first block), at 4x4, 8x8 and 16x16"""
    seen = set()
    for r in all_records():
        if r["plane"]:
            v = r["unit"]["chroma"]
            assert r["mode"] == ir.chroma_mode(v, r["unit"]["modes"][0])
            seen.add((r["n"], v, r["mode"] == 34 and v != 4))
    missing = [(n, v, s) for n in (4, 8, 16) for v in range(5) for s in (False, True) if not (v == 4 and s) and (n, v, s) not in seen]
    assert not missing, f"(chroma size, intra_chroma_pred_mode, replaced by 34) that no case has: {missing}"
    assert any(r["plane"] and r["unit"]["chroma"] == 4 and len(r["unit"]["modes"]) == 4 and r["mode"] != r["unit"]["modes"][3] for r in all_records())


def test_neighbour_groups_substitution_starts_and_nothing_available():
    recs = all_records()
    for plane in (0, 1, 2):
        for g, name in enumerate(ir.GROUPS):
            states = {r["avail"][g] for r in recs if r["plane"] == plane}
            assert {0, 2} <= states, f"plane {plane}: {name} is never {'unavailable' if 0 not in states else 'available'}"
            # each group missing ALONE too (the corner alone: only under constrained_intra_pred_flag)
            assert any(r["avail"][g] == 0 and all(q == 2 for i, q in enumerate(r["avail"]) if i != g) for r in recs if r["plane"] == plane), (plane, name)
    assert any(1 in r["avail"] for r in recs) and any(r["gap"] for r in recs)           # an edge available in part; a gap inside the search order
    for n in (4, 8, 16, 32):
        starts = {r["start"] for r in recs if r["plane"] == 0 and r["n"] == n}
        assert {"column", "top", None} <= starts, (n, starts)
    assert {"column", "corner", "top"} <= {r["start"] for r in recs}
    assert {"column", "corner", "top"} <= {r["start"] for r in case("intra_constrained")[4]}
    nothing = [r for r in recs if r["avail"] == (0,) * 5]
    assert {r["n"] for r in nothing if r["plane"] == 0} >= {8, 16, 32} and any(r["plane"] for r in nothing)
    # intra_constrained: the unit enclosed by skipped units, inside the picture and the slice, predicts from 128
    assert any(r["avail"] == (0,) * 5 and (r["x"], r["y"], r["pic"]) == (40, 40, 3) for r in case("intra_constrained")[4])
    assert not any(r["avail"] == (0,) * 5 and (r["x"], r["y"], r["pic"]) == (40, 40, 3) for r in case("intra_constrained-flag_off")[4])
    # the partial CTBs at the right and bottom edge hold intra blocks
    for name in ("intra_substitution-ctb64", "intra_substitution-ctb32", "intra_substitution-ctb16"):
        seq, pics, data, planes, records = case(name)
        s = 1 << seq["ctb_log2"]
        W, H = hw.coded_size(seq)
        assert W % s and H % s and W % 8 == 0 and H % 8 == 0
        assert any(r["x"] >= W // s * s for r in records if r["plane"] == 0) and any(r["y"] >= H // s * s for r in records if r["plane"] == 0), name
        assert {p.get("layout") for p in pics} == {"ctb", "row", "pic"}
        # what slices and picture edges can take away (6.4.1): everything; the below-left; the left column with the corner; the upper right; the row
        # above with the left column present (with and without the below-left)
        assert {(0, 0, 0, 0, 0), (0, 2, 2, 2, 2), (0, 0, 0, 2, 2), (2, 2, 2, 2, 0), (2, 2, 0, 0, 0), (0, 2, 0, 0, 0)} <= {r["avail"] for r in records}, name


def test_smoothing_on_both_sides_of_every_threshold():
    recs = [r for r in all_records() if r["plane"] == 0 and r["mode"] != 1]
    dist = lambda r: min(abs(r["mode"] - 26), abs(r["mode"] - 10))
    for n, thr in ((8, 7), (16, 1), (32, 0)):
        assert any(r["n"] == n and dist(r) == thr + 1 and r["filt"] == "121" for r in recs), (n, "taken")
        assert any(r["n"] == n and dist(r) == thr and r["filt"] == "none" for r in recs), (n, "not taken")
    assert all(r["filt"] == "none" for r in all_records() if r["plane"] or r["n"] == 4 or r["mode"] == 1)
    # the bi-linear filter: taken at 7 and 7, refused by the row above alone at 8, by the left column alone at 8 -- with every neighbour available and
    # with the upper-right neighbours substituted
    strong = [r for r in case("intra_strong_smoothing")[4] if r["plane"] == 0]
    for all_avail in (True, False):
        got = {(r["strong_values"], r["filt"]) for r in strong if r["all_avail"] == all_avail}
        assert {((7, 7), "strong"), ((8, 7), "121"), ((7, 8), "121"), ((8, 8), "121")} <= got, (all_avail, got)
        assert all(r["avail"] == ((2, 2, 2, 2, 2) if all_avail else (2, 2, 2, 2, 0)) for r in strong if r["all_avail"] == all_avail)
    assert len(strong) == 14 and sum(r["filt"] == "strong" for r in strong) == 4
    off = [r for r in case("intra_strong_smoothing-flag_off")[4] if r["plane"] == 0]
    assert all(r["filt"] == "121" and r["strong_values"] is None for r in off)


def test_edge_filter_and_residual_clip_act_both_ways():
    recs = all_records()
    for mode in (10, 26):
        for n in (4, 8, 16):
            cuts = [r["hv_cut"] for r in recs if r["plane"] == 0 and r["mode"] == mode and r["n"] == n]
            assert any(c[0] for c in cuts) and any(c[1] for c in cuts) and any(c == (False, False) for c in cuts), (mode, n)
    res = [r for r in case("intra_dc_residual")[4] if r["level"]]
    for plane in (0, 1, 2):
        for n in ((4, 8, 16, 32) if plane == 0 else (4, 8, 16)):
            q = [r for r in res if r["plane"] == plane and r["n"] == n]
            assert any(r["level"] > 0 for r in q) and any(r["level"] < 0 for r in q), (plane, n)
            assert any(r["res_cut"][0] for r in q) and any(r["res_cut"][1] for r in q), (plane, n)
        assert any(r["res_cut"] == (False, False) for r in res if r["plane"] == plane), plane
    assert {p["qp"] % 6 for p in case("intra_dc_residual")[1]} == set(range(6))
    assert len({r["level"] for r in res}) > 100
    assert any(r["level"] == 0 for r in case("intra_dc_residual")[4])


def test_wavefront_and_scattered_cases_have_the_shapes_they_are_about():
    seq, pics, data, planes, records = case("intra_wavefront-ctb16")
    assert hw.ctb_dims(seq)[0] >= 9                                 # a run of eight segments holds two CTBs: hand-overs inside a run and between runs
    seq, pics, data, planes, records = case("intra_wavefront-ctb64")
    assert sum(1 for r in records if r["pic"] == 0 and 64 <= r["x"] << (r["plane"] > 0) < 128 and 64 <= r["y"] << (r["plane"] > 0) < 128) == 384
    for name in ("intra_wavefront-ctb16", "intra_wavefront-ctb64"):
        seq, pics, data, planes, records = case(name)
        s = 1 << seq["ctb_log2"]
        assert all(u["t"] == ("pcm" if x < s or y < s else "intra") for p in pics for (x, y, lg, d, u) in hw.walk(seq, p))
        # texture survives the copying from block to block: in every picture at least 70 % of the 16x16 areas behind the PCM border are not flat
        for pl in planes:
            dev = [pl[0][y:y + 16, x:x + 16].std() for y in range(s, pl[0].shape[0], 16) for x in range(s, pl[0].shape[1], 16)]
            assert np.mean(np.array(dev) > 10) >= 0.7, name
    for name in ("intra_scattered_in_b-ctb32", "intra_scattered_in_b-ctb64"):
        seq, pics, data, planes, records = case(name)
        s = 1 << seq["ctb_log2"]
        assert [p["kind"] for p in pics] == ["I", "P", "B", "B", "B"]
        for k in (2, 3, 4):
            units = [(x, y, lg, u) for (x, y, lg, d, u) in hw.walk(seq, pics[k])]
            intra = [(x, y, lg) for (x, y, lg, u) in units if u["t"] == "intra"]
            assert 0 < len(intra) < len(units) // 4 and all(u["t"] in ("skip", "intra") for (_, _, _, u) in units)
            at_edge = [((x + (1 << lg)) % s == 0 or (y + (1 << lg)) % s == 0) for (x, y, lg) in intra]
            assert any(at_edge) and not all(at_edge), (name, k)


# ---- 5. discrimination ----------------------------------------------------------------------------------------------------------------------------
def reads_corner(r):
    return 11 <= r["mode"] <= 25 or (r["mode"] in (10, 26) and r["plane"] == 0 and r["n"] < 32) or r["filt"] != "none"


SWITCH_CASES = [
    ("no_smoothing", "intra_every_mode_and_size-ctb32", lambda r: r["filt"] != "none"),
    ("weak_for_strong", "intra_strong_smoothing", lambda r: r["filt"] == "strong"),
    ("no_dc_edge", "intra_every_mode_and_size-ctb16", lambda r: r["plane"] == 0 and r["mode"] == 1 and r["n"] < 32),
    ("no_hv_edge", "intra_every_mode_and_size-ctb16", lambda r: r["plane"] == 0 and r["mode"] in (10, 26) and r["n"] < 32),
    ("no_hv_clip", "intra_every_mode_and_size-ctb16", lambda r: any(r["hv_cut"])),
    ("substitute_backwards", "intra_constrained", lambda r: r["gap"]),
    ("corner_from_top", "intra_substitution-ctb32", reads_corner),
    ("residual_no_clip", "intra_dc_residual", lambda r: r["res_cut"] is not None and any(r["res_cut"])),
]


@pytest.mark.parametrize("switch,name,touches", SWITCH_CASES, ids=[s[0] for s in SWITCH_CASES])
def test_a_restatement_that_is_wrong_on_purpose_differs(switch, name, touches):
    """In the case built for it, the switched restatement differs from the real one in at least a quarter of the blocks the switch can touch (judged
    on the real one's records): a decoder with that mistake fails the case."""
    assert sorted(s[0] for s in SWITCH_CASES) == sorted(ir.SWITCHES)
    seq, pics, data, planes, records = case(name)
    wrong, _ = ir.expect(seq, pics, **{switch: True})
    block = lambda pl, r: pl[r["pic"]][r["plane"]][r["y"]:r["y"] + r["n"], r["x"]:r["x"] + r["n"]]
    touched = [r for r in records if touches(r)]
    differ = sum(1 for r in touched if not np.array_equal(block(planes, r), block(wrong, r)))
    assert len(touched) >= 4 and differ * 4 >= len(touched), f"{switch} in {name}: {differ} of {len(touched)} blocks differ"
