"""H.265 residual coding, quantisation parameters, scaling and inverse transforms against clauses 7.3.8.11, 8.6.1 - 8.6.4.2 on the CPU: scripted streams
(tests/scripted_hevc.py, cases of tests/analytic_hevc_resid.py) whose expected pictures tests/hevc_resid_ref.py computes from the script -- no decoder
computed them.

  1. the restatement's own pins: values worked by hand;
  2. the writer: deterministic, and the new streams come out as recorded (tests/golden/scripted_hevc_digests.json, keys "resid_*"; the earlier
     streams are held by tests/test_hevc_intra_host.py);
  3. every case through the CPU oracle, I420 and NV12, bit for bit, and through a parse_only product handle;
  4. coverage, group by group, from the expectation's records and the writer's counters, without exemptions;
  5. discrimination: every switch of the restatement changes expected samples; every switch of the writer makes the oracle differ or refuse.
The GPU half is tests/test_hevc_resid_gpu.py."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import analytic_hevc_resid as ar
import hevc_resid_ref as rr
import scripted_hevc as hw
from test_analytic_host import parse_only
from tools import streams
from util import ROOT

NAMES = sorted(ar.CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(seq, pics, stream, expected planes, records, the writer's counters) of a case: computed once, never modified"""
    seq, pics = ar.CASES[name]()
    stats = {}
    data = hw.write(seq, pics, stats=stats)
    planes, records = rr.expect(seq, pics)
    return seq, pics, data, planes, records, stats


def group(name):
    """(records, counters, [(seq, pics)]) of a group's cases"""
    recs, stats, scripts = [], {}, []
    for n in ar.GROUPS.get(name, ()):
        if n in ar.CASES:
            c = case(n)
            recs += c[4]
            scripts.append((c[0], c[1]))
            for k, v in c[5].items():
                stats[k] = stats.get(k, 0) + v
    return recs, stats, scripts


def units_of(scripts):
    return [u for seq, pics in scripts for p in pics for (_, _, _, _, u) in hw.walk(seq, p)]


@pytest.fixture(scope="module")
def oracle_hevc():
    return streams.OracleHevc()


# ---- 1. worked by hand ----------------------------------------------------------------------------------------------------------------------------
def test_a_dst_block_worked_by_hand():
    # level 2 at (x, y) = (1, 0) of an intra 4x4 luma block, qP 28 (levelScale 64 << 4 = 1024), m = 16: d = (2 * 16 * 1024 + 16) >> 5 = 1024.
    # first stage, column 1: row 0 of the DST matrix (29 55 74 84) * 1024, (e + 64) >> 7 = 232 440 592 672 by y.
    # second stage, row y: g[y] * row 1 of the matrix (74 74 0 -74), (r + 2048) >> 12:
    #   y = 0: 232 * 74 = 17168 -> (17168 + 2048) >> 12 = 4, (-17168 + 2048) >> 12 = -4      y = 1: 440 * 74 = 32560 -> 8, -8
    #   y = 2: 592 * 74 = 43808 -> 11, (-43808 + 2048) >> 12 = -11                             y = 3: 672 * 74 = 49728 -> 12, -12
    lev = np.zeros((4, 4), np.int64); lev[0, 1] = 2
    r, d, cut, c1 = rr.residual(lev, 28, 2, np.full((4, 4), 16), True, False, False)
    assert d[0, 1] == 1024 and r.tolist() == [[4, 4, 0, -4], [8, 8, 0, -8], [11, 11, 0, -11], [12, 12, 0, -12]] and cut == (False, False) and not c1
    # the same coefficient through the DCT (an inter or chroma 4x4 block): column 1 by row 0 (64 64 64 64): g = 512 each; row 1 of the DCT (83 36 -36 -83):
    #   (512 * 83 + 2048) >> 12 = 10, (512 * 36 + 2048) >> 12 = 5, (-18432 + 2048) >> 12 = -4, (-42496 + 2048) >> 12 = -10
    assert rr.residual(lev, 28, 2, np.full((4, 4), 16), False, False, False)[0].tolist() == [[10, 5, -4, -10]] * 4
    # a list entry m[1][0] = 9 (x = 1, y = 0) instead of 16: d = (2 * 9 * 1024 + 16) >> 5 = 576; the transposed reading takes m[0][1]
    m = np.full((4, 4), 16); m[0, 1] = 9; m[1, 0] = 71
    assert rr.scale(lev, 28, 2, m)[0][0, 1] == 576 and rr.scale(lev, 28, 2, m.T)[0][0, 1] == (2 * 71 * 1024 + 16) >> 5


def test_a_transform_skip_sample_and_the_clips_worked_by_hand():
    # level 3 at qP 22 (levelScale 64 << 3 = 512): d = (3 * 16 * 512 + 16) >> 5 = 768; r = 768 << 7 = 98304; (98304 + 2048) >> 12 = 24
    # level -3: d = (-24576 + 16) >> 5 = -768 (floor of -767.5); (-98304 + 2048) >> 12 = -24 (floor of -23.5)
    lev = np.zeros((4, 4), np.int64); lev[2, 3], lev[1, 0] = 3, -3
    r = rr.residual(lev, 22, 2, np.full((4, 4), 16), False, True, False)[0]
    assert r[2, 3] == 24 and r[1, 0] == -24 and np.count_nonzero(r) == 2
    assert rr.residual(lev, 22, 2, np.full((4, 4), 16), False, False, True)[0].tolist() == lev.tolist()          # bypass: the levels
    # the 16-bit clip: level 900 at qP 51 (57 << 8 = 14592): 900 * 16 * 14592 >> 5 is far beyond 32767
    lev = np.zeros((4, 4), np.int64); lev[0, 0], lev[0, 1] = 900, -900
    r, d, cut, c1 = rr.residual(lev, 51, 2, np.full((4, 4), 16), False, False, False)
    assert d[0, 0] == 32767 and d[0, 1] == -32768 and cut == (True, True)
    # the first-stage clip: four coefficients of -32768 down column 0 through the DCT: e[0] = (64 + 83 + 64 + 36) * -32768 = -8093696,
    # (e + 64) >> 7 = -63232 -> -32768; second stage (64 * g + 2048) >> 12 = -512, without the clip (64 * -63232 + 2048) >> 12 = -988
    lev = np.zeros((4, 4), np.int64); lev[:, 0] = -900
    r, d, cut, c1 = rr.residual(lev, 51, 2, np.full((4, 4), 16), False, False, False)
    assert c1 and r[0, 0] == (64 * -32768 + 2048) >> 12 == -512
    assert rr.residual(lev, 51, 2, np.full((4, 4), 16), False, False, False, dict(no_stage1_clip=True))[0][0, 0] == (64 * -63232 + 2048) >> 12 == -988


def test_a_qp_chain_worked_by_hand():
    # one 32x32 CTB of four 16x16 units, a quantisation group each (diff_cu_qp_delta_depth 1), slice QP 50, deltas +3, +10, -8, 0:
    #   group 0: first of the slice: qPY_PREV = 50, no neighbour inside the CTB: pred 50; QpY = (50 + 3 + 52) % 52 = 1
    #   group 1 at (16, 0): PREV = 1, left = 1, above outside: (1 + 1 + 1) >> 1 = 1; QpY = 11
    #   group 2 at (0, 16): PREV = 11, left outside -> 11, above = group 0 = 1: (11 + 1 + 1) >> 1 = 6; QpY = (6 - 8 + 52) % 52 = 50
    #   group 3 at (16, 16): left = 50, above = 11: (50 + 11 + 1) >> 1 = 31; QpY = 31; Cb: qPi = 31 - 4 = 27 -> 27; Cr: qPi = 31 + 5 = 36 -> 34
    #   group 0's chroma: Cb qPi = 1 - 4 -> 0; group 2's Cr: qPi = 55 -> 49
    seq = ar.base_seq(32, 32, cu_qp_delta=1, diff_cu_qp_delta_depth=1, cb_qp_offset=-4, cr_qp_offset=5)
    coef = [{0: {(0, 0): 1}, 1: {(0, 0): 1}, 2: {(0, 0): 1}}]
    sub = [ar.intra([1], 4, 0, coef, dqp=d) for d in (3, 10, -8, 0)]
    _, recs = rr.expect(seq, [dict(kind="I", poc=0, qp=50, cus=[dict(t="split", sub=sub)])])
    assert [r["qp"] for r in recs if r["plane"] == 0] == [1, 11, 50, 31]
    assert [r["qp"] for r in recs if r["plane"] == 1] == [0, 7, 40, 27] and [r["qp"] for r in recs if r["plane"] == 2] == [6, 16, 49, 34]
    # the 16x16 list with DC: entry 0 of the list is replaced at (0, 0) only; entry i = 1 of the diagonal order is (x, y) = (0, 1)
    lists = rr.resolve_lists({(2, 0): ("coded", list(range(10, 74)), 99)})
    m = rr.scaling_factor(lists, 4, 0)
    assert m[0, 0] == 99 and m[0, 1] == 10 and m[1, 1] == 10 and m[2, 0] == 11 and m[0, 2] == 12 and m[15, 15] == 73
    assert rr.scaling_factor(lists, 4, 3)[0, 0] == 16 and rr.scaling_factor(lists, 4, 3)[15, 15] == 91 and rr.scaling_factor(lists, 5, 0)[31, 31] == 115


# ---- 2. the writer --------------------------------------------------------------------------------------------------------------------------------
def test_the_residual_streams_come_out_as_recorded():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "scripted_hevc_digests.json")))
    got = {n: hashlib.sha256(case(n)[2]).hexdigest() for n in NAMES}
    assert sorted(k for k in want if k.startswith("resid_")) == NAMES
    moved = [n for n in NAMES if got[n] != want[n]]
    assert not moved, moved


@pytest.mark.parametrize("name", NAMES)
def test_writer_is_deterministic(name):
    assert hw.write(*ar.CASES[name]()) == case(name)[2]


def test_the_writer_refuses_a_level_whose_parity_contradicts_the_hidden_sign():
    seq = ar.base_seq(16, 16, ctb_log2=4, sign_hiding=1)
    for lv, ok in ((-1, True), (1, False)):                         # positions 0 and 15 of the sub-block, sum 3 (odd): the hidden sign is negative
        pics = [dict(kind="I", poc=0, cus=[ar.intra([1], 4, 2, [{0: ar.sub_block(0, 0, {0: lv, 15: 2})}] + [None] * 15)])]
        if ok:
            hw.write(seq, pics)
        else:
            with pytest.raises(AssertionError):
                hw.write(seq, pics)


# ---- 3. the oracle and the host parser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_decodes_the_residual_expectation(oracle_hevc, name):
    seq, pics, data, planes, records, _ = case(name)
    for fmt in (1, 0):
        got, n, w, h = oracle_hevc.decode(data, fmt)
        assert (n, w, h) == (len(pics), seq["width"], seq["height"])
        fs = w * h * 3 // 2
        diff = rr.difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], fmt, planes, records)
        assert diff is None, f"{name} format {fmt}: {diff}"


@pytest.mark.parametrize("name", NAMES)
def test_host_parser_accepts_the_residual_stream(name):
    seq, pics, data, planes, records, _ = case(name)
    n, errors, info, err, failed = parse_only(data, codec=1)
    assert failed is None and errors == 0 and err == "", (failed, errors, err)
    assert n == len(pics) and info == (seq["width"], seq["height"])


# ---- 4. coverage ----------------------------------------------------------------------------------------------------------------------------------
SIZES = [(0, n) for n in (4, 8, 16, 32)] + [(c, n) for c in (1, 2) for n in (4, 8, 16)]


def test_sizes_cover_corners_dense_blocks_column_steps_and_rows():
    recs, stats, _ = group("sizes")
    for intra in (True, False):
        for (c, n) in SIZES:
            q = [r for r in recs if r["intra"] == intra and r["plane"] == c and r["n"] == n and not r["tskip"] and not r["bypass"]]
            single = {next(iter(r["coefs"])) for r in q if r["levels"] == 1}
            assert {(0, 0), (n - 1, 0), (0, n - 1), (n - 1, n - 1), (n // 2 - 1, n - 1), (n - 1, n // 2)} <= single, (intra, c, n, single)
            dense = max(r["scaled"] for r in q)
            assert dense == n * n if n <= 8 else dense > (400 if n == 32 else 64), (intra, c, n, dense)       # 8x8: exactly the 64 of one load; above: the second walk
            for col in ar.STEP_COLS:
                if col < n:
                    rows = {r["max_row"] for r in q if r["max_col"] == col}
                    assert {0, 1, n - 1} <= rows, (intra, c, n, col, rows)
            assert {rr.pad_cols(r["max_col"] + 1) for r in q} == {s for s in (4, 8, 16, 32) if s <= n}
            assert {r["max_row"] >> 1 for r in q} >= {0, (n - 1) >> 1}
        assert any(r["scaled"] > 64 for r in recs if r["intra"] == intra and r["plane"] and r["n"] == 16)
    assert any(r["dst"] for r in recs) and all(r["dst"] == (r["intra"] and r["plane"] == 0 and r["n"] == 4) for r in recs)


def test_scans_cover_every_mode_boundary_in_every_block_that_chooses_its_scan():
    recs, stats, _ = group("scans")
    for plane, n in ((0, 4), (0, 8), (1, 4), (2, 4)):
        modes = {r["mode"] for r in recs if r["plane"] == plane and r["n"] == n}
        assert set(ar.MODES) <= modes, (plane, n, modes)
    for lg, cidx in ((2, 0), (3, 0), (2, 1)):
        assert all(stats.get(("scan", "intra", lg, cidx, s), 0) >= 8 for s in (0, 1, 2)), (lg, cidx)
    # intra_chroma_pred_mode 4 hands down a luma mode with a scan of its own; the value that names the luma mode becomes 34 and scans diagonally
    assert any(r["plane"] and r["unit"]["chroma"] == 4 and r["mode"] in (6, 14, 22, 30) for r in recs)
    assert {r["unit"]["modes"][0] for r in recs if r["plane"] and r["mode"] == 34 and r["unit"]["chroma"] != 4} >= {26, 10}
    assert all(len(r["coefs"]) >= 2 and any((y, x) not in r["coefs"] for (x, y) in r["coefs"]) for r in recs), "a coefficient set is symmetric"
    all_stats = group("sizes")[1]                                   # larger blocks, chroma 8x8 and inter blocks never leave the diagonal scan
    assert not any(k[0] == "scan" and k[4] and (k[1] == "inter" or k[2] > 3 or (k[2] == 3 and k[3])) for k in {**all_stats, **stats})


def test_levels_cover_the_context_sets_the_rice_parameter_and_the_clips():
    recs, stats, _ = group("levels")
    assert stats.get(("more than 8 levels above 1",), 0) and stats.get(("sig_coeff_flag inferred",), 0)
    assert stats.get(("greater1Ctx carried", 0), 0) and stats.get(("greater1Ctx carried", 3), 0)
    assert any(k[:2] == ("coded_sub_block_flag", 0) for k in stats) and {k[2] for k in stats if k[:2] == ("coded_sub_block_flag", 1)} == {0, 1}
    assert stats.get(("cRiceParam raised to", 4), 0) and stats.get(("escape at cRiceParam", 4), 0)
    assert {k[1] for k in stats if k[0] == "last_suffix_bits"} >= {0, 1, 2}
    for intra in (True, False):
        q = [r for r in recs if r["intra"] == intra]
        assert any(r["d_max"] == 32767 for r in q) and any(r["d_min"] == -32768 for r in q), intra
        assert any(r["cut16"][0] for r in q) and any(r["cut16"][1] for r in q) and any(r["cut1"] for r in q), intra
        assert {(r["plane"], r["n"]) for r in q if r["cut1"]} >= {(0, 4), (0, 16), (1, 4), (1, 8)}, intra


def test_sign_hiding_covers_both_distances_both_parities_and_the_bypass_unit():
    recs, stats, _ = group("sign_hiding")
    for dist in (3, 4, 5):
        for parity in (0, 1):
            assert stats.get(("sign hiding", "coded", dist, parity), 0), (dist, parity)
    assert stats.get(("sign hiding", "bypass", 5, 1), 0) >= 2
    assert any(r["bypass"] and r["intra"] for r in recs) and any(r["bypass"] and not r["intra"] for r in recs)


def test_tskip_and_bypass_cover_every_component_choice_and_both_saturations():
    recs, stats, scripts = group("tskip_bypass")
    for t in ("intra", "inter"):
        seen = {(frozenset(e.get("tskip", ())), frozenset(k for k in (0, 1, 2) if e.get(k))) for u in units_of(scripts) if u["t"] == t for e in u.get("coef") or [] if e}
        for want in ({0}, {1}, {2}, {0, 1, 2}):
            assert (frozenset(want), frozenset({0, 1, 2})) in seen, (t, want)
        assert (frozenset({1}), frozenset({1})) in seen or (frozenset({2}), frozenset({2})) in seen, t      # the partner not coded
        assert (frozenset({0}), frozenset({0})) in seen and (frozenset(), frozenset({0, 1, 2})) in seen, t
    for intra in (True, False):
        for plane, sizes in ((0, (8, 16, 32)), (1, (4, 8, 16)), (2, (4, 8, 16))):
            for n in sizes:
                q = [r for r in recs if r["bypass"] and r["intra"] == intra and r["plane"] == plane and r["n"] == n]
                assert any(r["sat"][0] for r in q) and any(r["sat"][1] for r in q), (intra, plane, n)
    # both saturation directions in both adds (k_hevc_resid for inter units, k_hevc_intra for intra units), transformed blocks included
    every = [r for g in ar.GROUPS for r in group(g)[0]]
    for intra in (True, False):
        for plane in (0, 1, 2):
            q = [r for r in every if r["intra"] == intra and r["plane"] == plane and not r["bypass"] and not r["tskip"]]
            assert any(r["sat"][0] for r in q) and any(r["sat"][1] for r in q), (intra, plane)


def test_chroma_pairs_cover_both_one_and_the_other_at_every_size():
    recs, stats, _ = group("chroma_pairs")
    for n in (4, 8, 16):
        places = {}
        for r in recs:
            if r["plane"] and r["n"] == n and not r["intra"]:
                places.setdefault((r["pic"], r["x"], r["y"]), set()).add(r["plane"])
        assert {frozenset(v) for v in places.values()} == {frozenset({1, 2}), frozenset({1}), frozenset({2})}, n
    assert any(r["plane"] and r["unit"]["tu"] == 3 for r in recs), "the chroma pair behind four 4x4 luma blocks"
    # a chroma entry directly behind a luma entry, and directly behind another unit's chroma entry
    by_job = {(r["pic"], r["job"]): r for r in recs if r["job"] is not None}
    assert any(r["plane"] == 1 and by_job.get((p, j - 1), r)["plane"] == 2 for (p, j), r in by_job.items())
    assert any(r["plane"] == 2 and by_job.get((p, j - 1), r)["plane"] == 0 for (p, j), r in by_job.items())


def test_qp_covers_deltas_wraps_slices_offsets_and_every_remainder():
    recs, stats, scripts = group("qp")
    assert sorted(seq["diff_cu_qp_delta_depth"] for seq, _ in scripts) == [0, 1] and all(seq["ctb_log2"] == 5 for seq, _ in scripts)
    for depth, (seq, pics) in zip((0, 1), sorted(scripts, key=lambda s: s[0]["diff_cu_qp_delta_depth"])):
        q = [r for r in recs if r["unit"] in [u for p in pics for (_, _, _, _, u) in hw.walk(seq, p)]]
        luma = [r for r in q if r["plane"] == 0]
        assert any(r["qp_delta"] > 0 for r in luma) and any(r["qp_delta"] < 0 for r in luma), depth
        assert any(r["qp_pred"] + r["qp_delta"] > 51 for r in luma) and any(r["qp_pred"] + r["qp_delta"] < 0 for r in luma), depth
        assert {r["qp"] % 6 for r in luma} == set(range(6)) and {r["qp"] % 6 for r in q if r["plane"]} == set(range(6)), depth
        assert any(r["qp_reset"] for r in luma), depth              # a slice that starts in mid-picture
        assert {p.get("layout") for p in pics} == {"pic", "row", "ctb"}
        # a unit without cbf in front of the group's delta: the CTB's first unit codes nothing, the second carries the delta
        firsts = [c for p in pics for c in p["cus"] if c["sub"][0]["coef"] == [None]]
        assert firsts and all(c["sub"][1].get("dqp") is not None for c in firsts), depth
        # a unit that carries no delta of its own takes the group's (depth 0)
        assert depth == 1 or any("dqp" not in r["unit"] and r["qp_delta"] for r in luma)
    qpi = {r["qpi"] for r in recs if r["plane"]}
    assert min(qpi) < 0 and 0 in qpi and max(qpi) > 57 and set(range(30, 44)) <= qpi, sorted(qpi)


def test_scaling_lists_cover_asymmetry_prediction_dc_and_pps_over_sps():
    recs, stats, scripts = group("scaling_lists")
    specs = {("pps" if seq["scaling_lists"]["pps"] is not None else "sps" if seq["scaling_lists"]["sps"] is not None else "default"): seq for seq, _ in scripts}
    assert sorted(specs) == ["default", "pps", "sps"]
    sps = specs["sps"]["scaling_lists"]["sps"]
    assert {e[1] for e in sps.values() if e[0] == "ref"} >= {1, 2} and any(k not in sps for k in [(s, m) for s in range(3) for m in range(6)])
    lists = rr.lists_in_effect(specs["sps"])
    for log2 in (2, 3, 4, 5):
        for mid in ((0, 1) if log2 == 5 else (0, 3)):
            m = rr.scaling_factor(lists, log2, mid)
            assert not np.array_equal(m, m.T), (log2, mid)
    assert {lists[(2, 0)][1], lists[(2, 3)][1], lists[(3, 0)][1], lists[(3, 1)][1]}.isdisjoint({16})
    assert rr.lists_in_effect(specs["pps"]) != lists and rr.lists_in_effect(specs["pps"])[(1, 1)] != rr.lists_in_effect(specs["default"])[(1, 1)]
    for intra in (True, False):
        q = [r for r in recs if r["intra"] == intra and r["lists"]]
        assert {(r["plane"], r["n"]) for r in q} >= set(SIZES), intra
        assert any((0, 0) in r["coefs"] for r in q if r["n"] == 16) and any((0, 0) in r["coefs"] for r in q if r["n"] == 32), intra
        assert any(r["plane"] == 0 and r["levels"] and r["scaled"] == 0 for r in q), intra       # cbf_luma 1 and no coefficient left
        assert any(r["levels"] > r["scaled"] > 0 for r in q), intra
    assert any(r["job"] is not None and r["scaled"] == 0 for r in recs)


def test_job_split_has_the_counts_and_the_pairs_across_the_splits():
    recs, stats, scripts = group("job_split")
    by_pic = {}
    for r in recs:
        if r["job"] is not None:
            by_pic.setdefault(r["pic"], []).append(r)
    assert tuple(sorted(len(v) for v in by_pic.values())) == ar.JOB_COUNTS
    same = lambda a, b: (a["x"], a["y"], a["n"]) == (b["x"], b["y"], b["n"])
    for v in by_pic.values():
        assert [r["job"] for r in v] == list(range(len(v))) and all(r["scaled"] == r["levels"] > 0 for r in v)
        for cb in (7, 31):                                          # the pair across two waves' and across two workgroups' entries
            assert len(v) <= cb + 1 or (v[cb]["plane"] == 1 and v[cb + 1]["plane"] == 2 and same(v[cb], v[cb + 1])), (len(v), cb)
    assert any(len(v) > 32 for v in by_pic.values())
    assert {v[-1]["plane"] for v in by_pic.values()} == {0, 1, 2}    # lists that end on a luma block, on a Cb without its Cr, on a Cr
    assert max(len(v) for v in by_pic.values()) > 8 * 32            # more than eight workgroups: the remap over the XCDs permutes them
    content = [tuple(sorted(r["coefs"].items())) for r in recs]
    assert len(set(content)) == len(content), "two blocks with the same levels"


# ---- 5. discrimination ----------------------------------------------------------------------------------------------------------------------------
SWITCH_CASES = [("matrix_transposed", "resid_scaling_lists-sps"), ("dct_for_dst", "resid_sizes-intra"), ("dst_for_inter4", "resid_sizes-inter"),
                ("dst_for_chroma4", "resid_sizes-inter"), ("no_stage1_clip", "resid_levels"), ("no_coeff_clip", "resid_levels"),
                ("tskip_shift_6", "resid_tskip_bypass"), ("qpc_identity", "resid_qp-depth1"), ("qp_neighbours_outside_ctb", "resid_qp-depth1"),
                ("qp_prev_not_reset", "resid_qp-depth0"), ("inter32_from_intra", "resid_scaling_lists-default"), ("dc16_ignored", "resid_scaling_lists-sps")]


@pytest.mark.parametrize("switch,name", SWITCH_CASES, ids=[s[0] for s in SWITCH_CASES])
def test_a_restatement_that_is_wrong_on_purpose_differs(switch, name):
    assert sorted(s[0] for s in SWITCH_CASES) == sorted(rr.SWITCHES)
    seq, pics, data, planes, records, _ = case(name)
    wrong, _ = rr.expect(seq, pics, **{switch: True})
    differ = sum(int((a != b).sum()) for e, q in zip(planes, wrong) for a, b in zip(e, q))
    assert differ > 0, f"{switch} changes no sample of {name}"


WRITER_SWITCH_CASES = [("scan_ignored", "resid_scans"), ("hidden_sign_written", "resid_sign_hiding"), ("ctxset_not_raised", "resid_levels"),
                       ("rice_never_raised", "resid_levels"), ("csbf_wrong_neighbours", "resid_levels")]


@pytest.mark.parametrize("switch,name", WRITER_SWITCH_CASES, ids=[s[0] for s in WRITER_SWITCH_CASES])
def test_a_writer_that_is_wrong_on_purpose_is_noticed(oracle_hevc, switch, name):
    """The oracle decodes the wrong stream to another picture than the expectation, or refuses it"""
    assert sorted(s[0] for s in WRITER_SWITCH_CASES) == sorted(hw.WRITER_SWITCHES)
    seq, pics, data, planes, records, _ = case(name)
    bad = hw.write(seq, pics, **{switch: True})
    assert bad != data
    try:
        got, n, w, h = oracle_hevc.decode(bad, 1)
    except Exception:
        return
    fs = w * h * 3 // 2
    assert n != len(pics) or rr.difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], 1, planes, records) is not None
