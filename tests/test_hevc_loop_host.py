"""H.265 deblocking and SAO against clause 8.7 on the CPU: scripted streams (tests/scripted_hevc.py, cases of tests/analytic_hevc_loop.py) whose
expected pictures tests/hevc_loop_ref.py computes from the script -- no decoder computed them.

  1. the restatement's own pins: a strong and a normal luma line, a chroma line, a band sample and an edge sample worked by hand; its two tables against
     the separately kept copies of the product;
  2. the writer: deterministic, and the new streams come out as recorded (tests/golden/scripted_hevc_digests.json, keys "loop_*"; the earlier streams
     are held by the sibling modules);
  3. every case through the CPU oracle, I420 and NV12, bit for bit, and through a parse_only product handle whose syntax digest (the SAO parameters of
     every CTB among it) and unit count must be the oracle's;
  4. coverage, group by group, from the expectation's records and the writer's counters, without exemptions;
  5. discrimination: every switch of the restatement changes expected samples of a named case; every switch of the writer's new syntax makes the
     oracle differ or refuse.
The GPU half is tests/test_hevc_loop_gpu.py."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import analytic_hevc_loop as al
import hevc_loop_ref as lr
import scripted_hevc as hw
from test_analytic_host import parse_only
from test_hevc_host_parser import product_digest
from tools import streams
from util import ROOT, c_array

NAMES = sorted(al.CASES)
DIRECTIONS = ["%+d%+d" % d for d in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1), (1, -1), (-1, 1))]


@functools.lru_cache(maxsize=None)
def case(name):
    """(seq, pics, stream, expected planes, records, the writer's counters) of a case: computed once, never modified"""
    seq, pics = al.CASES[name]()
    planes, records = lr.expect(seq, pics)
    stats = {}
    return seq, pics, hw.write(seq, pics, stats), planes, records, stats


def recs(group, kind=None):
    return [r for n in al.GROUPS[group] for r in case(n)[4] if kind is None or r["kind"] == kind]


def filtered(group):
    """the luma segments of a group that went through the decisions of 8.7.2.5.3"""
    return [r for r in recs(group, "luma") if "d" in r]


def top(gap):
    return max(map(int, gap.split(",")))


@pytest.fixture(scope="module")
def oracle_hevc():
    return streams.OracleHevc()


# ---- 1. worked by hand ----------------------------------------------------------------------------------------------------------------------------
def test_the_tables_are_those_of_table_8_12():
    tables = os.path.join(ROOT, "jmcodec_amd", "csrc", "hevc_tables.h")
    assert c_array(tables, "hevc_beta_tab") == lr.BETA and c_array(tables, "hevc_tc_tab") == lr.TC
    assert (lr.BETA[15], lr.BETA[16], lr.BETA[28], lr.BETA[29], lr.BETA[51]) == (0, 6, 18, 20, 64)
    assert (lr.TC[17], lr.TC[18], lr.TC[26], lr.TC[27], lr.TC[37], lr.TC[38], lr.TC[53]) == (0, 1, 1, 2, 4, 5, 24)


def test_a_strong_and_a_normal_luma_line_worked_by_hand():
    flat = lambda v: [[v] * 4 for _ in range(4)]
    # beta 38, tC 4.  p = 100 and q = 108 flat: dp = dq = 0, d = 0 < 38; 2 * dpq = 0 < 9, |p3 - p0| + |q0 - q3| = 0 < 4, |p0 - q0| = 8 < (5 * 4 + 1) >> 1 = 10: strong.
    #   p0' = (100 + 200 + 200 + 216 + 108 + 4) >> 3 = 828 >> 3 = 103     p1' = (300 + 108 + 2) >> 2 = 102     p2' = (200 + 300 + 100 + 100 + 108 + 4) >> 3 = 101
    #   q0' = (100 + 200 + 216 + 216 + 108 + 4) >> 3 = 844 >> 3 = 105     q1' = (100 + 324 + 2) >> 2 = 106     q2' = (100 + 108 + 108 + 324 + 216 + 4) >> 3 = 107
    dec, p, q = lr.luma_segment(flat(100), flat(108), 38, 4)
    assert (dec["dE"], dec["dEp"], dec["dEq"]) == (2, 1, 1) and p[0] == [103, 102, 101, 100] and q[3] == [105, 106, 107, 108]
    # the same with tC 1: 8 >= (5 + 1) >> 1: not strong; delta = (9 * 8 - 3 * 8 + 8) >> 4 = 3 < 10: clipped to 1.  With the strong clip of tC 1 forced on
    # the strong outputs: 103 -> 100 + 2, 105 -> 108 - 2
    assert lr.luma_line([100] * 4, [108] * 4, 2, 1, 1, 1) == ([102, 102, 101, 100], [106, 106, 107, 108])
    assert lr.luma_line([100] * 4, [108] * 4, 2, 1, 1, 1, dict(strong_clip_tc=1)) == ([101, 101, 101, 100], [107, 107, 107, 108])
    # beta 38, tC 4, q = 112: |p0 - q0| = 12 >= 10: normal.  delta = (9 * 12 - 3 * 12 + 8) >> 4 = 80 >> 4 = 5, below 40, clipped to 4: p0' = 104, q0' = 108.
    #   dp = 0 < (38 + 19) >> 3 = 7: the side taps.  p: (((100 + 100 + 1) >> 1) - 100 + 4) >> 1 = 2, inside +-2: p1' = 102; q: ((112 - 112) - 4) >> 1 = -2: q1' = 110
    dec, p, q = lr.luma_segment(flat(100), flat(112), 38, 4)
    assert (dec["dE"], dec["dEp"], dec["dEq"], dec["side"]) == (1, 1, 1, 7) and p[2] == [104, 102, 100, 100] and q[1] == [108, 110, 112, 112]
    # q = 172 with tC 4: delta = (6 * 72 + 8) >> 4 = 27 < 40: filtered; q = 206: (6 * 106 + 8) >> 4 = 40: the gate, nothing changes
    assert lr.luma_line([100] * 4, [172] * 4, 1, 0, 0, 4) == ([104, 100, 100, 100], [168, 172, 172, 172])
    assert lr.luma_line([100] * 4, [206] * 4, 1, 0, 0, 4) == ([100] * 4, [206] * 4)
    # d = beta: dp0 = |104 - 200 + 100| = 4 on both sides and lines: d = 16 = beta'(26): no filter at all; beta 17: filtered
    P = [[100, 100, 104, 104]] * 4
    assert lr.luma_decisions(P, P, 16, 2)["dE"] == 0 and lr.luma_decisions(P, P, 17, 2)["dE"] == 1


def test_a_chroma_line_worked_by_hand():
    # qPL 36, cQpPicOffset 4: qPi 40 -> QpC 36 (Table 8-10: 30 .. 43 -> 29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37); Q = 36 + 2 = 38: tC 5
    assert [lr.qpc_of(i) for i in range(29, 46)] == [29, 29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39] and lr.TC[38] == 5
    # p0 100, p1 98, q0 110, q1 111, tC 3: delta = ((10 << 2) + 98 - 111 + 4) >> 3 = 31 >> 3 = 3: p0' = 103, q0' = 107; tC 2: 102, 108
    assert lr.chroma_line([100, 98], [110, 111], 3) == (103, 107) and lr.chroma_line([100, 98], [110, 111], 2) == (102, 108)
    assert lr.chroma_line([2, 0], [250, 255], 24) == (26, 226) and lr.chroma_line([250, 255], [2, 0], 24) == (226, 26)


def test_a_band_sample_and_an_edge_sample_worked_by_hand():
    # sao_band_position 30: the bands 30, 31, 0, 1 carry the offsets 1 .. 4.  250 >> 3 = 31: the second offset; 7 >> 3 = 0: the third; 16 >> 3 = 2: none
    t = lr.band_table(30)
    assert (t[250 >> 3], t[7 >> 3], t[16 >> 3], t[30]) == (2, 3, 0, 1) and sum(1 for v in t if v) == 4
    assert sum(1 for v in lr.band_table(30, dict(band_no_wrap=1)) if v) == 2
    # c 10 between 12 and 12: 2 - 1 - 1 = 0 -> 1 (a valley, + the first magnitude); 10, 10 | 12: 1 -> 2; 10 | 10, 10: 2 -> 0; 12 | 10, 12: 3; 12 | 10, 10: 4 (a peak)
    assert [lr.edge_idx(*v) for v in ((10, 12, 12), (10, 10, 12), (10, 10, 10), (12, 10, 12), (12, 10, 10))] == [1, 2, 0, 3, 4]
    assert lr.edge_values((1, 2, 3, 4)) == [0, 1, 2, -3, -4]


# ---- 2. the writer --------------------------------------------------------------------------------------------------------------------------------
def test_the_loop_streams_come_out_as_recorded():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "scripted_hevc_digests.json")))
    got = {n: hashlib.sha256(case(n)[2]).hexdigest() for n in NAMES}
    assert sorted(k for k in want if k.startswith("loop_")) == NAMES
    moved = [n for n in NAMES if got[n] != want[n]]
    assert not moved, moved


def test_writer_is_deterministic():
    for name in NAMES:
        assert hw.write(*al.CASES[name]()) == case(name)[2], name


def test_the_writer_refuses_what_the_syntax_cannot_say():
    rng = np.random.default_rng(5)
    seq = al.loop_seq(48, 32, sao=1)
    y = ("edge", 0, (1, 1, 1, 1))

    def write(ctbs, seq=seq, **kw):
        kw.setdefault("sao", (1, 1))
        return hw.write(seq, [dict(al.pcm_pic(seq, al.gradient(rng, seq), 4, **kw), sao_ctbs=ctbs)])
    on = dict(y=y, c=None)
    write([on] * 6)
    write([on, dict(merge="left"), on, dict(merge="up"), on, on])
    for bad in ([dict(merge="left")] + [on] * 5, [dict(merge="up")] + [on] * 5, [on, on, on, dict(merge="left"), on, on]):     # outside the picture
        with pytest.raises(AssertionError):
            write(bad)
    two = [dict(first=0), dict(first=4)]
    write([on, on, on, on, on, dict(merge="left")], slices=two)
    for bad in ([on, on, on, on, dict(merge="up"), on], [on, on, on, on, dict(merge="left"), on]):       # the source lies in the slice before
        with pytest.raises(AssertionError):
            write(bad, slices=two)
    with pytest.raises(AssertionError):                             # Cr with a class of its own
        write([dict(y=None, c=(("edge", 1, (1, 1, 1, 1)), ("edge", 2, (1, 1, 1, 1))))] + [on] * 5)
    with pytest.raises(AssertionError):                             # an entry for a component whose slice flag is 0
        write([on] * 6, sao=(0, 1))
    with pytest.raises(AssertionError):                             # an edge offset has no signs, a magnitude ends at 7
        write([dict(y=("edge", 0, (1, -1, 1, 1)), c=None)] + [on] * 5)
    with pytest.raises(AssertionError):
        write([dict(y=("band", 0, (8, 0, 0, 0)), c=None)] + [on] * 5)
    with pytest.raises(AssertionError):                             # slice offsets without the override; SAO flags without the SPS flag
        hw.write(seq, [al.pcm_pic(seq, al.gradient(rng, seq), 4, beta=2)])
    with pytest.raises(AssertionError):
        write([None] * 6, seq=al.loop_seq(48, 32))
    with pytest.raises(AssertionError):                             # the across flag is absent (no SAO, no deblocking) and inferred to be the PPS flag
        hw.write(seq, [al.pcm_pic(seq, al.gradient(rng, seq), 4, deblock=0, across=0)])


# ---- 3. the oracle and the host parser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_decodes_the_loop_expectation(oracle_hevc, name):
    seq, pics, data, planes, records, _ = case(name)
    for fmt in (1, 0):
        got, n, w, h = oracle_hevc.decode(data, fmt)
        assert (n, w, h) == (len(pics), seq["width"], seq["height"])
        fs = w * h * 3 // 2
        diff = lr.difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], fmt, planes, records)
        assert diff is None, f"{name} format {fmt}: {diff}"


@pytest.mark.parametrize("name", NAMES)
def test_host_parser_reads_the_oracles_syntax(oracle_hevc, name):
    seq, pics, data, planes, records, _ = case(name)
    n, errors, info, err, failed = parse_only(data, codec=1)
    assert failed is None and errors == 0 and err == "", (failed, errors, err)
    assert n == len(pics) and info == (seq["width"], seq["height"])
    want, ncu = oracle_hevc.syntax_digest(data)
    got, cus, n, errors, _ = product_digest(data)
    assert errors == 0 and (n, cus) == (len(pics), ncu)
    assert ncu == sum(1 for p in pics for _ in hw.walk(seq, p))
    assert got == want, f"{name}: host parser and oracle disagree on the syntax"


# ---- 4. coverage ----------------------------------------------------------------------------------------------------------------------------------
def test_pictures_are_small():
    for name in NAMES:
        seq, pics = case(name)[:2]
        assert seq["width"] <= 264 and seq["height"] <= 136 and len(pics) <= 12, name


@pytest.mark.parametrize("vertical", [True, False], ids=["vertical", "horizontal"])
def test_decisions_meet_every_inequality_at_its_threshold_and_every_clip_from_both_sides(vertical):
    met = set()
    for r in filtered("loop_decisions"):
        if r["vertical"] == vertical and r["bs"] == 2 and r["pcm"] == (True, True) and r["exempt"] == (False, False):
            met |= al.segment_tags(r)
    assert not set(al.DECISION_TAGS) - met, sorted(set(al.DECISION_TAGS) - met)


def test_decisions_cover_the_quantiser_range_and_both_index_clips():
    rs = filtered("loop_decisions")
    pics = [p for n in al.GROUPS["loop_decisions"] for p in case(n)[1]]
    assert {0, 51} <= {p["qp"] for p in pics}
    assert any(r["tc"] == 0 and r["beta"] == 0 for r in rs) and any(r["tc"] == 0 and r["beta"] > 0 for r in rs)
    assert {-6, 6} <= {r["beta_off"] for r in rs} and {-6, 6} <= {r["tc_off"] for r in rs}
    assert any(r["q_beta_raw"] > 51 for r in rs) and any(r["q_tc_raw"] > 53 for r in rs) and any(r["q_beta_raw"] < 0 for r in rs) and any(r["q_tc_raw"] < 0 for r in rs)
    assert any(r["q_beta"] == 51 for r in rs) and any(r["q_tc"] == 53 for r in rs)
    for vertical in (True, False):
        assert {0, 1, 2} <= {r["dE"] for r in rs if r["vertical"] == vertical}
    # a corner where both orders of filtering give different samples: within three samples of a vertical AND of a horizontal edge of the 8x8 units
    seq, pics, _, planes, _, _ = case("loop_decisions-qp")
    other, _ = lr.expect(seq, pics, horizontal_before_vertical=True)
    differ = np.argwhere(np.stack([a[0] for a in planes]) != np.stack([b[0] for b in other]))
    # (a decision reads four samples a side and holds for four lines, so the difference spreads from the corners along the edges, never off them)
    assert any((x + 3) % 8 < 6 and (y + 3) % 8 < 6 for (_, y, x) in differ) and all((x + 3) % 8 < 6 or (y + 3) % 8 < 6 for (_, y, x) in differ), len(differ)


def test_strength_meets_every_rule_at_3_and_at_4():
    rs = recs("loop_strength", "luma")
    why = {r["why"] for r in rs}
    assert {"one:near:3,0", "one:far:4,0", "one:near:0,3", "one:far:0,4", "pictures", "count", "cbf:p", "cbf:q", "cbf:both", "intra:p", "intra:q", "intra:both"} <= why, sorted(why)
    for pairing in ("straight", "crossed"):
        near = {w.split(":")[3] for w in why if w.startswith(f"two:{pairing}:near")}
        far = {w.split(":")[3] for w in why if w.startswith(f"two:{pairing}:far")}
        assert {"3,0", "0,3"} <= near and {"4,0", "0,4"} <= far, (pairing, near, far)       # each component
    # both vectors on one picture: for the straight and for the crossed pairing, x and y each at 3 (that pairing near while the other is far: bS 0) and
    # each at 4 as the ONLY component of the ONLY pair that makes the pairing far (the other pairing far as well: bS 1 -- a 3 in its place gives bS 0)
    same = [r for r in rs if r["pairs"] is not None]
    assert {"straight near", "crossed near", "both far"} <= {r["why"].split(":")[1] for r in same}
    is_far = lambda pair_gaps: any(v >= 4 for g in pair_gaps for v in g)
    assert all(r["bs"] == int(is_far(r["pairs"]["straight"]) and is_far(r["pairs"]["crossed"])) for r in same)
    for pairing, other in (("straight", "crossed"), ("crossed", "straight")):
        for c in (0, 1):
            near = [r for r in same if r["bs"] == 0 and is_far(r["pairs"][other]) and max(g[c] for g in r["pairs"][pairing]) == 3
                    and max(g[1 - c] for g in r["pairs"][pairing]) < 3]
            far = [r for r in same if r["bs"] == 1 and is_far(r["pairs"][other]) and sorted(v for g in r["pairs"][pairing] for v in g)[-2:][0] <= 3
                   and sum(1 for g in r["pairs"][pairing] if g[c] == 4) == 1 and max(g[1 - c] for g in r["pairs"][pairing]) <= 3]
            assert near and far, (pairing, "xy"[c], len(near), len(far))
    assert all(r["bs"] == {"near": 0, "far": 1}[r["why"].split(":")[-2]] for r in rs if r["why"].startswith(("one:", "two:")))
    # one picture through two indices, and through the two lists: the strength is that of one picture
    idx = lambda u: [(k, v[0]) for pu in u[4].get("pus", []) for k, v in sorted(pu.items()) if k in ("l0", "l1")]
    twice = [r for r in rs if r["why"] == "one:near:0,0" and r["cu_edge"] and idx(r["units"][0]) != idx(r["units"][1])]
    assert {tuple(k for k, _ in idx(u)) for r in twice for u in r["units"]} >= {("l0",), ("l1",)} and any(idx(r["units"][0])[0][0] == idx(r["units"][1])[0][0] for r in twice)
    # bS 1 leaves chroma alone, on the chroma grid too
    assert all(r["bs"] == 2 for r in recs("loop_strength", "chroma"))
    assert any(r["bs"] == 1 and "d" in r and r["changed"] and (r["x"] if r["vertical"] else r["y"]) % 16 == 0 for r in rs)


def test_strength_meets_every_transform_and_prediction_edge():
    rs = recs("loop_strength", "luma")
    inner = [(r, (r["x"] - r["units"][1][0]) if r["vertical"] else (r["y"] - r["units"][1][1])) for r in rs if not r["cu_edge"]]
    assert {8, 16, 32} <= {o for r, o in inner if r["transform"] and r["units"][1][3] == "inter"}
    assert {8, 16, 24} <= {o for r, o in inner if r["transform"] and r["units"][1][3] == "intra"}
    assert all((r["x"] if r["vertical"] else r["y"]) % 8 == 0 for r in rs), "an edge off the 8x8 grid"
    units = {(u[2], u[4].get("part", "NxN" if len(u[4].get("modes", ())) == 4 else "2Nx2N"), u[4].get("tu", 0)) for n in al.GROUPS["loop_strength"]
             for p in case(n)[1] for (x, y, log2, d, v) in hw.walk(case(n)[0], p) for u in [(x, y, 1 << log2, v["t"], v)] if v["t"] in ("inter", "intra")}
    assert any(n == 8 and part == "NxN" for (n, part, tu) in units) and any(n >> tu == 4 for (n, part, tu) in units)     # inner edges at 4: not in the edge set
    parts = ("2NxN", "Nx2N") + tuple(al.ai.AMP)
    assert {(n, p) for n in (16, 32) for p in parts} <= {(n, part) for (n, part, tu) in units}
    pred_only = {(r["units"][1][2], r["units"][1][4].get("part"), o) for r, o in inner if r["prediction"] and not r["transform"]}
    assert {(32, "2NxnU", 8), (32, "2NxnD", 24), (32, "nLx2N", 8), (32, "nRx2N", 24)} <= pred_only, sorted(pred_only)      # AMP at 32: on the grid
    assert not any(n == 16 and part in al.ai.AMP for (n, part, o) in pred_only)                                        # AMP at 16: at 4 and 12, off the grid
    assert any(r["prediction"] and r["units"][1][2] == 16 and r["units"][1][4].get("part") in ("2NxN", "Nx2N") and o == 8 for r, o in inner)
    assert {r["ctb"] for r in rs} == {4, 5, 6}


def test_qp_cases_meet_every_source_of_a_quantiser():
    rs = filtered("loop_qp")
    assert any((r["qp"][0] + r["qp"][1]) % 2 == 1 and r["changed"] for r in rs) and any(r["qp"][0] != r["qp"][1] and (r["qp"][0] + r["qp"][1]) % 2 == 0 for r in rs)
    kinds = lambda r: (r["units"][0][3], r["units"][1][3])
    assert any(kinds(r) == ("skip", "intra") and r["qp"][0] != r["qp"][1] and "dqp" in r["units"][1][4] for r in rs)   # the skipped unit in front of the delta: the predicted QP
    assert any(kinds(r) == ("skip", "skip") and r["qp"][0] != r["qp"][1] for r in recs("loop_qp", "luma"))                # ... and the one behind it: the group's QP
    for name in al.GROUPS["loop_qp"]:
        seq, pics, _, _, records, _ = case(name)
        pcm = [r for r in records if r["kind"] == "luma" and "d" in r and r["pcm"][0] != r["pcm"][1]]
        assert any(r["qp"][0] != r["qp"][1] for r in pcm)
        assert any(r["qp"][i] not in (0, pics[r["pic"]]["qp"]) for r in pcm for i in (0, 1) if r["pcm"][i]), "a PCM unit has the predicted QP"
        assert seq["cb_qp_offset"] != seq["cr_qp_offset"] and any(p.get("cb_qp_offset") for p in pics) and any(p.get("cr_qp_offset") for p in pics)
    assert {(True, False), (False, True), (True, True)} <= {r["bypass"] for r in rs}
    chroma = recs("loop_qp", "chroma")
    assert any(r["qpi"] < 30 for r in chroma) and any(30 <= r["qpi"] <= 43 for r in chroma) and any(r["qpi"] > 43 for r in chroma)
    at = {}
    for r in chroma:
        at.setdefault((r["pic"], r["vertical"], r["x"], r["y"]), {})[r["plane"]] = r["qpi"]
    assert all(v[1] + 14 == v[2] for v in at.values() if len(v) == 2)
    # PCM units under pcm_loop_filter_disabled_flag 1, on each side, for the strong and the normal luma filter and for chroma
    seq, _, _, _, records, _ = case("loop_qp-depth0-pcm_exempt")
    assert seq["pcm_loop_filter_disabled"] == 1 and case("loop_qp-depth1-pcm_filtered")[0]["pcm_loop_filter_disabled"] == 0
    for side in ((True, False), (False, True)):
        luma = [r for r in records if r["kind"] == "luma" and "d" in r and r["pcm"] == side and r["bypass"] == (False, False)]
        assert all(r["exempt"] == side for r in luma) and {1, 2} <= {r["dE"] for r in luma if r["changed"]}, side
        assert any(r["exempt"] == side and r["changed"] for r in records if r["kind"] == "chroma")
    both = [r for r in records if r["kind"] == "luma" and "d" in r and r["pcm"] == (True, True)]
    assert all(r["exempt"] == (True, True) and not r["changed"] for r in both) and {1, 2} <= {r["dE"] for r in both}
    assert any(r["exempt"] == (True, True) and not r["changed"] and r["hit"] for r in records if r["kind"] == "chroma")
    assert not any(r["exempt"] != r["bypass"] for r in case("loop_qp-depth1-pcm_filtered")[4] if r["kind"] == "luma" and "d" in r)


def test_slices_meet_every_flag_on_both_sides_of_a_boundary():
    seq, pics, _, _, records, stats = case("loop_slices")
    luma = [r for r in records if r["kind"] == "luma"]
    assert pics[0]["layout"] == "ctb" and pics[1]["layout"] == "row"
    at = lambda k, sl, vertical: [r for r in luma if r["pic"] == k and r["slices"] == sl and r["vertical"] == vertical]
    for vertical in (True, False):
        assert at(2, (0, 1), vertical) and all(r["off"] == "disabled" for r in at(2, (0, 1), vertical) + at(2, (1, 1), vertical))       # disabled between enabled neighbours
        assert at(2, (1, 2), vertical) and all(r["off"] is None and r["changed"] is not None for r in at(2, (1, 2), vertical) if "d" in r)
        for k, (earlier, later) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            edge = at(5 + k, (0, 1), vertical)
            assert edge and all((r["off"] == "slice") == (later == 0) for r in edge), (earlier, later, vertical)
            assert all(r["off"] is None for r in luma if r["pic"] == 5 + k and r["slices"][0] == r["slices"][1])
        assert {r["beta_off"] for r in at(3, (0, 1), vertical)} == {5} and {r["tc_off"] for r in at(3, (0, 1), vertical)} == {-4}      # the slice that holds q0,0
        assert {(r["beta_off"], r["tc_off"]) for r in at(3, (0, 0), vertical)} == {(-3, 2)}
        assert {(r["beta_off"], r["tc_off"]) for r in at(4, (0, 0), vertical)} == {(2, -2)} == {(seq["pps_beta"], seq["pps_tc"])}       # inherited
        assert {(r["beta_off"], r["tc_off"]) for r in at(4, (0, 1), vertical) + at(4, (1, 1), vertical)} == {(-4, 4)}                        # overridden
    assert any(r["changed"] for r in luma if r["pic"] == 0 and r["slices"][0] != r["slices"][1])
    assert stats[("slice", "across", 0, "coded")] and stats[("slice", "across", 1, "coded")] and stats[("slice", "override", True, True)]


def test_sao_cases_meet_every_type_class_category_and_border():
    rs = recs("loop_sao", "sao")
    band, edge = [r for r in rs if r["type"] == "band"], [r for r in rs if r["type"] == "edge"]
    for plane in (0, 1, 2):
        assert set(al.BAND_POSITIONS) <= {r["where"] for r in band if r["plane"] == plane}, plane
    wrapped = [r for r in band if r["where"] in (29, 31)]
    assert any(set(r["counts"]) & {1, 2, 3} and 4 in r["counts"] for r in wrapped), "a band table that wraps, met on both sides of the wrap"
    assert any(0 in r["counts"] and len(r["counts"]) > 1 for r in band)                                # samples on both sides of a band limit
    assert {"<0", ">255"} <= {s for r in band if {7, -7} & set(r["offsets"]) for s in r["sat"]}
    assert {"<0", ">255"} <= {s for r in edge if 7 in r["offsets"] for s in r["sat"]}
    for plane in (0, 1, 2):
        for cls in range(4):
            met = {c for r in edge if r["where"] == cls and r["plane"] == plane and all(r["offsets"]) for c in r["counts"]}
            assert met == {0, 1, 2, 3, 4}, (plane, cls, met)
    for name in al.GROUPS["loop_sao"]:
        seq, pics, _, _, records, _ = case(name)
        cw, ch = hw.ctb_dims(seq)
        border = {(r["ctb"] % cw == 0, r["ctb"] % cw == cw - 1, r["ctb"] // cw == 0, r["ctb"] // cw == ch - 1) for r in records if r["kind"] == "sao" and "picture" in r["blocked"]}
        assert all(any(b[i] for b in border) for i in range(4)), name
    assert {"left", "up"} <= {r["merged"] for r in rs}
    chained, between = [], {0: [], 1: []}
    for name in al.GROUPS["loop_sao"]:
        seq, pics = case(name)[:2]
        cw = hw.ctb_dims(seq)[0]
        plans = hw.plan(seq, pics)
        for k, p in enumerate(pics):
            script = [e or {} for e in p["sao_ctbs"]]
            source = lambda a: a - 1 if script[a]["merge"] == "left" else a - cw
            chained += [(name, k, a) for a, e in enumerate(script) if e.get("merge") and script[source(a)].get("merge")]
            M = lr.Maps(seq, pics, k, plans, {}, {})
            params = lr.sao_params(M)                               # merges followed, slice flags applied
            for a in range(1, len(params) - 1):
                if a % cw in (0, cw - 1):
                    continue                                        # both neighbours in the CTB's own row
                for c in (0, 1):
                    if M.slices[M.slice_no[a]]["sao"][c] and params[a][c] is None and params[a - 1][c] is not None and params[a + 1][c] is not None:
                        between[c].append((name, k, a))
    assert chained, "a merge of a CTB that is itself merged"
    assert between[0] and between[1], "a CTB with SaoTypeIdx 0, in a slice with the flag on, between CTBs of its row with SAO -- luma and chroma"
    flags = {tuple(sl["sao"]) for n in al.GROUPS["loop_sao"] for p in case(n)[1] for sl in hw.slice_table(case(n)[0], p)}
    assert {(1, 1), (1, 0), (0, 1), (0, 0)} <= flags
    assert any(len({tuple(sl["sao"]) for sl in hw.slice_table(case(n)[0], p)}) > 1 for n in al.GROUPS["loop_sao"] for p in case(n)[1])
    by_ctb = {}
    for r in edge:
        by_ctb.setdefault((r["pic"], r["ctb"], r["x"], r["y"], r["where"]), {})[r["plane"]] = r["offsets"]
    assert any(v.get(1) and v.get(2) and v[1] != v[2] for v in by_ctb.values())                         # Cr with offsets of its own under Cb's class
    assert any(r["plane"] == 2 and r["type"] == "band" for r in band) and len({(r["pic"], r["ctb"], r["where"]) for r in band if r["plane"] in (1, 2)}) > len({(r["pic"], r["ctb"]) for r in band if r["plane"] == 1})
    # neighbouring samples that SAO itself changes: filtering in place gives other samples
    seq, pics, _, planes, _, _ = case("loop_sao-8x32")
    in_place, _ = lr.expect(seq, pics, sao_in_place=True)
    assert sum(int((a != b).sum()) for e, q in zip(planes, in_place) for a, b in zip(e, q)) > 0
    # deblocking off and on under SAO
    off_on = {hw.slice_table(case(n)[0], p)[0]["disabled"] for n in al.GROUPS["loop_sao"] for p in case(n)[1] if any(hw.slice_table(case(n)[0], p)[0]["sao"])}
    assert off_on == {True, False}
    # exempt units of 8x8 inside CTBs that SAO changes
    seq, pics, _, _, records, _ = case("loop_sao-exempt")
    units = {(v["t"], bool(v.get("bypass")), log2) for p in pics for (_, _, log2, _, v) in hw.walk(seq, p)}
    assert {("pcm", False, 3), ("intra", True, 3)} <= units and seq["pcm_loop_filter_disabled"] == 1
    for plane in (0, 1, 2):
        assert any("exempt" in r["blocked"] and r["changed"] for r in records if r["kind"] == "sao" and r["plane"] == plane), plane
    # geometry
    sizes = {(case(n)[0]["width"], case(n)[0]["ctb_log2"]) for n in al.GROUPS["loop_sao"]}
    assert {8, 72, 88, 264} <= {w for w, _ in sizes} and {4, 5, 6} <= {c for _, c in sizes}
    counters = {}
    for n in al.GROUPS["loop_sao"]:
        for key, v in case(n)[5].items():
            counters[key] = counters.get(key, 0) + v
    assert all(counters.get(("sao", "abs", v)) for v in range(8)) and counters[("sao", "sign", 0)] and counters[("sao", "sign", 1)]
    assert all(counters.get(("sao", "type", c, t)) for c in (0, 1, 2) for t in (0, 1, 2)) and all(counters.get(("sao", "class", c, k)) for c in (0, 1) for k in range(4))
    assert all(counters.get(("sao", m, v)) for m in ("merge_left", "merge_up") for v in (0, 1)) and not any(key[:3] == ("sao", "class", 2) for key in counters)


def test_sao_slices_meet_every_direction_across_a_boundary_under_both_flags():
    for name, blocked_pair, open_pair in (("loop_sao_slices-later0", (0, 1), (1, 2)), ("loop_sao_slices-earlier0", (1, 2), (0, 1))):
        seq, pics, _, _, records, _ = case(name)
        tables = [hw.slice_table(seq, p) for p in pics]
        assert all([sl["first"] for sl in t] == [0, 5, 10] for t in tables)                            # slices that begin in mid-row
        assert all(t[blocked_pair[1]]["across"] == 0 and t[open_pair[1]]["across"] == 1 for t in tables)
        assert all(t[open_pair[0]]["across"] == 0 or open_pair[0] != 1 for t in tables)                  # 5 | 10: the EARLIER slice's flag is 0 and does not count
        tags = {t for r in records if r["kind"] == "sao" for t in r["blocked"]}
        for d in DIRECTIONS:
            assert any(t.startswith("slice:" + d) for t in tags) and "across:" + d in tags, (name, d, sorted(tags))
        for r in records:
            if r["kind"] == "sao":
                assert all(t.startswith("across") or t == "picture" or r["slice"] in blocked_pair for t in r["blocked"]), r["blocked"]
        assert {r["where"] for r in records if r["kind"] == "sao"} == {0, 1, 2, 3}


def test_reference_and_launch_cases_are_what_they_are_meant_to_be():
    seq, pics, _, planes, records, _ = case("loop_reference")
    assert [p["kind"] for p in pics] == ["I", "P", "B"]
    for k in (0, 1):                                                # both references were changed by both filters
        assert sum(r.get("changed") or 0 for r in records if r["pic"] == k and r["kind"] in ("luma", "chroma")) > 0
        assert sum(r["changed"] for r in records if r["pic"] == k and r["kind"] == "sao") > 0
    mvs = [pu[l][1] for p in pics[1:] for u in p["cus"] for pu in u["pus"] for l in ("l0", "l1") if l in pu]
    assert any(v != (0, 0) and v[0] % 4 == 0 and v[1] % 4 == 0 for v in mvs) and any(v[0] % 4 and v[1] % 4 for v in mvs) and any(v[0] % 4 and not v[1] % 4 for v in mvs)
    sizes = {(case(n)[0]["width"], case(n)[0]["height"]) for n in al.GROUPS["loop_launch"]}
    assert {(64, 128), (64, 120), (72, 120), (64, 136)} <= sizes
    seq, pics, _, _, records, _ = case("loop_launch-alternate")
    modes = [(hw.slice_table(seq, p)[0]["disabled"], hw.slice_table(seq, p)[0]["sao"]) for p in pics]
    assert len(set(modes)) >= 5 and all(a[0] != b[0] for a, b in zip(modes, modes[1:]))


# ---- 5. discrimination ----------------------------------------------------------------------------------------------------------------------------
SWITCH_CASES = [("horizontal_before_vertical", "loop_decisions-qp"), ("tc_without_bs_term", "loop_decisions-qp"), ("offsets_of_p_slice", "loop_slices"),
                ("qp_sum_without_plus_1", "loop_qp-depth1-pcm_filtered"), ("pcm_qp_zero", "loop_qp-depth1-pcm_filtered"),
                ("chroma_uses_slice_qp_offset", "loop_qp-depth1-pcm_filtered"), ("chroma_at_bs1", "loop_strength-p"), ("chroma_on_luma_grid", "loop_decisions-qp"),
                ("dE_side_thresholds_swapped", "loop_decisions-vertical"), ("no_10tc_gate", "loop_decisions-horizontal"), ("strong_clip_tc", "loop_decisions-vertical"),
                ("edges_on_4_grid", "loop_strength-intra"), ("across_flag_of_earlier_slice", "loop_slices"), ("disabled_by_p_slice", "loop_slices"),
                ("sao_before_deblock", "loop_sao-72x40"), ("sao_in_place", "loop_sao-8x32"), ("band_no_wrap", "loop_sao-264x24"), ("edge_idx_unmapped", "loop_sao-88x72"),
                ("edge_signs_plus_minus_swapped", "loop_sao-8x32"), ("cr_own_class", "loop_sao-72x40"), ("sao_at_picture_border", "loop_sao-8x32"),
                ("sao_ignores_exempt_units", "loop_sao-exempt"), ("sao_flag_of_earlier_slice", "loop_sao_slices-later0"), ("reference_is_unfiltered", "loop_reference")]


@pytest.mark.parametrize("switch,name", SWITCH_CASES, ids=[s[0] for s in SWITCH_CASES])
def test_a_restatement_that_is_wrong_on_purpose_differs(switch, name):
    assert sorted(s[0] for s in SWITCH_CASES) == sorted(lr.SWITCHES)
    assert name in NAMES
    seq, pics, data, planes, records, _ = case(name)
    wrong, _ = lr.expect(seq, pics, **{switch: True})
    differ = sum(int((a != b).sum()) for e, q in zip(planes, wrong) for a, b in zip(e, q))
    assert differ > 0, f"{switch} changes no sample of {name}"


WRITER_SWITCH_CASES = [("across_tied_to_deblock", "loop_sao-72x40"), ("sao_edge_signs_coded", "loop_sao-8x32"), ("sao_type_second_bin_context", "loop_sao-8x32"),
                       ("sao_cr_class_coded", "loop_sao-72x40"), ("sao_up_after_left", "loop_sao-72x40"), ("sao_abs_cmax_31", "loop_sao-8x32")]


@pytest.mark.parametrize("switch,name", WRITER_SWITCH_CASES, ids=[s[0] for s in WRITER_SWITCH_CASES])
def test_a_writer_that_is_wrong_on_purpose_is_noticed(oracle_hevc, switch, name):
    """The oracle decodes the wrong stream to another picture than the expectation, or refuses it"""
    assert sorted(s[0] for s in WRITER_SWITCH_CASES) == sorted(hw.LOOP_WRITER_SWITCHES)
    seq, pics, data, planes, records, _ = case(name)
    bad = hw.write(seq, pics, **{switch: True})
    assert bad != data
    try:
        got, n, w, h = oracle_hevc.decode(bad, 1)
    except Exception:
        return
    fs = w * h * 3 // 2
    assert n != len(pics) or lr.difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], 1, planes, records) is not None
