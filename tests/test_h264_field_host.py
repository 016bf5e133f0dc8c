"""H.264 field pictures, the CPU half: what tests/h264_field_ref.py restates is pinned by hand-worked values, every scripted case of
tests/analytic_h264_field.py is held to the CPU oracle bit for bit and to the product's parser (parse_only), every wrong-on-purpose switch is noticed
by a named case, and every case covers what it is there for.  tests/test_h264_field_gpu.py holds the product's pictures to the same expectations.

No tolerances: the expected pictures are integers from the clauses."""
import numpy as np
import pytest

import analytic_expect as ae
import analytic_h264_field as hf
import analytic_h264_recon as hr
import deblock_ref
import h264_field_ref as fr
import scripted_h264 as sw
from jmcodec_amd import api
from spec_tables_h264 import FIELD_SCAN_4x4, FIELD_SCAN_8x8, ZIGZAG_4x4, ZIGZAG_8x8
from test_h264_recon_host import stored_coefficients

CASES = [(n, s) for n in sorted(hf.CASES) for s in hf.case_sizes(n)]
IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]


# ---- 1. by hand ---------------------------------------------------------------------------------------------------------------------------------
def lines(n, w=8):
    """a store whose line y holds 10 y everywhere"""
    return np.tile((10 * np.arange(n))[:, None], (1, w)).astype(np.uint8)


def test_cross_parity_chroma_sample_at_the_field_border_by_hand():
    """Table 8-9 with 8-270.  A top field predicts from the bottom field, vector 0: the chroma vector is -2, so yIntC = -1 and yFracC = 6; field lines -1
    and 0 are both the bottom field's line 0 after the clamp = store line 1 = 10: (2 * 10 + 6 * 10) / 8 = 10.  With the sign swapped: +2, lines 0 and 1
    of the field = store lines 1 and 3: (6 * 10 + 2 * 30 + 4) >> 3 = 15.  A bottom field predicts its last chroma line (field line 3 of 4) from the top
    field: +2, lines 3 and 4 -> 3 and 3 = store line 6 = 60; a clamp at the FRAME's border would read store line 7 for the second: (6 * 60 + 2 * 70 +
    4) >> 3 = 63."""
    S = lines(8)
    assert fr.chroma_mvy_offset("top", "bottom") == -2 and fr.chroma_mvy_offset("bottom", "top") == 2
    assert fr.chroma_mvy_offset("top", "top") == fr.chroma_mvy_offset("bottom", "bottom") == fr.chroma_mvy_offset(None, None) == 0
    assert ae.mc_chroma(fr.FieldRef(S, "bottom"), 0, 0, 1, 1, (0, -2))[0, 0] == 10
    assert ae.mc_chroma(fr.FieldRef(S, "bottom"), 0, 0, 1, 1, (0, fr.chroma_mvy_offset("top", "bottom", {"chroma_parity_offset_sign"})))[0, 0] == 15
    assert ae.mc_chroma(fr.FieldRef(S, "top"), 0, 3, 1, 1, (0, 2))[0, 0] == 60
    assert ae.mc_chroma(fr.FieldRef(S, "top", {"clamp_at_frame_border"}), 0, 3, 1, 1, (0, 2))[0, 0] == 63


def test_luma_window_past_the_bottom_of_the_field_by_hand():
    """A store of 16 lines: its top field has lines 0, 20 .. 140.  Two lines down from field lines 6, 7: lines 8, 9, clamped to 7: 140, 140.  The half
    sample below field line 7 (vector (0, 2)): taps on lines 5 .. 10 = 100, 120, 140, 140, 140, 140: 100 - 600 + 2800 + 2800 - 700 + 140 = 4540,
    (4540 + 16) >> 5 = 142.  The bottom field's line -1 is its line 0 = store line 1 = 10, not the store's line 0."""
    S = lines(16, 16)
    assert ae.mc_luma(fr.FieldRef(S, "top"), 0, 6, 4, 2, (0, 8)).tolist() == [[140] * 4] * 2
    assert ae.mc_luma(fr.FieldRef(S, "top"), 0, 7, 4, 1, (0, 2)).tolist() == [[142] * 4]
    assert ae.mc_luma(fr.FieldRef(S, "bottom"), 0, 0, 4, 1, (0, -4)).tolist() == [[10] * 4]
    assert ae.mc_luma(fr.FieldRef(S, "bottom", {"clamp_at_frame_border"}), 0, 0, 4, 1, (0, -4)).tolist() == [[0] * 4]


def test_field_list_of_three_stores_by_hand():
    """8.2.4.2.5.  Stores by descending FrameNumWrap: the current frame's (its first field, a top field, alone), one with both fields, one with both.
    The second field (bottom) starts with its own parity: b1, t2, b0, t1, and top is left over: t0.  A top field over the same stores: t2, b1, t1, b0,
    t0.  Both typings (the writer's and the restatement's) say so."""
    order = [dict(top="t2"), dict(top="t1", bottom="b1"), dict(top="t0", bottom="b0")]
    for f in (sw.alternate_fields, fr.interleave):
        assert f(order, "bottom") == ["b1", "t2", "b0", "t1", "t0"] and f(order, "top") == ["t2", "b1", "t1", "b0", "t0"]
        assert f([dict(bottom="b1"), dict(top="t0")], "top") == ["t0", "b1"] and f([dict(bottom="b1")], "top") == ["b1"]
    assert fr.interleave(order, "bottom", {"field_list_starts_other_parity"}) == ["t2", "b1", "t1", "b0", "t0"]
    assert fr.interleave(order, "bottom", {"field_list_no_alternation"}) == ["t2", "b1", "t1", "b0", "t0"]
    assert fr.interleave(order[1:], "bottom", {"field_list_no_alternation"}) == ["b1", "t1", "b0", "t0"]


def test_implicit_weight_from_field_counts_by_hand():
    """8.4.2.3.1 with reference fields of counts 0 and 8: td = 8, tx = (16384 + 4) / 8 = 2048.  The top field of count 2: tb = 2, DistScaleFactor =
    (2 * 2048 + 32) >> 6 = 64, w1 = 16, w0 = 48.  The bottom field of the same frame, count 3: (3 * 2048 + 32) >> 6 = 96, w1 = 24, w0 = 40.  One field
    through both lists: td = 0, (32, 32)."""
    assert ae.implicit_weights(2, 0, 8) == (48, 16) and ae.implicit_weights(3, 0, 8) == (40, 24) and ae.implicit_weights(3, 1, 1) == (32, 32)


def test_boundary_strength_field_rules_by_hand():
    assert fr.intra_edge_bs(True, True) == 3 and fr.intra_edge_bs(True, False) == 4 and fr.intra_edge_bs(False, True) == fr.intra_edge_bs(False, False) == 4
    one = lambda ref, mv: [(ref, mv)]
    assert fr.mvy_limit(True) == 2 and fr.mvy_limit(False) == 4
    assert deblock_ref.motion_bs(one(0, (0, 0)), one(0, (3, 1)), fr.mvy_limit(True)) == 0
    assert deblock_ref.motion_bs(one(0, (0, 0)), one(0, (0, 2)), fr.mvy_limit(True)) == 1
    assert deblock_ref.motion_bs(one(0, (0, 0)), one(0, (0, 3)), fr.mvy_limit(False)) == 0 and deblock_ref.motion_bs(one(0, (0, 0)), one(0, (0, 4))) == 1
    pics = [dict(field="top"), dict(field="bottom")]
    key = fr.reference_key(pics, True)
    assert deblock_ref.motion_bs(one(key(0), (0, 0)), one(key(1), (0, 0)), 2) == 1, "the two fields of a frame are two reference pictures"
    key = fr.reference_key(pics, True, {"fields_of_one_frame_same_reference"})
    assert deblock_ref.motion_bs(one(key(0), (0, 0)), one(key(1), (0, 0)), 2) == 0


def test_field_scans_differ_from_zigzag_everywhere_but_at_the_ends():
    d4, d8 = hf.scan_positions_that_differ()
    assert d4 == [1, 2] + list(range(4, 15)) and d8[0] == 1 and d8[-1] == 62 and len(d8) >= 56      # (0, 2) is third in both 4x4 scans
    p4, p8 = fr.decoder_scans(True)
    assert p4 == list(range(16)) and p8 == list(range(64)) and fr.decoder_scans(False) is None
    w4, w8 = fr.decoder_scans(True, {"zigzag_in_field_4x4", "zigzag_in_field_8x8"})
    assert w4[ZIGZAG_4x4[1]] == FIELD_SCAN_4x4[1] and w8[ZIGZAG_8x8[5]] == FIELD_SCAN_8x8[5] and w4 != p4 and w8 != p8


def test_both_typings_of_the_lists_agree_on_every_case():
    for name, size in CASES:
        seq, pics = hf.scripted(name, size)[:2]
        for k, (pl, (l0, l1)) in enumerate(zip(sw.plan(seq, pics), fr.decoder_lists(seq, pics))):
            assert pl["l0"] == l0[:len(pl["l0"])] and pl["l1"] == l1[:len(pl["l1"])], (name, k, pl, l0, l1)


def test_writer_refuses_what_it_cannot_state():
    rng = np.random.default_rng(1)
    top, bot = hf.noise_field(rng, 1, 1, "top", 0), hf.noise_field(rng, 1, 1, "bottom", 1, kind="P")
    seq = hf.base_seq(16, 32)
    lone_then_frame = [top, dict(kind="P", poc=2, mbs=[dict(t="16x16", l0=(0, (0, 0)))] * 2)]
    with pytest.raises(AssertionError):
        sw.write(seq, lone_then_frame)                              # a frame naming a store with one field (and a first field not followed by its pair)
    far_field = [top, bot, dict(kind="P", poc=2, field="top", num_ref=(1, 1), mbs=[dict(t="16x16", l0=(1, (0, 0)))])]
    with pytest.raises(AssertionError):
        sw.write(seq, far_field)                                    # a field naming a field that is not in its (cut) list
    with pytest.raises(AssertionError):
        sw.sps(dict(seq, height=30))                                # (coded_height - height) % 4 != 0 with frame_mbs_only_flag 0


# ---- 2. the oracle and the host parser ----------------------------------------------------------------------------------------------------------
def n_frames(pics):
    return len(fr.output_frames(pics, [()] * len(pics)))


@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_oracle_decodes_the_restated_expectation(oracle, name, size):
    seq, pics, data, planes, _, _ = hf.scripted(name, size)
    assert data == sw.write(*hf.CASES[name](*size)), "the case builder and the writer are deterministic"
    for fmt in (1, 0):
        got, n, w, h = oracle.decode(data, fmt)
        assert (n, w, h) == (n_frames(pics), size[0], size[1])
        fs = w * h * 3 // 2
        diff = ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], fmt, planes)
        assert diff is None, f"{name} {size} format {fmt}: {diff}"


@pytest.mark.parametrize("name", ["paff_mixed", "paff_mixed_sparse", "field_scan_levels", "field_p_parities"])
def test_oracle_decodes_the_cases_with_deblocking_on(oracle, name):
    """The variants with the filter on in every picture (the GPU test feeds the paff_mixed ones through chain launches): intra macroblocks with levels
    beside inter ones in fields and frames, coded inter blocks under both transforms in a field, vectors of every fraction across parities"""
    seq, pics, data, planes, stats = hf.scripted_deblocked(name)
    raw = hf.scripted(name)[3]
    assert any(not np.array_equal(a, b) for P, Q in zip(planes, raw) for a, b in zip(P, Q))
    assert stats.get("H:field_intra_mb_edge_bS3", 0) > 0 or name == "field_p_parities"
    got, n, w, h = oracle.decode(data, 1)
    fs = w * h * 3 // 2
    diff = ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], 1, planes)
    assert n == n_frames(pics) and diff is None, f"{name}: {diff}"


@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_host_parser_accepts_the_stream_and_counts_what_the_script_implies(name, size):
    seq, pics, data, _, _, _ = hf.scripted(name, size)
    fields, lone = fr.counts(pics)
    with api.JmAmdDec(0, 1, options={"parse_only": 1}) as d:
        n = d.decode_stream(data, keep=False)
        assert d.stat("errors") == 0 and api.lib().jm_amddec_last_error(d.h).decode() == ""
        assert n == n_frames(pics) and api.jm_nvdec_stream_info(d.h) == size
        assert d.stat("field_pictures") == fields and d.stat("lone_fields") == 0 and lone == name.startswith("field_lone")      # (counted only when a picture follows)
        assert d.stat("intra_mbs") == sum(i for i, _ in hr.intra_counts(seq, pics))
        assert d.stat("coef_int16") == sum(stored_coefficients(m) for p in pics for m in p["mbs"])


REACH = {   # the oracle's tool counters that a case is there to reach (beside field-pictures / second-fields, held to the script for every case)
    "field_p_parities": ["cross-parity-blocks"], "field_p_borders": ["cross-parity-blocks"], "field_p_lists": ["cross-parity-blocks"],
    "field_b": ["b-field-pictures", "cross-parity-blocks"], "field_b_implicit": ["b-field-pictures"], "field_b_explicit": ["b-field-pictures"],
    "paff_mixed": ["cross-parity-blocks"], "field_deblock_intra": ["field-bS3"], "field_deblock_inter": ["field-bS3", "field-mvy-limit"],
    "field_deblock_b": ["field-mvy-limit", "b-field-pictures"],}


@pytest.mark.parametrize("name", sorted(hf.CASES))
def test_oracle_tool_counters_confirm_the_reach(oracle, name):
    seq, pics, data = hf.scripted(name)[:3]
    tools = oracle.tools(data)
    st = fr.structure(pics)
    fields, lone = fr.counts(pics)
    assert tools.get("field-pictures", 0) == fields and tools.get("second-fields", 0) == sum(q[2] for q in st) and tools.get("lone-fields", 0) == 0
    assert tools.get("b-field-pictures", 0) == sum(1 for p in pics if p["kind"] == "B" and p.get("field"))
    for tool in REACH.get(name, []):
        assert tools.get(tool, 0) > 0, (name, tool, tools)


# ---- 3. wrong on purpose ------------------------------------------------------------------------------------------------------------------------
NOTICED_BY = {
    "clamp_at_frame_border": "field_p_borders", "no_chroma_parity_offset": "field_p_parities", "chroma_parity_offset_sign": "field_p_parities",
    "zigzag_in_field_4x4": "field_scan_levels", "zigzag_in_field_8x8": "field_scan_levels", "field_list_starts_other_parity": "field_p_lists",
    "field_list_no_alternation": "field_p_lists", "current_frames_first_field_not_listed": "field_p_lists",
    "implicit_weights_from_frame_poc": "field_b_implicit", "bs4_on_horizontal_field_edge": "field_deblock_intra",
    "frame_mvy_limit_in_field": "field_deblock_inter", "fields_of_one_frame_same_reference": "field_deblock_inter",
    "deblock_across_parities": "field_deblock_intra", "weave_swapped": "field_pcm_weave", "intra_neighbour_from_other_parity": "field_intra"}


def test_every_switch_has_a_named_case():
    assert set(NOTICED_BY) == set(fr.SWITCHES)


@pytest.mark.parametrize("switch", fr.SWITCHES)
def test_wrong_on_purpose_is_noticed_by_its_named_case(switch):
    """A decoder with this defect hands out other frames for the named case: the case fails on it."""
    name = NOTICED_BY[switch]
    seq, pics, _, planes, _, _ = hf.scripted(name)
    right = ae.expected_frames(seq, pics, 1, planes)
    wrong = ae.expected_frames(seq, pics, 1, ae.expect_h264(seq, pics, wrong={switch}), wrong={switch})
    assert len(right) == len(wrong) and right != wrong, f"{switch} does not show in {name}"
    differing = sum(a != b for a, b in zip(right, wrong))
    assert differing >= 1


# ---- 4. the cases cover what they are there for -------------------------------------------------------------------------------------------------
def parts_of(pics):
    """(picture index, macroblock address, x, y, w, h, name, vector) of every list-0 partition of every field picture"""
    for k, p in enumerate(pics):
        if not p.get("field"):
            continue
        for a, m in enumerate(p["mbs"]):
            if m["t"] in ("16x16", "16x8", "8x16"):
                for (px, py, w, h, l0, l1) in ae.partitions(m):
                    if l0 is not None:
                        yield k, a, px, py, w, h, l0[0], l0[1]


def test_pcm_weave_has_both_field_orders_and_a_frame_after_a_pair():
    seq, pics = hf.scripted("field_pcm_weave")[:2]
    st = fr.structure(pics)
    firsts = [pics[k]["field"] for k in range(len(pics)) if st[k][1] and not st[k][2]]
    assert "top" in firsts and "bottom" in firsts and any(st[k][2] and not st[k + 1][1] for k in range(len(pics) - 1))
    assert ae.display_order(pics) == [0, 2, 4, 6, 7]


def test_field_intra_covers_every_mode_of_every_kind_in_every_layout():
    for size in hf.case_sizes("field_intra"):
        seq, pics, _, _, cov, _ = hf.scripted("field_intra", size)
        assert {p["layout"] for p in pics} == {"pic", "row", "mb"} and {p["field"] for p in pics} == {"top", "bottom"}
        if size[0] > 16:
            assert {q[3] for q in cov if q[0] == "mode" and q[1] == 4} == set(range(9)) and {q[3] for q in cov if q[0] == "mode" and q[1] == 8} == set(range(9))
            assert {q[1] for q in cov if q[0] == "i16"} == {0, 1, 2, 3} and {q[2] for q in cov if q[0] == "i16"} == {0, 1, 2, 3}
        assert {q[1] for q in cov if q[0] == "residual"} == {4, 8}
        assert all("coef" in m for p in pics for m in p["mbs"] if m["t"] in ("i4", "i8"))


def test_scan_case_has_a_single_level_at_every_position_where_the_scans_differ():
    seq, pics = hf.scripted("field_scan_levels")[:2]
    d4, d8 = hf.scan_positions_that_differ()
    singles = {"y": set(), "y8": set(), "ydc": set(), "cac": set(), "y8_inter": set(), "y_i16": set()}
    for p in pics:
        for m in p["mbs"]:
            c = m.get("coef", {})
            for key in ("y", "y8", "cac"):
                for lv in c.get(key, {}).values():
                    nz = [i for i, v in enumerate(lv) if v]
                    if len(nz) == 1:
                        singles[("y8_inter" if m["t"] == "16x16" else "y8") if key == "y8" else ("y_i16" if key == "y" and m["t"] == "i16" else key)].add(nz[0])
            if "ydc" in c and sum(1 for v in c["ydc"] if v) == 1:
                singles["ydc"].add([i for i, v in enumerate(c["ydc"]) if v][0])
    raster4, raster8 = {FIELD_SCAN_4x4[k] for k in d4}, {FIELD_SCAN_8x8[k] for k in d8}
    assert raster4 <= singles["y"] and raster4 <= singles["ydc"] and raster8 <= singles["y8"] and raster8 <= singles["y8_inter"]
    assert {r - 1 for r in raster4} <= singles["cac"] and len(singles["y_i16"]) >= 14
    assert any(m.get("t8") and sum(1 for lv in m["coef"]["y8"].values() for v in lv if v) > 40 for m in pics[1]["mbs"]), "dense inter 8x8 blocks"


def test_parity_case_has_every_fraction_in_each_of_the_four_parity_pairs():
    seq, pics, _, _, cov, _ = hf.scripted("field_p_parities")
    seen = {}
    for k, a, px, py, w, h, name, mv in parts_of(pics):
        seen.setdefault((pics[k]["field"], fr.field_of(pics, name)[1]), set()).add((mv[0] & 7, mv[1] & 7, mv[0] % 4 == 0 and mv[1] % 4 == 0))
    assert set(seen) == {(a, b) for a in ("top", "bottom") for b in ("top", "bottom")}
    for pair, v in seen.items():
        assert {(x, y) for x, y, _ in v} == {(x, y) for x in range(8) for y in range(8)}, pair
    assert {q[1:] for q in cov if q[0] == "field_ref"} >= {("bottom", "top", True), ("top", "bottom", True), ("top", "top", False), ("bottom", "bottom", False),
                                                           ("top", "bottom", False), ("bottom", "top", False)}, "second fields predict from their frame's first"


def test_border_case_leaves_the_field_on_every_side_by_every_amount_in_both_parities():
    for size in hf.case_sizes("field_p_borders"):
        seq, pics = hf.scripted("field_p_borders", size)[:2]
        mbw, rows = hf.fdims(*size)
        W, H = mbw * 16, rows * 16
        over = {}
        for k, a, px, py, w, h, name, mv in parts_of(pics):
            X, Y = (a % mbw) * 16 + px, (a // mbw) * 16 + py
            cross = fr.field_of(pics, name)[1] != pics[k]["field"]
            par = pics[k]["field"]
            # whole lines by which the luma footprint (with the filter's reach when the position is fractional) leaves the field
            top = -(Y + (mv[1] >> 2) - (2 if mv[1] & 3 else 0))
            bottom = Y + h - 1 + (mv[1] >> 2) + (3 if mv[1] & 3 else 0) - (H - 1)
            left = -(X + (mv[0] >> 2) - (2 if mv[0] & 3 else 0))
            right = X + w - 1 + (mv[0] >> 2) + (3 if mv[0] & 3 else 0) - (W - 1)
            for side, v in (("top", top), ("bottom", bottom), ("left", left), ("right", right)):
                if v > 0:
                    over.setdefault((par, side), set()).add(v)
            if cross:                                               # chroma: the first / last line the window reads, with the offset
                cy = 8 * (Y // 2) + mv[1] + fr.chroma_mvy_offset(par, fr.field_of(pics, name)[1])
                last = 8 * (Y // 2 + h // 2 - 1) + mv[1] + fr.chroma_mvy_offset(par, fr.field_of(pics, name)[1])
                if par == "top":
                    over.setdefault("chroma_top", set()).add(cy)
                else:
                    over.setdefault("chroma_bottom", set()).add(last - 8 * (H // 2 - 1))
        for par in ("top", "bottom"):
            for side in ("top", "bottom", "left", "right"):
                got = over.get((par, side), set())
                assert 1 in got and ({2, 3} & got) and max(got) > 16, (size, par, side, sorted(got))
        # with the offset: exactly on the border (0), one step past it (-2 at the top; +2 past the last line at the bottom)
        assert {0, -2} <= over["chroma_top"] and {0, 2} <= over["chroma_bottom"], (size, sorted(over["chroma_top"])[:8], sorted(over["chroma_bottom"])[-8:])


def test_list_case_uses_every_index_of_lists_of_7_and_8_fields():
    seq, pics = hf.scripted("field_p_lists")[:2]
    pl = sw.plan(seq, pics)
    st = fr.structure(pics)
    seen = set()
    for k in range(8, 12):
        n = pl[k]["n"][0]
        used = {pl[k]["l0"].index(m["l0"][0]) for m in pics[k]["mbs"]}
        assert used == set(range(n)), (k, n, used)
        seen.add((pics[k]["field"], st[k][2], n))
        if st[k][2]:
            assert pl[k]["l0"][0] == k - 1 or pl[k]["l0"][1] == k - 1, "the first field of the current frame: a store that holds one field"
    assert seen == {("top", False, 8), ("bottom", True, 7), ("bottom", False, 8), ("top", True, 7)}
    assert seq["num_ref_frames"] == 4


def test_b_cases_use_both_lists_every_weighting_and_the_swap():
    for name, mode in (("field_b", 0), ("field_b_explicit", 1), ("field_b_implicit", 2)):
        seq, pics, _, _, cov, _ = hf.scripted(name)
        pl = sw.plan(seq, pics)
        assert seq["weighted_bipred"] == mode
        for k, p in enumerate(pics):
            if p["kind"] != "B":
                continue
            kinds = {("l0" in m, "l1" in m) for m in p["mbs"]}
            assert kinds == {(True, False), (False, True), (True, True)}
        swapped = [k for k, p in enumerate(pics) if p["kind"] == "B" and p["poc"] >= 10]
        for k in swapped:
            assert pl[k]["l1"][:2] == pl[k]["l0"][:2][::-1] and pl[k]["l1"][2:] == pl[k]["l0"][2:], "8.2.4.2.4: equal lists, the first two entries swapped"
            assert {pl[k]["l1"].index(m["l1"][0]) for m in pics[k]["mbs"] if "l1" in m} >= {0, 1}
    imp = {q[1:] for q in cov if q[0] == "implicit"}
    tops, bottoms = {q[1:] for q in imp if q[0] == "top"}, {q[1:] for q in imp if q[0] == "bottom"}
    assert (48, 16) in tops and (32, 32) in tops and (32, 32) in bottoms and tops != bottoms and len(tops | bottoms) >= 4


def test_paff_mixed_has_frames_predicting_from_field_pairs_and_fields_from_frames():
    for name in ("paff_mixed", "paff_mixed_sparse"):
        seq, pics = hf.scripted(name)[:2]
        kinds = [(p["kind"], p.get("field")) for p in pics]
        assert kinds == [("I", None), ("P", "top"), ("P", "bottom"), ("B", None), ("P", None), ("P", "bottom"), ("P", "top")]
        assert any(isinstance(m.get("l0", (0,))[0], tuple) for m in pics[1]["mbs"]), "a P field predicting from a field of a store coded as a frame"
        assert any(m.get("l0", (None,))[0] == 1 for m in pics[4]["mbs"]), "a frame P predicting from a store coded as two fields"
        assert any(m.get("l0", (None,))[0] == 1 or m.get("l1", (None,))[0] == 1 for m in pics[3]["mbs"]), "a B frame predicting from the woven pair"
        for n_intra, n_mbs in hr.intra_counts(seq, pics)[1:3] + hr.intra_counts(seq, pics)[4:]:
            assert n_intra > 0 and ((n_intra * 16 >= n_mbs) if name == "paff_mixed" else (n_intra * 16 < n_mbs)), (name, n_intra, n_mbs)


def test_deblock_cases_filter_under_every_field_rule():
    for size in hf.SIZES_EDGE:
        s = hf.scripted("field_deblock_intra", size)[5]
        assert s.get("H:field_intra_mb_edge_bS3", 0) > 0 and s.get("YH:on_bS3", 0) > 0 and s.get("YV:on_bS4", 0) > 0 or size[0] == 16
        assert s.get("YH:on_bS3", 0) > 0 and s.get("H:idc2_slice_edge_left_alone", 0) > 0
        s = hf.scripted("field_deblock_inter", size)[5]
        for key in ("field_mvy_differs_by_1_bS0", "field_mvy_differs_by_2_bS1", "H:field_intra_mb_edge_bS3", "YH:on_bS2", "YH:on_bS1", "YV:on_bS1"):
            assert s.get(key, 0) > 0 or (key == "YH:on_bS2" and size[0] == 16), (size, key, sorted(s))      # (1 x 3 macroblocks: no coded block meets a filtered edge)
        assert s.get("field_refs_are_the_two_fields_of_one_frame_bS1", 0) > 0 and (s.get("V:mb_edge_vectors_differ_by_3_bS0", 0) > 0 or size[0] == 16)
        assert s.get("V:mb_edge_vectors_differ_by_4_bS1", 0) > 0 or size[0] == 16
        s = hf.scripted("field_deblock_b", size)[5]
        assert s.get("YH:on_bS1", 0) + s.get("YV:on_bS1", 0) > 0


def test_lone_and_cropped_cases():
    for name, par in (("field_lone_top", "top"), ("field_lone_bottom", "bottom")):
        seq, pics, _, planes, _, _ = hf.scripted(name)
        assert fr.counts(pics) == (3, 1) and pics[-1]["field"] == par
        last = fr.output_frames(pics, planes)[-1][1]
        assert all(np.array_equal(pl[0::2], pl[1::2]) and np.array_equal(pl[0::2], f) for pl, f in zip(last, planes[-1])), "this decoder's convention: lines repeated"
    seq, pics, data, planes, _, _ = hf.scripted("field_cropped")
    assert (seq["width"], seq["height"]) == (96, 88) and len(ae.expected_frames(seq, pics, 1, planes)[0]) == 96 * 88 * 3 // 2
