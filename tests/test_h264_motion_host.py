"""H.264 motion vector derivation and direct prediction (clause 8.4.1), the CPU half: what tests/h264_motion_ref.py restates is pinned by hand-worked
values, every scripted case of tests/analytic_h264_motion.py is held to the CPU oracle bit for bit and to the product's parser (parse_only: frame count,
size, the per-macroblock syntax digest), every wrong-on-purpose switch is noticed by a named case, and every case covers what it is there for --
asserted from the branch counts the restatement keeps.  tests/test_h264_motion_gpu.py holds the product's pictures to the same expectations.

No tolerances: the expected pictures are integers from the clauses."""
import hashlib
import json
import os

import numpy as np
import pytest

import analytic_cases as ac
import analytic_expect as ae
import analytic_h264_field as hf
import analytic_h264_motion as hm
import analytic_h264_recon as hr
import h264_motion_ref as mr
import scripted_h264 as sw
from jmcodec_amd import api
from spec_tables_h264 import MB_TYPE_B, MB_TYPE_P, SUB_MB_TYPE_B, SUB_MB_TYPE_P

CASES = [(n, s) for n in sorted(hm.CASES) for s in hm.case_sizes(n)]
IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]


# ---- 1. by hand ---------------------------------------------------------------------------------------------------------------------------------
def flat(mbw, mbh, kind, poc):
    return ac.flat_pic(mbw, mbh, 100, 100, 100, kind, poc)


def p16(ref, mvd):
    return dict(t="mv", mb="P_L0_16x16", ref=([ref], [None]), mvd=([[mvd]], [None]))


def vectors(motion, l=0):
    """per macroblock the list-l vector of its first 4x4 block (None: intra or list unused)"""
    return [None if b is None or b[0][l] is None else b[0][l][1] for b in motion]


def test_median_and_single_match_by_hand():
    """3 x 2 macroblocks, one slice, two references, all 16x16.  Row 0: (4, 8) with no neighbour; then only A is available, so A stands for B and C:
    (4, 8) + (6, -10) = (10, -2), and for the third, which uses refIdx 1 (no neighbour's index matches: the median of three times A) (10, -2) + (-13, 5)
    = (-3, 3).  Row 1: A outside, B = (4, 8), C = (10, -2), two matches: median(0, 4, 10) = 4, median(0, 8, -2) = 0, + (1, 1) = (5, 1).  Then A = (5, 1),
    B = (10, -2), C = (-3, 3) (refIdx 1, but two others match): medians 5 and 1, + (0, 2) = (5, 3).  Last, refIdx 1: C lies outside the picture, so D =
    (10, -2) at refIdx 0 takes its place, A = (5, 3) at refIdx 0, B = (-3, 3) at refIdx 1: the one match, + (1, 1) = (-2, 4)."""
    seq = dict(width=48, height=32, num_ref_frames=2)
    mbs = [p16(0, (4, 8)), p16(0, (6, -10)), p16(1, (-13, 5)), p16(0, (1, 1)), p16(0, (0, 2)), p16(1, (1, 1))]
    pics = [flat(3, 2, "I", 0), flat(3, 2, "P", 2), dict(kind="P", poc=4, layout="pic", mbs=mbs)]
    cov = {}
    assert vectors(mr.derive(seq, pics, cov=cov)[0][2]) == [(4, 8), (10, -2), (-3, 3), (5, 1), (5, 3), (-2, 4)]
    assert cov["single_match"] == 1 and cov["only_A_available"] == 2 and cov["C_replaced_by_D_available"] == 1
    assert vectors(mr.derive(seq, pics, wrong={"median_even_when_one_matches"})[0][2])[5] == (6, 4)      # median((5, 3), (-3, 3), (10, -2)) + (1, 1)
    assert vectors(mr.derive(seq, pics, wrong={"c_not_replaced_by_d"})[0][2])[5] == (-2, 4)              # the one match stays B ...
    assert vectors(mr.derive(seq, pics, wrong={"c_not_replaced_by_d"})[0][2])[3] == (5, 1)


def test_directional_rules_by_hand():
    """One macroblock that is a slice.  16x8: the upper partition finds nothing: (8, 4); the lower one's A lies outside (refIdx -1), so the median
    process runs: B = the upper partition is the one match when the indices are equal: (8, 4) + (1, 1) = (9, 5); with refIdx 1 nothing matches:
    median(0, (8, 4), 0) = 0, + (1, 1).  8x16: the right partition's C and D lie outside, its directional neighbour C has refIdx -1; in the median
    process only A is available and stands for all three: (8, 4) + (1, 1) whatever the index."""
    seq = dict(width=16, height=16, num_ref_frames=2)
    for name, r1, want in (("P_L0_L0_16x8", 0, (9, 5)), ("P_L0_L0_16x8", 1, (1, 1)), ("P_L0_L0_8x16", 0, (9, 5)), ("P_L0_L0_8x16", 1, (9, 5))):
        m = dict(t="mv", mb=name, ref=([0, r1], [None, None]), mvd=([[(8, 4)], [(1, 1)]], [None, None]))
        pics = [flat(1, 1, "I", 0), flat(1, 1, "P", 2), dict(kind="P", poc=4, layout="mb", mbs=[m])]
        blocks = mr.derive(seq, pics)[0][2][0]
        assert blocks[0][0] == (1, (8, 4)) and blocks[15][0] == ([1, 0][r1], want), (name, r1, blocks[15])
    # two macroblocks side by side: the 16x8 partitions of the right one take A = the left macroblock when the index is equal (lower partition) ...
    left = p16(0, (20, -8))
    m = dict(t="mv", mb="P_L0_L0_16x8", ref=([1, 0], [None, None]), mvd=([[(1, 0)], [(0, 1)]], [None, None]))
    pics = [flat(2, 1, "I", 0), flat(2, 1, "P", 2), dict(kind="P", poc=4, layout="pic", mbs=[left, m])]
    blocks = mr.derive(dict(seq, width=32), pics)[0][2][1]
    assert blocks[0][0] == (0, (21, -8))        # upper, refIdx 1: B outside; median process: only A available -> A's vector, + (1, 0)
    assert blocks[15][0] == (1, (20, -7))       # lower, refIdx 0 = A's index: A's vector (20, -8) + (0, 1)
    swapped = mr.derive(dict(seq, width=32), pics, wrong={"directional_16x8_8x16_swapped"})[0][2][1]
    assert swapped[15][0] == (1, (20, -7)) and swapped[0][0] == (0, (21, -8))      # (this pair cannot tell; the scripted case does)


def test_p_skip_by_hand():
    """2 x 2 macroblocks, one slice.  (4, 4); then P_Skip in the first row: B is not available: zero.  Second row: A outside, B = (4, 4), C = the skipped
    macroblock (refIdx 0, zero): two... three entries, two of them matching refIdx 0: median(0, 4, 0) = 0, + (6, 2).  Then P_Skip with A = (6, 2) and
    B = the skipped macroblock above: refIdx 0 with a zero vector: zero.  With a moving macroblock (8, 0) in place of the first skipped one: the third
    is median(0, 4, 8) = 4, median(0, 4, 0) = 0, + (6, 2) = (10, 2), and the skipped one is predicted: A = (10, 2), B = (8, 0), C outside -> D = (4, 4):
    (8, 2)."""
    seq = dict(width=32, height=32)
    ref = [flat(2, 2, "I", 0)]
    mbs = [p16(0, (4, 4)), dict(t="skip"), p16(0, (6, 2)), dict(t="skip")]
    assert vectors(mr.derive(seq, ref + [dict(kind="P", poc=2, layout="pic", mbs=mbs)])[0][1]) == [(4, 4), (0, 0), (6, 2), (0, 0)]
    mbs[1] = p16(0, (4, -4))
    pics = ref + [dict(kind="P", poc=2, layout="pic", mbs=mbs)]
    assert vectors(mr.derive(seq, pics)[0][1]) == [(4, 4), (8, 0), (10, 2), (8, 2)]
    mbs[1] = dict(t="skip")
    assert vectors(mr.derive(seq, pics, wrong={"p_skip_without_zero_neighbour_rule"})[0][1])[3] == (4, 2)      # median((6, 2), 0, (4, 4))
    assert vectors(mr.derive(seq, pics, wrong={"p_skip_unavailable_and"})[0][1])[1] == (4, 4)                   # only B missing: predicted from A


def test_col_zero_flag_by_hand():
    """32x16, decode order I (0), P (4), B (2).  The B picture: B_Bi_16x16 with (8, 4) / (-4, 2), then B_Skip: refIdx 0 / 0 from A, predictors (8, 4) /
    (-4, 2).  The colocated macroblock of the skipped one moved by (1, -1) at refIdx 0: colZeroFlag, both vectors zero; by (2, 0): the predictors."""
    seq = dict(width=32, height=16, num_ref_frames=2, profile=77)
    bi = dict(t="mv", mb="B_Bi_16x16", ref=([0], [0]), mvd=([[(8, 4)]], [[(-4, 2)]]))
    for col, want in (((1, -1), ((0, 0), (0, 0))), ((2, 0), ((8, 4), (-4, 2))), ((0, -2), ((8, 4), (-4, 2))), ((-1, 1), ((0, 0), (0, 0)))):
        pics = [flat(2, 1, "I", 0), dict(kind="P", poc=4, layout="mb", mbs=[p16(0, (0, 0)), p16(0, col)]),
                dict(kind="B", poc=2, layout="pic", mbs=[bi, dict(t="skip")])]
        blocks = mr.derive(seq, pics)[0][2][1]
        assert all(b == ((0, want[0]), (1, want[1])) for b in blocks), (col, blocks[0])
    assert mr.derive(seq, pics, wrong={"col_zero_only_zero_vector"})[0][2][1][0] == ((0, (8, 4)), (1, (-4, 2)))
    assert mr.min_positive(-1, 2) == 2 and mr.min_positive(1, 2) == 1 and mr.min_positive(-1, -1) == -1 and mr.min_positive(0, -1) == 0


def test_dist_scale_factor_by_hand():
    """8-197 .. 8-202.  Current 10 between 8 and 12: tb = 2, td = 4, tx = (16384 + 2) / 4 = 4096, (2 * 4096 + 32) >> 6 = 128.  Current 18, the colocated
    block of the picture at 12 referred to 16: tb = 2, td = -4, tx = 16386 / -4 = -4096 (towards zero), (-8192 + 32) >> 6 = -128.  Current 14 between 0
    and 16: tb = 14, td = 16, tx = (16384 + 8) / 16 = 1024, (14336 + 32) >> 6 = 224.  mvCol = (37, -50) under 224: (8288 + 128) >> 8 = 32, (-11200 +
    128) >> 8 = -44 (-43.25 rounded down); mvL1 = mvL0 - mvCol = (-5, 6).  Under -128: (-4736 + 128) >> 8 = -18, (6400 + 128) >> 8 = 25."""
    assert mr.dist_scale_factor(10, 8, 12) == 128 and mr.dist_scale_factor(18, 16, 12) == -128 and mr.dist_scale_factor(14, 0, 16) == 224
    assert mr.scale_mv(224, (37, -50)) == (32, -44) and mr.scale_mv(-128, (37, -50)) == (-18, 25)
    assert mr.dist_scale_factor(14, 0, 16, {"dist_scale_without_rounding"}) == 224 and mr.scale_mv(-128, (37, -50), {"dist_scale_without_rounding"}) == (-19, 25)
    assert mr.dist_scale_factor(127, -128, 127) == 256 and mr.dist_scale_factor(100, 0, 2) == 1023 and mr.dist_scale_factor(-100, 0, 2) == -1024      # the clips
    seq = dict(width=16, height=16, num_ref_frames=2, profile=77)
    pics = [flat(1, 1, "I", 0), dict(kind="P", poc=16, layout="mb", mbs=[p16(0, (37, -50))]),
            dict(kind="B", poc=14, layout="pic", direct_spatial=0, mbs=[dict(t="skip")])]
    assert all(b == ((0, (32, -44)), (1, (-5, 6))) for b in mr.derive(seq, pics)[0][2][0])
    assert mr.derive(seq, pics, wrong={"mv_l1_sign_swapped"})[0][2][0][0] == ((0, (32, -44)), (1, (5, -6)))


def test_te_ranges_are_all_written():
    """9.1: te(v) with range 1 sends nothing, with range 2 the inverted bit, above that ue(v): the cases use active lists of 1, 2 and more entries"""
    seen = set()
    for name in sorted(hm.CASES):
        seq, pics = hm.scripted(name)[:2]
        for p, pl in zip(pics, sw.plan(seq, pics)):
            if sw.uses_new_forms(seq, p) and any(m["t"] == "mv" and m["mb"] != "P_8x8ref0" and "ref" in m for m in p["mbs"]):
                seen |= {min(n, 3) for n in (pl["n"] if p["kind"] == "B" else pl["n"][:1])}
    assert seen == {1, 2, 3}
    b = sw.Bits()
    b.te(1, 1); b.te(0, 1); b.te(2, 2); b.u(3, 0)
    assert b.bytes() == bytes([0b01011000])                         # inverted bits 0, 1, then ue(2) = 011


# ---- 2. the writer ------------------------------------------------------------------------------------------------------------------------------
def test_existing_streams_are_byte_identical():
    """The writer's new forms leave every stream of the earlier cases as it was: SHA-256 of each, recorded before the change"""
    with open(os.path.join(os.path.dirname(__file__), "golden", "scripted_h264_stream_hashes.json")) as f:
        want = json.load(f)
    got = {}
    for group, mod, cases in (("cases", ac, ac.H264_CASES), ("recon", hr, hr.CASES), ("field", hf, hf.CASES)):
        for n in sorted(cases):
            for s in mod.case_sizes(n):
                got[f"{group}/{n}/{s[0]}x{s[1]}"] = hashlib.sha256(sw.write(*cases[n](*s))).hexdigest()
    assert got == want


def test_both_typings_of_the_16x16_predictor_agree_on_every_existing_case():
    """scripted_h264.mv_predictor_16x16 (the writer's, for slices of 16x16 and intra macroblocks) and h264_motion_ref's 8.4.1.3"""
    compared = nontrivial = 0
    for cases, sizes in ((ac.H264_CASES, ac.case_sizes), (hr.CASES, hr.case_sizes)):
        for n in sorted(cases):
            seq, pics = cases[n](*sizes(n)[0])
            if any(p["kind"] == "B" for p in pics):
                continue
            mvp = {}
            mr.derive(seq, pics, mvp_out=mvp)
            pl = sw.plan(seq, pics)
            for k, p in enumerate(pics):
                step = sw.layout_step(seq, p)
                if p["kind"] != "P" or step == 1 or not all(m["t"] in sw.INTRA + ("16x16",) for m in p["mbs"]):
                    continue
                st = sw.PicState(seq, p["mbs"], step)
                for a, m in enumerate(p["mbs"]):
                    if m["t"] == "16x16":
                        theirs = sw.mv_predictor_16x16(st, a, m["l0"][0])
                        assert mvp[(k, a, 0, 0)] == theirs, (n, k, a)
                        compared += 1
                        nontrivial += theirs != (0, 0) and theirs != tuple(m["l0"][1])
    assert compared > 200 and nontrivial > 50, (compared, nontrivial)


def test_writer_refuses_what_it_cannot_state():
    rng = np.random.default_rng(2)
    seq = dict(width=16, height=16, profile=77, num_ref_frames=2)
    ref = [ac.noise_pic(rng, 1, 1, "I", 0)]
    ok = [ref[0], dict(kind="P", poc=4, layout="pic", mbs=[p16(0, (1, 2))])]
    assert sw.write(seq, ok)
    with pytest.raises(AssertionError):                             # a direct macroblock where list 1 is empty
        sw.write(seq, [dict(kind="B", poc=0, layout="pic", mbs=[dict(t="mv", mb="B_Direct_16x16")])])
    with pytest.raises(AssertionError):                             # mvd outside the scripted range of se(v)
        sw.write(seq, [ref[0], dict(kind="P", poc=4, layout="pic", mbs=[p16(0, (sw.MVD_RANGE + 1, 0))])])
    with pytest.raises(AssertionError):                             # ref_idx outside the active list
        sw.write(seq, [ref[0], dict(kind="P", poc=4, layout="pic", mbs=[p16(1, (1, 0))])])
    with pytest.raises(AssertionError):                             # a list the partition does not use
        sw.write(seq, [ref[0], dict(kind="P", poc=4, layout="pic", mbs=[dict(t="mv", mb="P_L0_16x16", ref=([0], [0]), mvd=([[(1, 1)]], [[(1, 1)]]))])])
    with pytest.raises(AssertionError):                             # P_8x8ref0 with an index
        sw.write(seq, ok[:1] + [ac.noise_pic(rng, 1, 1, "P", 2), dict(kind="P", poc=4, layout="pic", mbs=[
            dict(t="mv", mb="P_8x8ref0", sub=["P_L0_8x8"] * 4, ref=([0, 1, 0, 0], [None] * 4), mvd=([[(1, 1)]] * 4, [None] * 4))])])
    with pytest.raises(AssertionError):                             # the old forms beside the new ones in one picture
        sw.write(dict(seq, width=32), [ac.noise_pic(rng, 2, 1, "I", 0), dict(kind="P", poc=4, layout="pic", mbs=[p16(0, (1, 2)), ac.l0(0, 4, 4)])])
    fseq = dict(width=16, height=32, frame_mbs_only=0)
    top, bot = hf.noise_field(rng, 1, 1, "top", 0), hf.noise_field(rng, 1, 1, "bottom", 1, kind="P")
    with pytest.raises(AssertionError):                             # field pictures with the new forms
        sw.write(fseq, [top, bot, dict(kind="P", poc=2, field="top", layout="pic", mbs=[p16(0, (1, 2))]), hf.noise_field(rng, 1, 1, "bottom", 3, kind="P")])
    with pytest.raises(AssertionError):                             # a frame picture of a stream that may hold fields, too
        sw.write(fseq, [top, bot, dict(kind="P", poc=2, layout="pic", mbs=[p16(0, (1, 2))] * 2)])
    with pytest.raises(AssertionError):
        sw.sps(dict(fseq, direct_8x8_inference=0))                  # 7.4.2.1.1


def test_transform_size_8x8_flag_condition():
    """7.3.5: with transform_8x8_mode_flag and a coded luma block the flag follows only without sub-8x8 partitions, direct only under
    direct_8x8_inference_flag.  One coded DC coefficient on each kind of macroblock; the oracle and the parser read every stream to its end."""
    d8, l08, l044 = "B_Direct_8x8", "B_L0_8x8", "B_L0_4x4"
    ref = lambda subs: ([None if s == d8 else 0 for s in subs], [None] * 4)
    mvd = lambda subs: ([None if s == d8 else [(1, 2)] * (4 if s == l044 else 1) for s in subs], [None] * 4)
    b8 = lambda subs: dict(t="mv", mb="B_8x8", sub=subs, ref=ref(subs), mvd=mvd(subs))
    for inf in (1, 0):
        seq = dict(width=16, height=16)
        assert sw.transform8x8_flag_allowed(dict(seq, direct_8x8_inference=inf), "B", dict(t="mv", mb="B_Direct_16x16")) == bool(inf)
        assert sw.transform8x8_flag_allowed(dict(seq, direct_8x8_inference=inf), "B", b8([l08, d8, l08, l08])) == bool(inf)
        assert sw.transform8x8_flag_allowed(dict(seq, direct_8x8_inference=inf), "B", b8([l08] * 4))
        assert not sw.transform8x8_flag_allowed(dict(seq, direct_8x8_inference=inf), "B", b8([l08, l044, l08, l08]))
    assert sw.transform8x8_flag_allowed(dict(width=16, height=16), "P", p16(0, (0, 0)))


@pytest.mark.parametrize("inference", [1, 0])
def test_transform_flag_streams_decode(oracle, inference):
    seq, pics, seen = t8_script(inference)
    data = sw.write(seq, pics, seen)
    assert {q[2] for q in seen if q[0] == "transform_size_8x8_flag_possible" and q[3]} == {True, False}
    planes = ae.expect_h264(seq, pics)
    got, n, w, h = oracle.decode(data, 1)
    fs = w * h * 3 // 2
    diff = ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], 1, planes)
    assert n == 3 and diff is None, diff
    assert oracle.syntax_digest(data) == product_digest(data)[:2]


def t8_script(inference):
    """48x32: a B picture whose macroblocks each carry one DC coefficient, under transform_8x8_mode_flag: B_L0_16x16, B_Direct_16x16, B_8x8 of 8x8
    quadrants, with a direct quadrant, with a 4x4 quadrant; a skipped one"""
    rng = np.random.default_rng(0xD900 + inference)
    seq = dict(width=48, height=32, profile=100, transform8x8=1, num_ref_frames=2, direct_8x8_inference=inference)
    subs = [["B_L0_8x8", "B_Bi_8x8", "B_L1_8x8", "B_L0_8x8"], ["B_L0_8x8", "B_Direct_8x8", "B_L1_8x8", "B_Direct_8x8"], ["B_L0_8x8", "B_L0_4x4", "B_L1_8x4", "B_L0_8x8"]]
    mbs = [hm.mv_mb(rng, "B", "B_L0_16x16", (1, 1)), dict(t="mv", mb="B_Direct_16x16")] + [hm.mv_mb(rng, "B", "B_8x8", (1, 1), s) for s in subs] + [dict(t="skip")]
    for i, m in enumerate(mbs[:5]):
        m["resid"] = ((3 * i + 1) % 16, 1 if i % 2 else -1)
    pics = [ac.noise_pic(rng, 3, 2, "I", 0), ac.noise_pic(rng, 3, 2, "P", 4), dict(kind="B", poc=2, layout="pic", mbs=mbs)]
    return seq, pics, set()


# ---- 3. the oracle and the host parser ----------------------------------------------------------------------------------------------------------
def product_digest(data):
    with api.JmAmdDec(0, 1, options={"parse_only": 1, "digest": 1}) as d:
        n = d.decode_stream(data, keep=False)
        err = api.lib().jm_amddec_last_error(d.h).decode()
        return d.stat("syntax_digest") & (2 ** 64 - 1), d.stat("digest_mbs"), n, d.stat("errors"), err, api.jm_nvdec_stream_info(d.h)


@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_oracle_decodes_the_restated_expectation(oracle, name, size):
    seq, pics, data, planes, _, _ = hm.scripted(name, size)
    assert data == sw.write(*hm.CASES[name](*size)), "the case builder and the writer are deterministic"
    assert len(pics) <= 8
    for fmt in (1, 0):
        got, n, w, h = oracle.decode(data, fmt)
        assert (n, w, h) == (len(pics), size[0], size[1])
        fs = w * h * 3 // 2
        diff = ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], fmt, planes)
        assert diff is None, f"{name} {size} format {fmt}: {diff}"


@pytest.mark.parametrize("name", ["p_partitions", "reach_chain", "p_skip"])
def test_oracle_decodes_the_cases_with_deblocking_on(oracle, name):
    """the variants the GPU test sends through chain launches: 8.7 decides bS from the DERIVED vectors of every 4x4 block"""
    seq, pics, data, planes = hm.scripted_deblocked(name)
    raw = hm.scripted(name)[3] if name != "reach_chain" else ae.expect_h264(seq, [dict(p, deblock=(1, 0, 0)) for p in pics])
    assert any(not np.array_equal(a, b) for P, Q in zip(planes, raw) for a, b in zip(P, Q)), "the filter filters"
    got, n, w, h = oracle.decode(data, 1)
    fs = w * h * 3 // 2
    diff = ae.first_difference(seq, pics, [got[i * fs:(i + 1) * fs] for i in range(n)], 1, planes)
    assert n == len(pics) and diff is None, f"{name}: {diff}"


@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_host_parser_accepts_the_stream_and_reads_the_oracles_syntax(oracle, name, size):
    seq, pics, data, _, _, _ = hm.scripted(name, size)
    digest, mbs, n, errors, err, info = product_digest(data)
    assert errors == 0 and err == ""
    assert n == len(pics) and info == size
    assert (digest, mbs) == oracle.syntax_digest(data)
    assert mbs == sum(len(p["mbs"]) for p in pics)


def script_counts(pics):
    c = {}
    for p in pics:
        for m in p["mbs"]:
            key = {"skip": p["kind"] + "_Skip", "mv": m.get("mb"), "pcm": "I_PCM", "i16": "I16x16"}[m["t"]]
            c[key] = c.get(key, 0) + 1
    return c


@pytest.mark.parametrize("name", sorted(hm.CASES))
def test_oracle_tool_counters_are_the_scripts(oracle, name):
    seq, pics, data = hm.scripted(name)[:3]
    tools, c = oracle.tools(data), script_counts(pics)
    want = {"P_Skip": c.get("P_Skip", 0), "B_Skip": c.get("B_Skip", 0), "P16x16": c.get("P_L0_16x16", 0), "P16x8": c.get("P_L0_L0_16x8", 0),
            "P8x16": c.get("P_L0_L0_8x16", 0), "P8x8": c.get("P_8x8", 0) + c.get("P_8x8ref0", 0), "B_Direct": c.get("B_Direct_16x16", 0),
            "I_PCM": c.get("I_PCM", 0), "I16x16": c.get("I16x16", 0)}
    assert {k: tools.get(k, 0) for k in want} == want


# ---- 4. wrong on purpose ------------------------------------------------------------------------------------------------------------------------
NOTICED_BY = {
    "median_even_when_one_matches": "p_partitions", "c_not_replaced_by_d": "p_neighbours", "only_a_rule_dropped": "p_neighbours",
    "directional_16x8_8x16_swapped": "p_partitions", "directional_without_ref_check": "p_partitions", "p_skip_without_zero_neighbour_rule": "p_skip",
    "p_skip_unavailable_and": "p_skip", "later_partition_available": "p_partitions", "direct_pred_part_width_of_sub_partition": "b_spatial_direct",
    "spatial_min_instead_of_min_positive": "b_spatial_direct", "col_zero_any_ref_idx_col": "b_spatial_direct_no_inference",
    "col_zero_only_zero_vector": "b_spatial_direct", "col_zero_ignores_ref_idx": "b_spatial_direct_no_inference",
    "spatial_direct_own_partitions": "b_spatial_direct", "col_block_itself_under_inference": "b_spatial_direct",
    "col_list1_never_consulted": "b_temporal_direct", "temporal_ref_idx_unmapped": "b_temporal_direct", "dist_scale_without_rounding": "b_temporal_direct",
    "mv_l1_sign_swapped": "b_temporal_direct", "quadrant_list1_only_as_list0": "b_partitions"}


def test_every_switch_has_a_named_case():
    assert set(NOTICED_BY) == set(mr.SWITCHES) and len(mr.SWITCHES) == 20


@pytest.mark.parametrize("switch", mr.SWITCHES)
def test_wrong_on_purpose_is_noticed_by_its_named_case(switch):
    """A decoder with this defect hands out other frames for the named case: the case fails on it."""
    seq, pics, _, planes, _, _ = hm.scripted(NOTICED_BY[switch])
    right = ae.expected_frames(seq, pics, 1, planes)
    wrong = ae.expected_frames(seq, pics, 1, ae.expect_h264(seq, pics, wrong={switch}))
    assert len(right) == len(wrong) and right != wrong, f"{switch} does not show in {NOTICED_BY[switch]}"


# ---- 5. the cases cover what they are there for -------------------------------------------------------------------------------------------------
PREDICTOR = ["single_match", "median_0_matches", "median_2_matches", "median_3_matches", "only_A_available", "C_is_a_later_partition",
             "C_replaced_by_D_available", "C_replaced_by_D_unavailable"]
DIRECTIONAL = ["directional_%s_part%d_%s" % (s, i, e) for s in ("16x8", "8x16") for i in (0, 1) for e in ("taken", "falls_to_median")]
COVERAGE = {    # group -> the branches of tests/h264_motion_ref.py that its cases take (every one of them at each size)
    "p_partitions": PREDICTOR + DIRECTIONAL + ["intra_neighbour_A", "intra_neighbour_B", "intra_neighbour_C"],
    "p_neighbours": PREDICTOR + ["intra_neighbour_A", "intra_neighbour_B", "intra_neighbour_C", "other_slice_neighbour_A", "other_slice_neighbour_B",
                                 "other_slice_neighbour_C", "other_slice_neighbour_D"],
    "p_skip": ["p_skip_A_and_B_unavailable", "p_skip_A_or_B_unavailable", "p_skip_zero_neighbour_A", "p_skip_zero_neighbour_B", "p_skip_predicted_nonzero"],
    "b_partitions": PREDICTOR + DIRECTIONAL + ["quadrant_uses_L0", "quadrant_uses_L1", "quadrant_uses_Bi"],
    "b_spatial_direct": ["spatial_both_found", "spatial_only_list0", "spatial_only_list1", "spatial_both_negative", "spatial_inference",
                         "spatial_no_inference", "col_corner_block", "col_block_itself", "col_intra", "col_list0", "col_zero_applies",
                         "col_zero_true_but_ref_idx_not_0", "col_zero_blocked_by_ref_idx_col", "col_zero_mv_within_1", "col_zero_mv_beyond_1",
                         "col_component_+1", "col_component_+2", "col_component_-1", "col_component_-2", "col_zero_differs_inside_a_quadrant"],
    "b_temporal_direct": ["temporal_inference", "temporal_no_inference", "col_corner_block", "col_block_itself", "col_intra", "temporal_col_intra",
                          "col_list0", "col_list1", "temporal_ref_idx_mapped_same", "temporal_ref_idx_mapped_differs", "dsf_dyadic", "dsf_non_dyadic",
                          "dsf_negative", "temporal_rounding_matters"]}


def group_cases(group):
    return [n for n in sorted(hm.CASES) if n == group or n.startswith(group + "_")]


def test_every_branch_of_the_restatement_is_taken_in_its_group(capsys):
    rows = []
    for group, branches in COVERAGE.items():
        for size in hm.SIZES:
            total = {}
            for n in group_cases(group):
                for k, v in hm.scripted(n, size)[4].items():
                    total[k] = total.get(k, 0) + v
            missing = [b for b in branches if not total.get(b)]
            assert not missing, (group, size, missing)
            if size == hm.SIZES[0]:
                rows += [(group, b, total[b]) for b in branches]
    with capsys.disabled():
        print("\nbranch coverage of tests/h264_motion_ref.py at 96x80 (group, branch, times taken)")
        for r in rows:
            print("    %-18s %-44s %6d" % r)


def test_every_mb_type_and_sub_mb_type_occurs():
    seen = set()
    for n in sorted(hm.CASES):
        seen |= {k[1:] for k in hm.scripted(n)[4] if isinstance(k, tuple)}
    names = {q[0] for q in MB_TYPE_P + MB_TYPE_B} | {"P_Skip", "B_Skip"}
    assert {q[0] for q in seen if len(q) == 1} == names | {q[0] for q in SUB_MB_TYPE_P + SUB_MB_TYPE_B}
    cov = {}
    for n in group_cases("b_partitions"):
        cov.update(hm.scripted(n)[4])
    assert {k[1:] for k in cov if isinstance(k, tuple) and k[0] == "sub_mb_type_in_quadrant"} == {(q[0], i) for q in SUB_MB_TYPE_B for i in range(4)}
    assert {k[1] for k in hm.scripted("b_partitions")[4] if isinstance(k, tuple) and k[0] == "mb_type"} == {q[0] for q in MB_TYPE_B}
    assert {k[1] for k in hm.scripted("p_partitions")[4] if isinstance(k, tuple)} == {q[0] for q in MB_TYPE_P + SUB_MB_TYPE_P}


def test_b_partitions_have_quadrants_of_four_different_list_and_reference_pairs():
    for name, mode in (("b_partitions", 0), ("b_partitions_explicit", 1), ("b_partitions_implicit", 2)):
        seq, pics, _, _, _, _ = hm.scripted(name)
        assert seq["weighted_bipred"] == mode
        motion = mr.derive(seq, pics)[0]
        four = pairs = 0
        for k, p in enumerate(pics):
            for blocks in motion[k]:
                if p["kind"] == "B" and blocks is not None:
                    quads = {tuple(None if q is None else q[0] for q in blocks[i]) for i in (0, 2, 8, 10)}
                    four += len(quads) == 4 and all(sum(q is not None for q in u) == 1 for u in quads)
                    pairs += any(u[0] is not None and u[1] is not None for u in quads) and len(quads) > 1
        assert four >= 3 and pairs >= 10, (name, four, pairs)       # per-quadrant index pairs reach the weighting


def quadrant_windows(seq, pics, kind):
    """(macroblock key, list, xi, yi, the quadrant's four blocks are one vector) of every quadrant and list in use of the `kind` pictures that state
    syntax: where the 13x13 window of the quadrant's first block lies"""
    mbw = (seq["width"] + 15) // 16
    motion = mr.derive(seq, pics)[0]
    for k, p in enumerate(pics):
        if p["kind"] != kind or not sw.uses_new_forms(seq, p):
            continue
        for a, blocks in enumerate(motion[k]):
            for g in range(4):
                first = (g >> 1) * 8 + (g & 1) * 2
                for l in (0, 1):
                    if blocks is not None and blocks[first][l] is not None:
                        xi, yi = hm.window_origin((a % mbw) * 16 + (g & 1) * 8, (a // mbw) * 16 + (g >> 1) * 8, blocks[first][l][1])
                        yield (k, a), l, xi, yi, len({blocks[first + d][l] for d in (0, 1, 4, 5)}) == 1


@pytest.mark.parametrize("size", hm.case_sizes("window_borders"), ids=lambda s: f"{s[0]}x{s[1]}")
def test_window_borders_meet_each_inequality_with_equality_and_miss_it_by_one(size):
    """xi >= 0, yi >= 0, xi + 13 <= W, yi + 13 <= H of the CODED picture (at 90x70: of 96x80): for P and for B pictures each is met with equality and
    missed by one; per side a macroblock with every window inside and one touching, and one with exactly one window out, by one sample"""
    seq, pics = hm.scripted("window_borders", size)[:2]
    W, H = (size[0] + 15) // 16 * 16, (size[1] + 15) // 16 * 16
    for kind in ("P", "B"):
        per_mb, deviating, far = {}, 0, 0
        for key, l, xi, yi, one in quadrant_windows(seq, pics, kind):
            d = (-xi, -yi, xi + 13 - W, yi + 13 - H)                # by how much each inequality is missed (0: met with equality)
            per_mb.setdefault(key, []).append(d)
            deviating += not one
            far += max(d) > W
        sides_touch, sides_out = set(), set()
        for ds in per_mb.values():
            worst = [max(d[s] for d in ds) for s in range(4)]
            if max(worst) == 0:
                sides_touch |= {s for s in range(4) if worst[s] == 0}
            out = [(s, d[s]) for d in ds for s in range(4) if d[s] > 0]
            if len(out) == 1 and out[0][1] == 1:
                sides_out.add(out[0][0])
        assert sides_touch == {0, 1, 2, 3} and sides_out == {0, 1, 2, 3}, (size, kind, sides_touch, sides_out)
        assert size[0] < 90 or (deviating >= 4 and far >= 2), (size, kind, deviating, far)


def test_the_border_of_the_cropped_picture_is_the_coded_pictures():
    """90x70 is cropped from 96x80: the windows above lie against x = 96 and y = 80, and samples beyond x = 90 / y = 70 are predicted from: with other
    samples there in the references, the VISIBLE part of the predicted pictures changes"""
    seq, pics, _, planes, _, _ = hm.scripted("window_borders", (90, 70))
    seq2, pics2 = hm.window_borders(90, 70, alter_cropped=True)
    assert ae.pack(seq, planes[0], 1) == ae.pack(seq2, ae.expect_h264(seq2, pics2[:1])[0], 1), "the references look the same"
    other = ae.expect_h264(seq2, pics2)
    assert all(ae.pack(seq, a, 1) != ae.pack(seq, b, 1) for a, b in zip(planes[2:], other[2:]))


@pytest.mark.parametrize("size", hm.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reach_chain_has_its_longest_vector_in_one_inner_4x4_block(size):
    seq, pics = hm.scripted("reach_chain", size)[:2]
    motion = mr.derive(seq, pics)[0]
    q, j = hm.REACH_BLOCK
    at = ((q >> 1) * 2 + (j >> 1)) * 4 + (q & 1) * 2 + (j & 1)
    assert at == 9 and at % 4 in (1, 2) and at // 4 in (1, 2) and j != 0, "inside the macroblock: no other macroblock's A, B, C or D"
    for k, p in enumerate(pics[1:], 1):
        assert p["deblock"] == (0, 0, 0) and sw.plan(seq, pics)[k]["l0"] == [k - 1]
        vs = [(b[0][1], a, i) for a, blocks in enumerate(motion[k]) if blocks is not None for i, b in enumerate(blocks)]
        for c in (0, 1):
            top = max(v[0][c] for v in vs)
            holders = [(a, i) for v, a, i in vs if v[c] == top]
            assert len(holders) == 1 and holders[0][1] == at and top > 4 * 30, (k, c, top, holders)
            assert sorted(v[0][c] for v in vs)[-2] < top - 4 * 16, "nothing else comes near"


@pytest.mark.parametrize("name", ["p_skip", "p_partitions", "p_neighbours", "reach_chain"])
def test_the_parsers_short_route_builds_the_same_job_lists(name):
    """P_Skip and P_L0_16x16 take a shorter route through the CAVLC parser (h264_cavlc.cpp, `fast`), which reads the neighbour data the general route
    wrote and writes what the general route reads: in these slices the two alternate.  The job lists the device would get are the same either way."""
    from test_host_parser import _job_digest
    data = hm.scripted(name)[2]
    a, b = _job_digest(data, True), _job_digest(data, False)
    assert a == b and a[2] == 0 and a[1] == len(hm.scripted(name)[1])


def test_p_skip_runs_end_slices_and_cross_row_ends():
    """mb_skip_run as the last syntax element of a slice (in a slice that ends in mid-row, and at the end of the picture), a run that goes on across
    the end of a macroblock row, and skipped macroblocks between P_L0_16x16 and P_8x8 in one slice"""
    seq, pics = hm.scripted("p_skip")[:2]
    mbw = (seq["width"] + 15) // 16
    ends_slice = crosses_row = beside = 0
    for p in pics[2:]:
        step, mbs = sw.layout_step(seq, p), p["mbs"]
        for a, m in enumerate(mbs):
            if m["t"] != "skip":
                continue
            last = a % step == step - 1 or a == len(mbs) - 1
            ends_slice += last and (a + 1) % mbw != 0 or a == len(mbs) - 1
            crosses_row += not last and (a + 1) % mbw == 0 and mbs[a + 1]["t"] == "skip"
            near = {mbs[b].get("mb") for b in (a - 1, a + 1) if 0 <= b < len(mbs) and b // step == a // step}
            beside += bool(near & {"P_L0_16x16"}) + bool(near & {"P_8x8"})
    assert ends_slice >= 3 and crosses_row >= 3 and beside >= 20, (ends_slice, crosses_row, beside)
