"""A scripted H.264 stream writer (CAVLC, pic_order_cnt_type 0, frame and field pictures, 4:2:0, 8 bit; Baseline / Main subset and the High tools below) for the
analytic known-answer tests.

The test says which macroblock carries which samples, vector, reference, weight, mode and levels; ``write`` turns that script into Annex-B bytes.  The
decoded picture follows from the script by arithmetic alone (tests/analytic_expect.py, tests/h264_recon_ref.py).  Typed from the syntax clauses (7.3.2.1,
7.3.2.1.1.1, 7.3.2.2, 7.3.3, 7.3.4, 7.3.5, 7.3.5.1, 7.3.5.2, 7.3.5.3, 9.1, 9.2) -- not from tools/h264gen.c, the oracle or the product: a fourth typing of the
syntax is part of the value.  The code tables are the separately typed ones of tests/spec_tables_h264.py.

The script
    seq  = dict(width, height, num_ref_frames=1, profile=66 | 77 | 100, weighted_pred=0, weighted_bipred=0, init_qp=26, chroma_qp_off=0,
                constrained_intra=0) and, with profile=100 only: transform8x8=0 | 1, second_chroma_qp_off, sps_lists, pps_lists -- eight scaling lists
                each (Intra Y, Cb, Cr, Inter Y, Cb, Cr 4x4, Intra Y, Inter Y 8x8): None (absent: the fall-back rule of Table 7-2 applies), "default" (the
                first delta_scale gives nextScale 0) or the 16 / 64 values in zig-zag order; key absent: no matrix in that parameter set
    pics = [dict(kind="I" | "P" | "B", poc=even int, layout="mb" | "row" | "pic" | n (slices of n macroblocks), mbs=[...], and optionally
                 direct_spatial (B: direct_spatial_mv_pred_flag, default 1),
                 is_ref (default: kind != "B"), qp (slice QP, default init_qp), deblock=(disable_idc, alpha_div2, beta_div2) (default (1, 0, 0)),
                 num_ref=(n0, n1) (active entries, sent with num_ref_idx_active_override), wp=dict(ld_y, ld_c, l0=[entry..], l1=[entry..]) with
                 entry = None (both flags 0) or dict(y=(w, o) | None, c=((w, o), (w, o)) | None))]
    mbs[addr] is one of
        dict(t="pcm", y=(16,16) uint8, cb=(8,8), cr=(8,8))
        dict(t="i16", mode=0..3, cmode=0..3)                       Intra16x16
        dict(t="i4", modes=[16 Intra4x4PredMode in luma4x4BlkIdx order], cmode=0..3)
        dict(t="i8", modes=[4 Intra8x8PredMode], cmode=0..3)       needs transform8x8=1
        dict(t="skip")                                             P_Skip
        dict(t="16x16", l0=(pic, (mvx, mvy)) | None, l1=(pic, (mvx, mvy)) | None)      pic = index into pics (decode order), vectors in quarter samples
        dict(t="16x8" | "8x16", parts=[(pic, mv), (pic, mv)])      P only
        dict(t="mv", mb=<name of Table 7-13 / 7-14>, sub=[4 names of Table 7-17 / 7-18] (P_8x8, P_8x8ref0, B_8x8),
             ref=([ref_idx_l0 per partition | None], [ref_idx_l1 ..]), mvd=([[(dx, dy) per sub-partition] | None per partition], [.. l1]))
                                                                   SYNTAX, not motion: the writer derives no vector for it (tests/h264_motion_ref.py
                                                                   does, for the expectation); B_Direct_16x16 carries mb only; resid= is allowed.  In a
                                                                   picture that holds one, every inter macroblock is of this form or t="skip" (P_Skip /
                                                                   B_Skip, in slices of any length: mb_skip_run spans macroblocks and ends slices).
                                                                   seq["direct_8x8_inference"] (default 1) is the SPS flag.  Refused: field pictures,
                                                                   direct prediction with an empty list 1, |mvd| > MVD_RANGE, ref_idx outside the list
    any of these but pcm and skip may carry levels, every matrix in RASTER order:
        coef=dict(y={blkIdx: 16 levels} (Intra16x16: the AC, element 0 is 0) or, under the 8x8 transform (t="i8", or t8=1 on an inter macroblock),
                  y8={8x8 block: 64 levels}; ydc=16 levels (Intra16x16 DC, the matrix c of 8.5.10); cdc=(4 Cb, 4 Cr); cac={(plane, blk): 15 levels, raster
                  positions 1 .. 15}) and dqp=.. (mb_qp_delta, accumulated per 7.4.5 within the slice: ``mb_qps``)
    The writer derives mb_type (the 24 Intra16x16 types among them), coded_block_pattern through me(v), transform_size_8x8_flag, prev_intra4x4 / 8x8_
    pred_mode_flag and rem_intra4x4 / 8x8_pred_mode from a mode derivation of its own (PicState.pred_mode), nC of 9.2.1 across macroblocks and slices
    (I_PCM counts 16, skipped macroblocks and blocks switched off by the pattern 0, the Intra16x16 DC block takes block 0's nC, chroma DC -1, the four
    interleaved 4x4 blocks of an 8x8 block each count their own levels) and the level coding of 9.2.2.1; it refuses by assertion what it cannot state,
    a level that needs level_prefix 16 outside profile 100 among it.
    and, for the streams on which the deblocking filter has to filter (tests/deblock_ref.py computes what it does):
        qp=.., deblock=(idc, a, b) on any macroblock of layout "mb": the macroblock is a slice, so slice_qp_delta and the three deblocking fields carry them
        resid=(blkIdx, +1 | -1) on a P 16x16 / 16x8 / 8x16 macroblock of layout "mb": ONE coded coefficient, the DC of luma block blkIdx (6.4.3 order), level
        +-1 -- coded_block_pattern has the luma bit of that block's 8x8 and nothing else, mb_qp_delta is 0; the block's sixteen samples move by one constant
        (analytic_expect.dc_only_residual)
layout "mb": one slice per macroblock (no neighbour is available: every vector predictor is (0, 0), mvd = the vector); "row" / "pic": one slice per
macroblock row / per picture -- the inter macroblocks of such a slice are 16x16 and not P_Skip.  Where they all repeat ONE vector and reference per list
the predictor is that vector as soon as a neighbour exists, whichever of 8.4.1.3's branches applies (B slices: only this); any other mixture of 16x16 P
and intra macroblocks goes through 8.4.1.3 typed out (``mv_predictor_16x16``).

Field pictures (PAFF).  With seq["frame_mbs_only"] = 0 a picture may carry field="top" | "bottom": a field is a picture of its own in pics, its mbs cover
mbw x mbh / 2 macroblocks, its poc is the FIELD's count; two consecutive fields of opposite parity are a frame (one frame_num; either parity first); a
first field without the other ends the stream.  Frame pictures of such a stream work as before (both fields have the frame's count).  A reference names a
FIELD when the current picture is a field: the field picture's index, or (index, "top" | "bottom") for one field of a picture coded as a frame; when the
current picture is a frame it names a frame or the first-decoded index of a field pair (the woven pair).  Typed from 7.3.3 (field_pic_flag,
bottom_field_flag, first_mb_in_slice in field macroblocks, num_ref_idx_active up to 32), 8.2.4.1, 8.2.4.2.2, 8.2.4.2.4, 8.2.4.2.5, 8.2.5.3 (``plan_paff``),
8.5.6 / 8.5.7 (every block of a field in field scan order; scaling lists stay zig-zag) and 7.4.2.1.1 (vertical crop unit of 4 luma rows).  Refused by
assertion: a frame that names a store holding one field, a field that names a field outside its list.  Out of scope: CABAC, direct prediction and
B_Skip in B fields (they carry 16x16 macroblocks with explicit vectors), long-term fields, marking operations, MBAFF.
"""
import re

import numpy as np

from spec_tables_h264 import (CBP_OF_CODENUM, COEFF_TOKEN, FIELD_SCAN_4x4, FIELD_SCAN_8x8, MB_TYPE_B, MB_TYPE_P, RUN_BEFORE, SUB_MB_TYPE_B, SUB_MB_TYPE_P,
                              TOTAL_ZEROS_4x4, TOTAL_ZEROS_CHROMA_DC, ZIGZAG_4x4 as FRAME_SCAN_4x4, ZIGZAG_8x8 as FRAME_SCAN_8x8, parse_code_table)


class Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def u(self, n, x):
        assert 0 <= x < (1 << n), (n, x)
        self.acc = self.acc << n | x
        self.n += n
        while self.n >= 8:
            self.n -= 8
            self.out.append(self.acc >> self.n)
            self.acc &= (1 << self.n) - 1

    def ue(self, x):
        assert x >= 0
        n = (x + 1).bit_length()
        self.u(2 * n - 1, x + 1)

    def se(self, x):
        self.ue(2 * x - 1 if x > 0 else -2 * x)

    def te(self, x, rng):                                          # 9.1.1: range 1 -> one inverted bit
        if rng == 1:
            self.u(1, 1 - x)
        else:
            self.ue(x)

    def align_zero(self):
        if self.n:
            self.u(8 - self.n, 0)

    def raw(self, b):
        assert self.n == 0
        self.out += bytes(b)

    def trailing(self):
        self.u(1, 1)
        self.align_zero()

    def bytes(self):
        assert self.n == 0
        return bytes(self.out)


def nal(ref_idc, typ, rbsp):
    """Annex B: start code, header byte, payload with emulation prevention (7.4.1.1): 03 goes in front of every byte <= 3 that follows two zero bytes."""
    return b"\x00\x00\x00\x01" + bytes([ref_idc << 5 | typ]) + re.sub(b"\x00\x00(?=[\x00-\x03])", b"\x00\x00\x03", rbsp)


LOG2_MAX_FRAME_NUM = 8
LOG2_MAX_POC_LSB = 8


def high_syntax(seq):
    """The PPS carries transform_8x8_mode_flag, pic_scaling_matrix_present_flag and second_chroma_qp_index_offset (7.3.2.2, after more_rbsp_data)"""
    return bool(seq.get("transform8x8", 0)) or "pps_lists" in seq or "second_chroma_qp_off" in seq


def scaling_matrix(b, lists, n):
    """7.3.2.1.1 / 7.3.2.2: the matrix present flag, then per list its present flag and scaling_list() (7.3.2.1.1.1).  lists[i]: None (absent: a fall-back
    rule applies), "default" (the first delta_scale makes nextScale 0: UseDefaultScalingMatrixFlag), or the 16 / 64 values in zig-zag order."""
    b.u(1, 0 if lists is None else 1)
    if lists is None:
        return
    assert len(lists) == 8
    for i in range(n):
        v = lists[i]
        b.u(1, 0 if v is None else 1)
        if v is None:
            continue
        if isinstance(v, str):
            assert v == "default"
            b.se(-8)                                                # nextScale = (8 - 8 + 256) % 256 = 0 at j = 0
            continue
        assert len(v) == (16 if i < 6 else 64) and all(1 <= x <= 255 for x in v), (i, v)
        last = 8
        for x in v:                                                 # every value coded: nextScale never becomes 0
            d = x - last
            b.se(d - 256 if d > 127 else (d + 256 if d < -128 else d))
            last = x


def sps(seq):
    b = Bits()
    w, h = seq["width"], seq["height"]
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    prof = seq.get("profile", 66)
    b.u(8, prof)
    b.u(8, {66: 0x80, 77: 0x40, 100: 0}[prof])                      # constraint_set0 / set1, reserved zero bits
    b.u(8, 40)                                                      # level_idc
    b.ue(0)                                                         # seq_parameter_set_id
    if prof == 100:
        b.ue(1)                                                     # chroma_format_idc: 4:2:0
        b.ue(0); b.ue(0)                                            # bit_depth_luma_minus8, bit_depth_chroma_minus8
        b.u(1, 0)                                                   # qpprime_y_zero_transform_bypass_flag
        scaling_matrix(b, seq.get("sps_lists"), 8)                  # seq_scaling_matrix_present_flag and the lists
    else:
        assert not high_syntax(seq) and "sps_lists" not in seq, "the 8x8 transform, scaling lists and the second chroma offset need profile 100"
    b.ue(LOG2_MAX_FRAME_NUM - 4)
    b.ue(0)                                                         # pic_order_cnt_type
    b.ue(LOG2_MAX_POC_LSB - 4)
    b.ue(seq.get("num_ref_frames", 1))
    b.u(1, 0)                                                       # gaps_in_frame_num_value_allowed_flag
    fmo = seq.get("frame_mbs_only", 1)                              # 0: the stream may hold field pictures (the scripts' pictures are all frames)
    assert fmo or mbh % 2 == 0
    b.ue(mbw - 1)
    b.ue((mbh if fmo else mbh // 2) - 1)                            # pic_height_in_map_units_minus1: field macroblock rows when frame_mbs_only_flag = 0
    b.u(1, fmo)                                                     # frame_mbs_only_flag
    if not fmo:
        b.u(1, 0)                                                   # mb_adaptive_frame_field_flag
    assert fmo or seq.get("direct_8x8_inference", 1), "7.4.2.1.1: frame_mbs_only_flag 0 needs direct_8x8_inference_flag 1"
    b.u(1, seq.get("direct_8x8_inference", 1))                      # direct_8x8_inference_flag
    cr, cb_ = mbw * 16 - w, mbh * 16 - h
    assert cr % 2 == 0 and cb_ % 2 == 0 and (fmo or cb_ % 4 == 0), "7.4.2.1.1: CropUnitY is SubHeightC * (2 - frame_mbs_only_flag) luma rows"
    if cr or cb_:
        b.u(1, 1)
        b.ue(0); b.ue(cr // 2); b.ue(0); b.ue(cb_ // (2 if fmo else 4))      # crop units: two luma samples; four luma rows when fields may occur
    else:
        b.u(1, 0)
    b.u(1, 0)                                                       # vui_parameters_present_flag
    b.trailing()
    return nal(3, 7, b.bytes())


def pps(seq):
    b = Bits()
    b.ue(0); b.ue(0)
    b.u(1, 0)                                                       # entropy_coding_mode_flag: CAVLC
    b.u(1, 0)                                                       # bottom_field_pic_order_in_frame_present_flag
    b.ue(0)                                                         # num_slice_groups_minus1
    n = seq.get("num_ref_frames", 1)
    b.ue(n - 1); b.ue(n - 1)                                        # num_ref_idx_l0 / l1_default_active_minus1
    b.u(1, seq.get("weighted_pred", 0))
    b.u(2, seq.get("weighted_bipred", 0))
    b.se(seq.get("init_qp", 26) - 26)
    b.se(0)                                                         # pic_init_qs_minus26
    b.se(seq.get("chroma_qp_off", 0))                               # chroma_qp_index_offset
    b.u(1, 1)                                                       # deblocking_filter_control_present_flag
    b.u(1, seq.get("constrained_intra", 0))                         # constrained_intra_pred_flag
    b.u(1, 0)                                                       # redundant_pic_cnt_present_flag
    if high_syntax(seq):
        assert seq.get("profile", 66) == 100
        t8 = seq.get("transform8x8", 0)
        b.u(1, t8)                                                  # transform_8x8_mode_flag
        scaling_matrix(b, seq.get("pps_lists"), 6 + 2 * t8)         # pic_scaling_matrix_present_flag and 6 + 2 * transform_8x8_mode_flag lists
        b.se(seq.get("second_chroma_qp_off", seq.get("chroma_qp_off", 0)))
    b.trailing()
    return nal(3, 8, b.bytes())


def ref_lists(pics, k, dpb):
    """8.2.4.2.1 / 8.2.4.2.3 for frames, short-term only: (RefPicList0, RefPicList1) of picture k as indices into pics; dpb = the reference pictures
    held when k is decoded, in decode order."""
    p = pics[k]
    if p["kind"] == "P":
        return dpb[::-1], []                                        # PicNum descending = most recently decoded first
    cur = p["poc"]
    before = sorted((i for i in dpb if pics[i]["poc"] < cur), key=lambda i: -pics[i]["poc"])
    after = sorted((i for i in dpb if pics[i]["poc"] > cur), key=lambda i: pics[i]["poc"])
    l0, l1 = before + after, after + before
    if len(l1) > 1 and l0 == l1:
        l1[0], l1[1] = l1[1], l1[0]
    return l0, l1


def pic_seq(seq, p):
    """The sequence as picture p sees it: a field picture is a picture of its own of half the coded rows (every per-picture routine takes this)."""
    return dict(seq, height=(seq["height"] + 15) // 16 * 8) if p.get("field") else seq


def second_field(pics, k):
    """picture k is the second field (decoding order) of a frame: the picture before it is a first field of the other parity"""
    f = pics[k].get("field")
    return bool(f) and k > 0 and pics[k - 1].get("field") not in (None, f) and not second_field(pics, k - 1)


def ref_name(pics, k, parity):
    """How a field picture's script names the field `parity` of the store that picture k belongs to: the field's own index when it was coded as a field,
    (index, parity) when it is one field of a picture coded as a frame"""
    return k if pics[k].get("field") else (k, parity)


def alternate_fields(stores, parity):
    """8.2.4.2.5: from the ordered stores (each {parity: name} of the fields it holds as references) fields are taken alternating in parity, starting
    with `parity`; a missing field is passed over; when one parity runs out the rest of the other follows in order."""
    other = "bottom" if parity == "top" else "top"
    same, opp = [s[parity] for s in stores if parity in s], [s[other] for s in stores if other in s]
    out = []
    while same and opp:
        out += [same.pop(0), opp.pop(0)]
    return out + same + opp


def plan_paff(seq, pics):
    """``plan`` for a stream with field pictures, short-term references only.  A store is a frame's worth of reference fields; PicNum of a field is
    2 * FrameNumWrap + 1 for the current parity and 2 * FrameNumWrap for the other (8.2.4.1), which for the list construction only says: stores by
    descending FrameNumWrap (8.2.4.2.2), then 8.2.4.2.5.  No frame_num wrap occurs (asserted)."""
    out, stores, frame_num = [], [], 0          # stores: dict(first=index, held={parity: index}, poc={parity: count}, frame_num) in decoding order
    nrf = seq.get("num_ref_frames", 1)
    assert not seq.get("frame_mbs_only", 1), "field pictures need frame_mbs_only=0"
    for k, p in enumerate(pics):
        par = p.get("field")
        assert par in (None, "top", "bottom")
        is_ref = p.get("is_ref", p["kind"] != "B")
        second = second_field(pics, k)
        if par and not second:
            assert k + 1 == len(pics) or second_field(pics, k + 1), "a first field is followed by the other field of its frame, or ends the stream"
        assert k > 0 or p["kind"] == "I"
        if second:
            assert is_ref == out[k - 1]["is_ref"], "both fields of a frame are reference fields or neither is"
        fn = out[k - 1]["frame_num"] if second else frame_num
        assert fn < (1 << LOG2_MAX_FRAME_NUM) - 1, "no frame_num wrap in these scripts"
        full = [s for s in stores if len(s["held"]) == 2]
        spoc = lambda s: min(s["poc"].values())                     # PicOrderCnt of a frame or pair: the smaller; of a single held field: its own
        l0, l1 = [], []
        if p["kind"] == "P" and par:
            l0 = alternate_fields([{q: ref_name(pics, i, q) for q, i in s["held"].items()} for s in stores[::-1]], par)
        elif p["kind"] == "P":
            l0 = [s["first"] for s in full[::-1]]                   # 8.2.4.2.1: frames (or pairs) with both fields marked, PicNum descending
        elif p["kind"] == "B":
            assert not is_ref or not par, "B fields are not references in these scripts"
            pool = stores if par else full
            cur = p["poc"]
            before = sorted((s for s in pool if spoc(s) <= cur), key=lambda s: -spoc(s))
            after = sorted((s for s in pool if spoc(s) > cur), key=spoc)
            if par:
                names = lambda ss: alternate_fields([{q: ref_name(pics, i, q) for q, i in s["held"].items()} for s in ss], par)
            else:
                names = lambda ss: [s["first"] for s in ss]
            l0, l1 = names(before + after), names(after + before)
            if len(l1) > 1 and l0 == l1:
                l1[0], l1[1] = l1[1], l1[0]
        cap = 2 * nrf if par else nrf
        n0, n1 = p.get("num_ref", (max(1, min(cap, len(l0))), max(1, min(cap, len(l1)))))
        if p["kind"] != "I":
            assert n0 <= len(l0) and (p["kind"] == "P" or n1 <= len(l1)) and max(n0, n1) <= (32 if par else 16), (k, n0, n1, l0, l1)
        out.append(dict(frame_num=fn, l0=l0[:n0], l1=l1[:n1], is_ref=is_ref, idr=k == 0, override=(n0, n1) != (nrf, nrf), n=(n0, n1)))
        if is_ref and second:
            s = stores[-1]
            assert s["first"] == k - 1
            s["held"][par], s["poc"][par] = k, p["poc"]             # 8.2.5.3: no sliding window for the second field of a reference frame
        elif is_ref:
            if len(stores) == nrf:
                stores.pop(0)                                       # sliding window, counted in frames: the smallest FrameNumWrap goes
            held = {par: k} if par else {"top": k, "bottom": k}
            stores.append(dict(first=k, held=held, poc={q: p["poc"] for q in held}, frame_num=fn))
        if is_ref and not second:
            frame_num = fn + 1
    return out


def plan(seq, pics):
    """Per picture: frame_num, the lists cut to their active length, nal_ref_idc.  Sliding window marking (8.2.5.3)."""
    if any(p.get("field") for p in pics):
        return plan_paff(seq, pics)
    out, dpb, frame_num = [], [], 0
    nrf = seq.get("num_ref_frames", 1)
    for k, p in enumerate(pics):
        is_ref = p.get("is_ref", p["kind"] != "B")
        if p["kind"] == "I" and k == 0:
            dpb, frame_num = [], 0
        l0, l1 = ([], []) if p["kind"] == "I" else ref_lists(pics, k, dpb)
        n0, n1 = p.get("num_ref", (max(1, min(nrf, len(l0))), max(1, min(nrf, len(l1)))))
        if p["kind"] != "I":
            # entries beyond the pictures held would be "no reference picture": the scripts never ask for them
            assert n0 <= len(l0) and (p["kind"] == "P" or n1 <= len(l1)), (k, n0, n1, l0, l1)
        out.append(dict(frame_num=frame_num, l0=l0[:n0], l1=l1[:n1], is_ref=is_ref, idr=k == 0, override=(n0, n1) != (nrf, nrf), n=(n0, n1)))
        if is_ref:
            dpb.append(k)
            if len(dpb) > nrf:
                dpb.pop(0)
            frame_num = (frame_num + 1) % (1 << LOG2_MAX_FRAME_NUM)
    return out


def slice_fields(seq, p, step, m):
    """(SliceQPY, (disable_deblocking_filter_idc, alpha_div2, beta_div2)) of the slice that starts at macroblock m: layout "mb" lets the macroblock say"""
    qp, db = p.get("qp", seq.get("init_qp", 26)), p.get("deblock", (1, 0, 0))
    if step == 1:
        qp, db = m.get("qp", qp), m.get("deblock", db)
    else:
        assert "qp" not in m and "deblock" not in m, "per-macroblock qp / deblock need layout mb"
    return qp, db


def layout_step(seq, p):
    mbw, mbh = (seq["width"] + 15) // 16, (seq["height"] + 15) // 16
    lay = p.get("layout", "mb" if p["kind"] != "I" else "pic")
    if isinstance(lay, int):                                        # slices of `lay` macroblocks each: a slice may begin in mid-row
        assert 1 <= lay <= mbw * mbh
        return lay
    return {"mb": 1, "row": mbw, "pic": mbw * mbh}[lay]


def mb_qps(seq, p):
    """QPY of every macroblock (7.4.5): QPY,PRED is the QPY of the previous macroblock of the slice in decoding order, SliceQPY for the first; a
    macroblock without mb_qp_delta (I_PCM included: the value is inferred to be 0) keeps QPY,PRED.  That the deblocking filter takes qPp = 0 for an I_PCM
    macroblock is a rule of 8.7.2.2 alone (tests/deblock_ref.py) and does not touch this chain."""
    step, out = layout_step(seq, p), []
    for a, m in enumerate(p["mbs"]):
        if a % step == 0:
            pred = slice_fields(seq, p, step, m)[0]
        qp = (pred + m.get("dqp", 0) + 52) % 52
        assert 0 <= pred <= 51 and -26 <= m.get("dqp", 0) <= 25
        out.append(qp)
        pred = qp
    return out


BLK_XY = [(((k >> 2) & 1) * 8 + (k & 1) * 4, ((k >> 3) & 1) * 8 + ((k >> 1) & 1) * 4) for k in range(16)]      # 6.4.3: luma4x4BlkIdx -> (x, y)
_COEFF_TOKEN = parse_code_table(COEFF_TOKEN, 5)
_TOTAL_ZEROS = parse_code_table(TOTAL_ZEROS_4x4, 15)


def one_dc_coefficient(b, blk, sign):
    """coded_block_pattern, mb_qp_delta and residual_luma of an Inter macroblock whose only coefficient is level `sign` at scan position 0 of block blk."""
    b8 = blk >> 2
    b.ue([c[1] for c in CBP_OF_CODENUM].index(1 << b8))               # me(v), Table 9-4, Inter column
    b.se(0)                                                         # mb_qp_delta
    total = {blk: 1}                                                # total_coeff of the blocks coded so far (others: 0)
    at = {xy: k for k, xy in enumerate(BLK_XY)}
    for k in range(4 * b8, 4 * b8 + 4):
        x, y = BLK_XY[k]
        # 9.2.1: blkA / blkB inside this macroblock are available (in an 8x8 without coded coefficients: total_coeff 0); outside it lies another slice
        na = total.get(at[(x - 4, y)], 0) if x > 0 else None
        nb = total.get(at[(x, y - 4)], 0) if y > 0 else None
        nc = (na + nb + 1) >> 1 if na is not None and nb is not None else (na if na is not None else (nb if nb is not None else 0))
        assert nc in (0, 1), nc
        ln, val = _COEFF_TOKEN[(1, 1) if k == blk else (0, 0)][0]       # column 0 <= nC < 2
        b.u(ln, val)
        if k == blk:
            b.u(1, 0 if sign > 0 else 1)                            # trailing_ones_sign_flag
            ln, val = _TOTAL_ZEROS[(0,)][0]                         # total_zeros 0, tzVlcIndex 1: the coefficient sits at scan position 0, the DC
            b.u(ln, val)


_TOTAL_ZEROS_CDC = parse_code_table(TOTAL_ZEROS_CHROMA_DC, 3)
_RUN_BEFORE = parse_code_table(RUN_BEFORE, 7)
INTRA = ("pcm", "i16", "i4", "i8")


def put(b, code):
    assert code is not None, "the table has no code for this combination"
    b.u(*code)


def residual_block(b, lv, nc, high, seen=None):
    """residual_block_cavlc (7.3.5.3.2, 9.2) of the levels lv in scan order (4, 15 or 16 of them) under nC = nc; returns TotalCoeff.  high: profile 100,
    which alone may use level_prefix 16.  seen: a set that receives what the block exercised (tests/analytic_h264_recon.py asserts from it)."""
    seen = seen if seen is not None else set()
    max_num = len(lv)
    nz = [i for i, v in enumerate(lv) if v]
    total = len(nz)
    t1 = 0
    for i in reversed(nz):                                          # trailing ones: up to three +-1 at the high-frequency end
        if abs(lv[i]) != 1 or t1 == 3:
            break
        t1 += 1
    col = 4 if nc == -1 else (0 if nc < 2 else (1 if nc < 4 else (2 if nc < 8 else 3)))
    seen.add(("nC", col))
    put(b, _COEFF_TOKEN[(t1, total)][col])
    if total == 0:
        return 0
    sl = 1 if total > 10 and t1 < 3 else 0                          # suffixLength
    if sl:
        seen.add("more_than_10_coefficients_fewer_than_3_trailing_ones")
    for k, i in enumerate(reversed(nz)):
        v = lv[i]
        if k < t1:
            b.u(1, int(v < 0))                                      # trailing_ones_sign_flag
            continue
        code = 2 * v - 2 if v > 0 else -2 * v - 1                   # levelCode
        if k == t1 and t1 < 3:
            code -= 2                                               # the first level after fewer than three trailing ones cannot be +-1
            seen.add("minus_2_after_fewer_than_3_trailing_ones")
        seen.add(("suffixLength", sl))
        # 9.2.2.1 backwards: levelCode = (Min(15, level_prefix) << suffixLength) + level_suffix, + 15 when level_prefix >= 15 and suffixLength = 0,
        # + (1 << (level_prefix - 3)) - 4096 when level_prefix >= 16; levelSuffixSize 4 for prefix 14 at suffixLength 0, level_prefix - 3 from 15 on
        if sl == 0 and code < 14:
            pre, nsuf, suf = code, 0, 0
        elif sl == 0 and code < 30:
            pre, nsuf, suf = 14, 4, code - 14
        elif sl > 0 and code < (15 << sl):
            pre, nsuf, suf = code >> sl, sl, code & ((1 << sl) - 1)
        else:
            rest = code - (15 << sl) - (15 if sl == 0 else 0)
            if rest < 4096:
                pre, nsuf, suf = 15, 12, rest
            else:
                assert high and rest < 4096 + 8192, "a level that needs level_prefix 16 (or more) -- profile 100 only, and 16 is the most this writer states"
                pre, nsuf, suf = 16, 13, rest - 4096
        if sl == 0 and pre >= 14 or pre == 16:
            seen.add(("level_prefix", pre, sl))
        b.u(pre + 1, 1)                                             # level_prefix: `pre` zeros and a one
        if nsuf:
            b.u(nsuf, suf)
        if sl == 0:
            sl = 1
        if abs(v) > (3 << (sl - 1)) and sl < 6:
            sl += 1
    if total < max_num:
        tz = nz[-1] + 1 - total                                     # zeros below the last coefficient
        put(b, (_TOTAL_ZEROS_CDC if max_num == 4 else _TOTAL_ZEROS)[(tz,)][total - 1])
        left = tz
        for k in range(total - 1, 0, -1):                           # run_before of every coefficient but the lowest, from the highest down
            if left == 0:
                break
            run = nz[k] - nz[k - 1] - 1
            if run > 6:
                seen.add("run_before_above_6")
            put(b, _RUN_BEFORE[(run,)][min(left, 7) - 1])
            left -= run
    return total


def mb_levels(m, field=False):
    """The levels of macroblock m in PARSING form, from its coef=dict(...) (every matrix there is in raster order):
    dc16: the 16 Intra16x16DCLevel in scan order or None; y[blk]: 16 (15 for Intra16x16: the AC) levels of every luma 4x4 block in scan order -- under the
    8x8 transform the four interleaved blocks of 7.3.5.3.1 (CAVLC): block i of an 8x8 takes levels 4 k + i of its 64; cdc[plane]: 4; cac[plane][blk]: 15;
    and the coded_block_pattern that follows from them: (luma bits, chroma 0 | 1 | 2).  field: the macroblock belongs to a field picture, where EVERY
    block is scanned by the field scans of 8.5.6 / 8.5.7 (the Intra16x16 DC matrix and the chroma AC blocks among them)."""
    ZIGZAG_4x4, ZIGZAG_8x8 = (FIELD_SCAN_4x4, FIELD_SCAN_8x8) if field else (FRAME_SCAN_4x4, FRAME_SCAN_8x8)
    c = m.get("coef", {})
    t = m["t"]
    assert set(c) <= {"y", "y8", "ydc", "cdc", "cac"} and t != "pcm" and t != "skip", (t, sorted(c))
    t8 = t == "i8" or m.get("t8", 0)
    assert ("y8" not in c or t8) and ("y" not in c or not t8) and ("ydc" not in c or t == "i16") and (not t8 or t != "i16")
    y = [[0] * (15 if t == "i16" else 16) for _ in range(16)]
    for blk, lv in c.get("y", {}).items():
        lv = [int(v) for v in np.asarray(lv).reshape(16)]
        assert t != "i16" or lv[0] == 0, "the DC of an Intra16x16 block is coded in ydc"
        y[blk] = [lv[ZIGZAG_4x4[k]] for k in range(1 if t == "i16" else 0, 16)]
    for b8, lv in c.get("y8", {}).items():
        lv = [int(v) for v in np.asarray(lv).reshape(64)]
        scan = [lv[ZIGZAG_8x8[k]] for k in range(64)]
        for i in range(4):
            y[4 * b8 + i] = scan[i::4]
    dc16 = None
    if t == "i16":
        lv = [int(v) for v in np.asarray(c.get("ydc", [0] * 16)).reshape(16)]
        dc16 = [lv[ZIGZAG_4x4[k]] for k in range(16)]
    cdc = [[int(v) for v in q] for q in c.get("cdc", ([0] * 4, [0] * 4))]
    cac = [[[0] * 15 for _ in range(4)] for _ in range(2)]
    for (pl_, blk), lv in c.get("cac", {}).items():
        lv = [0] + [int(v) for v in lv]
        assert len(lv) == 16
        cac[pl_][blk] = [lv[ZIGZAG_4x4[k]] for k in range(1, 16)]
    luma = sum(1 << b8 for b8 in range(4) if any(any(y[4 * b8 + i]) for i in range(4)))
    if t == "i16" and luma:
        luma = 15                                                   # Table 7-11: Intra16x16 has all of the AC or none of it
    chroma = 2 if any(any(q) for pl_ in cac for q in pl_) else (1 if any(any(q) for q in cdc) else 0)
    return dict(dc16=dc16, y=y, cdc=cdc, cac=cac, cbp=(luma, chroma), t8=int(bool(t8)))


def coded_luma_blocks(m):
    """The luma 4x4 blocks of m that 8.7.2.1 counts as "containing non-zero transform coefficients": under the 8x8 transform all four blocks of an 8x8
    that has one (the Intra16x16 DC levels count for no block: such a macroblock is intra, where the coefficients do not decide bS)."""
    if "resid" in m:
        return {m["resid"][0]}
    if "coef" not in m:
        return set()
    lv = mb_levels(m)
    if lv["t8"]:
        return {4 * b8 + i for b8 in range(4) for i in range(4) if any(any(lv["y"][4 * b8 + j]) for j in range(4))}
    return {k for k in range(16) if any(lv["y"][k])}


class PicState:
    """What one macroblock's syntax needs of the macroblocks before it: TotalCoeff of every 4x4 block (9.2.1), the Intra4x4 / Intra8x8 modes (8.3.1.1,
    8.3.2.1), whether a macroblock is inter.  Availability (6.4.x): inside the picture and in the same slice."""
    def __init__(self, seq, mbs, step):
        self.mbw = (seq["width"] + 15) // 16
        self.mbs, self.step = mbs, step
        self.constrained = seq.get("constrained_intra", 0)
        self.tc = [None] * len(mbs)                                 # per macroblock: [16 luma by (y / 4) * 4 + x / 4, 4 Cb, 4 Cr]
        self.modes = [None] * len(mbs)                              # per macroblock: 16 modes by (y / 4) * 4 + x / 4 (an 8x8 mode fills its four 4x4 blocks)

    def neighbour(self, a, dx, dy):
        """address of the macroblock at (dx, dy) macroblocks from a, or None when it is not available"""
        x, y = a % self.mbw + dx, a // self.mbw + dy
        n = y * self.mbw + x
        return n if 0 <= x < self.mbw and y >= 0 and n >= a - a % self.step and n < a else None

    def locate(self, a, px, py, size):
        """(macroblock address or None, px, py) of the sample (px, py) relative to macroblock a; px < size, py < size (left, above or inside)"""
        dx, dy = (-1 if px < 0 else 0), (-1 if py < 0 else 0)
        return (a if (dx, dy) == (0, 0) else self.neighbour(a, dx, dy)), px % size, py % size

    def n_c(self, a, comp, bx, by):
        """9.2.1 for the block at (bx, by) (in blocks) of component comp (0 luma: 4x4 blocks, 1 / 2 chroma: 2x2) of macroblock a"""
        g = 4 if comp == 0 else 2
        base = (0, 16, 20)[comp]
        n = []
        for (qx, qy) in ((bx - 1, by), (bx, by - 1)):
            mb, qx, qy = self.locate(a, qx, qy, g)
            n.append(None if mb is None else self.tc[mb][base + qy * g + qx])
        na, nb = n
        return (na + nb + 1) >> 1 if na is not None and nb is not None else (na if na is not None else (nb if nb is not None else 0))

    def pred_mode(self, a, x, y):
        """predIntra4x4PredMode / predIntra8x8PredMode of the block whose upper left sample is (x, y).  With an 8x8 mode stored in all four 4x4 blocks it
        covers, both clauses read: A is the 4x4 block that holds (x - 4, y), B the one that holds (x, y - 4) -- for an 8x8 block beside an Intra4x4
        macroblock these are that macroblock's blocks 8x8idx * 4 + 1 and 8x8idx * 4 + 2, as 8.3.2.1 says."""
        out = []
        for (qx, qy) in ((x - 4, y), (x, y - 4)):
            mb, qx, qy = self.locate(a, qx, qy, 16)
            if mb is None or (self.constrained and self.mbs[mb]["t"] not in INTRA):
                return 2                                            # dcPredModePredictedFlag
            out.append(self.modes[mb][(qy // 4) * 4 + qx // 4] if self.mbs[mb]["t"] in ("i4", "i8") else 2)
        return min(out)


def mv_predictor_16x16(st, a, ref):
    """8.4.1.3 for a 16x16 partition of a P macroblock in a slice of 16x16 inter and intra macroblocks (no P_Skip): neighbours A, B, C (D when C is not
    available); an intra or unavailable neighbour has no reference; B and C both unavailable and A available: A stands for all three; one matching
    reference: its vector; else the median."""
    def of(n):
        if n is None:
            return None
        m = st.mbs[n]
        assert m["t"] in INTRA or m["t"] == "16x16", "a slice of several macroblocks holds 16x16 inter and intra macroblocks only"
        return (m["l0"][0], m["l0"][1]) if m["t"] == "16x16" else (None, (0, 0))
    A, B, C = of(st.neighbour(a, -1, 0)), of(st.neighbour(a, 0, -1)), of(st.neighbour(a, 1, -1))
    if C is None:
        C = of(st.neighbour(a, -1, -1))
    if B is None and C is None and A is not None:
        B = C = A
    A, B, C = [(None, (0, 0)) if q is None else q for q in (A, B, C)]
    same = [q for q in (A, B, C) if q[0] == ref]
    if len(same) == 1:
        return same[0][1]
    return tuple(sorted(q[1][i] for q in (A, B, C))[1] for i in (0, 1))


def macroblock_residual(b, st, a, m, lv, high, seen):
    """residual() of 7.3.5.3 for CAVLC and 4:2:0, and the TotalCoeff bookkeeping of 9.2.1"""
    tc = st.tc[a]
    luma, chroma = lv["cbp"]
    if m["t"] == "i16":
        residual_block(b, lv["dc16"], st.n_c(a, 0, 0, 0), high, seen)      # Intra16x16DCLevel: nC of block 0; its TotalCoeff is stored nowhere
    for k in range(16):
        bx, by = BLK_XY[k][0] // 4, BLK_XY[k][1] // 4
        if luma >> (k >> 2) & 1:
            tc[by * 4 + bx] = residual_block(b, lv["y"][k], st.n_c(a, 0, bx, by), high, seen)
    if chroma:
        for c in (0, 1):
            residual_block(b, lv["cdc"][c], -1, high, seen)
    if chroma == 2:
        for c in (0, 1):
            for k in range(4):
                tc[16 + 4 * c + k] = residual_block(b, lv["cac"][c][k], st.n_c(a, 1 + c, k & 1, k >> 1), high, seen)


MVD_RANGE = 8191                                                    # the largest |mvd| (quarter samples) these scripts state through se(v)
_P_NAMES, _B_NAMES = [q[0] for q in MB_TYPE_P], [q[0] for q in MB_TYPE_B]
_PSUB_NAMES, _BSUB_NAMES = [q[0] for q in SUB_MB_TYPE_P], [q[0] for q in SUB_MB_TYPE_B]


def uses_new_forms(seq, p):
    """The picture holds a macroblock that states syntax, not motion (t="mv"), or a skipped macroblock whose vector a neighbour may decide"""
    step = layout_step(seq, p)
    return any(m["t"] == "mv" or (m["t"] == "skip" and (step > 1 or p["kind"] == "B")) for m in p["mbs"])


def mv_shape(kind, m):
    """Of a t="mv" macroblock: (mb_type value, name, [prediction mode per partition], [sub-partition count per partition], [sub_mb_type values] or
    None, [(x, y, w, h) of every partition's every sub-partition]) from Tables 7-13 / 7-14 / 7-17 / 7-18 and 6.4.2.1 / 6.4.2.2"""
    names, table = (_P_NAMES, MB_TYPE_P) if kind == "P" else (_B_NAMES, MB_TYPE_B)
    assert kind in ("P", "B") and m["mb"] in names, (kind, m["mb"])
    v = names.index(m["mb"])
    name, nparts, modes, pw, ph = table[v]
    if name == "B_Direct_16x16":
        assert not ({"ref", "mvd", "sub"} & set(m)), "B_Direct_16x16 carries no motion syntax"
        return v, name, ["Direct"] * 4, [4] * 4, None, [[(8 * (i & 1) + 4 * (j & 1), 8 * (i >> 1) + 4 * (j >> 1), 4, 4) for j in range(4)] for i in range(4)]
    if modes is not None:
        assert "sub" not in m
        rects = [[((i * pw) % 16, (i * pw) // 16 * ph, pw, ph)] for i in range(nparts)]
        return v, name, list(modes), [1] * nparts, None, rects
    snames, stable = (_PSUB_NAMES, SUB_MB_TYPE_P) if kind == "P" else (_BSUB_NAMES, SUB_MB_TYPE_B)
    assert len(m["sub"]) == 4 and all(s in snames for s in m["sub"]), m["sub"]
    subs = [snames.index(s) for s in m["sub"]]
    rects = []
    for i, s in enumerate(subs):
        _, n, _, w, h = stable[s]
        rects.append([(8 * (i & 1) + (j * w) % 8, 8 * (i >> 1) + (j * w) // 8 * h, w, h) for j in range(n)])
    return v, name, [stable[s][2] for s in subs], [stable[s][1] for s in subs], subs, rects


def transform8x8_flag_allowed(seq, kind, m):
    """7.3.5: the condition under which transform_size_8x8_flag follows a non-zero luma pattern of an inter macroblock: no sub-macroblock partition
    smaller than 8x8, a direct sub-macroblock or B_Direct_16x16 only with direct_8x8_inference_flag"""
    _, name, modes, counts, subs, _ = mv_shape(kind, m)
    inf = seq.get("direct_8x8_inference", 1)
    if name == "B_Direct_16x16":
        return bool(inf)
    if subs is None:
        return True
    return all((inf if mode == "Direct" else n == 1) for mode, n in zip(modes, counts))


def inter_syntax(b, kind, pl, m):
    """mb_type and mb_pred() / sub_mb_pred() (7.3.5.1, 7.3.5.2) of a macroblock that states its syntax: ref_idx per partition and list, mvd per
    (sub-)partition and list.  Nothing is derived."""
    v, name, modes, counts, subs, _ = mv_shape(kind, m)
    b.ue(v)
    if name == "B_Direct_16x16":
        return
    for s in subs or []:
        b.ue(s)
    ref, mvd = m["ref"], m["mvd"]
    uses = lambda l, i: modes[i] in (("L0", "Bi"), ("L1", "Bi"))[l]
    assert kind == "B" or all(q is None for q in ref[1]) and all(q is None for q in mvd[1])
    for l in (0, 1):
        assert len(ref[l]) == len(modes) and len(mvd[l]) == len(modes)
        for i in range(len(modes)):
            if not uses(l, i):
                assert ref[l][i] is None and mvd[l][i] is None, ("this partition does not use list %d" % l, name, i)
                continue
            assert ref[l][i] is not None and 0 <= ref[l][i] < pl["n"][l], ("ref_idx outside the active list", name, l, i, ref[l][i], pl["n"])
            if name == "P_8x8ref0":
                assert ref[l][i] == 0                                   # not sent: inferred 0
            elif pl["n"][l] > 1:
                b.te(ref[l][i], pl["n"][l] - 1)                       # range 1: nothing sent; 2: the inverted bit; more: ue(v)
    for l in (0, 1):
        for i in range(len(modes)):
            if uses(l, i):
                assert len(mvd[l][i]) == counts[i], (name, l, i)
                for d in mvd[l][i]:
                    assert all(-MVD_RANGE <= c <= MVD_RANGE for c in d), ("mvd outside the scripted range of se(v)", d)
                    b.se(d[0]); b.se(d[1])


def one_dc_coefficient_in_slice(b, st, a, blk, sign, t8_flag, high):
    """``one_dc_coefficient`` where neighbouring macroblocks may be available: nC from the TotalCoeff bookkeeping of 9.2.1; t8_flag: transform_size_8x8_
    flag is present (and 0: the coefficient belongs to a 4x4 block)"""
    b8 = blk >> 2
    b.ue([c[1] for c in CBP_OF_CODENUM].index(1 << b8))
    if t8_flag:
        b.u(1, 0)
    b.se(0)                                                         # mb_qp_delta
    for k in range(4 * b8, 4 * b8 + 4):
        bx, by = BLK_XY[k][0] // 4, BLK_XY[k][1] // 4
        st.tc[a][by * 4 + bx] = residual_block(b, [sign if k == blk else 0] + [0] * 15, st.n_c(a, 0, bx, by), high)


def slice_header(b, seq, p, pl, first_mb):
    kind = p["kind"]
    b.ue(first_mb)
    b.ue({"P": 0, "B": 1, "I": 2}[kind])
    b.ue(0)                                                         # pic_parameter_set_id
    b.u(LOG2_MAX_FRAME_NUM, pl["frame_num"])
    if not seq.get("frame_mbs_only", 1):
        b.u(1, int(bool(p.get("field"))))                           # field_pic_flag
        if p.get("field"):
            b.u(1, int(p["field"] == "bottom"))                     # bottom_field_flag
    if pl["idr"]:
        b.ue(0)                                                     # idr_pic_id
    b.u(LOG2_MAX_POC_LSB, p["poc"] % (1 << LOG2_MAX_POC_LSB))
    if kind == "B":
        b.u(1, p.get("direct_spatial", 1))                          # direct_spatial_mv_pred_flag
    if kind != "I":
        b.u(1, int(pl["override"]))
        if pl["override"]:
            b.ue(pl["n"][0] - 1)
            if kind == "B":
                b.ue(pl["n"][1] - 1)
        b.u(1, 0)                                                   # ref_pic_list_modification_flag_l0
        if kind == "B":
            b.u(1, 0)
    if (kind == "P" and seq.get("weighted_pred", 0)) or (kind == "B" and seq.get("weighted_bipred", 0) == 1):
        wp = p.get("wp", dict(ld_y=0, ld_c=0))                      # no table in the script: denominators 0, every flag off
        b.ue(wp["ld_y"]); b.ue(wp["ld_c"])
        for l, n in (("l0", pl["n"][0]),) + ((("l1", pl["n"][1]),) if kind == "B" else ()):
            ent = wp.get(l, [])
            for i in range(n):
                e = ent[i] if i < len(ent) and ent[i] else {}
                for key in ("y", "c"):
                    v = e.get(key)
                    b.u(1, 0 if v is None else 1)
                    if v is not None:
                        for w_, o_ in ([v] if key == "y" else v):
                            b.se(w_); b.se(o_)
    if pl["is_ref"]:
        if pl["idr"]:
            b.u(1, 0); b.u(1, 0)                                    # no_output_of_prior_pics_flag, long_term_reference_flag
        else:
            b.u(1, 0)                                               # adaptive_ref_pic_marking_mode_flag: sliding window
    b.se(p.get("qp", seq.get("init_qp", 26)) - seq.get("init_qp", 26))
    idc, a, be = p.get("deblock", (1, 0, 0))
    b.ue(idc)
    if idc != 1:
        b.se(a); b.se(be)


def coeff_token_zero(b, nc):
    """Table 9-5, TotalCoeff 0 / TrailingOnes 0."""
    if nc < 2:
        b.u(1, 1)
    elif nc < 4:
        b.u(2, 3)
    elif nc < 8:
        b.u(4, 15)
    else:
        b.u(6, 3)


def intra_pred_modes(b, st, a, m):
    """mb_pred of I_NxN (7.3.5.1): prev_intra4x4 / 8x8_pred_mode_flag and rem_intra4x4 / 8x8_pred_mode of every block, in block order"""
    n = 16 if m["t"] == "i4" else 4
    assert len(m["modes"]) == n and all(0 <= q <= 8 for q in m["modes"])
    st.modes[a] = [None] * 16
    coded = []
    for k, mode in enumerate(m["modes"]):
        x, y = BLK_XY[k] if n == 16 else ((k & 1) * 8, (k >> 1) * 8)
        pred = st.pred_mode(a, x, y)
        for j in ([0] if n == 16 else [0, 1, 4, 5]):
            st.modes[a][(y // 4) * 4 + x // 4 + j] = mode
        flag, rem = (1, None) if mode == pred else (0, mode if mode < pred else mode - 1)
        assert flag or (0 <= rem <= 7 and (rem if rem < pred else rem + 1) == mode), (mode, pred)
        b.u(1, flag)
        if not flag:
            b.u(3, rem)
        coded.append((pred, flag, rem))
    return coded


def write(seq, pics, seen=None, coded_modes=None):
    """The Annex-B stream of the script.  seen: a set that receives what the residual blocks exercised; coded_modes: a dict that receives, per (picture,
    macroblock), the (predicted mode, prev flag, rem) of every Intra4x4 / Intra8x8 block as written."""
    mbw = (seq["width"] + 15) // 16
    mbh = (seq["height"] + 15) // 16
    n_mbs = mbw * mbh
    high = seq.get("profile", 66) == 100
    t8mode = seq.get("transform8x8", 0)
    out = [sps(seq), pps(seq)]
    frame_mbs, frame_seq = n_mbs, seq
    for k, (p, pl) in enumerate(zip(pics, plan(seq, pics))):
        kind, mbs = p["kind"], p["mbs"]
        field = bool(p.get("field"))
        seq = pic_seq(frame_seq, p)                                 # a field: mbw x mbh / 2 macroblocks, first_mb_in_slice counts them
        n_mbs = frame_mbs // 2 if field else frame_mbs
        assert len(mbs) == n_mbs
        step = layout_step(seq, p)
        mb_qps(seq, p)                                              # its assertions
        st = PicState(seq, mbs, step)
        new_forms = uses_new_forms(seq, p)
        if new_forms:
            assert not field and frame_seq.get("frame_mbs_only", 1), "the forms that state syntax are for frame pictures of progressive streams"
            assert all(m["t"] in INTRA + ("mv", "skip") for m in mbs), "a picture states its motion syntax in every inter macroblock or in none"
        for first in range(0, n_mbs, step):
            b = Bits()
            qp, db = slice_fields(seq, p, step, mbs[first])
            slice_header(b, seq, dict(p, qp=qp, deblock=db), pl, first)
            skip_run = 0
            for a in range(first, min(first + step, n_mbs)):
                m = mbs[a]
                t = m["t"]
                st.tc[a] = [16 if t == "pcm" else 0] * 24            # 9.2.1: I_PCM counts 16, a skipped macroblock and a block without levels 0
                if t == "skip":
                    assert kind == "P" and step == 1 or (kind != "I" and new_forms)
                    assert kind == "P" or pl["l1"], "B_Skip is direct prediction: RefPicList1[0] must exist"
                    skip_run += 1
                    continue
                if kind != "I":
                    b.ue(skip_run)
                    skip_run = 0
                intra_base = {"I": 0, "P": 5, "B": 23}[kind]
                lv = mb_levels(m, field) if t != "pcm" else None
                assert "coef" not in m or "resid" not in m
                if t == "pcm":
                    b.ue(intra_base + 25)
                    b.align_zero()                                  # pcm_alignment_zero_bit
                    b.raw(np.asarray(m["y"], np.uint8).tobytes() + np.asarray(m["cb"], np.uint8).tobytes() + np.asarray(m["cr"], np.uint8).tobytes())
                    continue
                if t == "i16":
                    luma, chroma = lv["cbp"]
                    b.ue(intra_base + 1 + m["mode"] + 4 * chroma + (12 if luma else 0))      # Table 7-11: I_16x16_<mode>_<chroma>_<luma 0 | 15>
                    b.ue(m["cmode"])                                # intra_chroma_pred_mode
                elif t in ("i4", "i8"):
                    b.ue(intra_base)                                # I_NxN
                    assert t == "i4" or t8mode, "Intra8x8 needs transform8x8=1"
                    if t8mode:
                        b.u(1, int(t == "i8"))                      # transform_size_8x8_flag
                    coded = intra_pred_modes(b, st, a, m)
                    if coded_modes is not None:
                        coded_modes[(k, a)] = coded
                    b.ue(m["cmode"])                                # intra_chroma_pred_mode
                elif t == "mv":
                    assert "coef" not in m and "t8" not in m, "the forms that state syntax carry resid= at most"
                    assert "Direct" not in mv_shape(kind, m)[2] or pl["l1"], "direct prediction: RefPicList1[0] must exist"
                    inter_syntax(b, kind, pl, m)
                    flag = bool(t8mode) and transform8x8_flag_allowed(frame_seq, kind, m)
                    if seen is not None:
                        seen.add(("transform_size_8x8_flag_possible", m["mb"], flag, "resid" in m))
                    if "resid" in m:
                        one_dc_coefficient_in_slice(b, st, a, m["resid"][0], m["resid"][1], flag, high)
                    else:
                        b.ue([c[1] for c in CBP_OF_CODENUM].index(0))    # coded_block_pattern 0: nothing follows
                    continue
                else:
                    parts = [(m.get("l0"), m.get("l1"))] if t == "16x16" else [(q, None) for q in m["parts"]]
                    if kind == "P":
                        assert all(q[1] is None and q[0] is not None for q in parts)
                        b.ue({"16x16": 0, "16x8": 1, "8x16": 2}[t])
                    else:
                        assert t == "16x16"
                        b.ue(1 if parts[0][1] is None else (2 if parts[0][0] is None else 3))     # B_L0_16x16, B_L1_16x16, B_Bi_16x16
                    for l in (0, 1):
                        lst, n = pl["l%d" % l], pl["n"][l]
                        assert all(q[l] is None or q[l][0] in lst for q in parts), ("a reference that is not in the picture's list", k, a, lst)
                        for q in parts:
                            if q[l] is not None and n > 1:
                                b.te(lst.index(q[l][0]), n - 1)
                            elif q[l] is not None:
                                assert lst.index(q[l][0]) == 0
                    for l in (0, 1):
                        for i, q in enumerate(parts):
                            if q[l] is None:
                                continue
                            mv = q[l][1]
                            if step == 1:
                                # no neighbouring macroblock is available.  16x16 / first partition: predictor (0, 0).  Second partition (8.4.1.3): 16x8 --
                                # A, C, D lie outside, B is the upper partition: its vector when the reference indices match, else median(0, B, 0) = 0;
                                # 8x16 -- only A (the left partition) is available, so B and C take A's vector and reference: the predictor is A's vector
                                mvp = (0, 0)
                                if i == 1 and (t == "8x16" or parts[0][l][0] == q[l][0]):
                                    mvp = parts[0][l][1]
                            else:
                                inter = [(q_.get("l0"), q_.get("l1")) for q_ in mbs[first:min(first + step, n_mbs)] if q_["t"] == "16x16"]
                                whole = len(inter) == min(first + step, n_mbs) - first
                                if all(q_ == inter[0] for q_ in inter) and (whole or mbw == 1):
                                    # every macroblock of this slice is the same 16x16 block: as soon as one neighbour exists, every available neighbour
                                    # holds this vector and reference, and each branch of 8.4.1.3 (one neighbour, one matching reference, median)
                                    # returns it.  With intra macroblocks in between in a picture ONE macroblock wide: A, C and D lie outside the
                                    # picture, B is the macroblock above -- inter in this slice: the one neighbour whose reference matches, the
                                    # predictor is its vector (this vector); intra or in another slice: no reference matches, median(0, 0, 0)
                                    mvp = ((0, 0) if a == first else mv) if whole else (mv if a > first and mbs[a - 1]["t"] == "16x16" else (0, 0))
                                    assert kind != "P" or mvp == mv_predictor_16x16(st, a, q[l][0])
                                else:
                                    # any mixture of 16x16 P macroblocks and intra macroblocks: 8.4.1.3 typed out
                                    assert kind == "P" and t == "16x16"
                                    mvp = mv_predictor_16x16(st, a, q[l][0])
                            b.se(mv[0] - mvp[0]); b.se(mv[1] - mvp[1])
                    if "resid" in m:
                        assert kind == "P" and step == 1 and not t8mode
                        one_dc_coefficient(b, *m["resid"])
                        continue
                luma, chroma = lv["cbp"]
                if t != "i16":
                    b.ue([c[0 if t in INTRA else 1] for c in CBP_OF_CODENUM].index(luma | chroma << 4))      # coded_block_pattern: me(v), Table 9-4
                    if t not in INTRA and luma and t8mode:
                        b.u(1, lv["t8"])                            # transform_size_8x8_flag of an inter macroblock without sub-partitions
                    else:
                        assert t in INTRA or not lv["t8"], "t8=1 needs transform8x8=1 and luma levels"
                if t == "i16" or luma or chroma:
                    b.se(m.get("dqp", 0))                           # mb_qp_delta
                    macroblock_residual(b, st, a, m, lv, high, seen)
                else:
                    assert m.get("dqp", 0) == 0, "a macroblock without levels has no mb_qp_delta"
            if skip_run:
                b.ue(skip_run)
            b.trailing()
            out.append(nal(1 if pl["is_ref"] else 0, 5 if pl["idr"] else 1, b.bytes()))
    return b"".join(out)
