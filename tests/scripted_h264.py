"""A scripted H.264 stream writer (CAVLC, pic_order_cnt_type 0, frame pictures, Baseline / Main subset) for the analytic known-answer tests.

The test says which macroblock carries which samples, vector, reference, weight and mode; ``write`` turns that script into Annex-B bytes.  No residual is
ever coded, so the decoded picture follows from the script by arithmetic alone (tests/analytic_expect.py).  Typed from the syntax clauses (7.3.2.1, 7.3.2.2,
7.3.3, 7.3.4, 7.3.5, 9.1, 9.2.1) -- not from tools/h264gen.c, the oracle or the product: a fourth typing of the syntax is part of the value.

The script
    seq  = dict(width, height, num_ref_frames=1, profile=66 | 77, weighted_pred=0, weighted_bipred=0, init_qp=26, chroma_qp_off=0)
    pics = [dict(kind="I" | "P" | "B", poc=even int, layout="mb" | "row" | "pic", mbs=[...], and optionally
                 is_ref (default: kind != "B"), qp (slice QP, default init_qp), deblock=(disable_idc, alpha_div2, beta_div2) (default (1, 0, 0)),
                 num_ref=(n0, n1) (active entries, sent with num_ref_idx_active_override), wp=dict(ld_y, ld_c, l0=[entry..], l1=[entry..]) with
                 entry = None (both flags 0) or dict(y=(w, o) | None, c=((w, o), (w, o)) | None))]
    mbs[addr] is one of
        dict(t="pcm", y=(16,16) uint8, cb=(8,8), cr=(8,8))
        dict(t="i16", mode=0..3, cmode=0..3)                       Intra16x16 without coefficients
        dict(t="skip")                                             P_Skip
        dict(t="16x16", l0=(pic, (mvx, mvy)) | None, l1=(pic, (mvx, mvy)) | None)      pic = index into pics (decode order), vectors in quarter samples
        dict(t="16x8" | "8x16", parts=[(pic, mv), (pic, mv)])      P only
    and, for the streams on which the deblocking filter has to filter (tests/deblock_ref.py computes what it does):
        qp=.., deblock=(idc, a, b) on any macroblock of layout "mb": the macroblock is a slice, so slice_qp_delta and the three deblocking fields carry them
        dqp=.. on t="i16": mb_qp_delta, accumulated per 7.4.5 within the slice (``mb_qps``); layouts "row" / "pic"
        resid=(blkIdx, +1 | -1) on a P 16x16 / 16x8 / 8x16 macroblock of layout "mb": ONE coded coefficient, the DC of luma block blkIdx (6.4.3 order), level
        +-1 -- coded_block_pattern has the luma bit of that block's 8x8 and nothing else, mb_qp_delta is 0; the block's sixteen samples move by one constant
        (analytic_expect.dc_only_residual)
layout "mb": one slice per macroblock (no neighbour is available: every vector predictor is (0, 0), mvd = the vector); "row" / "pic": one slice per
macroblock row / per picture -- inter macroblocks of such a slice must be 16x16 with ONE vector and reference per list throughout the slice (the
predictor is then that vector as soon as a neighbour exists, whichever of 8.4.1.3's branches applies) and may not be P_Skip; intra macroblocks may sit
between them only in a picture one macroblock wide.  seq may carry frame_mbs_only=0 (frame pictures of a stream that could hold fields).
"""
import re

import numpy as np

from spec_tables_h264 import CBP_OF_CODENUM, COEFF_TOKEN, TOTAL_ZEROS_4x4, parse_code_table


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


def sps(seq):
    b = Bits()
    w, h = seq["width"], seq["height"]
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    prof = seq.get("profile", 66)
    b.u(8, prof)
    b.u(8, 0x80 if prof == 66 else 0x40)                            # constraint_set0 / set1, reserved zero bits
    b.u(8, 40)                                                      # level_idc
    b.ue(0)                                                         # seq_parameter_set_id
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
    b.u(1, 1)                                                       # direct_8x8_inference_flag
    cr, cb_ = mbw * 16 - w, mbh * 16 - h
    assert cr % 2 == 0 and cb_ % 2 == 0 and (fmo or cb_ == 0)
    if cr or cb_:
        b.u(1, 1)
        b.ue(0); b.ue(cr // 2); b.ue(0); b.ue(cb_ // 2)             # crop units: two luma samples (4:2:0 frames)
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
    b.u(1, 0)                                                       # constrained_intra_pred_flag
    b.u(1, 0)                                                       # redundant_pic_cnt_present_flag
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


def plan(seq, pics):
    """Per picture: frame_num, the lists cut to their active length, nal_ref_idc.  Sliding window marking (8.2.5.3)."""
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
    return {"mb": 1, "row": mbw, "pic": mbw * mbh}[p.get("layout", "mb" if p["kind"] != "I" else "pic")]


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


def slice_header(b, seq, p, pl, first_mb):
    kind = p["kind"]
    b.ue(first_mb)
    b.ue({"P": 0, "B": 1, "I": 2}[kind])
    b.ue(0)                                                         # pic_parameter_set_id
    b.u(LOG2_MAX_FRAME_NUM, pl["frame_num"])
    if not seq.get("frame_mbs_only", 1):
        b.u(1, 0)                                                   # field_pic_flag
    if pl["idr"]:
        b.ue(0)                                                     # idr_pic_id
    b.u(LOG2_MAX_POC_LSB, p["poc"] % (1 << LOG2_MAX_POC_LSB))
    if kind == "B":
        b.u(1, 1)                                                   # direct_spatial_mv_pred_flag
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


def write(seq, pics):
    """The Annex-B stream of the script."""
    mbw = (seq["width"] + 15) // 16
    mbh = (seq["height"] + 15) // 16
    n_mbs = mbw * mbh
    out = [sps(seq), pps(seq)]
    for k, (p, pl) in enumerate(zip(pics, plan(seq, pics))):
        kind, mbs = p["kind"], p["mbs"]
        assert len(mbs) == n_mbs
        step = layout_step(seq, p)
        mb_qps(seq, p)                                              # its assertions
        for first in range(0, n_mbs, step):
            b = Bits()
            qp, db = slice_fields(seq, p, step, mbs[first])
            slice_header(b, seq, dict(p, qp=qp, deblock=db), pl, first)
            skip_run = 0
            for a in range(first, min(first + step, n_mbs)):
                m = mbs[a]
                t = m["t"]
                if t == "skip":
                    assert kind == "P" and step == 1
                    skip_run += 1
                    continue
                if kind != "I":
                    b.ue(skip_run)
                    skip_run = 0
                intra_base = {"I": 0, "P": 5, "B": 23}[kind]
                if t == "pcm":
                    b.ue(intra_base + 25)
                    b.align_zero()                                  # pcm_alignment_zero_bit
                    b.raw(np.asarray(m["y"], np.uint8).tobytes() + np.asarray(m["cb"], np.uint8).tobytes() + np.asarray(m["cr"], np.uint8).tobytes())
                elif t == "i16":
                    b.ue(intra_base + 1 + m["mode"])                # I_16x16_<mode>_0_0
                    b.ue(m["cmode"])                                # intra_chroma_pred_mode
                    b.se(m.get("dqp", 0))                           # mb_qp_delta
                    # Intra16x16DCLevel, blkIdx 0: nC from the total_coeff of the blocks left of and above it (9.2.1): 16 in an I_PCM macroblock,
                    # 0 in every other macroblock a script can hold; a neighbour in another slice is not available
                    x, y = a % mbw, a // mbw
                    na = (16 if mbs[a - 1]["t"] == "pcm" else 0) if x > 0 and a - 1 >= first else None
                    nb = (16 if mbs[a - mbw]["t"] == "pcm" else 0) if y > 0 and a - mbw >= first else None
                    nc = (na + nb + 1) >> 1 if na is not None and nb is not None else (na if na is not None else (nb if nb is not None else 0))
                    coeff_token_zero(b, nc)
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
                                # every macroblock of this slice is the same 16x16 block: as soon as one neighbour exists, every available neighbour holds
                                # this vector and reference, and each branch of 8.4.1.3 (one neighbour, one matching reference, median) returns it
                                inter = [q_ for q_ in mbs[first:min(first + step, n_mbs)] if q_["t"] == "16x16"]
                                assert all(q_ == inter[0] for q_ in inter), "a slice of several macroblocks repeats one 16x16 inter macroblock"
                                if len(inter) == min(first + step, n_mbs) - first:
                                    mvp = (0, 0) if a == first else mv
                                else:
                                    # intra macroblocks in between, pictures ONE macroblock wide only: A, C and D lie outside the picture, B is the
                                    # macroblock above -- inter in this slice: the one neighbour whose reference matches, the predictor is its vector
                                    # (this vector); intra or in another slice: no reference matches, median(0, 0, 0)
                                    assert mbw == 1
                                    mvp = mv if a > first and mbs[a - 1]["t"] == "16x16" else (0, 0)
                            b.se(mv[0] - mvp[0]); b.se(mv[1] - mvp[1])
                    if "resid" in m:
                        assert kind == "P" and step == 1
                        one_dc_coefficient(b, *m["resid"])
                    else:
                        b.ue(0)                                     # coded_block_pattern 0 (Table 9-4, Inter, codeNum 0)
            if skip_run:
                b.ue(skip_run)
            b.trailing()
            out.append(nal(1 if pl["is_ref"] else 0, 5 if pl["idr"] else 1, b.bytes()))
    return b"".join(out)
