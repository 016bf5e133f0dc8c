"""A scripted H.265 stream writer (Main profile, 16x16 CTBs = 16x16 coding units, CABAC) for the analytic known-answer tests.

As tests/scripted_h264.py: the test says which coding unit carries which samples, vector, reference and weight; ``write`` turns the script into Annex-B
bytes; no residual is ever coded (rqt_root_cbf 0), so the decoded picture follows from the script by arithmetic (tests/analytic_expect_hevc.py).  Typed
from the syntax clauses (7.3.1.2, 7.3.2.1 - 7.3.2.3, 7.3.3, 7.3.6, 7.3.7, 7.3.8, 9.3) -- not from tools/hevcgen.c, the oracle or the product.

The CABAC encoder is 9.3.4 run backwards (the encoding flowcharts of 9.3.4.x / H.264 9.3.4.2: EncodeDecision, EncodeBypass, EncodeTerminate, EncodeFlush,
RenormE, PutBit).  Context initial values: the separately typed copy HEVC_INIT of tests/test_table_provenance.py; rangeTabLps: the separately typed copy
of tests/spec_tables_h264.py (the H.264 and H.265 engines share it); transIdxLps is read out of jmcodec_amd/csrc/hevc_tables.h -- an error there would
be shared by this encoder and the decoder and cancel, and entropy coding is not what these cases pin.

The script
    seq  = dict(width, height, weighted_pred=0, weighted_bipred=0, deblock=0 (1: filter on in the PPS), pcm_loop_filter_disabled=1, init_qp=26)
    pics = [dict(kind="I" | "P" | "B", poc, layout="ctb" | "row" | "pic", cus=[...], and optionally is_ref (default kind != "B"), qp,
                 deblock=None | 0 | 1 (slice override), wp=dict(ld_y, ld_c, l0=[entry..], l1=[entry..]) with entry = None or
                 dict(y=(weight, offset) | None, c=((weight, offset), (weight, offset)) | None) -- the FINAL weights and offsets of 7.4.7.3)]
    cus[ctb address] is one of
        dict(t="pcm", y=(16,16) uint8, cb=(8,8), cr=(8,8))
        dict(t="skip")                                             cu_skip_flag 1: with no candidate the zero vector on index 0 (both lists in B)
        dict(t="inter", l0=(pic, (mvx, mvy)) | None, l1=(pic, (mvx, mvy)) | None)      2Nx2N, merge_flag 0; quarter-sample vectors
Every picture decoded so far with is_ref stays in the reference picture set (at most 5).  RefPicList0 = pictures before the current one in output
order, nearest first, then those after it; RefPicList1 the other way round (8.3.4); both lists are active in full.
layout "ctb": one slice per CTB -- no spatial candidate exists, TMVP is off, both AMVP candidates are zero, mvd = the vector.  "row" / "pic": every CTB
of a slice repeats one inter unit: once a neighbour exists the first AMVP candidate is that vector (8.5.3.2.6 / 8.5.3.2.7), mvd is 0.
"""
import os
import re

import numpy as np

from scripted_h264 import Bits
from spec_tables_h264 import RANGE_TAB_LPS
from test_table_provenance import HEVC_INIT
from util import ROOT, c_array

TRANS_IDX_LPS = c_array(os.path.join(ROOT, "jmcodec_amd", "csrc", "hevc_tables.h"), "hevc_trans_lps")
LOG2_MAX_POC_LSB = 8
CTB = 16


class Cabac:
    """9.3.4.x: the arithmetic encoder, writing into a Bits."""

    def __init__(self, bits, init_type, qp):
        self.b = bits
        self.ctx = {}
        row = {2: 0, 1: 1, 0: 2}[init_type]                         # HEVC_INIT rows are [B, P, I] = initType 2, 1, 0
        for name, (_, rows) in HEVC_INIT.items():
            for i, v in enumerate(rows[row]):
                m, n = (v >> 4) * 5 - 45, ((v & 15) << 3) - 16      # 9.3.2.2
                pre = max(1, min(126, ((m * max(0, min(51, qp))) >> 4) + n))
                mps = 0 if pre <= 63 else 1
                self.ctx[(name, i)] = [pre - 64 if mps else 63 - pre, mps]
        self.start()

    def start(self):
        self.low, self.range, self.first, self.outstanding = 0, 510, True, 0

    def put(self, bit):
        if self.first:
            self.first = False
        else:
            self.b.u(1, bit)
        while self.outstanding:
            self.b.u(1, 1 - bit)
            self.outstanding -= 1

    def renorm(self):
        while self.range < 256:
            if self.low < 256:
                self.put(0)
            elif self.low >= 512:
                self.low -= 512
                self.put(1)
            else:
                self.low -= 256
                self.outstanding += 1
            self.range <<= 1
            self.low <<= 1

    def decision(self, name, inc, bin_):
        c = self.ctx[(name, inc)]
        lps = RANGE_TAB_LPS[c[0]][(self.range >> 6) & 3]
        self.range -= lps
        if bin_ != c[1]:
            self.low += self.range
            self.range = lps
            if c[0] == 0:
                c[1] = 1 - c[1]
            c[0] = TRANS_IDX_LPS[c[0]]
        else:
            c[0] = min(c[0] + 1, 62)
        self.renorm()

    def bypass(self, bin_):
        self.low <<= 1
        if bin_:
            self.low += self.range
        if self.low >= 1024:
            self.put(1)
            self.low -= 1024
        elif self.low < 512:
            self.put(0)
        else:
            self.low -= 512
            self.outstanding += 1

    def terminate(self, bin_):
        self.range -= 2
        if bin_:
            self.low += self.range
            self.range = 2                                          # EncodeFlush
            self.renorm()
            self.put((self.low >> 9) & 1)
            self.b.u(2, ((self.low >> 7) & 3) | 1)                  # the last bit is the stop bit / the bit in front of the alignment
        else:
            self.renorm()

    def egk(self, v, k):                                            # 9.3.3.5, bypass bins
        while v >= (1 << k):
            self.bypass(1)
            v -= 1 << k
            k += 1
        self.bypass(0)
        for i in range(k - 1, -1, -1):
            self.bypass((v >> i) & 1)


def nal(typ, rbsp):
    return b"\x00\x00\x00\x01" + bytes([typ << 1, 1]) + re.sub(b"\x00\x00(?=[\x00-\x03])", b"\x00\x00\x03", rbsp)


def profile_tier_level(b):
    b.u(2, 0); b.u(1, 0); b.u(5, 1)                                 # general_profile_space, tier, profile_idc: Main
    b.u(32, 0x60000000)                                             # compatibility flags: Main and Main 10
    b.u(1, 1); b.u(1, 0); b.u(1, 0); b.u(1, 1)                      # progressive, interlaced, non-packed, frame-only
    b.u(32, 0); b.u(12, 0)                                          # 43 reserved zero bits and general_inbld / reserved flag
    b.u(8, 120)                                                     # general_level_idc: 4


def vps():
    b = Bits()
    b.u(4, 0); b.u(1, 1); b.u(1, 1); b.u(6, 0); b.u(3, 0); b.u(1, 1); b.u(16, 0xFFFF)
    profile_tier_level(b)
    b.u(1, 1); b.ue(5); b.ue(2); b.ue(0)                            # ordering info: max_dec_pic_buffering_minus1, num_reorder, latency
    b.u(6, 0); b.ue(0); b.u(1, 0); b.u(1, 0)                        # max_layer_id, num_layer_sets_minus1, timing info, extension
    b.trailing()
    return nal(32, b.bytes())


def coded_size(seq):
    return (seq["width"] + CTB - 1) // CTB * CTB, (seq["height"] + CTB - 1) // CTB * CTB


def sps(seq):
    b = Bits()
    W, H = coded_size(seq)
    b.u(4, 0); b.u(3, 0); b.u(1, 1)
    profile_tier_level(b)
    b.ue(0); b.ue(1)                                                # sps id, chroma_format_idc 4:2:0
    b.ue(W); b.ue(H)
    cr, cb_ = W - seq["width"], H - seq["height"]
    assert cr % 2 == 0 and cb_ % 2 == 0
    b.u(1, 1 if cr or cb_ else 0)
    if cr or cb_:
        b.ue(0); b.ue(cr // 2); b.ue(0); b.ue(cb_ // 2)             # conformance window, units of two luma samples
    b.ue(0); b.ue(0)                                                # bit depths 8
    b.ue(LOG2_MAX_POC_LSB - 4)
    b.u(1, 1); b.ue(5); b.ue(2); b.ue(0)                            # sub-layer ordering info
    b.ue(1); b.ue(0)                                                # MinCbLog2SizeY 4, CtbLog2SizeY 4: a CTB is one coding unit, split_cu_flag is never coded
    b.ue(0); b.ue(2)                                                # transform blocks 4 .. 16
    b.ue(0); b.ue(0)                                                # max_transform_hierarchy_depth_inter / intra
    b.u(1, 0); b.u(1, 0); b.u(1, 0)                                 # scaling lists, AMP, SAO: off
    b.u(1, 1); b.u(4, 7); b.u(4, 7); b.ue(1); b.ue(0)               # PCM on: 8-bit samples, 16x16 only
    b.u(1, seq.get("pcm_loop_filter_disabled", 1))
    b.ue(0)                                                         # num_short_term_ref_pic_sets: every slice header carries its own
    b.u(1, 0); b.u(1, 0); b.u(1, 0)                                 # long-term pictures, TMVP, strong intra smoothing: off
    b.u(1, 0); b.u(1, 0)                                            # VUI, extension
    b.trailing()
    return nal(33, b.bytes())


def pps(seq):
    b = Bits()
    b.ue(0); b.ue(0)
    b.u(1, 0); b.u(1, 0); b.u(3, 0); b.u(1, 0); b.u(1, 0)           # dependent slices, output flag, extra bits, sign hiding, cabac_init_present
    b.ue(0); b.ue(0)                                                # num_ref_idx_default_active_minus1 (every P / B slice overrides)
    b.se(seq.get("init_qp", 26) - 26)
    b.u(1, 0); b.u(1, 0); b.u(1, 0)                                 # constrained intra, transform skip, cu_qp_delta
    b.se(0); b.se(0); b.u(1, 0)                                     # chroma QP offsets
    b.u(1, seq.get("weighted_pred", 0)); b.u(1, seq.get("weighted_bipred", 0))
    b.u(1, 0); b.u(1, 0); b.u(1, 0)                                 # transquant bypass, tiles, wavefronts
    b.u(1, 1)                                                       # pps_loop_filter_across_slices_enabled_flag
    b.u(1, 1); b.u(1, 1)                                            # deblocking_filter_control_present_flag, override enabled
    b.u(1, 0 if seq.get("deblock", 0) else 1)                       # pps_deblocking_filter_disabled_flag
    if seq.get("deblock", 0):
        b.se(0); b.se(0)
    b.u(1, 0); b.u(1, 0); b.ue(0); b.u(1, 0); b.u(1, 0)             # scaling lists, list modification, parallel merge level, header extension, extension
    b.trailing()
    return nal(34, b.bytes())


def plan(seq, pics):
    """Per picture: the reference picture set (pictures before / after in output order, nearest first), RefPicList0 / 1, the NAL type."""
    out, held = [], []
    for k, p in enumerate(pics):
        before = sorted((i for i in held if pics[i]["poc"] < p["poc"]), key=lambda i: -pics[i]["poc"])
        after = sorted((i for i in held if pics[i]["poc"] > p["poc"]), key=lambda i: pics[i]["poc"])
        is_ref = p.get("is_ref", p["kind"] != "B")
        out.append(dict(before=before, after=after, l0=before + after, l1=after + before, is_ref=is_ref, typ=19 if k == 0 else (1 if is_ref else 0)))
        if k == 0:
            held = []
        if is_ref:
            held.append(k)
            assert len(held) <= 5
    return out


def slice_header(b, seq, p, pl, first, addr, n_ctbs):
    kind = p["kind"]
    b.u(1, 1 if first else 0)
    if pl["typ"] >= 16:
        b.u(1, 0)                                                   # no_output_of_prior_pics_flag
    b.ue(0)                                                         # slice_pic_parameter_set_id
    if not first:
        b.u(max(1, (n_ctbs - 1).bit_length()), addr)                # Ceil(Log2(PicSizeInCtbsY)) bits
    b.ue({"B": 0, "P": 1, "I": 2}[kind])
    if pl["typ"] != 19:
        b.u(LOG2_MAX_POC_LSB, p["poc"] % (1 << LOG2_MAX_POC_LSB))
        b.u(1, 0)                                                   # short_term_ref_pic_set_sps_flag
        b.ue(len(pl["before"])); b.ue(len(pl["after"]))             # st_ref_pic_set(0): no inter-set prediction for index 0
        prev = p["poc"]
        for i in pl["before"]:
            b.ue(prev - pl["pocs"][i] - 1); b.u(1, 1)
            prev = pl["pocs"][i]
        prev = p["poc"]
        for i in pl["after"]:
            b.ue(pl["pocs"][i] - prev - 1); b.u(1, 1)
            prev = pl["pocs"][i]
    if kind != "I":
        b.u(1, 1)                                                   # num_ref_idx_active_override_flag
        b.ue(len(pl["l0"]) - 1)
        if kind == "B":
            b.ue(len(pl["l1"]) - 1)
            b.u(1, 0)                                               # mvd_l1_zero_flag
        if (kind == "P" and seq.get("weighted_pred", 0)) or (kind == "B" and seq.get("weighted_bipred", 0)):
            wp = p.get("wp", dict(ld_y=0, ld_c=0))
            b.ue(wp["ld_y"]); b.se(wp["ld_c"] - wp["ld_y"])
            for l in ("l0", "l1")[:2 if kind == "B" else 1]:
                n = len(pl[l])
                ent = [(wp.get(l, []) + [None] * n)[i] or {} for i in range(n)]
                for e in ent:
                    b.u(1, 0 if e.get("y") is None else 1)
                for e in ent:
                    b.u(1, 0 if e.get("c") is None else 1)
                for e in ent:
                    if e.get("y") is not None:
                        b.se(e["y"][0] - (1 << wp["ld_y"])); b.se(e["y"][1])
                    if e.get("c") is not None:
                        for (w_, o_) in e["c"]:
                            # 7-56: ChromaOffset = Clip3(-128, 127, 128 + delta - ((128 * ChromaWeight) >> ChromaLog2WeightDenom)): delta for the offset
                            b.se(w_ - (1 << wp["ld_c"])); b.se(o_ - 128 + ((128 * w_) >> wp["ld_c"]))
        b.ue(4)                                                     # five_minus_max_num_merge_cand: one candidate, merge_idx is never coded
    b.se(p.get("qp", seq.get("init_qp", 26)) - seq.get("init_qp", 26))
    ov = p.get("deblock")
    b.u(1, 0 if ov is None else 1)                                  # deblocking_filter_override_flag
    disabled = not seq.get("deblock", 0)
    if ov is not None:
        disabled = not ov
        b.u(1, 1 if disabled else 0)
        if not disabled:
            b.se(0); b.se(0)
    if not disabled:
        b.u(1, 1)                                                   # slice_loop_filter_across_slices_enabled_flag
    b.u(1, 1)                                                       # byte_alignment()
    b.align_zero()


def write(seq, pics):
    W, H = coded_size(seq)
    cw, ch = W // CTB, H // CTB
    n_ctbs = cw * ch
    out = [vps(), sps(seq), pps(seq)]
    plans = plan(seq, pics)
    pocs = [p["poc"] for p in pics]
    for k, (p, pl) in enumerate(zip(pics, plans)):
        pl["pocs"] = pocs
        kind, cus = p["kind"], p["cus"]
        assert len(cus) == n_ctbs
        step = {"ctb": 1, "row": cw, "pic": n_ctbs}[p.get("layout", "ctb" if kind != "I" else "pic")]
        for first in range(0, n_ctbs, step):
            b = Bits()
            slice_header(b, seq, p, pl, first == 0, first, n_ctbs)
            c = Cabac(b, {"I": 0, "P": 1, "B": 2}[kind], p.get("qp", seq.get("init_qp", 26)))
            last = min(first + step, n_ctbs) - 1
            for a in range(first, last + 1):
                u = cus[a]
                t = u["t"]
                x, y = a % cw, a // cw
                if kind != "I":
                    # 9.3.4.2.2: ctxInc = the skip flags of the left and upper units where those are available (same slice, decoded)
                    inc = (1 if x > 0 and a - 1 >= first and cus[a - 1]["t"] == "skip" else 0) + (1 if y > 0 and a - cw >= first and cus[a - cw]["t"] == "skip" else 0)
                    c.decision("cu_skip_flag", inc, 1 if t == "skip" else 0)
                if t == "pcm":
                    if kind != "I":
                        c.decision("pred_mode_flag", 0, 1)          # MODE_INTRA
                    c.decision("part_mode", 0, 1)                   # log2CbSize == MinCbLog2SizeY: part_mode is coded for intra units too; PART_2Nx2N
                    c.terminate(1)                                  # pcm_flag; the flush leaves the writer one bit in front of pcm_alignment_zero_bit
                    b.align_zero()
                    b.raw(np.asarray(u["y"], np.uint8).tobytes() + np.asarray(u["cb"], np.uint8).tobytes() + np.asarray(u["cr"], np.uint8).tobytes())
                    c.start()                                       # 9.3.2.5: the engine is initialised again behind the samples (contexts keep their state)
                elif t == "inter":
                    assert kind != "I" and (step == 1 or u == cus[first]), "a slice of several CTBs repeats one inter unit"
                    c.decision("pred_mode_flag", 0, 0)
                    c.decision("part_mode", 0, 1)
                    c.decision("merge_flag", 0, 0)
                    l0, l1 = u.get("l0"), u.get("l1")
                    if kind == "B":
                        c.decision("inter_pred_idc", 0, 1 if l0 and l1 else 0)          # nPbW + nPbH != 12: first bin with ctxInc = CtDepth = 0
                        if not (l0 and l1):
                            c.decision("inter_pred_idc", 4, 1 if l1 else 0)
                    else:
                        assert l0 and not l1
                    for name, q in (("l0", l0), ("l1", l1)):
                        if not q:
                            continue
                        n, idx = len(pl[name]), pl[name].index(q[0])
                        if n > 1:                                   # ref_idx_lX: truncated unary, cMax = n - 1; bins 0 and 1 with contexts, the rest bypass
                            for i in range(min(idx + 1, n - 1)):
                                bin_ = 1 if i < idx else 0
                                c.decision("ref_idx", i, bin_) if i < 2 else c.bypass(bin_)
                        mvd = q[1] if a == first else (0, 0)        # both AMVP candidates zero / the first candidate is this vector (module docstring)
                        g0 = [1 if v else 0 for v in mvd]
                        g1 = [1 if abs(v) > 1 else 0 for v in mvd]
                        c.decision("abs_mvd_greater0", 0, g0[0]); c.decision("abs_mvd_greater0", 0, g0[1])
                        if g0[0]:
                            c.decision("abs_mvd_greater1", 0, g1[0])
                        if g0[1]:
                            c.decision("abs_mvd_greater1", 0, g1[1])
                        for i in (0, 1):
                            if g0[i]:
                                if g1[i]:
                                    c.egk(abs(mvd[i]) - 2, 1)       # abs_mvd_minus2: EG1
                                c.bypass(1 if mvd[i] < 0 else 0)    # mvd_sign_flag
                        c.decision("mvp_flag", 0, 0)
                    c.decision("rqt_root_cbf", 0, 0)
                else:
                    assert t == "skip" and kind != "I" and step == 1        # (MaxNumMergeCand 1: no merge_idx)
                c.terminate(1 if a == last else 0)                  # end_of_slice_segment_flag; the flush's last bit is rbsp_slice_segment_trailing_bits' 1
            b.align_zero()
            out.append(nal(pl["typ"], b.bytes()))
    return b"".join(out)
