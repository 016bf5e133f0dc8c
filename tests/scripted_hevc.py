"""A scripted H.265 stream writer (Main profile, CABAC; by default 16x16 CTBs = 16x16 coding units) for the analytic known-answer tests.

As tests/scripted_h264.py: the test says which coding unit carries which samples, vector, reference, weight or intra mode; ``write`` turns the script
into Annex-B bytes; residuals are scripted level by level (``coef``; ``dc`` is the earlier short form for one coefficient at (0, 0)), so the decoded
picture follows from the script by arithmetic (tests/analytic_hevc.py, tests/hevc_intra_ref.py, tests/hevc_resid_ref.py).  Typed from the syntax
clauses (7.3.1.2, 7.3.2.1 - 7.3.2.3, 7.3.3, 7.3.4, 7.3.6, 7.3.7, 7.3.8.3 - 7.3.8.11, 9.3, the context selection of 9.3.4.2, the binarisations of
9.3.3.10 / 9.3.3.11, the part_mode binarisation of 9.3.3.7) -- not from tools/hevcgen.c, the oracle or the product.

The CABAC encoder is 9.3.4 run backwards (the encoding flowcharts of 9.3.4.x / H.264 9.3.4.2: EncodeDecision, EncodeBypass, EncodeTerminate, EncodeFlush,
RenormE, PutBit).  Context initial values: the separately typed copy HEVC_INIT of tests/test_table_provenance.py; rangeTabLps: the separately typed copy
of tests/spec_tables_h264.py (the H.264 and H.265 engines share it); transIdxLps is read out of jmcodec_amd/csrc/hevc_tables.h -- an error there would
be shared by this encoder and the decoder and cancel, and entropy coding is not what these cases pin.

The script
    seq  = dict(width, height, weighted_pred=0, weighted_bipred=0, deblock=0 (1: filter on in the PPS), pcm_loop_filter_disabled=1, init_qp=26,
                ctb_log2=4 (4, 5, 6), min_cb_log2=ctb_log2 (3 ..), max_tb_log2=4 (.. 5), tu_depth_intra=0 (max_transform_hierarchy_depth_intra),
                pcm_log2=(4, 4) (smallest and largest PCM unit), strong_intra=0, constrained_intra=0,
                tu_depth_inter=0 (max_transform_hierarchy_depth_inter), transform_skip=0, transquant_bypass=0, sign_hiding=0,
                cu_qp_delta=0 with diff_cu_qp_delta_depth=0, cb_qp_offset=0, cr_qp_offset=0 (PPS), slice_chroma_qp_offsets=0 (1: every picture's
                cb_qp_offset / cr_qp_offset go into its slice headers),
                scaling_lists=None | dict(sps=None | spec, pps=None | spec): scaling_list_enabled_flag 1; sps None = the default lists, a spec is
                what ``scaling_list_data`` takes; PPS lists replace the SPS ones)
           the coded size is width x height rounded up to the minimum coding block size: a picture may end inside a CTB
    pics = [dict(kind="I" | "P" | "B", poc, layout="ctb" | "row" | "pic", cus=[...], and optionally is_ref (default kind != "B"), qp,
                 deblock=None | 0 | 1 (slice override), wp=dict(ld_y, ld_c, l0=[entry..], l1=[entry..]) with entry = None or
                 dict(y=(weight, offset) | None, c=((weight, offset), (weight, offset)) | None) -- the FINAL weights and offsets of 7.4.7.3)]
    cus[ctb address] is a tree:
        dict(t="split", sub=[four trees in z order])               a block that crosses the picture edge MUST be a split (the flag is inferred); entries of
                                                                   sub that lie outside the picture are ignored (None will do)
      or a leaf, one of
        dict(t="pcm", y=(n,n) uint8, cb=(n/2,n/2), cr=(n/2,n/2))   n = the leaf's size, inside pcm_log2
        dict(t="skip")                                             cu_skip_flag 1: MaxNumMergeCand is 1 and every candidate is the zero vector on index 0
                                                                   (both lists in B) -- with one slice per CTB, or anywhere in a picture whose inter
                                                                   units are ALL skipped (a neighbour's vector is then that vector too)
        dict(t="inter", l0=(pic, (mvx, mvy)) | None, l1=(pic, (mvx, mvy)) | None)      2Nx2N, merge_flag 0; quarter-sample vectors; a whole 16x16 CTB
        dict(t="intra", modes=[m] | [m0, m1, m2, m3], chroma=0..4, tu=depth, dc=[(level_y, level_cb, level_cr) | None per transform unit])
                                                                   four modes: PART_NxN, only at the minimum coding block size; chroma is the VALUE of
                                                                   intra_chroma_pred_mode; tu the uniform depth of the transform tree (NxN: >= 1; where
                                                                   7.4.9.8 infers split_transform_flag the script must say what is inferred); dc in
                                                                   decoding order, a level 0 = cbf 0; with 4x4 luma blocks the chroma levels of four
                                                                   blocks are those of the fourth entry (7.3.8.10: blkIdx 3)
      intra and inter units (inter units of 16x16 and 32x32 CTBs) may carry, in place of dc,
        tu=depth, coef=[None | {0: {(x, y): level}, 1: {..}, 2: {..}, "tskip": {components with transform_skip_flag}} per transform unit]
                                                                   every level as scripted: with sign_hiding the writer asserts the parity that the
                                                                   hidden sign needs, it does not repair it; an inter unit with any level has
                                                                   rqt_root_cbf 1 and a transform tree of uniform depth tu
        bypass=1 (cu_transquant_bypass_flag), dqp=CuQpDeltaVal     dqp is coded with the unit's first transform unit that has a cbf, once per
                                                                   quantisation group: a unit that cannot carry its dqp is refused
Inter prediction as SYNTAX (tests/hevc_inter_ref.py derives the motion; the writer derives none), all with defaults that leave the forms above as they were:
    seq:  amp=0 (amp_enabled_flag), tmvp=0 (sps_temporal_mvp_enabled_flag), par_mrg_log2=2 (Log2ParMrgLevel, 2 .. CtbLog2SizeY)
    pics: max_merge=1 (MaxNumMergeCand, 1 .. 5), tmvp=the sequence's (slice_temporal_mvp_enabled_flag), col=(collocated_from_l0_flag, collocated_ref_idx)
          = (1, 0), mvd_l1_zero=0, n_ref=(entries of list 0, of list 1) that the slice header activates (default: as many as pictures are held; more
          repeat the pictures in turn, 8-8 / 8-10), slice_n_ref=[n_ref per slice, decoding order]: the slices of one picture with lists of their own
    leaves:
        dict(t="skip", merge=idx)                                  cu_skip_flag 1 and merge_idx
        dict(t="inter", part="2Nx2N" | "2NxN" | "Nx2N" | "NxN" | "2NxnU" | "2NxnD" | "nLx2N" | "nRx2N", pus=[one per prediction block, partIdx order])
                                                                   part_mode as 9.3.3.7 has it (NxN only at a minimum size above 8, AMP only above the
                                                                   minimum size with amp=1); any size the quadtree gives, any slice layout
            a prediction unit is dict(merge=idx)                   merge_flag 1, merge_idx (first bin with a context, the others bypass, cMax max_merge - 1)
                           or dict(l0=(ref_idx, (mvdx, mvdy), mvp_flag) | None, l1=...)
                                                                   merge_flag 0, inter_pred_idc (8x4 / 4x8: one bin, never both lists), ref_idx_lX, mvd_coding,
                                                                   mvp_lX_flag; with mvd_l1_zero the list 1 difference of a two-list unit is not coded
        coef / tu / dqp / bypass stay valid on such a unit: rqt_root_cbf is absent (and 1) only for a 2Nx2N merge unit; with tu_depth_inter 0 a unit
        that is not 2Nx2N has its transform tree split once without a flag (interSplitFlag), so tu is 1
The loop filters as SYNTAX (tests/hevc_loop_ref.py filters; the writer filters nothing), all with defaults that leave every earlier stream as it was:
    seq:  sao=0 (sample_adaptive_offset_enabled_flag), pps_beta=0, pps_tc=0 (pps_beta_offset_div2, pps_tc_offset_div2: written with deblock=1),
          pps_across=1 (pps_loop_filter_across_slices_enabled_flag)
    pics: slices=[dict(first=CTB address, ...)]: slices that begin where the script says (in place of layout); each entry may carry its own values of
          the keys below, which otherwise are the picture's:
          deblock=None | 0 | 1 (the override, as before), beta=0, tc=0 (slice_beta_offset_div2 / slice_tc_offset_div2: only under the override with
          deblock=1; without the override the slice has the PPS offsets), across=pps_across (slice_loop_filter_across_slices_enabled_flag: the
          script must say what is inferred where 7.3.6.1 leaves the flag out), sao=(slice_sao_luma_flag, slice_sao_chroma_flag)=(0, 0)
          sao_ctbs=[per CTB address dict(merge="left" | "up" | None, y=entry, c=(entry of Cb, entry of Cr)) or None (everything off)]
            an entry is None (SaoTypeIdx 0), ("band", sao_band_position, four signed offsets) or ("edge", SaoEoClass, four magnitudes); Cr has Cb's
            type and class; a merged CTB says nothing else; a merge from outside the slice or the picture is refused; the entries of a component
            whose slice flag is 0 must be None
``slice_table`` gives the slices of a picture with every such value resolved.
Every picture decoded so far with is_ref stays in the reference picture set (at most 5).  RefPicList0 = pictures before the current one in output
order, nearest first, then those after it; RefPicList1 the other way round (8.3.4); both lists are active in full unless n_ref says otherwise.
The script must keep sps_max_num_reorder_pics = 2: at most two pictures precede a picture in decoding order and follow it in output order.
layout "ctb": one slice per CTB -- no spatial candidate exists, TMVP is off, both AMVP candidates are zero, mvd = the vector.  "row" / "pic": every CTB
of a slice repeats one inter unit: once a neighbour exists the first AMVP candidate is that vector (8.5.3.2.6 / 8.5.3.2.7), mvd is 0.
Context increments follow maps kept per 8x8 block (CtDepth, cu_skip_flag, CuPredMode) and availability as 6.4.1 has it (``_Picture.avail``); the
three candidates of 8.4.2 come from the writer's own map of intra modes (``mpm_candidates``).
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


def geometry(seq):
    """The block sizes of the sequence (7.4.3.2.1), defaults = one 16x16 coding unit per CTB, transform blocks 4 .. 16, PCM at 16x16 only."""
    ctb = seq.get("ctb_log2", 4)
    g = dict(ctb=ctb, min_cb=seq.get("min_cb_log2", ctb), max_tb=seq.get("max_tb_log2", 4), tu_depth=seq.get("tu_depth_intra", 0),
             tu_depth_inter=seq.get("tu_depth_inter", 0), pcm=tuple(seq.get("pcm_log2", (4, 4))))
    assert ctb in (4, 5, 6) and 3 <= g["min_cb"] <= ctb and 2 < g["max_tb"] <= min(ctb, 5) and 0 <= g["tu_depth"] <= ctb - 2
    assert 3 <= g["pcm"][0] <= g["pcm"][1] <= min(ctb, 5) and g["pcm"][0] >= min(g["min_cb"], 5)
    return g


def coded_size(seq):
    m = 1 << geometry(seq)["min_cb"]                                # pic_width / height_in_luma_samples: multiples of MinCbSizeY (7.4.3.2.1)
    return (seq["width"] + m - 1) // m * m, (seq["height"] + m - 1) // m * m


def ctb_dims(seq):
    W, H = coded_size(seq)
    s = 1 << geometry(seq)["ctb"]
    return (W + s - 1) // s, (H + s - 1) // s


def zscan(x, y, ctb_log2, cw):
    """6.5.2 without tiles: the z-scan order address of the 4x4 block that holds (x, y) -- CTBs in raster order, bits of x and y interleaved inside"""
    z = 0
    for i in range(ctb_log2 - 2):
        z |= (((x >> (2 + i)) & 1) << (2 * i)) | (((y >> (2 + i)) & 1) << (2 * i + 1))
    return (((y >> ctb_log2) * cw + (x >> ctb_log2)) << (2 * (ctb_log2 - 2))) | z


def walk(seq, p):
    """The leaves of a picture's script in decoding order: (x, y, log2CbSize, CtDepth, unit).  A block that crosses the picture edge is split without
    a flag (7.3.8.4); children outside the picture do not exist (their script entry is ignored, None will do)."""
    W, H = coded_size(seq)
    g = geometry(seq)
    cw, ch = ctb_dims(seq)

    def tree(x, y, log2, depth, node):
        if node["t"] == "split":
            assert log2 > g["min_cb"]
            for i, sub in enumerate(node["sub"]):
                x1, y1 = x + ((i & 1) << (log2 - 1)), y + ((i >> 1) << (log2 - 1))
                if x1 < W and y1 < H:
                    yield from tree(x1, y1, log2 - 1, depth + 1, sub)
        else:
            assert x + (1 << log2) <= W and y + (1 << log2) <= H, "a leaf crosses the picture edge"
            yield x, y, log2, depth, node
    assert len(p["cus"]) == cw * ch
    for a, node in enumerate(p["cus"]):
        yield from tree((a % cw) << g["ctb"], (a // cw) << g["ctb"], g["ctb"], 0, node)


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
    g = geometry(seq)
    b.ue(g["min_cb"] - 3); b.ue(g["ctb"] - g["min_cb"])             # MinCbLog2SizeY, CtbLog2SizeY (default 4, 4: a CTB is one coding unit, no split_cu_flag)
    b.ue(0); b.ue(g["max_tb"] - 2)                                  # transform blocks 4 .. 16 (32)
    b.ue(g["tu_depth_inter"]); b.ue(g["tu_depth"])                  # max_transform_hierarchy_depth_inter / intra
    sl = seq.get("scaling_lists")
    b.u(1, 1 if sl is not None else 0)                              # scaling_list_enabled_flag
    if sl is not None:
        b.u(1, 1 if sl.get("sps") is not None else 0)               # sps_scaling_list_data_present_flag (0: the default lists of Tables 7-5 / 7-6)
        if sl.get("sps") is not None:
            scaling_list_data(b, sl["sps"])
    b.u(1, seq.get("amp", 0)); b.u(1, seq.get("sao", 0))            # amp_enabled_flag; sample_adaptive_offset_enabled_flag
    b.u(1, 1); b.u(4, 7); b.u(4, 7); b.ue(g["pcm"][0] - 3); b.ue(g["pcm"][1] - g["pcm"][0])          # PCM on: 8-bit samples (default 16x16 only)
    b.u(1, seq.get("pcm_loop_filter_disabled", 1))
    b.ue(0)                                                         # num_short_term_ref_pic_sets: every slice header carries its own
    b.u(1, 0); b.u(1, seq.get("tmvp", 0)); b.u(1, seq.get("strong_intra", 0))      # long-term pictures: off; sps_temporal_mvp_enabled_flag; strong_intra_smoothing_enabled_flag
    b.u(1, 0); b.u(1, 0)                                            # VUI, extension
    b.trailing()
    return nal(33, b.bytes())


def pps(seq):
    b = Bits()
    b.ue(0); b.ue(0)
    b.u(1, 0); b.u(1, 0); b.u(3, 0); b.u(1, seq.get("sign_hiding", 0)); b.u(1, 0)     # dependent slices, output flag, extra bits, sign hiding, cabac_init_present
    b.ue(0); b.ue(0)                                                # num_ref_idx_default_active_minus1 (every P / B slice overrides)
    b.se(seq.get("init_qp", 26) - 26)
    b.u(1, seq.get("constrained_intra", 0)); b.u(1, seq.get("transform_skip", 0))      # constrained_intra_pred_flag, transform_skip_enabled_flag
    b.u(1, seq.get("cu_qp_delta", 0))                               # cu_qp_delta_enabled_flag
    if seq.get("cu_qp_delta", 0):
        assert 0 <= seq.get("diff_cu_qp_delta_depth", 0) <= geometry(seq)["ctb"] - geometry(seq)["min_cb"]
        b.ue(seq.get("diff_cu_qp_delta_depth", 0))
    b.se(seq.get("cb_qp_offset", 0)); b.se(seq.get("cr_qp_offset", 0))
    b.u(1, seq.get("slice_chroma_qp_offsets", 0))                   # pps_slice_chroma_qp_offsets_present_flag
    b.u(1, seq.get("weighted_pred", 0)); b.u(1, seq.get("weighted_bipred", 0))
    b.u(1, seq.get("transquant_bypass", 0)); b.u(1, 0); b.u(1, 0)   # transquant_bypass_enabled_flag; tiles, wavefronts: off
    b.u(1, seq.get("pps_across", 1))                                # pps_loop_filter_across_slices_enabled_flag
    b.u(1, 1); b.u(1, 1)                                            # deblocking_filter_control_present_flag, override enabled
    b.u(1, 0 if seq.get("deblock", 0) else 1)                       # pps_deblocking_filter_disabled_flag
    if seq.get("deblock", 0):
        assert -6 <= seq.get("pps_beta", 0) <= 6 and -6 <= seq.get("pps_tc", 0) <= 6
        b.se(seq.get("pps_beta", 0)); b.se(seq.get("pps_tc", 0))    # pps_beta_offset_div2, pps_tc_offset_div2
    else:
        assert not seq.get("pps_beta", 0) and not seq.get("pps_tc", 0), "the PPS offsets are written only with the filter on in the PPS"
    pl = (seq.get("scaling_lists") or {}).get("pps")
    b.u(1, 1 if pl is not None else 0)                              # pps_scaling_list_data_present_flag
    if pl is not None:
        scaling_list_data(b, pl)
    assert 2 <= seq.get("par_mrg_log2", 2) <= geometry(seq)["ctb"]
    b.u(1, 0); b.ue(seq.get("par_mrg_log2", 2) - 2); b.u(1, 0); b.u(1, 0)         # list modification, log2_parallel_merge_level_minus2, header extension, extension
    b.trailing()
    return nal(34, b.bytes())


def plan(seq, pics):
    """Per picture: the reference picture set (pictures before / after in output order, nearest first), RefPicList0 / 1, the NAL type."""
    out, held = [], []
    for k, p in enumerate(pics):
        before = sorted((i for i in held if pics[i]["poc"] < p["poc"]), key=lambda i: -pics[i]["poc"])
        after = sorted((i for i in held if pics[i]["poc"] > p["poc"]), key=lambda i: pics[i]["poc"])
        is_ref = p.get("is_ref", p["kind"] != "B")
        n0, n1 = p.get("n_ref") or (len(held), len(held))          # num_ref_idx_l0 / l1_active_minus1 + 1: the lists' first entries
        assert k == 0 or p["kind"] == "I" or (1 <= n0 <= 15 and 1 <= n1 <= 15 and held), (k, n0, n1, held)
        cyc = lambda lst, n: [lst[i % len(lst)] for i in range(n)] if lst else []       # 8-8 / 8-10: more active entries than pictures repeat them in turn
        out.append(dict(before=before, after=after, l0=cyc(before + after, n0), l1=cyc(after + before, n1), is_ref=is_ref,
                        typ=19 if k == 0 else (1 if is_ref else 0)))
        if k == 0:
            held = []
        if is_ref:
            held.append(k)
            assert len(held) <= 5
    return out


def slice_plan(pl, p, ordinal):
    """The plan of a picture as slice number `ordinal` (decoding order) sees it: with slice_n_ref the slice activates its own number of entries"""
    if p.get("slice_n_ref") is None:
        return pl
    n0, n1 = p["slice_n_ref"][ordinal]
    assert 1 <= n0 <= 15 and 1 <= n1 <= 15 and p.get("wp") is None
    cyc = lambda lst, n: [lst[i % len(lst)] for i in range(n)]
    return dict(pl, l0=cyc(pl["before"] + pl["after"], n0), l1=cyc(pl["after"] + pl["before"], n1))


def slice_table(seq, p):
    """The slices of a picture in decoding order, every value resolved: [dict(first, count, disabled (slice_deblocking_filter_disabled_flag),
    override (deblocking_filter_override_flag), beta, tc (the offsets in effect, div2), across, across_coded, sao=(luma, chroma))]"""
    cw, ch = ctb_dims(seq)
    n = cw * ch
    if p.get("slices") is not None:
        own = p["slices"]
        firsts = [o["first"] for o in own]
        assert firsts[0] == 0 and all(a < b_ for a, b_ in zip(firsts, firsts[1:])) and firsts[-1] < n and "layout" not in p, firsts
    else:
        step = {"ctb": 1, "row": cw, "pic": n}[p.get("layout", "ctb" if p["kind"] != "I" else "pic")]
        firsts = list(range(0, n, step))
        own = [{}] * len(firsts)
    out = []
    for i, (f, o) in enumerate(zip(firsts, own)):
        get = lambda key, d: o.get(key, p.get(key, d))
        ov = get("deblock", None)
        disabled = (not seq.get("deblock", 0)) if ov is None else (not ov)
        beta, tc = get("beta", None), get("tc", None)
        if ov is None or disabled:
            assert beta is None and tc is None, "slice offsets are coded only under the override, with the filter on"
            beta, tc = (seq.get("pps_beta", 0), seq.get("pps_tc", 0)) if ov is None else (0, 0)
        beta, tc = beta or 0, tc or 0
        assert -6 <= beta <= 6 and -6 <= tc <= 6
        sao = tuple(get("sao", (0, 0)))
        assert seq.get("sao", 0) or sao == (0, 0), "slice_sao_*_flag without sample_adaptive_offset_enabled_flag"
        pa = seq.get("pps_across", 1)
        coded = bool(pa and (sao[0] or sao[1] or not disabled))     # 7.3.6.1
        across = get("across", pa)
        assert coded or across == pa, "slice_loop_filter_across_slices_enabled_flag is absent and inferred to be the PPS flag"
        out.append(dict(first=f, count=(firsts[i + 1] if i + 1 < len(firsts) else n) - f, disabled=bool(disabled), override=ov is not None,
                        beta=beta, tc=tc, across=across, across_coded=coded, sao=sao))
    return out


def slice_map(seq, p):
    """SliceAddrRs per CTB address"""
    m = np.zeros(ctb_dims(seq)[0] * ctb_dims(seq)[1], np.int32)
    for sl in slice_table(seq, p):
        m[sl["first"]:sl["first"] + sl["count"]] = sl["first"]
    return m


def slice_header(b, seq, p, pl, first, addr, n_ctbs, sw={}, sl=None, stats=None):
    kind = p["kind"]
    sl = sl or [q for q in slice_table(seq, p) if q["first"] == addr][0]
    tmvp = 0
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
        if seq.get("tmvp", 0):
            tmvp = p.get("tmvp", 1)
            b.u(1, tmvp)                                            # slice_temporal_mvp_enabled_flag
    if seq.get("sao", 0):
        b.u(1, sl["sao"][0]); b.u(1, sl["sao"][1])                  # slice_sao_luma_flag, slice_sao_chroma_flag
    if kind != "I":
        b.u(1, 1)                                                   # num_ref_idx_active_override_flag
        b.ue(len(pl["l0"]) - 1)
        if kind == "B":
            b.ue(len(pl["l1"]) - 1)
            b.u(1, p.get("mvd_l1_zero", 0))                         # mvd_l1_zero_flag
        if tmvp and kind != "I":
            from_l0, idx = p.get("col", (1, 0))
            assert (from_l0 == 1 or kind == "B") and 0 <= idx < len(pl["l0" if from_l0 else "l1"])
            if kind == "B":
                b.u(1, from_l0)                                     # collocated_from_l0_flag
            if len(pl["l0" if from_l0 else "l1"]) > 1 or sw.get("col_ref_idx_always"):
                b.ue(idx)                                           # collocated_ref_idx
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
        assert 1 <= p.get("max_merge", 1) <= 5
        b.ue(5 - p.get("max_merge", 1))                             # five_minus_max_num_merge_cand (default: one candidate, merge_idx is never coded)
    b.se(p.get("qp", seq.get("init_qp", 26)) - seq.get("init_qp", 26))
    if seq.get("slice_chroma_qp_offsets", 0):
        b.se(p.get("cb_qp_offset", 0)); b.se(p.get("cr_qp_offset", 0))
    b.u(1, 1 if sl["override"] else 0)                              # deblocking_filter_override_flag
    if sl["override"]:
        b.u(1, 1 if sl["disabled"] else 0)                          # slice_deblocking_filter_disabled_flag
        if not sl["disabled"]:
            b.se(sl["beta"]); b.se(sl["tc"])                        # slice_beta_offset_div2, slice_tc_offset_div2
    present = (seq.get("pps_across", 1) and not sl["disabled"]) if sw.get("across_tied_to_deblock") else sl["across_coded"]
    if present:
        b.u(1, sl["across"])                                        # slice_loop_filter_across_slices_enabled_flag
    if stats is not None:
        for key in (("slice", "override", sl["override"], sl["disabled"]), ("slice", "across", sl["across"], "coded" if present else "inferred"),
                    ("slice", "sao", sl["sao"]), ("slice", "offsets", sl["beta"], sl["tc"])):
            stats[key] = stats.get(key, 0) + 1
    b.u(1, 1)                                                       # byte_alignment()
    b.align_zero()


def partitions(part, x, y, n):
    """7.3.8.5: the prediction blocks (x, y, width, height) of a coding unit in partIdx order"""
    h, q = n // 2, n // 4
    return {"2Nx2N": [(x, y, n, n)], "2NxN": [(x, y, n, h), (x, y + h, n, h)], "Nx2N": [(x, y, h, n), (x + h, y, h, n)],
            "NxN": [(x, y, h, h), (x + h, y, h, h), (x, y + h, h, h), (x + h, y + h, h, h)],
            "2NxnU": [(x, y, n, q), (x, y + q, n, n - q)], "2NxnD": [(x, y, n, n - q), (x, y + n - q, n, q)],
            "nLx2N": [(x, y, q, n), (x + q, y, n - q, n)], "nRx2N": [(x, y, n - q, n), (x + n - q, y, q, n)]}[part]


def tu_leaves(log2cb, nxn, tu):
    """Number of transform units of an intra unit whose transform tree has uniform depth tu (NxN: tu >= 1)"""
    assert tu >= (1 if nxn else 0) and log2cb - tu >= 2
    return 4 ** tu


def scan_order(idx, blk):
    """6.5.3 - 6.5.5: the (x, y) of a blk x blk array in up-right diagonal (0), horizontal (1) or vertical (2) order"""
    if idx == 1:
        return [(x, y) for y in range(blk) for x in range(blk)]
    if idx == 2:
        return [(x, y) for x in range(blk) for y in range(blk)]
    out, x, y = [], 0, 0
    while len(out) < blk * blk:
        while y >= 0:
            if x < blk and y < blk:
                out.append((x, y))
            y -= 1
            x += 1
        y, x = x, 0
    return out


SCAN = [[scan_order(idx, 1 << lg) for lg in range(4)] for idx in range(3)]       # ScanOrder[log2BlockSize][scanIdx] as SCAN[scanIdx][log2BlockSize]
SIG_CTX_4X4 = [0, 1, 4, 5, 2, 3, 4, 5, 6, 6, 8, 8, 7, 7, 8]                       # ctxIdxMap of 9.3.4.2.5, i = (yC << 2) + xC
INTER_WRITER_SWITCHES = ("merge_idx_all_context", "amp_bypass_inverted", "col_ref_idx_always", "idc_first_bin_for_8x4")
LOOP_WRITER_SWITCHES = ("across_tied_to_deblock", "sao_edge_signs_coded", "sao_type_second_bin_context", "sao_cr_class_coded", "sao_up_after_left",
                        "sao_abs_cmax_31")
WRITER_SWITCHES = ("scan_ignored", "hidden_sign_written", "ctxset_not_raised", "rice_never_raised", "csbf_wrong_neighbours")


def sig_ctx_inc(lg, cidx, scan_idx, xc, yc, prev_csbf):
    """9.3.4.2.5: ctxInc of sig_coeff_flag at (xc, yc) of a 2^lg block; prev_csbf = coded_sub_block_flag of the sub-block to the right | below << 1"""
    if lg == 2:
        sig = SIG_CTX_4X4[(yc << 2) + xc]
    elif xc + yc == 0:
        sig = 0
    else:
        xp, yp = xc & 3, yc & 3
        if prev_csbf == 0:
            sig = 2 if xp + yp == 0 else (1 if xp + yp < 3 else 0)
        elif prev_csbf == 1:
            sig = 2 if yp == 0 else (1 if yp == 1 else 0)
        elif prev_csbf == 2:
            sig = 2 if xp == 0 else (1 if xp == 1 else 0)
        else:
            sig = 2
        if cidx == 0:
            if (xc >> 2) + (yc >> 2) > 0:
                sig += 3
            sig += (9 if scan_idx == 0 else 15) if lg == 3 else 21
        else:
            sig += 9 if lg == 3 else 12
    return sig if cidx == 0 else 27 + sig


def last_prefix(pos):
    """7.4.9.11 backwards: (last_sig_coeff prefix, number of suffix bits, suffix) of a coordinate"""
    if pos < 4:
        return pos, 0, 0
    for pre in range(4, 10):
        nb = (pre >> 1) - 1
        base = (1 << nb) * (2 + (pre & 1))
        if base <= pos < base + (1 << nb):
            return pre, nb, pos - base
    raise AssertionError(pos)


def scaling_list_data(b, spec):
    """7.3.4.  spec[(sizeId, matrixId)] = ("ref", scaling_list_pred_matrix_id_delta) or ("coded", the 16 / 64 entries in diagonal scan order, dc or None);
    a list that the spec does not name is predicted with delta 0: the default list (7.4.5).  sizeId 3 has the matrixId 0 and 1."""
    for size_id in range(4):
        for matrix_id in range(2 if size_id == 3 else 6):
            e = spec.get((size_id, matrix_id), ("ref", 0))
            b.u(1, 1 if e[0] == "coded" else 0)                     # scaling_list_pred_mode_flag
            if e[0] == "ref":
                assert 0 <= e[1] <= matrix_id
                b.ue(e[1])
                continue
            coefs, dc = e[1], e[2]
            assert len(coefs) == min(64, 1 << (4 + (size_id << 1))) and all(1 <= v <= 255 for v in coefs) and (dc is None) == (size_id < 2)
            nxt = 8
            if size_id > 1:
                assert 1 <= dc <= 255
                b.se(dc - 8)
                nxt = dc
            for v in coefs:
                d = (v - nxt + 128) % 256 - 128                     # scaling_list_delta_coef in -128 .. 127; nextCoef = (nextCoef + delta + 256) % 256
                b.se(d)
                nxt = v


def intra_chroma_mode(v, luma_mode):
    """8.4.3 (ChromaArrayType 1): only to choose scanIdx"""
    if v == 4:
        return luma_mode
    m = (0, 26, 10, 1)[v]
    return 34 if m == luma_mode else m


def unit_tus(u, count):
    """The transform units of a unit's script in one form: [{0: {(x, y): level}, 1: {..}, 2: {..}, "tskip": set of components}] -- from ``coef`` or ``dc``"""
    if u.get("coef") is not None:
        assert u.get("dc") is None and len(u["coef"]) == count, (len(u["coef"]), count)
        out = []
        for e in u["coef"]:
            e = e or {}
            t = {k: dict(e.get(k) or {}) for k in (0, 1, 2)}
            assert all(lv for k in (0, 1, 2) for lv in t[k].values()), "a level 0 is not a coefficient"
            t["tskip"] = set(e.get("tskip", ()))
            out.append(t)
        return out
    dc = u.get("dc") or [None] * count
    assert len(dc) == count
    return [{k: ({(0, 0): (e or (0, 0, 0))[k]} if (e or (0, 0, 0))[k] else {}) for k in (0, 1, 2)} | {"tskip": set()} for e in dc]


def mpm_candidates(a, b):
    """8.4.2: candModeList from candIntraPredModeA / B"""
    if a == b:
        return [0, 1, 26] if a < 2 else [a, 2 + ((a + 29) % 32), 2 + ((a - 2 + 1) % 32)]
    return [a, b, 0 if 0 not in (a, b) else (1 if 1 not in (a, b) else 26)]


class _Picture:
    """One picture's slice data (7.3.8): the maps that the context selection and the candidate derivation read, and the syntax itself."""

    def __init__(self, seq, p, pl, kind, sw=None, stats=None):
        self.seq, self.p, self.pl, self.kind, self.g = seq, p, pl, kind, geometry(seq)
        self.sw, self.dqp_coded, self.dqp_units = sw or {}, False, []
        self.stats = stats if stats is not None else {}             # what the residual syntax met, counted by name (the host test asserts coverage from it)
        self.W, self.H = coded_size(seq)
        self.cw, self.ch = ctb_dims(seq)
        h8, w8 = (self.H + 7) // 8, (self.W + 7) // 8
        self.depth = np.zeros((h8, w8), np.int32)                   # CtDepth, cu_skip_flag, CuPredMode (0 inter, 1 intra, 2 intra with pcm_flag) per 8x8
        self.skip = np.zeros((h8, w8), bool)
        self.pred = np.zeros((h8, w8), np.int32)
        self.mode = np.ones((self.H // 4, self.W // 4), np.int32)   # IntraPredModeY per 4x4
        self.slice_of = np.zeros(self.cw * self.ch, np.int32)       # SliceAddrRs per CTB
        inter = [u["t"] for (_, _, _, _, u) in walk(seq, p) if u["t"] in ("skip", "inter")]
        self.all_skip = all(t == "skip" for t in inter)

    def z(self, x, y):
        return zscan(x, y, self.g["ctb"], self.cw)

    def avail(self, xc, yc, xn, yn):
        """6.4.1: inside the picture, not later in z-scan order, in the same slice (no tiles)"""
        if xn < 0 or yn < 0 or xn >= self.W or yn >= self.H or self.z(xn, yn) > self.z(xc, yc):
            return False
        s = self.g["ctb"]
        return self.slice_of[(yn >> s) * self.cw + (xn >> s)] == self.slice_of[(yc >> s) * self.cw + (xc >> s)]

    def sao(self, c, a, sl):
        """7.3.8.3 for the CTB at address a of the slice sl.  sao_merge_*_flag on their one context; sao_type_idx: a context bin, then a bypass bin;
        sao_offset_abs: truncated unary, cMax 7 (8 bits), bypass; signs for band offsets that are not 0; sao_band_position 5 bits; sao_eo_class 2 bits"""
        sw = self.sw

        def met(*key):
            self.stats[("sao",) + key] = self.stats.get(("sao",) + key, 0) + 1
        e = (self.p.get("sao_ctbs") or [None] * (self.cw * self.ch))[a] or {}
        merge = e.get("merge")
        assert merge in (None, "left", "up") and (merge is None or (e.get("y") is None and e.get("c") is None)), e
        rx, ry = a % self.cw, a // self.cw
        left_ok, up_ok = rx > 0 and a - 1 >= sl["first"], ry > 0 and a - self.cw >= sl["first"]
        assert merge != "left" or left_ok, "sao_merge_left_flag: the CTB on the left lies outside the slice or the picture"
        assert merge != "up" or up_ok, "sao_merge_up_flag: the CTB above lies outside the slice or the picture"
        if left_ok:
            c.decision("sao_merge_flag", 0, 1 if merge == "left" else 0)
            met("merge_left", 1 if merge == "left" else 0)
        if up_ok and (merge != "left" or sw.get("sao_up_after_left")):
            c.decision("sao_merge_flag", 0, 1 if merge == "up" else 0)
            met("merge_up", 1 if merge == "up" else 0)
        if merge:
            return
        cb, cr = e.get("c") or (None, None)
        assert (cb is None) == (cr is None) and (cb is None or (cb[0] == cr[0] and (cb[0] == "band" or cb[1] == cr[1]))), "Cr has Cb's type and class"
        for cidx, ent in enumerate((e.get("y"), cb, cr)):
            if not sl["sao"][1 if cidx else 0]:
                assert ent is None, "an entry for a component whose slice flag is 0"
                continue
            typ = 0 if ent is None else {"band": 1, "edge": 2}[ent[0]]
            if cidx < 2:
                c.decision("sao_type_idx", 0, 1 if typ else 0)
                if typ:
                    c.decision("sao_type_idx", 0, typ - 1) if sw.get("sao_type_second_bin_context") else c.bypass(typ - 1)
            met("type", cidx, typ)
            if not typ:
                continue
            _, where, offs = ent
            assert len(offs) == 4 and all(abs(v) <= 7 for v in offs) and (typ == 1 or all(v >= 0 for v in offs)), ent
            cmax = 31 if sw.get("sao_abs_cmax_31") else 7
            for v in offs:
                for _ in range(abs(v)):
                    c.bypass(1)
                if abs(v) < cmax:
                    c.bypass(0)
                met("abs", abs(v))
            if typ == 1 or sw.get("sao_edge_signs_coded"):
                for v in offs:
                    if v:
                        c.bypass(1 if v < 0 else 0)
                        met("sign", 1 if v < 0 else 0)
            if typ == 1:
                assert 0 <= where <= 31
                for i in range(4, -1, -1):
                    c.bypass((where >> i) & 1)
                met("band_position", cidx, where)
            elif cidx < 2 or sw.get("sao_cr_class_coded"):
                assert 0 <= where <= 3
                c.bypass(where >> 1); c.bypass(where & 1)
                met("class", cidx, where)

    def quadtree(self, c, x, y, log2, depth, node):
        """7.3.8.4"""
        n = 1 << log2
        if self.seq.get("cu_qp_delta", 0) and log2 >= self.g["ctb"] - self.seq.get("diff_cu_qp_delta_depth", 0):
            self.dqp_coded = False                                  # IsCuQpDeltaCoded = 0 at the start of a quantisation group
        if x + n <= self.W and y + n <= self.H and log2 > self.g["min_cb"]:
            split = node["t"] == "split"
            inc = sum(1 for (xn, yn) in ((x - 1, y), (x, y - 1)) if self.avail(x, y, xn, yn) and self.depth[yn >> 3, xn >> 3] > depth)      # 9.3.4.2.2
            c.decision("split_cu_flag", inc, 1 if split else 0)
        else:
            split = log2 > self.g["min_cb"]                         # inferred
            assert (node["t"] == "split") == split, (x, y, log2, node["t"])
        if split:
            for i, sub in enumerate(node["sub"]):
                x1, y1 = x + (i & 1) * (n >> 1), y + (i >> 1) * (n >> 1)
                if x1 < self.W and y1 < self.H:
                    self.quadtree(c, x1, y1, log2 - 1, depth + 1, sub)
        else:
            self.coding_unit(c, x, y, log2, depth, node)

    def coding_unit(self, c, x, y, log2, depth, u):
        """7.3.8.5"""
        t, n, kind, b = u["t"], 1 << log2, self.kind, c.b
        if self.seq.get("transquant_bypass", 0):
            c.decision("cu_transquant_bypass", 0, 1 if u.get("bypass", 0) else 0)
        else:
            assert not u.get("bypass", 0)
        if kind != "I":
            inc = sum(1 for (xn, yn) in ((x - 1, y), (x, y - 1)) if self.avail(x, y, xn, yn) and self.skip[yn >> 3, xn >> 3])               # 9.3.4.2.2
            c.decision("cu_skip_flag", inc, 1 if t == "skip" else 0)
        area = (slice(y >> 3, (y + n) >> 3), slice(x >> 3, (x + n) >> 3))
        self.depth[area], self.skip[area], self.pred[area] = depth, t == "skip", {"pcm": 2, "intra": 1}.get(t, 0)
        self.mode[y >> 2:(y + n) >> 2, x >> 2:(x + n) >> 2] = 1
        if t == "skip":
            assert kind != "I"
            if "merge" in u:
                self.merge_idx(c, u["merge"])                       # prediction_unit() of a skipped unit: merge_idx alone
            else:
                assert (self.step == 1 or self.all_skip) and self.p.get("max_merge", 1) == 1     # (MaxNumMergeCand 1: no merge_idx)
            return
        if kind != "I":
            c.decision("pred_mode_flag", 0, 0 if t == "inter" else 1)
        if t == "inter":
            self.partitioned_unit(c, x, y, log2, depth, u) if "pus" in u else self.inter_unit(c, x, y, log2, depth, u)
            return
        assert t in ("pcm", "intra")
        nxn = t == "intra" and len(u["modes"]) == 4
        if log2 == self.g["min_cb"]:
            c.decision("part_mode", 0, 0 if nxn else 1)             # intra units: one bin, 1 = PART_2Nx2N
        else:
            assert not nxn, "NxN only at the minimum coding block size"
        if not nxn and self.g["pcm"][0] <= log2 <= self.g["pcm"][1]:
            c.terminate(1 if t == "pcm" else 0)                     # pcm_flag
        else:
            assert t != "pcm", "a PCM unit outside the PCM size range"
        if t == "pcm":
            b.align_zero()                                          # the flush leaves the writer one bit in front of pcm_alignment_zero_bit
            for key, s in (("y", n), ("cb", n // 2), ("cr", n // 2)):
                v = np.asarray(u[key], np.uint8)
                assert v.shape == (s, s), (key, v.shape, s)
                b.raw(v.tobytes())
            c.start()                                               # 9.3.2.5: the engine is initialised again behind the samples (contexts keep their state)
            return
        pb = n // 2 if nxn else n
        coded = []
        for i, m in enumerate(u["modes"]):
            bx, by = x + (i & 1) * pb, y + (i >> 1) * pb
            cand = []
            for k, (xn, yn) in enumerate(((bx - 1, by), (bx, by - 1))):     # 8.4.2
                ok = self.avail(bx, by, xn, yn) and self.pred[yn >> 3, xn >> 3] == 1
                if k == 1 and ok and yn < ((by >> self.g["ctb"]) << self.g["ctb"]):
                    ok = False
                cand.append(int(self.mode[yn >> 2, xn >> 2]) if ok else 1)
            coded.append((mpm_candidates(*cand), m))
            self.mode[by >> 2:(by + pb) >> 2, bx >> 2:(bx + pb) >> 2] = m
        for cand, m in coded:
            c.decision("prev_intra_luma_pred", 0, 1 if m in cand else 0)
        for cand, m in coded:
            if m in cand:
                i = cand.index(m)                                   # mpm_idx: truncated Rice, cMax 2, bypass
                c.bypass(1 if i else 0)
                if i:
                    c.bypass(i - 1)
            else:
                rem = m - sum(1 for q in cand if q < m)             # rem_intra_luma_pred_mode: five bits
                for i in range(4, -1, -1):
                    c.bypass((rem >> i) & 1)
        v = u.get("chroma", 4)
        c.decision("intra_chroma_pred_mode", 0, 0 if v == 4 else 1)
        if v != 4:
            c.bypass(v >> 1); c.bypass(v & 1)
        self.transform_tree(c, u, x, y, log2, nxn, True)

    def transform_tree(self, c, u, x, y, log2, nxn, intra):
        """7.3.8.8 / 7.3.8.10 for a tree of uniform depth u["tu"]"""
        tu = u.get("tu", 1 if nxn else 0)
        tus = unit_tus(u, tu_leaves(log2, nxn, tu))
        small = log2 - tu == 2                                      # 4x4 luma blocks: the chroma of four of them is one block, coded with the fourth
        max_depth = self.g["tu_depth"] + nxn if intra else self.g["tu_depth_inter"]
        inter_split = not intra and self.g["tu_depth_inter"] == 0 and u.get("part", "2Nx2N") != "2Nx2N"       # interSplitFlag (7.4.9.8), at depth 0
        bypass = bool(u.get("bypass", 0))
        cm = intra_chroma_mode(u.get("chroma", 4), u["modes"][0]) if intra else None

        def chroma_coded(first, count, comp):
            return any(tus[i][comp] for i in range(first, first + count) if not small or i % 4 == 3)

        def tree(x0, y0, lg, d, blk, first, par):
            count = 4 ** (tu - d)
            want = d < tu
            if lg <= self.g["max_tb"] and lg > 2 and d < max_depth and not (nxn and d == 0):
                c.decision("split_transform_flag", 5 - lg, 1 if want else 0)
            else:
                assert want == (lg > self.g["max_tb"] or ((nxn or inter_split) and d == 0)), ("the script's depth is not what 7.4.9.8 infers", x0, y0, lg, d, tu)
            cbf = list(par)
            if lg > 2:
                for k in (0, 1):
                    v_ = 1 if chroma_coded(first, count, k + 1) else 0
                    if d == 0 or par[k]:
                        c.decision("cbf_cb_cr", d, v_)
                    else:
                        assert not v_
                    cbf[k] = v_
            if want:
                for i in range(4):
                    tree(x0 + (i & 1) * (1 << (lg - 1)), y0 + (i >> 1) * (1 << (lg - 1)), lg - 1, d + 1, i, first + i * (count // 4), cbf)
                return
            t = tus[first]
            if intra or d != 0 or cbf[0] or cbf[1]:
                c.decision("cbf_luma", 1 if d == 0 else 0, 1 if t[0] else 0)
            else:
                assert t[0], "cbf_luma is inferred to be 1 at depth 0 of an inter unit without chroma coefficients"
            if (t[0] or cbf[0] or cbf[1]) and self.seq.get("cu_qp_delta", 0) and not self.dqp_coded:       # 7.3.8.10: cbfLuma || cbfChroma (4x4: the parent's)
                self.dqp_coded, self.dqp_units = True, self.dqp_units + [id(u)]
                v = u.get("dqp", 0)
                assert -26 <= v <= 25
                for i in range(min(abs(v), 5)):                     # cu_qp_delta_abs: prefix TU, cMax 5, ctxInc 0 for the first bin and 1 for the others
                    c.decision("cu_qp_delta_abs", 1 if i else 0, 1)
                if abs(v) < 5:
                    c.decision("cu_qp_delta_abs", 1 if v else 0, 0)
                else:
                    c.egk(abs(v) - 5, 0)
                if v:
                    c.bypass(1 if v < 0 else 0)                     # cu_qp_delta_sign_flag
            luma_mode = (u["modes"][(first >> (2 * (tu - 1))) & 3] if nxn else u["modes"][0]) if intra else None
            if t[0]:
                self.residual(c, lg, 0, t[0], luma_mode, 0 in t["tskip"], bypass)
            else:
                assert 0 not in t["tskip"]
            if lg > 2 or blk == 3:
                for k in (0, 1):
                    if cbf[k]:
                        self.residual(c, max(lg - 1, 2), k + 1, t[k + 1], cm, (k + 1) in t["tskip"], bypass)
                    else:
                        assert (k + 1) not in t["tskip"]
            elif u.get("coef") is not None:                         # (``dc`` ignores the chroma levels of the first three, as it always did)
                assert not t[1] and not t[2] and not (t["tskip"] - {0}), "the chroma of four 4x4 luma blocks is scripted with the fourth"
        tree(x, y, log2, 0, 0, 0, [0, 0])

    def residual(self, c, lg, cidx, coefs, intra_mode, tskip, bypass):
        """7.3.8.11 with the context selection of 9.3.4.2.3 - 9.3.4.2.7 and the binarisation of 9.3.3.11.  coefs {(x, y): level}, not empty;
        intra_mode: the block's intra prediction mode (None in an inter unit)"""
        sw, n = self.sw, 1 << lg

        def met(*key):
            self.stats[key] = self.stats.get(key, 0) + 1
        assert coefs and all(0 <= x < n and 0 <= y < n and lv and -32768 <= lv <= 32767 for (x, y), lv in coefs.items()), (lg, coefs)
        if self.seq.get("transform_skip", 0) and not bypass and lg == 2:
            c.decision("transform_skip_flag", 1 if cidx else 0, 1 if tskip else 0)
        else:
            assert not tskip
        scan_idx = 0
        if intra_mode is not None and (lg == 2 or (lg == 3 and cidx == 0)) and not sw.get("scan_ignored"):
            scan_idx = 2 if 6 <= intra_mode <= 14 else (1 if 22 <= intra_mode <= 30 else 0)
        sb_scan, pos_scan = SCAN[scan_idx][lg - 2], SCAN[scan_idx][2]
        met("scan", "intra" if intra_mode is not None else "inter", lg, min(cidx, 1), scan_idx)
        last_sb, last_pos = max((i, k) for i, (xs, ys) in enumerate(sb_scan) for k, (xp, yp) in enumerate(pos_scan) if (4 * xs + xp, 4 * ys + yp) in coefs)
        lx, ly = 4 * sb_scan[last_sb][0] + pos_scan[last_pos][0], 4 * sb_scan[last_sb][1] + pos_scan[last_pos][1]
        if scan_idx == 2:
            lx, ly = ly, lx                                         # 7.3.8.11: the coded pair is swapped for the vertical scan
        off, shift = (15, lg - 2) if cidx else (3 * (lg - 2) + ((lg - 1) >> 2), (lg + 1) >> 2)     # 9.3.4.2.3
        pre = [last_prefix(lx), last_prefix(ly)]
        for name, (p_, _, _) in zip(("last_sig_coeff_prefix", "last_sig_coeff_y_prefix"), pre):
            for i in range(p_):
                c.decision(name, off + (i >> shift), 1)
            if p_ < 2 * lg - 1:                                     # truncated unary, cMax = (log2TrafoSize << 1) - 1
                c.decision(name, off + (p_ >> shift), 0)
        for (_, nb, suf) in pre:
            met("last_suffix_bits", nb)
            for i in range(nb - 1, -1, -1):
                c.bypass((suf >> i) & 1)
        hiding = self.seq.get("sign_hiding", 0) and not bypass
        csbf = {}
        g1ctx, first_group = 1, True                                # greater1Ctx as the last flag of the previous sub-block left it (9.3.4.2.6)
        for i in range(last_sb, -1, -1):
            xs, ys = sb_scan[i]
            pos = [(4 * xs + xp, 4 * ys + yp) for (xp, yp) in pos_scan]
            lev = [coefs.get(q, 0) for q in pos]
            right, below = csbf.get((xs + 1, ys), 0), csbf.get((xs, ys + 1), 0)
            infer = False
            if 0 < i < last_sb:
                csbf[(xs, ys)] = 1 if any(lev) else 0
                ctx = csbf.get((xs - 1, ys), 0) | csbf.get((xs, ys - 1), 0) if sw.get("csbf_wrong_neighbours") else right | below
                c.decision("coded_sub_block_flag", ctx + (2 if cidx else 0), csbf[(xs, ys)])        # 9.3.4.2.4
                infer = True
                met("coded_sub_block_flag", csbf[(xs, ys)], right | below)
            else:
                csbf[(xs, ys)] = 1                                  # inferred for the first and the last sub-block
            if not csbf[(xs, ys)]:
                continue
            for k in range(last_pos - 1 if i == last_sb else 15, -1, -1):
                if k > 0 or not infer:
                    c.decision("sig_coeff_flag", sig_ctx_inc(lg, cidx, scan_idx, pos[k][0], pos[k][1], right | (below << 1)), 1 if lev[k] else 0)
                    if lev[k]:
                        infer = False
                else:
                    assert lev[0], "sig_coeff_flag of position 0 is inferred to be 1"
                    met("sig_coeff_flag inferred")
            sig = [k for k in range(15, -1, -1) if lev[k]]          # in decoding order
            if not sig:
                continue
            ctx_set = 0 if (i == 0 or cidx) else 2
            if not first_group:
                met("greater1Ctx carried", min(3, g1ctx))
            if not first_group and g1ctx == 0 and not sw.get("ctxset_not_raised"):
                ctx_set += 1
            if sum(1 for k in sig if abs(lev[k]) > 1) > 8:
                met("more than 8 levels above 1")
            first_group, g1ctx = False, 1
            first_g1 = None
            for k in sig[:8]:
                f = 1 if abs(lev[k]) > 1 else 0
                c.decision("coeff_abs_level_greater1", (16 if cidx else 0) + 4 * ctx_set + min(3, g1ctx), f)
                if g1ctx > 0:
                    g1ctx = 0 if f else g1ctx + 1
                if f and first_g1 is None:
                    first_g1 = k
            if first_g1 is not None:
                c.decision("coeff_abs_level_greater2", (4 if cidx else 0) + ctx_set, 1 if abs(lev[first_g1]) > 2 else 0)
            hidden = bool(hiding and sig[0] - sig[-1] > 3)
            if self.seq.get("sign_hiding", 0):
                met("sign hiding", "bypass" if bypass else "coded", min(sig[0] - sig[-1], 5), sum(abs(lev[k]) for k in sig) & 1)
            if hidden:
                assert (sum(abs(lev[k]) for k in sig) & 1) == (1 if lev[sig[-1]] < 0 else 0), "sign data hiding: the parity of the sum is the hidden sign"
            for k in sig:
                if not hidden or k != sig[-1] or sw.get("hidden_sign_written"):
                    c.bypass(1 if lev[k] < 0 else 0)
            rice = 0
            for m, k in enumerate(sig):
                base = (3 if k == first_g1 else 2) if m < 8 else 1
                if abs(lev[k]) >= base:
                    rem = abs(lev[k]) - base                        # coeff_abs_level_remaining, 9.3.3.11
                    cmax = 4 << rice
                    for _ in range(min(rem, cmax) >> rice):
                        c.bypass(1)
                    if rem < cmax:
                        c.bypass(0)
                        for j in range(rice - 1, -1, -1):
                            c.bypass((rem >> j) & 1)
                    else:
                        c.egk(rem - cmax, rice + 1)
                        met("escape at cRiceParam", rice)
                    if abs(lev[k]) > 3 * (1 << rice) and not sw.get("rice_never_raised"):
                        rice = min(rice + 1, 4)
                        met("cRiceParam raised to", rice)

    def merge_idx(self, c, idx):
        """merge_idx (9.3.3: truncated Rice, cMax = MaxNumMergeCand - 1; the first bin with a context, the others bypass)"""
        cmax = self.p.get("max_merge", 1) - 1
        assert 0 <= idx <= cmax, (idx, cmax)
        for i in range(min(idx + 1, cmax)):
            bin_ = 1 if i < idx else 0
            c.decision("merge_idx", 0, bin_) if i == 0 or self.sw.get("merge_idx_all_context") else c.bypass(bin_)

    def part_mode(self, c, log2, part):
        """9.3.3.7 for an inter unit.  Contexts 9.3.4.2: bin 0 -> 0, bin 1 -> 1, bin 2 -> 2 at the minimum size, else 3; bin 3 bypass"""
        at_min, amp = log2 == self.g["min_cb"], self.seq.get("amp", 0)
        if at_min:
            bins = {"2Nx2N": "1", "2NxN": "01", "Nx2N": "00"} if log2 == 3 else {"2Nx2N": "1", "2NxN": "01", "Nx2N": "001", "NxN": "000"}
        elif not amp:
            bins = {"2Nx2N": "1", "2NxN": "01", "Nx2N": "00"}
        else:
            bins = {"2Nx2N": "1", "2NxN": "011", "2NxnU": "0100", "2NxnD": "0101", "Nx2N": "001", "nLx2N": "0000", "nRx2N": "0001"}
        assert part in bins, (part, log2, "not a partition of this size")
        for i, ch in enumerate(bins[part]):
            if i == 3:
                c.bypass(int(ch) ^ (1 if self.sw.get("amp_bypass_inverted") else 0))
            else:
                c.decision("part_mode", i if i < 2 or at_min else 3, int(ch))

    def partitioned_unit(self, c, x, y, log2, depth, u):
        """7.3.8.5 / 7.3.8.6 / 7.3.8.9 as scripted: part_mode, then per prediction unit merge_flag and merge_idx or inter_pred_idc, ref_idx_lX, mvd_lX and
        mvp_lX_flag; the writer derives no motion"""
        pl, kind, n = self.pl, self.kind, 1 << log2
        assert kind != "I"
        self.part_mode(c, log2, u["part"])
        pbs = partitions(u["part"], x, y, n)
        assert len(pbs) == len(u["pus"]), (u["part"], len(u["pus"]))
        merged = False
        for (xp, yp, w, h), pu in zip(pbs, u["pus"]):
            merged = "merge" in pu
            c.decision("merge_flag", 0, 1 if merged else 0)
            if merged:
                self.merge_idx(c, pu["merge"])
                continue
            l0, l1 = pu.get("l0"), pu.get("l1")
            assert l0 or l1
            if kind == "B":
                assert not (l0 and l1 and w + h == 12), "8x4 and 4x8 blocks are never bi-predictive"
                if w + h != 12 or self.sw.get("idc_first_bin_for_8x4"):
                    c.decision("inter_pred_idc", depth, 1 if l0 and l1 else 0)
                if not (l0 and l1):
                    c.decision("inter_pred_idc", 4, 1 if l1 else 0)
            else:
                assert l0 and not l1
            for name, q in (("l0", l0), ("l1", l1)):
                if not q:
                    continue
                idx, mvd, flag = q
                cnt = len(pl[name])
                assert 0 <= idx < cnt
                if cnt > 1:
                    for i in range(min(idx + 1, cnt - 1)):
                        bin_ = 1 if i < idx else 0
                        c.decision("ref_idx", i, bin_) if i < 2 else c.bypass(bin_)
                if name == "l1" and self.p.get("mvd_l1_zero", 0) and l0 and l1:
                    assert tuple(mvd) == (0, 0), "mvd_l1_zero_flag: MvdL1 of a bi-predictive unit is not coded"
                else:
                    self.mvd(c, mvd)
                c.decision("mvp_flag", 0, flag)
        tus = unit_tus(u, tu_leaves(log2, False, u.get("tu", 0)))
        root = 1 if any(t[k] for t in tus for k in (0, 1, 2)) else 0
        if u["part"] == "2Nx2N" and merged:
            assert root, "a 2Nx2N merge unit without residual is a skipped unit: rqt_root_cbf is not coded and inferred to be 1"
        else:
            c.decision("rqt_root_cbf", 0, root)
        if root:
            self.transform_tree(c, u, x, y, log2, False, False)

    @staticmethod
    def mvd(c, mvd):
        """7.3.8.9"""
        assert all(-32768 <= v <= 32767 for v in mvd)
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
                    c.egk(abs(mvd[i]) - 2, 1)                       # abs_mvd_minus2: EG1
                c.bypass(1 if mvd[i] < 0 else 0)                    # mvd_sign_flag

    def inter_unit(self, c, x, y, log2, depth, u):
        pl, kind = self.pl, self.kind
        assert kind != "I" and log2 == self.g["ctb"] and log2 <= 5 and (self.step == 1 or u is self.first_unit or u == self.first_unit), \
            "a slice of several CTBs repeats one inter unit"
        c.decision("part_mode", 0, 1)
        c.decision("merge_flag", 0, 0)
        l0, l1 = u.get("l0"), u.get("l1")
        if kind == "B":
            c.decision("inter_pred_idc", depth, 1 if l0 and l1 else 0)          # nPbW + nPbH != 12: first bin with ctxInc = CtDepth
            if not (l0 and l1):
                c.decision("inter_pred_idc", 4, 1 if l1 else 0)
        else:
            assert l0 and not l1
        for name, q in (("l0", l0), ("l1", l1)):
            if not q:
                continue
            n, idx = len(pl[name]), pl[name].index(q[0])
            if n > 1:                                               # ref_idx_lX: truncated unary, cMax = n - 1; bins 0 and 1 with contexts, the rest bypass
                for i in range(min(idx + 1, n - 1)):
                    bin_ = 1 if i < idx else 0
                    c.decision("ref_idx", i, bin_) if i < 2 else c.bypass(bin_)
            mvd = q[1] if self.at_first else (0, 0)                 # both AMVP candidates zero / the first candidate is this vector (module docstring)
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
                        c.egk(abs(mvd[i]) - 2, 1)                   # abs_mvd_minus2: EG1
                    c.bypass(1 if mvd[i] < 0 else 0)                # mvd_sign_flag
            c.decision("mvp_flag", 0, 0)
        tus = unit_tus(u, tu_leaves(log2, False, u.get("tu", 0)))
        root = 1 if any(t[k] for t in tus for k in (0, 1, 2)) else 0
        c.decision("rqt_root_cbf", 0, root)
        if root:
            self.transform_tree(c, u, x, y, log2, False, False)


def write(seq, pics, stats=None, **sw):
    """Annex-B bytes of the script.  The keyword arguments (WRITER_SWITCHES, INTER_WRITER_SWITCHES, LOOP_WRITER_SWITCHES) make the residual / the inter / the
    loop filter syntax wrong on purpose; stats: a dict that counts what residual_coding, sao() and the slice headers met."""
    assert all(k in WRITER_SWITCHES + INTER_WRITER_SWITCHES + LOOP_WRITER_SWITCHES for k in sw), sw
    cw, ch = ctb_dims(seq)
    n_ctbs = cw * ch
    s = 1 << geometry(seq)["ctb"]
    out = [vps(), sps(seq), pps(seq)]
    plans = plan(seq, pics)
    pocs = [p["poc"] for p in pics]
    for k, (p, pl) in enumerate(zip(pics, plans)):
        pl["pocs"] = pocs
        kind, cus = p["kind"], p["cus"]
        assert len(cus) == n_ctbs
        pic = _Picture(seq, p, pl, kind, sw, stats)
        assert p.get("sao_ctbs") is None or len(p["sao_ctbs"]) == n_ctbs
        for ordinal, sl in enumerate(slice_table(seq, p)):
            first, pic.step = sl["first"], sl["count"]
            b = Bits()
            pic.pl = spl = slice_plan(pl, p, ordinal)
            slice_header(b, seq, p, spl, first == 0, first, n_ctbs, sw, sl, stats)
            c = Cabac(b, {"I": 0, "P": 1, "B": 2}[kind], p.get("qp", seq.get("init_qp", 26)))
            last = first + sl["count"] - 1
            pic.slice_of[first:last + 1] = first
            pic.first_unit = cus[first]
            for a in range(first, last + 1):
                pic.at_first = a == first
                if sl["sao"][0] or sl["sao"][1]:
                    pic.sao(c, a, sl)
                else:
                    assert not (p.get("sao_ctbs") or [None] * n_ctbs)[a], "SAO parameters in a slice with both flags 0"
                pic.quadtree(c, (a % cw) * s, (a // cw) * s, geometry(seq)["ctb"], 0, cus[a])
                c.terminate(1 if a == last else 0)                  # end_of_slice_segment_flag; the flush's last bit is rbsp_slice_segment_trailing_bits' 1
            b.align_zero()
            out.append(nal(pl["typ"], b.bytes()))
        assert all(id(u) in pic.dqp_units for (_, _, _, _, u) in walk(seq, p) if u.get("dqp")), "a dqp that no transform unit could carry"
    return b"".join(out)

