"""H.265 deblocking and sample adaptive offset typed out once more, in numpy and plain integers, for the scripted streams of tests/scripted_hevc.py.

Restated from the clauses and computed from the SCRIPT, never from a bitstream -- not from oracle/orc_hevc_filter.c, tools/hevcgen.c, hevc_bs.h or the kernels:
  8.7.2.3    the edges: transform block and prediction block edges on the 8x8 luma grid; filterEdgeFlag 0 at the picture edge, at the left / top edge of a
             slice whose slice_loop_filter_across_slices_enabled_flag is 0 (without tiles the q side of an edge is always the later slice, so "the flag
             of the later slice" and "the flag of the slice that holds q0" are one rule), and every edge of a unit whose slice has the filter disabled
  8.7.2.4    bS 2 intra, 1 a transform edge with a luma cbf, 1 by pictures / vector count / vectors 4 or more apart (pictures compared as pictures)
  8.7.2.5    all vertical edges, then all horizontal ones on the result; qPL, beta and tC with the offsets of the slice that holds q0,0; dE, dEp, dEq, the
             strong and the normal filter; nDp / nDq 0 for PCM units under pcm_loop_filter_disabled_flag and for bypass units; chroma at bS 2 on the 8-sample
             chroma grid with QpC through Table 8-10 from qPL + the PPS offset of the component
  8.7.3      SAO on the deblocked picture into a separate picture: band and edge offset, the samples it leaves alone, Clip1
The unfiltered pictures, the QpY of the coding units (8.6.1) and the motion come from tests/hevc_resid_ref.py or tests/hevc_inter_ref.py through their
``post`` hook; the picture that later pictures predict from is the FILTERED one.  Sample arrays are indexed [y, x].

``expect`` returns the planes and one record per luma edge segment (4 samples) of the edge set (filtered or not), per filtered chroma segment and per
CTB component with SAO; the switches make it wrong on purpose."""
import numpy as np

import hevc_inter_ref as hr
import hevc_intra_ref as ir
import hevc_resid_ref as rr
import scripted_hevc as hw

SWITCHES = ("horizontal_before_vertical", "tc_without_bs_term", "offsets_of_p_slice", "qp_sum_without_plus_1", "pcm_qp_zero", "chroma_uses_slice_qp_offset",
            "chroma_at_bs1", "chroma_on_luma_grid", "dE_side_thresholds_swapped", "no_10tc_gate", "strong_clip_tc", "edges_on_4_grid",
            "across_flag_of_earlier_slice", "disabled_by_p_slice", "sao_before_deblock", "sao_in_place", "band_no_wrap", "edge_idx_unmapped",
            "edge_signs_plus_minus_swapped", "cr_own_class", "sao_at_picture_border", "sao_ignores_exempt_units", "sao_flag_of_earlier_slice",
            "reference_is_unfiltered")
# Table 8-12: beta' for Q 0 .. 51 and tC' for Q 0 .. 53
BETA = [0] * 16 + list(range(6, 19)) + list(range(20, 66, 2))
TC = [0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24]
assert len(BETA) == 52 and len(TC) == 54
SAO_POS = (((-1, 0), (1, 0)), ((0, -1), (0, 1)), ((-1, -1), (1, 1)), ((1, -1), (-1, 1)))       # Table 8-13: (hPos, vPos) of the two neighbours by SaoEoClass


def clip3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


def qpc_of(qpi):
    """Table 8-10 (ChromaArrayType 1) as 8.7.2.5.5 uses it: no clip of qPi"""
    return qpi if qpi < 30 else (qpi - 6 if qpi > 43 else rr.QPC[qpi])


# ---- 8.7.2.5.3, 8.7.2.5.6, 8.7.2.5.7: one luma segment --------------------------------------------------------------------------------------------------
def luma_decisions(p, q, beta, tc, sw={}):
    """p, q: [4 lines][4 samples] with index 0 next to the edge -> dict(d, dE, dEp, dEq, and what each inequality had)"""
    ab = abs
    dp0, dp3 = ab(p[0][2] - 2 * p[0][1] + p[0][0]), ab(p[3][2] - 2 * p[3][1] + p[3][0])
    dq0, dq3 = ab(q[0][2] - 2 * q[0][1] + q[0][0]), ab(q[3][2] - 2 * q[3][1] + q[3][0])
    dpq0, dpq3, dp, dq = dp0 + dq0, dp3 + dq3, dp0 + dp3, dq0 + dq3
    d = dpq0 + dpq3
    out = dict(d=d, beta=beta, tc=tc, dE=0, dEp=0, dEq=0, dp=dp, dq=dq, side=(beta + (beta >> 1)) >> 3, strong=[])
    if d < beta:
        sam = []
        for k, dpq in ((0, 2 * dpq0), (3, 2 * dpq3)):
            c = (dpq, beta >> 2, ab(p[k][3] - p[k][0]) + ab(q[k][0] - q[k][3]), beta >> 3, ab(p[k][0] - q[k][0]), (5 * tc + 1) >> 1)
            out["strong"].append(c)                                 # (value, bound) three times: each value must be below its bound
            sam.append(c[0] < c[1] and c[2] < c[3] and c[4] < c[5])
        out["dE"] = 2 if all(sam) else 1
        a, b = (dq, dp) if sw.get("dE_side_thresholds_swapped") else (dp, dq)
        out["dEp"], out["dEq"] = int(a < out["side"]), int(b < out["side"])
    return out


def luma_line(p, q, dE, dEp, dEq, tc, sw={}, hit=None):
    """one line: p, q [4] -> (new p [4], new q [4]); hit collects the clips that were reached"""
    hit = hit if hit is not None else set()
    p, q = list(p), list(q)
    if dE == 2:
        c = tc if sw.get("strong_clip_tc") else 2 * tc
        raw = [(p[2] + 2 * p[1] + 2 * p[0] + 2 * q[0] + q[1] + 4) >> 3, (p[2] + p[1] + p[0] + q[0] + 2) >> 2, (2 * p[3] + 3 * p[2] + p[1] + p[0] + q[0] + 4) >> 3,
               (p[1] + 2 * p[0] + 2 * q[0] + 2 * q[1] + q[2] + 4) >> 3, (p[0] + q[0] + q[1] + q[2] + 2) >> 2, (p[0] + q[0] + q[1] + 3 * q[2] + 2 * q[3] + 4) >> 3]
        old = p[:3] + q[:3]
        new = [clip3(o - c, o + c, r) for o, r in zip(old, raw)]
        for o, r in zip(old, raw):
            if r - o >= c:
                hit.add("strong+" if r - o > c else "strong=+")
            if o - r >= c:
                hit.add("strong-" if o - r > c else "strong=-")
        return new[:3] + [p[3]], new[3:] + [q[3]]
    delta = (9 * (q[0] - p[0]) - 3 * (q[1] - p[1]) + 8) >> 4
    if tc and 0 <= 10 * tc - abs(delta) <= 1:
        hit.add("gate at 10tC" if abs(delta) == 10 * tc else "gate at 10tC-1")
    if abs(delta) >= 10 * tc and not sw.get("no_10tc_gate"):
        hit.add("gate")
        return p, q
    hit.add("delta+" if delta > tc else "delta-" if delta < -tc else "delta=+" if delta == tc and tc else "delta=-" if delta == -tc and tc else "delta in")
    delta = clip3(-tc, tc, delta)
    clip1 = lambda v, tag: (hit.add(tag + ("<0" if v < 0 else ">255")) or clip3(0, 255, v)) if not 0 <= v <= 255 else v
    new_p, new_q = list(p), list(q)
    new_p[0], new_q[0] = clip1(p[0] + delta, "p0"), clip1(q[0] - delta, "q0")
    h = tc >> 1
    if dEp:
        dl = (((p[2] + p[0] + 1) >> 1) - p[1] + delta) >> 1
        hit.add("side+" if dl > h else "side-" if dl < -h else "side in")
        new_p[1] = clip1(p[1] + clip3(-h, h, dl), "p1")
    if dEq:
        dl = (((q[2] + q[0] + 1) >> 1) - q[1] - delta) >> 1
        hit.add("side+" if dl > h else "side-" if dl < -h else "side in")
        new_q[1] = clip1(q[1] + clip3(-h, h, dl), "q1")
    return new_p, new_q


def luma_segment(P, Q, beta, tc, sw={}):
    """8.7.2.5.3 with 8.7.2.5.6 / 8.7.2.5.7 for the four lines of a segment -> (the decisions with "hit", new P, new Q); nDp / nDq are the caller's"""
    dec = luma_decisions(P, Q, beta, tc, sw)
    hit, new_p, new_q = set(), [list(l) for l in P], [list(l) for l in Q]
    if dec["dE"]:
        for l in range(4):
            new_p[l], new_q[l] = luma_line(P[l], Q[l], dec["dE"], dec["dEp"], dec["dEq"], tc, sw, hit)
    dec["hit"] = hit
    return dec, new_p, new_q


def chroma_line(p, q, tc, hit=None):
    """8.7.2.5.8: p, q [2] -> (p0', q0')"""
    delta = ((((q[0] - p[0]) << 2) + p[1] - q[1] + 4) >> 3)
    if hit is not None:
        hit.add("cdelta+" if delta > tc else "cdelta-" if delta < -tc else "cdelta in")
    delta = clip3(-tc, tc, delta)
    return clip3(0, 255, p[0] + delta), clip3(0, 255, q[0] - delta)


# ---- 8.7.3: one sample array ------------------------------------------------------------------------------------------------------------------------
def band_table(pos, sw={}):
    t = [0] * 32
    for k in range(4):
        if sw.get("band_no_wrap"):
            if k + pos < 32:
                t[k + pos] = k + 1
        else:
            t[(k + pos) & 31] = k + 1
    return t


def edge_idx(c, a, b, sw={}):
    sign = lambda v: (v > 0) - (v < 0)
    e = 2 + sign(c - a) + sign(c - b)
    return e if sw.get("edge_idx_unmapped") else (1, 2, 0, 3, 4)[e]


def edge_values(mags, sw={}):
    """SaoOffsetVal[0 .. 4] of an edge offset: + + - -"""
    s = (-1, -1, 1, 1) if sw.get("edge_signs_plus_minus_swapped") else (1, 1, -1, -1)
    return [0] + [m * g for m, g in zip(mags, s)]


class Maps:
    """What the script says about one picture, per 4x4 luma block unless stated"""

    def __init__(self, seq, pics, k, plans, ctx, sw):
        p = pics[k]
        self.seq, self.p, self.sw = seq, p, sw
        W, H = self.W, self.H = hw.coded_size(seq)
        g = hw.geometry(seq)
        self.ctb = g["ctb"]
        self.cw, self.ch = hw.ctb_dims(seq)
        self.slices = hw.slice_table(seq, p)
        self.slice_no = np.zeros(self.cw * self.ch, np.int64)       # the slice's number in decoding order, per CTB address
        for i, sl in enumerate(self.slices):
            self.slice_no[sl["first"]:sl["first"] + sl["count"]] = i
        h4, w4 = H // 4, W // 4
        self.intra, self.pcm, self.bypass, self.cbf = (np.zeros((h4, w4), bool) for _ in range(4))
        self.cu = np.zeros((h4, w4), np.int64)                      # the number of the coding unit
        self.tv, self.th, self.pv, self.ph = (np.zeros((h4, w4), bool) for _ in range(4))       # a transform / prediction block begins at this block's left / top edge
        slice_qp = p.get("qp", seq.get("init_qp", 26))
        self.qp = ctx["qpy"].copy() if "qpy" in ctx else np.full((h4, w4), slice_qp, np.int64)
        field = ctx.get("field")
        self.units = []                                             # (x, y, size, type, script) by coding unit number
        self.mot = {}                                               # 4x4 -> [(picture, (mvx, mvy))]: the vectors in use
        pl = plans[k]
        for n_cu, (x, y, log2, depth, u) in enumerate(hw.walk(seq, p)):
            n, t = 1 << log2, u["t"]
            a = (slice(y >> 2, (y + n) >> 2), slice(x >> 2, (x + n) >> 2))
            self.cu[a] = n_cu
            self.units.append((x, y, n, t, u))
            self.intra[a], self.pcm[a], self.bypass[a] = t in ("pcm", "intra"), t == "pcm", bool(u.get("bypass", 0))
            if t == "pcm" and sw.get("pcm_qp_zero"):
                self.qp[a] = 0
            nxn = t == "intra" and len(u["modes"]) == 4
            part = u.get("part", "2Nx2N") if t == "inter" else ("NxN" if nxn else "2Nx2N")
            for (xp, yp, w, h) in hw.partitions(part, x, y, n):
                self.pv[yp >> 2:(yp + h) >> 2, xp >> 2] = True
                self.ph[yp >> 2, xp >> 2:(xp + w) >> 2] = True
            tu = u.get("tu", 1 if nxn else 0) if t in ("intra", "inter") else 0
            tus = hw.unit_tus(u, 4 ** tu) if t in ("intra", "inter") else [None]
            if t == "inter" and not any(e[c] for e in tus for c in (0, 1, 2)):
                tu, tus = 0, [None]                                 # rqt_root_cbf 0: no transform tree
            m = n >> tu
            for i, e in enumerate(tus):
                ox, oy = ir.tu_origin(i, tu, log2) if tu else (0, 0)
                b = (slice((y + oy) >> 2, (y + oy + m) >> 2), slice((x + ox) >> 2, (x + ox + m) >> 2))
                self.tv[b[0], (x + ox) >> 2] = True
                self.th[(y + oy) >> 2, b[1]] = True
                self.cbf[b] = bool(e and e[0])
            if t in ("skip", "inter") and field is None:            # the units of tests/hevc_resid_ref.py: a skipped unit has the zero vector on index 0
                if t == "skip":
                    mv = [(pl["l0"][0], (0, 0))] + ([(pl["l1"][0], (0, 0))] if p["kind"] == "B" else [])
                else:
                    mv = [(q[0], tuple(q[1])) for q in (u.get("l0"), u.get("l1")) if q]
                for j in range(y >> 2, (y + n) >> 2):
                    for i in range(x >> 2, (x + n) >> 2):
                        self.mot[(j, i)] = mv
        if field is not None:
            poc_pic = {pics[i]["poc"]: i for i in set(pl["l0"]) | set(pl["l1"])}
            for j in range(h4):
                for i in range(w4):
                    pf = int(field.pf[j, i])
                    self.mot[(j, i)] = [(poc_pic[int(field.poc[j, i, l])], (int(field.mv[j, i, l, 0]), int(field.mv[j, i, l, 1]))) for l in (0, 1) if pf > 0 and (pf >> l) & 1]

    def slice_at(self, x, y):
        return self.slices[self.slice_no[(y >> self.ctb) * self.cw + (x >> self.ctb)]]

    def slice_number(self, x, y):
        return int(self.slice_no[(y >> self.ctb) * self.cw + (x >> self.ctb)])

    # ---- 8.7.2.4
    def strength(self, xq, yq, xp, yp, transform_edge):
        """-> (bS, the rule that gave it, for two vectors on one picture dict(straight=, crossed=) with the (|dx|, |dy|) of both pairs of each pairing, else None)"""
        jq, iq, jp, ip = yq >> 2, xq >> 2, yp >> 2, xp >> 2
        if self.intra[jq, iq] or self.intra[jp, ip]:
            return 2, "intra:" + ("both" if self.intra[jq, iq] and self.intra[jp, ip] else "q" if self.intra[jq, iq] else "p"), None
        if transform_edge and (self.cbf[jq, iq] or self.cbf[jp, ip]):
            return 1, "cbf:" + ("both" if self.cbf[jq, iq] and self.cbf[jp, ip] else "q" if self.cbf[jq, iq] else "p"), None
        a, b = self.mot[(jp, ip)], self.mot[(jq, iq)]
        far = lambda u, v: abs(u[0] - v[0]) >= 4 or abs(u[1] - v[1]) >= 4
        gap = lambda u, v: "%d,%d" % (abs(u[0] - v[0]), abs(u[1] - v[1]))
        worst = lambda *pairs: max((gap(u, v) for u, v in pairs), key=lambda g: max(map(int, g.split(","))))
        if len(a) != len(b):
            return 1, "count", None
        if sorted(r for r, _ in a) != sorted(r for r, _ in b):
            return 1, "pictures", None
        if len(a) == 1:
            return (1, "one:far:" + gap(a[0][1], b[0][1]), None) if far(a[0][1], b[0][1]) else (0, "one:near:" + gap(a[0][1], b[0][1]), None)
        if a[0][0] != a[1][0]:                                      # two pictures: the vectors of the same picture
            b_ = b if b[0][0] == a[0][0] else b[::-1]
            tag = "two:" + ("straight" if b_ is b else "crossed")
            g = worst((a[0][1], b_[0][1]), (a[1][1], b_[1][1]))
            return (1, tag + ":far:" + g, None) if far(a[0][1], b_[0][1]) or far(a[1][1], b_[1][1]) else (0, tag + ":near:" + g, None)
        straight = far(a[0][1], b[0][1]) or far(a[1][1], b[1][1])
        crossed = far(a[0][1], b[1][1]) or far(a[1][1], b[0][1])
        tail = ":" + worst((a[0][1], b[0][1]), (a[1][1], b[1][1])) + ":" + worst((a[0][1], b[1][1]), (a[1][1], b[0][1]))      # straight, crossed
        diff = lambda u, v: (abs(u[0] - v[0]), abs(u[1] - v[1]))
        pairs = dict(straight=[diff(a[0][1], b[0][1]), diff(a[1][1], b[1][1])], crossed=[diff(a[0][1], b[1][1]), diff(a[1][1], b[0][1])])
        if straight and crossed:
            return 1, "same:both far" + tail, pairs
        return 0, "same:" + ("straight near" if not straight and crossed else "crossed near" if straight else "both near") + tail, pairs


def deblock(M, planes, k, records):
    """8.7.2 on the planes of picture k, in place"""
    sw, W, H = M.sw, M.W, M.H
    grid = 4 if sw.get("edges_on_4_grid") else 8
    pcm_off = M.seq.get("pcm_loop_filter_disabled", 1)
    cgrid = 8 if sw.get("chroma_on_luma_grid") else 16               # in luma samples
    offs = [M.seq.get("cb_qp_offset", 0), M.seq.get("cr_qp_offset", 0)]
    if sw.get("chroma_uses_slice_qp_offset"):
        offs = [offs[0] + M.p.get("cb_qp_offset", 0), offs[1] + M.p.get("cr_qp_offset", 0)]

    def segments(vertical):
        for y in range(0, H, 4):
            for x in range(0, W, 4):
                e, o = (x, y) if vertical else (y, x)
                if e == 0 or e % grid:
                    continue
                j, i = y >> 2, x >> 2
                te, pe = (M.tv[j, i], M.pv[j, i]) if vertical else (M.th[j, i], M.ph[j, i])
                if not (te or pe):
                    continue
                xp, yp = (x - 1, y) if vertical else (x, y - 1)
                sq, sp = M.slice_at(x, y), M.slice_at(xp, yp)
                off = None
                if (sp if sw.get("disabled_by_p_slice") else sq)["disabled"]:
                    off = "disabled"
                elif sq is not sp and not (sp if sw.get("across_flag_of_earlier_slice") else sq)["across"]:
                    off = "slice"
                bs, why, pairs = M.strength(x, y, xp, yp, bool(te))
                yield x, y, xp, yp, sq, sp, off, bs, (why, pairs), bool(te), bool(pe)

    def one_direction(vertical):
        Y = planes[0]
        todo = list(segments(vertical))
        for (x, y, xp, yp, sq, sp, off, bs, why, te, pe) in todo:
            jq, iq, jp, ip = y >> 2, x >> 2, yp >> 2, xp >> 2
            why, pairs = why
            rec = dict(pic=k, kind="luma", vertical=vertical, x=x, y=y, bs=bs, why=why, pairs=pairs, off=off, transform=te, prediction=pe, cu_edge=M.cu[jq, iq] != M.cu[jp, ip],
                       slices=(M.slice_number(xp, yp), M.slice_number(x, y)), qp=(int(M.qp[jp, ip]), int(M.qp[jq, iq])),
                       units=(M.units[M.cu[jp, ip]], M.units[M.cu[jq, iq]]), ctb=M.ctb)
            records.append(rec)
            if off or not bs:
                continue
            so = sp if sw.get("offsets_of_p_slice") else sq
            qpl = (int(M.qp[jq, iq]) + int(M.qp[jp, ip]) + (0 if sw.get("qp_sum_without_plus_1") else 1)) >> 1
            qb = clip3(0, 51, qpl + (so["beta"] << 1))
            qt = clip3(0, 53, qpl + (0 if sw.get("tc_without_bs_term") else 2 * (bs - 1)) + (so["tc"] << 1))
            beta, tc = BETA[qb], TC[qt]
            np_ = 0 if (pcm_off and M.pcm[jp, ip]) or M.bypass[jp, ip] else 3
            nq_ = 0 if (pcm_off and M.pcm[jq, iq]) or M.bypass[jq, iq] else 3
            rec.update(qpl=qpl, q_beta=qb, q_tc=qt, q_beta_raw=qpl + (so["beta"] << 1), q_tc_raw=qpl + 2 * (bs - 1) + (so["tc"] << 1), beta_off=so["beta"], tc_off=so["tc"],
                       exempt=(np_ == 0, nq_ == 0), pcm=(bool(M.pcm[jp, ip]), bool(M.pcm[jq, iq])), bypass=(bool(M.bypass[jp, ip]), bool(M.bypass[jq, iq])))
            if vertical:
                P = [[int(Y[y + l, x - 1 - s]) for s in range(4)] for l in range(4)]
                Q = [[int(Y[y + l, x + s]) for s in range(4)] for l in range(4)]
            else:
                P = [[int(Y[y - 1 - s, x + l]) for s in range(4)] for l in range(4)]
                Q = [[int(Y[y + s, x + l]) for s in range(4)] for l in range(4)]
            dec, new_p, new_q = luma_segment(P, Q, beta, tc, sw)
            changed = 0
            rec.update(dec)
            for l in range(4):
                np2, nq2 = new_p[l], new_q[l]
                for s in range(3):
                    for (new, old, keep, (sx, sy)) in ((np2[s], P[l][s], np_, ((x - 1 - s, y + l) if vertical else (x + l, y - 1 - s))),
                                                       (nq2[s], Q[l][s], nq_, ((x + s, y + l) if vertical else (x + l, y + s)))):
                        if keep and new != old:
                            Y[sy, sx] = new
                            changed += 1
            rec.update(changed=changed)
        # ---- chroma: 8.7.2.5.5, the edges of the 8-sample chroma grid with bS 2 (or what a switch makes of it)
        for (x, y, xp, yp, sq, sp, off, bs, why, te, pe) in todo:
            e, o = (x, y) if vertical else (y, x)
            if off or bs < (1 if sw.get("chroma_at_bs1") else 2) or e % cgrid or o % 8:
                continue                                            # a chroma segment is 4 chroma samples = 8 luma samples long and takes the bS at its first sample
            jq, iq, jp, ip = y >> 2, x >> 2, yp >> 2, xp >> 2
            so = sp if sw.get("offsets_of_p_slice") else sq
            qpl = (int(M.qp[jq, iq]) + int(M.qp[jp, ip]) + (0 if sw.get("qp_sum_without_plus_1") else 1)) >> 1
            np_ = not ((pcm_off and M.pcm[jp, ip]) or M.bypass[jp, ip])
            nq_ = not ((pcm_off and M.pcm[jq, iq]) or M.bypass[jq, iq])
            for c in (1, 2):
                qpi = qpl + offs[c - 1]
                qt = clip3(0, 53, qpc_of(qpi) + 2 * (bs - 1) + (so["tc"] << 1))
                tc = TC[qt]
                C = planes[c]
                hit, changed = set(), 0
                cx, cy = x >> 1, y >> 1
                for l in range(4):
                    if vertical:
                        pp, qq = [(cx - 1 - s, cy + l) for s in range(2)], [(cx + s, cy + l) for s in range(2)]
                    else:
                        pp, qq = [(cx + l, cy - 1 - s) for s in range(2)], [(cx + l, cy + s) for s in range(2)]
                    if qq[0][0] >= W // 2 or qq[0][1] >= H // 2:
                        continue
                    p0, q0 = chroma_line([int(C[b, a]) for a, b in pp], [int(C[b, a]) for a, b in qq], tc, hit)
                    for (new, (sx, sy), keep) in ((p0, pp[0], np_), (q0, qq[0], nq_)):
                        if keep and new != C[sy, sx]:
                            C[sy, sx] = new
                            changed += 1
                records.append(dict(pic=k, kind="chroma", plane=c, vertical=vertical, x=x, y=y, bs=bs, qpl=qpl, qpi=qpi, qpc=qpc_of(qpi), q_tc=qt, tc=tc, hit=hit,
                                    changed=changed, exempt=(not np_, not nq_), tc_off=so["tc"], off=None, slices=(M.slice_number(xp, yp), M.slice_number(x, y))))
    for vertical in ((False, True) if sw.get("horizontal_before_vertical") else (True, False)):
        one_direction(vertical)


def sao_params(M):
    """[per CTB address: [per component: None | ("band", position, offsets) | ("edge", class, magnitudes)]]: merges followed, slice flags applied"""
    out = []
    script = M.p.get("sao_ctbs") or [None] * (M.cw * M.ch)
    for a in range(M.cw * M.ch):
        e = script[a] or {}
        sl = M.slices[M.slice_no[a]]
        if e.get("merge") == "left":
            out.append(out[a - 1])
        elif e.get("merge") == "up":
            out.append(out[a - M.cw])
        else:
            cb, cr = e.get("c") or (None, None)
            out.append([e.get("y") if sl["sao"][0] else None, cb if sl["sao"][1] else None, cr if sl["sao"][1] else None])
    return out


def sao(M, planes, k, records):
    """8.7.3 -> new planes"""
    sw = M.sw
    if not M.seq.get("sao", 0):
        return planes
    params = sao_params(M)
    pcm_off = M.seq.get("pcm_loop_filter_disabled", 1)
    exempt4 = (M.pcm & bool(pcm_off)) | M.bypass
    if sw.get("sao_ignores_exempt_units"):
        exempt4 = np.zeros_like(exempt4)
    out = []
    for c in range(3):
        sh = 1 if c else 0
        src = planes[c] if sw.get("sao_in_place") else planes[c].copy()
        dst = planes[c] if sw.get("sao_in_place") else planes[c].copy()
        h, w = planes[c].shape
        size = (1 << M.ctb) >> sh
        for a in range(M.cw * M.ch):
            ent = params[a][c]
            if ent is None:
                continue
            typ, where, offs = ent
            if typ == "edge" and c == 2 and sw.get("cr_own_class"):
                where = (where + 1) & 3                             # (wrong on purpose: a class that is not Cb's)
            x0, y0 = (a % M.cw) * size, (a // M.cw) * size
            counts, sat, blocked = {}, set(), set()
            table = band_table(where, sw) if typ == "band" else None
            vals = [0] + list(offs) if typ == "band" else edge_values(offs, sw)
            me = int(M.slice_no[a])
            for y in range(y0, min(y0 + size, h)):
                for x in range(x0, min(x0 + size, w)):
                    if exempt4[(y << sh) >> 2, (x << sh) >> 2]:
                        blocked.add("exempt")
                        continue
                    v = int(src[y, x])
                    if typ == "band":
                        idx = table[v >> 3]
                    else:
                        nb = []
                        for (hp, vp) in SAO_POS[where]:
                            xn, yn = x + hp, y + vp
                            if not (0 <= xn < w and 0 <= yn < h):
                                if sw.get("sao_at_picture_border"):
                                    xn, yn = clip3(0, w - 1, xn), clip3(0, h - 1, yn)
                                else:
                                    blocked.add("picture")
                                    nb = None
                                    break
                            other = M.slice_number(xn << sh, yn << sh)
                            if other != me:
                                later = min(me, other) if sw.get("sao_flag_of_earlier_slice") else max(me, other)
                                if not M.slices[later]["across"]:
                                    blocked.add("slice:%+d%+d:%s" % (hp, vp, "own" if later == me else "other"))
                                    nb = None
                                    break
                                blocked.add("across:%+d%+d" % (hp, vp))
                            nb.append(int(src[yn, xn]))
                        if nb is None:
                            continue
                        idx = edge_idx(v, nb[0], nb[1], sw)
                    counts[idx] = counts.get(idx, 0) + 1
                    r = v + vals[idx]
                    if not 0 <= r <= 255:
                        sat.add("<0" if r < 0 else ">255")
                    dst[y, x] = clip3(0, 255, r)
            records.append(dict(pic=k, kind="sao", plane=c, ctb=a, x=x0 << sh, y=y0 << sh, type=typ, where=where, offsets=tuple(offs), counts=counts, sat=sat,
                                blocked=blocked, merged=((M.p.get("sao_ctbs") or [None] * (a + 1))[a] or {}).get("merge"), slice=me,
                                changed=int((dst[y0:y0 + size, x0:x0 + size] != planes[c][y0:y0 + size, x0:x0 + size]).sum()) if not sw.get("sao_in_place") else None))
        out.append(dst)
    return out


def uses_inter_ref(pics):
    """tests/hevc_inter_ref.py derives the motion of partitioned and merged units; every other unit is tests/hevc_resid_ref.py's"""
    def leaves(node):
        if node is None:
            return
        if node["t"] == "split":
            for s in node["sub"]:
                yield from leaves(s)
        else:
            yield node
    return any("pus" in u or (u["t"] == "skip" and "merge" in u) for p in pics for n in p["cus"] for u in leaves(n))


def expect(seq, pics, **sw):
    """-> ([(Y, Cb, Cr)] per picture in DECODE order, coded size, uint8; records)"""
    assert all(k in SWITCHES for k in sw), sw
    plans = hw.plan(seq, pics)
    records, shown = [], {}

    def post(k, planes, ctx):
        M = Maps(seq, pics, k, plans, ctx, sw)
        before = [pl.copy() for pl in planes]
        work = [pl.copy() for pl in planes]
        if sw.get("sao_before_deblock"):
            work = sao(M, work, k, records)
            deblock(M, work, k, records)
        else:
            deblock(M, work, k, records)
            work = sao(M, work, k, records)
        shown[k] = tuple(work)
        return tuple(before) if sw.get("reference_is_unfiltered") else tuple(work)
    base = hr if uses_inter_ref(pics) else rr
    base.expect(seq, pics, post=post)
    return [shown[k] for k in range(len(pics))], records


def describe(r):
    if r["kind"] == "sao":
        return (f"SAO of picture {r['pic']} plane {('Y', 'Cb', 'Cr')[r['plane']]} CTB {r['ctb']} at luma ({r['x']}, {r['y']}): {r['type']} {r['where']} offsets {r['offsets']} "
                f"categories {r['counts']} left alone for {sorted(r['blocked'])}")
    if r["kind"] == "chroma":
        return (f"chroma edge of picture {r['pic']} plane {('Y', 'Cb', 'Cr')[r['plane']]} {'vertical' if r['vertical'] else 'horizontal'} at luma ({r['x']}, {r['y']}): "
                f"qPi {r['qpi']} QpC {r['qpc']} tC {r['tc']}")
    return (f"luma edge of picture {r['pic']} {'vertical' if r['vertical'] else 'horizontal'} at ({r['x']}, {r['y']}): bS {r['bs']} ({r['why']}) off {r['off']} "
            + (f"qPL {r['qpl']} beta {r['beta']} tC {r['tc']} d {r['d']} dE {r['dE']} dEp {r['dEp']} dEq {r['dEq']}" if "qpl" in r else ""))


def difference(seq, pics, frames, fmt, planes, records):
    """None when the display frames are the expected pictures, else a text that names the first picture, plane and sample that is wrong and the records
    of the edge segments and the CTB next to it"""
    if len(frames) != len(pics):
        return f"{len(frames)} frames, the script has {len(pics)}"
    w, h = seq["width"], seq["height"]
    ctb = 1 << hw.geometry(seq)["ctb"]
    order = sorted(range(len(pics)), key=lambda k: pics[k]["poc"])
    for d, k in enumerate(order):
        got = ir.unpack(seq, frames[d], fmt)
        for c in range(3):
            want = planes[k][c][:h >> (c > 0), :w >> (c > 0)]
            if np.array_equal(want, got[c]):
                continue
            j = np.argwhere(want != got[c])[0]
            X, Y = int(j[1]) << (c > 0), int(j[0]) << (c > 0)
            near = []
            for r in records:
                if r["pic"] != k:
                    continue
                if r["kind"] == "sao":
                    if r["plane"] == c and r["x"] <= X < r["x"] + ctb and r["y"] <= Y < r["y"] + ctb:
                        near.append(describe(r))
                elif (r["kind"] == "luma") == (c == 0) and r.get("plane", 0) == c:
                    reach = 8 if c else 4
                    inside = (abs(X - r["x"]) <= reach and r["y"] <= Y < r["y"] + reach) if r["vertical"] else (abs(Y - r["y"]) <= reach and r["x"] <= X < r["x"] + reach)
                    if inside:
                        near.append(describe(r))
            return (f"picture {k} ({pics[k]['kind']}, POC {pics[k]['poc']}) plane {('Y', 'Cb', 'Cr')[c]} sample ({j[1]}, {j[0]}): got {got[c][j[0], j[1]]} expected "
                    f"{want[j[0], j[1]]}, {int((want != got[c]).sum())} samples of the plane differ; near: " + ("; ".join(near[:6]) or "no edge and no SAO"))
    return None
