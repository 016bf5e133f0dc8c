"""H.264 clause 8.7 for the frame pictures of the scripted streams (tests/scripted_h264.py), typed out: macroblock by macroblock in raster order, per
macroblock the vertical edges left to right, then the horizontal edges top to bottom, luma and both chroma planes.  Plain Python on lists: it is meant to
be read beside the clause, not to be fast.  Tables come from tests/spec_tables_h264.py only.

What the script knows decides everything: bS (8.7.2.1) from the macroblock types, the luma 4x4 blocks that carry levels (under the 8x8 transform all
four blocks of a coded 8x8; scripted_h264.coded_luma_blocks) and the vectors and reference PICTURES of the 4x4 blocks; transform_size_8x8_flag leaves
the inner 4x4 edges alone; qPp / qPq per macroblock (I_PCM counts 0); chroma through QPC with the plane's own offset (chroma_qp_index_offset for Cb,
second_chroma_qp_index_offset for Cr), each side mapped before the average; FilterOffsetA / B and disable_deblocking_filter_idc of the slice that
holds q0; idc 2 leaves slice edges alone; the left and top picture edges are never filtered.

``stats`` (a dict of counters, keyed "<plane><direction>:<what>" with plane Y / C and direction V / H (vertical / horizontal EDGES)) records which paths
of the clause the pictures took; tests/test_analytic_host.py asserts from them that the filtering cases really filter on every path."""
import h264_field_ref as fr
import scripted_h264 as sw
from spec_tables_h264 import ALPHA, BETA, QPC_30_51, TC0


def clip3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


def qpc(qpy, off):
    """8.5.8 / Table 8-15 as 8.7.2.2 uses it: QPC of the macroblock's QPY"""
    qpi = clip3(0, 51, qpy + off)
    return qpi if qpi < 30 else QPC_30_51[qpi - 30]


def block_motion(m, bx, by, skip_ref):
    """[(reference picture, vector)] of the 4x4 block at (bx, by) of inter macroblock m: one entry per vector in use"""
    t = m["t"]
    if "blocks" in m:                                               # motion derived from the syntax (tests/h264_motion_ref.py): one entry per 4x4 block
        return [q for q in m["blocks"][(by // 4) * 4 + bx // 4] if q is not None]
    if t == "skip":
        return [(skip_ref, (0, 0))]
    if t == "16x16":
        return [q for q in (m.get("l0"), m.get("l1")) if q is not None]
    return [m["parts"][int(by >= 8 if t == "16x8" else bx >= 8)]]


def motion_bs(P, Q, ylimit=4):
    """The last two bullets of 8.7.2.1 that give bS 1: P, Q = block_motion of the two blocks.  ylimit: 4 for frame macroblocks; in a field picture
    the vertical component counts quarter FIELD samples and the limit of 4 quarter frame samples is h264_field_ref.FIELD_MVY_LIMIT."""
    def far(a, b):
        """a vector component differs by >= 4 in quarter luma frame samples"""
        return abs(a[0] - b[0]) >= 4 or abs(a[1] - b[1]) >= ylimit
    if len(P) != len(Q) or sorted(pic for pic, _ in P) != sorted(pic for pic, _ in Q):
        return 1                                                    # different reference pictures or a different number of motion vectors
    if len(P) == 1:
        return int(far(P[0][1], Q[0][1]))
    if P[0][0] != P[1][0]:                                          # two vectors, two different pictures: compare the vectors that use the same picture
        q = dict(Q)
        return int(any(far(mv, q[pic]) for pic, mv in P))
    # both vectors of both blocks use the same picture: bS 1 only when neither pairing of the vectors is close in both
    straight = far(P[0][1], Q[0][1]) or far(P[1][1], Q[1][1])
    cross = far(P[0][1], Q[1][1]) or far(P[1][1], Q[0][1])
    return int(straight and cross)


def filter_line(s, bS, alpha, beta, tc0, chroma, cnt, key):
    """8.7.2.2 - 8.7.2.4 on one line: s = [p3, p2, p1, p0, q0, q1, q2, q3] (chroma: [p1, p0, q0, q1]); returns the filtered line.  tc0 = tC0' (bS < 4)."""
    def hit(name):
        cnt[key + name] = cnt.get(key + name, 0) + 1
    if chroma:
        p1, p0, q0, q1 = s
        p2 = q2 = p3 = q3 = 0
    else:
        p3, p2, p1, p0, q0, q1, q2, q3 = s
    ta, tp, tq = abs(p0 - q0) < alpha, abs(p1 - p0) < beta, abs(q1 - q0) < beta
    if not (bS != 0 and ta and tp and tq):                          # filterSamplesFlag (8-468)
        if bS != 0:
            hit("off_lt4" if bS < 4 else "off_4")
            if not ta and tp and tq:
                hit("off_alpha_only")
            if ta and not tp and tq:
                hit("off_beta_p_only")
            if ta and tp and not tq:
                hit("off_beta_q_only")
        return list(s)
    hit("on_bS%d" % bS)
    hit("on_lt4" if bS < 4 else "on_4")
    np0, np1, np2, nq0, nq1, nq2 = p0, p1, p2, q0, q1, q2
    ap, aq = abs(p2 - p0), abs(q2 - q0)
    if bS < 4:                                                      # 8.7.2.3
        if chroma:
            tc = tc0 + 1                                            # (8-474)
        else:
            tc = tc0 + (1 if ap < beta else 0) + (1 if aq < beta else 0)      # (8-473)
            hit("ap%d_aq%d" % (ap < beta, aq < beta))
        raw = (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3
        delta = clip3(-tc, tc, raw)                                 # (8-475)
        hit("delta_clip_pos" if raw > tc else ("delta_clip_neg" if raw < -tc else "delta_unclipped"))
        for v in (p0 + delta, q0 - delta):
            if v < 0:
                hit("clip1_at_0")
            if v > 255:
                hit("clip1_at_255")
        np0, nq0 = clip3(0, 255, p0 + delta), clip3(0, 255, q0 - delta)      # (8-476), (8-477)
        if not chroma and ap < beta:
            np1 = p1 + clip3(-tc0, tc0, (p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1)      # (8-478)
        if not chroma and aq < beta:
            nq1 = q1 + clip3(-tc0, tc0, (q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1)      # (8-480)
    else:                                                           # 8.7.2.4
        small = abs(p0 - q0) < ((alpha >> 2) + 2)
        sp, sq = not chroma and ap < beta and small, not chroma and aq < beta and small
        if not chroma:
            hit("strong_both" if sp and sq else ("strong_p" if sp else ("strong_q" if sq else "strong_neither")))
        if sp:
            np0 = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3      # (8-485)
            np1 = (p2 + p1 + p0 + q0 + 2) >> 2
            np2 = (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3
        else:
            np0 = (2 * p1 + p0 + q1 + 2) >> 2                       # (8-488)
        if sq:
            nq0 = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3      # (8-492)
            nq1 = (p0 + q0 + q1 + q2 + 2) >> 2
            nq2 = (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3
        else:
            nq0 = (2 * q1 + q0 + p1 + 2) >> 2                       # (8-495)
    return [p1, np0, nq0, q1] if chroma else [p3, np2, np1, np0, nq0, nq1, nq2, q3]


def mb_table(seq, pics, pl, k):
    """Per macroblock of picture k what 8.7 needs: intra, QPY, slice (its first macroblock), (idc, FilterOffsetA, FilterOffsetB), the 4x4 blocks with a
    coefficient, and the macroblock itself for its motion."""
    p = pics[k]
    step, qps = sw.layout_step(seq, p), sw.mb_qps(seq, p)
    out = []
    for a, m in enumerate(p["mbs"]):
        first = a - a % step
        idc, ao, bo = sw.slice_fields(seq, p, step, p["mbs"][first])[1]
        # 8.7.2.2: qPp = 0 for an I_PCM macroblock
        # the luma 4x4 blocks that count as holding coefficients (under the 8x8 transform: all four of a coded 8x8) and transform_size_8x8_flag
        out.append(dict(m=m, intra=m["t"] in sw.INTRA, qp=0 if m["t"] == "pcm" else qps[a], slice=first, idc=idc, off_a=2 * ao, off_b=2 * bo,
                        coef=sw.coded_luma_blocks(m), t8=m["t"] == "i8" or bool(m.get("t8", 0) and sw.coded_luma_blocks(m))))
    return out


def deblock_picture(seq, pics, pl, k, planes, stats=None, wrong=frozenset()):
    """planes = (Y, Cb, Cr) of picture k as reconstructed (uint8 arrays); returns the three planes after 8.7, and counts into stats.  A field picture is
    filtered as a picture of its own (seq = scripted_h264.pic_seq: its macroblocks, its lines only, nothing across its top edge) under the field
    rules of 8.7.2.1 (tests/h264_field_ref.py); wrong: that module's switches."""
    field = bool(pics[k].get("field"))
    ylimit, refkey = fr.mvy_limit(field, wrong), fr.reference_key(pics, field, wrong)
    import numpy as np
    cnt = stats if stats is not None else {}
    mbw, mbh = (seq["width"] + 15) // 16, (seq["height"] + 15) // 16
    info = mb_table(seq, pics, pl, k)
    if all(q["idc"] == 1 for q in info):
        return planes
    off_c = seq.get("chroma_qp_off", 0)
    off_cr = seq.get("second_chroma_qp_off", off_c)                 # 8.7.2.2: each chroma plane with its own offset
    skip_ref = pl[k]["l0"][0] if pl[k]["l0"] else None
    S = [pl_.astype(np.int64).tolist() for pl_ in planes]
    blk_at = {xy: i for i, xy in enumerate(sw.BLK_XY)}

    def hit(name, n=1):
        cnt[name] = cnt.get(name, 0) + n

    for a, q in enumerate(info):
        mx, my = a % mbw, a // mbw
        if q["idc"] == 1:
            continue
        for d, D in ((0, "V"), (1, "H")):                           # vertical edges first, then horizontal
            nb = (info[a - 1] if mx > 0 else None) if d == 0 else (info[a - mbw] if my > 0 else None)
            for e in range(4):
                pmb = q
                if q["t8"] and e % 2 == 1:
                    continue                                        # transform_size_8x8_flag: the inner 4x4 edges are not filtered (chroma has none there)
                if e == 0:
                    if nb is None:
                        continue                                    # picture edge
                    if q["idc"] == 2 and nb["slice"] != q["slice"]:
                        hit(D + ":idc2_slice_edge_left_alone")
                        continue
                    pmb = nb
                # ---- per edge: thresholds.  qPp is the p macroblock's QPY (0 for I_PCM); offsets of the slice that holds q0 ----
                qpav = (pmb["qp"] + q["qp"] + 1) >> 1
                ia, ib = qpav + q["off_a"], qpav + q["off_b"]
                lum = (ALPHA[clip3(0, 51, ia)], BETA[clip3(0, 51, ib)], TC0[clip3(0, 51, ia)])
                chr_of = {}
                for c, off in ((1, off_c), (2, off_cr)):
                    cav = (qpc(pmb["qp"], off) + qpc(q["qp"], off) + 1) >> 1
                    ica, icb = cav + q["off_a"], cav + q["off_b"]
                    chr_of[c] = (ALPHA[clip3(0, 51, ica)], BETA[clip3(0, 51, icb)], TC0[clip3(0, 51, ica)])
                edge_on = {"Y": 0, "C": 0}
                edge_bs = 0
                for seg in range(4):
                    # ---- 8.7.2.1: bS of the four lines of this segment ----
                    qb = (4 * e, 4 * seg) if d == 0 else (4 * seg, 4 * e)
                    pb = ((qb[0] - 4) % 16, qb[1]) if d == 0 else (qb[0], (qb[1] - 4) % 16)
                    maxdiff = None
                    if e == 0 and (pmb["intra"] or q["intra"]):
                        bS = fr.intra_edge_bs(field, d == 1, wrong)
                        if field and d == 1:
                            hit("H:field_intra_mb_edge_bS%d" % bS)
                    elif pmb["intra"] or q["intra"]:
                        bS = 3
                    elif blk_at[pb] in pmb["coef"] or blk_at[qb] in q["coef"]:
                        bS = 2
                    else:
                        P, Q = block_motion(pmb["m"], pb[0], pb[1], skip_ref), block_motion(q["m"], qb[0], qb[1], skip_ref)
                        P, Q = [(refkey(r), mv) for r, mv in P], [(refkey(r), mv) for r, mv in Q]
                        bS = motion_bs(P, Q, ylimit)
                        if field and len(P) == 1 and len(Q) == 1:
                            if P[0][0] == Q[0][0] and abs(P[0][1][0] - Q[0][1][0]) < 4:
                                hit("field_mvy_differs_by_%d_bS%d" % (abs(P[0][1][1] - Q[0][1][1]), bS))
                            elif P[0][0] != Q[0][0] and fr.structure(pics)[fr.field_of(pics, P[0][0])[0]][0] == fr.structure(pics)[fr.field_of(pics, Q[0][0])[0]][0]:
                                hit("field_refs_are_the_two_fields_of_one_frame_bS%d" % bS)
                        if len(P) == 1 and len(Q) == 1 and P[0][0] == Q[0][0]:
                            maxdiff = max(abs(P[0][1][0] - Q[0][1][0]), abs(P[0][1][1] - Q[0][1][1]))
                    edge_bs = max(edge_bs, bS)
                    if bS == 0:
                        if e == 0 and maxdiff == 3:
                            hit(D + ":mb_edge_vectors_differ_by_3_bS0")
                        continue
                    # ---- luma: four lines ----
                    for i in range(4 * seg, 4 * seg + 4):
                        x0, y0 = mx * 16, my * 16
                        pos = [(x0 + 4 * e + j, y0 + i) for j in range(-4, 4)] if d == 0 else [(x0 + i, y0 + 4 * e + j) for j in range(-4, 4)]
                        line = [S[0][y][x] for x, y in pos]
                        new = filter_line(line, bS, lum[0], lum[1], lum[2][bS - 1] if bS < 4 else 0, False, cnt, "Y" + D + ":")
                        if new != line:
                            edge_on["Y"] += 1
                            for (x, y), v in zip(pos, new):
                                S[0][y][x] = v
                    # ---- chroma: edges 0 and 2 are the chroma edges 0 and 4; chroma line j takes the bS of luma line 2 j ----
                    if e % 2 == 0:
                        for c in (1, 2):
                            chr_ = chr_of[c]
                            for j in range(2 * seg, 2 * seg + 2):
                                x0, y0 = mx * 8, my * 8
                                pos = [(x0 + 2 * e + t, y0 + j) for t in range(-2, 2)] if d == 0 else [(x0 + j, y0 + 2 * e + t) for t in range(-2, 2)]
                                line = [S[c][y][x] for x, y in pos]
                                new = filter_line(line, bS, chr_[0], chr_[1], chr_[2][bS - 1] if bS < 4 else 0, True, cnt, "C" + D + ":")
                                if new != line:
                                    edge_on["C"] += 1
                                    for (x, y), v in zip(pos, new):
                                        S[c][y][x] = v
                    if e == 0 and maxdiff == 4 and bS == 1:
                        hit(D + ":mb_edge_vectors_differ_by_4_bS1")
                # ---- what this edge exercised (only edges on which a luma line was filtered count) ----
                if edge_bs and edge_on["Y"]:
                    for name, v in (("indexA", ia), ("indexB", ib)):
                        if v > 51:
                            hit(D + ":%s_clipped_at_51" % name)
                    if pmb["qp"] != q["qp"]:
                        hit(D + ":qPav_of_unequal_QPs")
                    if {pmb["qp"], q["qp"]} == {0, 51} and (pmb["m"]["t"] == "pcm" or q["m"]["t"] == "pcm"):
                        hit(D + ":qPav_of_I_PCM_and_51")
                    if e == 0 and pmb["slice"] != q["slice"] and q["idc"] == 0 and (pmb["off_a"], pmb["off_b"]) != (q["off_a"], q["off_b"]):
                        hit(D + ":idc0_slice_edge_filtered_with_q_offsets")
                if edge_bs:                                         # (alpha' and beta' are 0 there: such an edge is evaluated, never filtered)
                    for name, v in (("indexA", ia), ("indexB", ib)):
                        if v < 0:
                            hit(D + ":%s_clipped_at_0" % name)
                if edge_bs and edge_on["C"] and off_c != 0 and max(pmb["qp"], q["qp"]) + off_c >= 30:
                    hit(D + ":chroma_qp_from_table_with_offset")
    return tuple(np.array(pl_, dtype=np.uint8) for pl_ in S)


def woven_filter(frame_seq, pics, pl, k, store, raw_pair, wrong):
    """WRONG ON PURPOSE (h264_field_ref switch deblock_across_parities): what a decoder makes of a frame coded as two fields when it filters the woven
    frame instead of each field -- the unfiltered fields raw_pair = (picture k - 1, picture k) woven, filtered as a frame picture whose macroblock
    row r carries what the first field's macroblock row r / 2 carries.  Writes the store and returns the two fields as that decoder holds them."""
    import numpy as np
    first, mbw = pics[k - 1], (frame_seq["width"] + 15) // 16
    t, b = raw_pair if first["field"] == "top" else raw_pair[::-1]
    woven = tuple(fr.weave(x, y) for x, y in zip(t, b))
    rows = len(first["mbs"]) // mbw
    fake = dict({key: v for key, v in first.items() if key != "field"}, mbs=[first["mbs"][(r // 2) * mbw + x] for r in range(2 * rows) for x in range(mbw)])
    got = deblock_picture(frame_seq, pics[:k - 1] + [fake] + pics[k:], pl, k - 1, woven, None, frozenset(wrong) - {"deblock_across_parities"})
    for S, g in zip(store, got):
        S[:] = g
    tops, bots = tuple(g[0::2] for g in got), tuple(g[1::2] for g in got)
    return [tops, bots] if first["field"] == "top" else [bots, tops]
