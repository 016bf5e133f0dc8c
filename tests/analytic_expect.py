"""Expected pictures of the scripted H.264 streams (tests/scripted_h264.py), computed from the script alone: no decoder, generator or oracle is involved.

Sample interpolation is the literal restatement of 8.4.2.2.1 in tests/test_mc_packed.py (``luma_literal``), vectorised here (``mc_luma``; the host test
checks the vectorised form against the scalar one), and the chroma formula 8-270; weighted prediction is 8.4.2.3 typed out; Intra16x16 / chroma
prediction are 8.3.3 / 8.3.4 typed out.  The closed forms (ramps, half-sample chroma, flat fields) live beside them and are checked against these
restatements in tests/test_analytic_host.py before any stream relies on them.  Deblocking is clause 8.7 typed out in tests/deblock_ref.py, applied to
every finished picture before it serves as a reference (the identity cases choose streams on which it changes nothing; the deblock_filters_* cases
streams on which it changes most macroblocks).  A single DC coefficient of +-1 (resid=) is ``dc_only_residual``; Intra4x4 / Intra8x8 prediction and the
levels of coef=dict(...) are clauses 8.3.1, 8.3.2 and 8.5 typed out in tests/h264_recon_ref.py.
"""
import numpy as np

import deblock_ref
import h264_field_ref as fr
import h264_motion_ref as mr
import h264_recon_ref as rr
import scripted_h264 as sw
from spec_tables_h264 import NORM_ADJUST_4x4


def clip1(a):
    return np.clip(a, 0, 255)


def window(R, y0, x0, h, w):
    """R[y0 .. y0+h, x0 .. x0+w] with every coordinate clamped into the picture (8.4.2.2.1, equations 8-239 / 8-240; 8-266 .. 8-269 for chroma)."""
    if isinstance(R, fr.FieldRef):                                  # one parity of a store: its own clamp (the field's border) and line pitch
        return R.fetch(np.arange(y0, y0 + h), np.arange(x0, x0 + w))
    ys = np.clip(np.arange(y0, y0 + h), 0, R.shape[0] - 1)
    xs = np.clip(np.arange(x0, x0 + w), 0, R.shape[1] - 1)
    return R[np.ix_(ys, xs)].astype(np.int64)


def tap6(a, b, c, d, e, f):
    return a - 5 * b + 20 * c + 20 * d - 5 * e + f


def mc_luma(R, x0, y0, w, h, mv):
    """The w x h luma prediction at (x0, y0) for the quarter-sample vector mv: luma_literal of tests/test_mc_packed.py for every sample at once."""
    xi, yi, fx, fy = x0 + (mv[0] >> 2), y0 + (mv[1] >> 2), mv[0] & 3, mv[1] & 3
    P = window(R, yi - 2, xi - 2, h + 5, w + 5)
    b1 = tap6(*[P[:, k:k + w] for k in range(6)])                   # (h + 5, w): the horizontal sums of every row, dy = -2 .. 3
    h1 = tap6(*[P[k:k + h, :] for k in range(6)])                   # (h, w + 5): the vertical sums of every column, dx = -2 .. 3
    G, H, M = P[2:2 + h, 2:2 + w], P[2:2 + h, 3:3 + w], P[3:3 + h, 2:2 + w]
    b, s = clip1((b1[2:2 + h] + 16) >> 5), clip1((b1[3:3 + h] + 16) >> 5)
    hh, m = clip1((h1[:, 2:2 + w] + 16) >> 5), clip1((h1[:, 3:3 + w] + 16) >> 5)
    j = clip1((tap6(*[b1[k:k + h] for k in range(6)]) + 512) >> 10)
    avg = lambda p, q: (p + q + 1) >> 1
    table = {(0, 0): lambda: G, (1, 0): lambda: avg(G, b), (2, 0): lambda: b, (3, 0): lambda: avg(H, b),
             (0, 1): lambda: avg(G, hh), (1, 1): lambda: avg(b, hh), (2, 1): lambda: avg(b, j), (3, 1): lambda: avg(b, m),
             (0, 2): lambda: hh, (1, 2): lambda: avg(hh, j), (2, 2): lambda: j, (3, 2): lambda: avg(j, m),
             (0, 3): lambda: avg(M, hh), (1, 3): lambda: avg(hh, s), (2, 3): lambda: avg(j, s), (3, 3): lambda: avg(m, s)}
    return table[(fx, fy)]()


def mc_chroma(R, x0, y0, w, h, mv):
    """8.4.2.2.2 (8-270) on one chroma plane; (x0, y0) in chroma samples, the vector in eighth chroma samples (= the luma vector, 4:2:0 frames)."""
    xi, yi, fx, fy = x0 + (mv[0] >> 3), y0 + (mv[1] >> 3), mv[0] & 7, mv[1] & 7
    P = window(R, yi, xi, h + 1, w + 1)
    A, B, C, D = P[:h, :w], P[:h, 1:], P[1:, :w], P[1:, 1:]
    return ((8 - fx) * (8 - fy) * A + fx * (8 - fy) * B + (8 - fx) * fy * C + fx * fy * D + 32) >> 6


def implicit_weights(poc_cur, poc0, poc1):
    """8.4.2.3.1, implicit mode, frames, short-term references: (w0, w1); logWD is 5 and the offsets are 0."""
    c3 = lambda lo, hi, v: max(lo, min(hi, v))
    tb, td = c3(-128, 127, poc_cur - poc0), c3(-128, 127, poc1 - poc0)
    if td == 0:
        return 32, 32
    tx = int((16384 + abs(int(td / 2))) / td)                       # C division: towards zero
    w1 = c3(-1024, 1023, (tb * tx + 32) >> 6) >> 2
    if w1 < -64 or w1 > 128:
        return 32, 32
    return 64 - w1, w1


def weighted(p0, p1, mode, logwd, e0, e1):
    """8.4.2.3.1 / 8.4.2.3.2.  p0 / p1: the predictions of the lists in use (None: list not used); e0 / e1: (w, o) of the entry (explicit), or the
    implicit (w, 0)."""
    if mode == 0 or (mode == 2 and (p0 is None or p1 is None)):
        return p0 if p1 is None else (p1 if p0 is None else (p0 + p1 + 1) >> 1)                      # 8-271 .. 8-273
    if p0 is not None and p1 is not None:
        return clip1(((p0 * e0[0] + p1 * e1[0] + (1 << logwd)) >> (logwd + 1)) + ((e0[1] + e1[1] + 1) >> 1))          # 8-276
    p, (w, o) = (p0, e0) if p1 is None else (p1, e1)
    return clip1(((p * w + (1 << (logwd - 1))) >> logwd) + o) if logwd >= 1 else clip1(p * w + o)  # 8-274 / 8-275


def intra16_luma(Y, x0, y0, mode, al, at):
    """8.3.3.1 - 8.3.3.4.  al / at: left / upper macroblock available (the plane mode needs the corner too: the scripts only use it where it is)."""
    top = Y[y0 - 1, x0:x0 + 16].astype(np.int64) if at else None
    left = Y[y0:y0 + 16, x0 - 1].astype(np.int64) if al else None
    if mode == 0:
        return np.tile(top, (16, 1))
    if mode == 1:
        return np.tile(left[:, None], (1, 16))
    if mode == 2:
        if at and al:
            v = (top.sum() + left.sum() + 16) >> 5
        elif at or al:
            v = ((top if at else left).sum() + 8) >> 4
        else:
            v = 128
        return np.full((16, 16), v, np.int64)
    corner = int(Y[y0 - 1, x0 - 1])
    tp = lambda i: corner if i < 0 else int(top[i])
    lp = lambda i: corner if i < 0 else int(left[i])
    Hs = sum((k + 1) * (tp(8 + k) - tp(6 - k)) for k in range(8))
    Vs = sum((k + 1) * (lp(8 + k) - lp(6 - k)) for k in range(8))
    a, b, c = 16 * (lp(15) + tp(15)), (5 * Hs + 32) >> 6, (5 * Vs + 32) >> 6
    yy, xx = np.mgrid[0:16, 0:16]
    return clip1((a + b * (xx - 7) + c * (yy - 7) + 16) >> 5)


def intra_chroma(C, x0, y0, mode, al, at):
    """8.3.4.1 - 8.3.4.4 for 4:2:0 (one 8x8 chroma block)."""
    top = C[y0 - 1, x0:x0 + 8].astype(np.int64) if at else None
    left = C[y0:y0 + 8, x0 - 1].astype(np.int64) if al else None
    if mode == 2:
        return np.tile(top, (8, 1))
    if mode == 1:
        return np.tile(left[:, None], (1, 8))
    if mode == 0:
        out = np.zeros((8, 8), np.int64)
        for by in (0, 1):
            for bx in (0, 1):
                t = top[4 * bx:4 * bx + 4].sum() if at else None
                l = left[4 * by:4 * by + 4].sum() if al else None
                if (bx, by) == (1, 0):
                    pick = [t, l]                                   # the upper neighbours first, else the left ones
                elif (bx, by) == (0, 1):
                    pick = [l, t]
                else:
                    pick = [None if t is None or l is None else (t, l), t, l]
                v = next((q for q in pick if q is not None), None)
                out[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = 128 if v is None else ((v[0] + v[1] + 4) >> 3 if isinstance(v, tuple) else (v + 2) >> 2)
        return out
    corner = int(C[y0 - 1, x0 - 1])
    tp = lambda i: corner if i < 0 else int(top[i])
    lp = lambda i: corner if i < 0 else int(left[i])
    Hs = sum((k + 1) * (tp(4 + k) - tp(2 - k)) for k in range(4))
    Vs = sum((k + 1) * (lp(4 + k) - lp(2 - k)) for k in range(4))
    a, b, c = 16 * (lp(7) + tp(7)), (34 * Hs + 32) >> 6, (34 * Vs + 32) >> 6
    yy, xx = np.mgrid[0:8, 0:8]
    return clip1((a + b * (xx - 3) + c * (yy - 3) + 16) >> 5)


def dc_only_residual(qp, level):
    """What every sample of a 4x4 luma block gains when its only coefficient is c00 = level, flat scaling matrices, no transform bypass.
    8.5.12.1: LevelScale4x4(qP % 6, 0, 0) = 16 * normAdjust4x4(qP % 6, 0, 0) (8.5.9, Flat_4x4_16); d00 = (c00 * LevelScale) << (qP / 6 - 4) for qP >= 24,
    else (c00 * LevelScale + 2^(3 - qP / 6)) >> (4 - qP / 6).  8.5.12.2 with d00 alone: each one-dimensional transform of (d, 0, 0, 0) is (d, d, d, d)
    -- e0 = e1 = d, e2 = e3 = 0, f = (e0 + e3, e1 + e2, e1 - e2, e0 - e3) -- horizontally, then vertically on every column: h_ij = d00 everywhere, and
    r_ij = (h_ij + 32) >> 6 (8-354)."""
    ls = 16 * NORM_ADJUST_4x4[qp % 6][0]
    d = (level * ls) << (qp // 6 - 4) if qp >= 24 else (level * ls + (1 << (3 - qp // 6))) >> (4 - qp // 6)
    return (d + 32) >> 6


def partitions(m):
    """(x, y, w, h, l0, l1) of every partition of an inter macroblock of the script."""
    if m["t"] == "16x16":
        return [(0, 0, 16, 16, m.get("l0"), m.get("l1"))]
    (a, b) = m["parts"]
    return [(0, 0, 16, 8, a, None), (0, 8, 16, 8, b, None)] if m["t"] == "16x8" else [(0, 0, 8, 16, a, None), (8, 0, 8, 16, b, None)]


def expect_h264(seq, pics, stats=None, unfiltered=None, stale_ref_of=None, wrong=frozenset(), rstats=None, mcov=None):
    """[(Y, Cb, Cr)] per picture in DECODE order, coded size (multiples of 16), uint8.  stats: counters of deblock_ref; unfiltered: a list that receives
    each picture as reconstructed, before 8.7; stale_ref_of = k: picture k alone is predicted from the UNFILTERED picture k - 1 (what a decoder computes
    that reads its reference too early; the host test shows that this is visible).  wrong: wrong-on-purpose switches of tests/h264_recon_ref.py;
    rstats: a set that receives what the Intra4x4 / Intra8x8 blocks and the residuals exercised.
    A stream with field pictures (tests/h264_field_ref.py): a field picture's entry holds the field's own lines (half the rows); a reference name
    goes through the writer's list to an index and through the restated decoder's list back to a picture; the samples live in frame stores.
    A stream with macroblocks that state syntax, not motion (t="mv", skipped macroblocks among neighbours): their per-4x4 motion is derived by
    tests/h264_motion_ref.py (wrong: its switches too; mcov: a dict that receives its branch counts); every other form is handled as before."""
    frame_seq = seq
    pl = sw.plan(seq, pics)
    wrong = frozenset(wrong)
    lists = rr.scaling_matrices(seq, wrong)
    paff = fr.has_fields(pics)
    dec_lists = fr.decoder_lists(seq, pics, wrong) if paff else None
    st = fr.structure(pics)
    derived = None
    if any(sw.uses_new_forms(sw.pic_seq(seq, p), p) for p in pics):
        derived = mr.derive(seq, pics, pl, wrong & frozenset(mr.SWITCHES), mcov)[0]
    dpics = list(pics)                                              # for 8.7: the same pictures, the derived motion beside the syntax
    stores = {}                                                     # picture index -> the (Y, Cb, Cr) frame store it was written into
    out, raw = [], []
    for k, p in enumerate(pics):
        kind = p["kind"]
        parity = p.get("field")
        seq = sw.pic_seq(frame_seq, p)                              # a field is a picture of its own: neighbours, slices, QP chain inside the field
        mbw, mbh = (seq["width"] + 15) // 16, (seq["height"] + 15) // 16
        scans = fr.decoder_scans(bool(parity), wrong)
        if paff:
            cmbh = (frame_seq["height"] + 15) // 16
            stores[k] = stores[k - 1] if st[k][2] else tuple(np.zeros((cmbh * s, mbw * s), np.uint8) for s in (16, 8, 8))

        def resolve(l, name, k=k):
            """the picture a decoder reaches through the index that the stream carries for `name`"""
            if not paff:
                return name
            idx = pl[k]["l%d" % l].index(name)
            got = dec_lists[k][l]
            assert idx < len(got) or wrong, (k, l, name, got)
            return got[idx] if idx < len(got) else got[-1]

        def ref_plane(name, c, parity=parity):
            if not paff:
                return refs[name][c]
            i, q = fr.field_of(pics, name)
            return fr.FieldRef(stores[i][c], q, wrong) if parity else stores[i][c]
        qps = sw.mb_qps(seq, p)
        nxn_modes = rr.mode_tables(seq, p, wrong, rstats)[1]
        refs = out if stale_ref_of != k else out[:k - 1] + [raw[k - 1]]
        planes = [np.zeros((mbh * 16, mbw * 16), np.uint8), np.zeros((mbh * 8, mbw * 8), np.uint8), np.zeros((mbh * 8, mbw * 8), np.uint8)]
        step = sw.layout_step(seq, p)
        mode = 0
        if kind == "P" and seq.get("weighted_pred", 0):
            mode = 1
        elif kind == "B":
            mode = seq.get("weighted_bipred", 0)
        for a, m in enumerate(p["mbs"]):
            x, y = a % mbw, a // mbw
            first = a - a % step
            t = m["t"]

            avail = rr.mb_avail(seq, p, a)
            RES = rr.mb_residual(seq, m, qps[a], wrong, lists, scans) if "coef" in m else None
            if RES is not None and rstats is not None:
                rstats.add(("qp", t, qps[a]))
                for c in (0, 1, 2):
                    s = 16 if c == 0 else 8
                    v = None if t in ("i4", "i8") and c == 0 else RES[c]      # (the luma of I_NxN is counted block by block)
                    if v is not None and v.any():
                        rstats.add(("residual_sign", t, c, int(v.min()) < 0, int(v.max()) > 0))
            if t == "pcm":
                for c, key in enumerate(("y", "cb", "cr")):
                    s = 16 if c == 0 else 8
                    planes[c][y * s:(y + 1) * s, x * s:(x + 1) * s] = m[key]
            elif t in ("i16", "i4", "i8"):
                al, at = avail(-1, 0), avail(0, -1)
                saved = None
                if parity and at and "intra_neighbour_from_other_parity" in wrong:
                    # the line above in the FRAME: for a bottom field the top field's line of the same number, for a top field the bottom's before it
                    saved = [pl_[y * s - 1].copy() for pl_, s in zip(planes, (16, 8, 8))]
                    for pl_, s, S in zip(planes, (16, 8, 8), stores[k]):
                        pl_[y * s - 1] = S[2 * (y * s) + (parity == "bottom") - 1]
                assert (t != "i16" or m["mode"] != 3) and m["cmode"] != 3 or (al and at and avail(-1, -1)), "plane prediction needs the corner"
                assert (t != "i16" or (m["mode"] != 0 or at) and (m["mode"] != 1 or al)) and (m["cmode"] != 2 or at) and (m["cmode"] != 1 or al)
                if t == "i16":
                    planes[0][y * 16:(y + 1) * 16, x * 16:(x + 1) * 16] = intra16_luma(planes[0], x * 16, y * 16, m["mode"], al, at)
                else:
                    rr.intra_nxn_luma(planes[0], x * 16, y * 16, m, nxn_modes[a], RES[0] if RES else np.zeros((16, 16), np.int64), avail, wrong, rstats)
                for c in (1, 2):
                    planes[c][y * 8:(y + 1) * 8, x * 8:(x + 1) * 8] = intra_chroma(planes[c], x * 8, y * 8, m["cmode"], al, at)
                if saved is not None:
                    for pl_, s, row in zip(planes, (16, 8, 8), saved):
                        pl_[y * s - 1] = row
                if rstats is not None:
                    rstats.add(("kind", kind, t, "T" * at + "L" * al + "C" * avail(-1, -1) + "R" * avail(1, -1)))
                    if t == "i16":
                        rstats.add(("i16", m["mode"], m["cmode"], bool(RES and np.asarray(m["coef"].get("ydc", [0])).any()),
                                    bool(RES and m["coef"].get("y")), bool(RES and np.asarray(m["coef"].get("cdc", [0])).any()), bool(RES and m["coef"].get("cac"))))
            else:
                if derived is not None and t in ("mv", "skip"):
                    rects = mr.rectangles(derived[k][a])
                elif t == "skip":
                    rects = partitions(dict(t="16x16", l0=(pl[k]["l0"][0], (0, 0))))        # 8.4.1.1: no neighbour available -> zero vector, RefPicList0[0]
                else:
                    rects = partitions(m)
                for (px, py, w, h, l0, l1) in rects:
                    for c in (0, 1, 2):
                        sub = 1 if c == 0 else 2
                        X, Yy, W, Hh = (x * 16 + px) // sub, (y * 16 + py) // sub, w // sub, h // sub
                        pr = [None, None]
                        ent = [(0, 0), (0, 0)]
                        for l, q in enumerate((l0, l1)):
                            if q is None:
                                continue
                            got = resolve(l, q[0])
                            R = ref_plane(got, c)
                            mvc = (q[1][0], q[1][1] + fr.chroma_mvy_offset(parity, fr.field_of(pics, got)[1], wrong)) if paff else q[1]
                            pr[l] = mc_luma(R, X, Yy, W, Hh, q[1]) if c == 0 else mc_chroma(R, X, Yy, W, Hh, mvc)
                            if rstats is not None and parity:
                                rstats.add(("field_ref", parity, fr.field_of(pics, got)[1], st[fr.field_of(pics, got)[0]][0] == st[k][0]))
                            if mode == 1:
                                wp = p["wp"]
                                ld = wp["ld_y"] if c == 0 else wp["ld_c"]
                                idx = pl[k]["l%d" % l].index(q[0])
                                lst = wp.get("l%d" % l, [])
                                e = (lst[idx] if idx < len(lst) and lst[idx] else {})
                                v = e.get("y") if c == 0 else (e.get("c")[c - 1] if e.get("c") else None)
                                ent[l] = v if v is not None else (1 << ld, 0)        # 7.4.3.2: flag 0 -> weight 2^denominator, offset 0
                        logwd = 5
                        if mode == 1:
                            logwd = p["wp"]["ld_y"] if c == 0 else p["wp"]["ld_c"]
                        elif mode == 2 and l0 is not None and l1 is not None:
                            if paff:
                                n0, n1 = resolve(0, l0[0]), resolve(1, l1[0])
                                pocs = [p["poc"], fr.field_poc(pics, n0), fr.field_poc(pics, n1)]
                                if "implicit_weights_from_frame_poc" in wrong or not parity:      # a frame's count: the smaller of its two fields'
                                    fpoc = lambda i: min(pics[j]["poc"] for j in range(len(pics)) if st[j][0] == st[i][0])
                                    pocs = [fpoc(k), fpoc(fr.field_of(pics, n0)[0]), fpoc(fr.field_of(pics, n1)[0])]
                                w0, w1 = implicit_weights(*pocs)
                                if rstats is not None and parity:
                                    rstats.add(("implicit", parity, w0, w1))
                            else:
                                w0, w1 = implicit_weights(p["poc"], pics[l0[0]]["poc"], pics[l1[0]]["poc"])
                            ent = [(w0, 0), (w1, 0)]
                        planes[c][Yy:Yy + Hh, X:X + W] = weighted(pr[0], pr[1], mode, logwd, ent[0], ent[1])
                if rstats is not None and RES is not None:
                    rstats.add(("kind", kind, "inter_t8" if m.get("t8", 0) else "inter", ""))
                if "resid" in m:
                    bx, by = sw.BLK_XY[m["resid"][0]]
                    blk = planes[0][y * 16 + by:y * 16 + by + 4, x * 16 + bx:x * 16 + bx + 4]
                    blk[:] = clip1(blk.astype(np.int64) + dc_only_residual(qps[a], m["resid"][1]))      # 8.5.14: Clip1(pred + r)
            if RES is not None and t != "pcm":
                for c in (0, 1, 2):                                 # 8.5.14: u = Clip1(pred + r) (Intra4x4 / Intra8x8 luma: done block by block above)
                    if c == 0 and t in ("i4", "i8"):
                        continue
                    s = 16 if c == 0 else 8
                    blk = planes[c][y * s:(y + 1) * s, x * s:(x + 1) * s]
                    v = blk.astype(np.int64) + RES[c]
                    if rstats is not None and v.min() < 0:
                        rstats.add(("clip1_at_0", t, c))
                    if rstats is not None and v.max() > 255:
                        rstats.add(("clip1_at_255", t, c))
                    blk[:] = clip1(v)
        raw.append(tuple(planes))
        if derived is not None:
            dpics[k] = dict(p, mbs=[dict(m, blocks=derived[k][a]) if m["t"] in ("mv", "skip") else m for a, m in enumerate(p["mbs"])])
        out.append(deblock_ref.deblock_picture(seq, dpics, pl, k, tuple(planes), stats, wrong))
        if paff:
            for S, pl_ in zip(stores[k], out[-1]):
                if parity:
                    S[int(parity == "bottom")::2] = pl_
                else:
                    S[:] = pl_
            if st[k][2] and "deblock_across_parities" in wrong:
                out[-2:] = deblock_ref.woven_filter(frame_seq, pics, pl, k, stores[k], raw[-2:], wrong)
    if unfiltered is not None:
        unfiltered[:] = raw
    return out


def pack(seq, planes, fmt):
    """One display frame as the decoder hands it out: cropped, fmt 1 = I420 (Y, Cb, Cr), 0 = NV12."""
    w, h = seq["width"], seq["height"]
    assert w % 2 == 0 and h % 2 == 0
    y, cb, cr = planes[0][:h, :w], planes[1][:h // 2, :w // 2], planes[2][:h // 2, :w // 2]
    if fmt == 1:
        return y.tobytes() + cb.tobytes() + cr.tobytes()
    return y.tobytes() + np.stack([cb, cr], axis=-1).tobytes()


def display_order(pics):
    """decode index of every output frame (of a frame coded as two fields: of its first field), in output order"""
    if fr.has_fields(pics):
        return [k for k, _ in fr.output_frames(pics, [()] * len(pics))]
    return sorted(range(len(pics)), key=lambda k: pics[k]["poc"])


def expected_frames(seq, pics, fmt, planes=None, wrong=frozenset()):
    planes = planes if planes is not None else expect_h264(seq, pics)
    if fr.has_fields(pics):
        return [pack(seq, frame, fmt) for _, frame in fr.output_frames(pics, planes, wrong)]
    return [pack(seq, planes[k], fmt) for k in display_order(pics)]


def describe_mb(m):
    return {k: ("samples" if isinstance(v, np.ndarray) else (sorted(v) if k == "coef" else v)) for k, v in m.items()}


def first_difference(seq, pics, got_frames, fmt, planes=None, units="mbs"):
    """None when every frame is the expected one, else a text: which picture (display and decode index), plane, block and script entry differs first.
    planes: the expected pictures in decode order (default: expect_h264 of the script); units: the script's key of the 16x16 blocks ("cus" for H.265)."""
    block = 16
    want = expected_frames(seq, pics, fmt, planes)
    if len(got_frames) != len(want):
        return f"{len(got_frames)} frames, the script has {len(want)}"
    w, h = seq["width"], seq["height"]
    order = display_order(pics)
    for d, (g, e) in enumerate(zip(got_frames, want)):
        if g == e:
            continue
        if len(g) != len(e):
            return f"display frame {d}: {len(g)} bytes, expected {len(e)}"
        ga, ea = np.frombuffer(g, np.uint8), np.frombuffer(e, np.uint8)
        i = int(np.flatnonzero(ga != ea)[0])
        if i < w * h:
            plane, px, py = "Y", i % w, i // w
            bx, by = px // block, py // block
        else:
            j = i - w * h
            if fmt == 1:
                plane = "Cb" if j < w * h // 4 else "Cr"
                j %= w * h // 4
                px, py = j % (w // 2), j // (w // 2)
            else:
                plane, px, py = ("Cb", "Cr")[j & 1], (j % w) // 2, j // w
            bx, by = px * 2 // block, py * 2 // block
        k = order[d]
        a = by * ((w + block - 1) // block) + bx
        if pics[k].get("field"):                                    # the line's parity says which field; the field's line is half the frame's
            st = fr.structure(pics)
            if k + 1 < len(pics) and st[k + 1][2] and (pics[k]["field"] == "bottom") != bool(py & 1):
                k += 1
            a = (py // 2) // (block if plane == "Y" else block // 2) * ((w + block - 1) // block) + bx
        entry = describe_mb(pics[k][units][a])
        return (f"display frame {d} (decode index {k}, {pics[k]['kind']}, POC {pics[k]['poc']}), plane {plane}, sample x={px} y={py}, block {a} "
                f"(x {bx}, y {by}): got {ga[i]} expected {ea[i]}, {int((ga != ea).sum())} bytes differ in this frame; script entry {entry}")
    return None


# ---------------------------------------------------------------------------------------------------------------------------------------------
# closed forms (checked against the restatements above in tests/test_analytic_host.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ramp_luma_closed(f, a, c, fx, fy):
    """The fractional sample (fx, fy) at a position whose integer sample is f, on the ramp a*x + c*y + d, wherever the six-tap footprint lies inside
    the picture and the ramp inside 0..255.  The taps sum to 32 and are symmetric about the half position, so the unrounded sum at b is 32 f + 16 a:
    b = (32 f + 16 a + 16) >> 5 = f + ((a + 1) >> 1); h likewise with c; j's taps of taps give 1024 f + 512 (a + c): j = f + ((a + c + 1) >> 1); s is b
    one row down, m is h one column right; the quarter positions are the rounded means of 8.4.2.2.1."""
    b, h, j = f + ((a + 1) >> 1), f + ((c + 1) >> 1), f + ((a + c + 1) >> 1)
    G, H, M, s, m = f, f + a, f + c, b + c, h + a
    avg = lambda p, q: (p + q + 1) >> 1
    return {(0, 0): G, (1, 0): avg(G, b), (2, 0): b, (3, 0): avg(H, b), (0, 1): avg(G, h), (1, 1): avg(b, h), (2, 1): avg(b, j), (3, 1): avg(b, m),
            (0, 2): h, (1, 2): avg(h, j), (2, 2): j, (3, 2): avg(j, m), (0, 3): avg(M, h), (1, 3): avg(h, s), (2, 3): avg(j, s), (3, 3): avg(m, s)}[(fx, fy)]


def ramp_chroma_closed(f, a, c, fx, fy):
    """8-270 on the ramp a*x + c*y + d with A = f: the four weights sum to 64, B - A = D - C = a, C - A = c: (64 f + 8 a fx + 8 c fy + 32) >> 6."""
    return f + ((8 * a * fx + 8 * c * fy + 32) >> 6)


def ramp(h, w, a, c, d):
    yy, xx = np.mgrid[0:h, 0:w]
    v = a * xx + c * yy + d
    assert v.min() >= 0 and v.max() <= 255, (a, c, d, v.min(), v.max())
    return v.astype(np.uint8)


def ramp_closed_frame(seq, p, refs_params):
    """Closed-form luma / chroma of a P picture of 16x16 macroblocks over ramp references: (Y, Cb, Cr, maskY, maskCb) -- mask = where the form applies
    (luma: the integer position within 2 .. W-4, 2 .. H-4 of the coded picture; chroma: the 2x2 footprint inside the plane).  refs_params[pic] =
    ((a, c, d) luma, (a, c, d) Cb, (a, c, d) Cr)."""
    mbw, mbh = (seq["width"] + 15) // 16, (seq["height"] + 15) // 16
    W, H = mbw * 16, mbh * 16
    outs = [np.zeros((H, W), np.int64), np.zeros((H // 2, W // 2), np.int64), np.zeros((H // 2, W // 2), np.int64)]
    masks = [np.zeros((H, W), bool), np.zeros((H // 2, W // 2), bool)]
    for a_, m in enumerate(p["mbs"]):
        x, y = a_ % mbw, a_ // mbw
        pic, mv = m["l0"]
        for c in (0, 1, 2):
            s = 16 if c == 0 else 8
            fr = 4 if c == 0 else 8
            (ra, rc, rd) = refs_params[pic][c]
            yy, xx = np.mgrid[y * s:(y + 1) * s, x * s:(x + 1) * s]
            xi, yi = xx + (mv[0] // fr), yy + (mv[1] // fr)
            f = ra * xi + rc * yi + rd
            Wc, Hc = (W, H) if c == 0 else (W // 2, H // 2)
            if c == 0:
                outs[c][yy, xx] = ramp_luma_closed(f, ra, rc, mv[0] & 3, mv[1] & 3)
                masks[0][yy, xx] = (xi >= 2) & (xi <= Wc - 4) & (yi >= 2) & (yi <= Hc - 4)
            else:
                outs[c][yy, xx] = ramp_chroma_closed(f, ra, rc, mv[0] & 7, mv[1] & 7)
                masks[1][yy, xx] = (xi >= 0) & (xi <= Wc - 2) & (yi >= 0) & (yi <= Hc - 2)
    return outs[0], outs[1], outs[2], masks[0], masks[1]
