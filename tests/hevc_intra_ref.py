"""H.265 intra sample prediction typed out once more, in numpy, for the scripted streams of tests/scripted_hevc.py.

Restated from the clauses, not from tools/hevcgen.c, the oracle or the product:
  6.4.1        z-scan availability: inside the picture, not later in z-scan order, in the same slice (tiles are not used)
  8.4.3        the chroma mode from intra_chroma_pred_mode
  8.4.4.2.2    the 4 * nTbS + 1 neighbours, constrained_intra_pred_flag, 128 when nothing is available, the substitution search
  8.4.4.2.3    [1 2 1] and bi-linear filtering of the neighbours
  8.4.4.2.4-6  planar, DC, angular (intraPredAngle / invAngle: the separately typed copies of tests/test_table_provenance.py)
  8.6.2-8.6.4.2 for one coefficient at (0, 0), 8-bit samples, flat scaling factor m = 16: every shift written out
A block's neighbours are kept in SEARCH ORDER, v[0 .. 4 nTbS]: v[0] = p[-1][2 nTbS - 1] upwards to v[2 nTbS] = p[-1][-1], then p[0][-1] .. p[2 nTbS - 1][-1].

``expect`` walks the pictures in decoding order, transform block by transform block, predicting from its own reconstructed planes, and returns the
planes and one record per predicted block.  The switches make it wrong on purpose (tests/test_hevc_intra_host.py: a case that cannot tell such a
decoder from a right one pins nothing)."""
import numpy as np

import scripted_hevc as hw
from test_table_provenance import HEVC_INTRA_ANGLE, HEVC_INV_ANGLE

SWITCHES = ("no_smoothing", "weak_for_strong", "no_dc_edge", "no_hv_edge", "no_hv_clip", "substitute_backwards", "corner_from_top", "residual_no_clip")
LEVEL_SCALE = [40, 45, 51, 57, 64, 72]
QPC = list(range(30)) + [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37] + [q - 6 for q in range(44, 58)]      # Table 8-10, qPi 0 .. 57
DST_ROW0 = np.array([29, 55, 74, 84], np.int64)
GROUPS = ("below_left", "left", "corner", "above", "above_right")


def clip16(v):
    return np.clip(v, -32768, 32767)


def zorder(x, y, ctb_log2, cw):
    """6.5.2 without tiles, for numpy arrays of luma positions: CTB address in raster order, then the bits of x and y interleaved (4x4 units)"""
    z = ((y >> ctb_log2) * cw + (x >> ctb_log2)) << (2 * (ctb_log2 - 2))
    for i in range(ctb_log2 - 2):
        z = z | (((x >> (2 + i)) & 1) << (2 * i)) | (((y >> (2 + i)) & 1) << (2 * i + 1))
    return z


def neighbour_positions(x, y, n):
    """the 4 n + 1 neighbour positions of the block at (x, y) in search order (module docstring)"""
    xs = np.concatenate([np.full(2 * n + 1, x - 1), x + np.arange(2 * n)])
    ys = np.concatenate([y + np.arange(2 * n - 1, -2, -1), np.full(2 * n, y - 1)])
    return xs, ys


def substitute(v, ok, backwards=False):
    """8.4.4.2.2: v, ok in search order.  Returns (samples, where the search found the first available sample: None when v[0] is available or nothing is)"""
    n = (len(v) - 1) // 4
    if not ok.any():
        return np.full(len(v), 128, np.int64), None
    idx = np.where(ok, np.arange(len(v)), -1)
    first = int(np.argmax(ok))
    if backwards:                                                   # WRONG on purpose: an unavailable sample takes its successor
        idx = np.where(ok, np.arange(len(v)), len(v))
        idx = np.minimum.accumulate(idx[::-1])[::-1]
        idx[idx == len(v)] = len(v) - 1 - int(np.argmax(ok[::-1]))
    else:
        idx = np.maximum.accumulate(idx)
        idx[idx < 0] = first
    start = None if first == 0 else ("column" if first < 2 * n else ("corner" if first == 2 * n else "top"))
    return v[idx].astype(np.int64), start


def smooth(left, top, n, mode, strong_enabled, sw):
    """8.4.4.2.3 for a luma block: (left, top, which filter, the two values the bi-linear decision compares with 8 or None)"""
    if mode == 1 or n == 4 or sw.get("no_smoothing"):
        return left, top, "none", None
    if min(abs(mode - 26), abs(mode - 10)) <= {8: 7, 16: 1, 32: 0}[n]:
        return left, top, "none", None
    vals = None
    if strong_enabled and n == 32:
        vals = (abs(int(top[0] + top[64] - 2 * top[32])), abs(int(left[0] + left[64] - 2 * left[32])))
        if vals[0] < 8 and vals[1] < 8 and not sw.get("weak_for_strong"):
            i = np.arange(1, 64)
            fl, ft = left.copy(), top.copy()
            fl[1:64] = ((64 - i) * left[0] + i * left[64] + 32) >> 6
            ft[1:64] = ((64 - i) * top[0] + i * top[64] + 32) >> 6
            return fl, ft, "strong", vals
    fl, ft = left.copy(), top.copy()
    fl[0] = ft[0] = (left[1] + 2 * left[0] + top[1] + 2) >> 2
    fl[1:2 * n] = (left[2:] + 2 * left[1:2 * n] + left[:2 * n - 1] + 2) >> 2
    ft[1:2 * n] = (top[2:] + 2 * top[1:2 * n] + top[:2 * n - 1] + 2) >> 2
    return fl, ft, "121", vals


def angular(main, side, n, angle, inv):
    """8.4.4.2.6 for the modes 18 .. 34 (main = the row above, side = the left column; the caller swaps them and transposes for 2 .. 17):
    main[i] = p[-1 + i][-1], side[i] = p[-1][-1 + i]"""
    ref = np.zeros(3 * n + 2, np.int64)                             # ref[x] lives at ref[n + x], x = -n .. 2 n (+ 1: read with iFact 0, weight 0)
    ref[n:2 * n + 1] = main[:n + 1]
    last = (n * angle) >> 5
    if angle < 0:
        if last < -1:
            x = np.arange(last, 0)
            ref[n + x] = side[(x * inv + 128) >> 8]
    else:
        ref[2 * n + 1:3 * n + 1] = main[n + 1:2 * n + 1]
    yy, xx = np.mgrid[0:n, 0:n]
    idx, fact = ((yy + 1) * angle) >> 5, ((yy + 1) * angle) & 31
    return ((32 - fact) * ref[n + xx + idx + 1] + fact * ref[n + xx + idx + 2] + 16) >> 5


def predict(v, n, mode, c, strong_enabled=False, sw={}):
    """The n x n prediction [y][x] of plane c from the substituted neighbours v (search order); also the filter applied, the values of the
    bi-linear decision, and whether Clip1 of the mode 10 / 26 edge filter cut at 0 / at 255"""
    left, top = v[:2 * n + 1][::-1].copy(), v[2 * n:].copy()        # left[i] = p[-1][i - 1], top[i] = p[i - 1][-1]
    if sw.get("corner_from_top"):                                   # WRONG on purpose
        left[0] = top[0] = top[1]
    filt, vals, cut = "none", None, (False, False)
    if c == 0:
        left, top, filt, vals = smooth(left, top, n, mode, strong_enabled, sw)
    log2 = n.bit_length() - 1
    yy, xx = np.mgrid[0:n, 0:n]
    edge = c == 0 and n < 32
    if mode == 0:                                                   # 8.4.4.2.4
        pred = ((n - 1 - xx) * left[yy + 1] + (xx + 1) * top[n + 1] + (n - 1 - yy) * top[xx + 1] + (yy + 1) * left[n + 1] + n) >> (log2 + 1)
    elif mode == 1:                                                 # 8.4.4.2.5
        dc = (int(top[1:n + 1].sum()) + int(left[1:n + 1].sum()) + n) >> (log2 + 1)
        pred = np.full((n, n), dc, np.int64)
        if edge and not sw.get("no_dc_edge"):
            pred[0, :] = (top[1:n + 1] + 3 * dc + 2) >> 2
            pred[:, 0] = (left[1:n + 1] + 3 * dc + 2) >> 2
            pred[0, 0] = (left[1] + 2 * dc + top[1] + 2) >> 2
    else:
        angle, inv = HEVC_INTRA_ANGLE[mode], HEVC_INV_ANGLE[mode]
        pred = angular(top, left, n, angle, inv) if mode >= 18 else angular(left, top, n, angle, inv).T
        if mode in (10, 26) and edge and not sw.get("no_hv_edge"):
            main, side = (top, left) if mode == 26 else (left, top)
            e = main[1] + ((side[1:n + 1] - side[0]) >> 1)
            cut = (bool((e < 0).any()), bool((e > 255).any()))
            e = (e & 255) if sw.get("no_hv_clip") else np.clip(e, 0, 255)
            if mode == 26:
                pred[:, 0] = e
            else:
                pred[0, :] = e
    return pred, filt, vals, cut


def dc_residual(level, qp, log2, dst):
    """8.6.2 - 8.6.4.2 for one coefficient `level` at (0, 0) of a 2^log2 block at quantisation parameter qp, 8-bit samples: the residual [y][x]"""
    n = 1 << log2
    bd_shift = 8 + log2 - 5                                         # 8.6.3: BitDepth + Log2(nTbS) - 5
    d = int(clip16(((level * 16 * LEVEL_SCALE[qp % 6] << (qp // 6)) + (1 << (bd_shift - 1))) >> bd_shift))
    if dst:                                                         # 8.6.4.2 with the DST-VII matrix: column 0 of the coefficients meets row 0 of the matrix
        g = clip16((DST_ROW0 * d + 64) >> 7)                        # first (vertical) stage, by y
        return (DST_ROW0[None, :] * g[:, None] + 2048) >> 12        # second stage, bdShift = 20 - BitDepth
    g = int(clip16((64 * d + 64) >> 7))
    return np.full((n, n), (64 * g + 2048) >> 12, np.int64)


def chroma_qp(qp):
    return QPC[max(0, min(57, qp))]                                 # 8.6.1 with both offsets 0, ChromaArrayType 1


def chroma_mode(v, luma_mode):
    """8.4.3 (4:2:0)"""
    if v == 4:
        return luma_mode
    m = (0, 26, 10, 1)[v]
    return 34 if m == luma_mode else m


def tu_origin(i, tu, log2cb):
    """The offset of transform unit i (decoding order) in a tree of uniform depth tu"""
    x = y = 0
    for d in range(tu):
        q = (i >> (2 * (tu - 1 - d))) & 3
        x += (q & 1) << (log2cb - 1 - d)
        y += (q >> 1) << (log2cb - 1 - d)
    return x, y


def expect(seq, pics, **sw):
    """-> ([(Y, Cb, Cr)] per picture in DECODE order, coded size, uint8; [record per predicted block])"""
    assert all(k in SWITCHES for k in sw), sw
    W, H = hw.coded_size(seq)
    g = hw.geometry(seq)
    cw, ch = hw.ctb_dims(seq)
    plans = hw.plan(seq, pics)
    constrained, strong = seq.get("constrained_intra", 0), seq.get("strong_intra", 0)
    out, records = [], []
    for k, (p, pl) in enumerate(zip(pics, plans)):
        planes = [np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)]
        intra = np.zeros((H // 4, W // 4), bool)                    # CuPredMode == MODE_INTRA, per 4x4
        step = {"ctb": 1, "row": cw, "pic": cw * ch}[p.get("layout", "ctb" if p["kind"] != "I" else "pic")]
        slice_of = (np.arange(cw * ch) // step * step).reshape(ch, cw)
        qp = p.get("qp", seq.get("init_qp", 26))

        def block(c, x, y, n, mode, level, unit):
            """one transform block of plane c at (x, y) in that plane's samples: 8.4.4.2.2 - 8.4.4.2.6, then 8.6 and Clip1"""
            sh = 1 if c else 0
            xs, ys = neighbour_positions(x, y, n)
            X, Y = xs << sh, ys << sh
            ok = (X >= 0) & (Y >= 0) & (X < W) & (Y < H)
            Xc, Yc = np.clip(X, 0, W - 1), np.clip(Y, 0, H - 1)
            ok &= zorder(Xc, Yc, g["ctb"], cw) <= zorder(np.int64(x << sh), np.int64(y << sh), g["ctb"], cw)
            ok &= slice_of[Yc >> g["ctb"], Xc >> g["ctb"]] == slice_of[(y << sh) >> g["ctb"], (x << sh) >> g["ctb"]]
            if constrained:
                ok &= intra[Yc >> 2, Xc >> 2]
            v, start = substitute(planes[c][Yc >> sh, Xc >> sh], ok, sw.get("substitute_backwards", False))
            pred, filt, vals, cut = predict(v, n, mode, c, strong, sw)
            res_cut = None
            if level:
                log2 = n.bit_length() - 1
                s = pred + dc_residual(level, chroma_qp(qp) if c else qp, log2, c == 0 and n == 4)
                res_cut = (bool((s < 0).any()), bool((s > 255).any()))
                pred = (s & 255) if sw.get("residual_no_clip") else np.clip(s, 0, 255)
            planes[c][y:y + n, x:x + n] = pred
            grp = [ok[:n], ok[n:2 * n], ok[2 * n:2 * n + 1], ok[2 * n + 1:3 * n + 1], ok[3 * n + 1:]]
            records.append(dict(pic=k, plane=c, x=x, y=y, n=n, mode=mode, avail=tuple(2 if q.all() else (1 if q.any() else 0) for q in grp),
                                all_avail=bool(ok.all()), substituted=not ok.all(), start=start, filt=filt, strong_values=vals, hv_cut=cut,
                                gap=bool(ok.any() and not ok[int(np.argmax(ok)):len(ok) - int(np.argmax(ok[::-1]))].all()),
                                level=level, res_cut=res_cut, unit=unit))

        for (x, y, log2, depth, u) in hw.walk(seq, p):
            n, t = 1 << log2, u["t"]
            area = [(slice(y >> s, (y + n) >> s), slice(x >> s, (x + n) >> s)) for s in (0, 1, 1)]
            intra[y >> 2:(y + n) >> 2, x >> 2:(x + n) >> 2] = t in ("pcm", "intra")
            if t == "pcm":
                for c, key in enumerate(("y", "cb", "cr")):
                    planes[c][area[c]] = u[key]
            elif t == "skip":
                # MaxNumMergeCand 1: a neighbour's vector or the zero candidate, both the zero vector on index 0 (of both lists in a B slice)
                for c in range(3):
                    a = out[pl["l0"][0]][c][area[c]].astype(np.int64)
                    planes[c][area[c]] = a if p["kind"] == "P" else (a + out[pl["l1"][0]][c][area[c]] + 1) >> 1
            else:
                assert t == "intra", "units with a vector belong to tests/analytic_hevc.py"
                modes = u["modes"]
                nxn = len(modes) == 4
                tu = u.get("tu", 1 if nxn else 0)
                lg = log2 - tu
                dc = u.get("dc") or [None] * 4 ** tu
                cm = chroma_mode(u.get("chroma", 4), modes[0])
                for i in range(4 ** tu):
                    ox, oy = tu_origin(i, tu, log2)
                    lv = dc[i] or (0, 0, 0)
                    block(0, x + ox, y + oy, 1 << lg, modes[(i >> (2 * (tu - 1))) & 3] if nxn else modes[0], lv[0], u)
                    if lg > 2:
                        for c in (1, 2):
                            block(c, (x + ox) >> 1, (y + oy) >> 1, 1 << (lg - 1), cm, lv[c], u)
                    elif i % 4 == 3:                                # 4x4 luma blocks: one 4x4 block per chroma plane after the fourth, at the 8x8 origin
                        for c in (1, 2):
                            block(c, ((x + ox) & ~7) >> 1, ((y + oy) & ~7) >> 1, 4, cm, lv[c], u)
        out.append(tuple(planes))
    return out, records


def describe(r):
    a = ", ".join(f"{g} {('none', 'part', 'all')[q]}" for g, q in zip(GROUPS, r["avail"]))
    return (f"picture {r['pic']} plane {('Y', 'Cb', 'Cr')[r['plane']]} block at ({r['x']}, {r['y']}) {r['n']}x{r['n']} mode {r['mode']} [{a}] "
            f"filter {r['filt']} substitution start {r['start']} level {r['level']}")


def first_wrong_block(records, planes, got_planes):
    """The first record (decoding order) whose block differs between the expected planes and the decoded ones, described; None if there is none"""
    for r in records:
        e = planes[r["pic"]][r["plane"]][r["y"]:r["y"] + r["n"], r["x"]:r["x"] + r["n"]]
        q = got_planes[r["pic"]][r["plane"]][r["y"]:r["y"] + r["n"], r["x"]:r["x"] + r["n"]]
        e = e[:q.shape[0], :q.shape[1]]                             # (the decoded planes are cropped)
        if not np.array_equal(e, q):
            j = np.argwhere(e != q)[0]
            return describe(r) + f": first at ({r['x'] + j[1]}, {r['y'] + j[0]}) got {q[j[0], j[1]]} expected {e[j[0], j[1]]}"
    return None


def unpack(seq, frame, fmt):
    """a display frame as the decoder hands it out (cropped; fmt 1 = I420, 0 = NV12) -> (Y, Cb, Cr)"""
    w, h = seq["width"], seq["height"]
    f = np.frombuffer(frame, np.uint8)
    assert len(f) == w * h * 3 // 2, (len(f), w, h)
    y, c = f[:w * h].reshape(h, w), f[w * h:]
    if fmt == 1:
        return y, c[:w * h // 4].reshape(h // 2, w // 2), c[w * h // 4:].reshape(h // 2, w // 2)
    c = c.reshape(h // 2, w // 2, 2)
    return y, c[:, :, 0], c[:, :, 1]


def difference(seq, pics, frames, fmt, planes, records):
    """None when the display frames are the expected pictures, else a text that names the first predicted block (decoding order) that is wrong with
    its record, or, if every predicted block is right, the first wrong sample of a unit that is not intra"""
    if len(frames) != len(pics):
        return f"{len(frames)} frames, the script has {len(pics)}"
    w, h = seq["width"], seq["height"]
    order = sorted(range(len(pics)), key=lambda k: pics[k]["poc"])
    got = [None] * len(pics)
    for d, k in enumerate(order):
        got[k] = unpack(seq, frames[d], fmt)
    want = [tuple(pl[c][:h >> (c > 0), :w >> (c > 0)] for c in range(3)) for pl in planes]
    if all(np.array_equal(a, b) for e, q in zip(want, got) for a, b in zip(e, q)):
        return None
    msg = first_wrong_block(records, want, got)
    if msg is not None:
        return msg
    for k in range(len(pics)):
        for c in range(3):
            if not np.array_equal(want[k][c], got[k][c]):
                j = np.argwhere(want[k][c] != got[k][c])[0]
                return (f"picture {k} ({pics[k]['kind']}, POC {pics[k]['poc']}) plane {('Y', 'Cb', 'Cr')[c]} sample ({j[1]}, {j[0]}): got {got[k][c][j[0], j[1]]} "
                        f"expected {want[k][c][j[0], j[1]]}, outside every predicted block (a PCM or skipped unit)")
