"""H.265 quantisation parameters, scaling and inverse transforms typed out once more, in numpy int64, for the scripted streams of tests/scripted_hevc.py.

Restated from the clauses and computed from the SCRIPT, never from a bitstream -- not from tools/hevcgen.c, the oracle or the product:
  8.6.1      qPY_PRED from qPY_PREV and the left / above neighbours of the quantisation group inside the CTB, the first group of a slice,
             QpY = (qPY_PRED + CuQpDeltaVal + 52) % 52, chroma qPi = Clip3(0, 57, QpY + pps offset + slice offset) through Table 8-10
  7.4.5      the scaling lists in effect (PPS over SPS over the defaults), prediction from a reference list or the default, the up-sampling to 16x16 and
             32x32 and the DC replacement
  8.6.3      m = 16 or the list entry, levelScale, bdShift = BitDepth + Log2(nTbS) - 5, the 16-bit clip
  8.6.4.2    both transform stages with the intermediate clip, DST-VII only for intra 4x4 luma, transform skip (r = d << 7), then 8.6.2's
             (r + 2048) >> 12; cu_transquant_bypass_flag: the levels are the residual
Prediction: intra from tests/hevc_intra_ref.py (the neighbours come from this module's own reconstructed planes), inter from analytic_hevc.mc14 / weighted.
A matrix M here is indexed [y][x]: M[y, x] = the clause's m[x][y] / d[x][y].

``expect`` returns the planes and one record per transform block that codes a residual; the switches make it wrong on purpose."""
import numpy as np

import analytic_hevc as ah
import hevc_intra_ref as ir
import scripted_hevc as hw
from test_table_provenance import HEVC_DEFAULT_8X8, HEVC_LEVEL_SCALE, hevc_trans_matrix

SWITCHES = ("matrix_transposed", "dct_for_dst", "dst_for_inter4", "dst_for_chroma4", "no_stage1_clip", "no_coeff_clip", "tskip_shift_6", "qpc_identity",
            "qp_neighbours_outside_ctb", "qp_prev_not_reset", "inter32_from_intra", "dc16_ignored")
QPC = list(range(30)) + [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37] + [q - 6 for q in range(44, 58)]      # Table 8-10, qPi 0 .. 57
TRANS = np.array(hevc_trans_matrix(), np.int64).reshape(32, 32)
DST = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], np.int64)
DIAG = {4: hw.scan_order(0, 4), 8: hw.scan_order(0, 8)}


def clip16(v):
    return np.clip(v, -32768, 32767)


def pad_cols(w):
    """(the product's kernel pads the coefficient columns it transforms to 4, 8, 16 or 32: the steps the cases are built around)"""
    return 4 if w <= 4 else (8 if w <= 8 else (16 if w <= 16 else 32))


# ---- 7.4.5 ----------------------------------------------------------------------------------------------------------------------------------------
def default_list(size_id, matrix_id):
    if size_id == 0:
        return [16] * 16
    return list(HEVC_DEFAULT_8X8[0 if matrix_id < (1 if size_id == 3 else 3) else 1])


def resolve_lists(spec):
    """{(sizeId, matrixId): (the 16 / 64 entries in diagonal order, dc)} from a scaling_list_data() script (tests/scripted_hevc.py)"""
    out = {}
    for size_id in range(4):
        for matrix_id in range(2 if size_id == 3 else 6):
            e = spec.get((size_id, matrix_id), ("ref", 0))
            if e[0] == "coded":
                out[(size_id, matrix_id)] = (list(e[1]), e[2] if size_id > 1 else 16)
            elif e[1] == 0:
                out[(size_id, matrix_id)] = (default_list(size_id, matrix_id), 16)
            else:
                out[(size_id, matrix_id)] = out[(size_id, matrix_id - e[1])]
    return out


def lists_in_effect(seq):
    sl = seq.get("scaling_lists")
    if sl is None:
        return None
    spec = sl["pps"] if sl.get("pps") is not None else (sl["sps"] if sl.get("sps") is not None else {})
    return resolve_lists(spec)


def scaling_factor(lists, log2, matrix_id, sw={}):
    """M[y, x] = ScalingFactor[sizeId][matrixId][x][y] of 7.4.5 (sizeId 3: matrixId 0 intra, 1 inter)"""
    n = 1 << log2
    size_id = log2 - 2
    coefs, dc = lists[(size_id, matrix_id)]
    blk = 4 if size_id == 0 else 8
    m = np.zeros((blk, blk), np.int64)
    for i, (x, y) in enumerate(DIAG[blk]):
        m[y, x] = coefs[i]
    if size_id > 1:
        m = np.kron(m, np.ones((n // 8, n // 8), np.int64))
        if not (sw.get("dc16_ignored") and size_id == 2):
            m[0, 0] = dc
    return m.T.copy() if sw.get("matrix_transposed") else m


# ---- 8.6.3, 8.6.4.2 -------------------------------------------------------------------------------------------------------------------------------
def scale(levels, qp, log2, m):
    """8.6.3: levels [y][x] -> (d [y][x], whether the 16-bit clip cut at the bottom / at the top)"""
    bd_shift = 8 + log2 - 5
    v = ((levels * m * HEVC_LEVEL_SCALE[qp % 6]) << (qp // 6)) + (1 << (bd_shift - 1)) >> bd_shift
    return clip16(v), (bool((v < -32768).any()), bool((v > 32767).any()))


def transform(d, dst, sw={}):
    """8.6.4.2 and the last step of 8.6.2 -> (residual [y][x], whether the clip after the first stage cut)"""
    n = d.shape[0]
    t = DST if dst else TRANS[::32 // n, :n]                        # rows = basis functions: y[i] = sum_j t[j][i] x[j]
    e = (t.T @ d + 64) >> 7                                         # first stage: the columns
    g = e if sw.get("no_stage1_clip") else clip16(e)
    return (g @ t + 2048) >> 12, bool((e != clip16(e)).any())


def residual(levels, qp, log2, m, dst, tskip, bypass, sw={}):
    """levels [y][x] of one block -> (residual [y][x], d, (16-bit clip low, high), first-stage clip)"""
    if bypass:
        return levels.copy(), levels, (False, False), False
    d, cut = scale(levels, qp, log2, m)
    if sw.get("no_coeff_clip"):
        d = ((levels * m * HEVC_LEVEL_SCALE[qp % 6]) << (qp // 6)) + (1 << (log2 + 2)) >> (log2 + 3)
    if tskip:
        return ((d << (6 if sw.get("tskip_shift_6") else 7)) + 2048) >> 12, d, cut, False
    r, c1 = transform(d, dst, sw)
    return r, d, cut, c1


def chroma_qp(qpy, offset, sw={}):
    qpi = max(0, min(57, qpy + offset))
    if sw.get("qpc_identity") and qpi >= 30:
        return min(qpi, 51)
    return QPC[qpi]


# ---- the pictures ---------------------------------------------------------------------------------------------------------------------------------
def expect(seq, pics, post=None, **sw):
    """-> ([(Y, Cb, Cr)] per picture in DECODE order, coded size, uint8; [one record per transform block with coefficients, in decoding order]).
    post(k, planes, dict(qpy=QpY per 4x4)) -> the planes that picture k leaves for later pictures and for the output (tests/hevc_loop_ref.py: the loop
    filters); by default the reconstruction itself, as every stream without loop filters has it"""
    assert all(k in SWITCHES for k in sw), sw
    W, H = hw.coded_size(seq)
    g = hw.geometry(seq)
    cw, ch = hw.ctb_dims(seq)
    ctb = g["ctb"]
    plans = hw.plan(seq, pics)
    lists = lists_in_effect(seq)
    qg_log2 = ctb - seq.get("diff_cu_qp_delta_depth", 0) if seq.get("cu_qp_delta", 0) else ctb
    out, records = [], []
    for k, (p, pl) in enumerate(zip(pics, plans)):
        planes = [np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)]
        qpy = np.zeros((H // 4, W // 4), np.int64)                  # QpY per 4x4
        slice_of = hw.slice_map(seq, p).reshape(ch, cw)
        slice_qp = p.get("qp", seq.get("init_qp", 26))
        offs = (0, seq.get("cb_qp_offset", 0) + p.get("cb_qp_offset", 0), seq.get("cr_qp_offset", 0) + p.get("cr_qp_offset", 0))
        state = dict(qg=None, prev_qp=slice_qp, last_qp=slice_qp, delta=0, coded=False, pred=slice_qp, slice=None, reset=False)
        job = 0                                                     # index in the product's list of inter residual blocks (hevc_jobs.h: HevcTb)

        def intra_block(c, x, y, n, mode):
            sh = 1 if c else 0
            xs, ys = ir.neighbour_positions(x, y, n)
            X, Y = xs << sh, ys << sh
            ok = (X >= 0) & (Y >= 0) & (X < W) & (Y < H)
            Xc, Yc = np.clip(X, 0, W - 1), np.clip(Y, 0, H - 1)
            ok &= ir.zorder(Xc, Yc, ctb, cw) <= ir.zorder(np.int64(x << sh), np.int64(y << sh), ctb, cw)
            ok &= slice_of[Yc >> ctb, Xc >> ctb] == slice_of[(y << sh) >> ctb, (x << sh) >> ctb]
            v, _ = ir.substitute(planes[c][Yc >> sh, Xc >> sh], ok)
            planes[c][y:y + n, x:x + n] = ir.predict(v, n, mode, c, seq.get("strong_intra", 0))[0]

        def add(c, x, y, n, coefs, qp_y, intra, tskip, bypass, unit, mode):
            """the residual of one block of plane c at (x, y) (that plane's samples), added to what the plane holds there"""
            nonlocal job
            log2 = n.bit_length() - 1
            lev = np.zeros((n, n), np.int64)
            for (cx, cy), v in coefs.items():
                lev[cy, cx] = v
            qp = chroma_qp(qp_y, offs[c], sw) if c else qp_y
            m = np.full((n, n), 16, np.int64)
            if lists is not None and not (tskip and n > 4):
                mid = (0 if intra or sw.get("inter32_from_intra") else 1) if n == 32 else (0 if intra else 3) + c
                m = scaling_factor(lists, log2, mid, sw)
            dst = intra and c == 0 and n == 4
            if n == 4 and ((sw.get("dct_for_dst") and dst) or (sw.get("dst_for_inter4") and not intra and c == 0) or (sw.get("dst_for_chroma4") and c > 0)):
                dst = not dst
            r, d, cut16, cut1 = residual(lev, qp, log2, m, dst, tskip, bypass, sw)
            nz = d != 0
            listed = not intra and (c == 0 or bool(nz.any()))       # (a luma block of an inter unit is listed even when every level scaled to 0)
            s = planes[c][y:y + n, x:x + n].astype(np.int64) + r
            planes[c][y:y + n, x:x + n] = np.clip(s, 0, 255)
            records.append(dict(pic=k, plane=c, x=x, y=y, n=n, intra=intra, mode=mode, levels=len(coefs), scaled=int(nz.sum()), qp=qp, qp_y=qp_y,
                                max_col=int(np.nonzero(nz.any(axis=0))[0].max()) if nz.any() else -1,
                                max_row=int(np.nonzero(nz.any(axis=1))[0].max()) if nz.any() else -1,
                                tskip=bool(tskip), bypass=bool(bypass), dst=bool(dst), lists=lists is not None, cut16=cut16, cut1=cut1,
                                sat=(bool((s < 0).any()), bool((s > 255).any())), d_min=int(d.min()), d_max=int(d.max()),
                                job=job if listed else None, unit=unit, coefs=coefs, qp_pred=state["pred"], qp_delta=state["delta"],
                                qpi=qp_y + offs[c] if c else None, qp_reset=state["reset"]))
            if listed:
                job += 1

        for (x, y, log2, depth, u) in hw.walk(seq, p):
            n, t = 1 << log2, u["t"]
            area = [(slice(y >> s, (y + n) >> s), slice(x >> s, (x + n) >> s)) for s in (0, 1, 1)]
            # ---- 8.6.1
            key = (x >> qg_log2 << qg_log2, y >> qg_log2 << qg_log2) if log2 < qg_log2 else (x, y)
            if key != state["qg"]:
                xq, yq = key
                first_in_slice = slice_of[y >> ctb, x >> ctb] != state["slice"]
                state["slice"] = slice_of[y >> ctb, x >> ctb]
                prev = slice_qp if first_in_slice and not (sw.get("qp_prev_not_reset") and state["qg"] is not None) else state["last_qp"]
                nb = []
                for (xn, yn) in ((xq - 1, yq), (xq, yq - 1)):
                    inside = xn >= 0 and yn >= 0 and (xn >> ctb, yn >> ctb) == (xq >> ctb, yq >> ctb)
                    if sw.get("qp_neighbours_outside_ctb") and xn >= 0 and yn >= 0 and slice_of[yn >> ctb, xn >> ctb] == slice_of[yq >> ctb, xq >> ctb]:
                        inside = True
                    nb.append(int(qpy[yn >> 2, xn >> 2]) if inside else prev)
                # reset: a slice that starts in mid-picture put qPY_PREV back to the slice QP from something else
                state.update(qg=key, pred=(nb[0] + nb[1] + 1) >> 1, delta=0, coded=False, prev_qp=prev,
                             reset=bool(first_in_slice and state["last_qp"] != slice_qp))
            count = 4 ** u.get("tu", 1 if t == "intra" and len(u["modes"]) == 4 else 0) if t in ("intra", "inter") else 0
            tus = hw.unit_tus(u, count) if count else []
            if seq.get("cu_qp_delta", 0) and not state["coded"] and any(tu[c] for tu in tus for c in (0, 1, 2)):
                state["coded"], state["delta"] = True, u.get("dqp", 0)
            qp_y = (state["pred"] + state["delta"] + 52) % 52
            qpy[y >> 2:(y + n) >> 2, x >> 2:(x + n) >> 2] = qp_y
            state["last_qp"] = qp_y
            # ---- prediction and residual
            if t == "pcm":
                for c, name in enumerate(("y", "cb", "cr")):
                    planes[c][area[c]] = u[name]
                continue
            if t == "skip":
                for c in range(3):
                    q = out[pl["l0"][0]][c][area[c]].astype(np.int64)
                    planes[c][area[c]] = q if p["kind"] == "P" else (q + out[pl["l1"][0]][c][area[c]] + 1) >> 1
                continue
            intra = t == "intra"
            bypass = u.get("bypass", 0)
            if not intra:
                for c in range(3):
                    s = n >> (c > 0)
                    pr = [ah.mc14(out[q[0]][c], x >> (c > 0), y >> (c > 0), s, s, q[1], c > 0) if q else None for q in (u.get("l0"), u.get("l1"))]
                    planes[c][area[c]] = ah.weighted(pr[0], pr[1], False, 6, None, None)
            nxn = intra and len(u["modes"]) == 4
            tu = u.get("tu", 1 if nxn else 0)
            lg = log2 - tu
            cm = ir.chroma_mode(u.get("chroma", 4), u["modes"][0]) if intra else None
            for i, e in enumerate(tus):
                ox, oy = ir.tu_origin(i, tu, log2)
                mode = (u["modes"][(i >> (2 * (tu - 1))) & 3] if nxn else u["modes"][0]) if intra else None
                if intra:
                    intra_block(0, x + ox, y + oy, 1 << lg, mode)
                if e[0]:
                    add(0, x + ox, y + oy, 1 << lg, e[0], qp_y, intra, 0 in e["tskip"], bypass, u, mode)
                if lg > 2:
                    cx, cy, cn = (x + ox) >> 1, (y + oy) >> 1, 1 << (lg - 1)
                elif i % 4 == 3:
                    cx, cy, cn = ((x + ox) & ~7) >> 1, ((y + oy) & ~7) >> 1, 4
                else:
                    continue
                for c in (1, 2):
                    if intra:
                        intra_block(c, cx, cy, cn, cm)
                    if e[c]:
                        add(c, cx, cy, cn, e[c], qp_y, intra, c in e["tskip"], bypass, u, cm)
        out.append(tuple(post(k, planes, dict(qpy=qpy)) if post else planes))
    return out, records


def describe(r):
    what = "bypass" if r["bypass"] else ("transform skip" if r["tskip"] else ("DST" if r["dst"] else "DCT"))
    return (f"picture {r['pic']} plane {('Y', 'Cb', 'Cr')[r['plane']]} {'intra' if r['intra'] else 'inter'} block at ({r['x']}, {r['y']}) {r['n']}x{r['n']} "
            f"{what} qP {r['qp']} {r['levels']} levels, last column {r['max_col']} last row {r['max_row']}, job {r['job']}")


def difference(seq, pics, frames, fmt, planes, records):
    """None when the display frames are the expected pictures, else a text that names the first picture, plane and sample that is wrong and, if a
    residual block holds it, that block's record"""
    if len(frames) != len(pics):
        return f"{len(frames)} frames, the script has {len(pics)}"
    w, h = seq["width"], seq["height"]
    order = sorted(range(len(pics)), key=lambda k: pics[k]["poc"])
    for d, k in enumerate(order):
        got = ir.unpack(seq, frames[d], fmt)
        for c in range(3):
            want = planes[k][c][:h >> (c > 0), :w >> (c > 0)]
            if np.array_equal(want, got[c]):
                continue
            j = np.argwhere(want != got[c])[0]
            text = (f"picture {k} ({pics[k]['kind']}, POC {pics[k]['poc']}) plane {('Y', 'Cb', 'Cr')[c]} sample ({j[1]}, {j[0]}): got {got[c][j[0], j[1]]} "
                    f"expected {want[j[0], j[1]]}, {int((want != got[c]).sum())} samples of the plane differ")
            for r in records:
                if r["pic"] == k and r["plane"] == c and r["x"] <= j[1] < r["x"] + r["n"] and r["y"] <= j[0] < r["y"] + r["n"]:
                    return text + "; in " + describe(r)
            return text + "; outside every residual block"
    return None
