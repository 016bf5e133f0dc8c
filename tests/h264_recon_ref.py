"""H.264 clauses 8.3.1 (Intra4x4), 8.3.2 (Intra8x8) and 8.5 (residual reconstruction) for the frame pictures of the scripted streams
(tests/scripted_h264.py), typed out from the clauses: plain integers and numpy, computed from the SCRIPT, never from a bitstream, and without opening
the oracle or the product.  Tables come from tests/spec_tables_h264.py only.  tests/analytic_expect.py calls this for the macroblock kinds i4 / i8
and for the coef=dict(...) of any macroblock; Intra16x16 and chroma PREDICTION stay with analytic_expect.intra16_luma / intra_chroma.

8.5.12 requires every scaled coefficient, intermediate and residual to fit 16 bits (bitDepth 8: -2^15 .. 2^15 - 1).  Beyond that decoders may differ,
so a case that leaves the range is a wrong case: ``check16`` ASSERTS it for every block of every case.

``wrong``: a set of wrong-on-purpose switches (SWITCHES).  Each restates one way a decoder can be wrong that no test without coded residuals or I_NxN
macroblocks would notice; tests/test_h264_recon_host.py asserts that each changes the expected picture of the case named beside it.
"""
import numpy as np

import scripted_h264 as sw
from spec_tables_h264 import (DEFAULT_4x4_INTER, DEFAULT_4x4_INTRA, DEFAULT_8x8_INTER, DEFAULT_8x8_INTRA, NORM_ADJUST_4x4, NORM_ADJUST_8x8, QPC_30_51,
                              ZIGZAG_4x4, ZIGZAG_8x8)

SWITCHES = (
    # scaling and transforms
    "list_transposed", "inter_uses_intra_list", "cr_uses_cb_list", "norm8_class_3_4_swapped", "no_rounding_below_24", "no_rounding_below_36",
    "shift_branch_at_24", "shift_branch_at_36", "chroma_dc_shift_5_first", "cr_uses_cb_offset", "columns_before_rows_4x4", "columns_before_rows_8x8",
    # prediction from reconstructed samples
    "i16_dc_without_hadamard", "i4_left_from_prediction",
    # edge samples and availability
    "upper_right_of_block_3_available", "upper_right_of_block_5_unavailable", "no_substitution_of_upper_right", "i8_first_sample_unfiltered_without_corner",
    "i8_unfiltered",
    # mode prediction
    "mode_max", "i8_neighbour_wrong_block", "n1_n2_swapped", "constrained_inter_stored_mode", "rem_without_plus_1")
MODE_SWITCHES = frozenset(SWITCHES[-5:])
INTRA = ("pcm", "i16", "i4", "i8")


def blk_xy(k):
    """6.4.3: upper left luma sample of luma4x4BlkIdx k"""
    return (k // 4 % 2) * 8 + (k % 4 % 2) * 4, (k // 4 // 2) * 8 + (k % 4 // 2) * 4


BLK_AT = {blk_xy(k): k for k in range(16)}


def check16(*arrays):
    for a in arrays:
        a = np.asarray(a)
        assert -32768 <= int(a.min()) and int(a.max()) <= 32767, f"outside 16 bits ({int(a.min())} .. {int(a.max())}): not a conforming block (8.5.12)"


# ---- 7.4.2.1.1, Table 7-2: the scaling lists in force ------------------------------------------------------------------------------------------
def scaling_matrices(seq, wrong=frozenset()):
    """The eight weightScale matrices ([row][column] arrays: 0 .. 2 Intra Y / Cb / Cr 4x4, 3 .. 5 Inter, 6 / 7 Intra / Inter Y 8x8) that the SPS and PPS
    of the script leave in force.  Absent matrix: Flat_16 (SPS) / the SPS's lists (PPS).  An absent list inside a present matrix: fall-back rule A
    (Default_* for lists 0, 3, 6, 7) in the SPS; in the PPS rule B (the SPS's list for 0, 3, 6, 7) when the SPS has a matrix, rule A when it has none
    (7.4.2.2, pic_scaling_list_present_flag); the other lists fall back to the list before them.  "default": UseDefaultScalingMatrixFlag."""
    default = [DEFAULT_4x4_INTRA] * 3 + [DEFAULT_4x4_INTER] * 3 + [DEFAULT_8x8_INTRA, DEFAULT_8x8_INTER]

    def resolve(lists, n, first):
        out = []
        for i in range(8):
            v = lists[i] if i < n else None
            if v is None:
                out.append(first[i] if i in (0, 3, 6, 7) else out[i - 1])
            elif isinstance(v, str):
                out.append(default[i])
            else:
                out.append(list(v))
        return out
    lists = [[16] * 16] * 6 + [[16] * 64] * 2
    sps = seq.get("sps_lists")
    if sps is not None:
        lists = resolve(sps, 8, default)
    if seq.get("pps_lists") is not None:
        lists = resolve(seq["pps_lists"], 6 + 2 * seq.get("transform8x8", 0), lists if sps is not None else default)
    out = []
    for i, v in enumerate(lists):
        n, zz = (4, ZIGZAG_4x4) if i < 6 else (8, ZIGZAG_8x8)
        m = np.zeros(n * n, np.int64)
        for k, val in enumerate(v):                                 # 8.5.6: the lists are in zig-zag order
            m[zz[k]] = val
        m = m.reshape(n, n)
        out.append(m.T.copy() if "list_transposed" in wrong else m)
    return out


def norm_adjust4(q):
    v = NORM_ADJUST_4x4[q]
    return np.array([[v[0] if i % 2 == 0 and j % 2 == 0 else (v[1] if i % 2 == 1 and j % 2 == 1 else v[2]) for j in range(4)] for i in range(4)], np.int64)


def norm8_class(i, j):
    if i % 4 == 0 and j % 4 == 0:
        return 0
    if i % 2 == 1 and j % 2 == 1:
        return 1
    if i % 4 == 2 and j % 4 == 2:
        return 2
    if (i % 4 == 0 and j % 2 == 1) or (i % 2 == 1 and j % 4 == 0):
        return 3
    if (i % 4 == 0 and j % 4 == 2) or (i % 4 == 2 and j % 4 == 0):
        return 4
    return 5


def norm_adjust8(q, wrong=frozenset()):
    v = NORM_ADJUST_8x8[q]
    swap = {3: 4, 4: 3} if "norm8_class_3_4_swapped" in wrong else {}
    return np.array([[v[swap.get(norm8_class(i, j), norm8_class(i, j))] for j in range(8)] for i in range(8)], np.int64)


def qp_chroma(qpy, off):
    """8.5.8 (Table 8-15): QPc of a plane from QPY and that plane's offset"""
    qpi = max(0, min(51, qpy + off))
    return qpi if qpi < 30 else QPC_30_51[qpi - 30]


# ---- 8.5.12 / 8.5.13 / 8.5.10 / 8.5.11 ---------------------------------------------------------------------------------------------------------
def scale(c, ls, qp, at, wrong):
    """8.5.12.1 (at = 24: the shift is qP / 6 - 4) and 8.5.13.1, 8.5.10 (at = 36: qP / 6 - 6)"""
    s = qp // 6 - at // 6
    if "shift_branch_at_%d" % at in wrong and s == 0:
        return (c * ls + 1) >> 1                                    # took the rounding branch of the qP / 6 below
    if s >= 0:
        return (c * ls) << s
    return (c * ls + (0 if "no_rounding_below_%d" % at in wrong else 1 << (-s - 1))) >> -s


def one_d4(d0, d1, d2, d3):
    e0, e1, e2, e3 = d0 + d2, d0 - d2, (d1 >> 1) - d3, d1 + (d3 >> 1)
    f = (e0 + e3, e1 + e2, e1 - e2, e0 - e3)
    check16(e0, e1, e2, e3, *f)
    return f


def one_d8(d):
    e = [d[0] + d[4], -d[3] + d[5] - d[7] - (d[7] >> 1), d[0] - d[4], d[1] + d[7] - d[3] - (d[3] >> 1), (d[2] >> 1) - d[6],
         -d[1] + d[7] + d[5] + (d[5] >> 1), d[2] + (d[6] >> 1), d[3] + d[5] + d[1] + (d[1] >> 1)]
    f = [e[0] + e[6], e[1] + (e[7] >> 2), e[2] + e[4], e[3] + (e[5] >> 2), e[2] - e[4], (e[3] >> 2) - e[5], e[0] - e[6], e[7] - (e[1] >> 2)]
    g = [f[0] + f[7], f[2] + f[5], f[4] + f[3], f[6] + f[1], f[6] - f[1], f[4] - f[3], f[2] - f[5], f[0] - f[7]]
    check16(*e, *f, *g)
    return g


def transform(d, wrong=frozenset()):
    """8.5.12.2 / 8.5.13.2: every ROW first, then every column; r = (. + 32) >> 6"""
    d = np.asarray(d, np.int64)
    check16(d)
    one = (lambda v: one_d4(*v)) if d.shape[0] == 4 else one_d8
    if "columns_before_rows_%dx%d" % d.shape in wrong:
        return transform(d.T, wrong - {"columns_before_rows_%dx%d" % d.shape}).T
    f = np.stack(one([d[:, j] for j in range(d.shape[1])]), axis=1)       # element j of every row -> every row transformed at once
    h = np.stack(one([f[i, :] for i in range(d.shape[0])]), axis=0)
    r = (h + 32) >> 6
    check16(r)
    return r


def intra16_dc(c, ls00, qp, wrong=frozenset()):
    """8.5.10: c = the 4x4 matrix of Intra16x16DCLevel; returns dcY, whose element (i, j) is the DC of the 4x4 block in row i, column j"""
    A = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], np.int64)
    c = np.asarray(c, np.int64)
    f = c if "i16_dc_without_hadamard" in wrong else A @ c @ A
    check16(f)
    dc = scale(f, ls00, qp, 36, wrong)
    check16(dc)
    return dc


def chroma_dc(c, ls00, qpc, wrong=frozenset()):
    """8.5.11.1 / .2 for 4:2:0: c = [[c0, c1], [c2, c3]]; returns dcC, element (i, j) = the DC of chroma block 2 i + j"""
    A = np.array([[1, 1], [1, -1]], np.int64)
    f = A @ np.asarray(c, np.int64).reshape(2, 2) @ A
    check16(f)
    dc = ((f * ls00) >> 5) << (qpc // 6) if "chroma_dc_shift_5_first" in wrong else ((f * ls00) << (qpc // 6)) >> 5
    check16(dc)
    return dc


def rescanned(c, scans):
    """coef as a decoder holds it whose inverse scan is scans = (perm4, perm8) (tests/h264_field_ref.decoder_scans): matrix[j] = script matrix[perm[j]].
    Every scanned block goes through it: luma 4x4 and 8x8, the Intra16x16 DC matrix, chroma AC (raster positions 1 .. 15); chroma DC has no scan."""
    p4, p8 = scans
    take = lambda v, p: [int(np.asarray(v).reshape(-1)[p[j]]) for j in range(len(p))]
    out = dict(c)
    if "y" in c:
        out["y"] = {k: take(v, p4) for k, v in c["y"].items()}
    if "y8" in c:
        out["y8"] = {k: take(v, p8) for k, v in c["y8"].items()}
    if "ydc" in c:
        out["ydc"] = take(c["ydc"], p4)
    if "cac" in c:
        out["cac"] = {k: take([0] + [int(q) for q in v], p4)[1:] for k, v in c["cac"].items()}
    return out


def mb_residual(seq, m, qpy, wrong=frozenset(), lists=None, scans=None):
    """(Ry 16x16, Rcb 8x8, Rcr 8x8): the residual r of every sample of macroblock m (zeros where nothing is coded), from m["coef"] (raster matrices).
    scans: None for a frame picture (8.5.6 / 8.5.7 with the zig-zag scans: the matrices are the script's); for a field picture the inverse field
    scans as a decoder applies them (tests/h264_field_ref.decoder_scans)."""
    R = [np.zeros((16, 16), np.int64), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)]
    c = m.get("coef")
    if not c:
        return R
    if scans is not None:
        c = rescanned(c, scans)
    W = lists if lists is not None else scaling_matrices(seq, wrong)
    intra = m["t"] in INTRA or "inter_uses_intra_list" in wrong
    t = m["t"]
    # ---- luma
    if t == "i8" or m.get("t8", 0):
        ls = W[6 if intra else 7] * norm_adjust8(qpy % 6, wrong)
        for b8, lv in c.get("y8", {}).items():
            d = scale(np.asarray(lv, np.int64).reshape(8, 8), ls, qpy, 36, wrong)
            x, y = (b8 & 1) * 8, (b8 >> 1) * 8
            R[0][y:y + 8, x:x + 8] = transform(d, wrong)
    else:
        ls = W[0 if intra else 3] * norm_adjust4(qpy % 6)
        dc = intra16_dc(np.asarray(c.get("ydc", [0] * 16)).reshape(4, 4), int(ls[0, 0]), qpy, wrong) if t == "i16" else None
        for k in range(16):
            lv = c.get("y", {}).get(k)
            x, y = blk_xy(k)
            if lv is None and (dc is None or dc[y // 4, x // 4] == 0):
                continue
            d = scale(np.asarray(lv if lv is not None else [0] * 16, np.int64).reshape(4, 4), ls, qpy, 24, wrong)
            if dc is not None:
                d[0, 0] = dc[y // 4, x // 4]
            R[0][y:y + 4, x:x + 4] = transform(d, wrong)
    # ---- chroma: each plane its own offset (8.5.8) and its own list
    offs = (seq.get("chroma_qp_off", 0), seq.get("second_chroma_qp_off", seq.get("chroma_qp_off", 0)))
    for pl in (0, 1):
        has_ac = [blk for blk in range(4) if (pl, blk) in c.get("cac", {})]
        cdc = c.get("cdc", ([0] * 4, [0] * 4))[pl]
        if not has_ac and not any(cdc):
            continue
        qpc = qp_chroma(qpy, offs[0 if "cr_uses_cb_offset" in wrong else pl])
        ls = W[(1 if intra else 4) + (0 if "cr_uses_cb_list" in wrong else pl)] * norm_adjust4(qpc % 6)
        dc = chroma_dc(cdc, int(ls[0, 0]), qpc, wrong)
        for blk in range(4):
            lv = [0] + [int(v) for v in c.get("cac", {}).get((pl, blk), [0] * 15)]
            d = scale(np.asarray(lv, np.int64).reshape(4, 4), ls, qpc, 24, wrong)
            d[0, 0] = dc[blk >> 1, blk & 1]
            x, y = (blk & 1) * 4, (blk >> 1) * 4
            R[1 + pl][y:y + 4, x:x + 4] = transform(d, wrong)
    return R


# ---- 8.3.1.2 / 8.3.2.2: the nine modes, for N = 4 and N = 8 ------------------------------------------------------------------------------------
def filter_reference(P, wrong=frozenset()):
    """8.3.2.2.1: p' from p.  P: {(x, y): sample} holding the AVAILABLE neighbours (upper right already substituted)."""
    if "i8_unfiltered" in wrong:
        return dict(P)
    top, left, corner = (0, -1) in P, (-1, 0) in P, (-1, -1) in P
    F = {}
    if top:
        F[(0, -1)] = (P[(-1, -1)] + 2 * P[(0, -1)] + P[(1, -1)] + 2) >> 2 if corner else (3 * P[(0, -1)] + P[(1, -1)] + 2) >> 2
        if not corner and "i8_first_sample_unfiltered_without_corner" in wrong:
            F[(0, -1)] = P[(0, -1)]
        for x in range(1, 15):
            F[(x, -1)] = (P[(x - 1, -1)] + 2 * P[(x, -1)] + P[(x + 1, -1)] + 2) >> 2
        F[(15, -1)] = (P[(14, -1)] + 3 * P[(15, -1)] + 2) >> 2
    if corner:                                                      # (the branches with one neighbour missing feed no mode a stream may use there:
        if top and left:                                            #  modes 4, 5, 6 alone read p'[-1, -1], and they need all three)
            F[(-1, -1)] = (P[(0, -1)] + 2 * P[(-1, -1)] + P[(-1, 0)] + 2) >> 2
        elif top:
            F[(-1, -1)] = (3 * P[(-1, -1)] + P[(0, -1)] + 2) >> 2
        elif left:
            F[(-1, -1)] = (3 * P[(-1, -1)] + P[(-1, 0)] + 2) >> 2
        else:
            F[(-1, -1)] = P[(-1, -1)]
    if left:
        F[(-1, 0)] = (P[(-1, -1)] + 2 * P[(-1, 0)] + P[(-1, 1)] + 2) >> 2 if corner else (3 * P[(-1, 0)] + P[(-1, 1)] + 2) >> 2
        if not corner and "i8_first_sample_unfiltered_without_corner" in wrong:
            F[(-1, 0)] = P[(-1, 0)]
        for y in range(1, 7):
            F[(-1, y)] = (P[(-1, y - 1)] + 2 * P[(-1, y)] + P[(-1, y + 1)] + 2) >> 2
        F[(-1, 7)] = (P[(-1, 6)] + 3 * P[(-1, 7)] + 2) >> 2
    return F


def predict(P, N, mode):
    """8.3.1.2.1 - .9 (N = 4) and 8.3.2.2.2 - .10 (N = 8): the N x N prediction from the neighbours P (N = 8: the filtered ones).  A mode whose
    neighbours are missing is a wrong script: KeyError."""
    out = np.zeros((N, N), np.int64)
    lg = {4: 2, 8: 3}[N]
    if mode == 2:
        top, left = (0, -1) in P, (-1, 0) in P
        s = sum(P[(x, -1)] for x in range(N)) if top else 0
        s += sum(P[(-1, y)] for y in range(N)) if left else 0
        out[:] = (s + N) >> (lg + 1) if top and left else ((s + N // 2) >> lg if top or left else 128)
        return out
    T = lambda x: P[(x, -1)]                                        # T(-1) is the corner, like L(-1)
    L = lambda y: P[(-1, y)]
    for y in range(N):
        for x in range(N):
            if mode == 0:
                v = T(x)
            elif mode == 1:
                v = L(y)
            elif mode == 3:                                         # Diagonal_Down_Left
                v = (T(2 * N - 2) + 3 * T(2 * N - 1) + 2) >> 2 if x == N - 1 and y == N - 1 else (T(x + y) + 2 * T(x + y + 1) + T(x + y + 2) + 2) >> 2
            elif mode == 4:                                         # Diagonal_Down_Right
                if x > y:
                    v = (T(x - y - 2) + 2 * T(x - y - 1) + T(x - y) + 2) >> 2
                elif x < y:
                    v = (L(y - x - 2) + 2 * L(y - x - 1) + L(y - x) + 2) >> 2
                else:
                    v = (T(0) + 2 * T(-1) + L(0) + 2) >> 2
            elif mode == 5:                                         # Vertical_Right
                z, i = 2 * x - y, x - (y >> 1)
                if z >= 0 and z % 2 == 0:
                    v = (T(i - 1) + T(i) + 1) >> 1
                elif z >= 0:
                    v = (T(i - 2) + 2 * T(i - 1) + T(i) + 2) >> 2
                elif z == -1:
                    v = (L(0) + 2 * T(-1) + T(0) + 2) >> 2
                else:
                    v = (L(y - 2 * x - 1) + 2 * L(y - 2 * x - 2) + L(y - 2 * x - 3) + 2) >> 2
            elif mode == 6:                                         # Horizontal_Down
                z, i = 2 * y - x, y - (x >> 1)
                if z >= 0 and z % 2 == 0:
                    v = (L(i - 1) + L(i) + 1) >> 1
                elif z >= 0:
                    v = (L(i - 2) + 2 * L(i - 1) + L(i) + 2) >> 2
                elif z == -1:
                    v = (L(0) + 2 * T(-1) + T(0) + 2) >> 2
                else:
                    v = (T(x - 2 * y - 1) + 2 * T(x - 2 * y - 2) + T(x - 2 * y - 3) + 2) >> 2
            elif mode == 7:                                         # Vertical_Left
                i = x + (y >> 1)
                v = (T(i) + T(i + 1) + 1) >> 1 if y % 2 == 0 else (T(i) + 2 * T(i + 1) + T(i + 2) + 2) >> 2
            else:                                                   # Horizontal_Up
                z, i = x + 2 * y, y + (x >> 1)
                if z > 2 * N - 3:
                    v = L(N - 1)
                elif z == 2 * N - 3:
                    v = (L(N - 2) + 3 * L(N - 1) + 2) >> 2
                elif z % 2 == 0:
                    v = (L(i) + L(i + 1) + 1) >> 1
                else:
                    v = (L(i) + 2 * L(i + 1) + L(i + 2) + 2) >> 2
            out[y, x] = v
    return out


NEEDS = {0: "T", 1: "L", 2: "", 3: "T", 4: "TLC", 5: "TLC", 6: "TLC", 7: "T", 8: "L"}       # neighbours a mode may not be without (8.3.1.2.x)


def sample_ok(sx, sy, N, idx, avail):
    """the sample (sx, sy) relative to the macroblock is available to block idx (decoding order) of size N"""
    if sy < 0:
        return avail(-1 if sx < 0 else (1 if sx > 15 else 0), -1)
    if sx < 0:
        return avail(-1, 0)
    return sx <= 15 and (BLK_AT[(sx & ~3, sy & ~3)] if N == 4 else (sy // 8) * 2 + sx // 8) < idx


def pattern(bx, by, N, idx, avail):
    """which of T (above), L (left), C (corner), R (upper right) block idx has"""
    return "".join(ch for ch, (sx, sy) in (("T", (bx, by - 1)), ("L", (bx - 1, by)), ("C", (bx - 1, by - 1)), ("R", (bx + N, by - 1)))
                   if sample_ok(sx, sy, N, idx, avail))


def mb_avail(seq, p, a):
    """avail(dx, dy) of macroblock a of picture p: the macroblock (dx, dy) from it may be used for intra prediction -- in the picture, in this slice,
    decoded, and, under constrained_intra_pred_flag, not inter (8.3.1.2, 8.3.2.2, 8.3.3, 8.3.4)"""
    mbw = (seq["width"] + 15) // 16
    mbh = (seq["height"] + 15) // 16
    step = sw.layout_step(seq, p)

    def avail(dx, dy):
        n = a + dx + dy * mbw
        if not (0 <= a % mbw + dx < mbw and a - a % step <= n < a):
            return False
        return not (seq.get("constrained_intra", 0) and p["mbs"][n]["t"] not in INTRA)
    return avail


def neighbours(Y, Ysrc_left, X0, Y0, bx, by, N, idx, avail, wrong=frozenset(), stats=None):
    """The available neighbours {(x, y): sample} of the N x N block at (bx, by) of the macroblock at (X0, Y0), which is block `idx` in decoding order
    (6.4.11.4 / 6.4.11.2 with 6.4.12): a sample left of the macroblock belongs to A, above it to B, above and right of it to C, above and left to D;
    right of the macroblock and not above it: never available; inside it: available when its block precedes this one in decoding order.
    avail(dx, dy): that neighbouring macroblock can be used for intra prediction.  Returns (P, pattern of availability "TLCR")."""
    ok = lambda sx, sy: sample_ok(sx, sy, N, idx, avail)
    P = {}
    for x in range(-1, 2 * N):
        sx, sy = bx + x, by - 1
        good = ok(sx, sy)
        if N == 4 and x >= N:
            if "upper_right_of_block_3_available" in wrong and idx == 3:
                good = True
            if "upper_right_of_block_5_unavailable" in wrong and idx == 5:
                good = False
        if good:
            P[(x, -1)] = int(Y[Y0 + sy, X0 + sx])
    for y in range(N):
        if ok(bx - 1, by + y):
            src = Ysrc_left if bx > 0 else Y                        # (the wrong-on-purpose source only inside the macroblock)
            P[(-1, y)] = int(src[Y0 + by + y, X0 + bx - 1])
    pat = "".join(ch for ch, key in (("T", (0, -1)), ("L", (-1, 0)), ("C", (-1, -1)), ("R", (N, -1))) if key in P)
    if (N, -1) not in P and (N - 1, -1) in P:                       # 8.3.1.2 / 8.3.2.2: p[N - 1, -1] stands in for the missing upper right samples
        for x in range(N, 2 * N):
            P[(x, -1)] = 128 if "no_substitution_of_upper_right" in wrong else P[(N - 1, -1)]
    if stats is not None:
        stats.add(("pattern", N, pat))
    return P, pat


def intra_nxn_luma(Y, X0, Y0, m, modes, R, avail, wrong=frozenset(), stats=None):
    """Intra4x4 / Intra8x8 luma of one macroblock, written into Y: block after block in decoding order, each predicted from the samples CONSTRUCTED before
    it (8.3.1.2: "the ... constructed samples prior to the deblocking filter process"), u = Clip1(pred + r) (8.5.14)."""
    N = 4 if m["t"] == "i4" else 8
    Ypred = Y.copy() if "i4_left_from_prediction" in wrong else Y
    for idx, mode in enumerate(modes):
        bx, by = blk_xy(idx) if N == 4 else ((idx & 1) * 8, (idx >> 1) * 8)
        P, pat = neighbours(Y, Ypred, X0, Y0, bx, by, N, idx, avail, wrong, stats)
        assert all(ch in pat for ch in NEEDS[mode]), f"mode {mode} of block {idx} lacks a neighbour it needs (has {pat!r}): a wrong script"
        if N == 8:
            P = filter_reference(P, wrong)
        pred = predict(P, N, mode)
        v = pred + R[by:by + N, bx:bx + N]
        if stats is not None:
            stats.add(("mode", N, idx, mode))
            if R[by:by + N, bx:bx + N].any():
                stats.add(("residual", N, idx))
            if v.min() < 0:
                stats.add(("clip1_at_0", m["t"]))
            if v.max() > 255:
                stats.add(("clip1_at_255", m["t"]))
            if mode in (3, 7):
                stats.add(("upper_right_mode", N, idx, "R" in pat))
        Y[Y0 + by:Y0 + by + N, X0 + bx:X0 + bx + N] = np.clip(v, 0, 255)
        if Ypred is not Y:
            Ypred[Y0 + by:Y0 + by + N, X0 + bx:X0 + bx + N] = np.clip(pred, 0, 255)
            rest = np.ones_like(Y, bool)
            rest[Y0:Y0 + 16, X0:X0 + 16] = False
            Ypred[rest] = Y[rest]


# ---- 8.3.1.1 / 8.3.2.1: the mode prediction, and what a decoder makes of the coded flags --------------------------------------------------------
def mode_tables(seq, p, wrong=frozenset(), stats=None):
    """(coded, decoded).  coded[a] = [(predIntraNxNPredMode, prev_intraNxN_pred_mode_flag, rem_intraNxN_pred_mode | None)] of every block of every I_NxN
    macroblock a, derived by the clauses from the script's modes; decoded[a] = the modes a decoder derives from these flags -- the script's own, unless
    a switch of ``wrong`` makes the decoder's derivation wrong."""
    mbw = (seq["width"] + 15) // 16
    mbs = p["mbs"]
    kind = p["kind"]
    step = sw.layout_step(seq, p)
    constrained = seq.get("constrained_intra", 0)

    def derive(store, a, idx, N, wr):
        x, y = blk_xy(idx) if N == 4 else ((idx & 1) * 8, (idx >> 1) * 8)
        got = []
        for name, (nx, ny) in (("A", (x - 1, y)), ("B", (x, y - 1))):
            dx, dy = (-1 if nx < 0 else 0), (-1 if ny < 0 else 0)
            n = a + dx + dy * mbw
            inside = (a % mbw + dx >= 0) and n >= 0 and n >= a - a % step
            if not inside:
                if stats is not None:
                    stats.add(("neighbour", N, "unavailable"))
                return 2                                            # dcPredModePredictedFlag
            mb = mbs[n]
            nx, ny = nx % 16, ny % 16
            if mb["t"] not in INTRA and constrained:
                if stats is not None:
                    stats.add(("neighbour", N, "inter_constrained"))
                if "constrained_inter_stored_mode" not in wr:
                    return 2                                        # dcPredModePredictedFlag
            if stats is not None:
                stats.add(("neighbour", N, mb["t"] if mb["t"] in INTRA else "inter"))
            if mb["t"] not in ("i4", "i8"):
                got.append(2)
            elif N == 4:
                blk = BLK_AT[(nx & ~3, ny & ~3)]
                got.append(store[n][blk] if mb["t"] == "i4" else store[n][(blk >> 2) ^ (1 if "i8_neighbour_wrong_block" in wr else 0)])
            else:
                b8 = (ny // 8) * 2 + nx // 8
                nn = {"A": 1, "B": 2}[name] if "n1_n2_swapped" not in wr else {"A": 2, "B": 1}[name]
                got.append(store[n][b8] if mb["t"] == "i8" else store[n][b8 * 4 + nn])
        return max(got) if "mode_max" in wr else min(got)

    coded, decoded, true = {}, {}, {}
    for a, m in enumerate(mbs):
        if m["t"] not in ("i4", "i8"):
            continue
        N = 4 if m["t"] == "i4" else 8
        true[a], decoded[a], coded[a] = [], [], []
        for idx, mode in enumerate(m["modes"]):
            pred = derive(true, a, idx, N, frozenset())
            flag, rem = (1, None) if mode == pred else (0, mode if mode < pred else mode - 1)
            if stats is not None:
                stats.add(("coded", N, "predicted" if flag else ("below" if mode < pred else "above")))
            coded[a].append((pred, flag, rem))
            true[a].append(mode)
            wpred = derive(decoded, a, idx, N, wrong)
            decoded[a].append(wpred if flag else (rem if rem < wpred or "rem_without_plus_1" in wrong else rem + 1))
        assert wrong & MODE_SWITCHES or decoded[a] == list(m["modes"])
    return coded, decoded
