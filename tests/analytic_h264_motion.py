"""Scripted H.264 cases for motion vector derivation and direct prediction (clause 8.4.1): name -> builder(width, height) -> (seq, pics) for
tests/scripted_h264.py.  The inter macroblocks state SYNTAX (mb_type, sub_mb_type, ref_idx, mvd); tests/h264_motion_ref.py derives the vectors and
tests/analytic_expect.py samples with them.  Reference pictures are seeded noise, so that any wrong vector shows; the deblocking filter is off except
in reach_chain (and in the deblocked variants the GPU test sends through chain launches); one slice per picture unless a case says otherwise.

Every case at 96x80 (6 x 5 macroblocks) and 90x70 (cropped from 96x80: reference samples outside the cropped picture are still reference samples, and
the picture border at which coordinates clamp is the CODED picture's), window_borders also at 32x32.  At most 8 pictures per stream.

Where a case needs a VECTOR at a place (window_borders; the colocated pictures of the direct cases), the macroblock is a slice of its own (layout "mb"),
so that no other macroblock decides its predictor, and ``aim`` finds the mvd that reaches the vector by asking the restatement for the predictor of
each sub-partition in turn.  What the decoders make of that mvd is still held to the restatement by the oracle and by the hand-worked tests.
"""
import functools

import numpy as np

import analytic_cases as ac
import analytic_expect as ae
import analytic_h264_recon as hr
import h264_motion_ref as mr
import scripted_h264 as sw
from spec_tables_h264 import MB_TYPE_B, MB_TYPE_P, SUB_MB_TYPE_B, SUB_MB_TYPE_P

SIZES = [(96, 80), (90, 70)]
P_SUBS = [q[0] for q in SUB_MB_TYPE_P]
B_SUBS = [q[0] for q in SUB_MB_TYPE_B]
B_TYPES = [q[0] for q in MB_TYPE_B]
DC = dict(t="i16", mode=2, cmode=0)                                 # an intra macroblock that any neighbourhood allows


def distinct_mvds(rng, n, lim):
    """n non-zero, mutually different mvds"""
    out = []
    while len(out) < n:
        d = (int(rng.integers(-lim, lim + 1)), int(rng.integers(-lim, lim + 1)))
        if d != (0, 0) and d not in out:
            out.append(d)
    return out


def mv_mb(rng, kind, name, n, sub=None, lim=9, ref=None):
    """A macroblock of the given type with random ref_idx below n = (n0, n1) (or `ref` for every partition) and distinct non-zero mvds"""
    m = dict(t="mv", mb=name)
    if sub is not None:
        m["sub"] = list(sub)
    if name == "B_Direct_16x16":
        return m
    _, _, modes, counts, _, _ = sw.mv_shape(kind, m)
    pool = distinct_mvds(rng, 2 * sum(counts), lim)
    m["ref"], m["mvd"] = ([], []), ([], [])
    for l in (0, 1):
        for mode, c in zip(modes, counts):
            if mode in (("L0", "Bi"), ("L1", "Bi"))[l]:
                m["ref"][l].append(0 if name == "P_8x8ref0" else (int(rng.integers(0, n[l])) if ref is None else ref))
                m["mvd"][l].append([pool.pop() for _ in range(c)])
            else:
                m["ref"][l].append(None)
                m["mvd"][l].append(None)
    return m


def aim(kind, m, want, n=(1, 1)):
    """The macroblock m (a slice of its own) with the mvds that give the vectors want[l][partition][sub-partition]: one sub-partition after the other,
    the restatement says what the predictor is while the later mvds are still zero."""
    _, _, modes, counts, _, _ = sw.mv_shape(kind, m)
    m = dict(m, mvd=tuple([None if want[l][i] is None else [(0, 0)] * counts[i] for i in range(len(modes))] for l in (0, 1)))
    seq = dict(width=16, height=16, num_ref_frames=4)
    refs = [ac.flat_pic(1, 1, 0, 0, 0, "I" if k == 0 else "P", 2 * k) for k in range(max(n))]
    # B: as many pictures after as before, so that both lists are n long
    pics = refs + [ac.flat_pic(1, 1, 0, 0, 0, "P", 40 + 2 * k) for k in range(n[1] if kind == "B" else 0)]
    cur = dict(kind=kind, poc=20, layout="mb", num_ref=n, mbs=[m])
    for i in range(len(modes)):
        for j in range(counts[i]):
            for l in (0, 1):
                if want[l][i] is None:
                    continue
                got = mr.derive(seq, pics + [cur])[0][-1][0]
                x, y = sw.mv_shape(kind, m)[5][i][j][:2]
                mv = got[(y // 4) * 4 + x // 4][l][1]
                m["mvd"][l][i][j] = (want[l][i][j][0] - mv[0], want[l][i][j][1] - mv[1])
    return m


def noise(rng, w, h, kind, poc, **kw):
    return ac.noise_pic(rng, *ac.dims(w, h), kind, poc, **kw)


# ---- p_partitions -------------------------------------------------------------------------------------------------------------------------------
def p_partitions(w, h):
    """Every P mb_type and sub_mb_type, two references, non-zero and mutually different mvds in every sub-partition, random ref_idx: the single-match
    rule, the median and the four directional rules each meet an equal and a different reference index.  One macroblock in nine is intra."""
    rng = np.random.default_rng(0xD100)
    mbw, mbh = ac.dims(w, h)
    pics = [noise(rng, w, h, "I", 0), noise(rng, w, h, "P", 2)]
    forms = [("P_L0_16x16", None), ("P_L0_L0_16x8", None), ("P_L0_L0_8x16", None)] + [("P_8x8", [s] * 4) for s in P_SUBS]
    forms += [("P_8x8", P_SUBS), ("P_8x8", P_SUBS[::-1]), ("P_8x8ref0", P_SUBS[1:] + P_SUBS[:1]), ("P_8x8ref0", ["P_L0_8x8"] * 4)]
    for k in range(3):
        mbs = []
        for a in range(mbw * mbh):
            name, sub = forms[(a + 4 * k) % len(forms)]
            mbs.append(dict(DC) if a % 9 == 4 + k else mv_mb(rng, "P", name, (2, 1), sub))
        pics.append(dict(kind="P", poc=4 + 2 * k, layout="pic", mbs=mbs))
    return dict(width=w, height=h, num_ref_frames=2), pics


# ---- p_neighbours -------------------------------------------------------------------------------------------------------------------------------
def p_neighbours(w, h):
    """Neighbour availability: one slice per picture (C unavailable at the right edge and for later partitions: D), slices of 8 macroblocks (a slice
    begins in mid-row: A unavailable there, B / C / D in another slice for some of its macroblocks), one slice per row (B, C and D all in another
    slice: only A), and intra macroblocks scattered so that each of A, B, C is intra somewhere."""
    rng = np.random.default_rng(0xD200)
    mbw, mbh = ac.dims(w, h)
    pics = [noise(rng, w, h, "I", 0), noise(rng, w, h, "P", 2)]
    forms = [("P_L0_16x16", None), ("P_L0_L0_16x8", None), ("P_L0_L0_8x16", None), ("P_8x8", P_SUBS), ("P_L0_16x16", None), ("P_8x8", ["P_L0_4x4"] * 4)]
    for k, layout in enumerate(("pic", 8, "row")):
        mbs = []
        for a in range(mbw * mbh):
            name, sub = forms[(a * 5 + k) % len(forms)]
            mbs.append(dict(DC) if (a + 3 * k) % 7 == 3 else mv_mb(rng, "P", name, (2, 1), sub))
        pics.append(dict(kind="P", poc=4 + 2 * k, layout=layout, mbs=mbs))
    return dict(width=w, height=h, num_ref_frames=2), pics


# ---- p_skip -------------------------------------------------------------------------------------------------------------------------------------
def p_skip(w, h):
    """Runs of P_Skip between P_L0_16x16 and P_8x8 macroblocks (the parser's short route and its general route alternate and read each other's
    neighbour data): skipped macroblocks in the first row and column (A or B unavailable: zero), below or beside a skipped macroblock (refIdx 0 and a
    zero vector: zero), among moving neighbours (the 16x16 predictor), a run across a row end, a run that ends the slice and the picture"""
    rng = np.random.default_rng(0xD300)
    mbw, mbh = ac.dims(w, h)
    n = mbw * mbh
    pics = [noise(rng, w, h, "I", 0), noise(rng, w, h, "P", 2)]
    for k, layout in enumerate(("pic", 8, "pic")):
        mbs = []
        for a in range(n):
            r = (a * 7 + 3 * k) % 10
            if k == 0 and a < mbw + 2:
                # a moving first row, so that the second row's skipped macroblocks are predicted
                mbs.append(mv_mb(rng, "P", "P_L0_16x16", (2, 1), ref=0) if a != 3 else dict(t="skip"))
            elif a >= n - 3 or a % mbw == mbw - 1 and k != 1 or (a % mbw == 0 and k == 2) or r < 4:
                mbs.append(dict(t="skip"))
            elif r < 7:
                mbs.append(mv_mb(rng, "P", "P_L0_16x16", (2, 1), ref=0 if r < 6 else 1))
            else:
                mbs.append(mv_mb(rng, "P", "P_8x8", (2, 1), [P_SUBS[(a + j) % 4] for j in range(4)]))
        pics.append(dict(kind="P", poc=4 + 2 * k, layout=layout, mbs=mbs))
    return dict(width=w, height=h, num_ref_frames=2), pics


# ---- b_partitions -------------------------------------------------------------------------------------------------------------------------------
WP = dict(ld_y=5, ld_c=4, l0=[dict(y=(20, 3), c=((18, -2), (14, 1))), None], l1=[dict(y=(12, -4), c=None), dict(y=(40, 2), c=((10, 5), (22, -3)))])


def b_partitions(mode):
    def build(w, h):
        """Every row of Table 7-14 and every B sub_mb_type once in each quadrant (spatial direct among them), two entries in each list; quadrants that
        use only list 1; macroblocks whose four quadrants use four different (list, reference) combinations."""
        rng = np.random.default_rng(0xD400 + mode)
        mbw, mbh = ac.dims(w, h)
        n = mbw * mbh
        pics = [noise(rng, w, h, "I", 0), noise(rng, w, h, "P", 16)]
        forms = [(t, None) for t in B_TYPES[:22]] + [("B_8x8", [B_SUBS[(j + 3 * q) % 13] for q in range(4)]) for j in range(13)]
        four = dict(t="mv", mb="B_8x8", sub=["B_L0_8x8", "B_L0_8x8", "B_L1_8x8", "B_L1_8x8"], ref=([0, 1, None, None], [None, None, 0, 1]))
        for k in range(3):
            mbs = []
            for a in range(n):
                name, sub = forms[(a + n * k) % len(forms)]
                if k == 2 and a % 6 == 5:
                    pool = distinct_mvds(rng, 4, 9)
                    mbs.append(dict(four, mvd=([[pool[0]], [pool[1]], None, None], [None, None, [pool[2]], [pool[3]]])))
                else:
                    mbs.append(mv_mb(rng, "B", name, (2, 2), sub))
            p = dict(kind="B", poc=4 + 4 * k, layout="pic", mbs=mbs)
            if mode == 1:
                p["wp"] = WP
            pics.append(p)
        return dict(width=w, height=h, num_ref_frames=2, profile=77, weighted_bipred=mode), pics
    return build


# ---- direct prediction --------------------------------------------------------------------------------------------------------------------------
COL_VECTORS = [(1, 0), (2, 0), (-1, 0), (-2, 0), (0, 1), (0, 2), (0, -1), (0, -2), (1, -1), (0, 0)]


def col_p_picture(rng, w, h, poc, n0, big=False):
    """A P picture for later colocated use, every macroblock a slice of its own so that its vectors are the ones written here: 16x16 macroblocks
    with each of COL_VECTORS at refIdx 0 and at refIdx 1, an intra macroblock, and P_8x8 macroblocks of 4x4 sub-partitions whose sixteen vectors
    lie around the +-1 limit of colZeroFlag (big: vectors of tens of samples instead, for the scaling of temporal direct)"""
    mbw, mbh = ac.dims(w, h)
    mbs = []
    for a in range(mbw * mbh):
        r = a % 3
        if a == 7:
            mbs.append(dict(DC))
        elif r == 0 and not big:
            v = COL_VECTORS[(a // 3) % len(COL_VECTORS)]
            ref = (a // 3) // len(COL_VECTORS) % 2 if n0 > 1 else 0
            mbs.append(dict(t="mv", mb="P_L0_16x16", ref=([ref if a != 3 else min(1, n0 - 1)], [None]), mvd=([[v]], [None])))
        elif r == 0:
            mbs.append(mv_mb(rng, "P", ("P_L0_16x16", "P_L0_L0_16x8", "P_L0_L0_8x16")[(a // 3) % 3], (n0, 1), lim=150))
        else:
            ref = int(rng.integers(0, n0)) if r == 2 else 0
            lim = 150 if big else 2
            want = [[(int(rng.integers(-lim, lim + 1)), int(rng.integers(-lim, lim + 1))) for _ in range(4)] for _ in range(4)]
            m = dict(t="mv", mb="P_8x8", sub=["P_L0_4x4"] * 4, ref=([ref] * 4, [None] * 4))
            mbs.append(aim("P", m, (want, [None] * 4), (n0, 1)))
    return dict(kind="P", poc=poc, layout="mb", mbs=mbs)


def direct_mbs(rng, n, nrefs, step):
    """A B picture of B_Skip, B_Direct_16x16 and B_8x8 with direct quadrants between macroblocks that use list 0 only, list 1 only and both, and intra
    macroblocks: the neighbours of a direct macroblock give both lists, one list or none"""
    mbs = []
    for a in range(n):
        r = int(rng.integers(0, 12))
        if r < 3:
            mbs.append(dict(t="skip"))
        elif r < 5:
            mbs.append(dict(t="mv", mb="B_Direct_16x16"))
        elif r < 8:
            sub = [("B_Direct_8x8", B_SUBS[int(rng.integers(1, 13))])[int(rng.integers(0, 3)) == 0] for _ in range(4)]
            sub[int(rng.integers(0, 4))] = "B_Direct_8x8"
            mbs.append(mv_mb(rng, "B", "B_8x8", nrefs, sub))
        elif r == 11:
            mbs.append(dict(DC))
        else:
            mbs.append(mv_mb(rng, "B", ("B_L0_16x16", "B_L1_16x16", "B_Bi_16x16")[r - 8], nrefs, lim=3))
    # rows that use one list only, so that direct macroblocks below and beside them find one list
    for a in range(step, min(n, 2 * step)):
        if a % 2 == 0:
            mbs[a] = mv_mb(rng, "B", "B_L0_16x16" if a % 4 == 0 else "B_L1_16x16", nrefs, lim=3)
    return mbs


def b_spatial_direct(inference):
    def build(w, h):
        """Spatial direct prediction.  Pictures: I (0), P noise (4), the colocated P picture (12) with list 0 = [P(4), I(0)], then B pictures at 6, 8, 10
        with list 0 = [P(4), I(0)] and list 1 = [P(12)]: one slice per picture, slices of 8, one slice per row (whose first macroblock has no
        neighbour: both refIdx negative)."""
        rng = np.random.default_rng(0xD500 + inference)
        mbw, mbh = ac.dims(w, h)
        pics = [noise(rng, w, h, "I", 0), noise(rng, w, h, "P", 4), col_p_picture(rng, w, h, 12, 2)]
        for k, layout in enumerate(("pic", 8, "row")):
            pics.append(dict(kind="B", poc=6 + 2 * k, layout=layout, mbs=direct_mbs(rng, mbw * mbh, (2, 1), mbw)))
        return dict(width=w, height=h, num_ref_frames=3, profile=77, direct_8x8_inference=inference), pics
    return build


def b_temporal_direct(inference):
    def build(w, h):
        """Temporal direct prediction (direct_spatial_mv_pred_flag 0).  Decode order: I (0), P noise (4), P noise (8), P (16) with vectors of tens of
        samples over three references, a REFERENCE B picture (12) whose macroblocks use list 0, list 1 only, or both, then B (10): colocated in
        B(12), the picture a list-1-only block referred to, P(16), is entry 4 of list 0, tb / td = -6 / -4; B (14): colocated in P(16), list 0 begins
        with B(12) so every mapped refIdxL0 is refIdxCol + 1, tb / td = 6 / 8, 10 / 12, 14 / 16 (non-dyadic factors); B (18): list 1 is list 0 with
        the first two entries swapped, colocated in B(12), tb / td = 2 / -4 for its list-1-only blocks (a negative factor), 10 / 4 beyond."""
        rng = np.random.default_rng(0xD600 + inference)
        mbw, mbh = ac.dims(w, h)
        n = mbw * mbh
        pics = [noise(rng, w, h, "I", 0), noise(rng, w, h, "P", 4), noise(rng, w, h, "P", 8), col_p_picture(rng, w, h, 16, 3, big=True)]
        mbs = []
        for a in range(n):
            name = ("B_L1_16x16", "B_L0_16x16", "B_Bi_16x16", "B_8x8", "B_L1_L1_16x8", "B_L0_L1_8x16")[a % 6]
            sub = [("B_L1_4x4", "B_L0_8x8", "B_L1_8x4", "B_Bi_4x8")[(a // 6 + j) % 4] for j in range(4)] if name == "B_8x8" else None
            mbs.append(dict(DC) if a == 13 else mv_mb(rng, "B", name, (3, 1), sub, lim=90))
        pics.append(dict(kind="B", poc=12, is_ref=True, layout="mb", direct_spatial=0, mbs=mbs))
        for poc, layout in ((10, "pic"), (14, 8), (18, "pic")):
            l0n = {10: 5, 14: 4, 18: 5}[poc]
            nrefs = (l0n, 2 if poc != 14 else 1)
            pics.append(dict(kind="B", poc=poc, layout=layout, direct_spatial=0, num_ref=nrefs, mbs=direct_mbs(rng, n, nrefs, mbw)))
        return dict(width=w, height=h, num_ref_frames=5, profile=77, direct_8x8_inference=inference), pics
    return build


# ---- window_borders -----------------------------------------------------------------------------------------------------------------------------
def window_origin(X8, Y8, mv):
    """upper left sample of the 13x13 window that the six-tap filter of an 8x8 block at (X8, Y8) reads for the vector mv"""
    return X8 + (mv[0] >> 2) - 2, Y8 + (mv[1] >> 2) - 2


def window_borders(w, h, alter_cropped=False):
    """The vectors of the quadrants place the 13x13 window of an 8x8 block exactly at and one sample past each border of the CODED picture (xi = 0 /
    -1, xi + 13 = W / W + 1, likewise in y): per side once with every quadrant inside and one of them touching, once with exactly one quadrant out by
    one.  P macroblocks: P_8x8 of 8x8 sub-partitions, and with one quadrant of 4x4 sub-partitions one of which deviates by a quarter sample; B
    macroblocks: B_8x8 of L0 / L1 / Bi 8x8 quadrants, and one with a Bi 4x4 quadrant that deviates.  Further macroblocks reach further outside than the
    picture is wide.  alter_cropped: other samples in the reference pictures where the cropped 90x70 picture does not show them."""
    rng = np.random.default_rng(0xD700)
    mbw, mbh = ac.dims(w, h)
    W, H, n = mbw * 16, mbh * 16, mbw * mbh
    pics = [noise(rng, w, h, "I", 0), noise(rng, w, h, "P", 16)]
    if alter_cropped:
        for p in pics:
            for a, m in enumerate(p["mbs"]):
                if a % mbw == mbw - 1:
                    m["y"][:, 16 - (W - w):] ^= 0x55
                if a // mbw == mbh - 1:
                    m["y"][16 - (H - h):, :] ^= 0x55
    sides = [("x", 0), ("y", 0), ("x", 1), ("y", 1)]
    for kind in ("P", "B", "P", "B"):
        mbs = []
        for a in range(n):
            X, Y = (a % mbw) * 16, (a // mbw) * 16
            s = a + n * ((len(pics) - 2) // 2)                      # the scenarios go on where the picture of this kind before stopped
            axis, far_side = sides[s % 4]
            out_by_one, deviate = (s // 4) % 2, (s // 8) % 2
            sel = int(rng.integers(0, 4))
            lists = [0] if kind == "P" else [[0], [1], [0, 1]][a % 3]
            want = ([None] * 4, [None] * 4)
            sub = []
            for g in range(4):
                X8, Y8 = X + (g & 1) * 8, Y + (g >> 1) * 8
                gl = lists if kind == "P" or g == sel else [[0], [1], [0, 1]][(a + g) % 3]
                four = deviate and g == (sel + 1) % 4
                sub.append({(0,): "L0", (1,): "L1", (0, 1): "Bi"}[tuple(gl)])
                for l in gl:
                    xi, yi = int(rng.integers(0, W - 12)), int(rng.integers(0, H - 12))
                    if a % 11 == 10:
                        xi, yi = (-W - 40, H + W + 30, xi)[g % 3], (yi, -H - 50, 2 * H)[g % 3]      # further outside than the picture is wide
                    elif g == sel and l == gl[0]:
                        lim = (W if axis == "x" else H) - 13 if far_side else 0
                        v = lim + (1 if far_side else -1) * out_by_one
                        xi, yi = (v, yi) if axis == "x" else (xi, v)
                    mv = (4 * (xi + 2 - X8) + int(rng.integers(0, 4)), 4 * (yi + 2 - Y8) + int(rng.integers(0, 4)))
                    assert window_origin(X8, Y8, mv) == (xi, yi)
                    want[l][g] = [mv] * 4 if four else [mv]
                    if four:
                        want[l][g][2] = (mv[0] ^ 1, mv[1])          # the same whole sample, a quarter sample beside
                sub[-1] = ("P_L0_" if kind == "P" else "B_%s_" % sub[-1]) + ("4x4" if four else "8x8")
            nrefs = (2, 1) if kind == "P" else (1, 1)
            m = dict(t="mv", mb=kind + "_8x8", sub=sub, ref=tuple([None if want[l][g] is None else int(rng.integers(0, nrefs[l])) for g in range(4)] for l in (0, 1)))
            mbs.append(aim(kind, m, want, nrefs))
        pics.append(dict(kind=kind, poc=2 + 2 * (len(pics) - 2), layout="mb", is_ref=False, mbs=mbs))
    return dict(width=w, height=h, num_ref_frames=2, profile=77), pics


# ---- reach_chain --------------------------------------------------------------------------------------------------------------------------------
REACH_BLOCK = (2, 1)                                                # quadrant 2, sub-partition 1: the block at (4, 8), on no edge of the macroblock


def reach_chain(w, h):
    """P pictures with the deblocking filter ON, each predicting from the one before (one reference).  In every picture ONE 4x4 sub-partition, inside
    its macroblock and not the first of its quadrant, carries the picture's largest downward and rightward vector: what a chain launch has to wait
    for in the picture before is decided by that block alone."""
    rng = np.random.default_rng(0xD800)
    mbw, mbh = ac.dims(w, h)
    pics = [noise(rng, w, h, "I", 0, deblock=(0, 0, 0))]
    forms = [("P_L0_16x16", None), ("P_8x8", P_SUBS), ("P_L0_L0_16x8", None), ("P_L0_L0_8x16", None), ("P_8x8", ["P_L0_8x8"] * 4)]
    for k in range(5):
        far = (7 * k + 8) % (mbw * mbh)
        mbs = []
        for a in range(mbw * mbh):
            name, sub = forms[(a + k) % len(forms)]
            m = mv_mb(rng, "P", name, (1, 1), sub, lim=5)
            if a == far:
                m = mv_mb(rng, "P", "P_8x8", (1, 1), ["P_L0_8x8", "P_L0_8x4", "P_L0_4x4", "P_L0_4x8"], lim=5)
                m["mvd"][0][REACH_BLOCK[0]][REACH_BLOCK[1]] = (4 * 37 + 2, 4 * 33 + 1)
            elif a % 8 == 5:
                m = dict(t="skip")
            mbs.append(m)
        pics.append(dict(kind="P", poc=2 + 2 * k, layout="pic", deblock=(0, 0, 0), mbs=mbs))
    return dict(width=w, height=h, num_ref_frames=1), pics


CASES = {
    "p_partitions": p_partitions, "p_neighbours": p_neighbours, "p_skip": p_skip,
    "b_partitions": b_partitions(0), "b_partitions_explicit": b_partitions(1), "b_partitions_implicit": b_partitions(2),
    "b_spatial_direct": b_spatial_direct(1), "b_spatial_direct_no_inference": b_spatial_direct(0),
    "b_temporal_direct": b_temporal_direct(1), "b_temporal_direct_no_inference": b_temporal_direct(0),
    "window_borders": window_borders, "reach_chain": reach_chain}


def case_sizes(name):
    return SIZES + [(32, 32)] if name == "window_borders" else SIZES


@functools.lru_cache(maxsize=None)
def scripted(name, size=SIZES[0]):
    """(seq, pics, stream, expected planes per picture in decode order, branch counts of the restatement, what the writer recorded): computed once,
    never modified"""
    seq, pics = CASES[name](*size)
    cov, seen = {}, set()
    data = sw.write(seq, pics, seen)
    planes = ae.expect_h264(seq, pics, mcov=cov)
    return seq, pics, data, planes, cov, frozenset(seen)


@functools.lru_cache(maxsize=None)
def scripted_deblocked(name, size=SIZES[0]):
    """(seq, pics, stream, expected planes) of the case with the deblocking filter on in every picture"""
    seq, pics = CASES[name](*size)
    pics = hr.with_deblocking(pics)
    return seq, pics, sw.write(seq, pics), ae.expect_h264(seq, pics)
