"""Scripted H.264 cases for field pictures (PAFF): name -> builder(width, height) -> (seq, pics), for tests/scripted_h264.py with frame_mbs_only=0.

The expected pictures come from tests/analytic_expect.py with tests/h264_field_ref.py.  Content is seeded noise unless a closed form is the point, so
that a wrong line or a wrong parity always shows.  A field is a picture of its own in ``pics`` (mbw x mbh / 2 macroblocks); a frame is two consecutive
fields of opposite parity; order counts: a field's own.  ``scripted(name, size)`` also returns what the case exercised (the restatement's, the
writer's and the deblocking restatement's counters); tests/test_h264_field_host.py asserts each case's coverage from them and from the script.
"""
import functools

import numpy as np

import analytic_cases as ac
import analytic_expect as ae
import analytic_h264_recon as hr
import h264_field_ref as fr
import scripted_h264 as sw
from spec_tables_h264 import FIELD_SCAN_4x4, FIELD_SCAN_8x8, ZIGZAG_4x4, ZIGZAG_8x8

SIZE = (96, 160)                                                    # 6 x 5 field macroblocks: wider than the ring of four macroblock bottoms
SIZES_EDGE = [(96, 160), (16, 96), (48, 544)]                       # one macroblock wide; 17 field rows: two bands of kIBandRows / kBandRows = 16
OTHER = fr.OTHER


def fdims(w, h):
    mbw, mbh = ac.dims(w, h)
    assert mbh % 2 == 0
    return mbw, mbh // 2


def noise_field(rng, mbw, rows, field, poc, kind="I", **kw):
    return dict(ac.noise_pic(rng, mbw, rows, kind, poc, **kw), field=field)


def base_seq(w, h, **kw):
    return dict(width=w, height=h, frame_mbs_only=0, **kw)


# ---- field_pcm_weave ----------------------------------------------------------------------------------------------------------------------------
def field_pcm_weave(w, h):
    """I_PCM fields: a frame top field first, a frame bottom field first (the bottom field has the smaller count), a frame coded as fields followed by
    a frame coded as a frame"""
    rng = np.random.default_rng(0xF100)
    mbw, rows = fdims(w, h)
    pics = [noise_field(rng, mbw, rows, "top", 0), noise_field(rng, mbw, rows, "bottom", 1),
            noise_field(rng, mbw, rows, "bottom", 2), noise_field(rng, mbw, rows, "top", 3, kind="P"),
            noise_field(rng, mbw, rows, "top", 4), noise_field(rng, mbw, rows, "bottom", 5),
            ac.noise_pic(rng, mbw, 2 * rows, "I", 6), ac.noise_pic(rng, mbw, 2 * rows, "P", 8)]
    return base_seq(w, h), pics


# ---- field_intra --------------------------------------------------------------------------------------------------------------------------------
def field_intra(w, h):
    """I fields of Intra16x16, Intra4x4, Intra8x8 and I_PCM macroblocks, levels in every block, the modes in rotation among those the FIELD's
    neighbours allow; one slice per picture, per row and per macroblock"""
    rng, rota = np.random.default_rng(0xF200), hr.Rota()
    seq = base_seq(w, h, profile=100, transform8x8=1)
    pics = []
    for f, layout in enumerate(("pic", "row", "mb", "pic")):
        for i, par in enumerate(("top", "bottom") if f != 3 else ("bottom", "top")):
            p = hr.picture(rng, rota, sw.pic_seq(seq, dict(field=par)), lambda a, x, y: ("i4", "pcm", "i8", "i16", "i4", "i8", "i16")[(a + 2 * y + f + i) % 7],
                           (30, 24, 36, 27)[f], 2 * f + i, kind="I", layout=layout)
            pics.append(dict(p, field=par))
    return seq, pics


# ---- field_scan_levels --------------------------------------------------------------------------------------------------------------------------
def single(n, pos, v):
    out = [0] * n
    out[pos] = v
    return out


def field_scan_levels(w, h):
    """An I field and a P field whose blocks carry ONE level each, at every raster position of a 4x4 block (Intra4x4, and the AC of Intra16x16), of the
    Intra16x16 DC matrix, of a chroma AC block and of an 8x8 block (Intra8x8; inter with transform_size_8x8_flag), then dense blocks.  The field scan
    differs from the zig-zag scan at most positions: tests/test_h264_field_host.py asserts that from the tables."""
    rng = np.random.default_rng(0xF300)
    mbw, rows = fdims(w, h)
    seq = base_seq(w, h, profile=100, transform8x8=1)
    n = mbw * rows
    assert n >= 30
    sign = lambda k: 1 if k % 2 == 0 else -1
    want = [dict(t="i4", modes=[2] * 16, cmode=0, coef=dict(y={k: single(16, k, 9 * sign(k)) for k in range(16)}))]
    want += [dict(t="i8", modes=[2] * 4, cmode=0, coef=dict(y8={b: single(64, 4 * j + b, 11 * sign(j + b)) for b in range(4)})) for j in range(16)]
    want += [dict(t="i16", mode=2, cmode=0, coef=dict(ydc=single(16, k, 7 * sign(k)), y={k: single(16, max(k, 1), 6)},
                                                      cac={(k & 1, k % 4): single(15, (k * 7) % 15, 5 * sign(k))})) for k in range(16)]
    i16 = want[17:]
    want = want[:17]
    for lst in (want, i16):
        while len(lst) < n - 4:
            lst.append(dict(t="i4", modes=[2] * 16, cmode=0, coef=dict(y={k: hr.sparse(rng, 16, 12, 12) for k in range(16)})))
        while len(lst) < n:
            lst.append(dict(t="i8", modes=[2] * 4, cmode=0, coef=dict(y8={k: hr.sparse(rng, 64, 10, 40) for k in range(4)})))
    top = dict(kind="I", poc=0, field="top", layout="mb", qp=28, mbs=[hr.fit(seq, m, 28) for m in want[:n]])
    top2 = dict(kind="I", poc=2, field="top", layout="mb", qp=24, mbs=[hr.fit(seq, m, 24) for m in i16[:n]])
    mbs = []
    for a in range(n):
        m = dict(t="16x16", l0=(0, (int(rng.integers(-20, 21)), int(rng.integers(-12, 13)))))
        if a < 16:
            m.update(t8=1, coef=dict(y8={b: single(64, 4 * a + b, 10 * sign(a)) for b in range(4)}))
        elif a < 20:
            m.update(coef=dict(y={k: single(16, k, 8 * sign(k + a)) for k in range(16)}, cac={(a & 1, k): single(15, (4 * (a - 16) + k) % 15, 6) for k in range(4)}))
        else:
            m.update(t8=a & 1, coef=({"y8": {k: hr.sparse(rng, 64, 9, 30) for k in range(4)}} if a & 1 else {"y": {k: hr.sparse(rng, 16, 9, 10) for k in range(16)}}))
        mbs.append(hr.fit(seq, m, 30))
    bottom = dict(kind="P", poc=1, field="bottom", layout="mb", qp=30, mbs=mbs)
    return seq, [top, bottom, top2, noise_field(rng, mbw, rows, "bottom", 3, kind="P")]


# ---- inter: parities, borders, lists ------------------------------------------------------------------------------------------------------------
def names_for(seq, pics, p):
    """(RefPicList0, RefPicList1) of the picture p that is about to join pics, cut to its active length, in the script's names (the writer's plan)"""
    pl = sw.plan(seq, pics + [dict(p, mbs=[])])[-1]
    return pl["l0"], pl["l1"]


def field_p_parities(w, h):
    """P fields for the four (current parity, reference parity) pairs, the second field predicting from the first field of its own frame; in every
    pair the 64 fractional chroma positions (the 16 luma positions among them) and integer vectors; 8x16 / 16x8 macroblocks carry two vectors"""
    rng, rota = np.random.default_rng(0xF400), hr.Rota()
    mbw, rows = fdims(w, h)
    seq = base_seq(w, h, num_ref_frames=2)
    pics = [noise_field(rng, mbw, rows, "top", 0)]
    order = ["top", "bottom", "top", "bottom", "bottom", "top", "top", "bottom", "bottom", "top"]       # frames 2 and 4 have their bottom field first
    for k in range(1, 10):
        par = order[k]
        head = dict(kind="P", poc=k, field=par, is_ref=k < 8)
        l0, _ = names_for(seq, pics, head)
        mbs = []
        for a in range(mbw * rows):
            parts = []
            for i in range(2):
                ref = l0[(2 * a + i) % len(l0)]
                key = (par, fr.field_of(pics, ref)[1])
                frac = rota.pick(key, range(65))                    # 64: an integer vector once more
                mv = (4 * int(rng.integers(-6, 7)), 4 * int(rng.integers(-6, 7))) if frac == 64 else \
                     (8 * int(rng.integers(-3, 4)) + frac % 8, 8 * int(rng.integers(-3, 4)) + frac // 8)
                parts.append((ref, mv))
            mbs.append(dict(t=("16x8", "8x16")[a % 2], parts=parts))
        pics.append(dict(head, mbs=mbs, num_ref=(len(l0), 1)))
    return seq, pics


# quarter samples beyond the border: one line, the three lines below an integer position, a fraction (the filter's reach: 2 above, 3 below), two lines,
# more than a macroblock, and -- ("c", v) -- a cross-parity reference whose chroma vector v - 2 (top) / 2 - v (bottom) lands on the border and past it
BORDER_STEPS = [-4, ("c", 2), -12, -2, ("c", 0), -8, -80, -1, -9, -72, -5, 3]


def field_p_borders(w, h):
    """P fields, both parities, same-parity and cross-parity references, whose reference windows leave the FIELD at the top, the bottom, the left and
    the right: by one line, by the reach of the filter (2 above, 3 below), by fractions, by more than a macroblock.  With the Table 8-9 offset the
    cross-parity chroma window lands exactly on the border (a vector of +-2 against the offset) and one step past it (a vector of 0).  Every (parity,
    side) walks through BORDER_STEPS with a counter of its own; a picture of few macroblocks gets more pictures."""
    rng = np.random.default_rng(0xF500)
    mbw, rows = fdims(w, h)
    seq = base_seq(w, h, num_ref_frames=1)
    pics = [noise_field(rng, mbw, rows, "top", 0)]
    count = {}

    def step(par, side):
        count[(par, side)] = count.get((par, side), 0) + 1
        return BORDER_STEPS[(count[(par, side)] - 1) % len(BORDER_STEPS)]
    for k in range(1, 2 * -(-len(BORDER_STEPS) // mbw) + 2):       # each parity meets every step on every side
        par = ("top", "bottom")[k % 2]
        head = dict(kind="P", poc=k, field=par)
        l0, _ = names_for(seq, pics, head)
        cross = [q for q in l0 if fr.field_of(pics, q)[1] != par]
        mbs = []
        for a in range(mbw * rows):
            x, y = a % mbw, a // mbw
            tall = y in (0, rows - 1)                               # 8x16: both halves touch the top and the bottom of the macroblock; 16x8: both sides
            parts = []
            for i in range(2):
                mv = [int(rng.integers(-9, 10)), int(rng.integers(-9, 10))]
                ref = l0[(k + i + a) % len(l0)]
                side = "top" if y == 0 and (i == 0 or not tall or rows == 1) else ("bottom" if y == rows - 1 and (i == 1 or not tall) else None)
                if side:
                    v = step(par, side)
                    if isinstance(v, tuple):
                        ref, v = cross[0], v[1]
                    mv[1] = v if side == "top" else -v
                if x == 0 and i == 0:
                    v = step(par, "left")
                    mv[0] = -3 if isinstance(v, tuple) else v
                elif x == mbw - 1 and i == 1:
                    v = step(par, "right")
                    mv[0] = 3 if isinstance(v, tuple) else -v
                parts.append((ref, tuple(mv)))
            mbs.append(dict(t="8x16" if tall else "16x8", parts=parts))
        pics.append(dict(head, mbs=mbs, num_ref=(len(l0), 1)))
    return seq, pics


def field_p_lists(w, h):
    """num_ref_frames 4: P fields that use every index of a list of up to 8 fields, one macroblock per index in turn, each store with noise of its
    own; first and second fields of both parities; the second field's list begins with the first field of its own frame, a store that holds one field"""
    rng = np.random.default_rng(0xF600)
    mbw, rows = fdims(w, h)
    seq = base_seq(w, h, num_ref_frames=4)
    pics = [noise_field(rng, mbw, rows, "top", 0)]
    order = ["bottom", "top", "bottom", "bottom", "top", "top", "bottom"]          # frames 0, 1: top first; frame 2: bottom first; frame 3: top first
    for k, par in enumerate(order, 1):
        pics.append(noise_field(rng, mbw, rows, par, k, kind="P"))
    for k, par in enumerate(("top", "bottom", "bottom", "top"), 8):
        l0, _ = names_for(seq, pics, dict(kind="P", poc=k, field=par))          # every field held: 8, or 7 behind a sliding window and a first field
        n = len(l0)
        mbs = [dict(t="16x16", l0=(l0[a % n], (int(rng.integers(-30, 31)), int(rng.integers(-30, 31))))) for a in range(mbw * rows)]
        pics.append(dict(kind="P", poc=k, field=par, num_ref=(n, 1), mbs=mbs))
    return seq, pics


# ---- B fields -----------------------------------------------------------------------------------------------------------------------------------
def field_b(mode):
    """B fields between and behind two reference frames: list 0 only, list 1 only, both; weighted_bipred_idc = mode.  Implicit weights (2): the
    counts 2 / 3 of the two B fields between reference fields of 0 / 1 and 8 / 9 give (48, 16) for the top field and other weights for the bottom
    field from the same two references; a macroblock whose two references are ONE field falls back to (32, 32) (DiffPicOrderCnt(pic1, pic0) = 0).
    The B fields behind both frames (10, 11) have equal lists longer than one entry: list 1 is swapped."""
    def build(w, h):
        rng = np.random.default_rng(0xF700 + mode)
        mbw, rows = fdims(w, h)
        seq = base_seq(w, h, num_ref_frames=2, profile=77, weighted_bipred=mode)
        pics = [noise_field(rng, mbw, rows, "top", 0), noise_field(rng, mbw, rows, "bottom", 1, kind="P"),
                noise_field(rng, mbw, rows, "top", 8, kind="P"), noise_field(rng, mbw, rows, "bottom", 9, kind="P")]
        for poc, par in ((2, "top"), (3, "bottom"), (11, "bottom"), (10, "top")):
            head = dict(kind="B", poc=poc, field=par, is_ref=False, num_ref=(4, 4))
            l0, l1 = names_for(seq, pics, head)
            if mode == 1:
                ent = lambda: dict(y=(int(rng.integers(-20, 60)), int(rng.integers(-20, 21))) if rng.integers(4) else None,
                                   c=tuple((int(rng.integers(-10, 50)), int(rng.integers(-15, 16))) for _ in range(2)) if rng.integers(4) else None)
                head["wp"] = dict(ld_y=5, ld_c=4, l0=[ent() for _ in range(4)], l1=[ent() for _ in range(4)])
            mbs, both = [], 0
            for a in range(mbw * rows):
                mv = lambda: (int(rng.integers(-24, 25)), int(rng.integers(-24, 25)))
                i, j, use = a % 4, (a // 4) % 4, a % 5
                if use == 0:
                    m = dict(t="16x16", l0=(l0[i], mv()))
                elif use == 1:
                    m = dict(t="16x16", l1=(l1[i], mv()))
                elif use == 2 and a % 2 == 0:
                    m = dict(t="16x16", l0=(l0[i], mv()), l1=(l0[i], mv()))        # one field through both lists
                else:
                    i, j = both % 4, (both // 4) % 4                # every pair of entries in turn, (0, 0) first
                    both += 1
                    m = dict(t="16x16", l0=(l0[i], mv()), l1=(l1[j], mv()))
                mbs.append(m)
            pics.append(dict(head, mbs=mbs))
        return seq, pics
    return build


# ---- frames and fields in one stream ------------------------------------------------------------------------------------------------------------
def paff_mixed(dense):
    """A frame picture; a field pair whose fields predict from the two fields of that frame (and the second from the first); a B frame between them
    that predicts from the frame and from the woven pair; a P frame that predicts from the woven pair and from the frame; a last field pair that
    predicts from fields of the P frame.  Intra macroblocks with levels among the inter ones: one per picture (below 1 / 16 of them: k_recon_intra), or
    every third (dense: k_intra_band)."""
    def build(w, h):
        rng, rota = np.random.default_rng(0xF800 + dense), hr.Rota()
        mbw, rows = fdims(w, h)
        seq = base_seq(w, h, num_ref_frames=2, profile=77)
        pics = [ac.noise_pic(rng, mbw, 2 * rows, "I", 0)]

        def p_picture(head, refs_of):
            fseq = sw.pic_seq(seq, head)
            n = mbw * (rows if head.get("field") else 2 * rows)
            p = dict(head, layout="pic", qp=30, mbs=[])
            for a in range(n):
                if (a % 3 == 1) if dense else (a == n // 2 + 1):
                    p["mbs"].append(hr.make_nxn(rng, rota, fseq, p, a, 30, "i4") if a % 2 else hr.make_i16(rng, rota, fseq, p, a, 30, "rota"))
                else:
                    p["mbs"].append(dict(t="16x16", l0=(refs_of[a % len(refs_of)], (int(rng.integers(-20, 21)), int(rng.integers(-20, 21))))))
            return p
        for poc, par in ((8, "top"), (9, "bottom")):
            head = dict(kind="P", poc=poc, field=par)
            l0, _ = names_for(seq, pics, head)
            pics.append(dict(p_picture(head, l0), num_ref=(len(l0), 1)))
        l0, l1 = names_for(seq, pics, dict(kind="B", poc=4, is_ref=False))
        assert l0 == [0, 1] and l1 == [1, 0]
        mv = lambda: (int(rng.integers(-24, 25)), int(rng.integers(-24, 25)))
        pics.append(dict(kind="B", poc=4, is_ref=False, num_ref=(2, 2),
                         mbs=[[dict(t="16x16", l0=(0, mv())), dict(t="16x16", l1=(1, mv())), dict(t="16x16", l0=(1, mv()), l1=(0, mv())),
                               dict(t="16x16", l0=(0, mv()), l1=(1, mv()))][a % 4] for a in range(2 * mbw * rows)]))
        head = dict(kind="P", poc=12)
        l0, _ = names_for(seq, pics, head)
        assert l0 == [1, 0]
        pics.append(dict(p_picture(head, l0), num_ref=(2, 1)))
        for poc, par in ((17, "bottom"), (16, "top")):
            head = dict(kind="P", poc=poc, field=par)
            l0, _ = names_for(seq, pics, head)
            pics.append(dict(p_picture(head, l0), num_ref=(len(l0), 1)))
        return seq, pics
    return build


# ---- deblocking ---------------------------------------------------------------------------------------------------------------------------------
def field_deblock_intra(w, h):
    """I and P fields of Intra16x16 macroblocks beside I_PCM ones with the filter on: bS 4 on vertical and bS 3 on HORIZONTAL macroblock edges (the
    field rule), 3 inside; one slice per picture and per row; idc 0 and 2 (a slice per row: no horizontal macroblock edge is filtered)"""
    rng = np.random.default_rng(0xF900)
    mbw, rows = fdims(w, h)
    spec = [("I", "pic", (0, 0, 0), 26, 4), ("P", "pic", (0, 6, 6), 40, 40), ("P", "row", (0, -3, 3), 30, 1), ("P", "row", (2, 3, -2), 51, 4),
            ("P", "pic", (2, 1, 2), 20, 12), ("P", "pic", (0, 2, 2), 36, 12)]
    pics = [dict(ac.intra_filter_pic(rng, mbw, rows, kind, k, layout, db, amp, qp, k, (40, 12) if layout == "row" else (16, 36)), field=("top", "bottom")[k % 2])
            for k, (kind, layout, db, qp, amp) in enumerate(spec)]
    return base_seq(w, h, chroma_qp_off=-3), pics


def field_deblock_inter(w, h):
    """P fields, one slice per macroblock, filter on: 16x16 macroblocks whose vectors differ from their neighbours' vertically by exactly 1 (bS 0) and
    exactly 2 (bS 1: the field limit) and horizontally by 3 and 4; references that are the two fields of ONE frame (bS 1); I_PCM and Intra16x16
    macroblocks beside inter ones on vertical (bS 4) and horizontal (bS 3) macroblock edges; coded blocks (bS 2); 16x8 / 8x16 inner edges"""
    rng = np.random.default_rng(0xFA00)
    mbw, rows = fdims(w, h)
    seq = base_seq(w, h, num_ref_frames=2, chroma_qp_off=4)
    pics = [dict(ac.intra_filter_pic(rng, mbw, rows, "I", 0, "pic", (0, 6, 6), 4, 44, 0), field="top"),
            dict(ac.intra_filter_pic(rng, mbw, rows, "P", 1, "pic", (0, 3, 3), 12, 40, 1), field="bottom")]
    incx, incy = [3, 4, 0, 4, 3, 12], [1, 2, 0, 2, 1, 8]
    for k in range(2, 6):
        par = ("top", "bottom")[k % 2]
        head = dict(kind="P", poc=k, field=par, is_ref=k < 4)
        l0, _ = names_for(seq, pics, head)
        pcm = ac.stepped_pcm(rng, mbw, rows, ac.AMPS[k % 4])
        mbs = []
        for a in range(mbw * rows):
            x, y = a % mbw, a // mbw
            mv = (-20 + 8 * k + sum(incx[i % 6] for i in range(x)), 6 - 4 * (k % 3) + sum(incy[(i + k) % 6] for i in range(y)))
            t = (x + 3 * y + k) % 8
            ref = l0[int((x // 2 + y + k) % 3 == 0)]                # the two fields of the newest frame (or of the current frame and the one before)
            alt = l0[1 - int((x // 2 + y + k) % 3 == 0)]
            if t == 0:
                m = dict(pcm[a])
            elif t == 1:
                m = dict(t="i16", mode=2, cmode=0)
            elif t in (2, 3):
                second = [(ref, (mv[0] + 4, mv[1])), (alt, mv), (ref, (mv[0], mv[1] - 1)), (ref, (mv[0] - 3, mv[1] + 2))][(a + k) % 4]
                m = dict(t=("16x8", "8x16")[t - 2], parts=[(ref, mv), second])
            else:
                m = dict(t="16x16", l0=(ref, mv))
                if t == 4:
                    m["resid"] = (int(rng.integers(16)), (1, -1)[a & 1])
            m.update(ac.mb_slice_fields(x, y, k))
            if (x > 0 and (x - 1 + 3 * y + k) % 8 == 0) or (y > 0 and (x + 3 * (y - 1) + k) % 8 == 0):
                m["qp"] = 51
            mbs.append(m)
        pics.append(dict(head, mbs=mbs, num_ref=(2, 1)))
    return seq, pics


def field_deblock_b(w, h):
    """B fields with the filter on: list 0 only, list 1 only and bi-predicted neighbours over the four reference fields of two frames; pairs equal
    crosswise (bS 0), equal in fields but not in vectors, both vectors on one field, and pairs on the two fields of one frame (different pictures)"""
    rng = np.random.default_rng(0xFB00)
    mbw, rows = fdims(w, h)
    seq = base_seq(w, h, num_ref_frames=2, profile=77, chroma_qp_off=-2)
    pics = [dict(ac.intra_filter_pic(rng, mbw, rows, ("I", "P")[k > 0], poc, "pic", (0, 4, 2), 12, 40, k), field=("top", "bottom")[k % 2])
            for k, poc in enumerate((0, 1, 8, 9))]
    A, B = (12, -6), (-16, 10)
    for k, (poc, par) in enumerate(((4, "top"), (5, "bottom"))):
        head = dict(kind="B", poc=poc, field=par, is_ref=False, num_ref=(4, 4))
        l0, l1 = names_for(seq, pics, head)
        f0, f0o, f1, f1o = l0[0], l0[1], l1[0], l1[1]
        mbs = []
        for a in range(mbw * rows):
            x, y = a % mbw, a // mbw
            A2, B2 = (A[0] + 3 + (y & 1), A[1]), (B[0], B[1] - 2 + (x & 1))
            m = [dict(t="16x16", l0=(f0, A)), dict(t="16x16", l1=(f1, B)), dict(t="16x16", l0=(f0, A), l1=(f1, B)), dict(t="16x16", l0=(f1, B), l1=(f0, A)),
                 dict(t="16x16", l0=(f0, A2), l1=(f1, B)), dict(t="16x16", l0=(f0, A), l1=(f0, B)), dict(t="16x16", l0=(f0, B2), l1=(f0, A)),
                 dict(t="16x16", l0=(f0o, A)), dict(t="16x16", l0=(f0o, A), l1=(f1o, B)), dict(t="16x16", l0=(f0, A), l1=(f1, B))][(x + 4 * y + k) % 10]
            m.update(ac.mb_slice_fields(x, y, k))
            mbs.append(m)
        pics.append(dict(head, mbs=mbs))
    return seq, pics


# ---- the end of a stream, cropping --------------------------------------------------------------------------------------------------------------
def field_lone(first):
    """A frame, then ONE more field (a first field) and the end of the stream"""
    def build(w, h):
        rng = np.random.default_rng(0xFC00 + (first == "top"))
        mbw, rows = fdims(w, h)
        seq = base_seq(w, h)
        pics = [noise_field(rng, mbw, rows, first, 0)]
        for k, par in ((1, OTHER[first]), (2, first)):
            head = dict(kind="P", poc=k, field=par)
            l0, _ = names_for(seq, pics, head)
            pics.append(dict(head, num_ref=(len(l0), 1), mbs=[dict(t="16x16", l0=(l0[a % len(l0)], (int(rng.integers(-30, 31)), int(rng.integers(-30, 31)))))
                                                             for a in range(mbw * rows)]))
        return seq, pics
    return build


def field_cropped(w, h):
    """96x88 in a coded frame of 96x96: with frame_mbs_only_flag 0 the vertical crop unit is 4 luma rows (frame_crop_bottom_offset 2)"""
    assert (w, h) == (96, 88)
    rng = np.random.default_rng(0xFD00)
    mbw, rows = fdims(w, h)
    seq = base_seq(w, h)
    pics = [noise_field(rng, mbw, rows, "top", 0)]
    for k in range(1, 4):
        head = dict(kind="P", poc=k, field=("top", "bottom")[k % 2])
        l0, _ = names_for(seq, pics, head)
        pics.append(dict(head, num_ref=(len(l0), 1), mbs=[dict(t="16x16", l0=(l0[a % len(l0)], (int(rng.integers(-40, 41)), int(rng.integers(-40, 41)))))
                                                         for a in range(mbw * rows)]))
    return seq, pics


CASES = {
    "field_pcm_weave": field_pcm_weave, "field_intra": field_intra, "field_scan_levels": field_scan_levels, "field_p_parities": field_p_parities,
    "field_p_borders": field_p_borders, "field_p_lists": field_p_lists, "field_b": field_b(0), "field_b_explicit": field_b(1),
    "field_b_implicit": field_b(2), "paff_mixed": paff_mixed(1), "paff_mixed_sparse": paff_mixed(0), "field_deblock_intra": field_deblock_intra,
    "field_deblock_inter": field_deblock_inter, "field_deblock_b": field_deblock_b, "field_lone_top": field_lone("top"),
    "field_lone_bottom": field_lone("bottom"), "field_cropped": field_cropped}
EDGE_CASES = ["field_intra", "field_p_borders", "field_deblock_intra", "field_deblock_inter", "field_deblock_b"]


def case_sizes(name):
    return [(96, 88)] if name == "field_cropped" else (SIZES_EDGE if name in EDGE_CASES else [SIZE])


@functools.lru_cache(maxsize=None)
def scripted(name, size=None):
    """(seq, pics, stream, expected planes per picture in decode order, coverage set, deblock_ref counters): computed once, never modified"""
    seq, pics = CASES[name](*(size or case_sizes(name)[0]))
    cov, stats = set(), {}
    data = sw.write(seq, pics, cov)
    planes = ae.expect_h264(seq, pics, stats=stats, rstats=cov)
    return seq, pics, data, planes, frozenset(cov), stats


@functools.lru_cache(maxsize=None)
def scripted_deblocked(name, size=None):
    """(seq, pics, stream, expected planes, counters of deblock_ref) of the case with the deblocking filter on in every picture"""
    seq, pics = CASES[name](*(size or case_sizes(name)[0]))
    pics = hr.with_deblocking(pics)
    stats = {}
    return seq, pics, sw.write(seq, pics), ae.expect_h264(seq, pics, stats), stats


def scan_positions_that_differ():
    return ([k for k in range(16) if FIELD_SCAN_4x4[k] != ZIGZAG_4x4[k]], [k for k in range(64) if FIELD_SCAN_8x8[k] != ZIGZAG_8x8[k]])
