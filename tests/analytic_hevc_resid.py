"""The known-answer cases of the H.265 residual path: scripts for tests/scripted_hevc.py whose expected pictures tests/hevc_resid_ref.py computes from
clauses 8.6.1 - 8.6.4.2.  name -> builder() -> (seq, pics); every stream has the deblocking filter and SAO off; inter units predict from PCM noise
pictures, so the prediction is itself known.  The groups are chosen for where the code can go wrong, not for realism; what each owes is asserted in
tests/test_hevc_resid_host.py from the expectation's records and the writer's counters, not here."""
import numpy as np

import scripted_hevc as hw
from analytic_hevc_intra import pcm_picture

STEP_COLS = (3, 4, 7, 8, 15, 16, 31)                                # largest coefficient column at the steps of the kernel's column padding
MODES = (5, 6, 14, 15, 21, 22, 30, 31)                              # both sides of the mode ranges that choose the vertical / horizontal scan


def base_seq(width, height, ctb_log2=5, **kw):
    return dict(width=width, height=height, ctb_log2=ctb_log2, min_cb_log2=3, max_tb_log2=min(ctb_log2, 5), tu_depth_intra=2, tu_depth_inter=ctb_log2 - 2,
                pcm_log2=(3, min(ctb_log2, 5)), **kw)


def inter(ref, mv, tu, coef, **kw):
    return dict(t="inter", l0=(ref, mv), tu=tu, coef=coef, **kw)


def intra(modes, chroma, tu, coef, **kw):
    return dict(t="intra", modes=list(modes), chroma=chroma, tu=tu, coef=coef, **kw)


def patterns(n, rng):
    """Coefficient sets of an n x n block: one coefficient at each corner, in the last row and in the last column; a dense block; the largest column at
    each step with the largest row at 0, 1 and n - 1"""
    lv = lambda: int(rng.integers(1, 4)) * (1 if rng.random() < 0.5 else -1)
    out = [{(0, 0): 3}, {(n - 1, 0): -2}, {(0, n - 1): 2}, {(n - 1, n - 1): -3}, {(n // 2 - 1, n - 1): 2}, {(n - 1, n // 2): -2}]
    if n == 4:
        out.append({(x, y): lv() for x in range(4) for y in range(4)})
    elif n == 8:
        out.append({(x, y): lv() for x in range(8) for y in range(8)})                             # exactly 64: the last count served by one load
    else:
        cells = rng.permutation(n * n)[:200 if n == 16 else 420]
        out.append({(int(c) % n, int(c) // n): (1 if rng.random() < 0.5 else -1) for c in cells})
    for col in STEP_COLS:
        if col < n:
            for row in (0, 1, n - 1):
                out.append({(col, row): lv(), (0, row): lv(), (col, 0): lv(), (col // 2, row // 2): lv()})
    return out


def chunk_pictures(seq, units, kind, first_poc, **kw):
    """units (one per CTB) -> pictures; CTBs left over at the end repeat the first units"""
    cw, ch = hw.ctb_dims(seq)
    per = cw * ch
    pics = []
    for k in range(0, len(units), per):
        cus = units[k:k + per]
        cus += [dict(u) for u in units[:per - len(cus)]]
        assert len(cus) == per
        pics.append(dict(kind=kind, poc=first_poc + 2 * len(pics), is_ref=False, cus=cus, **kw))
    return pics


def size_units(rng, make, depths, ctb_log2=5):
    """CTB-sized units whose transform blocks run through patterns() at every depth of ``depths``: make(depth, coef, index) -> unit"""
    units = []
    for d in depths:
        lg = ctb_log2 - d
        luma, chroma = patterns(1 << lg, rng), patterns(1 << max(lg - 1, 2), rng)
        per = 4 ** d
        n_tus = max(len(luma), len(chroma) * (4 if lg == 2 else 1))
        n_tus = (n_tus + per - 1) // per * per
        coef, j = [], 0
        for i in range(n_tus):
            e = {0: luma[i % len(luma)]}
            if lg > 2 or i % 4 == 3:
                e[1], e[2] = chroma[j % len(chroma)], chroma[(j + 3) % len(chroma)]
                j += 1
            coef.append(e)
        for k in range(0, n_tus, per):
            units.append(make(d, coef[k:k + per], len(units)))
    return units


def sizes_intra():
    """Intra units of 32x32 with transform depth 0 .. 2 (luma 32, 16, 8 with chroma 16, 8, 4) and of 16x16 with depth 2 (luma 4, chroma 4 with the fourth)"""
    rng = np.random.default_rng(0xD101)
    seq = base_seq(128, 64)
    units = size_units(rng, lambda d, coef, i: intra([(1, 0, 26, 10, 18, 2, 34)[i % 7]], i % 5, d, coef), (0, 1, 2))
    small = size_units(rng, lambda d, coef, i: coef, (3,))
    for coef in small:                                              # 64 transform units of 4x4: four 16x16 units of depth 2
        units.append(dict(t="split", sub=[intra([(1, 0, 26, 10)[q]], q, 2, coef[16 * q:16 * q + 16]) for q in range(4)]))
    return seq, chunk_pictures(seq, units, "I", 0, qp=28)


def sizes_inter():
    """Inter units of 32x32 with transform depth 0 .. 3 (luma 32, 16, 8, 4 with chroma 16, 8, 4 and 4 with the fourth) over a PCM noise picture"""
    rng = np.random.default_rng(0xD102)
    seq = base_seq(128, 64)
    units = size_units(rng, lambda d, coef, i: inter(0, (int(rng.integers(-30, 30)), int(rng.integers(-30, 30))), d, coef), (0, 1, 2, 3))
    return seq, [pcm_picture(rng, seq)] + chunk_pictures(seq, units, "P", 2, qp=30)


# ---- scans ----------------------------------------------------------------------------------------------------------------------------------------
def scans():
    """8x8 intra units: one 8x8 luma block (and 4x4 chroma), or four 4x4 luma blocks of modes of their own, with coefficient sets that are not symmetric.
    intra_chroma_pred_mode 4 hands the luma mode to the chroma blocks; 1 beside luma mode 26 turns the chroma mode into 34 (diagonal scan) while the luma
    block scans horizontally"""
    rng = np.random.default_rng(0xD201)
    seq = base_seq(64, 48, ctb_log2=4)
    c4 = [{(3, 0): 2, (1, 2): -1, (0, 1): 1}, {(0, 3): -2, (2, 1): 1, (3, 3): 1}, {(2, 0): 1, (0, 1): -3}, {(1, 3): 2, (3, 0): -1, (2, 2): 1}]
    c8 = [{(6, 1): 1, (2, 5): -2, (0, 3): 1, (7, 0): 1}, {(1, 6): -1, (5, 2): 2, (3, 0): 1, (0, 7): -1}, {(7, 3): 1, (4, 4): -1, (0, 5): 2}]
    units = []
    for i, m in enumerate(MODES + (26, 10, 2, 18, 34)):
        chroma = 4 if m in MODES else (1 if m == 26 else (2 if m == 10 else i % 5))
        units.append(intra([m], chroma, 0, [{0: c8[i % 3], 1: c4[i % 4], 2: c4[(i + 1) % 4]}]))
        ms = [m, MODES[(i + 3) % 8], MODES[(i + 5) % 8], 1]
        units.append(intra(ms, chroma, 1, [{0: c4[(i + q) % 4], **({1: c4[(i + 2) % 4], 2: c4[(i + 3) % 4]} if q == 3 else {})} for q in range(4)]))
    cus = [dict(t="split", sub=[units[(4 * a + q) % len(units)] for q in range(4)]) for a in range(12)]
    cus2 = [dict(t="split", sub=[units[(4 * a + q + 2) % len(units)] for q in range(4)]) for a in range(12)]
    return seq, [dict(kind="I", poc=0, is_ref=False, qp=27, cus=cus), dict(kind="I", poc=2, is_ref=False, qp=33, cus=cus2)]


# ---- levels ---------------------------------------------------------------------------------------------------------------------------------------
def sub_block(xs, ys, levels_by_scan_pos):
    """coefficients of the 4x4 sub-block (xs, ys) given by diagonal scan position"""
    return {(4 * xs + hw.SCAN[0][2][k][0], 4 * ys + hw.SCAN[0][2][k][1]): v for k, v in levels_by_scan_pos.items()}


def level_blocks():
    """16x16 coefficient sets (diagonal scan; sub-blocks are decoded from the last one down):
    0: a sub-block with 12 levels above 1; one that ends with greater1Ctx 3 (ones only); one after it (ctxSet not raised); an empty one; one with
       only position 0 (sig_coeff_flag inferred); one ending with greater1Ctx 0 and its successor (ctxSet raised)
    1: levels 4, 8, 14, 26, 50, 200, 3000, 32767 in one sub-block: cRiceParam climbs to 4, the escape code follows
    2: more than 8 coefficients of level 1 and 2 mixed, then large ones coded with base level 1"""
    a = {}
    a.update(sub_block(3, 3, {k: (2 + k % 3) * (1 if k % 2 else -1) for k in range(2, 14)}))
    a.update(sub_block(2, 3, {0: 1, 3: -1, 5: 1, 9: 1}))
    a.update(sub_block(3, 2, {1: 1, 2: 2, 7: -1}))
    a.update(sub_block(2, 2, {0: -2}))
    a.update(sub_block(3, 0, {4: 3, 5: 1}))
    a.update(sub_block(0, 3, {6: 1, 2: -1}))
    a.update(sub_block(1, 1, {0: 1}))
    a.update(sub_block(0, 0, {0: 2, 1: 1, 15: -1}))
    b = sub_block(1, 0, {15: 4, 13: -8, 12: 14, 9: -26, 8: 50, 5: -200, 3: 3000, 1: -32768, 0: 32767})
    b.update(sub_block(0, 0, {0: 1}))
    c = sub_block(2, 1, {k: (1, -2, 1, 1, 2, -1, 1, 1, 9, -17, 33, 1, 2, -70, 1, 5)[k] for k in range(16)})
    c.update(sub_block(0, 1, {k: 1 for k in range(0, 16, 3)}))
    return [a, b, c]


def levels():
    """The sets of level_blocks() in 16x16 luma and chroma blocks, intra and inter, at a small QP (the large levels stay inside 16 bits) -- and blocks
    whose scaled coefficients meet the 16-bit clip at both ends and whose first transform stage clips, at QP 51"""
    rng = np.random.default_rng(0xD301)
    seq = base_seq(64, 64)
    blocks = level_blocks()
    clip = [{(0, 0): 900, (1, 0): -900, (0, 1): 700}, {(0, 0): -900, (0, 1): -900, (0, 2): -900, (0, 3): -900, (1, 1): 800},
            {(2, 0): 850, (2, 1): 850, (2, 2): 850, (2, 3): -850}]
    small = {(0, 0): 1, (1, 0): -1}
    pics = [pcm_picture(rng, seq)]
    for k, qp in enumerate((4, 51)):
        src = blocks if qp == 4 else clip
        iu, pu = [], []
        for a in range(4):
            crop = lambda s_: {(x, y): v for (x, y), v in s_.items() if x < 8 and y < 8}
            coef16 = [{0: src[(a + q) % len(src)], 1: (crop(src[(a + q + 1) % len(src)]) if q % 2 == 0 else small),
                       2: (crop(src[(a + q + 2) % len(src)]) if q % 2 else small)} for q in range(4)]
            coef4 = [{0: {(x, y): v for (x, y), v in clip[(a + i) % 3].items() if x < 4 and y < 4}} for i in range(64)]
            for i in range(3, 64, 4):
                coef4[i][1], coef4[i][2] = coef4[i][0], coef4[(i + 1) % 64][0]
            if a < 3 or qp == 4:
                iu.append(intra([(1, 10, 26, 0)[a]], a, 1, coef16))
                pu.append(inter(0, (4 * a - 5, 3 - 2 * a), 1, coef16))
            else:
                iu.append(dict(t="split", sub=[intra([1], q, 2, coef4[16 * q:16 * q + 16]) for q in range(4)]))
                pu.append(inter(0, (0, 0), 3, coef4))
        pics.append(dict(kind="P", poc=2 + 4 * k, is_ref=False, qp=qp, layout="pic", cus=iu))
        pics.append(dict(kind="P", poc=4 + 4 * k, is_ref=False, qp=qp, cus=pu))
    return seq, pics


# ---- sign_hiding ----------------------------------------------------------------------------------------------------------------------------------
def hidden(levels_by_pos):
    """the levels with the lowest position's sign set to what the parity of the sum says (9.3.4.3... 7.3.8.11: an odd sum is a negative level)"""
    lo = min(levels_by_pos)
    odd = sum(abs(v) for v in levels_by_pos.values()) & 1
    out = dict(levels_by_pos)
    out[lo] = -abs(out[lo]) if odd else abs(out[lo])
    return out


def sign_hiding():
    """sign_data_hiding_enabled_flag 1.  Sub-blocks whose first and last significant positions are exactly 3 apart (every sign coded) and exactly 4
    apart (one hidden), with odd and with even sums; a bypass unit in the same stream, where nothing is hidden whatever the distance.  (The sets are
    laid out by diagonal scan position, so the intra units that hide use modes with the diagonal scan.)"""
    rng = np.random.default_rng(0xD401)
    seq = base_seq(64, 32, ctb_log2=4, sign_hiding=1, transquant_bypass=1)
    sets = [sub_block(0, 0, {2: 3, 5: -2}), sub_block(0, 0, {2: -3, 5: 3}),                       # distance 3, sums 5 and 6: not hidden
            sub_block(0, 0, hidden({1: 3, 5: -2})), sub_block(0, 0, hidden({1: 2, 3: 1, 5: 3})),  # distance 4, odd and even
            sub_block(0, 0, hidden({0: 1, 15: -4, 7: 2})), sub_block(0, 0, hidden({0: 2, 9: 1, 15: 1}))]
    two = dict(sub_block(1, 1, hidden({3: 2, 10: -1, 12: 1})))      # 8x8: two sub-blocks that hide, one that does not
    two.update(sub_block(0, 1, hidden({2: 1, 6: -5})))
    two.update(sub_block(0, 0, {4: 1, 6: 2}))
    free = sub_block(0, 0, {0: -1, 15: 3, 7: 1})                    # odd sum with a negative and with a positive lowest level: legal only without hiding
    free2 = sub_block(0, 0, {0: 1, 15: 3, 7: 1})
    units = []
    for a in range(8):
        coef4 = [{0: sets[(a + i) % 6], **({1: sets[(a + i + 1) % 6], 2: sets[(a + i + 2) % 6]} if i % 4 == 3 else {})} for i in range(16)]
        coef8 = [{0: two, 1: sets[(a + q) % 6], 2: sets[(a + q + 3) % 6]} for q in range(4)]
        byp = [{0: (free, free2)[i % 2], **({1: free, 2: free2} if i % 4 == 3 else {})} for i in range(16)]
        units.append([intra([1], 0, 2, coef4), inter(0, (3, -2), 1, coef8), intra([10], 4, 2, byp, bypass=1), inter(0, (0, 5), 2, coef4),
                      intra([18], 3, 1, coef8), inter(0, (-4, 0), 2, byp, bypass=1), intra([0], 3, 2, coef4), inter(0, (1, 1), 1, coef8)][a])
    return seq, [pcm_picture(rng, seq), dict(kind="P", poc=2, is_ref=False, qp=24, cus=units)]


# ---- tskip_bypass ---------------------------------------------------------------------------------------------------------------------------------
def tskip_bypass():
    """transform_skip_enabled_flag and transquant_bypass_enabled_flag 1.  4x4 blocks with transform_skip_flag for luma only, Cb only, Cr only and all
    three (the chroma pair of "Cb only" / "Cr only" has its other component transformed); bypass units of 8 .. 32 whose levels of +-255 and less
    saturate the sum at 0 and at 255; intra and inter"""
    rng = np.random.default_rng(0xD501)
    seq = base_seq(64, 64, transform_skip=1, transquant_bypass=1)
    blk = lambda: {(int(x), int(y)): int(v) for x, y, v in zip(rng.integers(0, 4, 5), rng.integers(0, 4, 5), rng.choice([-9, -4, -1, 2, 5, 11], 5))}
    combos = [{0}, {1}, {2}, {0, 1, 2}, set()]

    def coef4(shift):
        out = []
        for i in range(64):
            e = {0: blk(), "tskip": combos[(i // 4 + shift) % 5] & {0}}
            if i % 4 == 3:
                e = {0: blk(), 1: blk(), 2: blk(), "tskip": combos[(i // 4 + shift) % 5]}
                if (i // 4) % 7 == 6:
                    e = {2: blk(), "tskip": {2}} if shift else {1: blk(), "tskip": {1}}      # a transform-skipped component whose partner is not coded
            out.append(e)
        return out

    def flood(n, sign):
        cells = rng.permutation(n * n)[:n * n // 2]
        return {(int(c) % n, int(c) // n): (sign if rng.random() < 0.75 else -sign) * int(rng.integers(130, 256)) for c in cells}

    def bypass_coef(d, flip):
        lg = 5 - d
        return [{0: flood(1 << lg, (1, -1)[(i + flip) % 2]), 1: flood(1 << (lg - 1), (-1, 1)[(i + flip) % 2]), 2: flood(1 << (lg - 1), (1, -1)[(i + flip) % 2])}
                for i in range(4 ** d)]
    iu = [dict(t="split", sub=[intra([(1, 0, 10, 26)[q]], q, 2, coef4(0)[16 * q:16 * q + 16]) for q in range(4)]),
          intra([1], 4, 0, bypass_coef(0, 0), bypass=1), intra([26], 0, 1, bypass_coef(1, 1), bypass=1), intra([10], 2, 2, bypass_coef(2, 0), bypass=1)]
    pu = [inter(0, (2, 3), 3, coef4(1)), inter(0, (0, 0), 0, bypass_coef(0, 1), bypass=1), inter(0, (-7, 2), 1, bypass_coef(1, 0), bypass=1),
          inter(0, (5, -6), 2, bypass_coef(2, 1), bypass=1)]
    return seq, [pcm_picture(rng, seq), dict(kind="P", poc=2, is_ref=False, qp=30, layout="pic", cus=iu), dict(kind="P", poc=4, is_ref=False, qp=22, cus=pu)]


# ---- chroma_pairs ---------------------------------------------------------------------------------------------------------------------------------
def chroma_pairs():
    """Inter units whose chroma blocks of 16, 8 and 4 code both components, only Cb, only Cr -- with and without a luma block in front; and 4x4 luma blocks,
    where the chroma pair follows the fourth"""
    rng = np.random.default_rng(0xD601)
    seq = base_seq(128, 64)
    units = []
    for d in (0, 1, 2, 3):
        lg = 5 - d
        cn = 1 << max(lg - 1, 2)
        blk = lambda n: {(int(x), int(y)): int(v) for x, y, v in zip(rng.integers(0, n, 6), rng.integers(0, n, 6), rng.choice([-6, -3, -1, 1, 2, 7], 6))}
        for turn in range(2):
            coef = []
            for i in range(4 ** d):
                e = {}
                if (i + turn) % 2 == 0 or d == 0:
                    e[0] = blk(1 << lg)
                if lg > 2 or i % 4 == 3:
                    which = ((i // 4 if lg == 2 else i) + turn) % 3
                    if which != 2:
                        e[1] = blk(cn)
                    if which != 1:
                        e[2] = blk(cn)
                coef.append(e)
            units.append(inter(0, (int(rng.integers(-20, 20)), int(rng.integers(-20, 20))), d, coef))
    units += [inter(0, (0, 0), 0, [{0: {(0, 0): 2}, 2: {(1, 1): -4}}]), inter(0, (8, 8), 0, [{0: {(3, 3): 2}, 1: {(1, 0): 5}}])]
    return seq, [pcm_picture(rng, seq)] + chunk_pictures(seq, units, "P", 2, qp=29)


# ---- qp -------------------------------------------------------------------------------------------------------------------------------------------
def qp_case(depth):
    """cu_qp_delta_enabled_flag 1 with diff_cu_qp_delta_depth ``depth`` under 32x32 CTBs split into 16x16 intra units (depth 0: four units share a
    quantisation group and its one delta; depth 1: a group each).  Per picture a slice QP and chroma offsets (PPS -4 / 5 plus the slice's); slices of a
    picture, a CTB row and a CTB, so that groups start slices in mid-picture; deltas of both signs through every QpY % 6 and through the wrap 51 -> 0; in
    every third CTB the first unit codes nothing, so the group's delta comes with a later unit and the first keeps the predicted QP"""
    rng = np.random.default_rng(0xD700 + depth)
    seq = base_seq(96, 64, cu_qp_delta=1, diff_cu_qp_delta_depth=depth, cb_qp_offset=-4, cr_qp_offset=5, slice_chroma_qp_offsets=1)
    plan = [(26, 0, 0, "pic"), (50, 0, 0, "row"), (3, -8, -12, "row"), (47, 12, 7, "ctb"), (30, 7, 3, "pic"), (14, -8, 2, "row"), (38, 4, -5, "pic")]
    pics = []
    for k, (qp, cb, cr, layout) in enumerate(plan):
        cus = []
        for a in range(6):
            sub = []
            for q in range(4):
                coef = [{0: {(0, 0): int(rng.integers(2, 6)), (int(rng.integers(1, 16)), int(rng.integers(0, 16))): -1},
                         1: {(int(rng.integers(0, 8)), 0): int(rng.integers(2, 5))}, 2: {(0, int(rng.integers(0, 8))): -int(rng.integers(2, 5))}}]
                dqp = int(rng.integers(-6, 7)) if qp not in (50, 3) else (int(rng.integers(1, 5)) if qp == 50 else -int(rng.integers(1, 5)))
                u = intra([(1, 0, 26, 10)[(a + q) % 4]], (a + q) % 5, 0, coef, dqp=dqp)
                if a % 3 == 2 and q == 0:
                    u = intra([1], 4, 0, [None])                    # no cbf: no delta yet
                elif depth == 0 and q > (1 if a % 3 == 2 else 0):
                    del u["dqp"]                                    # the group's delta is coded already
                sub.append(u)
            cus.append(dict(t="split", sub=sub))
        pics.append(dict(kind="I", poc=2 * k, is_ref=False, qp=qp, cb_qp_offset=cb, cr_qp_offset=cr, layout=layout, cus=cus))
    return seq, pics


# ---- scaling_lists --------------------------------------------------------------------------------------------------------------------------------
def coded_list(rng, count, dc, tiny_at=None):
    v = [int(x) for x in rng.integers(8, 120, count)]
    v[1], v[2] = 9, 71                                              # m[0][1] and m[1][0] far apart: the matrix is not symmetric
    if tiny_at is not None:
        v[tiny_at] = 1
    return ("coded", v, dc)


def list_spec(rng, which):
    """"sps": coded lists that are not symmetric for sizeId 0 .. 3, some predicted from a reference list (delta > 0), some from the default (delta 0,
    the lists not named), DC 40 / 90 for 16x16 and 7 / 33 for 32x32; "pps": other coded lists"""
    if which == "sps":
        return {(0, 0): coded_list(rng, 16, None), (0, 1): ("ref", 1), (0, 3): coded_list(rng, 16, None), (0, 4): coded_list(rng, 16, None),
                (1, 0): coded_list(rng, 64, None), (1, 2): ("ref", 2), (1, 3): coded_list(rng, 64, None), (1, 4): ("ref", 1),
                (2, 0): coded_list(rng, 64, 40, tiny_at=4), (2, 1): coded_list(rng, 64, 90), (2, 2): ("ref", 1), (2, 3): coded_list(rng, 64, 90, tiny_at=4),
                (2, 5): ("ref", 2), (3, 0): coded_list(rng, 64, 7), (3, 1): coded_list(rng, 64, 33)}
    return {(s, m): coded_list(rng, 16 if s == 0 else 64, None if s < 2 else 20 + 9 * m) for s in range(4) for m in range(2 if s == 3 else 6) if (s + m) % 3}


def scaling_lists(which):
    """scaling_list_enabled_flag 1 with the default lists ("default"), coded SPS lists ("sps") or PPS lists over the SPS ones ("pps"): intra and inter
    blocks of every size and component at slice QP 0 and 31.  In "sps" the 16x16 luma lists hold a 1 at diagonal position 4 = (1, 1) x 2: a level 1
    there scales to 0 at QP 0, so a block whose only coefficient it is keeps its cbf and loses its residual"""
    rng = np.random.default_rng(0xD800)
    spec = dict(sps=None if which == "default" else list_spec(rng, "sps"), pps=list_spec(rng, "pps") if which == "pps" else None)
    seq = base_seq(64, 64, scaling_lists=spec)
    blk = lambda n, k=5: {(0, 0): int(rng.choice([-3, 2, 4])),      # (the DC entry of the 16x16 and 32x32 lists is always met)
                          **{(int(x), int(y)): int(v) for x, y, v in zip(rng.integers(0, n, k), rng.integers(0, n, k), rng.choice([-9, -4, -2, 3, 5, 14], k))}}
    pics = [pcm_picture(rng, seq)]
    for k, qp in enumerate((0, 31)):
        iu, pu = [], []
        for d in (0, 1, 2):
            lg = 5 - d
            coef = [{0: blk(1 << lg, 8), 1: blk(1 << (lg - 1)), 2: blk(1 << (lg - 1))} for _ in range(4 ** d)]
            if d == 1:
                coef[1] = {0: {(2, 2): 1}, 1: blk(8), 2: blk(8)}    # (in "sps" at QP 0: scales to 0)
                coef[2] = {0: {(3, 3): 1, (2, 3): -1, (9, 6): 3}}            # (one level of three survives)
            iu.append(intra([(1, 26, 0)[d]], d, d, coef))
            pu.append(inter(0, (3 * d, -d), d, [dict(e) for e in coef]))
        coef4 = [{0: blk(4), **({1: blk(4), 2: blk(4)} if i % 4 == 3 else {})} for i in range(64)]
        iu.append(dict(t="split", sub=[intra([1], q, 2, coef4[16 * q:16 * q + 16]) for q in range(4)]))
        pu.append(inter(0, (1, 1), 3, coef4))
        pics.append(dict(kind="P", poc=2 + 4 * k, is_ref=False, qp=qp, layout="pic", cus=iu))
        pics.append(dict(kind="P", poc=4 + 4 * k, is_ref=False, qp=qp, cus=pu))
    return seq, pics


# ---- job_split ------------------------------------------------------------------------------------------------------------------------------------
JOB_COUNTS = (31, 32, 33, 255, 256, 257)


def job_split():
    """Inter pictures of 128x128 in 16x16 CTBs whose list of residual blocks (one entry per luma block with cbf_luma, one per chroma block with a
    coefficient that survives the scaling -- here every coded level does, flat lists at QP 30) has exactly JOB_COUNTS entries.

    Derivation: a CTB is one inter unit of transform depth 1 = four 8x8 transform units, each of which yields up to three entries in decoding order:
    luma 8x8, Cb 4x4, Cr 4x4.  The units are filled in decoding order until the count is reached, so entry j is luma for j % 3 == 0, Cb for j % 3 == 1
    and Cr for j % 3 == 2, a full CTB holds 12 entries, and the CTBs behind the last entry are inter units without residual.  Hence Cb sits at entry
    7 and its Cr at 8 (two waves of 8 entries) and Cb at 31 with Cr at 32 (two workgroups of 32 entries) in every picture that is long enough; a
    count of 3 k + 2 ends on a Cb whose Cr is not coded.  Every block draws levels of its own"""
    rng = np.random.default_rng(0xD901)
    seq = base_seq(128, 128, ctb_log2=4)
    pics = [pcm_picture(rng, seq)]
    for k, count in enumerate(JOB_COUNTS):
        cus, left = [], count
        for a in range(64):
            coef = []
            for q in range(4):
                e = {}
                for c in (0, 1, 2):
                    if left > 0:
                        n = 8 if c == 0 else 4
                        e[c] = {(int(x), int(y)): int(v) for x, y, v in zip(rng.integers(0, n, 4), rng.integers(0, n, 4), rng.choice([-7, -3, -1, 1, 2, 6], 4))}
                        left -= 1
                coef.append(e)
            mv = (int(rng.integers(-12, 12)), int(rng.integers(-12, 12)))
            cus.append(inter(0, mv, 1, coef) if any(e for e in coef) else dict(t="inter", l0=(0, mv)))
        assert left == 0
        pics.append(dict(kind="P", poc=2 + 2 * k, is_ref=False, qp=30, cus=cus))
    return seq, pics


GROUPS = {
    "sizes": ("resid_sizes-intra", "resid_sizes-inter"),
    "scans": ("resid_scans",),
    "levels": ("resid_levels",),
    "sign_hiding": ("resid_sign_hiding",),
    "tskip_bypass": ("resid_tskip_bypass",),
    "chroma_pairs": ("resid_chroma_pairs",),
    "qp": ("resid_qp-depth0", "resid_qp-depth1"),
    "scaling_lists": ("resid_scaling_lists-default", "resid_scaling_lists-sps", "resid_scaling_lists-pps"),
    "job_split": ("resid_job_split",),
}
CASES = {
    "resid_sizes-intra": sizes_intra,
    "resid_sizes-inter": sizes_inter,
    "resid_scans": scans,
    "resid_levels": levels,
    "resid_sign_hiding": sign_hiding,
    "resid_tskip_bypass": tskip_bypass,
    "resid_chroma_pairs": chroma_pairs,
    "resid_qp-depth0": lambda: qp_case(0),
    "resid_qp-depth1": lambda: qp_case(1),
    "resid_scaling_lists-default": lambda: scaling_lists("default"),
    "resid_scaling_lists-sps": lambda: scaling_lists("sps"),
    "resid_scaling_lists-pps": lambda: scaling_lists("pps"),
    "resid_job_split": job_split,
}
