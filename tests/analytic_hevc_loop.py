"""The scripted H.265 streams that pin deblocking and SAO (clause 8.7; k_hevc_bs, k_hevc_deblock, k_hevc_sao and the tables that HevcPicParser writes
at the end of a picture): name -> () -> (seq, pics).

The expectation is tests/hevc_loop_ref.py's, computed from the script.  Pictures are small (at most 264 wide and 136 high).  Where the samples on both
sides of an edge must be exact the units are PCM (bS 2, the samples are the script's); the decision cases place four-line vectors p3 .. p0 | q0 .. q3 that
a seeded search chose with the restatement's own line functions, one vector per edge segment, so that every inequality of 8.7.2.5.3 is met at its
threshold and one below it (``segment_tags`` names what a segment met; tests/test_hevc_loop_host.py asserts the tags from the expectation's records).
Everything else is smooth content -- a gradient with a little noise -- at QPs where the filters act, so that a wrong strength, QP, offset or flag changes
samples."""
import functools

import numpy as np

import analytic_hevc_inter as ai
import analytic_hevc_resid as ar
import hevc_loop_ref as lr
import scripted_hevc as hw

DECISION_SETTINGS = ((32, 0, 0), (40, 0, -6), (26, 6, 0), (51, 0, 0))          # slice QP, slice_beta_offset_div2, slice_tc_offset_div2 of the vector pictures
DECISION_TAGS = (["d=beta", "d=beta-1", "dp=side", "dp=side-1", "dq=side", "dq=side-1", "dEp only", "dEq only", "gate at 10tC", "gate at 10tC-1",
                  "delta+", "delta-", "delta=+", "delta=-", "side+", "side-", "strong+", "strong-", "clip1<0", "clip1>255"]
                 + ["strong %d at its bound alone" % i for i in range(3)] + ["strong %d one below" % i for i in range(3)])
BAND_POSITIONS = (0, 1, 28, 29, 31)


def segment_tags(r):
    """What a luma segment met, from its decisions (a record of the expectation, or lr.luma_segment's first result)"""
    t = set()
    if r["d"] in (r["beta"], r["beta"] - 1) and r["beta"]:
        t.add("d=beta" if r["d"] == r["beta"] else "d=beta-1")
    if not r["dE"]:
        return t
    c = r["strong"]
    for i in range(3):
        for k in (0, 1):
            rest = all(c[m][2 * j] < c[m][2 * j + 1] for m in (0, 1) for j in range(3) if (m, j) != (k, i))
            if rest and c[k][2 * i] == c[k][2 * i + 1]:
                t.add("strong %d at its bound alone" % i)           # every other condition holds: this one alone makes dE 1
            if rest and c[k][2 * i] == c[k][2 * i + 1] - 1:
                t.add("strong %d one below" % i)
    for name, v in (("dp", r["dp"]), ("dq", r["dq"])):
        if v in (r["side"], r["side"] - 1):
            t.add(name + ("=side" if v == r["side"] else "=side-1"))
    if r["dEp"] != r["dEq"]:
        t.add("dEp only" if r["dEp"] else "dEq only")
    t |= {h for h in r["hit"] if h in DECISION_TAGS}
    t |= {"clip1" + h[2:] for h in r["hit"] if h[:2] in ("p0", "p1", "q0", "q1")}
    return t


# ---- content ----------------------------------------------------------------------------------------------------------------------------------------
def gradient(rng, seq, spread=3, span=(60, 190)):
    """(Y, Cb, Cr) of the coded size: a diagonal ramp over ``span`` with noise of +-spread"""
    W, H = hw.coded_size(seq)
    out = []
    for (w, h) in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
        ramp = span[0] + (span[1] - span[0]) * (np.arange(w)[None, :] / max(w - 1, 1) * 0.6 + np.arange(h)[:, None] / max(h - 1, 1) * 0.4)
        out.append(np.clip(np.rint(ramp) + rng.integers(-spread, spread + 1, (h, w)), 0, 255).astype(np.uint8))
    return out


def pcm_of(planes):
    Y, Cb, Cr = planes
    return lambda x, y, log2: dict(t="pcm", y=Y[y:y + (1 << log2), x:x + (1 << log2)].copy(), cb=Cb[y >> 1:(y + (1 << log2)) >> 1, x >> 1:(x + (1 << log2)) >> 1].copy(),
                                   cr=Cr[y >> 1:(y + (1 << log2)) >> 1, x >> 1:(x + (1 << log2)) >> 1].copy())


def pcm_pic(seq, planes, unit_log2=3, kind="I", poc=0, **kw):
    """a picture of PCM units of 2^unit_log2 (smaller where the picture ends inside one)"""
    return dict(kind=kind, poc=poc, cus=ai.grow(seq, pcm_of(planes), lambda x, y, log2: log2 > unit_log2), **kw)


def loop_seq(w, h, ctb_log2=4, **kw):
    kw.setdefault("deblock", 1)
    kw.setdefault("pcm_loop_filter_disabled", 0)
    return ai.base_seq(w, h, ctb_log2=ctb_log2, **kw)


# ---- loop_decisions ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decision_vectors(qp, beta_off, tc_off):
    """[(P, Q)] with P, Q = [4 lines][4 samples], index 0 next to the edge: a greedy choice from seeded candidates, one more vector for every tag of
    DECISION_TAGS that the ones before it did not meet (bS 2: tC from qp + 2)"""
    beta = lr.BETA[max(0, min(51, qp + 2 * beta_off))]
    tc = lr.TC[max(0, min(53, qp + 2 + 2 * tc_off))]
    rng = np.random.default_rng(0x10070 + qp)
    covered, out, dry = set(), [], 0
    while dry < 12000:                                               # (some tags cannot occur at some settings: 2 * dpq against an even bound - 1)
        dry += 1
        m = int(rng.choice([0, 1, 1, 2, 3, 5, 9]))
        lim = int(rng.choice([tc + 1, (5 * tc + 1) // 2 + 1, 30 * tc + 3, 8]))
        e = rng.random()
        p0 = int(rng.integers(0, 6)) if e < 0.1 else int(rng.integers(250, 256)) if e < 0.2 else int(rng.integers(30, 226))
        step = int(rng.integers(-lim, lim + 1))

        def side(v0):
            a = [int(rng.integers(-m, m + 1)) for _ in range(3)]
            if rng.random() < 0.3:
                a[2] = int(rng.integers(-12, 13))
            return [v0, v0 + a[0], v0 + a[0] + a[1], v0 + a[0] + a[1] + a[2]]
        P, Q = [side(p0)], [side(p0 + step)]
        for l in (1, 2, 3):
            if rng.random() < 0.5:
                P.append(list(P[0])), Q.append(list(Q[0]))
            else:
                j = int(rng.integers(0, 3))
                P.append([v + int(rng.integers(-j, j + 1)) for v in P[0]]), Q.append([v + int(rng.integers(-j, j + 1)) for v in Q[0]])
        P, Q = [[max(0, min(255, v)) for v in l] for l in P], [[max(0, min(255, v)) for v in l] for l in Q]
        tags = segment_tags(lr.luma_segment(P, Q, beta, tc)[0]) & set(DECISION_TAGS)
        if tags - covered:
            covered |= tags
            dry = 0
            out.append((P, Q))
            if len(covered) == len(DECISION_TAGS):
                break
    return out


def decisions(vertical):
    """PCM units of 16x16 in a picture of 128x32 (vertical edges: every segment of the 7 edges takes a vector) or 32x128 (horizontal edges: the vectors lie in
    the columns 0 .. 11 and 20 .. 31, which the vertical edge at 16 -- filtered first -- leaves alone)"""
    def build():
        seq = loop_seq(128, 32) if vertical else loop_seq(32, 128)
        pics = []
        for (qp, bo, to) in DECISION_SETTINGS:
            vec = list(decision_vectors(qp, bo, to))
            slots = [(16 * e, 4 * s) for e in range(1, 8) for s in (range(8) if vertical else (0, 1, 2, 5, 6, 7))]
            while vec:
                Y = np.full((32, 128), 128, np.int64)
                for (edge, off), (P, Q) in zip(slots, vec):
                    for l in range(4):
                        Y[off + l, edge - 8:edge] = [P[l][3]] * 4 + P[l][::-1]
                        Y[off + l, edge:edge + 8] = Q[l] + [Q[l][3]] * 4
                vec = vec[len(slots):]
                Y = (Y if vertical else Y.T).astype(np.uint8)
                C = np.full((Y.shape[0] // 2, Y.shape[1] // 2), 128, np.uint8)
                pics.append(pcm_pic(seq, (Y, C, C), 4, poc=len(pics), is_ref=False, qp=qp, deblock=1, beta=bo, tc=to))
        return seq, pics
    return build


QP_PLAN = ((0, 0, 0), (10, 0, 0), (51, 6, 6), (51, -6, -6), (3, -6, -6), (20, 0, -3), (22, 6, 6), (45, -6, -6), (36, 3, -2))


def decisions_qp():
    """8x8 PCM units of smooth content at slice QPs 0 .. 51 with slice offsets -6 .. 6: beta and tC 0 at a low QP, both index clips (51 and 53, and 0)"""
    rng = np.random.default_rng(0x10071)
    seq = loop_seq(64, 32)
    return seq, [pcm_pic(seq, gradient(rng, seq, 2 + k % 3), 3, poc=k, is_ref=False, qp=qp, deblock=1, beta=bo, tc=to) for k, (qp, bo, to) in enumerate(QP_PLAN)]


# ---- loop_strength ----------------------------------------------------------------------------------------------------------------------------------
def one(l0=None, l1=None, coef=None):
    u = dict(t="inter", part="2Nx2N", pus=[{k: (v[0], v[1], 0) for k, v in (("l0", l0), ("l1", l1)) if v}])
    if coef:
        u.update(tu=0, coef=[{0: {(1, 0): coef}}])
    return u


def strength_p():
    """A P picture of 16x16 units, one slice each (the predictor is (0, 0): the scripted difference is the vector), over two PCM pictures; list 0 has
    three entries, the third is the first picture again.  Neighbours differ by 3 and by 4 in x and in y, by the picture, by the index alone; a unit with
    coefficients stands between two without"""
    rng = np.random.default_rng(0x10072)
    seq = loop_seq(128, 48, init_qp=44)
    row0 = [one((0, (0, 0))), one((0, (3, 0))), one((0, (7, 0))), one((0, (7, 3))), one((0, (7, 7))), one((1, (7, 7))), one((2, (7, 7))), one((0, (7, 7)))]
    row1 = [one((0, (0, 4))), one((0, (0, 4))), one((0, (0, 4)), coef=3), one((0, (0, 4))), one((0, (-4, 4))), one((0, (-4, 4)), coef=-3), one((0, (-4, 8))), one((2, (-4, 5)))]
    row2 = [one((0, (0, 1))), one((0, (0, 8))), one((0, (0, 4))), one((0, (0, 4))), one((2, (-4, 4))), one((0, (-4, 4))), one((0, (-7, 8))), one((1, (-4, 5)))]
    pics = [pcm_pic(seq, gradient(rng, seq), 4), pcm_pic(seq, gradient(rng, seq, span=(90, 160)), 4, "P", 1),
            dict(kind="P", poc=2, layout="ctb", n_ref=(3, 3), cus=row0 + row1 + row2)]
    return seq, pics


def strength_b():
    """A B picture at POC 4 between PCM pictures at POC 0 and 8: list 0 = (0, 8), list 1 = (8, 0).  Two vectors on two pictures in the same and in the
    other order of lists (straight and crossed), one against two vectors, both vectors on one picture with the straight and the crossed pairing 3 and 4
    apart"""
    rng = np.random.default_rng(0x10073)
    seq = loop_seq(128, 96, init_qp=44)
    two = lambda a, b: one((0, a), (0, b))                          # POC 0 by list 0, POC 8 by list 1
    rev = lambda a, b: one((1, b), (1, a))                          # POC 8 by list 0, POC 0 by list 1: the same pictures, the lists crossed
    same = lambda a, b: one((0, a), (1, b))                         # POC 0 twice
    row0 = [two((0, 0), (0, 0)), two((3, 0), (0, 3)), two((7, 0), (0, 3)), rev((7, 3), (0, 0)), two((7, 3), (0, 4)), rev((7, 7), (0, 4)), one((0, (7, 7))), one(None, (1, (7, 7)))]
    row1 = [same((0, 0), (8, 8)), same((3, 0), (8, 11)), same((11, 8), (0, 3)), same((4, 8), (4, 3)), same((4, 4), (8, 7)), same((8, 8), (4, 0)), same((12, 8), (0, 0)), two((12, 8), (0, 0))]
    row2 = [same((8, 8), (0, 0)), same((0, 0), (8, 8)), same((0, 4), (8, 8)), same((8, 8), (0, 0)), same((8, 12), (4, 0)), one((1, (0, 0))), one(None, (0, (0, 3))), one(None, (0, (0, 7)))]
    # row 0 has the straight pairing 3 and 4 apart in x and the crossed one in y; row 3 the other way round
    row3 = [two((0, 0), (0, 0)), two((0, 3), (3, 0)), two((0, 7), (3, 0)), rev((3, 7), (3, 0)), two((7, 7), (3, 0)), one((0, (0, 0))), one((0, (0, 0))), one((0, (0, 0)))]
    # rows 4 and 5: both vectors on POC 0, in pairs of units (0, 0) / (20, 20) | its neighbour.  Row 4: the straight pairing 3 apart in x, in y (the crossed
    # one far: bS 0), then far by 4 in x alone and in y alone, every other component of both straight pairs at 3 or below (bS 1).  Row 5: the same for the
    # crossed pairing -- the neighbour has the vectors in the other order
    base = same((0, 0), (20, 20))
    row4 = [base, same((3, 0), (20, 20)), base, same((0, 3), (20, 20)), base, same((4, 3), (23, 17)), base, same((3, 4), (17, 23))]
    row5 = [base, same((20, 20), (3, 0)), base, same((20, 20), (0, 3)), base, same((23, 17), (4, 3)), base, same((17, 23), (3, 4))]
    pics = [pcm_pic(seq, gradient(rng, seq), 4), pcm_pic(seq, gradient(rng, seq, span=(90, 160)), 4, "P", 8),
            dict(kind="B", poc=4, layout="ctb", n_ref=(2, 2), cus=row0 + row1 + row2 + row3 + row4 + row5)]
    return seq, pics


def strength_random(ctb_log2, seed):
    """P and B pictures of random units (all partitions, AMP, merge, skip, residual at both transform depths, PCM) in one slice over smooth PCM pictures"""
    def build():
        rng = np.random.default_rng(seed)
        size = {4: (80, 48), 5: (96, 72), 6: (136, 72)}[ctb_log2]
        seq = loop_seq(*size, ctb_log2=ctb_log2, amp=1, tu_depth_inter=1, init_qp=42)
        pics = [pcm_pic(seq, gradient(rng, seq), 3), pcm_pic(seq, gradient(rng, seq, span=(80, 170)), 4, "P", 8)]
        for kind, poc in (("P", 9), ("B", 4), ("B", 5)):
            pics.append(ai.random_pic(rng, seq, kind, poc, (2, 2), max_merge=3, layout="pic", p_pcm=0.05, p_skip=0.1, p_coef=0.4, wide=9, is_ref=False,
                                      p_split={4: 0.5, 5: 0.6, 6: 0.75}[ctb_log2]))
        if ctb_log2 == 6:                                           # a unit of 64 whose transform tree splits at 32 (inferred: 32 is the largest transform block)
            big = dict(t="inter", part="2Nx2N", pus=[dict(l0=(0, (2, 1), 0))], tu=1, coef=[{0: {(0, 0): 3}}, None, {0: {(1, 0): -2}}, {0: {(0, 0): 2}}])
            rest = ai.grow(seq, lambda x, y, log2: dict(t="skip", merge=0))
            pics.append(dict(kind="P", poc=10, layout="pic", n_ref=(2, 2), is_ref=False, cus=[big] + rest[1:]))
        return seq, pics
    return build


def strength_intra():
    """Intra units: 8x8 with four 4x4 prediction and transform blocks, 16x16 with transform depth 2 (4x4 blocks) and 1, 32x32 with depth 1 and 2: inner
    edges at 4 and 12 lie off the grid, those at 8, 16 and 24 on it"""
    rng = np.random.default_rng(0x10074)
    seq = ar.base_seq(64, 64, deblock=1, init_qp=38)
    lv = lambda: {0: {(0, 0): int(rng.integers(-6, 7)) or 2}}
    nxn = lambda: ar.intra([1, 0, 1, 0], 4, 1, [lv() for _ in range(4)])
    u16 = lambda tu: ar.intra([1], 4, tu, [lv() if i % 4 == 3 or tu < 2 else {0: {(0, 0): 1 + i % 3}} for i in range(4 ** tu)])
    split = lambda subs: dict(t="split", sub=subs)
    cus = [split([split([nxn() for _ in range(4)]), u16(2), u16(1), u16(0)]), ar.intra([0], 4, 1, [lv() for _ in range(4)]),
           ar.intra([1], 4, 2, [lv() for _ in range(16)]), split([u16(1), split([nxn() for _ in range(4)]), u16(2), u16(2)])]
    return seq, [dict(kind="I", poc=0, cus=cus)]


# ---- loop_qp ----------------------------------------------------------------------------------------------------------------------------------------
def qp_case(depth, pcm_disabled):
    """cu_qp_delta_enabled_flag 1 (diff_cu_qp_delta_depth ``depth``) under 32x32 CTBs of four 16x16 units: DC-predicted intra units with a delta, PCM
    units, bypass units, units without coefficients; PPS chroma offsets -5 (Cb) and 9 (Cr), slice offsets that the filter must ignore.  The last picture
    is a P picture, a slice per CTB: a skipped unit in front of the unit that carries the group's delta"""
    rng = np.random.default_rng(0x10075 + depth)
    seq = ar.base_seq(96, 64, cu_qp_delta=1, diff_cu_qp_delta_depth=depth, cb_qp_offset=-5, cr_qp_offset=9, slice_chroma_qp_offsets=1, transquant_bypass=1,
                      deblock=1, pcm_loop_filter_disabled=pcm_disabled)
    flat = lambda n, v: dict(t="pcm", y=np.clip(v + rng.integers(-2, 3, (n, n)), 0, 255).astype(np.uint8), cb=np.full((n // 2, n // 2), v - 6, np.uint8),
                             cr=np.full((n // 2, n // 2), v + 9, np.uint8))
    plan = [(27, 3, -4, "pic"), (44, -6, 5, "row"), (33, 0, 0, "ctb"), (49, 4, 4, "pic"), (38, -3, 2, "pic")]
    pics = []
    for k, (qp, cb, cr, layout) in enumerate(plan):
        cus = []
        for a in range(6):
            sub = []
            for q in range(4):
                kind = (a + q + k) % 5
                coef = [{0: {(0, 0): int(rng.integers(1, 4))}, 1: {(0, 0): int(rng.integers(1, 3))}, 2: {(0, 0): -int(rng.integers(1, 3))}}]
                dqp = int(rng.integers(-5, 6)) | 1 if q % 2 else int(rng.integers(-3, 4)) * 2      # odd and even deltas: sums of both parities
                if kind == 0:
                    u = flat(16, 118 + 2 * a)
                elif kind == 1:
                    u = ar.intra([1], 4, 0, [{0: {(0, 0): 2, (1, 0): -1}, 1: {(0, 0): 1}}], bypass=1)
                elif kind == 2 and q:
                    u = ar.intra([1], 4, 0, [None])
                else:
                    u = ar.intra([1], 4, 0, coef, dqp=dqp)
                if kind == 1:
                    u["dqp"] = dqp                                  # (a bypass unit with coefficients carries the delta like any other)
                if depth == 0 and "dqp" in u and any("dqp" in s for s in sub):
                    del u["dqp"]                                    # the group's delta is coded already
                sub.append(u)
            cus.append(dict(t="split", sub=sub))
        pics.append(dict(kind="I", poc=2 * k, is_ref=k == 0, qp=qp, cb_qp_offset=cb, cr_qp_offset=cr, layout=layout, cus=cus))
    cus = [dict(t="split", sub=[dict(t="skip"), ar.intra([1], 4, 0, [{0: {(0, 0): 2}}], dqp=(3, -5, 7, -2, 5, -7)[a]), dict(t="skip"), flat(16, 120)]) for a in range(6)]
    pics.append(dict(kind="P", poc=2 * len(plan), is_ref=False, qp=35, layout="ctb", cus=cus))
    return seq, pics


# ---- SAO scripts ------------------------------------------------------------------------------------------------------------------------------------
def sao_script(rng, seq, p, p_merge=0.25, p_off=0.12, classes=None, magnitudes=None):
    """sao_ctbs for the picture p (its slices and their flags are read): band positions through BAND_POSITIONS, all classes, merges where the slice allows"""
    cw, ch = hw.ctb_dims(seq)
    out, n_band = [], 0

    def entry(c):
        nonlocal n_band
        if rng.random() < p_off:
            return None
        if rng.random() < 0.45:
            n_band += 1
            pos = BAND_POSITIONS[n_band % 5] if n_band % 3 else int(rng.integers(0, 32))
            return ("band", pos, tuple(int(v) for v in rng.choice([-7, -6, -4, -3, -1, 0, 1, 2, 5, 7], 4)))
        mags = magnitudes or tuple(int(v) for v in rng.choice([0, 1, 2, 3, 4, 5, 6, 7], 4))
        return ("edge", int(rng.integers(0, 4)) if classes is None else classes[len(out) % len(classes)], mags)
    for sl in hw.slice_table(seq, p):
        for a in range(sl["first"], sl["first"] + sl["count"]):
            if not (sl["sao"][0] or sl["sao"][1]):
                out.append(None)
                continue
            left, up = a % cw > 0 and a - 1 >= sl["first"], a - cw >= sl["first"]
            r = rng.random()
            if left and r < p_merge:
                out.append(dict(merge="left"))
            elif up and r < 2 * p_merge:
                out.append(dict(merge="up"))
            else:
                y = entry(0) if sl["sao"][0] else None
                cb = entry(1) if sl["sao"][1] else None
                cr = None
                if cb is not None:
                    cr = entry(2)
                    while cr is None or cr[0] != cb[0]:
                        cr = entry(2)
                    if cb[0] == "edge":
                        cr = ("edge", cb[1], cr[2])
                out.append(dict(merge=None, y=y, c=(cb, cr) if cb is not None else None))
    return out


def with_sao(rng, seq, p, **kw):
    p["sao_ctbs"] = sao_script(rng, seq, p, **kw)
    return p


def sao_case(w, h, ctb_log2, seed):
    """Smooth PCM pictures that run from 0 to 255 (offsets of 7 clip at both ends) with SAO: deblocking on and off, luma only, chroma only, one slice
    with SAO between slices without, merges left and up and of merged CTBs"""
    def build():
        rng = np.random.default_rng(seed)
        seq = loop_seq(w, h, ctb_log2=ctb_log2, sao=1)
        n = hw.ctb_dims(seq)[0] * hw.ctb_dims(seq)[1]
        unit = min(ctb_log2, 5)
        pic = lambda k, **kw: pcm_pic(seq, gradient(rng, seq, 3, (-20, 275)), unit if k % 2 else 3, poc=k, is_ref=False, qp=(30, 40, 46)[k % 3], **kw)
        pics = [with_sao(rng, seq, pic(0, sao=(1, 1))), with_sao(rng, seq, pic(1, sao=(1, 1), deblock=0)), with_sao(rng, seq, pic(2, sao=(1, 0)), p_merge=0.35),
                with_sao(rng, seq, pic(3, sao=(0, 1), deblock=0)), with_sao(rng, seq, pic(4, sao=(1, 1)), p_merge=0.0, p_off=0.0, magnitudes=(7, 7, 7, 7))]
        seven = lambda pos, sign: ("band", pos, (7 * sign, 7 * sign, 7 * sign, 7 * sign))
        pics[4]["sao_ctbs"][0] = dict(merge=None, y=seven(0, -1), c=(seven(31, -1), seven(29, -1)))        # the ramp begins at 0 in the first CTB and ends at 255
        pics[4]["sao_ctbs"][-1] = dict(merge=None, y=seven(28, 1), c=(seven(29, 1), seven(31, 1)))         # in the last one
        if n >= 3:
            firsts = sorted({0, n // 3, 2 * n // 3})
            pics.append(with_sao(rng, seq, pic(5, slices=[dict(first=f, sao=(1, 1) if i == 1 else (0, 0)) for i, f in enumerate(firsts)])))
            pics.append(with_sao(rng, seq, pic(6, slices=[dict(first=f, sao=(0, 0) if i == 1 else (1, 1)) for i, f in enumerate(firsts)]), p_off=0.4))
        return seq, pics
    return build


def textured(rng, seq, exempt_every):
    """intra units of 16x16 and 8x8 with a few coefficients; every ``exempt_every``-th 8x8 unit is PCM or a bypass unit"""
    count = [0]

    def leaf(x, y, log2):
        n = 1 << log2
        count[0] += 1
        if log2 == 3 and count[0] % exempt_every == 0:
            if count[0] % (2 * exempt_every):
                return dict(t="pcm", y=rng.integers(100, 140, (n, n)).astype(np.uint8), cb=rng.integers(100, 140, (n // 2, n // 2)).astype(np.uint8),
                            cr=rng.integers(100, 140, (n // 2, n // 2)).astype(np.uint8))
            return ar.intra([1], 4, 0, [{0: {(int(rng.integers(0, 8)), int(rng.integers(0, 8))): int(rng.integers(4, 12)), (0, 0): -3}, 1: {(1, 1): 5}, 2: {(2, 0): -6}}], bypass=1)
        lv = lambda m: {(int(rng.integers(0, m)), int(rng.integers(0, m))): int(rng.choice([-3, -2, 2, 3])), (0, 0): int(rng.integers(-4, 5)) or 1}
        return ar.intra([int(rng.choice([0, 1, 10, 26, 18]))], 4, 0, [{0: lv(n), 1: lv(n // 2), 2: lv(n // 2)}])
    return ai.grow(seq, leaf, lambda x, y, log2: log2 > 4 or (log2 == 4 and (x + y) % 32 == 0))


def sao_exempt():
    """pcm_loop_filter_disabled_flag 1 and cu_transquant_bypass: 8x8 PCM and bypass units inside CTBs whose other units SAO changes"""
    rng = np.random.default_rng(0x10078)
    seq = ar.base_seq(64, 64, deblock=1, pcm_loop_filter_disabled=1, transquant_bypass=1, sao=1, init_qp=30)
    pics = []
    for k in range(2):
        p = dict(kind="I", poc=k, is_ref=False, sao=(1, 1), cus=textured(rng, seq, 3))
        pics.append(with_sao(rng, seq, p, p_merge=0.0, p_off=0.0))
    return seq, pics


def sao_slices(later, earlier):
    """64x48 in 16x16 CTBs, slices that begin at the CTBs 0, 5 and 10 (in mid-row), every CTB with the edge offset of one class per picture: each of the
    eight neighbour directions crosses a slice boundary.  The slice at 5 has the across flag ``later``, the slices at 0 and 10 have ``earlier``: the
    boundary 0 | 5 is decided by the later slice's flag, the boundary 5 | 10 too -- there the slice at 5 is the EARLIER one"""
    def build():
        rng = np.random.default_rng(0x10079)
        seq = loop_seq(64, 48, sao=1)
        pics = []
        for cls in range(4):
            p = pcm_pic(seq, gradient(rng, seq, 4), 4, poc=cls, is_ref=False, qp=40, sao=(1, 1),
                        slices=[dict(first=0, across=earlier), dict(first=5, across=later), dict(first=10, across=earlier)])
            pics.append(with_sao(rng, seq, p, p_merge=0.0, p_off=0.0, classes=[cls], magnitudes=(3, 1, 2, 4)))
            for e in p["sao_ctbs"]:                                 # edge offsets everywhere
                for key in ("y",):
                    if e[key][0] != "edge":
                        e[key] = ("edge", cls, (3, 1, 2, 4))
                if e["c"][0][0] != "edge":
                    e["c"] = (("edge", cls, (2, 2, 1, 1)), ("edge", cls, (1, 3, 3, 1)))
        return seq, pics
    return build


# ---- loop_slices ------------------------------------------------------------------------------------------------------------------------------------
def slices_case():
    """64x48 in 16x16 CTBs of 8x8 PCM units: slices of a CTB and of a CTB row; the filter disabled in the middle slice; the across flag 0 / 1 in the
    earlier and the later slice with the later slice beginning in mid-row (a left and a top boundary); offsets that differ between neighbouring slices;
    PPS offsets inherited by one slice and overridden by the next"""
    rng = np.random.default_rng(0x1007A)
    seq = loop_seq(64, 48, pps_beta=2, pps_tc=-2)
    pic = lambda k, **kw: pcm_pic(seq, gradient(rng, seq, 3), 3, poc=k, is_ref=False, qp=(38, 44)[k % 2], **kw)
    pics = [pic(0, layout="ctb"), pic(1, layout="row"),
            pic(2, slices=[dict(first=0), dict(first=5, deblock=0), dict(first=10)]),
            pic(3, slices=[dict(first=0, deblock=1, beta=-3, tc=2), dict(first=6, deblock=1, beta=5, tc=-4)]),
            pic(4, slices=[dict(first=0), dict(first=6, deblock=1, beta=-4, tc=4)])]
    for k, (e, l) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        pics.append(pic(5 + k, slices=[dict(first=0, across=e), dict(first=6, across=l)]))
    return seq, pics


# ---- loop_reference, loop_launch --------------------------------------------------------------------------------------------------------------------
def reference_case():
    """A P and a B picture, one slice per 16x16 CTB, with full-sample and fractional vectors into pictures that deblocking and SAO changed -- the P picture
    (itself filtered) is the B picture's second reference"""
    rng = np.random.default_rng(0x1007B)
    seq = loop_seq(64, 48, sao=1, init_qp=42)
    mv = [(0, 0), (4, 8), (-8, 4), (5, 0), (0, -7), (2, 2), (16, -16), (-3, 9), (12, 0), (0, 12), (-6, -6), (1, 3)]
    i0 = with_sao(rng, seq, pcm_pic(seq, gradient(rng, seq, 4), 3, sao=(1, 1)), p_off=0.0)
    p1 = with_sao(rng, seq, dict(kind="P", poc=8, layout="ctb", sao=(1, 1), cus=[one((0, v)) for v in mv]), p_merge=0.0)
    b2 = with_sao(rng, seq, dict(kind="B", poc=4, layout="ctb", sao=(1, 0), cus=[one((0, v), (0, mv[(i + 5) % 12])) for i, v in enumerate(mv)]), p_merge=0.0)
    return seq, [i0, p1, b2]


def launch_case(w, h):
    def build():
        rng = np.random.default_rng(0x1007C + w + h)
        seq = loop_seq(w, h, sao=1)
        pics = [with_sao(rng, seq, pcm_pic(seq, gradient(rng, seq, 3), 3, poc=k, is_ref=False, qp=36 + 4 * k, sao=(1, 1))) for k in range(2)]
        return seq, pics
    return build


def launch_alternate():
    """six pictures whose slice headers switch deblocking and SAO on and off in turn"""
    rng = np.random.default_rng(0x1007D)
    seq = loop_seq(64, 64, sao=1)
    pics = []
    for k in range(6):
        p = pcm_pic(seq, gradient(rng, seq, 3), 3, poc=k, is_ref=False, qp=40, deblock=k % 2, sao=((k >> 1) % 2, (k >> 1) % 2) if k < 4 else (1 - k % 2, k % 2))
        pics.append(with_sao(rng, seq, p))
    return seq, pics


GROUPS = {
    "loop_decisions": ("loop_decisions-vertical", "loop_decisions-horizontal", "loop_decisions-qp"),
    "loop_strength": ("loop_strength-p", "loop_strength-b", "loop_strength-random16", "loop_strength-random32", "loop_strength-random64", "loop_strength-intra"),
    "loop_qp": ("loop_qp-depth0-pcm_exempt", "loop_qp-depth1-pcm_filtered"),
    "loop_slices": ("loop_slices",),
    "loop_sao": ("loop_sao-8x32", "loop_sao-72x40", "loop_sao-88x72", "loop_sao-264x24", "loop_sao-exempt"),
    "loop_sao_slices": ("loop_sao_slices-later0", "loop_sao_slices-earlier0"),
    "loop_reference": ("loop_reference",),
    "loop_launch": ("loop_launch-64x128", "loop_launch-64x120", "loop_launch-72x120", "loop_launch-64x136", "loop_launch-alternate"),
}
CASES = {
    "loop_decisions-vertical": decisions(True),
    "loop_decisions-horizontal": decisions(False),
    "loop_decisions-qp": decisions_qp,
    "loop_strength-p": strength_p,
    "loop_strength-b": strength_b,
    "loop_strength-random16": strength_random(4, 0x10080),
    "loop_strength-random32": strength_random(5, 0x10081),
    "loop_strength-random64": strength_random(6, 0x10082),
    "loop_strength-intra": strength_intra,
    "loop_qp-depth0-pcm_exempt": lambda: qp_case(0, 1),
    "loop_qp-depth1-pcm_filtered": lambda: qp_case(1, 0),
    "loop_slices": slices_case,
    "loop_sao-8x32": sao_case(8, 32, 4, 0x10090),
    "loop_sao-72x40": sao_case(72, 40, 5, 0x10091),
    "loop_sao-88x72": sao_case(88, 72, 6, 0x10092),
    "loop_sao-264x24": sao_case(264, 24, 4, 0x10093),
    "loop_sao-exempt": sao_exempt,
    "loop_sao_slices-later0": sao_slices(0, 1),
    "loop_sao_slices-earlier0": sao_slices(1, 0),
    "loop_reference": reference_case,
    "loop_launch-64x128": launch_case(64, 128),
    "loop_launch-64x120": launch_case(64, 120),
    "loop_launch-72x120": launch_case(72, 120),
    "loop_launch-64x136": launch_case(64, 136),
    "loop_launch-alternate": launch_alternate,
}
assert sorted(n for g in GROUPS.values() for n in g) == sorted(CASES)
