"""Expected pictures and the known-answer cases of the scripted H.265 streams (tests/scripted_hevc.py): computed from the script alone.

Interpolation is the literal restatement of 8.5.3.3.3 in tests/test_hevc_mc_packed.py (``luma_literal`` / ``chroma_literal`` and the tap tables typed
there from Tables 8-11 / 8-12), vectorised here; the host test checks the vectorised form against the scalar one.  Weighted prediction is 8.5.3.3.4
typed out.  Deblocking is never computed: the cases choose streams on which the filter, when on, must be the identity.

Closed form on ramps.  For 8-bit video shift1 is 0, so the 14-bit intermediate is EXACT: the taps sum to 64, hence on f = a x + c y + d the row filter
gives 64 f + a Mx with Mx = sum_i tap_i (i - 3) -- 0, 15, 32, 49 for the luma fractions 0..3 (the quarter filters are NOT linear-exact: 15 and 49, not 16
and 48), 0, 8, 16, 26, 32, 38, 48, 56 for the chroma fractions 0..7 (i - 1 there).  The column filter over such rows gives 64 (64 f + a Mx) + 64 c My, and
shift2 = 6 removes the factor exactly: predSample = 64 f + a Mx + c My in every case.  The only rounding is the final (predSample + 32) >> 6:
    sample = f + ((a Mx[xFrac] + c My[yFrac] + 32) >> 6)
wherever the eight-tap (four-tap) footprint lies inside the picture.
"""
import numpy as np

import scripted_hevc as hw
from analytic_expect import clip1, ramp, window
from analytic_cases import pcm_from_planes
from test_hevc_mc_packed import FC, FL

CTB = hw.CTB
SIZES = [(96, 80), (90, 70)]
TAPS_L = {0: [0, 0, 0, 64, 0, 0, 0, 0], **FL}
TAPS_C = {0: [0, 64, 0, 0], **FC}
M_LUMA = [sum(t * (i - 3) for i, t in enumerate(TAPS_L[f])) for f in range(4)]
M_CHROMA = [sum(t * (i - 1) for i, t in enumerate(TAPS_C[f])) for f in range(8)]


def mc14(R, x0, y0, w, h, mv, chroma):
    """The 14-bit prediction samples of a w x h block at (x0, y0) of one plane (8.5.3.3.3.1 / .2, 8-bit video): the vector in quarter luma samples =
    eighth chroma samples; reference coordinates clamped into the picture."""
    sh, taps, n, back = (3, TAPS_C, 4, 1) if chroma else (2, TAPS_L, 8, 3)
    xi, yi, fx, fy = x0 + (mv[0] >> sh), y0 + (mv[1] >> sh), mv[0] & ((1 << sh) - 1), mv[1] & ((1 << sh) - 1)
    P = window(R, yi - back, xi - back, h + n - 1, w + n - 1)
    if fx == 0 and fy == 0:
        return P[back:back + h, back:back + w] << 6
    if fy == 0:
        return sum(taps[fx][i] * P[back:back + h, i:i + w] for i in range(n))
    if fx == 0:
        return sum(taps[fy][i] * P[i:i + h, back:back + w] for i in range(n))
    col = sum(taps[fx][i] * P[:, i:i + w] for i in range(n))
    return sum(taps[fy][j] * col[j:j + h] for j in range(n)) >> 6


def weighted(p0, p1, explicit, log2wd, e0, e1):
    """8.5.3.3.4.2 (default) / 8.5.3.3.4.3 (explicit) for 8-bit video: shift1 = 6; log2wd = the denominator + 6."""
    if not explicit:
        if p0 is not None and p1 is not None:
            return clip1((p0 + p1 + 64) >> 7)
        return clip1(((p0 if p1 is None else p1) + 32) >> 6)
    if p0 is not None and p1 is not None:
        return clip1((p0 * e0[0] + p1 * e1[0] + ((e0[1] + e1[1] + 1) << log2wd)) >> (log2wd + 1))
    p, (w, o) = (p0, e0) if p1 is None else (p1, e1)
    return clip1(((p * w + (1 << (log2wd - 1))) >> log2wd) + o)


def expect_hevc(seq, pics):
    """[(Y, Cb, Cr)] per picture in DECODE order, coded size, uint8."""
    W, H = hw.coded_size(seq)
    cw = W // CTB
    plans = hw.plan(seq, pics)
    out = []
    for k, (p, pl) in enumerate(zip(pics, plans)):
        planes = [np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)]
        kind = p["kind"]
        explicit = bool((kind == "P" and seq.get("weighted_pred", 0)) or (kind == "B" and seq.get("weighted_bipred", 0)))
        wp = p.get("wp", dict(ld_y=0, ld_c=0))
        for a, u in enumerate(p["cus"]):
            x, y = a % cw, a // cw
            if u["t"] == "pcm":
                for c, key in enumerate(("y", "cb", "cr")):
                    s = CTB if c == 0 else CTB // 2
                    planes[c][y * s:(y + 1) * s, x * s:(x + 1) * s] = u[key]
                continue
            if u["t"] == "skip":
                # 8.5.3.2.2 - 8.5.3.2.5: no spatial or temporal candidate -> the zero candidate: vector (0, 0) on index 0, of both lists in a B slice
                u = dict(t="inter", l0=(pl["l0"][0], (0, 0)), l1=(pl["l1"][0], (0, 0)) if kind == "B" else None)
            for c in (0, 1, 2):
                s = CTB if c == 0 else CTB // 2
                pr, ent = [None, None], [None, None]
                ld = wp["ld_y"] if c == 0 else wp["ld_c"]
                for l, q in enumerate((u.get("l0"), u.get("l1"))):
                    if not q:
                        continue
                    pr[l] = mc14(out[q[0]][c], x * s, y * s, s, s, q[1], c > 0)
                    lst = wp.get("l%d" % l, [])
                    idx = pl["l%d" % l].index(q[0])
                    e = (lst[idx] if idx < len(lst) and lst[idx] else {})
                    v = e.get("y") if c == 0 else (e.get("c")[c - 1] if e.get("c") else None)
                    ent[l] = v if v is not None else (1 << ld, 0)
                planes[c][y * s:(y + 1) * s, x * s:(x + 1) * s] = weighted(pr[0], pr[1], explicit, ld + 6, ent[0], ent[1])
        out.append(tuple(planes))
    return out


def ramp_closed(f, a, c, fx, fy, chroma):
    M = M_CHROMA if chroma else M_LUMA
    return f + ((a * M[fx] + c * M[fy] + 32) >> 6)


def ramp_closed_frame(seq, p, refs_params):
    """Closed-form planes of a P picture of inter units over ramp references, and where the form applies (the filter footprint inside the plane)."""
    W, H = hw.coded_size(seq)
    cw = W // CTB
    outs = [np.zeros((H, W), np.int64), np.zeros((H // 2, W // 2), np.int64), np.zeros((H // 2, W // 2), np.int64)]
    masks = [np.zeros((H, W), bool), np.zeros((H // 2, W // 2), bool)]
    for a_, u in enumerate(p["cus"]):
        x, y = a_ % cw, a_ // cw
        pic, mv = u["l0"]
        for c in (0, 1, 2):
            s, sh = (CTB, 2) if c == 0 else (CTB // 2, 3)
            ra, rc, rd = refs_params[pic][c]
            yy, xx = np.mgrid[y * s:(y + 1) * s, x * s:(x + 1) * s]
            xi, yi = xx + (mv[0] >> sh), yy + (mv[1] >> sh)
            outs[c][yy, xx] = ramp_closed(ra * xi + rc * yi + rd, ra, rc, mv[0] & ((1 << sh) - 1), mv[1] & ((1 << sh) - 1), c > 0)
            Wc, Hc = (W, H) if c == 0 else (W // 2, H // 2)
            lo, hi = (3, 4) if c == 0 else (1, 2)
            masks[min(c, 1)][yy, xx] = (xi >= lo) & (xi + hi <= Wc - 1) & (yi >= lo) & (yi + hi <= Hc - 1)
    return outs[0], outs[1], outs[2], masks[0], masks[1]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the cases: name -> builder(width, height) -> (seq, pics)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def dims(w, h):
    return (w + CTB - 1) // CTB, (h + CTB - 1) // CTB


def noise_pic(rng, cw, ch, kind="I", poc=0, **kw):
    Y = rng.integers(0, 256, (ch * 16, cw * 16), dtype=np.uint8)
    Cb = rng.integers(0, 256, (ch * 8, cw * 8), dtype=np.uint8)
    Cr = rng.integers(0, 256, (ch * 8, cw * 8), dtype=np.uint8)
    Y[3, 0:7] = 0; Y[5, 4:8] = (0, 0, 1, 0); Cb[0, 0:4] = (0, 0, 3, 0); Cr[7, 4:8] = (0, 0, 0, 2)     # bytes that need emulation prevention
    return dict(kind=kind, poc=poc, cus=pcm_from_planes(Y, Cb, Cr, cw, ch), **kw)


def flat_pic(cw, ch, y, cb, cr, kind="I", poc=0, **kw):
    f = lambda s, v: np.full((s, s), v, np.uint8)
    return dict(kind=kind, poc=poc, cus=[dict(t="pcm", y=f(16, y), cb=f(8, cb), cr=f(8, cr)) for _ in range(cw * ch)], **kw)


def ramp_pic(cw, ch, params, kind="I", poc=0, **kw):
    (ya, yc, yd), (ba, bc, bd), (ra, rc, rd) = params
    return dict(kind=kind, poc=poc, cus=pcm_from_planes(ramp(ch * 16, cw * 16, ya, yc, yd), ramp(ch * 8, cw * 8, ba, bc, bd),
                                                        ramp(ch * 8, cw * 8, ra, rc, rd), cw, ch), **kw)


def l0(pic, mvx, mvy):
    return dict(t="inter", l0=(pic, (mvx, mvy)))


def integer_vectors_noise(w, h):
    """The reference shifted, coordinates clamped (8-228 / 8-229): up to 40 samples outside on every side, and so far outside that a block reads one
    clamped row / column."""
    rng = np.random.default_rng(0xB101)
    cw, ch = dims(w, h)
    pics = [noise_pic(rng, cw, ch)]
    for k in range(3):
        cus = []
        for a in range(cw * ch):
            x, y = a % cw, a // cw
            if k < 2:
                tx, ty = int(rng.integers(-40, cw * 16 + 24)), int(rng.integers(-40, ch * 16 + 24))
                if a % 5 == 0:
                    tx = (-40, cw * 16 + 24)[(a // 5) & 1]
                if a % 7 == 0:
                    ty = (-40, ch * 16 + 24)[(a // 7) & 1]
                mv = (4 * (tx - x * 16), 4 * (ty - y * 16))
            else:
                far = [(-200, 0), (200, 0), (0, -200), (0, 200), (-200, -200), (200, 200), (200, -200), (-200, 200), (-200, 3), (5, 200)][a % 10]
                mv = (4 * far[0], 4 * far[1])
            cus.append(l0(0, *mv))
        pics.append(dict(kind="P", poc=2 + 2 * k, cus=cus, is_ref=False))
    return dict(width=w, height=h), pics


def fractional_positions_noise(w, h):
    """All 16 luma and all 64 chroma fractions over noise against the literal restatement, every unit a different vector, some far outside."""
    rng = np.random.default_rng(0xB102)
    cw, ch = dims(w, h)
    pics = [noise_pic(rng, cw, ch)]
    n = 0
    for k in range(5):
        cus = []
        for a in range(cw * ch):
            x, y = a % cw, a // cw
            tx, ty = int(rng.integers(-24, cw * 16 + 8)), int(rng.integers(-24, ch * 16 + 8))
            if n % 11 == 0:
                tx, ty = [(-300, ty), (tx, 300), (cw * 16 + 100, -90)][(n // 11) % 3]
            cus.append(l0(0, 8 * ((tx - x * 16) // 2) + n % 8, 8 * ((ty - y * 16) // 2) + (n // 8) % 8))
            n += 1
        pics.append(dict(kind="P", poc=2 + 2 * k, cus=cus, is_ref=False))
    return dict(width=w, height=h), pics


RAMP_PARAMS = [((1, 2, 0), (2, 1, 20), (-2, -1, 250)), ((-1, -1, 200), (-2, 2, 120), (1, -2, 100)), ((-2, 0, 220), (0, -2, 90), (2, 2, 10))]


def fractional_positions_ramps(w, h):
    """Three ramp references, then P pictures walking through every fraction with integer parts of -2 .. 0 samples: the closed form of the module
    docstring where the footprint is inside, the literal restatement elsewhere."""
    rng = np.random.default_rng(0xB103)
    cw, ch = dims(w, h)
    pics = [ramp_pic(cw, ch, RAMP_PARAMS[0])] + [ramp_pic(cw, ch, RAMP_PARAMS[k], "P", 2 * k) for k in (1, 2)]
    n = 0
    for k in range(6):
        cus = []
        for a in range(cw * ch):
            cus.append(l0(k % 3, 8 * int(rng.integers(-1, 1)) + n % 8, 8 * int(rng.integers(-1, 1)) + (n // 8) % 8))
            n += 1
        pics.append(dict(kind="P", poc=6 + 2 * k, cus=cus, is_ref=False))
    return dict(width=w, height=h), pics


def skip_copies(w, h):
    """cu_skip_flag 1 with no merge candidate: P -- a copy of RefPicList0[0] at the same place; B -- (a + b + 1) >> 1 of RefPicList0[0] and
    RefPicList1[0] ((64 a + 64 b + 64) >> 7).  Skipped and moved units mixed."""
    rng = np.random.default_rng(0xB104)
    cw, ch = dims(w, h)
    n = cw * ch
    pics = [noise_pic(rng, cw, ch),
            dict(kind="P", poc=8, cus=[dict(t="skip") if a % 3 else l0(0, 4 * int(rng.integers(-8, 8)), 4 * int(rng.integers(-8, 8))) for a in range(n)]),
            dict(kind="P", poc=12, cus=[dict(t="skip") for _ in range(n)]),
            dict(kind="B", poc=4, cus=[dict(t="skip") if a % 2 else dict(t="inter", l1=(2, (4, 8))) for a in range(n)])]
    return dict(width=w, height=h), pics


def bipred_default(w, h):
    """Two flat references u, v: (u + v + 1) >> 1; two noise references at integer and fractional vectors: 8-264; single-list units between."""
    rng = np.random.default_rng(0xB105)
    cw, ch = dims(w, h)
    n = cw * ch
    pics = [flat_pic(cw, ch, 10, 255, 1), flat_pic(cw, ch, 255, 0, 254, "P", 8)]
    pics.append(dict(kind="B", poc=4, cus=[dict(t="inter", l0=(0, (0, 0)), l1=(1, (0, 0))) if i % 3 == 0 else
                                           (dict(t="inter", l0=(1, (4, -8))) if i % 3 == 1 else dict(t="inter", l1=(0, (-12, 4)))) for i in range(n)]))
    pics += [noise_pic(rng, cw, ch, "P", 16), noise_pic(rng, cw, ch, "P", 24)]
    r = lambda s: int(rng.integers(-s, s))
    pics.append(dict(kind="B", poc=20, cus=[dict(t="inter", l0=(3, (4 * r(30), 4 * r(30))), l1=(4, (4 * r(30), 4 * r(30)))) for _ in range(n)]))
    pics.append(dict(kind="B", poc=18, cus=[dict(t="inter", l0=(3, (r(90), r(90))), l1=(4, (r(90), r(90)))) for _ in range(n)]))
    return dict(width=w, height=h), pics


def explicit_weights(w, h):
    """Flat references; luma and chroma denominators of their own (0 and 7 included), weights over the whole coded range (2^denominator - 128 ..
    2^denominator + 127), offsets -128 .. 127, Clip1 acting at both ends; entries with the flags off; one list (P) and two (B)."""
    cw, ch = dims(w, h)
    n = cw * ch
    seq = dict(width=w, height=h, weighted_pred=1, weighted_bipred=1)
    pics = [flat_pic(cw, ch, 200, 17, 130), flat_pic(cw, ch, 3, 250, 90, "P", 16), flat_pic(cw, ch, 100, 128, 255, "P", 32)]
    tables = [dict(ld_y=5, ld_c=3, l0=[dict(y=(33, -5), c=((7, 100), (-8, 127))), dict(y=(159, 127), c=((-12, -128), (30, -128))), None]),
              dict(ld_y=0, ld_c=0, l0=[dict(y=(1, -128), c=((2, -100), (1, 1))), dict(y=(-1, 10), c=None), dict(y=(2, 60), c=((-3, 127), (0, 77)))]),
              dict(ld_y=7, ld_c=6, l0=[dict(y=(0, 127), c=((191, 0), (64, -1))), dict(y=None, c=((65, 2), (-64, 120))), dict(y=(255, -128), c=None)]),
              dict(ld_y=1, ld_c=7, l0=[dict(y=(3, -100), c=((0, 5), (255, -127))), dict(y=(-126, 40), c=((127, -3), (1, 0))), dict(y=(129, 0), c=None)])]
    btables = [dict(ld_y=5, ld_c=4, l0=[dict(y=(60, 20), c=((20, -30), (-10, 40))), dict(y=(-20, -10), c=((5, 5), (30, -128)))],
                    l1=[dict(y=(-30, 127), c=((-4, 127), (26, -60))), dict(y=(60, -128), c=((11, -128), (-40, 127)))]),
               dict(ld_y=7, ld_c=0, l0=[None, dict(y=(255, 3), c=((1, 1), (2, 2)))], l1=[dict(y=(0, -90), c=((-1, 0), (3, 7))), dict(y=(100, 9), c=None)])]
    for k, tb in enumerate(btables):
        cus = []
        for a in range(n):
            r0, r1 = a % 2, (a // 2) % 2                              # POC 8 / 24 lie between pictures 0, 1 and 1, 2: both lists hold all three
            cus.append([dict(t="inter", l0=(r0, (0, 4)), l1=(r1 + 1, (8, 0))), dict(t="inter", l0=(r0, (4, 4))), dict(t="inter", l1=(r1 + 1, (0, 0)))][a % 3])
        pics.append(dict(kind="B", poc=8 + 16 * k, cus=cus, wp=tb))
    for k, tb in enumerate(tables):
        pics.append(dict(kind="P", poc=40 + 2 * k, cus=[l0(a % 3, 4 * (a % 5), -4 * (a % 3)) for a in range(n)], is_ref=False, wp=tb))
    return seq, pics


def deblock_identity_flat(w, h):
    """The filter ON (PCM units included: pcm_loop_filter_disabled_flag 0) over flat pictures at slice QP 0, 3 .. 51: every filter of 8.7.2.5.7 maps
    equal samples to themselves.  Intra (PCM) edges have Bs 2, edges between units with different vectors / references Bs 1, skipped units Bs 0."""
    cw, ch = dims(w, h)
    n = cw * ch
    seq = dict(width=w, height=h, deblock=1, pcm_loop_filter_disabled=0)
    pics = [flat_pic(cw, ch, 128, 128, 128), flat_pic(cw, ch, 128, 128, 128, "P", 2, layout="pic")]
    one = flat_pic(cw, ch, 128, 128, 128)["cus"][0]
    for k, qp in enumerate(range(0, 52, 3)):
        cus = [[one, l0(0, 5, -9), l0(1, -40, 22), dict(t="skip"), l0(1, 0, 0)][(a + k) % 5] for a in range(n)]
        pics.append(dict(kind="P", poc=4 + 2 * k, cus=cus, is_ref=False, qp=qp))
    return seq, pics


def deblock_identity_pcm_noise(w, h):
    """The filter ON over all-PCM noise pictures with pcm_loop_filter_disabled_flag 1: the samples of PCM units are not modified (8.7.2.5.7: nDp / nDq
    are 0 for them), at any QP."""
    rng = np.random.default_rng(0xB108)
    cw, ch = dims(w, h)
    seq = dict(width=w, height=h, deblock=1, pcm_loop_filter_disabled=1)
    pics = [noise_pic(rng, cw, ch), noise_pic(rng, cw, ch, "P", 2, layout="pic", qp=40), noise_pic(rng, cw, ch, "P", 4, layout="row", qp=51),
            noise_pic(rng, cw, ch, "P", 6, layout="ctb", qp=30)]
    return seq, pics


def row_and_picture_slices(w, h):
    """One slice per CTB row (a vector per row) and one slice per picture: the many-CTBs-per-slice paths (AMVP with spatial candidates)."""
    rng = np.random.default_rng(0xB109)
    cw, ch = dims(w, h)
    pics = [noise_pic(rng, cw, ch)]
    rows = []
    for y in range(ch):
        rows += [l0(0, int(rng.integers(-100, 100)), int(rng.integers(-100, 100)))] * cw
    pics.append(dict(kind="P", poc=2, cus=rows, layout="row", is_ref=False))
    pics.append(dict(kind="P", poc=4, cus=[l0(0, -13, 27)] * (cw * ch), layout="pic", is_ref=False))
    return dict(width=w, height=h), pics


def full_hd_rows(w=1920, h=1080):
    """1920x1080 (coded 1920x1088): PCM noise, then two P pictures with one slice per CTB row and a vector per row, integer and fractional."""
    rng = np.random.default_rng(0xB110)
    cw, ch = dims(w, h)
    pics = [noise_pic(rng, cw, ch)]
    for k in range(2):
        rows = []
        for y in range(ch):
            mv = (int(rng.integers(-140, 140)), int(rng.integers(-140, 140))) if (y + k) % 2 else (4 * int(rng.integers(-30, 30)), 4 * int(rng.integers(-30, 30)))
            rows += [l0(0, *mv)] * cw
        pics.append(dict(kind="P", poc=2 + 2 * k, cus=rows, layout="row", is_ref=False))
    return dict(width=w, height=h), pics


def one_slice_per_ctb_stream(w, h):
    rng = np.random.default_rng(0xB120 + w)
    cw, ch = dims(w, h)
    pics = [noise_pic(rng, cw, ch),
            dict(kind="P", poc=2, cus=[l0(0, 4 * int(rng.integers(-20, 20)) + a % 4, 4 * int(rng.integers(-20, 20))) for a in range(cw * ch)], is_ref=False)]
    return dict(width=w, height=h), pics


HEVC_CASES = {
    "integer_vectors_noise": integer_vectors_noise,
    "fractional_positions_noise": fractional_positions_noise,
    "fractional_positions_ramps": fractional_positions_ramps,
    "skip_copies": skip_copies,
    "bipred_default": bipred_default,
    "explicit_weights": explicit_weights,
    "deblock_identity_flat": deblock_identity_flat,
    "deblock_identity_pcm_noise": deblock_identity_pcm_noise,
    "row_and_picture_slices": row_and_picture_slices,
}
