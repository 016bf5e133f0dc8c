"""The scripted H.264 known-answer cases: name -> builder(width, height) -> (seq, pics).

Every case is a script for tests/scripted_h264.py; its expected frames come from tests/analytic_expect.py.  All randomness is seeded: two calls give the
same script.  Sizes: 96x80 and 90x70 (cropped from 96x80: the cropped-away samples are still reference samples); the deblock_filters_* cases also 48x288.
"""
import numpy as np

from analytic_expect import ramp

SIZES = [(96, 80), (90, 70)]


def dims(w, h):
    return (w + 15) // 16, (h + 15) // 16


def pcm_from_planes(Y, Cb, Cr, mbw, mbh):
    return [dict(t="pcm", y=Y[y * 16:(y + 1) * 16, x * 16:(x + 1) * 16].copy(), cb=Cb[y * 8:(y + 1) * 8, x * 8:(x + 1) * 8].copy(),
                 cr=Cr[y * 8:(y + 1) * 8, x * 8:(x + 1) * 8].copy()) for y in range(mbh) for x in range(mbw)]


def noise_pic(rng, mbw, mbh, kind="I", poc=0, **kw):
    """A picture of I_PCM macroblocks holding noise (with the byte patterns that need emulation prevention: runs of zeros)."""
    Y = rng.integers(0, 256, (mbh * 16, mbw * 16), dtype=np.uint8)
    Cb = rng.integers(0, 256, (mbh * 8, mbw * 8), dtype=np.uint8)
    Cr = rng.integers(0, 256, (mbh * 8, mbw * 8), dtype=np.uint8)
    Y[3, 0:7] = 0; Y[5, 4:8] = (0, 0, 1, 0); Cb[0, 0:4] = (0, 0, 3, 0); Cr[7, 4:8] = (0, 0, 0, 2)
    return dict(kind=kind, poc=poc, mbs=pcm_from_planes(Y, Cb, Cr, mbw, mbh), **kw)


def flat_pic(mbw, mbh, y, cb, cr, kind="I", poc=0, **kw):
    f = lambda s, v: np.full((s, s), v, np.uint8)
    return dict(kind=kind, poc=poc, mbs=[dict(t="pcm", y=f(16, y), cb=f(8, cb), cr=f(8, cr)) for _ in range(mbw * mbh)], **kw)


def ramp_pic(mbw, mbh, params, kind="I", poc=0, **kw):
    (ya, yc, yd), (ba, bc, bd), (ra, rc, rd) = params
    return dict(kind=kind, poc=poc, mbs=pcm_from_planes(ramp(mbh * 16, mbw * 16, ya, yc, yd), ramp(mbh * 8, mbw * 8, ba, bc, bd),
                                                        ramp(mbh * 8, mbw * 8, ra, rc, rd), mbw, mbh), **kw)


def p_pic(poc, mbs, **kw):
    return dict(kind="P", poc=poc, mbs=mbs, **kw)


def l0(pic, mvx, mvy):
    return dict(t="16x16", l0=(pic, (mvx, mvy)))


# -- 1: integer vectors over noise, clamped coordinates -------------------------------------------------------------------------------------------
def integer_vectors_noise(w, h):
    """Expected: the reference shifted by the vector, every coordinate clamped into the picture.  Vectors reach up to 40 samples outside on every
    side; the last picture's are so far outside that a whole block reads one clamped row / column (or one corner sample)."""
    rng = np.random.default_rng(0xA101)
    mbw, mbh = dims(w, h)
    pics = [noise_pic(rng, mbw, mbh)]
    for k in range(3):
        mbs = []
        for a in range(mbw * mbh):
            x, y = a % mbw, a // mbw
            if k < 2:
                tx, ty = int(rng.integers(-40, mbw * 16 + 40 - 16)), int(rng.integers(-40, mbh * 16 + 40 - 16))       # where the block reads from
                if a % 5 == 0:
                    tx = (-40, mbw * 16 + 24)[(a // 5) & 1]
                if a % 7 == 0:
                    ty = (-40, mbh * 16 + 24)[(a // 7) & 1]
                mv = (4 * (tx - x * 16), 4 * (ty - y * 16))
            else:
                far = [(-200, 0), (200, 0), (0, -200), (0, 200), (-200, -200), (200, 200), (200, -200), (-200, 200), (-200, 3), (5, 200)][a % 10]
                mv = (4 * far[0], 4 * far[1])
            mbs.append(l0(0, *mv))
        pics.append(p_pic(2 + 2 * k, mbs, is_ref=False))
    return dict(width=w, height=h), pics


# -- 2: odd integer luma vectors: chroma at the half-sample position ------------------------------------------------------------------------------
def odd_integer_vectors_chroma_half(w, h):
    """An odd integer luma vector is a chroma vector with the fraction 4/8 in that direction: 8-270 becomes (32 A + 32 B + 32) >> 6 = (A + B + 1) >> 1
    of the two chroma neighbours (four neighbours, (A + B + C + D + 2) >> 2, when both components are odd).  The host test checks that form."""
    rng = np.random.default_rng(0xA102)
    mbw, mbh = dims(w, h)
    pics = [noise_pic(rng, mbw, mbh)]
    mbs = []
    for a in range(mbw * mbh):
        ox, oy = int(rng.integers(-9, 10)), int(rng.integers(-9, 10))
        kind = a % 3
        mvx = 2 * ox + 1 if kind != 1 else 2 * ox
        mvy = 2 * oy + 1 if kind != 0 else 2 * oy
        mbs.append(l0(0, 4 * mvx, 4 * mvy))
    pics.append(p_pic(2, mbs))
    return dict(width=w, height=h), pics


# -- 3 / 5: every fractional position on ramps ----------------------------------------------------------------------------------------------------
RAMP_PARAMS = [((1, 2, 0), (2, 1, 20), (-2, -1, 250)),              # f = a*x + c*y + d per plane (luma, Cb, Cr): inside 0..255 over 96x80 / 48x40
               ((-1, -1, 200), (-2, 2, 120), (1, -2, 100)),
               ((-2, 0, 220), (0, -2, 90), (2, 2, 10))]


def fractional_positions_ramps(w, h):
    """Three ramp references (slopes (1, 2), (-1, -1), (-2, 0) in luma; chroma ramps of their own), then P pictures whose macroblocks walk through the
    16 luma quarter positions and the 64 chroma eighth positions with integer parts within +-3 samples.  Expected: analytic_expect.ramp_luma_closed /
    ramp_chroma_closed where the filter footprint lies inside the picture (at least 80 % of the luma samples: asserted), the literal restatement with
    clamped coordinates elsewhere."""
    rng = np.random.default_rng(0xA103)
    mbw, mbh = dims(w, h)
    pics = [ramp_pic(mbw, mbh, RAMP_PARAMS[0], "I", 0)] + [ramp_pic(mbw, mbh, RAMP_PARAMS[k], "P", 2 * k) for k in (1, 2)]
    n = 0
    for k in range(6):
        mbs = []
        for a in range(mbw * mbh):
            # the low three bits of the luma vector are the chroma eighth fraction, the low two the luma quarter fraction: 64 combinations hold both
            # sets of positions; integer parts -2 .. 0 luma samples, so every vector is within +-3 samples
            mbs.append(l0(k % 3, 8 * int(rng.integers(-1, 1)) + n % 8, 8 * int(rng.integers(-1, 1)) + (n // 8) % 8))
            n += 1
        pics.append(p_pic(6 + 2 * k, mbs, is_ref=False))
    return dict(width=w, height=h, num_ref_frames=3), pics


# -- 4: every fractional position over noise ------------------------------------------------------------------------------------------------------
def fractional_positions_noise(w, h):
    """All 16 luma and all 64 chroma positions over noise, every macroblock a different vector, some far outside the picture.  Expected: the literal
    restatements (luma_literal, 8-270) with clamped coordinates."""
    rng = np.random.default_rng(0xA104)
    mbw, mbh = dims(w, h)
    pics = [noise_pic(rng, mbw, mbh)]
    n = 0
    for k in range(5):
        mbs = []
        for a in range(mbw * mbh):
            x, y = a % mbw, a // mbw
            tx, ty = int(rng.integers(-24, mbw * 16 + 8)), int(rng.integers(-24, mbh * 16 + 8))
            if n % 11 == 0:
                tx, ty = [(-300, ty), (tx, 300), (mbw * 16 + 100, -90)][(n // 11) % 3]
            mv = (8 * ((tx - x * 16) // 2) + n % 8, 8 * ((ty - y * 16) // 2) + (n // 8) % 8)
            mbs.append(l0(0, *mv))
            n += 1
        pics.append(p_pic(2 + 2 * k, mbs, is_ref=False))
    return dict(width=w, height=h), pics


# -- 6: 16x8 and 8x16 partitions, a vector and a reference per partition ----------------------------------------------------------------------------
def partitions_multiref(w, h):
    """Four references: three flat fields of distinct values (a wrong ref_idx shows in every sample) and one noise picture; 16x8 / 8x16 macroblocks
    whose partitions differ in vector and reference, and some that share the reference (the other vector predictor of the second partition)."""
    rng = np.random.default_rng(0xA106)
    mbw, mbh = dims(w, h)
    pics = [flat_pic(mbw, mbh, 40, 60, 200), flat_pic(mbw, mbh, 90, 140, 30, "P", 2), flat_pic(mbw, mbh, 170, 220, 110, "P", 4),
            noise_pic(rng, mbw, mbh, "P", 6)]
    for k in range(2):
        mbs = []
        for a in range(mbw * mbh):
            r0, r1 = int(rng.integers(0, 4)), int(rng.integers(0, 4))
            if a % 4 == 0:
                r1 = r0
            if a % 6 == 1:
                r0, r1 = 3, 3
            mv = lambda: (int(rng.integers(-70, 70)), int(rng.integers(-70, 70)))
            mbs.append(dict(t=("16x8", "8x16")[(a + k) & 1], parts=[(r0, mv()), (r1, mv())]))
        pics.append(p_pic(8 + 2 * k, mbs, is_ref=False))
    return dict(width=w, height=h, num_ref_frames=4), pics


# -- 7: P_Skip ------------------------------------------------------------------------------------------------------------------------------------
def p_skip_copies(w, h):
    """P_Skip with no neighbour available (one slice per macroblock): the vector is (0, 0), the reference RefPicList0[0] (8.4.1.1): a copy.  The second
    P picture mixes skipped macroblocks with moved ones, so that the copy is of the right reference at the right place."""
    rng = np.random.default_rng(0xA107)
    mbw, mbh = dims(w, h)
    pics = [noise_pic(rng, mbw, mbh), p_pic(2, [dict(t="skip") for _ in range(mbw * mbh)])]
    pics.append(p_pic(4, [dict(t="skip") if a % 3 else l0(0, 4 * int(rng.integers(-8, 8)), 4 * int(rng.integers(-8, 8))) for a in range(mbw * mbh)],
                      num_ref=(2, 1)))
    return dict(width=w, height=h, num_ref_frames=2), pics


# -- 8: default bi-prediction ---------------------------------------------------------------------------------------------------------------------
def bipred_default(w, h):
    """Two flat references u, v: (u + v + 1) >> 1 (8-273); two noise references at integer vectors: the rounded mean of the two shifted pictures.
    B_L0 / B_L1 macroblocks between them copy one list."""
    rng = np.random.default_rng(0xA108)
    mbw, mbh = dims(w, h)
    n = mbw * mbh
    seq = dict(width=w, height=h, num_ref_frames=2, profile=77)
    pics = [flat_pic(mbw, mbh, 10, 255, 1), flat_pic(mbw, mbh, 255, 0, 254, "P", 8)]
    bi = lambda a, b: [dict(t="16x16", l0=(a, (0, 0)), l1=(b, (0, 0))) if i % 3 == 0 else
                       (dict(t="16x16", l0=(a, (4, -8))) if i % 3 == 1 else dict(t="16x16", l1=(b, (-12, 4)))) for i in range(n)]
    pics.append(dict(kind="B", poc=4, mbs=bi(0, 1)))
    pics += [noise_pic(rng, mbw, mbh, "P", 16), noise_pic(rng, mbw, mbh, "P", 24)]
    mbs = [dict(t="16x16", l0=(3, (4 * int(rng.integers(-30, 30)), 4 * int(rng.integers(-30, 30)))),
                l1=(4, (4 * int(rng.integers(-30, 30)), 4 * int(rng.integers(-30, 30))))) for _ in range(n)]
    pics.append(dict(kind="B", poc=20, mbs=mbs))
    mbs = [dict(t="16x16", l0=(3, (int(rng.integers(-90, 90)), int(rng.integers(-90, 90)))), l1=(4, (int(rng.integers(-90, 90)), int(rng.integers(-90, 90)))))
           for _ in range(n)]
    pics.append(dict(kind="B", poc=18, mbs=mbs))
    return seq, pics


# -- 9: explicit weights --------------------------------------------------------------------------------------------------------------------------
def explicit_weights_p(w, h):
    """One list.  Flat references, luma and chroma with their own denominators (0 included), weights and offsets across -128..127 chosen so that Clip1
    acts at both ends; entries with the flags off take the weight 2^denominator (7.4.3.2).  8.4.2.3 is typed out in analytic_expect.weighted."""
    mbw, mbh = dims(w, h)
    n = mbw * mbh
    seq = dict(width=w, height=h, num_ref_frames=3, profile=77, weighted_pred=1)
    pics = [flat_pic(mbw, mbh, 200, 17, 130), flat_pic(mbw, mbh, 3, 250, 90, "P", 2), flat_pic(mbw, mbh, 100, 128, 255, "P", 4)]
    tables = [dict(ld_y=5, ld_c=3, l0=[dict(y=(33, -5), c=((7, 100), (-8, 127))), dict(y=(127, 127), c=((-128, -128), (127, -128))), None]),
              dict(ld_y=0, ld_c=0, l0=[dict(y=(1, -128), c=((2, -100), (1, 1))), dict(y=(-1, 10), c=None), dict(y=(2, 60), c=((-3, 127), (0, 77)))]),
              dict(ld_y=7, ld_c=6, l0=[dict(y=(-128, 127), c=((127, 0), (64, -1))), dict(y=None, c=((65, 2), (63, -2))), dict(y=(127, -128), c=None)]),
              dict(ld_y=1, ld_c=7, l0=[dict(y=(3, -100), c=((-1, 5), (127, 127))), dict(y=(2, 0), c=((127, -3), (1, 0))), dict(y=(-128, 0), c=None)])]
    for k, tb in enumerate(tables):
        pics.append(p_pic(6 + 2 * k, [l0(a % 3, 4 * (a % 5), -4 * (a % 3)) for a in range(n)], is_ref=False, wp=tb, num_ref=(3, 1)))
    return seq, pics


def explicit_weights_b(w, h):
    """Two lists (weighted_bipred_idc 1): bi-predicted macroblocks (8-276, w0 + w1 within -128..127 as 8.4.2.3 demands) and single-list ones (8-274)."""
    mbw, mbh = dims(w, h)
    n = mbw * mbh
    seq = dict(width=w, height=h, num_ref_frames=2, profile=77, weighted_bipred=1)
    pics = [flat_pic(mbw, mbh, 220, 30, 128), flat_pic(mbw, mbh, 40, 240, 100, "P", 16)]
    tables = [dict(ld_y=5, ld_c=4, l0=[dict(y=(60, 20), c=((20, -30), (-10, 40))), dict(y=(-20, -10), c=((5, 5), (30, -128)))],
                   l1=[dict(y=(-30, 127), c=((-4, 127), (26, -60))), dict(y=(60, -128), c=((11, -128), (-40, 127)))]),
              dict(ld_y=0, ld_c=1, l0=[dict(y=(2, -7), c=((3, 1), (-2, 9))), dict(y=(1, 0), c=None)],
                   l1=[dict(y=(-1, 8), c=((-1, 0), (4, -90))), None]),
              dict(ld_y=6, ld_c=7, l0=[dict(y=(127, 100), c=((127, 127), (-128, 0))), dict(y=None, c=((-30, 4), (0, -4)))],
                   l1=[dict(y=(-128, -128), c=((-98, -128), (127, 5))), dict(y=(1, 1), c=((0, -1), (0, 3)))]),
              # denominator 7 with the flags off: the inferred weight is 128, which no coded weight can be
              dict(ld_y=7, ld_c=7, l0=[None, dict(y=(-100, 3), c=((1, 1), (2, 2)))],
                   l1=[dict(y=(-1, 0), c=((-128, 0), (-3, 7))), dict(y=(-28, 9), c=((-1, -1), (-2, -2)))])]
    for k, tb in enumerate(tables):
        mbs = []
        for a in range(n):
            r0, r1 = a % 2, (a // 2) % 2
            mbs.append([dict(t="16x16", l0=(r0, (0, 4)), l1=(r1, (8, 0))), dict(t="16x16", l0=(r0, (4, 4))), dict(t="16x16", l1=(r1, (0, 0)))][a % 3])
        pics.append(dict(kind="B", poc=4 + 2 * k, mbs=mbs, wp=tb, num_ref=(2, 2)))
    return seq, pics


# -- 10: implicit weights -------------------------------------------------------------------------------------------------------------------------
def implicit_weights_b(w, h):
    """weighted_bipred_idc 2 (8.4.2.3.1, typed out in analytic_expect.implicit_weights).  References at POC 0 and 16; B pictures at POC 4 (w1 = 16),
    8 (32), 12 (48) between them; at POC 20 and 60 behind both (both lists hold both pictures: the pairs (16, 0) extrapolate -- POC 20: w1 = -16, inside;
    POC 60: w1 = -176 -> the 32 / 32 fallback -- and (0, 16): POC 20: 80; POC 60: 240 -> fallback), and pairs of one picture with itself (equal order
    counts: 32 / 32).  Single-list macroblocks are not weighted."""
    mbw, mbh = dims(w, h)
    n = mbw * mbh
    seq = dict(width=w, height=h, num_ref_frames=2, profile=77, weighted_bipred=2)
    pics = [flat_pic(mbw, mbh, 250, 4, 128), flat_pic(mbw, mbh, 20, 200, 60, "P", 16)]
    for poc in (4, 8, 12, 20, 60):
        mbs = []
        for a in range(n):
            pair = [(0, 1), (1, 0), (0, 0), (1, 1)][a % 4] if poc < 16 else [(1, 0), (0, 1), (1, 1), (0, 0)][a % 4]
            mbs.append(dict(t="16x16", l0=(pair[0], (4 * (a % 3), 0)), l1=(pair[1], (0, -4 * (a % 2)))) if a % 5 else dict(t="16x16", l0=(pair[0], (0, 0))))
        pics.append(dict(kind="B", poc=poc, mbs=mbs, num_ref=(2, 2)))
    return seq, pics


# -- 11: Intra16x16 and chroma prediction without residual ----------------------------------------------------------------------------------------
def intra16_beside_pcm(w, h):
    """One slice per picture.  I_PCM macroblocks hold noise or ramps; Intra16x16 macroblocks beside them carry no coefficients, so they ARE their
    prediction: vertical / horizontal = a copy of the neighbouring row / column, DC = (sum + 16) >> 5 with both neighbours, (sum + 8) >> 4 with one,
    128 with none (the first macroblock of the second picture), plane = the ramp continued (8.3.3.4 on f = a x + c y + d in macroblock coordinates:
    H = sum (x'+1) a (2 x' + 2) = 408 a, b = (5 * 408 a + 32) >> 6 = 32 a for |a| <= 4, likewise c; a' = 16 (f(-1, 15) + f(15, -1)) = 32 (7 a + 7 c + d), so
    the prediction (a' + b (x - 7) + c (y - 7) + 16) >> 5 is a x + c y + d; chroma 8.3.4.4: H = 60 a, b = (34 * 60 a + 32) >> 6 = 32 a, the same).  The
    host test checks the plane form; the expectation here is 8.3.3 / 8.3.4 typed out."""
    rng = np.random.default_rng(0xA111)
    mbw, mbh = dims(w, h)
    pics = []
    # picture 0: noise I_PCM on a checkerboard, the four luma modes x four chroma modes between them (modes limited by what is available)
    base = noise_pic(rng, mbw, mbh)
    mbs = []
    n = 0
    for a in range(mbw * mbh):
        x, y = a % mbw, a // mbw
        if (x + y) % 2 == 0 or a == 0:
            mbs.append(base["mbs"][a])
            continue
        ok_l = [m for m in (0, 1, 2, 3) if (m != 0 or y > 0) and (m != 1 or x > 0) and (m != 3 or (x > 0 and y > 0))]
        ok_c = [m for m in (0, 1, 2, 3) if (m != 2 or y > 0) and (m != 1 or x > 0) and (m != 3 or (x > 0 and y > 0))]
        mbs.append(dict(t="i16", mode=ok_l[n % len(ok_l)], cmode=ok_c[(n // 4) % len(ok_c)]))
        n += 1
    pics.append(dict(kind="I", poc=0, mbs=mbs))
    # picture 1: starts with an Intra16x16 DC macroblock without neighbours (128), then chains of predicted macroblocks (prediction from prediction)
    mbs = []
    for a in range(mbw * mbh):
        x, y = a % mbw, a // mbw
        if a == 0:
            mbs.append(dict(t="i16", mode=2, cmode=0))
        elif y == 0:
            mbs.append(dict(t="i16", mode=(1, 2)[x % 2], cmode=(0, 1)[x % 2]) if x != 3 else base["mbs"][a])
        elif x == 0:
            mbs.append(dict(t="i16", mode=(0, 2)[y % 2], cmode=(0, 2)[y % 2]))
        else:
            mbs.append(base["mbs"][a] if (x * 3 + y) % 4 == 0 else dict(t="i16", mode=(x + y) % 4, cmode=(x + 2 * y) % 4))
    pics.append(dict(kind="P", poc=2, mbs=mbs, layout="pic"))
    # picture 2: ramps in I_PCM along the top row and the left column, plane prediction everywhere else: the ramp continues over the whole picture
    ya, yc, yd = 1, 1, 20
    Y = ramp(mbh * 16, mbw * 16, ya, yc, yd); Cb = ramp(mbh * 8, mbw * 8, 2, -1, 60); Cr = ramp(mbh * 8, mbw * 8, -3, 2, 160)
    rp = pcm_from_planes(Y, Cb, Cr, mbw, mbh)
    pics.append(dict(kind="P", poc=4, layout="pic", mbs=[rp[a] if a % mbw == 0 or a < mbw else dict(t="i16", mode=3, cmode=3) for a in range(mbw * mbh)]))
    return dict(width=w, height=h), pics


# -- 12: deblocking on, all I_PCM noise -----------------------------------------------------------------------------------------------------------
def deblock_identity_pcm_noise(w, h):
    """The filter is ON, every macroblock is I_PCM (qP = 0, 8.7.2.2): indexA = 0 + FilterOffsetA.  alpha(indexA) is 0 up to indexA 15 (Table 8-16),
    so filterSamplesFlag is never set: identity, with offset 0 and with slice_alpha_c0_offset_div2 = +6 (indexA 12); beta offset +6 likewise."""
    rng = np.random.default_rng(0xA112)
    mbw, mbh = dims(w, h)
    pics = [noise_pic(rng, mbw, mbh, deblock=(0, 0, 0)), noise_pic(rng, mbw, mbh, "P", 2, layout="pic", deblock=(0, 6, 6)),
            noise_pic(rng, mbw, mbh, "P", 4, layout="row", deblock=(2, 6, 0)), noise_pic(rng, mbw, mbh, "P", 6, layout="mb", deblock=(0, 6, -6))]
    return dict(width=w, height=h), pics


# -- 13: deblocking on, flat fields, every QP -----------------------------------------------------------------------------------------------------
def deblock_identity_flat_all_qp(w, h):
    """Flat pictures stay flat whatever the filter decides (every filter of 8.7.2.3 / 8.7.2.4 maps equal samples to themselves: the deltas are
    differences).  Slice QP 0, 3, .. 51: intra edges (Intra16x16 DC without neighbours = 128: bS 3 inside, 4 at macroblock edges), inter edges between
    different vectors and references (bS 1; both references are flat 128), disable_deblocking_filter_idc 0 and 2 alternating."""
    mbw, mbh = dims(w, h)
    pics = [flat_pic(mbw, mbh, 128, 128, 128, deblock=(0, 0, 0)), flat_pic(mbw, mbh, 128, 128, 128, "P", 2, deblock=(0, 0, 0), layout="pic")]
    for k, qp in enumerate(range(0, 52, 3)):
        mbs = []
        for a in range(mbw * mbh):
            c = (a + k) % 5
            mbs.append([dict(t="i16", mode=2, cmode=0), l0(0, 5, -9), l0(1, -40, 22), dict(t="16x8", parts=[(0, (3, 3)), (1, (-16, 8))]),
                        dict(t="8x16", parts=[(1, (0, 0)), (1, (17, 0))])][c])
        pics.append(p_pic(4 + 2 * k, mbs, is_ref=False, qp=qp, deblock=((0, 2)[k & 1], (0, 3, -3)[k % 3], (0, -2, 2)[k % 3]), num_ref=(2, 1)))
    return dict(width=w, height=h, num_ref_frames=2), pics


# -- 14: deblocking on, noise P pictures at low QP ------------------------------------------------------------------------------------------------
def deblock_identity_noise_low_qp(w, h):
    """P pictures over noise with slice QP <= 15 and offsets 0: indexA = qPav <= 15 -> alpha 0 -> no sample is filtered, although the edges between
    macroblocks with different vectors have bS 1 (and bS > 0 against the I_PCM macroblocks in between): the low end of the threshold lookup."""
    rng = np.random.default_rng(0xA114)
    mbw, mbh = dims(w, h)
    base = noise_pic(rng, mbw, mbh, deblock=(0, 0, 0))
    pics = [base]
    for k, qp in enumerate((0, 7, 12, 15)):
        mbs = [base["mbs"][a] if (a + k) % 7 == 0 else l0(0, int(rng.integers(-60, 60)), int(rng.integers(-60, 60))) for a in range(mbw * mbh)]
        pics.append(p_pic(2 + 2 * k, mbs, is_ref=False, qp=qp, deblock=((0, 2)[k & 1], 0, 0)))
    return dict(width=w, height=h), pics


# -- the second layout: many macroblocks per slice ------------------------------------------------------------------------------------------------
def row_and_picture_slices(w, h):
    """One slice per macroblock row (a vector per row) and one slice per picture (one vector): the many-macroblocks-per-slice paths.  Every macroblock
    of a slice repeats one vector, so the predictor is that vector whichever branch of 8.4.1.3 applies; mvd is 0 after the slice's first."""
    rng = np.random.default_rng(0xA115)
    mbw, mbh = dims(w, h)
    pics = [noise_pic(rng, mbw, mbh)]
    rows = []
    for y in range(mbh):
        rows += [l0(0, int(rng.integers(-100, 100)), int(rng.integers(-100, 100)))] * mbw
    pics.append(p_pic(2, rows, layout="row", is_ref=False))
    pics.append(p_pic(4, [l0(0, -13, 27)] * (mbw * mbh), layout="pic", is_ref=False))
    return dict(width=w, height=h), pics


H264_CASES = {
    "integer_vectors_noise": integer_vectors_noise,
    "odd_integer_vectors_chroma_half": odd_integer_vectors_chroma_half,
    "fractional_positions_ramps": fractional_positions_ramps,
    "fractional_positions_noise": fractional_positions_noise,
    "partitions_multiref": partitions_multiref,
    "p_skip_copies": p_skip_copies,
    "bipred_default": bipred_default,
    "explicit_weights_p": explicit_weights_p,
    "explicit_weights_b": explicit_weights_b,
    "implicit_weights_b": implicit_weights_b,
    "intra16_beside_pcm": intra16_beside_pcm,
    "deblock_identity_pcm_noise": deblock_identity_pcm_noise,
    "deblock_identity_flat_all_qp": deblock_identity_flat_all_qp,
    "deblock_identity_noise_low_qp": deblock_identity_noise_low_qp,
    "row_and_picture_slices": row_and_picture_slices,
}
# the inter cases that also run through chain launches on the GPU
H264_INTER_CASES = ["integer_vectors_noise", "fractional_positions_ramps", "fractional_positions_noise", "partitions_multiref", "p_skip_copies",
                    "bipred_default", "explicit_weights_p", "explicit_weights_b", "implicit_weights_b", "deblock_identity_noise_low_qp",
                    "row_and_picture_slices"]


def with_filter_on(pics, qp=12):
    """The same script with the deblocking filter ON in every picture at a slice QP of 12 and offsets 0.  indexA = qPav + 0 <= 15 for every edge (I_PCM
    macroblocks count qP 0), alpha(indexA) = 0 (Table 8-16), so no edge is filtered and the expected pictures are those of the script as it was -- but
    the decoder now runs its deblocking stage (and, on the GPU, may run the pictures inside chain launches, which need that stage)."""
    return [dict(p, deblock=(0, 0, 0), qp=qp) for p in pics]


# -- deblocking where it filters ------------------------------------------------------------------------------------------------------------------
# Content on which the filters fire: smooth, not noise -- a level per macroblock and plane that steps from neighbour to neighbour by amounts spread
# below and above alpha (Table 8-16: 4 .. 255), plus seeded noise whose amplitude is chosen per picture from 1, 4, 12, 40, so that ap / aq (and the
# |p1 - p0| / |q1 - q0| tests) fall on both sides of beta (2 .. 18).  Levels visit 0 and 255, where Clip1 acts.  tests/deblock_ref.py computes what the
# filter does; tests/test_analytic_host.py asserts from its counters that every path of 8.7.2 was taken, vertically and horizontally.
SIZES_FILTER = SIZES + [(48, 288)]          # 3 x 18 macroblocks: rows 16, 17 lie in the second deblocking band of the band kernels
STEPS = [1, 2, 3, 4, 6, 9, 13, 18, 25, 35, 50, 70, 100]
AMPS = [4, 12, 1, 40]


def stepped_planes(rng, mbw, mbh, amp):
    out = []
    for s in (16, 8, 8):
        lv = np.zeros((mbh, mbw), np.int64)
        for y in range(mbh):
            for x in range(mbw):
                prev = int(lv[y, x - 1]) if x else (int(lv[y - 1, 0]) if y else int(rng.integers(60, 200)))
                v = prev + int(rng.choice(STEPS)) * int(rng.choice([-1, 1]))
                if v < 0 or v > 255:
                    v = 2 * prev - v                                # step the other way instead
                lv[y, x] = min(255, max(0, v)) if rng.integers(0, 5) else int(rng.choice([0, 1, 254, 255]))
                if (y * mbw + x) % 5 == 2:
                    lv[y, x] = (0, 255)[((y * mbw + x) // 5) & 1]        # both ends in every picture, whatever the seed
        up = np.kron(lv, np.ones((s, s), np.int64))
        # At the two ends of the range a texture of period 4 takes the place of the noise: 0 7 1 0 along x and along y (255 - that at the top end).  Across
        # an edge at a multiple of 4 it reads p2 p1 p0 | q0 q1 q2 = 7 1 0 | 0 7 1: ((q0 - p0) << 2) + (p1 - q1) + 4 = -2, delta = -1, and p0 + delta = -1 is
        # what Clip1 is for (beta > 7 provided; 8.7.2.3); the mirror image gives 256.  An inter macroblock with an integer vector carries it to its edges.
        tex = np.maximum.outer(np.array([0, 7, 1, 0])[np.arange(mbh * s) % 4], np.array([0, 7, 1, 0])[np.arange(mbw * s) % 4])
        pl = np.where(up < 2, tex, np.where(up > 253, 255 - tex, up + rng.integers(-amp, amp + 1, up.shape)))
        out.append(np.clip(pl, 0, 255).astype(np.uint8))
    return out


def stepped_pcm(rng, mbw, mbh, amp):
    return pcm_from_planes(*stepped_planes(rng, mbw, mbh, amp), mbw, mbh)


def dqp_to(pred, target):
    """mb_qp_delta that takes QPY,PRED to target (7.4.5: (pred + delta + 52) % 52, delta in -26 .. 25): through the wrap where the straight way is too far"""
    d = target - pred
    return d - 52 if d > 25 else (d + 52 if d < -26 else d)


def intra_filter_pic(rng, mbw, mbh, kind, poc, layout, deblock, amp, qp, k, walk=(16, 36)):
    """Intra16x16 macroblocks (the modes their neighbours allow; mb_qp_delta walks QPY through 16 .. 51) beside I_PCM ones (qPp 0 in the filter)."""
    pcm = stepped_pcm(rng, mbw, mbh, amp)
    step = {"row": mbw, "pic": mbw * mbh}[layout]
    mbs, n, pred = [], k, qp
    for a in range(mbw * mbh):
        x, y = a % mbw, a // mbw
        if a % step == 0:
            pred = qp
        al, at = x > 0 and a - 1 >= a - a % step, y > 0 and a - mbw >= a - a % step
        if (x + 2 * y + k) % 3 == 0:
            mbs.append(pcm[a])                                      # (QPY,PRED passes through an I_PCM macroblock unchanged)
            continue
        ok_l = [m for m in (2, 0, 1, 3) if (m != 0 or at) and (m != 1 or al) and (m != 3 or (al and at))]
        ok_c = [m for m in (0, 2, 1, 3) if (m != 2 or at) and (m != 1 or al) and (m != 3 or (al and at))]
        target = walk[0] + (n * 7) % walk[1]
        mbs.append(dict(t="i16", mode=ok_l[n % len(ok_l)], cmode=ok_c[(n // 2) % len(ok_c)], dqp=dqp_to(pred, target)))
        pred = target
        n += 1
    return dict(kind=kind, poc=poc, layout=layout, deblock=deblock, qp=qp, mbs=mbs)


def deblock_filters_intra(w, h):
    """I and P pictures of Intra16x16 macroblocks (bS 3 inside, 4 at macroblock edges) beside I_PCM; one slice per picture and one per row; offsets that
    clip indexA / indexB at 51 (+12 at QP above 39) and at 0 (-12 between two I_PCM macroblocks); disable_deblocking_filter_idc 0 and 2."""
    rng = np.random.default_rng(0xA201)
    mbw, mbh = dims(w, h)
    spec = [("I", "pic", (0, 0, 0), 26, 4), ("P", "pic", (0, 6, 6), 40, 40), ("P", "row", (0, -3, 3), 30, 1), ("P", "row", (0, 3, -2), 51, 4),
            ("P", "pic", (2, 1, 2), 20, 12)]
    # (with a slice per row only DC and horizontal prediction remain, and idc 2 filters no horizontal macroblock edge there; the QPs of those two pictures
    # stay in 40 .. 51 so that what is left still changes most macroblocks; indexA / indexB below 0 come from the inner edges of their I_PCM macroblocks)
    pics = [intra_filter_pic(rng, mbw, mbh, kind, 2 * k, layout, db, amp, qp, k, (40, 12) if layout == "row" else (16, 36))
            for k, (kind, layout, db, qp, amp) in enumerate(spec)]
    return dict(width=w, height=h, chroma_qp_off=-3), pics


def mb_slice_fields(x, y, k):
    """QP and deblocking fields of a one-macroblock slice: left, top and own QP all different (the three edge classes get different alpha / beta), idc 0,
    1 and 2 mixed, offsets that differ across most edges"""
    return dict(qp=16 + (7 * x + 13 * y + 5 * k) % 36, deblock=((0, 0, 2, 0, 1, 0, 0)[(x + 3 * y + k) % 7], (-3, 0, 2, 6)[(x + y) % 4], (0, -2, 3, 6)[(2 * x + y + k) % 4]))


def deblock_filters_inter(w, h):
    """One slice per macroblock.  16x16 macroblocks whose vectors differ from their neighbours' by exactly 3 or exactly 4 in one component (bS 0 / bS 1),
    different reference pictures (bS 1), 16x8 / 8x16 with halves that differ (inner edges), I_PCM and Intra16x16 macroblocks in between (bS 4 / 3)."""
    rng = np.random.default_rng(0xA202)
    mbw, mbh = dims(w, h)
    pics = [intra_filter_pic(rng, mbw, mbh, "I", 0, "pic", (0, 6, 6), 4, 44, 0), intra_filter_pic(rng, mbw, mbh, "P", 2, "pic", (0, 3, 3), 12, 40, 1)]
    incx, incy = [3, 4, 0, 4, 3, 12], [4, 3, 3, 0, 4, 8]
    for k in range(3):
        pcm = stepped_pcm(rng, mbw, mbh, AMPS[(k + 2) % 4])
        mbs = []
        for a in range(mbw * mbh):
            x, y = a % mbw, a // mbw
            mv = (-20 + 8 * k + sum(incx[i % 6] for i in range(x)), 10 - 4 * k + sum(incy[(i + k) % 6] for i in range(y)))
            t = (x + 3 * y + k) % 8
            ref = int((x // 2 + y + k) % 3 == 0)
            if t == 0:
                m = dict(pcm[a])
            elif t == 1:
                m = dict(t="i16", mode=2, cmode=0)
            elif t in (2, 3):
                second = [(ref, (mv[0] + 4, mv[1])), (1 - ref, mv), (ref, (mv[0], mv[1] - 3)), (ref, (mv[0] - 3, mv[1] + 4))][(a + k) % 4]
                m = dict(t=("16x8", "8x16")[t - 2], parts=[(ref, mv), second])
            else:
                m = l0(ref, *mv)
            m.update(mb_slice_fields(x, y, k))
            if (x > 0 and (x - 1 + 3 * y + k) % 8 == 0) or (y > 0 and (x + 3 * (y - 1) + k) % 8 == 0):
                m["qp"] = 51                                        # beside or below an I_PCM macroblock (QPY 0): the widest qPav there is
            mbs.append(m)
        pics.append(p_pic(4 + 2 * k, mbs, is_ref=False, num_ref=(2, 1)))
    return dict(width=w, height=h, num_ref_frames=2, chroma_qp_off=4), pics


def deblock_filters_b(w, h):
    """B pictures of 16x16 macroblocks: L0-only, L1-only and bi-predicted neighbours; pairs of (picture, vector) that are equal crosswise (bS 0), equal in
    pictures but not in vectors, and both vectors on ONE picture (which is in both lists) -- 8.7.2.1 compares reference pictures, not indices or lists."""
    rng = np.random.default_rng(0xA203)
    mbw, mbh = dims(w, h)
    seq = dict(width=w, height=h, num_ref_frames=2, profile=77, chroma_qp_off=-2)
    pics = [intra_filter_pic(rng, mbw, mbh, "I", 0, "pic", (0, 6, 6), 4, 44, 2), intra_filter_pic(rng, mbw, mbh, "P", 8, "pic", (0, 4, 2), 12, 40, 3)]
    A, B = (12, -8), (-16, 20)
    for k, poc in enumerate((4, 12, 6)):
        mbs = []
        for a in range(mbw * mbh):
            x, y = a % mbw, a // mbw
            A2, B2 = (A[0] + 3 + (y & 1), A[1]), (B[0], B[1] - 4 + (x & 1))
            m = [dict(t="16x16", l0=(0, A)), dict(t="16x16", l1=(1, B)), dict(t="16x16", l0=(0, A), l1=(1, B)), dict(t="16x16", l0=(1, B), l1=(0, A)),
                 dict(t="16x16", l0=(0, A2), l1=(1, B)), dict(t="16x16", l0=(0, A), l1=(0, B)), dict(t="16x16", l0=(0, B2), l1=(0, A)),
                 dict(t="16x16", l0=(1, B), l1=(1, B2)), dict(t="16x16", l0=(0, A), l1=(1, B))][(x + 4 * y + k) % 9]
            m.update(mb_slice_fields(x, y, k))
            mbs.append(m)
        pics.append(dict(kind="B", poc=poc, mbs=mbs, num_ref=(2, 2)))
    return seq, pics


def deblock_filters_coeff(w, h):
    """P macroblocks with ONE coded coefficient (the DC of one 4x4 luma block, +-1): bS 2 on that block's edges -- inner 4x4 edges and macroblock edges,
    from the p side and from the q side -- beside neighbours with bS 1 (vector or reference differs) and bS 0."""
    rng = np.random.default_rng(0xA204)
    mbw, mbh = dims(w, h)
    pics = [intra_filter_pic(rng, mbw, mbh, "I", 0, "pic", (0, 6, 6), 4, 44, 4)]
    for k in range(3):
        mbs = []
        for a in range(mbw * mbh):
            x, y = a % mbw, a // mbw
            mv = (4 * (k - 1) + (4, 0, 0, 3)[(x + y) % 4], -16 + (0, 0, 4, 0, 3)[(x + 2 * y) % 5])
            t = (2 * x + y + k) % 5
            m = l0(0, *mv) if t < 3 else dict(t=("16x8", "8x16")[t - 3], parts=[(0, mv), (0, (mv[0], mv[1] + (4 if a % 2 else 0)))])
            if (x + y + k) % 3 != 2:
                m["resid"] = ((0, 5, 10, 15, 3, 12, 6, 9)[(a + 3 * k) % 8], (1, -1)[(a + k) & 1])
            m.update(mb_slice_fields(x, y, k))
            m["deblock"] = (0,) + m["deblock"][1:]
            mbs.append(m)
        pics.append(p_pic(2 + 2 * k, mbs, is_ref=False))
    return dict(width=w, height=h), pics


def deblock_filters_refs(w, h):
    """An intra picture, then four P pictures in a row, each the reference of the next, vectors up to +-24 samples, filtering at every edge: every
    expected picture depends on the previous one having been filtered BEFORE it was read (asserted in the host test).  A decoder that lets the
    reconstruction of picture n + 1 read a reference window before the deblocking of picture n has made it final fails here, and nowhere before."""
    rng = np.random.default_rng(0xA205)
    mbw, mbh = dims(w, h)
    pics = [intra_filter_pic(rng, mbw, mbh, "I", 0, "pic", (0, 6, 6), 12, 44, 1)]
    for k in range(4):
        mbs = []
        for a in range(mbw * mbh):
            x, y = a % mbw, a // mbw
            m = l0(k, 4 * int(rng.integers(-24, 25)) + int(rng.integers(0, 4)), 4 * int(rng.integers(-24, 25)) + int(rng.integers(0, 4)))
            m.update(qp=28 + (5 * x + 11 * y + 3 * k) % 24, deblock=(0, (0, 2, 4)[(x + k) % 3], (0, 3)[(y + k) % 2]))
            mbs.append(m)
        pics.append(p_pic(2 + 2 * k, mbs))
    return dict(width=w, height=h), pics


# the cases on which the deblocking filter changes samples; they also run at 48x288 (case_sizes) and, as scripted, through chain launches on the GPU
H264_FILTER_CASES = ["deblock_filters_intra", "deblock_filters_inter", "deblock_filters_b", "deblock_filters_coeff", "deblock_filters_refs"]
H264_CASES.update({n: globals()[n] for n in H264_FILTER_CASES})


def case_sizes(name):
    return SIZES_FILTER if name in H264_FILTER_CASES else SIZES


def tall_filter_script(w=16, h=8208):
    """1 x 513 macroblocks: taller than the 512 rows of the banded kernels, so the GPU decoder takes its spin-wait kernels (k_deblock, and k_recon_intra
    for the Intra16x16 macroblocks).  Two pictures in the manner of deblock_filters_intra, then two P pictures of one slice each: runs of 16x16
    macroblocks with the picture's one vector between Intra16x16 and I_PCM ones (bS 4 at their edges, 3 inside), each predicted from the picture
    before -- filtered.  One slice per picture: 513 slices would be beyond the 255 a picture may have."""
    rng = np.random.default_rng(0xA206)
    mbw, mbh = dims(w, h)
    pics = [intra_filter_pic(rng, mbw, mbh, "I", 0, "pic", (0, 6, 6), 4, 40, 0), intra_filter_pic(rng, mbw, mbh, "P", 2, "pic", (0, 2, 3), 12, 30, 1)]
    for k in (2, 3):
        base = intra_filter_pic(rng, mbw, mbh, "P", 2 * k, "pic", (0, (4, -1)[k - 2], (3, 5)[k - 2]), (4, 1)[k - 2], 34 + 6 * (k - 2), k)
        mv = l0(k - 1, (6, -9)[k - 2], (-37, 50)[k - 2])
        pred, mbs = base["qp"], []
        for a, m in enumerate(base["mbs"]):
            if a % 5 in (1, 2, 3) or a == 0:
                mbs.append(mv)                                      # (no mb_qp_delta: QPY,PRED passes through)
            elif m["t"] == "i16":
                target = 20 + (a * 5) % 32
                mbs.append(dict(m, mode=(2, 0)[a & 1] if mbs[a - 1] is not None else 2, dqp=dqp_to(pred, target)))
                pred = target
            else:
                mbs.append(m)
        pics.append(dict(base, mbs=mbs))
    return dict(width=w, height=h, chroma_qp_off=2), pics


def too_tall_stream(rows=1058):
    """A frame of `rows` macroblock rows in a stream with frame_mbs_only_flag = 0 (the only way past the 1024 map-unit rows of the parser)."""
    seq = dict(width=16, height=16 * rows, frame_mbs_only=0)
    return seq, [dict(kind="I", poc=0, layout="pic", mbs=[dict(t="i16", mode=2, cmode=0) for _ in range(rows)])]


def full_hd_rows(w=1920, h=1080):
    """1920x1080 (coded 1920x1088): an I_PCM noise picture, then two P pictures with one slice per macroblock row and one vector per row -- integer and
    fractional, some reaching outside the picture."""
    rng = np.random.default_rng(0xA116)
    mbw, mbh = dims(w, h)
    pics = [noise_pic(rng, mbw, mbh)]
    for k in range(2):
        rows = []
        for y in range(mbh):
            mv = (int(rng.integers(-140, 140)), int(rng.integers(-140, 140))) if (y + k) % 2 else (4 * int(rng.integers(-30, 30)), 4 * int(rng.integers(-30, 30)))
            rows += [l0(0, *mv)] * mbw
        pics.append(p_pic(2 + 2 * k, rows, layout="row", is_ref=False))
    return dict(width=w, height=h), pics
