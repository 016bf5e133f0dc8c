"""Scripted H.264 cases for intra prediction (8.3.1, 8.3.2) and residual reconstruction (8.5): name -> builder(width, height) -> (seq, pics).

Every case is a script for tests/scripted_h264.py; its expected pictures come from tests/analytic_expect.py with tests/h264_recon_ref.py.  All randomness is
seeded.  Neighbour texture comes from I_PCM macroblocks holding noise and from inter macroblocks copied out of a noise picture.  The levels are random
but CONFORMING: ``fit`` shrinks a macroblock's levels until the restatement's 16-bit assertion (8.5.12) holds -- a property of the stream, not of any
decoder.  ``scripted(name)`` also returns what a case exercised (the restatement's and the writer's counters); tests/test_h264_recon_host.py asserts from
them, and from the scripts, that each case covers what it is there for.
"""
import functools

import numpy as np

import analytic_cases as ac
import analytic_expect as ae
import h264_recon_ref as rr
import scripted_h264 as sw
from spec_tables_h264 import ZIGZAG_4x4

SIZE = (96, 80)
SIZES_INTRA = [(96, 80), (48, 288), (16, 48)]                       # 6 x 5; 18 macroblock rows: two bands of 16; one macroblock wide


def amp_for(qp, target=40):
    """a level that moves the samples by about `target`: r ~ level * 16 * 13 * 2^(qP / 6) / 1024"""
    return max(1, int(target / (0.2 * 2 ** (qp / 6))))


def sparse(rng, n, amp, nnz, first=0):
    v = [0] * n
    for i in rng.choice(np.arange(first, n), size=min(int(nnz), n - first), replace=False):
        v[int(i)] = int(rng.integers(1, amp + 1)) * (1 if rng.integers(2) else -1)
    return v


def level_lists(c):
    out = list(c.get("y", {}).values()) + list(c.get("y8", {}).values()) + list(c.get("cac", {}).values()) + list(c.get("cdc", ()))
    return out + ([c["ydc"]] if "ydc" in c else [])


def fit(seq, m, qp):
    """Shrinks the levels of m until every block is inside the 16-bit range of 8.5.12 (halves them; once all are +-1, drops the last one)."""
    for _ in range(64):
        try:
            rr.mb_residual(seq, m, qp)
            return m
        except AssertionError:
            lists = level_lists(m["coef"])
            if any(abs(v) > 1 for lv in lists for v in lv):
                for lv in lists:
                    lv[:] = [int(v / 2) for v in lv]
            else:
                lv = [lv for lv in lists if any(lv)][-1]
                lv[max(i for i, v in enumerate(lv) if v)] = 0
    raise AssertionError("no conforming levels found")


class Rota:
    """picks, among the allowed values, the one used least so far under a key: coverage by construction, not by luck"""
    def __init__(self):
        self.n = {}

    def pick(self, key, allowed):
        c = self.n.setdefault(key, {})
        v = min(allowed, key=lambda q: (c.get(q, 0), q))
        c[v] = c.get(v, 0) + 1
        return v


def allowed_modes(pat):
    return [mode for mode in range(9) if all(ch in pat for ch in rr.NEEDS[mode])]


def mb_pattern(avail):
    return "T" * avail(0, -1) + "L" * avail(-1, 0) + "C" * avail(-1, -1)


def chroma_coef(rng, qp, target=40, dc=True, ac=True):
    amp = amp_for(min(qp, 39), target)
    c = {}
    if dc:
        c["cdc"] = (sparse(rng, 4, amp, rng.integers(1, 5)), sparse(rng, 4, amp, rng.integers(1, 5)))
    if ac:
        c["cac"] = {(pl, blk): sparse(rng, 15, amp, rng.integers(1, 4)) for pl in (0, 1) for blk in range(4) if rng.integers(3)}
        c["cac"][(int(rng.integers(2)), int(rng.integers(4)))] = sparse(rng, 15, amp, 2)
    return c


def pcm_noise(rng):
    return dict(t="pcm", y=rng.integers(0, 256, (16, 16), dtype=np.uint8), cb=rng.integers(0, 256, (8, 8), dtype=np.uint8),
                cr=rng.integers(0, 256, (8, 8), dtype=np.uint8))


def make_nxn(rng, rota, seq, p, a, qp, t, target=40, chroma=True, modes=None):
    """an Intra4x4 / Intra8x8 macroblock at address a of p (whose earlier macroblocks exist): modes in rotation among those the block's neighbours
    allow, levels in every block"""
    avail = rr.mb_avail(seq, p, a)
    N, n = (4, 16) if t == "i4" else (8, 4)
    if modes is None:
        modes = []
        for idx in range(n):
            bx, by = rr.blk_xy(idx) if N == 4 else ((idx & 1) * 8, (idx >> 1) * 8)
            modes.append(rota.pick((N, idx), allowed_modes(rr.pattern(bx, by, N, idx, avail))))
    pat = mb_pattern(avail)
    cmode = rota.pick("cmode", [q for q, need in ((0, ""), (1, "L"), (2, "T"), (3, "TLC")) if all(ch in pat for ch in need)])
    amp = amp_for(qp, target)
    c = chroma_coef(rng, qp, target) if chroma else {}
    if N == 4:
        c["y"] = {k: sparse(rng, 16, amp, rng.integers(1, 5)) for k in range(16)}
    else:
        c["y8"] = {k: sparse(rng, 64, amp, rng.integers(1, 9)) for k in range(4)}
    return fit(seq, dict(t=t, modes=modes, cmode=cmode, coef=c), qp)


def make_i16(rng, rota, seq, p, a, qp, variant="both", target=40, chroma="both"):
    """an Intra16x16 macroblock: variant / chroma = "dc" | "ac" | "both" | "none" say which levels it carries"""
    pat = mb_pattern(rr.mb_avail(seq, p, a))
    mode = rota.pick("i16", [q for q, need in ((0, "T"), (1, "L"), (2, ""), (3, "TLC")) if all(ch in pat for ch in need)])
    cmode = rota.pick("cmode", [q for q, need in ((0, ""), (1, "L"), (2, "T"), (3, "TLC")) if all(ch in pat for ch in need)])
    if variant == "rota":                                           # every mode with DC only, AC only and both
        variant, chroma = rota.pick(("levels", mode), ["dc", "ac", "both"]), rota.pick(("clevels", cmode), ["dc", "ac", "both"])
    amp = amp_for(qp, target)
    c = chroma_coef(rng, qp, target, chroma in ("dc", "both"), chroma in ("ac", "both")) if chroma != "none" else {}
    if variant in ("dc", "both"):
        c["ydc"] = sparse(rng, 16, amp, rng.integers(1, 7))
    if variant in ("ac", "both"):
        c["y"] = {int(k): sparse(rng, 16, amp, rng.integers(1, 4), first=1) for k in rng.choice(16, size=6, replace=False)}
    m = dict(t="i16", mode=mode, cmode=cmode)
    if c:
        m["coef"] = c
        fit(seq, m, qp)
    return m


def make_inter(rng, seq, qp, ref=0, t8=False, target=40, coef=True):
    m = dict(t="16x16", l0=(ref, (int(rng.integers(-40, 41)), int(rng.integers(-40, 41)))))
    if coef:
        amp = amp_for(qp, target)
        c = chroma_coef(rng, qp, target)
        if t8:
            m["t8"] = 1
            c["y8"] = {int(k): sparse(rng, 64, amp, rng.integers(1, 9)) for k in rng.choice(4, size=int(rng.integers(1, 5)), replace=False)}
        else:
            c["y"] = {int(k): sparse(rng, 16, amp, rng.integers(1, 5)) for k in rng.choice(16, size=int(rng.integers(1, 17)), replace=False)}
        m["coef"] = c
        fit(seq, m, qp)
    return m


def picture(rng, rota, seq, kinds, qp, poc, kind="I", layout="pic", target=40, **kw):
    """kinds(a, x, y) -> "pcm" | "i4" | "i8" | "i16" | "inter" | "inter8" per macroblock"""
    mbw, mbh = ac.dims(seq["width"], seq["height"])
    p = dict(kind=kind, poc=poc, layout=layout, qp=qp, mbs=[], **kw)
    for a in range(mbw * mbh):
        t = kinds(a, a % mbw, a // mbw)
        if t == "pcm":
            p["mbs"].append(pcm_noise(rng))
        elif t in ("i4", "i8"):
            p["mbs"].append(make_nxn(rng, rota, seq, p, a, qp, t, target))
        elif t == "i16":
            p["mbs"].append(make_i16(rng, rota, seq, p, a, qp, "rota", target))
        else:
            p["mbs"].append(make_inter(rng, seq, qp, 0, t == "inter8", target))
    return p


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
def nxn_modes_case(t, seed):
    def build(w, h):
        rng, rota = np.random.default_rng(seed), Rota()
        seq = dict(width=w, height=h, profile=100, transform8x8=1) if t == "i8" else dict(width=w, height=h)
        pics = [picture(rng, rota, seq, lambda a, x, y: "pcm" if (x + 2 * y) % 5 == 2 else t, 28, 0),
                picture(rng, rota, seq, lambda a, x, y: "pcm" if (x + y) % 4 == 1 else t, 31, 2),
                picture(rng, rota, seq, lambda a, x, y: t, 24, 4, layout="mb"),                   # one slice per macroblock: no neighbour outside
                picture(rng, rota, seq, lambda a, x, y: "pcm" if (x + y) % 3 == 2 else t, 35, 6, layout="row"),
                picture(rng, rota, seq, lambda a, x, y: t, 22, 8)]
        return seq, pics
    return build


def i4_i8_mode_prediction(constrained):
    def build(w, h):
        rng, rota = np.random.default_rng(0xC300 + constrained), Rota()
        seq = dict(width=w, height=h, profile=100, transform8x8=1, constrained_intra=constrained)
        mbw, mbh = ac.dims(w, h)
        mix = ("i4", "i8", "i4", "i16", "i8", "pcm", "i8", "i4")
        pics = [ac.noise_pic(rng, mbw, mbh, qp=27),
                picture(rng, rota, seq, lambda a, x, y: mix[(a + y) % 8], 27, 2, is_ref=False),
                picture(rng, rota, seq, lambda a, x, y: mix[(3 * a + y) % 8], 30, 4, is_ref=False, layout="row"),
                picture(rng, rota, seq, lambda a, x, y: ("inter", "i4", "i8", "inter8", "i8", "i4", "inter")[(a + 2 * y) % 7], 29, 6, kind="P", is_ref=False),
                picture(rng, rota, seq, lambda a, x, y: ("i8", "inter", "i4", "i16")[(a + y) % 4], 26, 8, kind="P", is_ref=False)]
        return seq, pics
    return build


def i16_and_chroma_residual(w, h):
    """The four luma and four chroma modes with DC only, AC only and both (picture(): by address); then macroblocks whose DC matrix has ONE entry, at
    each of the 16 (chroma: 4) positions, with both signs."""
    rng, rota = np.random.default_rng(0xC400), Rota()
    seq = dict(width=w, height=h)
    mbw, mbh = ac.dims(w, h)
    pics = [picture(rng, rota, seq, lambda a, x, y: "pcm" if (x + 2 * y) % 5 == 3 else "i16", 30, 0),
            picture(rng, rota, seq, lambda a, x, y: "pcm" if (x + y) % 4 == 2 else "i16", 37, 2),
            picture(rng, rota, seq, lambda a, x, y: "i16", 20, 4)]
    p = dict(kind="I", poc=6, layout="pic", qp=33, mbs=[])
    for a in range(mbw * mbh):
        m = make_i16(rng, rota, seq, p, a, 33, "none", chroma="none")
        one = [0] * 16
        one[a % 16] = (3, -3, 2, -5)[(a // 16 + a) % 4]
        cdc = ([0] * 4, [0] * 4)
        cdc[a % 2][(a // 2) % 4] = (4, -4)[(a // 8) % 2]
        m["coef"] = dict(ydc=one, cdc=cdc)
        p["mbs"].append(fit(seq, m, 33))
    return seq, pics + [p]


def coded_list(rng, n, first_two):
    """n values in zig-zag order; zig-zag positions 1 and 2 are m[0][1] and m[1][0]: unequal, so a transposed table shows"""
    v = [int(q) for q in rng.integers(8, 60, n)]
    v[1], v[2] = first_two
    return v


def qp_sweep(lists, offs, seed):
    def build(w, h):
        rng, rota = np.random.default_rng(seed), Rota()
        seq = dict(width=w, height=h, profile=100, transform8x8=1, chroma_qp_off=offs[0], second_chroma_qp_off=offs[1])
        if lists == "default":
            seq["sps_lists"] = ["default"] * 8
        elif lists == "coded":
            seq["sps_lists"] = [coded_list(rng, 16, (71, 9)) for _ in range(6)] + [coded_list(rng, 64, (71, 9)) for _ in range(2)]
        mbw, mbh = ac.dims(w, h)
        # QPY 0 .. 51 upwards through mb_qp_delta (first 26 -> 51, then the wrap through 51 to 0), then downwards through 0 to 51, 38, 25, ...
        # and both sides of qP 24 and qP 36 in every macroblock kind
        kinds = ("i16", "i4", "i8")
        targets = [(q, None) for q in [51] + list(range(52)) + [0, 51, 38, 25, 12, 50]] + [(q, t) for t in kinds for q in (36, 35, 24, 23)]
        pics, n = [], 0
        for k in range((len(targets) + mbw * mbh - 1) // (mbw * mbh)):
            p = dict(kind="I", poc=2 * k, layout="pic", qp=26, mbs=[])
            pred = 26
            for a in range(mbw * mbh):
                qp, t = targets[n % len(targets)]
                n += 1
                t = t or kinds[n % 3]
                m = make_i16(rng, rota, seq, p, a, qp) if t == "i16" else make_nxn(rng, rota, seq, p, a, qp, t)
                m["dqp"] = (qp - pred + 26) % 52 - 26
                pred = qp
                p["mbs"].append(m)
            pics.append(p)
        return seq, pics
    return build


def scaling_lists(variant):
    def build(w, h):
        rng, rota = np.random.default_rng(0xC600 + len(variant)), Rota()
        c4 = lambda: coded_list(rng, 16, (71, 9))
        c8 = lambda: coded_list(rng, 64, (71, 9))
        seq = dict(width=w, height=h, profile=100, transform8x8=1)
        if variant in ("sps", "pps_over_sps"):
            # rule A: list 1 falls back to list 0; list 3 to Default_4x4_Inter; list 5 to list 4; list 7 to Default_8x8_Inter; list 2: the escape
            seq["sps_lists"] = [c4(), None, "default", None, c4(), None, c8(), None]
        if variant == "pps_over_sps":
            # rule B: lists 0 and 6 fall back to the SPS's; list 2 to the PPS's list 1; list 4 to the PPS's list 3 (here: Default through the escape)
            seq["pps_lists"] = [None, c4(), None, "default", None, c4(), None, c8()]
        if variant == "pps_only":
            # no matrix in the SPS: an absent list of the PPS follows rule A
            seq["pps_lists"] = [None, None, c4(), None, c4(), None, None, "default"]
        mbw, mbh = ac.dims(w, h)
        pics = [ac.noise_pic(rng, mbw, mbh, qp=28),
                picture(rng, rota, seq, lambda a, x, y: ("i4", "i8", "i16", "pcm")[(a + y) % 4], 28, 2, is_ref=False),
                picture(rng, rota, seq, lambda a, x, y: ("inter", "inter8", "i4", "inter", "i8", "inter8")[(a + y) % 6], 34, 4, kind="P", is_ref=False)]
        return seq, pics
    return build


def transform_8x8(w, h):
    """Intra8x8 and inter 16x16 with transform_size_8x8_flag: single coefficients at the four corners, in the last row and the last column, dense blocks
    of 64, and a DC level that brings d to within 8 of +-32767 (QPY 6, flat lists: d = (3276 * 320 + 16) >> 5 = 32760) -- which is also a level
    that needs level_prefix 16."""
    rng, rota = np.random.default_rng(0xC700), Rota()
    seq = dict(width=w, height=h, profile=100, transform8x8=1)
    mbw, mbh = ac.dims(w, h)
    spots = [(0, 0), (0, 7), (7, 0), (7, 7), (7, 3), (2, 7), (7, 6), (5, 7)]
    pics = [ac.noise_pic(rng, mbw, mbh, qp=30)]
    for k, (kind, qp) in enumerate((("I", 30), ("P", 38), ("I", 6), ("P", 6))):
        p = dict(kind=kind, poc=2 + 2 * k, layout="pic", qp=qp, mbs=[], is_ref=False)
        for a in range(mbw * mbh):
            m = make_nxn(rng, rota, seq, p, a, qp, "i8") if kind == "I" or a % 3 == 2 else make_inter(rng, seq, qp, 0, True)
            amp = amp_for(qp, 60)
            y8 = {}
            for b8 in range(4):
                lv = [0] * 64
                what = (a + b8) % 4
                if what == 0:
                    r, c = spots[(a // 4 + b8) % 8]
                    lv[8 * r + c] = amp * (1 if (a + b8) % 8 < 4 else -1)
                elif what == 1:
                    lv = [int(v) for v in rng.integers(-max(1, amp // 6), max(1, amp // 6) + 1, 64)]
                elif what == 2 and qp == 6:
                    lv[0] = 3276 * (1 if a % 2 else -1)
                else:
                    lv = sparse(rng, 64, amp, 5)
                y8[b8] = lv
            m["coef"]["y8"] = y8
            m["coef"].pop("y", None)
            p["mbs"].append(fit(seq, m, qp))
        pics.append(p)
    return seq, pics


def from_scan(scan):
    """16 levels in raster order from levels in scan order"""
    out = [0] * 16
    for k, v in enumerate(scan):
        out[ZIGZAG_4x4[k]] = v
    return out


def cavlc_levels(w, h):
    """Numerically dull (QPY 0, where large levels stay inside 16 bits), for the writer and the host parser: the level coding of 9.2.2.1 and the
    tables of 9.2.1 - 9.2.3 on every path (REQUIRED["cavlc_levels"])."""
    rng, rota = np.random.default_rng(0xC800), Rota()
    seq = dict(width=w, height=h, profile=100)
    mbw, mbh = ac.dims(w, h)
    blocks = [
        [60, 49, 25, 13, 7, 4, 2],                                  # coded from the last: suffixLength 0, 1, 2, 3, 4, 5, 6 (and the -2 rule on the first)
        [0, 8, 1, -1, 1],                                           # three trailing ones, then levelCode 14 at suffixLength 0: level_prefix 14
        [0, 0, -16, 1, 1, -1],                                      # ... levelCode 31: level_prefix 15 at suffixLength 0
        [17],                                                       # no trailing one: levelCode 32 - 2 = 30: level_prefix 15 at suffixLength 0
        [2, -2, 2, -2, 2, -2, 2, -2, 2, -2, 2, 1],                  # 12 coefficients, one trailing one: suffixLength starts at 1
        [3, 0, 0, 0, 0, 0, 0, 0, 0, -2, 0, 0, 0, 0, 0, 1],          # run_before 8 and 5 with zerosLeft above 6
        [1200],                                                     # levelCode 2398 - 2: level_prefix 15 with twelve suffix bits
        [-3000],                                                    # levelCode 5999 - 2 >= 30 + 4096: level_prefix 16
        [1] * 16, [2, 1, 1, 1, 1, 1, 1, 1, 1], [1, -1, 1, 1, -1], [1, 1, 1], [-1]]
    p = dict(kind="I", poc=0, layout="pic", qp=0, mbs=[])
    n = 0
    for a in range(mbw * mbh):
        modes = [2] * 16
        y = {}
        dense = (9, 5, 3, 1, 16)[a % 5]                             # TotalCoeff of the filler blocks: nC 8 and up, 4 - 7, 2 - 3, 0 - 1
        for k in range(16):
            if (k + a) % 3 == 0:
                y[k] = from_scan(blocks[n % len(blocks)])
                n += 1
            else:
                y[k] = from_scan([(1, -1, 2)[(i + k) % 3] for i in range(dense)])
        m = dict(t="i4", modes=modes, cmode=0, coef=dict(y=y, cdc=([3, 0, -1, 1], [0, 0, 0, 2]), cac={(0, 1): [1] * 15, (1, 2): [0] * 9 + [2] + [0] * 5}))
        rr.mb_residual(seq, m, 0)                                   # conforming as typed: nothing is shrunk here
        p["mbs"].append(m)
    return seq, [p]


def p_intra(dense, constrained):
    """P pictures over a noise picture: inter macroblocks with residual, and intra islands (I4x4, I8x8, I16) that touch horizontally, vertically and
    diagonally in both directions.  dense = False: fewer than 1/16 of a picture's macroblocks are intra; True: at least 1/16."""
    def build(w, h):
        rng, rota = np.random.default_rng(0xC900 + 2 * dense + constrained), Rota()
        seq = dict(width=w, height=h, profile=100, transform8x8=1, constrained_intra=constrained)
        mbw, mbh = ac.dims(w, h)
        n = mbw * mbh
        at = lambda x, y: y * mbw + x
        if dense:
            groups = [{a: ("i4", "i8", "i16")[(a // 2) % 3] for a in range(n) if (a + a // mbw) % 2 == 0},
                      {a: ("i8", "i16", "i4")[a % 3] for a in range(n) if a % mbw in (1, 2) or a // mbw == 2},
                      {a: ("i16", "i4", "i8")[a % 3] for a in range(n) if a % 5 != 0}]
        else:
            per = max(1, (n - 1) // 16)                             # per * 16 < n
            spots = [[(1, 1), (2, 1), (3, 1)], [(2, 1), (2, 2), (2, 3)], [(1, 1), (2, 2), (3, 3)], [(3, 1), (2, 2), (1, 3)], [(0, 0), (1, 0), (0, 1)],
                     [(mbw - 1, 1), (mbw - 2, 2), (mbw - 1, 2)], [(1, mbh - 1), (2, mbh - 1), (2, mbh - 2)], [(2, 2), (3, 2), (3, 3)]]
            groups = [{at(min(x, mbw - 1), min(y, mbh - 1)): ("i4", "i8", "i16")[(i + j) % 3] for j, (x, y) in enumerate(g[:per])} for i, g in enumerate(spots)]
        pics = [ac.noise_pic(rng, mbw, mbh, qp=30)]
        for k, g in enumerate(groups):
            pics.append(picture(rng, rota, seq, lambda a, x, y: g.get(a, "inter8" if (a + k) % 3 == 0 else "inter"), 26 + 3 * (k % 4), 2 + 2 * k, kind="P",
                                is_ref=False))
        return seq, pics
    return build


def clip1(w, h):
    """Prediction plus residual beyond 0 and beyond 255 in every macroblock kind and both chroma planes: levels aimed at +-250."""
    rng, rota = np.random.default_rng(0xCA00), Rota()
    seq = dict(width=w, height=h, profile=100, transform8x8=1)
    mbw, mbh = ac.dims(w, h)
    pics = [ac.noise_pic(rng, mbw, mbh, qp=32),
            picture(rng, rota, seq, lambda a, x, y: ("i4", "i8", "i16", "pcm")[(a + y) % 4], 32, 2, is_ref=False, target=250),
            picture(rng, rota, seq, lambda a, x, y: ("inter", "inter8", "i4", "i16", "i8", "inter")[(a + y) % 6], 36, 4, kind="P", is_ref=False, target=250)]
    return seq, pics


CASES = {
    "i4_modes": nxn_modes_case("i4", 0xC100),
    "i8_modes": nxn_modes_case("i8", 0xC200),
    "i4_i8_mode_prediction": i4_i8_mode_prediction(0),
    "i4_i8_mode_prediction_constrained": i4_i8_mode_prediction(1),
    "i16_and_chroma_residual": i16_and_chroma_residual,
    "qp_sweep_flat": qp_sweep("flat", (-12, 5), 0xC500),
    "qp_sweep_default_lists": qp_sweep("default", (0, -7), 0xC501),
    "qp_sweep_coded_lists": qp_sweep("coded", (12, 3), 0xC502),
    "scaling_lists_sps": scaling_lists("sps"),
    "scaling_lists_pps_over_sps": scaling_lists("pps_over_sps"),
    "scaling_lists_pps_only": scaling_lists("pps_only"),
    "transform_8x8": transform_8x8,
    "cavlc_levels": cavlc_levels,
    "p_intra_islands": p_intra(False, 0),
    "p_intra_islands_constrained": p_intra(False, 1),
    "p_intra_dense": p_intra(True, 0),
    "p_intra_dense_constrained": p_intra(True, 1),
    "clip1": clip1,
}
INTRA_ONLY = ["i4_modes", "i8_modes", "i16_and_chroma_residual", "qp_sweep_flat", "qp_sweep_default_lists", "qp_sweep_coded_lists", "cavlc_levels"]
P_CASES = ["p_intra_islands", "p_intra_islands_constrained", "p_intra_dense", "p_intra_dense_constrained"]


def case_sizes(name):
    return SIZES_INTRA if name in INTRA_ONLY else ([SIZE, (128, 128)] if name.startswith("p_intra_islands") else [SIZE])


def intra_counts(seq, pics):
    """(intra macroblocks that are predicted -- I_PCM is not --, macroblocks) per picture, from the script: what the decoder's "intra_mbs" counts"""
    return [(sum(m["t"] in ("i4", "i8", "i16") for m in p["mbs"]), len(p["mbs"])) for p in pics]


@functools.lru_cache(maxsize=None)
def scripted(name, size=SIZE):
    """(seq, pics, stream, expected planes, coverage) of a case: computed once, never modified.  coverage: the set of everything the restatement
    (rstats of analytic_expect.expect_h264) and the writer (seen of scripted_h264.write) counted."""
    seq, pics = CASES[name](*size)
    cov = set()
    data = sw.write(seq, pics, cov)
    planes = ae.expect_h264(seq, pics, rstats=cov)
    return seq, pics, data, planes, frozenset(cov)


def with_deblocking(pics):
    """the same script with the deblocking filter on in every picture (tests/deblock_ref.py then filters the expectation)"""
    return [dict(p, deblock=(0, 0, 0)) for p in pics]


ROUTE_CASES = ["i4_modes", "i8_modes", "i16_and_chroma_residual", "qp_sweep_coded_lists", "scaling_lists_pps_over_sps", "transform_8x8", "clip1"] + P_CASES


@functools.lru_cache(maxsize=None)
def scripted_deblocked(name, size=SIZE):
    """(seq, pics, stream, expected planes, counters of deblock_ref) of the case with the deblocking filter on in every picture"""
    seq, pics = CASES[name](*size)
    pics = with_deblocking(pics)
    stats = {}
    return seq, pics, sw.write(seq, pics), ae.expect_h264(seq, pics, stats), stats


@functools.lru_cache(maxsize=None)
def tall_intra_script():
    """16x8208 (1 x 513 macroblocks: above the 512 rows of the banded kernels, where k_recon_intra runs whatever the share of intra macroblocks):
    Intra4x4 with levels in every block, every fourth macroblock Intra16x16.  (seq, pics, stream, expected planes)"""
    rng, rota = np.random.default_rng(0xCB00), Rota()
    seq = dict(width=16, height=8208)
    pics = [picture(rng, rota, seq, lambda a, x, y: "i4" if a % 4 else "i16", 30, 0)]
    return seq, pics, sw.write(seq, pics), ae.expect_h264(seq, pics)
