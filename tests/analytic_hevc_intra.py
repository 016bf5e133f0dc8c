"""The known-answer cases of H.265 intra prediction: scripts for tests/scripted_hevc.py whose expected pictures tests/hevc_intra_ref.py computes
from the clauses.  name -> builder() -> (seq, pics); every stream has the deblocking filter and SAO off.

An intra block predicted only from other predicted blocks turns smooth and stops telling filters apart, so (except in intra_wavefront) intra units
are interleaved with PCM units of noise: pcm_log2 is (3, 5).  The coverage each case owes is asserted in tests/test_hevc_intra_host.py from the
records of the expectation, not here."""
import numpy as np

import scripted_hevc as hw


def pcm(rng, n, lo=0, hi=256):
    return dict(t="pcm", y=rng.integers(lo, hi, (n, n), dtype=np.uint8), cb=rng.integers(lo, hi, (n // 2, n // 2), dtype=np.uint8),
                cr=rng.integers(lo, hi, (n // 2, n // 2), dtype=np.uint8))


def intra(modes, chroma=4, tu=None, dc=None):
    u = dict(t="intra", modes=list(modes), chroma=chroma, tu=(1 if len(modes) == 4 else 0) if tu is None else tu)
    if dc is not None:
        u["dc"] = dc
    return u


SKIP = dict(t="skip")


def picture(seq, pick):
    """cus of one picture: pick(x, y, log2) -> a unit or "split"; blocks that cross the picture edge are split without asking"""
    W, H = hw.coded_size(seq)
    g = hw.geometry(seq)
    cw, ch = hw.ctb_dims(seq)

    def node(x, y, log2):
        n = 1 << log2
        if x >= W or y >= H:
            return None
        u = "split" if (x + n > W or y + n > H) else pick(x, y, log2)
        if isinstance(u, str):
            assert log2 > g["min_cb"], (x, y, log2)
            return dict(t="split", sub=[node(x + (i & 1) * (n >> 1), y + (i >> 1) * (n >> 1), log2 - 1) for i in range(4)])
        return u
    return [node((a % cw) << g["ctb"], (a // cw) << g["ctb"], g["ctb"]) for a in range(cw * ch)]


def geometric_all_available(seq, x, y, n):
    """whether all 4 n + 1 neighbours of the luma block lie inside the picture and earlier in z-scan order (slices aside): decided by the two ends
    of the below-left and of the above-right group.  Only steers which counter of ModeWheel a block draws its mode from."""
    W, H = hw.coded_size(seq)
    g = hw.geometry(seq)
    cw, _ = hw.ctb_dims(seq)
    if x == 0 or y == 0 or y + 2 * n > H or x + 2 * n > W:
        return False
    z = hw.zscan(x, y, g["ctb"], cw)
    return hw.zscan(x - 1, y + 2 * n - 1, g["ctb"], cw) < z and hw.zscan(x + 2 * n - 1, y - 1, g["ctb"], cw) < z and \
        hw.zscan(x - 1, y + n, g["ctb"], cw) < z and hw.zscan(x + n, y - 1, g["ctb"], cw) < z


class ModeWheel:
    """Hands out the 35 modes in turn, separately per (block size, all neighbours available or not), and intra_chroma_pred_mode values such that
    every value meets every luma mode class, the luma modes 0 / 26 / 10 / 1 meeting 'their' value (-> 34) in turn"""

    def __init__(self, start=0, only=None):
        self.count, self.k, self.start, self.only = {}, 0, start, only or list(range(35))

    def luma(self, n, all_available):
        key = (n, all_available)
        self.count[key] = self.count.get(key, self.start) + 1
        return self.only[(self.count[key] - 1) % len(self.only)]

    def chroma(self, mode):
        self.k += 1
        same = {0: 0, 26: 1, 10: 2, 1: 3}
        if mode in same and self.k % 2:
            return same[mode]
        return (self.k // 2) % 5


def mosaic_pick(seq, rng, wheel, top=None, p_intra64=0.15):
    """A checkerboard of PCM noise and intra units at every level: at a level, blocks of one colour are PCM; the others are intra units of that
    size (transform depth 0 .. 2, or NxN at 8x8) or, above 8x8, split into the next level"""
    g = hw.geometry(seq)
    top = min(g["ctb"], 5) if top is None else top

    def pick(x, y, log2):
        n = 1 << log2
        if log2 > top:
            if log2 == 6 and rng.random() < p_intra64:              # a 64x64 unit: four 32x32 transform blocks by inference (log2 > MaxTbLog2SizeY)
                m = wheel.luma(32, geometric_all_available(seq, x, y, 32))
                return intra([m], wheel.chroma(m), tu=1)
            return "split"
        if ((x >> log2) + (y >> log2)) & 1:
            return pcm(rng, n)
        r = rng.random()
        if log2 > 3 and geometric_all_available(seq, x, y, n) and (log2 == 5 or r < 0.5):     # rare at these sizes: do not split them away
            m = wheel.luma(n, True)
            return intra([m], wheel.chroma(m), tu=0)
        if log2 > 3 and r < (0.45 if log2 == 5 else 0.55):
            return "split"
        if log2 == 3 and r < 0.5:                                   # NxN: four 4x4 luma blocks, a mode each
            ms = [wheel.luma(4, geometric_all_available(seq, x + 4 * (i & 1), y + 4 * (i >> 1), 4)) for i in range(4)]
            return intra(ms, wheel.chroma(ms[0]))
        tu = int(rng.integers(0, min(g["tu_depth"], log2 - 2) + 1))
        if log2 - tu > g["max_tb"]:
            tu = log2 - g["max_tb"]
        tb = n >> tu
        m = wheel.luma(tb, geometric_all_available(seq, x, y, tb))
        return intra([m], wheel.chroma(m), tu=tu)
    return pick


def every_mode_and_size(ctb_log2, width, height, n_pics, seed, start=0, only=None):
    rng = np.random.default_rng(seed)
    seq = dict(width=width, height=height, ctb_log2=ctb_log2, min_cb_log2=3, max_tb_log2=min(ctb_log2, 5), tu_depth_intra=2,
               pcm_log2=(3, min(ctb_log2, 5)))
    wheel = ModeWheel(start, only)
    pics = [dict(kind="I", poc=2 * k, is_ref=False, cus=picture(seq, mosaic_pick(seq, rng, wheel))) for k in range(n_pics)]
    return seq, pics


def noise_planes(rng, seq):
    W, H = hw.coded_size(seq)
    return [rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8),
            rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8)]


def cut(planes, x, y, n):
    """the PCM unit that carries the planes' samples of the block at (x, y)"""
    return dict(t="pcm", y=planes[0][y:y + n, x:x + n].copy(), cb=planes[1][y // 2:(y + n) // 2, x // 2:(x + n) // 2].copy(),
                cr=planes[2][y // 2:(y + n) // 2, x // 2:(x + n) // 2].copy())


def pcm_picture(rng, seq, kind="I", poc=0, **kw):
    g = hw.geometry(seq)
    planes = noise_planes(rng, seq)
    return dict(kind=kind, poc=poc, cus=picture(seq, lambda x, y, log2: "split" if log2 > g["pcm"][1] else cut(planes, x, y, 1 << log2)), **kw)


# ---- intra_strong_smoothing ------------------------------------------------------------------------------------------------------------------
STRONG_VALUES = [(7, 7), (8, 7), (7, 8), (3, 5), (20, 2), (1, 31), (8, 8)]      # Abs(...) of the row above, of the left column (8.4.4.2.3), per picture
STRONG_MODES = [0, 2, 18, 34, 9, 27, 11]


def strong_smoothing(strong):
    """160x128 with 64x64 CTBs: a PCM first CTB row and column; the 32x32 block at (64, 64) has all 129 neighbours, the one at (128, 64) lies in
    the 32 samples wide last CTB column: its upper-right neighbours are outside the picture and take p[31][-1].  The samples p[-1][-1], p[31][-1],
    p[63][-1], p[-1][31], p[-1][63] are set in the PCM units around them such that the two expressions take the values of STRONG_VALUES."""
    rng = np.random.default_rng(0xC200)
    seq = dict(width=160, height=128, ctb_log2=6, min_cb_log2=5, max_tb_log2=5, pcm_log2=(5, 5), strong_intra=strong)
    pics = []
    for k, ((tt, tl), mode) in enumerate(zip(STRONG_VALUES, STRONG_MODES)):
        planes = noise_planes(rng, seq)
        Y = planes[0]
        for (x, y, substituted) in ((64, 64, False), (128, 64, True)):
            s = 1 if (k + substituted) % 2 else -1
            if substituted:                                         # its corner is the first block's p[63][-1]; p[63][-1] = p[31][-1] here: the
                a = int(Y[y - 1, x - 1])                            # expression is Abs(p[-1][-1] - p[31][-1])
                b = a + s * tt
            else:
                a, b = int(rng.integers(100, 156)), int(rng.integers(100, 156))
                Y[y - 1, x - 1], Y[y - 1, x + 63] = a, 2 * b - a + s * tt
            e = int(rng.integers(40, 216))
            e += (a + e + tl) & 1
            d = (a + e + s * tl) // 2                               # a + e - 2 d = -s * tl
            Y[y - 1, x + 31], Y[y + 31, x - 1], Y[y + 63, x - 1] = b, d, e
        pick = lambda x, y, log2: "split" if log2 == 6 else (intra([mode], k % 5) if (x, y) in ((64, 64), (128, 64)) else cut(planes, x, y, 32))
        pics.append(dict(kind="I", poc=2 * k, is_ref=False, cus=picture(seq, pick)))
    return seq, pics


# ---- intra_substitution ----------------------------------------------------------------------------------------------------------------------
def substitution(ctb_log2, width, height, n_pics, seed, start):
    """The mosaic in slices of one CTB, one CTB row and one picture, in pictures that end inside a CTB on both sides"""
    seq, pics = every_mode_and_size(ctb_log2, width, height, n_pics, seed, start)
    for k, p in enumerate(pics):
        p["layout"] = ("ctb", "row", "pic")[k % 3]
    return seq, pics


# ---- intra_constrained -----------------------------------------------------------------------------------------------------------------------
def random_intra(rng, wheel, log2, max_tu):
    if log2 == 3 and rng.random() < 0.4:
        ms = [wheel.luma(4, False) for _ in range(4)]
        return intra(ms, wheel.chroma(ms[0]))
    tu = int(rng.integers(0, min(max_tu, log2 - 2) + 1))
    m = wheel.luma((1 << log2) >> tu, False)
    return intra([m], wheel.chroma(m), tu=tu)


PROBES = [{0}, {1}, {2}, {3}, {4}, {1, 3}]      # the neighbour groups (hevc_intra_ref.GROUPS) that are skipped units, per CTB of the last picture


def constrained(flag):
    """A PCM noise I picture, then three P pictures in one slice of skipped, PCM and intra units of 8x8 .. 32x32 drawn at random (more and more of
    them skipped); the 8x8 unit at (40, 40) of the third is enclosed by skipped units.  A fourth P picture holds the probes: an intra unit per CTB
    whose neighbours are PCM units but for the groups of PROBES -- each of the five sides alone, then the left column and the row above together."""
    rng = np.random.default_rng(0xC400)
    seq = dict(width=104, height=72, ctb_log2=5, min_cb_log2=3, max_tb_log2=5, tu_depth_intra=1, pcm_log2=(3, 5), constrained_intra=flag)
    wheel = ModeWheel()
    pics = [pcm_picture(rng, seq)]
    for k, p_skip in enumerate((0.35, 0.6, 0.8)):
        def pick(x, y, log2):
            if k == 2 and 32 <= x < 64 and 32 <= y < 64:
                return "split" if log2 > 3 else (intra([wheel.luma(8, False)], 1) if (x, y) == (40, 40) else SKIP)
            if log2 > 3 and rng.random() < (0.7 if log2 == 5 else 0.5):
                return "split"
            r = rng.random()
            if r < p_skip:
                return SKIP
            if r < p_skip + (1 - p_skip) * 0.3:
                return pcm(rng, 1 << log2)
            return random_intra(rng, wheel, log2, 1)
        pics.append(dict(kind="P", poc=2 + 2 * k, layout="pic", cus=picture(seq, pick)))

    # probes: in every whole CTB the 8x8 unit at (16, 16) is intra, the five 8x8 units that hold its neighbour groups are PCM except those of PROBES
    def probe(x, y, log2):
        if log2 > 3:
            return "split"
        cx, cy = x >> 5, y >> 5
        if cx < 3 and cy < 2:
            dx, dy = (x & 31) - 16, (y & 31) - 16
            if (dx, dy) == (0, 0):
                return intra([wheel.luma(8, False)], wheel.chroma(0))
            where = {(-8, 8): 0, (-8, 0): 1, (-8, -8): 2, (0, -8): 3, (8, -8): 4}.get((dx, dy))
            if where in PROBES[cy * 3 + cx]:
                return SKIP
        return pcm(rng, 8)
    pics.append(dict(kind="P", poc=8, layout="pic", is_ref=False, cus=picture(seq, probe)))
    return seq, pics


# ---- intra_wavefront -------------------------------------------------------------------------------------------------------------------------
TEXTURE_MODES = (2, 18, 34, 10, 26)


def wavefront(ctb_log2, width, height, n_pics, seed):
    """A PCM noise first CTB row and first CTB column, every other CTB 8x8 units with four 4x4 blocks of modes that copy their neighbours: what
    a CTB predicts depends on CTBs far to the left and above"""
    rng = np.random.default_rng(seed)
    seq = dict(width=width, height=height, ctb_log2=ctb_log2, min_cb_log2=3, max_tb_log2=min(ctb_log2, 5), tu_depth_intra=1,
               pcm_log2=(3, min(ctb_log2, 5)))
    s = 1 << ctb_log2
    pics = []
    for k in range(n_pics):
        def pick(x, y, log2):
            if x < s or y < s:
                return "split" if log2 > 5 else pcm(rng, 1 << log2)
            if log2 > 3:
                return "split"
            if rng.random() < 0.25:
                return intra([TEXTURE_MODES[int(rng.integers(0, 5))]], int(rng.integers(0, 5)), tu=1)
            return intra([TEXTURE_MODES[int(i)] for i in rng.integers(0, 5, 4)], 4)
        pics.append(dict(kind="I", poc=2 * k, is_ref=False, cus=picture(seq, pick)))
    return seq, pics


# ---- intra_scattered_in_b --------------------------------------------------------------------------------------------------------------------
def scattered_in_b(ctb_log2, width, height, seed):
    """Two PCM noise pictures (POC 0 and 8), then B pictures between them of skipped units (the rounded mean of the two) with an intra unit here
    and there, at the bottom row / right column of its CTB and away from them; slices of a picture, a CTB, a CTB row"""
    rng = np.random.default_rng(seed)
    seq = dict(width=width, height=height, ctb_log2=ctb_log2, min_cb_log2=3, max_tb_log2=min(ctb_log2, 5), tu_depth_intra=1,
               pcm_log2=(3, min(ctb_log2, 5)))
    wheel = ModeWheel()
    pics = [pcm_picture(rng, seq), pcm_picture(rng, seq, "P", 8, layout="pic")]
    for poc, layout in ((4, "pic"), (2, "ctb"), (6, "row")):
        def pick(x, y, log2):
            if log2 > 3 and rng.random() < (0.8 if log2 > 4 else 0.5):
                return "split"
            return random_intra(rng, wheel, log2, 1) if rng.random() < 0.12 else SKIP
        pics.append(dict(kind="B", poc=poc, layout=layout, cus=picture(seq, pick)))
    return seq, pics


# ---- intra_dc_residual -----------------------------------------------------------------------------------------------------------------------
DC_QPS = (22, 23, 24, 25, 26, 27, 40, 4, 30, 35, 45, 51, 10, 16)


def dc_residual_case():
    """The mosaic with one coefficient at (0, 0) in the transform blocks: a level per block and plane, both signs, sized from the scaling factor
    such that the flat residual is about +-200, +-90 or +-25 in turn; slice QPs over every qP % 6, one where the chroma QP leaves the luma QP (40 -> 36)"""
    rng = np.random.default_rng(0xC700)
    seq = dict(width=104, height=72, ctb_log2=5, min_cb_log2=3, max_tb_log2=5, tu_depth_intra=2, pcm_log2=(3, 5))
    wheel = ModeWheel(7)
    scale = (40, 45, 51, 57, 64, 72)
    pics, turn = [], {}
    for k, qp in enumerate(DC_QPS):
        cus = picture(seq, mosaic_pick(seq, rng, wheel))
        p = dict(kind="I", poc=2 * k, is_ref=False, qp=qp, cus=cus)
        for (x, y, log2, depth, u) in hw.walk(seq, p):
            if u["t"] != "intra":
                continue
            lg = log2 - u["tu"]
            dc = []
            for i in range(4 ** u["tu"]):
                lv = []
                for c in range(3):
                    q = qp if c == 0 or qp < 30 else (qp - 6 if qp > 43 else 29 + (qp - 29) // 2)    # (about Table 8-10: only sizes the level)
                    gain = scale[q % 6] * 2.0 ** (q // 6) / 2.0 ** ((lg if c == 0 else max(lg - 1, 2)) + 6)
                    key = (c, lg)
                    turn[key] = turn.get(key, 0) + 1                # far beyond the sample range in both directions, and near nothing, in turn
                    want = (-200, 200, -25, 25, -90, 90)[turn[key] % 6] + int(rng.integers(-15, 16))
                    level = int(round(want / gain)) or (1 if want > 0 else -1)
                    lv.append(0 if rng.random() < 0.2 else max(-1500, min(1500, level)))
                dc.append(tuple(lv))
            u["dc"] = dc
        pics.append(p)
    return seq, pics


CASES = {
    "intra_every_mode_and_size-ctb64": lambda: every_mode_and_size(6, 200, 136, 18, 0xC164),
    "intra_every_mode_and_size-ctb32": lambda: every_mode_and_size(5, 104, 72, 10, 0xC132),
    "intra_every_mode_and_size-ctb16": lambda: every_mode_and_size(4, 72, 56, 10, 0xC116),
    "intra_every_mode_and_size-edge_filters": lambda: every_mode_and_size(4, 104, 72, 6, 0xC11E, only=[10, 26, 1]),
    "intra_strong_smoothing": lambda: strong_smoothing(1),
    "intra_strong_smoothing-flag_off": lambda: strong_smoothing(0),
    "intra_substitution-ctb64": lambda: substitution(6, 136, 104, 3, 0xC364, 14),
    "intra_substitution-ctb32": lambda: substitution(5, 104, 72, 9, 0xC332, 21),
    "intra_substitution-ctb16": lambda: substitution(4, 72, 56, 9, 0xC316, 28),
    "intra_constrained": lambda: constrained(1),
    "intra_constrained-flag_off": lambda: constrained(0),
    "intra_wavefront-ctb16": lambda: wavefront(4, 160, 48, 3, 0xC516),
    "intra_wavefront-ctb64": lambda: wavefront(6, 128, 128, 2, 0xC564),
    "intra_scattered_in_b-ctb32": lambda: scattered_in_b(5, 104, 72, 0xC632),
    "intra_scattered_in_b-ctb64": lambda: scattered_in_b(6, 136, 104, 0xC664),
    "intra_dc_residual": dc_residual_case,
}
