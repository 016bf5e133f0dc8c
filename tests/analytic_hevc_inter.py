"""The scripted H.265 streams that pin inter prediction (clauses 6.4.2, 8.5.3.2.2 - 8.5.3.2.9; k_hevc_mc with every tile shape): name -> () -> (seq, pics).

The expectation is tests/hevc_inter_ref.py's, computed from the script.  A script states SYNTAX (merge_idx, ref_idx, mvd, mvp flags); what motion that
means follows from the clauses, so most pictures here are drawn from a seeded generator -- units of 8, 16 and 32 samples in every partition, merged,
skipped, predicted, PCM (the intra neighbour) -- and tests/test_hevc_inter_host.py asserts from the expectation's records that every situation the
groups are meant to hold was met.  Vectors that must hit a given window (borders, fractions, alignments) are scripted in pictures with one slice per CTB
and no temporal candidate, where the first prediction unit of a CTB has the predictor (0, 0) and its mvd IS its vector.
References are PCM noise (and what earlier inter pictures made of it): a wrong vector or candidate changes samples."""
import numpy as np

import scripted_hevc as hw

SHAPES = [(8, 4), (4, 8), (8, 8), (16, 4), (16, 12), (4, 16), (12, 16), (16, 8), (8, 16), (16, 16)]       # (w, h) of the motion compensation tiles
JOB_COUNTS = (1, 4, 5, 32, 33, 36, 37)
AMP = ("2NxnU", "2NxnD", "nLx2N", "nRx2N")


def base_seq(w, h, **kw):
    ctb = kw.get("ctb_log2", 5)
    seq = dict(width=w, height=h, ctb_log2=ctb, min_cb_log2=3, max_tb_log2=min(ctb, 5), pcm_log2=(3, min(ctb, 5)))
    seq.update(kw)
    return seq


def pcm_leaf(rng, n):
    return dict(t="pcm", y=rng.integers(0, 256, (n, n), dtype=np.uint8), cb=rng.integers(0, 256, (n // 2, n // 2), dtype=np.uint8),
                cr=rng.integers(0, 256, (n // 2, n // 2), dtype=np.uint8))


def grow(seq, leaf, split=lambda x, y, log2: False):
    """The coding trees of a picture: leaf(x, y, log2) -> unit; a block that crosses the picture edge is split, others where split() says so"""
    W, H = hw.coded_size(seq)
    g = hw.geometry(seq)
    cw, ch = hw.ctb_dims(seq)

    def tree(x, y, log2):
        n = 1 << log2
        if x >= W or y >= H:
            return None
        if x + n > W or y + n > H or (log2 > g["min_cb"] and split(x, y, log2)):
            return dict(t="split", sub=[tree(x + (i & 1) * (n >> 1), y + (i >> 1) * (n >> 1), log2 - 1) for i in range(4)])
        return leaf(x, y, log2)
    return [tree((a % cw) << g["ctb"], (a // cw) << g["ctb"], g["ctb"]) for a in range(cw * ch)]


def noise(rng, seq, kind="I", poc=0, **kw):
    return dict(kind=kind, poc=poc, cus=grow(seq, lambda x, y, log2: pcm_leaf(rng, 1 << log2)), **kw)


def part_choices(seq, log2):
    g = hw.geometry(seq)
    if log2 == g["min_cb"]:
        return ["2Nx2N", "2NxN", "Nx2N"] + (["NxN"] if log2 > 3 else [])
    return ["2Nx2N", "2NxN", "Nx2N"] + (list(AMP) if seq.get("amp", 0) else [])


def coefs(rng, seq, log2, part):
    """A small residual for an inter unit: (tu, coef) at the depth that 7.4.9.8 infers or the script may choose"""
    g = hw.geometry(seq)
    tu = 1 if (g["tu_depth_inter"] == 0 and part != "2Nx2N") or log2 > g["max_tb"] else (int(rng.integers(0, 2)) if g["tu_depth_inter"] and log2 > 2 else 0)
    lg = log2 - tu
    lvl = lambda: {(int(rng.integers(0, 3)), int(rng.integers(0, 3))): int(rng.choice([-5, -2, -1, 1, 2, 4]))}
    out = []
    for i in range(4 ** tu):
        e = {0: lvl()} if i == 4 ** tu - 1 or rng.random() < 0.5 else {}
        if (lg > 2 or i % 4 == 3) and rng.random() < 0.5:
            e[1 + int(rng.integers(0, 2))] = lvl()
        out.append(e or None)
    return tu, out


def random_mvd(rng, wide):
    def one():
        r = rng.random()
        return 0 if r < 0.3 else int(rng.choice([-2, -1, 1, 2])) if r < 0.55 else int(rng.integers(-wide, wide + 1))
    return (0, 0) if rng.random() < 0.3 else (one(), one())


def random_pic(rng, seq, kind, poc, n_ref, *, p_split=0.6, p_pcm=0.06, p_skip=0.15, p_merge=0.4, p_coef=0.25, wide=40, **kw):
    """A P or B picture of random units.  n_ref = (entries of list 0, of list 1) as the slice header will activate them; with slice_n_ref (one
    slice per CTB row) every slice activates its own"""
    mm = kw.get("max_merge", 1)
    rows = kw.get("slice_n_ref")
    assert rows is None or kw.get("layout") == "row"

    def pu(w, h, n_ref):
        if rng.random() < p_merge:
            return dict(merge=int(rng.integers(0, mm)))
        use = [1, 0] if kind == "P" else [[1, 0], [0, 1], [1, 1]][int(rng.integers(0, 2 if w + h == 12 else 3))]
        out = {}
        for l, name in enumerate(("l0", "l1")):
            if use[l]:
                mvd = random_mvd(rng, wide)
                if l == 1 and use[0] and kw.get("mvd_l1_zero", 0):
                    mvd = (0, 0)
                out[name] = (int(rng.integers(0, n_ref[l])), mvd, int(rng.integers(0, 2)))
        return out

    def leaf(x, y, log2):
        n, r = 1 << log2, rng.random()
        if r < p_pcm and log2 <= 4:
            return pcm_leaf(rng, n)
        if r < p_pcm + p_skip:
            return dict(t="skip", merge=int(rng.integers(0, mm)))
        ch = part_choices(seq, log2)
        part = ch[int(rng.integers(0, len(ch)))] if rng.random() < 0.8 else "2Nx2N"
        nr = rows[y >> hw.geometry(seq)["ctb"]] if rows else n_ref
        u = dict(t="inter", part=part, pus=[pu(w, h, nr) for (_, _, w, h) in hw.partitions(part, x, y, n)])
        if (part == "2Nx2N" and "merge" in u["pus"][0]) or rng.random() < p_coef:
            u["tu"], u["coef"] = coefs(rng, seq, log2, part)
        return u
    return dict(kind=kind, poc=poc, n_ref=n_ref, cus=grow(seq, leaf, lambda x, y, log2: rng.random() < p_split), **kw)


def wp_table(rng, n_ref):
    """explicit weights for every entry of both lists (7.4.7.3's final values), some entries with their flags off"""
    ld_y, ld_c = int(rng.integers(0, 8)), int(rng.integers(0, 8))

    def entry():
        y = None if rng.random() < 0.2 else (int(rng.integers((1 << ld_y) - 128, (1 << ld_y) + 128)), int(rng.integers(-128, 128)))
        c = None if rng.random() < 0.2 else tuple((int(rng.integers((1 << ld_c) - 128, (1 << ld_c) + 128)), int(rng.integers(-128, 128))) for _ in (0, 1))
        # moderate weights keep most samples off the clip: a wrong prediction must show
        if y is not None and rng.random() < 0.7:
            y = ((1 << ld_y) + int(rng.integers(-(1 << ld_y) // 2 - 1, (1 << ld_y) // 2 + 2)), int(rng.integers(-20, 20)))
        if c is not None and rng.random() < 0.7:
            c = tuple(((1 << ld_c) + int(rng.integers(-(1 << ld_c) // 2 - 1, (1 << ld_c) // 2 + 2)), int(rng.integers(-20, 20))) for _ in (0, 1))
        if c is not None and not all(-512 <= o - 128 + ((128 * w) >> ld_c) <= 511 for (w, o) in c):      # delta_chroma_offset_l0 (7.4.7.3)
            return entry()
        return dict(y=y, c=c)
    return dict(ld_y=ld_y, ld_c=ld_c, l0=[entry() for _ in range(n_ref[0])], l1=[entry() for _ in range(n_ref[1])])


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------------
def shapes(explicit, seed):
    """Units of 8, 16 and 32 with all eight partitions (AMP on) on P and B pictures, every luma fraction and window alignment by chance over the group
    (asserted), default or explicit weights; 96x80: the coded height ends inside a 32x32 CTB"""
    def build():
        rng = np.random.default_rng(seed)
        seq = base_seq(96, 80, amp=1, weighted_pred=explicit, weighted_bipred=explicit)
        pics = [noise(rng, seq), noise(rng, seq, "P", 8), noise(rng, seq, "P", 16)]
        for k in range(3):
            for kind, poc, n_ref in (("P", 9 + 2 * k, (3, 3)), ("B", 10 + 2 * k, (3, 2))):     # (output order = decoding order but for the reference at POC 16)
                p = random_pic(rng, seq, kind, poc, n_ref, max_merge=2, p_merge=0.2, p_skip=0.08, wide=70, is_ref=False)
                if explicit:
                    p["wp"] = wp_table(rng, n_ref)
                pics.append(p)
        return seq, pics
    return build


# ---- scripted vectors: borders, fractions ---------------------------------------------------------------------------------------------------------
PART_OF = {(16, 16): "2Nx2N", (8, 8): "2Nx2N", (8, 4): "2NxN", (4, 8): "Nx2N", (16, 8): "2NxN", (8, 16): "Nx2N", (16, 4): "2NxnU", (16, 12): "2NxnD",
           (4, 16): "nLx2N", (12, 16): "nRx2N"}                     # the partition whose FIRST prediction unit has the shape (units of 8 and 16)


def whole_ctbs(seq):
    """the addresses of the 16x16 CTBs that lie inside the picture"""
    W, H = hw.coded_size(seq)
    cw, ch = hw.ctb_dims(seq)
    return [a for a in range(cw * ch) if (a % cw) * 16 + 16 <= W and (a // cw) * 16 + 16 <= H]


def directed(seq, blocks, kind="P", poc=40, **kw):
    """A picture with one slice per 16x16 CTB whose first prediction unit carries a scripted vector: blocks[ctb address] = (shape, lists, vector); its
    other units copy RefPicList0[0] (vector difference 0 on the predictor they get)."""
    other = dict(l0=(0, (0, 0), 0))

    def ctb(spec):
        if spec is None:
            return dict(t="skip", merge=0)
        (w, h), lists, mv = spec
        n = 8 if w <= 8 and h <= 8 else 16
        part = PART_OF[(w, h)]
        first = dict(t="inter", part=part, pus=[{("l0", "l1")[l]: (0, mv, 0) for l in lists}] + [other] * (len(hw.partitions(part, 0, 0, n)) - 1))
        return first if n == 16 else dict(t="split", sub=[first] + [dict(t="skip", merge=0)] * 3)
    cw, ch = hw.ctb_dims(seq)
    cut = grow(seq, lambda x, y, log2: dict(t="skip", merge=0))     # (a CTB that the picture edge cuts: skipped 8x8 units)
    whole = whole_ctbs(seq)
    assert all(a in whole for a in blocks)
    return dict(kind=kind, poc=poc, layout="ctb", cus=[ctb(blocks.get(a)) if a in whole else cut[a] for a in range(cw * ch)], is_ref=False, **kw)


def borders(width, height):
    """8x4, 4x8 and 16x16 blocks whose windows cross each side and corner of the reference by one sample and entirely, end exactly at the right edge, or
    lie thousands of samples outside (vectors near +-32767); every second picture B with the vector in list 1."""
    def build():
        rng = np.random.default_rng(0xB0DE + width)
        seq = base_seq(width, height, ctb_log2=4, amp=1)
        W, H = hw.coded_size(seq)
        cw, ch = hw.ctb_dims(seq)
        pics = [noise(rng, seq), noise(rng, seq, "P", 64)]
        wins = []
        for (w, h) in ((8, 4), (4, 8), (16, 16)):
            tw, th = w + 7, h + 7                                   # the luma window of a fractional vector: x - 3 .. x + w + 3
            xs = [-1, -tw, W - tw + 1, W, W - tw, 20]               # left by 1, left whole, right by 1, right whole, ends at the right edge, inside
            ys = [-1, -th, H - th + 1, H, 4]
            wins += [((w, h), x, y) for x in xs for y in ys if (x, y) != (20, 4)]
        far = [(-32768, 5), (32767, -6), (7, -32768), (-9, 32767), (32767, 32767), (-32768, -32768), (-32768, 32767), (32767, -32768)]
        wins += [(s, None, i) for s in ((8, 4), (4, 8), (16, 16)) for i in range(len(far))]
        whole = whole_ctbs(seq)
        per = len(whole)
        for k in range((len(wins) + per - 1) // per):
            blocks = {}
            for j, a in enumerate(whole):
                i = k * per + j
                if i >= len(wins):
                    break
                shape, x, y = wins[i]
                bx, by = (a % cw) * 16, (a // cw) * 16
                frac = (1 + i % 3, 1 + (i // 3) % 3) if i % 4 else (0, 0)     # (integer vectors: the kernel fetches the same window)
                mv = far[y] if x is None else (4 * (x + 3 - bx) + frac[0], 4 * (y + 3 - by) + frac[1])      # window origin = block + (mv >> 2) - 3
                blocks[a] = (shape, [k % 2], mv)
            pics.append(directed(seq, blocks, kind="B" if k % 2 else "P", poc=30 + k))
        return seq, pics
    return build


def fractions(explicit):
    """Every tile shape of units of 8 and 16 at every luma fraction and the four alignments of its window, from list 0, list 1 and both, on P and B
    pictures, default or explicit weights; the blocks are dealt over the pictures in a seeded order, so every picture holds every shape"""
    def build():
        rng = np.random.default_rng(0xF4AC + explicit)
        seq = base_seq(96, 80, ctb_log2=4, amp=1, weighted_pred=explicit, weighted_bipred=explicit)
        cw, ch = hw.ctb_dims(seq)
        pics = [noise(rng, seq), noise(rng, seq, "P", 64)]
        todo = [(s, f, al) for s in SHAPES for f in range(16) for al in range(4) if (f + al) % 4 == 0 or s in ((8, 4), (16, 16))]
        todo = [todo[i] for i in rng.permutation(len(todo))]
        per = cw * ch
        for k in range((len(todo) + per - 1) // per):
            blocks = {}
            for a in range(per):
                if k * per + a < len(todo):
                    s, f, al = todo[k * per + a]
                    ix, iy = int(rng.integers(-6, 6)) * 4 + al, int(rng.integers(-20, 20))
                    lists = [0] if k % 3 == 0 else ([[0], [1], [0, 1]][a % 3] if s[0] + s[1] != 12 else [a % 2])
                    blocks[a] = (s, lists, (4 * ix + (f & 3), 4 * iy + (f >> 2)))
            p = directed(seq, blocks, kind="B" if k % 3 else "P", poc=20 + k)
            if explicit:
                p["wp"] = wp_table(rng, (2, 2))
            pics.append(p)
        return seq, pics
    return build


# ---- job lists ------------------------------------------------------------------------------------------------------------------------------------
def job_lists():
    """Pictures whose number of motion compensation tiles is 1, 4, 5, 32, 33, 36, 37 (four waves per workgroup, the grid rounded to 8 with the remap over
    the XCDs), the rest PCM; then non-reference B pictures in a row with 1, 37 and 4 tiles: a batch whose pictures have fewer tiles than its largest"""
    rng = np.random.default_rng(0x10B5)
    seq = base_seq(96, 80, ctb_log2=4)
    cw, ch = hw.ctb_dims(seq)

    def pic(count, kind, poc):
        quads, ones = count // 4, count % 4                         # CTBs of four 8x8 units, then CTBs of one 16x16 unit, then PCM

        def leaf(x, y, log2):
            if (y >> 4) * cw + (x >> 4) >= quads + ones:
                return pcm_leaf(rng, 1 << log2)
            v = lambda: (int(rng.integers(-30, 30)), int(rng.integers(-30, 30)))
            if kind == "B":
                return dict(t="inter", part="2Nx2N", pus=[dict(l0=(0, v(), 0), l1=(0, v(), 1))])
            return dict(t="inter", part="2Nx2N", pus=[dict(l0=(int(rng.integers(0, 2)), v(), 0))])
        return dict(kind=kind, poc=poc, layout="pic", is_ref=False, cus=grow(seq, leaf, lambda x, y, log2: (y >> 4) * cw + (x >> 4) < quads))
    pics = [noise(rng, seq), noise(rng, seq, "P", 40)]
    pics += [pic(c, "P", 10 + i) for i, c in enumerate(JOB_COUNTS)]
    pics += [pic(c, "B", 20 + i) for i, c in enumerate((1, 37, 4))]
    return seq, pics


# ---- merge ----------------------------------------------------------------------------------------------------------------------------------------
def merge(par, min_cb, seed, mms=(1, 2, 3, 4, 5, 5)):
    """Mostly merged and skipped units, MaxNumMergeCand 1 .. 5 picture by picture, one slice per picture, per CTB row and per CTB, PCM units between;
    parallel merge level 2, 3 or 4; minimum coding block 8 (8x4 / 4x8 units, singleMCLFlag) or 16 (NxN)"""
    def build():
        rng = np.random.default_rng(seed)
        seq = base_seq(96, 80, amp=1, par_mrg_log2=par, min_cb_log2=min_cb, pcm_log2=(min_cb, 5))
        pics = [noise(rng, seq), random_pic(rng, seq, "P", 8, (1, 1), p_merge=0.2, p_skip=0.05, layout="pic", max_merge=2),
                random_pic(rng, seq, "P", 32, (2, 2), p_merge=0.3, layout="pic", max_merge=3)]
        k = 0
        for mm in mms:
            for kind in ("P", "B"):
                layout = ("pic", "pic", "row", "ctb")[k % 4]
                # list 1 of the B pictures at POC 10 .. 20 = (32, 8, 0), list 0 = (8, 0, 32): the same pictures at other indices
                n_ref = ((3, 3), (3, 2), (2, 3), (5, 4))[(k // 2) % 4] if kind == "B" else ((3, 3), (2, 2), (4, 4))[(k // 2) % 3]     # 3 pictures: 4 or 5 entries repeat them
                pics.append(random_pic(rng, seq, kind, 9 + k, n_ref, max_merge=mm, p_merge=0.75, p_skip=0.2, p_pcm=0.05,
                                       p_split=0.7, wide=6, layout=layout, is_ref=False))
                k += 1
        return seq, pics
    return build


def b2_at_four():
    """48x48, nine 16x16 CTBs in one slice.  The first 8x8 unit of the centre CTB merges with merge_idx 4 of five: A1 and A0 are the two 16x8 blocks of
    the CTB to the left, B1 and B0 the two 8x16 blocks of the CTB above, B2 the CTB above left, five motions that all differ -- four flags are set, so
    B2 is refused and index 4 is the first zero candidate (P) / the first combined one (B), not B2's motion."""
    rng = np.random.default_rng(0xB24)
    seq = base_seq(48, 48, ctb_log2=4)
    v = lambda idx, mvd: dict(l0=(idx, mvd, 0))
    one = lambda pu: dict(t="inter", part="2Nx2N", pus=[pu])
    target = dict(t="split", sub=[dict(t="skip", merge=4)] + [dict(t="skip", merge=0)] * 3)
    cus = [one(v(0, (-36, 20))), dict(t="inter", part="Nx2N", pus=[v(1, (44, 4)), v(0, (8, -28))]), one(v(0, (0, 0))),
           dict(t="inter", part="2NxN", pus=[v(0, (-12, -16)), v(1, (24, 60))]), target] + [one(v(0, (0, 0)))] * 4
    pics = [noise(rng, seq), noise(rng, seq, "P", 8), dict(kind="P", poc=2, layout="pic", max_merge=5, cus=cus, is_ref=False),
            dict(kind="B", poc=3, layout="pic", max_merge=5, cus=cus, is_ref=False)]
    return seq, pics


# ---- the motion vector predictor ------------------------------------------------------------------------------------------------------------------
def amvp():
    """Predicted units with four reference pictures (ref_idx 0 .. 3: two context bins and a bypass bin), both mvp flags, vector differences of 0, +-1,
    +-2 and up to +-32767 -- sums that wrap at 16 bits come by themselves --, a B picture with mvd_l1_zero_flag, lists that hold the same pictures at
    other indices (a neighbour that refers to the same picture through the other list), PCM units and slice edges that take neighbours away"""
    rng = np.random.default_rng(0xA3F9)
    seq = base_seq(96, 80, amp=1)
    pics = [noise(rng, seq)] + [random_pic(rng, seq, "P", 40 * k, (k, k), p_merge=0.1, p_skip=0.05, layout="pic") for k in (1, 2, 3)]
    k = 0
    for wide in (3, 40, 400, 32767):
        for kind in ("P", "B", "B"):
            pics.append(random_pic(rng, seq, kind, 41 + k, (4, 4) if k % 2 else (4, 3), p_merge=0.08, p_skip=0.04, p_pcm=0.08, wide=wide,
                                   layout=("pic", "row", "pic", "ctb")[k % 4], is_ref=False, mvd_l1_zero=1 if kind == "B" and k % 3 == 2 else 0))
            k += 1
    return seq, pics


# ---- the temporal candidate -----------------------------------------------------------------------------------------------------------------------
def tmvp(seed, low_delay):
    """sps_temporal_mvp_enabled_flag 1.  Collocated pictures: the all-intra first picture, P pictures and a B reference picture cut into 8x4 / 4x8 / 8x8
    units with vectors of their own (the 16x16 storage position decides), from list 0 and from list 1, collocated_ref_idx 0 and 1; one picture with the
    slice flag 0; POC distances from 1 to 100 and more (td and tb clipped, factors clipped both ways).  low_delay: every reference precedes the current
    picture (NoBackwardPredFlag 1)"""
    def build():
        rng = np.random.default_rng(seed)
        seq = base_seq(96, 80, amp=1, tmvp=1)
        # decode order; POC steps below 128 between reference pictures (8-bit POC LSB)
        pics = [noise(rng, seq),
                random_pic(rng, seq, "P", 100, (1, 1), p_merge=0.15, p_split=0.9, wide=300, layout="pic", max_merge=2),
                random_pic(rng, seq, "P", 200, (2, 2), p_merge=0.3, p_split=0.9, wide=300, layout="pic", max_merge=3, col=(1, 0)),
                random_pic(rng, seq, "B", 204 if low_delay else 150, (3, 3), p_merge=0.3, p_split=0.9, wide=200, layout="pic", max_merge=3, col=(0, 0), is_ref=True),
                random_pic(rng, seq, "B", 206 if low_delay else 151, (4, 4), p_merge=0.3, p_split=0.9, wide=900, layout="pic", max_merge=4, col=(1, 0), is_ref=True)]
        k = 0
        for kind in ("P", "B", "B", "P", "B", "B", "B", "P"):
            poc = 300 + k if low_delay else (152, 153, 160, 170, 180, 199, 201, 210)[k]
            n_ref = ((5, 5), (4, 2), (2, 4), (3, 3))[k % 4]
            col = (1, k % n_ref[0] % 2) if kind == "P" or k % 2 else (0, k // 2 % 2)
            pics.append(random_pic(rng, seq, kind, poc, n_ref, max_merge=(5, 2, 3)[k % 3], p_merge=0.45, p_skip=0.1, wide=(4, 60)[k % 2], col=col,
                                   layout=("pic", "pic", "row")[k % 3], is_ref=False, **({"tmvp": 0} if k == 6 else {})))
            k += 1
        return seq, pics
    return build


def tmvp_slices():
    """A collocated B picture of three slices (one per row of 32x32 CTBs) that activate (1, 1), (3, 3) and (2, 3) list entries: a block of the second
    or third slice with ref_idx 1 or 2 refers to a picture that the first slice's lists do not hold at that index.  The pictures behind it take their
    temporal candidates from it out of list 0 and out of list 1; the last one has slices with lists of their own itself."""
    rng = np.random.default_rng(0x7A12)
    seq = base_seq(96, 80, amp=1, tmvp=1)
    pics = [noise(rng, seq),
            random_pic(rng, seq, "P", 40, (1, 1), p_merge=0.15, p_split=0.9, wide=100, layout="pic", max_merge=2),
            random_pic(rng, seq, "P", 80, (2, 2), p_merge=0.3, p_split=0.9, wide=100, layout="pic", max_merge=3),
            random_pic(rng, seq, "B", 60, (3, 3), p_merge=0.15, p_skip=0.05, p_split=0.9, wide=100, layout="row", max_merge=3, is_ref=True,
                       slice_n_ref=[(1, 1), (3, 3), (2, 3)]),
            random_pic(rng, seq, "P", 61, (4, 4), p_merge=0.45, wide=8, layout="pic", max_merge=3, col=(1, 0), is_ref=False),
            random_pic(rng, seq, "B", 62, (4, 4), p_merge=0.45, wide=8, layout="row", max_merge=4, col=(1, 0), is_ref=False),
            random_pic(rng, seq, "B", 63, (4, 4), p_merge=0.45, wide=8, layout="pic", max_merge=5, col=(0, 1), is_ref=False),
            random_pic(rng, seq, "P", 64, (4, 4), p_merge=0.45, wide=8, layout="row", max_merge=3, col=(1, 0), is_ref=False,
                       slice_n_ref=[(4, 4), (2, 2), (1, 1)])]
    return seq, pics


PIN_VECTORS = [(-1, -129), (1, 129), (-32768, 32767), (300, -7), (-3, 2), (32767, -32768), (127, -128), (-640, 384)]


def scaling_pins():
    """Scripted vectors in the collocated picture and POC distances chosen for the corners of 8-179 - 8-183.  One 16x16 unit per CTB and one slice per
    CTB: the only candidates are the temporal one (mvp flag 0) and zeros, and every unit codes the vector difference (0, 0) or, in the collocated
    pictures (slice flag 0 or an all-intra collocated picture: predictor zero), its vector.  Decode order, POC, what RefPicList0 holds:
      0  I   0
      1  P   4  (0)              vectors PIN_VECTORS[a % 8] to POC 0: td 4                                       "A"
      2  B   2  l1 (4, 0)        slice flag 0; list 1 vectors to POC 4: td -2                                    "C"
      3  B   3  l1 (4, 2, 0)     collocated_from_l0_flag 0: A; list 1 ref_idx 0: tb -1, factor -64
      4  P   6  (4, 2, 0)        collocated A; ref_idx 0: tb 2, factor 128: -1 * 128 = -128 rounds to 0 in sign and magnitude, to -1 by a plain shift
      5  P   8  (4, 2, 0)        collocated A; ref_idx 0: tb 4 == td, ref_idx 2: tb 8, factor 512: +-32767 doubled are clipped
      6  P 100  (4, 2, 0)        collocated_ref_idx 1: C; ref_idx 0: tb 96, tx -8192: the factor clipped at -4096
      7  P 101  (100, 4, 2, 0)   collocated_ref_idx 1: A; ref_idx 2: tb 99, factor 6336 clipped at 4095; ref_idx 0: tb 1, factor 64
      8  P 227  (100, 4, 2, 0)   slice flag 0; vectors to POC 0: td 227                                          "D"
      9  P 300  (227, 100, ..)   collocated D; ref_idx 1: tb 200: both clipped to 127, factor 256 (td unclipped: 143)"""
    rng = np.random.default_rng(0x5CA1)
    seq = base_seq(96, 80, ctb_log2=4, tmvp=1)
    cw, ch = hw.ctb_dims(seq)

    def pic(kind, poc, col, unit, **kw):
        return dict(kind=kind, poc=poc, col=col, layout="ctb", cus=[unit(a) for a in range(cw * ch)], **kw)
    vec = lambda l, idx, shift=0: (lambda a: dict(t="inter", part="2Nx2N", pus=[{l: (idx, PIN_VECTORS[(a + shift) % 8], 0)}]))
    cand = lambda l, idxs: (lambda a: dict(t="inter", part="2Nx2N", pus=[{l: (idxs[(a // 8) % len(idxs)], (0, 0), 0)}]))
    pics = [noise(rng, seq),
            pic("P", 4, (1, 0), vec("l0", 0)),
            pic("B", 2, (1, 0), vec("l1", 0, 3), tmvp=0, is_ref=True),
            pic("B", 3, (0, 0), cand("l1", (0,)), is_ref=False),
            pic("P", 6, (1, 0), cand("l0", (0,)), is_ref=False),
            pic("P", 8, (1, 0), cand("l0", (0, 2)), is_ref=False),
            pic("P", 100, (1, 1), cand("l0", (0,))),
            pic("P", 101, (1, 1), cand("l0", (2, 0)), is_ref=False),
            pic("P", 227, (1, 0), vec("l0", 3, 5), tmvp=0),
            pic("P", 300, (1, 0), cand("l0", (1,)), is_ref=False)]
    return seq, pics


CASES = {
    "inter_shapes-default": shapes(0, 0x51A0),
    "inter_shapes-explicit": shapes(1, 0x51A1),
    "inter_fractions-default": fractions(0),
    "inter_fractions-explicit": fractions(1),
    "inter_borders-96x80": borders(96, 80),
    "inter_borders-86x70": borders(86, 70),
    "inter_borders-128x32": borders(128, 32),
    "inter_job_lists": job_lists,
    "inter_merge-level2": merge(2, 3, 0x3E20),
    "inter_merge-level3": merge(3, 3, 0x3E30, (3, 5, 5)),
    "inter_merge-level4": merge(4, 3, 0x3E40, (2, 4, 5, 5)),
    "inter_merge-nxn": merge(2, 4, 0x3E50, (2, 4, 5)),
    "inter_merge-b2_at_four": b2_at_four,
    "inter_amvp": amvp,
    "inter_tmvp-backward": tmvp(0x7A10, False),
    "inter_tmvp-low_delay": tmvp(0x7A11, True),
    "inter_tmvp-scaling": scaling_pins,
    "inter_tmvp-slices": tmvp_slices,
}
GROUPS = {
    "shapes": ["inter_shapes-default", "inter_shapes-explicit", "inter_fractions-default", "inter_fractions-explicit"],
    "borders": ["inter_borders-96x80", "inter_borders-86x70", "inter_borders-128x32"],
    "job_lists": ["inter_job_lists"],
    "merge": ["inter_merge-level2", "inter_merge-level3", "inter_merge-level4", "inter_merge-nxn", "inter_merge-b2_at_four"],
    "amvp": ["inter_amvp"],
    "tmvp": ["inter_tmvp-backward", "inter_tmvp-low_delay", "inter_tmvp-scaling", "inter_tmvp-slices"],
}
