"""Scripted VP8 inter frames on scripted_vp8's BoolEncoder: a stream writer that keeps what a decoder keeps from frame to frame (probabilities, the
macroblocks' vectors for the near-vector search, sign biases) and takes explicit header fields and per-macroblock references, modes and vectors, so
that every feature of RFC 6386 sections 9.7, 16, 17 and 18 can be put into a stream on purpose.  Tables, the near-vector search and the split context
are vp8_inter_ref's; nothing here reads the library's sources.

A macroblock is a dict.  Intra: as in scripted_vp8.key_frame (ymode, uvmode, bmodes, segment, skip, coefs).  Inter: ref (1 last, 2 golden, 3 altref),
mode (I.MV_ZERO .. I.MV_SPLIT), and for MV_NEW either mv=(row, col) -- the vector wanted, in eighth samples, even -- or delta=(row, col), the coded
difference in quarter samples; for MV_SPLIT split=kind and subs=[(leaf, mv-or-None) per partition] with mv for NEW4 given as delta=(row, col)."""
import random
import struct

import scripted_vp8 as S
import vp8_inter_ref as I
import vp8_ref as R
from scripted_vp8 import BoolEncoder


class _Nb:
    def __init__(self):
        self.ref, self.mv, self.split, self.bmv = 0, (0, 0), False, [(0, 0)] * 16


_OUTSIDE = _Nb()


def _write_mv_comp(e, p, x):
    a = abs(x)
    assert a <= 1023, x
    if a < 8:
        e.write(p[I.MV_IS_SHORT], 0)
        e.tree(I.SMALL_MV_TREE, p[I.MV_SHORT:I.MV_SHORT + 7], a)
    else:
        e.write(p[I.MV_IS_SHORT], 1)
        for i in range(3):
            e.write(p[I.MV_LONG + i], a >> i & 1)
        for i in range(I.MV_LONG_BITS - 1, 3, -1):
            e.write(p[I.MV_LONG + i], a >> i & 1)
        if a > 15:
            e.write(p[I.MV_LONG + 3], a >> 3 & 1)
    if a:
        e.write(p[I.MV_SIGN], 1 if x < 0 else 0)


class Stream:
    """The writer's side of one stream: key() and inter() return frames."""

    def __init__(self, width, height):
        self.w, self.h = width, height
        self.mbw, self.mbh = (width + 15) >> 4, (height + 15) >> 4
        self.coef = None

    def key(self, mbs, **kw):
        self.coef = [[[list(c) for c in b] for b in t] for t in R.DEFAULT_COEF_PROBS]
        if kw.get("refresh", 0):
            for (i, j, k, l), v in (kw.get("prob_updates") or {}).items():
                self.coef[i][j][k][l] = v
        self.mvp = [list(r) for r in I.DEFAULT_MV_PROBS]
        self.ymode_prob, self.uv_prob = list(I.YMODE_PROB), list(I.UV_MODE_PROB)
        self.sign_bias = [0, 0, 0, 0]
        return S.key_frame(self.w, self.h, mbs, **kw)

    def inter(self, mbs, version=0, show=1, segmentation=None, filter_type=0, level=0, sharpness=0, lf_delta=None, log2_parts=0, yac=40,
              q_deltas=(0, 0, 0, 0, 0), refresh_golden=0, refresh_alt=0, copy_gf=0, copy_arf=0, sign_bias=(0, 0), refresh_entropy=1, refresh_last=1,
              prob_updates=None, no_coeff_skip=1, prob_skip=128, prob_intra=128, prob_last=128, prob_gf=128, ymode_probs=None, uv_probs=None,
              mv_prob_updates=None, info=None):
        mbw, mbh = self.mbw, self.mbh
        assert len(mbs) == mbw * mbh and self.coef is not None
        e = BoolEncoder()
        seg = segmentation
        e.literal(1 if seg else 0, 1)
        seg_probs, update_map = [255] * 3, 0
        if seg:
            update_map = seg.get("update_map", 1)
            e.literal(update_map, 1)
            e.literal(seg.get("update_data", 1), 1)
            if seg.get("update_data", 1):
                e.literal(seg.get("abs", 0), 1)
                for v in seg.get("q", [0] * 4):
                    e.flagged(v, 7)
                for v in seg.get("lf", [0] * 4):
                    e.flagged(v, 6)
            if update_map:
                seg_probs = list(seg.get("probs", [128, 128, 128]))
                for p in seg_probs:
                    e.literal(1 if p != 255 else 0, 1)
                    if p != 255:
                        e.literal(p, 8)
        e.literal(filter_type, 1)
        e.literal(level, 6)
        e.literal(sharpness, 3)
        e.literal(1 if lf_delta else 0, 1)
        if lf_delta:
            e.literal(lf_delta.get("update", 1), 1)
            if lf_delta.get("update", 1):
                for v in list(lf_delta.get("ref", [None] * 4)) + list(lf_delta.get("mode", [None] * 4)):      # None: the delta keeps its value
                    e.literal(0 if v is None else 1, 1)
                    if v is not None:
                        e.literal(abs(v), 6)
                        e.literal(1 if v < 0 else 0, 1)
        e.literal(log2_parts, 2)
        e.literal(yac, 7)
        for v in q_deltas:
            e.flagged(v, 4)
        e.literal(refresh_golden, 1)
        e.literal(refresh_alt, 1)
        if not refresh_golden:
            e.literal(copy_gf, 2)
        if not refresh_alt:
            e.literal(copy_arf, 2)
        e.literal(sign_bias[0], 1)
        e.literal(sign_bias[1], 1)
        self.sign_bias[2], self.sign_bias[3] = sign_bias
        e.literal(refresh_entropy, 1)
        saved = None
        if not refresh_entropy:
            saved = ([[[list(c) for c in b] for b in t] for t in self.coef], [list(r) for r in self.mvp], list(self.ymode_prob), list(self.uv_prob))
        e.literal(refresh_last, 1)
        probs = self.coef
        prob_updates = prob_updates or {}
        for i in range(4):
            for j in range(8):
                for k in range(3):
                    for l in range(11):
                        up = prob_updates.get((i, j, k, l))
                        e.write(R.COEF_UPDATE_PROBS[i][j][k][l], 1 if up is not None else 0)
                        if up is not None:
                            e.literal(up, 8)
                            probs[i][j][k][l] = up
        e.literal(no_coeff_skip, 1)
        if no_coeff_skip:
            e.literal(prob_skip, 8)
        e.literal(prob_intra, 8)
        e.literal(prob_last, 8)
        e.literal(prob_gf, 8)
        e.literal(1 if ymode_probs else 0, 1)
        if ymode_probs:
            for v in ymode_probs:
                e.literal(v, 8)
            self.ymode_prob = list(ymode_probs)
        e.literal(1 if uv_probs else 0, 1)
        if uv_probs:
            for v in uv_probs:
                e.literal(v, 8)
            self.uv_prob = list(uv_probs)
        mv_prob_updates = mv_prob_updates or {}
        for i in range(2):
            for j in range(19):
                up = mv_prob_updates.get((i, j))
                e.write(I.MV_UPDATE_PROBS[i][j], 1 if up is not None else 0)
                if up is not None:
                    e.literal(up, 7)
                    self.mvp[i][j] = up << 1 if up else 1
        n_parts = 1 << log2_parts
        toks = [BoolEncoder() for _i in range(n_parts)]
        above_nz = [[0] * 9 for _i in range(mbw)]
        cats = set()
        grid = {}
        for my in range(mbh):
            ln = [0] * 9
            t = toks[my % n_parts]
            for mx in range(mbw):
                m = mbs[my * mbw + mx]
                coefs = m.get("coefs", {})
                skip = 1 if (no_coeff_skip and m.get("skip", not coefs)) else 0
                assert not (skip and coefs)
                if update_map:
                    e.tree(R.SEGMENT_TREE, seg_probs, m.get("segment", 0))
                if no_coeff_skip:
                    e.write(prob_skip, skip)
                nb = _Nb()
                grid[(mx, my)] = nb
                ref = m.get("ref", 0)
                e.write(prob_intra, 1 if ref else 0)
                if ref:
                    e.write(prob_last, 0 if ref == 1 else 1)
                    if ref != 1:
                        e.write(prob_gf, ref - 2)
                    A, L, AL = grid.get((mx, my - 1), _OUTSIDE), grid.get((mx - 1, my), _OUTSIDE), grid.get((mx - 1, my - 1), _OUTSIDE)
                    best, nearest, nearby, cnt = I.near_search(A, L, AL, ref, self.sign_bias, mx, my, mbw, mbh)
                    mode = m.get("mode", I.MV_ZERO)
                    e.tree(I.MV_REF_TREE, [I.MODE_CONTEXTS[cnt[i]][i] for i in range(4)], mode)

                    def write_mv(spec):
                        if "mv" in spec:
                            dr, dc = spec["mv"][0] - best[0], spec["mv"][1] - best[1]
                            assert dr % 2 == 0 and dc % 2 == 0, (spec, best)
                            dr, dc = dr // 2, dc // 2
                        else:
                            dr, dc = spec.get("delta", (0, 0))
                        _write_mv_comp(e, self.mvp[0], dr)
                        _write_mv_comp(e, self.mvp[1], dc)
                        return (R.s16(best[0] + 2 * dr), R.s16(best[1] + 2 * dc))
                    nb.ref = ref
                    if mode == I.MV_SPLIT:
                        kind = m["split"]
                        e.tree(I.SPLIT_TREE, I.SPLIT_PROBS, kind)
                        bmv = [(0, 0)] * 16
                        subs = m["subs"]
                        assert len(subs) == I.SPLIT_COUNT[kind]
                        for j, (leaf, spec) in enumerate(subs):
                            b0 = I.SPLITS[kind].index(j)
                            lm = bmv[b0 - 1] if b0 & 3 else L.bmv[b0 + 3]
                            am = bmv[b0 - 4] if b0 >> 2 else A.bmv[b0 + 12]
                            e.tree(I.SUB_MV_REF_TREE, I.SUB_MV_REF_PROBS[I.sub_mv_context(lm, am)], leaf)
                            v = lm if leaf == I.LEFT4 else am if leaf == I.ABOVE4 else (0, 0) if leaf == I.ZERO4 else write_mv(spec or {})
                            for b in range(16):
                                if I.SPLITS[kind][b] == j:
                                    bmv[b] = v
                        nb.bmv, nb.mv, nb.split = bmv, bmv[15], True
                    else:
                        nb.mv = (0, 0) if mode == I.MV_ZERO else nearest if mode == I.MV_NEAREST else nearby if mode == I.MV_NEAR else write_mv(m)
                        nb.bmv = [nb.mv] * 16
                    has_y2 = mode != I.MV_SPLIT
                else:
                    ymode = m.get("ymode", R.DC_PRED)
                    e.tree(I.YMODE_TREE, self.ymode_prob, ymode)
                    if ymode == R.B_PRED:
                        for b in m["bmodes"]:
                            e.tree(R.BMODE_TREE, I.BMODE_PROB, b)
                    e.tree(R.UV_MODE_TREE, self.uv_prob, m.get("uvmode", R.DC_PRED))
                    has_y2 = ymode != R.B_PRED
                an = above_nz[mx]
                if skip:
                    ka, kl = an[8], ln[8]
                    an[:] = [0] * 9
                    ln[:] = [0] * 9
                    if not has_y2:
                        an[8], ln[8] = ka, kl
                    continue
                zero = [0] * 16
                first = 0
                if has_y2:
                    an[8] = ln[8] = S._write_block(t, probs[1], an[8] + ln[8], 0, coefs.get(24, zero), cats)
                    first = 1
                else:
                    assert 24 not in coefs
                for b in range(16):
                    lv = coefs.get(b, zero)
                    assert not (first and lv[0])
                    an[b & 3] = ln[b >> 2] = S._write_block(t, probs[0 if first else 3], an[b & 3] + ln[b >> 2], first, lv, cats)
                for c in range(2):
                    for b in range(4):
                        ia, il = 4 + 2 * c + (b & 1), 4 + 2 * c + (b >> 1)
                        an[ia] = ln[il] = S._write_block(t, probs[2], an[ia] + ln[il], 0, coefs.get(16 + 4 * c + b, zero), cats)
        if saved is not None:
            self.coef, self.mvp, self.ymode_prob, self.uv_prob = saved
        if info is not None:
            info.setdefault("cats", set()).update(cats)
        first_part = e.finish()
        parts = [t.finish() for t in toks]
        tag = 1 | version << 1 | show << 4 | len(first_part) << 5
        out = struct.pack("<I", tag)[:3] + first_part
        for p in parts[:-1]:
            out += struct.pack("<I", len(p))[:3]
        return out + b"".join(parts)


def _coefs(rnd, density, has_y2, big=False):
    coefs = {}
    for b in list(range(24)) + ([24] if has_y2 else []):
        if rnd.random() < density:
            lv = [0] * 16
            for _k in range(rnd.randrange(1, 5)):
                i = min(15, int(rnd.expovariate(0.4)))
                lv[i] = rnd.choice((-1, 1)) * (rnd.randrange(1, 2000 if big else 12) if rnd.random() < 0.3 else 1)
            if b < 16 and has_y2:
                lv[0] = 0
            if any(lv):
                coefs[b] = lv
    return coefs


def random_inter_mbs(width, height, seed, intra=0.15, split=0.3, density=0.2, skip=0.2, refs=(1, 2, 3), far=0.05, segments=1):
    """Random inter macroblocks (and some intra ones) for every macroblock of a picture."""
    rnd = random.Random(seed)
    mbw, mbh = (width + 15) >> 4, (height + 15) >> 4

    def delta():
        if rnd.random() < far:
            return (rnd.randrange(-1023, 1024), rnd.randrange(-1023, 1024))
        return (rnd.randrange(-24, 25), rnd.randrange(-24, 25))
    out = []
    for _i in range(mbw * mbh):
        m = dict(segment=rnd.randrange(segments))
        if rnd.random() < intra:
            m.update(uvmode=rnd.randrange(4))
            if rnd.random() < 0.4:
                m.update(ymode=R.B_PRED, bmodes=[rnd.randrange(10) for _k in range(16)])
            else:
                m.update(ymode=rnd.randrange(4))
            has_y2 = m["ymode"] != R.B_PRED
        else:
            m.update(ref=rnd.choice(refs))
            if rnd.random() < split:
                kind = rnd.randrange(4)
                subs = []
                for _j in range(I.SPLIT_COUNT[kind]):
                    leaf = rnd.randrange(4)
                    subs.append((leaf, dict(delta=delta()) if leaf == I.NEW4 else None))
                m.update(mode=I.MV_SPLIT, split=kind, subs=subs)
                has_y2 = False
            else:
                m.update(mode=rnd.choice((I.MV_ZERO, I.MV_NEAREST, I.MV_NEAR, I.MV_NEW, I.MV_NEW)), delta=delta())
                has_y2 = True
        if rnd.random() >= skip:
            c = _coefs(rnd, density, has_y2)
            if c:
                m["coefs"] = c
        out.append(m)
    return out


def sized_stream(width, height, seed=1, frames=3, version=0, **hdr):
    """A key frame and `frames` random inter frames of one size; golden and altref are refreshed along the way, the filter filters."""
    st = Stream(width, height)
    kw = dict(level=20, sharpness=0, yac=30)
    kw.update(hdr)
    out = [st.key(S.random_mbs(width, height, seed * 1000), version=version, **kw)]
    for i in range(frames):
        out.append(st.inter(random_inter_mbs(width, height, seed * 1000 + 1 + i), version=version, refresh_golden=1 if i == 0 else 0,
                            refresh_alt=1 if i == 1 else 0, sign_bias=(i & 1, (i >> 1) & 1), **kw))
    return R.ivf(out, width, height)


SIZES = [(16, 16), (48, 32), (53, 37), (272, 16), (16, 272), (80, 272)]


def _flat_key(st, value_seed, **kw):
    """a key frame with texture: random modes and coefficients"""
    return st.key(S.random_mbs(st.w, st.h, value_seed, density=0.4, skip=0.0), **kw)


def zero_mbs(n, ref):
    return [dict(ref=ref, mode=I.MV_ZERO) for _i in range(n)]


def new_mbs(n, ref, mv):
    return [dict(ref=ref, mode=I.MV_NEW, mv=mv) for _i in range(n)]


def fraction_stream(version=0):
    """64 x 64: four inter frames whose 64 macroblocks take the 64 chroma fraction pairs (and with them all 16 luma ones), each from the key frame"""
    st = Stream(64, 64)
    out = [_flat_key(st, 300, yac=10, version=version)]
    for f in range(4):
        mbs = []
        for i in range(16):
            k = f * 16 + i
            mbs.append(dict(ref=2, mode=I.MV_NEW, mv=(2 * (k >> 3) + 16 * (i & 1), 2 * (k & 7) - 16 * (i >> 3))))
        out.append(st.inter(mbs, version=version, yac=10))
    return R.ivf(out, 64, 64)


def far_stream():
    """vectors of the largest coded magnitude in all four directions (255.75 samples: more than a whole 48 x 32 picture beyond every border)"""
    st = Stream(48, 32)
    out = [_flat_key(st, 310, yac=10)]
    far = [(1023, 1023), (-1023, -1023), (1023, -1023), (-1023, 1023), (-1023, 0), (0, 1023)]
    out.append(st.inter([dict(ref=1, mode=I.MV_NEW, delta=far[i]) for i in range(6)], yac=10, level=10))
    # split macroblocks with far sub-block vectors, and sums that wrap 16 bits: NEW on top of a best vector that is already at the clamp
    mbs = []
    for i in range(6):
        mbs.append(dict(ref=1, mode=I.MV_SPLIT, split=I.SPLIT_4x4, subs=[(I.NEW4, dict(delta=far[(i + j) % 6])) for j in range(16)]))
    out.append(st.inter(mbs, yac=10, level=10))
    return R.ivf(out, 48, 32)


def sub_mv_stream():
    """every sub_mv_ref leaf in each of its five contexts: 4x4 splits whose left / above vectors are arranged on purpose"""
    st = Stream(48, 32)
    out = [_flat_key(st, 320, yac=10)]
    rnd = random.Random(321)
    for f in range(6):
        mbs = []
        for i in range(6):
            kind = (f + i) % 4 if f < 2 else I.SPLIT_4x4
            subs = []
            for j in range(I.SPLIT_COUNT[kind]):
                leaf = rnd.choice((I.LEFT4, I.ABOVE4, I.ZERO4, I.NEW4, I.NEW4))
                subs.append((leaf, dict(delta=rnd.choice(((0, 0), (1, 0), (0, 1), (3, -2), (1, 0)))) if leaf == I.NEW4 else None))
            mbs.append(dict(ref=1 + (i + f) % 3, mode=I.MV_SPLIT, split=kind, subs=subs))
        out.append(st.inter(mbs, yac=10, level=12, refresh_golden=1 if f == 0 else 0, refresh_alt=1 if f == 1 else 0))
    return R.ivf(out, 48, 32)


def intra_beside_inter_stream():
    """intra macroblocks of every 16x16 mode and every sub-block mode beside inter neighbours"""
    st = Stream(48, 32)
    out = [_flat_key(st, 330, yac=10)]
    for f in range(5):
        mbs = []
        for i in range(6):
            if (i + f) & 1:
                mbs.append(dict(ref=1, mode=I.MV_NEW, delta=(f - 2, i - 3), coefs={3: [0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]}))
            elif f < 4:
                mbs.append(dict(ymode=f, uvmode=(f + i) % 4, coefs={24: [7] + [0] * 15}))
            else:
                mbs.append(dict(ymode=R.B_PRED, uvmode=i % 4, bmodes=[(i * 16 + k) % 10 for k in range(16)], coefs={5: [3, -2] + [0] * 14}))
        out.append(st.inter(mbs, yac=10, level=16))
    return R.ivf(out, 48, 32)


def filter_stream():
    """the filter levels either side of the inter-frame thresholds, and each reference class and mode class of the deltas"""
    st = Stream(48, 32)
    out = [_flat_key(st, 340, yac=40, level=30)]
    for f, lvl in enumerate((14, 15, 19, 20, 39, 40)):
        out.append(st.inter(random_inter_mbs(48, 32, 342 + f, density=0.5, skip=0.0, far=0.0), yac=60, level=lvl, refresh_golden=1 if f == 0 else 0,
                            refresh_alt=1 if f == 1 else 0))
    # deltas: set once, kept by a frame that has them on without an update, changed one at a time by a third
    mbs = random_inter_mbs(48, 32, 350, density=0.4, skip=0.0, far=0.0, intra=0.3)
    out.append(st.inter(mbs, yac=60, level=24, lf_delta=dict(ref=[6, -4, 9, -9], mode=[5, -3, 4, 12])))
    out.append(st.inter(random_inter_mbs(48, 32, 351, density=0.4, intra=0.3), yac=60, level=24, lf_delta=dict(update=0)))
    out.append(st.inter(random_inter_mbs(48, 32, 352, density=0.4, intra=0.3), yac=60, level=24, lf_delta=dict(ref=[None, 20, None, None], mode=[None, None, -20, None])))
    out.append(st.inter(random_inter_mbs(48, 32, 353, density=0.4, intra=0.3), yac=60, level=24))      # deltas off: they do not apply
    return R.ivf(out, 48, 32)


def entropy_stream():
    """refresh_entropy_probs 0: frame 1 updates coefficient, vector and mode probabilities for itself only; frame 2's tokens, vectors and modes
    parse only under the probabilities from before frame 1.  Frame 3 updates with refresh 1 and frame 4 depends on that."""
    st = Stream(48, 32)
    out = [_flat_key(st, 360, yac=20)]
    ups = {(0, 1, 0, 0): 3, (1, 0, 0, 0): 250, (2, 0, 0, 1): 240, (3, 0, 1, 2): 5, (0, 2, 1, 1): 7, (2, 1, 0, 0): 200}
    mvu = {(0, 0): 5, (1, 0): 120, (0, 2): 1, (1, 9): 0, (0, 1): 100}
    kw = dict(yac=20, level=10)
    out.append(st.inter(random_inter_mbs(48, 32, 361, density=0.5, skip=0.0), refresh_entropy=0, prob_updates=ups, mv_prob_updates=mvu,
                        ymode_probs=[10, 200, 30, 220], uv_probs=[240, 20, 128], **kw))
    out.append(st.inter(random_inter_mbs(48, 32, 362, density=0.5, skip=0.0), **kw))
    out.append(st.inter(random_inter_mbs(48, 32, 363, density=0.5, skip=0.0), refresh_entropy=1, prob_updates=ups, mv_prob_updates=mvu,
                        ymode_probs=[10, 200, 30, 220], uv_probs=[240, 20, 128], **kw))
    out.append(st.inter(random_inter_mbs(48, 32, 364, density=0.5, skip=0.0), **kw))
    return R.ivf(out, 48, 32)


def reference_stream():
    """Frames: 0 key K0; 1 inter P1 (random, refresh last only); 2 ZERO from golden (= K0); 3 ZERO from altref (= K0); 4 random P4 becomes golden,
    refresh_last 0; 5 ZERO from last (= frame 3's picture = K0, as frame 4 did not become last); 6 ZERO from golden (= P4); 7 copy golden -> altref,
    random from last; 8 ZERO from altref (= P4); 9 copy last -> golden (last = frame 8's picture); 10 ZERO from golden; 11 copy altref -> golden, copy
    last -> altref; 12 ZERO golden (= P4); 13 ZERO altref (= frame 10's picture).  expected(): which earlier frame each ZERO frame must equal."""
    st = Stream(48, 32)
    n = 6
    kw = dict(yac=16, level=0)
    f = [_flat_key(st, 370, yac=16, level=0)]
    f.append(st.inter(random_inter_mbs(48, 32, 371, refs=(1,), density=0.4), **kw))
    f.append(st.inter(zero_mbs(n, 2), **kw))
    f.append(st.inter(zero_mbs(n, 3), sign_bias=(0, 1), **kw))
    f.append(st.inter(random_inter_mbs(48, 32, 372, density=0.4), refresh_golden=1, refresh_last=0, sign_bias=(1, 0), **kw))
    f.append(st.inter(zero_mbs(n, 1), **kw))
    f.append(st.inter(zero_mbs(n, 2), sign_bias=(1, 1), **kw))
    f.append(st.inter(random_inter_mbs(48, 32, 373, refs=(1,), density=0.4), copy_arf=2, **kw))
    f.append(st.inter(zero_mbs(n, 3), **kw))
    f.append(st.inter(random_inter_mbs(48, 32, 374, refs=(1, 3), density=0.4), copy_gf=1, **kw))
    f.append(st.inter(zero_mbs(n, 2), **kw))
    f.append(st.inter(random_inter_mbs(48, 32, 375, refs=(1,), density=0.4), copy_gf=2, copy_arf=1, **kw))
    f.append(st.inter(zero_mbs(n, 2), **kw))
    f.append(st.inter(zero_mbs(n, 3), **kw))
    return R.ivf(f, 48, 32)


REFERENCE_EXPECTED = {2: 0, 3: 0, 5: 0, 6: 4, 8: 4, 10: 8, 12: 4, 13: 10}      # ZERO frame -> the frame it must equal (frame 8 = P4, so 10 = P4 too)


def long_golden_stream(frames=45):
    """48 x 32, `frames` frames: golden is the key frame 0 until the key frame in the middle, then that one; the last frame is ZERO from golden.  One
    hidden altref on the way."""
    st = Stream(48, 32)
    kw = dict(yac=24, level=12)
    mid = frames // 2
    out = []
    for i in range(frames):
        if i == 0 or i == mid:
            out.append(_flat_key(st, 380 + i, **kw))
        elif i == frames - 1 or i == mid - 1:
            out.append(st.inter(zero_mbs(6, 2), **kw))
        elif i == 5:
            out.append(st.inter(random_inter_mbs(48, 32, 380 + i, refs=(1,)), show=0, refresh_alt=1, refresh_last=0, **kw))
        else:
            out.append(st.inter(random_inter_mbs(48, 32, 380 + i, refs=(1, 1, 3)), **kw))
    return R.ivf(out, 48, 32)


def segment_stream():
    """a key frame sets the segment map; inter frames keep it (segmentation on, no map update; then off; then on again with new data)"""
    st = Stream(48, 32)
    seg = dict(abs=0, q=[0, -20, 15, 60], lf=[0, -10, 20, 30], probs=[100, 150, 200])
    out = [st.key(S.random_mbs(48, 32, 390, segments=4), segmentation=seg, yac=30, level=20)]
    out.append(st.inter(random_inter_mbs(48, 32, 391), segmentation=dict(update_map=0, update_data=0), yac=30, level=20))
    out.append(st.inter(random_inter_mbs(48, 32, 392), yac=30, level=20))
    out.append(st.inter(random_inter_mbs(48, 32, 393), segmentation=dict(update_map=0, abs=1, q=[5, 50, 100, 127], lf=[3, 13, 33, 63]), yac=30, level=20))
    out.append(st.inter(random_inter_mbs(48, 32, 394, segments=4), segmentation=dict(update_data=0, probs=[50, 255, 90]), yac=30, level=20))
    return R.ivf(out, 48, 32)


def feature_cases():
    """[(name, stream)]: IVF byte streams."""
    cases = [("version_%d" % v, sized_stream(48, 32, seed=400 + v, version=v, filter_type=1 if v else 0)) for v in range(4)]
    cases += [("fractions_v%d" % v, fraction_stream(v)) for v in (0, 1)]
    cases += [("far_vectors", far_stream()), ("sub_mv_refs", sub_mv_stream()), ("intra_beside_inter", intra_beside_inter_stream()),
              ("filter_levels_and_deltas", filter_stream()), ("refresh_entropy_0", entropy_stream()), ("references", reference_stream()),
              ("segment_map_kept", segment_stream())]
    st = Stream(48, 144)
    cases.append(("partitions_4", R.ivf([st.key(S.random_mbs(48, 144, 410), log2_parts=2, level=10, yac=30)] +
                                         [st.inter(random_inter_mbs(48, 144, 411 + i), log2_parts=2, level=10, yac=30) for i in range(2)], 48, 144)))
    st = Stream(48, 32)
    cases.append(("big_levels", R.ivf([_flat_key(st, 420, yac=100)] + [st.inter([dict(m, coefs=_coefs(random.Random(421 + k), 0.5, m.get("mode") != I.MV_SPLIT and m.get("ymode") != R.B_PRED, big=True))
                                                                                  for k, m in enumerate(random_inter_mbs(48, 32, 422, skip=1.0))], yac=100, level=20, no_coeff_skip=0)], 48, 32)))
    return cases


def damaged_cases():
    """[(name, stream)]: every picture decodes, deterministically, and the damaged ones count in errors."""
    w, h = 48, 32
    st = Stream(w, h)
    k = _flat_key(st, 430, yac=20, level=15)
    f = st.inter(random_inter_mbs(w, h, 431, density=0.5, skip=0.0), yac=20, level=15, log2_parts=1)
    g = st.inter(random_inter_mbs(w, h, 432), yac=20, level=15)
    part1 = (f[0] | f[1] << 8 | f[2] << 16) >> 5
    garbage = bytes(random.Random(433).randrange(256) for _i in range(400))
    return [("truncated_tokens", R.ivf([k, f[:len(f) - len(f) // 4], g], w, h)),
            ("truncated_first_partition", R.ivf([k, f[:3 + part1 // 2], g], w, h)),
            ("header_only", R.ivf([k, f[:3], g], w, h)),
            ("garbage_after_tag", R.ivf([k, f[:3] + garbage, g], w, h)),
            ("garbage_vectors", R.ivf([k, f[:3 + 12] + garbage[:200], g], w, h))]
