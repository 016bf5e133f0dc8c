"""Scripted VP8 key frames: a bool encoder (RFC 6386 7.3) and a frame writer that takes explicit header fields, per-macroblock modes and coefficient
levels, so that every syntax feature can be put into a stream on purpose.  The writer keeps the decoder's contexts (sub-block modes above / left,
non-zero flags) and codes with the RFC's trees and default probabilities; tables and trees are vp8_ref's.  Nothing here reads the library's sources.

feature_cases() holds one stream per feature that the libwebp fixtures (tests/golden/vp8) do not reach -- the README there has the list -- and the
streams the GPU and host tests share: sized_stream, the damaged streams, a size change, an inter frame behind a key frame."""
import random
import struct

import vp8_ref as R


_PATHS = {}      # (tree, leaf) -> the branches from the root; the trees are vp8_ref's module-level lists


class BoolEncoder:
    """The code word is the low end of the final interval, kept as one big integer: 8 bits of range register in front of one bit per shift."""

    def __init__(self):
        self.low, self.range, self.shifts = 0, 255, 0

    def write(self, prob, bit):
        split = 1 + (((self.range - 1) * prob) >> 8)
        if bit:
            self.low += split
            self.range -= split
        else:
            self.range = split
        while self.range < 128:
            self.range <<= 1
            self.low <<= 1
            self.shifts += 1

    def literal(self, v, n):
        for i in range(n - 1, -1, -1):
            self.write(128, v >> i & 1)

    def flagged(self, v, n, force=False):
        """an optional signed value: flag, magnitude, sign (force: the flag is set even for 0)"""
        if v == 0 and not force:
            self.write(128, 0)
            return
        self.write(128, 1)
        self.literal(abs(v), n)
        self.write(128, 1 if v < 0 else 0)

    def tree(self, tree, probs, leaf, start=0):
        key = (id(tree), leaf)
        steps = _PATHS.get(key)
        if steps is None:
            def path(i):
                for b in (0, 1):
                    t = tree[i + b]
                    if t <= 0:
                        if -t == leaf:
                            return [(i, b)]
                    else:
                        p = path(t)
                        if p is not None:
                            return [(i, b)] + p
                return None
            steps = _PATHS[key] = path(0)
            assert steps is not None, leaf
        for i, b in steps:
            if i >= start:
                self.write(probs[i >> 1], b)

    def finish(self):
        bits = 8 + self.shifts
        n = (bits + 7) // 8
        return (self.low << (8 * n - bits)).to_bytes(n, "big") + b"\x00\x00"      # (two spare bytes: the decoder's look-ahead stays inside)


def _write_block(e, probs, ctx, first, levels, cats):
    """levels: 16 values in zig-zag order -> the tokens; returns 1 when any token but end-of-block was written"""
    last = max([i for i in range(first, 16) if levels[i]], default=first - 1)
    i, start = first, 0
    while i < 16:
        p = probs[R.COEF_BANDS[i]][ctx]
        if i > last:
            e.tree(R.COEF_TREE, p, R.DCT_EOB, start)
            break
        v = abs(levels[i])
        if v == 0:
            e.tree(R.COEF_TREE, p, R.DCT_0, start)
            ctx, start = 0, 2
            i += 1
            continue
        if v <= 4:
            e.tree(R.COEF_TREE, p, v, start)
        else:
            c = max(k for k in range(6) if v >= R.CAT_BASE[k])
            assert v < R.CAT_BASE[c] + (1 << len(R.CAT_PROBS[c])), v
            e.tree(R.COEF_TREE, p, R.DCT_CAT1 + c, start)
            extra, n = v - R.CAT_BASE[c], len(R.CAT_PROBS[c])
            for k, pr in enumerate(R.CAT_PROBS[c]):
                e.write(pr, extra >> (n - 1 - k) & 1)
            cats.add(c + 1)
        e.write(128, 1 if levels[i] < 0 else 0)
        ctx, start = (1 if v == 1 else 2), 0
        i += 1
    return 1 if i > first or last >= first else 0


def key_frame(width, height, mbs, version=0, show=1, color_space=0, clamping=0, hscale=0, vscale=0, segmentation=None, filter_type=0, level=0,
              sharpness=0, lf_delta=None, log2_parts=0, yac=40, q_deltas=(0, 0, 0, 0, 0), refresh=0, prob_updates=None, no_coeff_skip=1, prob_skip=128,
              key=True, start_code=b"\x9d\x01\x2a", info=None):
    """mbs: per macroblock in raster order a dict(ymode, uvmode, bmodes (B_PRED), segment, skip, coefs {block: 16 levels in zig-zag order}); blocks
    0..15 luma, 16..19 U, 20..23 V, 24 Y2.  segmentation: dict(update_map, update_data, abs, q[4], lf[4], probs[3]); lf_delta: dict(update, ref[4], mode[4]);
    prob_updates: {(i, j, k, l): prob}."""
    mbw, mbh = (width + 15) >> 4, (height + 15) >> 4
    assert len(mbs) == mbw * mbh
    e = BoolEncoder()
    e.literal(color_space, 1)
    e.literal(clamping, 1)
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
            for v in lf_delta.get("ref", [0] * 4):
                e.flagged(v, 6, force=True)
            for v in lf_delta.get("mode", [0] * 4):
                e.flagged(v, 6)
    e.literal(log2_parts, 2)
    e.literal(yac, 7)
    for v in q_deltas:
        e.flagged(v, 4)
    e.literal(refresh, 1)
    probs = [[[list(c) for c in b] for b in t] for t in R.DEFAULT_COEF_PROBS]
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
    n_parts = 1 << log2_parts
    toks = [BoolEncoder() for _i in range(n_parts)]
    above_b = [[R.B_DC_PRED] * 4 for _i in range(mbw)]
    above_nz = [[0] * 9 for _i in range(mbw)]
    cats = set()
    for my in range(mbh):
        left_b, ln = [R.B_DC_PRED] * 4, [0] * 9
        t = toks[my % n_parts]
        for mx in range(mbw):
            m = mbs[my * mbw + mx]
            ymode, coefs = m.get("ymode", R.DC_PRED), m.get("coefs", {})
            skip = 1 if (no_coeff_skip and m.get("skip", not coefs)) else 0
            assert not (skip and coefs)
            if update_map:
                e.tree(R.SEGMENT_TREE, seg_probs, m.get("segment", 0))
            if no_coeff_skip:
                e.write(prob_skip, skip)
            e.tree(R.KF_YMODE_TREE, R.KF_YMODE_PROB, ymode)
            if ymode == R.B_PRED:
                bm = list(m["bmodes"])
                for b in range(16):
                    A = above_b[mx][b & 3] if b < 4 else bm[b - 4]
                    L = left_b[b >> 2] if not (b & 3) else bm[b - 1]
                    e.tree(R.BMODE_TREE, R.KF_BMODE_PROBS[A][L], bm[b])
            else:
                bm = [R.IMPLIED_BMODE[ymode]] * 16
            above_b[mx], left_b = bm[12:16], bm[3::4]
            e.tree(R.UV_MODE_TREE, R.KF_UV_MODE_PROB, m.get("uvmode", R.DC_PRED))
            an = above_nz[mx]
            if skip:
                ka, kl = an[8], ln[8]
                an[:] = [0] * 9
                ln[:] = [0] * 9
                if ymode == R.B_PRED:
                    an[8], ln[8] = ka, kl
                continue
            zero = [0] * 16
            first = 0
            if ymode != R.B_PRED:
                an[8] = ln[8] = _write_block(t, probs[1], an[8] + ln[8], 0, coefs.get(24, zero), cats)
                first = 1
            else:
                assert 24 not in coefs
            for b in range(16):
                lv = coefs.get(b, zero)
                assert not (first and lv[0])
                an[b & 3] = ln[b >> 2] = _write_block(t, probs[0 if first else 3], an[b & 3] + ln[b >> 2], first, lv, cats)
            for c in range(2):
                for b in range(4):
                    ia, il = 4 + 2 * c + (b & 1), 4 + 2 * c + (b >> 1)
                    an[ia] = ln[il] = _write_block(t, probs[2], an[ia] + ln[il], 0, coefs.get(16 + 4 * c + b, zero), cats)
    if info is not None:
        info.setdefault("cats", set()).update(cats)
    first_part = e.finish()
    parts = [t.finish() for t in toks]
    tag = (0 if key else 1) | version << 1 | show << 4 | len(first_part) << 5
    out = struct.pack("<I", tag)[:3]
    if key:
        out += start_code + struct.pack("<HH", width | hscale << 14, height | vscale << 14)
    out += first_part
    for p in parts[:-1]:
        out += struct.pack("<I", len(p))[:3]
    return out + b"".join(parts)


ALL_BMODES = list(range(10))


def random_mbs(width, height, seed, density=0.25, bpred=0.4, skip=0.15, segments=1, big=False):
    """Random modes and sparse levels for every macroblock of a picture."""
    rnd = random.Random(seed)
    mbw, mbh = (width + 15) >> 4, (height + 15) >> 4
    out = []
    for _i in range(mbw * mbh):
        m = dict(uvmode=rnd.randrange(4), segment=rnd.randrange(segments))
        if rnd.random() < bpred:
            m.update(ymode=R.B_PRED, bmodes=[rnd.randrange(10) for _k in range(16)])
        else:
            m.update(ymode=rnd.randrange(4))
        if rnd.random() >= skip:
            coefs = {}
            blocks = list(range(24)) + ([24] if m["ymode"] != R.B_PRED else [])
            for b in blocks:
                if rnd.random() < density:
                    lv = [0] * 16
                    for _k in range(rnd.randrange(1, 5)):
                        i = min(15, int(rnd.expovariate(0.4)))
                        lv[i] = rnd.choice((-1, 1)) * (rnd.randrange(1, 2000 if big else 12) if rnd.random() < 0.3 else 1)
                    if b < 16 and m["ymode"] != R.B_PRED:
                        lv[0] = 0
                    if any(lv):
                        coefs[b] = lv
            if coefs:
                m["coefs"] = coefs
        out.append(m)
    return out


def sized_stream(width, height, seed=1, frames=1, **hdr):
    """An IVF stream of `frames` random key frames of one size, normal loop filter at a level that filters."""
    kw = dict(level=20, sharpness=0, yac=30)
    kw.update(hdr)
    return R.ivf([key_frame(width, height, random_mbs(width, height, seed * 1000 + i, segments=4 if kw.get("segmentation") else 1), **kw) for i in range(frames)],
                 width, height)


SIZES = [(16, 16), (48, 32), (53, 37), (272, 16), (16, 272), (80, 272)]


def _corner_modes():
    """every sub-block mode at a picture corner, in the top row and in the left column: 10 pictures of 2 x 2 macroblocks, all B_PRED with one mode"""
    out = []
    for mode in ALL_BMODES:
        mbs = random_mbs(32, 32, 50 + mode, bpred=1.0, skip=0.0)
        for m in mbs:
            m["bmodes"] = [mode] * 16
        out.append(key_frame(32, 32, mbs, level=12, yac=20))
    return R.ivf(out, 32, 32)


def feature_cases():
    """[(name, stream)]: streams are IVF byte streams."""
    w, h = 48, 32
    cases = []

    def one(name, seed, mbs=None, **kw):
        kw.setdefault("level", 18)
        kw.setdefault("yac", 24)
        cases.append((name, R.ivf([key_frame(w, h, mbs or random_mbs(w, h, seed, segments=4 if kw.get("segmentation") else 1), **kw)], w, h)))
    for lp in (1, 2, 3):
        cases.append(("partitions_%d" % (1 << lp), R.ivf([key_frame(48, 144, random_mbs(48, 144, 10 + lp), log2_parts=lp, level=10, yac=30)], 48, 144)))
    one("simple_filter", 20, filter_type=1, level=30)
    one("simple_filter_sharp", 21, filter_type=1, level=44, sharpness=5, version=1)
    one("segments_delta", 22, segmentation=dict(abs=0, q=[0, -20, 15, 60], lf=[0, -10, 20, 40], probs=[100, 150, 200]))
    one("segments_absolute", 23, segmentation=dict(abs=1, q=[4, 40, 90, 127], lf=[0, 12, 33, 63], probs=[120, 255, 60]))
    one("segments_map_only", 24, segmentation=dict(update_data=0, probs=[90, 90, 90]))
    one("segments_no_map", 25, segmentation=dict(update_map=0, abs=1, q=[55, 1, 2, 3], lf=[25, 1, 2, 3]))
    one("no_coeff_skip_0", 26, no_coeff_skip=0)
    one("skip_prob_extremes", 27, prob_skip=1)
    for i, qd in enumerate([(15, 15, 15, 15, 15), (-15, -15, -15, -15, -15)]):
        one("q_deltas_clamp_high_%d" % i, 28 + i, yac=127, q_deltas=qd)
        one("q_deltas_clamp_low_%d" % i, 30 + i, yac=0, q_deltas=qd)
    one("uvdc_cap_132", 32, yac=120, q_deltas=(0, 0, 0, 7, 0))
    one("lf_deltas", 33, level=30, lf_delta=dict(ref=[-12, 5, 5, 5], mode=[9, 1, 2, 3]))
    one("lf_deltas_clamped", 34, level=60, lf_delta=dict(ref=[20, 0, 0, 0], mode=[-63, 0, 0, 0]))
    one("lf_deltas_no_update", 35, level=30, lf_delta=dict(update=0))
    one("lf_deltas_segments_out_of_range", 36, level=50, segmentation=dict(abs=0, lf=[30, -60, 0, 5], probs=[128, 128, 128]), lf_delta=dict(ref=[-10, 0, 0, 0], mode=[4, 0, 0, 0]))
    for s in range(1, 8):
        one("sharpness_%d" % s, 40 + s, level=7 * s + 5, sharpness=s)
    one("hev_thresholds", 48, level=63)
    one("level_0", 49, level=0)
    one("header_bits", 50, color_space=1, clamping=1, hscale=2, vscale=1, version=3, refresh=1)
    for v in (1, 2):
        one("version_%d" % v, 51 + v, version=v)
    one("prob_updates", 54, prob_updates={(0, 1, 0, 0): 200, (1, 0, 2, 3): 17, (2, 3, 1, 10): 1, (3, 7, 2, 5): 255, (3, 0, 0, 0): 90})
    # each DCT_CAT with its largest and smallest value, in luma with DC, Y2, chroma and luma after Y2
    mbs = random_mbs(w, h, 55, density=0.0, skip=0.0)
    top = [R.CAT_BASE[c] + (1 << len(R.CAT_PROBS[c])) - 1 for c in range(6)]
    for k, m in enumerate(mbs):
        lv = [0] * 16
        for c in range(6):
            lv[1 + 2 * c] = top[c] * (-1 if (c + k) & 1 else 1)
            lv[2 + 2 * c] = R.CAT_BASE[c]
        m["coefs"] = {(k * 5) % 16: lv, 16 + k % 8: [top[5]] + lv[1:]}
        if m["ymode"] != R.B_PRED:
            m["coefs"][24] = [-top[5]] + lv[1:]
        else:
            m["coefs"][(k * 5) % 16] = [top[4]] + lv[1:]
    one("dct_cats", 55, mbs=mbs, yac=0)
    one("dct_cats_coarse", 55, mbs=mbs, yac=127, q_deltas=(0, 15, 15, 0, 0))
    one("big_levels", 56, mbs=random_mbs(w, h, 56, density=0.5, big=True), yac=100)
    cases.append(("sub_block_modes_at_edges", _corner_modes()))
    # show_frame 0 between two shown frames
    cases.append(("hidden_frame", R.ivf([key_frame(w, h, random_mbs(w, h, 60 + i), show=0 if i == 1 else 1, level=9) for i in range(3)], w, h)))
    cases.append(("empty_ivf_frame", R.ivf([key_frame(w, h, random_mbs(w, h, 63), level=9), b"", key_frame(w, h, random_mbs(w, h, 64), level=9)], w, h)))
    return cases


def damaged_cases():
    """[(name, stream)]: every picture decodes, deterministically, and counts in errors."""
    w, h = 48, 32
    f = key_frame(w, h, random_mbs(w, h, 70, density=0.5, skip=0.0), level=15, log2_parts=1)
    part1 = (f[0] | f[1] << 8 | f[2] << 16) >> 5
    out = [("truncated_tokens", R.ivf([f[:len(f) - len(f) // 4]], w, h)),
           ("truncated_first_partition", R.ivf([f[:10 + part1 // 2]], w, h)),
           ("header_only", R.ivf([f[:10]], w, h))]
    big = bytearray(f)
    big[10 + part1:10 + part1 + 3] = b"\xff\xff\x0f"                      # the first token partition claims a megabyte
    out.append(("partition_overrun", R.ivf([bytes(big)], w, h)))
    tag = bytearray(f)
    t = (f[0] | f[1] << 8 | f[2] << 16) & 31 | (len(f) * 4) << 5          # the first partition claims four times the frame
    tag[0:3] = struct.pack("<I", t)[:3]
    out.append(("first_partition_overrun", R.ivf([bytes(tag)], w, h)))
    garbage = bytes(random.Random(71).randrange(256) for _i in range(300))
    out.append(("garbage_after_header", R.ivf([f[:10] + garbage], w, h)))
    return out


def size_change():
    return R.ivf([key_frame(48, 32, random_mbs(48, 32, 80), level=8), key_frame(48, 32, random_mbs(48, 32, 81), level=8),
                  key_frame(80, 48, random_mbs(80, 48, 82), level=8), key_frame(33, 17, random_mbs(33, 17, 83), level=8)], 48, 32)


def inter_after_key():
    w, h = 48, 32
    k = key_frame(w, h, random_mbs(w, h, 90), level=8)
    return R.ivf([k, key_frame(w, h, random_mbs(w, h, 91), key=False)], w, h)


def refused_cases():
    """[(name, stream, the error text the handle must show)]"""
    w, h = 32, 32
    k = key_frame(w, h, random_mbs(w, h, 92))
    return [("inter_after_key", inter_after_key(), "VP8 inter frames are not built"),
            ("first_frame_inter", R.ivf([key_frame(w, h, random_mbs(w, h, 93), key=False)], w, h), "VP8: the first frame is not a key frame"),
            ("bad_start_code", R.ivf([key_frame(w, h, random_mbs(w, h, 94), start_code=b"\x9d\x01\x2b")], w, h), "VP8: bad start code"),
            ("too_large", R.ivf([k[:6] + struct.pack("<HH", 8193, 32) + k[10:]], w, h), "VP8: picture size 8193x32 is not supported"),
            ("zero_size", R.ivf([k[:6] + struct.pack("<HH", 0, 32) + k[10:]], w, h), "VP8: picture size 0x32 is not supported")]
