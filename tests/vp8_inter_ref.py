"""RFC 6386 inter frames restated in numpy / plain Python (test reference for codec_type 5, options vp8 + vp8_inter).

It extends vp8_ref by import: the bool decoder, the token and transform routines, the intra predictors and the loop filters are vp8_ref's; the frame
loop is restated here because an inter frame threads state through it (probabilities, segment map, deltas, references).  Every table of sections
16 - 18 is typed in here, independently of jmcodec_amd/csrc/vp8_syntax.cpp and vp8_recon.h.

THERE IS NO INDEPENDENT PIN for inter frames: no VP8 inter encoder or decoder exists where this was written (libwebp does key frames only).  The C++ and
this file are two typings of the same text; a table typed wrong the same way twice would pass.  What holds inter frames is this restatement, the
structural checks below (check_tables) and the analytic answers of tests/test_vp8_inter_host.py that no decoder computed.

Rules fixed here (INTEGRATION.md "VP8"): reference windows are clamped to the DECODED area (16 mb_w x 16 mb_h, not the cropped size), "as if replicated
without end"; vectors are 16-bit sums and are never clamped, only near / nearest / best are; an intra macroblock and everything outside the frame
count as reference "intra" with a zero vector; buffer copies are taken from the references as they were before the frame, then the refreshes apply.
"""
import numpy as np

import vp8_ref as R
from jpeg_ref import frame_bytes

# ---- tables (RFC 6386 16.2, 16.3, 17.2, 18.3) ----
YMODE_PROB = [112, 86, 140, 37]
UV_MODE_PROB = [162, 101, 204]
YMODE_TREE = [-R.DC_PRED, 2, 4, 6, -R.V_PRED, -R.H_PRED, -R.TM_PRED, -R.B_PRED]
BMODE_PROB = [120, 90, 79, 133, 87, 85, 80, 111, 151]
MV_ZERO, MV_NEAREST, MV_NEAR, MV_NEW, MV_SPLIT = range(5)
MV_REF_TREE = [-MV_ZERO, 2, -MV_NEAREST, 4, -MV_NEAR, 6, -MV_NEW, -MV_SPLIT]
LEFT4, ABOVE4, ZERO4, NEW4 = range(4)
SUB_MV_REF_TREE = [-LEFT4, 2, -ABOVE4, 4, -ZERO4, -NEW4]
SPLIT_16x8, SPLIT_8x16, SPLIT_8x8, SPLIT_4x4 = range(4)
SPLIT_TREE = [-SPLIT_4x4, 2, -SPLIT_8x8, 4, -SPLIT_16x8, -SPLIT_8x16]
SPLIT_PROBS = [110, 111, 150]
SPLIT_COUNT = [2, 2, 4, 16]
SPLITS = [
    [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1],
    [0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1],
    [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3],
    list(range(16)),
]
SMALL_MV_TREE = [2, 8, 4, 6, -0, -1, -2, -3, 10, 12, -4, -5, -6, -7]
MODE_CONTEXTS = [[7, 1, 1, 143], [14, 18, 14, 107], [135, 64, 57, 68], [60, 56, 128, 65], [159, 134, 128, 34], [234, 188, 128, 28]]
# contexts: 0 normal, 1 left zero, 2 above zero, 3 left == above, 4 both zero
SUB_MV_REF_PROBS = [[147, 136, 18], [106, 145, 1], [179, 121, 1], [223, 1, 34], [208, 1, 1]]
# per component (rows, columns): is_short, sign, 7 of the short tree, 10 long bits
MV_IS_SHORT, MV_SIGN, MV_SHORT, MV_LONG, MV_LONG_BITS = 0, 1, 2, 9, 10
DEFAULT_MV_PROBS = [[162, 128, 225, 146, 172, 147, 214, 39, 156, 128, 129, 132, 75, 145, 178, 206, 239, 254, 254],
                    [164, 128, 204, 170, 119, 235, 140, 230, 228, 128, 130, 130, 74, 148, 180, 203, 236, 254, 254]]
MV_UPDATE_PROBS = [[237, 246, 253, 253, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 250, 250, 252, 254, 254],
                   [231, 243, 245, 253, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 251, 251, 254, 254, 254]]
SIXTAP = [[0, 0, 128, 0, 0, 0], [0, -6, 123, 12, -1, 0], [2, -11, 108, 36, -8, 1], [0, -9, 93, 50, -6, 0],
          [3, -16, 77, 77, -16, 3], [0, -6, 50, 93, -9, 0], [1, -8, 36, 108, -11, 2], [0, -1, 12, 123, -6, 0]]
BILINEAR = [[128, 0], [112, 16], [96, 32], [80, 48], [64, 64], [48, 80], [32, 96], [16, 112]]


def _leaves(tree):
    out, todo = [], [0]
    while todo:
        i = todo.pop()
        for b in (0, 1):
            t = tree[i + b]
            if t > 0:
                todo.append(t)
            else:
                out.append(-t)
    return sorted(out)


def check_tables():
    """Structural checks that need no decoder."""
    for k, row in enumerate(SIXTAP):
        assert sum(row) == 128, (k, row)
        assert row == SIXTAP[(8 - k) % 8][::-1] or k == 0, (k, row)
    for k in range(1, 8):
        assert SIXTAP[k] == SIXTAP[8 - k][::-1], k
    for k, row in enumerate(BILINEAR):
        assert row == [128 - 16 * k, 16 * k], (k, row)
    for s, n in zip(SPLITS, SPLIT_COUNT):
        assert len(s) == 16 and sorted(set(s)) == list(range(n)), s
        for p in range(n):      # every partition is a rectangle of blocks
            bl = [b for b in range(16) if s[b] == p]
            xs, ys = sorted({b & 3 for b in bl}), sorted({b >> 2 for b in bl})
            assert len(bl) == len(xs) * len(ys) and xs == list(range(xs[0], xs[-1] + 1)) and ys == list(range(ys[0], ys[-1] + 1)), (s, p)
    assert len(MODE_CONTEXTS) == 6 and all(len(r) == 4 for r in MODE_CONTEXTS)
    assert len(SUB_MV_REF_PROBS) == 5 and all(len(r) == 3 for r in SUB_MV_REF_PROBS)
    assert _leaves(MV_REF_TREE) == [0, 1, 2, 3, 4] and _leaves(SUB_MV_REF_TREE) == [0, 1, 2, 3] and _leaves(SPLIT_TREE) == [0, 1, 2, 3]
    assert _leaves(SMALL_MV_TREE) == list(range(8)) and _leaves(YMODE_TREE) == [0, 1, 2, 3, 4]
    for t in (DEFAULT_MV_PROBS, MV_UPDATE_PROBS):
        assert len(t) == 2 and all(len(r) == MV_LONG + MV_LONG_BITS == 19 for r in t)
        assert all(1 <= v <= 255 for r in t for v in r)
    assert len(YMODE_PROB) == 4 and len(UV_MODE_PROB) == 3 and len(BMODE_PROB) == 9


s16 = R.s16


def taps(interp, f):
    """the six taps over samples -2 .. +3 of fraction f; interp 0 six-tap, 1 bilinear"""
    if interp:
        return [0, 0, BILINEAR[f][0], BILINEAR[f][1], 0, 0]
    return SIXTAP[f]


def predict_block(plane, x0, y0, n, mvx, mvy, interp):
    """RFC 18: the n x n prediction of the block at (x0, y0) displaced by (mvx, mvy) eighth samples; the plane is replicated beyond its edges."""
    h, w = plane.shape
    xs = np.clip(np.arange(x0 + (mvx >> 3) - 2, x0 + (mvx >> 3) + n + 3), 0, w - 1)
    ys = np.clip(np.arange(y0 + (mvy >> 3) - 2, y0 + (mvy >> 3) + n + 3), 0, h - 1)
    win = plane[np.ix_(ys, xs)].astype(np.int64)
    tx, ty = taps(interp, mvx & 7), taps(interp, mvy & 7)
    tmp = sum(win[:, k:k + n] * tx[k] for k in range(6))
    tmp = np.clip((tmp + 64) >> 7, 0, 255)
    out = sum(tmp[k:k + n, :] * ty[k] for k in range(6))
    return np.clip((out + 64) >> 7, 0, 255)


def read_mv_component(d, p, info):
    x = 0
    if d.read(p[MV_IS_SHORT]):
        for i in range(3):
            x += d.read(p[MV_LONG + i]) << i
        for i in range(MV_LONG_BITS - 1, 3, -1):
            x += d.read(p[MV_LONG + i]) << i
        if x <= 15 or d.read(p[MV_LONG + 3]):     # bit 3 is coded only when a higher bit is set; otherwise it is 1 (a smaller vector is a short one)
            x += 8
        info["long_mvs"] += 1
        info["max_long"] = max(info["max_long"], x)
    else:
        x = d.tree(SMALL_MV_TREE, p[MV_SHORT:MV_SHORT + 7])
    if x and d.read(p[MV_SIGN]):
        x = -x
    return x


def near_search(A, L, AL, ref, sign_bias, mx, my, mbw, mbh):
    """RFC 16.3: (best, nearest, near, the four counts) from the macroblocks above, left and above-left (objects with ref, mv = (row, col), split).
    Above and left weigh 2, above-left 1; a neighbour whose reference has the other sign bias counts inverted; the three results are clamped to the
    window one macroblock beyond the frame."""
    near, cnt = [(0, 0)], [0, 0, 0, 0]
    for k, (o, wgt) in enumerate(((A, 2), (L, 2), (AL, 1))):
        if not o.ref:
            continue
        if o.mv != (0, 0):
            t = o.mv
            if sign_bias[o.ref] != sign_bias[ref]:
                t = (s16(-t[0]), s16(-t[1]))
            if k == 0 or t != near[-1]:
                near.append(t)
            cnt[len(near) - 1] += wgt
        else:
            cnt[0] += wgt
    if cnt[3] and near[-1] == near[1]:      # three distinct vectors were found, and the last equals the first
        cnt[1] += 1
    near += [(0, 0)] * (4 - len(near))
    cnt[3] = (int(A.split) + int(L.split)) * 2 + int(AL.split)
    if cnt[2] > cnt[1]:
        cnt[1], cnt[2] = cnt[2], cnt[1]
        near[1], near[2] = near[2], near[1]
    if cnt[1] >= cnt[0]:
        near[0] = near[1]
    lo_c, hi_c = -(mx * 128) - 128, (mbw - 1 - mx) * 128 + 128
    lo_r, hi_r = -(my * 128) - 128, (mbh - 1 - my) * 128 + 128

    def clamp(v):
        return (min(max(v[0], lo_r), hi_r), min(max(v[1], lo_c), hi_c))
    return clamp(near[0]), clamp(near[1]), clamp(near[2]), cnt


def sub_mv_context(lm, am):
    if lm == am:
        return 4 if lm == (0, 0) else 3
    if am == (0, 0):
        return 2
    if lm == (0, 0):
        return 1
    return 0


class Mb:
    pass


class InterDecoder:
    def __init__(self):
        self.base = R.RefDecoder()          # _block and _reconstruct, and the key-frame info
        self.info = self.base.info
        self.info.update(luma_fracs=set(), chroma_fracs=set(), beyond=set(), long_mvs=0, max_long=0, splits=set(), sub_mv=set(), ref_bias=set(),
                         mv_modes=set(), intra_beside_inter=set(), bmodes_beside_inter=set(), lf_ref_classes=set(), lf_mode_classes=set(),
                         inter_levels=set(), copy_flags=set(), refresh_last=set(), inter_versions=set(), mv_prob_updates=0, mode_prob_updates=0,
                         entropy_restored=0, kept_map_frames=0)
        self.errors = self.key_frames = self.inter_frames = self.hidden = self.empty = 0
        self.golden_refs = self.altref_refs = self.split_mbs = self.intra_in_inter = 0
        self.width = self.height = 0
        self.refs = [None, None, None, None]      # 1 last, 2 golden, 3 altref: [Y, U, V]

    def _reset(self, mbw, mbh):
        self.coef = [[[list(c) for c in b] for b in t] for t in R.DEFAULT_COEF_PROBS]
        self.mvp = [list(r) for r in DEFAULT_MV_PROBS]
        self.ymode_prob, self.uv_prob = list(YMODE_PROB), list(UV_MODE_PROB)
        self.seg_abs, self.seg_q, self.seg_lf = 0, [0] * 4, [0] * 4
        self.ref_delta, self.mode_delta = [0] * 4, [0] * 4
        self.sign_bias = [0, 0, 0, 0]
        self.seg_map = [0] * (mbw * mbh)

    def _entropy(self):
        return ([[[list(c) for c in b] for b in t] for t in self.coef], [list(r) for r in self.mvp], list(self.ymode_prob), list(self.uv_prob))

    def decode_frame(self, f):
        info = self.info
        if len(f) == 0:
            self.empty += 1
            return None
        damaged = False
        if len(f) < 3:
            f = bytes(f) + bytes(3 - len(f))
            damaged = True
        tag = f[0] | f[1] << 8 | f[2] << 16
        key, version, show, part1 = not (tag & 1), tag >> 1 & 7, tag >> 4 & 1, tag >> 5
        if not key and not self.key_frames:
            raise R.Refused("VP8: the first frame is not a key frame")
        if version > 3:
            raise R.Refused("VP8: version %d is not defined (RFC 6386 9.1)" % version)
        if key:
            hdr = bytes(f[3:10]) + bytes(max(0, 10 - len(f)))
            if len(f) < 10:
                damaged = True
            if hdr[0:3] != b"\x9d\x01\x2a":
                raise R.Refused("VP8: bad start code")
            w, hs = (hdr[3] | hdr[4] << 8) & 0x3FFF, hdr[4] >> 6
            h, vs = (hdr[5] | hdr[6] << 8) & 0x3FFF, hdr[6] >> 6
            if w == 0 or h == 0 or w > R.MAX_DIM or h > R.MAX_DIM:
                raise R.Refused("VP8: picture size %dx%d is not supported" % (w, h))
            info["scale"].add((hs, vs))
            body = f[10:]
        else:
            w, h = self.width, self.height
            body = f[3:]
        info["versions"].add(version)
        mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
        if key:
            self._reset(mbw, mbh)
        else:
            info["inter_versions"].add(version)
        if part1 > len(body):
            damaged = True
        d = R.BoolDecoder(body[:part1])
        if key:
            cs, cl = d.literal(1), d.literal(1)
            info["color_space"].add(cs)
            info["clamping"].add(cl)
        seg_probs = [255] * 3
        seg_on = d.literal(1)
        update_map = 0
        if seg_on:
            update_map = d.literal(1)
            if d.literal(1):
                self.seg_abs = d.literal(1)
                self.seg_q = [d.flagged(7) for _i in range(4)]
                self.seg_lf = [d.flagged(6) for _i in range(4)]
                info["seg_abs"].add(self.seg_abs)
            if update_map:
                seg_probs = [d.literal(8) if d.literal(1) else 255 for _i in range(3)]
            elif not key:
                info["kept_map_frames"] += 1
        filter_type, level, sharpness = d.literal(1), d.literal(6), d.literal(3)
        delta_on = d.literal(1)
        if delta_on and d.literal(1):
            for arr in (self.ref_delta, self.mode_delta):
                for i in range(4):
                    if d.literal(1):
                        v = d.literal(6)
                        arr[i] = -v if d.literal(1) else v
            info["lf_delta"].add((self.ref_delta[0], self.mode_delta[0]))
        info["filter_types"].add(filter_type)
        info["sharpness"].add(sharpness)
        n_parts = 1 << d.literal(2)
        info["partitions"].add(n_parts)
        yac = d.literal(7)
        ydc, y2dc, y2ac, uvdc, uvac = [d.flagged(4) for _i in range(5)]
        info["q_deltas"].add((ydc, y2dc, y2ac, uvdc, uvac))
        refresh_golden = refresh_alt = copy_gf = copy_arf = 0
        refresh_last = 1
        if not key:
            refresh_golden, refresh_alt = d.literal(1), d.literal(1)
            if not refresh_golden:
                copy_gf = d.literal(2)
            if not refresh_alt:
                copy_arf = d.literal(2)
            self.sign_bias[2], self.sign_bias[3] = d.literal(1), d.literal(1)
            info["copy_flags"].add((copy_gf, copy_arf))
        refresh_entropy = d.literal(1)
        info["refresh"].add(refresh_entropy)
        saved = None if refresh_entropy else self._entropy()
        if not key:
            refresh_last = d.literal(1)
            info["refresh_last"].add(refresh_last)
        probs = self.coef
        for i in range(4):
            for j in range(8):
                for k in range(3):
                    for l in range(11):
                        if d.read(R.COEF_UPDATE_PROBS[i][j][k][l]):
                            probs[i][j][k][l] = d.literal(8)
                            info["prob_updates"] += 1
        no_coeff_skip = d.literal(1)
        prob_skip = d.literal(8) if no_coeff_skip else 0
        info["no_coeff_skip"].add(no_coeff_skip)
        prob_intra = prob_last = prob_gf = 0
        if not key:
            prob_intra, prob_last, prob_gf = d.literal(8), d.literal(8), d.literal(8)
            if d.literal(1):
                self.ymode_prob = [d.literal(8) for _i in range(4)]
                info["mode_prob_updates"] += 1
            if d.literal(1):
                self.uv_prob = [d.literal(8) for _i in range(3)]
                info["mode_prob_updates"] += 1
            for i in range(2):
                for j in range(19):
                    if d.read(MV_UPDATE_PROBS[i][j]):
                        x = d.literal(7)
                        self.mvp[i][j] = x << 1 if x else 1
                        info["mv_prob_updates"] += 1

        def q(i):
            return 0 if i < 0 else 127 if i > 127 else i
        dq = []
        for s in range(4):
            base = yac
            if seg_on:
                base = self.seg_q[s] if self.seg_abs else yac + self.seg_q[s]
            base = q(base)
            dq.append((R.DC_Q[q(base + ydc)], R.AC_Q[base], R.DC_Q[q(base + y2dc)] * 2, max(R.AC_Q[q(base + y2ac)] * 155 // 100, 8),
                       min(R.DC_Q[q(base + uvdc)], 132), R.AC_Q[q(base + uvac)]))
        rest = body[part1:]
        sizes_len = 3 * (n_parts - 1)
        if len(rest) < sizes_len:
            damaged = True
        sizes = bytes(rest[:sizes_len]) + bytes(max(0, sizes_len - len(rest)))
        rest = rest[sizes_len:]
        parts, o = [], 0
        for p in range(n_parts):
            n = sizes[3 * p] | sizes[3 * p + 1] << 8 | sizes[3 * p + 2] << 16 if p < n_parts - 1 else max(0, len(rest) - o)
            if o + n > len(rest):
                damaged = True
            parts.append(R.BoolDecoder(rest[o:o + n]))
            o += n

        Y = np.zeros((mbh * 16, mbw * 16), np.int32)
        U = np.zeros((mbh * 8, mbw * 8), np.int32)
        V = np.zeros((mbh * 8, mbw * 8), np.int32)
        interp = 0 if version == 0 else 1
        above_b = [[R.B_DC_PRED] * 4 for _i in range(mbw)]
        above_nz = [[0] * 9 for _i in range(mbw)]
        outside = Mb()
        outside.ref, outside.mv, outside.split, outside.bmv, outside.ymode = 0, (0, 0), False, [(0, 0)] * 16, None
        grid = {}

        def at(x, y):
            return grid.get((x, y), outside)
        mbs = []
        for my in range(mbh):
            left_b = [R.B_DC_PRED] * 4
            left_nz = [0] * 9
            tok = parts[my % n_parts]
            for mx in range(mbw):
                m = Mb()
                if update_map:
                    self.seg_map[my * mbw + mx] = d.tree(R.SEGMENT_TREE, seg_probs)
                m.segment = self.seg_map[my * mbw + mx]
                m.skip = d.read(prob_skip) if no_coeff_skip else 0
                m.ref, m.mv, m.split, m.bmv, m.mvmode = 0, (0, 0), False, [(0, 0)] * 16, None
                if not key and d.read(prob_intra):
                    m.ref = 1
                    if d.read(prob_last):
                        m.ref = 2 + d.read(prob_gf)
                    self._inter_modes(d, m, at(mx, my - 1), at(mx - 1, my), at(mx - 1, my - 1), mx, my, mbw, mbh)
                    m.ymode = None
                    m.has_y2 = not m.split
                    above_b[mx], left_b = [R.B_DC_PRED] * 4, [R.B_DC_PRED] * 4
                    self.golden_refs += m.ref == 2
                    self.altref_refs += m.ref == 3
                    self.split_mbs += bool(m.split)
                else:
                    if key:
                        m.ymode = d.tree(R.KF_YMODE_TREE, R.KF_YMODE_PROB)
                    else:
                        m.ymode = d.tree(YMODE_TREE, self.ymode_prob)
                    if m.ymode == R.B_PRED:
                        m.bmodes = []
                        for b in range(16):
                            if key:
                                A = above_b[mx][b & 3] if b < 4 else m.bmodes[b - 4]
                                L = left_b[b >> 2] if not (b & 3) else m.bmodes[b - 1]
                                m.bmodes.append(d.tree(R.BMODE_TREE, R.KF_BMODE_PROBS[A][L]))
                            else:
                                m.bmodes.append(d.tree(R.BMODE_TREE, BMODE_PROB))
                        info["bmodes"].update(m.bmodes)
                        info["bpred_mbs"] += 1
                    else:
                        m.bmodes = [R.IMPLIED_BMODE[m.ymode]] * 16
                    above_b[mx] = m.bmodes[12:16]
                    left_b = m.bmodes[3::4]
                    m.uvmode = d.tree(R.UV_MODE_TREE, R.KF_UV_MODE_PROB if key else self.uv_prob)
                    m.has_y2 = m.ymode != R.B_PRED
                    info["ymodes"].add(m.ymode)
                    info["uvmodes"].add(m.uvmode)
                    if not key:
                        self.intra_in_inter += 1
                        if at(mx - 1, my).ref or at(mx, my - 1).ref:
                            info["intra_beside_inter"].add(m.ymode)
                            if m.ymode == R.B_PRED:
                                info["bmodes_beside_inter"].update(m.bmodes)
                grid[(mx, my)] = m
                if seg_on:
                    info["segments"].add(m.segment)
                coef = [[0] * 16 for _i in range(25)]
                any_nz = False
                an, ln = above_nz[mx], left_nz
                if m.skip:
                    info["skipped_mbs"] += 1
                    keep_a, keep_l = an[8], ln[8]
                    an[:] = [0] * 9
                    ln[:] = [0] * 9
                    if not m.has_y2:
                        an[8], ln[8] = keep_a, keep_l
                else:
                    info["coded_mbs"] += 1
                    D = dq[m.segment]
                    first = 0
                    if m.has_y2:
                        nz = self.base._block(tok, probs[1], an[8] + ln[8], 0, coef[24], D[2], D[3])
                        an[8] = ln[8] = nz
                        any_nz |= bool(nz)
                        first = 1
                    ptype = 0 if first else 3
                    for b in range(16):
                        nz = self.base._block(tok, probs[ptype], an[b & 3] + ln[b >> 2], first, coef[b], D[0], D[1])
                        an[b & 3] = ln[b >> 2] = nz
                        any_nz |= bool(nz)
                    for c in range(2):
                        for b in range(4):
                            ia, il = 4 + 2 * c + (b & 1), 4 + 2 * c + (b >> 1)
                            nz = self.base._block(tok, probs[2], an[ia] + ln[il], 0, coef[16 + 4 * c + b], D[4], D[5])
                            an[ia] = ln[il] = nz
                            any_nz |= bool(nz)
                m.inner = (not m.has_y2) or any_nz
                lv = level
                if seg_on:
                    lv = self.seg_lf[m.segment] if self.seg_abs else level + self.seg_lf[m.segment]
                lv = min(max(lv, 0), 63)
                if delta_on:
                    lv += self.ref_delta[m.ref]
                    if m.ref == 0:
                        if m.ymode == R.B_PRED:
                            lv += self.mode_delta[0]
                    else:
                        lv += self.mode_delta[1 if m.mvmode == MV_ZERO else 3 if m.mvmode == MV_SPLIT else 2]
                    lv = min(max(lv, 0), 63)
                    if not key:
                        info["lf_ref_classes"].add(m.ref)
                        info["lf_mode_classes"].add(0 if (m.ref == 0 and m.ymode == R.B_PRED) else None if m.ref == 0 else
                                                    1 if m.mvmode == MV_ZERO else 3 if m.mvmode == MV_SPLIT else 2)
                m.level = lv
                info["levels"].add(lv)
                if not key:
                    info["inter_levels"].add(lv)
                mbs.append(m)
                if m.ref:
                    self._predict_inter(m, coef, Y, U, V, mx, my, interp, version)
                else:
                    self.base._reconstruct(m, coef, Y, U, V, mx, my, mbw)
        past = max([d.past] + [p.past for p in parts])
        info["max_past"] = max(info["max_past"], past)
        if past > 2:
            damaged = True
        if damaged:
            self.errors += 1
            info["damaged"] += 1
        if saved is not None:
            self.coef, self.mvp, self.ymode_prob, self.uv_prob = saved
            info["entropy_restored"] += 1
        out = self._loop_filter(Y, U, V, mbs, mbw, mbh, filter_type, sharpness, not key)
        # references (9.7): copies from the references as they were, then the refreshes
        if key:
            self.refs = [None, out, out, out]
            self.key_frames += 1
        else:
            last, golden, alt = self.refs[1], self.refs[2], self.refs[3]
            if copy_arf == 1:
                self.refs[3] = last
            elif copy_arf == 2:
                self.refs[3] = golden
            if copy_gf == 1:
                self.refs[2] = last
            elif copy_gf == 2:
                self.refs[2] = alt
            if refresh_golden:
                self.refs[2] = out
            if refresh_alt:
                self.refs[3] = out
            if refresh_last:
                self.refs[1] = out
            self.inter_frames += 1
        if not show:
            self.hidden += 1
        self.width, self.height = w, h
        return out, w, h, bool(show)

    # -- 16.3: the vector(s) of an inter macroblock
    def _inter_modes(self, d, m, A, L, AL, mx, my, mbw, mbh):
        info = self.info
        info["ref_bias"].add((m.ref, self.sign_bias[m.ref]))
        best, nearest, nearby, cnt = near_search(A, L, AL, m.ref, self.sign_bias, mx, my, mbw, mbh)
        p = [MODE_CONTEXTS[cnt[i]][i] for i in range(4)]
        m.mvmode = d.tree(MV_REF_TREE, p)
        info["mv_modes"].add(m.mvmode)

        def read_mv():
            r = read_mv_component(d, self.mvp[0], info) * 2
            c = read_mv_component(d, self.mvp[1], info) * 2
            return (s16(best[0] + r), s16(best[1] + c))
        if m.mvmode == MV_SPLIT:
            kind = d.tree(SPLIT_TREE, SPLIT_PROBS)
            info["splits"].add(kind)
            bmv = [(0, 0)] * 16
            for j in range(SPLIT_COUNT[kind]):
                b0 = SPLITS[kind].index(j)
                lm = bmv[b0 - 1] if b0 & 3 else L.bmv[b0 + 3]
                am = bmv[b0 - 4] if b0 >> 2 else A.bmv[b0 + 12]
                ctx = sub_mv_context(lm, am)
                sub = d.tree(SUB_MV_REF_TREE, SUB_MV_REF_PROBS[ctx])
                info["sub_mv"].add((ctx, sub))
                v = lm if sub == LEFT4 else am if sub == ABOVE4 else (0, 0) if sub == ZERO4 else read_mv()
                for b in range(16):
                    if SPLITS[kind][b] == j:
                        bmv[b] = v
            m.bmv, m.mv, m.split, m.kind = bmv, bmv[15], True, kind
        else:
            m.mv = (0, 0) if m.mvmode == MV_ZERO else nearest if m.mvmode == MV_NEAREST else nearby if m.mvmode == MV_NEAR else read_mv()
            m.bmv = [m.mv] * 16

    def _predict_inter(self, m, coef, Y, U, V, mx, my, interp, version):
        info = self.info
        ref = self.refs[m.ref]
        ry, ru, rv = ref
        H, W = ry.shape

        def note(x, y, n, mvx, mvy, w, h):
            if x + (mvx >> 3) + n <= -w:
                info["beyond"].add("left")
            if x + (mvx >> 3) >= 2 * w:
                info["beyond"].add("right")
            if y + (mvy >> 3) + n <= -h:
                info["beyond"].add("top")
            if y + (mvy >> 3) >= 2 * h:
                info["beyond"].add("bottom")
        if m.has_y2:
            dc = R.iwht(coef[24])
            for b in range(16):
                coef[b][0] = dc[b]
        x0, y0 = mx * 16, my * 16
        if not m.split:
            r, c = m.mv
            P = predict_block(ry, x0, y0, 16, c, r, interp)
            info["luma_fracs"].add((c & 7, r & 7))
            note(x0, y0, 16, c, r, W, H)
            # the chroma vector: half the luma vector rounded away from zero -- the luma vector read in eighth samples of the chroma plane
            cc, cr = int((c + (1 if c >= 0 else -1)) / 2), int((r + (1 if r >= 0 else -1)) / 2)
            if version == 3:
                cc, cr = cc & ~7, cr & ~7
            info["chroma_fracs"].add((cc & 7, cr & 7))
            PU = predict_block(ru, mx * 8, my * 8, 8, cc, cr, interp)
            PV = predict_block(rv, mx * 8, my * 8, 8, cc, cr, interp)
        else:
            P = np.zeros((16, 16), np.int64)
            PU, PV = np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)
            for b in range(16):
                r, c = m.bmv[b]
                bx, by = (b & 3) * 4, (b >> 2) * 4
                P[by:by + 4, bx:bx + 4] = predict_block(ry, x0 + bx, y0 + by, 4, c, r, interp)
                info["luma_fracs"].add((c & 7, r & 7))
                note(x0 + bx, y0 + by, 4, c, r, W, H)
            for g in range(4):
                b = (g >> 1) * 8 + (g & 1) * 2
                sr = sum(m.bmv[k][0] for k in (b, b + 1, b + 4, b + 5))
                sc = sum(m.bmv[k][1] for k in (b, b + 1, b + 4, b + 5))
                cr, cc = int((sr + (4 if sr >= 0 else -4)) / 8), int((sc + (4 if sc >= 0 else -4)) / 8)      # (truncating division)
                if version == 3:
                    cc, cr = cc & ~7, cr & ~7
                info["chroma_fracs"].add((cc & 7, cr & 7))
                bx, by = (g & 1) * 4, (g >> 1) * 4
                PU[by:by + 4, bx:bx + 4] = predict_block(ru, mx * 8 + bx, my * 8 + by, 4, cc, cr, interp)
                PV[by:by + 4, bx:bx + 4] = predict_block(rv, mx * 8 + bx, my * 8 + by, 4, cc, cr, interp)
        for b in range(16):
            res = np.array(R.idct(coef[b]), np.int64).reshape(4, 4)
            bx, by = (b & 3) * 4, (b >> 2) * 4
            Y[y0 + by:y0 + by + 4, x0 + bx:x0 + bx + 4] = np.clip(P[by:by + 4, bx:bx + 4] + res, 0, 255)
        for ci, (pl, PP) in enumerate(((U, PU), (V, PV))):
            for b in range(4):
                res = np.array(R.idct(coef[16 + 4 * ci + b]), np.int64).reshape(4, 4)
                bx, by = (b & 1) * 4, (b >> 1) * 4
                pl[my * 8 + by:my * 8 + by + 4, mx * 8 + bx:mx * 8 + bx + 4] = np.clip(PP[by:by + 4, bx:bx + 4] + res, 0, 255)

    def _loop_filter(self, Y, U, V, mbs, mbw, mbh, filter_type, sharpness, inter):
        info = self.info
        planes = [Y.reshape(-1).tolist(), U.reshape(-1).tolist(), V.reshape(-1).tolist()]
        strides = [mbw * 16, mbw * 8, mbw * 8]
        for my in range(mbh):
            for mx in range(mbw):
                m = mbs[my * mbw + mx]
                if not m.level:
                    continue
                interior, sub_limit, mb_limit, thresh = R.filter_limits(m.level, sharpness)
                if inter:      # 15.3: frames that are no key frames take other high-edge-variance thresholds
                    thresh = 3 if m.level >= 40 else 2 if m.level >= 20 else 1 if m.level >= 15 else 0
                if mx or my:
                    info["mb_edge_mbs"] += 1
                if m.inner:
                    info["inner_edge_mbs"] += 1
                for pl in range(1 if filter_type else 3):
                    n, st = (16 if pl == 0 else 8), strides[pl]
                    px, o = planes[pl], my * n * st + mx * n
                    if mx:
                        for r in range(n):
                            if filter_type:
                                R.filter_simple(px, o + r * st, 1, mb_limit)
                            else:
                                R.filter_mbedge(px, o + r * st, 1, interior, mb_limit, thresh)
                    if m.inner:
                        for e in range(4, n, 4):
                            for r in range(n):
                                if filter_type:
                                    R.filter_simple(px, o + r * st + e, 1, sub_limit)
                                else:
                                    R.filter_subblock(px, o + r * st + e, 1, interior, sub_limit, thresh)
                    if my:
                        for c in range(n):
                            if filter_type:
                                R.filter_simple(px, o + c, st, mb_limit)
                            else:
                                R.filter_mbedge(px, o + c, st, interior, mb_limit, thresh)
                    if m.inner:
                        for e in range(4, n, 4):
                            for c in range(n):
                                if filter_type:
                                    R.filter_simple(px, o + e * st + c, st, sub_limit)
                                else:
                                    R.filter_subblock(px, o + e * st + c, st, interior, sub_limit, thresh)
        return [np.array(planes[0], np.uint8).reshape(mbh * 16, mbw * 16), np.array(planes[1], np.uint8).reshape(mbh * 8, mbw * 8),
                np.array(planes[2], np.uint8).reshape(mbh * 8, mbw * 8)]


def decode_stream(data, out_fmt=1, info=None, planes=None):
    """Every display frame of a stream -> [(frame bytes, dw, dh)].  data: an IVF byte stream or a list of frames.  planes: a list that receives every
    decoded frame's uncropped [Y, U, V], hidden ones too."""
    d = InterDecoder()
    out = []
    frames = R.split_ivf(data) if isinstance(data, (bytes, bytearray)) and bytes(data[:4]) == b"DKIF" else ([data] if isinstance(data, (bytes, bytearray)) else list(data))
    try:
        for f in frames:
            r = d.decode_frame(f)
            if r is None:
                continue
            if planes is not None:
                planes.append(r[0])
            if not r[3]:
                continue
            fr, dw, dh = R.nv12(r[0], r[1], r[2])
            out.append((frame_bytes(fr, dw, dh, out_fmt), dw, dh))
    finally:
        if info is not None:
            info.update(d.info)
            info.update(errors=d.errors, key_frames=d.key_frames, inter_frames=d.inter_frames, hidden=d.hidden, empty=d.empty, golden_refs=d.golden_refs,
                        altref_refs=d.altref_refs, split_mbs=d.split_mbs, intra_in_inter=d.intra_in_inter)
    return out
