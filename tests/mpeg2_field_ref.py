"""MPEG-2 field pictures, 16x8 motion compensation and dual prime (ISO/IEC 13818-2 6.3.17.1, 7.6.2.1, 7.6.3.3 - 7.6.3.6, 7.6.4, 7.6.6) restated in
numpy on top of mpeg2_ref: what option mpeg2_field_pictures decodes.  Typed from the standard; the blocks, the VLC tables, the vector component and
the half-sample filter are mpeg2_ref's.  B-11 (dmvector) is typed here.

Two field pictures make one frame: a field's sample (x, y) is frame line 2 y + parity.  A field picture is the second field of the waiting frame
when the picture before it was a first field of the opposite parity and the types pair (I-I, I-P, P-P, B-B); anything else leaves the first field
alone: its lines are repeated into the missing field's, an error is counted.  `sw` holds switches the discrimination tests flip -- each one turns
one rule of the standard into a plausible mistake."""
import numpy as np

import mpeg2_ref as R
from mpeg2_ref import Bits, Refused, _Damage, _half, predict, quantiser_scale, idct, dequantise      # noqa: F401

B11 = {0: "0", 1: "10", -1: "11"}

SWITCHES = dict(select=0,        # 1: the other field than motion_vertical_field_select names
                parity=0,        # 1: a field picture stores into the lines of the other parity
                e_sign=0,        # 1: e = +1 for a top field, -1 for a bottom field
                m_swap=0,        # 1: m = 3 where the standard says 1 and the other way round
                v_round=0,       # 1: (v * m) >> 1 without the (v > 0) term
                avg_round=0,     # 1: the dual-prime average without its + 1
                split=8,         # the first line of the second 16x8 vector
                pmv_halve=0)     # 1: a field picture halves the vertical predictor, as a field vector of a frame picture does (and, being a field
                                 #    picture, does not double the vector when it stores it back)


class FieldRefDecoder(R.RefDecoder):
    def __init__(self, **sw):
        super().__init__()
        self.sw = dict(SWITCHES, **sw)
        self.pend = None                        # the frame whose first field waits: dict(entry, par, type)
        self.lone = 0
        self.fields = 0
        self.dual = 0
        self.m16x8 = 0
        self.cases = set()                      # (mode, direction, select or parity read, hx, hy) of every vector that predicted luma

    # -- the stream: mpeg2_ref's loop with field pictures let through --
    def decode(self, data):
        data = bytes(data)
        units, o = [], data.find(b"\x00\x00\x01")
        while o >= 0:
            e = data.find(b"\x00\x00\x01", o + 3)
            units.append(data[o + 3:e if e >= 0 else len(data)])
            o = e
        pend, pic, expect_ext = None, None, False

        def finish():
            nonlocal pic
            if pic is not None and self.seq is not None and self.seq.valid:
                self._picture(pic)
            pic = None
        for u in units:
            if not u:
                continue
            code, b = u[0], Bits(u[1:])
            ext = (u[1] >> 4) if code == 0xB5 and len(u) > 1 else -1
            if expect_ext and ext != 1:
                raise Refused("MPEG-1 video is not supported")
            if pic is not None and code in (0x00, 0xB3, 0xB7, 0xB8):
                finish()
            if code == 0xB3:
                pend, expect_ext = self._sequence_header(b), True
            elif ext == 1 and pend is not None:
                s = pend
                b.get(4)
                s.profile_level, s.progressive_sequence, s.chroma_format = b.get(8), b.get(1), b.get(2)
                if expect_ext:
                    s.width |= b.get(2) << 12
                    s.height |= b.get(2) << 12
                else:
                    b.get(4)
                b.get(12 + 1 + 8 + 1)
                s.fr_n, s.fr_d = b.get(2), b.get(5)
                expect_ext = False
                if s.chroma_format != 1:
                    raise Refused("chroma_format 4:2:2 / 4:4:4 is not supported")
                if s.height > 2800:
                    raise Refused("slice_vertical_position_extension is not supported")
                s.valid = True
                if self.seq is not None and self.seq.valid and (self.seq.width, self.seq.height, self.seq.progressive_sequence) != (
                        s.width, s.height, s.progressive_sequence):
                    self._close_pending()
                    self._show_anchor()
                    self.anchors = [None, None]
                self.seq = s
            elif ext in (5, 9, 10):
                raise Refused("the scalable extensions are not supported")
            elif ext == 2 and self.seq is not None:
                b.get(4 + 3)
                matrix = None
                if b.get(1):
                    b.get(16)
                    matrix = b.get(8)
                dw = b.get(14)
                b.get(1)
                self.seq.display = (matrix, dw, b.get(14))
            elif ext == 3 and self.seq is not None:
                b.get(4)
                for i in range(4):
                    if b.get(1):
                        w = self._matrix(b)
                        if i < 2:
                            self.seq.w[i] = w
            elif code == 0x00:
                p = dict(temporal_reference=b.get(10), type=b.get(3), slices=[], ext=False)
                if p["type"] == 4:
                    raise Refused("D pictures are not supported")
                pic = p if 1 <= p["type"] <= 3 else None
            elif ext == 8 and pic is not None:
                b.get(4)
                pic["f_code"] = [[b.get(4), b.get(4)], [b.get(4), b.get(4)]]
                for k in ("intra_dc_precision", "picture_structure", "top_field_first", "frame_pred_frame_dct", "concealment_mv", "q_scale_type",
                          "intra_vlc_format", "alternate_scan", "repeat_first_field", "chroma_420_type", "progressive_frame"):
                    pic[k] = b.get(2 if k in ("intra_dc_precision", "picture_structure") else 1)
                if pic["picture_structure"] == 0:            # reserved: a damaged header, the picture is dropped
                    self.errors += 1
                    pic = None
                else:
                    pic["ext"] = True
            elif 1 <= code <= 0xAF and pic is not None:
                if not pic["ext"]:
                    raise Refused("MPEG-1 video is not supported")
                pic["slices"].append((code, u[1:]))
        finish()
        self._close_pending()
        self._show_anchor()
        return self.out

    # -- frames out of fields --
    def _close_pending(self):
        if self.pend is None:
            return
        planes, e = self.pend["entry"][0], self.pend["par"]
        for p in planes:
            p[1 - e::2] = p[e::2]
        self.pend["entry"][3]["lone"] = e + 1
        self.errors += 1
        self.lone += 1
        if self.pend["type"] == 3:
            self.out.append(self.pend["entry"])
        self.pend = None

    @staticmethod
    def _field(entry, p):
        return None if entry is None else [pl[p::2] for pl in entry[0]]

    def _picture(self, pic):
        if not pic["ext"]:
            self.errors += 1
            return
        s, t, ps = self.seq, pic["type"], pic["picture_structure"]
        fieldpic = ps in (1, 2)
        if fieldpic and s.progressive_sequence:
            self.errors += 1
            return
        par = 1 if ps == 2 else 0
        second = (self.pend is not None and fieldpic and par != self.pend["par"] and
                  (self.pend["type"] == t or (self.pend["type"] == 1 and t == 2)))
        if self.pend is not None and not second:
            self._close_pending()
        if not second and ((t == 2 and self.anchors[1] is None) or (t == 3 and (self.anchors[0] is None or self.anchors[1] is None))):
            self.dropped += 1
            return
        mb_w, mb_h = s.coded()
        self.W, self.H = mb_w * 16, mb_h * 16
        if second:
            entry = self.pend["entry"]
            self.pend = None
        else:
            planes = [np.zeros((self.H, self.W), np.uint8), np.zeros((self.H // 2, self.W // 2), np.uint8), np.zeros((self.H // 2, self.W // 2), np.uint8)]
            entry = (planes, s.width, s.height, dict(type=t, progressive_frame=pic["progressive_frame"], top_field_first=pic["top_field_first"],
                                                     display=s.display, first_parity=par if fieldpic else None, lone=0))
            if t != 3:
                self._show_anchor()
                self.anchors = [self.anchors[1], entry]
                self.anchor_shown = False
            if fieldpic:
                self.pend = dict(entry=entry, par=par, type=t)
        # references.  Frame pictures: frames; field pictures: fields, [direction][parity] (7.6.2.1)
        a0, a1 = self.anchors
        self.fieldpic, self.par = fieldpic, par
        if not fieldpic:
            self.refs = [a0[0] if t in (2, 3) and a0 is not None else None, a1[0] if t == 3 else None]      # (a P frame: the anchors have moved already)
            self.rf = [[self._field(a0, 0), self._field(a0, 1)] if t in (2, 3) else [None, None], [self._field(a1, 0), self._field(a1, 1)] if t == 3 else [None, None]]
            self.cur = entry[0]
            self.mb_h = mb_h
        else:
            self.fields += 1
            if t == 2:
                f = [self._field(a0, 0), self._field(a0, 1)]
                if second:
                    f[1 - par] = self._field(entry, 1 - par)
                self.rf = [f, [None, None]]
            elif t == 3:
                self.rf = [[self._field(a0, 0), self._field(a0, 1)], [self._field(a1, 0), self._field(a1, 1)]]
            else:
                self.rf = [[None, None], [None, None]]
            store = par ^ self.sw["parity"]
            self.cur = [pl[store::2] for pl in entry[0]]
            self.mb_h = mb_h // 2
            self.H //= 2
        self.pic, self.mb_w = pic, mb_w
        self.w = [list(s.w[0]), list(s.w[1])]
        covered = np.zeros(mb_w * self.mb_h, bool)
        self.covered, damaged, clamped0 = covered, False, self.clamped
        for code, payload in pic["slices"]:
            try:
                self._slice(code, payload)
            except _Damage:
                damaged = True
        for a in np.flatnonzero(~covered):
            damaged = True
            if t == 1:
                grey = [0] * 64
                grey[0] = 128 << pic["intra_dc_precision"]
                self._store(a, dict(intra=True), [idct(dequantise(grey, True, self.w[0], 2, 8 >> pic["intra_dc_precision"]))] * 6, False)
            else:
                self._store(a, self._zero_mb(), [None] * 6, False)
        self.errors += int(damaged) + int(self.clamped > clamped0)
        self.types.append(t)
        if t == 3 and self.pend is None:
            self.out.append(entry)

    def _zero_mb(self):
        """the zero vector: frame prediction in a frame picture, the field of the picture's own parity in a field picture"""
        if self.fieldpic:
            return dict(intra=False, fwd=[(0, 0)], bwd=None, mode="field", sel={(0, 0): self.par})
        return dict(intra=False, fwd=[(0, 0)], bwd=None, mode="frame", sel={})

    def _skipped(self, a):
        self._reset_dc()
        if self.pic["type"] == 2:
            self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
            mb = self._zero_mb()
        else:                                   # 7.6.6.4: the direction(s) and predictors of the macroblock before; a field picture: same-parity fields
            f, bk = self.prev_dir
            mb = dict(intra=False, fwd=[tuple(self.pmv[0][0])] if f else None, bwd=[tuple(self.pmv[0][1])] if bk else None,
                      mode="field" if self.fieldpic else "frame", sel={(0, 0): self.par, (0, 1): self.par} if self.fieldpic else {})
        self._store(a, mb, [None] * 6, False)

    def _vectors(self, b, s, mode, sel, dmv=None):
        """motion_vectors(s) (6.2.5.1, 6.2.5.2.1) with the predictor updates of 7.6.3.3 - 7.6.3.4"""
        count = 2 if mode in ("field2", "16x8") else 1
        halve = mode == "field2" or (mode == "dual" and not self.fieldpic)
        wrong = self.fieldpic and self.sw["pmv_halve"]
        out = []
        for r in range(count):
            if mode in ("field2", "field", "16x8"):
                sel[(r, s)] = b.get(1)
            x = self._mv_component(b, self.pic["f_code"][s][0], self.pmv[r][s][0])
            if mode == "dual":
                dmv.append(self._dmvector(b))
            y = self._mv_component(b, self.pic["f_code"][s][1], self.pmv[r][s][1] >> 1 if halve or wrong else self.pmv[r][s][1])
            if mode == "dual":
                dmv.append(self._dmvector(b))
            self.pmv[r][s] = [x, 2 * y if halve else y]
            out.append((x, y))
        if count == 1:
            self.pmv[1][s] = list(self.pmv[0][s])
        return out

    @staticmethod
    def _dmvector(b):
        """B-11: 0 -> 0, 10 -> 1, 11 -> -1"""
        if not b.get(1):
            return 0
        return -1 if b.get(1) else 1

    def _derive(self, v, dmv):
        """7.6.3.6: the opposite-parity vector(s) of a dual-prime macroblock"""
        sw = self.sw

        def one(m, e):
            if sw["m_swap"]:
                m = 4 - m
            if sw["e_sign"]:
                e = -e
            rx = 0 if sw["v_round"] else int(v[0] > 0)
            ry = 0 if sw["v_round"] else int(v[1] > 0)
            return (((v[0] * m + rx) >> 1) + dmv[0], ((v[1] * m + ry) >> 1) + e + dmv[1])
        if self.fieldpic:
            return [one(1, -1 if self.par == 0 else 1)]
        tff = self.pic["top_field_first"]
        return [one(1 if tff else 3, -1), one(3 if tff else 1, 1)]

    def _macroblock(self, b, addr):
        pic, t = self.pic, self.pic["type"]
        quant, mf, mbk, pattern, intra = b.vlc("B2" if t == 1 else ("B3" if t == 2 else "B4"), "macroblock_type")
        field_dct = False
        mode = "field" if self.fieldpic else "frame"
        if (mf or mbk) and self.fieldpic:
            fmt = b.get(2)
            if fmt == 0:
                raise _Damage("reserved field_motion_type")
            mode = {1: "field", 2: "16x8", 3: "dual"}[fmt]
        elif (mf or mbk) and not pic["frame_pred_frame_dct"]:
            fmt = b.get(2)
            if fmt == 0:
                raise _Damage("reserved frame_motion_type")
            mode = {1: "field2", 2: "frame", 3: "dual"}[fmt]
        if mode == "dual" and (t != 2 or not mf):
            raise _Damage("dual prime in a B picture")
        if not self.fieldpic and not pic["frame_pred_frame_dct"] and (intra or pattern):
            field_dct = bool(b.get(1))
        if quant:
            code = b.get(5)
            if code == 0:
                raise _Damage("quantiser_scale_code 0")
            self.qs = quantiser_scale(pic["q_scale_type"], code)
        mb = dict(intra=bool(intra), fwd=None, bwd=None, mode=mode, sel={})
        if intra:
            if pic["concealment_mv"]:
                self._vectors(b, 0, "field" if self.fieldpic else "frame", {})
                if not b.get(1):
                    raise _Damage("marker bit")
            else:
                self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        else:
            self._reset_dc()
            dmv = []
            if mf:
                mb["fwd"] = self._vectors(b, 0, mode, mb["sel"], dmv)
            if mbk:
                mb["bwd"] = self._vectors(b, 1, mode, mb["sel"], dmv)
            if mode == "dual":
                mb["derived"] = self._derive(mb["fwd"][0], dmv)
            if not mf and not mbk:
                if t != 2:
                    raise _Damage("no prediction in a B picture")
                mb = self._zero_mb()
                self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
            self.prev_dir = (mb["fwd"] is not None, mb["bwd"] is not None)
        cbp = 63 if intra else 0
        if pattern:
            cbp = b.vlc("B9", "coded_block_pattern")
            if cbp == 0:
                raise _Damage("coded_block_pattern 0")
        res = [self._block(b, k, bool(intra)) if cbp & (32 >> k) else None for k in range(6)]
        if b.over:
            raise _Damage("slice ends inside a macroblock")
        self._store(addr, mb, res, field_dct)

    # -- prediction --
    def _geometry(self, mb, r, my):
        """first line, lines and height of the luma block vector r of the macroblock predicts, in the lines of what it reads from"""
        mode = mb["mode"]
        if self.fieldpic:
            return (my * 16 + 8 * r, 8, self.H) if mode == "16x8" else (my * 16, 16, self.H)
        return (my * 8, 8, self.H // 2) if mode in ("field2", "dual") else (my * 16, 16, self.H)

    def _clamp(self, mb, mx, my):
        hit = False

        def one(v, r):
            nonlocal hit
            pos, span, size = self._geometry(mb, r, my)
            c = (min(max(v[0], -2 * mx * 16), 2 * (self.W - 16 - mx * 16)), min(max(v[1], -2 * pos), 2 * (size - span - pos)))
            hit |= c != tuple(v)
            return c
        for key in ("fwd", "bwd"):
            if mb.get(key) is not None:
                mb[key] = [one(v, r) for r, v in enumerate(mb[key])]
        if mb["mode"] == "dual":
            mb["derived"] = [one(v, 0) for v in mb["derived"]]
        self.clamped += int(hit)

    def _from_field(self, fld, c, x, y, w, h, v, tag):
        """w x h samples of component c at (x, y) of a reference field (None: 128) with the luma vector v"""
        if fld is None:
            return np.full((h, w), 128, np.int64)
        vx, vy = (_half(v[0]), _half(v[1])) if c else v
        if c == 0:
            self.cases.add(tag + (v[0] & 1, v[1] & 1))
        return predict(fld[c], x, y, w, h, vx, vy)

    def _predict_dir(self, mb, key, s, mx, my):
        out, mode, sw = [None] * 3, mb["mode"], self.sw
        for c in range(3):
            n, x, y = (16, mx * 16, my * 16) if c == 0 else (8, mx * 8, my * 8)
            if mode == "frame":
                vx, vy = mb[key][0]
                if c:
                    vx, vy = _half(vx), _half(vy)
                out[c] = predict(self.refs[s][c], x, y, n, n, vx, vy) if self.refs[s] is not None else np.full((n, n), 128, np.int64)
            elif mode == "field2":
                out[c] = np.zeros((n, n), np.int64)
                for r in range(2):
                    sel = mb["sel"][(r, s)] ^ sw["select"]
                    out[c][r::2] = self._from_field(self.rf[s][sel], c, x, y >> 1, n, n // 2, mb[key][r], ("field2", s, sel))
            elif mode == "field":
                sel = mb["sel"][(0, s)] ^ sw["select"]
                out[c] = self._from_field(self.rf[s][sel], c, x, y, n, n, mb[key][0], ("field", s, sel))
            elif mode == "16x8":
                out[c] = np.zeros((n, n), np.int64)
                cut = sw["split"] if c == 0 else sw["split"] // 2
                for r in range(2):
                    sel = mb["sel"][(r, s)] ^ sw["select"]
                    y0, y1 = (0, cut) if r == 0 else (cut, n)
                    out[c][y0:y1] = self._from_field(self.rf[s][sel], c, x, y + y0, n, y1 - y0, mb[key][r], ("16x8", s, sel))
            else:                               # dual prime: same parity with the vector sent, opposite parity with the derived one
                rnd = 0 if sw["avg_round"] else 1
                if self.fieldpic:
                    a = self._from_field(self.rf[0][self.par], c, x, y, n, n, mb["fwd"][0], ("dual_field", 0, self.par))
                    bb = self._from_field(self.rf[0][1 - self.par], c, x, y, n, n, mb["derived"][0], ("dual_field", 0, 1 - self.par))
                    out[c] = (a + bb + rnd) >> 1
                else:
                    out[c] = np.zeros((n, n), np.int64)
                    for p in range(2):
                        a = self._from_field(self.rf[0][p], c, x, y >> 1, n, n // 2, mb["fwd"][0], ("dual_frame", 0, p))
                        bb = self._from_field(self.rf[0][1 - p], c, x, y >> 1, n, n // 2, mb["derived"][p], ("dual_frame", 0, 1 - p))
                        out[c][p::2] = (a + bb + rnd) >> 1
        return out

    def _store(self, addr, mb, res, field_dct):
        mx, my = addr % self.mb_w, addr // self.mb_w
        self.covered[addr] = True
        if mb["intra"]:
            pred = [np.zeros((16, 16), np.int64), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)]
        else:
            self._clamp(mb, mx, my)
            self.dual += mb["mode"] == "dual"
            self.m16x8 += mb["mode"] == "16x8"
            f = self._predict_dir(mb, "fwd", 0, mx, my) if mb["fwd"] is not None else None
            bk = self._predict_dir(mb, "bwd", 1, mx, my) if mb["bwd"] is not None else None
            pred = [(a + c + 1) >> 1 for a, c in zip(f, bk)] if f is not None and bk is not None else (f if f is not None else bk)
        r = [np.zeros((16, 16), np.int64), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)]
        for k in range(4):
            if res[k] is None:
                continue
            if field_dct:
                r[0][(k >> 1)::2, 8 * (k & 1):8 * (k & 1) + 8] = res[k]
            else:
                r[0][8 * (k >> 1):8 * (k >> 1) + 8, 8 * (k & 1):8 * (k & 1) + 8] = res[k]
        for c in (1, 2):
            if res[3 + c] is not None:
                r[c] = res[3 + c]
        for c in range(3):
            n = 16 if c == 0 else 8
            self.cur[c][my * n:my * n + n, mx * n:mx * n + n] = np.clip(pred[c] + r[c], 0, 255)


def decode_stream(data, out_fmt=1, info=None, **sw):
    """Every display frame of a stream -> [(frame bytes, dw, dh)]; info receives errors, dropped, clamped, lone, fields, dual, m16x8, cases, types and
    the per-frame records (first_parity, lone, ...)."""
    d = FieldRefDecoder(**sw)
    out = []
    frames = d.decode(data)
    for planes, w, h, _ in frames:
        f, dw, dh = R.nv12(planes, w, h)
        out.append((R.frame_bytes(f, dw, dh, out_fmt), dw, dh))
    if info is not None:
        info.update(errors=d.errors, dropped=d.dropped, clamped=d.clamped, lone=d.lone, fields=d.fields, dual=d.dual, m16x8=d.m16x8, cases=d.cases,
                    types=d.types, frames=[i for _, _, _, i in frames])
    return out
