"""MPEG-2 video (ISO/IEC 13818-2) restated in numpy: 6.2 (headers, slices, macroblocks, blocks), 7.2 - 7.6 (VLC decode, inverse scan, inverse
quantisation, saturation, mismatch control, prediction, reconstruction), decoding whole elementary streams into display-order frames.

The tables below (B-1 to B-4, B-9, B-10, B-12 to B-16, the scans, the default matrix, the non-linear quantiser scale) are typed by hand as bit
strings; they are not generated from the C++ tables and the C++ tables are not generated from them -- tests/test_mpeg2_host.py compares the two.
The IDCT is the integer form of INTEGRATION.md "MPEG-2" (the matrix M of jpeg_ref); what the library refuses raises Refused.  Damage is concealed as
INTEGRATION.md says: the macroblock in which it shows and the rest of its slice are dropped, and macroblocks no slice covers become zero-vector
forward copies (P, B) or grey intra blocks (I)."""
import numpy as np

from jpeg_ref import M, frame_bytes


class Refused(Exception):
    pass


class _Damage(Exception):
    pass


# ---- Annex B, as bit strings ------------------------------------------------------------------------------------------------------------
B1 = {1: "1", 2: "011", 3: "010", 4: "0011", 5: "0010", 6: "00011", 7: "00010", 8: "0000111", 9: "0000110", 10: "00001011", 11: "00001010",
      12: "00001001", 13: "00001000", 14: "00000111", 15: "00000110", 16: "0000010111", 17: "0000010110", 18: "0000010101", 19: "0000010100",
      20: "0000010011", 21: "0000010010", 22: "00000100011", 23: "00000100010", 24: "00000100001", 25: "00000100000", 26: "00000011111",
      27: "00000011110", 28: "00000011101", 29: "00000011100", 30: "00000011011", 31: "00000011010", 32: "00000011001", 33: "00000011000"}
B1_ESCAPE = "00000001000"
# macroblock_type: (quant, forward, backward, pattern, intra) -> code
B2 = {(0, 0, 0, 0, 1): "1", (1, 0, 0, 0, 1): "01"}
B3 = {(0, 1, 0, 1, 0): "1", (0, 0, 0, 1, 0): "01", (0, 1, 0, 0, 0): "001", (0, 0, 0, 0, 1): "00011", (1, 1, 0, 1, 0): "00010", (1, 0, 0, 1, 0): "00001",
      (1, 0, 0, 0, 1): "000001"}
B4 = {(0, 1, 1, 0, 0): "10", (0, 1, 1, 1, 0): "11", (0, 0, 1, 0, 0): "010", (0, 0, 1, 1, 0): "011", (0, 1, 0, 0, 0): "0010", (0, 1, 0, 1, 0): "0011",
      (0, 0, 0, 0, 1): "00011", (1, 1, 1, 1, 0): "00010", (1, 1, 0, 1, 0): "000011", (1, 0, 1, 1, 0): "000010", (1, 0, 0, 0, 1): "000001"}
B9 = {60: "111", 4: "1101", 8: "1100", 16: "1011", 32: "1010", 12: "10011", 48: "10010", 20: "10001", 40: "10000", 28: "01111", 44: "01110",
      52: "01101", 56: "01100", 1: "01011", 61: "01010", 2: "01001", 62: "01000", 24: "001111", 36: "001110", 3: "001101", 63: "001100",
      5: "0010111", 9: "0010110", 17: "0010101", 33: "0010100", 6: "0010011", 10: "0010010", 18: "0010001", 34: "0010000", 7: "00011111",
      11: "00011110", 19: "00011101", 35: "00011100", 13: "00011011", 49: "00011010", 21: "00011001", 41: "00011000", 14: "00010111",
      50: "00010110", 22: "00010101", 42: "00010100", 15: "00010011", 51: "00010010", 23: "00010001", 43: "00010000", 25: "00001111",
      37: "00001110", 26: "00001101", 38: "00001100", 29: "00001011", 45: "00001010", 53: "00001001", 57: "00001000", 30: "00000111",
      46: "00000110", 54: "00000101", 58: "00000100", 31: "000000111", 47: "000000110", 55: "000000101", 59: "000000100", 27: "000000011",
      39: "000000010", 0: "000000001"}
# motion_code magnitude -> code (a sign bit follows the non-zero ones: 0 positive, 1 negative)
B10 = {0: "1", 1: "01", 2: "001", 3: "0001", 4: "000011", 5: "0000101", 6: "0000100", 7: "0000011", 8: "000001011", 9: "000001010", 10: "000001001",
       11: "0000010001", 12: "0000010000", 13: "0000001111", 14: "0000001110", 15: "0000001101", 16: "0000001100"}
B12 = {0: "100", 1: "00", 2: "01", 3: "101", 4: "110", 5: "1110", 6: "11110", 7: "111110", 8: "1111110", 9: "11111110", 10: "111111110", 11: "111111111"}
B13 = {0: "00", 1: "01", 2: "10", 3: "110", 4: "1110", 5: "11110", 6: "111110", 7: "1111110", 8: "11111110", 9: "111111110", 10: "1111111110",
       11: "1111111111"}
EOB, ESC = "eob", "esc"


def _tail(run, first_level, hi, n_bits, count):
    """count codes of n_bits bits with values hi, hi - 1, ...: (run, first_level), (run, first_level + 1), ..."""
    return {(run, first_level + i): format(hi - i, "0%db" % n_bits) for i in range(count)}


def _singles(first_run, hi_values, n_bits):
    return {(first_run + i, 1): format(v, "0%db" % n_bits) for i, v in enumerate(hi_values)}


# the long codes are the same in B-14 and B-15: (0, 16..31) 14 bits, (0, 32..40) 15 bits, (1, 8..14) 15 bits, (1, 15..18) 16 bits, the second and third
# levels of runs 6..16, and runs 17..31
_LONG = {}
_LONG.update(_tail(0, 16, 0b11111, 14, 16))
_LONG.update(_tail(0, 32, 0b11000, 15, 9))
_LONG.update(_tail(1, 8, 0b11111, 15, 7))
_LONG.update(_tail(1, 15, 0b10011, 16, 4))
_LONG.update({(1, 6): "0000000010110", (1, 7): "0000000010101", (2, 5): "0000000010100", (3, 3): "000000011100", (3, 4): "0000000010011",
              (4, 3): "000000010010", (5, 3): "0000000010010", (6, 2): "000000011110", (6, 3): "0000000000010100", (7, 2): "000000010101",
              (8, 2): "000000010001", (9, 2): "0000000010001", (10, 2): "0000000010000"})
_LONG.update({(11 + i, 2): format(0b11010 - i, "016b") for i in range(6)})
_LONG.update(_singles(17, [0b11111, 0b11010, 0b11001, 0b10111, 0b10110], 12))
_LONG.update(_singles(22, [0b11111, 0b11110, 0b11101, 0b11100, 0b11011], 13))
_LONG.update(_singles(27, [0b11111, 0b11110, 0b11101, 0b11100, 0b11011], 16))
B14 = dict(_LONG)
B14.update({EOB: "10", ESC: "000001", (0, 1): "11", (0, 2): "0100", (0, 3): "00101", (0, 4): "0000110", (0, 5): "00100110", (0, 6): "00100001",
            (0, 7): "0000001010", (0, 8): "000000011101", (0, 9): "000000011000", (0, 10): "000000010011", (0, 11): "000000010000",
            (0, 12): "0000000011010", (0, 13): "0000000011001", (0, 14): "0000000011000", (0, 15): "0000000010111",
            (1, 1): "011", (1, 2): "000110", (1, 3): "00100101", (1, 4): "0000001100", (1, 5): "000000011011",
            (2, 1): "0101", (2, 2): "0000100", (2, 3): "0000001011", (2, 4): "000000010100",
            (3, 1): "00111", (3, 2): "00100100", (4, 1): "00110", (4, 2): "0000001111", (5, 1): "000111", (5, 2): "0000001001",
            (6, 1): "000101", (7, 1): "000100", (8, 1): "0000111", (9, 1): "0000101", (10, 1): "00100111", (11, 1): "00100011",
            (12, 1): "00100010", (13, 1): "00100000", (14, 1): "0000001110", (15, 1): "0000001101", (16, 1): "0000001000"})
B15 = dict(_LONG)
B15.update({EOB: "0110", ESC: "000001", (0, 1): "10", (0, 2): "110", (0, 3): "0111", (0, 4): "11100", (0, 5): "11101", (0, 6): "000101",
            (0, 7): "000100", (0, 8): "1111011", (0, 9): "1111100", (0, 10): "00100011", (0, 11): "00100010", (0, 12): "11111010",
            (0, 13): "11111011", (0, 14): "11111110", (0, 15): "11111111",
            (1, 1): "010", (1, 2): "00110", (1, 3): "1111001", (1, 4): "00100111", (1, 5): "00100000",
            (2, 1): "00101", (2, 2): "0000111", (2, 3): "11111100", (2, 4): "0000001100",
            (3, 1): "00111", (3, 2): "00100110", (4, 1): "000110", (4, 2): "11111101", (5, 1): "000111", (5, 2): "000000100",
            (6, 1): "0000110", (7, 1): "0000100", (8, 1): "0000101", (9, 1): "1111000", (10, 1): "1111010", (11, 1): "00100001",
            (12, 1): "00100101", (13, 1): "00100100", (14, 1): "000000101", (15, 1): "000000111", (16, 1): "0000001101"})

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
ALTERNATE = [0, 8, 16, 24, 1, 9, 2, 10, 17, 25, 32, 40, 48, 56, 57, 49, 41, 33, 26, 18, 3, 11, 4, 12, 19, 27, 34, 42, 50, 58, 35, 43,
             51, 59, 20, 28, 5, 13, 6, 14, 21, 29, 36, 44, 52, 60, 37, 45, 53, 61, 22, 30, 7, 15, 23, 31, 38, 46, 54, 62, 39, 47, 55, 63]
SCAN = [ZIGZAG, ALTERNATE]
DEFAULT_INTRA = [8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40,
                 22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83]
NONLINEAR_SCALE = [0] + list(range(1, 9)) + list(range(10, 25, 2)) + list(range(28, 57, 4)) + list(range(64, 113, 8))
FRAME_RATES = {1: (24000, 1001), 2: (24, 1), 3: (25, 1), 4: (30000, 1001), 5: (30, 1), 6: (50, 1), 7: (60000, 1001), 8: (60, 1)}


def quantiser_scale(q_scale_type, code):
    return NONLINEAR_SCALE[code] if q_scale_type else 2 * code


def _decoder(table):
    return {v: k for k, v in table.items()}


_D = {name: _decoder(t) for name, t in dict(B1=B1, B2=B2, B3=B3, B4=B4, B9=B9, B10=B10, B12=B12, B13=B13, B14=B14, B15=B15).items()}
_MAXLEN = {name: max(len(c) for c in d) for name, d in _D.items()}


class Bits:
    """MSB first; bits beyond the end read as zero and set `over`."""

    def __init__(self, data):
        self.s = "".join(format(b, "08b") for b in data)
        self.pos = 0
        self.over = False

    def peek(self, n):
        return (self.s[self.pos:self.pos + n] + "0" * n)[:n]

    def get(self, n):
        v = int(self.peek(n), 2) if n else 0
        self.pos += n
        if self.pos > len(self.s):
            self.over = True
        return v

    def left(self):
        return max(0, len(self.s) - self.pos)

    def vlc(self, name, what):
        d, window = _D[name], self.peek(_MAXLEN[name])
        for n in range(1, _MAXLEN[name] + 1):
            if window[:n] in d:
                self.get(n)
                return d[window[:n]]
        raise _Damage("invalid " + what)


# ---- 7.4, 7.5: one block -------------------------------------------------------------------------------------------------------------------
def dequantise(QF, intra, W, qs, dc_mult):
    """QF, W: 64 values in natural order -> F after saturation and mismatch control (7.4.2 - 7.4.4); `/` truncates toward zero."""
    QF = np.asarray(QF, np.int64)
    W = np.asarray(W, np.int64)
    if intra:
        num = 2 * QF * W * qs
        F = np.sign(num) * (np.abs(num) // 32)
        F[0] = dc_mult * QF[0]
    else:
        num = (2 * QF + np.sign(QF)) * W * qs
        F = np.sign(num) * (np.abs(num) // 32)
    F = np.clip(F, -2048, 2047)
    if int(F.sum()) % 2 == 0:
        F[63] += -1 if F[63] & 1 else 1
    return F


def idct(F):
    """F (64,) natural order -> residual (8, 8), the two integer passes of INTEGRATION.md, clipped to [-256, 255]."""
    F = np.asarray(F, np.int64).reshape(8, 8)
    g = np.clip((np.einsum("vy,vu->yu", M, F) + 256) >> 9, -65536, 65535)
    return np.clip((np.einsum("ux,yu->yx", M, g) + 65536) >> 17, -256, 255)


def _half(v):
    """the chroma vector of a luma vector: / 2 truncating toward zero"""
    return -((-v) // 2) if v < 0 else v // 2


def predict(plane, x, y, w, h, mvx, mvy):
    """7.6.4: the w x h prediction at (x, y) of `plane` (a frame or one field of it) with a vector in half samples; coordinates clamp to the plane"""
    H, Wd = plane.shape
    ix, iy, hx, hy = x + (mvx >> 1), y + (mvy >> 1), mvx & 1, mvy & 1
    xs0, xs1 = np.clip(np.arange(ix, ix + w), 0, Wd - 1), np.clip(np.arange(ix, ix + w) + hx, 0, Wd - 1)
    ys0, ys1 = np.clip(np.arange(iy, iy + h), 0, H - 1), np.clip(np.arange(iy, iy + h) + hy, 0, H - 1)
    p = plane.astype(np.int64)
    a, b, c, d = p[np.ix_(ys0, xs0)], p[np.ix_(ys0, xs1)], p[np.ix_(ys1, xs0)], p[np.ix_(ys1, xs1)]
    if hx and hy:
        return (a + b + c + d + 2) >> 2
    if hx:
        return (a + b + 1) >> 1
    if hy:
        return (a + c + 1) >> 1
    return a


class Seq:
    def __init__(self):
        self.valid = False
        self.display = None                     # None, or (matrix or None, display_w, display_h)

    def coded(self):
        mb_w = (self.width + 15) // 16
        mb_h = (self.height + 15) // 16 if self.progressive_sequence else 2 * ((self.height + 31) // 32)
        return mb_w, mb_h


class RefDecoder:
    """One handle: feed(whole stream) -> display-order frames as (Y, Cb, Cr) planes of the coded size with (width, height)."""

    def __init__(self):
        self.seq = None
        self.anchors = [None, None]
        self.anchor_shown = True
        self.out = []                           # (planes, width, height, info dict)
        self.errors = 0
        self.dropped = 0
        self.clamped = 0
        self.types = []

    # -- headers --
    def _matrix(self, b):
        w = [0] * 64
        for k in range(64):
            v = b.get(8)
            w[ZIGZAG[k]] = v if v else 16
        return w

    def _sequence_header(self, b):
        s = Seq()
        s.width, s.height, s.aspect, s.frame_rate_code = b.get(12), b.get(12), b.get(4), b.get(4)
        b.get(18 + 1 + 10 + 1)
        s.w = [list(DEFAULT_INTRA), [16] * 64]
        if b.get(1):
            s.w[0] = self._matrix(b)
        if b.get(1):
            s.w[1] = self._matrix(b)
        return s

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
                if pic["picture_structure"] in (1, 2):
                    raise Refused("field pictures are not supported")
                pic["ext"] = True
            elif 1 <= code <= 0xAF and pic is not None:
                if not pic["ext"]:
                    raise Refused("MPEG-1 video is not supported")
                pic["slices"].append((code, u[1:]))
        finish()
        self._show_anchor()
        return self.out

    # -- pictures --
    def _show_anchor(self):
        if self.anchors[1] is not None and not self.anchor_shown:
            self.out.append(self.anchors[1])
            self.anchor_shown = True

    def _picture(self, pic):
        if not pic["ext"]:
            self.errors += 1
            return
        s, t = self.seq, pic["type"]
        if (t == 2 and self.anchors[1] is None) or (t == 3 and (self.anchors[0] is None or self.anchors[1] is None)):
            self.dropped += 1
            return
        mb_w, mb_h = s.coded()
        self.W, self.H = mb_w * 16, mb_h * 16
        cur = [np.zeros((self.H, self.W), np.uint8), np.zeros((self.H // 2, self.W // 2), np.uint8), np.zeros((self.H // 2, self.W // 2), np.uint8)]
        refs = [self.anchors[1][0] if t == 2 else (self.anchors[0][0] if t == 3 else None), self.anchors[1][0] if t == 3 else None]
        self.pic, self.cur, self.refs, self.mb_w, self.mb_h = pic, cur, refs, mb_w, mb_h
        self.w = [list(s.w[0]), list(s.w[1])]
        covered = np.zeros(mb_w * mb_h, bool)
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
                self._store(a, dict(intra=False, fwd=[(0, 0)], bwd=None, field=False, sel={}), [None] * 6, False)
        self.errors += int(damaged) + int(self.clamped > clamped0)
        entry = (cur, s.width, s.height, dict(type=t, progressive_frame=pic["progressive_frame"], top_field_first=pic["top_field_first"],
                                              display=s.display))
        self.types.append(t)
        if t == 3:
            self.out.append(entry)
        else:
            self._show_anchor()
            self.anchors = [self.anchors[1], entry]
            self.anchor_shown = False

    def _reset_dc(self):
        self.dc = [1 << (self.pic["intra_dc_precision"] + 7)] * 3

    def _slice(self, vpos, payload):
        pic, b = self.pic, Bits(payload)
        row = vpos - 1
        if row >= self.mb_h:
            raise _Damage("slice outside the picture")
        code = b.get(5)
        if code == 0:
            raise _Damage("quantiser_scale_code 0")
        self.qs = quantiser_scale(pic["q_scale_type"], code)
        if b.get(1):
            b.get(8)
            while b.get(1) and not b.over:
                b.get(8)
        self._reset_dc()
        self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]               # [r][s][t]
        self.prev_dir = (True, False)
        prev, first = row * self.mb_w - 1, True
        while not b.over and b.left() > 0 and "1" in b.peek(23):
            inc = 0
            while b.peek(11) == B1_ESCAPE:
                b.get(11)
                inc += 33
            inc += b.vlc("B1", "macroblock_address_increment")
            addr = prev + inc
            if addr >= self.mb_w * self.mb_h:
                raise _Damage("address beyond the picture")
            if not first and inc > 1:
                if pic["type"] == 1:
                    raise _Damage("skipped macroblock in an I picture")
                for a in range(prev + 1, addr):
                    self._skipped(a)
            self._macroblock(b, addr)
            prev, first = addr, False

    def _skipped(self, a):
        self._reset_dc()
        if self.pic["type"] == 2:
            self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
            mb = dict(intra=False, fwd=[(0, 0)], bwd=None, field=False, sel={})
        else:
            f, bk = self.prev_dir
            mb = dict(intra=False, fwd=[tuple(self.pmv[0][0])] if f else None, bwd=[tuple(self.pmv[0][1])] if bk else None, field=False, sel={})
        self._store(a, mb, [None] * 6, False)

    def _mv_component(self, b, f_code, pred):
        if not 1 <= f_code <= 9:
            raise _Damage("f_code")
        code = b.vlc("B10", "motion_code")
        delta = 0
        if code:
            neg = b.get(1)
            r_size = f_code - 1
            delta = ((code - 1) << r_size) + b.get(r_size) + 1
            delta = -delta if neg else delta
        f = 1 << (f_code - 1)
        v = pred + delta
        if v < -16 * f:
            v += 32 * f
        elif v > 16 * f - 1:
            v -= 32 * f
        return v

    def _motion_vectors(self, b, s, field, sel):
        out = []
        for r in range(2 if field else 1):
            if field:
                sel[(r, s)] = b.get(1)
            x = self._mv_component(b, self.pic["f_code"][s][0], self.pmv[r][s][0])
            y = self._mv_component(b, self.pic["f_code"][s][1], self.pmv[r][s][1] >> 1 if field else self.pmv[r][s][1])
            self.pmv[r][s] = [x, 2 * y if field else y]
            out.append((x, y))
        if not field:
            self.pmv[1][s] = list(self.pmv[0][s])
        return out

    def _block(self, b, k, intra):
        pic = self.pic
        QF, n = [0] * 64, 0
        if intra:
            size = b.vlc("B12" if k < 4 else "B13", "dct_dc_size")
            diff = 0
            if size:
                v, half = b.get(size), 1 << (size - 1)
                diff = v if v >= half else v + 1 - 2 * half
            cc = 0 if k < 4 else k - 3
            self.dc[cc] += diff
            if not 0 <= self.dc[cc] < 1 << (8 + pic["intra_dc_precision"]):
                raise _Damage("intra DC out of range")
            QF[0], n = self.dc[cc], 1
        table = "B15" if intra and pic["intra_vlc_format"] else "B14"
        scan = SCAN[pic["alternate_scan"]]
        while True:
            if not intra and n == 0 and b.peek(1) == "1":
                b.get(1)
                run, level = 0, (-1 if b.get(1) else 1)
            else:
                sym = b.vlc(table, "DCT coefficient")
                if sym == EOB:
                    if not intra and n == 0:
                        raise _Damage("empty coded block")
                    break
                if sym == ESC:
                    run, level = b.get(6), b.get(12)
                    level -= 4096 if level >= 2048 else 0
                    if level in (0, -2048):
                        raise _Damage("forbidden escape level")
                else:
                    run, level = sym
                    level = -level if b.get(1) else level
            n += run
            if n > 63 or b.over:
                raise _Damage("more than 64 coefficients")
            QF[scan[n]] = level
            n += 1
        return idct(dequantise(QF, intra, self.w[0 if intra else 1], self.qs, 8 >> pic["intra_dc_precision"]))

    def _macroblock(self, b, addr):
        pic, t = self.pic, self.pic["type"]
        quant, mf, mbk, pattern, intra = b.vlc("B2" if t == 1 else ("B3" if t == 2 else "B4"), "macroblock_type")
        field_mv = field_dct = False
        if (mf or mbk) and not pic["frame_pred_frame_dct"]:
            fmt = b.get(2)
            if fmt == 3:
                raise Refused("dual-prime prediction is not supported")
            if fmt == 0:
                raise _Damage("reserved frame_motion_type")
            field_mv = fmt == 1
        if not pic["frame_pred_frame_dct"] and (intra or pattern):
            field_dct = bool(b.get(1))
        if quant:
            code = b.get(5)
            if code == 0:
                raise _Damage("quantiser_scale_code 0")
            self.qs = quantiser_scale(pic["q_scale_type"], code)
        mb = dict(intra=bool(intra), fwd=None, bwd=None, field=field_mv, sel={})
        if intra:
            if pic["concealment_mv"]:
                self._motion_vectors(b, 0, False, {})
                if not b.get(1):
                    raise _Damage("marker bit")
            else:
                self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        else:
            self._reset_dc()
            if mf:
                mb["fwd"] = self._motion_vectors(b, 0, field_mv, mb["sel"])
            if mbk:
                mb["bwd"] = self._motion_vectors(b, 1, field_mv, mb["sel"])
            if not mf and not mbk:
                if t != 2:
                    raise _Damage("no prediction in a B picture")
                mb["fwd"], mb["field"] = [(0, 0)], False
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

    # -- 7.6: prediction and reconstruction of one macroblock --
    def _clamp(self, mb, mx, my):
        hit = False
        for key in ("fwd", "bwd"):
            if mb.get(key) is None:
                continue
            out = []
            for (x, y) in mb[key]:
                x_lo, x_hi = -2 * mx * 16, 2 * (self.W - 16 - mx * 16)
                y_lo, y_hi = (-2 * my * 8, 2 * (self.H // 2 - 8 - my * 8)) if mb["field"] else (-2 * my * 16, 2 * (self.H - 16 - my * 16))
                cx, cy = min(max(x, x_lo), x_hi), min(max(y, y_lo), y_hi)
                hit |= (cx, cy) != (x, y)
                out.append((cx, cy))
            mb[key] = out
        self.clamped += int(hit)

    def _predict_mb(self, mb, key, s, mx, my):
        ref = self.refs[s]
        out = [np.zeros((16, 16), np.int64), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)]
        for c in range(3):
            n, x, y = (16, mx * 16, my * 16) if c == 0 else (8, mx * 8, my * 8)
            if not mb["field"]:
                vx, vy = mb[key][0]
                if c:
                    vx, vy = _half(vx), _half(vy)
                out[c] = predict(ref[c], x, y, n, n, vx, vy)
            else:
                for r in range(2):
                    vx, vy = mb[key][r]
                    if c:
                        vx, vy = _half(vx), _half(vy)
                    out[c][r::2] = predict(ref[c][mb["sel"][(r, s)]::2], x, y >> 1, n, n // 2, vx, vy)
        return out

    def _store(self, addr, mb, res, field_dct):
        mx, my = addr % self.mb_w, addr // self.mb_w
        self.covered[addr] = True
        if mb["intra"]:
            pred = [np.zeros((16, 16), np.int64), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)]
        else:
            self._clamp(mb, mx, my)
            f = self._predict_mb(mb, "fwd", 0, mx, my) if mb["fwd"] is not None else None
            bk = self._predict_mb(mb, "bwd", 1, mx, my) if mb["bwd"] is not None else None
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


def nv12(planes, width, height):
    dw, dh = (width + 1) & ~1, (height + 1) & ~1
    f = np.zeros((dh * 3 // 2, dw), np.uint8)
    f[:dh] = planes[0][:dh, :dw]
    f[dh:, 0::2] = planes[1][:dh // 2, :dw // 2]
    f[dh:, 1::2] = planes[2][:dh // 2, :dw // 2]
    return f, dw, dh


def decode_stream(data, out_fmt=1, info=None):
    """Every display frame of a stream -> [(frame bytes, dw, dh)]; info (a dict) receives errors, dropped, clamped, types and per-frame records."""
    d = RefDecoder()
    out = []
    frames = d.decode(data)
    for planes, w, h, _ in frames:
        f, dw, dh = nv12(planes, w, h)
        out.append((frame_bytes(f, dw, dh, out_fmt), dw, dh))
    if info is not None:
        info.update(errors=d.errors, dropped=d.dropped, clamped=d.clamped, types=d.types, frames=[i for _, _, _, i in frames])
    return out
