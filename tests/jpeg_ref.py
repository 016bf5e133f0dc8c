"""MJPEG (codec_type 2) restated in Python / numpy, literally after INTEGRATION.md "MJPEG": marker walk, canonical Huffman decode, the integer IDCT
with its two clips, the chroma rules, the NV12 / I420 frame -- and a small ENCODER that turns chosen levels, tables, sampling and restart interval
into a stream, so that tests can state answers no decoder computed.  Nothing here is shared with the product."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_JPEG = os.path.join(HERE, "golden", "jpeg")

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# M[k][n] = rint(8192 c_k cos((2n + 1) k pi / 16)), c_0 = 1 / sqrt(8), c_k = 1 / 2 -- computed, the product types it
M = np.array([[int(np.rint(8192 * (1 / math.sqrt(8) if k == 0 else 0.5) * math.cos((2 * n + 1) * k * math.pi / 16))) for n in range(8)] for k in range(8)],
             dtype=np.int64)


class Refused(Exception):
    """A feature the decoder refuses (the handle fails)."""


class Damaged(Exception):
    """A picture that cannot be decoded (dropped, errors counts it)."""


# ---------------------------------------------------------------------------------------------------------------- stream level
def split_pictures(data):
    """The pictures (SOI .. EOI) of a byte stream of concatenated JPEG pictures; segments are walked by their length fields, so an APPn segment that
    embeds a thumbnail's SOI / EOI is skipped whole.  A last picture that has no EOI is returned as far as it goes when its scan had begun."""
    out, n, o = [], len(data), 0
    while True:
        o = data.find(b"\xff\xd8", o)
        if o < 0:
            return out
        soi, o, sos = o, o + 2, False
        while True:
            if o >= n:
                if sos:
                    out.append(bytes(data[soi:]))
                return out
            if data[o] != 0xFF:
                o += 1
                continue
            while o < n and data[o] == 0xFF:
                o += 1
            if o >= n:
                continue
            m = data[o]
            o += 1
            if m == 0 or m == 1 or 0xD0 <= m <= 0xD7:
                continue
            if m == 0xD9:
                out.append(bytes(data[soi:o]))
                break
            if m == 0xD8:
                if sos:
                    out.append(bytes(data[soi:o - 2]))
                soi, sos = o - 2, False
                continue
            if o + 2 > n:
                o = n
                continue
            ln = data[o] << 8 | data[o + 1]
            if ln < 2:
                continue
            if o + ln > n:
                o = n
                continue
            o += ln
            if m == 0xDA:
                sos = True
                o = _scan_end(data, o)


def _scan_end(data, o):
    n = len(data)
    while True:
        o = data.find(b"\xff", o)
        if o < 0 or o + 1 >= n:
            return n
        nx = data[o + 1]
        if nx == 0 or 0xD0 <= nx <= 0xD7:
            o += 2
            continue
        if nx == 0xFF:
            k = o + 1
            while k < n and data[k] == 0xFF:
                k += 1
            if k < n and 0xD0 <= data[k] <= 0xD7:
                o = k + 1
                continue
        return o


class Huff:
    def __init__(self, bits, vals):
        self.bits, self.vals = list(bits), list(vals)
        self.look = [None] * 65536         # next 16 bits -> (length, symbol)
        self.enc = {}
        code, k = 0, 0
        for ln in range(1, 17):
            for _ in range(self.bits[ln - 1]):
                if code >= 1 << ln or k >= len(self.vals):
                    raise Damaged("DHT")
                lo = code << (16 - ln)
                self.look[lo:lo + (1 << (16 - ln))] = [(ln, self.vals[k])] * (1 << (16 - ln))
                self.enc[self.vals[k]] = (code, ln)
                code += 1
                k += 1
            code <<= 1


_STD = None


def std_tables():
    """T.81 Annex K.3 tables, {(class, id): Huff}: read from the DHT segments of a picture libjpeg wrote with its default tables (a committed fixture)."""
    global _STD
    if _STD is None:
        d = RefDecoder()
        d.headers(open(os.path.join(GOLDEN_JPEG, "c420_16x16.jpg"), "rb").read())
        _STD = {k: d.huff[k] for k in ((0, 0), (0, 1), (1, 0), (1, 1))}
    return _STD


def _segments(data):
    """Entropy data of a scan -> [(bytes with FF 00 unstuffed, marker that ended it or None)]: one piece per restart interval.  Fill bytes (FF FF ..) before
    a marker belong to the marker; data that stops inside an FF pair, or without a marker, ends the last piece with None."""
    out, cur, o, n = [], bytearray(), 0, len(data)
    while o < n:
        b = data[o]
        if b != 0xFF:
            cur.append(b)
            o += 1
        elif o + 1 < n and data[o + 1] == 0:
            cur.append(0xFF)
            o += 2
        else:
            while o < n and data[o] == 0xFF:
                o += 1
            out.append((bytes(cur), data[o] if o < n else None))
            cur = bytearray()
            o += 1
    if cur or not out or out[-1][1] is not None:
        out.append((bytes(cur), None))
    return out


class _Bits:
    """The bits of one piece as one integer, followed by zeros for ever; `left` goes negative once more was read than the piece holds."""

    def __init__(self, piece):
        self.d, self.left = piece, 8 * len(piece)

    def _peek(self, k):                    # the next k <= 16 bits
        pos = 8 * len(self.d) - self.left
        w = int.from_bytes(self.d[pos >> 3:(pos >> 3) + 3].ljust(3, b"\0"), "big")
        return (w >> (24 - (pos & 7) - k)) & ((1 << k) - 1)

    def get(self, k):
        x = self._peek(k)
        self.left -= k
        return x

    def decode(self, h):
        e = h.look[self._peek(16)]
        if e is None:
            raise Damaged("invalid Huffman code")
        self.left -= e[0]
        return e[1]

    def overrun(self):
        return self.left < 0


def _extend(v, s):
    return v - (1 << s) + 1 if v < 1 << (s - 1) else v


class RefDecoder:
    """One handle: tables persist from picture to picture."""

    def __init__(self):
        self.q, self.huff, self.ri = {}, {}, 0
        self.errors = 0

    def headers(self, pic):
        """Walk the segments of one picture; returns a dict describing it (frame, scan, tables in force) or raises Refused / Damaged."""
        assert pic[:2] == b"\xff\xd8"
        o, n, sof, sos, adobe = 2, len(pic), None, None, None
        self.ri = 0                        # SOI disables restart intervals (T.81 B.2.4.4); the tables persist
        while o < n:
            if pic[o] != 0xFF:
                o += 1
                continue
            while o < n and pic[o] == 0xFF:
                o += 1
            if o >= n:
                break
            m = pic[o]
            o += 1
            if m == 0 or m == 1 or 0xD0 <= m <= 0xD7:
                continue
            if m in (0xD8, 0xD9) or o + 2 > n:
                break
            ln = pic[o] << 8 | pic[o + 1]
            if ln < 2 or o + ln > n:
                if sos:
                    break
                raise Damaged("segment runs past the end")
            s = pic[o + 2:o + ln]
            o += ln
            if m == 0xC4:
                i = 0
                while i < len(s):
                    tc, th = s[i] >> 4, s[i] & 15
                    bits = list(s[i + 1:i + 17])
                    if tc > 1 or th > 3 or len(bits) < 16 or sum(bits) > 256 or i + 17 + sum(bits) > len(s):
                        raise Damaged("DHT")
                    self.huff[(tc, th)] = Huff(bits, s[i + 17:i + 17 + sum(bits)])
                    i += 17 + sum(bits)
            elif m == 0xDB:
                i = 0
                while i < len(s):
                    if s[i] >> 4:
                        raise Refused("Pq = 1")
                    if (s[i] & 15) > 3 or i + 65 > len(s):
                        raise Damaged("DQT")
                    self.q[s[i] & 15] = list(s[i + 1:i + 65])
                    i += 65
            elif m == 0xDD:
                self.ri = s[0] << 8 | s[1]
            elif m == 0xEE:
                if len(s) >= 12 and s[:5] == b"Adobe":
                    adobe = s[11]
            elif m in (0xC0, 0xC1):
                if sof:
                    raise Damaged("two frame headers")
                if s[0] != 8:
                    raise Refused("precision")
                h, w, nc = s[1] << 8 | s[2], s[3] << 8 | s[4], s[5]
                if h == 0:
                    raise Refused("DNL")
                if w > 8192 or h > 8192:
                    raise Refused("size")
                if nc not in (1, 3):
                    raise Refused("components")
                comps = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(nc)]
                if nc == 3:
                    y = comps[0][1] << 4 | comps[0][2]
                    if any(c[1] != 1 or c[2] != 1 for c in comps[1:]) or y not in (0x22, 0x21, 0x11):
                        raise Refused("sampling")
                    samp = y
                else:
                    samp = 0x10
                sof = dict(w=w, h=h, comps=comps, sampling=samp)
            elif m == 0xC2:
                raise Refused("progressive")
            elif m in (0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF, 0xDC):
                raise Refused("marker %02x" % m)
            elif m == 0xDA:
                if sos:
                    raise Refused("several scans")
                if not sof:
                    raise Damaged("scan without frame")
                ns = s[0]
                if ns != len(sof["comps"]):
                    raise Refused("several scans")
                sel = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(ns)]
                if (s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns]) != (0, 63, 0):
                    raise Refused("spectral selection")
                e = _scan_end(pic, o)
                std = None
                tabs = []
                for c in range(ns):
                    if sof["comps"][c][3] not in self.q:
                        raise Damaged("quantisation table missing")
                    t = []
                    for cls in (0, 1):
                        key = (cls, sel[c][cls])
                        if key in self.huff:
                            t.append(self.huff[key])
                        elif key[1] > 1:
                            raise Damaged("Huffman table missing")
                        else:
                            std = std or std_tables()
                            t.append(std[key])
                    tabs.append((list(self.q[sof["comps"][c][3]]), t[0], t[1]))
                sos = dict(data=pic[o:e], tabs=tabs, ri=self.ri)
                o = e
        if not sof or not sos:
            raise Damaged("no frame header / scan")
        if adobe is not None and adobe != 1:
            raise Refused("Adobe transform")
        return dict(sof, **sos)

    def levels(self, hd):
        """Entropy decode: per component an int64 array (block rows, block columns, 64) of levels in NATURAL order; stops at damage."""
        samp, ncomp = hd["sampling"], len(hd["comps"])
        hs, vs = (samp >> 4, samp & 15) if ncomp == 3 else (1, 1)
        mx_n, my_n = -(-hd["w"] // (8 * hs)), -(-hd["h"] // (8 * vs))
        planes = [np.zeros((my_n * vs, mx_n * hs, 64), np.int64)] + [np.zeros((my_n, mx_n, 64), np.int64) for _ in range(ncomp - 1)]
        segs, si = _segments(hd["data"]), 0
        br, pred, ri = _Bits(segs[0][0]), [0] * 3, hd["ri"]
        try:
            for mcu in range(mx_n * my_n):
                my, mx = divmod(mcu, mx_n)
                if ri and mcu and mcu % ri == 0:
                    if br.overrun():
                        raise Damaged("data ends early")
                    # the piece must be used up to its last byte (what is left: padding bits), and the marker behind it must be an RSTn (any n)
                    if br.left >= 8 or segs[si][1] is None or not 0xD0 <= segs[si][1] <= 0xD7:
                        raise Damaged("restart marker missing")
                    si += 1
                    br = _Bits(segs[si][0]) if si < len(segs) else _Bits(b"")
                    pred = [0] * 3
                blocks = [(0, my * vs + v, mx * hs + h) for v in range(vs) for h in range(hs)] + [(c, my, mx) for c in range(1, ncomp)]
                for c, by, bx in blocks:
                    _, dc, ac = hd["tabs"][c]
                    blk = np.zeros(64, np.int64)
                    s = br.decode(dc)
                    if s:
                        pred[c] += _extend(br.get(s), s)
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = br.decode(ac)
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r == 15:
                                k += 16
                                continue
                            break
                        k += r
                        if k > 63:
                            raise Damaged("run past the block")
                        blk[ZZ[k]] = _extend(br.get(s), s)
                        k += 1
                    if br.overrun():
                        raise Damaged("data ends early")
                    planes[c][by, bx] = blk
        except Damaged:
            self.errors += 1
        return planes

    def decode_picture(self, pic):
        """One picture -> (NV12 frame as an array of (dh * 3 // 2, dw), dw, dh, planes): planes = the decoded component planes (padded to whole blocks)."""
        hd = self.headers(pic)
        lv = self.levels(hd)
        planes = [idct_plane(lv[c], natural_q(hd["tabs"][c][0])) for c in range(len(lv))]
        return nv12_from_planes(planes, hd["sampling"], hd["w"], hd["h"]) + (planes,)


def natural_q(qzz):
    q = np.zeros(64, np.int64)
    for k in range(64):
        q[ZZ[k]] = qzz[k]
    return q


def idct_plane(levels, q):
    """levels (bh, bw, 64) natural order, q (64,) natural order -> samples (bh * 8, bw * 8) uint8, by the two expressions of INTEGRATION.md."""
    bh, bw, _ = levels.shape
    F = np.clip(levels * q, -32768, 32767).reshape(bh, bw, 8, 8)                       # F[v][u]
    g = np.clip((np.einsum("vy,abvu->abyu", M, F) + 256) >> 9, -65536, 65535)          # g[y][u]
    r = (np.einsum("ux,abyu->abyx", M, g) + 65536) >> 17                               # r[y][x]
    s = np.clip(r + 128, 0, 255).astype(np.uint8)
    return s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def chroma_420(c, sampling):
    c = c.astype(np.int64)
    if sampling == 0x22:
        return c
    if sampling == 0x21:
        return (c[0::2] + c[1::2] + 1) >> 1
    return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2


def nv12_from_planes(planes, sampling, w, h):
    dw, dh = (w + 1) & ~1, (h + 1) & ~1
    f = np.full((dh * 3 // 2, dw), 128, np.uint8)
    f[:dh] = planes[0][:dh, :dw]
    if sampling != 0x10:
        for c in (0, 1):
            f[dh:, c::2] = chroma_420(planes[1 + c], sampling)[:dh // 2, :dw // 2]
    return f, dw, dh


def frame_bytes(nv12, dw, dh, out_fmt):
    """The frame as the library hands it out: out_fmt 0 = NV12, 1 = I420."""
    if out_fmt == 0:
        return nv12.tobytes()
    return nv12[:dh].tobytes() + nv12[dh:, 0::2].tobytes() + nv12[dh:, 1::2].tobytes()


def decode_stream(data, out_fmt=1):
    """Every picture of a stream -> [(frame bytes, dw, dh)], one handle (tables persist).  Refused features raise."""
    d, out = RefDecoder(), []
    for pic in split_pictures(data):
        try:
            f, dw, dh, _ = d.decode_picture(pic)
        except Damaged:
            continue
        out.append((frame_bytes(f, dw, dh, out_fmt), dw, dh))
    return out


# ---------------------------------------------------------------------------------------------------------------- the encoder
def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def dht_segment(tables):
    """tables: {(class, id): Huff}"""
    p = b""
    for (tc, th), h in tables.items():
        p += bytes([tc << 4 | th]) + bytes(h.bits) + bytes(h.vals)
    return _seg(0xC4, p)


class _Writer:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, ln):
        self.acc = self.acc << ln | code
        self.n += ln
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def align(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _cat(v):
    return int(abs(int(v))).bit_length()


def encode(levels, qtabs, sampling, width, height, dri=0, dht=True, sof=0xC0, app=(), fill_before_rst=0, rst_offset=0, one_dqt=False,
           soi=True, tables=True, tq=(0, 1, 1)):
    """levels: per component an array (block rows, block columns, 64) of levels in natural order (whole MCUs); qtabs: list of 64-entry tables in ZIG-ZAG
    order (as DQT carries them), component c uses qtabs[tq[c]].  sampling 0x22 / 0x21 / 0x11 / 0x10.  dht=False leaves the DHT out (Annex K tables
    apply); tables=False leaves DQT and DHT out (a later picture of a stream).  fill_before_rst: that many FF fill bytes in front of every RSTn;
    rst_offset: added to the restart index."""
    std = std_tables()
    ncomp = 1 if sampling == 0x10 else 3
    hs, vs = (1, 1) if ncomp == 1 else (sampling >> 4, sampling & 15)
    out = bytearray(b"\xff\xd8" if soi else b"")
    for mk, payload in app:
        out += _seg(mk, payload)
    if tables:
        used = sorted(set(tq[:ncomp]))
        if one_dqt:
            out += _seg(0xDB, b"".join(bytes([t]) + bytes(qtabs[t]) for t in used))
        else:
            for t in used:
                out += _seg(0xDB, bytes([t]) + bytes(qtabs[t]))
    comps = [(1, hs << 4 | vs, tq[0])] + [(2 + c, 0x11, tq[1 + c]) for c in range(ncomp - 1)]
    out += _seg(sof, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp]) + b"".join(bytes(c) for c in comps))
    if dht and tables:
        out += dht_segment(std if ncomp == 3 else {k: std[k] for k in ((0, 0), (1, 0))})
    if dri:
        out += _seg(0xDD, dri.to_bytes(2, "big"))
    out += _seg(0xDA, bytes([ncomp]) + b"".join(bytes([1 + c, 0x00 if c == 0 else 0x11]) for c in range(ncomp)) + bytes([0, 63, 0]))
    w = _Writer()
    mx_n, my_n = -(-width // (8 * hs)), -(-height // (8 * vs))
    pred, rst = [0] * 3, 0
    zz = np.array(ZZ)
    lv_zz = [np.asarray(levels[c])[:, :, zz] for c in range(ncomp)]
    for mcu in range(mx_n * my_n):
        my, mx = divmod(mcu, mx_n)
        if dri and mcu and mcu % dri == 0:
            w.align()
            w.out += b"\xff" * fill_before_rst + bytes([0xFF, 0xD0 + ((rst + rst_offset) & 7)])
            rst += 1
            pred = [0] * 3
        blocks = [(0, my * vs + v, mx * hs + h) for v in range(vs) for h in range(hs)] + [(c, my, mx) for c in range(1, ncomp)]
        for c, by, bx in blocks:
            dc, ac = std[(0, 0 if c == 0 else 1)], std[(1, 0 if c == 0 else 1)]
            blk = lv_zz[c][by, bx].tolist()
            d = blk[0] - pred[c]
            pred[c] = blk[0]
            s = _cat(d)
            w.put(*dc.enc[s])
            if s:
                w.put(d if d > 0 else d + (1 << s) - 1, s)
            run = 0
            for k in range(1, 64):
                v = blk[k]
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    w.put(*ac.enc[0xF0])
                    run -= 16
                s = _cat(v)
                w.put(*ac.enc[run << 4 | s])
                w.put(v if v > 0 else v + (1 << s) - 1, s)
                run = 0
            if run:
                w.put(*ac.enc[0])
    w.align()
    return bytes(out) + bytes(w.out) + b"\xff\xd9"


def random_levels(rng, sampling, width, height, density=0.2, amp=40, dc_amp=200):
    ncomp = 1 if sampling == 0x10 else 3
    hs, vs = (1, 1) if ncomp == 1 else (sampling >> 4, sampling & 15)
    mx_n, my_n = -(-width // (8 * hs)), -(-height // (8 * vs))
    out = []
    for c in range(ncomp):
        shp = (my_n * vs, mx_n * hs, 64) if c == 0 else (my_n, mx_n, 64)
        lv = rng.integers(-amp, amp + 1, shp) * (rng.random(shp) < density)
        lv[:, :, 0] = rng.integers(-dc_amp, dc_amp + 1, shp[:2])
        out.append(lv.astype(np.int64))
    return out
