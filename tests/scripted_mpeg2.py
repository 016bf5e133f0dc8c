"""A bit writer that turns a per-macroblock script into an MPEG-2 video elementary stream (ISO/IEC 13818-2 6.2): the tests choose picture types,
vectors, levels and every header field.  It is a syntax writer, not an encoder: nothing is estimated or quantised.  VLC tables: mpeg2_ref's.

A stream is a list of items:
    ("seq", dict)   sequence_header + sequence_extension [+ sequence_display_extension]: width, height, progressive_sequence (1), aspect (1),
                    frame_rate_code (3), fr_ext (0, 0), chroma_format (1), profile_level (0x48), intra_matrix / non_intra_matrix (64 values, natural
                    order) or None, display = dict(matrix=None or int, w, h) or None, ext = False writes the header alone (MPEG-1)
    ("gop", dict)   group_of_pictures_header: closed_gop (0)
    ("pic", dict)   picture_header + picture_coding_extension [+ quant_matrix_extension] + slices: type "I" / "P" / "B", temporal_reference,
                    f_code ((h, v) forward, (h, v) backward; 15 = unused), intra_dc_precision, picture_structure (3), top_field_first,
                    frame_pred_frame_dct (1), concealment_mv, q_scale_type, intra_vlc_format, alternate_scan, repeat_first_field,
                    progressive_frame (1), qme = dict(intra=..., non_intra=...) or None, slices = [slice]
    ("raw", bytes)  bytes as they are (user data, other extensions, damage)
    ("end", None)   sequence_end_code
A slice is dict(row, qcode, mbs=[mb]); a macroblock is dict(x, ...) with x its column.  Columns left out between two macroblocks of a slice are
skipped macroblocks.  Keys of a macroblock: intra (False); fwd / bwd: None, [(x, y)] frame prediction or [(select, x, y), (select, x, y)] field
prediction, vectors in half samples (a field vector's y in lines of its field); field_dct (0); qcode (None: unchanged); blocks = {k: 64 QF levels in
natural order} (an intra macroblock: QF[0] is the DC level itself, all six blocks are written); conceal = (x, y) concealment vector of an intra
macroblock; motion_type to force frame_motion_type (3 = dual prime, written without vectors' dmv: for the refusal test only)."""
import numpy as np

import mpeg2_ref as R


class Writer:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        if n:
            self.bits.append(format(v & ((1 << n) - 1), "0%db" % n))

    def code(self, s):
        self.bits.append(s)

    def bytes(self):
        s = "".join(self.bits)
        s += "0" * (-len(s) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


def _unit(code, w):
    return b"\x00\x00\x01" + bytes([code]) + w.bytes()


def _matrix(w, m):
    for k in range(64):
        w.put(int(m[R.ZIGZAG[k]]), 8)


def seq_units(s):
    w = Writer()
    width, height = s["width"], s["height"]
    w.put(width & 0xFFF, 12), w.put(height & 0xFFF, 12), w.put(s.get("aspect", 1), 4), w.put(s.get("frame_rate_code", 3), 4)
    w.put(0x3FFFF, 18), w.put(1, 1), w.put(112, 10), w.put(0, 1)
    for key in ("intra_matrix", "non_intra_matrix"):
        m = s.get(key)
        w.put(1 if m is not None else 0, 1)
        if m is not None:
            _matrix(w, m)
    out = _unit(0xB3, w)
    if not s.get("ext", True):
        return out
    w = Writer()
    w.put(1, 4), w.put(s.get("profile_level", 0x48), 8), w.put(s.get("progressive_sequence", 1), 1), w.put(s.get("chroma_format", 1), 2)
    w.put(width >> 12, 2), w.put(height >> 12, 2), w.put(0, 12), w.put(1, 1), w.put(0, 8), w.put(0, 1)
    fr = s.get("fr_ext", (0, 0))
    w.put(fr[0], 2), w.put(fr[1], 5)
    out += _unit(0xB5, w)
    d = s.get("display")
    if d is not None:
        w = Writer()
        w.put(2, 4), w.put(5, 3), w.put(1 if d.get("matrix") is not None else 0, 1)
        if d.get("matrix") is not None:
            w.put(d.get("primaries", 1), 8), w.put(d.get("transfer", 1), 8), w.put(d["matrix"], 8)
        w.put(d.get("w", width), 14), w.put(1, 1), w.put(d.get("h", height), 14)
        out += _unit(0xB5, w)
    return out


class _PicWriter:
    def __init__(self, seq, p):
        self.p, self.seq = p, seq
        self.mb_w = (seq["width"] + 15) // 16
        self.t = {"I": 1, "P": 2, "B": 3, "D": 4}[p["type"]]
        self.f_code = p.get("f_code", ((15, 15), (15, 15)))

    def header(self):
        p, w = self.p, Writer()
        w.put(p.get("temporal_reference", 0), 10), w.put(self.t, 3), w.put(0xFFFF, 16)
        if self.t in (2, 3):
            w.put(7, 4)
        if self.t == 3:
            w.put(7, 4)
        w.put(0, 1)
        out = _unit(0x00, w)
        if not p.get("ext", True):
            return out
        w = Writer()
        w.put(8, 4)
        for s in range(2):
            for t in range(2):
                w.put(self.f_code[s][t], 4)
        w.put(p.get("intra_dc_precision", 0), 2), w.put(p.get("picture_structure", 3), 2), w.put(p.get("top_field_first", 0), 1)
        w.put(p.get("frame_pred_frame_dct", 1), 1), w.put(p.get("concealment_mv", 0), 1), w.put(p.get("q_scale_type", 0), 1)
        w.put(p.get("intra_vlc_format", 0), 1), w.put(p.get("alternate_scan", 0), 1), w.put(p.get("repeat_first_field", 0), 1)
        w.put(1, 1), w.put(p.get("progressive_frame", 1), 1), w.put(0, 1)
        out += _unit(0xB5, w)
        q = p.get("qme")
        if q is not None:
            w = Writer()
            w.put(3, 4)
            for key in ("intra", "non_intra"):
                w.put(1 if q.get(key) is not None else 0, 1)
                if q.get(key) is not None:
                    _matrix(w, q[key])
            w.put(0, 2)
            out += _unit(0xB5, w)
        return out

    # -- motion --
    def _component(self, w, f_code, pred, v):
        f = 1 << (f_code - 1)
        delta = v - pred
        if delta < -16 * f:
            delta += 32 * f
        elif delta > 16 * f - 1:
            delta -= 32 * f
        if delta == 0:
            w.code(R.B10[0])
            return
        a = abs(delta) - 1
        w.code(R.B10[a // f + 1]), w.put(1 if delta < 0 else 0, 1), w.put(a % f, f_code - 1)

    def _vectors(self, w, s, vecs):
        field = len(vecs[0]) == 3
        for r, v in enumerate(vecs):
            if field:
                w.put(v[0], 1)
            x, y = v[-2], v[-1]
            self._component(w, self.f_code[s][0], self.pmv[r][s][0], x)
            self._component(w, self.f_code[s][1], self.pmv[r][s][1] >> 1 if field else self.pmv[r][s][1], y)
            self.pmv[r][s] = [x, 2 * y if field else y]
        if not field:
            self.pmv[1][s] = list(self.pmv[0][s])

    # -- blocks --
    def _block(self, w, k, intra, QF):
        p = self.p
        scan = R.SCAN[p.get("alternate_scan", 0)]
        table = R.B15 if intra and p.get("intra_vlc_format", 0) else R.B14
        start = 0
        if intra:
            cc = 0 if k < 4 else k - 3
            diff = int(QF[0]) - self.dc[cc]
            self.dc[cc] = int(QF[0])
            size = 0 if diff == 0 else abs(diff).bit_length()
            w.code((R.B12 if k < 4 else R.B13)[size])
            if size:
                w.put(diff if diff > 0 else diff + (1 << size) - 1, size)
            start = 1
        run, first = 0, not intra
        for n in range(start, 64):
            level = int(QF[scan[n]])
            if level == 0:
                run += 1
                continue
            if first and run == 0 and abs(level) == 1:
                w.code("1"), w.put(1 if level < 0 else 0, 1)
            elif (run, abs(level)) in table:
                w.code(table[(run, abs(level))]), w.put(1 if level < 0 else 0, 1)
            else:
                w.code(table[R.ESC]), w.put(run, 6), w.put(level, 12)
            run, first = 0, False
        w.code(table[R.EOB])

    def _macroblock(self, w, mb, inc):
        p = self.p
        while inc > 33:
            w.code(R.B1_ESCAPE)
            inc -= 33
        w.code(R.B1[inc])
        intra = bool(mb.get("intra"))
        fwd, bwd, blocks = mb.get("fwd"), mb.get("bwd"), mb.get("blocks", {})
        coded = [k for k in range(6) if intra or (k in blocks and np.any(np.asarray(blocks[k]) != 0))]
        cbp = sum(32 >> k for k in coded)
        quant = mb.get("qcode") is not None and (intra or cbp)
        key = (int(bool(quant)), int(fwd is not None and not intra), int(bwd is not None and not intra), int(bool(cbp) and not intra), int(intra))
        w.code({1: R.B2, 2: R.B3, 3: R.B4}[self.t][key])
        fpfd = p.get("frame_pred_frame_dct", 1)
        if (key[1] or key[2]) and not fpfd:
            field = len((fwd or bwd)[0]) == 3
            w.put(mb.get("motion_type", 1 if field else 2), 2)
        if not fpfd and (intra or cbp):
            w.put(mb.get("field_dct", 0), 1)
        if quant:
            w.put(mb["qcode"], 5)
        if mb.get("motion_type") == 3:
            return                                                     # (dual prime: the decoder refuses here)
        if intra:
            if p.get("concealment_mv", 0):
                self._vectors(w, 0, [mb.get("conceal", (0, 0))])
                w.put(mb.get("marker", 1), 1)
            else:
                self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        else:
            self.dc = [1 << (p.get("intra_dc_precision", 0) + 7)] * 3
            if key[1]:
                self._vectors(w, 0, fwd)
            if key[2]:
                self._vectors(w, 1, bwd)
            if not key[1] and not key[2]:
                self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        if cbp and not intra:
            w.code(R.B9[cbp])
        for k in coded:
            self._block(w, k, intra, blocks.get(k, [128 << p.get("intra_dc_precision", 0)] + [0] * 63) if intra else blocks[k])

    def slice(self, sl):
        p, w = self.p, Writer()
        w.put(sl.get("qcode", 4), 5), w.put(0, 1)
        self.dc = [1 << (p.get("intra_dc_precision", 0) + 7)] * 3
        self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        prev = -1
        for mb in sl["mbs"]:
            skipped = mb["x"] - prev - 1 if prev >= 0 else 0
            if skipped:                                                # what a decoder does at a skipped macroblock (7.6.6)
                self.dc = [1 << (p.get("intra_dc_precision", 0) + 7)] * 3
                if self.t == 2:
                    self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
            self._macroblock(w, mb, mb["x"] - prev if prev >= 0 else mb["x"] + 1)
            prev = mb["x"]
        return _unit(sl["row"] + 1, w)

    def bytes(self):
        return self.header() + b"".join(self.slice(s) if isinstance(s, dict) else s for s in self.p.get("slices", []))


def build(items):
    out, seq = b"", None
    for kind, v in items:
        if kind == "seq":
            seq = v
            out += seq_units(v)
        elif kind == "gop":
            w = Writer()
            w.put(0, 25), w.put(v.get("closed_gop", 0) if v else 0, 1), w.put(0, 1)
            out += _unit(0xB8, w)
        elif kind == "pic":
            out += _PicWriter(seq, v).bytes()
        elif kind == "raw":
            out += v
        elif kind == "end":
            out += b"\x00\x00\x01\xb7"
    return out


# ---- ready-made scripts ------------------------------------------------------------------------------------------------------------------
def random_block(rng, intra, precision=0, density=0.15, amp=30):
    QF = np.zeros(64, np.int64)
    mask = rng.random(64) < density
    QF[mask] = rng.integers(-amp, amp + 1, int(mask.sum()))
    if intra:
        QF[0] = int(rng.integers(0, 1 << (8 + precision)))
    elif not np.any(QF):
        QF[int(rng.integers(0, 64))] = 1 if rng.random() < 0.5 else -3
    return QF


def random_vector(rng, x, y, w, h, f_code, field):
    """a conforming vector for the macroblock at (x, y) of a w x h picture: inside the picture and inside the f_code's range"""
    out = []
    for pos, size, span, fc in ((x, w, 16, f_code[0]), (y // 2 if field else y, h // 2 if field else h, 8 if field else 16, f_code[1])):
        f = 1 << (fc - 1)
        lo, hi = max(-2 * pos, -16 * f), min(2 * (size - span - pos), 16 * f - 1)
        out.append(int(rng.integers(lo, hi + 1)))
    return tuple(out)


def random_picture(rng, typ, width, height, progressive_sequence=1, **kw):
    """a picture script with every macroblock chosen at random (some skipped), one or two slices per row; vectors conform"""
    mb_w = (width + 15) // 16
    mb_h = (height + 15) // 16 if progressive_sequence else 2 * ((height + 31) // 32)
    W, H = mb_w * 16, mb_h * 16
    p = dict(type=typ, intra_dc_precision=int(rng.integers(0, 4)), q_scale_type=int(rng.integers(0, 2)), intra_vlc_format=int(rng.integers(0, 2)),
             alternate_scan=int(rng.integers(0, 2)), frame_pred_frame_dct=int(rng.integers(0, 2)), concealment_mv=int(rng.integers(0, 2)),
             top_field_first=int(rng.integers(0, 2)), progressive_frame=int(rng.integers(0, 2)))
    p.update(kw)
    fc = lambda: (int(rng.integers(1, 5)), int(rng.integers(1, 4)))       # noqa: E731
    p["f_code"] = (fc() if typ != "I" or p["concealment_mv"] else (15, 15), fc() if typ == "B" else (15, 15))
    prec, slices = p["intra_dc_precision"], []
    for row in range(mb_h):
        cut = int(rng.integers(1, mb_w)) if mb_w > 1 and rng.random() < 0.4 else None
        cur = dict(row=row, qcode=int(rng.integers(1, 32)), mbs=[])
        last_was_intra, last_vx = True, []
        for x in range(mb_w):
            if x == cut:
                slices.append(cur)
                cur = dict(row=row, qcode=int(rng.integers(1, 32)), mbs=[])
                last_was_intra = True
            edge = not cur["mbs"] or x == mb_w - 1 or x + 1 == cut
            # (a skipped macroblock of a B picture repeats the vectors before it: they must conform at its own position too)
            b_ok = not last_was_intra and all(v <= 2 * (W - 16 - x * 16) for v in last_vx)
            if typ != "I" and not edge and rng.random() < 0.2 and (typ == "P" or b_ok):
                continue                                                 # skipped
            mb = dict(x=x)
            if rng.random() < 0.3:
                mb["qcode"] = int(rng.integers(1, 32))
            if typ == "I" or rng.random() < 0.15:
                mb["intra"] = True
                mb["blocks"] = {k: random_block(rng, True, prec) for k in range(6)}
                if p["concealment_mv"]:
                    mb["conceal"] = random_vector(rng, x * 16, row * 16, W, H, p["f_code"][0], False)
                last_was_intra = True
            else:
                field = not p["frame_pred_frame_dct"] and rng.random() < 0.5
                def vec(s):
                    if field:
                        return [(int(rng.integers(0, 2)),) + random_vector(rng, x * 16, row * 16, W, H, p["f_code"][s], True) for _ in range(2)]
                    return [random_vector(rng, x * 16, row * 16, W, H, p["f_code"][s], False)]
                mode = int(rng.integers(0, 3)) if typ == "B" else 0
                if mode in (0, 2):
                    mb["fwd"] = vec(0)
                if mode in (1, 2):
                    mb["bwd"] = vec(1)
                mb["blocks"] = {k: random_block(rng, False) for k in range(6) if rng.random() < 0.4}
                if typ == "P" and rng.random() < 0.2 and mb["blocks"]:
                    del mb["fwd"]                                        # "no MC, coded": the zero vector
                last_was_intra, last_vx = False, [v[0][-2] for v in (mb.get("fwd"), mb.get("bwd")) if v is not None]
            if not p["frame_pred_frame_dct"]:
                mb["field_dct"] = int(rng.integers(0, 2))
            cur["mbs"].append(mb)
        slices.append(cur)
    p["slices"] = slices
    return p


def random_stream(seed, max_size=64, max_pictures=4):
    rng = np.random.default_rng(seed)
    prog = int(rng.integers(0, 2))
    width, height = int(rng.integers(1, max_size // 2 + 1)) * 2, int(rng.integers(1, max_size // 2 + 1)) * 2
    seq = dict(width=width, height=height, progressive_sequence=prog, frame_rate_code=int(rng.integers(1, 9)))
    if rng.random() < 0.3:
        seq["intra_matrix"] = rng.integers(1, 256, 64)
    if rng.random() < 0.3:
        seq["non_intra_matrix"] = rng.integers(1, 256, 64)
    n = int(rng.integers(1, max_pictures + 1))
    types = ["I"] + [("P", "B")[int(rng.integers(0, 2))] if i >= 2 else "P" for i in range(1, n)]
    items = [("seq", seq)]
    for i, t in enumerate(types):
        items.append(("pic", random_picture(rng, t, width, height, prog, temporal_reference=i)))
    return build(items)


# ---- the scripted cases both test files use: name -> stream --------------------------------------------------------------------------
def _flat_intra(x, value, precision=0, **kw):
    """an intra macroblock whose six blocks are flat: DC-only, level value << precision (intra_dc_mult brings it back to 8 * value)"""
    return dict(x=x, intra=True, blocks={k: [value << precision] + [0] * 63 for k in range(6)}, **kw)


def staircase(width, height, precision=0, base=40, step=7, **kw):
    """an I picture of flat macroblocks, each with its own value: what it decodes to is known without a decoder (value of macroblock (x, y):
    base + step * (y * mb_w + x), staircase_frame)"""
    mb_w, mb_h = (width + 15) // 16, (height + 15) // 16
    return dict(type="I", intra_dc_precision=precision, slices=[dict(row=r, qcode=4, mbs=[_flat_intra(x, base + step * (r * mb_w + x), precision)
                                                                                         for x in range(mb_w)]) for r in range(mb_h)], **kw)


def sized_stream(seed, width, height, prog, types="IPBB"):
    rng = np.random.default_rng(seed)
    items = [("seq", dict(width=width, height=height, progressive_sequence=prog))]
    for i, t in enumerate(types):
        items.append(("pic", random_picture(rng, t, width, height, prog, temporal_reference=i)))
    return build(items)


def chain_stream(seed=77, width=48, height=32, n=12):
    """I B B P B B P ... in coding order I P B B P B B ...: every anchor predicts from the one before, every B from both"""
    rng = np.random.default_rng(seed)
    items = [("seq", dict(width=width, height=height)), ("gop", dict(closed_gop=1))]
    types = ["I"] + [t for _ in range(n) for t in "PBB"]
    for i, t in enumerate(types[:n]):
        items.append(("pic", random_picture(rng, t, width, height, 1, temporal_reference=i)))
    return build(items)


def _fit(v, x, r, cols, rows):
    """the vector with a component's sign turned where it would leave the picture at macroblock column x of cols / row r of rows"""
    vx, vy = v[-2], v[-1]
    if (vx > 0 and x == cols - 1) or (vx < 0 and x == 0):
        vx = -vx
    if (vy > 0 and r == rows - 1) or (vy < 0 and r == 0):
        vy = -vy
    return tuple(v[:-2]) + (vx, vy)


def feature_cases():
    rng = np.random.default_rng(0x4D32)
    W, H = 48, 32
    seq = dict(width=W, height=H)
    out = {}

    def one(name, pics, s=None):
        out[name] = build([("seq", s or seq)] + [("pic", p) for p in pics])
    for p in range(4):
        one(f"i_dc_precision_{p}", [random_picture(rng, "I", W, H, intra_dc_precision=p)])
    one("i_q_scale_type", [random_picture(rng, "I", W, H, q_scale_type=1)])
    one("i_alternate_scan", [random_picture(rng, "I", W, H, alternate_scan=1)])
    one("i_intra_vlc_format", [random_picture(rng, "I", W, H, intra_vlc_format=1)])
    one("i_matrices_seq", [random_picture(rng, "I", W, H), random_picture(rng, "P", W, H)],
        dict(seq, intra_matrix=rng.integers(1, 256, 64), non_intra_matrix=rng.integers(1, 256, 64)))
    one("i_matrices_qme", [random_picture(rng, "I", W, H, qme=dict(intra=rng.integers(1, 256, 64), non_intra=rng.integers(1, 256, 64))),
                           random_picture(rng, "P", W, H)])
    pic = random_picture(rng, "I", W, H, frame_pred_frame_dct=0)
    for s in pic["slices"]:
        for mb in s["mbs"]:
            mb["field_dct"] = 1
    one("i_field_dct", [pic], dict(seq, progressive_sequence=0))
    pic = random_picture(rng, "I", W, H, q_scale_type=1, intra_dc_precision=3)
    for s in pic["slices"]:
        s["qcode"] = 31
        for mb in s["mbs"]:
            mb.pop("qcode", None)
            for k in range(6):
                QF = np.zeros(64, np.int64)
                QF[0] = (0, 2047, 1024)[k % 3]
                QF[[1, 8, 63, 37]] = (2047, -2047, 2047, -2046)
                mb["blocks"][k] = QF
    one("i_extreme_levels", [pic, random_picture(rng, "P", W, H)])
    # P: every half-sample phase, from a random (textured) anchor
    anchor = random_picture(rng, "I", W, H)
    for ph, (hx, hy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        mbs = lambda r: [dict(x=x, fwd=[((4 if x == 0 else -6) + hx, (2 if r == 0 else -4) + hy)]) for x in range(3)]      # noqa: E731
        one(f"p_phase_{hx}{hy}", [anchor, dict(type="P", f_code=((2, 2), (15, 15)), slices=[dict(row=r, qcode=3, mbs=mbs(r)) for r in range(2)])])
    # P: vectors that touch each border exactly: every macroblock from the top left corner of the anchor, then every one from its bottom right corner
    pics = [anchor,
            dict(type="P", f_code=((4, 3), (15, 15)), slices=[dict(row=r, qcode=3, mbs=[dict(x=x, fwd=[(-32 * x, -32 * r)]) for x in range(3)]) for r in range(2)]),
            dict(type="P", f_code=((4, 3), (15, 15)), slices=[dict(row=r, qcode=3, mbs=[dict(x=x, fwd=[(2 * (W - 16 - 16 * x), 2 * (H - 16 - 16 * r))])
                                                                                         for x in range(3)]) for r in range(2)])]
    one("p_borders", pics)
    # P: skipped and zero-vector macroblocks ("no MC, coded" and "MC, not coded" with the zero vector)
    blk = lambda: {k: random_block(rng, False) for k in (0, 3, 5)}      # noqa: E731
    one("p_skipped_zero", [anchor, dict(type="P", f_code=((1, 1), (15, 15)), slices=[
        dict(row=0, qcode=5, mbs=[dict(x=0, blocks=blk()), dict(x=2, fwd=[(0, 0)])]),
        dict(row=1, qcode=5, mbs=[dict(x=0, fwd=[(1, -1)]), dict(x=2, blocks=blk())])])])
    one("p_intra_concealment", [random_picture(rng, "I", W, H, concealment_mv=1), random_picture(rng, "P", W, H, concealment_mv=1)])
    seq_i = dict(seq, progressive_sequence=0, height=40)       # coded height 64
    for s0, s1 in ((0, 1), (1, 0)):
        one(f"p_field_pred_{s0}{s1}", [random_picture(rng, "I", W, 40, 0), dict(type="P", frame_pred_frame_dct=0, progressive_frame=0, f_code=((2, 2), (15, 15)), slices=[
            dict(row=r, qcode=3, mbs=[dict(x=x, fwd=[_fit((s0, 3, -1), x, r, 3, 4), _fit((s1, -2, 1), x, r, 3, 4)], blocks={1: random_block(rng, False)}, field_dct=x & 1)
                                      for x in range(3)]) for r in range(4)])], seq_i)
    # B pictures
    a0, a1 = random_picture(rng, "I", W, H), random_picture(rng, "P", W, H)
    fc = ((2, 2), (2, 2))
    fit = lambda v, x, r: None if v is None else [_fit(v[0], x, r, 3, 2)]      # noqa: E731
    brow = lambda r, f, b: dict(row=r, qcode=3, mbs=[dict(x=x, fwd=fit(f, x, r), bwd=fit(b, x, r), blocks=({2: random_block(rng, False)} if x == 1 else {}))      # noqa: E731
                                                     for x in range(3)])
    one("b_forward", [a0, a1, dict(type="B", f_code=fc, slices=[brow(0, [(3, 1)], None), brow(1, [(-3, -2)], None)])])
    one("b_backward", [a0, a1, dict(type="B", f_code=fc, slices=[brow(0, None, [(1, 3)]), brow(1, None, [(-1, -3)])])])
    one("b_both", [a0, a1, dict(type="B", f_code=fc, slices=[brow(0, [(3, 1)], [(1, 2)]), brow(1, [(-3, -1)], [(2, -5)])])])
    one("b_skipped", [a0, a1, dict(type="B", f_code=fc, slices=[
        dict(row=0, qcode=3, mbs=[dict(x=0, fwd=[(5, 3)], bwd=[(1, 2)]), dict(x=2, fwd=[(0, 0)])]),
        dict(row=1, qcode=3, mbs=[dict(x=0, bwd=[(3, -3)]), dict(x=2, bwd=[(0, 0)])])])])
    one("b_field_bidirectional", [random_picture(rng, "I", W, 40, 0), random_picture(rng, "P", W, 40, 0), dict(
        type="B", frame_pred_frame_dct=0, progressive_frame=0, top_field_first=1, f_code=fc, slices=[
            dict(row=r, qcode=3, mbs=[dict(x=x, fwd=[_fit((x & 1, 3, 1), x, r, 3, 4), _fit((1, -2, -1), x, r, 3, 4)], bwd=[_fit((0, 1, 2), x, r, 3, 4), _fit((r & 1, 2, 0), x, r, 3, 4)],
                                           blocks={4: random_block(rng, False)}) for x in range(3)]) for r in range(4)])], seq_i)
    return out


def clamped_stream():
    """a P picture whose vectors reach outside the reference picture on every side: the host clamps them, marks the records and counts an error"""
    rng = np.random.default_rng(0xC1A)
    W, H = 48, 32
    vec = {(0, 0): (-9, -7), (1, 0): (0, -40), (2, 0): (30, -3), (0, 1): (-40, 9), (1, 1): (3, 40), (2, 1): (25, 21)}
    return build([("seq", dict(width=W, height=H)), ("pic", random_picture(rng, "I", W, H)),
                  ("pic", dict(type="P", f_code=((3, 3), (15, 15)), slices=[dict(row=r, qcode=3, mbs=[dict(x=x, fwd=[vec[(x, r)]]) for x in range(3)])
                                                                         for r in range(2)]))])


def truncated_stream():
    """I P P; the first P picture's second slice loses its second half, the last picture a whole slice (macroblocks no slice covers)"""
    rng = np.random.default_rng(0x7C)
    W, H = 48, 48
    pics = [random_picture(rng, t, W, H, 1, temporal_reference=i) for i, t in enumerate("IPP")]
    w1 = _PicWriter(dict(width=W, height=H), pics[1])
    sl = [w1.slice(s) for s in pics[1]["slices"]]
    sl[1] = sl[1][:4 + (len(sl[1]) - 4) // 2]
    w2 = _PicWriter(dict(width=W, height=H), pics[2])
    sl2 = [w2.slice(s) for s in pics[2]["slices"]]
    return (build([("seq", dict(width=W, height=H)), ("pic", pics[0])]) + w1.header() + b"".join(sl) + w2.header() + b"".join(sl2[:-1]))


def size_change_stream():
    return sized_stream(31, 48, 32, 1, "IPB") + sized_stream(32, 80, 48, 0, "IPBB")
