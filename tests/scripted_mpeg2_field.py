"""scripted_mpeg2's syntax writer for what option mpeg2_field_pictures decodes: field pictures (picture_structure 1 top, 2 bottom), 16x8 motion
compensation and dual prime with real dmvectors (ISO/IEC 13818-2 6.2.5, 6.3.17.1 - 6.3.17.3).  Items, slices and blocks are scripted_mpeg2's.

Macroblocks of a FIELD picture: a slice's row counts macroblock rows of the field.  field_motion_type is written with every forward or backward
macroblock, dct_type never.  Keys: mode "field" (default; fwd / bwd = [(select, x, y)]), "16x8" (fwd / bwd = [(select, x, y), (select, x, y)]: the
upper and the lower half), "dual" (fwd = [(x, y)], dmv = (dx, dy) each -1, 0 or 1; P pictures).  conceal = (select, x, y).  Every y counts lines of
a field.  Macroblocks of a FRAME picture are scripted_mpeg2's, plus mode "dual" (frame_pred_frame_dct 0; fwd = [(x, y)] in field format, dmv)."""
import numpy as np

import mpeg2_field_ref as F
import scripted_mpeg2 as S
from scripted_mpeg2 import Writer, _unit, random_block      # noqa: F401


class FieldPicWriter(S._PicWriter):
    def __init__(self, seq, p):
        super().__init__(seq, p)
        self.fieldpic = p.get("picture_structure", 3) in (1, 2)

    def _vectors(self, w, s, vecs, mode=None, dmv=None):
        if mode is None:                                               # a frame picture's frame or field vectors: the base class's
            return super()._vectors(w, s, vecs)
        halve = mode == "dual" and not self.fieldpic                   # (field format in a frame picture: the vertical predictor is halved)
        for r, v in enumerate(vecs):
            if mode != "dual":
                w.put(v[0], 1)
            x, y = v[-2], v[-1]
            self._component(w, self.f_code[s][0], self.pmv[r][s][0], x)
            if mode == "dual":
                w.code(F.B11[dmv[0]])
            self._component(w, self.f_code[s][1], self.pmv[r][s][1] >> 1 if halve else self.pmv[r][s][1], y)
            if mode == "dual":
                w.code(F.B11[dmv[1]])
            self.pmv[r][s] = [x, 2 * y if halve else y]
        if len(vecs) == 1:
            self.pmv[1][s] = list(self.pmv[0][s])

    def _macroblock(self, w, mb, inc):
        p = self.p
        if not self.fieldpic and mb.get("mode") != "dual":
            return super()._macroblock(w, mb, inc)
        while inc > 33:
            w.code(S.R.B1_ESCAPE)
            inc -= 33
        w.code(S.R.B1[inc])
        intra = bool(mb.get("intra"))
        fwd, bwd, blocks = mb.get("fwd"), mb.get("bwd"), mb.get("blocks", {})
        coded = [k for k in range(6) if intra or (k in blocks and np.any(np.asarray(blocks[k]) != 0))]
        cbp = sum(32 >> k for k in coded)
        quant = mb.get("qcode") is not None and (intra or cbp)
        key = (int(bool(quant)), int(fwd is not None and not intra), int(bwd is not None and not intra), int(bool(cbp) and not intra), int(intra))
        w.code({1: S.R.B2, 2: S.R.B3, 3: S.R.B4}[self.t][key])
        mode = mb.get("mode", "field")
        if key[1] or key[2]:
            w.put(mb.get("motion_type", {"field": 1, "16x8": 2, "dual": 3}[mode]), 2)      # field_motion_type, or frame_motion_type 3
        if not self.fieldpic and (intra or cbp):
            w.put(mb.get("field_dct", 0), 1)
        if quant:
            w.put(mb["qcode"], 5)
        if intra:
            if p.get("concealment_mv", 0):
                self._vectors(w, 0, [mb.get("conceal", (0, 0, 0))], "field")
                w.put(mb.get("marker", 1), 1)
            else:
                self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        else:
            self.dc = [1 << (p.get("intra_dc_precision", 0) + 7)] * 3
            if key[1]:
                self._vectors(w, 0, fwd, mode, mb.get("dmv"))
            if key[2]:
                self._vectors(w, 1, bwd, mode, mb.get("dmv"))
            if not key[1] and not key[2]:
                self.pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        if cbp and not intra:
            w.code(S.R.B9[cbp])
        for k in coded:
            self._block(w, k, intra, blocks.get(k, [128 << p.get("intra_dc_precision", 0)] + [0] * 63) if intra else blocks[k])


def build(items):
    out, seq = b"", None
    for kind, v in items:
        if kind == "seq":
            seq = v
            out += S.seq_units(v)
        elif kind == "pic":
            out += FieldPicWriter(seq, v).bytes()
        else:
            out += S.build([(kind, v)])
    return out


# ---- conforming vectors -------------------------------------------------------------------------------------------------------------------
def derived(v, dmv, m, e):
    """7.6.3.6, as the restatement has it: the opposite-parity vector of a dual-prime macroblock"""
    return (((v[0] * m + (v[0] > 0)) >> 1) + dmv[0], ((v[1] * m + (v[1] > 0)) >> 1) + e + dmv[1])


def _inside(v, x, y, span, W, size):
    return -2 * x <= v[0] <= 2 * (W - 16 - x) and -2 * y <= v[1] <= 2 * (size - span - y)


def _vector(rng, x, y, span, W, size, f_code):
    out = []
    for pos, total, sp, fc in ((x, W, 16, f_code[0]), (y, size, span, f_code[1])):
        f = 1 << (fc - 1)
        out.append(int(rng.integers(max(-2 * pos, -16 * f), min(2 * (total - sp - pos), 16 * f - 1) + 1)))
    return tuple(out)


def _dual(rng, x, y, span, W, size, f_code, ms_es):
    """a dual-prime vector with its dmvector such that every derived vector stays inside too; ms_es: [(m, e)] of the derived vectors"""
    for _ in range(50):
        v, dmv = _vector(rng, x, y, span, W, size, f_code), (int(rng.integers(-1, 2)), int(rng.integers(-1, 2)))
        if all(_inside(derived(v, dmv, m, e), x, y, span, W, size) for m, e in ms_es):
            return v, dmv
    return None


def random_field_picture(rng, typ, width, height, structure, **kw):
    """one field picture with every macroblock chosen at random among intra, field, 16x8, dual prime (P), skipped and "no MC"; vectors conform"""
    mb_w, mb_h = (width + 15) // 16, ((height + 31) // 32)                     # rows of the field
    W, Hf, par = mb_w * 16, mb_h * 16, structure - 1
    p = dict(type=typ, picture_structure=structure, frame_pred_frame_dct=0, progressive_frame=0, intra_dc_precision=int(rng.integers(0, 4)),
             q_scale_type=int(rng.integers(0, 2)), intra_vlc_format=int(rng.integers(0, 2)), alternate_scan=int(rng.integers(0, 2)),
             concealment_mv=int(rng.integers(0, 2)), top_field_first=0)
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
            b_ok = not last_was_intra and all(v <= 2 * (W - 16 - x * 16) for v in last_vx)
            if typ != "I" and not edge and rng.random() < 0.2 and (typ == "P" or b_ok):
                continue                                                 # skipped
            mb = dict(x=x)
            if rng.random() < 0.3:
                mb["qcode"] = int(rng.integers(1, 32))
            if typ == "I" or rng.random() < 0.12:
                mb["intra"] = True
                mb["blocks"] = {k: random_block(rng, True, prec) for k in range(6)}
                if p["concealment_mv"]:
                    mb["conceal"] = (int(rng.integers(0, 2)),) + _vector(rng, x * 16, row * 16, 16, W, Hf, p["f_code"][0])
                last_was_intra = True
            else:
                mode = ("field", "16x8", "dual")[int(rng.integers(0, 3 if typ == "P" else 2))]
                dual = _dual(rng, x * 16, row * 16, 16, W, Hf, p["f_code"][0], [(1, 1 if par else -1)]) if mode == "dual" else None
                if mode == "dual" and dual is None:
                    mode = "field"
                mb["mode"] = mode

                def vec(s):
                    if mode == "16x8":
                        return [(int(rng.integers(0, 2)),) + _vector(rng, x * 16, row * 16 + 8 * r, 8, W, Hf, p["f_code"][s]) for r in range(2)]
                    return [(int(rng.integers(0, 2)),) + _vector(rng, x * 16, row * 16, 16, W, Hf, p["f_code"][s])]
                if mode == "dual":
                    mb["fwd"], mb["dmv"] = [dual[0]], dual[1]
                else:
                    d = int(rng.integers(0, 3)) if typ == "B" else 0
                    if d in (0, 2):
                        mb["fwd"] = vec(0)
                    if d in (1, 2):
                        mb["bwd"] = vec(1)
                mb["blocks"] = {k: random_block(rng, False) for k in range(6) if rng.random() < 0.4}
                if typ == "P" and rng.random() < 0.15 and mb["blocks"]:
                    del mb["fwd"]                                        # "no MC, coded"
                    mb.pop("dmv", None)
                    mb["mode"] = "field"
                # (a skipped macroblock of a B picture repeats PMV[0]: after 16x8 that is the upper half's vector, a 16-line block further on)
                ok16 = mode != "16x8" or all(v[0][2] <= 2 * (Hf - 16 - row * 16) for v in (mb.get("fwd"), mb.get("bwd")) if v is not None)
                last_was_intra, last_vx = not ok16, [v[0][-2] for v in (mb.get("fwd"), mb.get("bwd")) if v is not None]
            cur["mbs"].append(mb)
        slices.append(cur)
    p["slices"] = slices
    return p


def random_dual_frame_picture(rng, width, height, tff, **kw):
    """a P frame picture (frame_pred_frame_dct 0) in which about half of the predicted macroblocks are dual prime"""
    p = S.random_picture(rng, "P", width, height, 0, frame_pred_frame_dct=0, top_field_first=tff, progressive_frame=0, **kw)
    mb_w, mb_h = (width + 15) // 16, 2 * ((height + 31) // 32)
    W, Hf = mb_w * 16, mb_h * 8
    ms_es = [(1 if tff else 3, -1), (3 if tff else 1, 1)]
    for sl in p["slices"]:
        for mb in sl["mbs"]:
            if mb.get("intra") or mb.get("fwd") is None or rng.random() < 0.5:
                continue
            dual = _dual(rng, mb["x"] * 16, sl["row"] * 8, 8, W, Hf, p["f_code"][0], ms_es)
            if dual is not None:
                mb["mode"], mb["fwd"], mb["dmv"] = "dual", [dual[0]], dual[1]
    return p


def field_stream(seed, width=48, height=64, layout="IP PP BB BB PP", **kw):
    """layout: frames in coding order; two letters = two field pictures (the first one's parity alternates from frame to frame unless `first`
    says it), one letter = a frame picture, "Pd" / "PD" = a P frame picture with dual prime, top_field_first 0 / 1"""
    rng = np.random.default_rng(seed)
    items = [("seq", dict(width=width, height=height, progressive_sequence=0))]
    first = kw.pop("first", None)
    for i, fr in enumerate(layout.split()):
        if fr in ("Pd", "PD"):
            items.append(("pic", random_dual_frame_picture(rng, width, height, int(fr == "PD"))))
        elif len(fr) == 1:
            items.append(("pic", S.random_picture(rng, fr, width, height, 0, temporal_reference=i)))
        else:
            s0 = first if first is not None else 1 + (i & 1)
            for j, t in enumerate(fr):
                items.append(("pic", random_field_picture(rng, t, width, height, s0 if j == 0 else 3 - s0, temporal_reference=i, **kw)))
    return build(items)


# ---- scripted cases both test files use ------------------------------------------------------------------------------------------------------
def fpic(typ, structure, rows, mbs_of_row, **kw):
    """a field picture with one slice per macroblock row of the field"""
    p = dict(type=typ, picture_structure=structure, frame_pred_frame_dct=0, progressive_frame=0, f_code=((4, 4), (4, 4) if typ == "B" else (15, 15)),
             slices=[dict(row=r, qcode=4, mbs=mbs_of_row(r)) for r in range(rows)])
    p.update(kw)
    return p


# The analytic reference: two I field pictures of flat blocks.  Luma of field sample (x, y): TOP[y // 8] + 2 * (x // 8) / BOT[y // 8] + 2 * (x // 8);
# chroma of field chroma sample (x, y): CTOP[y // 8] + 3 * (x // 8) / CBOT[y // 8] + 3 * (x // 8) (Cr: + 9).  48 x 64 coded: 3 x 2 macroblocks and
# 32 luma lines per field.
AW, AH = 48, 64
TOP, BOT = (40, 71, 102, 133), (200, 181, 150, 95)
CTOP, CBOT = (60, 97), (170, 121)
ASEQ = ("seq", dict(width=AW, height=AH, progressive_sequence=0))


def analytic_anchor(first=1):
    """the two I field pictures, the field of parity first - 1 first"""
    def ipic(structure):
        y, c = (TOP, CTOP) if structure == 1 else (BOT, CBOT)

        def blocks(r, x):
            b = {k: [y[2 * r + (k >> 1)] + 2 * (2 * x + (k & 1))] + [0] * 63 for k in range(4)}
            b.update({4: [c[r] + 3 * x] + [0] * 63, 5: [c[r] + 3 * x + 9] + [0] * 63})
            return b
        return ("pic", fpic("I", structure, 2, lambda r: [dict(x=x, intra=True, blocks=blocks(r, x)) for x in range(3)], f_code=((15, 15), (15, 15))))
    return [ASEQ, ipic(first), ipic(3 - first)]


def feature_cases():
    """one stream per feature of the option: name -> stream (each decodes clean)"""
    rng = np.random.default_rng(0xF1E1D)
    W, H = 48, 64
    out = {}
    out["i_p_frame"] = field_stream(11, W, H, "IP")                      # the second field of an I frame is a P field; its same-parity reference: none (128)
    out["i_p_frame_after_anchor"] = field_stream(12, W, H, "II IP PP")
    # the second P field reads the first field of its own frame: every macroblock selects the opposite parity
    second = fpic("P", 2, 2, lambda r: [dict(x=x, fwd=[S._fit((0, 2 * x - 3, 3 - 4 * r), x, r, 3, 2)], blocks={x: random_block(rng, False)}) for x in range(3)])
    out["second_p_reads_own_first_field"] = build([("seq", dict(width=W, height=H, progressive_sequence=0)),
                                                   ("pic", random_field_picture(rng, "I", W, H, 1)), ("pic", random_field_picture(rng, "I", W, H, 2)),
                                                   ("pic", random_field_picture(rng, "P", W, H, 1)), ("pic", second)])
    out["b_fields"] = field_stream(13, W, H, "II PP BB BB")
    out["b_fields_bottom_first"] = field_stream(14, W, H, "II PP BB", first=2)
    dual = lambda s: fpic("P", s, 2, lambda r: [dict(x=x, mode="dual", fwd=[((3, -5, -8)[x], (5, -7)[r])], dmv=((-1, 0, 1)[x], (1, -1)[r]),      # noqa: E731
                                                     blocks={4: random_block(rng, False)}) for x in range(3)])
    out["dual_prime_field_pictures"] = build([("seq", dict(width=W, height=H, progressive_sequence=0)),
                                              ("pic", random_field_picture(rng, "I", W, H, 1)), ("pic", random_field_picture(rng, "I", W, H, 2)),
                                              ("pic", dual(1)), ("pic", dual(2))])
    out["dual_prime_frame_tff0"] = field_stream(15, W, H, "I Pd Pd")
    out["dual_prime_frame_tff1"] = field_stream(16, W, H, "I PD PD")
    m16 = fpic("P", 1, 2, lambda r: [dict(x=x, mode="16x8", fwd=[S._fit((x & 1, 3, (4, -6)[r]), x, r, 3, 2), S._fit((1 - (x & 1), -5, (-3, 2)[r]), x, r, 3, 2)], blocks={1: random_block(rng, False)})
                                     for x in range(3)])
    out["16x8"] = build([("seq", dict(width=W, height=H, progressive_sequence=0)), ("pic", random_field_picture(rng, "I", W, H, 1)),
                         ("pic", random_field_picture(rng, "I", W, H, 2)), ("pic", m16), ("pic", random_field_picture(rng, "P", W, H, 2))])
    # skipped and motion-less macroblocks: P (zero vector, own parity, predictors reset) and B (the direction and vectors before, own parity)
    skip_p = lambda s: fpic("P", s, 2, lambda r: [dict(x=0, fwd=[(1 - r, 5, 3 - 6 * r)]), dict(x=2, blocks={0: random_block(rng, False)})] if r == 0      # noqa: E731
                            else [dict(x=0, blocks={5: random_block(rng, False)}), dict(x=2, fwd=[(r & 1, -3, -3)])])
    skip_b = lambda s: fpic("B", s, 2, lambda r: [dict(x=0, fwd=[(1, 5, 3)], bwd=[(0, 1, 2)]), dict(x=2, fwd=[(0, 0, 0)])] if r == 0      # noqa: E731
                            else [dict(x=0, mode="16x8", bwd=[(1, 3, -3), (0, 2, -1)]), dict(x=2, bwd=[(1, 0, 0)])])
    base = [("seq", dict(width=W, height=H, progressive_sequence=0)), ("pic", random_field_picture(rng, "I", W, H, 1)), ("pic", random_field_picture(rng, "I", W, H, 2))]
    out["skipped_p"] = build(base + [("pic", skip_p(1)), ("pic", skip_p(2))])
    out["skipped_b"] = build(base + [("pic", random_field_picture(rng, "P", W, H, 2)), ("pic", random_field_picture(rng, "P", W, H, 1)),
                                     ("pic", skip_b(1)), ("pic", skip_b(2))])
    out["concealment_vectors"] = build([("seq", dict(width=W, height=H, progressive_sequence=0))] +
                                       [("pic", random_field_picture(rng, t, W, H, s, concealment_mv=1)) for t, s in (("I", 2), ("P", 1), ("P", 2), ("P", 1))])
    return out


def clamped_cases():
    """per mode, vectors that reach outside the reference field on some side: name -> stream"""
    rng = np.random.default_rng(0xC1A3)
    W, H = 48, 64
    base = [("seq", dict(width=W, height=H, progressive_sequence=0)), ("pic", random_field_picture(rng, "I", W, H, 1)), ("pic", random_field_picture(rng, "I", W, H, 2))]
    out = {}
    out["field"] = build(base + [("pic", fpic("P", 1, 2, lambda r: [dict(x=x, fwd=[(x & 1, (-9, 0, 30)[x], (-40, 37)[r])]) for x in range(3)]))])
    out["16x8"] = build(base + [("pic", fpic("P", 1, 2, lambda r: [dict(x=x, mode="16x8", fwd=[(0, (-9, 0, 3)[x], (-3, 1)[r] * 17), (1, 2, (-35, 17)[r])])
                                                                     for x in range(3)]))])
    out["dual_field"] = build(base + [("pic", fpic("P", 2, 2, lambda r: [dict(x=x, mode="dual", fwd=[((-2, 0, 1)[x], (-1, 1)[r])], dmv=((-1, 0, 1)[x], (-1, 1)[r]))
                                                                           for x in range(3)]))])
    frame = dict(type="P", frame_pred_frame_dct=0, progressive_frame=0, top_field_first=1, f_code=((4, 4), (15, 15)),
                 slices=[dict(row=r, qcode=4, mbs=[dict(x=x, mode="dual", fwd=[((-1, 0, 1)[x], (-1, 0, 0, 1)[r])], dmv=((-1, 0, 1)[x], (-1, 0, 0, 1)[r]))
                                                   for x in range(3)]) for r in range(4)])
    out["dual_frame"] = build(base + [("pic", frame)])
    return out


def truncated_field_stream():
    """II PP; the first P field's second slice loses its second half, the second P field a whole slice"""
    rng = np.random.default_rng(0x7F)
    W, H = 48, 96
    seq = dict(width=W, height=H, progressive_sequence=0)
    pics = [random_field_picture(rng, t, W, H, s) for t, s in (("I", 1), ("I", 2), ("P", 1), ("P", 2))]
    w2 = FieldPicWriter(seq, pics[2])
    sl = [w2.slice(s) for s in pics[2]["slices"]]
    sl[1] = sl[1][:4 + (len(sl[1]) - 4) // 2]
    w3 = FieldPicWriter(seq, pics[3])
    sl3 = [w3.slice(s) for s in pics[3]["slices"]]
    return build([("seq", seq), ("pic", pics[0]), ("pic", pics[1])]) + w2.header() + b"".join(sl) + w3.header() + b"".join(sl3[:-1])


def mixed_chain(seed=91, width=48, height=64):
    """12 coded pictures, frame and field pictures, P and B: I-P fields, a P frame with dual prime, a B frame, B fields, P fields, B fields, a B frame,
    a P frame"""
    return field_stream(seed, width, height, "IP PD B BB PP BB B P")


def lone_cases():
    """name -> (stream, display frames, lone fields)"""
    rng = np.random.default_rng(0x10E)
    W, H = 48, 64
    seq = ("seq", dict(width=W, height=H, progressive_sequence=0))
    fld = lambda t, s: ("pic", random_field_picture(rng, t, W, H, s))      # noqa: E731
    frm = lambda t: ("pic", S.random_picture(rng, t, W, H, 0))             # noqa: E731
    return {"first_field_then_flush": (build([seq, fld("I", 1)]), 1, 1),
            "then_a_frame_picture": (build([seq, fld("I", 2), frm("P"), frm("B")]), 3, 1),
            "then_a_same_parity_field": (build([seq, fld("I", 1), fld("P", 1), fld("P", 2)]), 2, 1),
            "b_field_alone": (build([seq, frm("I"), frm("P"), fld("B", 1), frm("B")]), 4, 1),
            "types_that_do_not_pair": (build([seq, fld("I", 1), fld("I", 2), fld("P", 1), fld("I", 2), fld("I", 1)]), 3, 1)}
