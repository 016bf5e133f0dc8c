"""H.265 inter prediction typed out once more, in numpy int64 and plain integers, for the scripted streams of tests/scripted_hevc.py.

Restated from the clauses and computed from the SCRIPT, never from a bitstream -- not from tools/hevcgen.c, the oracle or the product:
  6.4.1 / 6.4.2           availability in z-scan order and of prediction blocks (the partIdx 1 exception of NxN, MODE_INTRA)
  8.5.3.2.2 - 8.5.3.2.5   merge: singleMCLFlag, the spatial candidates with the merge estimation region, their exclusions and pruning pairs, the
                          temporal candidate with refIdx 0, the combined candidates of Table 8-7 (COMB_L0 / COMB_L1) compared by picture order count, the
                          zero candidates, 8x4 / 4x8 falling back to list 0
  8.5.3.2.6 / 8.5.3.2.7   the motion vector predictor: A0 then A1, unscaled before scaled, list X before list Y, isScaledFlag, B copied into A, B
                          scaled only when neither A0 nor A1 is available, the duplicate, the temporal candidate below two, zeros; uLX modulo 2^16
  8.5.3.2.8 / 8.5.3.2.9   the temporal vector: bottom right inside the CTB row and the picture, then the centre, the 16x16 storage position, the
                          list choice, the collocated block's own reference picture -- its index read in the lists of the SLICE of the collocated
                          picture that holds the block --, the scaling of 8-179 - 8-183
Samples: analytic_hevc.mc14 / weighted; a residual (flat scaling, the slice's QP) through hevc_resid_ref.residual.

``expect`` returns the planes in decode order and one record per prediction unit; the switches make it wrong on purpose.  A motion is the tuple
(pf, (mv0x, mv0y), ref0, (mv1x, mv1y), ref1): pf bit 0 / 1 = predFlagL0 / L1, an unused list has the vector (0, 0) and the index -1."""
import numpy as np

import analytic_hevc as ah
import hevc_intra_ref as ir
import hevc_resid_ref as rr
import scripted_hevc as hw

SWITCHES = ("b0_b1_only_survivor", "b2_at_four", "prune_by_poc", "combined_by_index", "zero_max", "small_by_region", "col_not_rounded", "ln_lx_swapped", "td_unclipped", "scale_arithmetic_shift", "a_scaled_first", "br_across_ctb_row", "col_poc_from_first_slice")
UNOBSERVABLE = ("b_scaled_when_a_empty",)                           # isScaledFlag read as "A gave nothing": the same without long-term pictures (the host test shows it)
COMB_L0 = (0, 1, 0, 2, 1, 2, 0, 3, 1, 3, 2, 3)                      # Table 8-7: l0CandIdx, l1CandIdx by combIdx
COMB_L1 = (1, 0, 2, 0, 2, 1, 3, 0, 3, 1, 3, 2)


def clip3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


def scale_mv(mv, td, tb, sw={}):
    """8-179 - 8-183 (the same form in 8.5.3.2.7): -> (vector, distScaleFactor before its clip, whether the vector clip cut)"""
    if not sw.get("td_unclipped"):
        td = clip3(-128, 127, td)
    tb = clip3(-128, 127, tb)
    q = (16384 + (abs(td) >> 1)) // abs(td)                         # "/": towards zero
    tx = q if td > 0 else -q
    raw = (tb * tx + 32) >> 6
    dsf = clip3(-4096, 4095, raw)
    out, cut = [], False
    for v in mv:
        p = dsf * v
        s = (p + 127) >> 8 if sw.get("scale_arithmetic_shift") else (1 if p > 0 else -1 if p < 0 else 0) * ((abs(p) + 127) >> 8)
        cut = cut or not -32768 <= s <= 32767
        out.append(clip3(-32768, 32767, s))
    return tuple(out), raw, cut


def wrap16(v):
    u = (v + 65536) % 65536                                         # 8-94 .. 8-97
    return u - 65536 if u >= 32768 else u


class Field:
    """What a decoded picture keeps for later ones: per 4x4 block the motion and the POCs its reference indices meant in ITS slice"""

    def __init__(self, W, H):
        self.pf = np.full((H // 4, W // 4), -1, np.int64)           # -1: not decoded yet; 0: intra
        self.mv = np.zeros((H // 4, W // 4, 2, 2), np.int64)
        self.ref = np.full((H // 4, W // 4, 2), -1, np.int64)
        self.poc = np.zeros((H // 4, W // 4, 2), np.int64)
        self.poc_first = np.zeros((H // 4, W // 4, 2), np.int64)    # (what the indices would mean in the lists of the picture's FIRST slice)

    def at(self, x, y):
        j, i = y >> 2, x >> 2
        return (int(self.pf[j, i]), (int(self.mv[j, i, 0, 0]), int(self.mv[j, i, 0, 1])), int(self.ref[j, i, 0]),
                (int(self.mv[j, i, 1, 0]), int(self.mv[j, i, 1, 1])), int(self.ref[j, i, 1]))


class Pic:
    def __init__(self, seq, pics, k, plans, fields, sw):
        self.seq, self.pics, self.k, self.p, self.pl, self.sw = seq, pics, k, pics[k], plans[k], sw
        self.fields, self.kind, self.poc = fields, pics[k]["kind"], pics[k]["poc"]
        self.W, self.H = hw.coded_size(seq)
        self.g = hw.geometry(seq)
        self.cw, self.ch = hw.ctb_dims(seq)
        self.ctb = self.g["ctb"]
        self.f = Field(self.W, self.H)
        self.starts = [sl["first"] for sl in hw.slice_table(seq, self.p)]
        self.slice_of = hw.slice_map(seq, self.p).reshape(self.ch, self.cw)
        self.slice_lists = {}
        self.par = seq.get("par_mrg_log2", 2)
        self.max_merge = self.p.get("max_merge", 1)
        self.set_slice(0)
        self.first_lists = self.lists
        self.tmvp = bool(seq.get("tmvp", 0) and self.p.get("tmvp", 1) and self.kind != "I")
        self.col = self.p.get("col", (1, 0))

    def set_slice(self, x, y=None):
        """the lists of the slice that holds (x, y) (or of slice number x): a slice activates its own entries (slice_n_ref of the script)"""
        n = x if y is None else self.starts.index(self.slice_of[y >> self.ctb, x >> self.ctb])
        if n not in self.slice_lists:
            spl = hw.slice_plan(self.pl, self.p, n)
            lists = (spl["l0"], spl["l1"] if self.kind == "B" else [])
            self.slice_lists[n] = (lists, all(self.pics[i]["poc"] <= self.poc for l in lists for i in l))
        self.lists, self.no_backward = self.slice_lists[n]

    def ref_poc(self, l, idx):
        return self.pics[self.lists[l][idx]]["poc"]

    # ---- 6.4.1, 6.4.2 ---------------------------------------------------------------------------------------------------------------------------
    def z_avail(self, xc, yc, xn, yn):
        """-> None if available, else why not"""
        if xn < 0 or yn < 0 or xn >= self.W or yn >= self.H:
            return "edge"
        if hw.zscan(xn, yn, self.ctb, self.cw) > hw.zscan(xc, yc, self.ctb, self.cw):
            return "zorder"
        if self.slice_of[yn >> self.ctb, xn >> self.ctb] != self.slice_of[yc >> self.ctb, xc >> self.ctb]:
            return "slice"
        return None

    def pb_avail(self, cb, pb, part_idx, xn, yn):
        (xcb, ycb, n), (xp, yp, w, h) = cb, pb
        if xcb <= xn < xcb + n and ycb <= yn < ycb + n:
            why = None
            if 2 * w == n and 2 * h == n and part_idx == 1 and ycb + h <= yn and xcb + w > xn:
                why = "part2"                                       # the third block of NxN is not decoded when the second one is
        else:
            why = self.z_avail(xp, yp, xn, yn)
        if why is None:
            assert self.f.pf[yn >> 2, xn >> 2] >= 0, (cb, pb, part_idx, xn, yn)
            if self.f.pf[yn >> 2, xn >> 2] == 0:
                why = "intra"
        return why

    # ---- 8.5.3.2.8, 8.5.3.2.9 -------------------------------------------------------------------------------------------------------------------
    def temporal(self, pb, l, ref_idx, rules):
        """mvLXCol or None"""
        if not self.tmvp:
            rules.append("col:off")
            return None
        from_l0, cidx = self.col
        col_k = self.lists[0 if from_l0 or self.kind != "B" else 1][cidx]
        col = self.fields[col_k]
        xp, yp, w, h = pb
        rnd = (lambda v: v) if self.sw.get("col_not_rounded") else (lambda v: (v >> 4) << 4)

        def from_block(x, y, where):
            m = col.at(rnd(x), rnd(y))
            if m[0] <= 0:
                rules.append(f"col:{where}:intra")
                return None
            if not m[0] & 1:
                lc, why = 1, "uni1"
            elif not m[0] & 2:
                lc, why = 0, "uni0"
            elif self.no_backward != bool(self.sw.get("ln_lx_swapped")):
                lc, why = l, "bi:nobackward"                        # mvLXCol: the list this process is invoked for
            else:
                lc, why = from_l0, f"bi:collocated_from_l0={from_l0}"         # mvLNCol with N = collocated_from_l0_flag
            mv = m[1 + 2 * lc]
            own, first = int(col.poc[rnd(y) >> 2, rnd(x) >> 2, lc]), int(col.poc_first[rnd(y) >> 2, rnd(x) >> 2, lc])
            col_diff = self.pics[col_k]["poc"] - (first if self.sw.get("col_poc_from_first_slice") else own)
            tail = f":nobackward={int(self.no_backward)}:from_l0={from_l0}" + (":own slice decides" if own != first else "")
            cur_diff = self.poc - self.ref_poc(l, ref_idx)
            tag = f"col:{where}:{why}:L{lc}"
            if col_diff == cur_diff:
                rules.append(tag + ":unscaled" + tail)
                return mv
            out, raw, cut = scale_mv(mv, col_diff, cur_diff, self.sw)
            notes = [n for n, c in (("td<0", col_diff < 0), ("td>127", abs(col_diff) > 127 or abs(cur_diff) > 127), ("factor>4095", raw > 4095),
                                    ("factor<-4096", raw < -4096), ("vector clipped", cut),
                                    ("roundings differ", scale_mv(mv, col_diff, cur_diff, dict(self.sw, scale_arithmetic_shift=1))[0] != out)) if c]
            rules.append(tag + ":scaled" + "".join(":" + n for n in notes) + tail)
            return out
        xbr, ybr = xp + w, yp + h
        got = None
        if (yp >> self.ctb) != (ybr >> self.ctb) and not self.sw.get("br_across_ctb_row"):
            rules.append("col:br:ctbrow")
        elif ybr >= self.H:
            rules.append("col:br:bottom")
        elif xbr >= self.W:
            rules.append("col:br:right")
        else:
            got = from_block(xbr, ybr, "br")
        if got is None:
            got = from_block(xp + (w >> 1), yp + (h >> 1), "centre")
        if got is None:
            rules.append("col:none")
        return got

    # ---- 8.5.3.2.2 - 8.5.3.2.5 ------------------------------------------------------------------------------------------------------------------
    def same(self, a, b):
        if self.sw.get("prune_by_poc"):
            key = lambda m: (m[0], m[1] if m[0] & 1 else 0, self.ref_poc(0, m[2]) if m[0] & 1 else 0, m[3] if m[0] & 2 else 0, self.ref_poc(1, m[4]) if m[0] & 2 else 0)
            return key(a) == key(b)
        return a == b

    def merge(self, cb, pb, part, part_idx, idx):
        """-> (motion, candidate list, rules)"""
        rules = []
        orig = pb
        if self.par > 2 and cb[2] == 8:
            pb, part, part_idx = (cb[0], cb[1], 8, 8), "2Nx2N", 0   # singleMCLFlag
            rules.append("single")
        xp, yp, w, h = pb
        pos = dict(A1=(xp - 1, yp + h - 1), B1=(xp + w - 1, yp - 1), B0=(xp + w, yp - 1), A0=(xp - 1, yp + h), B2=(xp - 1, yp - 1))
        av, mo = {}, {}
        for name, (xn, yn) in pos.items():
            why = self.pb_avail(cb, pb, part_idx, xn, yn)
            if why is None and (xp >> self.par, yp >> self.par) == (xn >> self.par, yn >> self.par):
                why = "region"
            if why is None and part_idx == 1 and ((name == "A1" and part in ("Nx2N", "nLx2N", "nRx2N")) or (name == "B1" and part in ("2NxN", "2NxnU", "2NxnD"))):
                why = "second"
            av[name] = why is None
            if why is None:
                mo[name] = self.f.at(xn, yn)
            else:
                rules.append(f"{name}:unavailable:{why}")
        cands, flags = [], {}
        pairs = dict(A1=(), B1=("A1",), B0=("B1",), A0=("A1",), B2=("A1", "B1"))
        for name in ("A1", "B1", "B0", "A0", "B2"):
            flags[name] = False
            if not av[name]:
                continue
            if name == "B2":
                four = sum(flags[n] for n in ("A0", "A1", "B0", "B1")) == 4
                rules.append("B2:at:%d" % sum(flags[n] for n in ("A0", "A1", "B0", "B1")))
                if four and not self.sw.get("b2_at_four"):
                    rules.append("B2:refused:four")
                    continue
            hit = None
            for other in pairs[name]:
                present = flags[other] if self.sw.get("b0_b1_only_survivor") and (name, other) == ("B0", "B1") else av[other]
                if present:
                    eq = self.same(mo[other], mo[name])
                    rules.append(f"{name}:{'equal' if eq else 'unequal'}:{other}" + ("" if flags[other] else ":dropped"))
                    hit = hit or (other if eq else None)
            if hit:
                continue
            flags[name] = True
            cands.append((name, mo[name]))
        sub = []                                                    # (the clause derives Col whatever the count; merge_idx cannot reach past MaxNumMergeCand)
        c0 = self.temporal(pb, 0, 0, sub)
        c1 = self.temporal(pb, 1, 0, sub) if self.kind == "B" else None
        rules += ["merge:" + r for r in sub]
        if c0 is not None or c1 is not None:
            cands.append(("Col", ((1 if c0 is not None else 0) | (2 if c1 is not None else 0), c0 or (0, 0), 0 if c0 is not None else -1,
                                  c1 or (0, 0), 0 if c1 is not None else -1)))
        cands = cands[:self.max_merge]
        n_orig = len(cands)
        if self.kind == "B" and 1 < n_orig < self.max_merge:
            comb = 0
            while True:
                a, b = cands[COMB_L0[comb]][1], cands[COMB_L1[comb]][1]
                if a[0] & 1 and b[0] & 2:
                    differ = (a[2] != b[4]) if self.sw.get("combined_by_index") else (self.ref_poc(0, a[2]) != self.ref_poc(1, b[4]))
                    if differ or a[1] != b[3]:
                        cands.append((f"comb{comb}", (3, a[1], a[2], b[3], b[4])))
                    else:
                        rules.append(f"comb{comb}:refused:" + ("same index" if a[2] == b[4] else "same POC at different indices"))
                comb += 1
                if comb == n_orig * (n_orig - 1) or len(cands) == self.max_merge:
                    break
        n_ref = len(self.lists[0]) if self.kind == "P" else min(len(self.lists[0]), len(self.lists[1]))
        zero = 0
        while len(cands) < self.max_merge:
            r = zero if zero < n_ref else 0
            m = (1, (0, 0), r, (0, 0), -1) if self.kind == "P" else (3, (0, 0), r, (0, 0), r)
            if self.sw.get("zero_max") and self.kind == "B":        # (wrong on purpose: each list counts up to its own size)
                m = (3, (0, 0), zero if zero < len(self.lists[0]) else 0, (0, 0), zero if zero < len(self.lists[1]) else 0)
            cands.append((f"zero{zero}" + ("" if zero < n_ref else ":past"), m))
            zero += 1
        name, m = cands[idx]
        size = (w, h) if self.sw.get("small_by_region") else orig[2:]
        if m[0] == 3 and size[0] + size[1] == 12:
            m = (1, m[1], m[2], (0, 0), -1)
            rules.append("small:list0")
        rules.append("chosen:" + name)
        return m, cands, rules

    # ---- 8.5.3.2.6, 8.5.3.2.7 -------------------------------------------------------------------------------------------------------------------
    def mvp(self, cb, pb, part_idx, l, ref_idx, flag):
        """-> (predictor, candidate list [(source, vector)], rules)"""
        rules = []
        xp, yp, w, h = pb
        target = self.ref_poc(l, ref_idx)
        pos = dict(A0=(xp - 1, yp + h), A1=(xp - 1, yp + h - 1), B0=(xp + w, yp - 1), B1=(xp + w - 1, yp - 1), B2=(xp - 1, yp - 1))
        mo = {n: self.f.at(*q) for n, q in pos.items() if self.pb_avail(cb, pb, part_idx, *q) is None}

        def unscaled(names):
            for n in names:
                if n in mo:
                    for lst in (l, 1 - l):
                        if (mo[n][0] >> lst) & 1 and self.ref_poc(lst, mo[n][2 + 2 * lst]) == target:
                            return n, mo[n][1 + 2 * lst], f"{n}:{'X' if lst == l else 'Y'}"
            return None

        def scaled(names):
            for n in names:
                if n in mo:
                    for lst in (l, 1 - l):
                        if (mo[n][0] >> lst) & 1:
                            poc = self.ref_poc(lst, mo[n][2 + 2 * lst])
                            mv = mo[n][1 + 2 * lst]
                            if poc != target:
                                mv = scale_mv(mv, self.poc - poc, self.poc - target, self.sw)[0]
                            return n, mv, f"{n}:{'X' if lst == l else 'Y'}:" + ("scaled" if poc != target else "same")
            return None
        is_scaled = "A0" in mo or "A1" in mo
        a = (scaled(("A0", "A1")) or unscaled(("A0", "A1"))) if self.sw.get("a_scaled_first") else (unscaled(("A0", "A1")) or scaled(("A0", "A1")))
        if self.sw.get("b_scaled_when_a_empty"):
            is_scaled = a is not None
        b = unscaled(("B0", "B1", "B2"))
        if not is_scaled:
            if b is not None:
                a = (b[0], b[1], b[2] + ":copied to A")
            b = scaled(("B0", "B1", "B2"))
            if b is not None:
                b = (b[0], b[1], b[2] + ":B pass 2")
        cands = []
        if a is not None:
            cands.append((a[2], a[1]))
        if b is not None:
            if a is not None and a[1] == b[1]:
                rules.append("mvp:duplicate removed")
            else:
                cands.append((b[2], b[1]))
        if len(cands) < 2:
            sub = []
            c = self.temporal(pb, l, ref_idx, sub)
            rules += ["mvp:" + r for r in sub]
            if c is not None:
                cands.append(("Col", c))
        while len(cands) < 2:
            cands.append(("zero", (0, 0)))
        rules.append(f"mvp:chosen:{cands[flag][0]}:flag{flag}")
        return cands[flag][1], cands, rules


def expect(seq, pics, post=None, **sw):
    """-> ([(Y, Cb, Cr)] per picture in DECODE order, coded size, uint8; [one record per prediction unit, in decoding order]).
    post(k, planes, dict(field=the picture's Field)) -> the planes that picture k leaves for later pictures and for the output (tests/hevc_loop_ref.py:
    the loop filters); by default the reconstruction itself"""
    assert all(k in SWITCHES + UNOBSERVABLE for k in sw), sw
    assert not seq.get("cu_qp_delta", 0) and seq.get("scaling_lists") is None and not seq.get("transquant_bypass", 0)
    W, H = hw.coded_size(seq)
    plans = hw.plan(seq, pics)
    out, fields, records = [], [], []
    flat = {n: np.full((n, n), 16, np.int64) for n in (4, 8, 16, 32)}
    for k, (p, pl) in enumerate(zip(pics, plans)):
        P = Pic(seq, pics, k, plans, fields, sw)
        planes = [np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)]
        kind = p["kind"]
        explicit = bool((kind == "P" and seq.get("weighted_pred", 0)) or (kind == "B" and seq.get("weighted_bipred", 0)))
        wp = p.get("wp", dict(ld_y=0, ld_c=0))
        qp = p.get("qp", seq.get("init_qp", 26))
        qpc = [qp] + [rr.chroma_qp(qp, seq.get(n, 0) + p.get(n, 0)) for n in ("cb_qp_offset", "cr_qp_offset")]
        n_tiles = 0
        for (x, y, log2, depth, u) in hw.walk(seq, p):
            n, t = 1 << log2, u["t"]
            P.set_slice(x, y)
            area = [(slice(y >> s, (y + n) >> s), slice(x >> s, (x + n) >> s)) for s in (0, 1, 1)]
            if t == "pcm":
                for c, name in enumerate(("y", "cb", "cr")):
                    planes[c][area[c]] = u[name]
                P.f.pf[y >> 2:(y + n) >> 2, x >> 2:(x + n) >> 2] = 0
                continue
            assert t in ("skip", "inter") and (t == "skip" or "pus" in u), "hevc_inter_ref: PCM, skipped and partitioned inter units only"
            part = "2Nx2N" if t == "skip" else u["part"]
            pus = [dict(merge=u.get("merge", 0))] if t == "skip" else u["pus"]
            for part_idx, ((xp, yp, w, h), pu) in enumerate(zip(hw.partitions(part, x, y, n), pus)):
                cb, pb = (x, y, n), (xp, yp, w, h)
                rec = dict(pic=k, kind=kind, x=xp, y=yp, w=w, h=h, cu=cb, part=part, part_idx=part_idx, skip=t == "skip", merge="merge" in pu, unit=u,
                           explicit=explicit, lists=[])
                if "merge" in pu:
                    m, cands, rules = P.merge(cb, pb, part, part_idx, pu["merge"])
                    rec.update(idx=pu["merge"], cands=cands)
                else:
                    m, rules = [0, (0, 0), -1, (0, 0), -1], []
                    for l, q in enumerate((pu.get("l0"), pu.get("l1"))):
                        if not q:
                            continue
                        assert l == 0 or kind == "B"
                        ref_idx, mvd, flag = q
                        pred, cands, r = P.mvp(cb, pb, part_idx, l, ref_idx, flag)
                        rules += [f"L{l}:" + s for s in r]
                        s = (pred[0] + mvd[0], pred[1] + mvd[1])
                        if s != (wrap16(s[0]), wrap16(s[1])):
                            rules.append("mvp:wrapped")
                        m[0] |= 1 << l
                        m[1 + 2 * l], m[2 + 2 * l] = (wrap16(s[0]), wrap16(s[1])), ref_idx
                        rec["lists"].append(dict(l=l, ref_idx=ref_idx, mvd=tuple(mvd), flag=flag, cands=cands))
                    m = tuple(m)
                j0, j1, i0, i1 = yp >> 2, (yp + h) >> 2, xp >> 2, (xp + w) >> 2
                P.f.pf[j0:j1, i0:i1] = m[0]
                for l in (0, 1):
                    P.f.mv[j0:j1, i0:i1, l] = m[1 + 2 * l]
                    P.f.ref[j0:j1, i0:i1, l] = m[2 + 2 * l]
                    P.f.poc[j0:j1, i0:i1, l] = P.ref_poc(l, m[2 + 2 * l]) if (m[0] >> l) & 1 else 0
                    fl = P.first_lists[l]
                    P.f.poc_first[j0:j1, i0:i1, l] = pics[fl[m[2 + 2 * l] % len(fl)]]["poc"] if (m[0] >> l) & 1 else 0
                tiles = [(xp + tx, yp + ty, min(16, w - tx), min(16, h - ty)) for ty in range(0, h, 16) for tx in range(0, w, 16)]
                rec.update(motion=m, rules=rules, tiles=tiles, first_tile=n_tiles,
                           pocs=tuple(P.ref_poc(l, m[2 + 2 * l]) if (m[0] >> l) & 1 else None for l in (0, 1)))
                n_tiles += len(tiles)
                records.append(rec)
                for c in (0, 1, 2):
                    s = 1 if c else 0
                    pr, ent = [None, None], [None, None]
                    ld = wp["ld_y"] if c == 0 else wp["ld_c"]
                    for l in (0, 1):
                        if not (m[0] >> l) & 1:
                            continue
                        pr[l] = ah.mc14(out[P.lists[l][m[2 + 2 * l]]][c], xp >> s, yp >> s, w >> s, h >> s, m[1 + 2 * l], c > 0)
                        lst = wp.get("l%d" % l, [])
                        e = lst[m[2 + 2 * l]] if m[2 + 2 * l] < len(lst) and lst[m[2 + 2 * l]] else {}
                        v = e.get("y") if c == 0 else (e.get("c")[c - 1] if e.get("c") else None)
                        ent[l] = v if v is not None else (1 << ld, 0)
                    planes[c][yp >> s:(yp + h) >> s, xp >> s:(xp + w) >> s] = ah.weighted(pr[0], pr[1], explicit, ld + 6, ent[0], ent[1])
            # ---- the residual of the unit (8.6.2 - 8.6.4.2 through hevc_resid_ref), transform tree of uniform depth
            if t == "inter" and u.get("coef") is not None:
                tu = u.get("tu", 0)
                lg = log2 - tu
                for i, e in enumerate(hw.unit_tus(u, 4 ** tu)):
                    ox, oy = ir.tu_origin(i, tu, log2)
                    blocks = [(0, x + ox, y + oy, 1 << lg)]
                    if lg > 2:
                        blocks += [(c, (x + ox) >> 1, (y + oy) >> 1, 1 << (lg - 1)) for c in (1, 2)]
                    elif i % 4 == 3:
                        blocks += [(c, ((x + ox) & ~7) >> 1, ((y + oy) & ~7) >> 1, 4) for c in (1, 2)]
                    for (c, bx, by, bn) in blocks:
                        if e[c]:
                            lev = np.zeros((bn, bn), np.int64)
                            for (cx, cy), v in e[c].items():
                                lev[cy, cx] = v
                            r = rr.residual(lev, qpc[c], bn.bit_length() - 1, flat[bn], False, c in e["tskip"], False)[0]
                            planes[c][by:by + bn, bx:bx + bn] = np.clip(planes[c][by:by + bn, bx:bx + bn].astype(np.int64) + r, 0, 255)
        out.append(tuple(post(k, planes, dict(field=P.f)) if post else planes))
        fields.append(P.f)
    return out, records


def describe(r):
    m = r["motion"]
    how = f"merge_idx {r['idx']} of [{', '.join(n for n, _ in r['cands'])}]" if r["merge"] else \
        "; ".join(f"L{q['l']} ref_idx {q['ref_idx']} mvd {q['mvd']} mvp_flag {q['flag']} of {q['cands']}" for q in r["lists"])
    return (f"picture {r['pic']} ({r['kind']}) prediction unit {r['part_idx']} of {r['part']} at ({r['x']}, {r['y']}) {r['w']}x{r['h']} in the unit {r['cu']}: {how}; "
            f"motion L0 {m[1]} ref {m[2]} L1 {m[3]} ref {m[4]} (POC {r['pocs']}); rules {r['rules']}")


def difference(seq, pics, frames, fmt, planes, records):
    """None when the display frames are the expected pictures, else a text that names the first prediction unit (decoding order) that holds a wrong
    sample, its record and its 16x16 tile (the index in the picture's list of motion compensation jobs)"""
    if len(frames) != len(pics):
        return f"{len(frames)} frames, the script has {len(pics)}"
    w, h = seq["width"], seq["height"]
    order = sorted(range(len(pics)), key=lambda k: pics[k]["poc"])
    for d, k in enumerate(order):
        got = ir.unpack(seq, frames[d], fmt)
        bad = [planes[k][c][:h >> (c > 0), :w >> (c > 0)] != got[c] for c in range(3)]
        if not any(b.any() for b in bad):
            continue
        for r in records:
            if r["pic"] != k:
                continue
            for ti, (tx, ty, tw, th) in enumerate(r["tiles"]):
                for c in range(3):
                    s = 1 if c else 0
                    blk = bad[c][ty >> s:(ty + th) >> s, tx >> s:(tx + tw) >> s]
                    if blk.any():
                        j = np.argwhere(blk)[0]
                        X, Y = (tx >> s) + j[1], (ty >> s) + j[0]
                        return (f"picture {k} (POC {pics[k]['poc']}) plane {('Y', 'Cb', 'Cr')[c]} sample ({X}, {Y}): got {got[c][Y, X]} expected {planes[k][c][Y, X]}, "
                                f"{int(blk.sum())} samples of the tile differ; tile {r['first_tile'] + ti} at ({tx}, {ty}) {tw}x{th}; in " + describe(r))
        c = [i for i in range(3) if bad[i].any()][0]
        j = np.argwhere(bad[c])[0]
        return f"picture {k} (POC {pics[k]['poc']}) plane {('Y', 'Cb', 'Cr')[c]} sample ({j[1]}, {j[0]}) is wrong outside every prediction unit"
    return None
