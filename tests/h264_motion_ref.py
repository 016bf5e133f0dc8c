"""H.264 motion vector derivation restated from clause 8.4.1 for the scripted streams of tests/scripted_h264.py (frame pictures, CAVLC or not: the
derivation does not know): from the SYNTAX a macroblock states (mb_type, sub_mb_type, ref_idx and mvd per (sub-)partition and list) to refIdxL0 / L1,
predFlag and one vector per 4x4 block and list.  Plain Python; typed from the clauses, not from the writer, the oracle or the product.

    6.4.11.7 / 6.4.12   the neighbouring partitions A, B, C, D of every macroblock, sub-macroblock and sub-partition shape with predPartWidth (16 for
                        P_Skip / B_Skip / B_Direct_16x16 and for a direct sub-macroblock of B_8x8; the sub-partition's width in P_8x8 / B_8x8; else the
                        partition's); a partition later in decoding order, a macroblock of another slice or outside the picture is not available, C
                        falls to D when it is not; an intra neighbour is available and holds refIdx -1
    8.4.1.3             the median; exactly one neighbour with the partition's reference: its vector; B and C both unavailable and A available: A
                        stands for all three; the directional rules of 16x8 (B for the upper, A for the lower partition) and 8x16 (A left, C right),
                        each only when that neighbour's reference index is the partition's
    8.4.1.1             P_Skip: zero when A or B is not available or either has refIdx 0 with a zero vector, else the 16x16 predictor at refIdx 0
    8.4.1.2.2           spatial direct: refIdx = MinPositive over A, B, C of the MACROBLOCK per list; both negative: 0 / 0 and zero vectors; a list that
                        stays negative is unused; colZeroFlag (short-term RefPicList1[0], refIdxCol 0, both components within +-1) zeroes the vector of a
                        list whose refIdx is 0
    8.4.1.2.1           the colocated block in RefPicList1[0] (frames): the corner 4x4 block of the quadrant under direct_8x8_inference_flag, else the
                        block itself; its list 0 motion, its list 1 motion when list 0 is unused, nothing when it is intra
    8.4.1.2.3           temporal direct: refIdxL0 = the index in the CURRENT list 0 of the picture the colocated block referred to, refIdxL1 = 0, tb, td,
                        tx, DistScaleFactor with their clips, mvL0 = (DistScaleFactor * mvCol + 128) >> 8, mvL1 = mvL0 - mvCol; an intra colocated block:
                        refIdx 0 / 0 and zero vectors.  td = 0 needs RefPicList1[0] and the picture its block referred to to share an order count: two
                        different frames of these streams never do, so that branch (and the long-term one) is asserted away, not faked.
    and what a picture leaves behind for later colocated use: per 4x4 block refIdx, the referenced PICTURE and the vector of both lists, intra or not.

``derive`` returns the motion of every picture; tests/analytic_expect.py samples with it.  ``SWITCHES`` are wrong-on-purpose variants: a decoder with
that defect; tests/test_h264_motion_host.py shows that a named case notices each.  Coverage: ``cov`` counts every branch taken, by name.
"""
import scripted_h264 as sw

SWITCHES = [
    "median_even_when_one_matches", "c_not_replaced_by_d", "only_a_rule_dropped", "directional_16x8_8x16_swapped", "directional_without_ref_check",
    "p_skip_without_zero_neighbour_rule", "p_skip_unavailable_and", "later_partition_available", "direct_pred_part_width_of_sub_partition",
    "spatial_min_instead_of_min_positive", "col_zero_any_ref_idx_col", "col_zero_only_zero_vector", "col_zero_ignores_ref_idx", "spatial_direct_own_partitions",
    "col_block_itself_under_inference", "col_list1_never_consulted", "temporal_ref_idx_unmapped", "dist_scale_without_rounding", "mv_l1_sign_swapped",
    "quadrant_list1_only_as_list0"]

INTRA = sw.INTRA


class Field:
    """The motion field of one picture on its 4x4 block grid"""
    def __init__(self, mbw, mbh, lists):
        self.w4, self.h4, self.mbw = mbw * 4, mbh * 4, mbw
        n = self.w4 * self.h4
        self.ref = [[-1] * n, [-1] * n]                             # refIdxLX, -1: list unused (or intra)
        self.pic = [[None] * n, [None] * n]                         # the picture RefPicListX[refIdxLX] was when this picture was decoded
        self.mv = [[(0, 0)] * n, [(0, 0)] * n]
        self.intra = [False] * n
        self.done = [False] * n                                     # decoded so far (availability inside the picture being decoded)
        self.slice_of = [None] * (mbw * mbh)                        # first macroblock of the slice
        self.lists = lists

    def at(self, bx, by):
        return by * self.w4 + bx


def clip3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


def median(a, b, c):
    return sorted((a, b, c))[1]


def min_positive(x, y):
    """8-184"""
    return min(x, y) if x >= 0 and y >= 0 else max(x, y)


def cdiv(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def dist_scale_factor(poc_cur, poc0, poc1, wrong=frozenset()):
    """8-197 .. 8-202 for frames"""
    tb, td = clip3(-128, 127, poc_cur - poc0), clip3(-128, 127, poc1 - poc0)
    assert td != 0, "RefPicList1[0] and the picture its block referred to are different frames: their order counts differ"
    tx = cdiv(16384 + abs(cdiv(td, 2)), td)
    rnd = 0 if "dist_scale_without_rounding" in wrong else 32
    return clip3(-1024, 1023, (tb * tx + rnd) >> 6)


def scale_mv(dsf, mv, wrong=frozenset()):
    rnd = 0 if "dist_scale_without_rounding" in wrong else 128
    return tuple((dsf * c + rnd) >> 8 for c in mv)


class Deriver:
    def __init__(self, seq, pics, pl, k, fields, wrong, cov, mvp_out):
        self.seq, self.pics, self.k, self.p, self.pl = seq, pics, k, pics[k], pl[k]
        self.mbw, self.mbh = (seq["width"] + 15) // 16, (seq["height"] + 15) // 16
        self.F = Field(self.mbw, self.mbh, (list(pl[k]["l0"]), list(pl[k]["l1"])))
        self.fields, self.wrong, self.cov, self.mvp_out = fields, wrong, cov, mvp_out
        self.step = sw.layout_step(seq, self.p)

    def hit(self, name):
        if self.cov is not None:
            self.cov[name] = self.cov.get(name, 0) + 1

    # ---- 6.4.11.7 / 6.4.12 ----
    def available(self, bx, by):
        F = self.F
        if not (0 <= bx < F.w4 and 0 <= by < F.h4):
            return False
        mb = (by // 4) * self.mbw + bx // 4
        if F.slice_of[mb] != F.slice_of[self.cur]:
            return False                                            # another slice, or a macroblock that comes later (no slice yet)
        if F.done[F.at(bx, by)]:
            return True
        if mb == self.cur and "later_partition_available" in self.wrong:
            return True                                             # (holds nothing yet: refIdx -1)
        return False

    def data(self, l, bx, by, avail):
        """(refIdxLXN, mvLXN): -1 and zero for a partition that is not available, intra, or does not use the list"""
        if not avail:
            return -1, (0, 0)
        i = self.F.at(bx, by)
        if not self.F.done[i] or self.F.ref[l][i] < 0:
            return -1, (0, 0)
        return self.F.ref[l][i], self.F.mv[l][i]

    def neighbours(self, l, bx, by, w4):
        """A, B, C of 6.4.11.7 for the (sub-)partition whose upper left block is (bx, by), predPartWidth 4 * w4: [(available, refIdx, mv)] x 3"""
        pos = {"A": (bx - 1, by), "B": (bx, by - 1), "C": (bx + w4, by - 1), "D": (bx - 1, by - 1)}
        av = {n: self.available(*q) for n, q in pos.items()}
        c = "C"
        if not av["C"]:
            self.hit("C_unavailable")
            if 0 <= pos["C"][0] < self.F.w4 and pos["C"][1] >= 0:
                sl = self.F.slice_of[(pos["C"][1] // 4) * self.mbw + pos["C"][0] // 4]
                if sl is not None and sl != self.F.slice_of[self.cur]:
                    self.hit("other_slice_neighbour_C")
            if pos["C"][1] >= 0 and 0 <= pos["C"][0] < self.F.w4 and (pos["C"][1] // 4) * self.mbw + pos["C"][0] // 4 == self.cur:
                self.hit("C_is_a_later_partition")
            if "c_not_replaced_by_d" not in self.wrong:
                c = "D"
                self.hit("C_replaced_by_D_available" if av["D"] else "C_replaced_by_D_unavailable")
        out = []
        for n in ("A", "B", c):
            out.append((av[n],) + self.data(l, *pos[n], av[n]))
            if av[n] and self.F.intra[self.F.at(*pos[n])]:
                self.hit("intra_neighbour_" + ("C" if n == c else n))
            if not av[n] and 0 <= pos[n][0] < self.F.w4 and pos[n][1] >= 0:
                mb = (pos[n][1] // 4) * self.mbw + pos[n][0] // 4
                if self.F.slice_of[mb] is not None and self.F.slice_of[mb] != self.F.slice_of[self.cur]:
                    if n != "C":
                        self.hit("other_slice_neighbour_" + n)
        return out

    # ---- 8.4.1.3 ----
    def predict(self, l, bx, by, w4, ref_idx, shape=None, part=0):
        A, B, C = self.neighbours(l, bx, by, w4)
        if "directional_16x8_8x16_swapped" in self.wrong and shape:
            shape = "8x16" if shape == "16x8" else "16x8"
        if shape:
            N = {("16x8", 0): B, ("16x8", 1): A, ("8x16", 0): A, ("8x16", 1): C}[(shape, part)]
            if N[1] == ref_idx or "directional_without_ref_check" in self.wrong:
                self.hit("directional_%s_part%d_taken" % (shape, part))
                return N[2]
            self.hit("directional_%s_part%d_falls_to_median" % (shape, part))
        if not B[0] and not C[0] and A[0]:
            self.hit("only_A_available")
            if "only_a_rule_dropped" not in self.wrong:
                B = C = A
        same = [N for N in (A, B, C) if N[1] == ref_idx]
        if len(same) == 1 and "median_even_when_one_matches" not in self.wrong:
            self.hit("single_match")
            return same[0][2]
        self.hit("median_%d_matches" % len(same))
        return tuple(median(A[2][i], B[2][i], C[2][i]) for i in (0, 1))

    # ---- writing a (sub-)partition's motion into the field ----
    def put(self, x, y, w, h, l, ref_idx, mv):
        F = self.F
        for by in range(y // 4, (y + h) // 4):
            for bx in range(x // 4, (x + w) // 4):
                i = F.at(self.x4 + bx, self.y4 + by)
                F.ref[l][i], F.mv[l][i] = ref_idx, mv
                F.pic[l][i] = F.lists[l][ref_idx] if ref_idx >= 0 else None

    def mark(self, x, y, w, h, intra=False):
        for by in range(y // 4, (y + h) // 4):
            for bx in range(x // 4, (x + w) // 4):
                i = self.F.at(self.x4 + bx, self.y4 + by)
                self.F.done[i], self.F.intra[i] = True, intra

    # ---- 8.4.1.1 ----
    def p_skip(self):
        a_av, b_av = self.available(self.x4 - 1, self.y4), self.available(self.x4, self.y4 - 1)
        A, B = self.data(0, self.x4 - 1, self.y4, a_av), self.data(0, self.x4, self.y4 - 1, b_av)
        una = (not a_av and not b_av) if "p_skip_unavailable_and" in self.wrong else (not a_av or not b_av)
        zero_nb = (A == (0, (0, 0)) or B == (0, (0, 0))) and "p_skip_without_zero_neighbour_rule" not in self.wrong
        if not a_av or not b_av:
            self.hit("p_skip_A_or_B_unavailable" if a_av or b_av else "p_skip_A_and_B_unavailable")
        elif A == (0, (0, 0)) or B == (0, (0, 0)):
            self.hit("p_skip_zero_neighbour_" + ("A" if A == (0, (0, 0)) else "B"))
        if una or zero_nb:
            mv = (0, 0)
        else:
            mv = self.predict(0, self.x4, self.y4, 4, 0)
            self.hit("p_skip_predicted" + ("_nonzero" if mv != (0, 0) else ""))
        self.put(0, 0, 16, 16, 0, 0, mv)

    # ---- 8.4.1.2 ----
    def colocated(self, q, j):
        """8.4.1.2.1 for frames: (refIdxCol, mvCol, the picture referred to) of quadrant q, 4x4 block j (6.4.3 order inside the quadrant)"""
        inf = self.seq.get("direct_8x8_inference", 1)
        if inf and "col_block_itself_under_inference" not in self.wrong:
            bx, by = (q & 1) * 3, (q >> 1) * 3                      # the corner block of the macroblock on the quadrant's side
            self.hit("col_corner_block")
        else:
            bx, by = (q & 1) * 2 + (j & 1), (q >> 1) * 2 + (j >> 1)
            self.hit("col_block_itself")
        C = self.fields[self.F.lists[1][0]]
        i = C.at(self.x4 + bx, self.y4 + by)
        if C.intra[i]:
            self.hit("col_intra")
            return -1, (0, 0), None
        if C.ref[0][i] >= 0:
            self.hit("col_list0")
            return C.ref[0][i], C.mv[0][i], C.pic[0][i]
        if "col_list1_never_consulted" in self.wrong:
            return -1, (0, 0), None
        assert C.ref[1][i] >= 0
        self.hit("col_list1")
        return C.ref[1][i], C.mv[1][i], C.pic[1][i]

    def spatial_mb(self, q):
        """refIdxL0 / L1 and the predictors of 8.4.1.2.2: from the macroblock's neighbours, whichever quadrant asks"""
        bx, by, w4 = self.x4, self.y4, 4
        if "direct_pred_part_width_of_sub_partition" in self.wrong:
            w4 = 1
        if "spatial_direct_own_partitions" in self.wrong and q is not None:
            bx, by, w4 = self.x4 + (q & 1) * 2, self.y4 + (q >> 1) * 2, 2
        refs, mvp = [], []
        for l in (0, 1):
            A, B, C = self.neighbours(l, bx, by, w4)
            if "spatial_min_instead_of_min_positive" in self.wrong:
                refs.append(min(A[1], B[1], C[1]))
            else:
                refs.append(min_positive(A[1], min_positive(B[1], C[1])))
        zero_pred = refs[0] < 0 and refs[1] < 0
        if zero_pred:
            self.hit("spatial_both_negative")
            return [0, 0], [(0, 0), (0, 0)], True
        self.hit("spatial_both_found" if min(refs) >= 0 else "spatial_only_list%d" % (0 if refs[0] >= 0 else 1))
        for l in (0, 1):
            mvp.append(self.predict(l, bx, by, w4, refs[l]) if refs[l] >= 0 else (0, 0))
        return refs, mvp, False

    def direct(self, quads, in_b8x8):
        """direct prediction of the quadrants in `quads` of the current macroblock"""
        spatial = self.p.get("direct_spatial", 1)
        inf = self.seq.get("direct_8x8_inference", 1)
        assert self.F.lists[1], "direct prediction without RefPicList1[0]"
        self.hit(("spatial" if spatial else "temporal") + ("_inference" if inf else "_no_inference"))
        for q in quads:
            if spatial:
                refs, mvp, zero_pred = self.spatial_mb(q if in_b8x8 else None)
            flags = []
            for j in range(4):
                x, y = (q & 1) * 8 + (j & 1) * 4, (q >> 1) * 8 + (j >> 1) * 4
                ref_col, mv_col, pic_col = self.colocated(q, j)
                if spatial:
                    lim = 0 if "col_zero_only_zero_vector" in self.wrong else 1
                    ref_ok = ref_col >= 0 if "col_zero_any_ref_idx_col" in self.wrong else ref_col == 0
                    col_zero = ref_ok and abs(mv_col[0]) <= lim and abs(mv_col[1]) <= lim       # (RefPicList1[0] is a short-term picture: no other kind here)
                    flags.append(col_zero)
                    if ref_col == 0:
                        self.hit("col_zero_mv_%s" % ("within_1" if max(abs(mv_col[0]), abs(mv_col[1])) <= 1 else "beyond_1"))
                        for c in mv_col:
                            if abs(c) in (1, 2):
                                self.hit("col_component_%+d" % c)
                    elif ref_col > 0 and max(abs(mv_col[0]), abs(mv_col[1])) <= 1:
                        self.hit("col_zero_blocked_by_ref_idx_col")
                    for l in (0, 1):
                        if refs[l] < 0:
                            self.put(x, y, 4, 4, l, -1, (0, 0))
                            continue
                        z = zero_pred or (col_zero and (refs[l] == 0 or "col_zero_ignores_ref_idx" in self.wrong))
                        if not zero_pred and col_zero:
                            self.hit("col_zero_applies" if refs[l] == 0 else "col_zero_true_but_ref_idx_not_0")
                        self.put(x, y, 4, 4, l, refs[l], (0, 0) if z else mvp[l])
                else:
                    l0 = self.F.lists[0]
                    if ref_col < 0:
                        self.hit("temporal_col_intra")
                        r0, mv0, mv1 = 0, (0, 0), (0, 0)
                    else:
                        assert pic_col in l0, ("temporal direct: the picture the colocated block referred to is not in RefPicList0", self.k, pic_col, l0)
                        r0 = l0.index(pic_col)
                        self.hit("temporal_ref_idx_mapped_" + ("same" if r0 == ref_col else "differs"))
                        if "temporal_ref_idx_unmapped" in self.wrong:
                            r0 = min(ref_col, len(l0) - 1)
                        pocs = self.pics[self.k]["poc"], self.pics[l0[r0]]["poc"], self.pics[self.F.lists[1][0]]["poc"]
                        if pocs[1] == pocs[2]:
                            assert self.wrong, "td = 0: not with the different frames of these streams"
                            dsf = 256                                   # (a wrong refIdxL0 may name RefPicList1[0] itself: 8-191 / 8-192, mvL0 = mvCol)
                        else:
                            dsf = dist_scale_factor(*pocs, self.wrong)
                        self.hit("dsf_" + ("negative" if dsf < 0 else ("dyadic" if dsf & (dsf - 1) == 0 else "non_dyadic")))
                        mv0 = scale_mv(dsf, mv_col, self.wrong)
                        if any((dsf * c + 128) >> 8 != (dsf * c) >> 8 for c in mv_col):
                            self.hit("temporal_rounding_matters")
                        mv1 = tuple(a - b for a, b in zip(mv0, mv_col))
                        if "mv_l1_sign_swapped" in self.wrong:
                            mv1 = tuple(-c for c in mv1)
                    self.put(x, y, 4, 4, 0, r0, mv0)
                    self.put(x, y, 4, 4, 1, 0, mv1)
            if spatial and len(set(flags)) > 1:
                self.hit("col_zero_differs_inside_a_quadrant")
            self.mark((q & 1) * 8, (q >> 1) * 8, 8, 8)

    # ---- one macroblock ----
    def macroblock(self, a):
        m, kind, F = self.p["mbs"][a], self.p["kind"], self.F
        self.cur, self.x4, self.y4 = a, (a % self.mbw) * 4, (a // self.mbw) * 4
        F.slice_of[a] = a - a % self.step
        t = m["t"]
        if t in INTRA:
            self.mark(0, 0, 16, 16, intra=True)
            return
        if t == "skip":
            self.hit(("mb_type", "P_Skip" if kind == "P" else "B_Skip"))
            if kind == "P":
                self.p_skip()
                self.mark(0, 0, 16, 16)
            else:
                self.direct(range(4), False)
            return
        if t != "mv":
            # the forms that state their motion: taken as it stands (and the predictor 8.4.1.3 gives is handed out for the comparison of typings)
            parts = {"16x16": [(0, 0, 16, 16)], "16x8": [(0, 0, 16, 8), (0, 8, 16, 8)], "8x16": [(0, 0, 8, 16), (8, 0, 8, 16)]}[t]
            for i, (x, y, w, h) in enumerate(parts):
                for l in (0, 1):
                    q = (m.get("l%d" % l) if t == "16x16" else (m["parts"][i] if l == 0 else None))
                    if q is None:
                        continue
                    r = F.lists[l].index(q[0])
                    if self.mvp_out is not None:
                        self.mvp_out[(self.k, a, l, i)] = self.predict(l, self.x4 + x // 4, self.y4 + y // 4, w // 4, r, t if t != "16x16" else None, i)
                    self.put(x, y, w, h, l, r, tuple(q[1]))
                self.mark(x, y, w, h)
            return
        _, name, modes, counts, subs, rects = sw.mv_shape(kind, m)
        self.hit(("mb_type", name))
        if name == "B_Direct_16x16":
            self.direct(range(4), False)
            return
        shape = {(16, 8): "16x8", (8, 16): "8x16"}.get(rects[0][0][2:]) if subs is None else None
        for i, mode in enumerate(modes):
            if subs is not None:
                self.hit(("sub_mb_type", m["sub"][i]))
                self.hit(("sub_mb_type_in_quadrant", m["sub"][i], i))
            if mode == "Direct":
                self.direct([i], True)
                continue
            use = [mode in ("L0", "Bi"), mode in ("L1", "Bi")]
            if subs is not None and kind == "B":
                self.hit("quadrant_uses_" + mode)
            if use == [False, True] and "quadrant_list1_only_as_list0" in self.wrong and subs is not None:
                swap = True
            else:
                swap = False
            for j, (x, y, w, h) in enumerate(rects[i]):
                for l in (0, 1):
                    if not use[l]:
                        self.put(x, y, w, h, l ^ swap, -1, (0, 0))
                        continue
                    r = m["ref"][l][i]
                    mvp = self.predict(l, self.x4 + x // 4, self.y4 + y // 4, w // 4, r, shape, i)
                    d = m["mvd"][l][i][j]
                    lo = l ^ swap
                    ro = min(r, len(F.lists[lo]) - 1)
                    self.put(x, y, w, h, lo, ro if swap else r, (mvp[0] + d[0], mvp[1] + d[1]))
                self.mark(x, y, w, h)


def derive(seq, pics, pl=None, wrong=frozenset(), cov=None, mvp_out=None):
    """[per picture: [per macroblock: None (intra) or 16 entries in raster order of the 4x4 blocks, each (l0, l1) with lX = None (list unused) or
    (picture index, (mvx, mvy))]] and the fields (``Field``) the pictures leave behind.  cov: a dict that counts the branches taken; mvp_out: a dict
    that receives the predictor of 8.4.1.3 for every partition of the forms that state their vectors, keyed (picture, macroblock, list, partition)."""
    pl = pl or sw.plan(seq, pics)
    wrong = frozenset(wrong)
    fields, out = {}, []
    for k, p in enumerate(pics):
        assert not p.get("field"), "frame pictures only"
        d = Deriver(seq, pics, pl, k, fields, wrong, cov, mvp_out)
        for a in range(len(p["mbs"])):
            d.macroblock(a)
        F = d.F
        fields[k] = F
        motion = []
        for a, m in enumerate(p["mbs"]):
            if m["t"] in INTRA:
                motion.append(None)
                continue
            x4, y4 = (a % d.mbw) * 4, (a // d.mbw) * 4
            blocks = []
            for by in range(4):
                for bx in range(4):
                    i = F.at(x4 + bx, y4 + by)
                    blocks.append(tuple((F.pic[l][i], F.mv[l][i]) if F.ref[l][i] >= 0 else None for l in (0, 1)))
            motion.append(blocks)
        out.append(motion)
    return out, fields


def rectangles(blocks):
    """(x, y, w, h, l0, l1) covering the macroblock, blocks of equal motion merged: the whole macroblock, an 8x8 quadrant or a 4x4 block"""
    if all(b == blocks[0] for b in blocks):
        return [(0, 0, 16, 16) + blocks[0]]
    out = []
    for q in range(4):
        qx, qy = (q & 1) * 2, (q >> 1) * 2
        four = [blocks[(qy + j) * 4 + qx + i] for j in (0, 1) for i in (0, 1)]
        if all(b == four[0] for b in four):
            out.append((qx * 4, qy * 4, 8, 8) + four[0])
        else:
            out += [((qx + i) * 4, (qy + j) * 4, 4, 4) + blocks[(qy + j) * 4 + qx + i] for j in (0, 1) for i in (0, 1)]
    return out
