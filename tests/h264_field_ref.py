"""H.264 field pictures (PAFF) of the scripted streams (tests/scripted_h264.py with seq["frame_mbs_only"] = 0 and field="top" | "bottom" on a picture),
restated from the clauses: plain integers and numpy, computed from the SCRIPT, never from a bitstream, and without opening the oracle or the product.
tests/analytic_expect.expect_h264 and tests/deblock_ref.py call this wherever a rule differs between a frame picture and a field:

    8.2.4.1, 8.2.4.2.2 / .4 / .5   the reference lists a decoder builds for a field (``decoder_lists``): the script names its references by picture, the
                                   writer turns the name into the index of ITS list, and the expectation reads the picture back out of THIS list --
                                   two typings of the clause; a decoder whose list differs predicts from another field
    8.4.2.2                        the reference of a field is every second line of the store, clamped at the FIELD's border (``FieldRef``); the reference
                                   of a frame picture is the woven store, whichever way it was coded
    8.4.1.4 / Table 8-9            the vertical chroma vector offset of a cross-parity reference (``chroma_mvy_offset``)
    8.4.2.3.1                      implicit weights from the order counts of the current FIELD and the two reference FIELDS (``field_poc``)
    8.5.6 / 8.5.7                  the inverse field scans (``decoder_scans``)
    8.7.2.1                        the two field rules of the boundary strength (``FIELD_MVY_LIMIT``, ``intra_edge_bs``)
    C.4                            output: a frame goes out when both its fields are decoded, in the order of the smaller of their two counts

A lone first field at the end of a stream goes out with its lines repeated.  That is THIS DECODER's convention (jobs.h, "lone_field"), not the
standard's: the standard outputs the field and says nothing of the missing lines.

Out of scope, here as in the writer: direct prediction and B_Skip in B fields, long-term fields, memory management control operations, MBAFF, CABAC.

``wrong``: wrong-on-purpose switches (SWITCHES); tests/test_h264_field_host.py asserts that each changes the expected picture of a named case.
"""
import numpy as np

from spec_tables_h264 import FIELD_SCAN_4x4, FIELD_SCAN_8x8, ZIGZAG_4x4, ZIGZAG_8x8

SWITCHES = ("clamp_at_frame_border", "no_chroma_parity_offset", "chroma_parity_offset_sign", "zigzag_in_field_4x4", "zigzag_in_field_8x8",
            "field_list_starts_other_parity", "field_list_no_alternation", "current_frames_first_field_not_listed", "implicit_weights_from_frame_poc",
            "bs4_on_horizontal_field_edge", "frame_mvy_limit_in_field", "fields_of_one_frame_same_reference", "deblock_across_parities", "weave_swapped",
            "intra_neighbour_from_other_parity")
OTHER = {"top": "bottom", "bottom": "top"}
# 8.7.2.1: "... the absolute difference between the vertical component of the motion vectors used is greater than or equal to 4 in units of quarter
# FRAME luma samples"; a field's vector counts quarter FIELD samples, and one field line is two frame lines: a difference of 2.  (tests/SPEC_AUDIT.md
# records that this sentence is typed from memory and what the other reading would be.)
FIELD_MVY_LIMIT = 2


def has_fields(pics):
    return any(p.get("field") for p in pics)


def structure(pics):
    """Per picture (frame number in decoding order counting frames, parity or None, is the second field of its frame)"""
    out, f = [], -1
    for k, p in enumerate(pics):
        par = p.get("field")
        second = bool(par) and k > 0 and out[-1][1] == OTHER[par] and not out[-1][2]
        f += 0 if second else 1
        out.append((f, par, second))
    return out


def field_of(pics, name, parity=None):
    """(picture index, parity) of a reference name of the script: an index names a field picture (its own parity), or -- from a frame picture -- the
    store that starts there; (index, parity) names one field of a picture coded as a frame"""
    if isinstance(name, tuple):
        assert not pics[name[0]].get("field"), "(index, parity) names a field of a picture coded as a frame"
        return name
    return name, pics[name].get("field") or parity


def field_poc(pics, name):
    """PicOrderCnt of the reference FIELD `name` (8.2.1): a field's own count; both fields of a picture coded as a frame have the frame's"""
    return pics[field_of(pics, name)[0]]["poc"]


# ---- 8.2.4.2: the lists a decoder builds ---------------------------------------------------------------------------------------------------------
def interleave(order, parity, wrong=frozenset()):
    """8.2.4.2.5 by walking two cursors over the ordered stores: the next field of the wanted parity is taken, the wanted parity flips; a store that
    lacks the wanted field is stepped over; when the wanted parity has no field left the remaining fields of the other parity follow."""
    start = OTHER[parity] if "field_list_starts_other_parity" in wrong else parity
    if "field_list_no_alternation" in wrong:
        return [e[q] for e in order for q in (start, OTHER[start]) if q in e]
    at = {"top": 0, "bottom": 0}

    def take(q):
        while at[q] < len(order) and q not in order[at[q]]:
            at[q] += 1
        if at[q] == len(order):
            return None
        at[q] += 1
        return order[at[q] - 1][q]
    out, want = [], start
    while True:
        v = take(want)
        if v is None:
            while True:
                v = take(OTHER[want])
                if v is None:
                    return out
                out.append(v)
        out.append(v)
        want = OTHER[want]


def decoder_lists(seq, pics, wrong=frozenset()):
    """[(RefPicList0, RefPicList1)] per picture, uncut, as a decoder derives them (short-term references, sliding window), in the script's names.
    The decoded picture buffer holds frame stores: dict(fn=frame_num, top=name, bottom=name, poc={parity: count}) with the fields that are held."""
    nrf = seq.get("num_ref_frames", 1)
    st = structure(pics)
    dpb, out, fn = [], [], 0
    for k, p in enumerate(pics):
        f, par, second = st[k]
        is_ref = p.get("is_ref", p["kind"] != "B")
        if k == 0:
            dpb, fn = [], 0
        this_fn = dpb_fn if second else fn
        held = [e for e in dpb if not ("current_frames_first_field_not_listed" in wrong and second and e["fn"] == this_fn and e is dpb[-1])]
        both = [e for e in held if "top" in e and "bottom" in e]
        epoc = lambda e: min(e["poc"].values())
        l0, l1 = [], []
        if p["kind"] == "P":
            # 8.2.4.1: FrameNumWrap = frame_num (no wrap here); a field's PicNum is 2 * FrameNumWrap + 1 (same parity) or 2 * FrameNumWrap: the order of
            # 8.2.4.2.2 is the stores' by descending FrameNumWrap, the first field of the current frame (equal frame_num: the largest) in front
            order = sorted(held if par else both, key=lambda e: -e["fn"])
            l0 = interleave(order, par, wrong) if par else [e["first"] for e in order]
        elif p["kind"] == "B":
            pool = held if par else both
            lo = sorted((e for e in pool if epoc(e) <= p["poc"]), key=lambda e: -epoc(e))
            hi = sorted((e for e in pool if epoc(e) > p["poc"]), key=epoc)
            if par:
                l0, l1 = interleave(lo + hi, par, wrong), interleave(hi + lo, par, wrong)
            else:
                l0, l1 = [e["first"] for e in lo + hi], [e["first"] for e in hi + lo]
            if len(l1) > 1 and l0 == l1:
                l1[0], l1[1] = l1[1], l1[0]
        out.append((l0, l1))
        if is_ref and second:
            dpb[-1][par] = k
            dpb[-1]["poc"][par] = p["poc"]
        elif is_ref:
            if len(dpb) >= nrf:
                dpb.sort(key=lambda e: e["fn"])
                dpb.pop(0)
            e = dict(fn=this_fn, first=k, poc={})
            for q in ((par,) if par else ("top", "bottom")):
                e[q] = k if par else (k, q)
                e["poc"][q] = p["poc"]
            dpb.append(e)
        if not second:
            dpb_fn = this_fn
            if is_ref:
                fn = this_fn + 1
    return out


# ---- 8.4.2.2: the reference samples --------------------------------------------------------------------------------------------------------------
class FieldRef:
    """One parity of a frame store as a reference picture: line y of the field is line 2 y + parity of the store; coordinates are clamped to
    0 .. field height - 1 (8.4.2.2.1 with PicHeightInSamples of the FIELD)."""
    def __init__(self, store, parity, wrong=frozenset()):
        self.store, self.par, self.wrong = store, int(parity == "bottom"), wrong
        self.shape = (store.shape[0] // 2, store.shape[1])

    def fetch(self, ys, xs):
        xs = np.clip(xs, 0, self.shape[1] - 1)
        if "clamp_at_frame_border" in self.wrong:
            rows = np.clip(2 * ys + self.par, 0, self.store.shape[0] - 1)
        else:
            rows = 2 * np.clip(ys, 0, self.shape[0] - 1) + self.par
        return self.store[np.ix_(rows, xs)].astype(np.int64)


def chroma_mvy_offset(cur_parity, ref_parity, wrong=frozenset()):
    """Table 8-9 (8.4.1.4), in the chroma vector's units (eighth chroma samples = quarter luma samples): a field that predicts from a field of the other
    parity -- reference bottom, current top: -2; reference top, current bottom: +2; same parity, and every frame picture: 0.  (Relative to the luma lines of their
    own field the chroma lines of the two parities sit a quarter of a chroma field line apart in opposite directions: the offset undoes that.)"""
    if cur_parity is None or cur_parity == ref_parity or "no_chroma_parity_offset" in wrong:
        return 0
    off = -2 if cur_parity == "top" else 2
    return -off if "chroma_parity_offset_sign" in wrong else off


# ---- 8.5.6 / 8.5.7: the scans --------------------------------------------------------------------------------------------------------------------
def decoder_scans(field, wrong=frozenset()):
    """(perm4, perm8) for h264_recon_ref.mb_residual, or None for a frame picture: the script states every matrix in raster order; the stream carries
    its levels in the order of the picture's scan (a field: the field scan); a decoder puts level k at ITS scan's position k.  perm[j] = the raster
    position of the script whose level a decoder finds at raster position j -- the identity unless the decoder's scan is the wrong one."""
    if not field:
        return None
    out = []
    for n, true, zz in ((4, FIELD_SCAN_4x4, ZIGZAG_4x4), (8, FIELD_SCAN_8x8, ZIGZAG_8x8)):
        used = zz if "zigzag_in_field_%dx%d" % (n, n) in wrong else true
        perm = [0] * (n * n)
        for k in range(n * n):
            perm[used[k]] = true[k]
        out.append(perm)
    return tuple(out)


# ---- 8.7.2.1 ---------------------------------------------------------------------------------------------------------------------------------
def intra_edge_bs(field, horizontal_edge, wrong=frozenset()):
    """bS of a MACROBLOCK edge with an intra macroblock on either side: 4 -- but in a field picture only a vertical edge has it, a horizontal one 3"""
    return 3 if field and horizontal_edge and "bs4_on_horizontal_field_edge" not in wrong else 4


def mvy_limit(field, wrong=frozenset()):
    return FIELD_MVY_LIMIT if field and "frame_mvy_limit_in_field" not in wrong else 4


def reference_key(pics, field, wrong=frozenset()):
    """what counts as "the same reference picture" in 8.7.2.1: the picture a vector points into -- a field picture's references are fields, and the
    two fields of one frame are two pictures"""
    if not field or "fields_of_one_frame_same_reference" not in wrong:
        return lambda name: name
    st = structure(pics)
    return lambda name: st[field_of(pics, name)[0]][0]


# ---- output ----------------------------------------------------------------------------------------------------------------------------------
def weave(top, bottom):
    out = np.empty((top.shape[0] * 2, top.shape[1]), top.dtype)
    out[0::2], out[1::2] = top, bottom
    return out


def output_frames(pics, planes, wrong=frozenset()):
    """[(decode index of the frame's first picture, (Y, Cb, Cr) of the whole frame)] in output order: planes[k] is picture k as decoded (a field: its
    own lines).  A frame goes out when both fields are there, ordered by the smaller count; a lone first field fills both parities (this decoder's
    convention, see the module text)."""
    st = structure(pics)
    frames = []
    for k, p in enumerate(pics):
        f, par, second = st[k]
        if second:
            continue
        if not par:
            frames.append((p["poc"], k, planes[k]))
            continue
        if k + 1 < len(pics) and st[k + 1][2]:
            t, b = (planes[k], planes[k + 1]) if par == "top" else (planes[k + 1], planes[k])
            if "weave_swapped" in wrong:
                t, b = b, t
            frames.append((min(p["poc"], pics[k + 1]["poc"]), k, tuple(weave(x, y) for x, y in zip(t, b))))
        else:
            frames.append((p["poc"], k, tuple(weave(x, x) for x in planes[k])))
    return [(k, pl) for _, k, pl in sorted(frames, key=lambda q: q[0])]


def counts(pics):
    """(field pictures, first fields that END the stream without their partner) the script implies.  The decoders' "lone fields" counters count a field
    that a FOLLOWING picture leaves alone (tests/test_gpu_parity.py::test_a_field_without_partner_on_device); the writer refuses such a stream, so
    these counters stay 0 here and the field that ends a stream shows in its frame alone."""
    st = structure(pics)
    lone = sum(1 for k, (f, par, second) in enumerate(st) if par and not second and not (k + 1 < len(st) and st[k + 1][2]))
    return sum(1 for q in st if q[1]), lone
