"""MPEG-2 option mpeg2_field_pictures without a GPU: field pictures, 16x8 motion compensation and dual prime.

The product's host path with the switch on (tests/native/mpeg2_field_check.cpp: splitter, slice parser, the reconstruction of mpeg2_recon.h that
k_mpeg2_recon runs, field pairing) must equal the numpy restatement (tests/mpeg2_field_ref.py) bit for bit on seeded random streams and on one
scripted stream per feature (tests/scripted_mpeg2_field.py).  Analytic cases check both against closed forms written here, and one discrimination
test per switch of the restatement shows that the analytic streams tell the rule from its plausible mistake.  Then pairing, lone fields, options
and refusals through parse-only handles, the device-VLC lane's routine walked on the CPU over dual-prime frame pictures
(tests/native/mpeg2_field_vlc_check.cpp), and the stand-alone sanitizer program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mpeg2_field_ref as F
import mpeg2_ref as R
import scripted_mpeg2 as S
import scripted_mpeg2_field as SF
from jmcodec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libmpeg2_field_check.so")
    csrc = os.path.join(ROOT, "jmcodec_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "mpeg2_field_check.cpp"), os.path.join(csrc, "mpeg2_syntax.cpp")]
    deps = srcs + [os.path.join(ROOT, "tests", "native", "mpeg2_field_host.h")] + [os.path.join(csrc, h) for h in ("mpeg2_syntax.h", "mpeg2_recon.h", "mpeg2_jobs.h", "jpeg_recon.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so] + srcs)
    l = C.CDLL(so)
    l.m2f_decode.restype = C.c_long
    l.m2f_decode.argtypes = [C.c_char_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    l.m2f_error.restype = C.c_char_p

    def decode(data, chunk=0):
        """-> (n, [(NV12 bytes, w, h)], (errors, dropped, clamped, lone fields, field pictures, dual-prime mbs, 16x8 mbs))"""
        out_buf, dims, st = C.create_string_buffer(1 << 22), (C.c_int * 128)(), (C.c_int * 7)()
        n = l.m2f_decode(data, len(data), chunk, out_buf, len(out_buf), dims, 64, st)
        frames, o = [], 0
        for i in range(max(n, 0)):
            w, h = dims[2 * i], dims[2 * i + 1]
            frames.append((out_buf.raw[o:o + w * h * 3 // 2], w, h))
            o += w * h * 3 // 2
        return n, frames, tuple(st)
    decode.lib = l
    return decode


@pytest.fixture(scope="module")
def vlc_walk():
    """mpeg2_vlc_slice, the routine of k_mpeg2_vlc, over the frame pictures of a stream next to the host decoder -> the 16 counters of m2fv_stream"""
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libmpeg2_field_vlc_check.so")
    csrc = os.path.join(ROOT, "jmcodec_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "mpeg2_field_vlc_check.cpp"), os.path.join(csrc, "mpeg2_syntax.cpp")]
    deps = srcs + [os.path.join(ROOT, "tests", "native", "mpeg2_vlc_walk.h")] + [os.path.join(csrc, h) for h in ("mpeg2_syntax.h", "mpeg2_vlc.h", "mpeg2_jobs.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so] + srcs)
    l = C.CDLL(so)
    l.m2fv_stream.restype = C.c_long
    l.m2fv_stream.argtypes = [C.c_char_p, C.c_long, C.c_int, C.c_void_p]

    def walk(data, field_pictures):
        info = (C.c_int * 16)()
        rc = l.m2fv_stream(data, len(data), field_pictures, info)
        return rc, dict(zip(("pictures", "differ", "dual_status", "dual_walk", "dual_host", "refused", "error_differs", "clamped_walk", "clamped_host", "broken",
                             "fields", "rejected", "kinds"), info))
    return walk


def stats_of(info):
    return (info["errors"], info["dropped"], info["clamped"], info["lone"], info["fields"], info["dual"], info["m16x8"])


# ---- 1. the host path against the restatement ---------------------------------------------------------------------------------------------------
def test_dmvector_table_equals_the_restatement(native):
    v, got = (C.c_int * 4)(), {}
    for i in range(native.lib.m2f_table(11, 0, v)):
        native.lib.m2f_table(11, i, v)
        got[v[2]] = format(v[0], "0%db" % v[1])
    assert got == F.B11 == {0: "0", 1: "10", -1: "11"}


_SIZES = ((48, 64), (16, 32), (80, 40), (272, 32))
_LAYOUTS = ("IP PP BB BB PP", "II PP BB PD BB", "I PP BB Pd B PP", "IP Pd PD PP BB")


def test_host_path_equals_restatement_on_seeded_random_streams_that_cover_every_case(native):
    """40 random streams of frame and field pictures: clean on both sides, equal frames, and between them every prediction mode x direction x field
    read x half-sample phase -- counted by the restatement where it fetches."""
    cases = set()
    for seed in range(40):
        w, h = _SIZES[seed % 4]
        data, info = SF.field_stream(seed, w, h, _LAYOUTS[(seed // 4) % 4]), {}
        want = F.decode_stream(data, 0, info)
        n, frames, st = native(data)
        assert frames == want and st == stats_of(info), seed
        assert (info["errors"], info["clamped"], info["dropped"]) == (0, 0, 0), seed
        cases |= info["cases"]
    phases = [(hx, hy) for hx in (0, 1) for hy in (0, 1)]
    need = {(m, s, f) + ph for m in ("field", "16x8") for s in (0, 1) for f in (0, 1) for ph in phases}
    need |= {(m, 0, f) + ph for m in ("dual_field", "dual_frame") for f in (0, 1) for ph in phases}
    assert need <= cases, sorted(need - cases)


_CASES = dict(SF.feature_cases())
_CASES.update(mixed_chain=SF.mixed_chain(), truncated=SF.truncated_field_stream())
_CASES.update({"clamped_" + k: v for k, v in SF.clamped_cases().items()})
_CASES.update({"lone_" + k: v[0] for k, v in SF.lone_cases().items()})
_CASES.update({f"size_{w}x{h}": SF.field_stream(w + h, w, h, "IP PP BB") for w, h in _SIZES})


@pytest.mark.parametrize("name", sorted(_CASES))
def test_host_path_equals_restatement_on_scripted_cases_in_every_chunking(native, name):
    data, info = _CASES[name], {}
    want = F.decode_stream(data, 0, info)
    for chunk in (0, -1, 1, 5):
        n, frames, st = native(data, chunk)
        assert n == len(want) and frames == want, chunk
        assert st == stats_of(info)
    damaged = name.startswith(("clamped_", "lone_")) or name == "truncated"
    assert (info["errors"] > 0) == damaged
    assert info["fields"] > 0 or "dual_prime_frame" in name


@pytest.mark.parametrize("name", sorted(SF.clamped_cases()))
def test_vectors_are_clamped_at_the_border_of_the_reference_field(native, name):
    """5. every mode: the host clamps, counts the macroblocks and an error; restatement and host path agree on how many"""
    info = {}
    F.decode_stream(SF.clamped_cases()[name], 0, info)
    _, _, st = native(SF.clamped_cases()[name])
    assert st[2] == info["clamped"] > 0 and st[0] == info["errors"] > 0
    assert {"field": st[4] > 0, "16x8": st[6] > 0, "dual_field": st[5] > 0 and st[4] > 0, "dual_frame": st[5] > 0}[name]


def test_frame_picture_streams_are_unchanged_by_the_switch(native):
    for seed in range(1000, 1030):
        data = S.random_stream(seed)
        assert native(data)[1] == R.decode_stream(data, 0) == F.decode_stream(data, 0), seed


# ---- 2. analytic cases: the expected pictures are closed forms, computed by neither decoder -------------------------------------------------------
def field_planes(par):
    """the analytic anchor's field of a parity: luma 32 x 48, Cb and Cr 16 x 24 (scripted_mpeg2_field.analytic_anchor)"""
    y, c = (SF.TOP, SF.CTOP) if par == 0 else (SF.BOT, SF.CBOT)
    Y = np.repeat(np.array(y), 8)[:, None] + 2 * (np.arange(48) // 8)[None, :]
    Cb = np.repeat(np.array(c), 8)[:, None] + 3 * (np.arange(24) // 8)[None, :]
    return [Y, Cb, Cb + 9]


def fetch(p, x0, y0, w, h, vx, vy):
    """7.6.4 on an array: w x h samples at (x0, y0) displaced by a vector in half samples, coordinates clamped to the array"""
    H, W = p.shape
    ys, xs = np.arange(y0, y0 + h) + (vy >> 1), np.arange(x0, x0 + w) + (vx >> 1)
    at = lambda dy, dx: p[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)]      # noqa: E731
    fx, fy = vx & 1, vy & 1
    if fx and fy:
        return (at(0, 0) + at(0, 1) + at(1, 0) + at(1, 1) + 2) >> 2
    if fx or fy:
        return (at(0, 0) + at(fy, fx) + 1) >> 1
    return at(0, 0)


def toward_zero(v):
    return -((-v) // 2) if v < 0 else v // 2


def fetch_mb(fld, c, mx, y0, lines, v):
    """component c of a macroblock column mx: `lines` luma lines from field line y0 on (chroma: half of both), vector v of the luma"""
    if c == 0:
        return fetch(fld[0], mx * 16, y0, 16, lines, v[0], v[1])
    return fetch(fld[c], mx * 8, y0 // 2, 8, lines // 2, toward_zero(v[0]), toward_zero(v[1]))


def planes(frame, w, h):
    a = np.frombuffer(frame, np.uint8)
    uv = a[w * h:].reshape(h // 2, w // 2, 2)
    return [a[:w * h].reshape(h, w).astype(int), uv[:, :, 0].astype(int), uv[:, :, 1].astype(int)]


def both(native, items):
    data = SF.build(items)
    n, frames, st = native(data)
    info = {}
    assert frames == F.decode_stream(data, 0, info) and st[:4] == (0, 0, 0, 0) == stats_of(info)[:4], (st, stats_of(info))
    return [planes(f, w, h) for f, w, h in frames], data


def put(dst, c, mx, y0, block):
    n = 16 if c == 0 else 8
    yy = y0 if c == 0 else y0 // 2
    dst[c][yy:yy + block.shape[0], mx * n:mx * n + n] = block


def empty_field():
    return [np.zeros((32, 48), int), np.zeros((16, 24), int), np.zeros((16, 24), int)]


VX2 = (5, 1, -3)
VX = (3, -5, -2)                  # per macroblock column: inside the field, an odd positive and an odd negative one among them


def test_the_anchor_is_two_fields_interleaved(native):
    for first in (1, 2):
        (fr,), _ = both(native, SF.analytic_anchor(first))
        for c in range(3):
            assert np.array_equal(fr[c][0::2], field_planes(0)[c]) and np.array_equal(fr[c][1::2], field_planes(1)[c])


def field_prediction_items(sel):
    vy = (5, -3)
    p1 = SF.fpic("P", 1, 2, lambda r: [dict(x=x, fwd=[(sel, VX[x], vy[r])]) for x in range(3)])
    p2 = SF.fpic("P", 2, 2, lambda r: [dict(x=x, fwd=[(0, 0, 0)]) for x in range(3)])      # the bottom field copies the top field of its own frame
    return SF.analytic_anchor() + [("pic", p1), ("pic", p2)], vy


@pytest.mark.parametrize("sel", [0, 1])
def test_field_prediction_reads_the_selected_field_in_its_own_lines(native, sel):
    items, vy = field_prediction_items(sel)
    (_, fr), _ = both(native, items)
    want = empty_field()
    for r in range(2):
        for x in range(3):
            for c in range(3):
                put(want, c, x, r * 16, fetch_mb(field_planes(sel), c, x, r * 16, 16, (VX[x], vy[r])))
    for c in range(3):
        assert np.array_equal(fr[c][0::2], want[c]), c
        assert np.array_equal(fr[c][1::2], want[c]), c          # (the second P field read the first field of its own frame)


def m16x8_items():
    up, lo = (3, -7), (-5, -9)
    p1 = SF.fpic("P", 1, 2, lambda r: [dict(x=x, mode="16x8", fwd=[(0, VX[x], up[r]), (1, VX2[x], lo[r])]) for x in range(3)])
    p2 = SF.fpic("P", 2, 2, lambda r: [dict(x=x, fwd=[(1, 0, 0)]) for x in range(3)])
    return SF.analytic_anchor() + [("pic", p1), ("pic", p2)], up, lo


def test_16x8_splits_the_macroblock_at_line_8(native):
    items, up, lo = m16x8_items()
    (_, fr), _ = both(native, items)
    want = empty_field()
    for r in range(2):
        for x in range(3):
            for c in range(3):
                put(want, c, x, r * 16, fetch_mb(field_planes(0), c, x, r * 16, 8, (VX[x], up[r])))
                put(want, c, x, r * 16 + 8, fetch_mb(field_planes(1), c, x, r * 16 + 8, 8, (VX2[x], lo[r])))
    for c in range(3):
        assert np.array_equal(fr[c][0::2], want[c]), c
        assert np.array_equal(fr[c][1::2], field_planes(1)[c]), c


def opposite(v, dmv, m, e):
    """7.6.3.6, written out: ((v m + (v > 0)) >> 1) + dmv, the vertical one + e"""
    return (((v[0] * m + (1 if v[0] > 0 else 0)) >> 1) + dmv[0], ((v[1] * m + (1 if v[1] > 0 else 0)) >> 1) + e + dmv[1])


def dual_field_items(d):
    vy = (5, -7)
    pic = lambda s: SF.fpic("P", s, 2, lambda r: [dict(x=x, mode="dual", fwd=[(VX[x], vy[r])], dmv=(d, d)) for x in range(3)])      # noqa: E731
    return SF.analytic_anchor() + [("pic", pic(1)), ("pic", pic(2))], vy


@pytest.mark.parametrize("d", [-1, 1])
def test_dual_prime_in_field_pictures(native, d):
    """top field: same parity = the anchor's top field with v, opposite = its bottom field with the derived vector, e = -1.  Bottom field (the
    second): same parity = the anchor's bottom field, opposite = the top field just decoded, e = +1."""
    items, vy = dual_field_items(d)
    (_, fr), _ = both(native, items)
    top, bot, odd = empty_field(), empty_field(), 0
    for r in range(2):
        for x in range(3):
            v = (VX[x], vy[r])
            for c in range(3):
                a, b = fetch_mb(field_planes(0), c, x, r * 16, 16, v), fetch_mb(field_planes(1), c, x, r * 16, 16, opposite(v, (d, d), 1, -1))
                put(top, c, x, r * 16, (a + b + 1) >> 1)
                odd += int(((a + b) & 1).sum())
    for r in range(2):
        for x in range(3):
            v = (VX[x], vy[r])
            for c in range(3):
                a, b = fetch_mb(field_planes(1), c, x, r * 16, 16, v), fetch_mb(top, c, x, r * 16, 16, opposite(v, (d, d), 1, 1))
                put(bot, c, x, r * 16, (a + b + 1) >> 1)
    assert odd > 100                                            # the average's rounding is exercised
    for c in range(3):
        assert np.array_equal(fr[c][0::2], top[c]), c
        assert np.array_equal(fr[c][1::2], bot[c]), c


def dual_frame_items(tff, d):
    vy = (3, 5, -5, -3)
    pic = dict(type="P", frame_pred_frame_dct=0, progressive_frame=0, top_field_first=tff, f_code=((4, 4), (15, 15)),
               slices=[dict(row=r, qcode=4, mbs=[dict(x=x, mode="dual", fwd=[(VX[x], vy[r])], dmv=(d, -d)) for x in range(3)]) for r in range(4)])
    return SF.analytic_anchor() + [("pic", pic)], vy


@pytest.mark.parametrize("tff,d", [(0, 1), (1, 1), (1, -1)])
def test_dual_prime_in_frame_pictures(native, tff, d):
    """the top lines: the top field with v averaged with the bottom field with m = tff ? 1 : 3, e = -1; the bottom lines: the bottom field with v
    averaged with the top field with m = tff ? 3 : 1, e = +1.  A frame macroblock row is 8 lines of each field."""
    items, vy = dual_frame_items(tff, d)
    (_, fr), _ = both(native, items)
    top, bot = empty_field(), empty_field()
    for r in range(4):
        for x in range(3):
            v = (VX[x], vy[r])
            for c in range(3):
                a, b = fetch_mb(field_planes(0), c, x, r * 8, 8, v), fetch_mb(field_planes(1), c, x, r * 8, 8, opposite(v, (d, -d), 1 if tff else 3, -1))
                put(top, c, x, r * 8, (a + b + 1) >> 1)
                a, b = fetch_mb(field_planes(1), c, x, r * 8, 8, v), fetch_mb(field_planes(0), c, x, r * 8, 8, opposite(v, (d, -d), 3 if tff else 1, 1))
                put(bot, c, x, r * 8, (a + b + 1) >> 1)
    for c in range(3):
        assert np.array_equal(fr[c][0::2], top[c]), c
        assert np.array_equal(fr[c][1::2], bot[c]), c


def pmv_items():
    """4. one slice per row that goes through the modes: the vectors are coded as differences from predictors the writer tracks by 7.6.3.4"""
    row0 = [dict(x=0, fwd=[(0, 6, 9)]), dict(x=1, mode="16x8", fwd=[(1, -3, 5), (0, 4, 7)]), dict(x=2, mode="dual", fwd=[(-7, 3)], dmv=(1, -1))]
    row1 = [dict(x=0, mode="dual", fwd=[(5, -9)], dmv=(0, 1)), dict(x=1, fwd=[(1, 3, -4)]), dict(x=2, mode="16x8", fwd=[(0, -9, -11), (1, -1, -6)])]
    p1 = SF.fpic("P", 1, 2, lambda r: (row0, row1)[r])
    p2 = SF.fpic("P", 2, 2, lambda r: [dict(x=x, fwd=[(1, 0, 0)]) for x in range(3)])
    return SF.analytic_anchor() + [("pic", p1), ("pic", p2)], (row0, row1)


def test_predictors_across_modes_in_one_slice(native):
    items, rows = pmv_items()
    (_, fr), _ = both(native, items)
    want = empty_field()
    for r, mbs in enumerate(rows):
        for mb in mbs:
            x = mb["x"]
            for c in range(3):
                if mb.get("mode") == "16x8":
                    for k, (sel, vx, vy) in enumerate(mb["fwd"]):
                        put(want, c, x, r * 16 + 8 * k, fetch_mb(field_planes(sel), c, x, r * 16 + 8 * k, 8, (vx, vy)))
                elif mb.get("mode") == "dual":
                    v = mb["fwd"][0]
                    a, b = fetch_mb(field_planes(0), c, x, r * 16, 16, v), fetch_mb(field_planes(1), c, x, r * 16, 16, opposite(v, mb["dmv"], 1, -1))
                    put(want, c, x, r * 16, (a + b + 1) >> 1)
                else:
                    sel, vx, vy = mb["fwd"][0]
                    put(want, c, x, r * 16, fetch_mb(field_planes(sel), c, x, r * 16, 16, (vx, vy)))
    for c in range(3):
        assert np.array_equal(fr[c][0::2], want[c]), c


@pytest.mark.parametrize("switch,value,items", [
    ("select", 1, lambda: field_prediction_items(0)[0]), ("parity", 1, lambda: field_prediction_items(1)[0]),
    ("split", 4, lambda: m16x8_items()[0]), ("e_sign", 1, lambda: dual_field_items(1)[0]), ("v_round", 1, lambda: dual_field_items(-1)[0]),
    ("avg_round", 1, lambda: dual_field_items(1)[0]), ("m_swap", 1, lambda: dual_frame_items(1, 1)[0]), ("pmv_halve", 1, lambda: pmv_items()[0])])
def test_the_analytic_streams_tell_each_rule_from_its_mistake(native, switch, value, items):
    """one switch of the restatement flipped: the picture the closed forms above pin changes, and the product sides with the rule"""
    data = SF.build(items())
    right = F.decode_stream(data, 0)
    assert F.decode_stream(data, 0, **{switch: value}) != right
    assert native(data)[1] == right


# ---- 3., 6., 7. through the library, parse only ------------------------------------------------------------------------------------------------
STATS = ("errors", "dropped_pictures", "frames", "i_pictures", "p_pictures", "b_pictures", "interlaced_sequence", "failed", "mpeg2_field_pictures",
         "mpeg2_lone_fields", "mpeg2_dual_prime_mbs", "mpeg2_16x8_mbs", "mpeg2_clamped_mbs", "lone_fields")


def parse(data, chunks=None, **opt):
    with api.JmAmdDec(4, 1, options=dict(parse_only=1, mpeg2_field_pictures=1, **opt)) as d:
        n = d.decode_stream(data, keep=False, chunks=chunks if chunks is not None else [data])
        st = {k: d.stat(k) for k in STATS}
        st["order"] = [d.stat(f"display_poc:{i}") for i in range(n)]
        return n, st


def test_frames_pictures_and_display_order_of_a_mixed_chain():
    data, info = SF.mixed_chain(), {}
    want = F.decode_stream(data, 0, info)
    for chunks in (None, api.split_nalus(data)):
        n, st = parse(data, chunks)
        # coding order, frames 0..7: IP | PD | B | BB | PP | BB | B | P; an anchor is displayed when the next one arrives
        assert n == len(want) == 8 and st["order"] == [0, 2, 3, 1, 5, 6, 4, 7]
        assert st["dropped_pictures"] == 0 == info["dropped"] and st["errors"] == 0
        assert (st["i_pictures"], st["p_pictures"], st["b_pictures"]) == (1, 5, 6)          # coded pictures, 12 in all
        assert st["mpeg2_field_pictures"] == info["fields"] == 8 and st["mpeg2_lone_fields"] == 0
        assert st["mpeg2_dual_prime_mbs"] == info["dual"] > 0 and st["mpeg2_16x8_mbs"] == info["m16x8"] > 0


@pytest.mark.parametrize("name", sorted(SF.lone_cases()))
def test_lone_fields_are_displayed_and_counted(name):
    data, frames, lone = SF.lone_cases()[name]
    info = {}
    assert len(F.decode_stream(data, 0, info)) == frames and info["lone"] == lone
    n, st = parse(data)
    assert n == frames and st["mpeg2_lone_fields"] == lone and st["errors"] == info["errors"] == lone and st["failed"] == 0
    assert st["order"] == {"first_field_then_flush": [0], "then_a_frame_picture": [0, 2, 1], "then_a_same_parity_field": [0, 1],
                           "b_field_alone": [0, 2, 3, 1], "types_that_do_not_pair": [0, 1, 2]}[name]


def test_truncated_slice_in_a_field_picture():
    data, info = SF.truncated_field_stream(), {}
    F.decode_stream(data, 0, info)
    n, st = parse(data)
    assert n == 2 and st["errors"] == info["errors"] == 2 and st["failed"] == 0 and st["mpeg2_field_pictures"] == 4


def test_a_field_picture_in_a_progressive_sequence_is_skipped_as_damage(native):
    rng = np.random.default_rng(5)
    data = SF.build([("seq", dict(width=48, height=64, progressive_sequence=1)), ("pic", S.random_picture(rng, "I", 48, 64)),
                     ("pic", SF.random_field_picture(rng, "P", 48, 64, 1)), ("pic", S.random_picture(rng, "P", 48, 64))])
    n, st = parse(data)
    assert n == 2 and st["errors"] == 1 and st["failed"] == 0 and st["mpeg2_field_pictures"] == 0 and st["mpeg2_lone_fields"] == 0
    info = {}
    assert native(data)[1] == F.decode_stream(data, 0, info) and info["errors"] == 1


def test_option_values():
    l = api.lib()
    h = api.jm_nvdec_create_handle()
    try:
        assert l.jm_amddec_set_option(h, b"mpeg2_field_pictures", 2) == -1 and l.jm_amddec_set_option(h, b"mpeg2_field_pictures", -1) == -1
        assert l.jm_amddec_set_option(h, b"mpeg2_field_pictures", 1) == 0 and l.jm_amddec_set_option(h, b"mpeg2_field_pictures", 0) == 0
    finally:
        api.jm_nvdec_deinit(h)
    with api.JmAmdDec(4, 1, options=dict(parse_only=1, mpeg2_field_pictures=1)) as d:
        assert l.jm_amddec_set_option(d.h, b"mpeg2_field_pictures", 0) == -1            # after init
    for codec in (0, 1, 2):
        with pytest.raises(RuntimeError, match="mpeg2_field_pictures"):
            api.JmAmdDec(codec, 1, options=dict(parse_only=1, mpeg2_field_pictures=1))


@pytest.mark.parametrize("name,word", [("i_p_frame", "field pictures"), ("dual_prime_frame_tff1", "dual-prime")])
def test_option_0_keeps_refusing_with_the_same_words(name, word):
    data = SF.feature_cases()[name]
    with api.JmAmdDec(4, 1, options=dict(parse_only=1, mpeg2_field_pictures=0)) as d:
        with pytest.raises(RuntimeError):
            d.decode_stream(data, keep=False, chunks=[data])
        msg = api.lib().jm_amddec_last_error(d.h).decode()
        assert d.stat("failed") == 1
    assert "not supported" in msg and word in msg, msg
    n, st = parse(data)
    assert st["failed"] == 0 and n > 0


def test_dual_prime_in_a_b_picture_is_damage():
    rng = np.random.default_rng(6)
    b = SF.fpic("B", 1, 2, lambda r: [dict(x=x, mode="dual", fwd=[(0, 0)], dmv=(0, 0)) for x in range(3)])
    data = SF.build([("seq", dict(width=48, height=64, progressive_sequence=0))] + [("pic", S.random_picture(rng, t, 48, 64, 0)) for t in "IP"] +
                    [("pic", b), ("pic", SF.random_field_picture(rng, "B", 48, 64, 2))])
    n, st = parse(data)
    assert n == 3 and st["errors"] == 1 and st["failed"] == 0 and st["mpeg2_dual_prime_mbs"] == 0
    info = {}
    F.decode_stream(data, 0, info)
    assert info["errors"] == 1 and info["dual"] == 0


# ---- 8. the device-VLC lane's routine on the CPU ----------------------------------------------------------------------------------------------------
_DUAL_FRAME_STREAMS = {"tff0": lambda: SF.feature_cases()["dual_prime_frame_tff0"], "tff1": lambda: SF.feature_cases()["dual_prime_frame_tff1"],
                       "analytic": lambda: SF.build(dual_frame_items(1, -1)[0]), "clamped": lambda: SF.clamped_cases()["dual_frame"],
                       "chain": SF.mixed_chain, "random_272x32": lambda: SF.field_stream(77, 272, 32, "I Pd PD B Pd")}


@pytest.mark.parametrize("name", sorted(_DUAL_FRAME_STREAMS))
def test_the_lane_writes_the_hosts_records_for_dual_prime_frame_pictures(vlc_walk, name):
    """switch on: every frame picture's records equal the host's field by field apart from `first`, block by block the same entries, the same clamp;
    switch off: the lane reports the dual-prime status and the host refuses, as before the option"""
    data = _DUAL_FRAME_STREAMS[name]()
    rc, on = vlc_walk(data, 1)
    assert rc == 0 and on["pictures"] >= 1 and on["rejected"] == 0 and on["broken"] == 0
    assert on["differ"] == 0 and on["error_differs"] == 0 and on["dual_status"] == 0 and on["refused"] == 0
    assert on["dual_walk"] == on["dual_host"] > 0 and on["clamped_walk"] == on["clamped_host"]
    assert (on["clamped_walk"] > 0) == (name == "clamped")
    if name in ("tff0", "tff1"):                                 # (streams without field pictures: the splitter accepts them with the switch off)
        rc, off = vlc_walk(data, 0)
        assert rc == 0 and off["dual_status"] == off["refused"] == 2 and off["dual_walk"] == 0 and off["differ"] == 0


def test_the_lane_calls_dual_prime_in_a_b_frame_picture_damage_as_the_host_does(vlc_walk):
    rng = np.random.default_rng(8)
    b = dict(type="B", frame_pred_frame_dct=0, progressive_frame=0, f_code=((4, 4), (4, 4)),
             slices=[dict(row=r, qcode=4, mbs=[dict(x=x, mode="dual", fwd=[(0, 0)], dmv=(0, 0)) for x in range(3)]) for r in range(4)])
    data = SF.build([("seq", dict(width=48, height=64, progressive_sequence=0))] + [("pic", S.random_picture(rng, t, 48, 64, 0)) for t in "IP"] + [("pic", b)])
    rc, on = vlc_walk(data, 1)
    assert rc == 0 and on["pictures"] == 3 and on["differ"] == 0 and on["error_differs"] == 0 and on["dual_walk"] == 0 and on["dual_status"] == 0
    assert on["kinds"] == 1 << 21                                # kM2DmgDualPrimeInB, the kind behind kM2DmgDualPrime


# ---- 9. the sanitizer harness ---------------------------------------------------------------------------------------------------------------------
def test_mpeg2_field_asan_builds_and_runs_clean(tmp_path):
    """tools/mpeg2_field_asan.cpp: a stand-alone host program (its own main) under AddressSanitizer / UBSan: the scripted streams as they are and
    2 500 seeded mutations of them"""
    out = tmp_path / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "mpeg2_field_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    cases = SF.feature_cases()
    streams = {"a": SF.mixed_chain() + cases["dual_prime_field_pictures"] + cases["skipped_b"],
               "b": cases["16x8"] + cases["concealment_vectors"] + SF.clamped_cases()["dual_frame"] + SF.lone_cases()["then_a_frame_picture"][0]}
    for name, data in streams.items():
        path = tmp_path / (name + ".m2v")
        path.write_bytes(data)
        r = subprocess.run([str(out / "mpeg2_field_asan"), str(path), "1", "1250"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-4000:]
        assert "ok: 1250 trials" in r.stdout
        assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
