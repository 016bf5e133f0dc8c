"""MPEG-2 (codec_type 4) without a GPU.

No MPEG-2 encoder or decoder is available to pin the syntax against, so it is pinned the way H.264 and HEVC are here: the standard typed out twice.
tests/mpeg2_ref.py restates 13818-2 in numpy with tables typed by hand; the product's host path -- splitter, header and slice parser and the
reconstruction of mpeg2_recon.h, whose routines k_mpeg2_recon runs -- is built with g++ (tests/native/mpeg2_check.cpp) and must equal it bit for bit
on scripted streams (tests/scripted_mpeg2.py), and its tables must equal the restatement's.  Analytic cases check both against answers worked out in
the test itself; the IDCT is held to IEEE 1180-1990 with the standard's own generator.  Then parse-only handles through the library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpeg_ref
import mpeg2_ref as R
import scripted_mpeg2 as S
from jmcodec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libmpeg2_check.so")
    csrc = os.path.join(ROOT, "jmcodec_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "mpeg2_check.cpp"), os.path.join(csrc, "mpeg2_syntax.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("mpeg2_syntax.h", "mpeg2_recon.h", "mpeg2_jobs.h", "jpeg_recon.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so] + srcs)
    l = C.CDLL(so)
    l.m2c_decode.restype = C.c_long
    l.m2c_decode.argtypes = [C.c_char_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    l.m2c_error.restype = C.c_char_p
    l.m2c_idct.argtypes = [C.c_void_p, C.c_void_p, C.c_long]

    def decode(data, chunk=0):
        """chunk: bytes per call, 0 = all at once, -1 = one start-code unit per call -> (n, [(NV12 bytes, w, h)], (errors, dropped, clamped))"""
        out_buf, dims, st = C.create_string_buffer(1 << 22), (C.c_int * 128)(), (C.c_int * 3)()
        n = l.m2c_decode(data, len(data), chunk, out_buf, len(out_buf), dims, 64, st)
        frames, o = [], 0
        for i in range(max(n, 0)):
            w, h = dims[2 * i], dims[2 * i + 1]
            frames.append((out_buf.raw[o:o + w * h * 3 // 2], w, h))
            o += w * h * 3 // 2
        return n, frames, tuple(st)
    decode.lib = l
    return decode


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
def _cpp_table(l, which):
    v = (C.c_int * 4)()
    n = l.m2c_table(which, 0, v)
    out = []
    for i in range(n):
        l.m2c_table(which, i, v)
        out.append((format(v[0], "0%db" % v[1]), v[2], v[3]))
    return out


def test_cpp_tables_equal_the_restatements(native):
    l = native.lib
    assert {a: c for c, a, _ in _cpp_table(l, 1)} == {**R.B1, 34: R.B1_ESCAPE}
    flags = lambda a: (a & 1, a >> 1 & 1, a >> 2 & 1, a >> 3 & 1, a >> 4 & 1)      # noqa: E731
    for which, t in ((2, R.B2), (3, R.B3), (4, R.B4)):
        assert {flags(a): c for c, a, _ in _cpp_table(l, which)} == t
    for which, t in ((9, R.B9), (10, R.B10), (12, R.B12), (13, R.B13)):
        assert {a: c for c, a, _ in _cpp_table(l, which)} == t
    for which, t in ((14, R.B14), (15, R.B15)):
        assert {(R.EOB if a == -1 else R.ESC if a == -2 else (a, b)): c for c, a, b in _cpp_table(l, which)} == t
    assert [[l.m2c_scan(alt, k) for k in range(64)] for alt in (0, 1)] == R.SCAN
    assert [l.m2c_default_intra(k) for k in range(64)] == R.DEFAULT_INTRA
    assert [[l.m2c_quantiser_scale(t, c) for c in range(32)] for t in (0, 1)] == [[2 * c for c in range(32)], R.NONLINEAR_SCALE]
    assert all(sorted(s) == list(range(64)) for s in R.SCAN)


@pytest.mark.parametrize("name", ["B1", "B2", "B3", "B4", "B9", "B10", "B12", "B13", "B14", "B15"])
def test_tables_are_prefix_free_with_kraft_sum_at_most_one(name):
    t = getattr(R, name)
    codes = list(t.values()) + ([R.B1_ESCAPE] if name == "B1" else [])
    if name in ("B14", "B15"):                      # every (run, level) code is followed by its sign bit
        codes = [c + s for k, c in t.items() if k not in (R.EOB, R.ESC) for s in "01"] + [t[R.EOB], t[R.ESC]]
    if name == "B10":
        codes = [c + s for k, c in t.items() if k for s in "01"] + [t[0]]
    assert len(set(codes)) == len(codes)
    assert not any(a != b and b.startswith(a) for a in codes for b in codes)
    assert sum(2.0 ** -len(c) for c in codes) <= 1.0


def test_dct_tables_code_the_same_111_pairs_and_the_anchors():
    pairs14 = {k for k in R.B14 if k not in (R.EOB, R.ESC)}
    assert pairs14 == {k for k in R.B15 if k not in (R.EOB, R.ESC)} and len(pairs14) == 111
    top = {0: 40, 1: 18, 2: 5, 3: 4}
    top.update({**{r: 3 for r in (4, 5, 6)}, **{r: 2 for r in range(7, 17)}, **{r: 1 for r in range(17, 32)}})
    assert {r: max(l for rr, l in pairs14 if rr == r) for r in range(32)} == top
    assert all((r, l) in pairs14 for r in top for l in range(1, top[r] + 1))
    assert (R.B14[R.EOB], R.B14[(0, 1)], R.B14[(1, 1)], R.B14[(0, 2)], R.B14[R.ESC]) == ("10", "11", "011", "0100", "000001")
    assert (R.B15[R.EOB], R.B15[(0, 1)]) == ("0110", "10")
    # (0, 1) as the first coefficient of a non-intra block is "1s": a P macroblock with that single level decodes to it
    QF = [0] * 64
    QF[0] = -1
    data = S.build([("seq", dict(width=16, height=16)), ("pic", S.staircase(16, 16)),
                    ("pic", dict(type="P", f_code=((1, 1), (15, 15)), slices=[dict(row=0, qcode=8, mbs=[dict(x=0, blocks={0: QF})])]))])
    assert b"\x00\x00\x01\x01" + bytes([0b01000010, 0b11010111, 0b00000000]) in data      # code 8, extra 0, mba 1, type 01 | cbp 32 = 1010, "1" + sign 1, EOB 10
    f = R.decode_stream(data, 0)[1][0]
    assert f[0] == 40 - 3 and len(R.decode_stream(data, 0)) == 2      # F = (2 * -1 - 1) * 16 * 16 / 32 = -24: a DC of -24 lowers the flat 40 by 3
    assert R.NONLINEAR_SCALE[1:] == list(range(1, 9)) + list(range(10, 25, 2)) + list(range(28, 57, 4)) + list(range(64, 113, 8))
    assert len(R.NONLINEAR_SCALE) == 32


# ---- the IDCT -----------------------------------------------------------------------------------------------------------------------------------
def test_idct_matrix_is_jpeg_refs(native):
    assert [[native.lib.m2c_idct_m(k, n) for n in range(8)] for k in range(8)] == jpeg_ref.M.tolist()


def _ieee1180_blocks(lo, hi, n):
    """IEEE 1180-1990's generator: randx = randx * 1103515245 + 12345 in 32-bit arithmetic; x = (randx & 0x7ffffffe) / 0x7fffffff * (L + H + 1); the
    value is int(x) - L.  n blocks of 64, seed 1."""
    randx, out = 1, np.empty(n * 64, np.int64)
    for i in range(n * 64):
        randx = (randx * 1103515245 + 12345) & 0xFFFFFFFF
        out[i] = int((randx & 0x7FFFFFFE) / float(0x7FFFFFFF) * (lo + hi + 1)) - lo
    return out.reshape(n, 8, 8)


@pytest.mark.parametrize("lo,hi,sign", [(256, 255, 1), (256, 255, -1), (5, 5, 1), (5, 5, -1), (300, 300, 1), (300, 300, -1)])
def test_idct_meets_ieee_1180(native, lo, hi, sign):
    """13818-2 Annex A: the IDCT meets IEEE 1180-1990.  10 000 blocks per range and sign: forward DCT in double precision, rounded and clipped to
    [-2048, 2047]; the reference IDCT in double precision, rounded and clipped to [-256, 255]; the product's IDCT on the same coefficients.  The
    limits asserted are the standard's: peak error 1, per-sample mean square error 0.06, overall 0.02, per-sample mean error 0.015, overall 0.0015;
    and all-zero in gives all-zero out."""
    n = 10000
    x = sign * _ieee1180_blocks(lo, hi, n)
    c = np.array([[(np.sqrt(0.125) if k == 0 else 0.5) * np.cos((2 * j + 1) * k * np.pi / 16) for j in range(8)] for k in range(8)])
    F = np.clip(np.floor(np.einsum("vy,nyx,ux->nvu", c, x.astype(float), c) + 0.5), -2048, 2047)
    ref = np.clip(np.floor(np.einsum("vy,nvu,ux->nyx", c, F, c) + 0.5), -256, 255)
    Fi = np.ascontiguousarray(F.astype(np.int32))
    got = np.zeros_like(Fi)
    native.lib.m2c_idct(Fi.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p), n)
    e = got.astype(float) - ref
    assert np.abs(e).max() <= 1
    assert (e ** 2).mean(axis=0).max() <= 0.06
    assert (e ** 2).mean() <= 0.02
    assert np.abs(e.mean(axis=0)).max() <= 0.015
    assert abs(e.mean()) <= 0.0015
    zero = np.zeros((1, 8, 8), np.int32)
    out = np.ones_like(zero)
    native.lib.m2c_idct(zero.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 1)
    assert not out.any()
    # ... and the restatement's IDCT is the same function
    assert np.array_equal(np.array([R.idct(Fi[i].reshape(64)) for i in range(50)]), got[:50])


# ---- analytic cases: the answers come from arithmetic here, not from any decoder ------------------------------------------------------------
def planes(frame, w, h):
    a = np.frombuffer(frame, np.uint8)
    return a[:w * h].reshape(h, w).astype(int), a[w * h:].reshape(h // 2, w // 2, 2)[:, :, 0].astype(int), a[w * h:].reshape(h // 2, w // 2, 2)[:, :, 1].astype(int)


def both(native, items):
    """the stream through the host path and through the restatement: equal, clean; -> [(Y, Cb, Cr)] per display frame"""
    data = S.build(items)
    n, frames, st = native(data)
    assert frames == R.decode_stream(data, 0) and st == (0, 0, 0), st
    return [planes(f, w, h) for f, w, h in frames]


def stair(w, h, base=40, step=7):
    """what staircase() decodes to: flat macroblocks of value base + step * index, every plane (8 * value / 8: the DC alone)"""
    mb_w, mb_h = w // 16, h // 16
    v = base + step * np.arange(mb_w * mb_h).reshape(mb_h, mb_w)
    return np.kron(v, np.ones((16, 16), int)), np.kron(v, np.ones((8, 8), int))


W, H = 64, 48
SEQ = ("seq", dict(width=W, height=H))


def ppic(mbs_of_row, rows=3, **kw):
    return ("pic", dict(dict(type="P", f_code=((3, 3), (15, 15)), slices=[dict(row=r, qcode=4, mbs=mbs_of_row(r)) for r in range(rows)]), **kw))


def two_passes(F):
    """the integer IDCT of INTEGRATION.md on F[v][u]: g[y][u] = clip((sum_v M[v][y] F[v][u] + 256) >> 9), r[y][x] = clip((sum_u M[u][x] g[y][u] + 65536) >> 17)"""
    g = np.clip((jpeg_ref.M.T @ F + 256) >> 9, -65536, 65535)
    return np.clip((g @ jpeg_ref.M + 65536) >> 17, -256, 255)


def test_all_zero_intra_blocks_give_128(native):
    for p in range(4):
        pic = dict(type="I", intra_dc_precision=p, slices=[dict(row=0, qcode=9, mbs=[dict(x=0, intra=True, blocks={})])])
        (Y, Cb, Cr), = both(native, [("seq", dict(width=16, height=16)), ("pic", pic)])
        assert (Y == 128).all() and (Cb == 128).all() and (Cr == 128).all()


@pytest.mark.parametrize("p", [0, 1, 2, 3])
def test_dc_only_block_is_flat_at_each_precision(native, p):
    # QF_dc = v << p, intra_dc_mult = 8 >> p: F[0][0] = 8 v whatever the precision, and a DC of 8 v is a flat v
    (Y, Cb, Cr), = both(native, [SEQ, ("pic", S.staircase(W, H, precision=p, base=33 + p))])
    y, c = stair(W, H, base=33 + p)
    assert np.array_equal(Y, y) and np.array_equal(Cb, c) and np.array_equal(Cr, c)
    # the smallest and the largest DC level: F[0][0] = (8 >> p) * level, F[7][7] = 1 when that is even (mismatch control), through the two passes
    for level in (1, (1 << (8 + p)) - 1):
        pic = dict(type="I", intra_dc_precision=p, slices=[dict(row=0, qcode=9, mbs=[dict(x=0, intra=True, blocks={k: [level] + [0] * 63 for k in range(6)})])])
        (Y, _, _), = both(native, [("seq", dict(width=16, height=16)), ("pic", pic)])
        F = np.zeros((8, 8), np.int64)
        F[0, 0] = level * (8 >> p)
        F[7, 7] = 1 - (F[0, 0] & 1)
        assert np.array_equal(Y, np.kron(np.ones((2, 2), int), np.clip(two_passes(F), 0, 255)))


@pytest.mark.parametrize("level", [2047, -2047])
def test_saturation_and_mismatch_control_at_escape_levels(native, level):
    """An intra AC level of +-2047 at W = 16, quantiser_scale 62: 2 * 2047 * 16 * 62 / 32 = +-126 914, saturated to 2047 / -2048.  With the DC at
    1024 the sum is 3071 (odd: F[7][7] stays 0) or -1024 (even: F[7][7] becomes 1).  The block is the IDCT of exactly that F, by the two integer passes."""
    QF = [128] + [0] * 63
    QF[1] = level
    pic = dict(type="I", slices=[dict(row=0, qcode=31, mbs=[dict(x=0, intra=True, blocks={0: QF})])])
    (Y, _, _), = both(native, [("seq", dict(width=16, height=16, intra_matrix=[16] * 64)), ("pic", pic)])
    F = np.zeros((8, 8), np.int64)
    F[0, 0], F[0, 1] = 1024, (2047 if level > 0 else -2048)
    if level < 0:
        F[7, 7] = 1
    assert np.array_equal(Y[:8, :8], np.clip(two_passes(F), 0, 255)) and (Y[8:, :] == 128).all()
    assert Y[0, 0] == 255 if level > 0 else Y[0, 0] == 0


def test_p_picture_of_integer_vector_copies(native):
    y, c = stair(W, H)
    vec = {0: (32, 0), 1: (-32, 32), 2: (0, -64)}                                 # half samples: 16 right; 16 left and 16 down; 32 up
    mbs = lambda r: [dict(x=x, fwd=[vec[r] if 0 <= x * 16 + vec[r][0] // 2 <= W - 16 and 0 <= r * 16 + vec[r][1] // 2 <= H - 16 else (0, 0)]) for x in range(4)]      # noqa: E731
    _, (Y, Cb, Cr) = both(native, [SEQ, ("pic", S.staircase(W, H)), ppic(mbs)])
    for r in range(3):
        for x in range(4):
            vx, vy = mbs(r)[x]["fwd"][0]
            sx, sy = x * 16 + vx // 2, r * 16 + vy // 2
            assert np.array_equal(Y[r * 16:r * 16 + 16, x * 16:x * 16 + 16], y[sy:sy + 16, sx:sx + 16]), (r, x)
            assert np.array_equal(Cb[r * 8:r * 8 + 8, x * 8:x * 8 + 8], c[sy // 2:sy // 2 + 8, sx // 2:sx // 2 + 8]), (r, x)


@pytest.mark.parametrize("hx,hy", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_half_sample_phases_luma_and_chroma(native, hx, hy):
    """Macroblock (1, 1) predicted from 7 + hx / 2 to the left and 5 + hy / 2 up... in luma half samples (-15 + hx... ), so its window straddles four
    flat macroblocks; chroma: the vector / 2 toward zero, with its own half-sample flags."""
    y, c = stair(W, H)
    vx, vy = -14 + hx, -10 + hy
    mbs = lambda r: [dict(x=x, fwd=[(vx, vy) if (x, r) == (1, 1) else (0, 0)]) for x in range(4)]      # noqa: E731
    _, (Y, Cb, Cr) = both(native, [SEQ, ("pic", S.staircase(W, H)), ppic(mbs)])

    def interp(p, x0, y0, n, mx, my):
        ix, iy, fx, fy = x0 + (mx >> 1), y0 + (my >> 1), mx & 1, my & 1
        a, b = p[iy:iy + n, ix:ix + n], p[iy:iy + n, ix + fx:ix + fx + n]
        cc, d = p[iy + fy:iy + fy + n, ix:ix + n], p[iy + fy:iy + fy + n, ix + fx:ix + fx + n]
        return (a + b + cc + d + 2) >> 2 if fx and fy else (a + b + 1) >> 1 if fx else (a + cc + 1) >> 1 if fy else a
    assert np.array_equal(Y[16:32, 16:32], interp(y, 16, 16, 16, vx, vy))
    cvx, cvy = -((-vx) // 2), -((-vy) // 2)                                       # / 2 truncating toward zero (both are negative here)
    assert np.array_equal(Cb[8:16, 8:16], interp(c, 8, 8, 8, cvx, cvy)) and np.array_equal(Cr[8:16, 8:16], interp(c, 8, 8, 8, cvx, cvy))
    assert np.array_equal(Y[:16], y[:16]) and np.array_equal(Y[32:], y[32:])


def test_vector_of_minus_three_gives_chroma_minus_one(native):
    """-3 / 2 = -1 (toward zero), not -2: the chroma sample is the mean of positions x - 1 and x; luma is the mean of x - 2 and x - 1."""
    y, c = stair(W, H)
    mbs = lambda r: [dict(x=x, fwd=[(-3, 0) if (x, r) == (2, 0) else (0, 0)]) for x in range(4)]      # noqa: E731
    _, (Y, Cb, _) = both(native, [SEQ, ("pic", S.staircase(W, H)), ppic(mbs)])
    assert np.array_equal(Y[0:16, 32:48], (y[0:16, 30:46] + y[0:16, 31:47] + 1) >> 1)
    assert np.array_equal(Cb[0:8, 16:24], (c[0:8, 15:23] + c[0:8, 16:24] + 1) >> 1)
    assert Cb[0, 16] == (c[0, 15] + c[0, 16] + 1) >> 1 != c[0, 15]


def test_bidirectional_rounding_and_skipped_b_repeats_its_neighbour(native):
    """Anchors: staircases of base 40 and base 45 (values of different parity in every macroblock: 40 + 7 k, 45 + 7 k).  Row 0 of the B picture is
    bidirectional with zero vectors: (f + b + 1) >> 1.  Row 1: macroblock 0 forward by 16 samples to the right, macroblocks 1 and 2 skipped (they
    repeat that motion from their own positions), macroblock 3 coded."""
    y0, c0 = stair(W, H, base=40)
    y1, c1 = stair(W, H, base=45)
    p1 = S.staircase(W, H, base=45)
    p1.update(type="P", f_code=((1, 1), (15, 15)))
    b = dict(type="B", f_code=((3, 1), (1, 1)), slices=[
        dict(row=0, qcode=4, mbs=[dict(x=x, fwd=[(0, 0)], bwd=[(0, 0)]) for x in range(4)]),
        dict(row=1, qcode=4, mbs=[dict(x=0, fwd=[(32, 0)]), dict(x=3, fwd=[(0, 0)])]),
        dict(row=2, qcode=4, mbs=[dict(x=x, bwd=[(0, 0)]) for x in range(4)])])
    _, (Y, Cb, _), _ = both(native, [SEQ, ("pic", S.staircase(W, H)), ("pic", p1), ("pic", b)])
    assert np.array_equal(Y[:16], (y0[:16] + y1[:16] + 1) >> 1) and np.array_equal(Cb[:8], (c0[:8] + c1[:8] + 1) >> 1)
    assert ((y0[:16] + y1[:16]) & 1).all()                                       # every sample exercises the rounding
    assert np.array_equal(Y[16:32, 0:48], y0[16:32, 16:64]) and np.array_equal(Y[16:32, 48:], y0[16:32, 48:])
    assert np.array_equal(Y[32:], y1[32:])


@pytest.mark.parametrize("s0,s1", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_field_dct_and_field_prediction_with_each_select(native, s0, s1):
    """An I picture of field-DCT macroblocks whose top-field blocks are flat 60 and bottom-field blocks flat 150: its lines alternate 60 / 150 (that is
    field DCT).  A P picture predicts the top lines from the field s0 selects and the bottom lines from field s1, zero vectors."""
    seq = ("seq", dict(width=32, height=32, progressive_sequence=0))
    blocks = {k: [(60, 60, 150, 150, 90, 200)[k]] + [0] * 63 for k in range(6)}
    ipic = dict(type="I", frame_pred_frame_dct=0, progressive_frame=0, slices=[dict(row=r, qcode=4, mbs=[dict(x=x, intra=True, field_dct=1, blocks=blocks)
                                                                                                      for x in range(2)]) for r in range(2)])
    ppicture = dict(type="P", frame_pred_frame_dct=0, progressive_frame=0, f_code=((1, 1), (15, 15)),
                    slices=[dict(row=r, qcode=4, mbs=[dict(x=x, fwd=[(s0, 0, 0), (s1, 0, 0)]) for x in range(2)]) for r in range(2)])
    (Yi, Cbi, Cri), (Y, Cb, Cr) = both(native, [seq, ("pic", ipic), ("pic", ppicture)])
    assert (Yi[0::2] == 60).all() and (Yi[1::2] == 150).all() and (Cbi == 90).all() and (Cri == 200).all()
    assert (Y[0::2] == (60, 150)[s0]).all() and (Y[1::2] == (60, 150)[s1]).all() and (Cb == 90).all() and (Cr == 200).all()


# ---- the host path against the restatement ------------------------------------------------------------------------------------------------------
_CASES = dict(S.feature_cases())
_CASES.update(chain=S.chain_stream(), clamped=S.clamped_stream(), truncated=S.truncated_stream(), size_change=S.size_change_stream())
_CASES.update({f"size_{w}x{h}": S.sized_stream(w * h, w, h, p) for w, h, p in
               ((16, 16, 1), (48, 32, 1), (40, 24, 1), (88, 56, 1), (48, 40, 0), (272, 16, 1), (16, 272, 1))})


@pytest.mark.parametrize("name", sorted(_CASES))
def test_host_path_equals_restatement_on_scripted_cases_in_every_chunking(native, name):
    data, info = _CASES[name], {}
    want = R.decode_stream(data, 0, info)
    for chunk in (0, -1, 1, 5):
        n, frames, (errors, dropped, clamped) = native(data, chunk)
        assert n == len(want) and frames == want, chunk
        assert (errors, dropped, clamped) == (info["errors"], info["dropped"], info["clamped"])
    assert (info["errors"] > 0) == (name in ("clamped", "truncated"))


def test_start_code_prefix_without_a_code_byte_is_skipped(native):
    """00 00 01 directly in front of another start code, at the beginning, between two pictures and at the very end: a unit of no bytes"""
    data = S.chain_stream(n=4)
    i = data.find(b"\x00\x00\x01\x00", 20)
    odd = b"\x00\x00\x01" + data[:i] + b"\x00\x00\x01\x00\x00\x01" + data[i:] + b"\x00\x00\x01"
    want = R.decode_stream(data, 0)
    assert R.decode_stream(odd, 0) == want
    for chunk in (0, -1, 1, 7):
        n, frames, st = native(odd, chunk)
        assert frames == want and st == (0, 0, 0), chunk


@pytest.mark.parametrize("block", range(6))
def test_host_path_equals_restatement_on_seeded_random_scripts(native, block):
    """300 random scripts, each at most 64 x 64 and 4 pictures, all with conforming vectors: clean on both sides, equal frames."""
    for seed in range(1000 + 50 * block, 1050 + 50 * block):
        data, info = S.random_stream(seed), {}
        want = R.decode_stream(data, 0, info)
        n, frames, st = native(data)
        assert frames == want and st == (0, 0, 0) and info["errors"] == 0, seed


# ---- through the library, parse only ----------------------------------------------------------------------------------------------------------
STATS = ("errors", "dropped_pictures", "frames", "fps_num", "fps_den", "interlaced_sequence", "syntax_digest", "i_pictures", "p_pictures", "b_pictures",
         "coded_width", "coded_height", "out_width", "out_height", "sar_num", "sar_den", "mpeg2_repeat_first_field", "failed")


def parse(data, chunks=None, **opt):
    with api.JmAmdDec(4, 1, options=dict(parse_only=1, **opt)) as d:
        n = d.decode_stream(data, keep=False, chunks=chunks if chunks is not None else [data])
        st = {k: d.stat(k) for k in STATS}
        st["order"] = [d.stat(f"display_poc:{i}") for i in range(n)]
        st["info"] = api.jm_nvdec_show_dec_info(d.h)
        st["size"] = api.jm_nvdec_stream_info(d.h)
        return n, st


def test_counts_stream_info_frame_rate_and_interlace():
    data = S.build([("seq", dict(width=48, height=40, progressive_sequence=0, frame_rate_code=4, fr_ext=(1, 2), aspect=3,
                                 display=dict(matrix=5, w=48, h=36)))] +
                   [("pic", S.random_picture(np.random.default_rng(i), t, 48, 40, 0, repeat_first_field=i & 1)) for i, t in enumerate("IPBB")])
    n, st = parse(data)
    assert n == 4 == st["frames"] and (st["i_pictures"], st["p_pictures"], st["b_pictures"]) == (1, 1, 2) and st["errors"] == 0
    assert (st["fps_num"], st["fps_den"]) == (30000 * 2, 1001 * 3) and st["interlaced_sequence"] == 1
    assert (st["coded_width"], st["coded_height"], st["out_width"], st["out_height"]) == (48, 64, 48, 40)
    assert (st["sar_num"], st["sar_den"]) == (16 * 36 // 144, 9 * 48 // 144)          # 16:9 over the display area 48 x 36: 576 : 432 = 4 : 3
    assert st["mpeg2_repeat_first_field"] == 2                                      # recorded; no frame is repeated
    assert "MPEG-2" in str(st["info"])
    prog = S.sized_stream(1, 48, 32, 1, "I")
    assert parse(prog)[1]["interlaced_sequence"] == 0


def test_syntax_digest_is_invariant_under_chunking():
    data = S.chain_stream()
    digests = {parse(data, chunks, digest=1)[1]["syntax_digest"] for chunks in
               (None, api.split_nalus(data), [data[i:i + 1] for i in range(len(data))], [data[i:i + 5] for i in range(0, len(data), 5)])}
    assert len(digests) == 1
    assert parse(S.chain_stream(seed=78), digest=1)[1]["syntax_digest"] not in digests


def test_display_order_and_dropped_leading_b_pictures():
    n, st = parse(S.chain_stream(n=7))                     # coding order I P B B P B B
    assert st["order"] == [0, 2, 3, 1, 5, 6, 4] and st["dropped_pictures"] == 0
    # an open group at the start: B B before the first anchor pair, and a P picture before the first I
    n, st = parse(S.sized_stream(3, 48, 40, 0, "PBBIBBPBB"))
    assert n == 4 and st["dropped_pictures"] == 5 and st["errors"] == 0 and st["order"] == [0, 2, 3, 1]
    assert (st["i_pictures"], st["p_pictures"], st["b_pictures"]) == (1, 1, 2)


def test_size_change_mid_stream():
    n, st = parse(S.size_change_stream())
    assert n == 7 and st["errors"] == 0 and (st["out_width"], st["out_height"], st["coded_height"]) == (80, 48, 64)


def _refusal_streams():
    rng = np.random.default_rng(9)
    seq = dict(width=32, height=32)
    ipic = S.random_picture(rng, "I", 32, 32)
    p_dual = dict(type="P", frame_pred_frame_dct=0, f_code=((1, 1), (15, 15)), slices=[dict(row=0, qcode=4, mbs=[dict(x=0, fwd=[(0, 0)], motion_type=3)])])
    ext = lambda ident: ("raw", b"\x00\x00\x01\xb5" + bytes([ident << 4, 0, 0, 0]))      # noqa: E731
    return {
        "MPEG-1": ([("seq", dict(seq, ext=False)), ("pic", dict(ipic, ext=False))], "MPEG-1"),
        "field pictures": ([("seq", seq), ("pic", dict(ipic, picture_structure=1))], "field pictures"),
        "dual prime": ([("seq", seq), ("pic", ipic), ("pic", p_dual)], "dual-prime"),
        "4:2:2": ([("seq", dict(seq, chroma_format=2)), ("pic", ipic)], "4:2:2"),
        "4:4:4": ([("seq", dict(seq, chroma_format=3)), ("pic", ipic)], "4:4:4"),
        "sequence scalable": ([("seq", seq), ext(5), ("pic", ipic)], "scalable"),
        "spatial scalable": ([("seq", seq), ("pic", ipic), ext(9)], "scalable"),
        "D pictures": ([("seq", seq), ("pic", dict(type="D", slices=[]))], "D pictures"),
        "slice_vertical_position_extension": ([("seq", dict(width=32, height=2816)), ("pic", ipic)], "slice_vertical_position_extension"),
    }


@pytest.mark.parametrize("name", sorted(_refusal_streams()))
def test_refusals_name_the_feature(name, native):
    items, word = _refusal_streams()[name]
    data = S.build(items)
    with api.JmAmdDec(4, 1, options=dict(parse_only=1)) as d:
        with pytest.raises(RuntimeError) as e:
            d.decode_stream(data, keep=False, chunks=[data])
        msg = api.lib().jm_amddec_last_error(d.h).decode()
        assert d.stat("failed") == 1
    assert "not supported" in msg and word in msg, (msg, str(e.value))
    n, _, _ = native(data)
    assert n == -1 and word in native.lib.m2c_error().decode()
    with pytest.raises(R.Refused):
        R.decode_stream(data, 0)


@pytest.mark.parametrize("codec", [3, 5, 6, 7])
def test_other_codec_types_are_still_refused(codec):
    with pytest.raises(RuntimeError, match=r"0 \(H.264\), 1 \(HEVC\), 2 \(MJPEG\) and 4 \(MPEG-2\)"):
        api.JmAmdDec(codec, 1, options=dict(parse_only=1))


def test_deinterlace_temporal_is_refused_for_codec_4():
    with pytest.raises(RuntimeError, match="deinterlace_temporal"):
        api.JmAmdDec(4, 1, options=dict(parse_only=1, deinterlace=2, deinterlace_temporal=1))


def test_damage_finishes_with_errors():
    data = S.truncated_stream()
    n, st = parse(data)
    assert n == 3 and st["errors"] >= 2 and st["failed"] == 0
    n, st = parse(data[:len(data) * 2 // 3] + b"\x00\x00\x01\xb7")
    assert n >= 1 and st["errors"] > 0 and st["failed"] == 0


def test_split_mpeg2_pictures_helper():
    data = S.chain_stream(n=5)
    parts = api.split_mpeg2_pictures(data)
    assert b"".join(parts) == data and len(parts) == 5 and all(p.count(b"\x00\x00\x01\x00") == 1 for p in parts)
    n, st = parse(data, chunks=parts)
    assert n == 5 and st["errors"] == 0


# ---- the sanitizer harness -----------------------------------------------------------------------------------------------------------
def test_fuzz_mpeg2_builds_and_runs_clean(tmp_path):
    """tools/fuzz_mpeg2.cpp: a stand-alone host program (its own main) under AddressSanitizer / UBSan, a few seconds of mutated scripted streams"""
    out = tmp_path / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "fuzz_mpeg2_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    path = tmp_path / "a.m2v"
    path.write_bytes(S.chain_stream(n=7) + S.sized_stream(3, 48, 40, 0, "IPBB") + S.feature_cases()["b_field_bidirectional"])
    r = subprocess.run([str(out / "fuzz_mpeg2_asan"), str(path), "1", "150"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ok: 150 trials" in r.stdout
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
