"""Motion-adaptive deinterlaced output (option deinterlace_temporal), host side (no GPU): the closed forms of the function D3 on its numpy
restatement (deint3_ref.py), the strip routine of k_deint3 (jmcodec_amd/csrc/deint3_packed.h, host build) against that restatement, the same routine
under the sanitizers (tools/deint3_asan.cpp), the option's range, and what parse-only handles report per output frame against the stream
generator's own listing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from deint_ref import deint_plane
from deint3_ref import deint3_frame, deint3_plane
from jmcodec_amd import api
from tools import streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the closed forms of the definition, on the restatement --------------------------------------------------------------------
def _bob(P, p):
    return deint_plane(P, 1, p)


def test_identical_frames_stay_woven():
    rng = np.random.default_rng(0xD3)
    for H, W in ((2, 1), (2, 7), (5, 9), (16, 33)):
        for P in (rng.integers(0, 256, (H, W), dtype=np.uint8), np.where(np.arange(H)[:, None] & 1, 255, 0).astype(np.uint8) * np.ones((1, W), np.uint8)):
            for p in (0, 1):
                for T in (1, 10, 255):
                    assert np.array_equal(deint3_plane(P, P.copy(), p, T), P)


def test_everything_moving_is_bob():
    rng = np.random.default_rng(0xD4)
    for H, W in ((2, 1), (2, 6), (7, 5), (12, 40)):
        for T in (1, 10, 100):
            P = rng.integers(0, 255 - T, (H, W), dtype=np.uint8)
            Q = (P + np.uint8(T + 1)).astype(np.uint8) if T != 10 else np.full((H, W), 255, np.uint8)
            assert (np.abs(P.astype(int) - Q.astype(int)) > T).all()
            for p in (0, 1):
                assert np.array_equal(deint3_plane(P, Q, p, T), _bob(P, p))


@pytest.mark.parametrize("T", [1, 10, 120])
def test_one_sample_moves_its_clamped_neighbourhood_and_no_more(T):
    """One sample differing by T + 1 interpolates exactly the missing-row samples of its clamped 3 x 3 neighbourhood; by exactly T, nothing.  At the
    plane's edges too: columns 0 / W - 1, rows 0 / H - 1, H = 2."""
    rng = np.random.default_rng(0xD5 + T)
    for H, W in ((2, 1), (2, 5), (3, 4), (6, 7), (9, 18)):
        P = rng.integers(0, 256, (H, W), dtype=np.uint8)
        for r in sorted({0, 1, H // 2, H - 2, H - 1}):
            for c in sorted({0, 1, W // 2, W - 1} & set(range(W))):
                for delta, moves in ((T, False), (T + 1, True)):
                    Q = P.copy()
                    Q[r, c] = int(P[r, c]) + delta if int(P[r, c]) + delta <= 255 else int(P[r, c]) - delta     # (delta <= 121: one of them fits)
                    for p in (0, 1):
                        want = P.copy()
                        if moves:
                            bob = _bob(P, p)
                            for y in range(H):
                                if (y & 1) == p:
                                    continue
                                up = y - 1 if y - 1 >= 0 else y + 1
                                dn = y + 1 if y + 1 < H else y - 1
                                if r in (up, y, dn):
                                    lo, hi = max(c - 1, 0), min(c + 1, W - 1)
                                    want[y, lo:hi + 1] = bob[y, lo:hi + 1]
                        assert np.array_equal(deint3_plane(P, Q, p, T), want), (H, W, r, c, delta, p)


# ---- deint3_packed.h against the restatement -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libdeint3_packed_check.so")
    src = os.path.join(ROOT, "tests", "native", "deint3_packed_check.cpp")
    hdrs = [os.path.join(ROOT, "jmcodec_amd", "csrc", h) for h in ("deint3_packed.h", "deint2_packed.h", "deint_packed.h", "mc_packed.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so, src])
    l = C.CDLL(so)
    l.dei3_plane.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 4 + [C.c_int] * 2
    l.dei3_plane.restype = None
    l.dei3_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 2 + [C.c_int] * 3
    l.dei3_frame.restype = None
    return l


def _aligned(n, misalign=0):
    """n bytes whose first one lies `misalign` bytes behind a 16-byte boundary (a view; the base array stays alive through it)."""
    raw = np.zeros(n + 32, np.uint8)
    off = (-raw.ctypes.data) % 16 + misalign
    return raw[off:off + n]


def _plane_buf(P, pitch, misalign, fill):
    H, W = P.shape
    b = _aligned(H * pitch, misalign)
    b[:] = fill
    b.reshape(H, pitch)[:, :W] = P
    return b


def _run(lib, P, Q, step, T, p=0, both=True, pitch=None, qpitch=None, dst_pitch=None, misalign=0, split=False):
    """The strip routine over a whole plane (H x W bytes; step 2: interleaved chroma).  both: returns [top kept, bottom kept]; else [parity p kept].
    split: each output as its two planes."""
    H, W = P.shape
    src = _plane_buf(P, pitch or W, misalign, 0x5A)
    prev = _plane_buf(Q, qpitch or W, misalign, 0x3C)           # (different padding: nothing outside the W bytes may enter the decision)
    n_out = 2 if both else 1
    if split:
        d = [_aligned(H * (W // 2)) for _ in range(2 * n_out)]
        for x in d:
            x[:] = 0xA5
        ptr = [x.ctypes.data for x in d]
        if not both:
            ptr = ptr + [None, None] if p == 0 else [None, None] + ptr
        lib.dei3_plane(src.ctypes.data, pitch or W, prev.ctypes.data, qpitch or W, W, H, step, p, int(both), T, ptr[0], ptr[1], ptr[2], ptr[3], W // 2, 1)
        return [x.reshape(H, W // 2).copy() for x in d]
    dp = dst_pitch or W
    dst = [_aligned(H * dp) for _ in range(n_out)]
    for x in dst:
        x[:] = 0xA5
    ptr = [x.ctypes.data for x in dst]
    if not both:
        ptr = ptr + [None] if p == 0 else [None] + ptr
    lib.dei3_plane(src.ctypes.data, pitch or W, prev.ctypes.data, qpitch or W, W, H, step, p, int(both), T, ptr[0], None, ptr[1], None, dp, 0)
    outs = [x.reshape(H, dp) for x in dst]
    for o in outs:
        assert (o[:, W:] == 0xA5).all()                 # nothing is written beyond the W bytes of a row
    return [o[:, :W].copy() for o in outs]


def _ref(P, Q, step, p, T):
    if step == 1:
        return deint3_plane(P, Q, p, T)
    out = np.empty_like(P)
    out[:, 0::2] = deint3_plane(P[:, 0::2], Q[:, 0::2], p, T)
    out[:, 1::2] = deint3_plane(P[:, 1::2], Q[:, 1::2], p, T)
    return out


def _pair_of_planes(rng, H, W, kind, T):
    """P and Q: 0 noise against noise, 1 near-identical (differences around T: exactly T and T + 1 occur), 2 identical rows alternating 0 / 255 with a
    few samples moved, 3 a smooth picture with a displaced rectangle."""
    if kind == 0:
        return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == 1:
        P = rng.integers(0, 256, (H, W)).astype(np.int64)
        d = rng.choice([0, 0, 0, T - 1, T, T + 1, -T, -(T + 1)], (H, W))
        Q = np.where((P + d < 0) | (P + d > 255), P - d, P + d)
        Q = np.clip(Q, 0, 255)
        return P.astype(np.uint8), Q.astype(np.uint8)
    if kind == 2:
        P = np.zeros((H, W), np.uint8)
        P[1::2] = 255
        Q = P.copy()
        for _ in range(max(1, H * W // 40)):
            Q[rng.integers(0, H), rng.integers(0, W)] ^= 0x80
        return P, Q
    yy, xx = np.mgrid[0:H, 0:W]
    Q = ((yy * 3 + xx * 2) % 256).astype(np.uint8)
    P = Q.copy()
    y0, x0, hh, ww = H // 4, W // 4, max(1, H // 3), max(1, W // 3)
    P[y0:y0 + hh, x0:x0 + ww] = 250
    return P, Q


@pytest.mark.parametrize("step", [1, 2])
def test_strips_against_the_restatement_random(lib, step):
    """About 200 seeded planes per step: every W mod 16 (W even), H from 2 up (every H mod 8, odd row counts among them), aligned and unaligned
    pitches and bases, pitches that differ between the frame, the previous frame and the destination; four kinds of content; thresholds 1, 10, 255
    and random ones; both parities; single and paired output; NV12-style and split destinations."""
    assert lib.dei3_strip_rows() == 8
    rng = np.random.default_rng(0xD3D3 + step)
    seen_w, seen_h, share = set(), set(), [0, 0]
    for it in range(208):
        H = int(rng.integers(2, 45)) if it >= 24 else 2 + it
        W = 2 * int(rng.integers(1, 60)) if it >= 24 else 2 * (it % 8 + 1) + 16 * (it // 8)
        seen_w.add(W % 16)
        seen_h.add(H % 8)
        T = [10, 1, 255, int(rng.integers(1, 256))][it % 4] if it % 3 else 10
        P, Q = _pair_of_planes(rng, H, W, it % 4, T)
        if it % 2:                                      # 16-byte rows on every side: the fast path, with three different pitches
            pitch, qpitch, dp = ((W + 15) // 16 * 16 + 16 * int(rng.integers(0, 3)) for _ in range(3))
        else:
            pitch, qpitch, dp = W + 2 * int(rng.integers(0, 5)), W + 2 * int(rng.integers(0, 5)), W
        mis = 0 if it % 5 else 1
        want = [_ref(P, Q, step, p, T) for p in (0, 1)]
        got = _run(lib, P, Q, step, T, 0, True, pitch, qpitch, dp, mis)
        for p in (0, 1):
            assert np.array_equal(got[p], want[p]), (it, H, W, p, T, pitch, qpitch, dp, "pair")
            one = _run(lib, P, Q, step, T, p, False, pitch, qpitch, dp, mis)
            assert np.array_equal(one[0], want[p]), (it, H, W, p, T, pitch, qpitch, dp, "single")
            miss = want[p][(1 - p)::2]
            share[0] += int((miss != P[(1 - p)::2]).sum())
            share[1] += miss.size
        if step == 2:
            u0, v0, u1, v1 = _run(lib, P, Q, step, T, 0, True, pitch, qpitch, split=True)
            assert np.array_equal(u0, want[0][:, 0::2]) and np.array_equal(v0, want[0][:, 1::2]), (it, "split top")
            assert np.array_equal(u1, want[1][:, 0::2]) and np.array_equal(v1, want[1][:, 1::2]), (it, "split bottom")
            for p in (0, 1):
                u, v = _run(lib, P, Q, step, T, p, False, pitch, qpitch, split=True)
                assert np.array_equal(u, want[p][:, 0::2]) and np.array_equal(v, want[p][:, 1::2]), (it, p, "split single")
    assert seen_w == set(range(0, 16, 2)) and seen_h == set(range(8))
    assert 0.05 < share[0] / share[1] < 0.95            # both branches are taken


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("T", [1, 10, 255])
def test_strip_threshold_edge_at_every_column(lib, step, T):
    """One sample differing by exactly T (nothing moves) or by T + 1 (its neighbourhood does) at every position of a row in turn -- the plane's first
    and last columns and both sides of every 16-byte chunk edge -- on planes whose first / last rows are missing rows of one output or the other."""
    rng = np.random.default_rng(0xED6E + T)
    for Wc in (1, 2, 8, 16, 17, 33):
        W = Wc * step
        if W & 1:
            continue
        for H in (2, 3, 9):
            P = rng.integers(0, 256, (H, W), dtype=np.uint8)
            for r in range(H):
                for col in range(W):
                    for delta in (T, T + 1):
                        if delta > 255:
                            continue
                        v = int(P[r, col])
                        if v + delta > 255 and v - delta < 0:
                            continue
                        Q = P.copy()
                        Q[r, col] = v + delta if v + delta <= 255 else v - delta
                        got = _run(lib, P, Q, step, T, pitch=(W + 15) // 16 * 16, qpitch=(W + 15) // 16 * 16 + 16, dst_pitch=(W + 15) // 16 * 16)
                        for p in (0, 1):
                            want = _ref(P, Q, step, p, T)
                            assert np.array_equal(got[p], want), (Wc, H, r, col, delta, p)


def test_whole_frames_as_the_kernel_walks_them(lib):
    """Every work item of k_deint3 over a surface and its predecessor (deint3_item: luma strips, then chroma strips) into tight NV12 frames, NV12
    surfaces with a pitch of their own and tight I420 frames, for both kept fields, one output and two."""
    rng = np.random.default_rng(0xF4B3)
    for it, (w, h) in enumerate([(16, 4), (32, 16), (48, 18), (90, 70), (176, 160), (34, 22), (2, 4), (64, 36), (100, 52), (18, 6)]):
        pitch = (w + 127) // 128 * 128 if it % 2 == 0 else w + 6
        qpitch = (w + 63) // 64 * 64 + 64 if it % 2 == 0 else w + 2
        hs, qhs = h + 16 * (it % 2), h + 8 * (it % 3)   # surface rows (the coded heights)
        src, prev = _aligned(pitch * hs * 3 // 2), _aligned(qpitch * qhs * 3 // 2)
        src[:] = rng.integers(0, 256, src.size, dtype=np.uint8)
        prev[:] = rng.integers(0, 256, prev.size, dtype=np.uint8)
        Y = src[:pitch * hs].reshape(hs, pitch)[:h, :w]
        uv = src[pitch * hs:].reshape(hs // 2, pitch)[:h // 2, :w]
        Yq = prev[:qpitch * qhs].reshape(qhs, qpitch)[:h, :w]
        uvq = prev[qpitch * qhs:].reshape(qhs // 2, qpitch)[:h // 2, :w]
        if it % 3:                                      # mostly the same picture: both branches
            Yq[:] = np.clip(Y.astype(int) + rng.integers(-12, 13, Y.shape), 0, 255)
            uvq[:] = np.clip(uv.astype(int) + rng.integers(-12, 13, uv.shape), 0, 255)
        tight, tightq = Y.tobytes() + uv.tobytes(), Yq.tobytes() + uvq.tobytes()
        for first in (0, 1):
            want_nv12 = [deint3_frame(tight, tightq, w, h, 0, p, 10) for p in (first, 1 - first)]
            for both in (True, False):
                for fmt, dp in ((0, w), (0, pitch), (1, w)):
                    dco = dp * h + (0 if dp == w else 64)
                    dst = [_aligned(dco + dp * (h // 2) + 16) for _ in range(2 if both else 1)]
                    for x in dst:
                        x[:] = 0xA5
                    lib.dei3_frame(src.ctypes.data, pitch, pitch * hs, prev.ctypes.data, qpitch, qpitch * qhs, w, h, first, 10, dst[0].ctypes.data,
                                   dst[1].ctypes.data if both else None, dp, dco, fmt)
                    for n, d in enumerate(dst):
                        c = np.frombuffer(want_nv12[n], np.uint8)[w * h:].reshape(h // 2, w // 2, 2)
                        want_i420 = want_nv12[n][:w * h] + c[:, :, 0].tobytes() + c[:, :, 1].tobytes()
                        what = (w, h, first, both, n, fmt, dp)
                        if fmt == 1:
                            assert d[:w * h * 3 // 2].tobytes() == want_i420, what
                            assert (d[w * h * 3 // 2:] == 0xA5).all(), what
                        else:
                            gy = d[:dp * h].reshape(h, dp)
                            guv = d[dco:dco + dp * (h // 2)].reshape(h // 2, dp)
                            assert gy[:, :w].tobytes() + guv[:, :w].tobytes() == want_nv12[n], what
                            assert (gy[:, w:] == 0xA5).all() and (guv[:, w:] == 0xA5).all() and (d[dp * h:dco] == 0xA5).all(), what
                            assert (d[dco + dp * (h // 2):] == 0xA5).all(), what


# ---- the same routine under the sanitizers -------------------------------------------------------------------------------------
def test_strip_routine_under_asan_and_ubsan(tmp_path):
    """tools/deint3_asan: a stand-alone program that walks deint3_item over exact-size heap buffers (sizes that are no multiple of 16, odd chroma
    row counts, pitches equal to the width) with -fsanitize=address,undefined: no access outside the planes."""
    out = tmp_path / "bin"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "deint3_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(out / "deint3_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "frames ok" in r.stdout, r.stdout
    # the blocks are guarded from their last byte on: a deliberate read one byte behind one is reported
    r = subprocess.run([str(out / "deint3_asan"), "overread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stdout and "unnoticed" not in r.stdout, r.stdout


# ---- options -------------------------------------------------------------------------------------------------------------------
def _set(h, k, v):
    return api.lib().jm_amddec_set_option(h, k.encode(), v)


def test_option_range_and_init():
    h = api.jm_nvdec_create_handle()
    try:
        assert _set(h, "parse_only", 1) == 0
        assert _set(h, "deinterlace_temporal", 2) == -1 and _set(h, "deinterlace_temporal", -1) == -1
        assert _set(h, "deinterlace_temporal", 1) == 0 and _set(h, "deinterlace_temporal", 0) == 0 and _set(h, "deinterlace_temporal", 1) == 0
        for mode in (0, 1, 2):                          # accepted whatever the mode is
            assert _set(h, "deinterlace", mode) == 0 and _set(h, "deinterlace_temporal", 1) == 0
        assert api.jm_nvdec_init(0, 1, None, 0, h) == 0
        assert _set(h, "deinterlace_temporal", 1) == -1 and _set(h, "deinterlace_temporal", 0) == -1        # fixed at init
    finally:
        api.jm_nvdec_deinit(h)


def test_mjpeg_refuses_the_option_at_init():
    h = api.jm_nvdec_create_handle()
    try:
        assert _set(h, "parse_only", 1) == 0 and _set(h, "deinterlace", 2) == 0 and _set(h, "deinterlace_temporal", 1) == 0
        assert api.jm_nvdec_init(2, 1, None, 0, h) != 0
        err = api.lib().jm_amddec_last_error(h).decode()
        assert "deinterlace_temporal" in err and "MJPEG" in err
    finally:
        api.jm_nvdec_deinit(h)
    with api.JmAmdDec(2, 1, options=dict(parse_only=1, deinterlace=2)):         # without it: as before
        pass


# ---- streams through parse-only handles ----------------------------------------------------------------------------------------
STATS = ("deint_frames", "deint_temporal_frames", "field_rate_pairs", "interlaced_sequence", "lone_fields", "frames")


def _parse(data, codec=0, **opts):
    """Decode with a parse-only handle: per output frame (display_field, display_temporal), the stats, the Deinterlace: line of the info text."""
    with api.JmAmdDec(codec, 1, options=dict(parse_only=1, **opts)) as d:
        n = len(d.decode_stream(data))
        assert d.stat("errors") == 0
        stats = {k: d.stat(k) for k in STATS}
        assert stats["frames"] == n
        per = [(d.stat(f"display_field:{i}"), d.stat(f"display_temporal:{i}")) for i in range(n)]
        assert d.stat(f"display_temporal:{n}") == -1
        info = api.jm_nvdec_show_dec_info(d.h)
        return per, stats, "".join(l for l in info.splitlines(True) if l.startswith("Deinterlace:"))      # (the rest of the text holds timings)


def _gen(kw):
    """The stream and, per display frame, the field that is first in time (the generator's listing; see test_deinterlace_gpu._gen)."""
    data = streams.generate(**kw)
    listing = streams.last_fields()
    typed0 = kw.get("poc_type", 2) == 0 or kw.get("bframes", 0) > 0
    return data, [2 if (bottom and typed0) else 1 for _, bottom in listing]


def expect(first, lone=(), starts=(0,), rate=0):
    """What a temporal handle reports per output frame -- (kept field, reads a previous frame) -- for display pictures whose first fields are `first`
    (0: not chosen for D): a picture reads its predecessor when both are chosen, neither is in `lone` and it is not in `starts` (the first display
    picture of an activation)."""
    out = []
    for k, f in enumerate(first):
        t = int(bool(f) and k > 0 and bool(first[k - 1]) and k not in lone and k - 1 not in lone and k not in starts)
        out.append((f, t))
        if rate and f and k not in lone:
            out.append((3 - f, t))
    return out


PAFF_176 = dict(width=176, height=160, frames=7, gop=7, mode=1, num_ref=2, seed=0x5CA10004, cabac=1, paff=1, bframes=2)
PROGRESSIVE = dict(width=176, height=144, frames=6, gop=6, mode=1, num_ref=2, seed=0xDE1A0001, cabac=1, t8x8=1, bframes=2)
HEVC = dict(width=90, height=70, frames=5, ctb_log2=5, mode=1, seed=0xDE1A0002)
ON = dict(deinterlace=2, deinterlace_temporal=1)


def lone_stream():
    """test_deinterlace_gpu._lone_stream: a paff=2 stream cut before the second field of its last picture, then a second stream of the same size."""
    kw = dict(width=96, height=64, frames=4, gop=4, seed=302, paff=2, num_ref=2)
    data, f1 = _gen(kw)
    first_coded = [2 if bottom else 1 for _, bottom in streams.last_fields()]
    starts = [i for i in range(len(data) - 4) if data[i:i + 4] == b"\0\0\0\1" or (data[i:i + 3] == b"\0\0\1" and data[i - 1:i] != b"\0")]
    tail, f2 = _gen(dict(kw, seed=303, paff=1))
    return data[:starts[-1]] + tail, f1[:-1] + [first_coded[-1]] + f2, {len(f1) - 1}


@pytest.mark.parametrize("rate", [0, 1])
def test_paff_every_frame_but_the_first_reads_its_predecessor(rate):
    data, first = _gen(PAFF_176)
    n = len(first)
    per, stats, info = _parse(data, deinterlace_rate=rate, **ON)
    assert per == expect(first, rate=rate)
    assert stats["frames"] == (2 if rate else 1) * n and stats["field_rate_pairs"] == (n if rate else 0)
    assert stats["deint_frames"] == stats["frames"] and stats["deint_temporal_frames"] == (2 if rate else 1) * (n - 1)
    assert "Deinterlace:\tcomb-adaptive + temporal, auto" in info


@pytest.mark.parametrize("rate", [0, 1])
def test_lone_field_and_its_successor_read_nothing(rate):
    data, first, lone = lone_stream()
    n, k = len(first), min(lone)
    per, stats, _ = _parse(data, deinterlace_rate=rate, **ON)
    want = expect(first, lone, rate=rate)
    assert per == want
    assert stats["lone_fields"] == 1 and stats["frames"] == len(want) and stats["field_rate_pairs"] == (n - 1 if rate else 0)
    assert stats["deint_temporal_frames"] == sum(t for _, t in want) == (2 if rate else 1) * (n - 3)
    one = [t for (_, t), pic in zip(expect(first, lone), range(n))]
    assert one[k] == 0 and one[k + 1] == 0 and one[k - 1] == 1 and one[k + 2] == 1           # (the IDR flush inside one activation keeps the chain)


def test_two_sequences_of_different_size_start_a_chain_each():
    a, fa = _gen(PAFF_176)
    b, fb = _gen(dict(width=96, height=64, frames=5, gop=5, seed=304, paff=1, num_ref=2))
    per, stats, _ = _parse(a + b, **ON)
    assert per == expect(fa + fb, starts=(0, len(fa)))
    assert per[len(fa)][1] == 0 and per[len(fa) + 1][1] == 1
    assert stats["deint_temporal_frames"] == len(fa) + len(fb) - 2
    # the same size twice: one activation, the second IDR's flush and its own frames carry on
    c, fc = _gen(dict(PAFF_176, seed=0x5CA10005))
    per, stats, _ = _parse(a + c, **ON)
    assert per == expect(fa + fc) and stats["deint_temporal_frames"] == len(fa) + len(fc) - 1


def test_progressive_and_hevc_only_when_asked():
    data, first = _gen(PROGRESSIVE)
    n = len(first)
    per, stats, _ = _parse(data, **ON)
    assert per == [(0, 0)] * n and stats["deint_temporal_frames"] == 0 and stats["deint_frames"] == 0
    per, stats, _ = _parse(data, deinterlace_when=1, **ON)
    assert per == expect(first) and stats["deint_temporal_frames"] == n - 1 and stats["deint_frames"] == n
    hevc = streams.generate_hevc(**HEVC)
    per, stats, _ = _parse(hevc, 1, **ON)
    assert per == [(0, 0)] * 5 and stats["deint_temporal_frames"] == 0
    per, stats, info = _parse(hevc, 1, deinterlace_when=1, **ON)
    assert per == expect([1] * 5) and stats["deint_temporal_frames"] == 4 and "comb-adaptive + temporal, always" in info
    per, stats, _ = _parse(hevc, 1, deinterlace_when=1, deinterlace_rate=1, deinterlace_field=2, **ON)
    assert per == expect([2] * 5, rate=1) and stats["deint_temporal_frames"] == 8 and stats["frames"] == 10


@pytest.mark.parametrize("mode", [0, 1])
def test_no_effect_without_mode_2(mode):
    data, first = _gen(PAFF_176)
    base = _parse(data, deinterlace=mode)
    per, stats, info = _parse(data, deinterlace=mode, deinterlace_temporal=1)
    assert (per, stats, info) == base
    assert all(t == 0 for _, t in per) and stats["deint_temporal_frames"] == 0 and "temporal" not in info


def test_off_is_a_handle_without_the_key():
    data, first, _ = lone_stream()
    for opts in (dict(deinterlace=2), dict(deinterlace=2, deinterlace_rate=1), {}):
        assert _parse(data, deinterlace_temporal=0, **opts) == _parse(data, **opts)
    per, stats, info = _parse(data, deinterlace=2, deinterlace_temporal=0)
    assert all(t == 0 for _, t in per) and stats["deint_temporal_frames"] == 0 and "temporal" not in info
