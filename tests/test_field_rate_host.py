"""Field-rate deinterlaced output (option deinterlace_rate), host side (no GPU): the fused strip routine of k_deint2
(jmcodec_amd/csrc/deint2_packed.h, host build) against the numpy restatement of D (deint_ref.py) for BOTH parities of the same plane, the option's
range, and what parse-only handles count and report per output frame against the stream generator's own listing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from deint_ref import deint_frame, deint_plane
from jmcodec_amd import api
from tools import streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libdeint2_packed_check.so")
    src = os.path.join(ROOT, "tests", "native", "deint2_packed_check.cpp")
    hdrs = [os.path.join(ROOT, "jmcodec_amd", "csrc", h) for h in ("deint2_packed.h", "deint_packed.h", "mc_packed.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so, src])
    l = C.CDLL(so)
    l.dei2_plane.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4 + [C.c_int] * 2
    l.dei2_plane.restype = None
    l.dei2_frame.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 2 + [C.c_int] * 3
    l.dei2_frame.restype = None
    return l


def _aligned(n, misalign=0):
    """n bytes whose first one lies `misalign` bytes behind a 16-byte boundary (a view; the base array stays alive through it)."""
    raw = np.zeros(n + 32, np.uint8)
    off = (-raw.ctypes.data) % 16 + misalign
    return raw[off:off + n]


def _run(lib, P, step, mode, T, pitch=None, dst_pitch=None, misalign=0, split=False):
    """The fused strip routine over a whole plane P (H x W bytes; step 2: interleaved chroma).  Returns the two planes [top kept, bottom kept]
    (split: the two pairs of planes)."""
    H, W = P.shape
    pitch = pitch or W
    src = _aligned(H * pitch, misalign)
    src[:] = 0x5A
    src.reshape(H, pitch)[:, :W] = P
    if split:
        d = [_aligned(H * (W // 2)) for _ in range(4)]
        lib.dei2_plane(src.ctypes.data, pitch, W, H, step, mode, T, d[0].ctypes.data, d[1].ctypes.data, d[2].ctypes.data, d[3].ctypes.data, W // 2, 1)
        return [x.reshape(H, W // 2).copy() for x in d]
    dp = dst_pitch or W
    dst = [_aligned(H * dp), _aligned(H * dp)]
    for x in dst:
        x[:] = 0xA5
    lib.dei2_plane(src.ctypes.data, pitch, W, H, step, mode, T, dst[0].ctypes.data, None, dst[1].ctypes.data, None, dp, 0)
    outs = [x.reshape(H, dp) for x in dst]
    for o in outs:
        assert (o[:, W:] == 0xA5).all()                 # nothing is written beyond the W bytes of a row
    return [o[:, :W].copy() for o in outs]


def _ref(P, step, mode, p, T):
    if step == 1:
        return deint_plane(P, mode, p, T)
    out = np.empty_like(P)
    out[:, 0::2] = deint_plane(P[:, 0::2], mode, p, T)
    out[:, 1::2] = deint_plane(P[:, 1::2], mode, p, T)
    return out


# ---- deint2_packed.h against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2])
def test_fused_strips_against_the_restatement_random(lib, step):
    """Seeded random planes: every W mod 16 (W even), H from 2 up (no multiples of 8 among them), aligned and unaligned pitches and bases, noise,
    near-flat noise (both branches of mode 2) and rows alternating 0 / 255; both modes, thresholds 1, 10, 255 and random ones; NV12-style and
    split destinations.  Both outputs of one walk are compared, each with D of its own parity."""
    assert lib.dei2_strip_rows() == 8
    rng = np.random.default_rng(0xF1E1D + step)
    seen_w, seen_h, woven = set(), set(), [0, 0]
    for it in range(260):
        H = int(rng.integers(2, 45)) if it >= 24 else 2 + it
        W = 2 * int(rng.integers(1, 60)) if it >= 24 else 2 * (it % 8 + 1) + 16 * (it // 8)
        seen_w.add(W % 16)
        seen_h.add(H % 8)
        kind = it % 4
        P = rng.integers(0, 256, (H, W), dtype=np.uint8)
        if kind == 1:
            P = (100 + rng.integers(0, 9, (H, W))).astype(np.uint8)
        if kind == 2:
            P[0::2], P[1::2] = 0, 255
        T = [10, 1, 255, int(rng.integers(1, 256))][it % 4] if it % 3 else 10
        pitch = (W + 15) // 16 * 16 + 16 * int(rng.integers(0, 3)) if it % 2 else W + 2 * int(rng.integers(0, 5))
        dp = (W + 15) // 16 * 16 if it % 2 else W
        for mode in (1, 2):
            want = [_ref(P, step, mode, p, T) for p in (0, 1)]
            got = _run(lib, P, step, mode, T, pitch, dp, misalign=0 if it % 5 else 1)
            for p in (0, 1):
                assert np.array_equal(got[p], want[p]), (it, H, W, mode, p, T, pitch)
                if mode == 2:
                    woven[int(np.array_equal(want[p][(1 - p)::2], P[(1 - p)::2]))] += 1
            if step == 2:
                u0, v0, u1, v1 = _run(lib, P, step, mode, T, pitch, split=True)
                assert np.array_equal(u0, want[0][:, 0::2]) and np.array_equal(v0, want[0][:, 1::2]), (it, "split top")
                assert np.array_equal(u1, want[1][:, 0::2]) and np.array_equal(v1, want[1][:, 1::2]), (it, "split bottom")
    assert seen_w == set(range(0, 16, 2)) and seen_h == set(range(8))
    assert woven[0] and woven[1]                        # planes where something was interpolated, and planes left woven


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("T", [1, 10, 15, 255])
def test_fused_threshold_edge(lib, step, T):
    """M exactly 4 T^2 stays woven, above it is interpolated -- on a missing row of EACH output (rows 1 and 2 of a 4-row plane).  With s = a * a in
    every column (up = dn = cur + a), M = 4 a^2: a = T is the boundary itself, a = T + 1 lies above it (T = 255: a cannot exceed it, only the
    boundary is checked)."""
    Wc, b = 40, 0
    for a, combed in ((T, False), (T + 1, True)):
        if b + a > 255:
            continue
        plane = np.full((4, Wc), b + a, np.int64)
        for row, p in ((1, 0), (2, 1)):                 # the missing row of the output that keeps parity p
            Q = plane.copy()
            Q[row] = b
            P = Q.astype(np.uint8) if step == 1 else np.repeat(Q.astype(np.uint8), 2, axis=1)
            want = _ref(P, step, 2, p, T)
            assert ((want[row] != b).all() if combed else (want[row] == b).all()), (a, row)
            for pitch in (None, (P.shape[1] + 15) // 16 * 16):
                got = _run(lib, P, step, 2, T, pitch)
                assert np.array_equal(got[p], want), (T, a, row, pitch)
                assert np.array_equal(got[1 - p], _ref(P, step, 2, 1 - p, T)), (T, a, row, pitch, "other")


@pytest.mark.parametrize("step", [1, 2])
def test_fused_plane_edges_and_chunk_edges(lib, step):
    """A combed column at every position of a row in turn -- the plane's first and last columns and both sides of every 16-byte chunk edge -- on
    planes whose first / last rows are missing rows of one output or the other (up / dn mirror)."""
    for Wc in (1, 2, 8, 15, 16, 17, 31, 32, 33):
        W = Wc * step
        if W & 1:
            continue
        for H in (2, 3, 8, 9, 17):
            for col in range(W):
                P = np.full((H, W), 90, np.uint8)
                P[1::2, col] = 140
                P[0::2, col] = 60
                got = _run(lib, P, step, 2, 10, pitch=(W + 15) // 16 * 16)
                for p in (0, 1):
                    assert np.array_equal(got[p], _ref(P, step, 2, p, 10)), (Wc, H, col, p)


def test_whole_frame_pairs_as_the_kernel_walks_them(lib):
    """Every work item of k_deint2 over a surface (deint2_item: luma strips, then chroma strips) into two tight NV12 frames, two NV12 surfaces with
    a pitch of their own and two tight I420 frames, for both first fields: the first destination is D with the first field kept."""
    rng = np.random.default_rng(0xF4B)
    for it, (w, h) in enumerate([(16, 4), (32, 16), (48, 18), (90, 70), (176, 160), (34, 22), (2, 4), (64, 36), (100, 52), (128, 64)]):
        pitch = (w + 127) // 128 * 128 if it % 2 == 0 else w + 6
        hs = h + 16 * (it % 2)                          # surface rows (the coded height)
        src = _aligned(pitch * hs * 3 // 2)
        src[:] = (110 + rng.integers(0, 12, src.size)).astype(np.uint8) if it % 3 else rng.integers(0, 256, src.size, dtype=np.uint8)
        Y = src[:pitch * hs].reshape(hs, pitch)[:h, :w]
        uv = src[pitch * hs:].reshape(hs // 2, pitch)[:h // 2, :w]
        tight_nv12 = Y.tobytes() + uv.tobytes()
        for mode in (1, 2):
            for first in (0, 1):
                for fmt, dp in ((0, w), (0, pitch), (1, w)):
                    dco = dp * h + (0 if dp == w else 64)
                    dst = [_aligned(dco + dp * (h // 2) + 16) for _ in range(2)]
                    for x in dst:
                        x[:] = 0xA5
                    lib.dei2_frame(src.ctypes.data, pitch, pitch * hs, w, h, mode, first, 10, dst[0].ctypes.data, dst[1].ctypes.data, dp, dco, fmt)
                    for n, p in enumerate((first, 1 - first)):
                        want_nv12 = deint_frame(tight_nv12, w, h, 0, mode, p, 10)
                        c = np.frombuffer(want_nv12, np.uint8)[w * h:].reshape(h // 2, w // 2, 2)
                        want_i420 = want_nv12[:w * h] + c[:, :, 0].tobytes() + c[:, :, 1].tobytes()
                        what, d = (w, h, mode, first, n, fmt, dp), dst[n]
                        if fmt == 1:
                            assert d[:w * h * 3 // 2].tobytes() == want_i420, what
                            assert (d[w * h * 3 // 2:] == 0xA5).all(), what
                        else:
                            gy = d[:dp * h].reshape(h, dp)
                            guv = d[dco:dco + dp * (h // 2)].reshape(h // 2, dp)
                            assert gy[:, :w].tobytes() + guv[:, :w].tobytes() == want_nv12, what
                            assert (gy[:, w:] == 0xA5).all() and (guv[:, w:] == 0xA5).all() and (d[dp * h:dco] == 0xA5).all(), what
                            assert (d[dco + dp * (h // 2):] == 0xA5).all(), what


# ---- options -------------------------------------------------------------------------------------------------------------------
def _set(h, k, v):
    return api.lib().jm_amddec_set_option(h, k.encode(), v)


def test_option_range_and_init():
    h = api.jm_nvdec_create_handle()
    try:
        assert _set(h, "parse_only", 1) == 0
        assert _set(h, "deinterlace_rate", 2) == -1 and _set(h, "deinterlace_rate", -1) == -1
        assert _set(h, "deinterlace_rate", 1) == 0 and _set(h, "deinterlace_rate", 0) == 0 and _set(h, "deinterlace_rate", 1) == 0
        assert api.jm_nvdec_init(0, 1, None, 0, h) == 0
        assert _set(h, "deinterlace_rate", 1) == -1 and _set(h, "deinterlace_rate", 0) == -1        # fixed at init
    finally:
        api.jm_nvdec_deinit(h)


# ---- streams through parse-only handles ----------------------------------------------------------------------------------------
STATS = ("deint_frames", "field_rate_pairs", "interlaced_sequence", "lone_fields", "frames", "fps_num", "fps_den", "out_fps_num", "out_fps_den")


def _parse(data, codec=0, **opts):
    """Decode with a parse-only handle: per output frame (display_field, display_picture), the stats, the display pictures' order counts, the info."""
    with api.JmAmdDec(codec, 1, options=dict(parse_only=1, **opts)) as d:
        n = len(d.decode_stream(data))
        assert d.stat("errors") == 0
        stats = {k: d.stat(k) for k in STATS}
        assert stats["frames"] == n
        per = [(d.stat(f"display_field:{i}"), d.stat(f"display_picture:{i}")) for i in range(n)]
        assert d.stat(f"display_field:{n}") == -1 and d.stat(f"display_picture:{n}") == -1
        pocs = []
        while len(pocs) < (per[-1][1] + 1 if per else 0):
            pocs.append(d.stat(f"display_poc:{len(pocs)}"))
        assert d.stat(f"display_poc:{len(pocs)}") == -1                                 # (one entry per display picture, no more)
        return per, stats, pocs, api.jm_nvdec_show_dec_info(d.h)


def _gen(kw):
    """The stream and, per display frame, the field that is first in time (the generator's listing; see test_deinterlace_gpu._gen)."""
    data = streams.generate(**kw)
    listing = streams.last_fields()
    typed0 = kw.get("poc_type", 2) == 0 or kw.get("bframes", 0) > 0
    return data, [2 if (bottom and typed0) else 1 for _, bottom in listing]


def _pairs(first, lone=()):
    """What a field-rate handle reports per output frame for display pictures whose first fields are `first` (0: not deinterlaced)."""
    out = []
    for k, f in enumerate(first):
        out.append((f, k))
        if f and k not in lone:
            out.append((3 - f, k))
    return out


PAFF_176 = dict(width=176, height=160, frames=7, gop=7, mode=1, num_ref=2, seed=0x5CA10004, cabac=1, paff=1, bframes=2)
PROGRESSIVE = dict(width=176, height=144, frames=6, gop=6, mode=1, num_ref=2, seed=0xDE1A0001, cabac=1, t8x8=1, bframes=2)
HEVC = dict(width=90, height=70, frames=5, ctb_log2=5, mode=1, seed=0xDE1A0002)


@pytest.mark.parametrize("mode", [1, 2])
def test_paff_pairs_follow_the_generators_listing(mode):
    data, first = _gen(PAFF_176)
    n = len(first)
    assert 1 in first and 2 in first
    base, bstats, bpocs, _ = _parse(data, deinterlace=mode)
    per, stats, pocs, info = _parse(data, deinterlace=mode, deinterlace_rate=1)
    assert stats["lone_fields"] == 0 and stats["frames"] == 2 * n - 0
    assert stats["field_rate_pairs"] == n and stats["deint_frames"] == 2 * n
    assert per == _pairs(first)
    assert pocs == bpocs and len(pocs) == n             # display_poc stays per display picture
    assert f", field rate, {2 * n} frames" in info and ("bob" if mode == 1 else "comb-adaptive") in info
    for f in (1, 2):                                    # deinterlace_field names the field that comes first
        per, stats, _, _ = _parse(data, deinterlace=mode, deinterlace_rate=1, deinterlace_field=f)
        assert per == _pairs([f] * n) and stats["field_rate_pairs"] == n


def _lone_stream():
    """A paff=2 stream cut before the second field of its last picture, then a second stream (the stream of the deinterlace tests)."""
    kw = dict(width=96, height=64, frames=4, gop=4, seed=302, paff=2, num_ref=2)
    data, f1 = _gen(kw)
    first_coded = [2 if bottom else 1 for _, bottom in streams.last_fields()]
    starts = [i for i in range(len(data) - 4) if data[i:i + 4] == b"\0\0\0\1" or (data[i:i + 3] == b"\0\0\1" and data[i - 1:i] != b"\0")]
    tail, f2 = _gen(dict(kw, seed=303, paff=1))
    return data[:starts[-1]] + tail, f1[:-1] + [first_coded[-1]] + f2, {len(f1) - 1}


def test_lone_field_gives_one_frame_with_its_own_field():
    data, first, lone = _lone_stream()
    n = len(first)
    per, stats, _, _ = _parse(data, deinterlace=2, deinterlace_rate=1)
    assert stats["lone_fields"] == 1
    assert stats["frames"] == 2 * n - 1 and stats["field_rate_pairs"] == n - 1 and stats["deint_frames"] == 2 * n - 1
    assert per == _pairs(first, lone)
    k = min(lone)
    other = 3 - first[k]
    per, _, _, _ = _parse(data, deinterlace=2, deinterlace_rate=1, deinterlace_field=other)
    assert per == _pairs([first[k] if i == k else other for i in range(n)], lone)


def test_progressive_and_hevc_pair_only_when_asked():
    data, first = _gen(PROGRESSIVE)
    n = len(first)
    per, stats, _, _ = _parse(data, deinterlace=2, deinterlace_rate=1)
    assert per == [(0, k) for k in range(n)] and stats["field_rate_pairs"] == 0 and stats["frames"] == n and stats["deint_frames"] == 0
    per, stats, _, _ = _parse(data, deinterlace=2, deinterlace_rate=1, deinterlace_when=1)
    assert per == _pairs(first) and stats["field_rate_pairs"] == n and stats["frames"] == 2 * n
    hevc = streams.generate_hevc(**HEVC)
    per, stats, _, _ = _parse(hevc, 1, deinterlace=1, deinterlace_rate=1)
    assert per == [(0, k) for k in range(5)] and stats["field_rate_pairs"] == 0 and stats["frames"] == 5
    per, stats, _, _ = _parse(hevc, 1, deinterlace=1, deinterlace_rate=1, deinterlace_when=1, deinterlace_field=2)
    assert per == _pairs([2] * 5) and stats["field_rate_pairs"] == 5 and stats["frames"] == 10 and stats["deint_frames"] == 10


def test_interlaced_then_progressive_only_the_first_gives_pairs():
    a, fa = _gen(dict(PAFF_176, frames=6, gop=6))
    b, fb = _gen(dict(width=176, height=160, frames=5, gop=5, mode=1, num_ref=2, seed=0xDE1A0003, cabac=1, bframes=2))
    per, stats, _, _ = _parse(a + b, deinterlace=2, deinterlace_rate=1)
    assert per == _pairs(fa + [0] * len(fb))
    assert stats["field_rate_pairs"] == len(fa) and stats["frames"] == 2 * len(fa) + len(fb) and stats["interlaced_sequence"] == 0


@pytest.mark.parametrize("opts", [dict(deinterlace=2, deinterlace_rate=0), dict(deinterlace=0, deinterlace_rate=1), dict(deinterlace=1)])
def test_rate_off_or_no_deinterlacing_counts_as_before(opts):
    data, first = _gen(PAFF_176)
    n = len(first)
    per, stats, pocs, info = _parse(data, **opts)
    on = opts["deinterlace"] != 0
    assert per == [(f if on else 0, k) for k, f in enumerate(first)]                # display_picture is the identity
    assert stats["frames"] == n and stats["field_rate_pairs"] == 0 and stats["deint_frames"] == (n if on else 0)
    assert len(pocs) == n and "field rate" not in info
    assert (stats["out_fps_num"], stats["out_fps_den"]) == (stats["fps_num"], stats["fps_den"])


# ---- frame rate ----------------------------------------------------------------------------------------------------------------
def test_out_fps_doubles_only_at_field_rate_on_a_deinterlaced_sequence():
    kw = dict(width=96, height=64, frames=4, gop=4, seed=302, num_ref=2, vui_fps=25)
    inter, prog = streams.generate(paff=1, **kw), streams.generate(**kw)
    for data, opts, factor in ((inter, dict(deinterlace=2, deinterlace_rate=1), 2), (inter, dict(deinterlace=2), 1), (inter, dict(deinterlace_rate=1), 1),
                               (inter, {}, 1), (prog, dict(deinterlace=2, deinterlace_rate=1), 1),
                               (prog, dict(deinterlace=1, deinterlace_rate=1, deinterlace_when=1), 2)):
        _, st, _, _ = _parse(data, **opts)
        assert st["fps_num"] > 0 and st["fps_den"] > 0 and st["fps_num"] / st["fps_den"] == 25.0, opts
        assert (st["out_fps_num"], st["out_fps_den"]) == (factor * st["fps_num"], st["fps_den"]), opts
    hevc = streams.generate_hevc(width=128, height=96, frames=4, vui_fps=30)
    _, st, _, _ = _parse(hevc, 1, deinterlace=2, deinterlace_rate=1)
    assert (st["out_fps_num"], st["out_fps_den"]) == (st["fps_num"], st["fps_den"]) and st["fps_num"] > 0
    _, st, _, _ = _parse(hevc, 1, deinterlace=2, deinterlace_rate=1, deinterlace_when=1)
    assert (st["out_fps_num"], st["out_fps_den"]) == (2 * st["fps_num"], st["fps_den"])
