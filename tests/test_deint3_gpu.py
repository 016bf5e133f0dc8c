"""Motion-adaptive deinterlaced output on the device (option deinterlace_temporal, k_deint3), bit for bit against the numpy restatement of D3
(deint3_ref.py, written from INTEGRATION.md "Deinterlaced output") applied to the CPU oracle's consecutive frames, with today's mode 2 for the frames
that have no previous one: the stand-alone call, both codecs end to end, field rate, a lone field, in front of the resampler and of the colour
conversion, device-resident frames, every fetch route, and however the pictures were batched."""
import ctypes as C
import functools
import random
import threading

import numpy as np
import pytest

from deint_ref import deint_frame
from deint3_ref import deint3_frame, deint3_plane, moving_share
from jmcodec_amd import api
from test_deint3_host import HEVC, PAFF_176, PROGRESSIVE, _gen, expect, lone_stream
from test_rgb_output_host import rgb_frame
from test_scaled_output_host import scale_frame
from tools import streams

pytestmark = pytest.mark.gpu

T = 10          # the default threshold
PAFF2 = dict(width=96, height=64, frames=8, gop=4, seed=302, paff=2, num_ref=2, bframes=1)
RAN = {"temporal_frames": 0}        # deint_temporal_frames of the handles of this module (the closing test)


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


# ---- the stand-alone call --------------------------------------------------------------------------------------------------------
def _pair(rng, W, H, pitch, qpitch, kind, t):
    """Two pitch-linear NV12 surfaces (the frame, the previous frame): 0 noise against noise, 1 an identical pair, 2 a smooth picture with a
    displaced rectangle, 3 differences of exactly T and T + 1 (and 0, T - 1) all over."""
    R = H * 3 // 2
    if kind == 0:
        P, Q = rng.integers(0, 256, (R, W), dtype=np.uint8), rng.integers(0, 256, (R, W), dtype=np.uint8)
    elif kind == 1:
        P = rng.integers(0, 256, (R, W), dtype=np.uint8)
        Q = P.copy()
    elif kind == 2:
        y, x = np.mgrid[0:R, 0:W]
        Q = np.clip(96 + 60 * np.sin(x / 9.0) + 40 * np.cos(y / 7.0) + (y & 1) * 30, 0, 255).astype(np.uint8)
        P = Q.copy()
        for y0, y1 in ((H // 5, H // 5 + max(2, H // 3)), (H + H // 8, H + H // 8 + max(1, H // 6))):      # in the luma and in the chroma rows
            P[y0:y1, W // 4:W // 4 + max(2, W // 3)] = np.roll(Q[y0:y1, W // 4:W // 4 + max(2, W // 3)], 1, axis=0) ^ 0x40
    else:
        P = rng.integers(0, 256, (R, W)).astype(np.int64)
        d = rng.choice([0, 0, 0, 0, t - 1, t, t, t + 1], (R, W)) * rng.choice([-1, 1], (R, W))
        Q = np.where((P + d < 0) | (P + d > 255), P - d, P + d)
        P, Q = P.astype(np.uint8), np.clip(Q, 0, 255).astype(np.uint8)
    src, prev = np.full((R, pitch), 0x5A, np.uint8), np.full((R, qpitch), 0x3C, np.uint8)
    src[:, :W], prev[:, :W] = P, Q
    return src.reshape(-1), prev.reshape(-1)


def _planes(buf, W, H, pitch):
    Y = buf[:pitch * H].reshape(H, pitch)[:, :W]
    uv = buf[pitch * H:].reshape(H // 2, pitch)[:, :W]
    return Y, uv[:, 0::2], uv[:, 1::2]


def test_deinterlace3_device_random_cases():
    """jm_amddec_deinterlace3_device alone: 80 seeded sizes between 2 x 4 and 400 x 300 (no multiples of 16, odd chroma row counts), the small
    sizes at which the strip routine changes path and one 1920 x 1080; pitches of the frame, the previous frame and the destination that differ;
    four kinds of content; T 1, 10, 255; one output and two -- against D3 of the surfaces' planes, padding bytes untouched; then the refusals."""
    hip = _hip()
    rng = random.Random(0xD3D3D3)
    cap = 2048 * 1088 * 3 // 2
    d_src, d_prev, d_a, d_b = (C.c_void_p() for _ in range(4))
    for p in (d_src, d_prev, d_a, d_b):
        assert hip.hipMalloc(C.byref(p), cap) == 0
    shares = {"luma": [], "chroma": []}
    try:
        cases = [(rng.randrange(2, 400, 2), rng.randrange(4, 300, 2)) for _ in range(80)] + [(16, 4), (2, 4), (18, 6), (130, 70), (1920, 1080)]
        for n, (W, H) in enumerate(cases):
            big = W * H > 400 * 300
            pitch = W + rng.choice([0, 2, 14, 128 - W % 128])
            qpitch = W + rng.choice([0, 6, 128 - W % 128, 256 - W % 128])
            dp = W + rng.choice([0, 0, 6, 16, 128 - W % 128])
            if n % 2 or big:                            # 16-byte rows everywhere: the 16-byte path, with three different pitches
                pitch, qpitch, dp = (W + 15) // 16 * 16 + 16 * (n % 3), (W + 15) // 16 * 16 + 16 * ((n + 1) % 3), (W + 15) // 16 * 16 + 16 * ((n + 2) % 3)
            dco = dp * H + rng.choice([0, 16, 256])
            first, both = 1 + (n // 2) % 2, n % 3 != 0
            thr = (1, 10, 255)[n % 3] if not big else 10
            src, prev = _pair(np.random.default_rng(n), W, H, pitch, qpitch, 2 if big else n % 4, thr)
            out_n = dco + dp * (H // 2)
            assert max(src.size, prev.size, out_n) <= cap
            assert hip.hipMemcpy(d_src, src.ctypes.data_as(C.c_void_p), src.size, 1) == 0
            assert hip.hipMemcpy(d_prev, prev.ctypes.data_as(C.c_void_p), prev.size, 1) == 0
            assert hip.hipMemset(d_a, 0xA5, out_n) == 0 and hip.hipMemset(d_b, 0xA5, out_n) == 0
            rc = api.deinterlace3_device(d_src, pitch, pitch * H, d_prev, qpitch, qpitch * H, W, H, first, d_a, d_b if both else None, dst_pitch=dp,
                                         dst_chroma_offset=dco, threshold=thr)
            assert rc == 0, (n, W, H, rc)
            Pp, Qp = _planes(src, W, H, pitch), _planes(prev, W, H, qpitch)
            for which, (d_dst, keep) in enumerate(((d_a, first), (d_b, 3 - first))):
                out = np.zeros(out_n, np.uint8)
                assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d_dst, out_n, 2) == 0
                what = f"case {n}: {W}x{H} pitches {pitch} {qpitch} -> {dp} first {first} both {both} output {which} T {thr}"
                if which and not both:
                    assert (out == 0xA5).all(), what + " (no second output)"
                    continue
                want = [deint3_plane(Pp[k], Qp[k], keep - 1, thr, shares["chroma" if k else "luma"] if n % 4 in (2, 3) else None) for k in range(3)]
                gy = out[:dp * H].reshape(H, dp)
                guv = out[dco:dco + dp * (H // 2)].reshape(H // 2, dp)
                assert np.array_equal(gy[:, :W], want[0]), what + " (luma)"
                assert np.array_equal(guv[:, 0:W:2], want[1]) and np.array_equal(guv[:, 1:W:2], want[2]), what + " (chroma)"
                assert (gy[:, W:] == 0xA5).all() and (guv[:, W:] == 0xA5).all() and (out[dp * H:dco] == 0xA5).all(), what + " (padding)"
        # both branches ran in the cases built for it
        assert 0.05 <= moving_share(shares["luma"]) <= 0.95 and 0.01 <= moving_share(shares["chroma"]) <= 0.99
        # invalid arguments are refused before anything runs: those of jm_amddec_deinterlace2_device ...
        f = api.deinterlace3_device
        g = lambda **kw: f(**dict(dict(src=d_src, pitch=128, chroma_offset=128 * 64, prev=d_prev, prev_pitch=128, prev_chroma_offset=128 * 64, width=100,
                                       height=64, first_field=1, dst_first=d_a, dst_second=d_b), **kw))
        fs = 100 * 64 * 3 // 2
        assert g() == 0 and g(dst_second=None) == 0
        assert g(height=63) == -1 and g(width=99) == -1 and g(height=2, chroma_offset=256, prev_chroma_offset=256) == -1
        assert g(first_field=0) == -1 and g(first_field=3) == -1 and g(threshold=256) == -1 and g(threshold=-1) == -1
        assert g(pitch=64) == -1 and g(prev_pitch=64) == -1 and g(dst_pitch=98) == -1 and g(dst_first=None) == -1 and g(src=None) == -1
        assert g(dst_second=d_a) == -1 and g(dst_second=C.c_void_p(d_a.value + fs - 1)) == -1 and g(dst_second=C.c_void_p(d_a.value + fs)) == 0
        assert g(dst_first=d_src) == -1 and g(dst_second=C.c_void_p(d_src.value + 128 * 96 - 29)) == -1
        # ... no previous frame, and a destination over it
        assert g(prev=None) == -1
        assert g(dst_first=d_prev) == -1 and g(dst_second=d_prev) == -1 and g(dst_first=C.c_void_p(d_prev.value + 128 * 96 - 29), dst_second=None) == -1
        assert g(dst_first=C.c_void_p(d_prev.value + 128 * 96 - 28), dst_second=None) == 0                      # right behind its last byte is fine
    finally:
        for p in (d_src, d_prev, d_a, d_b):
            hip.hipFree(p)


# ---- through the decoder --------------------------------------------------------------------------------------------------------
STATS = ("deint_frames", "deint_temporal_frames", "field_rate_pairs", "lone_fields", "scaled_frames", "rgb_frames", "frames")
ON = dict(deinterlace=2, deinterlace_temporal=1)


def _decode(data, codec=0, fmt=1, rgb=None, chunks=None, knobs=(), **opts):
    """knobs: engine options (they belong to the device's engine, not to the handle: set after init and put back to 0 = default)."""
    with api.JmAmdDec(codec, fmt, options=opts, rgb=rgb) as d:
        try:
            for k, v in knobs:
                assert api.lib().jm_amddec_set_option(d.h, k.encode(), v) == 0
            frames = d.decode_stream(data, chunks=chunks)
        finally:
            for k, _ in knobs:
                api.lib().jm_amddec_set_option(d.h, k.encode(), 0)
        assert d.stat("errors") == 0, api.lib().jm_amddec_last_error(d.h)
        stats = {k: d.stat(k) for k in STATS}
        stats["per"] = [(d.stat(f"display_field:{i}"), d.stat(f"display_temporal:{i}")) for i in range(len(frames))]
        RAN["temporal_frames"] += stats["deint_temporal_frames"]
        return frames, stats


@functools.lru_cache(maxsize=None)
def _stream(name):
    """(data, codec, first field per display picture, lone pictures, the options that choose its frames for D)."""
    if name == "lone":
        data, fields, lone = lone_stream()
        return data, 0, tuple(fields), frozenset(lone), ()
    if name == "hevc":
        return streams.generate_hevc(**HEVC), 1, (1,) * HEVC["frames"], frozenset(), (("deinterlace_when", 1),)
    kw, when = {"paff_176": (PAFF_176, 0), "paff2": (PAFF2, 0), "progressive": (PROGRESSIVE, 1)}[name]
    data, fields = _gen(kw)
    return data, 0, tuple(fields), frozenset(), (("deinterlace_when", 1),) if when else ()


@functools.lru_cache(maxsize=None)
def _oracle_frames(name, fmt):
    data, codec = _stream(name)[:2]
    blob, n, W, H = (streams.OracleHevc() if codec else streams.Oracle()).decode(data, fmt)
    fs = W * H * 3 // 2
    return tuple(blob[i * fs:(i + 1) * fs] for i in range(n)), W, H


@functools.lru_cache(maxsize=None)
def _want(name, fmt, thr=T, rate=0, live=False):
    """What a temporal handle hands out for the stream: D3 of the oracle's consecutive frames where a previous frame exists (test_deint3_host.expect),
    today's mode 2 where not, bob for a lone field.  Returns (frames, (display_field, display_temporal) per frame).  live: assert, before anything
    is compared, that both branches of D3 live on these frames -- moving share of luma in [0.05, 0.95], of chroma in [0.01, 0.99]."""
    _, _, fields, lone, _ = _stream(name)
    F, W, H = _oracle_frames(name, fmt)
    assert len(F) == len(fields)
    per = expect(list(fields), lone, rate=rate)
    st = {"luma": [], "chroma": []}
    out, k = [], 0
    for i, f in enumerate(fields):
        for _ in range(2 if rate and f and i not in lone else 1):
            keep, temporal = per[k]
            k += 1
            if not keep:
                out.append(F[i])
            elif i in lone:
                out.append(deint_frame(F[i], W, H, fmt, 1, keep - 1))
            elif temporal:
                out.append(deint3_frame(F[i], F[i - 1], W, H, fmt, keep - 1, thr, st))
            else:
                out.append(deint_frame(F[i], W, H, fmt, 2, keep - 1, thr))
    assert k == len(per)
    if live:
        l, c = moving_share(st["luma"]), moving_share(st["chroma"])
        assert 0.05 <= l <= 0.95 and 0.01 <= c <= 0.99, (name, thr, l, c)
    return tuple(out), per


def _check(name, fmt=1, thr=T, rate=0, live=False, chunks=None, knobs=(), **more):
    data, codec, fields, lone, sel = _stream(name)
    want, per = _want(name, fmt, thr, rate, live)
    opts = dict(ON, **dict(sel), **more)
    if thr != T:
        opts["deinterlace_threshold"] = thr
    if rate:
        opts["deinterlace_rate"] = 1
    frames, stats = _decode(data, codec, fmt, chunks=chunks, knobs=knobs, **opts)
    assert len(frames) == len(want) and stats["per"] == per
    for i, f in enumerate(frames):
        assert f == want[i], f"{name}: frame {i} of {len(want)} differs (fmt {fmt}, T {thr}, rate {rate}, {per[i]})"
    assert stats["deint_temporal_frames"] == sum(t for _, t in per) > 0
    return frames, stats


@pytest.mark.parametrize("fmt", [1, 0])
def test_paff_frames_and_field_pairs(fmt):
    """PAFF_176 at T = 10 (measured with the top field kept: 0.72 of the missing luma samples move, 0.12 of the chroma ones)."""
    _check("paff_176", fmt, live=True)


def test_paff_every_picture_two_fields_threshold_5():
    """PAFF2 at T = 5 (0.88 / 0.044; at T = 10 its chroma share is 0.002, which is why it runs at 5)."""
    _check("paff2", 1, thr=5, live=True)


def test_progressive_when_asked():
    """PROGRESSIVE with deinterlace_when = 1 (0.57 / 0.064)."""
    _check("progressive", 1, live=True)


def test_hevc_when_asked():
    """The HEVC stream with deinterlace_when = 1 (0.82 / 0.75)."""
    _check("hevc", 1, live=True)
    _check("hevc", 0)


def test_field_rate_both_frames_of_a_pair_read_the_same_previous_frame():
    """deinterlace_rate = 1: D3 with f kept, then D3 with f' kept, both of (F_n, F_n-1) -- the frames interleaved first / second."""
    frames, stats = _check("paff_176", 1, rate=1)
    n = len(_stream("paff_176")[2])
    assert stats["field_rate_pairs"] == n and stats["frames"] == 2 * n and stats["deint_temporal_frames"] == 2 * (n - 1)
    _check("paff_176", 0, rate=1)


@pytest.mark.parametrize("rate", [0, 1])
def test_lone_field_stays_bob_and_breaks_the_chain(rate):
    frames, stats = _check("lone", 1, rate=rate)
    assert stats["lone_fields"] == 1


def test_scaled_and_rgb_behind_d3():
    """R_G(D3(F)) with the crop / target of test_downscaled_after_deinterlacing, and C(D3(F)) for one RGB spec: k_deint3 writes into the batch's
    scratch and the pack kernel reads it."""
    data, codec, fields, _, _ = _stream("paff_176")
    _, W, H = _oracle_frames("paff_176", 1)
    base, per = _want("paff_176", 1)
    crop, target = (8, 6, 160, 148), (100, 70)
    frames, stats = _decode(data, 0, 1, crop_x=8, crop_y=6, crop_w=160, crop_h=148, target_width=100, target_height=70, **ON)
    assert frames == [scale_frame(f, W, H, 1, crop, target) for f in base]
    assert stats["per"] == per and stats["scaled_frames"] == len(base) and stats["deint_temporal_frames"] == len(base) - 1
    rgb = api.rgb_spec("u8", planar=True)
    frames, stats = _decode(data, 0, 1, rgb=rgb, **ON)
    assert frames == [rgb_frame(f, W, H, 1, (0, 0, W, H), (W, H), rgb, 6, False) for f in base]
    assert stats["rgb_frames"] == len(base) and stats["deint_temporal_frames"] == len(base) - 1
    # field rate in front of the resampler: two scratch surfaces per picture
    base2, per2 = _want("paff_176", 1, rate=1)
    frames, stats = _decode(data, 0, 1, target_width=100, target_height=70, deinterlace_rate=1, **ON)
    assert frames == [scale_frame(f, W, H, 1, (0, 0, W, H), target) for f in base2] and stats["per"] == per2


def test_device_resident_frames():
    """device_output: output_frame_device hands out D3(F_n, F_n-1)."""
    hip = _hip()
    L = api.lib()
    data = _stream("paff_176")[0]
    want, per = _want("paff_176", 1)
    fs = len(want[0])
    with api.JmAmdDec(0, 1, options=dict(device_output=1, **ON)) as d:
        count = 0
        for nal in api.split_nalus(data) + [None] * 64:
            if api.jm_nvdec_is_exit(d.h):
                break
            _, got = api.jm_nvdec_decode_frame(nal, len(nal) if nal else 0, d.h)
            if not got:
                continue
            dev, ln = C.c_void_p(), C.c_int(0)
            assert L.jm_amddec_output_frame_device(C.byref(dev), C.byref(ln), d.h) == fs and ln.value == fs
            host = np.zeros(fs, np.uint8)
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, fs, 2) == 0
            assert host.tobytes() == want[count], f"frame {count}"
            count += 1
        assert count == len(want) and d.stat("deint_temporal_frames") == len(want) - 1 and d.stat("errors") == 0
        RAN["temporal_frames"] += d.stat("deint_temporal_frames")


@pytest.mark.parametrize("route", ["1/1", "0/1", "direct"])
def test_every_fetch_route(route, monkeypatch):
    monkeypatch.setenv("JM_AMD_DEC_OUT_FETCH", route)
    _check("paff_176", 1)
    _check("hevc", 0)


@pytest.mark.parametrize("name", ["paff_176", "hevc"])
def test_output_does_not_depend_on_batching(name):
    """The same stream as one chunk, NAL by NAL, with chain launches off (chain_depth 1) and on a synchronous handle (sync 1): identical bytes, all
    equal to the expectation -- the held surface is ordered like any surface a frame displays."""
    data = _stream(name)[0]
    a, _ = _check(name, 1, chunks=[data])
    b, _ = _check(name, 1)
    c, _ = _check(name, 1, sync=1)
    d, _ = _check(name, 1, knobs=(("chain_depth", 1),))
    assert a == b == c == d


def test_three_handles_side_by_side():
    """A temporal handle, a mode-2 handle without the option and a plain handle on three threads over the same stream: each matches its own
    expectation, so a held surface and k_deint3 in a batch leave the other handles' frames alone."""
    data, _, fields, _, _ = _stream("paff_176")
    F, W, H = _oracle_frames("paff_176", 1)
    wants = [list(_want("paff_176", 1)[0]), [deint_frame(F[i], W, H, 1, 2, f - 1) for i, f in enumerate(fields)], list(F)]
    opts = [ON, dict(deinterlace=2), {}]
    got, errs = [None] * 3, [None] * 3

    def run(i):
        try:
            got[i], st = _decode(data, 0, 1, **opts[i])
            assert st["deint_temporal_frames"] == (len(fields) - 1 if i == 0 else 0)
        except Exception as e:          # (reported below, on the main thread)
            errs[i] = e
    for rnd in range(2):
        ts = [threading.Thread(target=run, args=(i,)) for i in range(3)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        for i in range(3):
            assert errs[i] is None, errs[i]
            assert got[i] == wants[i], f"round {rnd}, handle {i}"


def test_k_deint3_ran():
    """The closing assertion: the handles above reported frames whose D read a previous frame (on its own, this test decodes one stream itself)."""
    if not RAN["temporal_frames"]:
        _check("paff_176", 1)
    assert RAN["temporal_frames"] > 0
