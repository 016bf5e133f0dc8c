"""Field-rate deinterlaced output on the device (option deinterlace_rate, k_deint2), bit for bit against the numpy restatement of D (deint_ref.py)
applied to the CPU oracle's frames, the expected list interleaved (first field, second field): the stand-alone call, both codecs end to end in
both modes and formats, every output route, in front of the resampler and of the colour conversion, through the push / pull facade, and beside
plain and frame-rate handles in the same batches."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

from deint_ref import combed_share, deint_frame, deint_plane
from jmcodec_amd import api
from test_rgb_output_host import rgb_frame
from test_scaled_output_host import scale_frame, split_frame
from tools import streams

pytestmark = pytest.mark.gpu

T = 10          # the default threshold


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def _surface(rng, W, H, pitch, kind):
    """A pitch-linear NV12 surface of H rows: noise, a smooth picture with a little noise (both branches of mode 2 live), or rows alternating 0 / 255."""
    n = pitch * H * 3 // 2
    if kind == 0:
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == 1:
        y, x = np.mgrid[0:H * 3 // 2, 0:pitch]
        base = (96 + 60 * np.sin(x / 9.0) + 40 * np.cos(y / 7.0)).astype(np.int64)
        comb = ((y & 1) * rng.integers(0, 2, (H * 3 // 2, 1)) * 40)           # some row pairs are combed
        return np.clip(base + comb + rng.integers(-3, 4, base.shape), 0, 255).astype(np.uint8).reshape(-1)
    s = np.zeros((H * 3 // 2, pitch), np.uint8)
    s[1::2] = 255
    return s.reshape(-1)


def test_deinterlace2_device_random_cases():
    """jm_amddec_deinterlace2_device alone: 240 seeded random sizes (no multiples of 16, odd chroma row counts), source and destination pitches,
    modes, first fields and thresholds -- both destinations against D of the surface's planes, padding bytes untouched; then the refusals."""
    hip = _hip()
    rng = random.Random(0xF1E1D2)
    d_src, d_a, d_b = C.c_void_p(), C.c_void_p(), C.c_void_p()
    cap = 2048 * 1200 * 3 // 2
    assert hip.hipMalloc(C.byref(d_src), cap) == 0 and hip.hipMalloc(C.byref(d_a), cap) == 0 and hip.hipMalloc(C.byref(d_b), cap) == 0
    shares = [{"luma": [], "chroma": []}, {"luma": [], "chroma": []}]           # per kept parity
    try:
        cases = [(rng.randrange(2, 400, 2), rng.randrange(4, 300, 2)) for _ in range(236)] + [(1920, 1080), (1920, 1088), (16, 4), (2, 4)]
        for n, (W, H) in enumerate(cases):
            pitch = W + rng.choice([0, 2, 14, 128 - W % 128])
            dp = W + rng.choice([0, 0, 6, 16, 128 - W % 128])
            dco = dp * H + rng.choice([0, 16, 256])
            mode, first = 1 + n % 2, 1 + (n // 2) % 2
            thr = rng.choice([0, 1, 10, 40, 255, rng.randrange(1, 256)])
            src = _surface(np.random.default_rng(n), W, H, pitch, n % 3 if n % 7 else 2)
            out_n = dco + dp * (H // 2)
            assert src.size <= cap and out_n <= cap
            assert hip.hipMemcpy(d_src, src.ctypes.data_as(C.c_void_p), src.size, 1) == 0
            assert hip.hipMemset(d_a, 0xA5, out_n) == 0 and hip.hipMemset(d_b, 0xA5, out_n) == 0
            rc = api.deinterlace2_device(d_src, pitch, pitch * H, W, H, mode, first, d_a, d_b, dst_pitch=dp, dst_chroma_offset=dco, threshold=thr)
            assert rc == 0, (n, W, H, rc)
            Y = src[:pitch * H].reshape(H, pitch)[:, :W]
            uv = src[pitch * H:].reshape(H // 2, pitch)[:, :W]
            t = thr or 10
            for which, (d_dst, keep) in enumerate(((d_a, first), (d_b, 3 - first))):
                out = np.zeros(out_n, np.uint8)
                assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d_dst, out_n, 2) == 0
                st = shares[keep - 1] if mode == 2 else None
                wy = deint_plane(Y, mode, keep - 1, t, st["luma"] if st else None)
                wu = deint_plane(uv[:, 0::2], mode, keep - 1, t, st["chroma"] if st else None)
                wv = deint_plane(uv[:, 1::2], mode, keep - 1, t, st["chroma"] if st else None)
                gy = out[:dp * H].reshape(H, dp)
                guv = out[dco:dco + dp * (H // 2)].reshape(H // 2, dp)
                what = f"case {n}: {W}x{H} pitch {pitch} -> {dp} mode {mode} first {first} output {which} T {t}"
                assert np.array_equal(gy[:, :W], wy), what + " (luma)"
                assert np.array_equal(guv[:, 0:W:2], wu) and np.array_equal(guv[:, 1:W:2], wv), what + " (chroma)"
                # nothing outside the rows' W bytes is written
                assert (gy[:, W:] == 0xA5).all() and (guv[:, W:] == 0xA5).all() and (out[dp * H:dco] == 0xA5).all(), what + " (padding)"
        # both branches of mode 2 ran, for either kept parity
        for st in shares:
            assert 0.05 <= combed_share(st["luma"]) <= 0.95 and 0.01 <= combed_share(st["chroma"]) <= 0.99
        # invalid arguments are refused before anything runs
        f = api.deinterlace2_device
        assert f(d_src, 128, 128 * 64, 100, 63, 1, 1, d_a, d_b) == -1          # odd height
        assert f(d_src, 128, 128 * 64, 99, 64, 1, 1, d_a, d_b) == -1           # odd width
        assert f(d_src, 128, 128 * 2, 100, 2, 1, 1, d_a, d_b) == -1            # h < 4
        assert f(d_src, 128, 128 * 64, 100, 64, 3, 1, d_a, d_b) == -1          # mode
        assert f(d_src, 128, 128 * 64, 100, 64, 2, 0, d_a, d_b) == -1          # first_field
        assert f(d_src, 128, 128 * 64, 100, 64, 2, 1, d_a, d_b, threshold=256) == -1
        assert f(d_src, 64, 64 * 64, 100, 64, 2, 1, d_a, d_b) == -1            # pitch < w
        assert f(d_src, 128, 128 * 64, 100, 64, 2, 1, d_a, None) == -1         # a destination is missing
        # overlapping destinations, a destination over the source
        fs = 100 * 64 * 3 // 2
        assert f(d_src, 128, 128 * 64, 100, 64, 2, 1, d_a, d_a) == -1
        assert f(d_src, 128, 128 * 64, 100, 64, 2, 1, d_a, C.c_void_p(d_a.value + fs - 1)) == -1
        assert f(d_src, 128, 128 * 64, 100, 64, 2, 1, C.c_void_p(d_a.value + fs - 1), d_a) == -1
        assert f(d_src, 128, 128 * 64, 100, 64, 2, 1, d_src, d_b) == -1
        assert f(d_src, 128, 128 * 64, 100, 64, 2, 1, d_a, C.c_void_p(d_src.value + 128 * 96 - 29)) == -1       # the source's last byte
        assert f(d_src, 128, 128 * 64, 100, 64, 2, 1, d_a, C.c_void_p(d_a.value + fs)) == 0                      # back to back is fine
    finally:
        hip.hipFree(d_src)
        hip.hipFree(d_a)
        hip.hipFree(d_b)


# ---- through the decoder --------------------------------------------------------------------------------------------------------
STATS = ("deint_frames", "field_rate_pairs", "lone_fields", "scaled_frames", "rgb_frames", "interlaced_sequence", "frames")


def _decode(data, codec=0, fmt=1, rgb=None, **opts):
    with api.JmAmdDec(codec, fmt, options=opts, rgb=rgb) as d:
        frames = d.decode_stream(data)
        assert d.stat("errors") == 0, api.lib().jm_amddec_last_error(d.h)
        stats = {k: d.stat(k) for k in STATS}
        stats["fields"] = [d.stat(f"display_field:{i}") for i in range(len(frames))]
        stats["pictures"] = [d.stat(f"display_picture:{i}") for i in range(len(frames))]
        return frames, stats


def _gen(kw):
    """The stream and, per display frame, the field that is first in time (the generator's listing; see test_deinterlace_gpu._gen)."""
    data = streams.generate(**kw)
    listing = streams.last_fields()
    typed0 = kw.get("poc_type", 2) == 0 or kw.get("bframes", 0) > 0
    return data, [2 if (bottom and typed0) else 1 for _, bottom in listing]


def _want(blob, n, W, H, fmt, mode, fields, lone=(), thr=T, stats=None):
    """The output frames of a field-rate handle: display picture i keeps fields[i] first, then the other field (0: it is not deinterlaced and
    leaves once; a picture in `lone` is bob from its one field, once).  Returns (frames, display_field per frame, display_picture per frame);
    stats: per kept parity, {"luma": [...], "chroma": [...]} as deint_frame's."""
    fs = W * H * 3 // 2
    out, kept, pic = [], [], []
    for i in range(n):
        F = blob[i * fs:(i + 1) * fs]
        order = [] if not fields[i] else [fields[i]] if i in lone else [fields[i], 3 - fields[i]]
        if not order:
            out.append(F), kept.append(0), pic.append(i)
        for f in order:
            st = stats[f - 1] if stats is not None and i not in lone else None
            out.append(deint_frame(F, W, H, fmt, 1 if i in lone else mode, f - 1, thr, st))
            kept.append(f), pic.append(i)
    return out, kept, pic


def _check(decode_ref, data, fields, mode, fmt=1, codec=0, lone=(), cond=False, **opts):
    blob, n, W, H = decode_ref(data, fmt)
    assert n == len(fields)
    st = [{"luma": [], "chroma": []}, {"luma": [], "chroma": []}]
    want, kept, pic = _want(blob, n, W, H, fmt, mode, fields, lone, opts.get("deinterlace_threshold", 0) or T, st)
    if cond:        # the inputs keep both branches of mode 2 alive for EACH parity (asserted on the oracle's frames, before anything is compared)
        assert mode == 2
        for p in (0, 1):
            l, c = combed_share(st[p]["luma"]), combed_share(st[p]["chroma"])
            assert 0.05 <= l <= 0.95 and 0.01 <= c <= 0.99, (p, l, c)
    frames, stats = _decode(data, codec, fmt, deinterlace=mode, deinterlace_rate=1, **opts)
    assert len(frames) == len(want)
    assert stats["fields"] == kept and stats["pictures"] == pic
    for i, f in enumerate(frames):
        assert f == want[i], f"output frame {i} of {len(want)} differs ({W}x{H}, mode {mode}, fmt {fmt}, picture {pic[i]}, field {kept[i]})"
    pairs = sum(1 for i, f in enumerate(fields) if f and i not in lone)
    assert stats["frames"] == len(want) and stats["field_rate_pairs"] == pairs and stats["deint_frames"] == sum(1 for f in kept if f)
    return stats


PAFF_176 = dict(width=176, height=160, frames=7, gop=7, mode=1, num_ref=2, seed=0x5CA10004, cabac=1, paff=1, bframes=2)
PAFF2 = dict(width=96, height=64, frames=8, gop=4, seed=302, paff=2, num_ref=2, bframes=1)
PAFF_1088 = dict(width=1920, height=1088, frames=4, gop=4, mode=1, num_ref=2, seed=0x5CA10004, cabac=1, paff=1)
PROGRESSIVE = dict(width=176, height=144, frames=6, gop=6, mode=1, num_ref=2, seed=0xDE1A0001, cabac=1, t8x8=1, bframes=2)
HEVC = dict(width=90, height=70, frames=5, ctb_log2=5, mode=1, seed=0xDE1A0002)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("fmt", [1, 0])
def test_paff_field_pairs_and_frames(oracle, mode, fmt):
    """Frame pictures and field pairs of either first parity, B pictures: two frames per picture, the field first in time first (auto); mode 2
    with both branches alive for each parity."""
    data, fields = _gen(PAFF_176)
    assert 1 in fields and 2 in fields
    stats = _check(oracle.decode, data, fields, mode, fmt, cond=mode == 2)
    assert stats["interlaced_sequence"] == 1 and stats["frames"] == 2 * len(fields)
    if mode == 2:
        _check(oracle.decode, data, [2] * len(fields), mode, fmt, deinterlace_field=2)
        _check(oracle.decode, data, [1] * len(fields), mode, fmt, deinterlace_field=1, deinterlace_threshold=3)


@pytest.mark.parametrize("mode", [1, 2])
def test_paff_every_picture_two_fields(oracle, mode):
    data, fields = _gen(PAFF2)
    _check(oracle.decode, data, fields, mode, 1)
    _check(oracle.decode, data, [2] * len(fields), mode, 0, deinterlace_field=2)


@pytest.mark.parametrize("mode", [1, 2])
def test_paff_1088(oracle, mode):
    """1920 x 1088, frame pictures and field pairs; carries the both-branches condition for each parity."""
    data, fields = _gen(PAFF_1088)
    _check(oracle.decode, data, fields, mode, 0, cond=mode == 2)


def _lone_stream():
    """A paff=2 stream cut before the second field of its last picture, then a second stream (the stream of the deinterlace tests)."""
    kw = dict(width=96, height=64, frames=4, gop=4, seed=302, paff=2, num_ref=2)
    data, f1 = _gen(kw)
    first_coded = [2 if bottom else 1 for _, bottom in streams.last_fields()]
    starts = [i for i in range(len(data) - 4) if data[i:i + 4] == b"\0\0\0\1" or (data[i:i + 3] == b"\0\0\1" and data[i - 1:i] != b"\0")]
    tail, f2 = _gen(dict(kw, seed=303, paff=1))
    return data[:starts[-1]] + tail, f1[:-1] + [first_coded[-1]] + f2, {len(f1) - 1}


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("variant", ["plain", "scaled", "rgb"])
def test_lone_field_is_one_frame_from_that_field(oracle, mode, variant):
    data, fields, lone = _lone_stream()
    blob, n, W, H = oracle.decode(data, 1)
    want, kept, pic = _want(blob, n, W, H, 1, mode, fields, lone)
    assert len(want) == 2 * n - 1
    opts, rgb = {}, None
    if variant == "scaled":
        crop, target = (4, 2, 90, 60), (60, 34)
        opts = dict(crop_x=4, crop_y=2, crop_w=90, crop_h=60, target_width=60, target_height=34)
        want = [scale_frame(f, W, H, 1, crop, target) for f in want]
    if variant == "rgb":
        rgb = api.rgb_spec("u8", planar=True)
        want = [rgb_frame(f, W, H, 1, (0, 0, W, H), (W, H), rgb, 6, False) for f in want]
    frames, stats = _decode(data, 0, 1, rgb=rgb, deinterlace=mode, deinterlace_rate=1, **opts)
    assert stats["lone_fields"] == 1 and stats["fields"] == kept and stats["pictures"] == pic
    assert stats["deint_frames"] == 2 * n - 1 and stats["field_rate_pairs"] == n - 1
    assert frames == want


@pytest.mark.parametrize("mode", [1, 2])
def test_progressive_h264_only_when_asked(oracle, mode):
    data, fields = _gen(PROGRESSIVE)
    stats = _check(oracle.decode, data, [0] * len(fields), mode, 1)                               # auto: frame_mbs_only_flag = 1
    assert stats["interlaced_sequence"] == 0 and stats["field_rate_pairs"] == 0
    _check(oracle.decode, data, fields, mode, 1, deinterlace_when=1)
    _check(oracle.decode, data, [2] * len(fields), mode, 0, deinterlace_when=1, deinterlace_field=2)


@pytest.mark.parametrize("mode", [1, 2])
def test_hevc_only_when_asked(mode):
    data = streams.generate_hevc(**HEVC)
    ref = streams.OracleHevc().decode
    _check(ref, data, [0] * 5, mode, 1, codec=1)
    _check(ref, data, [1] * 5, mode, 1, codec=1, deinterlace_when=1)
    _check(ref, data, [2] * 5, mode, 0, codec=1, deinterlace_when=1, deinterlace_field=2)


@pytest.mark.parametrize("route", [("JM_AMD_DEC_OUT_FETCH", "1/1"), ("JM_AMD_DEC_OUT_FETCH", "0/1"), ("JM_AMD_DEC_OUT_FETCH", "direct"),
                                   ("JM_AMD_DEC_OUT_PINNED", "1"), ("JM_AMD_DEC_OUT_DIRECT", "1")])
def test_every_output_route(oracle, route, monkeypatch):
    monkeypatch.setenv(*route)
    data, fields = _gen(PAFF_176)
    _check(oracle.decode, data, fields, 2, 1)
    _check(oracle.decode, data, fields, 1, 0)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("fmt", [1, 0])
def test_downscaled_after_deinterlacing(oracle, mode, fmt):
    """R_G(D_p(F)) for both p: k_deint2 writes the two frames into the batch's scratch and two k_scale_pack jobs read them."""
    data, fields = _gen(PAFF_176)
    blob, n, W, H = oracle.decode(data, fmt)
    crop, target = (8, 6, 160, 148), (100, 70)
    want = [scale_frame(f, W, H, fmt, crop, target) for f in _want(blob, n, W, H, fmt, mode, fields)[0]]
    frames, stats = _decode(data, 0, fmt, deinterlace=mode, deinterlace_rate=1, crop_x=8, crop_y=6, crop_w=160, crop_h=148, target_width=100,
                            target_height=70)
    assert frames == want
    assert stats["deint_frames"] == 2 * n and stats["scaled_frames"] == 2 * n and stats["field_rate_pairs"] == n


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("spec", [dict(dtype="u8", planar=True), dict(dtype="f16", planar=False)])
@pytest.mark.parametrize("scaled", [False, True])
def test_rgb_after_deinterlacing(oracle, mode, spec, scaled):
    """C(R_G(D_p(F))) for both p with u8 planar and f16 interleaved samples, with and without a geometry."""
    data, fields = _gen(PAFF_176)
    blob, n, W, H = oracle.decode(data, 1)
    rgb = api.rgb_spec(**spec)
    crop, target = ((0, 0, W, H), (120, 90)) if scaled else ((0, 0, W, H), (W, H))
    want = [rgb_frame(f, W, H, 1, crop, target, rgb, 6, False) for f in _want(blob, n, W, H, 1, mode, fields)[0]]
    opts = dict(target_width=120, target_height=90) if scaled else {}
    frames, stats = _decode(data, 0, 1, rgb=rgb, deinterlace=mode, deinterlace_rate=1, **opts)
    assert frames == want
    assert stats["deint_frames"] == 2 * n and stats["rgb_frames"] == 2 * n and stats["field_rate_pairs"] == n


def test_device_resident_frames_and_the_derived_calls(oracle):
    """device_output: output_frame_device hands out both frames of a pair in turn; output_argb_device and output_nv12_pitch_device work on
    whichever of the two is current."""
    hip = _hip()
    L = api.lib()
    L.jm_amddec_output_argb_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.jm_amddec_output_nv12_pitch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    data, fields = _gen(PAFF_176)
    for fmt in (1, 0):
        blob, n, W, H = oracle.decode(data, fmt)
        want, kept, _ = _want(blob, n, W, H, fmt, 2, fields)
        fs, pitch, npitch = W * H * 3 // 2, W * 4 + 64, W + 80
        d_argb, d_nv12 = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_argb), pitch * H) == 0 and hip.hipMalloc(C.byref(d_nv12), npitch * H * 3 // 2) == 0
        try:
            with api.JmAmdDec(0, fmt, options=dict(device_output=1, deinterlace=2, deinterlace_rate=1)) as d:
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
                    assert host.tobytes() == want[count], f"fmt {fmt} output frame {count}"
                    Y, U, V = split_frame(want[count], W, H, fmt)
                    assert L.jm_amddec_output_nv12_pitch_device(d_nv12, npitch, d.h) == 0
                    nv = np.zeros(npitch * H * 3 // 2, np.uint8)
                    assert hip.hipMemcpy(nv.ctypes.data_as(C.c_void_p), d_nv12, nv.size, 2) == 0
                    nv = nv.reshape(H * 3 // 2, npitch)
                    assert np.array_equal(nv[:H, :W], Y) and np.array_equal(nv[H:, 0:W:2], U) and np.array_equal(nv[H:, 1:W:2], V)
                    assert L.jm_amddec_output_argb_device(d_argb, pitch, d.h) == 0
                    argb = np.zeros(pitch * H, np.uint8)
                    assert hip.hipMemcpy(argb.ctypes.data_as(C.c_void_p), d_argb, pitch * H, 2) == 0
                    argb = argb.reshape(H, pitch)[:, :W * 4].reshape(H, W, 4).astype(np.int32)
                    Yi = Y.astype(np.int32)
                    Dc = U.astype(np.int32).repeat(2, 0).repeat(2, 1) - 128
                    Ec = V.astype(np.int32).repeat(2, 0).repeat(2, 1) - 128
                    c = 298 * (Yi - 16) + 128
                    R, G, B = np.clip((c + 409 * Ec) >> 8, 0, 255), np.clip((c - 100 * Dc - 208 * Ec) >> 8, 0, 255), np.clip((c + 516 * Dc) >> 8, 0, 255)
                    assert np.array_equal(argb[:, :, 0], B) and np.array_equal(argb[:, :, 1], G) and np.array_equal(argb[:, :, 2], R)
                    count += 1
                assert count == 2 * n and set(kept) == {1, 2} and d.stat("deint_frames") == 2 * n and d.stat("field_rate_pairs") == n
        finally:
            hip.hipFree(d_argb)
            hip.hipFree(d_nv12)


def test_feed_annexb(oracle):
    """jm_amddec_feed_annexb: the native feeding loop fetches the frames of a field-rate handle (the last one it fetched is in the buffer), the
    rest is drained."""
    L = api.lib()
    data, fields = _gen(PAFF_176)
    blob, n, W, H = oracle.decode(data, 1)
    want, _, _ = _want(blob, n, W, H, 1, 2, fields)
    fs = W * H * 3 // 2
    with api.JmAmdDec(0, 1, options=dict(deinterlace=2, deinterlace_rate=1)) as d:
        out = (C.c_ubyte * (fs + 64))()
        got = L.jm_amddec_feed_annexb(data, len(data), 1, out, len(out), d.h)
        assert 0 <= got <= 2 * n, api.lib().jm_amddec_last_error(d.h)
        if got:
            assert bytes(out[:fs]) == want[got - 1]
        rest = []
        while not api.jm_nvdec_is_exit(d.h):
            ret, g = api.jm_nvdec_decode_frame(None, 0, d.h)
            assert ret == 0
            if g == 1:
                d._pull(rest)
        assert rest == want[got:]
        assert d.stat("deint_frames") == 2 * n and d.stat("frames") == 2 * n


@pytest.mark.parametrize("callback", [False, True])
def test_push_pull_facade(oracle, callback):
    """jm_intel_dec_*: the options set through jm_amdintel_decoder before init."""
    data, fields = _gen(PAFF_176)
    blob, n, W, H = oracle.decode(data, 1)
    frames, info, _, _ = api.intel_push_pull(data, callback=callback, options=dict(deinterlace=2, deinterlace_rate=1))
    assert frames == _want(blob, n, W, H, 1, 2, fields)[0]
    assert f"Deinterlace:\tcomb-adaptive, auto, field rate, {2 * n} frames" in info


def test_two_sequences_keep_their_own_decision(oracle):
    """An interlaced sequence, then a progressive one of the same size: the frames the second IDR picture flushes leave as pairs, its own once."""
    a, fa = _gen(dict(PAFF_176, frames=6, gop=6))
    b, fb = _gen(dict(width=176, height=160, frames=5, gop=5, mode=1, num_ref=2, seed=0xDE1A0003, cabac=1, bframes=2))
    want, kept = [], []
    for x, f in ((a, fa), (b, [0] * len(fb))):
        blob, n, W, H = oracle.decode(x, 1)
        w, k, _ = _want(blob, n, W, H, 1, 2, f)
        want += w
        kept += k
    frames, stats = _decode(a + b, deinterlace=2, deinterlace_rate=1)
    assert stats["fields"] == kept and stats["field_rate_pairs"] == len(fa)
    assert stats["pictures"] == [i for i, f in enumerate(fa + [0] * len(fb)) for _ in range(2 if f else 1)]
    assert frames == want


def test_mixed_batches_of_field_rate_frame_rate_and_plain_handles(oracle):
    """8 handles on 8 threads over the same kind of stream: plain, frame-rate deinterlacing, field rate (both modes), field rate + scaled, field
    rate + RGB -- all exact, so pairs and single jobs share k_deint2's launches and leave every other handle's frames alone."""
    kinds = ["plain", "comb2", "bob2", "comb2_scaled", "comb1", "comb2_rgb", "comb2", "plain"]
    target, rgb = (88, 80), api.rgb_spec("u8", planar=True)
    gens = [_gen(dict(PAFF_176, seed=0xF1E1D100 + i, frames=10, gop=10)) for i in range(8)]
    wants = []
    for (data, fields), k in zip(gens, kinds):
        blob, n, W, H = oracle.decode(data, 1)
        assert n == 10
        fs = W * H * 3 // 2
        if k == "plain":
            w = [blob[j * fs:(j + 1) * fs] for j in range(n)]
        elif k == "comb1":
            w = [deint_frame(blob[j * fs:(j + 1) * fs], W, H, 1, 2, fields[j] - 1, T) for j in range(n)]
        else:
            w = _want(blob, n, W, H, 1, 1 if k == "bob2" else 2, fields)[0]
        if k == "comb2_scaled":
            w = [scale_frame(f, W, H, 1, (0, 0, W, H), target) for f in w]
        if k == "comb2_rgb":
            w = [rgb_frame(f, W, H, 1, (0, 0, W, H), (W, H), rgb, 6, False) for f in w]
        wants.append(w)
    got, errs = [None] * 8, [None] * 8

    def run(i):
        try:
            k = kinds[i]
            opts = {} if k == "plain" else dict(deinterlace=1 if k == "bob2" else 2, deinterlace_rate=0 if k == "comb1" else 1)
            if k == "comb2_scaled":
                opts.update(target_width=target[0], target_height=target[1])
            got[i], _ = _decode(gens[i][0], 0, 1, rgb=rgb if k == "comb2_rgb" else None, **opts)
        except Exception as e:          # (reported below, on the main thread)
            errs[i] = e
    ts = [threading.Thread(target=run, args=(i,)) for i in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for i in range(8):
        assert errs[i] is None, errs[i]
        assert len(got[i]) == len(wants[i]) == (10 if kinds[i] in ("plain", "comb1") else 20)
        assert got[i] == wants[i], f"handle {i} ({kinds[i]})"
