"""Placed output on the device (INTEGRATION.md "Placed output"), bit-exact against the numpy restatement (test_placed_output_host.py) applied to the
CPU oracle's unscaled frames: the stand-alone calls over the host test's case list, H.264 / HEVC / MJPEG end to end with a letterbox and with an
explicit rectangle in every output format, in front of the field-rate deinterlacer, across a resolution change, with a sample aspect ratio, in
device memory, and beside stretched and plain handles in the same batches."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import jpeg_ref
from jmcodec_amd import api
from tools import streams
from test_field_rate_gpu import PAFF2, _gen, _want
from test_placed_output_host import (FILL_RGB, FILL_YUV, _rgb3, fit_rect_ref, place_frame, place_rgb_frame, placed_cases, rgb_specs)
from test_scaled_output_host import _packout_ref, scale_frame

pytestmark = pytest.mark.gpu

KEYS = ("rect_x", "rect_y", "rect_w", "rect_h")


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


# ---- the stand-alone calls ---------------------------------------------------------------------------------------------------------
def test_rect_device_calls_over_the_shared_cases():
    """jm_amddec_scale_rect_device and jm_amddec_rgb_rect_device over the host walk's case list: every byte of the frame is written (it starts as
    0xA5 and every case has fill-only tiles), the bytes behind it are not; then no placement, and the refusals."""
    hip = _hip()
    d_src, d_dst = C.c_void_p(), C.c_void_p()
    src_cap, dst_cap, guard = 512 * 300 * 3 // 2, 1024 * 1024 * 3 // 2 + 64, 64
    assert hip.hipMalloc(C.byref(d_src), src_cap) == 0 and hip.hipMalloc(C.byref(d_dst), dst_cap) == 0

    def run(call, out_n):
        assert out_n + guard <= dst_cap
        assert hip.hipMemset(d_dst, 0xA5, out_n + guard) == 0
        assert call() == 0
        out = np.zeros(out_n + guard, np.uint8)
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d_dst, out_n + guard, 2) == 0
        assert (out[out_n:] == 0xA5).all(), "bytes behind the frame were written"
        return out[:out_n].tobytes()
    try:
        for n, name, W, H, crop, target, rect, pitch, lone, fmt, hs, src in placed_cases():
            assert src.size <= src_cap
            assert hip.hipMemcpy(d_src, src.ctypes.data_as(C.c_void_p), src.size, 1) == 0
            what = f"case {n} ({name}) lone {lone} fmt {fmt}"
            F = _packout_ref(src, pitch, hs, W, H, lone, fmt)
            for fill, ycc in ((-1, (16, 128, 128)), (FILL_YUV, _rgb3(FILL_YUV))):
                got = run(lambda: api.scale_rect_device(d_src, pitch, pitch * hs, W, H, crop, target, fmt, d_dst, rect, fill, lone_field=lone),
                          target[0] * target[1] * 3 // 2)
                assert got == place_frame(F, W, H, fmt, crop, target, rect, ycc), what + f" fill {fill:#x}"
            # no placement (all zero, or the whole target spelled out) is jm_amddec_scale_device
            t2 = (rect[2], rect[3])
            for r in ((0, 0, 0, 0), (0, 0) + t2):
                got = run(lambda: api.scale_rect_device(d_src, pitch, pitch * hs, W, H, crop, t2, fmt, d_dst, r, FILL_YUV, lone_field=lone), t2[0] * t2[1] * 3 // 2)
                assert got == scale_frame(F, W, H, fmt, crop, t2), what + f" unplaced {r}"
            if fmt:
                continue
            F = _packout_ref(src, pitch, hs, W, H, lone, 1)
            for spec in rgb_specs():
                sz = api.RGB_SAMPLE_BYTES[spec.dtype]
                got = run(lambda: api.rgb_rect_device(d_src, pitch, pitch * hs, W, H, crop, target, spec, d_dst, rect, FILL_RGB, lone_field=lone),
                          3 * target[0] * target[1] * sz)
                want = place_rgb_frame(F, W, H, crop, target, rect, spec, 1, False, _rgb3(FILL_RGB))
                assert got == want, what + f" dtype {spec.dtype} planar {spec.planar} bgr {spec.bgr}"
        # refusals, before anything runs: odd, negative, outside the target, a ratio beyond the limits into the rectangle, a fill out of range
        s = lambda rect, fill=-1, target=(96, 48): api.scale_rect_device(d_src, 128, 128 * 64, 100, 64, (0, 0, 100, 64), target, 1, d_dst, rect, fill)
        assert s((2, 2, 60, 34)) == 0
        for bad in ((1, 2, 60, 34), (2, 2, 61, 34), (-2, 2, 60, 34), (40, 2, 60, 34), (2, 16, 60, 34), (96, 0, 0, 0), (2, 2, 12, 34), (2, 2, 60, 6)):
            assert s(bad) == -1, bad
        assert s((2, 2, 60, 34), fill=-2) == -1 and s((2, 2, 60, 34), fill=0x1000000) == -1
        assert s((0, 0, 400, 256), target=(1024, 1024)) == 0 and s((0, 0, 0, 0), target=(1024, 1024)) == -1      # the limits apply to the rectangle
        spec = api.rgb_spec("u8", matrix=1, range=1)
        r = lambda rect, fill=-1: api.rgb_rect_device(d_src, 128, 128 * 64, 100, 64, (0, 0, 100, 64), (96, 48), spec, d_dst, rect, fill)
        assert r((2, 2, 60, 34)) == 0 and r((1, 2, 60, 34)) == -1 and r((40, 2, 60, 34)) == -1 and r((2, 2, 12, 34)) == -1 and r((2, 2, 60, 34), -2) == -1
    finally:
        hip.hipFree(d_src)
        hip.hipFree(d_dst)


# ---- through the decoder ---------------------------------------------------------------------------------------------------------
STREAMS = {
    "h264_96x80": (0, lambda: streams.generate(width=96, height=80, frames=4, gop=4, mode=1, num_ref=2, seed=0x91ACE01, bframes=1, poc_type=0)),
    "h264_90x70": (0, lambda: streams.generate(width=90, height=70, frames=3, gop=3, mode=1, seed=0x91ACE02, cabac=1)),
    "hevc_96x80": (1, lambda: streams.generate_hevc(width=96, height=80, frames=3, ctb_log2=5, mode=1, seed=0x91ACE03)),
    "hevc_90x70": (1, lambda: streams.generate_hevc(width=90, height=70, frames=3, ctb_log2=5, mode=1, seed=0x91ACE04)),
}
OUTPUTS = {"nv12": (0, None), "i420": (1, None), "rgb_u8_planar": (1, dict(dtype="u8", planar=True)), "rgb_f16_hwc": (1, dict(dtype="f16", planar=False))}
_ref_cache = {}


def _reference(name, oracle):
    """(stream, codec, the oracle's I420 frames, W, H) of one of STREAMS, decoded once."""
    if name not in _ref_cache:
        codec, gen = STREAMS[name]
        data = gen()
        blob, n, W, H = (oracle if codec == 0 else streams.OracleHevc()).decode(data, 1)
        fs = W * H * 3 // 2
        _ref_cache[name] = (data, codec, [blob[i * fs:(i + 1) * fs] for i in range(n)], W, H)
    return _ref_cache[name]


def _to_fmt(F, W, H, fmt):
    """An I420 frame as the frame of out_fmt."""
    return F if fmt == 1 else _i420_to_nv12(F, W, H)


def _i420_to_nv12(F, W, H):
    a = np.frombuffer(F, np.uint8)
    u, v = a[W * H:W * H * 5 // 4], a[W * H * 5 // 4:]
    return a[:W * H].tobytes() + np.stack([u, v], 1).tobytes()


def _expected(frames, W, H, fmt, rgb, crop, target, rect, fill, matrix=6, full=False):
    if rgb is None:
        ycc = (16, 128, 128) if fill < 0 else _rgb3(fill)
        return [place_frame(_to_fmt(F, W, H, fmt), W, H, fmt, crop, target, rect, ycc) for F in frames]
    return [place_rgb_frame(F, W, H, crop, target, rect, rgb, matrix, full, (0, 0, 0) if fill < 0 else _rgb3(fill)) for F in frames]


def _decode(data, codec=0, fmt=1, rgb=None, **opts):
    with api.JmAmdDec(codec, fmt, options=opts, rgb=rgb) as d:
        frames = d.decode_stream(data)
        assert d.stat("errors") == 0 and d.stat("failed") == 0, api.lib().jm_amddec_last_error(d.h)
        stats = {k: d.stat(k) for k in KEYS + ("placed_frames", "out_width", "out_height", "frames", "sar_num", "sar_den")}
        return frames, stats, api.jm_nvdec_show_dec_info(d.h)


@pytest.mark.parametrize("out", sorted(OUTPUTS))
@pytest.mark.parametrize("how", ["fit", "rect"])
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_placed_end_to_end(oracle, name, how, out):
    """A centred letterbox into 64x64, and an explicit 90x70 rectangle at (18, 10) of 128x96 with a fill colour (for the 90x70 streams pure padding
    with rx % 4 == 2): every frame is the restatement of the oracle's frame."""
    data, codec, F, W, H = _reference(name, oracle)
    fmt, rgbkw = OUTPUTS[out]
    rgb = api.rgb_spec(**rgbkw, scale=[1 / 255, 0.5 / 255, 2 / 255], bias=[-0.5, 0.25, 1.0]) if rgbkw and rgbkw["dtype"] != "u8" else \
        api.rgb_spec(**rgbkw) if rgbkw else None
    if how == "fit":
        target, rect, fill = (64, 64), fit_rect_ref(W, H, 64, 64), -1
        opts = dict(target_width=64, target_height=64, fit=1)
    else:
        target, rect, fill = (128, 96), (18, 10, 90, 70), 0x40A0C0
        opts = dict(target_width=128, target_height=96, rect_x=18, rect_y=10, rect_w=90, rect_h=70, fill=fill)
    frames, stats, text = _decode(data, codec, fmt, rgb, **opts)
    want = _expected(F, W, H, fmt, rgb, (0, 0, W, H), target, rect, fill)
    assert len(frames) == len(want)
    for i, f in enumerate(frames):
        assert f == want[i], f"frame {i} of {len(want)} differs ({name}, {how}, {out})"
    assert tuple(stats[k] for k in KEYS) == rect and stats["placed_frames"] == len(want)
    assert (stats["out_width"], stats["out_height"]) == target and f"Placement:\t{rect[0]},{rect[1]} {rect[2]}x{rect[3]}" in text


def test_paff_field_rate_letterboxed(oracle):
    """deinterlace 2 at field rate in front of a letterbox at the top left: two placed frames per picture, D before R."""
    data, fields = _gen(PAFF2)
    blob, n, W, H = oracle.decode(data, 1)
    D, _, _ = _want(blob, n, W, H, 1, 2, fields)
    rect = fit_rect_ref(W, H, 80, 80, 2)
    assert rect == (0, 0, 80, 54)
    frames, stats, _ = _decode(data, 0, 1, deinterlace=2, deinterlace_rate=1, target_width=80, target_height=80, fit=2)
    assert len(frames) == 2 * n and stats["placed_frames"] == 2 * n
    assert frames == [place_frame(f, W, H, 1, (0, 0, W, H), (80, 80), rect) for f in D]
    spec = api.rgb_spec("bf16", planar=True, bgr=True)
    frames, _, _ = _decode(data, 0, 1, rgb=spec, deinterlace=2, deinterlace_rate=1, target_width=80, target_height=80, fit=2, fill=0x102030)
    assert frames == [place_rgb_frame(f, W, H, (0, 0, W, H), (80, 80), rect, spec, 6, False, (0x10, 0x20, 0x30)) for f in D]


@pytest.mark.parametrize("fmt", [0, 1])
def test_mjpeg_fixture_letterboxed(fmt):
    data = open(os.path.join(jpeg_ref.GOLDEN_JPEG, "c420_72x40_rst3.jpg"), "rb").read()
    F = [f for f, _, _ in jpeg_ref.decode_stream(data, fmt)]
    rect = fit_rect_ref(72, 40, 64, 64)
    assert rect == (0, 14, 64, 36)
    with api.JmAmdDec(2, fmt, options=dict(target_width=64, target_height=64, fit=1)) as d:
        frames = d.decode_stream(data, chunks=[data])
        assert d.stat("errors") == 0 and tuple(d.stat(k) for k in KEYS) == rect
    assert frames == [place_frame(f, 72, 40, fmt, (0, 0, 72, 40), (64, 64), rect) for f in F]
    # JFIF: BT.601, full range
    spec = api.rgb_spec("u8", planar=False)
    with api.JmAmdDec(2, 1, options=dict(target_width=64, target_height=64, fit=1, fill=0xFF8000), rgb=spec) as d:
        frames = d.decode_stream(data, chunks=[data])
    F1 = [f for f, _, _ in jpeg_ref.decode_stream(data, 1)]
    assert frames == [place_rgb_frame(f, 72, 40, (0, 0, 72, 40), (64, 64), rect, spec, 6, True, (0xFF, 0x80, 0)) for f in F1]


def test_resolution_change_under_fit(oracle):
    """Three coded video sequences of different shapes, one square target: the rectangle is computed again at each, the stat follows, and every
    frame is the restatement with the rectangle of its own sequence."""
    parts = [streams.generate(width=96, height=80, frames=4, gop=4, mode=1, seed=1), streams.generate(width=320, height=176, frames=3, gop=3, mode=1, seed=2),
             streams.generate(width=64, height=112, frames=4, gop=4, mode=1, seed=3, bframes=2)]
    want, rects = [], []
    for x in parts:
        blob, n, W, H = oracle.decode(x, 1)
        fs = W * H * 3 // 2
        rects.append(fit_rect_ref(W, H, 128, 128))
        want += [place_frame(blob[i * fs:(i + 1) * fs], W, H, 1, (0, 0, W, H), (128, 128), rects[-1]) for i in range(n)]
    assert rects == [(0, 10, 128, 106), (0, 28, 128, 70), (26, 0, 74, 128)]
    seen, frames = [], []
    with api.JmAmdDec(0, 1, options=dict(target_width=128, target_height=128, fit=1)) as d:
        for nal in api.split_nalus(b"".join(parts)) + [None] * 64:
            if api.jm_nvdec_is_exit(d.h):
                break
            _, got = api.jm_nvdec_decode_frame(nal, len(nal) if nal else 0, d.h)
            r = tuple(d.stat(k) for k in KEYS)
            if r[2] and (not seen or seen[-1] != r):
                seen.append(r)
            if got == 1:
                d._pull(frames)
        assert d.stat("errors") == 0 and d.stat("placed_frames") == 11
    assert seen == rects
    assert [len(f) for f in frames] == [128 * 128 * 3 // 2] * 11
    assert frames == want


@pytest.mark.parametrize("codec", [0, 1])
def test_sar_4_3_with_and_without_fit_sar(oracle, codec):
    """An anamorphic stream (sample aspect ratio 4:3): fit_sar 1 letterboxes the shape it is shown in, fit_sar 0 the shape it is coded in."""
    kw = dict(vui_sar_idc=14)
    data = streams.generate(width=96, height=80, frames=3, gop=3, mode=1, seed=0x5A4, **kw) if codec == 0 else \
        streams.generate_hevc(width=96, height=80, frames=3, ctb_log2=5, mode=1, seed=0x5A5, **kw)
    blob, n, W, H = (oracle if codec == 0 else streams.OracleHevc()).decode(data, 1)
    fs = W * H * 3 // 2
    F = [blob[i * fs:(i + 1) * fs] for i in range(n)]
    for fit_sar, rect in ((1, (0, 12, 64, 40)), (0, (0, 4, 64, 54))):
        assert rect == fit_rect_ref(W, H, 64, 64, 1, (4, 3) if fit_sar else (0, 0))
        frames, stats, _ = _decode(data, codec, 1, target_width=64, target_height=64, fit=1, fit_sar=fit_sar)
        assert tuple(stats[k] for k in KEYS) == rect and (stats["sar_num"], stats["sar_den"]) == (4, 3)
        assert frames == [place_frame(f, W, H, 1, (0, 0, W, H), (64, 64), rect) for f in F]


def test_placed_stretched_and_plain_handles_together(oracle):
    """Three handles on three threads decoding at once -- letterboxed, stretched to the same target, plain -- each exact: placed and unplaced jobs
    share k_scale_pack's launches, and k_packout runs beside them."""
    datas = [streams.generate(**dict(streams.config_c1(stream_id=i, frames=10, width=352, height=240), seed=0x91ACE10 + i)) for i in range(3)]
    target, rect = (160, 160), fit_rect_ref(352, 240, 160, 160)
    opts = [dict(target_width=160, target_height=160, fit=1), dict(target_width=160, target_height=160), {}]
    wants = []
    for i, x in enumerate(datas):
        blob, n, W, H = oracle.decode(x, 1)
        fs = W * H * 3 // 2
        F = [blob[k * fs:(k + 1) * fs] for k in range(n)]
        wants.append([place_frame(f, W, H, 1, (0, 0, W, H), target, rect) for f in F] if i == 0 else
                     [scale_frame(f, W, H, 1, (0, 0, W, H), target) for f in F] if i == 1 else F)
    got, errs = [None] * 3, [None] * 3

    def run(i):
        try:
            got[i], st, _ = _decode(datas[i], **opts[i])
            assert st["placed_frames"] == (10 if i == 0 else 0)
        except Exception as e:          # (reported below, on the main thread)
            errs[i] = e
    ts = [threading.Thread(target=run, args=(i,)) for i in range(3)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for i in range(3):
        assert errs[i] is None, errs[i]
        assert len(got[i]) == len(wants[i]) == 10
        assert got[i] == wants[i], f"handle {i} ({('placed', 'stretched', 'plain')[i]})"


def test_device_output_of_a_placed_frame(oracle):
    """device_output 1: output_frame_device hands out the placed frame in device memory."""
    hip = _hip()
    L = api.lib()
    data, codec, F, W, H = _reference("h264_96x80", oracle)
    rect = fit_rect_ref(W, H, 64, 64)
    want = [place_frame(f, W, H, 1, (0, 0, W, H), (64, 64), rect) for f in F]
    fs, got_frames = 64 * 64 * 3 // 2, []
    with api.JmAmdDec(0, 1, options=dict(device_output=1, target_width=64, target_height=64, fit=1)) as d:
        for nal in api.split_nalus(data) + [None] * 64:
            if api.jm_nvdec_is_exit(d.h):
                break
            _, got = api.jm_nvdec_decode_frame(nal, len(nal) if nal else 0, d.h)
            if not got:
                continue
            assert api.jm_nvdec_stream_info(d.h) == (64, 64)
            dev, ln = C.c_void_p(), C.c_int(0)
            assert L.jm_amddec_output_frame_device(C.byref(dev), C.byref(ln), d.h) == fs and ln.value == fs
            host = np.zeros(fs, np.uint8)
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, fs, 2) == 0
            got_frames.append(host.tobytes())
    assert got_frames == want
