"""Scaled and cropped output on the device (k_scale_pack), bit-exact against the numpy restatement of the resampler R_G applied to the CPU
oracle's unscaled frames (test_scaled_output_host.py): the stand-alone kernel, both codecs end to end, every output route, a resolution
change under a fixed target, and scaled handles in the same batches as unscaled ones."""
import ctypes as C
import threading

import numpy as np
import pytest

from jmcodec_amd import api
from tools import streams
from test_scaled_output_host import _packout_ref, scale_device_cases, scale_frame, scale_frames, split_frame

pytestmark = pytest.mark.gpu


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def test_scale_device_random_geometries():
    """jm_amddec_scale_device alone: 240 seeded random geometries (sizes that are no multiples of 16, both formats, lone_field 0 / 1 / 2, the
    ratio limits 8:1 and 1:4) against R_G of the k_packout restatement."""
    hip = _hip()
    d_src, d_dst = C.c_void_p(), C.c_void_p()
    src_cap, dst_cap = 2048 * 1200 * 3 // 2, 1920 * 1088 * 3 // 2
    assert hip.hipMalloc(C.byref(d_src), src_cap) == 0 and hip.hipMalloc(C.byref(d_dst), dst_cap) == 0
    try:
        for n, W, H, crop, target, pitch, lone, fmt, hs, src in scale_device_cases():
            assert src.size <= src_cap
            out_n = target[0] * target[1] * 3 // 2
            assert out_n <= dst_cap
            assert hip.hipMemcpy(d_src, src.ctypes.data_as(C.c_void_p), src.size, 1) == 0
            assert hip.hipMemset(d_dst, 0xA5, out_n) == 0
            rc = api.scale_device(d_src, pitch, pitch * hs, W, H, crop, target, fmt, d_dst, lone_field=lone)
            assert rc == 0, (n, W, H, crop, target, rc)
            out = np.zeros(out_n, np.uint8)
            assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d_dst, out_n, 2) == 0
            F = _packout_ref(src, pitch, hs, W, H, lone, fmt)
            want = scale_frame(F, W, H, fmt, crop, target)
            assert out.tobytes() == want, f"case {n}: {W}x{H} crop {crop} -> {target} lone {lone} fmt {fmt}"
        # invalid geometries are refused before anything runs
        assert api.scale_device(d_src, 128, 128 * 64, 100, 64, (0, 0, 100, 64), (12, 8), 1, d_dst) == -1          # 100 -> 12: beyond 8:1
        assert api.scale_device(d_src, 128, 128 * 64, 100, 64, (2, 0, 100, 64), (50, 32), 1, d_dst) == -1         # outside the frame
        assert api.scale_device(d_src, 128, 128 * 64, 100, 64, (1, 0, 98, 64), (50, 32), 1, d_dst) == -1          # odd
    finally:
        hip.hipFree(d_src)
        hip.hipFree(d_dst)


def _decode(data, codec=0, fmt=1, **opts):
    with api.JmAmdDec(codec, fmt, options=opts) as d:
        frames = d.decode_stream(data)
        assert d.stat("errors") == 0, api.lib().jm_amddec_last_error(d.h)
        stats = {k: d.stat(k) for k in ("scaled_frames", "lone_fields", "out_width", "out_height")}
        return frames, stats


def _geo(crop, target):
    return dict(crop_x=crop[0], crop_y=crop[1], crop_w=crop[2], crop_h=crop[3], target_width=target[0], target_height=target[1])


def _check(oracle_decode, data, crop, target, codec=0, fmt=1, **opts):
    blob, n, W, H = oracle_decode(data, fmt)
    c = (crop[0], crop[1], crop[2] or W - crop[0], crop[3] or H - crop[1])
    frames, stats = _decode(data, codec, fmt, **_geo(crop, target), **opts)
    want = scale_frames(blob, n, W, H, fmt, c, target)
    assert len(frames) == n
    for i, f in enumerate(frames):
        assert f == want[i], f"frame {i} of {n} differs ({W}x{H} crop {c} -> {target}, fmt {fmt})"
    assert stats["scaled_frames"] == n and (stats["out_width"], stats["out_height"]) == target
    return stats


H264_CASES = {
    "c1_1080p_to_960x540": (streams.config_c1(frames=4), (0, 0, 0, 0), (960, 540)),
    "c1_1080p_to_640x360": (streams.config_c1(frames=3, stream_id=1), (0, 0, 0, 0), (640, 360)),
    "c1_crop_1280x720_at_320_180": (streams.config_c1(frames=3, stream_id=2), (320, 180, 1280, 720), (1280, 720)),
    "upscale_2x": (dict(width=176, height=144, frames=5, gop=5, mode=1, num_ref=2, seed=0x5CA10001), (0, 0, 0, 0), (352, 288)),
    "downscale_8x": (dict(width=704, height=576, frames=3, gop=3, mode=1, seed=0x5CA10002), (0, 0, 0, 0), (88, 72)),
    "high_cabac_ibbp": (dict(width=176, height=144, frames=7, gop=7, mode=1, num_ref=2, seed=0x5CA10003, cabac=1, t8x8=1, bframes=2),
                        (8, 6, 160, 128), (120, 96)),
    "paff": (dict(width=176, height=160, frames=7, gop=7, mode=1, num_ref=2, seed=0x5CA10004, cabac=1, paff=1, bframes=2), (0, 0, 0, 0), (130, 110)),
}


@pytest.mark.parametrize("name,fmt", [(n, 1) for n in sorted(H264_CASES)] + [(n, 0) for n in sorted(H264_CASES) if n == "c1_1080p_to_960x540" or
                                                                                  H264_CASES[n][0]["width"] < 1920])
def test_h264_scaled_end_to_end(oracle, name, fmt):
    kw, crop, target = H264_CASES[name]
    _check(oracle.decode, streams.generate(**kw), crop, target, fmt=fmt)


def test_h264_lone_field_scaled(oracle):
    """A field without its partner (shown with its lines twice) through the resampler: the row mapping happens before the crop."""
    kw = dict(width=96, height=64, frames=4, gop=4, seed=302, paff=2, num_ref=2)
    data = streams.generate(**kw)
    starts = [i for i in range(len(data) - 4) if data[i:i + 4] == b"\0\0\0\1" or (data[i:i + 3] == b"\0\0\1" and data[i - 1:i] != b"\0")]
    both = data[:starts[-1]] + streams.generate(**dict(kw, seed=303, paff=1))
    stats = _check(oracle.decode, both, (4, 2, 90, 60), (60, 34))
    assert stats["lone_fields"] == 1


def test_hevc_c3_prefix_4k_to_1080p():
    data = streams.generate_hevc(**streams.config_c3(frames=3))
    stats = _check(streams.OracleHevc().decode, data, (0, 0, 0, 0), (1920, 1080), codec=1)
    assert stats["scaled_frames"] == 3


@pytest.mark.parametrize("fmt", [1, 0])
def test_hevc_cropped_stream_scaled(fmt):
    """A stream with a conformance window (90x70 of 96x96 coded) cropped and scaled once more."""
    data = streams.generate_hevc(width=90, height=70, frames=5, ctb_log2=5, mode=1, seed=0x5CA10005)
    _check(streams.OracleHevc().decode, data, (6, 4, 78, 60), (104, 46), codec=1, fmt=fmt)


@pytest.mark.parametrize("route", [("JM_AMD_DEC_OUT_FETCH", "1/1"), ("JM_AMD_DEC_OUT_FETCH", "0/1"), ("JM_AMD_DEC_OUT_FETCH", "direct"),
                                   ("JM_AMD_DEC_OUT_PINNED", "1"), ("JM_AMD_DEC_OUT_DIRECT", "1")])
def test_every_output_route(oracle, route, monkeypatch):
    monkeypatch.setenv(*route)
    kw = dict(width=320, height=240, frames=6, gop=6, mode=1, num_ref=2, seed=0x5CA10006)
    _check(oracle.decode, streams.generate(**kw), (10, 6, 300, 220), (200, 150))


def test_device_output_and_argb_of_a_scaled_frame(oracle):
    """device_output: output_frame_device hands out the scaled frame; output_argb_device converts the scaled frame (its numpy restatement)."""
    hip = _hip()
    L = api.lib()
    L.jm_amddec_output_argb_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    data = streams.generate(width=176, height=144, frames=5, gop=5, mode=1, seed=0x5CA10007, cabac=1, t8x8=1)
    crop, (tw, th) = (16, 8, 144, 128), (100, 90)
    for fmt in (1, 0):
        blob, n, W, H = oracle.decode(data, fmt)
        want = scale_frames(blob, n, W, H, fmt, crop, (tw, th))
        fs, pitch = tw * th * 3 // 2, tw * 4 + 64
        d_argb = C.c_void_p()
        assert hip.hipMalloc(C.byref(d_argb), pitch * th) == 0
        try:
            with api.JmAmdDec(0, fmt, options=dict(device_output=1, **_geo(crop, (tw, th)))) as d:
                count = 0
                for nal in api.split_nalus(data) + [None] * 64:
                    if api.jm_nvdec_is_exit(d.h):
                        break
                    _, got = api.jm_nvdec_decode_frame(nal, len(nal) if nal else 0, d.h)
                    if not got:
                        continue
                    assert api.jm_nvdec_stream_info(d.h) == (tw, th)
                    dev, ln = C.c_void_p(), C.c_int(0)
                    assert L.jm_amddec_output_frame_device(C.byref(dev), C.byref(ln), d.h) == fs and ln.value == fs
                    host = np.zeros(fs, np.uint8)
                    assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, fs, 2) == 0
                    assert host.tobytes() == want[count], f"fmt {fmt} frame {count}"
                    assert L.jm_amddec_output_argb_device(d_argb, pitch, d.h) == 0
                    argb = np.zeros(pitch * th, np.uint8)
                    assert hip.hipMemcpy(argb.ctypes.data_as(C.c_void_p), d_argb, pitch * th, 2) == 0
                    argb = argb.reshape(th, pitch)[:, :tw * 4].reshape(th, tw, 4).astype(np.int32)
                    Y, U, V = split_frame(want[count], tw, th, fmt)
                    Y = Y.astype(np.int32)
                    Dc = U.astype(np.int32).repeat(2, 0).repeat(2, 1) - 128
                    Ec = V.astype(np.int32).repeat(2, 0).repeat(2, 1) - 128
                    c = 298 * (Y - 16) + 128
                    R, G, B = np.clip((c + 409 * Ec) >> 8, 0, 255), np.clip((c - 100 * Dc - 208 * Ec) >> 8, 0, 255), np.clip((c + 516 * Dc) >> 8, 0, 255)
                    assert np.array_equal(argb[:, :, 0], B) and np.array_equal(argb[:, :, 1], G) and np.array_equal(argb[:, :, 2], R)
                    assert (argb[:, :, 3] == 255).all()
                    count += 1
                assert count == n
        finally:
            hip.hipFree(d_argb)


def test_resolution_change_under_a_fixed_target(oracle):
    """Three coded video sequences of different sizes, one target: every frame has the target size and is R_G of its own sequence's frame."""
    a = streams.generate(width=96, height=80, frames=5, gop=5, mode=1, seed=1)
    b = streams.generate(width=320, height=240, frames=4, gop=4, mode=1, seed=2)
    c = streams.generate(width=64, height=48, frames=6, gop=6, mode=1, seed=3, bframes=2)
    target = (160, 120)
    want = []
    for x in (a, b, c):
        blob, n, W, H = oracle.decode(x, 1)
        want += scale_frames(blob, n, W, H, 1, (0, 0, W, H), target)
    frames, stats = _decode(a + b + c, target_width=160, target_height=120)
    assert [len(f) for f in frames] == [160 * 120 * 3 // 2] * 15
    assert frames == want
    assert stats["scaled_frames"] == 15


def test_mixed_batches_of_scaled_and_unscaled_handles(oracle):
    """8 handles on 8 threads, every second one scaled: all bit-exact, so k_scale_pack beside k_packout in one batch leaves both alone."""
    datas = [streams.generate(**dict(streams.config_c1(stream_id=i, frames=12, width=352, height=288), seed=0x5CA10100 + i)) for i in range(8)]
    target = (176, 98)
    wants = []
    for i, x in enumerate(datas):
        blob, n, W, H = oracle.decode(x, 1)
        fs = W * H * 3 // 2
        wants.append(scale_frames(blob, n, W, H, 1, (0, 0, W, H), target) if i % 2 else [blob[k * fs:(k + 1) * fs] for k in range(n)])
    got, errs = [None] * 8, [None] * 8

    def run(i):
        try:
            opts = dict(target_width=target[0], target_height=target[1]) if i % 2 else {}
            got[i], _ = _decode(datas[i], **opts)
        except Exception as e:          # (reported below, on the main thread)
            errs[i] = e
    ts = [threading.Thread(target=run, args=(i,)) for i in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for i in range(8):
        assert errs[i] is None, errs[i]
        assert len(got[i]) == len(wants[i]) == 12
        assert got[i] == wants[i], f"handle {i} ({'scaled' if i % 2 else 'unscaled'})"
