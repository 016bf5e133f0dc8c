"""RGB output on the device (k_rgb_pack), bit-exact against the numpy restatement C(R_G(F)) of test_rgb_output_host.py applied to the CPU
oracle's frames (the oracle decodes the same stream without its colour description, which changes no picture): the stand-alone kernel over
seeded random cases, both codecs end to end, every output route, the device and push / pull interfaces, a stream whose sequences change matrix
and size, RGB handles in the same batches as scaled and plain ones, and the 1 GiB rule of the output slots."""
import ctypes as C
import threading

import numpy as np
import pytest

from jmcodec_amd import api
from tools import streams
from test_rgb_output_host import IMAGENET, rgb_device_cases, rgb_frame
from test_scaled_output_gpu import _hip
from test_scaled_output_host import _packout_ref

pytestmark = pytest.mark.gpu


def test_rgb_device_random_cases():
    """jm_amddec_rgb_device alone: 200 seeded cases (sizes that are no multiples of 16, crops, identity / 8:1 / 1:4 / random targets, lone_field
    0 / 1 / 2, every sample type, layout, order, matrix and range, random surface bytes with 0 and 255) against C(R_G(F))."""
    hip = _hip()
    d_src, d_dst = C.c_void_p(), C.c_void_p()
    src_cap, dst_cap = 400 * 200 * 3 // 2, 3 * 960 * 720 * 4
    assert hip.hipMalloc(C.byref(d_src), src_cap) == 0 and hip.hipMalloc(C.byref(d_dst), dst_cap) == 0
    try:
        for n, spec, W, H, crop, target, pitch, lone, hs, src in rgb_device_cases():
            out_n = 3 * target[0] * target[1] * api.RGB_SAMPLE_BYTES[spec.dtype]
            assert src.size <= src_cap and out_n <= dst_cap
            assert hip.hipMemcpy(d_src, src.ctypes.data_as(C.c_void_p), src.size, 1) == 0
            assert hip.hipMemset(d_dst, 0xA5, out_n) == 0
            rc = api.rgb_device(d_src, pitch, pitch * hs, W, H, crop, target, spec, d_dst, lone_field=lone)
            assert rc == 0, (n, W, H, crop, target, rc)
            out = np.zeros(out_n, np.uint8)
            assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d_dst, out_n, 2) == 0
            want = rgb_frame(_packout_ref(src, pitch, hs, W, H, lone, 1), W, H, 1, crop, target, spec, spec.matrix, spec.range == 2)
            assert out.tobytes() == want, (f"case {n}: {W}x{H} crop {crop} -> {target} lone {lone} dtype {spec.dtype} planar {spec.planar} "
                                           f"bgr {spec.bgr} matrix {spec.matrix} range {spec.range}")
    finally:
        hip.hipFree(d_src)
        hip.hipFree(d_dst)


def _decode(data, spec, codec=0, **opts):
    with api.JmAmdDec(codec, 1, options=opts, rgb=spec) as d:
        frames = d.decode_stream(data)
        assert d.stat("errors") == 0, api.lib().jm_amddec_last_error(d.h)
        stats = {k: d.stat(k) for k in ("rgb_frames", "scaled_frames", "color_matrix", "color_range", "out_frame_bytes", "lone_fields",
                                         "out_slot_bytes")}
        return frames, stats


def _geo(crop, target):
    return dict(crop_x=crop[0], crop_y=crop[1], crop_w=crop[2], crop_h=crop[3], target_width=target[0], target_height=target[1]) if target else {}


def _want(blob, n, W, H, crop, target, spec, matrix, full):
    fs = W * H * 3 // 2
    c = (crop[0], crop[1], crop[2] or W - crop[0], crop[3] or H - crop[1]) if target else (0, 0, W, H)
    t = target or (W, H)
    return [rgb_frame(blob[i * fs:(i + 1) * fs], W, H, 1, c, t, spec, matrix, full) for i in range(n)]


def _check(decode_ref, kw, gen, vui, spec, crop=(0, 0, 0, 0), target=None, codec=0, **opts):
    """Decode gen(**kw, **vui colour parameters) as RGB and compare with C(R_G(F)) of the oracle's frames of gen(**kw)."""
    vkw, matrix, full = VUI[vui]
    blob, n, W, H = decode_ref(gen(**kw), 1)
    if matrix is None:
        matrix = 1 if H > 576 else 6
    frames, stats = _decode(gen(**kw, **vkw), spec, codec, **_geo(crop, target), **opts)
    want = _want(blob, n, W, H, crop, target, spec, matrix, full)
    assert len(frames) == n
    for i, f in enumerate(frames):
        assert f == want[i], f"frame {i} of {n} differs ({W}x{H} crop {crop} -> {target}, matrix {matrix} full {full})"
    assert stats["rgb_frames"] == n and (stats["color_matrix"], stats["color_range"]) == (matrix, 2 if full else 1)
    assert stats["scaled_frames"] == (n if target else 0)
    return stats


VUI = {"709_full": (dict(vui_matrix=1, vui_primaries=1, vui_transfer=1, vui_full_range=1), 1, True),
       "601_limited": (dict(vui_matrix=6, vui_primaries=6, vui_transfer=6), 6, False),
       "none": (dict(), None, False)}
H264 = {"cavlc": dict(width=176, height=144, frames=5, gop=5, mode=1, num_ref=2, seed=0xC0100001),
        "cabac_b": dict(width=176, height=144, frames=7, gop=7, mode=1, num_ref=2, seed=0xC0100002, cabac=1, t8x8=1, bframes=2),
        "paff": dict(width=176, height=160, frames=7, gop=7, mode=1, num_ref=2, seed=0xC0100003, cabac=1, paff=1, bframes=2)}
SPECS = [dict(dtype="f16", **IMAGENET), dict(dtype="u8", planar=False, bgr=True), dict(dtype="f32", planar=True), dict(dtype="bf16", planar=False)]


@pytest.mark.parametrize("stream", sorted(H264))
@pytest.mark.parametrize("vui", sorted(VUI))
@pytest.mark.parametrize("scaled", [False, True])
def test_h264_end_to_end(oracle, stream, vui, scaled):
    spec = api.rgb_spec(**SPECS[(sorted(H264).index(stream) + sorted(VUI).index(vui) + scaled) % 4])
    _check(oracle.decode, H264[stream], streams.generate, vui, spec, (8, 6, 160, 128) if scaled else (0, 0, 0, 0), (100, 70) if scaled else None)


@pytest.mark.parametrize("scaled", [False, True])
def test_h264_lone_field(oracle, scaled):
    """A field without its partner (its lines shown twice) through k_rgb_pack: the row mapping happens before the crop."""
    kw = dict(width=96, height=64, frames=4, gop=4, seed=302, paff=2, num_ref=2)

    def gen(**k):
        data = streams.generate(**dict(kw, **k))
        starts = [i for i in range(len(data) - 4) if data[i:i + 4] == b"\0\0\0\1" or (data[i:i + 3] == b"\0\0\1" and data[i - 1:i] != b"\0")]
        return data[:starts[-1]] + streams.generate(**dict(kw, seed=303, paff=1))
    stats = _check(oracle.decode, {}, gen, "none", api.rgb_spec("f32", planar=False), (4, 2, 90, 60) if scaled else (0, 0, 0, 0),
                   (60, 34) if scaled else None)
    assert stats["lone_fields"] == 1


@pytest.mark.parametrize("vui", sorted(VUI))
@pytest.mark.parametrize("scaled", [False, True])
def test_hevc_end_to_end(vui, scaled):
    """A stream with a conformance window (90x70 of 96x96 coded), unscaled and cropped + scaled."""
    kw = dict(width=90, height=70, frames=5, ctb_log2=5, mode=1, seed=0xC0100005)
    _check(streams.OracleHevc().decode, kw, streams.generate_hevc, vui, api.rgb_spec("bf16", **IMAGENET), (6, 4, 78, 60) if scaled else (0, 0, 0, 0),
           (104, 46) if scaled else None, codec=1)


@pytest.mark.parametrize("route", [("JM_AMD_DEC_OUT_FETCH", "1/1"), ("JM_AMD_DEC_OUT_FETCH", "0/1"), ("JM_AMD_DEC_OUT_FETCH", "direct"),
                                   ("JM_AMD_DEC_OUT_PINNED", "1"), ("JM_AMD_DEC_OUT_DIRECT", "1")])
def test_every_output_route(oracle, route, monkeypatch):
    monkeypatch.setenv(*route)
    kw = dict(width=320, height=240, frames=6, gop=6, mode=1, num_ref=2, seed=0xC0100006)
    _check(oracle.decode, kw, streams.generate, "709_full", api.rgb_spec("f16", **IMAGENET), (10, 6, 300, 220), (224, 224))
    _check(oracle.decode, kw, streams.generate, "601_limited", api.rgb_spec("u8"))


def test_device_output_of_an_rgb_handle(oracle):
    """device_output: output_frame_device hands out the RGB frame; output_argb_device and output_nv12_pitch_device refuse (not Y'CbCr)."""
    hip = _hip()
    L = api.lib()
    L.jm_amddec_output_argb_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.jm_amddec_output_nv12_pitch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    kw = dict(width=176, height=144, frames=5, gop=5, mode=1, seed=0xC0100007, cabac=1, t8x8=1)
    blob, n, W, H = oracle.decode(streams.generate(**kw), 1)
    data = streams.generate(**kw, vui_matrix=1, vui_full_range=1)
    spec = api.rgb_spec("bf16", planar=False, **IMAGENET)
    want = _want(blob, n, W, H, (0, 0, 0, 0), None, spec, 1, True)
    fs = 3 * W * H * 2
    d_buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_buf), W * H * 4 + 4096) == 0
    try:
        with api.JmAmdDec(0, 1, options=dict(device_output=1), rgb=spec) as d:
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
                assert L.jm_amddec_output_argb_device(d_buf, W * 4, d.h) == -1
                assert L.jm_amddec_output_nv12_pitch_device(d_buf, W, d.h) == -1
                count += 1
            assert count == n
    finally:
        hip.hipFree(d_buf)


@pytest.mark.parametrize("callback", [False, True])
def test_push_pull_facade(oracle, monkeypatch, callback):
    """jm_intel_dec_*: a spec set through jm_amdintel_decoder before init; frames through output_frame (sized from out_frame_bytes) or the
    callback."""
    kw = dict(width=320, height=240, frames=6, gop=6, mode=1, num_ref=2, seed=0xC0100008)
    blob, n, W, H = oracle.decode(streams.generate(**kw), 1)
    spec = api.rgb_spec("f32", planar=True)
    init = api.jm_intel_dec_init

    def init_rgb(codec, fmt, h):
        assert api.set_rgb(api.lib().jm_amdintel_decoder(h), spec) == 0
        return init(codec, fmt, h)
    monkeypatch.setattr(api, "jm_intel_dec_init", init_rgb)
    frames, info, _, _ = api.intel_push_pull(streams.generate(**kw, vui_matrix=5), callback=callback)
    assert frames == _want(blob, n, W, H, (0, 0, 0, 0), None, spec, 5, False)
    assert "RGB planar f32" in info


def test_each_frame_uses_its_own_sequence_colour(oracle):
    """Four coded video sequences: another matrix at the same size (the frames the IDR picture flushes keep the old one), then other sizes."""
    parts = [(dict(width=96, height=80, frames=6, gop=6, mode=1, seed=11, bframes=2, poc_type=0, num_ref=2), dict(vui_matrix=1, vui_full_range=1), 1, True),
             (dict(width=96, height=80, frames=5, gop=5, mode=1, seed=12, bframes=2, poc_type=0, num_ref=2), dict(vui_matrix=9), 9, False),
             (dict(width=160, height=96, frames=4, gop=4, mode=1, seed=13), dict(vui_matrix=4, vui_full_range=1), 4, True),
             (dict(width=64, height=48, frames=3, gop=3, mode=1, seed=14), dict(), 6, False)]
    spec = api.rgb_spec("f16", planar=False)
    want, data = [], b""
    for kw, vkw, matrix, full in parts:
        blob, n, W, H = oracle.decode(streams.generate(**kw), 1)
        want += _want(blob, n, W, H, (0, 0, 0, 0), None, spec, matrix, full)
        data += streams.generate(**kw, **vkw)
    frames, stats = _decode(data, spec)
    assert len(frames) == len(want) == 18
    for i, f in enumerate(frames):
        assert f == want[i], f"frame {i}"
    assert stats["rgb_frames"] == 18 and stats["color_matrix"] == 6


def _push_whole(data, codec, spec):
    """The whole stream in one jm_amddec_push_data call (the front end runs as far ahead of the parse workers as the job slots allow), then end of
    stream and every frame taken with decode_frame(NULL, 0)."""
    L = api.lib()
    L.jm_amddec_push_eos.argtypes = [C.c_void_p]
    frames = []
    with api.JmAmdDec(codec, 1, rgb=spec) as d:
        buf = C.create_string_buffer(data, len(data))
        assert L.jm_amddec_push_data(C.cast(buf, C.c_void_p), len(data), d.h) == 0
        assert L.jm_amddec_push_eos(d.h) == 0
        while not api.jm_nvdec_is_exit(d.h):
            ret, got = api.jm_nvdec_decode_frame(None, 0, d.h)
            assert ret == 0, api.lib().jm_amddec_last_error(d.h)
            if got == 1:
                out = C.create_string_buffer(d.stat("out_frame_bytes"))
                _, n = api.jm_nvdec_output_frame(out, len(out), d.h)
                frames.append(out.raw[:n])
        assert d.stat("errors") == 0
    return frames


@pytest.mark.parametrize("codec", [0, 1])
def test_same_size_colour_change_keeps_the_flushed_frames_colour(oracle, codec):
    """Two sequences of one size with different matrices and ranges, the whole stream pushed at once: the frames the second sequence's IDR picture
    flushes out of the DPB keep the first sequence's colour although the second sequence's pictures reuse their surfaces (24 pictures > 18
    surfaces) before that IDR picture reaches the device."""
    if codec == 0:
        gen, ref = streams.generate, oracle.decode
        parts = [dict(width=96, height=64, frames=8, gop=8, mode=1, seed=21, bframes=2, poc_type=0, num_ref=2),
                 dict(width=96, height=64, frames=24, gop=24, mode=1, seed=22, bframes=2, poc_type=0, num_ref=2)]
    else:
        gen, ref = streams.generate_hevc, streams.OracleHevc().decode
        parts = [dict(width=96, height=64, frames=9, gop=8, num_ref=2, ctb_log2=5, mode=1, seed=23),
                 dict(width=96, height=64, frames=24, gop=8, num_ref=2, ctb_log2=5, mode=1, seed=24)]
    colours = [(dict(vui_matrix=1, vui_full_range=1), 1, True), (dict(vui_matrix=9), 9, False)]
    spec = api.rgb_spec("u8")
    want, data = [], b""
    for kw, (vkw, matrix, full) in zip(parts, colours):
        blob, n, W, H = ref(gen(**kw), 1)
        want += _want(blob, n, W, H, (0, 0, 0, 0), None, spec, matrix, full)
        data += gen(**kw, **vkw)
    frames = _push_whole(data, codec, spec)
    assert len(frames) == len(want) == parts[0]["frames"] + 24
    for i, f in enumerate(frames):
        assert f == want[i], f"frame {i}"


def test_mixed_batches_of_rgb_scaled_and_plain_handles(oracle):
    """9 handles on 9 threads: plain NV12, scaled NV12 and RGB (unscaled and scaled) side by side -- all exact, the Y'CbCr handles byte-identical
    to the oracle's frames or R_G of them."""
    from test_scaled_output_host import scale_frames
    datas = [streams.generate(**dict(streams.config_c1(stream_id=i, frames=10, width=352, height=288), seed=0xC0100100 + i)) for i in range(9)]
    target, spec = (176, 98), api.rgb_spec("f16", **IMAGENET)
    kinds = ["plain", "scaled", "rgb", "plain", "scaled", "rgb_scaled", "rgb", "scaled", "rgb_scaled"]
    wants = []
    for i, x in enumerate(datas):
        blob, n, W, H = oracle.decode(x, 1)
        fs = W * H * 3 // 2
        k = kinds[i]
        wants.append([blob[j * fs:(j + 1) * fs] for j in range(n)] if k == "plain" else scale_frames(blob, n, W, H, 1, (0, 0, W, H), target)
                     if k == "scaled" else _want(blob, n, W, H, (0, 0, 0, 0), target if k == "rgb_scaled" else None, spec, 6, False))
    got, errs = [None] * 9, [None] * 9

    def run(i):
        try:
            k = kinds[i]
            opts = dict(target_width=target[0], target_height=target[1]) if k in ("scaled", "rgb_scaled") else {}
            with api.JmAmdDec(0, 1, options=opts, rgb=spec if k.startswith("rgb") else None) as d:
                got[i] = d.decode_stream(datas[i])
        except Exception as e:          # (reported below, on the main thread)
            errs[i] = e
    ts = [threading.Thread(target=run, args=(i,)) for i in range(9)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for i in range(9):
        assert errs[i] is None, errs[i]
        assert len(got[i]) == len(wants[i]) == 10
        assert got[i] == wants[i], f"handle {i} ({kinds[i]})"


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_f32_handles_keep_the_output_slots_within_1_gib(oracle, w, h):
    kw = dict(width=w, height=h, frames=2, gop=2, mode=1, seed=0xC0100200, level_idc=51)
    data = streams.generate(**kw)
    spec = api.rgb_spec("f32")
    frames, stats = _decode(data, spec)
    fb = 3 * w * h * 4
    assert stats["out_frame_bytes"] == fb and 0 < stats["out_slot_bytes"] <= max(1 << 30, 12 * fb)
    blob, n, W, H = oracle.decode(data, 1)
    assert frames == _want(blob, n, W, H, (0, 0, 0, 0), None, spec, 1, False)
