"""Interpolated chroma of the RGB output on the device (k_rgb_pack444, options rgb_chroma / chroma_loc), bit-exact against the numpy restatement
C(G') of test_rgb_chroma_host.py: the stand-alone kernel over the seeded cases, then end to end on the CPU oracle's frames (the oracle decodes the
same stream without its chroma location, which changes no picture) -- both H.264 entropy coders, a deinterlaced PAFF stream, a letterboxed HEVC
stream, an MJPEG 4:2:2 fixture, a stream whose second sequence changes size and location -- and handles with and without the option in the same
batches."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import jpeg_ref
from jmcodec_amd import api
from tools import streams
from test_deinterlace_gpu import PAFF_176, _gen as paff_gen, _want as deint_want
from test_placed_output_host import fit_rect_ref
from test_rgb_chroma_host import case_want, chroma_device_cases, describe, rgb_chroma_frame
from test_rgb_output_host import IMAGENET, rgb_frame
from test_scaled_output_gpu import _hip

pytestmark = pytest.mark.gpu


def test_rgb_chroma_device_seeded_cases():
    """jm_amddec_rgb_chroma_device alone: the 156 seeded cases of the CPU walk (sources <= 400 x 200, targets <= 960 x 720) into a buffer preset to
    0xA5, byte-equal to C(G'); the bytes behind the frame stay."""
    hip = _hip()
    d_src, d_dst = C.c_void_p(), C.c_void_p()
    src_cap, dst_cap, guard = 512 * 216 * 3 // 2, 3 * 960 * 720 * 4, 256          # (a surface: up to 112 bytes of pitch padding, 16 more rows)
    assert hip.hipMalloc(C.byref(d_src), src_cap) == 0 and hip.hipMalloc(C.byref(d_dst), dst_cap + guard) == 0
    count = 0
    try:
        for case in chroma_device_cases():
            n, spec, W, H, crop, target, rect, fill, loc, pitch, lone, hs, src = case
            out_n = 3 * target[0] * target[1] * api.RGB_SAMPLE_BYTES[spec.dtype]
            assert src.size <= src_cap and out_n <= dst_cap, describe(*case)
            assert hip.hipMemcpy(d_src, src.ctypes.data_as(C.c_void_p), src.size, 1) == 0
            assert hip.hipMemset(d_dst, 0xA5, out_n + guard) == 0
            rc = api.rgb_chroma_device(d_src, pitch, pitch * hs, W, H, crop, target, spec, d_dst, loc, rect=rect or (0, 0, 0, 0), fill=fill, lone_field=lone)
            assert rc == 0, (rc, describe(*case))
            out = np.zeros(out_n + guard, np.uint8)
            assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d_dst, out_n + guard, 2) == 0
            assert out[:out_n].tobytes() == case_want(*case[1:]), describe(*case)
            assert (out[out_n:] == 0xA5).all(), describe(*case)
            count += 1
    finally:
        hip.hipFree(d_src)
        hip.hipFree(d_dst)
    assert count == 156


# ---- through the decoder --------------------------------------------------------------------------------------------------------
STATS = ("rgb_chroma_frames", "chroma_loc", "rgb_frames", "vui_chroma_loc", "rgb_chroma", "errors")


def _decode(data, spec, codec=0, chunks=None, **opts):
    with api.JmAmdDec(codec, 1, options=opts, rgb=spec) as d:
        frames = d.decode_stream(data, chunks=chunks)
        assert d.stat("errors") == 0, api.lib().jm_amddec_last_error(d.h)
        return frames, {k: d.stat(k) for k in STATS}


def _frames_of(blob, n, W, H):
    fs = W * H * 3 // 2
    return [blob[i * fs:(i + 1) * fs] for i in range(n)]


def _check(data, F, W, H, spec, loc, matrix, full, crop=None, target=None, rect=None, fill_rgb=(0, 0, 0), codec=0, chunks=None, **opts):
    """Decode `data` with rgb_chroma 1 and compare with C(G') of the frames F; the same stream with rgb_chroma 0 must give other bytes (a coloured
    stream) of the same size, through none of the new kernel's frames."""
    crop, target = crop or (0, 0, W, H), target or (W, H)
    frames, st = _decode(data, spec, codec, chunks, rgb_chroma=1, **opts)
    want = [rgb_chroma_frame(f, W, H, crop, target, spec, matrix, full, loc, rect, fill_rgb) for f in F]
    assert len(frames) == len(want)
    for i, f in enumerate(frames):
        assert f == want[i], f"frame {i} of {len(want)} differs ({W}x{H} crop {crop} -> {target} rect {rect} loc {loc})"
    assert (st["rgb_chroma_frames"], st["chroma_loc"], st["rgb_frames"], st["rgb_chroma"]) == (len(F), loc, len(F), 1)
    plain, st0 = _decode(data, spec, codec, chunks, **opts)
    assert (st0["rgb_chroma_frames"], st0["rgb_frames"], st0["rgb_chroma"]) == (0, len(F), 0)
    assert [len(f) for f in plain] == [len(f) for f in frames] and all(a != b for a, b in zip(plain, frames))
    return frames, plain, st


def _geo(crop, target):
    return dict(crop_x=crop[0], crop_y=crop[1], crop_w=crop[2], crop_h=crop[3], target_width=target[0], target_height=target[1])


def test_h264_cavlc_identity_geometry_loc0(oracle):
    kw = dict(width=176, height=144, frames=5, gop=5, mode=1, num_ref=2, seed=0xC4120001)
    blob, n, W, H = oracle.decode(streams.generate(**kw), 1)
    spec = api.rgb_spec("u8", planar=True)
    _, plain, st = _check(streams.generate(**kw, vui_chroma_loc=0), _frames_of(blob, n, W, H), W, H, spec, 0, 6, False)
    assert st["vui_chroma_loc"] == 0
    # ... and rgb_chroma 0 is C(R_G(F)), as before
    assert plain == [rgb_frame(f, W, H, 1, (0, 0, W, H), (W, H), spec, 6, False) for f in _frames_of(blob, n, W, H)]


def test_h264_cabac_b_cropped_and_scaled_loc2(oracle):
    kw = dict(width=176, height=144, frames=7, gop=7, mode=1, num_ref=2, seed=0xC4120002, cabac=1, t8x8=1, bframes=2)
    blob, n, W, H = oracle.decode(streams.generate(**kw), 1)
    crop, target = (8, 6, 160, 128), (100, 70)
    _check(streams.generate(**kw, vui_chroma_loc=2, vui_matrix=1, vui_primaries=1, vui_transfer=1, vui_full_range=1), _frames_of(blob, n, W, H), W, H,
           api.rgb_spec("f16", **IMAGENET), 2, 1, True, crop, target, **_geo(crop, target))


def test_h264_paff_deinterlaced_loc1(oracle):
    """C(G'(D(F))): the frame's siting is applied to the deinterlaced frame."""
    data, fields = paff_gen(dict(PAFF_176, vui_chroma_loc=1))
    blob, n, W, H = oracle.decode(streams.generate(**PAFF_176), 1)
    D = deint_want(blob, n, W, H, 1, 1, fields)
    _check(data, D, W, H, api.rgb_spec("bf16", planar=False), 1, 6, False, deinterlace=1)


def test_hevc_letterboxed_loc3():
    kw = dict(width=90, height=70, frames=5, ctb_log2=5, mode=1, seed=0xC0100005)
    blob, n, W, H = streams.OracleHevc().decode(streams.generate_hevc(**kw), 1)
    rect = fit_rect_ref(W, H, 96, 96)
    _check(streams.generate_hevc(**kw, vui_chroma_loc=3), _frames_of(blob, n, W, H), W, H, api.rgb_spec("f32", planar=True, bgr=True), 3, 6, False,
           (0, 0, W, H), (96, 96), rect, (0x20, 0x40, 0x60), codec=1, target_width=96, target_height=96, fit=1, fill=0x204060)


def test_mjpeg_422_fixture_auto_location_is_one():
    data = open(os.path.join(jpeg_ref.GOLDEN_JPEG, "c422_48x32.jpg"), "rb").read()
    F = [f for f, _, _ in jpeg_ref.decode_stream(data, 1)]
    _, _, st = _check(data, F, 48, 32, api.rgb_spec("u8", planar=False), 1, 6, True, codec=2, chunks=[data])          # JFIF: BT.601, full range
    assert st["vui_chroma_loc"] == -1


def test_second_sequence_changes_size_and_location(oracle):
    parts = [(dict(width=96, height=80, frames=6, gop=6, mode=1, seed=31, bframes=2, poc_type=0, num_ref=2), 0),
             (dict(width=160, height=96, frames=4, gop=4, mode=1, seed=32), 5),
             (dict(width=160, height=96, frames=3, gop=3, mode=1, seed=33), 2)]          # ... and the location alone
    spec = api.rgb_spec("u8")
    want, data = [], b""
    for kw, loc in parts:
        blob, n, W, H = oracle.decode(streams.generate(**kw), 1)
        want += [rgb_chroma_frame(f, W, H, (0, 0, W, H), (W, H), spec, 6, False, loc) for f in _frames_of(blob, n, W, H)]
        data += streams.generate(**kw, vui_chroma_loc=loc)
    frames, st = _decode(data, spec, rgb_chroma=1)
    assert len(frames) == len(want) == 13
    for i, f in enumerate(frames):
        assert f == want[i], f"frame {i}"
    assert (st["rgb_chroma_frames"], st["chroma_loc"], st["rgb_frames"]) == (13, 2, 13)


def test_forced_location_overrides_the_stream(oracle):
    kw = dict(width=96, height=80, frames=3, gop=3, mode=1, seed=34)
    blob, n, W, H = oracle.decode(streams.generate(**kw), 1)
    spec = api.rgb_spec("u8")
    frames, st = _decode(streams.generate(**kw, vui_chroma_loc=2), spec, rgb_chroma=1, chroma_loc=4)
    assert frames == [rgb_chroma_frame(f, W, H, (0, 0, W, H), (W, H), spec, 6, False, 4) for f in _frames_of(blob, n, W, H)]
    assert (st["vui_chroma_loc"], st["chroma_loc"]) == (2, 4)


def test_rgb_chroma_zero_and_chroma_loc_alone_change_no_byte(oracle):
    """A handle with rgb_chroma 0, and one with only chroma_loc, hand out the bytes of a handle that never heard of either option."""
    kw = dict(width=176, height=144, frames=4, gop=4, mode=1, num_ref=2, seed=0xC4120003)
    data = streams.generate(**kw, vui_chroma_loc=3)
    spec = api.rgb_spec("f16", **IMAGENET)
    geo = _geo((8, 6, 160, 128), (100, 70))
    base, st = _decode(data, spec, **geo)
    assert _decode(data, spec, rgb_chroma=0, **geo)[0] == base
    assert _decode(data, spec, chroma_loc=5, **geo)[0] == base
    assert st["rgb_chroma_frames"] == 0
    blob, n, W, H = oracle.decode(streams.generate(**kw), 1)
    assert base == [rgb_frame(f, W, H, 1, (8, 6, 160, 128), (100, 70), spec, 6, False) for f in _frames_of(blob, n, W, H)]


def test_mixed_batches_of_chroma_nearest_and_plain_handles(oracle):
    """9 handles on 9 threads in the same batches: rgb_chroma 1 (identity geometry and scaled), rgb_chroma 0 and plain NV12 -- each gets its own
    bytes."""
    datas = [streams.generate(**dict(streams.config_c1(stream_id=i, frames=8, width=352, height=288), seed=0xC4120100 + i), vui_chroma_loc=i % 6)
             for i in range(9)]
    plain_datas = [streams.generate(**dict(streams.config_c1(stream_id=i, frames=8, width=352, height=288), seed=0xC4120100 + i)) for i in range(9)]
    target, spec = (176, 98), api.rgb_spec("f16", **IMAGENET)
    kinds = ["chroma", "nearest", "plain", "chroma_scaled", "nearest_scaled", "plain", "chroma", "chroma_scaled", "nearest"]
    wants = []
    for i in range(9):
        blob, n, W, H = oracle.decode(plain_datas[i], 1)
        F, k = _frames_of(blob, n, W, H), kinds[i]
        t = target if k.endswith("scaled") else (W, H)
        wants.append(F if k == "plain" else [rgb_chroma_frame(f, W, H, (0, 0, W, H), t, spec, 6, False, i % 6) for f in F] if k.startswith("chroma")
                     else [rgb_frame(f, W, H, 1, (0, 0, W, H), t, spec, 6, False) for f in F])
    got, errs = [None] * 9, [None] * 9

    def run(i):
        try:
            k = kinds[i]
            opts = dict(target_width=target[0], target_height=target[1]) if k.endswith("scaled") else {}
            if k.startswith("chroma"):
                opts["rgb_chroma"] = 1
            with api.JmAmdDec(0, 1, options=opts, rgb=None if k == "plain" else spec) as d:
                got[i] = d.decode_stream(datas[i])
        except Exception as e:          # (reported below, on the main thread)
            errs[i] = e
    ts = [threading.Thread(target=run, args=(i,)) for i in range(9)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for i in range(9):
        assert errs[i] is None, errs[i]
        assert len(got[i]) == len(wants[i]) == 8
        assert got[i] == wants[i], f"handle {i} ({kinds[i]})"
