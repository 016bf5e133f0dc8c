"""MJPEG decode (codec_type 2) on the device: k_jpeg_recon against the Python restatement tests/jpeg_ref.py, bit for bit -- the Pillow-encoded fixtures
of tests/golden/jpeg/ and streams of the test encoder at sizes that exercise partial strips -- and every output route behind it (scale, RGB,
deinterlace, device_output), a size change, mixed batches with H.264 and HEVC handles on the shared lane, and a truncated last picture."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import jpeg_ref
from deint_ref import deint_frame
from jmcodec_amd import api
from test_rgb_output_host import rgb_frame
from test_scaled_output_host import scale_frame
from tools import streams

pytestmark = pytest.mark.gpu

FIXTURES = ["g_8x8", "c420_16x16", "c420_53x37", "c420_72x40_rst3", "c422_48x32", "c444_40x24", "c444_53x37", "c420_64x48_opt", "c420_32x32_q1", "g_37x21"]


def fixture(name):
    return open(os.path.join(jpeg_ref.GOLDEN_JPEG, name + ".jpg"), "rb").read()


def _q(rng):
    return [[int(v) for v in rng.integers(1, 64, 64)] for _ in range(2)]


def encoded(seed, sampling, w, h, n=1, dri=0, **kw):
    rng = np.random.default_rng(seed)
    return b"".join(jpeg_ref.encode(jpeg_ref.random_levels(rng, sampling, w, h, density=0.25, amp=60, dc_amp=300), _q(rng), sampling, w, h, dri=dri, **kw)
                    for _ in range(n))


def decode(data, fmt, chunks=None, options=None, rgb=None):
    with api.JmAmdDec(2, fmt, options=options, rgb=rgb) as d:
        frames = d.decode_stream(data, chunks=chunks if chunks is not None else [data])
        return frames, d.stat("errors")


@pytest.fixture(scope="module")
def strip_streams():
    """Sizes at which the strips of k_jpeg_recon are partial: 136x24 4:2:0 (17 luma blocks per row: one full strip and one block; 8.5 chroma blocks),
    200x16 4:2:2, 24x136 4:4:4 (many rows of a short strip), each with its restatement frames for both output formats."""
    out = {}
    for name, (seed, samp, w, h) in {"420_136x24": (11, 0x22, 136, 24), "422_200x16": (12, 0x21, 200, 16), "444_24x136": (13, 0x11, 24, 136)}.items():
        data = encoded(seed, samp, w, h)
        out[name] = (data, {fmt: jpeg_ref.decode_stream(data, fmt) for fmt in (0, 1)})
    return out


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_bit_exact(name, fmt):
    data = fixture(name)
    want = jpeg_ref.decode_stream(data, fmt)
    frames, errors = decode(data, fmt)
    assert errors == 0 and len(frames) == 1
    assert frames[0] == want[0][0], f"{name} fmt {fmt}"


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", ["420_136x24", "422_200x16", "444_24x136"])
def test_partial_strips_bit_exact(strip_streams, name, fmt):
    data, want = strip_streams[name]
    frames, errors = decode(data, fmt)
    assert errors == 0 and len(frames) == 1
    assert frames[0] == want[fmt][0][0], f"{name} fmt {fmt}"


@pytest.mark.parametrize("fmt", [0, 1])
def test_five_pictures_with_restart_interval_through_split_nalus(fmt):
    """The reference harness cuts its input at H.264 start codes, i.e. anywhere for JPEG data (and drops what precedes the first one: the stream gets a
    start code in front, which the decoder skips as bytes between pictures)."""
    data = b"\x00\x00\x01" + encoded(14, 0x22, 320, 240, n=5, dri=7)
    want = jpeg_ref.decode_stream(data, fmt)
    frames, errors = decode(data, fmt, chunks=api.split_nalus(data))
    assert errors == 0 and len(frames) == 5 == len(want)
    for i in range(5):
        assert frames[i] == want[i][0], f"picture {i} fmt {fmt}"


@pytest.fixture(scope="module")
def comp_stream():
    data = encoded(15, 0x22, 72, 40, n=3, dri=4)
    return data, [f for f, _, _ in jpeg_ref.decode_stream(data, 1)]


def test_composition_scale(comp_stream):
    data, F = comp_stream
    frames, _ = decode(data, 1, options=dict(target_width=36, target_height=20))
    assert frames == [scale_frame(f, 72, 40, 1, (0, 0, 72, 40), (36, 20)) for f in F]


@pytest.mark.parametrize("dtype", ["u8", "f16"])
def test_composition_rgb_auto_matrix_is_bt601_full(comp_stream, dtype):
    data, F = comp_stream
    spec = api.rgb_spec(dtype)
    with api.JmAmdDec(2, 1, rgb=spec) as d:
        frames = d.decode_stream(data, chunks=[data])
        assert (d.stat("color_matrix"), d.stat("color_range")) == (6, 2)
    assert frames == [rgb_frame(f, 72, 40, 1, (0, 0, 72, 40), (72, 40), spec, 6, True) for f in F]


def test_composition_deinterlace_on_request(comp_stream):
    data, F = comp_stream
    frames, _ = decode(data, 1, options=dict(deinterlace=1, deinterlace_when=1))
    assert frames == [deint_frame(f, 72, 40, 1, 1, 0) for f in F]
    plain, _ = decode(data, 1, options=dict(deinterlace=1))                   # auto: never for JPEG
    assert plain == F


def test_device_output_route(comp_stream):
    data, F = comp_stream
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L = api.lib()
    got_frames = []
    with api.JmAmdDec(2, 1, options=dict(device_output=1)) as d:
        for chunk in [data] + [None] * 64:
            if api.jm_nvdec_is_exit(d.h):
                break
            _, got = api.jm_nvdec_decode_frame(chunk, len(chunk) if chunk else 0, d.h)
            if not got:
                continue
            dev, ln = C.c_void_p(), C.c_int(0)
            assert L.jm_amddec_output_frame_device(C.byref(dev), C.byref(ln), d.h) == 72 * 40 * 3 // 2
            host = np.zeros(ln.value, np.uint8)
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, ln.value, 2) == 0
            got_frames.append(host.tobytes())
    assert got_frames == F


def test_size_change_mid_stream():
    data = encoded(16, 0x22, 64, 48, n=2) + encoded(17, 0x21, 96, 80, n=2, dri=3)
    want = jpeg_ref.decode_stream(data, 1)
    assert [(w, h) for _, w, h in want] == [(64, 48)] * 2 + [(96, 80)] * 2
    frames, errors = decode(data, 1)
    assert errors == 0 and frames == [f for f, _, _ in want]


def test_eight_handles_beside_h264_and_hevc(oracle):
    """Eight codec-2 handles of different sizes and samplings, one H.264 and one HEVC handle, all decoding at once: MJPEG pictures share the HEVC lane's
    batches.  Every frame of every handle is exact."""
    cases = [(0x22, 136, 24), (0x21, 200, 16), (0x11, 24, 136), (0x10, 33, 17), (0x22, 53, 37), (0x21, 48, 32), (0x11, 53, 37), (0x22, 160, 120)]
    jobs = []
    for i, (samp, w, h) in enumerate(cases):
        data = encoded(100 + i, samp, w, h, n=6, dri=(0, 3, 5)[i % 3])
        jobs.append((2, data, [data[k:k + 997] for k in range(0, len(data), 997)], [f for f, _, _ in jpeg_ref.decode_stream(data, 1)]))
    h264 = streams.generate(width=96, height=80, frames=8, gop=4, mode=1, num_ref=2, seed=0x4A4D0A01)
    jobs.append((0, h264, None, None))
    hevc = streams.generate_hevc(width=96, height=80, frames=8, gop=4, num_ref=2, seed=0x4A4D0A02)
    jobs.append((1, hevc, None, None))
    w264, n264, _, _ = oracle.decode(h264, out_fmt=1)
    w265, n265, _, _ = streams.OracleHevc().decode(hevc, out_fmt=1)
    got = [None] * len(jobs)
    errs = []

    def run(i):
        codec, data, chunks, _ = jobs[i]
        try:
            with api.JmAmdDec(codec, 1) as d:
                got[i] = d.decode_stream(data, chunks=chunks)
        except Exception as e:          # noqa: BLE001 -- reported below, in the main thread
            errs.append((i, repr(e)))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i in range(8):
        assert got[i] == jobs[i][3], f"MJPEG handle {i}: {cases[i]}"
    assert b"".join(got[8]) == w264 and len(got[8]) == n264
    assert b"".join(got[9]) == w265 and len(got[9]) == n265


def test_truncated_last_picture():
    """Host-parser behaviour on bad input: the earlier frames are exact, the damaged picture is still handed out, the handle finishes."""
    data = encoded(18, 0x22, 72, 40, n=4, dri=0)
    pics = jpeg_ref.split_pictures(data)
    cut = data[:len(data) - len(pics[-1]) // 2]
    want = jpeg_ref.decode_stream(data, 1)
    frames, errors = decode(cut, 1)
    assert errors > 0 and len(frames) == 4
    assert frames[:3] == [f for f, _, _ in want[:3]]
    assert len(frames[3]) == 72 * 40 * 3 // 2
