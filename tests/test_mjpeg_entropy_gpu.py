"""MJPEG option jpeg_device_entropy on the device: k_jpeg_entropy decodes the restart segments in front of k_jpeg_recon.  Frames are compared bit for
bit with the Python restatement tests/jpeg_ref.py; every case checks through the jpeg_dev_pictures statistic that the device path really ran.  The
damaged streams at the end are the ones tests/test_mjpeg_entropy_host.py has walked on the CPU (and tools/jpeg_entropy_asan.cpp under the sanitizers)."""
import ctypes as C
import threading

import numpy as np
import pytest

import jpeg_ref
from jmcodec_amd import api
from test_mjpeg_entropy_host import Q, damaged_streams, run_beyond_63_stream
from test_mjpeg_gpu import FIXTURES, encoded, fixture
from test_rgb_output_host import rgb_frame
from tools import streams

pytestmark = pytest.mark.gpu


def decode(data, fmt, opt, chunks=None, options=None, rgb=None):
    with api.JmAmdDec(2, fmt, options=dict(options or {}, jpeg_device_entropy=opt), rgb=rgb) as d:
        frames = d.decode_stream(data, chunks=chunks if chunks is not None else [data])
        return frames, dict(errors=d.stat("errors"), dev=d.stat("jpeg_dev_pictures"), host=d.stat("jpeg_host_pictures"), segs=d.stat("jpeg_dev_segments"),
                            damaged=d.stat("jpeg_dev_damaged_segments"))


def exact(data, fmt, opt, n, **kw):
    want = jpeg_ref.decode_stream(data, fmt)
    frames, st = decode(data, fmt, opt, **kw)
    assert (st["errors"], st["dev"], st["host"], st["damaged"]) == (0, n, 0, 0), st
    assert len(frames) == n == len(want)
    for i in range(n):
        assert frames[i] == want[i][0], f"picture {i} fmt {fmt}"
    return st


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_with_every_picture_on_the_device(name, fmt):
    exact(fixture(name), fmt, 2, 1)


@pytest.mark.parametrize("fmt", [0, 1])
def test_restart_fixture_with_option_1(fmt):
    assert exact(fixture("c420_72x40_rst3"), fmt, 1, 1)["segs"] == 5


@pytest.mark.parametrize("w,h,segs", [(128, 32, 64), (104, 40, 65), (136, 40, 85)])
def test_wave_boundaries(w, h, segs):
    """4:4:4, one MCU per segment: exactly one wave, one lane into the second, a partial second wave."""
    assert exact(encoded(21, 0x11, w, h, dri=1), 1, 1, 1)["segs"] == segs


@pytest.mark.parametrize("samp,w,h", [(0x22, 136, 24), (0x21, 200, 16), (0x11, 24, 136)])
def test_partial_strips_with_restart_intervals(samp, w, h):
    exact(encoded(22, samp, w, h, dri=3), 0, 1, 1)


@pytest.mark.parametrize("fmt", [0, 1])
def test_five_pictures_through_split_nalus(fmt):
    data = b"\x00\x00\x01" + encoded(14, 0x22, 320, 240, n=5, dri=7)
    exact(data, fmt, 1, 5, chunks=api.split_nalus(data))


def test_tables_interval_and_size_change_from_picture_to_picture():
    """Snapshot semantics: each picture is decoded with the tables and the interval it was parsed with; a new size starts a new sequence."""
    rng = np.random.default_rng(23)
    lv = jpeg_ref.random_levels(rng, 0x22, 72, 40, density=0.3)
    q2 = [[int(v) for v in rng.integers(1, 30, 64)], Q[1]]
    data = (jpeg_ref.encode(lv, Q, 0x22, 72, 40, dri=2) + jpeg_ref.encode(lv, q2, 0x22, 72, 40, dht=False, dri=4) + jpeg_ref.encode(lv, q2, 0x22, 72, 40, tables=False, dri=1)
            + fixture("c420_64x48_opt") + encoded(24, 0x21, 96, 80, n=2, dri=3) + jpeg_ref.encode(lv, Q, 0x22, 72, 40, dri=15))
    want = jpeg_ref.decode_stream(data, 1)
    frames, st = decode(data, 1, 1)
    assert frames == [f for f, _, _ in want] and len(frames) == 7
    assert (st["errors"], st["dev"], st["host"]) == (0, 5, 2)                   # the optimised fixture has no DRI; dri = 15 is one segment
    exact(data, 1, 2, 7)


def test_mixed_batch_on_the_shared_lane(oracle):
    """A device-path handle, a host-path MJPEG handle and an HEVC handle at once: their pictures share the HEVC lane's batches."""
    dev = encoded(31, 0x22, 160, 120, n=8, dri=5)
    hostp = encoded(32, 0x21, 200, 16, n=8, dri=3)
    hevc = streams.generate_hevc(width=96, height=80, frames=8, gop=4, num_ref=2, seed=0x4A4D0A02)
    w265, n265, _, _ = streams.OracleHevc().decode(hevc, out_fmt=1)
    jobs = [(2, dev, {"jpeg_device_entropy": 1}), (2, hostp, {}), (1, hevc, {}), (2, dev, {"jpeg_device_entropy": 2})]
    got, stats, errs = [None] * len(jobs), [None] * len(jobs), []

    def run(i):
        codec, data, opts = jobs[i]
        try:
            with api.JmAmdDec(codec, 1, options=opts) as d:
                got[i] = d.decode_stream(data, chunks=[data[k:k + 997] for k in range(0, len(data), 997)] if codec == 2 else None)
                stats[i] = (d.stat("errors"), d.stat("jpeg_dev_pictures"), d.stat("jpeg_host_pictures"))
        except Exception as e:          # noqa: BLE001 -- reported below, in the main thread
            errs.append((i, repr(e)))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    assert got[0] == [f for f, _, _ in jpeg_ref.decode_stream(dev, 1)] == got[3]
    assert got[1] == [f for f, _, _ in jpeg_ref.decode_stream(hostp, 1)]
    assert b"".join(got[2]) == w265 and len(got[2]) == n265
    assert stats[0] == (0, 8, 0) and stats[1] == (0, 0, 0) and stats[3] == (0, 8, 0)


def test_device_resident_output():
    data = encoded(15, 0x22, 72, 40, n=3, dri=4)
    F = [f for f, _, _ in jpeg_ref.decode_stream(data, 1)]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L = api.lib()
    got_frames = []
    with api.JmAmdDec(2, 1, options=dict(device_output=1, jpeg_device_entropy=1)) as d:
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
        assert d.stat("jpeg_dev_pictures") == 3
    assert got_frames == F


def test_rgb_route():
    data = encoded(15, 0x22, 72, 40, n=3, dri=4)
    F = [f for f, _, _ in jpeg_ref.decode_stream(data, 1)]
    spec = api.rgb_spec("u8")
    frames, st = decode(data, 1, 1, rgb=spec)
    assert (st["errors"], st["dev"]) == (0, 3)
    assert frames == [rgb_frame(f, 72, 40, 1, (0, 0, 72, 40), (72, 40), spec, 6, True) for f in F]


def test_profile_counts_the_new_kernel_class():
    data = encoded(15, 0x22, 72, 40, n=3, dri=4)
    with api.JmAmdDec(2, 1, options=dict(jpeg_device_entropy=1, profile=1)) as d:
        before = d.stat("k_jpeg_entropy_pics")
        assert len(d.decode_stream(data, chunks=[data])) == 3
        assert d.stat("k_jpeg_entropy_pics") - before == 3 and d.stat("k_jpeg_entropy_n") >= 1
        assert d.stat("k_jpeg_entropy_ns") > 0 and d.stat("k_jpeg_entropy_alg_bytes") > 0


# ---- damage: contained per segment ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["truncated", "invalid_code"])
def test_damaged_segment_is_contained(name):
    """4:4:4 40 x 24, one MCU row per segment, the middle one damaged: luma rows 0-7 and 16-23 and chroma rows 0-3 and 8-11 equal the restatement of
    the undamaged picture; with the invalid code at the segment's first symbol the whole middle band is 128."""
    clean, damaged, seg, _ = damaged_streams()[name]
    want = np.frombuffer(jpeg_ref.decode_stream(clean, 0)[0][0], np.uint8).reshape(36, 40)
    frames, st = decode(b"".join([clean, damaged, clean]), 0, 1)
    assert len(frames) == 3 and (st["errors"], st["dev"], st["damaged"]) == (1, 3, 1), st
    assert frames[0] == want.tobytes() == frames[2]
    got = np.frombuffer(frames[1], np.uint8).reshape(36, 40)
    for rows in (slice(0, 8), slice(16, 24), slice(24, 28), slice(32, 36)):
        assert np.array_equal(got[rows], want[rows])
    if name == "invalid_code":
        assert (got[8:16] == 128).all() and (got[28:32] == 128).all()
    else:
        assert not np.array_equal(got[8:16], want[8:16])


def test_damaged_run_beyond_63_is_contained():
    """Grey 16 x 8, one block per segment: the first is damaged (128), the second decodes (DC -1, +1 at zig-zag position 15, Q = 1)."""
    lv = np.zeros((1, 1, 64), np.int64)
    lv[0, 0, 0], lv[0, 0, jpeg_ref.ZZ[15]] = -1, 1
    block = jpeg_ref.idct_plane(lv, np.ones(64, np.int64))
    frames, st = decode(run_beyond_63_stream(), 0, 1)
    assert len(frames) == 1 and (st["errors"], st["dev"], st["damaged"]) == (1, 1, 1), st
    got = np.frombuffer(frames[0], np.uint8).reshape(12, 16)
    assert (got[:8, :8] == 128).all() and np.array_equal(got[:8, 8:], block) and (got[8:] == 128).all()
