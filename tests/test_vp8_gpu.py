"""VP8 key-frame decode (codec_type 5) on the device: k_vp8_recon and k_vp8_filter, bit for bit in both output formats, against

  * libwebp's own planes for the committed fixtures (tests/golden/vp8: encoded by libwebp, decoded by libwebp's WebPDecodeYUV) -- no Pillow here;
  * the Python restatement tests/vp8_ref.py (itself equal to libwebp on every fixture: tests/test_vp8_host.py) for the scripted streams of
    tests/scripted_vp8.py: the sizes at which the wavefront has one macroblock, one row, a second band of rows, and live left / above-right
    neighbours in it; one stream per syntax feature; damaged streams; a size change; more pictures than a batch; the output routes behind the
    decoder; a mixed batch with the other four codecs.

Every case fails without the feature: option vp8 does not exist and init(5) is refused."""
import ctypes as C
import glob
import os
import threading

import numpy as np
import pytest

import jpeg_ref
import mpeg2_ref
import scripted_mpeg2
import scripted_vp8 as S
import vp8_ref
from jmcodec_amd import api
from test_rgb_output_host import rgb_frame
from test_scaled_output_host import scale_frame
from tools import streams

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vp8")
FIXTURES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLDEN, "*.webp")))
_FEATURES = dict(S.feature_cases())
_DAMAGED = dict(S.damaged_cases())
_REF = {}


def ref(key, data, fmt, info=None):
    """the restatement's frames, computed once per stream and format"""
    if (key, fmt) not in _REF:
        i = {}
        _REF[(key, fmt)] = (vp8_ref.decode_stream(data, fmt, i), i)
    if info is not None:
        info.update(_REF[(key, fmt)][1])
    return _REF[(key, fmt)][0]


def decode(data, fmt, chunks=None, options=None, rgb=None, stats=()):
    with api.JmAmdDec(5, fmt, options=dict(options or {}, vp8=1), rgb=rgb) as d:
        frames = d.decode_stream(data, chunks=chunks if chunks is not None else [data])
        return frames, {k: d.stat(k) for k in ("errors", "frames", "vp8_key_frames") + tuple(stats)}


def check_both_formats(key, data, chunks=None, errors=False):
    info = {}
    for fmt in (0, 1):
        want = ref(key, data, fmt, info)
        frames, st = decode(data, fmt, chunks=chunks)
        assert len(frames) == len(want) == st["frames"]
        for i, (f, w) in enumerate(zip(frames, want)):
            assert f == w[0], f"frame {i} of {len(want)}, out_fmt {fmt}"
        assert (st["errors"] > 0) == errors and st["vp8_key_frames"] == info["key_frames"]
    return info


def test_fixtures_exist():
    assert len(FIXTURES) >= 12


@pytest.mark.parametrize("name", FIXTURES)
def test_libwebp_fixture_bit_exact(name):
    """the product's frames = the planes libwebp decoded, cropped to them (an odd size is handed out as the even size just above)"""
    with open(os.path.join(GOLDEN, name + ".webp"), "rb") as f:
        data = api.webp_to_ivf(f.read())
    Y, U, V = (np.load(os.path.join(GOLDEN, "%s.%s.npy" % (name, p))) for p in "yuv")
    h, w = Y.shape
    dw, dh = (w + 1) & ~1, (h + 1) & ~1
    for fmt in (0, 1):
        frames, st = decode(data, fmt)
        assert len(frames) == 1 and st["errors"] == 0 and len(frames[0]) == dw * dh * 3 // 2
        f = np.frombuffer(frames[0], np.uint8)
        y = f[:dw * dh].reshape(dh, dw)
        if fmt == 0:
            c = f[dw * dh:].reshape(dh // 2, dw)
            u, v = c[:, 0::2], c[:, 1::2]
        else:
            u, v = f[dw * dh:dw * dh * 5 // 4].reshape(dh // 2, dw // 2), f[dw * dh * 5 // 4:].reshape(dh // 2, dw // 2)
        assert (y[:h, :w] == Y).all() and (u[:U.shape[0], :U.shape[1]] == U).all() and (v[:V.shape[0], :V.shape[1]] == V).all(), fmt


@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sized_stream_bit_exact(size):
    w, h = size
    info = check_both_formats(("sized", size), S.sized_stream(w, h, seed=w * h))
    assert info["key_frames"] == 1 and info["ymodes"] and info["levels"] != {0}


@pytest.mark.parametrize("name", sorted(_FEATURES))
def test_feature_bit_exact(name):
    check_both_formats(("feature", name), _FEATURES[name])


@pytest.mark.parametrize("name", sorted(_DAMAGED))
def test_damaged_stream_decodes_as_the_restatement_does(name):
    check_both_formats(("damaged", name), _DAMAGED[name], errors=True)


def test_size_change_mid_stream():
    data = S.size_change()
    assert [(w, h) for _, w, h in ref("size_change", data, 1)] == [(48, 32)] * 2 + [(80, 48), (34, 18)]
    check_both_formats("size_change", data)


def test_ivf_in_small_chunks_and_frame_per_call():
    data = S.sized_stream(48, 32, seed=7, frames=3)
    want = [f for f, _, _ in ref("chunks", data, 1)]
    assert decode(data, 1, chunks=[data[k:k + 7] for k in range(0, len(data), 7)])[0] == want
    assert decode(data, 1, chunks=vp8_ref.split_ivf(data))[0] == want


def test_thirty_three_pictures_more_than_one_batch():
    data = S.sized_stream(48, 32, seed=33, frames=33)
    info = check_both_formats("33", data)
    assert info["key_frames"] == 33


def test_inter_frame_fails_the_handle_by_name():
    with api.JmAmdDec(5, 1, options=dict(vp8=1)) as d:
        with pytest.raises(RuntimeError, match="VP8 inter frames are not built"):
            data = S.inter_after_key()
            d.decode_stream(data, chunks=[data])


def test_deinterlace_temporal_is_refused_at_init():
    with pytest.raises(RuntimeError, match="deinterlace_temporal"):
        api.JmAmdDec(5, 1, options=dict(vp8=1, deinterlace=2, deinterlace_temporal=1))


def test_stats_and_profile_counters():
    data = _FEATURES["partitions_4"]
    _, st = decode(data, 1, options=dict(profile=1), stats=("vp8_partitions", "vp8_filter_type", "vp8_bpred_mbs", "k_vp8_recon_ns", "k_vp8_recon_n",
                                                           "k_vp8_recon_pics", "k_vp8_recon_alg_bytes", "k_vp8_filter_ns", "k_vp8_filter_n",
                                                           "k_vp8_filter_pics", "k_vp8_filter_alg_bytes"))
    assert st["vp8_partitions"] == 4 and st["vp8_filter_type"] == 0 and st["vp8_bpred_mbs"] > 0
    assert all(st[k] > 0 for k in st if k.startswith("k_vp8_")), st
    _, st = decode(_FEATURES["simple_filter"], 1, stats=("vp8_filter_type", "vp8_hidden_frames"))
    assert st["vp8_filter_type"] == 1 and st["vp8_hidden_frames"] == 0
    _, st = decode(_FEATURES["hidden_frame"], 1, stats=("vp8_hidden_frames",))
    assert st["vp8_hidden_frames"] == 1 and st["vp8_key_frames"] == 3 and st["frames"] == 2


# ---- the output routes behind the decoder, one small case each ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    data = S.sized_stream(48, 32, seed=11, frames=2)
    return data, [f for f, _, _ in ref("small", data, 1)]


def test_composition_scale(small):
    data, F = small
    frames, _ = decode(data, 1, options=dict(target_width=24, target_height=20))
    assert frames == [scale_frame(f, 48, 32, 1, (0, 0, 48, 32), (24, 20)) for f in F]


def test_composition_rgb_is_bt601_limited_range(small):
    data, F = small
    spec = api.rgb_spec("u8")
    frames, st = decode(data, 1, rgb=spec, stats=("color_matrix", "color_range"))
    assert (st["color_matrix"], st["color_range"]) == (6, 1)
    assert frames == [rgb_frame(f, 48, 32, 1, (0, 0, 48, 32), (48, 32), spec, 6, False) for f in F]


def test_deinterlace_auto_never_fires(small):
    data, F = small
    frames, st = decode(data, 1, options=dict(deinterlace=1), stats=("deint_frames",))
    assert frames == F and st["deint_frames"] == 0


def test_device_output_route(small):
    data, F = small
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L = api.lib()
    got_frames = []
    with api.JmAmdDec(5, 1, options=dict(vp8=1, device_output=1)) as d:
        for chunk in [data] + [None] * 64:
            if api.jm_nvdec_is_exit(d.h):
                break
            _, got = api.jm_nvdec_decode_frame(chunk, len(chunk) if chunk else 0, d.h)
            if not got:
                continue
            dev, ln = C.c_void_p(), C.c_int(0)
            assert L.jm_amddec_output_frame_device(C.byref(dev), C.byref(ln), d.h) == 48 * 32 * 3 // 2
            host = np.zeros(ln.value, np.uint8)
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, ln.value, 2) == 0
            got_frames.append(host.tobytes())
    assert got_frames == F


def test_mixed_batch_with_the_other_four_codecs(oracle):
    """Three VP8 handles, one MPEG-2, one MJPEG, one HEVC and one H.264 handle decoding at once on threads: VP8, MPEG-2 and MJPEG pictures share the
    HEVC lane's batches.  Every frame of every handle is exact."""
    jobs = []
    for i, (w, h) in enumerate(((272, 16), (80, 272), (53, 37))):
        data = S.sized_stream(w, h, seed=500 + i, frames=5)
        jobs.append((5, data, [data[k:k + 1001] for k in range(0, len(data), 1001)], [f for f, _, _ in ref(("mixed", i), data, 1)]))
    m2 = scripted_mpeg2.sized_stream(200, 88, 56, 1, "IPBBPBB")
    jobs.append((4, m2, api.split_nalus(m2), [f for f, _, _ in mpeg2_ref.decode_stream(m2, 1)]))
    rng = np.random.default_rng(300)
    q = [[int(v) for v in rng.integers(1, 64, 64)] for _ in range(2)]
    mj = b"".join(jpeg_ref.encode(jpeg_ref.random_levels(rng, 0x22, 136, 24, density=0.25, amp=60, dc_amp=300), q, 0x22, 136, 24) for _ in range(5))
    jobs.append((2, mj, [mj[k:k + 997] for k in range(0, len(mj), 997)], [f for f, _, _ in jpeg_ref.decode_stream(mj, 1)]))
    n_ref = len(jobs)
    h264 = streams.generate(width=96, height=80, frames=8, gop=4, mode=1, num_ref=2, seed=0x4A4D0B01)
    hevc = streams.generate_hevc(width=96, height=80, frames=8, gop=4, num_ref=2, seed=0x4A4D0B02)
    w264, n264, _, _ = oracle.decode(h264, out_fmt=1)
    w265, n265, _, _ = streams.OracleHevc().decode(hevc, out_fmt=1)
    jobs += [(0, h264, None, None), (1, hevc, None, None)]
    got, errs = [None] * len(jobs), []

    def run(i):
        codec, data, chunks, _ = jobs[i]
        try:
            with api.JmAmdDec(codec, 1, options=dict(vp8=1) if codec == 5 else None) as d:
                got[i] = d.decode_stream(data, chunks=chunks)
        except Exception as e:          # noqa: BLE001 -- reported below, in the main thread
            errs.append((i, repr(e)))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i in range(n_ref):
        assert got[i] == jobs[i][3], f"handle {i} (codec {jobs[i][0]})"
    assert b"".join(got[n_ref]) == w264 and len(got[n_ref]) == n264
    assert b"".join(got[n_ref + 1]) == w265 and len(got[n_ref + 1]) == n265
