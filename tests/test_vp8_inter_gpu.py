"""VP8 inter-frame decode (codec_type 5, options vp8 + vp8_inter) on the device: k_vp8_inter, then k_vp8_recon for the intra macroblocks and
k_vp8_filter with the inter-frame thresholds, bit for bit in both output formats against the Python restatement tests/vp8_inter_ref.py.

There is no independent pin for inter frames (tests/test_vp8_inter_host.py says what holds them instead); the restatement's key frames are pinned by
libwebp (tests/test_vp8_host.py).  The streams are scripted_vp8_inter's: the sizes at which the wavefront kernels have one macroblock, one row, a
second band of rows; every feature case; damaged streams; a golden frame that outlives the surface pool and a batch; the input forms; handles in
threads that put key frames and inter frames into one batch; the output routes behind the decoder.

Every case fails without the feature: option vp8_inter does not exist, and an inter frame fails the handle."""
import ctypes as C
import threading

import numpy as np
import pytest

import scripted_vp8 as S
import scripted_vp8_inter as SI
import vp8_inter_ref as I
import vp8_ref
from jmcodec_amd import api
from test_rgb_output_host import rgb_frame
from test_scaled_output_host import scale_frame

pytestmark = pytest.mark.gpu

_FEATURES = dict(SI.feature_cases())
_DAMAGED = dict(SI.damaged_cases())
_REF = {}
STATS = ("errors", "frames", "vp8_key_frames", "vp8_inter_frames", "p_pictures", "vp8_golden_refs", "vp8_altref_refs", "vp8_split_mbs", "vp8_intra_in_inter_mbs",
         "vp8_hidden_frames")


def ref(key, data, fmt, info=None):
    """the restatement's frames, computed once per stream and format"""
    if (key, fmt) not in _REF:
        i = {}
        _REF[(key, fmt)] = (I.decode_stream(data, fmt, i), i)
    if info is not None:
        info.update(_REF[(key, fmt)][1])
    return _REF[(key, fmt)][0]


def decode(data, fmt, chunks=None, options=None, rgb=None, stats=()):
    with api.JmAmdDec(5, fmt, options=dict(options or {}, vp8=1, vp8_inter=1), rgb=rgb) as d:
        frames = d.decode_stream(data, chunks=chunks if chunks is not None else [data])
        return frames, {k: d.stat(k) for k in STATS + tuple(stats)}


def check_both_formats(key, data, chunks=None, errors=False):
    info = {}
    for fmt in (0, 1):
        want = ref(key, data, fmt, info)
        frames, st = decode(data, fmt, chunks=chunks)
        assert len(frames) == len(want) == st["frames"]
        for i, (f, w) in enumerate(zip(frames, want)):
            assert f == w[0], f"frame {i} of {len(want)}, out_fmt {fmt}"
        assert (st["errors"] > 0) == errors
        assert (st["vp8_key_frames"], st["vp8_inter_frames"], st["p_pictures"], st["vp8_hidden_frames"]) == (info["key_frames"], info["inter_frames"], info["inter_frames"], info["hidden"])
        assert (st["vp8_golden_refs"], st["vp8_altref_refs"], st["vp8_split_mbs"], st["vp8_intra_in_inter_mbs"]) == (info["golden_refs"], info["altref_refs"], info["split_mbs"], info["intra_in_inter"])
    return info


@pytest.mark.parametrize("size", SI.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sized_stream_bit_exact(size):
    """a key frame and three random inter frames.  16x16: every neighbour and every window lies outside the frame; 53x37: prediction reads the uncropped
    area; 272x16, 16x272, 80x272: the 16-row bands of the wavefront kernels"""
    w, h = size
    info = check_both_formats(("sized", size), SI.sized_stream(w, h, seed=w * h))
    assert (info["key_frames"], info["inter_frames"]) == (1, 3) and info["inter_levels"] != {0}


@pytest.mark.parametrize("name", sorted(_FEATURES))
def test_feature_bit_exact(name):
    check_both_formats(("feature", name), _FEATURES[name])


@pytest.mark.parametrize("name", sorted(_DAMAGED))
def test_damaged_stream_decodes_as_the_restatement_does(name):
    check_both_formats(("damaged", name), _DAMAGED[name], errors=True)


def test_golden_outlives_the_surface_pool_and_a_batch():
    """45 frames: golden is set at frame 0 and read by frame 21, set again by the key frame 22 and read by frame 44 -- more frames than surfaces and more
    than one batch; a hidden altref on the way"""
    info = check_both_formats("long_golden", SI.long_golden_stream(45))
    assert (info["key_frames"], info["inter_frames"], info["hidden"]) == (2, 43, 1)


def test_ivf_in_small_chunks_and_frame_per_call():
    data = SI.sized_stream(48, 32, seed=7, frames=4)
    want = [f for f, _, _ in ref("chunks", data, 1)]
    assert decode(data, 1, chunks=[data[k:k + 7] for k in range(0, len(data), 7)])[0] == want
    assert decode(data, 1, chunks=vp8_ref.split_ivf(data))[0] == want


def test_option_gating():
    """with the option an inter frame behind a key frame decodes (this fails on a library without the feature); without it the handle fails as before"""
    data = S.inter_after_key()
    frames, st = decode(data, 1)
    assert len(frames) == 2 == st["frames"] and frames == [f for f, _, _ in ref("inter_after_key", data, 1)]
    with api.JmAmdDec(5, 1, options=dict(vp8=1)) as d:
        with pytest.raises(RuntimeError, match="VP8 inter frames are not built"):
            d.decode_stream(data, chunks=[data])


def test_six_handles_mix_key_and_inter_frames_in_batches():
    """Six handles on threads: two key-frame-only streams, four inter streams (one of them without a single intra macroblock in its inter frames), so that
    batches hold key frames and inter frames side by side and k_vp8_recon runs for some pictures of a batch only.  Every frame of every handle is exact."""
    jobs = []
    for i, (w, h) in enumerate(((48, 32), (80, 272))):
        data = S.sized_stream(w, h, seed=700 + i, frames=6)
        jobs.append((data, dict(vp8=1, vp8_inter=i), [f for f, _, _ in vp8_ref.decode_stream(data, 1)]))
    for i, (w, h) in enumerate(((272, 16), (80, 272), (53, 37))):
        data = SI.sized_stream(w, h, seed=710 + i, frames=6)
        jobs.append((data, dict(vp8=1, vp8_inter=1), [f for f, _, _ in ref(("six", i), data, 1)]))
    st = SI.Stream(48, 32)
    frames = [st.key(S.random_mbs(48, 32, 720), level=10, yac=30)] + [st.inter(SI.random_inter_mbs(48, 32, 721 + k, intra=0.0), level=10, yac=30) for k in range(8)]
    data = vp8_ref.ivf(frames, 48, 32)
    jobs.append((data, dict(vp8=1, vp8_inter=1), [f for f, _, _ in ref(("six", "no_intra"), data, 1)]))
    got, errs = [None] * len(jobs), []

    def run(i):
        data, opts, _ = jobs[i]
        try:
            with api.JmAmdDec(5, 1, options=opts) as d:
                got[i] = d.decode_stream(data, chunks=[data[k:k + 1001] for k in range(0, len(data), 1001)])
        except Exception as e:          # noqa: BLE001 -- reported below, in the main thread
            errs.append((i, repr(e)))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i in range(len(jobs)):
        assert got[i] == jobs[i][2], f"handle {i}"


def test_profile_counters_of_the_three_kernels():
    keys = ("k_vp8_inter_ns", "k_vp8_inter_n", "k_vp8_inter_pics", "k_vp8_inter_alg_bytes", "k_vp8_recon_pics", "k_vp8_filter_pics")

    def counted(data):
        """what one stream adds to the engine's counters (they are the engine's, shared by the handles of the process)"""
        with api.JmAmdDec(5, 1, options=dict(vp8=1, vp8_inter=1, profile=1)) as d:
            before = {k: d.stat(k) for k in keys}
            d.decode_stream(data, chunks=[data])
            return {k: d.stat(k) - before[k] for k in keys}
    st = counted(_FEATURES["intra_beside_inter"])
    assert st["k_vp8_inter_ns"] > 0 and st["k_vp8_inter_n"] > 0 and st["k_vp8_inter_pics"] == 5 and st["k_vp8_inter_alg_bytes"] > 0
    assert st["k_vp8_recon_pics"] == 6 and st["k_vp8_filter_pics"] == 5       # (every inter frame of the stream has intra macroblocks; the key frame has level 0)
    # inter frames without intra macroblocks are no pictures of k_vp8_recon
    st = counted(_FEATURES["references"])
    assert st["k_vp8_inter_pics"] == 13 and 1 <= st["k_vp8_recon_pics"] < 14


# ---- the output routes behind the decoder, one small case each ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    data = SI.sized_stream(48, 32, seed=11, frames=2)
    return data, [f for f, _, _ in ref("small", data, 1)]


def test_composition_scale(small):
    data, F = small
    frames, _ = decode(data, 1, options=dict(target_width=24, target_height=20))
    assert frames == [scale_frame(f, 48, 32, 1, (0, 0, 48, 32), (24, 20)) for f in F]


def test_composition_rgb(small):
    data, F = small
    spec = api.rgb_spec("u8")
    frames, _ = decode(data, 1, rgb=spec)
    assert frames == [rgb_frame(f, 48, 32, 1, (0, 0, 48, 32), (48, 32), spec, 6, False) for f in F]


def test_device_output_route(small):
    data, F = small
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L = api.lib()
    got_frames = []
    with api.JmAmdDec(5, 1, options=dict(vp8=1, vp8_inter=1, device_output=1)) as d:
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
