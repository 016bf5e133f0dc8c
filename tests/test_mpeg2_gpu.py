"""MPEG-2 decode (codec_type 4) on the device: k_mpeg2_recon against the Python restatement tests/mpeg2_ref.py, bit for bit, in both output
formats -- scripted streams (tests/scripted_mpeg2.py) at the sizes where the kernel's four-macroblock strips are partial, one stream per syntax
feature, a chain of twelve pictures whose anchors build on each other, the host's vector clamp, damage, a size change, the output routes behind the
decoder and a mixed batch with the other three codecs on the shared lane.  Every case fails without the feature: init(4) is refused."""
import ctypes as C
import threading

import numpy as np
import pytest

import jpeg_ref
import mpeg2_ref
import scripted_mpeg2 as S
from deint_ref import deint_frame
from jmcodec_amd import api
from test_rgb_output_host import rgb_frame
from test_scaled_output_host import scale_frame
from tools import streams

pytestmark = pytest.mark.gpu

# (width, height, progressive_sequence): one macroblock; 3 x 2; a coded size above the display size; 5.5 strips-worth of odd counts; an interlaced
# sequence whose coded height is 64; 17 macroblocks in one row (four strips and one macroblock); one macroblock per row, 17 rows
SIZES = [(16, 16, 1), (48, 32, 1), (40, 24, 1), (88, 56, 1), (48, 40, 0), (272, 16, 1), (16, 272, 1)]
_FEATURES = S.feature_cases()


def decode(data, fmt, chunks=None, options=None, rgb=None, stats=()):
    with api.JmAmdDec(4, fmt, options=options, rgb=rgb) as d:
        frames = d.decode_stream(data, chunks=chunks if chunks is not None else [data])
        return frames, {k: d.stat(k) for k in ("errors", "dropped_pictures", "frames") + tuple(stats)}


def check_both_formats(data, chunks=None, errors=False):
    info = {}
    for fmt in (0, 1):
        want = mpeg2_ref.decode_stream(data, fmt, info)
        frames, st = decode(data, fmt, chunks=chunks)
        assert len(frames) == len(want) == st["frames"]
        for i, (f, w) in enumerate(zip(frames, want)):
            assert f == w[0], f"frame {i} of {len(want)}, out_fmt {fmt}"
        assert (st["errors"] > 0) == errors and st["dropped_pictures"] == info["dropped"]
    return info


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}{'' if s[2] else 'i'}")
def test_partial_strips_bit_exact(size):
    w, h, prog = size
    info = check_both_formats(S.sized_stream(w * h, w, h, prog))
    assert info["types"] == [1, 2, 3, 3]


@pytest.mark.parametrize("name", sorted(_FEATURES))
def test_feature_bit_exact(name):
    check_both_formats(_FEATURES[name])


def test_twelve_pictures_chain_per_start_code():
    """I B B P ... whose anchors chain: an error in one picture shows in every later one.  One start-code unit per call, as the reference harness
    delivers them: every slice on its own."""
    data = S.chain_stream()
    info = check_both_formats(data, chunks=api.split_nalus(data))
    assert len(info["types"]) == 12 and info["types"][:4] == [1, 2, 3, 3]


def test_clamped_records_equal_the_restatements_clamp():
    """Vectors that reach outside the reference picture: the host clamps them and marks the records (the kernel's own clamp is never reached), the
    picture counts in errors, and the frames equal the restatement's, which clamps the same way."""
    data = S.clamped_stream()
    info = check_both_formats(data, errors=True)
    _, st = decode(data, 1, stats=("mpeg2_clamped_mbs",))
    assert st["mpeg2_clamped_mbs"] == info["clamped"] == 6


def test_truncated_slice_is_concealed_deterministically():
    check_both_formats(S.truncated_stream(), errors=True)


def test_size_change_mid_stream():
    data = S.size_change_stream()
    want = mpeg2_ref.decode_stream(data, 1)
    assert [(w, h) for _, w, h in want] == [(48, 32)] * 3 + [(80, 48)] * 4
    check_both_formats(data)


# ---- the output routes behind the decoder, one small case each ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interlaced():
    """48 x 40 interlaced, I P B with progressive_frame 0; the restatement's I420 frames in display order with each frame's top_field_first"""
    rng = np.random.default_rng(5)
    items = [("seq", dict(width=48, height=40, progressive_sequence=0, display=dict(matrix=6)))]
    for i, (t, tff) in enumerate((("I", 1), ("P", 0), ("B", 1))):
        items.append(("pic", S.random_picture(rng, t, 48, 40, 0, progressive_frame=0, top_field_first=tff, temporal_reference=i)))
    data, info = S.build(items), {}
    F = [f for f, _, _ in mpeg2_ref.decode_stream(data, 1, info)]
    return data, F, [fr["top_field_first"] for fr in info["frames"]]


def test_composition_scale(interlaced):
    data, F, _ = interlaced
    frames, _ = decode(data, 1, options=dict(target_width=24, target_height=20))
    assert frames == [scale_frame(f, 48, 40, 1, (0, 0, 48, 40), (24, 20)) for f in F]


def test_composition_rgb_matrix_from_the_display_extension(interlaced):
    data, F, _ = interlaced
    spec = api.rgb_spec("u8")
    frames, st = decode(data, 1, rgb=spec, stats=("color_matrix", "color_range"))
    assert (st["color_matrix"], st["color_range"]) == (6, 1)
    assert frames == [rgb_frame(f, 48, 40, 1, (0, 0, 48, 40), (48, 40), spec, 6, False) for f in F]
    # without the extension: matrix 1, the standard's default
    plain = S.sized_stream(9, 48, 32, 1, "I")
    frames, st = decode(plain, 1, rgb=spec, stats=("color_matrix", "color_range"))
    assert (st["color_matrix"], st["color_range"]) == (1, 1)
    assert frames == [rgb_frame(f, 48, 32, 1, (0, 0, 48, 32), (48, 32), spec, 1, False) for f, _, _ in mpeg2_ref.decode_stream(plain, 1)]


def test_deinterlace_auto_follows_progressive_frame_and_top_field_first(interlaced):
    data, F, tff = interlaced
    assert tff == [1, 1, 0]                                      # display order I B P
    frames, st = decode(data, 1, options=dict(deinterlace=1), stats=("deint_frames", "interlaced_sequence"))
    assert frames == [deint_frame(f, 48, 40, 1, 1, 0 if t else 1) for f, t in zip(F, tff)]
    assert st["deint_frames"] == 3 and st["interlaced_sequence"] == 1
    prog = S.sized_stream(10, 48, 32, 1, "IP")                  # progressive_frame chosen per picture by the script
    info = {}
    want = mpeg2_ref.decode_stream(prog, 1, info)
    frames, _ = decode(prog, 1, options=dict(deinterlace=1))
    assert frames == [f if fr["progressive_frame"] else deint_frame(f, 48, 32, 1, 1, 0 if fr["top_field_first"] else 1)
                      for (f, _, _), fr in zip(want, info["frames"])]


def test_field_rate(interlaced):
    data, F, tff = interlaced
    frames, st = decode(data, 1, options=dict(deinterlace=2, deinterlace_rate=1), stats=("field_rate_pairs",))
    want = []
    for f, t in zip(F, tff):
        first = 0 if t else 1
        want += [deint_frame(f, 48, 40, 1, 2, first), deint_frame(f, 48, 40, 1, 2, 1 - first)]
    assert frames == want and st["field_rate_pairs"] == 3


def test_device_output_route(interlaced):
    data, F, _ = interlaced
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L = api.lib()
    got_frames = []
    with api.JmAmdDec(4, 1, options=dict(device_output=1)) as d:
        for chunk in [data] + [None] * 64:
            if api.jm_nvdec_is_exit(d.h):
                break
            _, got = api.jm_nvdec_decode_frame(chunk, len(chunk) if chunk else 0, d.h)
            if not got:
                continue
            dev, ln = C.c_void_p(), C.c_int(0)
            assert L.jm_amddec_output_frame_device(C.byref(dev), C.byref(ln), d.h) == 48 * 40 * 3 // 2
            host = np.zeros(ln.value, np.uint8)
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, ln.value, 2) == 0
            got_frames.append(host.tobytes())
    assert got_frames == F


def test_deinterlace_temporal_is_refused_at_init():
    with pytest.raises(RuntimeError, match="deinterlace_temporal"):
        api.JmAmdDec(4, 1, options=dict(deinterlace=2, deinterlace_temporal=1))


def test_mixed_batch_with_mjpeg_hevc_and_h264(oracle):
    """Four MPEG-2 handles, two MJPEG, one HEVC and one H.264 handle decoding at once on threads: MPEG-2 and MJPEG pictures share the HEVC lane's
    batches.  Every frame of every handle is exact."""
    jobs = []
    for i, (w, h, prog) in enumerate(((272, 16, 1), (48, 40, 0), (88, 56, 1), (16, 272, 1))):
        data = S.sized_stream(200 + i, w, h, prog, "IPBBPBB")
        jobs.append((4, data, api.split_nalus(data), [f for f, _, _ in mpeg2_ref.decode_stream(data, 1)]))
    for i, (samp, w, h) in enumerate(((0x22, 136, 24), (0x21, 48, 32))):
        rng = np.random.default_rng(300 + i)
        q = [[int(v) for v in rng.integers(1, 64, 64)] for _ in range(2)]
        data = b"".join(jpeg_ref.encode(jpeg_ref.random_levels(rng, samp, w, h, density=0.25, amp=60, dc_amp=300), q, samp, w, h) for _ in range(5))
        jobs.append((2, data, [data[k:k + 997] for k in range(0, len(data), 997)], [f for f, _, _ in jpeg_ref.decode_stream(data, 1)]))
    h264 = streams.generate(width=96, height=80, frames=8, gop=4, mode=1, num_ref=2, seed=0x4A4D0B01)
    hevc = streams.generate_hevc(width=96, height=80, frames=8, gop=4, num_ref=2, seed=0x4A4D0B02)
    w264, n264, _, _ = oracle.decode(h264, out_fmt=1)
    w265, n265, _, _ = streams.OracleHevc().decode(hevc, out_fmt=1)
    jobs += [(0, h264, None, None), (1, hevc, None, None)]
    got, errs = [None] * len(jobs), []

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
    for i in range(6):
        assert got[i] == jobs[i][3], f"handle {i} (codec {jobs[i][0]})"
    assert b"".join(got[6]) == w264 and len(got[6]) == n264
    assert b"".join(got[7]) == w265 and len(got[7]) == n265
