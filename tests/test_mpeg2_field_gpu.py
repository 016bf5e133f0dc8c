"""MPEG-2 option mpeg2_field_pictures on the device: k_mpeg2_recon with field pictures, 16x8 motion compensation and dual prime against the numpy
restatement tests/mpeg2_field_ref.py, bit for bit, in both output formats -- at the sizes where the strips and the field geometry can go wrong, one
stream per feature, a chain of twelve pictures mixing frame and field pictures fed one start-code unit per call, the analytic streams (closed
forms: tests/test_mpeg2_field_host.py pins the restatement to them), the vector clamp, damage, lone fields, the deinterlacers behind the decoder,
option mpeg2_device_vlc beside it, and a mixed batch with the other codecs.  Every case fails without the feature: the option does not exist."""
import threading

import pytest

import mpeg2_field_ref as F
import mpeg2_ref
import scripted_mpeg2 as S
import scripted_mpeg2_field as SF
from deint_ref import deint_frame
from jmcodec_amd import api
from test_mpeg2_field_host import dual_field_items, dual_frame_items, field_prediction_items, m16x8_items, pmv_items
from tools import streams

pytestmark = pytest.mark.gpu

# one macroblock per field; 3 x 2 per field (a partial strip); coded height 64 above a display of 20 lines per field; 17 macroblocks: four strips and one
SIZES = [(16, 32), (48, 64), (80, 40), (272, 32)]
STATS = ("mpeg2_field_pictures", "mpeg2_lone_fields", "mpeg2_dual_prime_mbs", "mpeg2_16x8_mbs", "mpeg2_clamped_mbs")
_FEATURES = SF.feature_cases()


def decode(data, fmt, chunks=None, options=None, stats=()):
    with api.JmAmdDec(4, fmt, options=dict(mpeg2_field_pictures=1, **(options or {}))) as d:
        frames = d.decode_stream(data, chunks=chunks if chunks is not None else [data])
        return frames, {k: d.stat(k) for k in ("errors", "dropped_pictures", "frames") + STATS + tuple(stats)}


def check_both_formats(data, chunks=None, options=None):
    info = {}
    for fmt in (0, 1):
        want = F.decode_stream(data, fmt, info)
        frames, st = decode(data, fmt, chunks=chunks, options=options)
        assert len(frames) == len(want) == st["frames"]
        for i, (f, w) in enumerate(zip(frames, want)):
            assert f == w[0], f"frame {i} of {len(want)}, out_fmt {fmt}"
        assert st["errors"] == info["errors"] and st["dropped_pictures"] == info["dropped"]
        assert (st["mpeg2_field_pictures"], st["mpeg2_lone_fields"], st["mpeg2_dual_prime_mbs"], st["mpeg2_16x8_mbs"], st["mpeg2_clamped_mbs"]) == (
            info["fields"], info["lone"], info["dual"], info["m16x8"], info["clamped"])
    return info


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_field_geometry_and_partial_strips_bit_exact(size):
    w, h = size
    info = check_both_formats(SF.field_stream(w + h, w, h, "IP PP BB Pd BB"))
    assert info["types"] == [1, 2, 2, 2, 3, 3, 2, 3, 3] and info["errors"] == 0 and info["dual"] > 0 and (info["m16x8"] > 0 or w == 16)


@pytest.mark.parametrize("name", sorted(_FEATURES))
def test_feature_bit_exact(name):
    assert check_both_formats(_FEATURES[name])["errors"] == 0


def test_twelve_pictures_of_frames_and_fields_per_start_code():
    """frame and field pictures, P and B, anchors that chain: an error in one picture shows in every later one.  One start-code unit per call."""
    data = SF.mixed_chain()
    info = check_both_formats(data, chunks=api.split_nalus(data))
    assert len(info["types"]) == 12 and info["fields"] == 8 and info["errors"] == 0 and info["dual"] > 0


@pytest.mark.parametrize("name", ["field_0", "field_1", "16x8", "dual_field", "dual_frame_tff0", "dual_frame_tff1", "pmv"])
def test_analytic_streams(name):
    items = {"field_0": lambda: field_prediction_items(0)[0], "field_1": lambda: field_prediction_items(1)[0], "16x8": lambda: m16x8_items()[0],
             "dual_field": lambda: dual_field_items(1)[0], "dual_frame_tff0": lambda: dual_frame_items(0, 1)[0],
             "dual_frame_tff1": lambda: dual_frame_items(1, -1)[0], "pmv": lambda: pmv_items()[0]}[name]()
    assert check_both_formats(SF.build(items))["errors"] == 0


@pytest.mark.parametrize("name", sorted(SF.clamped_cases()))
def test_clamped_records_equal_the_restatements_clamp(name):
    info = check_both_formats(SF.clamped_cases()[name])
    assert info["clamped"] > 0 and info["errors"] > 0


def test_truncated_slice_in_a_field_picture_is_concealed_deterministically():
    assert check_both_formats(SF.truncated_field_stream())["errors"] == 2


@pytest.mark.parametrize("name", sorted(SF.lone_cases()))
def test_lone_fields(name):
    """the frame of a lone field leaves with that field's lines repeated; an anchor's missing field is written, so later pictures predict from it"""
    data, frames, lone = SF.lone_cases()[name]
    info = check_both_formats(data)
    assert info["lone"] == lone and len(info["frames"]) == frames


@pytest.fixture(scope="module")
def field_stream_for_deint():
    """I-P fields bottom first, P fields top first, B fields bottom first, then a lone top field: I420 frames with the field first in time"""
    import numpy as np
    lone = SF.build([("seq", dict(width=48, height=64, progressive_sequence=0)), ("pic", SF.random_field_picture(np.random.default_rng(35), "I", 48, 64, 1))])
    data = SF.field_stream(33, 48, 64, "IP", first=2) + SF.field_stream(34, 48, 64, "PP BB", first=1) + lone      # (the sequence header is repeated)
    info = {}
    frames = [f for f, _, _ in F.decode_stream(data, 1, info)]
    return data, frames, info


def test_deinterlace_auto_keeps_the_field_first_in_the_stream(field_stream_for_deint):
    data, frames, info = field_stream_for_deint
    assert [(fr["first_parity"], fr["lone"]) for fr in info["frames"]] == [(1, 0), (0, 0), (0, 0), (0, 1)]      # display: IP, BB, PP, the lone I field
    got, st = decode(data, 1, options=dict(deinterlace=1), stats=("deint_frames",))
    want = [deint_frame(f, 48, 64, 1, 1, fr["lone"] - 1 if fr["lone"] else fr["first_parity"]) for f, fr in zip(frames, info["frames"])]
    assert got == want and st["deint_frames"] == 4 and st["mpeg2_lone_fields"] == 1


def test_field_rate_on_field_pictures(field_stream_for_deint):
    data, frames, info = field_stream_for_deint
    got, st = decode(data, 1, options=dict(deinterlace=2, deinterlace_rate=1), stats=("field_rate_pairs",))
    want = []
    for f, fr in zip(frames, info["frames"]):
        if fr["lone"]:                                           # a lone field has no other one: bob, once
            want.append(deint_frame(f, 48, 64, 1, 1, fr["lone"] - 1))
        else:
            want += [deint_frame(f, 48, 64, 1, 2, fr["first_parity"]), deint_frame(f, 48, 64, 1, 2, 1 - fr["first_parity"])]
    assert got == want and st["field_rate_pairs"] == 3


def test_device_vlc_beside_the_option():
    """mpeg2_device_vlc 1 with mpeg2_field_pictures 1: the 8 field pictures of the chain take the host path and count in mpeg2_host_pictures, its 4
    frame pictures -- the dual-prime P frame among them -- are decoded by the lane; the frames are the restatement's"""
    data, info = SF.mixed_chain(), {}
    want = F.decode_stream(data, 1, info)
    frames, st = decode(data, 1, options=dict(mpeg2_device_vlc=1), stats=("mpeg2_host_pictures", "mpeg2_dev_pictures"))
    assert frames == [f for f, _, _ in want] and st["errors"] == 0
    assert (st["mpeg2_host_pictures"], st["mpeg2_dev_pictures"]) == (8, 4)
    assert st["mpeg2_dual_prime_mbs"] == info["dual"] > 0


@pytest.mark.parametrize("layout,tff_word", [("I Pd Pd B", "tff0"), ("I PD PD B", "tff1")])
def test_the_lane_decodes_dual_prime_frame_pictures(layout, tff_word):
    """frame pictures only, so every picture is the lane's: the dual-prime records counted come from pictures counted in mpeg2_dev_pictures, and
    the frames equal the restatement's in both formats"""
    data, info = SF.field_stream(88, 80, 40, layout), {}
    for fmt in (0, 1):
        want = F.decode_stream(data, fmt, info)
        frames, st = decode(data, fmt, options=dict(mpeg2_device_vlc=1), stats=("mpeg2_host_pictures", "mpeg2_dev_pictures"))
        assert frames == [f for f, _, _ in want] and st["errors"] == 0 == info["errors"]
        assert (st["mpeg2_host_pictures"], st["mpeg2_dev_pictures"]) == (0, 4)
        assert st["mpeg2_dual_prime_mbs"] == info["dual"] > 0


def test_the_lane_without_the_option_still_fails_the_handle_on_dual_prime():
    data = _FEATURES["dual_prime_frame_tff1"]
    with api.JmAmdDec(4, 1, options=dict(mpeg2_device_vlc=1)) as d:
        with pytest.raises(RuntimeError):
            d.decode_stream(data, chunks=[data])
        msg = api.lib().jm_amddec_last_error(d.h).decode()
        assert d.stat("failed") == 1 and "dual-prime prediction is not supported" in msg


@pytest.mark.parametrize("name,word", [("b_fields", "field pictures"), ("dual_prime_frame_tff0", "dual-prime")])
def test_option_0_still_fails_the_handle(name, word):
    data = _FEATURES[name]
    with api.JmAmdDec(4, 1, options=dict(mpeg2_field_pictures=0)) as d:
        with pytest.raises(RuntimeError):
            d.decode_stream(data, chunks=[data])
        msg = api.lib().jm_amddec_last_error(d.h).decode()
        assert d.stat("failed") == 1 and "not supported" in msg and word in msg


def test_mixed_batch_field_pictures_beside_frame_pictures_hevc_h264_and_mjpeg(oracle):
    """Two field-picture handles beside two frame-picture MPEG-2 handles (option off), an MJPEG, an HEVC and an H.264 handle, at once on threads:
    batches of the shared lane hold field and frame pictures together.  Every frame of every handle is exact."""
    import jpeg_ref
    import numpy as np
    jobs = []
    for i, (w, h) in enumerate(((272, 32), (48, 64))):
        data = SF.field_stream(400 + i, w, h, "IP PD B BB PP BB B P")
        jobs.append((4, dict(mpeg2_field_pictures=1), data, api.split_nalus(data), [f for f, _, _ in F.decode_stream(data, 1)]))
    for i, (w, h, prog) in enumerate(((272, 16, 1), (48, 40, 0))):
        data = S.sized_stream(200 + i, w, h, prog, "IPBBPBB")
        jobs.append((4, None, data, api.split_nalus(data), [f for f, _, _ in mpeg2_ref.decode_stream(data, 1)]))
    rng = np.random.default_rng(300)
    q = [[int(v) for v in rng.integers(1, 64, 64)] for _ in range(2)]
    data = b"".join(jpeg_ref.encode(jpeg_ref.random_levels(rng, 0x22, 136, 24, density=0.25, amp=60, dc_amp=300), q, 0x22, 136, 24) for _ in range(5))
    jobs.append((2, None, data, [data[k:k + 997] for k in range(0, len(data), 997)], [f for f, _, _ in jpeg_ref.decode_stream(data, 1)]))
    h264 = streams.generate(width=96, height=80, frames=8, gop=4, mode=1, num_ref=2, seed=0x4A4D0B01)
    hevc = streams.generate_hevc(width=96, height=80, frames=8, gop=4, num_ref=2, seed=0x4A4D0B02)
    w264, n264, _, _ = oracle.decode(h264, out_fmt=1)
    w265, n265, _, _ = streams.OracleHevc().decode(hevc, out_fmt=1)
    jobs += [(0, None, h264, None, None), (1, None, hevc, None, None)]
    got, errs = [None] * len(jobs), []

    def run(i):
        codec, opts, data, chunks, _ = jobs[i]
        try:
            with api.JmAmdDec(codec, 1, options=opts) as d:
                got[i] = d.decode_stream(data, chunks=chunks)
        except Exception as e:          # noqa: BLE001 -- reported below, in the main thread
            errs.append((i, repr(e)))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i in range(5):
        assert got[i] == jobs[i][4], f"handle {i} (codec {jobs[i][0]})"
    assert b"".join(got[5]) == w264 and len(got[5]) == n264
    assert b"".join(got[6]) == w265 and len(got[6]) == n265
