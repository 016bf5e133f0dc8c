"""MPEG-2 option mpeg2_device_vlc on the device: k_mpeg2_vlc in front of k_mpeg2_recon.  Frames are compared bit for bit with the Python restatement
tests/mpeg2_ref.py in both output formats and with a handle that has the option at 0 -- the smallest shapes (one lane; a second, partial workgroup;
slices that start inside a row), one stream per syntax feature, a chain fed one start-code unit per call, the vector clamp, damage, a size change,
dual prime, a picture the prescan sends to the host path, a mixed batch with the other codecs, and the profile counters.  Every case fails without
the feature: set_option("mpeg2_device_vlc") is refused.  Damaged inputs are ones the CPU walk (tests/test_mpeg2_vlc_host.py) keeps inside every
buffer."""
import threading

import numpy as np
import pytest

import jpeg_ref
import mpeg2_ref
import scripted_mpeg2 as S
from jmcodec_amd import api
from test_mpeg2_host import _refusal_streams
from tools import streams

pytestmark = pytest.mark.gpu

STATS = ("errors", "dropped_pictures", "frames", "pictures", "mpeg2_dev_pictures", "mpeg2_host_pictures", "mpeg2_dev_slices", "mpeg2_dev_damaged_slices",
         "mpeg2_clamped_mbs")
_FEATURES = S.feature_cases()


def decode(data, fmt, chunks=None, device_vlc=1):
    with api.JmAmdDec(4, fmt, options=dict(mpeg2_device_vlc=device_vlc)) as d:
        frames = d.decode_stream(data, chunks=chunks if chunks is not None else [data])
        return frames, {k: d.stat(k) for k in STATS}


def check(data, chunks=None, errors=False, host_pictures=0):
    """both output formats against the restatement and against option 0; -> the restatement's info and the option-1 stats"""
    info, st = {}, None
    for fmt in (0, 1):
        want = mpeg2_ref.decode_stream(data, fmt, info)
        frames, st = decode(data, fmt, chunks=chunks)
        frames0, st0 = decode(data, fmt, chunks=chunks, device_vlc=0)
        assert len(frames) == len(want) == st["frames"]
        for i, (f, w) in enumerate(zip(frames, want)):
            assert f == w[0], f"frame {i} of {len(want)}, out_fmt {fmt}"
        assert frames == frames0
        assert (st["errors"] > 0) == errors and st["dropped_pictures"] == info["dropped"]
        assert (st["errors"], st["mpeg2_clamped_mbs"]) == (st0["errors"], st0["mpeg2_clamped_mbs"])
        assert st["mpeg2_host_pictures"] == host_pictures and st["mpeg2_dev_pictures"] == st["pictures"] - host_pictures > 0
        assert st0["mpeg2_dev_pictures"] == st0["mpeg2_host_pictures"] == st0["mpeg2_dev_slices"] == 0
    return info, st


def _four_slices_per_row():
    W, H = 272, 16
    rng = np.random.default_rng(3)
    cuts = (0, 3, 8, 13, 17)
    pic = dict(type="P", f_code=((2, 2), (15, 15)), slices=[
        dict(row=0, qcode=5, mbs=[dict(x=x, fwd=[(0, 0)], blocks={k: S.random_block(rng, False) for k in (0, 5)}) for x in range(cuts[i], cuts[i + 1])]) for i in range(4)])
    return S.build([("seq", dict(width=W, height=H)), ("pic", S.staircase(W, H, step=1)), ("pic", pic)])


# 16 x 16: a single lane; 48 x 32 and 88 x 56: I P B B of random macroblocks; 48 x 40 interlaced (coded height 64); 16 x 1072: 67 slices, the lanes
# spill into a second, partial workgroup
@pytest.mark.parametrize("size", [(16, 16, 1), (48, 32, 1), (88, 56, 1), (48, 40, 0), (16, 1072, 1)], ids=lambda s: f"{s[0]}x{s[1]}{'' if s[2] else 'i'}")
def test_smallest_shapes_bit_exact(size):
    w, h, prog = size
    info, st = check(S.sized_stream(w * h, w, h, prog))
    assert info["types"] == [1, 2, 3, 3]
    if size == (16, 16, 1):
        assert st["mpeg2_dev_slices"] == st["pictures"]
    if size == (16, 1072, 1):
        assert st["mpeg2_dev_slices"] == 67 * st["pictures"]


def test_four_slices_in_one_row_starting_mid_row():
    _, st = check(_four_slices_per_row())
    assert st["mpeg2_dev_slices"] == 1 + 4


@pytest.mark.parametrize("name", sorted(_FEATURES))
def test_feature_bit_exact(name):
    check(_FEATURES[name])


def test_chain_per_start_code_unit():
    data = S.chain_stream()
    info, _ = check(data, chunks=api.split_nalus(data))
    assert len(info["types"]) == 12


def test_clamped_vectors_are_counted_on_the_device():
    info, st = check(S.clamped_stream(), errors=True)
    assert st["mpeg2_clamped_mbs"] == info["clamped"] == 6 and st["errors"] > 0


def test_truncated_slice_is_concealed_like_the_restatement():
    _, st = check(S.truncated_stream(), errors=True)
    assert st["errors"] > 0 and st["mpeg2_dev_damaged_slices"] > 0


def test_size_change_mid_stream():
    data = S.size_change_stream()
    assert [(w, h) for _, w, h in mpeg2_ref.decode_stream(data, 1)] == [(48, 32)] * 3 + [(80, 48)] * 4
    check(data)


def test_dual_prime_fails_the_handle():
    items, _ = _refusal_streams()["dual prime"]
    data = S.build(items)
    with api.JmAmdDec(4, 1, options=dict(mpeg2_device_vlc=1)) as d:
        assert api.lib().jm_amddec_set_option(d.h, b"mpeg2_device_vlc", 1) == -1          # (known, and refused after init)
        with pytest.raises(RuntimeError):
            d.decode_stream(data, keep=False, chunks=[data])
        msg = api.lib().jm_amddec_last_error(d.h).decode()
        assert d.stat("failed") == 1
    assert "dual-prime" in msg and "not supported" in msg, msg


def test_out_of_order_slices_take_the_host_path():
    w = S._PicWriter(dict(width=48, height=48), S.staircase(48, 48))
    sl = [w.slice(s) for s in S.staircase(48, 48)["slices"]]
    data = S.build([("seq", dict(width=48, height=48))]) + w.header() + sl[1] + sl[0] + sl[2] + S._PicWriter(dict(width=48, height=48), S.staircase(48, 48, base=50)).bytes()
    # the first picture's slices are out of order (host path), the second's are not (device path)
    _, st = check(data, host_pictures=1)
    assert st["pictures"] == 2


def test_mixed_batch_with_option_off_mjpeg_and_h264(oracle):
    """Four handles at once on threads: MPEG-2 with the option, MPEG-2 without, MJPEG and H.264.  Every handle's frames are right; the device-path
    stats count on the first handle only."""
    m2a, m2b = S.sized_stream(200, 88, 56, 1, "IPBBPBB"), S.sized_stream(201, 48, 40, 0, "IPBBPBB")
    rng = np.random.default_rng(300)
    q = [[int(v) for v in rng.integers(1, 64, 64)] for _ in range(2)]
    jpg = b"".join(jpeg_ref.encode(jpeg_ref.random_levels(rng, 0x22, 136, 24, density=0.25, amp=60, dc_amp=300), q, 0x22, 136, 24) for _ in range(5))
    h264 = streams.generate(width=96, height=80, frames=8, gop=4, mode=1, num_ref=2, seed=0x4A4D0B01)
    w264, n264, _, _ = oracle.decode(h264, out_fmt=1)
    jobs = [(4, m2a, api.split_nalus(m2a), dict(mpeg2_device_vlc=1), [f for f, _, _ in mpeg2_ref.decode_stream(m2a, 1)]),
            (4, m2b, api.split_nalus(m2b), dict(mpeg2_device_vlc=0), [f for f, _, _ in mpeg2_ref.decode_stream(m2b, 1)]),
            (2, jpg, [jpg[k:k + 997] for k in range(0, len(jpg), 997)], None, [f for f, _, _ in jpeg_ref.decode_stream(jpg, 1)]),
            (0, h264, None, None, None)]
    got, stats, errs = [None] * 4, [None] * 4, []

    def run(i):
        codec, data, chunks, opt, _ = jobs[i]
        try:
            with api.JmAmdDec(codec, 1, options=opt) as d:
                got[i] = d.decode_stream(data, chunks=chunks)
                stats[i] = {k: d.stat(k) for k in STATS}
        except Exception as e:          # noqa: BLE001 -- reported below, in the main thread
            errs.append((i, repr(e)))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i in range(3):
        assert got[i] == jobs[i][4], f"handle {i} (codec {jobs[i][0]})"
    assert b"".join(got[3]) == w264 and len(got[3]) == n264
    assert stats[0]["mpeg2_dev_pictures"] == 7 and stats[0]["mpeg2_host_pictures"] == 0 and stats[0]["mpeg2_dev_slices"] > 0
    for i in (1, 2, 3):
        assert all(stats[i][k] == 0 for k in ("mpeg2_dev_pictures", "mpeg2_host_pictures", "mpeg2_dev_slices", "mpeg2_dev_damaged_slices")), (i, stats[i])


def test_profile_counters():
    data = S.chain_stream()
    with api.JmAmdDec(4, 1, options=dict(profile=1, mpeg2_device_vlc=1)) as d:
        before = {k: d.stat(k) for k in ("k_mpeg2_vlc_n", "k_mpeg2_vlc_pics", "k_mpeg2_vlc_ns", "k_mpeg2_vlc_alg_bytes")}
        frames = d.decode_stream(data, chunks=[data])
        after = {k: d.stat(k) for k in before}
        dev = d.stat("mpeg2_dev_pictures")
    assert frames == [f for f, _, _ in mpeg2_ref.decode_stream(data, 1)]
    assert dev == 12 and after["k_mpeg2_vlc_n"] - before["k_mpeg2_vlc_n"] > 0
    assert after["k_mpeg2_vlc_pics"] - before["k_mpeg2_vlc_pics"] == dev
    assert after["k_mpeg2_vlc_ns"] > before["k_mpeg2_vlc_ns"] and after["k_mpeg2_vlc_alg_bytes"] > before["k_mpeg2_vlc_alg_bytes"]
