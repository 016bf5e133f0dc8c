"""MD5 picture hash verification on the device (options verify_hash + verify_md5, k_hevc_md5; -m gpu).  Every expected digest is hashlib's
(tests/pichash_ref.py) over numpy planes: the stand-alone entry is compared with it directly, the analytic streams are stamped with the MD5 of the
ARITHMETIC expectation (analytic_hevc.expect_hevc), the generator streams with the MD5 of the CPU oracle's pictures.  The corrupt cases flip a bit of
the EXPECTED digest; the slice data is never touched."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import analytic_hevc as ah
import md5_sizes as sz
import pichash_ref as ref
import scripted_hevc as hw
from jmcodec_amd import api
from tools import hevc_hash_sei as hs
from tools import streams

pytestmark = pytest.mark.gpu

NO_POC = -2 ** 31


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def device_md5(planes, pitch, pad_rows=0, poison=0xA5):
    """[digest of Y, Cb, Cr] of the three planes laid out as an NV12 surface of that pitch on the device; what is not a sample is `poison`."""
    surf, chroma_offset = ref.surface(planes, pitch, pad_rows, poison)
    h, w = planes[0].shape
    hip, d = _hip(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d), surf.size) == 0
    try:
        assert hip.hipMemcpy(d, surf.ctypes.data_as(C.c_void_p), surf.size, 1) == 0
        rc, digests = api.picture_md5_device(d, pitch, chroma_offset, w, h)
        assert rc == 0, rc
        return digests
    finally:
        hip.hipFree(d)


def random_planes(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8))


def want(planes):
    return ref.picture_hash(planes, ref.MD5)


# ---- the stand-alone entry -----------------------------------------------------------------------------------------------------------------------
SIZES = sz.SMALL + [sz.LARGE]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_standalone_entry_equals_hashlib(w, h):
    """Random samples at two pitches above the width -- one a multiple of 16 (16-byte loads), one not (byte loads) -- with different padding values and
    a gap between the planes (md5_sizes.py says what each size is for)."""
    planes = random_planes(w, h, 1000 * w + h)
    expected = want(planes)
    assert device_md5(planes, (w + 15) // 16 * 16 + 16, pad_rows=0, poison=0xA5) == expected
    assert device_md5(planes, w + 6, pad_rows=3, poison=0x5A) == expected


@pytest.mark.parametrize("value", [0x00, 0xFF])
def test_constant_surfaces(value):
    for w, h in ((264, 40), (66, 34)):
        planes = (np.full((h, w), value, np.uint8), np.full((h // 2, w // 2), value, np.uint8), np.full((h // 2, w // 2), value, np.uint8))
        assert device_md5(planes, w + 8, poison=0xFF - value) == want(planes)
        assert device_md5(planes, w, poison=0xFF - value) == want(planes)           # tight rows


def test_standalone_entry_rejects_bad_arguments():
    hip, d = _hip(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d), 4096) == 0
    try:
        for pitch, co, w, h in ((16, 256, 0, 2), (16, 256, 3, 2), (16, 256, 2, 3), (16, 256, 32, 2), (16, -1, 2, 2), (16, 256, 2, 0)):
            assert api.picture_md5_device(d, pitch, co, w, h)[0] == -1
        assert api.picture_md5_device(None, 16, 256, 2, 2)[0] == -1
    finally:
        hip.hipFree(d)


# ---- streams ---------------------------------------------------------------------------------------------------------------------------------------
KEYS = ("errors", "device_wait_errors", "hash_pictures", "hash_checked", "hash_mismatch", "hash_unchecked", "hash_md5", "hash_first_bad_poc")


def stats(d):
    st = {k: d.stat(k) for k in KEYS}
    st["last"] = [bytes.fromhex("".join("%08x" % d.stat(f"hash_last_md5:{c}:{k}") for k in range(4))) for c in range(3)]
    return st


def decode(data, chunks=None, **options):
    """(frames, {stat: value}) of one handle."""
    with api.JmAmdDec(1, 1, options=options) as d:
        frames = d.decode_stream(data, chunks=chunks)
        return frames, stats(d)


def assert_all_verified(st, planes):
    assert st["errors"] == 0 and st["hash_checked"] == st["hash_pictures"] == st["hash_md5"] == len(planes)
    assert st["hash_mismatch"] == 0 and st["hash_unchecked"] == 0 and st["hash_first_bad_poc"] == NO_POC
    assert st["last"] == want(planes[-1])


@functools.lru_cache(maxsize=None)
def analytic(name):
    seq, pics = ah.HEVC_CASES[name](96, 80)
    assert hw.coded_size(seq) == (96, 80)
    return hw.write(seq, pics), ah.expect_hevc(seq, pics)


@pytest.mark.parametrize("name", sorted(ah.HEVC_CASES))
def test_analytic_streams_verify_against_the_arithmetic_expectation(name):
    data, planes = analytic(name)
    _, st = decode(hs.stamp(data, planes, ref.MD5), verify_hash=1, verify_md5=1)
    assert_all_verified(st, planes)


# (the four generator configurations of test_pichash_gpu.py)
GEN = {
    "low_delay": dict(width=176, height=144, frames=8, num_ref=2, seed=0x4A4D0B01, sdh=1),
    "gop8": dict(width=176, height=144, frames=9, gop=8, num_ref=2, seed=0x4A4D0B02, sdh=1),
    "partial_ctbs_200x120": dict(width=200, height=120, frames=5, gop=4, num_ref=2, ctb_log2=6, seed=0x4A4D0B03),
    "no_filters": dict(width=176, height=144, frames=5, gop=4, num_ref=2, sao=0, deblock=0, seed=0x4A4D0B04),
}


@functools.lru_cache(maxsize=None)
def generated(name):
    """(stream, oracle frames as handed out, oracle pictures in decode order, their POCs)"""
    data = streams.generate_hevc(**GEN[name])
    frames, n, w, h = streams.OracleHevc().decode(data, 1)
    planes, pocs = ref.oracle_pictures(data)
    assert (w, h) == (GEN[name]["width"], GEN[name]["height"]) and n == len(planes) == GEN[name]["frames"]
    return data, frames, planes, pocs


@pytest.mark.parametrize("name", sorted(GEN))
def test_generator_streams_verify_against_the_oracle(name):
    data, frames, planes, pocs = generated(name)
    got, st = decode(hs.stamp(data, planes, ref.MD5), verify_hash=1, verify_md5=1)
    assert b"".join(got) == frames
    assert_all_verified(st, planes)


# ---- negative cases ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,c", [(3, 0), (5, 1), (0, 2)], ids=["Y", "Cb", "Cr"])
def test_a_wrong_expected_digest_is_one_mismatch_and_every_frame_still_comes_out(k, c):
    data, frames, planes, pocs = generated("gop8")
    got, st = decode(hs.stamp(data, planes, ref.MD5, corrupt=(k, c)), verify_hash=1, verify_md5=1)
    assert st["hash_mismatch"] == 1 and st["hash_first_bad_poc"] == pocs[k] and st["hash_checked"] == st["hash_md5"] == len(planes)
    assert st["hash_unchecked"] == 0 and b"".join(got) == frames


def test_verify_hash_2_fails_the_handle_with_the_picture_component_and_both_digests():
    data, frames, planes, pocs = generated("gop8")
    good = want(planes[4])[1]
    bad = bytes([good[0] ^ 1]) + good[1:]
    text = f"picture hash mismatch: POC {pocs[4]}, component Cb, md5 expected {bad.hex()} got {good.hex()}"
    with api.JmAmdDec(1, 1, options={"verify_hash": 2, "verify_md5": 1}) as d:
        with pytest.raises(RuntimeError) as e:
            d.decode_stream(hs.stamp(data, planes, ref.MD5, corrupt=(4, 1)))
        assert str(e.value) == text == api.lib().jm_amddec_last_error(d.h).decode()
        assert d.stat("hash_mismatch") == 1 and d.stat("failed") == 1
    got, st = decode(hs.stamp(data, planes, ref.MD5), verify_hash=2, verify_md5=1)      # a clean stream is not disturbed
    assert b"".join(got) == frames
    assert_all_verified(st, planes)


def test_verify_hash_1_leaves_the_text_as_the_last_error():
    data, frames, planes, pocs = generated("low_delay")
    good = want(planes[2])[0]
    with api.JmAmdDec(1, 1, options={"verify_hash": 1, "verify_md5": 1}) as d:
        assert b"".join(d.decode_stream(hs.stamp(data, planes, ref.MD5, corrupt=(2, 0)))) == frames
        text = f"picture hash mismatch: POC {pocs[2]}, component Y, md5 expected {bytes([good[0] ^ 1]).hex()}{good[1:].hex()} got {good.hex()}"
        assert api.lib().jm_amddec_last_error(d.h).decode() == text and d.stat("failed") == 0


def test_without_verify_md5_a_corrupted_md5_stream_is_counted_and_never_compared():
    data, frames, planes, _ = generated("low_delay")
    for opts in (dict(verify_hash=1), dict(verify_hash=2), dict(verify_hash=1, verify_md5=0)):
        got, st = decode(hs.stamp(data, planes, ref.MD5, corrupt=(1, 0)), **opts)
        assert b"".join(got) == frames and st["errors"] == 0
        assert st["hash_md5"] == st["hash_pictures"] == len(planes) and st["hash_checked"] == 0 and st["hash_mismatch"] == 0 and st["hash_unchecked"] == 0
    got, st = decode(hs.stamp(data, planes, ref.MD5, corrupt=(1, 0)), verify_md5=1)       # verify_md5 alone: suffix SEI is not parsed at all
    assert b"".join(got) == frames and st["hash_pictures"] == st["hash_md5"] == st["hash_checked"] == 0


def test_four_handles_md5_crc_unverified_md5_and_plain_share_batches():
    """Four handles decode at once, each fed its whole stream three times: one verifies MD5, one verifies the CRC of a CRC-stamped stream, one carries
    MD5 with verify_md5 0, one is plain -- so the engine's batches hold pictures with bit 1, bit 0 and no bit of hash_mode in one launch."""
    data, frames, planes, _ = generated("gop8")
    md5_stream, crc_stream = hs.stamp(data, planes, ref.MD5), hs.stamp(data, planes, ref.CRC)
    jobs = [(md5_stream, dict(verify_hash=1, verify_md5=1)), (crc_stream, dict(verify_hash=1)), (md5_stream, dict(verify_hash=1)), (data, {})]
    out = [None] * 4

    def run(i):
        try:
            out[i] = decode(None, chunks=[jobs[i][0]] * 3, **jobs[i][1])
        except Exception as e:      # noqa: BLE001 -- reported by the assertion below
            out[i] = e
    ts = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    n = 3 * len(planes)
    expect = [dict(hash_pictures=n, hash_md5=n, hash_checked=n), dict(hash_pictures=n, hash_md5=0, hash_checked=n),
              dict(hash_pictures=n, hash_md5=n, hash_checked=0), dict(hash_pictures=0, hash_md5=0, hash_checked=0)]
    for i in range(4):
        assert isinstance(out[i], tuple), out[i]
        got, st = out[i]
        assert b"".join(got) == frames * 3 and st["errors"] == 0, i
        assert {k: st[k] for k in expect[i]} == expect[i] and st["hash_mismatch"] == 0 and st["hash_unchecked"] == 0, (i, st)
    assert out[0][1]["last"] == want(planes[-1])


def test_push_pull_facade_with_verify_hash_2_and_verify_md5():
    """The facade exposes no stats: a clean stamped stream runs to its end with every frame, a stream with one wrong digest stops."""
    data, frames, planes, pocs = generated("low_delay")
    opts = {"verify_hash": 2, "verify_md5": 1}
    got, _, _, _ = api.intel_push_pull(hs.stamp(data, planes, ref.MD5), codec_type=1, options=opts)
    assert b"".join(got) == frames
    with pytest.raises(RuntimeError, match=f"picture hash mismatch: POC {pocs[2]}, component Y, md5"):
        api.intel_push_pull(hs.stamp(data, planes, ref.MD5, corrupt=(2, 0)), codec_type=1, options=opts)
