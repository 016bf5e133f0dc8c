"""Picture hash verification on the device (option verify_hash, k_hevc_pichash; -m gpu).  The expected values never come from the product: the
stand-alone entry is compared with tests/pichash_ref.py, the analytic streams are stamped with hashes of the ARITHMETIC expectation
(analytic_hevc.expect_hevc -- no decoder of this project on that side), the generator streams with hashes of the CPU oracle's pictures.  The
corrupt cases flip a bit of the EXPECTED value; the slice data is never touched."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import analytic_hevc as ah
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


def device_hashes(planes, pitch, pad_rows=0, poison=0xA5):
    """([crc], [checksum]) of the three planes laid out as an NV12 surface of that pitch on the device; what is not a sample is `poison`."""
    surf, chroma_offset = ref.surface(planes, pitch, pad_rows, poison)
    h, w = planes[0].shape
    hip, d = _hip(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d), surf.size) == 0
    try:
        assert hip.hipMemcpy(d, surf.ctypes.data_as(C.c_void_p), surf.size, 1) == 0
        rc, crc, chk = api.picture_hash_device(d, pitch, chroma_offset, w, h)
        assert rc == 0, rc
        return crc, chk
    finally:
        hip.hipFree(d)


def random_planes(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8))


def want(planes):
    return ref.picture_hash(planes, ref.CRC), ref.picture_hash(planes, ref.CHECKSUM)


# ---- the stand-alone entry -----------------------------------------------------------------------------------------------------------------------
# 2x2 the smallest surface; 8x8 the smallest HEVC coded size; 24x16 a width that is no multiple of the widest load; 264x8 / 8x264 luma x >> 8 / y >> 8
# not 0; 520x520 chroma x >> 8 not 0 too, several workgroups; 66x34 a chroma row of an odd number of 4-byte units, a last band of 2 rows; 1920x1088 once
SIZES = [(2, 2), (8, 8), (24, 16), (264, 8), (8, 264), (520, 520), (66, 34), (1920, 1088)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_standalone_entry_equals_the_reference(w, h):
    """Random samples at two pitches above the width -- one a multiple of 16 (16-byte loads), one not (byte loads) -- with different padding values and
    a gap between the planes: both equal the reference, so the padding does not leak in."""
    planes = random_planes(w, h, 1000 * w + h)
    expected = want(planes)
    assert device_hashes(planes, (w + 15) // 16 * 16 + 16, pad_rows=0, poison=0xA5) == expected
    assert device_hashes(planes, w + 6, pad_rows=3, poison=0x5A) == expected


@pytest.mark.parametrize("value", [0x00, 0xFF])
def test_constant_surfaces(value):
    for w, h in ((264, 40), (66, 34)):
        planes = (np.full((h, w), value, np.uint8), np.full((h // 2, w // 2), value, np.uint8), np.full((h // 2, w // 2), value, np.uint8))
        assert device_hashes(planes, w + 8, poison=0xFF - value) == want(planes)
        assert device_hashes(planes, w, poison=0xFF - value) == want(planes)           # tight rows


def test_same_samples_at_two_pitches_and_paddings_hash_alike():
    planes = random_planes(200, 120, 77)
    assert device_hashes(planes, 200) == device_hashes(planes, 256, pad_rows=8, poison=0x00) == device_hashes(planes, 202, pad_rows=1, poison=0xFF)


def test_standalone_entry_rejects_bad_arguments():
    hip, d = _hip(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d), 4096) == 0
    try:
        for pitch, co, w, h in ((16, 256, 0, 2), (16, 256, 3, 2), (16, 256, 2, 3), (16, 256, 32, 2), (16, -1, 2, 2), (16, 256, 2, 0)):
            assert api.picture_hash_device(d, pitch, co, w, h)[0] == -1
        assert api.picture_hash_device(None, 16, 256, 2, 2)[0] == -1
    finally:
        hip.hipFree(d)


# ---- streams ---------------------------------------------------------------------------------------------------------------------------------------
def decode(data, chunks=None, **options):
    """(frames, {stat: value}) of one handle."""
    with api.JmAmdDec(1, 1, options=options) as d:
        frames = d.decode_stream(data, chunks=chunks)
        keys = ("errors", "device_wait_errors", "hash_pictures", "hash_checked", "hash_mismatch", "hash_unchecked", "hash_md5", "hash_first_bad_poc")
        st = {k: d.stat(k) for k in keys}
        st["last"] = ([d.stat(f"hash_last_crc:{c}") for c in range(3)], [d.stat(f"hash_last_checksum:{c}") for c in range(3)])
        return frames, st


@functools.lru_cache(maxsize=None)
def analytic(name):
    seq, pics = ah.HEVC_CASES[name](96, 80)
    assert hw.coded_size(seq) == (96, 80)
    return hw.write(seq, pics), ah.expect_hevc(seq, pics)


@pytest.mark.parametrize("hash_type", [ref.CRC, ref.CHECKSUM], ids=["crc", "checksum"])
@pytest.mark.parametrize("name", sorted(ah.HEVC_CASES))
def test_analytic_streams_verify_against_the_arithmetic_expectation(name, hash_type):
    data, planes = analytic(name)
    _, st = decode(hs.stamp(data, planes, hash_type), verify_hash=1)
    assert st["errors"] == 0 and st["hash_checked"] == st["hash_pictures"] == len(planes)
    assert st["hash_mismatch"] == 0 and st["hash_unchecked"] == 0 and st["hash_first_bad_poc"] == NO_POC
    assert st["last"] == want(planes[-1])


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


@pytest.mark.parametrize("hash_type", [ref.CRC, ref.CHECKSUM], ids=["crc", "checksum"])
@pytest.mark.parametrize("name", sorted(GEN))
def test_generator_streams_verify_against_the_oracle(name, hash_type):
    data, frames, planes, pocs = generated(name)
    if name == "gop8":
        assert pocs != sorted(pocs)                          # reordered: the messages follow decode order
    got, st = decode(hs.stamp(data, planes, hash_type), verify_hash=1)
    assert b"".join(got) == frames and st["errors"] == 0
    assert st["hash_checked"] == st["hash_pictures"] == len(planes) and st["hash_mismatch"] == 0 and st["hash_unchecked"] == 0
    assert st["last"] == want(planes[-1])


# ---- negative cases ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_type,k,c", [(ref.CRC, 3, 0), (ref.CHECKSUM, 5, 2), (ref.CRC, 0, 1)])
def test_a_wrong_expected_value_is_one_mismatch_and_every_frame_still_comes_out(hash_type, k, c):
    data, frames, planes, pocs = generated("gop8")
    got, st = decode(hs.stamp(data, planes, hash_type, corrupt=(k, c)), verify_hash=1)
    assert st["hash_mismatch"] == 1 and st["hash_first_bad_poc"] == pocs[k] and st["hash_checked"] == len(planes)
    assert b"".join(got) == frames


def test_verify_hash_2_fails_the_handle_with_the_picture_and_component():
    data, frames, planes, pocs = generated("gop8")
    bad = ref.picture_hash(planes[4], ref.CHECKSUM)[1]
    text = f"picture hash mismatch: POC {pocs[4]}, component Cb, checksum expected 0x{bad ^ 1:x} got 0x{bad:x}"
    with api.JmAmdDec(1, 1, options={"verify_hash": 2}) as d:
        with pytest.raises(RuntimeError) as e:
            d.decode_stream(hs.stamp(data, planes, ref.CHECKSUM, corrupt=(4, 1)))
        assert str(e.value) == text == api.lib().jm_amddec_last_error(d.h).decode()
        assert d.stat("hash_mismatch") == 1 and d.stat("failed") == 1
    got, st = decode(hs.stamp(data, planes, ref.CHECKSUM), verify_hash=2)      # a clean stream is not disturbed
    assert b"".join(got) == frames and st["hash_mismatch"] == 0 and st["hash_checked"] == len(planes)


def test_md5_is_counted_and_never_compared():
    data, frames, planes, _ = generated("low_delay")
    got, st = decode(hs.stamp(data, planes, ref.MD5, corrupt=(1, 0)), verify_hash=1)
    assert b"".join(got) == frames
    assert st["hash_md5"] == st["hash_pictures"] == len(planes) and st["hash_checked"] == 0 and st["hash_mismatch"] == 0 and st["hash_unchecked"] == 0


def test_option_off_changes_nothing():
    data, frames, planes, _ = generated("gop8")
    stamped = hs.stamp(data, planes, ref.CRC, corrupt=(2, 0))
    got, st = decode(stamped)
    assert b"".join(got) == frames and st["hash_pictures"] == 0 and st["hash_checked"] == 0 and st["errors"] == 0
    digests = []
    for s in (data, stamped):
        with api.JmAmdDec(1, 1, options={"digest": 1}) as d:
            assert b"".join(d.decode_stream(s)) == frames
            digests.append(d.stat("syntax_digest"))
    assert digests[0] == digests[1]


def test_four_handles_two_verifying_share_batches():
    """Four handles decode at once, each fed its whole stream in one call, so that the engine's batches mix pictures that ask for their hashes with
    pictures that do not (and, on the two plain handles, with stamped and unstamped streams)."""
    data, frames, planes, _ = generated("gop8")
    stamped = hs.stamp(data, planes, ref.CRC)
    jobs = [(stamped, dict(verify_hash=1)), (stamped, {}), (stamped, dict(verify_hash=1)), (data, {})]
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
    for i, (stream, opts) in enumerate(jobs):
        assert isinstance(out[i], tuple), out[i]
        got, st = out[i]
        assert b"".join(got) == frames * 3 and st["errors"] == 0, i
        if opts:
            assert st["hash_checked"] == st["hash_pictures"] == 3 * len(planes) and st["hash_mismatch"] == 0 and st["hash_unchecked"] == 0, i
        else:
            assert st["hash_pictures"] == 0 and st["hash_checked"] == 0, i


def test_push_pull_facade_with_verify_hash_2():
    """The facade exposes no stats: with verify_hash 2 a clean stamped stream runs to its end with every frame, a stream with one wrong value stops."""
    data, frames, planes, pocs = generated("low_delay")
    got, _, _, _ = api.intel_push_pull(hs.stamp(data, planes, ref.CRC), codec_type=1, options={"verify_hash": 2})
    assert b"".join(got) == frames
    with pytest.raises(RuntimeError, match=f"picture hash mismatch: POC {pocs[2]}, component Y, crc"):
        api.intel_push_pull(hs.stamp(data, planes, ref.CRC, corrupt=(2, 0)), codec_type=1, options={"verify_hash": 2})
