"""Picture hash verification (option verify_hash), host side, no GPU: the two hashes' definitions against known answers that no code of this project
computed, the lane routines of k_hevc_pichash on the CPU (tools/pichash_asan.cpp under AddressSanitizer / UBSan), the identity that makes the CRC
parallel, and the product's SEI parser on a parse_only handle fed with streams stamped by tools/hevc_hash_sei.py."""
import binascii
import os
import subprocess

import numpy as np
import pytest

import jmcodec_amd
import pichash_ref as ref
from tools import hevc_hash_sei as hs
from tools import streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = {"parse_only": 1, "digest": 1, "verify_hash": 1}


# ---- the definitions ---------------------------------------------------------------------------------------------------------------------------
def test_crc_check_value():
    """0xE5CC for "123456789": the catalogue check value of CRC-16/SPI-FUJITSU (init 0x1D0F, poly 0x1021, no reflection, no final xor)."""
    assert ref.crc_bit_serial(b"123456789") == 0xE5CC
    assert ref.crc(np.frombuffer(b"123456789", dtype=np.uint8)) == 0xE5CC


def test_checksum_of_a_zero_plane_is_the_sum_of_the_mask():
    """512 x 512 zeros: x = 256 a + u, y = 256 b + v, m = u ^ v ^ a ^ b.  For fixed a, b, v the map u -> u ^ v ^ (a ^ b) permutes 0 .. 255, so the sum is
    4 (a, b) * 256 (v) * (0 + ... + 255)."""
    assert ref.checksum(np.zeros((512, 512), np.uint8)) == 4 * 256 * (255 * 256 // 2)


def test_checksum_of_the_mask_itself_is_zero():
    """256 x 1 holding x at column x: s ^ m = x ^ x."""
    assert ref.checksum(np.arange(256, dtype=np.uint8)[None, :]) == 0


def test_bit_serial_crc_equals_crc_hqx():
    rng = np.random.default_rng(132)
    for shape in [(1, 1), (2, 2), (3, 7), (8, 8), (17, 33), (64, 48), (1, 4097)]:
        p = rng.integers(0, 256, size=shape, dtype=np.uint8)
        assert ref.crc_bit_serial(p.tobytes()) == ref.crc(p), shape
    assert ref.crc_bit_serial(bytes(40)) == ref.crc(np.zeros(40, np.uint8)) and ref.crc_bit_serial(b"\xff" * 40) == ref.crc(np.full(40, 255, np.uint8))


# ---- the lane routines on the CPU --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pichash_asan(tmp_path_factory):
    out = tmp_path_factory.mktemp("pichash") / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "pichash_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return str(out / "pichash_asan")


def test_pichash_asan_builds_and_runs_clean(pichash_asan):
    """tools/pichash_asan.cpp: every work item of the kernel over exact-size surfaces against the bit-serial CRC and the plain checksum loop."""
    r = subprocess.run([pichash_asan], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ok: 100 walks over 16 sizes" in r.stdout
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]


def test_crc_combines_across_chunks(pichash_asan):
    """CRC(data) = XOR_k R(chunk_k) * x^(8 * bytes behind chunk k) ^ 0x1D0F * x^(8 * bytes), R = crc_hqx(., 0): random cuts of random data, the
    products by the routine of pichash_packed.h (the program's `shift` mode), everything else by binascii."""
    rng = np.random.default_rng(40)
    cases, args = [], []
    for n in (1, 2, 16, 17, 255, 4096, 4097, 32767, 40000, 100000):
        data = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        cuts = sorted(set(int(c) for c in rng.integers(0, n + 1, size=min(n, 9)))) if n > 1 else []
        edges = [0] + [c for c in cuts if 0 < c < n] + [n]
        terms = [(binascii.crc_hqx(data[a:b], 0), n - b) for a, b in zip(edges, edges[1:])] + [(0x1D0F, n)]
        cases.append((data, len(terms)))
        for r, behind in terms:
            args += [str(r), str(behind)]
    out = subprocess.run([pichash_asan, "shift"] + args, stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert len(out) == len(args) // 2
    k = 0
    for data, n_terms in cases:
        acc = 0
        for v in out[k:k + n_terms]:
            acc ^= int(v, 16)
        k += n_terms
        assert acc == binascii.crc_hqx(data, 0x1D0F) == ref.crc_bit_serial(data), len(data)


# ---- the SEI parser of the product --------------------------------------------------------------------------------------------------------------
def small_stream(**kw):
    d = dict(width=64, height=64, frames=5, gop=4, num_ref=2, seed=0x4A4D0A01)
    d.update(kw)
    return streams.generate_hevc(**d)


def parse(data, options=OPTS):
    """(frames, {stat: value}, [(poc, type, [values])]) of a parse_only handle."""
    with jmcodec_amd.JmAmdDec(1, 1, options=options) as d:
        n = d.decode_stream(data, keep=False)
        st = {k: d.stat(k) for k in ("errors", "hash_pictures", "hash_md5", "hash_checked", "hash_mismatch", "hash_unchecked", "hash_first_bad_poc")}
        st["digest"] = d.stat("syntax_digest") & (2 ** 64 - 1)
        seen = [(d.stat(f"hash_sei_poc:{i}"), d.stat(f"hash_sei_type:{i}"), [d.stat(f"hash_sei_value:{i}:{c}") for c in range(3)])
                for i in range(st["hash_pictures"])]
        return n, st, seen


def noise_pictures(n, w, h, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8))
            for _ in range(n)]


@pytest.mark.parametrize("hash_type", [ref.CRC, ref.CHECKSUM])
def test_stamped_values_come_back_per_picture(hash_type):
    data = small_stream()
    pocs = streams.OracleHevc().display_pocs(data)
    pics = noise_pictures(5, 64, 64, 7)
    n, st, seen = parse(hs.stamp(data, pics, hash_type))
    assert n == 5 and st["errors"] == 0 and st["hash_pictures"] == 5 and st["hash_md5"] == 0
    assert [s[1] for s in seen] == [hash_type] * 5 and sorted(s[0] for s in seen) == sorted(pocs)
    assert [s[2] for s in seen] == [ref.picture_hash(p, hash_type) for p in pics]
    # nothing is compared without a device, and nothing is reported as compared
    assert st["hash_checked"] == st["hash_mismatch"] == st["hash_unchecked"] == 0 and st["hash_first_bad_poc"] == -2 ** 31


def test_md5_messages_are_counted_not_kept():
    data = small_stream()
    n, st, seen = parse(hs.stamp(data, noise_pictures(5, 64, 64, 8), ref.MD5))
    assert n == 5 and st["errors"] == 0 and st["hash_pictures"] == st["hash_md5"] == 5 and [s[1] for s in seen] == [0] * 5


def test_option_off_means_not_parsed_and_option_range():
    data = small_stream()
    stamped = hs.stamp(data, noise_pictures(5, 64, 64, 9), ref.CRC)
    n, st, _ = parse(stamped, {"parse_only": 1, "digest": 1})
    assert n == 5 and st["hash_pictures"] == 0 and st["digest"] == parse(data, {"parse_only": 1, "digest": 1})[1]["digest"]
    L = jmcodec_amd.lib()
    h = L.jm_amddec_create_handle()
    try:
        assert [L.jm_amddec_set_option(h, b"verify_hash", v) for v in (-1, 3, 0, 1, 2)] == [-1, -1, 0, 0, 0]
        L.jm_amddec_set_option(h, b"parse_only", 1)
        assert L.jm_amddec_init(1, 1, None, 0, h) == 0
        assert L.jm_amddec_set_option(h, b"verify_hash", 1) == -1          # after init
    finally:
        L.jm_amddec_deinit(h)


def special_nals(data):
    """The stream's NALs and pictures, and a dict builder: one special suffix SEI NAL per picture."""
    nals = hs.split_nals(data)
    return nals, hs.pictures_of(nals)


def test_message_walk_edge_cases():
    """Per picture of one stream: (0) two hash messages in one NAL -- the second replaces the first; (1) an unknown payload, with 0xFF-extended type
    and size, in front of the hash; (2) values full of 00 00 0x runs, which emulation prevention breaks up; (3) a truncated message: ignored and
    counted as an error; (4) a second NAL for the same picture replaces the first NAL's message."""
    data = small_stream()
    nals, pics = special_nals(data)
    crc_a, crc_b, sums = [0x1234, 0xABCD, 0x0001], [0x0000, 0x0300, 0xFFFF], [0x00000300, 0x00000001, 0x00000000]
    msg = lambda t, v: hs.sei_message(132, ref.sei_payload(t, v))
    unknown = hs.sei_message(5 + 255 * 2, bytes(range(256)) + bytes(44))          # type 515: two 0xFF type bytes; size 300: one 0xFF size byte
    truncated = msg(ref.CHECKSUM, sums)[:-5]                                      # says 13 bytes, brings 8
    extra = {
        pics[0][0]: hs.sei_nal(msg(ref.CRC, crc_a) + msg(ref.CRC, crc_b), pics[0][1]),
        pics[1][0]: hs.sei_nal(unknown + msg(ref.CRC, crc_a), pics[1][1]),
        pics[2][0]: hs.sei_nal(msg(ref.CHECKSUM, sums), pics[2][1]),
        pics[3][0]: hs.sei_nal(truncated, pics[3][1], raw=True),
        pics[4][0]: hs.sei_nal(msg(ref.CRC, crc_a), pics[4][1]) + hs.sei_nal(msg(ref.CHECKSUM, sums), pics[4][1]),
    }
    assert b"\x00\x00\x03" in extra[pics[2][0]][5:]
    n, st, seen = parse(hs.join(nals, extra))
    assert n == 5 and st["errors"] == 1 and st["hash_pictures"] == 4
    assert [(s[1], s[2]) for s in seen] == [(ref.CRC, crc_b), (ref.CRC, crc_a), (ref.CHECKSUM, sums), (ref.CHECKSUM, sums)]
    assert st["digest"] == parse(data)[1]["digest"]


def test_wrong_sizes_lying_sizes_and_reserved_types_are_ignored():
    data = small_stream()
    nals, pics = special_nals(data)
    bad = [hs.sei_message(132, ref.sei_payload(ref.CRC, [1, 2, 3]) + b"\x00"),           # oversized for its hash_type
           hs.sei_message(132, ref.sei_payload(ref.CHECKSUM, [1, 2, 3])[:-1]),           # one byte short (but its size byte is honest)
           hs.sei_message(132, b""),                                                     # no hash_type at all
           b"\x84\xff\xff\xff",                                                          # a size that never ends
           b"\xff\xff"]                                                                  # a type that never ends
    extra = {pics[k][0]: hs.sei_nal(m, pics[k][1]) for k, m in enumerate(bad)}
    n, st, seen = parse(hs.join(nals, extra))
    assert n == 5 and st["errors"] == 5 and st["hash_pictures"] == 0 and seen == []
    reserved = {pics[0][0]: hs.sei_nal(hs.sei_message(132, bytes([7]) + bytes(12)), pics[0][1])}     # hash_type 7: skipped like an unknown payload
    n, st, _ = parse(hs.join(nals, reserved))
    assert n == 5 and st["errors"] == 0 and st["hash_pictures"] == 0


def test_hash_in_a_prefix_sei_or_without_a_picture_is_ignored():
    data = small_stream()
    nals, pics = special_nals(data)
    m = hs.sei_message(132, ref.sei_payload(ref.CRC, [1, 2, 3]))
    n, st, _ = parse(hs.join(nals, {p[0]: hs.sei_nal(m, p[1], nal_unit_type=39) for p in pics}))
    assert n == 5 and st["errors"] == 0 and st["hash_pictures"] == 0
    # a suffix SEI in front of the first picture (behind the PPS): there is no picture to attach it to
    first_vcl = min(i for i, (_, nal) in enumerate(nals) if hs.is_vcl(nal))
    n, st, _ = parse(hs.join(nals, {first_vcl - 1: hs.sei_nal(m)}))
    assert n == 5 and st["errors"] == 0 and st["hash_pictures"] == 0


def test_suffix_sei_between_slice_segments_does_not_split_the_picture():
    """128 x 96 in slices of 5 CTBs with dependent segments: a hash NAL behind EVERY slice segment NAL.  The pictures, their order and their syntax are
    those of the unstamped stream, and every picture ends up with the last message sent for it."""
    kw = dict(width=128, height=96, frames=3, slice_ctus=5, dep_slices=1, ctb_log2=4, mode=1, seed=24)
    data = streams.generate_hevc(**kw)
    nals, pics = special_nals(data)
    vcl = [i for i, (_, nal) in enumerate(nals) if hs.is_vcl(nal)]
    assert len(vcl) > 3 * len(pics)
    extra = {i: hs.sei_nal(hs.sei_message(132, ref.sei_payload(ref.CRC, [k, k + 1, k + 2])), nals[i][1][1] & 7) for k, i in enumerate(vcl)}
    plain, stamped = parse(data), parse(hs.join(nals, extra))
    assert stamped[0] == plain[0] == 3 and stamped[1]["errors"] == 0 and stamped[1]["digest"] == plain[1]["digest"]
    assert stamped[1]["hash_pictures"] == 3
    assert [s[2][0] for s in stamped[2]] == [vcl.index(last) for last, _ in pics]
    # ... and with the option off the same bytes parse to the same syntax
    assert parse(hs.join(nals, extra), {"parse_only": 1, "digest": 1})[1]["digest"] == plain[1]["digest"]
