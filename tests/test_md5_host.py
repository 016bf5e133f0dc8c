"""MD5 of the decoded picture hash SEI (option verify_md5), host side, no GPU: the lane routines of k_hevc_md5 playing the kernel on the CPU
(tools/md5_asan.cpp under AddressSanitizer / UBSan) against hashlib, and the product's SEI parser keeping the digests on a parse_only handle.  Every
expected digest is hashlib's."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import jmcodec_amd
import md5_sizes as sz
import pichash_ref as ref
from tools import hevc_hash_sei as hs
from tools import streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def md5_asan(tmp_path_factory):
    out = tmp_path_factory.mktemp("md5") / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "md5_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return str(out / "md5_asan")


def run(program, *args):
    r = subprocess.run([program, *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
    return r.stdout.split("\n")


def test_md5_asan_builds_and_runs_clean(md5_asan):
    """Without arguments: the RFC 1321 test suite and the exact-size walks; the tile it prints is the literal the size list was built from."""
    lines = run(md5_asan)
    assert lines[0] == f"tile {sz.TILE}"
    assert any(ln.startswith("ok: ") for ln in lines), lines


@pytest.mark.parametrize("n", sz.RAW_LENGTHS)
def test_raw_stream_equals_hashlib(md5_asan, tmp_path, n):
    data = np.random.default_rng(n).integers(0, 256, n, np.uint8).tobytes()
    (tmp_path / "raw.bin").write_bytes(data)
    assert run(md5_asan, "raw", tmp_path / "raw.bin")[0] == hashlib.md5(data).hexdigest()


@pytest.mark.parametrize("w,h", sz.SMALL + [sz.LARGE], ids=[f"{w}x{h}" for w, h in sz.SMALL + [sz.LARGE]])
def test_surface_walk_equals_hashlib(md5_asan, tmp_path, w, h):
    """The kernel's staging items and tiles in order over a buffer of the exact size (the file ends with the last chroma sample), at a 16-aligned
    pitch and at w + 6 with other poison and a gap between the planes: an over-read is a sanitizer report, leaked padding a wrong digest."""
    rng = np.random.default_rng(1000 * w + h)
    planes = (rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8))
    want = [d.hex() for d in ref.picture_hash(planes, ref.MD5)]
    for pitch, pad_rows, poison in (((w + 15) // 16 * 16 + 16, 0, 0xA5), (w + 6, 3, 0x5A)):
        surf, chroma_offset = ref.surface(planes, pitch, pad_rows, poison)
        exact = surf[:chroma_offset + pitch * (h // 2 - 1) + w]
        (tmp_path / "surf.bin").write_bytes(exact.tobytes())
        assert run(md5_asan, "surface", tmp_path / "surf.bin", pitch, chroma_offset, w, h)[:3] == want, (pitch, pad_rows)


# ---- the SEI parser of the product --------------------------------------------------------------------------------------------------------------
def test_parse_only_handle_keeps_the_digests():
    data = streams.generate_hevc(width=64, height=64, frames=5, gop=4, num_ref=2, seed=0x4A4D0A01)
    rng = np.random.default_rng(14)
    pics = [(rng.integers(0, 256, (64, 64), np.uint8), rng.integers(0, 256, (32, 32), np.uint8), rng.integers(0, 256, (32, 32), np.uint8)) for _ in range(5)]
    for opts in ({"parse_only": 1, "verify_hash": 1}, {"parse_only": 1, "verify_hash": 1, "verify_md5": 1}):
        with jmcodec_amd.JmAmdDec(1, 1, options=opts) as d:
            assert d.decode_stream(hs.stamp(data, pics, ref.MD5), keep=False) == 5
            assert d.stat("errors") == 0 and d.stat("hash_pictures") == d.stat("hash_md5") == 5
            assert d.stat("hash_checked") == d.stat("hash_mismatch") == d.stat("hash_unchecked") == 0        # nothing is compared without a device
            for n, planes in enumerate(pics):
                assert d.stat(f"hash_sei_type:{n}") == 0
                for c, digest in enumerate(ref.picture_hash(planes, ref.MD5)):
                    words = [d.stat(f"hash_sei_md5:{n}:{c}:{k}") for k in range(4)]
                    assert "".join("%08x" % v for v in words) == digest.hex(), (n, c)
            assert d.stat("hash_sei_md5:5:0:0") == -1 and d.stat("hash_sei_md5:0:3:0") == -1 and d.stat("hash_sei_md5:0:0:4") == -1


def test_verify_md5_option_range():
    L = jmcodec_amd.lib()
    h = L.jm_amddec_create_handle()
    try:
        assert [L.jm_amddec_set_option(h, b"verify_md5", v) for v in (-1, 2, 0, 1)] == [-1, -1, 0, 0]
        assert [L.jm_amddec_set_option(h, b"verify_hash", v) for v in (3, 2)] == [-1, 0]                     # its range stays 0..2
        L.jm_amddec_set_option(h, b"parse_only", 1)
        assert L.jm_amddec_init(1, 1, None, 0, h) == 0
        assert L.jm_amddec_set_option(h, b"verify_md5", 1) == -1 and L.jm_amddec_set_option(h, b"verify_md5", 0) == -1          # after init
    finally:
        L.jm_amddec_deinit(h)
