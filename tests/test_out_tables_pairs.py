"""Field-rate pairs in the output stage's job tables (jmcodec_amd/csrc/out_tables.h, no GPU): a pair is one k_deint entry with two destinations,
counts as two frames and 3 / 2 of a frame's bytes, and -- for a scaled / RGB handle -- gets two scratch surfaces in queue order, each rounded to
256 bytes, which the two jobs behind it read.  Frames without a second destination are laid out as before (tests/test_out_tables.py)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = lambda i: 0x1000000 + 0x10000 * i        # noqa: E731  (the check's output slots)
SRC = 0x500000


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libout_tables_pairs_check.so")
    src = os.path.join(ROOT, "tests", "native", "out_tables_pairs_check.cpp")
    hdrs = [os.path.join(ROOT, "jmcodec_amd", "csrc", h) for h in ("out_tables.h", "jobs.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-missing-field-initializers", "-o", so, src])
    l = C.CDLL(so)
    l.otp_run.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    l.otp_run.restype = None
    return l


def _run(lib, pairs, feeds, w=100, h=52, pitch=128, scratch=0x40000000, deint_bytes=7800):
    n = len(pairs)
    out, info = (C.c_int64 * (4 * n))(), (C.c_int64 * 10)()
    lib.otp_run(n, (C.c_int * n)(*pairs), feeds, w, h, pitch, scratch, deint_bytes, out, info)
    keys = ("deint", "scale", "rgb", "pairs", "n_deint", "alg_deint", "scratch_used", "bytes_needed", "frames", "ok")
    return [tuple(out[4 * k:4 * k + 4]) for k in range(n)], dict(zip(keys, info))


PAIRS = [1, 0, 1, 1, 0]


def test_plain_handle_pairs_are_one_entry_two_frames(lib):
    rows, info = _run(lib, PAIRS, 0)
    assert rows == [(SLOT(2 * k), SLOT(2 * k + 1) if p else 0, -1, -1) for k, p in enumerate(PAIRS)]
    assert info["deint"] == 5 and info["pairs"] == 3 and info["frames"] == 8 and info["n_deint"] == 8
    assert info["alg_deint"] == 3 * (7800 * 3 // 2) + 2 * 7800
    assert info["scratch_used"] == 0 and info["bytes_needed"] == 0 and info["ok"] == 1


@pytest.mark.parametrize("feeds", [1, 2])
def test_scaled_and_rgb_pairs_get_two_scratch_surfaces_in_queue_order(lib, feeds):
    base, surf = 0x40000000, (128 * 52 * 3 // 2 + 255) // 256 * 256
    rows, info = _run(lib, PAIRS, feeds, scratch=base)
    at, want = base, []
    for p in PAIRS:
        want.append((at, at + surf if p else 0, at, at + surf if p else -1))
        at += surf * (2 if p else 1)
    assert rows == want
    assert info["scratch_used"] == info["bytes_needed"] == 8 * surf
    assert info["deint"] == 5 and info["pairs"] == 3 and info["n_deint"] == 8 and info["frames"] == 8
    assert info["scale" if feeds == 1 else "rgb"] == 8 and info["rgb" if feeds == 1 else "scale"] == 0 and info["ok"] == 1


def test_without_scratch_both_jobs_of_a_pair_read_the_picture(lib):
    rows, info = _run(lib, [1, 0], 1, scratch=0)
    assert rows == [(-1, -1, SRC, SRC), (-1, -1, SRC, -1)]
    assert info["ok"] == 0 and info["deint"] == 0 and info["scratch_used"] == 0


def test_no_pairs_is_the_layout_of_before(lib):
    rows, info = _run(lib, [0, 0, 0], 0)
    assert rows == [(SLOT(2 * k), 0, -1, -1) for k in range(3)]
    assert info["pairs"] == 0 and info["frames"] == 3 and info["n_deint"] == 3 and info["alg_deint"] == 3 * 7800
