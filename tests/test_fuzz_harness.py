"""The sanitizer harness of the host pipeline (tools/fuzz_host.cpp: parse-only mode under AddressSanitizer / UBSan) links against the stand-ins of
tools/fuzz_stubs.h instead of the device objects.  Every launcher the host sources call needs a stand-in there, and nothing else built the harness: a
kernel added without one went unnoticed.  Built here into a temporary directory and run for a few trials on one short stream per codec."""
import os
import subprocess

import pytest

from tools import streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_fuzz_host_asan_links_and_runs_clean(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc: the harness is built with it")
    out = tmp_path / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "fuzz_host_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    cases = {"a.h264": (0, streams.generate(width=64, height=48, frames=6, gop=3, mode=1, num_ref=2, seed=0x4A4D0901, cabac=1, bframes=1)),
             "a.h265": (1, streams.generate_hevc(width=64, height=64, frames=6, gop=4, num_ref=2, seed=0x4A4D0902))}
    for name, (codec, data) in cases.items():
        path = tmp_path / name
        path.write_bytes(data)
        r = subprocess.run([str(out / "fuzz_host_asan"), str(path), "1", "8", str(codec)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-4000:]
        assert "ok: 8 trials" in r.stdout
        assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
