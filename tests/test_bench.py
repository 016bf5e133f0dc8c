"""bench.py's plain run and its outputs: a plain run times the steps and prints the headline line (the untimed legs and the oracle check wait
for --full); --dump-outputs writes what the timed path returned in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
EXTRA_LEGS = ("c4_slice", "c2_4k", "c3_4k")             # the other BASELINE configurations (the headline workload only)
DEVICE_LEGS = ("cpu_baseline", "single_stream", "c0_pushpull", "device_resident_output")     # need decoded pixels: never under --parse-only


def _bench(args, env, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_nothing_else(tmp_path):
    """Without --full the headline workload's extra legs stay out, where the same invocation with --full adds them (JM_BENCH_TEST_LEGS: their code
    path at a toy size, no GPU), and --steps sets the timed steps: frames = streams x frames x steps."""
    env = dict(os.environ, JM_BENCH_CACHE=str(tmp_path), JM_BENCH_TEST_LEGS="176x144")
    args = ["--steps", "3", "--warmup", "1", "--parse-only", "--streams", "2", "--frames", "8", "--width", "176", "--height", "144"]
    d = _bench(args, env)
    for k in HEADLINE:
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["frames"] == 2 * 8 * 3
    assert d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["bit_exact"] is None
    for k in EXTRA_LEGS:
        assert k not in d, k
    full = _bench(args + ["--full"], env)
    assert full["steps"] == 3 and full["frames"] == d["frames"]
    for k in EXTRA_LEGS:
        assert k in full and "error" not in full[k], k


@pytest.mark.gpu
def test_dump_outputs_are_the_frames_the_timed_path_returned(tmp_path, oracle):
    """--dump-outputs at a toy size: the last frame each handle returned in the timed steps (Baseline I/P, so display frame F - 1 of its stream) equals
    the CPU oracle's, in the seeded sample and whole; the frame counts are those of the timed steps."""
    from tools import streams
    S, F, K, w, h = 2, 30, 2, 176, 144
    out = tmp_path / "out"
    env = dict(os.environ, JM_BENCH_CACHE=str(tmp_path))
    d = _bench(["--steps", str(K), "--warmup", "1", "--streams", str(S), "--frames", str(F), "--width", str(w), "--height", str(h),
                "--dump-outputs", str(out)], env)
    assert d["steps"] == K and d["frames"] == S * F * K
    assert d["bit_exact"] is None and d["frames_checked"] == 0           # a plain run: no oracle check, no untimed legs
    for k in DEVICE_LEGS:
        assert k not in d, k
    files = {p.name: np.load(p) for p in out.iterdir()}
    assert set(files) == {"frame_sample.npy", "frame_sample_index.npy", "frames_returned.npy", "last_frame_stream0.npy"}
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    for a in files.values():
        assert a.dtype in (np.float32, np.float64)
    fb = w * h * 3 // 2
    idx = files["frame_sample_index.npy"].astype(np.int64)
    assert files["frames_returned.npy"].tolist() == [F * K] * S
    assert files["frame_sample.npy"].shape == (S, len(idx))
    for i in range(S):
        yuv, n, _, _ = oracle.decode(streams.generate(**streams.config_c1(stream_id=i, frames=F, width=w, height=h)), 1)
        last = np.frombuffer(yuv[(n - 1) * fb:n * fb], np.uint8)
        assert np.array_equal(files["frame_sample.npy"][i], last[idx].astype(np.float32)), f"stream {i}"
        if i == 0:
            assert np.array_equal(files["last_frame_stream0.npy"], last.astype(np.float32))


@pytest.mark.gpu
def test_full_run_checks_against_the_oracle_and_adds_the_legs(tmp_path):
    """The same toy invocation with --full: the timed configuration is checked bit-exactly against the CPU oracle and the untimed legs are there."""
    env = dict(os.environ, JM_BENCH_CACHE=str(tmp_path))
    d = _bench(["--steps", "2", "--warmup", "1", "--streams", "2", "--frames", "30", "--width", "176", "--height", "144", "--full"], env)
    assert d["steps"] == 2 and d["frames"] == 2 * 30 * 2
    assert d["bit_exact"] is True and d["frames_checked"] > 0 and d["decode_errors"] == 0
    for k in DEVICE_LEGS:
        assert k in d, k
