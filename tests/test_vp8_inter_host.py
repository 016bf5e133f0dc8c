"""VP8 inter frames (codec_type 5, options vp8 + vp8_inter) without a GPU.

There is NO independent pin for inter frames: no VP8 inter encoder or decoder was available (libwebp does key frames only).  Inter frames are held the
way MPEG-2 is: RFC 6386 typed out twice -- tests/vp8_inter_ref.py in numpy, vp8_syntax.cpp / vp8_recon.h in C++ -- scripted streams, structural checks
of the tables, and answers worked out here that no decoder computed.  A table typed wrong the same way twice would pass.

Here:
  * the product's host path -- splitter, frame header, bool decoder, modes, vectors, tokens with the stream's state (vp8_syntax.cpp) and the lane
    routines of vp8_recon.h playing k_vp8_inter, k_vp8_recon and k_vp8_filter on the CPU in the kernels' order (tests/native/vp8_inter_check.cpp, built
    with g++) -- equals the restatement on every scripted stream, the damaged ones included, in every sample and every count; its tables equal the
    restatement's;
  * the analytic answers (a) - (d) below; the coverage conditions, asserted from the restatement's info: a class nobody visits fails;
  * option gating and refusals through the library; parse-only handles report the new statistics; the job digest does not depend on chunking or on
    the number of parse workers;
  * the stand-alone sanitizer program tools/vp8_inter_asan.cpp builds and ends clean, in both of its modes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import scripted_vp8 as S
import scripted_vp8_inter as SI
import vp8_inter_ref as I
import vp8_ref as R
from jmcodec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FEATURES = dict(SI.feature_cases())
_DAMAGED = dict(SI.damaged_cases())
_SCRIPTED = dict(_FEATURES, **_DAMAGED, long_golden=SI.long_golden_stream(), **{"sized_%dx%d" % s: SI.sized_stream(*s, seed=s[0] * s[1]) for s in SI.SIZES})
_REF = {}


def ref(name, data):
    """the restatement's frames (out_fmt 0), its info and every decoded frame's planes, computed once per stream"""
    if name not in _REF:
        info, planes = {}, []
        _REF[name] = (I.decode_stream(data, 0, info, planes), info, planes)
    return _REF[name]


@pytest.fixture(scope="module")
def native():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libvp8_inter_check.so")
    csrc = os.path.join(ROOT, "jmcodec_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "vp8_inter_check.cpp"), os.path.join(csrc, "vp8_syntax.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("vp8_syntax.h", "vp8_recon.h", "vp8_jobs.h", "jpeg_recon.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so] + srcs)
    l = C.CDLL(so)
    l.v8i_decode.restype = C.c_long
    l.v8i_decode.argtypes = [C.c_char_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    l.v8i_error.restype = C.c_char_p
    l.v8i_table.argtypes = [C.c_int, C.c_long]
    l.v8i_predict.argtypes = [C.c_char_p] + [C.c_int] * 10 + [C.c_void_p]

    def decode(data, chunk=0, inter=1, every=0):
        """chunk: bytes per call, 0 = all at once; a list of frames = one frame per call -> (n, [(NV12 bytes, w, h)], stats)"""
        if isinstance(data, list):
            data, chunk = b"".join(len(f).to_bytes(4, "little") + f for f in data), -1
        out_buf, dims, st = C.create_string_buffer(1 << 23), (C.c_int * 256)(), (C.c_longlong * 16)()
        n = l.v8i_decode(data, len(data), chunk, inter, every, out_buf, len(out_buf), dims, 128, st)
        frames, o = [], 0
        for i in range(max(n, 0)):
            w, h = dims[2 * i], dims[2 * i + 1]
            frames.append((out_buf.raw[o:o + w * h * 3 // 2], w, h))
            o += w * h * 3 // 2
        keys = ("errors", "key_frames", "inter_frames", "hidden", "empty", "bpred_mbs", "skipped_mbs", "job_bytes", "golden_refs", "altref_refs", "split_mbs",
                "intra_in_inter", "digest")
        return n, frames, dict(zip(keys, st))
    decode.lib = l
    return decode


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
def test_restatement_tables_have_the_rfcs_structure():
    I.check_tables()


def _cpp_table(l, which):
    out, i = [], 0
    while True:
        v = l.v8i_table(which, i)
        if v < 0:
            return out
        out.append(v)
        i += 1


def test_cpp_tables_equal_the_restatements(native):
    l = native.lib
    flat = lambda t: [int(v) for v in np.array(t).reshape(-1)]      # noqa: E731
    assert _cpp_table(l, 0) == I.YMODE_PROB and _cpp_table(l, 1) == I.UV_MODE_PROB and _cpp_table(l, 2) == I.BMODE_PROB
    assert _cpp_table(l, 3) == flat(I.MODE_CONTEXTS) and _cpp_table(l, 4) == flat(I.SUB_MV_REF_PROBS) and _cpp_table(l, 5) == I.SPLIT_PROBS
    assert _cpp_table(l, 6) == flat(I.DEFAULT_MV_PROBS) and _cpp_table(l, 7) == flat(I.MV_UPDATE_PROBS) and _cpp_table(l, 8) == flat(I.SPLITS)
    for which, t in ((9, I.YMODE_TREE), (10, I.MV_REF_TREE), (11, I.SUB_MV_REF_TREE), (12, I.SPLIT_TREE), (13, I.SMALL_MV_TREE)):
        assert [v - 128 for v in _cpp_table(l, which)] == t
    for k in (0, 1):
        for f in range(8):
            assert [v - 128 for v in _cpp_table(l, 14 + 16 * k + f)] == I.taps(k, f), (k, f)


# ---- the product's host path = the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_SCRIPTED))
def test_host_path_equals_the_restatement(native, name):
    data = _SCRIPTED[name]
    want, info, _ = ref(name, data)
    n, frames, st = native(data)
    assert n == len(want), native.lib.v8i_error()
    for i, (f, w) in enumerate(zip(frames, want)):
        assert f == w, f"frame {i} of {n}"
    assert (st["errors"], st["key_frames"], st["inter_frames"], st["hidden"], st["empty"]) == (info["errors"], info["key_frames"], info["inter_frames"], info["hidden"], info["empty"])
    assert (st["golden_refs"], st["altref_refs"], st["split_mbs"], st["intra_in_inter"]) == (info["golden_refs"], info["altref_refs"], info["split_mbs"], info["intra_in_inter"])
    assert (st["bpred_mbs"], st["skipped_mbs"]) == (info["bpred_mbs"], info["skipped_mbs"])
    assert (st["errors"] > 0) == (name in _DAMAGED)


def test_chunking_and_frame_per_call(native):
    data = _SCRIPTED["sized_48x32"]
    whole = native(data)
    assert native(data, chunk=7)[1:] == whole[1:] and native(data, chunk=1)[1:] == whole[1:] and native(R.split_ivf(data))[1:] == whole[1:]


def test_key_frame_job_lists_are_what_they_were(native):
    """with the state threaded through, a key-frame stream decodes to the key-frame restatement's frames, with inter frames allowed and refused alike
    (that the records and entries are byte for byte those of a handle without the option: test_key_frame_digest_does_not_depend_on_the_option)"""
    for data in (S.sized_stream(53, 37, seed=3, frames=3), dict(S.feature_cases())["segments_delta"], dict(S.feature_cases())["lf_deltas"]):
        a, b = native(data, inter=1), native(data, inter=0)
        assert a == b and a[2]["inter_frames"] == 0
        assert [f for f, _, _ in a[1]] == [f for f, _, _ in R.decode_stream(data, 0)]


# ---- analytic answers that no decoder computed ----------------------------------------------------------------------------------------------------
def test_zero_vector_without_residual_returns_the_referenced_frame(native):
    """(a) ZEROMV, no residual, filter off: the frame IS the referenced one -- last, golden and altref in turn, after each copy_buffer value and after
    refresh_last 0.  Frames 2, 3 and 5 must equal key frame 0, which libwebp's arithmetic pins."""
    data = SI.reference_stream()
    _, _, planes = ref("references", data)
    n, frames, _ = native(data)
    assert n == 14
    for i, j in SI.REFERENCE_EXPECTED.items():
        assert frames[i][0] == frames[j][0], (i, j)
        assert all((a == b).all() for a, b in zip(planes[i], planes[j])), (i, j)
    assert frames[1][0] != frames[0][0] and frames[4][0] != frames[0][0] and frames[7][0] != frames[4][0]
    key = R.decode_stream(R.ivf(R.split_ivf(data)[:1]), 0)[0][0]        # the key frame alone, by the key-frame restatement
    assert frames[0][0] == key == frames[2][0] == frames[3][0] == frames[5][0]


def _plane(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def _predict(native, plane, mbx, mby, mv, cmv, interp, split=0):
    h, w = plane.shape
    out = C.create_string_buffer(256 + 64)
    native.lib.v8i_predict(plane.tobytes(), w, h, mbx, mby, mv[0], mv[1], cmv[0], cmv[1], interp, split, out)
    b = np.frombuffer(out.raw, np.uint8)
    return b[:256].reshape(16, 16).astype(int), b[256:].reshape(8, 8).astype(int)


def test_whole_sample_vectors_are_a_slice_of_the_replicated_reference(native):
    """(b) a whole-sample vector copies: the prediction is a numpy slice of the edge-replicated plane, wherever it points -- inside, across each border,
    a whole picture beyond it -- for six-tap and bilinear, whole and split"""
    w, h = 48, 32
    p = _plane(w, h, 1)
    pad = 600
    big = np.pad(p, pad, mode="edge")
    for interp in (0, 1):
        for split in (0, 1):
            for mbx, mby, dx, dy in ((1, 0, 3, 2), (0, 0, -5, -9), (2, 1, 20, 17), (1, 1, -100, 4), (1, 0, 7, -77), (0, 1, 255, 255), (2, 0, -255, -255),
                                     (1, 1, 500, -500)):
                y, c = _predict(native, p, mbx, mby, (8 * dx, 8 * dy), (8 * dx, 8 * dy), interp, split)
                x0, y0 = pad + mbx * 16 + dx, pad + mby * 16 + dy
                assert (y == big[y0:y0 + 16, x0:x0 + 16]).all(), (interp, split, mbx, mby, dx, dy)
                # (the chroma plane of v8i_predict is the top-left quarter of the same plane)
                cb = np.pad(p[:h // 2, :w // 2], pad, mode="edge")
                x0, y0 = pad + mbx * 8 + dx, pad + mby * 8 + dy
                assert (c == cb[y0:y0 + 8, x0:x0 + 8]).all(), (interp, split, mbx, mby, dx, dy)


def test_impulse_returns_the_tap_row_and_a_constant_stays_constant(native):
    """(c) an impulse of 128 on black under a horizontal (vertical) fraction f returns the taps of f mirrored along the row (column): sample x sees the
    impulse at distance d = xi - x with tap[d + 2], times 128, +64 >> 7 = the tap itself, clamped at 0.  A constant plane stays the constant under
    every fraction, both filters, whole and split."""
    w, h = 48, 32
    for interp in (0, 1):
        for f in range(8):
            t = I.taps(interp, f)
            p = np.zeros((h, w), np.uint8)
            p[8, 24] = 128
            for split in (0, 1):
                y, c = _predict(native, p, 1, 0, (f, 0), (f, 0), interp, split)        # luma block covers x 16..31, y 0..15
                want = np.zeros((16, 16), int)
                for x in range(16):
                    d = 24 - (16 + x)
                    if -2 <= d <= 3:
                        want[8, x] = max(0, min(255, (128 * t[d + 2] + 64) >> 7))
                assert (y == want).all(), (interp, f, split)
                y, _ = _predict(native, p, 1, 0, (0, f), (0, f), interp, split)
                want = np.zeros((16, 16), int)
                for r in range(16):
                    d = 8 - r
                    if -2 <= d <= 3:
                        want[r, 8] = max(0, min(255, (128 * t[d + 2] + 64) >> 7))
                assert (y == want).all(), (interp, f, split)
    for value in (0, 1, 77, 254, 255):
        p = np.full((h, w), value, np.uint8)
        for interp in (0, 1):
            for fx in range(8):
                for fy in range(8):
                    y, c = _predict(native, p, 2, 1, (fx + 8 * 3, fy - 8 * 40), (fy, fx), interp, (fx + fy) & 1)
                    assert (y == value).all() and (c == value).all(), (value, interp, fx, fy)
    # and the restatement's own predictor gives the same two answers
    p = np.zeros((h, w), np.uint8)
    p[8, 24] = 128
    assert I.predict_block(p, 16, 0, 16, 4, 0, 0)[8, 5:11].tolist() == [max(0, v) for v in I.SIXTAP[4][::-1]]
    assert (I.predict_block(np.full((h, w), 200, np.uint8), 0, 0, 16, 3 - 800, 5 + 800, 0) == 200).all()


def test_refresh_entropy_probs_0_restores_the_probabilities(native):
    """(d) frame 1 changes coefficient, vector and mode probabilities with refresh_entropy_probs 0; frame 2 is written under the probabilities from
    before frame 1 and decodes without damage only under them.  A decoder that kept frame 1's set is shown to read frame 2 differently: the restatement
    with the restore switched off does not give the same pictures."""
    data = SI.entropy_stream()
    want, info, _ = ref("refresh_entropy_0", data)
    n, frames, st = native(data)
    assert n == 5 and frames == want and st["errors"] == 0 and info["mv_prob_updates"] == 10
    assert info["entropy_restored"] == 2          # (the key frame, whose refresh_entropy_probs is 0 too, and frame 1)
    d = I.InterDecoder()
    broken = []
    for k, f in enumerate(R.split_ivf(data)):
        r = d.decode_frame(f)
        if k == 1:      # put two of frame 1's updates back, as a decoder without the restore would have them
            d.coef[0][1][0][0], d.mvp[0][0] = 3, 10
        broken.append(R.nv12(r[0], r[1], r[2])[0].tobytes())
    assert broken[:2] == [f for f, _, _ in frames][:2] and broken[2] != frames[2][0]


# ---- coverage: what the scripted streams visit, from the restatement's info ------------------------------------------------------------------------
def _union(key):
    out = set()
    for name, data in _SCRIPTED.items():
        out |= ref(name, data)[1][key]
    return out


def test_scripted_streams_visit_every_class():
    assert _union("chroma_fracs") == {(x, y) for x in range(8) for y in range(8)}
    assert _union("luma_fracs") == {(x, y) for x in range(0, 8, 2) for y in range(0, 8, 2)}
    assert _union("beyond") == {"left", "right", "top", "bottom"}
    assert max(ref(n, d)[1]["max_long"] for n, d in _SCRIPTED.items()) == 1023
    assert _union("splits") == {0, 1, 2, 3}
    assert _union("sub_mv") == {(c, l) for c in range(5) for l in range(4)}
    assert _union("ref_bias") >= {(1, 0), (2, 0), (2, 1), (3, 0), (3, 1)}
    assert _union("inter_versions") == {0, 1, 2, 3}
    assert _union("mv_modes") == {0, 1, 2, 3, 4}
    assert _union("intra_beside_inter") == {R.DC_PRED, R.V_PRED, R.H_PRED, R.TM_PRED, R.B_PRED} and _union("bmodes_beside_inter") == set(range(10))
    assert _union("lf_ref_classes") == {0, 1, 2, 3} and _union("lf_mode_classes") >= {0, 1, 2, 3}
    assert _union("inter_levels") >= {14, 15, 19, 20, 39, 40}
    assert {c[0] for c in _union("copy_flags")} == {0, 1, 2} == {c[1] for c in _union("copy_flags")}
    assert _union("refresh_last") == {0, 1} and _union("refresh") == {0, 1}
    assert sum(ref(n, d)[1]["kept_map_frames"] for n, d in _SCRIPTED.items()) >= 2
    assert ref("long_golden", _SCRIPTED["long_golden"])[1]["hidden"] == 1


# ---- through the library ------------------------------------------------------------------------------------------------------------------------
STATS = ("errors", "frames", "failed", "i_pictures", "p_pictures", "job_digest", "job_bytes", "vp8_key_frames", "vp8_hidden_frames", "vp8_bpred_mbs",
         "vp8_skipped_mbs", "vp8_inter_frames", "vp8_golden_refs", "vp8_altref_refs", "vp8_split_mbs", "vp8_intra_in_inter_mbs")


def parse(data, chunks=None, **opt):
    with api.JmAmdDec(5, 1, options=dict(dict(vp8=1, vp8_inter=1, parse_only=1, sync=1), **opt)) as d:
        n = d.decode_stream(data, keep=False, chunks=chunks if chunks is not None else [data])
        return n, {k: d.stat(k) for k in STATS}


def test_option_gating_and_refusals():
    with api.JmAmdDec(5, 1, options=dict(vp8=1, vp8_inter=1, parse_only=1)):
        pass
    for codec, opts in ((0, dict(vp8_inter=1)), (5, dict(vp8_inter=1)), (4, dict(vp8_inter=1)), (1, dict(vp8_inter=1))):
        with pytest.raises(RuntimeError, match="option vp8_inter is only available for VP8"):
            api.JmAmdDec(codec, 1, options=dict(opts, parse_only=1))
    with pytest.raises(RuntimeError, match=r"and 5 \(VP8\) for key frames with option vp8 1"):      # init(5) without vp8: the text it always had
        api.JmAmdDec(5, 1, options=dict(parse_only=1))
    data = S.inter_after_key()
    with api.JmAmdDec(5, 1, options=dict(vp8=1, parse_only=1, sync=1)) as d:                         # the option off: the old message
        with pytest.raises(RuntimeError, match="VP8 inter frames are not built"):
            d.decode_stream(data, keep=False, chunks=[data])
    n, st = parse(data)       # (its second frame is a key frame's body behind an inter tag: it parses as damage, and decodes)
    info = {}
    assert n == 2 == len(I.decode_stream(data, 0, info))
    assert (st["vp8_key_frames"], st["vp8_inter_frames"], st["i_pictures"], st["p_pictures"], st["errors"], st["failed"]) == (1, 1, 1, 1, info["errors"], 0)
    first = dict((n, s) for n, s, _ in S.refused_cases())["first_frame_inter"]
    with api.JmAmdDec(5, 1, options=dict(vp8=1, vp8_inter=1, parse_only=1, sync=1)) as d:
        with pytest.raises(RuntimeError, match="VP8: the first frame is not a key frame"):
            d.decode_stream(first, keep=False, chunks=[first])


def test_parse_only_stats_equal_the_restatements():
    for name in ("references", "sub_mv_refs", "filter_levels_and_deltas", "long_golden", "truncated_tokens"):
        data = _SCRIPTED[name]
        want, info, _ = ref(name, data)
        n, st = parse(data)
        assert n == len(want) == st["frames"] and st["failed"] == 0, name
        assert (st["vp8_key_frames"], st["vp8_inter_frames"], st["p_pictures"], st["vp8_hidden_frames"]) == (info["key_frames"], info["inter_frames"], info["inter_frames"], info["hidden"])
        assert (st["vp8_golden_refs"], st["vp8_altref_refs"], st["vp8_split_mbs"], st["vp8_intra_in_inter_mbs"]) == (info["golden_refs"], info["altref_refs"], info["split_mbs"], info["intra_in_inter"])
        assert (st["vp8_bpred_mbs"], st["vp8_skipped_mbs"], st["errors"] > 0) == (info["bpred_mbs"], info["skipped_mbs"], info["errors"] > 0)


def test_key_frame_digest_does_not_depend_on_the_option():
    data = S.sized_stream(48, 32, seed=5, frames=4)
    with api.JmAmdDec(5, 1, options=dict(vp8=1, parse_only=1, sync=1, job_digest=1)) as d:
        d.decode_stream(data, keep=False, chunks=[data])
        off = (d.stat("job_digest"), d.stat("job_bytes"))
    n, st = parse(data, job_digest=1)
    assert (st["job_digest"], st["job_bytes"]) == off and n == 4


def test_job_digest_is_invariant_under_chunking():
    data = _SCRIPTED["sized_53x37"]
    forms = (None, [data[i:i + 7] for i in range(0, len(data), 7)], R.split_ivf(data))
    assert len({parse(data, chunks, job_digest=1)[1]["job_digest"] for chunks in forms}) == 1


_WORKER = """
import sys
sys.path[:0] = [%r, %r]
import scripted_vp8_inter as SI
from jmcodec_amd import api
out = []
for data in (SI.sized_stream(80, 272, seed=7), SI.long_golden_stream()):
    with api.JmAmdDec(5, 1, options=dict(vp8=1, vp8_inter=1, parse_only=1, job_digest=1)) as d:
        n = d.decode_stream(data, keep=False, chunks=[data])
        out.append((n, d.stat("job_digest"), d.stat("job_bytes"), d.stat("threads")))
print(out)
"""


def test_digest_is_equal_with_one_parse_worker_and_with_many():
    """the pool's size is fixed per process (JM_AMD_DEC_THREADS): two fresh processes, without option sync, so that pictures overlap where they can"""
    got = []
    for threads in ("1", "24"):
        env = dict(os.environ, JM_AMD_DEC_THREADS=threads)
        r = subprocess.run([sys.executable, "-c", _WORKER % (ROOT, os.path.join(ROOT, "tests"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        got.append(eval(r.stdout.strip().splitlines()[-1]))
    assert [g[:3] for g in got[0]] == [g[:3] for g in got[1]] and got[0][0][3] != got[1][0][3], got


# ---- the sanitizer program -------------------------------------------------------------------------------------------------------------------------
def test_vp8_inter_asan_builds_and_runs_clean(tmp_path):
    """tools/vp8_inter_asan.cpp: a stand-alone host program (its own main) under AddressSanitizer / UBSan -- the lane routines over exact-size surfaces and
    reference windows at every border with arbitrary 16-bit vectors, on valid and damaged job lists; and the inter parse on mutated streams, a bounded count"""
    out = tmp_path / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "vp8_inter_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]

    def clean(r):
        assert r.returncode == 0, r.stdout[-4000:]
        assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
    r = subprocess.run([str(out / "vp8_inter_asan"), "1", "6"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    clean(r)
    assert "ok: 6 trials, 36 pictures" in r.stdout
    for i, name in enumerate(("sub_mv_refs", "far_vectors", "sized_53x37")):
        path = tmp_path / ("a%d.ivf" % i)
        path.write_bytes(_SCRIPTED[name])
        r = subprocess.run([str(out / "vp8_inter_asan"), str(i + 1), "100", str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        clean(r)
        assert "ok: 100 trials" in r.stdout
