"""VP8 key frames (codec_type 5) without a GPU.

VP8's decoding process is exact integer arithmetic (RFC 6386), and libwebp -- an encoder and a decoder nobody in this project wrote -- pins it:
tests/golden/vp8 holds pictures from libwebp's encoder with libwebp's own decode of each as Y, U and V planes (tests/golden/make_golden_vp8.py).
Here, from the committed files alone (no Pillow):
  * the Python restatement tests/vp8_ref.py equals libwebp's planes in every sample of every fixture, and the fixtures together with
    scripted_vp8.feature_cases() leave no syntax feature unvisited;
  * the product's host path -- splitter, frame header, bool decoder, modes, tokens (vp8_syntax.cpp) and the lane routines of vp8_recon.h playing both
    kernels on the CPU in the kernels' wavefront order (tests/native/vp8_check.cpp, built with g++) -- equals libwebp's planes on every fixture and the
    restatement on every scripted stream, the damaged ones included, bit for bit; its tables equal the restatement's;
  * refusals with their text, parse-only handles through the library, every chunking of the input;
  * the two stand-alone sanitizer programs tools/vp8_asan.cpp and tools/fuzz_vp8.cpp build and end clean."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import scripted_vp8 as S
import vp8_ref as R
from jmcodec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vp8")
FIXTURES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLDEN, "*.webp")))
_FEATURES = dict(S.feature_cases())
_DAMAGED = dict(S.damaged_cases())
_SCRIPTED = dict(_FEATURES, **_DAMAGED, size_change=S.size_change(), **{"sized_%dx%d" % s: S.sized_stream(*s, seed=s[0] * s[1]) for s in S.SIZES})
_REF = {}


def ref(name, data):
    if name not in _REF:
        info = {}
        _REF[name] = (R.decode_stream(data, 0, info), info)
    return _REF[name]


def fixture(name):
    with open(os.path.join(GOLDEN, name + ".webp"), "rb") as f:
        data = f.read()
    return data, tuple(np.load(os.path.join(GOLDEN, "%s.%s.npy" % (name, p))) for p in "yuv")


@pytest.fixture(scope="module")
def native():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libvp8_check.so")
    csrc = os.path.join(ROOT, "jmcodec_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "vp8_check.cpp"), os.path.join(csrc, "vp8_syntax.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("vp8_syntax.h", "vp8_recon.h", "vp8_jobs.h", "jpeg_recon.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so] + srcs)
    l = C.CDLL(so)
    l.v8c_decode.restype = C.c_long
    l.v8c_decode.argtypes = [C.c_char_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    l.v8c_error.restype = C.c_char_p
    l.v8c_table.argtypes = [C.c_int, C.c_long]

    def decode(data, chunk=0):
        """chunk: bytes per call, 0 = all at once; a list of frames = one frame per call -> (n, [(NV12 bytes, w, h)], stats)"""
        if isinstance(data, list):
            data, chunk = b"".join(len(f).to_bytes(4, "little") + f for f in data), -1
        out_buf, dims, st = C.create_string_buffer(1 << 23), (C.c_int * 128)(), (C.c_longlong * 12)()
        n = l.v8c_decode(data, len(data), chunk, out_buf, len(out_buf), dims, 64, st)
        frames, o = [], 0
        for i in range(max(n, 0)):
            w, h = dims[2 * i], dims[2 * i + 1]
            frames.append((out_buf.raw[o:o + w * h * 3 // 2], w, h))
            o += w * h * 3 // 2
        keys = ("errors", "key_frames", "hidden", "empty", "partitions", "segments", "filter_type", "color_space", "scale", "bpred_mbs", "skipped_mbs", "job_bytes")
        return n, frames, dict(zip(keys, st))
    decode.lib = l
    return decode


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
def _cpp_table(l, which):
    out, i = [], 0
    while True:
        v = l.v8c_table(which, i)
        if v < 0:
            return out
        out.append(v)
        i += 1


def test_cpp_tables_equal_the_restatements(native):
    l = native.lib
    flat = lambda t: [int(v) for v in np.array(t).reshape(-1)]      # noqa: E731
    assert _cpp_table(l, 0) == R.DC_Q
    ac = _cpp_table(l, 1)
    assert [ac[2 * i] | ac[2 * i + 1] << 8 for i in range(128)] == R.AC_Q
    assert _cpp_table(l, 2) == flat(R.DEFAULT_COEF_PROBS) and _cpp_table(l, 3) == flat(R.COEF_UPDATE_PROBS)
    assert _cpp_table(l, 4) == R.KF_YMODE_PROB and _cpp_table(l, 5) == R.KF_UV_MODE_PROB and _cpp_table(l, 6) == flat(R.KF_BMODE_PROBS)
    for which, t in ((7, R.KF_YMODE_TREE), (8, R.UV_MODE_TREE), (9, R.BMODE_TREE), (10, R.SEGMENT_TREE)):
        assert [v - 128 for v in _cpp_table(l, which)] == t
    # the product numbers the tokens 0..4 values, 5..10 categories, 11 end of block; the restatement numbers them DCT_0 .. DCT_EOB = 0 .. 11 alike
    assert [v - 128 for v in _cpp_table(l, 11)] == R.COEF_TREE and R.DCT_EOB == 11 and R.DCT_CAT1 == 5
    assert _cpp_table(l, 12) == R.COEF_BANDS and _cpp_table(l, 13) == R.ZIGZAG and _cpp_table(l, 15) == R.CAT_BASE
    cats = _cpp_table(l, 14)
    assert [[p for p in cats[12 * c:12 * c + 12] if p] for c in range(6)] == R.CAT_PROBS


def test_tables_have_the_rfcs_shape_and_anchors():
    assert np.array(R.DEFAULT_COEF_PROBS).shape == (4, 8, 3, 11) and np.array(R.COEF_UPDATE_PROBS).shape == (4, 8, 3, 11)
    assert np.array(R.KF_BMODE_PROBS).shape == (10, 10, 9)
    assert R.DC_Q[0] == 4 and R.DC_Q[127] == 157 and R.AC_Q[0] == 4 and R.AC_Q[127] == 284 and sorted(R.DC_Q) == R.DC_Q and sorted(R.AC_Q) == R.AC_Q
    assert sorted(R.ZIGZAG) == list(range(16)) and R.COEF_BANDS[0] == 0 and R.COEF_BANDS[15] == 7
    # luma after Y2 never codes position 0: its band 0 is the unused 128s
    assert R.DEFAULT_COEF_PROBS[0][0] == [[128] * 11] * 3
    for tree, leaves in ((R.KF_YMODE_TREE, 5), (R.UV_MODE_TREE, 4), (R.BMODE_TREE, 10), (R.SEGMENT_TREE, 4), (R.COEF_TREE, 12)):
        assert sorted(-v for v in tree if v <= 0) == list(range(leaves)) and sorted(v for v in tree if v > 0) == list(range(2, len(tree), 2))


# ---- arithmetic anchors worked out here -------------------------------------------------------------------------------------------------------------
def test_transforms_on_hand_cases():
    assert R.iwht([8] + [0] * 15) == [1] * 16 and R.iwht([-8] + [0] * 15) == [-1] * 16 and R.iwht([0] * 16) == [0] * 16
    assert R.idct([80] + [0] * 15) == [10] * 16 and R.idct([-3] + [0] * 15) == [0] * 16 and R.idct([-4] + [0] * 15) == [0] * 16 and R.idct([-5] + [0] * 15) == [-1] * 16
    # a lone horizontal AC of 64: (64 + (64 * 20091 >> 16)) = 83, (64 * 35468 >> 16) = 34 -> rows of (83, 34, -34, -83) + 4 >> 3
    assert R.idct([0, 64] + [0] * 14) == [10, 4, -4, -10] * 4


def test_filter_limits_and_hev_thresholds():
    assert R.filter_limits(63, 0) == (63, 189, 193, 2) and R.filter_limits(40, 0)[3] == 2 and R.filter_limits(39, 0)[3] == 1
    assert R.filter_limits(15, 0)[3] == 1 and R.filter_limits(14, 0)[3] == 0
    assert R.filter_limits(20, 3) == (6, 46, 50, 1) and R.filter_limits(20, 5) == (4, 44, 48, 1) and R.filter_limits(1, 7) == (1, 3, 7, 0)


# ---- libwebp's planes ---------------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_committed():
    assert len(FIXTURES) >= 12 and all(os.path.getsize(p) < (1 << 20) for p in glob.glob(os.path.join(GOLDEN, "*")))


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_and_host_path_equal_libwebp(name, native):
    data, (Y, U, V) = fixture(name)
    frame = R.webp_payload(data)
    y, u, v, info = R.decode_planes(frame)
    assert (y == Y).all() and (u == U).all() and (v == V).all() and info["errors"] == 0
    want = ref("fixture:" + name, R.ivf([frame]))[0]
    assert api.webp_to_ivf(data)[32:] == R.ivf([frame])[32:]
    for chunk in (0, 1, 7):
        n, frames, st = native(R.ivf([frame]), chunk)
        assert n == 1 and frames[0] == want[0] and st["errors"] == 0, chunk
    n, frames, st = native([frame])
    assert n == 1 and frames[0] == want[0]
    # ... and cropped to libwebp's planes
    h, w = Y.shape
    dw, dh = frames[0][1], frames[0][2]
    f = np.frombuffer(frames[0][0], np.uint8)
    c = f[dw * dh:].reshape(dh // 2, dw)
    assert (f[:dw * dh].reshape(dh, dw)[:h, :w] == Y).all() and (c[:U.shape[0], 0:2 * U.shape[1]:2] == U).all() and (c[:V.shape[0], 1:2 * V.shape[1]:2] == V).all()


def test_fixtures_and_feature_cases_together_leave_no_hole():
    agg = {}

    def add(info):
        for k, v in info.items():
            if isinstance(v, set):
                agg.setdefault(k, set()).update(v)
            elif isinstance(v, int) and not isinstance(v, bool):
                agg[k] = agg.get(k, 0) + v
    for name in FIXTURES:
        add(R.decode_planes(R.webp_payload(fixture(name)[0]))[3])
    # what libwebp pins on its own (tests/golden/vp8/README.md)
    assert agg["ymodes"] == set(range(5)) and agg["uvmodes"] == set(range(4)) and agg["bmodes"] == set(range(10)) and agg["cats"] == set(range(1, 7))
    assert len(agg["segments"]) >= 2 and agg["skipped_mbs"] > 0 and agg["coded_mbs"] > 0 and agg["prob_updates"] > 0
    assert agg["filter_types"] == {0, 1} and max(agg["levels"]) > 0 and agg["mb_edge_mbs"] > 0 and agg["inner_edge_mbs"] > 0
    assert agg["partitions"] == {1, 2, 4, 8} and {0, 7} <= agg["sharpness"] and agg["seg_abs"] == {1} and agg["no_coeff_skip"] == {0, 1}
    # what only the scripted streams reach
    for name, data in _FEATURES.items():
        add(ref(name, data)[1])
    assert agg["seg_abs"] == {0, 1} and agg["sharpness"] == set(range(8)) and agg["versions"] == {0, 1, 2, 3} and agg["lf_delta"]
    assert agg["color_space"] == {0, 1} and agg["clamping"] == {0, 1} and (2, 1) in agg["scale"] and agg["refresh"] == {0, 1} and agg["hidden"] > 0 and agg["empty"] > 0
    assert any(max(q) == 15 for q in agg["q_deltas"]) and any(min(q) == -15 for q in agg["q_deltas"]) and {0, 63} <= agg["levels"]


# ---- scripted streams ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_SCRIPTED))
def test_host_path_equals_restatement_in_every_chunking(name, native):
    data = _SCRIPTED[name]
    want, info = ref(name, data)
    for chunk in (0, 1, 7):
        n, frames, st = native(data, chunk)
        assert n == len(want) and frames == want, chunk
        assert st["errors"] == info["errors"] and st["key_frames"] == info["key_frames"] and st["hidden"] == info["hidden"] and st["empty"] == info["empty"]
    n, frames, st = native(R.split_ivf(data))
    assert frames == want and st["errors"] == info["errors"]
    assert (info["errors"] > 0) == (name in _DAMAGED)


def test_bool_encoder_round_trip():
    import random
    rnd = random.Random(5)
    seq = [(rnd.randrange(1, 256), rnd.randrange(2)) for _i in range(5000)]
    e = S.BoolEncoder()
    for p, b in seq:
        e.write(p, b)
    d = R.BoolDecoder(e.finish())
    assert [d.read(p) for p, _b in seq] == [b for _p, b in seq] and d.past == 0


@pytest.mark.parametrize("name,data,msg", S.refused_cases(), ids=[c[0] for c in S.refused_cases()])
def test_refusals_with_their_text(name, data, msg, native):
    with pytest.raises(R.Refused, match=msg.replace("(", r"\(")):
        R.decode_stream(data, 0)
    n, _, _ = native(data)
    assert n == -1 and native.lib.v8c_error().decode() == msg
    with api.JmAmdDec(5, 1, options=dict(vp8=1, parse_only=1)) as d:
        with pytest.raises(RuntimeError):
            d.decode_stream(data, keep=False, chunks=[data])
        assert api.lib().jm_amddec_last_error(d.h).decode() == msg and d.stat("failed") == 1


# ---- through the library, parse only ----------------------------------------------------------------------------------------------------------
STATS = ("errors", "frames", "failed", "i_pictures", "out_width", "out_height", "coded_width", "coded_height", "job_digest", "job_bytes", "vp8_key_frames",
         "vp8_hidden_frames", "vp8_empty_frames", "vp8_partitions", "vp8_segments", "vp8_filter_type", "vp8_color_space", "vp8_scale", "vp8_bpred_mbs", "vp8_skipped_mbs")


def parse(data, chunks=None, **opt):
    with api.JmAmdDec(5, 1, options=dict(vp8=1, parse_only=1, sync=1, **opt)) as d:
        n = d.decode_stream(data, keep=False, chunks=chunks if chunks is not None else [data])
        st = {k: d.stat(k) for k in STATS}
        st["info"] = api.jm_nvdec_show_dec_info(d.h)
        st["size"] = api.jm_nvdec_stream_info(d.h)
        return n, st


def test_codec_5_needs_option_vp8_and_the_rest_stay_refused():
    with api.JmAmdDec(5, 1, options=dict(vp8=1, parse_only=1)):
        pass
    # without the option nothing changes for a caller: 5 is refused like 3, 6 and 7, and the text says how to get it
    for codec in (3, 5, 6, 7):
        with pytest.raises(RuntimeError, match=r"and 5 \(VP8\) for key frames with option vp8 1"):
            api.JmAmdDec(codec, 1, options=dict(parse_only=1))
    for codec in (3, 6, 7):
        with pytest.raises(RuntimeError):
            api.JmAmdDec(codec, 1, options=dict(vp8=1, parse_only=1))
    with pytest.raises(RuntimeError, match="option vp8 is only available for VP8"):
        api.JmAmdDec(0, 1, options=dict(vp8=1, parse_only=1))
    with pytest.raises(RuntimeError, match="deinterlace_temporal"):
        api.JmAmdDec(5, 1, options=dict(vp8=1, parse_only=1, deinterlace=2, deinterlace_temporal=1))
    h = api.jm_intel_dec_create_handle()                           # the push / pull facade does not get VP8
    assert api.jm_intel_dec_init(5, 1, h) == -1
    api.jm_intel_dec_deinit(h)


def test_parse_only_stats(native):
    data = _FEATURES["partitions_4"]
    n, st = parse(data)
    nat = native(data)[2]
    assert n == 1 == st["frames"] == st["vp8_key_frames"] == st["i_pictures"] and st["errors"] == 0 and st["failed"] == 0
    assert st["vp8_partitions"] == 4 and (st["out_width"], st["out_height"], st["coded_width"], st["coded_height"]) == (48, 144, 48, 144)
    assert (st["vp8_bpred_mbs"], st["vp8_skipped_mbs"]) == (nat["bpred_mbs"], nat["skipped_mbs"]) and "VP8" in str(st["info"])
    n, st = parse(_FEATURES["header_bits"])
    assert (st["vp8_color_space"], st["vp8_scale"]) == (3, 2 | 1 << 2)
    n, st = parse(_FEATURES["segments_absolute"])
    assert st["vp8_segments"] == len(ref("segments_absolute", _FEATURES["segments_absolute"])[1]["segments"]) >= 2
    n, st = parse(_FEATURES["simple_filter"])
    assert st["vp8_filter_type"] == 1
    n, st = parse(_FEATURES["hidden_frame"])
    assert n == 2 and (st["vp8_key_frames"], st["vp8_hidden_frames"]) == (3, 1)
    n, st = parse(_FEATURES["empty_ivf_frame"])
    assert n == 2 and st["vp8_empty_frames"] == 1 and st["errors"] == 0
    n, st = parse(S.sized_stream(53, 37, seed=2))
    assert (st["out_width"], st["out_height"], st["coded_width"], st["coded_height"]) == (54, 38, 64, 48)      # an odd size: the even size just above


def test_job_digest_is_invariant_under_chunking_and_input_form():
    data = S.sized_stream(48, 32, seed=5, frames=4)
    forms = (None, [data[i:i + 1] for i in range(len(data))], [data[i:i + 7] for i in range(0, len(data), 7)], R.split_ivf(data))
    digests = {parse(data, chunks, job_digest=1)[1]["job_digest"] for chunks in forms}
    assert len(digests) == 1
    assert parse(S.sized_stream(48, 32, seed=6, frames=4), job_digest=1)[1]["job_digest"] not in digests


def test_job_list_is_sparse():
    """a record of 32 bytes per macroblock and 4 bytes per non-zero level: far from 800 bytes per macroblock even at a high density"""
    data = S.sized_stream(80, 272, seed=9)
    n, st = parse(data)
    assert st["job_bytes"] < 85 * 200


def test_size_change_and_damage_through_the_library():
    n, st = parse(S.size_change())
    assert n == 4 and st["errors"] == 0 and (st["out_width"], st["out_height"]) == (34, 18)
    for name, data in _DAMAGED.items():
        n, st = parse(data)
        assert n == 1 and st["errors"] > 0 and st["failed"] == 0, name
    cut = S.sized_stream(48, 32, seed=3, frames=2)
    n, st = parse(cut[:-40])                                       # the stream ends inside the second IVF frame: decoded as far as it goes
    assert n == 2 and st["errors"] > 0 and st["failed"] == 0


def test_feed_annexb_is_refused_for_vp8():
    data = S.sized_stream(16, 16)
    with api.JmAmdDec(5, 1, options=dict(vp8=1, parse_only=1)) as d:
        assert api.lib().jm_amddec_feed_annexb(data, len(data), 1, None, 0, d.h) == -1
        assert "feed_annexb" in api.lib().jm_amddec_last_error(d.h).decode() and d.stat("failed") == 0


def test_webp_to_ivf_helper():
    data, _ = fixture(FIXTURES[0])
    ivf = api.webp_to_ivf(data)
    assert ivf[:4] == b"DKIF" and R.split_ivf(ivf) == [R.webp_payload(data)]
    with pytest.raises(ValueError):
        api.webp_to_ivf(b"RIFF\x04\x00\x00\x00WEBP")
    with pytest.raises(ValueError):
        api.webp_to_ivf(b"not a webp file")


# ---- the sanitizer programs ---------------------------------------------------------------------------------------------------------------------
def _make(target, out):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), target, f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


def _clean(r):
    assert r.returncode == 0, r.stdout[-4000:]
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]


def test_vp8_asan_builds_and_runs_clean(tmp_path):
    """tools/vp8_asan.cpp: a stand-alone host program (its own main) under AddressSanitizer / UBSan: the kernels' lane routines over exact-size surfaces,
    on valid and on damaged job lists, at the sizes of the GPU tests"""
    out = tmp_path / "out"
    _make("vp8_asan", out)
    r = subprocess.run([str(out / "vp8_asan"), "1", "6"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    _clean(r)
    assert "ok: 6 trials, 36 pictures" in r.stdout


def test_fuzz_vp8_builds_and_runs_clean(tmp_path):
    """tools/fuzz_vp8.cpp: the host path on mutated fixtures and scripted streams under AddressSanitizer / UBSan, a bounded count"""
    out = tmp_path / "out"
    _make("fuzz_vp8_asan", out)
    streams = [R.ivf([R.webp_payload(fixture(FIXTURES[0])[0]), R.webp_payload(fixture(FIXTURES[-1])[0])]), _FEATURES["partitions_8"] , _FEATURES["segments_delta"]]
    for i, data in enumerate(streams):
        path = tmp_path / ("a%d.ivf" % i)
        path.write_bytes(data)
        r = subprocess.run([str(out / "fuzz_vp8_asan"), str(path), str(i + 1), "120"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        _clean(r)
        assert "ok: 120 trials" in r.stdout
