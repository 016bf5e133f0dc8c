"""MJPEG (codec_type 2) without a GPU.

The pin: tests/golden/jpeg/ holds pictures Pillow (libjpeg) encoded and Pillow's own decode of them; the restatement tests/jpeg_ref.py must agree with
that decode within +-1 (JPEG leaves the IDCT open: as exact as two decoders get).  The product's host path -- splitter, marker parser, Huffman decode
and the reconstruction of jpeg_recon.h, whose routines k_jpeg_recon runs -- is built with g++ (tests/native/jpeg_check.cpp) and must equal the
restatement bit for bit, on the fixtures and on seeded streams of the test encoder.  Then parse-only handles: counts, sizes, chunking, refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpeg_ref
from jmcodec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODABLE = ["g_8x8", "c420_16x16", "c420_53x37", "c420_72x40_rst3", "c422_48x32", "c444_40x24", "c444_53x37", "c420_64x48_opt", "c420_32x32_q1", "g_37x21"]


def fixture(name):
    return open(os.path.join(jpeg_ref.GOLDEN_JPEG, name + ".jpg"), "rb").read()


def pin_conditions(frame, dh, planes):
    """The two conditions of the pin; planes = Pillow's [Y] or [Y, Cb, Cr]."""
    h, w = planes[0].shape
    d = np.abs(frame[:h, :w].astype(int) - planes[0].astype(int))
    assert d.max() <= 1, int(d.max())
    assert (d != 0).mean() <= 0.05, float((d != 0).mean())
    if len(planes) == 3:
        hh, ww = h // 2, w // 2
        for c in (0, 1):
            p = planes[1 + c].astype(int)
            box = (p[0:2 * hh:2, 0:2 * ww:2] + p[0:2 * hh:2, 1:2 * ww:2] + p[1:2 * hh:2, 0:2 * ww:2] + p[1:2 * hh:2, 1:2 * ww:2] + 2) >> 2
            assert np.abs(frame[dh:dh + hh, c:2 * ww:2].astype(int) - box).max() <= 1


# ---- the pin -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DECODABLE)
def test_restatement_agrees_with_pillow_within_one(name):
    planes = [np.load(os.path.join(jpeg_ref.GOLDEN_JPEG, f"{name}.y.npy"))]
    if name.startswith("c444"):
        planes += [np.load(os.path.join(jpeg_ref.GOLDEN_JPEG, f"{name}.{c}.npy")) for c in ("cb", "cr")]
    f, dw, dh, _ = jpeg_ref.RefDecoder().decode_picture(fixture(name))
    pin_conditions(f, dh, planes)


def test_restatement_agrees_with_a_live_pillow_encode():
    PIL = pytest.importorskip("PIL")
    import io
    from PIL import Image
    rng = np.random.default_rng(7)
    for w, h, sub, q in ((45, 29, 2, 55), (40, 24, 0, 85), (64, 32, 1, 35)):
        a = np.clip(128 + 60 * np.sin(np.arange(w)[None, :, None] / 6.0 + np.arange(h)[:, None, None] / 9.0) + rng.normal(0, 15, (h, w, 3)), 0, 255)
        buf = io.BytesIO()
        Image.fromarray(a.astype(np.uint8), "YCbCr").save(buf, "JPEG", quality=q, subsampling=sub)
        im = Image.open(io.BytesIO(buf.getvalue()))
        im.draft("YCbCr", im.size)
        p = np.asarray(im)
        f, dw, dh, _ = jpeg_ref.RefDecoder().decode_picture(buf.getvalue())
        pin_conditions(f, dh, [p[:, :, 0]] + ([p[:, :, 1], p[:, :, 2]] if sub == 0 else []))
    assert PIL


# ---- the product's host path, bit for bit ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libjpeg_check.so")
    csrc = os.path.join(ROOT, "jmcodec_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "jpeg_check.cpp"), os.path.join(csrc, "jpeg_syntax.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("jpeg_syntax.h", "jpeg_recon.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so] + srcs)
    l = C.CDLL(so)
    l.jc_decode.restype = C.c_long
    l.jc_decode.argtypes = [C.c_char_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    l.jc_error.restype = C.c_char_p
    l.jc_std_table.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def decode(data, chunk=0):
        out_buf, dims, err = C.create_string_buffer(1 << 22), (C.c_int * 128)(), C.c_int()
        n = l.jc_decode(data, len(data), chunk, out_buf, len(out_buf), dims, 64, C.byref(err))
        frames, o = [], 0
        for i in range(max(n, 0)):
            w, h = dims[2 * i], dims[2 * i + 1]
            frames.append((out_buf.raw[o:o + w * h * 3 // 2], w, h))
            o += w * h * 3 // 2
        return n, frames, err.value
    decode.lib = l
    return decode


@pytest.mark.parametrize("name", DECODABLE)
def test_host_path_equals_restatement_on_fixtures(native, name):
    data = fixture(name)
    n, frames, errors = native(data)
    assert (n, errors) == (1, 0)
    assert frames == jpeg_ref.decode_stream(data, 0)


def _special_streams():
    """Hand-made corners, each a (name, stream)."""
    rng = np.random.default_rng(0x4A50)
    q = [[int(v) for v in rng.integers(1, 40, 64)], [int(v) for v in rng.integers(1, 90, 64)]]
    qmax = [[255] * 64, [255] * 64]
    out = []
    lv = jpeg_ref.random_levels(rng, 0x22, 32, 16, density=0.0)
    lv[0][0, 0, 40] = 5
    lv[0][0, 1, 63] = -3                                           # ZRL runs: 39 and 62 zeros in front of one level
    lv[0][1, 2, 1:] = rng.integers(1, 9, 63)                       # 63 AC coefficients: no EOB
    out.append(("zrl_and_no_eob", jpeg_ref.encode(lv, q, 0x22, 32, 16)))
    lv = jpeg_ref.random_levels(rng, 0x11, 16, 8, density=0.0, dc_amp=0)
    lv[0][0, 0, 0], lv[0][0, 1, 0] = 1023, -1024                   # DC differences of category 10, then 11 (-2047)
    lv[0][0, 0, 9], lv[1][0, 0, 3] = 1023, -1000                   # AC category 10
    out.append(("dc_cat11_ac_cat10", jpeg_ref.encode(lv, q, 0x11, 16, 8)))
    lv = jpeg_ref.random_levels(rng, 0x21, 32, 8, density=0.5, amp=1023, dc_amp=1023)      # x 255: both clips saturate
    out.append(("saturating", jpeg_ref.encode(lv, qmax, 0x21, 32, 8)))
    lv = jpeg_ref.random_levels(rng, 0x10, 24, 24, density=0.0, dc_amp=0)
    lv[0][:, :, 1] = 255                                           # long runs of 1 bits: stuffed FF bytes
    lv[0][:, :, 2] = -256
    s = jpeg_ref.encode(lv, q, 0x10, 24, 24)
    assert b"\xff\x00" in s
    out.append(("stuffed_ff", s))
    lv = jpeg_ref.random_levels(rng, 0x22, 48, 32, density=0.3)
    out.append(("fill_before_rst_any_index", jpeg_ref.encode(lv, q, 0x22, 48, 32, dri=2, fill_before_rst=3, rst_offset=5)))
    out.append(("two_tables_in_one_dqt", jpeg_ref.encode(lv, q, 0x22, 48, 32, one_dqt=True, sof=0xC1)))
    q2 = [[int(v) for v in rng.integers(1, 20, 64)], q[1]]
    out.append(("table_redefined_between_pictures", jpeg_ref.encode(lv, q, 0x22, 48, 32) + jpeg_ref.encode(lv, q2, 0x22, 48, 32, dht=False)
                + jpeg_ref.encode(lv, q2, 0x22, 48, 32, tables=False)))
    thumb = b"Exif\x00\x00" + b"\xff\xd8\xff\xdb\x00\x03\x00\xff\xda\x00\x02junk\xff\xd9"
    out.append(("app1_with_embedded_soi_eoi", jpeg_ref.encode(lv, q, 0x22, 48, 32, app=[(0xE1, thumb)]) + jpeg_ref.encode(lv, q, 0x22, 48, 32)))
    out.append(("missing_dht", jpeg_ref.encode(lv, q, 0x22, 48, 32, dht=False) + jpeg_ref.encode(lv[:1], q, 0x10, 48, 32, dht=False)))
    out.append(("adobe_transform_1", jpeg_ref.encode(lv, q, 0x22, 48, 32, app=[(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01")])))
    return out


SPECIAL = _special_streams()


@pytest.mark.parametrize("name,data", SPECIAL, ids=[n for n, _ in SPECIAL])
def test_host_path_equals_restatement_on_corner_streams(native, name, data):
    want = jpeg_ref.decode_stream(data, 0)
    assert want
    for chunk in (0, 1, 13):
        n, frames, errors = native(data, chunk)
        assert errors == 0 and n == len(want), (name, chunk, n, native.lib.jc_error())
        assert frames == want, (name, chunk)


def test_host_path_equals_restatement_on_seeded_streams(native):
    """About 200 seeded streams: every sampling, odd sizes, restart intervals, missing DHT, random tables."""
    rng = np.random.default_rng(0x4A504701)
    for i in range(200):
        samp = (0x22, 0x21, 0x11, 0x10)[i % 4]
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 50))
        lv = jpeg_ref.random_levels(rng, samp, w, h, density=float(rng.choice([0.05, 0.3, 0.9])), amp=int(rng.choice([3, 60, 1023])), dc_amp=int(rng.choice([50, 1023])))
        q = [[int(v) for v in rng.integers(1, int(rng.choice([4, 64, 256])), 64)] for _ in range(2)]
        data = jpeg_ref.encode(lv, q, samp, w, h, dri=int(rng.choice([0, 0, 1, 3, 10])), dht=bool(i % 5), fill_before_rst=int(rng.integers(0, 3)),
                               rst_offset=int(rng.integers(0, 8)), sof=0xC1 if i % 7 == 0 else 0xC0)
        n, frames, errors = native(data, int(rng.choice([0, 1, 5, 64])))
        assert (n, errors) == (1, 0), (i, native.lib.jc_error())
        assert frames == jpeg_ref.decode_stream(data, 0), f"seeded stream {i}: sampling {samp:#x} {w}x{h}"


# ---- analytic cases: levels in, closed form out ------------------------------------------------------------------------------------------
def _analytic(native, lv, q, samp, w, h):
    data = jpeg_ref.encode(lv, q, samp, w, h)
    n, frames, errors = native(data)
    assert (n, errors) == (1, 0)
    dw, dh = (w + 1) & ~1, (h + 1) & ~1
    return np.frombuffer(frames[0][0], np.uint8).reshape(dh * 3 // 2, dw), dh


def test_all_zero_levels_give_128(native):
    for samp in (0x22, 0x21, 0x11, 0x10):
        ncomp = 1 if samp == 0x10 else 3
        chroma = [] if ncomp == 1 else [(4 // (samp & 15), 4 // (samp >> 4), 64)] * 2
        lv = [np.zeros(s, np.int64) for s in [(4, 4, 64)] + chroma]
        f, _ = _analytic(native, lv, [[16] * 64] * 2, samp, 32, 32)
        assert (f == 128).all()


def test_dc_only_block_is_flat_by_the_two_expressions(native):
    for level, qv in ((1, 1), (3, 16), (-7, 33), (100, 255), (-1024, 255), (1023, 255), (5, 7)):
        F = max(-32768, min(32767, level * qv))
        g = max(-65536, min(65535, (2896 * F + 256) >> 9))
        want = max(0, min(255, ((2896 * g + 65536) >> 17) + 128))
        lv = [np.zeros((1, 1, 64), np.int64)]
        lv[0][0, 0, 0] = level
        f, dh = _analytic(native, lv, [[qv] * 64] * 2, 0x10, 8, 8)
        assert (f[:dh] == want).all(), (level, qv, want)
        assert (f[dh:] == 128).all()                               # grey: chroma 128


def test_chroma_rules_on_hand_made_blocks(native):
    """Chroma planes with a vertical and a horizontal AC term: the decoded plane comes from the IDCT restatement, the surface's chroma from the rule."""
    q = [[8] * 64] * 2
    for samp in (0x22, 0x21, 0x11):
        hs, vs = samp >> 4, samp & 15
        lv = [np.zeros((vs, hs, 64), np.int64), np.zeros((1, 1, 64), np.int64), np.zeros((1, 1, 64), np.int64)]
        lv[1][0, 0, [0, 1, 8]] = (10, 30, -25)
        lv[2][0, 0, [0, 8, 9]] = (-12, 40, 17)
        w, h = 8 * hs, 8 * vs
        f, dh = _analytic(native, lv, q, samp, w, h)
        for c in (0, 1):
            plane = jpeg_ref.idct_plane(lv[1 + c], np.full(64, 8, np.int64)).astype(int)
            if samp == 0x22:
                want = plane
            elif samp == 0x21:
                want = np.array([[(plane[2 * y][x] + plane[2 * y + 1][x] + 1) >> 1 for x in range(8)] for y in range(4)])
            else:
                want = np.array([[(plane[2 * y][2 * x] + plane[2 * y][2 * x + 1] + plane[2 * y + 1][2 * x] + plane[2 * y + 1][2 * x + 1] + 2) >> 2
                                  for x in range(4)] for y in range(4)])
            assert np.array_equal(f[dh:, c::2], want), (hex(samp), c)


def test_idct_table_is_the_rounded_cosine_table(native):
    native.lib.jc_idct_m.argtypes = [C.c_int, C.c_int]
    assert [[native.lib.jc_idct_m(k, n) for n in range(8)] for k in range(8)] == jpeg_ref.M.tolist()
    assert int(np.abs(jpeg_ref.M).sum(axis=0).max()) <= 21641


# ---- table provenance ----------------------------------------------------------------------------------------------------------------
def test_annex_k_tables_equal_libjpegs_dht(native):
    d = jpeg_ref.RefDecoder()
    d.headers(fixture("c420_16x16"))                               # not optimised: libjpeg wrote its default tables
    for cls in (0, 1):
        for tid in (0, 1):
            bits, vals = (C.c_ubyte * 16)(), (C.c_ubyte * 256)()
            n = native.lib.jc_std_table(cls, tid, bits, vals)
            assert list(bits) == d.huff[(cls, tid)].bits and list(vals[:n]) == d.huff[(cls, tid)].vals, (cls, tid)


# ---- parse-only handles ----------------------------------------------------------------------------------------------------------------
def _handle(data, chunks=None, fmt=1):
    with api.JmAmdDec(2, fmt, options={"parse_only": 1}) as d:
        frames = d.decode_stream(data, chunks=chunks if chunks is not None else [data])
        return dict(n=len(frames), sizes=[len(f) for f in frames], errors=d.stat("errors"), info=api.jm_nvdec_stream_info(d.h),
                    sampling=d.stat("jpeg_sampling"), pictures=d.stat("jpeg_pictures"), ri=d.stat("jpeg_restart_intervals"),
                    text=api.jm_nvdec_show_dec_info(d.h))


def test_frame_counts_stream_info_and_sampling():
    for name, samp, (dw, dh) in (("c420_53x37", 0x22, (54, 38)), ("c422_48x32", 0x21, (48, 32)), ("c444_53x37", 0x11, (54, 38)), ("g_37x21", 0x10, (38, 22))):
        r = _handle(fixture(name) * 3)
        assert (r["n"], r["errors"], r["pictures"]) == (3, 0, 3)
        assert r["info"] == (dw, dh) and r["sizes"] == [dw * dh * 3 // 2] * 3          # even-rounded sizes
        assert r["sampling"] == samp
        assert "MJPEG" in r["text"]
    assert _handle(fixture("c420_72x40_rst3") * 2)["ri"] == 2


def test_chunking_invariance():
    data = b"\x00\x00\x01" + b"".join(fixture(n) for n in ("c420_72x40_rst3", "c420_72x40_rst3", "c444_53x37", "g_37x21", "c422_48x32"))
    whole = _handle(data)
    assert whole["n"] == 5 and whole["errors"] == 0
    for chunks in (api.split_nalus(data), [data[i:i + 1] for i in range(len(data))], api.split_jpegs(data)):
        assert b"".join(chunks) == data
        r = _handle(data, chunks)
        assert (r["n"], r["sizes"], r["errors"]) == (5, whole["sizes"], 0)
    assert len(api.split_jpegs(data)) == 5


def test_size_change_mid_stream():
    r = _handle(fixture("c420_16x16") * 2 + fixture("c420_53x37") * 2 + fixture("c444_53x37"))
    assert r["n"] == 5 and r["errors"] == 0
    assert r["sizes"] == [384, 384, 54 * 38 * 3 // 2, 54 * 38 * 3 // 2, 54 * 38 * 3 // 2] and r["sampling"] == 0x11


def _patched(data, marker, at, value):
    """The picture with byte `at` of the payload of its first `marker` segment replaced."""
    i = data.index(bytes([0xFF, marker]))
    b = bytearray(data)
    b[i + 4 + at] = value
    return bytes(b)


def _refusals():
    rng = np.random.default_rng(3)
    q = [[16] * 64] * 2
    lv = jpeg_ref.random_levels(rng, 0x22, 16, 16)
    base = jpeg_ref.encode(lv, q, 0x22, 16, 16)
    sof = base.index(b"\xff\xc0")
    return {
        "progressive": (fixture("prog_32x32"), "progressive"),
        "cmyk": (fixture("cmyk_16x16"), "four components"),
        "arithmetic": (base[:sof] + b"\xff\xc9" + base[sof + 2:], "arithmetic"),
        "lossless": (base[:sof] + b"\xff\xc3" + base[sof + 2:], "lossless"),
        "twelve_bit": (_patched(base, 0xC0, 0, 12), "12-bit"),
        "two_components": (_patched(base, 0xC0, 5, 2), "component count"),
        "sampling_411": (_patched(base, 0xC0, 7, 0x41), "sampling factors"),
        "sampling_440": (_patched(base, 0xC0, 7, 0x12), "sampling factors"),
        "several_scans": (_patched(base, 0xDA, 0, 1), "several scans"),
        "spectral_selection": (_patched(base, 0xDA, 8, 5), "spectral selection"),
        "pq_1": (_patched(base, 0xDB, 0, 0x10), "Pq = 1"),
        "dnl": (base[:sof] + b"\xff\xdc\x00\x04\x00\x10" + base[sof:], "DNL"),
        "adobe_rgb": (jpeg_ref.encode(lv, q, 0x22, 16, 16, app=[(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00")]), "Adobe"),
        "too_large": (_patched(base, 0xC0, 3, 0x30), "8192"),
    }


REFUSALS = _refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refused_features_fail_the_handle_with_a_reason(name):
    data, word = REFUSALS[name]
    with api.JmAmdDec(2, 1, options={"parse_only": 1}) as d:
        with pytest.raises(RuntimeError) as e:
            d.decode_stream(data, chunks=[data])
        assert word in str(e.value) and "not supported" in str(e.value), str(e.value)
        assert word in api.lib().jm_amddec_last_error(d.h).decode()


def test_push_pull_facade_still_refuses_2():
    h = api.jm_intel_dec_create_handle()
    try:
        assert api.jm_intel_dec_init(2, 1, h) != 0
    finally:
        api.jm_intel_dec_deinit(h)


def test_truncated_streams_finish_with_errors():
    data = fixture("c420_72x40_rst3") * 3
    one = len(data) // 3
    for cut in (one * 2 + 20, one * 2 + one // 2, len(data) - 2, one * 2 + 700):
        r = _handle(data[:cut])
        assert r["errors"] > 0 and r["n"] in (2, 3), (cut, r)
    # a missing restart marker: the picture in the middle is damaged, handed out all the same, and the one behind it is whole
    pics = jpeg_ref.split_pictures(data)
    rst = pics[0].index(b"\xff\xd1")
    broken = pics[0][:rst] + pics[0][rst + 2:]
    r = _handle(pics[0] + broken + pics[0])
    assert r["n"] == 3 and r["errors"] > 0


# ---- the sanitizer harness -----------------------------------------------------------------------------------------------------------
def test_fuzz_jpeg_builds_and_runs_clean(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "fuzz_jpeg", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    path = tmp_path / "a.mjpeg"
    path.write_bytes(b"".join(fixture(n) for n in ("c420_72x40_rst3", "c444_53x37", "g_37x21", "c422_48x32")))
    r = subprocess.run([str(out / "fuzz_jpeg"), str(path), "1", "400"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ok: 400 trials" in r.stdout
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
