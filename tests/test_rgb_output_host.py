"""RGB output, host side (no GPU): the colour coefficients against an exact rational computation, a numpy restatement of the conversion C
(INTEGRATION.md "RGB output") and its closed forms, the colour description of both parsers, and the RGB spec of parse-only handles.  The
restatement here is what the GPU tests (test_rgb_output_gpu.py) compare the device output with."""
from fractions import Fraction

import numpy as np
import pytest

from jmcodec_amd import api
from tools import streams
from test_scaled_output_host import scale_frame, split_frame

MATRICES = (1, 4, 5, 6, 7, 9)
KRKB = {1: ("0.2126", "0.0722"), 4: ("0.30", "0.11"), 5: ("0.299", "0.114"), 6: ("0.299", "0.114"), 7: ("0.212", "0.087"), 9: ("0.2627", "0.0593")}


# ---- C restated ----------------------------------------------------------------------------------------------------------------
def coefs_ref(matrix, full):
    """cy, crv, cgu, cgv, cbu: exact rationals from the decimal Kr, Kb, rounded half away from zero (all positive)."""
    kr, kb = (Fraction(s) for s in KRKB[matrix])
    kg = 1 - kr - kb
    sy, sc = (Fraction(1), Fraction(1)) if full else (Fraction(255, 219), Fraction(255, 224))
    rnd = lambda x: int(x * 16384 + Fraction(1, 2))
    return (rnd(sy), rnd(sc * 2 * (1 - kr)), rnd(sc * 2 * kb * (1 - kb) / kg), rnd(sc * 2 * kr * (1 - kr) / kg), rnd(sc * 2 * (1 - kb)))


def rgb_accumulators(Y, U, V, matrix, full):
    """(aR, aG, aB) int64 arrays of C for a 4:2:0 frame G (Y h x w, U / V h/2 x w/2): nearest chroma."""
    cy, crv, cgu, cgv, cbu = coefs_ref(matrix, full)
    yo = 0 if full else 16
    Y = Y.astype(np.int64)
    d = U.astype(np.int64).repeat(2, 0).repeat(2, 1) - 128
    e = V.astype(np.int64).repeat(2, 0).repeat(2, 1) - 128
    yv = cy * (Y - yo)
    return yv + crv * e, yv - cgu * d - cgv * e, yv + cbu * d


def f32_to_bf16_bits(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def convert(Y, U, V, dtype, planar, bgr, matrix, full, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """C of a frame G as the bytes the library hands out.  dtype 0 u8, 1 f32, 2 f16, 3 bf16."""
    aR, aG, aB = rgb_accumulators(Y, U, V, matrix, full)
    chans = [aB, aG, aR] if bgr else [aR, aG, aB]
    out = []
    for c, a in enumerate(chans):
        if dtype == 0:
            out.append(np.clip((a + 8192) >> 14, 0, 255).astype(np.uint8))
            continue
        v = np.clip(a, 0, 255 * 16384).astype(np.float32)
        k = np.float32(scale[c]) * np.float32(2.0 ** -14)
        f = ((v * k).astype(np.float32) + np.float32(bias[c])).astype(np.float32)     # two float32 roundings, no FMA
        out.append(f if dtype == 1 else f.astype(np.float16) if dtype == 2 else f32_to_bf16_bits(f))
    return np.stack(out, 0 if planar else 2).tobytes()


def rgb_frame(F, W, H, fmt, crop, target, spec, matrix, full):
    """C(R_G(F)) for a tight frame F (NV12 fmt 0 / I420 fmt 1) of W x H, the geometry crop / target and an RgbSpec."""
    G = scale_frame(F, W, H, fmt, crop, target)
    Y, U, V = split_frame(G, target[0], target[1], fmt)
    return convert(Y, U, V, spec.dtype, spec.planar, spec.bgr, matrix, full, tuple(spec.scale), tuple(spec.bias))


# ---- coefficients ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("full", [0, 1])
def test_color_coefs_equal_the_exact_computation(matrix, full):
    assert api.color_coefs(matrix, full) == coefs_ref(matrix, full)


def test_color_coefs_refuse_unsupported_matrices():
    for m in (0, 2, 3, 8, 10, 11, 14, 255, -1):
        assert api.color_coefs(m, 0) is None and api.color_coefs(m, 1) is None
    assert api.color_coefs(1, 0)[0] == 19077 and api.color_coefs(1, 1)[0] == 16384      # 255 / 219 and 1 in 14 bits


# ---- closed forms of C -----------------------------------------------------------------------------------------------------------
def test_limited_range_black_and_white():
    for m in MATRICES:
        for y, want in ((16, 0), (235, 255)):
            Y = np.full((2, 2), y, np.uint8)
            N = np.full((1, 1), 128, np.uint8)
            out = np.frombuffer(convert(Y, N, N, 0, 1, 0, m, False), np.uint8)
            assert (out == want).all(), (m, y)
            f = np.frombuffer(convert(Y, N, N, 1, 1, 0, m, False), np.float32)
            assert np.allclose(f, want, atol=0.02), (m, y)


def test_greys_stay_grey_under_every_matrix():
    Y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    N = np.full((8, 8), 128, np.uint8)
    for m in MATRICES:
        for full in (False, True):
            for dtype in (0, 1, 2, 3):
                out = np.frombuffer(convert(Y, N, N, dtype, 1, 0, m, full), {0: np.uint8, 1: np.float32, 2: np.float16, 3: np.uint16}[dtype])
                r, g, b = out.reshape(3, -1)
                assert np.array_equal(r, g) and np.array_equal(g, b), (m, full, dtype)


def test_full_range_luma_passes_through():
    Y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    N = np.full((8, 8), 128, np.uint8)
    out = np.frombuffer(convert(Y, N, N, 0, 1, 0, 1, True), np.uint8).reshape(3, 16, 16)
    assert np.array_equal(out[0], Y) and np.array_equal(out[2], Y)


def test_f32_keeps_what_u8_rounds_away():
    rng = np.random.default_rng(7)
    Y = rng.integers(0, 256, (6, 8), dtype=np.uint8)
    U = rng.integers(0, 256, (3, 4), dtype=np.uint8)
    V = rng.integers(0, 256, (3, 4), dtype=np.uint8)
    u8 = np.frombuffer(convert(Y, U, V, 0, 0, 0, 1, False), np.uint8).astype(np.float64)
    f = np.frombuffer(convert(Y, U, V, 1, 0, 0, 1, False), np.float32).astype(np.float64)
    assert np.all(np.abs(np.clip(f, 0, 255) - u8) <= 0.5 + 1e-6) and not np.array_equal(f, np.round(f))


def test_layouts_and_order():
    rng = np.random.default_rng(8)
    Y = rng.integers(0, 256, (4, 6), dtype=np.uint8)
    U = rng.integers(0, 256, (2, 3), dtype=np.uint8)
    V = rng.integers(0, 256, (2, 3), dtype=np.uint8)
    chw = np.frombuffer(convert(Y, U, V, 0, 1, 0, 6, False), np.uint8).reshape(3, 4, 6)
    hwc = np.frombuffer(convert(Y, U, V, 0, 0, 0, 6, False), np.uint8).reshape(4, 6, 3)
    bgr = np.frombuffer(convert(Y, U, V, 0, 1, 1, 6, False), np.uint8).reshape(3, 4, 6)
    assert np.array_equal(chw.transpose(1, 2, 0), hwc) and np.array_equal(bgr, chw[::-1])
    assert np.array_equal(api.rgb_array(hwc.tobytes(), 6, 4, api.rgb_spec("u8", planar=False)), hwc)


def test_imagenet_spec_and_bf16_helper():
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    s = api.rgb_spec("f16", mean=mean, std=std)
    for c in range(3):
        assert abs(s.scale[c] - 1 / (255 * std[c])) < 1e-9 and abs(s.bias[c] + mean[c] / std[c]) < 1e-6
    x = np.array([1.0, -2.5, 0.15625, 255.0], np.float32)
    assert np.array_equal(api.bf16_to_f32(f32_to_bf16_bits(x)), x)
    assert f32_to_bf16_bits(np.float32(1.0 + 2 ** -8)) == 0x3F80               # a tie rounds to even
    assert f32_to_bf16_bits(np.float32(1.0 + 3 * 2 ** -8)) == 0x3F82


# ---- the colour description (VUI) of both parsers --------------------------------------------------------------------------------
def _parse(data, codec=0, rgb=None, **opts):
    o = {"parse_only": 1}
    o.update(opts)
    with api.JmAmdDec(codec, 1, options=o, rgb=rgb) as d:
        frames = d.decode_stream(data)
        keys = ("vui_matrix", "vui_primaries", "vui_transfer", "vui_full_range", "color_matrix", "color_range", "out_frame_bytes", "rgb_frames",
                "fps_num", "fps_den")
        return [len(f) for f in frames], {k: d.stat(k) for k in keys}, api.jm_nvdec_show_dec_info(d.h)


def _h264(w=64, h=48, **kw):
    return streams.generate(width=w, height=h, frames=2, gop=2, mode=1, seed=0xC010, **kw)


def _hevc(w=64, h=48, **kw):
    return streams.generate_hevc(width=w, height=h, frames=2, ctb_log2=5, mode=1, seed=0xC011, **kw)


GEN = {0: _h264, 1: _hevc}


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("matrix", MATRICES)
def test_vui_matrix_and_range(codec, matrix):
    for full in (0, 1):
        _, st, _ = _parse(GEN[codec](vui_matrix=matrix, vui_primaries=1, vui_transfer=1, vui_full_range=full), codec)
        assert (st["vui_matrix"], st["vui_primaries"], st["vui_transfer"], st["vui_full_range"]) == (matrix, 1, 1, full)
        assert (st["color_matrix"], st["color_range"]) == (matrix, 2 if full else 1)


@pytest.mark.parametrize("codec", [0, 1])
def test_unspecified_and_unsupported_matrices_follow_the_height(codec):
    for m in (2, 8, 10):
        _, st, _ = _parse(GEN[codec](1280, 720, vui_matrix=m, vui_primaries=2, vui_transfer=2), codec)
        assert (st["vui_matrix"], st["color_matrix"], st["color_range"]) == (m, 1, 1)
        _, st, _ = _parse(GEN[codec](640, 480, vui_matrix=m, vui_primaries=2, vui_transfer=2), codec)
        assert (st["vui_matrix"], st["color_matrix"]) == (m, 6)
    _, st, _ = _parse(GEN[codec](640, 480, vui_primaries=1), codec)          # matrix 0 (GBR): not supported either
    assert (st["vui_matrix"], st["color_matrix"]) == (0, 6)


@pytest.mark.parametrize("codec", [0, 1])
def test_no_vui(codec):
    _, st, _ = _parse(GEN[codec](), codec)
    assert (st["vui_matrix"], st["vui_primaries"], st["vui_transfer"], st["vui_full_range"]) == (-1, -1, -1, -1)
    assert (st["color_matrix"], st["color_range"]) == (6, 1)
    _, st, _ = _parse(GEN[codec](vui_full_range=1), codec)                   # video_signal_type without a colour description
    assert (st["vui_matrix"], st["vui_full_range"], st["color_matrix"], st["color_range"]) == (-1, 1, 6, 2)


@pytest.mark.parametrize("codec", [0, 1])
def test_vui_with_timing_and_colour(codec):
    _, st, _ = _parse(GEN[codec](vui_fps=25, vui_matrix=9, vui_primaries=9, vui_transfer=14), codec)
    assert (st["vui_matrix"], st["vui_primaries"], st["vui_transfer"], st["vui_full_range"]) == (9, 9, 14, 0)
    assert st["fps_den"] > 0 and st["fps_num"] / st["fps_den"] == 25


def test_spec_forces_matrix_and_range():
    _, st, _ = _parse(_h264(vui_matrix=1, vui_primaries=1, vui_transfer=1), rgb=dict(dtype="u8", matrix=9, range=2))
    assert (st["vui_matrix"], st["color_matrix"], st["color_range"]) == (1, 9, 2)


def test_truncated_hevc_vui_leaves_the_colour_unknown():
    nals = api.split_nalus(_hevc(vui_fps=30, vui_matrix=1, vui_primaries=1, vui_transfer=1))
    sps = [i for i, n in enumerate(nals) if ((n[n.index(b"\x00\x01") + 2] >> 1) & 63) == 33][0]
    nals[sps] = nals[sps][:-6]                              # the SPS ends inside the VUI timing information: valid, its VUI unknown
    lens, st, _ = _parse(b"".join(nals), 1)
    assert len(lens) == 2
    assert (st["vui_matrix"], st["vui_full_range"], st["fps_num"]) == (-1, -1, 0)
    assert st["color_matrix"] == 6


def test_colour_parameters_at_zero_change_no_stream():
    zero = dict(vui_matrix=0, vui_primaries=0, vui_transfer=0, vui_full_range=0)
    for kw in (dict(), dict(vui_fps=30), dict(cabac=1, bframes=2, poc_type=0)):
        a = streams.generate(width=64, height=48, frames=3, gop=3, mode=1, seed=5, **kw)
        assert a == streams.generate(width=64, height=48, frames=3, gop=3, mode=1, seed=5, **zero, **kw)
    for kw in (dict(), dict(vui_fps=30)):
        a = streams.generate_hevc(width=64, height=48, frames=2, seed=5, **kw)
        assert a == streams.generate_hevc(width=64, height=48, frames=2, seed=5, **zero, **kw)


# ---- the spec ---------------------------------------------------------------------------------------------------------------------
def test_set_rgb_validation():
    L = api.lib()
    h = api.jm_nvdec_create_handle()
    try:
        assert api.set_rgb(h, "f16") == 0 and api.set_rgb(h, None) == 0
        for bad in (dict(dtype=4), dict(dtype=-1), dict(matrix=3), dict(matrix=8), dict(matrix=2), dict(range=3), dict(matrix=-1), dict(planar=2)):
            s = api.rgb_spec()
            for k, v in bad.items():
                setattr(s, k, v)
            assert api.set_rgb(h, s) == -1, bad
        assert api.set_rgb(h, "u8", matrix=9, range=2) == 0
        assert L.jm_amddec_set_option(h, b"parse_only", 1) == 0
        assert api.jm_nvdec_init(0, 1, None, 0, h) == 0
        assert api.set_rgb(h, "f32") == -1 and api.set_rgb(h, None) == -1                # after init
    finally:
        api.jm_nvdec_deinit(h)


def test_rgb_device_refuses_an_auto_matrix_a_misaligned_destination_and_bad_ratios():
    # (refused before anything touches the device: the addresses are never dereferenced)
    s = api.rgb_spec("u8", matrix=0)
    assert api.rgb_device(1 << 20, 128, 128 * 64, 64, 64, (0, 0, 64, 64), (64, 64), s, 1 << 21) == -1
    s = api.rgb_spec("f32", matrix=1)
    assert api.rgb_device(1 << 20, 128, 128 * 64, 64, 64, (0, 0, 64, 64), (64, 64), s, (1 << 21) + 2) == -1
    s = api.rgb_spec("u8", matrix=1)
    assert api.rgb_device(1 << 20, 128, 128 * 64, 64, 64, (0, 0, 64, 64), (6, 64), s, 1 << 21) == -1          # beyond 8:1


@pytest.mark.parametrize("codec", [0, 1])
def test_parse_only_rgb_handles_report_rgb_frame_bytes(codec):
    for dtype, size in (("u8", 1), ("f32", 4), ("f16", 2), ("bf16", 2)):
        lens, st, text = _parse(GEN[codec](), codec, rgb=dict(dtype=dtype, planar=dtype != "f16"))
        assert lens == [3 * 64 * 48 * size] * 2 and st["out_frame_bytes"] == 3 * 64 * 48 * size, dtype
        assert ("RGB planar " if dtype != "f16" else "RGB interleaved ") + dtype in text
    lens, st, _ = _parse(GEN[codec](), codec, rgb=dict(dtype="f32", bgr=True), crop_x=8, crop_w=32, target_width=16, target_height=24)
    assert lens == [3 * 16 * 24 * 4] * 2 and st["out_frame_bytes"] == 3 * 16 * 24 * 4
    lens, st, text = _parse(GEN[codec](), codec)
    assert lens == [64 * 48 * 3 // 2] * 2 and st["out_frame_bytes"] == 64 * 48 * 3 // 2 and "YV12" in text
