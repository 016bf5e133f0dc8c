"""RGB output, host side (no GPU): the colour coefficients against an exact rational computation, a numpy restatement of the conversion C
(INTEGRATION.md "RGB output") and its closed forms, the lane routines of both k_rgb_pack instantiations (jmcodec_amd/csrc/rgb_packed.h) walked over
whole frames on the CPU, the colour description of both parsers, and the RGB spec of parse-only handles.  The restatement and the case list here are
what the GPU tests (test_rgb_output_gpu.py) compare the device output with."""
import ctypes as C
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from jmcodec_amd import api
from tools import streams
from test_scaled_output_host import _packout_ref, build_native, load_scale_check, scale_device_cases, scale_frame, scale_walk, split_frame

MATRICES = (1, 4, 5, 6, 7, 9)
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
HIPCC = "/opt/rocm/bin/hipcc"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


# ---- the cases of the stand-alone kernel tests (CPU walk here, the device in test_rgb_output_gpu.py) ------------------------------------
def _case_spec(n, rng):
    """Case n of 192 covers every dtype x layout x order x matrix x range once; floats get the defaults, ImageNet or a random scale / bias."""
    dtype, planar, bgr, matrix, rng_ = n % 4, (n // 4) % 2, (n // 8) % 2, MATRICES[(n // 16) % 6], 1 + (n // 96) % 2
    kind = rng.randrange(3)
    if dtype == 0 or kind == 0:
        return api.rgb_spec(dtype, planar, bgr, matrix, rng_)
    if kind == 1:
        return api.rgb_spec(dtype, planar, bgr, matrix, rng_, **IMAGENET)
    return api.rgb_spec(dtype, planar, bgr, matrix, rng_, scale=[rng.uniform(-2, 2) for _ in range(3)], bias=[rng.uniform(-100, 100) for _ in range(3)])


def _case_geometry(n, rng):
    W, H = rng.randrange(2, 240, 2), rng.randrange(2, 180, 2)
    cw, ch = rng.randrange(2, W + 1, 2), rng.randrange(2, H + 1, 2)
    cx, cy = rng.randrange(0, W - cw + 1, 2), rng.randrange(0, H - ch + 1, 2)
    kind = n % 5                                            # identity, the 8:1 and 1:4 limits, random

    def dst(s):
        lo, hi = -(-s // 8), 4 * s
        lo += lo & 1
        return s if kind == 0 else lo if kind == 1 else hi if kind == 2 else rng.randrange(lo, hi + 1, 2)
    return W, H, (cx, cy, cw, ch), (dst(cw), dst(ch))


def rgb_device_cases():
    """200 seeded cases (sizes that are no multiples of 16, crops, identity / 8:1 / 1:4 / random targets, lone_field 0 / 1 / 2, every sample type,
    layout, order, matrix and range, random surface bytes with 0 and 255); yields (n, spec, W, H, crop, target, pitch, lone, hs, src)."""
    rng = random.Random(0xC0105)
    for n in range(200):
        spec = _case_spec(n % 192, rng)
        W, H, crop, target = _case_geometry(n, rng)
        pitch = W + rng.choice([0, 2, 14, 128 - W % 128])
        lone = rng.randrange(3)
        hs = H + (16 if lone and H % 4 else rng.choice([0, 16]))
        src = np.random.default_rng(n).integers(0, 256, pitch * hs * 3 // 2, dtype=np.uint8)
        src[::7], src[3::11] = 0, 255
        yield n, spec, W, H, crop, target, pitch, lone, hs, src


# ---- rgb_packed.h: k_rgb_pack's lanes on the CPU ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc: the f16 samples need its clang (_Float16)")
    l = build_native("rgb_packed_check", [HIPCC, "-x", "c++"], ("scale_packed.h", "rgb_packed.h", "mc_packed.h", "jobs.h"),
                     ("scale_packed_walk.h", "rgb_packed_walk.h"))
    l.rgbp_frame.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3
    return l


@pytest.fixture(scope="module")
def scale_lib():
    return load_scale_check()


def rgb_walk(lib, src, pitch, hs, crop, target, spec, lone, coefs=None, misalign=0, guard=64):
    """k_rgb_pack's lanes (the instantiation of the job's kind) over one job on the CPU.  The frame starts `misalign` samples behind a 16-byte boundary
    and has `guard` bytes of 0xA5 before and behind it, which must stay."""
    src = np.ascontiguousarray(src)
    sz = api.RGB_SAMPLE_BYTES[spec.dtype]
    out_n = 3 * target[0] * target[1] * sz
    raw = np.full(out_n + 2 * guard + 16 + misalign * sz, 0xA5, np.uint8)
    off = guard + (-(raw.ctypes.data + guard)) % 16 + misalign * sz
    coefs = (C.c_int * 5)(*(coefs or api.color_coefs(spec.matrix, spec.range == 2)))
    scale, bias = (C.c_float * 3)(*spec.scale), (C.c_float * 3)(*spec.bias)
    rc = lib.rgbp_frame(src.ctypes.data, pitch, pitch * hs, lone, *crop, *target, coefs, int(spec.range == 2), spec.dtype, spec.planar, spec.bgr, scale, bias,
                        raw.ctypes.data + off)
    assert rc == 0, rc
    assert (raw[:off] == 0xA5).all() and (raw[off + out_n:] == 0xA5).all(), "bytes outside the frame were written"
    return raw[off:off + out_n].tobytes()


def _describe(n, W, H, crop, target, lone, spec):
    return (f"case {n}: {W}x{H} crop {crop} -> {target} lone {lone} dtype {spec.dtype} planar {spec.planar} bgr {spec.bgr} matrix {spec.matrix} "
            f"range {spec.range}")


def test_rgb_packed_walk_equals_the_restatement(lib):
    """Every tile of every one of the device test's 200 cases (every dtype, layout, order, matrix and range; identity and scaled jobs), 256 lanes per
    tile in the kernel's order, byte for byte against C(R_G(F))."""
    kinds = set()
    for n, spec, W, H, crop, target, pitch, lone, hs, src in rgb_device_cases():
        got = rgb_walk(lib, src, pitch, hs, crop, target, spec, lone)
        want = rgb_frame(_packout_ref(src, pitch, hs, W, H, lone, 1), W, H, 1, crop, target, spec, spec.matrix, spec.range == 2)
        assert got == want, _describe(n, W, H, crop, target, lone, spec)
        kinds.add((spec.dtype, target == crop[2:]))
    assert len(kinds) == 8                                  # each dtype through both instantiations


@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
def test_rgb_packed_walk_with_a_misaligned_destination(lib, dtype):
    """A frame that starts one sample behind a 16-byte boundary: no vector store of a planar row start is aligned, store4's scalar tails run."""
    rng = np.random.default_rng(0xA11 + dtype)
    W, H, pitch = 70, 22, 72
    src = rng.integers(0, 256, pitch * H * 3 // 2, dtype=np.uint8)
    for planar in (1, 0):
        for crop, target in (((0, 0, W, H), (W, H)), ((2, 2, 66, 18), (50, 26))):
            spec = api.rgb_spec(dtype, planar, 0, 1, 1, **({} if dtype == 0 else IMAGENET))
            got = rgb_walk(lib, src, pitch, H, crop, target, spec, 0, misalign=1)
            want = rgb_frame(_packout_ref(src, pitch, H, W, H, 0, 1), W, H, 1, crop, target, spec, 1, False)
            assert got == want, (dtype, planar, crop, target)


def test_rgb_luma_of_a_scaled_tile_is_k_scale_packs(lib, scale_lib):
    """G is shared: with cy = 1, no chroma terms, full range and u8, k_rgb_pack's R = G = B = the luma of G, which must be k_scale_pack's output for
    the same geometry (both go through the same lane routines)."""
    spec = api.rgb_spec(0, 1, 0, 1, 2)
    seen = 0
    for n, W, H, crop, target, pitch, lone, fmt, hs, src in scale_device_cases():
        if n % 8 or target == crop[2:]:
            continue
        rgb = rgb_walk(lib, src, pitch, hs, crop, target, spec, lone, coefs=(16384, 0, 0, 0, 0))
        Y = scale_walk(scale_lib, src, pitch, hs, crop, target, fmt, lone)[:target[0] * target[1]]
        assert rgb == Y * 3, f"case {n}"
        seen += 1
    assert seen >= 25


def test_out_packed_asan_builds_and_runs_clean(tmp_path):
    """tools/out_packed_asan.cpp: both walks over edge geometries under AddressSanitizer / UBSan, every buffer of the exact size."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc: the program is built with its clang")
    out = tmp_path / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "out_packed_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(out / "out_packed_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ok: 198 walks" in r.stdout
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]


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
