"""Placed output, host side (no GPU): the letterbox rectangle against its formula, a numpy restatement of INTEGRATION.md "Placed output" on top of
the restatements of R_G and C, the placed paths of the lane routines (scale_packed.h, rgb_packed.h) walked over whole frames on the CPU, the sample
aspect ratio of both parsers, and the placement options of parse-only handles.  The restatement and the case list here are what the GPU tests
(test_placed_output_gpu.py) compare the device output with."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from jmcodec_amd import api
from tools import streams
from test_scaled_output_host import _packout_ref, build_native, join_frame, load_scale_check, scale_frame, scale_walk, split_frame
from test_rgb_output_host import convert, f32_to_bf16_bits

HIPCC = "/opt/rocm/bin/hipcc"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_DTYPE = {0: np.uint8, 1: np.float32, 2: np.float16, 3: np.uint16}
SAR_TABLE = {1: (1, 1), 2: (12, 11), 3: (10, 11), 4: (16, 11), 5: (40, 33), 6: (24, 11), 7: (20, 11), 8: (32, 11), 9: (80, 33), 10: (18, 11),
             11: (15, 11), 12: (64, 33), 13: (160, 99), 14: (4, 3), 15: (3, 2), 16: (2, 1)}


# ---- "Placed output" restated ------------------------------------------------------------------------------------------------------
def fit_rect_ref(cw, ch, tw, th, fit=1, sar=(0, 0)):
    """The letterbox rectangle (x, y, w, h) in Python integers."""
    sn, sd = sar if sar[0] and sar[1] else (1, 1)
    Wp, Hp = cw * sn, ch * sd
    if Wp * th >= Hp * tw:
        rw, rh = tw, min(max(2 * ((tw * Hp + Wp) // (2 * Wp)), 2), th)
    else:
        rw, rh = min(max(2 * ((th * Wp + Hp) // (2 * Hp)), 2), tw), th
    if fit == 2:
        return 0, 0, rw, rh
    return 2 * ((tw - rw) // 4), 2 * ((th - rh) // 4), rw, rh


def place_frame(F, W, H, fmt, crop, target, rect, fill=(16, 128, 128)):
    """L: the 4:2:0 frame of a Y'CbCr handle -- P = R(F) with destination rw x rh inside the rectangle, the fill outside, chroma on the half grid."""
    tw, th = target
    rx, ry, rw, rh = rect
    planes = split_frame(scale_frame(F, W, H, fmt, crop, (rw, rh)), rw, rh, fmt)
    out = []
    for k, p in enumerate(planes):
        s = 1 if k == 0 else 2
        L = np.full((th // s, tw // s), fill[k], np.uint8)
        L[ry // s:(ry + rh) // s, rx // s:(rx + rw) // s] = p
        out.append(L)
    return join_frame(*out, fmt)


def fill_samples(fill, spec):
    """The three samples of the fill colour in storage order: the accumulator fill_c << 14 through C's sample step."""
    chans = fill[::-1] if spec.bgr else fill
    out = []
    for c, v in enumerate(chans):
        a = np.int64(v) << 14
        if spec.dtype == 0:
            out.append(np.uint8((a + 8192) >> 14))
            continue
        k = np.float32(spec.scale[c]) * np.float32(2.0 ** -14)
        f = np.float32(np.float32(np.float32(a) * k) + np.float32(spec.bias[c]))
        out.append(f if spec.dtype == 1 else np.float16(f) if spec.dtype == 2 else f32_to_bf16_bits(f))
    return out


def place_rgb_frame(F, W, H, crop, target, rect, spec, matrix, full, fill=(0, 0, 0)):
    """The frame of an RGB handle: C of L's samples inside the rectangle, the fill colour's samples outside."""
    tw, th = target
    rx, ry, rw, rh = rect
    Y, U, V = split_frame(place_frame(F, W, H, 1, crop, target, rect), tw, th, 1)
    raw = convert(Y, U, V, spec.dtype, spec.planar, spec.bgr, matrix, full, tuple(spec.scale), tuple(spec.bias))
    a = np.frombuffer(raw, NP_DTYPE[spec.dtype]).reshape((3, th, tw) if spec.planar else (th, tw, 3)).copy()
    chw = a if spec.planar else a.transpose(2, 0, 1)
    inside = np.zeros((th, tw), bool)
    inside[ry:ry + rh, rx:rx + rw] = True
    for c, v in enumerate(fill_samples(fill, spec)):
        chw[c][~inside] = v
    return a.tobytes()


# ---- the cases of the stand-alone tests (CPU walk here, the device in test_placed_output_gpu.py) ------------------------------------
#       name                          W    H   crop               target     rect
GEOMETRIES = [
    ("rx%4==2, odd chroma origin", 120,  68, (0, 0, 120, 68),   (96, 48),  (2, 2, 60, 34)),
    ("rectangle 2x2",                8,   8, (0, 0, 8, 8),      (32, 16),  (10, 6, 2, 2)),
    ("inside one tile",             40,  20, (0, 0, 40, 20),    (128, 32), (70, 18, 20, 10)),
    ("crosses column 64 and row 16", 100, 40, (0, 0, 100, 40),  (128, 48), (40, 8, 50, 20)),
    ("most tiles fill only",        64,  32, (0, 0, 64, 32),    (160, 64), (128, 48, 32, 16)),
    ("target no multiple of 4",     90,  70, (2, 4, 80, 60),    (70, 38),  (6, 2, 58, 34)),
    ("pure padding",                90,  70, (0, 0, 90, 70),    (96, 80),  (4, 6, 90, 70)),
    ("8:1 down",                   480, 272, (0, 0, 480, 272),  (96, 48),  (18, 6, 60, 34)),
    ("1:4 up",                      16,  10, (0, 0, 16, 10),    (96, 48),  (16, 4, 64, 40)),
    ("up to the edge",              60,  44, (4, 2, 52, 40),    (98, 50),  (46, 14, 52, 36)),
]


def placed_cases():
    """Every geometry with both out_fmts; the first and the pure-padding one also with a lone top / bottom field.  Yields
    (n, name, W, H, crop, target, rect, pitch, lone, fmt, hs, src)."""
    n = 0
    for g, (name, W, H, crop, target, rect) in enumerate(GEOMETRIES):
        for lone in ((0, 1, 2) if g in (0, 6) else (0,)):
            for fmt in (0, 1):
                pitch = W + (0, 2, 14)[n % 3]
                hs = H + (16 if lone and H % 4 else 0)
                src = np.random.default_rng(0x91ACE + n).integers(0, 256, pitch * hs * 3 // 2, dtype=np.uint8)
                src[::7], src[3::11] = 0, 255
                yield n, name, W, H, crop, target, rect, pitch, lone, fmt, hs, src
                n += 1


def rgb_specs():
    """Every dtype x planar / interleaved x bgr; floats with a scale and a bias that differ per storage position."""
    for dtype in range(4):
        for planar in (1, 0):
            for bgr in (0, 1):
                kw = {} if dtype == 0 else dict(scale=[1 / 255, 0.5 / 255, 2 / 255], bias=[-0.5, 0.25, 1.0])
                yield api.rgb_spec(dtype, planar, bgr, 1, 1, **kw)


FILL_YUV, FILL_RGB = 0x123456, 0x123456


def _rgb3(v):
    return (v >> 16) & 255, (v >> 8) & 255, v & 255


# ---- the lane routines' placed paths on the CPU ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc: the f16 samples need its clang (_Float16)")
    l = build_native("place_packed_check", [HIPCC, "-x", "c++"], ("scale_packed.h", "rgb_packed.h", "mc_packed.h", "jobs.h"),
                     ("scale_packed_walk.h", "rgb_packed_walk.h", "place_packed_walk.h"))
    l.place_scl_frame.argtypes = [C.c_void_p] + [C.c_int] * 10 + [C.c_void_p, C.c_int, C.c_void_p]
    l.place_rgb_frame.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    return l


def place_scale_walk(lib, src, pitch, hs, crop, target, fmt, lone, rect, fill, guard=64):
    """k_scale_pack's lanes over one placed job; `guard` bytes of 0xA5 around the frame must stay."""
    src = np.ascontiguousarray(src)
    out_n = target[0] * target[1] * 3 // 2
    out = np.full(out_n + 2 * guard, 0xA5, np.uint8)
    rc = lib.place_scl_frame(src.ctypes.data, pitch, pitch * hs, lone, *crop, *target, fmt, (C.c_int * 4)(*rect), fill, out.ctypes.data + guard)
    assert rc == 0, rc
    assert (out[:guard] == 0xA5).all() and (out[guard + out_n:] == 0xA5).all(), "bytes around the frame were written"
    return out[guard:guard + out_n].tobytes()


def place_rgb_walk(lib, src, pitch, hs, crop, target, spec, lone, rect, fill, misalign=0, guard=64):
    """k_rgb_pack's lanes over one placed job; the frame starts `misalign` samples behind a 16-byte boundary, the bytes around it must stay."""
    src = np.ascontiguousarray(src)
    sz = api.RGB_SAMPLE_BYTES[spec.dtype]
    out_n = 3 * target[0] * target[1] * sz
    raw = np.full(out_n + 2 * guard + 16 + misalign * sz, 0xA5, np.uint8)
    off = guard + (-(raw.ctypes.data + guard)) % 16 + misalign * sz
    coefs = (C.c_int * 5)(*api.color_coefs(spec.matrix, spec.range == 2))
    scale, bias = (C.c_float * 3)(*spec.scale), (C.c_float * 3)(*spec.bias)
    rc = lib.place_rgb_frame(src.ctypes.data, pitch, pitch * hs, lone, *crop, *target, coefs, int(spec.range == 2), spec.dtype, spec.planar, spec.bgr,
                             scale, bias, (C.c_int * 4)(*rect), fill, raw.ctypes.data + off)
    assert rc == 0, rc
    assert (raw[:off] == 0xA5).all() and (raw[off + out_n:] == 0xA5).all(), "bytes around the frame were written"
    return raw[off:off + out_n].tobytes()


def test_placed_scale_walk_equals_the_restatement(lib):
    """Every tile of every case -- fill-only, full and partial tiles, lanes that are part fill and part picture, the I420 lane mapping -- byte for
    byte against L, with the default fill and with 0x123456."""
    count = 0
    for n, name, W, H, crop, target, rect, pitch, lone, fmt, hs, src in placed_cases():
        F = _packout_ref(src, pitch, hs, W, H, lone, fmt)
        for fill in (0x108080, FILL_YUV):
            got = place_scale_walk(lib, src, pitch, hs, crop, target, fmt, lone, rect, fill)
            assert got == place_frame(F, W, H, fmt, crop, target, rect, _rgb3(fill)), f"case {n} ({name}) lone {lone} fmt {fmt} fill {fill:#x}"
        count += 1
    assert count == 28


def test_placed_rgb_walk_equals_the_restatement(lib):
    """Every case x every dtype x layout x order: C inside the rectangle, the fill through the sample step of its storage position outside; pure
    padding runs the instantiation without LDS."""
    kinds = set()
    for n, name, W, H, crop, target, rect, pitch, lone, fmt, hs, src in placed_cases():
        if fmt:
            continue
        F = _packout_ref(src, pitch, hs, W, H, lone, 1)
        for spec in rgb_specs():
            got = place_rgb_walk(lib, src, pitch, hs, crop, target, spec, lone, rect, FILL_RGB)
            want = place_rgb_frame(F, W, H, crop, target, rect, spec, 1, False, _rgb3(FILL_RGB))
            assert got == want, f"case {n} ({name}) lone {lone} dtype {spec.dtype} planar {spec.planar} bgr {spec.bgr}"
            kinds.add((spec.dtype, rect[2:] == crop[2:]))
    assert len(kinds) == 8


@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
def test_placed_rgb_walk_with_a_misaligned_destination(lib, dtype):
    """A frame that starts one sample off a 16-byte boundary, default fill (black): the scalar tails of store4 with mixed lanes."""
    for g in (0, 6):
        name, W, H, crop, target, rect = GEOMETRIES[g]
        src = np.random.default_rng(0xA11 + dtype + g).integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
        F = _packout_ref(src, W, H, W, H, 0, 1)
        for spec in rgb_specs():
            if spec.dtype != dtype:
                continue
            got = place_rgb_walk(lib, src, W, H, crop, target, spec, 0, rect, 0, misalign=1)
            assert got == place_rgb_frame(F, W, H, crop, target, rect, spec, 1, False), (name, dtype, spec.planar, spec.bgr)


def test_an_unplaced_job_gives_todays_bytes(lib):
    """rw == 0 (and a rectangle that is the whole target) is no placement: the bytes of the unplaced walk and of R_G."""
    old = load_scale_check()
    for n, name, W, H, crop, target, rect, pitch, lone, fmt, hs, src in placed_cases():
        want = scale_walk(old, src, pitch, hs, crop, (rect[2], rect[3]), fmt, lone)
        assert want == scale_frame(_packout_ref(src, pitch, hs, W, H, lone, fmt), W, H, fmt, crop, (rect[2], rect[3]))
        for r in ((0, 0, 0, 0), (0, 0, rect[2], rect[3])):
            assert place_scale_walk(lib, src, pitch, hs, crop, (rect[2], rect[3]), fmt, lone, r, FILL_YUV) == want, (n, name, r)
    spec = api.rgb_spec(2, 0, 1, 1, 1, scale=[1 / 255] * 3)
    name, W, H, crop, target, rect = GEOMETRIES[5]
    src = np.random.default_rng(5).integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    F = _packout_ref(src, W, H, W, H, 0, 1)
    got = place_rgb_walk(lib, src, W, H, crop, target, spec, 0, (0, 0, 0, 0), FILL_RGB)
    Y, U, V = split_frame(scale_frame(F, W, H, 1, crop, target), target[0], target[1], 1)
    assert got == convert(Y, U, V, 2, 0, 1, 1, False, tuple(spec.scale), tuple(spec.bias))


def test_place_packed_asan_builds_and_runs_clean(tmp_path):
    """tools/place_packed_asan.cpp: the placed walks under AddressSanitizer / UBSan; source, destination and tap tables of the exact size."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc: the program is built with its clang")
    out = tmp_path / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "place_packed_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(out / "place_packed_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ok: 216 walks" in r.stdout
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]


# ---- the letterbox rectangle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,want", [
    ((1920, 1080, 640, 640, 1, (0, 0)), (0, 140, 640, 360)),        # 16:9 into a square
    ((640, 480, 416, 416, 1, (0, 0)), (0, 52, 416, 312)),           # 4:3 into a square
    ((1080, 1920, 640, 640, 1, (0, 0)), (140, 0, 360, 640)),        # portrait: bars left and right
    ((1440, 1080, 640, 640, 1, (4, 3)), (0, 140, 640, 360)),        # anamorphic 1440x1080 is 16:9
    ((720, 576, 512, 512, 1, (16, 15)), (0, 64, 512, 384)),         # 720x576 at 16:15 is 4:3
    ((720, 576, 512, 512, 2, (16, 15)), (0, 0, 512, 384)),          # ... at the top left
    ((1920, 1080, 960, 540, 1, (0, 0)), (0, 0, 960, 540)),          # already the target's shape
    ((4000, 2, 64, 64, 1, (0, 0)), (0, 30, 64, 2)),                 # the clamp to 2
    ((2, 4000, 64, 64, 1, (0, 0)), (30, 0, 2, 64)),
])
def test_fit_rect_known_answers(args, want):
    cw, ch, tw, th, fit, sar = args
    assert fit_rect_ref(cw, ch, tw, th, fit, sar) == want
    assert api.fit_rect(cw, ch, tw, th, fit, sar) == want


def test_fit_rect_equals_the_formula():
    rng = np.random.default_rng(0xF17)
    sars = [(0, 0), (1, 1), (4, 3), (16, 15), (12, 11), (160, 99), (65535, 1), (1, 65535), (0, 5), (7, 0)]
    for _ in range(3000):
        cw, ch = (int(v) for v in rng.integers(1, 8193, 2))
        tw, th = (2 * int(v) for v in rng.integers(1, 2049, 2))
        fit, sar = int(rng.integers(1, 3)), sars[int(rng.integers(len(sars)))]
        got = api.fit_rect(cw, ch, tw, th, fit, sar)
        assert got == fit_rect_ref(cw, ch, tw, th, fit, sar), (cw, ch, tw, th, fit, sar)
        x, y, w, h = got
        assert x % 2 == y % 2 == w % 2 == h % 2 == 0 and w >= 2 and h >= 2 and x + w <= tw and y + h <= th and (w == tw or h == th)


def test_fit_rect_refuses_invalid_arguments():
    for a in ((0, 4, 8, 8, 1), (4, 0, 8, 8, 1), (4, 4, 7, 8, 1), (4, 4, 8, 0, 1), (4, 4, 8, 8, 0), (4, 4, 8, 8, 3), (4, 4, -8, 8, 1)):
        assert api.fit_rect(*a) is None, a
    assert api.fit_rect(4, 4, 8, 8, 1, (-1, 1)) is None
    assert api.lib().jm_amddec_fit_rect(4, 4, 1, 1, 8, 8, 1, None) == -1


# ---- sample aspect ratio of both parsers -----------------------------------------------------------------------------------------------
def _h264(**kw):
    return streams.generate(width=96, height=80, frames=2, gop=2, mode=1, seed=0x5A2, **kw)


def _hevc(**kw):
    return streams.generate_hevc(width=96, height=80, frames=2, ctb_log2=5, mode=1, seed=7, **kw)


GEN = {0: _h264, 1: _hevc}


def _parse(data, codec=0, rgb=None, **opts):
    """Decode with a parse-only handle; returns (stats, frame lengths or None, last_error, info text, stream_info)."""
    o = {"parse_only": 1}
    o.update(opts)
    with api.JmAmdDec(codec, 1, options=o, **({"rgb": rgb} if rgb is not None else {})) as d:
        try:
            lens = [len(f) for f in d.decode_stream(data)]
        except RuntimeError:
            lens = None
        keys = ("rect_x", "rect_y", "rect_w", "rect_h", "placed_frames", "sar_num", "sar_den", "out_width", "out_height", "out_frame_bytes", "scaled_frames")
        st = {k: d.stat(k) for k in keys}
        return st, lens, api.lib().jm_amddec_last_error(d.h).decode(), api.jm_nvdec_show_dec_info(d.h), api.jm_nvdec_stream_info(d.h)


@pytest.mark.parametrize("codec", [0, 1])
def test_sar_table_extended_and_absent(codec):
    for idc, want in SAR_TABLE.items():
        st = _parse(GEN[codec](vui_sar_idc=idc), codec)[0]
        assert (st["sar_num"], st["sar_den"]) == want, idc
    st = _parse(GEN[codec](vui_sar_idc=255, vui_sar_w=64, vui_sar_h=45), codec)[0]
    assert (st["sar_num"], st["sar_den"]) == (64, 45)
    st = _parse(GEN[codec](vui_sar_idc=255, vui_sar_w=65535, vui_sar_h=1), codec)[0]
    assert (st["sar_num"], st["sar_den"]) == (65535, 1)
    for kw in (dict(), dict(vui_sar_idc=17), dict(vui_sar_idc=200), dict(vui_sar_idc=255, vui_sar_w=0, vui_sar_h=9), dict(vui_sar_idc=255, vui_sar_w=9)):
        st = _parse(GEN[codec](**kw), codec)[0]
        assert (st["sar_num"], st["sar_den"]) == (0, 0), kw
    # the fields behind the aspect ratio are still found
    st = _parse(GEN[codec](vui_sar_idc=255, vui_sar_w=4, vui_sar_h=3, vui_fps=25), codec)[0]
    assert (st["sar_num"], st["sar_den"]) == (4, 3)


@pytest.mark.parametrize("codec", [0, 1])
def test_streams_without_sar_parameters_are_unchanged(codec):
    assert GEN[codec]() == GEN[codec](vui_sar_idc=0, vui_sar_w=0, vui_sar_h=0)
    assert GEN[codec](vui_fps=25) == GEN[codec](vui_fps=25, vui_sar_w=5, vui_sar_h=7)       # (w / h alone mean nothing)
    assert GEN[codec](vui_fps=25) == GEN[codec](vui_fps=25, vui_sar_idc=1)                  # idc 1 is what a VUI carried before


# ---- options of parse-only handles ---------------------------------------------------------------------------------------------------------
def test_placement_options_validate():
    L = api.lib()
    h = api.jm_nvdec_create_handle()
    try:
        for k in ("rect_x", "rect_y", "rect_w", "rect_h"):
            for bad in (3, -2, 32770, 1 << 40):
                assert L.jm_amddec_set_option(h, k.encode(), bad) == -1, (k, bad)
            assert L.jm_amddec_set_option(h, k.encode(), 64) == 0 and L.jm_amddec_set_option(h, k.encode(), 0) == 0
        for k, good, bad in (("fit", (0, 1, 2), (-1, 3)), ("fit_sar", (0, 1), (-1, 2)), ("fill", (-1, 0, 0x123456, 0xFFFFFF), (-2, 0x1000000))):
            for v in bad:
                assert L.jm_amddec_set_option(h, k.encode(), v) == -1, (k, v)
            for v in good:
                assert L.jm_amddec_set_option(h, k.encode(), v) == 0, (k, v)
        assert L.jm_amddec_set_option(h, b"parse_only", 1) == 0
        assert api.jm_nvdec_init(0, 1, None, 0, h) == 0
        for k in ("rect_x", "rect_y", "rect_w", "rect_h", "fit", "fit_sar", "fill"):
            assert L.jm_amddec_set_option(h, k.encode(), 0) == -1, k
    finally:
        api.jm_nvdec_deinit(h)


@pytest.mark.parametrize("codec", [0, 1])
def test_fit_reports_the_target_and_the_rectangle(codec):
    st, lens, err, text, info = _parse(GEN[codec](), codec, target_width=64, target_height=64, fit=1)
    want = fit_rect_ref(96, 80, 64, 64)
    assert want == (0, 4, 64, 54)
    assert info == (64, 64) and lens == [64 * 64 * 3 // 2] * 2, err
    assert (st["rect_x"], st["rect_y"], st["rect_w"], st["rect_h"]) == want
    assert (st["out_width"], st["out_height"], st["out_frame_bytes"], st["placed_frames"]) == (64, 64, 64 * 64 * 3 // 2, 2)
    assert "Display:\t64 x 64" in text and "Placement:\t0,4 64x54" in text
    # top left, and the sample aspect ratio only with fit_sar
    st = _parse(GEN[codec](vui_sar_idc=14), codec, target_width=64, target_height=64, fit=2)[0]
    assert (st["rect_x"], st["rect_y"], st["rect_w"], st["rect_h"]) == (0, 0, 64, 54)
    st = _parse(GEN[codec](vui_sar_idc=14), codec, target_width=64, target_height=64, fit=1, fit_sar=1)[0]
    assert (st["rect_x"], st["rect_y"], st["rect_w"], st["rect_h"]) == fit_rect_ref(96, 80, 64, 64, 1, (4, 3)) == (0, 12, 64, 40)
    # the crop is what is fitted
    st = _parse(GEN[codec](), codec, crop_x=8, crop_w=40, target_width=64, target_height=64, fit=1)[0]
    assert (st["rect_x"], st["rect_y"], st["rect_w"], st["rect_h"]) == fit_rect_ref(40, 80, 64, 64) == (16, 0, 32, 64)


def test_explicit_rectangle_and_rgb_handle():
    st, lens, err, text, info = _parse(_h264(), target_width=128, target_height=96, rect_x=16, rect_y=8)
    assert (st["rect_x"], st["rect_y"], st["rect_w"], st["rect_h"]) == (16, 8, 112, 88) and info == (128, 96), err
    assert "Placement:\t16,8 112x88" in text
    st, lens, err, _, info = _parse(_h264(), rgb=api.rgb_spec("f16", planar=False), target_width=128, target_height=96, rect_x=16, rect_y=8, rect_w=96,
                                    rect_h=80, fill=0x123456)
    assert (st["rect_w"], st["rect_h"], st["placed_frames"]) == (96, 80, 2) and lens == [128 * 96 * 3 * 2] * 2, err


def test_without_the_new_options_nothing_is_placed():
    for opts in (dict(), dict(target_width=64, target_height=48), dict(target_width=64, target_height=48, rect_w=64, rect_h=48), dict(fill=0x445566),
                 dict(target_width=96, target_height=80, fit=1)):
        st, lens, err, text, _ = _parse(_h264(), **opts)
        tw, th = opts.get("target_width", 96), opts.get("target_height", 80)
        assert (st["rect_x"], st["rect_y"], st["rect_w"], st["rect_h"], st["placed_frames"]) == (0, 0, tw, th, 0), (opts, err)
        assert "Placement" not in text and lens == [tw * th * 3 // 2] * 2
    assert _parse(_h264())[0]["scaled_frames"] == 0


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("opts,words", [
    (dict(fit=1), "fit needs both target_width and target_height"),
    (dict(fit=2, target_width=64), "fit needs both target_width and target_height"),
    (dict(fit=1, target_width=64, target_height=64, rect_x=2), "fit and rect_x / rect_y / rect_w / rect_h exclude each other"),
    (dict(target_width=64, target_height=64, rect_x=32, rect_w=34), "the placement rectangle 34x64 at (32, 0) does not lie inside the target 64x64"),
    (dict(target_width=64, target_height=64, rect_y=64), "does not lie inside the target"),
    (dict(rect_x=96), "does not lie inside the target"),
    (dict(target_width=64, target_height=64, rect_w=10, rect_h=10), "the scaling ratio 96x80 -> 10x10 is out of range"),      # 96 > 8 * 10
    (dict(crop_w=8, crop_h=8, target_width=64, target_height=64, rect_w=34, rect_h=8), "the scaling ratio 8x8 -> 34x8 is out of range"),
    # 96x20 stretched to 12x12 is legal (8:1 and 5:3); its letterbox is 12x2, 10:1 down in y
    (dict(crop_w=96, crop_h=20, target_width=12, target_height=12, fit=1), "the scaling ratio 96x20 -> 12x2 is out of range"),
])
def test_activation_errors_say_why(codec, opts, words):
    st, lens, err, _, _ = _parse(GEN[codec](), codec, **opts)
    assert "output geometry" in err and words in err, err
    assert lens is None or lens == []


def test_the_ratio_limits_apply_to_the_rectangle():
    """96x80 into a 1024x1024 target is beyond 1:4 as a stretch and fine as a rectangle; 8:1 down into a corner of a big target too."""
    _, _, err, _, _ = _parse(_h264(), target_width=1024, target_height=1024)
    assert "scaling ratio" in err
    st, lens, err, _, _ = _parse(_h264(), target_width=1024, target_height=1024, rect_w=384, rect_h=320)
    assert lens == [1024 * 1024 * 3 // 2] * 2 and st["placed_frames"] == 2, err
    st, lens, err, _, _ = _parse(_h264(), target_width=1024, target_height=1024, rect_x=1000, rect_y=1000, rect_w=12, rect_h=10)
    assert lens is not None and st["rect_w"] == 12, err
    # ... and to the letterbox: 96 -> 400 is beyond 1:4 as a stretch, the fitted rectangle 76x64 is not
    _, _, err, _, _ = _parse(_h264(), target_width=400, target_height=64)
    assert "scaling ratio" in err
    st, lens, err, _, _ = _parse(_h264(), target_width=400, target_height=64, fit=1)
    assert lens == [400 * 64 * 3 // 2] * 2 and (st["rect_x"], st["rect_y"], st["rect_w"], st["rect_h"]) == fit_rect_ref(96, 80, 400, 64) == (162, 0, 76, 64), err


@pytest.mark.parametrize("codec", [0, 1])
def test_a_sample_aspect_ratio_change_resolves_the_rectangle_again(codec):
    """Two sequences of the same size, sample aspect ratio 1:1 then 4:3: with fit_sar 1 the second one is activated again (the handle is drained, the
    rectangle computed again); with fit_sar 0 nothing changes."""
    data = GEN[codec](vui_sar_idc=1) + GEN[codec](vui_sar_idc=14)
    for fit_sar, want in ((1, [(0, 4, 64, 54), (0, 12, 64, 40)]), (0, [(0, 4, 64, 54)])):
        seen, frames = [], []
        with api.JmAmdDec(codec, 1, options=dict(parse_only=1, target_width=64, target_height=64, fit=1, fit_sar=fit_sar)) as d:
            for nal in api.split_nalus(data) + [None] * 64:
                if api.jm_nvdec_is_exit(d.h):
                    break
                _, got = api.jm_nvdec_decode_frame(nal, len(nal) if nal else 0, d.h)
                r = tuple(d.stat(k) for k in ("rect_x", "rect_y", "rect_w", "rect_h"))
                if r[2] and (not seen or seen[-1] != r):
                    seen.append(r)
                if got == 1:
                    d._pull(frames)
            assert d.stat("errors") == 0 and d.stat("failed") == 0 and (d.stat("sar_num"), d.stat("sar_den")) == (4, 3)
            assert d.stat("placed_frames") == 4
        assert seen == want and [len(f) for f in frames] == [64 * 64 * 3 // 2] * 4, (fit_sar, seen)
