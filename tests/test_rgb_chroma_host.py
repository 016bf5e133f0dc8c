"""Interpolated chroma of the RGB output (options rgb_chroma / chroma_loc), host side (no GPU): the chroma tap builder against a numpy restatement
of INTEGRATION.md "RGB output" (C applied to the 4:4:4 frame G'), the closed forms it must satisfy, the lane routines of k_rgb_pack444
(jmcodec_amd/csrc/chroma_packed.h) walked over whole frames on the CPU, the chroma sample location of both parsers, and the two options of parse-only
handles.  The restatement and the case list here are what the GPU tests (test_rgb_chroma_gpu.py) compare the device output with."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

from jmcodec_amd import api
from tools import streams
from test_scaled_output_host import _packout_ref, build_native, scale_frame, split_frame, taps_ref
from test_rgb_output_host import MATRICES, IMAGENET, coefs_ref, f32_to_bf16_bits, rgb_frame
from test_placed_output_host import NP_DTYPE, fill_samples

HIPCC = "/opt/rocm/bin/hipcc"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition restated ---------------------------------------------------------------------------------------------------
def siting(loc):
    """(q horizontal, q vertical) of chroma_sample_loc_type 0..5."""
    return (0 if loc & 1 else -1), (0 if loc < 2 else -1 if loc < 4 else 1)


def chroma_taps_ref(Sc, D, q):
    """Per output j: (first source index, [weights]) of one chroma axis, Sc chroma samples -> D outputs of the full target, siting shift q."""
    out = []
    for j in range(D):
        if D >= Sc:
            num = 2 * (2 * j + 1) * Sc - (2 + q) * D
            i0 = num // (4 * D)
            f = num - 4 * D * i0
            w1 = (f * 16384 + 2 * D) // (4 * D)
            out.append((i0, [16384 - w1, w1]))
        else:
            lo = (4 * j * Sc - q * D) // (4 * D)
            hi = -((-(4 * (j + 1) * Sc - q * D)) // (4 * D))
            a = [min((4 * k + 4 + q) * D, 4 * (j + 1) * Sc) - max((4 * k + q) * D, 4 * j * Sc) for k in range(lo, hi)]
            w = [x * 16384 // (4 * Sc) for x in a]
            w[a.index(max(a))] += 16384 - sum(w)
            out.append((lo, w))
    return out


def _gather(table, S):
    T = max(len(w) for _, w in table)
    idx = np.zeros((len(table), T), np.int64)
    wt = np.zeros((len(table), T), np.int64)
    for j, (f, w) in enumerate(table):
        for k in range(T):
            idx[j, k] = min(max(f + k, 0), S - 1)
            wt[j, k] = w[k] if k < len(w) else 0
    return idx, wt


def resample_chroma(p, tw, th, loc):
    """One chroma plane of the crop (Sc x Sc') -> tw x th: R_G's two passes and roundings with the shifted tables."""
    p = p.astype(np.int64)
    ch, cw = p.shape
    qx, qy = siting(loc)
    ix, wx = _gather(chroma_taps_ref(cw, tw, qx), cw)
    iy, wy = _gather(chroma_taps_ref(ch, th, qy), ch)
    h = np.zeros((ch, tw), np.int64)
    for k in range(ix.shape[1]):
        h += wx[:, k][None, :] * p[:, ix[:, k]]
    h = (h + 64) >> 7
    o = np.zeros((th, tw), np.int64)
    for k in range(iy.shape[1]):
        o += wy[:, k][:, None] * h[iy[:, k], :]
    return np.minimum(255, (o + (1 << 20)) >> 21).astype(np.uint8)


def frame444(F, W, H, crop, size, loc):
    """G' for a tight I420 frame F: (Y, Cb, Cr), each size[1] x size[0]."""
    x, y, cw, ch = crop
    tw, th = size
    Y, U, V = split_frame(F, W, H, 1)
    Gy = split_frame(scale_frame(F, W, H, 1, crop, size), tw, th, 1)[0]
    cu = U[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2]
    cv = V[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2]
    return Gy, resample_chroma(cu, tw, th, loc), resample_chroma(cv, tw, th, loc)


def convert444(Y, U, V, dtype, planar, bgr, matrix, full, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """C pointwise on a 4:4:4 frame, as the bytes the library hands out (test_rgb_output_host.convert with a chroma pair per pixel)."""
    cy, crv, cgu, cgv, cbu = coefs_ref(matrix, full)
    yv = cy * (Y.astype(np.int64) - (0 if full else 16))
    d, e = U.astype(np.int64) - 128, V.astype(np.int64) - 128
    aR, aG, aB = yv + crv * e, yv - cgu * d - cgv * e, yv + cbu * d
    out = []
    for c, a in enumerate([aB, aG, aR] if bgr else [aR, aG, aB]):
        if dtype == 0:
            out.append(np.clip((a + 8192) >> 14, 0, 255).astype(np.uint8))
            continue
        v = np.clip(a, 0, 255 * 16384).astype(np.float32)
        k = np.float32(scale[c]) * np.float32(2.0 ** -14)
        f = ((v * k).astype(np.float32) + np.float32(bias[c])).astype(np.float32)
        out.append(f if dtype == 1 else f.astype(np.float16) if dtype == 2 else f32_to_bf16_bits(f))
    return np.stack(out, 0 if planar else 2).tobytes()


def rgb_chroma_frame(F, W, H, crop, target, spec, matrix, full, loc, rect=None, fill=(0, 0, 0)):
    """The frame of an rgb_chroma 1 handle: C(G'); a placed job: G' has the rectangle's size, the fill colour's samples lie outside it."""
    tw, th = target
    if rect is None or rect[2] == 0 or tuple(rect) == (0, 0, tw, th):
        return convert444(*frame444(F, W, H, crop, target, loc), spec.dtype, spec.planar, spec.bgr, matrix, full, tuple(spec.scale), tuple(spec.bias))
    rx, ry, rw, rh = rect
    inner = convert444(*frame444(F, W, H, crop, (rw, rh), loc), spec.dtype, 1, spec.bgr, matrix, full, tuple(spec.scale), tuple(spec.bias))
    inner = np.frombuffer(inner, NP_DTYPE[spec.dtype]).reshape(3, rh, rw)
    chw = np.zeros((3, th, tw), NP_DTYPE[spec.dtype])
    for c, v in enumerate(fill_samples(fill, spec)):
        chw[c][:] = v
    chw[:, ry:ry + rh, rx:rx + rw] = inner
    return (chw if spec.planar else np.ascontiguousarray(chw.transpose(1, 2, 0))).tobytes()


# ---- the cases of the stand-alone kernel tests (CPU walk here, the device in test_rgb_chroma_gpu.py) --------------------------------
FIXED = [  # W, H, crop, target, rect
    (2, 2, (0, 0, 2, 2), (2, 2), None),                               # a 2 x 2 crop: Sc = 1
    (40, 30, (6, 10, 2, 2), (8, 8), None),                            # ... inside a picture, 1:4 up, odd chroma origin
    (70, 22, (2, 2, 66, 18), (50, 26), None),                         # crop_x = 2: the chroma origin is odd
    (400, 200, (0, 0, 400, 200), (50, 26), None),                     # 8:1 down
    (240, 180, (0, 0, 240, 180), (960, 720), None),                   # 1:4 up, the largest target
    (130, 34, (0, 0, 130, 34), (130, 34), None),                      # identity, a width of two tiles and two columns
    (120, 68, (0, 0, 120, 68), (96, 48), (2, 2, 60, 34)),             # placed: rx % 4 == 2
    (100, 40, (0, 0, 100, 40), (128, 48), (40, 8, 50, 20)),           # ... the rectangle crosses column 64 and row 16, edges inside tiles
    (64, 32, (0, 0, 64, 32), (160, 64), (128, 48, 32, 16)),           # ... most tiles are fill only
    (90, 70, (0, 0, 90, 70), (96, 80), (4, 6, 90, 70)),               # ... pure padding
    (8, 8, (0, 0, 8, 8), (32, 16), (10, 6, 2, 2)),                    # ... the smallest rectangle
    (60, 44, (4, 2, 52, 40), (98, 50), (46, 14, 52, 36)),             # ... up to the target's right / bottom edge
]


def _case_geometry(n, rng):
    kind = n % 6                                            # fixed list, identity, the 8:1 and 1:4 limits, random, placed
    if kind == 0:
        return FIXED[(n // 6) % len(FIXED)]
    W, H = rng.randrange(2, 240, 2), rng.randrange(2, 180, 2)
    cw, ch = rng.randrange(2, W + 1, 2), rng.randrange(2, H + 1, 2)
    cx, cy = rng.randrange(0, W - cw + 1, 2), rng.randrange(0, H - ch + 1, 2)

    def dst(s):
        lo, hi = -(-s // 8), 4 * s
        lo += lo & 1
        return s if kind == 1 else lo if kind == 2 else hi if kind == 3 else rng.randrange(lo, min(hi, 400) + 1, 2)
    size = (dst(cw), dst(ch))
    if kind != 5:
        return W, H, (cx, cy, cw, ch), size, None
    rx, ry = rng.randrange(0, 80, 2), rng.randrange(0, 40, 2)
    return W, H, (cx, cy, cw, ch), (rx + size[0] + rng.randrange(0, 80, 2), ry + size[1] + rng.randrange(0, 40, 2)), (rx, ry) + size


def chroma_device_cases(count=156):
    """Seeded cases: sizes that are no multiples of 64 / 16, crops with an odd chroma origin, a 2 x 2 crop, 8:1 down, 1:4 up, identity, placed jobs
    whose rectangle ends inside a tile, pure padding, lone_field 0 / 1 / 2, all six locations, every sample type, both layouts, both orders, every
    matrix and range.  Yields (n, spec, W, H, crop, target, rect, fill, loc, pitch, lone, hs, src)."""
    rng = random.Random(0xC4120A)
    for n in range(count):
        dtype, planar, bgr, matrix, rng_ = n % 4, (n // 4) % 2, (n // 8) % 2, MATRICES[(n // 16) % 6], 1 + (n // 3) % 2
        kw = {} if dtype == 0 else (IMAGENET if n % 3 else dict(scale=[rng.uniform(-2, 2) for _ in range(3)], bias=[rng.uniform(-100, 100) for _ in range(3)]))
        spec = api.rgb_spec(dtype, planar, bgr, matrix, rng_, **kw)
        W, H, crop, target, rect = _case_geometry(n, rng)
        loc = (n // 6 + n) % 6
        pitch = W + rng.choice([0, 2, 14, 128 - W % 128])
        lone = rng.randrange(3)
        hs = H + (16 if lone and H % 4 else rng.choice([0, 16]))
        src = np.random.default_rng(0xC412 + n).integers(0, 256, pitch * hs * 3 // 2, dtype=np.uint8)
        src[::7], src[3::11] = 0, 255
        yield n, spec, W, H, crop, target, rect, (0x123456 if n % 2 else -1), loc, pitch, lone, hs, src


def case_want(spec, W, H, crop, target, rect, fill, loc, pitch, lone, hs, src):
    f = (0, 0, 0) if fill < 0 else ((fill >> 16) & 255, (fill >> 8) & 255, fill & 255)
    return rgb_chroma_frame(_packout_ref(src, pitch, hs, W, H, lone, 1), W, H, crop, target, spec, spec.matrix, spec.range == 2, loc, rect, f)


def describe(n, spec, W, H, crop, target, rect, fill, loc, pitch, lone, *_):
    return (f"case {n}: {W}x{H} crop {crop} -> {target} rect {rect} fill {fill:#x} loc {loc} pitch {pitch} lone {lone} dtype {spec.dtype} "
            f"planar {spec.planar} bgr {spec.bgr} matrix {spec.matrix} range {spec.range}")


# ---- the tap tables ----------------------------------------------------------------------------------------------------------------
def _even_targets(Sc):
    lo = -(-Sc // 4)
    return range(lo + (lo & 1), 8 * Sc + 1, 2)


def test_chroma_taps_equal_the_restatement():
    """jm_amddec_chroma_taps for Sc 1..64, every even D inside the ratios (Sc <= 4 D, D <= 8 Sc) and the three shifts; the properties the issue's
    scratch script checked hold on the way: weights sum to 16384, at most 5 taps, first >= -1, a tap at most one sample past the end."""
    for Sc in range(1, 65):
        for D in _even_targets(Sc):
            for q in (-1, 0, 1):
                ref = chroma_taps_ref(Sc, D, q)
                T = max(len(w) for _, w in ref)
                got = api.chroma_taps(Sc, D, q)
                assert got is not None, (Sc, D, q)
                first, w = got
                assert first == [f for f, _ in ref], (Sc, D, q)
                assert w == [x + [0] * (T - len(x)) for _, x in ref], (Sc, D, q)
                assert T <= 5 and min(first) >= -1 and all(sum(x) == 16384 for x in w)
                assert all(f + len(x) - 1 <= Sc for f, x in ref)
            if D <= 4 * Sc:                                 # (jm_amddec_scale_taps itself stops at 1:4 up; the restatement of R_G's table does not)
                assert api.chroma_taps(Sc, D, 0) == api.scale_taps(Sc, D), (Sc, D)
            assert [(f, x) for f, x in chroma_taps_ref(Sc, D, 0)] == taps_ref(Sc, D), (Sc, D)


def test_chroma_taps_refuse_bad_arguments():
    assert api.chroma_taps(8, 16, 2) is None and api.chroma_taps(8, 16, -2) is None
    assert api.chroma_taps(0, 16, 0) is None and api.chroma_taps(8, 0, 0) is None
    assert api.chroma_taps(33, 8, 0) is None and api.chroma_taps(8, 65, 0) is None            # beyond 4:1 down / 1:8 up
    assert api.chroma_taps(32, 8, 1) is not None and api.chroma_taps(8, 64, -1) is not None
    assert api.lib().jm_amddec_chroma_taps(32, 8, 0, None, None, 0) == 4                         # no buffers: the taps per output
    first, w = (C.c_int * 8)(), (C.c_short * 16)()
    assert api.lib().jm_amddec_chroma_taps(32, 8, 0, first, w, 2) == -1                           # more taps than max_taps


# ---- closed forms --------------------------------------------------------------------------------------------------------------
def _axis(c, D, q):
    """One row of chroma through the horizontal tables alone, exact (weights / 16384 as a fraction of 16384)."""
    Sc = len(c)
    return [sum(w * int(c[min(max(f + k, 0), Sc - 1)]) for k, w in enumerate(ws)) for f, ws in chroma_taps_ref(Sc, D, q)]


def test_identity_geometry_closed_forms():
    c = np.random.default_rng(3).integers(0, 256, 19)
    Sc, D = len(c), 2 * len(c)
    cos = _axis(c, D, -1)                                   # cosited: even pixels take their sample, odd ones the mean of two
    for k in range(Sc):
        assert cos[2 * k] == 16384 * c[k]
        assert cos[2 * k + 1] == 8192 * (c[k] + c[min(k + 1, Sc - 1)])
    cen = _axis(c, D, 0)                                    # centred: 12288 / 4096 alternate, pixel 0 is c_0
    assert cen[0] == 16384 * c[0] and cen[-1] == 16384 * c[-1]
    for k in range(Sc - 1):
        assert cen[2 * k + 1] == 12288 * c[k] + 4096 * c[k + 1] and cen[2 * k + 2] == 4096 * c[k] + 12288 * c[k + 1]
    assert [w for _, w in chroma_taps_ref(Sc, D, 0)][1:3] == [[12288, 4096], [4096, 12288]]
    bot = _axis(c, D, 1)                                    # the mirror image of -1
    assert bot == _axis(c[::-1], D, -1)[::-1]


def test_exact_two_to_one_closed_forms():
    c = np.random.default_rng(4).integers(0, 256, 23)
    Sc = len(c)
    assert _axis(c, Sc, 0) == [16384 * int(v) for v in c]                                           # D = Sc, centred: the chroma plane itself
    got = _axis(c, Sc, -1)
    assert got == [12288 * int(c[j]) + 4096 * int(c[min(j + 1, Sc - 1)]) for j in range(Sc)]       # cosited: 3/4 c_j + 1/4 c_(j+1)
    p = np.random.default_rng(5).integers(0, 256, (9, 11), dtype=np.uint8)
    assert np.array_equal(resample_chroma(p, 11, 9, 1), p)                                          # both passes, loc 1: exact


def test_flat_chroma_stays_flat_and_grey_stays_grey():
    rng = np.random.default_rng(6)
    for loc in range(6):
        for (cw, ch), (tw, th) in (((10, 6), (20, 12)), ((10, 6), (10, 6)), ((33, 17), (10, 8)), ((5, 3), (40, 24)), ((1, 1), (2, 2))):
            for v in (0, 1, 128, 254, 255):
                assert (resample_chroma(np.full((ch, cw), v, np.uint8), tw, th, loc) == v).all(), (loc, cw, ch, tw, th, v)
    W, H = 24, 16
    Y = rng.integers(0, 256, (H, W), dtype=np.uint8)
    F = Y.tobytes() + bytes([128]) * (W * H // 2)
    for m in MATRICES:
        for full in (False, True):
            for loc in (0, 3, 5):
                spec = api.rgb_spec("u8", True, False, m, 2 if full else 1)
                out = np.frombuffer(rgb_chroma_frame(F, W, H, (0, 0, W, H), (36, 20), spec, m, full, loc), np.uint8).reshape(3, -1)
                assert np.array_equal(out[0], out[1]) and np.array_equal(out[1], out[2]), (m, full, loc)


def test_centred_identity_differs_from_nearest_only_in_chroma():
    """C(G') with a flat chroma equals C(R_G(F)); with a chroma edge it does not (the case list below would be vacuous otherwise)."""
    rng = np.random.default_rng(7)
    W, H = 32, 16
    Y = rng.integers(16, 236, (H, W), dtype=np.uint8)
    spec = api.rgb_spec("u8", True, False, 1, 1)
    flat = Y.tobytes() + bytes([90]) * (W * H // 4) + bytes([200]) * (W * H // 4)
    for loc in range(6):
        assert rgb_chroma_frame(flat, W, H, (0, 0, W, H), (W, H), spec, 1, False, loc) == rgb_frame(flat, W, H, 1, (0, 0, W, H), (W, H), spec, 1, False)
    U = np.zeros((H // 2, W // 2), np.uint8)
    U[:, W // 4:] = 255
    edge = Y.tobytes() + U.tobytes() + bytes([128]) * (W * H // 4)
    assert rgb_chroma_frame(edge, W, H, (0, 0, W, H), (W, H), spec, 1, False, 0) != rgb_frame(edge, W, H, 1, (0, 0, W, H), (W, H), spec, 1, False)


# ---- chroma_packed.h: k_rgb_pack444's lanes on the CPU ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc: the f16 samples need its clang (_Float16)")
    l = build_native("chroma_packed_check", [HIPCC, "-x", "c++"], ("scale_packed.h", "rgb_packed.h", "chroma_packed.h", "mc_packed.h", "jobs.h"),
                     ("scale_packed_walk.h", "rgb_packed_walk.h", "place_packed_walk.h", "chroma_packed_walk.h"))
    l.chroma_rgb_frame.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p]
    return l


def chroma_walk(lib, src, pitch, hs, crop, target, spec, lone, loc, rect=None, fill=-1, misalign=0, guard=64):
    """k_rgb_pack444's lanes over one job on the CPU.  The frame starts `misalign` samples behind a 16-byte boundary and has `guard` bytes of 0xA5
    before and behind it, which must stay."""
    src = np.ascontiguousarray(src)
    sz = api.RGB_SAMPLE_BYTES[spec.dtype]
    out_n = 3 * target[0] * target[1] * sz
    raw = np.full(out_n + 2 * guard + 16 + misalign * sz, 0xA5, np.uint8)
    off = guard + (-(raw.ctypes.data + guard)) % 16 + misalign * sz
    coefs = (C.c_int * 5)(*api.color_coefs(spec.matrix, spec.range == 2))
    scale, bias = (C.c_float * 3)(*spec.scale), (C.c_float * 3)(*spec.bias)
    rc = lib.chroma_rgb_frame(src.ctypes.data, pitch, pitch * hs, lone, *crop, *target, coefs, int(spec.range == 2), spec.dtype, spec.planar, spec.bgr,
                              scale, bias, (C.c_int * 4)(*(rect or (0, 0, 0, 0))), max(fill, 0), loc, raw.ctypes.data + off)
    assert rc == 0, rc
    assert (raw[:off] == 0xA5).all() and (raw[off + out_n:] == 0xA5).all(), "bytes outside the frame were written"
    return raw[off:off + out_n].tobytes()


def test_chroma_packed_walk_equals_the_restatement(lib):
    """Every tile of every one of the device test's cases, 256 lanes per tile in the kernel's order, byte for byte against C(G')."""
    seen = set()
    for case in chroma_device_cases():
        n, spec, W, H, crop, target, rect, fill, loc, pitch, lone, hs, src = case
        got = chroma_walk(lib, src, pitch, hs, crop, target, spec, lone, loc, rect, fill)
        assert got == case_want(*case[1:]), describe(*case)
        seen.add((spec.dtype, loc))
        seen.add(("lone", lone))
        seen.add(("layout", spec.planar, spec.bgr))
    assert len(seen) == 24 + 3 + 4                          # every sample type at every location, the three field modes, the four layouts


@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
def test_chroma_packed_walk_with_a_misaligned_destination(lib, dtype):
    """A frame that starts one sample behind a 16-byte boundary: store4's scalar tails, unplaced and placed."""
    rng = np.random.default_rng(0xA12 + dtype)
    W, H, pitch = 70, 22, 72
    src = rng.integers(0, 256, pitch * H * 3 // 2, dtype=np.uint8)
    for planar in (1, 0):
        for crop, target, rect in (((0, 0, W, H), (W, H), None), ((2, 2, 66, 18), (50, 26), None), ((0, 0, W, H), (98, 30), (10, 4, 70, 22))):
            spec = api.rgb_spec(dtype, planar, 0, 1, 1, **({} if dtype == 0 else IMAGENET))
            got = chroma_walk(lib, src, pitch, H, crop, target, spec, 0, 2 + planar, rect, 0x0A0B0C, misalign=1)
            want = rgb_chroma_frame(_packout_ref(src, pitch, H, W, H, 0, 1), W, H, crop, target, spec, 1, False, 2 + planar, rect, (10, 11, 12))
            assert got == want, (dtype, planar, crop, target, rect)


def test_chroma_packed_asan_builds_and_runs_clean(tmp_path):
    """tools/chroma_packed_asan.cpp: the walk over edge geometries under AddressSanitizer / UBSan, every buffer and every tap table of the exact size."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc: the program is built with its clang")
    out = tmp_path / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "chroma_packed_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(out / "chroma_packed_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ok: 288 walks" in r.stdout
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]


# ---- the chroma sample location of both parsers (parse-only handles) ---------------------------------------------------------------
KEYS = ("vui_chroma_loc", "vui_chroma_loc_bottom", "chroma_loc", "rgb_chroma", "rgb_chroma_frames", "rgb_frames", "out_frame_bytes", "vui_matrix", "fps_num")


def _parse(data, codec=0, rgb=None, **opts):
    o = {"parse_only": 1}
    o.update(opts)
    with api.JmAmdDec(codec, 1, options=o, rgb=rgb) as d:
        frames = d.decode_stream(data)
        return [len(f) for f in frames], {k: d.stat(k) for k in KEYS}, api.jm_nvdec_show_dec_info(d.h)


def _h264(w=64, h=48, **kw):
    return streams.generate(width=w, height=h, frames=2, gop=2, mode=1, seed=0xC412, **kw)


def _hevc(w=64, h=48, **kw):
    return streams.generate_hevc(width=w, height=h, frames=2, ctb_log2=5, mode=1, seed=0xC413, **kw)


GEN = {0: _h264, 1: _hevc}
RGB = dict(dtype="u8")


@pytest.mark.parametrize("codec", [0, 1])
def test_vui_chroma_loc_is_kept_and_used(codec):
    for loc in range(6):
        lens, st, text = _parse(GEN[codec](vui_chroma_loc=loc), codec, rgb=RGB, rgb_chroma=1)
        assert (st["vui_chroma_loc"], st["vui_chroma_loc_bottom"], st["chroma_loc"], st["rgb_chroma"]) == (loc, loc, loc, 1)
        assert lens == [3 * 64 * 48] * 2 and f", chroma interpolated (loc {loc})" in text
    _, st, _ = _parse(GEN[codec](vui_chroma_loc=2, vui_fps=25, vui_matrix=1, vui_primaries=1, vui_transfer=1), codec, rgb=RGB, rgb_chroma=1)
    assert (st["vui_chroma_loc"], st["chroma_loc"], st["vui_matrix"]) == (2, 2, 1) and st["fps_num"] > 0       # the fields around it still parse


@pytest.mark.parametrize("codec", [0, 1])
def test_absent_and_out_of_range_locations_fall_to_zero(codec):
    for kw in (dict(), dict(vui_fps=30)):                   # no VUI; a VUI without chroma_loc_info
        _, st, _ = _parse(GEN[codec](**kw), codec, rgb=RGB, rgb_chroma=1)
        assert (st["vui_chroma_loc"], st["vui_chroma_loc_bottom"], st["chroma_loc"]) == (-1, -1, 0)
    _, st, _ = _parse(GEN[codec](vui_chroma_loc=6), codec, rgb=RGB, rgb_chroma=1)
    assert (st["vui_chroma_loc"], st["chroma_loc"]) == (6, 0)


@pytest.mark.parametrize("codec", [0, 1])
def test_forced_location_and_location_without_rgb_chroma(codec):
    _, st, text = _parse(GEN[codec](vui_chroma_loc=2), codec, rgb=RGB, rgb_chroma=1, chroma_loc=5)
    assert (st["vui_chroma_loc"], st["chroma_loc"]) == (2, 5) and "(loc 5)" in text
    _, st, _ = _parse(GEN[codec](vui_chroma_loc=2), codec, rgb=RGB, rgb_chroma=1, chroma_loc=-1)
    assert st["chroma_loc"] == 2
    # chroma_loc without rgb_chroma: accepted, recorded, and the info text is what it was
    lens, st, text = _parse(GEN[codec](vui_chroma_loc=2), codec, rgb=RGB, chroma_loc=4)
    lens0, st0, text0 = _parse(GEN[codec](vui_chroma_loc=2), codec, rgb=RGB)
    assert (st["rgb_chroma"], st["chroma_loc"]) == (0, 4) and lens == lens0 and "chroma interpolated" not in text
    strip = lambda t: [l for l in t.splitlines() if "ime" not in l and "fps" not in l.lower()]
    assert strip(text) == strip(text0)
    lens, st, text = _parse(GEN[codec](vui_chroma_loc=2), codec)                 # a Y'CbCr handle records the location too
    assert (st["vui_chroma_loc"], st["rgb_chroma"]) == (2, 0) and lens == [64 * 48 * 3 // 2] * 2


def test_mjpeg_auto_location_is_one():
    data = open(os.path.join(ROOT, "tests", "golden", "jpeg", "c420_64x48_opt.jpg"), "rb").read()
    with api.JmAmdDec(2, 1, options={"parse_only": 1, "rgb_chroma": 1}, rgb=RGB) as d:
        frames = d.decode_stream(data, chunks=[data])
        assert len(frames) == 1 and (d.stat("vui_chroma_loc"), d.stat("chroma_loc")) == (-1, 1)
    with api.JmAmdDec(2, 1, options={"parse_only": 1, "rgb_chroma": 1, "chroma_loc": 0}, rgb=RGB) as d:
        d.decode_stream(data, chunks=[data])
        assert d.stat("chroma_loc") == 0


def test_truncated_hevc_vui_leaves_the_location_unknown():
    nals = api.split_nalus(_hevc(vui_fps=30, vui_chroma_loc=3, vui_matrix=1, vui_primaries=1, vui_transfer=1))
    sps = [i for i, n in enumerate(nals) if ((n[n.index(b"\x00\x01") + 2] >> 1) & 63) == 33][0]
    nals[sps] = nals[sps][:-6]                              # the SPS ends inside the VUI timing information: valid, its VUI unknown
    lens, st, _ = _parse(b"".join(nals), 1, rgb=RGB, rgb_chroma=1)
    assert len(lens) == 2
    assert (st["vui_chroma_loc"], st["vui_chroma_loc_bottom"], st["vui_matrix"], st["chroma_loc"]) == (-1, -1, -1, 0)


def test_generators_at_the_default_write_the_streams_of_before():
    """vui_chroma_loc -1 (the default) writes chroma_loc_info_present_flag 0 and no VUI of its own: the streams are the ones the generators wrote before
    they knew the parameter (digests recorded from those), and any other value changes the parameter sets only."""
    want = {"h264": "0d2b64604da63704b4754bd8ba02e6a7", "h264_vui": "1c2c8e3c484a84e352e5cef8260da678", "hevc_vui": "82eba43c84f84b202f9237184e15c522"}
    a = streams.generate(width=64, height=48, frames=3, gop=3, mode=1, seed=5)
    b = streams.generate(width=64, height=48, frames=3, gop=3, mode=1, seed=5, vui_fps=30)
    c = streams.generate_hevc(width=64, height=48, frames=2, seed=5, vui_fps=30)
    assert {"h264": hashlib.md5(a).hexdigest(), "h264_vui": hashlib.md5(b).hexdigest(), "hevc_vui": hashlib.md5(c).hexdigest()} == want
    assert a == streams.generate(width=64, height=48, frames=3, gop=3, mode=1, seed=5, vui_chroma_loc=-1)
    assert c == streams.generate_hevc(width=64, height=48, frames=2, seed=5, vui_fps=30, vui_chroma_loc=-1)
    for gen, codec in ((_h264, 0), (_hevc, 1)):
        plain, sited = api.split_nalus(gen()), api.split_nalus(gen(vui_chroma_loc=1))
        kind = (lambda n: (n[n.index(b"\x00\x01") + 2] >> 1) & 63) if codec else (lambda n: n[n.index(b"\x00\x01") + 2] & 31)
        diff = [kind(x) for x, y in zip(plain, sited) if x != y]
        assert len(plain) == len(sited) and diff == [33 if codec else 7]


# ---- validation ----------------------------------------------------------------------------------------------------------------
def test_set_option_ranges_and_set_option_after_init():
    L = api.lib()
    h = api.jm_nvdec_create_handle()
    try:
        for key, good, bad in ((b"rgb_chroma", (0, 1), (-1, 2, 255)), (b"chroma_loc", (-1, 0, 3, 5), (-2, 6, 100))):
            for v in bad:
                assert L.jm_amddec_set_option(h, key, v) == -1, (key, v)
            for v in good:
                assert L.jm_amddec_set_option(h, key, v) == 0, (key, v)
        assert L.jm_amddec_set_option(h, b"rgb_chroma", 1) == 0 and api.set_rgb(h, "u8") == 0
        assert L.jm_amddec_set_option(h, b"parse_only", 1) == 0
        assert api.jm_nvdec_init(0, 1, None, 0, h) == 0
        assert L.jm_amddec_set_option(h, b"rgb_chroma", 0) == -1 and L.jm_amddec_set_option(h, b"chroma_loc", 1) == -1      # after init
        assert L.jm_amddec_get_stat(h, b"rgb_chroma") == 1
    finally:
        api.jm_nvdec_deinit(h)


def test_rgb_chroma_without_a_spec_fails_init_and_names_the_option():
    L = api.lib()
    h = api.jm_nvdec_create_handle()
    try:
        assert L.jm_amddec_set_option(h, b"parse_only", 1) == 0 and L.jm_amddec_set_option(h, b"rgb_chroma", 1) == 0
        assert api.jm_nvdec_init(0, 1, None, 0, h) != 0
        assert b"rgb_chroma" in L.jm_amddec_last_error(h)
    finally:
        api.jm_nvdec_deinit(h)
    with pytest.raises(RuntimeError, match="rgb_chroma"):
        api.JmAmdDec(0, 1, options={"parse_only": 1, "rgb_chroma": 1})
    with api.JmAmdDec(0, 1, options={"parse_only": 1, "chroma_loc": 3}) as d:               # chroma_loc alone needs no spec
        assert d.stat("rgb_chroma") == 0


def test_rgb_chroma_device_refuses_bad_arguments():
    # (refused before anything touches the device: the addresses are never dereferenced)
    s = api.rgb_spec("u8", matrix=1)
    args = (1 << 20, 128, 128 * 64, 64, 64, (0, 0, 64, 64), (64, 64), s, 1 << 21)
    assert api.rgb_chroma_device(*args, 6) == -1 and api.rgb_chroma_device(*args, -1) == -1
    assert api.rgb_chroma_device(1 << 20, 128, 128 * 64, 64, 64, (0, 0, 64, 64), (6, 64), s, 1 << 21, 0) == -1            # beyond 8:1
    assert api.rgb_chroma_device(1 << 20, 128, 128 * 64, 64, 64, (0, 0, 64, 64), (64, 64), api.rgb_spec("u8", matrix=0), 1 << 21, 0) == -1
    assert api.rgb_chroma_device(1 << 20, 128, 128 * 64, 64, 64, (0, 0, 64, 64), (64, 64), api.rgb_spec("f32", matrix=1), (1 << 21) + 2, 0) == -1
    assert api.rgb_chroma_device(*args, 0, rect=(0, 0, 66, 64)) == -1                                                        # outside the target


# ---- old behaviour ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [0, 1])
def test_rgb_chroma_zero_is_a_handle_that_never_heard_of_the_option(codec):
    """Parse-only: the same frames, frame bytes, statistics and info text (the pixels: test_rgb_chroma_gpu.py)."""
    data = GEN[codec](vui_chroma_loc=3)
    a = _parse(data, codec, rgb=dict(dtype="f16"), crop_x=8, crop_w=32, target_width=16, target_height=24)
    b = _parse(data, codec, rgb=dict(dtype="f16"), crop_x=8, crop_w=32, target_width=16, target_height=24, rgb_chroma=0)
    strip = lambda t: [l for l in t.splitlines() if "ime" not in l and "fps" not in l.lower()]
    assert a[0] == b[0] and a[1] == b[1] and strip(a[2]) == strip(b[2])
    assert a[1]["rgb_chroma_frames"] == 0
    c = _parse(data, codec, rgb=dict(dtype="f16"), crop_x=8, crop_w=32, target_width=16, target_height=24, rgb_chroma=1)
    assert c[0] == a[0] and c[1]["rgb_chroma_frames"] == 0           # (parse-only frames carry no pixels: nothing is converted)
