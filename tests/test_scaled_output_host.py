"""Scaled and cropped output, host side (no GPU): the tap builder against a numpy restatement of the resampler R_G (INTEGRATION.md
"Scaled and cropped output"), the closed forms R_G must satisfy, the lane routines of k_scale_pack (jmcodec_amd/csrc/scale_packed.h) walked over
whole frames on the CPU, and the geometry options of parse-only handles.  The restatement and the case list here are what the GPU tests
(test_scaled_output_gpu.py) compare the device output with."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from jmcodec_amd import api
from tools import streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- R_G restated ---------------------------------------------------------------------------------------------------------
def taps_ref(S, D):
    """Per output j: (first source index, [weights]) of one axis, S source samples -> D outputs."""
    out = []
    for j in range(D):
        if D >= S:                                                   # bilinear, half-sample centres
            num = (2 * j + 1) * S - D
            i0 = num // (2 * D)
            w1 = ((num - 2 * D * i0) * 16384 + D) // (2 * D)
            out.append((i0, [16384 - w1, w1]))
        else:                                                        # area average
            lo, hi = j * S // D, -(-(j + 1) * S // D)
            a = [min((i + 1) * D, (j + 1) * S) - max(i * D, j * S) for i in range(lo, hi)]
            w = [x * 16384 // S for x in a]
            w[a.index(max(a))] += 16384 - sum(w)
            out.append((lo, w))
    return out


def _gather(S, D):
    """(idx, wt): D x T arrays of clamped source indices and weights (missing taps weigh 0)."""
    t = taps_ref(S, D)
    T = max(len(w) for _, w in t)
    idx = np.zeros((D, T), np.int64)
    wt = np.zeros((D, T), np.int64)
    for j, (f, w) in enumerate(t):
        for k in range(T):
            idx[j, k] = min(max(f + k, 0), S - 1)
            wt[j, k] = w[k] if k < len(w) else 0
    return idx, wt


def resample_plane(p, tw, th):
    """R_G of one plane (the crop already cut out): horizontal pass, int16-range intermediate, vertical pass."""
    p = p.astype(np.int64)
    ch, cw = p.shape
    ix, wx = _gather(cw, tw)
    iy, wy = _gather(ch, th)
    h = np.zeros((ch, tw), np.int64)
    for k in range(ix.shape[1]):
        h += wx[:, k][None, :] * p[:, ix[:, k]]
    h = (h + 64) >> 7
    assert h.max(initial=0) <= 32640
    o = np.zeros((th, tw), np.int64)
    for k in range(iy.shape[1]):
        o += wy[:, k][:, None] * h[iy[:, k], :]
    return np.minimum(255, (o + (1 << 20)) >> 21).astype(np.uint8)


def split_frame(F, W, H, fmt):
    F = np.frombuffer(F, np.uint8) if isinstance(F, (bytes, bytearray)) else F
    Y = F[:W * H].reshape(H, W)
    if fmt == 1:
        U = F[W * H:W * H + W * H // 4].reshape(H // 2, W // 2)
        V = F[W * H + W * H // 4:W * H * 3 // 2].reshape(H // 2, W // 2)
    else:
        uv = F[W * H:W * H * 3 // 2].reshape(H // 2, W // 2, 2)
        U, V = uv[:, :, 0], uv[:, :, 1]
    return Y, U, V


def join_frame(Y, U, V, fmt):
    if fmt == 1:
        return Y.tobytes() + U.tobytes() + V.tobytes()
    return Y.tobytes() + np.stack([U, V], axis=2).tobytes()


def scale_frame(F, W, H, fmt, crop, target):
    """R_G(F): F a tight frame (NV12 fmt 0 / I420 fmt 1) of W x H; crop (x, y, w, h), target (tw, th).  Chroma planes are planes of their own
    on the half-resolution grid (no chroma siting shift)."""
    x, y, cw, ch = crop
    tw, th = target
    Y, U, V = split_frame(F, W, H, fmt)
    Yo = resample_plane(Y[y:y + ch, x:x + cw], tw, th)
    Uo = resample_plane(U[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2], tw // 2, th // 2)
    Vo = resample_plane(V[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2], tw // 2, th // 2)
    return join_frame(Yo, Uo, Vo, fmt)


def scale_frames(blob, n, W, H, fmt, crop, target):
    fs = W * H * 3 // 2
    return [scale_frame(blob[i * fs:(i + 1) * fs], W, H, fmt, crop, target) for i in range(n)]


# ---- the cases of the stand-alone kernel tests (CPU walk here, the device in test_scaled_output_gpu.py) ---------------------------------
def _packout_ref(src, pitch, hs, w, h, lone, fmt):
    """The frame F k_packout makes of a pitch-linear NV12 surface of hs rows (lone-field row mapping included)."""
    rows = np.arange(h)
    rows_c = np.arange(h // 2)
    if lone:
        rows, rows_c = (rows & ~1) | (lone - 1), (rows_c & ~1) | (lone - 1)
    Y = src[:pitch * hs].reshape(hs, pitch)[rows, :w]
    uv = src[pitch * hs:pitch * hs + pitch * (hs // 2)].reshape(hs // 2, pitch)[rows_c, :w]
    U, V = uv[:, 0::2], uv[:, 1::2]
    return Y.tobytes() + (np.stack([U, V], 2).tobytes() if fmt == 0 else U.tobytes() + V.tobytes())


def _random_geometry(rng, limit=None):
    W = rng.randrange(2, 400, 2)
    H = rng.randrange(2, 300, 2)
    cw = rng.randrange(2, W + 1, 2)
    ch = rng.randrange(2, H + 1, 2)
    cx = rng.randrange(0, W - cw + 1, 2)
    cy = rng.randrange(0, H - ch + 1, 2)

    def dst(s):
        lo, hi = -(-s // 8), 4 * s
        lo += lo & 1
        if limit == "down":
            return lo
        if limit == "up":
            return hi
        return rng.randrange(lo, hi + 1, 2)
    return W, H, (cx, cy, cw, ch), (dst(cw), dst(ch))


def scale_device_cases():
    """240 seeded random geometries (sizes that are no multiples of 16, both formats, lone_field 0 / 1 / 2, the ratio limits 8:1 and 1:4) and two
    fixed ones; yields (n, W, H, crop, target, pitch, lone, fmt, hs, src): src a surface of hs rows (the coded height) at the given pitch."""
    rng = random.Random(0x5CA1ED)
    cases = [_random_geometry(rng) for _ in range(200)] + [_random_geometry(rng, "down") for _ in range(20)] + \
            [_random_geometry(rng, "up") for _ in range(20)]
    cases.append((1920, 1080, (0, 0, 1920, 1080), (240, 136)))
    cases.append((180, 100, (0, 0, 180, 100), (720, 400)))
    for n, (W, H, crop, target) in enumerate(cases):
        pitch = W + rng.choice([0, 2, 14, 128 - W % 128])
        lone, fmt = n % 3, (n // 3) % 2
        # surface rows (the coded height): a lone field of a frame with an odd number of chroma rows reads the surface's next one
        hs = H + (16 if lone and H % 4 else rng.choice([0, 16]))
        src = np.random.default_rng(n).integers(0, 256, pitch * hs * 3 // 2, dtype=np.uint8)
        yield n, W, H, crop, target, pitch, lone, fmt, hs, src


# ---- scale_packed.h: k_scale_pack's lanes on the CPU ------------------------------------------------------------------------------------
def build_native(name, compiler, hdrs, walks=("scale_packed_walk.h",)):
    """tests/native/<name>.cpp as a shared library under tests/_build (rebuilt when the source or one of the headers is newer)."""
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, f"lib{name}.so")
    src = os.path.join(ROOT, "tests", "native", name + ".cpp")
    deps = [src] + [os.path.join(ROOT, "tests", "native", h) for h in walks] + [os.path.join(ROOT, "jmcodec_amd", "csrc", h) for h in hdrs]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(compiler + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so, src])
    return C.CDLL(so)


def load_scale_check():
    l = build_native("scale_packed_check", ["g++"], ("scale_packed.h", "mc_packed.h", "jobs.h"))
    l.scl_frame.argtypes = [C.c_void_p] + [C.c_int] * 10 + [C.c_void_p]
    return l


@pytest.fixture(scope="module")
def lib():
    return load_scale_check()


def scale_walk(lib, src, pitch, hs, crop, target, fmt, lone, guard=64):
    """k_scale_pack's lanes over one job on the CPU.  The surface is a heap copy of exactly its size; the frame has `guard` bytes of 0xA5 behind it,
    which must stay."""
    src = np.ascontiguousarray(src)
    out_n = target[0] * target[1] * 3 // 2
    out = np.full(out_n + guard, 0xA5, np.uint8)
    rc = lib.scl_frame(src.ctypes.data, pitch, pitch * hs, lone, *crop, *target, fmt, out.ctypes.data)
    assert rc == 0, rc
    assert (out[out_n:] == 0xA5).all(), "bytes behind the frame were written"
    return out[:out_n].tobytes()


def test_scale_packed_walk_equals_the_restatement(lib):
    """Every tile of every one of the device test's 242 cases, 256 lanes per tile, horizontal pass then vertical pass, byte for byte against R_G of
    the k_packout restatement: tile edges, the clamp of the row range, the I420 lane mapping and the tail stores run here without a GPU."""
    count = 0
    for n, W, H, crop, target, pitch, lone, fmt, hs, src in scale_device_cases():
        got = scale_walk(lib, src, pitch, hs, crop, target, fmt, lone)
        want = scale_frame(_packout_ref(src, pitch, hs, W, H, lone, fmt), W, H, fmt, crop, target)
        assert got == want, f"case {n}: {W}x{H} crop {crop} -> {target} lone {lone} fmt {fmt}"
        count += 1
    assert count == 242


# ---- the library's tap builder ---------------------------------------------------------------------------------------------
def _sweep():
    rng = random.Random(0x5CA1E)
    sizes = [2, 4, 6, 10, 18, 30, 34, 90, 126, 144, 176, 270, 360, 540, 720, 1080, 1918, 1920, 2160, 3840]
    pairs = set()
    for S in sizes:
        for D in {max(1, -(-S // 8)), S // 8, S // 3, S // 2, S - 2, S, S + 2, 2 * S, 3 * S - 1, 4 * S}:
            if D >= 1 and S <= 8 * D <= 32 * S:
                pairs.add((S, D))
        for _ in range(6):
            pairs.add((S, rng.randint(max(1, -(-S // 8)), 4 * S)))
    for _ in range(300):
        S = rng.randint(1, 4000)
        pairs.add((S, rng.randint(max(1, -(-S // 8)), 4 * S)))
    return sorted(pairs)


def test_scale_taps_equal_the_restatement():
    pairs = _sweep()
    assert len(pairs) > 400 and (1080, 135) in pairs and (540, 2160) in pairs
    for S, D in pairs:
        got = api.scale_taps(S, D)
        assert got is not None, (S, D)
        first, weights = got
        want = taps_ref(S, D)
        T = len(weights[0])
        assert T == max(len(w) for _, w in want) <= 9, (S, D)
        for j, (f, w) in enumerate(want):
            assert first[j] == f, (S, D, j)
            assert weights[j] == w + [0] * (T - len(w)), (S, D, j)
            assert min(weights[j]) >= 0 and sum(weights[j]) == 16384, (S, D, j)


def test_scale_taps_refuse_ratios_beyond_the_limits():
    assert api.scale_taps(800, 100) is not None and api.scale_taps(801, 100) is None          # 8:1 down
    assert api.scale_taps(100, 400) is not None and api.scale_taps(100, 401) is None          # 1:4 up
    assert api.scale_taps(0, 4) is None and api.scale_taps(4, 0) is None
    assert api.lib().jm_amddec_scale_taps(1080, 135, None, None, 0) == 8                      # a table query without buffers: exactly 8:1
    assert api.lib().jm_amddec_scale_taps(1078, 135, None, None, 0) == 9                      # ... not a whole ratio: one tap more
    assert api.scale_taps(1078, 135, max_taps=8) is None                                      # too few taps per output for it


# ---- closed forms of R_G ---------------------------------------------------------------------------------------------------
def test_identity_geometry_returns_the_input():
    rng = np.random.default_rng(1)
    for W, H in ((18, 10), (90, 70), (176, 144)):
        F = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8).tobytes()
        for fmt in (0, 1):
            assert scale_frame(F, W, H, fmt, (0, 0, W, H), (W, H)) == F


def test_exact_2x_downscale_is_the_rounded_block_mean():
    rng = np.random.default_rng(2)
    p = rng.integers(0, 256, (38, 58), dtype=np.uint8)
    q = p.astype(np.int32)
    want = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2
    assert np.array_equal(resample_plane(p, 29, 19), want)


def test_a_flat_field_stays_flat():
    for v in (0, 1, 16, 128, 235, 254, 255):
        for (cw, ch), (tw, th) in (((90, 70), (12, 10)), ((90, 70), (360, 280)), ((34, 18), (30, 20)), ((200, 8), (26, 32))):
            assert (resample_plane(np.full((ch, cw), v, np.uint8), tw, th) == v).all()


def test_restatement_is_the_identity_when_target_equals_crop():
    rng = np.random.default_rng(3)
    p = rng.integers(0, 256, (22, 34), dtype=np.uint8)
    assert np.array_equal(resample_plane(p, 34, 22), p)


# ---- geometry options of parse-only handles ----------------------------------------------------------------------------------
def _parse_only(data, codec=0, **geo):
    """Decode with a parse-only handle and the given geometry; returns (stream_info, frame lengths, stats, last_error, info)."""
    opts = {"parse_only": 1}
    opts.update(geo)
    with api.JmAmdDec(codec, 1, options=opts) as d:
        try:
            frames = d.decode_stream(data)
        except RuntimeError:
            frames = None
        info = api.jm_nvdec_stream_info(d.h)
        err = api.lib().jm_amddec_last_error(d.h).decode()
        stats = {k: d.stat(k) for k in ("out_width", "out_height", "scaled_frames", "frames")}
        text = api.jm_nvdec_show_dec_info(d.h)
    return info, None if frames is None else [len(f) for f in frames], stats, err, text


def _h264():
    return streams.generate(width=176, height=144, frames=4, gop=4, mode=1, seed=0x5CA1)


def _hevc():
    return streams.generate_hevc(width=90, height=70, frames=3, ctb_log2=5, mode=1, seed=6)


def test_stream_info_reports_the_target_h264():
    info, lens, stats, err, text = _parse_only(_h264(), target_width=96, target_height=54)
    assert info == (96, 54) and lens == [96 * 54 * 3 // 2] * 4, err
    assert (stats["out_width"], stats["out_height"]) == (96, 54)
    assert "Display:\t96 x 54" in text
    # a crop alone: the target is the crop size
    info, lens, _, err, _ = _parse_only(_h264(), crop_x=16, crop_y=8, crop_w=64, crop_h=48)
    assert info == (64, 48) and lens == [64 * 48 * 3 // 2] * 4, err
    # crop_w / crop_h 0: up to the display area's edge
    info, _, _, err, _ = _parse_only(_h264(), crop_x=16, crop_y=8)
    assert info == (160, 136), err


def test_stream_info_reports_the_target_hevc():
    info, lens, stats, err, _ = _parse_only(_hevc(), codec=1, crop_x=2, crop_y=4, crop_w=80, crop_h=60, target_width=40, target_height=30)
    assert info == (40, 30) and lens == [40 * 30 * 3 // 2] * 3, err
    assert (stats["out_width"], stats["out_height"]) == (40, 30)


def test_without_options_nothing_changes():
    info, lens, stats, _, text = _parse_only(_h264())
    assert info == (176, 144) and lens == [176 * 144 * 3 // 2] * 4
    assert (stats["out_width"], stats["out_height"], stats["scaled_frames"]) == (176, 144, 0)
    assert "Display:\t176 x 144" in text
    info, _, _, _, _ = _parse_only(_hevc(), codec=1)
    assert info == (90, 70)
    # the identity geometry spelled out is no geometry
    info, lens, stats, _, _ = _parse_only(_h264(), crop_w=176, crop_h=144, target_width=176, target_height=144)
    assert info == (176, 144) and stats["scaled_frames"] == 0


@pytest.mark.parametrize("geo,words", [
    (dict(crop_x=160, crop_w=32), "crop rectangle"),                       # 160 + 32 > 176
    (dict(crop_y=144), "crop rectangle"),                                   # nothing left below y = 144
    (dict(crop_h=160), "crop rectangle"),
    (dict(target_width=20), "scaling ratio"),                               # 176 -> 20: beyond 8:1
    (dict(target_height=578), "scaling ratio"),                             # 144 -> 578: beyond 1:4
    (dict(crop_w=16, crop_h=16, target_width=66), "scaling ratio"),
])
def test_invalid_geometry_fails_with_a_reason(geo, words):
    info, lens, _, err, _ = _parse_only(_h264(), **geo)
    assert words in err and "output geometry" in err, err


def test_invalid_geometry_fails_hevc():
    _, _, _, err, _ = _parse_only(_hevc(), codec=1, crop_x=50, crop_w=50)
    assert "crop rectangle" in err


def test_geometry_options_are_even_and_before_init_only():
    L = api.lib()
    h = api.jm_nvdec_create_handle()
    try:
        for k in ("crop_x", "crop_y", "crop_w", "crop_h", "target_width", "target_height"):
            assert L.jm_amddec_set_option(h, k.encode(), 3) == -1
            assert L.jm_amddec_set_option(h, k.encode(), -2) == -1
            assert L.jm_amddec_set_option(h, k.encode(), 64) == 0
        assert L.jm_amddec_set_option(h, b"parse_only", 1) == 0
        assert api.jm_nvdec_init(0, 1, None, 0, h) == 0
        for k in ("crop_x", "crop_y", "crop_w", "crop_h", "target_width", "target_height"):
            assert L.jm_amddec_set_option(h, k.encode(), 64) == -1
    finally:
        api.jm_nvdec_deinit(h)
