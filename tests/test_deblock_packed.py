"""The H.264 edge filters as the deblocking kernels run them (jmcodec_amd/csrc/deblock_packed.h: flt_luma on packed 16-bit pairs with sign masks and bit
blends, the branch-free flt_chroma, and the scalar filter_luma / filter_chroma of k_deblock) against a literal, clause-ordered restatement of 8.7.2.2,
8.7.2.3 and 8.7.2.4, on the CPU: the header restates v_sad_u8, v_alignbit_b32, the packed 16-bit arithmetic and the one-lane ballot in plain C++ for host
builds.  Both sides are compiled from tests/native/deblock_packed_check.cpp; the lines, and alpha / beta / tC0, come from here and from
tests/spec_tables_h264.py.

The sweep: bS 0..4 x every (indexA, indexB) in 0..51 x lines of three kinds -- random octets, octets whose differences sit on the thresholds of the clause
(alpha, beta, (alpha >> 2) + 2, each at -1 / 0 / +1, near sample values 0 and 255), and octets aimed at a delta of +-tC and +-(tC + 1).  The restatement counts
the paths it took; every one of them must have been taken by the sweep itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from spec_tables_h264 import ALPHA, BETA, TC0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LUMA_COUNTERS = ["on_bS1", "on_bS2", "on_bS3", "on_bS4", "off_alpha_only", "off_beta_p_only", "off_beta_q_only", "ap0_aq0", "ap0_aq1", "ap1_aq0", "ap1_aq1",
                 "delta_clipped_at_plus_tC", "delta_clipped_at_minus_tC", "delta_unclipped", "delta_is_plus_tC", "delta_is_minus_tC", "delta_is_tC_plus_1",
                 "delta_is_minus_tC_minus_1", "clip1_at_0", "clip1_at_255", "sum_is_0", "sum_is_255", "strong_both", "strong_p_only", "strong_q_only",
                 "strong_neither", "bS0", "p1_term_clipped", "p1_term_unclipped"]
CHROMA_COUNTERS = ["bS_lt4_filtered", "bS_lt4_not_filtered", "bS4_filtered", "bS4_not_filtered", "delta_clipped_at_plus_tC", "delta_clipped_at_minus_tC",
                   "delta_unclipped", "clip1_at_0", "clip1_at_255", "bS0"]


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libdeblock_packed_check.so")
    src = os.path.join(ROOT, "tests", "native", "deblock_packed_check.cpp")
    hdr = os.path.join(ROOT, "jmcodec_amd", "csrc", "deblock_packed.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so, src])
    l = ctypes.CDLL(so)
    assert l.dbp_luma_counters() == len(LUMA_COUNTERS) and l.dbp_chroma_counters() == len(CHROMA_COUNTERS)
    return l


def _ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return ctypes.c_void_p(a.ctypes.data)


def _place(rng, base, mag):
    """base +- mag with a random sign; the other sign where the first leaves 0..255, clipped where both do"""
    sign = rng.choice(np.array([-1, 1]), size=base.shape)
    v = base + sign * mag
    w = base - sign * mag
    v = np.where((v < 0) | (v > 255), w, v)
    return np.clip(v, 0, 255)


def _pick(rng, options):
    """per line, one of the option arrays"""
    o = np.stack(options)
    return o[rng.integers(0, len(options), size=o.shape[1]), np.arange(o.shape[1])]


def sweep_lines(seed, per_kind):
    """-> bS, alpha, beta, tc0 rows (n, 3), lines (n, 8) = p3 p2 p1 p0 q0 q1 q2 q3 -- for every bS 0..4 and every (indexA, indexB), 3 * per_kind lines"""
    rng = np.random.default_rng(seed)
    ia, ib, bs = np.meshgrid(np.arange(52), np.arange(52), np.arange(5), indexing="ij")
    ia, ib, bs = (np.repeat(v.reshape(-1), 3 * per_kind) for v in (ia, ib, bs))
    n = ia.size
    alpha, beta = np.array(ALPHA)[ia], np.array(BETA)[ib]
    tc0row = np.array(TC0, dtype=np.int64)[ia]
    tc0 = np.where((bs >= 1) & (bs <= 3), tc0row[np.arange(n), np.clip(bs - 1, 0, 2)], 0)
    kind = np.tile(np.repeat(np.arange(3), per_kind), n // (3 * per_kind))
    rnd = lambda lo, hi: rng.integers(lo, hi, size=n)          # noqa: E731
    # ---- kind 1: on the thresholds ----
    p0 = _pick(rng, [np.full(n, 0), np.full(n, 1), np.full(n, 2), np.full(n, 128), np.full(n, 253), np.full(n, 254), np.full(n, 255), rnd(0, 256), rnd(0, 256)])
    strong = (alpha >> 2) + 2
    dq = _pick(rng, [alpha - 1, alpha, alpha + 1, strong - 1, strong, strong + 1, np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64),
                     rnd(0, 256) % (alpha + 1), rnd(0, 256) % (strong + 1)])
    q0 = _place(rng, p0, np.maximum(dq, 0))
    around_beta = lambda: np.maximum(_pick(rng, [beta - 1, beta, beta + 1, beta - 1, np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64),      # noqa: E731
                                                 rnd(0, 256) % (beta + 1), rnd(0, 256) % (beta + 1)]), 0)
    p1, q1, p2, q2 = _place(rng, p0, around_beta()), _place(rng, q0, around_beta()), _place(rng, p0, around_beta()), _place(rng, q0, around_beta())
    thr = np.stack([rnd(0, 256), p2, p1, p0, q0, q1, q2, rnd(0, 256)], axis=1)
    # ---- kind 2: ((q0 - p0) << 2) + (p1 - q1) + 4 = 8 t + r, for t = +-tC, +-(tC + 1) and r = 0 or 7 (the two ends of the >> 3 bucket) ----
    tc = tc0 + rng.integers(0, 3, size=n)                     # luma: tC0 + 0, 1 or 2; chroma reads tC0 + 1 from the same lines
    t = _pick(rng, [tc, -tc, tc + 1, -(tc + 1)])
    r = rng.choice(np.array([0, 7]), size=n)
    d = _pick(rng, [t, 2 * t, t + (t >> 1)])                  # q0 - p0
    e = 8 * t + r - 4 - 4 * d                                 # p1 - q1
    a = (e + d) >> 1                                          # p1 - p0 and q1 - q0 share the rest as evenly as they can
    b = a - (e + d)
    c0 = _pick(rng, [np.full(n, 128), rnd(70, 186), np.full(n, 0), np.full(n, 255), np.full(n, 3), np.full(n, 252)])
    c0 = np.clip(c0, np.maximum(0, np.maximum(-a, np.maximum(-d, -(d + b)))), 255 - np.maximum(0, np.maximum(a, np.maximum(d, d + b))))
    tp0, tq0 = c0, c0 + d
    tp1, tq1 = tp0 + a, tq0 + b
    tp2, tq2 = _place(rng, tp0, around_beta()), _place(rng, tq0, around_beta())
    aim = np.clip(np.stack([rnd(0, 256), tp2, tp1, tp0, tq0, tq1, tq2, rnd(0, 256)], axis=1), 0, 255)
    # ---- kind 0: random octets, half of them smooth (a level + noise of a few steps) so that they pass the tests often ----
    noise = rng.integers(0, 256, size=(n, 8))
    amp = _pick(rng, [np.full(n, 2), np.full(n, 5), np.full(n, 12), np.full(n, 40)])
    smooth = np.clip(rnd(0, 256)[:, None] + (noise % (2 * amp[:, None] + 1)) - amp[:, None], 0, 255)
    rand = np.where((rng.integers(0, 2, size=n) == 1)[:, None], smooth, rng.integers(0, 256, size=(n, 8)))
    lines = np.where((kind == 0)[:, None], rand, np.where((kind == 1)[:, None], thr, aim))
    u8 = lambda v: np.ascontiguousarray(v, dtype=np.uint8)      # noqa: E731
    return u8(bs), u8(alpha), u8(beta), u8(tc0row), u8(lines)


@pytest.fixture(scope="module")
def sweep():
    return sweep_lines(0x4A4D0870, 40)


def _first_mismatch(name, want, got, lines, bs, alpha, beta, tc0row):
    bad = np.nonzero((want != got).any(axis=1))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return "%s: %d of %d lines differ; first: line %s bS %d alpha %d beta %d tC0 %s -> %s, the clause gives %s" % (
        name, bad.size, len(lines), lines[i].tolist(), bs[i], alpha[i], beta[i], tc0row[i].tolist(), got[i].tolist(), want[i].tolist())


def test_luma_filters_equal_the_clause_on_every_path(lib, sweep):
    bs, alpha, beta, tc0row, lines = sweep
    n = len(lines)
    assert n == 5 * 52 * 52 * 120
    want, packed, scalar = np.zeros_like(lines), np.zeros_like(lines), np.zeros_like(lines)
    cnt = np.zeros(len(LUMA_COUNTERS), dtype=np.uint64)
    lib.dbp_luma_literal(n, _ptr(lines), _ptr(bs), _ptr(alpha), _ptr(beta), _ptr(tc0row), _ptr(want), _ptr(cnt))
    lib.dbp_luma_packed(n, _ptr(lines), _ptr(bs), _ptr(alpha), _ptr(beta), _ptr(tc0row), _ptr(packed))
    lib.dbp_luma_scalar(n, _ptr(lines), _ptr(bs), _ptr(alpha), _ptr(beta), _ptr(tc0row), _ptr(scalar))
    counts = dict(zip(LUMA_COUNTERS, (int(v) for v in cnt)))
    print("luma paths:", counts)
    assert _first_mismatch("flt_luma (packed)", want, packed, lines, bs, alpha, beta, tc0row) is None
    assert _first_mismatch("filter_luma (scalar)", want, scalar, lines, bs, alpha, beta, tc0row) is None
    # the kernels store single bytes of the packed halves: no half may leave 0..255
    assert lib.dbp_luma_packed_out_of_range(n, _ptr(lines), _ptr(bs), _ptr(alpha), _ptr(beta), _ptr(tc0row)) == 0
    assert (want != lines).any(axis=1).sum() > n // 20                      # the sweep filters: it is not a test of the identity
    missed = [k for k, v in counts.items() if v == 0]
    assert not missed, "paths of 8.7.2.3 / 8.7.2.4 the sweep never took: %s" % missed


def test_chroma_filters_equal_the_clause_on_every_path(lib, sweep):
    bs, alpha, beta, tc0row, lines8 = sweep
    lines = np.ascontiguousarray(lines8[:, 2:6])                              # p1 p0 q0 q1
    n = len(lines)
    want, packed, scalar = np.zeros_like(lines), np.zeros_like(lines), np.zeros_like(lines)
    cnt = np.zeros(len(CHROMA_COUNTERS), dtype=np.uint64)
    lib.dbp_chroma_literal(n, _ptr(lines), _ptr(bs), _ptr(alpha), _ptr(beta), _ptr(tc0row), _ptr(want), _ptr(cnt))
    lib.dbp_chroma_packed(n, _ptr(lines), _ptr(bs), _ptr(alpha), _ptr(beta), _ptr(tc0row), _ptr(packed))
    lib.dbp_chroma_scalar(n, _ptr(lines), _ptr(bs), _ptr(alpha), _ptr(beta), _ptr(tc0row), _ptr(scalar))
    counts = dict(zip(CHROMA_COUNTERS, (int(v) for v in cnt)))
    print("chroma paths:", counts)
    assert _first_mismatch("flt_chroma (branch-free)", want, packed, lines, bs, alpha, beta, tc0row) is None
    assert _first_mismatch("filter_chroma (scalar)", want, scalar, lines, bs, alpha, beta, tc0row) is None
    assert (want != lines).any(axis=1).sum() > n // 20
    missed = [k for k, v in counts.items() if v == 0]
    assert not missed, "paths of the chroma filter the sweep never took: %s" % missed


def test_the_literal_filter_on_lines_worked_by_hand(lib):
    """Four lines whose answers are worked out here from the equations, so that the restatement the sweep trusts is itself pinned to something typed."""
    def run(line, bS, ia, ib):
        a = np.array([line], dtype=np.uint8)
        out = np.zeros_like(a)
        cnt = np.zeros(len(LUMA_COUNTERS), dtype=np.uint64)
        args = [np.array([v], dtype=np.uint8) for v in (bS, ALPHA[ia], BETA[ib])] + [np.array([TC0[ia]], dtype=np.uint8)]      # kept alive over the call
        lib.dbp_luma_literal(1, _ptr(a), *[_ptr(v) for v in args], _ptr(out), _ptr(cnt))
        return out[0].tolist()
    # indexA = indexB = 36: alpha 50, beta 11, tC0 (2, 3, 4)
    assert (ALPHA[36], BETA[36], TC0[36]) == (50, 11, (2, 3, 4))
    # bS 2: ap = |100 - 104| = 4 < 11, aq = |120 - 112| = 8 < 11 -> tC = 3 + 2 = 5; raw = ((112 - 104) * 4 + (102 - 116) + 4) >> 3 = 22 >> 3 = 2 -> delta 2
    # p1' = 102 + Clip3(-3, 3, (100 + 108 - 204) >> 1 = 2) = 104; q1' = 116 + Clip3(-3, 3, (120 + 108 - 232) >> 1 = -2) = 114
    assert run([90, 100, 102, 104, 112, 116, 120, 130], 2, 36, 36) == [90, 100, 104, 106, 110, 114, 120, 130]
    # bS 1, delta clipped: raw = ((130 - 104) * 4 + (104 - 130) + 4) >> 3 = 82 >> 3 = 10 > tC = 2 + 1 + 1 = 4; p1' = 104 + Clip3(-2, 2, (104 + 117 - 208) >> 1 = 6) = 106
    assert run([104, 104, 104, 104, 130, 130, 130, 130], 1, 36, 36) == [104, 104, 106, 108, 126, 128, 130, 130]
    # bS 4, |p0 - q0| = 8 < (50 >> 2) + 2 = 14, ap = 0 < 11, aq = 12 >= 11: strong on p only
    # p0' = (100 + 200 + 200 + 216 + 110 + 4) >> 3 = 103, p1' = (100 + 100 + 100 + 108 + 2) >> 2 = 102, p2' = (2 * 96 + 300 + 100 + 100 + 108 + 4) >> 3 = 100
    # q0' = (2 * 110 + 108 + 100 + 2) >> 2 = 107
    assert run([96, 100, 100, 100, 108, 110, 120, 121], 4, 36, 36) == [96, 100, 102, 103, 107, 110, 120, 121]
    # beta test on q fails (|q1 - q0| = 11): nothing changes
    assert run([96, 100, 100, 100, 108, 119, 120, 121], 3, 36, 36) == [96, 100, 100, 100, 108, 119, 120, 121]
