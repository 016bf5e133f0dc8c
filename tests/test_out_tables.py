"""The job tables of a batch's output stage (jmcodec_amd/csrc/out_tables.h), checked on seeded random batches against a restatement of the layout rules:

  * each of the four output kernels (k_packout, k_scale_pack, k_rgb_pack, k_deint) has one table of 4 * kMaxBatch jobs; the frames packed BEFORE the batch's
    decode kernels start at entry 0, those packed AFTER them at 2 * kMaxBatch; entries are in picture order and, within a picture, in the order queued;
  * the launch grids are maxima over both sides: k_packout's frame size over the pictures with a plain job, the tiles of the scaled jobs, of the identity and
    of the resampled RGB jobs, the items of the k_deint jobs;
  * a deinterlaced frame of a scaled / RGB handle goes through a scratch surface: surfaces are handed out picture by picture, before side first, each
    (dst_pitch * height * 3 / 2) bytes rounded up to 256; k_deint's dst and the src of the ScaleJob / RgbJob at `index` of the same picture and side are
    that address.  Without scratch the k_deint job is left out, the consumer reads the picture's surface, and the caller is told;
  * frames: every plain / scaled / RGB job and every k_deint job that feeds nobody is one frame.
"""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, SCALE, RGB, DEINT = 0, 1, 2, 3
BEFORE, AFTER = 0, 1
SCRATCH = 0x7000_0000_0000


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libout_tables_check.so")
    src = os.path.join(ROOT, "tests", "native", "out_tables_check.cpp")
    hdrs = [os.path.join(ROOT, "jmcodec_amd", "csrc", h) for h in ("out_tables.h", "jobs.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so, src])
    l = ctypes.CDLL(so)
    l.ot_max_batch.restype = ctypes.c_int
    return l


# the grid functions of tests/native/out_tables_check.cpp
def scale_tiles(tw, th): return 3 * tw + th
def rgb_tiles(tw, th): return tw + 5 * th
def deint_items(w, h): return w * h // 8


def surface_bytes(pitch, height):
    return (pitch * height * 3 // 2 + 255) & ~255


class Batch:
    """A batch as the decoders hand it to the engine: per picture its display size and byte counts, and the rows of tests/native/out_tables_check.cpp."""

    def __init__(self):
        self.pics, self.rows, self.n_frames = [], [], 0
        self._ids = 0

    def tag(self):
        self._ids += 1
        return 0x1000 * self._ids

    def count(self, pic, side, kind):
        return sum(1 for r in self.rows if r[0] == pic and r[1] == side and r[2] == kind)

    def frame(self, pic, side, handle, deinterlaced, rng):
        """One display frame of a handle of the given kind ('plain', 'scale', 'rgb'), queued the way Decoder::enqueue_output does."""
        w, h = self.pics[pic][0], self.pics[pic][1]
        dst, surf = self.tag(), self.tag()
        tw, th = rng.choice([(w, h), (w // 2 & ~1, h // 2 & ~1), (640, 360), (2 * w, 2 * h), (96, 64)])
        src = surf
        if deinterlaced:
            if handle == "plain":
                self.rows.append([pic, side, DEINT, dst, surf, w, h, w, 0, 0])
            else:
                pitch = ((w + 63) & ~63) + rng.choice([0, 16, 80])      # (surfaces whose size is no multiple of 256 among them)
                self.rows.append([pic, side, DEINT, 0, surf, w, h, pitch, 1 if handle == "scale" else 2,
                                  self.count(pic, side, SCALE if handle == "scale" else RGB)])
                src = 0
        if handle == "scale":
            self.rows.append([pic, side, SCALE, dst, src, tw, th, 0, 0, 0])
        elif handle == "rgb":
            self.rows.append([pic, side, RGB, dst, src, tw, th, 1 if (tw, th) == (w, h) else 0, 0, 0])
        elif not deinterlaced:
            self.rows.append([pic, side, PLAIN, dst, surf, w, h, 0, 0, 0])
        self.n_frames += 1


def random_batch(rng, max_batch):
    b = Batch()
    n_pics = rng.choice([1, 2, 5, rng.randrange(1, max_batch + 1), max_batch])
    left = [2 * max_batch, 2 * max_batch]           # what Engine::form leaves room for, per side
    for i in range(n_pics):
        w, h = rng.choice([(176, 144), (720, 576), (1280, 720), (1920, 1080), (3840, 2160), (90, 70)])
        b.pics.append([w, h, rng.randrange(1, 1 << 24), rng.randrange(1, 1 << 24)])
        handle = rng.choice(["plain", "scale", "rgb"])
        deint = rng.random() < 0.5                  # the handle deinterlaces (its progressive frames pass through untouched)
        for side in (BEFORE, AFTER):
            n = rng.choice([0, 0, 1, 1, 1, 2, 3, rng.randrange(0, 17), 16])
            if side == BEFORE and rng.random() < 0.6:
                n = 0
            n = min(n, left[side])
            left[side] -= n
            for _ in range(n):
                b.frame(i, side, handle, deint and rng.random() < 0.8, rng)
    return b


def run(lib, b, scratch):
    cap = 4 * lib.ot_max_batch()
    pics = np.ascontiguousarray(np.array(b.pics, dtype=np.int64).reshape(-1, 4))
    rows = np.ascontiguousarray(np.array(b.rows, dtype=np.int64).reshape(-1, 10))
    out = np.zeros((4, cap, 4), dtype=np.int64)
    info = np.zeros(23, dtype=np.int64)
    ok = np.zeros((len(b.pics), 2), dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.ot_run(p(pics), len(b.pics), p(rows), len(b.rows), ctypes.c_int64(scratch), p(out), p(info), p(ok))
    return out, info, ok


def check(lib, b, scratch):
    """The header's tables against the rules of the module docstring."""
    max_batch = lib.ot_max_batch()
    out, info, ok = run(lib, b, scratch)
    # scratch surfaces: picture by picture, before side first, in the order queued
    offsets, used = {}, 0
    for i in range(len(b.pics)):
        for side in (BEFORE, AFTER):
            for k, r in enumerate(b.rows):
                if r[0] == i and r[1] == side and r[2] == DEINT and r[8]:
                    offsets[k] = used
                    used += surface_bytes(r[7], r[6])
    assert info[21] == used, "bytes_needed, added up over the batch"
    assert info[22] == b.n_frames, "OutSide::frames(), added up over the batch"
    spans = sorted((o, o + b.rows[k][7] * b.rows[k][6] * 3 // 2) for k, o in offsets.items())
    assert all(o % 256 == 0 for o, _ in spans)
    ragged = any((e - o) % 256 for o, e in spans)
    assert all(spans[k][1] <= spans[k + 1][0] for k in range(len(spans) - 1)), "no two scratch surfaces overlap"
    assert not spans or spans[-1][1] <= used
    # what every table must hold
    want = {(kind, side): [] for kind in range(4) for side in (BEFORE, AFTER)}
    told = set()
    for i in range(len(b.pics)):
        for side in (BEFORE, AFTER):
            consumers = {SCALE: [], RGB: []}
            for k, r in enumerate(b.rows):
                if r[0] != i or r[1] != side:
                    continue
                entry = [r[3], r[4], r[5], r[6]]
                if r[2] in consumers:
                    consumers[r[2]].append(entry)
                if r[2] == DEINT and r[8] and not scratch:
                    told.add((i, side))
                    continue                                    # (left out; its consumer is patched below)
                if r[2] == DEINT and r[8]:
                    entry[0] = scratch + offsets[k]
                want[(r[2], side)].append(entry)
            for k, r in enumerate(b.rows):
                if r[0] == i and r[1] == side and r[2] == DEINT and r[8]:
                    consumers[SCALE if r[8] == 1 else RGB][r[9]][1] = scratch + offsets[k] if scratch else r[4]
    for kind in range(4):
        for side in (BEFORE, AFTER):
            w = want[(kind, side)]
            assert info[2 * kind + side] == len(w), (kind, side)
            assert len(w) <= 2 * max_batch
            start = 0 if side == BEFORE else 2 * max_batch
            assert out[kind, start:start + len(w)].tolist() == w, (kind, side)
            assert (out[kind, start + len(w):start + 2 * max_batch] == -1).all(), "entries past the count are not touched"
    # every fed ScaleJob / RgbJob reads what its k_deint job writes
    if scratch:
        for side in (BEFORE, AFTER):
            fed = {tuple(e[:1]) for e in want[(DEINT, side)] if e[0] >= scratch}
            readers = {(e[1],) for kind in (SCALE, RGB) for e in want[(kind, side)] if e[1] >= scratch}
            assert fed == readers
            assert len(fed) == sum(1 for r in b.rows if r[1] == side and r[2] == DEINT and r[8])
    for i in range(len(b.pics)):
        for side in (BEFORE, AFTER):
            assert bool(ok[i, side]) == ((i, side) not in told), "add() reports exactly the sides that needed scratch and found none"
    # grids: maxima over both sides
    plain_pics = {r[0] for r in b.rows if r[2] == PLAIN}
    every = lambda kind: [e for side in (BEFORE, AFTER) for e in want[(kind, side)]]
    rgb_rows = [r for r in b.rows if r[2] == RGB]
    assert info[8] == max([b.pics[i][0] for i in plain_pics], default=0)
    assert info[9] == max([b.pics[i][1] for i in plain_pics], default=0)
    assert info[10] == max([scale_tiles(e[2], e[3]) for e in every(SCALE)], default=0)
    assert info[11] == max([rgb_tiles(r[5], r[6]) for r in rgb_rows if r[7]], default=0)
    assert info[12] == max([rgb_tiles(r[5], r[6]) for r in rgb_rows if not r[7]], default=0)
    assert info[13] == max([deint_items(e[2], e[3]) for e in every(DEINT)], default=0)
    # profiling sums
    frames_of = lambda i: sum(1 for r in b.rows if r[0] == i and (r[2] != DEINT or not r[8]))
    assert info[14] == sum(b.pics[i][2] * frames_of(i) for i in range(len(b.pics)))
    assert info[15] == sum(b.pics[r[0]][2] for r in rgb_rows)
    launched = [r for r in b.rows if r[2] == DEINT and (scratch or not r[8])]
    assert info[16] == sum(b.pics[r[0]][3] for r in launched)
    assert (info[17], info[18], info[19]) == (b.n_frames, len(rgb_rows), len(launched))
    assert info[20] == (used if scratch else 0)
    return info, ragged


def test_random_batches_follow_the_layout_rules(lib):
    rng = random.Random(0x0A7B)
    seen = np.zeros(8, dtype=np.int64)
    fed = rounded = 0
    for trial in range(150):
        b = random_batch(rng, lib.ot_max_batch())
        info, ragged = check(lib, b, SCRATCH)
        seen += info[:8]
        fed += int(info[20] > 0)
        rounded += ragged
    assert (seen > 0).all(), "every table was exercised on both sides"
    assert fed > 50 and rounded > 20, "scratch surfaces were handed out, some of a size that needs the rounding"


def test_without_scratch_the_consumers_read_the_surface_and_the_caller_is_told(lib):
    rng = random.Random(0x5C7A)
    told = 0
    for trial in range(60):
        b = random_batch(rng, lib.ot_max_batch())
        check(lib, b, 0)
        told += any(r[2] == DEINT and r[8] for r in b.rows)
    assert told > 20


def test_full_sides_fit_their_half_of_a_table(lib):
    """2 * kMaxBatch frames on each side, of one kind each: the before side ends where the after side starts."""
    n = lib.ot_max_batch()
    for handle, deint in (("plain", False), ("scale", False), ("rgb", True), ("plain", True), ("scale", True)):
        rng = random.Random(11)
        b = Batch()
        for i in range(n):
            b.pics.append([1280, 720, 1000 + i, 7])
            for side in (BEFORE, AFTER):
                for _ in range(2):
                    b.frame(i, side, handle, deint, rng)
        info, _ = check(lib, b, SCRATCH)
        assert max(info[:8]) == 2 * n
