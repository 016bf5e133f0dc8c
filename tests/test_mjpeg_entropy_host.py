"""MJPEG option jpeg_device_entropy without a GPU.

The device routine of k_jpeg_entropy (jpeg_entropy.h) is a __host__ __device__ function: tests/native/jpeg_entropy_check.cpp walks it on the CPU over
every segment the segmenter (jpeg_segment_scan) makes, with buffers of exactly the device's sizes, and this file compares the result, per block the
list of (position, level), with the host decoder jpeg_decode_scan.  Then crafted extremes, damage per kind, parse-only handles and the sanitizer
program tools/jpeg_entropy_asan.cpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import jpeg_ref
from jmcodec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODABLE = ["g_8x8", "c420_16x16", "c420_53x37", "c420_72x40_rst3", "c422_48x32", "c444_40x24", "c444_53x37", "c420_64x48_opt", "c420_32x32_q1", "g_37x21"]
Q = [[16] * 64, [17] * 64]


def fixture(name):
    return open(os.path.join(jpeg_ref.GOLDEN_JPEG, name + ".jpg"), "rb").read()


@pytest.fixture(scope="module")
def native():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libjpeg_entropy_check.so")
    csrc = os.path.join(ROOT, "jmcodec_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "jpeg_entropy_check.cpp"), os.path.join(csrc, "jpeg_syntax.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("jpeg_syntax.h", "jpeg_entropy.h")] + [os.path.join(ROOT, "tests", "native", "jpeg_entropy_walk.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so] + srcs)
    l = C.CDLL(so)
    l.jec_error.restype = C.c_char_p
    l.jec_capacity.restype = C.c_uint
    l.jec_capacity.argtypes = [C.c_uint, C.c_uint]
    vp = C.c_void_p
    l.jec_host.restype = C.c_long
    l.jec_host.argtypes = [C.c_char_p, C.c_long, vp, vp, vp, C.c_long, C.c_long, vp]
    l.jec_walk.restype = C.c_long
    l.jec_walk.argtypes = [C.c_char_p, C.c_long, vp, vp, vp, C.c_long, C.c_long, vp, vp, C.c_long, vp, C.c_long, vp]
    return l


NB, NE, NS, NC = 1 << 14, 1 << 20, 1 << 12, 1 << 20


def _lists(first, count, entries, n):
    return [tuple(int(v) for v in entries[first[i]:first[i] + count[i]]) for i in range(n)]


def host(native, pic, reset=True):
    """The host decoder's blocks of one picture: a list per block of entry words (position | level << 16)."""
    if reset:
        native.jec_reset()
    first, count, entries, info = np.zeros(NB, np.uint32), np.zeros(NB, np.uint8), np.zeros(NE, np.uint32), (C.c_int * 4)()
    rc = native.jec_host(pic, len(pic), first.ctypes.data, count.ctypes.data, entries.ctypes.data, NB, NE, info)
    assert rc == 0, (rc, native.jec_error())
    return dict(blocks=_lists(first, count, entries, info[0]), error=bool(info[2]))


def walk(native, pic, reset=True):
    if reset:
        native.jec_reset()
    first, count, entries = np.zeros(NB, np.uint32), np.zeros(NB, np.uint8), np.zeros(NE, np.uint32)
    segs, dmg, clean, info = np.zeros((NS, 6), np.uint32), np.zeros(NS, np.int32), np.zeros(NC, np.uint8), (C.c_int * 12)()
    rc = native.jec_walk(pic, len(pic), first.ctypes.data, count.ctypes.data, entries.ctypes.data, NB, NE, segs.ctypes.data, dmg.ctypes.data, NS,
                         clean.ctypes.data, NC, info)
    assert rc == 0, (rc, native.jec_error())
    n_seg = info[1]
    keys = ("blocks", "segments", "capacity", "damaged", "seg_error", "bound_ok", "cap_reached", "covered", "differ", "host_error", "clean_bytes", "host_entries")
    r = dict(zip(keys, list(info)))
    r.update(lists=_lists(first, count, entries, info[0]), first=first[:info[0]].copy(), count=count[:info[0]].copy(),
             segs=[dict(zip(("off", "len", "first_mcu", "n_mcus", "first_entry", "cap"), (int(v) for v in s))) for s in segs[:n_seg]],
             seg_damage=[int(v) for v in dmg[:n_seg]], clean=clean[:info[10]].tobytes(), error=native.jec_error().decode())
    return r


def clean_walk(native, pic, reset=True):
    """A picture both decoders accept: the walk equals the host decoder block for block, within every bound."""
    r = walk(native, pic, reset)
    assert (r["damaged"], r["seg_error"], r["host_error"]) == (0, 0, 0), r["error"]
    assert r["bound_ok"] and r["covered"] and r["differ"] == 0
    assert sum(int(c) for c in r["count"]) == r["host_entries"]
    return r


def geometry(pic):
    hd = jpeg_ref.RefDecoder().headers(pic)
    ncomp = len(hd["comps"])
    hs, vs = (hd["sampling"] >> 4, hd["sampling"] & 15) if ncomp == 3 else (1, 1)
    mx, my = -(-hd["w"] // (8 * hs)), -(-hd["h"] // (8 * vs))
    return dict(ncomp=ncomp, hs=hs, vs=vs, mx=mx, my=my, bpm=hs * vs + 2 if ncomp == 3 else 1, data=hd["data"])


def seg_blocks(g, seg):
    """Block indices (plane raster order, the indexing of jpeg_decode_scan) of a segment, in scan order."""
    out, nY, nC = [], g["mx"] * g["hs"] * g["my"] * g["vs"], g["mx"] * g["my"]
    for mcu in range(seg["first_mcu"], seg["first_mcu"] + seg["n_mcus"]):
        my, mx = divmod(mcu, g["mx"])
        out += [(my * g["vs"] + v) * g["mx"] * g["hs"] + mx * g["hs"] + h for v in range(g["vs"]) for h in range(g["hs"])]
        out += [nY + c * nC + my * g["mx"] + mx for c in range(g["ncomp"] - 1)]
    return out


def check_layout(native, r, g, pieces, dri):
    """Offsets, lengths, unstuffing, alignment, guard, MCU ranges, entry ranges of a walk against the pieces of the scan."""
    guard, mcus, off, ent = native.jec_guard(), g["mx"] * g["my"], 0, 0
    per = dri if dri else mcus
    assert len(r["segs"]) == -(-mcus // per)
    for i, s in enumerate(r["segs"]):
        piece = pieces[i] if i < len(pieces) else b""
        assert s["off"] == off and s["off"] % 4 == 0 and s["len"] == len(piece)
        padded = (len(piece) + 3 & ~3) + guard
        assert r["clean"][off:off + len(piece)] == piece                       # FF 00 unstuffed, fill bytes and the marker gone
        assert r["clean"][off + len(piece):off + padded] == bytes(padded - len(piece))      # padding and guard: zeros
        assert (s["first_mcu"], s["n_mcus"]) == (i * per, min(per, mcus - i * per))
        assert s["first_entry"] == ent and s["cap"] == min(64 * s["n_mcus"] * g["bpm"], 4 * len(piece) + s["n_mcus"] * g["bpm"])
        assert s["cap"] == native.jec_capacity(len(piece), s["n_mcus"] * g["bpm"])
        off, ent = off + padded, ent + s["cap"]
    assert len(r["clean"]) == off and r["capacity"] == ent


# ---- the segmenter ------------------------------------------------------------------------------------------------------------------------
def test_segmenter_on_the_restart_fixture(native):
    pic = fixture("c420_72x40_rst3")
    g = geometry(pic)
    r = clean_walk(native, pic)
    pieces = [p for p, _ in jpeg_ref._segments(g["data"])]
    assert len(pieces) == 5 and len(r["segs"]) == 5                            # 15 MCUs, 3 per interval
    check_layout(native, r, g, pieces, 3)


@pytest.mark.parametrize("dri,fill,rst_offset", [(1, 0, 0), (2, 3, 5), (4, 1, 7), (7, 2, 3)])
def test_segmenter_fill_bytes_odd_indices_and_unstuffing(native, dri, fill, rst_offset):
    rng = np.random.default_rng(0x5E60 + dri)
    lv = jpeg_ref.random_levels(rng, 0x22, 72, 40, density=0.4, amp=300)
    lv[0][:, :, 1] = 255                                                        # long runs of 1 bits: stuffed FF bytes
    pic = jpeg_ref.encode(lv, Q, 0x22, 72, 40, dri=dri, fill_before_rst=fill, rst_offset=rst_offset)
    g = geometry(pic)
    assert b"\xff\x00" in g["data"]
    r = clean_walk(native, pic)
    pieces = [p for p, _ in jpeg_ref._segments(g["data"])]
    assert any(0xFF in p for p in pieces)
    check_layout(native, r, g, pieces, dri)


def _rst_stream(dri=5, w=40, h=24, samp=0x11, seed=5):
    rng = np.random.default_rng(seed)
    lv = jpeg_ref.random_levels(rng, samp, w, h, density=0.3)
    return jpeg_ref.encode(lv, Q, samp, w, h, dri=dri)


def test_a_missing_marker_gives_empty_segments_and_an_error(native):
    pic = _rst_stream()                                                         # 5 x 3 MCUs, one row per segment
    at = pic.index(b"\xff\xd1")
    broken = pic[:at] + pic[at + 2:]                                            # the second marker gone: segments 1 and 2 run together
    r = walk(native, broken)
    assert r["seg_error"] == 1 and "restart marker is missing" in r["error"]
    assert [s["n_mcus"] for s in r["segs"]] == [5, 5, 5] and r["covered"] and r["bound_ok"]
    assert r["segs"][2]["len"] == 0 and r["segs"][2]["cap"] == 5 * 3            # nothing left for the last one: empty, capacity B
    good = clean_walk(native, pic)
    g = geometry(pic)
    for i in seg_blocks(g, r["segs"][0]):
        assert r["lists"][i] == good["lists"][i]
    for i in seg_blocks(g, r["segs"][2]):
        assert r["lists"][i] == ()
    assert r["seg_damage"][2] != 0 and r["seg_damage"][0] == 0


def test_a_surplus_marker_is_dropped_with_an_error(native):
    pic = _rst_stream()
    eoi = pic.rindex(b"\xff\xd9")
    extra = pic[:eoi] + b"\xff\xd3" + b"\x12\x34\x56" + pic[eoi:]
    r = walk(native, extra)
    assert r["seg_error"] == 1 and "more restart markers" in r["error"]
    assert len(r["segs"]) == 3 and r["damaged"] == 0 and r["bound_ok"] and r["covered"]
    assert r["lists"] == clean_walk(native, pic)["lists"]


# ---- the CPU walk against the host decoder ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DECODABLE)
def test_walk_equals_host_decoder_on_fixtures_as_one_segment(native, name):
    """Option 2 semantics: a picture without DRI is one segment.  (The restart fixture keeps its five.)"""
    r = clean_walk(native, fixture(name))
    assert r["segments"] == (5 if name == "c420_72x40_rst3" else 1)


@pytest.mark.parametrize("samp", [0x22, 0x21, 0x11, 0x10])
@pytest.mark.parametrize("dri", [1, 2, 4, 7])
def test_walk_equals_host_decoder_on_seeded_streams(native, samp, dri):
    rng = np.random.default_rng(0x4A45 + samp * 16 + dri)
    for density, amp in ((0.05, 3), (0.3, 60), (0.9, 1023)):
        lv = jpeg_ref.random_levels(rng, samp, 72, 40, density=density, amp=amp, dc_amp=1023)
        pic = jpeg_ref.encode(lv, Q, samp, 72, 40, dri=dri, fill_before_rst=int(rng.integers(0, 3)), rst_offset=int(rng.integers(0, 8)))
        g = geometry(pic)
        r = clean_walk(native, pic)
        mcus = g["mx"] * g["my"]
        assert [s["n_mcus"] for s in r["segs"]] == [min(dri, mcus - i) for i in range(0, mcus, dri)]
        if samp == 0x22 and dri == 4:
            assert [s["n_mcus"] for s in r["segs"]] == [4, 4, 4, 3]


@pytest.mark.parametrize("w,h,samp,dri", [(72, 40, 0x22, 15), (72, 40, 0x22, 16), (72, 40, 0x22, 1000), (200, 16, 0x21, 3), (37, 21, 0x10, 2)])
def test_walk_interval_as_long_as_the_picture_and_odd_sizes(native, w, h, samp, dri):
    rng = np.random.default_rng(w * 131 + dri)
    pic = jpeg_ref.encode(jpeg_ref.random_levels(rng, samp, w, h, density=0.4, amp=200), Q, samp, w, h, dri=dri)
    g = geometry(pic)
    r = clean_walk(native, pic)
    assert r["segments"] == -(-g["mx"] * g["my"] // dri)


def test_walk_keeps_tables_from_picture_to_picture(native):
    rng = np.random.default_rng(11)
    lv = jpeg_ref.random_levels(rng, 0x22, 48, 32, density=0.3)
    pics = [jpeg_ref.encode(lv, Q, 0x22, 48, 32, dri=2), jpeg_ref.encode(lv, Q, 0x22, 48, 32, tables=False), jpeg_ref.encode(lv, Q, 0x22, 48, 32, dht=False, dri=3)]
    native.jec_reset()
    segs = [clean_walk(native, p, reset=False)["segments"] for p in pics]
    assert segs == [3, 1, 2]                                                    # SOI disables the restart interval: the second picture is one segment


# ---- extremes: hand-written DHT segments ----------------------------------------------------------------------------------------------------
def crafted(w, h, dc, ac, scan, dri=0):
    """A grey picture with its own DC / AC table (jpeg_ref.Huff) and entropy-coded bytes written by the test."""
    out = b"\xff\xd8" + jpeg_ref._seg(0xDB, bytes([0]) + bytes([1] * 64))
    out += jpeg_ref._seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([1, 1, 0x11, 0]))
    out += jpeg_ref.dht_segment({(0, 0): dc, (1, 0): ac})
    if dri:
        out += jpeg_ref._seg(0xDD, dri.to_bytes(2, "big"))
    return out + jpeg_ref._seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + scan + b"\xff\xd9"


def huff(lengths):
    """{code length: [symbols]} -> jpeg_ref.Huff"""
    return jpeg_ref.Huff([len(lengths.get(l, [])) for l in range(1, 17)], [v for l in range(1, 17) for v in lengths.get(l, [])])


def entry(pos, level):
    return pos | (level & 0xFFFF) << 16


def one_bit_stream():
    """DC table: one code, '0' -> category 1; AC table: one code, '0' -> run 0, size 1.  Every entry costs 2 bits: 64 entries in 16 bytes, k reaches 63
    without an EOB, and min(64 B, 4 L + B) = min(64, 65) entries are all used."""
    dc, ac = huff({1: [1]}), huff({1: [0x01]})
    w = jpeg_ref._Writer()
    signs = [1 if (i * 7) % 3 else 0 for i in range(64)]
    for s in signs:
        w.put(0, 1)
        w.put(s, 1)
    assert w.n == 0 and len(w.out) == 16
    return crafted(8, 8, dc, ac, bytes(w.out)), signs


def test_one_bit_codes_a_block_of_64_entries_no_eob_and_the_capacity_reached_exactly(native):
    pic, signs = one_bit_stream()
    r = clean_walk(native, pic)
    assert r["segs"][0]["len"] == 16 and r["segs"][0]["cap"] == 64 and r["cap_reached"] == 1
    assert r["lists"] == [tuple(entry(k, 1 if s else -1) for k, s in enumerate(signs))]


def sixteen_bit_stream():
    """AC table: '0' -> 0x01, then two 16-bit codes: 0x8000 -> EOB, 0x8001 -> ZRL."""
    dc, ac = huff({1: [1]}), huff({1: [0x01], 16: [0x00, 0xF0]})
    assert ac.enc[0x00] == (0x8000, 16) and ac.enc[0xF0] == (0x8001, 16)
    w = jpeg_ref._Writer()
    for code, ln in ((0, 1), (1, 1),                                            # DC +1
                     (0, 1), (1, 1),                                            # k = 1: +1
                     ac.enc[0xF0], ac.enc[0xF0], (0, 1), (0, 1),                # two ZRL: k = 34: -1
                     ac.enc[0xF0], (0, 1), (1, 1),                              # k = 51: +1
                     ac.enc[0x00],                                              # EOB
                     (0, 1), (0, 1),                                            # second block: DC -1 -> 0, no entry
                     ac.enc[0xF0], ac.enc[0xF0], ac.enc[0xF0], ac.enc[0xF0]):   # four ZRL pass position 63: the block ends, as on the host
        w.put(code, ln)
    w.align()
    return crafted(16, 8, dc, ac, bytes(w.out))


def test_sixteen_bit_codes_and_zrl_runs(native):
    r = clean_walk(native, sixteen_bit_stream())
    assert r["lists"] == [(entry(0, 1), entry(1, 1), entry(34, -1), entry(51, 1)), ()]


def test_dc_sum_that_leaves_int16_saturates(native):
    lv = [np.zeros((1, 20, 64), np.int64)]
    lv[0][0, :, 0] = [2047 * (i + 1) for i in range(20)]                        # differences of category 11; the sum passes 32767 at the 17th block
    pic = jpeg_ref.encode(lv, Q, 0x10, 160, 8)
    r = clean_walk(native, pic)
    assert r["lists"] == [(entry(0, min(32767, 2047 * (i + 1))),) for i in range(20)]
    lv[0][0, :, 0] = [-2047 * (i + 1) for i in range(20)]
    r = clean_walk(native, jpeg_ref.encode(lv, Q, 0x10, 160, 8))
    assert r["lists"][-1] == (entry(0, -32768),)


# ---- damage ---------------------------------------------------------------------------------------------------------------------------------
def check_contained(native, clean, damaged, seg, kind=None):
    """Segment `seg` of `damaged` is damaged: the other segments equal the clean picture's blocks, the damaged one equals them up to some block
    and is empty from there on; the bounds hold."""
    good, r, g = clean_walk(native, clean), walk(native, damaged), geometry(clean)
    assert r["bound_ok"] and r["covered"] and r["damaged"] == 1 and r["host_error"] == 1
    assert [bool(d) for d in r["seg_damage"]] == [i == seg for i in range(len(r["segs"]))]
    if kind is not None:
        assert r["seg_damage"][seg] == kind
    for i, s in enumerate(r["segs"]):
        idx = seg_blocks(g, s)
        if i != seg:
            assert [r["lists"][b] for b in idx] == [good["lists"][b] for b in idx], i
            continue
        same = [r["lists"][b] == good["lists"][b] for b in idx]
        cut = same.index(False) if False in same else len(idx)
        assert cut < len(idx) and all(r["lists"][b] == () for b in idx[cut:])
    return r


def damaged_streams():
    """name -> (clean picture, damaged picture, damaged segment, kind): 4:4:4 40 x 24, one MCU row (8 luma rows) per segment, the middle one damaged.
    tests/test_mjpeg_entropy_gpu.py runs these on the device after the walk here has passed them."""
    pic = _rst_stream()
    a, b = pic.index(b"\xff\xd0") + 2, pic.index(b"\xff\xd1")                   # segment 1 lies between the two markers
    keep = (b - a) // 2
    while pic[a + keep - 1] == 0xFF:                                            # (do not cut a stuffed pair)
        keep -= 1
    return {"truncated": (pic, pic[:a + keep] + pic[b:], 1, 2),
            # sixteen 1 bits: no code of the Annex K tables
            "invalid_code": (pic, pic[:a] + b"\xff\x00\xff\x00\xff\x00" + pic[a + 6:], 1, 1)}


@pytest.mark.parametrize("name", ["truncated", "invalid_code"])
def test_damage_truncation_and_invalid_code(native, name):
    clean, damaged, seg, kind = damaged_streams()[name]
    r = check_contained(native, clean, damaged, seg, kind)
    if name == "invalid_code":                                                  # at the segment's first symbol: the whole segment is empty
        assert all(r["lists"][b] == () for b in seg_blocks(geometry(clean), r["segs"][seg]))


def run_beyond_63_stream():
    """AC table: '0' -> 0xE1 (run 14, size 1), '10' -> EOB.  Five of them pass position 63.  Grey 16 x 8, two MCUs, one per segment: the second decodes
    to DC -1 and +1 at zig-zag position 15."""
    dc, ac = huff({1: [1]}), huff({1: [0xE1], 2: [0x00]})
    w = jpeg_ref._Writer()
    for code, ln in [(0, 1), (1, 1)] + [(0, 1), (1, 1)] * 5:
        w.put(code, ln)
    w.align()
    first = bytes(w.out)
    w = jpeg_ref._Writer()
    for code, ln in ((0, 1), (0, 1), (0, 1), (1, 1), (2, 2)):                   # DC -1, (run 14, +1) at k = 15, EOB
        w.put(code, ln)
    w.align()
    return crafted(16, 8, dc, ac, first + b"\xff\xd0" + bytes(w.out), dri=1)


def test_damage_run_beyond_63(native):
    pic = run_beyond_63_stream()
    r = walk(native, pic)
    assert r["bound_ok"] and r["covered"] and r["seg_damage"] == [1, 0] and r["host_error"] == 1
    assert r["lists"] == [(), (entry(0, -1), entry(15, 1))]


# ---- parse-only handles ---------------------------------------------------------------------------------------------------------------------
def _handle(data, opt, codec=2, extra=None):
    opts = {"parse_only": 1, "job_digest": 1}
    if opt is not None:
        opts["jpeg_device_entropy"] = opt
    opts.update(extra or {})
    with api.JmAmdDec(codec, 1, options=opts) as d:
        frames = d.decode_stream(data, chunks=api.split_jpegs(data))
        return dict(n=len(frames), errors=d.stat("errors"), dev=d.stat("jpeg_dev_pictures"), host=d.stat("jpeg_host_pictures"), segs=d.stat("jpeg_dev_segments"),
                    damaged=d.stat("jpeg_dev_damaged_segments"), digest=d.stat("job_digest"), late=api.lib().jm_amddec_set_option(d.h, b"jpeg_device_entropy", 1))


def test_option_values_and_refusals():
    h = api.jm_nvdec_create_handle()
    try:
        so = api.lib().jm_amddec_set_option
        assert [so(h, b"jpeg_device_entropy", v) for v in (0, 1, 2, 1, 0)] == [0] * 5
        assert [so(h, b"jpeg_device_entropy", v) for v in (-1, 3, 256)] == [-1] * 3
    finally:
        api.jm_nvdec_deinit(h)
    assert _handle(fixture("g_8x8"), 1)["late"] == -1                           # after init
    for codec in (0, 1, 4):
        with pytest.raises(RuntimeError) as e:
            api.JmAmdDec(codec, 1, options={"parse_only": 1, "jpeg_device_entropy": 1})
        assert "jpeg_device_entropy" in str(e.value)
        api.JmAmdDec(codec, 1, options={"parse_only": 1, "jpeg_device_entropy": 0}).close()


def test_option_1_takes_restart_pictures_and_leaves_the_others_to_the_host():
    rst, plain = fixture("c420_72x40_rst3"), fixture("c420_53x37")
    rng = np.random.default_rng(2)
    lv = jpeg_ref.random_levels(rng, 0x22, 72, 40)
    no_dri_second = jpeg_ref.encode(lv, Q, 0x22, 72, 40, dri=3) + jpeg_ref.encode(lv, Q, 0x22, 72, 40, tables=False)      # SOI disables the interval
    one_segment = jpeg_ref.encode(lv, Q, 0x22, 72, 40, dri=15)                 # a restart interval, but a single segment: host
    r = _handle(rst + no_dri_second + one_segment + rst, 1)
    assert (r["n"], r["errors"], r["dev"], r["host"], r["segs"], r["damaged"]) == (5, 0, 3, 2, 15, 0)
    r = _handle(rst + plain + plain, 2)
    assert (r["n"], r["errors"], r["dev"], r["host"], r["segs"]) == (3, 0, 3, 0, 5 + 1 + 1)
    r = _handle(rst + plain, 0)
    assert (r["n"], r["dev"], r["host"], r["segs"]) == (2, 0, 0, 0)


def test_option_0_leaves_the_job_digest_alone():
    for name in DECODABLE:
        a, b = _handle(fixture(name), None), _handle(fixture(name), 0)
        assert a["digest"] == b["digest"] and a["digest"] != 0
    assert _handle(fixture("c420_72x40_rst3"), 1)["digest"] != _handle(fixture("c420_72x40_rst3"), 0)["digest"]      # (another upload: tables, segments, bytes)


def test_segmenter_errors_count_the_picture_once():
    pic = _rst_stream()
    at = pic.index(b"\xff\xd1")
    r = _handle(pic + pic[:at] + pic[at + 2:] + pic, 1)
    assert (r["n"], r["errors"], r["dev"]) == (3, 1, 3)


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------------------
def test_jpeg_entropy_asan_builds_and_runs_clean(tmp_path):
    """tools/jpeg_entropy_asan.cpp: a stand-alone host program (its own main) under AddressSanitizer / UBSan: the segmenter and the device routine over
    exact-size heap buffers, the streams of this file and a few seconds of mutations of them"""
    out = tmp_path / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "jpeg_entropy_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    rng = np.random.default_rng(77)
    stream = b"".join(fixture(n) for n in ("c420_72x40_rst3", "c444_53x37", "g_37x21", "c422_48x32", "c420_64x48_opt"))
    for samp, w, h, dri in ((0x22, 72, 40, 4), (0x21, 200, 16, 3), (0x10, 37, 21, 2), (0x11, 40, 24, 1)):
        stream += jpeg_ref.encode(jpeg_ref.random_levels(rng, samp, w, h, density=0.5, amp=500), Q, samp, w, h, dri=dri, fill_before_rst=1)
    stream += one_bit_stream()[0] + sixteen_bit_stream()                        # (their DHTs replace table 0: last)
    path = tmp_path / "a.mjpeg"
    path.write_bytes(stream)
    r = subprocess.run([str(out / "jpeg_entropy_asan"), str(path), "1", "400", "5"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ok: " in r.stdout and " trials" in r.stdout
    assert int(re.search(r", (\d+) damaged", r.stdout).group(1)) > 0           # the mutations did reach the damage paths
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
    # the damaged streams of this file (the ones tests/test_mjpeg_entropy_gpu.py runs on the device) as they are, and mutated
    bad = tmp_path / "damaged.mjpeg"
    bad.write_bytes(b"".join(d for _, d, _, _ in damaged_streams().values()) + run_beyond_63_stream())
    r = subprocess.run([str(out / "jpeg_entropy_asan"), str(bad), "2", "200", "3", "damaged"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ok: " in r.stdout and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
