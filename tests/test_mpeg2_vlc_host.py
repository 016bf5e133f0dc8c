"""MPEG-2 option mpeg2_device_vlc without a GPU.

The device routine of k_mpeg2_vlc (mpeg2_vlc.h) is a __host__ __device__ function: tests/native/mpeg2_vlc_check.cpp walks it on the CPU over every
slice the prescan (mpeg2_slice_scan) lists, with buffers of exactly the device's sizes, next to the host decoder mpeg2_decode_picture, and compares
the records (without `first`), every block's entry sequence, the clamped count and the error flag.  Then crafted extremes, damage per kind, the
pictures the prescan sends to the host path, the option's refusals, parse-only handles and the sanitizer program tools/mpeg2_vlc_asan.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scripted_mpeg2 as S
from jmcodec_amd import api
from test_mpeg2_gpu import SIZES
from test_mpeg2_host import _refusal_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the kinds of damage of mpeg2_vlc.h, by their place in the enumeration
KIND = {name: i + 1 for i, name in enumerate(
    ("fcode", "motion_code", "dc_size", "dc_range", "dct_code", "empty_block", "escape_level", "block_length", "mb_type", "motion_type", "quant_code",
     "marker", "no_prediction", "cbp", "slice_end", "increment", "address", "skipped_in_i", "capacity", "dual_prime"))}
FIELDS = ("pictures", "accepted", "host_path", "mb_diff", "error_flag_diff", "clamped", "host_clamped", "damaged_slices", "bound_broken", "not_tiled",
          "dual_prime", "slices", "holes", "damaged_pictures", "cap_reached", "mid_row_slices", "kinds", "host_refused", "host_damaged", "row_gap",
          "max_slices")


@pytest.fixture(scope="module")
def native():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libmpeg2_vlc_check.so")
    csrc = os.path.join(ROOT, "jmcodec_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "mpeg2_vlc_check.cpp"), os.path.join(csrc, "mpeg2_syntax.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("mpeg2_syntax.h", "mpeg2_vlc.h", "mpeg2_jobs.h")] + [os.path.join(ROOT, "tests", "native", "mpeg2_vlc_walk.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so] + srcs)
    l = C.CDLL(so)
    l.m2v_error.restype = C.c_char_p
    l.m2v_damage_text.restype = C.c_char_p
    l.m2v_capacity.restype = l.m2v_padded.restype = C.c_uint
    l.m2v_capacity.argtypes = [C.c_uint, C.c_uint]
    l.m2v_padded.argtypes = [C.c_uint]
    l.m2v_stream.restype = l.m2v_slices.restype = C.c_long
    l.m2v_stream.argtypes = [C.c_char_p, C.c_long, C.c_void_p]
    l.m2v_slices.argtypes = [C.c_char_p, C.c_long, C.c_void_p, C.c_long]
    return l


def walk(native, data):
    info = (C.c_int * 32)()
    rc = native.m2v_stream(data, len(data), info)
    return rc, dict(zip(FIELDS, info))


def same(native, data, damaged=False):
    """every picture takes the device path, and the walk equals the host decoder; the loop bound and the capacity held"""
    rc, r = walk(native, data)
    assert rc == 0 and r["pictures"] > 0 and r["accepted"] == r["pictures"] and r["host_path"] == 0, r
    assert r["mb_diff"] == 0 and r["error_flag_diff"] == 0 and r["clamped"] == r["host_clamped"], r
    assert r["bound_broken"] == 0 and r["not_tiled"] == 0 and r["dual_prime"] == 0, r
    assert (r["damaged_pictures"] > 0) == damaged and r["damaged_pictures"] == r["host_damaged"], r
    return r


def slices_of(native, data):
    out = np.zeros((256, 8), np.uint32)
    n = native.m2v_slices(data, len(data), out.ctypes.data, 256)
    return [dict(zip(("byte_off", "n_bytes", "row", "lo", "hi", "first_entry", "entry_cap"), (int(v) for v in out[i]))) for i in range(n)]


# ---- the streams of the existing suites ------------------------------------------------------------------------------------------------------
_CASES = dict(S.feature_cases())
_CASES.update(chain=S.chain_stream(), size_change=S.size_change_stream())
_CASES.update({f"size_{w}x{h}": S.sized_stream(w * h, w, h, p) for w, h, p in SIZES})


@pytest.mark.parametrize("name", sorted(_CASES))
def test_walk_equals_host_decoder_on_scripted_cases(native, name):
    same(native, _CASES[name])


def test_clamped_stream_counts_six(native):
    r = same(native, S.clamped_stream(), damaged=False)
    assert r["clamped"] == 6


def test_truncated_stream_is_concealed_like_the_host_path(native):
    r = same(native, S.truncated_stream(), damaged=True)
    assert r["damaged_slices"] == 1 and r["holes"] == 2           # the cut slice (its rest concealed), and the picture that lost a whole slice


@pytest.mark.parametrize("block", range(4))
def test_walk_equals_host_decoder_on_seeded_random_scripts(native, block):
    mid = 0
    for seed in range(50 * block, 50 * block + 50):
        mid += same(native, S.random_stream(seed))["mid_row_slices"]
    assert mid > 0


# ---- crafted cases -----------------------------------------------------------------------------------------------------------------------------
def _anchor(w, h, **kw):
    return ("pic", S.staircase(w, h, **kw))


def test_several_slices_per_row_starting_mid_row(native):
    W, H = 272, 32
    rng = np.random.default_rng(3)
    cuts = (0, 3, 8, 13, 17)
    pic = dict(type="P", f_code=((2, 2), (15, 15)), slices=[
        dict(row=r, qcode=5, mbs=[dict(x=x, fwd=[(0, 0)], blocks={k: S.random_block(rng, False) for k in (0, 5)}) for x in range(cuts[i], cuts[i + 1])])
        for r in range(2) for i in range(4)])
    data = S.build([("seq", dict(width=W, height=H)), _anchor(W, H, step=1), ("pic", pic)])
    r = same(native, data)
    assert r["max_slices"] == 8 and r["mid_row_slices"] == 6
    sl = slices_of(native, data)
    assert [(s["lo"], s["hi"]) for s in sl] == [(17 * r + cuts[i], 17 * r + cuts[i + 1]) for r in range(2) for i in range(4)]
    assert all(s["byte_off"] % 4 == 0 for s in sl)
    assert all(b["byte_off"] == a["byte_off"] + native.m2v_padded(a["n_bytes"]) for a, b in zip(sl, sl[1:]))
    assert native.m2v_guard() >= 55 and native.m2v_padded(5) == 8 + native.m2v_guard()


def test_address_increment_escapes(native):
    """36 macroblocks per row: a skipped run of 34 inside a slice (increment 35 = escape + 2), and a slice whose first macroblock is at column 35
    (first increment 36 = escape + 3) behind a slice that ends at column 0 -- the 34 macroblocks between them are concealed by the first lane"""
    W, H = 576, 16
    p1 = dict(type="P", f_code=((1, 1), (15, 15)), slices=[dict(row=0, qcode=4, mbs=[dict(x=0, fwd=[(0, 0)]), dict(x=35, fwd=[(-1, 0)])])])
    same(native, S.build([("seq", dict(width=W, height=H)), _anchor(W, H, step=1), ("pic", p1)]))
    p2 = dict(type="P", f_code=((1, 1), (15, 15)), slices=[dict(row=0, qcode=4, mbs=[dict(x=0, fwd=[(0, 0)])]), dict(row=0, qcode=4, mbs=[dict(x=35, fwd=[(-1, 0)])])])
    data = S.build([("seq", dict(width=W, height=H)), _anchor(W, H, step=1), ("pic", p2)])
    r = same(native, data, damaged=True)
    assert r["row_gap"] == 35 and r["holes"] == 1 and r["damaged_slices"] == 0
    assert [(s["lo"], s["hi"]) for s in slices_of(native, data)] == [(0, 35), (35, 36)]


def test_one_macroblock_fills_the_capacity_and_the_capacity_formula(native):
    QF = [7] * 64
    pic = dict(type="I", slices=[dict(row=0, qcode=4, mbs=[dict(x=0, intra=True, blocks={k: [100 + k] + QF[1:] for k in range(6)})])])
    data = S.build([("seq", dict(width=16, height=16)), ("pic", pic)])
    r = same(native, data)
    assert r["cap_reached"] == 1
    (s,) = slices_of(native, data)
    assert s["entry_cap"] == 384 and 4 * s["n_bytes"] + 6 > 384
    # a slice of 3 bytes and one macroblock, counted by hand: 00 00 01 01 | 42 d7 00 -- min(384, 4 * 3 + 6) = 18
    QF1 = [0] * 64
    QF1[0] = -1
    data = S.build([("seq", dict(width=16, height=16)), ("pic", S.staircase(16, 16)),
                    ("pic", dict(type="P", f_code=((1, 1), (15, 15)), slices=[dict(row=0, qcode=8, mbs=[dict(x=0, blocks={0: QF1})])]))])
    assert data.endswith(b"\x00\x00\x01\x01\x42\xd7\x00")
    same(native, data)
    (s,) = slices_of(native, data)
    assert (s["n_bytes"], s["lo"], s["hi"], s["entry_cap"]) == (3, 0, 1, 18)
    for L, M in ((0, 1), (3, 1), (95, 1), (94, 1), (1000, 3), (10, 8160), (1 << 20, 8160)):
        assert native.m2v_capacity(L, M) == min(384 * M, 4 * L + 6 * M)


@pytest.mark.parametrize("typ", ["I", "P"])
def test_missing_first_slice_is_concealed_by_the_first_lane(native, typ):
    W, H = 48, 48
    rng = np.random.default_rng(11)
    pic = S.random_picture(rng, typ, W, H, 1, intra_dc_precision=2)
    pic["slices"] = [s for s in pic["slices"] if s["row"] > 0]
    data = S.build([("seq", dict(width=W, height=H)), _anchor(W, H), ("pic", pic)])
    r = same(native, data, damaged=True)
    assert r["holes"] == 1 and r["damaged_slices"] == 0 and r["kinds"] == 0
    assert slices_of(native, data)[0]["lo"] == 0 and slices_of(native, data)[0]["row"] == 1


def _three_rows(bad_slice, typ="I", **kw):
    """48 x 48, I (and P): the slice of row 1 is `bad_slice` (a script or raw bytes), rows 0 and 2 are sound"""
    rng = np.random.default_rng(21)
    pic = S.random_picture(rng, typ, 48, 48, 1, intra_dc_precision=0, frame_pred_frame_dct=1, concealment_mv=0, intra_vlc_format=0, **kw)
    pic["slices"] = [s for s in pic["slices"] if s["row"] == 0][:1] + [bad_slice] + [s for s in pic["slices"] if s["row"] == 2][:1]
    pic["slices"][0]["mbs"] = [dict(x=x, intra=True, blocks={}) for x in range(3)]
    pic["slices"][2]["mbs"] = [dict(x=x, intra=True, blocks={}) for x in range(3)]
    return S.build([("seq", dict(width=48, height=48)), _anchor(48, 48), ("pic", pic)])


def _slice_ending_inside_a_macroblock():
    # the last symbol is the end of block `10`: find levels for which its `1` is the last bit of a byte, and drop the byte that holds its `0`
    for v in range(1, 120):
        sl = dict(row=1, qcode=4, mbs=[dict(x=0, intra=True, blocks={k: [128] + [v if k == 5 else 0] + [0] * 62 for k in range(6)})])
        raw = S._PicWriter(dict(width=48, height=48), dict(type="I")).slice(sl)
        if raw[-1] == 0 and raw[-2] & 1:
            return raw[:-1]
    raise AssertionError("no level puts the end of block across a byte boundary")


_DAMAGE = {
    "invalid_code": (b"\x00\x00\x01\x02" + bytes([0b00100010, 0x00, 0x80]), "mb_type"),           # qcode 4, no extra bits, increment 1, then `000000`
    "slice_ends_inside_a_macroblock": (_slice_ending_inside_a_macroblock(), "slice_end"),
    "dc_out_of_range": (dict(row=1, qcode=4, mbs=[dict(x=0, intra=True, blocks={0: [300] + [0] * 63})]), "dc_range"),
    "skipped_in_i_picture": (dict(row=1, qcode=4, mbs=[dict(x=0, intra=True, blocks={}), dict(x=2, intra=True, blocks={})]), "skipped_in_i"),
    "forbidden_escape_level": (dict(row=1, qcode=4, mbs=[dict(x=0, intra=True, blocks={0: [128, -2048] + [0] * 62})]), "escape_level"),
}


@pytest.mark.parametrize("name", sorted(_DAMAGE))
def test_damage_is_confined_to_its_slice(native, name):
    bad, kind = _DAMAGE[name]
    r = same(native, _three_rows(bad), damaged=True)
    assert r["damaged_slices"] == 1 and r["kinds"] == 1 << KIND[kind] and r["holes"] == 1, r
    assert native.m2v_damage_text(KIND[kind]).decode() in native.m2v_error().decode()          # the host path's wording


def test_damage_texts_are_the_host_paths(native):
    src = open(os.path.join(ROOT, "jmcodec_amd", "csrc", "mpeg2_syntax.cpp")).read()
    for kind in KIND.values():
        if kind != KIND["capacity"]:
            assert 'bad("%s")' % native.m2v_damage_text(kind).decode() in src, kind


def _swapped_slices():
    w = S._PicWriter(dict(width=48, height=48), S.staircase(48, 48))
    sl = [w.slice(s) for s in S.staircase(48, 48)["slices"]]
    return S.build([("seq", dict(width=48, height=48))]) + w.header() + sl[1] + sl[0] + sl[2]


def _qcode_zero():
    return _three_rows(b"\x00\x00\x01\x02" + bytes([0b00000010, 0x80]))


def test_prescan_sends_pictures_it_cannot_accept_to_the_host_path(native):
    for data, word in ((_swapped_slices(), "out of order"), (_qcode_zero(), "quantiser_scale_code 0"),
                       (_three_rows(b"\x00\x00\x01\x09" + bytes([0x22, 0x80])), "outside the picture"),
                       (_three_rows(b"\x00\x00\x01\x02" + bytes([0b00100000, 0x00, 0x00, 0x40])), "invalid macroblock_address_increment"),
                       (_three_rows(b"\x00\x00\x01\x03" + bytes([0b00100000, 0b11000000])), "beyond the picture")):          # row 2, increment 4 = address 9
        rc, r = walk(native, data)
        assert rc == 0 and r["host_path"] == 1 and r["accepted"] == r["pictures"] - 1, (word, r)
        assert word in native.m2v_error().decode(), (word, native.m2v_error())


def test_dual_prime_gives_the_dual_prime_status(native):
    items, _ = _refusal_streams()["dual prime"]
    rc, r = walk(native, S.build(items))
    assert rc == 0 and r["dual_prime"] == 1 and r["host_refused"] == 1 and r["kinds"] == 1 << KIND["dual_prime"], r
    assert native.m2v_damage_text(KIND["dual_prime"]) == b"dual-prime prediction is not supported"


def test_table_size_fits_lds(native):
    assert native.m2v_table_bytes() == 15936 < 64 * 1024


# ---- through the library, without a device -----------------------------------------------------------------------------------------------------
def _parse(data, **opt):
    with api.JmAmdDec(4, 1, options=dict(parse_only=1, **opt)) as d:
        n = d.decode_stream(data, keep=False, chunks=[data])
        return n, {k: d.stat(k) for k in ("errors", "pictures", "syntax_digest", "mpeg2_dev_pictures", "mpeg2_host_pictures", "mpeg2_dev_slices",
                                          "mpeg2_dev_damaged_slices", "mpeg2_clamped_mbs")}


@pytest.mark.parametrize("name", ["chain", "swapped", "qcode_zero", "truncated"])
def test_parse_only_and_digest_handles_take_the_host_path(name):
    data = dict(chain=S.chain_stream(), swapped=_swapped_slices(), qcode_zero=_qcode_zero(), truncated=S.truncated_stream())[name]
    for extra in (dict(), dict(digest=1)):
        n0, st0 = _parse(data, **extra)
        n1, st1 = _parse(data, mpeg2_device_vlc=1, **extra)
        assert n0 == n1 and st1["mpeg2_host_pictures"] == st1["pictures"] > 0 and st1["mpeg2_dev_pictures"] == 0 and st1["mpeg2_dev_slices"] == 0
        assert st0["mpeg2_host_pictures"] == 0                      # counted only on handles that have the option on
        assert (st1["errors"], st1["syntax_digest"], st1["mpeg2_clamped_mbs"]) == (st0["errors"], st0["syntax_digest"], st0["mpeg2_clamped_mbs"])


def test_option_values_and_refusals():
    L = api.lib()
    h = api.jm_nvdec_create_handle()
    try:
        assert L.jm_amddec_set_option(h, b"mpeg2_device_vlc", -1) == -1
        assert L.jm_amddec_set_option(h, b"mpeg2_device_vlc", 2) == -1
        assert L.jm_amddec_set_option(h, b"mpeg2_device_vlc", 1) == 0
        assert L.jm_amddec_set_option(h, b"mpeg2_device_vlc", 0) == 0
        assert L.jm_amddec_set_option(h, b"parse_only", 1) == 0
        assert api.jm_nvdec_init(4, 1, None, 0, h) == 0
        assert L.jm_amddec_set_option(h, b"mpeg2_device_vlc", 1) == -1          # after init
    finally:
        api.jm_nvdec_deinit(h)
    with pytest.raises(RuntimeError, match="mpeg2_device_vlc"):
        api.JmAmdDec(0, 1, options=dict(parse_only=1, mpeg2_device_vlc=1))
    with pytest.raises(RuntimeError, match="jpeg_device_entropy"):               # (its own refusal for codec 4 stays)
        api.JmAmdDec(4, 1, options=dict(parse_only=1, jpeg_device_entropy=1))


# ---- the sanitizer program -----------------------------------------------------------------------------------------------------------------------
def test_mpeg2_vlc_asan_builds_and_runs_clean(tmp_path):
    """tools/mpeg2_vlc_asan.cpp: a stand-alone host program (its own main) under AddressSanitizer / UBSan: the prescan and the device routine over heap
    buffers of exactly the stated sizes, on a few small streams and 2000 seeded mutations of them"""
    out = tmp_path / "out"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "mpeg2_vlc_asan", f"OUT={out}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    path = tmp_path / "a.m2v"
    path.write_bytes(S.chain_stream(n=7) + S.sized_stream(3, 48, 40, 0, "IPBB") + S.feature_cases()["b_field_bidirectional"] +
                     S.feature_cases()["p_intra_concealment"] + S.truncated_stream())
    r = subprocess.run([str(out / "mpeg2_vlc_asan"), str(path), "1", "2001", "100"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=150)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ok: 2001 trials" in r.stdout
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
