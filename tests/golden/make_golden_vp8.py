"""Writes tests/golden/vp8: small lossy WebP pictures from libwebp's encoder (through Pillow) and libwebp's own decode of each -- the Y, U and V planes
that WebPDecodeYUV returns, not RGB -- as *.y.npy / *.u.npy / *.v.npy.  Needs Pillow with its bundled libwebp; the tests need neither.

While writing it asserts what tests/test_vp8_host.py re-checks from the committed files: the Python restatement (tests/vp8_ref.py) equals libwebp's
planes in every sample, and the fixtures together show the features listed in REQUIRED.  With the library's WebPEncode reached through ctypes (a
WebPConfig of our own) it adds pictures with the simple filter, several token partitions, one segment and filter_sharpness 7; if the structure
layout does not validate (WebPConfigInitInternal / WebPValidateConfig return 0: an ABI mismatch) those are left out and the script says so.

Run from the repository root:  python tests/golden/make_golden_vp8.py"""
import ctypes as C
import glob
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vp8_ref as R      # noqa: E402

OUT = os.path.join(HERE, "vp8")
_d = os.path.join(os.path.dirname(PIL.__file__), "..", "pillow.libs")
C.CDLL(glob.glob(_d + "/libsharpyuv*")[0], mode=C.RTLD_GLOBAL)      # first, or libwebp does not load
L = C.CDLL(glob.glob(_d + "/libwebp-*")[0])
L.WebPDecodeYUV.restype = C.POINTER(C.c_uint8)


def webp_yuv(data):
    w, h, st, ust = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    u, v = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)()
    y = L.WebPDecodeYUV(data, len(data), C.byref(w), C.byref(h), C.byref(u), C.byref(v), C.byref(st), C.byref(ust))
    assert y, "WebPDecodeYUV failed"
    W, H = w.value, h.value
    Y = np.ctypeslib.as_array(y, (H, st.value))[:, :W].copy()
    U = np.ctypeslib.as_array(u, ((H + 1) // 2, ust.value))[:, :(W + 1) // 2].copy()
    V = np.ctypeslib.as_array(v, ((H + 1) // 2, ust.value))[:, :(W + 1) // 2].copy()
    return Y, U, V


def content(w, h, seed, flat=False):
    """flat areas, edges, texture and a gradient, from a seed"""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 3), np.float64)
    img[..., 0] = xx * 255.0 / max(w - 1, 1)
    img[..., 1] = yy * 255.0 / max(h - 1, 1)
    img[..., 2] = 128
    img[: h // 2, : w // 2] = r.randint(0, 256, 3)
    img[h // 3: h // 3 + 5, :] = 255 - img[h // 3: h // 3 + 5, :]
    t = r.randint(0, 256, (h, w, 3))
    img[h // 2:, w // 2:] = t[h // 2:, w // 2:]
    img[:, w // 4: w // 4 + 2] = 0
    if flat:
        img[:, : (3 * w) // 4] = r.randint(0, 256, 3)
    if flat == 2:
        img[2 * (h // 3):] = r.randint(0, 256, 3)          # (a flat lower third on top of it: whole macroblock rows without coefficients)
    return np.clip(img, 0, 255).astype(np.uint8)


# (name, width, height, quality, method, flat)
PILLOW = [("p16x16_q50_m4", 16, 16, 50, 4, False), ("p16x16_q1_m0", 16, 16, 1, 0, False), ("p48x32_q90_m4", 48, 32, 90, 4, False),
          ("p48x32_q10_m0", 48, 32, 10, 0, False), ("p53x37_q10_m6", 53, 37, 10, 6, False), ("p53x37_q100_m4", 53, 37, 100, 4, False),
          ("p272x16_q1_m0", 272, 16, 1, 0, False), ("p272x16_q50_m6", 272, 16, 50, 6, False), ("p16x272_q100_m4", 16, 272, 100, 4, False),
          ("p80x272_q50_m6", 80, 272, 50, 6, False), ("p64x48_q30_m0", 64, 48, 30, 0, False), ("p96x64_flat_q50_m0", 96, 64, 50, 0, True),
          ("p33x17_q90_m6", 33, 17, 90, 6, False), ("p64x96_flat_q75_m0", 64, 96, 75, 0, 2)]


# ---- WebPEncode through ctypes (libwebp's src/webp/encode.h, ABI 0x02xx) ----
class WebPConfig(C.Structure):
    _fields_ = [(n, C.c_float if n in ("quality", "target_PSNR") else C.c_int) for n in (
        "lossless", "quality", "method", "image_hint", "target_size", "target_PSNR", "segments", "sns_strength", "filter_strength", "filter_sharpness",
        "filter_type", "autofilter", "alpha_compression", "alpha_filtering", "alpha_quality", "pass_", "show_compressed", "preprocessing", "partitions",
        "partition_limit", "emulate_jpeg_size", "thread_level", "low_memory", "near_lossless", "exact", "use_delta_palette", "use_sharp_yuv", "qmin", "qmax")]


class WebPMemoryWriter(C.Structure):
    _fields_ = [("mem", C.POINTER(C.c_uint8)), ("size", C.c_size_t), ("max_size", C.c_size_t), ("pad", C.c_uint32 * 1)]


class WebPPicture(C.Structure):
    _fields_ = [("use_argb", C.c_int), ("colorspace", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("y_stride", C.c_int), ("uv_stride", C.c_int), ("a", C.c_void_p), ("a_stride", C.c_int),
                ("pad1", C.c_uint32 * 2), ("argb", C.c_void_p), ("argb_stride", C.c_int), ("pad2", C.c_uint32 * 3),
                ("writer", C.c_void_p), ("custom_ptr", C.c_void_p), ("extra_info_type", C.c_int), ("extra_info", C.c_void_p), ("stats", C.c_void_p),
                ("error_code", C.c_int), ("progress_hook", C.c_void_p), ("user_data", C.c_void_p), ("pad3", C.c_uint32 * 3),
                ("pad4", C.c_void_p), ("pad5", C.c_void_p), ("pad6", C.c_uint32 * 8), ("memory_", C.c_void_p), ("memory_argb_", C.c_void_p), ("pad7", C.c_void_p * 2),
                ("slack", C.c_uint8 * 256)]      # (room to spare, should a later version have grown the structure)


def encode_config(rgb, **settings):
    """rgb: h x w x 3 uint8 -> the WebP file's bytes, or None when the structures do not validate against this libwebp"""
    for abi in (0x020f, 0x0210, 0x0211, 0x020e):
        cfg = WebPConfig()
        if L.WebPConfigInitInternal(C.byref(cfg), 0, C.c_float(settings.get("quality", 50.0)), abi):
            break
    else:
        return None
    for k, v in settings.items():
        setattr(cfg, k, v)
    if not L.WebPValidateConfig(C.byref(cfg)):
        return None
    pic = WebPPicture()
    if not L.WebPPictureInitInternal(C.byref(pic), abi):
        return None
    h, w = rgb.shape[:2]
    pic.width, pic.height = w, h
    buf = np.ascontiguousarray(rgb)
    if not L.WebPPictureImportRGB(C.byref(pic), buf.ctypes.data_as(C.c_void_p), w * 3):
        return None
    wr = WebPMemoryWriter()
    L.WebPMemoryWriterInit(C.byref(wr))
    pic.writer = C.cast(L.WebPMemoryWrite, C.c_void_p)
    pic.custom_ptr = C.cast(C.pointer(wr), C.c_void_p)
    ok = L.WebPEncode(C.byref(cfg), C.byref(pic))
    data = bytes(C.string_at(wr.mem, wr.size)) if ok else None
    L.WebPPictureFree(C.byref(pic))
    L.WebPMemoryWriterClear(C.byref(wr))
    return data


# (name, width, height, seed, settings)
CONFIG = [("c48x32_simple", 48, 32, 3, dict(quality=40.0, filter_type=0, filter_strength=40, autofilter=0)),
          ("c48x144_parts2", 48, 144, 4, dict(quality=60.0, partitions=1, method=2)), ("c48x144_parts8", 48, 144, 5, dict(quality=60.0, partitions=3, method=2)),
          ("c64x48_seg1", 64, 48, 6, dict(quality=50.0, segments=1)), ("c64x48_sharp7", 64, 48, 7, dict(quality=30.0, filter_sharpness=7, filter_strength=60)),
          ("c80x48_parts4_simple", 80, 48, 8, dict(quality=20.0, partitions=2, method=1, filter_type=0, filter_strength=50, segments=4, sns_strength=100))]

REQUIRED = "every 16x16 luma mode, every chroma mode, all ten sub-block modes, >= 2 segments, skipped and coded macroblocks, the normal filter " \
           "with non-zero levels, macroblock-edge and inner-edge filtering"


def main():
    os.makedirs(OUT, exist_ok=True)
    files = []
    for name, w, h, q, m, flat in PILLOW:
        b = io.BytesIO()
        Image.fromarray(content(w, h, w * h + q, flat)).save(b, "WEBP", quality=q, method=m)
        files.append((name, b.getvalue()))
    skipped = []
    for name, w, h, seed, st in CONFIG:
        data = encode_config(content(w, h, seed), **st)
        if data is None:
            skipped.append(name)
        else:
            files.append((name, data))
    agg = {}
    for name, data in files:
        Y, U, V = webp_yuv(data)
        y, u, v, info = R.decode_planes(R.webp_payload(data))
        assert (y == Y).all() and (u == U).all() and (v == V).all(), name + ": the restatement differs from libwebp"
        assert info["errors"] == 0, name
        with open(os.path.join(OUT, name + ".webp"), "wb") as f:
            f.write(data)
        for pl, a in (("y", Y), ("u", U), ("v", V)):
            np.save(os.path.join(OUT, "%s.%s.npy" % (name, pl)), a)
        for k, val in info.items():
            if isinstance(val, set):
                agg.setdefault(k, set()).update(val)
            elif isinstance(val, int):
                agg[k] = agg.get(k, 0) + val
        print(name, len(data), "bytes", {k: sorted(info[k]) for k in ("partitions", "filter_types", "sharpness", "segments")}, "skipped", info["skipped_mbs"])
    assert agg["ymodes"] == set(range(5)) and agg["uvmodes"] == set(range(4)) and agg["bmodes"] == set(range(10)), agg
    assert len(agg["segments"]) >= 2 and agg["skipped_mbs"] > 0 and agg["coded_mbs"] > 0, agg
    assert 0 in agg["filter_types"] and any(agg["levels"]) and agg["mb_edge_mbs"] > 0 and agg["inner_edge_mbs"] > 0, agg
    print("all fixtures equal libwebp; together they show", REQUIRED)
    print({k: (sorted(v) if isinstance(v, set) else v) for k, v in agg.items()})
    if skipped:
        print("NOT written (WebPConfig did not validate against this libwebp):", skipped)


if __name__ == "__main__":
    main()
