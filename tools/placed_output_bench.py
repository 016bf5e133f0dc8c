"""Placed against stretched output, and one build of the library against another, on the bench's workload: S x 1080p H.264 streams of config C1 fed
through jm_amddec_feed_annexb with every frame fetched into a host buffer.  Per leg one JSON line: frames / s and, from the engine's profile counters
(option profile: HIP events around the output launches), the kernel time per frame of the leg's kernel class (packout = k_packout / k_scale_pack,
rgb_pack = k_rgb_pack).  Legs: scale540 (1080p -> 960x540), rgb224 (centre 1080x1080 crop -> 224x224 planar f16, ImageNet normalisation),
stretch640x360, fit640 (1080p letterboxed into 640x640: rectangle 640x360), rgbfit224 (centre 1440x1080 crop letterboxed into 224x224, planar f16).
The library is loaded with plain ctypes from --lib, so a build from before the placement options loads too (for its legs): run one process per
library, alternating, and compare the lines by their --tag.  profiles/r15_letterbox.txt was made with

    python tools/placed_output_bench.py --lib <parent build>/libjm_amd_dec.so --tag parent --legs scale540,rgb224
    python tools/placed_output_bench.py --lib jmcodec_amd/lib/libjm_amd_dec.so --tag new --legs scale540,rgb224        (the two alternated, three times)
    python tools/placed_output_bench.py --lib jmcodec_amd/lib/libjm_amd_dec.so --tag new --legs stretch640x360,fit640   (three times)"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import streams  # noqa: E402


class RgbSpec(C.Structure):
    _fields_ = [("dtype", C.c_int), ("planar", C.c_int), ("bgr", C.c_int), ("matrix", C.c_int), ("range", C.c_int), ("scale", C.c_float * 3),
                ("bias", C.c_float * 3)]


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CROP = dict(crop_x=420, crop_y=0, crop_w=1080, crop_h=1080, target_width=224, target_height=224)
LEGS = {
    "scale540": (dict(target_width=960, target_height=540), False, (960, 540)),
    "rgb224": (CROP, True, (224, 224)),
    "stretch640x360": (dict(target_width=640, target_height=360), False, (640, 360)),
    "fit640": (dict(target_width=640, target_height=640, fit=1), False, (640, 640)),
    "rgbfit224": (dict(crop_x=240, crop_w=1440, target_width=224, target_height=224, fit=1), True, (224, 224)),
}


def run_leg(L, datas, opts, rgb, size, passes):
    S = len(datas)
    fb = size[0] * size[1] * (6 if rgb else 3) // (1 if rgb else 2)
    hs = []
    for _ in range(S):
        h = L.jm_amddec_create_handle()
        for k, v in dict(opts, profile=1).items():
            assert L.jm_amddec_set_option(h, k.encode(), v) == 0, k
        if rgb:
            s = RgbSpec(2, 1, 0, 0, 0)
            for c in range(3):
                s.scale[c], s.bias[c] = 1.0 / (255.0 * STD[c]), -MEAN[c] / STD[c]
            assert L.jm_amddec_set_rgb(h, C.byref(s)) == 0
        assert L.jm_amddec_init(0, 1, None, 0, h) == 0
        hs.append(h)
    outs = [C.create_string_buffer(fb) for _ in range(S)]
    counts = [0] * S
    aud = b"\x00\x00\x01\x09\x10"

    def feed(i, n):
        got, ln = C.c_int(0), C.c_int(0)
        k = L.jm_amddec_feed_annexb(datas[i], len(datas[i]), n, C.cast(outs[i], C.POINTER(C.c_ubyte)), fb, hs[i])
        assert k >= 0, L.jm_amddec_last_error(hs[i])
        for step in range(66):
            if step == 2:
                L.jm_amddec_set_option(hs[i], b"wait_idle", 1)
            L.jm_amddec_decode_frame(C.cast(C.c_char_p(aud), C.c_void_p), len(aud), C.byref(got), hs[i])
            if got.value != 1:
                if step < 2:
                    continue
                break
            ln.value = fb
            if L.jm_amddec_output_frame(C.cast(outs[i], C.c_void_p), C.byref(ln), hs[i]) > 0:
                k += 1
        counts[i] += k

    def everyone(n):
        ts = [threading.Thread(target=feed, args=(i, n)) for i in range(S)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    everyone(1)
    for i in range(S):
        counts[i] = 0
    cls = "rgb_pack" if rgb else "packout"
    stat = lambda k: L.jm_amddec_get_stat(hs[0], k.encode())
    ns0, p0 = stat(f"k_{cls}_ns"), stat(f"k_{cls}_pics")
    t0 = time.perf_counter()
    everyone(passes)
    dt = time.perf_counter() - t0
    ns1, p1 = stat(f"k_{cls}_ns"), stat(f"k_{cls}_pics")
    for h in hs:
        assert L.jm_amddec_get_stat(h, b"errors") == 0
        L.jm_amddec_deinit(h)
    n = sum(counts)
    return dict(frames=n, seconds=round(dt, 3), frames_per_s=round(n / dt, 1), kernel_class=cls, kernel_pics=p1 - p0,
                kernel_us_per_frame=round((ns1 - ns0) / 1000.0 / max(1, p1 - p0), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jmcodec_amd", "lib", "libjm_amd_dec.so"))
    ap.add_argument("--tag", default="new")
    ap.add_argument("--legs", default="scale540,rgb224")
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--passes", type=int, default=4)
    args = ap.parse_args()
    L = C.CDLL(args.lib)
    vp, cp = C.c_void_p, C.c_char_p
    L.jm_amddec_create_handle.restype = vp
    L.jm_amddec_set_option.argtypes = [vp, cp, C.c_longlong]
    L.jm_amddec_set_rgb.argtypes = [vp, C.POINTER(RgbSpec)]
    L.jm_amddec_init.argtypes = [C.c_int, C.c_int, cp, C.c_int, vp]
    L.jm_amddec_deinit.argtypes = [vp]
    L.jm_amddec_feed_annexb.argtypes = [cp, C.c_long, C.c_int, C.POINTER(C.c_ubyte), C.c_int, vp]
    L.jm_amddec_feed_annexb.restype = C.c_long
    L.jm_amddec_decode_frame.argtypes = [vp, C.c_int, C.POINTER(C.c_int), vp]
    L.jm_amddec_output_frame.argtypes = [vp, C.POINTER(C.c_int), vp]
    L.jm_amddec_get_stat.argtypes = [vp, cp]
    L.jm_amddec_get_stat.restype = C.c_longlong
    L.jm_amddec_last_error.argtypes = [vp]
    L.jm_amddec_last_error.restype = cp
    with ThreadPoolExecutor(16) as ex:
        datas = list(ex.map(lambda i: streams.generate(**streams.config_c1(stream_id=i, frames=args.frames)), range(args.streams)))
    for leg in args.legs.split(","):
        opts, rgb, size = LEGS[leg]
        r = run_leg(L, datas, opts, rgb, size, args.passes)
        print(json.dumps(dict(tag=args.tag, leg=leg, streams=args.streams, **r)), flush=True)


if __name__ == "__main__":
    main()
