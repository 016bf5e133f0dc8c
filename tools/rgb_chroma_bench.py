"""Interpolated against nearest chroma on the RGB output (option rgb_chroma): S x 1080p H.264 streams of config C1, fed NAL by NAL through
jm_amddec_feed_annexb (the bench's hot loop) with every frame fetched, the legs alternated in one process, option profile on:
  c0 / c1  RGB planar f16 with ImageNet normalisation, centre 1080x1080 crop -> 224x224, rgb_chroma 0 / 1
  d0 / d1  RGB planar u8 at 1920x1080 (identity geometry), rgb_chroma 0 / 1
One JSON line per leg and round -- frames / s, and the kernel time per frame from the engine's profile counters (k_rgb_pack_ns over k_rgb_pack_pics;
for rgb_chroma 1 also k_rgb_pack444_ns over k_rgb_pack444_pics) -- then a summary line with the medians and the ratios.

    python tools/rgb_chroma_bench.py [--streams 32] [--frames 30] [--passes 4] [--rounds 3] [--legs c0,c1,d0,d1]

The library is the one JM_AMD_DEC_LIB names (else the tree's), loaded with the handful of entry points the loop needs: a library of before the
option runs the rgb_chroma 0 legs (--legs c0,d0), which is how k_rgb_pack's time per frame is compared across builds."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jmcodec_amd import api  # noqa: E402
from tools import streams  # noqa: E402

IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
CROP = dict(crop_x=420, crop_y=0, crop_w=1080, crop_h=1080, target_width=224, target_height=224)
LEGS = {"c0": (CROP, dict(dtype="f16", **IMAGENET), 0), "c1": (CROP, dict(dtype="f16", **IMAGENET), 1),
        "d0": ({}, dict(dtype="u8"), 0), "d1": ({}, dict(dtype="u8"), 1)}
KERNELS = ("rgb_pack", "rgb_pack444")


def load():
    L = C.CDLL(api.lib_path())
    vp, cp, ip = C.c_void_p, C.c_char_p, C.POINTER(C.c_int)
    L.jm_amddec_create_handle.restype = vp
    L.jm_amddec_init.argtypes = [C.c_int, C.c_int, cp, C.c_int, vp]
    L.jm_amddec_deinit.argtypes = [vp]
    L.jm_amddec_decode_frame.argtypes = [vp, C.c_int, ip, vp]
    L.jm_amddec_output_frame.argtypes = [vp, ip, vp]
    L.jm_amddec_set_option.argtypes = [vp, cp, C.c_longlong]
    L.jm_amddec_get_stat.argtypes = [vp, cp]
    L.jm_amddec_get_stat.restype = C.c_longlong
    L.jm_amddec_last_error.argtypes = [vp]
    L.jm_amddec_last_error.restype = cp
    L.jm_amddec_set_rgb.argtypes = [vp, C.POINTER(api.RgbSpec)]
    L.jm_amddec_feed_annexb.argtypes = [cp, C.c_long, C.c_int, C.POINTER(C.c_ubyte), C.c_int, vp]
    L.jm_amddec_feed_annexb.restype = C.c_long
    return L


def run_leg(L, datas, opts, rgb, chroma, passes):
    """One leg: fresh handles, one warm-up pass, then `passes` timed passes of every stream on its own thread.  Returns frames / s, frames, and per
    kernel class (ns, frames) of the timed passes."""
    S = len(datas)
    spec = api.rgb_spec(**rgb)
    hs = []
    for _ in range(S):
        h = L.jm_amddec_create_handle()
        for k, v in dict(opts, profile=1, **({"rgb_chroma": 1} if chroma else {})).items():
            if L.jm_amddec_set_option(h, k.encode(), v) != 0:
                raise SystemExit(f"this library does not take option {k}")
        assert L.jm_amddec_set_rgb(h, C.byref(spec)) == 0
        if L.jm_amddec_init(0, 1, None, 0, h) != 0:
            raise SystemExit("init failed: " + L.jm_amddec_last_error(h).decode())
        hs.append(h)
    tw, th = opts.get("target_width", 1920), opts.get("target_height", 1080)
    fb = 3 * tw * th * api.RGB_SAMPLE_BYTES[spec.dtype]
    outs = [C.create_string_buffer(fb) for _ in range(S)]
    counts = [0] * S
    aud = b"\x00\x00\x01\x09\x10"

    def feed(i, n):
        got = C.c_int(0)
        k = L.jm_amddec_feed_annexb(datas[i], len(datas[i]), n, C.cast(outs[i], C.POINTER(C.c_ubyte)), fb, hs[i])
        if k < 0:
            raise SystemExit("feed failed: " + L.jm_amddec_last_error(hs[i]).decode())
        for step in range(66):                              # drain as bench.py does
            if step == 2:
                L.jm_amddec_set_option(hs[i], b"wait_idle", 1)
            L.jm_amddec_decode_frame(C.cast(C.c_char_p(aud), C.c_void_p), len(aud), C.byref(got), hs[i])
            if got.value != 1:
                if step < 2:
                    continue
                break
            ln = C.c_int(fb)
            if L.jm_amddec_output_frame(C.cast(outs[i], C.c_void_p), C.byref(ln), hs[i]) > 0:
                k += 1
        counts[i] += k

    def everyone(n):
        ts = [threading.Thread(target=feed, args=(i, n)) for i in range(S)]
        [t.start() for t in ts]
        [t.join() for t in ts]

    def counters():
        return {k: (L.jm_amddec_get_stat(hs[0], f"k_{k}_ns".encode()), L.jm_amddec_get_stat(hs[0], f"k_{k}_pics".encode())) for k in KERNELS}
    everyone(1)
    for i in range(S):
        counts[i] = 0
    c0 = counters()
    t0 = time.perf_counter()
    everyone(passes)
    dt = time.perf_counter() - t0
    c1 = counters()
    for h in hs:
        assert L.jm_amddec_get_stat(h, b"errors") == 0 and L.jm_amddec_get_stat(h, b"out_frame_bytes") == fb
        assert L.jm_amddec_get_stat(h, b"rgb_frames") > 0
        if chroma:
            assert L.jm_amddec_get_stat(h, b"rgb_chroma_frames") == L.jm_amddec_get_stat(h, b"rgb_frames")
        L.jm_amddec_deinit(h)
    return sum(counts) / dt, sum(counts), {k: (c1[k][0] - c0[k][0], c1[k][1] - c0[k][1]) for k in KERNELS}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of: " + ", ".join(LEGS))
    ap.add_argument("--tag", default="", help="copied into every line (which build this is)")
    args = ap.parse_args()
    L = load()
    with ThreadPoolExecutor(16) as ex:
        datas = list(ex.map(lambda i: streams.generate(**streams.config_c1(stream_id=i, frames=args.frames)), range(args.streams)))
    names = [n for n in args.legs.split(",") if n]
    fps, us = {n: [] for n in names}, {n: [] for n in names}
    for r in range(args.rounds):
        for name in names:
            opts, rgb, chroma = LEGS[name]
            rate, n, k = run_leg(L, datas, opts, rgb, chroma, args.passes)
            per = {c: round(ns / 1e3 / pics, 3) if pics > 0 else None for c, (ns, pics) in k.items()}
            fps[name].append(rate)
            us[name].append(per["rgb_pack"])
            print(json.dumps({"tag": args.tag, "leg": name, "round": r, "frames": n, "frames_per_s": round(rate, 1), "k_us_per_frame": per,
                              "k_frames": {c: pics for c, (_, pics) in k.items()}}), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    line = {"tag": args.tag, "summary": True, "streams": args.streams, "median_fps": {k: round(med(v), 1) for k, v in fps.items()},
            "k_rgb_pack_us_per_frame": {k: [min(v), med(v), max(v)] for k, v in us.items() if all(x is not None for x in v)}}
    for a, b in (("c0", "c1"), ("d0", "d1")):
        if a in fps and b in fps:
            line[f"{b}_over_{a}_fps"] = round(med(fps[b]) / med(fps[a]), 3)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
