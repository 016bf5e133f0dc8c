"""NV12 against RGB output on the bench's workload: S x 1080p H.264 streams of config C1, fed NAL by NAL through jm_amddec_feed_annexb (the
bench's hot loop) with every frame fetched, legs alternated in one process:
  a  NV12, full size (k_packout)
  b  NV12, centre 1080x1080 crop -> 224x224 (k_scale_pack)
  c  RGB planar f16 with ImageNet normalisation at b's geometry (k_rgb_pack)
  d  RGB planar u8 at 1920x1080 (k_rgb_pack, identity geometry)
and, frames left in device memory (option device_output, jm_amddec_output_frame_device): c again and RGB planar f32 at 1920x1080.
One JSON line per leg and round, then a summary line with the median frames / s per leg.

    python tools/rgb_output_bench.py [--streams 32] [--frames 30] [--passes 4] [--rounds 3] [--fit 1]

--fit 1 / 2: the 224x224 legs letterbox the centre 1440x1080 of the picture (option fit, INTEGRATION.md "Placed output": rectangle 224x168, 6.4:1 down)
instead of stretching the centre 1080x1080 -- the whole 1920x1080 picture would be 8.6:1 down into 224x126, beyond the resampler's 8:1.

Kernel times per frame: run it under rocprofv3 --kernel-trace --stats and divide the kernels' totals by the frames the legs report."""
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
LEGS = {"a_nv12_full": ({}, None, False),
        "b_nv12_224": (CROP, None, False),
        "c_rgb_f16_224": (CROP, dict(dtype="f16", **IMAGENET), False),
        "d_rgb_u8_1080p": ({}, dict(dtype="u8"), False),
        "c_rgb_f16_224_device": (CROP, dict(dtype="f16", **IMAGENET), True),
        "f32_1080p_device": ({}, dict(dtype="f32"), True)}


def run_leg(L, datas, opts, rgb, device, passes):
    """One leg: fresh handles, one warm-up pass, then `passes` timed passes of every stream on its own thread.  Returns frames / s, frames, s."""
    S = len(datas)
    hs = []
    for _ in range(S):
        h = api.jm_nvdec_create_handle()
        for k, v in dict(opts, **({"device_output": 1} if device else {})).items():
            assert L.jm_amddec_set_option(h, k.encode(), v) == 0
        if rgb is not None:
            assert api.set_rgb(h, **rgb) == 0
        if api.jm_nvdec_init(0, 1, None, 0, h) != 0:
            raise SystemExit("init failed: " + L.jm_amddec_last_error(h).decode())
        hs.append(h)
    tw, th = opts.get("target_width", 1920), opts.get("target_height", 1080)
    fb = 3 * tw * th * api.RGB_SAMPLE_BYTES[api.RGB_DTYPES[rgb["dtype"]]] if rgb else tw * th * 3 // 2
    outs = [None if device else C.create_string_buffer(fb) for _ in range(S)]
    counts = [0] * S
    aud = b"\x00\x00\x01\x09\x10"

    def take(i):
        if device:
            dev, ln = C.c_void_p(), C.c_int(0)
            return L.jm_amddec_output_frame_device(C.byref(dev), C.byref(ln), hs[i]) > 0
        ln = C.c_int(fb)
        return L.jm_amddec_output_frame(C.cast(outs[i], C.c_void_p), C.byref(ln), hs[i]) > 0

    def feed(i, n):
        got = C.c_int(0)
        out = None if device else C.cast(outs[i], C.POINTER(C.c_ubyte))
        k = L.jm_amddec_feed_annexb(datas[i], len(datas[i]), n, out, fb, hs[i])
        if k < 0:
            raise SystemExit("feed failed: " + L.jm_amddec_last_error(hs[i]).decode())
        # drain as bench.py does: access-unit delimiters close the last picture, then take what is finished
        for step in range(66):
            if step == 2:
                L.jm_amddec_set_option(hs[i], b"wait_idle", 1)
            L.jm_amddec_decode_frame(C.cast(C.c_char_p(aud), C.c_void_p), len(aud), C.byref(got), hs[i])
            if got.value != 1:
                if step < 2:
                    continue
                break
            if take(i):
                k += 1
        counts[i] += k

    def everyone(n):
        ts = [threading.Thread(target=feed, args=(i, n)) for i in range(S)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    everyone(1)
    for i in range(S):
        counts[i] = 0
    t0 = time.perf_counter()
    everyone(passes)
    dt = time.perf_counter() - t0
    for h in hs:
        assert L.jm_amddec_get_stat(h, b"errors") == 0
        assert L.jm_amddec_get_stat(h, b"out_frame_bytes") == fb
        assert (L.jm_amddec_get_stat(h, b"rgb_frames") > 0) == (rgb is not None)
        api.jm_nvdec_deinit(h)
    return sum(counts) / dt, sum(counts), dt


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of: " + ", ".join(LEGS))
    ap.add_argument("--fit", type=int, default=0, choices=(0, 1, 2), help="the 224x224 legs letterbox the centre 1440x1080 (1 centred, 2 top left)")
    args = ap.parse_args()
    L = api.lib()
    L.jm_amddec_output_frame_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]
    with ThreadPoolExecutor(16) as ex:
        datas = list(ex.map(lambda i: streams.generate(**streams.config_c1(stream_id=i, frames=args.frames)), range(args.streams)))
    names = [n for n in args.legs.split(",") if n]
    rates = {n: [] for n in names}
    for r in range(args.rounds):
        for name in names:
            opts, rgb, device = LEGS[name]
            if args.fit and opts:
                opts = dict(crop_x=240, crop_y=0, crop_w=1440, crop_h=1080, target_width=opts["target_width"], target_height=opts["target_height"], fit=args.fit)
            fps, n, dt = run_leg(L, datas, opts, rgb, device, args.passes)
            rates[name].append(fps)
            print(json.dumps({"leg": name, "round": r, "frames": n, "seconds": round(dt, 3), "frames_per_s": round(fps, 1)}), flush=True)
    med = {k: round(sorted(v)[len(v) // 2], 1) for k, v in rates.items()}
    line = {"summary": True, "streams": args.streams, "median_fps": med}
    if "b_nv12_224" in med and "c_rgb_f16_224" in med:
        line["c_over_b"] = round(med["c_rgb_f16_224"] / med["b_nv12_224"], 3)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
