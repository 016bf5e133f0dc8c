"""MJPEG decode (codec_type 2) on a many-stream workload: one 1080p 4:2:0 picture, encoded once with the test encoder (tests/jpeg_ref.py: noisy
levels, a few seconds), repeated `--frames` times in each of S streams; every stream on its own thread, one picture per jm_amddec_decode_frame call,
every frame fetched.  Legs, alternated in one process:
  host    frames copied into the caller's buffer (jm_amddec_output_frame)
  device  frames left in device memory (option device_output, jm_amddec_output_frame_device)
Per leg and round one JSON line: frames / s, host CPU ms per frame (process CPU time over the frames: parse threads, feeders, engine), the Huffman
decode's share (stat parse_ns_i), and -- option profile -- k_jpeg_recon's microseconds per frame and its algorithmic bytes (job list + 1.5 W H)
against 8 TB/s.  Then a summary line with the medians.
--dri N (MCUs; "row" = one MCU row) encodes the picture with a restart interval.  --device-entropy runs every leg twice, option jpeg_device_entropy
at 0 and at 1, alternating within each round on the same picture, and adds k_jpeg_entropy's microseconds per frame; the summary then carries
min / median / max frames per second of every leg, and the option-0 leg of the same call is the reference of every figure.  --streams takes a list.

    python tools/mjpeg_bench.py [--streams 32,1] [--frames 60] [--rounds 3] [--density 0.12] [--dri row] [--device-entropy]
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref  # noqa: E402
from jmcodec_amd import api  # noqa: E402

W, H = 1920, 1080


def make_picture(density, dri=0):
    rng = np.random.default_rng(0x4D4A5047)
    lv = jpeg_ref.random_levels(rng, 0x22, W, H, density=density, amp=12, dc_amp=60)
    for p in lv:                                     # natural pictures: energy falls off with frequency
        keep = (np.add.outer(np.arange(8), np.arange(8)).reshape(64) < 7)
        p *= keep[None, None, :]
    q = [[int(min(255, 4 + 3 * (k % 8 + k // 8))) for k in range(64)]] * 2
    return jpeg_ref.encode(lv, q, 0x22, W, H, dri=dri)


def run_leg(L, pic, S, frames, device, entropy=0):
    hs = []
    for _ in range(S):
        h = api.jm_nvdec_create_handle()
        for k, v in (dict(device_output=1) if device else {}).items():
            assert L.jm_amddec_set_option(h, k.encode(), v) == 0
        assert L.jm_amddec_set_option(h, b"profile", 1) == 0
        if entropy:
            assert L.jm_amddec_set_option(h, b"jpeg_device_entropy", entropy) == 0
        if api.jm_nvdec_init(2, 0, None, 0, h) != 0:
            raise SystemExit("init failed: " + L.jm_amddec_last_error(h).decode())
        hs.append(h)
    fb = (W) * (H) * 3 // 2
    counts = [0] * S
    buf = C.cast(C.c_char_p(pic), C.c_void_p)

    def take(i, out):
        if device:
            dev, ln = C.c_void_p(), C.c_int(0)
            return L.jm_amddec_output_frame_device(C.byref(dev), C.byref(ln), hs[i]) > 0
        ln = C.c_int(fb)
        return L.jm_amddec_output_frame(C.cast(out, C.c_void_p), C.byref(ln), hs[i]) > 0

    def feed(i, n, last):
        out = None if device else C.create_string_buffer(fb)
        got = C.c_int(0)
        for _ in range(n):
            L.jm_amddec_decode_frame(buf, len(pic), C.byref(got), hs[i])
            if got.value == 1 and take(i, out):
                counts[i] += 1
        if last:
            while not api.jm_nvdec_is_exit(hs[i]):
                L.jm_amddec_decode_frame(None, 0, C.byref(got), hs[i])
                if got.value == 1 and take(i, out):
                    counts[i] += 1

    def everyone(n, last):
        ts = [threading.Thread(target=feed, args=(i, n, last)) for i in range(S)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    everyone(8, False)                               # warm-up: surfaces, job slots, the engine's tables
    base = sum(counts)
    k0 = (L.jm_amddec_get_stat(hs[0], b"k_jpeg_ns"), L.jm_amddec_get_stat(hs[0], b"k_jpeg_pics"), L.jm_amddec_get_stat(hs[0], b"k_jpeg_alg_bytes"))
    e0 = (L.jm_amddec_get_stat(hs[0], b"k_jpeg_entropy_ns"), L.jm_amddec_get_stat(hs[0], b"k_jpeg_entropy_pics"))
    p0 = sum(L.jm_amddec_get_stat(h, b"parse_ns_i") for h in hs)
    t0, c0 = time.perf_counter(), time.process_time()
    everyone(frames, True)
    dt, cpu = time.perf_counter() - t0, time.process_time() - c0
    n = sum(counts) - base
    k1 = (L.jm_amddec_get_stat(hs[0], b"k_jpeg_ns"), L.jm_amddec_get_stat(hs[0], b"k_jpeg_pics"), L.jm_amddec_get_stat(hs[0], b"k_jpeg_alg_bytes"))
    e1 = (L.jm_amddec_get_stat(hs[0], b"k_jpeg_entropy_ns"), L.jm_amddec_get_stat(hs[0], b"k_jpeg_entropy_pics"))
    p1 = sum(L.jm_amddec_get_stat(h, b"parse_ns_i") for h in hs)
    dev_pics = sum(L.jm_amddec_get_stat(h, b"jpeg_dev_pictures") for h in hs)
    job = L.jm_amddec_get_stat(hs[0], b"job_bytes") / max(1, L.jm_amddec_get_stat(hs[0], b"pictures"))
    for h in hs:
        assert L.jm_amddec_get_stat(h, b"errors") == 0
        api.jm_nvdec_deinit(h)
    kp = max(1, k1[1] - k0[1])
    k_us, k_bytes = (k1[0] - k0[0]) / kp / 1e3, (k1[2] - k0[2]) / kp
    return dict(frames=n, seconds=round(dt, 3), frames_per_s=round(n / dt, 1), host_cpu_ms_per_frame=round(1e3 * cpu / max(1, n), 3),
                huffman_ms_per_frame=round((p1 - p0) / 1e6 / max(1, S * frames), 3), k_jpeg_recon_us_per_frame=round(k_us, 2),
                k_jpeg_alg_bytes_per_frame=int(k_bytes), k_jpeg_share_of_8TBps=round(k_bytes / max(1e-9, k_us * 1e-6) / 8e12, 4),
                job_list_bytes_per_frame=int(job), k_jpeg_entropy_us_per_frame=round((e1[0] - e0[0]) / max(1, e1[1] - e0[1]) / 1e3, 2),
                device_entropy_pictures=int(dev_pics))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--streams", default="32", help="stream counts, comma separated")
    ap.add_argument("--dri", default="0", help='restart interval in MCUs, or "row" for one MCU row')
    ap.add_argument("--device-entropy", action="store_true", help="run every leg with option jpeg_device_entropy at 0 and at 1")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.12)
    args = ap.parse_args()
    L = api.lib()
    L.jm_amddec_output_frame_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]
    t0 = time.perf_counter()
    dri = (W + 15) // 16 if args.dri == "row" else int(args.dri)
    pic = make_picture(args.density, dri)
    print(json.dumps({"picture_bytes": len(pic), "dri": dri, "encode_seconds": round(time.perf_counter() - t0, 1)}), flush=True)
    for S in [int(v) for v in args.streams.split(",")]:
        legs = [(out, ent) for out in ("host", "device") for ent in ((0, 1) if args.device_entropy else (0,))]
        res = {leg: [] for leg in legs}
        for r in range(args.rounds):
            for leg in (legs if r % 2 == 0 else legs[::-1]):          # alternating: neither setting always runs first
                out = run_leg(L, pic, S, args.frames, leg[0] == "device", leg[1])
                res[leg].append(out)
                print(json.dumps(dict(out, leg=leg[0], device_entropy=leg[1], streams=S, round=r)), flush=True)
        for leg, v in res.items():
            v = sorted(v, key=lambda o: o["frames_per_s"])
            print(json.dumps({"summary": True, "streams": S, "leg": leg[0], "device_entropy": leg[1], "frames_per_s_min": v[0]["frames_per_s"],
                              "frames_per_s_max": v[-1]["frames_per_s"], "median": v[len(v) // 2]}), flush=True)


if __name__ == "__main__":
    main()
