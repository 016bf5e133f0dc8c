"""Picture hash verification (option verify_hash, k_hevc_pichash), measured on the device.

1. The kernel alone through jm_amddec_picture_hash_device on one 1920x1088 pitch-linear NV12 surface of noise (and on one 7680x4320 surface, where
   the launch no longer dominates): device events around REPS back-to-back calls after a warm-up, ROUNDS times.  Every call allocates its result
   words, uploads its job, clears, launches, copies six words back and waits for the stream, so a call's time holds that host work too: the kernel's
   own time comes from leg 2's profile events (k_pichash_ns over k_pichash_pics) or from running this tool under rocprofv3 --kernel-trace --stats.
   The kernel reads 1.5 w h bytes once; the line gives bytes / s over that and the share of the 8 TB/s HBM peak, and the values are checked against
   tests/pichash_ref.py first.
2. End to end: S x 1080p HEVC streams of config C3 (streams.config_c3 at 1920x1080), each stamped with the CRC of the CPU oracle's pictures
   (tools/hevc_hash_sei.py), fed through jm_amddec_feed_annexb with the frames left in device memory, every frame taken.  Legs, alternated ROUNDS
   times in this process: "plain" the unstamped streams, "off" the stamped streams with verify_hash 0, "on" with verify_hash 1.  One JSON line
   per leg and round, then a summary: median frames / s per leg, the spread of "plain" (max - min over median), on / off, and the kernel's time per
   hashed picture from the engine's events.

    python tools/pichash_bench.py [--reps 200] [--rounds 5] [--warmup 20] [--streams 8] [--frames 16] [--passes 6] [--cache DIR] [--no-kernel] [--no-streams]

--cache DIR keeps the generated and stamped streams (the generator and the oracle take about half a minute of CPU per 1080p stream)."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
from jmcodec_amd import api  # noqa: E402
from tools import hevc_hash_sei, streams  # noqa: E402
import pichash_ref as ref  # noqa: E402

HBM_PEAK = 8.0e12           # bytes / s (specification)


def kernel_leg(args):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    try:
        for w, h in ((1920, 1088), (7680, 4320)):
            rng = np.random.default_rng(w)
            planes = (rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8))
            pitch = (w + 255) // 256 * 256
            surf, chroma_offset = ref.surface(planes, pitch)
            d = C.c_void_p()
            assert hip.hipMalloc(C.byref(d), surf.size) == 0
            try:
                assert hip.hipMemcpy(d, surf.ctypes.data_as(C.c_void_p), surf.size, 1) == 0
                rc, crc, chk = api.picture_hash_device(d, pitch, chroma_offset, w, h)
                assert rc == 0 and crc == ref.picture_hash(planes, ref.CRC) and chk == ref.picture_hash(planes, ref.CHECKSUM), "device and reference differ"
                times = []
                for _ in range(args.rounds):
                    for _ in range(args.warmup):
                        api.picture_hash_device(d, pitch, chroma_offset, w, h)
                    assert hip.hipEventRecord(e0, None) == 0
                    for _ in range(args.reps):
                        api.picture_hash_device(d, pitch, chroma_offset, w, h)
                    assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
                    ms = C.c_float(0)
                    assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                    times.append(ms.value * 1e3 / args.reps)
                xs = sorted(times)
                med, nbytes = xs[len(xs) // 2], w * h * 3 // 2
                print(json.dumps(dict(leg="call", width=w, height=h, reps=args.reps, rounds=args.rounds, us_per_call_median=round(med, 3),
                                      us_per_call_min=round(xs[0], 3), us_per_call_max=round(xs[-1], 3), alg_bytes=nbytes,
                                      gb_per_s=round(nbytes / med / 1e3, 1), share_of_hbm_peak=round(nbytes / (med * 1e-6) / HBM_PEAK, 4))), flush=True)
            finally:
                hip.hipFree(d)
    finally:
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)


def make_streams(args):
    """[(plain, stamped)] per stream, from the cache when it holds them."""
    def one(i):
        path = os.path.join(args.cache, f"c3_1080p_{args.frames}f_{i}.npz") if args.cache else None
        if path and os.path.exists(path):
            z = np.load(path)
            return z["plain"].tobytes(), z["stamped"].tobytes()
        plain = streams.generate_hevc(**streams.config_c3(frames=args.frames, width=1920, height=1080, stream_id=i))
        planes, _ = ref.oracle_pictures(plain)
        stamped = hevc_hash_sei.stamp(plain, planes, ref.CRC)
        if path:
            os.makedirs(args.cache, exist_ok=True)
            np.savez(path, plain=np.frombuffer(plain, np.uint8), stamped=np.frombuffer(stamped, np.uint8))
        return plain, stamped
    with ThreadPoolExecutor(min(16, args.streams)) as ex:
        return list(ex.map(one, range(args.streams)))


def run_leg(L, datas, verify, passes):
    """Fresh handles, one warm-up pass, then `passes` timed passes of every stream on its own thread.  (frames / s, frames, seconds, stats)"""
    S = len(datas)
    hs = []
    for _ in range(S):
        h = api.jm_nvdec_create_handle()
        for k, v in (("device_output", 1), ("profile", 1), ("verify_hash", verify)):
            assert L.jm_amddec_set_option(h, k.encode(), v) == 0
        if api.jm_nvdec_init(1, 1, None, 0, h) != 0:
            raise SystemExit("init failed: " + L.jm_amddec_last_error(h).decode())
        hs.append(h)
    counts = [0] * S
    aud = b"\x00\x00\x01\x46\x01\x50"

    def feed(i, n):
        got, dev, ln = C.c_int(0), C.c_void_p(), C.c_int(0)
        k = L.jm_amddec_feed_annexb(datas[i], len(datas[i]), n, None, 0, hs[i])
        if k < 0:
            raise SystemExit("feed failed: " + L.jm_amddec_last_error(hs[i]).decode())
        for step in range(66):              # drain as bench.py does: an access unit delimiter closes the last picture, then take what is finished
            if step == 2:
                L.jm_amddec_set_option(hs[i], b"wait_idle", 1)
            L.jm_amddec_decode_frame(C.cast(C.c_char_p(aud), C.c_void_p), len(aud), C.byref(got), hs[i])
            if got.value != 1:
                if step < 2:
                    continue
                break
            if L.jm_amddec_output_frame_device(C.byref(dev), C.byref(ln), hs[i]) > 0:
                k += 1
        counts[i] += k

    def everyone(n):
        ts = [threading.Thread(target=feed, args=(i, n)) for i in range(S)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    stat = lambda h, k: L.jm_amddec_get_stat(h, k.encode())
    everyone(1)
    counts[:] = [0] * S
    before = {k: stat(hs[0], k) for k in ("k_pichash_ns", "k_pichash_pics", "k_pichash_n")}
    t0 = time.perf_counter()
    everyone(passes)
    dt = time.perf_counter() - t0
    st = {k: stat(hs[0], k) - v for k, v in before.items()}          # engine-wide counters
    for k in ("hash_pictures", "hash_checked", "hash_mismatch", "hash_unchecked", "errors"):
        st[k] = sum(stat(h, k) for h in hs)
    for h in hs:
        api.jm_nvdec_deinit(h)
    return sum(counts) / dt, sum(counts), dt, st


def stream_legs(args):
    L = api.lib()
    L.jm_amddec_output_frame_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]
    pairs = make_streams(args)
    legs = {"plain": ([p for p, _ in pairs], 0), "off": ([s for _, s in pairs], 0), "on": ([s for _, s in pairs], 1)}
    rates, kernel = {n: [] for n in legs}, [0, 0, 0]
    for r in range(args.rounds):
        for name, (datas, verify) in legs.items():
            fps, n, dt, st = run_leg(L, datas, verify, args.passes)
            assert st["errors"] == 0 and st["hash_mismatch"] == 0 and st["hash_unchecked"] == 0, st
            assert (st["hash_checked"] > 0) == (name == "on") and (st["hash_checked"] == st["hash_pictures"]), st
            if name == "on":
                kernel = [kernel[0] + st["k_pichash_ns"], kernel[1] + st["k_pichash_pics"], kernel[2] + st["k_pichash_n"]]
            rates[name].append(fps)
            print(json.dumps(dict(leg=name, round=r, frames=n, seconds=round(dt, 3), frames_per_s=round(fps, 1), **st)), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    print(json.dumps(dict(summary=True, streams=args.streams, frames=args.frames, passes=args.passes, rounds=args.rounds,
                          median_fps={k: round(v, 1) for k, v in med.items()},
                          plain_spread=round((max(rates["plain"]) - min(rates["plain"])) / med["plain"], 4),
                          off_over_plain=round(med["off"] / med["plain"], 4), on_over_off=round(med["on"] / med["off"], 4),
                          pichash_us_per_picture=round(kernel[0] / 1e3 / kernel[1], 3) if kernel[1] else None,
                          pichash_pictures_per_launch=round(kernel[1] / kernel[2], 2) if kernel[2] else None)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--passes", type=int, default=6)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-streams", action="store_true")
    ap.add_argument("--prepare", action="store_true", help="only generate and stamp the streams into --cache (needs no GPU)")
    args = ap.parse_args()
    if args.prepare:
        make_streams(args)
        return 0
    if not api.jm_nvdec_is_hw_support():
        raise SystemExit("no GPU: this tool measures on the device only")
    if not args.no_kernel:
        kernel_leg(args)
    if not args.no_streams:
        stream_legs(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
