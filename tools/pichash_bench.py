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

--md5 measures option verify_md5 (k_hevc_md5) instead, with the same two legs:
1. jm_amddec_picture_md5_device on the 1920x1088 noise surface (checked against hashlib first).  The kernel is three serial chains, so a call is
   milliseconds: --reps and --warmup are capped at 20 and 2.  The line adds ns per 64-byte block of the luma chain, the longest of the three (an upper
   bound: the call's host work is in it; the kernel's own time is the k_hevc_md5 row of a rocprofv3 --kernel-trace --stats run of this tool).
2. The same streams stamped with MD5.  Legs: "off" verify_hash 0, "counted" verify_hash 1 with verify_md5 0 (parsed and counted, nothing launched),
   "md5" verify_hash 1 with verify_md5 1.  The summary gives counted / off (the check that a process without verify_md5 pays nothing), md5 / off
   (the price of the option: every batch waits for its slowest chain) and the kernel's time per picture from the engine's events.

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


def md5_call(d, pitch, chroma_offset, w, h):
    return api.picture_md5_device(d, pitch, chroma_offset, w, h)


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
        reps, warmup = (min(args.reps, 20), min(args.warmup, 2)) if args.md5 else (args.reps, args.warmup)
        call = md5_call if args.md5 else api.picture_hash_device
        for w, h in ((1920, 1088),) if args.md5 else ((1920, 1088), (7680, 4320)):
            rng = np.random.default_rng(w)
            planes = (rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8))
            pitch = (w + 255) // 256 * 256
            surf, chroma_offset = ref.surface(planes, pitch)
            d = C.c_void_p()
            assert hip.hipMalloc(C.byref(d), surf.size) == 0
            try:
                assert hip.hipMemcpy(d, surf.ctypes.data_as(C.c_void_p), surf.size, 1) == 0
                if args.md5:
                    rc, digests = md5_call(d, pitch, chroma_offset, w, h)
                    assert rc == 0 and digests == ref.picture_hash(planes, ref.MD5), "device and hashlib differ"
                else:
                    rc, crc, chk = api.picture_hash_device(d, pitch, chroma_offset, w, h)
                    assert rc == 0 and crc == ref.picture_hash(planes, ref.CRC) and chk == ref.picture_hash(planes, ref.CHECKSUM), "device and reference differ"
                times = []
                for _ in range(args.rounds):
                    for _ in range(warmup):
                        call(d, pitch, chroma_offset, w, h)
                    assert hip.hipEventRecord(e0, None) == 0
                    for _ in range(reps):
                        call(d, pitch, chroma_offset, w, h)
                    assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
                    ms = C.c_float(0)
                    assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                    times.append(ms.value * 1e3 / reps)
                xs = sorted(times)
                med, nbytes = xs[len(xs) // 2], w * h * 3 // 2
                line = dict(leg="md5_call" if args.md5 else "call", width=w, height=h, reps=reps, rounds=args.rounds, us_per_call_median=round(med, 3),
                            us_per_call_min=round(xs[0], 3), us_per_call_max=round(xs[-1], 3), alg_bytes=nbytes,
                            gb_per_s=round(nbytes / med / 1e3, 1), share_of_hbm_peak=round(nbytes / (med * 1e-6) / HBM_PEAK, 4))
                if args.md5:
                    blocks = (w * h + 8) // 64 + 1            # of the luma chain, padding included
                    line.update(luma_blocks=blocks, ns_per_block_median=round(med * 1e3 / blocks, 2), ns_per_block_min=round(xs[0] * 1e3 / blocks, 2))
                print(json.dumps(line), flush=True)
            finally:
                hip.hipFree(d)
    finally:
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)


def make_streams(args):
    """[(plain, stamped)] per stream, from the cache when it holds them."""
    def one(i):
        path = os.path.join(args.cache, f"c3_1080p_{args.frames}f_{i}{'_md5' if args.md5 else ''}.npz") if args.cache else None
        if path and os.path.exists(path):
            z = np.load(path)
            return z["plain"].tobytes(), z["stamped"].tobytes()
        plain = streams.generate_hevc(**streams.config_c3(frames=args.frames, width=1920, height=1080, stream_id=i))
        planes, _ = ref.oracle_pictures(plain)
        stamped = hevc_hash_sei.stamp(plain, planes, ref.MD5 if args.md5 else ref.CRC)
        if path:
            os.makedirs(args.cache, exist_ok=True)
            np.savez(path, plain=np.frombuffer(plain, np.uint8), stamped=np.frombuffer(stamped, np.uint8))
        return plain, stamped
    with ThreadPoolExecutor(min(16, args.streams)) as ex:
        return list(ex.map(one, range(args.streams)))


def run_leg(L, datas, verify, passes, verify_md5=None):
    """Fresh handles, one warm-up pass, then `passes` timed passes of every stream on its own thread.  (frames / s, frames, seconds, stats)"""
    S = len(datas)
    hs = []
    for _ in range(S):
        h = api.jm_nvdec_create_handle()
        for k, v in (("device_output", 1), ("profile", 1), ("verify_hash", verify)) + ((("verify_md5", verify_md5),) if verify_md5 is not None else ()):
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
    before = {k: stat(hs[0], k) for k in ("k_pichash_ns", "k_pichash_pics", "k_pichash_n") + (("k_md5_ns", "k_md5_pics", "k_md5_n") if verify_md5 is not None else ())}
    t0 = time.perf_counter()
    everyone(passes)
    dt = time.perf_counter() - t0
    st = {k: stat(hs[0], k) - v for k, v in before.items()}          # engine-wide counters
    for k in ("hash_pictures", "hash_checked", "hash_mismatch", "hash_unchecked", "errors") + (("hash_md5",) if verify_md5 is not None else ()):
        st[k] = sum(stat(h, k) for h in hs)
    for h in hs:
        api.jm_nvdec_deinit(h)
    return sum(counts) / dt, sum(counts), dt, st


def md5_stream_legs(L, pairs, args):
    stamped = [s for _, s in pairs]
    legs = {"off": (0, 0), "counted": (1, 0), "md5": (1, 1)}
    rates, kernel = {n: [] for n in legs}, [0, 0, 0]
    for r in range(args.rounds):
        for name, (verify, verify_md5) in legs.items():
            fps, n, dt, st = run_leg(L, stamped, verify, args.passes, verify_md5)
            assert st["errors"] == 0 and st["hash_mismatch"] == 0 and st["hash_unchecked"] == 0, st
            assert st["hash_md5"] == st["hash_pictures"] and (st["hash_pictures"] > 0) == (name != "off"), st
            assert st["hash_checked"] == (st["hash_pictures"] if name == "md5" else 0) and st["k_pichash_n"] == 0, st
            assert (st["k_md5_n"] > 0) == (name == "md5"), st
            if name == "md5":
                kernel = [kernel[0] + st["k_md5_ns"], kernel[1] + st["k_md5_pics"], kernel[2] + st["k_md5_n"]]
            rates[name].append(fps)
            print(json.dumps(dict(leg=name, round=r, frames=n, seconds=round(dt, 3), frames_per_s=round(fps, 1), **st)), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    print(json.dumps(dict(summary=True, md5=True, streams=args.streams, frames=args.frames, passes=args.passes, rounds=args.rounds,
                          median_fps={k: round(v, 1) for k, v in med.items()},
                          off_spread=round((max(rates["off"]) - min(rates["off"])) / med["off"], 4),
                          counted_over_off=round(med["counted"] / med["off"], 4), md5_over_off=round(med["md5"] / med["off"], 4),
                          md5_us_per_picture=round(kernel[0] / 1e3 / kernel[1], 3) if kernel[1] else None,
                          md5_us_per_launch=round(kernel[0] / 1e3 / kernel[2], 3) if kernel[2] else None,
                          md5_pictures_per_launch=round(kernel[1] / kernel[2], 2) if kernel[2] else None)), flush=True)


def stream_legs(args):
    L = api.lib()
    L.jm_amddec_output_frame_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]
    pairs = make_streams(args)
    if args.md5:
        return md5_stream_legs(L, pairs, args)
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
    ap.add_argument("--md5", action="store_true", help="measure option verify_md5 (k_hevc_md5) instead of the CRC / checksum kernel")
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
