"""Deinterlaced against plain output on the bench's workload: S x 1080p H.264 streams of config C1, fed NAL by NAL through jm_amddec_feed_annexb
(the bench's hot loop), every leg once with deinterlace = 0 and once with deinterlace = MODE and deinterlace_when = 1 (so that the decode side of
the twins is identical: the streams are progressive), the twins alternated in one process.  Legs: `host` frames fetched into host buffers as NV12,
`hbm` frames left in device memory, `scaled` 960x540 fetched, `rgb` planar u8 RGB fetched.  One JSON line per leg, twin and round -- with the
engine's profile counters: k_deint and all pack-out kernels, microseconds per frame and GB/s -- then a summary line per leg.

    python tools/deint_output_bench.py [--streams 32] [--frames 60] [--passes 2] [--rounds 3] [--mode 2] [--rate 0] [--temporal] [--legs host,hbm,scaled,rgb]

--rate 1 compares field rate with frame rate instead: the twins are deinterlace = MODE with deinterlace_rate = 0 and with deinterlace_rate = 1.
Frames per second count OUTPUT frames (a field-rate handle puts out two per picture; `pictures_per_s` is the decode rate), and the pair counters
are printed: `field_rate_pairs` and k_deint's microseconds per pair.

--temporal compares the motion-adaptive deinterlacer with mode 2: the twins are deinterlace = 2 (at the --rate given) without and with
deinterlace_temporal = 1, so k_deint / k_deint2 and k_deint3 are timed side by side in one run (`deint_us_per_frame`, at field rate also
`deint_us_per_pair`; `deint_temporal_frames` says how many frames read a previous one).  Without the flag the key is never set, so the tool
also runs against a library of before the option (JM_AMD_DEC_LIB), which is how the off side is compared across builds.

The twin's k_packout time per frame is its `pack_us_per_frame` on the `host` / `hbm` legs (k_packout is the only pack-out kernel there); launch
counts: run one leg under rocprofv3 --kernel-trace --stats."""
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

W, H = 1920, 1080
LEGS = {"host": dict(), "hbm": dict(device=True), "scaled": dict(target=(960, 540)), "rgb": dict(rgb=True)}
COUNTERS = ("k_deint_ns", "k_deint_pics", "k_deint_alg_bytes", "k_deint_n", "k_packout_ns", "k_packout_pics", "k_packout_n")


def run_leg(L, datas, leg, mode, passes, parse_only=False, rate=0, temporal=0):
    """One twin of one leg: fresh handles, one warm-up pass, then `passes` timed passes of every stream on its own thread."""
    S = len(datas)
    cfg = LEGS[leg]
    tw, th = cfg.get("target") or (W, H)
    fb = tw * th * 3 if cfg.get("rgb") else tw * th * 3 // 2
    hs = []
    for _ in range(S):
        h = api.jm_nvdec_create_handle()
        opts = {"profile": 1}
        if parse_only:
            opts["parse_only"] = 1
        if cfg.get("device"):
            opts["device_output"] = 1
        if cfg.get("target"):
            opts.update(target_width=tw, target_height=th)
        if mode:
            opts.update(deinterlace=mode, deinterlace_when=1, deinterlace_rate=rate)
        if temporal:
            opts["deinterlace_temporal"] = 1
        for k, v in opts.items():
            assert L.jm_amddec_set_option(h, k.encode(), v) == 0, k
        if cfg.get("rgb"):
            assert api.set_rgb(h, "u8", planar=True) == 0
        if api.jm_nvdec_init(0, 0, None, 0, h) != 0:             # out_fmt 0: NV12
            raise SystemExit("init failed: " + L.jm_amddec_last_error(h).decode())
        hs.append(h)
    to_host = not cfg.get("device")
    outs = [C.create_string_buffer(fb) if to_host else None for _ in range(S)]
    counts = [0] * S
    aud = b"\x00\x00\x01\x09\x10"
    L.jm_amddec_output_frame_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]

    def feed(i, n):
        got, ln, dev = C.c_int(0), C.c_int(0), C.c_void_p()
        k = L.jm_amddec_feed_annexb(datas[i], len(datas[i]), n, C.cast(outs[i], C.POINTER(C.c_ubyte)) if to_host else None, fb if to_host else 0, hs[i])
        if k < 0:
            raise SystemExit("feed failed: " + L.jm_amddec_last_error(hs[i]).decode())
        # drain as bench.py does: access-unit delimiters close the last picture, then take what is finished
        for step in range(66 * (2 if rate else 1)):
            if step == 2:
                L.jm_amddec_set_option(hs[i], b"wait_idle", 1)
            L.jm_amddec_decode_frame(C.cast(C.c_char_p(aud), C.c_void_p), len(aud), C.byref(got), hs[i])
            if got.value != 1:
                if step < 2:
                    continue
                break
            ln.value = fb
            if to_host:
                if L.jm_amddec_output_frame(C.cast(outs[i], C.c_void_p), C.byref(ln), hs[i]) > 0:
                    k += 1
            elif L.jm_amddec_output_frame_device(C.byref(dev), C.byref(ln), hs[i]) > 0:
                k += 1
        counts[i] += k

    def everyone(n):
        ts = [threading.Thread(target=feed, args=(i, n)) for i in range(S)]
        [t.start() for t in ts]
        [t.join() for t in ts]

    def counters():
        return {k: L.jm_amddec_get_stat(hs[0], k.encode()) for k in COUNTERS}          # engine-wide: any handle of the device reports them
    everyone(1)
    for i in range(S):
        counts[i] = 0
    c0 = counters()
    t0 = time.perf_counter()
    everyone(passes)
    dt = time.perf_counter() - t0
    c1 = counters()
    d = {k: c1[k] - c0[k] for k in COUNTERS}
    deint_frames = pairs = temporal_frames = 0
    for h in hs:
        assert L.jm_amddec_get_stat(h, b"errors") == 0
        deint_frames += L.jm_amddec_get_stat(h, b"deint_frames")
        temporal_frames += max(0, L.jm_amddec_get_stat(h, b"deint_temporal_frames")) if temporal else 0
        pairs += max(0, L.jm_amddec_get_stat(h, b"field_rate_pairs"))
        api.jm_nvdec_deinit(h)
    n = sum(counts)
    res = {"leg": leg, "deinterlace": mode, "rate": rate, "frames": n, "seconds": round(dt, 3), "frames_per_s": round(n / dt, 1),
           "deint_frames": deint_frames, "field_rate_pairs": pairs}
    if temporal:
        res.update(temporal=1, deint_temporal_frames=temporal_frames)
    if rate:
        # (the handles' counters include the warm-up pass; the timed passes hold passes / (passes + 1) of the pairs)
        res["pictures_per_s"] = round(n / 2 / dt, 1)
    if d["k_deint_pics"] > 0:
        res.update(deint_us_per_frame=round(d["k_deint_ns"] / 1e3 / d["k_deint_pics"], 3), deint_launches=d["k_deint_n"],
                   deint_gb_per_s=round(d["k_deint_alg_bytes"] / max(1, d["k_deint_ns"]), 1))
        if rate:
            res["deint_us_per_pair"] = round(2 * d["k_deint_ns"] / 1e3 / d["k_deint_pics"], 3)       # (k_deint_pics counts a pair as two frames)
    if d["k_packout_pics"] > 0:
        # (every pack-out kernel of the launch points, k_deint included when it runs there)
        res.update(pack_us_per_frame=round(d["k_packout_ns"] / 1e3 / d["k_packout_pics"], 3), pack_launches=d["k_packout_n"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mode", type=int, default=2, choices=[1, 2])
    ap.add_argument("--rate", type=int, default=0, choices=[0, 1], help="1: the twins are frame rate and field rate of the same mode")
    ap.add_argument("--temporal", action="store_true", help="the twins are mode 2 without and with deinterlace_temporal (at the --rate given)")
    ap.add_argument("--legs", default="host,hbm,scaled,rgb")
    ap.add_argument("--parse-only", action="store_true", help="host half only (no GPU): checks the tool itself, the numbers mean nothing")
    args = ap.parse_args()
    legs = args.legs.split(",")
    assert all(l in LEGS for l in legs), legs
    L = api.lib()
    with ThreadPoolExecutor(16) as ex:
        datas = list(ex.map(lambda i: streams.generate(**streams.config_c1(stream_id=i, frames=args.frames)), range(args.streams)))
    # the twins of a leg as (deinterlace, deinterlace_rate): plain against deinterlaced, or -- --rate 1 -- frame rate against field rate
    # (or -- --temporal -- mode 2 against the motion-adaptive deinterlacer; the third entry is deinterlace_temporal)
    twins = [(args.mode, 0, 0), (args.mode, 1, 0)] if args.rate else [(0, 0, 0), (args.mode, 0, 0)]
    if args.temporal:
        assert args.mode == 2, "deinterlace_temporal acts while deinterlace is 2"
        twins = [(2, args.rate, 0), (2, args.rate, 1)]
    fps = {(l, t): [] for l in legs for t in twins}
    last = {}
    for r in range(args.rounds):
        for leg in legs:
            for t in twins:
                res = run_leg(L, datas, leg, t[0], args.passes, args.parse_only, t[1], t[2])
                res["round"] = r
                fps[(leg, t)].append(res["frames_per_s"])
                last[(leg, t)] = res
                print(json.dumps(res), flush=True)
    for leg in legs:
        med = {t: sorted(fps[(leg, t)])[len(fps[(leg, t)]) // 2] for t in twins}
        b, a = last[(leg, twins[0])], last[(leg, twins[1])]
        if args.temporal:
            key = "deint_us_per_pair" if args.rate else "deint_us_per_frame"
            out = {"summary": True, "leg": leg, "streams": args.streams, "rate": args.rate, "median_mode2_fps": med[twins[0]], "median_temporal_fps": med[twins[1]],
                   "ratio": round(med[twins[1]] / med[twins[0]], 3) if med[twins[0]] else None}
            if key in a and key in b:
                out.update({"temporal_" + key: a[key], "mode2_" + key: b[key], "temporal_over_mode2": round(a[key] / b[key], 3)})
        elif args.rate:
            out = {"summary": True, "leg": leg, "streams": args.streams, "median_frame_rate_fps": med[twins[0]], "median_field_rate_fps": med[twins[1]],
                   "ratio": round(med[twins[1]] / med[twins[0]], 3) if med[twins[0]] else None}
            if "deint_us_per_pair" in a and "deint_us_per_frame" in b:
                out.update(deint_us_per_pair=a["deint_us_per_pair"], twin_deint_us_per_frame=b["deint_us_per_frame"],
                           pair_over_two_frames=round(a["deint_us_per_pair"] / (2 * b["deint_us_per_frame"]), 3))
        else:
            out = {"summary": True, "leg": leg, "streams": args.streams, "median_plain_fps": med[twins[0]], "median_deint_fps": med[twins[1]],
                   "ratio": round(med[twins[1]] / med[twins[0]], 3) if med[twins[0]] else None}
            if "deint_us_per_frame" in a and "pack_us_per_frame" in b:
                out.update(deint_us_per_frame=a["deint_us_per_frame"], twin_pack_us_per_frame=b["pack_us_per_frame"],
                           deint_over_twin_pack=round(a["deint_us_per_frame"] / b["pack_us_per_frame"], 3))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
