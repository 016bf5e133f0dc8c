"""MPEG-2 decode (codec_type 4) on a many-stream workload: one 1080p group of pictures of the test encoder (tests/scripted_mpeg2.py: random
macroblocks, conforming vectors; `--kind` I = intra pictures only, IP = I P P P, IBBP = I P B B P B B in coding order), written once (or read from
`--stream`: the bit writer takes minutes at this size) and repeated `--groups` times in each of S streams; every stream on its own thread, one picture
per jm_amddec_decode_frame call, every frame fetched.  Legs, alternated in one process:
  host    frames copied into the caller's buffer (jm_amddec_output_frame)
  device  frames left in device memory (option device_output, jm_amddec_output_frame_device)
Per leg and round one JSON line: frames / s, host CPU ms per frame (process CPU time over the frames: parse threads, feeders, engine), the VLC
decode's share (stats parse_ns_i + parse_ns_p), and -- option profile -- k_mpeg2_recon's microseconds per picture and its algorithmic bytes (job
list + reference rows + 1.5 W H) against 8 TB/s.  The kernel's time per picture TYPE comes from running the three kinds: I alone, then P from the IP
run and B from the IBBP run by subtracting the shares already known (`--split`).  Then a summary line with the medians.
--device-vlc runs every leg twice, option mpeg2_device_vlc at 0 and at 1, alternating within each round on the same group, for every stream count of
`--streams` (a list: 32,1 adds the lone-stream pair), and adds upload bytes per picture and k_mpeg2_vlc's microseconds per picture; the summary then
carries min / median / max frames per second of every leg, and the option-0 leg of the same call is the reference of every figure.  A library
without the option (JM_AMD_DEC_LIB names the parent commit's) runs the option-0 legs only.
--field-pictures compares field pictures with frame pictures (option mpeg2_field_pictures 1 in every leg): the same kind of group written twice for
a 1080i sequence (progressive_sequence 0), once as frame pictures and once with every frame as two field pictures (tests/scripted_mpeg2_field.py:
field, 16x8 and dual-prime macroblocks), legs frame / field x host / device alternating within each round; `--stream` and `--write` then name the
frame-picture file and the field-picture file goes beside it with ".fields" appended.

    python tools/mpeg2_bench.py [--streams 32,1] [--groups 8] [--rounds 3] [--kind IBBP] [--stream file.m2v] [--write file.m2v] [--split] [--device-vlc]
                                [--field-pictures]
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
import scripted_mpeg2 as S  # noqa: E402
import scripted_mpeg2_field as SF  # noqa: E402
from jmcodec_amd import api  # noqa: E402

W, H = 1920, 1080
KINDS = {"I": "IIII", "IP": "IPPP", "IBBP": "IPBBPBB"}


def make_group(kind, width=W, height=H):
    """one group in coding order; progressive sequence, frame prediction only (what progressive material uses)"""
    rng = np.random.default_rng(0x4D504732)
    items = [("seq", dict(width=width, height=height, frame_rate_code=4))]
    for i, t in enumerate(KINDS[kind]):
        items.append(("pic", S.random_picture(rng, t, width, height, 1, temporal_reference=i, frame_pred_frame_dct=1, concealment_mv=0, progressive_frame=1)))
    return S.build(items)


def make_interlaced_group(kind, fields, width=W, height=H):
    """one group of a 1080i sequence in coding order: frame pictures (frame and field prediction, both DCT types), or every frame as two field
    pictures, top field first"""
    rng = np.random.default_rng(0x4D504733)
    items = [("seq", dict(width=width, height=height, frame_rate_code=4, progressive_sequence=0))]
    for i, t in enumerate(KINDS[kind]):
        if fields:
            items += [("pic", SF.random_field_picture(rng, t, width, height, s, temporal_reference=i, concealment_mv=0)) for s in (1, 2)]
        else:
            items.append(("pic", S.random_picture(rng, t, width, height, 0, temporal_reference=i, frame_pred_frame_dct=0, concealment_mv=0, progressive_frame=0)))
    return SF.build(items)


def run_leg(L, pics, S_, groups, device, device_vlc=0, field_pictures=0):
    hs = []
    for _ in range(S_):
        h = api.jm_nvdec_create_handle()
        for k, v in (dict(device_output=1) if device else {}).items():
            assert L.jm_amddec_set_option(h, k.encode(), v) == 0
        assert L.jm_amddec_set_option(h, b"profile", 1) == 0
        if device_vlc:
            assert L.jm_amddec_set_option(h, b"mpeg2_device_vlc", device_vlc) == 0
        if field_pictures:
            assert L.jm_amddec_set_option(h, b"mpeg2_field_pictures", field_pictures) == 0
        if api.jm_nvdec_init(4, 0, None, 0, h) != 0:
            raise SystemExit("init failed: " + L.jm_amddec_last_error(h).decode())
        hs.append(h)
    fb = W * H * 3 // 2
    counts = [0] * S_
    bufs = [(C.cast(C.c_char_p(p), C.c_void_p), len(p)) for p in pics]

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
            for b, ln in bufs:
                L.jm_amddec_decode_frame(b, ln, C.byref(got), hs[i])
                if got.value == 1 and take(i, out):
                    counts[i] += 1
        if last:
            while not api.jm_nvdec_is_exit(hs[i]):
                L.jm_amddec_decode_frame(None, 0, C.byref(got), hs[i])
                if got.value == 1 and take(i, out):
                    counts[i] += 1

    def everyone(n, last):
        ts = [threading.Thread(target=feed, args=(i, n, last)) for i in range(S_)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    stat = lambda h, k: L.jm_amddec_get_stat(h, k)      # noqa: E731
    everyone(2, False)                               # warm-up: surfaces, job slots, the engine's tables
    base = sum(counts)
    k0 = (stat(hs[0], b"k_mpeg2_ns"), stat(hs[0], b"k_mpeg2_pics"), stat(hs[0], b"k_mpeg2_alg_bytes"))
    v0 = (stat(hs[0], b"k_mpeg2_vlc_ns"), stat(hs[0], b"k_mpeg2_vlc_pics"))
    p0 = sum(stat(h, b"parse_ns_i") + stat(h, b"parse_ns_p") for h in hs)
    t0, c0 = time.perf_counter(), time.process_time()
    everyone(groups, True)
    dt, cpu = time.perf_counter() - t0, time.process_time() - c0
    n = sum(counts) - base
    k1 = (stat(hs[0], b"k_mpeg2_ns"), stat(hs[0], b"k_mpeg2_pics"), stat(hs[0], b"k_mpeg2_alg_bytes"))
    v1 = (stat(hs[0], b"k_mpeg2_vlc_ns"), stat(hs[0], b"k_mpeg2_vlc_pics"))
    dev_pics = sum(max(0, stat(h, b"mpeg2_dev_pictures")) for h in hs)
    p1 = sum(stat(h, b"parse_ns_i") + stat(h, b"parse_ns_p") for h in hs)
    job = stat(hs[0], b"job_bytes") / max(1, stat(hs[0], b"pictures"))
    for h in hs:
        assert stat(h, b"errors") == 0, L.jm_amddec_last_error(h).decode()
        api.jm_nvdec_deinit(h)
    kp = max(1, k1[1] - k0[1])
    k_us, k_bytes = (k1[0] - k0[0]) / kp / 1e3, (k1[2] - k0[2]) / kp
    return dict(frames=n, seconds=round(dt, 3), frames_per_s=round(n / dt, 1), host_cpu_ms_per_frame=round(1e3 * cpu / max(1, n), 3),
                vlc_ms_per_picture=round((p1 - p0) / 1e6 / max(1, S_ * groups * len(pics)), 3), k_mpeg2_recon_us_per_picture=round(k_us, 2),
                k_mpeg2_alg_bytes_per_picture=int(k_bytes), k_mpeg2_achieved_TBps=round(k_bytes / max(1e-9, k_us * 1e-6) / 1e12, 4),
                k_mpeg2_share_of_8TBps=round(k_bytes / max(1e-9, k_us * 1e-6) / 8e12, 4), job_list_bytes_per_picture=int(job),
                k_mpeg2_vlc_us_per_picture=round((v1[0] - v0[0]) / max(1, v1[1] - v0[1]) / 1e3, 2), device_vlc_pictures=int(dev_pics))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--streams", default="32", help="stream counts, comma separated")
    ap.add_argument("--device-vlc", action="store_true", help="run every leg with option mpeg2_device_vlc at 0 and at 1")
    ap.add_argument("--field-pictures", action="store_true", help="a 1080i group as frame pictures against the same kind as field pictures")
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kind", default="IBBP", choices=sorted(KINDS))
    ap.add_argument("--stream", help="read the group from this file instead of writing it")
    ap.add_argument("--write", help="write the group to this file and stop")
    ap.add_argument("--split", action="store_true", help="device leg only, one round: the kernel's time per picture for this kind")
    args = ap.parse_args()
    counts = [int(v) for v in args.streams.split(",")]
    t0 = time.perf_counter()
    if args.field_pictures:
        data = open(args.stream, "rb").read() if args.stream else make_interlaced_group(args.kind, False)
        fdata = open(args.stream + ".fields", "rb").read() if args.stream else make_interlaced_group(args.kind, True)
    else:
        data = open(args.stream, "rb").read() if args.stream else make_group(args.kind)
    if args.write:
        open(args.write, "wb").write(data)
        if args.field_pictures:
            open(args.write + ".fields", "wb").write(fdata)
        print(json.dumps({"wrote": args.write, "bytes": len(data), "seconds": round(time.perf_counter() - t0, 1)}))
        return
    pics = api.split_mpeg2_pictures(data)
    print(json.dumps({"kind": args.kind, "pictures_per_group": len(pics), "group_bytes": len(data), "prepare_seconds": round(time.perf_counter() - t0, 1)}), flush=True)
    L = api.lib()
    L.jm_amddec_output_frame_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]
    if args.split:
        print(json.dumps(dict(run_leg(L, pics, counts[0], args.groups, True), leg="device", kind=args.kind, split=True)), flush=True)
        return
    if args.field_pictures:
        fpics = api.split_mpeg2_pictures(fdata)
        legs = [(out, coded) for out in ("host", "device") for coded in ("frame", "field")]
        res = {leg: [] for leg in legs}
        for r in range(args.rounds):
            for leg in (legs if r % 2 == 0 else legs[::-1]):
                out = run_leg(L, fpics if leg[1] == "field" else pics, counts[0], args.groups, leg[0] == "device", field_pictures=1)
                out["k_mpeg2_recon_us_per_frame"] = round(out["k_mpeg2_recon_us_per_picture"] * (2 if leg[1] == "field" else 1), 2)
                res[leg].append(out)
                print(json.dumps(dict(out, leg=leg[0], pictures=leg[1], streams=counts[0], round=r, kind=args.kind)), flush=True)
        for leg, v in res.items():
            v = sorted(v, key=lambda o: o["frames_per_s"])
            print(json.dumps({"summary": True, "streams": counts[0], "kind": args.kind, "leg": leg[0], "pictures": leg[1], "frames_per_s_min": v[0]["frames_per_s"],
                              "frames_per_s_max": v[-1]["frames_per_s"], "median": v[len(v) // 2]}), flush=True)
        return
    if args.device_vlc:
        h = api.jm_nvdec_create_handle()
        has_option = L.jm_amddec_set_option(h, b"mpeg2_device_vlc", 1) == 0
        api.jm_nvdec_deinit(h)
        for S_ in counts:
            legs = [(out, v) for out in ("host", "device") for v in ((0, 1) if has_option else (0,))]
            res = {leg: [] for leg in legs}
            for r in range(args.rounds):
                for leg in (legs if r % 2 == 0 else legs[::-1]):          # alternating: neither setting always runs first
                    out = run_leg(L, pics, S_, args.groups, leg[0] == "device", leg[1])
                    res[leg].append(out)
                    print(json.dumps(dict(out, leg=leg[0], device_vlc=leg[1], streams=S_, round=r, kind=args.kind)), flush=True)
            for leg, v in res.items():
                v = sorted(v, key=lambda o: o["frames_per_s"])
                print(json.dumps({"summary": True, "streams": S_, "kind": args.kind, "leg": leg[0], "device_vlc": leg[1], "frames_per_s_min": v[0]["frames_per_s"],
                                  "frames_per_s_max": v[-1]["frames_per_s"], "median": v[len(v) // 2]}), flush=True)
        return
    res = {"host": [], "device": []}
    for r in range(args.rounds):
        for leg in ("host", "device"):
            out = run_leg(L, pics, counts[0], args.groups, leg == "device")
            res[leg].append(out)
            print(json.dumps(dict(out, leg=leg, round=r, kind=args.kind)), flush=True)
    med = {leg: sorted(v, key=lambda o: o["frames_per_s"])[len(v) // 2] for leg, v in res.items()}
    print(json.dumps({"summary": True, "streams": counts[0], "kind": args.kind, "median": med}), flush=True)


if __name__ == "__main__":
    main()
