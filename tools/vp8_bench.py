"""VP8 key-frame decode (codec_type 5) on a many-stream workload: a few 1080p key frames from the scripted writer (tests/scripted_vp8.py: random modes
and sparse random levels, normal loop filter, four token partitions; no Pillow), written once (or read from `--stream`: the Python bool encoder takes
a while at this size) and repeated `--groups` times in each of S streams; every stream on its own thread, one frame per jm_amddec_decode_frame
call, every frame fetched.  Legs, alternated in one process:
  host    frames copied into the caller's buffer (jm_amddec_output_frame)
  device  frames left in device memory (option device_output, jm_amddec_output_frame_device)
Per leg and round one JSON line: frames / s, host CPU ms per frame (process CPU time over the frames), the bool decode's share per picture (stat
parse_ns_i), and -- option profile -- microseconds per picture of k_vp8_recon and k_vp8_filter (a launch holds a batch's pictures side by side: the
launch time over its pictures) and the uploaded job-list bytes per picture.  Then a summary with min / median / max frames per second per leg.

--inter N (option vp8_inter): the group is one key frame and N inter frames from tests/scripted_vp8_inter.py (random references, vector modes, a third
of the inter macroblocks SPLITMV, sparse levels; --intra: the share of intra macroblocks in the inter frames, 0 for none).  The lines then also carry
k_vp8_inter per picture and per launch, and k_vp8_recon's pictures (the key frames and the inter frames with intra macroblocks) beside its launches.

    python tools/vp8_bench.py [--streams 32,1] [--groups 8] [--rounds 3] [--frames 4] [--inter N [--intra 0.002]] [--stream file.ivf] [--write file.ivf]
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scripted_vp8 as S  # noqa: E402
import scripted_vp8_inter as SI  # noqa: E402
import vp8_ref  # noqa: E402
from jmcodec_amd import api  # noqa: E402

W, H = 1920, 1080


def make_stream(frames, width=W, height=H):
    return vp8_ref.ivf([S.key_frame(width, height, S.random_mbs(width, height, 0x565038 + i, density=0.2), level=16, yac=36, log2_parts=2)
                        for i in range(frames)], width, height)


def make_inter_stream(n_inter, intra, width=W, height=H):
    st = SI.Stream(width, height)
    kw = dict(level=16, yac=36, log2_parts=2)
    frames = [st.key(S.random_mbs(width, height, 0x565038, density=0.2), **kw)]
    for i in range(n_inter):
        frames.append(st.inter(SI.random_inter_mbs(width, height, 0x565039 + i, intra=intra, split=0.3, density=0.1, far=0.01), refresh_golden=1 if i == 0 else 0, **kw))
    return vp8_ref.ivf(frames, width, height)


def run_leg(L, pics, S_, groups, device, inter=False):
    hs = []
    for _ in range(S_):
        h = api.jm_nvdec_create_handle()
        if device:
            assert L.jm_amddec_set_option(h, b"device_output", 1) == 0
        assert L.jm_amddec_set_option(h, b"profile", 1) == 0
        assert L.jm_amddec_set_option(h, b"vp8", 1) == 0
        if inter:
            assert L.jm_amddec_set_option(h, b"vp8_inter", 1) == 0
        if api.jm_nvdec_init(5, 0, None, 0, h) != 0:
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
    kk = (b"k_vp8_recon_ns", b"k_vp8_recon_pics", b"k_vp8_recon_n", b"k_vp8_filter_ns", b"k_vp8_filter_pics", b"k_vp8_inter_ns", b"k_vp8_inter_pics", b"k_vp8_inter_n",
          b"k_vp8_filter_n")
    everyone(2, False)                               # warm-up: surfaces, job slots, the engine's tables
    base = sum(counts)
    k0 = [stat(hs[0], k) for k in kk]
    p0 = sum(stat(h, b"parse_ns_i") for h in hs)
    t0, c0 = time.perf_counter(), time.process_time()
    everyone(groups, True)
    dt, cpu = time.perf_counter() - t0, time.process_time() - c0
    n = sum(counts) - base
    k1 = [stat(hs[0], k) for k in kk]
    p1 = sum(stat(h, b"parse_ns_i") for h in hs)
    job = stat(hs[0], b"job_bytes") / max(1, stat(hs[0], b"pictures"))
    for h in hs:
        assert stat(h, b"errors") == 0, L.jm_amddec_last_error(h).decode()
        api.jm_nvdec_deinit(h)
    d = [b - a for a, b in zip(k0, k1)]
    extra = {}
    if inter:
        extra = dict(k_vp8_inter_us_per_picture=round(d[5] / max(1, d[6]) / 1e3, 2), k_vp8_inter_us_per_launch=round(d[5] / max(1, d[7]) / 1e3, 2),
                     k_vp8_inter_pictures_per_launch=round(d[6] / max(1, d[7]), 2), k_vp8_recon_launches=d[2], k_vp8_recon_pictures=d[1],
                     k_vp8_filter_us_per_launch=round(d[3] / max(1, d[8]) / 1e3, 2))
    return dict(extra, frames=n, seconds=round(dt, 3), frames_per_s=round(n / dt, 1), host_cpu_ms_per_frame=round(1e3 * cpu / max(1, n), 3),
                bool_decode_ms_per_picture=round((p1 - p0) / 1e6 / max(1, S_ * groups * len(pics)), 3),
                k_vp8_recon_us_per_picture=round(d[0] / max(1, d[1]) / 1e3, 2), k_vp8_recon_us_per_launch=round(d[0] / max(1, d[2]) / 1e3, 2),
                pictures_per_launch=round(d[1] / max(1, d[2]), 2), k_vp8_filter_us_per_picture=round(d[3] / max(1, d[4]) / 1e3, 2),
                upload_bytes_per_picture=int(job))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--streams", default="32", help="stream counts, comma separated")
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4, help="distinct key frames in the group")
    ap.add_argument("--inter", type=int, default=0, help="option vp8_inter: the group is one key frame and this many inter frames")
    ap.add_argument("--intra", type=float, default=0.002, help="--inter: share of intra macroblocks in the inter frames")
    ap.add_argument("--stream", help="read the group from this IVF file instead of writing it")
    ap.add_argument("--write", help="write the group to this file and stop")
    args = ap.parse_args()
    t0 = time.perf_counter()
    data = open(args.stream, "rb").read() if args.stream else (make_inter_stream(args.inter, args.intra) if args.inter else make_stream(args.frames))
    if args.write:
        open(args.write, "wb").write(data)
        print(json.dumps({"wrote": args.write, "bytes": len(data), "seconds": round(time.perf_counter() - t0, 1)}))
        return
    pics = vp8_ref.split_ivf(data)
    print(json.dumps({"pictures_per_group": len(pics), "group_bytes": len(data), "prepare_seconds": round(time.perf_counter() - t0, 1)}), flush=True)
    L = api.lib()
    L.jm_amddec_output_frame_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]
    for S_ in [int(v) for v in args.streams.split(",")]:
        res = {"host": [], "device": []}
        for r in range(args.rounds):
            for leg in (("host", "device") if r % 2 == 0 else ("device", "host")):      # alternating: neither leg always runs first
                out = run_leg(L, pics, S_, args.groups, leg == "device", inter=args.inter > 0)
                res[leg].append(out)
                print(json.dumps(dict(out, leg=leg, streams=S_, round=r)), flush=True)
        for leg, v in res.items():
            v = sorted(v, key=lambda o: o["frames_per_s"])
            print(json.dumps({"summary": True, "streams": S_, "leg": leg, "frames_per_s_min": v[0]["frames_per_s"], "frames_per_s_max": v[-1]["frames_per_s"],
                              "median": v[len(v) // 2]}), flush=True)


if __name__ == "__main__":
    main()
