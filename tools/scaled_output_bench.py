"""Full-size against scaled output on the bench's workload: S x 1080p H.264 streams of config C1, fed NAL by NAL through jm_amddec_feed_annexb
(the bench's hot loop) with every frame fetched into a host buffer -- once at the display size (k_packout) and once with target 960x540
(k_scale_pack), the two legs alternated in one process.  One JSON line per leg and round, then a summary line.

    python tools/scaled_output_bench.py [--streams 32] [--frames 60] [--passes 2] [--rounds 3] [--target 960x540] [--fit 1]

--fit 1 / 2: the scaled leg letterboxes the picture into the target (option fit, INTEGRATION.md "Placed output") instead of stretching it, e.g.
--target 640x640 --fit 1 beside --target 640x360.

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


def run_leg(L, datas, target, passes, W, H, fit=0):
    """One leg: fresh handles, one warm-up pass, then `passes` timed passes of every stream on its own thread.  Returns frames / s and frames."""
    S = len(datas)
    tw, th = target or (W, H)
    fb = tw * th * 3 // 2
    hs = []
    for _ in range(S):
        h = api.jm_nvdec_create_handle()
        if target:
            for k, v in (("target_width", tw), ("target_height", th)) + ((("fit", fit),) if fit else ()):
                assert L.jm_amddec_set_option(h, k.encode(), v) == 0
        if api.jm_nvdec_init(0, 1, None, 0, h) != 0:
            raise SystemExit("init failed: " + L.jm_amddec_last_error(h).decode())
        hs.append(h)
    outs = [C.create_string_buffer(fb) for _ in range(S)]
    counts = [0] * S
    aud = b"\x00\x00\x01\x09\x10"

    def feed(i, n):
        got, ln = C.c_int(0), C.c_int(0)
        k = L.jm_amddec_feed_annexb(datas[i], len(datas[i]), n, C.cast(outs[i], C.POINTER(C.c_ubyte)), fb, hs[i])
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
    t0 = time.perf_counter()
    everyone(passes)
    dt = time.perf_counter() - t0
    sizes = set()
    for h in hs:
        w, hh = api.jm_nvdec_stream_info(h)
        sizes.add((w, hh))
        assert L.jm_amddec_get_stat(h, b"errors") == 0
        api.jm_nvdec_deinit(h)
    assert sizes == {(tw, th)}, sizes
    return sum(counts) / dt, sum(counts), dt


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--target", default="960x540")
    ap.add_argument("--fit", type=int, default=0, choices=(0, 1, 2), help="letterbox into the target (1 centred, 2 top left) instead of stretching")
    args = ap.parse_args()
    tw, th = (int(x) for x in args.target.split("x"))
    L = api.lib()
    with ThreadPoolExecutor(16) as ex:
        datas = list(ex.map(lambda i: streams.generate(**streams.config_c1(stream_id=i, frames=args.frames)), range(args.streams)))
    legs = {"full": [], "scaled": []}
    for r in range(args.rounds):
        for name, target in (("full", None), ("scaled", (tw, th))):
            fps, n, dt = run_leg(L, datas, target, args.passes, 1920, 1080, args.fit if target else 0)
            legs[name].append(fps)
            print(json.dumps({"leg": name, "round": r, "target": f"{tw}x{th}" if target else "1920x1080", "fit": args.fit if target else 0, "frames": n, "seconds": round(dt, 3),
                              "frames_per_s": round(fps, 1)}), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in legs.items()}
    print(json.dumps({"summary": True, "streams": args.streams, "median_full_fps": round(med["full"], 1), "median_scaled_fps": round(med["scaled"], 1),
                      "ratio": round(med["scaled"] / med["full"], 3)}), flush=True)


if __name__ == "__main__":
    main()
