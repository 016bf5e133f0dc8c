"""Field-rate deinterlacing, kernel against kernel: one 1920x1080 pitch-linear NV12 surface (a smooth picture with combed row pairs, so that both
branches of mode 2 run) turned into its two field-rate frames by

    A  two jm_amddec_deinterlace_device calls, keep_field 1 and 2 (k_deint twice), and
    B  one jm_amddec_deinterlace2_device call (k_deint2 once).

Each variant is timed with device events around REPS back-to-back invocations after a warm-up; A and B alternate ROUNDS times in this process, for
modes 1 and 2.  Both variants' frames are compared byte for byte first.  Every invocation of either call uploads its job, launches and waits for
the stream, so a call's time holds that host work too (twice in A): the kernels' own times come from running this tool under
rocprofv3 --kernel-trace --stats.  One JSON line per mode and variant -- median and min-max of the time per frame PAIR, GB/s over the algorithmic
bytes (S = 1.5 w h: A moves 4 S in mode 2 and 3 S in mode 1, B 3 S) and the share of the HBM peak -- then the verdict: B's median may not lie above
A's by more than A's own min-max spread (exit status 1 otherwise).

    python tools/field_rate_kernel_bench.py [--reps 200] [--rounds 5] [--warmup 20]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jmcodec_amd import api  # noqa: E402

W, H, PITCH = 1920, 1080, 1920
HBM_PEAK = 8.0e12           # bytes / s (specification)


def surface(seed=1):
    """The smooth-plus-combed pattern of the stand-alone deinterlace tests."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H * 3 // 2, 0:PITCH]
    base = (96 + 60 * np.sin(x / 9.0) + 40 * np.cos(y / 7.0)).astype(np.int64)
    comb = ((y & 1) * rng.integers(0, 2, (H * 3 // 2, 1)) * 40)
    return np.clip(base + comb + rng.integers(-3, 4, base.shape), 0, 255).astype(np.uint8).reshape(-1)


def alg_bytes(variant, mode):
    s = W * H * 3 // 2
    return (4 if mode == 2 else 3) * s if variant == "A" else 3 * s


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    if hip.hipGetDeviceCount(C.byref(C.c_int(0))) != 0 or not api.jm_nvdec_is_hw_support():
        raise SystemExit("no GPU: this tool measures on the device only")
    api.lib()
    src = surface()
    fs = W * H * 3 // 2
    d_src, bufs = C.c_void_p(), [C.c_void_p() for _ in range(4)]
    assert hip.hipMalloc(C.byref(d_src), src.size) == 0
    for b in bufs:
        assert hip.hipMalloc(C.byref(b), fs) == 0
    assert hip.hipMemcpy(d_src, src.ctypes.data_as(C.c_void_p), src.size, 1) == 0
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    def variant_a(mode):
        assert api.deinterlace_device(d_src, PITCH, PITCH * H, W, H, mode, 1, bufs[0]) == 0
        assert api.deinterlace_device(d_src, PITCH, PITCH * H, W, H, mode, 2, bufs[1]) == 0

    def variant_b(mode):
        assert api.deinterlace2_device(d_src, PITCH, PITCH * H, W, H, mode, 1, bufs[2], bufs[3]) == 0

    def fetch(b):
        out = np.zeros(fs, np.uint8)
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), b, fs, 2) == 0
        return out

    def timed(fn, mode):
        for _ in range(args.warmup):
            fn(mode)
        assert hip.hipEventRecord(e0, None) == 0
        for _ in range(args.reps):
            fn(mode)
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value * 1e3 / args.reps          # microseconds per frame pair

    ok = True
    try:
        for mode in (1, 2):
            variant_a(mode)
            variant_b(mode)
            assert np.array_equal(fetch(bufs[0]), fetch(bufs[2])) and np.array_equal(fetch(bufs[1]), fetch(bufs[3])), f"mode {mode}: A and B differ"
            t = {"A": [], "B": []}
            for _ in range(args.rounds):
                t["A"].append(timed(variant_a, mode))
                t["B"].append(timed(variant_b, mode))
            res = {}
            for v in ("A", "B"):
                xs = sorted(t[v])
                med = xs[len(xs) // 2]
                res[v] = dict(mode=mode, variant=v, calls_per_pair=2 if v == "A" else 1, reps=args.reps, rounds=args.rounds,
                              us_per_pair_median=round(med, 3), us_per_pair_min=round(xs[0], 3), us_per_pair_max=round(xs[-1], 3),
                              alg_bytes=alg_bytes(v, mode), gb_per_s=round(alg_bytes(v, mode) / med / 1e3, 1),
                              share_of_hbm_peak=round(alg_bytes(v, mode) / (med * 1e-6) / HBM_PEAK, 4))
                print(json.dumps(res[v]), flush=True)
            a, b = res["A"], res["B"]
            spread = a["us_per_pair_max"] - a["us_per_pair_min"]
            good = b["us_per_pair_median"] <= a["us_per_pair_median"] + spread
            ok &= good
            print(json.dumps(dict(summary=True, mode=mode, a_median_us=a["us_per_pair_median"], b_median_us=b["us_per_pair_median"],
                                  a_spread_us=round(spread, 3), b_over_a=round(b["us_per_pair_median"] / a["us_per_pair_median"], 3),
                                  requirement_met=bool(good))), flush=True)
    finally:
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        for b in [d_src] + bufs:
            hip.hipFree(b)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
