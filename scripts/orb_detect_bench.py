#!/usr/bin/env python3
"""Times the full ORB detector (csrc/orbdet.hip) next to the full SIFT detector,
in one run on one device:

  orb_500 / orb_10000     slam_orb_detect_batch over 16 resident 1080p synthetic
                          frames (8 levels, scale factor 1.2, FAST threshold 20,
                          Harris score) at nfeatures 500 and 10000; keypoints and
                          descriptors stay in device memory, counts come back.
                          Reported per call: the host clock around the synchronous
                          call, and the device events the library records around
                          its kernel families (slam_profile_read): the pyramid
                          (orbdet_gray + orbdet_down), FAST, the selections
                          (orbdet_select + orbdet_pack), orbdet_harris +
                          orbdet_angle, orb_blur, orb_desc and orbdet_emit.
  sift                    slam_sift_detect_batch on the same frames.

Every case is warmed up first; the cases then alternate for about --window-s
seconds each and the medians are reported.  The bytes the pyramid, FAST and blur
kernels must move (computed from the level sizes) over their event times are
given against the 8 TB/s HBM peak.  Before anything is timed, frame 0's result at
nfeatures 500 is checked against tests/orb_detect_ref.py.

    python scripts/orb_detect_bench.py --out profiles/orb_detect_bench.json

Needs a HIP device; there is no fallback.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-indoor-code_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import orb_detect_ref as R              # noqa: E402
import slamhip                          # noqa: E402
from slamhip import _lib as L           # noqa: E402

HBM_PEAK = 8.0e12
W, H = 1920, 1080
NLEVELS, SCALE, THRESHOLD = 8, 1.2, 20
ORB_FAMILIES = {"pyramid": 8, "fast_detect": 0, "select_pack": 9, "harris_angle": 10, "orb_blur": 4, "orb_desc": 3,
                "emit": 11}


def read_family(ctx, fam):
    ms, n = ctypes.c_double(0), ctypes.c_int(0)
    L.check(slamhip.lib().slam_profile_read(ctx.handle, fam, ctypes.byref(ms), ctypes.byref(n)), ctx.handle)
    return ms.value * n.value        # the call's total over the family's launches


def stats(v):
    return {"repeats": len(v), "ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v))}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=2.0)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("orb_detect_bench needs a HIP device")
    ctx = slamhip.Context(0)
    n = a.frames
    frames = slamhip.synth_frames_dev(W, H, 0, n, seed=1234, path=slamhip.SYNTH_STEADY, ctx=ctx)

    # ---- the device against the definition on frame 0 ----
    host0 = frames[0].cpu().numpy()
    rk, rd = R.detect_and_compute(host0, 500, SCALE, NLEVELS, THRESHOLD)
    gk, gd = slamhip.orbDetectAndComputeBatch(frames[:1], 500, SCALE, NLEVELS, THRESHOLD, ctx=ctx).host(0)
    assert gk.tobytes() == rk.tobytes() and np.array_equal(gd, rd)

    def orb(nf):
        return lambda: slamhip.orbDetectAndComputeBatch(frames, nf, SCALE, NLEVELS, THRESHOLD, ctx=ctx,
                                                        cap=2 * nf + 4096).counts

    def sift():
        return slamhip.siftDetectAndComputeBatch(frames, ctx=ctx).counts

    cases = {"orb_500": (orb(500), ORB_FAMILIES), "orb_10000": (orb(10000), ORB_FAMILIES), "sift": (sift, {})}
    counts = {k: fn() for k, (fn, _) in cases.items()}
    for fn, _ in cases.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    L.check(slamhip.lib().slam_profile_enable(ctx.handle, 1), ctx.handle)
    call = {k: [] for k in cases}
    fam = {k: {f: [] for f in fams} for k, (_, fams) in cases.items()}
    t_end = time.perf_counter() + a.window_s * len(cases)
    while time.perf_counter() < t_end or min(len(v) for v in call.values()) < 3:
        for k, (fn, fams) in cases.items():
            for f in range(12):
                read_family(ctx, f)          # drop what another case recorded
            t0 = time.perf_counter()
            fn()
            call[k].append((time.perf_counter() - t0) * 1e3)
            for f, idx in fams.items():
                fam[k][f].append(read_family(ctx, idx))
    L.check(slamhip.lib().slam_profile_enable(ctx.handle, 0), ctx.handle)

    sizes = [s for s in R.level_sizes(W, H, SCALE, NLEVELS) if s[0] > 62 and s[1] > 62]
    px = [w * h for w, h in sizes]
    need = {
        # each BGR frame read once, each level written once and read once by the next level's resize
        "pyramid": n * (3 * px[0] + sum(px) + sum(px[:-1])),
        # each level read once; FAST's copy of it, and its score plane's kept pixels, written
        "fast_detect": n * 2 * sum(px),
        "orb_blur": n * 2 * sum(px),
    }
    out = {"frame": [W, H], "frames": n, "nlevels": NLEVELS, "scale_factor": SCALE, "fast_threshold": THRESHOLD,
           "levels": sizes, "hbm_peak_bytes_per_s": HBM_PEAK}
    for k in cases:
        ms = call[k]
        out[k] = {"call": stats(ms), "frames_per_s": n / (float(np.median(ms)) * 1e-3),
                  "keypoints_per_frame": {"min": int(counts[k].min()), "median": float(np.median(counts[k])),
                                          "max": int(counts[k].max())}}
        if fam[k]:
            km = {f: float(np.median(v)) for f, v in fam[k].items()}
            out[k]["kernels_ms_median"] = km
            out[k]["kernels_ms_sum"] = float(sum(km.values()))
            out[k]["bytes_needed"] = {f: int(b) for f, b in need.items()}
            out[k]["hbm_fraction"] = {f: (b / (km[f] * 1e-3) / HBM_PEAK if km[f] > 0 else None)
                                      for f, b in need.items()}
    out["orb_10000_over_sift_call_time"] = out["orb_10000"]["call"]["ms_median"] / out["sift"]["call"]["ms_median"]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
