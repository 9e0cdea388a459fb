#!/usr/bin/env python3
"""Times the tracker search (csrc/klt.hip) next to the descriptor search it can
replace, in one run on one device:

  search, 210 x 1080p     slam_klt_track_batch_dev: the previous frame's ~10k FAST
                          points tracked into 210 resident candidates of the steady
                          synthetic sequence (bench.py's configs[1] frames and FAST
                          threshold), counts only back to the host.  Reported per
                          call: the host clock around the synchronous call, and the
                          device events the library records around the pyramid
                          kernels (klt_gray_pyr for 211 frames + klt_scharr) and
                          around klt_track (slam_profile_read families 6 and 7).
  single pair             slam_klt_track_dev on two resident frames, the same points,
                          results back to the host.
  descriptor search       slam_batch_extract_match (FAST + SIFT descriptors + BF-L2 kNN
                          + ratio 0.7) over the same 210 candidates against the same
                          previous frame: GpuOps.search's device pass, with the
                          library's event times of its kernel families.

Every shape is warmed up first; the cases then alternate for about --window-s
seconds each and the medians are reported.  The bytes the pyramid kernels must
move (each BGR frame read once, each level written once and read once by the
next step) over their event time is given against the 8 TB/s HBM peak.  The
tracker's result on the first candidate is checked against tests/klt_ref.py on a
subset of the points before anything is timed.

    python scripts/klt_bench.py --out profiles/klt_bench.json

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

import klt_ref as R                     # noqa: E402
import slamhip                          # noqa: E402
from slamhip import _lib as L           # noqa: E402
from slamhip.batch import DeviceBatch   # noqa: E402

HBM_PEAK = 8.0e12
W, H = 1920, 1080
THRESHOLD = 33            # bench.py: ~10k FAST keypoints on every frame of the steady sequence
RATIO = 0.7
FAMILIES = {"fast": 0, "sift_desc": 1, "knn": 2, "sift_blur": 4, "ratio_compact": 5, "klt_pyramid": 6, "klt_track": 7}


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
    ap.add_argument("--candidates", type=int, default=210)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("klt_bench needs a HIP device")
    ctx = slamhip.Context(0)
    n = a.candidates
    seq = slamhip.synth_frames_dev(W, H, 0, n + 1, seed=1234, path=slamhip.SYNTH_STEADY, ctx=ctx)
    prev, cand = seq[0], seq[1:]
    db = DeviceBatch(ctx)
    db.extract(prev.unsqueeze(0), THRESHOLD, slamhip.SIFT_FLANN)
    kps = db.keypoints(0).copy()
    q, nq = db.export_desc(0)
    pts = np.stack([kps["x"], kps["y"]], 1).astype(np.float32)

    # ---- the device against the reference on the first candidate (every 40th point) ----
    sub = pts[::40]
    h0, h1 = prev.cpu().numpy(), cand[0].cpu().numpy()
    ref = R.track(h0, h1, sub)
    got = slamhip.calcOpticalFlowPyrLK(prev, cand[0], sub, ctx=ctx)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, ref))

    def search():
        return db.track(prev, cand, pts, counts_only=True)[3]

    def pair():
        return slamhip.calcOpticalFlowPyrLK(prev, cand[0], pts, ctx=ctx)

    def descriptors():
        return db.extract_match(cand, THRESHOLD, slamhip.SIFT_FLANN, q, nq, RATIO)[1]

    cases = {"klt_search": (search, ("klt_pyramid", "klt_track")), "klt_pair": (pair, ("klt_pyramid", "klt_track")),
             "descriptor_search": (descriptors, ("fast", "sift_blur", "sift_desc", "knn", "ratio_compact"))}
    counts = search()
    matches = descriptors()
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
            t0 = time.perf_counter()
            fn()
            call[k].append((time.perf_counter() - t0) * 1e3)
            for f in fams:
                fam[k][f].append(read_family(ctx, FAMILIES[f]))
    L.check(slamhip.lib().slam_profile_enable(ctx.handle, 0), ctx.handle)

    out = {"frame": [W, H], "candidates": n, "points": int(len(pts)), "fast_threshold": THRESHOLD,
           "window": [21, 21], "max_level": 3, "criteria": [30, 0.01]}
    for k in cases:
        out[k] = {"call": stats(call[k]), "kernels_ms_median": {f: float(np.median(v)) for f, v in fam[k].items()}}
    out["klt_search"]["status1_per_candidate"] = {"min": int(counts.min()), "median": float(np.median(counts)),
                                                  "max": int(counts.max())}
    out["descriptor_search"]["matches_per_candidate"] = {"min": int(matches.min()), "median": float(np.median(matches)),
                                                         "max": int(matches.max())}
    sizes = slamhip.kltLevelSizes(W, H, (21, 21), 3)
    px = [w * h for w, h in sizes]
    # per frame: the BGR frame read, every level written, every level but the last read by the next step
    need = (n + 1) * (3 * px[0] + sum(px) + sum(px[1:-1])) + 4 * px[0] + sum(px) * 5
    t = out["klt_search"]["kernels_ms_median"]["klt_pyramid"] * 1e-3
    out["klt_search"]["pyramid_bytes_needed"] = int(need)
    out["klt_search"]["pyramid_hbm_fraction"] = need / t / HBM_PEAK
    out["klt_search"]["ms_per_candidate"] = out["klt_search"]["call"]["ms_median"] / n
    out["descriptor_search"]["ms_per_candidate"] = out["descriptor_search"]["call"]["ms_median"] / n
    out["search_speedup_call"] = out["descriptor_search"]["call"]["ms_median"] / out["klt_search"]["call"]["ms_median"]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
