#!/usr/bin/env python3
"""Times cv::undistortPoints on the device (csrc/undistort.hip, undist_points)
next to the frame remap it replaces in slam_main(undistort="points"), with the K
and DC of the reference's samsung-hv calibration
(tests/golden/calib_samsung_hv.xml), all in one run and in turn:

  device entry, 2.1M points   slam_undistort_points_dev over 210 x 10^4 points,
                              the keypoints of a whole 210-frame batch
  device entry, 10k points    what one search hands to geometry
  host entry, 10k points      slam_undistort_points: upload, kernel, download
                              and the host synchronise, on the host clock
  each at criteria (5, 0), OpenCV's default, and (50, 0.01), the pipeline's
  undist_remap<3>, 210 frames slam_undistort_batch over 210 resident 1920x1080
                              BGR frames, re-measured here

The points are uniform over the 1920x1080 image (seeded), so they include the
13 % beyond the fold of the lens model that leave early and the slow ones near
it; lanes of a wave leave the loop at different iterations.  Device times are
HIP events around each call on one stream, after a warm-up of every shape;
every measurement gets about --window-s of timed work, taken in rounds that
alternate over all of them.  The 10k results are checked against
tests/undistort_points_ref.py bit for bit.

Reports ms per call (median, min, max), points per second, and for the kernel
the bytes it must move (8 in, 12 out per point) over its time; it is bound by
f64 arithmetic and the divergent loop, not by those bytes.

    python scripts/undistort_points_bench.py --out profiles/undistort_points_bench.json

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

import slamhip                          # noqa: E402
import undistort_points_ref as R        # noqa: E402
from slamhip import _lib as L           # noqa: E402

CALIB = os.path.join(ROOT, "tests", "golden", "calib_samsung_hv.xml")
CRITERIA = ((5, 0.0), (50, 0.01))


def stats(ms, n=None):
    out = {"repeats": len(ms), "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}
    if n:
        out["points_per_s"] = n / (out["ms_median"] * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=210)
    ap.add_argument("--points-per-frame", type=int, default=10000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--window-s", type=float, default=0.5, help="timed work per measurement")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_points_bench.json"))
    args = ap.parse_args()
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("undistort_points_bench needs a HIP device")
    import torch
    nf, w, h = args.frames, args.width, args.height
    small, big = args.points_per_frame, args.points_per_frame * nf
    K = slamhip.load_calibration(CALIB).copy()
    D = slamhip.load_calibration(CALIB, "DC").ravel()
    K[:2] *= w / 1920.0
    Kc, Dc = np.ascontiguousarray(K.ravel()), np.ascontiguousarray(D)
    ctx = slamhip.Context(0)
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(1234)
    pts = np.stack([rng.uniform(0, w, big), rng.uniform(0, h, big)], 1).astype(np.float32)
    d_pts = torch.from_numpy(pts).to(dev)
    d_xy = torch.empty((big, 2), dtype=torch.float32, device=dev)
    d_err = torch.empty(big, dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    src = torch.randint(0, 256, (nf, h, w, 3), dtype=torch.uint8, device=dev, generator=g)
    dst = torch.empty_like(src)
    h_xy, h_err = np.empty((small, 2), np.float32), np.empty(small, np.float32)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    torch.cuda.set_stream(stream)
    lib = slamhip.lib()

    def device_entry(n, criteria):
        def call():
            L.check(lib.slam_undistort_points_dev(ctx.handle, sp, ctypes.c_void_p(d_pts.data_ptr()), 8, n, L.ptr(Kc),
                                                  L.ptr(Dc), Dc.size, L.ptr(Kc), criteria[0], criteria[1],
                                                  ctypes.c_void_p(d_xy.data_ptr()), ctypes.c_void_p(d_err.data_ptr())),
                    ctx.handle)
        return call

    def host_entry(criteria):
        def call():
            L.check(lib.slam_undistort_points(ctx.handle, L.ptr(pts), 8, small, L.ptr(Kc), L.ptr(Dc), Dc.size, L.ptr(Kc),
                                              criteria[0], criteria[1], L.ptr(h_xy), L.ptr(h_err)), ctx.handle)
        return call

    def remap():
        slamhip.undistortBatch(src, K, D, ctx=ctx, out=dst, stream=sp)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def host_ms(fn):                      # the entry synchronises before it returns
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    runs = {}                             # name -> (timer, call, points)
    for c in CRITERIA:
        tag = "%d_%g" % c
        runs["device_%d_points_%s" % (big, tag)] = (event_ms, device_entry(big, c), big)
        runs["device_%d_points_%s" % (small, tag)] = (event_ms, device_entry(small, c), small)
        runs["host_%d_points_%s" % (small, tag)] = (host_ms, host_entry(c), small)
    runs["undist_remap3_%d_frames" % nf] = (event_ms, remap, None)

    for _ in range(args.warmup):          # code objects, the map, the staging buffer
        for timer, call, _n in runs.values():
            call()
    stream.synchronize()
    probe = {name: float(np.median([timer(call) for _ in range(3)])) for name, (timer, call, _n) in runs.items()}
    want = {name: int(min(2000, max(10, args.window_s * 1e3 / max(ms, 1e-3)))) for name, ms in probe.items()}
    ms = {name: [] for name in runs}
    rounds = max(want.values())
    for r in range(rounds):               # in turn: the same neighbours and clocks for all
        for name, (timer, call, _n) in runs.items():
            if r * want[name] // rounds != (r + 1) * want[name] // rounds:
                ms[name].append(timer(call))

    # the results are the contract's
    checked = []
    for c in CRITERIA:
        device_entry(small, c)()
        stream.synchronize()
        ref = R.undistort_points(pts[:small], K, D, K, c)
        host_entry(c)()
        for name, xy, err in (("device", d_xy[:small].cpu().numpy(), d_err[:small].cpu().numpy()),
                              ("host", h_xy, h_err)):
            if not (np.array_equal(xy, ref[0], equal_nan=True) and np.array_equal(err, ref[1], equal_nan=True)):
                raise SystemExit(f"{name} entry at {c} differs from tests/undistort_points_ref.py")
        checked.append({"criteria": list(c), "valid_share": float((ref[1] <= 0.01).mean())})

    result = {
        "entries": "slam_undistort_points_dev (HIP events around each call) and slam_undistort_points (host clock, "
                   "the entry synchronises), slam_undistort_batch for the remap; measured in turn in one run",
        "camera": "tests/golden/calib_samsung_hv.xml (K, DC)", "width": w, "height": h,
        "points": "uniform over the image, seed 1234", "kernel_bytes_per_point": {"in": 8, "out": 12},
        "measurements": {name: stats(ms[name], runs[name][2]) for name in runs},
        "verified": "the first %d points of both entries equal tests/undistort_points_ref.py at both criteria" % small,
        "residual_at_most_0.01_px": checked,
    }
    big5 = result["measurements"]["device_%d_points_5_0" % big]["ms_median"]
    big50 = result["measurements"]["device_%d_points_50_0.01" % big]["ms_median"]
    rm = result["measurements"]["undist_remap3_%d_frames" % nf]["ms_median"]
    result["remap_over_points_2.1M"] = {"5_0": rm / big5, "50_0.01": rm / big50}
    result["kernel_gb_per_s_2.1M"] = {"5_0": 20 * big / (big5 * 1e-3) / 1e9, "50_0.01": 20 * big / (big50 * 1e-3) / 1e9}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
