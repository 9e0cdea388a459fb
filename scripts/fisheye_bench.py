"""Measure the fisheye lens model beside the polynomial one:

  map build     slam_fisheye_undistort_map / slam_undistort_map at 1920 x 1080, a
                new camera every call so the cache always misses (the time
                includes the map's copy to the host, the same for both);
  frames        fisheyeUndistortBatch / undistortBatch on 16 resident 1080p BGR
                frames, map cached: the remap kernel is the same, so the
                expectation is parity at equal source footprint; each model is
                timed at unit scale (newK = K) and at half scale, and the
                polynomial model also on the fisheye case's camera;
  points        fisheyeUndistortPoints / undistortPoints on 10 000 host points.

The two models alternate within every round, so the spread between rounds of
one case is the margin a difference has to exceed.  Writes one JSON document.

    python scripts/fisheye_bench.py [--rounds 7] [--out profiles/fisheye_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-indoor-code_amd"))

W, H, NFRAMES, NPOINTS = 1920, 1080, 16, 10000
K = np.array([[1724.676, 0, 995.966], [0, 1730.482, 550.192], [0, 0, 1.0]])
BROWN = np.array([-0.21, 0.07, 0.0013, -0.0021, 0.011])
KHALF = np.array([[1724.676 / 2, 0, 960.0], [0, 1730.482 / 2, 540.0], [0, 0, 1.0]])
KF = np.array([[534.0, 0, 987.0], [0, 534.2, 615.0], [0, 0, 1.0]])     # the prototype's camera scaled to 1080p
FISH = np.array([-0.0360, 0.0053, -0.0084, 0.0018])
NEWKF = np.array([[267.0, 0, 960.0], [0, 267.1, 540.0], [0, 0, 1.0]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fisheye_bench.json"))
    a = ap.parse_args()
    import torch
    import slamhip
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("fisheye_bench needs a HIP device")
    ctx = slamhip.Context(0)
    rng = np.random.default_rng(1)
    frames = torch.from_numpy(rng.integers(0, 256, (NFRAMES, H, W, 3), dtype=np.uint8)).cuda()
    out = torch.empty_like(frames)
    pts = np.stack([rng.uniform(0, W, NPOINTS), rng.uniform(0, H, NPOINTS)], 1).astype(np.float32)
    torch.cuda.synchronize()

    def device_ms(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def host_ms(fn, reps):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t) * 1e3 / reps

    bump = [0]

    def fresh(Km):
        bump[0] += 1
        Kn = Km.copy()
        Kn[0, 2] += bump[0] * 1e-6          # a camera the cache has not seen
        return Kn

    cases = {
        "map_brown_ms": lambda: host_ms(lambda: slamhip.undistortMap(W, H, fresh(K), BROWN, ctx=ctx), 3),
        "map_fisheye_ms": lambda: host_ms(lambda: slamhip.fisheyeUndistortMap(W, H, fresh(KF), FISH, NEWKF, ctx=ctx), 3),
        "frames16_brown_ms": lambda: device_ms(lambda: slamhip.undistortBatch(frames, K, BROWN, ctx=ctx, out=out), 20),
        "frames16_fisheye_ms": lambda: device_ms(
            lambda: slamhip.fisheyeUndistortBatch(frames, KF, FISH, NEWKF, ctx=ctx, out=out), 20),
        # the remap's time follows the source footprint of the map, not the model: both models at half scale
        # (the view a fisheye frame needs to keep its field) and at unit scale
        "frames16_brown_half_ms": lambda: device_ms(lambda: slamhip.undistortBatch(frames, K, BROWN, KHALF, ctx=ctx, out=out), 20),
        "frames16_fisheye_unit_ms": lambda: device_ms(
            lambda: slamhip.fisheyeUndistortBatch(frames, KF, FISH, None, ctx=ctx, out=out), 20),
        # the polynomial model on the fisheye case's own camera (f = 534 px), so that the models differ and not the cameras
        "frames16_brown_kf_unit_ms": lambda: device_ms(lambda: slamhip.undistortBatch(frames, KF, BROWN, None, ctx=ctx, out=out), 20),
        "frames16_brown_kf_half_ms": lambda: device_ms(lambda: slamhip.undistortBatch(frames, KF, BROWN, NEWKF, ctx=ctx, out=out), 20),
        "points10k_brown_ms": lambda: host_ms(lambda: slamhip.undistortPoints(pts, K, BROWN, K, (5, 0.0), ctx=ctx), 20),
        "points10k_fisheye_ms": lambda: host_ms(
            lambda: slamhip.fisheyeUndistortPoints(pts, KF, FISH, KF, (10, 1e-8), ctx=ctx), 20),
    }
    for fn in cases.values():               # warm up every shape
        fn()
    runs = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, fn in cases.items():         # the models alternate within a round
            runs[k].append(fn())
    torch.cuda.synchronize()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "w": W, "h": H, "frames": NFRAMES,
           "points": NPOINTS}
    for k, v in runs.items():
        res[k] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
