#!/usr/bin/env python3
"""Times slam_delaunay_2d_dev (csrc/delaunay.hip) with HIP events after one
warm-up: n = 2 000, 20 000 and 100 000 uniform points, and the projected
components of tests/scene_ref.py's clustered_cloud(100000) as scene.segment
produces them.  Reports the median and range of the repeats, the share of
predicates that took the exact path and the number of tie passes
(slam_delaunay_last_stats), and scipy.spatial.Delaunay (qhull) on the host of
the same machine as the only baseline there is ("not available" where scipy
does not import).  qhull is O(n log n); this kernel is O(n^2).

    python scripts/mesh_bench.py --out profiles/mesh_bench.json

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

import mesh_ref as M    # noqa: E402
import scene_ref as R   # noqa: E402
import slamhip          # noqa: E402
from slamhip import _lib as L   # noqa: E402
from slamhip import api, cycle, scene  # noqa: E402

CLUSTER = dict(TriangleMaxDistance=0.25, TriangleEuclidDistanceWeight=1.0, TriangleColorDistance=0.02,
               TriangleMinimumPoints=3)
REPEATS = {2000: 30, 20000: 10, 100000: 3}

try:
    from scipy.spatial import Delaunay as _Qhull
except ImportError:
    _Qhull = None


def qhull_seconds(xy, repeats=3):
    if _Qhull is None:
        return "not available"
    p = np.asarray(xy, np.float64)
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        try:
            _Qhull(p)
        except Exception as e:                      # qhull refuses flat input (fewer than 3 points, all collinear)
            return f"failed: {type(e).__name__}"
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


class Runner:
    def __init__(self, ctx):
        import torch
        self.torch = torch
        self.ctx = ctx
        self.dev = torch.device("cuda", ctx.device)
        self.stream = torch.cuda.Stream(self.dev)
        self.lib = slamhip.lib()

    def run(self, xy, repeats):
        """(ms per repeat, triangles (T, 3), stats) of slam_delaunay_2d_dev on xy; one warm-up first"""
        torch = self.torch
        n = len(xy)
        d_xy = torch.from_numpy(np.ascontiguousarray(xy, np.float32)).to(self.dev)
        cap = max(2 * n, 1)
        d_tris = torch.empty((cap, 3), dtype=torch.int32, device=self.dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=self.dev)

        def launch():
            L.check(self.lib.slam_delaunay_2d_dev(self.ctx.handle, ctypes.c_void_p(self.stream.cuda_stream),
                                                  ctypes.c_void_p(d_xy.data_ptr()), n,
                                                  ctypes.c_void_p(d_tris.data_ptr()), cap,
                                                  ctypes.c_void_p(d_n.data_ptr())), self.ctx.handle)

        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        launch()
        self.stream.synchronize()
        warm_s = time.perf_counter() - t0
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(self.stream)
            launch()
            b.record(self.stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        nt = int(d_n.cpu()[0])
        return ms, d_tris[:nt].cpu().numpy(), api.delaunayStats(ctx=self.ctx), warm_s


def row_of(n, ms, tris, stats, warm_s):
    pred, exact, ties = stats
    med = float(np.median(ms))
    return {"n": n, "repeats": len(ms), "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
            "warmup_s": warm_s, "triangles": int(len(tris)), "predicates": pred,
            "predicates_per_s": pred / (med * 1e-3), "exact_predicates": exact,
            "exact_fraction": exact / max(pred, 1), "tie_passes": ties}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[2000, 20000, 100000])
    ap.add_argument("--cloud", type=int, default=100000, help="clustered_cloud size for the component run (0: skip)")
    ap.add_argument("--budget-s", type=float, default=120.0, help="time a size may take, warm-up included")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    args = ap.parse_args()
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("mesh_bench needs a HIP device")
    ctx = slamhip.Context(0)
    run = Runner(ctx)
    result = {"entry": "slam_delaunay_2d_dev, HIP events around the call, one warm-up",
              "complexity": "this kernel: O(n^2) exact predicates; qhull (the baseline): O(n log n)",
              "uniform": [], "components": None}
    prev = None
    for n in args.sizes:
        repeats = REPEATS.get(n, 3)
        if prev is not None:
            expect_s = prev["ms_median"] * 1e-3 * (n / prev["n"]) ** 2       # all-pairs-class work
            repeats = max(1, min(repeats, int(args.budget_s / max(expect_s, 1e-9)) - 1))
            if expect_s * 2 > args.budget_s:
                result["uniform"].append({"n": n, "skipped": True, "expected_s_per_call": expect_s})
                print(json.dumps(result["uniform"][-1]), flush=True)
                continue
        xy = M.uniform(n, seed=n)
        ms, tris, stats, warm_s = run.run(xy, repeats)
        M.check_delaunay(xy, tris)
        row = row_of(n, ms, tris, stats, warm_s)
        row["verified"] = "check_delaunay"
        row["qhull_host_s"] = qhull_seconds(xy)
        prev = row
        result["uniform"].append(row)
        print(json.dumps(row), flush=True)

    if args.cloud:
        pts, cols = R.clustered_cloud(args.cloud)
        gd = cycle.GlobalData()
        gd.push_points(pts.astype(np.float64), cols)
        cfg = slamhip.reference_example()
        cfg.update(CLUSTER)
        segs = scene.segment(gd, slamhip.ConfigService(cfg), ctx=ctx)
        rows, total_ms, total_q, skipped = [], 0.0, 0.0, 0
        for s in segs:
            if not M.in_range(s.xy):
                skipped += 1
                continue
            ms, tris, stats, warm_s = run.run(s.xy, 1)
            r = row_of(len(s.xy), ms, tris, stats, warm_s)
            q = qhull_seconds(s.xy, 1)
            r["qhull_host_s"] = q
            rows.append(r)
            total_ms += r["ms_median"]
            if _Qhull is None:
                total_q = q
            elif not isinstance(q, str):
                total_q += q
        sizes = [r["n"] for r in rows]
        pred = sum(r["predicates"] for r in rows)
        exact = sum(r["exact_predicates"] for r in rows)
        result["components"] = {
            "cloud": f"tests/scene_ref.py clustered_cloud({args.cloud}), clustered with {CLUSTER}",
            "components": len(rows), "skipped_out_of_range": skipped,
            "points_min": int(min(sizes)), "points_median": float(np.median(sizes)), "points_max": int(max(sizes)),
            "ms_total": total_ms, "ms_largest": max(r["ms_median"] for r in rows),
            "triangles": sum(r["triangles"] for r in rows), "predicates": pred, "exact_predicates": exact,
            "exact_fraction": exact / max(pred, 1), "tie_passes": sum(r["tie_passes"] for r in rows),
            "qhull_host_s_total": total_q,
            "largest": sorted(rows, key=lambda r: -r["n"])[:5]}
        print(json.dumps({k: v for k, v in result["components"].items() if k != "largest"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
