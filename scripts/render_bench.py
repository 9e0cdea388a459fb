#!/usr/bin/env python3
"""Times slam_render_views_dev (csrc/render.hip) with HIP events after one
warm-up, median of the repeats: the scene is tests/scene_ref.py's
clustered_cloud(100000) with the meshes scene.segment / scene.mesh give it and
a 100-pose trajectory, at 1000 x 1000 with the default camera; one view, and a
64-view fly-through (scene.fly) in one call.  Reports ms per view, fragments
per second, the share of the four passes (slam_render_last_stats) and the
traffic floor the passes imply: per pixel an 8-byte key cleared, 8 read and 3
written, plus the geometry read once per view, at the 6.29 TB/s a float4 copy
reaches on this part.  A last case measures the contended 64-bit atomicMin:
4096 coincident faces of about 2000 pixels at staggered depths, every fragment
aimed at the same few pixels.

    python scripts/render_bench.py --out profiles/render_bench.json

Needs a HIP device; there is no fallback.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-indoor-code_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import scene_ref as R   # noqa: E402
import slamhip          # noqa: E402
from slamhip import _lib as L   # noqa: E402
from slamhip import api, cycle, scene  # noqa: E402

CLUSTER = dict(TriangleMaxDistance=0.25, TriangleEuclidDistanceWeight=1.0, TriangleColorDistance=0.02,
               TriangleMinimumPoints=3)
COPY_BYTES_PER_S = 6.29e12
FLY_KEYS = "w" * 12 + "d" * 4 + "w" * 12 + "a" * 8 + "s" * 12 + "c" * 8 + " " * 8


def rot_y(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


class Runner:
    def __init__(self, ctx, prims, size):
        import torch
        self.torch, self.ctx, self.size = torch, ctx, size
        self.dev = torch.device("cuda", ctx.device)
        self.stream = torch.cuda.Stream(self.dev)
        self.lib = slamhip.lib()
        self.t = [torch.from_numpy(np.ascontiguousarray(a)).to(self.dev) for a in prims]
        self.cam = np.asarray(api.renderCamera(size), np.float64)
        torch.cuda.synchronize(self.dev)

    def run(self, views, repeats, mode=L.RENDER_AUTO):
        torch = self.torch
        w, h = self.size
        vw = api._views(views)
        out = torch.empty((len(vw), h, w, 3), dtype=torch.uint8, device=self.dev)
        pts, cols, faces, lines, lcols = self.t
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None

        def launch():
            L.check(self.lib.slam_render_views_dev(self.ctx.handle, ctypes.c_void_p(self.stream.cuda_stream), p(pts), p(cols),
                                                   len(pts), p(faces), len(faces), p(lines), p(lcols), len(lines), L.ptr(vw),
                                                   len(vw), L.ptr(self.cam), w, h, 1, p(out), None, None, 0, mode),
                    self.ctx.handle)

        t0 = time.perf_counter()
        launch()
        warm_s = time.perf_counter() - t0
        ms, passes = [], []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(self.stream)
            launch()
            b.record(self.stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
            passes.append(list(api.renderStats(self.ctx)[1].values()))
        stats = api.renderStats(self.ctx)[0]
        med = float(np.median(ms))
        pm = np.median(np.array(passes), 0)
        geometry = 15 * len(pts) + 12 * len(faces) + 27 * len(lines)
        floor_ms = len(vw) * (w * h * 19 + geometry) / COPY_BYTES_PER_S * 1e3
        return {"views": len(vw), "repeats": repeats, "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                "warmup_s": warm_s, "ms_per_view": med / len(vw), **stats,
                "fragments_per_s": stats["fragments"] / (med * 1e-3),
                "pass_ms": dict(zip(("clear", "points_lines", "faces", "resolve"), pm.tolist())),
                "pass_share": dict(zip(("clear", "points_lines", "faces", "resolve"), (pm / max(pm.sum(), 1e-12)).tolist())),
                "passes_ms_sum": float(pm.sum()), "traffic_floor_ms": floor_ms, "times_the_floor": med / floor_ms,
                "drawn_fraction": float((out != 255).any(-1).float().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    args = ap.parse_args()
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("render_bench needs a HIP device")
    ctx = slamhip.Context(0)
    pts, cols = R.clustered_cloud(args.cloud)
    gd = cycle.GlobalData()
    gd.push_points(pts.astype(np.float64), cols)
    ang = np.linspace(0, 2 * np.pi, 100, endpoint=False)
    gd.cameraRotations = [rot_y(a) for a in ang]
    gd.spatialCameraPositions = [np.array([4 * math.sin(a), 0.5 * math.sin(3 * a), 4 * math.cos(a)]).reshape(3, 1) for a in ang]
    cfg = slamhip.reference_example()
    cfg.update(CLUSTER)
    t0 = time.perf_counter()
    meshes = scene.mesh(scene.segment(gd, slamhip.ConfigService(cfg), ctx=ctx), ctx=ctx)
    prep_s = time.perf_counter() - t0
    prims = scene.scene_primitives(gd, meshes)
    size = (1000, 1000)
    run = Runner(ctx, prims, size)
    start = (rot_y(math.pi), np.array([0.0, 0.0, 12.0]))              # in front of the cloud, looking back at it
    fly = scene.fly(start, FLY_KEYS)
    result = {"entry": "slam_render_views_dev, HIP events around the call (it returns when the work is done), one warm-up",
              "scene": {"cloud": f"tests/scene_ref.py clustered_cloud({args.cloud}), clustered with {CLUSTER}",
                        "points": len(prims[0]), "faces": len(prims[2]), "meshes": sum(m is not None for m in meshes),
                        "lines": len(prims[3]), "size": list(size), "segment_and_mesh_s": prep_s},
              "floor": "per view: w * h * (8 cleared + 8 read + 3 written) + 15 B per point + 12 B per face + 27 B per line, "
                       f"at {COPY_BYTES_PER_S / 1e12} TB/s"}
    result["one_view"] = run.run([start], args.repeats)
    print(json.dumps(result["one_view"]), flush=True)
    result["fly_64"] = run.run(fly, args.repeats)
    print(json.dumps(result["fly_64"]), flush=True)
    result["fly_64_thread_per_face"] = run.run(fly, 3, L.RENDER_THREAD)
    result["fly_64_wave_per_tile"] = run.run(fly, 3, L.RENDER_WAVE)

    # contended atomicMin: coincident faces, depth staggered so that later faces are nearer
    n = 4096
    tri = np.array([[-0.35, -0.3, 0], [0.4, -0.25, 0], [0.0, 0.45, 0]])
    cpts = np.concatenate([tri + [0, 0, 6 - 1e-3 * i] for i in range(n)]).astype(np.float32)
    cprims = (cpts, np.full((3 * n, 3), 128, np.uint8), np.arange(3 * n, dtype=np.int32).reshape(n, 3),
              np.zeros((0, 6), np.float32), np.zeros((0, 3), np.uint8))
    crun = Runner(ctx, cprims, size)
    for mode, name in ((L.RENDER_THREAD, "contended_thread_per_face"), (L.RENDER_WAVE, "contended_wave_per_tile")):
        r = crun.run([(np.eye(3), np.zeros(3))], args.repeats, mode)
        r["fragments_per_s_in_the_face_pass"] = r["fragments"] / max(r["pass_ms"]["faces"] * 1e-3, 1e-12)
        result[name] = r
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
