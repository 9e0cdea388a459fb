#!/usr/bin/env python3
"""Times global bundle adjustment (csrc/gba.hip) with device events on the stream the call runs on, after a
warm-up, and the host twin beside it with a wall clock.  Reported, not gated.

The problem is generated at the size of a long indoor run: `--keyframes` cameras on a walk along x, each seeing
`--obs` points, every point tracked through `--track` consecutive keyframes (so points = keyframes * obs / track).
The defaults, 2 000 keyframes x 2 000 observations x 8, are what a run of a few minutes logs with the project's
feature budget (requiredExtractedPointsCount in the thousands) and the track lengths the windowed tracker gives.

One call is timed at three settings that differ only in the work they do, all with pcg_tol = 0 so that every
allowed iteration runs: max_lm = 0 (copy in, plan, upload, one linearisation), and max_lm = L with max_pcg = A and
with max_pcg = B.  From those: the time per PCG iteration (B - A apart), the time of an LM step without its PCG
iterations, and the set-up.  Bytes per PCG iteration are what the two passes must move: the 18 doubles of Jacobian
per observation read twice, the three index lists, and the vectors once each; the rate is that over the time per
iteration, beside the HBM peak.

    python scripts/gba_bench.py --out profiles/gba_bench.json
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

import slamhip                      # noqa: E402
from slamhip import _lib as L       # noqa: E402
from slamhip import globalba as G   # noqa: E402

HBM_PEAK_TBS = 8.0                  # MI355X HBM3E, specified
K4 = np.array([600.0, 600.0, 640.0, 360.0])


def problem(rng, n, per, track):
    """cameras k centred at x = 0.1 k with small rotations, looking down +z; point p is born at keyframe b = p // (per / track)
    and seen by keyframes b .. b + track - 1 (those below n)"""
    born = per // track
    m = n * born
    b = np.arange(m) // born
    X = np.stack([0.1 * (b + track / 2) + rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(4, 6, m)], 1)
    ang = rng.normal(size=(n, 3)) * 0.02
    q = np.concatenate([np.ones((n, 1)), ang / 2], 1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = (q[:, i] for i in range(4))
    Rk = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                   2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                   2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    centre = np.stack([0.1 * np.arange(n), np.zeros(n), np.zeros(n)], 1)
    cams = np.concatenate([q, -np.einsum("nij,nj->ni", Rk, centre)], 1)      # t = -R c
    oc = (b[:, None] + np.arange(track)[None, :]).reshape(-1)
    op = np.repeat(np.arange(m), track)
    ok = oc < n
    oc, op = oc[ok].astype(np.int32), op[ok].astype(np.int32)
    w, x, y, z = (cams[oc, i] for i in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    Xc = np.einsum("nij,nj->ni", R, X[op]) + cams[oc, 4:]
    xy = np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], 1) + 0.3 * rng.normal(size=(len(oc), 2))
    xy = xy.astype(np.float32).astype(np.float64)
    cams0 = cams.copy()
    cams0[1:, 4:] += 0.01 * rng.normal(size=(n - 1, 3))
    cams0[1:, 1:4] += 0.002 * rng.normal(size=(n - 1, 3))
    cams0[:, :4] /= np.linalg.norm(cams0[:, :4], axis=1, keepdims=True)
    return cams0, X + 0.02 * rng.normal(size=X.shape), oc, op, np.ascontiguousarray(xy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gba_bench.json"))
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--obs", type=int, default=2000)
    ap.add_argument("--track", type=int, default=8)
    ap.add_argument("--lm", type=int, default=2)
    ap.add_argument("--pcg", type=int, nargs=2, default=[16, 80])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-twin", action="store_true")
    a = ap.parse_args()
    import torch
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("gba_bench needs a HIP device")
    ctx = slamhip.Context(0)
    h, lib = ctx.handle, slamhip.lib()
    rng = np.random.default_rng(1)
    cams, pts, oc, op, xy = problem(rng, a.keyframes, a.obs, a.track)
    n, m, nobs = len(cams), len(pts), len(oc)
    d0c, d0p = torch.from_numpy(cams).cuda(), torch.from_numpy(pts).cuda()
    dc, dp = d0c.clone(), d0p.clone()
    out = L.GbaSummary()
    stream = torch.cuda.current_stream()

    def call(max_lm, max_pcg):
        prm = L.GbaParams(0, 1.0, 0.1, 1e-4, max_lm, max_pcg, 0.0, 0.0)
        dc.copy_(d0c)
        dp.copy_(d0p)
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record(stream)
        L.check(lib.slam_gba_dev(h, stream.cuda_stream, L.ptr(K4), ctypes.c_void_p(dc.data_ptr()), n, ctypes.c_void_p(dp.data_ptr()), m,
                                 L.ptr(oc), L.ptr(op), L.ptr(xy), nobs, ctypes.byref(prm), ctypes.byref(out)), h)
        b_.record(stream)
        b_.synchronize()
        return a_.elapsed_time(b_), {k: getattr(out, k) for k in G.SUMMARY_FIELDS}

    settings = [(0, 0), (a.lm, a.pcg[0]), (a.lm, a.pcg[1])]
    for s in settings:
        call(*s)                                   # warm-up of every setting: code objects, the workspace
    times = {s: [] for s in settings}
    summ = {}
    for _ in range(a.repeats):                     # alternating, so drift on a shared host spreads over all three
        for s in settings:
            ms, summ[s] = call(*s)
            times[s].append(ms)
    t0, tA, tB = (min(times[s]) for s in settings)
    sA, sB = summ[settings[1]], summ[settings[2]]
    steps = max(1, sA["lm_steps"])
    it_diff = sB["pcg_iters"] - sA["pcg_iters"]
    per_it = (tB - tA) / it_diff if it_diff > 0 else float("nan")
    per_step = (tA - t0) / steps - per_it * sA["pcg_iters"] / steps
    nk = sA["kept_obs"]
    # per PCG iteration: J_c (12) + J_p (6) doubles per observation in each of the two passes, the camera and point index of
    # each pass (3 int32 per observation), w written and read (3 m), p read by both passes, lambda D, Ap, and the vector
    # kernels' x r z p Ap and the 36 doubles of each factor
    bytes_it = nk * (2 * 18 * 8 + 3 * 4) + 8 * (2 * 3 * m + 6 * n * 4) + 8 * n * (6 * 12 + 36)
    res = {"device": torch.cuda.get_device_name(0), "keyframes": n, "points": m, "observations": nobs, "kept_observations": nk,
           "track": a.track, "settings": {"lm": a.lm, "pcg": a.pcg, "pcg_tol": 0.0, "repeats": a.repeats},
           "call_ms": {f"lm{s[0]}_pcg{s[1]}": {"min": round(min(times[s]), 3), "median": round(float(np.median(times[s])), 3)} for s in settings},
           "summary": {f"lm{s[0]}_pcg{s[1]}": summ[s] for s in settings},
           "setup_and_first_linearisation_ms": round(t0, 3),
           "ms_per_pcg_iteration": round(per_it, 4),
           "ms_per_lm_step_without_pcg": round(per_step, 3),
           "ms_per_lm_step_at_first_cap": round((tA - t0) / steps, 3),
           "bytes_per_pcg_iteration": int(bytes_it),
           "tb_per_s_in_pcg": round(bytes_it / (per_it * 1e-3) / 1e12, 3) if per_it == per_it else None,
           "hbm_peak_tb_per_s": HBM_PEAK_TBS,
           "share_of_hbm_peak": round(bytes_it / (per_it * 1e-3) / 1e12 / HBM_PEAK_TBS, 3) if per_it == per_it else None}
    if not a.no_twin:
        ms, sd = call(a.lm, a.pcg[0])
        got_c, got_p = dc.cpu().numpy(), dp.cpu().numpy()
        t = time.perf_counter()
        hc, hp, hs = G.solve(K4, cams, pts, oc, op, xy, max_lm=a.lm, max_pcg=a.pcg[0], pcg_tol=0.0, cost_tol=0.0, host=True)
        res["host_twin_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        res["host_twin_setting"] = f"lm{a.lm}_pcg{a.pcg[0]}"
        res["equals_twin"] = bool(hs == sd and np.array_equal(got_c.view(np.uint64), hc.view(np.uint64))
                                  and np.array_equal(got_p.view(np.uint64), hp.view(np.uint64)))
    res["not_measured"] = ["per-kernel times and hardware counters (a profiler run)", "a solve run to convergence at this size"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
