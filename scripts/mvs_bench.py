#!/usr/bin/env python3
"""Times plane-sweep stereo (csrc/mvs.hip) with the library's own HIP events
(slam_mvs_last_timing) after one warm-up: 8 resident references at 1920 x 1080 and
960 x 540, S in {2, 4} sources, D in {64, 128} planes, radius 2, then the fuse of
the 8 maps.  Reports per-kernel times, mvs_sweep's projections per second and
an upper bound of the census bytes it gathers per second, and says which bound
the kernel sits on.

Nothing on the parent commit computes depth maps, so the baselines are this
repository's own: slam_mvs_depth_host (the host twin, up to 16 threads) on one
reference of each size, and tests/mvs_ref.py (numpy) on one small reference.

    python scripts/mvs_bench.py --out profiles/mvs_bench.json

Needs a HIP device; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-indoor-code_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mvs_ref as R          # noqa: E402
import slamhip               # noqa: E402
from slamhip import _lib as L   # noqa: E402
from slamhip import dense    # noqa: E402

TILE_W, TILE_H = 32, 16      # mvs_sweep's tile (csrc/mvs.hip)
NREF = 8
# counted in the compiled plane loop of mvs_sweep<2> (hipcc -S, gfx950): 872 instructions, 309 of them f64,
# per 8 projections (4 positions x 2 sources); the peaks are the data-sheet vector rates in lane-instructions
F64_PER_PROJECTION, INSTR_PER_PROJECTION = 309 / 8.0, 872 / 8.0
PEAK_F64_LANE_INSTR, PEAK_F32_LANE_INSTR = 39.3e12, 78.6e12


def sequence(w, h, n):
    """n frames of the synthetic sequence at w x h and a camera that slides along x with a small yaw:
    the planes span disparities of 1 .. 96 pixels at 1080p against the nearest frame"""
    frames = slamhip.synth_frames(w, h, 100, n, seed=1234)
    f = 0.9 * w
    K = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1.0]])
    rot, pos = [], []
    for i in range(n):
        a = 0.004 * i
        rot.append(np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]))
        pos.append(np.array([0.05 * i, 0.002 * i, 0.0]))
    return frames, K, rot, pos


def timing(ctx):
    ms = np.zeros(4)
    L.check(slamhip.lib().slam_mvs_last_timing(ctx.handle, L.ptr(ms)), ctx.handle)
    return ms.tolist()


def bench_size(ctx, w, h, out, repeats):
    import torch
    n = NREF + 4
    frames, K, rot, pos = sequence(w, h, n)
    dev = torch.from_numpy(frames).cuda()
    refs = list(range(2, 2 + NREF))
    for S in (2, 4):
        src = [dense.source_order(i, n, S) for i in refs]
        M = np.zeros((NREF, 4, 9))
        v = np.zeros((NREF, 4, 3))
        for m, i in enumerate(refs):
            for k, j in enumerate(src[m]):
                Mk, vk = dense.sweep_matrices(K, rot[i], pos[i], rot[j], pos[j])
                M[m, k], v[m, k] = Mk.reshape(9), vk
        for D in (64, 128):
            planes = np.tile(np.linspace(1.0 / 48, 2.0, D), (NREF, 1))
            args = (dev, refs, src, M, v, planes, 2, 80, 1)
            slamhip.planeSweepDepthBatch(*args, ctx=ctx)                 # warm-up
            cen, swp = [], []
            for _ in range(repeats):
                _, _, inv = slamhip.planeSweepDepthBatch(*args, ctx=ctx)
                t = timing(ctx)
                cen.append(t[0])
                swp.append(t[1])
            ntiles = -(-w // TILE_W) * -(-h // TILE_H)
            proj = NREF * ntiles * (TILE_W + 4) * (TILE_H + 4) * S * D       # tile + radius-2 halo, every source and plane
            useful = NREF * w * h * S * D
            med = float(np.median(swp))
            row = {"w": w, "h": h, "refs": NREF, "S": S, "D": D, "radius": 2, "repeats": repeats,
                   "distinct_frames": len({i for i in refs} | {j for s in src for j in s}),
                   "mvs_census_ms": float(np.median(cen)), "mvs_sweep_ms": med, "mvs_sweep_ms_min": float(min(swp)),
                   "mvs_sweep_ms_max": float(max(swp)), "projections": proj, "projections_window_centres": useful,
                   "projections_per_s": proj / (med * 1e-3), "gather_bytes_upper": proj * 8,
                   "gather_bytes_per_s_upper": proj * 8 / (med * 1e-3),
                   "accepted_fraction": float((inv > 0).float().mean().item())}
            if S == 2 and D == 64:                                          # the fuse of these 8 maps
                nbr = [[refs.index(j) for j in s if j in refs] for s in src]
                nM, nv = np.zeros((NREF, 4, 9)), np.zeros((NREF, 4, 3))
                B, c = np.zeros((NREF, 9)), np.zeros((NREF, 3))
                for m, i in enumerate(refs):
                    k = 0
                    for q, j in enumerate(src[m]):
                        if j in refs:
                            nM[m, k], nv[m, k] = M[m, q], v[m, q]
                            k += 1
                    Bm, cm = dense.backproject_matrices(K, rot[i], pos[i])
                    B[m], c[m] = Bm.reshape(9), cm
                fa = (dev, inv, nbr, nM, nv, B, c, 0.01, 1, 4, 2)
                slamhip.fuseDepthMaps(*fa, frame_idx=refs, ctx=ctx)
                fl, em = [], []
                for _ in range(repeats):
                    pts, _ = slamhip.fuseDepthMaps(*fa, frame_idx=refs, ctx=ctx)
                    t = timing(ctx)
                    fl.append(t[2])
                    em.append(t[3])
                row.update({"mvs_filter_count_ms": float(np.median(fl)), "mvs_emit_ms": float(np.median(em)),
                            "points_emitted": int(len(pts))})
            out.append(row)
            print(json.dumps(row), flush=True)
    # host twin: one reference, S = 2, D = 64
    i = refs[0]
    s2 = dense.source_order(i, n, 2)
    Mv = [dense.sweep_matrices(K, rot[i], pos[i], rot[j], pos[j]) for j in s2]
    Mh, vh = np.array([m.reshape(9) for m, _ in Mv]), np.array([x for _, x in Mv])
    t0 = time.perf_counter()
    host = slamhip.planeSweepDepth(frames[i], [frames[j] for j in s2], Mh, vh, np.linspace(1.0 / 48, 2.0, 64), host=True)
    host_s = time.perf_counter() - t0
    got = slamhip.planeSweepDepth(frames[i], [frames[j] for j in s2], Mh, vh, np.linspace(1.0 / 48, 2.0, 64), ctx=ctx)
    same = all(R.same_bits(a, b) for a, b in zip(host, got))
    return {"w": w, "h": h, "S": 2, "D": 64, "slam_mvs_depth_host_s_per_reference": host_s,
            "threads": min(16, os.cpu_count() or 1), "equals_device_bit_for_bit": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvs_bench.json"))
    args = ap.parse_args()
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("mvs_bench needs a HIP device")
    ctx = slamhip.Context(0)
    result = {"entry": "slam_mvs_depth_batch_dev / slam_mvs_fuse_dev; times from slam_mvs_last_timing (HIP events "
                       "around each kernel's launches), median of the repeats after one warm-up",
              "baseline_note": "nothing on the parent commit computes depth maps; the baselines are slam_mvs_depth_host "
                               "(this repository's host twin, up to 16 threads) and tests/mvs_ref.py (numpy)",
              "projections_note": "projections = references x tiles x (32 + 4) x (16 + 4) x S x D: every position of a "
                                  "tile and its radius-2 halo is projected; gather bytes are 8 per projection, an upper "
                                  "bound (invalid projections gather nothing)",
              "device": [], "host_twin": []}
    for w, h in ((1920, 1080), (960, 540)):
        result["host_twin"].append(bench_size(ctx, w, h, result["device"], args.repeats))
        print(json.dumps(result["host_twin"][-1]), flush=True)
    sc = R.general_pose(135, 240, 2, 64, 1)
    t0 = time.perf_counter()
    R.depth(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"])
    result["mvs_ref_numpy"] = {"w": 240, "h": 135, "S": 2, "D": 64, "s_per_reference": time.perf_counter() - t0}
    # which bound: compare the gather rate with the memory system and the projection rate with the f64 pipe
    top = max(result["device"], key=lambda r: r["projections_per_s"])
    f64_share = top["projections_per_s"] * F64_PER_PROJECTION / PEAK_F64_LANE_INSTR
    other_share = top["projections_per_s"] * (INSTR_PER_PROJECTION - F64_PER_PROJECTION) / PEAK_F32_LANE_INSTR
    unique = (top["S"] + 1) * 8.0 * top["w"] * top["h"] * top["refs"]       # every census map read once per reference
    result["bound"] = {
        "best_projections_per_s": top["projections_per_s"], "best_gather_bytes_per_s_upper": top["gather_bytes_per_s_upper"],
        "f64_instructions_per_projection": F64_PER_PROJECTION, "instructions_per_projection": INSTR_PER_PROJECTION,
        "f64_issue_share": f64_share, "other_issue_share": other_share,
        "census_bytes_if_read_once": unique, "census_bytes_if_read_once_per_s": unique / (top["mvs_sweep_ms"] * 1e-3),
        "statement": "instruction issue (the f64 VALU), not memory: the plane loop of mvs_sweep<2> compiles to 872 "
                     "instructions, 309 of them f64 (two IEEE divisions per projection), for 8 projections; at the measured "
                     "rate the f64 instructions alone fill f64_issue_share of the chip's f64 lane rate (39.3e12/s, half "
                     "of the 78.6 TFLOPS data-sheet figure, every f64 instruction counted as one full-rate slot although "
                     "v_rcp_f64 and the division steps are slower) and the rest other_issue_share of the f32 rate; the "
                     "gathered bytes are at most gather_bytes_per_s_upper, mostly L2 hits (neighbouring pixels read "
                     "neighbouring words), and the census maps read once are census_bytes_if_read_once_per_s, far below "
                     "HBM's 6 TB/s.  Instruction counts are read from the compiled kernel; no hardware counters were "
                     "collected and the clock under load was not measured"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
