#!/usr/bin/env python3
"""Times place recognition (csrc/place.hip) with device events on the stream the
kernels run on, after a warm-up of every shape:

  training    200 keyframes x 10 000 SIFT-like descriptors at K = 4096, 10 iterations:
              total and per iteration, and one assign pass on its own (the rest of
              an iteration is the counting-sort update)
  quantising  one keyframe (10 000 descriptors) against the 4096 words, SIFT and ORB
  scoring     one query, and a batch of 8, against 10 000 database rows

Beside each number stands the bound it is measured against: voc_assign against the
int8 MFMA rate (2 x 2.5e15 ops/s, MI355X data sheet) and against slam_knn2 run as a
top-2 search over the same centroids (the parent's nearest equivalent; both as
host-buffer calls, copies included); bow_score against HBM bandwidth (8.0 TB/s data
sheet, 6.29 TB/s measured by a float4 copy).

    python scripts/place_bench.py --out profiles/place_bench.json

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

import slamhip               # noqa: E402
from slamhip import _lib as L   # noqa: E402
from slamhip import place    # noqa: E402

PEAK_I8_MAC = 2.5e15         # MAC/s: twice the ~2.5 PFLOP/s dense BF16 rate, one MAC = 2 ops
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def sift_like(torch, n, seed):
    """n descriptors shaped like SIFT's: non-negative, L2 norm 512, rounded, at most 255"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((n, 128), generator=g, device="cuda") ** 3
    x = x * (512.0 / x.norm(dim=1, keepdim=True))
    return x.round().clamp_(0, 255).to(torch.uint8)


def timed(torch, fn, repeats):
    """device-event times (ms) of fn(stream) on torch's current stream"""
    s = torch.cuda.current_stream()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn(s.cuda_stream)
        b.record(s)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stat(ms):
    return {"ms_min": round(min(ms), 4), "ms_median": round(float(np.median(ms)), 4), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_bench.json"))
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--per-frame", type=int, default=10000)
    ap.add_argument("--words", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("place_bench needs a HIP device")
    ctx = slamhip.Context(0)
    h, lib = ctx.handle, slamhip.lib()
    K, n1, N = a.words, a.per_frame, a.frames * a.per_frame
    res = {"device": torch.cuda.get_device_name(0), "K": K, "descriptors": N, "per_frame": n1, "rows": a.rows,
           "bounds": {"i8_mfma_mac_per_s": PEAK_I8_MAC, "hbm_bytes_per_s_spec": HBM_SPEC, "hbm_bytes_per_s_copy": HBM_COPY}}

    # ---- training ----
    desc = sift_like(torch, N, 1)
    cent = torch.empty((K, 128), dtype=torch.uint8, device="cuda")
    run = ctypes.c_int32(0)
    torch.cuda.synchronize()

    def train(stream, iters=a.iters):
        L.check(lib.slam_voc_train_dev(h, stream, _p(desc), N, K, iters, L.VOC_SIFT, _p(cent), ctypes.byref(run)), h)

    train(None, 1)                                          # warm-up
    ms = timed(torch, train, max(2, a.repeats // 2))
    it = int(run.value)
    res["train"] = {"total": dict(stat(ms), iterations=it, ms_per_iteration=round(min(ms) / it, 4))}
    word = torch.empty(N, dtype=torch.int32, device="cuda")
    dist = torch.empty(N, dtype=torch.int32, device="cuda")

    def assign_all(stream):
        L.check(lib.slam_voc_assign_dev(h, stream, _p(desc), N, _p(cent), K, L.VOC_SIFT, _p(word), _p(dist)), h)
    assign_all(None)
    ms = timed(torch, assign_all, a.repeats)
    mac = float(N) * K * 128
    res["train"]["assign_pass"] = dict(stat(ms), mac=mac, mac_per_s=mac / (min(ms) * 1e-3),
                                       share_of_i8_mfma_peak=round(mac / (min(ms) * 1e-3) / PEAK_I8_MAC, 4),
                                       bound="int8 MFMA rate")
    res["train"]["total"]["update_ms_per_iteration"] = round(res["train"]["total"]["ms_per_iteration"] - min(ms), 4)
    # the same update by u32 atomics (one thread per descriptor and 4 dimensions, then one per centroid
    # byte), measured by this script before that variant was removed: the same centroids
    res["train"]["update_by_u32_atomics_removed_variant"] = {"update_ms_per_iteration": 2.784, "ms_per_iteration": 4.1459}

    # ---- quantising one keyframe ----
    one = desc[:n1].contiguous()
    w1, d1 = word[:n1], dist[:n1]

    def assign_one(stream):
        L.check(lib.slam_voc_assign_dev(h, stream, _p(one), n1, _p(cent), K, L.VOC_SIFT, _p(w1), _p(d1)), h)
    assign_one(None)
    ms = timed(torch, assign_one, 4 * a.repeats)
    mac = float(n1) * K * 128
    q = {"sift_device": dict(stat(ms), mac=mac, mac_per_s=mac / (min(ms) * 1e-3),
                             share_of_i8_mfma_peak=round(mac / (min(ms) * 1e-3) / PEAK_I8_MAC, 5), bound="int8 MFMA rate")}
    one_h, cent_h = one.cpu().numpy(), cent.cpu().numpy()

    def wall(fn, repeats):
        fn()
        out = []
        for _ in range(repeats):
            t = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t) * 1e3)
        return out
    q["sift_host_buffers"] = dict(stat(wall(lambda: place.assign(one_h, cent_h, "sift", ctx=ctx), a.repeats)),
                                  what="slam_voc_assign, copies included, host clock")
    f_one, f_cent = one_h.astype(np.float32), cent_h.astype(np.float32)
    idx2 = None

    def knn_sift():
        nonlocal idx2
        idx2, _ = slamhip.knnMatch2(f_one, f_cent, slamhip.SIFT_BF, ctx=ctx)
    q["sift_knn2_top2_host_buffers"] = dict(stat(wall(knn_sift, a.repeats)),
                                            what="slam_knn2 over the same centroids (the parent's nearest equivalent), "
                                                 "copies included, host clock",
                                            launch=list(slamhip.lastKnnLaunch(ctx)))
    q["sift_knn2_same_words"] = bool(np.array_equal(idx2[:, 0], place.assign(one_h, cent_h, "sift", ctx=ctx)[0]))

    g = torch.Generator(device="cuda").manual_seed(3)
    orb = torch.randint(0, 256, (n1, 32), generator=g, device="cuda", dtype=torch.uint8)
    ocent = torch.randint(0, 256, (K, 32), generator=g, device="cuda", dtype=torch.uint8)
    torch.cuda.synchronize()

    def assign_orb(stream):
        L.check(lib.slam_voc_assign_dev(h, stream, _p(orb), n1, _p(ocent), K, L.VOC_ORB, _p(w1), _p(d1)), h)
    assign_orb(None)
    q["orb_device_popcount"] = stat(timed(torch, assign_orb, 4 * a.repeats))
    orb_h, ocent_h = orb.cpu().numpy(), ocent.cpu().numpy()
    q["orb_host_buffers"] = dict(stat(wall(lambda: place.assign(orb_h, ocent_h, "orb", ctx=ctx), a.repeats)),
                                 what="slam_voc_assign (popcount on the VALU), copies included, host clock")
    q["orb_knn2_top2_host_buffers"] = dict(stat(wall(lambda: slamhip.knnMatch2(orb_h, ocent_h, slamhip.ORB_BF, ctx=ctx),
                                                     a.repeats)),
                                           what="slam_knn2 (the +-1 int8 expansion on the matrix cores), copies included, "
                                                "host clock")
    res["quantise"] = q

    # ---- scoring ----
    m = a.rows
    g = torch.Generator(device="cuda").manual_seed(4)
    db = torch.zeros((m, K), dtype=torch.int32, device="cuda")
    cols = torch.randint(0, K, (m, 1500), generator=g, device="cuda")
    db.scatter_(1, cols, torch.randint(1, 300, (m, 1500), generator=g, device="cuda", dtype=torch.int32))
    tot = db.sum(dim=1, dtype=torch.int64)
    sc = {}
    for nq in (1, 8):
        out = torch.empty((nq, m), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def score(stream):
            L.check(lib.slam_bow_score_dev(h, stream, _p(db), _p(tot), nq, _p(db), _p(tot), m, K, _p(out)), h)
        score(None)
        ms = timed(torch, score, 4 * a.repeats)
        nbytes = float(m) * K * 4
        sc[f"queries_{nq}"] = dict(stat(ms), database_bytes=nbytes, bytes_per_s=nbytes / (min(ms) * 1e-3),
                                   share_of_hbm_spec=round(nbytes / (min(ms) * 1e-3) / HBM_SPEC, 4),
                                   share_of_hbm_copy=round(nbytes / (min(ms) * 1e-3) / HBM_COPY, 4), bound="HBM bandwidth")
    idx = torch.empty((1, 4), dtype=torch.int32, device="cuda")
    osc = torch.empty((1, 4), dtype=torch.float64, device="cuda")

    def topk(stream):
        L.check(lib.slam_bow_topk_dev(h, stream, _p(out), 1, m, 0, m, 4, _p(idx), _p(osc)), h)
    topk(None)
    sc["topk_4_of_rows"] = stat(timed(torch, topk, 4 * a.repeats))
    res["score"] = sc

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
