#!/usr/bin/env python3
"""Times the Motion-JPEG reader (slamhip/video.py over csrc/avi_parse.cpp and
csrc/jpeg.hip) on what one candidate search consumes: 210 frames of 1080p per call,
the committed real_1080p_q90.jpg (quality 90, 4:2:0, no restart markers) wrapped 210
times into an AVI by write_mjpeg_avi.

Per setting: wall ms per call and frames/s (median over the repeats, after a warm-up
call), the library's split of the call (slam_jpeg_last_timing) and of the
chunk-parallel entropy decoder (slam_jpeg_last_sync: ms per kernel, chunks, rounds,
fall-backs).  Settings: SLAM_OPT_JPEG_SYNC off (one lane per frame: the parent's
decoder) against auto at 64 .. 1024 bytes per chunk; the same for batches of 1, 8
and 32 frames at the default chunk; the restart-per-row stream
(real_1080p_q90_drirow.jpg), which never takes the parallel path under auto, as the
unchanged control; cycle.VideoMedia end to end (open, index, decode 210 frames in
chunks of 32, fetch the host copies).  Baseline on the same host: PIL over the same
210 streams on 16 threads.  Frame 0 and the last frame of every decode are checked
against the committed SHA-256 of PIL's decode.

    python scripts/video_bench.py --out profiles/video_bench.json

Needs a HIP device; there is no fallback.
"""
import argparse
import hashlib
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-indoor-code_amd"))

import slamhip                      # noqa: E402
from slamhip import _lib as L       # noqa: E402
from slamhip import cycle, video    # noqa: E402

DIR = os.path.join(ROOT, "tests", "golden", "jpeg")
STEP_MS = 15.1                      # the headline search step (README)
THREADS = 16


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def med(v):
    return float(np.median(v))


def timed(cap, ctx, n, out, sync, chunk, repeats, want):
    ctx.set_option(L.OPT_JPEG_SYNC, sync)
    ctx.set_option(L.OPT_JPEG_CHUNK, chunk)
    wall, split, stats = [], [], []
    try:
        for r in range(repeats + 1):
            bufs = [cap.stream(i) for i in range(n)]
            t0 = time.perf_counter()
            _, status, _ = slamhip.imdecode_batch(bufs, ctx=ctx, out=out[:n], flags=L.JPEG_MJPEG)
            dt = (time.perf_counter() - t0) * 1e3
            assert not status.any()
            if r:
                wall.append(dt)
                split.append(slamhip.jpegLastTiming(ctx)[0])
                stats.append(slamhip.jpegLastSync(ctx))
    finally:
        ctx.set_option(L.OPT_JPEG_SYNC, 0)
        ctx.set_option(L.OPT_JPEG_CHUNK, 0)
    assert sha(out[0].cpu().numpy()) == want and sha(out[n - 1].cpu().numpy()) == want
    s = {k: med([t[k] for t in split]) for k in split[0]}
    s["wall_ms"] = med(wall)
    s["frames_per_s"] = n / s["wall_ms"] * 1e3
    s["fits_beside_step"] = bool(s["wall_ms"] <= STEP_MS)
    last = stats[-1]
    s["sync"] = {k: v for k, v in last.items() if k != "ms"}
    s["sync"]["ms"] = {k: med([t["ms"][k] for t in stats]) for k in last["ms"]}
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=210)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunks", default="64,128,256,512,1024")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_bench.json"))
    args = ap.parse_args()
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("video_bench needs a HIP device")
    import torch
    ctx = slamhip.Context(0)
    with open(os.path.join(DIR, "hashes.json")) as f:
        hashes = json.load(f)
    n = args.frames
    result = {"frames": n, "threads": THREADS, "step_ms": STEP_MS, "device": torch.cuda.get_device_name(0), "streams": {}}
    tmp = tempfile.mkdtemp()
    for name in ("real_1080p_q90", "real_1080p_q90_drirow"):
        with open(os.path.join(DIR, name + ".jpg"), "rb") as f:
            data = f.read()
        info = slamhip.jpegInfo(data)
        path = os.path.join(tmp, name + ".avi")
        t0 = time.perf_counter()
        nbytes = video.write_mjpeg_avi(path, [data] * n, 30, (info["width"], info["height"]))
        entry = {"stream_bytes": len(data), "avi_bytes": nbytes, "write_ms": (time.perf_counter() - t0) * 1e3, "settings": {}}
        t0 = time.perf_counter()
        cap = slamhip.VideoCapture(path, ctx=ctx)
        entry["open_and_index_ms"] = (time.perf_counter() - t0) * 1e3
        assert cap.isOpened() and cap.get(video.CAP_PROP_FRAME_COUNT) == n
        out = torch.empty((n, info["height"], info["width"], 3), dtype=torch.uint8, device="cuda:0")
        entry["settings"]["sync_off"] = timed(cap, ctx, n, out, 0, 0, args.repeats, hashes[name])
        if name.endswith("drirow"):
            entry["settings"]["sync_auto"] = timed(cap, ctx, n, out, 1, 0, args.repeats, hashes[name])
        else:
            for c in [int(v) for v in args.chunks.split(",") if v]:
                entry["settings"][f"sync_auto_chunk{c}"] = timed(cap, ctx, n, out, 1, c, args.repeats, hashes[name])
            for b in [int(v) for v in args.batches.split(",") if v]:
                entry["settings"][f"batch{b}_sync_off"] = timed(cap, ctx, b, out, 0, 0, args.repeats, hashes[name])
                entry["settings"][f"batch{b}_sync_auto"] = timed(cap, ctx, b, out, 1, 0, args.repeats, hashes[name])
            # end to end: what a pipeline pays per 210 frames, host copies included
            ops = cycle.GpuOps(ctx)
            e2e = []
            for _ in range(3):
                t0 = time.perf_counter()
                media = cycle.VideoMedia(path, ops, chunk=32)
                got = 0
                while True:
                    f = media.take(32)
                    if not f:
                        break
                    got += len(f)
                e2e.append((time.perf_counter() - t0) * 1e3)
                assert got == n
                media.cap.release()
            entry["video_media_end_to_end"] = {"ms": med(e2e[1:]), "frames_per_s": n / med(e2e[1:]) * 1e3, "chunk": 32}
            try:
                from PIL import Image
                with ThreadPoolExecutor(THREADS) as pool:
                    fn = lambda d: np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))      # noqa: E731
                    list(pool.map(fn, [data] * THREADS))
                    t = []
                    for _ in range(2):
                        t0 = time.perf_counter()
                        list(pool.map(fn, [data] * n))
                        t.append((time.perf_counter() - t0) * 1e3)
                entry["pil_16_threads"] = {"ms": med(t), "frames_per_s": n / med(t) * 1e3}
            except ImportError:
                pass
        cap.release()
        os.remove(path)
        result["streams"][name] = entry
        del out
    os.rmdir(tmp)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
