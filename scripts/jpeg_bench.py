#!/usr/bin/env python3
"""Times slam_jpeg_decode_batch_dev (csrc/jpeg.hip) on what one candidate search
consumes: 210 copies of each committed 1080p stream (tests/golden/jpeg:
quality 90, 4:2:0, without DRI and with a restart per MCU row) decoded into
resident BGR frames, one call per batch.

Per stream: wall ms per call and frames/s (median over the repeats, after a
warm-up call), the library's own split of the call (host parse + segment table,
staging + upload, jpeg_huff with the clearing of the coefficients, jpeg_idct,
jpeg_upcolor: HIP events, slam_jpeg_last_timing), the bytes moved, and jpeg_huff
at forced lanes-per-wave settings (SLAM_OPT_JPEG_LANES).  Baselines in the same
run on the same host: slam_jpeg_decode_host and PIL (where it imports) over the
same 210 streams on 16 threads.  Frame 0 and frame n - 1 of every decode are
checked against the committed SHA-256 of PIL's decode.

    python scripts/jpeg_bench.py --out profiles/jpeg_bench.json

Needs a HIP device; there is no fallback.
"""
import argparse
import hashlib
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-indoor-code_amd"))

import slamhip                      # noqa: E402
from slamhip import _lib as L       # noqa: E402

DIR = os.path.join(ROOT, "tests", "golden", "jpeg")
STEP_MS = 15.1                      # the headline search step (README)
THREADS = 16


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def med(v):
    return float(np.median(v))


def host_baseline(fn, data, n, repeats):
    """n decodes of one stream on THREADS threads: wall ms per n"""
    out = []
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(fn, [data] * THREADS))
        for _ in range(repeats):
            t0 = time.perf_counter()
            list(pool.map(fn, [data] * n))
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=210)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--lanes", default="1,4,16,64", help="forced SLAM_OPT_JPEG_LANES settings timed besides auto")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    args = ap.parse_args()
    if slamhip.lib().slam_device_count() < 1:
        raise SystemExit("jpeg_bench needs a HIP device")
    import torch
    ctx = slamhip.Context(0)
    with open(os.path.join(DIR, "hashes.json")) as f:
        hashes = json.load(f)
    n = args.frames
    result = {"frames": n, "threads": THREADS, "step_ms": STEP_MS, "device": torch.cuda.get_device_name(0), "streams": {}}
    try:
        from PIL import Image
    except ImportError:
        Image = None

    def pil(data):
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))

    def host(data):
        return slamhip.imdecode(data, host=True, apply_orientation=False)

    for name in ("real_1080p_q90", "real_1080p_q90_drirow"):
        with open(os.path.join(DIR, name + ".jpg"), "rb") as f:
            data = f.read()
        info = slamhip.jpegInfo(data)
        out = torch.empty((n, info["height"], info["width"], 3), dtype=torch.uint8, device="cuda:0")
        bufs = [data] * n
        entry = {"stream_bytes": len(data), "segments_per_stream": info["segments"], "settings": {}}
        for lanes in [0] + [int(v) for v in args.lanes.split(",") if v]:
            ctx.set_option(L.OPT_JPEG_LANES, lanes)
            wall, split = [], []
            for r in range(args.repeats + 1):
                t0 = time.perf_counter()
                _, status, _ = slamhip.imdecode_batch(bufs, ctx=ctx, out=out)
                dt = (time.perf_counter() - t0) * 1e3
                assert not status.any()
                if r:                               # the first call grows the buffers
                    wall.append(dt)
                    split.append(slamhip.jpegLastTiming(ctx))
            assert sha(out[0].cpu().numpy()) == hashes[name] and sha(out[n - 1].cpu().numpy()) == hashes[name]
            s = {k: med([t[0][k] for t in split]) for k in split[0][0]}
            s["wall_ms"] = med(wall)
            s["frames_per_s"] = n / s["wall_ms"] * 1e3
            s["device_ms"] = s["upload_ms"] + s["huff_ms"] + s["idct_ms"] + s["upcolor_ms"]
            s["huff_share_of_device"] = s["huff_ms"] / s["device_ms"]
            s["fits_beside_step"] = bool(s["wall_ms"] <= STEP_MS)
            entry["settings"]["auto" if lanes == 0 else f"lanes{lanes}"] = s
            entry["bytes"] = split[-1][1]
        ctx.set_option(L.OPT_JPEG_LANES, 0)
        hb = host_baseline(host, data, n, args.host_repeats)
        entry["host_decode_16_threads"] = {"ms": med(hb), "frames_per_s": n / med(hb) * 1e3}
        if Image is not None:
            pb = host_baseline(pil, data, n, args.host_repeats)
            entry["pil_16_threads"] = {"ms": med(pb), "frames_per_s": n / med(pb) * 1e3}
        result["streams"][name] = entry
        del out
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
