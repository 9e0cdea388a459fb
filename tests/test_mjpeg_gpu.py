"""Motion-JPEG on the device: the chunk-parallel entropy decoder (jpeg.hip's jpeg_sync,
jpeg_sync_count, jpeg_sync_scan, jpeg_sync_write) against the committed expectations
and against the host driver that runs the same shared functions in the same round
structure (tests/test_mjpeg.py checks that driver against the serial decoder), the
fall-back on corrupt streams, VideoCapture.read_batch, and the pipeline over
VideoMedia."""
import glob
import hashlib
import json
import os

import numpy as np
import pytest

import slamhip
from slamhip import _lib as L
from slamhip import cycle, video

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "mjpeg")
OLD = os.path.join(ROOT, "tests", "golden", "jpeg")
NEW_CLEAN = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "m96x80_*.jpg")))
with open(os.path.join(OLD, "hashes.json")) as _f:
    HASHES = json.load(_f)
OLD_SMALL = sorted(n for n in HASHES if not n.startswith("real_"))
CORRUPT = [(OLD, os.path.basename(p)[:-4]) for p in sorted(glob.glob(os.path.join(OLD, "bad_*.jpg")))] + \
          [(DIR, "bad_cut"), (DIR, "bad_mid_flip")]
INT_STATS = ("parallel_segments", "fallback_segments", "chunk_bytes", "lanes", "chunks", "wg_rounds_max",
             "launch_rounds_max", "wg_rounds_total", "launch_rounds_total")


def stream(d, name):
    with open(os.path.join(d, name + ".jpg"), "rb") as f:
        return f.read()


def strip_dht(data):
    out, pos = bytearray(data[:2]), 2
    while data[pos + 1] != 0xDA:
        n = 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
        if data[pos + 1] != 0xC4:
            out += data[pos:pos + n]
        pos += n
    return bytes(out + data[pos:])


def batch(datas, ctx, sync, chunk=0, **kw):
    ctx.set_option(L.OPT_JPEG_SYNC, sync)
    ctx.set_option(L.OPT_JPEG_CHUNK, chunk)
    try:
        frames, status, _ = slamhip.imdecode_batch(datas, ctx=ctx, **kw)
        stats = slamhip.jpegLastSync(ctx)
    finally:
        ctx.set_option(L.OPT_JPEG_SYNC, 0)
        ctx.set_option(L.OPT_JPEG_CHUNK, 0)
    return frames.cpu().numpy(), status, stats


def host_stats(datas, chunk):
    """the host driver's statistics of a batch: sums, and maxima of the maxima"""
    tot = dict.fromkeys(INT_STATS, 0)
    for data in datas:
        s = slamhip.imdecode_host_sync(data, chunk)[2]
        for k in INT_STATS:
            tot[k] = max(tot[k], s[k]) if k.endswith("_max") or k in ("chunk_bytes", "lanes") else tot[k] + s[k]
    return tot


def by_size(names_dirs):
    groups = {}
    for d, n in names_dirs:
        i = slamhip.jpegInfo(stream(d, n))
        groups.setdefault((i["width"], i["height"]), []).append((d, n))
    return list(groups.values())


@pytest.mark.parametrize("chunk", [16, 64, 256])
def test_device_equals_expected_and_the_host_driver(gpu_ctx, chunk):
    """every clean stream but the two 1080p ones, one size per batch, every segment of more than one chunk parallel"""
    groups = by_size([(DIR, n) for n in NEW_CLEAN] + [(OLD, n) for n in OLD_SMALL])
    assert len(groups) >= 5
    ran = 0
    for g in groups:
        datas = [stream(d, n) for d, n in g]
        frames, status, stats = batch(datas, gpu_ctx, 2, chunk)
        assert not status.any(), [n for _, n in g]
        for f, (d, n) in zip(frames, g):
            np.testing.assert_array_equal(f, np.load(os.path.join(d, n + ".npy")), err_msg=n)
        want = host_stats(datas, chunk)
        assert {k: stats[k] for k in INT_STATS} == want, [n for _, n in g]
        assert stats["fallback_segments"] == 0, [n for _, n in g]
        ran += stats["parallel_segments"]
        if g[0][0] == DIR:
            assert stats["parallel_segments"] == len(NEW_CLEAN)
    assert ran >= len(NEW_CLEAN) + 10


def test_more_workgroups_than_one_round_of_residency(gpu_ctx):
    """70 copies of the 19 KB stream at 16 bytes per chunk: 350 workgroups of 256 lanes with 11.4 KB of tables each"""
    data = stream(DIR, "m96x80_noise_444_q95")
    frames, status, stats = batch([data] * 70, gpu_ctx, 2, 16)
    assert not status.any()
    assert (frames == np.load(os.path.join(DIR, "m96x80_noise_444_q95.npy"))[None]).all()
    one = host_stats([data], 16)
    assert stats["parallel_segments"] == 70 and stats["fallback_segments"] == 0
    assert stats["chunks"] == 70 * one["chunks"] and stats["wg_rounds_total"] == 70 * one["wg_rounds_total"]
    assert stats["wg_rounds_max"] == one["wg_rounds_max"] and stats["launch_rounds_max"] == one["launch_rounds_max"] >= 2


@pytest.mark.parametrize("sync", [1, 2])
def test_mixed_batch_is_unchanged(gpu_ctx, sync):
    """restart-per-row streams and restart-free streams of one size: the same frames as with the option off"""
    names = [n for n in OLD_SMALL if n.split("_")[0] in ("s48x50", "n48x50")]
    assert any("drirow" in n for n in names) and any("dri" not in n for n in names)
    datas = [stream(OLD, n) for n in names]
    base, st0, s0 = batch(datas, gpu_ctx, 0)
    assert not st0.any() and s0["parallel_segments"] == 0 and s0["chunks"] == 0
    got, st, stats = batch(datas, gpu_ctx, sync, 16)
    assert not st.any() and stats["fallback_segments"] == 0
    np.testing.assert_array_equal(got, base)
    if sync == 2:
        assert stats["parallel_segments"] >= len(names)      # restart intervals of more than 16 bytes take it too
    else:
        assert stats["parallel_segments"] == 0               # nothing here reaches the auto threshold


def test_corrupt_streams_equal_the_serial_decoder(gpu_ctx):
    """the eight committed corrupt streams: status and pixels are the host serial decoder's, the bytes around the
    frame are untouched, and the fall-back count is the host driver's"""
    import torch
    decoded = 0
    for d, name in CORRUPT:
        data = stream(d, name)
        try:
            want, wst = slamhip.imdecode_host(data)
        except L.SlamError:
            continue      # refused by the parser: never reaches a kernel (tests/test_jpeg_gpu.py)
        decoded += 1
        h, w = want.shape[:2]
        n, pad = h * w * 3, 4096
        for chunk in (16, 64):
            whole = torch.full((n + 2 * pad,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", gpu_ctx.device))
            out = whole[pad:pad + n].view(1, h, w, 3)
            _, status, stats = batch([data], gpu_ctx, 2, chunk, out=out)
            got = whole.cpu().numpy()
            assert status[0] == wst and wst != 0, name
            np.testing.assert_array_equal(got[pad:pad + n].reshape(h, w, 3), want, err_msg=name)
            assert (got[:pad] == 0xA5).all() and (got[pad + n:] == 0xA5).all(), name
            hs = host_stats([data], chunk)
            assert stats["fallback_segments"] == hs["fallback_segments"] and stats["parallel_segments"] == hs["parallel_segments"]
            if wst & 7:
                assert stats["fallback_segments"] >= 1
    assert decoded == 5


def test_1080p_takes_the_parallel_path(gpu_ctx):
    name = "real_1080p_q90"
    frames, status, stats = batch([stream(OLD, name)], gpu_ctx, 1)
    assert not status.any()
    assert hashlib.sha256(np.ascontiguousarray(frames[0]).tobytes()).hexdigest() == HASHES[name]
    assert stats["parallel_segments"] == 1 and stats["fallback_segments"] == 0 and stats["chunk_bytes"] == 256
    assert stats["chunks"] > 1000 and all(v >= 0 for v in stats["ms"].values()) and stats["ms"]["sync"] > 0


def test_parallel_keyword_turns_auto_on_for_one_call(gpu_ctx):
    names = ["m96x80_noise_444_q95", "m96x80_noise_444_q100", "m96x80_smooth_420_q75"]
    datas = [stream(DIR, n) for n in names]
    want = np.stack([np.load(os.path.join(DIR, n + ".npy")) for n in names])
    frames, status, _ = slamhip.imdecode_batch(datas, ctx=gpu_ctx, parallel=True)
    assert not status.any()
    np.testing.assert_array_equal(frames.cpu().numpy(), want)
    s = slamhip.jpegLastSync(gpu_ctx)
    assert s["parallel_segments"] == 2 and s["fallback_segments"] == 0      # the two streams above 16 KiB
    frames, status, _ = slamhip.imdecode_batch(datas, ctx=gpu_ctx)          # and off again afterwards
    assert slamhip.jpegLastSync(gpu_ctx)["parallel_segments"] == 0
    np.testing.assert_array_equal(frames.cpu().numpy(), want)
    ops = cycle.GpuOps(gpu_ctx)
    media = cycle.JpegMedia(datas, ops, chunk=3, parallel=True)
    got = media.take(3)
    assert slamhip.jpegLastSync(gpu_ctx)["parallel_segments"] == 2
    np.testing.assert_array_equal(np.stack([np.asarray(f) for f in got]), want)
    ops.close()
    for bad in ((L.OPT_JPEG_SYNC, 3), (L.OPT_JPEG_CHUNK, 48), (L.OPT_JPEG_CHUNK, 2048)):
        with pytest.raises(L.SlamError):
            gpu_ctx.set_option(*bad)


def _avi(tmp_path, streams, size, name="v.avi"):
    path = str(tmp_path / name)
    video.write_mjpeg_avi(path, streams, 25, size)
    return path


def test_read_batch_of_streams_without_dht(gpu_ctx, tmp_path):
    names = ["m96x80_noise_444_q95", "m96x80_smooth_420_q75", "m96x80_mixed_422_q90", "m96x80_gray_q85", "m96x80_noise_444_q100"]
    path = _avi(tmp_path, [strip_dht(stream(DIR, n)) for n in names], (96, 80))
    cap = slamhip.VideoCapture(path, ctx=gpu_ctx)
    assert cap.isOpened() and cap.get(video.CAP_PROP_FRAME_COUNT) == 5
    dev, status = cap.read_batch(3)
    assert tuple(dev.shape) == (3, 80, 96, 3) and not status.any()
    assert slamhip.jpegLastSync(gpu_ctx)["parallel_segments"] == 1      # the 19 KB frame is above the auto threshold
    rest, status2 = cap.read_batch(10)
    assert tuple(rest.shape) == (2, 80, 96, 3) and not status2.any() and cap.read_batch(1) == (None, None)
    got = np.concatenate([dev.cpu().numpy(), rest.cpu().numpy()])
    for f, n in zip(got, names):
        np.testing.assert_array_equal(f, np.load(os.path.join(DIR, n + ".npy")), err_msg=n)
    assert cap.set(video.CAP_PROP_POS_FRAMES, 1)
    ok, frame = cap.read()
    assert ok
    np.testing.assert_array_equal(frame, np.load(os.path.join(DIR, names[1] + ".npy")))
    cap.release()


def test_video_media_hands_out_jpeg_medias_frames_and_slam_main_writes_the_same_files(gpu_ctx, tmp_path):
    paths = sorted(glob.glob(os.path.join(OLD, "seq_*.jpg")))
    streams = [open(p, "rb").read() for p in paths]
    i = slamhip.jpegInfo(streams[0])
    avi = _avi(tmp_path, streams, (i["width"], i["height"]))
    ops = cycle.GpuOps(gpu_ctx)
    a, b = cycle.VideoMedia(avi, ops, chunk=3), cycle.JpegMedia(paths, ops, chunk=3)
    n = 0
    while True:
        fa, fb = a.take(2), b.take(2)
        assert len(fa) == len(fb)
        if not fa:
            break
        for x, y in zip(fa, fb):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
            np.testing.assert_array_equal(x.dev.cpu().numpy(), np.asarray(y))
            n += 1
    assert n == len(paths) and a.next_frame() is None
    ops.close()
    d = slamhip.reference_example()
    d.update({"featureExtractingThreshold": 10, "requiredExtractedPointsCount": 2000, "framesBatchSize": 2,
              "requiredMatchedPointsCount": 300, "useFM-SIFT-FLANN": True, "useFM-SIFT-BF": False,
              "useFM-ORB": False, "useBundleAdjustment": False, "BAMaxFramesCnt": 4})
    K = np.array([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]])
    files = {}
    for tag in ("video", "jpeg"):
        ops = cycle.GpuOps(gpu_ctx)
        cfg = dict(d)
        cfg.update({"usePhotosCycle": tag == "jpeg", "photosPathPattern": os.path.join(OLD, "seq_*.jpg"), "videoSourcePath": avi})
        media = cycle.media_from_config(slamhip.ConfigService(cfg), ops, chunk=3)
        assert isinstance(media, cycle.VideoMedia if tag == "video" else cycle.JpegMedia)
        out = tmp_path / tag
        gd, logs = cycle.slam_main(media, K.copy(), slamhip.ConfigService(d), ops, out_dir=str(out))
        ops.close()
        assert len(logs.pose_list) >= 3
        files[tag] = {f: open(os.path.join(out, f)).read() for f in ("points.txt", "poses.txt", "rotations.txt", "colors.txt")}
    assert files["video"]["poses.txt"] and files["video"] == files["jpeg"]
