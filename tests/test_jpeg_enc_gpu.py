"""The device JPEG encoder (slam-indoor-code_amd/csrc/jpeg_enc.hip) against the host
encoder slam_jpeg_encode_host, byte for byte, on every committed case
(tests/golden/jpeg_enc; tests/test_jpeg_enc.py holds the host encoder to the numpy
contract and to PIL on the same cases); batches, the capacity rule with sentinels,
encode -> decode on the device, VideoWriter -> VideoCapture, and the scene's
fly-through written as one AVI."""
import ctypes
import json

import numpy as np
import pytest

import jpeg_ref
from jpeg_enc_cases import CASES, SAMPLINGS, SOURCES, source
import scene_ref as SR
import slamhip
from slamhip import _lib as L
from slamhip import api, cycle, scene

pytestmark = pytest.mark.gpu


def host(img, quality, sampling, restart=0, cap=None):
    return api.jpegEncode(img, quality, sampling, restart, host=True, cap=cap)


def test_device_equals_host_on_all_fixtures(gpu_ctx):
    for c in CASES:
        args = (source(c), c["quality"], SAMPLINGS[c["sampling"]], c["restart"])
        got = api.jpegEncode(*args, ctx=gpu_ctx)
        want = host(*args)
        assert got[1] == want[1] == c["size"] and got[2] == want[2] == 0, c
        assert got[0] == want[0], c


def test_batch_of_five_different_images(gpu_ctx):
    """one set of launches, five stream lengths"""
    rng = np.random.default_rng(11)
    fr = rng.integers(0, 256, (5, 48, 50, 3), dtype=np.uint8)
    fr[1] = 93
    fr[2] //= 8
    fr[3, :, :25] = 200
    fr[4] = SOURCES["n48x50"]
    for sampling, restart in ((0x22, 0), (0x21, 4), (0x11, 1), (0, 7)):
        out = api.imencode_batch(fr, 90, sampling, restart, ctx=gpu_ctx)
        want = [host(f, 90, sampling, restart)[0] for f in fr]
        assert out == want
        assert len({len(s) for s in out}) == 5
    gray = api.imencode_batch(fr[..., 1], 70, 0x22, 0, ctx=gpu_ctx)
    assert gray == [host(f, 70, 0, 0)[0] for f in fr[..., 1]]
    ms, nb = api.jpegEncLastTiming(gpu_ctx)
    assert len(ms) == 7 and nb["frame_bytes"] == 5 * 48 * 50


def test_overflow_with_sentinels(gpu_ctx):
    """capacity between the shortest and the longest stream of the batch: the images that overflow
    report their true size and write their first cap bytes, and nothing lands outside a slot"""
    import torch
    rng = np.random.default_rng(12)
    fr = rng.integers(0, 256, (4, 40, 25, 3), dtype=np.uint8)
    fr[1] = 7
    fr[2] //= 32
    want = [host(f, 95, 0x22, 3) for f in fr]
    sizes = sorted(w[1] for w in want)
    for cap in (sizes[1], sizes[3] - 1, 1, 629):
        pad = 64
        dev = torch.device("cuda", gpu_ctx.device)
        buf = torch.full((pad + 4 * cap + pad,), 0xA5, dtype=torch.uint8, device=dev)
        d_fr = torch.from_numpy(fr).to(dev)
        d_size = torch.zeros(4, dtype=torch.int64, device=dev)
        d_stat = torch.full((4,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rc = L.lib().slam_jpeg_encode_batch_dev(gpu_ctx.handle, None, ctypes.c_void_p(d_fr.data_ptr()), 4, 40, 25, 3, 75, 3000, 95,
                                                0x22, 3, ctypes.c_void_p(buf.data_ptr() + pad), cap,
                                                ctypes.c_void_p(d_size.data_ptr()), ctypes.c_void_p(d_stat.data_ptr()))
        assert rc == L.SLAM_OK
        out = buf.cpu().numpy()
        assert (out[:pad] == 0xA5).all() and (out[pad + 4 * cap:] == 0xA5).all()
        for i, (data, size, _) in enumerate(want):
            slot = out[pad + i * cap:pad + (i + 1) * cap]
            cap_i = cap if size > cap else 0
            hdata, hsize, hst = host(fr[i], 95, 0x22, 3, cap=cap)
            assert int(d_size[i]) == size == hsize and int(d_stat[i]) == hst == (L.JPEG_ENC_OVERFLOW if cap_i else 0)
            k = min(size, cap)
            assert slot[:k].tobytes() == data[:k] == hdata[:k]
            assert (slot[k:] == 0xA5).all()


def test_encode_then_decode_on_the_device(gpu_ctx):
    """restart interval 0 through the chunk-parallel decoder (SLAM_OPT_JPEG_SYNC = 2) and one MCU row
    through the serial one: the frames are jpeg_ref.decode's of the same bytes"""
    rng = np.random.default_rng(13)
    fr = rng.integers(0, 256, (3, 48, 50, 3), dtype=np.uint8)
    fr[1] = (fr[1] // 64) * 64
    yy, xx = np.mgrid[0:48, 0:50]
    fr[2] = np.stack([xx * 5, yy * 5, xx + yy], axis=2).astype(np.uint8)
    for restart, sync in ((0, 2), (4, 0)):
        streams = api.imencode_batch(fr, 90, 0x22, restart, ctx=gpu_ctx)
        gpu_ctx.set_option(L.OPT_JPEG_SYNC, sync)
        try:
            frames, status, _ = api.imdecode_batch(streams, ctx=gpu_ctx)
        finally:
            gpu_ctx.set_option(L.OPT_JPEG_SYNC, 0)
        assert (status == 0).all()
        got = frames.cpu().numpy()
        for i, s in enumerate(streams):
            np.testing.assert_array_equal(got[i], jpeg_ref.decode(s, 3))
        assert np.abs(got[2].astype(int) - fr[2]).mean() < 8        # and the smooth one is the picture that went in


def test_video_writer_round_trip(gpu_ctx, tmp_path):
    import torch
    rng = np.random.default_rng(14)
    fr = (rng.integers(0, 256, (6, 48, 50, 3)) // 16 * 16).astype(np.uint8)
    path = str(tmp_path / "six.avi")
    wr = slamhip.VideoWriter(path, "MJPG", 30, (50, 48), quality=92, restart_rows=1, ctx=gpu_ctx)
    wr.write_batch(torch.from_numpy(fr[:4]).to(torch.device("cuda", gpu_ctx.device)))
    wr.write_batch(fr[4:])
    streams = list(wr.streams)
    assert streams == [host(f, 92, 0x22, 4)[0] for f in fr]
    wr.release()
    cap = slamhip.VideoCapture(path, ctx=gpu_ctx)
    assert cap.isOpened() and cap.info["frames"] == 6 and (cap.info["width"], cap.info["height"]) == (50, 48)
    frames, status = cap.read_batch(6)
    assert (status == 0).all()
    got = frames.cpu().numpy()
    for i in range(6):
        np.testing.assert_array_equal(got[i], jpeg_ref.decode(streams[i], 3))
    cap.release()


def test_scene_fly_through_as_avi(tmp_path):
    """scene.main(render=("fly.avi", "wwad")): the AVI's decoded frames are the decode of imencode of
    scene.render's frames; a .jpg name goes through imwrite"""
    pts, cols = SR.clustered_cloud(3000, blobs=4)
    pts[:, 2] += 14.0      # in front of the reference viewer, which looks along +z from z = 7.9
    gd = cycle.GlobalData()
    gd.push_points(pts.astype(np.float64), cols)
    cfg = slamhip.reference_example()
    cfg.update(TriangleMaxDistance=0.25, TriangleEuclidDistanceWeight=1.0, TriangleColorDistance=0.02,
               TriangleMinimumPoints=6, onlyViz=True, outputDataDir=str(tmp_path))
    centre = pts.astype(np.float64).mean(0)
    gd.cameraRotations = [np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) for a in (0.0, 0.2, 0.4)]
    gd.spatialCameraPositions = [(centre + d).reshape(3, 1) for d in ([-0.3, 0.1, -0.2], [0.0, -0.1, -0.25], [0.3, 0.15, -0.2])]
    logs = cycle.Logs(str(tmp_path))
    for Rm, p in zip(gd.cameraRotations, gd.spatialCameraPositions):
        logs.pose(Rm, p)
    logs.close(gd)
    cfg_path = tmp_path / "config.json"
    cfg_path.write_text(json.dumps(cfg))
    scene.main(str(cfg_path), render=("fly.avi", "wwad"))
    loaded = scene.load_global_data(str(tmp_path))
    meshes = scene.mesh(scene.segment(loaded, slamhip.ConfigService(cfg)))
    views = scene.fly(scene.reference_view(loaded), "wwad")
    frames = scene.render(loaded, meshes, views=views)
    assert frames.shape == (4, 1000, 1000, 3) and len({f.tobytes() for f in frames}) > 1 and frames.max() > 0
    cap = slamhip.VideoCapture(str(tmp_path / "fly.avi"))
    assert cap.isOpened() and cap.info["frames"] == 4
    got, status = cap.read_batch(4)
    assert (status == 0).all()
    streams = [slamhip.imencode(".jpg", f)[1] for f in frames]
    assert [bytes(cap.stream(i)) for i in range(4)] == streams
    want, status, _ = api.imdecode_batch(streams)
    assert (status == 0).all() and bool((got == want).all())
    cap.release()
    scene.main(str(cfg_path), render="view.jpg")
    with open(tmp_path / "view.jpg", "rb") as f:
        assert f.read() == slamhip.imencode(".jpg", scene.render(loaded, meshes)[0])[1]
